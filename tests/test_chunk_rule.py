"""The chunk rule of watched runs (j2p_internal.h: j2p_next_chunk), which compute() and the batch engine share: iterations
per device round trip are a sixth of those done so far, at most about 50 ms worth at the pace so far, at most 256, at
most what is left, and at least one while any are left.  Compiled from the header as C11 (which also shows that the
header's shared part is C) and compared with the rule restated here."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <stdio.h>
#include "j2p_internal.h"
int main(int argc, char **argv)
{
        for(int i = 1; i + 2 < argc; i += 3) {
                printf("%u\n", j2p_next_chunk((unsigned)strtoul(argv[i], NULL, 10), (unsigned)strtoul(argv[i + 1], NULL, 10), strtod(argv[i + 2], NULL)));
        }
        return 0;
}
"""


def rule(done, left, elapsed_ms):
    chunk = done // 6
    if done:
        per_it = elapsed_ms / done
        chunk = min(chunk, int(50.0 / per_it) if per_it > 0 else 256)
    return min(max(min(chunk, 256), 1), left)


def schedule(iterations, ms_per_iteration):
    """the (done, left, elapsed_ms) triples of a whole run at a constant pace"""
    triples, done = [], 0
    while done < iterations:
        triples.append((done, iterations - done, float(done * ms_per_iteration)))
        done += rule(*triples[-1])
    return triples


@pytest.fixture(scope="module")
def chunk_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("chunk")
    src, exe = str(d / "chunk.c"), str(d / "chunk")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "jpeg2png_amd", "csrc"), src, "-o", exe], check=True)
    return exe


def chunks(exe, triples):
    args = [repr(v) for t in triples for v in t]
    return [int(x) for x in subprocess.run([exe, *args], capture_output=True, text=True, check=True).stdout.split()]


def test_schedule_of_50_iterations_with_no_time_elapsed(chunk_program):
    triples = schedule(50, 0)
    want = [rule(*t) for t in triples]
    assert want[:12] == [1] * 12 and want[12] == 2 and sum(want) == 50          # a sixth of what is done
    assert chunks(chunk_program, triples) == want


def test_schedule_of_50_iterations_at_10_ms_each(chunk_program):
    triples = schedule(50, 10)
    want = [rule(*t) for t in triples]
    assert max(want) == 5 and sum(want) == 50                                   # 50 ms worth
    assert chunks(chunk_program, triples) == want


def test_caps_and_edges(chunk_program):
    triples = [(60, 3, 0.0), (60, 10, 0.0), (60, 11, 0.0),        # left smaller than, equal to, larger than the chunk of 10
               (0, 50, 0.0), (0, 50, 123.0), (0, 1, 0.0), (0, 0, 0.0), (5, 0, 1.0),   # done = 0; nothing left
               (6000, 10000, 0.0), (1536, 10000, 0.0), (1542, 10000, 0.0),     # the cap of 256
               (600, 1000, 600.0), (600, 1000, 60000.0), (600, 1000, 6.0)]     # 1 ms, 100 ms, 0.01 ms per iteration
    want = [rule(*t) for t in triples]
    assert want == [3, 10, 10, 1, 1, 1, 0, 0, 256, 256, 256, 50, 1, 100]
    assert chunks(chunk_program, triples) == want
