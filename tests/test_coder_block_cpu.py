"""The block a file coder works in (jpeg2png_amd/csrc/j2p_coder_block.h): what it queues again when the block moved is what was
queued, in the order it was queued — the rule whose loss writes a file from uninitialised memory.  tests/c/coder_block_main.cpp
includes nothing but that header and drives it with a host buffer for `memory`; it is compiled as C++17, plainly and once more
with the address and undefined-behaviour sanitizers (the buffer a move leaves behind is freed: a stage that kept the old base
writes into freed memory), and checks itself.  tests/test_regrow_gpu.py holds the coders that use the block to their files."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_a_block_that_moved_has_its_stages_queued_again_in_order(build, tmp_path):
    exe = str(tmp_path / "coder_block")
    # (the sanitizers' runtimes linked in: the program then runs whatever else the environment loads before it)
    flags = (["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g"]
             if build == "sanitized" else ["-O2"])
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", os.path.join(ROOT, "jpeg2png_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "coder_block_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "ok\n", r.stdout + r.stderr
