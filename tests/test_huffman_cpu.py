"""Optimised Huffman tables (include/jpeg2png_amd.h: "Optimised Huffman tables"), checked without a GPU: the plain-Python
restatement in tests/huffman_cases.py against libjpeg itself with optimize_coding = TRUE (tests/c/write_coefficients_optimized.c
makes the calls of the command-line driver's write_jpeg() under -O on the same arrays), the C table builder of
jpeg2png_amd/csrc/j2p_huffman.h against the restatement's BITS and HUFFVAL through the stand-alone tests/c/huffman_main.c —
compiled plainly and once more with the address and undefined-behaviour sanitizers — and the properties the directed cases are
there for."""
import io
import os
import subprocess

import numpy as np
import pytest

import entropy_cases as ec
import huffman_cases as hc
from test_entropy_cpu import libjpeg_file
from test_jpeg_out_cli import _helper

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def write_optimized(tmp_path_factory):
    """tests/c/write_coefficients_optimized.c compiled against the same libjpeg as the driver"""
    return _helper(tmp_path_factory, "write_coefficients_optimized")


@pytest.fixture(scope="module")
def cases():
    out = dict(hc.sweep())
    out.update(hc.directed_cases())
    return out


@pytest.fixture(scope="module")
def reports(cases):
    """{name: (file, report)} of the restatement, computed once"""
    return {name: hc.encode_case(case) for name, case in cases.items()}


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def builder(request, tmp_path_factory):
    """callable: count vectors -> per vector ("refused", code) or (longest, BITS, HUFFVAL) as the C builder gives them"""
    exe = str(tmp_path_factory.mktemp("huffman") / "huffman")
    flags = (["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g"]
             if request.param == "sanitized" else ["-O2"])
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", *flags, "-I", os.path.join(ROOT, "jpeg2png_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "huffman_main.c"), "-o", exe], check=True)

    def run(vectors):
        text = "\n".join(" ".join(str(int(c)) for c in v) for v in vectors) + "\n"
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out = []
        for line in r.stdout.splitlines():
            words = line.split()
            if words[0] == "refused":
                out.append(("refused", int(words[1])))
                continue
            n = [int(x) for x in words]
            assert len(n) == 18 + n[1]
            out.append((n[0], n[2:18], n[18:]))
        assert len(out) == len(vectors)
        return out
    return run


def restated_table(count):
    try:
        bits, vals, longest = hc.table(count)
    except hc.Refused:
        return None
    return longest, bits, vals


def test_restatement_is_libjpeg_with_optimize_coding_byte_for_byte(write_optimized, cases, reports):
    assert len(cases) >= 178 + 6
    for name, case in cases.items():
        assert reports[name][0] == libjpeg_file(write_optimized, case), name


def test_c_builder_gives_the_restatements_tables_for_every_case(builder, cases, reports):
    vectors, want = [], []
    for name, (_file, report) in reports.items():
        for k in range(4 if len(cases[name]["coefficients"]) == 3 else 2):
            vectors.append(report["counts"][k])
            bits, vals, longest = report["tables"][k]
            want.append((longest, bits, vals))
    assert builder(vectors) == want


def random_counts():
    """200 count vectors: 1 to 256 symbols in use — uniform counts, a few distinct values (ties), counts that grow geometrically
    (deep trees: lengths above 16, and for ratios near 2 and 34 symbols or more a code above 32 bits, which is refused) and counts
    next to the limit"""
    rng = np.random.default_rng(2024)
    out = []
    for k in range(200):
        n = (1, 2, 3, 256, 255, 17, 162)[k] if k < 7 else int(rng.integers(1, 257))
        where = rng.permutation(256)[:n]
        v = np.zeros(256, dtype=np.int64)
        kind = k % 4
        if kind == 0:
            v[where] = rng.integers(1, 100000, size=n)
        elif kind == 1:
            v[where] = rng.integers(1, 4, size=n)
        elif kind == 2:
            ratio = float(rng.uniform(1.3, 2.1))
            v[where] = np.minimum(np.ceil(ratio ** np.arange(n)), hc.COUNT_LIMIT).astype(np.int64)
        else:
            v[where] = hc.COUNT_LIMIT - rng.integers(0, 3, size=n)
        out.append([int(x) for x in v])
    return out


def test_c_builder_gives_the_restatements_tables_for_random_counts(builder):
    vectors = random_counts()
    want = [restated_table(v) for v in vectors]
    got = builder(vectors)
    limited = refused = 0
    for k, (g, w) in enumerate(zip(got, want)):
        if w is None:
            assert g == ("refused", 2), k           # (every count is within the limit: only the tree's depth is left)
            refused += 1
        else:
            assert g == w, k
            limited += w[0] > 16
    assert limited >= 10 and 1 <= refused < 50, "the vectors no longer cover limiting, or the geometric quarter is all refused"


def test_a_count_above_the_limit_is_refused(builder):
    v = [0] * 256
    v[0x11] = hc.COUNT_LIMIT + 1
    at_limit = [0] * 256
    at_limit[0x11] = hc.COUNT_LIMIT
    got = builder([v, at_limit, [0] * 256])
    assert got[0] == ("refused", 1)
    assert got[1] == (1, [1] + [0] * 15, [0x11])
    assert got[2] == (0, [0] * 16, [])          # no symbol: the empty table
    with pytest.raises(hc.Refused):
        hc.table(v)


def test_case_preconditions(cases, reports):
    """what the directed cases are there for, by the restatement alone"""
    report = reports["limited"][1]
    assert report["tables"][1][2] > 16, "the tree of `limited` is no deeper than 16: nothing is limited"
    assert report["tables"][1][0] == [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 9]
    assert sum(hc.LIMITED_COUNTS) == 58072 and len(ec.scan_order(1928, 1928, 1, (1, 1))) == 241 * 241
    report = reports["single_symbol"][1]
    assert [(t[0], t[1]) for t in report["tables"]] == [([1] + [0] * 15, [0])] * 4
    report = reports["zrl_heavy"][1]
    assert report["counts"][1][0xf0] == 3 + 2 + 1 + 1 and report["counts"][1][0x00] == 3
    # 81 positions: five trips and one position of a sixth for the first wavefront (16 positions a trip), a second workgroup that
    # holds 17 of its 64
    assert len(ec.scan_order(72, 72, 1, (1, 1))) == 81
    assert sum(1 for s in ec.scan_order(41, 23, 3, (2, 2)) if s[1] is None) == 6
    assert reports["dummies_41x23_420"][1]["counts"][0][0] >= 6
    # ties: twenty symbols of one count, which only the order by value separates — and the order by value within a LENGTH, as
    # libjpeg 6b has it, is another file
    count = reports["ties"][1]["counts"][1]
    assert sorted(c for c in count if c) == [3] * 20 + [60]
    bits, vals, _ = reports["ties"][1]["tables"][1]
    assert vals == [0x00] + sorted(s for s in range(1, 256) if count[s])
    different = 0
    for name, (_file, report) in reports.items():
        for bits, vals, _longest in report["tables"]:
            by_length, k = [], 0
            for n in bits:
                by_length += sorted(vals[k:k + n])
                k += n
            different += by_length != vals
    assert different > 0


def test_no_file_is_larger_than_with_the_default_tables(cases, reports):
    for name, case in cases.items():
        plain = ec.encode(case["coefficients"], case["width"], case["height"], case["quant"], case["sub"])
        assert len(reports[name][0]) <= len(plain), name
        head = reports[name][0].index(b"\xff\xda")
        assert head <= plain.index(b"\xff\xda"), name


def test_pil_opens_the_files(reports):
    from PIL import Image
    opened = 0
    for name, case in hc.directed_cases().items():
        if "dense" in name or "last" in name or name in ("dc_swing", "run_lengths"):
            continue            # (valid files, but coefficients no decoder's range checks were written for)
        im = Image.open(io.BytesIO(reports[name][0]))
        im.load()
        assert im.size == (case["width"], case["height"]) and im.mode == ("L" if len(case["coefficients"]) == 1 else "RGB"), name
        opened += 1
    assert opened >= 12
