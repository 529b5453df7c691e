"""The geometry every layer shares (jpeg2png_amd/csrc/j2p_geometry.h): canvas and band alignment, the least band, near-equal
cuts, the gradient strip schedule and the per-channel row windows of a band.  tests/c/geometry_main.c includes nothing but
that header; it is compiled as C11, plainly and once more with the address and undefined-behaviour sanitizers, and what
it prints is compared with the rules restated here and with jpeg2png_amd.tiled, which keeps its own band_alignment and
split_rows for the runs that have no library."""
import itertools
import math
import os
import subprocess
from types import SimpleNamespace

import pytest

from jpeg2png_amd import tiled

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def geometry(request, tmp_path_factory):
    """callable: cases (strings) -> one list of ints per case, or the word the program printed"""
    exe = str(tmp_path_factory.mktemp("geometry") / "geometry")
    # (the sanitizers' runtimes linked in: the program then runs whatever else the environment loads before it)
    flags = (["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g"]
             if request.param == "sanitized" else ["-O2"])
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", *flags, "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "jpeg2png_amd", "csrc"), os.path.join(ROOT, "tests", "c", "geometry_main.c"), "-o", exe], check=True)

    def run(cases):
        out = []
        for k in range(0, len(cases), 500):          # (argument lists stay short)
            r = subprocess.run([exe, *cases[k:k + 500]], capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            out += [line if line == "refused" else [int(x) for x in line.split()] for line in r.stdout.splitlines()]
        assert len(out) == len(cases)
        return out
    return run


def ceil_div(a, b):
    return -(-a // b)


# ---- alignment ----
H_SAMP_SETS = [(1,), (1, 2, 2), (1, 1, 1), (2, 1), (3, 6, 6), (1, 4, 4), (3, 4)]


def test_alignment_is_the_least_common_multiple_in_either_channel_order(geometry):
    orders = [o for hs in H_SAMP_SETS for o in {hs, hs[::-1]}]
    got = geometry(["canvas " + " ".join(f"8 8 1 {h}" for h in o) for o in orders])
    for o, (W, H, align, min_band) in zip(orders, got):
        want = math.lcm(16, *[8 * h for h in o])
        assert align == want == tiled.band_alignment([SimpleNamespace(h_samp=h) for h in o]), o
        assert (W, H) == (8, 8 * max(o))
        assert min_band == ceil_div(48, want) * want                # three 16-row tile rows, rounded up to the alignment
    # neither factor divides the other: stepping in 16s until the channel at hand divides stops at 64, or at 48
    assert dict(zip(orders, (g[2] for g in got)))[(3, 4)] == dict(zip(orders, (g[2] for g in got)))[(4, 3)] == 96


def test_canvas_is_the_largest_plane_in_pixels(geometry):
    # 4:2:0 with padded chroma (tests/golden/rgb420_padded_40x20.npz): luma 40x24, chroma 24x16 at 2x2
    assert geometry(["canvas 40 24 1 1 24 16 2 2 24 16 2 2", "canvas 1920 1080 1 1", "canvas 8 8 4 1 16 8 1 3"]) == \
        [[48, 32, 16, 48], [1920, 1080, 16, 48], [32, 24, 48, 48]]


# ---- cuts ----
def test_cuts_of_ceil_units_are_split_rows(geometry):
    cases, want = [], []
    for H, align in itertools.product((16, 40, 96, 100, 416, 16384), (16, 32, 48)):
        units = ceil_div(H, align)
        for nband in range(1, min(units, 8) + 1):
            cases.append(f"cuts {units} {nband} {align}")
            want.append([b for b, _ in tiled.split_rows(H, nband, align)])
        cases.append(f"cuts {units} {units + 1} {align}")             # fewer units than bands
        want.append("refused")
        with pytest.raises(ValueError):
            tiled.split_rows(H, units + 1, align)
    assert geometry(cases) == want


def batch_cuts(hmin, nband, align):
    """run_job_tiled's rule (j2p_batch.hip): whole units of the shortest canvas; the remainder goes to the last band"""
    units = hmin // align
    cuts, start = [], 0
    for b in range(nband):
        cuts.append(start * align)
        start += units // nband + (1 if b < units % nband else 0)
    return cuts


def test_cuts_of_floor_units_are_the_batch_layers(geometry):
    cases, want = [], []
    for hmin, align in itertools.product((96, 100, 104, 416, 1080, 16384), (16, 32, 48)):
        for nband in range(2, min(hmin // (ceil_div(48, align) * align), 8) + 1):
            cases.append(f"cuts {hmin // align} {nband} {align}")
            want.append(batch_cuts(hmin, nband, align))
    assert len(cases) > 30 and geometry(cases) == want


# ---- the strip schedule ----
def schedule(W, H, band_rows, nch):
    """the strip schedule restated: [strips per row, rows per strip, zone shares d, b, c]"""
    strips = 1 if W <= 4 else ceil_div(W - 4, 124)
    rpw = 16
    if strips * nch * ceil_div(H, 16) < 2048:
        rpw = 8
        if strips * nch * ceil_div(H, 8) < 2048:
            rpw = 4
    launch_waves = strips * ceil_div(band_rows, rpw)
    d = b = c = 0
    if nch == 1 and rpw >= 8 and launch_waves < 3 * 4096:
        b, c = 32, (10 if rpw >= 16 else 0)
    elif nch == 1 and rpw >= 16:
        d, b, c = 200, 24, 8
    b = min(b, 256)
    c = min(c, 256 - b)
    d = min(d, 256 - b - c)
    return [strips, rpw, d, b, c]


def test_strip_schedule_over_the_grid(geometry):
    grid = [(W, H, rows, nch) for W in (8, 124, 128, 129, 512, 1920, 4096, 16384) for H in (8, 16, 100, 1080, 4096, 16384)
            for nch in (1, 3) for rows in ([H, 48] if H >= 48 else [H])]
    got = geometry(["schedule %u %u %u %u" % g for g in grid])
    for g, have in zip(grid, got):
        assert have == schedule(*g), g
    assert {tuple(h[1:]) for h in got} >= {(16, 0, 32, 10), (16, 200, 24, 8), (8, 0, 32, 0), (4, 0, 0, 0), (16, 0, 0, 0)}   # every branch


def test_strip_schedule_fixed_rows(geometry):
    rows = {                                    # nchannel, W, H, band rows -> strips, rpw, zone_d, zone_b, zone_c
        (1, 4096, 4096, 4096): [33, 16, 0, 32, 10],
        (1, 16384, 2048, 2048): [133, 16, 200, 24, 8],
        (1, 1920, 1080, 1080): [16, 8, 0, 32, 0],
        (3, 512, 512, 512): [5, 4, 0, 0, 0],
        (1, 4096, 4096, 1024): [33, 16, 0, 32, 10],
    }
    got = geometry([f"schedule {W} {H} {band} {nch}" for nch, W, H, band in rows])
    assert got == list(rows.values())


# ---- row windows ----
def window(ch, hs, H, row0, row1, band_local):
    """[covers, crow0, crows, frow0, frows] of a channel of ch coefficient rows at vertical sampling hs (halo: 2 rows)"""
    c0, c1 = min(row0 // hs, ch), min(ceil_div(row1, hs), ch)
    if band_local:
        return [1, c0, c1 - c0, c0, c1 - c0] if ch * hs >= H else [0]
    y0, y1 = max(row0 - 2, 0), min(row1 + 2, H)
    f0 = min(y0 // hs, ch - 1)
    f1 = max(min((y1 - 1) // hs + 1, ch), f0 + 1)
    return [1, c0, c1 - c0, f0, f1 - f0]


def check_windows(geometry, H, channels, bands):
    cases = [(ch, hs, H, r0, r1, local) for (r0, r1, local) in bands for (ch, hs) in channels]
    got = geometry(["window %u %u %u %u %u %u" % c for c in cases])
    for c, have in zip(cases, got):
        want = window(*c)
        assert have[:len(want)] == want, c
    return dict(zip(cases, got))


def test_row_windows_of_a_420_canvas(geometry):
    got = check_windows(geometry, 96, [(96, 1), (48, 2)], [(0, 96, 0), (0, 32, 0), (32, 64, 0), (64, 96, 0), (32, 64, 1)])
    assert got[(96, 1, 96, 32, 64, 0)] == [1, 32, 32, 30, 36] and got[(48, 2, 96, 32, 64, 0)] == [1, 16, 16, 15, 18]
    assert got[(48, 2, 96, 32, 64, 1)] == [1, 16, 16, 16, 16]


def test_row_windows_of_a_padded_chroma_canvas(geometry):
    # the canvas of rgb420_padded_40x20: 32 rows from the chroma (16 coefficient rows at 2), of which the luma (24 rows)
    # covers 24; the last band ends at H
    got = check_windows(geometry, 32, [(24, 1), (16, 2)], [(0, 32, 0), (0, 16, 0), (16, 32, 0), (16, 32, 1)])
    assert got[(24, 1, 32, 16, 32, 0)] == [1, 16, 8, 14, 10]
    assert got[(24, 1, 32, 16, 32, 1)][0] == 0 and got[(16, 2, 32, 16, 32, 1)] == [1, 8, 8, 8, 8]
