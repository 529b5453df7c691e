"""One buffer for the gradient and the prob state (jpeg2png_amd/csrc/j2p_geometry.h: j2p_shares_state, j2p_live_bytes_add,
j2p_nt_level): which channels share, and what a solver then counts as live for the non-temporal policy.  tests/c/share_main.c
includes nothing but that header; it is compiled as C11, plainly and once more with the address and undefined-behaviour
sanitizers, and what it prints is compared with the rules restated here."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALO = 2
CACHE = 260 << 20           # the policy's limit (j2p_solver.hip: kNtWorkingSet)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def share(request, tmp_path_factory):
    """callable: cases (strings) -> one list of ints per case"""
    exe = str(tmp_path_factory.mktemp("share") / "share")
    flags = (["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g"]
             if request.param == "sanitized" else ["-O2"])
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", *flags, "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "jpeg2png_amd", "csrc"), os.path.join(ROOT, "tests", "c", "share_main.c"), "-o", exe], check=True)

    def run(cases):
        r = subprocess.run([exe, *cases], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out = [[int(x) for x in line.split()] for line in r.stdout.splitlines()]
        assert len(out) == len(cases)
        return out
    return run


def shares(cw, ch, ws, hs, W, H, row0, row1, prob_on=1, wide=0):
    return f"shares {cw} {ch} {ws} {hs} {W} {H} {row0} {row1} {prob_on} {wide}"


def test_the_issues_table(share):
    cases = {
        shares(4096, 4096, 1, 1, 4096, 4096, 0, 4096): 1,          # 1x1 full-pitch plane
        shares(136, 40, 1, 1, 136, 40, 0, 40): 1,
        shares(4088, 4096, 1, 1, 4096, 4096, 0, 4096): 0,          # cw < W
        shares(2048, 4096, 2, 1, 4096, 4096, 0, 4096): 0,          # 2x1
        shares(4096, 2048, 1, 2, 4096, 4096, 0, 4096): 0,          # 1x2
        shares(2048, 2048, 2, 2, 4096, 4096, 0, 4096): 0,          # 2x2
        shares(4096, 4096, 1, 1, 4096, 4096, 0, 4096, prob_on=0): 0,
        shares(4096, 4096, 1, 1, 4096, 4096, 0, 4096, wide=1): 0,
        shares(16384, 16384, 1, 1, 16384, 16384, 2048, 4096): 1,   # a band: crow0 == row0
        shares(264, 40, 1, 1, 264, 40, 16, 40): 1,
    }
    got = share(list(cases))
    assert [g[0] for g in got] == list(cases.values())
    assert got[8][1:] == [2048, 2048] and got[9][1:] == [16, 24]


def test_a_full_pitch_plane_with_fewer_rows_than_the_canvas_shares_while_its_first_row_is_the_bands(share):
    # the luma of rgb420_padded_40x20: 48 x 24 coefficients on a 48 x 32 canvas.  Beyond its coverage no prob state is
    # written and none is used, so the plane shares, whole and as the band that still starts inside it; a band that starts
    # at or past the channel's last row has its window clipped to [ch, ch): first row ch, shared only if that IS the band's
    got = share([shares(48, 24, 1, 1, 48, 32, 0, 32), shares(48, 24, 1, 1, 48, 32, 16, 32), shares(48, 16, 1, 1, 48, 48, 32, 48),
                 shares(48, 16, 1, 1, 48, 48, 16, 32)])
    assert got == [[1, 0, 24], [1, 16, 8], [0, 16, 0], [1, 16, 0]]


def test_the_rule_over_a_grid(share):
    grid = [(cw, ws, hs, row0, prob, wide) for cw in (64, 128, 136) for ws in (1, 2, 3) for hs in (1, 2) for row0 in (0, 16, 32)
            for prob in (0, 1) for wide in (0, 1) if cw * ws <= 136 * 3]
    W, H = 136, 96
    cases, want = [], []
    for cw, ws, hs, row0, prob, wide in grid:
        ch = H // hs
        cases.append(shares(cw, ch, ws, hs, W, H, row0, H, prob, wide))
        crow0 = min(row0 // hs, ch)
        want.append(int(ws == 1 and hs == 1 and cw == W and crow0 == row0 and prob == 1 and wide == 0))
    got = [g[0] for g in share(cases)]
    assert got == want
    assert 0 < sum(got) < len(got)


def live(rows, W, channels, limit=CACHE):
    return f"live {rows} {W} {limit} " + " ".join("%u %u %u %u" % c for c in channels)


def restated(rows, W, channels):
    """[working_set, g, planes, d] of a solver of rows x W with channels (cw, crows, d_bytes, shared)"""
    planes = 2 * (rows + 2 * HALO) * W * 4 * len(channels)
    ws = g = d = 0
    for cw, crows, d_bytes, shared in channels:
        cells = max(crows, 1) * cw
        d += cells * d_bytes
        ws += rows * W * 4 + (0 if shared else cells * 4)
        g += 0 if shared else rows * W * 4
    return [ws + planes + d, g, planes, d]


@pytest.mark.parametrize("d_bytes", [1, 2])
def test_a_shared_one_channel_solver_keeps_13_bytes_per_pixel_and_d_an_unshared_one_17(share, d_bytes):
    for W, rows in ((4096, 4096), (4096, 3584), (264, 40), (16384, 2048)):
        px = rows * W
        halo = 2 * 2 * HALO * W * 4                # the halo rows of x_k and x_{k-1}: not pixels of the canvas
        (ws_s, g_s, planes_s, d_s, _), (ws_u, g_u, planes_u, d_u, _) = share([live(rows, W, [(W, rows, d_bytes, 1)]), live(rows, W, [(W, rows, d_bytes, 0)])])
        assert ws_s - halo == 12 * px + px * d_bytes                     # 13 B/px with byte coefficients
        assert ws_u - halo == 16 * px + px * d_bytes                     # 17 B/px with two buffers
        assert (g_s, g_u) == (0, 4 * px) and planes_s == planes_u == 8 * px + halo and d_s == d_u == px * d_bytes
        assert [ws_s, g_s, planes_s, d_s] == restated(rows, W, [(W, rows, d_bytes, 1)])
        assert [ws_u, g_u, planes_u, d_u] == restated(rows, W, [(W, rows, d_bytes, 0)])


def test_live_bytes_of_joint_images(share):
    # 4:4:4: all three share; 4:2:0: luma shares, the chroma planes keep two buffers and stay "g"
    c444 = [(136, 40, 1, 1)] * 3
    c420 = [(136, 40, 2, 1), (72, 24, 2, 0), (72, 24, 2, 0)]
    got = share([live(40, 136, c444), live(40, 136, c420), live(48, 144, c420)])
    assert [g[:4] for g in got] == [restated(40, 136, c444), restated(40, 136, c420), restated(48, 144, c420)]
    assert got[0][1] == 0 and got[1][1] == 2 * 40 * 136 * 4


def level(ws, g, planes, d, limit):
    if ws <= limit:
        return 0
    if ws - g <= limit:
        return 1
    return 2 if planes + d <= limit else 3


def test_policy_levels_and_a_fully_shared_solver_never_gets_level_one(share):
    shapes = [(4096, 3584), (4096, 4096), (4096, 4608), (4096, 5120), (8192, 4096), (16384, 2048), (8192, 8192)]
    cases = [(rows, W, shared) for (W, rows), shared in itertools.product(shapes, (0, 1))]
    got = share([live(rows, W, [(W, rows, 1, shared)]) for rows, W, shared in cases])
    levels = {}
    for (rows, W, shared), g in zip(cases, got):
        assert g[4] == level(*g[:4], CACHE), (rows, W, shared)
        levels[(W, rows, shared)] = g[4]
    assert all(lv != 1 for (_, _, shared), lv in levels.items() if shared)
    # the headline: two buffers push it past the cache (level 1: g hinted), one buffer fits whole
    assert (levels[(4096, 4096, 0)], levels[(4096, 4096, 1)]) == (1, 0)
    assert (levels[(4096, 3584, 0)], levels[(4096, 4608, 1)], levels[(4096, 5120, 1)]) == (0, 0, 2)
    assert levels[(16384, 2048, 1)] == levels[(16384, 2048, 0)] == 3


def test_which_solvers_fit_the_cache_with_one_buffer(share):
    """the solver's second condition (j2p_solver.hip: place): channels share only where one buffer makes the solver's own
    working set fit — level 0 with the coefficients counted as int16, as they are before their range is known"""
    shapes = {(1920, 1080): 0, (4096, 3584): 0, (4096, 4096): 0, (4096, 4608): 0, (4096, 5120): 2, (8192, 4096): 3, (16384, 2048): 3, (8192, 8192): 3}
    got = share([live(rows, W, [(W, rows, 2, 1)]) for W, rows in shapes])
    assert [g[4] for g in got] == list(shapes.values())
    joint = share([live(4096, 4096, [(4096, 4096, 2, 1)] * 3), live(40, 136, [(136, 40, 2, 1)] * 3)])
    assert [g[4] for g in joint] == [3, 0]
