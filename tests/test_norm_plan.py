"""The solver's norm plan — who reduces ||g|| between the two phase kernels of one iteration (j2p_solver.hip: norm_plan,
DESIGN.md section 4) — over the full cross product of its inputs, through the host-only hook j2p_debug_norm_plan.  The
expected values are the table of DESIGN.md written out; no GPU needed."""
import ctypes
import itertools
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# include/jpeg2png_amd.h: J2P_NORM_L1_* / J2P_NORM_L2_*
NONE, TICKETS, ROWSUMS = 0, 1, 2
GRADIENT, NORM_WHOLE, NORM_FINISH, PROJECT_WAVES, PROJECT_FIRST, EXTERNAL = 0, 1, 2, 3, 4, 5

ANY2 = (0, 1)
NIP = (0, 1, 2)
ROWS = (1, 1024, 1025)
IN_TREE = (1, 1024)          # tile rows one in-kernel tree takes
# (whole, fold, norm_in_project, band_nip, tile rows, split, log) -> (level 1, level 2, launches); a tuple = any of these
TABLE = [
    # whole canvas, folding off: k_norm_whole reads the strips' partials
    ((1,), (0,), NIP, ANY2, ROWS, ANY2, ANY2, (NONE, NORM_WHOLE, 3)),
    # whole canvas, folding on: level 2 inside k_project where asked for (whole phases, no logging, one tree's rows) ...
    ((1,), (1,), (1,), ANY2, IN_TREE, (0,), (0,), (TICKETS, PROJECT_WAVES, 2)),
    ((1,), (1,), (2,), ANY2, IN_TREE, (0,), (0,), (TICKETS, PROJECT_FIRST, 2)),
    # ... else behind the gradient launch's own tickets
    ((1,), (1,), (0,), ANY2, IN_TREE, (0,), ANY2, (TICKETS, GRADIENT, 2)),
    ((1,), (1,), (1, 2), ANY2, IN_TREE, (0,), (1,), (TICKETS, GRADIENT, 2)),
    # ... and by k_norm_finish when the gradient phase is split or the rows are too many for one tree
    ((1,), (1,), NIP, ANY2, ROWS, (1,), ANY2, (TICKETS, NORM_FINISH, 3)),
    ((1,), (1,), NIP, ANY2, (1025,), (0,), ANY2, (TICKETS, NORM_FINISH, 3)),
    # band, folding on: NIP 2 in whole phases of one tree's rows unless switched off, else k_norm_finish
    ((0,), (1,), NIP, (1,), IN_TREE, (0,), ANY2, (TICKETS, PROJECT_FIRST, 2)),
    ((0,), (1,), NIP, (0,), ROWS, ANY2, ANY2, (TICKETS, NORM_FINISH, 3)),
    ((0,), (1,), NIP, (1,), ROWS, (1,), ANY2, (TICKETS, NORM_FINISH, 3)),
    ((0,), (1,), NIP, (1,), (1025,), (0,), ANY2, (TICKETS, NORM_FINISH, 3)),
    # band, folding off: the same behind a k_rowsums launch
    ((0,), (0,), NIP, (1,), IN_TREE, (0,), ANY2, (ROWSUMS, PROJECT_FIRST, 3)),
    ((0,), (0,), NIP, (0,), ROWS, ANY2, ANY2, (ROWSUMS, NORM_FINISH, 4)),
    ((0,), (0,), NIP, (1,), ROWS, (1,), ANY2, (ROWSUMS, NORM_FINISH, 4)),
    ((0,), (0,), NIP, (1,), (1025,), (0,), ANY2, (ROWSUMS, NORM_FINISH, 4)),
]


def plan(lib, whole, fold, nip, band_nip, rows, split, log):
    l1, l2, n = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_uint(0)
    rc = lib.j2p_debug_norm_plan(whole, fold, nip, band_nip, rows, split, log, ctypes.byref(l1), ctypes.byref(l2), ctypes.byref(n))
    assert rc == 0
    return l1.value, l2.value, n.value


def test_norm_plan_is_the_table(lib):
    lib.j2p_debug_norm_plan.argtypes = [ctypes.c_int] * 4 + [ctypes.c_uint, ctypes.c_int, ctypes.c_int,
                                        ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint)]
    seen = 0
    for case in itertools.product(ANY2, ANY2, NIP, ANY2, ROWS, ANY2, ANY2):
        rows_of_table = [r for r in TABLE if all(v in allowed for v, allowed in zip(case, r[:7]))]
        assert len(rows_of_table) == 1, f"{case}: {len(rows_of_table)} rows of the table"
        want = rows_of_table[0][7]
        got = plan(lib, *case)
        assert got == want, f"(whole, fold, nip, band_nip, rows, split, log) = {case}: plan {got}, table {want}"
        # 2 + the plan's reduction launches; never the caller's
        assert got[2] == 2 + (got[0] == ROWSUMS) + (got[1] in (NORM_WHOLE, NORM_FINISH))
        assert got[1] != EXTERNAL
        seen += 1
    assert seen == 2 * 2 * 3 * 2 * 3 * 2 * 2


def test_the_tree_limit_on_both_sides(lib):
    lib.j2p_debug_norm_plan.argtypes = [ctypes.c_int] * 4 + [ctypes.c_uint, ctypes.c_int, ctypes.c_int,
                                        ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint)]
    # 1024 tile rows take the in-kernel tree, 1025 a k_norm_finish launch: every form of the tree
    assert plan(lib, 1, 1, 0, 1, 1024, 0, 0) == (TICKETS, GRADIENT, 2)
    assert plan(lib, 1, 1, 0, 1, 1025, 0, 0) == (TICKETS, NORM_FINISH, 3)
    assert plan(lib, 1, 1, 1, 1, 1024, 0, 0) == (TICKETS, PROJECT_WAVES, 2)
    assert plan(lib, 1, 1, 1, 1, 1025, 0, 0) == (TICKETS, NORM_FINISH, 3)
    assert plan(lib, 1, 1, 2, 1, 1024, 0, 0) == (TICKETS, PROJECT_FIRST, 2)
    assert plan(lib, 1, 1, 2, 1, 1025, 0, 0) == (TICKETS, NORM_FINISH, 3)
    assert plan(lib, 0, 1, 0, 1, 1024, 0, 0) == (TICKETS, PROJECT_FIRST, 2)
    assert plan(lib, 0, 1, 0, 1, 1025, 0, 0) == (TICKETS, NORM_FINISH, 3)
    assert plan(lib, 0, 0, 0, 1, 1024, 0, 0) == (ROWSUMS, PROJECT_FIRST, 3)
    assert plan(lib, 0, 0, 0, 1, 1025, 0, 0) == (ROWSUMS, NORM_FINISH, 4)
    # bad arguments are refused
    n = ctypes.c_uint()
    l1 = ctypes.c_int()
    assert lib.j2p_debug_norm_plan(1, 1, 3, 1, 16, 0, 0, ctypes.byref(l1), ctypes.byref(l1), ctypes.byref(n)) != 0
    assert lib.j2p_debug_norm_plan(1, 1, 0, 1, 0, 0, 0, ctypes.byref(l1), ctypes.byref(l1), ctypes.byref(n)) != 0
    assert lib.j2p_debug_norm_plan(1, 1, 0, 1, 16, 0, 0, None, ctypes.byref(l1), ctypes.byref(n)) != 0


def test_the_header_documents_the_values_the_test_uses():
    text = open(os.path.join(ROOT, "include", "jpeg2png_amd.h")).read()
    got = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define J2P_NORM_(L[12]_\w+) (\d+)", text, flags=re.M)}
    assert got == {"L1_NONE": NONE, "L1_TICKETS": TICKETS, "L1_ROWSUMS": ROWSUMS, "L2_GRADIENT": GRADIENT, "L2_NORM_WHOLE": NORM_WHOLE,
                   "L2_NORM_FINISH": NORM_FINISH, "L2_PROJECT_WAVES": PROJECT_WAVES, "L2_PROJECT_FIRST": PROJECT_FIRST, "L2_EXTERNAL": EXTERNAL}
