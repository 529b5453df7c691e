"""Estimated tables without a GPU: the C rule (j2p_quant_estimate, jpeg2png_amd/csrc/j2p_quant_estimate.h) against its restatement
(tests/estimate_cases.py) on the corpus' histograms and on directed ones, and the rule against the truth — the tables of the files
the corpus was decoded from.  The histograms here are the restatement's; tests/test_estimate_gpu.py holds the kernel to them.

Determined entries, luma, per corpus file (the same for 4:4:4 and 4:2:0; the 200x120 counts are recorded, not gated):
  512x384: q50 15  q75 25  q85 44  q90 55  q95 62  q98 53
  200x120: q50 11  q75 21  q85 26  q90 37  q95 61  q98 52
Recompressed, quality 50 saved again at 95 (512x384 luma): 7 determined, all 7 equal the quality-50 table."""
import ctypes

import numpy as np
import pytest

import estimate_cases as es

LOW = (0, 1, 8)                         # luma entries (0,0), (0,1), (1,0) in natural order


def c_estimate(lib, hist, chroma):
    import jpeg2png_amd as j
    return j.estimate_quant_table(hist, chroma=chroma)


def same(a, b):
    return np.array_equal(a[0], b[0]) and a[0].dtype == b[0].dtype and np.array_equal(a[1], b[1]) and a[2] == b[2]


# ---- 1. C against the restatement ----

@pytest.mark.parametrize("name", sorted(es.directed_histograms()))
@pytest.mark.parametrize("chroma", (False, True), ids=("luma", "chroma"))
def test_c_rule_equals_the_restatement_on_directed_histograms(lib, name, chroma):
    hist = es.directed_histograms()[name]
    got, want = c_estimate(lib, hist, chroma), es.estimate(hist, chroma)
    assert same(got, want), (name, got, want)


def test_directed_histograms_say_what_they_were_built_for():
    d = es.directed_histograms()
    table, det, quality = es.estimate(d["all_zero"])
    assert not det.any() and quality == 100 and (table == 1).all()                     # ijg(100) is all ones
    assert not es.estimate(d["single_value"])[1].any()
    table, det, _ = es.estimate(d["values_only_at_q"])
    assert (table[0], det[0], table[9], det[9]) == (10, True, 37, True)                # 11 and 38 explain them too: the cost picks
    assert es.estimate(d["q4"])[0][0] == 4 and es.estimate(d["q4"])[1][0]
    assert [es.step_of(d[n][0])[0] for n in ("only_3", "q3", "q2", "q1", "clusters", "noisy_zeros")] == [4, 3, 2, 1, 0, 0]
    assert es.estimate(d["q255"])[0][0] == 255 and es.estimate(d["q255"])[1][0]
    assert es.step_of(d["outliers_at_allowance"][0]) == (20, 204)
    assert es.step_of(d["outliers_above_allowance"][0]) == (10, 205)
    assert es.step_of(d["nz_11"][0]) == (16, 11) and not es.estimate(d["nz_11"])[1][0]
    assert es.step_of(d["nz_12"][0]) == (16, 12) and es.estimate(d["nz_12"])[1][0]
    assert es.step_of(d["nz_15"][0]) == (16, 15) and es.step_of(d["nz_16"][0]) == (16, 16)
    table, det, quality = es.estimate(d["quality_50_chroma"], chroma=True)
    assert det.all() and quality == 50 and np.array_equal(table, es.ijg_table(50, True))
    table, det, _ = es.estimate(d["fill_lifted_by_mmax"])
    assert not det[63] and table[63] == 255                                           # 2 * (200 - 1) clamped


@pytest.fixture(scope="module")
def corpus(oracle):
    return es.corpus_channels()


def test_c_rule_equals_the_restatement_on_every_corpus_histogram(lib, corpus):
    assert len(corpus) == 12 * 3 + 6 * 1 + 6 * 3
    for ch in corpus:
        hist = ch.hist[0]
        assert same(c_estimate(lib, hist, ch.chroma), es.estimate(hist, ch.chroma)), ch.name


def test_estimate_refuses_null(lib):
    import jpeg2png_amd as j
    assert lib.j2p_quant_estimate(None, 0, ctypes.byref(j._CQuantEstimate())) == -1
    assert lib.j2p_quant_estimate(np.zeros((64, 1024), np.uint32).ctypes.data, 0, None) == -1
    with pytest.raises(j.J2PError):
        j.estimate_quant_table(np.zeros((64, 1000), np.uint32))


# ---- 2. the rule against the files' tables ----

def test_no_determined_entry_differs_from_the_files_table(corpus):
    counts = {}
    for ch in corpus:
        hist, blocks, excluded = ch.hist
        assert blocks > 0 and (hist.sum(axis=1) == blocks).all()
        table, det, quality = es.estimate(hist, ch.chroma)
        wrong = [(j, int(table[j]), int(ch.table[j])) for j in range(64) if det[j] and table[j] != ch.table[j]]
        assert not wrong, f"{ch.name}: (entry, estimated, the file's) {wrong}"
        counts[ch.name] = int(det.sum())
        print(f"{ch.name}: {blocks} blocks, {excluded} excluded, {counts[ch.name]} determined, quality {quality}")
    assert any("_own" in n for n in counts)


def test_the_large_files_determine_the_low_luma_entries_and_fifteen_in_all(corpus):
    seen = 0
    for ch in corpus:
        if not ch.name.startswith("512x384") or ch.chroma:
            continue
        seen += 1
        _, det, _ = es.estimate(ch.hist[0], False)
        assert all(det[j] for j in LOW), f"{ch.name}: entries (0,0), (0,1), (1,0) determined: {[bool(det[j]) for j in LOW]}"
        assert det.sum() >= 15, f"{ch.name}: {int(det.sum())} luma entries determined"
    assert seen == 12


def test_clipped_blocks_of_the_corpus_are_excluded(corpus):
    """the image's patches of 255 and 0 reach the luma of every file: without them the exclusion would go untested"""
    assert all(ch.hist[2] > 0 for ch in corpus if not ch.chroma)


def test_recompressed_file_is_measured_not_gated(oracle):
    """quality 50 saved again at 95: how many determined luma entries equal the quality-50 table (DESIGN.md records the figure)"""
    samples, first, second = es.recompressed()
    table, det, quality = es.estimate(es.histogram(samples)[0], False)
    print(f"recompressed 50 -> 95: {int(det.sum())} determined, {int((det & (table == first)).sum())} equal the first table, "
          f"{int((det & (table == second)).sum())} the second, quality {quality}")
    assert table.dtype == np.uint16 and table.min() >= 1 and table.max() <= 255
