"""The inputs of tests/test_regrow_gpu.py — images and coefficients whose file is larger than the coders' first guess, so that the one
device block a coder works in has to grow in the middle of a call — and the coders' requests for that block restated from the sizes
of the restatements' files (tests/entropy_cases.py, tests/huffman_cases.py, tests/progressive_cases.py, tests/png_cases.py).  Nothing here
imports the library: tests/test_regrow_cpu.py holds the arithmetic, tests/test_regrow_gpu.py the library's count of the blocks it took
against it.

The block's layout is the one jpeg2png_amd/csrc/j2p_codec.hip documents above j2p_encode_scan, j2p_encode_progressive and j2p_png_write: parts aligned to 256
bytes; the parts whose size is not known yet are guessed in the earlier requests."""
import numpy as np

import entropy_cases as ec

PART = 256                              # every part of a block begins on a multiple of it
SCAN_TILE, STUFF_CHUNK = 1024, 256      # elements per workgroup of the scans; bytes of the stream per wavefront of the stuffing pass
HISTOGRAM_BYTES = 2 * 268 * 8           # the symbol counts, when they are taken (optimize, stats)
SCRATCH_STEP = 256 << 10                # a solver's scratch grows to a multiple of it
PNG_COUNTS_BYTES = 288 * 4              # per deflate block: its counts
PNG_BLOCK_RECORD = 8 + 8 + 286 * 4 + 520        # per deflate block: its place, code and header as the pack kernel reads them


def carve(*parts):
    return sum(-(-max(int(b), 1) // PART) * PART for b in parts)


def takes(requests, step=0):
    """how many blocks a call takes whose requests these are, from nothing: a request larger than the block held takes another one,
    of the request's size (step: rounded up to a multiple of it, as a solver's scratch is)"""
    held, n = 0, 0
    for r in requests:
        if held < r:
            held = -(-r // step) * step if step else r
            n += 1
    return n


# ---- JPEG ----
def heavy_case():
    """32x32 grey: every block DC 0 and all 63 AC coefficients 1023 — the longest codes and ten 1-bits behind each: FF bytes far
    beyond a sixteenth of the stream"""
    case = ec.make(32, 32, 1, (1, 1), "zero")
    case["coefficients"][0][:, :, 1:] = 1023
    return case


def sparse_case():
    return ec.make(32, 32, 1, (1, 1), "sparse", seed=32)


def scan_sizes(file):
    """(bytes of the entropy-coded data before stuffing, FF bytes stuffed) of a baseline file with one scan"""
    sos = file.index(b"\xff\xda")
    begin = sos + 2 + ((file[sos + 2] << 8) | file[sos + 3])
    assert file[-2:] == b"\xff\xd9"
    data = file[begin:-2]
    stuffed = data.count(b"\xff\x00")
    assert data.count(b"\xff") == stuffed
    return len(data) - stuffed, stuffed


def jpeg_requests(case, nbytes, stuffed, counting=False):
    """the three sizes j2p_encode_scan asks its block to have, for a file whose scan has nbytes bytes before stuffing (its bits:
    anything in the last byte gives the same words) and `stuffed` FF bytes; counting: the symbols are counted (optimize, stats)"""
    ncomp = len(case["coefficients"])
    grids = ec.grids(case["width"], case["height"], ncomp, case["sub"])
    nslots = len(ec.scan_order(case["width"], case["height"], ncomp, case["sub"]))
    coefficients = [gh * gw * 128 for gh, gw in grids]
    fixed = carve(*coefficients, nslots * 4, nslots * 8, (-(-nslots // SCAN_TILE) + 1) * 8, *([HISTOGRAM_BYTES] if counting else []))
    words = -(-nbytes * 8 // 32) + 1
    chunks = -(-nbytes // STUFF_CHUNK)
    out_at = fixed + carve(words * 4, chunks * 4, chunks * 8, (-(-chunks // SCAN_TILE) + 1) * 8)
    return [fixed + carve(*coefficients) // 4, out_at + nbytes + nbytes // 16 + 256, out_at + nbytes + stuffed]


def progressive_requests(case, report):
    """the three sizes j2p_encode_progressive asks its block to have, for a file whose scans `report` describes
    (progressive_cases.encode_report: per scan its bits before padding and its stuffed FF bytes).  A scan's items are its positions (DC)
    or its component's blocks (AC); the counts are 512 per scan and a flush counter each"""
    import progressive_cases as prc
    ncomp = len(case["coefficients"])
    grids = ec.grids(case["width"], case["height"], ncomp, case["sub"])
    nslots = len(ec.scan_order(case["width"], case["height"], ncomp, case["sub"]))
    scans = prc.SCANS[ncomp]
    assert len(report) == len(scans)
    items = [nslots if ss == 0 else grids[comps[0]][0] * grids[comps[0]][1] for comps, ss, _se, _ah, _al in scans]
    ac = [n for n, (_comps, ss, _se, _ah, _al) in zip(items, scans) if ss]
    coefficients = [gh * gw * 128 for gh, gw in grids]
    nitems = sum(items)
    fixed = carve(*coefficients, nitems * 4, nitems * 8, (-(-nitems // SCAN_TILE) + 1) * 8, *ac, *[4 * n for n in ac], len(scans) * 513 * 8)
    nbytes = [-(-r["bits"] // 8) for r in report]
    words = sum(-(-r["bits"] // 32) + 1 for r in report)
    chunks = sum(-(-n // STUFF_CHUNK) for n in nbytes)
    out_at = fixed + carve(words * 4, chunks * 4, chunks * 8, (-(-chunks // SCAN_TILE) + 1) * 8)
    data, stuffed = sum(nbytes), sum(r["stuffed"] for r in report)
    return [fixed + carve(*coefficients) // 4, out_at + data + data // 16 + 256, out_at + data + stuffed]


def noisy_planes(width, height, seed=304, density=0.6):
    """three 4:4:4 planes of quality-10 coefficients, `density` of them -2..2 at random: as a solver's iterate, requantised with steps
    of 1, a stream of several bits per coefficient"""
    from jpeg2png_amd import quality_tables, synth
    rng = np.random.default_rng(seed)
    tables = quality_tables(10, 3)
    shape = (height // 8, width // 8, 64)
    return [synth.Plane(width, height, 1, 1, np.where(rng.random(shape) < density, rng.integers(-2, 3, size=shape), 0).astype(np.int16).reshape(-1),
                        tables[c]) for c in range(3)]


# ---- PNG ----
def noise_image():
    """48x48 RGB noise: a zlib stream as long as the filtered rows, and with idat_bytes=16 three quarters as much again of chunk
    framing"""
    return np.random.default_rng(48).integers(0, 256, size=(48, 48, 3)).astype(np.uint8)


def png_requests(width, height, channels, bits, zlen, block_bytes=0, idat_bytes=0):
    """the two sizes j2p_png_write asks its block to have, for an image whose zlib stream has zlen bytes"""
    import png_cases as pc
    row = width * channels * bits // 8
    total = height * (row + 1)
    blocks = -(-total // (block_bytes or pc.BLOCK_BYTES_DEFAULT))
    chunks = -(-zlen // (idat_bytes or pc.IDAT_BYTES_DEFAULT))
    fixed = carve(height * row, total, 5 * 4, blocks * PNG_COUNTS_BYTES, blocks * PNG_BLOCK_RECORD)
    return [fixed + total // 2 + total // 4 + 4096, fixed + carve((-(-zlen // 4) + 1) * 4, zlen + 12 * chunks)]
