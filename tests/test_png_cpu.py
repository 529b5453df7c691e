"""The PNG file made on the GPU (include/jpeg2png_amd.h: "The PNG file"), checked without one: the plain-Python restatement in
tests/png_cases.py against zlib's inflate — the whole stream, and every block alone from its byte offset — and against PIL; the host C
of jpeg2png_amd/csrc/j2p_deflate.h (code lengths, codes, block headers and sizes, CRC-32, Adler-32 from block sums) against the
restatement through the stand-alone tests/c/deflate_main.c, compiled plainly and once more with the address and undefined-behaviour
sanitizers; and the properties the directed cases are there for."""
import io
import os
import subprocess
import zlib
from fractions import Fraction

import numpy as np
import pytest

import png_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return pc.directed_cases()


@pytest.fixture(scope="module")
def reports(cases):
    """{name: (file, report)} of the restatement, computed once"""
    return {name: pc.encode_case(case) for name, case in cases.items()}


def unfiltered(stream, height, row_bytes, bpp):
    """the samples a decoder gets back from a filtered stream (PNG's reconstruction, written on its own)"""
    rows, above = [], [0] * row_bytes
    for y in range(height):
        line = stream[y * (row_bytes + 1):(y + 1) * (row_bytes + 1)]
        f, row = line[0], []
        for x, v in enumerate(line[1:]):
            a = row[x - bpp] if x >= bpp else 0
            b = above[x]
            c = above[x - bpp] if x >= bpp else 0
            if f == 4:
                p = a + b - c
                pa, pb, pcc = abs(p - a), abs(p - b), abs(p - c)
                pred = a if pa <= pb and pa <= pcc else (b if pb <= pcc else c)
            else:
                pred = (0, a, b, (a + b) // 2)[f]
            row.append((v + pred) & 255)
        rows.append(row)
        above = row
    return np.array(rows, dtype=np.uint8)


def test_zlib_inflates_every_stream_to_the_filtered_bytes(cases, reports):
    assert len(cases) >= 17
    for name, case in cases.items():
        file, report = reports[name]
        data, kinds = pc.idat_data(file)
        assert kinds[0] == b"IHDR" and kinds[-1] == b"IEND" and set(kinds[1:-1]) == {b"IDAT"}, name
        assert data == report["zlib"] and zlib.decompress(data) == report["filtered"], name
        bpp = case["channels"] * case["bits"] // 8
        back = unfiltered(report["filtered"], case["height"], case["width"] * bpp, bpp)
        assert np.array_equal(back, case["samples"]), name
        idat = case["idat_bytes"] or pc.IDAT_BYTES_DEFAULT
        assert len(kinds) - 2 == -(-len(data) // idat), name


def test_every_block_inflates_alone_from_its_byte_offset(cases, reports):
    for name, case in cases.items():
        _file, report = reports[name]
        z, stream = report["zlib"], report["filtered"]
        size = case["block_bytes"] or pc.BLOCK_BYTES_DEFAULT
        assert report["blocks"][0]["offset"] == 2 and report["blocks"][-1]["offset"] + report["blocks"][-1]["bytes"] + 4 == len(z), name
        for b in report["blocks"]:
            at = b["stream_offset"]
            chunk = z[b["offset"]:b["offset"] + b["bytes"]]
            # with the bytes before it as dictionary, as an inflater in mid-stream has them — and with nothing at all: no match
            # reaches back across a block's first byte
            for inflater in (zlib.decompressobj(wbits=-15, zdict=stream[max(0, at - 32768):at]) if at else zlib.decompressobj(wbits=-15),
                             zlib.decompressobj(wbits=-15)):
                assert inflater.decompress(chunk) == stream[at:at + size], (name, at)


def test_pil_decodes_the_files_to_the_samples(cases, reports):
    from PIL import Image
    for name, case in cases.items():
        im = Image.open(io.BytesIO(reports[name][0]))
        im.load()
        assert im.size == (case["width"], case["height"]), name
        got = np.asarray(im)
        if case["bits"] == 8:
            assert im.mode == ("RGB" if case["channels"] == 3 else "L"), name
            assert np.array_equal(got.reshape(case["height"], -1), case["samples"]), name
        elif case["channels"] == 1:
            want = case["samples"].view(">u2").astype(np.uint16)
            assert np.array_equal(got.astype(np.uint16), want), name
        else:
            # (PIL keeps the high byte of 16-bit colour; the low bytes are held by the inflate test's reconstruction)
            assert np.array_equal(np.asarray(im.convert("RGB")).reshape(case["height"], -1), case["samples"][:, 0::2]), name


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def host(request, tmp_path_factory):
    """callable: the records of tests/c/deflate_main.c -> its output lines as lists of numbers"""
    exe = str(tmp_path_factory.mktemp("deflate") / "deflate")
    flags = (["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g"]
             if request.param == "sanitized" else ["-O2"])
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", *flags, "-I", os.path.join(ROOT, "jpeg2png_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "deflate_main.c"), "-o", exe], check=True)

    def run(records):
        text = "\n".join(" ".join(str(int(v)) for v in r) for r in records) + "\n"
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out = [[int(x) for x in line.split()] for line in r.stdout.splitlines()]
        assert len(out) == len(records)
        return out
    return run


def restated_block(count, final):
    """what deflate_main prints for a block, from the restatement's own functions"""
    lengths, longest = pc.code_lengths(count, 15)
    codes = pc.canonical_codes(lengths)
    matches, literals = sum(count[257:]), sum(count[:256])
    hlit = max(lengths) + 1 - 257
    seq = [lengths.get(s, 0) for s in range(257 + hlit)] + [1 if matches else 0]
    syms = pc.length_sequence(seq)
    cl_count = [0] * 19
    for s, _, _ in syms:
        cl_count[s] += 1
    cl_lengths, _ = pc.code_lengths(cl_count, 7)
    cl_codes = pc.canonical_codes(cl_lengths)
    hclen = max(max(k for k, s in enumerate(pc.CL_ORDER) if s in cl_lengths) + 1 - 4, 0)
    w = pc.BitWriter()
    for v, n in ((1 if final else 0, 1), (2, 2), (hlit, 5), (0, 5), (hclen, 4)):
        w.value(v, n)
    for s in pc.CL_ORDER[:hclen + 4]:
        w.value(cl_lengths.get(s, 0), 3)
    for s, nbits, extra in syms:
        w.code(cl_codes[s])
        w.value(extra, nbits)
    header_bits = len(w.bits)
    w.pad()
    bits = header_bits + sum(count[s] * lengths[s] for s in lengths)
    bits += sum(count[257 + k] * (pc.LENGTH_EXTRA[k] + 1) for k in range(29))
    size = (bits + 7) // 8 if final else (bits + 3 + 7) // 8 + 4
    table = []
    for s in range(286):
        if s in codes:
            c, n = codes[s]
            table.append((n << 16) | int(format(c, "0%db" % n)[::-1], 2))
        else:
            table.append(0)
    return ([longest, hlit, hclen, 1 if matches else 0, header_bits, size, literals, matches] + [lengths.get(s, 0) for s in range(286)] +
            [cl_lengths.get(s, 0) for s in range(19)] + table + list(w.bytes()))


def test_host_c_makes_the_restatements_blocks_for_every_case(host, cases, reports):
    records, want = [], []
    for name, (_file, report) in reports.items():
        for k, b in enumerate(report["blocks"]):
            final = k == len(report["blocks"]) - 1
            records.append([0, int(final)] + b["count"])
            line = restated_block(b["count"], final)
            # the restatement's own report of the block it wrote says the same
            assert line[:6] == [b["longest"], b["hlit"], b["hclen"], b["dist_length"], b["header_bits"], b["bytes"]], name
            assert line[8:8 + 286] == b["lengths"] and bytes(line[8 + 286 + 19 + 286:]) == b["header"], name
            want.append(line)
    got = host(records)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, k


def random_counts():
    """120 count vectors: a few symbols to all 286 in use — uniform counts, a few distinct values (ties), counts that grow
    geometrically (trees deeper than 15) and blocks of the largest size"""
    rng = np.random.default_rng(77)
    out = []
    for k in range(120):
        n = (2, 3, 286, 285, 40)[k] if k < 5 else int(rng.integers(2, 287))
        where = rng.permutation(286)[:n]
        v = np.zeros(286, dtype=np.int64)
        kind = k % 4
        if kind == 0:
            v[where] = rng.integers(1, 5000, size=n)
        elif kind == 1:
            v[where] = rng.integers(1, 4, size=n)
        elif kind == 2:
            v[where] = np.minimum(np.ceil(float(rng.uniform(1.3, 2.1)) ** np.arange(n)), 1 << 24).astype(np.int64)
        else:
            v[where] = (1 << 24) // n - rng.integers(0, 3, size=n)
        v[256] = 1
        out.append([int(x) for x in v])
    return out


def test_host_c_makes_the_restatements_blocks_for_random_counts(host):
    vectors = random_counts()
    got = host([[0, k & 1] + v for k, v in enumerate(vectors)])
    limited = 0
    for k, (g, v) in enumerate(zip(got, vectors)):
        assert g == restated_block(v, bool(k & 1)), k
        limited += g[0] > 15
    assert limited >= 10, "the vectors no longer cover limiting"


def test_host_c_checksums(host, reports):
    rng = np.random.default_rng(5)
    records, want = [], []
    for n in (0, 1, 4, 255, 3000):
        data = rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
        records.append([1, n] + list(data))
        want.append([zlib.crc32(data)])
    for name in ("ff_300x300", "rgb_10x7", "fibonacci", "1x1"):
        stream, blocks = reports[name][1]["filtered"], reports[name][1]["blocks"]
        size = pc.directed_cases()[name]["block_bytes"] or pc.BLOCK_BYTES_DEFAULT
        record = [2, len(blocks)]
        for b in blocks:
            d = stream[b["stream_offset"]:b["stream_offset"] + size]
            record += [len(d), sum(d) % 65521, sum((len(d) - i) * v for i, v in enumerate(d)) % 65521]
        records.append(record)
        want.append([zlib.adler32(stream)])
        assert pc.adler32(stream) == zlib.adler32(stream), name
    # the largest block there is, all FF: the sums the device folds are at their largest
    n = 1 << 24
    records.append([2, 2, n, n * 255 % 65521, 255 * (n * (n + 1) // 2) % 65521, 5, 5 * 255 % 65521, 255 * 15 % 65521])
    want.append([zlib.adler32(b"\xff" * (n + 5))])
    assert host(records) == want


def kraft(lengths):
    return sum(Fraction(1, 1 << n) for n in lengths if n)


def test_every_table_is_complete(reports):
    tables = 0
    for name, (_file, report) in reports.items():
        for b in report["blocks"]:
            assert kraft(b["lengths"]) == 1 and max(b["lengths"]) <= 15, name
            assert kraft(b["cl_lengths"]) == 1 and max(b["cl_lengths"]) <= 7, name
            # the distance code: none, or its one symbol with one bit (RFC 1951 3.2.7: "one distance code of one bit")
            assert b["dist_length"] == (1 if b["matches"] else 0), name
            tables += 1
    assert tables > 1400
    for v in random_counts():
        lengths, _ = pc.code_lengths(v, 15)
        assert kraft(lengths.values()) == 1 and max(lengths.values()) <= 15


def test_a_flat_image_is_under_a_two_hundredth_of_its_samples():
    flat = np.full((512, 512 * 3), 90, dtype=np.uint8)
    file, report = pc.encode(flat, 512, 512)
    assert len(file) * 200 < flat.size
    assert zlib.decompress(pc.idat_data(file)[0]) == report["filtered"]


def test_case_preconditions(cases, reports):
    """what the directed cases are there for, by the restatement alone"""
    def blocks(name):
        return reports[name][1]["blocks"]

    def stats(name):
        return reports[name][1]["stats"]

    assert len(reports["rgb_10x7"][1]["filtered"]) == 7 * 31 and cases["rgb_10x7"]["block_bytes"] % 31 != 0
    assert len(reports["last_block_1"][1]["filtered"]) % cases["last_block_1"]["block_bytes"] == 1
    # two symbols: a literal and EOB, a bit each
    last = blocks("two_symbols")[-1]
    assert [c for c in last["count"] if c] == [3, 1] and sorted(n for n in last["lengths"] if n) == [1, 1] and last["dist_length"] == 0
    assert blocks("two_symbols")[0]["matches"] == 1
    assert all(blocks("all_256")[0]["count"][s] >= 1 for s in range(257)) and stats("all_256")["matches"] == 0
    fib = blocks("fibonacci")
    assert len(fib) == 1 and fib[0]["longest"] > 15 and max(fib[0]["lengths"]) == 15 and fib[0]["matches"] == 0
    assert sorted(c for c in fib[0]["count"] if c)[:6] == [1, 1, 2, 3, 5, 8] and 6500 < len(reports["fibonacci"][1]["filtered"]) < 7500
    # runs: the head a literal, then 2 -> two literals, 3 and 4 -> one match, 258 -> one, 259 -> a match and a literal,
    # 260 -> a match and two literals, 261 -> two matches (258 + 3), 517 -> three (258 + 258 + 1: two and a literal)
    assert pc.tokens(bytes([7] * 3)) == [("lit", 7)] * 3
    assert pc.tokens(bytes([7] * 4)) == [("lit", 7), ("match", 3)]
    assert pc.tokens(bytes([7] * 260)) == [("lit", 7), ("match", 258), ("lit", 7)]
    assert pc.tokens(bytes([7] * 262)) == [("lit", 7), ("match", 258), ("match", 3)]
    assert pc.tokens(bytes([7] * 518)) == [("lit", 7), ("match", 258), ("match", 258), ("lit", 7)]
    assert stats("runs")["matches"] == 0 + 1 + 1 + 1 + 1 + 1 + 2 + 2 and stats("runs")["literals"] == 1 + 8 + 2 + 1 + 2 + 1
    assert stats("run_across_blocks")["blocks"] == 4 and stats("run_across_blocks")["matches"] == 4
    end = reports["run_to_the_end"][1]["filtered"]
    assert end[-40:] == bytes([9]) * 40 and stats("run_to_the_end")["matches"] == 1
    # every filter wins a row, and row 0 is a tie that the lowest number wins
    assert all(n > 0 for n in stats("filters")["rows"]) and sum(stats("filters")["rows"]) == 12
    row0 = [int(v) for v in cases["filters"]["samples"][0]]
    assert pc.filtered_row(0, row0, [0] * 24, 1) == pc.filtered_row(2, row0, [0] * 24, 1) and reports["filters"][1]["filtered"][0] == 0
    assert stats("rgb16")["blocks"] > 1 and stats("grey16")["blocks"] > 1
    # Adler: 90300 bytes, 300 x 300 of them FF — sums far beyond 65521 in every block and across them
    assert stats("ff_300x300")["adler"] == zlib.adler32(reports["ff_300x300"][1]["filtered"])
    n = len(reports["idat_exact"][1]["zlib"])
    assert n % cases["idat_exact"]["idat_bytes"] == 0 and n % cases["idat_plus_1"]["idat_bytes"] == 1
    assert pc.idat_data(reports["idat_plus_1"][0])[1].count(b"IDAT") == n // cases["idat_plus_1"]["idat_bytes"] + 1
    for name, case in cases.items():
        if name not in ("all_256", "fibonacci", "runs") + pc.TILE_CASE_NAMES:
            assert 16 <= case["block_bytes"] <= 64 and 16 <= case["idat_bytes"] <= 64, name


def token_bits(token, lengths):
    """the bits a token takes under a block's code lengths: a literal's code; a match's length code, its extra bits and the distance's bit"""
    if token[0] == "lit":
        return lengths[token[1]]
    symbol, extra_bits, _extra = pc.length_symbol(token[1])
    return lengths[symbol] + extra_bits + 1


def test_tile_edge_case_preconditions(cases, reports):
    """what each case of png_cases.tile_cases() is there for, position by position, by the restatement alone: a later change of the
    cases cannot quietly miss the edge.  Positions are those of the block's bytes; a tile is 1024 of them."""
    T = pc.TILE
    assert set(pc.TILE_CASE_NAMES) <= set(cases)

    def block(name, k=0):
        """(block k's bytes, {position: token}, its report)"""
        size = cases[name]["block_bytes"]
        data = reports[name][1]["filtered"][k * size:(k + 1) * size]
        return data, pc.token_positions(data), reports[name][1]["blocks"][k]

    def breaking(data, lo, hi):
        """the positions lo..hi-1 whose byte does not equal the one before"""
        return [p for p in range(lo, min(hi, len(data))) if p == 0 or data[p] != data[p - 1]]

    for name in pc.TILE_CASE_NAMES:
        case = cases[name]
        assert (case["height"], case["channels"], case["bits"], case["filter"]) == (1, 1, 8, 0), name
        assert reports[name][1]["filtered"][0] == 0 and len(reports[name][1]["filtered"]) == case["width"] + 1, name
    data, at, _ = block("tiles_exact")
    assert len(data) == 4 * T == cases["tiles_exact"]["block_bytes"] and len(reports["tiles_exact"][1]["blocks"]) == 1
    data, at, _ = block("tiles_plus_1")
    assert len(data) == 4 * T + 1 == cases["tiles_plus_1"]["block_bytes"] and len(reports["tiles_plus_1"][1]["blocks"]) == 1
    v = data[4 * T]
    assert data[4 * T - 3] != v and [at.get(p) for p in range(4 * T - 2, 4 * T + 1)] == [("lit", v)] * 3      # the head, place 0, place 1
    data, at, _ = block("block_1025")
    assert len(data) == T + 1 and len(reports["block_1025"][1]["blocks"]) == 1

    data, at, _ = block("run_over_tiles")
    assert len(data) == 4 * T and len(reports["run_over_tiles"][1]["blocks"]) == 1
    assert breaking(data, 500, 3702) == [500, 3701] and not breaking(data, T, 2 * T) and not breaking(data, 2 * T, 3 * T)
    assert at[500][0] == "lit" and at[1017] == ("match", 258) and not any(p in at for p in range(1018, 1275)) and 1275 in at
    assert at[3597] == ("match", 3700 - 3597 + 1) and 3 * T <= 3597 and 3700 < 4 * T and at[3701][0] == "lit"
    # (nothing else matches: the noise has no two neighbours equal)
    assert reports["run_over_tiles"][1]["stats"]["matches"] == 13 and len(breaking(data, 0, 4 * T)) == 4 * T - 3200

    data, at, _ = block("match_at_tile_end")
    assert breaking(data, 248, 1402) == [248, 1401] and at[T - 1] == ("match", 258) and T - 1 + 257 < len(data)
    assert [p for p in at if 249 <= p <= T - 1] == [249, 507, 765, T - 1]
    data, at, _ = block("match_at_tile_start")
    assert breaking(data, 249, 1402) == [249, 1401] and at[T] == ("match", 258) and T - 1 not in at and data[T - 1] == data[T]
    assert [p for p in at if 250 <= p <= T] == [250, 508, 766, T]

    for k in (1, 2, 3):
        data, at, _ = block(f"tail_{k}")
        last = 248 + 3 * 258 + k
        assert breaking(data, 248, last + 2) == [248, last + 1] and last == T - 2 + k and at[765] == ("match", 258), k
    data, at, _ = block("tail_1")
    assert at[T - 1] == ("lit", data[248]) and at[T] == ("lit", data[T]) and data[T] != data[248]
    data, at, _ = block("tail_2")
    assert at[T - 1] == at[T] == ("lit", data[248]) and at[T + 1][0] == "lit" and data[T + 1] != data[248]
    data, at, _ = block("tail_3")
    assert at[T - 1] == ("match", 3) and T not in at and T + 1 not in at and at[T + 2][0] == "lit"

    assert reports["block_ends_in_ahead"][1]["filtered"] == reports["run_cut_at_tile"][1]["filtered"] == reports["match_at_tile_end"][1]["filtered"]
    data, at, _ = block("block_ends_in_ahead")
    assert len(data) == T + 100 and at[T - 1] == ("match", 101) and T - 1 + 101 == len(data) and len(reports["block_ends_in_ahead"][1]["blocks"]) == 2
    data, at, _ = block("run_cut_at_tile")
    assert len(data) == T and at[T - 1] == ("lit", data[248]) and data[T - 2] == data[T - 1] and T - 2 not in at      # place 0 with nothing behind it
    data, at, _ = block("run_cut_at_tile", 1)
    assert at[0] == ("lit", data[0]) and at[1] == ("match", 258) and data[0] == block("run_cut_at_tile")[0][T - 1]

    # the dense tile: 1023 literals of 15 bits and a match of 15 + 5 + 1 at the tile's last position — the bound of kPngWords
    data, at, b = block("dense_tile")
    assert len(reports["dense_tile"][1]["blocks"]) == 1 and len(data) == T - 1 + 200 + (1 << 18) - 1
    assert b["longest"] == 18 and max(b["lengths"]) == 15 and b["header_bits"] == 296
    assert all(at[p][0] == "lit" for p in range(T - 1)) and at[T - 1] == ("match", 200) and T + 199 in at and T + 198 not in at
    assert all(token_bits(at[p], b["lengths"]) == 15 for p in range(T - 1)) and token_bits(at[T - 1], b["lengths"]) == 21
    assert sum(token_bits(at[p], b["lengths"]) for p in range(T)) == pc.DENSE_TILE_BITS == 15366
    # ... which begin 24 bits into a word of the stream: the first and last word of the tile are both shared
    assert (b["offset"] * 8 + b["header_bits"]) % 32 >= 24
