"""The PNG file the GPU writes (include/jpeg2png_amd.h: "The PNG file"), restated in plain Python, and the directed cases the CPU
and GPU tests share.  Nothing here imports the library: the restatement is held against zlib's inflate and PIL by
tests/test_png_cpu.py, and the library against the restatement byte for byte by tests/test_png_gpu.py.

A case is a dict: samples (uint8 [height, row bytes], 16-bit samples big-endian), width, height, bits, channels, filter (None:
adaptive, or 0..4), block_bytes, idat_bytes (0: the default)."""
import struct
import zlib

import numpy as np

BLOCK_BYTES_DEFAULT = 65536
IDAT_BYTES_DEFAULT = 8192
SIZE_MIN, SIZE_MAX = 16, 1 << 24
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
# RFC 1951 3.2.5: length symbol 257 + k codes lengths LENGTH_BASE[k] .. with LENGTH_EXTRA[k] extra bits
LENGTH_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LENGTH_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
FILTER_NAMES = ("none", "sub", "up", "average", "paeth")


# ---- 2. filtering ----
def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    if pa <= pb and pa <= pc:
        return a
    return b if pb <= pc else c


def filtered_row(f, row, above, bpp):
    out = []
    for x, v in enumerate(row):
        a = row[x - bpp] if x >= bpp else 0
        b = above[x]
        c = above[x - bpp] if x >= bpp else 0
        pred = (0, a, b, (a + b) >> 1, _paeth(a, b, c))[f]
        out.append((v - pred) & 255)
    return out


def filter_stream(samples, bpp, filter=None):
    """-> (the filtered stream, rows per filter type)"""
    rows = [[int(v) for v in r] for r in samples]
    above = [0] * len(rows[0])
    out, chosen = bytearray(), [0] * 5
    for row in rows:
        if filter is None:
            best = None
            for f in range(5):
                fr = filtered_row(f, row, above, bpp)
                cost = sum(v if v < 128 else 256 - v for v in fr)
                if best is None or cost < best[0]:      # (strictly: the lowest number wins a tie)
                    best = (cost, f, fr)
            _, f, fr = best
        else:
            f, fr = filter, filtered_row(filter, row, above, bpp)
        chosen[f] += 1
        out.append(f)
        out += bytes(fr)
        above = row
    return bytes(out), chosen


# ---- 3. tokens ----
def tokens(block):
    """-> list of ("lit", byte) and ("match", length); every match has distance 1"""
    out, i, n = [], 0, len(block)
    while i < n:
        out.append(("lit", block[i]))           # the head of a stretch (or a lone byte)
        j = i + 1
        while j < n and block[j] == block[i]:
            j += 1
        left = j - i - 1                        # the same bytes behind it
        while left:
            piece = min(left, 258)
            out += [("match", piece)] if piece >= 3 else [("lit", block[i])] * piece
            left -= piece
        i = j
    return out


def token_positions(block):
    """{position in the block: its token} of tokens(block): a literal at its byte, a match at its first byte (the bytes behind it
    in the match — the silent ones — have no entry)"""
    out, at = {}, 0
    for token in tokens(block):
        out[at] = token
        at += 1 if token[0] == "lit" else token[1]
    assert at == len(block)
    return out


def length_symbol(n):
    """-> (symbol, extra bits, their value)"""
    k = max(i for i in range(29) if LENGTH_BASE[i] <= n)
    return 257 + k, LENGTH_EXTRA[k], n - LENGTH_BASE[k]


# ---- 4. coding ----
def code_lengths(count, limit):
    """{symbol: length} of the symbols with a non-zero count, and the longest length before limiting"""
    used = sorted((c, s) for s, c in enumerate(count) if c)
    if len(used) == 1:
        return {used[0][1]: 1}, 1
    # Huffman's algorithm with two queues: the leaves by count ascending and the nodes in the order they were made; the two
    # smallest heads are joined, a leaf before a node of the same weight
    weight = [c for c, _ in used]
    parent = [None] * (2 * len(used) - 1)
    leaf, node, made = 0, len(used), len(used)
    for _ in range(len(used) - 1):
        pick = []
        for _ in range(2):
            if leaf < len(used) and (node >= made or weight[leaf] <= weight[node]):
                pick.append(leaf)
                leaf += 1
            else:
                pick.append(node)
                node += 1
        weight.append(weight[pick[0]] + weight[pick[1]])
        parent[pick[0]] = parent[pick[1]] = made
        made += 1
    depth = [0] * len(parent)
    for k in range(len(parent) - 2, -1, -1):
        depth[k] = depth[parent[k]] + 1
    longest = max(depth[:len(used)])
    bits = [0] * (max(longest, limit) + 1)
    for d in depth[:len(used)]:
        bits[d] += 1
    for i in range(longest, limit, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    # dealt out by count descending, then symbol value ascending: the shortest first
    order = sorted(used, key=lambda cs: (-cs[0], cs[1]))
    lengths, k = {}, 0
    for n in range(1, limit + 1):
        for _ in range(bits[n]):
            lengths[order[k][1]] = n
            k += 1
    assert k == len(order)
    return lengths, longest


def canonical_codes(lengths):
    """RFC 1951 3.2.2: {symbol: (code, length)}, the code's first bit highest"""
    out, code, prev = {}, 0, 0
    for n, s in sorted((n, s) for s, n in lengths.items()):
        code <<= n - prev
        out[s] = (code, n)
        code += 1
        prev = n
    return out


class BitWriter:
    """deflate's order: bits fill a byte from its lowest bit up; Huffman codes go first bit first, everything else lowest first"""

    def __init__(self):
        self.bits = []

    def value(self, v, n):
        self.bits += [(v >> k) & 1 for k in range(n)]

    def code(self, c):
        self.bits += [(c[0] >> k) & 1 for k in range(c[1] - 1, -1, -1)]

    def pad(self):
        self.bits += [0] * (-len(self.bits) % 8)

    def bytes(self):
        assert len(self.bits) % 8 == 0
        return bytes(sum(b << k for k, b in enumerate(self.bits[i:i + 8])) for i in range(0, len(self.bits), 8))


def length_sequence(seq):
    """the code lengths of a block's header as symbols of the code-length code: [(symbol, extra bits, their value)]"""
    out, i = [], 0
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        n = j - i
        if v == 0:
            while n >= 11:
                r = min(n, 138)
                out.append((18, 7, r - 11))
                n -= r
            if n >= 3:
                out.append((17, 3, n - 3))
                n = 0
        else:
            out.append((v, 0, 0))
            n -= 1
            while n >= 3:
                r = min(n, 6)
                out.append((16, 2, r - 3))
                n -= r
        out += [(v, 0, 0)] * n
        i = j
    return out


def deflate_block(block, final):
    """-> (the block's bytes, its report)"""
    toks = tokens(block)
    count = [0] * 286
    for kind, v in toks:
        count[v if kind == "lit" else length_symbol(v)[0]] += 1
    count[256] = 1
    matches = sum(1 for kind, _ in toks if kind == "match")
    lengths, longest = code_lengths(count, 15)
    codes = canonical_codes(lengths)
    hlit = max(lengths) + 1 - 257
    dist_length = 1 if matches else 0
    seq = [lengths.get(s, 0) for s in range(257 + hlit)] + [dist_length]
    cl_syms = length_sequence(seq)
    cl_count = [0] * 19
    for s, _, _ in cl_syms:
        cl_count[s] += 1
    cl_lengths, _ = code_lengths(cl_count, 7)
    cl_codes = canonical_codes(cl_lengths)
    hclen = max(k for k, s in enumerate(CL_ORDER) if s in cl_lengths) + 1 - 4
    hclen = max(hclen, 0)
    w = BitWriter()
    w.value(1 if final else 0, 1)
    w.value(2, 2)
    w.value(hlit, 5)
    w.value(0, 5)
    w.value(hclen, 4)
    for s in CL_ORDER[:hclen + 4]:
        w.value(cl_lengths.get(s, 0), 3)
    for s, nbits, extra in cl_syms:
        w.code(cl_codes[s])
        w.value(extra, nbits)
    header_bits = len(w.bits)
    for kind, v in toks:
        if kind == "lit":
            w.code(codes[v])
        else:
            s, nbits, extra = length_symbol(v)
            w.code(codes[s])
            w.value(extra, nbits)
            w.value(0, 1)               # the one distance code there is: distance 1
    w.code(codes[256])
    if not final:
        w.value(0, 3)                   # an empty stored block: the next block starts on a byte
        w.pad()
        w.bits += [0] * 16 + [1] * 16
    w.pad()
    report = {"count": count, "matches": matches, "literals": len(toks) - matches, "lengths": [lengths.get(s, 0) for s in range(286)],
              "longest": longest, "dist_length": dist_length, "hlit": hlit, "hclen": hclen,
              "cl_lengths": [cl_lengths.get(s, 0) for s in range(19)], "header_bits": header_bits}
    data = w.bytes()
    head = BitWriter()
    head.bits = w.bits[:header_bits]
    head.pad()
    report["header"] = head.bytes()
    report["bytes"] = len(data)
    return data, report


def adler32(data):
    a, b = 1, 0
    for v in data:
        a = (a + v) % 65521
        b = (b + a) % 65521
    return (b << 16) | a


def zlib_stream(stream, block_bytes=0):
    """-> (the zlib stream, the blocks' reports with their byte offsets in it)"""
    block_bytes = block_bytes or BLOCK_BYTES_DEFAULT
    out, reports = bytearray(b"\x78\x01"), []
    for at in range(0, len(stream), block_bytes):
        data, report = deflate_block(stream[at:at + block_bytes], at + block_bytes >= len(stream))
        report["offset"], report["stream_offset"] = len(out), at
        out += data
        reports.append(report)
    out += struct.pack(">I", adler32(stream))
    return bytes(out), reports


# ---- 5. container ----
def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def encode(samples, width, height, bits=8, channels=3, filter=None, block_bytes=0, idat_bytes=0):
    """-> (the file, its report: the stats the library gives, and what the tests look at)"""
    samples = np.asarray(samples, dtype=np.uint8).reshape(height, -1)
    bpp = channels * bits // 8
    assert samples.shape == (height, width * bpp) and channels in (1, 3) and bits in (8, 16)
    for size in (block_bytes, idat_bytes):
        assert size == 0 or SIZE_MIN <= size <= SIZE_MAX
    stream, rows = filter_stream(samples, bpp, filter)
    z, blocks = zlib_stream(stream, block_bytes)
    idat_bytes = idat_bytes or IDAT_BYTES_DEFAULT
    out = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, bits, 2 if channels == 3 else 0, 0, 0, 0))
    for at in range(0, len(z), idat_bytes):
        out += chunk(b"IDAT", z[at:at + idat_bytes])
    out += chunk(b"IEND", b"")
    stats = {"rows": rows, "blocks": len(blocks), "literals": sum(b["literals"] for b in blocks),
             "matches": sum(b["matches"] for b in blocks), "stream_bytes": len(z), "adler": adler32(stream)}
    return out, {"stats": stats, "filtered": stream, "zlib": z, "blocks": blocks}


def encode_case(case):
    return encode(**case)


def idat_data(file):
    """the concatenated data of a file's IDAT chunks, and the chunk kinds in order (every CRC checked)"""
    assert file[:8] == b"\x89PNG\r\n\x1a\n"
    at, data, kinds = 8, bytearray(), []
    while at < len(file):
        n, kind = struct.unpack(">I", file[at:at + 4])[0], file[at + 4:at + 8]
        body = file[at + 8:at + 8 + n]
        assert struct.unpack(">I", file[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + body), kind
        kinds.append(kind)
        if kind == b"IDAT":
            data += body
        at += 12 + n
    assert at == len(file)
    return bytes(data), kinds


# ---- the directed cases ----
def _case(samples, width, height, bits=8, channels=1, filter=None, block_bytes=32, idat_bytes=32):
    samples = np.ascontiguousarray(samples, dtype=np.uint8).reshape(height, width * channels * bits // 8)
    return {"samples": samples, "width": width, "height": height, "bits": bits, "channels": channels, "filter": filter,
            "block_bytes": block_bytes, "idat_bytes": idat_bytes}


def _spread(counts):
    """the values with these counts in an order in which no two neighbours are equal"""
    left, out, prev = dict(counts), [], None
    while left:
        v = max((v for v in left if v != prev), key=lambda v: (left[v], -v))
        out.append(v)
        left[v] -= 1
        if not left[v]:
            del left[v]
        prev = v
    return out


def fibonacci_samples():
    """one row of 6762 bytes: value k (1..16) F(k + 2) times — 2, 3, 5, ... 2584 — no two neighbours equal: literals only.  With the
    row's filter byte (one 0) and EOB (once) the block's counts are 1, 1, 2, 3, 5, ... 2584: a tree 17 deep"""
    fib = [1, 1]
    while len(fib) < 18:
        fib.append(fib[-1] + fib[-2])
    return np.array(_spread({k + 1: f for k, f in enumerate(fib[2:])}), dtype=np.uint8).reshape(1, 6762)


RUN_LENGTHS = (2, 3, 4, 258, 259, 260, 261, 517)


def filters_image():
    """12 x 24 grey: noise, ramps and their repeats, shifts and blends, chosen so that each of the five filters wins a row by the
    restatement's own count (tests/test_png_cpu.py asserts it); row 0 is a tie — none and up give the same bytes there — that none wins"""
    x = np.arange(24)
    noise = np.random.default_rng(7).integers(0, 256, size=(3, 24))
    ramp = (x * 9 + 3) % 256
    rows = [
        np.where(x % 2 == 0, 1, 255),
        noise[0],
        noise[0],
        ramp,
        ramp,
        (ramp + 40) % 256,
        noise[1],
        (noise[1] // 2 + np.roll(noise[1], 1) // 2) % 256,
        (x * x) % 256,
        ((x * x) % 256 + x * 5) % 256,
        noise[2],
        (noise[2].astype(int) + np.roll(noise[2], 1) - np.roll(noise[1], 1)) % 256,
    ]
    return np.array(rows, dtype=np.uint8)


# ---- the edges of a tile: the 1024 positions of a block that its workgroup takes per trip (k_png_count, k_png_pack) ----
TILE = 1024
# every name tile_cases() gives (tests/test_png_cpu.py asserts of each what it is there for)
TILE_CASE_NAMES = ("tiles_exact", "tiles_plus_1", "block_1025", "run_over_tiles", "match_at_tile_end", "match_at_tile_start", "tail_1", "tail_2",
                   "tail_3", "block_ends_in_ahead", "run_cut_at_tile", "dense_tile")
DENSE_TILE_BITS = TILE * 15 + 6         # what k_png_pack's staging words of a tile are sized for


def _stream_case(stream, block_bytes, idat_bytes=64):
    """one greyscale row under filter 0 whose filtered stream is `stream` (its first byte the filter byte: 0)"""
    assert stream[0] == 0
    return _case([list(stream[1:])], len(stream) - 1, 1, filter=0, block_bytes=block_bytes, idat_bytes=idat_bytes)


def _noise(rng, n, values=256):
    """a stream of n bytes behind its filter byte in which no two neighbours are equal"""
    out = [0]
    while len(out) < n:
        v = int(rng.integers(0, values))
        if v != out[-1]:
            out.append(v)
    return out


def _with_run(stream, head, last, value=None):
    """stream with positions head..last (inclusive) holding one value that the bytes on either side do not hold"""
    out = list(stream)
    around = {out[head - 1]} | ({out[last + 1]} if last + 1 < len(out) else set())
    value = next(v for v in range(200, 256) if v not in around) if value is None else value
    assert value not in around
    out[head:last + 1] = [value] * (last + 1 - head)
    return out


def ruler(n):
    """(i & -i).bit_length() for i = 1 .. 2^n - 1: value k 2^(n - k) times, no two neighbours equal"""
    return [(i & -i).bit_length() for i in range(1, 1 << n)]


def dense_tile_stream():
    """a block whose tile 0 has as many bits as a tile can have: 1023 literals of 15 bits and, at its last position, a match with 15
    bits of length code, 5 extra bits and the distance's bit.  The filter byte and 230 values a few times each are the rare symbols;
    the ruler sequence behind (values 1..18, 2^17 down to 1 times) makes the tree 18 deep, so that limiting to 15 bits leaves every
    rare symbol — the match of 200 among them, counted once — with 15"""
    stream = [0] + [20 + p % 230 for p in range(1, TILE - 1)]
    stream += [stream[-1]] * 200
    return stream + ruler(18)


def tile_cases():
    rng = np.random.default_rng(1024)
    out = {}
    # an exact number of tiles, one byte more, and a tile and a byte: values 0..2, so that short runs lie on every tile edge
    small = [0] + [int(v) for v in rng.integers(0, 3, size=4 * TILE)]
    out["tiles_exact"] = _stream_case(small[:4 * TILE], 4 * TILE)
    # (the last tile's one byte is place 1 of its piece: a literal whose stretch began in the tile before)
    plus1 = list(small)
    plus1[4 * TILE - 3:] = [7, 9, 9, 9]
    out["tiles_plus_1"] = _stream_case(plus1, 4 * TILE + 1)
    out["block_1025"] = _stream_case(small[:TILE + 1], 2 * TILE)
    # one value from 500 to 3700: tile 1024..2047 and tile 2048..3071 hold no byte that breaks the run
    out["run_over_tiles"] = _stream_case(_with_run(_noise(rng, 4 * TILE), 500, 3700), 4 * TILE)
    # the pieces behind a head at 248 begin at 249, 507, 765 and 1023; behind one at 249, at 1024
    long_run = _with_run(_noise(rng, 1600), 248, 1400)
    out["match_at_tile_end"] = _stream_case(long_run, 2 * TILE)
    out["match_at_tile_start"] = _stream_case(_with_run(_noise(rng, 1600), 249, 1400), 2 * TILE)
    for k in (1, 2, 3):
        out[f"tail_{k}"] = _stream_case(_with_run(_noise(rng, 1100), 248, 248 + 3 * 258 + k), 2 * TILE)
    # the same stream cut 101 bytes into the look-ahead of position 1023, and at the tile's end
    out["block_ends_in_ahead"] = _stream_case(long_run, TILE + 100)
    out["run_cut_at_tile"] = _stream_case(long_run, TILE)
    out["dense_tile"] = _stream_case(dense_tile_stream(), 1 << 19, idat_bytes=0)
    assert tuple(out) == TILE_CASE_NAMES
    return out


def directed_cases():
    rng = np.random.default_rng(2025)
    out = {}
    out["1x1"] = _case([[200]], 1, 1, block_bytes=16, idat_bytes=16)
    out["strip_1x7"] = _case(rng.integers(0, 256, size=(7, 1)), 1, 7, block_bytes=16, idat_bytes=16)
    out["strip_7x1"] = _case(rng.integers(0, 256, size=(1, 7)), 7, 1, block_bytes=16, idat_bytes=16)
    out["rgb_10x7"] = _case(rng.integers(0, 256, size=(7, 30)), 10, 7, channels=3, block_bytes=24, idat_bytes=40)
    # 3 rows of 11 bytes: blocks of 16, 16 and 1
    out["last_block_1"] = _case(rng.integers(0, 256, size=(3, 10)), 10, 3, block_bytes=16, idat_bytes=20)
    # 19 zeros: a block of 16 (a literal and a match) and one of 3 — one distinct value, too short to match: that literal and EOB
    out["two_symbols"] = _case(np.zeros((1, 18)), 18, 1, filter=0, block_bytes=16, idat_bytes=64)
    out["all_256"] = _case(rng.permutation(256).reshape(1, 256), 256, 1, filter=0, block_bytes=512, idat_bytes=64)
    out["fibonacci"] = _case(fibonacci_samples(), 6762, 1, filter=0, block_bytes=0, idat_bytes=64)
    row = []
    for k, n in enumerate(RUN_LENGTHS):
        row += [10 + k] * (1 + n)
    out["runs"] = _case([row], len(row), 1, filter=0, block_bytes=2048, idat_bytes=64)
    # one value throughout: every block edge cuts the run, and it ends with the stream
    out["run_across_blocks"] = _case(np.full((1, 100), 77), 100, 1, filter=0, block_bytes=32, idat_bytes=48)
    out["run_to_the_end"] = _case([[1, 2, 3, 4, 5, 6, 7] + [9] * 40], 47, 1, filter=0, block_bytes=64, idat_bytes=16)
    out["filters"] = _case(filters_image(), 24, 12, block_bytes=48, idat_bytes=56)
    ramp = (np.arange(9 * 5 * 3).reshape(5, 27) * 37 + rng.integers(0, 3, size=(5, 27))).astype(">u2")
    out["rgb16"] = _case(ramp.view(np.uint8).reshape(5, 54), 9, 5, bits=16, channels=3, block_bytes=40, idat_bytes=32)
    grey = (np.arange(13 * 6).reshape(6, 13) * 811 + rng.integers(0, 3, size=(6, 13))).astype(">u2")
    out["grey16"] = _case(grey.view(np.uint8).reshape(6, 26), 13, 6, bits=16, block_bytes=33, idat_bytes=17)
    out["ff_300x300"] = _case(np.full((300, 300), 255), 300, 300, filter=0, block_bytes=64, idat_bytes=64)
    # the zlib stream an exact number of IDAT chunks, and one byte more: the Adler's four bytes in two chunks
    base = _case(rng.integers(0, 256, size=(5, 33)), 11, 5, channels=3, block_bytes=48)
    n = len(encode_case(base)[1]["zlib"])
    exact = [d for d in range(16, 65) if n % d == 0]
    plus1 = [d for d in range(16, 65) if n % d == 1]
    assert exact and plus1, n
    out["idat_exact"] = dict(base, idat_bytes=exact[0])
    out["idat_plus_1"] = dict(base, idat_bytes=plus1[0])
    out.update(tile_cases())
    return out
