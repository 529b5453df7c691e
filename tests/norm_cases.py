"""The ||g|| reduction restated in float64, one addition here per addition of a kernel, and the arrays that tell its
association from the plausible wrong ones.

||g|| = sqrtf((float) sum of g^2) is reduced in three steps (DESIGN.md sections 2 and 4, jpeg2png_amd/csrc/j2p_kernels.hip.h):

  strip partial   one double per (tile row, strip): what one wavefront of k_gradient sums over its rows and lanes
                  (march_rows, gradient_strip)                                                     -> strip_partial
  level 1         the strips of one tile row: eight interleaved running sums, combined pairwise
                  (strip_sum; k_rowsums, k_norm_whole, fold_tile_row)                              -> strip_sum
  level 2         the tile rows: a stride tree over the array padded to a power of two
                  (tree_sum_lds; k_norm_finish, k_norm_whole, k_norm_bands, fold_tree, norm_tree_*) -> tree, norm

The pinned functions and the mutants below are written with `+` alone on Python floats (IEEE doubles), so the same code
also runs on symbols (_Sym): that is how `live` decides whether a mutant is another function at a given length at all.
Nothing in a pinned path uses np.sum or math.fsum.  strip_sums / tree_rows are the same additions on whole numpy arrays
(tests/test_norm_cases_cpu.py holds them to the scalar forms bit for bit)."""
import math

import numpy as np

STRIP_COLS = 124            # kStripCols
# the exact sum every fixture is completed to: the midpoint of two neighbouring floats whose square roots differ as floats
MIDPOINT = float.fromhex("0x1.0e147fp+1")
SEARCH_SEEDS = 300


def _items(p):
    return p.tolist() if isinstance(p, np.ndarray) else list(p)


def _out(x):
    return np.float64(x) if isinstance(x, float) else x


# ---- level 1 --------------------------------------------------------------------------------------------------------
def strip_sum(p):
    """strip_sum (j2p_kernels.hip.h): running sum i % 8 takes element i in increasing i, then the pairwise combine"""
    s = [0.0] * 8
    for i, x in enumerate(_items(p)):
        s[i % 8] = s[i % 8] + x
    return _out(((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7])))


def l1_sequential(p):
    s = 0.0
    for x in _items(p):
        s = s + x
    return _out(s)


def l1_interleaved4(p):
    s = [0.0] * 4
    for i, x in enumerate(_items(p)):
        s[i % 4] = s[i % 4] + x
    return _out((s[0] + s[1]) + (s[2] + s[3]))


def l1_interleaved16(p):
    s = [0.0] * 16
    for i, x in enumerate(_items(p)):
        s[i % 16] = s[i % 16] + x
    while len(s) > 1:
        s = [s[2 * i] + s[2 * i + 1] for i in range(len(s) // 2)]
    return _out(s[0])


def l1_interleaved8_sequential_combine(p):
    s = [0.0] * 8
    for i, x in enumerate(_items(p)):
        s[i % 8] = s[i % 8] + x
    t = s[0]
    for j in range(1, 8):
        t = t + s[j]
    return _out(t)


# ---- level 2 --------------------------------------------------------------------------------------------------------
def _pow2(n, least=1):
    P = least
    while P < n:
        P <<= 1
    return P


def tree(v, least=1):
    """tree_sum_lds: pad with +0.0 to the next power of two P (norm_tree_load: at least 64), then
    buf[:s] = buf[:s] + buf[s:2s] for s = P/2 ... 1"""
    buf = _items(v)
    P = _pow2(len(buf), least)
    buf = buf + [0.0] * (P - len(buf))
    s = P >> 1
    while s >= 1:
        for i in range(s):
            buf[i] = buf[i] + buf[i + s]
        s >>= 1
    return _out(buf[0])


def l2_sequential(v):
    return l1_sequential(v)


def l2_reversed(v):
    return l1_sequential(_items(v)[::-1])


def l2_adjacent_pairs(v):
    buf = _items(v)
    buf = buf + [0.0] * (_pow2(len(buf)) - len(buf))
    while len(buf) > 1:
        buf = [buf[2 * i] + buf[2 * i + 1] for i in range(len(buf) // 2)]
    return _out(buf[0])


PINNED = {1: strip_sum, 2: tree}
MUTANTS = {
    1: {"sequential": l1_sequential, "interleaved4": l1_interleaved4, "interleaved16": l1_interleaved16,
        "interleaved8_sequential_combine": l1_interleaved8_sequential_combine},
    2: {"sequential": l2_sequential, "reversed": l2_reversed, "adjacent_pairs": l2_adjacent_pairs},
}


def to_norm(total):
    """sqrtf((float) total), both roundings IEEE (compute.c:205)"""
    return np.sqrt(np.float32(total), dtype=np.float32)


def norm(v):
    return to_norm(tree(v))


def norm_bits(x):
    return int(np.float32(x).view(np.uint32))


# ---- the same additions on whole arrays ---------------------------------------------------------------------------
def strip_sums(a):
    """strip_sum over the last axis of a float64 array"""
    a = np.asarray(a, np.float64)
    n = a.shape[-1]
    s = np.zeros(a.shape[:-1] + (8,), np.float64)
    for t in range(0, n - n % 8, 8):
        s = s + a[..., t:t + 8]
    r = n % 8
    if r:
        s[..., :r] = s[..., :r] + a[..., n - r:]
    return ((s[..., 0] + s[..., 1]) + (s[..., 2] + s[..., 3])) + ((s[..., 4] + s[..., 5]) + (s[..., 6] + s[..., 7]))


def tree_rows(a, least=1):
    """tree over the first axis of a float64 array ([tile row][channel] row sums -> [channel])"""
    a = np.asarray(a, np.float64)
    P = _pow2(a.shape[0], least)
    buf = np.zeros((P,) + a.shape[1:], np.float64)
    buf[:a.shape[0]] = a
    s = P >> 1
    while s >= 1:
        buf[:s] = buf[:s] + buf[s:2 * s]
        s >>= 1
    return buf[0]


def norms_of_rows(a):
    return np.sqrt(tree_rows(a).astype(np.float32), dtype=np.float32)


# ---- the strip partial ------------------------------------------------------------------------------------------------
def ntx_of(W):
    return 1 if W <= 4 else (W - 4 + STRIP_COLS - 1) // STRIP_COLS          # j2p_solver_create: strips


def strip_partial(g, rpw, tile_row, strip):
    """The partial of (tile_row, strip) from the gradient plane g (float32 [rows, W], the solver's own rows) in march_rows'
    canonical order (line numbers: jpeg2png_amd/csrc/j2p_kernels.hip.h).
      lane l holds the columns strip * 124 + 2 l and + 1 (:990) and owns them when they are in the image and are not the
        strip's two halo columns on either side — which the first strip owns on the left and the last on the right (:993);
      a row adds float(g * g) of the first pixel, then of the second (:1222; add_elements :368-372), rows in increasing
        order into the running sum of their group of FOUR rows (g2, :1105);
      a closed group goes into lo (row index within the tile row & 8 clear) or hi (set) (close_group :1108-1126; a short
        last tile row closes its open group the same way, :1258);
      the lane's value is lo + hi, summed over the 64 lanes by v[l] += v[l + off], off = 32 ... 1 (gradient_strip
        :1325-1327)."""
    g = np.asarray(g, np.float32)
    rows, W = g.shape
    lane = np.arange(64)
    xl = strip * STRIP_COLS + 2 * lane
    own = (xl < W) & ((lane >= 1) | (strip == 0)) & ((lane <= 62) | (strip * STRIP_COLS + 128 >= W))
    col = np.minimum(xl, W - 2)
    tile0 = tile_row * rpw
    t1 = min(tile0 + rpw, rows)
    lo, hi, g2 = np.zeros(64), np.zeros(64), np.zeros(64)

    def close(t):
        nonlocal lo, hi, g2
        if (t - tile0) & 8:
            hi = hi + g2
        else:
            lo = lo + g2
        g2 = np.zeros(64)

    for t in range(tile0, t1):
        e0 = np.where(own, g[t, col] * g[t, col], np.float32(0)).astype(np.float64)          # float products
        e1 = np.where(own, g[t, col + 1] * g[t, col + 1], np.float32(0)).astype(np.float64)
        g2 = g2 + e0
        g2 = g2 + e1
        if (t - tile0) & 3 == 3:
            close(t)
    if (t1 - tile0) & 3:
        close(t1 - 1)
    v = lo + hi
    off = 32
    while off >= 1:
        v[:64 - off] = v[:64 - off] + v[off:]
        off >>= 1
    return np.float64(v[0])


def strip_partials(g, rpw):
    """[tile row][strip] partials of a whole plane"""
    rows, W = g.shape
    ntr, ntx = (rows + rpw - 1) // rpw, ntx_of(W)
    return np.array([[strip_partial(g, rpw, tr, x) for x in range(ntx)] for tr in range(ntr)], np.float64)


# ---- which mutants are another function at all ----------------------------------------------------------------------
class _Sym:
    """a sum as a symbol: commutative, x + 0.0 = x, nothing else.  Two sums are the same function of their elements
    exactly when their ids agree."""
    _table = {}

    def __init__(self, ident):
        self.ident = ident

    def __add__(self, other):
        if isinstance(other, float):
            assert other == 0.0
            return self
        key = (min(self.ident, other.ident), max(self.ident, other.ident))
        if key not in _Sym._table:
            _Sym._table[key] = 1_000_000 + len(_Sym._table)
        return _Sym(_Sym._table[key])

    __radd__ = __add__


def live(level, n):
    """names of the level's mutants that are not the pinned function at length n"""
    x = [_Sym(i) for i in range(n)]
    want = PINNED[level](x)
    out = []
    for name, fn in MUTANTS[level].items():
        got = fn(x)
        if n and got.ident != want.ident:
            out.append(name)
    return out


# ---- fixtures ---------------------------------------------------------------------------------------------------------
def candidate(n, seed):
    """n - 1 values uniform(0, 1) * 2^k, k in -40 ... -27, and one at a seeded position that completes the exact sum to
    MIDPOINT: the associations of the sum then land on either side of a float rounding boundary"""
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.0, 1.0, n) * 2.0 ** rng.integers(-40, -26, n)
    pos = int(rng.integers(n))
    v[pos] = 0.0
    v[pos] = MIDPOINT - math.fsum(v.tolist())
    return v


_fixtures = {}
SEEDS = {}                  # (level, n, mutant name) -> the seed of its fixture: candidate(n, seed)


def fixtures(level, n):
    """{mutant name: float64 array of n values} for every live mutant: the pinned function and the mutant give different
    FLOAT norms on it.  The first seed that does; RuntimeError when none of SEARCH_SEEDS does."""
    if (level, n) in _fixtures:
        return _fixtures[(level, n)]
    pinned, found = PINNED[level], {}
    for name in live(level, n):
        mutant = MUTANTS[level][name]
        for seed in range(SEARCH_SEEDS):
            v = candidate(n, seed)
            if norm_bits(to_norm(pinned(v))) != norm_bits(to_norm(mutant(v))):
                found[name] = v
                SEEDS[(level, n, name)] = seed
                break
        else:
            raise RuntimeError(f"level {level}, n = {n}: no array among {SEARCH_SEEDS} seeds separates the pinned sum from '{name}'")
    _fixtures[(level, n)] = found
    return found


# the sizes the GPU tests run (tests/test_norm_gpu.py), searched here once, at import
LEVEL2_SIZES = (1, 2, 3, 5, 63, 64, 65, 127, 128, 129, 1023, 1024)          # every level-2 form
LEVEL2_LAUNCH_SIZES = LEVEL2_SIZES + (1025, 4096)                            # k_norm_finish, k_norm_bands (kMaxTileRows)
LEVEL1_SIZES = (1, 5, 7, 8, 9, 16, 17, 48, 49, 65, 256, 257, 529)           # strips per tile row (k_norm_whole)
for _n in LEVEL2_LAUNCH_SIZES:
    fixtures(2, _n)
for _n in LEVEL1_SIZES:
    fixtures(1, _n)


def in_channel(v, nch, c, seed=0):
    """v as channel c of an interleaved [row][channel] array, unrelated sums of like magnitudes in the other channels"""
    rng = np.random.default_rng(1000 + seed)
    a = rng.uniform(0.0, 1.0, (len(v), nch)) * 2.0 ** rng.integers(-40, 2, (len(v), nch))
    a[:, c] = v
    return a
