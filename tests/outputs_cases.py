"""Multi-output tensor resampling (j2p_planes_to_tensors_resampled): the output sets both test files go through.  No tests here.

An output is (box or None for the whole image, out_w, out_h, filter name, dtype name, layout).  The images are those of
filter_cases.IMAGES; the truth of every output is the single call on the same solver."""
import filter_cases as fc

MAX_OUTPUTS = 16                                                # J2P_MAX_OUTPUTS
DTYPES = {"u8": 0, "f16": 1, "bf16": 2, "f32": 3}               # J2P_DTYPE_*
BOX = (3, 2, 20, 17)

# the second enlarges, the third is the identity
K3 = [(None, 7, 5, "cubic", "f32", "chw"), (BOX, 64, 33, "triangle", "f32", "chw"), (BOX, 20, 17, "triangle", "f32", "chw")]

# widths on the edges of the 32- and 64-lane tiles, heights on the edges of 4 rows per wavefront and 4 wavefronts per workgroup;
# boxes overlap ((3, 1, 40, 30) and (10, 5, 30, 30)), repeat, and one output is its box (33 x 17)
_W16 = [1, 31, 32, 33, 63, 64, 65, 129, 129, 65, 64, 63, 33, 32, 31, 1]
_H16 = [1, 3, 4, 5, 15, 16, 17, 1, 17, 16, 15, 5, 17, 3, 4, 37]
_B16 = [None, (3, 1, 40, 30), (3, 1, 40, 30), (10, 5, 30, 30)]
K16 = [((3, 1, 33, 17) if (w, h) == (33, 17) else _B16[i % 4], w, h, "cubic" if i % 3 == 0 else "triangle", "f32", "chw")
       for i, (w, h) in enumerate(zip(_W16, _H16))]

# rows of two 512-column chunks and a tail next to grids of one workgroup; the last is the identity
WIDE = [(None, 1039, 5, "triangle", "f32", "chw"), (None, 1041, 30, "cubic", "f32", "chw"), (None, 1, 1, "triangle", "f32", "chw"),
        (None, 3, 5, "cubic", "f32", "chw"), ((517, 3, 520, 20), 520, 20, "cubic", "f32", "chw")]

# every dtype in both layouts in one call: four sampling launches of two outputs each; shrinking, enlarging, identity
MIXED = [(None, 24, 20, "triangle", "u8", "chw"), (None, 96, 50, "cubic", "f16", "hwc"), ((5, 3, 16, 16), 16, 16, "cubic", "bf16", "chw"),
         (None, 7, 5, "triangle", "f32", "hwc"), ((5, 3, 16, 16), 37, 41, "cubic", "u8", "hwc"), (None, 12, 10, "triangle", "f16", "chw"),
         (None, 53, 41, "triangle", "bf16", "hwc"), ((7, 9, 5, 3), 64, 40, "cubic", "f32", "chw")]

SETS = {"k3": ("padded_420", K3), "k3_reversed": ("padded_420", K3[::-1]), "k16": ("grey", K16), "wide": ("wide", WIDE),
        "mixed": ("clamping_444", MIXED)}
assert len(K16) == MAX_OUTPUTS and len({(w, h) for _, w, h, *_ in K16}) == 16
assert {(o[4], o[5]) for o in MIXED} == {(d, layout) for d in DTYPES for layout in ("chw", "hwc")}

# outputs at the limits of a side, in an image that large: a grid of one workgroup, of 2047 tile columns, of 16375 row groups
EXTREME = (65536, 65536, [((0, 0, 1, 1), 1, 1, "triangle", "f32", "chw"), ((0, 0, 65500, 1), 65500, 1, "triangle", "f32", "chw"),
                          ((0, 0, 1, 65500), 1, 65500, "cubic", "f32", "chw")])


def spec(image_size, out):
    """(box_x, box_y, box_w, box_h, out_w, out_h, filter code) of an output of an image of that size"""
    box, ow, oh, name = out[:4]
    return (*((0, 0, *image_size) if box is None else box), ow, oh, fc.FILTERS[name])


def own_grid(tile, ow, oh):
    """(tile columns, row groups) of one output's launch: a workgroup is 4 wavefronts, one above the other, of one tile"""
    lanes, slots, rows = tile
    return -(-ow // (lanes * slots)), -(-(-(-oh // rows)) // 4)
