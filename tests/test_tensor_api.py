"""Tensor output, the parts that need no GPU: the rule that picks k_to_tensor's destination path (j2p_debug_tensor_path —
the host function that is the only place to know it), the layout of j2p_job with its appended out_tensor field against the
binding's mirror of it, and the lazy torch import."""
import ctypes
import os
import subprocess
import sys

import pytest

U8, F16, BF16, F32 = 0, 1, 2, 3
GENERIC, PLANAR, INTERLEAVED = "generic", "planar", "interleaved"
BASE = 1 << 20                      # an address aligned to anything

# (w, nplane, dtype, (stride_c, stride_y, stride_x), address) -> path.  A vector store is 4 elements: 16 / 8 / 4 bytes for
# f32 / 16-bit / u8, and the address, stride_y and — planar, three planes — stride_c must keep every one of them aligned.
TABLE = [
    # contiguous CHW and HWC
    (48, 3, F32, (32 * 48, 48, 1), BASE, PLANAR),
    (48, 3, U8, (32 * 48, 48, 1), BASE, PLANAR),
    (48, 3, F32, (1, 144, 3), BASE, INTERLEAVED),
    (48, 3, U8, (1, 144, 3), BASE, INTERLEAVED),
    (48, 1, F16, (32 * 48, 48, 1), BASE, PLANAR),
    (48, 1, BF16, (1, 48, 1), BASE, PLANAR),                    # (H, W, 1): one plane interleaved IS planar
    # the alignment threshold of the address, per dtype: the store width and nothing less
    (48, 3, F32, (1536, 48, 1), BASE + 16, PLANAR), (48, 3, F32, (1536, 48, 1), BASE + 8, GENERIC), (48, 3, F32, (1536, 48, 1), BASE + 4, GENERIC),
    (48, 3, F16, (1536, 48, 1), BASE + 8, PLANAR), (48, 3, F16, (1536, 48, 1), BASE + 4, GENERIC), (48, 3, F16, (1536, 48, 1), BASE + 2, GENERIC),
    (48, 3, BF16, (1536, 48, 1), BASE + 8, PLANAR), (48, 3, BF16, (1536, 48, 1), BASE + 4, GENERIC), (48, 3, BF16, (1536, 48, 1), BASE + 2, GENERIC),
    (48, 3, U8, (1536, 48, 1), BASE + 4, PLANAR), (48, 3, U8, (1536, 48, 1), BASE + 2, GENERIC), (48, 3, U8, (1536, 48, 1), BASE + 1, GENERIC),
    (48, 3, F32, (1, 144, 3), BASE + 16, INTERLEAVED), (48, 3, F32, (1, 144, 3), BASE + 8, GENERIC),
    (48, 3, F16, (1, 144, 3), BASE + 8, INTERLEAVED), (48, 3, F16, (1, 144, 3), BASE + 4, GENERIC),
    (48, 3, U8, (1, 144, 3), BASE + 4, INTERLEAVED), (48, 3, U8, (1, 144, 3), BASE + 3, GENERIC),
    # rows and channels that are not a multiple of 4 elements apart: some row or channel would be misaligned
    (47, 3, F32, (32 * 47, 47, 1), BASE, GENERIC),
    (46, 3, U8, (32 * 46, 46, 1), BASE, GENERIC),
    (47, 3, U8, (1, 141, 3), BASE, GENERIC),
    (48, 3, F16, (1538, 48, 1), BASE, GENERIC),
    (48, 1, F16, (1538, 48, 1), BASE, PLANAR),                  # one plane: stride_c is never used
    (47, 3, F32, (40 * 64, 64, 1), BASE, PLANAR),               # a 47-wide crop of rows 64 apart: the tail takes element stores
    # padded and batched destinations
    (48, 3, F16, (40 * 64, 64, 1), BASE + 2 * (3 * 40 * 64 + 4 * 64 + 8), PLANAR),
    (48, 3, F16, (40 * 64, 64, 1), BASE + 2 * (3 * 40 * 64 + 4 * 64 + 2), GENERIC),
    (48, 3, U8, (1, 4 * 64, 4), BASE, GENERIC),                 # RGB inside RGBA pixels
    # other strides
    (48, 3, F32, (1536, 1, 32), BASE, GENERIC),                 # transposed
    (48, 3, F32, (1536, 96, 2), BASE, GENERIC),                 # every second column
    (48, 3, F32, (2, 144, 3), BASE, GENERIC),
    # narrower than one group of four pixels
    (1, 3, F32, (32, 4, 1), BASE, GENERIC), (2, 3, U8, (1, 8, 3), BASE, GENERIC), (3, 1, F16, (96, 4, 1), BASE, GENERIC),
    (4, 3, F32, (128, 4, 1), BASE, PLANAR), (4, 3, U8, (1, 12, 3), BASE, INTERLEAVED), (5, 3, BF16, (256, 8, 1), BASE, PLANAR),
]


@pytest.mark.parametrize("w,nplane,dtype,strides,address,want", TABLE)
def test_tensor_path_table(lib, w, nplane, dtype, strides, address, want):
    import jpeg2png_amd as j
    assert j.tensor_path(w, nplane, dtype, *strides, address) == want


def test_tensor_path_refuses_what_the_call_refuses(lib):
    import jpeg2png_amd as j
    for args in ((48, 2, F32, 1536, 48, 1, BASE), (48, 3, 4, 1536, 48, 1, BASE), (48, 3, -1, 1536, 48, 1, BASE), (0, 3, F32, 1536, 48, 1, BASE),
                 (48, 3, F32, 0, 48, 1, BASE), (48, 3, F32, 1536, 0, 1, BASE), (48, 3, F32, 1536, 48, -1, BASE)):
        with pytest.raises(j.J2PError):
            j.tensor_path(*args)


def test_job_struct_matches_the_library(lib):
    """out_tensor is appended to j2p_job: the binding's mirror has the size and the offset the library was compiled with,
    and the fields before it sit where they sat (a job built by an older caller reads as "no tensor" only if so)"""
    import jpeg2png_amd as j
    size, offset = j.job_layout()
    assert ctypes.sizeof(j._CJob) == size
    assert j._CJob.out_tensor.offset == offset
    assert offset + ctypes.sizeof(j._CTensor) == size
    last = j._CJob.out_sub_h
    assert last.offset + last.size <= offset < last.offset + last.size + 8
    t = j._CTensor
    assert (t.data.offset, t.dtype.offset, t.stride_c.offset, t.stride_y.offset, t.stride_x.offset, t.scale.offset, t.bias.offset,
            ctypes.sizeof(t)) == (0, 8, 16, 24, 32, 40, 52, 64)
    assert j._CJob().out_tensor.data is None                    # zero-initialised jobs have no tensor output


def test_symbols_are_exported(lib):
    for name in ("j2p_planes_to_tensor", "j2p_planes_rows_to_tensor", "j2p_debug_tensor_path", "j2p_debug_job_layout"):
        assert hasattr(lib, name)


def test_the_package_does_not_import_torch():
    """torch is only needed — and only imported — by tensor output"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; import jpeg2png_amd as j; j.load_library(); j.tensor_path(48, 3, 3, 1536, 48, 1, 4096); "
            "b = j.Batch.__new__(j.Batch); assert 'torch' not in sys.modules, 'torch was imported'")
    r = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
