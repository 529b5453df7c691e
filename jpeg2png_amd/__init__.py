"""jpeg2png_amd — MI355X (gfx950) implementation of jpeg2png's TV/TGV deblocking solver.

Python here is only a ctypes binding of the C-ABI in include/jpeg2png_amd.h (used by
tests/ and bench.py, and as the host-side mirror of the reference's compute()
interface).  The product is libjpeg2png_amd.so: hand-written HIP kernels behind a
plain-C shim plus a C `compute()` with the reference's own signature.

There is NO CPU fallback: if the shared library is missing or no GPU is present the
calls raise.
"""
import collections
import contextlib
import ctypes
import os

import numpy as np

from .synth import Plane  # noqa: F401  (re-export: the Python twin of struct coef)

_HERE = os.path.dirname(os.path.abspath(__file__))
# J2P_LIBRARY selects another build of the library (A/B timing of kernel variants on one box)
LIB_PATH = os.environ.get("J2P_LIBRARY") or os.path.join(_HERE, "libjpeg2png_amd.so")

J2P_MAX_CHANNELS = 3
J2P_HALO_ROWS = 2
J2P_TILE_ROWS = 16


class J2PError(RuntimeError):
    """code: the library's J2P_E* code where the error came from a library call (J2P_EFORMAT, J2P_ENOTSUP, ...), else None"""
    code = None


class _CPlane(ctypes.Structure):
    _fields_ = [("w", ctypes.c_uint), ("h", ctypes.c_uint),
                ("w_samp", ctypes.c_uint), ("h_samp", ctypes.c_uint),
                ("data", ctypes.c_void_p), ("fdata", ctypes.c_void_p),
                ("quant_table", ctypes.c_void_p)]


class _CBand(ctypes.Structure):
    _fields_ = [("row_begin", ctypes.c_uint), ("row_end", ctypes.c_uint)]


class _CLogRow(ctypes.Structure):
    _fields_ = [("objective", ctypes.c_double), ("prob_dist", ctypes.c_double),
                ("tv", ctypes.c_double), ("tv2", ctypes.c_double)]


_ROWS_CB = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.POINTER(_CLogRow))
_PROGRESS_CB = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_uint)


class _CTensor(ctypes.Structure):
    """j2p_tensor: a strided destination in device memory (strides in elements)"""
    _fields_ = [("data", ctypes.c_void_p), ("dtype", ctypes.c_int),
                ("stride_c", ctypes.c_ssize_t), ("stride_y", ctypes.c_ssize_t), ("stride_x", ctypes.c_ssize_t),
                ("scale", ctypes.c_float * 3), ("bias", ctypes.c_float * 3)]


class _CResize(ctypes.Structure):
    """j2p_resize: a source rectangle of the image and the size it is area-resampled to"""
    _fields_ = [("box_x", ctypes.c_uint), ("box_y", ctypes.c_uint), ("box_w", ctypes.c_uint), ("box_h", ctypes.c_uint),
                ("out_w", ctypes.c_uint), ("out_h", ctypes.c_uint)]


class _CResample(ctypes.Structure):
    """j2p_resample: a source rectangle of the image, the size it is resampled to (smaller or larger) and the filter"""
    _fields_ = [("box_x", ctypes.c_uint), ("box_y", ctypes.c_uint), ("box_w", ctypes.c_uint), ("box_h", ctypes.c_uint),
                ("out_w", ctypes.c_uint), ("out_h", ctypes.c_uint), ("filter", ctypes.c_int)]


class _COutput(ctypes.Structure):
    """j2p_output: one item of a multi-output call — what is resampled, and the tensor that receives it"""
    _fields_ = [("r", _CResample), ("t", _CTensor)]


J2P_MAX_OUTPUTS = 16


class _CSamples(ctypes.Structure):
    """j2p_samples: one channel's 8-bit samples in device or host memory (strides in bytes)"""
    _fields_ = [("data", ctypes.c_void_p), ("w", ctypes.c_uint), ("h", ctypes.c_uint),
                ("stride_y", ctypes.c_ssize_t), ("stride_x", ctypes.c_ssize_t)]


class _CQuantEstimate(ctypes.Structure):
    """j2p_quant_estimate_result: one channel's estimated table"""
    _fields_ = [("table", ctypes.c_uint16 * 64), ("determined", ctypes.c_uint8 * 64), ("quality", ctypes.c_int)]


class _CJpeg(ctypes.Structure):
    """j2p_jpeg: the image, its chroma subsampling and the quantisation tables of a JPEG file made on the device"""
    _fields_ = [("width", ctypes.c_uint), ("height", ctypes.c_uint), ("sub_w", ctypes.c_uint), ("sub_h", ctypes.c_uint),
                ("quant", ctypes.c_void_p * 3)]


J2P_ESPACE = -5         # the caller's output buffer is too small; the size needed has been stored
J2P_EFORMAT = -6        # a JPEG file given to the library is damaged
J2P_ENOTSUP = -7        # a JPEG file given to the library is valid, and of a kind its decoder does not read


class _CJpegComponent(ctypes.Structure):
    """j2p_jpeg_component"""
    _fields_ = [("id", ctypes.c_uint), ("h_samp_factor", ctypes.c_uint), ("v_samp_factor", ctypes.c_uint),
                ("blocks_w", ctypes.c_uint), ("blocks_h", ctypes.c_uint), ("w_samp", ctypes.c_uint), ("h_samp", ctypes.c_uint),
                ("quant_slot", ctypes.c_uint), ("dc_slot", ctypes.c_uint), ("ac_slot", ctypes.c_uint), ("quant", ctypes.c_uint16 * 64)]


class _CJpegInfo(ctypes.Structure):
    """j2p_jpeg_info: what j2p_jpeg_parse reads from a file's marker segments"""
    _fields_ = [("width", ctypes.c_uint), ("height", ctypes.c_uint), ("ncomp", ctypes.c_uint), ("extended", ctypes.c_uint),
                ("comp", _CJpegComponent * 3), ("mcus_w", ctypes.c_uint), ("mcus_h", ctypes.c_uint), ("blocks_per_mcu", ctypes.c_uint),
                ("restart_interval", ctypes.c_uint), ("intervals", ctypes.c_uint), ("scan_begin", ctypes.c_size_t), ("scan_end", ctypes.c_size_t)]


J2P_JPEG_OPTIMIZE = 1    # j2p_*_ex flags: Huffman tables made for the image


class _CEncodeStats(ctypes.Structure):
    """j2p_encode_stats"""
    _fields_ = [("dc0", ctypes.c_ulonglong * 256), ("ac0", ctypes.c_ulonglong * 256), ("dc1", ctypes.c_ulonglong * 256),
                ("ac1", ctypes.c_ulonglong * 256), ("scan_bits", ctypes.c_ulonglong), ("stuffed_bytes", ctypes.c_ulonglong)]


class _CProgressiveScan(ctypes.Structure):
    """j2p_progressive_scan"""
    _fields_ = [("ncomp", ctypes.c_uint), ("comp", ctypes.c_uint * 3), ("ss", ctypes.c_uint), ("se", ctypes.c_uint), ("ah", ctypes.c_uint),
                ("al", ctypes.c_uint), ("ntables", ctypes.c_uint), ("table", ctypes.c_uint * 2), ("counts", (ctypes.c_ulonglong * 256) * 2),
                ("bits", ctypes.c_ulonglong), ("stuffed_bytes", ctypes.c_ulonglong), ("eob_runs", ctypes.c_ulonglong)]


class _CProgressiveStats(ctypes.Structure):
    """j2p_progressive_stats"""
    _fields_ = [("nscans", ctypes.c_uint), ("scan", _CProgressiveScan * 10)]


class _CJpegOptions(ctypes.Structure):
    """j2p_jpeg_options"""
    _fields_ = [("flags", ctypes.c_uint), ("progressive", ctypes.c_uint), ("restart_interval", ctypes.c_uint), ("restart_in_rows", ctypes.c_uint)]


class _CRestartScan(ctypes.Structure):
    """j2p_restart_scan"""
    _fields_ = [("units", ctypes.c_uint), ("units_per_row", ctypes.c_uint), ("interval", ctypes.c_uint), ("intervals", ctypes.c_uint),
                ("dri", ctypes.c_uint)]


class _CRestartPlan(ctypes.Structure):
    """j2p_restart_plan"""
    _fields_ = [("nscans", ctypes.c_uint), ("scan", _CRestartScan * 10)]


class _CRestartScanStats(ctypes.Structure):
    """j2p_restart_scan_stats"""
    _fields_ = [("interval", ctypes.c_uint), ("intervals", ctypes.c_uint), ("padding_bits", ctypes.c_ulonglong), ("markers", ctypes.c_ulonglong)]


class _CRestartStats(ctypes.Structure):
    """j2p_restart_stats"""
    _fields_ = [("nscans", ctypes.c_uint), ("scan", _CRestartScanStats * 10)]


class _CPng(ctypes.Structure):
    """j2p_png: the image, the filter and the block sizes of a PNG file made on the device"""
    _fields_ = [("width", ctypes.c_uint), ("height", ctypes.c_uint), ("bits", ctypes.c_uint), ("filter", ctypes.c_int),
                ("block_bytes", ctypes.c_uint), ("idat_bytes", ctypes.c_uint)]


class _CPngStats(ctypes.Structure):
    """j2p_png_stats"""
    _fields_ = [("rows", ctypes.c_ulonglong * 5), ("blocks", ctypes.c_ulonglong), ("literals", ctypes.c_ulonglong),
                ("matches", ctypes.c_ulonglong), ("stream_bytes", ctypes.c_ulonglong), ("adler", ctypes.c_uint)]


J2P_PNG_FILTER_ADAPTIVE = -1
J2P_PNG_BLOCK_BYTES, J2P_PNG_IDAT_BYTES, J2P_PNG_SIZE_MIN, J2P_PNG_SIZE_MAX = 65536, 8192, 16, 1 << 24
PNG_FILTERS = {None: -1, "adaptive": -1, "none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4}

J2P_DECODE_SUBSEQUENCE_BITS, J2P_DECODE_SUBSEQUENCE_MIN, J2P_DECODE_SUBSEQUENCE_MAX = 1024, 32, 65536
J2P_DECODE_STATS_ROUNDS = 16


class _CDecodeStats(ctypes.Structure):
    """j2p_decode_stats"""
    _fields_ = [("subsequences", ctypes.c_uint), ("intervals", ctypes.c_uint), ("rounds", ctypes.c_uint),
                ("recomputed", ctypes.c_uint * J2P_DECODE_STATS_ROUNDS), ("data_bytes", ctypes.c_ulonglong), ("decode_ms", ctypes.c_double)]


J2P_DECODE_SCANS_MAX = 128


class _CJpegScan(ctypes.Structure):
    """j2p_jpeg_scan"""
    _fields_ = [("ncomp", ctypes.c_uint), ("comp", ctypes.c_uint * 3), ("ss", ctypes.c_uint), ("se", ctypes.c_uint), ("ah", ctypes.c_uint),
                ("al", ctypes.c_uint), ("dc_slot", ctypes.c_uint * 3), ("ac_slot", ctypes.c_uint * 3), ("restart_interval", ctypes.c_uint),
                ("intervals", ctypes.c_uint), ("begin", ctypes.c_size_t), ("end", ctypes.c_size_t)]


class _CJpegScans(ctypes.Structure):
    """j2p_jpeg_scans"""
    _fields_ = [("nscans", ctypes.c_uint), ("progressive", ctypes.c_uint), ("scan", _CJpegScan * J2P_DECODE_SCANS_MAX)]


class _CScansStats(ctypes.Structure):
    """j2p_scans_stats"""
    _fields_ = [("scans", ctypes.c_uint), ("dc_first", ctypes.c_uint), ("ac_first", ctypes.c_uint), ("dc_refine", ctypes.c_uint),
                ("ac_refine", ctypes.c_uint), ("subsequences", ctypes.c_uint), ("rounds", ctypes.c_uint), ("host_waits", ctypes.c_uint),
                ("data_bytes", ctypes.c_ulonglong), ("decode_ms", ctypes.c_double), ("ac_refine_share", ctypes.c_double)]


class _CJob(ctypes.Structure):
    _fields_ = [("nchannel", ctypes.c_uint), ("planes", _CPlane * 3), ("separate", ctypes.c_int),
                ("weight", ctypes.c_float * 3), ("pweight", ctypes.c_float * 3), ("iterations", ctypes.c_uint * 3),
                ("out_bits", ctypes.c_uint), ("out_w", ctypes.c_uint), ("out_h", ctypes.c_uint),
                ("out_rgb", ctypes.c_void_p), ("out_planes", ctypes.c_void_p * 3),
                ("on_rows", _ROWS_CB), ("on_progress", _PROGRESS_CB), ("user", ctypes.c_void_p), ("tile", ctypes.c_int),
                ("tile_first", ctypes.c_uint), ("tile_count", ctypes.c_uint), ("tile_min_band_pixels", ctypes.c_size_t),
                ("out_quant", ctypes.c_void_p * 3), ("out_coef", ctypes.c_void_p * 3),
                ("out_blocks_w", ctypes.c_uint), ("out_blocks_h", ctypes.c_uint),
                ("out_sub_w", ctypes.c_uint * 3), ("out_sub_h", ctypes.c_uint * 3),
                ("out_tensor", _CTensor)]


class _CPlaneRef(ctypes.Structure):
    _fields_ = [("solver", ctypes.c_void_p), ("channel", ctypes.c_uint)]


class _CExchange(ctypes.Structure):
    _fields_ = [("partials_local", ctypes.c_void_p), ("local_tile_rows", ctypes.c_uint),
                ("partials_all", ctypes.c_void_p), ("global_tile_rows", ctypes.c_uint),
                ("first_tile_row", ctypes.c_uint),
                ("send_top", ctypes.c_void_p * 3), ("recv_top", ctypes.c_void_p * 3),
                ("send_bottom", ctypes.c_void_p * 3), ("recv_bottom", ctypes.c_void_p * 3),
                ("halo_floats", ctypes.c_size_t), ("log_local", ctypes.c_void_p)]


# every symbol include/jpeg2png_amd.h and include/jpeg2png_amd_compute.h declare
C_ABI_SYMBOLS = [
    "j2p_version", "j2p_last_error", "j2p_device_count",
    "j2p_solver_create", "j2p_solver_destroy", "j2p_solver_canvas", "j2p_solver_band",
    "j2p_solver_reset", "j2p_solver_run", "j2p_solver_phase_gradient", "j2p_solver_phase_project",
    "j2p_solver_phase_gradient_part", "j2p_solver_phase_rowsums", "j2p_solver_phase_project_part",
    "j2p_solver_exchange_info", "j2p_solver_commit_initial_halo", "j2p_solver_download",
    "j2p_solver_download_gradient", "j2p_solver_set_logging", "j2p_log_rows_from_sums",
    "j2p_solver_plane_ptr", "j2p_solver_sync", "j2p_solver_kernel_times", "j2p_solver_enable_timing",
    "j2p_decode_plane", "j2p_dct8x8_blocks", "j2p_math_selftest", "j2p_planes_to_rgb", "j2p_planes_rows_to_rgb", "j2p_sqrt_exhaustive",
    "j2p_planes_to_grey", "j2p_planes_rows_to_grey", "j2p_planes_to_coefficients", "j2p_planes_rows_to_coefficients",
    "j2p_planes_to_coefficients_sub", "j2p_planes_rows_to_coefficients_sub",
    "j2p_planes_to_tensor", "j2p_planes_rows_to_tensor", "j2p_debug_tensor_path", "j2p_debug_job_layout",
    "j2p_planes_to_tensor_resized", "j2p_batch_submit_resized",
    "j2p_planes_to_tensor_resampled", "j2p_batch_submit_resampled", "j2p_debug_filter_taps",
    "j2p_planes_to_tensors_resampled", "j2p_batch_submit_outputs", "j2p_debug_outputs_plan", "j2p_debug_outputs_workgroups",
    "j2p_pool_trim", "j2p_solver_debug_option", "j2p_solver_stream", "j2p_solver_halo_rows",
    "j2p_solver_norm_from_bands", "j2p_solver_copy_rows", "j2p_solver_alternate_rowsums",
    "j2p_tiled_create", "j2p_tiled_destroy", "j2p_tiled_canvas", "j2p_tiled_band", "j2p_tiled_run", "j2p_tiled_reset", "j2p_tiled_sync",
    "j2p_tiled_download", "j2p_tiled_host_cpu_seconds", "j2p_rccl_version", "j2p_solver_norm_ptr", "j2p_solver_norm_external",
    "j2p_solver_global_rowsums", "j2p_solver_link_bands", "j2p_tiled_exchange",
    "j2p_batch_create", "j2p_batch_destroy", "j2p_batch_submit", "j2p_batch_wait",
    "compute", "j2p_compute", "j2p_compute_tiled", "j2p_compute_timing", "j2p_debug_fail_run_after", "j2p_solver_launches_per_iteration", "j2p_solver_timing_overhead",
    "j2p_debug_build", "j2p_debug_grad_items", "j2p_debug_norm_plan", "j2p_experiments_build", "j2p_solver_debug_violations", "j2p_solver_trace", "j2p_division_exhaustive",
    "j2p_solver_coefficient_bytes", "j2p_solver_wide_footprint", "j2p_solver_shares_state", "j2p_solver_arena_bytes",
    "j2p_solver_debug_partials", "j2p_norm_selftest", "j2p_norm_selftest_bands",
    "j2p_solver_create_from_samples", "j2p_solver_download_coefficients", "j2p_solver_clipped_samples", "j2p_batch_submit_samples",
    "j2p_planes_to_jpeg", "j2p_entropy_encode", "j2p_batch_submit_jpeg",
    "j2p_jpeg_parse", "j2p_entropy_decode", "j2p_entropy_decode_ex", "j2p_solver_create_from_jpeg",
    "j2p_batch_submit_file", "j2p_batch_submit_file_jpeg",
    "j2p_planes_to_jpeg_ex", "j2p_entropy_encode_ex", "j2p_batch_submit_jpeg_ex", "j2p_batch_submit_file_jpeg_ex",
    "j2p_solver_output_scratch_bytes",
    "j2p_planes_to_jpeg_progressive", "j2p_entropy_encode_progressive", "j2p_batch_submit_jpeg_progressive",
    "j2p_batch_submit_file_jpeg_progressive",
    "j2p_planes_to_png", "j2p_png_encode", "j2p_batch_submit_png", "j2p_batch_submit_file_png",
    "j2p_jpeg_orientation", "j2p_solver_set_orientation", "j2p_solver_orientation", "j2p_solver_upright_bytes",
    "j2p_batch_next_orientation",
    "j2p_solver_phase_order", "j2p_debug_project_items", "j2p_debug_phase_order", "j2p_debug_grad_items_workgroups",
    "j2p_pool_thread_takes",
    "j2p_jpeg_parse_scans", "j2p_entropy_decode_scans", "j2p_solver_create_from_jpeg_scans", "j2p_batch_next_file_scans",
    "j2p_debug_restart_plan", "j2p_planes_to_jpeg_opt", "j2p_entropy_encode_opt", "j2p_batch_submit_jpeg_opt", "j2p_batch_submit_file_jpeg_opt",
    "j2p_samples_histogram", "j2p_quant_estimate", "j2p_batch_submit_samples_estimated",
]
J2P_ORIENTATION_EXIF = 0xffffffff           # j2p_batch_next_orientation: the tag of the job's file
# the forms of the ||g|| reduction j2p_norm_selftest launches (J2P_NORM_FORM_*)
NORM_FORMS = {"rowsums": 0, "norm_whole": 1, "norm_finish": 2, "norm_bands": 3, "fold_tree": 4, "project_tree": 5}
J2P_OPT_NORM_FOLD, J2P_OPT_NORM_IN_PROJECT, J2P_OPT_NT_GRADIENT, J2P_OPT_MIXED_PROJECT = 1, 4, 5, 6
J2P_OPT_NARROW_COEFFICIENTS = 7
J2P_OPT_WIDE_FOOTPRINT = 8
J2P_OPT_PHASE_ORDER = 9
# the order in which every XCD walks its run of a phase launch (J2P_ORDER_*): top-down, or its own run bottom-up
J2P_ORDER_FORWARD, J2P_ORDER_REVERSE = 0, 1


def phase_order(gradient, project):
    """the value of J2P_OPT_PHASE_ORDER (and of the environment's J2P_PHASE_ORDER) for the two phases' orders"""
    return int(gradient) | (int(project) << 1)


ZOOM_MAX = 4
J2P_DTYPE_U8, J2P_DTYPE_F16, J2P_DTYPE_BF16, J2P_DTYPE_F32 = 0, 1, 2, 3
TENSOR_PATHS = ("generic", "planar", "interleaved")     # what j2p_debug_tensor_path reports: 0, 1, 2

_lib = None


def build(force=False, verbose=False):
    from .buildlib import build as _build
    return _build(force=force, verbose=verbose)


def _share_torch_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64 / libhsa-runtime64.  A process must not end up with
    two HIP runtimes (ours from /opt/rocm loaded first, torch's afterwards: torch then reports "No HIP GPUs
    are available"), so when torch is installed but not imported yet, load ITS runtime first; our library's
    libamdhip64.so.N dependency then resolves to that copy, exactly as when torch was imported first."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    bundled = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(bundled):
        try:
            ctypes.CDLL(bundled, mode=ctypes.RTLD_GLOBAL)
        except OSError:
            pass


def hip_runtime():
    """ctypes handle of the HIP runtime this process (and our library) is bound to — for tests and tools that
    want hipMemcpy & co.  Loading "libamdhip64.so" by name could pull a second copy of the runtime in."""
    load_library()
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    if not paths:
        raise J2PError("no HIP runtime is mapped into this process")
    return ctypes.CDLL(sorted(paths)[0])


def load_library():
    """dlopen libjpeg2png_amd.so; raises J2PError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    _lib = _bind(LIB_PATH)
    return _lib


class library:
    """context manager: another build of the library for the objects created inside the block — the experiments build
    (-DJ2P_EXPERIMENTS: the release kernels plus environment knobs and split phases the release build does not carry, buildlib.build_experiments)
    in the schedule-equivalence tests.  Solvers remember the library they were created from; both copies share the
    process's HIP runtime."""

    def __init__(self, path):
        self.path = path

    def __enter__(self):
        global _lib
        load_library()
        self._saved = _lib
        _lib = _bind(self.path)
        return _lib

    def __exit__(self, *exc):
        global _lib
        _lib = self._saved


_bound = {}


def _bind(path):
    if path in _bound:
        return _bound[path]
    if not os.path.exists(path):
        raise J2PError(f"{path} is missing: run `python -m jpeg2png_amd.buildlib` "
                       "(the HIP extension is the only implementation; there is no fallback)")
    _share_torch_hip_runtime()
    lib = ctypes.CDLL(path)   # RTLD_LOCAL: our `compute` must not interpose other libraries' symbols
    lib.j2p_version.restype = ctypes.c_char_p
    lib.j2p_last_error.restype = ctypes.c_char_p
    lib.j2p_solver_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_void_p,
                                      ctypes.c_uint, ctypes.POINTER(_CPlane), ctypes.c_float,
                                      ctypes.POINTER(ctypes.c_float), ctypes.c_uint, _CBand, ctypes.c_int]
    lib.j2p_solver_destroy.argtypes = [ctypes.c_void_p]
    lib.j2p_solver_destroy.restype = None
    lib.j2p_solver_phase_gradient_part.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    lib.j2p_solver_phase_project_part.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.j2p_solver_set_logging.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.j2p_log_rows_from_sums.argtypes = [ctypes.c_uint, ctypes.c_float, ctypes.POINTER(ctypes.c_float), ctypes.c_uint,
                                           ctypes.c_void_p, ctypes.POINTER(_CLogRow)]
    for name in ("j2p_solver_reset", "j2p_solver_phase_gradient", "j2p_solver_phase_project",
                 "j2p_solver_sync", "j2p_solver_commit_initial_halo", "j2p_solver_phase_rowsums"):
        getattr(lib, name).argtypes = [ctypes.c_void_p]
    lib.j2p_solver_canvas.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_uint)]
    lib.j2p_solver_band.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_uint)]
    lib.j2p_solver_run.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.POINTER(_CLogRow)]
    lib.j2p_solver_exchange_info.argtypes = [ctypes.c_void_p, ctypes.POINTER(_CExchange)]
    lib.j2p_solver_download.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p]
    lib.j2p_solver_download_gradient.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p]
    lib.j2p_solver_plane_ptr.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.POINTER(ctypes.c_void_p)]
    lib.j2p_solver_kernel_times.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double),
                                            ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint)]
    lib.j2p_solver_enable_timing.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.j2p_decode_plane.argtypes = [ctypes.c_int, ctypes.c_uint, ctypes.c_uint, ctypes.c_void_p,
                                     ctypes.c_void_p, ctypes.c_void_p]
    lib.j2p_dct8x8_blocks.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    lib.j2p_device_count.argtypes = [ctypes.POINTER(ctypes.c_int)]
    lib.j2p_math_selftest.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_uint,
                                      ctypes.POINTER(ctypes.c_ulonglong), ctypes.POINTER(ctypes.c_ulonglong)]
    lib.j2p_solver_debug_partials.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint),
                                              ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_uint)]
    lib.j2p_norm_selftest_bands.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.c_void_p,
                                            ctypes.c_uint, ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_uint),
                                            ctypes.c_void_p, ctypes.c_void_p]
    lib.j2p_norm_selftest.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_void_p]
    lib.j2p_solver_debug_option.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    lib.j2p_solver_debug_violations.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_ulonglong), ctypes.POINTER(ctypes.c_uint),
                                                ctypes.POINTER(ctypes.c_ulonglong)]
    lib.j2p_pool_trim.restype = None
    if hasattr(lib, "j2p_pool_thread_takes"):
        # (a build of an earlier commit, loaded as the baseline of an A/B timing, does not count its takes)
        lib.j2p_pool_thread_takes.argtypes = []
        lib.j2p_pool_thread_takes.restype = ctypes.c_ulonglong
    lib.j2p_tiled_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint, ctypes.POINTER(ctypes.c_int),
                                     ctypes.POINTER(ctypes.c_uint), ctypes.c_uint, ctypes.POINTER(_CPlane), ctypes.c_float,
                                     ctypes.POINTER(ctypes.c_float), ctypes.c_uint]
    lib.j2p_tiled_destroy.argtypes = [ctypes.c_void_p]
    lib.j2p_tiled_destroy.restype = None
    lib.j2p_tiled_canvas.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_uint),
                                     ctypes.POINTER(ctypes.c_uint)]
    lib.j2p_tiled_band.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint),
                                   ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_void_p)]
    lib.j2p_tiled_run.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.POINTER(_CLogRow)]
    lib.j2p_tiled_sync.argtypes = [ctypes.c_void_p]
    lib.j2p_tiled_reset.argtypes = [ctypes.c_void_p]
    lib.j2p_tiled_download.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p]
    lib.j2p_tiled_host_cpu_seconds.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]
    lib.j2p_planes_rows_to_coefficients_sub.argtypes = [ctypes.POINTER(_CPlaneRef), ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint,
                                                        ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p]
    lib.j2p_planes_to_coefficients_sub.argtypes = [ctypes.POINTER(_CPlaneRef), ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint,
                                                   ctypes.c_void_p, ctypes.c_void_p]
    lib.j2p_planes_to_tensor.argtypes = [ctypes.POINTER(_CPlaneRef), ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.POINTER(_CTensor)]
    lib.j2p_planes_rows_to_tensor.argtypes = [ctypes.POINTER(_CPlaneRef), ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint,
                                              ctypes.POINTER(_CTensor)]
    lib.j2p_planes_to_tensor_resized.argtypes = [ctypes.POINTER(_CPlaneRef), ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.POINTER(_CResize),
                                                 ctypes.POINTER(_CTensor)]
    lib.j2p_batch_submit_resized.argtypes = [ctypes.c_void_p, ctypes.POINTER(_CJob), ctypes.POINTER(_CResize), ctypes.POINTER(ctypes.c_int)]
    lib.j2p_planes_to_tensor_resampled.argtypes = [ctypes.POINTER(_CPlaneRef), ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.POINTER(_CResample),
                                                   ctypes.POINTER(_CTensor)]
    lib.j2p_batch_submit_resampled.argtypes = [ctypes.c_void_p, ctypes.POINTER(_CJob), ctypes.POINTER(_CResample), ctypes.POINTER(ctypes.c_int)]
    lib.j2p_debug_filter_taps.argtypes = [ctypes.c_int, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.POINTER(ctypes.c_uint),
                                          ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_float), ctypes.c_uint]
    if hasattr(lib, "j2p_planes_to_tensors_resampled"):
        # (a build of an earlier commit, loaded next to this one as the baseline of an A/B timing — tools/outputs_probe.py — has
        # not got the multi-output calls; using them on it is an AttributeError)
        lib.j2p_planes_to_tensors_resampled.argtypes = [ctypes.POINTER(_CPlaneRef), ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint,
                                                        ctypes.POINTER(_COutput)]
        lib.j2p_batch_submit_outputs.argtypes = [ctypes.c_void_p, ctypes.POINTER(_CJob), ctypes.c_uint, ctypes.POINTER(_COutput),
                                                 ctypes.POINTER(ctypes.c_int)]
        lib.j2p_debug_outputs_plan.argtypes = [ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.POINTER(_CResample), ctypes.POINTER(ctypes.c_int),
                                               ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_uint),
                                               ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint)]
        lib.j2p_debug_outputs_workgroups.argtypes = [ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.POINTER(_CResample),
                                                     ctypes.POINTER(ctypes.c_int), ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.c_void_p]
    if hasattr(lib, "j2p_solver_create_from_samples"):
        # (as above: an earlier commit's build has no sample input)
        lib.j2p_solver_create_from_samples.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_void_p, ctypes.c_uint,
                                                       ctypes.POINTER(_CPlane), ctypes.POINTER(_CSamples), ctypes.c_float,
                                                       ctypes.POINTER(ctypes.c_float), ctypes.c_uint]
        lib.j2p_solver_download_coefficients.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p]
        lib.j2p_solver_clipped_samples.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.POINTER(ctypes.c_ulonglong)]
        lib.j2p_batch_submit_samples.argtypes = [ctypes.c_void_p, ctypes.POINTER(_CJob), ctypes.POINTER(_CSamples), ctypes.c_uint,
                                                 ctypes.POINTER(_COutput), ctypes.POINTER(ctypes.c_int)]
    if hasattr(lib, "j2p_samples_histogram"):
        # (as above: an earlier commit's build estimates no tables)
        lib.j2p_samples_histogram.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(_CSamples), ctypes.c_void_p,
                                              ctypes.POINTER(ctypes.c_ulonglong), ctypes.POINTER(ctypes.c_ulonglong)]
        lib.j2p_quant_estimate.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(_CQuantEstimate)]
        lib.j2p_batch_submit_samples_estimated.argtypes = [ctypes.c_void_p, ctypes.POINTER(_CJob), ctypes.POINTER(_CSamples), ctypes.c_uint,
                                                           ctypes.POINTER(_COutput), ctypes.POINTER(_CQuantEstimate), ctypes.POINTER(ctypes.c_int)]
    if hasattr(lib, "j2p_entropy_encode_opt"):
        # (as above: an earlier commit's build does not write files, or not every kind).  The record describes a JPEG write: the
        # three _opt calls and the one behind a batch's file are what this module calls, the twelve older ones are their shorthands
        planes = [ctypes.POINTER(_CPlaneRef), ctypes.c_uint, ctypes.POINTER(_CJpeg), ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
        coded = [ctypes.c_int, ctypes.POINTER(_CJpeg), ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint, ctypes.c_void_p, ctypes.c_size_t,
                 ctypes.POINTER(ctypes.c_size_t)]
        to = [ctypes.POINTER(_CJpeg), ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
        job = [ctypes.c_void_p, ctypes.POINTER(_CJob), ctypes.POINTER(_CSamples)] + to
        file = [ctypes.c_void_p, ctypes.POINTER(_CJob), ctypes.c_void_p, ctypes.c_size_t] + to
        options, ticket = [ctypes.POINTER(_CJpegOptions)], [ctypes.POINTER(ctypes.c_int)]
        lib.j2p_debug_restart_plan.argtypes = [ctypes.c_uint] * 5 + options + [ctypes.POINTER(_CRestartPlan)]
        lib.j2p_planes_to_jpeg_opt.argtypes = planes + options
        lib.j2p_planes_to_jpeg.argtypes = lib.j2p_planes_to_jpeg_progressive.argtypes = planes
        lib.j2p_planes_to_jpeg_ex.argtypes = planes + [ctypes.c_uint]
        lib.j2p_entropy_encode_opt.argtypes = coded + options + [ctypes.POINTER(_CEncodeStats), ctypes.POINTER(_CProgressiveStats),
                                                                 ctypes.POINTER(_CRestartStats)]
        lib.j2p_entropy_encode.argtypes = coded
        lib.j2p_entropy_encode_ex.argtypes = coded + [ctypes.c_uint, ctypes.POINTER(_CEncodeStats)]
        lib.j2p_entropy_encode_progressive.argtypes = coded + [ctypes.POINTER(_CProgressiveStats)]
        lib.j2p_batch_submit_jpeg_opt.argtypes = job + options + ticket
        lib.j2p_batch_submit_jpeg.argtypes = lib.j2p_batch_submit_jpeg_progressive.argtypes = job + ticket
        lib.j2p_batch_submit_jpeg_ex.argtypes = job + [ctypes.c_uint] + ticket
        lib.j2p_batch_submit_file_jpeg_opt.argtypes = file + options + ticket
        lib.j2p_batch_submit_file_jpeg.argtypes = lib.j2p_batch_submit_file_jpeg_progressive.argtypes = file + ticket
        lib.j2p_batch_submit_file_jpeg_ex.argtypes = file + [ctypes.c_uint] + ticket
    if hasattr(lib, "j2p_png_encode"):
        # (as above: an earlier commit's build writes no PNG)
        lib.j2p_planes_to_png.argtypes = [ctypes.POINTER(_CPlaneRef), ctypes.c_uint, ctypes.POINTER(_CPng), ctypes.c_void_p, ctypes.c_size_t,
                                          ctypes.POINTER(ctypes.c_size_t)]
        lib.j2p_png_encode.argtypes = [ctypes.c_int, ctypes.POINTER(_CPng), ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p, ctypes.c_size_t,
                                       ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(_CPngStats)]
        lib.j2p_batch_submit_png.argtypes = [ctypes.c_void_p, ctypes.POINTER(_CJob), ctypes.POINTER(_CSamples), ctypes.POINTER(_CPng), ctypes.c_void_p,
                                             ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int)]
        lib.j2p_batch_submit_file_png.argtypes = [ctypes.c_void_p, ctypes.POINTER(_CJob), ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(_CPng),
                                                  ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int)]
    if hasattr(lib, "j2p_jpeg_orientation"):
        # (as above: an earlier commit's build has no upright output)
        lib.j2p_jpeg_orientation.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint)]
        lib.j2p_solver_set_orientation.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint]
        lib.j2p_solver_orientation.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_uint),
                                               ctypes.POINTER(ctypes.c_uint)]
        lib.j2p_solver_upright_bytes.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
        lib.j2p_batch_next_orientation.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint]
    if hasattr(lib, "j2p_entropy_decode_ex"):
        # (as above: an earlier commit's build does not read files)
        lib.j2p_jpeg_parse.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(_CJpegInfo)]
        lib.j2p_entropy_decode.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p,
                                           ctypes.POINTER(_CJpegInfo)]
        lib.j2p_entropy_decode_ex.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p,
                                              ctypes.POINTER(_CJpegInfo), ctypes.c_uint, ctypes.POINTER(_CDecodeStats)]
        lib.j2p_batch_submit_file.argtypes = [ctypes.c_void_p, ctypes.POINTER(_CJob), ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint,
                                              ctypes.POINTER(_COutput), ctypes.POINTER(ctypes.c_int)]
        lib.j2p_solver_create_from_jpeg.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                                    ctypes.c_float, ctypes.POINTER(ctypes.c_float), ctypes.c_uint, ctypes.POINTER(_CJpegInfo)]
    if hasattr(lib, "j2p_entropy_decode_scans"):
        # (as above: an earlier commit's build does not read progressive files)
        lib.j2p_jpeg_parse_scans.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(_CJpegInfo), ctypes.POINTER(_CJpegScans)]
        lib.j2p_entropy_decode_scans.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p,
                                                 ctypes.POINTER(_CJpegInfo), ctypes.c_uint, ctypes.POINTER(_CScansStats)]
        lib.j2p_solver_create_from_jpeg_scans.argtypes = lib.j2p_solver_create_from_jpeg.argtypes
        lib.j2p_batch_next_file_scans.argtypes = [ctypes.c_void_p, ctypes.c_uint]
    lib.j2p_debug_tensor_path.argtypes = [ctypes.c_uint, ctypes.c_uint, ctypes.c_int, ctypes.c_ssize_t, ctypes.c_ssize_t, ctypes.c_ssize_t,
                                          ctypes.c_size_t, ctypes.POINTER(ctypes.c_int)]
    lib.j2p_debug_job_layout.argtypes = [ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]
    lib.j2p_debug_job_layout.restype = None
    lib.j2p_solver_stream.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
    lib.j2p_batch_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint, ctypes.POINTER(ctypes.c_int), ctypes.c_uint]
    lib.j2p_batch_destroy.argtypes = [ctypes.c_void_p]
    lib.j2p_batch_destroy.restype = None
    lib.j2p_batch_submit.argtypes = [ctypes.c_void_p, ctypes.POINTER(_CJob), ctypes.POINTER(ctypes.c_int)]
    lib.j2p_batch_wait.argtypes = [ctypes.c_void_p, ctypes.c_int]
    _bound[path] = lib
    return lib


def _check(rc):
    if rc != 0:
        err = J2PError(f"jpeg2png_amd error {rc}: {load_library().j2p_last_error().decode()}")
        err.code = rc
        raise err


def debug_build():
    """True when the loaded library was compiled with -DJ2P_DEBUG (address checks in the phase kernels)"""
    return bool(load_library().j2p_debug_build())


def rccl_version():
    """ncclGetVersion of the librccl the C row tiling would dlopen for its `rccl` exchange, or None (no usable library)"""
    v = ctypes.c_int(0)
    return v.value if load_library().j2p_rccl_version(ctypes.byref(v)) == 0 else None


def experiments_build():
    """True when the loaded library is the experiments build (-DJ2P_EXPERIMENTS): the environment knobs that move choices
    among the release kernels, and the split phases, answer only there"""
    return bool(load_library().j2p_experiments_build())


def device_count():
    n = ctypes.c_int(0)
    _check(load_library().j2p_device_count(ctypes.byref(n)))
    return n.value


def decode_plane(plane, device=0):
    """decode_coefficients + unbox on the GPU (jpeg.c:83-92, box.c:5-19) -> float32 [h, w]."""
    lib = load_library()
    data = np.ascontiguousarray(plane.data, dtype=np.int16)
    q = np.ascontiguousarray(plane.quant_table, dtype=np.uint16)
    out = np.empty((plane.h, plane.w), dtype=np.float32)
    _check(lib.j2p_decode_plane(device, plane.w, plane.h, data.ctypes.data, q.ctypes.data, out.ctypes.data))
    return out


def dct8x8_blocks(blocks, inverse=False, device=0):
    """dct8x8s / idct8x8s (ooura/dct.c:98 / :34) of n blocks of 64 floats on the GPU."""
    lib = load_library()
    b = np.array(blocks, dtype=np.float32, order="C").reshape(-1, 64)
    _check(lib.j2p_dct8x8_blocks(device, b.ctypes.data, b.shape[0], 1 if inverse else 0))
    return b


def math_selftest(n, seed=1, device=0):
    """(division mismatches, sqrt mismatches) of the fast paths vs IEEE on n random operand pairs."""
    d, q = ctypes.c_ulonglong(), ctypes.c_ulonglong()
    _check(load_library().j2p_math_selftest(device, n, seed, ctypes.byref(d), ctypes.byref(q)))
    return d.value, q.value


def norm_selftest(form, data, bands=None, device=0):
    """One form of the ||g|| reduction (a key of NORM_FORMS) on the caller's float64 array, launched as a solve launches
    it (j2p_norm_selftest).  "rowsums", "norm_whole": data = partials [channel, tile row, strip]; every other form: row
    sums [tile row, channel].  Returns the float32 norms [channel] — "rowsums": the float64 level-1 sums [tile row, channel].
    bands ("norm_bands" only): [(first tile row, tile rows), ...] in the order the kernel is to take them; default: one."""
    lib = load_library()
    a = np.ascontiguousarray(data, dtype=np.float64)
    from_partials = form in ("rowsums", "norm_whole")
    if a.ndim != (3 if from_partials else 2):
        raise J2PError(f"norm_selftest: '{form}' takes a {3 if from_partials else 2}-dimensional array")
    nch, rows, ntx = a.shape if from_partials else (a.shape[1], a.shape[0], 0)
    rowsums = np.full((rows, nch), np.nan, dtype=np.float64)
    norms = np.full(nch, np.nan, dtype=np.float32)
    if bands is None:
        _check(lib.j2p_norm_selftest(device, NORM_FORMS[form], nch, rows, ntx, a.ctypes.data, rowsums.ctypes.data, norms.ctypes.data))
    else:
        first = (ctypes.c_uint * len(bands))(*[int(b[0]) for b in bands])
        count = (ctypes.c_uint * len(bands))(*[int(b[1]) for b in bands])
        _check(lib.j2p_norm_selftest_bands(device, NORM_FORMS[form], nch, rows, ntx, a.ctypes.data, len(bands), first, count,
                                           rowsums.ctypes.data, norms.ctypes.data))
    return rowsums if form == "rowsums" else norms


def sqrt_exhaustive(device=0):
    """(rsq-sequence mismatches, sqrt-sequence mismatches) vs sqrtf() over every float in [2^-100, 2^127)."""
    a, b = ctypes.c_ulonglong(), ctypes.c_ulonglong()
    lib = load_library()
    lib.j2p_sqrt_exhaustive.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_ulonglong), ctypes.POINTER(ctypes.c_ulonglong)]
    _check(lib.j2p_sqrt_exhaustive(device, ctypes.byref(a), ctypes.byref(b)))
    return a.value, b.value


def division_exhaustive(which, first=0, count=0, device=0):
    """exhaustive checks of the short division, pass 1 / 2 / 3 (include/jpeg2png_amd.h): (mismatches, first offenders)"""
    lib = load_library()
    lib.j2p_division_exhaustive.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint, ctypes.c_uint, ctypes.POINTER(ctypes.c_ulonglong)]
    rep = (ctypes.c_ulonglong * 9)()
    _check(lib.j2p_division_exhaustive(device, which, first, count, rep))
    return rep[0], [hex(v) for v in rep[1:] if v]


def tensor_path(w, nplane, dtype, stride_c, stride_y, stride_x, address):
    """which destination path the tensor kernel takes for the full-width rows of such an image: "generic", "planar" or
    "interleaved" (j2p_debug_tensor_path; no device needed).  dtype: a J2P_DTYPE_* code; strides in elements"""
    path = ctypes.c_int(-1)
    _check(load_library().j2p_debug_tensor_path(int(w), int(nplane), int(dtype), int(stride_c), int(stride_y), int(stride_x), int(address),
                                                ctypes.byref(path)))
    return TENSOR_PATHS[path.value]


def _c_specs(specs, dtypes):
    n = len(specs)
    if len(dtypes) != n:
        raise J2PError("outputs: one dtype per spec")
    return (_CResample * max(n, 1))(*[s if isinstance(s, _CResample) else _CResample(*[int(v) for v in s]) for s in specs]), \
        (ctypes.c_int * max(n, 1))(*[int(d) for d in dtypes])


def outputs_plan(width, height, specs, dtypes):
    """the work map of a multi-output call (j2p_debug_outputs_plan; no device needed) for specs — _CResample, or tuples (box_x,
    box_y, box_w, box_h, out_w, out_h, filter code) — of a width x height image and their tensors' J2P_DTYPE_* codes: a dict of
    tiles [(lanes, slots, rows)], grids [(tile columns, row groups)] and launch_of per output, and launches [(dtype,
    workgroups)].  J2PError for what the call refuses."""
    n = len(specs)
    cs, cd = _c_specs(specs, dtypes)
    tiles, grids, launch_of = (ctypes.c_uint * (3 * max(n, 1)))(), (ctypes.c_uint * (2 * max(n, 1)))(), (ctypes.c_uint * max(n, 1))()
    nlaunch, ldtype, lwg = ctypes.c_uint(0), (ctypes.c_int * 4)(), (ctypes.c_uint * 4)()
    _check(load_library().j2p_debug_outputs_plan(int(width), int(height), n, cs, cd, tiles, grids, launch_of, ctypes.byref(nlaunch), ldtype, lwg))
    return {"tiles": [tuple(tiles[3 * i:3 * i + 3]) for i in range(n)], "grids": [tuple(grids[2 * i:2 * i + 2]) for i in range(n)],
            "launch_of": list(launch_of[:n]), "launches": [(ldtype[k], lwg[k]) for k in range(nlaunch.value)]}


def outputs_workgroups(width, height, specs, dtypes, launch, first=0, count=None):
    """(output, tile column, row group) of workgroups [first, first + count) of sampling launch `launch` of that call, as the
    kernel's workgroups find them in their prefix table (j2p_debug_outputs_workgroups): an array [count, 3].  count None: to
    the end of the launch's grid."""
    cs, cd = _c_specs(specs, dtypes)
    if count is None:
        count = outputs_plan(width, height, specs, dtypes)["launches"][launch][1] - first
    out = np.zeros((int(count), 3), np.uint32)
    _check(load_library().j2p_debug_outputs_workgroups(int(width), int(height), len(specs), cs, cd, int(launch), int(first), int(count),
                                                       out.ctypes.data))
    return out


def job_layout():
    """(sizeof(j2p_job), offsetof(j2p_job, out_tensor)) as the loaded library was compiled"""
    size, off = ctypes.c_size_t(), ctypes.c_size_t()
    load_library().j2p_debug_job_layout(ctypes.byref(size), ctypes.byref(off))
    return size.value, off.value


def _torch():
    """torch, imported on first use: only tensor output needs it"""
    try:
        import torch
    except ImportError:
        raise J2PError("tensor output needs PyTorch (torch is not installed)") from None
    return torch


def _tensor_dtype(torch, dtype):
    codes = {torch.uint8: J2P_DTYPE_U8, torch.float16: J2P_DTYPE_F16, torch.bfloat16: J2P_DTYPE_BF16, torch.float32: J2P_DTYPE_F32}
    if dtype not in codes:
        raise J2PError(f"tensor output: dtype must be torch.uint8, float16, bfloat16 or float32, not {dtype!r}")
    return codes[dtype]


def _c_tensor(t, nplane, width, height, layout, scale, bias, device=None):
    """the j2p_tensor of the CUDA tensor t — (nplane, height, width) for layout "chw", (height, width, nplane) for "hwc", any
    view: the strides are the tensor's — with per-channel scale and bias (None: 1 and 0).  J2PError for anything else."""
    torch = _torch()
    if layout not in ("chw", "hwc"):
        raise J2PError(f"tensor output: layout must be 'chw' or 'hwc', not {layout!r}")
    if nplane not in (1, 3):
        raise J2PError("tensor output needs three planes (RGB) or one (greyscale)")
    if width is None or height is None or int(width) < 1 or int(height) < 1:
        raise J2PError("tensor output needs width and height")
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise J2PError("tensor output needs a torch.Tensor on a GPU")
    if device is not None and t.device.index != device:
        raise J2PError(f"tensor output: the tensor is on {t.device}, the solver on device {device}")
    shape = (nplane, int(height), int(width)) if layout == "chw" else (int(height), int(width), nplane)
    if tuple(t.shape) != shape:
        raise J2PError(f"tensor output: shape {tuple(t.shape)}, expected {shape} for layout {layout!r}")
    code = _tensor_dtype(torch, t.dtype)
    sc, sy, sx = t.stride() if layout == "chw" else (t.stride(2), t.stride(0), t.stride(1))
    if nplane == 1:
        sc = max(sc, 1)             # (a dimension of size 1 is never stepped over; torch may report any stride for it)
    if min(sc, sy, sx) < 1:
        raise J2PError(f"tensor output: strides (c, y, x) = ({sc}, {sy}, {sx}) must all be at least 1 (no expanded views)")

    def three(v, default, what):
        if v is None:
            return [default] * 3
        v = [float(x) for x in (v if isinstance(v, (list, tuple, np.ndarray)) else [v] * nplane)]
        if len(v) != nplane:
            raise J2PError(f"tensor output: {what} must have one value per plane")
        return v + [default] * (3 - nplane)

    scale, bias = three(scale, 1.0, "scale"), three(bias, 0.0, "bias")
    if code == J2P_DTYPE_U8 and (scale != [1.0] * 3 or bias != [0.0] * 3):
        raise J2PError("tensor output: uint8 elements are the 8-bit samples; scale and bias apply to float dtypes only")
    return _CTensor(t.data_ptr(), code, sc, sy, sx, (ctypes.c_float * 3)(*scale), (ctypes.c_float * 3)(*bias))


def _c_box(width, height, out_width, out_height, box):
    """(x, y, w, h, out_w, out_h) of the keywords out_width / out_height / box of Solver.to_tensor and Batch.submit for a width x
    height image: box (x, y, w, h) defaults to the whole image, a missing output size to the box's (a pure crop)"""
    if width is None or height is None or int(width) < 1 or int(height) < 1:
        raise J2PError("tensor output needs width and height")
    try:
        bx, by, bw, bh = (0, 0, int(width), int(height)) if box is None else (int(v) for v in box)
    except (TypeError, ValueError):
        raise J2PError("resize: box must be (x, y, width, height)") from None
    if bw < 1 or bh < 1:
        raise J2PError("resize: empty box")
    if bx < 0 or by < 0 or bx + bw > int(width) or by + bh > int(height):
        raise J2PError(f"resize: the box {(bx, by, bw, bh)} leaves the {int(width)} x {int(height)} image")
    ow, oh = bw if out_width is None else int(out_width), bh if out_height is None else int(out_height)
    if ow < 1 or oh < 1:
        raise J2PError("resize: empty output")
    return bx, by, bw, bh, ow, oh


def _c_resize(width, height, out_width, out_height, box):
    """the j2p_resize of those keywords: the area form, never larger than the box.  Refuses what the library refuses
    (j2p_resize_error), before anything is allocated."""
    bx, by, bw, bh, ow, oh = _c_box(width, height, out_width, out_height, box)
    if ow > bw or oh > bh:
        raise J2PError(f"resize: the output {ow} x {oh} is larger than the box {bw} x {bh} (enlarging is what zooming is for)")
    return _CResize(bx, by, bw, bh, ow, oh)


# filter= of Solver.to_tensor and Batch.submit: None and "area" are the area form (j2p_resize), the others J2P_FILTER_*
FILTERS = {"triangle": 1, "cubic": 2}
J2P_RESAMPLE_MAX_OUT = 65536


def _filter_code(filter):
    """None for the area form (filter None or "area"), otherwise the J2P_FILTER_* code"""
    if filter is None or filter == "area":
        return None
    if filter not in FILTERS:
        raise J2PError(f"resize: unknown filter {filter!r} (\"area\", \"triangle\" or \"cubic\")")
    return FILTERS[filter]


def _c_resample(width, height, out_width, out_height, box, code):
    """the j2p_resample of the same keywords with filter="triangle" / "cubic": the output may be larger than the box (up to
    J2P_RESAMPLE_MAX_OUT a side).  Refuses what the library refuses (j2p_resample_error)."""
    bx, by, bw, bh, ow, oh = _c_box(width, height, out_width, out_height, box)
    if ow > J2P_RESAMPLE_MAX_OUT or oh > J2P_RESAMPLE_MAX_OUT:
        raise J2PError(f"resize: the output {ow} x {oh} is larger than {J2P_RESAMPLE_MAX_OUT} a side")
    return _CResample(bx, by, bw, bh, ow, oh, code)


def _resize_spec(width, height, out_width, out_height, box, filter):
    """what the keywords out_width / out_height / box / filter of Solver.to_tensor and Batch.submit ask for: None (none of them is
    given), the j2p_resize of the area form (filter None or "area") or the j2p_resample of a filter"""
    code = _filter_code(filter)
    if code is not None:
        return _c_resample(width, height, out_width, out_height, box, code)
    if out_width is not None or out_height is not None or box is not None:
        return _c_resize(width, height, out_width, out_height, box)
    return None


def _tensor_to_fill(torch, out, dtype, layout, nplane, width, height, device):
    """the tensor Solver.to_tensor / to_tensors write into: the caller's `out` (whose dtype must be `dtype` where that is given), or
    a new one of `dtype` (default float32) in that layout on the device"""
    if out is not None:
        if dtype is not None and isinstance(out, torch.Tensor) and out.dtype != dtype:
            raise J2PError(f"tensor output: out is {out.dtype}, dtype says {dtype}")
        return out
    dtype = torch.float32 if dtype is None else dtype
    _tensor_dtype(torch, dtype)
    if width is None or height is None or int(width) < 1 or int(height) < 1:
        raise J2PError("tensor output needs width and height")
    if layout not in ("chw", "hwc"):
        raise J2PError(f"tensor output: layout must be 'chw' or 'hwc', not {layout!r}")
    shape = (nplane, int(height), int(width)) if layout == "chw" else (int(height), int(width), nplane)
    return torch.empty(shape, dtype=dtype, device=torch.device("cuda", device))


_OUTPUT_KEYS = {"out_width", "out_height", "box", "filter", "dtype", "layout", "scale", "bias"}


def _output_spec(width, height, o, tensor_key):
    """(j2p_resample, the dict) of one item of outputs= of Solver.to_tensors / Batch.submit: the keywords of to_tensor, filter
    required and "triangle" or "cubic" — the area form has no place in a list"""
    if not isinstance(o, dict):
        raise J2PError("outputs: every output is a dict")
    unknown = set(o) - _OUTPUT_KEYS - {tensor_key}
    if unknown:
        raise J2PError(f"outputs: unknown key(s) {sorted(unknown)}")
    code = _filter_code(o.get("filter"))
    if code is None:
        raise J2PError("outputs: every output names its filter, \"triangle\" or \"cubic\" (the area form is not part of a list)")
    return _c_resample(width, height, o.get("out_width"), o.get("out_height"), o.get("box"), code)


def _output_count(outputs):
    try:
        n = len(outputs)
    except TypeError:
        raise J2PError("outputs must be a list of dicts") from None
    if n < 1 or n > J2P_MAX_OUTPUTS:
        raise J2PError(f"outputs: {n} outputs (1 to {J2P_MAX_OUTPUTS} per call)")
    return n


def _sampling(subsampling):
    """(sx, sy) of a coefficient output: 1 or 2 each"""
    try:
        sx, sy = (int(v) for v in subsampling)
    except (TypeError, ValueError):
        raise J2PError("subsampling must be a pair (sx, sy)") from None
    if sx not in (1, 2) or sy not in (1, 2):
        raise J2PError(f"sampling factors {sx}x{sy} (1 and 2 are supported)")
    return sx, sy


def quality_tables(quality, ncomp):
    """libjpeg's quantisation tables for jpeg_set_quality(quality, TRUE): the base tables of Annex K scaled by the IJG rule and
    clamped to 1..255 -> ncomp (1 or 3) uint16[64] arrays in natural order, luma first, then the chroma table twice"""
    from .synth import quant_table
    if ncomp not in (1, 3):
        raise J2PError("quality_tables: three components or one")
    q = min(max(int(quality), 1), 100)
    return [quant_table("luma", q)] + [quant_table("chroma", q) for _ in range(ncomp - 1)]


def _c_jpeg(width, height, ncomp, quality, quant_tables, subsampling):
    """(j2p_jpeg, what it points into) of a file's keywords: quality or quant_tables, and subsampling=(sx, sy)"""
    if (quality is None) == (quant_tables is None):
        raise J2PError("jpeg: give quality or quant_tables, one of them")
    if width is None or height is None or int(width) < 1 or int(height) < 1:
        raise J2PError("jpeg: needs width and height")
    tables = quality_tables(quality, ncomp) if quant_tables is None else list(quant_tables)
    if len(tables) != ncomp:
        raise J2PError("jpeg: one quantisation table per plane")
    arrays = []
    for q in tables:
        q = np.asarray(q).reshape(-1)
        if q.size != 64:
            raise J2PError("jpeg: a quantisation table has 64 entries")
        if q.min() < 1 or q.max() > 255:
            raise J2PError("jpeg: quantisation steps must be 1..255 (the file is 8-bit baseline)")
        arrays.append(np.ascontiguousarray(q, dtype=np.uint16))
    sx, sy = _sampling(subsampling)
    spec = _CJpeg(int(width), int(height), sx, sy)
    for c in range(ncomp):
        spec.quant[c] = arrays[c].ctypes.data
    return spec, arrays


def _jpeg_bytes(call, guess):
    """what call(buffer address, capacity, size) leaves: once with room for `guess` bytes, again when the file is larger"""
    size = ctypes.c_size_t(0)
    for _ in range(2):
        buf = np.empty(max(int(guess), size.value), dtype=np.uint8)
        rc = call(buf.ctypes.data, buf.size, ctypes.byref(size))
        if rc != J2P_ESPACE:
            break
    _check(rc)
    return buf[:size.value].tobytes()


def _restart_options(optimize, progressive, restart_rows, restart_interval):
    """j2p_jpeg_options of a file's keywords: the record that every call which writes a JPEG file takes"""
    rows, interval = int(restart_rows or 0), int(restart_interval or 0)
    if rows < 0 or interval < 0:
        raise J2PError("jpeg: restart_rows and restart_interval are not negative")
    if rows > 0xffffffff or interval > 0xffffffff:       # (what the record cannot hold; the library refuses everything above 65535)
        raise J2PError("jpeg: restart_rows and restart_interval are above 65535")
    return _CJpegOptions(J2P_JPEG_OPTIMIZE if optimize and not progressive else 0, 1 if progressive else 0, interval, rows)


def _restart_plan(width, height, ncomp, subsampling=(1, 1), progressive=False, restart_rows=0, restart_interval=0):
    """test hook: the restart intervals of the file these keywords describe, from the library's host arithmetic alone (j2p_debug_restart_plan; no
    device): per scan a dict of units, units_per_row, interval, intervals and dri (a DRI segment precedes its SOS)"""
    lib = load_library()
    sx, sy = _sampling(subsampling)
    options = _CJpegOptions(0, 1 if progressive else 0, int(restart_interval or 0), int(restart_rows or 0))
    plan = _CRestartPlan()
    _check(lib.j2p_debug_restart_plan(int(width), int(height), int(ncomp), sx, sy, ctypes.byref(options), ctypes.byref(plan)))
    return [{"units": k.units, "units_per_row": k.units_per_row, "interval": k.interval, "intervals": k.intervals, "dri": bool(k.dri)}
            for k in plan.scan[:plan.nscans]]


def entropy_encode(coefficients, width, height, quant_tables, subsampling=(1, 1), device=0, optimize=False, stats=False, progressive=False,
                   restart_rows=0, restart_interval=0):
    """a baseline JPEG file (bytes) from quantised coefficients, entropy-coded on the GPU (j2p_entropy_encode_opt): coefficients is a
    list of 1 or 3 int16 arrays [blocks_h, blocks_w, 64] in natural order — component 0's grid ceil(height / 8) x ceil(width / 8),
    the others' ceil of that over subsampling=(sx, sy) — every value in [-1023, 1023]; quant_tables: one per component, steps
    1..255, the third equal to the second.  Byte for byte what libjpeg's jpeg_write_coefficients writes with its defaults.
    optimize=True: with Huffman tables made for these coefficients from symbol counts taken on the GPU (J2P_JPEG_OPTIMIZE) — byte
    for byte libjpeg's file with optimize_coding (IJG 9d and later).  stats=True: (file, dict of the device's counts dc0, ac0, dc1,
    ac1 — 256 each — scan_bits and stuffed_bytes).
    progressive=True: the progressive file of libjpeg's jpeg_simple_progression() (include/jpeg2png_amd.h:
    "The progressive JPEG file"), every scan with tables of its own — optimize= changes nothing about it.  stats=True then gives
    (file, list of one dict per scan: components, ss, se, ah, al, tables — {(class << 4) | slot: 256 counts}, in DHT order —, bits,
    stuffed_bytes and eob_runs).
    restart_rows=R or restart_interval=N: the same file with restart intervals of R rows of MCUs (of blocks, in a scan of one
    component) or of N MCUs (blocks) — libjpeg's restart_in_rows and restart_interval (include/jpeg2png_amd.h:
    "Restart intervals").  stats=True then gives the dict, or each scan's dict, one more entry: "restart", a dict of interval,
    intervals, padding_bits and markers as taken on the device (for a baseline file under the dict's own key "restart")."""
    lib = load_library()
    n = len(coefficients)
    if n not in (1, 3):
        raise J2PError("jpeg: three components or one")
    spec, _held = _c_jpeg(width, height, n, None, quant_tables, subsampling)
    bw, bh = -(-int(width) // 8), -(-int(height) // 8)
    sx, sy = (spec.sub_w, spec.sub_h) if n == 3 else (1, 1)
    arrays = []
    for c, a in enumerate(coefficients):
        grid = (bh, bw, 64) if c == 0 else (-(-bh // sy), -(-bw // sx), 64)
        a = np.ascontiguousarray(a, dtype=np.int16)
        if a.shape != grid:
            raise J2PError(f"jpeg: component {c} has shape {a.shape}, its grid is {grid}")
        arrays.append(a)
    ptrs = (ctypes.c_void_p * 3)(*[a.ctypes.data for a in arrays])
    total = sum(a.size for a in arrays)
    options = _restart_options(optimize, progressive, restart_rows, restart_interval)
    restarts = bool(options.restart_interval or options.restart_in_rows)
    # (a record the caller does not ask for stays NULL: without stats and optimize= the baseline coder counts nothing)
    st = _CEncodeStats() if stats and not progressive else None
    ps = _CProgressiveStats() if stats and progressive else None
    rs = _CRestartStats() if stats and restarts else None
    ref = lambda record: None if record is None else ctypes.byref(record)
    file = _jpeg_bytes(lambda out, cap, size: lib.j2p_entropy_encode_opt(int(device), ctypes.byref(spec), ptrs, n, out, cap, size, ctypes.byref(options),
                                                                         ref(st), ref(ps), ref(rs)),
                       4096 + total // 4 + (total // 32 if restarts else 0))      # (room for markers and pads only where there are any)
    if not stats:
        return file
    restart = [{"interval": k.interval, "intervals": k.intervals, "padding_bits": k.padding_bits, "markers": k.markers}
               for k in (rs.scan[:rs.nscans] if restarts else ())]
    if progressive:
        scans = [{"components": tuple(k.comp[:k.ncomp]), "ss": k.ss, "se": k.se, "ah": k.ah, "al": k.al,
                  "tables": {k.table[t]: list(k.counts[t]) for t in range(k.ntables)}, "bits": k.bits, "stuffed_bytes": k.stuffed_bytes,
                  "eob_runs": k.eob_runs} for k in ps.scan[:ps.nscans]]
        assert not restarts or len(restart) == len(scans)       # (the coder reports every scan's intervals)
        for scan, r in zip(scans, restart):
            scan["restart"] = r
        return file, scans
    scan = {"dc0": list(st.dc0), "ac0": list(st.ac0), "dc1": list(st.dc1), "ac1": list(st.ac1), "scan_bits": st.scan_bits,
            "stuffed_bytes": st.stuffed_bytes}
    if restarts:
        scan["restart"] = restart[0]
    return file, scan


def _c_png(width, height, bits=8, filter=None, block_bytes=0, idat_bytes=0):
    """j2p_png of a file's keywords: filter None or "adaptive" (chosen per row), 0..4 or "none", "sub", "up", "average", "paeth"
    (that one for every row); block_bytes, idat_bytes: 0 for the defaults"""
    if width is None or height is None or int(width) < 1 or int(height) < 1:
        raise J2PError("png: needs width and height")
    if isinstance(filter, str) or filter is None:
        if filter not in PNG_FILTERS:
            raise J2PError(f"png: unknown filter {filter!r}")
        filter = PNG_FILTERS[filter]
    return _CPng(int(width), int(height), int(bits), int(filter), int(block_bytes), int(idat_bytes))


def png_encode(samples, bits=8, filter=None, block_bytes=0, idat_bytes=0, device=0, stats=False):
    """a PNG file (bytes) from samples, filtered and deflated on the GPU (j2p_png_encode): samples is [height, width, 3] (RGB) or
    [height, width] (greyscale), uint8 for bits=8 and uint16 for bits=16 (written high byte first, as PNG wants them).  filter: None
    chooses per row by libpng's heuristic, 0..4 (or "none", "sub", "up", "average", "paeth") uses one for every row.  block_bytes: the
    filtered bytes per deflate block, idat_bytes: the data bytes per IDAT chunk; 0 for the defaults, 16..2^24 otherwise.  Every byte
    is defined in include/jpeg2png_amd.h, "The PNG file".  stats=True: (file, dict of rows per filter type, blocks, literals,
    matches, stream_bytes and adler)."""
    lib = load_library()
    a = np.asarray(samples)
    if int(bits) not in (8, 16) or a.dtype != (np.uint8 if int(bits) == 8 else np.uint16):
        raise J2PError("png: uint8 samples with bits=8, uint16 samples with bits=16")
    if a.ndim == 2:
        channels = 1
    elif a.ndim == 3 and a.shape[2] in (1, 3):
        channels = a.shape[2]
    else:
        raise J2PError(f"png: samples of shape {a.shape}: [height, width, 3] or [height, width]")
    height, width = a.shape[:2]
    a = np.ascontiguousarray(a.astype(">u2") if int(bits) == 16 else a)
    spec = _c_png(width, height, bits, filter, block_bytes, idat_bytes)
    st = _CPngStats()
    file = _jpeg_bytes(lambda out, cap, size: lib.j2p_png_encode(int(device), ctypes.byref(spec), a.ctypes.data, channels, out, cap, size,
                                                                 ctypes.byref(st) if stats else None), 4096 + a.nbytes * 3 // 4)
    if not stats:
        return file
    return file, {"rows": list(st.rows), "blocks": st.blocks, "literals": st.literals, "matches": st.matches, "stream_bytes": st.stream_bytes,
                  "adler": st.adler}


def _file_bytes(data):
    """(address, size, what keeps it alive) of a JPEG file given as bytes-like host data, or as a 1-D uint8 torch tensor in device
    memory, which the library reads in place"""
    if hasattr(data, "data_ptr"):
        if str(data.dtype) != "torch.uint8" or data.dim() != 1 or not data.is_contiguous():
            raise J2PError("a file in a tensor is a contiguous 1-D uint8 tensor")
        return data.data_ptr(), int(data.numel()), data
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    return a.ctypes.data, a.size, a


def _jpeg_info_dict(info):
    comps = [{"id": k.id, "h_samp_factor": k.h_samp_factor, "v_samp_factor": k.v_samp_factor, "blocks_w": k.blocks_w, "blocks_h": k.blocks_h,
              "w": k.blocks_w * 8, "h": k.blocks_h * 8, "w_samp": k.w_samp, "h_samp": k.h_samp, "quant_slot": k.quant_slot, "dc_slot": k.dc_slot,
              "ac_slot": k.ac_slot, "quant_table": np.array(k.quant, dtype=np.uint16)} for k in info.comp[:info.ncomp]]
    return {"width": info.width, "height": info.height, "extended": bool(info.extended), "components": comps, "mcus_w": info.mcus_w,
            "mcus_h": info.mcus_h, "blocks_per_mcu": info.blocks_per_mcu, "restart_interval": info.restart_interval, "intervals": info.intervals,
            "scan_begin": info.scan_begin, "scan_end": info.scan_end}


def jpeg_parse(data, progressive=False):
    """j2p_jpeg_parse: the marker segments of a baseline JPEG file (host bytes), read by the library's C parser without touching a
    device -> dict of width, height, components (per component id, sampling factors, the block grid, table slots, quant_table),
    the MCU grid, restart_interval, intervals and the byte range of the entropy-coded data.  J2PError with code J2P_EFORMAT
    (damaged) or J2P_ENOTSUP (valid, not read: progressive, arithmetic, 12-bit, several scans, ...).
    progressive=True: j2p_jpeg_parse_scans — progressive files are read too, and the dict gains "progressive" and "scans": per scan
    its components (frame indices), ss, se, ah, al, dc_slots, ac_slots, restart_interval, intervals, begin, end."""
    addr, size, _keep = _file_bytes(bytes(data))
    info = _CJpegInfo()
    if progressive:
        scans = _CJpegScans()
        _check(load_library().j2p_jpeg_parse_scans(addr, size, ctypes.byref(info), ctypes.byref(scans)))
        out = _jpeg_info_dict(info)
        out["progressive"] = bool(scans.progressive)
        out["scans"] = [{"components": list(q.comp[:q.ncomp]), "ss": q.ss, "se": q.se, "ah": q.ah, "al": q.al,
                         "dc_slots": list(q.dc_slot[:q.ncomp]), "ac_slots": list(q.ac_slot[:q.ncomp]), "restart_interval": q.restart_interval,
                         "intervals": q.intervals, "begin": q.begin, "end": q.end} for q in scans.scan[:scans.nscans]]
        return out
    _check(load_library().j2p_jpeg_parse(addr, size, ctypes.byref(info)))
    return _jpeg_info_dict(info)


def jpeg_orientation_c(data):
    """j2p_jpeg_orientation: the EXIF Orientation tag of a JPEG file (host bytes), 1..8, read by the library's C reader; 1 where the
    file has none that counts.  jpeg_orientation is its pure-Python twin."""
    addr, size, _keep = _file_bytes(bytes(data))
    o = ctypes.c_uint(0)
    _check(load_library().j2p_jpeg_orientation(addr, size, ctypes.byref(o)))
    return o.value


def upright_size(orientation, width, height):
    """(width, height) of the upright image of a width x height source under EXIF orientation 1..8"""
    return (int(height), int(width)) if int(orientation) >= 5 else (int(width), int(height))


def entropy_decode(data, device=0, subsequence_bits=0, stats=False, progressive=False):
    """the quantised coefficients of a baseline JPEG file, Huffman-decoded on the GPU (j2p_entropy_decode): a list of 1 or 3 int16
    arrays [blocks_h, blocks_w, 64] in natural order — what libjpeg's jpeg_read_coefficients delivers.  data: bytes, or a 1-D uint8
    torch tensor on the device, read in place.  subsequence_bits: 0 for the default, or J2P_DECODE_SUBSEQUENCE_MIN..MAX (the result
    does not depend on it).  stats=True: (arrays, dict of subsequences, intervals, rounds, recomputed per round, data_bytes).
    J2PError with code J2P_EFORMAT for a damaged file, J2P_ENOTSUP for a valid one of another kind."""
    lib = load_library()
    addr, size, _keep = _file_bytes(data)
    info = _CJpegInfo()
    # (the grids' sizes are needed before the call, so the marker segments are read here too — microseconds of host work; a device
    # tensor's from a copy)
    parsed = jpeg_parse(data.cpu().numpy().tobytes() if hasattr(data, "data_ptr") else data, progressive=progressive)
    arrays = [np.full((k["blocks_h"], k["blocks_w"], 64), 0, dtype=np.int16) for k in parsed["components"]]
    ptrs = (ctypes.c_void_p * 3)(*[a.ctypes.data for a in arrays])
    if progressive:
        # j2p_entropy_decode_scans: progressive files too; stats=True: (arrays, dict of j2p_scans_stats)
        ss = _CScansStats()
        _check(lib.j2p_entropy_decode_scans(int(device), addr, size, ptrs, None, ctypes.byref(info), int(subsequence_bits), ctypes.byref(ss)))
        return (arrays, {name: getattr(ss, name) for name, _ in _CScansStats._fields_}) if stats else arrays
    st = _CDecodeStats()
    _check(lib.j2p_entropy_decode_ex(int(device), addr, size, ptrs, None, ctypes.byref(info), int(subsequence_bits), ctypes.byref(st)))
    if not stats:
        return arrays
    return arrays, {"subsequences": st.subsequences, "intervals": st.intervals, "rounds": st.rounds,
                    "recomputed": list(st.recomputed)[:min(st.rounds, J2P_DECODE_STATS_ROUNDS)], "data_bytes": st.data_bytes, "decode_ms": st.decode_ms}


class Solver:
    """Device-resident working set of one compute() call (include/jpeg2png_amd.h)."""

    def __init__(self, planes, weight, pweight, iterations, device=0, stream=None, band=None,
                 band_local_arrays=False):
        lib = load_library()
        self._lib = lib
        self._h = None
        self.nch = len(planes)
        keep = []
        cpl = (_CPlane * self.nch)()
        for i, p in enumerate(planes):
            d = np.ascontiguousarray(p.data, dtype=np.int16)
            q = np.ascontiguousarray(p.quant_table, dtype=np.uint16)
            f = None if p.fdata is None else np.ascontiguousarray(p.fdata, dtype=np.float32)
            keep += [d, q, f]
            cpl[i] = _CPlane(p.w, p.h, p.w_samp, p.h_samp, d.ctypes.data, None if f is None else f.ctypes.data,
                             q.ctypes.data)
        pw = (ctypes.c_float * self.nch)(*[float(x) for x in pweight])
        b = _CBand(0, 0) if band is None else _CBand(int(band[0]), int(band[1]))
        h = ctypes.c_void_p()
        _check(lib.j2p_solver_create(ctypes.byref(h), device, stream, self.nch, cpl, float(weight), pw,
                                     int(iterations), b, 1 if band_local_arrays else 0))
        del keep
        self._geom = [(int(p.w), int(p.h)) for p in planes]
        self._adopt(h, device)

    def _adopt(self, h, device):
        """the rest of construction, once the C solver exists"""
        lib = self._lib
        self._h = h
        self.device = int(device)
        W, H = ctypes.c_uint(), ctypes.c_uint()
        _check(lib.j2p_solver_canvas(h, ctypes.byref(W), ctypes.byref(H)))
        self.W, self.H = W.value, H.value
        r0, r1 = ctypes.c_uint(), ctypes.c_uint()
        _check(lib.j2p_solver_band(h, ctypes.byref(r0), ctypes.byref(r1)))
        self.row_begin, self.row_end = r0.value, r1.value

    @classmethod
    def from_samples(cls, samples, planes, weight, pweight, iterations, device=0, stream=None, quant=None):
        """A solver made from decoded 8-bit planes instead of coefficients (j2p_solver_create_from_samples): what a hardware JPEG
        decoder, PyAV (`yuvj420p`) or libjpeg's raw-data mode hands over.  planes: Plane-likes with w, h, w_samp, h_samp and
        quant_table, data=None (jpeg_header(...)["planes"] are such).  samples: one entry per plane — a 2-D torch.uint8 tensor
        (on the solver's GPU: read in place; on the CPU: served like an array) or a 2-D numpy uint8 array, any strides >= 1 —
        of (rows, columns) <= (plane.h, plane.w); the last row and column are replicated up to the plane's size.  The
        coefficients are recomputed on the device (the header states the definition and when the file's are recovered
        exactly); from there on the solver is the one Solver(planes with those coefficients) is.
        For tensors on the GPU the solver's stream is made to wait for torch's current stream before the kernel reads them;
        when the call returns they have been read.
        quant="estimate": the tables are read off the samples — one histogram launch per channel (samples_histogram) and the
        estimator (estimate_quant_table; channel 0 against the luminance base table, the others against the chrominance one) —
        and the call proceeds with them as it does with given ones.  The planes' quant_table may then be None (in every plane;
        tables given in every plane are ignored).  Solver.estimated_tables keeps the (table, determined, quality) triples;
        it is None for every other solver."""
        self = cls.__new__(cls)
        lib = load_library()
        self._lib = lib
        self._h = None
        self.nch = len(planes)
        self.estimated_tables = None
        if len(samples) != self.nch:
            raise J2PError(f"from_samples: {len(samples)} sample arrays for {self.nch} planes")
        estimate = _want_estimate(quant, planes, "from_samples")
        for i, p in enumerate(planes):
            if getattr(p, "data", None) is not None or getattr(p, "fdata", None) is not None:
                raise J2PError(f"from_samples: plane {i} carries data / fdata; a solver made from samples takes neither")
        csm, held, on_gpu = _c_samples(samples, device)
        if on_gpu:
            # a stream of torch's, so that it can be made to wait for torch's current one (the library synchronises it before
            # it returns); it lives as long as the solver, which launches on it
            torch = _torch()
            dev = torch.device("cuda", int(device))
            ours = torch.cuda.Stream(device=dev) if stream is None else torch.cuda.ExternalStream(int(stream), device=dev)
            ours.wait_stream(torch.cuda.current_stream(dev))
            self._torch_stream = ours
            stream = ours.cuda_stream
        tables = [p.quant_table for p in planes]
        if estimate:
            # (on the solver's stream, which waits for the samples' producer; each call returns with its channel read)
            self.estimated_tables = [estimate_quant_table(samples_histogram(a, device, stream)[0], chroma=c > 0) for c, a in enumerate(samples)]
            tables = [t for t, _, _ in self.estimated_tables]
        cpl = (_CPlane * self.nch)()
        keep = []
        for i, p in enumerate(planes):
            q = np.ascontiguousarray(tables[i], dtype=np.uint16)
            keep.append(q)
            cpl[i] = _CPlane(p.w, p.h, p.w_samp, p.h_samp, None, None, q.ctypes.data)
        pw = (ctypes.c_float * self.nch)(*[float(x) for x in pweight])
        h = ctypes.c_void_p()
        _check(lib.j2p_solver_create_from_samples(ctypes.byref(h), int(device), stream, self.nch, cpl, csm, float(weight), pw, int(iterations)))
        del keep, held
        self._geom = [(int(p.w), int(p.h)) for p in planes]
        self._adopt(h, device)
        return self

    @classmethod
    def from_jpeg(cls, data, weight, pweight, iterations, device=0, stream=None, upright=False, progressive=False):
        """A solver made from a baseline JPEG FILE (j2p_solver_create_from_jpeg): the file's entropy-coded data is Huffman-decoded
        on the GPU straight into the solver's resident coefficients — no libjpeg, and the file's true coefficients at every
        quality.  data: bytes, or a 1-D uint8 torch tensor (on the solver's GPU: the scan is read in place).  pweight: one per
        component of the file (1 or 3).  From there on the solver is the one Solver(planes with those coefficients) is.
        self.jpeg holds what jpeg_parse returns.  J2PError with code J2P_EFORMAT / J2P_ENOTSUP for files that are refused.
        upright=True: the file's EXIF Orientation tag (jpeg_orientation) is set on the solver with the file's size
        (set_orientation): every output form then delivers the upright image.
        progressive=True: j2p_solver_create_from_jpeg_scans — a progressive file's scans are all decoded on the GPU too."""
        self = cls.__new__(cls)
        lib = load_library()
        self._lib = lib
        self._h = None
        addr, size, held = _file_bytes(data)
        # (the marker segments first, on the host: a refused file and a pweight list of the wrong length cost no GPU work)
        head = jpeg_parse(data.cpu().numpy().tobytes() if hasattr(data, "data_ptr") else data, progressive=progressive)
        if len(pweight) != len(head["components"]):
            raise J2PError(f"from_jpeg: {len(pweight)} pweights for a file of {len(head['components'])} components")
        if hasattr(data, "data_ptr") and data.is_cuda:
            torch = _torch()
            dev = torch.device("cuda", int(device))
            ours = torch.cuda.Stream(device=dev) if stream is None else torch.cuda.ExternalStream(int(stream), device=dev)
            ours.wait_stream(torch.cuda.current_stream(dev))
            ours.synchronize()          # (the host parses a copy of the file before anything is queued)
            self._torch_stream = ours
            stream = ours.cuda_stream
        pw = (ctypes.c_float * len(pweight))(*[float(x) for x in pweight])
        info = _CJpegInfo()
        h = ctypes.c_void_p()
        _check((lib.j2p_solver_create_from_jpeg_scans if progressive else lib.j2p_solver_create_from_jpeg)(ctypes.byref(h), int(device), stream, addr, size, float(weight), pw, int(iterations), ctypes.byref(info)))
        del held
        self.jpeg = head if progressive else _jpeg_info_dict(info)      # (with the scans: what jpeg_parse(progressive=True) returned)
        self.nch = info.ncomp
        self._geom = [(k["w"], k["h"]) for k in self.jpeg["components"]]
        self._adopt(h, device)
        if upright:
            self.set_orientation(jpeg_orientation(data.cpu().numpy().tobytes() if hasattr(data, "data_ptr") else data),
                                 self.jpeg["width"], self.jpeg["height"])
        return self

    def set_orientation(self, orientation, width, height):
        """EXIF orientation 1..8 of a source image of width x height pixels (j2p_solver_set_orientation): from now on every output
        form — to_tensor(s), coefficients, to_jpeg, to_png, the sample forms — is that form of the UPRIGHT image (the header states
        the permutation), whose width, height, boxes and specs the calls then take: height x width for orientations 5..8.  1 is
        none.  download() and plane_ptr() stay the solver's canvas.  Whole-canvas solvers only."""
        _check(self._lib.j2p_solver_set_orientation(self._h, int(orientation), int(width), int(height)))

    @property
    def orientation(self):
        """the orientation set_orientation left (1: none)"""
        if not hasattr(self._lib, "j2p_solver_orientation"):        # (an earlier commit's build: nothing to set)
            return 1
        o = ctypes.c_uint()
        _check(self._lib.j2p_solver_orientation(self._h, ctypes.byref(o), None, None))
        return o.value

    def _upright_canvas(self):
        """(W, H) of the canvas the output forms see: the solver's, or for an oriented solver the upright image rounded up to 16"""
        if not hasattr(self._lib, "j2p_solver_orientation"):
            return None
        o, w, h = ctypes.c_uint(), ctypes.c_uint(), ctypes.c_uint()
        _check(self._lib.j2p_solver_orientation(self._h, ctypes.byref(o), ctypes.byref(w), ctypes.byref(h)))
        if o.value <= 1:
            return None
        uw, uh = upright_size(o.value, w.value, h.value)
        return -(-uw // 16) * 16, -(-uh // 16) * 16

    def upright_bytes(self):
        """bytes of the block of upright planes an oriented solver's output calls permute into (j2p_solver_upright_bytes): 0 until
        the first such call, unchanged by a second one"""
        n = ctypes.c_size_t()
        _check(self._lib.j2p_solver_upright_bytes(self._h, ctypes.byref(n)))
        return n.value

    def download_coefficients(self, c):
        """diagnostics: the quantised coefficients channel c holds, int16 [block rows, blocks per row, 64] (j2p_solver_download_coefficients)"""
        geom = getattr(self, "_geom", None)
        if geom is None or (self.row_begin, self.row_end) != (0, self.H):
            raise J2PError("download_coefficients: whole-canvas solvers made by Solver(...) or Solver.from_samples(...) only")
        if not 0 <= int(c) < self.nch:
            raise J2PError(f"download_coefficients: no channel {c}")
        w, h = geom[int(c)]
        out = np.empty((h // 8, w // 8, 64), dtype=np.int16)
        _check(self._lib.j2p_solver_download_coefficients(self._h, int(c), out.ctypes.data))
        return out

    def clipped_samples(self, c):
        """how many of channel c's samples were 0 or 255 (a solver made by from_samples): where not 0, the file's coefficients
        are not guaranteed to have been recovered (j2p_solver_clipped_samples)"""
        n = ctypes.c_ulonglong()
        _check(self._lib.j2p_solver_clipped_samples(self._h, int(c), ctypes.byref(n)))
        return n.value

    def close(self):
        if getattr(self, "_h", None) and not getattr(self, "_borrowed", False):
            self._lib.j2p_solver_destroy(self._h)
        self._h = None
        self._torch_stream = None       # (after the solver, which synchronised it)

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def reset(self):
        _check(self._lib.j2p_solver_reset(self._h))

    def run(self, n, log=False):
        """n iterations of the loop compute.c:427-453; returns [n,4] (objective, prob_dist, tv, tv2) if log."""
        if not log:
            _check(self._lib.j2p_solver_run(self._h, n, None))
            return None
        rows = (_CLogRow * max(n, 1))()
        _check(self._lib.j2p_solver_run(self._h, n, rows))
        return np.array([[r.objective, r.prob_dist, r.tv, r.tv2] for r in rows[:n]], dtype=np.float64).reshape(n, 4)

    def phase_gradient(self):
        _check(self._lib.j2p_solver_phase_gradient(self._h))

    def phase_project(self):
        _check(self._lib.j2p_solver_phase_project(self._h))

    def phase_gradient_part(self, part, stream=None):
        """part 1 = interior segments (no halo needed), 2 = the band's first/last segment (optionally
        on another hipStream_t); follow part 2 with phase_rowsums() once the solver's stream waits for it."""
        _check(self._lib.j2p_solver_phase_gradient_part(self._h, int(part), stream))

    def phase_project_part(self, part):
        """part 1 = norm + the band's first/last block rows (the rows the neighbours need), 2 = the rest"""
        _check(self._lib.j2p_solver_phase_project_part(self._h, int(part)))

    def set_logging(self, on=True):
        """band solvers: the phase calls also leave the band's tv / tv2 / prob sums in exchange_info().log_local"""
        _check(self._lib.j2p_solver_set_logging(self._h, 1 if on else 0))

    def phase_rowsums(self):
        _check(self._lib.j2p_solver_phase_rowsums(self._h))

    def commit_initial_halo(self):
        _check(self._lib.j2p_solver_commit_initial_halo(self._h))

    def exchange_info(self):
        e = _CExchange()
        _check(self._lib.j2p_solver_exchange_info(self._h, ctypes.byref(e)))
        return e

    def norm_ptr(self):
        """device address of the solver's [channel] float norms (j2p_solver_norm_ptr)"""
        p = ctypes.c_void_p()
        self._lib.j2p_solver_norm_ptr.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
        _check(self._lib.j2p_solver_norm_ptr(self._h, ctypes.byref(p)))
        return p.value

    def norm_from_bands(self, bands):
        """between the two phases: ||g|| from the level-1 sums of the bands [(device address, first tile row, tile rows), ...],
        in the order given, into this solver's norm (j2p_solver_norm_from_bands with nout = 0)"""
        n = len(bands)
        rs = (ctypes.c_void_p * n)(*[int(b[0]) for b in bands])
        first = (ctypes.c_uint * n)(*[int(b[1]) for b in bands])
        count = (ctypes.c_uint * n)(*[int(b[2]) for b in bands])
        self._lib.j2p_solver_norm_from_bands.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p,
                                                         ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p]
        _check(self._lib.j2p_solver_norm_from_bands(self._h, n, rs, first, count, 0, None))

    def debug_partials(self):
        """diagnostics: (device address of the strip partials, float64 [channel][local tile row][strip]; strips per tile
        row; local tile rows; rows per tile row) — j2p_solver_debug_partials"""
        p, ntx, ntr, rpw = ctypes.c_void_p(), ctypes.c_uint(), ctypes.c_uint(), ctypes.c_uint()
        _check(self._lib.j2p_solver_debug_partials(self._h, ctypes.byref(p), ctypes.byref(ntx), ctypes.byref(ntr), ctypes.byref(rpw)))
        return p.value, ntx.value, ntr.value, rpw.value

    def sync(self):
        _check(self._lib.j2p_solver_sync(self._h))

    def download(self, c):
        out = np.empty((self.row_end - self.row_begin, self.W), dtype=np.float32)
        _check(self._lib.j2p_solver_download(self._h, c, out.ctypes.data))
        return out

    def coefficients(self, c, quant_table, blocks_w=None, blocks_h=None, subsampling=(1, 1)):
        """channel c's current iterate as quantised DCT coefficients for a JPEG writer (j2p_planes_rows_to_coefficients_sub):
        dct8x8s of every 8x8 block, divided by quant_table (64 non-zero steps, natural order), rounded to nearest even,
        clamped to +-1023 -> int16 [blocks_h, blocks_w, 64], natural order.  Default: the whole canvas; a band solver
        gives its own block rows.
        subsampling=(sx, sy), each 1 or 2: of the plane at 1/sx x 1/sy of the resolution,
        every sample the mean of its sy x sx canvas values; a grid that overhangs the canvas replicates the canvas's last
        column / row (every block must start inside).  Default grid: ceil(canvas blocks / (sx, sy))."""
        q = np.ascontiguousarray(quant_table, dtype=np.uint16).reshape(-1)
        if q.size != 64:
            raise J2PError("quant_table must have 64 entries")
        sx, sy = _sampling(subsampling)
        upright = self._upright_canvas()
        # a band's block rows: those that start in it (cuts are multiples of 16 rows); an oriented solver: the upright canvas's
        r0, r1 = (-(-self.row_begin // (8 * sy)), -(-self.row_end // (8 * sy))) if upright is None else (0, -(-upright[1] // (8 * sy)))
        bw = -(-(self.W if upright is None else upright[0]) // (8 * sx)) if blocks_w is None else int(blocks_w)
        bh = (r1 - r0) if blocks_h is None else int(blocks_h)
        if bw < 0 or bh < 0:
            raise J2PError("blocks_w / blocks_h must not be negative")
        out = np.empty((bh, bw, 64), dtype=np.int16)
        ref = _CPlaneRef(self._h, int(c))
        if upright is not None:         # (the rows forms take no oriented solver)
            _check(self._lib.j2p_planes_to_coefficients_sub(ctypes.byref(ref), sx, sy, bw, bh, q.ctypes.data, out.ctypes.data))
            return out
        _check(self._lib.j2p_planes_rows_to_coefficients_sub(ctypes.byref(ref), sx, sy, bw, r0, r0 + bh, q.ctypes.data, out.ctypes.data))
        return out

    def to_jpeg(self, width, height, quality=None, quant_tables=None, subsampling=(1, 1), others=(), optimize=False, progressive=False,
                restart_rows=0, restart_interval=0):
        """the current iterate as a complete baseline JPEG file (bytes), quantised AND entropy-coded on the GPU (j2p_planes_to_jpeg_opt):
        only the file comes down.  width x height: the image, cropped from the canvas's top left corner.  quality: libjpeg's
        tables for it (quality_tables), or quant_tables: one 64-entry table per component, steps 1..255, natural order, the third
        equal to the second.  subsampling=(sx, sy), 1 or 2 each: the sampling of components 1 and 2.  A solver of three channels
        gives a colour file, one of one channel a greyscale file; others=(solver, solver): this solver's channel 0 and the
        channel 0 of two more solvers (the separate solves of `-s`) give a colour file.  Whole-canvas solvers only.  Byte for
        byte what libjpeg's jpeg_write_coefficients writes from Solver.coefficients() with its defaults.  optimize=True: with
        Huffman tables made for the image, as entropy_encode(optimize=True) makes them — the same
        coefficients in fewer bytes, for one more wait on the way.  progressive=True: the progressive file, as
        entropy_encode(progressive=True) writes it; optimize= changes nothing about it.
        restart_rows=R or restart_interval=N: any of the three with restart intervals, as entropy_encode(restart_rows=,
        restart_interval=) writes them."""
        solvers = [self] + list(others)
        if len(solvers) not in (1, 3):
            raise J2PError("jpeg: others= takes the two other solvers of a colour file")
        n = 3 if len(solvers) == 3 else self.nch
        refs = (_CPlaneRef * 3)()
        for c in range(n):
            refs[c] = _CPlaneRef(solvers[c]._h, 0) if len(solvers) == 3 else _CPlaneRef(self._h, c)
        spec, _held = _c_jpeg(width, height, n, quality, quant_tables, subsampling)
        guess = 4096 + int(width) * int(height) * n // 4
        options = _restart_options(optimize, progressive, restart_rows, restart_interval)
        if options.restart_interval or options.restart_in_rows:     # (room for markers and pads only where there are any)
            guess += guess // 8
        return _jpeg_bytes(lambda out, cap, size: self._lib.j2p_planes_to_jpeg_opt(refs, n, ctypes.byref(spec), out, cap, size, ctypes.byref(options)), guess)

    def to_png(self, width, height, bits=8, filter=None, others=(), block_bytes=0, idat_bytes=0):
        """the current iterate as a complete PNG file (bytes), converted to samples, filtered AND deflated on the GPU
        (j2p_planes_to_png): only the file comes down.  width x height: the image, cropped from the canvas's top left corner; bits 8
        or 16.  A solver of three channels gives an RGB file, one of one channel a greyscale file; others=(solver, solver): this
        solver's channel 0 and the channel 0 of two more solvers (the separate solves of `-s`) give an RGB file.  Whole-canvas
        solvers only.  The pixels are the bytes of j2p_planes_to_rgb / j2p_planes_to_grey; filter, block_bytes and idat_bytes as for
        png_encode, whose file of those bytes this is."""
        solvers = [self] + list(others)
        if len(solvers) not in (1, 3):
            raise J2PError("png: others= takes the two other solvers of an RGB file")
        n = 3 if len(solvers) == 3 else self.nch
        refs = (_CPlaneRef * 3)()
        for c in range(min(n, 3)):
            refs[c] = _CPlaneRef(solvers[c]._h, 0) if len(solvers) == 3 else _CPlaneRef(self._h, c)
        spec = _c_png(width, height, bits, filter, block_bytes, idat_bytes)
        guess = 4096 + int(width) * int(height) * n * (int(bits) // 8) * 3 // 4
        return _jpeg_bytes(lambda out, cap, size: self._lib.j2p_planes_to_png(refs, n, ctypes.byref(spec), out, cap, size), guess)

    def stream(self):
        """the hipStream_t the solver launches on (an integer address)"""
        p = ctypes.c_void_p()
        _check(self._lib.j2p_solver_stream(self._h, ctypes.byref(p)))
        return p.value or 0

    def to_tensor(self, width, height, dtype=None, layout="chw", scale=None, bias=None, out=None, out_width=None, out_height=None,
                  box=None, filter=None):
        """The solved image, cropped to width x height, as an RGB (three-channel solver) or greyscale (one-channel solver)
        torch.Tensor on the solver's GPU — (3|1, height, width) for layout "chw", (height, width, 3|1) for "hwc" — without
        leaving the device (j2p_planes_rows_to_tensor): png.c's colour conversion and clamp to [0, 255], then per channel
        `* scale[k] + bias[k]` in float32 (two rounded operations), stored as dtype: torch.float32 (default), float16,
        bfloat16 (rounded to nearest even) or uint8 (the 8-bit samples; no scale / bias).  out: a tensor to write into, any
        view of that shape and dtype (a slot of a batch tensor, ...).  A band solver writes its own rows: height is then
        the band's row count and the rows are [row_begin, row_begin + height).
        out_width, out_height, box=(x, y, w, h): the rectangle `box` of the width x height image (default: all of it),
        area-resampled to out_width x out_height (default: the box's size, a pure crop; never larger than the box), is what
        the tensor receives (j2p_planes_to_tensor_resized) — its shape is then (3|1, out_height, out_width) or the "hwc"
        form.  Whole-canvas solvers only.  Without any of the three the call is what it was.
        filter: None or "area" — that area form; "triangle" or "cubic" — the antialiased triangle / cubic filter of
        torchvision's Resize, F.interpolate(antialias=True) and Pillow (j2p_planes_to_tensor_resampled), with which
        out_width / out_height may also be LARGER than the box.
        Nothing waits on the host: the kernel is queued on the solver's stream and torch's current stream is made to wait
        for it, so torch operations issued afterwards see the finished tensor."""
        resize = _resize_spec(width, height, out_width, out_height, box, filter)
        torch = _torch()
        if self.nch not in (1, 3):
            raise J2PError("tensor output needs a solver of three channels (RGB) or one (greyscale)")
        tw, th = (width, height) if resize is None else (resize.out_w, resize.out_h)        # the tensor's
        out = _tensor_to_fill(torch, out, dtype, layout, self.nch, tw, th, self.device)
        ct = _c_tensor(out, self.nch, tw, th, layout, scale, bias, device=self.device)
        refs = (_CPlaneRef * self.nch)(*[_CPlaneRef(self._h, c) for c in range(self.nch)])
        with self._filling(torch, [out]):
            if isinstance(resize, _CResample):
                _check(self._lib.j2p_planes_to_tensor_resampled(refs, self.nch, int(width), int(height), ctypes.byref(resize), ctypes.byref(ct)))
            elif resize is not None:
                _check(self._lib.j2p_planes_to_tensor_resized(refs, self.nch, int(width), int(height), ctypes.byref(resize), ctypes.byref(ct)))
            elif self.orientation > 1:          # (the rows forms take no oriented solver)
                _check(self._lib.j2p_planes_to_tensor(refs, self.nch, int(width), int(height), ctypes.byref(ct)))
            else:
                _check(self._lib.j2p_planes_rows_to_tensor(refs, self.nch, int(width), self.row_begin, self.row_begin + int(height), ctypes.byref(ct)))
        return out

    @contextlib.contextmanager
    def _filling(self, torch, tensors):
        """the stream hand-off of to_tensor / to_tensors, around the call that queues the kernels which fill `tensors`"""
        dev = torch.device("cuda", self.device)
        ours = torch.cuda.ExternalStream(self.stream(), device=dev)
        theirs = torch.cuda.current_stream(dev)
        ours.wait_stream(theirs)            # whatever torch still does with the tensors (their allocation, a fill) comes first
        yield
        theirs.wait_stream(ours)
        # The tensors are now in use on torch's current stream, behind the kernels: an allocator that owns them for another stream
        # must not hand them out again before that.  (Recorded for THEIR stream, never for ours: the allocator records an event on
        # every recorded stream when a tensor is freed, and the solver's stream is destroyed with the solver — which a tensor may
        # well outlive.)
        for t in tensors:
            t.record_stream(theirs)

    def to_tensors(self, width, height, outputs):
        """Several resampled views of the solved width x height image from ONE call (j2p_planes_to_tensors_resampled): the crops
        of multi-crop training, FiveCrop / TenCrop, a pyramid of sizes.  outputs: 1 to 16 dicts of out_width, out_height, box,
        filter ("triangle" or "cubic", required) and optionally out=, dtype, layout, scale, bias, each with the meaning it has in
        to_tensor.  Returns the list of tensors; tensor i holds bit for bit what to_tensor(width, height, **outputs[i]) gives.
        Two launches (the taps of all outputs, the sampling) plus one sampling launch per further dtype, whatever the number
        of outputs.  Stream handling is to_tensor's, once for the call and for every tensor."""
        n = _output_count(outputs)
        specs = [_output_spec(width, height, o, "out") for o in outputs]
        torch = _torch()
        if self.nch not in (1, 3):
            raise J2PError("tensor output needs a solver of three channels (RGB) or one (greyscale)")
        tensors, items = [], (_COutput * n)()
        for i, (o, r) in enumerate(zip(outputs, specs)):
            layout = o.get("layout", "chw")
            out = _tensor_to_fill(torch, o.get("out"), o.get("dtype"), layout, self.nch, r.out_w, r.out_h, self.device)
            items[i].r = r
            items[i].t = _c_tensor(out, self.nch, r.out_w, r.out_h, layout, o.get("scale"), o.get("bias"), device=self.device)
            tensors.append(out)
        refs = (_CPlaneRef * self.nch)(*[_CPlaneRef(self._h, c) for c in range(self.nch)])
        with self._filling(torch, tensors):
            _check(self._lib.j2p_planes_to_tensors_resampled(refs, self.nch, int(width), int(height), n, items))
        return tensors

    def download_gradient(self, c):
        """diagnostics: the objective gradient the last gradient phase wrote for channel c — between phase_gradient() and
        phase_project() only: afterwards the buffer of a channel that shares (shares_state) holds the next prob state"""
        out = np.empty((self.row_end - self.row_begin, self.W), dtype=np.float32)
        _check(self._lib.j2p_solver_download_gradient(self._h, c, out.ctypes.data))
        return out

    def plane_ptr(self, c):
        p = ctypes.c_void_p()
        _check(self._lib.j2p_solver_plane_ptr(self._h, c, ctypes.byref(p)))
        return p.value

    def launches_per_iteration(self):
        """kernel launches per iteration of an unlogged run of whole phases: 2 + the reduction launches of the solver's norm plan"""
        n = ctypes.c_uint()
        _check(self._lib.j2p_solver_launches_per_iteration(self._h, ctypes.byref(n)))
        return n.value

    def coefficient_bytes(self, c=0):
        """bytes per quantised coefficient the projection reads for channel c: 1 (every |d| <= 127) or 2"""
        n = ctypes.c_uint()
        _check(self._lib.j2p_solver_coefficient_bytes(self._h, int(c), ctypes.byref(n)))
        return n.value

    def shares_state(self, c=0):
        """True when channel c keeps its gradient and its prob state in one buffer (1x1 sampling at the canvas's pitch, prob term on)"""
        n = ctypes.c_int()
        _check(self._lib.j2p_solver_shares_state(self._h, int(c), ctypes.byref(n)))
        return bool(n.value)

    def arena_bytes(self):
        """bytes of device memory the solver carved its planes, state and reduction buffers from"""
        n = ctypes.c_size_t()
        _check(self._lib.j2p_solver_arena_bytes(self._h, ctypes.byref(n)))
        return n.value

    def wide_footprint(self, c=0):
        """True when the interior strips of channel c take the wide-footprint projection path (J2P_OPT_WIDE_FOOTPRINT)"""
        n = ctypes.c_uint()
        _check(self._lib.j2p_solver_wide_footprint(self._h, int(c), ctypes.byref(n)))
        return bool(n.value)

    def output_scratch_bytes(self):
        """bytes of the block the output stage keeps for this solver (j2p_solver_output_scratch_bytes): a call that finds it
        large enough allocates nothing"""
        n = ctypes.c_size_t()
        _check(self._lib.j2p_solver_output_scratch_bytes(self._h, ctypes.byref(n)))
        return n.value

    def debug_option(self, option, value):
        """schedule switches (J2P_OPT_*): speed only, never results"""
        _check(self._lib.j2p_solver_debug_option(self._h, int(option), int(value)))

    def phase_order(self):
        """(gradient, project): the J2P_ORDER_* the next iteration's phase launches take (J2P_OPT_PHASE_ORDER)"""
        self._lib.j2p_solver_phase_order.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_uint)]
        g, p = ctypes.c_uint(), ctypes.c_uint()
        _check(self._lib.j2p_solver_phase_order(self._h, ctypes.byref(g), ctypes.byref(p)))
        return g.value, p.value

    def debug_violations(self):
        """J2P_DEBUG builds: (count, first site code, first offset) of the phase kernels' address checks"""
        n, site, off = ctypes.c_ulonglong(), ctypes.c_uint(), ctypes.c_ulonglong()
        _check(self._lib.j2p_solver_debug_violations(self._h, ctypes.byref(n), ctypes.byref(site), ctypes.byref(off)))
        return n.value, site.value, off.value

    def trace(self, on=True, fetch=False, max_records=1 << 19):
        """J2P_TRACE builds (tools/wave_trace.py): switch the per-wavefront records on / off; fetch=True returns the
        records collected so far as an [n, 4] uint64 array (start, first data, end in 10 ns ticks, id)"""
        self._lib.j2p_solver_trace.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint,
                                               ctypes.POINTER(ctypes.c_uint)]
        if not fetch:
            _check(self._lib.j2p_solver_trace(self._h, 1 if on else 0, None, 0, None))
            return None
        out = np.zeros((max_records, 4), dtype=np.uint64)
        n = ctypes.c_uint()
        _check(self._lib.j2p_solver_trace(self._h, 1 if on else 0, out.ctypes.data, max_records, ctypes.byref(n)))
        return out[: n.value]

    def enable_timing(self, every=1):
        """record HIP events around the two phase kernels of every `every`-th iteration (0 = off)."""
        _check(self._lib.j2p_solver_enable_timing(self._h, int(every)))

    def timing_overhead_ms(self):
        """what a bracket of two event records measures by itself on this solver's stream (the scale of what the brackets add to kernel_times())"""
        v = ctypes.c_double()
        _check(self._lib.j2p_solver_timing_overhead(self._h, ctypes.byref(v)))
        return v.value

    def kernel_times(self):
        g, p, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_uint()
        _check(self._lib.j2p_solver_kernel_times(self._h, ctypes.byref(g), ctypes.byref(p), ctypes.byref(n)))
        return g.value, p.value, n.value


def _c_samples(samples, device=None):
    """the j2p_samples array of one 2-D uint8 torch tensor or numpy array per channel; returns (array, what must stay alive, the
    GPU tensors among them).  device: the GPU a tensor in device memory must be on (None: any, but all on one)."""
    arr = (_CSamples * len(samples))()
    held, on_gpu = [], []
    for i, a in enumerate(samples):
        if isinstance(a, np.ndarray):
            if a.dtype != np.uint8 or a.ndim != 2:
                raise J2PError(f"samples[{i}]: a 2-D uint8 array is needed, not {a.dtype} with {a.ndim} dimensions")
            ptr, shape, strides = a.ctypes.data, a.shape, a.strides
        else:
            torch = _torch()
            if not isinstance(a, torch.Tensor):
                raise J2PError(f"samples[{i}]: a torch.uint8 tensor or a numpy uint8 array is needed, not {type(a).__name__}")
            if a.dtype != torch.uint8 or a.dim() != 2:
                raise J2PError(f"samples[{i}]: a 2-D torch.uint8 tensor is needed, not {a.dtype} with {a.dim()} dimensions")
            if a.is_cuda:
                if device is not None and a.device.index != int(device):
                    raise J2PError(f"samples[{i}]: the tensor is on {a.device}, the solver on device {device}")
                if on_gpu and on_gpu[0].device != a.device:
                    raise J2PError("samples: the tensors must live on one GPU")
                on_gpu.append(a)
            ptr, shape, strides = a.data_ptr(), tuple(a.shape), a.stride()
        # (a dimension of size 1 is never stepped over; numpy and torch may report any stride for it)
        sy = max(int(strides[0]), 1) if shape[0] == 1 else int(strides[0])
        sx = max(int(strides[1]), 1) if shape[1] == 1 else int(strides[1])
        if shape[0] < 1 or shape[1] < 1:
            raise J2PError(f"samples[{i}]: empty ({shape[0]} x {shape[1]})")
        arr[i] = _CSamples(ptr, int(shape[1]), int(shape[0]), sy, sx)
        held.append(a)
    return arr, held, on_gpu


def _c_planes(planes):
    keep = []
    cpl = (_CPlane * len(planes))()
    for i, p in enumerate(planes):
        # (data None: the planes of a job made from samples — Batch.submit(samples=...); quant_table None: with quant="estimate")
        d = None if p.data is None else np.ascontiguousarray(p.data, dtype=np.int16)
        q = None if p.quant_table is None else np.ascontiguousarray(p.quant_table, dtype=np.uint16)
        f = None if p.fdata is None else np.ascontiguousarray(p.fdata, dtype=np.float32)
        keep += [d, q, f]
        cpl[i] = _CPlane(p.w, p.h, p.w_samp, p.h_samp, None if d is None else d.ctypes.data, None if f is None else f.ctypes.data,
                         None if q is None else q.ctypes.data)
    return cpl, keep


def samples_histogram(samples, device=0, stream=None):
    """The histogram the table estimator reads (j2p_samples_histogram; the header's "Estimated tables" is the definition): samples
    is ONE channel — a 2-D torch.uint8 tensor (on GPU `device`: read in place; on the CPU: served like an array) or a 2-D numpy uint8
    array, any strides >= 1.  Every complete 8x8 block without a sample of 0 or 255 goes through the DCT on the device and the
    magnitudes of its 64 rounded coefficients are counted -> (hist uint32 [64, 1024], blocks counted, blocks excluded).
    stream: the stream to queue on (the caller has ordered the samples' producer before it); None: for a tensor on the GPU a
    stream that is made to wait for torch's current one, as in Solver.from_samples, otherwise one of the call's own.  The call
    returns with the samples read."""
    lib = load_library()
    csm, held, on_gpu = _c_samples([samples], device)
    if on_gpu and stream is None:
        torch = _torch()
        dev = torch.device("cuda", int(device))
        ours = torch.cuda.Stream(device=dev)
        ours.wait_stream(torch.cuda.current_stream(dev))
        held.append(ours)
        stream = ours.cuda_stream
    hist = np.empty((64, 1024), np.uint32)
    blocks, excluded = ctypes.c_ulonglong(), ctypes.c_ulonglong()
    _check(lib.j2p_samples_histogram(int(device), stream, csm, hist.ctypes.data, ctypes.byref(blocks), ctypes.byref(excluded)))
    del held
    return hist, blocks.value, excluded.value


def _estimate_triple(r):
    return (np.array(r.table, dtype=np.uint16), np.array(r.determined, dtype=np.uint8).astype(bool), int(r.quality))


def estimate_quant_table(hist, chroma=False):
    """A quantisation table from a channel's histogram (j2p_quant_estimate: host code; the header's "Estimated tables" is the rule)
    -> (table uint16 [64] in natural order, determined bool [64], the fitted IJG quality).  chroma: fit and fill against the
    chrominance base table instead of the luminance one.  Entries that are not determined are filled from the fitted table."""
    lib = load_library()
    h = np.ascontiguousarray(hist, dtype=np.uint32)
    if h.shape != (64, 1024):
        raise J2PError(f"estimate_quant_table: a [64, 1024] histogram is needed, not {h.shape}")
    r = _CQuantEstimate()
    _check(lib.j2p_quant_estimate(h.ctypes.data, 1 if chroma else 0, ctypes.byref(r)))
    return _estimate_triple(r)


def _want_estimate(quant, planes, what):
    """quant=None or "estimate"; with "estimate" the planes carry no table at all or one each (which is then ignored)"""
    if quant is None:
        return False
    if quant != "estimate":
        raise J2PError(f"{what}: quant={quant!r} (None or \"estimate\")")
    have = [getattr(p, "quant_table", None) is not None for p in planes]
    if any(have) and not all(have):
        err = J2PError(f"{what}: quant=\"estimate\" with a quant_table in some planes and none in others")
        err.code = -1       # J2P_EINVAL, as the library's own refusals carry it
        raise err
    return True


class TiledSolver:
    """One plane set cut into row bands, band i on devices[i] (ids may repeat), driven from C by one host thread
    per band (include/jpeg2png_amd.h: j2p_tiled_*).  cuts = band boundaries or None for near-equal bands."""

    def __init__(self, planes, weight, pweight, iterations, devices, cuts=None):
        lib = load_library()
        self._lib = lib
        self._h = None
        self.nch = len(planes)
        cpl, keep = _c_planes(planes)
        n = len(devices)
        devs = (ctypes.c_int * n)(*[int(d) for d in devices])
        ccuts = None if cuts is None else (ctypes.c_uint * (n + 1))(*[int(c) for c in cuts])
        pw = (ctypes.c_float * self.nch)(*[float(x) for x in pweight])
        h = ctypes.c_void_p()
        _check(lib.j2p_tiled_create(ctypes.byref(h), n, devs, ccuts, self.nch, cpl, float(weight), pw, int(iterations)))
        self._h = h
        del keep
        W, H, nb = ctypes.c_uint(), ctypes.c_uint(), ctypes.c_uint()
        _check(lib.j2p_tiled_canvas(h, ctypes.byref(W), ctypes.byref(H), ctypes.byref(nb)))
        self.W, self.H, self.nband = W.value, H.value, nb.value

    def bands(self):
        out = []
        for b in range(self.nband):
            d, r0, r1 = ctypes.c_int(), ctypes.c_uint(), ctypes.c_uint()
            _check(self._lib.j2p_tiled_band(self._h, b, ctypes.byref(d), ctypes.byref(r0), ctypes.byref(r1), None))
            out.append((d.value, r0.value, r1.value))
        return out

    def run(self, n, log=False):
        if not log:
            _check(self._lib.j2p_tiled_run(self._h, n, None))
            return None
        rows = (_CLogRow * max(n, 1))()
        _check(self._lib.j2p_tiled_run(self._h, n, rows))
        return np.array([[r.objective, r.prob_dist, r.tv, r.tv2] for r in rows[:n]], dtype=np.float64).reshape(n, 4)

    def sync(self):
        _check(self._lib.j2p_tiled_sync(self._h))

    def reset(self):
        _check(self._lib.j2p_tiled_reset(self._h))

    def exchange(self):
        """how the bands exchange row sums and edge rows: "direct", "copy", "rccl" ("none": one plain band)"""
        name = ctypes.c_char_p()
        _check(self._lib.j2p_tiled_exchange(self._h, ctypes.byref(name)))
        return name.value.decode()

    def host_cpu_seconds(self):
        """user + system time the band threads have spent issuing work (they sleep while waiting for each other)"""
        v = ctypes.c_double()
        _check(self._lib.j2p_tiled_host_cpu_seconds(self._h, ctypes.byref(v)))
        return v.value

    def band_solver(self, b):
        """borrowed handle of band b's j2p_solver (kernel timing in bench.py); owned by the TiledSolver"""
        h, d, r0, r1 = ctypes.c_void_p(), ctypes.c_int(), ctypes.c_uint(), ctypes.c_uint()
        _check(self._lib.j2p_tiled_band(self._h, b, ctypes.byref(d), ctypes.byref(r0), ctypes.byref(r1), ctypes.byref(h)))
        s = Solver.__new__(Solver)
        s._lib, s._h, s._borrowed = self._lib, h, True
        s.nch, s.device, s.W, s.H, s.row_begin, s.row_end = self.nch, d.value, self.W, self.H, r0.value, r1.value
        return s

    def download(self, c):
        out = np.empty((self.H, self.W), dtype=np.float32)
        _check(self._lib.j2p_tiled_download(self._h, c, out.ctypes.data))
        return out

    def close(self):
        if getattr(self, "_h", None):
            self._lib.j2p_tiled_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class _JpegResult:
    """what a jpeg= job of a Batch fills: the buffer and the file's size in it"""

    def __init__(self, buffer, size):
        self.buffer, self.size = buffer, size


# ---- a job of a Batch: Batch.submit resolves the input (1) and the output (2) its keywords ask for, fills the _CJob (3) and calls the
# C entry point of that (input kind, output kind) pair (4) ----

# the keywords of Batch.submit that decide a job's output form; resized: one of out_width / out_height / box / filter is given
_Wanted = collections.namedtuple("_Wanted", "separate tile bits out quant_tables subsampling tensor layout scale bias out_width out_height box filter outputs "
                                            "jpeg resized png")


def _torch_has_finished(device):
    """The workers' streams know nothing of torch's: what torch has queued on its current stream of that device for memory a job
    reads or writes (a fill, the work of the memory's previous owner) has to be over before the job is queued."""
    _torch().cuda.current_stream(device).synchronize()


def _job_input(planes, width, height, samples, file, tile, resized, progressive=False):
    """step 1 -> (input kind: "planes", "samples" or "file"; the planes; the image's width and height; the C entry point's arguments
    for that input; what they point into).  resized: a tensor with out_width / out_height / box / filter is asked for."""
    if file is not None:
        if samples is not None or tile:
            raise J2PError("job: file= excludes samples= and tile")
        if resized:
            raise J2PError("job: with file= a resized tensor is an output of outputs=")
        address, size, held = _file_bytes(file)
        head = jpeg_parse(file.cpu().numpy().tobytes() if hasattr(file, "data_ptr") else file, progressive=progressive)
        if planes is None:
            planes = [Plane(k["w"], k["h"], k["w_samp"], k["h_samp"], None, k["quant_table"]) for k in head["components"]]
        if any(p.data is not None or p.fdata is not None for p in planes):
            raise J2PError("job: with file= the planes carry neither data nor fdata")
        width = head["width"] if width is None else width
        height = head["height"] if height is None else height
        if hasattr(file, "data_ptr") and file.is_cuda:
            _torch_has_finished(file.device)
        return "file", planes, width, height, (address, size), [held]
    if samples is not None:
        if tile:
            raise J2PError("job: samples= excludes tile")
        if resized:
            raise J2PError("job: with samples= a resized tensor is an output of outputs=")
        if len(samples) != len(planes):
            raise J2PError(f"job: {len(samples)} sample arrays for {len(planes)} planes")
        if any(p.data is not None or p.fdata is not None for p in planes):
            raise J2PError("job: with samples= the planes carry neither data nor fdata")
        csm, held, on_gpu = _c_samples(samples)
        if on_gpu:
            _torch_has_finished(on_gpu[0].device)
        return "samples", planes, width, height, (csm,), [held]
    return "planes", planes, width, height, (), []


def _job_output(job, want, planes, width, height):
    """step 2 -> (output kind: "own" (the job's own fields: float planes, samples, coefficients or a tensor's rows), "resized",
    "resampled", "outputs" or "jpeg"; what wait() hands back; what must stay alive until then; the C entry point's arguments for
    that output).  Refuses the keywords that no form takes together; the form's function refuses the rest and fills its fields of
    the job."""
    n, filled = len(planes), None
    if want.jpeg is not None:
        if want.bits or want.quant_tables is not None or want.subsampling is not None or want.tensor is not None or want.outputs is not None or \
                want.tile or want.out is not None:
            raise J2PError("job: jpeg= excludes bits, quant_tables, subsampling, tensor=, outputs=, out and tile")
        filled = ("jpeg",) + _fill_jpeg(job, want.jpeg, n, width, height)
    if want.png is not None:
        if want.jpeg is not None or want.bits or want.quant_tables is not None or want.subsampling is not None or want.tensor is not None or \
                want.outputs is not None or want.tile or want.out is not None:
            raise J2PError("job: png= excludes jpeg=, bits, quant_tables, subsampling, tensor=, outputs=, out and tile")
        filled = ("png",) + _fill_png(job, want.png, n, width, height)
    if want.outputs is not None:
        if want.tensor is not None or want.bits or want.quant_tables is not None or want.subsampling is not None or want.tile:
            raise J2PError("job: outputs= excludes tensor=, bits, quant_tables and tile")
        if want.out is not None or want.resized or want.layout != "chw" or want.scale is not None or want.bias is not None:
            raise J2PError("job: with outputs= every output carries its own keywords (out_width, out_height, box, filter, layout, scale, bias)")
        filled = ("outputs",) + _fill_outputs(job, want.outputs, n, width, height)
    if want.tensor is None and _filter_code(want.filter) is not None:
        raise J2PError("job: filter belongs to tensor output (tensor=)")
    if want.tensor is None and (want.out_width is not None or want.out_height is not None or want.box is not None):
        raise J2PError("job: out_width, out_height and box belong to tensor output (tensor=)")
    if want.outputs is not None:
        return filled
    if want.tensor is not None:
        resize = _resize_spec(width, height, want.out_width, want.out_height, want.box, want.filter)
        kind = "own" if resize is None else "resampled" if isinstance(resize, _CResample) else "resized"
        return (kind,) + _fill_tensor(job, want, resize, n, width, height)
    if want.layout != "chw" or want.scale is not None or want.bias is not None:
        raise J2PError("job: layout, scale and bias belong to tensor output (tensor=)")
    if want.jpeg is not None or want.png is not None:
        return filled
    if want.quant_tables is not None:
        return ("own",) + _fill_coefficients(job, want, n, width, height)
    if want.subsampling is not None:
        raise J2PError("job: subsampling needs coefficient output (quant_tables)")
    return ("own",) + (_fill_samples(job, want, n, width, height) if want.bits else _fill_planes(job, planes, want.separate))


# The output forms: each refuses what is wrong with its own keywords, fills its fields of the job and returns (what wait() hands
# back, what must stay alive until then, the C entry point's arguments for that output).

def _fill_jpeg(job, jpeg, n, width, height):
    if not isinstance(jpeg, dict) or set(jpeg) - {"quality", "quant_tables", "subsampling", "capacity", "optimize", "progressive", "restart_rows",
                                                   "restart_interval"}:
        raise J2PError("job: jpeg= is a dict of quality or quant_tables, subsampling and capacity")
    if n not in (1, 3):
        raise J2PError("jpeg: three components or one")
    cjpeg, held = _c_jpeg(width, height, n, jpeg.get("quality"), jpeg.get("quant_tables"), jpeg.get("subsampling", (1, 1)))
    sx, sy = (cjpeg.sub_w, cjpeg.sub_h) if n == 3 else (1, 1)
    room = 4096 + 2 * 64 * (-(-int(width) // 8) * -(-int(height) // 8)) * (1 + (n - 1) / (sx * sy))
    options = _restart_options(jpeg.get("optimize"), jpeg.get("progressive"), jpeg.get("restart_rows"), jpeg.get("restart_interval"))
    if options.restart_interval or options.restart_in_rows:     # (a marker and a pad per block per scan at the most)
        room += 3 * 10 * (-(-int(width) // 8) * -(-int(height) // 8)) * (1 + (n - 1) / (sx * sy))
    buffer, size = np.empty(int(jpeg.get("capacity") or room), dtype=np.uint8), ctypes.c_size_t(0)
    job.out_w, job.out_h = int(width), int(height)
    return _JpegResult(buffer, size), [cjpeg, held, options], (ctypes.byref(cjpeg), buffer.ctypes.data, buffer.size, ctypes.byref(size),
                                                               ctypes.byref(options))


def _fill_png(job, png, n, width, height):
    if not isinstance(png, dict) or set(png) - {"bits", "filter", "block_bytes", "idat_bytes", "capacity"}:
        raise J2PError("job: png= is a dict of bits, filter, block_bytes, idat_bytes and capacity")
    if n not in (1, 3):
        raise J2PError("png: three planes (RGB) or one (greyscale)")
    cpng = _c_png(width, height, png.get("bits", 8), png.get("filter"), png.get("block_bytes", 0), png.get("idat_bytes", 0))
    # (room for samples that do not compress at all: 9 bits a byte at most, and the framing)
    room = 4096 + (int(width) * n * (cpng.bits // 8 or 1) + 1) * int(height) * 5 // 4
    buffer, size = np.empty(int(png.get("capacity") or room), dtype=np.uint8), ctypes.c_size_t(0)
    job.out_w, job.out_h = int(width), int(height)
    return _JpegResult(buffer, size), [cpng], (ctypes.byref(cpng), buffer.ctypes.data, buffer.size, ctypes.byref(size))


def _fill_outputs(job, outputs, n, width, height):
    specs = [_output_spec(width, height, o, "tensor") for o in outputs[:_output_count(outputs)]]
    if any(o.get("tensor") is None for o in outputs):
        raise J2PError("job: every output of outputs= needs its tensor=")
    items = (_COutput * len(specs))()
    for i, (o, r) in enumerate(zip(outputs, specs)):
        t = o["tensor"]
        if o.get("dtype") is not None and getattr(t, "dtype", None) != o["dtype"]:
            raise J2PError(f"tensor output: tensor is {getattr(t, 'dtype', None)}, dtype says {o['dtype']}")
        items[i].r = r
        items[i].t = _c_tensor(t, n, r.out_w, r.out_h, o.get("layout", "chw"), o.get("scale"), o.get("bias"))
    if len({o["tensor"].device for o in outputs}) != 1:
        raise J2PError("job: the tensors of outputs= must live on one GPU")
    job.out_w, job.out_h = int(width), int(height)
    _torch_has_finished(outputs[0]["tensor"].device)
    return [o["tensor"] for o in outputs], [], (len(items), items)


def _fill_tensor(job, want, resize, n, width, height):
    if want.quant_tables is not None or want.subsampling is not None:
        raise J2PError("job: tensor output and coefficient output (quant_tables) exclude each other")
    if want.bits:
        raise J2PError("job: tensor output needs bits = 0")
    if want.out is not None:
        raise J2PError("job: tensor output is written into `tensor`; out is for host arrays")
    tw, th = (width, height) if resize is None else (resize.out_w, resize.out_h)        # the tensor's
    job.out_tensor = _c_tensor(want.tensor, n, tw, th, want.layout, want.scale, want.bias)
    job.out_w, job.out_h = int(width), int(height)
    _torch_has_finished(want.tensor.device)
    return want.tensor, [], () if resize is None else (ctypes.byref(resize),)


def _fill_coefficients(job, want, n, width, height):
    out = want.out
    if want.bits:
        raise J2PError("job: coefficient output (quant_tables) needs bits = 0")
    if len(want.quant_tables) != n:
        raise J2PError("job: one quantisation table per plane")
    if width is None or height is None or int(width) < 1 or int(height) < 1:
        raise J2PError("job: coefficient output needs width and height")
    bw, bh = (int(width) + 7) // 8, (int(height) + 7) // 8
    subs = [(1, 1)] * n if want.subsampling is None else [_sampling(v) for v in want.subsampling]
    if len(subs) != n:
        raise J2PError("job: one (sx, sy) pair per plane")
    grids = [(-(-bh // sy), -(-bw // sx), 64) for sx, sy in subs]
    tables = [np.ascontiguousarray(q, dtype=np.uint16).reshape(-1) for q in want.quant_tables]
    if any(q.size != 64 for q in tables):
        raise J2PError("job: a quantisation table has 64 entries")
    if out is None:
        out = [np.empty(g, dtype=np.int16) for g in grids]
    if not (isinstance(out, (list, tuple)) and len(out) == n and all(
            isinstance(a, np.ndarray) and a.shape == g and a.dtype == np.int16 and a.flags["C_CONTIGUOUS"]
            and a.flags["WRITEABLE"] for a, g in zip(out, grids))):
        raise J2PError(f"out must be a list of {n} writeable C-contiguous int16 arrays of shapes {grids}")
    for c in range(n):
        job.out_quant[c] = tables[c].ctypes.data
        job.out_coef[c] = out[c].ctypes.data
        job.out_sub_w[c], job.out_sub_h[c] = subs[c]
    job.out_blocks_w, job.out_blocks_h = bw, bh
    return out, [tables], ()


def _fill_samples(job, want, n, width, height):
    """(out: a caller's own RGB array, reused between jobs — nothing is then mapped or faulted in while other jobs' kernels run,
    which costs those a stalled launch each time)"""
    bits, out = want.bits, want.out
    # (the C side writes height * width * 3 samples of bits / 8 bytes: anything else is a heap overflow or a half-written array,
    # so it is an error here, not an assert that -O strips)
    if bits not in (8, 16):
        raise J2PError("job: out_bits must be 0, 8 or 16")
    if n == 2:
        raise J2PError("job: sample output needs three planes (RGB) or one (greyscale)")
    shape = (height, width) if n == 1 else (height, width, 3)           # one plane: greyscale, one sample per pixel
    if out is None:
        out = np.empty(shape, dtype=np.uint8 if bits == 8 else ">u2")
    if not (isinstance(out, np.ndarray) and out.shape == shape and out.flags["C_CONTIGUOUS"]
            and out.flags["WRITEABLE"] and out.dtype.itemsize == bits // 8 and out.dtype.kind in "ui"):
        raise J2PError(f"out must be a writeable C-contiguous {shape} array of "
                                   f"{bits // 8}-byte integers for bits = {bits}")
    job.out_bits, job.out_w, job.out_h = bits, width, height
    job.out_rgb = out.ctypes.data
    return out, [], ()


def _fill_planes(job, planes, separate):
    """the float planes: the canvas of a compute() call (compute.c:410-416) — all components' for a joint solve, its own for each of
    the separate calls of `-s` (jpeg2png.c:147-152)"""
    W = max(p.w * p.w_samp for p in planes)
    H = max(p.h * p.h_samp for p in planes)
    out = [np.empty((p.h * p.h_samp, p.w * p.w_samp) if separate else (H, W), dtype=np.float32) for p in planes]
    for c, a in enumerate(out):
        job.out_planes[c] = a.ctypes.data
    return out, [], ()


def _job_record(job, planes, weight, pweight, iterations, want, tile_devices, tile_min_band_pixels):
    """step 3: everything of the _CJob but its output form -> what it points into"""
    n = len(planes)
    job.nchannel = n
    job.tile = 1 if want.tile else 0
    if tile_devices:
        job.tile_first, job.tile_count = int(tile_devices[0]), int(tile_devices[1])
    if tile_min_band_pixels is not None:           # 0 = no gate at all (tests with small images)
        job.tile_min_band_pixels = int(tile_min_band_pixels) if tile_min_band_pixels else ctypes.c_size_t(-1).value
    cpl, keep = _c_planes(planes)
    for c in range(n):
        job.planes[c] = cpl[c]
    job.separate = 1 if want.separate else 0
    ws = list(weight) if isinstance(weight, (list, tuple)) else [weight] * n
    its = list(iterations) if isinstance(iterations, (list, tuple)) else [iterations] * n
    for c in range(n):
        job.weight[c], job.pweight[c], job.iterations[c] = float(ws[c]), float(pweight[c]), int(its[c])
    return keep


def _entry_point(source, source_args, kind, output_args):
    """step 4 -> (the C entry point of an (input kind, output kind) pair, its arguments between the job and the ticket)"""
    if kind == "jpeg":
        if source == "file":
            return "j2p_batch_submit_file_jpeg_opt", source_args + output_args
        return "j2p_batch_submit_jpeg_opt", (source_args or (None,)) + output_args      # (samples NULL: the planes' coefficients)
    if kind == "png":
        if source == "file":
            return "j2p_batch_submit_file_png", source_args + output_args
        return "j2p_batch_submit_png", (source_args or (None,)) + output_args           # (samples NULL: the planes' coefficients)
    if source != "planes":
        # (step 1 has refused the resized kinds; no outputs: the job's own form)
        return "j2p_batch_submit_" + source, source_args + (output_args or (0, None))
    return {"own": "j2p_batch_submit", "resized": "j2p_batch_submit_resized", "resampled": "j2p_batch_submit_resampled",
            "outputs": "j2p_batch_submit_outputs"}[kind], output_args


class Batch:
    """Images in flight over slots_per_device worker threads per GPU (include/jpeg2png_amd.h: j2p_batch_*).
    submit() returns a ticket; wait(ticket) returns the job's output: RGB samples [h, w, 3] (bits 8 / 16), greyscale
    samples [h, w] for a one-plane job (bits 8 / 16: the plane's compute(1, ...) written as png.c writes it with
    Cb = Cr = 0), or the list of float canvas planes (bits 0)."""

    def __init__(self, devices=(0,), slots_per_device=3):
        lib = load_library()
        self._lib = lib
        self._h = None
        devs = (ctypes.c_int * len(devices))(*[int(d) for d in devices])
        h = ctypes.c_void_p()
        _check(lib.j2p_batch_create(ctypes.byref(h), len(devices), devs, int(slots_per_device)))
        self._h = h
        self._pending = {}
        self._estimates = {}

    def submit(self, planes, weight, pweight, iterations, separate=False, width=None, height=None, bits=0, tile=False,
               tile_devices=None, tile_min_band_pixels=None, out=None, on_progress=None, quant_tables=None, subsampling=None,
               tensor=None, layout="chw", scale=None, bias=None, out_width=None, out_height=None, box=None, filter=None, outputs=None,
               samples=None, jpeg=None, file=None, png=None, orientation=None, progressive=False, quant=None):
        """quant="estimate" (with samples=; not with tile, jpeg= or png=): the worker reads the job's quantisation tables off the
        samples before it makes the solvers — a histogram launch per channel and the estimator, as
        Solver.from_samples(quant="estimate") does (j2p_batch_submit_samples_estimated).  The planes' quant_table may then be None
        (in every plane; tables given in every plane are ignored).  After wait(ticket), estimated_tables(ticket) returns the
        (table, determined, quality) triples;
        progressive=True (with file=): the file may be a progressive JPEG, every scan of which the worker decodes on its GPU
        (j2p_batch_next_file_scans, Solver.from_jpeg(progressive=True)); without it a progressive file is refused as before;
        orientation=1..8 or "exif" (the tag of file=, read at submit; file jobs only; not with tile): every solver of the job is
        oriented (Solver.set_orientation) and every output kind but the float planes delivers the UPRIGHT image, whose size width and
        height then are — for a file job they default to the file's upright size; the source image is the file's frame, or without
        a file width x height turned back;
        png={"bits": 8 or 16, "filter": None or 0..4 or a name, "block_bytes": n, "idat_bytes": n, "capacity": bytes} (with width and
        height; not with jpeg=, bits, quant_tables, tensor=, outputs= or tile; samples= and file= are allowed): wait() returns the image
        as a complete PNG file (bytes) that the worker converted, filtered and deflated on its GPU (j2p_batch_submit_png,
        Solver.to_png) — one or three planes.  capacity: room for the file (default: 5/4 of the filtered samples, which no image
        reaches; a larger file fails the job with the size it needs in the message);
        file=bytes or a 1-D uint8 torch tensor (on a GPU of the batch: read in place, and the job runs there): the job's solvers
        are made from that baseline JPEG file, Huffman-decoded on the worker's GPU (j2p_batch_submit_file, Solver.from_jpeg) —
        planes may be None (all of the file's components at the file's sampling) or Plane-likes with data=None, as
        jpeg_header(file)["planes"] are; width and height default to the file's.  Every output form is available (bits, tensor=,
        outputs=, quant_tables=, jpeg=: file in and file out in one job); not with samples=, tile, nor a resized tensor outside
        outputs=.  A file the parser refuses raises J2PError (code J2P_EFORMAT / J2P_ENOTSUP) here; damage only its data
        shows fails the job in wait(), and no other job.
        jpeg={"quality": Q or "quant_tables": [...], "subsampling": (sx, sy), "capacity": bytes, "optimize": bool, "progressive": bool} (with width and height; not
        with bits, quant_tables, tensor=, outputs= or tile; samples= is allowed): wait() returns the image as a complete baseline
        JPEG file (bytes) that the worker quantised and entropy-coded on its GPU (j2p_batch_submit_jpeg_opt, with file= j2p_batch_submit_file_jpeg_opt; Solver.to_jpeg) — one or
        three planes.  optimize: Huffman tables made for the image, as Solver.to_jpeg(optimize=True).  progressive: the
        progressive file, as Solver.to_jpeg(progressive=True); optimize changes nothing about it.
        "restart_rows": R or "restart_interval": N in the dict: restart intervals, as Solver.to_jpeg(restart_rows=, restart_interval=).
        capacity: room for the file (default: 4096 + 2 bytes per sample, which a file of natural content never
        reaches; a larger file fails the job with the size it needs in the message);
        samples=[one 2-D uint8 torch tensor or numpy array per plane] (planes with data=None; not with tile, nor with the
        out_width / out_height / box / filter of tensor=, which outputs= covers): the job's solvers are made from decoded 8-bit
        samples as Solver.from_samples makes them (j2p_batch_submit_samples) — every output form is available.  Tensors on a GPU
        pin the job to a worker of that GPU (one of the batch's, and the output tensors'); what torch has queued for them on its
        current stream is waited for before the job is queued.  Arrays and tensors must stay unchanged until wait();
        tensor=<torch CUDA tensor> (with width and height, bits 0; not with quant_tables or tile): the image is left on the
        GPU as that tensor's elements — shape (3|1, height, width) for layout "chw" or (height, width, 3|1) for "hwc", dtype
        uint8 / float16 / bfloat16 / float32, any view, with per-channel scale and bias as in Solver.to_tensor — by a worker
        of the tensor's GPU; wait() returns the tensor, complete for any stream.  What torch has queued for the tensor on its
        current stream is waited for before the job is queued;
        out_width, out_height, box=(x, y, w, h) (with tensor= only): the tensor receives the rectangle `box` of the width x height
        image (default: all of it) area-resampled to out_width x out_height (default: the box's size), as in Solver.to_tensor;
        its shape is (3|1, out_height, out_width) or the "hwc" form, while width and height stay the image's;
        filter (with tensor= only): None or "area" — that; "triangle" or "cubic" — the antialiased filter instead, which also
        enlarges (an image smaller than its slot), as in Solver.to_tensor;
        outputs=[dicts] (with width and height; not with tensor=, bits, quant_tables or tile): the one solve fills 1 to 16 tensors
        (j2p_batch_submit_outputs) — the dicts of Solver.to_tensors with tensor= in place of out= (required: a worker cannot
        allocate for torch), all on one GPU of the batch; wait() returns the list of tensors, each complete for any stream;
        quant_tables=[one 64-entry table per plane] (with width and height, bits 0): wait() returns the list of the planes'
        quantised coefficients, int16 [ceil(height / 8), ceil(width / 8), 64] each (Solver.coefficients) — what a JPEG
        writer entropy-codes — instead of the float planes;
        subsampling=[(sx, sy) per plane] (with quant_tables; 1 or 2 each): plane c at 1/sx x 1/sy of the resolution, int16
        [ceil(ceil(height / 8) / sy), ceil(ceil(width / 8) / sx), 64] — the component of a 4:2:0 / 4:2:2 / 4:4:0 JPEG;
        tile=True: the image is row-tiled over the batch's devices instead of solved on one of them;
        tile_devices=(first, count): over that slice of the batch's device list only; on_progress(n): called from the worker
        thread whenever n more iterations of one of the job's solves have finished (the CLI's progress bar, jpeg2png.c:449-452)"""
        resized = filter is not None or out_width is not None or out_height is not None or box is not None
        want = _Wanted(separate, tile, bits, out, quant_tables, subsampling, tensor, layout, scale, bias, out_width, out_height, box, filter, outputs,
                       jpeg, resized, png)
        job = _CJob()
        oriented = (0, 0, 0)            # what travels next to the job: j2p_batch_next_orientation
        if orientation is not None:
            # (what else is wrong with it — "exif" without file=, tile — the library refuses at submit)
            host = None if file is None else (file.cpu().numpy().tobytes() if hasattr(file, "data_ptr") else file)    # (one copy of a device file)
            if orientation == "exif":
                code = J2P_ORIENTATION_EXIF
                found = 1 if host is None else jpeg_orientation(host)
            else:
                code = found = int(orientation)
                if not 1 <= code <= 8:
                    err = J2PError(f"job: orientation {orientation!r} (1..8 or \"exif\")")
                    err.code = -1       # J2P_EINVAL, as the library's own refusals carry it
                    raise err
            oriented = (code, 0, 0)
            if host is not None and (width is None or height is None):
                head = jpeg_parse(host, progressive=progressive)
                uw, uh = upright_size(found, head["width"], head["height"])
                width, height = (uw if width is None else width), (uh if height is None else height)
            elif file is None and width is not None and height is not None:
                oriented = (code,) + upright_size(found, width, height)     # (turned back: the same swap)
        estimates = None
        if _want_estimate(quant, planes or (), "job"):
            if samples is None or tile or jpeg is not None or png is not None:
                err = J2PError("job: quant=\"estimate\" needs samples= and excludes tile, jpeg= and png=")
                err.code = -1       # J2P_EINVAL, as the library's own refusals carry it
                raise err
            estimates = (_CQuantEstimate * len(planes))()
        source, planes, width, height, source_args, keep = _job_input(planes, width, height, samples, file, tile, resized, progressive)
        kind, result, filled, output_args = _job_output(job, want, planes, width, height)
        keep += filled + _job_record(job, planes, weight, pweight, iterations, want, tile_devices, tile_min_band_pixels)
        if on_progress is not None:
            cb = _PROGRESS_CB(lambda _user, n: on_progress(int(n)))
            job.on_progress = cb
            keep.append(cb)                         # the trampoline lives as long as the job
        name, args = _entry_point(source, source_args, kind, output_args)
        if estimates is not None:
            name, args = name + "_estimated", args + (estimates,)
        t = ctypes.c_int()
        if oriented[0]:
            _check(self._lib.j2p_batch_next_orientation(self._h, *oriented))        # (this thread's next submit: the one below)
        if progressive and file is not None:
            _check(self._lib.j2p_batch_next_file_scans(self._h, 1))
        _check(getattr(self._lib, name)(self._h, ctypes.byref(job), *args, ctypes.byref(t)))
        self._pending[t.value] = (result, keep)
        if estimates is not None:
            self._estimates[t.value] = estimates
        return t.value

    def estimated_tables(self, ticket):
        """the (table, determined, quality) triples, one per plane, of a job submitted with quant="estimate" — once, after wait(ticket)"""
        if ticket in self._pending:
            raise J2PError(f"estimated_tables: job {ticket} has not been waited for")
        return [_estimate_triple(r) for r in self._estimates.pop(ticket)]

    def wait(self, ticket):
        out, _keep = self._pending.pop(ticket)
        _check(self._lib.j2p_batch_wait(self._h, ticket))
        if isinstance(out, _JpegResult):
            return out.buffer[:out.size.value].tobytes()
        return out

    def close(self):
        if getattr(self, "_h", None):
            self._lib.j2p_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def log_rows_from_sums(nch, weight, pweight, sums):
    """log rows [objective, prob_dist, tv, tv2] from per-iteration global sums (n x 5: tv, tv2, prob per channel)"""
    lib = load_library()
    sums = np.ascontiguousarray(sums, dtype=np.float64).reshape(-1, 2 + J2P_MAX_CHANNELS)
    n = sums.shape[0]
    rows = (_CLogRow * max(n, 1))()
    pw = (ctypes.c_float * nch)(*[float(x) for x in pweight])
    _check(lib.j2p_log_rows_from_sums(nch, float(weight), pw, n, sums.ctypes.data, rows))
    return np.array([[r.objective, r.prob_dist, r.tv, r.tv2] for r in rows[:n]], dtype=np.float64).reshape(n, 4)


class _CCoef(ctypes.Structure):
    """struct coef (jpeg2png.h:7-20, restated in include/jpeg2png_amd_compute.h)"""
    _fields_ = [("h", ctypes.c_uint), ("w", ctypes.c_uint), ("h_samp", ctypes.c_uint), ("w_samp", ctypes.c_uint),
                ("data", ctypes.c_void_p), ("fdata", ctypes.c_void_p), ("quant_table", ctypes.c_uint16 * 64)]


class _CComputeTimes(ctypes.Structure):
    _fields_ = [(k, ctypes.c_double) for k in ("create_ms", "issue_ms", "housekeeping_ms", "wait_ms", "download_ms", "destroy_ms", "total_ms")]


def compute_c(planes, weight, pweight, iterations, device=0, repeat=1, splits=None):
    """The C drop-in itself — j2p_compute(), what compute() (compute.h:8) is behind its die() wrapper — called the way
    the reference's decode_file() calls it (jpeg2png.c:141-152): planes that libc allocated (alloc_simd, utils.h:89-98),
    the float plane freed and a new one handed back (compute.c:304-305, 455-461), no logger, no progress bar.
    Returns (canvas planes of the last call, [seconds inside j2p_compute per call]): the host-to-host cost of the
    boundary, pageable memory on both sides.  `splits` (a list) receives one dict per call from j2p_compute_timing():
    where that call's wall time went."""
    import time
    lib = load_library()
    libc = ctypes.CDLL(None)
    libc.aligned_alloc.restype = ctypes.c_void_p
    libc.aligned_alloc.argtypes = [ctypes.c_size_t, ctypes.c_size_t]
    libc.malloc.restype = ctypes.c_void_p
    libc.malloc.argtypes = [ctypes.c_size_t]
    libc.free.argtypes = [ctypes.c_void_p]
    lib.j2p_compute.argtypes = [ctypes.c_int, ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float,
                                ctypes.c_void_p, ctypes.c_uint]
    n = len(planes)
    pw = (ctypes.c_float * n)(*[float(x) for x in pweight])
    seconds, outs = [], None
    for _ in range(repeat):
        coefs = (_CCoef * n)()
        for c, p in enumerate(planes):
            if p.fdata is None:
                raise J2PError("compute_c() expects decoded planes in fdata (jpeg.c:83-92); use decode_plane()")
            d = np.ascontiguousarray(p.data, dtype=np.int16)
            f = np.ascontiguousarray(p.fdata, dtype=np.float32)
            coefs[c].w, coefs[c].h, coefs[c].w_samp, coefs[c].h_samp = p.w, p.h, p.w_samp, p.h_samp
            coefs[c].data = libc.malloc(d.nbytes)
            coefs[c].fdata = libc.aligned_alloc(16, (f.nbytes + 15) & ~15)
            ctypes.memmove(coefs[c].data, d.ctypes.data, d.nbytes)
            ctypes.memmove(coefs[c].fdata, f.ctypes.data, f.nbytes)
            for k, q in enumerate(np.asarray(p.quant_table, dtype=np.uint16).reshape(64)):
                coefs[c].quant_table[k] = int(q)
        t0 = time.perf_counter()
        rc = lib.j2p_compute(int(device), n, coefs, None, None, float(weight), pw, int(iterations))
        seconds.append(time.perf_counter() - t0)
        if splits is not None and rc == 0:
            ct = _CComputeTimes()
            if lib.j2p_compute_timing(ctypes.byref(ct)) == 0:
                splits.append({k: getattr(ct, k) for k, _ in _CComputeTimes._fields_})
        try:
            _check(rc)
            outs = []
            for c in range(n):
                a = np.ctypeslib.as_array(ctypes.cast(coefs[c].fdata, ctypes.POINTER(ctypes.c_float)), shape=(coefs[c].h, coefs[c].w))
                outs.append(a.copy())
        finally:
            for c in range(n):
                libc.free(coefs[c].fdata)              # free_simd, jpeg2png.c:169
                libc.free(coefs[c].data)
    return outs, seconds


def zoomed(planes, s):
    """The planes of an image zoomed by the integer factor s (1..4): copies whose sampling factors are s times the
    given ones.  The solve of those is the smoothest image s times as wide and as high whose block means re-encode to
    the same coefficients (compute.c:295-309, 334-404 with every footprint s times larger).  Solver, TiledSolver,
    compute() and Batch.submit(..., width=s*w, height=s*h) take them as they are."""
    import copy
    if isinstance(s, bool) or not isinstance(s, (int, np.integer)) or not 1 <= int(s) <= ZOOM_MAX:
        raise J2PError(f"zoom factor must be an integer in 1..{ZOOM_MAX}, not {s!r}")
    out = []
    for p in planes:
        q = copy.copy(p)
        q.w_samp, q.h_samp = p.w_samp * int(s), p.h_samp * int(s)
        out.append(q)
    return out


def compute(planes, weight, pweight, iterations, log=False, device=0):
    """Python twin of the reference's compute() (compute.h:8): same arguments and the same
    in/out convention — on return every plane's `fdata` is the W x H canvas plane and its
    w/h are rewritten to the canvas size (compute.c:455-461).  Returns the log rows when asked."""
    for p in planes:
        if p.fdata is None:
            raise J2PError("compute() expects decoded planes in fdata (jpeg.c:83-92); use decode_plane()")
    with Solver(planes, weight, pweight, iterations, device=device) as s:
        rows = s.run(iterations, log=log)
        outs = [s.download(c) for c in range(len(planes))]
        W, H = s.W, s.H
    for p, o in zip(planes, outs):
        p.fdata = o
        p.w, p.h = W, H
    return rows


def _zigzag_to_natural():
    """natural-order index of the k-th coefficient of a zigzag scan (T.81 figure A.6): DQT segments store their steps in that order"""
    order = sorted(((x, y) for y in range(8) for x in range(8)), key=lambda p: (p[0] + p[1], p[1] if (p[0] + p[1]) % 2 else p[0]))
    return [y * 8 + x for x, y in order]


_NATURAL_OF_ZIGZAG = _zigzag_to_natural()


def jpeg_orientation(data):
    """The EXIF Orientation tag of a JPEG file (bytes), 1..8 — the pure-Python twin of j2p_jpeg_orientation: the SHORT 0x0112 in
    IFD0 of the first APP1 segment whose payload begins b"Exif\\0\\0", byte order II or MM, the magic 42 and the IFD0 offset
    honoured, nothing read outside the segment, segments read only up to SOS.  1 where there is no such segment, the TIFF
    structure is damaged or truncated, the tag has another type or count, or its value is outside 1..8 (PIL's behaviour)."""
    f = bytes(data)
    if len(f) < 4 or f[0] != 0xff or f[1] != 0xd8:
        return 1
    pos = 2
    while True:
        if pos + 2 > len(f) or f[pos] != 0xff:
            return 1
        marker = f[pos + 1]
        if marker == 0xff:
            pos += 1
            continue
        pos += 2
        if marker == 0x01 or 0xd0 <= marker <= 0xd8:
            continue
        if marker in (0xd9, 0xda) or pos + 2 > len(f):
            return 1
        length = (f[pos] << 8) | f[pos + 1]
        if length < 2 or length > len(f) - pos:
            return 1
        body = f[pos + 2:pos + length]
        pos += length
        if marker == 0xe1 and body[:6] == b"Exif\0\0":
            return _tiff_orientation(body[6:])


def _tiff_orientation(t):
    if len(t) < 8 or t[:2] not in (b"MM", b"II"):
        return 1
    order = "big" if t[:2] == b"MM" else "little"
    u = lambda at, n: int.from_bytes(t[at:at + n], order)
    if u(2, 2) != 42:
        return 1
    ifd = u(4, 4)
    if ifd > len(t) - 2:
        return 1
    entries = u(ifd, 2)
    if entries * 12 > len(t) - 2 - ifd:
        return 1
    for k in range(entries):
        e = ifd + 2 + 12 * k
        if u(e, 2) != 0x0112:
            continue
        if u(e + 2, 2) != 3 or u(e + 4, 4) != 1:
            return 1
        v = u(e + 8, 2)
        return v if 1 <= v <= 8 else 1
    return 1


def jpeg_header(data):
    """What Solver.from_samples needs of a JPEG besides its decoded planes, read from the file's bytes in pure Python (no libjpeg):
    the marker segments up to the first SOS.  Returns a dict:
      width, height     the image's size;
      progressive       True for SOF2;
      components        per component a dict of id, h_samp_factor, v_samp_factor, quant_table (uint16[64], natural order), the
                        coefficient plane's size w, h (whole blocks) and w_samp, h_samp as read_jpeg derives them (jpeg.c:49-58:
                        the largest sampling factor over the component's), and samples_w, samples_h: the samples a decoder
                        delivers for it, ceil(width * h_samp_factor / the largest), likewise the rows;
      planes            the same as Plane(w, h, w_samp, h_samp, data=None, quant_table) — what from_samples takes.
    Handles baseline, extended and progressive files (SOF0 / SOF1 / SOF2), 8- and 16-bit tables, several tables per DQT segment.
    ValueError for anything else: a component without its table, more than 3 components, 12-bit samples, a truncated segment,
    no SOF before SOS, another coding process."""
    data = bytes(data)
    if len(data) < 4 or data[0:2] != b"\xff\xd8":
        raise ValueError("not a JPEG: no SOI marker")
    tables, frame, pos = {}, None, 2
    while True:
        if pos + 2 > len(data):
            raise ValueError("truncated JPEG: no SOS marker")
        if data[pos] != 0xFF:
            raise ValueError(f"no marker at byte {pos}")
        marker = data[pos + 1]
        if marker == 0xFF:                      # fill byte
            pos += 1
            continue
        pos += 2
        if marker == 0x01 or 0xD0 <= marker <= 0xD8:      # TEM, RSTn, SOI: no segment
            continue
        if marker == 0xD9:
            raise ValueError("truncated JPEG: EOI before SOS")
        if pos + 2 > len(data):
            raise ValueError("truncated segment")
        length = int.from_bytes(data[pos:pos + 2], "big")
        if length < 2 or pos + length > len(data):
            raise ValueError(f"truncated segment (marker 0xFF{marker:02X})")
        body = data[pos + 2:pos + length]
        pos += length
        if marker == 0xDB:                      # DQT: one or more tables
            at = 0
            while at < len(body):
                precision, slot = body[at] >> 4, body[at] & 15
                at += 1
                if precision > 1 or slot > 3:
                    raise ValueError("invalid DQT segment")
                size = 128 if precision else 64
                if at + size > len(body):
                    raise ValueError("truncated segment (DQT)")
                raw = np.frombuffer(body, ">u2" if precision else np.uint8, 64, at).astype(np.uint16)
                at += size
                q = np.zeros(64, np.uint16)
                q[_NATURAL_OF_ZIGZAG] = raw
                tables[slot] = q
        elif marker in (0xC0, 0xC1, 0xC2):      # SOF0 / SOF1 / SOF2
            if len(body) < 6:
                raise ValueError("truncated segment (SOF)")
            if body[0] != 8:
                raise ValueError(f"{body[0]}-bit samples (only 8-bit JPEGs are supported)")
            n = body[5]
            if n < 1 or n > 3:
                raise ValueError(f"{n} components (1 to 3 are supported)")
            if len(body) < 6 + 3 * n:
                raise ValueError("truncated segment (SOF)")
            frame = {"height": int.from_bytes(body[1:3], "big"), "width": int.from_bytes(body[3:5], "big"), "progressive": marker == 0xC2,
                     "components": [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(n)]}
            if frame["width"] == 0 or frame["height"] == 0 or any(h == 0 or v == 0 for _, h, v, _ in frame["components"]):
                raise ValueError("invalid SOF segment")
        elif 0xC0 <= marker <= 0xCF and marker not in (0xC4, 0xC8, 0xCC):
            raise ValueError(f"unsupported coding process (marker 0xFF{marker:02X})")
        elif marker == 0xDA:                    # SOS: the header ends here
            break
    if frame is None:
        raise ValueError("no SOF segment before SOS")
    hmax = max(h for _, h, _, _ in frame["components"])
    vmax = max(v for _, _, v, _ in frame["components"])
    width, height = frame["width"], frame["height"]
    comps, planes = [], []
    for cid, hs, vs, slot in frame["components"]:
        if slot not in tables:
            raise ValueError(f"component {cid}: quantisation table {slot} is missing")
        sw, sh = -(-width * hs // hmax), -(-height * vs // vmax)
        w, h = -(-sw // 8) * 8, -(-sh // 8) * 8
        q = tables[slot].copy()
        comps.append({"id": cid, "h_samp_factor": hs, "v_samp_factor": vs, "quant_table": q, "w": w, "h": h,
                      "w_samp": hmax // hs, "h_samp": vmax // vs, "samples_w": sw, "samples_h": sh})
        planes.append(Plane(w, h, hmax // hs, vmax // vs, None, q))
    return {"width": width, "height": height, "progressive": frame["progressive"], "components": comps, "planes": planes}
