"""Build libjpeg2png_amd.so (HIP kernels + C-ABI shim + C host drop-in) in-tree for gfx950.

hipcc cross-compiles without a GPU, so this runs in the CPU-only container too.
Device code is built with -ffp-contract=off and no fast-math: the solver has to
reproduce the reference arithmetic operation for operation.
"""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
INCLUDE = os.path.join(ROOT, "include")
LIB = os.path.join(HERE, "libjpeg2png_amd.so")

HIP_FLAGS = [
    "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
    "-ffp-contract=off",            # no fused multiply-add: reference is built with -ffp-contract=off (Makefile:41-45)
    "-fno-fast-math",
    "-fhip-fp32-correctly-rounded-divide-sqrt",
    "-fno-gpu-flush-denormals-to-zero",
    # the kernels say themselves which float operations are packed (float2 arithmetic); left to the SLP pass, pairs of scalar
    # operations — the DCT butterflies of k_project above all — are packed too, with v_mov / v_pk_mov to line the operands
    # up, and a packed f32 operation costs two plain ones on gfx950 anyway (profiles/r03_valu_rates.json).  Same bits;
    # measured 4096^2 136.8 -> 140.6 Gpx-it/s (k_project 65.4 -> 62.0 us), 16384x2048 141.9 -> 146.3
    "-fno-slp-vectorize",
    "-Wall", "-Wno-unused-function",
]


def _newer(target, sources):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in sources)


# every translation unit with the project headers it includes, directly or through another: what an edit rebuilds
UNIT_HEADERS = {
    "j2p_solver.hip": ("j2p_kernels.hip.h", "j2p_dct.hip.h", "j2p_hip_host.h", "j2p_internal.h", "j2p_geometry.h"),
    "j2p_output.hip": ("j2p_output_kernels.hip.h", "j2p_dct.hip.h", "j2p_hip_host.h", "j2p_internal.h"),
    "j2p_codec.hip": ("j2p_codec_kernels.hip.h", "j2p_progressive_kernels.hip.h", "j2p_decode_kernels.hip.h", "j2p_scan_decode_kernels.hip.h", "j2p_png_kernels.hip.h",
                      "j2p_hip_host.h", "j2p_internal.h", "j2p_coder_block.h", "j2p_huffman.h", "j2p_deflate.h", "j2p_restart.h"),
    "j2p_estimate.hip": ("j2p_estimate_kernels.hip.h", "j2p_dct.hip.h", "j2p_hip_host.h", "j2p_internal.h"),
    "j2p_pool.hip": ("j2p_hip_host.h", "j2p_internal.h"),
    "j2p_tiled.hip": ("j2p_internal.h", "j2p_geometry.h"),
    "j2p_batch.hip": ("j2p_internal.h", "j2p_geometry.h"),
    "compute_host.c": ("j2p_internal.h", "j2p_geometry.h", "j2p_quant_estimate.h"),
    "j2p_jpeg_parse.c": ("j2p_internal.h",),
}
# the units the experiments build takes from the release build: they have no knobs
NO_KNOBS = ("j2p_output.hip", "j2p_codec.hip", "j2p_estimate.hip", "j2p_pool.hip")
HIP_UNITS = tuple(u for u in UNIT_HEADERS if u.endswith(".hip"))
# the pure C units (host code, gcc): the same objects in every build of the library
C_UNITS = tuple(u for u in UNIT_HEADERS if u.endswith(".c"))
C_OBJECTS = tuple(os.path.join(CSRC, u.replace(".c", ".o")) for u in C_UNITS)
# the units that hold device code (the others are host code).  Only the solver's knows -DJ2P_DEBUG, -DJ2P_TRACE and
# -DJ2P_EXP_*: the checked build and the A/B variants compile it alone and take every other object from the release build
DEVICE_UNITS = ("j2p_solver.hip", "j2p_output.hip", "j2p_codec.hip", "j2p_estimate.hip")
PUBLIC_HEADERS = ("jpeg2png_amd.h", "jpeg2png_amd_compute.h")


def _deps(unit):
    """the files whose change rebuilds a unit's object"""
    return ([os.path.join(CSRC, unit)] + [os.path.join(CSRC, h) for h in UNIT_HEADERS[unit]] +
            [os.path.join(INCLUDE, h) for h in PUBLIC_HEADERS] + [os.path.abspath(__file__)])


def _run(cmd, verbose):
    if verbose:
        print(" ".join(cmd), flush=True)
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise RuntimeError("build failed: " + " ".join(cmd))
    if verbose and (r.stdout or r.stderr):
        print(r.stdout + r.stderr)


def build(force=False, verbose=False):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    gcc = shutil.which("gcc") or "gcc"
    objs = []
    extra = os.environ.get("J2P_CXXFLAGS", "").split()
    jobs = []
    for u in HIP_UNITS:
        src, obj = os.path.join(CSRC, u), os.path.join(CSRC, u.replace(".hip", ".o"))
        objs.append(obj)
        if force or _newer(obj, _deps(u)):
            jobs.append([hipcc, *HIP_FLAGS, *extra, "-I", INCLUDE, "-I", CSRC, "-c", src, "-o", obj])
    for u, cobj in zip(C_UNITS, C_OBJECTS):
        objs.append(cobj)
        if force or _newer(cobj, _deps(u)):
            jobs.append([gcc, "-std=c11", "-O2", "-fPIC", "-Wall", "-Wextra", "-ffp-contract=off", "-I", INCLUDE, "-I", CSRC, "-c", os.path.join(CSRC, u),
                         "-o", cobj])
    if not jobs and not _newer(LIB, objs):
        return LIB
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(lambda c: _run(c, verbose), jobs))
    # SONAME so that programs linked with -ljpeg2png_amd find the library through their RUNPATH ($ORIGIN),
    # wherever the checkout lives
    _run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-lpthread", "-Wl,-soname,libjpeg2png_amd.so", "-o", LIB], verbose)
    return LIB


DEBUG_LIB = os.path.join(HERE, "libjpeg2png_amd_debug.so")


def build_debug(force=False, verbose=False):
    """The checked build (-DJ2P_DEBUG): every global access of the two phase kernels is compared with the range
    it is meant to stay in, the counterpart of the reference's DEBUG=1 build with its asserting pixel indexer
    (utils.h:68-81).  Same sources; only the solver's translation unit is compiled a second time.  Loaded with
    J2P_LIBRARY=<this file> (tests/test_debug_build_gpu.py, tools/debug_sweep.py)."""
    build(force=False, verbose=verbose)             # the host-only objects are shared with the release build
    src = os.path.join(CSRC, "j2p_solver.hip")
    obj = os.path.join(CSRC, "j2p_solver_debug.o")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if force or _newer(obj, _deps("j2p_solver.hip")):
        _run([hipcc, *HIP_FLAGS, "-DJ2P_DEBUG", "-I", INCLUDE, "-I", CSRC, "-c", src, "-o", obj], verbose)
    objs = [obj] + [os.path.join(CSRC, u.replace(".hip", ".o")) for u in HIP_UNITS if u != "j2p_solver.hip"]
    objs.extend(C_OBJECTS)
    if force or _newer(DEBUG_LIB, objs):
        _run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-lpthread", "-Wl,-soname,libjpeg2png_amd_debug.so", "-o", DEBUG_LIB], verbose)
    return DEBUG_LIB


EXP_LIB = os.path.join(HERE, "libjpeg2png_amd_exp.so")


def build_experiments(force=False, verbose=False):
    """The experiments build (-DJ2P_EXPERIMENTS, jpeg2png_amd/libjpeg2png_amd_exp.so): the release kernels plus the
    environment knobs that move choices among them — rows per strip, the shares of a gradient launch's item sizes, launch
    direction, where the norm is finished, ... (j2p_internal.h: j2p_exp_env) — and the split phases.  Same device code as
    the release build.  What the schedule-equivalence tests load (conftest.exp_lib)
    and the timing tools run on (J2P_LIBRARY=<this file>); never what a user of the library gets."""
    build(force=False, verbose=verbose)             # compute_host.o and the NO_KNOBS objects are shared
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    # (the objects do not travel with a gpurun lease, the library does: up to date against the SOURCES is enough)
    sources = {f for u in UNIT_HEADERS for f in _deps(u)}
    if not force and os.path.exists(EXP_LIB) and not _newer(EXP_LIB, sources):
        return EXP_LIB
    jobs, objs = [], []
    for u in HIP_UNITS:
        if u in NO_KNOBS:
            objs.append(os.path.join(CSRC, u.replace(".hip", ".o")))
            continue
        src, obj = os.path.join(CSRC, u), os.path.join(CSRC, u.replace(".hip", "_exp.o"))
        objs.append(obj)
        if force or _newer(obj, _deps(u)):
            jobs.append([hipcc, *HIP_FLAGS, "-DJ2P_EXPERIMENTS", "-I", INCLUDE, "-I", CSRC, "-c", src, "-o", obj])
    objs.extend(C_OBJECTS)
    if jobs or _newer(EXP_LIB, objs):
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=4) as ex:
            list(ex.map(lambda c: _run(c, verbose), jobs))
        _run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-lpthread", "-Wl,-soname,libjpeg2png_amd_exp.so", "-o", EXP_LIB], verbose)
    return EXP_LIB


CLI = os.path.join(HERE, "jpeg2png_gpu")


def build_cli(force=False, verbose=False, prefix=None):
    """Build the command-line driver cli/jpeg2png_gpu.c (needs libjpeg + libpng headers; this image
    ships them under /opt/conda).  Returns the path, or None when the libraries are not available."""
    prefix = prefix or os.environ.get("J2P_IMG_PREFIX", "/opt/conda")
    src = os.path.join(ROOT, "cli", "jpeg2png_gpu.c")
    if not (os.path.exists(os.path.join(prefix, "include", "jpeglib.h")) and os.path.exists(os.path.join(prefix, "include", "png.h"))):
        return None
    lib = build(force=False, verbose=verbose)
    if not force and not _newer(CLI, [src, lib, os.path.join(INCLUDE, "jpeg2png_amd.h")]):
        return CLI
    gcc = shutil.which("gcc") or "gcc"
    plib = os.path.join(prefix, "lib")
    # the image libraries are named by full path and found at run time through RUNPATH (direct
    # dependencies only), so that the HIP runtime keeps resolving libstdc++ from the system
    cmd = [gcc, "-std=c11", "-O2", "-Wall", "-Wextra", "-I", INCLUDE, "-I", os.path.join(prefix, "include"), src, "-o", CLI,
           "-L", HERE, "-ljpeg2png_amd", os.path.join(plib, "libjpeg.so"), os.path.join(plib, "libpng16.so"), os.path.join(plib, "libz.so"), "-lpthread",
           "-Wl,--enable-new-dtags", "-Wl,-rpath-link,/usr/lib/x86_64-linux-gnu:/opt/rocm/lib",
           "-Wl,-rpath,$ORIGIN", "-Wl,-rpath," + plib]
    if verbose:
        print(" ".join(cmd), flush=True)
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise RuntimeError("CLI build failed")
    return CLI


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
    print(build_cli(force="--force" in sys.argv, verbose=True))
