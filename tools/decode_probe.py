"""File input on the GPU, measured: python tools/decode_probe.py ROUNDS OUT.jsonl   (one MI355X, one process)

Images: synth.synth_rgb at 4096x3072 and 1920x1080, saved by PIL as 4:2:0 at quality 75 and 95 in three forms — plain, with
optimised Huffman tables, with one restart interval per MCU row.  Lines written:
  decode   j2p_entropy_decode_ex at three subsequence lengths: decode_ms — the library's own clock around the decode alone (the data's
           way up, every kernel, the rounds' read-backs; not the coefficients' way down) — and wall ms of the whole call, each median,
           min, max over ROUNDS after a warm-up call; subsequences, rounds, subsequences decoded again per round
  create   Solver.from_jpeg end to end against the path without it — the file's coefficients out of libjpeg (a run of the
           tests' read_coefficients helper, a process of its own, its start included) plus Solver(planes) from those host
           arrays — the two taken in turn, the order reversed every other round
  batch    images/s through Batch (three slots, 50 iterations, 12 jobs a burst) for 1920x1080 jobs resampled into f16 224x224 slots,
           file= jobs against coefficient jobs, bursts alternated
  cli      the driver end to end on the 4096x3072 quality-95 file: plain against -d, and -j 95 -e against -d -j 95 -e, alternated
The result of every decode is compared with libjpeg's coefficients first."""
import io
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FORMS = {"plain": {}, "optimize": {"optimize": True}, "restart_rows": {"restart_marker_rows": 1}}
LENGTHS = (512, 1024, 4096)


def helper(tmp):
    prefix = os.environ.get("J2P_IMG_PREFIX", "/opt/conda")
    exe = os.path.join(tmp, "read_coefficients")
    subprocess.run(["gcc", "-O2", "-I", os.path.join(prefix, "include"), os.path.join(ROOT, "tests", "c", "read_coefficients.c"), "-o", exe,
                    os.path.join(prefix, "lib", "libjpeg.so"), "-Wl,-rpath," + os.path.join(prefix, "lib")], check=True)
    return exe


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "n": len(ms)}


def batch_lines(j, emit, tag, data, planes, rounds):
    import torch
    jobs, per = 12, {"file": [], "coefficients": []}
    slots = [torch.zeros((3, 224, 224), dtype=torch.float16, device="cuda") for _ in range(jobs)]
    with j.Batch(devices=(0,), slots_per_device=3) as b:
        for r in range(2 * (rounds + 1)):
            kind = ("file", "coefficients")[r % 2]
            t0 = time.perf_counter()
            tickets = [b.submit(None if kind == "file" else planes, 0.3, [0.001] * 3, 50, width=1920, height=1080,
                                outputs=[{"tensor": t, "out_width": 224, "out_height": 224, "filter": "triangle"}],
                                file=data if kind == "file" else None) for t in slots]
            for t in tickets:
                b.wait(t)
            if r >= 2:
                per[kind].append(jobs / (time.perf_counter() - t0))
    emit({"kind": "batch", **tag, **{k: {"median_images_s": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)} for k, v in per.items()}})


def cli_lines(emit, tag, path, tmp, rounds):
    from jpeg2png_amd.buildlib import build_cli
    exe = build_cli()
    forms = {"png": [], "png -d": ["-d"], "-j 95 -e": ["-j", "95", "-e"], "-d -j 95 -e": ["-d", "-j", "95", "-e"]}
    ms = {k: [] for k in forms}
    for r in range(rounds + 1):
        for name in (list(forms) if r % 2 else list(forms)[::-1]):
            out = os.path.join(tmp, "out.jpg" if "-j" in name else "out.png")
            t0 = time.perf_counter()
            subprocess.run([exe, path, "-o", out, "-q", "-i", "50", *forms[name]], check=True)
            if r:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    emit({"kind": "cli", **tag, **{k: spread(v) for k, v in ms.items()}})


def main():
    rounds, out_path = int(sys.argv[1]), sys.argv[2]
    import jpeg2png_amd as j
    from jpeg2png_amd import synth
    from PIL import Image
    from test_jpeg_out_cli import load_coefficients
    j.load_library()
    tmp = tempfile.mkdtemp()
    exe = helper(tmp)
    with open(out_path, "a") as out:
        def emit(line):
            out.write(json.dumps(line) + "\n")
            out.flush()
            print(json.dumps(line), flush=True)

        for w, h in ((4096, 3072), (1920, 1080)):
            im = Image.fromarray(synth.synth_rgb(w, h, 5).astype(np.uint8), "RGB")
            for quality in (75, 95):
                for form, kw in FORMS.items():
                    buf = io.BytesIO()
                    im.save(buf, "JPEG", quality=quality, subsampling=2, **kw)
                    data = buf.getvalue()
                    path = os.path.join(tmp, "in.jpg")
                    open(path, "wb").write(data)
                    _w, _h, planes = load_coefficients(exe, path)
                    tag = {"image": f"{w}x{h}", "quality": quality, "form": form, "file_bytes": len(data)}
                    for bits in LENGTHS:
                        got, stats = j.entropy_decode(data, subsequence_bits=bits, stats=True)
                        for c in range(3):
                            assert np.array_equal(got[c].reshape(-1), np.asarray(planes[c].data).reshape(-1)), (tag, bits, c)
                        ms, inner = [], []
                        for _ in range(rounds):
                            t0 = time.perf_counter()
                            _arrays, st = j.entropy_decode(data, subsequence_bits=bits, stats=True)
                            ms.append((time.perf_counter() - t0) * 1e3)
                            inner.append(st["decode_ms"])
                        stats.pop("decode_ms")
                        emit({"kind": "decode", **tag, "subsequence_bits": bits, **stats, "decode_ms": spread(inner), "whole_call": spread(ms),
                              "default": bits == j.J2P_DECODE_SUBSEQUENCE_BITS})
                    if (w, quality, form) in ((1920, 75, "plain"), (1920, 95, "plain")):
                        batch_lines(j, emit, tag, data, planes, rounds)
                    if (w, quality, form) == (4096, 95, "plain"):
                        cli_lines(emit, tag, path, tmp, rounds)
                    ours, lib_ms, up_ms = [], [], []
                    for r in range(rounds + 1):
                        def from_file():
                            t0 = time.perf_counter()
                            with j.Solver.from_jpeg(data, 0.3, [0.001] * 3, 50):
                                pass
                            return (time.perf_counter() - t0) * 1e3

                        def from_libjpeg():
                            t0 = time.perf_counter()
                            _w, _h, p = load_coefficients(exe, path)
                            t1 = time.perf_counter()
                            with j.Solver(p, 0.3, [0.001] * 3, 50):
                                pass
                            return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3
                        if r % 2:
                            a, (b, c) = from_file(), from_libjpeg()
                        else:
                            (b, c), a = from_libjpeg(), from_file()
                        if r:                               # (round 0 warms both paths up)
                            ours.append(a)
                            lib_ms.append(b)
                            up_ms.append(c)
                    emit({"kind": "create", **tag, "from_jpeg": spread(ours), "libjpeg_helper_process": spread(lib_ms), "solver_from_host_arrays": spread(up_ms)})


if __name__ == "__main__":
    main()
