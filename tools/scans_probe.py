"""Progressive file input on the GPU, measured: python tools/scans_probe.py ROUNDS OUT.jsonl   (one MI355X, one process)

Images: synth.synth_rgb at 4096x3072, saved by PIL as 4:2:0 at quality 75 and 95, progressive and baseline.  Lines written:
  decode   j2p_entropy_decode_scans on the progressive file: decode_ms — the library's own clock around the decode alone — and its
           AC-refinement share (events around the AC refinement launches), the rounds, the host waits, the subsequences; beside it
           j2p_entropy_decode_ex on the baseline file of the same image, and the libjpeg helper process of tools/decode_probe.py on
           the progressive file; each median, min, max over ROUNDS after a warm-up call, the three taken in turn
  create   Solver.from_jpeg(progressive=True) end to end against the libjpeg helper plus Solver(planes), alternated
  batch    images/s through Batch (three slots, 50 iterations, 12 jobs a burst) for 1920x1080 jobs resampled into f16 224x224 slots:
           progressive file= jobs against baseline file= jobs, bursts alternated
The result of every decode is compared with libjpeg's coefficients first."""
import io
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from decode_probe import helper, spread  # noqa: E402


def pil_file(im, quality, progressive):
    buf = io.BytesIO()
    im.save(buf, "JPEG", quality=quality, subsampling=2, progressive=progressive)
    return buf.getvalue()


def batch_line(j, emit, tag, files, rounds):
    import torch
    jobs, per = 12, {k: [] for k in files}
    slots = [torch.zeros((3, 224, 224), dtype=torch.float16, device="cuda") for _ in range(jobs)]
    with j.Batch(devices=(0,), slots_per_device=3) as b:
        for r in range(2 * (rounds + 1)):
            kind = list(files)[r % 2]
            t0 = time.perf_counter()
            tickets = [b.submit(None, 0.3, [0.001] * 3, 50, width=1920, height=1080, file=files[kind], progressive=kind == "progressive",
                                outputs=[{"tensor": t, "out_width": 224, "out_height": 224, "filter": "triangle"}]) for t in slots]
            for t in tickets:
                b.wait(t)
            if r >= 2:
                per[kind].append(jobs / (time.perf_counter() - t0))
    emit({"kind": "batch", **tag, **{k: {"median_images_s": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)} for k, v in per.items()}})


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

        im = Image.fromarray(synth.synth_rgb(4096, 3072, 5).astype(np.uint8), "RGB")
        for quality in (75, 95):
            prog, base = pil_file(im, quality, True), pil_file(im, quality, False)
            path = os.path.join(tmp, "in.jpg")
            open(path, "wb").write(prog)
            _w, _h, planes = load_coefficients(exe, path)
            tag = {"image": "4096x3072", "quality": quality, "progressive_bytes": len(prog), "baseline_bytes": len(base)}
            got, stats = j.entropy_decode(prog, stats=True, progressive=True)
            for c in range(3):
                assert np.array_equal(got[c].reshape(-1), np.asarray(planes[c].data).reshape(-1)), (tag, c)
            j.entropy_decode(base)
            ours, share, baseline, libjpeg = [], [], [], []
            for _ in range(rounds):
                _a, st = j.entropy_decode(prog, stats=True, progressive=True)
                ours.append(st["decode_ms"])
                share.append(st["ac_refine_share"])
                _a, st = j.entropy_decode(base, stats=True)
                baseline.append(st["decode_ms"])
                t0 = time.perf_counter()
                load_coefficients(exe, path)
                libjpeg.append((time.perf_counter() - t0) * 1e3)
            for k in ("decode_ms", "ac_refine_share"):
                stats.pop(k)
            emit({"kind": "decode", **tag, **stats, "decode_ms": spread(ours), "ac_refine_share": round(statistics.median(share), 4),
                  "baseline_file_decode_ms": spread(baseline), "libjpeg_helper_process": spread(libjpeg)})
            mine, lib_ms, up_ms = [], [], []
            for r in range(rounds + 1):
                def from_file():
                    t0 = time.perf_counter()
                    with j.Solver.from_jpeg(prog, 0.3, [0.001] * 3, 50, progressive=True):
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
                if r:
                    mine.append(a)
                    lib_ms.append(b)
                    up_ms.append(c)
            emit({"kind": "create", **tag, "from_jpeg_progressive": spread(mine), "libjpeg_helper_process": spread(lib_ms), "solver_from_host_arrays": spread(up_ms)})
        small = Image.fromarray(synth.synth_rgb(1920, 1080, 5).astype(np.uint8), "RGB")
        for quality in (75, 95):
            files = {"progressive": pil_file(small, quality, True), "baseline": pil_file(small, quality, False)}
            batch_line(j, emit, {"image": "1920x1080", "quality": quality, **{k + "_bytes": len(v) for k, v in files.items()}}, files, rounds)


if __name__ == "__main__":
    main()
