#!/usr/bin/env python3
"""Resized tensor output on one 4096x3072 4:2:0 image solved jointly, box = the whole image, f16 CHW outputs of 224x224,
1024x768 and 4095x3071, all in one process and alternated:
  (a)  the new launch: j2p_planes_to_tensor_resized (k_to_tensor_resized<3, f16>);
  (b)  the existing full-size launch: j2p_planes_to_tensor, f32 CHW (k_to_tensor<3, f32, planar>);
  (c)  what a caller does without (a): Solver.to_tensor f32 at full size, torch.nn.functional.interpolate(mode="area") at
       integer ratios (adaptive_avg_pool2d otherwise), then the cast and the copy into a slot of an f16 batch tensor;
  batch  images per second through Batch (three slots), resized f16 jobs into 224x224 slots against full-size f16 tensor jobs.
(a), (b) and (c) are device-event times per call over LAUNCHES back-to-back calls on one stream (so they hold the launch gaps
of a stream that is never idle, not only the kernels), REPEATS repeats each, taken in turn; the median, minimum and maximum of
the repeats are recorded.  (a) is also compared with (c)'s result: the largest difference, in f16 units of the output.
Public API only.  Appends one JSON line per measurement to OUT (default profiles/resized_tensor.jsonl) and prints them;
COMMIT, when given, goes into every line as "commit".
    python tools/resize_probe.py [ITERATIONS] [ROUNDS] [OUT] [COMMIT]"""
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import jpeg2png_amd as j  # noqa: E402
from jpeg2png_amd import synth  # noqa: E402

import torch  # noqa: E402

W, H = 4096, 3072
WEIGHT, PWEIGHT = 0.3, 0.001
SIZES = [(224, 224), (1024, 768), (4095, 3071)]
LAUNCHES, REPEATS = 50, 5

args = sys.argv[1:]
its = int(args[0]) if args else 50
rounds = int(args[1]) if len(args) > 1 else 3
out_path = args[2] if len(args) > 2 else os.path.join(ROOT, "profiles", "resized_tensor.jsonl")
commit = {"commit": args[3]} if len(args) > 3 else {}
lines = []


def emit(rec):
    rec = {**commit, **rec}
    lines.append(rec)
    print(json.dumps(rec), flush=True)


if not torch.cuda.is_available():
    sys.exit("resize_probe needs a GPU: nothing here is measured without one")

planes = synth.make_planes(W, H, "420", 50, seed=1240)
scale = [1.0 / (255.0 * s) for s in (0.229, 0.224, 0.225)]
bias = [-m / s for m, s in zip((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))]


def timed(stream, call):
    """microseconds per call: LAUNCHES calls between two events on `stream`"""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record(stream)
    for _ in range(LAUNCHES):
        call()
    end.record(stream)
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / LAUNCHES


with j.Solver(planes, WEIGHT, [PWEIGHT] * 3, 1) as s:
    s.run(1)
    s.sync()
    lib = s._lib
    refs = (j._CPlaneRef * 3)(*[j._CPlaneRef(s._h, c) for c in range(3)])
    ours = torch.cuda.ExternalStream(s.stream(), device=torch.device("cuda", 0))
    theirs = torch.cuda.current_stream()
    full32 = torch.empty((3, H, W), dtype=torch.float32, device="cuda:0")
    ct32 = j._c_tensor(full32, 3, W, H, "chw", None, None)
    s32 = torch.tensor(scale, device="cuda:0").view(3, 1, 1)
    b32 = torch.tensor(bias, device="cuda:0").view(3, 1, 1)

    def launch_b():
        j._check(lib.j2p_planes_to_tensor(refs, 3, W, H, ctypes.byref(ct32)))

    for ow, oh in SIZES:
        slots = torch.zeros((2, 3, oh, ow), dtype=torch.float16, device="cuda:0")
        ct16 = j._c_tensor(slots[0], 3, ow, oh, "chw", scale, bias)
        resize = j._CResize(0, 0, W, H, ow, oh)
        integer = W % ow == 0 and H % oh == 0

        def launch_a():
            j._check(lib.j2p_planes_to_tensor_resized(refs, 3, W, H, ctypes.byref(resize), ctypes.byref(ct16)))

        def today():
            t = s.to_tensor(W, H, out=full32)
            if integer:
                small = torch.nn.functional.interpolate(t[None], size=(oh, ow), mode="area")[0]
            else:
                small = torch.nn.functional.adaptive_avg_pool2d(t, (oh, ow))
            slots[1].copy_(small * s32 + b32)          # (the normalisation (a) applies on the way, then the cast and the copy)

        torch.cuda.synchronize()
        for _ in range(3):                               # every shape of the timed window, warmed up
            launch_a()
            launch_b()
            today()
        torch.cuda.synchronize()
        us = {"a": [], "b": [], "c": []}
        for _ in range(REPEATS):
            us["a"].append(timed(ours, launch_a))
            us["b"].append(timed(ours, launch_b))
            torch.cuda.synchronize()
            us["c"].append(timed(theirs, today))
            torch.cuda.synchronize()
        diff = float((slots[0].float() - slots[1].float()).abs().max())
        what = {"a": "j2p_planes_to_tensor_resized f16 chw", "b": f"j2p_planes_to_tensor f32 chw {W}x{H}",
                "c": "to_tensor f32 + " + ("interpolate(mode='area')" if integer else "adaptive_avg_pool2d") + " + scale, bias, cast, copy into the slot"}
        med = {k: statistics.median(v) for k, v in us.items()}
        for k in "abc":
            emit({"what": k, "call": what[k], "source": f"{W}x{H} 4:2:0 joint", "output": f"{ow}x{oh}", "calls_per_repeat": LAUNCHES,
                  "repeats": REPEATS, "us_median": round(med[k], 2), "us_min": round(min(us[k]), 2), "us_max": round(max(us[k]), 2)})

        def verdict(x, y):
            """x against y: "equal" when the medians differ by less than the repeats of either spread"""
            spread = max(max(us[x]) - min(us[x]), max(us[y]) - min(us[y]))
            return "equal" if abs(med[x] - med[y]) <= spread else ("faster" if med[x] < med[y] else "slower")

        emit({"what": "compare", "output": f"{ow}x{oh}", "a_against_b": verdict("a", "b"), "a_against_c": verdict("a", "c"),
              "a_minus_c_max_abs": diff, "source_bytes_read_MB": round(3 * 4 * W * H / 1e6, 1), "bytes_written_MB": round(3 * 2 * ow * oh / 1e6, 2)})
        del slots

# ---- batch: images per second, resized slots against full-size tensors ----
IN_FLIGHT, IMAGES = 3, 12
full = torch.empty((IN_FLIGHT, 3, H, W), dtype=torch.float16, device="cuda:0")
small = torch.empty((IN_FLIGHT, 3, 224, 224), dtype=torch.float16, device="cuda:0")
with j.Batch(devices=(0,), slots_per_device=IN_FLIGHT) as b:
    def run(kind, n):
        def submit(i):
            if kind == "f16 chw 224x224 resized":
                return b.submit(planes, WEIGHT, [PWEIGHT] * 3, its, width=W, height=H, tensor=small[i % IN_FLIGHT], scale=scale, bias=bias,
                                out_width=224, out_height=224)
            return b.submit(planes, WEIGHT, [PWEIGHT] * 3, its, width=W, height=H, tensor=full[i % IN_FLIGHT], scale=scale, bias=bias)
        t0 = time.perf_counter()
        tickets = [submit(i) for i in range(min(IN_FLIGHT, n))]
        for i in range(n):
            b.wait(tickets[i])
            if i + IN_FLIGHT < n:
                tickets.append(submit(i + IN_FLIGHT))
        return n / (time.perf_counter() - t0)

    kinds = ["f16 chw 224x224 resized", f"f16 chw {W}x{H} tensor"]
    for kind in kinds:
        run(kind, IN_FLIGHT)
    rates = {k: [] for k in kinds}
    for r in range(rounds):
        for kind in (kinds if r % 2 == 0 else kinds[::-1]):
            rates[kind].append(run(kind, IMAGES))
    for kind in kinds:
        emit({"what": "batch", "image": f"{W}x{H} 4:2:0 joint", "output": kind, "iterations": its, "rounds": rounds, "images_per_round": IMAGES,
              "slots": IN_FLIGHT, "images_per_s_median": round(statistics.median(rates[kind]), 2), "images_per_s_best": round(max(rates[kind]), 2),
              "images_per_s_worst": round(min(rates[kind]), 2)})

with open(out_path, "a") as f:
    for r in lines:
        f.write(json.dumps(r) + "\n")
