#!/usr/bin/env python3
"""Filtered tensor output on one 4096x3072 4:2:0 image solved jointly, f16 CHW outputs with scale and bias, all in one process and
alternated (the protocol of tools/resize_probe.py):
  (a)  the new launches, per filter: j2p_planes_to_tensor_resampled (k_filter_taps + k_to_tensor_filtered<3, f16>), the whole
       image to 224x224, 1024x768 and 4095x3071, and the box (0, 0, 640, 480) enlarged to 1024x768;
  (b)  the area launch at the three shrinking sizes: j2p_planes_to_tensor_resized (k_to_tensor_resized<3, f16>);
  (c)  what a caller does without (a): Solver.to_tensor f32 at full size, the crop, torch.nn.functional.interpolate(mode=
       "bilinear" | "bicubic", antialias=True), then scale, bias, the cast and the copy into a slot of an f16 batch tensor;
  batch  images per second through Batch (three slots), triangle jobs into 224x224 slots against area jobs into the same.
(a), (b) and (c) are device-event times per call over LAUNCHES back-to-back calls on one stream (so they hold the launch gaps
of a stream that is never idle, not only the kernels), REPEATS repeats each, taken in turn; the median, minimum and maximum of
the repeats are recorded.  (a) is also compared with (c)'s result: the largest difference, in f16 units of the output.
Public API only.  Appends one JSON line per measurement to OUT (default profiles/filtered_tensor.jsonl) and prints them;
COMMIT, when given, goes into every line as "commit".
    python tools/filter_probe.py [ITERATIONS] [ROUNDS] [OUT] [COMMIT]"""
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
WHOLE = (0, 0, W, H)
# (box, output): three shrinks of the whole image and one enlargement of a corner
SHAPES = [(WHOLE, (224, 224)), (WHOLE, (1024, 768)), (WHOLE, (4095, 3071)), ((0, 0, 640, 480), (1024, 768))]
MODES = {"triangle": "bilinear", "cubic": "bicubic"}
LAUNCHES, REPEATS = 50, 5

args = sys.argv[1:]
its = int(args[0]) if args else 50
rounds = int(args[1]) if len(args) > 1 else 3
out_path = args[2] if len(args) > 2 else os.path.join(ROOT, "profiles", "filtered_tensor.jsonl")
commit = {"commit": args[3]} if len(args) > 3 else {}
lines = []


def emit(rec):
    rec = {**commit, **rec}
    lines.append(rec)
    print(json.dumps(rec), flush=True)


if not torch.cuda.is_available():
    sys.exit("filter_probe needs a GPU: nothing here is measured without one")

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


def stats(us):
    return {"calls_per_repeat": LAUNCHES, "repeats": REPEATS, "us_median": round(statistics.median(us), 2), "us_min": round(min(us), 2),
            "us_max": round(max(us), 2)}


with j.Solver(planes, WEIGHT, [PWEIGHT] * 3, 1) as s:
    s.run(1)
    s.sync()
    lib = s._lib
    refs = (j._CPlaneRef * 3)(*[j._CPlaneRef(s._h, c) for c in range(3)])
    ours = torch.cuda.ExternalStream(s.stream(), device=torch.device("cuda", 0))
    theirs = torch.cuda.current_stream()
    full32 = torch.empty((3, H, W), dtype=torch.float32, device="cuda:0")
    s32 = torch.tensor(scale, device="cuda:0").view(3, 1, 1)
    b32 = torch.tensor(bias, device="cuda:0").view(3, 1, 1)

    for box, (ow, oh) in SHAPES:
        bx, by, bw, bh = box
        source = f"{W}x{H} 4:2:0 joint" + ("" if box == WHOLE else f", box {bw}x{bh}")
        slots = torch.zeros((2, 3, oh, ow), dtype=torch.float16, device="cuda:0")
        ct16 = j._c_tensor(slots[0], 3, ow, oh, "chw", scale, bias)
        us = {}
        calls = {}
        if ow <= bw and oh <= bh:
            resize = j._CResize(bx, by, bw, bh, ow, oh)
            calls["b"] = lambda resize=resize: j._check(lib.j2p_planes_to_tensor_resized(refs, 3, W, H, ctypes.byref(resize), ctypes.byref(ct16)))
        for name, code in j.FILTERS.items():
            resample = j._CResample(bx, by, bw, bh, ow, oh, code)
            calls["a " + name] = lambda resample=resample: j._check(
                lib.j2p_planes_to_tensor_resampled(refs, 3, W, H, ctypes.byref(resample), ctypes.byref(ct16)))

            def today(mode=MODES[name]):
                t = s.to_tensor(W, H, out=full32)
                small = torch.nn.functional.interpolate(t[None, :, by:by + bh, bx:bx + bw], size=(oh, ow), mode=mode, antialias=True,
                                                        align_corners=False)[0]
                slots[1].copy_(small.clamp_(0, 255) * s32 + b32)   # (the clamp and the normalisation (a) applies on the way, the cast, the copy)
            calls["c " + name] = today
        torch.cuda.synchronize()
        for _ in range(3):                               # every shape of the timed window, warmed up
            for call in calls.values():
                call()
        torch.cuda.synchronize()
        us = {k: [] for k in calls}
        for _ in range(REPEATS):
            for k, call in calls.items():
                torch.cuda.synchronize()
                us[k].append(timed(theirs if k.startswith("c") else ours, call))
        torch.cuda.synchronize()
        what = {"b": "j2p_planes_to_tensor_resized f16 chw (area)"}
        for name in j.FILTERS:
            what["a " + name] = f"j2p_planes_to_tensor_resampled f16 chw, {name}"
            what["c " + name] = f"to_tensor f32 + interpolate(mode='{MODES[name]}', antialias=True) + clamp, scale, bias, cast, copy into the slot"
        for k in calls:
            emit({"what": k, "call": what[k], "source": source, "output": f"{ow}x{oh}", **stats(us[k])})
        med = {k: statistics.median(v) for k, v in us.items()}
        for name in j.FILTERS:
            calls["a " + name]()
            calls["c " + name]()
            torch.cuda.synchronize()
            diff = float((slots[0].float() - slots[1].float()).abs().max())
            a, c = "a " + name, "c " + name
            spread = max(max(us[a]) - min(us[a]), max(us[c]) - min(us[c]))
            emit({"what": "compare", "filter": name, "source": source, "output": f"{ow}x{oh}",
                  "a_against_c": "equal" if abs(med[a] - med[c]) <= spread else ("faster" if med[a] < med[c] else "slower"),
                  "a_over_b": round(med[a] / med["b"], 2) if "b" in med else None, "a_minus_c_max_abs": diff})
        del slots

# ---- batch: images per second, triangle jobs against area jobs, both into 224x224 slots ----
IN_FLIGHT, IMAGES = 3, 12
small = torch.empty((IN_FLIGHT, 3, 224, 224), dtype=torch.float16, device="cuda:0")
with j.Batch(devices=(0,), slots_per_device=IN_FLIGHT) as b:
    def run(kind, n):
        def submit(i):
            return b.submit(planes, WEIGHT, [PWEIGHT] * 3, its, width=W, height=H, tensor=small[i % IN_FLIGHT], scale=scale, bias=bias,
                            out_width=224, out_height=224, filter=kind)
        t0 = time.perf_counter()
        tickets = [submit(i) for i in range(min(IN_FLIGHT, n))]
        for i in range(n):
            b.wait(tickets[i])
            if i + IN_FLIGHT < n:
                tickets.append(submit(i + IN_FLIGHT))
        return n / (time.perf_counter() - t0)

    kinds = ["triangle", "area"]
    for kind in kinds:
        run(kind, IN_FLIGHT)
    rates = {k: [] for k in kinds}
    for r in range(rounds):
        for kind in (kinds if r % 2 == 0 else kinds[::-1]):
            rates[kind].append(run(kind, IMAGES))
    for kind in kinds:
        emit({"what": "batch", "image": f"{W}x{H} 4:2:0 joint", "output": f"f16 chw 224x224, {kind}", "iterations": its, "rounds": rounds,
              "images_per_round": IMAGES, "slots": IN_FLIGHT, "images_per_s_median": round(statistics.median(rates[kind]), 2),
              "images_per_s_best": round(max(rates[kind]), 2), "images_per_s_worst": round(min(rates[kind]), 2)})

with open(out_path, "a") as f:
    for r in lines:
        f.write(json.dumps(r) + "\n")
