#!/usr/bin/env python3
"""Multi-output tensor resampling (j2p_planes_to_tensors_resampled) against the loop of single calls it replaces, on one
4096x3072 4:2:0 image solved jointly, f16 CHW outputs with scale and bias, triangle and cubic.  The BASELINE is another build
of the library — the parent commit's, given as PARENT: build it in a checkout of that commit (python -m jpeg2png_amd.buildlib)
and copy its libjpeg2png_amd.so to ab/ — loaded into the same process (jpeg2png_amd.library), with a solver of its own on the
same planes; never this library's own loop, which is measured too but only for information.
  set A, multi-crop: 2 x 224x224 from boxes of half the image's area and 8 x 96x96 from boxes of 15 % of it, all overlapping;
  set B, pyramid:    2048x1536, 1024x768, 512x384 and 256x192 of the whole image;
  single:            the single call's four cases of tools/filter_probe.py, this library against the parent and — the spread —
                     the parent against itself (two solvers of the parent library, alternated like the others);
  batch:             views per second through Batch at ITERATIONS iterations, jobs with the 10 outputs of set A against 10
                     single-output jobs per image on the parent.
Times are device events on the solver's stream around LAUNCHES back-to-back calls (a "call" of a loop is the whole loop), REPEATS
repeats, the contenders of a comparison taken in turn within every repeat.  Appends one JSON line per measurement to OUT
(default profiles/multi_outputs.jsonl) and prints them; COMMIT, when given, goes into every line.
    python tools/outputs_probe.py PARENT [ITERATIONS] [ROUNDS] [OUT] [COMMIT]"""
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
LAUNCHES, REPEATS = 20, 7
SET_A = [((1200 * i, 900 * i, 2896, 2172), (224, 224)) for i in range(2)] + \
        [((300 * i + 17, 200 * i + 9, 1586, 1190), (96, 96)) for i in range(8)]
SET_B = [(WHOLE, (2048 >> k, 1536 >> k)) for k in range(4)]
SINGLE = [(WHOLE, (224, 224)), (WHOLE, (1024, 768)), (WHOLE, (4095, 3071)), ((0, 0, 640, 480), (1024, 768))]

args = sys.argv[1:]
if not args:
    sys.exit(__doc__)
parent_path = os.path.abspath(args[0])
its = int(args[1]) if len(args) > 1 else 50
rounds = int(args[2]) if len(args) > 2 else 3
out_path = args[3] if len(args) > 3 else os.path.join(ROOT, "profiles", "multi_outputs.jsonl")
commit = {"commit": args[4]} if len(args) > 4 else {}
lines = []


def emit(rec):
    rec = {**commit, **rec}
    lines.append(rec)
    print(json.dumps(rec), flush=True)


if not os.path.exists(parent_path):
    sys.exit(f"outputs_probe: no parent library at {parent_path}")
if not torch.cuda.is_available():
    sys.exit("outputs_probe needs a GPU: nothing here is measured without one")

planes = synth.make_planes(W, H, "420", 50, seed=1240)
scale = [1.0 / (255.0 * s) for s in (0.229, 0.224, 0.225)]
bias = [-m / s for m, s in zip((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))]
dev = torch.device("cuda", 0)


class Side:
    """one library's solver on the planes, solved once, and the calls on it"""

    def __init__(self, name, path=None):
        self.name = name
        if path is None:
            self.s = j.Solver(planes, WEIGHT, [PWEIGHT] * 3, 1)
        else:
            with j.library(path):
                self.s = j.Solver(planes, WEIGHT, [PWEIGHT] * 3, 1)
        self.s.run(1)
        self.s.sync()
        self.lib = self.s._lib
        self.refs = (j._CPlaneRef * 3)(*[j._CPlaneRef(self.s._h, c) for c in range(3)])
        self.stream = torch.cuda.ExternalStream(self.s.stream(), device=dev)

    def loop(self, views, code, tensors):
        """the loop of single calls"""
        pairs = [(j._CResample(*box, ow, oh, code), j._c_tensor(t, 3, ow, oh, "chw", scale, bias)) for (box, (ow, oh)), t in zip(views, tensors)]

        def call():
            for r, ct in pairs:
                j._check(self.lib.j2p_planes_to_tensor_resampled(self.refs, 3, W, H, ctypes.byref(r), ctypes.byref(ct)))
        return call

    def multi(self, views, code, tensors):
        items = (j._COutput * len(views))()
        for i, ((box, (ow, oh)), t) in enumerate(zip(views, tensors)):
            items[i].r = j._CResample(*box, ow, oh, code)
            items[i].t = j._c_tensor(t, 3, ow, oh, "chw", scale, bias)
        return lambda: j._check(self.lib.j2p_planes_to_tensors_resampled(self.refs, 3, W, H, len(views), items))


def timed(stream, call):
    """microseconds per call: LAUNCHES calls between two events on `stream`"""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record(stream)
    for _ in range(LAUNCHES):
        call()
    end.record(stream)
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / LAUNCHES


def contest(calls):
    """calls: {name: (stream, call)}; every repeat takes each contender once, in turn.  Returns {name: [us per repeat]}"""
    torch.cuda.synchronize()
    for _ in range(3):
        for _, call in calls.values():
            call()
    torch.cuda.synchronize()
    us = {k: [] for k in calls}
    for r in range(REPEATS):
        order = list(calls) if r % 2 == 0 else list(calls)[::-1]
        for k in order:
            torch.cuda.synchronize()
            us[k].append(timed(*calls[k]))
    torch.cuda.synchronize()
    return us


def stats(v):
    return {"us_median": round(statistics.median(v), 2), "us_min": round(min(v), 2), "us_max": round(max(v), 2)}


def alloc(views):
    return [torch.zeros((3, oh, ow), dtype=torch.float16, device=dev) for _, (ow, oh) in views]


new, parent, parent2 = Side("new"), Side("parent", parent_path), Side("parent again", parent_path)
base = {"image": f"{W}x{H} 4:2:0 joint", "dtype": "f16 chw", "calls_per_repeat": LAUNCHES, "repeats": REPEATS}

# ---- the single call: new against parent, and the spread of parent against parent ----
spread = {}
for box, (ow, oh) in SINGLE:
    view = [(box, (ow, oh))]
    for name, code in j.FILTERS.items():
        ts = [alloc(view) for _ in range(3)]
        us = contest({"new": (new.stream, new.loop(view, code, ts[0])), "parent": (parent.stream, parent.loop(view, code, ts[1])),
                      "parent again": (parent2.stream, parent2.loop(view, code, ts[2]))})
        torch.cuda.synchronize()
        same = bool(torch.equal(ts[0][0], ts[1][0]))
        med = {k: statistics.median(v) for k, v in us.items()}
        pp = abs(med["parent"] - med["parent again"]) / med["parent"]
        spread[(ow, oh, name)] = pp
        emit({"what": "single", **base, "box": list(box), "output": f"{ow}x{oh}", "filter": name, **{k.replace(" ", "_"): stats(v) for k, v in us.items()},
              "new_over_parent": round(med["new"] / med["parent"], 4), "parent_again_over_parent": round(med["parent again"] / med["parent"], 4),
              "within_spread": bool(abs(med["new"] - med["parent"]) / med["parent"] <= max(pp, (max(us["parent"]) - min(us["parent"])) / med["parent"])),
              "same_bits": same})
        del ts

# ---- the sets: one multi call against the parent's loop ----
for set_name, views in (("A multi-crop", SET_A), ("B pyramid", SET_B)):
    for name, code in j.FILTERS.items():
        ts = [alloc(views) for _ in range(4)]
        us = contest({"multi": (new.stream, new.multi(views, code, ts[0])), "parent loop": (parent.stream, parent.loop(views, code, ts[1])),
                      "parent loop again": (parent2.stream, parent2.loop(views, code, ts[2])), "new loop": (new.stream, new.loop(views, code, ts[3]))})
        torch.cuda.synchronize()
        same = all(bool(torch.equal(a, b)) for a, b in zip(ts[0], ts[1]))
        med = {k: statistics.median(v) for k, v in us.items()}
        pp = max(abs(med["parent loop"] - med["parent loop again"]), max(us["parent loop"]) - min(us["parent loop"])) / med["parent loop"]
        emit({"what": "set", **base, "set": set_name, "views": [f"{ow}x{oh} of {bw}x{bh}" for (_, _, bw, bh), (ow, oh) in views], "filter": name,
              **{k.replace(" ", "_"): stats(v) for k, v in us.items()}, "multi_over_parent_loop": round(med["multi"] / med["parent loop"], 4),
              "parent_spread": round(pp, 4), "faster_beyond_spread": bool(med["multi"] < med["parent loop"] * (1 - pp)), "same_bits": same})
        del ts

# ---- batch: views per second, jobs with 10 outputs against 10 single-output jobs per image on the parent ----
IN_FLIGHT, IMAGES = 3, 8
views = SET_A
slots = [alloc(views) for _ in range(IN_FLIGHT)]


def run_multi(b, n):
    def submit(i):
        return b.submit(planes, WEIGHT, [PWEIGHT] * 3, its, width=W, height=H, outputs=[
            {"tensor": t, "box": box, "out_width": ow, "out_height": oh, "filter": "triangle", "scale": scale, "bias": bias}
            for (box, (ow, oh)), t in zip(views, slots[i % IN_FLIGHT])])
    t0 = time.perf_counter()
    tickets = [submit(i) for i in range(min(IN_FLIGHT, n))]
    for i in range(n):
        b.wait(tickets[i])
        if i + IN_FLIGHT < n:
            tickets.append(submit(i + IN_FLIGHT))
    return n * len(views) / (time.perf_counter() - t0)


def run_single(b, n):
    """every view a job of its own: the image is solved once per view"""
    todo = [(i, v) for i in range(n) for v in range(len(views))]

    def submit(k):
        i, v = todo[k]
        box, (ow, oh) = views[v]
        return b.submit(planes, WEIGHT, [PWEIGHT] * 3, its, width=W, height=H, tensor=slots[k % IN_FLIGHT][v], box=box, out_width=ow, out_height=oh,
                        filter="triangle", scale=scale, bias=bias)
    t0 = time.perf_counter()
    tickets = [submit(k) for k in range(min(IN_FLIGHT, len(todo)))]
    for k in range(len(todo)):
        b.wait(tickets[k])
        if k + IN_FLIGHT < len(todo):
            tickets.append(submit(k + IN_FLIGHT))
    return len(todo) / (time.perf_counter() - t0)


with j.library(parent_path):
    b_parent = j.Batch(devices=(0,), slots_per_device=IN_FLIGHT)
with j.Batch(devices=(0,), slots_per_device=IN_FLIGHT) as b_new, b_parent:
    kinds = {"jobs of 10 outputs": lambda n: run_multi(b_new, n), "parent: 10 jobs per image": lambda n: run_single(b_parent, n),
             "10 jobs per image": lambda n: run_single(b_new, n)}
    for run in kinds.values():
        run(1)
    rates = {k: [] for k in kinds}
    for r in range(rounds):
        for k in (list(kinds) if r % 2 == 0 else list(kinds)[::-1]):
            rates[k].append(kinds[k](IMAGES if k == "jobs of 10 outputs" else 2))
    for k in kinds:
        emit({"what": "batch", "image": f"{W}x{H} 4:2:0 joint", "views": "set A, triangle, f16 chw", "kind": k, "iterations": its, "rounds": rounds,
              "slots": IN_FLIGHT, "views_per_s_median": round(statistics.median(rates[k]), 1), "views_per_s_best": round(max(rates[k]), 1),
              "views_per_s_worst": round(min(rates[k]), 1)})

with open(out_path, "a") as f:
    for r in lines:
        f.write(json.dumps(r) + "\n")
