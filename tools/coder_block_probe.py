#!/usr/bin/env python3
"""Host time per call of the three file coders under one build of the library, for changes that touch no device code: the `call`
rows of tools/progressive_probe.py and tools/png_probe.py (same 4096x3072 4:2:0 image, same method: one warm call, then ROUNDS
timed ones, the JPEG forms in alternating order) and the stand-alone entry points on the same data, which bring the pooled block.
Run it once per library (J2P_LIBRARY selects one), alternating the libraries; each run prints one JSON line per row, tagged with
LABEL, with a sha256 per file so that two libraries' bytes can be compared.
    [J2P_LIBRARY=lib.so] python tools/coder_block_probe.py LABEL [ITERATIONS = 50] [ROUNDS = 5] >> OUT"""
import hashlib
import io
import json
import os
import statistics
import sys
import time

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import jpeg2png_amd as j  # noqa: E402
from jpeg2png_amd import synth  # noqa: E402

W, H = 4096, 3072
SUB = (2, 2)
IMAGE = f"{W}x{H} 4:2:0"
FORMS = ("progressive", "optimize", "plain")
label = sys.argv[1]
its = int(sys.argv[2]) if len(sys.argv) > 2 else 50
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5


def spread(prefix, values, digits=3):
    return {prefix + "_median": round(statistics.median(values), digits), prefix + "_min": round(min(values), digits), prefix + "_max": round(max(values), digits)}


def emit(rec):
    print(json.dumps(dict({"library": label, "image": IMAGE, "rounds": rounds}, **rec)), flush=True)


def clock(call):
    t0 = time.perf_counter()
    data = call()
    return (time.perf_counter() - t0) * 1e3, data


def sha(data):
    return hashlib.sha256(data).hexdigest()[:16]


planes = synth.make_planes(W, H, "420", 50, seed=1240)
s = j.Solver(planes, 0.3, [0.001] * 3, its)
s.run(its)
s.sync()
for q in (75, 95):
    calls = {form: (lambda form=form: s.to_jpeg(W, H, quality=q, subsampling=SUB, progressive=form == "progressive", optimize=form == "optimize")) for form in FORMS}
    for form in FORMS:
        calls[form]()
    t, files = {form: [] for form in FORMS}, {}
    for r in range(rounds):
        for form in (FORMS if r % 2 == 0 else FORMS[::-1]):
            ms, files[form] = clock(calls[form])
            t[form].append(ms)
    rec = {"what": "call", "entry": "Solver.to_jpeg", "quality": q}
    for form in FORMS:
        rec.update(spread(form + "_ms", t[form]))
        rec[form + "_sha256"] = sha(files[form])
    emit(rec)
for bits in (8, 16):
    s.to_png(W, H, bits=bits)
    ms, data = [], b""
    for _ in range(rounds):
        m, data = clock(lambda: s.to_png(W, H, bits=bits))
        ms.append(m)
    emit(dict({"what": "call", "entry": "Solver.to_png", "bits": bits, "sha256": sha(data)}, **spread("ms", ms)))
# the stand-alone entry points on the same data: the coefficients and the samples come from the host, the block from the pool
tables = j.quality_tables(75, 3)
bw, bh = W // 8, H // 8
coef = [s.coefficients(c, tables[c], blocks_w=bw // (2 if c else 1), blocks_h=bh // (2 if c else 1), subsampling=SUB if c else (1, 1)) for c in range(3)]
pixels = np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(s.to_png(W, H, bits=8)))))
s.close()
calls = {form: (lambda form=form: j.entropy_encode(coef, W, H, tables, SUB, progressive=form == "progressive", optimize=form == "optimize")) for form in FORMS}
for form in FORMS:
    calls[form]()
t, files = {form: [] for form in FORMS}, {}
for r in range(rounds):
    for form in (FORMS if r % 2 == 0 else FORMS[::-1]):
        ms, files[form] = clock(calls[form])
        t[form].append(ms)
rec = {"what": "call", "entry": "entropy_encode", "quality": 75}
for form in FORMS:
    rec.update(spread(form + "_ms", t[form]))
    rec[form + "_sha256"] = sha(files[form])
emit(rec)
j.png_encode(pixels)
ms, data = [], b""
for _ in range(rounds):
    m, data = clock(lambda: j.png_encode(pixels))
    ms.append(m)
emit(dict({"what": "call", "entry": "png_encode", "bits": 8, "sha256": sha(data)}, **spread("ms", ms)))
