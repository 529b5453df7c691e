"""The PNG file made on the GPU (k_png_filter, k_png_count, k_png_pack, k_png_chunks, k_png_crc; j2p_png_encode, j2p_planes_to_png,
Solver.to_png, png_encode): byte for byte, and stat for stat, the plain-Python restatement of tests/png_cases.py — which
tests/test_png_cpu.py holds against zlib's inflate and PIL — on the directed cases; from a solver, the pixels PIL reads back are the
bytes of j2p_planes_to_rgb / j2p_planes_to_grey from the same solver, and the file is png_encode's of those bytes."""
import ctypes
import io

import numpy as np
import pytest

import png_cases as pc
from conftest import make_case


def case_samples(case):
    """a case's samples as png_encode takes them"""
    h, w, ch = case["height"], case["width"], case["channels"]
    a = case["samples"].view(">u2").astype(np.uint16) if case["bits"] == 16 else case["samples"]
    return a.reshape(h, w, 3) if ch == 3 else a.reshape(h, w)


def gpu_file(j, case, stats=True):
    return j.png_encode(case_samples(case), bits=case["bits"], filter=case["filter"], block_bytes=case["block_bytes"],
                        idat_bytes=case["idat_bytes"], stats=stats)


@pytest.fixture(scope="module")
def restated():
    """{name: (case, file, report)} of the restatement, computed once"""
    return {name: (case,) + pc.encode_case(case) for name, case in pc.directed_cases().items()}


CASE_NAMES = sorted(pc.directed_cases())


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_png_encode_is_the_restatement_byte_for_byte(lib, restated, name):
    import jpeg2png_amd as j
    case, want, report = restated[name]
    got, stats = gpu_file(j, case)
    assert stats == report["stats"], name
    assert got == want, (name, len(got), len(want), next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), None))


@pytest.mark.gpu
def test_every_filter_wins_a_row_and_a_tie_goes_to_the_lowest(lib, restated):
    import jpeg2png_amd as j
    case, _want, report = restated["filters"]
    _file, stats = gpu_file(j, case)
    assert all(n > 0 for n in stats["rows"]) and sum(stats["rows"]) == case["height"]
    # row 0 of any image: none and up give the same bytes, and none is chosen — and a black image ties all five in every row
    assert report["filtered"][0] == 0
    black, stats = j.png_encode(np.zeros((5, 9, 3), np.uint8), block_bytes=32, idat_bytes=32, stats=True)
    assert stats["rows"] == [5, 0, 0, 0, 0] and black == pc.encode(np.zeros((5, 27), np.uint8), 9, 5, block_bytes=32, idat_bytes=32)[0]
    for f in range(5):
        fixed = dict(case, filter=f)
        got, stats = gpu_file(j, fixed)
        assert stats["rows"] == [case["height"] if k == f else 0 for k in range(5)]
        assert got == pc.encode_case(fixed)[0], f


@pytest.mark.gpu
def test_more_than_one_tile_of_a_block_and_default_sizes(lib):
    """a 2500-byte block is three trips of its workgroup (1024 positions each): runs that cross the trips, a match whose length lies
    beyond its trip, and the default block and chunk sizes on 77 KB of noise and flats"""
    import jpeg2png_amd as j
    rng = np.random.default_rng(11)
    row = np.concatenate([rng.integers(0, 256, 1000), np.full(60, 5), rng.integers(0, 4, 900), np.full(700, 200), rng.integers(0, 256, 339)])
    case = {"samples": row.astype(np.uint8).reshape(1, -1), "width": 2999, "height": 1, "bits": 8, "channels": 1, "filter": 0,
            "block_bytes": 2500, "idat_bytes": 1000}
    got, stats = gpu_file(j, case)
    want, report = pc.encode_case(case)
    assert stats == report["stats"] and got == want
    img = rng.integers(0, 256, size=(150, 170, 3)).astype(np.uint8)
    img[20:60, 30:140] = (10, 200, 90)
    case = {"samples": img.reshape(150, -1), "width": 170, "height": 150, "bits": 8, "channels": 3, "filter": None, "block_bytes": 0, "idat_bytes": 0}
    got, stats = gpu_file(j, case)
    want, report = pc.encode_case(case)
    assert stats == report["stats"] and stats["blocks"] == 2 and got == want


@pytest.mark.gpu
def test_espace_reports_the_size_and_touches_nothing(lib, restated):
    import jpeg2png_amd as j
    case, want, _report = restated["rgb_10x7"]
    a = np.ascontiguousarray(case_samples(case))
    spec = j._c_png(10, 7, 8, None, case["block_bytes"], case["idat_bytes"])
    size = ctypes.c_size_t(0)
    buf = np.full(len(want) + 8, 0xA5, np.uint8)
    assert lib.j2p_png_encode(0, ctypes.byref(spec), a.ctypes.data, 3, buf.ctypes.data, len(want) - 1, ctypes.byref(size), None) == j.J2P_ESPACE
    assert size.value == len(want) and (buf == 0xA5).all()
    size = ctypes.c_size_t(0)
    assert lib.j2p_png_encode(0, ctypes.byref(spec), a.ctypes.data, 3, None, 0, ctypes.byref(size), None) == j.J2P_ESPACE
    assert size.value == len(want)
    assert lib.j2p_png_encode(0, ctypes.byref(spec), a.ctypes.data, 3, buf.ctypes.data, len(want), ctypes.byref(size), None) == 0
    assert buf[:len(want)].tobytes() == want and (buf[len(want):] == 0xA5).all()


@pytest.mark.gpu
def test_refusals(lib):
    import jpeg2png_amd as j
    ok = np.zeros((4, 4, 3), np.uint8)
    for kw, what in (({"block_bytes": 15}, "block_bytes"), ({"block_bytes": (1 << 24) + 1}, "block_bytes"), ({"idat_bytes": 8}, "idat_bytes"),
                     ({"filter": 5}, "filter"), ({"filter": -2}, "filter")):
        with pytest.raises(j.J2PError, match=what):
            j.png_encode(ok, **kw)
    with pytest.raises(j.J2PError, match="uint16"):
        j.png_encode(ok, bits=16)
    with pytest.raises(j.J2PError, match="shape"):
        j.png_encode(np.zeros((4, 4, 2), np.uint8))
    # more deflate blocks than J2P_PNG_BLOCKS_MAX (2^20): 4097 rows of 4097 bytes in blocks of 16 — refused before any block is taken
    takes = lib.j2p_pool_thread_takes()
    with pytest.raises(j.J2PError, match="deflate blocks"):
        j.png_encode(np.zeros((4097, 4096), np.uint8), block_bytes=16)
    assert lib.j2p_pool_thread_takes() == takes
    spec = j._c_png(4, 4, 12)
    size = ctypes.c_size_t(0)
    assert lib.j2p_png_encode(0, ctypes.byref(spec), ok.ctypes.data, 3, None, 0, ctypes.byref(size), None) == -1
    assert b"bits" in lib.j2p_last_error()
    assert lib.j2p_png_encode(0, None, ok.ctypes.data, 3, None, 0, ctypes.byref(size), None) == -1
    assert lib.j2p_planes_to_png(None, 3, ctypes.byref(spec), None, 0, ctypes.byref(size)) == -1


def solver_bytes(lib, j, solvers, n, w, h, bits):
    """the bytes of j2p_planes_to_rgb / j2p_planes_to_grey from the same solver(s)"""
    refs = (j._CPlaneRef * 3)()
    for c in range(n):
        refs[c] = j._CPlaneRef(solvers[c]._h, 0) if len(solvers) == 3 else j._CPlaneRef(solvers[0]._h, c)
    lib.j2p_planes_to_rgb.argtypes = lib.j2p_planes_to_grey.argtypes = [ctypes.POINTER(j._CPlaneRef), ctypes.c_uint, ctypes.c_uint, ctypes.c_uint,
                                                                        ctypes.c_void_p]
    out = np.empty((h, w * n * bits // 8), np.uint8)
    assert getattr(lib, "j2p_planes_to_rgb" if n == 3 else "j2p_planes_to_grey")(refs, w, h, bits, out.ctypes.data) == 0
    return out


def pil_bytes(file, n, bits):
    """a file's pixels as PIL reads them, in the layout of the samples (16-bit colour: PIL keeps the high bytes)"""
    from PIL import Image
    im = Image.open(io.BytesIO(file))
    im.load()
    a = np.asarray(im)
    if bits == 16 and n == 1:
        return a.astype(">u2").view(np.uint8).reshape(a.shape[0], -1)
    return a.reshape(a.shape[0], -1)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["joint", "separate", "grey"])
def test_to_png_holds_the_solvers_own_samples(lib, kind):
    import jpeg2png_amd as j
    w, h, its = 45, 38, 6
    planes = make_case(48, 48, "420", 30, seed=21, y_only=kind == "grey")
    if kind == "separate":
        solvers = [j.Solver([p], 0.3, [0.001], its) for p in planes]
    else:
        solvers = [j.Solver(planes, 0.3, [0.001] * len(planes), its)]
    try:
        for s in solvers:
            s.run(its)
        n = 1 if kind == "grey" else 3
        for bits in (8, 16):
            want = solver_bytes(lib, j, solvers, n, w, h, bits)
            file = solvers[0].to_png(w, h, bits=bits, others=solvers[1:], block_bytes=1000, idat_bytes=300)
            got = pil_bytes(file, n, bits)
            assert np.array_equal(got, want if not (bits == 16 and n == 3) else want[:, 0::2]), (kind, bits)
            samples = want.view(">u2").astype(np.uint16) if bits == 16 else want
            samples = samples.reshape(h, w, 3) if n == 3 else samples.reshape(h, w)
            assert file == j.png_encode(samples, bits=bits, block_bytes=1000, idat_bytes=300), (kind, bits)
            assert file == pc.encode(want, w, h, bits=bits, channels=n, block_bytes=1000, idat_bytes=300)[0], (kind, bits)
        # the defaults, and a fixed filter
        want = solver_bytes(lib, j, solvers, n, w, h, 8)
        assert solvers[0].to_png(w, h, others=solvers[1:]) == pc.encode(want, w, h, channels=n)[0]
        assert solvers[0].to_png(w, h, others=solvers[1:], filter="paeth") == pc.encode(want, w, h, channels=n, filter=4)[0]
    finally:
        for s in solvers:
            s.close()


@pytest.mark.gpu
def test_to_png_espace_second_call_and_refusals(lib):
    import jpeg2png_amd as j
    w, h = 45, 38
    planes = make_case(48, 48, "420", 30, seed=22)
    with j.Solver(planes, 0.3, [0.001] * 3, 3) as s:
        s.run(3)
        file = s.to_png(w, h)
        room = s.output_scratch_bytes()
        assert room > 0
        hip = j.hip_runtime()
        free = [ctypes.c_size_t(0), ctypes.c_size_t(0)]
        total = ctypes.c_size_t(0)
        assert hip.hipMemGetInfo(ctypes.byref(free[0]), ctypes.byref(total)) == 0
        assert s.to_png(w, h) == file
        assert hip.hipMemGetInfo(ctypes.byref(free[1]), ctypes.byref(total)) == 0
        assert s.output_scratch_bytes() == room and free[0].value == free[1].value, "the second call of the same size allocated"
        refs = (j._CPlaneRef * 3)(*[j._CPlaneRef(s._h, c) for c in range(3)])
        spec = j._c_png(w, h)
        size = ctypes.c_size_t(0)
        buf = np.full(len(file) + 8, 0xA5, np.uint8)
        assert lib.j2p_planes_to_png(refs, 3, ctypes.byref(spec), buf.ctypes.data, len(file) - 1, ctypes.byref(size)) == j.J2P_ESPACE
        assert size.value == len(file) and (buf == 0xA5).all()
        assert lib.j2p_planes_to_png(refs, 3, ctypes.byref(spec), buf.ctypes.data, buf.size, ctypes.byref(size)) == 0
        assert buf[:size.value].tobytes() == file and (buf[size.value:] == 0xA5).all()
        with pytest.raises(j.J2PError, match="not inside"):
            s.to_png(49, 38)
        with pytest.raises(j.J2PError, match="bits"):
            s.to_png(w, h, bits=12)
        assert s.to_png(w, h) == file
    # a band solver is refused, as by j2p_planes_to_rgb
    big = make_case(48, 96, "444", 30, seed=23, y_only=True)
    with j.Solver(big, 0.3, [0.001], 2, band=(0, 48)) as s:
        with pytest.raises(j.J2PError, match="whole-canvas"):
            s.to_png(48, 48)
    # png_encode through the pool: a second call of the same size allocates nothing
    a = np.random.default_rng(3).integers(0, 256, size=(64, 64, 3)).astype(np.uint8)
    first = j.png_encode(a)
    assert hip.hipMemGetInfo(ctypes.byref(free[0]), ctypes.byref(total)) == 0
    assert j.png_encode(a) == first
    assert hip.hipMemGetInfo(ctypes.byref(free[1]), ctypes.byref(total)) == 0
    assert free[0].value == free[1].value


# ---- batch engine ----
PNG = dict(bits=8, block_bytes=200, idat_bytes=100)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["planes", "samples", "file"])
def test_batch_png_jobs_equal_to_png(lib, kind):
    """the smallest job that takes every path (job_refusal_cases: 4:2:0, image 30x13, 2 iterations), from coefficient planes, decoded
    samples and a JPEG file, joint and separate, 8 and 16 bits, and component 0 alone as a greyscale file"""
    import jpeg2png_amd as j
    import job_refusal_cases as rc
    from test_job_matrix_gpu import Source, W, H, N
    torch = None
    if kind == "samples":
        import torch
    source = Source(j, torch, kind)
    args = (source.planes, rc.WEIGHT, rc.PWEIGHT, N)
    with j.Batch(devices=(0,), slots_per_device=2) as b:
        tickets = {(separate, bits): b.submit(*args, separate=separate, width=W, height=H, png=dict(PNG, bits=bits), **source.keywords)
                   for separate in (False, True) for bits in (8, 16)}
        grey = b.submit(source.planes[:1], rc.WEIGHT, rc.PWEIGHT[:1], N, width=W, height=H, png=dict(PNG, filter="up"),
                        **{k: (v[:1] if k == "samples" else v) for k, v in source.keywords.items()})
        got = {key: b.wait(t) for key, t in tickets.items()}
        got_grey = b.wait(grey)
    for separate in (False, True):
        ss = source.solvers(separate)
        try:
            for bits in (8, 16):
                assert got[(separate, bits)] == ss[0].to_png(W, H, bits=bits, others=ss[1:], block_bytes=200, idat_bytes=100), (kind, separate, bits)
            if separate:
                assert got_grey == ss[0].to_png(W, H, filter="up", block_bytes=200, idat_bytes=100), kind
        finally:
            for s in ss:
                s.close()
    assert pil_bytes(got[(False, 8)], 3, 8).shape == (H, W * 3) and pil_bytes(got_grey, 1, 8).shape == (H, W)


@pytest.mark.gpu
def test_batch_png_refusals_get_no_ticket(lib):
    import jpeg2png_amd as j
    import job_refusal_cases as rc
    W, H, N = rc.WIDTH, rc.HEIGHT, rc.ITERATIONS
    args = (rc.planes(), rc.WEIGHT, rc.PWEIGHT, N)
    with j.Batch(devices=(0,), slots_per_device=1) as b:
        for kw, what in ((dict(png=dict(PNG), bits=8), "excludes"), (dict(png=dict(PNG), tile=True), "excludes"),
                         (dict(png=dict(PNG), jpeg=dict(quality=90)), "excludes"), (dict(png=dict(PNG, bits=12)), "bits"),
                         (dict(png=dict(PNG, block_bytes=8)), "block_bytes"), (dict(png=dict(PNG, filter=7)), "filter"),
                         (dict(png=dict(PNG, quality=3)), "dict")):
            with pytest.raises(j.J2PError, match=what):
                b.submit(*args, **dict(dict(width=W, height=H), **kw))
            assert not b._pending, kw
        with pytest.raises(j.J2PError, match="three planes"):
            b.submit(rc.planes()[:2], rc.WEIGHT, rc.PWEIGHT[:2], N, width=W, height=H, png=dict(PNG))
        # the library's own checks, which the binding cannot reach: a row-tiled job, sample output next to the file, a size that is
        # not the job's — each before any device work, and no ticket is written
        job = j._CJob()
        keep = j._job_record(job, rc.planes(), rc.WEIGHT, rc.PWEIGHT, N, j._Wanted(**dict({f: None for f in j._Wanted._fields}, separate=False, tile=False, bits=0, layout="chw")), None, None)
        job.out_w, job.out_h = W, H
        spec, size, ticket = j._c_png(W, H, **PNG), ctypes.c_size_t(0), ctypes.c_int(-7)
        buf = np.zeros(4096, np.uint8)

        def submit():
            return lib.j2p_batch_submit_png(b._h, ctypes.byref(job), None, ctypes.byref(spec), buf.ctypes.data, buf.size, ctypes.byref(size), ctypes.byref(ticket))
        job.tile = 1
        assert submit() == -1 and b"row-tiled" in lib.j2p_last_error() and ticket.value == -7
        job.tile, job.out_bits = 0, 8
        assert submit() == -1 and b"out_bits" in lib.j2p_last_error() and ticket.value == -7
        job.out_bits, job.out_w = 0, W - 1
        assert submit() == -1 and b"the PNG is" in lib.j2p_last_error() and ticket.value == -7
        job.out_w = W
        assert lib.j2p_batch_submit_png(b._h, ctypes.byref(job), None, None, buf.ctypes.data, buf.size, ctypes.byref(size), ctypes.byref(ticket)) == -1
        assert lib.j2p_batch_submit_file_png(b._h, ctypes.byref(job), None, 0, ctypes.byref(spec), buf.ctypes.data, buf.size, ctypes.byref(size),
                                             ctypes.byref(ticket)) == -1 and ticket.value == -7
        # too little room: the job fails with J2P_ESPACE and the size it needs; its neighbour does not
        small = b.submit(*args, width=W, height=H, png=dict(PNG, capacity=40))
        fine = b.submit(*args, width=W, height=H, png=dict(PNG))
        with pytest.raises(j.J2PError, match="the file has") as e:
            b.wait(small)
        assert e.value.code == j.J2P_ESPACE
        assert submit() == 0
        assert lib.j2p_batch_wait(b._h, ticket.value) == 0
        assert buf[:size.value].tobytes() == b.wait(fine)
        del keep
