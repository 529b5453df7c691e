"""The block that moves in the middle of a call.  The three file coders (j2p_encode_scan, j2p_encode_progressive, j2p_png_write) ask
their `memory` callback for one device block several times, the earlier times with a guess for the part whose size is not known yet;
when a later request is larger the block is ANOTHER one, its contents are gone, and the coder's j2p_coder_block
(jpeg2png_amd/csrc/j2p_coder_block.h) queues again every stage the coder had handed it: coefficients, lengths and streams for the
JPEG files, the filtered rows for the PNG.  tests/test_coder_block_cpu.py holds that rule by itself; here every later request of
every coder moves its block on purpose, through both callbacks — the pooled block of the stand-alone entry points and a solver's
scratch, which grows in steps of 256 KiB — and the file is held byte for byte against the restatement all the same.

That the block moved is seen from j2p_pool_thread_takes(): a call took 1 + moves blocks.  Every test empties the pool first
(a cached block of another size would be taken in place of a fresh one and change the count) and asserts the count of every call
it makes, so a test that no longer reaches its path fails.  tests/test_regrow_cpu.py holds the arithmetic of the sizes."""
import ctypes
import struct

import numpy as np
import pytest

import entropy_cases as ec
import huffman_cases as hc
import png_cases as pc
import regrow_cases as rg

J2P_ESPACE = -5


def counted(lib, call):
    """(what call() returns, the blocks this thread took from the pool meanwhile)"""
    before = lib.j2p_pool_thread_takes()
    out = call()
    return out, lib.j2p_pool_thread_takes() - before


def png_call(lib, samples, room, **spec):
    """j2p_png_encode itself, once, into `room` bytes -> (file, stats as png_encode gives them)"""
    import jpeg2png_amd as j
    a = np.ascontiguousarray(samples)
    height, width = a.shape[:2]
    c_spec = j._c_png(width, height, **spec)
    st, size, buf = j._CPngStats(), ctypes.c_size_t(0), np.zeros(room, np.uint8)
    rc = lib.j2p_png_encode(0, ctypes.byref(c_spec), a.ctypes.data, 3 if a.ndim == 3 else 1, buf.ctypes.data, room, ctypes.byref(size), ctypes.byref(st))
    assert rc == 0, lib.j2p_last_error().decode()
    return buf[:size.value].tobytes(), {"rows": list(st.rows), "blocks": st.blocks, "literals": st.literals, "matches": st.matches,
                                        "stream_bytes": st.stream_bytes, "adler": st.adler}


@pytest.mark.gpu
def test_png_encode_whose_stream_outgrows_the_guess(lib):
    """j2p_png_encode, the second request, which runs the one stage (filter) again — with the adaptive filter, whose rows per filter
    type are counted in the block (chosen[], zeroed inside filter()): the second call gets the first call's blocks back from the
    pool, counts and all, and must report the same rows"""
    lib.j2p_pool_trim()
    image = rg.noise_image()
    want, report = pc.encode(image.reshape(48, -1), 48, 48, idat_bytes=16)
    (got, stats), took = counted(lib, lambda: png_call(lib, image, 1 << 16, idat_bytes=16))
    assert took == 2, "the block did not move"
    assert stats == report["stats"] and sum(stats["rows"]) == 48 and got == want
    # once more: the pool now holds both blocks, and gives the small one first again
    (again, stats), took = counted(lib, lambda: png_call(lib, image, 1 << 16, idat_bytes=16))
    assert took == 2 and again == want and stats == report["stats"]
    # the control: zeros deflate to next to nothing, and the first block is large enough
    lib.j2p_pool_trim()
    zeros = np.zeros_like(image)
    (got, stats), took = counted(lib, lambda: png_call(lib, zeros, 1 << 16, idat_bytes=16))
    want, report = pc.encode(zeros.reshape(48, -1), 48, 48, idat_bytes=16)
    assert took == 1 and got == want and stats == report["stats"]


def jpeg_takes(case, file, counting=False):
    """the blocks j2p_encode_scan takes for `case`, by the sizes of the restatement's file"""
    return rg.takes(rg.jpeg_requests(case, *rg.scan_sizes(file), counting=counting))


@pytest.mark.gpu
def test_entropy_encode_whose_stream_outgrows_both_guesses(lib):
    """j2p_entropy_encode, the second and the third request: the coefficients and the lengths are queued again, then those and the
    stream — 32x32 grey blocks of 63 coefficients of 1023: 3280 bytes of stream for a guess of 512, and 1744 FF bytes in them for
    a guess of 461"""
    import test_entropy_gpu as teg
    case = rg.heavy_case()
    want = ec.encode(case["coefficients"], 32, 32, case["quant"])
    assert jpeg_takes(case, want) == 3
    lib.j2p_pool_trim()
    (rc, size, buf), took = counted(lib, lambda: teg.c_call(lib, case, len(want) + 64))
    assert rc == 0, lib.j2p_last_error().decode()
    assert took == 3, "the block did not move twice"
    assert buf[:size].tobytes() == want and (buf[size:] == 0xA5).all()
    # the control: a sparse image of the same size — its stream still outgrows the first guess (16 blocks are a small grid), its FF
    # bytes do not outgrow theirs
    sparse = rg.sparse_case()
    want = ec.encode(sparse["coefficients"], 32, 32, sparse["quant"])
    assert jpeg_takes(sparse, want) == 2
    lib.j2p_pool_trim()
    (rc, size, buf), took = counted(lib, lambda: teg.c_call(lib, sparse, len(want) + 64))
    assert rc == 0 and took == 2 and buf[:size].tobytes() == want


@pytest.mark.gpu
def test_progressive_encode_whose_stream_outgrows_both_guesses(lib):
    """j2p_entropy_encode_progressive, the second and the third request, on the same blocks: six scans whose streams together have
    1392 bytes for a guess of 512, and 376 FF bytes in them for a guess of 343.  What is queued again reaches over all scans: the
    coefficients with every AC scan's flags and EOB runs, every scan's lengths, every scan's stream"""
    import progressive_cases as prc
    import test_progressive_gpu as tpg
    case = rg.heavy_case()
    want, report = prc.encode_case(case)
    assert rg.takes(rg.progressive_requests(case, report)) == 3
    lib.j2p_pool_trim()
    (rc, size, buf), took = counted(lib, lambda: tpg.c_call(lib, case, len(want) + 64))
    assert rc == 0, lib.j2p_last_error().decode()
    assert took == 3, "the block did not move twice"
    assert buf[:size].tobytes() == want and (buf[size:] == 0xA5).all()
    # the control: the sparse image's streams outgrow the first guess, its FF bytes (none) not theirs
    sparse = rg.sparse_case()
    want, report = prc.encode_case(sparse)
    assert rg.takes(rg.progressive_requests(sparse, report)) == 2
    lib.j2p_pool_trim()
    (rc, size, buf), took = counted(lib, lambda: tpg.c_call(lib, sparse, len(want) + 64))
    assert rc == 0 and took == 2 and buf[:size].tobytes() == want


@pytest.mark.gpu
def test_optimised_tables_survive_both_moves(lib):
    """the same blocks with J2P_JPEG_OPTIMIZE: the symbol counts are on the host before the second request, the block that held them
    is gone after it, and the tables made from them code the stream that is packed a second and a third time.  The second request
    moves the block (1388 bytes of stream for a guess of 512) and the third does (380 FF bytes for a guess of 342): three takes"""
    import test_huffman_gpu as thg
    case = rg.heavy_case()
    want, report = hc.encode_report(case["coefficients"], 32, 32, case["quant"])
    assert rg.scan_sizes(want) == (1388, 380) and jpeg_takes(case, want, counting=True) == 3
    lib.j2p_pool_trim()
    (rc, size, buf), took = counted(lib, lambda: thg.c_call_ex(lib, case, len(want) + 64, 1))
    assert rc == 0, lib.j2p_last_error().decode()
    assert took == 3, "the block did not move twice"
    assert buf[:size].tobytes() == want and (buf[size:] == 0xA5).all()
    # ... and the counts the caller asks for are the ones taken before the moves
    import jpeg2png_amd as j
    lib.j2p_pool_trim()
    (got, stats), took = counted(lib, lambda: j.entropy_encode(case["coefficients"], 32, 32, case["quant"], optimize=True, stats=True))
    assert took == 3 and got == want and stats["scan_bits"] == report["bits"] and stats["stuffed_bytes"] == report["stuffed"]
    thg.same_counts(stats, report, "heavy")


def plane_refs(j, s):
    return (j._CPlaneRef * 3)(*[j._CPlaneRef(s._h, c) for c in range(3)])


@pytest.mark.gpu
@pytest.mark.parametrize("orientation", [1, 6], ids=["as_solved", "turned"])
def test_solver_scratch_moves_under_the_png_coder(lib, orientation):
    """j2p_planes_to_png in a solver's scratch: 16-bit samples of a 320x240 solve deflate to about nine tenths of their bytes, and
    with 16 data bytes per IDAT chunk the second request is past the 256 KiB the first was rounded up to.  The move is seen twice:
    a call without a buffer answers J2P_ESPACE between the two requests and leaves the scratch smaller than the call that writes
    the file, which takes one more block.  Oriented (6: a quarter turn), filter()'s second run reads the upright planes — a block of
    their own, taken by the first call — again."""
    import jpeg2png_amd as j
    from jpeg2png_amd import synth
    from test_png_gpu import solver_bytes
    lib.j2p_pool_trim()
    w, h = 320, 240
    with j.Solver(synth.make_planes(w, h, "420", 30, seed=320), 0.3, [0.001] * 3, 2) as s:
        s.run(2)
        uw, uh = w, h
        if orientation != 1:
            s.set_orientation(orientation, w, h)
            uw, uh = j.upright_size(orientation, w, h)
        refs, spec, size = plane_refs(j, s), j._c_png(uw, uh, 16, "none", 0, 16), ctypes.c_size_t(0)
        assert s.output_scratch_bytes() == 0 and s.upright_bytes() == 0
        rc, took = counted(lib, lambda: lib.j2p_planes_to_png(refs, 3, ctypes.byref(spec), None, 0, ctypes.byref(size)))
        probed = s.output_scratch_bytes()
        # (the scratch, and an oriented solver's upright planes)
        assert rc == J2P_ESPACE and took == (1 if orientation == 1 else 2) and probed > 0
        buf = np.zeros(size.value + 8, np.uint8)
        rc, took = counted(lib, lambda: lib.j2p_planes_to_png(refs, 3, ctypes.byref(spec), buf.ctypes.data, buf.size, ctypes.byref(size)))
        assert rc == 0, lib.j2p_last_error().decode()
        assert took == 1 and s.output_scratch_bytes() > probed, "the scratch did not move between the two requests"
        moved = buf[:size.value].tobytes()
        room = s.output_scratch_bytes()
        buf[:] = 0
        rc, took = counted(lib, lambda: lib.j2p_planes_to_png(refs, 3, ctypes.byref(spec), buf.ctypes.data, buf.size, ctypes.byref(size)))
        assert rc == 0 and took == 0 and s.output_scratch_bytes() == room
        assert buf[:size.value].tobytes() == moved, "the file of the call whose block moved is not the file of a call whose block stayed"
        samples = solver_bytes(lib, j, [s], 3, uw, uh, 16)
    assert struct.unpack(">II", moved[16:24]) == (uw, uh)
    want, report = pc.encode(samples, uw, uh, bits=16, channels=3, filter=0, idat_bytes=16)
    assert rg.takes(rg.png_requests(uw, uh, 3, 16, len(report["zlib"]), idat_bytes=16), rg.SCRATCH_STEP) == 2
    assert moved == want


@pytest.mark.gpu
def test_solver_scratch_moves_under_the_jpeg_coder(lib):
    """j2p_planes_to_jpeg in a solver's scratch, the second request: a 304x256 4:4:4 solve from noisy quality-10 coefficients,
    written at quality 100, is a stream of several hundred KB for a guess of a quarter of the coefficients (114 KB), rounded up to
    768 KB with the fixed parts.  The file is the restatement of the solver's own coefficients (0.3 s of Python at this size).
    The third request does not move the scratch here, and hardly can at a size a test may have: the second is rounded up to a
    multiple of 256 KiB (1.25 MiB for 1.09 MiB asked), and the FF bytes would have to exceed their guess — a sixteenth of the stream
    and 256 — by the rest of that step (here by about 160 KB; they exceed it by about 25 KB).  test_entropy_encode_whose_stream_outgrows_both_guesses
    covers that re-queue through the pool, whose blocks are not rounded."""
    import jpeg2png_amd as j
    from test_entropy_gpu import restated_from
    lib.j2p_pool_trim()
    w, h = 304, 256
    tables = j.quality_tables(100, 3)
    with j.Solver(rg.noisy_planes(w, h), 0.3, [0.001] * 3, 1) as s:
        s.run(1)
        refs, size = plane_refs(j, s), ctypes.c_size_t(0)
        spec, _held = j._c_jpeg(w, h, 3, 100, None, (1, 1))
        buf = np.zeros(4 << 20, np.uint8)
        rc, took = counted(lib, lambda: lib.j2p_planes_to_jpeg(refs, 3, ctypes.byref(spec), buf.ctypes.data, buf.size, ctypes.byref(size)))
        assert rc == 0, lib.j2p_last_error().decode()
        assert took == 2, "the scratch did not move at the second request"
        moved = buf[:size.value].tobytes()
        room = s.output_scratch_bytes()
        buf[:] = 0
        rc, took = counted(lib, lambda: lib.j2p_planes_to_jpeg(refs, 3, ctypes.byref(spec), buf.ctypes.data, buf.size, ctypes.byref(size)))
        assert rc == 0 and took == 0 and s.output_scratch_bytes() == room and buf[:size.value].tobytes() == moved
        want = restated_from([(s, c) for c in range(3)], w, h, tables, (1, 1))
    case = {"width": w, "height": h, "sub": (1, 1), "coefficients": [None] * 3}
    assert rg.takes(rg.jpeg_requests(case, *rg.scan_sizes(want)), rg.SCRATCH_STEP) == 2
    assert moved == want
