"""The arithmetic tests/test_regrow_gpu.py stands on, checked without a GPU: by the restatements' own sizes the directed inputs of
tests/regrow_cases.py make each later request of a coder for its block larger than the one before (the block moves), and the
controls do not."""
import entropy_cases as ec
import huffman_cases as hc
import png_cases as pc
import regrow_cases as rg


def test_the_heavy_blocks_outgrow_both_guesses():
    case = rg.heavy_case()
    file, stuffed, _short = ec.encode_report(case["coefficients"], 32, 32, case["quant"])
    nbytes, ffs = rg.scan_sizes(file)
    assert (nbytes, ffs) == (3280, 1744) and ffs == stuffed
    assert ffs > nbytes // 16 + 256 == 461                      # the third request's guess
    first, second, third = rg.jpeg_requests(case, nbytes, ffs)
    assert first < second < third and rg.takes([first, second, third]) == 3
    assert first - rg.carve(16 * 128, 16 * 4, 16 * 8, 2 * 8) == 16 * 128 // 4 == 512       # the first request's guess


def test_the_optimised_file_of_the_heavy_blocks_outgrows_both_guesses_too():
    case = rg.heavy_case()
    file, report = hc.encode_report(case["coefficients"], 32, 32, case["quant"])
    nbytes, ffs = rg.scan_sizes(file)
    assert ffs == report["stuffed"] and nbytes == -(-report["bits"] // 8)
    assert (nbytes, ffs) == (1388, 380) and ffs > nbytes // 16 + 256 == 342
    requests = rg.jpeg_requests(case, nbytes, ffs, counting=True)
    assert requests[0] < requests[1] < requests[2] and rg.takes(requests) == 3


def test_a_sparse_image_of_the_same_size_outgrows_the_first_guess_only():
    case = rg.sparse_case()
    nbytes, ffs = rg.scan_sizes(ec.encode(case["coefficients"], 32, 32, case["quant"]))
    first, second, third = rg.jpeg_requests(case, nbytes, ffs)
    # (16 blocks of coefficients are small next to the staging's parts of 256 bytes: the first guess is too small even here)
    assert ffs <= nbytes // 16 + 256 and first < second and third <= second and rg.takes([first, second, third]) == 2


def test_the_progressive_file_of_the_heavy_blocks_outgrows_both_guesses_and_the_sparse_one_the_first():
    """the layout above j2p_encode_progressive: six scans of 16 items each; 30464 bytes are known from the spec, 24624 of them the
    counts"""
    import progressive_cases as prc
    case = rg.heavy_case()
    _file, report = prc.encode_case(case)
    nbytes, ffs = sum(-(-r["bits"] // 8) for r in report), sum(r["stuffed"] for r in report)
    assert (nbytes, ffs) == (1392, 376) and ffs > nbytes // 16 + 256 == 343
    requests = rg.progressive_requests(case, report)
    assert requests == [30976, 34503, 34536] and rg.takes(requests) == 3
    assert requests[0] - 16 * 128 // 4 == rg.carve(16 * 128, 96 * 4, 96 * 8, 2 * 8, *[16] * 4, *[64] * 4, 6 * 513 * 8) == 30464
    case = rg.sparse_case()
    _file, report = prc.encode_case(case)
    assert (sum(-(-r["bits"] // 8) for r in report), sum(r["stuffed"] for r in report)) == (48, 0)
    requests = rg.progressive_requests(case, report)
    # (the third request is smaller than the second: its guess for the FF bytes was 259)
    assert requests == [30976, 31795, 31536] and rg.takes(requests) == 2


def test_noise_outgrows_the_png_coders_guess_and_zeros_do_not():
    image = rg.noise_image()
    _file, report = pc.encode(image.reshape(48, -1), 48, 48, idat_bytes=16)
    assert len(report["filtered"]) == 6960
    first, second = rg.png_requests(48, 48, 3, 8, len(report["zlib"]), idat_bytes=16)
    assert second > first and rg.takes([first, second]) == 2
    _file, report = pc.encode(image.reshape(48, -1) * 0, 48, 48, idat_bytes=16)
    first, second = rg.png_requests(48, 48, 3, 8, len(report["zlib"]), idat_bytes=16)
    assert second < first and rg.takes([first, second]) == 1


def test_a_scratch_that_grows_in_steps_needs_more_than_a_step():
    step = rg.SCRATCH_STEP
    assert rg.takes([step - 5, step], step) == 1 and rg.takes([step - 5, step + 1], step) == 2
    assert rg.takes([10, 5, 11]) == 2 and rg.takes([10, 11, 12]) == 3
