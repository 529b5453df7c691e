"""Multi-output tensor resampling without a device: the work map of j2p_planes_to_tensors_resampled's sampling launches, read
through the hooks that compute it with the launch's own code (j2p_debug_outputs_plan, j2p_debug_outputs_workgroups), and what
the call, the batch engine and the bindings refuse before they need a GPU."""
import ctypes

import numpy as np
import pytest

import filter_cases as fc
import outputs_cases as oc

J2P_EINVAL = -1


def single_call_tile(ow, oh):
    """filter_tile of j2p_output.hip restated: 256 columns x 4 rows per wavefront; while that gives fewer than 2048 wavefronts
    the columns are halved down to 64, then the rows down to 1, and last the tile is 32 columns"""
    tile, rows = 256, 4

    def few():
        return -(-ow // tile) * -(-oh // rows) < 2048
    while tile > 64 and few():
        tile //= 2
    while rows > 1 and few():
        rows //= 2
    if few():
        tile = 32
    lanes = min(tile, 64)
    return lanes, tile // lanes, rows


def all_sets():
    sets = {name: (fc.IMAGES[image], outs) for name, (image, outs) in oc.SETS.items()}
    sets["extreme"] = (oc.EXTREME[:2], oc.EXTREME[2])
    # what the measurements launch: ten crops of a 12-Mpixel image, and a pyramid of it
    big = (4096, 3072)
    sets["multi_crop"] = (big, [((8 * i, 8 * i, 2048, 1536), 224, 224, "triangle", "f16", "chw") for i in range(2)] +
                          [((100 * i, 60 * i, 614, 460), 96, 96, "cubic", "f16", "chw") for i in range(8)])
    sets["pyramid"] = (big, [(None, 2048 >> k, 1536 >> k, "triangle", "f16", "chw") for k in range(4)])
    return sets


@pytest.mark.parametrize("name", sorted(all_sets()))
def test_every_workgroup_of_every_output_occurs_exactly_once(lib, name):
    import jpeg2png_amd as j
    size, outs = all_sets()[name]
    specs = [oc.spec(size, o) for o in outs]
    dtypes = [oc.DTYPES[o[4]] for o in outs]
    plan = j.outputs_plan(*size, specs, dtypes)
    # the grouping: one launch per dtype present, ascending, every output in the launch of its dtype
    assert [d for d, _ in plan["launches"]] == sorted(set(dtypes))
    assert [plan["launches"][k][0] for k in plan["launch_of"]] == dtypes
    for i, (o, tile, grid) in enumerate(zip(outs, plan["tiles"], plan["grids"])):
        assert tile == single_call_tile(o[1], o[2]), (name, i)          # (the tile is the output's own, as in the single call)
        assert grid == oc.own_grid(tile, o[1], o[2]), (name, i)
    for k, (dtype, workgroups) in enumerate(plan["launches"]):
        members = [i for i, d in enumerate(dtypes) if d == dtype]
        # exactly the sum of the outputs' own grids: no workgroup without work
        assert workgroups == sum(plan["grids"][i][0] * plan["grids"][i][1] for i in members)
        got = j.outputs_workgroups(*size, specs, dtypes, k).astype(np.int64)
        assert got.shape == (workgroups, 3)
        want = np.concatenate([np.array([(i, x, y) for y in range(plan["grids"][i][1]) for x in range(plan["grids"][i][0])], np.int64)
                               for i in members])
        # every (output, tile column, row group) of every member's own grid exactly once — in the order of the outputs' own
        # launches, tile column fastest — and hence none beyond a grid
        assert np.array_equal(got, want), name
        # a window of the launch is the same map; one index beyond the grid is refused
        if workgroups > 2:
            assert np.array_equal(j.outputs_workgroups(*size, specs, dtypes, k, first=1, count=workgroups - 2), want[1:-1])
        with pytest.raises(j.J2PError):
            j.outputs_workgroups(*size, specs, dtypes, k, first=workgroups, count=1)
    with pytest.raises(j.J2PError):
        j.outputs_workgroups(*size, specs, dtypes, len(plan["launches"]), first=0, count=0)


@pytest.mark.parametrize("case", fc.CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}x{c[3]}")
def test_one_output_takes_the_tile_of_the_single_call(lib, case):
    import jpeg2png_amd as j
    image, box, ow, oh = case
    size = fc.IMAGES[image]
    for name in sorted(fc.FILTERS):
        plan = j.outputs_plan(*size, [oc.spec(size, (box, ow, oh, name))], [3])
        assert plan["tiles"] == [single_call_tile(ow, oh)] and plan["launches"] == [(3, plan["grids"][0][0] * plan["grids"][0][1])]
        assert plan["grids"] == [oc.own_grid(plan["tiles"][0], ow, oh)]


def test_the_restated_tile_rule_reaches_every_tile(lib):
    """the restatement is not vacuous: the cases above meet tiles of 32, 64 and 256 columns and 1, 2 and 4 rows"""
    tiles = {single_call_tile(ow, oh) for _, _, ow, oh in fc.CASES}
    assert {lanes * slots for lanes, slots, _ in tiles} >= {32, 64, 256} and {rows for _, _, rows in tiles} == {1, 2, 4}


def test_refusals_that_need_no_device(lib):
    import jpeg2png_amd as j
    ok = (0, 0, 45, 37, 7, 5, fc.TRIANGLE)
    assert j.outputs_plan(45, 37, [ok] * 16, [3] * 16)["launches"] == [(3, 16 * 2)]
    refused = {
        "17 outputs": ([ok] * 17, [3] * 17),
        "no output": ([], []),
        "a box that leaves the image": ([ok, (40, 0, 6, 5, 3, 3, fc.TRIANGLE)], [3, 3]),
        "filter 0 (the area form)": ([ok, (0, 0, 45, 37, 7, 5, 0)], [3, 3]),
        "filter 3": ([(0, 0, 45, 37, 7, 5, 3), ok], [3, 3]),
        "an empty box": ([ok, (0, 0, 0, 5, 1, 1, fc.CUBIC)], [3, 3]),
        "out_w 65537": ([ok, (0, 0, 45, 37, 65537, 5, fc.CUBIC)], [3, 3]),
        "dtype 4": ([ok, ok], [3, 4]),
    }
    for what, (specs, dtypes) in refused.items():
        with pytest.raises(j.J2PError):
            j.outputs_plan(45, 37, specs, dtypes)
        with pytest.raises(j.J2PError):
            j.outputs_workgroups(45, 37, specs, dtypes, 0, first=0, count=0)
    # the entry points themselves: what they refuse before they look at a solver or a device
    outs = (j._COutput * 17)()
    refs = (j._CPlaneRef * 3)()
    assert lib.j2p_planes_to_tensors_resampled(refs, 3, 45, 37, 0, outs) == J2P_EINVAL
    assert lib.j2p_planes_to_tensors_resampled(refs, 3, 45, 37, 17, outs) == J2P_EINVAL
    assert lib.j2p_planes_to_tensors_resampled(refs, 3, 45, 37, 2, None) == J2P_EINVAL
    assert lib.j2p_planes_to_tensors_resampled(None, 3, 45, 37, 2, outs) == J2P_EINVAL
    for i in range(2):
        outs[i].r = j._CResample(*ok)
    outs[1].r.filter = 0
    assert lib.j2p_planes_to_tensors_resampled(refs, 3, 45, 37, 2, outs) == J2P_EINVAL
    assert b"output 1" in lib.j2p_last_error()
    assert lib.j2p_batch_submit_outputs(None, None, 2, outs, None) == J2P_EINVAL


def test_the_bindings_refuse_before_they_need_torch_or_a_batch(lib):
    import jpeg2png_amd as j
    good = {"out_width": 7, "out_height": 5, "filter": "triangle"}
    b, s = object.__new__(j.Batch), object.__new__(j.Solver)
    submit = lambda **kw: j.Batch.submit(b, [None] * 3, 0.3, [0.001] * 3, 2, width=45, height=37, **kw)     # noqa: E731
    for kw in ({"tensor": object()}, {"bits": 8}, {"quant_tables": [None] * 3}, {"tile": True}, {"filter": "cubic"}, {"out_width": 8},
               {"scale": 2.0}, {"layout": "hwc"}):
        with pytest.raises(j.J2PError, match="outputs="):
            submit(outputs=[dict(good, tensor=object())], **kw)
    for outputs in ([], [dict(good, tensor=object())] * 17, [dict(good)], [dict(good, tensor=object(), out=object())],
                    [{"out_width": 7, "tensor": object()}], [dict(good, filter="area", tensor=object())],
                    [dict(good, box=(40, 0, 6, 5), tensor=object())], [dict(good, tensor=object()), 5], 7):
        with pytest.raises(j.J2PError):
            submit(outputs=outputs)
    for outputs in ([], [good] * 17, [dict(good, tensor=object())], [{"out_width": 7}], [dict(good, filter="area")], [dict(good, filter=None)],
                    [dict(good, box=(40, 0, 6, 5))], [dict(good, out_width=65537)], [good, None]):
        with pytest.raises(j.J2PError):
            j.Solver.to_tensors(s, 45, 37, outputs)


def test_symbols_and_structs(lib):
    import jpeg2png_amd as j
    for name in ("j2p_planes_to_tensors_resampled", "j2p_batch_submit_outputs", "j2p_debug_outputs_plan", "j2p_debug_outputs_workgroups"):
        assert name in j.C_ABI_SYMBOLS and hasattr(lib, name)
    assert ctypes.sizeof(j._COutput) == 96 and j._COutput.t.offset == 32 and j.J2P_MAX_OUTPUTS == oc.MAX_OUTPUTS
    # the job did not grow: the outputs travel next to it
    size, off = j.job_layout()
    assert size == ctypes.sizeof(j._CJob) and off + ctypes.sizeof(j._CTensor) == size
