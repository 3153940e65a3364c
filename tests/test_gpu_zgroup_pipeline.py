"""-m gpu: the pipelined plane groups (OFFT_HIP_OPT_ZGROUP_PIPELINE) on the device.

fft_pair_yx_k carries the x pass of one group of z-planes and the y pass of the next in one grid; both bodies are the
ones the alternating launches run, so the result has to be the same BITS with the option on and off -- at every group
count (one group: prologue and epilogue only; two; four and more; a short last group), in synchronous mode, in
asynchronous mode and on a caller-owned stream.  A plan outside the scope must not take the route at all."""
import numpy as np
import pytest
import torch

import oracle_lib as O
from gpu_util import make_input
from offt_amd import api

pytestmark = pytest.mark.gpu


def transform(shape, mib, pipeline, mode="sync", field=None, direction=-1, precision=api.F64, repeat=1, **params):
    """(raw device array after the execute(s), pipelined launches, paired bits) of one plan"""
    L = api.lib()
    po = api.offt_3d_init(*shape, custom_params=api.make_params(**params), precision=precision)
    stream = None
    try:
        assert L.offt_hip_set_option(po, api.OPT_ZGROUP_MIB, mib) == 0
        assert L.offt_hip_set_option(po, api.OPT_ZGROUP_PIPELINE, pipeline) == 0
        L.offt_hip_set_output_scale(po, 2.0 ** -7)
        dev, _ = make_input(po, O.hash_field(*shape) if field is None else field, precision)
        if mode == "stream":
            stream = torch.cuda.Stream()
            stream.wait_stream(torch.cuda.current_stream())
            L.offt_hip_set_stream(po, stream.cuda_stream)
        L.offt_hip_set_async(po, 0 if mode == "sync" else 1)
        for _ in range(repeat):
            api.offt_3d_execute_dir(po, dev.data_ptr(), dev.data_ptr(), direction)
        assert L.offt_hip_wait(po) == 0
        if stream is not None:
            stream.synchronize()
        return dev.cpu().numpy().copy(), L.offt_hip_last_pipelined_launches(po), L.offt_hip_last_passes_paired(po)
    finally:
        api.offt_3d_fin(po)


# planes of 64 KiB, 64 of them: MiB per group -> groups.  4: one group; 2: two; 1: four; 3: 48 + 16 planes (a short last group)
# 32 x 128 x 64 (unequal x and y): no paired kernel -- a short body next to a longer one would lose occupancy -- so the launches
# alternate whatever the option says, and the bits are the same for that reason
SMALL = [((64, 64, 64), 4, 1), ((64, 64, 64), 2, 2), ((64, 64, 64), 1, 4), ((64, 64, 64), 3, 2),
         ((32, 128, 64), 4, 1), ((32, 128, 64), 2, 2), ((32, 128, 64), 1, 4), ((32, 128, 64), 3, 2),
         # the 128-, 256- and 512-point entries (planes of 256 KiB, 1 MiB, 4 MiB), each with a short last group
         ((128, 128, 10), 1, 3), ((256, 256, 7), 2, 4), ((512, 512, 5), 8, 3)]
_ref = {}


def reference(shape, mib):
    """the alternating launches of the same group size, computed once"""
    if (shape, mib) not in _ref:
        got, n, paired = transform(shape, mib, 0)
        assert n == 0 and paired == 6
        _ref[shape, mib] = got
    return _ref[shape, mib]


@pytest.mark.parametrize("mode", ["sync", "async", "stream"])
@pytest.mark.parametrize("shape,mib,groups", SMALL)
def test_pipeline_on_is_bit_identical_to_off(built, shape, mib, groups, mode):
    want = reference(shape, mib)
    got, n, paired = transform(shape, mib, 1, mode, repeat=1)
    assert n == (groups - 1 if shape[0] == shape[1] else 0) and paired == 6
    assert np.array_equal(got, want)


@pytest.mark.parametrize("mode", ["sync", "async", "stream"])
def test_flagship_kernel_instance(built, mode):
    """1024 x 1024 x 8 (128 MiB): the 1024-point instance on both roles; 3-plane groups (384 panels per role in a middle launch:
    the first 256 in the XCD-aware order, a tail of 128 behind them) with a short last one"""
    shape = (1024, 1024, 8)
    rng = np.random.default_rng(5)
    if "field" not in _ref:
        _ref["field"] = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))
    want = _ref.get("flag")
    if want is None:
        want, n, _ = transform(shape, 48, 0, field=_ref["field"])
        assert n == 0
        _ref["flag"] = want
    got, n, paired = transform(shape, 48, 1, mode, field=_ref["field"])
    assert n == 2 and paired == 6
    assert np.array_equal(got, want)


def test_second_execute_on_the_same_plan(built):
    want, _, _ = transform((64, 64, 64), 1, 0, repeat=2)
    got, n, _ = transform((64, 64, 64), 1, 1, "async", repeat=2)
    assert n == 3 and np.array_equal(got, want)


@pytest.mark.parametrize("kw", [dict(direction=+1), dict(precision=api.F32), dict(S=1), dict(shape=(96, 64, 64))],
                         ids=["inverse", "f32", "xyz", "mixed-radix"])
def test_out_of_scope_plans_do_not_take_the_route(built, kw):
    kw = dict(kw)
    shape = kw.pop("shape", (64, 64, 64))
    off, n_off, paired_off = transform(shape, 1, 0, **kw)
    on, n_on, paired_on = transform(shape, 1, 1, **kw)
    assert n_on == 0 and n_off == 0 and paired_on == paired_off
    assert np.array_equal(on, off)


def test_on_by_default(built):
    """a plan nobody configured runs the pipelined launches: 64^3 with the library's 256 MiB groups is one group (no middle
    launch), with 1 MiB groups it is four"""
    L = api.lib()
    po = api.offt_3d_init(64, 64, 64)
    try:
        assert L.offt_hip_get_option(po, api.OPT_ZGROUP_PIPELINE) == 1
        L.offt_hip_set_option(po, api.OPT_ZGROUP_MIB, 1)
        dev, _ = make_input(po, O.hash_field(64, 64, 64))
        api.offt_3d_execute(po, dev.data_ptr(), dev.data_ptr())
        assert L.offt_hip_last_pipelined_launches(po) == 3
    finally:
        api.offt_3d_fin(po)
