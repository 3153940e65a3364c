"""-m gpu: the two-chain plane groups (OFFT_HIP_OPT_ZGROUP_CHAINS = 2) on the device.

Both chains launch the kernels the one chain launches, on the same planes, so the result has to be the same BITS as with one
chain and as with plain alternating launches (OFFT_HIP_OPT_ZGROUP_PIPELINE = 0) -- with an even and an odd number of groups,
a short last group in either chain, in synchronous mode, on a caller-owned stream and in asynchronous mode with several
executes behind one another and a single wait (the second stream's work of one execute must be over before the z pass of
the next overwrites the scratch volume, and before the caller reads)."""
import numpy as np
import pytest
import torch

import oracle_lib as O
from gpu_util import make_input
from offt_amd import api

pytestmark = pytest.mark.gpu


def transform(shape, planes, pipeline, chains, mode="sync", repeat=1):
    """(raw device array after the execute(s), paired launches, chains) of one plan"""
    L = api.lib()
    po = api.offt_3d_init(*shape)
    stream = None
    try:
        assert L.offt_hip_set_option(po, api.OPT_ZGROUP_PLANES, planes) == 0
        assert L.offt_hip_set_option(po, api.OPT_ZGROUP_PIPELINE, pipeline) == 0
        assert L.offt_hip_set_option(po, api.OPT_ZGROUP_CHAINS, chains) == 0
        L.offt_hip_set_output_scale(po, 2.0 ** -7)
        dev, _ = make_input(po, O.hash_field(*shape))
        if mode == "stream":
            stream = torch.cuda.Stream()
            stream.wait_stream(torch.cuda.current_stream())
            L.offt_hip_set_stream(po, stream.cuda_stream)
        L.offt_hip_set_async(po, 0 if mode == "sync" else 1)
        for _ in range(repeat):
            api.offt_3d_execute(po, dev.data_ptr(), dev.data_ptr())
        assert L.offt_hip_wait(po) == 0
        if stream is not None:
            stream.synchronize()
        return dev.cpu().numpy().copy(), L.offt_hip_last_pipelined_launches(po), L.offt_hip_last_pipelined_chains(po)
    finally:
        api.offt_3d_fin(po)


# (shape, planes per group, groups): 8 groups; 13 groups, the last of 4 planes in the even chain; 16; 26 groups, the last of
# 3 planes in the odd chain; the 256-point kernels with 8 groups
CASES = [((64, 64, 64), 8, 8), ((64, 64, 64), 5, 13), ((128, 128, 128), 8, 16), ((128, 128, 128), 5, 26), ((256, 256, 64), 8, 8)]
_ref = {}


def references(shape, planes, repeat=1):
    """one chain, and plain alternating launches, of the same group size: computed once"""
    key = (shape, planes, repeat)
    if key not in _ref:
        one, n1, c1 = transform(shape, planes, 1, 1, repeat=repeat)
        off, n0, c0 = transform(shape, planes, 0, 1, repeat=repeat)
        groups = -(-shape[2] // planes)
        assert (n1, c1, n0, c0) == (groups - 1, 1, 0, 0)
        _ref[key] = (one, off)
    return _ref[key]


@pytest.mark.parametrize("shape,planes,groups", CASES)
def test_two_chains_are_bit_identical(built, shape, planes, groups):
    one, off = references(shape, planes)
    got, n, chains = transform(shape, planes, 1, 2)
    assert chains == 2 and n == groups - 2  # y | pairs | x per chain: (Ge - 1) + (Go - 1) paired launches
    assert np.array_equal(got, one) and np.array_equal(got, off)


def test_on_a_caller_owned_stream(built):
    one, off = references((64, 64, 64), 5)
    got, n, chains = transform((64, 64, 64), 5, 1, 2, mode="stream")
    assert chains == 2 and n == 11
    assert np.array_equal(got, one) and np.array_equal(got, off)


def test_async_three_executes_one_wait(built):
    one, off = references((128, 128, 128), 5, repeat=3)
    got, n, chains = transform((128, 128, 128), 5, 1, 2, mode="async", repeat=3)
    assert chains == 2 and n == 24
    assert np.array_equal(got, one) and np.array_equal(got, off)


def test_fewer_than_four_groups_is_one_chain(built):
    one, off = references((64, 64, 64), 24)
    got, n, chains = transform((64, 64, 64), 24, 1, 2)
    assert chains == 1 and n == 2 and np.array_equal(got, one)
