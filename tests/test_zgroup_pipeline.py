"""CPU tier: the host path of the pipelined plane groups (OFFT_HIP_OPT_ZGROUP_PIPELINE, execute_single).

The forward z-y-x transform of one rank runs its y and x passes over groups of z-planes.  With the pipeline the x launch of
group g-1 and the y launch of group g are ONE backend call (offt_backend::pass_pair):

    y(0) | {x(0), y(1)} | ... | {x(G-2), y(G-1)} | x(G-1)

tests/cpu_backend_pipeline.c runs such a call as the two passes one after the other and logs every pass and pass_pair, so
the schedule is read off the log and the values are compared, bit for bit, with the alternating launches."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cpu_world
import oracle_lib as O
from offt_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Rec(C.Structure):  # cpu_backend_pipeline.c: prec
    _fields_ = [(n, C.c_int) for n in ("kind", "n", "nb1", "out_keep", "out_contig", "n2", "nb1_2", "out_keep2")] + \
               [("out_off", C.c_longlong), ("out_off2", C.c_longlong)]


@pytest.fixture(scope="module")
def world(built):
    subprocess.check_call(["make", "-s", "-C", ROOT, "tests/libcpubackend.so", "tests/libcpubackend_pipeline.so"])
    cpu_world.install(0, 1)  # (the library routing; the table is replaced below)
    CB = C.CDLL(os.path.join(ROOT, "tests", "libcpubackend_pipeline.so"))
    CB.cpu_backend_pipeline_table.restype = C.c_void_p
    CB.cpu_backend_pipeline_len.restype = C.c_long
    CB.cpu_backend_pipeline_reset.argtypes = [C.c_void_p]
    CB.cpu_backend_pipeline_copy_log.argtypes = [C.c_void_p]
    assert CB.cpu_backend_pipeline_rec_bytes() == C.sizeof(Rec)
    L = api.lib()
    L.offt_hip_test_set_backend(CB.cpu_backend_pipeline_table(), 0, 1)
    try:
        yield CB, L
    finally:
        cpu_world.uninstall()


def run(world, shape, planes, pipeline, direction=-1, precision=api.F64, is_equalxy=0, asyn=0, repeat=1, **params):
    """one plan, `repeat` executes in place on the hash field: (result, log of the LAST execute, pipelined launches, paired bits)"""
    CB, L = world
    po = api.offt_3d_init(*shape, custom_params=api.make_params(**params), is_equalxy=is_equalxy, precision=precision)
    try:
        assert L.offt_hip_set_option(po, api.OPT_ZGROUP_PLANES, planes) == 0
        assert L.offt_hip_set_option(po, api.OPT_ZGROUP_PIPELINE, pipeline) == 0
        assert L.offt_hip_get_option(po, api.OPT_ZGROUP_PIPELINE) == pipeline
        ct = np.complex128 if precision == api.F64 else np.complex64
        buf = np.zeros(api.local_elems(po), dtype=ct)
        c = api.comm_dict(po)
        s0, s1, s2 = c["istride"]
        idx = (np.arange(shape[0])[:, None, None] * s0 + np.arange(shape[1])[None, :, None] * s1 + np.arange(shape[2])[None, None, :] * s2).ravel()
        buf[idx] = O.hash_field(*shape).astype(ct).ravel()
        L.offt_hip_set_output_scale(po, 0.25)
        L.offt_hip_set_async(po, asyn)
        for _ in range(repeat):
            CB.cpu_backend_pipeline_reset(buf.ctypes.data)
            api.offt_3d_execute_dir(po, buf.ctypes.data, buf.ctypes.data, direction)
            assert L.offt_hip_wait(po) == 0
        log = (Rec * CB.cpu_backend_pipeline_len())()
        CB.cpu_backend_pipeline_copy_log(log)
        return buf, list(log), L.offt_hip_last_pipelined_launches(po), L.offt_hip_last_passes_paired(po)
    finally:
        api.offt_3d_fin(po)


# (shape, planes per group): G = 1 (prologue and epilogue only), 2, >= 4, and a last group smaller than the others
CASES = [((16, 16, 16), 16), ((16, 16, 16), 8), ((16, 16, 16), 4), ((16, 16, 16), 1), ((16, 16, 16), 5), ((16, 16, 16), 15),
         ((32, 16, 24), 24), ((32, 16, 24), 12), ((32, 16, 24), 5), ((16, 32, 32), 7), ((32, 32, 32), 3)]


@pytest.mark.parametrize("shape,planes", CASES)
def test_schedule_and_bits(world, shape, planes):
    nx, ny, nz = shape
    groups = [min(planes, nz - z0) for z0 in range(0, nz, planes)]
    off, log_off, n_off, paired_off = run(world, shape, planes, 0)
    on, log_on, n_on, paired_on = run(world, shape, planes, 1)
    assert np.array_equal(on, off)
    assert n_off == 0 and n_on == len(groups) - 1
    assert paired_on == paired_off == 6  # the y and x timer slots, measured as a pair: as before
    # off: z, then y(g), x(g) for every group
    assert [(r.kind, r.n, r.nb1) for r in log_off] == [(0, nz, nx)] + [e for g in groups for e in ((0, ny, g), (0, nx, g))]
    # on: z | y(0) | {x(g-1), y(g)} ... | x(G-1)
    want = [(0, nz, nx, 0, 0), (0, ny, groups[0], 0, 0)] + [(1, ny, groups[g], nx, groups[g - 1]) for g in range(1, len(groups))] + \
           [(0, nx, groups[-1], 0, 0)]
    assert [(r.kind, r.n, r.nb1, r.n2, r.nb1_2) for r in log_on] == want
    plane_bytes = nx * ny * 16
    z0 = 0
    for g, r in enumerate(log_on[1:-1]):  # every y launch keeps its stores and writes its own group; x takes the group before
        assert r.out_keep == 1 and r.out_contig == 0 and r.out_off == z0 * plane_bytes
        if r.kind == 1:
            assert r.out_keep2 == 0 and r.out_off2 == (z0 - planes) * plane_bytes
        z0 += groups[g]
    assert log_on[-1].out_off == (nz - groups[-1]) * plane_bytes and log_on[-1].out_keep == 0


def test_async_and_repeated_executes(world):
    """asynchronous mode (no timing events) and a second execute on the same plan: the same schedule, the same bits"""
    ref, log_ref, _, _ = run(world, (16, 16, 16), 5, 0, repeat=2)
    for asyn in (0, 1):
        got, log, n, paired = run(world, (16, 16, 16), 5, 1, asyn=asyn, repeat=2)
        assert np.array_equal(got, ref)
        assert n == 3 and paired == 6
        assert [r.kind for r in log] == [0, 0, 1, 1, 1, 0]


@pytest.mark.parametrize("kw", [dict(direction=+1), dict(precision=api.F32), dict(S=1), dict(is_equalxy=1)],
                         ids=["inverse", "f32", "xyz", "yzx"])
def test_out_of_scope_plans_launch_what_they_launched(world, kw):
    """the inverse, single precision and the other layouts keep their launches, pass for pass, with the option set"""
    shape = (16, 16, 16)
    off, log_off, n_off, paired_off = run(world, shape, 4, 0, **kw)
    on, log_on, n_on, paired_on = run(world, shape, 4, 1, **kw)
    assert n_on == 0 and n_off == 0 and paired_on == paired_off
    assert np.array_equal(on, off)
    key = lambda r: (r.kind, r.n, r.nb1, r.out_keep, r.out_contig)  # (not the offsets: some stores go to the plan's scratch)
    assert [key(r) for r in log_on] == [key(r) for r in log_off]
    assert all(r.kind == 0 for r in log_on)


def test_second_stream_is_never_pipelined(world):
    CB, L = world
    po = api.offt_3d_init(16, 16, 16)
    try:
        L.offt_hip_set_option(po, api.OPT_ZGROUP_PLANES, 4)
        L.offt_hip_set_option(po, api.OPT_ZGROUP_PIPELINE, 1)
        L.offt_hip_set_option(po, 1, 2)  # OFFT_HIP_OPT_ZGROUP_STREAMS
        buf = np.zeros(api.local_elems(po), dtype=np.complex128)
        CB.cpu_backend_pipeline_reset(buf.ctypes.data)
        api.offt_3d_execute(po, buf.ctypes.data, buf.ctypes.data)
        assert L.offt_hip_last_pipelined_launches(po) == 0 and L.offt_hip_last_passes_paired(po) == 6
    finally:
        api.offt_3d_fin(po)


def test_default(world, monkeypatch):
    """the option is on by default; the environment variable is read at plan time.  A table handed to
    offt_hip_test_set_backend may be older than pass_pair, so its entry is used only once the option has been SET"""
    CB, L = world
    po = api.offt_3d_init(16, 16, 16)
    try:
        assert L.offt_hip_get_option(po, api.OPT_ZGROUP_PIPELINE) == 1 and L.offt_hip_get_option(po, api.OPT_ZGROUP_PLANES) == 0
        L.offt_hip_set_option(po, api.OPT_ZGROUP_PLANES, 4)
        buf = np.zeros(api.local_elems(po), dtype=np.complex128)
        CB.cpu_backend_pipeline_reset(buf.ctypes.data)
        api.offt_3d_execute(po, buf.ctypes.data, buf.ctypes.data)
        assert L.offt_hip_last_pipelined_launches(po) == 0 and CB.cpu_backend_pipeline_len() == 9
        L.offt_hip_set_option(po, api.OPT_ZGROUP_PIPELINE, 1)
        api.offt_3d_execute(po, buf.ctypes.data, buf.ctypes.data)
        assert L.offt_hip_last_pipelined_launches(po) == 3
    finally:
        api.offt_3d_fin(po)
    monkeypatch.setenv("OFFT_ZGROUP_PIPELINE", "0")
    monkeypatch.setenv("OFFT_ZGROUP_PLANES", "3")
    po = api.offt_3d_init(16, 16, 16)
    assert L.offt_hip_get_option(po, api.OPT_ZGROUP_PIPELINE) == 0 and L.offt_hip_get_option(po, api.OPT_ZGROUP_PLANES) == 3
    api.offt_3d_fin(po)


def test_planes_turn_nothing_on(world):
    """OFFT_HIP_OPT_ZGROUP_PLANES sizes groups that exist: with OFFT_HIP_OPT_ZGROUP_MIB = 0 the transform is three plain launches"""
    CB, L = world
    po = api.offt_3d_init(16, 16, 16)
    try:
        L.offt_hip_set_option(po, api.OPT_ZGROUP_MIB, 0)
        L.offt_hip_set_option(po, api.OPT_ZGROUP_PLANES, 4)
        L.offt_hip_set_option(po, api.OPT_ZGROUP_PIPELINE, 1)
        buf = np.zeros(api.local_elems(po), dtype=np.complex128)
        CB.cpu_backend_pipeline_reset(buf.ctypes.data)
        api.offt_3d_execute(po, buf.ctypes.data, buf.ctypes.data)
        assert CB.cpu_backend_pipeline_len() == 3 and L.offt_hip_last_pipelined_launches(po) == 0 and L.offt_hip_last_passes_paired(po) == 0
    finally:
        api.offt_3d_fin(po)
