"""Pseudo-spectral product: offt_hip_execute_product (two inverses, a multiply in physical space, one forward), without a GPU.

  * routing of the fused launch without a device (offt_hipk_prod_has_fused, offt_hip_product_fused, the option);
  * the host's two routes on the CPU backend of tests/cpu_backend_prod.c, read off its launch log: complex and r2c plans, odd
    shapes, every single-rank layout, every aliasing of `out`, squaring, the output scale, the identity B = fftn(1), older
    backend tables, refusals, the life of the second scratch volume, a half box, a gloo world of 2 ranks.

The reference is numpy in complex128 (float64 fields for r2c plans) on the host: N^2 fftn(ifftn(A) ifftn(B)).  Tolerance:
the project's plan-level W.tol (1e-12 f64, 2e-5 f32), rel-L2 against the norm of the reference.  Single precision, checked
with torch.fft in complex64 on the inputs of _prod_world.problem (the chain ifftn, ifftn, multiply, fftn computed in
single precision by the reference alone): 2.2e-7 ... 2.7e-7 rel-L2 at the shapes used here and in test_gpu_product.py, inside
both single-precision bounds (1e-5 descriptor level, 2e-5 plan level), which therefore stand."""
import ctypes as C
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import _conv_world as W
import _half_world as HW
import _prod_world as PW
from offt_amd import api
from test_convolve_multi import Desc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def prod_desc(n, prec, ncols, nb1, pitch=None, plane_pad=0):
    """strided lines: column c of plane b1 at b1 * plane + c, axis index k at k * pitch (the z pass over W[x][z][y])"""
    pitch = pitch or ncols
    d = Desc()
    d.n, d.precision, d.direction, d.ncols, d.nb1, d.nb2 = n, prec, +1, ncols, nb1, 1
    d.in_axis_stride, d.in_col_stride, d.in_b1_stride = pitch, 1, n * pitch + plane_pad
    d.out_axis_stride, d.out_col_stride, d.out_b1_stride = 1, n, n * ncols
    d.in_contig, d.out_contig, d.variant, d.scale = 0, 1, -1, 1.0
    return d


@pytest.fixture(scope="module")
def kl(built):
    L = api.lib()
    L.offt_hipk_prod_has_fused.argtypes = [C.POINTER(Desc)]
    L.offt_hipk_prod_kernel_name.restype = C.c_char_p
    L.offt_hipk_prod_kernel_name.argtypes = [C.POINTER(Desc)]
    return L


# ---- 1. routing without a device --------------------------------------------------------------------------------------------
def test_prod_kernel_routing_without_a_gpu(kl):
    L = kl
    for prec in (api.F64, api.F32):
        for n in (64, 128, 256, 512, 1024):          # (every length has a spill-free instance)
            d = prod_desc(n, prec, 12, 3, pitch=20)
            assert L.offt_hipk_prod_has_fused(C.byref(d)) == 1, (n, prec)
            assert L.offt_hipk_prod_kernel_name(C.byref(d)) == b"fft_prod_panel_k"
        for n in (32, 96, 2048):
            d = prod_desc(n, prec, 12, 3)
            assert L.offt_hipk_prod_has_fused(C.byref(d)) == 0, (n, prec)
            assert L.offt_hipk_prod_kernel_name(C.byref(d)) == b"no fused kernel"
        for field, val in (("in_contig", 1), ("in_split", 64), ("real_input", 2), ("half", 2)):
            d = prod_desc(256, prec, 8, 2)
            setattr(d, field, val)
            assert L.offt_hipk_prod_has_fused(C.byref(d)) == 0, (field, prec)


# ---- CPU tier ---------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def prod_cpu(built):
    import cpu_world
    subprocess.check_call(["make", "-s", "-C", ROOT, "tests/libcpubackend_prod.so"])
    orig = cpu_world._cb_lib
    cpu_world._cb_lib = PW.prod_cb_lib
    CB = cpu_world.install(0, 1, p1=1)
    yield CB
    cpu_world.uninstall()
    cpu_world._cb_lib = orig


def _plan(case, fused_opt):
    po = HW.make_plan(api, case)
    assert api.lib().offt_hip_set_option(po, api.OPT_PROD_FUSED, fused_opt) == 0
    if case.get("half"):
        api.offt_hip_set_half_box(po, True)
    return po


def _run(CB, case, fused_opt, keep=None, scale=None):
    """plan + product on the installed backend: (error, fused route?, launch counts, launch log)"""
    po = _plan(case, fused_opt)
    try:
        n0 = PW.counts(CB)
        CB.cpu_backend_prod_log_reset()
        err = PW.run_product(api, po, case, HW.Host(), keep=keep, scale=scale)
        n1 = PW.counts(CB)
        return err, api.offt_hip_product_fused(po), {k: n1[k] - n0[k] for k in n0}, PW.launches(CB)
    finally:
        api.offt_3d_fin(po)


def _assert_route(case, fused, cnt, log):
    two = case.get("mode", "two") in ("two", "a", "b")
    nz = case["N"][2]
    if fused:
        assert cnt["prod"] == 1 and cnt["pointwise_prod"] == 0, (case, cnt)
        assert [r[7] for r in log if r[0] == 1] == [2 if two else 1], (case, log)
        # no z pass of either direction: every plain pass is an x or a y pass (two per inverse, two of the forward)
        passes = [r for r in log if r[0] == 0]
        assert len(passes) == (4 if two else 2) + 2, (case, passes)
        assert case["N"][0] != nz and case["N"][1] != nz and all(r[1] != nz for r in passes), (case, passes)
        kinds = [(r[0], r[2]) for r in log]
        assert kinds == [(0, 1)] * (4 if two else 2) + [(1, 1)] + [(0, -1)] * 2, (case, kinds)
    else:
        assert cnt["prod"] == 0 and cnt["pointwise_prod"] == 1, (case, cnt)
        assert cnt["pass"] == 3 * ((2 if two else 1) + 1), (case, cnt)


def test_prod_option_and_query(prod_cpu):
    L = api.lib()
    for shape, kw, want in (((10, 12, 64), {}, 1), ((6, 8, 128), {}, 1), ((6, 8, 96), {}, 0), ((4, 4, 2048), {}, 0),
                            ((8, 6, 64), dict(r2c=1), 0), ((8, 8, 64), dict(params={"S": 1}), 0), ((8, 8, 64), dict(eq=1), 0),
                            ((8, 8, 64), dict(f32=1), 1)):
        po = HW.make_plan(api, dict(N=list(shape), **kw))
        try:
            for val, back in ((1, 1), (0, 0), (5, 1)):
                assert L.offt_hip_set_option(po, api.OPT_PROD_FUSED, val) == 0
                assert L.offt_hip_get_option(po, api.OPT_PROD_FUSED) == back
                assert L.offt_hip_product_fused(po) == (want if back else 0), (shape, kw, val)
            for unassigned in (15, 17, 22):
                assert L.offt_hip_set_option(po, unassigned, 1) == -1 and L.offt_hip_get_option(po, unassigned) == -1
        finally:
            api.offt_3d_fin(po)
    po = HW.make_plan(api, dict(N=[16, 16, 64]))                # a half box: generic
    try:
        assert L.offt_hip_set_option(po, api.OPT_PROD_FUSED, 1) == 0 and L.offt_hip_product_fused(po) == 1
        api.offt_hip_set_half_box(po, True)
        assert L.offt_hip_product_fused(po) == 0
    finally:
        api.offt_3d_fin(po)


@pytest.mark.parametrize("shape", [(10, 12, 64), (6, 8, 128)])
@pytest.mark.parametrize("f32", [0, 1])
def test_prod_single_rank_both_routes(prod_cpu, shape, f32):
    case = dict(N=list(shape), f32=f32)
    for opt in (1, 0):
        err, fused, cnt, log = _run(prod_cpu, case, opt)
        assert fused == bool(opt), (case, opt)
        assert err <= W.tol(case), (case, opt, err)
        _assert_route(case, fused, cnt, log)


@pytest.mark.parametrize("case", [dict(N=[12, 10, 9]), dict(N=[8, 6, 16], r2c=1), dict(N=[6, 5, 9], r2c=1),
                                  dict(N=[8, 8, 16], params={"S": 1}), dict(N=[8, 8, 16], eq=1), dict(N=[8, 6, 16], r2c=1, f32=1)])
def test_prod_generic_shapes(prod_cpu, case):
    for mode in ("two", "null"):
        c = dict(case, mode=mode)
        err, fused, cnt, log = _run(prod_cpu, c, 1)
        assert not fused and err <= W.tol(c), (c, err)
        _assert_route(c, fused, cnt, log)


@pytest.mark.parametrize("opt", [1, 0])
def test_prod_aliasing_and_squaring(prod_cpu, opt):
    base = dict(N=[6, 8, 64])
    got = {}
    for mode in ("two", "a", "b", "null", "same"):
        keep = {}
        case = dict(base, mode=mode)
        err, fused, cnt, log = _run(prod_cpu, case, opt, keep=keep)
        assert fused == bool(opt) and err <= W.tol(case), (mode, opt, err)
        _assert_route(case, fused, cnt, log)
        got[mode] = keep["got"]
    # squaring against the two-buffer call on a copy of a: equal to rounding
    po = _plan(base, opt)
    try:
        c, ne = api.comm_dict(po), api.local_elems(po)
        A = PW.problem(base)[0]
        a, a2, out = PW.spec_buffer(c, ne, base, A), PW.spec_buffer(c, ne, base, A), np.zeros(ne, dtype=np.complex128)
        api.offt_hip_execute_product(po, a.ctypes.data, a2.ctypes.data, out.ctypes.data)
        idx = W.out_index(c)
        for mode in ("null", "same"):
            assert np.linalg.norm(got[mode][idx] - out[idx]) <= 1e-13 * np.linalg.norm(out[idx]), mode
    finally:
        api.offt_3d_fin(po)


@pytest.mark.parametrize("opt", [1, 0])
def test_prod_scale_once(prod_cpu, opt):
    case = dict(N=[6, 8, 64])
    n2 = float(np.prod(case["N"])) ** 2
    k1, ks = {}, {}
    e1 = _run(prod_cpu, case, opt, keep=k1)[0]
    es = _run(prod_cpu, case, opt, keep=ks, scale=1.0 / n2)[0]          # fftn(ifftn(A) ifftn(B)) itself
    assert e1 <= 1e-12 and es <= 1e-12, (e1, es)
    assert np.linalg.norm(ks["got"] - k1["got"] / n2) <= 1e-14 * np.linalg.norm(ks["got"])


@pytest.mark.parametrize("opt", [1, 0])
def test_prod_identity(prod_cpu, opt):
    """B = fftn(ones): ifftn(B) N = N everywhere, so the call returns N^2 A"""
    case = dict(N=[6, 8, 64])
    po = _plan(case, opt)
    try:
        c, ne = api.comm_dict(po), api.local_elems(po)
        A = PW.problem(case)[0]
        n = float(np.prod(case["N"]))
        a, b = PW.spec_buffer(c, ne, case, A), PW.spec_buffer(c, ne, case, np.fft.fftn(np.ones(case["N"])))
        api.offt_hip_execute_product(po, a.ctypes.data, b.ctypes.data, a.ctypes.data)
        assert PW.out_err(c, a, A * n * n) <= 1e-12
    finally:
        api.offt_3d_fin(po)


def test_prod_older_backend_tables(prod_cpu):
    import cpu_world
    L, CB = cpu_world.test_lib(), prod_cpu
    case = dict(N=[6, 8, 64])
    L.offt_hip_test_set_backend(CB.cpu_backend_prod_table_nofused(), 0, 1)      # prod_pass NULL: generic
    err, fused, cnt, log = _run(CB, case, 1)
    assert not fused and err <= 1e-12
    _assert_route(case, fused, cnt, log)
    L.offt_hip_test_set_backend(CB.cpu_backend_prod_table_old(), 0, 1)          # both NULL: refused, nothing launched
    po = _plan(case, 1)
    try:
        c, ne = api.comm_dict(po), api.local_elems(po)
        a = PW.spec_buffer(c, ne, case, PW.problem(case)[0])
        n0 = PW.counts(CB)
        assert api.lib().offt_hip_execute_product(po, a.ctypes.data, None, a.ctypes.data) == -1
        assert b"no pointwise product" in api.lib().offt_hip_last_error() and po.contents.t[api.ALL] >= 99999999.0
        assert PW.counts(CB) == n0 and api.lib().offt_hip_product_fused(po) == 0
    finally:
        api.offt_3d_fin(po)


def test_prod_refusals(prod_cpu):
    """NULL a / out (a host pointer counts as device memory on the CPU backend: test_gpu_product.py refuses those); the plan
    still transforms afterwards"""
    L, CB = api.lib(), prod_cpu
    case = dict(N=[6, 8, 64])
    po = _plan(case, 1)
    try:
        c, ne = api.comm_dict(po), api.local_elems(po)
        A = PW.problem(case)[0]
        a = PW.spec_buffer(c, ne, case, A)
        n0 = PW.counts(CB)
        for args, text in (((None, a.ctypes.data, a.ctypes.data), b"the first spectrum"), ((a.ctypes.data, None, None), b"the output")):
            assert L.offt_hip_execute_product(po, *args) == -1
            assert text in L.offt_hip_last_error() and b"NULL" in L.offt_hip_last_error()
            assert po.contents.t[api.ALL] >= 99999999.0
        assert PW.counts(CB) == n0
        x = np.fft.ifftn(A)
        buf = np.zeros(ne, dtype=np.complex128)
        buf[W.in_index(c, False)] = x.ravel()
        api.offt_3d_execute_dir(po, buf.ctypes.data, buf.ctypes.data, -1)
        assert PW.out_err(c, buf, A) <= 1e-12
    finally:
        api.offt_3d_fin(po)


def test_prod_second_scratch_lifecycle(prod_cpu):
    CB = prod_cpu
    case = dict(N=[6, 8, 64])
    allocs = CB.cpu_backend_alloc_count

    def call(po, mode):
        n0 = allocs()
        CB.cpu_backend_prod_log_reset()
        err = PW.run_product(api, po, dict(case, mode=mode), HW.Host())
        assert err <= 1e-12, (mode, err)
        return allocs() - n0, [r[0] for r in PW.launches(CB)].count(1)

    po = _plan(case, 0)                      # the generic route: none
    try:
        assert call(po, "two") == (0, 0)
    finally:
        api.offt_3d_fin(po)
    po = _plan(case, 1)
    try:
        assert call(po, "null") == (0, 1)    # squaring: none
        assert call(po, "two") == (1, 1)     # the first two-source call makes it ...
        assert call(po, "b") == (0, 1)       # ... the second reuses it
    finally:
        api.offt_3d_fin(po)
    po = _plan(case, 1)
    try:
        CB.cpu_backend_fail_alloc_at(1)      # no memory for it: this call and the later ones run generic, and stay correct
        assert call(po, "two") == (1, 0)
        assert call(po, "two") == (0, 0)
    finally:
        api.offt_3d_fin(po)


def test_prod_half_box(prod_cpu):
    case = dict(N=[16, 16, 16], half=1)
    for mode in ("two", "a"):
        err, fused, cnt, log = _run(prod_cpu, dict(case, mode=mode), 1)
        assert not fused and err <= 1e-12, (mode, err)
        assert cnt["prod"] == 0 and cnt["pointwise_prod"] == 1


# ---- gloo world ----------------------------------------------------------------------------------------------------------------
def test_prod_gloo_world2(built, tmp_path):
    """The product is the FIRST call on each plan, so its inverses are the plan's first transforms: the slab schedule used to
    record the K1 passes of such an inverse under chunk 0's tag and replay them ahead of the exchanges (rel-L2 0.71)."""
    subprocess.check_call(["make", "-s", "-C", ROOT, "tests/libcpubackend_prod.so"])
    cases = [dict(N=[16, 12, 8]), dict(N=[16, 12, 8], r2c=1, mode="a")]
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OFFT_PROD_FUSED="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_prod_world.py"), "gloo", json.dumps(cases),
                                       str(tmp_path)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = [p.communicate(timeout=600)[0].decode() for p in procs]
    for r, p in enumerate(procs):
        assert p.returncode == 0, outs[r][-3000:]
    for r in range(2):
        for rec in json.load(open(tmp_path / f"gloo_rank{r}.json")):
            assert rec["rel"] <= rec["tol"], (r, rec)
            assert not rec["fused"] and rec["counts"]["prod"] == 0 and rec["counts"]["pointwise_prod"] == 1, rec
