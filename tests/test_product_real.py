"""Pseudo-spectral product on real-input (r2c) plans, the fused route (OFFT_HIP_OPT_PROD_REAL on top of
OFFT_HIP_OPT_PROD_FUSED), without a GPU.

  * the option (25), its environment default, and offt_hip_product_fused: 1 only with both options and the backend entry
    prod_pass_real, 0 for everything the route leaves to the generic one;
  * the registry lookup of the real kernel (offt_hipk_prod_real_has_fused) without a device;
  * both host routes on the CPU backend of tests/cpu_backend_prod_real.c, whose prod_pass_real is written from the definition
    (one source at a time, no packing), read off the launch logs: aliasing of `out`, squaring, the second scratch volume and
    its failure, the output scale, a gloo world of 2 ranks.

The reference is numpy in float64 on the host: N^2 rfftn(irfftn(A) irfftn(B)) (_prod_world.problem).  Tolerance: the project's
plan-level W.tol (1e-12 f64, 2e-5 f32), rel-L2 against the norm of the reference.  Single precision: the kernel's packed chain
(A~ + i B~, one complex64 inverse, -Re.Im, complex64 forward) emulated in complex64 on the CPU (torch.fft, against numpy in
double) gives rel-L2 2.0e-7 on 1024-point lines and 2.7e-7 on the (4, 24, 1024) plan, inside both
single-precision bounds (1e-5 descriptor level, 2e-5 plan level), which therefore stand."""
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
import _prod_real_world as RW
import _prod_world as PW
from offt_amd import api
from test_convolve_multi import Desc
from test_product import prod_desc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(10, 12, 64), (6, 8, 128)]
MODES = ("two", "a", "b", "null", "same")


def real_desc(n, prec, ncols, nb1, pitch=None, plane_pad=0):
    """the real-output z pass over W[x][z][y]: lines of n/2+1 complex values, column c of plane b1 at b1 * plane + c, element
    k at k * pitch; the real rows on the output side"""
    pitch = pitch or ncols
    d = prod_desc(n, prec, ncols, nb1, pitch=pitch)
    d.in_b1_stride = (n // 2 + 1) * pitch + plane_pad
    d.real_input = 2
    return d


# ---- 1. routing without a device ---------------------------------------------------------------------------------------------
def test_prod_real_kernel_routing_without_a_gpu(built):
    L = api.lib()
    L.offt_hipk_prod_real_has_fused.argtypes = [C.POINTER(Desc)]
    L.offt_hipk_prod_real_kernel_name.restype = C.c_char_p
    L.offt_hipk_prod_real_kernel_name.argtypes = [C.POINTER(Desc)]
    L.offt_hipk_prod_has_fused.argtypes = [C.POINTER(Desc)]
    for prec in (api.F64, api.F32):
        for n in (64, 128, 256, 512, 1024):
            d = real_desc(n, prec, 12, 3, pitch=20)
            assert L.offt_hipk_prod_real_has_fused(C.byref(d)) == 1, (n, prec)
            assert L.offt_hipk_prod_real_kernel_name(C.byref(d)) == b"fft_prod_real_panel_k"
            assert L.offt_hipk_prod_has_fused(C.byref(d)) == 0       # the complex entry still refuses real_input = 2
        for n in (32, 96, 2048):
            d = real_desc(n, prec, 12, 3)
            assert L.offt_hipk_prod_real_has_fused(C.byref(d)) == 0, (n, prec)
            assert L.offt_hipk_prod_real_kernel_name(C.byref(d)) == b"no fused kernel"
        for field, val in (("in_contig", 1), ("in_split", 64), ("half", 2), ("real_input", 0), ("real_input", 1)):
            d = real_desc(256, prec, 8, 2)
            setattr(d, field, val)
            assert L.offt_hipk_prod_real_has_fused(C.byref(d)) == 0, (field, val, prec)
    assert L.offt_hipk_prod_real_has_fused(None) == 0


# ---- CPU tier ----------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def real_cpu(built):
    import cpu_world
    subprocess.check_call(["make", "-s", "-C", ROOT, "tests/libcpubackend_prod_real.so"])
    orig = cpu_world._cb_lib
    cpu_world._cb_lib = RW.real_cb_lib
    CB = cpu_world.install(0, 1, p1=1)
    yield CB
    cpu_world.uninstall()
    cpu_world._cb_lib = orig


def _plan(case, fused=1, real=1):
    po = HW.make_plan(api, case)
    L = api.lib()
    assert L.offt_hip_set_option(po, api.OPT_PROD_FUSED, fused) == 0 and L.offt_hip_set_option(po, api.OPT_PROD_REAL, real) == 0
    return po


def _call(CB, po, case, keep=None, scale=None):
    """one product on the plan: (error, launch counts, plain-pass log, real-launch log)"""
    n0 = RW.counts(CB)
    RW.log_reset(CB)
    err = PW.run_product(api, po, case, HW.Host(), keep=keep, scale=scale)
    n1 = RW.counts(CB)
    return err, {k: n1[k] - n0[k] for k in n0}, PW.launches(CB), RW.real_launches(CB)


def _run(CB, case, fused=1, real=1, keep=None, scale=None):
    po = _plan(case, fused, real)
    try:
        return (api.offt_hip_product_fused(po),) + _call(CB, po, case, keep=keep, scale=scale)
    finally:
        api.offt_3d_fin(po)


def _assert_route(case, fused, cnt, log, rlog):
    two = case.get("mode", "two") in ("two", "a", "b")
    nz = case["N"][2]
    assert cnt["prod"] == 0, (case, cnt)                          # never the complex launch on a real-input plan
    if fused:
        assert cnt["prod_real"] == 1 and cnt["pointwise_prod"] == 0, (case, cnt)
        ninv = 4 if two else 2
        # exactly one real launch: the real-output z pass's descriptor, after the inverses' x and y passes, before the forward's
        assert [(r[1], r[6], r[7], r[8]) for r in rlog] == [(nz, 2, 2 if two else 1, ninv)], (case, rlog)
        assert all(r[0] == 0 for r in log) and len(log) == ninv + 2, (case, log)
        # no z pass of either direction: no pass of the z length, none with a real side
        assert case["N"][0] != nz and case["N"][1] != nz and all(r[1] != nz and r[6] == 0 for r in log), (case, log)
        assert [r[2] for r in log] == [1] * ninv + [-1] * 2, (case, log)
        assert all(r[4] == nz // 2 + 1 for r in log), (case, log)   # over the Nz/2+1 planes of the half spectrum
    else:
        assert cnt["prod_real"] == 0 and cnt["pointwise_prod"] == 1 and rlog == [], (case, cnt)
        assert cnt["pass"] == 3 * ((2 if two else 1) + 1), (case, cnt)


def test_prod_real_option(real_cpu, monkeypatch):
    L = api.lib()
    po = HW.make_plan(api, dict(N=[8, 6, 64], r2c=1))
    try:
        assert L.offt_hip_get_option(po, api.OPT_PROD_REAL) == 0 and L.offt_hip_get_option(po, api.OPT_PROD_FUSED) == 0   # both defaults
        for val, back in ((1, 1), (0, 0), (5, 1), (-3, 1)):
            assert L.offt_hip_set_option(po, api.OPT_PROD_REAL, val) == 0
            assert L.offt_hip_get_option(po, api.OPT_PROD_REAL) == back
        assert api.OPT_PROD_REAL == 25
        for unassigned in (15, 17, 22, 26):
            assert L.offt_hip_set_option(po, unassigned, 1) == -1 and L.offt_hip_get_option(po, unassigned) == -1
    finally:
        api.offt_3d_fin(po)
    for env, want in (("1", 1), ("0", 0), ("7", 1)):
        monkeypatch.setenv("OFFT_PROD_REAL", env)
        po = HW.make_plan(api, dict(N=[8, 6, 64], r2c=1))
        try:
            assert L.offt_hip_get_option(po, api.OPT_PROD_REAL) == want, env
            assert L.offt_hip_get_option(po, api.OPT_PROD_FUSED) == 0        # one default does not set the other
        finally:
            api.offt_3d_fin(po)


def test_prod_real_query(real_cpu):
    import cpu_world
    L, CB = api.lib(), real_cpu

    def fused(case, f=1, r=1, half=False):
        po = _plan(case, f, r)
        try:
            if half:
                api.offt_hip_set_half_box(po, True)
            return L.offt_hip_product_fused(po)
        finally:
            api.offt_3d_fin(po)

    for shape in SHAPES + [(8, 6, 1024)]:
        for f32 in (0, 1):
            case = dict(N=list(shape), r2c=1, f32=f32)
            assert fused(case) == 1, case
            assert fused(case, 1, 0) == 0 and fused(case, 0, 1) == 0 and fused(case, 0, 0) == 0, case   # one option alone: generic
    for nz in (96, 32, 2048):
        assert fused(dict(N=[6, 8, nz], r2c=1)) == 0, nz
    assert fused(dict(N=[8, 8, 64], r2c=1, params={"S": 1})) == 0
    assert fused(dict(N=[8, 8, 64], r2c=1, eq=1)) == 0
    assert fused(dict(N=[16, 16, 64], r2c=1)) == 1 and fused(dict(N=[16, 16, 64], r2c=1), half=True) == 0
    # a complex plan does not read the option
    assert fused(dict(N=[6, 8, 64]), 1, 0) == 1 and fused(dict(N=[6, 8, 64]), 0, 1) == 0
    # a backend table older than the entry: generic, whatever the options
    cpu_world.test_lib().offt_hip_test_set_backend(CB.cpu_backend_prod_table(), 0, 1)
    assert fused(dict(N=[6, 8, 64], r2c=1)) == 0 and fused(dict(N=[6, 8, 64])) == 1
    case = dict(N=[6, 8, 64], r2c=1)
    isf, err, cnt, log, rlog = _run(CB, case)
    assert not isf and err <= W.tol(case)
    _assert_route(case, False, cnt, log, rlog)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("f32", [0, 1])
def test_prod_real_both_routes(real_cpu, shape, f32):
    base = dict(N=list(shape), r2c=1, f32=f32)
    got = {}
    for real in (1, 0):
        for mode in MODES:
            case = dict(base, mode=mode)
            keep = {}
            fused, err, cnt, log, rlog = _run(real_cpu, case, 1, real, keep=keep)
            assert fused == real, (case, real)
            assert err <= W.tol(case), (case, real, err)
            _assert_route(case, fused, cnt, log, rlog)
            got[real, mode] = keep["got"]
    po = _plan(base)
    try:
        idx = W.out_index(api.comm_dict(po))
    finally:
        api.offt_3d_fin(po)
    for mode in MODES:           # the two routes agree to the tolerance as well
        a, b = got[1, mode][idx].astype(np.complex128), got[0, mode][idx].astype(np.complex128)
        assert np.linalg.norm(a - b) <= W.tol(base) * np.linalg.norm(b), mode
    for mode in ("null", "same"):  # squaring is squaring
        a, b = got[1, mode][idx].astype(np.complex128), got[1, "null"][idx].astype(np.complex128)
        assert np.array_equal(a, b)


def test_prod_real_second_scratch_lifecycle(real_cpu):
    CB = real_cpu
    case = dict(N=[6, 8, 64], r2c=1)
    allocs = CB.cpu_backend_alloc_count

    def call(po, mode, keep=None):
        n0 = allocs()
        err, cnt, log, rlog = _call(CB, po, dict(case, mode=mode), keep=keep)
        assert err <= 1e-12, (mode, err)
        return allocs() - n0, cnt["prod_real"], cnt["pointwise_prod"]

    po = _plan(case)
    try:
        assert call(po, "null") == (0, 1, 0)    # squaring: none
        good = {}
        assert call(po, "two", good) == (1, 1, 0)   # the first two-source call makes it ...
        assert call(po, "b") == (0, 1, 0)       # ... the second reuses it
    finally:
        api.offt_3d_fin(po)
    po = _plan(case)
    try:
        CB.cpu_backend_fail_alloc_at(1)         # no memory for it: this call and the later ones run generic, with equal results
        k1, k2 = {}, {}
        assert call(po, "two", k1) == (1, 0, 1)
        assert call(po, "two", k2) == (0, 0, 1)
        idx = W.out_index(api.comm_dict(po))
        assert np.array_equal(k1["got"][idx], k2["got"][idx])
        assert np.linalg.norm(k1["got"][idx] - good["got"][idx]) <= 1e-12 * np.linalg.norm(good["got"][idx])
    finally:
        api.offt_3d_fin(po)


@pytest.mark.parametrize("real", [1, 0])
def test_prod_real_scale_once(real_cpu, real):
    case = dict(N=[6, 8, 64], r2c=1)
    n2 = float(np.prod(case["N"])) ** 2
    k1, ks = {}, {}
    f1, e1 = _run(real_cpu, case, 1, real, keep=k1)[:2]
    fs, es = _run(real_cpu, case, 1, real, keep=ks, scale=1.0 / n2)[:2]      # rfftn(irfftn(A) irfftn(B)) itself
    assert f1 == real and fs == real
    assert e1 <= 1e-12 and es <= 1e-12, (e1, es)
    po = _plan(case)
    try:
        idx = W.out_index(api.comm_dict(po))
    finally:
        api.offt_3d_fin(po)
    assert np.linalg.norm(ks["got"][idx] - k1["got"][idx] / n2) <= 1e-14 * np.linalg.norm(ks["got"][idx])


def test_prod_real_end_planes_have_no_effect(real_cpu):
    """A constant added to the imaginary parts of the planes z = 0 and z = Nz/2 of both inputs: the inverse's x and y passes
    turn it into a purely imaginary end element of the z line at x = y = 0, which a c2r inverse discards.  The packed form
    would carry Im A[0] into field b and Im B[0] into field a unless it drops them: the result must not move on either route."""
    case = dict(N=[6, 8, 64], r2c=1)
    A, B, want, _ = PW.problem(case)
    for real in (1, 0):
        po = _plan(case, 1, real)
        try:
            c, ne = api.comm_dict(po), api.local_elems(po)
            outs = []
            for bump in (0.0, 0.37):
                A2, B2 = A.copy(), B.copy()
                for X, s in ((A2, 1.0), (B2, -2.0)):
                    X[:, :, 0] += 1j * bump * s
                    X[:, :, -1] += 1j * bump * s * 0.5
                a, b = PW.spec_buffer(c, ne, case, A2), PW.spec_buffer(c, ne, case, B2)
                out = np.zeros(ne, dtype=np.complex128)
                api.offt_hip_execute_product(po, a.ctypes.data, b.ctypes.data, out.ctypes.data)
                assert PW.out_err(c, out, want) <= 1e-12, (real, bump)
                outs.append(out[W.out_index(c)])
            assert np.linalg.norm(outs[1] - outs[0]) <= 1e-13 * np.linalg.norm(outs[0]), real
        finally:
            api.offt_3d_fin(po)


# ---- gloo world -----------------------------------------------------------------------------------------------------------------
def test_prod_real_gloo_world2(built, tmp_path):
    """two ranks: the generic route, with both options set through the environment and the backend entry present"""
    subprocess.check_call(["make", "-s", "-C", ROOT, "tests/libcpubackend_prod_real.so"])
    cases = [dict(N=[16, 12, 64], r2c=1)]
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OFFT_PROD_FUSED="1",
                   OFFT_PROD_REAL="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_prod_real_world.py"), "gloo", json.dumps(cases),
                                       str(tmp_path)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = [p.communicate(timeout=600)[0].decode() for p in procs]
    for r, p in enumerate(procs):
        assert p.returncode == 0, outs[r][-3000:]
    for r in range(2):
        for rec in json.load(open(tmp_path / f"gloo_rank{r}.json")):
            assert rec["opts"] == [1, 1], rec
            assert rec["rel"] <= rec["tol"], (r, rec)
            assert not rec["fused"] and rec["counts"]["prod_real"] == 0 and rec["counts"]["prod"] == 0, rec
            assert rec["counts"]["pointwise_prod"] == 1, rec
