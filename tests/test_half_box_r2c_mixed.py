"""Real-input half-box plans at mixed-radix lengths: OFFT_HIP_OPT_HALF_R2C_MIXED (include/offt_hip.h), bit 4 of
offt_pass_desc::half and the two kernels under it, fft_half_r2c_panelx_k (real_input = 1 with half = 1 | 4) and
fft_half_c2r_panelx_k (real_input = 2 with half = 2 | 4).

  * routing without a device: with bit 4 the two real forms have a kernel at every registered mixed-radix (length,
    precision) pair, without it they have none (what tests/test_half_box_mixed.py pins), and bit 4 opens nothing else;
  * the host's route on the CPU backend of tests/cpu_backend_padreal_mixed.c, the padding NaN: the new option and its two
    older siblings one by one and in pairs (fallback), all three (pruned, half = 5 / 6 on the real passes exactly where Nz
    is mixed), the option switched on and off on a live plan, a power-of-two plan;
  * the environment default in a fresh process;
  * -m gpu: the two kernels descriptor by descriptor (NaN in what must not be read, a sentinel in what must not be
    written), plans on one rank, a free-space convolution of a 48^3 box on a real 96^3 plan, unfused and fused."""
import ctypes as C
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _conv_world as W
import _half_world as HW
from offt_amd import api
from test_half_box import _check, kl  # noqa: F401  (kl: the fixture that binds the kernel ABI)
from test_half_box_mixed import LENGTHS, _free_space_problem
from test_half_box_r2c import _cidx, real_desc, table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R2C_K, C2R_K = "fft_half_r2c_panelx_k", "fft_half_c2r_panelx_k"
OPTS = ("OPT_HALF_R2C", "OPT_HALF_MIXED", "OPT_HALF_R2C_MIXED")


def _bit4(d):
    d.half |= 4
    return d


# ---- routing without a device ---------------------------------------------------------------------------------------------
def test_half_real_mixed_kernel_routing_without_a_gpu(kl):
    L = kl
    has = lambda d: L.offt_hipk_has_half(C.byref(d))
    name = lambda d: L.offt_hipk_kernel_name(C.byref(d)).decode()
    none = lambda d: has(d) == 0 and name(d) == "no half-line kernel"
    for prec, lengths in LENGTHS.items():
        for n in lengths:
            for ncols in (8, 7):
                for form, want in (("r2c", R2C_K), ("c2r", C2R_K)):
                    d = _bit4(real_desc(n, prec, ncols, 2, form))
                    assert d.half == (5 if form == "r2c" else 6)
                    assert has(d) == 1 and name(d) == want, (n, prec, ncols, form)
                    assert L.offt_hipk_keeps_output(C.byref(d)) == 0
                    # the same descriptor without the permission: no kernel, as before there was one to permit
                    assert none(real_desc(n, prec, ncols, 2, form)), (n, prec, ncols, form)
            # with bit 4: the other bit, both bits, the other real kind, the other flavours -- no kernel
            for form, ri, half, inc, outc in [("r2c", 1, 2, 1, 0), ("r2c", 1, 3, 1, 0), ("r2c", 2, 1, 1, 0), ("r2c", 1, 1, 1, 1), ("r2c", 1, 1, 0, 1),
                                              ("r2c", 1, 1, 0, 0), ("c2r", 2, 1, 0, 1), ("c2r", 2, 3, 0, 1), ("c2r", 1, 2, 0, 1), ("c2r", 2, 2, 1, 1),
                                              ("c2r", 2, 2, 1, 0), ("c2r", 2, 2, 0, 0)]:
                d = real_desc(n, prec, 8, 2, form)
                d.real_input, d.half, d.in_contig, d.out_contig = ri, half | 4, inc, outc
                assert none(d), (n, prec, ri, half, inc, outc)
            for form in ("r2c", "c2r"):
                # a split, four-step twiddles
                for field in ("in_split", "out_split", "in_split_nfloor", "out_split_nfloor"):
                    d = _bit4(real_desc(n, prec, 8, 2, form))
                    setattr(d, field, n // 4)
                    assert none(d), (n, prec, form, field)
                d = _bit4(real_desc(n, prec, 8, 2, form))
                d.tw4 = 64   # (any non-NULL value: a lookup never follows it)
                assert has(d) == 0, (n, prec, form)
                # a complex descriptor with bit 4, and bit 4 alone
                d = _bit4(real_desc(n, prec, 8, 2, form))
                d.real_input = 0
                assert none(d), (n, prec, form)
                d = real_desc(n, prec, 8, 2, form)
                d.half = 4
                assert none(d), (n, prec, form)
                d.real_input = 0
                assert none(d), (n, prec, form)
            d = _bit4(real_desc(n, prec, 8, 2, "r2c"))
            d.direction = +1   # a real-input pass is a forward pass (as on full lines)
            assert has(d) == 0, (n, prec)
    # single precision has no mixed-radix instance below 384 points; 250, 240, 48: swept, but not registered
    for prec, lengths in ((api.F32, (96, 192, 320)), (api.F32, (250, 240, 48)), (api.F64, (250, 240, 48))):
        for n in lengths:
            for form in ("r2c", "c2r"):
                assert none(_bit4(real_desc(n, prec, 8, 2, form))), (n, prec, form)
    # a power of two resolves with the permission to what it resolves to without it
    for prec in (api.F64, api.F32):
        for n in (64, 128, 256, 512, 1024):
            for form, want in (("r2c", "fft_half_r2c_panel_k"), ("c2r", "fft_half_c2r_panel_k")):
                d = _bit4(real_desc(n, prec, 8, 2, form))
                assert has(d) == 1 and name(d) == want, (n, prec, form)
                assert name(real_desc(n, prec, 8, 2, form)) == want


# ---- CPU tier: the host's route on the padreal-mixed backend --------------------------------------------------------------
def padreal_mixed_cb_lib():
    """tests/libcpubackend_padreal_mixed.so, shaped like cpu_world's backend library (its table = the padreal-mixed table)"""
    L = C.CDLL(os.path.join(ROOT, "tests", "libcpubackend_padreal_mixed.so"))
    for f in ("cpu_backend_padreal_mixed_table", "cpu_backend_padreal_mixed_table_unfused"):
        getattr(L, f).restype = C.c_void_p
    L.cpu_backend_table = L.cpu_backend_padreal_mixed_table
    for f in ("cpu_backend_pass_count", "cpu_backend_pad_zero_count", "cpu_backend_pointwise_count"):
        getattr(L, f).restype = C.c_long
    L.cpu_backend_padreal_mixed_log.argtypes = [C.c_int, C.POINTER(C.c_int)]
    return L


def launches(CB):
    """the launches recorded since the last reset, as the host sent them: (n, ncols, nb1, nb2, half, conv, real_input)"""
    out, rec, i = [], (C.c_int * 7)(), 0
    while CB.cpu_backend_padreal_mixed_log(i, rec) == 0:
        out.append(tuple(rec))
        i += 1
    return out


@pytest.fixture()
def padreal_mixed_cpu(built):
    import cpu_world
    subprocess.check_call(["make", "-s", "-C", ROOT, "tests/libcpubackend_padreal_mixed.so"])
    orig = cpu_world._cb_lib
    cpu_world._cb_lib = padreal_mixed_cb_lib
    CB = cpu_world.install(0, 1, p1=1)
    yield CB
    cpu_world.uninstall()
    cpu_world._cb_lib = orig


def mixed_table(shape):
    """test_half_box_r2c.table with bit 4 on the two real passes exactly where Nz is no power of two"""
    Nz = shape[2]
    bit = 4 if Nz & (Nz - 1) else 0
    return tuple([r[:4] + (r[4] | (bit if r[6] else 0),) + r[5:] for r in part] for part in table(shape))


def _set(L, po, **opts):
    for k, v in opts.items():
        assert L.offt_hip_set_option(po, getattr(api, k), v) == 0, L.offt_hip_last_error()
        assert L.offt_hip_get_option(po, getattr(api, k)) == v


def _fallback_run(CB, po, case, pr):
    """one run of the plan that has to take the fallback: two clears, no half launch, results within the bounds"""
    assert not api.offt_hip_half_box_pruned(po)
    z0 = CB.cpu_backend_pad_zero_count()
    CB.cpu_backend_padreal_mixed_log_reset()
    res, _ = HW.run_plan(api, po, case, HW.Host(), pr)
    _check(res, case)
    assert CB.cpu_backend_pad_zero_count() == z0 + 2, "the forward and the convolve clear the padding, the inverse does not"
    assert launches(CB) and all(r[4] == 0 for r in launches(CB)), "no half-line launch on the fallback route"


# only z mixed; only x mixed (no descriptor carries bit 4); y and z mixed with x = 64
@pytest.mark.parametrize("shape", [(64, 64, 96), (96, 64, 64), (64, 96, 192)])
def test_half_box_r2c_mixed_route_cpu(padreal_mixed_cpu, shape):
    CB = padreal_mixed_cpu
    L = api.lib()
    case = dict(N=list(shape), r2c=1)
    po = HW.make_plan(api, case)
    try:
        pr = HW.problem(case["N"], 1)
        for k in OPTS:
            assert L.offt_hip_get_option(po, getattr(api, k)) == 0, "off by default"
        _set(L, po, OPT_HALF_R2C_MIXED=1)
        assert not api.offt_hip_half_box_pruned(po), "the option alone switches no half box on"
        _set(L, po, OPT_HALF_R2C_MIXED=0)
        api.offt_hip_set_half_box(po, True)
        # none, each of the three alone, each pair: the fallback (the subsets are set on the live plan, half box on)
        for r in (0, 1, 2):
            for on in itertools.combinations(OPTS, r):
                _set(L, po, **{k: int(k in on) for k in OPTS})
                assert not api.offt_hip_half_box_pruned(po), on
                _fallback_run(CB, po, case, pr)
        # all three, the last one switched on on the live plan (its inverse schedule is cached by now): the pruned route
        _set(L, po, OPT_HALF_R2C=1, OPT_HALF_MIXED=1, OPT_HALF_R2C_MIXED=0)
        assert not api.offt_hip_half_box_pruned(po)
        _set(L, po, OPT_HALF_R2C_MIXED=1)
        assert api.offt_hip_half_box_pruned(po), "the half box was on: the option re-evaluates the route"
        z0 = CB.cpu_backend_pad_zero_count()
        p0 = CB.cpu_backend_pointwise_count()
        CB.cpu_backend_padreal_mixed_log_reset()
        res, _ = HW.run_plan(api, po, case, HW.Host(), pr)
        _check(res, case)
        assert CB.cpu_backend_pad_zero_count() == z0, "a pruned plan clears nothing"
        fwd, inv, conv = mixed_table(shape)
        real_half = (5, 6) if shape[2] & (shape[2] - 1) else (1, 2)
        assert (fwd[0][4], inv[2][4]) == real_half
        assert all(r[4] in (1, 2, 3) for r in fwd[1:] + inv[:2] + conv[2:3]), "bit 4 on the real passes only"
        if shape[0] == 64:
            assert api.offt_hip_convolve_fused(po)
            assert launches(CB) == fwd + inv + conv and CB.cpu_backend_pointwise_count() == p0
        else:   # pruned forward, one multiply, pruned inverse
            assert not api.offt_hip_convolve_fused(po)
            assert launches(CB) == fwd + inv + fwd + inv and CB.cpu_backend_pointwise_count() == p0 + 1
        # off again on the live plan: back to the fallback, and no pruned inverse schedule is replayed
        _set(L, po, OPT_HALF_R2C_MIXED=0)
        _fallback_run(CB, po, case, pr)
        # the two older options switched on the live plan re-evaluate the route with the new one set
        _set(L, po, OPT_HALF_R2C_MIXED=1)
        assert api.offt_hip_half_box_pruned(po)
        _set(L, po, OPT_HALF_MIXED=0)
        assert not api.offt_hip_half_box_pruned(po)
        _set(L, po, OPT_HALF_MIXED=1, OPT_HALF_R2C=0)
        assert not api.offt_hip_half_box_pruned(po)
        _set(L, po, OPT_HALF_R2C=1)
        assert api.offt_hip_half_box_pruned(po)
        api.offt_hip_set_half_box(po, False)
        assert not api.offt_hip_half_box_pruned(po)
    finally:
        api.offt_3d_fin(po)


def test_half_box_r2c_mixed_other_plans_cpu(padreal_mixed_cpu):
    CB = padreal_mixed_cpu
    L = api.lib()
    # a power-of-two r2c plan with the option on: the descriptors of before, half = 1 / 2 and nothing else
    shape = (64, 64, 64)
    case = dict(N=list(shape), r2c=1)
    po = HW.make_plan(api, case)
    try:
        _set(L, po, OPT_HALF_R2C=1, OPT_HALF_R2C_MIXED=1)
        api.offt_hip_set_half_box(po, True)
        assert api.offt_hip_half_box_pruned(po)
        CB.cpu_backend_padreal_mixed_log_reset()
        res, _ = HW.run_plan(api, po, case, HW.Host())
        _check(res, case)
        fwd, inv, conv = table(shape)
        assert launches(CB) == fwd + inv + conv
        assert {r[4] for r in launches(CB) if r[6]} == {1, 2}
    finally:
        api.offt_3d_fin(po)
    # a complex mixed-radix plan does not care about the option: OFFT_HIP_OPT_HALF_MIXED alone decides, as before
    po = HW.make_plan(api, dict(N=[96, 64, 192]))
    try:
        api.offt_hip_set_half_box(po, True)
        for mixed, new in ((0, 1), (1, 0), (1, 1), (0, 0)):
            _set(L, po, OPT_HALF_MIXED=mixed, OPT_HALF_R2C_MIXED=new)
            assert api.offt_hip_half_box_pruned(po) == mixed, (mixed, new)
    finally:
        api.offt_3d_fin(po)
    # all three options on, but a length without a half-line kernel, another layout: the fallback
    for case in (dict(N=[96, 64, 250], r2c=1), dict(N=[48, 40, 30], r2c=1), dict(N=[64, 64, 96], r2c=1, params={"S": 1})):
        po = HW.make_plan(api, case)
        try:
            _set(L, po, OPT_HALF_R2C=1, OPT_HALF_MIXED=1, OPT_HALF_R2C_MIXED=1)
            api.offt_hip_set_half_box(po, True)
            assert not api.offt_hip_half_box_pruned(po), case
        finally:
            api.offt_3d_fin(po)


_ENV_CHILD = """
import sys
sys.path[:0] = [%r, %r]
import cpu_world, test_half_box_r2c_mixed as T, _half_world as HW
from offt_amd import api
cpu_world._cb_lib = T.padreal_mixed_cb_lib
cpu_world.install(0, 1, p1=1)
po = HW.make_plan(api, dict(N=[64, 64, 96], r2c=1))
L = api.lib()
v = L.offt_hip_get_option(po, api.OPT_HALF_R2C_MIXED)
assert L.offt_hip_set_option(po, api.OPT_HALF_R2C, 1) == 0 and L.offt_hip_set_option(po, api.OPT_HALF_MIXED, 1) == 0
api.offt_hip_set_half_box(po, True)
print("RESULT", v, int(api.offt_hip_half_box_pruned(po)))
api.offt_3d_fin(po)
"""


def test_half_box_r2c_mixed_environment_default(built):
    """OFFT_HALF_R2C_MIXED is read once, by offt_3d_init, as the option's default"""
    subprocess.check_call(["make", "-s", "-C", ROOT, "tests/libcpubackend_padreal_mixed.so"])
    for val, want in ((None, "RESULT 0 0"), ("1", "RESULT 1 1"), ("0", "RESULT 0 0")):
        env = {k: v for k, v in os.environ.items() if k not in ("OFFT_HALF_R2C_MIXED", "OFFT_HALF_R2C", "OFFT_HALF_MIXED")}
        if val is not None:
            env["OFFT_HALF_R2C_MIXED"] = val
        p = subprocess.run([sys.executable, "-c", _ENV_CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=300)
        out = p.stdout.decode()
        assert p.returncode == 0 and want in out.splitlines(), (val, out[-2000:])


# ---- GPU tier ----------------------------------------------------------------------------------------------------------
# 96: the smallest; 192: another radix order than its full-line kernel; 320: a predicated first butterfly (40 butterflies on
# 16 threads); 1000 f64: 100 threads a line; 384 f32: the smallest single-precision instance; 1000 f32: predicated first and
# last butterflies (50 and 100 on 40 threads)
@pytest.mark.gpu
@pytest.mark.parametrize("prec,n", [(api.F64, 96), (api.F64, 192), (api.F64, 320), (api.F64, 1000), (api.F32, 384), (api.F32, 1000)])
def test_half_real_mixed_random_descriptors(kl, prec, n):
    """tolerances: those of test_half_box_r2c.py::test_real_half_random_descriptors, 1e-12 / 1e-5 rel-L2 against numpy in
    complex128"""
    import torch
    L = kl
    rng = np.random.default_rng(5200 + n + 7 * prec)
    SENT = 8   # guard, in complex elements
    K = n // 2 + 1
    assert L.offt_hipk_prepare(n, prec) == 0, L.offt_hipk_last_error()
    ft, ct = (np.float64, np.complex128) if prec == api.F64 else (np.float32, np.complex64)
    for ncols in (3, 13, 21, 18):
        nb1 = int(rng.integers(2, 4))
        pad = int(rng.integers(1, 3))
        scale = float(rng.choice([0.5, 1.0 / n, 3.0]))
        # ---- real input: n/2 reals of a row in, n/2+1 complex values out
        d = _bit4(real_desc(n, prec, ncols, nb1, "r2c", pad=pad, scale=scale))
        assert L.offt_hipk_kernel_name(C.byref(d)).decode() == R2C_K
        ri = 2 * _cidx(0, d.in_col_stride, d.in_b1_stride, nb1, ncols, 1) + np.arange(n)[None, None, :]   # scalar index of real k of a row
        oi = _cidx(d.out_axis_stride, d.out_col_stride, d.out_b1_stride, nb1, ncols, K)
        nin, nout = int(ri.max()) // 2 + 2 + pad, int(oi.max()) + 1 + pad
        rows = rng.standard_normal((nb1, ncols, n)).astype(ft)
        rows[:, :, n // 2:] = 0
        x = rng.standard_normal(2 * nin).astype(ft)
        x[ri.ravel()] = rows.ravel()
        x[ri[:, :, n // 2:].ravel()] = np.nan           # what must not be read is NaN, and counts as zero ...
        tail = np.ones(2 * nin, dtype=bool)
        tail[ri.ravel()] = False
        x[tail] = np.nan                                # ... and so is the tail of every row and whatever lies between rows
        want = np.fft.rfft(rows.astype(np.float64), axis=2) * scale
        out0 = np.full(nout + 2 * SENT, 7.0 + 7.0j, dtype=ct)
        out0[SENT:SENT + nout] = (rng.standard_normal(nout) + 1j * rng.standard_normal(nout)).astype(ct)
        dx = torch.from_numpy(x.copy()).cuda()
        do = torch.from_numpy(out0.view(ft).copy()).cuda()
        torch.cuda.synchronize()
        rc = L.offt_hipk_fft_pass(C.byref(d), dx.data_ptr(), do.data_ptr() + SENT * out0.itemsize, None)
        assert rc == 0, L.offt_hipk_last_error()
        torch.cuda.synchronize()
        got = do.cpu().numpy().view(ct)
        written = np.zeros(nout + 2 * SENT, dtype=bool)
        written[SENT + oi.ravel()] = True
        # guard elements and the padding between lines: bit-identical -- exactly the n/2+1 outputs of each line are stored
        assert np.array_equal(got[~written].view(ft), out0[~written].view(ft)), (n, prec, "r2c", ncols)
        g = got[SENT + oi].astype(np.complex128)
        assert np.all(np.isfinite(g.view(np.float64))), (n, prec, "r2c", ncols)
        assert not np.any(got[SENT + oi] == out0[SENT + oi]), "every one of them changed"
        err = np.linalg.norm(g - want) / np.linalg.norm(want)
        print("r2c", n, prec, ncols, err)
        assert err <= (1e-12 if prec == api.F64 else 1e-5), (n, prec, "r2c", ncols, err)
        # ---- real output: n/2+1 complex values in, the reals n < n/2 of a row out
        d = _bit4(real_desc(n, prec, ncols, nb1, "c2r", pad=pad, scale=scale))
        assert L.offt_hipk_kernel_name(C.byref(d)).decode() == C2R_K
        ii = _cidx(d.in_axis_stride, d.in_col_stride, d.in_b1_stride, nb1, ncols, K)
        ro = 2 * _cidx(0, d.out_col_stride, d.out_b1_stride, nb1, ncols, 1) + np.arange(n)[None, None, :]
        nin, nout = int(ii.max()) + 1 + pad, int(ro.max()) // 2 + 2 + pad
        X = (rng.standard_normal((nb1, ncols, K)) + 1j * rng.standard_normal((nb1, ncols, K))).astype(ct)
        xin = (rng.standard_normal(nin) + 1j * rng.standard_normal(nin)).astype(ct)
        xin[ii.ravel()] = X.ravel()
        want = np.fft.irfft(X.astype(np.complex128), n=n, axis=2)[:, :, :n // 2] * n * scale
        out0 = np.full(2 * (nout + 2 * SENT), 7.0, dtype=ft)   # a sentinel in the whole output: rows, padding, guards
        dx = torch.from_numpy(xin.view(ft).copy()).cuda()
        do = torch.from_numpy(out0.copy()).cuda()
        torch.cuda.synchronize()
        rc = L.offt_hipk_fft_pass(C.byref(d), dx.data_ptr(), do.data_ptr() + 2 * SENT * out0.itemsize, None)
        assert rc == 0, L.offt_hipk_last_error()
        torch.cuda.synchronize()
        got = do.cpu().numpy()
        written = np.zeros(out0.size, dtype=bool)
        written[2 * SENT + ro[:, :, :n // 2].ravel()] = True
        # the reals n >= n/2 of every row, the scalars behind the row, the padding and the guards still hold the sentinel
        assert np.array_equal(got[~written], out0[~written]), (n, prec, "c2r", ncols)
        g = got[2 * SENT + ro[:, :, :n // 2]].astype(np.float64)
        assert np.all(np.isfinite(g)), (n, prec, "c2r", ncols)
        err = np.linalg.norm(g - want) / np.linalg.norm(want)
        print("c2r", n, prec, ncols, err)
        assert err <= (1e-12 if prec == api.F64 else 1e-5), (n, prec, "c2r", ncols, err)
    # without the permission the same descriptors fail, they do not run the full line
    for form in ("r2c", "c2r"):
        d = real_desc(n, prec, 4, 1, form)
        buf = torch.zeros(2 * (4 * (n + 2) + 64), dtype=torch.float64, device="cuda")
        assert L.offt_hipk_fft_pass(C.byref(d), buf.data_ptr(), buf.data_ptr(), None) == -1
        assert b"half" in L.offt_hipk_last_error()


@pytest.mark.gpu
@pytest.mark.parametrize("case", [dict(N=[64, 96, 192], r2c=1), dict(N=[96, 64, 384], r2c=1), dict(N=[96, 192, 320], r2c=1),
                                  dict(N=[64, 64, 384], r2c=1, f32=1)], ids=lambda c: json.dumps(c))
def test_half_box_r2c_mixed_one_rank_gpu(built, case):
    import torch
    torch.cuda.set_device(0)
    L = api.lib()
    dev = HW.Gpu(torch)
    po = HW.make_plan(api, case)
    try:
        api.offt_hip_set_half_box(po, True)
        # pruned only with all three options
        for r in (0, 1, 2):
            for on in itertools.combinations(OPTS, r):
                _set(L, po, **{k: int(k in on) for k in OPTS})
                assert not api.offt_hip_half_box_pruned(po), (case, on)
        _set(L, po, OPT_HALF_R2C=1, OPT_HALF_MIXED=1, OPT_HALF_R2C_MIXED=1)
        assert api.offt_hip_half_box_pruned(po), case
        assert api.offt_hip_convolve_fused(po) == (case["N"][0] == 64)
        pr = HW.problem(case["N"], 1)
        res, out_on = HW.run_plan(api, po, case, dev, pr)
        for k, e in res.items():
            print(case, k, e)
        _check(res, case)
        if not case.get("f32"):
            # the same plan with the half box off on explicitly zeroed input.  The pruned passes differ from the ordinary ones
            # in the order of operations on exact zeros and, at 192 and 320 points, in the radix order: two roundings of the
            # same transform.  The bound is that of test_half_box_mixed_one_rank_gpu.
            api.offt_hip_set_half_box(po, False)
            c = api.comm_dict(po)
            data, _ = W.local_arrays(c, api.local_elems(po), case, pr["xp"], np.zeros((1, 1, 1)))
            h, p = dev.put(data)
            api.offt_3d_execute_dir(po, p, p, -1)
            out_off = dev.get(h, data)
            i = W.out_index(c)
            rel = np.linalg.norm(out_on[i] - out_off[i]) / np.linalg.norm(out_off[i])
            print(case, "pruned against the ordinary schedule", rel)
            assert rel <= 1e-14, rel
    finally:
        api.offt_3d_fin(po)


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [0, 1])
def test_half_box_r2c_mixed_free_space(built, fused):
    """test_half_box_mixed.py::test_half_box_mixed_free_space on a real plan: a delta at p in the 48^3 box, convolved on a real
    96^3 half-box plan (pruned) with the plan's own transform of the Gaussian that does not wrap: inside the box, g shifted by
    p with no periodic image (test_free_space_claim_at_48_on_the_cpu has the numpy side of the claim, on real data).  Once
    pruned forward, multiply, pruned inverse; once with OFFT_HIP_OPT_CONV_MIXED, the fused launch (96 has a fused kernel in
    double precision)."""
    import torch
    torch.cuda.set_device(0)
    g, p, want = _free_space_problem()
    N = (96, 96, 96)
    case = dict(N=list(N), r2c=1)
    po = HW.make_plan(api, case)
    L = api.lib()
    try:
        c = api.comm_dict(po)
        gbuf, _ = W.local_arrays(c, api.local_elems(po), case, g, np.zeros((1, 1, 1)))
        dh = torch.from_numpy(gbuf.view(np.float64).copy()).cuda()
        api.offt_3d_execute(po, dh.data_ptr(), dh.data_ptr())   # H = F(g): the full real-input transform, no half box
        _set(L, po, OPT_HALF_R2C=1, OPT_HALF_MIXED=1, OPT_HALF_R2C_MIXED=1, OPT_CONV_MIXED=fused)
        api.offt_hip_set_half_box(po, True)
        assert api.offt_hip_half_box_pruned(po) and api.offt_hip_convolve_fused(po) == fused
        delta = np.zeros(N)
        delta[p] = 1.0
        dbuf = HW.poisoned_input(c, api.local_elems(po), case, delta)
        dd = torch.from_numpy(dbuf.view(np.float64).copy()).cuda()
        L.offt_hip_set_output_scale(po, 1.0 / np.prod(N))
        api.offt_hip_execute_convolve(po, dd.data_ptr(), dh.data_ptr(), api.FILTER_COMPLEX)
        torch.cuda.synchronize()
        full = np.zeros(N)
        full[:48, :48, :48] = want
        err = HW.box_err(c, case, dd.cpu().numpy().view(np.complex128), full)
        print("free space, real plan, fused =", fused, err)
        assert err <= 1e-12, err
    finally:
        api.offt_3d_fin(po)
