"""Real-input half-box plans that skip the padding: OFFT_HIP_OPT_HALF_R2C (include/offt_hip.h) and the two kernels under it,
fft_half_r2c_panel_k (real_input = 1 with half = 1) and fft_half_c2r_panel_k (real_input = 2 with half = 2).

  * routing without a device: the two new forms have a kernel for 64 ... 1024 points, every other real form has none;
  * the host's schedules on the CPU backend of tests/cpu_backend_padreal.c, the padding NaN every time: option off (what
    every real-input half-box plan did before the option), option on (pruned, no clear, the launch table of the schedule),
    plans that still fall back, the unfused convolve, the option switched on and off on a live plan;
  * -m gpu: the two kernels descriptor by descriptor (NaN in what must not be read, a sentinel in what must not be
    written), plans on one rank, a free-space convolution on a real plan."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import _conv_world as W
import _half_world as HW
from offt_amd import api
from test_half_box import Desc, _check, _free_space_problem, kl  # noqa: F401  (kl: the fixture that binds the kernel ABI)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [64, 128, 256, 512, 1024]


def real_desc(n, prec, ncols, nb1, form, pad=0, scale=1.0):
    """form "r2c": rows of n reals in (row pitch n/2+1+pad complex slots), n/2+1 strided complex values out;
    form "c2r": the mirror image.  The strided side leaves room for exactly n/2+1 axis indices per batch entry."""
    d = Desc()
    d.n, d.precision, d.ncols, d.nb1, d.nb2, d.variant, d.scale = n, prec, ncols, nb1, 1, -1, scale
    rp = n // 2 + 1 + pad
    rows = (1, rp, rp * ncols + pad)
    cols = (ncols + pad, 1, (ncols + pad) * (n // 2 + 1) + pad)
    if form == "r2c":
        d.real_input, d.half, d.direction, d.in_contig, d.out_contig = 1, 1, -1, 1, 0
        (d.in_axis_stride, d.in_col_stride, d.in_b1_stride), (d.out_axis_stride, d.out_col_stride, d.out_b1_stride) = rows, cols
    else:
        d.real_input, d.half, d.direction, d.in_contig, d.out_contig = 2, 2, +1, 0, 1
        (d.in_axis_stride, d.in_col_stride, d.in_b1_stride), (d.out_axis_stride, d.out_col_stride, d.out_b1_stride) = cols, rows
    return d


# ---- routing without a device ---------------------------------------------------------------------------------------------
def test_real_half_kernel_routing_without_a_gpu(kl):
    L = kl
    has = lambda d: L.offt_hipk_has_half(C.byref(d))
    name = lambda d: L.offt_hipk_kernel_name(C.byref(d)).decode()
    for prec in (api.F64, api.F32):
        for n in LENGTHS:
            for ncols in (8, 7):
                d = real_desc(n, prec, ncols, 2, "r2c")
                assert has(d) == 1 and name(d) == "fft_half_r2c_panel_k", (n, prec, ncols)
                assert L.offt_hipk_keeps_output(C.byref(d)) == 0
                d = real_desc(n, prec, ncols, 2, "c2r")
                assert has(d) == 1 and name(d) == "fft_half_c2r_panel_k", (n, prec, ncols)
            # a split or four-step twiddles on the new forms: no kernel
            for form in ("r2c", "c2r"):
                for field in ("in_split", "out_split", "in_split_nfloor", "out_split_nfloor"):
                    d = real_desc(n, prec, 8, 2, form)
                    setattr(d, field, 16)
                    assert has(d) == 0 and name(d) == "no half-line kernel", (n, form, field)
                d = real_desc(n, prec, 8, 2, form)
                d.tw4 = 64   # (any non-NULL value: a lookup never follows it)
                assert has(d) == 0, (n, form)
            # the other bit, both bits, the other real kind, the other flavours: no kernel
            for form, ri, half, inc, outc in [("r2c", 1, 2, 1, 0), ("r2c", 1, 3, 1, 0), ("r2c", 2, 1, 1, 0), ("r2c", 1, 1, 1, 1), ("r2c", 1, 1, 0, 1),
                                              ("r2c", 1, 1, 0, 0), ("c2r", 2, 1, 0, 1), ("c2r", 2, 3, 0, 1), ("c2r", 1, 2, 0, 1), ("c2r", 2, 2, 1, 1),
                                              ("c2r", 2, 2, 1, 0), ("c2r", 2, 2, 0, 0)]:
                d = real_desc(n, prec, 8, 2, form)
                d.real_input, d.half, d.in_contig, d.out_contig = ri, half, inc, outc
                assert has(d) == 0 and name(d) == "no half-line kernel", (n, ri, half, inc, outc)
            d = real_desc(n, prec, 8, 2, "r2c")
            d.direction = +1   # a real-input pass is a forward pass (as on full lines)
            assert has(d) == 0
        for n in (32, 2048, 48):
            for form in ("r2c", "c2r"):
                d = real_desc(n, prec, 8, 2, form)
                assert has(d) == 0 and name(d) == "no half-line kernel", (n, prec, form)


# ---- CPU tier: the host's schedules on the padreal backend ---------------------------------------------------------------
def padreal_cb_lib():
    """tests/libcpubackend_padreal.so, shaped like cpu_world's backend library (its table = the padreal table)"""
    L = C.CDLL(os.path.join(ROOT, "tests", "libcpubackend_padreal.so"))
    for f in ("cpu_backend_padreal_table", "cpu_backend_padreal_table_unfused"):
        getattr(L, f).restype = C.c_void_p
    L.cpu_backend_table = L.cpu_backend_padreal_table
    for f in ("cpu_backend_pass_count", "cpu_backend_pad_zero_count", "cpu_backend_pointwise_count", "cpu_backend_padreal_real_half_count"):
        getattr(L, f).restype = C.c_long
    L.cpu_backend_padreal_log.argtypes = [C.c_int, C.POINTER(C.c_int)]
    return L


def launches(CB):
    """the launches recorded since the last reset: (n, ncols, nb1, nb2, half, conv, real_input)"""
    out, rec, i = [], (C.c_int * 7)(), 0
    while CB.cpu_backend_padreal_log(i, rec) == 0:
        out.append(tuple(rec))
        i += 1
    return out


@pytest.fixture()
def padreal_cpu(built):
    import cpu_world
    subprocess.check_call(["make", "-s", "-C", ROOT, "tests/libcpubackend_padreal.so"])
    orig = cpu_world._cb_lib
    cpu_world._cb_lib = padreal_cb_lib
    CB = cpu_world.install(0, 1, p1=1)
    yield CB
    cpu_world.uninstall()
    cpu_world._cb_lib = orig


SHAPES = [(64, 64, 64), (128, 64, 256)]


def table(shape):
    """the launches of a pruned real-input plan (the schedule table of offt_host.c): forward, inverse, fused convolve"""
    Nx, Ny, Nz = shape
    K = Nz // 2 + 1
    fwd = [(Nz, Ny // 2, Nx // 2, 1, 1, 0, 1), (Ny, Nx // 2, K, 1, 1, 0, 0), (Nx, Ny, K, 1, 1, 0, 0)]
    inv = [(Nx, Ny, K, 1, 2, 0, 0), (Ny, Nx // 2, K, 1, 2, 0, 0), (Nz, Ny // 2, Nx // 2, 1, 2, 0, 2)]
    conv = fwd[:2] + [(Nx, Ny, K, 1, 3, 1, 0)] + inv[1:]
    return fwd, inv, conv


@pytest.mark.parametrize("shape", SHAPES)
def test_half_box_r2c_option_off_cpu(padreal_cpu, shape):
    """what a real-input half-box plan does without the option, and did before it existed"""
    CB = padreal_cpu
    case = dict(N=list(shape), r2c=1)
    po = HW.make_plan(api, case)
    try:
        api.offt_hip_set_half_box(po, True)
        assert not api.offt_hip_half_box_pruned(po)
        z0 = CB.cpu_backend_pad_zero_count()
        CB.cpu_backend_padreal_log_reset()
        res, _ = HW.run_plan(api, po, case, HW.Host())
        _check(res, case)
        assert CB.cpu_backend_pad_zero_count() == z0 + 2, "the forward and the convolve clear the padding, the inverse does not"
        assert launches(CB) and all(r[4] == 0 for r in launches(CB)), "no half-line launch on the fallback route"
    finally:
        api.offt_3d_fin(po)


@pytest.mark.parametrize("shape", SHAPES)
def test_half_box_r2c_pruned_cpu(padreal_cpu, shape):
    CB = padreal_cpu
    L = api.lib()
    case = dict(N=list(shape), r2c=1)
    po = HW.make_plan(api, case)
    try:
        assert L.offt_hip_get_option(po, api.OPT_HALF_R2C) == 0, "off by default"
        assert L.offt_hip_set_option(po, api.OPT_HALF_R2C, 1) == 0, L.offt_hip_last_error()
        assert L.offt_hip_get_option(po, api.OPT_HALF_R2C) == 1
        assert not api.offt_hip_half_box_pruned(po), "the option alone switches no half box on"
        api.offt_hip_set_half_box(po, True)
        assert api.offt_hip_half_box_pruned(po)
        z0 = CB.cpu_backend_pad_zero_count()
        pr = HW.problem(case["N"], 1)
        CB.cpu_backend_padreal_log_reset()
        res, _ = HW.run_plan(api, po, case, HW.Host(), pr)
        _check(res, case)
        assert CB.cpu_backend_pad_zero_count() == z0, "a pruned plan clears nothing"
        fwd, inv, conv = table(shape)
        assert api.offt_hip_convolve_fused(po)
        assert launches(CB) == fwd + inv + conv
        # a backend without the fused launch: the pruned forward, one multiply, the pruned inverse
        L.offt_hip_test_set_backend(CB.cpu_backend_padreal_table_unfused(), 0, 1)
        assert not api.offt_hip_convolve_fused(po)
        CB.cpu_backend_padreal_log_reset()
        p0 = CB.cpu_backend_pointwise_count()
        res, _ = HW.run_plan(api, po, case, HW.Host(), pr)
        _check(res, case)
        assert launches(CB) == fwd + inv + fwd + inv and CB.cpu_backend_pointwise_count() == p0 + 1
        assert CB.cpu_backend_pad_zero_count() == z0
        L.offt_hip_test_set_backend(CB.cpu_backend_padreal_table(), 0, 1)
    finally:
        api.offt_3d_fin(po)


@pytest.mark.parametrize("case", [dict(N=[12, 10, 8], r2c=1), dict(N=[64, 64, 64], r2c=1, params={"S": 1})], ids=lambda c: json.dumps(c))
def test_half_box_r2c_still_falls_back_cpu(padreal_cpu, case):
    """the option on, but no half-line kernel for these lengths / another layout: clear and the ordinary schedule"""
    CB = padreal_cpu
    L = api.lib()
    po = HW.make_plan(api, case)
    try:
        assert L.offt_hip_set_option(po, api.OPT_HALF_R2C, 1) == 0, L.offt_hip_last_error()
        api.offt_hip_set_half_box(po, True)
        assert not api.offt_hip_half_box_pruned(po)
        z0 = CB.cpu_backend_pad_zero_count()
        CB.cpu_backend_padreal_log_reset()
        res, _ = HW.run_plan(api, po, case, HW.Host())
        _check(res, case)
        assert CB.cpu_backend_pad_zero_count() == z0 + 2
        assert launches(CB) and all(r[4] == 0 for r in launches(CB))
    finally:
        api.offt_3d_fin(po)


def test_half_box_r2c_option_flips_a_live_plan_cpu(padreal_cpu, monkeypatch):
    CB = padreal_cpu
    L = api.lib()
    case = dict(N=[64, 64, 64], r2c=1)
    po = HW.make_plan(api, case)
    try:
        api.offt_hip_set_half_box(po, True)
        assert not api.offt_hip_half_box_pruned(po)
        pr = HW.problem(case["N"], 1)
        buf = np.zeros(api.local_elems(po), dtype=np.complex128)
        c = api.comm_dict(po)
        buf[W.out_index(c)] = HW.out_block(c, pr["Y"])
        api.offt_3d_execute_dir(po, buf.ctypes.data, buf.ctypes.data, +1)       # (the inverse schedule is cached now)
        assert L.offt_hip_set_option(po, api.OPT_HALF_R2C, 1) == 0, L.offt_hip_last_error()
        assert api.offt_hip_half_box_pruned(po), "the half box was on: the option re-evaluates the route"
        CB.cpu_backend_padreal_log_reset()
        buf[:] = 0
        buf[W.out_index(c)] = HW.out_block(c, pr["Y"])
        api.offt_3d_execute_dir(po, buf.ctypes.data, buf.ctypes.data, +1)
        assert launches(CB) == table((64, 64, 64))[1], "and no inverse schedule of the other route is replayed"
        assert HW.box_err(c, case, buf, pr["inv"]) <= HW.tol(case)
        assert L.offt_hip_set_option(po, api.OPT_HALF_R2C, 0) == 0
        assert not api.offt_hip_half_box_pruned(po) and L.offt_hip_get_option(po, api.OPT_HALF_R2C) == 0
        z0 = CB.cpu_backend_pad_zero_count()
        CB.cpu_backend_padreal_log_reset()
        res, _ = HW.run_plan(api, po, case, HW.Host(), pr)
        _check(res, case)
        assert CB.cpu_backend_pad_zero_count() == z0 + 2 and all(r[4] == 0 for r in launches(CB))
        # a complex plan does not care
        api.offt_hip_set_half_box(po, False)
        assert L.offt_hip_set_option(po, api.OPT_HALF_R2C, 1) == 0 and not api.offt_hip_half_box_pruned(po)
    finally:
        api.offt_3d_fin(po)
    po = HW.make_plan(api, dict(N=[64, 64, 64]))
    try:
        api.offt_hip_set_half_box(po, True)
        assert api.offt_hip_half_box_pruned(po)
        assert L.offt_hip_set_option(po, api.OPT_HALF_R2C, 0) == 0 and api.offt_hip_half_box_pruned(po)
    finally:
        api.offt_3d_fin(po)
    # the environment variable is the default of a new plan
    monkeypatch.setenv("OFFT_HALF_R2C", "1")
    po = HW.make_plan(api, case)
    try:
        assert L.offt_hip_get_option(po, api.OPT_HALF_R2C) == 1
        api.offt_hip_set_half_box(po, True)
        assert api.offt_hip_half_box_pruned(po)
    finally:
        api.offt_3d_fin(po)


# ---- GPU tier ----------------------------------------------------------------------------------------------------------
def _cidx(ax, col, b1, nb1, ncols, n):
    return np.arange(nb1)[:, None, None] * b1 + np.arange(ncols)[None, :, None] * col + np.arange(n)[None, None, :] * ax


@pytest.mark.gpu
@pytest.mark.parametrize("n", LENGTHS)
def test_real_half_random_descriptors(kl, n):
    """tolerances: those of test_half_box.py::test_half_random_descriptors, 1e-12 / 1e-5 rel-L2"""
    import torch
    L = kl
    rng = np.random.default_rng(4100 + n)
    SENT = 8   # guard, in complex elements
    K = n // 2 + 1
    for prec in (api.F64, api.F32):
        assert L.offt_hipk_prepare(n, prec) == 0
        ft, ct = (np.float64, np.complex128) if prec == api.F64 else (np.float32, np.complex64)
        for ncols in (3, 13, 21):   # no multiple of the 8 or 16 columns of a panel
            nb1 = int(rng.integers(2, 4))
            pad = int(rng.integers(1, 3))
            scale = float(rng.choice([0.5, 1.0 / n, 3.0]))
            # ---- real input: n/2 reals of a row in, n/2+1 complex values out
            d = real_desc(n, prec, ncols, nb1, "r2c", pad=pad, scale=scale)
            assert L.offt_hipk_kernel_name(C.byref(d)).decode() == "fft_half_r2c_panel_k"
            ri = 2 * _cidx(0, d.in_col_stride, d.in_b1_stride, nb1, ncols, 1) + np.arange(n)[None, None, :]   # scalar index of real k of a row
            oi = _cidx(d.out_axis_stride, d.out_col_stride, d.out_b1_stride, nb1, ncols, K)
            nin, nout = int(ri.max()) // 2 + 2 + pad, int(oi.max()) + 1 + pad
            rows = rng.standard_normal((nb1, ncols, n)).astype(ft)
            rows[:, :, n // 2:] = 0
            x = rng.standard_normal(2 * nin).astype(ft)
            x[ri.ravel()] = rows.ravel()
            x[ri[:, :, n // 2:].ravel()] = np.nan           # what must not be read is NaN, and counts as zero
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
            d = real_desc(n, prec, ncols, nb1, "c2r", pad=pad, scale=scale)
            assert L.offt_hipk_kernel_name(C.byref(d)).decode() == "fft_half_c2r_panel_k"
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
            # every scalar from n/2 on of every row, the padding and the guards still hold the sentinel
            assert np.array_equal(got[~written], out0[~written]), (n, prec, "c2r", ncols)
            g = got[2 * SENT + ro[:, :, :n // 2]].astype(np.float64)
            assert np.all(np.isfinite(g)), (n, prec, "c2r", ncols)
            err = np.linalg.norm(g - want) / np.linalg.norm(want)
            print("c2r", n, prec, ncols, err)
            assert err <= (1e-12 if prec == api.F64 else 1e-5), (n, prec, "c2r", ncols, err)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("f32", [0, 1])
def test_half_box_r2c_one_rank_gpu(built, shape, f32):
    import torch
    torch.cuda.set_device(0)
    L = api.lib()
    case = dict(N=list(shape), r2c=1, f32=f32)
    dev = HW.Gpu(torch)
    po = HW.make_plan(api, case)
    try:
        assert L.offt_hip_set_option(po, api.OPT_HALF_R2C, 1) == 0, L.offt_hip_last_error()
        api.offt_hip_set_half_box(po, True)
        assert api.offt_hip_half_box_pruned(po) and api.offt_hip_convolve_fused(po)
        pr = HW.problem(case["N"], 1)
        res, out_on = HW.run_plan(api, po, case, dev, pr)
        for k, e in res.items():
            print(case, k, e)
        _check(res, case)
        if not f32:
            # the same plan with the option and the half box off, on explicitly zeroed input: only operations on exact zeros
            # differ (the bound and the reasoning of test_half_box.py::test_half_box_one_rank_gpu)
            assert L.offt_hip_set_option(po, api.OPT_HALF_R2C, 0) == 0
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
def test_half_box_r2c_free_space(built):
    """test_half_box.py::test_half_box_free_space on a real plan: a delta at p in the 32^3 box, convolved on a 64^3 real-input
    half-box plan (pruned) with the plan's own transform of the Gaussian that does not wrap: inside the box, g shifted by p
    with no periodic image (test_free_space_claim_on_the_cpu has the numpy side of the claim)."""
    import torch
    torch.cuda.set_device(0)
    g, p, want = _free_space_problem()
    N = (64, 64, 64)
    case = dict(N=list(N), r2c=1)
    po = HW.make_plan(api, case)
    L = api.lib()
    try:
        c = api.comm_dict(po)
        gbuf, _ = W.local_arrays(c, api.local_elems(po), case, g, np.zeros((1, 1, 1)))
        dh = torch.from_numpy(gbuf.view(np.float64).copy()).cuda()
        api.offt_3d_execute(po, dh.data_ptr(), dh.data_ptr())   # H = F(g): the full real-input transform, no half box
        assert L.offt_hip_set_option(po, api.OPT_HALF_R2C, 1) == 0, L.offt_hip_last_error()
        api.offt_hip_set_half_box(po, True)
        assert api.offt_hip_half_box_pruned(po) and api.offt_hip_convolve_fused(po)
        delta = np.zeros(N)
        delta[p] = 1.0
        dbuf = HW.poisoned_input(c, api.local_elems(po), case, delta)
        dd = torch.from_numpy(dbuf.view(np.float64).copy()).cuda()
        L.offt_hip_set_output_scale(po, 1.0 / np.prod(N))
        api.offt_hip_execute_convolve(po, dd.data_ptr(), dh.data_ptr(), api.FILTER_COMPLEX)
        torch.cuda.synchronize()
        full = np.zeros(N)
        full[:32, :32, :32] = want
        err = HW.box_err(c, case, dd.cpu().numpy().view(np.complex128), full)
        print("free space, real plan", err)
        assert err <= 1e-12, err
    finally:
        api.offt_3d_fin(po)
