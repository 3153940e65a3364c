"""Half-box plans at mixed-radix lengths: OFFT_HIP_OPT_HALF_MIXED (include/offt_hip.h) and the kernel under it,
fft_half_panelx_k (offt_pass_desc::half on the mixed-radix panel kernel).

  * routing without a device: the registered (length, precision) pairs in the four flavours of tests/test_half_box.py,
    and everything that has no kernel;
  * the host's route on the CPU pad backend (tests/cpu_backend_pad.c), the padding NaN: option off = the fallback of
    before, option on = the pruned schedule with half = 1, 2, the convolve unfused where x has no fused kernel;
  * the environment default in a fresh process;
  * -m gpu: the four flavours descriptor by descriptor (NaN in what must not be read, a sentinel in what must not be
    written), plans on one rank, a free-space convolution of a 48^3 box on a 96^3 plan."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _conv_world as W
import _half_world as HW
from offt_amd import api
from test_half_box import FLAVOURS, _check, _index, half_desc, kl, pad_cpu  # noqa: F401  (kl, pad_cpu: fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the registered half-line instances of the mixed-radix kernel (offt_reg_half_mixed_*.hip)
LENGTHS = {api.F64: (96, 192, 320, 384, 640, 768, 1000), api.F32: (384, 640, 768, 1000)}


# ---- routing without a device ---------------------------------------------------------------------------------------------
def test_half_mixed_kernel_routing_without_a_gpu(kl):
    L = kl
    name = lambda d: L.offt_hipk_kernel_name(C.byref(d)).decode()
    for prec, lengths in LENGTHS.items():
        for n in lengths:
            for ncols in (8, 7):   # (an even count with unit column stride too: there are no column-pair instances here)
                for inc, outc, half in FLAVOURS:
                    d = half_desc(n, prec, ncols, 2, inc, outc, half)
                    assert L.offt_hipk_has_half(C.byref(d)) == 1, (n, prec, inc, outc, half)
                    assert name(d) == "fft_half_panelx_k", (n, prec, inc, outc, half)
                    assert L.offt_hipk_keeps_output(C.byref(d)) == 0
            # the other bit on these flavours, both bits, and strided on both sides: no kernel
            for inc, outc, half in [(1, 0, 2), (0, 1, 1), (0, 0, 1), (0, 0, 2), (1, 1, 3), (1, 0, 3)]:
                d = half_desc(n, prec, 8, 2, inc, outc, half)
                assert L.offt_hipk_has_half(C.byref(d)) == 0 and name(d) == "no half-line kernel", (n, inc, outc, half)
            d = half_desc(n, prec, 8, 2, 1, 1, 1)
            d.in_split = n // 4                              # a split line
            assert L.offt_hipk_has_half(C.byref(d)) == 0
            d = half_desc(n, prec, 8, 2, 1, 1, 2)
            d.out_split = n // 4
            assert L.offt_hipk_has_half(C.byref(d)) == 0
            for inc, outc, half, real in [(1, 0, 1, 1), (0, 1, 2, 2), (1, 1, 1, 1), (1, 1, 2, 2)]:   # real rows: no kernel
                d = half_desc(n, prec, 8, 2, inc, outc, half)
                d.real_input = real
                assert L.offt_hipk_has_half(C.byref(d)) == 0 and name(d) == "no half-line kernel", (n, prec, real)
    # single precision has no mixed-radix instance below 384 points
    for n in (96, 192, 320):
        for inc, outc, half in FLAVOURS:
            d = half_desc(n, api.F32, 8, 2, inc, outc, half)
            assert L.offt_hipk_has_half(C.byref(d)) == 0 and name(d) == "no half-line kernel", n
    for prec in (api.F64, api.F32):
        d = half_desc(768, prec, 8, 2, 1, 1, 0)              # half = 0: the usual kernel, named as ever
        assert L.offt_hipk_has_half(C.byref(d)) == 0 and name(d) == "fft_panelx_k"
        for n in (250, 240, 48):                             # one factor of 2; swept, but not registered
            for inc, outc, half in FLAVOURS:
                d = half_desc(n, prec, 8, 2, inc, outc, half)
                assert L.offt_hipk_has_half(C.byref(d)) == 0 and name(d) == "no half-line kernel", (n, prec)


# ---- CPU tier: the host's route on the pad backend ------------------------------------------------------------------------
def _tables(shape):
    Nx, Ny, Nz = shape
    fwd = [(Nz, Ny // 2, Nx // 2, 1, 1, 0), (Ny, Nx // 2, Nz, 1, 1, 0), (Nx, Ny, Nz, 1, 1, 0)]
    inv = [(Nx, Ny, Nz, 1, 2, 0), (Ny, Nx // 2, Nz, 1, 2, 0), (Nz, Ny // 2, Nx // 2, 1, 2, 0)]
    conv = fwd[:2] + [(Nx, Ny, Nz, 1, 3, 1)] + inv[1:]
    return fwd, inv, conv


# (x = 96 and 320 have no fused convolve kernel; the third shape has x = 64, which has one)
@pytest.mark.parametrize("shape", [(96, 64, 192), (320, 96, 64), (64, 96, 192)])
def test_half_box_mixed_route_cpu(pad_cpu, shape):
    CB = pad_cpu
    L = api.lib()
    case = dict(N=list(shape))
    po = HW.make_plan(api, case)
    try:
        pr = HW.problem(case["N"], 0)
        # option off: what such a plan does today -- clear and the ordinary schedule
        assert L.offt_hip_get_option(po, api.OPT_HALF_MIXED) == 0, "off by default"
        api.offt_hip_set_half_box(po, True)
        assert not api.offt_hip_half_box_pruned(po)
        z0 = CB.cpu_backend_pad_zero_count()
        CB.cpu_backend_pad_log_reset()
        res, _ = HW.run_plan(api, po, case, HW.Host(), pr)
        _check(res, case)
        assert CB.cpu_backend_pad_zero_count() == z0 + 2, "the forward and the convolve clear the padding, the inverse does not"
        assert HW.launches(CB) and all(r[4] == 0 for r in HW.launches(CB)), "no half-line launch on the fallback route"
        # option on, on the live plan (its inverse schedule is cached by now): the pruned route
        assert L.offt_hip_set_option(po, api.OPT_HALF_MIXED, 1) == 0, L.offt_hip_last_error()
        assert L.offt_hip_get_option(po, api.OPT_HALF_MIXED) == 1
        assert api.offt_hip_half_box_pruned(po), "the half box was on: the option re-evaluates the route"
        z0 = CB.cpu_backend_pad_zero_count()
        p0 = CB.cpu_backend_pointwise_count()
        CB.cpu_backend_pad_log_reset()
        res, _ = HW.run_plan(api, po, case, HW.Host(), pr)
        _check(res, case)
        assert CB.cpu_backend_pad_zero_count() == z0, "a pruned plan clears nothing"
        fwd, inv, conv = _tables(shape)
        if shape[0] == 64:
            assert api.offt_hip_convolve_fused(po)
            assert HW.launches(CB) == fwd + inv + conv and CB.cpu_backend_pointwise_count() == p0
        else:   # pruned forward, one multiply, pruned inverse
            assert not api.offt_hip_convolve_fused(po)
            assert HW.launches(CB) == fwd + inv + fwd + inv and CB.cpu_backend_pointwise_count() == p0 + 1
        # off again on the live plan: back to the fallback
        assert L.offt_hip_set_option(po, api.OPT_HALF_MIXED, 0) == 0
        assert not api.offt_hip_half_box_pruned(po) and L.offt_hip_get_option(po, api.OPT_HALF_MIXED) == 0
        z0 = CB.cpu_backend_pad_zero_count()
        CB.cpu_backend_pad_log_reset()
        res, _ = HW.run_plan(api, po, case, HW.Host(), pr)
        _check(res, case)
        assert CB.cpu_backend_pad_zero_count() == z0 + 2 and all(r[4] == 0 for r in HW.launches(CB))
        # the option alone switches no half box on
        api.offt_hip_set_half_box(po, False)
        assert L.offt_hip_set_option(po, api.OPT_HALF_MIXED, 1) == 0 and not api.offt_hip_half_box_pruned(po)
    finally:
        api.offt_3d_fin(po)


def test_half_box_mixed_other_plans_cpu(pad_cpu):
    CB = pad_cpu
    L = api.lib()
    # a real-input plan with a mixed-radix length: no real-row kernel, whatever the two options say
    case = dict(N=[96, 64, 64], r2c=1)
    po = HW.make_plan(api, case)
    try:
        assert L.offt_hip_set_option(po, api.OPT_HALF_MIXED, 1) == 0 and L.offt_hip_set_option(po, api.OPT_HALF_R2C, 1) == 0
        api.offt_hip_set_half_box(po, True)
        assert not api.offt_hip_half_box_pruned(po)
        z0 = CB.cpu_backend_pad_zero_count()
        CB.cpu_backend_pad_log_reset()
        res, _ = HW.run_plan(api, po, case, HW.Host())
        _check(res, case)
        assert CB.cpu_backend_pad_zero_count() == z0 + 2 and all(r[4] == 0 for r in HW.launches(CB))
    finally:
        api.offt_3d_fin(po)
    # lengths without a half-line kernel stay on the fallback with the option on; a power-of-two plan does not care
    for N, want in (((48, 40, 30), 0), ((96, 64, 250), 0), ((64, 64, 64), 1)):
        po = HW.make_plan(api, dict(N=list(N)))
        try:
            for v in (1, 0):
                assert L.offt_hip_set_option(po, api.OPT_HALF_MIXED, v) == 0
                api.offt_hip_set_half_box(po, True)
                assert api.offt_hip_half_box_pruned(po) == want, (N, v)
        finally:
            api.offt_3d_fin(po)


_ENV_CHILD = """
import sys
sys.path[:0] = [%r, %r]
import cpu_world, _half_world as HW
from offt_amd import api
cpu_world._cb_lib = HW.pad_cb_lib
cpu_world.install(0, 1, p1=1)
po = HW.make_plan(api, dict(N=[96, 64, 64]))
v = api.lib().offt_hip_get_option(po, api.OPT_HALF_MIXED)
api.offt_hip_set_half_box(po, True)
print("RESULT", v, int(api.offt_hip_half_box_pruned(po)))
api.offt_3d_fin(po)
"""


def test_half_box_mixed_environment_default(built):
    """OFFT_HALF_MIXED is read once, by offt_3d_init, as the option's default"""
    subprocess.check_call(["make", "-s", "-C", ROOT, "tests/libcpubackend_pad.so"])
    for val, want in ((None, "RESULT 0 0"), ("1", "RESULT 1 1"), ("0", "RESULT 0 0")):
        env = {k: v for k, v in os.environ.items() if k != "OFFT_HALF_MIXED"}
        if val is not None:
            env["OFFT_HALF_MIXED"] = val
        p = subprocess.run([sys.executable, "-c", _ENV_CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=300)
        out = p.stdout.decode()
        assert p.returncode == 0 and want in out.splitlines(), (val, out[-2000:])


def _free_space_problem():
    """the problem of test_half_box._free_space_problem one size up: a 48^3 box on a 96^3 grid.  g: a Gaussian of width
    sigma = 3 centred at (8,8,8) and cut to exactly zero beyond 8 cells from its centre along any axis, so its support
    [0,16]^3 and every shift of it by p < 48 stay on the 96-grid: nothing wraps.  A delta at p = (36, 3, 17) puts the peak at
    p + 8 = (44, 11, 25); on a periodic 48^3 grid the cells x = 48 ... 52 of the shifted kernel come back at x = 0 ... 4, the
    first of them 4 cells from the peak, exp(-16/18) = 0.41 of it."""
    n = 96
    ax = np.arange(n) - 8.0
    cut = np.abs(ax) > 8
    g = np.exp(-(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2) / 18.0)
    g[cut[:, None, None] | cut[None, :, None] | cut[None, None, :]] = 0.0
    p = (36, 3, 17)
    want = np.roll(g, p, axis=(0, 1, 2))[:48, :48, :48].copy()   # (index k of g moves to k + p <= 16 + 47: no wrap on the 96-grid)
    return g, p, want


def test_free_space_claim_at_48_on_the_cpu():
    """the claim test_half_box_mixed_free_space rests on: the periodic convolution on the 48^3 grid differs from the
    free-space one by far more than 1e-3, and the zero-padded 96^3 one does not differ"""
    g, p, want = _free_space_problem()
    n = 48
    d = np.zeros((n, n, n))
    d[p] = 1.0
    per = np.fft.ifftn(np.fft.fftn(d) * np.fft.fftn(g[:n, :n, :n])).real   # (g's support lies inside [0,48)^3)
    assert np.linalg.norm(per - want) / np.linalg.norm(want) > 1e-3
    d2 = np.zeros((96, 96, 96))
    d2[p] = 1.0
    free = np.fft.ifftn(np.fft.fftn(d2) * np.fft.fftn(g)).real[:n, :n, :n]
    assert np.linalg.norm(free - want) / np.linalg.norm(want) <= 1e-12


# ---- GPU tier ----------------------------------------------------------------------------------------------------------
# 96: the smallest; 192: another radix order than its full-line kernel; 320: a predicated first butterfly (40 butterflies on
# 16 threads); 1000 f64: a narrow contiguous / contiguous shape beside the wide one; 384 f32: the smallest single-precision
# instance; 1000 f32: predicated first and last butterflies (50 and 100 on 40 threads)
@pytest.mark.gpu
@pytest.mark.parametrize("prec,n", [(api.F64, 96), (api.F64, 192), (api.F64, 320), (api.F64, 1000), (api.F32, 384), (api.F32, 1000)])
def test_half_mixed_random_descriptors(kl, prec, n):
    import torch
    L = kl
    rng = np.random.default_rng(4100 + n + 7 * prec)
    SENT = 8
    assert L.offt_hipk_prepare(n, prec) == 0, L.offt_hipk_last_error()
    ft, ct = (np.float64, np.complex128) if prec == api.F64 else (np.float32, np.complex64)
    for inc, outc, half in FLAVOURS:
        for ncols in (3, 13, 21, 18):
            nb1 = int(rng.integers(2, 4))
            pad = int(rng.integers(1, 3))
            direction = int(rng.choice([-1, 1]))
            scale = float(rng.choice([0.5, 1.0 / n, 3.0]))
            d = half_desc(n, prec, ncols, nb1, inc, outc, half, pad=pad, direction=direction, scale=scale)
            assert L.offt_hipk_kernel_name(C.byref(d)).decode() == "fft_half_panelx_k"
            ii, oi = _index(d, "in", nb1, ncols, n), _index(d, "out", nb1, ncols, n)
            nin, nout = int(ii.max()) + 1 + pad, int(oi.max()) + 1 + pad
            lines = (rng.standard_normal((nb1, ncols, n)) + 1j * rng.standard_normal((nb1, ncols, n))).astype(ct)
            x = (rng.standard_normal(nin) + 1j * rng.standard_normal(nin)).astype(ct)
            x[ii.ravel()] = lines.ravel()
            if half & 1:    # what must not be read is NaN, and counts as zero
                x[ii[:, :, n // 2:].ravel()] = np.nan + 1j * np.nan
                lines[:, :, n // 2:] = 0
            l128 = lines.astype(np.complex128)
            want = (np.fft.fft(l128, axis=2) if direction < 0 else np.fft.ifft(l128, axis=2) * n) * scale
            out0 = np.full(nout + 2 * SENT, 7.0 + 7.0j, dtype=ct)
            out0[SENT:SENT + nout] = (rng.standard_normal(nout) + 1j * rng.standard_normal(nout)).astype(ct)
            dx = torch.from_numpy(x.view(ft).copy()).cuda()
            do = torch.from_numpy(out0.view(ft).copy()).cuda()
            torch.cuda.synchronize()
            rc = L.offt_hipk_fft_pass(C.byref(d), dx.data_ptr(), do.data_ptr() + SENT * out0.itemsize, None)
            assert rc == 0, L.offt_hipk_last_error()
            torch.cuda.synchronize()
            got = do.cpu().numpy().view(ct)
            kept = n // 2 if half & 2 else n
            written = np.zeros(nout + 2 * SENT, dtype=bool)
            written[SENT + oi[:, :, :kept].ravel()] = True
            # guard elements, the padding between lines and (bit 2) the upper half of every line: bit-identical
            assert np.array_equal(got[~written].view(ft), out0[~written].view(ft)), (n, prec, inc, outc, half, ncols)
            g = got[SENT + oi[:, :, :kept]].astype(np.complex128)
            assert np.all(np.isfinite(g.view(np.float64))), (n, prec, inc, outc, half, ncols)
            err = np.linalg.norm(g - want[:, :, :kept]) / np.linalg.norm(want[:, :, :kept])
            print(n, prec, (inc, outc, half), ncols, err)
            assert err <= (1e-12 if prec == api.F64 else 1e-5), (n, prec, inc, outc, half, ncols, err)
    # a flavour no kernel implements fails, it does not run the full line
    d = half_desc(n, prec, 4, 1, 0, 0, 1)
    buf = torch.zeros(2 * (4 * n + 64), dtype=torch.float64, device="cuda")
    assert L.offt_hipk_fft_pass(C.byref(d), buf.data_ptr(), buf.data_ptr(), None) == -1
    assert b"half" in L.offt_hipk_last_error()


@pytest.mark.gpu
@pytest.mark.parametrize("case", [dict(N=[96, 192, 384]), dict(N=[384, 96, 64]), dict(N=[384, 64, 640], f32=1)], ids=lambda c: json.dumps(c))
def test_half_box_mixed_one_rank_gpu(built, case):
    import torch
    torch.cuda.set_device(0)
    L = api.lib()
    dev = HW.Gpu(torch)
    po = HW.make_plan(api, case)
    try:
        api.offt_hip_set_half_box(po, True)
        assert not api.offt_hip_half_box_pruned(po), "the option is off by default"
        assert L.offt_hip_set_option(po, api.OPT_HALF_MIXED, 1) == 0, L.offt_hip_last_error()
        assert api.offt_hip_half_box_pruned(po), case
        assert api.offt_hip_convolve_fused(po) == (case["N"][0] == 64)
        pr = HW.problem(case["N"], 0)
        res, out_on = HW.run_plan(api, po, case, dev, pr)
        for k, e in res.items():
            print(case, k, e)
        _check(res, case)
        if not case.get("f32"):
            # the same plan with the half box off on explicitly zeroed input.  The pruned passes differ from the ordinary ones
            # in the order of operations on exact zeros and, at 192 points, in the radix order (8 x 3 x 8 against 8 x 8 x 3):
            # two roundings of the same transform.  The bound is that of test_half_box_one_rank_gpu.
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
def test_half_box_mixed_free_space(built):
    """a delta at p in the 48^3 box, convolved on a 96^3 half-box plan with the plan's own transform of a Gaussian that does
    not wrap: inside the box, g shifted by p with no periodic image (test_free_space_claim_at_48_on_the_cpu checks with numpy
    that the periodic 48^3 route differs by > 1e-3).  96 points have no fused convolve kernel: pruned forward, multiply,
    pruned inverse."""
    import torch
    torch.cuda.set_device(0)
    g, p, want = _free_space_problem()
    N = (96, 96, 96)
    po = api.offt_3d_init(*N)
    L = api.lib()
    try:
        c = api.comm_dict(po)
        case = dict(N=list(N))
        gbuf, _ = W.local_arrays(c, api.local_elems(po), case, g.astype(np.complex128), np.zeros((1, 1, 1)))
        dh = torch.from_numpy(gbuf.view(np.float64).copy()).cuda()
        api.offt_3d_execute(po, dh.data_ptr(), dh.data_ptr())   # H = F(g): the full transform, half box off
        assert L.offt_hip_set_option(po, api.OPT_HALF_MIXED, 1) == 0, L.offt_hip_last_error()
        api.offt_hip_set_half_box(po, True)
        assert api.offt_hip_half_box_pruned(po) and not api.offt_hip_convolve_fused(po)
        delta = np.zeros(N)
        delta[p] = 1.0
        dbuf = HW.poisoned_input(c, api.local_elems(po), case, delta.astype(np.complex128))
        dd = torch.from_numpy(dbuf.view(np.float64).copy()).cuda()
        L.offt_hip_set_output_scale(po, 1.0 / np.prod(N))
        api.offt_hip_execute_convolve(po, dd.data_ptr(), dh.data_ptr(), api.FILTER_COMPLEX)
        torch.cuda.synchronize()
        full = np.zeros(N)
        full[:48, :48, :48] = want
        err = HW.box_err(c, case, dd.cpu().numpy().view(np.complex128), full.astype(np.complex128))
        print("free space", err)
        assert err <= 1e-12, err
    finally:
        api.offt_3d_fin(po)
