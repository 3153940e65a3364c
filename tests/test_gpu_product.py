"""Pseudo-spectral product on the device (-m gpu): the fused launch on random strided descriptors, whole plans on both routes,
the multiply sweep alone, caller-owned streams and async mode, repeatability, refusals of host memory.

The reference is numpy in complex128 (float64 fields for r2c plans).  Tolerances are the project's own, rel-L2 against the norm
of the reference: 1e-12 / 1e-5 at descriptor level, W.tol (1e-12 / 2e-5) at plan level; the single-precision bounds were checked
against torch.fft in complex64 on the same inputs (tests/test_product.py: 2.2e-7 ... 2.7e-7)."""
import ctypes as C

import numpy as np
import pytest

import _conv_world as W
import _half_world as HW
import _prod_world as PW
from offt_amd import api
from test_convolve_multi import Desc
from test_product import prod_desc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(built):
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    L = api.lib()
    L.offt_hipk_prod_pass.argtypes = [C.POINTER(Desc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.offt_hipk_pointwise_prod.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_int] * 3 + [C.c_longlong] * 3 + [C.c_void_p]
    L.offt_hipk_prepare.argtypes = [C.c_int, C.c_int]
    L.offt_hipk_last_error.restype = C.c_char_p
    return L, torch, HW.Gpu(torch)


SENT = 7.25 - 3.5j


def _lines(d, buf):
    """the lines of a product descriptor as an array [nb1][ncols][n] of indices into buf"""
    b1, c, k = np.arange(d.nb1)[:, None, None], np.arange(d.ncols)[None, :, None], np.arange(d.n)[None, None, :]
    return b1 * d.in_b1_stride + c * d.in_col_stride + k * d.in_axis_stride


@pytest.mark.parametrize("prec", [api.F64, api.F32])
@pytest.mark.parametrize("n", [64, 128, 256, 512, 1024])
def test_prod_pass_descriptors(gpu, n, prec):
    L, torch, dev = gpu
    ct = np.complex128 if prec == api.F64 else np.complex64
    assert L.offt_hipk_prepare(n, prec) == 0
    rng = np.random.default_rng(n + prec)
    for ncols in (8, 12, 5):                      # a full column group, a ragged one, fewer columns than a panel
        d = prod_desc(n, prec, ncols, 3, pitch=ncols + 3, plane_pad=5)
        d.scale = 0.5
        idx = _lines(d, None)
        size = 3 * d.in_b1_stride
        assert idx.max() < size
        owned = np.zeros(size, dtype=bool)
        owned[idx.ravel()] = True
        srcs = []
        for _ in range(2):
            s = np.full(size, SENT, dtype=ct)
            s[idx.ravel()] = ((rng.standard_normal(idx.shape) + 1j * rng.standard_normal(idx.shape)) / n).astype(ct).ravel()
            srcs.append(s)
        la, lb = srcs[0][idx].astype(np.complex128), srcs[1][idx].astype(np.complex128)
        ia, ib = np.fft.ifft(la, axis=2) * n, np.fft.ifft(lb, axis=2) * n
        for two, inplace in ((True, False), (True, True), (False, False), (False, True)):
            want = np.fft.fft(ia * (ib if two else ia), axis=2) * 0.5
            h0, h1 = dev.put(srcs[0]), dev.put(srcs[1])
            ho = h0 if inplace else dev.put(np.full(size, SENT, dtype=ct))
            assert L.offt_hipk_prod_pass(C.byref(d), h0[1], h1[1] if two else None, ho[1], None) == 0, L.offt_hipk_last_error()
            got = dev.get(ho[0], srcs[0])
            err = np.linalg.norm(got[idx].astype(np.complex128) - want) / np.linalg.norm(want)
            assert err <= (1e-12 if prec == api.F64 else 1e-5), (n, prec, ncols, two, inplace, err)
            assert np.all(got[~owned] == ct(SENT)), (n, prec, ncols, "an element no line owns was written")
            if not inplace:                       # a source that is not dst is not written
                assert np.array_equal(dev.get(h0[0], srcs[0]), srcs[0])
            assert np.array_equal(dev.get(h1[0], srcs[1]), srcs[1])


def _plan(case, opt):
    po = HW.make_plan(api, case)
    assert api.lib().offt_hip_set_option(po, api.OPT_PROD_FUSED, opt) == 0
    return po


@pytest.mark.parametrize("f32", [0, 1])
@pytest.mark.parametrize("shape", [(10, 12, 64), (6, 8, 128), (4, 24, 1024), (13, 5, 512)])
def test_prod_plans_fused(gpu, shape, f32):
    L, torch, dev = gpu
    case = dict(N=list(shape), f32=f32)
    pr = PW.problem(case)
    po = _plan(case, 1)
    try:
        assert api.offt_hip_product_fused(po)
        got = {}
        for mode in ("two", "a", "b", "null", "same"):
            keep = {}
            err = PW.run_product(api, po, dict(case, mode=mode), dev, pr=pr, keep=keep)
            assert err <= W.tol(case), (shape, f32, mode, err)
            got[mode] = keep["got"]
        # squaring against the two-buffer call on a copy of a
        c, ne = api.comm_dict(po), api.local_elems(po)
        a = PW.spec_buffer(c, ne, case, pr[0])
        h0, h1, ho = dev.put(a), dev.put(a), dev.put(np.zeros_like(a))
        api.offt_hip_execute_product(po, h0[1], h1[1], ho[1])
        idx, out = W.out_index(c), dev.get(ho[0], a).astype(np.complex128)
        for mode in ("null", "same"):
            d = np.linalg.norm(got[mode][idx].astype(np.complex128) - out[idx]) / np.linalg.norm(out[idx])
            assert d <= (2e-6 if f32 else 1e-14), (mode, d)
    finally:
        api.offt_3d_fin(po)


@pytest.mark.parametrize("case", [dict(N=[48, 40, 30]), dict(N=[32, 16, 64], r2c=1), dict(N=[16, 16, 64]),
                                  dict(N=[32, 16, 64], r2c=1, f32=1), dict(N=[16, 16, 64], f32=1)])
def test_prod_plans_generic_on_the_device(gpu, case):
    L, torch, dev = gpu
    po = _plan(case, 0)
    try:
        assert not api.offt_hip_product_fused(po)
        for mode in ("two", "b", "null"):
            err = PW.run_product(api, po, dict(case, mode=mode), dev)
            assert err <= W.tol(case), (case, mode, err)
    finally:
        api.offt_3d_fin(po)


@pytest.mark.parametrize("prec", [api.F64, api.F32])
@pytest.mark.parametrize("real", [0, 1])
def test_pointwise_prod_alone(gpu, prec, real):
    L, torch, dev = gpu
    ft = np.float64 if prec == api.F64 else np.float32
    n0, n1, n2 = 5, 7, 24
    s1, s0 = n2 + 4, (n2 + 4) * n1 + 8                      # row pitches wider than the rows
    rng = np.random.default_rng(3 + prec + real)
    size = n0 * s0
    idx = (np.arange(n0)[:, None, None] * s0 + np.arange(n1)[None, :, None] * s1 + np.arange(n2)[None, None, :]).ravel()
    if real:
        x, y = rng.standard_normal(size).astype(ft), rng.standard_normal(size).astype(ft)
    else:
        ct = np.complex128 if prec == api.F64 else np.complex64
        x = (rng.standard_normal(size) + 1j * rng.standard_normal(size)).astype(ct)
        y = (rng.standard_normal(size) + 1j * rng.standard_normal(size)).astype(ct)
    p = prec | (0x100 if real else 0)
    for out_is, yy in ((0, y), (1, y), (0, None)):
        hx, hy = dev.put(x.copy()), dev.put(y.copy())
        ho = hx if out_is == 0 else hy
        assert L.offt_hipk_pointwise_prod(hx[1], hy[1] if yy is not None else None, ho[1], p, n0, n1, n2, s0, s1, 1, None) == 0
        got = dev.get(ho[0], x)
        want = (x if out_is == 0 else y).copy()
        want[idx] = (x[idx] * (y[idx] if yy is not None else x[idx])).astype(want.dtype)
        rel = np.linalg.norm(got.astype(np.complex128) - want) / np.linalg.norm(want)
        assert rel <= (1e-15 if prec == api.F64 else 2e-7), (prec, real, out_is, rel)
        rest = np.ones(size, dtype=bool)
        rest[idx] = False
        assert np.array_equal(got[rest], want[rest])        # the pitch padding is not written


def test_prod_streams_and_async(gpu):
    L, torch, dev = gpu
    case = dict(N=[6, 8, 128])
    po = _plan(case, 1)
    try:
        s = torch.cuda.Stream()
        L.offt_hip_set_stream(po, s.cuda_stream)
        assert PW.run_product(api, po, case, dev) <= 1e-12
        assert L.offt_hip_last_device_seconds(po) > 0.0
        t = (C.c_double * 3)(1, 1, 1)
        L.offt_hip_last_pass_seconds(po, t)
        assert list(t) == [0.0, 0.0, 0.0]
        L.offt_hip_set_async(po, 1)
        c, ne = api.comm_dict(po), api.local_elems(po)
        A, B, want, _ = PW.problem(case)
        ha, hb = dev.put(PW.spec_buffer(c, ne, case, A)), dev.put(PW.spec_buffer(c, ne, case, B))
        api.offt_hip_execute_product(po, ha[1], hb[1], ha[1])
        assert L.offt_hip_wait(po) == 0
        assert PW.out_err(c, dev.get(ha[0], np.zeros(1, dtype=np.complex128)), want) <= 1e-12
        L.offt_hip_set_async(po, 0)
        L.offt_hip_set_stream(po, None)
    finally:
        api.offt_3d_fin(po)


@pytest.mark.parametrize("opt", [1, 0])
def test_prod_repeatable(gpu, opt):
    L, torch, dev = gpu
    case = dict(N=[6, 8, 128], f32=1)
    po = _plan(case, opt)
    try:
        k1, k2 = {}, {}
        PW.run_product(api, po, case, dev, keep=k1)
        PW.run_product(api, po, case, dev, keep=k2)
        assert np.array_equal(k1["got"].view(np.uint8), k2["got"].view(np.uint8))
    finally:
        api.offt_3d_fin(po)


def test_prod_refuses_host_memory(gpu):
    L, torch, dev = gpu
    case = dict(N=[6, 8, 64])
    po = _plan(case, 1)
    try:
        c, ne = api.comm_dict(po), api.local_elems(po)
        A = PW.problem(case)[0]
        host = PW.spec_buffer(c, ne, case, A)
        h = dev.put(host)
        for args, text in (((host.ctypes.data, None, h[1]), b"the first spectrum"), ((h[1], host.ctypes.data, h[1]), b"the second spectrum"),
                           ((h[1], None, host.ctypes.data), b"the output"), ((None, None, h[1]), b"the first spectrum")):
            assert L.offt_hip_execute_product(po, *args) == -1
            assert text in L.offt_hip_last_error() and po.contents.t[api.ALL] >= 99999999.0
        buf = np.zeros(ne, dtype=np.complex128)
        buf[W.in_index(c, False)] = np.fft.ifftn(A).ravel()
        hb = dev.put(buf)
        api.offt_3d_execute_dir(po, hb[1], hb[1], -1)
        assert PW.out_err(c, dev.get(hb[0], buf), A) <= 1e-12
    finally:
        api.offt_3d_fin(po)
