"""Pseudo-spectral product of real fields on the device (-m gpu): the fused real-row launch (fft_prod_real_panel_k) on strided
descriptors, whole r2c plans on the fused route (OFFT_HIP_OPT_PROD_FUSED and OFFT_HIP_OPT_PROD_REAL) against numpy and against
the same plan's generic route, a caller-owned stream, async mode, repeatability.

The reference is numpy in float64 / complex128.  Tolerances are the project's own, rel-L2 against the norm of the reference:
1e-12 / 1e-5 at descriptor level, W.tol (1e-12 / 2e-5) at plan level; the single-precision bounds were checked against the
packed chain emulated in complex64 on the CPU (tests/test_product_real.py: 2.0e-7 on 1024-point lines, 2.7e-7 on the
(4, 24, 1024) plan)."""
import ctypes as C

import numpy as np
import pytest

import _conv_world as W
import _half_world as HW
import _prod_world as PW
from offt_amd import api
from test_convolve_multi import Desc
from test_product_real import real_desc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(built):
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    L = api.lib()
    L.offt_hipk_prod_real_pass.argtypes = [C.POINTER(Desc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.offt_hipk_prepare.argtypes = [C.c_int, C.c_int]
    L.offt_hipk_last_error.restype = C.c_char_p
    return L, torch, HW.Gpu(torch)


SENT = 7.25 - 3.5j


@pytest.mark.parametrize("prec", [api.F64, api.F32])
@pytest.mark.parametrize("n", [64, 128, 256, 512, 1024])
def test_prod_real_pass_descriptors(gpu, n, prec):
    L, torch, dev = gpu
    ct = np.complex128 if prec == api.F64 else np.complex64
    assert L.offt_hipk_prepare(n, prec) == 0
    rng = np.random.default_rng(2 * n + prec)
    h, nb1, nb2 = n // 2 + 1, 3, 2
    for ncols in (12, 3):                         # a ragged last column group; a single partial group
        # a line pitch wider than the columns, and a plane pitch with room for n elements a line: the elements h ... n-1 of a
        # line's pitch belong to no line and must keep the sentinel
        d = real_desc(n, prec, ncols, nb1, pitch=ncols + 3)
        d.in_b1_stride = n * (ncols + 3) + 5
        d.in_b2_stride = nb1 * d.in_b1_stride + 7
        d.nb2 = nb2
        d.scale = 0.5
        b2, b1 = np.arange(nb2)[:, None, None, None], np.arange(nb1)[None, :, None, None]
        c, k = np.arange(ncols)[None, None, :, None], np.arange(h)[None, None, None, :]
        idx = b2 * d.in_b2_stride + b1 * d.in_b1_stride + c * d.in_col_stride + k * d.in_axis_stride
        size = nb2 * d.in_b2_stride
        assert idx.max() < size and len(np.unique(idx)) == idx.size
        owned = np.zeros(size, dtype=bool)
        owned[idx.ravel()] = True
        srcs = []
        for _ in range(2):
            s = np.full(size, SENT, dtype=ct)
            # every element complex, the ends k = 0 and k = n/2 included: their imaginary parts must have no effect
            s[idx.ravel()] = ((rng.standard_normal(idx.shape) + 1j * rng.standard_normal(idx.shape)) / n).astype(ct).ravel()
            srcs.append(s)
        la, lb = srcs[0][idx].astype(np.complex128), srcs[1][idx].astype(np.complex128)
        assert np.abs(la[..., 0].imag).min() > 0 and np.abs(lb[..., h - 1].imag).min() > 0
        ia, ib = np.fft.irfft(la, n, axis=3) * n, np.fft.irfft(lb, n, axis=3) * n
        for two, inplace in ((True, False), (True, True), (False, False), (False, True)):
            want = np.fft.rfft(ia * (ib if two else ia), axis=3) * 0.5
            h0, h1 = dev.put(srcs[0]), dev.put(srcs[1])
            ho = h0 if inplace else dev.put(np.full(size, SENT, dtype=ct))
            assert L.offt_hipk_prod_real_pass(C.byref(d), h0[1], h1[1] if two else None, ho[1], None) == 0, L.offt_hipk_last_error()
            got = dev.get(ho[0], srcs[0])
            err = np.linalg.norm(got[idx].astype(np.complex128) - want) / np.linalg.norm(want)
            print(f"prod_real_pass n={n} prec={prec} ncols={ncols} two={two} inplace={inplace} rel={err:.3e}")
            assert err <= (1e-12 if prec == api.F64 else 1e-5), (n, prec, ncols, two, inplace, err)
            assert np.all(got[~owned] == ct(SENT)), (n, prec, ncols, "an element no line owns was written")
            if not inplace:                       # a source that is not dst is not written
                assert np.array_equal(dev.get(h0[0], srcs[0]), srcs[0])
            assert np.array_equal(dev.get(h1[0], srcs[1]), srcs[1])


def _plan(case, fused=1, real=1):
    po = HW.make_plan(api, case)
    L = api.lib()
    assert L.offt_hip_set_option(po, api.OPT_PROD_FUSED, fused) == 0 and L.offt_hip_set_option(po, api.OPT_PROD_REAL, real) == 0
    return po


@pytest.mark.parametrize("f32", [0, 1])
@pytest.mark.parametrize("shape", [(10, 12, 64), (6, 8, 128), (13, 5, 512), (4, 24, 1024)])
def test_prod_real_plans_fused(gpu, shape, f32):
    L, torch, dev = gpu
    case = dict(N=list(shape), r2c=1, f32=f32)
    pr = PW.problem(case)
    po = _plan(case)
    try:
        assert api.offt_hip_product_fused(po) == 1
        c, ne = api.comm_dict(po), api.local_elems(po)
        idx = W.out_index(c)
        got = {}
        for mode in ("two", "a", "b", "null", "same"):
            keep = {}
            err = PW.run_product(api, po, dict(case, mode=mode), dev, pr=pr, keep=keep)
            print(f"prod_real plan {shape} f32={f32} mode={mode} rel={err:.3e}")
            assert err <= W.tol(case), (shape, f32, mode, err)
            got[mode] = keep["got"][idx].astype(np.complex128)
        # squaring against the two-buffer call on a copy of a
        a = PW.spec_buffer(c, ne, case, pr[0])
        h0, h1, ho = dev.put(a), dev.put(a), dev.put(np.zeros_like(a))
        api.offt_hip_execute_product(po, h0[1], h1[1], ho[1])
        out = dev.get(ho[0], a).astype(np.complex128)[idx]
        for mode in ("null", "same"):
            dd = np.linalg.norm(got[mode] - out) / np.linalg.norm(out)
            assert dd <= (2e-6 if f32 else 1e-14), (mode, dd)
        # ... and the fused route against the same plan's generic route
        assert L.offt_hip_set_option(po, api.OPT_PROD_REAL, 0) == 0 and api.offt_hip_product_fused(po) == 0
        for mode in ("two", "null"):
            keep = {}
            err = PW.run_product(api, po, dict(case, mode=mode), dev, pr=pr, keep=keep)
            assert err <= W.tol(case), (shape, f32, mode, "generic", err)
            g = keep["got"][idx].astype(np.complex128)
            dd = np.linalg.norm(got[mode] - g) / np.linalg.norm(g)
            assert dd <= W.tol(case), (shape, f32, mode, "fused against generic", dd)
    finally:
        api.offt_3d_fin(po)


def test_prod_real_streams_async_and_repeatable(gpu):
    L, torch, dev = gpu
    case = dict(N=[6, 8, 128], r2c=1)
    po = _plan(case)
    try:
        assert api.offt_hip_product_fused(po) == 1
        s = torch.cuda.Stream()
        L.offt_hip_set_stream(po, s.cuda_stream)
        k1, k2 = {}, {}
        assert PW.run_product(api, po, case, dev, keep=k1) <= 1e-12
        assert L.offt_hip_last_device_seconds(po) > 0.0
        assert PW.run_product(api, po, case, dev, keep=k2) <= 1e-12
        assert np.array_equal(k1["got"].view(np.uint8), k2["got"].view(np.uint8))     # two identical calls: identical bits
        L.offt_hip_set_async(po, 1)
        c, ne = api.comm_dict(po), api.local_elems(po)
        A, B, want, _ = PW.problem(case)
        ha, hb = dev.put(PW.spec_buffer(c, ne, case, A)), dev.put(PW.spec_buffer(c, ne, case, B))
        api.offt_hip_execute_product(po, ha[1], hb[1], ha[1])
        assert L.offt_hip_wait(po) == 0
        out = dev.get(ha[0], np.zeros(1, dtype=np.complex128))
        assert PW.out_err(c, out, want) <= 1e-12
        idx = W.out_index(c)
        assert np.array_equal(out[idx], k1["got"][idx])                                # ... and the async call the same bits again
        L.offt_hip_set_async(po, 0)
        L.offt_hip_set_stream(po, None)
    finally:
        api.offt_3d_fin(po)
