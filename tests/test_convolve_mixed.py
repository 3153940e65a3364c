"""Fused spectral convolution at mixed-radix line lengths: OFFT_HIP_OPT_CONV_MIXED (include/offt_hip.h),
offt_filter_desc::mixed (offt_amd/csrc/offt_hipk.h) and the kernels under them, fft_conv_panelx_k and
fft_conv_half_panelx_k (convx_body, offt_amd/csrc/offt_panel.hpp).

  * routing without a device: the registered (length, precision) pairs with the field set, the same descriptors without
    it, and everything that has no fused kernel either way;
  * the host's route on the CPU convolution and pad backends: option on = one fused launch, option off = forward, multiply,
    inverse as before; the layouts that never fuse; the environment default; a pruned half box with both options;
  * -m gpu: random fused descriptors of every instance against numpy (full lines and half lines, sentinels, NaN in what
    must not be read), plans on one rank against numpy and against the option-off route, the fallback from a
    cache-keeping request, a free-space convolution of a 48 x 32 x 32 box on a 96 x 64 x 64 plan."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _conv_world as W
import _half_world as HW
from offt_amd import api
from test_half_box import Desc, _index, half_desc, pad_cpu  # noqa: F401  (pad_cpu: fixture)
from test_convolve import conv_cpu  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the registered instances (offt_reg_conv_mixed_*.hip)
LENGTHS = {api.F64: (96, 192, 320, 384, 640, 768, 1000), api.F32: (384, 640, 768, 1000)}
INSTANCES = [(prec, n) for prec, ns in LENGTHS.items() for n in ns]
OPT_CONV_MIXED = 12  # include/offt_hip.h (api.OPT_CONV_MIXED)
OPT_ZGROUP_MIB = 0


class FDesc(C.Structure):
    """offt_filter_desc (offt_amd/csrc/offt_hipk.h), `mixed` included"""
    _fields_ = [("kind", C.c_int), ("mixed", C.c_int), ("axis_stride", C.c_longlong), ("col_stride", C.c_longlong),
                ("b1_stride", C.c_longlong), ("b2_stride", C.c_longlong)]


def conv_desc(n, prec, ncols, nb1, half=0, mixed=1, pad=0, fpad=0, kind=0, scale=1.0):
    """contiguous lines in rows of n + pad elements, the filter in rows of n + fpad"""
    d = half_desc(n, prec, ncols, nb1, 1, 1, half, pad=pad, scale=scale)
    d.out_axis_stride, d.out_col_stride, d.out_b1_stride = 1, n + fpad, (n + fpad) * ncols
    f = FDesc()
    f.kind, f.mixed, f.axis_stride, f.col_stride, f.b1_stride = kind, mixed, 1, n + fpad, (n + fpad) * ncols
    return d, f


@pytest.fixture(scope="module")
def kl(built):
    L = api.lib()
    L.offt_hipk_conv_kernel_name.restype = C.c_char_p
    L.offt_hipk_conv_kernel_name.argtypes = [C.POINTER(Desc), C.POINTER(FDesc)]
    L.offt_hipk_conv_has_fused.argtypes = [C.POINTER(Desc), C.POINTER(FDesc)]
    L.offt_hipk_conv_pass.argtypes = [C.POINTER(Desc), C.POINTER(FDesc), C.c_void_p, C.c_void_p, C.c_void_p]
    L.offt_hipk_prepare.argtypes = [C.c_int, C.c_int]
    L.offt_hipk_last_error.restype = C.c_char_p
    return L


# ---- routing without a device ---------------------------------------------------------------------------------------------
def test_filter_desc_layout_is_what_it_was():
    """`mixed` sits in the alignment padding behind kind: the mirror of the older tests (no such field) still describes it"""
    from test_convolve import FDesc as Old
    assert C.sizeof(FDesc) == C.sizeof(Old) == 40
    for f in ("kind", "axis_stride", "col_stride", "b1_stride", "b2_stride"):
        assert getattr(FDesc, f).offset == getattr(Old, f).offset, f
    assert FDesc.mixed.offset == 4 and FDesc.axis_stride.offset == 8
    assert api.OPT_CONV_MIXED == OPT_CONV_MIXED


def test_conv_mixed_kernel_routing_without_a_gpu(kl):
    L = kl
    name = lambda d, f: L.offt_hipk_conv_kernel_name(C.byref(d), C.byref(f)).decode()
    fused = lambda d, f: L.offt_hipk_conv_has_fused(C.byref(d), C.byref(f))
    for prec, n in INSTANCES:
        for kind in (0, 1):
            for ncols in (8, 7):
                d, f = conv_desc(n, prec, ncols, 2, kind=kind)
                assert name(d, f) == "fft_conv_panelx_k" and fused(d, f) == 1, (n, prec, kind)
                d, f = conv_desc(n, prec, ncols, 2, half=3, kind=kind)
                assert name(d, f) == "fft_conv_half_panelx_k" and fused(d, f) == 1, (n, prec, kind)
                for half in (0, 3):   # the field at 0: as before
                    d, f = conv_desc(n, prec, ncols, 2, half=half, mixed=0, kind=kind)
                    assert name(d, f) == "no fused kernel" and fused(d, f) == 0, (n, prec, kind, half)
        for half in (1, 2):           # one bit alone
            d, f = conv_desc(n, prec, 8, 2, half=half)
            assert name(d, f) == "no fused kernel" and fused(d, f) == 0, (n, prec, half)
        d, f = conv_desc(n, prec, 8, 2)
        f.axis_stride = 8                                # strided filter axis
        assert name(d, f) == "no fused kernel"
        d, f = conv_desc(n, prec, 8, 2)
        d.in_contig, d.in_axis_stride, d.in_col_stride = 0, 8, 1   # strided lines
        assert name(d, f) == "no fused kernel"
        d, f = conv_desc(n, prec, 8, 2)
        d.in_split = n // 4                              # a split line
        assert name(d, f) == "no fused kernel"
        d, f = conv_desc(n, prec, 8, 2)
        d.real_input = 1
        assert name(d, f) == "no fused kernel"
        d, f = conv_desc(n, prec, 8, 2, kind=2)          # no such filter kind
        assert name(d, f) == "no fused kernel"
    for prec in (api.F64, api.F32):
        for n in (48, 250, 1001, 67, 2048):              # swept but not registered, Bluestein, too long
            for half in (0, 3):
                d, f = conv_desc(n, prec, 8, 2, half=half)
                assert name(d, f) == "no fused kernel" and fused(d, f) == 0, (n, prec, half)
        for mixed in (0, 1):                             # the powers of two do not care
            d, f = conv_desc(1024, prec, 8, 2, mixed=mixed)
            assert name(d, f) == "fft_conv_panel_k"
            d, f = conv_desc(1024, prec, 8, 2, half=3, mixed=mixed)
            assert name(d, f) == "fft_conv_half_panel_k"
    for n in (96, 192, 320):                             # single precision has no instance below 384 points
        d, f = conv_desc(n, api.F32, 8, 2)
        assert name(d, f) == "no fused kernel", n


# ---- CPU tier: the host's route ----------------------------------------------------------------------------------------------
def _cpu_convolve(case, conv_mixed):
    """W.cpu_convolve with the option set on the plan before the call; (rel-L2, offt_hip_convolve_fused)"""
    L = api.lib()
    po = HW.make_plan(api, case)
    try:
        assert L.offt_hip_get_option(po, OPT_CONV_MIXED) == 0, "off by default"
        assert L.offt_hip_set_option(po, OPT_CONV_MIXED, conv_mixed) == 0, L.offt_hip_last_error()
        assert L.offt_hip_get_option(po, OPT_CONV_MIXED) == (1 if conv_mixed else 0)
        c = api.comm_dict(po)
        x, H, want = W.problem(case["N"], case.get("r2c"), case.get("cplx"))
        data, filt = W.local_arrays(c, api.local_elems(po), case, x, H)
        L.offt_hip_set_output_scale(po, W.SCALE)
        api.offt_hip_execute_convolve(po, data.ctypes.data, filt.ctypes.data, api.FILTER_COMPLEX if case.get("cplx") else api.FILTER_REAL)
        return W.check(c, case, data, want), api.offt_hip_convolve_fused(po)
    finally:
        api.offt_3d_fin(po)


@pytest.mark.parametrize("r2c", [0, 1])
def test_conv_mixed_route_cpu(conv_cpu, r2c):
    CB = conv_cpu
    for cplx in (0, 1):
        case = dict(N=[96, 8, 16], r2c=r2c, cplx=cplx)
        for on in (1, 7, 0):   # (any non-zero value switches it on)
            k0, p0 = CB.cpu_backend_conv_count(), CB.cpu_backend_pointwise_count()
            err, fused = _cpu_convolve(case, on)
            assert err <= 1e-12, (case, on, err)
            assert fused == bool(on), (case, on)
            # the fused route launches conv_pass once, the unfused one the multiply once
            assert CB.cpu_backend_conv_count() - k0 == (1 if on else 0), (case, on)
            assert CB.cpu_backend_pointwise_count() - p0 == (0 if on else 1), (case, on)


def test_conv_mixed_other_layouts_and_lengths_cpu(conv_cpu):
    CB = conv_cpu
    # S = 1 (x-y-z, in place and rotated): the x lines are not contiguous where the fused launch would run
    for r2c in (0, 1):
        case = dict(N=[96, 8, 16], r2c=r2c, cplx=1 - r2c, params={"S": 1})
        k0, p0 = CB.cpu_backend_conv_count(), CB.cpu_backend_pointwise_count()
        err, fused = _cpu_convolve(case, 1)
        assert not fused and err <= 1e-12, (case, err)
        assert CB.cpu_backend_conv_count() == k0 and CB.cpu_backend_pointwise_count() == p0 + 1
    # the y-z-x layout: whichever route it reports is the one that ran
    case = dict(N=[96, 96, 8], eq=1, cplx=1)
    k0, p0 = CB.cpu_backend_conv_count(), CB.cpu_backend_pointwise_count()
    err, fused = _cpu_convolve(case, 1)
    assert err <= 1e-12, err
    assert (CB.cpu_backend_conv_count() > k0) == fused and (CB.cpu_backend_pointwise_count() > p0) == (not fused)
    # an x length without an instance stays unfused with the option on; single precision below 384 points too
    for case in (dict(N=[48, 8, 16]), dict(N=[250, 4, 6]), dict(N=[96, 8, 16], f32=1)):
        err, fused = _cpu_convolve(case, 1)
        assert not fused and err <= W.tol(case), (case, err)
    err, fused = _cpu_convolve(dict(N=[384, 4, 6], f32=1, cplx=1), 1)
    assert fused and err <= 2e-5, err
    # a power-of-two plan does not care
    for on in (0, 1):
        err, fused = _cpu_convolve(dict(N=[64, 8, 16]), on)
        assert fused and err <= 1e-12


def test_conv_mixed_unknown_to_no_one_cpu(conv_cpu):
    """set / get round trip on a live plan; the option is read by the next convolve"""
    L = api.lib()
    po = api.offt_3d_init(96, 8, 16)
    try:
        assert L.offt_hip_get_option(po, OPT_CONV_MIXED) == 0 and not api.offt_hip_convolve_fused(po)
        for v, want in ((1, 1), (0, 0), (5, 1), (0, 0)):
            assert L.offt_hip_set_option(po, OPT_CONV_MIXED, v) == 0, L.offt_hip_last_error()
            assert L.offt_hip_get_option(po, OPT_CONV_MIXED) == want
            assert api.offt_hip_convolve_fused(po) == bool(want)
    finally:
        api.offt_3d_fin(po)


_ENV_CHILD = """
import os, sys
sys.path[:0] = [%r, %r]
import cpu_world, _conv_world as W
from offt_amd import api
cpu_world._cb_lib = W.conv_cb_lib
cpu_world.install(0, 1, p1=1)
L = api.lib()
po = api.offt_3d_init(96, 8, 16)
v = L.offt_hip_get_option(po, 12)
f = int(api.offt_hip_convolve_fused(po))
# the environment after the plan exists changes nothing on it; the next plan reads it
os.environ["OFFT_CONV_MIXED"] = "0" if v else "1"
v1, f1 = L.offt_hip_get_option(po, 12), int(api.offt_hip_convolve_fused(po))
p2 = api.offt_3d_init(96, 8, 16)
v2 = L.offt_hip_get_option(p2, 12)
print("RESULT", v, f, v1, f1, v2)
api.offt_3d_fin(p2)
api.offt_3d_fin(po)
"""


def test_conv_mixed_environment_default(built):
    """OFFT_CONV_MIXED is read once, by offt_3d_init, as the option's default"""
    subprocess.check_call(["make", "-s", "-C", ROOT, "tests/libcpubackend_conv.so"])
    for val, want in ((None, "RESULT 0 0 0 0 1"), ("1", "RESULT 1 1 1 1 0"), ("0", "RESULT 0 0 0 0 1")):
        env = {k: v for k, v in os.environ.items() if k != "OFFT_CONV_MIXED"}
        if val is not None:
            env["OFFT_CONV_MIXED"] = val
        p = subprocess.run([sys.executable, "-c", _ENV_CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=300)
        out = p.stdout.decode()
        assert p.returncode == 0 and want in out.splitlines(), (val, out[-2000:])


def _check(res, case):
    for k, e in res.items():
        assert np.isfinite(e) and e <= HW.tol(case), (case, k, e)


def test_conv_mixed_half_box_route_cpu(pad_cpu):
    CB = pad_cpu
    L = api.lib()
    shape = (96, 64, 64)
    Nx, Ny, Nz = shape
    fwd = [(Nz, Ny // 2, Nx // 2, 1, 1, 0), (Ny, Nx // 2, Nz, 1, 1, 0), (Nx, Ny, Nz, 1, 1, 0)]
    inv = [(Nx, Ny, Nz, 1, 2, 0), (Ny, Nx // 2, Nz, 1, 2, 0), (Nz, Ny // 2, Nx // 2, 1, 2, 0)]
    conv = fwd[:2] + [(Nx, Ny, Nz, 1, 3, 1)] + inv[1:]
    case = dict(N=list(shape))
    po = HW.make_plan(api, case)
    try:
        pr = HW.problem(case["N"], 0)
        assert L.offt_hip_set_option(po, api.OPT_HALF_MIXED, 1) == 0 and L.offt_hip_set_option(po, OPT_CONV_MIXED, 1) == 0
        api.offt_hip_set_half_box(po, True)
        assert api.offt_hip_half_box_pruned(po) and api.offt_hip_convolve_fused(po)
        z0, p0 = CB.cpu_backend_pad_zero_count(), CB.cpu_backend_pointwise_count()
        CB.cpu_backend_pad_log_reset()
        res, _ = HW.run_plan(api, po, case, HW.Host(), pr)
        _check(res, case)
        assert CB.cpu_backend_pad_zero_count() == z0 and CB.cpu_backend_pointwise_count() == p0
        got = HW.launches(CB)
        assert got == fwd + inv + conv, got
        assert [r for r in got if r[5]] == [(96, Ny, Nz, 1, 3, 1)], "one fused launch on the half lines of x"
        # the fused route off on the live plan: pruned forward, one multiply, pruned inverse, as before
        assert L.offt_hip_set_option(po, OPT_CONV_MIXED, 0) == 0
        assert api.offt_hip_half_box_pruned(po) and not api.offt_hip_convolve_fused(po)
        p0 = CB.cpu_backend_pointwise_count()
        CB.cpu_backend_pad_log_reset()
        res, _ = HW.run_plan(api, po, case, HW.Host(), pr)
        _check(res, case)
        assert HW.launches(CB) == fwd + inv + fwd + inv and CB.cpu_backend_pointwise_count() == p0 + 1
        # the fused route on, the pruning off: the fallback clears the padding, and its convolve fuses on full lines
        assert L.offt_hip_set_option(po, OPT_CONV_MIXED, 1) == 0 and L.offt_hip_set_option(po, api.OPT_HALF_MIXED, 0) == 0
        assert not api.offt_hip_half_box_pruned(po) and api.offt_hip_convolve_fused(po)
        z0 = CB.cpu_backend_pad_zero_count()
        CB.cpu_backend_pad_log_reset()
        res, _ = HW.run_plan(api, po, case, HW.Host(), pr)
        _check(res, case)
        got = HW.launches(CB)
        assert CB.cpu_backend_pad_zero_count() == z0 + 2 and all(r[4] == 0 for r in got)
        assert [r for r in got if r[5]] == [(96, Ny, Nz, 1, 0, 1)]
    finally:
        api.offt_3d_fin(po)


# ---- GPU tier ----------------------------------------------------------------------------------------------------------
SENT = 8  # sentinel elements on either side of the array


def _random_descriptors(L, prec, n, half):
    """every filter kind and panel remainder of one instance: the lines against numpy, everything else bitwise untouched"""
    import torch
    rng = np.random.default_rng(5200 + n + 7 * prec + half)
    assert L.offt_hipk_prepare(n, prec) == 0, L.offt_hipk_last_error()
    ft, ct = (np.float64, np.complex128) if prec == api.F64 else (np.float32, np.complex64)
    kept = n // 2 if half else n
    for kind in (0, 1):
        for ncols in (3, 13, 21):                    # never a whole number of panels (4, 8 or 16 columns)
            nb1 = int(rng.integers(2, 4))
            pad, fpad = int(rng.integers(0, 3)), int(rng.integers(0, 3))
            scale = float(rng.choice([0.5, 1.0 / n, 3.0]))
            d, f = conv_desc(n, prec, ncols, nb1, half=half, pad=pad, fpad=fpad, kind=kind, scale=scale)
            assert L.offt_hipk_conv_kernel_name(C.byref(d), C.byref(f)).decode() == ("fft_conv_half_panelx_k" if half else "fft_conv_panelx_k")
            ii = _index(d, "in", nb1, ncols, n)
            fi = np.arange(nb1)[:, None, None] * f.b1_stride + np.arange(ncols)[None, :, None] * f.col_stride + np.arange(n)[None, None, :]
            nin, nf = int(ii.max()) + 1 + pad, int(fi.max()) + 1 + 16
            lines = (rng.standard_normal((nb1, ncols, n)) + 1j * rng.standard_normal((nb1, ncols, n))).astype(ct)
            if half:
                lines[:, :, n // 2:] = 0
            h = (rng.standard_normal(nf) + 1j * rng.standard_normal(nf)) if kind else rng.standard_normal(nf)
            H = h[fi].astype(ct if kind else ft).astype(np.complex128)
            want = np.fft.ifft(H * np.fft.fft(lines.astype(np.complex128), axis=2), axis=2)[:, :, :kept] * n * scale
            buf = np.full(nin + 2 * SENT, 7.0 + 7.0j, dtype=ct)
            buf[SENT:SENT + nin] = (rng.standard_normal(nin) + 1j * rng.standard_normal(nin)).astype(ct)
            buf[SENT + ii.ravel()] = lines.ravel()
            if half:
                buf[SENT + ii[:, :, n // 2:].ravel()] = np.nan + 1j * np.nan   # neither read nor written
            dx = torch.from_numpy(buf.view(ft).copy()).cuda()
            dh = torch.from_numpy((h.astype(ct).view(ft) if kind else h.astype(ft)).copy()).cuda()
            torch.cuda.synchronize()
            rc = L.offt_hipk_conv_pass(C.byref(d), C.byref(f), dh.data_ptr(), dx.data_ptr() + SENT * buf.itemsize, None)
            assert rc == 0, L.offt_hipk_last_error()
            torch.cuda.synchronize()
            got = dx.cpu().numpy().view(ct)
            written = np.zeros(nin + 2 * SENT, dtype=bool)
            written[SENT + ii[:, :, :kept].ravel()] = True
            # sentinels, the padding between lines and (half lines) the upper half of every line: bit-identical
            assert np.array_equal(got[~written].view(ft), buf[~written].view(ft), equal_nan=True), (n, prec, half, kind, ncols)
            g = got[SENT + ii[:, :, :kept]].astype(np.complex128)
            err = np.linalg.norm(g - want) / np.linalg.norm(want)
            print(n, prec, half, kind, ncols, err)
            assert np.isfinite(err) and err <= (1e-12 if prec == api.F64 else 1e-5), (n, prec, half, kind, ncols, err)
    # without the field these lines have no fused kernel: the launch fails, it runs nothing
    d, f = conv_desc(n, prec, 4, 1, half=half, mixed=0)
    assert L.offt_hipk_conv_pass(C.byref(d), C.byref(f), None, None, None) == -1


@pytest.mark.gpu
@pytest.mark.parametrize("prec,n", INSTANCES)
def test_conv_mixed_random_fused_descriptors(kl, prec, n):
    _random_descriptors(kl, prec, n, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("prec,n", INSTANCES)
def test_conv_mixed_random_fused_half_descriptors(kl, prec, n):
    _random_descriptors(kl, prec, n, 3)


def _gpu_convolve(po, case):
    """convolve this plan's block on the device; (rel-L2 against numpy, the result's elements of the input block)"""
    import torch
    L = api.lib()
    c = api.comm_dict(po)
    x, H, want = W.problem(case["N"], case.get("r2c"), case.get("cplx"))
    data, filt = W.local_arrays(c, api.local_elems(po), case, x, H)
    dd = torch.from_numpy(data.view(data.real.dtype).copy()).cuda()
    df = torch.from_numpy(filt.view(filt.real.dtype if filt.dtype.kind == "c" else filt.dtype).copy()).cuda()
    torch.cuda.synchronize()
    L.offt_hip_set_output_scale(po, W.SCALE)
    api.offt_hip_execute_convolve(po, dd.data_ptr(), df.data_ptr(), api.FILTER_COMPLEX if case.get("cplx") else api.FILTER_REAL)
    torch.cuda.synchronize()
    got = dd.cpu().numpy().view(data.dtype)
    r2c = bool(case.get("r2c"))
    blk = got.view(np.float32 if got.dtype == np.complex64 else np.float64)[W.in_index(c, True)] if r2c else got[W.in_index(c, False)]
    return W.check(c, case, got, want), blk.astype(np.complex128 if not r2c else np.float64)


def _on_and_off(case, zgroup_mib=None):
    L = api.lib()
    po = HW.make_plan(api, case)
    try:
        if zgroup_mib is not None:
            assert L.offt_hip_set_option(po, OPT_ZGROUP_MIB, zgroup_mib) == 0
        assert not api.offt_hip_convolve_fused(po), "the option is off by default"
        err_off, off = _gpu_convolve(po, case)
        assert L.offt_hip_set_option(po, OPT_CONV_MIXED, 1) == 0, L.offt_hip_last_error()
        assert api.offt_hip_convolve_fused(po), case
        err_on, on = _gpu_convolve(po, case)
        rel = float(np.linalg.norm(on - off) / np.linalg.norm(off))
        print(case, "fused", err_on, "unfused", err_off, "fused against unfused", rel)
        assert err_off <= W.tol(case) and err_on <= W.tol(case) and rel <= W.tol(case), (case, err_on, err_off, rel)
    finally:
        api.offt_3d_fin(po)


@pytest.mark.gpu
@pytest.mark.parametrize("r2c", [0, 1])
@pytest.mark.parametrize("shape,f32", [((96, 40, 30), 0), ((96, 96, 96), 0), ((192, 64, 67), 0), ((384, 16, 8), 1)])
def test_conv_mixed_one_rank_gpu(built, shape, f32, r2c):
    import torch
    torch.cuda.set_device(0)
    for cplx in (0, 1):
        _on_and_off(dict(N=list(shape), f32=f32, r2c=r2c, cplx=cplx))


@pytest.mark.gpu
def test_conv_mixed_cache_keeping_request_falls_back(built):
    """groups of 1 MiB on a 96 x 64 x 64 plan are 10 z-planes of 96 KiB, which do not divide 64: the y pass of a group keeps
    its stores and asks the fused launch to keep its own (out_keep) -- the mixed-radix instances have no cache-keeping
    twin, the launch runs on the plain one"""
    import torch
    torch.cuda.set_device(0)
    assert int(1.0 / (96 * 64 * 16 / 2.0 ** 20)) == 10 and 64 % 10
    for r2c in (0, 1):
        _on_and_off(dict(N=[96, 64, 64], r2c=r2c, cplx=1), zgroup_mib=1)


def _free_space_problem():
    """a Gaussian of width sigma = 3 centred at (8,8,8) and cut to exactly zero beyond 8 cells from its centre along any
    axis, on the 96 x 64 x 64 grid: its support [0,16]^3 and every shift of it by p inside the 48 x 32 x 32 box stay on the
    grid, nothing wraps.  A delta at p = (36, 20, 3) puts the peak at (44, 28, 11): on a periodic grid of the box's size the
    cells x = 48 ... 52 and y = 32 ... 36 of the shifted kernel would come back at x = 0 ... 4 and y = 0 ... 4."""
    N = (96, 64, 64)
    ax = [np.arange(n) - 8.0 for n in N]
    g = np.exp(-(ax[0][:, None, None] ** 2 + ax[1][None, :, None] ** 2 + ax[2][None, None, :] ** 2) / 18.0)
    g[(np.abs(ax[0]) > 8)[:, None, None] | (np.abs(ax[1]) > 8)[None, :, None] | (np.abs(ax[2]) > 8)[None, None, :]] = 0.0
    p = (36, 20, 3)
    want = np.roll(g, p, axis=(0, 1, 2))[:48, :32, :32].copy()
    return N, g, p, want


def test_conv_mixed_free_space_claim_on_the_cpu():
    """the claim test_conv_mixed_half_box_free_space rests on: the zero-padded convolution equals the shifted kernel inside
    the box, the periodic one on the box's own grid does not"""
    N, g, p, want = _free_space_problem()
    d = np.zeros((48, 32, 32))
    d[p] = 1.0
    per = np.fft.ifftn(np.fft.fftn(d) * np.fft.fftn(g[:48, :32, :32])).real
    assert np.linalg.norm(per - want) / np.linalg.norm(want) > 1e-3
    d2 = np.zeros(N)
    d2[p] = 1.0
    free = np.fft.ifftn(np.fft.fftn(d2) * np.fft.fftn(g)).real[:48, :32, :32]
    assert np.linalg.norm(free - want) / np.linalg.norm(want) <= 1e-12


@pytest.mark.gpu
def test_conv_mixed_half_box_free_space(built):
    """box in, box out on a pruned and fused 96 x 64 x 64 half-box plan: a delta at p convolved with the plan's own
    transform of a kernel that does not wrap is the kernel shifted by p, with no periodic image; and the random problem of
    the other half-box tests (forward, inverse, convolve against numpy on the zero-padded array)"""
    import torch
    torch.cuda.set_device(0)
    N, g, p, want = _free_space_problem()
    po = api.offt_3d_init(*N)
    L = api.lib()
    try:
        c = api.comm_dict(po)
        case = dict(N=list(N))
        gbuf, _ = W.local_arrays(c, api.local_elems(po), case, g.astype(np.complex128), np.zeros((1, 1, 1)))
        dh = torch.from_numpy(gbuf.view(np.float64).copy()).cuda()
        api.offt_3d_execute(po, dh.data_ptr(), dh.data_ptr())   # H = F(g): the full transform, half box off
        assert L.offt_hip_set_option(po, api.OPT_HALF_MIXED, 1) == 0 and L.offt_hip_set_option(po, OPT_CONV_MIXED, 1) == 0
        api.offt_hip_set_half_box(po, True)
        assert api.offt_hip_half_box_pruned(po) and api.offt_hip_convolve_fused(po)
        delta = np.zeros(N)
        delta[p] = 1.0
        dbuf = HW.poisoned_input(c, api.local_elems(po), case, delta.astype(np.complex128))
        dd = torch.from_numpy(dbuf.view(np.float64).copy()).cuda()
        L.offt_hip_set_output_scale(po, 1.0 / np.prod(N))
        api.offt_hip_execute_convolve(po, dd.data_ptr(), dh.data_ptr(), api.FILTER_COMPLEX)
        torch.cuda.synchronize()
        L.offt_hip_set_output_scale(po, 1.0)
        full = np.zeros(N)
        full[:48, :32, :32] = want
        err = HW.box_err(c, case, dd.cpu().numpy().view(np.complex128), full.astype(np.complex128))
        print("free space", err)
        assert err <= 1e-12, err
        res, _ = HW.run_plan(api, po, case, HW.Gpu(torch))
        print(res)
        _check(res, case)
    finally:
        api.offt_3d_fin(po)
