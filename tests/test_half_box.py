"""Half-box plans: offt_hip_set_half_box (zero-padded input in the low half of every axis) and the half-line kernels under it.

  * routing without a device: offt_hipk_has_half / offt_hipk_kernel_name, the fused convolve's half = 3 form, the layout
    of offt_pass_desc;
  * the host's schedules on the CPU pad backend (tests/cpu_backend_pad.c), the padding NaN every time: pruned and fallback
    plans against numpy on the explicitly padded array, the recorded batch counts, refusals, gloo worlds of 2 and 4 ranks;
  * -m gpu: the four half-line flavours and the fused half convolve descriptor by descriptor (NaN in what must not be read,
    a sentinel in what must not be written), plans on one rank, a free-space convolution, a thread world of 2 ranks."""
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
from offt_amd import api
from test_convolve import FDesc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Desc(C.Structure):
    """offt_pass_desc (offt_amd/csrc/offt_hipk.h), field by field, `half` included"""
    _fields_ = [("n", C.c_int), ("precision", C.c_int), ("direction", C.c_int), ("ncols", C.c_int),
                ("nb1", C.c_int), ("nb2", C.c_int),
                ("in_axis_stride", C.c_longlong), ("in_col_stride", C.c_longlong), ("in_b1_stride", C.c_longlong),
                ("in_b2_stride", C.c_longlong),
                ("out_axis_stride", C.c_longlong), ("out_col_stride", C.c_longlong), ("out_b1_stride", C.c_longlong),
                ("out_b2_stride", C.c_longlong),
                ("in_split", C.c_int), ("in_split_nfloor", C.c_int), ("out_split", C.c_int), ("out_split_nfloor", C.c_int),
                ("in_block_stride", C.c_longlong), ("out_block_stride", C.c_longlong),
                ("in_block_tab", C.c_void_p), ("out_block_tab", C.c_void_p),
                ("in_contig", C.c_int), ("out_contig", C.c_int), ("variant", C.c_int), ("scale", C.c_double),
                ("real_input", C.c_int), ("out_keep", C.c_int), ("no_pairs", C.c_int), ("half", C.c_int), ("tw4", C.c_void_p),
                ("tw4_b1", C.c_int), ("tw4_n2", C.c_int)]


FLAVOURS = [(1, 0, 1), (1, 1, 1), (1, 1, 2), (0, 1, 2)]  # (in_contig, out_contig, half): what the z-y-x schedule and its mirror launch


def half_desc(n, prec, ncols, nb1, inc, outc, half, pad=0, direction=-1, scale=1.0):
    """a contiguous side: rows of n + pad elements, one per column; a strided side: rows of ncols + pad elements, one per axis index"""
    d = Desc()
    d.n, d.precision, d.direction, d.ncols, d.nb1, d.nb2 = n, prec, direction, ncols, nb1, 1
    d.in_contig, d.out_contig, d.variant, d.scale, d.half = inc, outc, -1, scale, half

    def side(contig):
        if contig:
            return 1, n + pad, (n + pad) * ncols + pad
        return ncols + pad, 1, (ncols + pad) * n + pad
    d.in_axis_stride, d.in_col_stride, d.in_b1_stride = side(inc)
    d.out_axis_stride, d.out_col_stride, d.out_b1_stride = side(outc)
    return d


@pytest.fixture(scope="module")
def kl(built):
    L = api.lib()
    L.offt_hipk_has_half.argtypes = [C.POINTER(Desc)]
    L.offt_hipk_kernel_name.restype = C.c_char_p
    L.offt_hipk_kernel_name.argtypes = [C.POINTER(Desc)]
    L.offt_hipk_keeps_output.argtypes = [C.POINTER(Desc)]
    L.offt_hipk_fft_pass.argtypes = [C.POINTER(Desc), C.c_void_p, C.c_void_p, C.c_void_p]
    L.offt_hipk_conv_kernel_name.restype = C.c_char_p
    L.offt_hipk_conv_kernel_name.argtypes = [C.POINTER(Desc), C.POINTER(FDesc)]
    L.offt_hipk_conv_has_fused.argtypes = [C.POINTER(Desc), C.POINTER(FDesc)]
    L.offt_hipk_conv_pass.argtypes = [C.POINTER(Desc), C.POINTER(FDesc), C.c_void_p, C.c_void_p, C.c_void_p]
    L.offt_hipk_zero_outside.argtypes = [C.c_void_p] + [C.c_int] * 7 + [C.c_longlong] * 3 + [C.c_void_p]
    L.offt_hipk_prepare.argtypes = [C.c_int, C.c_int]
    L.offt_hipk_last_error.restype = C.c_char_p
    return L


def conv_half_desc(n, prec, ncols, nb1, half, pad=0, fpad=0, kind=0, scale=1.0):
    d = half_desc(n, prec, ncols, nb1, 1, 1, half, pad=pad, scale=scale)
    d.out_axis_stride, d.out_col_stride, d.out_b1_stride = 1, n + fpad, (n + fpad) * ncols
    f = FDesc()
    f.kind, f.axis_stride, f.col_stride, f.b1_stride = kind, 1, n + fpad, (n + fpad) * ncols
    return d, f


# ---- routing without a device ---------------------------------------------------------------------------------------------
def test_desc_layout_is_what_it_was():
    """`half` sits in the old alignment padding: the mirrors of the older tests (no such field) still describe the struct"""
    from test_convolve import Desc as Old
    assert C.sizeof(Desc) == C.sizeof(Old) == 192
    for f in ("no_pairs", "tw4", "tw4_b1", "tw4_n2", "scale"):
        assert getattr(Desc, f).offset == getattr(Old, f).offset, f
    assert Desc.half.offset == Old.no_pairs.offset + 4 and Desc.tw4.offset == 176


def test_half_kernel_routing_without_a_gpu(kl):
    L = kl
    name = lambda d: L.offt_hipk_kernel_name(C.byref(d)).decode()
    for prec in (api.F64, api.F32):
        for n in (64, 128, 256, 512, 1024):
            for inc, outc, half in FLAVOURS:
                d = half_desc(n, prec, 8, 2, inc, outc, half)
                assert L.offt_hipk_has_half(C.byref(d)) == 1, (n, prec, inc, outc, half)
                pairs = prec == api.F32 and n >= 512     # even column count, unit column stride: the column-pair form
                assert name(d) == ("fft_half_panel_k<pairs>" if pairs else "fft_half_panel_k"), (n, prec, inc, outc, half)
                assert L.offt_hipk_keeps_output(C.byref(d)) == 0
                d.ncols = 7                              # an odd column count: one column per lane
                assert name(d) == "fft_half_panel_k" and L.offt_hipk_has_half(C.byref(d)) == 1
            # the other bit on these flavours, both bits, and strided on both sides: no kernel
            for inc, outc, half in [(1, 0, 2), (0, 1, 1), (0, 0, 1), (0, 0, 2), (1, 1, 3), (1, 0, 3)]:
                d = half_desc(n, prec, 8, 2, inc, outc, half)
                assert L.offt_hipk_has_half(C.byref(d)) == 0 and name(d) == "no half-line kernel", (n, inc, outc, half)
        for n in (32, 2048, 48, 67, 63):
            for inc, outc, half in FLAVOURS:
                d = half_desc(n, prec, 8, 2, inc, outc, half)
                assert L.offt_hipk_has_half(C.byref(d)) == 0 and name(d) == "no half-line kernel", (n, prec)
        d = half_desc(256, prec, 8, 2, 1, 1, 1)
        d.in_split = 64                                  # a split line
        assert L.offt_hipk_has_half(C.byref(d)) == 0
        d = half_desc(256, prec, 8, 2, 1, 1, 2)
        d.out_split = 64
        assert L.offt_hipk_has_half(C.byref(d)) == 0
        d = half_desc(256, prec, 8, 2, 1, 1, 1)
        d.real_input = 1
        assert L.offt_hipk_has_half(C.byref(d)) == 0
        d = half_desc(256, prec, 8, 2, 1, 1, 2)
        d.real_input = 2
        assert L.offt_hipk_has_half(C.byref(d)) == 0
        d = half_desc(256, prec, 8, 2, 1, 1, 0)          # half = 0: the usual kernels, named as ever
        assert L.offt_hipk_has_half(C.byref(d)) == 0 and name(d) == "fft_panel_k"
        # the fused convolve takes both bits together or none
        cname = lambda d, f: L.offt_hipk_conv_kernel_name(C.byref(d), C.byref(f)).decode()
        for n in (64, 128, 256, 512, 1024):
            for kind in (0, 1):
                d, f = conv_half_desc(n, prec, 8, 2, 3, kind=kind)
                assert cname(d, f) == "fft_conv_half_panel_k" and L.offt_hipk_conv_has_fused(C.byref(d), C.byref(f)) == 1
                for half in (1, 2):
                    d, f = conv_half_desc(n, prec, 8, 2, half, kind=kind)
                    assert cname(d, f) == "no fused kernel" and L.offt_hipk_conv_has_fused(C.byref(d), C.byref(f)) == 0
                d, f = conv_half_desc(n, prec, 8, 2, 0, kind=kind)
                assert cname(d, f) == "fft_conv_panel_k"
        d, f = conv_half_desc(2048, prec, 8, 2, 3)
        assert cname(d, f) == "no fused kernel"


# ---- CPU tier: the host's schedules on the pad backend ------------------------------------------------------------------
@pytest.fixture()
def pad_cpu(built):
    import cpu_world
    subprocess.check_call(["make", "-s", "-C", ROOT, "tests/libcpubackend_pad.so"])
    orig = cpu_world._cb_lib
    cpu_world._cb_lib = HW.pad_cb_lib
    CB = cpu_world.install(0, 1, p1=1)
    yield CB
    cpu_world.uninstall()
    cpu_world._cb_lib = orig


PRUNED = [(64, 64, 64), (128, 64, 256)]
FALLBACK = [dict(N=[64, 64, 64], params={"S": 1}), dict(N=[64, 64, 64], eq=1), dict(N=[12, 10, 8]), dict(N=[64, 64, 64], r2c=1)]


def _check(res, case):
    for k, e in res.items():
        assert np.isfinite(e) and e <= HW.tol(case), (case, k, e)


@pytest.mark.parametrize("shape", PRUNED)
def test_half_box_pruned_cpu(pad_cpu, shape):
    CB = pad_cpu
    Nx, Ny, Nz = shape
    case = dict(N=list(shape))
    po = HW.make_plan(api, case)
    L = api.lib()
    try:
        assert not api.offt_hip_half_box_pruned(po)
        api.offt_hip_set_half_box(po, True)
        assert api.offt_hip_half_box_pruned(po)
        z0 = CB.cpu_backend_pad_zero_count()
        pr = HW.problem(case["N"], 0)
        CB.cpu_backend_pad_log_reset()
        res, _ = HW.run_plan(api, po, case, HW.Host(), pr)
        _check(res, case)
        assert CB.cpu_backend_pad_zero_count() == z0, "a pruned plan clears nothing"
        fwd = [(Nz, Ny // 2, Nx // 2, 1, 1, 0), (Ny, Nx // 2, Nz, 1, 1, 0), (Nx, Ny, Nz, 1, 1, 0)]
        inv = [(Nx, Ny, Nz, 1, 2, 0), (Ny, Nx // 2, Nz, 1, 2, 0), (Nz, Ny // 2, Nx // 2, 1, 2, 0)]
        conv = fwd[:2] + [(Nx, Ny, Nz, 1, 3, 1)] + inv[1:]
        assert api.offt_hip_convolve_fused(po)
        assert HW.launches(CB) == fwd + inv + conv
        # a backend without the fused launch: the pruned forward, the multiply, the pruned inverse
        L.offt_hip_test_set_backend(CB.cpu_backend_pad_table_unfused(), 0, 1)
        assert not api.offt_hip_convolve_fused(po)
        CB.cpu_backend_pad_log_reset()
        p0 = CB.cpu_backend_pointwise_count()
        res, _ = HW.run_plan(api, po, case, HW.Host(), pr)
        _check(res, case)
        assert HW.launches(CB) == fwd + inv + fwd + inv and CB.cpu_backend_pointwise_count() == p0 + 1
        L.offt_hip_test_set_backend(CB.cpu_backend_pad_table(), 0, 1)
        # switched off again: the ordinary schedule on the ordinary data
        api.offt_hip_set_half_box(po, False)
        assert not api.offt_hip_half_box_pruned(po)
        CB.cpu_backend_pad_log_reset()
        buf = pr["xp"].astype(np.complex128).ravel().copy()
        api.offt_3d_execute_dir(po, buf.ctypes.data, buf.ctypes.data, -1)
        assert [r[4] for r in HW.launches(CB)] == [0, 0, 0] and HW.launches(CB)[0][1:3] == (Ny, Nx)
    finally:
        api.offt_3d_fin(po)


@pytest.mark.parametrize("case", FALLBACK, ids=lambda c: json.dumps(c))
def test_half_box_fallback_cpu(pad_cpu, case):
    CB = pad_cpu
    z0, h0 = CB.cpu_backend_pad_zero_count(), CB.cpu_backend_pad_half_count()
    res, pruned = HW.run_case(api, case, HW.Host())
    assert not pruned
    _check(res, case)
    assert CB.cpu_backend_pad_zero_count() == z0 + 2, "the forward and the convolve clear the padding, the inverse does not"
    assert CB.cpu_backend_pad_half_count() == h0, "no half-line launch on the fallback route"


def test_half_box_f32_cpu(pad_cpu):
    res, pruned = HW.run_case(api, dict(N=[64, 64, 64], f32=1), HW.Host())
    assert pruned
    _check(res, dict(f32=1))


def test_half_box_refusals_cpu(pad_cpu):
    CB = pad_cpu
    L = api.lib()
    case = dict(N=[64, 64, 67])
    po = HW.make_plan(api, case)
    try:
        assert L.offt_hip_set_half_box(po, 1) == -1
        assert "even" in L.offt_hip_last_error().decode() and not api.offt_hip_half_box_pruned(po)
        with pytest.raises(ValueError):
            api.offt_hip_set_half_box(po, True)
        # the plan is unchanged and usable: an ordinary transform
        rng = np.random.default_rng(3)
        x = rng.standard_normal((64, 64, 67)) + 1j * rng.standard_normal((64, 64, 67))
        buf = x.ravel().copy()
        api.offt_3d_execute_dir(po, buf.ctypes.data, buf.ctypes.data, -1)
        c = api.comm_dict(po)
        want = np.fft.fftn(x)
        got = buf[W.out_index(c)].reshape(c["osize"])
        assert np.linalg.norm(got - want) / np.linalg.norm(want) <= 1e-12
    finally:
        api.offt_3d_fin(po)
    po = HW.make_plan(api, dict(N=[16, 16, 16]))
    try:
        L.offt_hip_test_set_backend(CB.cpu_backend_pad_table_nozero(), 0, 1)   # a backend without zero_outside: refused
        assert L.offt_hip_set_half_box(po, 1) == -1 and "padding" in L.offt_hip_last_error().decode()
        L.offt_hip_test_set_backend(CB.cpu_backend_pad_table(), 0, 1)
        assert L.offt_hip_set_half_box(po, 1) == 0
    finally:
        api.offt_3d_fin(po)


def _gloo(size, cases, tmp_path):
    subprocess.check_call(["make", "-s", "-C", ROOT, "tests/libcpubackend_pad.so"])
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    procs = []
    for r in range(size):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(size), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_half_world.py"), "gloo", json.dumps(cases), str(tmp_path)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = [p.communicate(timeout=900)[0].decode() for p in procs]
    for r, p in enumerate(procs):
        assert p.returncode == 0, f"rank {r}:\n{outs[r][-3000:]}"
    for r in range(size):
        for rec in json.load(open(tmp_path / f"gloo_rank{r}.json")):
            assert not rec["pruned"] and rec["zeroed"] == 2, rec
            _check(rec["res"], rec["case"])


def test_half_box_gloo_world2(built, tmp_path):
    _gloo(2, [dict(N=[16, 16, 16]), dict(N=[16, 12, 10])], tmp_path)                                     # slab


def test_half_box_gloo_world4(built, tmp_path):
    _gloo(4, [dict(N=[16, 16, 16], params={"P1": 2}), dict(N=[16, 12, 10], params={"P1": 2}),           # pencil
              dict(N=[16, 16, 16]), dict(N=[16, 12, 10])], tmp_path)                                     # slab


def test_free_space_claim_on_the_cpu():
    """the claim test_half_box_free_space rests on: with the p and the width used there, the periodic convolution on the
    32^3 grid differs from the free-space one by far more than the tolerance, and the zero-padded 64^3 one does not"""
    g, p, want = _free_space_problem()
    n = 32
    d = np.zeros((n, n, n))
    d[p] = 1.0
    per = np.fft.ifftn(np.fft.fftn(d) * np.fft.fftn(g[:n, :n, :n])).real   # (g's support lies inside [0,32)^3)
    assert np.linalg.norm(per - want) / np.linalg.norm(want) > 0.1
    d2 = np.zeros((64, 64, 64))
    d2[p] = 1.0
    free = np.fft.ifftn(np.fft.fftn(d2) * np.fft.fftn(g)).real[:n, :n, :n]
    assert np.linalg.norm(free - want) / np.linalg.norm(want) <= 1e-12


def _free_space_problem():
    """g: a Gaussian of width sigma = 3 centred at (8,8,8) of the 64^3 grid and cut to exactly zero beyond 8 cells from its
    centre along any axis, so its support [0,16]^3 and every shift of it by p < 32 stay on the grid: nothing wraps.  A delta
    at p = (20, 3, 17) puts the peak at p + 8 = (28, 11, 25); in the 32^3 box the free-space answer is g shifted by p and cut
    at the box faces.  On a periodic 32^3 grid the cells x = 32 ... 36 of the shifted kernel come back at x = 0 ... 4 -- the
    first of them 4 cells from the peak, exp(-16/18) = 0.41 of it -- so the periodic route is wrong by tens of per cent."""
    n = 64
    ax = np.arange(n) - 8.0
    cut = np.abs(ax) > 8
    g = np.exp(-(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2) / 18.0)
    g[cut[:, None, None] | cut[None, :, None] | cut[None, None, :]] = 0.0
    p = (20, 3, 17)
    want = np.roll(g, p, axis=(0, 1, 2))[:32, :32, :32].copy()   # (index k of g moves to k + p <= 16 + 31: no wrap on the 64-grid)
    return g, p, want


# ---- GPU tier ----------------------------------------------------------------------------------------------------------
def _index(d, side, nb1, ncols, n):
    ax, col, b1 = ((d.in_axis_stride, d.in_col_stride, d.in_b1_stride) if side == "in" else
                   (d.out_axis_stride, d.out_col_stride, d.out_b1_stride))
    return np.arange(nb1)[:, None, None] * b1 + np.arange(ncols)[None, :, None] * col + np.arange(n)[None, None, :] * ax


@pytest.mark.gpu
@pytest.mark.parametrize("n", [64, 128, 256, 512, 1024])
def test_half_random_descriptors(kl, n):
    import torch
    L = kl
    rng = np.random.default_rng(1700 + n)
    SENT = 8
    for prec in (api.F64, api.F32):
        assert L.offt_hipk_prepare(n, prec) == 0
        ft, ct = (np.float64, np.complex128) if prec == api.F64 else (np.float32, np.complex64)
        for inc, outc, half in FLAVOURS:
            for ncols in (3, 13, 21, 18):
                nb1 = int(rng.integers(2, 4))
                pad = int(rng.integers(1, 3))
                if ncols == 18:   # an even count with even pitches: single precision takes the column-pair form where it has one
                    pad = 2
                direction = int(rng.choice([-1, 1]))
                scale = float(rng.choice([0.5, 1.0 / n, 3.0]))
                d = half_desc(n, prec, ncols, nb1, inc, outc, half, pad=pad, direction=direction, scale=scale)
                if ncols == 18:
                    pairs = prec == api.F32 and n >= 512
                    assert L.offt_hipk_kernel_name(C.byref(d)).decode() == ("fft_half_panel_k<pairs>" if pairs else "fft_half_panel_k")
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
                assert err <= (1e-12 if prec == api.F64 else 1e-5), (n, prec, inc, outc, half, ncols, err)
    # a bit no kernel implements fails, it does not run the full line
    d = half_desc(n, api.F64, 4, 1, 0, 0, 1)
    buf = torch.zeros(2 * (4 * n + 64), dtype=torch.float64, device="cuda")
    assert L.offt_hipk_fft_pass(C.byref(d), buf.data_ptr(), buf.data_ptr(), None) == -1
    assert b"half" in L.offt_hipk_last_error()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [64, 128, 256, 512, 1024])
def test_half_random_fused_conv_descriptors(kl, n):
    import torch
    L = kl
    rng = np.random.default_rng(2300 + n)
    SENT = 8
    for prec in (api.F64, api.F32):
        assert L.offt_hipk_prepare(n, prec) == 0
        ft, ct = (np.float64, np.complex128) if prec == api.F64 else (np.float32, np.complex64)
        for kind in (0, 1):
            for ncols in (3, 13, 21):
                nb1 = int(rng.integers(2, 4))
                pad, fpad = int(rng.integers(1, 3)), int(rng.integers(0, 3))
                scale = float(rng.choice([0.5, 1.0 / n, 3.0]))
                d, f = conv_half_desc(n, prec, ncols, nb1, 3, pad=pad, fpad=fpad, kind=kind, scale=scale)
                ii = _index(d, "in", nb1, ncols, n)
                fi = np.arange(nb1)[:, None, None] * f.b1_stride + np.arange(ncols)[None, :, None] * f.col_stride + np.arange(n)[None, None, :]
                nin, nf = int(ii.max()) + 1 + pad, int(fi.max()) + 1 + 16
                lines = (rng.standard_normal((nb1, ncols, n)) + 1j * rng.standard_normal((nb1, ncols, n))).astype(ct)
                lines[:, :, n // 2:] = 0
                h = (rng.standard_normal(nf) + 1j * rng.standard_normal(nf)) if kind else rng.standard_normal(nf)
                H = h[fi].astype(ct if kind else ft).astype(np.complex128)
                want = np.fft.ifft(H * np.fft.fft(lines.astype(np.complex128), axis=2), axis=2)[:, :, :n // 2] * n * scale
                buf = np.full(nin + 2 * SENT, 7.0 + 7.0j, dtype=ct)
                buf[SENT:SENT + nin] = (rng.standard_normal(nin) + 1j * rng.standard_normal(nin)).astype(ct)
                buf[SENT + ii.ravel()] = lines.ravel()
                buf[SENT + ii[:, :, n // 2:].ravel()] = np.nan + 1j * np.nan   # neither read nor written
                dx = torch.from_numpy(buf.view(ft).copy()).cuda()
                dh = torch.from_numpy((h.astype(ct).view(ft) if kind else h.astype(ft)).copy()).cuda()
                torch.cuda.synchronize()
                rc = L.offt_hipk_conv_pass(C.byref(d), C.byref(f), dh.data_ptr(), dx.data_ptr() + SENT * buf.itemsize, None)
                assert rc == 0, L.offt_hipk_last_error()
                torch.cuda.synchronize()
                got = dx.cpu().numpy().view(ct)
                written = np.zeros(nin + 2 * SENT, dtype=bool)
                written[SENT + ii[:, :, :n // 2].ravel()] = True
                assert np.array_equal(got[~written].view(ft), buf[~written].view(ft), equal_nan=True), (n, prec, kind, ncols)
                g = got[SENT + ii[:, :, :n // 2]].astype(np.complex128)
                err = np.linalg.norm(g - want) / np.linalg.norm(want)
                assert np.isfinite(err) and err <= (1e-12 if prec == api.F64 else 1e-5), (n, prec, kind, ncols, err)
        d, f = conv_half_desc(n, prec, 4, 1, 1)
        assert L.offt_hipk_conv_pass(C.byref(d), C.byref(f), None, None, None) == -1


@pytest.mark.gpu
def test_zero_outside_gpu(kl):
    import torch
    L = kl
    rng = np.random.default_rng(5)
    for prec, real in ((api.F64, 0), (api.F32, 0), (api.F64, 1), (api.F32, 1)):
        ft = np.float64 if prec == api.F64 else np.float32
        spe = 1 if real else 2
        for (n0, n1, n2), (k0, k1, k2), rowpad, off in (((5, 6, 14), (2, 3, 7), 0, 0), ((4, 3, 9), (4, 1, 5), 1, 0), ((3, 5, 8), (0, 5, 3), 2, 1),
                                                          ((2, 2, 300), (1, 2, 150), 0, 0)):
            s1 = n2 + rowpad
            s0 = s1 * n1 + rowpad
            tot = (s0 * n0 + 8) * spe
            a = rng.standard_normal(tot + 16).astype(ft)
            t = torch.from_numpy(a.copy()).cuda()
            torch.cuda.synchronize()
            rc = L.offt_hipk_zero_outside(t.data_ptr() + off * spe * a.itemsize, prec | (0x100 if real else 0), n0, n1, n2, k0, k1, k2, s0, s1, 1, None)
            assert rc == 0, L.offt_hipk_last_error()
            torch.cuda.synchronize()
            want = a.copy()
            for i0 in range(n0):
                for i1 in range(n1):
                    lo = k2 if (i0 < k0 and i1 < k1) else 0
                    b = (off + i0 * s0 + i1 * s1) * spe
                    want[b + lo * spe:b + n2 * spe] = 0
            assert np.array_equal(t.cpu().numpy(), want), (prec, real, n0, n1, n2)


PLAN_CASES = [dict(N=list(s)) for s in PRUNED] + FALLBACK + [dict(N=[48, 40, 30])]


@pytest.mark.gpu
@pytest.mark.parametrize("case", PLAN_CASES, ids=lambda c: json.dumps(c))
@pytest.mark.parametrize("f32", [0, 1])
def test_half_box_one_rank_gpu(built, case, f32):
    import torch
    torch.cuda.set_device(0)
    case = dict(case, f32=f32)
    want_pruned = tuple(case["N"]) in PRUNED and len(case) == 2
    dev = HW.Gpu(torch)
    po = HW.make_plan(api, case)
    try:
        api.offt_hip_set_half_box(po, True)
        assert api.offt_hip_half_box_pruned(po) == want_pruned, case
        pr = HW.problem(case["N"], case.get("r2c"))
        res, out_on = HW.run_plan(api, po, case, dev, pr)
        for k, e in res.items():
            print(case, k, e)
        _check(res, case)
        if want_pruned and not f32:
            # the same plan with the option off on explicitly zeroed input: only the order of operations on exact zeros differs
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
def test_half_box_free_space(built):
    """a delta at p in the 32^3 box, convolved on a 64^3 half-box plan with the plan's own transform of a Gaussian that does
    not wrap: inside the box, g shifted by p with no periodic image.  p = (28, 3, 17) and sigma = 3 make the periodic
    32^3 route differ by > 1e-3 (test_free_space_claim_on_the_cpu checks that with numpy)."""
    import torch
    torch.cuda.set_device(0)
    g, p, want = _free_space_problem()
    N = (64, 64, 64)
    po = api.offt_3d_init(*N)
    L = api.lib()
    try:
        c = api.comm_dict(po)
        case = dict(N=list(N))
        gbuf, _ = W.local_arrays(c, api.local_elems(po), case, g.astype(np.complex128), np.zeros((1, 1, 1)))
        dh = torch.from_numpy(gbuf.view(np.float64).copy()).cuda()
        api.offt_3d_execute(po, dh.data_ptr(), dh.data_ptr())   # H = F(g): the full transform, option off
        api.offt_hip_set_half_box(po, True)
        assert api.offt_hip_half_box_pruned(po) and api.offt_hip_convolve_fused(po)
        delta = np.zeros(N)
        delta[p] = 1.0
        dbuf = HW.poisoned_input(c, api.local_elems(po), case, delta.astype(np.complex128))
        dd = torch.from_numpy(dbuf.view(np.float64).copy()).cuda()
        L.offt_hip_set_output_scale(po, 1.0 / np.prod(N))
        api.offt_hip_execute_convolve(po, dd.data_ptr(), dh.data_ptr(), api.FILTER_COMPLEX)
        torch.cuda.synchronize()
        full = np.zeros(N)
        full[:32, :32, :32] = want
        err = HW.box_err(c, case, dd.cpu().numpy().view(np.complex128), full.astype(np.complex128))
        print("free space", err)
        assert err <= 1e-12, err
    finally:
        api.offt_3d_fin(po)


@pytest.mark.gpu
def test_half_box_thread_world(built, tmp_path):
    env = dict(os.environ, GPU_MAX_HW_QUEUES="24")
    cases = [dict(N=[16, 16, 16], params={})]
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_half_world.py"), "2", json.dumps(cases), str(tmp_path)],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert p.returncode == 0, p.stdout.decode()[-4000:]
    res = json.load(open(tmp_path / "summary.json"))
    assert len(res) == len(cases)
    for r in res:
        assert r["rel"] <= r["tol"], r
