"""Spectral convolution: offt_hip_execute_convolve (forward, filter, inverse in one call).

  * kernel routing of the fused launch without a device (offt_hipk_conv_kernel_name);
  * the host's schedules on the CPU convolution backend (tests/cpu_backend_conv.c): every single-rank layout, complex and
    r2c plans, real and complex filters, gloo worlds of 2 and 4 ranks (slab and pencil), refusals;
  * -m gpu: random fused descriptors against numpy with a sentinel, every layout on one rank, the routes, a convolution
    with a delta, a Poisson solve, thread-rank worlds on the one GPU, and 1024^3 / 512^3 against the caller's route."""
import ctypes as C
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import _conv_world as W
from offt_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Desc(C.Structure):
    """offt_pass_desc (offt_amd/csrc/offt_hipk.h), field by field"""
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
                ("real_input", C.c_int), ("out_keep", C.c_int), ("no_pairs", C.c_int), ("tw4", C.c_void_p), ("tw4_b1", C.c_int), ("tw4_n2", C.c_int)]


class FDesc(C.Structure):
    """offt_filter_desc (offt_amd/csrc/offt_hipk.h)"""
    _fields_ = [("kind", C.c_int), ("axis_stride", C.c_longlong), ("col_stride", C.c_longlong), ("b1_stride", C.c_longlong),
                ("b2_stride", C.c_longlong)]


def conv_desc(n, prec, ncols, nb1, pad=0, fpad=0, kind=0, scale=1.0):
    """contiguous lines (rows of n + pad elements), the filter in rows of n + fpad"""
    d = Desc()
    d.n, d.precision, d.direction, d.ncols, d.nb1, d.nb2 = n, prec, -1, ncols, nb1, 1
    d.in_axis_stride, d.in_col_stride = 1, n + pad
    d.in_b1_stride = (n + pad) * ncols + pad
    d.in_contig, d.out_contig, d.variant, d.scale = 1, 1, -1, scale
    d.out_axis_stride, d.out_col_stride, d.out_b1_stride = 1, n + fpad, (n + fpad) * ncols
    f = FDesc()
    f.kind, f.axis_stride, f.col_stride, f.b1_stride = kind, 1, n + fpad, (n + fpad) * ncols
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


def test_conv_kernel_routing_without_a_gpu(kl):
    L = kl
    name = lambda d, f: L.offt_hipk_conv_kernel_name(C.byref(d), C.byref(f)).decode()
    for prec in (api.F64, api.F32):
        for n in (64, 128, 256, 512, 1024):
            for kind in (0, 1):
                d, f = conv_desc(n, prec, 8, 2, kind=kind)
                assert name(d, f) == "fft_conv_panel_k", (n, prec, kind)
                assert L.offt_hipk_conv_has_fused(C.byref(d), C.byref(f)) == 1
        for n in (48, 1000, 67, 2048, 8192, 32):        # mixed radix, Bluestein, longer and shorter than the fused range
            d, f = conv_desc(n, prec, 8, 2)
            assert name(d, f) == "no fused kernel", (n, prec)
        d, f = conv_desc(1024, prec, 8, 2)
        f.axis_stride = 8                                # strided filter (the rotated x-y-z layout)
        assert name(d, f) == "no fused kernel"
        d, f = conv_desc(1024, prec, 8, 2)
        d.in_contig, d.in_axis_stride, d.in_col_stride = 0, 8, 1  # strided lines
        assert name(d, f) == "no fused kernel"
        d, f = conv_desc(1024, prec, 8, 2)
        d.in_split = 256                                 # a split line (multi-rank pass)
        assert name(d, f) == "no fused kernel"
        d, f = conv_desc(1024, prec, 8, 2, kind=2)       # no such filter kind
        assert name(d, f) == "no fused kernel"


# ---- CPU tier: the host's schedules on the CPU convolution backend ------------------------------------------------------
@pytest.fixture()
def conv_cpu(built):
    import cpu_world
    subprocess.check_call(["make", "-s", "-C", ROOT, "tests/libcpubackend_conv.so"])
    orig = cpu_world._cb_lib
    cpu_world._cb_lib = W.conv_cb_lib
    CB = cpu_world.install(0, 1, p1=1)
    yield CB
    cpu_world.uninstall()
    cpu_world._cb_lib = orig


LAYOUTS = [dict(), dict(params={"S": 1}), dict(eq=1)]


# (the y-z-x layout needs Nx == Ny)
CPU_CASES = [(shape, lay) for shape in [(64, 8, 16), (64, 64, 8), (12, 10, 9), (128, 6, 5)] for lay in LAYOUTS
             if not lay.get("eq") or shape[0] == shape[1]]


@pytest.mark.parametrize("shape,lay", CPU_CASES)
@pytest.mark.parametrize("r2c", [0, 1])
def test_conv_single_rank_cpu(conv_cpu, shape, lay, r2c):
    CB = conv_cpu
    for cplx in (0, 1):
        case = dict(N=list(shape), r2c=r2c, cplx=cplx, **lay)
        k0, p0 = CB.cpu_backend_conv_count(), CB.cpu_backend_pointwise_count()
        err, fused, _ = W.cpu_convolve(api, case)
        assert err <= 1e-12, (case, err)
        # the fused route launches conv_pass, the unfused one the pointwise multiply: exactly one of them ran
        ran_fused = CB.cpu_backend_conv_count() > k0
        assert ran_fused == fused and (CB.cpu_backend_pointwise_count() > p0) == (not fused), case
    if not lay and shape[0] in (64, 128):
        assert fused, "power-of-two x lines of the z-y-x layout take the fused route"


def test_conv_single_rank_cpu_f32_and_unfused_table(conv_cpu):
    import cpu_world
    err, fused, _ = W.cpu_convolve(api, dict(N=[64, 8, 16], f32=1, cplx=1))
    assert fused and err <= 2e-5, err
    # a backend without conv_pass: the same result through the unfused route
    L = api.lib()
    L.offt_hip_test_set_backend(conv_cpu.cpu_backend_conv_table_unfused(), 0, 1)
    err, fused, _ = W.cpu_convolve(api, dict(N=[64, 8, 16], cplx=1))
    assert not fused and err <= 1e-12, err


def test_conv_refusals_cpu(conv_cpu):
    L = api.lib()
    po = api.offt_3d_init(64, 8, 16)
    try:
        buf = np.zeros(api.local_elems(po), dtype=np.complex128)
        filt = np.ones(api.local_elems(po), dtype=np.complex128)
        assert L.offt_hip_execute_convolve(po, buf.ctypes.data, None, api.FILTER_REAL) == -1
        assert "filter" in L.offt_hip_last_error().decode() and po.contents.t[api.ALL] >= 99999999.0
        assert L.offt_hip_execute_convolve(po, buf.ctypes.data, filt.ctypes.data, 2) == -1
        assert "filter_kind" in L.offt_hip_last_error().decode()
        assert L.offt_hip_execute_convolve(po, buf.ctypes.data, filt.ctypes.data, -1) == -1
        # a backend without the pointwise multiply (tests/cpu_backend.c's table): refused
        L.offt_hip_test_set_backend(conv_cpu.cpu_backend_conv_table_none(), 0, 1)
        assert L.offt_hip_execute_convolve(po, buf.ctypes.data, filt.ctypes.data, api.FILTER_COMPLEX) == -1
        assert "pointwise" in L.offt_hip_last_error().decode()
        L.offt_hip_test_set_backend(conv_cpu.cpu_backend_conv_table(), 0, 1)
        assert L.offt_hip_execute_convolve(po, buf.ctypes.data, filt.ctypes.data, api.FILTER_COMPLEX) == 0
    finally:
        api.offt_3d_fin(po)


def _gloo(size, cases, tmp_path):
    subprocess.check_call(["make", "-s", "-C", ROOT, "tests/libcpubackend_conv.so"])
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    procs = []
    for r in range(size):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(size), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_conv_world.py"), "gloo", json.dumps(cases), str(tmp_path)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = [p.communicate(timeout=900)[0].decode() for p in procs]
    for r, p in enumerate(procs):
        assert p.returncode == 0, f"rank {r}:\n{outs[r][-3000:]}"
    for r in range(size):
        for rec in json.load(open(tmp_path / f"gloo_rank{r}.json")):
            assert rec["rel"] <= rec["tol"], (r, rec)
            assert not rec["fused"] and rec["pointwise"] == 1, rec   # several ranks: always the unfused composition


def test_conv_gloo_world2(built, tmp_path):
    _gloo(2, [dict(N=[16, 16, 16]), dict(N=[16, 12, 10], r2c=1, cplx=1), dict(N=[8, 8, 8], params={"S": 1}, cplx=1),
              dict(N=[16, 16, 8], eq=1, r2c=1)], tmp_path)


def test_conv_gloo_world4(built, tmp_path):
    _gloo(4, [dict(N=[16, 16, 16], params={"P1": 2}), dict(N=[16, 16, 16], params={"P1": 2}, r2c=1, cplx=1),
              dict(N=[16, 16, 32]), dict(N=[16, 12, 10], r2c=1)], tmp_path)


# ---- GPU tier ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [64, 128, 256, 512, 1024])
def test_conv_random_fused_descriptors(kl, n):
    import torch
    L = kl
    rng = np.random.default_rng(900 + n)
    for prec in (api.F64, api.F32):
        assert L.offt_hipk_prepare(n, prec) == 0
        ft, ct = (np.float64, np.complex128) if prec == api.F64 else (np.float32, np.complex64)
        for kind in (0, 1):
            ncols = int(rng.choice([3, 13, 21]))      # never a whole number of panels
            nb1 = int(rng.integers(2, 4))
            pad, fpad = int(rng.integers(0, 3)), int(rng.integers(0, 3))
            scale = float(rng.choice([0.5, 1.0 / n, 3.0]))
            d, f = conv_desc(n, prec, ncols, nb1, pad=pad, fpad=fpad, kind=kind, scale=scale)
            nin = d.in_b1_stride * nb1 + 16
            nf = f.b1_stride * nb1 + 16
            x = (rng.standard_normal(nin) + 1j * rng.standard_normal(nin)).astype(ct)
            h = (rng.standard_normal(nf) + 1j * rng.standard_normal(nf)) if kind else rng.standard_normal(nf)
            want = x.astype(np.complex128).copy()
            for b1 in range(nb1):
                for c in range(ncols):
                    i = b1 * d.in_b1_stride + c * d.in_col_stride
                    fo = b1 * f.b1_stride + c * f.col_stride
                    H = h[fo:fo + n].astype(ct if kind else ft).astype(np.complex128)
                    want[i:i + n] = np.fft.ifft(H * np.fft.fft(want[i:i + n])) * n * scale
            SENT = 8  # sentinel elements on either side of the array
            buf = np.full(nin + 2 * SENT, 7.0 + 7.0j, dtype=ct)
            buf[SENT:SENT + nin] = x
            dx = torch.from_numpy(buf.view(ft).copy()).cuda()
            dh = torch.from_numpy((h.astype(ct).view(ft) if kind else h.astype(ft)).copy()).cuda()
            torch.cuda.synchronize()
            rc = L.offt_hipk_conv_pass(C.byref(d), C.byref(f), dh.data_ptr(), dx.data_ptr() + SENT * buf.itemsize, None)
            assert rc == 0, L.offt_hipk_last_error()
            torch.cuda.synchronize()
            got = dx.cpu().numpy().view(ct)
            assert np.all(got[:SENT] == buf[:SENT]) and np.all(got[SENT + nin:] == buf[SENT + nin:]), "sentinel overwritten"
            mid = got[SENT:SENT + nin].astype(np.complex128)
            lines = np.zeros(nin, dtype=bool)
            for b1 in range(nb1):
                for c in range(ncols):
                    i = b1 * d.in_b1_stride + c * d.in_col_stride
                    lines[i:i + n] = True
            assert np.array_equal(mid[~lines], x[~lines].astype(np.complex128)), "padding between lines written"
            err = np.linalg.norm(mid[lines] - want[lines]) / np.linalg.norm(want[lines])
            assert err <= (1e-12 if prec == api.F64 else 1e-5), (n, prec, kind, err)


def _gpu_one_rank(case, rotate=None):
    import torch
    if rotate is not None:
        os.environ["OFFT_ROTATE"] = str(rotate)
    try:
        po = api.offt_3d_init(*case["N"], custom_params=api.make_params(**case.get("params", {})), is_equalxy=case.get("eq", 0),
                              precision=api.F32 if case.get("f32") else api.F64, is_r2c=int(case.get("r2c", 0)))
    finally:
        os.environ.pop("OFFT_ROTATE", None)
    try:
        err, _ = W.gpu_rank(api.lib(), api, torch, po, case)
        return err, api.offt_hip_convolve_fused(po)
    finally:
        api.offt_3d_fin(po)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(32, 32, 32), (64, 64, 64), (128, 128, 128), (48, 40, 30), (64, 64, 67)])
def test_conv_one_rank_every_layout(built, shape):
    import torch
    torch.cuda.set_device(0)
    lays = [(dict(), None), (dict(params={"S": 1}), 1), (dict(params={"S": 1}), 0)]
    if shape[0] == shape[1]:
        lays += [(dict(eq=1), 1), (dict(eq=1), 0)]
    for f32 in (0, 1):
        for r2c in (0, 1):
            for lay, rot in lays:
                case = dict(N=list(shape), f32=f32, r2c=r2c, cplx=(r2c + f32) % 2, **lay)
                err, _ = _gpu_one_rank(case, rot)
                assert err <= W.tol(case), (case, rot, err)


@pytest.mark.gpu
def test_conv_routes(built):
    import torch
    torch.cuda.set_device(0)
    # the fused launch is the x pass of the z-y-x layout: its route depends on the x length only
    for shape, want in (((64, 64, 64), True), ((128, 128, 128), True), ((64, 64, 67), True), ((67, 64, 64), False),
                        ((67, 67, 67), False), ((48, 40, 30), False)):
        po = api.offt_3d_init(*shape)
        try:
            assert api.offt_hip_convolve_fused(po) == want, shape
        finally:
            api.offt_3d_fin(po)


@pytest.mark.gpu
@pytest.mark.parametrize("r2c", [0, 1])
def test_conv_delta_gives_the_shifted_kernel(built, r2c):
    """H = the plan's own forward transform of a Gaussian g; a delta at p convolved with scale 1/N is g shifted to p"""
    import torch
    torch.cuda.set_device(0)
    N = (64, 64, 64)
    po = api.offt_3d_init(*N, is_r2c=r2c)
    L = api.lib()
    try:
        c = api.comm_dict(po)
        ax = [np.minimum(np.arange(n), n - np.arange(n)) for n in N]
        g = np.exp(-(ax[0][:, None, None] ** 2 + ax[1][None, :, None] ** 2 + ax[2][None, None, :] ** 2) / 18.0)
        case = dict(N=list(N), r2c=r2c, cplx=1)
        gbuf, _ = W.local_arrays(c, api.local_elems(po), case, g.astype(np.complex128), np.zeros((1, 1, 1)))
        dh = torch.from_numpy(gbuf.view(np.float64).copy()).cuda()
        api.offt_3d_execute(po, dh.data_ptr(), dh.data_ptr())         # H = F(g), in the forward's output layout
        p = (5, 17, 40)
        delta = np.zeros(N)
        delta[p] = 1.0
        dbuf, _ = W.local_arrays(c, api.local_elems(po), case, delta.astype(np.complex128), np.zeros((1, 1, 1)))
        dd = torch.from_numpy(dbuf.view(np.float64).copy()).cuda()
        L.offt_hip_set_output_scale(po, 1.0 / np.prod(N))
        api.offt_hip_execute_convolve(po, dd.data_ptr(), dh.data_ptr(), api.FILTER_COMPLEX)
        torch.cuda.synchronize()
        want = np.roll(g, p, axis=(0, 1, 2))
        err = W.check(c, case, dd.cpu().numpy().view(np.complex128), want)
        assert err <= 1e-12, err
        t = (C.c_double * 3)()
        L.offt_hip_last_pass_seconds(po, t)
        assert list(t) == [0.0, 0.0, 0.0] and L.offt_hip_last_device_seconds(po) > 0
    finally:
        api.offt_3d_fin(po)


@pytest.mark.gpu
def test_conv_refusals_gpu(built):
    import torch
    torch.cuda.set_device(0)
    po = api.offt_3d_init(32, 32, 32)
    L = api.lib()
    try:
        d = torch.zeros(2 * api.local_elems(po), dtype=torch.float64, device="cuda")
        hf = np.ones(api.local_elems(po))
        assert L.offt_hip_execute_convolve(po, d.data_ptr(), hf.ctypes.data, api.FILTER_REAL) == -1
        assert "device memory" in L.offt_hip_last_error().decode()
        hd = np.zeros(2 * api.local_elems(po))
        df = torch.ones(api.local_elems(po), dtype=torch.float64, device="cuda")
        assert L.offt_hip_execute_convolve(po, hd.ctypes.data, df.data_ptr(), api.FILTER_REAL) == -1
        assert L.offt_hip_execute_convolve(po, d.data_ptr(), None, api.FILTER_REAL) == -1
        assert L.offt_hip_execute_convolve(po, d.data_ptr(), df.data_ptr(), 5) == -1
        assert L.offt_hip_execute_convolve(po, d.data_ptr(), df.data_ptr(), api.FILTER_REAL) == 0
    finally:
        api.offt_3d_fin(po)


@pytest.mark.gpu
def test_conv_poisson_256(built):
    """H = -1/|k|^2 (0 at k = 0) on a sum of sine modes: the analytic solution of the periodic Poisson equation"""
    import torch
    torch.cuda.set_device(0)
    n = 256
    po = api.offt_3d_init(n, n, n)
    L = api.lib()
    try:
        c = api.comm_dict(po)
        k = np.fft.fftfreq(n, 1.0 / n) * 2 * np.pi / (2 * np.pi)   # integer wave numbers on a 2 pi box
        modes = [((1, 2, 3), 1.0), ((5, 0, 7), 0.5), ((0, 11, 2), -0.25)]
        xs = np.arange(n) * 2 * np.pi / n
        td = torch.float64
        X = torch.tensor(xs, dtype=td, device="cuda")
        f = torch.zeros((n, n, n), dtype=td, device="cuda")
        u = torch.zeros((n, n, n), dtype=td, device="cuda")
        for (a, b, cc), amp in modes:
            m = amp * torch.sin(a * X[:, None, None] + b * X[None, :, None] + cc * X[None, None, :])
            f += m
            u -= m / float(a * a + b * b + cc * cc)                   # lap u = f
        kk = torch.tensor(k, dtype=td, device="cuda")
        k2 = kk[:, None, None] ** 2 + kk[None, :, None] ** 2 + kk[None, None, :] ** 2
        Hg = torch.where(k2 > 0, -1.0 / torch.where(k2 > 0, k2, torch.ones_like(k2)), torch.zeros_like(k2))
        s0, s1, s2 = c["istride"]
        data = torch.zeros(2 * api.local_elems(po), dtype=td, device="cuda")
        torch.as_strided(data, (n, n, n), (2 * s0, 2 * s1, 2 * s2)).copy_(f)
        o0, o1, o2 = c["ostride"]
        filt = torch.zeros(api.local_elems(po), dtype=td, device="cuda")
        torch.as_strided(filt, (n, n, n), (o0, o1, o2)).copy_(Hg)
        del Hg, k2
        L.offt_hip_set_output_scale(po, 1.0 / n ** 3)
        api.offt_hip_execute_convolve(po, data.data_ptr(), filt.data_ptr(), api.FILTER_REAL)
        torch.cuda.synchronize()
        got = torch.as_strided(data, (n, n, n), (2 * s0, 2 * s1, 2 * s2))
        err = float((got - u).norm() / u.norm())
        assert err <= 1e-12, err
        assert float(torch.as_strided(data, (n, n, n), (2 * s0, 2 * s1, 2 * s2), 1).abs().max()) < 1e-12
    finally:
        api.offt_3d_fin(po)


def _thread_world(size, cases, tmp_path):
    env = dict(os.environ, GPU_MAX_HW_QUEUES="24")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_conv_world.py"), str(size), json.dumps(cases), str(tmp_path)],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-4000:]
    res = json.load(open(tmp_path / "summary.json"))
    assert len(res) == len(cases)
    for r in res:
        assert r["rel"] <= r["tol"], r


@pytest.mark.gpu
def test_conv_thread_worlds(built, tmp_path):
    _thread_world(2, [dict(N=[16, 16, 16], params={}), dict(N=[32, 16, 64], params={}, r2c=1, cplx=1, p2p=1),
                      dict(N=[16, 8, 18], params={}, f32=1, r2c=1)], tmp_path)
    _thread_world(3, [dict(N=[12, 9, 16], params={}, cplx=1), dict(N=[12, 12, 20], params={}, r2c=1, p2p=1)], tmp_path)
    _thread_world(8, [dict(N=[16, 16, 16], params={"P1": 2}, r2c=1), dict(N=[16, 16, 32], params={"P1": 4}, cplx=1, p2p=1),
                      dict(N=[16, 16, 32], params={}, f32=1)], tmp_path)


def _full_size_vs_callers_route(shape, r2c):
    """the fused convolve against forward + torch multiply + inverse, on the device (real filter, scale 1/N)"""
    import torch
    L = api.lib()
    po = api.offt_3d_init(*shape, is_r2c=r2c)
    try:
        c = api.comm_dict(po)
        n = 2 * api.local_elems(po)
        a = torch.empty(n, dtype=torch.float64, device="cuda")
        assert L.offt_hip_fill_input(po, a.data_ptr(), 1) == 0
        b = a.clone()
        g = torch.Generator(device="cuda").manual_seed(3)
        H = torch.rand(api.local_elems(po), dtype=torch.float64, device="cuda", generator=g)
        L.offt_hip_set_output_scale(po, 1.0 / float(np.prod(shape)))
        api.offt_hip_execute_convolve(po, a.data_ptr(), H.data_ptr(), api.FILTER_REAL)
        fused = api.offt_hip_convolve_fused(po)
        L.offt_hip_set_output_scale(po, 1.0)
        api.offt_3d_execute(po, b.data_ptr(), b.data_ptr())
        o0, o1, o2 = c["ostride"]
        osz = c["osize"]
        bv = torch.as_strided(b, tuple(osz) + (2,), (2 * o0, 2 * o1, 2 * o2, 1))
        bv.mul_(torch.as_strided(H, tuple(osz) + (1,), (o0, o1, o2, 0)))
        L.offt_hip_set_output_scale(po, 1.0 / float(np.prod(shape)))
        api.offt_3d_execute_dir(po, b.data_ptr(), b.data_ptr(), +1)
        torch.cuda.synchronize()
        s0, s1, s2 = c["istride"]
        sh, st = (tuple(shape), (2 * s0, 2 * s1, 1)) if r2c else (tuple(shape) + (2,), (2 * s0, 2 * s1, 2 * s2, 1))
        va, vb = torch.as_strided(a, sh, st), torch.as_strided(b, sh, st)
        num = den = 0.0
        for x0 in range(0, shape[0], 64):
            num += float((va[x0:x0 + 64] - vb[x0:x0 + 64]).square().sum())
            den += float(vb[x0:x0 + 64].square().sum())
        return (num / den) ** 0.5, fused
    finally:
        api.offt_3d_fin(po)


@pytest.mark.gpu
def test_conv_full_size(built):
    import torch
    torch.cuda.set_device(0)
    err, fused = _full_size_vs_callers_route((1024, 1024, 1024), 0)
    assert fused and err <= 1e-13, (err, fused)
    torch.cuda.empty_cache()
    err, _ = _full_size_vs_callers_route((512, 512, 512), 1)
    assert err <= 1e-13, err
