"""The complex-to-real inverse of real-input (r2c) plans: offt_3d_execute_dir(po, ..., +1) on a plan made with is_r2c = 1.

  * kernel routing of real-output pass descriptors (offt_pass_desc::real_input = 2), without a device;
  * -m gpu, descriptor level: random real_input = 2 descriptors (strided / contiguous input, even / uneven / table splits
    on the input side, scale, f64 / f32, non-Hermitian input) against numpy.fft.irfft, with a sentinel around the rows;
  * -m gpu, one rank: every layout, c2r of a given half spectrum against numpy.fft.irfftn, and forward then inverse;
  * -m gpu, several ranks on the one GPU (threads of one process, the test transport; processes over hipIpc);
  * -m gpu, full size: 512^3 in three layouts and 1024^3, forward then inverse, compared on the device."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from offt_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREP_C2R = 0x200  # offt_hipk.h OFFT_HIPK_PREP_C2R


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


def c2r_desc(n, prec, ncols=16, nb1=2, in_contig=0):
    """the real-output z pass of a one-rank inverse: n/2+1 complex values per line in, n reals at the head of each row out"""
    nh = n // 2 + 1
    d = Desc()
    d.n, d.precision, d.direction, d.ncols, d.nb1, d.nb2 = n, prec, +1, ncols, nb1, 1
    if in_contig:
        d.in_axis_stride, d.in_col_stride = 1, nh
    else:
        d.in_axis_stride, d.in_col_stride = ncols, 1
    d.in_b1_stride = nh * ncols
    d.out_axis_stride, d.out_col_stride, d.out_b1_stride = 1, nh, nh * ncols
    d.in_contig, d.out_contig, d.variant, d.scale, d.real_input = in_contig, 1, -1, 1.0, 2
    return d


def test_c2r_kernel_routing_without_a_gpu(built):
    """a real-output descriptor resolves to a real-output panel instance (power-of-two and precompiled mixed-radix lengths,
    strided and contiguous input), never to the real-input kernels; a store side it cannot take goes elsewhere"""
    L = api.lib()
    L.offt_hipk_kernel_name.restype = C.c_char_p
    L.offt_hipk_kernel_name.argtypes = [C.POINTER(Desc)]
    name = lambda d: L.offt_hipk_kernel_name(C.byref(d)).decode()
    for n, prec, want in ((1024, api.F64, "fft_c2r_panel_k"), (2048, api.F64, "fft_c2r_panel_k"), (1000, api.F64, "fft_c2r_panelx_k"),
                          (2048, api.F32, "fft_c2r_panel_k"), (64, api.F64, "fft_c2r_panel_k"), (768, api.F64, "fft_c2r_panelx_k"),
                          (512, api.F32, "fft_c2r_panel_k")):
        for inc in (0, 1):
            assert name(c2r_desc(n, prec, in_contig=inc)) == want, (n, prec, inc)
    d = c2r_desc(1024, api.F64)
    d.in_split = 64                                  # power-of-two blocks on the input side: still the panel kernel
    assert name(d) == "fft_c2r_panel_k"
    d.in_split, d.in_split_nfloor = 128, 3           # 513 values over 4 peers: 128, 128, 128, 129 (uneven blocks)
    assert name(d) == "fft_c2r_panelx_k"             # the any-split instance of the length
    d = c2r_desc(1024, api.F64)
    d.out_contig, d.out_axis_stride, d.out_col_stride = 0, 16, 1   # real rows must be contiguous: no panel kernel
    assert name(d) == "fft_mixed_k"


# ---------------------------------------------------------------------------------------------------------------------
# GPU tier
# ---------------------------------------------------------------------------------------------------------------------
TOL = {api.F64: 1e-13, api.F32: 5e-6}


def _offsets(k, split, nfloor, axis, blk, tab):
    """element offset of axis index k (array) under a per-peer split (offt_hipk.h)"""
    if not (split or nfloor):
        return k * axis
    lim = split * nfloor if nfloor else 1 << 60
    b = np.where(k < lim, k // max(split, 1), nfloor + (k - lim) // (split + 1))
    r = np.where(k < lim, k - b * split, (k - lim) - (b - nfloor) * (split + 1))
    base = tab[b] if tab is not None else b * blk
    return base + r * axis


def _rand_desc(rng, n, prec):
    nh = n // 2 + 1
    d = Desc()
    d.n, d.precision, d.direction = n, prec, +1
    d.ncols, d.nb1, d.nb2 = int(rng.integers(1, 13)), int(rng.integers(1, 4)), int(rng.integers(1, 3))
    d.in_contig, d.out_contig, d.variant, d.real_input = int(rng.integers(0, 2)), 1, -1, 2
    d.scale = float(rng.choice([1.0, 0.5, 1.0 / n]))
    kind = int(rng.integers(0, 3)) if nh >= 4 else 0
    split = nfloor = 0
    if kind == 1:        # even split of the nh input values (power-of-two or any other divisor)
        split = int(rng.choice([f for f in range(1, nh) if nh % f == 0]))
    elif kind == 2:      # uneven F / F+1 blocks
        p = int(rng.integers(2, min(nh, 6) + 1))
        F, b = nh // p, nh % p
        split, nfloor = (F, p - b) if b else (F, 0)
    d.in_split, d.in_split_nfloor = split, nfloor
    nblk = (nfloor + (nh - split * nfloor + split) // (split + 1) if nfloor else -(-nh // split)) if split else 1
    inner = (split + (1 if nfloor else 0)) if split else nh
    pad = int(rng.integers(0, 3))
    if d.in_contig:
        axis, col = 1, inner + pad
        plane = col * d.ncols
    else:
        col, axis = 1, d.ncols + pad
        plane = axis * inner
    blk = plane + int(rng.integers(0, 5))
    b1 = blk * nblk + int(rng.integers(0, 4))
    b2 = b1 * d.nb1 + int(rng.integers(0, 4))
    nin = b2 * d.nb2 + 8
    d.in_axis_stride, d.in_col_stride, d.in_b1_stride, d.in_b2_stride = axis, col, b1, b2
    d.in_block_stride = blk if split else 0
    tab = None
    if split and rng.integers(0, 2):   # the blocks at shuffled places behind the array (per-block base table)
        slots = rng.permutation(nblk + 2)[:nblk]
        tab = np.array([b * blk + (int(s) + 1) * nin for b, s in zip(range(nblk), slots)], dtype=np.int64)
        nin = nin * (nblk + 4)
        d.in_block_stride = 1   # wrong on purpose: the table must be used
    # output rows of complex slots (as the forward's input layout: nh slots per row plus padding)
    orow = nh + int(rng.integers(0, 3))
    d.out_axis_stride, d.out_col_stride = 1, orow
    d.out_b1_stride = orow * d.ncols + int(rng.integers(0, 3))
    d.out_b2_stride = d.out_b1_stride * d.nb1 + int(rng.integers(0, 3))
    nout = d.out_b2_stride * d.nb2 + 4
    return d, nin, nout, tab, blk


def _run_desc(L, d, nin, nout, tab, blk, rng):
    import torch
    prec = d.precision
    ft, ct = (np.float64, np.complex128) if prec == api.F64 else (np.float32, np.complex64)
    n, nh = d.n, d.n // 2 + 1
    src = (rng.standard_normal(nin) + 1j * rng.standard_normal(nin)).astype(ct)   # not Hermitian anywhere
    # reference: every line through numpy.fft.irfft
    k = np.arange(nh)
    offs = _offsets(k, d.in_split, d.in_split_nfloor, d.in_axis_stride, blk, tab)
    want = np.full(2 * nout, 7.0, dtype=np.float64)
    rows = []
    for b2 in range(d.nb2):
        for b1 in range(d.nb1):
            for c in range(d.ncols):
                base = b2 * d.in_b2_stride + b1 * d.in_b1_stride + c * d.in_col_stride
                line = src[base + offs].astype(np.complex128)
                obase = 2 * (b2 * d.out_b2_stride + b1 * d.out_b1_stride + c * d.out_col_stride)
                want[obase:obase + n] = np.fft.irfft(line, n) * n * d.scale
                rows.append(obase)
    dt = torch.from_numpy(tab.copy()).cuda() if tab is not None else None
    d.in_block_tab = dt.data_ptr() if dt is not None else None
    din = torch.from_numpy(src.view(ft).copy()).cuda()
    dout = torch.full((2 * nout,), 7.0, dtype=torch.float64 if prec == api.F64 else torch.float32, device="cuda")
    torch.cuda.synchronize()
    rc = L.offt_hipk_fft_pass(C.byref(d), din.data_ptr(), dout.data_ptr(), None)
    assert rc == 0, L.offt_hipk_last_error()
    torch.cuda.synchronize()
    got = dout.cpu().numpy().astype(np.float64)
    mask = np.zeros(2 * nout, dtype=bool)
    for o in rows:
        mask[o:o + n] = True
    desc = {f: getattr(d, f) for f, _ in Desc._fields_}
    assert np.array_equal(got[~mask], want[~mask]), ("scalars outside the rows' n reals were written", desc)
    err = np.linalg.norm(got[mask] - want[mask]) / np.linalg.norm(want[mask])
    assert err <= TOL[prec], (err, desc)


@pytest.fixture(scope="module")
def kl(built):
    L = api.lib()
    L.offt_hipk_fft_pass.argtypes = [C.POINTER(Desc), C.c_void_p, C.c_void_p, C.c_void_p]
    L.offt_hipk_prepare.argtypes = [C.c_int, C.c_int]
    L.offt_hipk_last_error.restype = C.c_char_p
    L.offt_hipk_kernel_name.restype = C.c_char_p
    L.offt_hipk_kernel_name.argtypes = [C.POINTER(Desc)]
    return L


POW2 = [2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192]
OTHER = [6, 10, 30, 48, 1000, 2000, 15, 243, 432, 1016, 6000, 10007]   # mixed radix, odd, plan-time, Bluestein, four-step, prime


@pytest.mark.gpu
@pytest.mark.parametrize("n", POW2 + OTHER)
def test_c2r_random_descriptors(kl, n):
    L = kl
    rng = np.random.default_rng(5000 + n)
    reps = 4 if n <= 2048 else 2
    for prec in (api.F64, api.F32):
        assert L.offt_hipk_prepare(n, prec | PREP_C2R) == 0, L.offt_hipk_last_error()
        for _ in range(reps):
            d, nin, nout, tab, blk = _rand_desc(rng, n, prec)
            _run_desc(L, d, nin, nout, tab, blk, rng)


@pytest.mark.gpu
def test_c2r_plan_time_length_has_real_output_kernels(kl):
    """432 points has no precompiled panel kernel: an r2c-style prepare compiles the real-output flavours as well"""
    L = kl
    for prec in (api.F64, api.F32):
        assert L.offt_hipk_prepare(432, prec | PREP_C2R) == 0
        for inc in (0, 1):
            assert L.offt_hipk_kernel_name(C.byref(c2r_desc(432, prec, in_contig=inc))).decode() == "fft_c2r_panelx_k", (prec, inc)


# ---- one rank, 3-D ----------------------------------------------------------------------------------------------------
def _real_rows_index(c, shape):
    s0, s1, _ = c["istride"]
    n0, n1, n2 = shape
    return (np.arange(n0)[:, None, None] * 2 * s0 + np.arange(n1)[None, :, None] * 2 * s1 + np.arange(n2)[None, None, :]).ravel()


def _out_index(c, shape):
    s0, s1, s2 = c["ostride"]
    n0, n1, n2 = shape
    return (np.arange(n0)[:, None, None] * s0 + np.arange(n1)[None, :, None] * s1 + np.arange(n2)[None, None, :] * s2).ravel()


def one_rank_c2r(shape, precision=api.F64, eq=0, rotate=None, **params):
    """(a) c2r of rfftn(field), (b) forward then c2r with output scale 1/N, (c) c2r of a random half spectrum:
    the three rel-L2 errors"""
    import torch
    if rotate is not None:
        os.environ["OFFT_ROTATE"] = str(rotate)
    try:
        po = api.offt_3d_init(*shape, custom_params=api.make_params(**params), is_equalxy=eq, precision=precision, is_r2c=1)
    finally:
        os.environ.pop("OFFT_ROTATE", None)
    L = api.lib()
    try:
        c = api.comm_dict(po)
        ft, ct = (np.float64, np.complex128) if precision == api.F64 else (np.float32, np.complex64)
        N = int(np.prod(shape))
        hshape = (shape[0], shape[1], shape[2] // 2 + 1)
        ridx, oidx = _real_rows_index(c, shape), _out_index(c, hshape)
        rng = np.random.default_rng(sum(shape))
        field = rng.standard_normal(shape)
        errs = []
        for X in (np.fft.rfftn(field), rng.standard_normal(hshape) + 1j * rng.standard_normal(hshape)):
            buf = np.zeros(api.local_elems(po), dtype=ct)
            buf[oidx] = X.astype(ct).ravel()
            dev = torch.from_numpy(buf.view(ft)).cuda()
            L.offt_hip_set_output_scale(po, 1.0)
            api.offt_3d_execute_dir(po, dev.data_ptr(), dev.data_ptr(), +1)
            got = dev.cpu().numpy()[ridx].reshape(shape).astype(np.float64)
            want = np.fft.irfftn(X, s=shape) * N
            errs.append(float(np.linalg.norm(got - want) / np.linalg.norm(want)))
        rv = np.zeros(2 * api.local_elems(po), dtype=ft)
        rv[ridx] = field.ravel()
        dev = torch.from_numpy(rv).cuda()
        api.offt_3d_execute(po, dev.data_ptr(), dev.data_ptr())
        L.offt_hip_set_output_scale(po, 1.0 / N)
        api.offt_3d_execute_dir(po, dev.data_ptr(), dev.data_ptr(), +1)
        back = dev.cpu().numpy()[ridx].reshape(shape).astype(np.float64)
        errs.insert(1, float(np.linalg.norm(back - field) / np.linalg.norm(field)))
        return errs
    finally:
        api.offt_3d_fin(po)


SHAPES = [(16, 16, 16), (64, 64, 64), (128, 32, 256), (32, 32, 1024), (20, 12, 18), (8, 8, 2), (8, 6, 15), (6, 4, 1016),
          (4, 4, 6000), (4, 4, 10007)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_c2r_one_rank(built, shape):
    import torch
    torch.cuda.set_device(0)
    layouts = [dict(), dict(S=1, rotate=0), dict(S=1, rotate=1), dict(eq=1)] if shape[0] == shape[1] else [dict(), dict(S=1)]
    for precision in (api.F64, api.F32):
        for lay in layouts:
            errs = one_rank_c2r(shape, precision, **lay)
            assert max(errs) <= TOL[precision], (shape, precision, lay, errs)


# ---- several ranks on the one GPU -------------------------------------------------------------------------------------
def _thread_world(size, cases, tmp_path):
    env = dict(os.environ, GPU_MAX_HW_QUEUES="24")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_c2r_world.py"), str(size), json.dumps(cases), str(tmp_path)],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-4000:]
    res = json.load(open(tmp_path / "summary.json"))
    assert len(res) == len(cases)
    for r in res:
        assert r["rel"] <= r["tol"], r
    return res


@pytest.mark.gpu
def test_c2r_thread_worlds(built, tmp_path):
    cases2 = [dict(N=[16, 16, 16], params={}), dict(N=[32, 16, 64], params={}, p2p=1), dict(N=[16, 8, 18], params={}, f32=1),
              dict(N=[16, 16, 32], params={}, k1=2, comm=2)]
    cases3 = [dict(N=[12, 9, 16], params={}), dict(N=[12, 12, 20], params={}, p2p=1), dict(N=[12, 9, 15], params={})]
    cases4 = [dict(N=[16, 16, 16], params={"P1": 2}), dict(N=[16, 16, 32], params={"P1": 2}, p2p=1),
              dict(N=[16, 16, 64], params={}), dict(N=[16, 16, 64], params={}, p2p=1),
              dict(N=[10, 6, 9], params={"P1": 2, "T1": 2, "T2": 3}), dict(N=[16, 16, 32], params={"P1": 2}, f32=1)]
    _thread_world(2, cases2, tmp_path)
    _thread_world(3, cases3, tmp_path)
    _thread_world(4, cases4, tmp_path)


@pytest.mark.gpu
def test_c2r_process_world_direct_store(built, tmp_path):
    """processes sharing the card, the direct-store exchange over hipIpc"""
    env = dict(os.environ, GPU_MAX_HW_QUEUES="8")
    procs = []
    case = dict(N=[16, 16, 32], params={}, p2p=1)
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    for r in range(2):
        e = dict(env, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_c2r_world.py"), "proc", json.dumps(case), str(tmp_path)],
                                      env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = [p.communicate(timeout=600)[0].decode() for p in procs]
    for r, p in enumerate(procs):
        assert p.returncode == 0, f"rank {r}:\n{outs[r][-3000:]}"
    for r in range(2):
        rec = json.load(open(tmp_path / f"proc_rank{r}.json"))
        assert rec["exchange"] == 1 and rec["rel"] <= 1e-13, rec


# ---- full size ----------------------------------------------------------------------------------------------------------
def _full_size(shape, precision=api.F64, eq=0, **params):
    """fill (seeded hash) -> forward -> c2r with scale 1/N -> rel-L2 against a second fill, on the device, slab by slab"""
    import torch
    L = api.lib()
    po = api.offt_3d_init(*shape, custom_params=api.make_params(**params), is_equalxy=eq, precision=precision, is_r2c=1)
    try:
        c = api.comm_dict(po)
        td = torch.float64 if precision == api.F64 else torch.float32
        n = 2 * api.local_elems(po)
        a = torch.empty(n, dtype=td, device="cuda")
        b = torch.empty(n, dtype=td, device="cuda")
        assert L.offt_hip_fill_input(po, a.data_ptr(), 1) == 0 and L.offt_hip_fill_input(po, b.data_ptr(), 1) == 0
        torch.cuda.synchronize()
        api.offt_3d_execute(po, a.data_ptr(), a.data_ptr())
        L.offt_hip_set_output_scale(po, 1.0 / float(np.prod(shape)))
        api.offt_3d_execute_dir(po, a.data_ptr(), a.data_ptr(), +1)
        torch.cuda.synchronize()
        s0, s1, _ = c["istride"]
        va = torch.as_strided(a, shape, (2 * s0, 2 * s1, 1))
        vb = torch.as_strided(b, shape, (2 * s0, 2 * s1, 1))
        num = den = 0.0
        for x0 in range(0, shape[0], 64):
            d = (va[x0:x0 + 64].double() - vb[x0:x0 + 64].double())
            num += float(d.square().sum())
            den += float(vb[x0:x0 + 64].double().square().sum())
        del a, b, va, vb
        return (num / den) ** 0.5
    finally:
        api.offt_3d_fin(po)


@pytest.mark.gpu
def test_c2r_full_size(built):
    import torch
    torch.cuda.set_device(0)
    for kw in (dict(), dict(S=1), dict(eq=1)):
        err = _full_size((512, 512, 512), **kw)
        assert err <= 1e-13, (kw, err)
    err = _full_size((1024, 1024, 1024))
    assert err <= 1e-13, err
