"""Half-box plans (offt_hip_set_half_box): the pieces tests/test_half_box.py shares, and worlds of several ranks.

  _half_world.py gloo <cases.json> <outdir>       one gloo rank per PROCESS on the CPU pad backend (tests/libcpubackend_pad.so)
  _half_world.py <size> <cases.json> <outdir>     ranks as THREADS of one process on the one GPU (the thread world of
                                                   _c2r_world.py)

A case: {"N": [Nx, Ny, Nz], "params": {...}, "r2c": 0/1, "f32": 0/1, "eq": 0/1}.  The data occupies the box
[0,Nx/2) x [0,Ny/2) x [0,Nz/2); every other element of a rank's input block is NaN going in.  Forward, inverse and convolve
are compared with numpy on the explicitly zero-padded array (rel-L2), the inverse and the convolve inside the box only."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import _conv_world as W  # noqa: E402

SCALE = 0.5


def tol(case):
    """the project's own tolerances (tests/test_convolve.py)"""
    return 1e-5 if case.get("f32") else 1e-12


def problem(N, r2c, seed=11):
    """the zero-padded field, its spectrum; a spectrum Y with its inverse; a filter H with the convolution"""
    N = tuple(N)
    rng = np.random.default_rng(seed + sum(N))
    h = tuple(n // 2 for n in N)
    box = rng.standard_normal(h) if r2c else rng.standard_normal(h) + 1j * rng.standard_normal(h)
    xp = np.zeros(N, dtype=box.dtype)
    xp[:h[0], :h[1], :h[2]] = box
    n = float(np.prod(N))
    if r2c:
        spec = np.fft.rfftn(xp, axes=(0, 1, 2))
        r = rng.standard_normal(N)
        Y, inv = np.fft.rfftn(r, axes=(0, 1, 2)), r * n
        H = rng.standard_normal(spec.shape) + 1j * rng.standard_normal(spec.shape)
        conv = np.fft.irfftn(H * spec, s=N, axes=(0, 1, 2)) * n * SCALE
    else:
        spec = np.fft.fftn(xp)
        Y = rng.standard_normal(N) + 1j * rng.standard_normal(N)
        inv = np.fft.ifftn(Y) * n
        H = rng.standard_normal(N) + 1j * rng.standard_normal(N)
        conv = np.fft.ifftn(H * spec) * n * SCALE
    return dict(xp=xp, spec=spec, Y=Y, inv=inv, H=H, conv=conv)


def box_mask(c, N):
    """which elements of this rank's input block lie inside the box (raveled like _conv_world.in_index)"""
    i0, i1, i2 = c["istart"]
    n0, n1, n2 = c["isize"]
    m = ((np.arange(n0) + i0 < N[0] // 2)[:, None, None] & (np.arange(n1) + i1 < N[1] // 2)[None, :, None] &
         (np.arange(n2) + i2 < N[2] // 2)[None, None, :])
    return m.ravel()


def poisoned_input(c, nelems, case, xp):
    """this rank's input buffer: the box from xp, NaN in the rest of the block"""
    f32, r2c = bool(case.get("f32")), bool(case.get("r2c"))
    ft, ct = (np.float32, np.complex64) if f32 else (np.float64, np.complex128)
    i0, i1, i2 = c["istart"]
    n0, n1, n2 = c["isize"]
    blk = xp[i0:i0 + n0, i1:i1 + n1, i2:i2 + n2].ravel()
    idx, m = W.in_index(c, r2c), box_mask(c, case["N"])
    data = np.zeros(nelems, dtype=ct)
    if r2c:
        v = data.view(ft)
        v[idx] = np.nan
        v[idx[m]] = blk.real[m].astype(ft)
    else:
        data[idx] = np.nan + 1j * np.nan
        data[idx[m]] = blk[m].astype(ct)
    return data


def box_err(c, case, got, want):
    """rel-L2 inside the box of this rank's block of the input layout"""
    r2c = bool(case.get("r2c"))
    i0, i1, i2 = c["istart"]
    n0, n1, n2 = c["isize"]
    idx, m = W.in_index(c, r2c), box_mask(c, case["N"])
    if not m.any():
        return 0.0
    w = want[i0:i0 + n0, i1:i1 + n1, i2:i2 + n2].ravel()[m]
    g = got.view(np.float32 if got.dtype == np.complex64 else np.float64)[idx[m]] if r2c else got[idx[m]]
    g = g.astype(np.complex128 if np.iscomplexobj(g) else np.float64)
    return float(np.linalg.norm(g - w) / np.linalg.norm(w))


def out_block(c, A):
    o0, o1, o2 = c["ostart"]
    m0, m1, m2 = c["osize"]
    return A[o0:o0 + m0, o1:o1 + m1, o2:o2 + m2].ravel()


class Host:
    """buffers of the CPU backend: numpy arrays as they are"""
    def put(self, a):
        return a, a.ctypes.data

    def get(self, h, like):
        return h


class Gpu:
    def __init__(self, torch):
        self.torch = torch

    def put(self, a):
        t = self.torch.from_numpy(a.view(a.real.dtype).copy()).cuda()
        self.torch.cuda.synchronize()
        return t, t.data_ptr()

    def get(self, h, like):
        self.torch.cuda.synchronize()
        return h.cpu().numpy().view(like.dtype)


def run_plan(api, po, case, dev, pr=None):
    """forward, inverse and convolve of a half-box plan; {"fwd", "inv", "conv"} rel-L2 and the forward's output buffer"""
    L = api.lib()
    c = api.comm_dict(po)
    ne = api.local_elems(po)
    pr = pr or problem(case["N"], case.get("r2c"))
    ct = np.complex64 if case.get("f32") else np.complex128
    res = {}
    data = poisoned_input(c, ne, case, pr["xp"])
    h, p = dev.put(data)
    api.offt_3d_execute_dir(po, p, p, -1)
    got = dev.get(h, data)
    want = out_block(c, pr["spec"])
    res["fwd"] = float(np.linalg.norm(got[W.out_index(c)].astype(np.complex128) - want) / np.linalg.norm(want)) if want.size else 0.0
    fwd_out = got.copy()
    buf = np.zeros(ne, dtype=ct)
    buf[W.out_index(c)] = out_block(c, pr["Y"]).astype(ct)
    h, p = dev.put(buf)
    api.offt_3d_execute_dir(po, p, p, +1)
    res["inv"] = box_err(c, case, dev.get(h, buf), pr["inv"])
    data = poisoned_input(c, ne, case, pr["xp"])
    filt = np.zeros(ne, dtype=ct)
    filt[W.out_index(c)] = out_block(c, pr["H"]).astype(ct)
    h, p = dev.put(data)
    hf, pf = dev.put(filt)
    L.offt_hip_set_output_scale(po, SCALE)
    api.offt_hip_execute_convolve(po, p, pf, api.FILTER_COMPLEX)
    L.offt_hip_set_output_scale(po, 1.0)
    res["conv"] = box_err(c, case, dev.get(h, data), pr["conv"])
    return res, fwd_out


def make_plan(api, case):
    return api.offt_3d_init(*case["N"], custom_params=api.make_params(**case.get("params", {})), is_equalxy=case.get("eq", 0),
                            precision=api.F32 if case.get("f32") else api.F64, is_r2c=int(case.get("r2c", 0)))


def run_case(api, case, dev):
    """plan, switch the half box on, run; (errors, pruned?)"""
    po = make_plan(api, case)
    try:
        api.offt_hip_set_half_box(po, True)
        res, _ = run_plan(api, po, case, dev)
        return res, api.offt_hip_half_box_pruned(po)
    finally:
        api.offt_3d_fin(po)


# ---- CPU: the pad backend -----------------------------------------------------------------------------------------------
def pad_cb_lib():
    """tests/libcpubackend_pad.so, shaped like cpu_world's backend library (its table = the pad table)"""
    L = C.CDLL(os.path.join(ROOT, "tests", "libcpubackend_pad.so"))
    for f in ("cpu_backend_pad_table", "cpu_backend_pad_table_unfused", "cpu_backend_pad_table_nozero"):
        getattr(L, f).restype = C.c_void_p
    L.cpu_backend_table = L.cpu_backend_pad_table
    L.cpu_backend_pass_count.restype = C.c_long
    L.cpu_backend_pad_zero_count.restype = C.c_long
    L.cpu_backend_pad_half_count.restype = C.c_long
    L.cpu_backend_pad_log.argtypes = [C.c_int, C.POINTER(C.c_int)]
    return L


def launches(CB):
    """the launches recorded since the last reset: (n, ncols, nb1, nb2, half, conv)"""
    out, rec, i = [], (C.c_int * 6)(), 0
    while CB.cpu_backend_pad_log(i, rec) == 0:
        out.append(tuple(rec))
        i += 1
    return out


def gloo_main(cases, outdir):
    import torch.distributed as dist
    import cpu_world
    from offt_amd import api
    rank, size = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=size)
    cpu_world._cb_lib = pad_cb_lib
    out = []
    for case in cases:
        CB = cpu_world.install(rank, size, dist=dist)
        z0 = CB.cpu_backend_pad_zero_count()
        res, pruned = run_case(api, case, Host())
        out.append({"case": case, "res": res, "pruned": pruned, "zeroed": CB.cpu_backend_pad_zero_count() - z0, "tol": tol(case)})
        dist.barrier()
    cpu_world.uninstall()
    json.dump(out, open(os.path.join(outdir, f"gloo_rank{rank}.json"), "w"))
    dist.destroy_process_group()


# ---- GPU: ranks as threads of one process ------------------------------------------------------------------------------
def gpu_rank(L, api, torch, po, case):
    """the thread world's per-rank step: the three half-box checks on this rank's block; the largest error over its tolerance"""
    api.offt_hip_set_half_box(po, True)
    assert not api.offt_hip_half_box_pruned(po), "several ranks take the fallback"
    res, _ = run_plan(api, po, case, Gpu(torch))
    return max(res.values()), api.comm_dict(po)


def threads_main(size, cases, outdir):
    import _c2r_world
    from offt_amd import api
    summary = []
    orig_init = api.offt_3d_init
    for case in cases:
        api.offt_3d_init = lambda *a, _r2c=int(case.get("r2c", 0)), **kw: orig_init(*a, **dict(kw, is_r2c=_r2c))
        _c2r_world.roundtrip = gpu_rank
        _c2r_world.threads_main(size, [case], outdir)
        rec = json.load(open(os.path.join(outdir, "summary.json")))[0]
        rec["tol"] = tol(case)
        summary.append(rec)
    api.offt_3d_init = orig_init
    json.dump(summary, open(os.path.join(outdir, "summary.json"), "w"))


if __name__ == "__main__":
    if sys.argv[1] == "gloo":
        gloo_main(json.loads(sys.argv[2]), sys.argv[3])
    else:
        threads_main(int(sys.argv[1]), json.loads(sys.argv[2]), sys.argv[3])
