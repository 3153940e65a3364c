"""Spectral convolution (offt_hip_execute_convolve) on worlds of several ranks, and the pieces the single-rank tests share.

  _conv_world.py gloo <cases.json> <outdir>       one gloo rank per PROCESS (RANK / WORLD_SIZE / MASTER_* set) on the CPU
                                                   convolution backend (tests/libcpubackend_conv.so)
  _conv_world.py <size> <cases.json> <outdir>     ranks as THREADS of one process on the one GPU, the test build's transport
                                                   seam (the thread-world machinery of _c2r_world.py)

A case: {"N": [Nx, Ny, Nz], "params": {...}, "r2c": 0/1, "f32": 0/1, "cplx": 0/1 (complex filter), "p2p": 0/1, "eq": 0/1}.
Every rank builds the same global field x and filter H from a seed, hands in its input block and its part of H, and
compares its result block with numpy (rel-L2)."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SCALE = 0.5


def problem(N, r2c, cplx, seed=7):
    """global x, H and the expected SCALE * N * ifftn(H * fftn(x)) (irfftn / rfftn for r2c)"""
    rng = np.random.default_rng(seed + sum(N))
    N = tuple(N)
    x = rng.standard_normal(N) if r2c else rng.standard_normal(N) + 1j * rng.standard_normal(N)
    hs = (N[0], N[1], N[2] // 2 + 1) if r2c else N
    H = rng.standard_normal(hs) + (1j * rng.standard_normal(hs) if cplx else 0.0)
    n = float(np.prod(N))
    want = (np.fft.irfftn(H * np.fft.rfftn(x), s=N, axes=(0, 1, 2)) if r2c else np.fft.ifftn(H * np.fft.fftn(x))) * n * SCALE
    return x, H, want


def in_index(c, r2c):
    """indices of the input block: scalars of the real rows (r2c) or complex elements"""
    n0, n1, n2 = c["isize"]
    s0, s1, s2 = c["istride"]
    if r2c:
        s0, s1, s2 = 2 * s0, 2 * s1, 1
    return (np.arange(n0)[:, None, None] * s0 + np.arange(n1)[None, :, None] * s1 + np.arange(n2)[None, None, :] * s2).ravel()


def out_index(c):
    n0, n1, n2 = c["osize"]
    s0, s1, s2 = c["ostride"]
    return (np.arange(n0)[:, None, None] * s0 + np.arange(n1)[None, :, None] * s1 + np.arange(n2)[None, None, :] * s2).ravel()


def local_arrays(c, nelems, case, x, H):
    """this rank's data buffer (complex elements, or their scalars for r2c) and filter buffer (complex, or one scalar per
    complex slot for a real filter), as numpy arrays of the plan's precision"""
    f32 = bool(case.get("f32"))
    ft, ct = (np.float32, np.complex64) if f32 else (np.float64, np.complex128)
    r2c = bool(case.get("r2c"))
    i0, i1, i2 = c["istart"]
    n0, n1, n2 = c["isize"]
    o0, o1, o2 = c["ostart"]
    m0, m1, m2 = c["osize"]
    data = np.zeros(nelems, dtype=ct)
    blk = x[i0:i0 + n0, i1:i1 + n1, i2:i2 + n2]
    if r2c:
        data.view(ft)[in_index(c, True)] = blk.real.ravel().astype(ft)
    else:
        data[in_index(c, False)] = blk.ravel().astype(ct)
    hb = H[o0:o0 + m0, o1:o1 + m1, o2:o2 + m2].ravel()
    if case.get("cplx"):
        filt = np.zeros(nelems, dtype=ct)
        filt[out_index(c)] = hb.astype(ct)
    else:
        filt = np.zeros(nelems, dtype=ft)
        filt[out_index(c)] = hb.real.astype(ft)
    return data, filt


def check(c, case, got, want):
    """rel-L2 of this rank's result block (data buffer `got`, numpy) against the global expectation"""
    r2c = bool(case.get("r2c"))
    i0, i1, i2 = c["istart"]
    n0, n1, n2 = c["isize"]
    if n0 * n1 * n2 == 0:
        return 0.0
    w = want[i0:i0 + n0, i1:i1 + n1, i2:i2 + n2].ravel()
    g = (got.view(np.float32 if got.dtype == np.complex64 else np.float64)[in_index(c, True)] if r2c else got[in_index(c, False)])
    g = g.astype(np.complex128 if np.iscomplexobj(g) else np.float64)  # (a complex result is compared whole)
    return float(np.linalg.norm(g - w) / np.linalg.norm(w))


def tol(case):
    return 2e-5 if case.get("f32") else 1e-12


# ---- CPU: one gloo rank per process ----------------------------------------------------------------------------------
def conv_cb_lib():
    """tests/libcpubackend_conv.so, shaped like cpu_world's backend library (its table = the convolution table)"""
    so = os.path.join(ROOT, "tests", "libcpubackend_conv.so")
    L = C.CDLL(so)
    for f in ("cpu_backend_conv_table", "cpu_backend_conv_table_unfused", "cpu_backend_conv_table_none"):
        getattr(L, f).restype = C.c_void_p
    L.cpu_backend_table = L.cpu_backend_conv_table
    L.cpu_backend_pass_count.restype = C.c_long
    L.cpu_backend_conv_count.restype = C.c_long
    L.cpu_backend_pointwise_count.restype = C.c_long
    return L


def cpu_convolve(api, case, rank=0):
    """plan + convolve on the installed CPU backend; (rel-L2, fused route?, comm dict)"""
    prec = api.F32 if case.get("f32") else api.F64
    po = api.offt_3d_init(*case["N"], custom_params=api.make_params(**case.get("params", {})), is_equalxy=case.get("eq", 0),
                          precision=prec, is_r2c=int(case.get("r2c", 0)))
    try:
        L = api.lib()
        c = api.comm_dict(po)
        x, H, want = problem(case["N"], case.get("r2c"), case.get("cplx"))
        data, filt = local_arrays(c, api.local_elems(po), case, x, H)
        L.offt_hip_set_output_scale(po, SCALE)
        api.offt_hip_execute_convolve(po, data.ctypes.data, filt.ctypes.data, api.FILTER_COMPLEX if case.get("cplx") else api.FILTER_REAL)
        return check(c, case, data, want), api.offt_hip_convolve_fused(po), c
    finally:
        api.offt_3d_fin(po)


def gloo_main(cases, outdir):
    import torch.distributed as dist
    import cpu_world
    from offt_amd import api
    rank, size = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=size)
    cpu_world._cb_lib = conv_cb_lib
    out = []
    for case in cases:
        if case.get("p2p"):
            os.environ["OFFT_EXCHANGE"] = "p2p"
        CB = cpu_world.install(rank, size, dist=dist)
        n0 = CB.cpu_backend_pointwise_count()
        err, fused, _ = cpu_convolve(api, case, rank)
        out.append({"case": case, "rel": err, "fused": fused, "pointwise": CB.cpu_backend_pointwise_count() - n0, "tol": tol(case)})
        os.environ.pop("OFFT_EXCHANGE", None)
        dist.barrier()
    cpu_world.uninstall()
    json.dump(out, open(os.path.join(outdir, f"gloo_rank{rank}.json"), "w"))
    dist.destroy_process_group()


# ---- GPU: ranks as threads of one process ------------------------------------------------------------------------------
def gpu_rank(L, api, torch, po, case):
    """the thread world's per-rank step (replaces _c2r_world.roundtrip): convolve this rank's block on the device"""
    c = api.comm_dict(po)
    x, H, want = problem(case["N"], case.get("r2c"), case.get("cplx"))
    data, filt = local_arrays(c, api.local_elems(po), case, x, H)
    dd = torch.from_numpy(data.view(data.real.dtype).copy()).cuda()
    df = torch.from_numpy(filt.view(filt.real.dtype if filt.dtype.kind == "c" else filt.dtype).copy()).cuda()
    torch.cuda.synchronize()
    L.offt_hip_set_output_scale(po, SCALE)
    api.offt_hip_execute_convolve(po, dd.data_ptr(), df.data_ptr(), api.FILTER_COMPLEX if case.get("cplx") else api.FILTER_REAL)
    torch.cuda.synchronize()
    got = dd.cpu().numpy().view(data.dtype)
    return check(c, case, got, want), c


def threads_main(size, cases, outdir):
    import _c2r_world
    from offt_amd import api
    summary = []
    orig_init = api.offt_3d_init
    for case in cases:
        # _c2r_world's thread world makes real-input plans: the case says which kind this one is
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
