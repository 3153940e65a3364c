"""Multi-input spectral convolution (offt_hip_execute_convolve_sum): the pieces tests/test_convolve_sum.py shares, and the gloo
worlds of several ranks.

  _conv_sum_world.py gloo <cases.json> <outdir>     one gloo rank per PROCESS on the CPU backend of tests/cpu_backend_sum.c
                                                     (tests/libcpubackend_sum.so)
  _conv_sum_world.py <size> <cases.json> <outdir>   ranks as THREADS of one process on the one GPU (the thread-world
                                                     machinery of _c2r_world.py, as _conv_multi_world.py uses it)

A case is a case of _conv_world.py plus "K" (inputs), "inplace" (index of the input that is `out`, or None) and "half" (1: a
half-box plan; the padding of every input is poisoned with NaN and only the box of the output is compared)."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import _conv_world as W  # noqa: E402
import _half_world as HW  # noqa: E402

SCALE = W.SCALE
KINDS = {"pass": 0, "conv": 1, "conv_sum": 2, "pointwise": 3, "pointwise_sum": 4, "memcpy": 5, "zero": 6}


def problem(case, seed=41):
    """K global inputs (zero outside the box of a half-box case), K filters and the expected output.  Asserts, on the numpy
    side alone, that the sum does not cancel: its norm is at least that of its largest term."""
    N, r2c, cplx, K = tuple(case["N"]), bool(case.get("r2c")), bool(case.get("cplx")), int(case.get("K", 3))
    rng = np.random.default_rng(seed + sum(N) + K)
    hs = (N[0], N[1], N[2] // 2 + 1) if r2c else N
    n = float(np.prod(N))
    xs, Hs, terms = [], [], []
    for _ in range(K):
        x = rng.standard_normal(N) if r2c else rng.standard_normal(N) + 1j * rng.standard_normal(N)
        if case.get("half"):
            xp = np.zeros_like(x)
            h = tuple(m // 2 for m in N)
            xp[:h[0], :h[1], :h[2]] = x[:h[0], :h[1], :h[2]]
            x = xp
        H = rng.standard_normal(hs) + (1j * rng.standard_normal(hs) if cplx else 0.0)
        X = np.fft.rfftn(x, axes=(0, 1, 2)) if r2c else np.fft.fftn(x)
        terms.append((np.fft.irfftn(H * X, s=N, axes=(0, 1, 2)) if r2c else np.fft.ifftn(H * X)) * n * SCALE)
        xs.append(x)
        Hs.append(H)
    want = sum(terms[1:], terms[0])
    assert np.linalg.norm(want) >= max(np.linalg.norm(t) for t in terms), "the sum cancels: a relative error would mean nothing"
    return xs, Hs, want


def run_sum(api, po, case, dev, pr=None, keep=None):
    """the multi-input call on a plan; rel-L2 of the output (inside the box for a half-box case)"""
    L = api.lib()
    c = api.comm_dict(po)
    ne = api.local_elems(po)
    xs, Hs, want = pr or problem(case)
    ins, filts = [], []
    for x, H in zip(xs, Hs):
        d, f = W.local_arrays(c, ne, case, x, H)
        if case.get("half"):
            d = HW.poisoned_input(c, ne, case, x)
        ins.append(d)
        filts.append(f)
    inplace = case.get("inplace")
    hi = [dev.put(d) for d in ins]
    hf = [dev.put(f) for f in filts]
    ho = hi[inplace] if inplace is not None else dev.put(np.full(ne, 3.0 - 2.0j, dtype=ins[0].dtype))
    L.offt_hip_set_output_scale(po, SCALE)
    api.offt_hip_execute_convolve_sum(po, [p for _, p in hi], [p for _, p in hf], ho[1],
                                      api.FILTER_COMPLEX if case.get("cplx") else api.FILTER_REAL)
    L.offt_hip_set_output_scale(po, 1.0)
    got = dev.get(ho[0], ins[0])
    if keep is not None:
        keep["got"] = np.array(got, copy=True)
    err = HW.box_err if case.get("half") else W.check
    return err(c, case, got, want)


def sum_cb_lib():
    """tests/libcpubackend_sum.so, shaped like cpu_world's backend library (its table = the full sum table)"""
    L = C.CDLL(os.path.join(ROOT, "tests", "libcpubackend_sum.so"))
    for f in ("cpu_backend_sum_table", "cpu_backend_sum_table_old", "cpu_backend_sum_table_nofused"):
        getattr(L, f).restype = C.c_void_p
    L.cpu_backend_table = L.cpu_backend_sum_table
    L.cpu_backend_sum_count.restype = C.c_long
    L.cpu_backend_sum_count.argtypes = [C.c_int]
    L.cpu_backend_sum_log.argtypes = [C.c_int, C.POINTER(C.c_int)]
    return L


def counts(CB):
    return {k: CB.cpu_backend_sum_count(v) for k, v in KINDS.items()}


def launches(CB):
    """the launches logged since the last reset: (kind, n, direction, ncols, nb1, half, real_input, nin)"""
    out, rec, i = [], (C.c_int * 8)(), 0
    while CB.cpu_backend_sum_log(i, rec) == 0:
        out.append(tuple(rec))
        i += 1
    return out


def gloo_main(cases, outdir):
    import torch.distributed as dist
    import cpu_world
    from offt_amd import api
    rank, size = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=size)
    cpu_world._cb_lib = sum_cb_lib
    out = []
    for case in cases:
        CB = cpu_world.install(rank, size, dist=dist)
        n0 = counts(CB)
        po = HW.make_plan(api, case)
        try:
            err = run_sum(api, po, case, HW.Host())
            fused = api.offt_hip_convolve_sum_fused(po)
        finally:
            api.offt_3d_fin(po)
        n1 = counts(CB)
        out.append({"case": case, "rel": err, "fused": fused, "tol": W.tol(case), "counts": {k: n1[k] - n0[k] for k in n0}})
        dist.barrier()
    cpu_world.uninstall()
    json.dump(out, open(os.path.join(outdir, f"gloo_rank{rank}.json"), "w"))
    dist.destroy_process_group()


# ---- GPU: ranks as threads of one process ------------------------------------------------------------------------------
def gpu_rank(L, api, torch, po, case):
    return run_sum(api, po, case, HW.Gpu(torch)), api.comm_dict(po)


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
        rec["tol"] = W.tol(case)
        summary.append(rec)
    api.offt_3d_init = orig_init
    json.dump(summary, open(os.path.join(outdir, "summary.json"), "w"))


if __name__ == "__main__":
    if sys.argv[1] == "gloo":
        gloo_main(json.loads(sys.argv[2]), sys.argv[3])
    else:
        threads_main(int(sys.argv[1]), json.loads(sys.argv[2]), sys.argv[3])
