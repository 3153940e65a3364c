"""Pseudo-spectral product (offt_hip_execute_product): the pieces tests/test_product.py and tests/test_gpu_product.py share,
and the gloo worlds of several ranks.

  _prod_world.py gloo <cases.json> <outdir>     one gloo rank per PROCESS on the CPU backend of tests/cpu_backend_prod.c
                                                 (tests/libcpubackend_prod.so)

A case is a case of _conv_world.py plus "mode" ("two": out a buffer of its own; "a" / "b": out is that input; "null": b = NULL;
"same": b is a) and "half" (1: a half-box plan: the spectra are those of zero-padded fields)."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import _conv_world as W  # noqa: E402
import _half_world as HW  # noqa: E402

KINDS = {"pass": 0, "prod": 1, "pointwise_prod": 2, "zero": 3}


def problem(case, seed=53):
    """two global spectra A and B in the forward's output layout (the half spectrum of real fields on an r2c plan; of
    zero-padded fields for a half box) and N^2 fftn(ifftn(A) ifftn(B)).  Seeded random fields: the product does not cancel."""
    N, r2c = tuple(case["N"]), bool(case.get("r2c"))
    rng = np.random.default_rng(seed + sum(N))
    n = float(np.prod(N))

    def field():
        x = rng.standard_normal(N) if r2c else rng.standard_normal(N) + 1j * rng.standard_normal(N)
        if case.get("half"):
            xp = np.zeros_like(x)
            h = tuple(m // 2 for m in N)
            xp[:h[0], :h[1], :h[2]] = x[:h[0], :h[1], :h[2]]
            x = xp
        return x / np.sqrt(n)

    fwd = (lambda x: np.fft.rfftn(x, axes=(0, 1, 2))) if r2c else np.fft.fftn
    u, v = field(), field()
    return fwd(u), fwd(v), fwd(u * v) * n * n, fwd(u * u) * n * n


def spec_buffer(c, ne, case, A):
    ct = np.complex64 if case.get("f32") else np.complex128
    buf = np.zeros(ne, dtype=ct)
    buf[W.out_index(c)] = HW.out_block(c, A).astype(ct)
    return buf


def out_err(c, got, want):
    w = HW.out_block(c, want)
    if not w.size:
        return 0.0
    return float(np.linalg.norm(got[W.out_index(c)].astype(np.complex128) - w) / np.linalg.norm(w))


def run_product(api, po, case, dev, pr=None, keep=None, scale=None):
    """the product call on a plan; rel-L2 of this rank's output block against numpy"""
    L = api.lib()
    c = api.comm_dict(po)
    ne = api.local_elems(po)
    A, B, want, want_sq = pr or problem(case)
    mode = case.get("mode", "two")
    a = spec_buffer(c, ne, case, A)
    ha = dev.put(a)
    if mode in ("null", "same"):
        hb = (None, None) if mode == "null" else ha
        want = want_sq
    else:
        hb = dev.put(spec_buffer(c, ne, case, B))
    ho = ha if mode == "a" else hb if mode == "b" else dev.put(np.full(ne, 3.0 - 2.0j, dtype=a.dtype))
    if scale is not None:
        L.offt_hip_set_output_scale(po, scale)
        want = want * scale
    api.offt_hip_execute_product(po, ha[1], hb[1], ho[1])
    if scale is not None:
        L.offt_hip_set_output_scale(po, 1.0)
    got = dev.get(ho[0], a)
    if keep is not None:
        keep["got"] = np.array(got, copy=True)
    return out_err(c, got, want)


def prod_cb_lib():
    """tests/libcpubackend_prod.so, shaped like cpu_world's backend library (its table = the full product table)"""
    L = C.CDLL(os.path.join(ROOT, "tests", "libcpubackend_prod.so"))
    for f in ("cpu_backend_prod_table", "cpu_backend_prod_table_old", "cpu_backend_prod_table_nofused"):
        getattr(L, f).restype = C.c_void_p
    L.cpu_backend_table = L.cpu_backend_prod_table
    L.cpu_backend_prod_count.restype = C.c_long
    L.cpu_backend_prod_count.argtypes = [C.c_int]
    L.cpu_backend_prod_log.argtypes = [C.c_int, C.POINTER(C.c_int)]
    L.cpu_backend_alloc_count.restype = C.c_long
    L.cpu_backend_fail_alloc_at.argtypes = [C.c_long]
    return L


def counts(CB):
    return {k: CB.cpu_backend_prod_count(v) for k, v in KINDS.items()}


def launches(CB):
    """the launches logged since the last reset: (kind, n, direction, ncols, nb1, half, real_input, sources)"""
    out, rec, i = [], (C.c_int * 8)(), 0
    while CB.cpu_backend_prod_log(i, rec) == 0:
        out.append(tuple(rec))
        i += 1
    return out


def gloo_main(cases, outdir):
    import torch.distributed as dist
    import cpu_world
    from offt_amd import api
    rank, size = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=size)
    cpu_world._cb_lib = prod_cb_lib
    out = []
    for case in cases:
        CB = cpu_world.install(rank, size, dist=dist)
        n0 = counts(CB)
        po = HW.make_plan(api, case)
        try:
            err = run_product(api, po, case, HW.Host())
            fused = api.offt_hip_product_fused(po)
        finally:
            api.offt_3d_fin(po)
        n1 = counts(CB)
        out.append({"case": case, "rel": err, "fused": fused, "tol": W.tol(case), "counts": {k: n1[k] - n0[k] for k in n0}})
        dist.barrier()
    cpu_world.uninstall()
    json.dump(out, open(os.path.join(outdir, f"gloo_rank{rank}.json"), "w"))
    dist.destroy_process_group()


if __name__ == "__main__":
    gloo_main(json.loads(sys.argv[2]), sys.argv[3])
