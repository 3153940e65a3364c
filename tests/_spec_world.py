"""Filtered forward and filtered inverse (offt_hip_execute_forward_filtered, offt_hip_execute_inverse_filtered): the pieces
tests/test_spectral_filtered.py shares, and the worlds of several ranks.

  _spec_world.py gloo <cases.json> <outdir>     one gloo rank per PROCESS on the CPU backend of tests/cpu_backend_spec.c
                                                 (tests/libcpubackend_spec.so)
  _spec_world.py <size> <cases.json> <outdir>   ranks as THREADS of one process on the one GPU (the thread-world machinery of
                                                 _c2r_world.py, as _conv_world.py uses it)

A case is a case of _conv_world.py plus "K" (outputs of the inverse) and "inplace" (index of the output that is `spec`, or
None)."""
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
KINDS = {"pass": 0, "filt_fwd": 1, "filt_inv": 2, "pointwise": 3, "pointwise_oop": 4, "memcpy": 5, "zero": 6}


def problem(case, seed=31):
    """global x with a forward filter H0 and the expected SCALE * H0 * fftn(x); a spectrum S with K filters and the expected
    SCALE * N * ifftn(H_k * S) (rfftn / irfftn for r2c)"""
    N, r2c, cplx, K = tuple(case["N"]), bool(case.get("r2c")), bool(case.get("cplx")), int(case.get("K", 3))
    rng = np.random.default_rng(seed + sum(N) + K)
    x = rng.standard_normal(N) if r2c else rng.standard_normal(N) + 1j * rng.standard_normal(N)
    y = rng.standard_normal(N) if r2c else rng.standard_normal(N) + 1j * rng.standard_normal(N)
    hs = (N[0], N[1], N[2] // 2 + 1) if r2c else N
    n = float(np.prod(N))
    fwd = (lambda a: np.fft.rfftn(a, axes=(0, 1, 2))) if r2c else np.fft.fftn
    inv = (lambda a: np.fft.irfftn(a, s=N, axes=(0, 1, 2))) if r2c else np.fft.ifftn
    filt = lambda: rng.standard_normal(hs) + (1j * rng.standard_normal(hs) if cplx else 0.0)
    H0, S, Hs = filt(), fwd(y), [filt() for _ in range(K)]
    return dict(x=x, H0=H0, fwd=SCALE * H0 * fwd(x), S=S, Hs=Hs, inv=[inv(H * S) * n * SCALE for H in Hs],
                conv=[inv(H * H0 * fwd(x)) * n for H in Hs])


def out_buffer(c, ne, case, A):
    """this rank's block of the spectrum A in the forward's output layout"""
    ct = np.complex64 if case.get("f32") else np.complex128
    buf = np.zeros(ne, dtype=ct)
    buf[W.out_index(c)] = HW.out_block(c, A).astype(ct)
    return buf


def out_err(c, got, want):
    w = HW.out_block(c, want)
    if w.size == 0:
        return 0.0
    return float(np.linalg.norm(got[W.out_index(c)].astype(np.complex128) - w) / np.linalg.norm(w))


def kind_of(api, case):
    return api.FILTER_COMPLEX if case.get("cplx") else api.FILTER_REAL


def run_forward(api, po, case, dev, pr=None):
    """the filtered forward on a plan: rel-L2 of this rank's output block against numpy, and the block"""
    L = api.lib()
    c, ne = api.comm_dict(po), api.local_elems(po)
    pr = pr or problem(case)
    data, filt = W.local_arrays(c, ne, case, pr["x"], pr["H0"])
    (hd, pd), (hf, pf) = dev.put(data), dev.put(filt)
    L.offt_hip_set_output_scale(po, SCALE)
    api.offt_hip_execute_forward_filtered(po, pd, pf, kind_of(api, case))
    L.offt_hip_set_output_scale(po, 1.0)
    got = dev.get(hd, data)
    return out_err(c, got, pr["fwd"]), got


def run_inverse(api, po, case, dev, pr=None):
    """the filtered inverse on a plan: rel-L2 of every output, whether the spectrum is bit-identical afterwards (None where it
    is one of the outputs), and the outputs"""
    L = api.lib()
    c, ne = api.comm_dict(po), api.local_elems(po)
    pr = pr or problem(case)
    spec = out_buffer(c, ne, case, pr["S"])
    filts = [W.local_arrays(c, ne, case, pr["x"], H)[1] for H in pr["Hs"]]
    inplace = case.get("inplace")
    hs, ps = dev.put(spec)
    hf = [dev.put(f) for f in filts]
    ho = [(hs, ps) if k == inplace else dev.put(np.full(ne, 3.0 - 2.0j, dtype=spec.dtype)) for k in range(len(filts))]
    L.offt_hip_set_output_scale(po, SCALE)
    api.offt_hip_execute_inverse_filtered(po, ps, [p for _, p in ho], [p for _, p in hf], kind_of(api, case))
    L.offt_hip_set_output_scale(po, 1.0)
    outs = [np.array(dev.get(h, spec), copy=True) for h, _ in ho]
    intact = None if inplace is not None else bool(np.array_equal(dev.get(hs, spec).view(np.uint8), spec.view(np.uint8)))
    return [W.check(c, case, o, w) for o, w in zip(outs, pr["inv"])], intact, outs


def run_compose(api, po, case, dev, pr=None):
    """forward_filtered(x, H0) then inverse_filtered in place with Hs[0], against offt_hip_execute_convolve with H0 * Hs[0] and
    against numpy: (rel-L2 to numpy, rel-L2 between the two library results)"""
    c, ne = api.comm_dict(po), api.local_elems(po)
    pr = pr or problem(case)
    data, f0 = W.local_arrays(c, ne, case, pr["x"], pr["H0"])
    _, f1 = W.local_arrays(c, ne, case, pr["x"], pr["Hs"][0])
    _, f01 = W.local_arrays(c, ne, case, pr["x"], pr["H0"] * pr["Hs"][0])
    (ha, pa), (hb, pb) = dev.put(data), dev.put(data.copy())
    (_h0, p0), (_h1, p1), (_h01, p01) = dev.put(f0), dev.put(f1), dev.put(f01)
    k = kind_of(api, case)
    api.offt_hip_execute_forward_filtered(po, pa, p0, k)
    api.offt_hip_execute_inverse_filtered(po, pa, [pa], [p1], k)
    api.offt_hip_execute_convolve(po, pb, p01, k)
    a, b = np.array(dev.get(ha, data), copy=True), np.array(dev.get(hb, data), copy=True)
    idx = W.in_index(c, bool(case.get("r2c")))
    va, vb = (a.view(a.real.dtype)[idx], b.view(b.real.dtype)[idx]) if case.get("r2c") else (a[idx], b[idx])
    between = float(np.linalg.norm(va.astype(np.complex128) - vb) / np.linalg.norm(vb)) if vb.size else 0.0
    return W.check(c, case, a, pr["conv"][0]), between, a


def spec_cb_lib():
    """tests/libcpubackend_spec.so, shaped like cpu_world's backend library (its table = the spec table)"""
    L = C.CDLL(os.path.join(ROOT, "tests", "libcpubackend_spec.so"))
    for f in ("cpu_backend_spec_table", "cpu_backend_spec_table_nofilt", "cpu_backend_spec_table_old", "cpu_backend_spec_table_none"):
        getattr(L, f).restype = C.c_void_p
    L.cpu_backend_table = L.cpu_backend_spec_table
    L.cpu_backend_spec_count.restype = C.c_long
    L.cpu_backend_spec_count.argtypes = [C.c_int]
    L.cpu_backend_spec_log.argtypes = [C.c_int, C.POINTER(C.c_int)]
    return L


def counts(CB):
    return {k: CB.cpu_backend_spec_count(v) for k, v in KINDS.items()}


def launches(CB):
    """the launches logged since the last reset: (kind, n, direction, ncols, nb1, half, real_input, out_keep, src == dst)"""
    out, rec, i = [], (C.c_int * 9)(), 0
    while CB.cpu_backend_spec_log(i, rec) == 0:
        out.append(tuple(rec))
        i += 1
    return out


# ---- CPU: one gloo rank per process ----------------------------------------------------------------------------------
def gloo_main(cases, outdir):
    import torch.distributed as dist
    import cpu_world
    from offt_amd import api
    rank, size = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=size)
    cpu_world._cb_lib = spec_cb_lib
    out = []
    for case in cases:
        if case.get("p2p"):
            os.environ["OFFT_EXCHANGE"] = "p2p"
        CB = cpu_world.install(rank, size, dist=dist)
        n0 = counts(CB)
        po = HW.make_plan(api, case)
        try:
            ferr, _ = run_forward(api, po, case, HW.Host())
            ierrs, intact, _ = run_inverse(api, po, case, HW.Host())
            fused = api.offt_hip_spectral_fused(po)
        finally:
            api.offt_3d_fin(po)
        n1 = counts(CB)
        out.append({"case": case, "rel": max([ferr] + ierrs), "intact": intact, "fused": fused, "tol": W.tol(case),
                    "counts": {k: n1[k] - n0[k] for k in n0}})
        os.environ.pop("OFFT_EXCHANGE", None)
        dist.barrier()
    cpu_world.uninstall()
    json.dump(out, open(os.path.join(outdir, f"gloo_rank{rank}.json"), "w"))
    dist.destroy_process_group()


# ---- GPU: ranks as threads of one process ------------------------------------------------------------------------------
def gpu_rank(L, api, torch, po, case):
    dev = HW.Gpu(torch)
    ferr, _ = run_forward(api, po, case, dev)
    ierrs, intact, _ = run_inverse(api, po, case, dev)
    assert intact is not False, "the spectrum was written"
    assert not api.offt_hip_spectral_fused(po), "several ranks take the generic route"
    return max([ferr] + ierrs), api.comm_dict(po)


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
