"""Shell-binned spectra (offt_hip_spectrum_shells): the numpy reference and the pieces tests/test_spectrum_shells.py shares,
and the gloo worlds of several ranks.

  _shells_world.py gloo <cases.json> <outdir>   one gloo rank per PROCESS on the CPU backend of tests/cpu_backend_shells.c
                                                 (tests/libcpubackend_shells.so)

A case: "N", and optionally "r2c", "f32", "eq", "params" (the plan, as _half_world.make_plan reads them), "kmul", "nbins"
(default: every shell), "data" ("int" or "rand"), "cross"."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import _conv_world as W  # noqa: E402
import _half_world as HW  # noqa: E402

EPS = 2.0 ** -52
POISON = -7.25


def shells(N, kmul=None):
    """the shell of every mode of the full N grid: the s >= 0 with (2s-1)^2 <= 4 K2 < (2s+1)^2 (s = 0: 4 K2 < 1), in integers"""
    km = kmul or (1, 1, 1)
    k = [np.where(2 * np.arange(n) <= n, np.arange(n), np.arange(n) - n).astype(np.int64) * m for n, m in zip(N, km)]
    K2 = k[0][:, None, None] ** 2 + k[1][None, :, None] ** 2 + k[2][None, None, :] ** 2
    s = np.rint(np.sqrt(K2.astype(np.float64))).astype(np.int64)
    for _ in range(4):
        s = s + ((2 * s + 1) ** 2 <= 4 * K2) - ((s > 0) & ((2 * s - 1) ** 2 > 4 * K2))
    assert np.all((s == 0) | ((2 * s - 1) ** 2 <= 4 * K2)) and np.all(4 * K2 < (2 * s + 1) ** 2)
    return s


def max_shell(N, kmul=None):
    return int(shells(N, kmul).max())


def full_spectrum(A, N, r2c):
    """the fftn-shaped spectrum: A itself, or the Nz/2+1 half rebuilt by Hermitian symmetry"""
    if not r2c:
        return A
    Nx, Ny, Nz = N
    F = np.zeros(N, dtype=np.complex128)
    F[:, :, :Nz // 2 + 1] = A
    ix, iy = (-np.arange(Nx)) % Nx, (-np.arange(Ny)) % Ny
    for kz in range(Nz // 2 + 1, Nz):
        F[:, :, kz] = np.conj(A[ix][:, iy][:, :, Nz - kz])
    return F


def reference(A, B, N, r2c, kmul, nbins):
    """np.bincount over the full spectrum: (sums, counts, sum of w |A| |B|), each of nbins entries, modes of shells >= nbins
    left out"""
    FA, FB = full_spectrum(A.astype(np.complex128), N, r2c), full_spectrum(B.astype(np.complex128), N, r2c)
    s = shells(N, kmul).ravel()
    keep = s < nbins
    term = (FA * np.conj(FB)).real.ravel()
    mag = (np.abs(FA) * np.abs(FB)).ravel()
    sums = np.bincount(s[keep], weights=term[keep], minlength=nbins)
    counts = np.bincount(s[keep], minlength=nbins)
    absw = np.bincount(s[keep], weights=mag[keep], minlength=nbins)
    return sums, counts.astype(np.int64), absw


def bound(counts, absw):
    """twice the standard bound for summing n terms in double, once for each side of the comparison"""
    return 2.0 * (counts + 4) * EPS * absw


def spectra(case, seed=5):
    """the global spectra A and B of a case (the half spectrum for r2c), already rounded to the plan's precision"""
    N, r2c = tuple(case["N"]), bool(case.get("r2c"))
    hs = (N[0], N[1], N[2] // 2 + 1) if r2c else N
    rng = np.random.default_rng(seed + sum(N))
    ct = np.complex64 if case.get("f32") else np.complex128
    if case.get("data", "int") == "int":
        A = rng.integers(-8, 9, hs) + 1j * rng.integers(-8, 9, hs)
        B = rng.integers(-8, 9, hs) + 1j * rng.integers(-8, 9, hs)
    else:
        A = rng.standard_normal(hs) + 1j * rng.standard_normal(hs)
        B = rng.standard_normal(hs) + 1j * rng.standard_normal(hs)
    return A.astype(ct), B.astype(ct)


def nbins_of(case):
    return int(case.get("nbins") or max_shell(case["N"], case.get("kmul")) + 1)


def local_buffer(c, ne, A):
    """this rank's block of the global spectrum A in the forward's output layout (the padding poisoned)"""
    buf = np.full(ne, 1e30 + 1e30j, dtype=A.dtype)
    buf[W.out_index(c)] = HW.out_block(c, A)
    return buf


def call(api, po, case, dev, A, B=None, counts=True, nbins=None):
    """the call on this rank's block of A (and B): (sums, counts or None, whether a and b are bit-identical afterwards)"""
    c, ne = api.comm_dict(po), api.local_elems(po)
    nb = nbins or nbins_of(case)
    a = local_buffer(c, ne, A)
    b = local_buffer(c, ne, B) if B is not None else None
    ha, pa = dev.put(a)
    hb, pb = dev.put(b) if b is not None else (None, None)
    hs, ps = dev.put(np.full(nb, POISON))
    hc, pc = dev.put(np.full(nb, -3, dtype=np.int64)) if counts else (None, None)
    api.offt_hip_spectrum_shells(po, pa, pb, nb, ps, pc, kmul=case.get("kmul"))
    sums = np.array(dev.get(hs, np.zeros(1)), copy=True)
    cnt = np.array(dev.get(hc, np.zeros(1, dtype=np.int64)), copy=True) if counts else None
    same = np.array_equal(dev.get(ha, a).view(np.uint8), a.view(np.uint8))
    if b is not None:
        same = same and np.array_equal(dev.get(hb, b).view(np.uint8), b.view(np.uint8))
    return sums, cnt, bool(same)


def check(case, sums, cnt, A, B=None):
    """exact for integer data, the bound for random data; counts exact"""
    N, nb = tuple(case["N"]), len(sums)
    rs, rc, rw = reference(A, A if B is None else B, N, bool(case.get("r2c")), case.get("kmul"), nb)
    if cnt is not None:
        assert np.array_equal(cnt, rc), (case, cnt, rc)
    if case.get("data", "int") == "int":
        assert np.array_equal(sums, rs), (case, np.flatnonzero(sums != rs)[:8])
    else:
        err, lim = np.abs(sums - rs), bound(rc, rw)
        assert np.all(err <= lim), (case, np.flatnonzero(err > lim)[:8], err.max())


def shells_cb_lib():
    """tests/libcpubackend_shells.so, shaped like cpu_world's backend library (its table = the shells table)"""
    L = C.CDLL(os.path.join(ROOT, "tests", "libcpubackend_shells.so"))
    for f in ("cpu_backend_shells_table", "cpu_backend_spec_table"):
        getattr(L, f).restype = C.c_void_p
    L.cpu_backend_table = L.cpu_backend_shells_table
    L.cpu_backend_shells_calls.restype = C.c_long
    L.cpu_backend_spec_count.restype = C.c_long
    L.cpu_backend_spec_count.argtypes = [C.c_int]
    L.cpu_backend_spec_log.argtypes = [C.c_int, C.POINTER(C.c_int)]
    return L


# ---- CPU: one gloo rank per process ----------------------------------------------------------------------------------
def gloo_main(cases, outdir):
    import torch.distributed as dist
    import cpu_world
    from offt_amd import api
    rank, size = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=size)
    cpu_world._cb_lib = shells_cb_lib
    cpu_world.install(rank, size, dist=dist)
    out = []
    for case in cases:
        po = HW.make_plan(api, case)
        try:
            A, B = spectra(case)
            sums, cnt, same = call(api, po, case, HW.Host(), A, B if case.get("cross") else None)
            c = api.comm_dict(po)
        finally:
            api.offt_3d_fin(po)
        out.append({"case": case, "sums": [float(v) for v in sums], "counts": [int(v) for v in cnt], "intact": same,
                    "osize": c["osize"], "ostart": c["ostart"]})
        dist.barrier()
    cpu_world.uninstall()
    json.dump(out, open(os.path.join(outdir, f"shells_rank{rank}.json"), "w"))
    dist.destroy_process_group()


if __name__ == "__main__":
    gloo_main(json.loads(sys.argv[2]), sys.argv[3])
