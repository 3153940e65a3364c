"""Pseudo-spectral product on real-input plans (OFFT_HIP_OPT_PROD_REAL): what tests/test_product_real.py and
tests/test_gpu_product_real.py share on top of _prod_world.py, and a gloo world of several ranks.

  _prod_real_world.py gloo <cases.json> <outdir>    one gloo rank per PROCESS on the CPU backend of tests/cpu_backend_prod_real.c
                                                     (tests/libcpubackend_prod_real.so)"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import _conv_world as W  # noqa: E402
import _half_world as HW  # noqa: E402
import _prod_world as PW  # noqa: E402


def real_cb_lib():
    """tests/libcpubackend_prod_real.so, shaped like cpu_world's backend library (its table = the product table with
    prod_pass_real; cpu_backend_prod_table is the table of a backend older than that entry)"""
    L = C.CDLL(os.path.join(ROOT, "tests", "libcpubackend_prod_real.so"))
    for f in ("cpu_backend_prod_table", "cpu_backend_prod_table_old", "cpu_backend_prod_table_nofused", "cpu_backend_prod_real_table"):
        getattr(L, f).restype = C.c_void_p
    L.cpu_backend_table = L.cpu_backend_prod_real_table
    L.cpu_backend_prod_count.restype = C.c_long
    L.cpu_backend_prod_count.argtypes = [C.c_int]
    L.cpu_backend_prod_log.argtypes = [C.c_int, C.POINTER(C.c_int)]
    L.cpu_backend_prod_real_count.restype = C.c_long
    L.cpu_backend_prod_real_log.argtypes = [C.c_int, C.POINTER(C.c_int)]
    L.cpu_backend_alloc_count.restype = C.c_long
    L.cpu_backend_fail_alloc_at.argtypes = [C.c_long]
    return L


def counts(CB):
    return dict(PW.counts(CB), prod_real=CB.cpu_backend_prod_real_count())


def log_reset(CB):
    CB.cpu_backend_prod_log_reset()
    CB.cpu_backend_prod_real_log_reset()


def real_launches(CB):
    """the real fused launches since the last reset: (4, n, direction, ncols, nb1, half, real_input, sources, launches of
    PW.launches(CB) logged before it)"""
    out, rec, i = [], (C.c_int * 9)(), 0
    while CB.cpu_backend_prod_real_log(i, rec) == 0:
        out.append(tuple(rec))
        i += 1
    return out


def gloo_main(cases, outdir):
    import torch.distributed as dist
    import cpu_world
    from offt_amd import api
    rank, size = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=size)
    cpu_world._cb_lib = real_cb_lib
    out = []
    for case in cases:
        CB = cpu_world.install(rank, size, dist=dist)
        n0 = counts(CB)
        po = HW.make_plan(api, case)
        try:
            opts = [api.lib().offt_hip_get_option(po, o) for o in (api.OPT_PROD_FUSED, api.OPT_PROD_REAL)]
            err = PW.run_product(api, po, case, HW.Host())
            fused = api.offt_hip_product_fused(po)
        finally:
            api.offt_3d_fin(po)
        n1 = counts(CB)
        out.append({"case": case, "rel": err, "fused": fused, "opts": opts, "tol": W.tol(case), "counts": {k: n1[k] - n0[k] for k in n0}})
        dist.barrier()
    cpu_world.uninstall()
    json.dump(out, open(os.path.join(outdir, f"gloo_rank{rank}.json"), "w"))
    dist.destroy_process_group()


if __name__ == "__main__":
    gloo_main(json.loads(sys.argv[2]), sys.argv[3])
