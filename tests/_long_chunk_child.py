"""Child process of tests/test_gpu_long_descriptors.py::test_four_step_chunk_loops: four-step descriptors whose work
does not fit one chunk of scratch.  The parent sets OFFT_FOURSTEP_CHUNK_MIB=1 (read once per process); at 8192
double-precision or 16384 single-precision points a chunk then holds 8 lines, and
    ncols=20, nb1=3, nb2=2  runs as column chunks of 8, 8 and 4 per (b2, b1)
    ncols=3,  nb1=5         runs as b1 chunks of 2, 2 and 1
in every flavour and both directions, one of each with a divisible split through block tables, against the CPU
interpreter with the sentinel in every element the pass does not own: a ragged last chunk that stores past its end
shows there.  Prints CHUNKS OK and exits 0, or dies on the first failed assertion."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

ROUTE_PANEL, ROUTE_FOUR_STEP = 1, 4


def main():
    assert os.environ.get("OFFT_FOURSTEP_CHUNK_MIB") == "1", "run by test_four_step_chunk_loops with a 1 MiB window"
    from offt_amd import api
    from test_gpu_descriptors import Desc, layout, run_both, with_tables
    L = api.lib()
    L.offt_hipk_fft_pass.argtypes = [C.POINTER(Desc), C.c_void_p, C.c_void_p, C.c_void_p]
    L.offt_hipk_prepare.argtypes = [C.c_int, C.c_int]
    L.offt_hipk_last_error.restype = C.c_char_p
    L.offt_hipk_pass_route.argtypes = [C.POINTER(Desc), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    CB = C.CDLL(os.path.join(ROOT, "tests", "libcpubackend.so"))
    CB.cpu_backend_run_pass.argtypes = [C.POINTER(Desc), C.c_void_p, C.c_void_p]
    rng = np.random.default_rng(8192)
    ran = 0
    for n, prec in ((8192, api.F64), (16384, api.F32)):
        assert L.offt_hipk_prepare(n, prec) == 0
        ft, ct = (np.float64, np.complex128) if prec == api.F64 else (np.float32, np.complex64)
        tol = 1e-13 if prec == api.F64 else 5e-6
        for ncols, nb1, nb2 in ((20, 3, 2), (3, 5, 1)):
            for case, (inc, outc, direction) in enumerate([(i, o, s) for i in (1, 0) for o in (1, 0) for s in (-1, 1)]):
                d = Desc()
                d.n, d.precision, d.direction, d.ncols, d.nb1, d.nb2 = n, prec, direction, ncols, nb1, nb2
                d.in_contig, d.out_contig, d.variant = inc, outc, -1
                d.scale, d.out_keep = float(rng.choice([1.0, 0.5, 1.0 / n])), int(rng.integers(0, 2))
                # the four-step factors of this length, from a descriptor without a split
                n1, n2 = C.c_int(0), C.c_int(0)
                via = L.offt_hipk_pass_route(C.byref(d), None, C.byref(n1), C.byref(n2))
                if n == 8192 and inc and outc:  # the one-column register kernel: no scratch, nothing to chunk
                    assert via == ROUTE_PANEL, via
                else:
                    assert via == ROUTE_FOUR_STEP and n1.value * n2.value == n, (via, n1.value, n2.value)
                    if case % 4 == 2:  # blocks the decomposition divides by n2 and n1, moved through tables
                        d.in_split, d.out_split = 2 * n2.value, 4 * n1.value
                        assert L.offt_hipk_pass_route(C.byref(d), None, None, None) == ROUTE_FOUR_STEP
                li = layout(rng, n, ncols, nb1, nb2, d.in_split, 0, inc)
                lo = layout(rng, n, ncols, nb1, nb2, d.out_split, 0, outc)
                d.in_axis_stride, d.in_col_stride, d.in_b1_stride, d.in_b2_stride, d.in_block_stride = li["axis"], li["col"], li["b1"], li["b2"], li["blk"]
                d.out_axis_stride, d.out_col_stride, d.out_b1_stride, d.out_b2_stride, d.out_block_stride = lo["axis"], lo["col"], lo["b1"], lo["b2"], lo["blk"]
                nin, nout, tabs = li["total"], lo["total"], [None, None]
                if d.in_split:
                    nin, nout, tabs = with_tables(rng, d, nin, nout)
                src = (rng.standard_normal(nin) + 1j * rng.standard_normal(nin)).astype(ct)
                want, got = run_both(L, CB, d, src, nout, ct, ft, tabs)
                desc = {f: getattr(d, f) for f, _ in Desc._fields_}
                assert np.abs(got - want).max() <= tol * np.abs(want).max() * np.log2(n), desc
                ran += 1
    assert ran == 32
    print("CHUNKS OK", ran)


if __name__ == "__main__":
    main()
