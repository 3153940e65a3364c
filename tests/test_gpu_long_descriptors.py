"""-m gpu: lines longer than the panel kernels take, at DESCRIPTOR level, against the CPU interpreter.

Lines above 4096 points run through two decomposing routes of the launcher: the four-step split n = n1 n2 (four_pass:
three forms of its second sub-pass, twiddles fused into the first one's stores or as a sweep of their own, per-peer
splits divided by n2 and n1) and contiguous scratch lines (long_pass: gather and scatter with every split form).  The
whole-plan tests of tests/test_gpu_parity.py reach them on one rank only: no split, no block table, one batch dimension,
scale 1.  The multi-GPU schedules hand them exactly the descriptors that are missing there, and a one-GPU box can check
those only here (the argument of tests/test_gpu_descriptors.py, for the short lengths).  Three parts: random long
descriptors with the route asserted (offt_hipk_pass_route); the sixteen four-step-twiddle instances launched directly;
the chunk loops of both routes made to iterate (a child process with a 1 MiB four-step window, and one descriptor with
more scratch lines than long_pass's window holds)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from offt_amd import api
from test_gpu_descriptors import Desc, layout, libs, make_case, run_both, with_tables  # noqa: F401 (libs: fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTE_NONE, ROUTE_PANEL, ROUTE_ANY_LENGTH, ROUTE_FOUR_STEP, ROUTE_SCRATCH = 0, 1, 3, 4, 5


def bind_route(L):
    L.offt_hipk_pass_route.argtypes = [C.POINTER(Desc), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]


def route(L, d):
    vid, n1, n2 = C.c_int(-9), C.c_int(-9), C.c_int(-9)
    via = L.offt_hipk_pass_route(C.byref(d), C.byref(vid), C.byref(n1), C.byref(n2))
    return via, vid.value, n1.value, n2.value


def relayout(rng, d):
    """strides for the descriptor's present shape, flavour and splits -> element counts of the two arrays"""
    li = layout(rng, d.n, d.ncols, d.nb1, d.nb2, d.in_split, d.in_split_nfloor, d.in_contig)
    lo = layout(rng, d.n, d.ncols, d.nb1, d.nb2, d.out_split, d.out_split_nfloor, d.out_contig)
    d.in_axis_stride, d.in_col_stride, d.in_b1_stride, d.in_b2_stride, d.in_block_stride = li["axis"], li["col"], li["b1"], li["b2"], li["blk"]
    d.out_axis_stride, d.out_col_stride, d.out_b1_stride, d.out_b2_stride, d.out_block_stride = lo["axis"], lo["col"], lo["b1"], lo["b2"], lo["blk"]
    return li["total"], lo["total"]


def long_case(rng, n, prec, n1, n2, inc, outc, direction):
    """make_case's descriptor (scale, out_keep) in the given flavour and direction with few lines and, per side, no split,
    a divisor of n the four-step route can follow (a multiple of n2 on the load side, of n1 on the store side) or uneven
    F / F+1"""
    d, _, _ = make_case(rng, n, prec)
    d.real_input, d.in_contig, d.out_contig, d.direction = 0, inc, outc, direction
    d.ncols, d.nb1, d.nb2 = int(rng.integers(1, 13)), int(rng.integers(1, 3)), int(rng.integers(1, 3))

    def pick_split(unit):
        kind = int(rng.integers(0, 3))
        if kind == 0:
            return 0, 0
        if kind == 1:
            cands = [f for f in range(unit, n, unit) if n % f == 0]
            return int(rng.choice(cands)), 0
        p = int(rng.integers(2, 10))  # (up to 9 peers: 2 ... 6 all divide 6000 and 12000)
        F, b = n // p, n % p
        return (F, p - b) if b else (F, 0)
    d.in_split, d.in_split_nfloor = pick_split(n2)
    d.out_split, d.out_split_nfloor = pick_split(n1)
    nin, nout = relayout(rng, d)
    return d, nin, nout


# the two decomposing routes per (n, precision).  Uneven blocks go through scratch lines where the any-length kernel
# cannot take the line (above 5120 double / 10240 single points); 5000 and 4076 double and 10000 single points fit it, and
# resolve() leaves their uneven descriptors there: those three lengths cannot show "scratch lines with an uneven split".
LONG = [(8192, api.F64, True), (8192, api.F32, True), (16384, api.F64, True), (16384, api.F32, True), (6000, api.F64, True),
        (5000, api.F64, False), (4076, api.F64, False), (12000, api.F32, True), (10000, api.F32, False)]


@pytest.mark.parametrize("n,prec,scratch_uneven", LONG)
def test_random_long_descriptors(libs, n, prec, scratch_uneven):
    L, CB = libs
    bind_route(L)
    rng = np.random.default_rng(31000 + 2 * n + prec)
    assert L.offt_hipk_prepare(n, prec) == 0
    ft, ct = (np.float64, np.complex128) if prec == api.F64 else (np.float32, np.complex64)
    tol = 1e-13 if prec == api.F64 else 5e-6
    probe, _, _ = make_case(rng, n, prec)
    probe.real_input, probe.in_contig, probe.out_contig = 0, 0, 0
    probe.in_split = probe.in_split_nfloor = probe.out_split = probe.out_split_nfloor = 0
    via, _, n1, n2 = route(L, probe)
    assert via == ROUTE_FOUR_STEP and n1 * n2 == n and n1 > 1 and n2 > 1, (via, n1, n2)
    four_split = scratch = 0
    for it in range(40):  # the four flavours in turn, forward and inverse by turns of four
        d, nin, nout = long_case(rng, n, prec, n1, n2, (it >> 1) & 1, it & 1, 1 if it & 4 else -1)
        tabs = [None, None]
        if it % 2 == 1:
            nin, nout, tabs = with_tables(rng, d, nin, nout)
        desc = {f: getattr(d, f) for f, _ in Desc._fields_}
        via, vid, r1, r2 = route(L, d)
        uneven = d.in_split_nfloor > 0 or d.out_split_nfloor > 0
        follows = not uneven and d.in_split % n2 == 0 and d.out_split % n1 == 0
        both_contig = d.in_contig and d.out_contig
        if n == 8192 and both_contig:  # the one-column register kernel takes what it can address itself
            assert via == (ROUTE_PANEL if follows else ROUTE_SCRATCH if prec == api.F64 else ROUTE_ANY_LENGTH), desc
        elif follows:
            assert (via, r1, r2) == (ROUTE_FOUR_STEP, n1, n2), desc
        else:
            assert via == (ROUTE_SCRATCH if scratch_uneven else ROUTE_ANY_LENGTH), desc
        src = (rng.standard_normal(nin) + 1j * rng.standard_normal(nin)).astype(ct)
        want, got = run_both(L, CB, d, src, nout, ct, ft, tabs)
        assert np.abs(got - want).max() <= tol * np.abs(want).max() * max(1.0, np.log2(n)), desc
        four_split += via == ROUTE_FOUR_STEP and bool(d.in_split or d.out_split)
        scratch += via == ROUTE_SCRATCH and uneven
        if it >= 15 and four_split and (scratch or not scratch_uneven):
            break
    assert four_split >= 1, "no four-step descriptor with a split was drawn"
    assert scratch >= 1 or not scratch_uneven, "no scratch-lines descriptor with an uneven split was drawn"


@pytest.mark.parametrize("prec", [api.F64, api.F32])
@pytest.mark.parametrize("n1", [2, 4, 8, 16, 32, 64, 128, 256])
def test_four_step_twiddle_instances(libs, n1, prec):
    """the strided / strided instances with the long line's twiddles on their stores (Role::TW4), launched as the
    four-step route launches them: tw4[k1][j2] = w^(k1 j2) of n1 n2 points, j2 the column (tw4_b1 = 0) or the b1 entry
    (tw4_b1 = 1).  Reference: the interpreter's result of the same descriptor without the table, times the table (its
    conjugate for the inverse: the kernel multiplies before its conjugating store)."""
    L, CB = libs
    bind_route(L)
    rng = np.random.default_rng(52000 + 2 * n1 + prec)
    assert L.offt_hipk_prepare(n1, prec) == 0
    ft, ct = (np.float64, np.complex128) if prec == api.F64 else (np.float32, np.complex64)
    tol = 1e-13 if prec == api.F64 else 5e-6
    case = 0
    for n2 in (24, 128):
        t = np.exp(-2j * np.pi * np.outer(np.arange(n1), np.arange(n2)) / (n1 * n2)).astype(ct)  # float64, then cast
        # (a tail behind the table: lanes of a ragged last panel form their address before the store is masked)
        dev_t = torch.from_numpy(np.concatenate([t.ravel(), np.zeros(64, dtype=ct)]).view(ft).copy()).cuda()
        for b1_mode in (0, 1):
            for direction in (-1, 1):
                d, _, _ = make_case(rng, n1, prec)
                d.real_input, d.in_contig, d.out_contig, d.direction = 0, 0, 0, direction
                if b1_mode:
                    d.ncols, d.nb1, d.nb2 = int(rng.choice([3, 5, 13])), n2, int(rng.integers(1, 3))
                else:
                    d.ncols, d.nb1, d.nb2 = n2, int(rng.integers(1, 4)), int(rng.integers(1, 3))
                pow2 = [0] + [1 << s for s in range(n1.bit_length() - 1)]
                d.in_split, d.out_split, d.in_split_nfloor, d.out_split_nfloor = int(rng.choice(pow2)), int(rng.choice(pow2)), 0, 0
                nin, nout = relayout(rng, d)
                tabs = [None, None]
                case += 1
                if case % 2 == 0:
                    nin, nout, tabs = with_tables(rng, d, nin, nout)
                desc = {f: getattr(d, f) for f, _ in Desc._fields_}
                src = (rng.standard_normal(nin) + 1j * rng.standard_normal(nin)).astype(ct)
                # reference: without the table on the interpreter, then every stored element times t[k1][j2]
                d.tw4 = None
                want = np.full(nout, 7 - 3j, dtype=ct)
                d.in_block_tab = tabs[0].ctypes.data if tabs[0] is not None else None
                d.out_block_tab = tabs[1].ctypes.data if tabs[1] is not None else None
                assert CB.cpu_backend_run_pass(C.byref(d), src.ctypes.data_as(C.c_void_p), want.ctypes.data_as(C.c_void_p)) == 0
                k = np.arange(n1)
                if d.out_split:
                    blk = tabs[1][k // d.out_split] if tabs[1] is not None else (k // d.out_split) * d.out_block_stride
                    koff = blk + (k % d.out_split) * d.out_axis_stride
                else:
                    koff = k * d.out_axis_stride
                b2, b1, c = np.meshgrid(np.arange(d.nb2), np.arange(d.nb1), np.arange(d.ncols), indexing="ij")
                base = b2 * d.out_b2_stride + b1 * d.out_b1_stride + c * d.out_col_stride      # [b2][b1][c]
                off = base[..., None] + koff                                                   # [b2][b1][c][k1]
                j2 = (b1 if b1_mode else c)[..., None]
                w = t[k[None, None, None, :], j2]
                assert np.all(want[off] != 7 - 3j) and np.unique(off).size == off.size
                want[off] = (want[off].astype(np.complex128) * (np.conj(w) if direction > 0 else w).astype(np.complex128)).astype(ct)
                # the kernel
                d.tw4, d.tw4_b1, d.tw4_n2 = dev_t.data_ptr(), b1_mode, n2
                assert route(L, d)[0] == ROUTE_PANEL, desc
                dt = [torch.from_numpy(x.copy()).cuda() if x is not None else None for x in tabs]
                d.in_block_tab = dt[0].data_ptr() if dt[0] is not None else None
                d.out_block_tab = dt[1].data_ptr() if dt[1] is not None else None
                din = torch.from_numpy(src.view(ft).copy()).cuda()
                dout = torch.from_numpy(np.full(nout, 7 - 3j, dtype=ct).view(ft).copy()).cuda()
                torch.cuda.synchronize()
                rc = L.offt_hipk_fft_pass(C.byref(d), din.data_ptr(), dout.data_ptr(), None)
                assert rc == 0, L.offt_hipk_last_error()
                torch.cuda.synchronize()
                got = dout.cpu().numpy().view(ct)
                assert np.abs(got - want).max() <= tol * np.abs(want).max() * max(1.0, np.log2(n1)), desc
    # the twiddles exist on strided / strided stores only: a contiguous side is refused, not run without them
    for inc, outc in ((1, 0), (0, 1), (1, 1)):
        d, _, _ = make_case(rng, n1, prec)
        d.real_input, d.in_contig, d.out_contig = 0, inc, outc
        d.in_split = d.in_split_nfloor = d.out_split = d.out_split_nfloor = 0
        d.ncols, d.nb1, d.nb2 = 24, 1, 1
        nin, nout = relayout(rng, d)
        d.tw4, d.tw4_b1, d.tw4_n2 = dev_t.data_ptr(), 0, 128
        assert route(L, d)[:2] == (ROUTE_NONE, -1)
        din, dout = torch.zeros(2 * nin, dtype=dev_t.dtype).cuda(), torch.zeros(2 * nout, dtype=dev_t.dtype).cuda()
        assert L.offt_hipk_fft_pass(C.byref(d), din.data_ptr(), dout.data_ptr(), None) != 0
        assert not bool(dout.any())


def test_four_step_chunk_loops():
    """four_pass cuts a pass into chunks of OFFT_FOURSTEP_CHUNK_MIB of scratch, ragged in columns or in b1; the switch is
    read once per process, so the cases (tests/_long_chunk_child.py) run in a child with a 1 MiB window -- once with the
    twiddles fused into the first sub-pass, once with the twiddle sweeps"""
    for extra in ({}, {"OFFT_FOURSTEP_FUSE": "0"}):
        env = dict(os.environ, OFFT_FOURSTEP_CHUNK_MIB="1", **extra)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_long_chunk_child.py")], env=env, timeout=120,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, (extra, r.stdout[-3000:])
        assert "CHUNKS OK" in r.stdout, (extra, r.stdout[-3000:])


def test_scratch_line_chunks(libs):
    """long_pass holds 256 MiB of scratch lines at a time: 1100 lines of 10007 double-precision points (a Bluestein
    convolution on M <= 32768 points, so at most 512 lines fit) run as two or three ragged chunks.  Contiguous in, strided
    out, once forward and once inverse, against numpy along the axis (the oracle's prime lines are O(n^2) sums)."""
    L, _ = libs
    bind_route(L)
    n, ncols, nb1, nb2 = 10007, 11, 10, 10
    assert L.offt_hipk_prepare(n, api.F64) == 0
    rng = np.random.default_rng(10007)
    x = rng.standard_normal((nb2, nb1, ncols, n)) + 1j * rng.standard_normal((nb2, nb1, ncols, n))
    din = torch.from_numpy(x.view(np.float64).copy()).cuda()
    d = Desc()
    d.n, d.precision, d.ncols, d.nb1, d.nb2, d.variant, d.scale = n, api.F64, ncols, nb1, nb2, -1, 1.0
    d.in_contig, d.in_axis_stride, d.in_col_stride, d.in_b1_stride, d.in_b2_stride = 1, 1, n, n * ncols, n * ncols * nb1
    d.out_contig, d.out_axis_stride, d.out_col_stride, d.out_b1_stride, d.out_b2_stride = 0, ncols, 1, n * ncols, n * ncols * nb1
    for direction in (-1, 1):
        d.direction = direction
        assert route(L, d)[:2] == (ROUTE_SCRATCH, -1)
        tail = 16
        dout = torch.from_numpy(np.full(x.size + tail, 7 - 3j, dtype=np.complex128).view(np.float64).copy()).cuda()
        torch.cuda.synchronize()
        rc = L.offt_hipk_fft_pass(C.byref(d), din.data_ptr(), dout.data_ptr(), None)
        assert rc == 0, L.offt_hipk_last_error()
        torch.cuda.synchronize()
        got = dout.cpu().numpy().view(np.complex128)
        assert np.all(got[x.size:] == 7 - 3j)
        got = got[:x.size].reshape(nb2, nb1, n, ncols).transpose(0, 1, 3, 2)
        want = np.fft.fft(x, axis=-1) if direction < 0 else np.fft.ifft(x, axis=-1) * n
        assert np.linalg.norm(got - want) / np.linalg.norm(want) <= 1e-13, direction
