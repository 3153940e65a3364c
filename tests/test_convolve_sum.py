"""Multi-input spectral convolution: offt_hip_execute_convolve_sum (several forwards, one inverse).

  * routing of the gather launch without a device (offt_hipk_conv_sum_kernel_name);
  * the host's routes on the CPU backend of tests/cpu_backend_sum.c, read off its launch log: every single-rank layout,
    complex and r2c plans, real and complex filters, `out` separate and `out` one of the inputs, plane groups, older backend
    tables, gloo worlds of 2 and 4 ranks, refusals, the single-input equivalence, half boxes;
  * -m gpu: random gather descriptors against numpy (every source bit-identical afterwards, sentinels, half lines, the
    cache-keeping twin, dst one of the sources), the multiply-and-sum sweep, one rank through the API on both routes, a
    pruned half box, the pressure projection of a vector field, refusals of host memory, a thread-rank world of 2 under the
    direct-store exchange.

The expected value is numpy's sum_k ifftn(H_k fftn(x_k)) N scale; every test first asserts on the numpy side that the sum
does not cancel (its norm is at least that of its largest term).  Tolerances are the project's own: 1e-12 / 1e-5 rel-L2 at
kernel level (test_multi_random_oop_descriptors), W.tol (1e-12 f64, 2e-5 f32) at plan level."""
import ctypes as C
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import _conv_sum_world as SW
import _conv_world as W
import _half_world as HW
from offt_amd import api
from test_convolve_multi import CPU_CASES, Desc, FDesc, conv_desc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PP = C.POINTER(C.c_void_p)


def ptrs(ps):
    return (C.c_void_p * max(len(ps), 1))(*ps)


@pytest.fixture(scope="module")
def kl(built):
    L = api.lib()
    L.offt_hipk_conv_sum_kernel_name.restype = C.c_char_p
    L.offt_hipk_conv_sum_kernel_name.argtypes = [C.POINTER(Desc), C.POINTER(FDesc)]
    L.offt_hipk_conv_has_fused_sum.argtypes = [C.POINTER(Desc), C.POINTER(FDesc)]
    L.offt_hipk_conv_pass_sum.argtypes = [C.POINTER(Desc), C.POINTER(FDesc), C.c_int, PP, PP, C.c_void_p, C.c_void_p]
    L.offt_hipk_pointwise_sum.argtypes = [C.c_int, PP, PP, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong,
                                          C.c_longlong, C.c_longlong, C.c_void_p]
    L.offt_hipk_prepare.argtypes = [C.c_int, C.c_int]
    L.offt_hipk_last_error.restype = C.c_char_p
    return L


# ---- 1. routing without a device ------------------------------------------------------------------------------------------
def test_sum_kernel_routing_without_a_gpu(kl):
    L = kl
    name = lambda d, f: L.offt_hipk_conv_sum_kernel_name(C.byref(d), C.byref(f)).decode()
    for prec in (api.F64, api.F32):
        for n in (64, 128, 256, 512, 1024):              # (no instance spills, none is dropped)
            for kind in (0, 1):
                for half, want in ((0, "fft_conv_sum_panel_k"), (3, "fft_conv_sum_half_panel_k")):
                    d, f = conv_desc(n, prec, 8, 2, kind=kind, half=half)
                    assert name(d, f) == want, (n, prec, kind, half)
                    assert L.offt_hipk_conv_has_fused_sum(C.byref(d), C.byref(f)) == 1
        for n in (32, 48, 1000, 2048):
            for mixed in (0, 1, 3):                      # (1000 has single-input mixed-radix kernels, but no gather kernel)
                d, f = conv_desc(n, prec, 8, 2)
                f.mixed = mixed
                assert name(d, f) == "no fused kernel", (n, prec, mixed)
                assert L.offt_hipk_conv_has_fused_sum(C.byref(d), C.byref(f)) == 0
        d, f = conv_desc(1024, prec, 8, 2)
        f.axis_stride = 8                                # strided filter axis
        assert name(d, f) == "no fused kernel"
        d, f = conv_desc(1024, prec, 8, 2)
        d.in_contig, d.in_axis_stride, d.in_col_stride = 0, 8, 1  # strided lines
        assert name(d, f) == "no fused kernel"
        d, f = conv_desc(1024, prec, 8, 2)
        d.in_split = 256                                 # a split line
        assert name(d, f) == "no fused kernel"
        for half in (1, 2):                              # half lines: loads and stores together, or not at all
            d, f = conv_desc(1024, prec, 8, 2, half=half)
            assert name(d, f) == "no fused kernel"
        # nin out of range: refused before anything is launched
        d, f = conv_desc(64, prec, 8, 2)
        buf = np.zeros(4096, dtype=np.complex128)
        nine = ptrs([buf.ctypes.data] * 9)
        for nin in (0, 9):
            assert L.offt_hipk_conv_pass_sum(C.byref(d), C.byref(f), nin, nine, nine, buf.ctypes.data, None) == -1
            assert "nin" in L.offt_hipk_last_error().decode()


# ---- CPU tier ---------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def sum_cpu(built):
    import cpu_world
    subprocess.check_call(["make", "-s", "-C", ROOT, "tests/libcpubackend_sum.so"])
    orig = cpu_world._cb_lib
    cpu_world._cb_lib = SW.sum_cb_lib
    CB = cpu_world.install(0, 1, p1=1)
    yield CB
    cpu_world.uninstall()
    cpu_world._cb_lib = orig


def _run_counted(CB, case, opts=(), keep=None):
    """plan + sum call on the installed backend: (error, fused route?, launch counts, launch log); keep["got"]: the output"""
    po = HW.make_plan(api, case)
    try:
        for o, v in opts:
            assert api.lib().offt_hip_set_option(po, o, v) == 0
        if case.get("half"):
            api.offt_hip_set_half_box(po, True)
        n0 = SW.counts(CB)
        CB.cpu_backend_sum_log_reset()
        err = SW.run_sum(api, po, case, HW.Host(), keep=keep)
        n1 = SW.counts(CB)
        return err, api.offt_hip_convolve_sum_fused(po), {k: n1[k] - n0[k] for k in n0}, SW.launches(CB)
    finally:
        api.offt_3d_fin(po)


def _assert_route(case, fused, cnt, log, groups=1):
    K = case.get("K", 3)
    if fused:
        fwd = [r for r in log if r[0] == 0 and r[2] < 0]
        inv = [r for r in log if r[0] == 0 and r[2] > 0]
        assert len(fwd) == K + (K - 1) + groups, (case, fwd)     # z per input, y per input -- the last one per group
        assert len(inv) == groups + 1, (case, inv)               # y per group and z, ONCE
        gather = [r for r in log if r[0] == 2]
        assert len(gather) == groups and all(r[7] == K for r in gather), (case, gather)
        assert cnt["pointwise"] == 0 and cnt["pointwise_sum"] == 0 and cnt["memcpy"] == 0 and cnt["conv"] == 0, (case, cnt)
        # the order: every forward z / y of the earlier inputs, then per group y, gather, inverse y; the inverse z last
        tail = [(r[0], r[2]) for r in log[-(3 * groups + 1):]]
        assert tail == [(0, -1), (2, -1), (0, 1)] * groups + [(0, 1)], (case, tail)
    else:
        assert cnt["conv_sum"] == 0 and cnt["conv"] == 0, (case, cnt)
        assert cnt["pointwise_sum"] == 1 and cnt["pointwise"] == 0 and cnt["memcpy"] == 0, (case, cnt)
        assert cnt["pass"] == 3 * (K + 1), (case, cnt)           # K forwards, one inverse
        assert [r[7] for r in log if r[0] == 4] == [K], (case, log)


# ---- 2. single rank against numpy, the route read off the launches ----------------------------------------------------
@pytest.mark.parametrize("shape,lay", CPU_CASES)
@pytest.mark.parametrize("r2c", [0, 1])
def test_sum_single_rank_cpu(sum_cpu, shape, lay, r2c):
    for cplx in (0, 1):
        for inplace in (None, 0, 2):
            case = dict(N=list(shape), r2c=r2c, cplx=cplx, K=3, inplace=inplace, **lay)
            err, fused, cnt, log = _run_counted(sum_cpu, case)
            assert err <= 1e-12, (case, err)
            _assert_route(case, fused, cnt, log)
            if not lay and shape[0] in (64, 128):
                assert fused, "power-of-two x lines of the z-y-x layout take the fused route"
            if lay or shape[0] == 12:
                assert not fused, case


# ---- 3. single precision ----------------------------------------------------------------------------------------------
def test_sum_single_rank_cpu_f32(sum_cpu):
    case = dict(N=[64, 8, 16], f32=1, cplx=1, K=3)
    err, fused, cnt, log = _run_counted(sum_cpu, case)
    assert fused and err <= 2e-5, err
    _assert_route(case, fused, cnt, log)


# ---- 4. plane groups ----------------------------------------------------------------------------------------------------
def test_sum_plane_groups_cpu(sum_cpu):
    """1 MiB groups on 1024 x 24 planes (384 KiB each in double): 2 planes per group, 13 planes -> 7 groups, the last ragged"""
    for r2c, groups in ((0, 7), (1, 4)):  # (r2c: 13 // 2 + 1 = 7 planes)
        case = dict(N=[1024, 24, 13], r2c=r2c, K=2, inplace=0)
        err, fused, cnt, log = _run_counted(sum_cpu, case, opts=[(0, 1)])
        assert fused and err <= 1e-12, err
        _assert_route(case, fused, cnt, log, groups=groups)
        assert [r[4] for r in log if r[0] == 2] == [2] * (groups - 1) + [1], log   # planes per gather launch: none lost
        case = dict(N=[1024, 24, 13], r2c=r2c, K=2)
        err, fused, cnt, log = _run_counted(sum_cpu, case, opts=[(0, 0)])          # option 0: plain launches
        assert fused and err <= 1e-12, err
        _assert_route(case, fused, cnt, log, groups=1)


# ---- 5. backends without the new entries ------------------------------------------------------------------------------------
def test_sum_older_backend_tables_cpu(sum_cpu):
    CB = sum_cpu
    L = api.lib()
    for shape in ((64, 8, 16), (12, 10, 9)):
        for inplace in (None, 1):
            case = dict(N=list(shape), cplx=1, K=3, inplace=inplace)
            keep_full, keep_gen = {}, {}
            po = HW.make_plan(api, case)
            try:
                assert SW.run_sum(api, po, case, HW.Host(), keep=keep_full) <= 1e-12
            finally:
                api.offt_3d_fin(po)
            L.offt_hip_test_set_backend(CB.cpu_backend_sum_table_nofused(), 0, 1)   # no gather launch: the generic route
            err, fused, cnt, log = _run_counted(CB, case, keep=keep_gen)
            assert not fused and err <= 1e-12, err
            _assert_route(case, False, cnt, log)
            L.offt_hip_test_set_backend(CB.cpu_backend_sum_table(), 0, 1)
            # the same results: both tables evaluate one formula in f64 and differ in the order of operations alone, which
            # is worth eps log2(N) ~ 2.2e-16 x 13 = 3e-15 rel-L2; 1e-13 is the project's bound for two f64 evaluations
            a, b = keep_full["got"], keep_gen["got"]
            assert np.linalg.norm(a - b) <= 1e-13 * np.linalg.norm(a), (shape, inplace, np.linalg.norm(a - b) / np.linalg.norm(a))
    # no multiply-and-sum at all: refused, the marker set
    L.offt_hip_test_set_backend(CB.cpu_backend_sum_table_old(), 0, 1)
    po = api.offt_3d_init(64, 8, 16)
    try:
        n = api.local_elems(po)
        a, b, o, h = (np.zeros(n, dtype=np.complex128) for _ in range(4))
        CB.cpu_backend_sum_log_reset()
        with pytest.raises(RuntimeError, match="multiply-and-sum"):
            api.offt_hip_execute_convolve_sum(po, [a.ctypes.data, b.ctypes.data], [h.ctypes.data] * 2, o.ctypes.data, api.FILTER_COMPLEX)
        assert po.contents.t[api.ALL] >= 99999999.0 and SW.launches(CB) == []
        L.offt_hip_test_set_backend(CB.cpu_backend_sum_table(), 0, 1)
    finally:
        api.offt_3d_fin(po)


# ---- 6. gloo worlds ---------------------------------------------------------------------------------------------------------
def _gloo(size, cases, tmp_path):
    subprocess.check_call(["make", "-s", "-C", ROOT, "tests/libcpubackend_sum.so"])
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    procs = []
    for r in range(size):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(size), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_conv_sum_world.py"), "gloo", json.dumps(cases),
                                       str(tmp_path)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = [p.communicate(timeout=900)[0].decode() for p in procs]
    for r, p in enumerate(procs):
        assert p.returncode == 0, f"rank {r}:\n{outs[r][-3000:]}"
    for r in range(size):
        for rec in json.load(open(tmp_path / f"gloo_rank{r}.json")):
            assert rec["rel"] <= rec["tol"], (r, rec)
            cnt = rec["counts"]
            assert not rec["fused"] and cnt["conv_sum"] == 0 and cnt["conv"] == 0, rec   # several ranks: the generic route
            assert cnt["pointwise_sum"] == 1 and cnt["pointwise"] == 0, rec


def test_sum_gloo_world2(built, tmp_path):
    _gloo(2, [dict(N=[16, 16, 16], K=2), dict(N=[16, 12, 10], r2c=1, cplx=1, K=2, inplace=1),
              dict(N=[8, 8, 8], params={"S": 1}, cplx=1, K=2), dict(N=[16, 16, 8], eq=1, r2c=1, K=2, inplace=0)], tmp_path)


def test_sum_gloo_world4(built, tmp_path):
    _gloo(4, [dict(N=[16, 16, 16], params={"P1": 2}, K=2), dict(N=[16, 16, 16], params={"P1": 2}, r2c=1, cplx=1, K=2, inplace=0),
              dict(N=[16, 16, 32], K=2, inplace=1), dict(N=[16, 12, 10], r2c=1, K=2)], tmp_path)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------
def _call(L, po, ins, filts, kind, out, nin=None):
    n = len(ins)
    return L.offt_hip_execute_convolve_sum(po, n if nin is None else nin, ptrs(ins), ptrs(filts), kind, out)


def test_sum_refusals_cpu(sum_cpu):
    CB = sum_cpu
    L = api.lib()
    po = api.offt_3d_init(64, 8, 16)
    try:
        ne = api.local_elems(po)
        a, b, o, h = (np.zeros(ne, dtype=np.complex128) for _ in range(4))
        A, B, O, H = (x.ctypes.data for x in (a, b, o, h))
        CB.cpu_backend_sum_log_reset()

        def refused(rc, word):
            assert rc == -1 and word in L.offt_hip_last_error().decode() and po.contents.t[api.ALL] >= 99999999.0, \
                (rc, word, L.offt_hip_last_error())
            po.contents.t[api.ALL] = 0.0

        refused(_call(L, po, [], [], api.FILTER_REAL, O), "nin")
        refused(_call(L, po, [A], [H], api.FILTER_REAL, O, nin=-1), "nin")
        nine = [np.zeros(ne, dtype=np.complex128) for _ in range(api.CONV_MAX_IN + 1)]
        refused(_call(L, po, [x.ctypes.data for x in nine], [H] * len(nine), api.FILTER_REAL, O), "nin")
        refused(L.offt_hip_execute_convolve_sum(po, 1, None, None, api.FILTER_REAL, O), "NULL")
        refused(_call(L, po, [A, None], [H, H], api.FILTER_REAL, O), "input 1")
        refused(_call(L, po, [A, B], [H, None], api.FILTER_REAL, O), "filter 1")
        refused(_call(L, po, [A, B], [H, H], api.FILTER_REAL, None), "output")
        refused(_call(L, po, [A, B, A], [H, H, H], api.FILTER_REAL, O), "same array")
        refused(_call(L, po, [A], [H], 2, O), "filter_kind")
        refused(_call(L, po, [A], [H], -1, O), "filter_kind")
        assert SW.launches(CB) == [], "a refusal launches nothing"
        # not covered: the refusal after a failed communicator ((uses_rccl || p2p) && comm_failed).  It needs a world of several
        # ranks whose exchange has failed, which no backend of the suite can bring about on purpose.
    finally:
        api.offt_3d_fin(po)
    # the plan still works after a refusal (and the Python wrapper raises on one)
    po = api.offt_3d_init(64, 8, 16)
    try:
        with pytest.raises(RuntimeError, match="nin"):
            api.offt_hip_execute_convolve_sum(po, [], [], O, api.FILTER_REAL)
        with pytest.raises(ValueError):
            api.offt_hip_execute_convolve_sum(po, [A], [], O, api.FILTER_REAL)
        assert SW.run_sum(api, po, dict(N=[64, 8, 16], K=2), HW.Host()) <= 1e-12
    finally:
        api.offt_3d_fin(po)


# ---- 8. one input, in place: the single-output call ------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(64, 8, 16), (12, 10, 9)])
def test_sum_one_input_in_place_is_convolve_cpu(sum_cpu, shape):
    CB = sum_cpu
    case = dict(N=list(shape), cplx=1, K=1, inplace=0)
    po = HW.make_plan(api, case)
    try:
        c, ne = api.comm_dict(po), api.local_elems(po)
        xs, Hs, _ = SW.problem(case)
        d, f = W.local_arrays(c, ne, case, xs[0], Hs[0])
        one, two = d.copy(), d.copy()
        api.lib().offt_hip_set_output_scale(po, 0.5)
        CB.cpu_backend_sum_log_reset()
        api.offt_hip_execute_convolve(po, one.ctypes.data, f.ctypes.data, api.FILTER_COMPLEX)
        ref_log = [r[:7] for r in SW.launches(CB)]
        CB.cpu_backend_sum_log_reset()
        api.offt_hip_execute_convolve_sum(po, [two.ctypes.data], [f.ctypes.data], two.ctypes.data, api.FILTER_COMPLEX)
        assert [r[:7] for r in SW.launches(CB)] == ref_log and all(r[0] not in (2, 4) for r in SW.launches(CB))
        assert one.tobytes() == two.tobytes()
    finally:
        api.offt_3d_fin(po)


# ---- 9. half box ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,pruned", [(dict(N=[64, 64, 64], cplx=1), True), (dict(N=[64, 64, 64], r2c=1), True),
                                         (dict(N=[64, 64, 64], r2c=1, off=1), False), (dict(N=[12, 10, 8], cplx=1), False),
                                         (dict(N=[12, 10, 8], r2c=1, inplace=1), False), (dict(N=[64, 64, 64], inplace=0), True)])
def test_sum_half_box_cpu(sum_cpu, case, pruned):
    CB = sum_cpu
    case = dict(case, K=2, half=1)
    opts = [(api.OPT_HALF_R2C, 1)] if case.get("r2c") and not case.get("off") else []
    po = HW.make_plan(api, case)
    try:
        for o, v in opts:
            assert api.lib().offt_hip_set_option(po, o, v) == 0
        api.offt_hip_set_half_box(po, True)
        assert api.offt_hip_half_box_pruned(po) == pruned
        n0 = SW.counts(CB)
        CB.cpu_backend_sum_log_reset()
        err = SW.run_sum(api, po, case, HW.Host())
        assert err <= 1e-12, (case, err)
        n1 = SW.counts(CB)
        cnt = {k: n1[k] - n0[k] for k in n0}
        log = SW.launches(CB)
        fused = api.offt_hip_convolve_sum_fused(po)
        assert fused == (case["N"][0] == 64)
        _assert_route(case, fused, cnt, [r for r in log if r[0] != 6])
        if pruned:   # every launch of a pruned plan is a half-line launch, the gather launch in the half = 3 form
            assert cnt["zero"] == 0 and all(r[5] == (3 if r[0] == 2 else r[5]) and r[5] != 0 for r in log), log
        else:        # every input is cleared
            assert cnt["zero"] == case["K"], cnt
            if case["N"][0] == 12:
                assert not fused
    finally:
        api.offt_3d_fin(po)


# ---- GPU tier ---------------------------------------------------------------------------------------------------------------
# ---- 10. random gather descriptors -----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [64, 128, 256, 512, 1024])   # every registered length (256: two-stage 16 x 16 packed; 1024: split images in f64)
def test_sum_random_gather_descriptors(kl, n):
    import torch
    L = kl
    rng = np.random.default_rng(2300 + n)
    SENT = 8  # sentinel elements on either side of every array
    alias_done = {api.F64: False, api.F32: False}
    for prec in (api.F64, api.F32):
        assert L.offt_hipk_prepare(n, prec) == 0
        ft, ct = (np.float64, np.complex128) if prec == api.F64 else (np.float32, np.complex64)
        combo = (n // 64 + (prec == api.F32)) % 4        # nin cycles over the 8 combinations: each of 1, 2, 3, 8 twice
        for kind in (0, 1):
            for half in (0, 3):
                for keep in (0, 1):
                    K = (1, 2, 3, 8)[combo % 4]
                    combo += 3                           # (the start moves with n and the precision)
                    ncols = int(rng.choice([3, 13, 21]))      # never a whole number of panels
                    nb1 = int(rng.integers(2, 4))
                    pad, fpad = int(rng.integers(0, 3)), int(rng.integers(0, 3))
                    scale = float(rng.choice([0.5, 1.0 / n, 3.0]))
                    d, f = conv_desc(n, prec, ncols, nb1, pad=pad, fpad=fpad, kind=kind, scale=scale, half=half, keep=keep)
                    nel = d.in_b1_stride * nb1 + 16
                    nf = f.b1_stride * nb1 + 16
                    nio = n // 2 if half else n
                    xs = [(rng.standard_normal(nel) + 1j * rng.standard_normal(nel)).astype(ct) for _ in range(K)]
                    hs = [(rng.standard_normal(nf) + 1j * rng.standard_normal(nf)) if kind else rng.standard_normal(nf) for _ in range(K)]
                    lines = np.zeros(nel, dtype=bool)         # what the launch may write
                    terms = [np.zeros(nel, dtype=np.complex128) for _ in range(K)]
                    for b1 in range(nb1):
                        for c in range(ncols):
                            i = b1 * d.in_b1_stride + c * d.in_col_stride
                            fo = b1 * f.b1_stride + c * f.col_stride
                            for k in range(K):
                                H = hs[k][fo:fo + n].astype(ct if kind else ft).astype(np.complex128)
                                xin = xs[k][i:i + n].astype(np.complex128)
                                if half:
                                    xin[n // 2:] = 0.0
                                    xs[k][i + n // 2:i + n] = np.nan + 1j * np.nan   # the upper halves must not be read
                                terms[k][i:i + nio] = (np.fft.ifft(H * np.fft.fft(xin)) * n * scale)[:nio]
                            lines[i:i + nio] = True
                    want = sum(terms[1:], terms[0])
                    assert np.linalg.norm(want[lines]) >= max(np.linalg.norm(t[lines]) for t in terms), "the sum cancels"
                    srcs = []
                    for x in xs:
                        s = np.full(nel + 2 * SENT, 7.0 + 7.0j, dtype=ct)
                        s[SENT:SENT + nel] = x
                        srcs.append(s)
                    dst = np.full(nel + 2 * SENT, -5.0 + 9.0j, dtype=ct)
                    ds = [torch.from_numpy(s.view(ft).copy()).cuda() for s in srcs]
                    dd = torch.from_numpy(dst.view(ft).copy()).cuda()
                    dh = [torch.from_numpy((h.astype(ct).view(ft) if kind else h.astype(ft)).copy()).cuda() for h in hs]
                    torch.cuda.synchronize()
                    sp = ptrs([t.data_ptr() + SENT * dst.itemsize for t in ds])
                    fp = ptrs([t.data_ptr() for t in dh])
                    tag = (n, prec, kind, half, keep, K)
                    rc = L.offt_hipk_conv_pass_sum(C.byref(d), C.byref(f), K, fp, sp, dd.data_ptr() + SENT * dst.itemsize, None)
                    assert rc == 0, L.offt_hipk_last_error()
                    torch.cuda.synchronize()
                    for k in range(K):
                        assert ds[k].cpu().numpy().tobytes() == srcs[k].view(ft).tobytes(), ("a source was written", tag, k)
                    got = dd.cpu().numpy().view(ct)
                    assert np.all(got[:SENT] == dst[:SENT]) and np.all(got[SENT + nel:] == dst[SENT + nel:]), ("sentinel overwritten", tag)
                    mid = got[SENT:SENT + nel]
                    assert np.all(mid[~lines] == dst[SENT:SENT + nel][~lines]), ("padding or upper halves written", tag)
                    err = np.linalg.norm(mid[lines].astype(np.complex128) - want[lines]) / np.linalg.norm(want[lines])
                    print("gather descriptor", tag, "rel-L2", err)
                    assert err <= (1e-12 if prec == api.F64 else 1e-5), (tag, err)
                    if not alias_done[prec] and K >= 2:
                        # dst == srcs[j]: the other sources stay untouched, the lines are what they were out of place, and
                        # whatever else srcs[j] held (padding, NaN upper halves, sentinels) stays as it was
                        alias_done[prec] = True
                        j = int(rng.integers(0, K))
                        rc = L.offt_hipk_conv_pass_sum(C.byref(d), C.byref(f), K, fp, sp, sp[j], None)
                        assert rc == 0, L.offt_hipk_last_error()
                        torch.cuda.synchronize()
                        for k in range(K):
                            if k != j:
                                assert ds[k].cpu().numpy().tobytes() == srcs[k].view(ft).tobytes(), ("a source was written", tag, k, j)
                        gj = ds[j].cpu().numpy().view(ct)
                        full = np.zeros(nel + 2 * SENT, dtype=bool)
                        full[SENT:SENT + nel] = lines
                        assert gj[~full].tobytes() == srcs[j][~full].tobytes(), ("in place: more than the lines written", tag, j)
                        assert gj[full].tobytes() == mid[lines].tobytes(), ("in place differs from out of place", tag, j)
    assert all(alias_done.values())


# ---- 11. the multiply-and-sum sweep ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_sum_pointwise_sum_gpu(kl):
    import torch
    L = kl
    rng = np.random.default_rng(77)
    n0, n1, n2 = 5, 7, 24
    s2, s1 = 1, n2 + 2
    s0 = s1 * n1 + 6
    SENT, nel = 8, s0 * n0
    idx = (np.arange(n0)[:, None, None] * s0 + np.arange(n1)[None, :, None] * s1 + np.arange(n2)[None, None, :] * s2).ravel()
    for prec in (api.F64, api.F32):
        ft, ct = (np.float64, np.complex128) if prec == api.F64 else (np.float32, np.complex64)
        for kind in (0, 1):
            for K in (1, 3, 8):
                for alias in (False, True):
                    xs = [(rng.standard_normal(nel) + 1j * rng.standard_normal(nel)).astype(ct) for _ in range(K)]
                    hs = [((rng.standard_normal(nel) + 1j * rng.standard_normal(nel)).astype(ct) if kind
                           else rng.standard_normal(nel).astype(ft)) for _ in range(K)]
                    terms = [x[idx].astype(np.complex128) * h[idx].astype(np.complex128) for x, h in zip(xs, hs)]
                    want = sum(terms[1:], terms[0])
                    bufs = []
                    for x in xs:
                        b = np.full(nel + 2 * SENT, 7.0 + 7.0j, dtype=ct)
                        b[SENT:SENT + nel] = x
                        bufs.append(b)
                    out = np.full(nel + 2 * SENT, -5.0 + 9.0j, dtype=ct)
                    db = [torch.from_numpy(b.view(ft).copy()).cuda() for b in bufs]
                    do = torch.from_numpy(out.view(ft).copy()).cuda()
                    dh = [torch.from_numpy((h.view(ft) if kind else h).copy()).cuda() for h in hs]
                    torch.cuda.synchronize()
                    j = min(1, K - 1)                                  # out == in_1 (in_0 when there is only one)
                    ip = ptrs([t.data_ptr() + SENT * out.itemsize for t in db])
                    op = ip[j] if alias else do.data_ptr() + SENT * out.itemsize
                    rc = L.offt_hipk_pointwise_sum(K, ip, ptrs([t.data_ptr() for t in dh]), op, prec, kind, n0, n1, n2, s0, s1, s2, None)
                    assert rc == 0, L.offt_hipk_last_error()
                    torch.cuda.synchronize()
                    before = bufs[j] if alias else out
                    got = (db[j] if alias else do).cpu().numpy().view(ct)
                    mask = np.zeros(nel + 2 * SENT, dtype=bool)
                    mask[SENT + idx] = True
                    assert got[~mask].tobytes() == before[~mask].tobytes(), ("padding or sentinels written", prec, kind, K, alias)
                    for k in range(K):
                        if not (alias and k == j):
                            assert db[k].cpu().numpy().tobytes() == bufs[k].view(ft).tobytes(), ("an input was written", k)
                    err = np.linalg.norm(got[SENT + idx].astype(np.complex128) - want) / np.linalg.norm(want)
                    print("pointwise_sum", (prec, kind, K, alias), "rel-L2", err)
                    assert err <= (1e-14 if prec == api.F64 else 1e-6), (prec, kind, K, alias, err)


# ---- 12. / 13. one rank through the API -------------------------------------------------------------------------------------
def _gpu_case(case, zgroup=None, opts=()):
    import torch
    L = api.lib()
    po = HW.make_plan(api, case)
    try:
        for o, v in opts:
            assert L.offt_hip_set_option(po, o, v) == 0
        if zgroup is not None:
            assert L.offt_hip_set_option(po, 0, zgroup) == 0
        if case.get("half"):
            api.offt_hip_set_half_box(po, True)
        err = SW.run_sum(api, po, case, HW.Gpu(torch))
        return err, api.offt_hip_convolve_sum_fused(po)
    finally:
        api.offt_3d_fin(po)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(64, 12, 10), (128, 8, 6), (1024, 4, 6), (1024, 24, 13)])
@pytest.mark.parametrize("f32", [0, 1])
def test_sum_single_rank_fused_gpu(built, shape, f32):
    for r2c in (0, 1):
        for zgroup in (0, -1, 1):
            case = dict(N=list(shape), f32=f32, r2c=r2c, K=3, cplx=(zgroup == 0), inplace=(None if zgroup else 1))
            err, fused = _gpu_case(case, zgroup)
            print("fused", case, zgroup, "rel-L2", err)
            assert fused, case                 # (no length is dropped by the spill rule: DESIGN.md 4.5)
            assert err <= W.tol(case), (case, zgroup, err)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [dict(N=[48, 40, 30]), dict(N=[64, 64, 64], params={"S": 1})])
def test_sum_single_rank_generic_gpu(built, case):
    for f32 in (0, 1):
        for inplace in (None, 2):
            cs = dict(case, f32=f32, K=3, inplace=inplace, cplx=f32)
            err, fused = _gpu_case(cs)
            print("generic", cs, "rel-L2", err)
            assert not fused and err <= W.tol(cs), (cs, err)


# ---- 14. pruned half box ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("r2c", [0, 1])
def test_sum_half_box_pruned_gpu(built, r2c):
    for inplace in (None, 1):
        case = dict(N=[64, 64, 64], r2c=r2c, cplx=1 - r2c, K=3, half=1, inplace=inplace)
        import torch
        L = api.lib()
        po = HW.make_plan(api, case)
        try:
            if r2c:
                assert L.offt_hip_set_option(po, api.OPT_HALF_R2C, 1) == 0
            api.offt_hip_set_half_box(po, True)
            assert api.offt_hip_half_box_pruned(po) and api.offt_hip_convolve_sum_fused(po)
            err = SW.run_sum(api, po, case, HW.Gpu(torch))
            print("half box", case, "rel-L2", err)
            assert err <= W.tol(case), (case, err)
        finally:
            api.offt_3d_fin(po)


# ---- 15. pressure projection ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_sum_pressure_projection_gpu(built):
    """u_c = k_c cos(k.x): the inverse Laplacian of its divergence, sum_c (-i k_c / k^2) u^_c, is sin(k.x)"""
    import torch
    n, kv = 64, (3, 5, 2)
    po = api.offt_3d_init(n, n, n, is_r2c=1)
    try:
        c, ne = api.comm_dict(po), api.local_elems(po)
        case = dict(N=[n, n, n], r2c=1, cplx=1)
        g = 2.0 * np.pi * np.arange(n) / n
        ph = kv[0] * g[:, None, None] + kv[1] * g[None, :, None] + kv[2] * g[None, None, :]
        kx = np.fft.fftfreq(n, 1.0 / n)[:, None, None]
        ky = np.fft.fftfreq(n, 1.0 / n)[None, :, None]
        kz = np.arange(n // 2 + 1, dtype=np.float64)[None, None, :]
        k2 = kx * kx + ky * ky + kz * kz
        k2[0, 0, 0] = 1.0
        dev = HW.Gpu(torch)
        ins, filts = [], []
        for kc, kk in zip(kv, (kx, ky, kz)):
            H = -1j * kk / k2 + 0.0 * k2
            H[0, 0, 0] = 0.0
            d, f = W.local_arrays(c, ne, case, kc * np.cos(ph), H)
            ins.append(dev.put(d))
            filts.append(dev.put(f))
        api.lib().offt_hip_set_output_scale(po, 1.0 / n ** 3)
        api.offt_hip_execute_convolve_sum(po, [p for _, p in ins], [p for _, p in filts], ins[2][1], api.FILTER_COMPLEX)
        assert api.offt_hip_convolve_sum_fused(po)
        err = W.check(c, case, dev.get(ins[2][0], np.zeros(1, dtype=np.complex128)), np.sin(ph))
        print("pressure projection rel-L2", err)
        assert err <= 1e-12, err
    finally:
        api.offt_3d_fin(po)


# ---- 16. refusals of host memory ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_sum_host_memory_refused_gpu(built):
    import torch
    L = api.lib()
    case = dict(N=[64, 12, 10], K=2)
    po = HW.make_plan(api, case)
    try:
        ne = api.local_elems(po)
        host = np.full(ne, 1.0 + 2.0j, dtype=np.complex128)
        keep = host.copy()
        a, b, o = (torch.full((2 * ne,), 4.0, dtype=torch.float64, device="cuda") for _ in range(3))
        h = torch.ones(ne, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        for ins, filts, out, word in (([a.data_ptr(), host.ctypes.data], [h.data_ptr()] * 2, o.data_ptr(), "input 1"),
                                      ([a.data_ptr(), b.data_ptr()], [h.data_ptr(), host.ctypes.data], o.data_ptr(), "filter 1"),
                                      ([a.data_ptr(), b.data_ptr()], [h.data_ptr()] * 2, host.ctypes.data, "output")):
            with pytest.raises(RuntimeError, match=word):
                api.offt_hip_execute_convolve_sum(po, ins, filts, out, api.FILTER_REAL)
            assert po.contents.t[api.ALL] >= 99999999.0
            torch.cuda.synchronize()
            assert host.tobytes() == keep.tobytes()
            assert all(bool((t == 4.0).all()) for t in (a, b, o)), "a refusal writes nothing"
        err = SW.run_sum(api, po, case, HW.Gpu(torch))
        assert err <= W.tol(case), err
    finally:
        api.offt_3d_fin(po)


# ---- 17. thread-rank world --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_sum_thread_world_gpu(built, tmp_path):
    # the direct-store exchange (p2p) on the generic route of several ranks: a forward per input through the pipeline, the
    # multiply-and-sum sweep on the device, execute_inverse_multi on `out`, which is the first input
    cases = [dict(N=[32, 16, 64], params={}, r2c=1, cplx=1, K=2, inplace=0, p2p=1)]
    env = dict(os.environ, GPU_MAX_HW_QUEUES="24")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_conv_sum_world.py"), "2", json.dumps(cases), str(tmp_path)],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert p.returncode == 0, p.stdout.decode()[-4000:]
    res = json.load(open(tmp_path / "summary.json"))
    assert len(res) == len(cases)
    for r in res:
        assert r["rel"] <= r["tol"], r
