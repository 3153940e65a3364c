"""Multi-output spectral convolution: offt_hip_execute_convolve_multi (one forward, several filters).

  * routing of the out-of-place fused launch without a device (offt_hipk_conv_oop_kernel_name);
  * the host's routes on the CPU backend of tests/cpu_backend_multi.c, read off its launch log: every single-rank layout,
    complex and r2c plans, real and complex filters, all outputs separate and one of them `data`, older backend tables,
    gloo worlds of 2 and 4 ranks, refusals, the single-output equivalence, half boxes;
  * -m gpu: random out-of-place descriptors against numpy (source untouched, sentinels, half lines, the cache-keeping twin),
    one rank through the API against numpy and against single-output calls, plane groups, a pruned half box, the gradient
    of a Poisson solve, a thread-rank world, and nout = 1 bit for bit.

Tolerances are the project's own: 1e-12 / 1e-5 rel-L2 at kernel level (test_conv_random_fused_descriptors), W.tol
(1e-12 f64, 2e-5 f32) at plan level."""
import ctypes as C
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import _conv_multi_world as MW
import _conv_world as W
import _half_world as HW
from offt_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Desc(C.Structure):
    """offt_pass_desc (offt_amd/csrc/offt_hipk.h), field by field"""
    _fields_ = [("n", C.c_int), ("precision", C.c_int), ("direction", C.c_int), ("ncols", C.c_int),
                ("nb1", C.c_int), ("nb2", C.c_int),
                ("in_axis_stride", C.c_longlong), ("in_col_stride", C.c_longlong), ("in_b1_stride", C.c_longlong),
                ("in_b2_stride", C.c_longlong),
                ("out_axis_stride", C.c_longlong), ("out_col_stride", C.c_longlong), ("out_b1_stride", C.c_longlong),
                ("out_b2_stride", C.c_longlong),
                ("in_split", C.c_int), ("in_split_nfloor", C.c_int), ("out_split", C.c_int), ("out_split_nfloor", C.c_int),
                ("in_block_stride", C.c_longlong), ("out_block_stride", C.c_longlong),
                ("in_block_tab", C.c_void_p), ("out_block_tab", C.c_void_p),
                ("in_contig", C.c_int), ("out_contig", C.c_int), ("variant", C.c_int), ("scale", C.c_double),
                ("real_input", C.c_int), ("out_keep", C.c_int), ("no_pairs", C.c_int), ("half", C.c_int),
                ("tw4", C.c_void_p), ("tw4_b1", C.c_int), ("tw4_n2", C.c_int)]


class FDesc(C.Structure):
    """offt_filter_desc (offt_amd/csrc/offt_hipk.h)"""
    _fields_ = [("kind", C.c_int), ("mixed", C.c_int), ("axis_stride", C.c_longlong), ("col_stride", C.c_longlong),
                ("b1_stride", C.c_longlong), ("b2_stride", C.c_longlong)]


assert C.sizeof(Desc) == 192 and Desc.tw4.offset == 176 and C.sizeof(FDesc) == 40


def conv_desc(n, prec, ncols, nb1, pad=0, fpad=0, kind=0, scale=1.0, half=0, keep=0):
    """contiguous lines (rows of n + pad elements), the filter in rows of n + fpad"""
    d = Desc()
    d.n, d.precision, d.direction, d.ncols, d.nb1, d.nb2 = n, prec, -1, ncols, nb1, 1
    d.in_axis_stride, d.in_col_stride = 1, n + pad
    d.in_b1_stride = (n + pad) * ncols + pad
    d.in_contig, d.out_contig, d.variant, d.scale = 1, 1, -1, scale
    d.out_axis_stride, d.out_col_stride, d.out_b1_stride = 1, n + fpad, (n + fpad) * ncols
    d.half, d.out_keep = half, keep
    f = FDesc()
    f.kind, f.axis_stride, f.col_stride, f.b1_stride = kind, 1, n + fpad, (n + fpad) * ncols
    return d, f


@pytest.fixture(scope="module")
def kl(built):
    L = api.lib()
    L.offt_hipk_conv_oop_kernel_name.restype = C.c_char_p
    L.offt_hipk_conv_oop_kernel_name.argtypes = [C.POINTER(Desc), C.POINTER(FDesc)]
    L.offt_hipk_conv_has_fused_oop.argtypes = [C.POINTER(Desc), C.POINTER(FDesc)]
    L.offt_hipk_conv_pass_oop.argtypes = [C.POINTER(Desc), C.POINTER(FDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.offt_hipk_prepare.argtypes = [C.c_int, C.c_int]
    L.offt_hipk_last_error.restype = C.c_char_p
    return L


# ---- 1. routing without a device ------------------------------------------------------------------------------------------
def test_multi_kernel_routing_without_a_gpu(kl):
    L = kl
    name = lambda d, f: L.offt_hipk_conv_oop_kernel_name(C.byref(d), C.byref(f)).decode()
    for prec in (api.F64, api.F32):
        for n in (64, 128, 256, 512, 1024):
            for kind in (0, 1):
                for half, want in ((0, "fft_conv_oop_panel_k"), (3, "fft_conv_oop_half_panel_k")):
                    d, f = conv_desc(n, prec, 8, 2, kind=kind, half=half)
                    assert name(d, f) == want, (n, prec, kind, half)
                    assert L.offt_hipk_conv_has_fused_oop(C.byref(d), C.byref(f)) == 1
        for n in (32, 48, 1000, 2048):
            for mixed in (0, 1):                         # (1000 has an in-place mixed-radix kernel, but no out-of-place one)
                d, f = conv_desc(n, prec, 8, 2)
                f.mixed = mixed
                assert name(d, f) == "no fused kernel", (n, prec, mixed)
                assert L.offt_hipk_conv_has_fused_oop(C.byref(d), C.byref(f)) == 0
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
        # src == dst is the in-place launch's business: refused before anything is launched
        d, f = conv_desc(64, prec, 8, 2)
        buf = np.zeros(4096, dtype=np.complex128)
        assert L.offt_hipk_conv_pass_oop(C.byref(d), C.byref(f), buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, None) == -1
        assert "src == dst" in L.offt_hipk_last_error().decode()


# ---- CPU tier ---------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def multi_cpu(built):
    import cpu_world
    subprocess.check_call(["make", "-s", "-C", ROOT, "tests/libcpubackend_multi.so"])
    orig = cpu_world._cb_lib
    cpu_world._cb_lib = MW.multi_cb_lib
    CB = cpu_world.install(0, 1, p1=1)
    yield CB
    cpu_world.uninstall()
    cpu_world._cb_lib = orig


def _run_counted(CB, case, opts=()):
    """plan + multi call on the installed backend: (errors, fused route?, launch counts, launch log)"""
    po = HW.make_plan(api, case)
    try:
        if case.get("half"):
            api.offt_hip_set_half_box(po, True)
        for o, v in opts:
            assert api.lib().offt_hip_set_option(po, o, v) == 0
        n0 = MW.counts(CB)
        CB.cpu_backend_multi_log_reset()
        errs = MW.run_multi(api, po, case, HW.Host())
        n1 = MW.counts(CB)
        return errs, api.offt_hip_convolve_multi_fused(po), {k: n1[k] - n0[k] for k in n0}, MW.launches(CB)
    finally:
        api.offt_3d_fin(po)


def _assert_route(case, fused, cnt, log, groups=1):
    """the launch counts of one multi call with K outputs, `inplace` of them (0 or 1) being data"""
    K, inpl = case.get("K", 3), 0 if case.get("inplace") is None else 1
    if fused:
        fwd = [r for r in log if r[0] == 0 and r[2] < 0]
        inv = [r for r in log if r[0] == 0 and r[2] > 0]
        assert len(fwd) == 1 + groups, (case, fwd)              # z once, y once per group: not K times
        assert len(inv) == K * (groups + 1), (case, inv)                # x (fused), then y per group and z, per output
        assert cnt["conv_oop"] == (K - inpl) * groups and cnt["conv"] == inpl * groups, (case, cnt)
        assert cnt["pointwise"] == 0 and cnt["pointwise_oop"] == 0 and cnt["memcpy"] == 0, (case, cnt)
        if inpl:                                                   # the output that is data comes last
            kinds = [r[0] for r in log if r[0] in (1, 2)]
            assert kinds == [2] * ((K - 1) * groups) + [1] * groups, (case, kinds)
    else:
        assert cnt["conv_oop"] == 0 and cnt["conv"] == 0, (case, cnt)
        assert cnt["pointwise_oop"] == K - inpl and cnt["pointwise"] == inpl and cnt["memcpy"] == 0, (case, cnt)
        assert cnt["pass"] == 3 * (K + 1), (case, cnt)             # one forward, K inverses


LAYOUTS = [dict(), dict(params={"S": 1}), dict(eq=1)]
CPU_CASES = [(shape, lay) for shape in [(64, 8, 16), (64, 64, 8), (12, 10, 9), (128, 6, 5)] for lay in LAYOUTS
             if not lay.get("eq") or shape[0] == shape[1]]


# ---- 2. single rank against numpy, the route read off the launches ----------------------------------------------------
@pytest.mark.parametrize("shape,lay", CPU_CASES)
@pytest.mark.parametrize("r2c", [0, 1])
def test_multi_single_rank_cpu(multi_cpu, shape, lay, r2c):
    CB = multi_cpu
    for cplx in (0, 1):
        for inplace in (None, 1):
            case = dict(N=list(shape), r2c=r2c, cplx=cplx, K=3, inplace=inplace, **lay)
            errs, fused, cnt, log = _run_counted(CB, case)
            assert max(errs) <= 1e-12, (case, errs)
            _assert_route(case, fused, cnt, log)
            if not lay and shape[0] in (64, 128):
                assert fused, "power-of-two x lines of the z-y-x layout take the fused route"
            if lay or shape[0] == 12:
                assert not fused, case


def test_multi_single_rank_cpu_f32(multi_cpu):
    case = dict(N=[64, 8, 16], f32=1, cplx=1, K=3)
    errs, fused, cnt, log = _run_counted(multi_cpu, case)
    assert fused and max(errs) <= 2e-5, errs
    _assert_route(case, fused, cnt, log)


def test_multi_plane_groups_cpu(multi_cpu):
    """1 MiB groups on 1024 x 24 planes (384 KiB each in double): 2 planes per group, 13 planes -> 7 groups, the last ragged"""
    for r2c, groups in ((0, 7), (1, 4)):  # (r2c: 13 // 2 + 1 = 7 planes)
        case = dict(N=[1024, 24, 13], r2c=r2c, K=2, inplace=0)
        errs, fused, cnt, log = _run_counted(multi_cpu, case, opts=[(0, 1)])
        assert fused and max(errs) <= 1e-12, errs
        _assert_route(case, fused, cnt, log, groups=groups)
        oop = [r[4] for r in log if r[0] == 2]
        assert oop == [2] * (groups - 1) + [1], oop               # planes per out-of-place launch: none lost, the last ragged
        case = dict(N=[1024, 24, 13], r2c=r2c, K=2)
        errs, fused, cnt, log = _run_counted(multi_cpu, case, opts=[(0, 0)])  # option 0: plain launches
        assert fused and max(errs) <= 1e-12, errs
        _assert_route(case, fused, cnt, log, groups=1)


# ---- 3. backends without the new entries ------------------------------------------------------------------------------------
def test_multi_older_backend_tables_cpu(multi_cpu):
    CB = multi_cpu
    L = api.lib()
    for shape in ((64, 8, 16), (12, 10, 9)):
        for inplace in (None, 2):
            case = dict(N=list(shape), cplx=1, K=3, inplace=inplace)
            inpl = 0 if inplace is None else 1
            want, _, _, _ = _run_counted(CB, case)
            # the logging table without conv_pass_oop and pointwise_oop: copy + in-place multiply per output, no fused route
            L.offt_hip_test_set_backend(CB.cpu_backend_multi_table_old(), 0, 1)
            errs, fused, cnt, _ = _run_counted(CB, case)
            assert not fused and max(errs) <= 1e-12, errs
            assert cnt["memcpy"] == 3 - inpl and cnt["pointwise"] == 3 and cnt["pointwise_oop"] == 0 and cnt["conv_oop"] == 0, cnt
            # the multiply with a destination, but no out-of-place fused launch
            L.offt_hip_test_set_backend(CB.cpu_backend_multi_table_unfused(), 0, 1)
            errs, fused, cnt, log = _run_counted(CB, case)
            assert not fused and max(errs) <= 1e-12, errs
            _assert_route(case, False, cnt, log)
            # the conv backend's own table, as tests/test_convolve.py installs it (written before the entries existed)
            L.offt_hip_test_set_backend(CB.cpu_backend_conv_table(), 0, 1)
            errs, fused, _, _ = _run_counted(CB, case)
            assert not fused and max(errs) <= 1e-12, errs
            L.offt_hip_test_set_backend(CB.cpu_backend_multi_table(), 0, 1)
            assert max(want) <= 1e-12
    # no pointwise multiply at all: refused
    L.offt_hip_test_set_backend(CB.cpu_backend_conv_table_none(), 0, 1)
    po = api.offt_3d_init(64, 8, 16)
    try:
        n = api.local_elems(po)
        a, b, h = (np.zeros(n, dtype=np.complex128) for _ in range(3))
        with pytest.raises(RuntimeError, match="pointwise"):
            api.offt_hip_execute_convolve_multi(po, a.ctypes.data, [b.ctypes.data], [h.ctypes.data], api.FILTER_COMPLEX)
        assert po.contents.t[api.ALL] >= 99999999.0
        L.offt_hip_test_set_backend(CB.cpu_backend_multi_table(), 0, 1)
    finally:
        api.offt_3d_fin(po)


# ---- 4. gloo worlds ---------------------------------------------------------------------------------------------------------
def _gloo(size, cases, tmp_path):
    subprocess.check_call(["make", "-s", "-C", ROOT, "tests/libcpubackend_multi.so"])
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    procs = []
    for r in range(size):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(size), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_conv_multi_world.py"), "gloo", json.dumps(cases),
                                       str(tmp_path)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = [p.communicate(timeout=900)[0].decode() for p in procs]
    for r, p in enumerate(procs):
        assert p.returncode == 0, f"rank {r}:\n{outs[r][-3000:]}"
    for r in range(size):
        for rec in json.load(open(tmp_path / f"gloo_rank{r}.json")):
            assert rec["rel"] <= rec["tol"], (r, rec)
            K, inpl = rec["case"]["K"], 0 if rec["case"].get("inplace") is None else 1
            cnt = rec["counts"]
            assert not rec["fused"] and cnt["conv_oop"] == 0 and cnt["conv"] == 0, rec   # several ranks: the generic route
            assert cnt["pointwise_oop"] == K - inpl and cnt["pointwise"] == inpl, rec


def test_multi_gloo_world2(built, tmp_path):
    _gloo(2, [dict(N=[16, 16, 16], K=2), dict(N=[16, 12, 10], r2c=1, cplx=1, K=2, inplace=1),
              dict(N=[8, 8, 8], params={"S": 1}, cplx=1, K=2), dict(N=[16, 16, 8], eq=1, r2c=1, K=2, inplace=0)], tmp_path)


def test_multi_gloo_world4(built, tmp_path):
    _gloo(4, [dict(N=[16, 16, 16], params={"P1": 2}, K=2), dict(N=[16, 16, 16], params={"P1": 2}, r2c=1, cplx=1, K=2, inplace=0),
              dict(N=[16, 16, 32], K=2, inplace=1), dict(N=[16, 12, 10], r2c=1, K=2)], tmp_path)


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------
def _call(L, po, data, outs, filts, kind, nout=None):
    n = len(outs)
    O, F = (C.c_void_p * max(n, 1))(*outs), (C.c_void_p * max(n, 1))(*filts)
    return L.offt_hip_execute_convolve_multi(po, data, n if nout is None else nout, O, F, kind)


def test_multi_refusals_cpu(multi_cpu):
    L = api.lib()
    po = api.offt_3d_init(64, 8, 16)
    try:
        ne = api.local_elems(po)
        d, o1, o2, h = (np.zeros(ne, dtype=np.complex128) for _ in range(4))
        D, O1, O2, H = (a.ctypes.data for a in (d, o1, o2, h))

        def refused(rc, word):
            assert rc == -1 and word in L.offt_hip_last_error().decode() and po.contents.t[api.ALL] >= 99999999.0, \
                (rc, word, L.offt_hip_last_error())
            po.contents.t[api.ALL] = 0.0

        refused(_call(L, po, D, [], [], api.FILTER_REAL), "nout")
        refused(_call(L, po, D, [O1], [H], api.FILTER_REAL, nout=-1), "nout")
        nine = [np.zeros(ne, dtype=np.complex128) for _ in range(api.CONV_MAX_OUT + 1)]
        refused(_call(L, po, D, [a.ctypes.data for a in nine], [H] * len(nine), api.FILTER_REAL), "nout")
        refused(_call(L, po, D, [O1, None], [H, H], api.FILTER_REAL), "output 1")
        refused(_call(L, po, D, [O1, O2], [H, None], api.FILTER_REAL), "filter 1")
        refused(_call(L, po, D, [O1, O2, O1], [H, H, H], api.FILTER_REAL), "same array")
        refused(_call(L, po, D, [D, O1, D], [H, H, H], api.FILTER_REAL), "same array")
        refused(_call(L, po, D, [O1], [H], 2), "filter_kind")
        refused(_call(L, po, D, [O1], [H], -1), "filter_kind")
        refused(_call(L, po, None, [O1], [H], api.FILTER_REAL), "data")
        refused(L.offt_hip_execute_convolve_multi(po, D, 1, None, None, api.FILTER_REAL), "NULL")
    finally:
        api.offt_3d_fin(po)
    # the plan still works after a refusal (and the Python wrapper raises on one)
    po = api.offt_3d_init(64, 8, 16)
    try:
        with pytest.raises(RuntimeError, match="nout"):
            api.offt_hip_execute_convolve_multi(po, D, [], [], api.FILTER_REAL)
        with pytest.raises(ValueError):
            api.offt_hip_execute_convolve_multi(po, D, [O1], [], api.FILTER_REAL)
        errs = MW.run_multi(api, po, dict(N=[64, 8, 16], K=2), HW.Host())
        assert max(errs) <= 1e-12, errs
    finally:
        api.offt_3d_fin(po)


def test_multi_failed_exchange_leaves_the_marker_cpu(built, monkeypatch):
    """An exchange that fails inside the multi call ends it with -1 and the failure marker.  (The refusal of a communicator
    that failed EARLIER needs a real RCCL world: no test backend can mark the communicator failed, as for the other executes.)"""
    import cpu_world
    subprocess.check_call(["make", "-s", "-C", ROOT, "tests/libcpubackend_multi.so"])
    monkeypatch.setenv("OFFT_FORCE_PIPELINE", "1")   # the multi-rank schedule, exchanges included, on one rank
    monkeypatch.setenv("OFFT_FORCE_A2A", "1")
    orig = cpu_world._cb_lib
    cpu_world._cb_lib = MW.multi_cb_lib
    try:
        cpu_world.install(0, 1, fail_after=3)
        po = api.offt_3d_init(8, 8, 8, custom_params=api.make_params(T1=2, W1=1, T2=2))
        try:
            ne = api.local_elems(po)
            d, o, h = (np.zeros(ne, dtype=np.complex128) for _ in range(3))
            with pytest.raises(RuntimeError, match="offt_hip_execute_convolve_multi failed"):
                api.offt_hip_execute_convolve_multi(po, d.ctypes.data, [o.ctypes.data], [h.ctypes.data], api.FILTER_COMPLEX)
            assert po.contents.t[api.ALL] >= 99999999.0
        finally:
            api.offt_3d_fin(po)
    finally:
        cpu_world.uninstall()
        cpu_world._cb_lib = orig


# ---- 6. single-output equivalence -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [dict(N=[64, 8, 16], cplx=1), dict(N=[12, 10, 9], r2c=1), dict(N=[64, 8, 16], params={"S": 1})])
def test_multi_one_output_in_place_is_the_single_call_cpu(multi_cpu, case):
    po = HW.make_plan(api, case)
    try:
        c, ne = api.comm_dict(po), api.local_elems(po)
        x, H, _ = W.problem(case["N"], case.get("r2c"), case.get("cplx"))
        data, filt = W.local_arrays(c, ne, case, x, H)
        kind = api.FILTER_COMPLEX if case.get("cplx") else api.FILTER_REAL
        a, b = data.copy(), data.copy()
        api.lib().offt_hip_set_output_scale(po, 0.25)
        api.offt_hip_execute_convolve(po, a.ctypes.data, filt.ctypes.data, kind)
        api.offt_hip_execute_convolve_multi(po, b.ctypes.data, [b.ctypes.data], [filt.ctypes.data], kind)
        assert a.tobytes() == b.tobytes()
    finally:
        api.offt_3d_fin(po)


# ---- 7. half box --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,pruned", [(dict(N=[64, 64, 64], cplx=1), True), (dict(N=[64, 64, 64], r2c=1), True),
                                         (dict(N=[64, 64, 64], r2c=1, off=1), False), (dict(N=[12, 10, 8], cplx=1), False),
                                         (dict(N=[12, 10, 8], r2c=1, inplace=1), False), (dict(N=[64, 64, 64], inplace=0), True)])
def test_multi_half_box_cpu(multi_cpu, case, pruned):
    CB = multi_cpu
    case = dict(case, K=2, half=1)
    opts = [(api.OPT_HALF_R2C, 1)] if case.get("r2c") and not case.get("off") else []
    po = HW.make_plan(api, case)
    try:
        for o, v in opts:
            assert api.lib().offt_hip_set_option(po, o, v) == 0
        api.offt_hip_set_half_box(po, True)
        assert api.offt_hip_half_box_pruned(po) == pruned
        n0 = MW.counts(CB)
        CB.cpu_backend_multi_log_reset()
        errs = MW.run_multi(api, po, case, HW.Host())
        assert max(errs) <= 1e-12, (case, errs)
        n1 = MW.counts(CB)
        cnt = {k: n1[k] - n0[k] for k in n0}
        fused = api.offt_hip_convolve_multi_fused(po)
        assert fused == (case["N"][0] == 64)
        _assert_route(case, fused, cnt, MW.launches(CB))
        if pruned:   # every launch of a pruned plan is a half-line launch, the out-of-place ones in the half = 3 form
            assert all(r[5] == (3 if r[0] in (1, 2) else r[5]) and r[5] != 0 for r in MW.launches(CB)), MW.launches(CB)
    finally:
        api.offt_3d_fin(po)


# ---- GPU tier ---------------------------------------------------------------------------------------------------------------
# ---- 8. random out-of-place descriptors -------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [64, 128, 256, 512, 1024])   # every registered length
def test_multi_random_oop_descriptors(kl, n):
    import torch
    L = kl
    rng = np.random.default_rng(1900 + n)
    SENT = 8  # sentinel elements on either side of both arrays
    for prec in (api.F64, api.F32):
        assert L.offt_hipk_prepare(n, prec) == 0
        ft, ct = (np.float64, np.complex128) if prec == api.F64 else (np.float32, np.complex64)
        for kind in (0, 1):
            for half in (0, 3):
                for keep in (0, 1):
                    ncols = int(rng.choice([3, 13, 21]))      # never a whole number of panels
                    nb1 = int(rng.integers(2, 4))
                    pad, fpad = int(rng.integers(0, 3)), int(rng.integers(0, 3))
                    scale = float(rng.choice([0.5, 1.0 / n, 3.0]))
                    d, f = conv_desc(n, prec, ncols, nb1, pad=pad, fpad=fpad, kind=kind, scale=scale, half=half, keep=keep)
                    nin = d.in_b1_stride * nb1 + 16
                    nf = f.b1_stride * nb1 + 16
                    nio = n // 2 if half else n
                    x = (rng.standard_normal(nin) + 1j * rng.standard_normal(nin)).astype(ct)
                    h = (rng.standard_normal(nf) + 1j * rng.standard_normal(nf)) if kind else rng.standard_normal(nf)
                    lines = np.zeros(nin, dtype=bool)         # what the launch may write
                    want = np.zeros(nin, dtype=np.complex128)
                    for b1 in range(nb1):
                        for c in range(ncols):
                            i = b1 * d.in_b1_stride + c * d.in_col_stride
                            fo = b1 * f.b1_stride + c * f.col_stride
                            H = h[fo:fo + n].astype(ct if kind else ft).astype(np.complex128)
                            xin = x[i:i + n].astype(np.complex128)
                            if half:
                                xin[n // 2:] = 0.0
                                x[i + n // 2:i + n] = np.nan + 1j * np.nan   # the upper halves must not be read
                            want[i:i + nio] = (np.fft.ifft(H * np.fft.fft(xin)) * n * scale)[:nio]
                            lines[i:i + nio] = True
                    src = np.full(nin + 2 * SENT, 7.0 + 7.0j, dtype=ct)
                    src[SENT:SENT + nin] = x
                    dst = np.full(nin + 2 * SENT, -5.0 + 9.0j, dtype=ct)
                    ds = torch.from_numpy(src.view(ft).copy()).cuda()
                    dd = torch.from_numpy(dst.view(ft).copy()).cuda()
                    dh = torch.from_numpy((h.astype(ct).view(ft) if kind else h.astype(ft)).copy()).cuda()
                    torch.cuda.synchronize()
                    rc = L.offt_hipk_conv_pass_oop(C.byref(d), C.byref(f), dh.data_ptr(), ds.data_ptr() + SENT * src.itemsize,
                                                   dd.data_ptr() + SENT * dst.itemsize, None)
                    assert rc == 0, L.offt_hipk_last_error()
                    torch.cuda.synchronize()
                    tag = (n, prec, kind, half, keep)
                    assert ds.cpu().numpy().tobytes() == src.view(ft).tobytes(), ("the source was written", tag)
                    got = dd.cpu().numpy().view(ct)
                    assert np.all(got[:SENT] == dst[:SENT]) and np.all(got[SENT + nin:] == dst[SENT + nin:]), ("sentinel overwritten", tag)
                    mid = got[SENT:SENT + nin]
                    assert np.all(mid[~lines] == dst[SENT:SENT + nin][~lines]), ("padding or upper halves written", tag)
                    err = np.linalg.norm(mid[lines].astype(np.complex128) - want[lines]) / np.linalg.norm(want[lines])
                    print("oop descriptor", tag, "rel-L2", err)
                    assert err <= (1e-12 if prec == api.F64 else 1e-5), (tag, err)


# ---- 9. one rank through the API --------------------------------------------------------------------------------------------
FUSED_SHAPES = [(64, 12, 10), (128, 8, 6), (1024, 4, 6)]
GROUPED = (1024, 24, 13)   # 1 MiB groups: 2 (f64) or 5 (f32) planes of 1024 x 24 per group, a ragged last group either way


def _groups(shape, f32, r2c, mib):
    """plane_group's rule (offt_host.c): planes per group and planes of the spectrum"""
    cnt = shape[2] // 2 + 1 if r2c else shape[2]
    plane_mib = shape[0] * shape[1] * (8 if f32 else 16) / (1024.0 * 1024.0)
    return min(int(mib / plane_mib), cnt), cnt


def _gpu_multi_vs_single(case, zgroup):
    import torch
    L = api.lib()
    po = HW.make_plan(api, case)
    try:
        if zgroup is not None:
            assert L.offt_hip_set_option(po, 0, zgroup) == 0
        dev = HW.Gpu(torch)
        pr = MW.problem(case)
        c, ne = api.comm_dict(po), api.local_elems(po)
        data, filts = MW.buffers(c, ne, case, pr[0], pr[1])
        kind = api.FILTER_COMPLEX if case.get("cplx") else api.FILTER_REAL
        hd, pd = dev.put(data)
        hf = [dev.put(f) for f in filts]
        ho = [dev.put(np.zeros(ne, dtype=data.dtype)) for _ in filts]
        L.offt_hip_set_output_scale(po, MW.SCALE)
        api.offt_hip_execute_convolve_multi(po, pd, [p for _, p in ho], [p for _, p in hf], kind)
        multi = [dev.get(h, data) for h, _ in ho]
        errs, vs = [], []
        for k, (_, pf) in enumerate(hf):
            hs, ps = dev.put(data)                                 # the restored input
            api.offt_hip_execute_convolve(po, ps, pf, kind)
            single = dev.get(hs, data)
            errs.append(W.check(c, case, multi[k], pr[2][k]))
            ref = W.check(c, case, single, pr[2][k])
            assert ref <= W.tol(case), (case, k, ref)
            idx = W.in_index(c, bool(case.get("r2c")))
            a, b = (m.view(m.real.dtype)[idx] if case.get("r2c") else m[idx] for m in (multi[k], single))
            vs.append(float(np.linalg.norm(a.astype(np.complex128) - b.astype(np.complex128)) / np.linalg.norm(b.astype(np.complex128))))
        return errs, vs, api.offt_hip_convolve_multi_fused(po)
    finally:
        api.offt_3d_fin(po)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", FUSED_SHAPES + [GROUPED])
def test_multi_one_rank_fused_gpu(built, shape):
    import torch
    torch.cuda.set_device(0)
    for f32 in (0, 1):
        for r2c in (0, 1):
            for zgroup in (0, -1, 1):       # plain launches; the library's rule; 1 MiB groups
                case = dict(N=list(shape), f32=f32, r2c=r2c, cplx=(r2c + f32) % 2, K=3)
                if shape == GROUPED and zgroup == 1:
                    # _groups restates plane_group's rule; that the library's own loop then runs these groups (7 and 4 of them
                    # in double, the last ragged, none lost) is read off the launch log by test_multi_plane_groups_cpu on this
                    # very shape and option -- the host loop is the same code on both backends, only the launches differ
                    ng, cnt = _groups(shape, f32, r2c, 1)
                    assert 1 <= ng < cnt and cnt % ng, "more than one plane group, the last one ragged"
                errs, vs, fused = _gpu_multi_vs_single(case, zgroup)
                print("multi", case, "zgroup", zgroup, "vs numpy", errs, "vs single calls", vs)
                assert fused, case
                assert max(errs) <= W.tol(case) and max(vs) <= 2 * W.tol(case), (case, zgroup, errs, vs)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,lay", [((48, 40, 30), dict()), ((64, 64, 64), dict(params={"S": 1}))])
def test_multi_one_rank_generic_gpu(built, shape, lay):
    import torch
    torch.cuda.set_device(0)
    for f32 in (0, 1):
        for r2c in (0, 1):
            case = dict(N=list(shape), f32=f32, r2c=r2c, cplx=(r2c + f32) % 2, K=3, **lay)
            errs, vs, fused = _gpu_multi_vs_single(case, None)
            print("multi", case, "vs numpy", errs, "vs single calls", vs)
            assert not fused, case
            assert max(errs) <= W.tol(case) and max(vs) <= 2 * W.tol(case), (case, errs, vs)


@pytest.mark.gpu
def test_multi_refusals_gpu(built):
    """host memory as data, as an output, as a filter: each refused before anything is launched, then a good call"""
    import torch
    torch.cuda.set_device(0)
    po = api.offt_3d_init(32, 32, 32)
    L = api.lib()
    try:
        ne = api.local_elems(po)
        d, o1, o2 = (torch.zeros(2 * ne, dtype=torch.float64, device="cuda") for _ in range(3))
        h = torch.ones(ne, dtype=torch.float64, device="cuda")
        host = np.zeros(2 * ne)
        D, O1, O2, H, HOST = d.data_ptr(), o1.data_ptr(), o2.data_ptr(), h.data_ptr(), host.ctypes.data
        for data, outs, filts, word in ((HOST, [O1, O2], [H, H], "data must be device memory"),
                                        (D, [O1, HOST], [H, H], "output 1 must be device memory"),
                                        (D, [HOST, D], [H, H], "output 0 must be device memory"),
                                        (D, [O1, O2], [H, HOST], "filter 1 must be device memory"),
                                        (D, [O1, None], [H, H], "output 1 must be device memory (got NULL)"),
                                        (D, [O1, O2], [None, H], "filter 0 must be device memory (got NULL)"),
                                        (D, [O1, O1], [H, H], "same array"), (D, [O1], [H], "filter_kind")):
            po.contents.t[api.ALL] = 0.0
            rc = _call(L, po, data, outs, filts, 5 if word == "filter_kind" else api.FILTER_REAL)
            msg = L.offt_hip_last_error().decode()
            assert rc == -1 and word in msg and po.contents.t[api.ALL] >= 99999999.0, (word, rc, msg)
        torch.cuda.synchronize()
        assert not host.any(), "a refused call wrote host memory"
        assert _call(L, po, D, [O1, D], [H, H], api.FILTER_REAL) == 0, L.offt_hip_last_error()
        errs = MW.run_multi(api, po, dict(N=[32, 32, 32], K=2), HW.Gpu(torch))
        assert max(errs) <= 1e-12, errs
    finally:
        api.offt_3d_fin(po)


# ---- 10. pruned half box ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("r2c", [0, 1])
def test_multi_pruned_half_box_gpu(built, r2c):
    import torch
    torch.cuda.set_device(0)
    for inplace in (None, 1):
        case = dict(N=[64, 64, 64], r2c=r2c, cplx=1, K=2, half=1, inplace=inplace)
        po = HW.make_plan(api, case)
        try:
            if r2c:
                assert api.lib().offt_hip_set_option(po, api.OPT_HALF_R2C, 1) == 0
            api.offt_hip_set_half_box(po, True)
            assert api.offt_hip_half_box_pruned(po) and api.offt_hip_convolve_multi_fused(po)
            errs = MW.run_multi(api, po, case, HW.Gpu(torch))
            print("multi half box", case, errs)
            assert max(errs) <= W.tol(case), (case, errs)
        finally:
            api.offt_3d_fin(po)


# ---- 11. gradient of a Poisson solve ------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_multi_poisson_gradient_gpu(built):
    """lap u = f for one sine mode f = sin(k.x); the filters i k_c / k^2 give d f / d x_c / k^2 = k_c cos(k.x) / k^2 (= -grad u)"""
    import torch
    torch.cuda.set_device(0)
    n = 64
    po = api.offt_3d_init(n, n, n, is_r2c=1)
    L = api.lib()
    try:
        c = api.comm_dict(po)
        ne = api.local_elems(po)
        mode = (3, 5, 2)
        xs = np.arange(n) * 2 * np.pi / n
        phase = mode[0] * xs[:, None, None] + mode[1] * xs[None, :, None] + mode[2] * xs[None, None, :]
        k = np.fft.fftfreq(n, 1.0 / n)
        kz = np.arange(n // 2 + 1, dtype=np.float64)
        K3 = (k[:, None, None] + 0 * kz[None, None, :] + 0 * k[None, :, None], k[None, :, None] + 0 * kz[None, None, :] + 0 * k[:, None, None],
              kz[None, None, :] + 0 * k[:, None, None] + 0 * k[None, :, None])
        k2 = K3[0] ** 2 + K3[1] ** 2 + K3[2] ** 2
        k2[0, 0, 0] = 1.0
        case = dict(N=[n, n, n], r2c=1, cplx=1)
        data = None
        dfs = []
        for cc in range(3):
            H = 1j * K3[cc] / k2
            H[0, 0, 0] = 0.0
            d, f = W.local_arrays(c, ne, case, np.sin(phase), H)
            data = d if data is None else data
            dfs.append(torch.from_numpy(f.view(np.float64).copy()).cuda())
        dd = torch.from_numpy(data.view(np.float64).copy()).cuda()
        outs = [torch.zeros_like(dd), torch.zeros_like(dd), dd]      # the last component lands in data
        torch.cuda.synchronize()
        L.offt_hip_set_output_scale(po, 1.0 / n ** 3)
        api.offt_hip_execute_convolve_multi(po, dd.data_ptr(), [o.data_ptr() for o in outs], [f.data_ptr() for f in dfs], api.FILTER_COMPLEX)
        torch.cuda.synchronize()
        kk = float(sum(m * m for m in mode))
        for cc in range(3):
            want = mode[cc] * np.cos(phase) / kk
            err = W.check(c, case, outs[cc].cpu().numpy().view(np.complex128), want)
            print("poisson gradient component", cc, err)
            assert err <= 1e-12, (cc, err)
        t = (C.c_double * 3)()
        L.offt_hip_last_pass_seconds(po, t)
        assert list(t) == [0.0, 0.0, 0.0] and L.offt_hip_last_device_seconds(po) > 0
    finally:
        api.offt_3d_fin(po)


# ---- 12. thread-rank world ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_multi_thread_world_gpu(built, tmp_path):
    # the direct-store exchange (p2p): every output but `data` runs execute_inverse_multi on an array the forward never saw
    cases = [dict(N=[32, 16, 64], params={}, r2c=1, cplx=1, K=2, inplace=1, p2p=1)]
    env = dict(os.environ, GPU_MAX_HW_QUEUES="24")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_conv_multi_world.py"), "2", json.dumps(cases), str(tmp_path)],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert p.returncode == 0, p.stdout.decode()[-4000:]
    res = json.load(open(tmp_path / "summary.json"))
    assert len(res) == len(cases)
    for r in res:
        assert r["rel"] <= r["tol"], r


# ---- 13. nout = 1, outs[0] = data ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", [dict(N=[64, 12, 10], cplx=1), dict(N=[48, 40, 30], r2c=1, f32=1)])
def test_multi_one_output_in_place_is_the_single_call_gpu(built, case):
    import torch
    torch.cuda.set_device(0)
    po = HW.make_plan(api, case)
    try:
        c, ne = api.comm_dict(po), api.local_elems(po)
        x, H, _ = W.problem(case["N"], case.get("r2c"), case.get("cplx"))
        data, filt = W.local_arrays(c, ne, case, x, H)
        kind = api.FILTER_COMPLEX if case.get("cplx") else api.FILTER_REAL
        dev = HW.Gpu(torch)
        (ha, pa), (hb, pb), (hf, pf) = dev.put(data), dev.put(data), dev.put(filt)
        api.lib().offt_hip_set_output_scale(po, 0.25)
        api.offt_hip_execute_convolve(po, pa, pf, kind)
        api.offt_hip_execute_convolve_multi(po, pb, [pb], [pf], kind)
        torch.cuda.synchronize()
        assert torch.equal(ha, hb)
    finally:
        api.offt_3d_fin(po)
