"""Filtered forward and filtered inverse: offt_hip_execute_forward_filtered, offt_hip_execute_inverse_filtered.

  * routing of the two kernels without a device (offt_hipk_filt_fwd_kernel_name, offt_hipk_filt_inv_kernel_name);
  * the host's routes on the CPU backend of tests/cpu_backend_spec.c, read off its launch log: every single-rank layout,
    complex and r2c plans, real and complex filters, nout 1, 3 and 8, one output equal to the spectrum, plane groups, older
    backend tables, a half box, the option, gloo worlds of 2 and 4 ranks, refusals;
  * -m gpu: random descriptors of both kernels against numpy line FFTs, one rank through the API against numpy and against
    the generic route on the same device, plane groups, the generic route, a pseudo-spectral step, bit-for-bit repeats, a
    thread-rank world.

Tolerances are the project's own: 1e-12 / 1e-5 rel-L2 at kernel level, W.tol (1e-12 f64, 2e-5 f32) at plan level, 2 W.tol
between two routes of the library."""
import ctypes as C
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import _conv_world as W
import _half_world as HW
import _spec_world as SW
from offt_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT_ZGROUP_MIB = 0


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


def filt_desc(n, prec, ncols, nb1, pad=0, fpad=0, kind=0, scale=1.0, keep=0):
    """contiguous lines (rows of n + pad elements), the filter in rows of n + fpad"""
    d = Desc()
    d.n, d.precision, d.direction, d.ncols, d.nb1, d.nb2 = n, prec, -1, ncols, nb1, 1
    d.in_axis_stride, d.in_col_stride = 1, n + pad
    d.in_b1_stride = (n + pad) * ncols + pad
    d.in_contig, d.out_contig, d.variant, d.scale = 1, 1, -1, scale
    d.out_axis_stride, d.out_col_stride, d.out_b1_stride = 1, n + fpad, (n + fpad) * ncols
    d.out_keep = keep
    f = FDesc()
    f.kind, f.axis_stride, f.col_stride, f.b1_stride = kind, 1, n + fpad, (n + fpad) * ncols
    return d, f


@pytest.fixture(scope="module")
def kl(built):
    L = api.lib()
    DP, FP, V = C.POINTER(Desc), C.POINTER(FDesc), C.c_void_p
    for f in (L.offt_hipk_filt_fwd_kernel_name, L.offt_hipk_filt_inv_kernel_name):
        f.restype = C.c_char_p
        f.argtypes = [DP, FP]
    L.offt_hipk_filt_has_fused.argtypes = [DP, FP]
    L.offt_hipk_filt_pass_fwd.argtypes = [DP, FP, V, V, V]
    L.offt_hipk_filt_pass_inv.argtypes = [DP, FP, V, V, V, V]
    L.offt_hipk_prepare.argtypes = [C.c_int, C.c_int]
    L.offt_hipk_last_error.restype = C.c_char_p
    return L


# ---- 1. routing without a device ------------------------------------------------------------------------------------------
def test_spec_kernel_routing_without_a_gpu(kl):
    L = kl
    names = lambda d, f: (L.offt_hipk_filt_fwd_kernel_name(C.byref(d), C.byref(f)).decode(),
                          L.offt_hipk_filt_inv_kernel_name(C.byref(d), C.byref(f)).decode())
    none = ("no fused kernel", "no fused kernel")
    for prec in (api.F64, api.F32):
        for n in (64, 128, 256, 512, 1024):
            for kind in (0, 1):
                for keep in (0, 1):
                    d, f = filt_desc(n, prec, 8, 2, kind=kind, keep=keep)
                    assert names(d, f) == ("fft_filt_fwd_panel_k", "fft_filt_inv_panel_k"), (n, prec, kind)
                    assert L.offt_hipk_filt_has_fused(C.byref(d), C.byref(f)) == 1
        for n in (32, 2048, 96):
            for mixed in (0, 7):
                d, f = filt_desc(n, prec, 8, 2)
                f.mixed = mixed
                assert names(d, f) == none, (n, prec)
                assert L.offt_hipk_filt_has_fused(C.byref(d), C.byref(f)) == 0
        d, f = filt_desc(1024, prec, 8, 2)
        d.in_contig, d.in_axis_stride, d.in_col_stride = 0, 8, 1   # strided lines
        assert names(d, f) == none
        d, f = filt_desc(1024, prec, 8, 2)
        f.axis_stride = 8                                          # strided filter axis
        assert names(d, f) == none
        d, f = filt_desc(1024, prec, 8, 2)
        d.in_split = 256                                           # a split line
        assert names(d, f) == none
        for ri in (1, 2):                                          # real rows
            d, f = filt_desc(1024, prec, 8, 2)
            d.real_input = ri
            assert names(d, f) == none
        for half in (1, 2, 3):                                     # half lines
            d, f = filt_desc(1024, prec, 8, 2)
            d.half = half
            assert names(d, f) == none
        d, f = filt_desc(64, prec, 8, 2)
        f.kind = 2
        assert names(d, f) == none


# ---- CPU tier ---------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def spec_cpu(built):
    import cpu_world
    subprocess.check_call(["make", "-s", "-C", ROOT, "tests/libcpubackend_spec.so"])
    orig = cpu_world._cb_lib
    cpu_world._cb_lib = SW.spec_cb_lib
    CB = cpu_world.install(0, 1, p1=1)
    yield CB
    cpu_world.uninstall()
    cpu_world._cb_lib = orig


def _counted(CB, fn):
    n0 = SW.counts(CB)
    CB.cpu_backend_spec_log_reset()
    res = fn()
    n1 = SW.counts(CB)
    return res, {k: n1[k] - n0[k] for k in n0}, SW.launches(CB)


def _run_both(CB, case, opts=(), half=False, spec_fused=1):
    """plan + both calls on the installed backend, OFFT_HIP_OPT_SPEC_FUSED on unless told otherwise; checks the answers and
    returns the routes read off the launch log"""
    po = HW.make_plan(api, case)
    try:
        for o, v in ([(api.OPT_SPEC_FUSED, spec_fused)] if spec_fused is not None else []) + list(opts):
            assert api.lib().offt_hip_set_option(po, o, v) == 0
        if half:
            api.offt_hip_set_half_box(po, True)
        fused = api.offt_hip_spectral_fused(po)
        pr = SW.problem(case)
        if half:   # a half-box forward reads the box only
            h = [n // 2 for n in case["N"]]
            xp = np.zeros_like(pr["x"]); xp[:h[0], :h[1], :h[2]] = pr["x"][:h[0], :h[1], :h[2]]
            pr["x"] = xp
            pr["fwd"] = SW.SCALE * pr["H0"] * (np.fft.rfftn(xp, axes=(0, 1, 2)) if case.get("r2c") else np.fft.fftn(xp))
        (ferr, _), fcnt, flog = _counted(CB, lambda: SW.run_forward(api, po, case, HW.Host(), pr))
        assert ferr <= W.tol(case), (case, "forward", ferr)
        K, inpl = case.get("K", 3), 0 if case.get("inplace") is None else 1
        if not half:
            (ierrs, intact, _), icnt, ilog = _counted(CB, lambda: SW.run_inverse(api, po, case, HW.Host(), pr))
            assert max(ierrs) <= W.tol(case), (case, "inverse", ierrs)
            assert intact is not False, (case, "the spectrum was written")
        return fused, (fcnt, flog), (icnt, ilog) if not half else None
    finally:
        api.offt_3d_fin(po)


def _assert_routes(case, fused, fwd, inv, groups=1, oop=True, plain=False):
    K, inpl = case.get("K", 3), 0 if case.get("inplace") is None else 1
    fcnt, flog = fwd
    icnt, ilog = inv
    if fused:
        assert fcnt["filt_fwd"] == groups and fcnt["pass"] == 1 + groups and fcnt["pointwise"] == 0, (case, fcnt)
        assert [r[0] for r in flog] == [0] + [0, 1] * groups, (case, flog)               # z; per group y, filtered x
        assert icnt["filt_inv"] == K * groups and icnt["pass"] == K * (groups + 1), (case, icnt)
        assert icnt["pointwise"] == 0 and icnt["pointwise_oop"] == 0 and icnt["memcpy"] == 0, (case, icnt)
        assert [r[0] for r in ilog] == ([2, 0] * groups + [0]) * K, (case, ilog)           # per output: per group x, y; then z
        same = [r[8] for r in ilog if r[0] == 2]
        assert same == [0] * ((K - inpl) * groups) + [1] * (inpl * groups), (case, same)   # the output that is spec comes last
        if plain:        # OFFT_HIP_OPT_ZGROUP_MIB 0: plain launches, nothing kept
            assert all(r[7] == 0 for r in flog + ilog), (flog, ilog)
        else:            # the producer of every pair keeps its stores, the consumer does not
            assert all(r[7] == 1 for r in flog[1:] if r[0] == 0) and all(r[7] == 1 for r in ilog if r[0] == 2), (flog, ilog)
            assert all(r[7] == 0 for r in flog if r[0] == 1) and all(r[7] == 0 for r in ilog if r[0] == 0), (flog, ilog)
    else:
        assert fcnt["filt_fwd"] == 0 and fcnt["pointwise"] == 1 and fcnt["pass"] == 3, (case, fcnt)
        assert [r[0] for r in flog if r[0] != 6] == [0, 0, 0, 3], (case, flog)
        assert icnt["filt_inv"] == 0 and icnt["pass"] == 3 * K, (case, icnt)
        if oop:
            assert icnt["pointwise_oop"] == K - inpl and icnt["pointwise"] == inpl and icnt["memcpy"] == 0, (case, icnt)
        else:
            assert icnt["pointwise_oop"] == 0 and icnt["pointwise"] == K and icnt["memcpy"] == K - inpl, (case, icnt)
        mult = [r[0] for r in ilog if r[0] in (3, 4)]
        if oop and inpl:
            assert mult == [4] * (K - 1) + [3], (case, mult)                                # the output that is spec comes last


LAYOUTS = [dict(), dict(params={"S": 1}), dict(eq=1)]
CPU_CASES = [(shape, lay) for shape in [(64, 8, 16), (64, 64, 8), (12, 10, 9), (128, 6, 5)] for lay in LAYOUTS
             if not lay.get("eq") or shape[0] == shape[1]]


# ---- 2. single rank against numpy, the route read off the launches ----------------------------------------------------
@pytest.mark.parametrize("shape,lay", CPU_CASES)
@pytest.mark.parametrize("r2c", [0, 1])
def test_spec_single_rank_cpu(spec_cpu, shape, lay, r2c):
    for cplx in (0, 1):
        for inplace in (None, 0):   # the output that is the spectrum is FIRST in the list: it is still made last
            case = dict(N=list(shape), r2c=r2c, cplx=cplx, K=3, inplace=inplace, **lay)
            fused, fwd, inv = _run_both(spec_cpu, case)
            _assert_routes(case, fused, fwd, inv)
            assert fused == (not lay and shape[0] in (64, 128)), case


def test_spec_single_rank_cpu_f32(spec_cpu):
    case = dict(N=[64, 8, 16], f32=1, cplx=1, K=3)
    fused, fwd, inv = _run_both(spec_cpu, case)
    assert fused
    _assert_routes(case, fused, fwd, inv)


@pytest.mark.parametrize("K", [1, 8])
def test_spec_nout_cpu(spec_cpu, K):
    for shape in ((64, 8, 6), (12, 10, 9)):
        for inplace in (None, K - 1):
            case = dict(N=list(shape), cplx=1, K=K, inplace=inplace)
            fused, fwd, inv = _run_both(spec_cpu, case)
            _assert_routes(case, fused, fwd, inv)


def test_spec_plane_groups_cpu(spec_cpu):
    """1 MiB groups on 1024 x 24 planes (384 KiB each in double): 2 planes per group, 13 planes -> 7 groups, the last ragged"""
    for r2c, groups in ((0, 7), (1, 4)):  # (r2c: 13 // 2 + 1 = 7 planes)
        case = dict(N=[1024, 24, 13], r2c=r2c, K=2, inplace=1)
        fused, fwd, inv = _run_both(spec_cpu, case, opts=[(OPT_ZGROUP_MIB, 1)])
        assert fused
        _assert_routes(case, fused, fwd, inv, groups=groups)
        assert [r[4] for r in fwd[1] if r[0] == 1] == [2] * (groups - 1) + [1]           # planes per launch: none lost
        assert [r[4] for r in inv[1] if r[0] == 2] == ([2] * (groups - 1) + [1]) * 2
        fused, fwd, inv = _run_both(spec_cpu, case, opts=[(OPT_ZGROUP_MIB, 0)])             # option 0: plain launches
        assert fused
        _assert_routes(case, fused, fwd, inv, groups=1, plain=True)


def test_spec_older_backend_tables_cpu(spec_cpu):
    CB, L = spec_cpu, api.lib()
    try:
        for shape in ((64, 8, 16), (12, 10, 9)):
            for inplace in (None, 2):
                case = dict(N=list(shape), cplx=1, K=3, inplace=inplace)
                L.offt_hip_test_set_backend(CB.cpu_backend_spec_table_nofilt(), 0, 1)   # from before the two entries
                fused, fwd, inv = _run_both(CB, case)
                assert not fused
                _assert_routes(case, fused, fwd, inv)
                L.offt_hip_test_set_backend(CB.cpu_backend_spec_table_old(), 0, 1)      # ... and before pointwise_oop
                fused, fwd, inv = _run_both(CB, case)
                assert not fused
                _assert_routes(case, fused, fwd, inv, oop=False)
        L.offt_hip_test_set_backend(CB.cpu_backend_spec_table_none(), 0, 1)             # no multiply at all: refused
        po = api.offt_3d_init(64, 8, 16)
        try:
            n = api.local_elems(po)
            a, b, h = (np.zeros(n, dtype=np.complex128) for _ in range(3))
            with pytest.raises(RuntimeError, match="pointwise"):
                api.offt_hip_execute_forward_filtered(po, a.ctypes.data, h.ctypes.data, api.FILTER_COMPLEX)
            assert po.contents.t[api.ALL] >= 99999999.0
            with pytest.raises(RuntimeError, match="pointwise"):
                api.offt_hip_execute_inverse_filtered(po, a.ctypes.data, [b.ctypes.data], [h.ctypes.data], api.FILTER_COMPLEX)
            assert po.contents.t[api.ALL] >= 99999999.0
        finally:
            api.offt_3d_fin(po)
    finally:
        L.offt_hip_test_set_backend(CB.cpu_backend_spec_table(), 0, 1)


@pytest.mark.parametrize("r2c", [0, 1])
def test_spec_half_box_takes_the_generic_route_cpu(spec_cpu, r2c):
    case = dict(N=[64, 64, 64], r2c=r2c, cplx=1, K=2)
    fused, fwd, _ = _run_both(spec_cpu, case, half=True)
    assert not fused
    assert fwd[0]["filt_fwd"] == 0 and fwd[0]["pointwise"] == 1 and fwd[0]["pass"] == 3, fwd[0]
    # the inverse of a half-box plan defines the box only: the generic route, compared inside the box
    po = HW.make_plan(api, case)
    try:
        api.offt_hip_set_half_box(po, True)
        c, ne = api.comm_dict(po), api.local_elems(po)
        pr = SW.problem(case)
        spec = SW.out_buffer(c, ne, case, pr["S"])
        filt = W.local_arrays(c, ne, case, pr["x"], pr["Hs"][0])[1]
        out = np.zeros(ne, dtype=spec.dtype)
        (_, cnt, _) = _counted(spec_cpu, lambda: api.offt_hip_execute_inverse_filtered(po, spec.ctypes.data, [out.ctypes.data],
                                                                                        [filt.ctypes.data], api.FILTER_COMPLEX))
        assert cnt["filt_inv"] == 0 and cnt["pointwise_oop"] == 1 and cnt["pass"] == 3, cnt
        assert HW.box_err(c, case, out, pr["inv"][0] / SW.SCALE) <= 1e-12
    finally:
        api.offt_3d_fin(po)


def test_spec_option_cpu(spec_cpu):
    L = api.lib()
    assert api.OPT_SPEC_FUSED == 18
    case = dict(N=[64, 8, 16], K=2)
    po = api.offt_3d_init(64, 8, 16)
    try:
        assert L.offt_hip_get_option(po, api.OPT_SPEC_FUSED) == 0 and not api.offt_hip_spectral_fused(po), "off by default"
        for v, want in ((0, 0), (1, 1), (5, 1), (0, 0)):
            assert L.offt_hip_set_option(po, api.OPT_SPEC_FUSED, v) == 0
            assert L.offt_hip_get_option(po, api.OPT_SPEC_FUSED) == want
            assert api.offt_hip_spectral_fused(po) == bool(want)
    finally:
        api.offt_3d_fin(po)
    for v in (None, 0):          # the default, and the option at 0: the generic route
        fused, fwd, inv = _run_both(spec_cpu, case, spec_fused=v)
        assert not fused
        _assert_routes(case, fused, fwd, inv)
    fused, fwd, inv = _run_both(spec_cpu, case, spec_fused=1)
    assert fused
    _assert_routes(case, fused, fwd, inv)


@pytest.mark.parametrize("case", [dict(N=[64, 8, 16], cplx=1), dict(N=[64, 8, 16], r2c=1), dict(N=[12, 10, 9], r2c=1, cplx=1),
                                  dict(N=[64, 64, 8], params={"S": 1}), dict(N=[64, 64, 8], eq=1, cplx=1)])
def test_spec_composition_is_the_convolve_cpu(spec_cpu, case):
    po = HW.make_plan(api, case)
    try:
        assert api.lib().offt_hip_set_option(po, api.OPT_SPEC_FUSED, 1) == 0
        err, between, _ = SW.run_compose(api, po, case, HW.Host())
        assert err <= W.tol(case) and between <= 2 * W.tol(case), (case, err, between)
    finally:
        api.offt_3d_fin(po)


# ---- 3. gloo worlds ---------------------------------------------------------------------------------------------------------
def _gloo(size, cases, tmp_path):
    subprocess.check_call(["make", "-s", "-C", ROOT, "tests/libcpubackend_spec.so"])
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    procs = []
    for r in range(size):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(size), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_spec_world.py"), "gloo", json.dumps(cases),
                                       str(tmp_path)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = [p.communicate(timeout=900)[0].decode() for p in procs]
    for r, p in enumerate(procs):
        assert p.returncode == 0, f"rank {r}:\n{outs[r][-3000:]}"
    for r in range(size):
        for rec in json.load(open(tmp_path / f"gloo_rank{r}.json")):
            assert rec["rel"] <= rec["tol"], (r, rec)
            assert rec["intact"] is not False, (r, rec)
            K, inpl = rec["case"]["K"], 0 if rec["case"].get("inplace") is None else 1
            cnt = rec["counts"]
            assert not rec["fused"] and cnt["filt_fwd"] == 0 and cnt["filt_inv"] == 0, rec   # several ranks: the generic route
            assert cnt["pointwise_oop"] == K - inpl and cnt["pointwise"] == 1 + inpl, rec


def test_spec_gloo_world2(built, tmp_path):
    _gloo(2, [dict(N=[16, 16, 16], K=2), dict(N=[16, 12, 10], r2c=1, cplx=1, K=2, inplace=1),
              dict(N=[8, 8, 8], params={"S": 1}, cplx=1, K=2), dict(N=[16, 16, 8], eq=1, r2c=1, K=2, inplace=0),
              dict(N=[16, 16, 16], K=2, p2p=1, cplx=1)], tmp_path)


def test_spec_gloo_world4(built, tmp_path):
    _gloo(4, [dict(N=[16, 16, 16], params={"P1": 2}, K=2), dict(N=[16, 16, 16], params={"P1": 2}, r2c=1, cplx=1, K=2, inplace=0),
              dict(N=[16, 16, 32], K=2, inplace=1), dict(N=[16, 12, 10], r2c=1, K=2)], tmp_path)


# ---- 4. refusals: one test each, the marker set and nothing launched ---------------------------------------------------------
def _inv(L, po, spec, outs, filts, kind, nout=None):
    n = len(outs)
    O, F = (C.c_void_p * max(n, 1))(*outs), (C.c_void_p * max(n, 1))(*filts)
    return L.offt_hip_execute_inverse_filtered(po, spec, n if nout is None else nout, O, F, kind)


@pytest.fixture()
def refusal(spec_cpu):
    L = api.lib()
    po = api.offt_3d_init(64, 8, 16)
    ne = api.local_elems(po)
    arrs = [np.zeros(ne, dtype=np.complex128) for _ in range(4 + api.CONV_MAX_OUT)]
    ptrs = [a.ctypes.data for a in arrs]

    def refused(call, *words):
        spec_cpu.cpu_backend_spec_log_reset()
        po.contents.t[api.ALL] = 0.0
        rc = call()
        msg = L.offt_hip_last_error().decode()
        assert rc == -1 and all(w in msg for w in words) and po.contents.t[api.ALL] >= 99999999.0, (rc, words, msg)
        assert spec_cpu.cpu_backend_spec_log_len() == 0, "a refused call launched something"

    yield L, po, ptrs, refused
    api.offt_3d_fin(po)
    del arrs


def test_spec_refuses_null_arguments_cpu(refusal):
    L, po, (S, O1, O2, H, *_), refused = refusal
    refused(lambda: L.offt_hip_execute_forward_filtered(po, None, H, api.FILTER_REAL), "forward_filtered", "the data", "NULL")
    refused(lambda: L.offt_hip_execute_forward_filtered(po, S, None, api.FILTER_REAL), "forward_filtered", "the filter", "NULL")
    refused(lambda: _inv(L, po, None, [O1], [H], api.FILTER_REAL), "inverse_filtered", "the spectrum", "NULL")
    refused(lambda: _inv(L, po, S, [O1, None], [H, H], api.FILTER_REAL), "inverse_filtered", "output 1", "NULL")
    refused(lambda: _inv(L, po, S, [O1, O2, S], [H, H, None], api.FILTER_REAL), "inverse_filtered", "filter 2", "NULL")
    refused(lambda: L.offt_hip_execute_inverse_filtered(po, S, 1, None, None, api.FILTER_REAL), "inverse_filtered", "NULL")


def test_spec_refuses_bad_nout_cpu(refusal):
    L, po, (S, O1, O2, H, *more), refused = refusal
    refused(lambda: _inv(L, po, S, [], [], api.FILTER_REAL), "inverse_filtered", "nout = 0")
    refused(lambda: _inv(L, po, S, [O1], [H], api.FILTER_REAL, nout=-1), "nout = -1")
    nine = [O1] + more[:api.CONV_MAX_OUT]
    refused(lambda: _inv(L, po, S, nine, [H] * len(nine), api.FILTER_REAL), "nout = 9")


def test_spec_refuses_equal_outputs_cpu(refusal):
    L, po, (S, O1, O2, H, *_), refused = refusal
    refused(lambda: _inv(L, po, S, [O1, O2, O1], [H, H, H], api.FILTER_REAL), "outputs 0 and 2", "same array")
    refused(lambda: _inv(L, po, S, [S, O1, S], [H, H, H], api.FILTER_REAL), "same array")   # at most one output may be the spectrum


def test_spec_refuses_unknown_filter_kind_cpu(refusal):
    L, po, (S, O1, O2, H, *_), refused = refusal
    refused(lambda: L.offt_hip_execute_forward_filtered(po, S, H, 2), "forward_filtered", "filter_kind 2")
    refused(lambda: _inv(L, po, S, [O1], [H], -1), "inverse_filtered", "filter_kind -1")


def test_spec_works_after_a_refusal_cpu(refusal):
    L, po, (S, O1, O2, H, *_), refused = refusal
    refused(lambda: _inv(L, po, S, [], [], api.FILTER_REAL), "nout")
    with pytest.raises(RuntimeError, match="nout"):
        api.offt_hip_execute_inverse_filtered(po, S, [], [], api.FILTER_REAL)
    with pytest.raises(ValueError):
        api.offt_hip_execute_inverse_filtered(po, S, [O1], [], api.FILTER_REAL)
    case = dict(N=[64, 8, 16], K=2)
    assert SW.run_forward(api, po, case, HW.Host())[0] <= 1e-12
    assert max(SW.run_inverse(api, po, case, HW.Host())[0]) <= 1e-12


def test_spec_failed_exchange_leaves_the_marker_cpu(built, monkeypatch):
    """An exchange that fails inside either call ends it with -1 and the failure marker.  (The refusal of a communicator that
    failed EARLIER needs a real RCCL world: no test backend can mark the communicator failed, as for the other executes.)"""
    import cpu_world
    subprocess.check_call(["make", "-s", "-C", ROOT, "tests/libcpubackend_spec.so"])
    monkeypatch.setenv("OFFT_FORCE_PIPELINE", "1")   # the multi-rank schedule, exchanges included, on one rank
    monkeypatch.setenv("OFFT_FORCE_A2A", "1")
    orig = cpu_world._cb_lib
    cpu_world._cb_lib = SW.spec_cb_lib
    try:
        for which in ("fwd", "inv"):
            cpu_world.install(0, 1, fail_after=1)
            po = api.offt_3d_init(8, 8, 8, custom_params=api.make_params(T1=2, W1=1, T2=2))
            try:
                ne = api.local_elems(po)
                d, o, h = (np.zeros(ne, dtype=np.complex128) for _ in range(3))
                with pytest.raises(RuntimeError, match="filtered failed"):
                    if which == "fwd":
                        api.offt_hip_execute_forward_filtered(po, d.ctypes.data, h.ctypes.data, api.FILTER_COMPLEX)
                    else:
                        api.offt_hip_execute_inverse_filtered(po, d.ctypes.data, [o.ctypes.data], [h.ctypes.data], api.FILTER_COMPLEX)
                assert po.contents.t[api.ALL] >= 99999999.0
            finally:
                api.offt_3d_fin(po)
    finally:
        cpu_world.uninstall()
        cpu_world._cb_lib = orig


# ---- GPU tier ---------------------------------------------------------------------------------------------------------------
# ---- 5. random descriptors of both kernels ----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [64, 128, 256, 512, 1024])   # every registered length
def test_spec_random_descriptors_gpu(kl, n):
    import torch
    L = kl
    rng = np.random.default_rng(2300 + n)
    SENT = 8  # sentinel elements on either side of both arrays
    for prec in (api.F64, api.F32):
        assert L.offt_hipk_prepare(n, prec) == 0
        ft, ct = (np.float64, np.complex128) if prec == api.F64 else (np.float32, np.complex64)
        for inv, kind, keep in [(i, k, kp) for i in (0, 1, 2) for k in (0, 1) for kp in (0, 1)]:  # inv 2: the inverse in place
            ncols = int(rng.choice([3, 13, 21]))      # never a whole number of panels
            nb1 = int(rng.integers(2, 4))
            pad, fpad = int(rng.integers(1, 3)), int(rng.integers(1, 3))
            scale = float(rng.choice([0.5, 1.0 / n, 3.0]))
            d, f = filt_desc(n, prec, ncols, nb1, pad=pad, fpad=fpad, kind=kind, scale=scale, keep=keep)
            nin = d.in_b1_stride * nb1 + 16
            nf = f.b1_stride * nb1 + 16
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
                    want[i:i + n] = (np.fft.ifft(H * xin) * n if inv else H * np.fft.fft(xin)) * scale
                    lines[i:i + n] = True
            src = np.full(nin + 2 * SENT, 7.0 + 7.0j, dtype=ct)
            src[SENT:SENT + nin] = x
            dst = src.copy() if inv != 1 else np.full(nin + 2 * SENT, -5.0 + 9.0j, dtype=ct)
            ds = torch.from_numpy(src.view(ft).copy()).cuda()
            dd = torch.from_numpy(dst.view(ft).copy()).cuda() if inv == 1 else ds
            dh = torch.from_numpy((h.astype(ct).view(ft) if kind else h.astype(ft)).copy()).cuda()
            torch.cuda.synchronize()
            ps, pd = ds.data_ptr() + SENT * src.itemsize, dd.data_ptr() + SENT * dst.itemsize
            if inv:
                rc = L.offt_hipk_filt_pass_inv(C.byref(d), C.byref(f), dh.data_ptr(), ps, pd, None)
            else:
                rc = L.offt_hipk_filt_pass_fwd(C.byref(d), C.byref(f), dh.data_ptr(), pd, None)
            assert rc == 0, L.offt_hipk_last_error()
            torch.cuda.synchronize()
            tag = (n, prec, ("fwd", "inv", "inv in place")[inv], kind, keep)
            if inv == 1:
                assert ds.cpu().numpy().tobytes() == src.view(ft).tobytes(), ("the source was written", tag)
            got = dd.cpu().numpy().view(ct)
            assert np.all(got[:SENT] == dst[:SENT]) and np.all(got[SENT + nin:] == dst[SENT + nin:]), ("sentinel overwritten", tag)
            mid = got[SENT:SENT + nin]
            assert np.all(mid[~lines] == dst[SENT:SENT + nin][~lines]), ("padding written", tag)
            err = np.linalg.norm(mid[lines].astype(np.complex128) - want[lines]) / np.linalg.norm(want[lines])
            print("filt descriptor", tag, "rel-L2", err)
            assert err <= (1e-12 if prec == api.F64 else 1e-5), (tag, err)


# ---- 6. one rank through the API --------------------------------------------------------------------------------------------
def _no_filt_table(L):
    L.offt_hip_test_hip_backend_no_filt.restype = C.c_void_p
    return L.offt_hip_test_hip_backend_no_filt()


def _rel(a, b):
    a, b = a.astype(np.complex128), b.astype(np.complex128)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _gpu_both_routes(case, zgroup=None):
    """both calls on the fused route against numpy, and against the generic route on the same device (a plan made under the
    HIP backend with the two entries withheld)"""
    import cpu_world
    import torch
    L = cpu_world.test_lib()
    try:
        dev, pr, res = HW.Gpu(torch), SW.problem(case), {}
        for name in ("generic", "fused"):
            L.offt_hip_test_set_backend(_no_filt_table(L) if name == "generic" else None, 0, 1)
            po = HW.make_plan(api, case)
            try:
                if zgroup is not None:
                    assert L.offt_hip_set_option(po, OPT_ZGROUP_MIB, zgroup) == 0
                assert L.offt_hip_set_option(po, api.OPT_SPEC_FUSED, 1) == 0
                assert api.offt_hip_spectral_fused(po) == (name == "fused"), (case, name)
                ferr, fgot = SW.run_forward(api, po, case, dev, pr)
                ierrs, intact, outs = SW.run_inverse(api, po, case, dev, pr)
                assert intact is not False, (case, name, "the spectrum was written")
                c = api.comm_dict(po)
                res[name] = (ferr, ierrs, np.array(fgot, copy=True)[W.out_index(c)], [o[W.in_index(c, False)] if not case.get("r2c") else
                                                                                     o.view(o.real.dtype)[W.in_index(c, True)] for o in outs])
            finally:
                api.offt_3d_fin(po)
        (ferr, ierrs, fa, oa), (gferr, gierrs, fb, ob) = res["fused"], res["generic"]
        between = [_rel(fa, fb)] + [_rel(a, b) for a, b in zip(oa, ob)]
        print("spec", case, "zgroup", zgroup, "fused vs numpy", ferr, ierrs, "generic vs numpy", gferr, gierrs, "between", between)
        assert max([ferr, gferr] + ierrs + gierrs) <= W.tol(case), (case, ferr, ierrs, gferr, gierrs)
        assert max(between) <= 2 * W.tol(case), (case, between)
    finally:
        L.offt_hip_test_set_backend(None, 0, 1)
        api.use_library(None)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(64, 12, 10), (256, 8, 6), (1024, 4, 4)])
def test_spec_one_rank_fused_gpu(built, shape):
    import torch
    torch.cuda.set_device(0)
    for r2c in (0, 1):
        _gpu_both_routes(dict(N=list(shape), r2c=r2c, cplx=1 - r2c, K=3, inplace=None if r2c else 1))
    _gpu_both_routes(dict(N=list(shape), f32=1, cplx=1, K=2))


@pytest.mark.gpu
@pytest.mark.parametrize("case", [dict(N=[1024, 16, 10], cplx=1, K=2, inplace=0), dict(N=[1024, 16, 10], r2c=1, K=2)])
def test_spec_plane_groups_gpu(built, case):
    """1 MiB groups of 1024 x 16 planes (256 KiB each in double): 4 planes per group; the complex plan's 10 planes run as groups
    of 4, 4 and 2, the r2c plan's 10 / 2 + 1 = 6 as 4 and 2 (that the library's loop runs exactly these groups is read off the
    launch log on the CPU backend, test_spec_plane_groups_cpu: the host loop is the same code on both backends)"""
    import torch
    torch.cuda.set_device(0)
    _gpu_both_routes(case, zgroup=1)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,lay", [((48, 40, 30), dict()), ((64, 64, 64), dict(params={"S": 1}))])
def test_spec_one_rank_generic_gpu(built, shape, lay):
    import torch
    torch.cuda.set_device(0)
    dev = HW.Gpu(torch)
    for f32, r2c in ((0, 0), (0, 1), (1, 0)):
        case = dict(N=list(shape), f32=f32, r2c=r2c, cplx=(r2c + f32 + 1) % 2, K=2, inplace=1 if r2c else None, **lay)
        po = HW.make_plan(api, case)
        try:
            assert not api.offt_hip_spectral_fused(po), case
            ferr, _ = SW.run_forward(api, po, case, dev)
            ierrs, intact, _ = SW.run_inverse(api, po, case, dev)
            print("spec generic", case, ferr, ierrs)
            assert intact is not False and max([ferr] + ierrs) <= W.tol(case), (case, ferr, ierrs)
        finally:
            api.offt_3d_fin(po)


# ---- 7. a pseudo-spectral step ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_spec_spectral_step_gradient_gpu(built):
    """u = sin(k.x) + 0.5 cos(q.x): forward_filtered with the 2/3-rule mask (both modes lie inside it, a third one outside is
    removed), then inverse_filtered with the three filters i k_c: the gradient of the kept field"""
    import torch
    torch.cuda.set_device(0)
    n = 64
    po = api.offt_3d_init(n, n, n, is_r2c=1)
    L = api.lib()
    try:
        assert L.offt_hip_set_option(po, api.OPT_SPEC_FUSED, 1) == 0 and api.offt_hip_spectral_fused(po)
        c, ne = api.comm_dict(po), api.local_elems(po)
        k1, k2, k3 = (3, 5, 2), (7, 1, 4), (25, 3, 1)          # |k| <= n/3 = 21 is kept: k3 is dealiased away
        xs = np.arange(n) * 2 * np.pi / n
        ph = lambda m: m[0] * xs[:, None, None] + m[1] * xs[None, :, None] + m[2] * xs[None, None, :]
        u = np.sin(ph(k1)) + 0.5 * np.cos(ph(k2)) + 0.25 * np.sin(ph(k3))
        k = np.fft.fftfreq(n, 1.0 / n)
        kz = np.arange(n // 2 + 1, dtype=np.float64)
        K3 = np.broadcast_arrays(k[:, None, None], k[None, :, None], kz[None, None, :])
        mask = ((np.abs(K3[0]) <= n // 3) & (np.abs(K3[1]) <= n // 3) & (K3[2] <= n // 3)).astype(np.float64)
        data, fm = W.local_arrays(c, ne, dict(N=[n] * 3, r2c=1), u, mask)
        case = dict(N=[n] * 3, r2c=1, cplx=1)
        dfs = [torch.from_numpy(W.local_arrays(c, ne, case, u, 1j * K3[cc])[1].view(np.float64).copy()).cuda() for cc in range(3)]
        dd = torch.from_numpy(data.view(np.float64).copy()).cuda()
        dm = torch.from_numpy(fm.copy()).cuda()
        outs = [torch.zeros_like(dd), torch.zeros_like(dd), dd]      # the last component lands in the spectrum's array
        torch.cuda.synchronize()
        L.offt_hip_set_output_scale(po, 1.0 / n ** 3)                # the forward carries the normalisation
        api.offt_hip_execute_forward_filtered(po, dd.data_ptr(), dm.data_ptr(), api.FILTER_REAL)
        L.offt_hip_set_output_scale(po, 1.0)
        api.offt_hip_execute_inverse_filtered(po, dd.data_ptr(), [o.data_ptr() for o in outs], [f.data_ptr() for f in dfs], api.FILTER_COMPLEX)
        torch.cuda.synchronize()
        for cc in range(3):
            want = k1[cc] * np.cos(ph(k1)) - 0.5 * k2[cc] * np.sin(ph(k2))
            err = W.check(c, case, outs[cc].cpu().numpy().view(np.complex128), want)
            print("spectral step gradient component", cc, err)
            assert err <= 1e-12, (cc, err)
        assert L.offt_hip_last_device_seconds(po) > 0
    finally:
        api.offt_3d_fin(po)


# ---- 8. nout = 1 in place: the same bits twice, the convolve to rounding ------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", [dict(N=[64, 12, 10], cplx=1), dict(N=[256, 8, 6], r2c=1), dict(N=[48, 40, 30], r2c=1, f32=1)])
def test_spec_composition_bit_for_bit_gpu(built, case):
    import torch
    torch.cuda.set_device(0)
    po = HW.make_plan(api, case)
    try:
        assert api.lib().offt_hip_set_option(po, api.OPT_SPEC_FUSED, 1) == 0
        assert api.offt_hip_spectral_fused(po) == (case["N"][0] in (64, 256)), case
        dev = HW.Gpu(torch)
        err, between, a = SW.run_compose(api, po, case, dev)
        err2, _, b = SW.run_compose(api, po, case, dev)
        print("spec composition", case, "vs numpy", err, "vs convolve", between)
        assert a.tobytes() == b.tobytes(), "the same two calls repeated differ"
        assert err <= W.tol(case) and between <= 2 * W.tol(case), (case, err, between)
    finally:
        api.offt_3d_fin(po)


# ---- 9. thread-rank world -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_spec_thread_world_gpu(built, tmp_path):
    cases = [dict(N=[32, 16, 64], params={}, r2c=1, cplx=1, K=2, inplace=1, p2p=1)]
    env = dict(os.environ, GPU_MAX_HW_QUEUES="24")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_spec_world.py"), "2", json.dumps(cases), str(tmp_path)],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert p.returncode == 0, p.stdout.decode()[-4000:]
    res = json.load(open(tmp_path / "summary.json"))
    assert len(res) == len(cases)
    for r in res:
        assert r["rel"] <= r["tol"], r
