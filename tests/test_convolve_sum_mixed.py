"""Multi-input spectral convolution at mixed-radix x lengths: OFFT_HIP_OPT_CONV_SUM_MIXED (include/offt_hip.h), bit 3 of
offt_filter_desc::mixed (offt_amd/csrc/offt_hipk.h) and the kernels under them, fft_conv_sum_panelx_k and
fft_conv_sum_half_panelx_k (convx_sum_body, offt_amd/csrc/offt_panel.hpp).

  * routing of the gather launch without a device: every registered (precision, length) with bits 1 and 3 of the field, the
    same descriptors with every other value, the powers of two, and everything that has no kernel either way;
  * the host's route on the CPU backend of tests/cpu_backend_sum.c, read off its launch log: both options on = the fused
    gather route, either alone = the generic one; the layouts and lengths that never fuse; plane groups; the option's set /
    get round trip and its environment default; a pruned half box;
  * -m gpu: random gather descriptors of all 22 instances (numpy, every other source untouched, sentinels, in place bit for
    bit what out of place gives, the same bits on a second launch), plans on one rank on both routes, ragged plane groups,
    a pruned half box.

The expected value is numpy's sum_k ifft(H_k fft(x_k)) N scale; the filters are random as in test_convolve_sum.py and every
test asserts on the numpy side that the sum does not cancel.  Tolerances are the project's own: 1e-12 / 1e-5 rel-L2 at
kernel level, W.tol (1e-12 f64, 2e-5 f32) at plan level and between the fused and the generic route."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _conv_sum_world as SW
import _conv_world as W
import _half_world as HW
from offt_amd import api
from test_convolve_multi import _groups, conv_desc
from test_convolve_sum import _assert_route, _run_counted, kl, ptrs, sum_cpu  # noqa: F401  (kl, sum_cpu: fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the registered instances (offt_reg_conv_sum_mixed_*.hip): every length of the in-place kernels has a spill-free shape
LENGTHS = {api.F64: (96, 192, 320, 384, 640, 768, 1000), api.F32: (384, 640, 768, 1000)}
INSTANCES = [(prec, n) for prec, ns in LENGTHS.items() for n in ns]
OPT_ZGROUP_MIB, OPT_HALF_MIXED, OPT_CONV_MIXED, OPT_CONV_MULTI_MIXED, OPT_CONV_SUM_MIXED = 0, 11, 12, 14, 16  # include/offt_hip.h
BOTH = [(OPT_CONV_MIXED, 1), (OPT_CONV_SUM_MIXED, 1)]
FULL, HALF = "fft_conv_sum_panelx_k", "fft_conv_sum_half_panelx_k"


# ---- 1. routing without a device ------------------------------------------------------------------------------------------
def test_sum_mixed_kernel_routing_without_a_gpu(kl):
    L = kl
    name = lambda d, f: L.offt_hipk_conv_sum_kernel_name(C.byref(d), C.byref(f)).decode()
    has = lambda d, f: L.offt_hipk_conv_has_fused_sum(C.byref(d), C.byref(f))

    def desc(n, prec, mixed, **kw):
        d, f = conv_desc(n, prec, 7, 2, **kw)
        f.mixed = mixed
        return d, f

    for prec, n in INSTANCES:
        for kind in (0, 1):
            for half, want in ((0, FULL), (3, HALF)):
                for mixed in (5, 7):                         # bits 1 and 3; bit 2 belongs to the out-of-place launch
                    d, f = desc(n, prec, mixed, kind=kind, half=half)
                    assert name(d, f) == want and has(d, f) == 1, (n, prec, kind, half, mixed)
                for mixed in (0, 1, 2, 3, 4, 6):             # one of the two bits missing: as before
                    d, f = desc(n, prec, mixed, kind=kind, half=half)
                    assert name(d, f) == "no fused kernel" and has(d, f) == 0, (n, prec, kind, half, mixed)
        d, f = desc(n, prec, 7)
        f.axis_stride = 8                                    # strided filter axis
        assert name(d, f) == "no fused kernel" and has(d, f) == 0
        d, f = desc(n, prec, 7)
        d.in_contig, d.in_axis_stride, d.in_col_stride = 0, 8, 1   # strided lines
        assert name(d, f) == "no fused kernel" and has(d, f) == 0
        d, f = desc(n, prec, 7)
        d.in_split = n // 4                                  # a split line
        assert name(d, f) == "no fused kernel" and has(d, f) == 0
        for half in (1, 2):                                  # half lines: loads and stores together, or not at all
            d, f = desc(n, prec, 7, half=half)
            assert name(d, f) == "no fused kernel" and has(d, f) == 0, (n, prec, half)
    for prec in (api.F64, api.F32):
        for n in (64, 128, 256, 512, 1024):                  # the powers of two do not care
            for half, want in ((0, "fft_conv_sum_panel_k"), (3, "fft_conv_sum_half_panel_k")):
                names = {name(*desc(n, prec, mixed, half=half)) for mixed in (0, 7)}
                assert names == {want}, (n, prec, half, names)
        for n in (48, 2048):                                 # swept but not registered; too long
            for half in (0, 3):
                d, f = desc(n, prec, 7, half=half)
                assert name(d, f) == "no fused kernel" and has(d, f) == 0, (n, prec, half)
    d, f = desc(96, api.F32, 7)                              # single precision has no instance below 384 points
    assert name(d, f) == "no fused kernel" and has(d, f) == 0


# ---- 2. the host's route on the CPU backend ---------------------------------------------------------------------------------
@pytest.mark.parametrize("r2c", [0, 1])
def test_sum_mixed_route_cpu(sum_cpu, r2c):
    CB = sum_cpu
    for cplx in (0, 1):
        for inplace in (None, 0):
            case = dict(N=[96, 8, 16], r2c=r2c, cplx=cplx, K=3, inplace=inplace)
            err, fused, cnt, log = _run_counted(CB, case, opts=BOTH)
            assert fused and err <= 1e-12, (case, err)
            _assert_route(case, True, cnt, log)
            assert cnt["conv_sum"] == 1 and cnt["pointwise_sum"] == 0, (case, cnt)
            # either option alone, or neither: a forward per input, one multiply-and-sum sweep, one inverse
            for opts in ([(OPT_CONV_MIXED, 1)], [(OPT_CONV_SUM_MIXED, 1)], []):
                err, fused, cnt, log = _run_counted(CB, case, opts=opts)
                assert not fused and err <= 1e-12, (case, opts, err)
                _assert_route(case, False, cnt, log)


def test_sum_mixed_other_layouts_and_lengths_cpu(sum_cpu):
    CB = sum_cpu
    # no instance at 12 points; S = 1 and the y-z-x layout are not z-y-x; single precision has no 96: generic with both options on
    for case in (dict(N=[12, 10, 9]), dict(N=[96, 8, 16], params={"S": 1}), dict(N=[96, 96, 8], eq=1),
                 dict(N=[96, 8, 16], f32=1)):
        for r2c in (0, 1):
            case = dict(case, r2c=r2c, cplx=1 - r2c, K=3, inplace=None)
            err, fused, cnt, log = _run_counted(CB, case, opts=BOTH)
            assert not fused and err <= W.tol(case), (case, err)
            _assert_route(case, False, cnt, log)
    case = dict(N=[384, 4, 6], f32=1, cplx=1, K=3)
    err, fused, cnt, log = _run_counted(CB, case, opts=BOTH)
    assert fused and err <= 2e-5, err
    _assert_route(case, True, cnt, log)
    # a power-of-two plan does not care
    for opts in ([], BOTH, [(OPT_CONV_SUM_MIXED, 1)]):
        case = dict(N=[64, 8, 16], K=3, inplace=2)
        err, fused, cnt, log = _run_counted(CB, case, opts=opts)
        assert fused and err <= 1e-12, (opts, err)
        _assert_route(case, True, cnt, log)


def test_sum_mixed_plane_groups_cpu(sum_cpu):
    """1 MiB groups on 768 x 24 planes (288 KiB each in double): 3 planes per group, 13 planes -> 5 groups, the last of one
    plane (r2c: 7 planes -> 3 groups).  The host loop is the same code on the device: test_sum_mixed_plane_groups_gpu runs
    this shape and option there."""
    for r2c in (0, 1):
        ng, cnt_planes = _groups((768, 24, 13), 0, r2c, 1)
        assert ng == 3 and cnt_planes == (7 if r2c else 13)
        groups = -(-cnt_planes // ng)
        case = dict(N=[768, 24, 13], r2c=r2c, K=3, inplace=0)
        err, fused, cnt, log = _run_counted(sum_cpu, case, opts=BOTH + [(OPT_ZGROUP_MIB, 1)])
        assert fused and err <= 1e-12, err
        _assert_route(case, True, cnt, log, groups=groups)
        want = [ng] * (groups - 1) + [cnt_planes - ng * (groups - 1)]
        assert want[-1] == 1 and sum(want) == cnt_planes
        assert [r[4] for r in log if r[0] == 2] == want, log     # planes per gather launch: none lost, the last ragged


# ---- 3. option plumbing -------------------------------------------------------------------------------------------------------
def test_sum_mixed_option_round_trip_cpu(sum_cpu):
    L = api.lib()
    assert api.OPT_CONV_SUM_MIXED == OPT_CONV_SUM_MIXED
    po = api.offt_3d_init(96, 8, 16)
    try:
        assert L.offt_hip_get_option(po, OPT_CONV_SUM_MIXED) == 0, "off by default"
        assert not api.offt_hip_convolve_sum_fused(po)
        assert L.offt_hip_set_option(po, OPT_CONV_SUM_MIXED, 1) == 0
        assert not api.offt_hip_convolve_sum_fused(po) and not api.offt_hip_convolve_fused(po), "alone it changes nothing"
        assert L.offt_hip_set_option(po, OPT_CONV_SUM_MIXED, 0) == 0
        assert L.offt_hip_set_option(po, OPT_CONV_MIXED, 1) == 0
        assert api.offt_hip_convolve_fused(po) and not api.offt_hip_convolve_sum_fused(po)
        for v, want in ((1, 1), (0, 0), (5, 1), (0, 0)):
            assert L.offt_hip_set_option(po, OPT_CONV_SUM_MIXED, v) == 0, L.offt_hip_last_error()
            assert L.offt_hip_get_option(po, OPT_CONV_SUM_MIXED) == want
            assert api.offt_hip_convolve_sum_fused(po) == bool(want)
            assert api.offt_hip_convolve_fused(po), "the single-output route does not read the option"
            assert not api.offt_hip_convolve_multi_fused(po), "the multi-output route does not read the option"
        assert L.offt_hip_set_option(po, OPT_CONV_MULTI_MIXED, 1) == 0   # bit 2 is not bit 3
        assert not api.offt_hip_convolve_sum_fused(po) and L.offt_hip_set_option(po, OPT_CONV_MULTI_MIXED, 0) == 0
        assert L.offt_hip_set_option(po, OPT_CONV_SUM_MIXED, 1) == 0 and L.offt_hip_set_option(po, OPT_CONV_MIXED, 0) == 0
        assert L.offt_hip_get_option(po, OPT_CONV_SUM_MIXED) == 1 and not api.offt_hip_convolve_sum_fused(po)
        assert L.offt_hip_set_option(po, 17, 1) == -1 and b"unknown option 17" in L.offt_hip_last_error()
        assert L.offt_hip_get_option(po, 17) == -1
    finally:
        api.offt_3d_fin(po)


_ENV_CHILD = """
import os, sys
sys.path[:0] = [%r, %r]
import cpu_world, _conv_sum_world as SW
from offt_amd import api
cpu_world._cb_lib = SW.sum_cb_lib
cpu_world.install(0, 1, p1=1)
L = api.lib()
po = api.offt_3d_init(96, 8, 16)
v = L.offt_hip_get_option(po, 16)
f0 = int(api.offt_hip_convolve_sum_fused(po))   # (OFFT_CONV_MIXED is not set: the option alone changes nothing)
L.offt_hip_set_option(po, 12, 1)
f = int(api.offt_hip_convolve_sum_fused(po))
# the environment after the plan exists changes nothing on it; the next plan reads it
os.environ["OFFT_CONV_SUM_MIXED"] = "0" if v else "1"
v1, f1 = L.offt_hip_get_option(po, 16), int(api.offt_hip_convolve_sum_fused(po))
p2 = api.offt_3d_init(96, 8, 16)
v2 = L.offt_hip_get_option(p2, 16)
print("RESULT", v, f0, f, v1, f1, v2)
api.offt_3d_fin(p2)
api.offt_3d_fin(po)
"""


def test_sum_mixed_environment_default(built):
    """OFFT_CONV_SUM_MIXED is read once, by offt_3d_init, as the option's default"""
    subprocess.check_call(["make", "-s", "-C", ROOT, "tests/libcpubackend_sum.so"])
    for val, want in ((None, "RESULT 0 0 0 0 0 1"), ("1", "RESULT 1 0 1 1 1 0"), ("0", "RESULT 0 0 0 0 0 1")):
        env = {k: v for k, v in os.environ.items() if k not in ("OFFT_CONV_SUM_MIXED", "OFFT_CONV_MIXED")}
        if val is not None:
            env["OFFT_CONV_SUM_MIXED"] = val
        p = subprocess.run([sys.executable, "-c", _ENV_CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=300)
        out = p.stdout.decode()
        assert p.returncode == 0 and want in out.splitlines(), (val, out[-2000:])


# ---- 4. one plan on both routes -----------------------------------------------------------------------------------------------
def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _block(po, case, got):
    """the elements of the input block (of its box for a half-box case) of an output buffer, in double precision"""
    c, r2c = api.comm_dict(po), bool(case.get("r2c"))
    idx = W.in_index(c, r2c)
    if case.get("half"):
        idx = idx[HW.box_mask(c, case["N"])]
    blk = got.view(got.real.dtype)[idx] if r2c else got[idx]
    return blk.astype(np.float64 if r2c else np.complex128)


def _on_and_off(case, dev, opts=(), zgroup=None):
    """one plan: the call with OFFT_HIP_OPT_CONV_MIXED and OFFT_HIP_OPT_CONV_SUM_MIXED on (fused), then with the second one
    off (generic).  (error of either against numpy, fused against generic)"""
    L = api.lib()
    pr = SW.problem(case)
    po = HW.make_plan(api, case)
    try:
        if zgroup is not None:
            assert L.offt_hip_set_option(po, OPT_ZGROUP_MIB, zgroup) == 0
        for o, v in opts:
            assert L.offt_hip_set_option(po, o, v) == 0, L.offt_hip_last_error()
        if case.get("half"):
            api.offt_hip_set_half_box(po, True)
            assert api.offt_hip_half_box_pruned(po)
        assert not api.offt_hip_convolve_sum_fused(po), "the options are off by default"
        for o, v in BOTH:
            assert L.offt_hip_set_option(po, o, v) == 0, L.offt_hip_last_error()
        assert api.offt_hip_convolve_sum_fused(po) and api.offt_hip_convolve_fused(po), case
        k_on, k_off = {}, {}
        e_on = SW.run_sum(api, po, case, dev, pr=pr, keep=k_on)
        assert L.offt_hip_set_option(po, OPT_CONV_SUM_MIXED, 0) == 0
        assert not api.offt_hip_convolve_sum_fused(po) and api.offt_hip_convolve_fused(po), case
        e_off = SW.run_sum(api, po, case, dev, pr=pr, keep=k_off)
        rel = _rel(_block(po, case, k_on["got"]), _block(po, case, k_off["got"]))
    finally:
        api.offt_3d_fin(po)
    print("sum mixed", case, "fused", e_on, "generic", e_off, "fused against generic", rel)
    assert e_on <= W.tol(case) and e_off <= W.tol(case) and rel <= W.tol(case), (case, e_on, e_off, rel)


# ---- 5. pruned half box -------------------------------------------------------------------------------------------------------
HALF_BOX = dict(N=[96, 96, 96], cplx=1, K=2, half=1)  # a 48^3 box


def test_sum_mixed_half_box_cpu(sum_cpu):
    CB = sum_cpu
    CB.cpu_backend_sum_log_reset()
    n0 = SW.counts(CB)
    _on_and_off(dict(HALF_BOX, inplace=0), HW.Host(), opts=[(OPT_HALF_MIXED, 1)])
    n1 = SW.counts(CB)
    # the fused call: one gather launch on half lines; the generic one: one multiply-and-sum sweep; nothing is cleared
    assert n1["conv_sum"] - n0["conv_sum"] == 1 and n1["pointwise_sum"] - n0["pointwise_sum"] == 1, (n0, n1)
    assert n1["zero"] == n0["zero"] and n1["conv"] == n0["conv"] and n1["pointwise"] == n0["pointwise"], (n0, n1)
    log = SW.launches(CB)
    assert [r[5] for r in log if r[0] == 2] == [3], "the gather launch of a pruned plan runs on half lines"
    passes = [r for r in log if r[0] == 0]
    assert passes and all(r[5] != 0 for r in passes), "every pass of both calls is a half-line pass"


# ---- GPU tier ---------------------------------------------------------------------------------------------------------------
SENT = 8  # sentinel elements on either side of every array


# ---- 6. random gather descriptors -------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("prec,n", INSTANCES)
def test_sum_mixed_random_gather_descriptors(kl, prec, n):
    import torch
    L = kl
    rng = np.random.default_rng(9100 + n + 7 * prec)
    assert L.offt_hipk_prepare(n, prec) == 0, L.offt_hipk_last_error()
    ft, ct = (np.float64, np.complex128) if prec == api.F64 else (np.float32, np.complex64)
    KMAX = 8

    def gpu(a):
        return torch.from_numpy(a.view(ft).copy()).cuda()

    for half in (0, 3):
        for kind in (0, 1):
            for ncols in (5, 19):                            # never a whole number of panels (2 ... 16 columns)
                nb1 = 2
                pad, fpad = int(rng.integers(1, 4)), int(rng.integers(1, 4))
                scale = float(rng.choice([0.5, 1.0 / n, 3.0]))
                d, f = conv_desc(n, prec, ncols, nb1, pad=pad, fpad=fpad, kind=kind, scale=scale, half=half)
                f.mixed = 5 if ncols == 5 else 7
                assert L.offt_hipk_conv_sum_kernel_name(C.byref(d), C.byref(f)).decode() == (HALF if half else FULL)
                nel = d.in_b1_stride * nb1 + 16
                nf = f.b1_stride * nb1 + 16
                nio = n // 2 if half else n
                xs = [(rng.standard_normal(nel) + 1j * rng.standard_normal(nel)).astype(ct) for _ in range(KMAX)]
                hs = [(rng.standard_normal(nf) + 1j * rng.standard_normal(nf)) if kind else rng.standard_normal(nf) for _ in range(KMAX)]
                lines = np.zeros(nel, dtype=bool)            # what the launch may write
                terms = [np.zeros(nel, dtype=np.complex128) for _ in range(KMAX)]
                for b1 in range(nb1):
                    for c in range(ncols):
                        i = b1 * d.in_b1_stride + c * d.in_col_stride
                        fo = b1 * f.b1_stride + c * f.col_stride
                        for k in range(KMAX):
                            H = hs[k][fo:fo + n].astype(ct if kind else ft).astype(np.complex128)
                            xin = xs[k][i:i + n].astype(np.complex128)
                            if half:
                                xin[n // 2:] = 0.0
                                xs[k][i + n // 2:i + n] = np.nan + 1j * np.nan   # the upper halves must not be read
                            terms[k][i:i + nio] = (np.fft.ifft(H * np.fft.fft(xin)) * n * scale)[:nio]
                        lines[i:i + nio] = True
                srcs = []
                for x in xs:
                    s = np.full(nel + 2 * SENT, 7.0 + 7.0j, dtype=ct)
                    s[SENT:SENT + nel] = x
                    srcs.append(s)
                dst = np.full(nel + 2 * SENT, -5.0 + 9.0j, dtype=ct)
                full = np.zeros(nel + 2 * SENT, dtype=bool)
                full[SENT:SENT + nel] = lines
                dh = [gpu(h.astype(ct)) if kind else torch.from_numpy(h.astype(ft)).cuda() for h in hs]
                fp = ptrs([t.data_ptr() for t in dh])
                off = SENT * dst.itemsize
                for K in (1, 3, 8):                          # the first K sources and filters
                    tag = (n, prec, half, kind, ncols, K)
                    want = sum(terms[1:K], terms[0])
                    assert np.linalg.norm(want[lines]) >= max(np.linalg.norm(t[lines]) for t in terms[:K]), "the sum cancels"
                    # (a) dst a buffer of its own
                    ds, dd = [gpu(s) for s in srcs[:K]], gpu(dst)
                    torch.cuda.synchronize()
                    sp = ptrs([t.data_ptr() + off for t in ds])
                    rc = L.offt_hipk_conv_pass_sum(C.byref(d), C.byref(f), K, fp, sp, dd.data_ptr() + off, None)
                    assert rc == 0, L.offt_hipk_last_error()
                    torch.cuda.synchronize()
                    for k in range(K):
                        assert ds[k].cpu().numpy().tobytes() == srcs[k].view(ft).tobytes(), ("a source was written", tag, k)
                    got = dd.cpu().numpy().view(ct)
                    assert got[~full].tobytes() == dst[~full].tobytes(), ("sentinel, padding or upper halves written", tag)
                    err = np.linalg.norm(got[full].astype(np.complex128) - want[lines]) / np.linalg.norm(want[lines])
                    print("mixed gather descriptor", tag, "rel-L2", err)
                    assert np.isfinite(err) and err <= (1e-12 if prec == api.F64 else 1e-5), (tag, err)
                    # (b) a second launch on fresh copies: the same bits
                    ds2, dd2 = [gpu(s) for s in srcs[:K]], gpu(dst)
                    torch.cuda.synchronize()
                    sp2 = ptrs([t.data_ptr() + off for t in ds2])
                    rc = L.offt_hipk_conv_pass_sum(C.byref(d), C.byref(f), K, fp, sp2, dd2.data_ptr() + off, None)
                    assert rc == 0, L.offt_hipk_last_error()
                    torch.cuda.synchronize()
                    assert dd2.cpu().numpy().tobytes() == got.view(ft).tobytes(), ("a second launch gives other bits", tag)
                    # (c) dst one of the sources: the others untouched, the lines what they were out of place, and whatever
                    # else that source held (padding, NaN upper halves, sentinels) as it was
                    j = int(rng.integers(0, K))
                    rc = L.offt_hipk_conv_pass_sum(C.byref(d), C.byref(f), K, fp, sp2, sp2[j], None)
                    assert rc == 0, L.offt_hipk_last_error()
                    torch.cuda.synchronize()
                    for k in range(K):
                        if k != j:
                            assert ds2[k].cpu().numpy().tobytes() == srcs[k].view(ft).tobytes(), ("a source was written", tag, k, j)
                    gj = ds2[j].cpu().numpy().view(ct)
                    assert gj[~full].tobytes() == srcs[j][~full].tobytes(), ("in place: more than the lines written", tag, j)
                    assert gj[full].tobytes() == got[full].tobytes(), ("in place differs from out of place", tag, j)
    # without bits 1 and 3 these lines have no gather kernel: the launch fails, it runs nothing
    keep = dd.cpu().numpy().tobytes()
    for mixed in (0, 1, 2, 3, 4, 6):
        d, f = conv_desc(n, prec, 4, 1)
        f.mixed = mixed
        assert L.offt_hipk_conv_pass_sum(C.byref(d), C.byref(f), 1, fp, sp, dd.data_ptr() + off, None) == -1
        assert b"no multi-input fused convolution kernel" in L.offt_hipk_last_error()
    torch.cuda.synchronize()
    assert dd.cpu().numpy().tobytes() == keep


# ---- 7. one rank through the API --------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("r2c", [0, 1])
@pytest.mark.parametrize("shape,f32", [((96, 40, 30), 0), ((1000, 8, 6), 0), ((384, 16, 8), 1)])
def test_sum_mixed_one_rank_gpu(built, shape, f32, r2c):
    import torch
    torch.cuda.set_device(0)
    _on_and_off(dict(N=list(shape), f32=f32, r2c=r2c, cplx=(r2c + f32) % 2, K=3, inplace=0), HW.Gpu(torch))


@pytest.mark.gpu
def test_sum_mixed_plane_groups_gpu(built):
    """(768, 24, 13) in double with 1 MiB groups: planes of 288 KiB, 3 per group, a last group of one plane.  That the
    library's loop runs exactly these groups is read off the launch log by test_sum_mixed_plane_groups_cpu on this shape and
    option -- the host loop is the same code on both backends.  The y pass of a group asks the gather launch to keep its
    stores; the mixed-radix instances have no keeping twin and run plain."""
    import torch
    torch.cuda.set_device(0)
    ng, cnt = _groups((768, 24, 13), 0, 0, 1)
    assert ng == 3 and cnt == 13 and cnt % ng == 1, "more than one plane group, the last one ragged"
    _on_and_off(dict(N=[768, 24, 13], K=3, inplace=0), HW.Gpu(torch), zgroup=1)


# ---- 8. pruned half box -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_sum_mixed_pruned_half_box_gpu(built):
    import torch
    torch.cuda.set_device(0)
    for inplace in (None, 0):
        _on_and_off(dict(HALF_BOX, inplace=inplace), HW.Gpu(torch), opts=[(OPT_HALF_MIXED, 1)])
