"""Multi-output spectral convolution at mixed-radix x lengths: OFFT_HIP_OPT_CONV_MULTI_MIXED (include/offt_hip.h), bit 2 of
offt_filter_desc::mixed (offt_amd/csrc/offt_hipk.h) and the kernels under them, fft_conv_oop_panelx_k and
fft_conv_oop_half_panelx_k (convx_body with a store base, offt_amd/csrc/offt_panel.hpp).

  * routing of the out-of-place launch without a device: every registered (precision, length) with both bits of the field,
    the same descriptors with 0, 1 or 2, the powers of two, and everything that has no kernel either way;
  * the host's route on the CPU backend of tests/cpu_backend_multi.c, read off its launch log: both options on = the fused
    multi route, either alone = the generic one; the layouts and lengths that never fuse; plane groups; the option's set /
    get round trip and its environment default; a pruned half box;
  * -m gpu: random out-of-place descriptors of all 22 instances (bit for bit what the in-place kernel leaves in a copy of
    the source, the source untouched, sentinels, numpy), plans on one rank against three single-output calls and against
    the option-off route, ragged plane groups, a pruned half box.

Tolerances are the project's own: 1e-12 / 1e-5 rel-L2 at kernel level (test_conv_mixed_random_fused_descriptors), W.tol
(1e-12 f64, 2e-5 f32) at plan level, twice that between the multi call and single-output calls (test_convolve_multi.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _conv_multi_world as MW
import _conv_world as W
import _half_world as HW
from offt_amd import api
from test_convolve_multi import Desc, FDesc, _assert_route, _groups, _run_counted, conv_desc, multi_cpu  # noqa: F401  (multi_cpu: fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the registered instances (offt_reg_conv_oop_mixed_*.hip): those of the in-place kernels (offt_reg_conv_mixed_*.hip)
LENGTHS = {api.F64: (96, 192, 320, 384, 640, 768, 1000), api.F32: (384, 640, 768, 1000)}
INSTANCES = [(prec, n) for prec, ns in LENGTHS.items() for n in ns]
OPT_ZGROUP_MIB, OPT_HALF_MIXED, OPT_CONV_MIXED, OPT_CONV_MULTI_MIXED = 0, 11, 12, 14  # include/offt_hip.h
BOTH = [(OPT_CONV_MIXED, 1), (OPT_CONV_MULTI_MIXED, 1)]


@pytest.fixture(scope="module")
def kl(built):
    """a handle of the product library of its own: the argument types set here stay out of every other module's way"""
    api._lib.load()                                   # (makes the HIP runtime visible first)
    L = C.CDLL(api._lib.LIB_PATH, mode=C.RTLD_LOCAL)
    PD, PF, vp = C.POINTER(Desc), C.POINTER(FDesc), C.c_void_p
    L.offt_hipk_conv_oop_kernel_name.restype = C.c_char_p
    L.offt_hipk_conv_oop_kernel_name.argtypes = [PD, PF]
    L.offt_hipk_conv_has_fused_oop.argtypes = [PD, PF]
    L.offt_hipk_conv_pass_oop.argtypes = [PD, PF, vp, vp, vp, vp]
    L.offt_hipk_conv_pass.argtypes = [PD, PF, vp, vp, vp]
    L.offt_hipk_prepare.argtypes = [C.c_int, C.c_int]
    L.offt_hipk_last_error.restype = C.c_char_p
    return L


# ---- 1. routing without a device ------------------------------------------------------------------------------------------
def test_multi_mixed_kernel_routing_without_a_gpu(kl):
    L = kl
    name = lambda d, f: L.offt_hipk_conv_oop_kernel_name(C.byref(d), C.byref(f)).decode()
    has = lambda d, f: L.offt_hipk_conv_has_fused_oop(C.byref(d), C.byref(f))

    def desc(n, prec, mixed, **kw):
        d, f = conv_desc(n, prec, 7, 2, **kw)
        f.mixed = mixed
        return d, f

    for prec, n in INSTANCES:
        for kind in (0, 1):
            for half, want in ((0, "fft_conv_oop_panelx_k"), (3, "fft_conv_oop_half_panelx_k")):
                d, f = desc(n, prec, 3, kind=kind, half=half)
                assert name(d, f) == want and has(d, f) == 1, (n, prec, kind, half)
                for mixed in (0, 1, 2):                      # one bit alone, or none: as before
                    d, f = desc(n, prec, mixed, kind=kind, half=half)
                    assert name(d, f) == "no fused kernel" and has(d, f) == 0, (n, prec, kind, half, mixed)
        d, f = desc(n, prec, 3)
        f.axis_stride = 8                                    # strided filter axis
        assert name(d, f) == "no fused kernel" and has(d, f) == 0
        d, f = desc(n, prec, 3)
        d.in_contig, d.in_axis_stride, d.in_col_stride = 0, 8, 1   # strided lines
        assert name(d, f) == "no fused kernel" and has(d, f) == 0
        d, f = desc(n, prec, 3)
        d.in_split = n // 4                                  # a split line
        assert name(d, f) == "no fused kernel" and has(d, f) == 0
        for half in (1, 2):                                  # half lines: loads and stores together, or not at all
            d, f = desc(n, prec, 3, half=half)
            assert name(d, f) == "no fused kernel" and has(d, f) == 0, (n, prec, half)
    for prec in (api.F64, api.F32):
        for n in (64, 128, 256, 512, 1024):                  # the powers of two do not care
            for half, want in ((0, "fft_conv_oop_panel_k"), (3, "fft_conv_oop_half_panel_k")):
                names = {name(*desc(n, prec, mixed, half=half)) for mixed in (0, 3)}
                assert names == {want}, (n, prec, half, names)
        for n in (48, 2048):                                 # swept but not registered; too long
            for half in (0, 3):
                d, f = desc(n, prec, 3, half=half)
                assert name(d, f) == "no fused kernel" and has(d, f) == 0, (n, prec, half)
    d, f = desc(96, api.F32, 3)                              # single precision has no instance below 384 points
    assert name(d, f) == "no fused kernel" and has(d, f) == 0


# ---- 2. the host's route on the CPU backend ---------------------------------------------------------------------------------
@pytest.mark.parametrize("r2c", [0, 1])
def test_multi_mixed_route_cpu(multi_cpu, r2c):
    CB = multi_cpu
    for cplx in (0, 1):
        case = dict(N=[96, 8, 16], r2c=r2c, cplx=cplx, K=3, inplace=1 + cplx)
        errs, fused, cnt, log = _run_counted(CB, case, opts=BOTH)
        assert fused and max(errs) <= 1e-12, (case, errs)
        _assert_route(case, True, cnt, log)
        # either option alone, or neither: forward, then a multiply and an inverse per output
        for opts in ([(OPT_CONV_MIXED, 1)], [(OPT_CONV_MULTI_MIXED, 1)], []):
            errs, fused, cnt, log = _run_counted(CB, case, opts=opts)
            assert not fused and max(errs) <= 1e-12, (case, opts, errs)
            _assert_route(case, False, cnt, log)


def test_multi_mixed_other_layouts_and_lengths_cpu(multi_cpu):
    CB = multi_cpu
    # no instance at 12 points; S = 1 and the y-z-x layout are not z-y-x: generic with both options on
    for case in (dict(N=[12, 10, 9]), dict(N=[96, 8, 16], params={"S": 1}), dict(N=[96, 96, 8], eq=1),
                 dict(N=[96, 8, 16], f32=1)):
        for r2c in (0, 1):
            case = dict(case, r2c=r2c, cplx=1 - r2c, K=3, inplace=0)
            errs, fused, cnt, log = _run_counted(CB, case, opts=BOTH)
            assert not fused and max(errs) <= W.tol(case), (case, errs)
            _assert_route(case, False, cnt, log)
    case = dict(N=[384, 4, 6], f32=1, cplx=1, K=3)
    errs, fused, cnt, log = _run_counted(CB, case, opts=BOTH)
    assert fused and max(errs) <= 2e-5, errs
    _assert_route(case, True, cnt, log)
    # a power-of-two plan does not care
    for opts in ([], BOTH, [(OPT_CONV_MULTI_MIXED, 1)]):
        case = dict(N=[64, 8, 16], K=3, inplace=2)
        errs, fused, cnt, log = _run_counted(CB, case, opts=opts)
        assert fused and max(errs) <= 1e-12, (opts, errs)
        _assert_route(case, True, cnt, log)


def test_multi_mixed_plane_groups_cpu(multi_cpu):
    """1 MiB groups on 768 x 24 planes (288 KiB each in double): 3 planes per group, 13 planes -> 5 groups, the last of one
    plane.  The host loop is the same code on the device: test_multi_mixed_plane_groups_gpu runs this shape and option there."""
    for r2c in (0, 1):
        ng, cnt_planes = _groups((768, 24, 13), 0, r2c, 1)
        assert ng == 3 and cnt_planes == (7 if r2c else 13)
        groups = -(-cnt_planes // ng)
        case = dict(N=[768, 24, 13], r2c=r2c, K=3, inplace=0)
        errs, fused, cnt, log = _run_counted(multi_cpu, case, opts=BOTH + [(OPT_ZGROUP_MIB, 1)])
        assert fused and max(errs) <= 1e-12, errs
        oop = [r[4] for r in log if r[0] == 2]
        if len(oop) == 2:                                        # plane_group gave no groups: the plain launch order
            _assert_route(case, True, cnt, log, groups=1)
            assert oop == [cnt_planes] * 2, oop
            continue
        _assert_route(case, True, cnt, log, groups=groups)
        want = [ng] * (groups - 1) + [cnt_planes - ng * (groups - 1)]
        assert oop == want * 2, oop                              # planes per out-of-place launch: none lost, the last ragged
        assert [r[4] for r in log if r[0] == 1] == want          # ... and of the in-place launch of the output that is data


# ---- 3. option plumbing -------------------------------------------------------------------------------------------------------
def test_multi_mixed_option_round_trip_cpu(multi_cpu):
    L = api.lib()
    assert api.OPT_CONV_MULTI_MIXED == OPT_CONV_MULTI_MIXED
    po = api.offt_3d_init(96, 8, 16)
    try:
        assert L.offt_hip_get_option(po, OPT_CONV_MULTI_MIXED) == 0, "off by default"
        assert not api.offt_hip_convolve_multi_fused(po)
        assert L.offt_hip_set_option(po, OPT_CONV_MIXED, 1) == 0
        assert api.offt_hip_convolve_fused(po) and not api.offt_hip_convolve_multi_fused(po)
        for v, want in ((1, 1), (0, 0), (5, 1), (0, 0)):
            assert L.offt_hip_set_option(po, OPT_CONV_MULTI_MIXED, v) == 0, L.offt_hip_last_error()
            assert L.offt_hip_get_option(po, OPT_CONV_MULTI_MIXED) == want
            assert api.offt_hip_convolve_multi_fused(po) == bool(want)
            assert api.offt_hip_convolve_fused(po), "the single-output route does not read the option"
        assert L.offt_hip_set_option(po, OPT_CONV_MULTI_MIXED, 1) == 0 and L.offt_hip_set_option(po, OPT_CONV_MIXED, 0) == 0
        assert L.offt_hip_get_option(po, OPT_CONV_MULTI_MIXED) == 1 and not api.offt_hip_convolve_multi_fused(po)
        assert L.offt_hip_set_option(po, 15, 1) == -1 and b"unknown option 15" in L.offt_hip_last_error()
        assert L.offt_hip_get_option(po, 15) == -1
    finally:
        api.offt_3d_fin(po)


_ENV_CHILD = """
import os, sys
sys.path[:0] = [%r, %r]
import cpu_world, _conv_multi_world as MW
from offt_amd import api
cpu_world._cb_lib = MW.multi_cb_lib
cpu_world.install(0, 1, p1=1)
L = api.lib()
po = api.offt_3d_init(96, 8, 16)
v = L.offt_hip_get_option(po, 14)
f0 = int(api.offt_hip_convolve_multi_fused(po))   # (OFFT_CONV_MIXED is not set: the option alone changes nothing)
L.offt_hip_set_option(po, 12, 1)
f = int(api.offt_hip_convolve_multi_fused(po))
# the environment after the plan exists changes nothing on it; the next plan reads it
os.environ["OFFT_CONV_MULTI_MIXED"] = "0" if v else "1"
v1, f1 = L.offt_hip_get_option(po, 14), int(api.offt_hip_convolve_multi_fused(po))
p2 = api.offt_3d_init(96, 8, 16)
v2 = L.offt_hip_get_option(p2, 14)
print("RESULT", v, f0, f, v1, f1, v2)
api.offt_3d_fin(p2)
api.offt_3d_fin(po)
"""


def test_multi_mixed_environment_default(built):
    """OFFT_CONV_MULTI_MIXED is read once, by offt_3d_init, as the option's default"""
    subprocess.check_call(["make", "-s", "-C", ROOT, "tests/libcpubackend_multi.so"])
    for val, want in ((None, "RESULT 0 0 0 0 0 1"), ("1", "RESULT 1 0 1 1 1 0"), ("0", "RESULT 0 0 0 0 0 1")):
        env = {k: v for k, v in os.environ.items() if k not in ("OFFT_CONV_MULTI_MIXED", "OFFT_CONV_MIXED")}
        if val is not None:
            env["OFFT_CONV_MULTI_MIXED"] = val
        p = subprocess.run([sys.executable, "-c", _ENV_CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=300)
        out = p.stdout.decode()
        assert p.returncode == 0 and want in out.splitlines(), (val, out[-2000:])


# ---- 4. pruned half box -------------------------------------------------------------------------------------------------------
def _multi_outputs(po, case, dev, pr):
    """the multi call on a plan: (every output's elements of the input block, or of its box for a half-box case; rel-L2 of
    every output against numpy)"""
    L = api.lib()
    c, ne = api.comm_dict(po), api.local_elems(po)
    r2c = bool(case.get("r2c"))
    data, filts = MW.buffers(c, ne, case, pr[0], pr[1])
    hd, pd = dev.put(data)
    hf = [dev.put(f) for f in filts]
    ho = [(hd, pd) if k == case.get("inplace") else dev.put(np.full(ne, 3.0 - 2.0j, dtype=data.dtype)) for k in range(len(filts))]
    L.offt_hip_set_output_scale(po, MW.SCALE)
    api.offt_hip_execute_convolve_multi(po, pd, [p for _, p in ho], [p for _, p in hf],
                                        api.FILTER_COMPLEX if case.get("cplx") else api.FILTER_REAL)
    L.offt_hip_set_output_scale(po, 1.0)
    idx = W.in_index(c, r2c)
    if case.get("half"):
        idx = idx[HW.box_mask(c, case["N"])]
    err = HW.box_err if case.get("half") else W.check
    blocks, errs = [], []
    for (h, _), want in zip(ho, pr[2]):
        got = dev.get(h, data)
        errs.append(err(c, case, got, want))
        blk = got.view(got.real.dtype)[idx] if r2c else got[idx]
        blocks.append(blk.astype(np.float64 if r2c else np.complex128))
    return blocks, errs


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _half_box_on_and_off(dev, inplace):
    """a 48^3 box of a (96, 96, 96) plan, every option on, then OFFT_HIP_OPT_CONV_MULTI_MIXED off on the same plan"""
    L = api.lib()
    case = dict(N=[96, 96, 96], cplx=1, K=2, half=1, inplace=inplace)
    pr = MW.problem(case)
    po = HW.make_plan(api, case)
    try:
        for o in (OPT_HALF_MIXED, OPT_CONV_MIXED, OPT_CONV_MULTI_MIXED):
            assert L.offt_hip_set_option(po, o, 1) == 0, L.offt_hip_last_error()
        api.offt_hip_set_half_box(po, True)
        assert api.offt_hip_half_box_pruned(po) and api.offt_hip_convolve_multi_fused(po)
        on, errs_on = _multi_outputs(po, case, dev, pr)
        assert L.offt_hip_set_option(po, OPT_CONV_MULTI_MIXED, 0) == 0
        assert api.offt_hip_half_box_pruned(po) and not api.offt_hip_convolve_multi_fused(po)
        off, errs_off = _multi_outputs(po, case, dev, pr)
    finally:
        api.offt_3d_fin(po)
    rel = [_rel(a, b) for a, b in zip(on, off)]     # inside the box; outside it nothing is compared
    print("multi mixed half box", case, "fused", errs_on, "generic", errs_off, "fused against generic", rel)
    assert max(errs_on) <= W.tol(case) and max(errs_off) <= W.tol(case) and max(rel) <= W.tol(case), (errs_on, errs_off, rel)


def test_multi_mixed_half_box_cpu(multi_cpu):
    CB = multi_cpu
    CB.cpu_backend_multi_log_reset()
    n0 = MW.counts(CB)
    _half_box_on_and_off(HW.Host(), 1)
    n1 = MW.counts(CB)
    # the fused call: one out-of-place and one in-place launch on half lines; the generic one: two multiplies
    assert n1["conv_oop"] - n0["conv_oop"] == 1 and n1["conv"] - n0["conv"] == 1, (n0, n1)
    assert n1["pointwise_oop"] - n0["pointwise_oop"] == 1 and n1["pointwise"] - n0["pointwise"] == 1, (n0, n1)
    log = MW.launches(CB)
    assert [r[5] for r in log if r[0] in (1, 2)] == [3, 3], "the fused launches of a pruned plan run on half lines"
    assert all(r[5] != 0 for r in log if r[0] == 0), "every pass of both calls is a half-line pass"


# ---- GPU tier ---------------------------------------------------------------------------------------------------------------
SENT = 8  # sentinel elements on either side of both arrays


# ---- 5. random out-of-place descriptors -------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("prec,n", INSTANCES)
def test_multi_mixed_random_oop_descriptors(kl, prec, n):
    import torch
    L = kl
    rng = np.random.default_rng(7300 + n + 7 * prec)
    assert L.offt_hipk_prepare(n, prec) == 0, L.offt_hipk_last_error()
    ft, ct = (np.float64, np.complex128) if prec == api.F64 else (np.float32, np.complex64)
    for half in (0, 3):
        for kind in (0, 1):
            for ncols in (5, 19):                            # never a whole number of panels (4, 8 or 16 columns)
                nb1 = 2
                pad, fpad = int(rng.integers(1, 4)), int(rng.integers(1, 4))
                scale = float(rng.choice([0.5, 1.0 / n, 3.0]))
                d, f = conv_desc(n, prec, ncols, nb1, pad=pad, fpad=fpad, kind=kind, scale=scale, half=half)
                f.mixed = 3
                assert L.offt_hipk_conv_oop_kernel_name(C.byref(d), C.byref(f)).decode() == \
                    ("fft_conv_oop_half_panelx_k" if half else "fft_conv_oop_panelx_k")
                nin = d.in_b1_stride * nb1 + 16
                nf = f.b1_stride * nb1 + 16
                nio = n // 2 if half else n
                x = (rng.standard_normal(nin) + 1j * rng.standard_normal(nin)).astype(ct)
                h = (rng.standard_normal(nf) + 1j * rng.standard_normal(nf)) if kind else rng.standard_normal(nf)
                lines = np.zeros(nin, dtype=bool)            # what the launch may write
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
                dc = torch.from_numpy(src.view(ft).copy()).cuda()     # the copy the in-place kernel works on
                dd = torch.from_numpy(dst.view(ft).copy()).cuda()
                dh = torch.from_numpy((h.astype(ct).view(ft) if kind else h.astype(ft)).copy()).cuda()
                torch.cuda.synchronize()
                rc = L.offt_hipk_conv_pass_oop(C.byref(d), C.byref(f), dh.data_ptr(), ds.data_ptr() + SENT * src.itemsize,
                                               dd.data_ptr() + SENT * dst.itemsize, None)
                assert rc == 0, L.offt_hipk_last_error()
                f.mixed = 1
                rc = L.offt_hipk_conv_pass(C.byref(d), C.byref(f), dh.data_ptr(), dc.data_ptr() + SENT * src.itemsize, None)
                assert rc == 0, L.offt_hipk_last_error()
                torch.cuda.synchronize()
                tag = (n, prec, half, kind, ncols)
                # (b) the source and everything around the destination's lines
                assert ds.cpu().numpy().tobytes() == src.view(ft).tobytes(), ("the source was written", tag)
                got = dd.cpu().numpy().view(ct)
                assert np.all(got[:SENT] == dst[:SENT]) and np.all(got[SENT + nin:] == dst[SENT + nin:]), ("sentinel overwritten", tag)
                mid = got[SENT:SENT + nin]
                assert np.all(mid[~lines] == dst[SENT:SENT + nin][~lines]), ("padding or upper halves written", tag)
                # (a) the same body with a second base: the bits of the in-place launch
                inpl = dc.cpu().numpy().view(ct)[SENT:SENT + nin]
                assert mid[lines].tobytes() == inpl[lines].tobytes(), ("differs from the in-place kernel", tag)
                # (c) numpy
                err = np.linalg.norm(mid[lines].astype(np.complex128) - want[lines]) / np.linalg.norm(want[lines])
                print("mixed oop descriptor", tag, "rel-L2", err)
                assert np.isfinite(err) and err <= (1e-12 if prec == api.F64 else 1e-5), (tag, err)
    # without both bits these lines have no out-of-place kernel: the launch fails, it runs nothing
    for mixed in (0, 1, 2):
        d, f = conv_desc(n, prec, 4, 1)
        f.mixed = mixed
        assert L.offt_hipk_conv_pass_oop(C.byref(d), C.byref(f), None, ds.data_ptr(), dd.data_ptr(), None) == -1


# ---- 6. one rank through the API --------------------------------------------------------------------------------------------
def _gpu_on_single_off(case, zgroup=None):
    """one plan: the multi call with both options on (fused), three single-output calls with OFFT_HIP_OPT_CONV_MIXED on, the
    multi call with OFFT_HIP_OPT_CONV_MULTI_MIXED off (generic).  (errors against numpy, multi against single calls,
    fused against generic)"""
    import torch
    L = api.lib()
    po = HW.make_plan(api, case)
    try:
        if zgroup is not None:
            assert L.offt_hip_set_option(po, OPT_ZGROUP_MIB, zgroup) == 0
        dev = HW.Gpu(torch)
        pr = MW.problem(case)
        c, ne = api.comm_dict(po), api.local_elems(po)
        assert not api.offt_hip_convolve_multi_fused(po), "the options are off by default"
        for o, v in BOTH:
            assert L.offt_hip_set_option(po, o, v) == 0, L.offt_hip_last_error()
        assert api.offt_hip_convolve_multi_fused(po) and api.offt_hip_convolve_fused(po), case
        on, errs = _multi_outputs(po, case, dev, pr)
        data, filts = MW.buffers(c, ne, case, pr[0], pr[1])
        kind = api.FILTER_COMPLEX if case.get("cplx") else api.FILTER_REAL
        idx = W.in_index(c, bool(case.get("r2c")))
        vs = []
        L.offt_hip_set_output_scale(po, MW.SCALE)
        for k, filt in enumerate(filts):
            (hs, ps), (_, pf) = dev.put(data), dev.put(filt)
            api.offt_hip_execute_convolve(po, ps, pf, kind)
            single = dev.get(hs, data)
            ref = W.check(c, case, single, pr[2][k])
            assert ref <= W.tol(case), (case, k, ref)
            b = (single.view(single.real.dtype)[idx] if case.get("r2c") else single[idx]).astype(on[k].dtype)
            vs.append(_rel(on[k], b))
        L.offt_hip_set_output_scale(po, 1.0)
        assert L.offt_hip_set_option(po, OPT_CONV_MULTI_MIXED, 0) == 0
        assert not api.offt_hip_convolve_multi_fused(po), case
        off, errs_off = _multi_outputs(po, case, dev, pr)
        assert max(errs_off) <= W.tol(case), (case, errs_off)
        return errs, vs, [_rel(a, b) for a, b in zip(on, off)]
    finally:
        api.offt_3d_fin(po)


@pytest.mark.gpu
@pytest.mark.parametrize("r2c", [0, 1])
@pytest.mark.parametrize("shape,f32", [((96, 40, 30), 0), ((192, 64, 67), 0), ((384, 16, 8), 1)])
def test_multi_mixed_one_rank_gpu(built, shape, f32, r2c):
    import torch
    torch.cuda.set_device(0)
    case = dict(N=list(shape), f32=f32, r2c=r2c, cplx=(r2c + f32) % 2, K=3, inplace=1)
    errs, vs, rel = _gpu_on_single_off(case)
    print("multi mixed", case, "vs numpy", errs, "vs single calls", vs, "vs the generic route", rel)
    assert max(errs) <= W.tol(case) and max(vs) <= 2 * W.tol(case) and max(rel) <= W.tol(case), (case, errs, vs, rel)


@pytest.mark.gpu
def test_multi_mixed_plane_groups_gpu(built):
    """(768, 24, 13) in double with 1 MiB groups: planes of 288 KiB, 3 per group, a last group of one plane.  That the
    library's loop runs exactly these groups is read off the launch log by test_multi_mixed_plane_groups_cpu on this shape
    and option -- the host loop is the same code on both backends.  The y pass of a group asks the fused launches to keep
    their stores; the mixed-radix instances have no keeping twin and run plain."""
    import torch
    torch.cuda.set_device(0)
    ng, cnt = _groups((768, 24, 13), 0, 0, 1)
    assert ng == 3 and cnt == 13 and cnt % ng == 1, "more than one plane group, the last one ragged"
    case = dict(N=[768, 24, 13], K=3, inplace=2)
    errs, vs, rel = _gpu_on_single_off(case, zgroup=1)
    print("multi mixed groups", case, "vs numpy", errs, "vs single calls", vs, "vs the generic route", rel)
    assert max(errs) <= W.tol(case) and max(vs) <= 2 * W.tol(case) and max(rel) <= W.tol(case), (case, errs, vs, rel)


# ---- 7. pruned half box -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_multi_mixed_pruned_half_box_gpu(built):
    import torch
    torch.cuda.set_device(0)
    for inplace in (None, 1):
        _half_box_on_and_off(HW.Gpu(torch), inplace)
