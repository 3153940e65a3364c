"""Filtered forward and filtered inverse at mixed-radix x lengths: OFFT_HIP_OPT_SPEC_MIXED (include/offt_hip.h), bit 4 of
offt_filter_desc::mixed (offt_amd/csrc/offt_hipk.h) and the kernels under them, fft_filt_fwd_panelx_k and
fft_filt_inv_panelx_k (filtx_body, offt_amd/csrc/offt_panel.hpp).

  * routing of the two launches without a device: every registered (precision, length) with bit 4 of the field, the same
    descriptors with every value that lacks it, the powers of two, and everything that has no kernel either way;
  * the host's route on the CPU backend of tests/cpu_backend_spec.c, read off its launch log: both options on = the fused
    route, either alone = the generic one; the layouts and lengths that never fuse; plane groups; the option's set / get
    round trip and its environment default;
  * -m gpu: descriptors of all 11 instances of both kernels (numpy line FFTs, sentinels, the source untouched, in place bit
    for bit what out of place gives, the same bits on a second launch), plans on one rank on both routes, the composition
    against the convolve, ragged plane groups, a caller-owned stream in async mode.

Tolerances are the project's own: 1e-12 / 1e-5 rel-L2 at kernel level, W.tol (1e-12 f64, 2e-5 f32) at plan level, 2 W.tol
between two routes of the library."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _conv_world as W
import _half_world as HW
import _spec_world as SW
from offt_amd import api
from test_convolve_multi import _groups
from test_spectral_filtered import _assert_routes, _run_both, filt_desc, kl, spec_cpu  # noqa: F401  (kl, spec_cpu: fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the registered instances (offt_reg_spec_mixed_*.hip)
LENGTHS = {api.F64: (96, 192, 320, 384, 640, 768, 1000), api.F32: (384, 640, 768, 1000)}
INSTANCES = [(prec, n) for prec, ns in LENGTHS.items() for n in ns]
OPT_ZGROUP_MIB, OPT_SPEC_FUSED, OPT_SPEC_MIXED = 0, 18, 21  # include/offt_hip.h
MIXED = [(OPT_SPEC_MIXED, 1)]   # on top of OFFT_HIP_OPT_SPEC_FUSED, which _run_both sets
FWD, INV = "fft_filt_fwd_panelx_k", "fft_filt_inv_panelx_k"
NONE = ("no fused kernel", "no fused kernel")


# ---- 1. routing without a device ------------------------------------------------------------------------------------------
def test_spec_mixed_kernel_routing_without_a_gpu(kl):
    L = kl
    names = lambda d, f: (L.offt_hipk_filt_fwd_kernel_name(C.byref(d), C.byref(f)).decode(),
                          L.offt_hipk_filt_inv_kernel_name(C.byref(d), C.byref(f)).decode())
    has = lambda d, f: L.offt_hipk_filt_has_fused(C.byref(d), C.byref(f))

    def desc(n, prec, mixed, **kw):
        d, f = filt_desc(n, prec, 7, 2, **kw)
        f.mixed = mixed
        return d, f

    assert len(INSTANCES) == 11
    for prec, n in INSTANCES:
        for kind in (0, 1):
            for keep in (0, 1):                              # no keeping twin: out_keep falls back to the plain instance
                for mixed in (8, 15):                        # bit 4 stands alone; bits 1-3 mean nothing here
                    d, f = desc(n, prec, mixed, kind=kind, keep=keep)
                    assert names(d, f) == (FWD, INV) and has(d, f) == 1, (n, prec, kind, keep, mixed)
                for mixed in range(8):
                    d, f = desc(n, prec, mixed, kind=kind, keep=keep)
                    assert names(d, f) == NONE and has(d, f) == 0, (n, prec, kind, keep, mixed)
        d, f = desc(n, prec, 8)
        d.in_contig, d.in_axis_stride, d.in_col_stride = 0, 8, 1   # strided lines
        assert names(d, f) == NONE and has(d, f) == 0
        d, f = desc(n, prec, 8)
        f.axis_stride = 8                                    # strided filter axis
        assert names(d, f) == NONE and has(d, f) == 0
        d, f = desc(n, prec, 8)
        d.in_split = n // 4                                  # a split line
        assert names(d, f) == NONE and has(d, f) == 0
        for ri in (1, 2):                                    # real rows
            d, f = desc(n, prec, 8)
            d.real_input = ri
            assert names(d, f) == NONE and has(d, f) == 0
        for half in (1, 2, 3):                               # half lines
            d, f = desc(n, prec, 8)
            d.half = half
            assert names(d, f) == NONE and has(d, f) == 0
    for prec in (api.F64, api.F32):
        for n in (48, 2048):                                 # swept but not registered; too long
            d, f = desc(n, prec, 8)
            assert names(d, f) == NONE and has(d, f) == 0, (n, prec)
        for n in (64, 128, 256, 512, 1024):                  # the powers of two do not care
            for mixed in (0, 8):
                d, f = desc(n, prec, mixed)
                assert names(d, f) == ("fft_filt_fwd_panel_k", "fft_filt_inv_panel_k") and has(d, f) == 1, (n, prec, mixed)
    d, f = desc(96, api.F32, 8)                              # single precision has no instance below 384 points
    assert names(d, f) == NONE and has(d, f) == 0


# ---- 2. the host's route on the CPU backend ---------------------------------------------------------------------------------
def _rel(a, b):
    a, b = a.astype(np.complex128), b.astype(np.complex128)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _on_and_off(case, dev, zgroup=None):
    """one plan: both calls with OFFT_HIP_OPT_SPEC_FUSED and OFFT_HIP_OPT_SPEC_MIXED on (fused), then with the second one off
    (generic).  Each route against numpy within W.tol, the two against each other within 2 W.tol, the spectrum unwritten where
    it is not an output."""
    L = api.lib()
    pr, res = SW.problem(case), {}
    po = HW.make_plan(api, case)
    try:
        if zgroup is not None:
            assert L.offt_hip_set_option(po, OPT_ZGROUP_MIB, zgroup) == 0
        assert not api.offt_hip_spectral_fused(po), "the options are off by default"
        assert L.offt_hip_set_option(po, OPT_SPEC_FUSED, 1) == 0
        for name, on in (("fused", 1), ("generic", 0)):
            assert L.offt_hip_set_option(po, OPT_SPEC_MIXED, on) == 0, L.offt_hip_last_error()
            assert api.offt_hip_spectral_fused(po) == bool(on), (case, name)
            ferr, fgot = SW.run_forward(api, po, case, dev, pr)
            ierrs, intact, outs = SW.run_inverse(api, po, case, dev, pr)
            assert intact is not False, (case, name, "the spectrum was written")
            c = api.comm_dict(po)
            res[name] = (ferr, ierrs, np.array(fgot, copy=True)[W.out_index(c)],
                         [o.view(o.real.dtype)[W.in_index(c, True)] if case.get("r2c") else o[W.in_index(c, False)] for o in outs])
    finally:
        api.offt_3d_fin(po)
    (ferr, ierrs, fa, oa), (gferr, gierrs, fb, ob) = res["fused"], res["generic"]
    between = [_rel(fa, fb)] + [_rel(a, b) for a, b in zip(oa, ob)]
    print("spec mixed", case, "zgroup", zgroup, "fused vs numpy", ferr, ierrs, "generic vs numpy", gferr, gierrs, "between", between)
    assert max([ferr, gferr] + ierrs + gierrs) <= W.tol(case), (case, ferr, ierrs, gferr, gierrs)
    assert max(between) <= 2 * W.tol(case), (case, between)


@pytest.mark.parametrize("r2c", [0, 1])
def test_spec_mixed_route_cpu(spec_cpu, r2c):
    CB = spec_cpu
    for cplx in (0, 1):
        for K, inplace in ((1, None), (3, 0), (3, None)):
            case = dict(N=[96, 8, 16], r2c=r2c, cplx=cplx, K=K, inplace=inplace)
            fused, fwd, inv = _run_both(CB, case, opts=MIXED)   # (_run_both holds every answer to numpy within W.tol)
            assert fused, case
            _assert_routes(case, True, fwd, inv)
            assert fwd[0]["pointwise"] == 0 and inv[0]["pointwise"] == 0 and inv[0]["pointwise_oop"] == 0, (case, fwd[0], inv[0])
            # either option alone, or neither: transform and multiply in separate launches
            for sf, opts in ((1, []), (0, MIXED), (None, MIXED), (None, [])):
                fused, fwd, inv = _run_both(CB, case, opts=opts, spec_fused=sf)
                assert not fused, (case, sf, opts)
                _assert_routes(case, False, fwd, inv)
    _on_and_off(dict(N=[96, 8, 16], r2c=r2c, cplx=1 - r2c, K=3, inplace=None if r2c else 1), HW.Host())


def test_spec_mixed_other_layouts_and_lengths_cpu(spec_cpu):
    CB = spec_cpu
    case = dict(N=[384, 4, 6], f32=1, cplx=1, K=3)
    fused, fwd, inv = _run_both(CB, case, opts=MIXED)
    assert fused
    _assert_routes(case, True, fwd, inv)
    _on_and_off(dict(case, inplace=0), HW.Host())
    # single precision has no 96; no instance at 12 points; S = 1 and the y-z-x layout are not z-y-x: generic with both options on
    for case in (dict(N=[96, 8, 16], f32=1), dict(N=[12, 10, 9]), dict(N=[96, 8, 16], params={"S": 1}), dict(N=[96, 96, 8], eq=1)):
        for r2c in (0, 1):
            case = dict(case, r2c=r2c, cplx=1 - r2c, K=3, inplace=None)
            fused, fwd, inv = _run_both(CB, case, opts=MIXED)
            assert not fused, case
            _assert_routes(case, False, fwd, inv)
    # a half box takes the generic route (the inverse of a half-box plan defines the box only: the forward is what is read)
    case = dict(N=[96, 8, 16], cplx=1, K=2)
    fused, fwd, _ = _run_both(CB, case, opts=MIXED, half=True)
    assert not fused
    assert fwd[0]["filt_fwd"] == 0 and fwd[0]["pointwise"] == 1 and fwd[0]["pass"] == 3, fwd[0]
    # a power-of-two plan does not care
    for opts in ([], MIXED):
        case = dict(N=[64, 8, 16], K=3, inplace=2)
        fused, fwd, inv = _run_both(CB, case, opts=opts)
        assert fused, opts
        _assert_routes(case, True, fwd, inv)
    fused, fwd, inv = _run_both(CB, case, opts=MIXED, spec_fused=0)
    assert not fused
    _assert_routes(case, False, fwd, inv)


def test_spec_mixed_plane_groups_cpu(spec_cpu):
    """1 MiB groups on 768 x 24 planes (288 KiB each in double): 3 planes per group, 13 planes -> 5 groups, the last of one
    plane (r2c: 7 planes -> 3 groups).  The host loop is the same code on the device: test_spec_mixed_plane_groups_gpu runs
    this shape and option there."""
    for r2c in (0, 1):
        ng, cnt_planes = _groups((768, 24, 13), 0, r2c, 1)
        assert ng == 3 and cnt_planes == (7 if r2c else 13)
        groups = -(-cnt_planes // ng)
        case = dict(N=[768, 24, 13], r2c=r2c, K=2, inplace=1)
        fused, fwd, inv = _run_both(spec_cpu, case, opts=MIXED + [(OPT_ZGROUP_MIB, 1)])
        assert fused
        _assert_routes(case, True, fwd, inv, groups=groups)
        want = [ng] * (groups - 1) + [cnt_planes - ng * (groups - 1)]
        assert want[-1] == 1 and sum(want) == cnt_planes
        assert [r[4] for r in fwd[1] if r[0] == 1] == want, fwd[1]     # planes per filtered launch: none lost, the last ragged
        assert [r[4] for r in inv[1] if r[0] == 2] == want * 2, inv[1]


# ---- 3. option plumbing -------------------------------------------------------------------------------------------------------
def test_spec_mixed_option_round_trip_cpu(spec_cpu):
    L = api.lib()
    assert api.OPT_SPEC_MIXED == OPT_SPEC_MIXED == 21 and api.OPT_SPEC_FUSED == OPT_SPEC_FUSED
    po = api.offt_3d_init(96, 8, 16)
    try:
        assert L.offt_hip_get_option(po, OPT_SPEC_MIXED) == 0, "off by default"
        assert not api.offt_hip_spectral_fused(po)
        assert L.offt_hip_set_option(po, OPT_SPEC_MIXED, 1) == 0, L.offt_hip_last_error()
        assert L.offt_hip_get_option(po, OPT_SPEC_MIXED) == 1 and not api.offt_hip_spectral_fused(po), "alone it changes nothing"
        assert L.offt_hip_set_option(po, OPT_SPEC_MIXED, 0) == 0 and L.offt_hip_set_option(po, OPT_SPEC_FUSED, 1) == 0
        assert not api.offt_hip_spectral_fused(po), "96 points have no power-of-two kernel"
        for v, want in ((1, 1), (0, 0), (5, 1), (0, 0), (1, 1)):
            assert L.offt_hip_set_option(po, OPT_SPEC_MIXED, v) == 0, L.offt_hip_last_error()
            assert L.offt_hip_get_option(po, OPT_SPEC_MIXED) == want
            assert api.offt_hip_spectral_fused(po) == bool(want)
            assert not api.offt_hip_convolve_fused(po), "the convolve does not read the option"
        assert L.offt_hip_set_option(po, OPT_SPEC_FUSED, 0) == 0
        assert L.offt_hip_get_option(po, OPT_SPEC_MIXED) == 1 and not api.offt_hip_spectral_fused(po)
        for unassigned in (15, 17, 22):
            assert L.offt_hip_set_option(po, unassigned, 1) == -1 and b"unknown option" in L.offt_hip_last_error()
            assert L.offt_hip_get_option(po, unassigned) == -1
    finally:
        api.offt_3d_fin(po)


_ENV_CHILD = """
import os, sys
sys.path[:0] = [%r, %r]
import cpu_world, _spec_world as SW
from offt_amd import api
cpu_world._cb_lib = SW.spec_cb_lib
cpu_world.install(0, 1, p1=1)
L = api.lib()
po = api.offt_3d_init(96, 8, 16)
v = L.offt_hip_get_option(po, 21)
f0 = int(api.offt_hip_spectral_fused(po))   # (OFFT_SPEC_FUSED is not set: the option alone changes nothing)
L.offt_hip_set_option(po, 18, 1)
f = int(api.offt_hip_spectral_fused(po))
# the environment after the plan exists changes nothing on it; the next plan reads it
os.environ["OFFT_SPEC_MIXED"] = "0" if v else "1"
v1, f1 = L.offt_hip_get_option(po, 21), int(api.offt_hip_spectral_fused(po))
p2 = api.offt_3d_init(96, 8, 16)
v2 = L.offt_hip_get_option(p2, 21)
print("RESULT", v, f0, f, v1, f1, v2)
api.offt_3d_fin(p2)
api.offt_3d_fin(po)
"""


def test_spec_mixed_environment_default(built):
    """OFFT_SPEC_MIXED is read once, by offt_3d_init, as the option's default"""
    subprocess.check_call(["make", "-s", "-C", ROOT, "tests/libcpubackend_spec.so"])
    for val, want in ((None, "RESULT 0 0 0 0 0 1"), ("1", "RESULT 1 0 1 1 1 0"), ("0", "RESULT 0 0 0 0 0 1")):
        env = {k: v for k, v in os.environ.items() if k not in ("OFFT_SPEC_MIXED", "OFFT_SPEC_FUSED")}
        if val is not None:
            env["OFFT_SPEC_MIXED"] = val
        p = subprocess.run([sys.executable, "-c", _ENV_CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=300)
        out = p.stdout.decode()
        assert p.returncode == 0 and want in out.splitlines(), (val, out[-2000:])


# ---- GPU tier ---------------------------------------------------------------------------------------------------------------
SENT = 8  # sentinel elements on either side of both arrays


# ---- 4. descriptors of both kernels, every instance -------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("prec,n", INSTANCES)
def test_spec_mixed_descriptors_gpu(kl, prec, n):
    """7 columns (no instance has a COLS that divides it: the column tail), two blocks, rows padded by 3 and filter rows by 5
    elements, scale 0.5.  96 and 1000 points (and 768 in double) have a predicated last butterfly."""
    import torch
    L = kl
    rng = np.random.default_rng(4100 + n + 7 * prec)
    assert L.offt_hipk_prepare(n, prec) == 0, L.offt_hipk_last_error()
    ft, ct = (np.float64, np.complex128) if prec == api.F64 else (np.float32, np.complex64)
    tol = 1e-12 if prec == api.F64 else 1e-5
    ncols, nb1, pad, fpad, scale = 7, 2, 3, 5, 0.5

    def gpu(a):
        return torch.from_numpy(a.view(ft).copy()).cuda()

    for kind in (0, 1):
        d, f = filt_desc(n, prec, ncols, nb1, pad=pad, fpad=fpad, kind=kind, scale=scale)
        f.mixed = 8
        assert L.offt_hipk_filt_fwd_kernel_name(C.byref(d), C.byref(f)).decode() == FWD
        assert L.offt_hipk_filt_inv_kernel_name(C.byref(d), C.byref(f)).decode() == INV
        nin = d.in_b1_stride * nb1 + 16
        nf = f.b1_stride * nb1 + 16
        x = (rng.standard_normal(nin) + 1j * rng.standard_normal(nin)).astype(ct)
        h = (rng.standard_normal(nf) + 1j * rng.standard_normal(nf)) if kind else rng.standard_normal(nf)
        lines = np.zeros(nin + 2 * SENT, dtype=bool)     # what a launch may write
        want = {w: np.zeros(nin, dtype=np.complex128) for w in ("fwd", "inv")}
        for b1 in range(nb1):
            for c in range(ncols):
                i = b1 * d.in_b1_stride + c * d.in_col_stride
                fo = b1 * f.b1_stride + c * f.col_stride
                H = h[fo:fo + n].astype(ct if kind else ft).astype(np.complex128)
                xin = x[i:i + n].astype(np.complex128)
                want["fwd"][i:i + n] = H * np.fft.fft(xin) * scale
                want["inv"][i:i + n] = np.fft.ifft(H * xin) * n * scale
                lines[SENT + i:SENT + i + n] = True
        src = np.full(nin + 2 * SENT, 7.0 + 7.0j, dtype=ct)
        src[SENT:SENT + nin] = x
        other = np.full(nin + 2 * SENT, -5.0 + 9.0j, dtype=ct)
        dh = gpu(h.astype(ct)) if kind else torch.from_numpy(h.astype(ft)).cuda()
        off = SENT * src.itemsize

        def launch(which, ds, dd):
            if which == "fwd":
                rc = L.offt_hipk_filt_pass_fwd(C.byref(d), C.byref(f), dh.data_ptr(), dd.data_ptr() + off, None)
            else:
                rc = L.offt_hipk_filt_pass_inv(C.byref(d), C.byref(f), dh.data_ptr(), ds.data_ptr() + off, dd.data_ptr() + off, None)
            assert rc == 0, L.offt_hipk_last_error()
            torch.cuda.synchronize()

        def check(which, got, before, tag):
            assert got[~lines].tobytes() == before[~lines].tobytes(), ("sentinel or padding written", tag)
            w = want[which][lines[SENT:SENT + nin]]
            err = np.linalg.norm(got[lines].astype(np.complex128) - w) / np.linalg.norm(w)
            print("mixed filt descriptor", tag, "rel-L2", err)
            assert np.isfinite(err) and err <= tol, (tag, err)

        # the forward, in place; a second launch on a fresh copy gives the same bits
        a, b = gpu(src), gpu(src)
        torch.cuda.synchronize()
        launch("fwd", a, a)
        launch("fwd", b, b)
        ga = a.cpu().numpy().view(ct)
        check("fwd", ga, src, (n, prec, "fwd", kind))
        assert b.cpu().numpy().tobytes() == ga.view(ft).tobytes(), ("a second launch gives other bits", n, prec, "fwd", kind)
        # the inverse out of place: the source bit-identical; again; in place: the bits of out of place
        s, o, o2, ip = gpu(src), gpu(other), gpu(other), gpu(src)
        torch.cuda.synchronize()
        launch("inv", s, o)
        launch("inv", s, o2)
        launch("inv", ip, ip)
        assert s.cpu().numpy().tobytes() == src.view(ft).tobytes(), ("the source was written", n, prec, kind)
        go = o.cpu().numpy().view(ct)
        check("inv", go, other, (n, prec, "inv", kind))
        assert o2.cpu().numpy().tobytes() == go.view(ft).tobytes(), ("a second launch gives other bits", n, prec, "inv", kind)
        gi = ip.cpu().numpy().view(ct)
        assert gi[~lines].tobytes() == src[~lines].tobytes(), ("in place: more than the lines written", n, prec, kind)
        assert gi[lines].tobytes() == go[lines].tobytes(), ("in place differs from out of place", n, prec, kind)
    # without bit 4 these lines have no filtered kernel: the launch fails, it runs nothing
    keep = o.cpu().numpy().tobytes()
    for mixed in (0, 7):
        d, f = filt_desc(n, prec, 4, 1)
        f.mixed = mixed
        assert L.offt_hipk_filt_pass_fwd(C.byref(d), C.byref(f), dh.data_ptr(), o.data_ptr() + off, None) == -1
        assert b"no filtered forward kernel" in L.offt_hipk_last_error()
        assert L.offt_hipk_filt_pass_inv(C.byref(d), C.byref(f), dh.data_ptr(), s.data_ptr() + off, o.data_ptr() + off, None) == -1
        assert b"no filtered inverse kernel" in L.offt_hipk_last_error()
    torch.cuda.synchronize()
    assert o.cpu().numpy().tobytes() == keep


# ---- 5. one rank through the API --------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape,f32,r2c", [((96, 8, 16), 0, 0), ((96, 8, 16), 0, 1), ((1000, 4, 6), 0, 0), ((1000, 4, 6), 0, 1),
                                           ((384, 4, 6), 1, 0)])
def test_spec_mixed_one_rank_gpu(built, shape, f32, r2c):
    import torch
    torch.cuda.set_device(0)
    dev = HW.Gpu(torch)
    # three outputs, one of them the spectrum; and none of them the spectrum, which then stays bit-identical
    for inplace in (1, None):
        _on_and_off(dict(N=list(shape), f32=f32, r2c=r2c, cplx=1 - r2c, K=3, inplace=inplace), dev)
    case = dict(N=list(shape), f32=f32, r2c=r2c, cplx=1 - r2c)
    po = HW.make_plan(api, case)
    try:
        for o in (OPT_SPEC_FUSED, OPT_SPEC_MIXED):
            assert api.lib().offt_hip_set_option(po, o, 1) == 0
        assert api.offt_hip_spectral_fused(po), case
        err, between, a = SW.run_compose(api, po, case, dev)
        _, _, b = SW.run_compose(api, po, case, dev)
        print("spec mixed composition", case, "vs numpy", err, "vs convolve", between)
        assert a.tobytes() == b.tobytes(), "the same two calls repeated differ"
        assert err <= W.tol(case) and between <= 2 * W.tol(case), (case, err, between)
    finally:
        api.offt_3d_fin(po)


@pytest.mark.gpu
@pytest.mark.parametrize("r2c", [0, 1])
def test_spec_mixed_plane_groups_gpu(built, r2c):
    """(768, 24, 13) in double with 1 MiB groups: planes of 288 KiB, 3 per group, a last group of one plane.  That the
    library's loop runs exactly these groups is read off the launch log by test_spec_mixed_plane_groups_cpu on this shape and
    option.  The y pass of a group asks the filtered launch to keep its stores; the mixed-radix instances have no keeping twin
    and run plain."""
    import torch
    torch.cuda.set_device(0)
    ng, cnt = _groups((768, 24, 13), 0, r2c, 1)
    assert ng == 3 and cnt == (7 if r2c else 13) and cnt % ng == 1, "more than one plane group, the last one ragged"
    _on_and_off(dict(N=[768, 24, 13], r2c=r2c, cplx=1 - r2c, K=2, inplace=0), HW.Gpu(torch), zgroup=1)


# ---- 6. a caller-owned stream in async mode -----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("call", ["forward_filtered", "inverse_filtered"])
def test_spec_mixed_on_caller_stream_gpu(built, call):
    """the protocol of tests/test_streams.py: the call on a caller-owned stream in asynchronous mode behind a delay, between a
    producer and a consumer on that stream, bit for bit the synchronous call on the plan's own stream"""
    from test_streams import _conv_gcase, _protocol
    _protocol(_conv_gcase(f"{call}-mixed", call, dict(N=[96, 8, 16], cplx=1), [(OPT_SPEC_FUSED, 1), (OPT_SPEC_MIXED, 1)], fused=True))
