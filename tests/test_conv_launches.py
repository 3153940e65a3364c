"""The launch sequences of the multi-output and the multi-input convolve and of the two filtered transforms, pinned: every
backend call of offt_hip_execute_convolve_multi, offt_hip_execute_convolve_sum, offt_hip_execute_forward_filtered and
offt_hip_execute_inverse_filtered on one rank (descriptors field by field, filter descriptors, buffers, strides, out_keep, the
scale, order, streams, event edges) and the routes a plan reports, against tests/golden/conv_launches.json.

The sibling of tests/test_single_rank_launches.py, whose Recorder it extends to the whole of offt_backend: memcpy_dd,
zero_outside, conv_pass_oop, pointwise_oop, conv_pass_sum, pointwise_sum, filt_pass_fwd and filt_pass_inv are logged too,
pointers, streams and events named as there ("data", "spec", "out1", "in0", "filter2" are the caller's arrays).  The tables are
those of tests/cpu_backend_multi.c, tests/cpu_backend_sum.c and tests/cpu_backend_spec.c, the older ones among them (no fused
launch; no multiply with a destination).

  python tests/test_conv_launches.py --record [<commit>]    rewrites the fixture (with the library that OFFT_AMD_TEST_LIB
                                                            names, built from <commit>)

As there, the fixture is a record of what the library did at one commit (its "recorded_from"), not of what it should do."""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tests")) if p not in sys.path]

import numpy as np

import _conv_multi_world as MW
import _conv_sum_world as SW
import _spec_world as SPW
import cpu_world
import test_single_rank_launches as SRL
from offt_amd import api
from test_convolve_multi import Desc, FDesc  # (offt_pass_desc with its `half` field, which test_convolve's leaves out)
from test_single_rank_launches import DESC_POINTERS, ENV_KEYS, LAYOUTS, I, LL, V

FIXTURE = os.path.join(ROOT, "tests", "golden", "conv_launches.json")
DESC_FIELDS = [f[0] for f in Desc._fields_]
FDESC_FIELDS = [f[0] for f in FDesc._fields_]

# offt_backend (offt_amd/csrc/offt_backend.h), entry by entry, to its end
TABLE_ENTRIES = SRL.TABLE_ENTRIES + ["zero_outside", "conv_pass_oop", "pointwise_oop", "conv_pass_sum", "pointwise_sum",
                                     "filt_pass_fwd", "filt_pass_inv"]


class Table(C.Structure):
    _fields_ = [(name, V) for name in TABLE_ENTRIES]


PV = C.POINTER(V)
SIGNATURES = dict(SRL.SIGNATURES,
                  **{"pass": C.CFUNCTYPE(I, C.POINTER(Desc), V, V, V)},
                  conv_pass=C.CFUNCTYPE(I, C.POINTER(Desc), C.POINTER(FDesc), V, V, V),
                  memcpy_dd=C.CFUNCTYPE(I, V, V, C.c_size_t, V),
                  zero_outside=C.CFUNCTYPE(I, V, I, I, I, I, I, I, I, LL, LL, LL, V),
                  conv_pass_oop=C.CFUNCTYPE(I, C.POINTER(Desc), C.POINTER(FDesc), V, V, V, V),
                  pointwise_oop=C.CFUNCTYPE(I, V, V, V, I, I, I, I, I, LL, LL, LL, V),
                  conv_pass_sum=C.CFUNCTYPE(I, C.POINTER(Desc), C.POINTER(FDesc), I, PV, PV, V, V),
                  pointwise_sum=C.CFUNCTYPE(I, I, PV, PV, V, I, I, I, I, I, LL, LL, LL, V),
                  filt_pass_fwd=C.CFUNCTYPE(I, C.POINTER(Desc), C.POINTER(FDesc), V, V, V),
                  filt_pass_inv=C.CFUNCTYPE(I, C.POINTER(Desc), C.POINTER(FDesc), V, V, V, V))


class Recorder(SRL.Recorder):
    table_type, signatures = Table, SIGNATURES

    def desc(self, dp):
        d = dp.contents
        return [self.ptr(getattr(d, f)) if f in DESC_POINTERS else getattr(d, f) for f in DESC_FIELDS]

    def _conv_pass(self, orig):
        def f(d, fl, filt, data, stream):
            self.log.append(["conv_pass", self.desc(d), self.fdesc(fl), self.ptr(filt), self.ptr(data), self.name("s", stream)])
            return orig(d, fl, filt, data, stream)
        return f

    def fdesc(self, fl):
        return [getattr(fl.contents, k) for k in FDESC_FIELDS]

    def ptrs(self, pp, n):
        return [self.ptr(pp[k]) for k in range(n)]

    def _memcpy_dd(self, orig):
        def f(dst, src, nbytes, stream):
            self.log.append(["memcpy_dd", self.ptr(dst), self.ptr(src), nbytes, self.name("s", stream)])
            return orig(dst, src, nbytes, stream)
        return f

    def _zero_outside(self, orig):
        def f(buf, prec, n0, n1, n2, k0, k1, k2, s0, s1, s2, stream):
            self.log.append(["zero_outside", self.ptr(buf), prec, n0, n1, n2, k0, k1, k2, s0, s1, s2, self.name("s", stream)])
            return orig(buf, prec, n0, n1, n2, k0, k1, k2, s0, s1, s2, stream)
        return f

    def _conv_pass_oop(self, orig):
        def f(d, fl, filt, src, dst, stream):
            self.log.append(["conv_pass_oop", self.desc(d), self.fdesc(fl), self.ptr(filt), self.ptr(src), self.ptr(dst),
                             self.name("s", stream)])
            return orig(d, fl, filt, src, dst, stream)
        return f

    def _pointwise_oop(self, orig):
        def f(src, dst, filt, prec, kind, n0, n1, n2, s0, s1, s2, stream):
            self.log.append(["pointwise_oop", self.ptr(src), self.ptr(dst), self.ptr(filt), prec, kind, n0, n1, n2, s0, s1, s2,
                             self.name("s", stream)])
            return orig(src, dst, filt, prec, kind, n0, n1, n2, s0, s1, s2, stream)
        return f

    def _conv_pass_sum(self, orig):
        def f(d, fl, nin, filts, srcs, dst, stream):
            self.log.append(["conv_pass_sum", self.desc(d), self.fdesc(fl), nin, self.ptrs(filts, nin), self.ptrs(srcs, nin),
                             self.ptr(dst), self.name("s", stream)])
            return orig(d, fl, nin, filts, srcs, dst, stream)
        return f

    def _pointwise_sum(self, orig):
        def f(nin, ins, filts, out, prec, kind, n0, n1, n2, s0, s1, s2, stream):
            self.log.append(["pointwise_sum", nin, self.ptrs(ins, nin), self.ptrs(filts, nin), self.ptr(out), prec, kind, n0, n1, n2,
                             s0, s1, s2, self.name("s", stream)])
            return orig(nin, ins, filts, out, prec, kind, n0, n1, n2, s0, s1, s2, stream)
        return f

    def _filt_pass_fwd(self, orig):
        def f(d, fl, filt, data, stream):
            self.log.append(["filt_pass_fwd", self.desc(d), self.fdesc(fl), self.ptr(filt), self.ptr(data), self.name("s", stream)])
            return orig(d, fl, filt, data, stream)
        return f

    def _filt_pass_inv(self, orig):
        def f(d, fl, filt, src, dst, stream):
            self.log.append(["filt_pass_inv", self.desc(d), self.fdesc(fl), self.ptr(filt), self.ptr(src), self.ptr(dst),
                             self.name("s", stream)])
            return orig(d, fl, filt, src, dst, stream)
        return f


# ---- the cases -----------------------------------------------------------------------------------------------------------
GRID = [64, 64, 40]                             # (x == y: the rotating y-z-x layout needs it)
CUBE = [64, 64, 64]                             # powers of two throughout: a half-box plan of it skips the padding (Nz = 40: clears it)
MIXED_GRID, MIXED_GRID_96 = [48, 64, 40], [96, 64, 40]  # mixed-radix x lengths
BOTH_MIXED = [(api.OPT_CONV_MIXED, 1), (api.OPT_CONV_MULTI_MIXED, 1)]
ZG0 = {"OFFT_ZGROUP_MIB": "0"}                  # plain launches (unset, this grid is ONE group of all its planes, stores kept)
ZG = {"OFFT_ZGROUP_MIB": "1"}                   # 1 MiB plane groups: 16 of the 40 z-planes of 64 x 64 in double, so three groups
SPEC = [(api.OPT_SPEC_FUSED, 1)]                # the filtered calls' fused route is opt-in


def all_cases():
    """a case: run ("multi" / "sum" / "fwdfilt" / "invfilt"), id, layout, N, r2c, f32, cplx (complex filter), env, K (outputs /
    inputs / filters), inplace (index of the output that is `data` or `spec` / of the input that is `out`, or None), opts
    (offt_hip_set_option pairs), half (1: half box on, the padding cleared; 2: on, every launch skips the padding), table (which
    backend table), fused (the route the call under test must take: the case is there for it)"""
    def case(run, cid, fused, **kw):
        return dict(dict(run=run, id=f"{run}-{cid}", fused=fused, layout="zyx", N=GRID, r2c=0, f32=0, cplx=0, env={}, K=2, inplace=None,
                         opts=[], half=0, table="full"), **kw)
    cases = [case("multi", "zyx-2out", 1), case("multi", "zyx-2out-zgroup1", 1, env=ZG), case("multi", "zyx-2out-zgroup0", 1, env=ZG0),
             case("multi", "zyx-3out-data-in-the-middle", 1, K=3, inplace=1),
             case("multi", "zyx-r2c-f32-cplx", 1, r2c=1, f32=1, cplx=1),
             case("multi", "zyx-48x64x40-conv_mixed", 0, N=MIXED_GRID, opts=[(api.OPT_CONV_MIXED, 1)]),
             # (48 is swept but has no registered fused mixed-radix kernel -- 96 is the shortest in double --, so both options
             # together still give the generic route there; at 96 they give the fused one)
             case("multi", "zyx-48x64x40-conv_mixed-multi_mixed", 0, N=MIXED_GRID, opts=BOTH_MIXED),
             case("multi", "zyx-96x64x40-conv_mixed", 0, N=MIXED_GRID_96, opts=[(api.OPT_CONV_MIXED, 1)]),
             case("multi", "zyx-96x64x40-conv_mixed-multi_mixed", 1, N=MIXED_GRID_96, opts=BOTH_MIXED),
             case("multi", "zyx-64x64x64-half-pruned", 1, N=CUBE, half=2),
             case("multi", "zyx-half-unpruned", 1, half=1),
             case("multi", "zyx-table_unfused", 0, table="unfused"), case("multi", "zyx-table_old", 0, table="old"),
             case("multi", "yzx_rot", 0, layout="yzx_rot"), case("multi", "xyz_inplace", 0, layout="xyz_inplace"),
             case("sum", "zyx-3in", 1, K=3), case("sum", "zyx-3in-zgroup1", 1, K=3, env=ZG), case("sum", "zyx-3in-zgroup0", 1, K=3, env=ZG0),
             case("sum", "zyx-2in-out-is-in0", 1, inplace=0),
             case("sum", "zyx-r2c-f32", 1, r2c=1, f32=1),
             case("sum", "zyx-64x64x64-half-pruned", 1, N=CUBE, half=2),
             case("sum", "zyx-half-unpruned", 1, half=1),
             case("sum", "zyx-table_nofused", 0, table="nofused"),
             case("sum", "yzx_rot", 0, layout="yzx_rot"), case("sum", "xyz_inplace", 0, layout="xyz_inplace")]
    # the filtered forward (one filter) and the filtered inverse (K outputs of one spectrum): the fused route in z-y-x with both
    # backend entries and OFFT_HIP_OPT_SPEC_FUSED set, the generic one everywhere else
    for run, kw in (("fwdfilt", dict(K=1)), ("invfilt", dict(K=2))):
        cases += [case(run, "zyx", 1, opts=SPEC, **kw), case(run, "zyx-zgroup1", 1, opts=SPEC, env=ZG, **kw),
                  case(run, "zyx-zgroup0", 1, opts=SPEC, env=ZG0, **kw),
                  case(run, "zyx-r2c-f32-cplx", 1, opts=SPEC, r2c=1, f32=1, cplx=1, **kw),
                  case(run, "zyx-spec_fused-off", 0, **kw), case(run, "zyx-half-unpruned", 0, opts=SPEC, half=1, **kw),
                  case(run, "zyx-table_nofilt", 0, opts=SPEC, table="nofilt", **kw),
                  case(run, "yzx_rot", 0, opts=SPEC, layout="yzx_rot", **kw),
                  case(run, "xyz_inplace", 0, opts=SPEC, layout="xyz_inplace", **kw)]
    cases += [case("invfilt", "zyx-3out-spec-in-the-middle", 1, opts=SPEC, K=3, inplace=1),
              case("invfilt", "zyx-1out-is-spec", 1, opts=SPEC, K=1, inplace=0),
              case("invfilt", "zyx-table_old", 0, opts=SPEC, table="old")]
    return cases


def is_filtered(case):
    return case["run"] in ("fwdfilt", "invfilt")


def run_case(rec, case):
    """plan (under the case's environment: the library reads it at plan time), run, and return the log"""
    L = api.lib()
    params, eq, rotate = LAYOUTS[case["layout"]]
    saved = {k: os.environ.pop(k, None) for k in ENV_KEYS}
    rec.begin()
    try:
        os.environ.update(case["env"])
        if rotate is not None:
            os.environ["OFFT_ROTATE"] = rotate
        po = api.offt_3d_init(*case["N"], custom_params=api.make_params(**params), is_equalxy=eq,
                              precision=api.F32 if case["f32"] else api.F64, is_r2c=case["r2c"])
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    try:
        for o, v in case["opts"]:
            assert L.offt_hip_set_option(po, o, v) == 0
        if case["half"]:
            api.offt_hip_set_half_box(po, True)
        ct = np.complex64 if case["f32"] else np.complex128
        ne, K, inplace = api.local_elems(po), case["K"], case["inplace"]
        filts = [np.ones(ne, dtype=ct if case["cplx"] else (np.float32 if case["f32"] else np.float64)) for _ in range(K)]
        rec.arrays = {f"filter{k}": f for k, f in enumerate(filts)}
        kind = api.FILTER_COMPLEX if case["cplx"] else api.FILTER_REAL
        L.offt_hip_set_output_scale(po, 0.5)  # (not 1.0: which launch carries the scale is part of the record)
        routes = [int(bool(q(po))) for q in (api.offt_hip_convolve_fused, api.offt_hip_convolve_multi_fused, api.offt_hip_convolve_sum_fused)]
        names = ["convolve_fused", "convolve_multi_fused", "convolve_sum_fused"]
        if is_filtered(case):
            names.append("spectral_fused")
            routes.append(int(bool(api.offt_hip_spectral_fused(po))))
        assert routes[{"multi": 1, "sum": 2}.get(case["run"], 3)] == case["fused"], (case["id"], routes)
        rec.log.append(names + routes)
        assert bool(api.offt_hip_half_box_pruned(po)) == (case["half"] == 2), case["id"]
        rec.log.append(["half_box_pruned", int(case["half"] == 2)])
        if case["run"] == "multi":
            data = np.zeros(ne, dtype=ct)
            outs = [data if k == inplace else np.zeros(ne, dtype=ct) for k in range(K)]
            rec.arrays.update({"data": data}, **{f"out{k}": o for k, o in enumerate(outs) if o is not data})
            api.offt_hip_execute_convolve_multi(po, data.ctypes.data, [o.ctypes.data for o in outs], [f.ctypes.data for f in filts], kind)
        elif case["run"] == "fwdfilt":
            data = np.zeros(ne, dtype=ct)
            rec.arrays["data"] = data
            api.offt_hip_execute_forward_filtered(po, data.ctypes.data, filts[0].ctypes.data, kind)
        elif case["run"] == "invfilt":
            spec = np.zeros(ne, dtype=ct)
            outs = [spec if k == inplace else np.zeros(ne, dtype=ct) for k in range(K)]
            rec.arrays.update({"spec": spec}, **{f"out{k}": o for k, o in enumerate(outs) if o is not spec})
            api.offt_hip_execute_inverse_filtered(po, spec.ctypes.data, [o.ctypes.data for o in outs], [f.ctypes.data for f in filts], kind)
        else:
            ins = [np.zeros(ne, dtype=ct) for _ in range(K)]
            out = np.zeros(ne, dtype=ct) if inplace is None else ins[inplace]
            rec.arrays.update({f"in{k}": a for k, a in enumerate(ins)}, **({"out": out} if inplace is None else {}))
            api.offt_hip_execute_convolve_sum(po, [a.ctypes.data for a in ins], [f.ctypes.data for f in filts], out.ctypes.data, kind)
        return rec.log
    finally:
        api.offt_3d_fin(po)


def run_all():
    """{case id: log} for every case"""
    subprocess.check_call(["make", "-s", "-C", ROOT, "tests/libcpubackend.so", "tests/libcpubackend_multi.so", "tests/libcpubackend_sum.so",
                           "tests/libcpubackend_spec.so"])
    cpu_world.install(0, 1)  # (the library routing; the table is replaced below)
    L = api.lib()
    M, S, F = MW.multi_cb_lib(), SW.sum_cb_lib(), SPW.spec_cb_lib()
    recs = {("multi", "full"): Recorder(M.cpu_backend_multi_table()), ("multi", "unfused"): Recorder(M.cpu_backend_multi_table_unfused()),
            ("multi", "old"): Recorder(M.cpu_backend_multi_table_old()), ("sum", "full"): Recorder(S.cpu_backend_sum_table()),
            ("sum", "nofused"): Recorder(S.cpu_backend_sum_table_nofused())}
    for run in ("fwdfilt", "invfilt"):  # (a recorder per run kind, as above; the three tables are statics of their own)
        recs.update({(run, "full"): Recorder(F.cpu_backend_spec_table()), (run, "nofilt"): Recorder(F.cpu_backend_spec_table_nofilt()),
                     (run, "old"): Recorder(F.cpu_backend_spec_table_old())})
    out = {}
    try:
        for case in all_cases():
            rec = recs[case["run"], case["table"]]
            L.offt_hip_test_set_backend(C.addressof(rec.table), 0, 1)
            out[case["id"]] = run_case(rec, case)
    finally:
        cpu_world.uninstall()
    assert len(out) == len(all_cases()), "case ids must be unique"
    return out


def test_conv_launches(built, capfd):
    want = json.load(open(FIXTURE))
    assert want["desc_fields"] == DESC_FIELDS and want["filter_fields"] == FDESC_FIELDS
    got = json.loads(json.dumps(run_all()))
    capfd.readouterr()  # (the plans' own prints)
    assert sorted(got) == sorted(want["cases"])
    for cid in got:
        for k, (g, w) in enumerate(zip(got[cid], want["cases"][cid])):
            assert g == w, f"{cid}: backend call {k} differs"
        assert len(got[cid]) == len(want["cases"][cid]), cid


if __name__ == "__main__":
    if sys.argv[1:2] != ["--record"] or len(sys.argv) > 3:
        sys.exit("usage: test_conv_launches.py --record [<commit the library was built from>]")
    head = {"recorded_from": sys.argv[2] if len(sys.argv) > 2 else "", "desc_fields": DESC_FIELDS, "filter_fields": FDESC_FIELDS}
    cases = run_all()
    with open(FIXTURE, "w") as f:  # one backend call per line
        f.write("{" + "".join(f"{json.dumps(k)}: {json.dumps(v)},\n " for k, v in head.items()) + '"cases": {\n')
        f.write(",\n".join("  %s: [\n%s]" % (json.dumps(cid), ",\n".join("   " + json.dumps(e, separators=(",", ":")) for e in log))
                           for cid, log in cases.items()))
        f.write("\n }}\n")
    print(f"{len(cases)} cases, {os.path.getsize(FIXTURE)} bytes -> {FIXTURE}")
