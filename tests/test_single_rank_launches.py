"""The launch sequence of the single-rank path, pinned: every backend call an execute makes (descriptors field by field,
buffers, order, streams, event edges) and the convolve route a plan reports, against tests/golden/single_rank_launches.json.

The value tests run on a descriptor interpreter that ignores the coalescing hints, the cache hint, the variant and the
launch order; this one sees them.  The CPU backend is installed as cpu_world.install() does, but through a COPY of its table
whose dmalloc / pass / conv_pass / pointwise / event_record / stream_wait entries log and then forward to the original.
Pointers are logged as (allocation, byte offset) -- "data" and "filter" are the caller's arrays, a number is the n-th
allocation of the plan --, streams and events by order of first appearance, so that the log does not depend on the run.

  python tests/test_single_rank_launches.py --record [<commit>]    rewrites the fixture (with the library that
                                                                   OFFT_AMD_TEST_LIB names, built from <commit>)

The fixture is a record of what the library did at one commit (its "recorded_from"), not of what it should do: rewrite it
only together with a change that is MEANT to alter a schedule."""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tests")) if p not in sys.path]

import numpy as np

import _conv_world as W
import cpu_world
from offt_amd import api
from test_convolve import Desc, FDesc

FIXTURE = os.path.join(ROOT, "tests", "golden", "single_rank_launches.json")
DESC_FIELDS = [f[0] for f in Desc._fields_]
DESC_POINTERS = ("in_block_tab", "out_block_tab", "tw4")
FDESC_FIELDS = [f[0] for f in FDesc._fields_]

# offt_backend (offt_amd/csrc/offt_backend.h), entry by entry
TABLE_ENTRIES = ["dmalloc", "dfree", "prepare", "pass", "stream_create", "stream_destroy", "event_create", "event_destroy",
                 "event_record", "stream_wait", "stream_sync", "event_ms", "a2a", "memcpy_dd", "upload", "peer_open", "peer_close",
                 "flag_alloc", "flag_free", "flag_signal", "flag_wait", "conv_pass", "pointwise"]


class Table(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in TABLE_ENTRIES]


V, I, LL = C.c_void_p, C.c_int, C.c_longlong
SIGNATURES = {"dmalloc": C.CFUNCTYPE(V, C.c_size_t),
              "pass": C.CFUNCTYPE(I, C.POINTER(Desc), V, V, V),
              "conv_pass": C.CFUNCTYPE(I, C.POINTER(Desc), C.POINTER(FDesc), V, V, V),
              "pointwise": C.CFUNCTYPE(I, V, V, I, I, I, I, I, LL, LL, LL, V),
              "event_record": C.CFUNCTYPE(I, V, V),
              "stream_wait": C.CFUNCTYPE(I, V, V)}


class Recorder:
    """a copy of a backend table whose logged entries append to self.log and forward to the original's"""

    table_type, signatures = Table, SIGNATURES  # (a subclass that logs more entries names a longer table: test_conv_launches.py)

    def __init__(self, table_addr):
        self.table = self.table_type.from_buffer_copy(C.string_at(table_addr, C.sizeof(self.table_type)))
        self._callbacks = []  # (the copied struct and its callbacks must outlive the installation)
        for name, sig in self.signatures.items():
            orig = getattr(self.table, name)
            if not orig:
                continue  # (the plain table has no conv_pass / pointwise: they stay NULL)
            cb = sig(getattr(self, "_" + name)(sig(orig)))
            self._callbacks.append(cb)
            setattr(self.table, name, C.cast(cb, V).value)
        self.begin()

    def begin(self):
        """a new case: forget the allocations, streams and events of the last one"""
        self.log, self.allocs, self.names, self.arrays = [], [], {}, {}

    def ptr(self, p):
        if not p:
            return None
        for name, a in self.arrays.items():  # the caller's (numpy) arrays
            if a.ctypes.data <= p < a.ctypes.data + a.nbytes:
                return [name, p - a.ctypes.data]
        for k in range(len(self.allocs) - 1, -1, -1):
            base, size = self.allocs[k]
            if base <= p < base + size:
                return [k, p - base]
        raise AssertionError(f"a launch points outside every known allocation: {p:#x}")

    def name(self, kind, p):
        """streams ("s") and events ("e") by order of first appearance"""
        if not p:
            return None
        if (kind, p) not in self.names:
            self.names[kind, p] = kind + str(sum(1 for k, _ in self.names if k == kind))
        return self.names[kind, p]

    def desc(self, dp):
        d = dp.contents
        return [self.ptr(getattr(d, f)) if f in DESC_POINTERS else getattr(d, f) for f in DESC_FIELDS]

    def _dmalloc(self, orig):
        def f(nbytes):
            p = orig(nbytes)
            self.log.append(["dmalloc", nbytes])
            if p:
                self.allocs.append((p, nbytes))
            return p
        return f

    def _pass(self, orig):
        def f(d, src, dst, stream):
            self.log.append(["pass", self.desc(d), self.ptr(src), self.ptr(dst), self.name("s", stream)])
            return orig(d, src, dst, stream)
        return f

    def _conv_pass(self, orig):
        def f(d, fl, filt, data, stream):
            self.log.append(["conv_pass", self.desc(d), [getattr(fl.contents, k) for k in FDESC_FIELDS], self.ptr(filt),
                             self.ptr(data), self.name("s", stream)])
            return orig(d, fl, filt, data, stream)
        return f

    def _pointwise(self, orig):
        def f(data, filt, prec, kind, n0, n1, n2, s0, s1, s2, stream):
            self.log.append(["pointwise", self.ptr(data), self.ptr(filt), prec, kind, n0, n1, n2, s0, s1, s2, self.name("s", stream)])
            return orig(data, filt, prec, kind, n0, n1, n2, s0, s1, s2, stream)
        return f

    def _event_record(self, orig):
        def f(e, s):
            self.log.append(["event_record", self.name("e", e), self.name("s", s)])
            return orig(e, s)
        return f

    def _stream_wait(self, orig):
        def f(s, e):
            self.log.append(["stream_wait", self.name("s", s), self.name("e", e)])
            return orig(s, e)
        return f


# ---- the cases -----------------------------------------------------------------------------------------------------------
# layout -> (custom params, is_equalxy, OFFT_ROTATE)
LAYOUTS = {"zyx": ({}, 0, None), "xyz_inplace": ({"S": 1}, 0, "0"), "xyz_rot": ({"S": 1}, 0, "1"),
           "yzx_rot": ({}, 1, "1"), "yzx_scratch": ({}, 1, "0")}
GRIDS = [[64, 64, 40], [32, 32, 32]]  # distinct extents (x == y: the y-z-x layouts need it), and a cube


def all_cases():
    """a case: layout, N, r2c, f32, env (OFFT_ZGROUP_*), and what to run -- "transform" (forward, then inverse; with
    "asyn" both once more in asynchronous mode, without the timing events) or "convolve" with a real (cplx 0) or complex
    filter"""
    cases = []
    for lay in LAYOUTS:
        for N in GRIDS:
            for r2c in (0, 1):
                for f32 in (0, 1):
                    cases.append(dict(layout=lay, N=N, r2c=r2c, f32=f32, env={}, run="transform", asyn=int(N == GRIDS[0] and not f32)))
    # the Infinity-Cache plane groups: off, and 1 MiB groups (several per transform at this size) on one and on two streams
    for lay in ("zyx", "xyz_inplace"):
        for r2c in (0, 1):
            for env in ({"OFFT_ZGROUP_MIB": "0"}, {"OFFT_ZGROUP_MIB": "1", "OFFT_ZGROUP_STREAMS": "1"},
                        {"OFFT_ZGROUP_MIB": "1", "OFFT_ZGROUP_STREAMS": "2"}):
                cases.append(dict(layout=lay, N=GRIDS[0], r2c=r2c, f32=0, env=env, run="transform", asyn=0))
    # spectral convolution: z-y-x and rotating y-z-x take the fused route, in-place x-y-z the unfused one
    for lay in ("zyx", "yzx_rot", "xyz_inplace"):
        for r2c in (0, 1):
            for cplx in (0, 1):
                cases.append(dict(layout=lay, N=GRIDS[0], r2c=r2c, f32=0, env={}, run="convolve", cplx=cplx))
    for lay in ("zyx", "yzx_rot"):
        cases.append(dict(layout=lay, N=GRIDS[0], r2c=0, f32=0, env={"OFFT_ZGROUP_MIB": "1"}, run="convolve", cplx=0))
        cases.append(dict(layout=lay, N=GRIDS[1], r2c=1, f32=1, env={"OFFT_ZGROUP_MIB": "0"}, run="convolve", cplx=1))
    return cases


def case_id(c):
    return "-".join([c["layout"], "x".join(map(str, c["N"])), "r2c" if c["r2c"] else "c2c", "f32" if c["f32"] else "f64",
                     c["run"] + (str(c["cplx"]) if c["run"] == "convolve" else "")] + [f"{k[5:]}={v}" for k, v in sorted(c["env"].items())])


ENV_KEYS = ("OFFT_ROTATE", "OFFT_S1_INPLACE", "OFFT_ZGROUP_MIB", "OFFT_ZGROUP_STREAMS")


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
        ct = np.complex64 if case["f32"] else np.complex128
        data = np.zeros(api.local_elems(po), dtype=ct)
        filt = np.ones(api.local_elems(po), dtype=ct if case.get("cplx") else data.real.dtype)
        rec.arrays = {"data": data, "filter": filt}
        L.offt_hip_set_output_scale(po, 0.5)  # (not 1.0: which launch carries the scale is part of the record)
        rec.log.append(["convolve_fused", bool(api.offt_hip_convolve_fused(po))])
        if case["run"] == "convolve":
            api.offt_hip_execute_convolve(po, data.ctypes.data, filt.ctypes.data, api.FILTER_COMPLEX if case["cplx"] else api.FILTER_REAL)
        else:
            for asyn in range(1 + case["asyn"]):
                L.offt_hip_set_async(po, asyn)
                for direction in (-1, +1):
                    rec.log.append(["execute", direction, "async" if asyn else "timed"])
                    api.offt_3d_execute_dir(po, data.ctypes.data, data.ctypes.data, direction)
                    assert L.offt_hip_wait(po) == 0
                    rec.log.append(["passes_paired", L.offt_hip_last_passes_paired(po)])
        return rec.log
    finally:
        api.offt_3d_fin(po)


def run_all():
    """{case id: log} for every case, on the plain CPU table (complex transforms) and the convolution table (real-input
    plans, whose inverse ends in a real-output pass only that table interprets, and convolves)"""
    subprocess.check_call(["make", "-s", "-C", ROOT, "tests/libcpubackend.so", "tests/libcpubackend_conv.so"])
    CB = cpu_world.install(0, 1)  # (the library routing and the all-to-all callback; the table is replaced below)
    L = api.lib()
    plain = Recorder(CB.cpu_backend_table())
    conv = Recorder(W.conv_cb_lib().cpu_backend_conv_table())
    out = {}
    try:
        for case in all_cases():
            rec = conv if case["r2c"] or case["run"] == "convolve" else plain
            L.offt_hip_test_set_backend(C.addressof(rec.table), 0, 1)
            out[case_id(case)] = run_case(rec, case)
    finally:
        cpu_world.uninstall()
    assert len(out) == len(all_cases()), "case ids must be unique"
    return out


def test_single_rank_launches(built, capfd):
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
        sys.exit("usage: test_single_rank_launches.py --record [<commit the library was built from>]")
    head = {"recorded_from": sys.argv[2] if len(sys.argv) > 2 else "", "desc_fields": DESC_FIELDS, "filter_fields": FDESC_FIELDS}
    cases = run_all()
    with open(FIXTURE, "w") as f:  # one backend call per line
        f.write("{" + "".join(f"{json.dumps(k)}: {json.dumps(v)},\n " for k, v in head.items()) + '"cases": {\n')
        f.write(",\n".join("  %s: [\n%s]" % (json.dumps(cid), ",\n".join("   " + json.dumps(e, separators=(",", ":")) for e in log))
                           for cid, log in cases.items()))
        f.write("\n }}\n")
    print(f"{len(cases)} cases, {os.path.getsize(FIXTURE)} bytes -> {FIXTURE}")
