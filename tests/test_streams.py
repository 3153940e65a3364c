"""Every execute call on a caller-owned stream (offt_hip_set_stream) in asynchronous mode (offt_hip_set_async).

CPU tier: the launch graph.  tests/cpu_backend_streams.c logs every launch with its stream and every event_record,
stream_wait and stream_sync; tests/_stream_graph.py rebuilds happens-before and reports a launch that is not ordered behind
the caller's stream at entry (fork), not ahead of it at return (join), a host wait inside the call, and two unordered
launches that touch the same memory (hazard).  Routes: single rank plain, plane groups on one and two streams, the S = 1 and
is_equalxy layouts, the forced pipeline (slab and pencil, one and two comm streams, two K1 streams), gloo worlds of 2 and 4
ranks with the overlapped inverse, the convolve family, the filtered calls and the half box.  Checker self-tests: hand-written
logs, a real log with a stream_wait removed, and every edge of the library's edge-drop seam (OFFT_TEST_DROP_EDGE).

Intended host waits on the caller's stream in asynchronous mode, by route: one, on the long-line routes (four-step, lines
through scratch) -- the launcher's per-stream scratch drains its stream when it has to grow, so none after the first call of
the longest length on that stream.  It happens below the backend table, where the CPU tier cannot see it; the GPU tier runs it
in test_gpu_long_plan_regrows_scratch_behind_work_in_flight.  Every other route: none.  (In synchronous mode every call ends
in the bounded final wait of wait_compute; offt_hip_set_option / offt_hip_set_exchange drain the stream before they rebuild
buffers.)

GPU tier (-m gpu): the same calls on a torch stream T with no host synchronisation between the producer of the input, the
call and the consumer of the output.  A delay kernel holds T while the call is enqueued, so a side stream that did not fork
reads NaN; the output is cloned and poisoned right behind the call, so a side stream that did not join is caught too.  The
result must be bit-identical to the same call on a fresh plan with default settings, that one within the project's
tolerances against numpy, and the call must return within the delay D (else the run is inconclusive).

D per case (ms; `enqueue` = host time of the call on the plan's own stream, measured on an MI355X, D >= 5 x enqueue):

  case                          enqueue ms   D ms
  plain-f64-fwd                    0.018      20
  plain-f64-inv                    0.010      20
  plain-f32-fwd                    0.012      20
  plain-f32-inv                    0.010      20
  groups-s1-f64-fwd                0.075      20
  groups-s1-f64-inv                0.087      20
  groups-s1-f32-fwd                0.075      20
  groups-s1-r2c-fwd                0.080      20
  groups-s1-c2r-inv                0.082      20
  groups-s2-f64-fwd                0.151      20
  groups-s2-f64-inv                0.139      20
  groups-s2-f32-fwd                0.131      20
  groups-s2-r2c-fwd                0.148      20
  groups-s2-c2r-inv                0.168      20
  rot-S1-fwd                       0.014      20
  rot-S1-inv                       0.010      20
  rot-eq-fwd                       0.018      20
  rot-eq-inv                       0.010      20
  pipe-slab-fwd                    0.100      20
  pipe-slab-inv                    0.088      20
  pipe-pencil-fwd                  0.154      20
  pipe-pencil-inv                  0.137      20
  long-four-step                   0.029      20
  long-scratch-lines               0.072      20
  long-r2c                         0.090      20
  bluestein-first-call             1.317      50
  plan-time-kernel-first-call      0.047      50
  convolve-fused                   0.018      20
  convolve-generic                 0.021      20
  convolve-r2c                     0.015      20
  convolve-groups                  0.127      20
  convolve_multi-fused             0.079      20
  convolve_multi-generic           0.069      20
  convolve_multi-r2c               0.059      20
  convolve_multi-groups            0.168      20
  convolve_sum-fused               0.034      20
  convolve_sum-generic             0.077      20
  convolve_sum-r2c                 0.023      20
  convolve_sum-groups              0.131      20
  forward_filtered-fused           0.022      20
  forward_filtered-generic         0.013      20
  forward_filtered-fused-off       0.014      20
  forward_filtered-r2c             0.017      20
  forward_filtered-groups          0.104      20
  inverse_filtered-fused           0.021      20
  inverse_filtered-generic         0.066      20
  inverse_filtered-fused-off       0.055      20
  inverse_filtered-r2c             0.019      20
  inverse_filtered-groups          0.141      20
  half-clearing-forward            0.014      20
  half-clearing-convolve           0.055      20
  half-pruned-forward              0.018      20
  half-pruned-convolve             0.016      20
  two-long-plans                   0.102      20   (both calls behind one delay)
  two-live-plans                   0.301      20   (per stream)

(the largest of three measurements; for the two first-call cases the first of them is the first call of that length in the
process, hence their larger D; test_gpu_delays_are_five_times_the_enqueue_time holds the condition on every run)
"""
import ctypes as C
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import pytest

import _conv_world as W
import _half_world as HW
import _spec_world as SW
import _stream_graph as SG
from offt_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT_ZGROUP_MIB, OPT_ZGROUP_STREAMS, OPT_COMM_STREAMS, OPT_K1_STREAMS = 0, 1, 3, 5
K = SG.KIND


# ---- checker self-tests on hand-written logs --------------------------------------------------------------------------------
def _g(*a):
    return np.array(a, dtype=np.uint64)


def _hand(fork=True, join=True, overlap=False):
    """S: mark, pass A, record e1; side waits e1 (the fork), pass B, record e2; S: pass C, waits e2 (the join), mark.  B and C
    are unordered: they may not touch the same memory."""
    S, X = 0x10, 0x20
    ops = [SG.Op("mark", S, value=SG.ENTRY), SG.Op("pass", S, reads=_g(1, 2), writes=_g(3, 4)), SG.Op("event_record", S, event=1)]
    if fork:
        ops.append(SG.Op("stream_wait", X, event=1))
    ops += [SG.Op("pass", X, reads=_g(3, 4), writes=_g(5, 6)), SG.Op("event_record", X, event=2),
            SG.Op("pass", S, reads=_g(3, 4), writes=_g(6, 7) if overlap else _g(7, 8))]
    if join:
        ops.append(SG.Op("stream_wait", S, event=2))
    ops.append(SG.Op("mark", S, value=SG.EXIT))
    return ops


def test_checker_accepts_a_correct_hand_written_log():
    assert SG.check(_hand()) == []


def test_checker_flags_a_missing_fork():
    v = SG.check(_hand(fork=False))
    assert any(s.startswith("fork") for s in v) and any(s.startswith("hazard") for s in v), v   # B reads what A writes


def test_checker_flags_a_missing_join():
    v = SG.check(_hand(join=False))
    assert [s.split(":")[0] for s in v] == ["join"], v


def test_checker_flags_an_overlapping_unordered_pair():
    v = SG.check(_hand(overlap=True))
    assert [s.split(":")[0] for s in v] == ["hazard"], v


def test_checker_flags_a_host_wait_and_a_stale_event():
    ops = _hand()
    ops.insert(5, SG.Op("stream_sync", 0x10))
    assert any(s.startswith("host wait") for s in SG.check(ops))
    assert SG.check(ops, allowed_syncs=("S",)) == []
    # an event recorded BEFORE the call orders nothing inside it: the wait sees the latest earlier record only
    ops = [SG.Op("event_record", 0x10, event=1)] + [o for o in _hand() if not (o.kind == K["event_record"] and o.event == 1)]
    assert any(s.startswith("fork") for s in SG.check(ops))


# ---- CPU tier: the library on the logging backend -----------------------------------------------------------------------------
@pytest.fixture()
def cb(built):
    import cpu_world
    orig = cpu_world._cb_lib
    cpu_world._cb_lib = SG.streams_cb_lib
    CB = cpu_world.install(0, 1, p1=1)
    CB.caller_streams = []
    yield CB
    CB.cpu_backend_streams_record_access(0)
    cpu_world.uninstall()
    cpu_world._cb_lib = orig
    for S in CB.caller_streams:     # (every plan that ran on them is gone by now)
        CB.cpu_backend_streams_free_stream(S)


def _traced(CB, po, call, warm=True, access=True):
    """`call` on a caller stream in async mode, once as a warm-up, then between the marks, with access recording on unless told
    otherwise"""
    L = api.lib()
    S = CB.cpu_backend_streams_new_stream()
    CB.caller_streams.append(S)
    L.offt_hip_set_stream(po, S)
    L.offt_hip_set_async(po, 1)
    if warm:
        call()
    CB.cpu_backend_streams_reset()
    CB.cpu_backend_streams_record_access(1 if access else 0)
    CB.cpu_backend_streams_mark(S, SG.ENTRY)
    res = call()
    CB.cpu_backend_streams_mark(S, SG.EXIT)
    ops = SG.read_log(CB)
    CB.cpu_backend_streams_record_access(0)
    return ops, res, S


def _shape_of(ops, S):
    launches = [o for o in ops if o.launch]
    return dict(launches=len(launches), streams=len({o.stream for o in launches}), side=sum(o.stream != S for o in launches),
                kinds=[o.name for o in launches], same=[o.desc.get("same", 0) for o in launches], waits=sum(o.kind == K["stream_wait"] for o in ops))


def _transform(CB, N, r2c=0, eq=0, params=None, opts=()):
    """forward and inverse of one plan, each traced: the violations, the shape of each log, and the answers against numpy"""
    po = api.offt_3d_init(*N, custom_params=api.make_params(**(params or {})), is_equalxy=eq, is_r2c=r2c)
    try:
        L = api.lib()
        for o, v in opts:
            assert L.offt_hip_set_option(po, o, v) == 0
        c, ne = api.comm_dict(po), api.local_elems(po)
        rng = np.random.default_rng(5 + sum(N))
        x = rng.standard_normal(N) if r2c else rng.standard_normal(N) + 1j * rng.standard_normal(N)
        F = np.fft.rfftn(x, axes=(0, 1, 2)) if r2c else np.fft.fftn(x)
        buf = np.zeros(ne, dtype=np.complex128)
        ptr = buf.ctypes.data_as(C.c_void_p)

        def fwd():
            buf[:] = 0
            if r2c:
                buf.view(np.float64)[W.in_index(c, True)] = x.ravel()
            else:
                buf[W.in_index(c, False)] = x.ravel()
            api.offt_3d_execute_dir(po, ptr, ptr, -1)
            return buf[W.out_index(c)].reshape(F.shape)

        def inv():
            buf[:] = 0
            buf[W.out_index(c)] = F.ravel()
            api.offt_3d_execute_dir(po, ptr, ptr, +1)
            got = buf.view(np.float64)[W.in_index(c, True)] if r2c else buf[W.in_index(c, False)]
            return got.reshape(N) / np.prod(N)
        out = {}
        for name, fn, want in (("forward", fwd, F), ("inverse", inv, x)):
            ops, got, S = _traced(CB, po, fn)
            assert np.linalg.norm(got - want) / np.linalg.norm(want) <= 1e-12, (N, name)
            out[name] = (ops, _shape_of(ops, S), S)
        return out
    finally:
        api.offt_3d_fin(po)


def _clean(res, what):
    for name, (ops, shape, _S) in res.items():
        assert SG.check(ops) == [], (what, name, shape)


@pytest.mark.parametrize("r2c", [0, 1])
def test_graph_single_rank_plain_and_layouts(cb, r2c):
    for N, kw in (((12, 10, 8), {}), ((12, 10, 8), dict(params={"S": 1})), ((8, 8, 6), dict(eq=1))):
        res = _transform(cb, N, r2c=r2c, opts=[(OPT_ZGROUP_MIB, 0)], **kw)
        _clean(res, (N, kw))
        for name, (ops, shape, _S) in res.items():
            assert shape["launches"] == 3 and shape["streams"] == 1, (N, kw, name, shape)   # plain launches on S alone


@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("N,r2c", [((256, 128, 5), 0), ((256, 128, 8), 1)])
def test_graph_plane_groups(cb, streams, N, r2c):
    """OFFT_HIP_OPT_ZGROUP_MIB = 1 with 512 KiB planes: groups of 2, 2 and 1 planes (the option counts whole MiB, so these are
    the smallest planes that give three groups; the hazard sets stay at some 10^5 granules a launch)"""
    res = _transform(cb, N, r2c=r2c, opts=[(OPT_ZGROUP_MIB, 1), (OPT_ZGROUP_STREAMS, streams)])
    _clean(res, (N, streams))
    for name, (ops, shape, S) in res.items():
        assert shape["launches"] == 1 + 2 * 3, (name, shape)                 # z; per group y, x (or x, y)
        assert shape["streams"] == streams and shape["side"] == (3 if streams == 2 else 0), (name, shape)
    if streams == 2:
        # the control on a real log: without any one of its stream_wait lines the checker objects
        ops = res["forward"][0]
        waits = [i for i, o in enumerate(ops) if o.kind == K["stream_wait"]]
        assert len(waits) == 4                                               # three forks, one join
        for i in waits:
            assert SG.check(ops[:i] + ops[i + 1:]) != [], ("removed wait", i)


def _pipeline(cb, monkeypatch, N, params, opts, env=None, r2c=0):
    monkeypatch.setenv("OFFT_FORCE_PIPELINE", "1")
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    return _transform(cb, N, r2c=r2c, params=params, opts=opts)


@pytest.mark.parametrize("r2c", [0, 1])
@pytest.mark.parametrize("comm,k1", [(1, 1), (2, 1), (1, 2)])
def test_graph_forced_pipeline_slab(cb, monkeypatch, comm, k1, r2c):
    """p = 1, z-y-x output: the slab schedule, four x-tiles; OFFT_FORCE_A2A sends the one block through the exchange, so the
    comm stream carries work"""
    res = _pipeline(cb, monkeypatch, (16, 8, 8), dict(T1=4, T2=4), [(OPT_COMM_STREAMS, comm), (OPT_K1_STREAMS, k1)], {"OFFT_FORCE_A2A": "1"}, r2c=r2c)
    _clean(res, ("slab", comm, k1))
    f = res["forward"][1]
    assert "a2a" in f["kinds"] and f["streams"] == (3 if k1 == 2 else 2), f
    assert "a2a" in res["inverse"][1]["kinds"] and res["inverse"][1]["streams"] == 2, res["inverse"][1]   # the overlapped inverse


@pytest.mark.parametrize("r2c", [0, 1])
@pytest.mark.parametrize("comm", [1, 2])
def test_graph_forced_pipeline_pencil(cb, monkeypatch, comm, r2c):
    """p = 1 with S = 1: the tile pipeline (ring of W1 + 1 slots), both exchanges forced"""
    res = _pipeline(cb, monkeypatch, (16, 8, 8), dict(T1=4, W1=1, T2=4, S=1), [(OPT_COMM_STREAMS, comm)], {"OFFT_FORCE_A2A": "1"}, r2c=r2c)
    _clean(res, ("pencil", comm))
    for name in ("forward", "inverse"):
        s = res[name][1]
        assert "a2a" in s["kinds"] and s["streams"] == 1 + comm, (name, s)


@pytest.mark.parametrize("r2c", [0, 1])
def test_graph_forced_pipeline_without_exchange(cb, monkeypatch, r2c):
    for N, params in (((16, 8, 8), dict(T1=4, T2=4)), ((16, 8, 8), dict(T1=4, W1=1, S=1))):
        res = _pipeline(cb, monkeypatch, N, params, [(OPT_K1_STREAMS, 2)], r2c=r2c)
        _clean(res, (N, params))


@pytest.mark.parametrize("kw", [dict(params={"S": 1}), dict(eq=1)], ids=["S1", "eq"])
def test_graph_rotating_layouts(cb, monkeypatch, kw):
    """the rotating schedules of the x-y-z and y-z-x layouts (through two scratch volumes; on the device where an x-plane is a
    whole number of MiB, here forced by OFFT_ROTATE=1): read off the launches -- no pass runs in place, where the schedule
    without the volumes (OFFT_ROTATE=0) has in-place passes"""
    same = {}
    for rot in ("1", "0"):
        monkeypatch.setenv("OFFT_ROTATE", rot)
        res = _transform(cb, (8, 8, 6), opts=[(OPT_ZGROUP_MIB, 0)], **kw)
        _clean(res, (kw, rot))
        same[rot] = {name: r[1]["same"] for name, r in res.items()}
    for name in ("forward", "inverse"):
        assert same["1"][name] == [0, 0, 0], (kw, name, same)
        assert sum(same["0"][name]) >= 1, (kw, name, same)


# ---- the convolve family, the filtered calls, the half box --------------------------------------------------------------------
def _conv_case(CB, case, call, opts=(), half=False, access=True):
    """one of the convolve / filtered calls traced; `call(po, pr, c, ne)` returns (closure, kinds that must be in the log)"""
    po = HW.make_plan(api, case)
    try:
        L = api.lib()
        for o, v in opts:
            assert L.offt_hip_set_option(po, o, v) == 0
        if half:
            api.offt_hip_set_half_box(po, True)
        fn = call(po)
        ops, res, S = _traced(CB, po, fn, access=access)
        return ops, _shape_of(ops, S), res
    finally:
        api.offt_3d_fin(po)


def _kind(case):
    return api.FILTER_COMPLEX if case.get("cplx") else api.FILTER_REAL


def _convolve_calls(case):
    """closures for the five calls on `case` (K = 2): name -> (po -> fn returning the rel-L2 error against numpy)"""
    N, r2c = case["N"], bool(case.get("r2c"))
    x, H, want = W.problem(N, r2c, case.get("cplx"))
    rng = np.random.default_rng(3)
    hs = H.shape
    H2 = rng.standard_normal(hs) + (1j * rng.standard_normal(hs) if case.get("cplx") else 0.0)
    x2 = rng.standard_normal(N) if r2c else rng.standard_normal(N) + 1j * rng.standard_normal(N)
    n = float(np.prod(N))
    fw = (lambda a: np.fft.rfftn(a, axes=(0, 1, 2))) if r2c else np.fft.fftn
    iv = (lambda a: np.fft.irfftn(a, s=N, axes=(0, 1, 2))) if r2c else np.fft.ifftn

    def setup(po):
        c, ne = api.comm_dict(po), api.local_elems(po)
        api.lib().offt_hip_set_output_scale(po, W.SCALE)
        return c, ne

    def conv(po):
        c, ne = setup(po)

        def fn():
            data, filt = W.local_arrays(c, ne, case, x, H)
            api.offt_hip_execute_convolve(po, data.ctypes.data, filt.ctypes.data, _kind(case))
            return W.check(c, case, data, want)
        return fn

    def multi(po):
        c, ne = setup(po)

        def fn():
            data, f1 = W.local_arrays(c, ne, case, x, H)
            _, f2 = W.local_arrays(c, ne, case, x, H2)
            o2 = np.zeros_like(data)
            api.offt_hip_execute_convolve_multi(po, data.ctypes.data, [data.ctypes.data, o2.ctypes.data], [f1.ctypes.data, f2.ctypes.data], _kind(case))
            return max(W.check(c, case, data, want), W.check(c, case, o2, iv(H2 * fw(x)) * n * W.SCALE))
        return fn

    def summ(po):
        c, ne = setup(po)

        def fn():
            d1, f1 = W.local_arrays(c, ne, case, x, H)
            d2, f2 = W.local_arrays(c, ne, case, x2, H2)
            api.offt_hip_execute_convolve_sum(po, [d1.ctypes.data, d2.ctypes.data], [f1.ctypes.data, f2.ctypes.data], d1.ctypes.data, _kind(case))
            return W.check(c, case, d1, iv(H * fw(x) + H2 * fw(x2)) * n * W.SCALE)
        return fn

    def ffwd(po):
        pr = SW.problem(dict(case, K=2))
        return lambda: SW.run_forward(api, po, case, HW.Host(), pr)[0]

    def finv(po):
        pr = SW.problem(dict(case, K=2))
        return lambda: max(SW.run_inverse(api, po, dict(case, K=2), HW.Host(), pr)[0])
    return dict(convolve=conv, convolve_multi=multi, convolve_sum=summ, forward_filtered=ffwd, inverse_filtered=finv)


FUSED_KIND = dict(convolve="conv", convolve_multi="conv_oop", convolve_sum="conv_sum", forward_filtered="filt_fwd", inverse_filtered="filt_inv")
GENERIC_KIND = dict(convolve="pointwise", convolve_multi="pointwise_oop", convolve_sum="pointwise_sum", forward_filtered="pointwise",
                    inverse_filtered="pointwise_oop")


@pytest.mark.parametrize("name", list(FUSED_KIND))
@pytest.mark.parametrize("route", ["fused", "generic", "fused_groups"])
def test_graph_convolve_family(cb, name, route):
    """fused: a 64-point x extent (the smallest with a fused kernel); generic: no such kernel at 12 points; fused_groups: the
    fused route over plane groups (r2c, 5 half-spectrum planes of 512 KiB: groups of 2, 2 and 1); these launch on the caller's
    stream alone, whatever OFFT_HIP_OPT_ZGROUP_STREAMS says"""
    if route == "fused":
        case, opts = dict(N=[64, 6, 4], cplx=1), [(api.OPT_SPEC_FUSED, 1)]
    elif route == "generic":
        case, opts = dict(N=[12, 10, 8]), [(api.OPT_SPEC_FUSED, 0)]
    else:
        case, opts = dict(N=[256, 128, 8], r2c=1), [(api.OPT_SPEC_FUSED, 1), (OPT_ZGROUP_MIB, 1), (OPT_ZGROUP_STREAMS, 2)]
    ops, shape, err = _conv_case(cb, case, _convolve_calls(case)[name], opts)
    assert err <= W.tol(case), (name, route, err)
    assert SG.check(ops) == [], (name, route, shape)
    want = GENERIC_KIND[name] if route == "generic" else FUSED_KIND[name]
    assert want in shape["kinds"], (name, route, shape)
    if route != "generic":
        assert GENERIC_KIND[name] not in shape["kinds"], (name, route, shape)
    if route == "fused_groups":
        # one fused launch per group and output (K = 2 for the multi-output call and the filtered inverse; the output that is
        # the source runs the in-place launch)
        fused = sum(k in ("conv", "conv_oop", "conv_sum", "filt_fwd", "filt_inv") for k in shape["kinds"])
        assert fused == 3 * (2 if name in ("convolve_multi", "inverse_filtered") else 1), (name, shape)
        assert shape["streams"] == 1, (name, shape)


@pytest.mark.parametrize("N,pruned", [([12, 10, 8], False), ([64, 64, 64], True)])
def test_graph_half_box(cb, N, pruned):
    """the clearing route (zero_outside on the caller's stream, then the ordinary schedule) and the pruned route"""
    case = dict(N=N)
    pr = HW.problem(N, False)
    for call in ("forward", "convolve"):
        def mk(po, call=call):
            assert api.offt_hip_half_box_pruned(po) == pruned
            c, ne = api.comm_dict(po), api.local_elems(po)
            api.lib().offt_hip_set_output_scale(po, HW.SCALE if call == "convolve" else 1.0)

            def fn():
                data = HW.poisoned_input(c, ne, case, pr["xp"])
                if call == "forward":
                    api.offt_3d_execute_dir(po, data.ctypes.data, data.ctypes.data, -1)
                    return SW.out_err(c, data, pr["spec"])
                filt = np.zeros(ne, dtype=np.complex128)
                filt[W.out_index(c)] = HW.out_block(c, pr["H"])
                api.offt_hip_execute_convolve(po, data.ctypes.data, filt.ctypes.data, api.FILTER_COMPLEX)
                return HW.box_err(c, case, data, pr["conv"])
            return fn
        # (64^3 with access recording would be a million granules a launch: the pruned route is checked for order only)
        ops, shape, err = _conv_case(cb, case, mk, half=True, access=not pruned)
        assert err <= HW.tol(case), (N, call, err)
        assert SG.check(ops) == [], (N, call, shape)
        assert ("zero" in shape["kinds"]) == (not pruned), (N, call, shape)
        assert any(o.desc.get("half") for o in ops if o.launch) == pruned, (N, call)


# ---- worlds of several ranks ----------------------------------------------------------------------------------------------------
def _gloo(size, cases, tmp_path):
    subprocess.check_call(["make", "-s", "-C", ROOT, "tests/libcpubackend_streams.so"])
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    procs = []
    for r in range(size):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(size), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_stream_graph.py"), "gloo", json.dumps(cases),
                                       str(tmp_path)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    try:
        outs = [p.communicate(timeout=300)[0].decode() for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    for r, p in enumerate(procs):
        assert p.returncode == 0, outs[r][-3000:]
    recs = [json.load(open(tmp_path / f"gloo_rank{r}.json")) for r in range(size)]
    for r in range(size):
        for rec in recs[r]:
            assert rec["violations"] == [], (r, rec)
            assert "a2a" in rec["kinds"] and rec["streams"] >= 2, (r, rec)     # the staged exchange on a comm stream
    return recs


def test_graph_gloo_world2(built, tmp_path):
    """two ranks: the slab schedule and its overlapped inverse, two K1 streams, r2c; S = 1: the pencil pipeline"""
    _gloo(2, [dict(N=[16, 16, 16], params={"T1": 4, "T2": 4}, inv=1),
              dict(N=[16, 16, 16], params={"T1": 4, "T2": 4}, inv=1, env={"OFFT_K1_STREAMS": "2"}),
              dict(N=[16, 12, 10], params={}, r2c=1, inv=1),
              dict(N=[8, 8, 8], params={"S": 1}, inv=1, env={"OFFT_COMM_STREAMS": "2"})], tmp_path)


def test_graph_gloo_world4(built, tmp_path):
    """four ranks as 2 x 2 (the pencil pipeline with both exchanges and its overlapped inverse, one and two comm streams) and as 1 x 4"""
    _gloo(4, [dict(N=[16, 16, 16], params={"P1": 2, "T1": 2, "W1": 1, "T2": 2}, inv=1),
              dict(N=[16, 16, 16], params={"P1": 2, "T1": 2, "W1": 1, "T2": 2}, inv=1, env={"OFFT_COMM_STREAMS": "2"}),
              dict(N=[16, 16, 16], params={"T1": 2, "T2": 2}, inv=1)], tmp_path)


# every edge of the edge-drop seam (offt_host.c, edge_dropped): the world whose schedule has the edge, run with it dropped
_SLAB = dict(N=[16, 16, 16], params={"T1": 4, "T2": 4})
_PENCIL = dict(N=[16, 16, 16], params={"P1": 2, "T1": 2, "W1": 1, "T2": 2})
EDGES = {1: (2, dict(_SLAB)), 2: (2, dict(_SLAB)), 3: (4, dict(_PENCIL)), 4: (4, dict(_PENCIL)), 5: (4, dict(_PENCIL)), 6: (4, dict(_PENCIL)),
         7: (2, dict(_SLAB, inv=1)), 8: (2, dict(_SLAB, inv=1)), 9: (2, dict(_SLAB, p2p=1, repeat=2)), 10: (2, dict(_SLAB, p2p=1, repeat=2)),
         11: (4, dict(_PENCIL, inv=1)), 12: (4, dict(_PENCIL, inv=1)), 13: (4, dict(_PENCIL, inv=1)), 14: (4, dict(_PENCIL, inv=1))}


def _world(size, case, tmp_path, drop=None):
    env = dict(os.environ)
    env.pop("OFFT_TEST_DROP_EDGE", None)
    if drop is not None:
        env["OFFT_TEST_DROP_EDGE"] = str(drop)
    out = tmp_path / f"world_{drop}.json"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_stream_graph.py"), "world", str(size), json.dumps([case]), str(out)],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode()[-3000:]
    return json.load(open(out))[0]


@pytest.mark.parametrize("world", ["slab", "slab_inv", "slab_p2p", "pencil", "pencil_inv"])
def test_graph_thread_worlds_are_clean(built, tmp_path, world):
    """the worlds of the edge controls with every edge in place: no violation (ranks as threads share one log, so the direct
    stores into a peer's memory and the flag edges between ranks are checked as well)"""
    size, case = {"slab": EDGES[1], "slab_inv": EDGES[7], "slab_p2p": EDGES[9], "pencil": EDGES[3], "pencil_inv": EDGES[11]}[world]
    rec = _world(size, case, tmp_path)
    assert rec["violations"] == [], rec
    assert ("flag_wait" if case.get("p2p") else "a2a") in rec["kinds"], rec


@pytest.mark.parametrize("edge", sorted(EDGES))
def test_checker_flags_every_dropped_edge(built, tmp_path, edge):
    size, case = EDGES[edge]
    rec = _world(size, case, tmp_path, drop=edge)
    assert rec["violations"] != [], (edge, rec)


# ---- GPU tier -------------------------------------------------------------------------------------------------------------------
pytest_gpu = pytest.mark.gpu
FIRST_CALL = ("bluestein-first-call", "plan-time-kernel-first-call")


def _delay_ms(name):
    """D of the table above: 50 ms for the two first-call cases, 20 ms for every other"""
    return 50 if name in FIRST_CALL else 20


NAN = float("nan")
ROUTE_BLUESTEIN, ROUTE_FOUR_STEP, ROUTE_SCRATCH_LINES = 2, 4, 5   # offt_hipk.h OFFT_ROUTE_*


def _torch():
    import torch
    return torch


def _glib():
    L = api.lib()
    L.offt_hipk_delay.argtypes = [C.c_double, C.c_void_p]
    return L


class _Env:
    """environment variables a plan reads at init, set for the duration of the plan's creation"""

    def __init__(self, env):
        self.env = env or {}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class GCase:
    """one call of the GPU tier: plan() makes a fresh plan (route options set, stream and mode left at their defaults),
    bufs(po) the buffers the call consumes (name -> numpy; NaN-poisoned around the call) and the constant ones (filters),
    call(po, ptrs) enqueues, check(po, outs) holds the synchronous result to numpy and asserts the route"""

    def __init__(self, name, plan, bufs, call, check, warm=True, prestage=None):
        self.name, self.plan, self.bufs, self.call, self.check, self.warm = name, plan, bufs, call, check, warm
        self.prestage = prestage   # warm = False: the buffers of bufs(po), made WITHOUT a plan (staged ahead of offt_3d_init)


def _real(a):
    return a.view(a.real.dtype) if np.iscomplexobj(a) else a


def _sync_twin(case):
    """the call on a fresh plan with default settings: own stream, synchronous, host syncs around"""
    torch = _torch()
    po = case.plan()
    try:
        work, const = case.bufs(po)
        dev = {k: torch.from_numpy(_real(v).copy()).cuda() for k, v in {**work, **const}.items()}
        torch.cuda.synchronize()
        case.call(po, {k: t.data_ptr() for k, t in dev.items()})
        torch.cuda.synchronize()
        ref = {k: dev[k].cpu().numpy() for k in work}
        case.check(po, {k: ref[k].view(work[k].dtype) for k in work})
        return ref
    finally:
        api.offt_3d_fin(po)


class _OnStream:
    """a plan of `case` on the caller stream T in asynchronous mode, its buffers on the device: data NaN, the input in staging"""

    def __init__(self, case, T, first_call=False):
        L = _glib()
        self.case, self.T = case, T
        if first_call:
            # everything the device needs is staged and waited for BEFORE the plan exists: from offt_3d_init to the call nothing
            # synchronises the device, so work the plan left unfinished at init would still be in flight
            work, const = case.prestage()
            self._stage(work, const)
            self.po = case.plan()
            planned = case.bufs(self.po)[0]
            assert all(np.array_equal(work[k], planned[k]) for k in work), "the plan's input layout is not the one staged"
        else:
            self.po = case.plan()
            self._stage(*case.bufs(self.po))
        L.offt_hip_set_stream(self.po, T.cuda_stream)
        L.offt_hip_set_async(self.po, 1)

    def _stage(self, work, const):
        torch = _torch()
        self.staging = {k: torch.from_numpy(_real(v).copy()).cuda() for k, v in work.items()}
        self.const = {k: torch.from_numpy(_real(v).copy()).cuda() for k, v in const.items()}
        self.data = {k: torch.full_like(t, NAN) for k, t in self.staging.items()}
        self.out = {k: torch.empty_like(t) for k, t in self.staging.items()}
        self.ptrs = {k: t.data_ptr() for k, t in {**self.data, **self.const}.items()}
        torch.cuda.synchronize()

    def warm_up(self):
        torch = _torch()
        for k in self.data:
            self.data[k].copy_(self.staging[k])
        torch.cuda.synchronize()
        self.case.call(self.po, self.ptrs)
        self.T.synchronize()
        assert _glib().offt_hip_wait(self.po) == 0
        for k in self.data:
            self.data[k].fill_(NAN)
        torch.cuda.synchronize()

    def enqueue(self, D):
        """on T, no host synchronisation in between: delay, producer, THE CALL, consumer, poison; returns the call's host ms"""
        torch = _torch()
        with torch.cuda.stream(self.T):
            if D:
                assert _glib().offt_hipk_delay(float(D), self.T.cuda_stream) == 0
            for k in self.data:
                self.data[k].copy_(self.staging[k], non_blocking=True)
            t0 = time.perf_counter()
            self.case.call(self.po, self.ptrs)
            host_ms = 1e3 * (time.perf_counter() - t0)
            for k in self.data:
                self.out[k].copy_(self.data[k], non_blocking=True)
                self.data[k].fill_(NAN)
        return host_ms

    def results(self):
        self.T.synchronize()
        assert _glib().offt_hip_wait(self.po) == 0
        return {k: t.cpu().numpy() for k, t in self.out.items()}

    def fin(self):
        api.offt_3d_fin(self.po)


def _assert_same(case, D, host_ms, got, ref):
    assert host_ms < D, f"{case.name}: INCONCLUSIVE, not a wrong result: the call took {host_ms:.2f} ms on the host, the delay is {D} ms"
    for k in ref:
        # bit for bit, as bytes: the padding of a half box keeps the NaN it came with on both sides
        assert np.array_equal(got[k].view(np.uint8), ref[k].view(np.uint8)), (case.name, k, "differs from the synchronous call on the plan's own stream",
                                                int(np.isnan(got[k]).sum()), "NaN")


def _protocol(case):
    torch = _torch()
    D = _delay_ms(case.name)
    if not case.warm:
        return _protocol_first_call(case, D)
    ref = _sync_twin(case)
    run = _OnStream(case, torch.cuda.Stream())
    try:
        run.warm_up()
        host_ms = run.enqueue(D)
        _assert_same(case, D, host_ms, run.results(), ref)
    finally:
        run.fin()


def _protocol_first_call(case, D):
    """the plan on T comes FIRST in the process for its lengths, and its first call follows offt_3d_init at once, without a
    delay (a delay would give work the plan left on another stream the time to finish); then the call again behind the delay;
    the synchronous twin, which would otherwise have built the tables, runs last"""
    torch = _torch()
    run = _OnStream(case, torch.cuda.Stream(), first_call=True)
    try:
        run.enqueue(0)
        first = run.results()
        host_ms = run.enqueue(D)
        again = run.results()
    finally:
        run.fin()
    ref = _sync_twin(case)
    _assert_same(case, D, 0.0, first, ref)
    _assert_same(case, D, host_ms, again, ref)


def enqueue_ms(case):
    """host time of the call on the plan's own stream, asynchronous, no delay, after one warm-up (what the table above holds)"""
    torch = _torch()
    L = _glib()
    po = case.plan()
    try:
        L.offt_hip_set_async(po, 1)
        work, const = case.bufs(po)
        dev = {k: torch.from_numpy(_real(v).copy()).cuda() for k, v in {**work, **const}.items()}
        ptrs = {k: t.data_ptr() for k, t in dev.items()}
        torch.cuda.synchronize()
        if case.warm:
            case.call(po, ptrs)
            assert L.offt_hip_wait(po) == 0
        t0 = time.perf_counter()
        case.call(po, ptrs)
        ms = 1e3 * (time.perf_counter() - t0)
        assert L.offt_hip_wait(po) == 0
        return ms
    finally:
        api.offt_3d_fin(po)


def _tol_check(got, want, f32):
    from test_gpu_parity import TOL32, check64
    if f32:
        assert np.linalg.norm(got.astype(np.complex128) - want) / np.linalg.norm(want) <= TOL32
    else:
        check64(got, want)


def _paired(po):
    return api.lib().offt_hip_last_passes_paired(po) != 0


def _tx(name, N, direction=-1, f32=0, r2c=0, eq=0, params=None, opts=(), env=None, route=None, warm=True):
    """a forward (-1) or inverse (+1) transform as a GCase; route(po): asserted on the synchronous twin after its call"""
    N = tuple(N)
    ct, ft = (np.complex64, np.float32) if f32 else (np.complex128, np.float64)
    rng = np.random.default_rng(17 + sum(N))
    x = (rng.standard_normal(N) if r2c else rng.standard_normal(N) + 1j * rng.standard_normal(N))
    x = x.astype(ft if r2c else ct)
    F = np.fft.rfftn(x.astype(np.float64), axes=(0, 1, 2)) if r2c else np.fft.fftn(x.astype(np.complex128))

    def plan():
        with _Env(env):
            po = api.offt_3d_init(*N, custom_params=api.make_params(**(params or {})), is_equalxy=eq, is_r2c=r2c,
                                  precision=api.F32 if f32 else api.F64)
        for o, v in opts:
            assert api.lib().offt_hip_set_option(po, o, v) == 0
        return po

    def bufs(po):
        c = api.comm_dict(po)
        buf = np.zeros(api.local_elems(po), dtype=ct)
        if direction < 0 and r2c:
            buf.view(ft)[W.in_index(c, True)] = x.ravel()
        elif direction < 0:
            buf[W.in_index(c, False)] = x.ravel()
        else:
            buf[W.out_index(c)] = F.astype(ct).ravel()
        return {"data": buf}, {}

    def prestage():   # the z-y-x plan of one rank reads x[i][j][k] at (i Ny + j) Nz + k: checked against bufs(po) once the plan exists
        assert direction < 0 and not r2c and not params and not eq
        return {"data": x.ravel().copy()}, {}

    def call(po, p):
        api.offt_3d_execute_dir(po, p["data"], p["data"], direction)

    def check(po, outs):
        c = api.comm_dict(po)
        if direction < 0:
            _tol_check(outs["data"][W.out_index(c)].reshape(F.shape), F, f32)
        else:
            got = outs["data"].view(ft)[W.in_index(c, True)] if r2c else outs["data"][W.in_index(c, False)]
            want = x.astype(np.float64 if r2c else np.complex128) * np.prod(N)
            if r2c:   # a real result: rel-L2 alone (check64's max-norm term is the same bound on complex data)
                assert np.linalg.norm(got.reshape(N) - want) / np.linalg.norm(want) <= (5e-6 if f32 else 1e-13)
            else:
                _tol_check(got.reshape(N), want, f32)
        if route:
            route(po)
    return GCase(name, plan, bufs, call, check, warm, prestage)


def _pipeline_taken(po):
    assert po.contents.t[api.PACK1] > 0 and po.contents.t[api.FFTz] == 0, "the plan did not run the tile pipeline"


def _groups_taken(N, f32=0, r2c=0):
    def route(po):
        planes = (N[2] // 2 + 1) if r2c else N[2]
        per = int(1.0 / (N[0] * N[1] * (8 if f32 else 16) / 2.0 ** 20))
        assert _paired(po) and per >= 1 and -(-planes // per) >= 5 and planes % per, (N, per, planes)   # >= 5 groups, a ragged last one
    return route


def _line_route(n, want, f32=0, real=0):
    """offt_hipk_pass_route of a strided line of n points, or of a real row of n points (real = 1): the launcher's own
    resolve(), after the plan prepared the length"""
    from test_spectral_filtered import Desc

    def route(po):
        L = api.lib()
        d = Desc()
        d.n, d.precision, d.direction, d.ncols, d.nb1, d.nb2 = n, api.F32 if f32 else api.F64, -1, 16, 1, 1
        d.in_axis_stride, d.in_col_stride, d.out_axis_stride, d.out_col_stride = 16, 1, 16, 1
        d.variant, d.scale = -1, 1.0
        if real:   # the z pass of a real-input plan: contiguous real rows in, n/2 + 1 values out
            d.real_input, d.in_contig, d.in_axis_stride, d.in_col_stride = 1, 1, 1, n // 2 + 1
        L.offt_hipk_pass_route.argtypes = [C.POINTER(Desc), C.c_void_p, C.c_void_p, C.c_void_p]
        got = L.offt_hipk_pass_route(C.byref(d), None, None, None)
        assert got in want, (n, got, want)
    return route


def _gpu_cases():
    cases = []
    add = cases.append
    # 1: plain single rank
    for f32 in (0, 1):
        for d in (-1, +1):
            add(_tx(f"plain-{'f32' if f32 else 'f64'}-{'fwd' if d < 0 else 'inv'}", (64, 32, 16), d, f32=f32, opts=[(OPT_ZGROUP_MIB, 0)]))
    # 2: plane groups, one and two streams.  (128, 128, 21) in f32 and the 12 half-spectrum planes of (128, 128, 22) give three
    # groups of 1 MiB; 41 planes in f32 (8 a group) and Nz = 40 (21 planes, 4 a group) are the next with >= 5 ragged groups
    for s in (1, 2):
        o = [(OPT_ZGROUP_MIB, 1), (OPT_ZGROUP_STREAMS, s)]
        add(_tx(f"groups-s{s}-f64-fwd", (128, 128, 21), -1, opts=o, route=_groups_taken((128, 128, 21))))
        add(_tx(f"groups-s{s}-f64-inv", (128, 128, 21), +1, opts=o, route=_groups_taken((128, 128, 21))))
        add(_tx(f"groups-s{s}-f32-fwd", (128, 128, 41), -1, f32=1, opts=o, route=_groups_taken((128, 128, 41), f32=1)))
        add(_tx(f"groups-s{s}-r2c-fwd", (128, 128, 40), -1, r2c=1, opts=o, route=_groups_taken((128, 128, 40), r2c=1)))
        add(_tx(f"groups-s{s}-c2r-inv", (128, 128, 40), +1, r2c=1, opts=o, route=_groups_taken((128, 128, 40), r2c=1)))
    # 3: rotating layouts with work volumes (an x-plane of 1 MiB: 256 x 256 x 16 B)
    # ((256, 256, 8) has x-planes of 32 KiB and keeps the older y-z-x schedule: the next is_equalxy shape that rotates is used)
    for nm, N, kw in (("rot-S1", (8, 256, 256), dict(params={"S": 1})), ("rot-eq", (64, 64, 1024), dict(eq=1))):
        def rot(po, eq=kw.get("eq", 0)):
            # a plan does not report its schedule on the device: the rule of offt_3d_init on what the plan does report (an x-plane
            # is a whole number of MiB; y-z-x also needs M1 = M4).  That the rule leads to the rotating launches is read off the
            # descriptors in test_graph_rotating_layouts.
            p, c = po.contents, api.comm_dict(po)
            assert (p.Ny * p.Nz * 16) % (1 << 20) == 0 and (not eq or (p.is_equalxy and c["M1"] == c["M4"])), (p.Nx, p.Ny, p.Nz)
        for d in (-1, +1):
            add(_tx(f"{nm}-{'fwd' if d < 0 else 'inv'}", N, d, route=rot, **kw))
    # 4: the forced pipeline on one GPU
    for nm, N, p, o in (("pipe-slab", (64, 64, 64), dict(T1=8, W1=2), [(OPT_K1_STREAMS, 2)]),
                        ("pipe-pencil", (32, 16, 64), dict(T1=5, W1=1, S=1), [(OPT_COMM_STREAMS, 2)])):
        for d in (-1, +1):
            add(_tx(f"{nm}-{'fwd' if d < 0 else 'inv'}", N, d, params=p, opts=o, env={"OFFT_FORCE_PIPELINE": "1"},
                    route=_pipeline_taken))
    # 5: long lines through per-stream scratch
    add(_tx("long-four-step", (4, 4, 6000), -1, route=_line_route(6000, (ROUTE_FOUR_STEP,))))
    add(_tx("long-scratch-lines", (4, 4, 10007), -1, route=_line_route(10007, (ROUTE_SCRATCH_LINES,))))
    add(_tx("long-r2c", (4, 4, 6122), -1, r2c=1, route=_line_route(6122, (ROUTE_SCRATCH_LINES,), real=1)))
    # 6: tables built at plan time, first call right after init (no warm-up).  The launcher's tables are kept per process by
    # (n, precision), so the lengths are ones no other test of the suite prepares: 139 for 127, 648 = 2^3 3^4 for 432
    add(_tx("bluestein-first-call", (139, 8, 4), -1, warm=False, route=_line_route(139, (ROUTE_BLUESTEIN,))))
    add(_tx("plan-time-kernel-first-call", (648, 6, 10), -1, warm=False, route=_line_route(648, (1,))))
    return cases


GPU_CASES = {c.name: c for c in _gpu_cases()}


@pytest_gpu
@pytest.mark.parametrize("name", [n for n in GPU_CASES])
def test_gpu_transform_on_caller_stream(built, name):
    _protocol(GPU_CASES[name])


# ---- case 7 and 8: the convolve family and the half box --------------------------------------------------------------------------
def _conv_gcase(name, call_name, case, opts=(), fused=None, half=False, pruned=None, groups=None):
    """one of the five calls (K = 2) as a GCase, on the problems of the convolve tests; fused / pruned / groups: the route
    asserted (groups: how many plane groups conv_plane_groups makes, from the plan's extents and its ZGROUP_MIB option by the
    rule of plane_group; the CPU tier counts the fused launches of such a plan in test_graph_convolve_family)"""
    N, r2c, f32 = tuple(case["N"]), bool(case.get("r2c")), bool(case.get("f32"))
    ct = np.complex64 if f32 else np.complex128
    n = float(np.prod(N))
    fw = (lambda a: np.fft.rfftn(a, axes=(0, 1, 2))) if r2c else np.fft.fftn
    iv = (lambda a: np.fft.irfftn(a, s=N, axes=(0, 1, 2))) if r2c else np.fft.ifftn
    if half:
        hp = HW.problem(N, r2c)
        x, H = hp["xp"], hp["H"]
    else:
        x, H, _ = W.problem(N, r2c, case.get("cplx"))
    rng = np.random.default_rng(23)
    H2 = rng.standard_normal(H.shape) + (1j * rng.standard_normal(H.shape) if case.get("cplx") else 0.0)
    x2 = rng.standard_normal(N) if r2c else rng.standard_normal(N) + 1j * rng.standard_normal(N)
    S = fw(x2)
    fk = api.FILTER_COMPLEX if case.get("cplx") else api.FILTER_REAL

    def plan():
        po = HW.make_plan(api, case)
        for o, v in opts:
            assert api.lib().offt_hip_set_option(po, o, v) == 0
        if half:
            api.offt_hip_set_half_box(po, True)
        api.lib().offt_hip_set_output_scale(po, W.SCALE)
        return po

    def bufs(po):
        c, ne = api.comm_dict(po), api.local_elems(po)
        d1, f1 = W.local_arrays(c, ne, case, x, H)
        d2, f2 = W.local_arrays(c, ne, case, x2, H2)
        if half:
            d1 = HW.poisoned_input(c, ne, case, x)
        const = {"f1": f1, "f2": f2}
        if call_name in ("convolve", "forward_filtered", "half_forward"):
            return {"a": d1}, const
        if call_name == "convolve_multi":
            return {"a": d1, "b": np.zeros_like(d1)}, const
        if call_name == "convolve_sum":
            return {"a": d1, "b": d2}, const
        spec = np.zeros(ne, dtype=ct)
        spec[W.out_index(c)] = HW.out_block(c, S).astype(ct)
        return {"a": spec, "b": np.zeros_like(spec)}, const   # inverse_filtered: output 0 in place of the spectrum, output 1 apart

    def call(po, p):
        if call_name == "convolve":
            api.offt_hip_execute_convolve(po, p["a"], p["f1"], fk)
        elif call_name == "convolve_multi":
            api.offt_hip_execute_convolve_multi(po, p["a"], [p["a"], p["b"]], [p["f1"], p["f2"]], fk)
        elif call_name == "convolve_sum":
            api.offt_hip_execute_convolve_sum(po, [p["a"], p["b"]], [p["f1"], p["f2"]], p["a"], fk)
        elif call_name == "forward_filtered":
            api.offt_hip_execute_forward_filtered(po, p["a"], p["f1"], fk)
        elif call_name == "inverse_filtered":
            api.offt_hip_execute_inverse_filtered(po, p["a"], [p["b"], p["a"]], [p["f2"], p["f1"]], fk)
        else:
            api.offt_3d_execute_dir(po, p["a"], p["a"], -1)

    def check(po, outs):
        c = api.comm_dict(po)
        tol = HW.tol(case) if half else W.tol(case)
        if call_name == "convolve":
            want = iv(H * fw(x)) * n * W.SCALE
            err = HW.box_err(c, case, outs["a"], want) if half else W.check(c, case, outs["a"], want)
        elif call_name == "convolve_multi":
            err = max(W.check(c, case, outs["a"], iv(H * fw(x)) * n * W.SCALE), W.check(c, case, outs["b"], iv(H2 * fw(x)) * n * W.SCALE))
        elif call_name == "convolve_sum":
            err = W.check(c, case, outs["a"], iv(H * fw(x) + H2 * fw(x2)) * n * W.SCALE)
        elif call_name == "forward_filtered":
            err = SW.out_err(c, outs["a"], W.SCALE * H * fw(x))
        elif call_name == "inverse_filtered":
            err = max(W.check(c, case, outs["a"], iv(H * S) * n * W.SCALE), W.check(c, case, outs["b"], iv(H2 * S) * n * W.SCALE))
        else:
            err = SW.out_err(c, outs["a"], W.SCALE * fw(x))
        assert err <= tol, (name, err, tol)
        if fused is not None:
            q = dict(convolve=api.offt_hip_convolve_fused, convolve_multi=api.offt_hip_convolve_multi_fused,
                     convolve_sum=api.offt_hip_convolve_sum_fused, forward_filtered=api.offt_hip_spectral_fused,
                     inverse_filtered=api.offt_hip_spectral_fused)[call_name]
            assert q(po) == fused, (name, "route")
        if pruned is not None:
            assert api.offt_hip_half_box_pruned(po) == pruned, (name, "route")
        if groups is not None:
            p = po.contents
            planes = p.Nz // 2 + 1 if p.is_r2c else p.Nz
            per = int(api.lib().offt_hip_get_option(po, OPT_ZGROUP_MIB) / (p.Nx * p.Ny * (8 if f32 else 16) / 2.0 ** 20))
            assert 1 <= per < planes and -(-planes // per) == groups and planes % per, (name, per, planes)   # ragged last group
    return GCase(name, plan, bufs, call, check)


CONV_CALLS = ["convolve", "convolve_multi", "convolve_sum", "forward_filtered", "inverse_filtered"]


def _conv_gpu_cases():
    out = []
    for cn in CONV_CALLS:
        spec = cn.endswith("filtered")
        out.append(_conv_gcase(f"{cn}-fused", cn, dict(N=[64, 12, 10], cplx=1), [(api.OPT_SPEC_FUSED, 1)], fused=True))
        out.append(_conv_gcase(f"{cn}-generic", cn, dict(N=[48, 40, 30]), [(api.OPT_SPEC_FUSED, 0)], fused=False))
        if spec:   # the generic route of the filtered calls at a shape that has the fused one
            out.append(_conv_gcase(f"{cn}-fused-off", cn, dict(N=[64, 12, 10], cplx=1), [(api.OPT_SPEC_FUSED, 0)], fused=False))
        out.append(_conv_gcase(f"{cn}-r2c", cn, dict(N=[64, 12, 10], r2c=1), [(api.OPT_SPEC_FUSED, 1)], fused=True))
        # ((64, 32, 21) has planes of 32 KiB, one group: 128 x 128 planes as in case 2 give 6 groups of 4, 4, 4, 4, 4 and 1)
        out.append(_conv_gcase(f"{cn}-groups", cn, dict(N=[128, 128, 21]), [(api.OPT_SPEC_FUSED, 1), (OPT_ZGROUP_MIB, 1), (OPT_ZGROUP_STREAMS, 2)],
                               fused=True, groups=6))
    for N, pruned, nm in (([12, 10, 8], False, "clearing"), ([64, 64, 64], True, "pruned")):
        out.append(_conv_gcase(f"half-{nm}-forward", "half_forward", dict(N=N, cplx=1), half=True, pruned=pruned))
        out.append(_conv_gcase(f"half-{nm}-convolve", "convolve", dict(N=N, cplx=1), half=True, pruned=pruned))
    return out


GPU_CONV_CASES = {c.name: c for c in _conv_gpu_cases()}


@pytest_gpu
@pytest.mark.parametrize("name", [n for n in GPU_CONV_CASES])
def test_gpu_convolve_family_on_caller_stream(built, name):
    _protocol(GPU_CONV_CASES[name])


# ---- cases 5 (second half), 9, 10: several plans, several streams ---------------------------------------------------------------
@pytest_gpu
def test_gpu_two_long_plans_alternating_on_one_stream(built):
    """two plans of different long lengths share the caller stream's scratch (keyed by stream, grown to the larger need): called
    alternately, each result bit-identical to its synchronous twin"""
    torch = _torch()
    a, b = GPU_CASES["long-four-step"], GPU_CASES["long-scratch-lines"]
    refs = [_sync_twin(a), _sync_twin(b)]
    T = torch.cuda.Stream()
    runs = [_OnStream(a, T), _OnStream(b, T)]
    try:
        for r in runs:
            r.warm_up()
        D = _delay_ms("two-long-plans")
        for rnd in range(2):
            host, got = [], []
            for i, r in enumerate(runs):
                host.append(r.enqueue(D if i == 0 else 0))     # one delay holds T for the pair: nothing is waited for in between
            for r in runs:
                got.append(r.results())
            for i, r in enumerate(runs):
                _assert_same(r.case, D, sum(host), got[i], refs[i])
    finally:
        for r in runs:
            r.fin()


@pytest_gpu
@pytest.mark.parametrize("order", [("long-four-step", "long-scratch-lines"), ("long-scratch-lines", "long-four-step")])
def test_gpu_long_plan_regrows_scratch_behind_work_in_flight(built, order):
    """only the first plan has run on T; behind its call, held by the delay, comes the FIRST call of the other plan, whose
    longer lines make the stream's scratch grow (in one of the two orders): the old buffer is freed while the first plan's work
    that uses it is still in flight.  The launcher drains T before it frees -- the one intended host wait in asynchronous mode
    -- so that second call may take as long as the delay: its host time is not asserted, only the first call's."""
    torch = _torch()
    a, b = GPU_CASES[order[0]], GPU_CASES[order[1]]
    refs = [_sync_twin(a), _sync_twin(b)]
    T = torch.cuda.Stream()
    runs = [_OnStream(a, T), _OnStream(b, T)]
    try:
        runs[0].warm_up()
        D = _delay_ms("two-long-plans")
        host_a = runs[0].enqueue(D)
        runs[1].enqueue(0)
        got = [r.results() for r in runs]
        _assert_same(a, D, host_a, got[0], refs[0])
        _assert_same(b, D, 0.0, got[1], refs[1])
    finally:
        for r in runs:
            r.fin()


@pytest_gpu
def test_gpu_delays_are_five_times_the_enqueue_time(built):
    """the condition on D: at least 5 times the host's enqueue time of the call (plan's own stream, no delay), at most 1000 ms"""
    for name, case in {**GPU_CASES, **GPU_CONV_CASES}.items():
        ms = enqueue_ms(case)
        assert 5 * ms <= _delay_ms(name) <= 1000, (name, ms, "INCONCLUSIVE: the delay no longer covers the enqueue time")


@pytest_gpu
def test_gpu_two_live_plans_on_two_streams(built):
    """an f64 and an f32 plan of the same lengths (registries and tables are keyed by (n, precision)) on two caller streams,
    calls interleaved from the host, each stream with its own delay"""
    torch = _torch()
    cases = [GPU_CASES["groups-s2-f64-fwd"], _tx("two-plans-f32", (128, 128, 21), -1, f32=1, opts=[(OPT_ZGROUP_MIB, 1), (OPT_ZGROUP_STREAMS, 2)])]
    refs = [_sync_twin(c) for c in cases]
    runs = [_OnStream(c, torch.cuda.Stream()) for c in cases]
    try:
        for r in runs:
            r.warm_up()
        D = _delay_ms("two-live-plans")
        host = [0.0, 0.0]
        for rnd in range(2):
            for i, r in enumerate(runs):
                host[i] += r.enqueue(D if rnd == 0 else 0)
        got = [r.results() for r in runs]
        for i, r in enumerate(runs):
            _assert_same(r.case, D, sum(host), got[i], refs[i])
    finally:
        for r in runs:
            r.fin()


@pytest_gpu
def test_gpu_back_to_own_stream_and_to_the_caller_again(built):
    """offt_hip_set_stream(po, NULL) after a caller stream: a stream of the plan's own, the same bits; then T again"""
    torch = _torch()
    L = _glib()
    case = GPU_CASES["groups-s2-f64-fwd"]
    ref = _sync_twin(case)
    T = torch.cuda.Stream()
    run = _OnStream(case, T)
    try:
        run.warm_up()
        D = _delay_ms(case.name)
        _assert_same(case, D, run.enqueue(D), run.results(), ref)
        L.offt_hip_set_stream(run.po, None)                      # the plan's own stream: host syncs around, as the twin
        for k in run.data:
            run.data[k].copy_(run.staging[k])
        torch.cuda.synchronize()
        case.call(run.po, run.ptrs)
        assert L.offt_hip_wait(run.po) == 0
        torch.cuda.synchronize()
        for k in ref:
            assert np.array_equal(run.data[k].cpu().numpy().view(np.uint8), ref[k].view(np.uint8)), (k, "own stream")
            run.data[k].fill_(NAN)
        torch.cuda.synchronize()
        L.offt_hip_set_stream(run.po, T.cuda_stream)
        _assert_same(case, D, run.enqueue(D), run.results(), ref)
    finally:
        run.fin()
