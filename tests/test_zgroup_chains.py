"""CPU tier: the host path of the two-chain plane groups (OFFT_HIP_OPT_ZGROUP_CHAINS, execute_single).

With the option at 2 the pipelined y / x plane groups of the forward z-y-x transform run as two independent paired chains,
the even groups on the plan's stream and the odd groups on a second one:

    s      z | y(0) | {x(0), y(2)} | {x(2), y(4)} | ... | x(last even)
    s_aux       fork> y(1) | {x(1), y(3)} | {x(3), y(5)} | ... | x(last odd) >join

tests/cpu_backend_chains.c logs every launch and every stream operation with its stream, so the schedule is read off the
log; its replay mode queues the operations and runs them in the orders the event edges allow, which is how the fork and the
join are shown to be NEEDED: with either one ignored the result comes out wrong."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cpu_world
import oracle_lib as O
from offt_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PASS, PAIR, RECORD, WAIT, SYNC = range(5)
SCALE = 0.25


class Rec(C.Structure):  # cpu_backend_chains.c: crec
    _fields_ = [(n, C.c_int) for n in ("kind", "stream", "event", "n", "nb1", "n2", "nb1_2", "out_keep")] + \
               [("out_off", C.c_longlong), ("out_off2", C.c_longlong)]


@pytest.fixture(scope="module")
def world(built):
    subprocess.check_call(["make", "-s", "-C", ROOT, "tests/libcpubackend.so", "tests/libcpubackend_chains.so"])
    cpu_world.install(0, 1)  # (the library routing; the table is replaced below)
    CB = C.CDLL(os.path.join(ROOT, "tests", "libcpubackend_chains.so"))
    CB.cpu_backend_chains_table.restype = C.c_void_p
    CB.cpu_backend_chains_len.restype = C.c_long
    CB.cpu_backend_chains_flush.restype = C.c_long
    CB.cpu_backend_chains_reset.argtypes = [C.c_void_p, C.c_int, C.c_int]
    CB.cpu_backend_chains_copy_log.argtypes = [C.c_void_p]
    assert CB.cpu_backend_chains_rec_bytes() == C.sizeof(Rec)
    L = api.lib()
    L.offt_hip_test_set_backend(CB.cpu_backend_chains_table(), 0, 1)
    try:
        yield CB, L
    finally:
        cpu_world.uninstall()


def run(world, shape, planes, chains, policy=0, drop=-1, asyn=0, repeat=1, pipeline=1, set_chains=True):
    """one plan, `repeat` executes in place on the hash field: (the caller's array when the last wait returned, the log of the
    LAST execute, paired launches, chains, launches the replay had not run by then)"""
    CB, L = world
    po = api.offt_3d_init(*shape)
    try:
        assert L.offt_hip_set_option(po, api.OPT_ZGROUP_PLANES, planes) == 0
        assert L.offt_hip_set_option(po, api.OPT_ZGROUP_PIPELINE, pipeline) == 0
        if set_chains:
            assert L.offt_hip_set_option(po, api.OPT_ZGROUP_CHAINS, chains) == 0
            assert L.offt_hip_get_option(po, api.OPT_ZGROUP_CHAINS) == chains
        buf = np.zeros(api.local_elems(po), dtype=np.complex128)
        c = api.comm_dict(po)
        s0, s1, s2 = c["istride"]
        idx = (np.arange(shape[0])[:, None, None] * s0 + np.arange(shape[1])[None, :, None] * s1 + np.arange(shape[2])[None, None, :] * s2).ravel()
        buf[idx] = O.hash_field(*shape).ravel()
        L.offt_hip_set_output_scale(po, SCALE)
        L.offt_hip_set_async(po, asyn)
        left = 0
        for _ in range(repeat):
            CB.cpu_backend_chains_reset(buf.ctypes.data, policy, drop)
            api.offt_3d_execute(po, buf.ctypes.data, buf.ctypes.data)
            assert L.offt_hip_wait(po) == 0
            seen = buf.copy()  # what the caller finds when the wait has returned
            assert not CB.cpu_backend_chains_stuck()
            left = CB.cpu_backend_chains_flush()
        log = (Rec * CB.cpu_backend_chains_len())()
        CB.cpu_backend_chains_copy_log(log)
        o0, o1, o2 = c["ostride"]
        odx = np.arange(shape[0])[:, None, None] * o0 + np.arange(shape[1])[None, :, None] * o1 + np.arange(shape[2])[None, None, :] * o2
        return seen[odx], list(log), L.offt_hip_last_pipelined_launches(po), L.offt_hip_last_pipelined_chains(po), left
    finally:
        api.offt_3d_fin(po)


_want = {}


def numpy_fft(shape):
    if shape not in _want:
        _want[shape] = np.fft.fftn(O.hash_field(*shape)) * SCALE
    return _want[shape]


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def launches(log):
    return [r for r in log if r.kind in (PASS, PAIR)]


def check_two_chain_log(log, shape, planes):
    """the schedule of the docstring, read off the log"""
    nx, ny, nz = shape
    plane_bytes = nx * ny * 16
    groups = [min(planes, nz - z0) for z0 in range(0, nz, planes)]
    G = len(groups)
    ls = launches(log)
    zpass = ls[0]
    assert (zpass.kind, zpass.n, zpass.nb1) == (PASS, nz, nx)
    s_a = zpass.stream
    streams = {r.stream for r in ls}
    assert len(streams) == 2 and s_a in streams
    s_b = (streams - {s_a}).pop()
    # where every group's y and x ran: (position in the log, stream)
    ypos, xpos = {}, {}
    for i, r in enumerate(log):
        if r.kind not in (PASS, PAIR) or r is zpass:
            continue
        if r.kind == PAIR or r.n == ny and r.out_keep == 1:  # a y launch keeps its stores, alone or in a pair
            g, rem = divmod(r.out_off, planes * plane_bytes)
            assert rem == 0 and r.n == ny and r.nb1 == groups[g] and g not in ypos
            ypos[g] = (i, r.stream)
        if r.kind == PAIR:
            g, rem = divmod(r.out_off2, planes * plane_bytes)
            assert rem == 0 and r.n2 == nx and r.nb1_2 == groups[g] and g not in xpos
            xpos[g] = (i, r.stream)
        elif not (r.n == ny and r.out_keep == 1):
            g, rem = divmod(r.out_off, planes * plane_bytes)
            assert rem == 0 and r.n == nx and r.nb1 == groups[g] and g not in xpos
            xpos[g] = (i, r.stream)
    # every plane y-transformed once and x-transformed once; x of a group on its y's stream, and later
    assert sorted(ypos) == sorted(xpos) == list(range(G))
    for g in range(G):
        assert ypos[g][1] == xpos[g][1] == (s_a if g % 2 == 0 else s_b)
        assert xpos[g][0] > ypos[g][0]
    # per chain: y | pairs | x
    for s, mine in ((s_a, groups[0::2]), (s_b, groups[1::2])):
        kinds = [r.kind for r in ls if r.stream == s and r is not zpass]
        assert kinds == [PASS] + [PAIR] * (len(mine) - 1) + [PASS]
    # fork: a record on A behind the z pass and ahead of everything else, and B waits for that event before its first launch
    iz = log.index(zpass)
    first_b = min(i for i, r in enumerate(log) if r.kind in (PASS, PAIR) and r.stream == s_b)
    waits = [i for i, r in enumerate(log) if r.kind == WAIT]
    assert len(waits) == 2
    fork, join = waits
    assert log[fork].stream == s_b and fork < first_b
    rec = max(i for i in range(fork) if log[i].kind == RECORD and log[i].event == log[fork].event)
    assert log[rec].stream == s_a and iz < rec
    assert all(i > rec for i, r in enumerate(log) if r.kind in (PASS, PAIR) and r is not zpass)
    # join: a record on B behind its last launch, A waits for it, and nothing else is issued on A before that wait is
    last = max(i for i, r in enumerate(log) if r.kind in (PASS, PAIR))
    last_b = max(i for i, r in enumerate(log) if r.kind in (PASS, PAIR) and r.stream == s_b)
    assert log[join].stream == s_a and join > last
    rec = max(i for i in range(join) if log[i].kind == RECORD and log[i].event == log[join].event)
    assert log[rec].stream == s_b and rec > last_b
    # nothing behind the pair precedes the join: between A's last launch of the pair and the join, A gets no operation at all
    last_a = max(i for i, r in enumerate(log) if r.kind in (PASS, PAIR) and r.stream == s_a)
    assert [r.kind for r in log[last_a + 1:join] if r.stream == s_a] == []
    return G


# (shape, planes per group): 4, 5, 7 and 8 groups, and a short last group that falls into the odd chain (16 = 3 * 5 + 1: group 3;
# 24 = 4 * 5 + 4 would be group 4, even) and into the even one
CASES = [((16, 16, 16), 4), ((16, 16, 20), 4), ((16, 16, 28), 4), ((16, 16, 16), 2), ((16, 16, 16), 5), ((16, 16, 24), 5),
         ((32, 32, 14), 2), ((16, 16, 16), 1)]


@pytest.mark.parametrize("shape,planes", CASES)
def test_schedule_bits_and_numpy(world, shape, planes):
    one, log1, n1, c1, _ = run(world, shape, planes, 1)
    two, log2, n2, c2, left = run(world, shape, planes, 2)
    G = check_two_chain_log(log2, shape, planes)
    assert G >= 4 and c2 == 2 and c1 == 1 and left == 0
    assert n1 == G - 1 and n2 == G - 2  # paired launches: one chain, and the two chains together
    assert np.array_equal(two, one)
    assert rel(two, numpy_fft(shape)) < 1e-13


@pytest.mark.parametrize("shape,planes", [((16, 16, 16), 16), ((16, 16, 16), 8), ((16, 16, 16), 6)])
def test_fewer_than_four_groups_run_as_one_chain(world, shape, planes):
    one, log1, n1, c1, _ = run(world, shape, planes, 1)
    two, log2, n2, c2, _ = run(world, shape, planes, 2)
    def keys(log):  # streams relative to the plan's; the z pass stores into the plan's scratch volume: no offset for it
        zpass = launches(log)[0]
        return [(r.kind, r.stream - log[0].stream, r.n, r.nb1, r.n2, r.nb1_2, r.out_keep, 0 if r is zpass else r.out_off, r.out_off2) for r in log]
    assert keys(log2) == keys(log1)
    assert c2 == 1 and n2 == n1 and not any(r.kind == WAIT for r in log2)
    assert np.array_equal(two, one)


@pytest.mark.parametrize("shape,planes", [((16, 16, 16), 4), ((16, 16, 16), 5), ((32, 16, 24), 5)])
def test_one_chain_is_the_launch_list_it_was(world, shape, planes):
    """with the option at 1 -- or never touched, on a test table, whose plans take two chains only once it is SET -- the log is  z | y(0) | {x(g-1), y(g)} ... | x(G-1)  on one stream,
    with no stream operation beyond the timing records"""
    nx, ny, nz = shape
    groups = [min(planes, nz - z0) for z0 in range(0, nz, planes)]
    want = [(PASS, nz, nx, 0, 0), (PASS, ny, groups[0], 0, 0)] + [(PAIR, ny, groups[g], nx, groups[g - 1]) for g in range(1, len(groups))] + \
           [(PASS, nx, groups[-1], 0, 0)]
    logs = []
    for set_chains in (True, False):
        got, log, n, c, _ = run(world, shape, planes, 1, set_chains=set_chains)
        ls = launches(log)
        assert [(r.kind, r.n, r.nb1, r.n2, r.nb1_2) for r in ls] == want
        assert len({r.stream for r in log}) == 1 and not any(r.kind == WAIT for r in log)
        assert n == len(groups) - 1 and c == 1
        plane_bytes = nx * ny * 16
        assert [r.out_off for r in ls[1:-1]] == [z0 * plane_bytes for z0 in range(0, nz, planes)]
        assert [r.out_off2 for r in ls[2:-1]] == [z0 * plane_bytes for z0 in range(0, nz - planes, planes)]
        assert rel(got, numpy_fft(shape)) < 1e-13
        logs.append([(r.kind, r.stream - log[0].stream, r.n, r.nb1, 0 if r is ls[0] else r.out_off) for r in log])
    assert logs[0] == logs[1]


def test_not_pipelined_means_no_chains(world):
    got, log, n, c, _ = run(world, (16, 16, 16), 4, 2, pipeline=0)
    assert n == 0 and c == 0 and len({r.stream for r in log}) == 1 and all(r.kind != PAIR for r in log)
    assert rel(got, numpy_fft((16, 16, 16))) < 1e-13


def test_option_values(world):
    CB, L = world
    po = api.offt_3d_init(16, 16, 16)
    try:
        assert L.offt_hip_get_option(po, api.OPT_ZGROUP_CHAINS) == 2  # the default (which a test table's plans do not follow, see below)
        for bad in (0, 3, -1):
            assert L.offt_hip_set_option(po, api.OPT_ZGROUP_CHAINS, bad) == -1
        assert L.offt_hip_get_option(po, api.OPT_ZGROUP_CHAINS) == 2
        assert L.offt_hip_set_option(po, api.OPT_ZGROUP_CHAINS, 1) == 0 and L.offt_hip_get_option(po, api.OPT_ZGROUP_CHAINS) == 1
    finally:
        api.offt_3d_fin(po)


def test_environment_default(world, monkeypatch):
    CB, L = world
    for value in ("1", "2"):
        monkeypatch.setenv("OFFT_ZGROUP_CHAINS", value)
        po = api.offt_3d_init(16, 16, 16)
        try:
            assert L.offt_hip_get_option(po, api.OPT_ZGROUP_CHAINS) == int(value)
        finally:
            api.offt_3d_fin(po)


def test_group_size_halves_unless_fixed(world):
    """nobody fixed the group size: the library's rule (256 MiB: all 16 planes of 16^3) is ONE group and half of it two --
    fewer than 4, so the plan runs one chain at the full size"""
    CB, L = world
    po = api.offt_3d_init(16, 16, 16)
    try:
        L.offt_hip_set_option(po, api.OPT_ZGROUP_PIPELINE, 1)
        L.offt_hip_set_option(po, api.OPT_ZGROUP_CHAINS, 2)
        buf = np.zeros(api.local_elems(po), dtype=np.complex128)
        CB.cpu_backend_chains_reset(buf.ctypes.data, 0, -1)
        api.offt_3d_execute(po, buf.ctypes.data, buf.ctypes.data)
        assert L.offt_hip_last_pipelined_chains(po) == 1 and L.offt_hip_last_pipelined_launches(po) == 0
    finally:
        api.offt_3d_fin(po)


@pytest.mark.parametrize("asyn", [0, 1])
def test_async_and_repeated_executes(world, asyn):
    ref, _, _, _, _ = run(world, (16, 16, 16), 3, 1, repeat=3)
    got, log, n, c, left = run(world, (16, 16, 16), 3, 2, asyn=asyn, repeat=3)
    assert check_two_chain_log(log, (16, 16, 16), 3) == 6 and n == 4 and c == 2 and left == 0
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("policy", [1, 2])
@pytest.mark.parametrize("shape,planes", [((16, 16, 16), 4), ((16, 16, 16), 5), ((16, 16, 28), 4)])
def test_replay_with_both_edges_is_right_in_every_order(world, shape, planes, policy):
    want, _, _, _, _ = run(world, shape, planes, 1)
    got, log, n, c, left = run(world, shape, planes, 2, policy=policy)
    assert c == 2 and left == 0
    assert np.array_equal(got, want)


@pytest.mark.parametrize("shape,planes", [((16, 16, 16), 4), ((16, 16, 16), 5)])
def test_negative_control_fork_and_join_are_needed(world, shape, planes):
    """host-side negative control: the replay ignores one wait.  Without the fork the second chain may run ahead of the z pass
    (eager order); without the join the caller may read before the second chain has run (lazy order)."""
    want, _, _, _, _ = run(world, shape, planes, 1)
    no_fork, log, _, c, _ = run(world, shape, planes, 2, policy=2, drop=0)
    assert c == 2 and [r.kind for r in log].count(WAIT) == 2
    assert rel(no_fork, want) > 1e-3
    no_join, log, _, c, left = run(world, shape, planes, 2, policy=1, drop=1)
    assert c == 2 and left > 0  # launches of the second chain nobody waited for
    assert rel(no_join, want) > 1e-3
    # the same orders with the edge in place: right (the control is about the edge, not about the order)
    for policy in (1, 2):
        ok, _, _, _, left = run(world, shape, planes, 2, policy=policy)
        assert left == 0 and np.array_equal(ok, want)


def test_a_shorter_backend_table_keeps_working(world):
    """a table written before pass_pair existed (the first 23 entries; the rest NULL) installed in place of the logging one: the
    plan runs plain alternating launches whatever OFFT_HIP_OPT_ZGROUP_CHAINS says, and the entry is never read"""
    CB, L = world
    nptr = 23
    full = (C.c_void_p * 64).from_address(CB.cpu_backend_chains_table())
    short = (C.c_void_p * 64)()
    for i in range(nptr):
        short[i] = full[i]
    L.offt_hip_test_set_backend(C.cast(short, C.c_void_p), 0, 1)
    try:
        po = api.offt_3d_init(16, 16, 16)
        try:
            L.offt_hip_set_option(po, api.OPT_ZGROUP_PLANES, 4)
            L.offt_hip_set_option(po, api.OPT_ZGROUP_CHAINS, 2)
            buf = np.zeros(api.local_elems(po), dtype=np.complex128)
            CB.cpu_backend_chains_reset(buf.ctypes.data, 0, -1)
            api.offt_3d_execute(po, buf.ctypes.data, buf.ctypes.data)
            assert L.offt_hip_last_pipelined_chains(po) == 0 and L.offt_hip_last_pipelined_launches(po) == 0
            log = (Rec * CB.cpu_backend_chains_len())()
            CB.cpu_backend_chains_copy_log(log)
            assert [r.kind for r in launches(log)] == [PASS] * 9
        finally:
            api.offt_3d_fin(po)
    finally:
        L.offt_hip_test_set_backend(CB.cpu_backend_chains_table(), 0, 1)
