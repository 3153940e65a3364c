"""Shell-binned power and cross spectra of a stored spectrum: offt_hip_spectrum_shells.

  * the host call on the CPU backend of tests/cpu_backend_shells.c: complex and r2c plans (even and odd Nz), the three output
    layouts, kmul, nbins of 1, 5, max + 1 and 4096, gloo worlds of 2 and 3 ranks (one with an empty block), refusals, an
    older backend table, b == a, a and b untouched;
  * -m gpu: the kernels through the API (short rows, many workgroups, the pair rows of single precision, r2c weights, the
    three stride orders, kmul, nbins), the launcher on the blocks of multi-rank plans, bit-for-bit repeats on the plan's and
    on a caller's stream, a forward followed by the call.

The reference is numpy (np.bincount over the full spectrum, _shells_world.reference).  Integer spectra (|re|, |im| <= 8) must
match EXACTLY; random spectra to |sums - ref| <= 2 (counts + 4) 2^-52 sum w |A| |B| per bin, twice the standard bound for
summing n terms in double.  There is no other tolerance; the end-to-end test adds the forward's own parity tolerance
(tests/test_gpu_parity.py: max-abs / max <= 1e-12) carried through |A|^2."""
import ctypes as C
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import _half_world as HW
import _shells_world as S
from offt_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAIL = 99999999.0


# ---- CPU tier ---------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def shells_cpu(built):
    import cpu_world
    subprocess.check_call(["make", "-s", "-C", ROOT, "tests/libcpubackend_shells.so"])
    orig = cpu_world._cb_lib
    cpu_world._cb_lib = S.shells_cb_lib
    CB = cpu_world.install(0, 1, p1=1)
    yield CB
    cpu_world.uninstall()
    cpu_world._cb_lib = orig


def _run(case, dev, **kw):
    po = HW.make_plan(api, case)
    try:
        A, B = S.spectra(case)
        B = B if case.get("cross") else None
        sums, cnt, same = S.call(api, po, case, dev, A, B, **kw)
        assert same, (case, "a or b was written")
        S.check(case, sums, cnt, A, B)
        t = (C.c_double * 3)(1, 1, 1)
        api.lib().offt_hip_last_pass_seconds(po, t)
        assert list(t) == [0.0, 0.0, 0.0]
        return sums, cnt
    finally:
        api.offt_3d_fin(po)


CPU_CASES = [dict(N=[10, 9, 7]), dict(N=[8, 8, 8], cross=1), dict(N=[10, 9, 7], r2c=1), dict(N=[12, 10, 8], r2c=1, cross=1),
             dict(N=[8, 6, 10], params={"S": 1}), dict(N=[8, 6, 9], params={"S": 1}, r2c=1), dict(N=[8, 8, 6], eq=1),
             dict(N=[8, 8, 6], eq=1, r2c=1, cross=1), dict(N=[16, 8, 8], kmul=[1, 2, 2]), dict(N=[16, 8, 8], kmul=[1, 2, 2], r2c=1),
             dict(N=[10, 9, 7], f32=1, cross=1), dict(N=[12, 10, 8], f32=1, r2c=1)]


@pytest.mark.parametrize("data", ["int", "rand"])
@pytest.mark.parametrize("case", CPU_CASES, ids=lambda c: json.dumps(c, separators=(",", ":")))
def test_shells_cpu(shells_cpu, case, data):
    n0 = shells_cpu.cpu_backend_shells_calls()
    sums, cnt = _run(dict(case, data=data), HW.Host())
    assert shells_cpu.cpu_backend_shells_calls() == n0 + 1
    assert cnt.sum() == np.prod(case["N"])   # nbins covers every shell


@pytest.mark.parametrize("r2c", [0, 1])
@pytest.mark.parametrize("nbins", [1, 5, "max+1", 4096])
def test_shells_nbins_cpu(shells_cpu, nbins, r2c):
    N = [10, 9, 7]
    top = S.max_shell(N)
    nb = top + 1 if nbins == "max+1" else nbins
    for data in ("int", "rand"):
        sums, cnt = _run(dict(N=N, r2c=r2c, nbins=nb, data=data, cross=1), HW.Host())
        assert len(sums) == nb
        if nb > top:
            assert cnt.sum() == np.prod(N) and not sums[top + 1:].any() and not cnt[top + 1:].any()
        else:
            assert cnt.sum() < np.prod(N)   # modes dropped


def test_shells_without_counts_and_b_equal_a_cpu(shells_cpu):
    case = dict(N=[10, 9, 7], r2c=1, data="rand")
    po = HW.make_plan(api, case)
    try:
        A, _ = S.spectra(case)
        auto, cnt, _ = S.call(api, po, case, HW.Host(), A)
        none, nocnt, _ = S.call(api, po, case, HW.Host(), A, counts=False)
        assert nocnt is None and np.array_equal(auto.view(np.uint64), none.view(np.uint64))
        # b == a: the same pointer, the same bits as b == NULL
        c, ne = api.comm_dict(po), api.local_elems(po)
        a = S.local_buffer(c, ne, A)
        sums = np.full(len(auto), S.POISON)
        api.offt_hip_spectrum_shells(po, a.ctypes.data, a.ctypes.data, len(sums), sums.ctypes.data, None)
        assert np.array_equal(sums.view(np.uint64), auto.view(np.uint64))
    finally:
        api.offt_3d_fin(po)


def _gloo(size, cases, tmp_path):
    subprocess.check_call(["make", "-s", "-C", ROOT, "tests/libcpubackend_shells.so"])
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    procs = []
    for r in range(size):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(size), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_shells_world.py"), "gloo", json.dumps(cases),
                                       str(tmp_path)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = [p.communicate(timeout=600)[0].decode() for p in procs]
    for r, p in enumerate(procs):
        assert p.returncode == 0, f"rank {r}:\n{outs[r][-3000:]}"
    return [json.load(open(tmp_path / f"shells_rank{r}.json")) for r in range(size)]


def _world(shells_cpu, size, cases, tmp_path, want_empty=()):
    ranks = _gloo(size, cases, tmp_path)
    empties = []
    for i, case in enumerate(cases):
        recs = [ranks[r][i] for r in range(size)]
        assert all(rec["intact"] for rec in recs)
        sums = np.sum([np.array(rec["sums"]) for rec in recs], axis=0)
        cnt = np.sum([np.array(rec["counts"], dtype=np.int64) for rec in recs], axis=0)
        A, B = S.spectra(case)
        B = B if case.get("cross") else None
        # against the one-rank result of the library and against numpy: exactly for integer data, to the bound for random data
        po = HW.make_plan(api, {k: v for k, v in case.items() if k != "params"})
        try:
            one, onecnt, _ = S.call(api, po, case, HW.Host(), A, B)
        finally:
            api.offt_3d_fin(po)
        assert np.array_equal(cnt, onecnt) and cnt.sum() == np.prod(case["N"])
        S.check(case, sums, cnt, A, B)
        if case["data"] == "int":
            assert np.array_equal(sums, one)
        else:
            _, rc, rw = S.reference(A, A if B is None else B, tuple(case["N"]), bool(case.get("r2c")), case.get("kmul"), len(sums))
            assert np.all(np.abs(sums - one) <= S.bound(rc, rw))
        empty = [r for r, rec in enumerate(recs) if 0 in rec["osize"]]
        for r in empty:   # an empty block: zeros
            assert not np.array(recs[r]["sums"]).any() and not np.array(recs[r]["counts"]).any()
        empties.append(bool(empty))
    for i in want_empty:
        assert empties[i], (cases[i], "no rank's block is empty")


WORLD = [dict(N=[10, 9, 7], r2c=1, data="int"), dict(N=[10, 9, 7], r2c=1, data="rand", cross=1),
         dict(N=[12, 10, 8], r2c=1, data="int", cross=1), dict(N=[12, 10, 8], r2c=1, data="rand")]


def test_shells_gloo_world2(shells_cpu, tmp_path):
    _world(shells_cpu, 2, WORLD + [dict(N=[12, 10, 8], r2c=1, data="int", params={"P1": 2})], tmp_path)


def test_shells_gloo_world3(shells_cpu, tmp_path):
    """... and [8, 6, 2] r2c: two planes of the half spectrum over three ranks, so that one rank's block is empty"""
    empty = dict(N=[8, 6, 2], r2c=1, data="int", cross=1)
    # beforehand, on one process: a rank of that world of 3 really has an empty block
    import cpu_world
    sizes = []
    for r in range(3):
        cpu_world.install(r, 3)
        po = HW.make_plan(api, empty)
        sizes.append(api.comm_dict(po)["osize"])
        api.offt_3d_fin(po)
    cpu_world.install(0, 1, p1=1)
    assert any(0 in o for o in sizes), sizes
    _world(shells_cpu, 3, WORLD + [empty, dict(N=[10, 9, 7], r2c=1, data="rand", params={"P1": 3})], tmp_path, want_empty=(4,))


# ---- refusals: -1, the marker, the text, nothing launched, sums untouched ----------------------------------------------------
def _refused(L, po, CB, args, word, sums):
    import _spec_world as SW
    n0, c0 = (CB.cpu_backend_shells_calls(), SW.counts(CB)) if CB is not None else (None, None)
    before = sums.copy() if sums is not None else None
    assert L.offt_hip_spectrum_shells(po, *args) == -1
    assert po.contents.t[api.ALL] >= FAIL
    assert word in L.offt_hip_last_error().decode(), L.offt_hip_last_error().decode()
    if CB is not None:
        assert CB.cpu_backend_shells_calls() == n0 and SW.counts(CB) == c0
    if sums is not None:
        assert np.array_equal(sums, before)


def test_shells_refusals_cpu(shells_cpu):
    L = api.lib()
    po = api.offt_3d_init(10, 9, 7)
    try:
        ne = api.local_elems(po)
        a, sums, cnt = np.ones(ne, dtype=np.complex128), np.full(8, S.POISON), np.zeros(8, dtype=np.int64)
        A, SU, CN = a.ctypes.data, sums.ctypes.data, cnt.ctypes.data
        km = lambda *v: (C.c_int * 3)(*v)
        for args, word in (((None, None, None, 8, SU, CN), "the spectrum must be device memory (got NULL)"),
                           ((A, None, None, 8, None, CN), "sums must be device memory (got NULL)"),
                           ((A, None, None, 0, SU, CN), "nbins = 0"),
                           ((A, None, None, -3, SU, CN), "nbins = -3"),
                           ((A, None, None, api.SHELLS_MAX_BINS + 1, SU, CN), "nbins = 4097"),
                           ((A, A, km(1, 0, 1), 8, SU, CN), "kmul[1] = 0"),
                           ((A, None, km(1, 1, -2), 8, SU, CN), "kmul[2] = -2")):
            _refused(L, po, shells_cpu, args, word, sums)
        assert L.offt_hip_spectrum_shells(po, A, None, None, 8, SU, CN) == 0 and po.contents.t[api.ALL] < FAIL
        assert sums[0] == 1.0 and cnt[0] == 1
    finally:
        api.offt_3d_fin(po)


def test_shells_older_backend_table_is_refused_cpu(shells_cpu):
    """the table of tests/libcpubackend_spec.so (built before the entry existed in it): refused, nothing launched"""
    import cpu_world
    import _spec_world as SW
    subprocess.check_call(["make", "-s", "-C", ROOT, "tests/libcpubackend_spec.so"])
    cpu_world._cb_lib = SW.spec_cb_lib
    CB = cpu_world.install(0, 1, p1=1)
    L = api.lib()
    po = api.offt_3d_init(10, 9, 7)
    try:
        ne = api.local_elems(po)
        a, sums = np.ones(ne, dtype=np.complex128), np.full(8, S.POISON)
        c0 = SW.counts(CB)
        assert L.offt_hip_spectrum_shells(po, a.ctypes.data, None, None, 8, sums.ctypes.data, None) == -1
        assert po.contents.t[api.ALL] >= FAIL and "this backend has no shell-binned spectrum" in L.offt_hip_last_error().decode()
        assert SW.counts(CB) == c0 and np.all(sums == S.POISON)
    finally:
        api.offt_3d_fin(po)


# ---- GPU tier ---------------------------------------------------------------------------------------------------------------
def _gpu():
    import torch
    torch.cuda.set_device(0)
    return HW.Gpu(torch)


GPU_CASES = [dict(N=[16, 12, 20]),                       # rows shorter than a wave: several rows and run boundaries per wave
             dict(N=[64, 64, 64]), dict(N=[64, 64, 64], f32=1),   # many workgroups, the pair rows (f32), the combine
             dict(N=[32, 32, 32], r2c=1), dict(N=[16, 16, 15], r2c=1, f32=1),   # the weights, even and odd Nz
             dict(N=[32, 32, 32], params={"S": 1}), dict(N=[32, 32, 32], eq=1),   # the other two stride orders
             dict(N=[32, 32, 32], params={"S": 1}, r2c=1), dict(N=[64, 32, 32], kmul=[1, 2, 2]),
             dict(N=[32, 32, 32], nbins=1), dict(N=[32, 32, 32], nbins=5), dict(N=[32, 32, 32], nbins=4096)]


@pytest.mark.gpu
@pytest.mark.parametrize("data", ["int", "rand"])
@pytest.mark.parametrize("case", GPU_CASES, ids=lambda c: json.dumps(c, separators=(",", ":")))
def test_shells_gpu(built, case, data):
    sums, cnt = _run(dict(case, data=data), _gpu())
    if not case.get("nbins") or case["nbins"] == 4096:
        assert cnt.sum() == np.prod(case["N"])
    if case.get("nbins") == 4096:
        top = S.max_shell(case["N"])
        assert not sums[top + 1:].any() and not cnt[top + 1:].any()


@pytest.mark.gpu
@pytest.mark.parametrize("f32", [0, 1])
@pytest.mark.parametrize("data", ["int", "rand"])
def test_shells_cross_rolled_gpu(built, f32, data):
    """64^3: the cross spectrum of a with a rolled by one plane; and without counts"""
    case = dict(N=[64, 64, 64], f32=f32, data=data)
    po = HW.make_plan(api, case)
    try:
        A, _ = S.spectra(case)
        B = np.roll(A, 1, axis=0)
        sums, cnt, same = S.call(api, po, case, _gpu(), A, B)
        assert same
        S.check(case, sums, cnt, A, B)
        none, nocnt, _ = S.call(api, po, case, _gpu(), A, B, counts=False)
        assert nocnt is None and np.array_equal(none.view(np.uint64), sums.view(np.uint64))
    finally:
        api.offt_3d_fin(po)


def _blk(r, n, p):
    F, b = n // p, n % p
    return ((r * F) if r < p - b else (p - b) * F + (r - (p - b)) * (F + 1)), (F if r < p - b else F + 1)


def _rank_geometry(N, r2c, p1, p2, rank):
    """ostart / osize / ostride (z-y-x) and the local elements of `rank` in a p1 x p2 world: comm_build of offt_host.c"""
    Nx, Ny, Nzn = N[0], N[1], N[2] // 2 + 1 if r2c else N[2]
    rx, ry = rank // p2, rank % p2
    M1, M2, M3, M4 = -(-Nx // p1), -(-Ny // p2), -(-Nzn // p2), -(-Ny // p1)
    (s1, m4), (s2, m3) = _blk(rx, Ny, p1), _blk(ry, Nzn, p2)
    ne = M1 * M2 * M3 * p2 if M2 * p2 > M4 * p1 else M1 * M3 * M4 * p1
    return dict(ostart=[0, s1, s2], osize=[Nx, m4, m3], ostride=[1, M1 * p1, M1 * p1 * M4]), ne


@pytest.mark.gpu
@pytest.mark.parametrize("r2c,p1,p2", [(1, 1, 3), (1, 3, 1), (0, 1, 3), (1, 1, 5)])
@pytest.mark.parametrize("data", ["int", "rand"])
def test_shells_launcher_on_rank_blocks_gpu(built, r2c, p1, p2, data):
    """offt_hipk_spectrum_shells on the start, size and padded strides of every rank's block of a 10 x 9 x 7 plan on p1 x p2
    ranks (1 x 5 on the four planes of the half spectrum: the last block is empty): the arrays add up to the one-rank answer"""
    import torch
    dev = _gpu()
    L = api.lib()
    I3, LL3, V = C.c_int * 3, C.c_longlong * 3, C.c_void_p
    L.offt_hipk_spectrum_shells.argtypes = [V, V, C.c_int, C.c_int, I3, LL3, I3, I3, V, C.c_int, V, V, V, C.c_longlong, V]
    L.offt_hipk_spectrum_shells_partials.restype = C.c_longlong
    L.offt_hipk_spectrum_shells_partials.argtypes = [C.c_int, I3, I3, V, C.c_int]
    L.offt_hipk_last_error.restype = C.c_char_p
    case = dict(N=[10, 9, 7], r2c=r2c, data=data)
    N, nb = case["N"], S.nbins_of(case)
    A, B = S.spectra(case)
    tot, totc, empty = np.zeros(nb), np.zeros(nb, dtype=np.int64), 0
    for rank in range(p1 * p2):
        c, ne = _rank_geometry(N, r2c, p1, p2, rank)
        empty += 0 in c["osize"]
        (ha, pa), (hb, pb) = dev.put(S.local_buffer(c, ne, A)), dev.put(S.local_buffer(c, ne, B))
        (hs, ps), (hc, pc) = dev.put(np.full(nb, S.POISON)), dev.put(np.full(nb, -3, dtype=np.int64))
        need = L.offt_hipk_spectrum_shells_partials(api.F64, I3(*c["osize"]), I3(*N), None, nb)
        assert (need == 0) == (0 in c["osize"])
        part = torch.empty(max(need, 8), dtype=torch.uint8, device="cuda")
        rc = L.offt_hipk_spectrum_shells(pa, pb, api.F64, r2c, I3(*c["osize"]), LL3(*c["ostride"]), I3(*c["ostart"]), I3(*N), None, nb,
                                         ps, pc, part.data_ptr(), need, None)
        assert rc == 0, L.offt_hipk_last_error().decode()
        sums, cnt = dev.get(hs, np.zeros(1)), dev.get(hc, np.zeros(1, dtype=np.int64))
        if 0 in c["osize"]:
            assert not sums.any() and not cnt.any()
        tot, totc = tot + sums, totc + cnt
    assert empty == (1 if p2 == 5 else 0)
    assert totc.sum() == np.prod(N)
    S.check(case, tot, totc, A, B)


@pytest.mark.gpu
def test_shells_repeat_bits_and_caller_stream_gpu(built):
    """64^3 f64 random: two calls give the same bits; so does a call in async mode on a caller-owned stream"""
    import torch
    dev = _gpu()
    case = dict(N=[64, 64, 64], data="rand")
    L = api.lib()
    po = HW.make_plan(api, case)
    try:
        A, B = S.spectra(case)
        c, ne = api.comm_dict(po), api.local_elems(po)
        nb = S.nbins_of(case)
        (ha, pa), (hb, pb) = dev.put(S.local_buffer(c, ne, A)), dev.put(S.local_buffer(c, ne, B))
        out = []
        for _ in range(2):
            hs, ps = dev.put(np.full(nb, S.POISON))
            api.offt_hip_spectrum_shells(po, pa, pb, nb, ps, None)
            assert L.offt_hip_last_device_seconds(po) > 0.0
            out.append(dev.get(hs, np.zeros(1)).view(np.uint64).copy())
        assert np.array_equal(out[0], out[1])
        stream = torch.cuda.Stream()
        L.offt_hip_set_stream(po, stream.cuda_stream)
        L.offt_hip_set_async(po, 1)
        hs, ps = dev.put(np.full(nb, S.POISON))
        api.offt_hip_spectrum_shells(po, pa, pb, nb, ps, None)
        stream.synchronize()
        assert np.array_equal(dev.get(hs, np.zeros(1)).view(np.uint64), out[0])
        L.offt_hip_set_async(po, 0)
        L.offt_hip_set_stream(po, None)
        sums = out[0].view(np.float64)
        S.check(case, sums, None, A, B)
    finally:
        api.offt_3d_fin(po)


@pytest.mark.gpu
@pytest.mark.parametrize("r2c", [0, 1])
def test_shells_after_a_forward_gpu(built, r2c):
    """a plan's forward of a seeded field at 32^3, then the call, against the numpy fftn binning: the summation bound plus
    the forward's parity tolerance d = 1e-12 max|A| per element, which moves |A|^2 by at most 2 |A| d + d^2"""
    import torch
    from gpu_util import make_input
    _gpu()
    N = (32, 32, 32)
    rng = np.random.default_rng(77)
    x = rng.standard_normal(N) + (0 if r2c else 1j * rng.standard_normal(N))
    po = api.offt_3d_init(*N, is_r2c=r2c)
    try:
        c = api.comm_dict(po)
        if r2c:
            buf = np.zeros(2 * api.local_elems(po))
            s0, s1, _ = c["istride"]
            idx = (np.arange(N[0])[:, None, None] * 2 * s0 + np.arange(N[1])[None, :, None] * 2 * s1 + np.arange(N[2])[None, None, :]).ravel()
            buf[idx] = x.ravel()
            dev = torch.from_numpy(buf).cuda()
        else:
            dev, _ = make_input(po, x)
        api.offt_3d_execute(po, dev.data_ptr(), dev.data_ptr())
        nb = S.max_shell(N) + 1
        sums = torch.full((nb,), S.POISON, dtype=torch.float64, device="cuda")
        cnt = torch.full((nb,), -3, dtype=torch.int64, device="cuda")
        api.offt_hip_spectrum_shells(po, dev.data_ptr(), None, nb, sums.data_ptr(), cnt.data_ptr())
        torch.cuda.synchronize()
        F = np.fft.fftn(x)
        s = S.shells(N).ravel()
        rs = np.bincount(s, weights=(np.abs(F) ** 2).ravel(), minlength=nb)
        rc = np.bincount(s, minlength=nb)
        d = 1e-12 * np.abs(F).max()
        lim = S.bound(rc, rs) + np.bincount(s, weights=(2 * np.abs(F) * d + d * d).ravel(), minlength=nb)
        assert np.array_equal(cnt.cpu().numpy(), rc)
        err = np.abs(sums.cpu().numpy() - rs)
        assert np.all(err <= lim), (np.flatnonzero(err > lim)[:8], err.max())
    finally:
        api.offt_3d_fin(po)


@pytest.mark.gpu
def test_shells_refusals_gpu(built):
    """host memory as a, b, sums, counts: each refused before anything is launched, then a good call"""
    import torch
    torch.cuda.set_device(0)
    L = api.lib()
    po = api.offt_3d_init(32, 32, 32)
    try:
        ne = api.local_elems(po)
        a = torch.ones(2 * ne, dtype=torch.float64, device="cuda")
        sums = torch.full((8,), S.POISON, dtype=torch.float64, device="cuda")
        cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
        host = np.zeros(2 * ne)
        A, SU, CN, HOST = a.data_ptr(), sums.data_ptr(), cnt.data_ptr(), host.ctypes.data
        for args, word in (((HOST, None, None, 8, SU, CN), "the spectrum must be device memory"),
                           ((None, None, None, 8, SU, CN), "the spectrum must be device memory (got NULL)"),
                           ((A, HOST, None, 8, SU, CN), "the second spectrum must be device memory"),
                           ((A, None, None, 8, HOST, CN), "sums must be device memory"),
                           ((A, None, None, 8, None, CN), "sums must be device memory (got NULL)"),
                           ((A, None, None, 8, SU, HOST), "counts must be device memory"),
                           ((A, None, None, 0, SU, CN), "nbins = 0"),
                           ((A, None, (C.c_int * 3)(1, 1, 0), 8, SU, CN), "kmul[2] = 0")):
            _refused(L, po, None, args, word, None)
            torch.cuda.synchronize()
            assert bool((sums == S.POISON).all())
        api.offt_hip_spectrum_shells(po, A, None, 8, SU, CN)
        assert float(sums[0]) == 2.0 and int(cnt[0]) == 1 and int(cnt[1]) == 18   # K2 = 1 and K2 = 2 both round to shell 1
    finally:
        api.offt_3d_fin(po)
