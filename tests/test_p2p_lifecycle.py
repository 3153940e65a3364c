"""The life cycle of the DIRECT-STORE exchange (OFFT_EXCHANGE=p2p) in the host code, on the CPU thread world
(tests/_thread_world.py ... cpu: ranks as threads on the descriptor interpreter, a pass of one rank really writes into
another rank's receive volume):

  1. the static sweep (max_loop > 0) rebuilds the exchange volumes point by point -- the peers' mappings, flag groups, slot
     counters and per-block tables have to follow every rebuild (offt_hip_test_p2p_consistent, offt_backend.h);
  2. a rank that cannot map a peer must not leave the collective steps of the mapping: all ranks fall back to the staged
     exchange together, once, and compute the right answer;
  3. a pass that fails on one rank makes that rank's plan fail fast from then on (its flag counters are out of step with
     its peers'), and the peer's wait for the flag that never comes ends in an error.

The same sweep cases run on real device memory in tests/test_gpu_world.py."""
import pytest

from test_p2p_world import run_cpu_thread_world

FAILED = 99999999.0  # the failure marker of an execute, t[ALL] (offt-compute.c:3881)

# the smallest grids that still retile: (ranks, case)
SWEEP_CASES = {
    "slab-8": (2, dict(N=[8, 8, 8], params=dict(P1=1), max_loop=6)),
    "pencil-8": (2, dict(N=[8, 8, 8], params=dict(P1=2), max_loop=6)),
    "slab-ragged": (2, dict(N=[10, 6, 9], params=dict(P1=1), max_loop=5, inv=2)),
    "pencil-T2-stage": (2, dict(N=[9, 7, 11], params=dict(P1=2), max_loop=9, repeat=2)),
    "four-ranks-mesh-then-tiling": (4, dict(N=[16, 16, 16], params=dict(), max_loop=7)),
    "slab-f32": (2, dict(N=[16, 8, 8], params=dict(P1=1), max_loop=4, f32=1)),
}


def executes_of(case):
    """how many executes _thread_world.py's cpu_rank makes for a case (one note each, after the one that follows init)"""
    n = 1 + case.get("repeat", 0)
    if case.get("inv"):
        n += (2 if case["inv"] == 2 else 1) + (1 if case.get("repeat") else 0)
    return n


@pytest.mark.parametrize("p2p", [0, 1], ids=["staged", "direct-store"])
@pytest.mark.parametrize("name", list(SWEEP_CASES))
def test_sweep_retiles_under_either_exchange(built, tmp_path, name, p2p):
    """every point of the sweep frees and reallocates R1 / the recv1 ring / recv2 and may change the ring: with the
    direct-store exchange the peers' mappings, tables, flags and slot counters are rebuilt with them, the exchange stays the
    direct-store one, and all ranks end on the same mesh and tiling; the staged exchange sweeps as before"""
    size, case = SWEEP_CASES[name]
    case = dict(case, p2p=p2p)
    (rec,) = run_cpu_thread_world(size, [case], tmp_path)  # exit status 0, rel_numpy / rel_oracle / rel_inverse below tol
    assert "rel_numpy" in rec and "rel_oracle" in rec and ("rel_inverse" in rec) == bool(case.get("inv"))
    ranks = rec["ranks"]
    assert len(ranks) == size
    for r in ranks:
        assert r["consistent"] == [1] * (1 + executes_of(case)), r
        assert r["exchange"] == [p2p] * (1 + executes_of(case)), r  # (1: the sweep did not drop to the staged exchange)
        assert r["mesh"] == ranks[0]["mesh"] and r["tiling"] == ranks[0]["tiling"], ranks
    assert ranks[0]["mesh"][0] * ranks[0]["mesh"][1] == size


# (ranks, params, the peer_open calls p2p_open makes on that mesh: two per exchange -- its flags, its receive volume)
MAP_RENDEZVOUS_S = 15
MAP_MESHES = {"1x2": (2, dict(P1=1), 2), "2x1": (2, dict(P1=2), 2), "2x2": (4, dict(), 4)}


@pytest.mark.parametrize("mesh,call", [(m, k) for m in MAP_MESHES for k in range(MAP_MESHES[m][2])])
def test_one_rank_cannot_map(built, tmp_path, mesh, call):
    """rank 1's k-th peer_open fails: it still takes part in every later collective step, the world agrees, and ALL ranks
    fall back to the staged exchange together.  Nobody may wait for a rank that left: a rendezvous of the world's ranks that
    runs out of time (MAP_RENDEZVOUS_S, far above what these worlds need and far below the subprocess time-out) ends the
    world with exit status 1, so ranks that lost step cannot meet again later and pass.  (After the LAST call of a mesh no
    collective step of the mapping follows: that case checks the fall-back alone.)"""
    size, params, _ = MAP_MESHES[mesh]
    out = []
    case = dict(N=[8, 8, 8], params=params, p2p=1, inv=1, fail_map=dict(rank=1, call=call), rendezvous_s=MAP_RENDEZVOUS_S)
    (rec,) = run_cpu_thread_world(size, [case], tmp_path, output=out)
    assert "rendezvous timed out" not in out[0], out[0][-2000:]
    if mesh == "2x2":
        assert rec["mesh"] == [2, 2]
    for r in rec["ranks"]:
        assert r["exchange"] == [0, 0, 0] and r["consistent"] == [1, 1, 1], r
    assert out[0].count("direct-store exchange not available here") == 1, out[0][-2000:]


def test_one_rank_cannot_map_during_a_sweep_retile(built, tmp_path):
    """... and when the mapping fails while the sweep rebuilds the volumes (calls 0 and 1 are the plan's own, 2 and 3 the first
    rebuild's): the world falls back together for the rest of the sweep and still computes the right answer"""
    out = []
    # (call 2, the flags of the first rebuild: the mapping of its R1 still follows, so a rank that left would be missed)
    case = dict(N=[8, 8, 8], params=dict(P1=1), p2p=1, max_loop=6, inv=1, fail_map=dict(rank=1, call=2), rendezvous_s=MAP_RENDEZVOUS_S)
    (rec,) = run_cpu_thread_world(2, [case], tmp_path, output=out)
    assert "rendezvous timed out" not in out[0], out[0][-2000:]
    for r in rec["ranks"]:
        assert r["exchange"] == [0, 0, 0] and r["consistent"] == [1, 1, 1], r
        assert r["tiling"] == rec["ranks"][0]["tiling"]
    assert out[0].count("direct-store exchange not available here") == 1, out[0][-2000:]


@pytest.mark.parametrize("p1", [1, 2], ids=["slab", "pencil"])
def test_failed_pass_is_sticky(built, tmp_path, p1):
    """rank 1's first pass of its first execute fails: that execute reports the failure marker, and so does the next one
    WITHOUT launching anything (epoch / use1 / tiles2 have advanced for signals that were never sent).  Rank 0 waits for a
    flag that never comes: an error after OFFT_P2P_TIMEOUT, not a hang, and its next execute fails at once as well."""
    (rec,) = run_cpu_thread_world(2, [dict(N=[8, 8, 8], params=dict(P1=p1), p2p=1, fail_pass=dict(rank=1, execute=0, **{"pass": 0}))], tmp_path,
                                  env=dict(OFFT_P2P_TIMEOUT="2"))
    r0, r1 = (r["executes"] for r in rec["ranks"])
    assert len(r0) == 2 and len(r1) == 2
    assert r1[0]["t_all"] == FAILED and r1[0]["launches"] >= 1, r1
    assert r1[1]["t_all"] == FAILED and r1[1]["launches"] == 0, r1
    assert "communicator failed earlier" in r1[1]["error"], r1
    assert r0[0]["t_all"] == FAILED and "a flag of the direct-store exchange did not arrive" in r0[0]["error"], r0
    assert r0[1]["t_all"] == FAILED and r0[1]["launches"] == 0, r0

