"""-m gpu: every environment switch of the kernel launcher (struct Env of offt_kernels.hip; the table of INTEGRATION.md)
against the CPU interpreter of pass descriptors.

The switches are read once per process, so each (group, setting) runs in a fresh child, tests/_launcher_env_child.py, one
at a time.  The child is told what setting to EXPECT (OFFT_TEST_EXPECT) separately from the switches themselves and asserts
with the library's device-free queries that the expected path is the one its descriptors resolve to before it launches
anything; it prints the SHA-256 of all its GPU outputs.  On top of "every child is green" the hashes are compared: a panel
order or a dispatch order of the paired kernel changes no arithmetic (order, pair: equal bits in every setting), plain
stores instead of cache-keeping ones neither (keep), an impossible OFFT_FOURSTEP_N1 leaves the default split, and the
default child of a group computes the bits of the same cases run inside this process.

A child that ends by a signal, with status 134 or 139 or at its time limit sets a flag, and every later case of this
module fails without starting anything on the card.

Time limits: a child takes an interpreter start-up plus at most a few seconds.  The hipRTC children compile at plan time;
one shape of the 260-point length took 3.3 s on an MI355X (the child prints it as "prepare(260)"), three shapes in one
program 7.8 s: their limit is the common one plus three times 7.8 s."""
import os
import subprocess
import sys

import pytest

import _launcher_env_child as child

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "_launcher_env_child.py")
LIMIT_S = 90          # start-up (importing torch on a cold cache dominates) plus the cases
RTC_EXTRA_S = 24      # 3 x 7.8 s, the measured plan-time compile of three shapes

# the any-length kernel is reached at 1001 single-precision and 4099 points only with the plan-time kernels and the long
# Bluestein net out of the way: every child of the mix group runs with these two as well
MIX_BASE = {"OFFT_RTC": "0", "OFFT_BLUESTEIN_LONG": "0"}

CASES = (
    [("order", {})] + [("order", {"OFFT_XCD_REMAP": v}) for v in ("0", "1", "8", "48", "256")] +
    [("pair", {})] + [("pair", {"OFFT_PAIR_RUN": v}) for v in ("8", "64", "4096")] + [("pair", {"OFFT_XCD_REMAP": "0"})] +
    [("keep", {}), ("keep", {"OFFT_KEEP_STORES": "0"})] +
    [("pairs32", {}), ("pairs32", {"OFFT_F32_PAIRS": "0"})] +
    [("blue", {}), ("blue", {"OFFT_BLUESTEIN": "0"}), ("blue", {"OFFT_R2C_BLUESTEIN": "0"}), ("blue", {"OFFT_BLUESTEIN_LONG_POW2": "1"})] +
    [("four", {})] + [("four", {"OFFT_FOURSTEP_N1": str(v)}) for v in child.FOUR_FORCED + (3,)] + [("four", {"OFFT_FOURSTEP": "0"})] +
    [("mix", {})] + [("mix", {"OFFT_MIX_THREADS": v}) for v in ("64", "256", "1024", "63")] +
    [("rtc", {}), ("rtc", {"OFFT_RTC": "0"}), ("rtc", {"OFFT_RTC_SHAPES": "3"})]
)


def key(group, switches):
    return group + "".join("-%s=%s" % kv for kv in sorted(switches.items()))


RESULTS = {}          # key -> (cases run, sha256)
FAULTED = []          # the key of the child that died, hung or aborted: nothing more is started after it


def run_child(group, switches, expect=None):
    """one child under `switches`, told to expect `expect` (default: the same) -> CompletedProcess"""
    assert not FAULTED, "not started: child %s ended by a signal, an abort or its time limit" % FAULTED[0]
    env = {k: v for k, v in os.environ.items() if k not in child.SWITCHES and k != "OFFT_BLUESTEIN_LONG"}
    env.update(MIX_BASE if group == "mix" else {})
    env.update(switches)
    env["OFFT_TEST_EXPECT"] = ",".join("%s=%s" % kv for kv in sorted((switches if expect is None else expect).items()))
    limit = LIMIT_S + (RTC_EXTRA_S if group == "rtc" else 0)
    try:
        r = subprocess.run([sys.executable, CHILD, group], env=env, timeout=limit, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    except subprocess.TimeoutExpired as e:
        FAULTED.append(key(group, switches))
        raise AssertionError("child %s hit its limit of %d s: %s" % (key(group, switches), limit, (e.stdout or "")[-3000:]))
    if r.returncode < 0 or r.returncode in (134, 139):
        FAULTED.append(key(group, switches))
    return r


@pytest.mark.parametrize("group,switches", CASES, ids=[key(g, s) for g, s in CASES])
def test_switch(group, switches):
    r = run_child(group, switches)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:])
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[:3] == ["SWITCH", "OK", group] and len(last) == 5, r.stdout[-3000:]
    RESULTS[key(group, switches)] = (int(last[3]), last[4])


def hashes(group):
    want = [key(g, s) for g, s in CASES if g == group]
    missing = [k for k in want if k not in RESULTS]
    assert not missing, "no result of %s (run the module whole: these compare what test_switch collected)" % missing
    return {k: RESULTS[k] for k in want}


@pytest.mark.parametrize("group", ["order", "pair"])
def test_equal_bits_in_every_setting(group):
    """a panel order and a dispatch order of the two roles change no arithmetic (48 is no power of two and runs as G = 32)"""
    h = hashes(group)
    assert len(set(h.values())) == 1, h


def test_keep_twins_compute_the_plain_kernels_bits():
    """OFFT_KEEP_STORES=0 against the default child of the same cases: a store's cache policy is no arithmetic.  (It once
    was: with a struct store in gstore_p<KEEP> the single-precision 256- and 1024-point twins were compiled to other
    packed-math and contraction choices than the plain kernels -- 17735 of 56854 and 132526 of 239630 elements differed in
    the last place, at most 1.1e-7 of max|want|, both kernels 1.6e-7 from the interpreter.  Both forms now store a vector.)"""
    h = hashes("keep")
    assert len(set(h.values())) == 1, h


def test_impossible_first_factor_leaves_the_default_split():
    h = hashes("four")
    assert h["four-OFFT_FOURSTEP_N1=3"] == h["four"], h
    assert h["four-OFFT_FOURSTEP_N1=64"] != h["four-OFFT_FOURSTEP_N1=2"], h   # (a forced factor is another computation)


def test_out_of_range_workgroup_size_is_ignored():
    """(the any-length kernel's workgroup size does not change the order of its additions either: every output is one
    thread's sum -- but that is not promised, so the sizes in range are held to the tolerance only)"""
    h = hashes("mix")
    assert h["mix-OFFT_MIX_THREADS=63"] == h["mix"], h


@pytest.mark.parametrize("group", [g for g in child.GROUPS if g != "mix"])
def test_default_child_computes_what_this_process_computes(group, built):
    """the children test what the library does: the cases of a group run here, in the suite's own process with the
    defaults, give the bits of the group's default child.  (Not the mix group: its children need two switches that this
    process was not started with.)"""
    assert not FAULTED, "not started: child %s ended by a signal, an abort or its time limit" % FAULTED[0]
    assert not [k for k in child.SWITCHES + ("OFFT_BLUESTEIN_LONG",) if k in os.environ], "the suite itself runs under a launcher switch"
    want = hashes(group)[group]
    assert child.run_group(group, {}) == want
