"""Which registry entry a forced sweep variant gets (offt_hipk_pass_route), pinned against tests/golden/variant_flavours.json.

d->variant = id names an entry of the descriptor's (in_contig, out_contig) flavour; where the flavour has no entry with
that id the launcher falls back to the flavour's default without a word.  The fixture lists every (n, precision, id,
in_contig, out_contig) that really resolves to the asked id, over all lengths with at least two variants: these are the
instances tests/test_gpu_variants.py launches, and a registration that appears, disappears or moves to another flavour
shows here.  Registry lookups only: no device.

Recorded with `python tests/test_variant_flavours.py --record` and compared by hand with the reg_variant / reg_variantx
lines of offt_reg_pow2_*.hip and offt_reg_mixed_f64_*.hip; EXPECTED below restates those lines independently."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from offt_amd import api  # noqa: E402
from test_gpu_descriptors import Desc  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "variant_flavours.json")
NMAX = 8192
ROUTE_PANEL = 1
CC, SS, CS, SC = (1, 1), (0, 0), (1, 0), (0, 1)
FLAVOURS = [CC, SS, CS, SC]
STRIDED = [SS, CS, SC]
ENV_SWITCHES = [k for k in os.environ if k.startswith("OFFT_") and k not in ("OFFT_AMD_LIB", "OFFT_AMD_TEST_LIB")]

# (n, precision) -> {id: flavours the id is registered for and is NOT the default of}, from the registration lines
NON_DEFAULT = {
    (512, api.F64): {0: FLAVOURS},
    (1024, api.F64): {0: FLAVOURS, 2: FLAVOURS},
    (2048, api.F64): {0: [CC], 1: STRIDED},
    (512, api.F32): {0: [CC], 1: STRIDED},
    (1024, api.F32): {0: [CC], 1: STRIDED},
    (2048, api.F32): {1: FLAVOURS, 3: FLAVOURS, 0: [CC], 2: STRIDED},
}
# double-precision mixed-radix lengths with a narrow contiguous / contiguous shape: variant 1 exists for that flavour only
MIXED_NARROW_CC = [640, 896, 1000, 1001, 1120, 1152, 1200, 1500, 1792, 1920]


def bind():
    L = api.lib()
    L.offt_hipk_pass_route.argtypes = [C.POINTER(Desc), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.offt_hipk_variant_info.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    return L


def plain_desc(n, prec, variant, inc, outc, out_keep=0, ncols=63):
    """a descriptor without a split; the odd column count keeps single precision on the one-column kernels"""
    d = Desc()
    d.n, d.precision, d.direction, d.ncols, d.nb1, d.nb2, d.scale = n, prec, -1, ncols, 2, 1, 1.0
    d.in_contig, d.out_contig, d.variant, d.out_keep = inc, outc, variant, out_keep
    d.in_axis_stride, d.in_col_stride = (1, n) if inc else (ncols, 1)
    d.out_axis_stride, d.out_col_stride = (1, n) if outc else (ncols, 1)
    d.in_b1_stride = d.out_b1_stride = n * ncols
    return d


def route(L, d):
    vid, n1, n2 = C.c_int(-9), C.c_int(-9), C.c_int(-9)
    via = L.offt_hipk_pass_route(C.byref(d), C.byref(vid), C.byref(n1), C.byref(n2))
    return via, vid.value, n1.value, n2.value


def collect(L):
    """every (n, prec, id, in_contig, out_contig) whose forced id is the id that runs"""
    out = []
    for prec in (api.F64, api.F32):
        for n in range(1, NMAX + 1):
            nv = L.offt_hipk_variant_count(n, prec)
            if nv < 2:
                continue
            for vid in range(nv):
                for inc, outc in FLAVOURS:
                    got = []
                    for keep in (0, 1):
                        via, rid, n1, n2 = route(L, plain_desc(n, prec, vid, inc, outc, keep))
                        dvia, did, _, _ = route(L, plain_desc(n, prec, -1, inc, outc, keep))
                        assert via == ROUTE_PANEL and dvia == ROUTE_PANEL and (n1, n2) == (0, 0), (n, prec, vid, inc, outc, keep)
                        # never a third kernel: the asked id, or what the flavour runs by default
                        assert rid == vid or rid == did, (n, prec, vid, inc, outc, keep, rid, did)
                        got.append(rid == vid)
                    assert got[0] == got[1], "out_keep changes which id runs: %s" % ((n, prec, vid, inc, outc),)
                    if got[0]:
                        out.append([n, prec, vid, inc, outc])
    return out


def test_forced_variants_match_the_fixture(built):
    assert not ENV_SWITCHES, "recorded with no OFFT_* switch set: %s" % ENV_SWITCHES
    with open(GOLDEN) as fh:
        want = json.load(fh)["entries"]
    got = collect(bind())
    assert got == want, [e for e in got if e not in want] + [e for e in want if e not in got]


def test_fixture_holds_the_registered_non_default_instances(built):
    """the fixture against the registration lines, restated by hand above -- not against the library"""
    with open(GOLDEN) as fh:
        have = {tuple(e) for e in json.load(fh)["entries"]}
    assert len(have) >= 100
    for (n, prec), ids in NON_DEFAULT.items():
        for vid, flavours in ids.items():
            for inc, outc in flavours:
                assert (n, prec, vid, inc, outc) in have, (n, prec, vid, inc, outc)
    for n in MIXED_NARROW_CC:
        assert [e for e in have if e[0] == n and e[2] == 1] == [(n, api.F64, 1, 1, 1)], n
        assert {e[3:] for e in have if e[0] == n and e[1] == api.F64 and e[2] == 0} == set(STRIDED), n
    # every flavour of every length in it runs SOME listed id (its default), and no id is listed for a flavour twice
    for n, prec in {(e[0], e[1]) for e in have}:
        for inc, outc in FLAVOURS:
            assert any(e[0] == n and e[1] == prec and e[3:] == (inc, outc) for e in have), (n, prec, inc, outc)


def test_route_query_on_registry_only_descriptors(built):
    """answers that need no device: the any-split instance and a column-pair entry report their ranges, a forced id a
    flavour does not have falls back, four-step twiddles on a contiguous side and an empty batch launch nothing"""
    L = bind()
    d = plain_desc(1024, api.F64, 0, 1, 1)
    d.out_split, d.out_split_nfloor, d.out_block_stride = 341, 2, 4096
    assert route(L, d)[:2] == (ROUTE_PANEL, 100)
    d = plain_desc(1024, api.F32, -1, 1, 1, ncols=64)
    assert route(L, d)[:2] == (ROUTE_PANEL, 200)
    d.no_pairs = 1
    assert route(L, d)[:2] == (ROUTE_PANEL, 1)
    assert route(L, plain_desc(640, api.F64, 0, 1, 1))[:2] == (ROUTE_PANEL, 1)   # contiguous / contiguous has variant 1 only
    assert route(L, plain_desc(4099, api.F64, -1, 1, 1))[:2] == (3, -1)          # the any-length kernel
    tab = C.addressof(C.create_string_buffer(64))
    d = plain_desc(64, api.F64, -1, 0, 0)
    d.tw4, d.tw4_n2 = tab, 1
    assert route(L, d)[:2] == (ROUTE_PANEL, 0)
    d.in_contig = 1
    assert route(L, d)[:2] == (0, -1)
    d = plain_desc(64, api.F64, -1, 1, 1)
    d.ncols = 0
    assert route(L, d)[:2] == (0, -1)


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_variant_flavours.py --record")
    assert not ENV_SWITCHES, ENV_SWITCHES
    entries = collect(bind())
    with open(GOLDEN, "w") as fh:
        fh.write('{"fields":["n","precision","id","in_contig","out_contig"],"entries":[\n')
        fh.write(",\n".join(json.dumps(e, separators=(",", ":")) for e in entries))
        fh.write("\n]}\n")
    print("recorded", GOLDEN, len(entries), "entries")
