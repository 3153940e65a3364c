"""Which kernel a pass descriptor resolves to, pinned against a fixture (tests/golden/pass_routes.json).

Everything asked here depends only on the kernel registry and needs no device: offt_hipk_kernel_name,
offt_hipk_keeps_output, offt_hipk_has_fast_path, offt_hipk_variant_count / _info / _name and the two convolution
queries.  The per-length calls are made for every n in 1..8192 in both precisions; the per-descriptor calls for every
length with a registered kernel plus a seeded sample of those without, crossed with the flavours of AXES below.

The fixture was recorded once, with no OFFT_* environment switch set, from the library as it stood BEFORE the kernel
launcher resolved routes in one place (`python tests/test_pass_routes.py --record`); it is not re-recorded when the
launcher changes: a difference is a change of behaviour.  Answers are grouped: the per-length part maps each answer to
the lengths that give it, the per-descriptor part shares equal sub-tables of the flavour product (class Shared)."""
import ctypes as C
import itertools
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from offt_amd import api  # noqa: E402
from test_gpu_descriptors import Desc  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "pass_routes.json")
NMAX = 8192
ENV_SWITCHES = [k for k in os.environ if k.startswith("OFFT_") and k not in ("OFFT_AMD_LIB", "OFFT_AMD_TEST_LIB")]


class Filter(C.Structure):
    _fields_ = [("kind", C.c_int), ("axis_stride", C.c_longlong), ("col_stride", C.c_longlong), ("b1_stride", C.c_longlong),
                ("b2_stride", C.c_longlong)]


# flavour axes of the per-descriptor part, crossed in this order (the last one varies fastest)
SPLITS = [(0, 0, 0, 0),      # (in_split, in_split_nfloor, out_split, out_split_nfloor): absent
          (8, 0, 0, 0), (0, 0, 8, 0), (8, 0, 8, 0),  # a power of two
          (6, 0, 0, 0), (0, 0, 6, 0),                # not a power of two
          (5, 3, 0, 0), (0, 0, 5, 3), (8, 0, 5, 3)]  # uneven
AXES = [("contig", [(1, 1), (1, 0), (0, 1), (0, 0)]),  # (in_contig, out_contig)
        ("real_input", [0, 1, 2]),
        ("direction", [-1, 1]),
        ("ncols", [64, 63]),
        ("strides", [0, 1, 2]),  # 0 plain; 1 odd b1 and block strides on a strided side; 2 axis stride 2 on a contiguous side
        ("split", SPLITS),
        ("block_tab", [0, 1]),   # any non-null pointer: nothing dereferences it
        ("variant", None),       # per length: -1, every registered id, the any-split id, the pair range, one that does not exist
        ("keep_nopairs_tw4", list(itertools.product((0, 1), repeat=3)))]  # (out_keep, no_pairs, tw4 non-null)
FILTERS = [(0, 1), (1, 1), (1, 2), (2, 1)]  # (kind, axis_stride) of the convolution queries; kind 2 does not exist
UNREGISTERED_FIXED = [1, 2, 3, 7, 31, 127, 254, 432, 1016, 1019, 2039, 3057, 4076, 4800, 5000, 5120, 5121, 6000, 8191,
                      10000, 10007, 10240, 10241, 12000, 16384, 32768]


def bind():
    L = api.lib()
    L.offt_hipk_kernel_name.restype = C.c_char_p
    L.offt_hipk_kernel_name.argtypes = [C.POINTER(Desc)]
    L.offt_hipk_keeps_output.argtypes = [C.POINTER(Desc)]
    L.offt_hipk_variant_name.restype = C.c_char_p
    L.offt_hipk_variant_name.argtypes = [C.c_int, C.c_int, C.c_int]
    L.offt_hipk_variant_info.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.offt_hipk_conv_kernel_name.restype = C.c_char_p
    L.offt_hipk_conv_kernel_name.argtypes = [C.POINTER(Desc), C.POINTER(Filter)]
    L.offt_hipk_conv_has_fused.argtypes = [C.POINTER(Desc), C.POINTER(Filter)]
    return L


def variant_ids(L, n, prec):
    return [-1] + list(range(L.offt_hipk_variant_count(n, prec))) + [100, 200, 201, 57]


def per_length(L, n, prec):
    """the per-length answers as one string"""
    out = [str(L.offt_hipk_has_fast_path(n, prec)), str(L.offt_hipk_variant_count(n, prec))]
    for v in variant_ids(L, n, prec):
        e, cols = C.c_int(-9), C.c_int(-9)
        rid = L.offt_hipk_variant_info(n, prec, v, C.byref(e), C.byref(cols))
        out.append("%d:%d,%d,%d:%s" % (v, rid, e.value, cols.value, L.offt_hipk_variant_name(n, prec, v).decode()))
    return "|".join(out)


def descriptor_answers(L, n, prec):
    """answers over the flavour product for one length, in product order"""
    d = Desc()
    f = Filter()
    f.col_stride, f.b1_stride = n, 64 * n
    ref = C.byref(d)
    name, keeps, cname, cfused = L.offt_hipk_kernel_name, L.offt_hipk_keeps_output, L.offt_hipk_conv_kernel_name, L.offt_hipk_conv_has_fused
    tab = C.addressof(C.create_string_buffer(64))
    axes = [vals if vals is not None else variant_ids(L, n, prec) for _, vals in AXES]
    d.n, d.precision, d.nb1, d.nb2, d.scale = n, prec, 4, 1, 1.0
    out = []
    for (inc, outc), ri, direction, ncols, sf, (isp, inf, osp, onf), bt in itertools.product(*axes[:7]):
        d.in_contig, d.out_contig, d.real_input, d.direction, d.ncols = inc, outc, ri, direction, ncols
        d.in_axis_stride, d.in_col_stride = (2 if sf == 2 else 1, 2 * n) if inc else (ncols + (ncols & 1), 1)
        d.out_axis_stride, d.out_col_stride = (2 if sf == 2 else 1, 2 * n) if outc else (ncols + (ncols & 1), 1)
        d.in_b1_stride = 2 * n * 64 + (1 if sf == 1 and not inc else 0)
        d.out_b1_stride = 2 * n * 64 + (1 if sf == 1 and not outc else 0)
        d.in_split, d.in_split_nfloor, d.out_split, d.out_split_nfloor = isp, inf, osp, onf
        d.in_block_stride = (4096 + (1 if sf == 1 else 0)) if isp else 0
        d.out_block_stride = (4096 + (1 if sf == 1 else 0)) if osp else 0
        d.in_block_tab = tab if bt and isp else None
        d.out_block_tab = tab if bt and osp else None
        for variant in axes[7]:
            d.variant = variant
            for keep, nopairs, tw4 in axes[8]:
                d.out_keep, d.no_pairs, d.tw4 = keep, nopairs, tab if tw4 else None
                a = "%s/%d" % (name(ref).decode(), keeps(ref))
                if variant == -1 and not nopairs:  # the convolution queries read neither
                    for kind, fax in FILTERS:
                        f.kind, f.axis_stride = kind, fax
                        a += "/%s%d" % ("C" if cname(ref, C.byref(f)) == b"fft_conv_panel_k" else "-", cfused(ref, C.byref(f)))
                out.append(a)
    return out


def rle(indices):
    """sorted indices -> 'start+count' runs"""
    runs, start, prev = [], None, None
    for i in indices:
        if start is None:
            start = prev = i
        elif i == prev + 1:
            prev = i
        else:
            runs.append((start, prev - start + 1))
            start = prev = i
    if start is not None:
        runs.append((start, prev - start + 1))
    return " ".join("%d+%d" % r if r[1] > 1 else "%d" % r[0] for r in runs)


class Shared:
    """The answers of one length over the flavour product, folded axis by axis from the fastest one: equal runs of
    children become one node, shared between lengths and precisions.  nodes[i] is an answer (a string) or the list of
    its children, one per value of its axis; a length's answers are the leaves under its root, in product order."""

    def __init__(self, nodes=None):
        self.nodes = [tuple(x) if isinstance(x, list) else x for x in (nodes or [])]
        self.ids = {x: i for i, x in enumerate(self.nodes)}
        self.flat = {}

    def node(self, x):
        if x not in self.ids:
            self.ids[x] = len(self.nodes)
            self.nodes.append(x)
        return self.ids[x]

    def fold(self, answers, sizes):
        level = [self.node(a) for a in answers]
        for k in reversed(sizes):
            level = [self.node(tuple(level[i:i + k])) for i in range(0, len(level), k)]
        assert len(level) == 1
        return level[0]

    def unfold(self, i):
        x = self.nodes[i]
        if isinstance(x, str):
            return [x]
        if i not in self.flat:
            self.flat[i] = [a for c in x for a in self.unfold(c)]
        return self.flat[i]


def descriptor_lengths(L, prec):
    reg = [n for n in range(1, NMAX + 1) if L.offt_hipk_has_fast_path(n, prec)]
    rng = random.Random(20240607 + prec)
    pool = [n for n in range(1, 2 * NMAX) if n not in reg and n not in UNREGISTERED_FIXED]
    return reg, sorted([n for n in UNREGISTERED_FIXED if n not in reg] + rng.sample(pool, 12))


def axis_sizes(L, n, prec):
    return [len(vals) if vals is not None else len(variant_ids(L, n, prec)) for _, vals in AXES]


def collect_lengths(L, prec):
    by = {}
    for n in range(1, NMAX + 1):
        by.setdefault(per_length(L, n, prec), []).append(n)
    return {a: rle(ns) for a, ns in sorted(by.items())}


def record(L):
    sh = Shared()
    res = {"axes": [[k, v] for k, v in AXES], "filters": FILTERS, "precisions": {}}
    for prec in (api.F64, api.F32):
        reg, unreg = descriptor_lengths(L, prec)
        roots = {str(n): sh.fold(descriptor_answers(L, n, prec), axis_sizes(L, n, prec)) for n in reg + unreg}
        res["precisions"][str(prec)] = {"per_length": collect_lengths(L, prec), "registered": reg, "unregistered_sample": unreg, "roots": roots}
    res["nodes"] = sh.nodes
    return res


def where(L, n, prec, index):
    """the flavour of entry `index` of a length's product, in words"""
    out = []
    for (name, vals), size in reversed(list(zip(AXES, axis_sizes(L, n, prec)))):
        v = (vals if vals is not None else variant_ids(L, n, prec))[index % size]
        out.append("%s=%s" % (name, v))
        index //= size
    return " ".join(reversed(out))


def test_pass_routes_match_the_fixture(built):
    assert not ENV_SWITCHES, "recorded with no OFFT_* switch set: %s" % ENV_SWITCHES
    with open(GOLDEN) as fh:
        want = json.load(fh)
    assert want["axes"] == json.loads(json.dumps([[k, v] for k, v in AXES])) and want["filters"] == json.loads(json.dumps(FILTERS))
    L = bind()
    sh = Shared(want["nodes"])
    for prec in (api.F64, api.F32):
        w = want["precisions"][str(prec)]
        got = collect_lengths(L, prec)
        assert sorted(got) == sorted(w["per_length"]), "per-length answers differ (precision %d)" % prec
        for a in got:
            assert got[a] == w["per_length"][a], (prec, a)
        reg, unreg = descriptor_lengths(L, prec)
        assert reg == w["registered"] and unreg == w["unregistered_sample"] and len(reg) >= 25
        assert sorted(w["roots"], key=int) == [str(n) for n in sorted(reg + unreg)]
        for n in reg + unreg:
            g, e = descriptor_answers(L, n, prec), sh.unfold(w["roots"][str(n)])
            assert len(g) == len(e), (prec, n)
            if g != e:
                i = next(i for i in range(len(g)) if g[i] != e[i])
                raise AssertionError("precision %d n=%d %s: %s, the fixture has %s (%d entries differ)" % (
                    prec, n, where(L, n, prec, i), g[i], e[i], sum(x != y for x, y in zip(g, e))))


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_pass_routes.py --record")
    assert not ENV_SWITCHES, ENV_SWITCHES
    with open(GOLDEN, "w") as fh:
        json.dump(record(bind()), fh, separators=(",", ":"), sort_keys=True)
        fh.write("\n")
    print("recorded", GOLDEN, os.path.getsize(GOLDEN), "bytes from", api._lib.LIB_PATH)
