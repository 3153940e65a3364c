"""The routes test_pass_routes.py does not reach, pinned against a fixture (tests/golden/pass_routes_ext.json): descriptors
with offt_pass_desc::half set, filters with offt_filter_desc::mixed set, and the out-of-place convolution queries.

Like there, everything asked depends only on the kernel registry and needs no device: offt_hipk_kernel_name,
offt_hipk_has_half and offt_hipk_keeps_output over the half-line product (HALF_AXES), offt_hipk_conv_kernel_name,
offt_hipk_conv_has_fused, offt_hipk_conv_oop_kernel_name and offt_hipk_conv_has_fused_oop over the convolution product
(CONV_AXES), for the lengths of LENGTHS in both precisions.

The fixture was recorded once, with no OFFT_* environment switch set, from a build of the PARENT of the commit that
keyed the kernel registry by a typed role (`python tests/test_pass_routes_ext.py --record` with OFFT_AMD_LIB pointing at
that build), and it is never re-recorded: a difference is a change of behaviour.  Answers are folded with the Shared
tree of test_pass_routes.py; lengths that share a root are listed as runs of indices into LENGTHS."""
import ctypes as C
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from offt_amd import api  # noqa: E402
from test_pass_routes import ENV_SWITCHES, Desc, Shared, rle  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "pass_routes_ext.json")
LENGTHS = [32, 64, 128, 256, 512, 1024, 2048, 96, 192, 320, 384, 640, 768, 1000, 100, 896, 1536]

# Desc with offt_pass_desc::half: the field sits in the four bytes of padding in front of tw4
_fields = list(Desc._fields_)
_fields.insert([name for name, _ in _fields].index("tw4"), ("half", C.c_int))


class HalfDesc(C.Structure):
    _fields_ = _fields


assert C.sizeof(HalfDesc) == C.sizeof(Desc) == 192 and HalfDesc.tw4.offset == Desc.tw4.offset == 176 and HalfDesc.half.offset == 172


class MixedFilter(C.Structure):
    _fields_ = [("kind", C.c_int), ("mixed", C.c_int), ("axis_stride", C.c_longlong), ("col_stride", C.c_longlong),
                ("b1_stride", C.c_longlong), ("b2_stride", C.c_longlong)]


# crossed in this order (the last one varies fastest)
HALF_AXES = [("half", list(range(9))),
             ("contig", [(1, 1), (1, 0), (0, 1), (0, 0)]),  # (in_contig, out_contig)
             ("real_input", [0, 1, 2]),
             ("direction", [-1, 1]),
             ("ncols", [64, 63]),
             ("no_pairs", [0, 1]),
             ("in_split", [0, 8]),
             ("tw4", [0, 1])]                                # any non-null pointer: nothing dereferences it
CONV_AXES = [("half", [0, 1, 3]),
             ("mixed", [0, 1, 2, 3]),
             ("kind", [0, 1, 2]),                            # kind 2 does not exist
             ("axis_stride", [1, 2]),
             ("in_contig", [1, 0]),
             ("real_input", [0, 1]),
             ("in_split", [0, 8])]
# every answer the name queries could give without a device before the registry knew its kernels' names; the recording
# refuses a product that misses one ("fft_bluestein_k" needs tables that only offt_hipk_prepare builds, on a device)
FAMILIES = ["fft_panel_k", "fft_panel_k<pairs>", "fft_panelx_k", "fft_c2r_panel_k", "fft_c2r_panelx_k", "fft_mixed_k",
            "fft_half_panel_k", "fft_half_panel_k<pairs>", "fft_half_panelx_k", "fft_half_r2c_panel_k", "fft_half_c2r_panel_k",
            "fft_half_r2c_panelx_k", "fft_half_c2r_panelx_k", "no half-line kernel",
            "fft_conv_panel_k", "fft_conv_half_panel_k", "fft_conv_panelx_k", "fft_conv_half_panelx_k",
            "fft_conv_oop_panel_k", "fft_conv_oop_half_panel_k", "fft_conv_oop_panelx_k", "fft_conv_oop_half_panelx_k", "no fused kernel"]


class Bound:
    """prototypes of this module's own: the library object is shared with tests that bind the same symbols to their structs"""

    def __init__(self, lib):
        for name in ("offt_hipk_kernel_name", "offt_hipk_has_half", "offt_hipk_keeps_output", "offt_hipk_conv_kernel_name",
                     "offt_hipk_conv_has_fused", "offt_hipk_conv_oop_kernel_name", "offt_hipk_conv_has_fused_oop"):
            args = [C.POINTER(HalfDesc)] + ([C.POINTER(MixedFilter)] if "_conv_" in name else [])
            setattr(self, name, C.CFUNCTYPE(C.c_char_p if name.endswith("_name") else C.c_int, *args)((name, lib)))


def bind():
    return Bound(api.lib())


def base_desc(n, prec):
    d = HalfDesc()
    d.n, d.precision, d.nb1, d.nb2, d.scale, d.variant = n, prec, 4, 1, 1.0, -1
    return d


def set_sides(d, inc, outc, ncols, in_split):
    """a contiguous side has axis stride 1, a strided one unit column stride, as test_pass_routes.descriptor_answers has them"""
    n = d.n
    d.in_contig, d.out_contig, d.ncols = inc, outc, ncols
    d.in_axis_stride, d.in_col_stride = (1, 2 * n) if inc else (ncols + (ncols & 1), 1)
    d.out_axis_stride, d.out_col_stride = (1, 2 * n) if outc else (ncols + (ncols & 1), 1)
    d.in_b1_stride = d.out_b1_stride = 2 * n * 64
    d.in_split, d.in_block_stride = in_split, 4096 if in_split else 0


def half_answers(L, n, prec):
    d = base_desc(n, prec)
    d.out_keep = 1
    ref = C.byref(d)
    tab = C.addressof(C.create_string_buffer(64))
    out = []
    for half, (inc, outc), ri, direction, ncols, nopairs, isp, tw4 in itertools.product(*[v for _, v in HALF_AXES]):
        set_sides(d, inc, outc, ncols, isp)
        d.half, d.real_input, d.direction, d.no_pairs, d.tw4 = half, ri, direction, nopairs, tab if tw4 else None
        out.append("%s/%d/%d" % (L.offt_hipk_kernel_name(ref).decode(), L.offt_hipk_has_half(ref), L.offt_hipk_keeps_output(ref)))
    return out


def conv_answers(L, n, prec):
    d = base_desc(n, prec)
    d.direction = -1
    f = MixedFilter()
    f.col_stride, f.b1_stride = n, 64 * n
    ref, fref = C.byref(d), C.byref(f)
    out = []
    for half, mixed, kind, fax, inc, ri, isp in itertools.product(*[v for _, v in CONV_AXES]):
        set_sides(d, inc, 1, 64, isp)
        d.half, d.real_input = half, ri
        f.mixed, f.kind, f.axis_stride = mixed, kind, fax
        out.append("%s/%d/%s/%d" % (L.offt_hipk_conv_kernel_name(ref, fref).decode(), L.offt_hipk_conv_has_fused(ref, fref),
                                    L.offt_hipk_conv_oop_kernel_name(ref, fref).decode(), L.offt_hipk_conv_has_fused_oop(ref, fref)))
    return out


PARTS = [("half", HALF_AXES, half_answers), ("conv", CONV_AXES, conv_answers)]


def record(L):
    sh = Shared()
    res = {"lengths": LENGTHS, "axes": {part: [[k, v] for k, v in axes] for part, axes, _ in PARTS}, "precisions": {}}
    seen = set()
    for prec in (api.F64, api.F32):
        res["precisions"][str(prec)] = {}
        for part, axes, answers in PARTS:
            by_root = {}
            for i, n in enumerate(LENGTHS):
                a = answers(L, n, prec)
                seen.update(x for s in a for x in s.split("/"))
                by_root.setdefault(sh.fold(a, [len(v) for _, v in axes]), []).append(i)
            res["precisions"][str(prec)][part] = {str(root): rle(idx) for root, idx in sorted(by_root.items())}
    missing = [k for k in FAMILIES if k not in seen]
    assert not missing, "the product lacks a flavour for %s" % missing
    res["nodes"] = sh.nodes
    return res


def expand(runs):
    """'start+count' runs -> indices"""
    for r in runs.split():
        start, _, count = r.partition("+")
        yield from range(int(start), int(start) + int(count or 1))


def where(axes, index):
    out = []
    for name, vals in reversed(axes):
        out.append("%s=%s" % (name, vals[index % len(vals)]))
        index //= len(vals)
    return " ".join(reversed(out))


def test_half_mixed_and_out_of_place_routes_match_the_fixture(built):
    assert not ENV_SWITCHES, "recorded with no OFFT_* switch set: %s" % ENV_SWITCHES
    with open(GOLDEN) as fh:
        want = json.load(fh)
    assert want["lengths"] == LENGTHS
    assert want["axes"] == json.loads(json.dumps({part: [[k, v] for k, v in axes] for part, axes, _ in PARTS}))
    L = bind()
    sh = Shared(want["nodes"])
    for prec in (api.F64, api.F32):
        for part, axes, answers in PARTS:
            roots = {i: int(root) for root, runs in want["precisions"][str(prec)][part].items() for i in expand(runs)}
            assert sorted(roots) == list(range(len(LENGTHS))), (prec, part)
            for i, n in enumerate(LENGTHS):
                g, e = answers(L, n, prec), sh.unfold(roots[i])
                assert len(g) == len(e), (prec, part, n)
                if g != e:
                    k = next(k for k in range(len(g)) if g[k] != e[k])
                    raise AssertionError("%s part, precision %d n=%d %s: %s, the fixture has %s (%d entries differ)" % (
                        part, prec, n, where(axes, k), g[k], e[k], sum(x != y for x, y in zip(g, e))))


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_pass_routes_ext.py --record")
    assert not ENV_SWITCHES, ENV_SWITCHES
    with open(GOLDEN, "w") as fh:
        json.dump(record(bind()), fh, separators=(",", ":"), sort_keys=True)
        fh.write("\n")
    print("recorded", GOLDEN, os.path.getsize(GOLDEN), "bytes from", api._lib.LIB_PATH)
