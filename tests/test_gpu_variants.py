"""-m gpu: every sweep variant of the panel kernels, forced through offt_pass_desc::variant, against the CPU interpreter.

The static sweep (run-fft -l) and offt_hip_set_variant hand out registry entries that are the default of no flavour;
tests/test_gpu_descriptors.py always asks for variant -1 and never reaches them.  Here every (n, precision, id, flavour)
of tests/golden/variant_flavours.json -- the entries a forced id really resolves to -- is launched in both directions on
descriptors drawn as in test_gpu_descriptors.make_case: a ragged column count over several panels, both batch
dimensions, random out_keep and scale, per-peer splits on either side, every other case through per-block base tables.
Before each launch offt_hipk_pass_route has to name the asked id: a forced variant that fell back to the default would
make the case a repetition of test_random_descriptors."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from offt_amd import api
from test_gpu_descriptors import Desc, layout, libs, make_case, run_both, with_tables  # noqa: F401 (libs: fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTE_PANEL, VARIANT_ANYSPLIT = 1, 100

with open(os.path.join(ROOT, "tests", "golden", "variant_flavours.json")) as _fh:
    ENTRIES = [tuple(e) for e in json.load(_fh)["entries"]]
LENGTHS = sorted({(e[0], e[1]) for e in ENTRIES})


def route(L, d):
    vid = C.c_int(-9)
    via = L.offt_hipk_pass_route(C.byref(d), C.byref(vid), None, None)
    return via, vid.value


def variant_case(rng, n, prec, vid, inc, outc, direction, cols, any_split, uneven=False):
    """make_case's descriptor with the flavour, direction and variant fixed, nb1, nb2 > 1, a column count that is no
    multiple of the panel width and fills at least two panels, and splits the entry's kernel addresses: power-of-two
    blocks for fft_panel_k, anything (other divisors, uneven F / F+1) for fft_panelx_k.  uneven: an F / F+1 split on one
    side of a power-of-two length, which has to leave fft_panel_k for the any-split instance"""
    d, _, _ = make_case(rng, n, prec)
    d.in_contig, d.out_contig, d.direction, d.variant, d.real_input = inc, outc, direction, vid, 0
    d.nb1, d.nb2 = int(rng.integers(2, 4)), 2
    if cols:  # one to two full panels and a ragged one
        d.ncols = cols * int(rng.integers(1, 3)) + int(rng.integers(1, cols))
    else:     # the panel width of this entry is not on record (offt_hipk_variant_info reads the contiguous / contiguous
        d.ncols = 33 + 2 * int(rng.integers(0, 4))  # flavour): odd and > 32 is ragged over >= 3 panels for widths 2 .. 16
    def pick_split():
        kind = int(rng.integers(0, 3))
        if kind == 0:
            return 0, 0
        if kind == 1 or not any_split:
            # (at most 32 blocks: with_tables spreads them over nblocks + 4 copies of the array's span)
            cands = [f for f in range(n // 32, n) if f and n % f == 0 and (any_split or f & (f - 1) == 0)]
            return int(rng.choice(cands)), 0
        p = int(rng.integers(2, 7))
        F, b = n // p, n % p
        return (F, p - b) if b else (F, 0)
    d.in_split, d.in_split_nfloor = pick_split()
    d.out_split, d.out_split_nfloor = pick_split()
    if uneven:
        F, b = n // 3, n % 3
        if rng.integers(0, 2):
            d.in_split, d.in_split_nfloor = F, 3 - b
        else:
            d.out_split, d.out_split_nfloor = F, 3 - b
    li = layout(rng, n, d.ncols, d.nb1, d.nb2, d.in_split, d.in_split_nfloor, d.in_contig)
    lo = layout(rng, n, d.ncols, d.nb1, d.nb2, d.out_split, d.out_split_nfloor, d.out_contig)
    d.in_axis_stride, d.in_col_stride, d.in_b1_stride, d.in_b2_stride, d.in_block_stride = li["axis"], li["col"], li["b1"], li["b2"], li["blk"]
    d.out_axis_stride, d.out_col_stride, d.out_b1_stride, d.out_b2_stride, d.out_block_stride = lo["axis"], lo["col"], lo["b1"], lo["b2"], lo["blk"]
    return d, li["total"], lo["total"]


def test_fixture_lengths_are_the_parametrisation():
    assert len(ENTRIES) >= 100 and len(LENGTHS) == 16


@pytest.mark.parametrize("n,prec", LENGTHS)
def test_forced_variant_descriptors(libs, n, prec):
    L, CB = libs
    L.offt_hipk_pass_route.argtypes = [C.POINTER(Desc), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.offt_hipk_variant_info.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    rng = np.random.default_rng(9000 + 2 * n + prec)
    assert L.offt_hipk_prepare(n, prec) == 0
    ft, ct = (np.float64, np.complex128) if prec == api.F64 else (np.float32, np.complex64)
    tol = 1e-13 if prec == api.F64 else 5e-6
    pow2 = n & (n - 1) == 0
    mine = [e for e in ENTRIES if e[:2] == (n, prec)]
    confirmed = set()

    def check(d, nin, nout, tables, want_id):
        tabs = [None, None]
        if tables:
            nin, nout, tabs = with_tables(rng, d, nin, nout)
        desc = {f: getattr(d, f) for f, _ in Desc._fields_}
        assert route(L, d) == (ROUTE_PANEL, want_id), desc
        src = (rng.standard_normal(nin) + 1j * rng.standard_normal(nin)).astype(ct)
        want, got = run_both(L, CB, d, src, nout, ct, ft, tabs)
        assert np.abs(got - want).max() <= tol * np.abs(want).max() * max(1.0, np.log2(n)), desc

    for _, _, vid, inc, outc in mine:
        cols = C.c_int(0)
        known = L.offt_hipk_variant_info(n, prec, vid, None, C.byref(cols)) == vid
        for direction in (-1, 1):
            for rep in range(2):
                d, nin, nout = variant_case(rng, n, prec, vid, inc, outc, direction, cols.value if known else 0, not pow2)
                if known:
                    assert d.ncols % cols.value and d.ncols > cols.value
                check(d, nin, nout, rep == 1, vid)
                confirmed.add((n, prec, vid, inc, outc, direction))
        if pow2:  # a split fft_panel_k cannot address: the forced id gives way to the length's any-split instance
            d, nin, nout = variant_case(rng, n, prec, vid, inc, outc, -1, cols.value if known else 0, True, uneven=True)
            check(d, nin, nout, bool(vid & 1), VARIANT_ANYSPLIT)
    # every entry of the fixture ran, in both directions, with the route query naming its id
    assert confirmed == {e + (s,) for e in mine for s in (-1, 1)}
