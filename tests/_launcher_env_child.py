"""Child process of tests/test_gpu_launcher_switches.py: one process, one setting of the launcher's environment switches
(struct Env of offt_kernels.hip, read once per process), one named group of cases.

    python tests/_launcher_env_child.py <group>        with OFFT_TEST_EXPECT="NAME=VALUE,..." in the environment

OFFT_TEST_EXPECT names the switch settings the parent MEANT to run the child under (empty: the defaults).  The child does
not look at the switches themselves: before it launches anything it asks the library's device-free queries what a
descriptor resolves to and asserts that this is what the expected setting selects, so a child started without its switch
(or under another group's) fails there instead of testing the default path once more.  Then it runs the group's fixed,
seeded descriptors through offt_hipk_fft_pass (the pair group: offt_hipk_fft_pass_pair) and through the CPU interpreter of
tests/libcpubackend.so, the sentinel in every element a pass does not own, tolerance 1e-13 (double) / 5e-6 (single) times
max|want| max(1, log2 n), and ends with

    SWITCH OK <group> <cases run> <sha256 of all GPU outputs concatenated>

or dies on the first failed assertion.  run_group() is what the parent calls in-process for the default setting."""
import ctypes as C
import hashlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

ROUTE_NONE, ROUTE_PANEL, ROUTE_BLUE, ROUTE_ANY_LENGTH, ROUTE_FOUR_STEP, ROUTE_SCRATCH = 0, 1, 2, 3, 4, 5
PREP_C2R = 0x200
SWITCHES = ("OFFT_XCD_REMAP", "OFFT_PAIR_RUN", "OFFT_KEEP_STORES", "OFFT_F32_PAIRS", "OFFT_BLUESTEIN", "OFFT_R2C_BLUESTEIN",
            "OFFT_BLUESTEIN_LONG_POW2", "OFFT_FOURSTEP", "OFFT_FOURSTEP_N1", "OFFT_MIX_THREADS", "OFFT_RTC", "OFFT_RTC_SHAPES")
GROUPS = ("order", "pair", "keep", "pairs32", "blue", "four", "mix", "rtc")


def parse_expect(text):
    out = {}
    for item in filter(None, (text or "").split(",")):
        k, v = item.split("=")
        assert k in SWITCHES, k
        out[k] = int(v)
    return out


class Ctx:
    """the two libraries, the running hash and the case count"""

    def __init__(self):
        import torch
        from offt_amd import api
        import test_gpu_descriptors as T
        self.torch, self.api, self.T, self.Desc = torch, api, T, T.Desc
        D = C.POINTER(T.Desc)
        L = api.lib()
        L.offt_hipk_fft_pass.argtypes = [D, C.c_void_p, C.c_void_p, C.c_void_p]
        L.offt_hipk_fft_pass_pair.argtypes = [D, C.c_void_p, C.c_void_p, D, C.c_void_p, C.c_void_p, C.c_void_p]
        L.offt_hipk_prepare.argtypes = [C.c_int, C.c_int]
        L.offt_hipk_last_error.restype = C.c_char_p
        L.offt_hipk_kernel_name.restype = C.c_char_p
        L.offt_hipk_kernel_name.argtypes = [D]
        L.offt_hipk_pair_kernel_name.restype = C.c_char_p
        L.offt_hipk_pair_kernel_name.argtypes = [D, D]
        L.offt_hipk_has_pass_pair.argtypes = [D, D]
        L.offt_hipk_pass_pair_grid.argtypes = [D, D, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
        L.offt_hipk_panel_order.argtypes = [C.c_longlong, C.POINTER(C.c_longlong)]
        L.offt_hipk_any_length_threads.argtypes = [C.c_int, C.c_int]
        L.offt_hipk_keeps_output.argtypes = [D]
        L.offt_hipk_pass_route.argtypes = [D, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.offt_hipk_variant_count.argtypes = [C.c_int, C.c_int]
        L.offt_hipk_variant_info.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.offt_hipk_has_fast_path.argtypes = [C.c_int, C.c_int]
        CB = C.CDLL(os.path.join(ROOT, "tests", "libcpubackend.so"))
        CB.cpu_backend_run_pass.argtypes = [D, C.c_void_p, C.c_void_p]
        self.L, self.CB = L, CB
        self.sha = hashlib.sha256()
        self.ran = 0

    # ---- queries ----
    def types(self, prec):
        return (np.float64, np.complex128, 1e-13) if prec == self.api.F64 else (np.float32, np.complex64, 5e-6)

    def name(self, d):
        return self.L.offt_hipk_kernel_name(C.byref(d)).decode()

    def route(self, d):
        vid, n1, n2 = C.c_int(-9), C.c_int(-9), C.c_int(-9)
        via = self.L.offt_hipk_pass_route(C.byref(d), C.byref(vid), C.byref(n1), C.byref(n2))
        return via, vid.value, n1.value, n2.value

    def cols_of(self, d):
        """columns per workgroup of the panel kernel the descriptor's flavour resolves to: the registry id from the
        route, the shape of that id from offt_hipk_variant_info"""
        p = self.copy(d)
        p.ncols = p.nb1 = p.nb2 = 1
        via, vid, _, _ = self.route(p)
        assert via == ROUTE_PANEL and 0 <= vid < 100, (via, vid, d.n)
        cols = C.c_int(0)
        assert self.L.offt_hipk_variant_info(d.n, d.precision, vid, None, C.byref(cols)) == vid
        return cols.value

    def copy(self, d):
        return self.Desc.from_buffer_copy(bytes(d))

    def fields(self, d):
        return {f: getattr(d, f) for f, _ in self.Desc._fields_}

    def prepare(self, n, prec):
        assert self.L.offt_hipk_prepare(n, prec) == 0, self.L.offt_hipk_last_error()

    # ---- descriptors ----
    def plain(self, n, prec, inc, outc, direction=-1, scale=1.0):
        d = self.Desc()
        d.n, d.precision, d.direction, d.ncols, d.nb1, d.nb2 = n, prec, direction, 1, 1, 1
        d.in_contig, d.out_contig, d.variant, d.scale = inc, outc, -1, scale
        return d

    def relayout(self, rng, d):
        T = self.T
        li = T.layout(rng, d.n, d.ncols, d.nb1, d.nb2, d.in_split, d.in_split_nfloor, d.in_contig)
        lo = T.layout(rng, d.n, d.ncols, d.nb1, d.nb2, d.out_split, d.out_split_nfloor, d.out_contig)
        d.in_axis_stride, d.in_col_stride, d.in_b1_stride, d.in_b2_stride, d.in_block_stride = li["axis"], li["col"], li["b1"], li["b2"], li["blk"]
        d.out_axis_stride, d.out_col_stride, d.out_b1_stride, d.out_b2_stride, d.out_block_stride = lo["axis"], lo["col"], lo["b1"], lo["b2"], lo["blk"]
        return li["total"], lo["total"]

    def shape_panels(self, d, panels):
        """ncols, nb1, nb2 for a grid of exactly `panels` workgroups, the last column panel ragged"""
        cols = self.cols_of(d)
        for nb2 in (3, 2, 1):
            for nb1 in (7, 5, 4, 3, 2, 1):
                if panels % (nb1 * nb2) == 0:
                    ncp = panels // (nb1 * nb2)
                    d.ncols, d.nb1, d.nb2 = ncp * cols - (cols // 2 if cols > 1 else 0), nb1, nb2
                    assert -(-d.ncols // cols) * nb1 * nb2 == panels
                    return cols

    # ---- running ----
    def check(self, rng, d, nin, nout, tabs=(None, None)):
        """one descriptor on the interpreter and on the GPU, compared whole (sentinel included); the GPU's bits go into
        the hash"""
        ft, ct, tol = self.types(d.precision)
        src = (rng.standard_normal(nin) + 1j * rng.standard_normal(nin)).astype(ct)
        want, got = self.T.run_both(self.L, self.CB, d, src, nout, ct, ft, list(tabs))
        err, bound = np.abs(got - want).max(), tol * np.abs(want).max() * max(1.0, np.log2(d.n))
        assert err <= bound, (err, bound, self.fields(d))
        self.add(got, d)
        return want, got

    def add(self, *outputs_and_desc):
        """the GPU's bits of one case into the running hash; one line per case, so that two children can be compared"""
        *outputs, d = outputs_and_desc
        one = hashlib.sha256()
        for o in outputs:
            one.update(o.tobytes())
            self.sha.update(o.tobytes())
        self.ran += 1
        print("case %d: n=%d prec=%d %s %s" % (self.ran, d.n, d.precision, self.name(d), one.hexdigest()[:16]), flush=True)


def xcd_g(expect):
    v = expect.get("OFFT_XCD_REMAP", 32)
    return 0 if v <= 0 else 1 << (v.bit_length() - 1)


# ---------------------------------------------------------------------------------------------------------------------
def group_order(cx, expect):
    L, api = cx.L, cx.api
    G = xcd_g(expect)
    # the switch took effect: the order every launch works out for a grid is the expected one
    for nblk in (5, 255, 256, 4096, 10000, 70001):
        lim = C.c_longlong(-1)
        g = L.offt_hipk_panel_order(nblk, C.byref(lim))
        assert (g, lim.value) == (G, nblk // (8 * G) * (8 * G) if G else 0), ("OFFT_XCD_REMAP not in effect", nblk, g, lim.value, G)
    rng = np.random.default_rng(64001)
    for n in (16, 96):
        for prec in (api.F64, api.F32):
            cx.prepare(n, prec)
            for _ in range(2):
                d, nin, nout = cx.T.make_case(rng, n, prec, big_grid=True)
                cx.check(rng, d, nin, nout)
    # hand-built grids: per run length in play a panel count below 8 G (nothing renumbered), an exact multiple of 8 G,
    # and a multiple plus a tail that keeps launch order
    regimes = set()
    case = 0
    for g, counts in ((1, (5, 24, 29)), (8, (61, 192, 227)), (32, (253, 512, 643)), (256, (2045, 2048, 3075))):
        for panels in counts:
            prec = api.F64 if case % 2 == 0 else api.F32
            inc, outc = ((1, 1), (1, 0), (0, 1), (0, 0))[(case + case // 4) % 4]
            d = cx.plain(16, prec, inc, outc, direction=1 if case % 5 == 4 else -1, scale=0.5 if case % 2 else 1.0)
            cx.shape_panels(d, panels)
            nin, nout = cx.relayout(rng, d)
            lim = C.c_longlong(-1)
            L.offt_hipk_panel_order(panels, C.byref(lim))
            if g == G:
                regimes.add("below" if lim.value == 0 else "exact" if lim.value == panels else "tail")
                assert 0 <= lim.value <= panels and lim.value % (8 * G) == 0
            cx.check(rng, d, nin, nout)
            case += 1
    assert G not in (1, 8, 32, 256) or regimes == {"below", "exact", "tail"}, (G, regimes)


# ---------------------------------------------------------------------------------------------------------------------
# (y blocks, x blocks) per length.  Under the default run of 256 blocks: y longer than x and the reverse with neither a
# multiple of any run length in play (8, 64, 256, 4096); one role shorter than a single run of every setting (both == 0);
# equal counts that are a multiple of 8, 64 and 256; 601 and 512 exceed one period; and one case beyond 4096 blocks per
# role, so that OFFT_PAIR_RUN=4096 alternates at all.
PAIR_BLOCKS = {64: ((333, 77), (283, 601), (5, 21), (512, 512), (4136, 4105)),
               128: ((301, 75), (270, 777), (3, 9), (256, 256))}


def group_pair(cx, expect):
    L, api, torch = cx.L, cx.api, cx.torch
    G = xcd_g(expect)
    run = expect.get("OFFT_PAIR_RUN", 0)
    run = run if run >= 8 and run & (run - 1) == 0 else 8 * max(G, 1)
    rng = np.random.default_rng(64002)
    ct, ft = np.complex128, np.float64

    def pair(n, nyb, nxb, direction_x=-1, variant_y=-1):
        dy = cx.plain(n, api.F64, 1, 0, scale=float(rng.choice([1.0, 0.5, 1.0 / n])))
        dx = cx.plain(n, api.F64, 1, 1, direction=direction_x, scale=float(rng.choice([1.0, 0.5, 1.0 / n])))
        cx.shape_panels(dy, nyb)
        cx.shape_panels(dx, nxb)
        dy.variant = variant_y
        return dy, dx, cx.relayout(rng, dy), cx.relayout(rng, dx)

    def launch_pair(dy, dx, srcy, srcx, nouty, noutx):
        iny, inx = torch.from_numpy(srcy.view(ft).copy()).cuda(), torch.from_numpy(srcx.view(ft).copy()).cuda()
        outy = torch.from_numpy(np.full(nouty, 7 - 3j, dtype=ct).view(ft).copy()).cuda()
        outx = torch.from_numpy(np.full(noutx, 7 - 3j, dtype=ct).view(ft).copy()).cuda()
        torch.cuda.synchronize()
        rc = L.offt_hipk_fft_pass_pair(C.byref(dy), iny.data_ptr(), outy.data_ptr(), C.byref(dx), inx.data_ptr(), outx.data_ptr(), None)
        torch.cuda.synchronize()
        return rc, outy.cpu().numpy().view(ct), outx.cpu().numpy().view(ct)

    for n, blocks in PAIR_BLOCKS.items():
        cx.prepare(n, api.F64)
        for nyb, nxb in blocks:
            dy, dx, (niny, nouty), (ninx, noutx) = pair(n, nyb, nxb)
            assert L.offt_hipk_pair_kernel_name(C.byref(dy), C.byref(dx)).decode() == "fft_pair_yx_k", (n, nyb, nxb)
            # the switch took effect: run length and alternating part of this very grid
            ny, nx, both = C.c_longlong(-1), C.c_longlong(-1), C.c_longlong(-1)
            got_run = L.offt_hipk_pass_pair_grid(C.byref(dy), C.byref(dx), C.byref(ny), C.byref(nx), C.byref(both))
            assert (ny.value, nx.value) == (nyb, nxb), (ny.value, nx.value, nyb, nxb)
            assert (got_run, both.value) == (run, min(nyb, nxb) // run * run), ("OFFT_PAIR_RUN / OFFT_XCD_REMAP not in effect", got_run, both.value, run)
            # the two passes as launches of their own (the paired launch stores y with the default cache policy: out_keep)
            ky = cx.copy(dy)
            ky.out_keep = 1
            srcy = (rng.standard_normal(niny) + 1j * rng.standard_normal(niny)).astype(ct)
            srcx = (rng.standard_normal(ninx) + 1j * rng.standard_normal(ninx)).astype(ct)
            wanty, sepy = cx.T.run_both(L, cx.CB, ky, srcy, nouty, ct, ft, [None, None])
            wantx, sepx = cx.T.run_both(L, cx.CB, dx, srcx, noutx, ct, ft, [None, None])
            rc, goty, gotx = launch_pair(dy, dx, srcy, srcx, nouty, noutx)
            assert rc == 0, L.offt_hipk_last_error()
            for want, sep, got, d in ((wanty, sepy, goty, dy), (wantx, sepx, gotx, dx)):
                err, bound = np.abs(got - want).max(), 1e-13 * np.abs(want).max() * np.log2(n)
                assert err <= bound, (err, bound, nyb, nxb, cx.fields(d))
                assert got.tobytes() == sep.tobytes(), ("paired and separate launches differ in bits", nyb, nxb, cx.fields(d))
            cx.add(goty, gotx, dy)
    # what the paired launch must refuse, with nothing written: a forced variant that is another kernel, an inverse x pass,
    # a length without a paired kernel
    forced = None
    for n in (64, 128, 256, 512, 1024):
        probe = cx.plain(n, api.F64, 1, 0)
        probe.out_keep = 1
        default_id = cx.route(probe)[1]
        for v in range(L.offt_hipk_variant_count(n, api.F64)):
            probe.variant = v
            if forced is None and cx.route(probe)[:2] == (ROUTE_PANEL, v) and v != default_id:
                forced = (n, v)
    assert forced is not None, "no length of the paired kernels has a second y-pass variant"
    cx.prepare(forced[0], api.F64)
    cx.prepare(96, api.F64)
    for n, kw in ((forced[0], dict(variant_y=forced[1])), (64, dict(direction_x=1)), (96, {})):
        dy, dx, (niny, nouty), (ninx, noutx) = pair(n, 3, 3, **kw)
        assert L.offt_hipk_has_pass_pair(C.byref(dy), C.byref(dx)) == 0, (n, kw)
        assert L.offt_hipk_pair_kernel_name(C.byref(dy), C.byref(dx)).decode() == "no paired kernel"
        assert L.offt_hipk_pass_pair_grid(C.byref(dy), C.byref(dx), None, None, None) == -1
        rc, goty, gotx = launch_pair(dy, dx, np.ones(niny, dtype=ct), np.ones(ninx, dtype=ct), nouty, noutx)
        assert rc == -1 and L.offt_hipk_last_error(), (n, kw, rc)
        assert np.all(goty == 7 - 3j) and np.all(gotx == 7 - 3j), (n, kw)


# ---------------------------------------------------------------------------------------------------------------------
def group_keep(cx, expect):
    L, api = cx.L, cx.api
    on = expect.get("OFFT_KEEP_STORES", 1) != 0
    rng = np.random.default_rng(64003)
    cases = []
    for n in (64, 256, 1024):
        for prec in (api.F64, api.F32):
            cx.prepare(n, prec)
            for it in range(4):
                d, nin, nout = cx.T.make_case(rng, n, prec)
                d.out_keep = 1
                tabs = [None, None]
                if it % 2 == 1:
                    nin, nout, tabs = cx.T.with_tables(rng, d, nin, nout)
                cases.append((d, nin, nout, tabs))
    keeps = [L.offt_hipk_keeps_output(C.byref(d)) for d, _, _, _ in cases]
    if on:
        assert sum(keeps) >= 3, ("no case of the list has a cache-keeping twin", keeps)
    else:
        assert sum(keeps) == 0, ("OFFT_KEEP_STORES=0 not in effect", keeps)
    for d, nin, nout, tabs in cases:
        cx.check(rng, d, nin, nout, tabs)


# ---------------------------------------------------------------------------------------------------------------------
def group_pairs32(cx, expect):
    api = cx.api
    on = expect.get("OFFT_F32_PAIRS", 1) != 0
    rng = np.random.default_rng(64004)
    for n in (512, 1024):
        cx.prepare(n, api.F32)
        for it in range(8):
            # every other case forces pair variant 0: pick_variant0 honours it whatever the switch says
            d, nin, nout = cx.T.make_pair_case(rng, n, 200 if it % 2 else -1)
            tabs = [None, None]
            if it % 4 >= 2:
                nin, nout, tabs = cx.T.with_tables(rng, d, nin, nout)
            d.in_block_tab = tabs[0].ctypes.data if tabs[0] is not None else None   # (the eligibility looks at the tables)
            d.out_block_tab = tabs[1].ctypes.data if tabs[1] is not None else None
            want = "fft_panel_k<pairs>" if on or d.variant == 200 else "fft_panel_k"
            assert cx.name(d) == want, ("OFFT_F32_PAIRS not in effect" if d.variant < 0 else "forced pair variant not honoured", cx.name(d), cx.fields(d))
            assert (cx.route(d)[1] >= 200) == (want != "fft_panel_k"), cx.route(d)
            cx.check(rng, d, nin, nout, tabs)


# ---------------------------------------------------------------------------------------------------------------------
def c2r_check(cx, rng, n, prec):
    """a real-output descriptor (real_input = 2; the interpreter of libcpubackend.so does not know them) against
    numpy.fft.irfft in double precision, as tests/test_c2r.py does, in this file's tolerance"""
    import test_c2r as R
    torch = cx.torch
    ft, ct, tol = cx.types(prec)
    d, nin, nout, tab, blk = R._rand_desc(rng, n, prec)
    d = cx.Desc.from_buffer_copy(bytes(d))   # (the same structure, declared a second time over there)
    nh = n // 2 + 1
    src = (rng.standard_normal(nin) + 1j * rng.standard_normal(nin)).astype(ct)
    offs = R._offsets(np.arange(nh), d.in_split, d.in_split_nfloor, d.in_axis_stride, blk, tab)
    want = np.full(2 * nout, 7.0, dtype=np.float64)
    for b2 in range(d.nb2):
        for b1 in range(d.nb1):
            for c in range(d.ncols):
                base = b2 * d.in_b2_stride + b1 * d.in_b1_stride + c * d.in_col_stride
                obase = 2 * (b2 * d.out_b2_stride + b1 * d.out_b1_stride + c * d.out_col_stride)
                want[obase:obase + n] = np.fft.irfft(src[base + offs].astype(np.complex128), n) * n * d.scale
    dt = torch.from_numpy(tab.copy()).cuda() if tab is not None else None
    d.in_block_tab = dt.data_ptr() if dt is not None else None
    return d, src, want, nout, dt   # (dt: the device table d points to -- the caller keeps it alive across the launch)


def group_blue(cx, expect):
    L, api, torch = cx.L, cx.api, cx.torch
    blue = expect.get("OFFT_BLUESTEIN", 1) != 0
    r2c = expect.get("OFFT_R2C_BLUESTEIN", 1) != 0
    pow2 = expect.get("OFFT_BLUESTEIN_LONG_POW2", 0) != 0
    rng = np.random.default_rng(64005)
    # complex lines of Bluestein lengths
    for n in (37, 127, 509):
        for prec in (api.F64, api.F32):
            cx.prepare(n, prec)
            for it in range(3):
                d, nin, nout = cx.T.make_case(rng, n, prec)
                if not d.real_input:
                    assert cx.name(d) == ("fft_bluestein_k" if blue else "fft_mixed_k"), ("OFFT_BLUESTEIN not in effect", cx.name(d), n)
                    assert cx.route(d)[0] == (ROUTE_BLUE if blue else ROUTE_ANY_LENGTH), cx.route(d)
                tabs = [None, None]
                if it == 1:
                    nin, nout, tabs = cx.T.with_tables(rng, d, nin, nout)
                cx.check(rng, d, nin, nout, tabs)
    # real lines of Bluestein lengths: scratch lines + the Bluestein kernel, or the any-length kernel
    for n in (254, 1016):
        for prec in (api.F64, api.F32):
            ft, ct, tol = cx.types(prec)
            cx.prepare(n, prec | PREP_C2R)
            want_route = ROUTE_SCRATCH if blue and r2c else ROUTE_ANY_LENGTH
            d = cx.plain(n, prec, 1, int(rng.integers(0, 2)), scale=0.5)
            d.real_input, d.ncols, d.nb1, d.nb2 = 1, int(rng.integers(3, 12)), 2, 2
            li = cx.T.layout(rng, n // 2 + 1, d.ncols, d.nb1, d.nb2, 0, 0, 1)
            lo = cx.T.layout(rng, n, d.ncols, d.nb1, d.nb2, 0, 0, d.out_contig)
            d.in_axis_stride, d.in_col_stride, d.in_b1_stride, d.in_b2_stride = li["axis"], li["col"], li["b1"], li["b2"]
            d.out_axis_stride, d.out_col_stride, d.out_b1_stride, d.out_b2_stride = lo["axis"], lo["col"], lo["b1"], lo["b2"]
            assert cx.route(d)[0] == want_route, ("OFFT_R2C_BLUESTEIN / OFFT_BLUESTEIN not in effect (real input)", cx.route(d), n)
            cx.check(rng, d, li["total"], lo["total"])
            d, src, want, nout, table = c2r_check(cx, rng, n, prec)
            assert cx.route(d)[0] == want_route, ("OFFT_R2C_BLUESTEIN / OFFT_BLUESTEIN not in effect (real output)", cx.route(d), n)
            din = torch.from_numpy(src.view(ft).copy()).cuda()
            dout = torch.full((2 * nout,), 7.0, dtype=torch.float64 if prec == api.F64 else torch.float32, device="cuda")
            torch.cuda.synchronize()
            assert L.offt_hipk_fft_pass(C.byref(d), din.data_ptr(), dout.data_ptr(), None) == 0, L.offt_hipk_last_error()
            torch.cuda.synchronize()
            got = dout.cpu().numpy()
            err, bound = np.abs(got.astype(np.float64) - want).max(), tol * np.abs(want).max() * np.log2(n)
            assert err <= bound, (err, bound, cx.fields(d))   # (the sentinel 7.0 outside the rows' n reals included)
            cx.add(got, d)
            del table
    # a long prime line: a Bluestein convolution through scratch lines of M points.  Which M is visible in what prepare()
    # made ready: 20480 = 64 x 320 points (the shortest fused four-step length >= 2 n - 1) or 32768
    n, prec = 10007, api.F64
    if blue:
        cx.prepare(n, prec)
        ready = {m: cx.route(cx.plain(m, prec, 1, 1))[0] for m in (20480, 32768)}
        if pow2:
            assert ready == {20480: ROUTE_NONE, 32768: ROUTE_FOUR_STEP}, ("OFFT_BLUESTEIN_LONG_POW2 not in effect", ready)
        else:  # (32768 points may have been prepared by somebody else in this process)
            assert ready[20480] == ROUTE_FOUR_STEP, ("OFFT_BLUESTEIN_LONG_POW2: not the default convolution length", ready)
        for inc, outc, direction in ((1, 1, -1), (0, 0, 1), (1, 0, 1), (0, 1, -1)):
            d = cx.plain(n, prec, inc, outc, direction=direction, scale=1.0 / n if direction > 0 else 1.0)
            d.ncols, d.nb1, d.nb2 = 2, 1, 1
            nin, nout = cx.relayout(rng, d)
            assert cx.route(d)[0] == ROUTE_SCRATCH, cx.route(d)
            cx.check(rng, d, nin, nout)
    else:  # the long net needs the Bluestein switch: the prime is refused at plan time, with a message
        assert L.offt_hipk_prepare(n, prec) != 0 and b"no kernel" in L.offt_hipk_last_error()


# ---------------------------------------------------------------------------------------------------------------------
FOUR_DEFAULT_N1 = {8192: 64, 16384: 32}   # 64 points in double, 32 in single precision
FOUR_FORCED = (2, 4, 8, 16, 32, 64)       # the first factors n1 <= sqrt(8192) of 8192


def group_four(cx, expect):
    L, api, torch = cx.L, cx.api, cx.torch
    on = expect.get("OFFT_FOURSTEP", 1) != 0
    forced = expect.get("OFFT_FOURSTEP_N1", 0)
    rng = np.random.default_rng(64006)
    for n, prec in ((8192, api.F64), (16384, api.F32)):
        ft, ct, tol = cx.types(prec)
        if not on and n == 16384:
            # no single launch takes the line and the decomposition is off: refused at plan time, and a pass launches nothing
            assert L.offt_hipk_prepare(n, prec) != 0, "OFFT_FOURSTEP=0 not in effect"
            assert b"no kernel for lines of 16384" in L.offt_hipk_last_error(), L.offt_hipk_last_error()
            d = cx.plain(n, prec, 0, 0)
            d.ncols = 4
            nin, nout = cx.relayout(rng, d)
            assert cx.route(d)[0] == ROUTE_NONE, cx.route(d)
            din = torch.zeros(2 * nin, dtype=torch.float32, device="cuda")
            dout = torch.full((2 * nout,), 7.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            assert L.offt_hipk_fft_pass(C.byref(d), din.data_ptr(), dout.data_ptr(), None) != 0
            assert L.offt_hipk_last_error(), "no message"
            torch.cuda.synchronize()
            assert bool((dout == 7.0).all())
            continue
        cx.prepare(n, prec)
        want_n1 = forced if forced in FOUR_FORCED else FOUR_DEFAULT_N1[n]
        for case, (inc, outc) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
            d = cx.plain(n, prec, inc, outc, direction=1 if case % 2 else -1, scale=float(rng.choice([1.0, 0.5, 1.0 / n])))
            d.ncols, d.nb1, d.nb2, d.out_keep = int(rng.integers(3, 8)), 2, int(rng.integers(1, 3)), case & 1
            via, vid, n1, n2 = cx.route(d)
            if n == 8192 and (not on or (inc and outc)):   # the one-column register kernel
                assert via == ROUTE_PANEL and cx.name(d) == "fft_panel_k", ("OFFT_FOURSTEP=0 not in effect", via, cx.name(d))
            else:
                assert (via, n1, n2) == (ROUTE_FOUR_STEP, want_n1, n // want_n1), ("OFFT_FOURSTEP_N1 / OFFT_FOURSTEP not in effect", via, n1, n2, want_n1)
                if case == 0 and n1 > 2:  # blocks the decomposition divides by n2 and n1, moved through tables
                    d.in_split, d.out_split = 2 * n2, 4 * n1
                    assert cx.route(d)[:1] == (ROUTE_FOUR_STEP,)
            nin, nout = cx.relayout(rng, d)
            tabs = [None, None]
            if d.in_split:
                nin, nout, tabs = cx.T.with_tables(rng, d, nin, nout)
            cx.check(rng, d, nin, nout, tabs)


# ---------------------------------------------------------------------------------------------------------------------
def group_mix(cx, expect):
    """(every child of this group also runs under OFFT_RTC=0: 1001 points is a plan-time length otherwise)"""
    L, api = cx.L, cx.api
    forced = expect.get("OFFT_MIX_THREADS", 0)
    rng = np.random.default_rng(64007)
    for n in (6, 90, 1001, 4099):
        for prec in (api.F64, api.F32):
            if (n, prec) == (1001, api.F64):   # has a precompiled fft_panelx_k instance: nothing sends it to the any-length kernel
                assert L.offt_hipk_has_fast_path(n, prec) == 1
                continue
            cx.prepare(n, prec)
            nt = L.offt_hipk_any_length_threads(n, prec)
            if 64 <= forced <= 1024:
                assert nt == forced, ("OFFT_MIX_THREADS not in effect", nt, forced)
            else:  # unset or out of range: the size the LDS footprint gives, never the out-of-range value
                assert nt in (64, 128, 256, 512, 1024) and nt * 2 <= max(128, 8 * n), (nt, n)
            kept = [0, 0]   # draws of make_case until two cases with an uneven F / F+1 split and two without are run
            while kept != [2, 2]:
                d, nin, nout = cx.T.make_case(rng, n, prec)
                uneven = int(bool(d.in_split_nfloor or d.out_split_nfloor))
                if kept[uneven] == 2:
                    continue
                kept[uneven] += 1
                if n == 4099:   # the interpreter's prime lines are O(n^2) sums: a handful of complex lines, still several panels
                    d.real_input, d.ncols, d.nb1, d.nb2 = 0, 1 + d.ncols % 3, 1, 1 + d.nb2 % 2
                    nin, nout = cx.relayout(rng, d)
                assert cx.name(d) == "fft_mixed_k" and cx.route(d)[0] == ROUTE_ANY_LENGTH, (cx.name(d), cx.route(d), n)
                tabs = [None, None]
                if kept[uneven] == 2:
                    nin, nout, tabs = cx.T.with_tables(rng, d, nin, nout)
                cx.check(rng, d, nin, nout, tabs)


# ---------------------------------------------------------------------------------------------------------------------
def group_rtc(cx, expect):
    L, api = cx.L, cx.api
    on = expect.get("OFFT_RTC", 1) != 0
    shapes = expect.get("OFFT_RTC_SHAPES", 1)
    prec = api.F64

    def smooth31(n):
        for p in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31):
            while n % p == 0:
                n //= p
        return n == 1
    # the first 31-smooth length of 256 .. 4096 points without a precompiled instance (one length: each shape is a compile)
    n = next(m for m in range(257, 4097) if smooth31(m) and not L.offt_hipk_has_fast_path(m, prec))
    t0 = time.time()
    cx.prepare(n, prec)
    print("prepare(%d): %.2f s" % (n, time.time() - t0), flush=True)
    count = L.offt_hipk_variant_count(n, prec)
    if not on:
        assert L.offt_hipk_has_fast_path(n, prec) == 0 and count == 0, ("OFFT_RTC=0 not in effect", count)
        variants = [-1]
    else:
        assert L.offt_hipk_has_fast_path(n, prec) == 1, "no plan-time kernel for n=%d" % n
        if shapes > 1:
            assert 2 <= count <= shapes, ("OFFT_RTC_SHAPES not in effect", count, shapes)
        else:
            assert count == 1, ("OFFT_RTC_SHAPES: more than the default shape compiled", count)
        variants = list(range(count))
    rng = np.random.default_rng(64008)
    for v in variants:
        for case, (inc, outc) in enumerate(((1, 1), (0, 0), (1, 0), (0, 1))):
            d, _, _ = cx.T.make_case(rng, n, prec)
            d.real_input, d.in_contig, d.out_contig, d.variant = 0, inc, outc, v
            nin, nout = cx.relayout(rng, d)
            if on:
                assert cx.name(d) == "fft_panelx_k" and cx.route(d)[:2] == (ROUTE_PANEL, v), (cx.name(d), cx.route(d), v)
            else:
                assert cx.name(d) == "fft_mixed_k" and cx.route(d)[0] == ROUTE_ANY_LENGTH, (cx.name(d), cx.route(d))
            tabs = [None, None]
            if case % 2 == 1:
                nin, nout, tabs = cx.T.with_tables(rng, d, nin, nout)
            cx.check(rng, d, nin, nout, tabs)


def run_group(group, expect):
    """-> (cases run, sha256 of the GPU outputs)"""
    cx = Ctx()
    {"order": group_order, "pair": group_pair, "keep": group_keep, "pairs32": group_pairs32, "blue": group_blue, "four": group_four,
     "mix": group_mix, "rtc": group_rtc}[group](cx, expect)
    assert cx.ran > 0
    return cx.ran, cx.sha.hexdigest()


if __name__ == "__main__":
    ran, digest = run_group(sys.argv[1], parse_expect(os.environ.get("OFFT_TEST_EXPECT")))
    print("SWITCH OK", sys.argv[1], ran, digest)
