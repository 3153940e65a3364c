"""Launch-for-launch probe of the kernel launcher (offt_kernels.hip: resolve() and offt_hipk_prepare()).

One process, a fixed case list with at least one case per route and per kind of four-step split, in both precisions.
Per case: offt_hipk_prepare, one offt_hipk_fft_pass (or offt_hipk_conv_pass) on a seeded input of a few lines, a device
sync, and one printed line

    case  kernel_name  sha256(output bytes)

Two builds of the library compute the same thing launch for launch when these lines are identical and a kernel trace of
the run (rocprofv3 --kernel-trace --stats -- python tools/route_probe.py) lists the same dispatches in the same order.
OFFT_AMD_LIB selects the build (offt_amd/_lib.py).  Needs a GPU."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from offt_amd import api  # noqa: E402
from test_gpu_descriptors import Desc  # noqa: E402
from test_pass_routes import Filter  # noqa: E402

F64, F32 = api.F64, api.F32
NB1, NB2 = 2, 1


def blocks_of(n, split, nfloor):
    if nfloor:
        return nfloor + (n - split * nfloor) // (split + 1)
    return (n + split - 1) // split if split else 1


def side(n, ncols, contig, split, nfloor, rng, table):
    """a dense layout of [b1][block][..] for one side -> (axis, col, b1, blk, table or None, elements)"""
    big = (split + (1 if nfloor else 0)) if split else n  # longest block
    nblk = blocks_of(n, split, nfloor)
    axis, col = (1, big) if contig else (ncols, 1)
    blk = big * ncols
    b1 = blk * nblk
    tab = None
    if split and table:  # the blocks in shuffled places; the block stride is then a value that would be wrong
        tab = torch.from_numpy((rng.permutation(nblk) * blk).astype(np.int64)).cuda()
    return axis, col, b1, (blk if split else 0), tab, b1 * NB1 * NB2


def max_offset(n, ncols, axis, col, b1, blk, split, nfloor, tab):
    """largest element offset the side addresses (checked against the allocation before anything is launched)"""
    t = tab.cpu().numpy() if tab is not None else None
    top = 0
    for k in range(n):
        if not split:
            o = k * axis
        else:
            if nfloor and k >= split * nfloor:
                a, r = nfloor + (k - split * nfloor) // (split + 1), (k - split * nfloor) % (split + 1)
            else:
                a, r = k // split, k % split
            o = (int(t[a]) if t is not None else a * blk) + r * axis
        top = max(top, o)
    return top + (ncols - 1) * col + (NB1 - 1) * b1


def cases():
    out = []

    def add(name, n, prec, inc=1, outc=1, ncols=8, **kw):
        out.append((("%s n=%d %s %s%s" % (name, n, "f32" if prec else "f64", "c" if inc else "s", "c" if outc else "s")), n, prec, inc, outc, ncols, kw))

    for prec in (F64, F32):
        # every direct and decomposing route, each with contiguous and strided sides
        for n in (1024, 256, 768, 1000, 432, 127, 1016, 90, 8192, 6000, 12000, 16384, 4800, 5000, 10000, 4076, 3057, 10007):
            for inc, outc in ((1, 1), (1, 0), (0, 1), (0, 0)):
                add("plain", n, prec, inc, outc)
        add("odd-ncols", 1024, prec, 1, 0, ncols=7)
        add("inverse-scaled", 1024, prec, 0, 1, direction=1, scale=1.0 / 1024)
        add("out_keep", 1024, prec, 1, 0, out_keep=1)
        add("out_keep", 768, prec, 1, 0, out_keep=1)
        add("no_pairs", 1024, prec, 1, 0, no_pairs=1)
        add("variant", 1024, prec, 1, 1, variant=1)
        add("variant-pair-range", 1024, prec, 1, 0, variant=200)
        add("variant-missing", 1024, prec, 1, 1, variant=57)
        # per-peer splits: power of two, another length, uneven, through a block table
        for n in (1024, 768, 127, 90):
            f = n // 3
            add("split-out-uneven", n, prec, 1, 0, out_split=(f, 3 - n % 3) if n % 3 else (f, 0))
            add("split-in-uneven-tab", n, prec, 0, 1, in_split=(f, 3 - n % 3) if n % 3 else (f, 0), table=1)
        add("split-out-pow2", 1024, prec, 1, 0, out_split=(256, 0))
        add("split-in-pow2-tab", 1024, prec, 0, 0, in_split=(128, 0), table=1)
        add("split-out-6", 768, prec, 1, 0, out_split=(6, 0))
        add("split-out-384", 1024 + 512, prec, 1, 0, out_split=(384, 0))
        # four-step lines: splits the decomposition follows, does not follow, uneven, through a table
        for n in (8192, 16384, 6000):
            add("four-split-follows", n, prec, 0, 0, in_split=(n // 4, 0), out_split=(n // 2, 0))
            add("four-split-follows-tab", n, prec, 1, 0, out_split=(n // 2, 0), table=1)
            add("four-split-not-followed", n, prec, 1, 0, out_split=(n // 1000 * 8 + 24, 0) if n % 1000 == 0 else (96, 0))
            f = n // 3
            add("four-split-uneven", n, prec, 0, 0, out_split=(f, 3 - n % 3) if n % 3 else (f + 1, 0), table=1)
        # real input and real output: panel, plan-time, Bluestein, any-length, four-step lengths, and 8192 with blocks fft_panel_k cannot address
        for n in (1024, 768, 1016, 90, 16384, 6000, 8192):
            add("r2c", n, prec, 1, 1, real_input=1)
            add("r2c", n, prec, 1, 0, real_input=1)
            add("c2r", n, prec, 1, 1, real_input=2, direction=1)
            add("c2r", n, prec, 0, 1, real_input=2, direction=1)
        add("c2r-split-uneven", 8192, prec, 0, 1, real_input=2, direction=1, in_split=(2730, 1))
        add("c2r-split-uneven", 1024, prec, 0, 1, real_input=2, direction=1, in_split=(341, 2))
        add("r2c-bad-shape", 1024, prec, 1, 0, real_input=1, direction=1)
        # fused convolution
        add("conv-real", 256, prec, conv=0)
        add("conv-complex", 1024, prec, conv=1, ncols=7)
        add("conv-complex-keep", 512, prec, conv=1, out_keep=1)
    add("pair-off-16B-grid", 1024, F32, 0, 1, misalign=1)
    add("pair-off-16B-grid", 2048, F32, 1, 0, misalign=1)
    add("pair-odd-b1-stride", 1024, F32, 0, 0, odd_b1=1)
    return out


def main():
    L = api.lib()
    L.offt_hipk_fft_pass.argtypes = [C.POINTER(Desc), C.c_void_p, C.c_void_p, C.c_void_p]
    L.offt_hipk_conv_pass.argtypes = [C.POINTER(Desc), C.POINTER(Filter), C.c_void_p, C.c_void_p, C.c_void_p]
    L.offt_hipk_prepare.argtypes = [C.c_int, C.c_int]
    L.offt_hipk_last_error.restype = C.c_char_p
    L.offt_hipk_kernel_name.restype = C.c_char_p
    L.offt_hipk_kernel_name.argtypes = [C.POINTER(Desc)]
    L.offt_hipk_conv_kernel_name.restype = C.c_char_p
    L.offt_hipk_conv_kernel_name.argtypes = [C.POINTER(Desc), C.POINTER(Filter)]
    torch.cuda.set_device(0)
    print("library:", os.path.basename(os.path.dirname(api._lib.LIB_PATH)) + "/" + os.path.basename(api._lib.LIB_PATH), flush=True)
    for idx, (name, n, prec, inc, outc, ncols, kw) in enumerate(cases()):
        rng = np.random.default_rng(1000 + idx)
        ct, ft = (np.complex64, torch.float32) if prec else (np.complex128, torch.float64)
        isp, inf = kw.get("in_split", (0, 0))
        osp, onf = kw.get("out_split", (0, 0))
        d = Desc()
        d.n, d.precision, d.direction, d.ncols, d.nb1, d.nb2 = n, prec, kw.get("direction", -1), ncols, NB1, NB2
        d.in_contig, d.out_contig, d.variant, d.scale = inc, outc, kw.get("variant", -1), kw.get("scale", 1.0)
        d.real_input, d.out_keep, d.no_pairs = kw.get("real_input", 0), kw.get("out_keep", 0), kw.get("no_pairs", 0)
        d.in_split, d.in_split_nfloor, d.out_split, d.out_split_nfloor = isp, inf, osp, onf
        ia, ic, ib1, iblk, itab, isize = side(n, ncols, inc, isp, inf, rng, kw.get("table"))
        oa, oc, ob1, oblk, otab, osize = side(n, ncols, outc, osp, onf, rng, kw.get("table"))
        if kw.get("odd_b1"):
            ib1, ob1, isize, osize = ib1 + 1, ob1 + 1, isize + NB1, osize + NB1
        d.in_axis_stride, d.in_col_stride, d.in_b1_stride, d.in_block_stride = ia, ic, ib1, (1 if itab is not None else iblk)
        d.out_axis_stride, d.out_col_stride, d.out_b1_stride, d.out_block_stride = oa, oc, ob1, (1 if otab is not None else oblk)
        d.in_block_tab = itab.data_ptr() if itab is not None else None
        d.out_block_tab = otab.data_ptr() if otab is not None else None
        assert max_offset(n, ncols, ia, ic, ib1, iblk, isp, inf, itab) < isize, name
        assert max_offset(n, ncols, oa, oc, ob1, oblk, osp, onf, otab) < osize, name
        off = 1 if kw.get("misalign") else 0  # one complex64 = 8 bytes off the 16-B grid
        src = (rng.standard_normal(isize + off) + 1j * rng.standard_normal(isize + off)).astype(ct)
        din = torch.from_numpy(src.view(np.float32 if prec else np.float64).copy()).cuda()
        dout = torch.from_numpy(np.full(osize + off, 7 - 3j, dtype=ct).view(np.float32 if prec else np.float64).copy()).cuda()
        esz = 8 if prec else 16
        assert L.offt_hipk_prepare(n, prec | (0x200 if d.real_input == 2 else 0)) == 0, (name, L.offt_hipk_last_error())
        torch.cuda.synchronize()
        if "conv" in kw:
            f = Filter()
            f.kind, f.axis_stride, f.col_stride, f.b1_stride = kw["conv"], 1, n, n * ncols
            h = rng.standard_normal(isize * (2 if kw["conv"] else 1)).astype(np.float32 if prec else np.float64)
            dh = torch.from_numpy(h).cuda()
            kname = L.offt_hipk_conv_kernel_name(C.byref(d), C.byref(f)).decode()
            rc = L.offt_hipk_conv_pass(C.byref(d), C.byref(f), dh.data_ptr(), din.data_ptr(), None)
            result = din
        else:
            kname = L.offt_hipk_kernel_name(C.byref(d)).decode()
            rc = L.offt_hipk_fft_pass(C.byref(d), din.data_ptr() + off * esz, dout.data_ptr() + off * esz, None)
            result = dout
        assert rc == 0, (name, L.offt_hipk_last_error())
        torch.cuda.synchronize()
        print("%-44s %-20s %s" % (name, kname, hashlib.sha256(result.cpu().numpy().tobytes()).hexdigest()[:32]), flush=True)
    print("route_probe done:", len(cases()), "cases")


if __name__ == "__main__":
    main()
