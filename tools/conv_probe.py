#!/usr/bin/env python3
"""Developer probe: spectral convolution (offt_hip_execute_convolve) against the two ways a caller has without it, in one
process.  After a warm-up the three ALTERNATE, so that all see the same box state, and the best of each is reported:
  (a) forward + inverse            offt_3d_execute, offt_3d_execute_dir(+1)
  (b) the caller's route           (a) with a torch multiply of the spectrum by H in between
  (c) the convolve                 one call (fused route where the plan has one)
against the byte model for complex data with a real filter, per point: (a) 6 x 2 esz x 2 (every pass reads and writes the
volume), (b) (a) + 2 x 2 esz + esz (multiply sweep: read, filter, write), (c) 4 x 2 esz x 2 + 2 x 2 esz + esz (r2c: the
same counts on the half spectrum for the y / x / fused passes, the z passes on the real rows).
A spec with the prefix mixed: measures OFFT_HIP_OPT_CONV_MIXED instead (x lengths that are no powers of two): the plan's
convolve with the option at 1 and at 0 ALTERNATES after a warm-up, MIXED_REPS times each (default 20), and the line
reports min and median of both, their ratios, the option-off route's own spread (median / min - 1) and the byte model
(c) / (b).  mixed:half:N does so on a pruned half-box plan (OFFT_HIP_OPT_HALF_MIXED, an N/2 box).
A spec with the prefix multi: measures offt_hip_execute_convolve_multi with K = 3 real filters (two outputs of their own,
the third in `data`) against three offt_hip_execute_convolve calls on the same plan and buffers -- the single-output code
is the baseline.  The two ALTERNATE after a warm-up, MIXED_REPS times each, and the line reports min and median of both,
their ratios, the baseline's own spread (median / min - 1) and the byte model of DESIGN.md 4.5.  multi:half:N does so on a
pruned half-box plan (an N/2 box).
A spec with the prefix multi:mixed: measures OFFT_HIP_OPT_CONV_MULTI_MIXED (the fused multi-output route at x lengths that
are no powers of two), with OFFT_HIP_OPT_CONV_MIXED on throughout: the multi call with the option at 1 ALTERNATES with three
offt_hip_execute_convolve calls and with the multi call with the option at 0 (the generic route: the code of before the
option existed), MIXED_REPS times each after a warm-up.  The line reports min and median of all three, the ratios against
both baselines, each baseline's own spread (median / min - 1) and the byte model of DESIGN.md 4.5 (376 / 504 for K = 3,
against either baseline).  multi:mixed:half:N does so on a pruned half-box plan (OFFT_HIP_OPT_HALF_MIXED, an N/2 box).
A spec with the prefix sum: measures offt_hip_execute_convolve_sum with K = 3 real filters and out = ins[0] against what a
caller does without it (three offt_hip_execute_convolve calls on the same plan and buffers plus two in-place torch adds) and
against the call's own generic route (a second plan made under the HIP backend with conv_pass_sum withheld, a seam of
tests/liboffthip_test.so, which the probe then loads instead of the product; not a public option).  The three ALTERNATE
after a warm-up, MIXED_REPS times each, and the line reports min and median of all three, the ratios against both, each
baseline's own spread (median / min - 1) and the byte model of DESIGN.md 4.5 (344 / 600 and 344 / 472 for K = 3).
sum:half:N does so on a pruned half-box plan (an N/2 box).
A spec with the prefix sum:mixed: measures OFFT_HIP_OPT_CONV_SUM_MIXED (the fused multi-input route at x lengths that are no
powers of two), with OFFT_HIP_OPT_CONV_MIXED on throughout, K = 3 real filters and out = ins[0]: the call with the option at 1
ALTERNATES with the call with the option at 0 (the generic route: the code of before the option existed) and with three
offt_hip_execute_convolve calls plus two in-place torch adds, on the same plan and buffers, MIXED_REPS times each after a
warm-up.  The line reports min and median of all three, the ratios against both baselines, each baseline's own spread
(median / min - 1) and the byte model of DESIGN.md 4.5 (344 / 472 and 344 / 600 for K = 3).  sum:mixed:half:N does so on a
pruned half-box plan (OFFT_HIP_OPT_HALF_MIXED, an N/2 box).
A spec with the prefix spec: measures offt_hip_execute_forward_filtered and offt_hip_execute_inverse_filtered (one output, a
buffer of its own; real filters), a line each, on the same plan and buffers: the fused route, the call's own generic route (a
second plan made under the HIP backend with filt_pass_fwd / filt_pass_inv withheld, a seam of tests/liboffthip_test.so) and
the caller's route built from calls that predate the two (offt_3d_execute + offt_hipk_pointwise; offt_hipk_pointwise_oop +
offt_3d_execute_dir(+1)).  The three ALTERNATE after a warm-up, MIXED_REPS times each, and a line reports min and median of
all three, the ratios against both, each baseline's own spread (median / min - 1) and the byte model of DESIGN.md 4.5
(104 / 136).  The fused side has OFFT_HIP_OPT_SPEC_FUSED and OFFT_HIP_OPT_SPEC_MIXED set, so an x length that is no power of
two (768, 1000) measures the mixed-radix filtered kernels.
A spec with the prefix shells: measures offt_hip_spectrum_shells (the power spectrum, every shell, with counts) on a plan's
output block filled with random numbers, next to the in-place REAL offt_hipk_pointwise sweep over the same block (40 B per
point in double precision against the call's 16 B).  The two ALTERNATE after a warm-up, MIXED_REPS times each, device time by
events on one stream; the line reports min and median of both, their ratio (the condition: below 1; the byte model: 0.4) and
the call's rate over the bytes it reads.
A spec with the prefix prod: measures offt_hip_execute_product (two spectra, out = the first) on one plan and the same buffers:
the fused route (OFFT_HIP_OPT_PROD_FUSED and, for prod:r2c:, OFFT_HIP_OPT_PROD_REAL set), the call's own generic route (a
second plan made under the HIP backend with prod_pass / prod_pass_real withheld, a seam of tests/liboffthip_test.so) and the
caller's route (two offt_3d_execute_dir(+1), a torch multiply, one offt_3d_execute).  The call consumes its inputs, so every
run starts from copies made outside the timed region.  The three ALTERNATE after a warm-up, MIXED_REPS times each, and the line
reports min and median of all three, the ratios against both, each baseline's own spread (median / min - 1) and the byte
model of DESIGN.md 4.5 (240 / 336 per point in f64, per half-spectrum point on an r2c plan: a model, not a measurement).
usage: conv_probe.py [mixed:|multi:|multi:mixed:|sum:|sum:mixed:|spec:|shells:|prod:][half:][f64|f32|r2c:]N ... [--zgroup-mib M]
       (default: 1024 f32:1024 r2c:512 mixed:768 mixed:f32:768 mixed:1000 mixed:f32:1000 mixed:half:768;
        the multi: set of profiles/conv_multi.txt: multi:512 multi:1024 multi:f32:1024 multi:r2c:512 multi:half:512;
        the multi:mixed: set of profiles/conv_multi_mixed.txt: multi:mixed:768 multi:mixed:f32:768 multi:mixed:1000
        multi:mixed:f32:1000 multi:mixed:half:768;
        the sum: set of profiles/conv_sum.txt: sum:512 sum:1024 sum:f32:1024 sum:r2c:512 sum:half:512, and for the shorter
        x lengths sum:64 sum:128 sum:256 sum:f32:256 sum:f32:512;
        the sum:mixed: set of profiles/conv_sum_mixed.txt: sum:mixed:768 sum:mixed:f32:768 sum:mixed:1000 sum:mixed:f32:1000
        sum:mixed:half:768;
        the spec: set of profiles/spec_filtered.txt: spec:512 spec:f32:512 spec:1024 spec:f32:1024 spec:r2c:512 spec:r2c:f32:512;
        the spec: set of profiles/spec_filtered_mixed.txt: spec:768 spec:f32:768 spec:1000 spec:f32:1000 spec:r2c:768;
        the shells: set of profiles/spectrum_shells.txt: shells:512 shells:f32:512 shells:r2c:512 shells:r2c:f32:512 shells:1024
        shells:f32:1024 shells:r2c:1024 shells:r2c:f32:1024;
        the prod: set of profiles/product.txt: prod:64 prod:128 prod:256 prod:512 prod:1024 prod:f32:1024 and the same with
        prod:r2c: (prod:r2c:64 ... prod:r2c:1024 prod:r2c:f32:1024))"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from offt_amd import api  # noqa: E402

if any((a.startswith("sum:") and not a.startswith("sum:mixed:")) or a.startswith("spec:") or a.startswith("prod:") for a in sys.argv[1:]):
    # the sum:, spec: and prod: specs time the generic route as well, which needs the build with the test seams (the same kernel objects)
    api.use_library(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "liboffthip_test.so"))
L = api.lib()
REPS = int(os.environ.get("CONV_PROBE_REPS", "5"))
MIXED_REPS = int(os.environ.get("CONV_PROBE_MIXED_REPS", "20"))
OPT_ZGROUP_MIB = 0  # include/offt_hip.h


def model(n, esz, r2c):
    """bytes of (a), (b), (c)"""
    if not r2c:
        v = 2 * esz * float(n) ** 3               # complex volume
        a = 6 * 2 * v
        mul = 2 * v + esz * float(n) ** 3
        return a, a + mul, 4 * 2 * v + mul
    h = n // 2 + 1
    vr, vh = esz * float(n) ** 3, 2 * esz * float(h) * n * n
    z = vr + vh                                   # one z pass: real rows one way, half spectrum the other
    a = 2 * z + 4 * 2 * vh
    mul = 2 * vh + esz * float(h) * n * n
    return a, a + mul, 2 * z + 2 * 2 * vh + mul


def probe_sum(rest, zg):
    """sum:[half:][f64|f32|r2c:]N -- offt_hip_execute_convolve_sum with K = 3 real filters and out = ins[0]"""
    K = 3
    half = rest.startswith("half:")
    kind, _, n_s = rest[(5 if half else 0):].rpartition(":")
    n = int(n_s)
    prec = api.F32 if kind == "f32" else api.F64
    r2c = kind == "r2c"
    T = api.lib()
    T.offt_hip_test_hip_backend_no_conv_sum.restype = C.c_void_p
    T.offt_hip_test_set_backend.argtypes = [C.c_void_p, C.c_int, C.c_int]
    plans = {}
    for name in ("generic", "sum"):  # the plan made under the table without conv_pass_sum first, then the product's own
        T.offt_hip_test_set_backend(T.offt_hip_test_hip_backend_no_conv_sum() if name == "generic" else None, 0, 1)
        po = plans[name] = api.offt_3d_init(n, n, n, precision=prec, is_r2c=int(r2c))
        if zg is not None:
            T.offt_hip_set_option(po, OPT_ZGROUP_MIB, zg)
        if half:
            api.offt_hip_set_half_box(po, True)
    po = plans["sum"]
    td = torch.float32 if prec == api.F32 else torch.float64
    ne = api.local_elems(po)
    ins = [torch.zeros(ne * 2, dtype=td, device="cuda") for _ in range(K)]
    for x in ins:
        T.offt_hip_fill_input(po, x.data_ptr(), 1)
    Hs = [torch.rand(ne, dtype=td, device="cuda") * (1.0 / (K * float(n) ** 3)) for _ in range(K)]  # keeps the field bounded
    ip, fp = [x.data_ptr() for x in ins], [h.data_ptr() for h in Hs]
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def run(fn):
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e-3

    def base():  # what a caller does without the call: K convolves and K - 1 add sweeps of their own
        for x, h in zip(ip, fp):
            api.offt_hip_execute_convolve(po, x, h, api.FILTER_REAL)
        for x in ins[1:]:
            ins[0].add_(x)

    def sm():
        api.offt_hip_execute_convolve_sum(po, ip, fp, ip[0], api.FILTER_REAL)

    def gen():
        api.offt_hip_execute_convolve_sum(plans["generic"], ip, fp, ip[0], api.FILTER_REAL)

    t = {"sum": [], "base": [], "generic": []}
    for rep_i in range(2 + MIXED_REPS):
        for name, fn in (("sum", sm), ("base", base), ("generic", gen)):
            dt = run(fn)
            if rep_i >= 2:
                t[name].append(dt)
    mn, md = {k: min(v) for k, v in t.items()}, {k: float(np.median(v)) for k, v in t.items()}
    fused1, fusedk, fusedg = api.offt_hip_convolve_fused(po), api.offt_hip_convolve_sum_fused(po), api.offt_hip_convolve_sum_fused(plans["generic"])
    tag = f"{'r2c f64' if r2c else ('f32' if prec == api.F32 else 'f64')} {n}^3 K={K}"
    if half:
        tag += f" half box {n // 2}^3 [{'pruned' if api.offt_hip_half_box_pruned(po) else 'fallback'}]"
    # bytes per point, f64, complex plan, full lines: baseline 168 K + 48 (K - 1), generic 120 K + 112, fused 88 K + 80
    mb, mg, mf = 168 * K + 48 * (K - 1), 120 * K + 112, 88 * K + 80
    print(f"sum: {tag}: sum [{'fused' if fusedk else 'generic'}] min {mn['sum'] * 1e3:.3f} ms median {md['sum'] * 1e3:.3f} ms  "
          f"{K} calls + {K - 1} adds [{'fused' if fused1 else 'unfused'}] min {mn['base'] * 1e3:.3f} ms median {md['base'] * 1e3:.3f} ms  "
          f"sum without conv_pass_sum [{'fused' if fusedg else 'generic'}] min {mn['generic'] * 1e3:.3f} ms median {md['generic'] * 1e3:.3f} ms  "
          f"sum/base min {mn['sum'] / mn['base']:.3f} median {md['sum'] / md['base']:.3f}  "
          f"sum/generic min {mn['sum'] / mn['generic']:.3f} median {md['sum'] / md['generic']:.3f}  "
          f"base spread {md['base'] / mn['base'] - 1:.3f}  generic spread {md['generic'] / mn['generic'] - 1:.3f}  "
          f"byte model (complex, full lines) fused/base {mf / mb:.3f} fused/generic {mf / mg:.3f} generic/base {mg / mb:.3f}  "
          f"n {MIXED_REPS}  zgroup_mib {T.offt_hip_get_option(po, OPT_ZGROUP_MIB)}", flush=True)
    for p in plans.values():
        api.offt_3d_fin(p)
    del ins, Hs
    torch.cuda.empty_cache()


def probe_spec(rest, zg):
    """spec:[r2c:][f64|f32:]N -- the filtered forward and the filtered inverse (one output), three routes each"""
    r2c = rest.startswith("r2c:")
    kind, _, n_s = rest[(4 if r2c else 0):].rpartition(":")
    n = int(n_s)
    prec = api.F32 if kind == "f32" else api.F64
    T = api.lib()
    T.offt_hip_test_hip_backend_no_filt.restype = C.c_void_p
    T.offt_hip_test_set_backend.argtypes = [C.c_void_p, C.c_int, C.c_int]
    V, I, LL = C.c_void_p, C.c_int, C.c_longlong
    T.offt_hipk_pointwise.argtypes = [V, V, I, I, I, I, I, LL, LL, LL, V]
    T.offt_hipk_pointwise_oop.argtypes = [V, V, V, I, I, I, I, I, LL, LL, LL, V]
    plans = {}
    for name in ("generic", "fused"):  # the plan made under the table without the two entries first, then the product's own
        T.offt_hip_test_set_backend(T.offt_hip_test_hip_backend_no_filt() if name == "generic" else None, 0, 1)
        po = plans[name] = api.offt_3d_init(n, n, n, precision=prec, is_r2c=int(r2c))
        if zg is not None:
            T.offt_hip_set_option(po, OPT_ZGROUP_MIB, zg)
    po = plans["fused"]
    T.offt_hip_set_option(po, api.OPT_SPEC_FUSED, 1)
    T.offt_hip_set_option(po, api.OPT_SPEC_MIXED, 1)  # (an x length that is no power of two; a power of two does not read it)
    stream = torch.cuda.Stream()  # one stream for both plans, the caller's multiply and the timing events
    for p in plans.values():
        T.offt_hip_set_stream(p, stream.cuda_stream)
    td = torch.float32 if prec == api.F32 else torch.float64
    ne = api.local_elems(po)
    c = api.comm_dict(po)
    osz, ost = c["osize"], c["ostride"]
    x = torch.zeros(ne * 2, dtype=td, device="cuda")
    T.offt_hip_fill_input(po, x.data_ptr(), 1)
    spec = x.clone()
    api.offt_3d_execute(po, spec.data_ptr(), spec.data_ptr())
    out = torch.zeros_like(x)
    H = torch.rand(ne, dtype=td, device="cuda") * float(n) ** -1.5  # keeps a field that is transformed again and again bounded
    px, ps, pout, ph = x.data_ptr(), spec.data_ptr(), out.data_ptr(), H.data_ptr()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def run(fn):
        ev[0].record(stream)
        fn()
        ev[1].record(stream)
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e-3

    def point(src, dst):
        sp = stream.cuda_stream
        if src == dst:
            rc = T.offt_hipk_pointwise(dst, ph, prec, api.FILTER_REAL, osz[0], osz[1], osz[2], ost[0], ost[1], ost[2], sp)
        else:
            rc = T.offt_hipk_pointwise_oop(src, dst, ph, prec, api.FILTER_REAL, osz[0], osz[1], osz[2], ost[0], ost[1], ost[2], sp)
        assert rc == 0

    def caller_fwd():
        api.offt_3d_execute(po, px, px)
        point(px, px)

    def caller_inv():
        point(ps, pout)
        api.offt_3d_execute_dir(po, pout, pout, +1)

    routes = {
        "fwd": (("fused", lambda: api.offt_hip_execute_forward_filtered(po, px, ph, api.FILTER_REAL)),
                ("generic", lambda: api.offt_hip_execute_forward_filtered(plans["generic"], px, ph, api.FILTER_REAL)),
                ("caller", caller_fwd)),
        "inv": (("fused", lambda: api.offt_hip_execute_inverse_filtered(po, ps, [pout], [ph], api.FILTER_REAL)),
                ("generic", lambda: api.offt_hip_execute_inverse_filtered(plans["generic"], ps, [pout], [ph], api.FILTER_REAL)),
                ("caller", caller_inv)),
    }
    fusedp, fusedg = api.offt_hip_spectral_fused(po), api.offt_hip_spectral_fused(plans["generic"])
    tag = f"{'r2c ' if r2c else ''}{'f32' if prec == api.F32 else 'f64'} {n}^3"
    for which, rs in routes.items():
        t = {k: [] for k, _ in rs}
        for rep_i in range(2 + MIXED_REPS):
            for name, fn in rs:
                dt = run(fn)
                if rep_i >= 2:
                    t[name].append(dt)
        mn, md = {k: min(v) for k, v in t.items()}, {k: float(np.median(v)) for k, v in t.items()}
        print(f"spec: {which} {tag}: call [{'fused' if fusedp else 'generic'}] min {mn['fused'] * 1e3:.3f} ms median {md['fused'] * 1e3:.3f} ms  "
              f"call without filt_pass [{'fused' if fusedg else 'generic'}] min {mn['generic'] * 1e3:.3f} ms median {md['generic'] * 1e3:.3f} ms  "
              f"caller's route min {mn['caller'] * 1e3:.3f} ms median {md['caller'] * 1e3:.3f} ms  "
              f"fused/generic min {mn['fused'] / mn['generic']:.3f} median {md['fused'] / md['generic']:.3f}  "
              f"fused/caller min {mn['fused'] / mn['caller']:.3f} median {md['fused'] / md['caller']:.3f}  "
              f"generic spread {md['generic'] / mn['generic'] - 1:.3f}  caller spread {md['caller'] / mn['caller'] - 1:.3f}  "
              f"byte model (complex f64, real filter) {104 / 136:.3f}  n {MIXED_REPS}  zgroup_mib {T.offt_hip_get_option(po, OPT_ZGROUP_MIB)}",
              flush=True)
    for p in plans.values():
        api.offt_3d_fin(p)
    del x, spec, out, H
    torch.cuda.empty_cache()


def probe_prod(rest, zg):
    """prod:[r2c:][f64|f32:]N -- offt_hip_execute_product (two spectra, out = the first), three routes on the same buffers"""
    r2c = rest.startswith("r2c:")
    kind, _, n_s = rest[(4 if r2c else 0):].rpartition(":")
    n = int(n_s)
    prec = api.F32 if kind == "f32" else api.F64
    T = api.lib()
    T.offt_hip_test_hip_backend_no_prod.restype = C.c_void_p
    T.offt_hip_test_set_backend.argtypes = [C.c_void_p, C.c_int, C.c_int]
    plans = {}
    for name in ("generic", "fused"):  # the plan made under the table without the fused launches first, then the product's own
        T.offt_hip_test_set_backend(T.offt_hip_test_hip_backend_no_prod() if name == "generic" else None, 0, 1)
        po = plans[name] = api.offt_3d_init(n, n, n, precision=prec, is_r2c=int(r2c))
        if zg is not None:
            T.offt_hip_set_option(po, OPT_ZGROUP_MIB, zg)
        T.offt_hip_set_option(po, api.OPT_PROD_FUSED, 1)
        T.offt_hip_set_option(po, api.OPT_PROD_REAL, 1)  # (a complex plan does not read it)
    po = plans["fused"]
    stream = torch.cuda.Stream()  # one stream for both plans, the caller's multiply, the copies and the timing events
    for p in plans.values():
        T.offt_hip_set_stream(p, stream.cuda_stream)
    td = torch.float32 if prec == api.F32 else torch.float64
    ne = api.local_elems(po)
    with torch.cuda.stream(stream):
        # the spectra of two random fields, kept aside: the call consumes its inputs, so every timed run starts from a copy
        # (made outside the timed region)
        a0 = torch.zeros(ne * 2, dtype=td, device="cuda")
        T.offt_hip_fill_input(po, a0.data_ptr(), 1)
        api.offt_3d_execute(po, a0.data_ptr(), a0.data_ptr())
        b0 = a0 * 0.5
        a, b = a0.clone(), b0.clone()
    pa, pb = a.data_ptr(), b.data_ptr()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def run(fn):
        with torch.cuda.stream(stream):
            a.copy_(a0)
            b.copy_(b0)
            ev[0].record(stream)
            fn()
            ev[1].record(stream)
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e-3

    def caller():  # without the call: two inverses, a multiply of the caller's own, one forward
        api.offt_3d_execute_dir(po, pa, pa, +1)
        api.offt_3d_execute_dir(po, pb, pb, +1)
        if r2c:  # real rows (with their two padding scalars a row: (n + 2) / n of the field)
            a.mul_(b)
        else:
            torch.view_as_complex(a.view(-1, 2)).mul_(torch.view_as_complex(b.view(-1, 2)))
        api.offt_3d_execute(po, pa, pa)

    rs = (("fused", lambda: api.offt_hip_execute_product(po, pa, pb, pa)),
          ("generic", lambda: api.offt_hip_execute_product(plans["generic"], pa, pb, pa)),
          ("caller", caller))
    fusedp, fusedg = api.offt_hip_product_fused(po), api.offt_hip_product_fused(plans["generic"])
    t = {k: [] for k, _ in rs}
    for rep_i in range(2 + MIXED_REPS):
        for name, fn in rs:
            dt = run(fn)
            if rep_i >= 2:
                t[name].append(dt)
    mn, md = {k: min(v) for k, v in t.items()}, {k: float(np.median(v)) for k, v in t.items()}
    tag = f"{'r2c ' if r2c else ''}{'f32' if prec == api.F32 else 'f64'} {n}^3"
    # bytes per point (per half-spectrum point on an r2c plan), f64: a MODEL, not a measurement
    print(f"prod: {tag}: call [{'fused' if fusedp else 'generic'}] min {mn['fused'] * 1e3:.3f} ms median {md['fused'] * 1e3:.3f} ms  "
          f"call without prod_pass [{'fused' if fusedg else 'generic'}] min {mn['generic'] * 1e3:.3f} ms median {md['generic'] * 1e3:.3f} ms  "
          f"caller's route min {mn['caller'] * 1e3:.3f} ms median {md['caller'] * 1e3:.3f} ms  "
          f"fused/generic min {mn['fused'] / mn['generic']:.3f} median {md['fused'] / md['generic']:.3f}  "
          f"fused/caller min {mn['fused'] / mn['caller']:.3f} median {md['fused'] / md['caller']:.3f}  "
          f"generic spread {md['generic'] / mn['generic'] - 1:.3f}  caller spread {md['caller'] / mn['caller'] - 1:.3f}  "
          f"byte model (f64, 240 / 336 B per point) {240 / 336:.3f}  n {MIXED_REPS}  zgroup_mib {T.offt_hip_get_option(po, OPT_ZGROUP_MIB)}",
          flush=True)
    for p in plans.values():
        api.offt_3d_fin(p)
    del a, b, a0, b0
    torch.cuda.empty_cache()


def probe_shells(rest):
    """shells:[r2c:][f64|f32:]N -- offt_hip_spectrum_shells next to the in-place real pointwise sweep over the same block"""
    r2c = rest.startswith("r2c:")
    kind, _, n_s = rest[(4 if r2c else 0):].rpartition(":")
    n = int(n_s)
    prec = api.F32 if kind == "f32" else api.F64
    V, I, LL = C.c_void_p, C.c_int, C.c_longlong
    L.offt_hipk_pointwise.argtypes = [V, V, I, I, I, I, I, LL, LL, LL, V]
    po = api.offt_3d_init(n, n, n, precision=prec, is_r2c=int(r2c))
    stream = torch.cuda.Stream()
    L.offt_hip_set_stream(po, stream.cuda_stream)
    td = torch.float32 if prec == api.F32 else torch.float64
    ne = api.local_elems(po)
    c = api.comm_dict(po)
    osz, ost = c["osize"], c["ostride"]
    a = torch.randn(ne * 2, dtype=td, device="cuda")
    H = torch.ones(ne, dtype=td, device="cuda")
    nb = int(np.rint(np.sqrt(3.0) * (n // 2))) + 1
    sums = torch.zeros(nb, dtype=torch.float64, device="cuda")
    cnt = torch.zeros(nb, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def run(fn):
        ev[0].record(stream)
        fn()
        ev[1].record(stream)
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e-3

    def point():
        assert L.offt_hipk_pointwise(a.data_ptr(), H.data_ptr(), prec, api.FILTER_REAL, osz[0], osz[1], osz[2], ost[0], ost[1], ost[2],
                                     stream.cuda_stream) == 0

    rs = (("shells", lambda: api.offt_hip_spectrum_shells(po, a.data_ptr(), None, nb, sums.data_ptr(), cnt.data_ptr())), ("pointwise", point))
    t = {k: [] for k, _ in rs}
    for rep_i in range(2 + MIXED_REPS):
        for name, fn in rs:
            dt = run(fn)
            if rep_i >= 2:
                t[name].append(dt)
    assert int(cnt.sum()) == n ** 3
    mn, md = {k: min(v) for k, v in t.items()}, {k: float(np.median(v)) for k, v in t.items()}
    esz = 4 if prec == api.F32 else 8
    read = 2.0 * esz * osz[0] * osz[1] * osz[2]
    print(f"shells: {'r2c ' if r2c else ''}{'f32' if prec == api.F32 else 'f64'} {n}^3: call min {mn['shells'] * 1e3:.3f} ms median {md['shells'] * 1e3:.3f} ms "
          f"({read / mn['shells'] / 1e9:.0f} GB/s read)  pointwise (in place, real) min {mn['pointwise'] * 1e3:.3f} ms median {md['pointwise'] * 1e3:.3f} ms  "
          f"call/pointwise min {mn['shells'] / mn['pointwise']:.3f} median {md['shells'] / md['pointwise']:.3f}  "
          f"pointwise spread {md['pointwise'] / mn['pointwise'] - 1:.3f}  byte model {16 / 40:.3f}  bins {nb}  n {MIXED_REPS}", flush=True)
    api.offt_3d_fin(po)
    del a, H
    torch.cuda.empty_cache()


def probe_sum_mixed(rest, zg):
    """sum:mixed:[half:][f64|f32|r2c:]N -- OFFT_HIP_OPT_CONV_SUM_MIXED at 1 and at 0 and the caller's route, on one plan"""
    K = 3
    half = rest.startswith("half:")
    kind, _, n_s = rest[(5 if half else 0):].rpartition(":")
    n = int(n_s)
    prec = api.F32 if kind == "f32" else api.F64
    r2c = kind == "r2c"
    po = api.offt_3d_init(n, n, n, precision=prec, is_r2c=int(r2c))
    if zg is not None:
        L.offt_hip_set_option(po, OPT_ZGROUP_MIB, zg)
    L.offt_hip_set_option(po, api.OPT_CONV_MIXED, 1)
    if half:
        L.offt_hip_set_option(po, api.OPT_HALF_MIXED, 1)
        api.offt_hip_set_half_box(po, True)
    td = torch.float32 if prec == api.F32 else torch.float64
    ne = api.local_elems(po)
    ins = [torch.zeros(ne * 2, dtype=td, device="cuda") for _ in range(K)]
    for x in ins:
        L.offt_hip_fill_input(po, x.data_ptr(), 1)
    Hs = [torch.rand(ne, dtype=td, device="cuda") * (1.0 / (K * float(n) ** 3)) for _ in range(K)]  # keeps the field bounded
    ip, fp = [x.data_ptr() for x in ins], [h.data_ptr() for h in Hs]
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def run(fn):
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e-3

    def base():  # what a caller does without the call: K convolves and K - 1 add sweeps of their own
        for x, h in zip(ip, fp):
            api.offt_hip_execute_convolve(po, x, h, api.FILTER_REAL)
        for x in ins[1:]:
            ins[0].add_(x)

    def sm():
        api.offt_hip_execute_convolve_sum(po, ip, fp, ip[0], api.FILTER_REAL)

    t = {"on": [], "off": [], "base": []}
    route = {}
    for rep_i in range(2 + MIXED_REPS):
        for name, fn, v in (("on", sm, 1), ("off", sm, 0), ("base", base, 1)):
            L.offt_hip_set_option(po, api.OPT_CONV_SUM_MIXED, v)  # (outside the timed region)
            route[name] = api.offt_hip_convolve_sum_fused(po)
            dt = run(fn)
            if rep_i >= 2:
                t[name].append(dt)
    L.offt_hip_set_option(po, api.OPT_CONV_SUM_MIXED, 0)
    mn, md = {k: min(v) for k, v in t.items()}, {k: float(np.median(v)) for k, v in t.items()}
    fused1 = api.offt_hip_convolve_fused(po)
    tag = f"{'r2c f64' if r2c else ('f32' if prec == api.F32 else 'f64')} {n}^3 K={K}"
    if half:
        tag += f" half box {n // 2}^3 [{'pruned' if api.offt_hip_half_box_pruned(po) else 'fallback'}]"
    # bytes per point, f64, complex plan, full lines: baseline 168 K + 48 (K - 1), generic 120 K + 112, fused 88 K + 80
    mb, mg, mf = 168 * K + 48 * (K - 1), 120 * K + 112, 88 * K + 80
    print(f"sum:mixed: {tag}: option 1 [{'fused' if route['on'] else 'generic'}] min {mn['on'] * 1e3:.3f} ms median {md['on'] * 1e3:.3f} ms  "
          f"option 0 [{'fused' if route['off'] else 'generic'}] min {mn['off'] * 1e3:.3f} ms median {md['off'] * 1e3:.3f} ms  "
          f"{K} calls + {K - 1} adds [{'fused' if fused1 else 'unfused'}] min {mn['base'] * 1e3:.3f} ms median {md['base'] * 1e3:.3f} ms  "
          f"1/0 min {mn['on'] / mn['off']:.3f} median {md['on'] / md['off']:.3f}  "
          f"1/base min {mn['on'] / mn['base']:.3f} median {md['on'] / md['base']:.3f}  "
          f"option-0 spread {md['off'] / mn['off'] - 1:.3f}  base spread {md['base'] / mn['base'] - 1:.3f}  "
          f"byte model (complex, full lines) fused/generic {mf / mg:.3f} fused/base {mf / mb:.3f}  "
          f"n {MIXED_REPS}  zgroup_mib {L.offt_hip_get_option(po, OPT_ZGROUP_MIB)}", flush=True)
    api.offt_3d_fin(po)
    del ins, Hs
    torch.cuda.empty_cache()


def main():
    args = sys.argv[1:]
    zg = None
    if "--zgroup-mib" in args:
        i = args.index("--zgroup-mib")
        zg = int(args[i + 1])
        del args[i:i + 2]
    specs = args or ["1024", "f32:1024", "r2c:512", "mixed:768", "mixed:f32:768", "mixed:1000", "mixed:f32:1000", "mixed:half:768"]
    torch.cuda.set_device(0)
    for spec in specs:
        if spec.startswith("spec:"):
            probe_spec(spec[5:], zg)
            continue
        if spec.startswith("shells:"):
            probe_shells(spec[7:])
            continue
        if spec.startswith("prod:"):
            probe_prod(spec[5:], zg)
            continue
        if spec.startswith("sum:mixed:"):
            probe_sum_mixed(spec[10:], zg)
            continue
        if spec.startswith("sum:"):
            probe_sum(spec[4:], zg)
            continue
        multi = spec.startswith("multi:")
        mixed = spec.startswith("mixed:") or multi  # (the same grammar behind the prefix)
        multi_mixed = multi and spec[6:].startswith("mixed:")
        rest = spec[(6 if mixed else 0) + (6 if multi_mixed else 0):]
        half = mixed and rest.startswith("half:")
        kind, _, n_s = rest[(5 if half else 0):].rpartition(":")
        n = int(n_s)
        prec = api.F32 if kind == "f32" else api.F64
        r2c = kind == "r2c"
        po = api.offt_3d_init(n, n, n, precision=prec, is_r2c=int(r2c))
        if zg is not None:
            L.offt_hip_set_option(po, OPT_ZGROUP_MIB, zg)
        c = api.comm_dict(po)
        td = torch.float32 if prec == api.F32 else torch.float64
        esz = 4 if prec == api.F32 else 8
        dev = torch.zeros(api.local_elems(po) * 2, dtype=td, device="cuda")
        L.offt_hip_fill_input(po, dev.data_ptr(), 1)
        H = torch.rand(api.local_elems(po), dtype=td, device="cuda") * (1.0 / float(n) ** 3)  # keeps the field bounded
        o = c["ostride"]
        osz = tuple(c["osize"])
        spec_v = torch.as_strided(dev, osz + (2,), (2 * o[0], 2 * o[1], 2 * o[2], 1))
        hv = torch.as_strided(H, osz + (1,), (o[0], o[1], o[2], 0))
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

        def run(fn):
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            return ev[0].elapsed_time(ev[1]) * 1e-3

        def a():
            api.offt_3d_execute(po, dev.data_ptr(), dev.data_ptr())
            L.offt_hip_set_output_scale(po, 1.0 / float(n) ** 3)
            api.offt_3d_execute_dir(po, dev.data_ptr(), dev.data_ptr(), +1)
            L.offt_hip_set_output_scale(po, 1.0)

        def b():
            api.offt_3d_execute(po, dev.data_ptr(), dev.data_ptr())
            spec_v.mul_(hv)
            api.offt_3d_execute_dir(po, dev.data_ptr(), dev.data_ptr(), +1)

        def cv():
            api.offt_hip_execute_convolve(po, dev.data_ptr(), H.data_ptr(), api.FILTER_REAL)

        if multi:
            K = 3
            if multi_mixed:
                L.offt_hip_set_option(po, api.OPT_CONV_MIXED, 1)
                if half:
                    L.offt_hip_set_option(po, api.OPT_HALF_MIXED, 1)
            if half:
                api.offt_hip_set_half_box(po, True)
            Hs = [H] + [torch.rand(api.local_elems(po), dtype=td, device="cuda") * (1.0 / float(n) ** 3) for _ in range(K - 1)]
            outs = [torch.zeros_like(dev) for _ in range(K - 1)] + [dev]
            op, fp = [o_.data_ptr() for o_ in outs], [h_.data_ptr() for h_ in Hs]

            def mv():
                api.offt_hip_execute_convolve_multi(po, dev.data_ptr(), op, fp, api.FILTER_REAL)

            def three():
                for h_ in Hs:
                    api.offt_hip_execute_convolve(po, dev.data_ptr(), h_.data_ptr(), api.FILTER_REAL)

            if multi_mixed:
                # the same plan and buffers; the option is set outside the timed region
                def opt(v):
                    L.offt_hip_set_option(po, api.OPT_CONV_MULTI_MIXED, v)

                t = {"on": [], "three": [], "off": []}
                route = {}
                for rep_i in range(2 + MIXED_REPS):
                    for name, fn, v in (("on", mv, 1), ("three", three, 1), ("off", mv, 0)):
                        opt(v)
                        route[name] = api.offt_hip_convolve_multi_fused(po)
                        dt = run(fn)
                        if rep_i >= 2:
                            t[name].append(dt)
                opt(0)
                mn, md = {k: min(v) for k, v in t.items()}, {k: float(np.median(v)) for k, v in t.items()}
                fused1 = api.offt_hip_convolve_fused(po)
                tag = f"{'r2c f64' if r2c else ('f32' if prec == api.F32 else 'f64')} {n}^3 K={K}"
                if half:
                    tag += f" half box {n // 2}^3 [{'pruned' if api.offt_hip_half_box_pruned(po) else 'fallback'}]"
                print(f"multi:mixed: {tag}: option 1 [{'fused' if route['on'] else 'generic'}] min {mn['on'] * 1e3:.3f} ms median {md['on'] * 1e3:.3f} ms  "
                      f"three calls [{'fused' if fused1 else 'unfused'}] min {mn['three'] * 1e3:.3f} ms median {md['three'] * 1e3:.3f} ms  "
                      f"option 0 [{'fused' if route['off'] else 'generic'}] min {mn['off'] * 1e3:.3f} ms median {md['off'] * 1e3:.3f} ms  "
                      f"1/three min {mn['on'] / mn['three']:.3f} median {md['on'] / md['three']:.3f}  "
                      f"1/0 min {mn['on'] / mn['off']:.3f} median {md['on'] / md['off']:.3f}  "
                      f"three-calls spread {md['three'] / mn['three'] - 1:.3f}  option-0 spread {md['off'] / mn['off'] - 1:.3f}  "
                      f"byte model (complex, full lines) {(8 + 13 * K) / (21.0 * K):.3f}  n {MIXED_REPS}  "
                      f"zgroup_mib {L.offt_hip_get_option(po, OPT_ZGROUP_MIB)}", flush=True)
                api.offt_3d_fin(po)
                del dev, H, Hs, outs, spec_v, hv
                torch.cuda.empty_cache()
                continue
            t = {"multi": [], "three": []}
            for rep_i in range(2 + MIXED_REPS):
                for name, fn in (("multi", mv), ("three", three)):
                    dt = run(fn)
                    if rep_i >= 2:
                        t[name].append(dt)
            mn, md = {k: min(v) for k, v in t.items()}, {k: float(np.median(v)) for k, v in t.items()}
            fused1, fusedk = api.offt_hip_convolve_fused(po), api.offt_hip_convolve_multi_fused(po)
            # bytes per point in units of esz (f64: x 8), complex plan, full lines: K fused calls 168 K / 8, the fused multi
            # route (64 + 104 K) / 8; unfused 232 K / 8 against (96 + 136 K) / 8
            byte_model = (8 + 13 * K) / (21.0 * K) if fusedk else (12 + 17 * K) / (29.0 * K)
            tag = f"{'r2c f64' if r2c else ('f32' if prec == api.F32 else 'f64')} {n}^3 K={K}"
            if half:
                tag += f" half box {n // 2}^3 [{'pruned' if api.offt_hip_half_box_pruned(po) else 'fallback'}]"
            print(f"multi: {tag}: multi [{'fused' if fusedk else 'generic'}] min {mn['multi'] * 1e3:.3f} ms median {md['multi'] * 1e3:.3f} ms  "
                  f"three calls [{'fused' if fused1 else 'unfused'}] min {mn['three'] * 1e3:.3f} ms median {md['three'] * 1e3:.3f} ms  "
                  f"multi/three min {mn['multi'] / mn['three']:.3f} median {md['multi'] / md['three']:.3f}  "
                  f"three-calls spread {md['three'] / mn['three'] - 1:.3f}  byte model (complex, full lines) {byte_model:.3f}  "
                  f"n {MIXED_REPS}  zgroup_mib {L.offt_hip_get_option(po, OPT_ZGROUP_MIB)}", flush=True)
            api.offt_3d_fin(po)
            del dev, H, Hs, outs, spec_v, hv
            torch.cuda.empty_cache()
            continue
        if mixed:
            # the same plan and buffers, the option alternating between 1 and 0 (set outside the timed region)
            if half:
                L.offt_hip_set_option(po, api.OPT_HALF_MIXED, 1)
                api.offt_hip_set_half_box(po, True)
            t = {1: [], 0: []}
            fused = {}
            for rep_i in range(2 + MIXED_REPS):
                for on in (1, 0):
                    L.offt_hip_set_option(po, api.OPT_CONV_MIXED, on)
                    fused[on] = api.offt_hip_convolve_fused(po)
                    dt = run(cv)
                    if rep_i >= 2:
                        t[on].append(dt)
            _, mb, mc = model(n, esz, r2c)
            mn, md = {k: min(v) for k, v in t.items()}, {k: float(np.median(v)) for k, v in t.items()}
            tag = f"{'r2c f64' if r2c else ('f32' if prec == api.F32 else 'f64')} {n}^3"
            if half:
                tag += f" half box {n // 2}^3 [{'pruned' if api.offt_hip_half_box_pruned(po) else 'fallback'}]"
            print(f"mixed: {tag}: option 1 [{'fused' if fused[1] else 'unfused'}] min {mn[1] * 1e3:.3f} ms median {md[1] * 1e3:.3f} ms  "
                  f"option 0 [{'fused' if fused[0] else 'unfused'}] min {mn[0] * 1e3:.3f} ms median {md[0] * 1e3:.3f} ms  "
                  f"1/0 min {mn[1] / mn[0]:.3f} median {md[1] / md[0]:.3f}  option-0 spread {md[0] / mn[0] - 1:.3f}  "
                  f"byte model (full lines) {mc / mb:.3f}  n {MIXED_REPS}", flush=True)
            api.offt_3d_fin(po)
            del dev, H, spec_v, hv
            torch.cuda.empty_cache()
            continue
        for _ in range(2):
            a(); b(); cv()
        best = [1e30, 1e30, 1e30]
        for _ in range(REPS):
            for i, fn in enumerate((a, b, cv)):
                best[i] = min(best[i], run(fn))
        ma, mb, mc = model(n, esz, r2c)
        tag = f"{'r2c f64' if r2c else ('f32' if prec == api.F32 else 'f64')} {n}^3"
        fused = api.offt_hip_convolve_fused(po)
        print(f"{tag}: (a) fwd+inv {best[0] * 1e3:.3f} ms ({ma / best[0] / 1e9:.0f} GB/s model)  "
              f"(b) caller's route {best[1] * 1e3:.3f} ms ({mb / best[1] / 1e9:.0f} GB/s)  "
              f"(c) convolve[{'fused' if fused else 'unfused'}] {best[2] * 1e3:.3f} ms ({mc / best[2] / 1e9:.0f} GB/s)  "
              f"c/b {best[2] / best[1]:.3f}  c/a {best[2] / best[0]:.3f}  zgroup_mib {L.offt_hip_get_option(po, OPT_ZGROUP_MIB)}",
              flush=True)
        api.offt_3d_fin(po)
        del dev, H, spec_v, hv
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
