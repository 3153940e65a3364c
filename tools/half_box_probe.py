#!/usr/bin/env python3
"""Developer probe: half-box plans (offt_hip_set_half_box) against what a caller does without the option -- clear the
padding (the 7/8 of the volume outside the box, three torch fills of exactly those bytes on the stream), then the ordinary
execute.  Forward, inverse and convolve (real filter), one plan per size and precision, the option switched on and off
between runs so that both routes see the same box state.  After a warm-up each is timed RUNS times with events on the
stream; min and median are reported, the baseline's own spread ((median - min) / min) beside the ratio, and the achieved
bytes per second of the option-on run against its byte model:
  forward / inverse   (1/8 + 1/4 + 1/4 + 1/2 + 1/2 + 1) = 2.625 sweeps over the complex volume (the full transform makes 6)
  convolve            z 3/8, y 3/4, fused x 1 (half in, half out), y 3/4, z 3/8 = 3.25 sweeps, plus the filter once
Real-input plans (r2c:): the half box stays on and OFFT_HIP_OPT_HALF_R2C is switched between 1 (the passes skip the
padding) and 0 (the library clears the padding of the real rows and runs the ordinary schedule: what a caller gets without
the option).  The models are the same numbers of sweeps, over the half-spectrum volume Nx Ny (Nz/2+1) complex elements --
the real field has as many bytes, its box is 1/8 of a sweep; the baseline makes 6 sweeps and its clear writes 7/8 of one.
Mixed-radix lengths (mixed:): likewise the half box stays on and OFFT_HIP_OPT_HALF_MIXED is switched between 1 and 0.
Their x pass has no fused convolve kernel: the convolve is the pruned forward, a multiply (the spectrum read and written,
the filter read) and the pruned inverse, 2.625 + 2 + 2.625 = 7.25 sweeps plus the filter.
Real-input plans at mixed-radix lengths (r2c:mixed:): the half box, OFFT_HIP_OPT_HALF_R2C and OFFT_HIP_OPT_HALF_MIXED stay on
and OFFT_HIP_OPT_HALF_R2C_MIXED is switched between 1 and 0 on the same plan and buffers; the models are those of the two
kinds together (sweeps over the half-spectrum volume, the unfused convolve).
usage: half_box_probe.py [r2c:][mixed:][f64|f32:]N ... [--runs R] [--out FILE]
       (default: 512 f32:512 1024 f32:1024 r2c:512 r2c:f32:512 r2c:1024 r2c:f32:1024;
        the mixed-radix lines: mixed:768 mixed:f32:768 mixed:1000 mixed:f32:1000
                               r2c:mixed:768 r2c:mixed:f32:768 r2c:mixed:1000 r2c:mixed:f32:1000)"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from offt_amd import api  # noqa: E402

L = api.lib()


def main():
    args = sys.argv[1:]
    runs, out = 20, None
    if "--runs" in args:
        i = args.index("--runs")
        runs = int(args[i + 1])
        del args[i:i + 2]
    if "--out" in args:
        i = args.index("--out")
        out = open(args[i + 1], "a")
        del args[i:i + 2]
    specs = args or ["512", "f32:512", "1024", "f32:1024", "r2c:512", "r2c:f32:512", "r2c:1024", "r2c:f32:1024"]
    torch.cuda.set_device(0)

    def emit(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for spec in specs:
        *kinds, n_s = spec.split(":")
        n = int(n_s)
        r2c = "r2c" in kinds
        mixed = "mixed" in kinds
        opt = r2c or mixed   # the baseline is the library's own fallback: the half box on, the route's option off
        prec = api.F32 if "f32" in kinds else api.F64
        td = torch.float32 if prec == api.F32 else torch.float64
        esz = 4 if prec == api.F32 else 8
        po = api.offt_3d_init(n, n, n, precision=prec, is_r2c=int(r2c))
        c = api.comm_dict(po)
        dev = torch.zeros(api.local_elems(po) * 2, dtype=td, device="cuda")
        H = torch.rand(api.local_elems(po), dtype=td, device="cuda") * (1.0 / float(n) ** 3)
        s = c["istride"]
        if r2c:   # the real rows: scalar strides
            vol = torch.as_strided(dev, (n, n, n), (2 * s[0], 2 * s[1], 1))
        else:
            vol = torch.as_strided(dev, (n, n, n, 2), (2 * s[0], 2 * s[1], 2 * s[2], 1))
        h = n // 2
        vol[:h, :h, :h].uniform_(-1.0, 1.0)
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        p = dev.data_ptr()

        def clear():
            vol[h:].zero_()
            vol[:h, h:].zero_()
            vol[:h, :h, h:].zero_()

        def fwd(on):
            if not on and not opt:
                clear()
            api.offt_3d_execute_dir(po, p, p, -1)

        def inv(on):
            api.offt_3d_execute_dir(po, p, p, +1)

        def conv(on):
            if not on and not opt:
                clear()
            api.offt_hip_execute_convolve(po, p, H.data_ptr(), api.FILTER_REAL)

        def route(on):
            if r2c and mixed:
                assert L.offt_hip_set_option(po, api.OPT_HALF_R2C_MIXED, 1 if on else 0) == 0
            elif r2c:
                assert L.offt_hip_set_option(po, api.OPT_HALF_R2C, 1 if on else 0) == 0
            elif mixed:
                assert L.offt_hip_set_option(po, api.OPT_HALF_MIXED, 1 if on else 0) == 0
            else:
                api.offt_hip_set_half_box(po, on)

        def timed(fn, on):
            route(on)
            ev[0].record()
            fn(on)
            ev[1].record()
            torch.cuda.synchronize()
            return ev[0].elapsed_time(ev[1]) * 1e-3

        V = 2.0 * esz * float(n) ** 2 * (n // 2 + 1 if r2c else n)
        api.offt_hip_set_half_box(po, True)
        if r2c and mixed:   # the two older options stay on: alone they leave such a plan on the fallback
            assert L.offt_hip_set_option(po, api.OPT_HALF_R2C, 1) == 0 and L.offt_hip_set_option(po, api.OPT_HALF_MIXED, 1) == 0
        route(True)
        pruned = api.offt_hip_half_box_pruned(po)
        fused = api.offt_hip_convolve_fused(po)
        models = {"forward": 2.625 * V, "inverse": 2.625 * V, "convolve": (3.25 if fused else 7.25) * V + 0.5 * V}
        tag = f"{'r2c ' if r2c else ''}{'mixed ' if mixed else ''}{'f32' if prec == api.F32 else 'f64'} {n}^3"
        base = "option off: library clear + ordinary" if opt else "clear + ordinary"
        for name, fn in (("forward", fwd), ("inverse", inv), ("convolve", conv)):
            t = {True: [], False: []}
            for _ in range(3):
                timed(fn, True)
                timed(fn, False)
            for _ in range(runs):   # alternating: both routes see the same state of the machine
                t[True].append(timed(fn, True))
                t[False].append(timed(fn, False))
                vol[:h, :h, :h].mul_(1e-9 if name != "convolve" else 0.5)   # keeps the field bounded over the repetitions
            on_min, on_med = min(t[True]), statistics.median(t[True])
            off_min, off_med = min(t[False]), statistics.median(t[False])
            emit(f"{tag} {name}: half box [{'pruned' if pruned else 'fallback'}{', fused' if name == 'convolve' and fused else ''}] "
                 f"min {on_min * 1e3:.3f} median {on_med * 1e3:.3f} ms ({models[name] / on_min / 1e12:.2f} TB/s of the {models[name] / V:.3f}-sweep model)  "
                 f"baseline ({base}) min {off_min * 1e3:.3f} median {off_med * 1e3:.3f} ms (spread {(off_med - off_min) / off_min * 100:.1f} %)  "
                 f"ratio min {off_min / on_min:.2f}x median {off_med / on_med:.2f}x  runs {runs}")
        api.offt_3d_fin(po)
        del dev, H, vol
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
