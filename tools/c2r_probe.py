#!/usr/bin/env python3
"""Developer probe: complex-to-real inverse against the real-to-complex forward of the same plan, in one process.

After a warm-up of both, the two transforms ALTERNATE (forward, inverse, forward, ...), so that both see the same box state;
the best of each is reported with its pass split against the byte model: the r2c z pass reads 8 Nz and writes 16 (Nz/2+1)
bytes per line, the c2r z pass the reverse; the y and x passes read and write 16 (Nz/2+1) bytes per point of their plane.
usage: c2r_probe.py [f64|f32:]N ...     (default: 512 1024 f32:1024)"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from offt_amd import api  # noqa: E402

L = api.lib()
REPS = int(os.environ.get("C2R_PROBE_REPS", "6"))


def timed(po, fn):
    fn()
    t = (C.c_double * 3)()
    L.offt_hip_last_pass_seconds(po, t)
    return L.offt_hip_last_device_seconds(po), list(t)


def line(tag, n, esz, best):
    h = n // 2 + 1
    # bytes per pass (z, y, x) of the algorithm: every value read and written once
    alg = [esz * n ** 3 + 2 * esz * h * n * n, 4.0 * esz * h * n * n, 4.0 * esz * h * n * n]
    d, t = best
    return (f"{tag} {n}^3: {d * 1e3:.3f} ms; z/y/x " + " ".join(f"{x * 1e3:.3f}ms({a / x / 1e9:.0f}GB/s)" for x, a in zip(t, alg))
            + f" => {sum(alg) / d / 8e12 * 100:.1f}% of 8 TB/s")


def main():
    specs = sys.argv[1:] or ["512", "1024", "f32:1024"]
    torch.cuda.set_device(0)
    for spec in specs:
        prec_s, _, n_s = spec.rpartition(":")
        prec = api.F32 if prec_s == "f32" else api.F64
        n = int(n_s)
        po = api.offt_3d_init(n, n, n, is_r2c=1, precision=prec)
        td = torch.float32 if prec == api.F32 else torch.float64
        dev = torch.zeros(api.local_elems(po) * 2, dtype=td, device="cuda")
        torch.cuda.synchronize()
        L.offt_hip_fill_input(po, dev.data_ptr(), 1)
        L.offt_hip_set_output_scale(po, 1.0 / float(n) ** 3)  # the round trip keeps the field bounded
        fwd = lambda: api.offt_3d_execute(po, dev.data_ptr(), dev.data_ptr())
        inv = lambda: api.offt_3d_execute_dir(po, dev.data_ptr(), dev.data_ptr(), +1)
        for _ in range(2):  # warm-up
            fwd(); inv()
        bf = bi = None
        for _ in range(REPS):
            f = timed(po, fwd)
            i = timed(po, inv)
            bf = f if bf is None or f[0] < bf[0] else bf
            bi = i if bi is None or i[0] < bi[0] else bi
        esz = 4 if prec == api.F32 else 8
        tag = "f32" if prec == api.F32 else "f64"
        print(line(f"r2c {tag}", n, esz, bf), flush=True)
        print(line(f"c2r {tag}", n, esz, bi) + f"   (c2r / r2c = {bi[0] / bf[0]:.3f})", flush=True)
        api.offt_3d_fin(po)
        del dev
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
