#!/usr/bin/env python3
"""Regenerate the committed golden fixtures (run in the development container).

PARITY UNPINNED: none of these fixtures is a pin by the reference's own tests (it has none) or by a
genuine reference build (FFTW is absent from the image).  Item 1 comes from a STAND-IN build and is kept as
corroboration only; the numerics are pinned by numpy (item 3) and the closed-form ramp.

1. ref_n18_p6_p1-2_S1.npz -- output of a STAND-IN BUILD of the reference: the survey stage
   compiled the unmodified rchyena/offt sources against declarations-only fftw3.h /
   fftw3-mpi.h stand-ins, MPICH + MKL's FFTW3 wrapper symbols and ran `mpiexec -n 6 ./dump 18 2 0 1` (SURVEY.md Appendix D
   step 5: N=18, p1=2, is_equalxy=0, S=1, seeded position-hash input).  Each
   rank dumped `gx gy gz re im` through ostart/osize/ostride into
   /tmp/oracle/out.<rank>.txt; this script only repackages those text files
   (data, no reference source) together with their `# ostart.. osize.. ostride..`
   header lines.  It does not run or build the reference.
2. survey_recorded.json -- values the survey recorded from reference runs
   (BASELINE.md 2): default-parameter line for N=128 p=2, the
   run-fft -v spot values at 128^3 on 2 ranks, and the default P1 choices.
3. numpy_fftn_*.npz -- independent second oracle: numpy.fft.fftn (pocketfft) of
   the seeded hash field for 8^3, 16^3 and 20^3.
4. reference_boundary.json -- only with a reference checkout and the directory of an
   MPI's mpi.h given as arguments (`make_fixtures.py <checkout> <mpi include dir>`): what tests/test_boundary_pin.py pins our header
   against, as data -- the names of offt.h its run-fft.c uses, the offsets, sizes
   and macro values of its offt.h compiled with the Hopper flags (stand-in FFTW
   names from tests/compile_shim/, an MPI header), and SHA-256 hashes of its five
   entry points' prototypes.  No reference text is stored.
"""
import glob
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracle_lib as O  # noqa: E402  (hash_field only)


def ref_dump(src="/tmp/oracle"):
    files = sorted(glob.glob(os.path.join(src, "out.*.txt")))
    if len(files) != 6:
        print("survey dump not present; keeping the committed fixture")
        return
    coords, vals, layout = [], [], []
    for r, fn in enumerate(files):
        h = open(fn).readline().split()
        layout.append([int(x) for x in h[2:5] + h[6:9] + h[10:13]])
        d = np.loadtxt(fn, ndmin=2)
        coords.append(np.concatenate([np.full((len(d), 1), r), d[:, :3]], axis=1).astype(np.int16))
        vals.append(d[:, 3] + 1j * d[:, 4])
    np.savez_compressed(os.path.join(HERE, "ref_n18_p6_p1-2_S1.npz"), rank_xyz=np.concatenate(coords),
                        value=np.concatenate(vals), ostart_osize_ostride=np.array(layout, dtype=np.int32))


def survey_values():
    rec = {
        "source": "SURVEY.md 8(c) fixtures row, BASELINE.md section 2 (reference run in the survey container)",
        "default_params_N128_p2": {"P1": 1, "T1": 8, "W1": 2, "Px1": 8, "Py1": 8, "Fz": 1, "FP1": 1, "Ux1": 8,
                                    "Uz1": 8, "FU1": 1, "Fy1": 1, "Ry": 5, "T2": 4, "W2": 2, "Pz2": 4, "Px2": 16,
                                    "Fy2": 0, "FP2": 0, "Uz2": 4, "Uy2": 16, "FU2": 0, "Fx": 0, "V": 0, "S": 0},
        "default_P1": {"8": 2, "2": 1},
        "ramp_128_p2_X000": 14781775872.0,
        "ramp_closed_form": "X[0,0,0]=N^3*111*(N-1)/2 ; X[0,0,k]=N^3*(-1/2 + (i/2)cot(pi k/N)), k != 0",
        "layout_1024_p8_2x4": {"M1": 512, "M2": 256, "M3": 256, "M4": 512, "istride": [262144, 1024, 1],
                               "ostride_zyx": [1, 1024, 524288]},
    }
    json.dump(rec, open(os.path.join(HERE, "survey_recorded.json"), "w"), indent=1)


def numpy_goldens():
    for n in (8, 16, 20):
        f = O.hash_field(n, n, n)
        np.savez_compressed(os.path.join(HERE, f"numpy_fftn_hash_{n}.npz"), F=np.fft.fftn(f))


def reference_boundary(ref, mpi_inc):
    import pathlib
    import test_boundary_pin as B
    hop = ["-DA2AV", "-DSTRIDE", "-DSHSONG_HOPPER", "-DSHSONG_MPICH"]
    header = os.path.join(ref, "offt.h")
    with tempfile.TemporaryDirectory() as tmp:
        layout = B.layout_program(hop + ["-I" + os.path.join(HERE, "..", "compile_shim"), "-I" + mpi_inc, "-include", header],
                                  pathlib.Path(tmp), "ref")
    htxt = open(header).read()
    code = re.sub(r"//[^\n]*|/\*.*?\*/", " ", open(os.path.join(ref, "run-fft.c")).read(), flags=re.S)
    owner = {f: st for st, fields in B.PUBLIC.items() for f in fields}
    members = {f: owner[f] for f in re.findall(r"->\s*(\w+)", code) if f in owner}
    idents = set(re.findall(r"\b\w+\b", code))
    declared = set(re.findall(r"\b(\w+)\s*\([^;{)]*\)\s*[;{]", htxt))  # functions the header declares or defines
    uses = {"members": dict(sorted(members.items())),
            "macros": [m for m in B.MACROS if m in idents],
            "switches": sorted(m for m in set(re.findall(r"#\s*ifn?def\s+(\w+)", code))
                               if re.search(r"#\s*define\s+%s\s*(/[/*].*)?$" % m, htxt, flags=re.M)),
            "functions": sorted(f for f in declared if re.search(r"\b%s\s*\(" % f, code))}
    rec = {"source": "reference checkout: run-fft.c (names used) and offt.h (layout, prototype hashes); make_fixtures.py item 4",
           "caller_uses": uses, "layout": layout,
           "prototype_sha256": sorted(hashlib.sha256(p.encode()).hexdigest() for p in B.normalised_prototypes(header))}
    json.dump(rec, open(os.path.join(HERE, "reference_boundary.json"), "w"), indent=1)


if __name__ == "__main__":
    if len(sys.argv) > 2:
        reference_boundary(sys.argv[1], sys.argv[2])
    ref_dump()
    survey_values()
    numpy_goldens()
    print("fixtures written to", HERE)
