"""The drop-in boundary pinned against the reference's own files, through what was recorded from them: nothing of the
reference is read at test time.  tests/golden/reference_boundary.json holds data only -- names, numbers and hashes --
written by `tests/golden/make_fixtures.py <reference checkout>`.

1. Every name of offt.h that the reference's caller, run-fft.c, uses (struct members it reaches through `->`, macros,
   functions; recorded as `caller_uses`) must exist in include/offt.h as the same kind of name: a probe generated from the
   list is checked with `gcc -fsyntax-only` against our header alone -- no MPI or FFTW header needed.
2. offsetof / sizeof of every public field of _offt_params, _offt_comm and _offt_plan, and the values of the public
   macros, equal those recorded from the reference's offt.h preprocessed with its Hopper flags (-DA2AV -DSTRIDE
   -DSHSONG_HOPPER, Makefile:27-29); the five entry points' prototypes equal the recorded ones (whitespace removed,
   compared by SHA-256)."""
import hashlib
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "reference_boundary.json")
HEADER = os.path.join(ROOT, "include", "offt.h")
ENTRY_POINTS = ("struct _offt_plan* offt_3d_init", "void offt_3d_", "void print_params", "void offt_print_time")

PUBLIC = {
    "_offt_params": ["is_converged", "is_infeasible", "is_in_database", "v"],
    "_offt_comm": ["p1", "p2", "M1", "M2", "M3", "M4", "F1", "F2", "F3", "F4", "m1", "m2", "m3", "m4", "b1", "b2", "b3", "b4",
                   "istart", "isize", "istride", "ostart", "osize", "ostride"],
    "_offt_plan": ["p", "rank", "Nx", "Ny", "Nz", "is_r2c", "fftw_flag", "ah_strategy", "max_loop", "tuning_mode", "is_W0",
                   "extrapolation_window", "is_oned", "is_a2a", "is_equalxy", "is_notest", "t_init", "t", "point_database_file",
                   "user_vertex_file", "params", "comm"],
}
MACROS = ["PARAM_COUNT", "LOG0", "_P1_", "_T1_", "_W1_", "_Px1_", "_Py1_", "_Fz_", "_FP1_", "_Ux1_", "_Uz1_", "_FU1_", "_Fy1_", "_Ry_",
          "_T2_", "_W2_", "_Pz2_", "_Px2_", "_Fy2_", "_FP2_", "_Uz2_", "_Uy2_", "_FU2_", "_Fx_", "_V_", "_S_", "INIT_ALL", "INIT_FFTW",
          "INIT_AH", "INIT_BUFFER", "T_INIT_COUNT", "ALL", "INIT1", "WAIT1", "TEST1", "INIT2", "WAIT2", "TEST2", "FFTz", "FFTy1", "FFTy2",
          "FFTx", "TRANSPOSE", "PACK1", "UNPACK1", "PACK2", "UNPACK2", "GES", "TUNING_REPS", "SUBTILE_SIZE", "BUFFER_SIZE_LIMIT"]


def normalised_prototypes(path):
    """the entry points' declarations of a header, whitespace removed"""
    return ["".join(ln.split()) for ln in open(path) if ln.startswith(ENTRY_POINTS)]


def layout_program(header_args, tmp_path, tag):
    lines = ["#include <stdio.h>", "#include <stddef.h>"]
    body = []
    for st, fields in PUBLIC.items():
        body.append(f'  printf("sizeof {st} %zu\\n", sizeof(struct {st}));') if st != "_offt_plan" else None
        for f in fields:
            body.append(f'  printf("{st}.{f} %zu %zu\\n", offsetof(struct {st}, {f}), sizeof(((struct {st} *)0)->{f}));')
    for m in MACROS:
        body.append(f'  printf("macro {m} %ld\\n", (long)({m}));')
    src = tmp_path / f"layout_{tag}.c"
    src.write_text("\n".join(lines) + "\nint main(void) {\n" + "\n".join(body) + "\n  return 0;\n}\n")
    exe = tmp_path / f"layout_{tag}"
    p = subprocess.run(["gcc", "-std=gnu99", "-w"] + header_args + [str(src), "-o", str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    return subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()


def uses_probe(uses):
    """a translation unit that names every recorded use: members through offsetof, macros as constant expressions (or,
    for a switch without a value, through #ifndef), functions through their address"""
    lines = ["#include <stddef.h>"]
    for m in uses["switches"]:
        lines += [f"#ifndef {m}", f'#error "{m} is not defined"', "#endif"]
    body = [f"  s += (long)offsetof(struct {st}, {f});" for f, st in sorted(uses["members"].items())]
    body += [f"  s += (long)({m});" for m in uses["macros"]]
    body += [f"  f = (const void *)&{fn};" for fn in uses["functions"]]
    return "\n".join(lines) + "\nlong probe(void) {\n  long s = 0;\n  const void *f = 0;\n" + "\n".join(body) + "\n  return s + (f != 0);\n}\n"


def test_reference_caller_compiles_against_our_header(tmp_path):
    uses = json.load(open(FIXTURE))["caller_uses"]
    assert len(uses["members"]) >= 8 and len(uses["macros"]) >= 20 and len(uses["functions"]) >= 5
    assert all(st in PUBLIC and f in PUBLIC[st] for f, st in uses["members"].items())
    src = tmp_path / "caller_uses.c"
    src.write_text(uses_probe(uses))
    cmd = ["gcc", "-std=gnu99", "-fsyntax-only", "-Werror=implicit-function-declaration", "-Werror=incompatible-pointer-types",
           "-Werror=int-conversion", "-w", "-include", HEADER, str(src)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    # the communicator members are opaque pointers in our header: a caller needs no MPI header to include it
    probe = subprocess.run(["gcc", "-E", "-include", HEADER, str(src)], capture_output=True, text=True)
    assert probe.returncode == 0 and "MPI_Comm" not in probe.stdout and "void *comm1" in probe.stdout


def test_public_field_layout_equals_the_reference_header(tmp_path):
    rec = json.load(open(FIXTURE))
    ours = layout_program(["-include", HEADER], tmp_path, "ours")
    assert len(ours) == len(rec["layout"]) > 90
    for a, b in zip(ours, rec["layout"]):
        assert a == b, (a, b)
    protos = normalised_prototypes(HEADER)
    assert len(protos) == 5 and all(hashlib.sha256(a.encode()).hexdigest() in rec["prototype_sha256"] for a in protos), protos
