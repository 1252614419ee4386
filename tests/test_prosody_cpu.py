"""CPU: the prosody controls' boundary (include/zerovox_amd.h zv_prosody) — struct layout, exported entry points, the Python
binding's conversions and the CLI flags' usage errors.  None of these needs a GPU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "zerovox.cpp_amd", "zerovox")
NEW_SYMBOLS = ("zv_encode_taps_prosody", "zv_synthesize_prosody", "zv_synthesize_batch_prosody", "zv_synthesize_batch_begin_prosody")
FLAGS = ("--duration-scale", "--pitch-scale", "--pitch-shift", "--energy-scale", "--energy-shift")


def test_struct_layout_matches_ctypes(tmp_path):
    """sizeof / offsetof of the C struct, compiled against the header, equal the ctypes mirror's"""
    import ctypes as C
    from zerovox_cpp_amd import capi
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "zerovox_amd.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(zv_prosody), offsetof(zv_prosody, duration_scale), '
                   'offsetof(zv_prosody, pitch_scale), offsetof(zv_prosody, pitch_shift), offsetof(zv_prosody, energy_scale), '
                   'offsetof(zv_prosody, energy_shift)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P = capi.Prosody
    assert got == [C.sizeof(P), P.duration_scale.offset, P.pitch_scale.offset, P.pitch_shift.offset, P.energy_scale.offset,
                   P.energy_shift.offset]
    assert got[0] == 20


def test_new_entry_points_are_declared_exported_and_bound():
    from zerovox_cpp_amd import capi
    lib = capi.load_library()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zerovox_amd.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name) and name in capi.SYMBOLS, name
        assert getattr(lib, name).argtypes[-1] is C_POINTER_PROSODY(), name


def C_POINTER_PROSODY():
    import ctypes as C
    from zerovox_cpp_amd import capi
    return C.POINTER(capi.Prosody)


def test_prosody_conversions():
    from zerovox_cpp_amd import capi
    ident = capi.Prosody()
    assert [ident.duration_scale, ident.pitch_scale, ident.pitch_shift, ident.energy_scale, ident.energy_shift] == [1, 1, 0, 1, 0]
    p = capi._prosody(dict(duration_scale=1.5, pitch_shift=0.25))
    assert (p.duration_scale, p.pitch_scale, p.pitch_shift, p.energy_scale, p.energy_shift) == (1.5, 1.0, 0.25, 1.0, 0.0)
    q = capi._prosody((2.0, 0.5, -0.125, 0.75, 0.0625))
    assert (q.duration_scale, q.pitch_scale, q.pitch_shift, q.energy_scale, q.energy_shift) == (2.0, 0.5, -0.125, 0.75, 0.0625)
    assert capi._prosody(None) is None and capi._prosody(q) is q


def test_cli_lists_the_prosody_flags():
    assert os.access(CLI, os.X_OK), "run __graft_entry__.build() first"
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for f in FLAGS:
        assert f in r.stdout, f


@pytest.mark.parametrize("flag,value", [("--duration-scale", "0"), ("--duration-scale", "-1"), ("--duration-scale", "16.5"),
                                        ("--duration-scale", "nan"), ("--duration-scale", "abc"), ("--pitch-scale", "inf"),
                                        ("--pitch-shift", "1x"), ("--pitch-shift", ""), ("--energy-scale", "-inf"),
                                        ("--energy-shift", "nan"), ("--energy-shift", None)])
def test_cli_bad_prosody_values_are_usage_errors(tmp_path, flag, value):
    """exit 2 before any device work: the model path does not even exist (a load would exit 1) and no output is written"""
    out = tmp_path / "o.wav"
    args = [CLI, "-m", str(tmp_path / "missing.gguf"), "-o", str(out), flag] + ([] if value is None else [value])
    r = subprocess.run(args, capture_output=True, text=True)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert flag in r.stderr and not out.exists()


def test_cli_accepts_good_prosody_values_up_to_the_model_load(tmp_path):
    """valid values pass the parser: the run then fails where any run without the file fails (exit 1, the load)"""
    r = subprocess.run([CLI, "-m", str(tmp_path / "missing.gguf"), "-o", str(tmp_path / "o.wav"), "--duration-scale", "16",
                        "--pitch-scale", "0.9", "--pitch-shift", "-0.05", "--energy-scale", "1.2", "--energy-shift", "1e-3"],
                       capture_output=True, text=True)
    assert r.returncode == 1 and "zerovox:" in r.stderr
