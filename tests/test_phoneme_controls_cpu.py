"""CPU: the per-phoneme controls' boundary (include/zerovox_amd.h zv_phoneme_controls) — struct layout, exported entry points, the
Python binding's conversions and the CLI's usage errors for --phoneme-controls files.  None of these needs a GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "zerovox.cpp_amd", "zerovox")
NEW_SYMBOLS = ("zv_encode_taps_phonemes", "zv_synthesize_phonemes", "zv_synthesize_batch_phonemes",
               "zv_synthesize_batch_begin_phonemes")
FIELDS = ("duration_frames", "duration_scale", "pitch_shift", "energy_shift")


def test_struct_layout_matches_ctypes(tmp_path):
    """sizeof / offsetof of the C struct, compiled against the header, equal the ctypes mirror's"""
    import ctypes as C
    from zerovox_cpp_amd import capi
    src = tmp_path / "layout.c"
    offs = ", ".join("offsetof(zv_phoneme_controls, %s)" % f for f in FIELDS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "zerovox_amd.h"\n'
                   'int main(void) { printf("%%zu %%zu %%zu %%zu %%zu\\n", sizeof(zv_phoneme_controls), %s); return 0; }\n' % offs)
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P = capi.PhonemeControlsC
    assert got == [C.sizeof(P)] + [getattr(P, f).offset for f in FIELDS]
    assert got[0] == 4 * C.sizeof(C.c_void_p)


def test_new_entry_points_are_declared_exported_and_bound():
    import ctypes as C
    from zerovox_cpp_amd import capi
    lib = capi.load_library()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zerovox_amd.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name) and name in capi.SYMBOLS, name
        assert C.POINTER(capi.PhonemeControlsC) in getattr(lib, name).argtypes, name
        assert C.POINTER(capi.Prosody) in getattr(lib, name).argtypes, name


def test_phoneme_controls_conversions():
    import ctypes as C
    from zerovox_cpp_amd import capi
    empty = capi.PhonemeControls(5)
    assert all(getattr(empty.struct, f) is None for f in FIELDS)
    pc = capi.PhonemeControls(3, dict(duration_frames=[4, -1, 0], pitch_shift=np.array([0.5, 0, -0.25], np.float64)),
                              energy_shift=None)
    assert pc.arrays["duration_frames"].dtype == np.int32 and pc.arrays["pitch_shift"].dtype == np.float32
    assert pc.struct.duration_scale is None and pc.struct.energy_shift is None
    fr = np.ctypeslib.as_array(C.cast(pc.struct.duration_frames, C.POINTER(C.c_int32)), shape=(3,))
    ps = np.ctypeslib.as_array(C.cast(pc.struct.pitch_shift, C.POINTER(C.c_float)), shape=(3,))
    assert fr.tolist() == [4, -1, 0] and ps.tolist() == [0.5, 0.0, -0.25]
    assert capi._phoneme_controls(None, 3) is None
    assert capi._phoneme_controls(pc, 3) is pc
    assert capi._phoneme_controls(dict(duration_scale=[1.0, 2.0]), 2).arrays["duration_scale"].tolist() == [1.0, 2.0]


@pytest.mark.parametrize("kw", [dict(duration_frames=[1, 2]), dict(duration_scale=[1.0] * 4), dict(pitch_shift=[[0.0, 0.0, 0.0]]),
                                dict(energy_shift=0.5), dict(bogus=[1, 2, 3])])
def test_phoneme_controls_reject_wrong_lengths_and_names(kw):
    from zerovox_cpp_amd import capi
    with pytest.raises(ValueError):
        capi.PhonemeControls(3, kw)


def test_phoneme_controls_for_another_length_are_rejected():
    from zerovox_cpp_amd import capi
    with pytest.raises(ValueError):
        capi._phoneme_controls(capi.PhonemeControls(4), 3)


def test_cli_lists_the_new_flags():
    assert os.access(CLI, os.X_OK), "run __graft_entry__.build() first"
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    assert "--phoneme-controls" in r.stdout and "--alignment" in r.stdout


def _utt_file(tmp_path, n):
    utt = tmp_path / "utt.txt"
    utt.write_text(" ".join(["3"] * n) + "\n" + " ".join(["0"] * n) + "\n0\n")
    return utt


BAD_FILES = [
    ("-1 1 0 0\n" * 4, "lines"),                                   # one line short
    ("-1 1 0 0\n" * 6, "lines"),                                   # one line too many
    ("-1 1 0 0\n" * 4 + "-1 1 0\n", "4 values"),
    ("-1 1 0 0\n" * 4 + "-1 1 0 0 0\n", "4 values"),
    ("-2 1 0 0\n" + "-1 1 0 0\n" * 4, "frames"),
    ("32769 1 0 0\n" + "-1 1 0 0\n" * 4, "frames"),
    ("1.5 1 0 0\n" + "-1 1 0 0\n" * 4, "frames"),
    ("x 1 0 0\n" + "-1 1 0 0\n" * 4, "frames"),
    ("-1 0 0 0\n" + "-1 1 0 0\n" * 4, "scale"),
    ("-1 16.5 0 0\n" + "-1 1 0 0\n" * 4, "scale"),
    ("-1 -1 0 0\n" + "-1 1 0 0\n" * 4, "scale"),
    ("-1 nan 0 0\n" + "-1 1 0 0\n" * 4, "finite"),
    ("-1 1 inf 0\n" + "-1 1 0 0\n" * 4, "finite"),
    ("-1 1 0 nan\n" + "-1 1 0 0\n" * 4, "finite"),
    ("-1 1 0 0x\n" + "-1 1 0 0\n" * 4, "finite"),
]


@pytest.mark.parametrize("text,what", BAD_FILES)
def test_cli_bad_phoneme_control_files_are_usage_errors(tmp_path, text, what):
    """exit 2 before any device work: the model path does not even exist (a load would exit 1) and no output is written"""
    pcf = tmp_path / "pc.txt"
    pcf.write_text(text)
    out = tmp_path / "o.wav"
    r = subprocess.run([CLI, "-m", str(tmp_path / "missing.gguf"), "-u", str(_utt_file(tmp_path, 5)), "-o", str(out),
                        "--phoneme-controls", str(pcf)], capture_output=True, text=True)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert "--phoneme-controls" in r.stderr and what in r.stderr and not out.exists(), r.stderr


def test_cli_missing_phoneme_control_file_is_a_usage_error(tmp_path):
    r = subprocess.run([CLI, "-m", str(tmp_path / "missing.gguf"), "-o", str(tmp_path / "o.wav"), "--phoneme-controls",
                        str(tmp_path / "nope.txt")], capture_output=True, text=True)
    assert r.returncode == 2 and "--phoneme-controls" in r.stderr


def test_cli_built_in_utterance_needs_120_lines(tmp_path):
    pcf = tmp_path / "pc.txt"
    pcf.write_text("-1 1 0 0\n" * 119)
    r = subprocess.run([CLI, "-m", str(tmp_path / "missing.gguf"), "-o", str(tmp_path / "o.wav"), "--phoneme-controls", str(pcf)],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "120 phonemes" in r.stderr, r.stderr


def test_cli_accepts_a_good_file_up_to_the_model_load(tmp_path):
    """a valid file (blank lines ignored) passes the parser: the run then fails where any run without the model fails (exit 1)"""
    pcf = tmp_path / "pc.txt"
    pcf.write_text("-1 1 0 0\n12 1 0 0\n\n0 2.5 -0.1 0.2\n-1 16 1e-3 -0\n32768 0.01 0 0\n")
    r = subprocess.run([CLI, "-m", str(tmp_path / "missing.gguf"), "-u", str(_utt_file(tmp_path, 5)), "-o", str(tmp_path / "o.wav"),
                        "--phoneme-controls", str(pcf), "--alignment", str(tmp_path / "a.tsv")], capture_output=True, text=True)
    assert r.returncode == 1 and "zerovox:" in r.stderr, (r.returncode, r.stderr)
