"""CPU: the waveform stages' plumbing (csrc/wave_stages.h), driven through tests/native/wave_stages_check.cpp.

The check program holds the expectations, restated from the code as it stood inline before the header existed: capi.cpp's layouts of
run_single's block and batch_enqueue's three blocks, its bind blocks, its `env || ctr || pit || bnd` rule for the scan, and
Model::vocode_tail's offsets of a tail group.  Over all 64 subsets of the six stages, every frame / phoneme ask of the three table
stages and (nseg, n_rows, t_rows) = (1, 9, 40), (3, 96, 192), (64, 2048, 65536) it asserts that every region is 256-aligned, that the
regions of a block are disjoint and inside the block's size(), that a region of an off stage takes zero bytes, that every offset is
the inline layout's, that the single-utterance carve is the batch's at nseg = 1, that the group for g0 = 0, 1, 63 moves exactly the
per-utterance tables, that changing any one pointer of a WaveStages makes it compare unequal, and the ask's rules from the public
structs.  The cases once more through a build with -fsanitize=address,undefined, as a stand-alone program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zerovox.cpp_amd", "csrc")
CHECK = os.path.join(ROOT, "tests", "native", "wave_stages_check.cpp")


def _build(tmp, name, extra, inc=()):
    out = str(tmp / name)
    r = subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Werror"] + ["-I" + i for i in inc] + ["-I" + CSRC] + extra + [CHECK, "-o", out],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("wave_stages")
    return _build(tmp, "wave_stages_check", []), _build(tmp, "wave_stages_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def test_carves_binds_groups_and_asks(exes):
    r = subprocess.run([exes[0], "cases"], capture_output=True, text=True, timeout=120)
    # 3 row spaces x 1 000 (subset, ask) pairs x 3 leads: over a hundred single checks each
    assert r.returncode == 0 and r.stdout.split()[0] == "ok" and int(r.stdout.split()[1]) >= 100000, (r.stdout[-1000:], r.stderr[-500:])


def test_header_under_address_and_undefined_sanitizers(exes):
    r = subprocess.run([exes[1], "cases"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split()[0] == "ok", (r.stdout[-1000:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]


@pytest.mark.parametrize("name,old,new", [
    # a parameter row of the wrong stride: the input block's offsets move
    ("stride", "{WS_PITCH, ROWS_UTTERANCE, PITCH_PARAM_STRIDE * 4, WR_INPUT", "{WS_PITCH, ROWS_UTTERANCE, PITCH_PARAM_STRIDE * 8, WR_INPUT"),
    # a per-utterance table declared per token row: a tail group no longer moves it
    ("group", "{WS_FILTER, ROWS_UTTERANCE,", "{WS_FILTER, ROWS_TOKEN,"),
    # the frame counts left behind by a tail group
    ("nframes", "    if (d_nframes) s.d_nframes = d_nframes + g0;\n", ""),
    # a stage forgotten in the scan's rule
    ("scan", "return d_env || d_ctr_frames || d_pit_frames || d_bnd_frames;", "return d_env || d_ctr_frames || d_pit_frames;"),
])
def test_the_check_program_sees_a_wrong_header(tmp_path, name, old, new):
    """the same program over a header with one plumbing mistake fails: the check is not vacuous"""
    h = open(os.path.join(CSRC, "wave_stages.h")).read()
    assert h.count(old) == 1, name
    (tmp_path / "wave_stages.h").write_text(h.replace(old, new))
    out = _build(tmp_path, "bad", [], inc=[str(tmp_path)])
    r = subprocess.run([out, "cases"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "FAILED" in r.stdout and "ok" not in r.stdout.split(), r.stdout[-500:]
