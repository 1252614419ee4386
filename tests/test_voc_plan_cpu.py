"""CPU: which kernel forms a vocoder call runs (csrc/voc_plan.h), driven through tests/native/voc_plan_check.cpp with csrc/knobs.cpp.

The check program holds the expectations, each derived by hand from the schedule as it stood inline in Model::vocode_group and
quoted by line there: on the medium checkpoint's geometry (256 / 128 / 64 / 32 channels at 5 / 25 / 100 / 300 rows per frame, taps
3 / 7 / 11, dilations 1 / 3 / 5, 256 CUs) both sides of every length threshold of the plan (the 256-channel stage fused from 929
frames, block64 from 2 499, the merged sum from 2 520 / 4 834 / 11 060 at 64 / 128 / 256 channels and from 840 at 32 without the
whole-block kernel, the second upsample conv's operand pass from 3 277, run-shortening and the input conv's f16 output from 16 384
rows), fitted, switched-off and tapped calls, the benchmark batch, a tail group of 4 of its utterances planned from 4 segments, a
32-channel stage with a 5-tap pair (unfused as a whole), a 64-channel branch whose first two pairs differ in taps (not block64's,
its neighbours are: the guard no checkpoint reaches), the tail group count, and the shared batch-switch rule.  On the small
checkpoint at 256, 496, 768 and 1 024 vocoder channels (synth.VOC_WIDTH_GEOMETRIES; what the loader derives from a width pinned by
hand): one short utterance, BATCH_REGIME on one utterance, the benchmark batch's shape, ZV_MERGE_ALWAYS, and a tail group of 4 of
16 x 900 fitted frames — fused, whole_block, block64[], merge and up_pass of every stage.  Then every regime of
tests/parity_helpers.py (VOCODER_REGIMES, BATCH_REGIME) on one utterance of 16 frames.  The cases once more through a build with
-fsanitize=address,undefined, as a stand-alone program."""
import os
import subprocess

import pytest

from parity_helpers import BATCH_REGIME, VOCODER_REGIMES, WIDTH_MERGE_CASES, WIDTH_MERGE_T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zerovox.cpp_amd", "csrc")


def _build(tmp, name, extra):
    out = str(tmp / name)
    r = subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC] + extra +
                       [os.path.join(ROOT, "tests", "native", "voc_plan_check.cpp"), os.path.join(CSRC, "knobs.cpp"), "-o", out],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("voc_plan")
    return _build(tmp, "voc_plan_check", []), _build(tmp, "voc_plan_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def test_plans_thresholds_and_group_counts(exes):
    r = subprocess.run([exes[0], "cases"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.split()[0] == "ok" and int(r.stdout.split()[1]) >= 88, (r.stdout[-1000:], r.stderr[-500:])


def test_every_regime_of_the_parity_helpers(exes):
    regimes = list(VOCODER_REGIMES) + [("batch_regime", BATCH_REGIME)]
    assert len({n for n, _ in regimes}) == len(regimes)
    for name, sw in regimes:
        r = subprocess.run([exes[0], "regime", name] + ["%s=%d" % (k, int(v)) for k, v in sw.items()], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stdout.strip() == "ok", (name, r.stdout[-1000:], r.stderr[-500:])


def test_merged_output_conv_cases_of_the_width_tests(exes):
    """parity_helpers.WIDTH_MERGE_CASES: the plan of one utterance of WIDTH_MERGE_T frames under each case's switches is the one the
    table states — tests/test_gpu_vocoder_widths.py runs exactly these and takes from the table which form ran.  At least one case
    per width stores the last stage's merged sum (the output conv's one-input form)"""
    assert {g for g, _, _, merged in WIDTH_MERGE_CASES if merged} == {"small_v1024", "small_v496"}
    for gname, sw, plan, merged in WIDTH_MERGE_CASES:
        assert gname.startswith("small_v")
        r = subprocess.run([exes[0], "plan", gname[len("small_"):], "1", str(WIDTH_MERGE_T), str(WIDTH_MERGE_T)] +
                           ["%s=%d" % (k, int(v)) for k, v in sw.items()], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stdout.strip() == plan, (gname, sw, r.stdout[-1000:], r.stderr[-500:])
        assert (plan.split()[-1][-1] == "1") == merged, (gname, sw)


def test_header_under_address_and_undefined_sanitizers(exes):
    r = subprocess.run([exes[1], "cases"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.split()[0] == "ok", (r.stdout[-1000:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]


def test_the_check_program_sees_a_wrong_threshold(tmp_path):
    """the same program over a header whose 256-channel stage fuses one frame early fails: the check is not vacuous"""
    h = open(os.path.join(CSRC, "voc_plan.h")).read()
    assert "(Lbatch / 54) * 3 >= (long)c.n_cu" in h
    (tmp_path / "voc_plan.h").write_text(h.replace("(Lbatch / 54) * 3 >= (long)c.n_cu", "((Lbatch + 5) / 54) * 3 >= (long)c.n_cu"))
    out = str(tmp_path / "bad")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-I" + str(tmp_path), "-I" + CSRC, os.path.join(ROOT, "tests", "native", "voc_plan_check.cpp"),
                        os.path.join(CSRC, "knobs.cpp"), "-o", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([out, "cases"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "ok" not in r.stdout.split(), r.stdout[-500:]
