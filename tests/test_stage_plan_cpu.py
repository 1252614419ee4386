"""CPU: what the attention, linear and length-regulator launchers do and which regime the encoder and decoder schedules run in
(csrc/stage_plan.h), driven through tests/native/stage_plan_check.cpp with csrc/knobs.cpp.

The check program holds the expectations, each worked out by hand from the code as it stood inline in misc_kernels.hip, decoder.cpp
and encoder.cpp and quoted by line there: the matrix-core attention's predicate clause by clause (head width, row stride, the LDS
formula at the token limits the GPU tests use, 47 against 48 workgroups, ZV_ATT_SCALAR / ZV_ATT_MFMA), its grid, LDS bytes and the
48 KiB attribute, the scalar form's 60 KiB refusal; the linear layers' 64- and 32-row forms on both sides of 256 workgroups; the
regulator's three forms with their grids and LDS bytes; the LayerNorm tails' 768 channels; the encoder's merged segment and tails;
the decoder's pre-pass, run table and packing under every value of their switches; and the benchmark batch.  The cases once more
through a build with -fsanitize=address,undefined, as a stand-alone program; and the header's constants and token limits against
their one restatement in tests/parity_helpers.py."""
import os
import subprocess

import pytest

import parity_helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zerovox.cpp_amd", "csrc")
SRCS = [os.path.join(ROOT, "tests", "native", "stage_plan_check.cpp"), os.path.join(CSRC, "knobs.cpp")]


def _build(out, flags, includes=()):
    r = subprocess.run(["g++", "-std=c++17", "-Wall"] + flags + ["-I" + i for i in (*includes, CSRC)] + SRCS + ["-o", out],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("stage_plan")
    return (_build(str(tmp / "stage_plan_check"), ["-O2", "-g", "-Werror"]),
            _build(str(tmp / "stage_plan_check_san"), ["-O2", "-g", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))


def test_plans_forms_grids_lds_and_regimes(exes):
    r = subprocess.run([exes[0], "cases"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.split()[0] == "ok" and int(r.stdout.split()[1]) >= 95, (r.stdout[-1000:], r.stderr[-500:])


def test_attention_limits_match_the_parity_helpers(exes):
    r = subprocess.run([exes[0], "constants"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-500:]
    assert [int(x) for x in r.stdout.split()] == [parity_helpers.ATT_NS_MAX, parity_helpers.ATT_LDS_MAX, parity_helpers.LN_TAIL_MAX]
    r = subprocess.run([exes[0], "att_limits"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-500:]
    rows = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    assert [dk for dk, _ in rows] == list(range(2, 601, 2))
    for dk, n in rows:
        assert n == parity_helpers.mfma_max_tokens(dk), dk
    # the limits tests/test_gpu_attention_heads.py walks both sides of, and the head dims it expects the scalar kernel at
    lim = dict(rows)
    assert (lim[264], lim[176], lim[132], lim[288], lim[292], lim[528], lim[66]) == (352, 416, 480, 320, 0, 0, 0)


def test_header_under_address_and_undefined_sanitizers(exes):
    r = subprocess.run([exes[1], "cases"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.split()[0] == "ok", (r.stdout[-1000:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]


@pytest.mark.parametrize("good, bad", [
    ("wgs_mfma >= ATT_MIN_WGS", "wgs_mfma >= ATT_MIN_WGS + 1"),                              # the matrix-core attention one workgroup late
    ("lds > ATT_SCALAR_LDS_MAX ?", "lds > ATT_SCALAR_LDS_MAX + 4 ?"),                        # the scalar attention's refusal one token late
    ("wg64 >= LINEAR_WG64_MIN", "wg64 >= LINEAR_WG64_MIN + 1"),                              # 64-row linear workgroups one workgroup late
    ("tokens_max <= LR_FUSED_TOKENS", "tokens_max <= LR_FUSED_TOKENS + 1"),                  # the fused regulator one token long
    ("(long)t_max * nseg >= DEC_PREPASS_ROWS", "(long)t_max * nseg >= DEC_PREPASS_ROWS + 1"),  # the decoder's pre-pass one row late
])
def test_the_check_program_sees_a_wrong_threshold(tmp_path, good, bad):
    """the same program over a header with one threshold moved by one fails: the check is not vacuous"""
    h = open(os.path.join(CSRC, "stage_plan.h")).read()
    assert h.count(good) == 1
    (tmp_path / "stage_plan.h").write_text(h.replace(good, bad))
    out = _build(str(tmp_path / "bad"), ["-O0"], includes=(str(tmp_path),))
    r = subprocess.run([out, "cases"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "ok" not in r.stdout.split(), r.stdout[-500:]
