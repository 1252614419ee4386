"""CPU: the loader-wave conv form's workgroup -> (row tile, channel group) map (csrc/conv_xcd.h), driven through
tests/native/conv_xcd_check.cpp.

For every ny in 1..40 and nx in 1..600, with the spread map on (launches over several segments) and off (one utterance):
grid.x is a multiple of 8, every (bx, by) of the nx x ny space is produced exactly once and every other workgroup is dead; for
ny >= 8 — and for every ny with the spread map off — the map equals the closed form the kernel used before the header existed
(written out in the check program); for ny < 8 with the spread map on, a channel group's row tiles sit on that group's p XCDs
(p = 8 / 4 / 2 / 1 for ny = 1 / 2 / 3-4 / 5-7) and on no other, ny * min(p, nx) XCDs receive live work (min(8, ny * p) once a
group has p row tiles), and the live counts of a group's XCDs differ by at most one.  The same once more through a build with
-fsanitize=address,undefined, as a stand-alone program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zerovox.cpp_amd", "csrc")
NY, NX = (1, 40), (1, 600)
CASES = (NY[1] - NY[0] + 1) * (NX[1] - NX[0] + 1) * 2


def _build(tmp, name, extra):
    out = str(tmp / name)
    r = subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC] + extra +
                       [os.path.join(ROOT, "tests", "native", "conv_xcd_check.cpp"), "-o", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("conv_xcd")
    return _build(tmp, "conv_xcd_check", []), _build(tmp, "conv_xcd_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _run(exe):
    return subprocess.run([exe] + [str(v) for v in NY + NX], capture_output=True, text=True, timeout=600)


def test_every_slot_once_and_groups_on_their_xcds(exes):
    r = _run(exes[0])
    assert r.returncode == 0 and r.stdout.strip() == "ok %d" % CASES, (r.stdout[-500:], r.stderr[-500:])


def test_header_under_address_and_undefined_sanitizers(exes):
    r = _run(exes[1])
    assert r.returncode == 0 and r.stdout.strip() == "ok %d" % CASES, (r.stdout[-500:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]


def test_the_check_program_sees_a_wrong_map(tmp_path):
    """the same program over a header whose spread map leaves a row tile out fails: the check is not vacuous"""
    h = open(os.path.join(CSRC, "conv_xcd.h")).read()
    assert "s.bx = q * p + r;" in h
    (tmp_path / "conv_xcd.h").write_text(h.replace("s.bx = q * p + r;", "s.bx = q * p + r + (q == 3);"))
    out = str(tmp_path / "bad")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-I" + str(tmp_path), os.path.join(ROOT, "tests", "native", "conv_xcd_check.cpp"), "-o", out],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([out, "1", "7", "1", "64"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "ok" not in r.stdout, r.stdout[-500:]
