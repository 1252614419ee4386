"""CPU: which regions a batch request's three blocks hold for a stage range (csrc/stage_range.h), driven through
tests/native/stage_range_check.cpp.

The check program holds the expectations: over every range of encoder -> decoder -> vocoder, the request's options, four asks of the
waveform stages, (nseg, n_rows, t_rows) = (1, 32, 64), (3, 96, 192), (64, 2048, 65536) and all / half / none of the rows travelling back
it asserts that every region is 256-aligned, that the regions of a block are disjoint, ascending and inside the block's size, that a
region the range does not touch takes zero bytes and one it needs has the bytes written out there, and that the full range reproduces
every offset of capi.cpp's batch_enqueue as it carved inline before the header existed.  The cases once more through a build with
-fsanitize=address,undefined, as a stand-alone program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zerovox.cpp_amd", "csrc")
CHECK = os.path.join(ROOT, "tests", "native", "stage_range_check.cpp")


def _build(tmp, name, extra, inc=()):
    out = str(tmp / name)
    r = subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Werror"] + ["-I" + i for i in inc] + ["-I" + CSRC] + extra + [CHECK, "-o", out],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("stage_range")
    return _build(tmp, "stage_range_check", []), _build(tmp, "stage_range_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def test_every_range_carves_disjoint_aligned_blocks_and_the_chain_keeps_its_offsets(exes):
    r = subprocess.run([exes[0], "cases"], capture_output=True, text=True, timeout=120)
    # 6 ranges x 3 shapes x 16 option sets x 4 asks x 3 result sizes: over a hundred single checks each
    assert r.returncode == 0 and r.stdout.split()[0] == "ok" and int(r.stdout.split()[1]) >= 300000, (r.stdout[-1000:], r.stderr[-500:])


def test_header_under_address_and_undefined_sanitizers(exes):
    r = subprocess.run([exes[1], "cases"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split()[0] == "ok", (r.stdout[-1000:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]


@pytest.mark.parametrize("name,old,new", [
    # a token table carved for a batch without the encoder
    ("tokens", "case BI_TOK: return enc ? tab : 0;", "case BI_TOK: return tab;"),
    # the decoder's run table handed to a stand-alone decode
    ("runs", "case BD_RUNS: return enc && dec && !q.fitted ? tab : 0;", "case BD_RUNS: return dec && !q.fitted ? tab : 0;"),
    # the source rows carved ahead of the staging regions: the chain's offsets would move
    ("order", "    take(pin, BP_SRC);      // the newest region", "    // the newest region"),
    # the stages' regions carved for a range without the vocoder
    ("wave", "const WaveAsk ask = r.has(ST_VOCODER) ? ask_in : WaveAsk{};", "const WaveAsk ask = ask_in;"),
])
def test_the_check_program_sees_a_wrong_header(tmp_path, name, old, new):
    """the same program over a header with one mistake fails: the check is not vacuous"""
    h = open(os.path.join(CSRC, "stage_range.h")).read()
    assert h.count(old) == 1, name
    (tmp_path / "stage_range.h").write_text(h.replace(old, new))
    out = _build(tmp_path, "bad", [], inc=[str(tmp_path)])
    r = subprocess.run([out, "cases"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "FAILED" in r.stdout and "ok" not in r.stdout.split(), r.stdout[-500:]
