"""CPU: what every conv and ResBlock launcher does (csrc/conv_plan.h), driven through tests/native/conv_plan_check.cpp with csrc/knobs.cpp.

The check program holds the expectations, each worked out by hand from the launchers as they stood inline in conv.hip, conv1d_mfma.hip
and conv_gemm.hip and quoted by line there, at 256 CUs: the generic conv's wave tile (WN by output tiles, the MT ladder, the 80 KB cut,
the memory-bound cap, every clause of the two-tiles-per-wave rule, ZV_CONV_MT / ZV_CONV_NT), conv_stream_kernel's predicate clause by
clause, its switch, strips and two widths, the loader-wave form clause by clause with its XCD grids, its warm-up flag and the
two-tile LDS overflow that falls back to the one-tile form, the split between conv_gemm_kernel and the generic kernel, the pair
kernels' ring form, tile heights, ZV_PAIR_MT and LDS bytes, the whole-block kernels' tile, weight buffers, interleave and fallback,
block64's grid and 80 KB refusal, the output conv's LDS bound (out_conv_supported: 7 taps take 112 channels, not 113 or 128; the loader
refuses a checkpoint beyond it with ZV_ERR_SHAPE and launch_out_conv a call — pinned here alone: a checkpoint with a last stage of 128
channels has 2 048 vocoder channels and, even with 1-tap residual blocks, about 100 MB of weights, too large for a GPU test of the
refusal), and the shapes tests/test_gpu_conv_xcd.py and the benchmark batch were built for.  The cases once
more through a build with -fsanitize=address,undefined, as a stand-alone program; and conv_gemm_groups / conv_gemm_tiles against their
restatement in tests/parity_helpers.py."""
import os
import subprocess

import pytest

import parity_helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zerovox.cpp_amd", "csrc")
SRCS = [os.path.join(ROOT, "tests", "native", "conv_plan_check.cpp"), os.path.join(CSRC, "knobs.cpp")]


def _build(out, flags, includes=()):
    r = subprocess.run(["g++", "-std=c++17", "-Wall"] + flags + ["-I" + i for i in (*includes, CSRC)] + SRCS + ["-o", out],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("conv_plan")
    return (_build(str(tmp / "conv_plan_check"), ["-O2", "-g", "-Werror"]),
            _build(str(tmp / "conv_plan_check_san"), ["-O2", "-g", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))


def test_plans_forms_tiles_grids_and_lds(exes):
    r = subprocess.run([exes[0], "cases"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.split()[0] == "ok" and int(r.stdout.split()[1]) >= 212, (r.stdout[-1000:], r.stderr[-500:])


def test_gemm_tiles_match_the_parity_helpers(exes):
    r = subprocess.run([exes[0], "gemm_tiles"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-500:]
    rows = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    assert [c for c, _, _ in rows] == list(range(16, 2113, 16))
    for cout_p, groups, tiles in rows:
        assert (groups, tiles) == (parity_helpers.conv_gemm_groups(cout_p), parity_helpers.conv_gemm_tiles(cout_p)), cout_p
    # the decoder convs of the benchmark batch: every tile on conv_gemm_kernel
    assert parity_helpers.conv_tile_split(1056) == (33, 33, 0) and parity_helpers.conv_tile_split(528) == (17, 17, 0)


def test_header_under_address_and_undefined_sanitizers(exes):
    r = subprocess.run([exes[1], "cases"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.split()[0] == "ok", (r.stdout[-1000:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]


@pytest.mark.parametrize("good, bad", [
    ("wgs(1, 1) <= 2L * n_cu", "wgs(1, 1) <= 2L * n_cu + 1"),                      # the loader form one workgroup late
    ("rwgs >= 6L * n_cu", "rwgs >= 6L * n_cu + 1"),                                # the ring form one workgroup late
    ("njobs >= 7000L * c.n_cu", "njobs >= 7000L * c.n_cu + 3"),                    # 512-row tiles one row late
])
def test_the_check_program_sees_a_wrong_threshold(tmp_path, good, bad):
    """the same program over a header with one threshold moved by one fails: the check is not vacuous"""
    h = open(os.path.join(CSRC, "conv_plan.h")).read()
    assert h.count(good) == 1
    (tmp_path / "conv_plan.h").write_text(h.replace(good, bad))
    out = _build(str(tmp_path / "bad"), ["-O0"], includes=(str(tmp_path),))
    r = subprocess.run([out, "cases"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "ok" not in r.stdout.split(), r.stdout[-500:]
