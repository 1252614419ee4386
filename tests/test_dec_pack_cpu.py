"""CPU: densely packed decoding's layout rule and launch plans (csrc/dec_runs.h, csrc/conv_plan.h), driven through
tests/native/dec_pack_check.cpp with csrc/knobs.cpp.

1. Sweep: batches of one, two and three to eight small utterances (capacities around the multiples of 32, frame counts on both sides
   of a run, the empty batch) at R = 2 and 14: slots disjoint and in order, every row0_p a multiple of 32, a guard of 1 .. 32 rows
   (32 exactly when rows_c is a multiple of 32), L_p <= sum T + 32 nseg; a zero-padded 3-tap filter over the packed array with zeros
   in the guards gives the per-utterance filter's f32 bits on every live row; the pair of a partial last statistics block, summed
   again from the live rows (dec_pack_tail_pair), has the f64 bits of the conv epilogue's two chains.  Built a second time with
   the address and undefined-behaviour sanitizers.
2. The benchmark batch (tests/test_tile_deal_cpu.py FRAMES, T = 1 024, R = 14): L_p = 20 448 rows = 80 tiles of 256 rows, against
   89 tiles with every utterance tiled by itself.
3. Plans: the decoder's conv launches over the packed rows as one segment of t_rows + 32 nseg rows that states its 32 utterances name
   the kernels of today's 32-segment launches — form, template arguments, LDS, grid.y / grid.z — and the utterance count is what
   routes a one-segment launch away from the single-utterance forms."""
import os
import subprocess

import pytest

from test_tile_deal_cpu import FRAMES, T_CAP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zerovox.cpp_amd", "csrc")
SRCS = [os.path.join(ROOT, "tests", "native", "dec_pack_check.cpp"), os.path.join(CSRC, "knobs.cpp")]


def _build(out, flags):
    r = subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC] + flags + SRCS + ["-o", out],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("dec_pack")
    return (_build(str(tmp / "dec_pack_check"), []),
            _build(str(tmp / "dec_pack_check_san"), ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))


@pytest.mark.parametrize("R", [2, 14])
def test_slots_guards_filter_and_tail_pair(exes, R):
    for exe in exes:
        r = subprocess.run([exe, "sweep", str(R)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
        ok, batches, utts, taken = r.stdout.split()
        assert ok == "ok" and int(batches) > 10000 and 0 < int(taken) < int(utts)          # runs taken and not taken


def test_benchmark_batch_packs_into_80_tiles(exes):
    r = subprocess.run([exes[0], "rows", str(T_CAP), "14"] + [str(n) for n in FRAMES], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-500:]
    assert len(FRAMES) == 32 and [int(x) for x in r.stdout.split()] == [20448, 80, 89]


def test_packed_launches_name_the_kernels_of_the_segment_launches(exes):
    cap = len(FRAMES) * T_CAP + 32 * len(FRAMES)          # the one segment's rows: dec_pack_rows_cap
    for exe in exes:
        r = subprocess.run([exe, "plan", str(T_CAP), str(len(FRAMES)), str(cap)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stdout.split()[0] == "same", (r.stdout[-500:], r.stderr[-2000:])
        assert int(r.stdout.split()[1]) >= 13             # every conv of the decoder was planned, on conv_gemm_kernel or the generic kernel
