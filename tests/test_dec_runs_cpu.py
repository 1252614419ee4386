"""CPU: run-shortened decoding's row arithmetic (csrc/dec_runs.h), driven through tests/native/dec_runs_check.cpp.

1. For every (n, T) with 1 <= n <= T <= 200 and R in {2, 14}: a and b are multiples of 32, a - 32 >= n + R, b <= T - R - 1,
   rows_c + 32 G = T, a run not taken is exactly (T, 0), the expansion map sends every original row to a compact row that a
   brute-force model of the constant region says holds the same value (and every compact row has the neighbours' values its original
   row has), and the gap sum over compact partial sums has the f64 bits of the plain block-order sum over the expanded array.
2. On the benchmark batch's frame counts (tests/test_tile_deal_cpu.py FRAMES: the CPU oracle's encoder on bench.py's batch) at the
   capacity T = 1 024 with the shipped decoder's reach R = 14, the decoder keeps 19 424 of 32 768 rows and 31 of 32 utterances take
   their run."""
import os
import subprocess

import pytest

from test_tile_deal_cpu import FRAMES, T_CAP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zerovox.cpp_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dec_runs") / "dec_runs_check")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, os.path.join(ROOT, "tests", "native", "dec_runs_check.cpp"),
                        "-o", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def test_bounds_expansion_map_and_gap_sum(exe):
    r = subprocess.run([exe, "sweep", "200", "2", "14"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-500:])
    ok, cases, taken = r.stdout.split()
    assert ok == "ok" and int(cases) == 2 * 200 * 201 // 2
    assert 0 < int(taken) < int(cases)          # both outcomes were exercised


def test_benchmark_batch_rows(exe):
    r = subprocess.run([exe, "rows", str(T_CAP), "14"] + [str(n) for n in FRAMES], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-500:]
    rows, taken = (int(x) for x in r.stdout.split())
    assert len(FRAMES) == 32 and (rows, taken) == (19424, 31)
