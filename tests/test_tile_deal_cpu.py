"""CPU: the ResBlock kernels' workgroup -> tile map (csrc/tile_deal.h), driven through tests/native/tile_deal_check.cpp.

1. Launches with several segments: for nseg in 2..40 and 1..700 tiles per segment, with the chunk lengths the library ships and
   the launchers' grid rule, every tile is produced exactly once, every other workgroup gets the dead index and the tiles of a
   chunk share their XCD (b & 7).
2. Balance on the benchmark batch.  The frame counts below are the CPU oracle's encoder on bench.py's batch (seed 3, 32 utterances,
   capacity T = 1 024); the run-shortened vocoder keeps n + 2H + 30 rows of each (H = the vocoder's halo of 20 frames; + 1 for
   the run's own frame and the padding's first rows, which are not yet constant), capped at T.  Per stage, with the tile heights
   the launchers really use on that batch, the busiest XCD may hold at most 1.15 x the mean of the live tiles — in the whole-batch
   launches and in each of the eight groups of four utterances the last stage runs in.  The one-segment map (a contiguous eighth
   of the capacity per XCD), which every launch used before, must be at least 1.3 x the mean in the same computation (the
   eight groups taken together, as the stage runs them): the test does not pass because the batch is balanced anyway."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zerovox.cpp_amd", "csrc")

FRAMES = [437, 596, 255, 603, 662, 486, 368, 551, 639, 249, 881, 606, 529, 721, 815, 946,
          819, 666, 610, 142, 752, 374, 759, 143, 744, 341, 269, 477, 159, 239, 281, 309]
T_CAP, HALO = 1024, 20

# (channels, rows per frame, tile heights TM of the jobs) of the launches on that batch, from conv1d_mfma.hip's launchers and the
# medium checkpoint's residual blocks (3 / 7 / 11 taps, dilations 1, 3, 5):
#   256: resblock_pair_kernel, 96-row tiles (MT = 3), TM = 96 - (K - 1); the merged last pair runs as three such launches
#   128: resblock_pair_kernel, 128-row tiles (MT = 4), TM = 128 - (K - 1); the merged last pair uses the widest K for all
#    64: resblock_block64_kernel for the 3-tap branch, TM = 256 - 2 (1 + 3 + 2); resblock_pair64_kernel, TM = 256 - (K - 1)
#    32: resblock_block32_kernel on 512-row tiles, TM = 512 - (K - 1) (1 + 3 + 5 + 3)
STAGES = [(256, 5, [94, 90, 86]), (128, 25, [126, 122, 118]), (64, 100, [244, 254, 250, 246]), (32, 300, [488, 440, 392])]
GROUP = 4                     # utterances per launch group of the last stage (ZV_TAIL_GROUPS = 8 on 32 utterances)
CAP, FLOOR_OLD = 1.15, 1.3


def shipped_chunks():
    """channels -> chunk length, from the header's defaults"""
    h = open(os.path.join(CSRC, "tile_deal.h")).read()
    out = {}
    for cp in (256, 128, 64, 32):
        m = re.search(r"#ifndef ZV_DEAL_C%d\s*\n#define ZV_DEAL_C%d (\d+)" % (cp, cp), h)
        assert m, cp
        out[cp] = int(m.group(1))
        assert out[cp] in (1, 2, 4, 8)
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("tile_deal") / "tile_deal_check")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, os.path.join(ROOT, "tests", "native", "tile_deal_check.cpp"),
                        "-o", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def test_every_tile_once_and_chunks_on_one_xcd(exe):
    for c in sorted(set(shipped_chunks().values())):
        r = subprocess.run([exe, "cover", str(c), "2", "40", "1", "700"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.strip() == "ok %d" % (39 * 700), (c, r.stdout[-500:], r.stderr[-500:])


def _ratio(exe, which, c, TM, rate, rows):
    r = subprocess.run([exe, "load", which, str(c), str(TM), str(rate), str(T_CAP), str(len(rows))] + [str(x) for x in rows],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-500:]
    per = [int(x) for x in r.stdout.split()]
    assert len(per) == 8 and sum(per) == sum((x * rate + TM - 1) // TM for x in rows), (per, which, TM)
    return max(per), sum(per) / 8.0


def test_busiest_xcd_on_the_benchmark_batch(exe):
    rows = [min(n + 2 * HALO + 30, T_CAP) for n in FRAMES]
    assert len(rows) == 32 and sum(FRAMES) == 16428
    chunks = shipped_chunks()
    for cp, rate, tms in STAGES:
        for TM in tms:
            mx, mean = _ratio(exe, "new", chunks[cp], TM, rate, rows)
            omx, omean = _ratio(exe, "old", 1, TM, rate, rows)
            print("whole batch  C %3d TM %3d c %d: busiest / mean  new %.3f  old %.3f" % (cp, TM, chunks[cp], mx / mean, omx / omean))
            assert mean == omean
            assert mx <= CAP * mean, (cp, TM, mx, mean)
            assert omx >= FLOOR_OLD * omean, (cp, TM, omx, omean)
    cp, rate, tms = STAGES[-1]
    for TM in tms:
        old_busiest = old_mean = 0.0
        for g0 in range(0, len(rows), GROUP):
            mx, mean = _ratio(exe, "new", chunks[cp], TM, rate, rows[g0:g0 + GROUP])
            omx, omean = _ratio(exe, "old", 1, TM, rate, rows[g0:g0 + GROUP])
            print("group of %d at %2d  TM %3d c %d: busiest / mean  new %.3f  old %.3f" % (GROUP, g0, TM, chunks[cp], mx / mean, omx / omean))
            assert mx <= CAP * mean, (g0, TM, mx, mean)
            old_busiest += omx
            old_mean += omean
        # the groups run one after the other, so the stage lasts the sum of their busiest XCDs: that sum is what the one-segment
        # map must miss (a group of four long utterances alone is nearly balanced under either map: 1.24 at frames 529 .. 946)
        print("eight groups, TM %3d: sum of busiest / sum of means, old %.3f" % (TM, old_busiest / old_mean))
        assert old_busiest >= FLOOR_OLD * old_mean, (TM, old_busiest, old_mean)
