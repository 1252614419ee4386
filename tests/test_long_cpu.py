"""CPU: the arithmetic tests/test_gpu_long.py rests on — how zv_synthesize_batch splits utterances into launch groups, which
frames of a zv_max_frames() utterance hold the bytes where a vocoder stage's offsets cross a power of two, and the oracle's own
window property (a window of the vocoder's output computed from the window's frames and the halo alone is the whole run's, bit
for bit), so that the windowed comparison there has no error of its own."""
import os
import re

import numpy as np

import parity_helpers as ph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TMAX = 32768


def test_launch_group_mirror_restates_the_source():
    src = open(os.path.join(ROOT, "zerovox.cpp_amd", "csrc", "capi.cpp")).read()
    body = src[src.index("static uint32_t batch_group_end"):]
    body = body[:body.index("\n}\n")]
    assert re.search(r"b - a < %d\b" % ph.GROUP_MAX_UTTERANCES, body)
    assert re.search(r"b > a && \(uint64_t\)\(b - a \+ 1\) \* zv::round_up\(\(int\)tm, 64\) > %d\b" % ph.GROUP_MAX_FRAMES, body)


def test_launch_groups_of_the_limit_compositions():
    """64 x 1 024 = 65 536 frames and 3 x 21 824 = 65 472 fit one group; 21 825 rounds up to 21 888 (3 x: 65 664), 1 025 to 1 088
    (60 x: 65 280, 61 x: 66 368); a 65th utterance starts a group whatever its length"""
    assert ph.launch_groups([1024] * 64) == [64]
    assert ph.launch_groups([32768] * 2) == [2]
    assert ph.launch_groups([16384] * 4) == [4]
    assert ph.launch_groups([21824] * 3) == [3] and 3 * 21824 == 65472
    assert ph.launch_groups([21825] * 3) == [2, 1] and 3 * 21888 == 65664
    assert ph.launch_groups([1025] * 64) == [60, 4] and 60 * 1088 == 65280 and 61 * 1088 == 66368
    assert ph.launch_groups([1008] * 65) == [64, 1]
    # edges of the rule itself: one utterance always fits; the longest so far decides, not the sum
    assert ph.launch_groups([32768]) == [1] and ph.launch_groups([32768] * 3) == [2, 1]
    assert ph.launch_groups([1] * 63 + [1024]) == [64] and ph.launch_groups([1] * 63 + [1025]) == [63, 1]
    assert ph.launch_groups([1025] + [1] * 63) == [60, 4]
    assert ph.launch_groups([64] * 200) == [64, 64, 64, 8]
    assert ph.launch_groups([]) == []


def test_offset_crossing_frames_of_the_medium_vocoder():
    from zerovox_cpp_amd import synth
    g = synth.MEDIUM
    bpf = ph.voc_stage_bytes_per_frame(g.upsample_scales, g.voc_channels)
    assert bpf == [5120, 12800, 25600, 38400]
    assert bpf[-1] * TMAX == 1258291200 < 2 ** 31                 # Model::max_frames_per_utterance: offsets stay signed 32-bit
    cross = ph.offset_crossing_frames(bpf, TMAX)
    assert cross[27962] == [(3, 30)] and 2 ** 23 // 300 == 27962      # the last stage's byte 2^30 and its row 2^23
    assert sorted(cross[20971]) == [(1, 28), (2, 29)]
    assert sorted(cross[10485]) == [(1, 27), (2, 28)]
    assert sorted(cross) == [3495, 5242, 6990, 10485, 13981, 20971, 26214, 27962]
    for f, where in cross.items():
        for stage, k in where:
            assert f * bpf[stage] <= 2 ** k < (f + 1) * bpf[stage], (f, stage, k)
    windows = ph.oracle_windows(cross, TMAX)
    assert windows[0] == (0, 64) and windows[-1] == (TMAX - 64, TMAX) and len(windows) == len(cross) + 2
    for f in cross:
        assert sum(a <= f < b for a, b in windows) == 1, f
    assert all(b - a == ph.WINDOW_FRAMES for a, b in windows)
    # a 64 Ki-frame group: the segments of utterances 55 ... 63 of 64 x 1 024 start past 2^31 bytes of the last stage's tensor
    assert [u for u in range(64) if u * 1024 * bpf[-1] >= 2 ** 31] == list(range(55, 64))
    assert 65536 * bpf[-1] > 2 ** 31 and 65536 * 300 > 2 ** 24


def test_oracle_vocoder_windows_are_the_whole_runs_bits(ckpt):
    """T = 600 at the production geometry, the halo the exact receptive radius (20 frames; the library's
    zv_vocoder_halo_frames() is at least that, which tests/test_gpu_long.py asserts): start, interior and end windows, in both
    summation orders"""
    from oracle import zvoracle
    from zerovox_cpp_amd import synth
    _, g, tensors = ckpt("medium")
    o = zvoracle.Oracle(tensors)
    T, hop = 600, g.hop_size
    H = ph.receptive_radius(g, tensors)
    assert H == 20
    mel = synth.vocoder_mel(g, tensors, 61, T)
    for order in (zvoracle.ORDER_GGML_AVX2, zvoracle.ORDER_SEQ_F32):
        o.set_order(order)
        full = o.vocoder(mel)
        for a, b in ((0, 64), (300, 364), (T - 64, T)):
            w = ph.window_of_oracle(o.vocoder, mel, a, b, H, hop)
            assert w.shape == ((b - a) * hop,) and np.array_equal(w, full[a * hop:b * hop]), (order, a, b)
        # the comparison can tell: without the context the window's edges differ
        w = ph.window_of_oracle(o.vocoder, mel, 300, 364, 0, hop)
        assert not np.array_equal(w, full[300 * hop:364 * hop]), order
