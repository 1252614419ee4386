"""What mel alignment costs (include/zerovox_amd.h "mel alignment"): the event-timed entries of zv_profile_end for the five kernels
(`align_means`, `align_quant`, `align_cost`, `align_dp`, `align_walk`) and the wall time of the call on the host, for one
1 024 x 1 024 x 80 pair, a batch of 32 such pairs (ONE launch per kernel) and one 4 096 x 4 096 x 80 pair.  The yardstick of the call
is csrc/align.h's host reference on rows of the same sizes, built -O2 (tests/native/align_check.cpp bench), on one core of the same
box; the ratio is stated per shape and per step, so a kernel that is slower than the host's step shows.  The cost kernel's 8-bit
multiply-add rate (four digit-plane products over K = M rounded up to 64 channels per cell) is set next to `mel_frames`'s rate over
32 x 1 024 frames of noise in the same process, both against the i8 matrix rate, a CONSTANT from the chip's data sheet.  Last,
synthesize_like on a reference the model made itself with forced durations D*: the sum of |d_b - D*| is reported, not judged (the
synthetic weights promise nothing about it).

usage (GPU box):  python scripts/mel_align_ab.py [--profiled 9] [--out FILE]
profiles/mel_align_ab.txt holds this output behind the bench.py rounds against the parent commit's library (scripts/ab_lib.sh)."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from fitted_ab import workload  # noqa: E402

I8_MACS_PER_S = 2.5e15                     # dense i8 MFMA: twice the bf16 rate of 2.5e15 FLOP/s
KERNELS = ("align_means", "align_quant", "align_cost", "align_dp", "align_walk")
F = np.float32


def pair(seed, Ta, Tb, M):
    """mel-like rows and a re-timed, noisy take of them"""
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal((Ta, M)) * 1.5 - 4.0 + np.cumsum(rng.standard_normal((Ta, 1)) * 0.3, axis=0)).astype(F)
    b = a[np.sort(rng.integers(0, Ta, Tb))] + (rng.standard_normal((Tb, M)) * 0.2).astype(F)
    return a, b


def host_reference(Ta, Tb, M, reps):
    """ms of the host reference's steps (quantise, cost, path, walk), the least of reps runs"""
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "align_check")
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "zerovox.cpp_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "align_check.cpp"), "-o", exe], check=True, timeout=600)
        out = subprocess.run([exe, "bench", str(Ta), str(Tb), str(M), str(reps)], check=True, capture_output=True, text=True, timeout=900).stdout
    return [float(x) for x in out.split()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profiled", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    capi, synth, g, ckpt, utts = workload()
    model = capi.Model(ckpt, device=0)
    model.set_graph_mode(False)
    M = model.hp.audio_num_mels
    K = (M + 63) // 64 * 64
    p = capi.AlignParams(normalise=True)
    lines = ["# scripts/mel_align_ab.py: mel alignment, eager, event-timed, %d profiled calls per shape, one MI355X box, one process; M = %d (K = %d)"
             % (args.profiled, M, K)]
    shapes = (("one 1024 x 1024 pair", [pair(1, 1024, 1024, M)]), ("32 pairs of 1024 x 1024", [pair(10 + k, 1024, 1024, M) for k in range(32)]),
              ("one 4096 x 4096 pair", [pair(2, 4096, 4096, M)]))
    cost_rate = {}
    for name, pairs in shapes:
        call = (lambda: model.mel_align_batch(pairs, p)) if len(pairs) > 1 else (lambda: model.mel_align(*pairs[0], p))
        first = call()                                       # (the I/O block's growth happens here)
        if len(pairs) > 1:
            one = model.mel_align(*pairs[5], p)
            assert (one.total, one.distance, one.path_len) == (first[5].total, first[5].distance, first[5].path_len) and np.array_equal(one.map_a, first[5].map_a)
        model.profile_begin()
        wall = []
        for _ in range(args.profiled):
            t0 = time.perf_counter()
            call()
            wall.append((time.perf_counter() - t0) * 1e3)
        stats = {s["name"]: s for s in model.profile_end()}
        Ta, Tb = pairs[0][0].shape[0], pairs[0][1].shape[0]
        host = host_reference(Ta, Tb, M, 3 if Ta <= 1024 else 1)
        n = len(pairs)
        lines.append("## %s" % name)
        per = {}
        for k in KERNELS:
            s = stats[k]
            assert s["launches"] == args.profiled, (k, s)     # ONE launch per kernel per call: the batch is one launch group
            per[k] = s["total_ms"] / s["launches"]
            lines.append("%-12s %10.3f ms per launch   (%d launches, event-timed, eager)" % (k, per[k], s["launches"]))
        dev = {"quantise": per["align_means"] + per["align_quant"], "cost": per["align_cost"], "path": per["align_dp"], "walk": per["align_walk"]}
        for step, h in zip(("quantise", "cost", "path", "walk"), host):
            lines.append("# %-8s host reference %10.3f ms (%d x %.3f, one core, -O2)   device %8.3f ms   host / device = %.2f%s"
                         % (step, h * n, n, h, dev[step], h * n / dev[step], "" if h * n >= dev[step] else "   <- the device step is SLOWER than the host's"))
        w = float(np.median(wall))
        lines.append("# the call, wall time on the host (uploads from pageable memory, five launches, one download): median %.3f ms, min %.3f, max %.3f; "
                     "the host reference %.3f ms: %.1f times the call" % (w, min(wall), max(wall), sum(host) * n, sum(host) * n / w))
        macs = float(n) * Ta * Tb * K * 4
        cost_rate[name] = macs / (per["align_cost"] * 1e-3)
        lines.append("# align_cost: %.3e 8-bit multiply-adds in %.3f ms = %.2fe12 per second = %.2f %% of the i8 matrix rate's %.0fe12 (a constant, not "
                     "measured here); it stores %.1f MB of costs at %.1f GB/s" % (macs, per["align_cost"], cost_rate[name] / 1e12,
                                                                                 100.0 * cost_rate[name] / I8_MACS_PER_S, I8_MACS_PER_S / 1e12,
                                                                                 4.0 * n * Ta * Tb / 1e6, 4.0 * n * Ta * Tb / per["align_cost"] / 1e6))
    # mel_frames in the same process: 32 x 1 024 frames of noise
    hop = model.hp.audio_hop_size
    rng = np.random.default_rng(3)
    wavs = [(rng.standard_normal(1024 * hop) * 0.1).astype(F) for _ in range(32)]
    mp = capi.MelAnalysis(log="ln")
    model.mel_wave_batch(wavs, mp)
    model.profile_begin()
    for _ in range(args.profiled):
        model.mel_wave_batch(wavs, mp)
    s = {x["name"]: x for x in model.profile_end()}["mel_frames"]
    ms = s["total_ms"] / s["launches"]
    macs = 32.0 * 1024 * 1024 * 1026 * 4
    lines.append("## next to mel_frames (32 x 1024 frames of noise, the same process)")
    lines.append("# mel_frames: %.3e 8-bit multiply-adds in %.3f ms = %.2fe12 per second = %.2f %% of the i8 matrix rate; align_cost over 32 pairs: %.2fe12 "
                 "per second" % (macs, ms, macs / (ms * 1e-3) / 1e12, 100.0 * macs / (ms * 1e-3) / I8_MACS_PER_S, cost_rate["32 pairs of 1024 x 1024"] / 1e12))
    # synthesize_like on a self-made reference
    rng = np.random.default_rng(4)
    ids, puncts, style = utts[0][:3]
    n = len(ids)
    forced = rng.integers(2, 9, n).astype(np.int32)
    Tb = int(forced.sum())
    ref, nf = model.synthesize(ids, puncts, style, Tb, phonemes=dict(duration_frames=forced), fitted=True)
    assert nf == Tb
    t0 = time.perf_counter()
    wav, nf2, dur_b, al = model.synthesize_like(ids, puncts, style, model.hp.max_seq_len, ref[:Tb * hop])
    w = (time.perf_counter() - t0) * 1e3
    assert nf2 == Tb and dur_b.sum() == Tb
    lines.append("## synthesize_like on a reference the model made itself (%d phonemes, forced durations D* of 2 .. 8 frames, %d frames)" % (n, Tb))
    lines.append("# sum |d_b - D*| = %d frames over %d phonemes (largest %d); alignment: Ta = %d, path_len %d, distance %.4f; the whole call %.1f ms "
                 "(reported, not judged: synthetic weights)" % (int(np.abs(dur_b - forced).sum()), n, int(np.abs(dur_b - forced).max()), len(al.map_a),
                                                               al.path_len, al.distance, w))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    model.close()


if __name__ == "__main__":
    main()
