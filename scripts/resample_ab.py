"""What resampling costs (include/zerovox_amd.h "resampling"): the event-timed entries of zv_profile_end for the two launches (`resample`,
`resample_reduce`) and the wall time of the call on the host, for one utterance of 1 024 frames and a batch of 32 such utterances (ONE
launch per kernel), at the default design, for 22050 -> 48000 and 22050 -> 8000, f32 and dithered PCM16 out.  `voc_filter` at 255 taps
over bench.py's batch stands next to them in the same run: the yardstick for f64 multiply-adds per second.  The yardstick of the call is
csrc/resample.h's host reference over the same samples, built -O2 (tests/native/resample_check.cpp bench), on one core of the same box.

usage (GPU box):  python scripts/resample_ab.py [--profiled 9] [--out FILE]
profiles/resample_ab.txt holds this output behind the bench.py rounds against the parent commit's library (scripts/ab_lib.sh)."""
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

KERNELS = ("resample", "resample_reduce")
F = np.float32
F64_MACS_PER_S = 39.3e12      # the vector f64 rate of the data sheet, 78.6 TFLOP/s, as multiply-adds (scripts/filter_ab.py)
TAPS = 255


def host_reference(L, M, P, n, reps):
    """ms of the host reference over n samples, the least of reps runs"""
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "resample_check")
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "zerovox.cpp_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "resample_check.cpp"), "-o", exe], check=True, timeout=600)
        out = subprocess.run([exe, "bench", str(L), str(M), str(P), str(n), str(reps)], check=True, capture_output=True, text=True, timeout=900).stdout
    return float(out.split()[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profiled", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    capi, synth, g, ckpt, utts = workload()
    model = capi.Model(ckpt, device=0)
    model.set_graph_mode(False)
    hop, rate = model.hp.audio_hop_size, model.hp.audio_sampling_rate
    rng = np.random.default_rng(5)
    wavs = [(rng.standard_normal(1024 * hop) * 0.1).astype(F) for _ in range(32)]
    lines = ["# scripts/resample_ab.py: resampling, eager, event-timed, %d profiled calls per shape, one MI355X box, one process; %d Hz, hop %d, "
             "1 024 frames = %d samples per utterance; noise of sigma 0.1; f32 and dithered PCM16 out" % (args.profiled, rate, hop, 1024 * hop)]
    for rate_out in (48000, 8000):
        L, M, table = capi.resample_design(rate, rate_out)
        P = table.shape[1]
        q = capi.Resample(rate, rate_out, dither=True, seed=1)
        host_one = host_reference(L, M, P, 1024 * hop, 3)
        for name, ws in (("one utterance of 1024 frames", wavs[:1]), ("32 x 1024 frames", wavs)):
            n = len(ws)
            call = (lambda: model.resample_wave_batch(ws, q, pcm=True)) if n > 1 else (lambda: model.resample_wave(ws[0], q, pcm=True))
            first = call()                                       # (the I/O block's growth and the design happen here)
            if n > 1:
                one = model.resample_wave(ws[5], capi.Resample(rate, rate_out, dither=True, seed=6), pcm=True)
                assert repr(one[0]) == repr(first[5][0]) and np.array_equal(one[1], first[5][1]) and np.array_equal(one[2], first[5][2])
            n_out = sum(r[0].n_out for r in first) if n > 1 else first[0].n_out
            model.profile_begin()
            wall = []
            for _ in range(args.profiled):
                t0 = time.perf_counter()
                call()
                wall.append((time.perf_counter() - t0) * 1e3)
            stats = {s["name"]: s for s in model.profile_end()}
            lines.append("## %s, %d -> %d Hz (L %d, M %d, %d taps per phase): %d outputs, %.3e f64 multiply-adds" % (name, rate, rate_out, L, M, P, n_out, n_out * P))
            total = 0.0
            for k in KERNELS:
                s = stats[k]
                assert s["launches"] == args.profiled, (k, s)     # ONE launch per kernel per call: the batch is one launch group
                ms = s["total_ms"] / s["launches"]
                total += ms
                lines.append("%-17s %10.3f ms per launch   (%d launches, event-timed, eager)" % (k, ms, s["launches"]))
            t = stats["resample"]["total_ms"] / args.profiled * 1e-3
            lines.append("# resample: %.2fe12 f64 multiply-adds per second = %.1f %% of the vector f64 rate's %.1fe12 (a constant from the data sheet, not "
                         "measured here)" % (n_out * P / t / 1e12, 100.0 * n_out * P / t / F64_MACS_PER_S, F64_MACS_PER_S / 1e12))
            w = float(np.median(wall))
            lines.append("# the launches together %.3f ms; the call, wall time on the host (uploads from pageable memory, the launches, the downloads): "
                         "median %.3f ms, min %.3f, max %.3f" % (total, w, min(wall), max(wall)))
            lines.append("# the host reference (one core, -O2): %d x %.3f = %.3f ms: %.1f times the call, %.1f times the launches"
                         % (n, host_one, n * host_one, n * host_one / w, n * host_one / total))
    # the yardstick: the waveform filter at 255 taps over bench.py's batch, event-timed in the same run
    gains_db = np.random.default_rng(1).uniform(-12.0, 12.0, 16)
    call = model.prepare_batch(utts, filter=[capi.Filter.from_band_gains_db(gains_db, None, TAPS) for _ in utts])
    call.run()
    model.profile_begin()
    for _ in range(args.profiled):
        call.run()
    s = {s["name"]: s for s in model.profile_end()}["voc_filter"]
    samples = sum(u[3] for u in utts) * hop
    t = s["total_ms"] / s["launches"] * 1e-3
    lines.append("## the yardstick: voc_filter at %d taps over %d utterances x %d frames (%d samples), same run" % (TAPS, len(utts), utts[0][3], samples))
    lines.append("%-17s %10.3f ms per launch   (%d launches, event-timed, eager): %.2fe12 f64 multiply-adds per second = %.1f %% of the vector f64 rate"
                 % ("voc_filter", t * 1e3, s["launches"], samples * TAPS / t / 1e12, 100.0 * samples * TAPS / t / F64_MACS_PER_S))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    model.close()


if __name__ == "__main__":
    main()
