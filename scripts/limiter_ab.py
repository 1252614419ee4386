"""What the limiter costs (include/zerovox_amd.h "limiter"): the event-timed entries of zv_profile_end for the five launches
(`limit_peak`, `limit_min`, `limit_mean`, `limit_peak_after`, `limit_reduce`) and the wall time of the call on the host, for one
utterance of 1 024 frames and a batch of 32 such utterances (ONE launch per kernel), at the default windows, at W = 3 and at
W = 8 192.  `loud_peak` and `loud_apply` of a normalising loudness call over the same waveforms stand next to them in the same run.  The
yardstick of the call is csrc/limiter.h's host reference over the same samples, built -O2 (tests/native/limiter_check.cpp bench), on one
core of the same box.

usage (GPU box):  python scripts/limiter_ab.py [--profiled 9] [--out FILE]
profiles/limiter_ab.txt holds this output behind the bench.py rounds against the parent commit's library (scripts/ab_lib.sh)."""
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

KERNELS = ("limit_peak", "limit_min", "limit_mean", "limit_peak_after", "limit_reduce")
LOUD = ("loud_peak", "loud_apply")
F = np.float32


def host_reference(rate, n, attack, release, reps):
    """ms of the host reference over n samples, the least of reps runs"""
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "limiter_check")
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "zerovox.cpp_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "limiter_check.cpp"), "-o", exe], check=True, timeout=600)
        out = subprocess.run([exe, "bench", str(rate), str(n), str(attack), str(release), str(reps)], check=True, capture_output=True, text=True,
                             timeout=900).stdout
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
    lines = ["# scripts/limiter_ab.py: limiter, eager, event-timed, %d profiled calls per shape, one MI355X box, one process; %d Hz, hop %d, "
             "1 024 frames = %d samples per utterance; noise of sigma 0.1 under gain 4 and ceiling 0.1 (most samples limited)"
             % (args.profiled, rate, hop, 1024 * hop)]
    windows = (("default windows", capi.limit_design(rate)), ("W = 3", (1, 1)), ("W = 8192", (2047, 6144)))
    for wname, (attack, release) in windows:
        q = capi.Limiter(4.0, 0.1, attack, release)
        host_one = host_reference(rate, 1024 * hop, attack, release, 3)
        for name, ws in (("one utterance of 1024 frames", wavs[:1]), ("32 x 1024 frames", wavs)):
            n = len(ws)
            call = (lambda: model.limit_wave_batch(ws, [q] * n)) if n > 1 else (lambda: model.limit_wave(ws[0], q))
            first = call()                                       # (the I/O block's growth happens here)
            if n > 1:
                one = model.limit_wave(ws[5], q)
                assert repr(one[0]) == repr(first[5][0]) and np.array_equal(one[1], first[5][1])
            model.profile_begin()
            wall = []
            for _ in range(args.profiled):
                t0 = time.perf_counter()
                call()
                wall.append((time.perf_counter() - t0) * 1e3)
            stats = {s["name"]: s for s in model.profile_end()}
            lines.append("## %s, %s (attack %d, release %d)" % (name, wname, attack, release))
            total = 0.0
            for k in KERNELS:
                s = stats[k]
                assert s["launches"] == args.profiled, (k, s)     # ONE launch per kernel per call: the batch is one launch group
                ms = s["total_ms"] / s["launches"]
                total += ms
                lines.append("%-17s %10.3f ms per launch   (%d launches, event-timed, eager)" % (k, ms, s["launches"]))
            w = float(np.median(wall))
            lines.append("# the launches together %.3f ms; the call, wall time on the host (uploads from pageable memory, the launches, the downloads): "
                         "median %.3f ms, min %.3f, max %.3f" % (total, w, min(wall), max(wall)))
            lines.append("# the host reference (one core, -O2): %d x %.3f = %.3f ms: %.1f times the call, %.1f times the launches"
                         % (n, host_one, n * host_one, n * host_one / w, n * host_one / total))
            if wname == "default windows":
                lq = capi.Loudness(4.0, None, 0.1)
                lcall = (lambda: model.loudness_wave_batch(ws, [lq] * n)) if n > 1 else (lambda: model.loudness_wave(ws[0], lq))
                lcall()
                model.profile_begin()
                for _ in range(args.profiled):
                    lcall()
                lstats = {s["name"]: s for s in model.profile_end()}
                for k in LOUD:
                    s = lstats[k]
                    lines.append("%-17s %10.3f ms per launch   (%d launches, a normalising loudness call over the same waveforms, same run)"
                                 % (k, s["total_ms"] / s["launches"], s["launches"]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    model.close()


if __name__ == "__main__":
    main()
