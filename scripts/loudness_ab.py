"""What loudness costs (include/zerovox_amd.h "loudness"): the event-timed entries of zv_profile_end for the six launches
(`loud_chunks_a`, `loud_states`, `loud_chunks_c`, `loud_peak`, `loud_gate`, `loud_apply`) and the wall time of the call on the host, for
one utterance of 1 024 frames and a batch of 32 such utterances (ONE launch per kernel), with and without the apply pass.  The
yardstick of the call is csrc/loudness.h's host reference over the same samples, built -O2 (tests/native/loudness_check.cpp bench), on
one core of the same box.

usage (GPU box):  python scripts/loudness_ab.py [--profiled 9] [--out FILE]
profiles/loudness_ab.txt holds this output behind the bench.py rounds against the parent commit's library (scripts/ab_lib.sh)."""
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

KERNELS = ("loud_chunks_a", "loud_states", "loud_chunks_c", "loud_peak", "loud_gate", "loud_apply")
F = np.float32


def host_reference(rate, n, reps):
    """ms of the host reference over n samples, the least of reps runs"""
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "loudness_check")
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "zerovox.cpp_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "loudness_check.cpp"), "-o", exe], check=True, timeout=600)
        out = subprocess.run([exe, "bench", str(rate), str(n), str(reps)], check=True, capture_output=True, text=True, timeout=900).stdout
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
    q = capi.Loudness.from_lufs(-16.0, true_peak_dbtp=-1.0)
    lines = ["# scripts/loudness_ab.py: loudness, eager, event-timed, %d profiled calls per shape, one MI355X box, one process; %d Hz, hop %d, "
             "1 024 frames = %d samples = %d chunks per utterance" % (args.profiled, rate, hop, 1024 * hop, -(-1024 * hop // 256))]
    host_one = host_reference(rate, 1024 * hop, 3)
    for name, ws, apply in (("one utterance of 1024 frames, meter", wavs[:1], False), ("one utterance of 1024 frames, normalised", wavs[:1], True),
                            ("32 x 1024 frames, meter", wavs, False), ("32 x 1024 frames, normalised", wavs, True)):
        n = len(ws)
        call = (lambda: model.loudness_wave_batch(ws, [q] * n, apply=apply)) if n > 1 else (lambda: model.loudness_wave(ws[0], q, apply=apply))
        first = call()                                       # (the I/O block's growth happens here)
        if n > 1:
            one = model.loudness_wave(ws[5], q, apply=apply)
            assert repr(one[0]) == repr(first[5][0]) and (not apply or np.array_equal(one[1], first[5][1]))
        model.profile_begin()
        wall = []
        for _ in range(args.profiled):
            t0 = time.perf_counter()
            call()
            wall.append((time.perf_counter() - t0) * 1e3)
        stats = {s["name"]: s for s in model.profile_end()}
        lines.append("## %s" % name)
        total = 0.0
        for k in KERNELS:
            if k not in stats:
                assert k == "loud_apply" and not apply, k
                continue
            s = stats[k]
            assert s["launches"] == args.profiled, (k, s)     # ONE launch per kernel per call: the batch is one launch group
            ms = s["total_ms"] / s["launches"]
            total += ms
            lines.append("%-14s %10.3f ms per launch   (%d launches, event-timed, eager)" % (k, ms, s["launches"]))
        w = float(np.median(wall))
        lines.append("# the launches together %.3f ms; the call, wall time on the host (uploads from pageable memory, the launches, the downloads): "
                     "median %.3f ms, min %.3f, max %.3f" % (total, w, min(wall), max(wall)))
        lines.append("# the host reference (a meter, one core, -O2): %d x %.3f = %.3f ms: %.1f times the call, %.1f times the launches"
                     % (n, host_one, n * host_one, n * host_one / w, n * host_one / total))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    model.close()


if __name__ == "__main__":
    main()
