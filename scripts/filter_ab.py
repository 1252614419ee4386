"""What the waveform filter costs on the benchmark's own batch (BASELINE.json configs[3], built as scripts/fitted_ab.py builds it: 32
utterances, capacity 1 024 frames each), hipGraph replay, two batches in flight as bench.py keeps them:

  P   the plain batch (zv_synthesize_batch_begin / _end);
  F   the same batch with a 255-tap filter on every utterance (zv_synthesize_batch_begin_filter).

The two alternate round by round in one process, every round `steps` pipelined steps; the difference of the medians is the one new
launch per tail group and the 2 KB of taps per utterance in the input block.  Then the event-timed `voc_filter` entry of
zv_profile_end over a few eager, profiled runs of a batch that carries the filter, an envelope AND band levels, so that
`voc_env_apply` — the other write pass over the same waveform — and `voc_bands_frames` are timed in the same runs.  The pass is
reported as f64 multiply-adds per second (samples of the capacity x taps) and against the vector f64 rate.  That roof is a CONSTANT
taken from the chip's data sheet, not a measurement of this run: 78.6e12 FLOP/s, i.e. 39.3e12 multiply-adds per second.  The profiled
runs are repeated at 33 and 511 taps: a pass bound by its multiply-adds scales with the taps, one bound by its samples does not.

usage (GPU box):  python scripts/filter_ab.py [--steps 24] [--rounds 7] [--out FILE]      (--rounds 0: the event-timed launches alone)
profiles/filter_ab.txt holds this output behind the bench.py rounds against the parent commit's library (scripts/ab_lib.sh)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from fitted_ab import summary, workload  # noqa: E402

F64_MACS_PER_S = 39.3e12                   # vector f64: 78.6e12 FLOP/s on the data sheet
TAPS = 255


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--profiled", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    capi, synth, g, ckpt, utts = workload()
    model = capi.Model(ckpt, device=0)
    nfs = [nf for _, nf in model.synthesize_batch(utts)]
    rng = np.random.default_rng(1)
    gains_db = rng.uniform(-12.0, 12.0, 16)

    def filters(n_taps):
        return [capi.Filter.from_band_gains_db(gains_db, None, n_taps) for _ in utts]

    model.set_graph_mode(True)
    arms = {"P": [model.prepare_batch(utts) for _ in range(2)], "F": [model.prepare_batch(utts, filter=filters(TAPS)) for _ in range(2)]}

    def run_steps(lanes, k_steps):                       # bench.py's loop: step k is enqueued before step k - 1 is waited for
        for k in range(k_steps):
            lanes[k % 2].begin(k % 2)
            if k >= 1:
                lanes[(k - 1) % 2].end((k - 1) % 2)
        lanes[(k_steps - 1) % 2].end((k_steps - 1) % 2)

    ms = {name: [] for name in arms}
    for name, lanes in arms.items():
        run_steps(lanes, max(args.warmup, 2))
    if args.rounds == 0:                                 # --rounds 0: the event-timed launches alone
        for name in arms:
            ms[name] = [float("nan")]
    for _ in range(args.rounds):
        for name, lanes in arms.items():
            model.synchronize()
            t0 = time.perf_counter()
            run_steps(lanes, args.steps)
            model.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / args.steps)
    assert [n for _, n in arms["F"][0].results()] == nfs
    plain, filtered = arms["P"][0].results(), arms["F"][0].results()
    assert all(np.isfinite(w).all() and not np.array_equal(w, p) for (w, _), (p, _) in zip(filtered, plain))
    hop = model.hp.audio_hop_size
    samples = sum(u[3] for u in utts) * hop
    macs = float(samples) * TAPS
    lines = ["# scripts/filter_ab.py: bench.py's batch (%d utterances x %d frames of capacity, %d frames of speech), two batches in "
             "flight, hipGraph replay; %d rounds of %d steps per arm, arms alternating, one MI355X box, one process" %
             (len(utts), utts[0][3], sum(nfs), args.rounds, args.steps),
             "# P: plain batch; F: a %d-tap filter on every utterance (%d samples of capacity x %d taps = %.3e f64 multiply-adds per step)" %
             (TAPS, samples, TAPS, macs)]
    for name in arms:
        lines.append("%s ms_per_step  %s   rounds: %s" % (name, summary(ms[name]), " ".join("%.3f" % x for x in ms[name])))
    d = statistics.median(ms["F"]) - statistics.median(ms["P"])
    lines.append("# F - P (medians): %+.3f ms per step = %+.1f us; P's own spread %.3f ms" % (d, d * 1e3, max(ms["P"]) - min(ms["P"])))
    # the launches, event-timed: eager, profiled, one synchronous batch per pass (one tail group under a profile)
    model.set_graph_mode(False)
    envs = [capi.Envelope(np.linspace(0.5, 2.0, len(u[0])).astype(np.float32), 2, 100, 100) for u in utts]
    for n_taps in (TAPS, 33, 511):
        call = model.prepare_batch(utts, filter=filters(n_taps), envelope=envs, return_bands=True)
        call.run()
        model.profile_begin()
        for _ in range(args.profiled):
            call.run()
        stats = {s["name"]: s for s in model.profile_end()}
        lines.append("# %d taps:" % n_taps)
        per = {}
        for name in ("voc_filter", "voc_env_apply", "voc_bands_frames"):
            s = stats[name]
            us, by = s["total_ms"] * 1e3 / s["launches"], s["algo_bytes"] / s["launches"]
            assert s["launches"] == args.profiled, (name, s)
            per[name] = us
            lines.append("%-20s %8.2f us per launch  %8.2f MB  %7.1f GB/s   (%d launches, event-timed, eager)" % (name, us, by / 1e6, by / us / 1e3, s["launches"]))
        t, mac = per["voc_filter"] * 1e-6, float(samples) * n_taps
        lines.append("# voc_filter: %.3e f64 multiply-adds in %.2f us = %.2fe12 per second = %.1f %% of the vector f64 rate's %.1fe12 (a constant from "
                     "the data sheet, not measured here)" % (mac, per["voc_filter"], mac / t / 1e12, 100.0 * mac / t / F64_MACS_PER_S, F64_MACS_PER_S / 1e12))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    model.close()


if __name__ == "__main__":
    main()
