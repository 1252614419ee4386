"""What band levels cost on the benchmark's own batch (BASELINE.json configs[3], built as scripts/fitted_ab.py builds it: 32
utterances, capacity 1 024 frames each), hipGraph replay, two batches in flight as bench.py keeps them:

  P   the plain batch (zv_synthesize_batch_begin / _end);
  F   the same batch with band levels, frames and phonemes, the 16 default bands, on every utterance (zv_synthesize_batch_begin_bands).

The two alternate round by round in one process, every round `steps` pipelined steps; the difference of the medians is the two new
launches per tail group, the two downloads per group and the hand-out in _end.  Then the event-timed `voc_bands_frames` /
`voc_bands_phonemes` entries of zv_profile_end over a few eager, profiled runs of a batch that carries band levels, a pitch track AND a
contour, so that `voc_pitch_frames` and `voc_contour_frames` — passes over the same waveform — are timed in the same runs.  The frames
pass is reported as 8-bit multiply-adds per second, both digit planes counted (frames x 1 024 samples x 1 026 columns x 2), against the
i8 matrix rate.  That roof is a CONSTANT taken from the chip's data sheet, not a measurement of this run: twice the dense bf16 rate
of 2.5e15 FLOP/s, i.e. 2.5e15 8-bit multiply-adds per second.  The table stream is reported likewise: the workgroups of a launch each
read the whole fragment table (bands.h BANDS_TABLE_BYTES) once, from L2 or beyond.

usage (GPU box):  python scripts/bands_ab.py [--steps 24] [--rounds 7] [--out FILE]
profiles/bands_ab.txt holds this output behind the bench.py rounds against the parent commit's library (scripts/ab_lib.sh)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from fitted_ab import summary, workload  # noqa: E402

I8_MACS_PER_S = 2.5e15                     # dense i8 MFMA: twice the bf16 rate of 2.5e15 FLOP/s (1.25e15 multiply-adds per second)
TILE_FRAMES, TABLE_BYTES = 32, 2 * 34 * 16 * 64 * 16      # bands.h BANDS_TILE_FRAMES, BANDS_TABLE_BYTES


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
    model.set_graph_mode(True)
    arms = {"P": [model.prepare_batch(utts) for _ in range(2)], "F": [model.prepare_batch(utts, return_bands=True) for _ in range(2)]}

    def run_steps(lanes, k_steps):                       # bench.py's loop: step k is enqueued before step k - 1 is waited for
        for k in range(k_steps):
            lanes[k % 2].begin(k % 2)
            if k >= 1:
                lanes[(k - 1) % 2].end((k - 1) % 2)
        lanes[(k_steps - 1) % 2].end((k_steps - 1) % 2)

    ms = {name: [] for name in arms}
    for name, lanes in arms.items():
        run_steps(lanes, max(args.warmup, 2))
    for _ in range(args.rounds):
        for name, lanes in arms.items():
            model.synchronize()
            t0 = time.perf_counter()
            run_steps(lanes, args.steps)
            model.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / args.steps)
    assert [n for _, n in arms["F"][0].results()] == nfs
    assert all(b.frames.any() and b.frames.shape == (u[3], 16) and b.phonemes.shape == (len(u[0]), 16) for b, u in zip(arms["F"][0].bands, utts))
    frames, tokens = sum(u[3] for u in utts), sum(len(u[0]) for u in utts)
    macs = float(frames) * 1024 * 1026 * 2
    lines = ["# scripts/bands_ab.py: bench.py's batch (%d utterances x %d frames of capacity, %d frames of speech, %d phonemes), two batches in "
             "flight, hipGraph replay; %d rounds of %d steps per arm, arms alternating, one MI355X box, one process" %
             (len(utts), utts[0][3], sum(nfs), tokens, args.rounds, args.steps),
             "# P: plain batch; F: band levels on every utterance, both tables, the 16 default bands (1 024 samples x 1 026 columns x 2 digit "
             "planes = %d 8-bit multiply-adds per frame, %.3e per step; %d frame rows and %d phoneme rows of 64 floats come back per step)" %
             (1024 * 1026 * 2, macs, frames, tokens)]
    for name in arms:
        lines.append("%s ms_per_step  %s   rounds: %s" % (name, summary(ms[name]), " ".join("%.3f" % x for x in ms[name])))
    d = statistics.median(ms["F"]) - statistics.median(ms["P"])
    lines.append("# F - P (medians): %+.3f ms per step = %+.1f us; P's own spread %.3f ms" % (d, d * 1e3, max(ms["P"]) - min(ms["P"])))
    # the launches, event-timed: eager, profiled, one synchronous batch per pass (one tail group under a profile)
    model.set_graph_mode(False)
    call = model.prepare_batch(utts, return_bands=True, return_pitch=True, return_contour=True)
    call.run()
    model.profile_begin()
    for _ in range(args.profiled):
        call.run()
    stats = {s["name"]: s for s in model.profile_end()}
    per = {}
    for name in ("voc_contour_frames", "voc_pitch_frames", "voc_bands_frames", "voc_bands_phonemes"):
        s = stats[name]
        us, by = s["total_ms"] * 1e3 / s["launches"], s["algo_bytes"] / s["launches"]
        assert s["launches"] == args.profiled, (name, s)
        per[name] = us
        lines.append("%-20s %8.2f us per launch  %8.2f MB  %7.1f GB/s   (%d launches, event-timed, eager)" % (name, us, by / 1e6, by / us / 1e3, s["launches"]))
    t = per["voc_bands_frames"] * 1e-6
    stream = float(frames) / TILE_FRAMES * TABLE_BYTES
    lines.append("# voc_bands_frames: %.3e 8-bit multiply-adds in %.2f us = %.2fe12 per second = %.1f %% of the i8 matrix rate's %.0fe12 (a constant: twice "
                 "the dense bf16 rate, not measured here); its table stream, %.2f GB per launch (%d workgroups x %.2f MB), runs at %.2f TB/s" %
                 (macs, per["voc_bands_frames"], macs / t / 1e12, 100.0 * macs / t / (I8_MACS_PER_S), I8_MACS_PER_S / 1e12, stream / 1e9,
                  frames // TILE_FRAMES, TABLE_BYTES / 1e6, stream / t / 1e12))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    model.close()


if __name__ == "__main__":
    main()
