"""What a pitch track costs on the benchmark's own batch (BASELINE.json configs[3], built as scripts/fitted_ab.py builds it: 32
utterances, capacity 1 024 frames each), hipGraph replay, two batches in flight as bench.py keeps them:

  P   the plain batch (zv_synthesize_batch_begin / _end);
  F   the same batch with a pitch track, frames and phonemes, default parameters, on every utterance (zv_synthesize_batch_begin_pitch).

The two alternate round by round in one process, every round `steps` pipelined steps; the difference of the medians is the two new
launches per tail group, the two downloads per group and the hand-out in _end.  Then the event-timed `voc_pitch_frames` /
`voc_pitch_phonemes` entries of zv_profile_end over a few eager, profiled runs of a batch that carries a pitch track, a contour AND a
volume, so that `voc_contour_frames` and `voc_level_apply` — passes over the same waveform that are bound by memory and by f64
conversions — are timed in the same runs.  The frames pass is reported as multiply-adds per second (window x lags per frame of
capacity, from the shapes) and against the two roofs it could meet, both taken from the chip's constants, not from this run:
  the vector ALU  v_dot2_i32_i16 is two multiply-adds per lane; a wave64 instruction takes 2 cycles of its SIMD: 256 multiply-adds per
                  clock and CU, 256 CUs, 2.4 GHz: 157.3e12 multiply-adds per second if every vector instruction were a dot product;
  the LDS         ds_read_b32 delivers 128 bytes per clock and CU: 78.6e12 bytes per second; the kernel reads 4 new dwords per lane
                  per 8 samples and lag block.

usage (GPU box):  python scripts/pitch_ab.py [--steps 24] [--rounds 7] [--out FILE]
profiles/pitch_ab.txt holds this output behind the bench.py rounds against the parent commit's library (scripts/ab_lib.sh)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from fitted_ab import summary, workload  # noqa: E402

VALU_MACS_PER_S = 256 * 256 * 2.4e9          # v_dot2_i32_i16 on every issue slot of every SIMD
LDS_B32_BYTES_PER_S = 128 * 256 * 2.4e9      # ds_read_b32, every CU


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
    hop, sr = model.hp.audio_hop_size, model.hp.audio_sampling_rate
    nfs = [nf for _, nf in model.synthesize_batch(utts)]
    model.set_graph_mode(True)
    arms = {"P": [model.prepare_batch(utts) for _ in range(2)], "F": [model.prepare_batch(utts, return_pitch=True) for _ in range(2)]}

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
    assert all(p.frames[:, 1].any() and p.frames.shape == (u[3], 2) and p.phonemes.shape == (len(u[0]), 2) for p, u in zip(arms["F"][0].pitches, utts))
    voiced = sum(int((p.frames[:, 0] > 0).sum()) for p in arms["F"][0].pitches)
    frames, tokens = sum(u[3] for u in utts), sum(len(u[0]) for u in utts)
    lo, hi, window = sr // 441, sr // 63, 2 * hop
    lags = hi - lo + 3
    macs = float(frames) * window * lags
    lines = ["# scripts/pitch_ab.py: bench.py's batch (%d utterances x %d frames of capacity, %d frames of speech, %d phonemes), two batches in "
             "flight, hipGraph replay; %d rounds of %d steps per arm, arms alternating, one MI355X box, one process" %
             (len(utts), utts[0][3], sum(nfs), tokens, args.rounds, args.steps),
             "# P: plain batch; F: a pitch track on every utterance, both tables, default parameters (lags %d .. %d, window %d: %d lags x %d "
             "samples = %d multiply-adds per frame, %.3e per step; %d frame rows and %d phoneme rows of 8 bytes come back per step; %d frames voiced)" %
             (lo, hi, window, lags, window, lags * window, macs, frames, tokens, voiced)]
    for name in arms:
        lines.append("%s ms_per_step  %s   rounds: %s" % (name, summary(ms[name]), " ".join("%.3f" % x for x in ms[name])))
    d = statistics.median(ms["F"]) - statistics.median(ms["P"])
    lines.append("# F - P (medians): %+.3f ms per step = %+.1f us; P's own spread %.3f ms" % (d, d * 1e3, max(ms["P"]) - min(ms["P"])))
    # the launches, event-timed: eager, profiled, one synchronous batch per pass (one tail group under a profile)
    model.set_graph_mode(False)
    call = model.prepare_batch(utts, return_pitch=True, return_contour=True, volume=[capi.Volume.from_db(target_dbfs=-20, peak_dbfs=-1)] * len(utts))
    call.run()
    model.profile_begin()
    for _ in range(args.profiled):
        call.run()
    stats = {s["name"]: s for s in model.profile_end()}
    per = {}
    for name in ("voc_level_apply", "voc_contour_frames", "voc_pitch_frames", "voc_pitch_phonemes"):
        s = stats[name]
        us, by = s["total_ms"] * 1e3 / s["launches"], s["algo_bytes"] / s["launches"]
        assert s["launches"] == args.profiled, (name, s)
        per[name] = us
        lines.append("%-20s %8.2f us per launch  %8.2f MB  %7.1f GB/s   (%d launches, event-timed, eager)" % (name, us, by / 1e6, by / us / 1e3, s["launches"]))
    t = per["voc_pitch_frames"] * 1e-6
    lds_bytes = float(frames) * ((window + 7) // 8) * 64 * 16            # 4 new dwords per lane and block of 8 samples
    lines.append("# voc_pitch_frames: %.3e multiply-adds in %.2f us = %.2fe12 per second = %.1f %% of the vector ALU's %.1fe12 (v_dot2_i32_i16 on every "
                 "issue slot); its window reads, %.2f GB of ds_read_b32 per launch, are %.1f %% of the LDS's %.1fe12 bytes per second" %
                 (macs, per["voc_pitch_frames"], macs / t / 1e12, 100.0 * macs / t / VALU_MACS_PER_S, VALU_MACS_PER_S / 1e12, lds_bytes / 1e9,
                  100.0 * lds_bytes / t / LDS_B32_BYTES_PER_S, LDS_B32_BYTES_PER_S / 1e12))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    model.close()


if __name__ == "__main__":
    main()
