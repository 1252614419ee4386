"""What a level contour costs on the benchmark's own batch (BASELINE.json configs[3], built as scripts/fitted_ab.py builds it: 32
utterances, capacity 1 024 frames each), hipGraph replay, two batches in flight as bench.py keeps them:

  P   the plain batch (zv_synthesize_batch_begin / _end);
  C   the same batch with a contour, frames and phonemes, on every utterance (zv_synthesize_batch_begin_contour).

The two alternate round by round in one process, every round `steps` pipelined steps; the difference of the medians is the two new
launches per tail group, the two downloads per group and the hand-out in _end.  Then the event-timed `voc_contour_frames` /
`voc_contour_phonemes` entries of zv_profile_end over a few eager, profiled runs of a batch that carries a contour AND a volume, so that
`voc_level_apply` — the yardstick of the frames pass: the same grid, the same bytes read, and as many written again — is timed in the
same runs.

usage (GPU box):  python scripts/contour_ab.py [--steps 24] [--rounds 7] [--out FILE]
profiles/contour_ab.txt holds this output behind the bench.py rounds against the parent commit's library (scripts/ab_lib.sh)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from fitted_ab import summary, workload  # noqa: E402


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
    hop = model.hp.audio_hop_size
    nfs = [nf for _, nf in model.synthesize_batch(utts)]
    model.set_graph_mode(True)
    arms = {"P": [model.prepare_batch(utts) for _ in range(2)], "C": [model.prepare_batch(utts, return_contour=True) for _ in range(2)]}

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
    assert [n for _, n in arms["C"][0].results()] == nfs
    assert all(c.frames[:nf, 1].all() and c.phonemes.any() for c, nf in zip(arms["C"][0].contours, nfs))
    frames, tokens = sum(u[3] for u in utts), sum(len(u[0]) for u in utts)
    lines = ["# scripts/contour_ab.py: bench.py's batch (%d utterances x %d frames of capacity, %d frames of speech, %d phonemes), two batches in "
             "flight, hipGraph replay; %d rounds of %d steps per arm, arms alternating, one MI355X box, one process" %
             (len(utts), utts[0][3], sum(nfs), tokens, args.rounds, args.steps),
             "# P: plain batch; C: a contour on every utterance, both tables (%d frame rows and %d phoneme rows of 8 bytes come back per step)" %
             (frames, tokens)]
    for name in arms:
        lines.append("%s ms_per_step  %s   rounds: %s" % (name, summary(ms[name]), " ".join("%.3f" % x for x in ms[name])))
    d = statistics.median(ms["C"]) - statistics.median(ms["P"])
    lines.append("# C - P (medians): %+.3f ms per step = %+.1f us; P's own spread %.3f ms" % (d, d * 1e3, max(ms["P"]) - min(ms["P"])))
    # the launches, event-timed: eager, profiled, one synchronous batch per pass (one tail group under a profile)
    model.set_graph_mode(False)
    call = model.prepare_batch(utts, return_contour=True, volume=[capi.Volume.from_db(target_dbfs=-20, peak_dbfs=-1)] * len(utts))
    call.run()
    model.profile_begin()
    for _ in range(args.profiled):
        call.run()
    stats = {s["name"]: s for s in model.profile_end()}
    per = {}
    for name in ("voc_level_measure", "voc_level_apply", "voc_contour_frames", "voc_contour_phonemes"):
        s = stats[name]
        us, by = s["total_ms"] * 1e3 / s["launches"], s["algo_bytes"] / s["launches"]
        assert s["launches"] == args.profiled, (name, s)
        per[name] = us
        lines.append("%-20s %7.2f us per launch  %8.2f MB  %7.1f GB/s   (%d launches, event-timed, eager)" % (name, us, by / 1e6, by / us / 1e3, s["launches"]))
    assert stats["voc_contour_frames"]["algo_bytes"] == args.profiled * 4.0 * frames * hop
    lines.append("# voc_contour_frames against its yardstick voc_level_apply (same grid, the same bytes read, same runs): %.2fx the time" %
                 (per["voc_contour_frames"] / per["voc_level_apply"]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    model.close()


if __name__ == "__main__":
    main()
