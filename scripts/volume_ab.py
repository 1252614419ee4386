"""What volume controls cost on the benchmark's own batch (BASELINE.json configs[3], built as scripts/fitted_ab.py builds it: 32
utterances, capacity 1 024 frames each), hipGraph replay, two batches in flight as bench.py keeps them:

  P   the plain batch (zv_synthesize_batch_begin / _end);
  V   the same batch with a volume on every utterance (zv_synthesize_batch_begin_volume): a loudness target and a peak ceiling.

The two alternate round by round in one process, every round `steps` pipelined steps; the difference of the medians is the two new
launches per tail group and the level rows' copy.  Then the event-timed `voc_level_measure` / `voc_level_apply` entries of
zv_profile_end over a few eager, profiled runs of V, with the bytes they moved (4 B per speech sample read; 8 B per capacity sample
read and written) and the rate that makes, next to the 5.1-5.6 TB/s the project's memory-bound convs reach (README.md).

usage (GPU box):  python scripts/volume_ab.py [--steps 24] [--rounds 7] [--out profiles/volume_cost.txt]"""
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
    vols = [capi.Volume.from_db(target_dbfs=-20, peak_dbfs=-1)] * len(utts)
    model.set_graph_mode(True)
    arms = {"P": [model.prepare_batch(utts) for _ in range(2)], "V": [model.prepare_batch(utts, volume=vols) for _ in range(2)]}

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
    assert [n for _, n in arms["V"][0].results()] == nfs
    gains = [lv.gain for lv in arms["V"][0].levels]
    lines = ["# scripts/volume_ab.py: bench.py's batch (%d utterances x %d frames of capacity, %d frames of speech), two batches in flight, "
             "hipGraph replay; %d rounds of %d steps per arm, arms alternating, one MI355X box, one process" %
             (len(utts), utts[0][3], sum(nfs), args.rounds, args.steps),
             "# P: plain batch; V: a loudness target (-20 dBFS) and a peak ceiling (-1 dBFS) on every utterance; gains applied %.3g .. %.3g" %
             (min(gains), max(gains))]
    for name in arms:
        lines.append("%s ms_per_step  %s   rounds: %s" % (name, summary(ms[name]), " ".join("%.3f" % x for x in ms[name])))
    d = statistics.median(ms["V"]) - statistics.median(ms["P"])
    lines.append("# V - P (medians): %+.3f ms per step = %+.1f us; P's own spread %.3f ms" % (d, d * 1e3, max(ms["P"]) - min(ms["P"])))
    # the two launches, event-timed: eager, profiled, one synchronous batch per pass (one tail group under a profile)
    model.set_graph_mode(False)
    call = arms["V"][0]
    call.run()
    model.profile_begin()
    for _ in range(args.profiled):
        call.run()
    stats = {s["name"]: s for s in model.profile_end()}
    want = {"voc_level_measure": 4.0 * sum(nfs) * hop, "voc_level_apply": 8.0 * sum(u[3] for u in utts) * hop}
    tot_us = tot_b = 0.0
    for name, b in want.items():
        s = stats[name]
        us, by = s["total_ms"] * 1e3 / s["launches"], s["algo_bytes"] / s["launches"]
        assert s["launches"] == args.profiled and by == b, (name, s, b)
        tot_us += us
        tot_b += by
        lines.append("%-18s %7.2f us per launch  %8.2f MB  %7.1f GB/s   (%d launches, event-timed, eager)" % (name, us, by / 1e6, by / us / 1e3, s["launches"]))
    lines.append("# both: %.2f us, %.2f MB, %.1f GB/s; at the 5.1-5.6 TB/s of the memory-bound convs %.2f MB take %.1f-%.1f us" %
                 (tot_us, tot_b / 1e6, tot_b / tot_us / 1e3, tot_b / 1e6, tot_b / 5.6e6, tot_b / 5.1e6))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    model.close()


if __name__ == "__main__":
    main()
