"""What target durations cost on the benchmark's own batch (BASELINE.json configs[3], built as scripts/fitted_ab.py builds it: 32
utterances, capacity 1 024 frames each), hipGraph replay, one synchronous zv_synthesize_batch* call per step:

  T   every utterance with a target (zv_synthesize_batch_target): 9/10 of its uncontrolled frame count;
  F   the same batch at the parent's capability: the durations T produced, forced through duration_frames
      (zv_synthesize_batch_phonemes) — the same control rows, the same regulator input, one launch fewer.

The two alternate step by step in one process; the difference of the medians is the one new launch (fit_durations_kernel).  Then the
event-timed `enc_fit_durations` entry of zv_profile_end over a few eager, profiled runs of T.

usage (GPU box):  python scripts/fit_durations_ab.py [--steps 24] [--out profiles/fit_durations_ab.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402

from fitted_ab import summary, workload  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--profiled", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    capi, synth, g, ckpt, utts = workload()
    model = capi.Model(ckpt, device=0)
    nfs = [nf for _, nf in model.synthesize_batch(utts)]
    targets = [max(1, 9 * nf // 10) for nf in nfs]
    tb = model.prepare_batch([u + (None, None, t) for u, t in zip(utts, targets)], durations=True)
    tb.run()
    durs = [d.copy() for d in tb.durations]
    assert [n for _, n in tb.results()] == targets and [int(d.sum()) for d in durs] == targets
    want = [w.copy() for w, _ in tb.results()]
    fb = model.prepare_batch([u + (None, dict(duration_frames=d)) for u, d in zip(utts, durs)], durations=True)
    model.set_graph_mode(True)
    arms = {"T": tb, "F": fb}
    ms = {"T": [], "F": []}
    for k in range(2 * (args.warmup + args.steps)):
        name = "TF"[k % 2]
        model.synchronize()
        t0 = time.perf_counter()
        arms[name].run()
        dt = 1e3 * (time.perf_counter() - t0)
        if k >= 2 * args.warmup:
            ms[name].append(dt)
    for name, bc in arms.items():
        for (w, n), wr, t in zip(bc.results(), want, targets):
            assert n == t and np.array_equal(w, wr), "the two arms must produce the same audio"
    # the kernel alone: HIP events around every launch of an eager run
    model.set_graph_mode(False)
    fit_ms, enc_ms, launches = [], [], 0
    for _ in range(args.profiled):
        model.profile_begin()
        tb.run()
        stats = model.profile_end()
        mine = [s for s in stats if s["name"] == "enc_fit_durations"]
        assert len(mine) == 1, [s["name"] for s in stats]
        launches = mine[0]["launches"]
        fit_ms.append(mine[0]["total_ms"])
        enc_ms.append(sum(s["total_ms"] for s in stats if s["name"].startswith("enc_")))
    model.close()
    mt, mf = statistics.median(ms["T"]), statistics.median(ms["F"])
    out = ["target durations on the benchmark batch (BASELINE.json configs[3]: %d utterances of %d .. %d phonemes, capacity %d frames each;"
           % (len(utts), min(len(u[0]) for u in utts), max(len(u[0]) for u in utts), utts[0][3]),
           "targets = 9/10 of each utterance's uncontrolled frame count, %d frames in all), hipGraph replay, one synchronous call per step," % sum(targets),
           "%d steps per arm after %d warm-up steps, the arms alternating step by step in one process" % (args.steps, args.warmup), "",
           "T  zv_synthesize_batch_target                        ms/step: %s" % summary(ms["T"]),
           "F  zv_synthesize_batch_phonemes, the same durations forced  ms/step: %s" % summary(ms["F"]), "",
           "T - F = %+.3f ms (medians) = %+.2f %% of F; the spreads of the arms: %.3f and %.3f ms" %
           (mt - mf, 100.0 * (mt - mf) / mf, max(ms["T"]) - min(ms["T"]), max(ms["F"]) - min(ms["F"])), "",
           "enc_fit_durations (zv_profile_end, HIP events, eager, %d launch per run, %d profiled runs)  ms: %s" %
           (launches, args.profiled, summary(fit_ms)),
           "all enc_* entries of the same runs                                                      ms: %s" % summary(enc_ms)]
    text = "\n".join(out) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
