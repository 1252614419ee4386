"""What the stage calls over a batch buy, on the benchmark's own batch (BASELINE.json configs[3], built as scripts/fitted_ab.py builds
it: 32 utterances, capacity 1 024 frames each), hipGraph replay, host buffers in and out, wall-clock per call:

  (a) vocode     V1  zv_vocode_batch of the batch's 32 mels, one call
                 V2  the same work as 32 zv_vocode calls in a loop — what a caller had to write before the batch form
                 V3  zv_vocode_batch_begin / _end with two batches in flight on lanes 0 and 1, as bench.py keeps its chain (per batch)
  (b) planning   P1  zv_encode_batch without hidden (return_hidden=False): the 32 frame counts, one call
                 P2  32 zv_encode_taps calls (Model.encode), hidden and taps downloaded as that call does
  (c) chain      C1  encode_batch -> decode_batch -> vocode_batch, hidden and mel over the host
                 C2  zv_synthesize_batch of the same utterances

The arms of a group alternate round by round in one process; a round is `steps` calls of the arm (V2, P2: `steps` loops of 32 calls)
and reports the time per batch.  Medians over the rounds, each arm's spread (max - min) beside it.  The mels of (a) are the decoder's
own, taken once from the stage chain; the bits of V1, V2 and V3 are compared before anything is timed.

usage (GPU box):  python scripts/stage_batch_ab.py [--steps 8] [--rounds 7] [--out profiles/stage_batch_ab.txt]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from fitted_ab import summary, workload  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.rounds < 7:
        ap.error("--rounds must be at least 7")
    capi, synth, g, ckpt, utts = workload()
    model = capi.Model(ckpt, device=0)
    model.set_graph_mode(True)
    styles = [u[2] for u in utts]
    enc = model.encode_batch(utts)
    nfs = [e["n_frames"] for e in enc]
    mels = model.decode_batch([e["hidden"] for e in enc], styles)
    del enc
    # the three vocode arms give the same bits, and the stage chain gives the chain's
    wav_batch = model.vocode_batch(mels)
    for u, mel in enumerate(mels):
        assert np.array_equal(model.vocode(mel).view(np.uint32), wav_batch[u].view(np.uint32)), u
    model.vocode_batch_begin(0, mels)
    model.vocode_batch_begin(1, mels)
    for lane in (0, 1):
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(model.vocode_batch_end(lane), wav_batch)), lane
    chain = model.synthesize_batch(utts)
    assert [nf for _, nf in chain] == nfs
    chain_same = sum(np.array_equal(w.view(np.uint32), b.view(np.uint32)) for (w, _), b in zip(chain, wav_batch))
    del chain, wav_batch

    def v3(k_steps):                                      # bench.py's loop at depth 2
        for k in range(k_steps):
            model.vocode_batch_begin(k % 2, mels)
            if k >= 1:
                model.vocode_batch_end((k - 1) % 2)
        model.vocode_batch_end((k_steps - 1) % 2)

    def stage_chain():
        e = model.encode_batch(utts)
        model.vocode_batch(model.decode_batch([x["hidden"] for x in e], styles))

    def each(fn):
        return lambda k_steps: [fn() for _ in range(k_steps)]

    groups = [
        ("(a) vocode", [("V1 vocode_batch", each(lambda: model.vocode_batch(mels))),
                        ("V2 32 x vocode", each(lambda: [model.vocode(m) for m in mels])),
                        ("V3 vocode_batch_begin/_end, 2 lanes", v3)]),
        ("(b) planning", [("P1 encode_batch(return_hidden=False)", each(lambda: model.encode_batch(utts, return_hidden=False))),
                          ("P2 32 x encode", each(lambda: [model.encode(*u) for u in utts]))]),
        ("(c) chain", [("C1 encode_batch + decode_batch + vocode_batch", each(stage_chain)),
                       ("C2 synthesize_batch", each(lambda: model.synthesize_batch(utts)))]),
    ]
    lines = ["# scripts/stage_batch_ab.py: bench.py's batch (%d utterances x %d frames of capacity, %d frames of speech), hipGraph replay, "
             "host buffers in and out; %d rounds of %d batches per arm, the arms of a group alternating, one MI355X, one process" %
             (len(utts), utts[0][3], sum(nfs), args.rounds, args.steps),
             "# before the timing: vocode_batch, 32 x vocode and both lanes of vocode_batch_begin / _end gave the same bits; the stage chain gave "
             "the bits of synthesize_batch for %d of %d utterances" % (chain_same, len(utts))]
    medians = {}
    for title, arms in groups:
        ms = {name: [] for name, _ in arms}
        for name, run in arms:
            run(max(args.warmup, 2))
        for _ in range(args.rounds):
            for name, run in arms:
                model.synchronize()
                t0 = time.perf_counter()
                run(args.steps)
                model.synchronize()
                ms[name].append((time.perf_counter() - t0) * 1e3 / args.steps)
        lines.append("# %s: ms per batch" % title)
        for name, _ in arms:
            medians[name[:2]] = statistics.median(ms[name])
            lines.append("%-46s %s   rounds: %s" % (name, summary(ms[name]), " ".join("%.3f" % x for x in ms[name])))
    lines.append("# V2 / V1 = %.2f, V2 / V3 = %.2f, P2 / P1 = %.2f, C1 / C2 = %.2f (medians)" %
                 (medians["V2"] / medians["V1"], medians["V2"] / medians["V3"], medians["P2"] / medians["P1"], medians["C1"] / medians["C2"]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    model.close()


if __name__ == "__main__":
    main()
