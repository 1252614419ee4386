"""What fitted synthesis buys on the benchmark's own batch (BASELINE.json configs[3], built exactly as bench.py builds it), two batches
in flight as in the benchmark, hipGraph replay:

  A   zv_synthesize_batch at capacity (T = bench.FRAMES for every utterance): what bench.py times;
  A0  the same from another build of the library (--parent-lib: the parent commit's), to show A is unchanged;
  B   zv_synthesize_batch_fitted at the same capacities;
  C   zv_synthesize_batch with T[u] = n_frames[u] taken from a previous run: the floor — the right sizes with no table rewrite and
      no empty workgroups;
  S   one 128-phoneme utterance (configs[2], T = 512), zv_synthesize against zv_synthesize_fitted, alternating in one process.

usage (GPU box):  python scripts/fitted_ab.py [--rounds 8] [--parent-lib other.so] [--out profiles/fitted_ab.txt]
Every measurement is a child process of its own under its own time limit (`timeout`), the variants alternate round by round, and
the driver stops at the first child that fails.  One variant alone: --variant A|B|C|S (prints one JSON line)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def workload():
    """bench.py's batch: the same constants, the same constructors"""
    import bench
    from __graft_entry__ import load_package
    load_package()
    from zerovox_cpp_amd import capi, sharding, synth
    g = synth.MEDIUM
    ckpt = os.path.join(os.environ.get("TMPDIR", tempfile.gettempdir()), f"zerovox_medium_seed{bench.SEED_W}.gguf")
    if not os.path.exists(ckpt):
        synth.write_checkpoint(ckpt + ".tmp", g, bench.SEED_W)
        os.replace(ckpt + ".tmp", ckpt)
    lens = sharding.mixed_length_batch(bench.SEED_BATCH, bench.UTTS_PER_GPU)
    utts = [(*synth.encoder_inputs(g, 200 + u, lens[u]), bench.FRAMES) for u in range(bench.UTTS_PER_GPU)]
    return capi, synth, g, ckpt, utts


def run_batch_variant(variant, steps, warmup):
    capi, synth, g, ckpt, utts = workload()
    model = capi.Model(ckpt, device=0)
    hop, sr = model.hp.audio_hop_size, model.hp.audio_sampling_rate
    nfs = [nf for _, nf in model.synthesize_batch(utts)]            # the frames that hold speech
    if variant == "C":
        utts = [u[:3] + (max(nf, 1),) for u, nf in zip(utts, nfs)]
    model.set_graph_mode(True)
    lanes = [model.prepare_batch(utts, fitted=variant == "B") for _ in range(2)]

    def run_steps(k_steps):                      # bench.py's loop at depth 2
        for k in range(k_steps):
            lanes[k % 2].begin(k % 2)
            if k >= 1:
                lanes[(k - 1) % 2].end((k - 1) % 2)
        lanes[(k_steps - 1) % 2].end((k_steps - 1) % 2)

    run_steps(max(warmup, 2))
    model.synchronize()
    t0 = time.perf_counter()
    run_steps(steps)
    model.synchronize()
    dt = (time.perf_counter() - t0) / steps
    got = [nf for _, nf in lanes[0].results()]
    assert got == nfs, "the variant changed the frame counts"
    live = sum(nfs)
    out = {"variant": variant, "ms_per_batch": 1e3 * dt, "utterances": len(utts), "live_frames": live,
           "capacity_frames": sum(u[3] for u in utts),
           "live_audio_xrt": live * hop / sr / dt, "lib": os.environ.get("ZEROVOX_AMD_LIB", "tree")}
    model.close()
    return out


def run_single_variant(rounds):
    capi, synth, g, ckpt, _ = workload()
    model = capi.Model(ckpt, device=0)
    model.set_graph_mode(True)
    ids, puncts, style = synth.encoder_inputs(g, 5, 128)
    T = 512
    ms = {False: [], True: []}
    nf = None
    for fitted in (False, True):
        for _ in range(3):
            nf = model.synthesize(ids, puncts, style, T, fitted=fitted)[1]
    for _ in range(rounds):
        for fitted in (False, True):
            t0 = time.perf_counter()
            for _ in range(20):
                model.synthesize(ids, puncts, style, T, fitted=fitted)
            ms[fitted].append(1e3 * (time.perf_counter() - t0) / 20)
    model.close()
    return {"variant": "S", "T": T, "n_frames": nf, "unfitted_ms": ms[False], "fitted_ms": ms[True]}


def summary(xs):
    return "median %.3f  mean %.3f  min %.3f  max %.3f  spread %.3f" % (statistics.median(xs), statistics.fmean(xs), min(xs), max(xs),
                                                                         max(xs) - min(xs))


def drive(args):
    arms = [("A", None), ("B", None), ("C", None)]
    if args.parent_lib:
        arms.insert(1, ("A0", os.path.abspath(args.parent_lib)))
    res = {name: [] for name, _ in arms}
    lines = []

    def child(variant, lib, limit):
        env = dict(os.environ)
        env.pop("ZEROVOX_AMD_LIB", None)
        if lib:
            env["ZEROVOX_AMD_LIB"] = lib
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--variant", variant[0],
               "--steps", str(args.steps), "--warmup", str(args.warmup), "--rounds", str(args.rounds)]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit("fitted_ab: variant %s ended with status %d: nothing more is started" % (variant, r.returncode))
        return json.loads(r.stdout.strip().splitlines()[-1])

    for rnd in range(args.rounds):
        for name, lib in arms:
            d = child(name, lib, 120)
            res[name].append(d)
            line = "round %d  %-2s  %8.3f ms/batch  live-audio %8.1f x real time  (live %d of %d frames)" % (
                rnd, name, d["ms_per_batch"], d["live_audio_xrt"], d["live_frames"], d["capacity_frames"])
            print(line, flush=True)
            lines.append(line)
    s = child("S", None, 180)
    out = ["fitted synthesis on the benchmark batch (BASELINE.json configs[3]: %d utterances, capacity %d frames each), hipGraph replay,"
           % (res["A"][0]["utterances"], res["A"][0]["capacity_frames"] // res["A"][0]["utterances"]),
           "two batches in flight, %d alternating runs per variant of %d steps after %d warm-up steps, one process per run" %
           (args.rounds, args.steps, args.warmup), ""] + lines + [""]
    for name, _ in arms:
        ms = [d["ms_per_batch"] for d in res[name]]
        xr = [d["live_audio_xrt"] for d in res[name]]
        out.append("%-2s  ms/batch: %s" % (name, summary(ms)))
        out.append("    live-audio x real time: median %.1f  (frames that hold speech: %d of %d)" %
                   (statistics.median(xr), res[name][0]["live_frames"], res[name][0]["capacity_frames"]))
    a, b, c = ([d["ms_per_batch"] for d in res[k]] for k in ("A", "B", "C"))
    sp = lambda x: max(x) - min(x)
    out += ["", "A - B = %.3f ms (medians); sum of the two spreads = %.3f ms" % (statistics.median(a) - statistics.median(b), sp(a) + sp(b)),
            "B / A = %.3f;  B / C = %.3f (B above the floor by %.1f %%)" %
            (statistics.median(b) / statistics.median(a), statistics.median(b) / statistics.median(c),
             100.0 * (statistics.median(b) / statistics.median(c) - 1.0)), "",
            "one 128-phoneme utterance (BASELINE.json configs[2]), capacity T = %d, n_frames = %d, %d alternating rounds of 20 calls:" %
            (s["T"], s["n_frames"], args.rounds),
            "    zv_synthesize         ms/call: %s" % summary(s["unfitted_ms"]),
            "    zv_synthesize_fitted  ms/call: %s" % summary(s["fitted_ms"])]
    text = "\n".join(out) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=["A", "B", "C", "S"], default=None)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.variant is None:
        drive(args)
    elif args.variant == "S":
        print(json.dumps(run_single_variant(args.rounds)))
    else:
        print(json.dumps(run_batch_variant(args.variant, args.steps, args.warmup)))


if __name__ == "__main__":
    main()
