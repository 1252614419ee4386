"""A serving stream whose batch shapes change (DESIGN.md "Serving under changing shapes"): 300 pipelined batches on two lanes
(zv_synthesize_batch_begin / _end, batch k enqueued before batch k - 1 is waited for), medium checkpoint, seeded draws: 1-32 utterances
per batch, 32-256 phonemes and a capacity of 256-1 024 frames per utterance.  Two streams from the same draws:

  raw       the draws as they are;
  bucketed  what a careful caller would do: utterances padded to a multiple of 4 (copies of the batch's first), every capacity
            rounded up to a multiple of 128.

Arms, each a process of its own so that two builds never share one (the driver below starts them one after the other, round by
round, every one under its own time limit, and stops at the first that fails):

  parent    another build of the library (ZEROVOX_AMD_LIB=..., the parent commit's: it has no stats call, so only times are printed)
  c16 c64 c256   this tree at that capacity (zv_set_graph_cache)
  off       this tree with graph mode off

Per arm and stream: captures, hit rate, evictions (zv_graph_cache_stats), the median / 99th percentile / worst time of a batch from
its begin() to the return of its end(), the wall time per batch, and the free device memory lost per graph held at the end.  Both
lanes run the largest shape once, eagerly, before anything is timed: no block regrows under the clock in any arm.

  cost      this tree: what a capture costs next to a replay — 16 distinct shapes, one lane, synchronous, each shape's first call
            (capture + run) and second call (replay) timed
  lookup    this tree, small checkpoint: 1 024 graphs held (zv_vocode_device at T = 1 .. 1 024), then the host time of a replaying
            call whose slot is the first the scan meets against one whose slot is the last, the way scripts/hosttime.py times a call

usage (GPU box):  python scripts/serve_stream.py --arms parent,c16,c64,c256,off --rounds 2 --parent-lib zerovox.cpp_amd/_ab/libzv_parent.so [--out FILE]
                  python scripts/serve_stream.py --arm c16            (one arm, in this process)
profiles/serve_stream.txt holds this output behind the bench.py rounds against the parent commit's library (scripts/ab_lib.sh)."""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES, SEED = 300, 20260
ARM_LIMIT_S = 420


def draws(n_batches=BATCHES, seed=SEED):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_batches):
        nseg = int(rng.integers(1, 33))
        out.append([(int(rng.integers(32, 257)), int(rng.integers(256, 1025))) for _ in range(nseg)])
    return out


def bucketed(batch):
    b = [(n, (t + 127) // 128 * 128) for n, t in batch]
    return b + [b[0]] * (-len(b) % 4)


def free_bytes():
    hip = ctypes.CDLL("libamdhip64.so")
    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(np.ceil(q * len(xs))) - 1)]


def load(geometry):
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    load_package()
    from zerovox_cpp_amd import capi, synth
    g = synth.GEOMETRIES[geometry]
    ckpt = os.path.join(os.environ.get("TMPDIR", "/tmp"), "zerovox_%s_seed1234.gguf" % geometry)
    if not os.path.exists(ckpt):
        synth.write_checkpoint(ckpt, g, 1234)
    return capi, synth, g, capi.Model(ckpt, 0)


def stats_of(model):
    return model.graph_cache_stats().as_dict() if hasattr(model.lib, "zv_graph_cache_stats") else None


def run_arm(arm):
    capi, synth, g, model = load("medium")
    inputs = {}

    def utterance(n, t):
        if n not in inputs:
            inputs[n] = synth.encoder_inputs(g, 700 + n, n)
        return (*inputs[n], t)

    def grow():
        model.set_graph_mode(False)
        for lane in (0, 1):
            c = model.prepare_batch([utterance(256, 1024)] * 32)
            c.begin(lane)
            c.end(lane)
        model.synchronize()

    grow()
    if arm == "cost":
        return run_cost(model, utterance)
    graph = arm != "off"
    if arm.startswith("c"):
        model.set_graph_cache(int(arm[1:]))
    for name, shape in (("raw", lambda b: b), ("bucketed", bucketed)):
        batches = [shape(b) for b in draws()]
        keys = {(len(b), -(-max(n for n, _ in b) // 32), -(-max(t for _, t in b) // 64)) for b in batches}
        calls = [model.prepare_batch([utterance(n, t) for n, t in b]) for b in batches]
        model.set_graph_mode(graph)
        model.synchronize()
        s0, free0 = stats_of(model), free_bytes()
        t_begin, ms = [0.0] * len(calls), []
        wall0 = time.perf_counter()
        for k, c in enumerate(calls):
            t_begin[k] = time.perf_counter()
            c.begin(k % 2)
            if k >= 1:
                calls[k - 1].end((k - 1) % 2)
                ms.append((time.perf_counter() - t_begin[k - 1]) * 1e3)
                calls[k - 1] = None
        calls[-1].end((len(calls) - 1) % 2)
        ms.append((time.perf_counter() - t_begin[-1]) * 1e3)
        wall = (time.perf_counter() - wall0) * 1e3 / len(batches)
        model.synchronize()
        s1, free1 = stats_of(model), free_bytes()
        line = "%-7s %-8s batches %d keys %d  batch ms median %.3f p99 %.3f worst %.3f  wall/batch %.3f" % (
            arm, name, len(batches), len(keys), statistics.median(ms), pct(ms, 0.99), max(ms), wall)
        if s1 is not None:
            d = {k: s1[k] - s0[k] for k in s1}
            held = s1["entries"] - s0["entries"]
            line += "  captures %d hit_rate %.3f evictions %d lane_drops %d full_drops %d entries %d retired %d" % (
                d["captures"], d["hits"] / max(1, d["lookups"]), d["evictions"] + d["stale_evictions"], d["lane_drops"], d["full_drops"],
                s1["entries"], s1["retired"])
            line += "  free_mem_delta_MB %.1f (%.2f MB per graph held more)" % ((free0 - free1) / 1e6, (free0 - free1) / 1e6 / held) if held > 0 else \
                    "  free_mem_delta_MB %.1f" % ((free0 - free1) / 1e6)
        else:
            line += "  free_mem_delta_MB %.1f (no stats call in this build)" % ((free0 - free1) / 1e6)
        print(line, flush=True)
        model.set_graph_mode(False)
    model.close()


def run_cost(model, utterance):
    """first call (capture + run) against second call (replay) of 16 distinct shapes, one lane, nothing else in flight"""
    model.set_graph_cache(64)
    model.set_graph_mode(True)
    first, second, eager = [], [], []
    shapes = [(nseg, n, t) for nseg in (1, 4, 12, 32) for n, t in ((40, 300), (100, 520), (200, 800), (256, 1024))]
    for nseg, n, t in shapes:
        c = model.prepare_batch([utterance(n, t)] * nseg)
        times = []
        for _ in range(3):
            model.synchronize()
            t0 = time.perf_counter()
            c.begin(0)
            c.end(0)
            times.append((time.perf_counter() - t0) * 1e3)
        first.append(times[0])
        second.append(min(times[1:]))
        model.set_graph_mode(False)
        t0 = time.perf_counter()
        c.begin(0)
        c.end(0)
        eager.append((time.perf_counter() - t0) * 1e3)
        model.set_graph_mode(True)
        print("cost    shape (%2d utt, %3d phonemes, %4d frames): capture+run %.3f ms  replay %.3f ms  eager %.3f ms" % (nseg, n, t, first[-1], second[-1], eager[-1]), flush=True)
    extra = [a - b for a, b in zip(first, second)]
    print("cost    capture - replay: median %.3f ms, min %.3f, max %.3f; median replay %.3f ms, median eager %.3f ms; captures %d" % (
        statistics.median(extra), min(extra), max(extra), statistics.median(second), statistics.median(eager), model.graph_cache_stats().captures))
    model.close()


def run_lookup():
    capi, synth, g, model = load("small")
    hop, M = g.hop_size, g.num_mels
    N = 1024
    d_mel, d_wav = model.device_alloc(N * M * 4), model.device_alloc(N * hop * 4)
    model.h2d(d_mel, np.zeros((N, M), np.float32))
    model.vocode_device(d_mel, N, d_wav)                  # the arena at its largest, eagerly
    model.synchronize()
    model.set_graph_cache(N)
    model.set_graph_mode(True)
    free0 = free_bytes()
    t0 = time.perf_counter()
    for T in range(1, N + 1):
        model.vocode_device(d_mel, T, d_wav)
    model.synchronize()
    fill_s = time.perf_counter() - t0
    s = model.graph_cache_stats().as_dict()
    assert s["entries"] == N and s["captures"] == N, s
    print("lookup  %d graphs held: %.2f ms per capturing call, %.3f MB of device memory per graph" % (N, fill_s * 1e3 / N, (free0 - free_bytes()) / 1e6 / N))

    def host_us(T, reps=400):
        xs = []
        for _ in range(reps):
            model.synchronize()
            a = time.perf_counter()
            model.vocode_device(d_mel, T, d_wav)          # returns when the replay is enqueued
            xs.append((time.perf_counter() - a) * 1e6)
        return statistics.median(xs)
    for _ in range(2):
        a, b = host_us(1), host_us(2)                     # T = 1: the first slot the scan meets; T = 2: the second
        c, d = host_us(N), host_us(N - 1)                 # the last two
        print("lookup  host time of a replaying call, median of 400: first slots %.2f / %.2f us, last slots (1 024 hashes compared) %.2f / %.2f us" % (a, b, d, c))
    s2 = model.graph_cache_stats().as_dict()
    assert s2["captures"] == N and s2["entries"] == N
    model.set_graph_mode(False)
    model.device_free(d_mel)
    model.device_free(d_wav)
    model.close()


def drive(args):
    lines = []
    for r in range(args.rounds):
        for arm in args.arms.split(","):
            env = dict(os.environ)
            if arm == "parent":
                env["ZEROVOX_AMD_LIB"] = os.path.abspath(args.parent_lib)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", arm], env=env, capture_output=True, text=True, timeout=ARM_LIMIT_S)
            sys.stdout.write(p.stdout)
            sys.stdout.flush()
            lines.append(p.stdout)
            if p.returncode != 0:                         # a failed arm ends the session: nothing more is started on the card
                sys.stderr.write(p.stderr[-3000:])
                return p.returncode
    if args.out:
        with open(args.out, "w") as f:
            f.write("".join(lines))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", default=None)
    ap.add_argument("--arms", default="parent,c16,c64,c256,off")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--parent-lib", default=os.path.join(ROOT, "zerovox.cpp_amd", "_ab", "libzv_parent.so"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.arm == "lookup":
        return run_lookup()
    if args.arm:
        return run_arm(args.arm)
    return drive(args)


if __name__ == "__main__":
    sys.exit(main())
