"""What mel analysis costs at the benchmark batch's size (BASELINE.json configs[3], built as scripts/fitted_ab.py builds it: 32
utterances, 1 024 frames each): the batch is synthesised once, then its 32 waveforms go through zv_mel_wave_batch — ONE launch of
`mel_frames` and one of `mel_rows` — in a few eager, profiled runs, and the event-timed entries of zv_profile_end are set next to
`voc_bands_frames`, the band levels' frames pass over the same waveforms (a profiled eager batch that carries band levels), in the
same process.  By MFMA count and table bytes mel_frames is twice that kernel: four digit-plane products where it has two, two
table planes where it has one.  Both are reported as 8-bit multiply-adds per second against the i8 matrix rate, a CONSTANT from the
chip's data sheet (twice the dense bf16 rate of 2.5e15 FLOP/s), and as the rate of the table stream (every workgroup reads its
kernel's whole fragment table once, from L2 or beyond).  The host's share of a call (uploading 39 MB of samples from pageable memory,
downloading the rows) is reported as the wall time of a call.

usage (GPU box):  python scripts/mel_ab.py [--profiled 9] [--out FILE]
profiles/mel_ab.txt holds this output behind the bench.py rounds against the parent commit's library (scripts/ab_lib.sh)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from fitted_ab import workload  # noqa: E402

I8_MACS_PER_S = 2.5e15                     # dense i8 MFMA: twice the bf16 rate of 2.5e15 FLOP/s
TILE_FRAMES, BANDS_TABLE = 32, 2 * 34 * 16 * 64 * 16      # bands.h / mel.h: the tiles of both kernels, BANDS_TABLE_BYTES; mel.h's table is twice that
PLANES = {"voc_bands_frames": 2, "mel_frames": 4}         # digit-plane products per (frame, column)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profiled", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    capi, synth, g, ckpt, utts = workload()
    model = capi.Model(ckpt, device=0)
    model.set_graph_mode(False)
    call = model.prepare_batch(utts, return_bands="frames")
    call.run()
    wavs = [np.array(w, np.float32) for w, _ in call.results()]
    frames = sum(u[3] for u in utts)
    assert all(w.size == u[3] * model.hp.audio_hop_size for w, u in zip(wavs, utts))
    params = capi.MelAnalysis(log="ln", pad="reflect")
    rows = model.mel_wave_batch(wavs, params)             # (the table's upload and the I/O block's growth happen here)
    assert all(r.shape == (u[3], model.hp.audio_num_mels) and np.isfinite(r).all() for r, u in zip(rows, utts))
    one = model.mel_wave(wavs[5], params)
    assert np.array_equal(one.view(np.uint32), rows[5].view(np.uint32))
    model.profile_begin()
    wall = []
    for _ in range(args.profiled):
        call.run()
        t0 = time.perf_counter()
        model.mel_wave_batch(wavs, params)
        wall.append((time.perf_counter() - t0) * 1e3)
    stats = {s["name"]: s for s in model.profile_end()}
    lines = ["# scripts/mel_ab.py: bench.py's batch (%d utterances x %d frames = %d frames, %.1f MB of samples), eager, event-timed; %d profiled "
             "runs of zv_mel_wave_batch (ONE launch per kernel) next to a batch with band levels, one MI355X box, one process" %
             (len(utts), utts[0][3], frames, sum(w.nbytes for w in wavs) / 1e6, args.profiled)]
    per = {}
    for name in ("voc_bands_frames", "mel_frames", "mel_rows"):
        s = stats[name]
        assert s["launches"] == args.profiled, (name, s)
        us, by = s["total_ms"] * 1e3 / s["launches"], s["algo_bytes"] / s["launches"]
        per[name] = us
        lines.append("%-18s %8.2f us per launch  %8.2f MB  %7.1f GB/s   (%d launches, event-timed, eager)" % (name, us, by / 1e6, by / us / 1e3, s["launches"]))
    for name, planes in PLANES.items():
        macs, t = float(frames) * 1024 * 1026 * planes, per[name] * 1e-6
        stream = float(frames) / TILE_FRAMES * BANDS_TABLE * planes / 2
        lines.append("# %s: %.3e 8-bit multiply-adds in %.2f us = %.2fe12 per second = %.1f %% of the i8 matrix rate's %.0fe12 (a constant, not measured "
                     "here); its table stream, %.2f GB per launch (%d workgroups x %.2f MB), runs at %.2f TB/s" %
                     (name, macs, per[name], macs / t / 1e12, 100.0 * macs / t / I8_MACS_PER_S, I8_MACS_PER_S / 1e12, stream / 1e9,
                      frames // TILE_FRAMES, BANDS_TABLE * planes / 2 / 1e6, stream / t / 1e12))
    lines.append("# mel_frames / voc_bands_frames = %.2f (2 by MFMA count and table bytes)" % (per["mel_frames"] / per["voc_bands_frames"]))
    lines.append("# a zv_mel_wave_batch call, wall time on the host (uploads from pageable memory, both launches, the rows' download): "
                 "median %.2f ms, min %.2f, max %.2f" % (float(np.median(wall)), min(wall), max(wall)))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    model.close()


if __name__ == "__main__":
    main()
