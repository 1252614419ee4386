#!/usr/bin/env python3
"""Generate the golden fixtures from the compiled reference (oracle/_ref/zvref).

Run in the build container only (it needs /root/reference to have been compiled by `make -C oracle ref`):
    python tests/golden/make_golden.py          (all fixtures)
    python tests/golden/make_golden.py fresh    (only the fresh-seed fixtures)
    python tests/golden/make_golden.py trained  (only the trained-like weight family's fixture)
    python tests/golden/make_golden.py heads    (only the encoder head-count fixture)
    python tests/golden/make_golden.py value_ranges    (only the value-range stage fixture)
    python tests/golden/make_golden.py resblock_geometries    (only the residual-block tap-count fixture)
    python tests/golden/make_golden.py encdec_geometries    (only the encoder / decoder width, FFN tap and mel-count fixture)
    python tests/golden/make_golden.py voc_widths    (only the vocoder-width fixture)
Fixtures hold inputs' *recipes* (geometry, seeds — inputs are regenerated bit-identically by
zerovox.cpp_amd/synth.py) and the reference's OUTPUTS: in full for the small geometries, as strided
samples + SHA-256 of the full f32 buffer for the full-size configs of BASELINE.json.  ISA of the
reference build: x86-64-v3 (AVX2+FMA+F16C), 4 threads (results do not depend on the thread count).
Also slices the reference's only own known-answer data, utils/norm1dexample.json (InstanceNorm1d pair).
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

load_package()
from zerovox_cpp_amd import gguf, synth  # noqa: E402
from oracle import zvoracle  # noqa: E402

SEED_W = 1234
STRIDE = 61      # prime stride for the sampled goldens


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def case(geom_name, T, N, full, tmp="/tmp"):
    g = synth.GEOMETRIES[geom_name]
    path = os.path.join(tmp, f"golden_{geom_name}.gguf")
    synth.write_checkpoint(path, g, SEED_W)
    _, tensors = gguf.read_gguf(path)
    mel_in = synth.vocoder_mel(g, tensors, 7, T)
    hid_in = synth.decoder_hidden(g, 11, T)
    ids, puncts, style = synth.encoder_inputs(g, 5, N)
    v = zvoracle.run_reference(path, T=T, voc=mel_in)
    d = zvoracle.run_reference(path, T=T, dec=(hid_in, style))
    e = zvoracle.run_reference(path, T=T, N=N, enc=(ids, puncts, style), E=g.E)
    out = dict(geometry=geom_name, seed_w=SEED_W, T=T, N=N, seed_mel=7, seed_hidden=11, seed_enc=5, stride=STRIDE,
               wav_sha256=sha(v["wav"]), mel_sha256=sha(d["mel"]), hidden_sha256=sha(e["hidden"]),
               features_sha256=sha(e["features"]), logdur=e["logdur"], energy=e["energy"],
               pitch_bucket=e["pitch_bucket"], energy_bucket=e["energy_bucket"], n_frames=e["n_frames"],
               wav_rms=float(np.sqrt(np.mean(v["wav"].astype(np.float64) ** 2))),
               mel_rms=float(np.sqrt(np.mean(d["mel"].astype(np.float64) ** 2))))
    if full:
        out.update(wav=v["wav"], mel=d["mel"], hidden=e["hidden"], features=e["features"])
    else:
        out.update(wav_samples=v["wav"][::STRIDE].copy(), mel_samples=d["mel"].reshape(-1)[::STRIDE].copy(),
                   hidden_samples=e["hidden"].reshape(-1)[::STRIDE].copy(),
                   features_samples=e["features"].reshape(-1)[::STRIDE].copy())
    np.savez_compressed(os.path.join(HERE, f"{geom_name}_T{T}_N{N}.npz"), **out)
    print(geom_name, T, N, "frames", e["n_frames"], "wav rms", out["wav_rms"])
    os.remove(path)


def demo_case(tmp="/tmp"):
    """ZeroVOXModel::eval() of the reference (src/zerovox.cpp:198-335): its hard-coded utterance (120 phonemes, the
    528-float style vector) through encoder -> decoder -> vocoder back to back at T = max_seq_len, on the synthetic
    medium checkpoint.  The utterance comes from the product library's zv_demo_utterance (data extracted from the
    reference source by scripts/extract_demo_utterance.py)."""
    from zerovox_cpp_amd import capi
    g = synth.MEDIUM
    path = os.path.join(tmp, "golden_medium.gguf")
    synth.write_checkpoint(path, g, SEED_W)
    ids, puncts, style = capi.demo_utterance()
    T = g.max_seq_len
    r = zvoracle.run_reference_chain(path, ids, puncts, style, T=T)
    # (the pitch prediction's buffer is recycled by ggml's graph allocator before the graph ends: not a valid tap)
    out = dict(geometry="medium", seed_w=SEED_W, T=T, N=len(ids), stride=STRIDE, n_frames=r["n_frames"], logdur=r["logdur"],
               energy=r["energy"], pitch_bucket=r["pitch_bucket"], energy_bucket=r["energy_bucket"],
               hidden_sha256=sha(r["hidden"]), mel_sha256=sha(r["mel"]), wav_sha256=sha(r["wav"]),
               features_sha256=sha(r["features"]),
               wav_samples=r["wav"][::STRIDE].copy(), mel_samples=r["mel"].reshape(-1)[::STRIDE].copy(),
               wav_rms=float(np.sqrt(np.mean(r["wav"].astype(np.float64) ** 2))))
    np.savez_compressed(os.path.join(HERE, "demo_medium_T%d.npz" % T), **out)
    print("demo utterance: frames", r["n_frames"], "wav rms", out["wav_rms"])
    os.remove(path)


def numph_case(tmp="/tmp"):
    """FS2Encoder::eval with num_phonemes < max_n_phonemes (reference src/fs2encoder.cpp:594-650): the graph encodes all
    max_n_phonemes tokens, the length regulator walks the first num_phonemes."""
    g = synth.SMALL
    path = os.path.join(tmp, "golden_small.gguf")
    synth.write_checkpoint(path, g, SEED_W)
    N, num, T = 16, 9, 64
    ids, puncts, style = synth.encoder_inputs(g, 5, N)
    e = zvoracle.run_reference(path, T=T, N=N, enc=(ids, puncts, style), E=g.E, num_phonemes=num)
    full = zvoracle.run_reference(path, T=T, N=N, enc=(ids, puncts, style), E=g.E)
    assert np.array_equal(e["features"], full["features"]) and e["n_frames"] < full["n_frames"]
    np.savez_compressed(os.path.join(HERE, "small_T64_N16_num9.npz"), geometry="small", seed_w=SEED_W, T=T, N=N, num=num,
                        seed_enc=5, hidden=e["hidden"], n_frames=e["n_frames"], logdur=e["logdur"],
                        features_sha256=sha(e["features"]))
    print("num_phonemes case: frames", e["n_frames"], "of", full["n_frames"])
    os.remove(path)


def robust_case(tmp="/tmp", search=0):
    """An UN-FORCED end-to-end golden: ZeroVOXModel::eval's chain (src/zerovox.cpp:326-334) on an utterance whose integer
    decisions do not depend on summation order.  Geometry medium8 (8 variance bins); the utterance seed was found by
    search (search=N re-runs it over N seeds with our oracle, which reproduces the reference bit for bit): every pitch /
    energy prediction >= 0.1 bin from a bucket boundary, every duration >= 0.04 frames from a rounding boundary.  Besides
    the reference's outputs the fixture stores the reference semantics' own un-forced re-association noise (our oracle in
    sequential-f32 order against the reference): the floor the GPU is gated against."""
    g = synth.GEOMETRIES["medium8"]
    path = os.path.join(tmp, "golden_medium8.gguf")
    synth.write_checkpoint(path, g, SEED_W)
    _, tensors = gguf.read_gguf(path)
    N, T, seed = 16, 96, 11167
    nb = g.ve_n_bins

    def margins(e):
        def bm(p):
            x = p.astype(np.float64) * (nb - 1) + 0.5
            fr = x - np.floor(x)
            m = np.minimum(fr, 1 - fr)
            m = np.where(x < 0, -x, m)
            return np.where(x >= nb, x - nb + 1, m)
        d = np.exp(e["logdur"].astype(np.float64)) - 1.0 + 0.5
        fd = d - np.floor(d)
        return float(bm(e["pitch"]).min()), float(bm(e["energy"]).min()), float(np.where(d < 0, -d, np.minimum(fd, 1 - fd)).min())

    orc = zvoracle.Oracle(tensors, threads=8)
    if search:
        best = (0.0, seed)
        for sd in range(1000, 1000 + search):
            ids, puncts, style = synth.encoder_inputs(g, sd, N)
            mp, me, md = margins(orc.encoder(g, ids, puncts, style, T))
            best = max(best, (min(mp, me, 4 * md), sd))
        seed = best[1]
    ids, puncts, style = synth.encoder_inputs(g, seed, N)
    r = zvoracle.run_reference_chain(path, ids, puncts, style, T=T)
    e = orc.encoder(g, ids, puncts, style, T)        # (the reference's pitch tap is recycled by its graph allocator: ours)
    assert np.array_equal(e["hidden"], r["hidden"]) and e["n_frames"] == r["n_frames"]
    mp, me, md = margins(e)
    alt = zvoracle.Oracle(tensors, threads=8, order=zvoracle.ORDER_SEQ_F32)
    ea = alt.encoder(g, ids, puncts, style, T)
    mela = alt.decoder(ea["hidden"], style)
    wava = alt.vocoder(mela)
    assert ea["n_frames"] == r["n_frames"] and np.array_equal(ea["pitch_bucket"], r["pitch_bucket"]) and np.array_equal(ea["energy_bucket"], r["energy_bucket"])
    rms = lambda a: float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))
    out = dict(geometry="medium8", seed_w=SEED_W, T=T, N=N, seed_enc=seed, n_frames=r["n_frames"], logdur=r["logdur"],
               pitch=e["pitch"], energy=r["energy"], pitch_bucket=r["pitch_bucket"], energy_bucket=r["energy_bucket"],
               margin_pitch_bins=mp, margin_energy_bins=me, margin_duration_frames=md,
               hidden_sha256=sha(r["hidden"]), mel=r["mel"], wav=r["wav"], wav_rms=rms(r["wav"]), mel_rms=rms(r["mel"]),
               floor_wav_rms=rms(wava - r["wav"]), floor_wav_max=float(np.max(np.abs(wava - r["wav"]))),
               floor_mel_rms=rms(mela - r["mel"]), floor_mel_max=float(np.max(np.abs(mela - r["mel"]))),
               floor_hidden_max=float(np.max(np.abs(ea["hidden"] - r["hidden"]))))
    np.savez_compressed(os.path.join(HERE, "robust_medium8_T%d_N%d.npz" % (T, N)), **out)
    print("robust un-forced case: seed %d frames %d margins pitch %.3f energy %.3f bins, duration %.3f frames; un-forced floor wav rms %.3e mel max %.3e"
          % (seed, r["n_frames"], mp, me, md, out["floor_wav_rms"], out["floor_mel_max"]))
    os.remove(path)


def add_floors(tmp="/tmp"):
    """the reference semantics' own re-association noise on each full-size fixture's stage inputs (our oracle in sequential-f32
    order against the stored reference samples): the floor the GPU's stage outputs are gated against (1.5 x), stored in
    the fixture itself so that the tests carry no hand-written tolerance"""
    g = synth.MEDIUM
    path = os.path.join(tmp, "golden_medium.gguf")
    synth.write_checkpoint(path, g, SEED_W)
    _, tensors = gguf.read_gguf(path)
    alt = zvoracle.Oracle(tensors, threads=8, order=zvoracle.ORDER_SEQ_F32)
    rms = lambda a: float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))
    for name in ("medium_T512_N64.npz", "medium_T512_N128.npz", "medium_T1024_N256.npz"):
        f = os.path.join(HERE, name)
        z = dict(np.load(f))
        T, s_ = int(z["T"]), int(z["stride"])
        mel_in = synth.vocoder_mel(g, tensors, int(z["seed_mel"]), T)
        hid_in = synth.decoder_hidden(g, int(z["seed_hidden"]), T)
        _, _, style = synth.encoder_inputs(g, int(z["seed_enc"]), int(z["N"]))
        dm = alt.decoder(hid_in, style).reshape(-1)[::s_] - z["mel_samples"]
        dw = alt.vocoder(mel_in)[::s_] - z["wav_samples"]
        z.update(floor_mel_max=float(np.max(np.abs(dm))), floor_mel_rms=rms(dm), floor_wav_rms=rms(dw), floor_wav_max=float(np.max(np.abs(dw))))
        np.savez_compressed(f, **z)
        print(name, "floors: mel max %.3e rms %.3e, wav rms %.3e" % (z["floor_mel_max"], z["floor_mel_rms"], z["floor_wav_rms"]))
    # the reference's demo utterance (chain mode: the decoder's input is the reference's own hidden, not regenerable from a
    # seed): teacher-force our oracle with the reference's hidden / mel via the reference chain's outputs
    from zerovox_cpp_amd import capi
    f = os.path.join(HERE, "demo_medium_T1500.npz")
    z = dict(np.load(f))
    ids, puncts, style = capi.demo_utterance()
    T, s_ = int(z["T"]), int(z["stride"])
    r = zvoracle.run_reference_chain(path, ids, puncts, style, T=T)
    dm = alt.decoder(r["hidden"], style).reshape(-1)[::s_] - z["mel_samples"]
    dw = alt.vocoder(r["mel"])[::s_] - z["wav_samples"]
    z.update(floor_mel_max=float(np.max(np.abs(dm))), floor_mel_rms=rms(dm), floor_wav_rms=rms(dw), floor_wav_max=float(np.max(np.abs(dw))))
    np.savez_compressed(f, **z)
    print("demo floors (stages teacher-forced with the reference's own hidden / mel): mel max %.3e rms %.3e, wav rms %.3e"
          % (z["floor_mel_max"], z["floor_mel_rms"], z["floor_wav_rms"]))
    os.remove(path)


def _encoder_margins(ref, a, ex):
    """the reference semantics' own re-association noise on an encoder run: ref = the reference's outputs, a = our oracle in
    sequential-f32 order, ex = our oracle in the reference's order (bit-exact; it supplies the float pitch prediction)"""
    # the float pitch prediction comes from the bit-exact oracle: the reference's own pitch tensor is recycled by ggml's
    # graph allocator before the harness can read it (its buckets, energy, log-durations and hidden are read and agree)
    assert np.array_equal(ex["pitch_bucket"], ref["pitch_bucket"]) and np.array_equal(ex["energy"], ref["energy"])
    assert np.array_equal(ex["logdur"], ref["logdur"]) and np.array_equal(ex["energy_bucket"], ref["energy_bucket"])
    ref = dict(ref, pitch=ex["pitch"])
    dur_r = np.exp(ref["logdur"].astype(np.float64)) - 1 + 0.5
    dur_a = np.exp(a["logdur"].astype(np.float64)) - 1 + 0.5
    pflip = a["pitch_bucket"] != ref["pitch_bucket"]
    near = np.convolve(pflip.astype(np.int32), np.ones(5, np.int32), mode="same") > 0      # the energy predictor sees two k = 3 convs of x + pitch embedding
    clean = ~near
    return dict(pitch=ref["pitch"], energy=ref["energy"],
                floor_logdur_max=float(np.max(np.abs(a["logdur"] - ref["logdur"]))),
                floor_pitch_max=float(np.max(np.abs(a["pitch"] - ref["pitch"]))),
                floor_energy_max=float(np.max(np.abs(a["energy"][clean] - ref["energy"][clean]))) if clean.any() else 0.0,
                floor_dur_flips=int(np.sum(dur_r.astype(np.int64) != dur_a.astype(np.int64))),
                floor_pitch_flips=int(pflip.sum()),
                floor_energy_flips=int(np.sum(a["energy_bucket"] != ref["energy_bucket"])),
                floor_frames=int(abs(int(a["n_frames"]) - int(ref["n_frames"]))))


def add_encoder_margins(tmp="/tmp"):
    """what the reference semantics' own re-association noise does to the ENCODER of each full-size fixture (our oracle in
    sequential-f32 order against the reference on the same ids): the floors of the float predictions and of the integer
    decisions.  The fixtures also get the reference's float pitch predictions, so that a test can measure how far every flipped
    bucket / duration of the GPU sat from a rounding boundary IN THE REFERENCE — the gates of tests/test_gpu_full_size.py and
    tests/test_gpu_round2.py carry no hand-written tolerance any more."""
    from zerovox_cpp_amd import capi
    g = synth.MEDIUM
    path = os.path.join(tmp, "golden_medium.gguf")
    synth.write_checkpoint(path, g, SEED_W)
    _, tensors = gguf.read_gguf(path)
    alt = zvoracle.Oracle(tensors, threads=8, order=zvoracle.ORDER_SEQ_F32)
    exact = zvoracle.Oracle(tensors, threads=8)          # the reference's summation order: reproduces it bit for bit

    margins = _encoder_margins
    for name in ("medium_T512_N64.npz", "medium_T512_N128.npz", "medium_T1024_N256.npz"):
        f = os.path.join(HERE, name)
        z = dict(np.load(f))
        T, N = int(z["T"]), int(z["N"])
        ids, puncts, style = synth.encoder_inputs(g, int(z["seed_enc"]), N)
        ref = zvoracle.run_reference(path, T=T, N=N, enc=(ids, puncts, style), E=g.E)
        assert np.array_equal(ref["logdur"], z["logdur"]) and np.array_equal(ref["pitch_bucket"], z["pitch_bucket"])
        z.update(margins(ref, alt.encoder(g, ids, puncts, style, T), exact.encoder(g, ids, puncts, style, T)))
        np.savez_compressed(f, **z)
        print(name, {k: z[k] for k in z if k.startswith("floor_") and "mel" not in k and "wav" not in k})
    f = os.path.join(HERE, "demo_medium_T1500.npz")
    z = dict(np.load(f))
    ids, puncts, style = capi.demo_utterance()
    T = int(z["T"])
    ref = zvoracle.run_reference(path, T=T, N=len(ids), enc=(ids, puncts, style), E=g.E)
    assert np.array_equal(ref["logdur"], z["logdur"]) and np.array_equal(ref["pitch_bucket"], z["pitch_bucket"])
    z.update(margins(ref, alt.encoder(g, ids, puncts, style, T), exact.encoder(g, ids, puncts, style, T)))
    np.savez_compressed(f, **z)
    print("demo", {k: z[k] for k in z if k.startswith("floor_") and "mel" not in k and "wav" not in k})
    os.remove(path)


HEAD_GEOMETRIES = ("medium_h1", "medium_h3", "medium_h4", "medium_h8")
HEAD_CASES = ((37, 160), (300, 1200), (450, 1500))       # (N, T): attention over 37 / 300 / 450 keys


def heads_cases(tmp="/tmp"):
    """The reference's encoder at `encoder.head` = 1, 3, 4, 8 (dk = 528, 176, 132, 66; every other fixture has 2): log-durations,
    energies, buckets and frame counts in full, features / hidden as SHA-256, and the re-association floors of
    _encoder_margins (so that a GPU test can gate its encoder on them).  One file for the four geometries."""
    out = dict(geometries=np.array(HEAD_GEOMETRIES), cases=np.array(HEAD_CASES), seed_w=SEED_W, seed_enc=5)
    for gname in HEAD_GEOMETRIES:
        g = synth.GEOMETRIES[gname]
        path = os.path.join(tmp, f"golden_{gname}.gguf")
        synth.write_checkpoint(path, g, SEED_W)
        _, tensors = gguf.read_gguf(path)
        alt = zvoracle.Oracle(tensors, threads=8, order=zvoracle.ORDER_SEQ_F32)
        exact = zvoracle.Oracle(tensors, threads=8)
        for N, T in HEAD_CASES:
            ids, puncts, style = synth.encoder_inputs(g, 5, N)
            r = zvoracle.run_reference(path, T=T, N=N, enc=(ids, puncts, style), E=g.E)
            k = "%s_N%d_" % (gname, N)
            for name in ("logdur", "energy", "pitch_bucket", "energy_bucket", "n_frames"):
                out[k + name] = r[name]
            out[k + "features_sha256"], out[k + "hidden_sha256"] = sha(r["features"]), sha(r["hidden"])
            m = _encoder_margins(r, alt.encoder(g, ids, puncts, style, T), exact.encoder(g, ids, puncts, style, T))
            out.update({k + name: v for name, v in m.items()})
            print(gname, N, T, "frames", r["n_frames"], {n: m[n] for n in m if n.startswith("floor_")})
        os.remove(path)
    np.savez_compressed(os.path.join(HERE, "medium_heads.npz"), **out)


def norm_kat():
    src = "/root/reference/utils/norm1dexample.json"
    if not os.path.exists(src):
        return
    j = json.load(open(src))
    x_in, x_out = np.array(j["x_in"], np.float32)[0], np.array(j["x_out"], np.float32)[0]
    w, b = np.array(j["weight"], np.float32), np.array(j["bias"], np.float32)
    sel = np.arange(0, x_in.shape[0], 16)
    np.savez_compressed(os.path.join(HERE, "instnorm1d_kat.npz"), x_in=x_in[sel], x_out=x_out[sel], weight=w[sel], bias=b[sel],
                        channels=sel)
    print("instnorm KAT:", x_in[sel].shape)


def fresh_cases(tmp="/tmp"):
    """The reference's outputs on weights seeds no other fixture uses (the cases of
    tests/test_oracle_golden.py::test_oracle_vs_live_reference_fresh_seed and
    tests/test_gpu_vocoder.py::test_gpu_vs_live_reference_fresh_seed), stored in full so that those tests run where
    oracle/_ref/zvref is not built; where it is, the tests also check that it still reproduces these files."""
    g = synth.TINY
    path = os.path.join(tmp, "golden_fresh_tiny.gguf")
    synth.write_checkpoint(path, g, 99, trim_dims=True)      # ggml-C-writer style n_dims
    _, tensors = gguf.read_gguf(path)
    out = dict(geometry="tiny", seed_w=99, trim_dims=True, seed_mel=21, seed_hidden=22, seed_enc=23, cases=np.array([[7, 3], [33, 17]]))
    for T, N in out["cases"]:
        T, N = int(T), int(N)
        mel = synth.vocoder_mel(g, tensors, 21, T)
        hid = synth.decoder_hidden(g, 22, T)
        ids, puncts, style = synth.encoder_inputs(g, 23, N)
        k = "T%d_N%d_" % (T, N)
        out[k + "wav"] = zvoracle.run_reference(path, T=T, voc=mel)["wav"]
        out[k + "mel"] = zvoracle.run_reference(path, T=T, dec=(hid, style))["mel"]
        r = zvoracle.run_reference(path, T=T, N=N, enc=(ids, puncts, style), E=g.E)
        for name in ("hidden", "features", "logdur", "energy", "pitch_bucket", "energy_bucket", "n_frames"):
            out[k + name] = r[name]
    np.savez_compressed(os.path.join(HERE, "fresh_tiny_seed99.npz"), **out)
    os.remove(path)
    g = synth.SMALL
    path = os.path.join(tmp, "golden_fresh_small.gguf")
    synth.write_checkpoint(path, g, 4321)
    _, tensors = gguf.read_gguf(path)
    T, N = 72, 18
    mel = synth.vocoder_mel(g, tensors, 23, T)
    ids, puncts, style = synth.encoder_inputs(g, 24, N)
    hid = synth.decoder_hidden(g, 25, T)
    v = zvoracle.run_reference(path, T=T, voc=mel)
    d = zvoracle.run_reference(path, T=T, dec=(hid, style))
    e = zvoracle.run_reference(path, T=T, N=N, enc=(ids, puncts, style), E=g.E)
    np.savez_compressed(os.path.join(HERE, "fresh_small_seed4321_T%d_N%d.npz" % (T, N)), geometry="small", seed_w=4321, T=T, N=N,
                        seed_mel=23, seed_enc=24, seed_hidden=25, wav=v["wav"], mel=d["mel"], logdur=e["logdur"],
                        n_frames=e["n_frames"])
    print("fresh-seed cases: tiny seed 99 (T, N) =", [tuple(c) for c in out["cases"]], "| small seed 4321 frames", e["n_frames"])
    os.remove(path)


TRAINED_SEED = 2719         # a weights seed no other fixture uses


def trained_cases(tmp="/tmp"):
    """The reference's outputs on the "trained" weight family of synth.make_tensors (heavy-tailed f16 conv weights with exact
    zeros, f16 subnormals and pruned channels; norm gains that include 0 and negatives): small geometry, ragged (N, T) = (18, 72),
    all three stages, stored in full (the case of tests/test_oracle_golden.py::test_oracle_vs_reference_trained_family)."""
    g = synth.SMALL
    path = os.path.join(tmp, "golden_trained_small.gguf")
    synth.write_checkpoint(path, g, TRAINED_SEED, family="trained")
    _, tensors = gguf.read_gguf(path)
    T, N = 72, 18
    mel = synth.vocoder_mel(g, tensors, 26, T)
    ids, puncts, style = synth.encoder_inputs(g, 27, N)
    hid = synth.decoder_hidden(g, 28, T)
    out = dict(geometry="small", family="trained", seed_w=TRAINED_SEED, T=T, N=N, seed_mel=26, seed_enc=27, seed_hidden=28)
    out["wav"] = zvoracle.run_reference(path, T=T, voc=mel)["wav"]
    out["mel"] = zvoracle.run_reference(path, T=T, dec=(hid, style))["mel"]
    r = zvoracle.run_reference(path, T=T, N=N, enc=(ids, puncts, style), E=g.E)
    for name in ("hidden", "features", "logdur", "energy", "pitch_bucket", "energy_bucket", "n_frames"):
        out[name] = r[name]
    assert all(np.isfinite(out[k]).all() for k in ("wav", "mel", "hidden", "features", "logdur", "energy"))
    np.savez_compressed(os.path.join(HERE, "trained_small_seed%d_T%d_N%d.npz" % (TRAINED_SEED, T, N)), **out)
    print("trained-family case: small seed %d frames %d wav rms %.4f peak %.3f" % (
        TRAINED_SEED, r["n_frames"], float(np.sqrt(np.mean(out["wav"].astype(np.float64) ** 2))), float(np.max(np.abs(out["wav"])))))
    os.remove(path)


def value_ranges_case(tmp="/tmp"):
    """The reference's decoder and vocoder on the crafted stage inputs of tests/parity_helpers.value_range_stage_inputs (small
    geometry): a decoder hidden with per-channel offsets up to 1e3 sigma, constant channels and an all-zero band; a vocoder mel
    in magnitude bands, the first exactly at hifigan.mean.  SHA-256 + strided samples of the outputs, and per gated region the
    reference semantics' own re-association floor (our oracle in sequential-f32 order against the reference, as add_floors)."""
    sys.path.insert(0, os.path.dirname(HERE))
    import parity_helpers as ph
    g = synth.SMALL
    path = os.path.join(tmp, "golden_value_ranges_small.gguf")
    synth.write_checkpoint(path, g, SEED_W)
    _, tensors = gguf.read_gguf(path)
    hid, style, mel_in, dreg, vreg = ph.value_range_stage_inputs(g, tensors)
    mel = zvoracle.run_reference(path, T=hid.shape[0], dec=(hid, style))["mel"]
    wav = zvoracle.run_reference(path, T=mel_in.shape[0], voc=mel_in)["wav"]
    alt = zvoracle.Oracle(tensors, threads=8, order=zvoracle.ORDER_SEQ_F32)
    dm, dw = alt.decoder(hid, style) - mel, alt.vocoder(mel_in) - wav
    rms = lambda a: float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))
    out = dict(geometry="small", seed_w=SEED_W, stride=STRIDE, mel_sha256=sha(mel), wav_sha256=sha(wav),
               mel_samples=mel.reshape(-1)[::STRIDE].copy(), wav_samples=wav[::STRIDE].copy())
    for stage, d, ref, regs in (("mel", dm, mel, dreg), ("wav", dw, wav, vreg)):
        out[stage + "_floor_rms"] = np.array([rms(d[idx]) for _, idx in regs])
        out[stage + "_floor_max"] = np.array([float(np.max(np.abs(d[idx]))) for _, idx in regs])
        out[stage + "_rms"] = np.array([rms(ref[idx]) for _, idx in regs])
        for (lbl, _), f, fm, r in zip(regs, out[stage + "_floor_rms"], out[stage + "_floor_max"], out[stage + "_rms"]):
            print(f"value ranges {stage} [{lbl}]: rms {r:.3e}, floor rms {f:.3e} max {fm:.3e}")
    np.savez_compressed(os.path.join(HERE, "value_ranges_small.npz"), **out)
    os.remove(path)


RB_T = 24                   # frames of the residual-block geometry fixture
RB_CHAIN = "medium_rb_c1c2"    # the geometry whose decoder -> vocoder chain is stored as well


def resblock_geometries_case(tmp="/tmp"):
    """The reference's vocoder on every residual-block geometry of synth.RESBLOCK_GEOMETRIES (tap counts other than 3 / 7 / 11, a
    K that changes over one branch's dilations, convs1 and convs2 of one pair with different K), RB_T frames of
    synth.vocoder_mel; and on RB_CHAIN the decoder -> vocoder chain (the reference's own mel fed to its vocoder).  SHA-256 +
    strided samples of every output."""
    out = dict(geometries=np.array(synth.RESBLOCK_GEOMETRIES), seed_w=SEED_W, T=RB_T, seed_mel=7, seed_hidden=11, seed_style=5,
               stride=STRIDE, chain=RB_CHAIN)
    for gname in synth.RESBLOCK_GEOMETRIES:
        g = synth.GEOMETRIES[gname]
        path = os.path.join(tmp, f"golden_{gname}.gguf")
        synth.write_checkpoint(path, g, SEED_W)
        _, tensors = gguf.read_gguf(path)
        wav = zvoracle.run_reference(path, T=RB_T, voc=synth.vocoder_mel(g, tensors, 7, RB_T))["wav"]
        out[gname + "/wav_sha256"] = sha(wav)
        out[gname + "/wav_samples"] = wav[::STRIDE].copy()
        print(f"{gname}: wav rms {float(np.sqrt(np.mean(wav.astype(np.float64) ** 2))):.4f}")
        if gname == RB_CHAIN:
            hid = synth.decoder_hidden(g, 11, RB_T)
            style = synth.encoder_inputs(g, 5, 8)[2]
            mel = zvoracle.run_reference(path, T=RB_T, dec=(hid, style))["mel"]
            cw = zvoracle.run_reference(path, T=RB_T, voc=mel)["wav"]
            out.update(chain_mel_sha256=sha(mel), chain_mel_samples=mel.reshape(-1)[::STRIDE].copy(), chain_wav_sha256=sha(cw),
                       chain_wav_samples=cw[::STRIDE].copy())
        os.remove(path)
    np.savez_compressed(os.path.join(HERE, "resblock_geometries_T%d.npz" % RB_T), **out)


ED_N, ED_T_ENC, ED_T = 16, 160, 24       # phonemes and frames of the encoder, frames of the decoder -> vocoder chain


def encdec_geometries_case(tmp="/tmp"):
    """The reference on every geometry of synth.ENCDEC_GEOMETRIES (other widths E, FFN tap counts, predictor widths V, layer and
    mel counts): the encoder on ED_N phonemes (log-durations, energies, buckets and frame count in full; features / hidden as
    SHA-256 — the reference's float pitch tensor is recycled by ggml's allocator before the harness reads it), the decoder on
    ED_T frames of synth.decoder_hidden and the vocoder on that mel (SHA-256 + strided samples)."""
    out = dict(geometries=np.array(synth.ENCDEC_GEOMETRIES), seed_w=SEED_W, N=ED_N, T_enc=ED_T_ENC, T=ED_T, seed_enc=5,
               seed_hidden=11, seed_style=5, stride=STRIDE)
    for gname in synth.ENCDEC_GEOMETRIES:
        g = synth.GEOMETRIES[gname]
        path = os.path.join(tmp, f"golden_{gname}.gguf")
        synth.write_checkpoint(path, g, SEED_W)
        ids, puncts, style = synth.encoder_inputs(g, 5, ED_N)
        e = zvoracle.run_reference(path, T=ED_T_ENC, N=ED_N, enc=(ids, puncts, style), E=g.E)
        for name in ("logdur", "energy", "pitch_bucket", "energy_bucket", "n_frames"):
            out[f"{gname}/{name}"] = e[name]
        out[gname + "/features_sha256"], out[gname + "/hidden_sha256"] = sha(e["features"]), sha(e["hidden"])
        hid = synth.decoder_hidden(g, 11, ED_T)
        mel = zvoracle.run_reference(path, T=ED_T, dec=(hid, synth.encoder_inputs(g, 5, 8)[2]))["mel"]
        assert mel.shape == (ED_T, g.num_mels)
        wav = zvoracle.run_reference(path, T=ED_T, voc=mel)["wav"]
        out.update({gname + "/mel_sha256": sha(mel), gname + "/mel_samples": mel.reshape(-1)[::STRIDE].copy(),
                    gname + "/wav_sha256": sha(wav), gname + "/wav_samples": wav[::STRIDE].copy()})
        print(f"{gname}: frames {e['n_frames']}, mel rms {float(np.sqrt(np.mean(mel.astype(np.float64) ** 2))):.3f}, "
              f"wav rms {float(np.sqrt(np.mean(wav.astype(np.float64) ** 2))):.4f}")
        os.remove(path)
    np.savez_compressed(os.path.join(HERE, "encdec_geometries_N%d_T%d.npz" % (ED_N, ED_T)), **out)


VW_T = 24                   # frames of the vocoder-width fixture


def voc_widths_case(tmp="/tmp"):
    """The reference's vocoder on every geometry of synth.VOC_WIDTH_GEOMETRIES (256, 496, 768 and 1 024 vocoder channels: stages the
    project's schedule runs on other kernels than at 512, 128 and 48), VW_T frames of synth.vocoder_mel.  SHA-256 + strided samples
    of every output."""
    out = dict(geometries=np.array(synth.VOC_WIDTH_GEOMETRIES), seed_w=SEED_W, T=VW_T, seed_mel=7, stride=STRIDE)
    for gname in synth.VOC_WIDTH_GEOMETRIES:
        g = synth.GEOMETRIES[gname]
        path = os.path.join(tmp, f"golden_{gname}.gguf")
        synth.write_checkpoint(path, g, SEED_W)
        _, tensors = gguf.read_gguf(path)
        wav = zvoracle.run_reference(path, T=VW_T, voc=synth.vocoder_mel(g, tensors, 7, VW_T))["wav"]
        assert wav.shape == (VW_T * g.hop_size,) and np.isfinite(wav).all(), gname
        out[gname + "/wav_sha256"] = sha(wav)
        out[gname + "/wav_samples"] = wav[::STRIDE].copy()
        print(f"{gname}: wav rms {float(np.sqrt(np.mean(wav.astype(np.float64) ** 2))):.4f}")
        os.remove(path)
    np.savez_compressed(os.path.join(HERE, "voc_widths_T%d.npz" % VW_T), **out)


if __name__ == "__main__":
    if not zvoracle.have_reference():
        sys.exit("oracle/_ref/zvref missing: run `make -C oracle ref` first")
    if sys.argv[1:] == ["fresh"]:           # only the fresh-seed fixtures (the others are left as they are)
        fresh_cases()
        sys.exit(0)
    if sys.argv[1:] == ["trained"]:         # only the trained-like weight family's fixture
        trained_cases()
        sys.exit(0)
    if sys.argv[1:] == ["value_ranges"]:    # only the value-range stage fixture
        value_ranges_case()
        sys.exit(0)
    if sys.argv[1:] == ["resblock_geometries"]:     # only the residual-block tap-count fixture
        resblock_geometries_case()
        sys.exit(0)
    if sys.argv[1:] == ["encdec_geometries"]:       # only the encoder / decoder geometry fixture
        encdec_geometries_case()
        sys.exit(0)
    if sys.argv[1:] == ["voc_widths"]:              # only the vocoder-width fixture
        voc_widths_case()
        sys.exit(0)
    if sys.argv[1:] == ["heads"]:           # only the encoder head-count fixture
        heads_cases()
        sys.exit(0)
    case("tiny", 40, 10, full=True)
    case("small", 64, 16, full=True)
    case("medium", 512, 64, full=False)      # BASELINE.json configs[0] (N=64) and [1] (vocoder, 512 frames)
    case("medium", 512, 128, full=False)     # configs[2]
    case("medium", 1024, 256, full=False)    # configs[3]: T = 1 024, its longest utterance (256 phonemes)
    norm_kat()
    demo_case()
    numph_case()
    robust_case()
    add_floors()
    add_encoder_margins()
    fresh_cases()
    trained_cases()
    heads_cases()
    value_ranges_case()
    resblock_geometries_case()
    encdec_geometries_case()
    voc_widths_case()
