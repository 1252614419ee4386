"""CPU: the oracle (oracle/zv_oracle.c) against the golden vectors produced by the compiled reference.

The fixtures under tests/golden/ are OUTPUTS OF THE REFERENCE ITSELF (tests/golden/make_golden.py drives
oracle/_ref/zvref = the unmodified stage classes on ggml-CPU).  The oracle must reproduce them bit for bit
(ZVO_ORDER_GGML_AVX2).  Where oracle/_ref exists the fresh-seed case is also checked live against it."""
import hashlib
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _inputs(g, tensors, z):
    from zerovox_cpp_amd import synth
    T, N = int(z["T"]), int(z["N"])
    mel = synth.vocoder_mel(g, tensors, int(z["seed_mel"]), T)
    hid = synth.decoder_hidden(g, int(z["seed_hidden"]), T)
    ids, puncts, style = synth.encoder_inputs(g, int(z["seed_enc"]), N)
    return T, N, mel, hid, ids, puncts, style


@pytest.mark.parametrize("fixture", ["tiny_T40_N10.npz", "small_T64_N16.npz"])
def test_oracle_reproduces_reference_full(ckpt, fixture):
    from oracle import zvoracle
    z = np.load(os.path.join(GOLD, fixture))
    path, g, tensors = ckpt(str(z["geometry"]), int(z["seed_w"]))
    T, N, mel, hid, ids, puncts, style = _inputs(g, tensors, z)
    orc = zvoracle.Oracle(tensors)
    assert np.array_equal(orc.vocoder(mel), z["wav"])
    assert np.array_equal(orc.decoder(hid, style), z["mel"])
    e = orc.encoder(g, ids, puncts, style, T)
    assert np.array_equal(e["hidden"], z["hidden"])
    assert np.array_equal(e["features"], z["features"])
    assert np.array_equal(e["logdur"], z["logdur"])
    assert np.array_equal(e["energy"], z["energy"])
    assert np.array_equal(e["pitch_bucket"], z["pitch_bucket"])
    assert np.array_equal(e["energy_bucket"], z["energy_bucket"])
    assert e["n_frames"] == int(z["n_frames"])


@pytest.mark.parametrize("fixture", ["medium_T512_N64.npz", "medium_T512_N128.npz", "medium_T1024_N256.npz"])
def test_oracle_reproduces_reference_full_size(ckpt, fixture):
    """BASELINE.json configs[0..3] at full size: SHA-256 of the whole buffers + strided samples"""
    from oracle import zvoracle
    z = np.load(os.path.join(GOLD, fixture))
    path, g, tensors = ckpt("medium", int(z["seed_w"]))
    T, N, mel, hid, ids, puncts, style = _inputs(g, tensors, z)
    s = int(z["stride"])
    orc = zvoracle.Oracle(tensors)
    e = orc.encoder(g, ids, puncts, style, T)
    assert e["n_frames"] == int(z["n_frames"])
    assert np.array_equal(e["pitch_bucket"], z["pitch_bucket"]) and np.array_equal(e["energy_bucket"], z["energy_bucket"])
    assert np.array_equal(e["logdur"], z["logdur"])
    assert np.array_equal(e["hidden"].reshape(-1)[::s], z["hidden_samples"])
    assert sha(e["hidden"]) == str(z["hidden_sha256"])
    if N != 128:       # decoder / vocoder inputs depend on T only: once per T (512: the N = 64 fixture; 1 024)
        d = orc.decoder(hid, style)
        assert np.array_equal(d.reshape(-1)[::s], z["mel_samples"]) and sha(d) == str(z["mel_sha256"])
        w = orc.vocoder(mel)
        assert np.array_equal(w[::s], z["wav_samples"]) and sha(w) == str(z["wav_sha256"])


def test_oracle_vs_live_reference_fresh_seed(tmp_path):
    """different weights seed + ragged sizes against the reference's outputs stored in tests/golden/fresh_tiny_seed99.npz,
    and live against oracle/_ref when it is present (which must still reproduce the stored outputs)"""
    from zerovox_cpp_amd import gguf, synth
    from oracle import zvoracle
    z = np.load(os.path.join(GOLD, "fresh_tiny_seed99.npz"))
    live = zvoracle.have_reference()
    g = synth.GEOMETRIES[str(z["geometry"])]
    path = str(tmp_path / "t.gguf")
    synth.write_checkpoint(path, g, int(z["seed_w"]), trim_dims=bool(z["trim_dims"]))      # ggml-C-writer style n_dims
    _, tensors = gguf.read_gguf(path)
    orc = zvoracle.Oracle(tensors)
    for T, N in z["cases"]:
        T, N = int(T), int(N)
        k = "T%d_N%d_" % (T, N)
        mel = synth.vocoder_mel(g, tensors, int(z["seed_mel"]), T)
        hid = synth.decoder_hidden(g, int(z["seed_hidden"]), T)
        ids, puncts, style = synth.encoder_inputs(g, int(z["seed_enc"]), N)
        assert np.array_equal(orc.vocoder(mel), z[k + "wav"])
        assert np.array_equal(orc.decoder(hid, style), z[k + "mel"])
        e = orc.encoder(g, ids, puncts, style, T)
        for name in ("hidden", "features", "logdur", "energy", "pitch_bucket", "energy_bucket"):
            assert np.array_equal(e[name], z[k + name]), name
        assert e["n_frames"] == int(z[k + "n_frames"])
        if live:
            assert np.array_equal(zvoracle.run_reference(path, T=T, voc=mel)["wav"], z[k + "wav"])
            assert np.array_equal(zvoracle.run_reference(path, T=T, dec=(hid, style))["mel"], z[k + "mel"])
            r = zvoracle.run_reference(path, T=T, N=N, enc=(ids, puncts, style), E=g.E)
            for name in ("hidden", "features", "logdur", "energy", "pitch_bucket", "energy_bucket"):
                assert np.array_equal(r[name], z[k + name]), name
            assert r["n_frames"] == int(z[k + "n_frames"])


def test_oracle_vs_reference_trained_family(tmp_path):
    """the "trained" weight family (synth.make_tensors: heavy-tailed f16 weights with exact zeros, f16 subnormals and pruned
    channels, norm gains that include 0 and negatives), a weights seed no other fixture uses and ragged sizes, against the
    reference's outputs stored in tests/golden/trained_small_seed2719_T72_N18.npz — the assertions of the fresh-seed case — and
    live against oracle/_ref when it is present"""
    from zerovox_cpp_amd import gguf, synth
    from oracle import zvoracle
    z = np.load(os.path.join(GOLD, "trained_small_seed2719_T72_N18.npz"))
    live = zvoracle.have_reference()
    g = synth.GEOMETRIES[str(z["geometry"])]
    path = str(tmp_path / "t.gguf")
    synth.write_checkpoint(path, g, int(z["seed_w"]), family=str(z["family"]))
    _, tensors = gguf.read_gguf(path)
    orc = zvoracle.Oracle(tensors)
    T, N = int(z["T"]), int(z["N"])
    mel = synth.vocoder_mel(g, tensors, int(z["seed_mel"]), T)
    hid = synth.decoder_hidden(g, int(z["seed_hidden"]), T)
    ids, puncts, style = synth.encoder_inputs(g, int(z["seed_enc"]), N)
    assert np.array_equal(orc.vocoder(mel), z["wav"])
    assert np.array_equal(orc.decoder(hid, style), z["mel"])
    e = orc.encoder(g, ids, puncts, style, T)
    for name in ("hidden", "features", "logdur", "energy", "pitch_bucket", "energy_bucket"):
        assert np.array_equal(e[name], z[name]), name
    assert e["n_frames"] == int(z["n_frames"])
    if live:
        assert np.array_equal(zvoracle.run_reference(path, T=T, voc=mel)["wav"], z["wav"])
        assert np.array_equal(zvoracle.run_reference(path, T=T, dec=(hid, style))["mel"], z["mel"])
        r = zvoracle.run_reference(path, T=T, N=N, enc=(ids, puncts, style), E=g.E)
        for name in ("hidden", "features", "logdur", "energy", "pitch_bucket", "energy_bucket"):
            assert np.array_equal(r[name], z[name]), name
        assert r["n_frames"] == int(z["n_frames"])


def test_instancenorm_known_answer():
    """the reference repo's only own golden data: utils/norm1dexample.json (PyTorch InstanceNorm1d(affine) pair,
    weights rounded to 4 decimals in the file -> 2e-4 tolerance)"""
    from oracle import zvoracle
    z = np.load(os.path.join(GOLD, "instnorm1d_kat.npz"))
    orc = zvoracle.Oracle({})
    y = orc.norm_rows(z["x_in"]) * z["weight"][:, None] + z["bias"][:, None]
    assert np.max(np.abs(y - z["x_out"])) < 2e-4


def test_length_regulator_edge_cases():
    from oracle import zvoracle
    orc = zvoracle.Oracle({})
    feat = np.arange(12, dtype=np.float32).reshape(3, 4)
    # durations: exp(ld)-1 -> 0.4 (-> 0), 2.5 (-> 3: truncating x+0.5, not half-even), 100 (clipped at T)
    ld = np.log(np.array([1.4, 3.5, 101.0], np.float32)).astype(np.float32)
    hid, nf = orc.length_regulator(feat, ld, 6)
    assert nf == 6 and np.array_equal(hid[:3], np.repeat(feat[1:2], 3, 0)) and np.array_equal(hid[3:], np.repeat(feat[2:3], 3, 0))
    hid, nf = orc.length_regulator(feat, np.full(3, -5, np.float32), 4)
    assert nf == 0 and not hid.any()


def test_oracle_self_noise_floor(ckpt):
    """re-association noise of the reference semantics (SURVEY.md Appx D): bounded, and the reason GPU gates are
    noise-aware.  wav floor stays well under the 1e-4 RMS gate at speech-like amplitude."""
    from zerovox_cpp_amd import synth
    from oracle import zvoracle
    path, g, tensors = ckpt("small")
    mel = synth.vocoder_mel(g, tensors, 7, 32)
    orc = zvoracle.Oracle(tensors)
    a = orc.vocoder(mel)
    orc.set_order(zvoracle.ORDER_SEQ_F32)
    b = orc.vocoder(mel)
    floor = float(np.sqrt(np.mean((a.astype(np.float64) - b) ** 2)))
    assert 0 < floor < 6e-5


@pytest.mark.parametrize("k,dil,ic,oc,L", [(3, 1, 24, 40, 50), (7, 3, 32, 32, 97), (11, 5, 16, 48, 130), (1, 1, 33, 17, 20)])
def test_oracle_conv_against_independent_torch_fp32(k, dil, ic, oc, L):
    """an implementation that shares no code with the oracle: torch's fp32 conv1d on operands rounded to f16 exactly where
    ggml rounds them (the im2col of the activations, the stored weights).  Products of two f16 values are exact in f32, so
    the two differ only by f32 summation order: a few ulp of the accumulated magnitude"""
    import torch
    from oracle import zvoracle
    rng = np.random.default_rng(k * 100 + dil)
    x = rng.standard_normal((ic, L)).astype(np.float32)               # channels-first, like the reference's conv input
    w = (rng.standard_normal((oc, ic, k)) / np.sqrt(ic * k)).astype(np.float16)
    b = rng.standard_normal(oc).astype(np.float32)
    pad = (k - 1) // 2 * dil
    got = zvoracle.Oracle({}).conv1d(x, w, b, pad, dil)
    x16 = torch.from_numpy(x.astype(np.float16).astype(np.float32))[None]
    ref = torch.nn.functional.conv1d(x16, torch.from_numpy(w.astype(np.float32)), torch.from_numpy(b), padding=pad, dilation=dil)[0].numpy()
    assert got.shape == ref.shape == (oc, L)
    assert np.max(np.abs(got - ref)) <= 2e-5 * max(1.0, float(np.max(np.abs(ref))))


def test_oracle_reproduces_reference_demo_utterance(ckpt):
    """ZeroVOXModel::eval() of the reference (its hard-coded 120-phoneme utterance + 528-float style vector, the three
    stages back to back at T = max_seq_len, src/zerovox.cpp:198-335) on the synthetic medium checkpoint: the oracle
    chain reproduces every stage of the compiled reference bit for bit.  The utterance data is served by the product
    library (zv_demo_utterance), which needs no GPU."""
    from zerovox_cpp_amd import capi
    from oracle import zvoracle
    z = np.load(os.path.join(GOLD, "demo_medium_T1500.npz"))
    path, g, tensors = ckpt("medium", int(z["seed_w"]))
    ids, puncts, style = capi.demo_utterance()
    assert len(ids) == 120 == int(z["N"]) and style.shape == (528,) and g.E == 528
    assert ids[0] == 69 and ids[-1] == 87 and puncts[-1] == 3            # first / last entries of the reference's literals
    T, s = int(z["T"]), int(z["stride"])
    assert T == g.max_seq_len
    orc = zvoracle.Oracle(tensors)
    e = orc.encoder(g, ids, puncts, style, T)
    assert e["n_frames"] == int(z["n_frames"])
    for k in ("logdur", "energy", "pitch_bucket", "energy_bucket"):
        assert np.array_equal(e[k], z[k]), k
    assert sha(e["features"]) == str(z["features_sha256"]) and sha(e["hidden"]) == str(z["hidden_sha256"])
    mel = orc.decoder(e["hidden"], style)
    assert np.array_equal(mel.reshape(-1)[::s], z["mel_samples"]) and sha(mel) == str(z["mel_sha256"])
    wav = orc.vocoder(mel)
    assert np.array_equal(wav[::s], z["wav_samples"]) and sha(wav) == str(z["wav_sha256"])


def test_oracle_reproduces_reference_num_phonemes_below_max(ckpt):
    """FS2Encoder::eval(num_phonemes < max_n_phonemes): all tokens are encoded, the regulator walks the first num
    (reference src/fs2encoder.cpp:594-650)"""
    from zerovox_cpp_amd import synth
    from oracle import zvoracle
    z = np.load(os.path.join(GOLD, "small_T64_N16_num9.npz"))
    path, g, tensors = ckpt("small", int(z["seed_w"]))
    ids, puncts, style = synth.encoder_inputs(g, int(z["seed_enc"]), int(z["N"]))
    e = zvoracle.Oracle(tensors).encoder(g, ids, puncts, style, int(z["T"]), num_phonemes=int(z["num"]))
    assert e["n_frames"] == int(z["n_frames"]) and np.array_equal(e["hidden"], z["hidden"])
    assert np.array_equal(e["logdur"], z["logdur"]) and sha(e["features"]) == str(z["features_sha256"])


def test_oracle_layers_compose_to_the_oracle_vocoder(tmp_path):
    """zvo_layer's vocoder kinds (input conv, transposed convs, residual blocks, output conv: the per-layer checkers of
    tests/test_gpu_layers.py) chained by hand reproduce zvo_vocoder — which reproduces the compiled reference — bit for bit"""
    from zerovox_cpp_amd import gguf, synth
    from oracle import zvoracle
    g = synth.TINY
    path = str(tmp_path / "tiny.gguf")
    synth.write_checkpoint(path, g, 1234)
    _, t = gguf.read_gguf(path)
    o = zvoracle.Oracle(t)
    mel = synth.vocoder_mel(g, t, 7, 16)
    x = o.layer(o.LAYER_VOC_INPUT, 0, mel, g.voc_channels)
    for i, s in enumerate(g.upsample_scales):
        up = o.layer(o.LAYER_VOC_UPSAMPLE, i, x, x.shape[1] // 2, out_rows=x.shape[0] * s)
        ys = [o.layer(o.LAYER_VOC_RESBLOCK, i * 3 + j, up, up.shape[1]) for j in range(3)]
        x = ((ys[0] + ys[1]) + ys[2]) * np.float32(1.0 / np.float32(3))          # src/hifigan.cpp:300-315
    assert np.array_equal(o.layer(o.LAYER_VOC_OUTPUT, 0, x, 0), o.vocoder(mel))


@pytest.mark.parametrize("geom", ["medium_h1", "medium_h3", "medium_h4", "medium_h8"])
def test_oracle_encoder_at_other_head_counts(ckpt, geom):
    """`encoder.head` is read from the checkpoint (reference src/zerovox.cpp, src/fs2encoder.cpp:71-140 splits E into H heads of
    dk = E / H); every other fixture has H = 2.  At H = 1, 3, 4, 8 (dk = 528, 176, 132, 66) and 37 / 300 / 450 tokens the oracle's
    encoder must reproduce the reference's outputs stored in tests/golden/medium_heads.npz bit for bit — and, where oracle/_ref is
    built, a live run of the reference must still reproduce the stored outputs"""
    from zerovox_cpp_amd import synth
    from oracle import zvoracle
    z = np.load(os.path.join(GOLD, "medium_heads.npz"))
    assert geom in [str(x) for x in z["geometries"]]
    path, g, tensors = ckpt(geom, int(z["seed_w"]))
    assert g.E % g.encoder_head == 0 and g.encoder_head != 2
    orc = zvoracle.Oracle(tensors)
    live = zvoracle.have_reference()
    for N, T in z["cases"]:
        N, T = int(N), int(T)
        k = "%s_N%d_" % (geom, N)
        ids, puncts, style = synth.encoder_inputs(g, int(z["seed_enc"]), N)
        e = orc.encoder(g, ids, puncts, style, T)
        for name in ("logdur", "energy", "pitch_bucket", "energy_bucket"):
            assert np.array_equal(e[name], z[k + name]), (N, name)
        assert e["n_frames"] == int(z[k + "n_frames"])
        assert sha(e["features"]) == str(z[k + "features_sha256"]) and sha(e["hidden"]) == str(z[k + "hidden_sha256"])
        assert np.array_equal(e["pitch"], z[k + "pitch"])
        if live:
            r = zvoracle.run_reference(path, T=T, N=N, enc=(ids, puncts, style), E=g.E)
            assert np.array_equal(r["logdur"], z[k + "logdur"]) and sha(r["hidden"]) == str(z[k + "hidden_sha256"])


def test_oracle_value_ranges_small(ckpt):
    """the oracle at the value-range edges (tests/golden/value_ranges_small.npz: a decoder hidden with per-channel offsets up to
    1e3 sigma, constant channels and an all-zero band; a vocoder mel in magnitude bands, the first exactly at hifigan.mean)
    against the reference's outputs bit for bit, and live against oracle/_ref where it is present"""
    import parity_helpers as ph
    from oracle import zvoracle
    z = np.load(os.path.join(GOLD, "value_ranges_small.npz"))
    path, g, tensors = ckpt(str(z["geometry"]), int(z["seed_w"]))
    hid, style, mel_in, _, _ = ph.value_range_stage_inputs(g, tensors)
    s = int(z["stride"])
    orc = zvoracle.Oracle(tensors)
    mel, wav = orc.decoder(hid, style), orc.vocoder(mel_in)
    assert np.array_equal(mel.reshape(-1)[::s], z["mel_samples"]) and sha(mel) == str(z["mel_sha256"])
    assert np.array_equal(wav[::s], z["wav_samples"]) and sha(wav) == str(z["wav_sha256"])
    if zvoracle.have_reference():
        assert sha(zvoracle.run_reference(path, T=hid.shape[0], dec=(hid, style))["mel"]) == str(z["mel_sha256"])
        assert sha(zvoracle.run_reference(path, T=mel_in.shape[0], voc=mel_in)["wav"]) == str(z["wav_sha256"])


def test_oracle_layernorm_alone_on_value_range_rows(ckpt):
    """ZVO_LAYER_ENC_LN (the LayerNorm alone, used by the value-range tests) against an f64 LayerNorm of the same rows: constant
    rows give b exactly, the others agree to f32 rounding"""
    import parity_helpers as ph
    from oracle import zvoracle
    path, g, tensors = ckpt("small")
    x, reg = ph.ln_rows(2200, 40, g.E)
    o = zvoracle.Oracle(tensors)
    for j, sub in ((0, "slf_attn"), (1, "pos_ffn")):
        y = o.layer(o.LAYER_ENC_LN, 2 + j, x, g.E)
        w = tensors[f"_pe._enc.laystk.1.{sub}.layer_norm.w"].astype(np.float64)
        b = tensors[f"_pe._enc.laystk.1.{sub}.layer_norm.b"].astype(np.float64)
        xd = x.astype(np.float64)
        want = (xd - xd.mean(1, keepdims=True)) / np.sqrt(xd.var(1, keepdims=True) + 1e-5) * w + b
        c = dict(reg)["constant rows"]
        assert np.array_equal(y[c], np.broadcast_to(b.astype(np.float32), y[c].shape))
        assert np.max(np.abs(y - want)) <= 1e-5 * np.max(np.abs(want))


def test_oracle_resblock_geometries(ckpt):
    """the oracle on checkpoints whose residual-block convs have other tap counts (synth.RESBLOCK_GEOMETRIES: 3 / 5 / 7, 15 / 9 / 1,
    a branch whose last dilation pair is narrower, convs1 and convs2 of one pair with different K) against the reference's
    vocoder outputs (tests/golden/resblock_geometries_T24.npz) bit for bit, plus one decoder -> vocoder chain; and live against
    oracle/_ref where it is present"""
    from zerovox_cpp_amd import synth
    from oracle import zvoracle
    z = np.load(os.path.join(GOLD, "resblock_geometries_T24.npz"))
    T, s = int(z["T"]), int(z["stride"])
    assert tuple(str(n) for n in z["geometries"]) == synth.RESBLOCK_GEOMETRIES
    for gname in synth.RESBLOCK_GEOMETRIES:
        path, g, tensors = ckpt(gname, int(z["seed_w"]))
        orc = zvoracle.Oracle(tensors)
        mel_in = synth.vocoder_mel(g, tensors, int(z["seed_mel"]), T)
        wav = orc.vocoder(mel_in)
        assert np.array_equal(wav[::s], z[gname + "/wav_samples"]) and sha(wav) == str(z[gname + "/wav_sha256"]), gname
        if zvoracle.have_reference():
            assert sha(zvoracle.run_reference(path, T=T, voc=mel_in)["wav"]) == str(z[gname + "/wav_sha256"]), gname
        if gname == str(z["chain"]):
            hid = synth.decoder_hidden(g, int(z["seed_hidden"]), T)
            style = synth.encoder_inputs(g, int(z["seed_style"]), 8)[2]
            mel = orc.decoder(hid, style)
            assert np.array_equal(mel.reshape(-1)[::s], z["chain_mel_samples"]) and sha(mel) == str(z["chain_mel_sha256"])
            cw = orc.vocoder(mel)
            assert np.array_equal(cw[::s], z["chain_wav_samples"]) and sha(cw) == str(z["chain_wav_sha256"])
            if zvoracle.have_reference():
                assert sha(zvoracle.run_reference(path, T=T, dec=(hid, style))["mel"]) == str(z["chain_mel_sha256"])


def test_oracle_voc_widths(ckpt):
    """the oracle on checkpoints of 256, 496, 768 and 1 024 vocoder channels (synth.VOC_WIDTH_GEOMETRIES) against the reference's
    vocoder outputs (tests/golden/voc_widths_T24.npz) bit for bit; and live against oracle/_ref where it is present.  The reference
    takes all four widths (it reads every channel count from the tensors' shapes): none stands on the oracle alone"""
    from zerovox_cpp_amd import synth
    from oracle import zvoracle
    z = np.load(os.path.join(GOLD, "voc_widths_T24.npz"))
    T, s = int(z["T"]), int(z["stride"])
    assert tuple(str(n) for n in z["geometries"]) == synth.VOC_WIDTH_GEOMETRIES
    for gname in synth.VOC_WIDTH_GEOMETRIES:
        path, g, tensors = ckpt(gname, int(z["seed_w"]))
        orc = zvoracle.Oracle(tensors)
        mel_in = synth.vocoder_mel(g, tensors, int(z["seed_mel"]), T)
        wav = orc.vocoder(mel_in)
        assert wav.shape == (T * g.hop_size,), gname
        assert np.array_equal(wav[::s], z[gname + "/wav_samples"]) and sha(wav) == str(z[gname + "/wav_sha256"]), gname
        if zvoracle.have_reference():
            assert sha(zvoracle.run_reference(path, T=T, voc=mel_in)["wav"]) == str(z[gname + "/wav_sha256"]), gname


def test_oracle_encdec_geometries(ckpt):
    """the oracle on checkpoints of other widths, FFN tap counts, predictor widths and mel counts (synth.ENCDEC_GEOMETRIES: E = 576 /
    720 / 304 / 1 024, FFN taps (3, 3) / (17, 1) / (1, 5), V = 784, one encoder layer, 128 / 272 / 16 mels) against the reference's
    encoder, decoder and vocoder outputs (tests/golden/encdec_geometries_N16_T24.npz) bit for bit; every shape it runs comes from the
    checkpoint (a num_mels or FFN tap count given that disagrees raises); and live against oracle/_ref where it is present"""
    from zerovox_cpp_amd import synth
    from oracle import zvoracle
    z = np.load(os.path.join(GOLD, "encdec_geometries_N16_T24.npz"))
    N, T_enc, T, s = int(z["N"]), int(z["T_enc"]), int(z["T"]), int(z["stride"])
    assert tuple(str(n) for n in z["geometries"]) == synth.ENCDEC_GEOMETRIES
    for gname in synth.ENCDEC_GEOMETRIES:
        path, g, tensors = ckpt(gname, int(z["seed_w"]))
        orc = zvoracle.Oracle(tensors)
        assert orc.num_mels == g.num_mels and orc.ffn_taps == tuple(g.conv_kernel_size), gname
        ids, puncts, style = synth.encoder_inputs(g, int(z["seed_enc"]), N)
        e = orc.encoder(g, ids, puncts, style, T_enc)
        for name in ("logdur", "energy", "pitch_bucket", "energy_bucket"):
            assert np.array_equal(e[name], z[f"{gname}/{name}"]), (gname, name)
        assert e["n_frames"] == int(z[gname + "/n_frames"]), gname
        assert sha(e["features"]) == str(z[gname + "/features_sha256"]) and sha(e["hidden"]) == str(z[gname + "/hidden_sha256"]), gname
        hid = synth.decoder_hidden(g, int(z["seed_hidden"]), T)
        dstyle = synth.encoder_inputs(g, int(z["seed_style"]), 8)[2]
        mel = orc.decoder(hid, dstyle)
        assert mel.shape == (T, g.num_mels), gname
        assert np.array_equal(mel.reshape(-1)[::s], z[gname + "/mel_samples"]) and sha(mel) == str(z[gname + "/mel_sha256"]), gname
        wav = orc.vocoder(mel)
        assert np.array_equal(wav[::s], z[gname + "/wav_samples"]) and sha(wav) == str(z[gname + "/wav_sha256"]), gname
        with pytest.raises(ValueError):
            orc.decoder(hid, dstyle, num_mels=g.num_mels + 16)
        with pytest.raises(ValueError):
            orc.layer(orc.LAYER_ENC_FFN, 0, np.zeros((4, g.E), np.float32), g.E, heads=g.encoder_head, ksz=(g.conv_kernel_size[0] + 2, 1))
        if zvoracle.have_reference():
            r = zvoracle.run_reference(path, T=T, dec=(hid, dstyle))
            assert r["mel"].shape == (T, g.num_mels) and sha(r["mel"]) == str(z[gname + "/mel_sha256"]), gname
            assert sha(zvoracle.run_reference(path, T=T, voc=mel)["wav"]) == str(z[gname + "/wav_sha256"]), gname
            r = zvoracle.run_reference(path, T=T_enc, N=N, enc=(ids, puncts, style), E=g.E)
            assert np.array_equal(r["logdur"], e["logdur"]) and sha(r["hidden"]) == str(z[gname + "/hidden_sha256"]), gname
