"""-m gpu: the encoder and decoder at other widths, FFN tap counts, predictor widths and mel counts (synth.ENCDEC_GEOMETRIES).

The reference reads E = emb_dim + punct_emb_dim, the FFN convs' tap counts, encoder.vp_filter_size, encoder.layer and
audio.num_mels from the checkpoint; so does the loader.  Every other test runs E = 64, 128 or 528, FFN taps (9, 1) and 80 mels.
Per geometry (R = 64; the decoder's wide convs have E and 2E output channels, batches run whole groups of 8 32-channel tiles on
conv_gemm_kernel and two or more leftovers on conv1d_mfma_kernel from tile nt_begin on):
  * medium_e576: 18 / 36 tiles, GEMM 16 / 32 + 2 / 4 at nt_begin (the generic kernel's tile span and its InstanceNorm partial
    sums for those channels); dk = 288, the matrix-core attention's widest head, which falls back to the scalar kernel by LDS
    above 320 tokens (encode at N = 321); 128 mels; a 3-tap FFN w_2 over 1 024 f16 channels, run per utterance;
  * medium_e720: 23 / 45 tiles, 7 / 5 leftover, the last tile half padding; dk = 240; 272 mels: the vocoder input conv stages two
    256-channel chunks under its (mel - mean) / scale prologue, to_out has 8.5 tiles; V = 784 turns the LayerNorm tails off by V
    alone (the predictors' wide-row LayerNorm on a Vp-strided buffer); a 17-tap FFN w_1 (16 halo rows);
  * small_e304: 10 / 19 tiles, GEMM 8 / 16 + 2 / 3; one encoder layer; 16 mels; an FFN operand of 200 -> 208 columns, 1-tap w_1
    and 5-tap w_2;
  * medium_e1024: the whole encoder with the tails off by E; decoder convs of 2 048 / 2 112 channels, GEMM groups with no leftover.
Checked: every encoder, predictor and decoder layer alone against the oracle (the decoder blocks with and without the operand
pre-pass, and on conv_gemm_kernel + the generic remainder at 96 frames with the default's bits); decode, encode (near-tie
accounting against the oracle's own re-association noise) and vocode against the oracle; every conv / attention / LayerNorm
regime's bits; ragged batches of >= 16 384 frame rows (the GEMM path by itself) eager, captured and replayed against stand-alone
calls.  Also: the loader refuses 100 mels and an even FFN tap count."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ZV_ERR_SHAPE = 4
WAV_RMS_GATE = 1e-4                 # tests/test_gpu_vocoder.py


def _geoms():
    from zerovox_cpp_amd import synth
    return synth.ENCDEC_GEOMETRIES


_M = {}


def _model(ckpt, gname):
    from zerovox_cpp_amd import capi
    if gname not in _M:
        _M[gname] = capi.Model(ckpt(gname)[0], 0)
    return _M[gname]


def teardown_module(module):
    for m in _M.values():
        m.close()
    _M.clear()


def _rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))


def _decoder_widths(g):
    E, R = g.E, g.residual_dim
    return [E, 2 * E, 2 * E + R, 2 * E + R, 2 * E + R, E, E], [2 * E, 2 * E, 2 * E, 2 * E, E, E, E]


@pytest.mark.parametrize("gname", _geoms())
def test_every_encoder_layer(ckpt, gname):
    """every layer's attention sublayer (both attention kernels, same bits), feed-forward sublayer and whole FFT block, and the three
    variance predictors, on 96 tokens against the oracle at the checkpoint's heads and FFN taps"""
    from zerovox_cpp_amd import capi
    from oracle import zvoracle
    from parity_helpers import layer_gate, oracle_pair
    _, g, tensors = ckpt(gname)
    m = _model(ckpt, gname)
    o = zvoracle.Oracle(tensors)
    kw = dict(heads=g.encoder_head, ksz=g.conv_kernel_size)
    for layer in range(g.encoder_layer):
        x = np.random.default_rng(200 + layer).standard_normal((96, g.E)).astype(np.float32)
        ref, alt = oracle_pair(o, "layer", o.LAYER_ENC_MHA, layer, x, g.E, **kw)
        outs = {}
        for sw in ("ZV_ATT_SCALAR", "ZV_ATT_MFMA"):
            with capi.switches(**{sw: 1}):
                outs[sw] = m.debug_layer(m.LAYER_ENC_MHA, layer, x, g.E)
            layer_gate(f"{gname} attention {layer} {sw}", outs[sw], ref, alt, 1e-4)
        assert np.array_equal(outs["ZV_ATT_SCALAR"], outs["ZV_ATT_MFMA"]), (gname, layer)
        for kind, okind, nm in ((m.LAYER_ENC_FFN, o.LAYER_ENC_FFN, "feed-forward"), (m.LAYER_ENC_FFT, o.LAYER_ENC_FFT, "FFT block")):
            got = m.debug_layer(kind, layer, x, g.E)
            ref, alt = oracle_pair(o, "layer", okind, layer, x, g.E, **kw)
            layer_gate(f"{gname} {nm} {layer} K={g.conv_kernel_size}", got, ref, alt, 1e-4)
    # (one value per token: 320 tokens (small_e304: its 256), so that the rms rests on more than a handful of f16 re-rounding flips; at V = 64 the
    # oracle's own two orders still differ on only a few of them, hence 3 x its noise)
    for p in range(3):
        x = np.random.default_rng(400 + p).standard_normal((min(320, g.max_seq_len), g.E)).astype(np.float32)
        got = m.debug_layer(m.LAYER_VAR_PRED, p, x, 0)
        ref, alt = oracle_pair(o, "layer", o.LAYER_VAR_PRED, p, x, 0, ksz=(g.vp_kernel_size,))
        layer_gate(f"{gname} variance predictor {p} V={g.vp_filter_size}", got, ref, alt, 1e-4, floor_mult=3.0)


@pytest.mark.parametrize("gname", _geoms())
def test_every_decoder_layer(ckpt, gname):
    """the 7 decoder residual blocks with and without the operand pre-pass (and, behind the pre-pass, conv_gemm_kernel + the generic
    kernel's remainder tiles forced on at 96 frames: the default's bits), the 10 AdaIN layers, asr_res, to_out (Cout = num_mels)
    and the vocoder input conv (Cin = num_mels under the (mel - mean) / scale prologue), 96 frames, against the oracle"""
    from zerovox_cpp_amd import capi, synth
    from oracle import zvoracle
    from parity_helpers import layer_gate, oracle_pair
    _, g, tensors = ckpt(gname)
    m = _model(ckpt, gname)
    o = zvoracle.Oracle(tensors)
    T, E = 96, g.E
    cin, cout = _decoder_widths(g)
    style = (0.05 * np.random.default_rng(7).standard_normal(E)).astype(np.float32)
    for block in range(7):
        x = (1.2 * np.random.default_rng(300 + block).standard_normal((T, cin[block]))).astype(np.float32)
        ref, alt = oracle_pair(o, "layer", o.LAYER_DEC_BLOCK, block, x, cout[block], style=style)
        for pre in (0, 1):
            with capi.switches(ZV_DEC_PREPASS=pre):
                got = m.debug_layer(m.LAYER_DEC_BLOCK, block, x, cout[block], style=style)
            layer_gate(f"{gname} decoder block {block} ({cin[block]}->{cout[block]}) prepass={pre}", got, ref, alt, 3e-4)
            with capi.switches(ZV_DEC_PREPASS=pre, ZV_CONV_GEMM=2):
                gemm = m.debug_layer(m.LAYER_DEC_BLOCK, block, x, cout[block], style=style)
            assert np.array_equal(gemm, got), (gname, block, pre, "conv_gemm_kernel + remainder")
    adain_c = [c for i in range(5) for c in (cin[2 + i], cout[2 + i])]
    for idx, C in enumerate(adain_c):
        x = (1.2 * np.random.default_rng(600 + idx).standard_normal((T, C)) + 0.3).astype(np.float32)
        got = m.debug_layer(m.LAYER_DEC_ADAIN, idx, x, C, style=style)
        ref, alt = oracle_pair(o, "layer", o.LAYER_DEC_ADAIN, idx, x, C, style=style)
        layer_gate(f"{gname} AdaIN {idx} (C={C})", got, ref, alt, 1e-5, floor_mult=4.0)
    x = (1.1 * np.random.default_rng(44).standard_normal((T, E))).astype(np.float32)
    for kind, okind, C, nm in ((m.LAYER_DEC_ASR_RES, o.LAYER_DEC_ASR_RES, g.residual_dim, "asr_res"),
                               (m.LAYER_DEC_TO_OUT, o.LAYER_DEC_TO_OUT, g.num_mels, "to_out")):
        got = m.debug_layer(kind, 0, x, C)
        ref, alt = oracle_pair(o, "layer", okind, 0, x, C)
        assert got.shape == (T, C)
        layer_gate(f"{gname} {nm} (C={C})", got, ref, alt, 1e-4)
    mel = synth.vocoder_mel(g, tensors, 41, T)
    got = m.debug_layer(m.LAYER_VOC_INPUT, 0, mel, g.voc_channels)
    ref, alt = oracle_pair(o, "layer", o.LAYER_VOC_INPUT, 0, mel, g.voc_channels)
    layer_gate(f"{gname} vocoder input conv (M={g.num_mels})", got, ref, alt, 1e-4)


@pytest.mark.parametrize("gname", _geoms())
def test_stages_match_oracle(ckpt, gname):
    """decode at T = 1, 37, 200 (gates of test_gpu_decoder_encoder.py::test_decoder_matches_oracle); encode at N = 1, 33, 321 with the decisions'
    near-tie accounting against the oracle's own re-association noise (its float floors the largest of the three runs'), and the regulator teacher-forced bit-exact; vocode of the
    new mel count at 37 frames within the waveform gate"""
    from zerovox_cpp_amd import synth
    from oracle import zvoracle
    from parity_helpers import encoder_decisions_vs_reference, encoder_margins, oracle_pair
    _, g, tensors = ckpt(gname)
    m = _model(ckpt, gname)
    o = zvoracle.Oracle(tensors)
    _, _, style = synth.encoder_inputs(g, 5, 4)
    for T in (1, 37, 200):
        hid = synth.decoder_hidden(g, 60 + T, T, frames_per_phoneme=1, fill=1.0)
        mel = m.decode(hid, style)
        ref, alt = oracle_pair(o, "decoder", hid, style)
        d, floor = mel - ref, alt - ref
        print(f"{gname} decode T={T}: rms {_rms(d):.3e} max {np.max(np.abs(d)):.3e} (floor rms {_rms(floor):.3e} max {np.max(np.abs(floor)):.3e})")
        assert mel.shape == (T, g.num_mels) and np.isfinite(mel).all(), T
        assert _rms(d) <= 1.5 * _rms(floor) + 1e-6 and np.max(np.abs(d)) <= 2.0 * np.max(np.abs(floor)) + 1e-6, (gname, T)
    nb = g.ve_n_bins - 1
    runs = []
    for N in (1, 33, 321):
        N = min(N, g.max_seq_len)
        ids, puncts, sty = synth.encoder_inputs(g, 70 + N, N)
        T = min(8 * N + 16, 1500)
        runs.append((N, T, m.encode(ids, puncts, sty, T), encoder_margins(*oracle_pair(o, "encoder", g, ids, puncts, sty, T))))
    # the float floors are the checkpoint's: the largest of the three runs' (one token's own re-association noise is one draw)
    floors = {k: max(z[k] for *_, z in runs) for k in ("floor_logdur_max", "floor_pitch_max", "floor_energy_max")}
    for N, T, e, z in runs:
        encoder_decisions_vs_reference(e, dict(z, **floors), nb, T, count_energy_near_pitch=False)
        hid, nf = o.length_regulator(e["features"], e["logdur"], T)
        assert nf == e["n_frames"] and np.array_equal(hid, e["hidden"]), (gname, N)
    mel = synth.vocoder_mel(g, tensors, 7, 37)
    wav, ref = m.vocode(mel), o.vocoder(mel)
    err = _rms(wav - ref)
    print(f"{gname} vocode M={g.num_mels}: wav rms err {err:.3e}, signal rms {_rms(ref):.3f}")
    assert wav.shape == ref.shape and err <= WAV_RMS_GATE


REGIMES = (("prepass_0", {"ZV_DEC_PREPASS": 0}), ("prepass_1", {"ZV_DEC_PREPASS": 1}), ("gemm_0", {"ZV_CONV_GEMM": 0}),
           ("gemm_2", {"ZV_CONV_GEMM": 2}), ("prepass_1_gemm_2", {"ZV_DEC_PREPASS": 1, "ZV_CONV_GEMM": 2}),
           ("gemm_2_plain_grid", {"ZV_DEC_PREPASS": 1, "ZV_CONV_GEMM": 2, "ZV_CONV_XCD": 0}),
           ("single_0", {"ZV_CONV_SINGLE": 0}), ("single_2", {"ZV_CONV_SINGLE": 2}), ("plain_grid", {"ZV_CONV_XCD": 0}),
           ("nt_1", {"ZV_CONV_NT": 1}), ("nt_2", {"ZV_CONV_NT": 2}), ("linear_per_utterance", {"ZV_LINEAR_MERGED": 0}),
           ("no_ln_tail", {"ZV_LN_TAIL": 0}), ("att_scalar", {"ZV_ATT_SCALAR": 1}), ("att_mfma", {"ZV_ATT_MFMA": 1}))
ENC_TAPS = ("logdur", "pitch", "energy", "pitch_bucket", "energy_bucket", "features", "hidden")


@pytest.mark.parametrize("gname", _geoms())
def test_kernel_regimes_give_the_same_bits(ckpt, gname):
    """decode (300 frames: the operand pre-pass by default) and encode (200 tokens) under every regime of the conv, attention,
    linear and LayerNorm launches: every output the default's bits"""
    from zerovox_cpp_amd import capi, synth
    _, g, tensors = ckpt(gname)
    m = _model(ckpt, gname)
    hid = synth.decoder_hidden(g, 77, 300)
    N = min(200, g.max_seq_len)
    ids, puncts, style = synth.encoder_inputs(g, 78, N)
    mel0, e0 = m.decode(hid, style), m.encode(ids, puncts, style, 1200)
    for name, env in REGIMES:
        with capi.switches(**env):
            mel, e = m.decode(hid, style), m.encode(ids, puncts, style, 1200)
        assert np.array_equal(mel, mel0), (gname, name, "decode")
        assert e["n_frames"] == e0["n_frames"], (gname, name)
        for k in ENC_TAPS:
            assert np.array_equal(e[k], e0[k]), (gname, name, k)


# (N, T) per utterance: mixed lengths, T up to 1 500 over 12 utterances (>= 16 384 frame rows: conv_gemm_kernel without a knob)
BATCH = [(1, 1), (3, 7), (17, 40), (40, 100), (90, 333), (33, 65), (150, 700), (200, 900), (400, 1500), (300, 1200), (120, 480),
         (250, 1100)]


@pytest.mark.parametrize("gname", _geoms())
def test_ragged_batch_equals_standalone(ckpt, gname):
    """zv_synthesize_batch of 12 ragged utterances: eager, graph capture and graph replay each give every utterance's stand-alone
    bits — with a multi-tap FFN w_2 run per utterance, an utterance that read another's token rows would differ"""
    from zerovox_cpp_amd import synth
    _, g, tensors = ckpt(gname)
    m = _model(ckpt, gname)
    utts = [(*synth.encoder_inputs(g, 9000 + 13 * i + N, min(N, g.max_seq_len)), T) for i, (N, T) in enumerate(BATCH)]
    assert len(utts) * max(T for *_, T in utts) >= 16384
    got = m.synthesize_batch(utts)
    m.set_graph_mode(True)
    try:
        got_c = m.synthesize_batch(utts)          # capture
        got_r = m.synthesize_batch(utts)          # replay
    finally:
        m.set_graph_mode(False)
    for i, ((ids, puncts, style, T), (w, nf), (wc, nfc), (wr, nfr)) in enumerate(zip(utts, got, got_c, got_r)):
        ref, nf_ref = m.synthesize(ids, puncts, style, T)
        assert nf == nfc == nfr == nf_ref and 0 < nf <= T and np.isfinite(w).all(), (gname, i)
        assert np.array_equal(w, ref) and np.array_equal(wc, ref) and np.array_equal(wr, ref), (gname, i)


@pytest.mark.parametrize("gname,what", [("medium_m100", "num_mels"), ("medium_ffn8", "_pe._enc.laystk.0.pos_ffn.w_1.w")])
def test_loader_refuses(ckpt, gname, what):
    """100 mels (the loader requires num_mels % 16 == 0; the reference does not — a known gap) and an 8-tap FFN conv (not a 'same'
    conv): ZV_ERR_SHAPE with a message naming it, at load"""
    from zerovox_cpp_amd import capi
    path, g, _ = ckpt(gname)
    with pytest.raises(capi.ZvError) as ei:
        capi.Model(path, 0)
    print(ei.value)
    assert ei.value.status == ZV_ERR_SHAPE and what in str(ei.value)
