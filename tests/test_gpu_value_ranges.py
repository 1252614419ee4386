"""GPU: every layer kind at the edges of the value range, one layer at a time (zv_debug_layer) against the oracle's layer.

The other parity tests feed values near 1.  Here the inputs are the families of parity_helpers: magnitude bands along time
from 2^-22 (every f16 operand subnormal) to 2^12, per-channel / per-row offsets up to 1e3 sigma with constant channels and
variances at and far below eps, sparse inputs (90 % exact +-0, heavy tail), inputs whose largest f16 operand is near 65504,
single elements that round to +-inf in f16, and attention logits far above 88 with exactly tied keys.

Gates (parity_helpers.region_gates): layer_gate on every gated region alone, its floor the farther of the oracle's sequential-f32
and f64 orders from its AVX2 order on that region, and the f64 judge (the oracle in ORDER_SEQ_F64 on the same f16 operand points:
2 x the farther f32 order's distance, DESIGN.md section 2 gate 7) on it.  LayerNorm rows go through LAYER_ENC_LN (the LayerNorm
alone), so the crafted rows are its input.  For the banded family also the response to
the input, f(x) - f(0), from the GPU and the oracle alike: the synthetic biases (~0.1) would swamp a 2^-22 band.  Where an
input rounds to inf, the GPU's non-finite values must cover the oracle's, every GPU inf must be the oracle's, and the rows
that read no such input must be finite and pass the usual gates (parity_helpers.nonfinite_footprint).  The batch kernels (parity_helpers.BATCH_REGIME) and the two
attention kernels must give the default's bits here too."""
import numpy as np
import pytest

import parity_helpers as ph

pytestmark = pytest.mark.gpu
_M = {}

RES_BLOCKS = (0, 4, 8, 11)          # one residual block of each stage: k = 3, 7, 11, 11
UPSAMPLES = (0, 3)                  # conv_gemm (deep) / conv_stream (memory-bound) under BATCH_REGIME
DEC_BLOCKS = (0, 4)                 # ResBlk1d (affine InstanceNorm, E -> 2E) / AdainResBlk1d (2E + R -> E, learned shortcut)
ADAINS = (0, 5, 9)


@pytest.fixture(scope="module")
def env(ckpt):
    from zerovox_cpp_amd import capi
    from oracle import zvoracle
    if "m" not in _M:
        path, g, tensors = ckpt("medium")
        _M.update(m=capi.Model(path, 0), g=g, t=tensors, o=zvoracle.Oracle(tensors))
    yield _M["m"], _M["g"], _M["t"], _M["o"]


def teardown_module(module):
    for k in ("m", "mw"):
        if k in _M:
            _M[k].close()
    _M.clear()


def _pad_rows(x, mult):
    """zero rows appended up to a multiple of the stage's rate (not gated)"""
    extra = -x.shape[0] % mult
    return np.concatenate([x, np.zeros((extra, x.shape[1]), np.float32)]) if extra else x


def _run_both(m, *args, **kw):
    """the default kernels and the batch kernels on one input (one model: every switch is read at the call; its lane is poisoned in
    between, so that the second run cannot find the first one's values); their bits must be equal"""
    from zerovox_cpp_amd import capi
    got = m.debug_layer(*args, **kw)
    m.poison()
    with capi.switches(**ph.BATCH_REGIME):
        gb = m.debug_layer(*args, **kw)
    assert np.array_equal(got, gb) and np.array_equal(np.signbit(got), np.signbit(gb)), "batch kernels"
    return got, gb


def _banded_case(name, m, o, kind, idx, x, regions, out_cols, rel_gate, **kw):
    got, _ = _run_both(m, kind, idx, x, out_cols, **kw)
    ref, alt, hi = ph.oracle_triple(o, "layer", kind, idx, x, out_cols, **kw)
    ph.region_gates(name, got, ref, alt, hi, regions, rel_gate)
    # the response to the input, with the bias's share cancelled on both sides
    x0 = np.zeros_like(x)
    g0, _ = _run_both(m, kind, idx, x0, out_cols, **kw)
    r0, a0 = ph.oracle_pair(o, "layer", kind, idx, x0, out_cols, **kw)
    # (below 2^-16 a residual block's response is made of f16 re-roundings of its bias-level operands: its floor, not a fixed
    # fraction, is the gate there; the error must stay below the response itself)
    ph.region_gates(name + " f(x)-f(0)", got - g0, ref - r0, alt - a0, None, regions, 1.0,
                    resolution=np.spacing(np.abs(ref)) + np.spacing(np.abs(r0)))


def _crossing_case(name, m, o, kind, idx, x, regions, out_cols, rel_gate, **kw):
    rows = kw.get("out_rows", x.shape[0])
    clean = np.zeros(rows, bool)
    for _, sl in regions:
        clean[sl] = True
    from zerovox_cpp_amd import capi
    got = m.debug_layer(kind, idx, x, out_cols, **kw)
    m.poison()
    with capi.switches(**ph.BATCH_REGIME):
        gb = m.debug_layer(kind, idx, x, out_cols, **kw)
    ref, alt, hi = ph.oracle_triple(o, "layer", kind, idx, x, out_cols, **kw)
    assert not np.isfinite(ref).all(), "the crossing inputs did not reach inf"
    ph.nonfinite_masks_equal(name + " (oracle orders)", alt, ref)
    ph.nonfinite_footprint(name, got, ref, clean)
    ph.nonfinite_footprint(name + " batch kernels", gb, ref, clean)
    d = np.flatnonzero(np.any(got[clean] != gb[clean], axis=tuple(range(1, got.ndim))))
    assert np.array_equal(got[clean], gb[clean]), f"batch kernels: clean rows differ at {np.flatnonzero(clean)[d][:16]}"
    # the finite remainder as one region (a clean stretch alone is a few hundred values: one f16 re-rounding flip decides it)
    ph.region_gates(name, got, ref, alt, hi, [("clean rows", clean)], rel_gate)


@pytest.mark.parametrize("block", RES_BLOCKS)
def test_residual_block_value_ranges(env, block):
    """banded (per band + response), sparse, near-saturation and inf-crossing inputs through one residual block, default and
    batch kernels"""
    m, g, t, o = env
    stage, k = block // 3, g.resblock_kernels[block % 3]
    C, rate = m.voc_channels(stage), m.voc_rate(stage)
    halo = ph.resblock_halo(k, g.resblock_dilations)
    K = m.LAYER_VOC_RESBLOCK
    name = f"resblock {block} (C={C}, k={k})"
    x, reg = ph.banded(1000 + block, C, halo)
    _banded_case(name + " banded", m, o, K, block, _pad_rows(x, rate), reg, C, 1e-3)
    for fam, (x, reg) in (("sparse", ph.sparse(1100 + block, 32 * rate, C)),
                          ("near-saturation", ph.near_saturation(1200 + block, 32 * rate, C))):
        got, _ = _run_both(m, K, block, x, C)
        ref, alt, hi = ph.oracle_triple(o, "layer", K, block, x, C)
        assert np.isfinite(ref).all(), f"{fam}: the oracle's output is not finite"
        if fam == "near-saturation":
            print(f"   largest f16 operand {np.max(np.abs(x)):.0f}, largest output {np.max(np.abs(ref)):.0f}")
        ph.region_gates(f"{name} {fam}", got, ref, alt, hi, reg, 2e-4)
    x, reg = ph.crossing(1300 + block, C, halo, ph.resblock_cross_margin(g.resblock_dilations))
    _crossing_case(name + " crossing", m, o, K, block, _pad_rows(x, rate), reg, C, 2e-4)


@pytest.mark.parametrize("idx", UPSAMPLES)
def test_transposed_conv_value_ranges(env, idx):
    m, g, t, o = env
    cin = g.voc_channels >> idx
    cout, s = cin // 2, g.upsample_scales[idx]
    rate_in = 1 if idx == 0 else m.voc_rate(idx - 1)
    halo = ph.upsample_halo(g.upsample_kernels[idx], s)
    K = m.LAYER_VOC_UPSAMPLE
    name = f"conv_transpose1d {idx} ({cin}->{cout})"
    x, reg = ph.banded(1400 + idx, cin, halo, out_rate=s)
    x = _pad_rows(x, rate_in)
    _banded_case(name + " banded", m, o, K, idx, x, reg, cout, 1e-3, out_rows=x.shape[0] * s)
    x, reg = ph.sparse(1500 + idx, 48 * rate_in, cin)
    got, _ = _run_both(m, K, idx, x, cout, out_rows=x.shape[0] * s)
    ref, alt, hi = ph.oracle_triple(o, "layer", K, idx, x, cout, out_rows=x.shape[0] * s)
    ph.region_gates(name + " sparse", got, ref, alt, hi, reg, 1e-4)
    x, reg = ph.crossing(1600 + idx, cin, halo, 0, out_rate=s)
    x = _pad_rows(x, rate_in)
    _crossing_case(name + " crossing", m, o, K, idx, x, reg, cout, 1e-4, out_rows=x.shape[0] * s)


def test_vocoder_input_conv_mel_offsets(env):
    """(mel - mean) / scale per bin: bins exactly at hifigan.mean (a normalised input of exactly 0), constant bins, bins with
    offsets up to 1e3 sigma; then the k7 input conv"""
    m, g, t, o = env
    M = g.num_mels
    n, reg = ph.offset(1700, 96, M)
    n[:, 0] = 0.0                       # the first constant bin: exactly at the mean
    n[40:56, :] = 0.0                   # a silent stretch: every bin at the mean
    mean, scale = t["hifigan.mean"].astype(np.float32), t["hifigan.scale"].astype(np.float32)
    mel = (mean + 4.0 * scale * n).astype(np.float32)
    mel[:, 0] = mean[0]
    mel[40:56, :] = mean
    got = m.debug_layer(m.LAYER_VOC_INPUT, 0, mel, g.voc_channels)
    ref, alt, hi = ph.oracle_triple(o, "layer", o.LAYER_VOC_INPUT, 0, mel, g.voc_channels)
    ph.region_gates("vocoder input conv, mel offsets", got, ref, alt, hi, [("all", slice(None)), ("silent", slice(43, 53))], 1e-4)


def test_vocoder_output_conv_tanh_saturation(env):
    """pre-tanh magnitudes from ~1e-4 to ~20 (tanh saturated to exactly +-1 in f32) in bands along time"""
    m, g, t, o = env
    C = g.voc_channels >> len(g.upsample_scales)
    x, reg = ph.banded(1800, C, 3, exponents=(-14, -10, -6, -2, 2, 4, 5))
    x = _pad_rows(x, g.hop_size)
    got = m.debug_layer(m.LAYER_VOC_OUTPUT, 0, x, 0)
    ref, alt, hi = ph.oracle_triple(o, "layer", o.LAYER_VOC_OUTPUT, 0, x, 0)
    assert np.sum(np.abs(ref) == 1.0) > 0, "no output saturated"
    ph.region_gates("vocoder output conv + tanh", got, ref, alt, hi, reg, 1e-4)


def _dec_style(E):
    return (0.05 * np.random.default_rng(7).standard_normal(E)).astype(np.float32)


@pytest.mark.parametrize("block", DEC_BLOCKS)
def test_decoder_block_offsets(env, block):
    """per-channel offsets (constant channels, sigma^2 ~ eps and << eps, |mu| / sigma up to 1e3) through a decoder residual
    block, both ways of feeding its convs (ZV_DEC_PREPASS 0 / 1)"""
    from zerovox_cpp_amd import capi
    m, g, t, o = env
    E, R = g.E, g.residual_dim
    cin = [E, 2 * E, 2 * E + R, 2 * E + R, 2 * E + R, E, E][block]
    cout = [2 * E, 2 * E, 2 * E, 2 * E, E, E, E][block]
    style = _dec_style(E)
    for ratio in (None, 1e3):
        x, _ = ph.offset(1900 + block, 96, cin, common_ratio=ratio)
        ref, alt, hi = ph.oracle_triple(o, "layer", o.LAYER_DEC_BLOCK, block, x, cout, style=style)
        outs = []
        for pre in (0, 1):
            with capi.switches(ZV_DEC_PREPASS=pre):
                got = m.debug_layer(m.LAYER_DEC_BLOCK, block, x, cout, style=style)
            ph.region_gates(f"decoder block {block} offsets ratio={ratio} prepass={pre}", got, ref, alt, hi,
                            [("all", slice(None))], 3e-4)
            outs.append(got)
        assert np.array_equal(outs[0], outs[1]), "ZV_DEC_PREPASS 0 and 1 differ"


@pytest.mark.parametrize("idx", ADAINS)
def test_adain_offsets(env, idx):
    """AdaIN1d alone: every channel class gated on its own (the layer keeps channels apart)"""
    m, g, t, o = env
    E, R = g.E, g.residual_dim
    C = ((2 * E, 2 * E, E, E, E) if idx & 1 else (2 * E + R, 2 * E + R, 2 * E + R, E, E))[idx // 2]
    x, reg = ph.offset(2000 + idx, 96, C)
    x[:, 3 * 4] *= 1e3 / np.max(np.abs(x[:, 3 * 4]))       # the first of the rest columns (mu / sigma = 0) at |x| ~ 1e3
    style = _dec_style(E)
    got = m.debug_layer(m.LAYER_DEC_ADAIN, idx, x, C, style=style)
    ref, alt, hi = ph.oracle_triple(o, "layer", o.LAYER_DEC_ADAIN, idx, x, C, style=style)
    ph.region_gates(f"AdaIN {idx} (C={C}) offsets", got, ref, alt, hi, reg, 1e-5, floor_mult=4.0)


def test_asr_res_offsets(env):
    """InstanceNorm(conv1x1(x)): with every channel at |mu| / sigma = 1e3 the conv's output keeps the offset, so the
    statistics of the conv epilogue (tile_stats_store) see it"""
    m, g, t, o = env
    for ratio in (None, 1e3):
        x, _ = ph.offset(2100, 96, g.E, common_ratio=ratio)
        got = m.debug_layer(m.LAYER_DEC_ASR_RES, 0, x, g.residual_dim)
        ref, alt, hi = ph.oracle_triple(o, "layer", o.LAYER_DEC_ASR_RES, 0, x, g.residual_dim)
        ph.region_gates(f"decoder asr_res offsets ratio={ratio}", got, ref, alt, hi, [("all", slice(None))], 1e-3)


def _encoder_cases(m, g, t, o, tag, layer=0):
    """the LayerNorms alone on row families that ARE their input (LAYER_ENC_LN), then the sublayers on attention extremes and on
    the same rows (there the residual x + sublayer(x) is the LayerNorm's input, whose rows are then ordinary: gated whole)"""
    from zerovox_cpp_amd import capi
    kw = dict(heads=g.encoder_head, ksz=g.conv_kernel_size)
    x, reg = ph.ln_rows(2200, 96, g.E)
    ph.ln_rows_reached(x, reg)
    for j, sub in ((0, "slf_attn"), (1, "pos_ffn")):
        got = m.debug_layer(m.LAYER_ENC_LN, 2 * layer + j, x, g.E)
        ref, alt, hi = ph.oracle_triple(o, "layer", o.LAYER_ENC_LN, 2 * layer + j, x, g.E)
        ln = "_pe._enc.laystk.%d.%s.layer_norm." % (layer, sub)
        w, b = t[ln + "w"].astype(np.float64), t[ln + "b"].astype(np.float64)
        ph.ln_scales_reached(f"{tag} {sub} LayerNorm", ref, w, b, reg)
        ph.region_gates(f"{tag} {sub} LayerNorm", got, ref, alt, hi, reg, 1e-5)
        ph.ln_row_scale_gate(f"{tag} {sub} LayerNorm", got, ref, alt, w, b)
    xa, _ = ph.attention_extremes(2300, 96, g.E)
    whole = [("all", slice(None))]
    for kind, ok, nm, inputs in ((m.LAYER_ENC_MHA, o.LAYER_ENC_MHA, "attention sublayer", (x, xa)),
                                 (m.LAYER_ENC_FFN, o.LAYER_ENC_FFN, "feed-forward sublayer", (x,)),
                                 (m.LAYER_ENC_FFT, o.LAYER_ENC_FFT, "FFT block", (x, xa))):
        for xi in inputs:
            ref, alt, hi = ph.oracle_triple(o, "layer", ok, layer, xi, g.E, **kw)
            outs = {}
            for sw in ("ZV_ATT_SCALAR", "ZV_ATT_MFMA"):
                with capi.switches(**{sw: 1}):
                    outs[sw] = m.debug_layer(kind, layer, xi, g.E)
            assert np.array_equal(outs["ZV_ATT_SCALAR"], outs["ZV_ATT_MFMA"]), nm
            what = "row-family input" if xi is x else "logits >> 88, tied keys"
            ph.region_gates(f"{tag} {nm} {what}", outs["ZV_ATT_SCALAR"], ref, alt, hi, whole, 1e-4)
    ref, alt, hi = ph.oracle_triple(o, "layer", o.LAYER_VAR_PRED, 0, x, 0, ksz=(g.vp_kernel_size,))
    got = m.debug_layer(m.LAYER_VAR_PRED, 0, x, 0)
    ph.region_gates(f"{tag} variance predictor 0 row-family input", got, ref, alt, hi, whole, 1e-4)


def test_encoder_layernorm_rows_and_attention_extremes(env):
    """LayerNorm alone on constant rows, rows offset up to 1e3 sigma and rows of variance <= 2 eps (add_layernorm_kernel's
    register path, E = 528); attention with logits far above 88 (exp overflows without the max subtraction) and keys tied
    exactly in groups of 4; both attention kernels, bit-equal"""
    m, g, t, o = env
    _encoder_cases(m, g, t, o, "medium")


def test_encoder_layernorm_above_768_channels(ckpt):
    """E = 1024 (synth MEDIUM_E1024): the same cases on add_layernorm_kernel's path for rows wider than 64 x LN_MAXE = 768
    channels"""
    from zerovox_cpp_amd import capi
    from oracle import zvoracle
    path, g, tensors = ckpt("medium_e1024")
    assert g.E > 768
    if "mw" not in _M:
        _M["mw"] = capi.Model(path, 0)
    _encoder_cases(_M["mw"], g, tensors, zvoracle.Oracle(tensors), f"E={g.E}")


def test_stages_at_value_ranges_vs_reference(ckpt):
    """zv_decode / zv_vocode on the stage inputs of tests/golden/value_ranges_small.npz, gated per region on the fixture's floors
    (1.5 x rms and max, as the other stage gates; and rms within 1e-3 of the region's signal); the oracle they are compared with reproduces the
    reference's SHA-256 here too"""
    import hashlib
    import os
    from zerovox_cpp_amd import capi
    from oracle import zvoracle
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "value_ranges_small.npz"))
    path, g, tensors = ckpt(str(z["geometry"]), int(z["seed_w"]))
    hid, style, mel_in, dreg, vreg = ph.value_range_stage_inputs(g, tensors)
    orc = zvoracle.Oracle(tensors)
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    mel_ref, wav_ref = orc.decoder(hid, style), orc.vocoder(mel_in)
    assert sha(mel_ref) == str(z["mel_sha256"]) and sha(wav_ref) == str(z["wav_sha256"])
    m = capi.Model(path, 0)
    try:
        mel, wav = m.decode(hid, style), m.vocode(mel_in)
    finally:
        m.close()
    for stage, got, ref, regs in (("mel", mel, mel_ref, dreg), ("wav", wav, wav_ref, vreg)):
        assert np.isfinite(got).all(), stage
        for (lbl, idx), f, fm, sig in zip(regs, z[stage + "_floor_rms"], z[stage + "_floor_max"], z[stage + "_rms"]):
            d = got[idx].astype(np.float64) - ref[idx]
            e, mx = float(np.sqrt(np.mean(d ** 2))), float(np.max(np.abs(d)))
            print(f"{stage} [{lbl}]: rms err {e:.3e} (floor {f:.3e}), max {mx:.3e} (floor {fm:.3e})")
            assert e <= 1.5 * f and mx <= 1.5 * fm and e <= 1e-3 * sig, f"{stage} [{lbl}]"
