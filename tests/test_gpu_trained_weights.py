"""GPU: every layer and every same-bits promise on the "trained" weight family (synth.make_tensors family="trained": heavy-tailed
f16 conv weights whose channel gains spread over octaves, with exact zeros of both signs, f16 subnormals, pruned channels and a few
outliers; norm gains in [-1.5, 3] with an exact 0 and negatives; biases up to +-1).  Every other parity test and every same-bits
assertion runs on weights uniform in +-sqrt(3 / fan-in); here one chain adds products that span 2^16 and more, which is where two
matrix-core instruction shapes, or two tilings of one conv, could round differently (tests/test_gpu_mfma_chain.py holds the
instruction-level half of this).

One medium checkpoint of the family, one model, one oracle.  Per layer: zv_debug_layer against the oracle's layer through
parity_helpers.layer_gate — error <= max(2 x the oracle's own reorder noise, 3e-7) and <= the relative gate the layer has in
tests/test_gpu_layers.py — in the default regime and, the lane poisoned in between, under BATCH_REGIME, whose bits must be the
default's; a column the oracle leaves exactly constant (a pruned output channel under a bias, a norm gain of 0) must be constant on
the GPU.  Whole stages: bits only."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED_W = 5150
_M = {}


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    from zerovox_cpp_amd import capi, gguf, synth
    from oracle import zvoracle
    if "m" not in _M:
        g = synth.MEDIUM
        path = str(tmp_path_factory.mktemp("trained") / "medium_trained.gguf")
        synth.write_checkpoint(path, g, SEED_W, family="trained")
        _, tensors = gguf.read_gguf(path)
        _M.update(m=capi.Model(path, 0), g=g, t=tensors, o=zvoracle.Oracle(tensors))
    return _M["m"], _M["g"], _M["t"], _M["o"]


def teardown_module(module):
    if "m" in _M:
        _M["m"].set_graph_mode(False)
        _M["m"].close()
    _M.clear()


def _first_row(a, b):
    """first row (index along axis 0) at which two arrays differ in bits, and how many elements do"""
    ne = np.ascontiguousarray(a, np.float32).view(np.uint32) != np.ascontiguousarray(b, np.float32).view(np.uint32)
    rows = np.flatnonzero(ne.reshape(ne.shape[0], -1).any(axis=1)) if ne.ndim else np.flatnonzero(ne)
    return (int(rows[0]) if len(rows) else -1), int(ne.sum())


def _same_bits(got, want, what):
    assert got.shape == want.shape, what
    row, n = _first_row(got, want)
    assert n == 0, f"{what}: {n} of {got.size} elements differ, first in row {row}"


def _constant_columns(name, got, ref):
    """where a column of the oracle's output is exactly constant, the GPU's is"""
    if ref.ndim != 2 or ref.shape[0] < 2:
        return
    const = np.flatnonzero(np.all(ref == ref[:1], axis=0))
    for c in const:
        assert np.all(got[:, c] == got[0, c]), f"{name}: column {c} is constant ({ref[0, c]!r}) in the oracle, not on the GPU"
    if len(const):
        print(f"{name:28s} {len(const)} exactly constant column(s) in the oracle {list(const[:6])}: constant on the GPU too")


def _layer(env, name, kind, index, x, out_cols, rel_gate, style=None, out_rows=None, okw=None, regimes=(),
           batch=True):
    """one layer: default regime vs the oracle; `regimes` ((label, switches)) vs the oracle and the default's bits; then, the lane
    poisoned, BATCH_REGIME vs the oracle and the default's bits.  layer_gate at its default floor: 2 x the oracle's own reorder noise"""
    from zerovox_cpp_amd import capi
    from parity_helpers import BATCH_REGIME, layer_gate, oracle_pair
    m, g, t, o = env
    gkw = dict(style=style, out_rows=out_rows)
    okw = dict(okw or {})
    if style is not None:
        okw["style"] = style
    if out_rows is not None:
        okw["out_rows"] = out_rows
    ref, alt = oracle_pair(o, "layer", getattr(o, kind), index, x, out_cols, **okw)
    assert np.isfinite(ref).all() and np.isfinite(alt).all(), f"{name}: the oracle is not finite"
    got = m.debug_layer(getattr(m, kind), index, x, out_cols, **gkw)
    layer_gate(name, got, ref, alt, rel_gate)
    _constant_columns(name, got, ref)
    for label, sw in regimes:
        with capi.switches(**sw):
            r = m.debug_layer(getattr(m, kind), index, x, out_cols, **gkw)
        layer_gate(f"{name} {label}", r, ref, alt, rel_gate)
        _same_bits(r, got, f"{name}: {label} vs the default regime")
    if batch:
        m.poison()
        with capi.switches(**BATCH_REGIME):
            r = m.debug_layer(getattr(m, kind), index, x, out_cols, **gkw)
        layer_gate(f"{name} batch kernels", r, ref, alt, rel_gate)
        _same_bits(r, got, f"{name}: BATCH_REGIME vs the default regime")
    return got


def _rate(g, stage):
    return int(np.prod(g.upsample_scales[:stage + 1]))


SPARSE_BLOCKS = (0, 4, 8, 9)        # one residual block per stage (3, 7, 11 and 3 taps) also on parity_helpers.sparse


@pytest.mark.parametrize("block", list(range(12)))
def test_every_hifigan_residual_block(env, block):
    """32 frames at the stage's rate (stage 3: 9 600 rows, enough for the 512-row tiles of ZV_TRIPLE_V2 = 3)"""
    import parity_helpers as ph
    m, g, t, o = env
    stage = block // 3
    C, rows = g.voc_channels >> (stage + 1), 32 * _rate(g, stage)
    x = (0.5 * np.random.default_rng(100 + block).standard_normal((rows, C))).astype(np.float32)
    _layer(env, f"hifigan block {block} (C={C})", "LAYER_VOC_RESBLOCK", block, x, C, 2e-4)
    if block in SPARSE_BLOCKS:
        xs, _ = ph.sparse(1100 + block, rows, C)
        _layer(env, f"hifigan block {block} sparse", "LAYER_VOC_RESBLOCK", block, xs, C, 2e-4)


@pytest.mark.parametrize("idx", [0, 1, 2, 3])
def test_every_transposed_conv(env, idx):
    m, g, t, o = env
    cin = g.voc_channels >> idx
    cout, s = cin // 2, g.upsample_scales[idx]
    rows = 48 * (1 if idx == 0 else _rate(g, idx - 1))
    x = (0.7 * np.random.default_rng(400 + idx).standard_normal((rows, cin))).astype(np.float32)
    _layer(env, f"conv_transpose1d {idx} ({cin}->{cout}, x{s})", "LAYER_VOC_UPSAMPLE", idx, x, cout, 1e-4, out_rows=rows * s)


def test_vocoder_input_and_output_conv(env):
    from zerovox_cpp_amd import synth
    m, g, t, o = env
    _layer(env, "vocoder input conv", "LAYER_VOC_INPUT", 0, synth.vocoder_mel(g, t, 41, 96), g.voc_channels, 1e-4)
    C = g.voc_channels >> len(g.upsample_scales)
    x = (0.6 * np.random.default_rng(43).standard_normal((16 * g.hop_size, C))).astype(np.float32)
    _layer(env, "vocoder output conv + tanh", "LAYER_VOC_OUTPUT", 0, x, 0, 1e-4)


DEC_REGIMES = (("prepass=0", {"ZV_DEC_PREPASS": 0}), ("prepass=1", {"ZV_DEC_PREPASS": 1}),
               ("prepass=1 conv_gemm", {"ZV_DEC_PREPASS": 1, "ZV_CONV_GEMM": 2}))


@pytest.mark.parametrize("block", list(range(7)))
def test_every_decoder_residual_block(env, block):
    import parity_helpers as ph
    m, g, t, o = env
    E, R = g.E, g.residual_dim
    cin = [E, 2 * E, 2 * E + R, 2 * E + R, 2 * E + R, E, E][block]
    cout = [2 * E, 2 * E, 2 * E, 2 * E, E, E, E][block]
    x = (1.2 * np.random.default_rng(300 + block).standard_normal((96, cin))).astype(np.float32)
    style = (0.05 * np.random.default_rng(7).standard_normal(E)).astype(np.float32)
    _layer(env, f"decoder block {block} ({cin}->{cout})", "LAYER_DEC_BLOCK", block, x, cout, 3e-4, style=style, regimes=DEC_REGIMES)
    if block == 3:
        xs, _ = ph.sparse(1300 + block, 96, cin)
        _layer(env, f"decoder block {block} sparse", "LAYER_DEC_BLOCK", block, xs, cout, 3e-4, style=style, regimes=DEC_REGIMES)


@pytest.mark.parametrize("idx", list(range(10)))
def test_every_adain(env, idx):
    m, g, t, o = env
    E, R = g.E, g.residual_dim
    cin, cout = [2 * E + R, 2 * E + R, 2 * E + R, E, E], [2 * E, 2 * E, E, E, E]
    C = (cout if idx & 1 else cin)[idx // 2]
    x = (1.2 * np.random.default_rng(600 + idx).standard_normal((96, C)) + 0.3).astype(np.float32)
    style = (0.05 * np.random.default_rng(8).standard_normal(E)).astype(np.float32)
    _layer(env, f"AdaIN decode.{idx // 2}.norm{1 + (idx & 1)} (C={C})", "LAYER_DEC_ADAIN", idx, x, C, 1e-5, style=style)


def test_decoder_asr_res_and_to_out(env):
    m, g, t, o = env
    x = (1.1 * np.random.default_rng(44).standard_normal((96, g.E))).astype(np.float32)
    _layer(env, "decoder asr_res", "LAYER_DEC_ASR_RES", 0, x, g.residual_dim, 1e-4)
    _layer(env, "decoder to_out", "LAYER_DEC_TO_OUT", 0, x, g.num_mels, 1e-4)


ATT = (("ZV_ATT_SCALAR", {"ZV_ATT_SCALAR": 1}), ("ZV_ATT_MFMA", {"ZV_ATT_MFMA": 1}))


@pytest.mark.parametrize("layer", [0, 1, 2, 3])
def test_every_encoder_fft_block(env, layer):
    """the whole block, the attention sublayer with both attention kernels, the feed-forward sublayer, 96 tokens"""
    m, g, t, o = env
    okw = dict(heads=g.encoder_head, ksz=g.conv_kernel_size)
    x = np.random.default_rng(200 + layer).standard_normal((96, g.E)).astype(np.float32)
    _layer(env, f"encoder FFT block {layer}", "LAYER_ENC_FFT", layer, x, g.E, 1e-4, okw=okw, regimes=ATT)
    x = np.random.default_rng(500 + layer).standard_normal((96, g.E)).astype(np.float32)
    _layer(env, f"attention sublayer {layer}", "LAYER_ENC_MHA", layer, x, g.E, 1e-4, okw=okw, regimes=ATT)
    _layer(env, f"feed-forward sublayer {layer}", "LAYER_ENC_FFN", layer, x, g.E, 1e-4, okw=okw)


@pytest.mark.parametrize("idx", list(range(8)))
def test_every_encoder_layernorm(env, idx):
    """LAYER_ENC_LN: gains in [-1.5, 3]; the column whose gain is exactly 0 is the bias itself"""
    m, g, t, o = env
    x = (1.5 * np.random.default_rng(700 + idx).standard_normal((96, g.E)) + 0.2).astype(np.float32)
    sub = "slf_attn" if idx % 2 == 0 else "pos_ffn"
    w = t[f"_pe._enc.laystk.{idx // 2}.{sub}.layer_norm.w"]
    assert (w == 0).any() and (w < 0).any()
    got = _layer(env, f"encoder LayerNorm {idx}", "LAYER_ENC_LN", idx, x, g.E, 1e-5)
    b = t[f"_pe._enc.laystk.{idx // 2}.{sub}.layer_norm.b"]
    z = np.flatnonzero(w == 0)
    assert np.array_equal(got[:, z], np.broadcast_to(b[z], got[:, z].shape)), "a gain of exactly 0 leaves the bias"


@pytest.mark.parametrize("p", [0, 1, 2])
def test_every_variance_predictor(env, p):
    m, g, t, o = env
    x = np.random.default_rng(400 + p).standard_normal((80, g.E)).astype(np.float32)
    _layer(env, f"variance predictor {p}", "LAYER_VAR_PRED", p, x, 0, 1e-4, okw=dict(ksz=(g.vp_kernel_size,)))


# ---- whole stages: bits only ------------------------------------------------------------------------------------------------

def test_vocoder_regimes_give_the_same_bits(env):
    """every entry of parity_helpers.VOCODER_REGIMES on a 64-frame mel: the default's bits (the regimes mix kernels on
    v_mfma_f32_32x32x16_f16 with kernels on v_mfma_f32_16x16x32_f16)"""
    from zerovox_cpp_amd import capi, synth
    from parity_helpers import VOCODER_REGIMES
    m, g, t, o = env
    mel = synth.vocoder_mel(g, t, 51, 64)
    want = m.vocode(mel)
    assert np.isfinite(want).all() and float(np.max(np.abs(want))) < 1.0
    bad = []
    for name, sw in VOCODER_REGIMES:
        m.poison()
        with capi.switches(**{k: int(v) for k, v in sw.items()}):
            got = m.vocode(mel)
        row, n = _first_row(got.reshape(-1, g.hop_size), want.reshape(-1, g.hop_size))
        if n:
            bad.append(f"{name}: {n} samples differ, first in frame {row}")
    assert not bad, "\n".join(bad)


ENC_TAPS = ("logdur", "pitch", "energy", "pitch_bucket", "energy_bucket", "features", "hidden")


def test_decoder_and_encoder_regimes_give_the_same_bits(env):
    """decode 96 frames and encode 24 tokens under every regime of the conv, attention, linear and LayerNorm launches"""
    from zerovox_cpp_amd import capi, synth
    from test_gpu_encdec_geometries import REGIMES as ENCDEC_REGIMES
    m, g, t, o = env
    N, T = 24, 96
    hid = synth.decoder_hidden(g, 77, T)
    ids, puncts, style = synth.encoder_inputs(g, 78, N)
    mel0, e0 = m.decode(hid, style), m.encode(ids, puncts, style, T)
    assert np.isfinite(mel0).all() and 0 < e0["n_frames"] <= T
    bad = []
    for name, sw in ENCDEC_REGIMES:
        m.poison()
        with capi.switches(**sw):
            mel, e = m.decode(hid, style), m.encode(ids, puncts, style, T)
        row, n = _first_row(mel, mel0)
        if n:
            bad.append(f"{name}: decode, {n} values differ, first in frame {row}")
        if e["n_frames"] != e0["n_frames"]:
            bad.append(f"{name}: encode, {e['n_frames']} frames vs {e0['n_frames']}")
        for k in ENC_TAPS:
            if not np.array_equal(e[k], e0[k]):
                bad.append(f"{name}: encode tap {k}, first differing row {_first_row(e[k].astype(np.float32), e0[k].astype(np.float32))[0]}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("chunk", [16, 50])
def test_streamed_vocoding_equals_whole(env, chunk):
    from zerovox_cpp_amd import synth
    m, g, t, o = env
    T = 100
    mel = synth.vocoder_mel(g, t, 52, T)
    whole = m.vocode(mel)
    m.poison()
    pieces = m.vocode_stream(mel, chunk)
    assert [f for f, _ in pieces] == [i * chunk * g.hop_size for i in range(-(-T // chunk))]
    got = np.concatenate([w for _, w in pieces])
    assert got.shape == whole.shape
    row, n = _first_row(got.reshape(-1, g.hop_size), whole.reshape(-1, g.hop_size))
    assert n == 0, f"zv_vocode_stream in chunks of {chunk} vs zv_vocode: {n} samples differ, first in frame {row}"


def _padded(g):
    """three utterances whose capacity T is far above what their durations fill"""
    from zerovox_cpp_amd import synth
    return [(*synth.encoder_inputs(g, 8100 + i, N), T) for i, (N, T) in enumerate(((12, 160), (20, 256), (5, 96)))]


def test_run_shortening_and_packing_change_no_bit(env):
    """ZV_VOC_RUNS and ZV_DEC_RUNS 2 vs 0 and ZV_DEC_PACK 1 vs 0 on padded utterances, alone and in a batch (the batch kernels on)"""
    from zerovox_cpp_amd import capi
    m, g, t, o = env
    utts = _padded(g)
    base = dict(ZV_CONV_GEMM=2, ZV_DEC_PREPASS=1)
    with capi.switches(ZV_VOC_RUNS=0, ZV_DEC_RUNS=0, ZV_DEC_PACK=0, **base):
        want = m.synthesize_batch(utts)
        alone = [m.synthesize(*u) for u in utts]
    assert all(0 < nf < u[3] for (w, nf), u in zip(want, utts)), "an utterance is not padded"
    arms = (("ZV_VOC_RUNS=2", dict(ZV_VOC_RUNS=2, ZV_DEC_RUNS=0, ZV_DEC_PACK=0)),
            ("ZV_DEC_RUNS=2", dict(ZV_VOC_RUNS=0, ZV_DEC_RUNS=2, ZV_DEC_PACK=0)),
            ("ZV_DEC_RUNS=2 ZV_DEC_PACK=1", dict(ZV_VOC_RUNS=0, ZV_DEC_RUNS=2, ZV_DEC_PACK=1)),
            ("ZV_VOC_RUNS=2 ZV_DEC_RUNS=2 ZV_DEC_PACK=1", dict(ZV_VOC_RUNS=2, ZV_DEC_RUNS=2, ZV_DEC_PACK=1)),
            ("ZV_VOC_RUNS=2 ZV_DEC_RUNS=2 ZV_DEC_PACK=0", dict(ZV_VOC_RUNS=2, ZV_DEC_RUNS=2, ZV_DEC_PACK=0)))
    bad = []
    for name, sw in arms:
        m.poison()
        with capi.switches(**sw, **base):
            got = m.synthesize_batch(utts)
            got1 = [m.synthesize(*u) for u in utts]
        for what, res, ref in (("batch", got, want), ("alone", got1, alone)):
            for i, ((w, nf), (wr, nfr)) in enumerate(zip(res, ref)):
                row, n = _first_row(w.reshape(-1, g.hop_size), wr.reshape(-1, g.hop_size))
                if nf != nfr or n:
                    bad.append(f"{name} {what} utterance {i}: frames {nf} vs {nfr}, {n} samples differ, first in frame {row}")
    for i, ((w, nf), (wr, nfr)) in enumerate(zip(want, alone)):
        _same_bits(w, wr, f"runs off: batch vs alone, utterance {i}")
    assert not bad, "\n".join(bad)


RAGGED = ((5, 11), (33, 96), (16, 64), (1, 55), (40, 130))


def test_ragged_batch_equals_standalone(env):
    """five ragged utterances: eager, captured, replayed on a lane poisoned with 0xFF, and fitted (T a capacity: the live samples
    are those of the stand-alone call at T = n_frames, zeros behind them)"""
    from zerovox_cpp_amd import synth
    m, g, t, o = env
    hop = g.hop_size
    utts = [(*synth.encoder_inputs(g, 9000 + 13 * i + N, N), T) for i, (N, T) in enumerate(RAGGED)]
    alone = [m.synthesize(*u) for u in utts]
    assert all(np.isfinite(w).all() and 0 < nf <= u[3] for (w, nf), u in zip(alone, utts))
    runs = {"eager": m.synthesize_batch(utts)}
    m.set_graph_mode(True)
    try:
        bc = m.prepare_batch(utts)
        bc.run()
        runs["captured"] = [(w.copy(), nf) for w, nf in bc.results()]
        for w in bc.wavs:
            w[:] = np.nan
        m.poison(0xFF)
        bc.run()
        runs["replayed on a poisoned lane"] = [(w.copy(), nf) for w, nf in bc.results()]
    finally:
        m.set_graph_mode(False)
    bad = []
    for name, res in runs.items():
        for i, ((w, nf), (wr, nfr)) in enumerate(zip(res, alone)):
            row, n = _first_row(w.reshape(-1, hop), wr.reshape(-1, hop))
            if nf != nfr or n:
                bad.append(f"{name} utterance {i} {RAGGED[i]}: frames {nf} vs {nfr}, {n} samples differ, first in frame {row}")
    m.poison(0xFF)
    for i, ((w, nf), u) in enumerate(zip(m.synthesize_batch(utts, fitted=True), utts)):
        ids, puncts, style, T = u
        wr, nfr = m.synthesize(ids, puncts, style, nf)
        row, n = _first_row(w[:nf * hop].reshape(-1, hop), wr.reshape(-1, hop)) if nfr == nf else (-1, -1)
        if nf != alone[i][1] or nfr != nf or n or w[nf * hop:].any() or w.shape != (T * hop,):
            bad.append(f"fitted utterance {i} {RAGGED[i]}: frames {nf} (unfitted at T = n_frames: {nfr}, padded: {alone[i][1]}), "
                       f"{n} live samples differ, first in frame {row}; tail zero: {not w[nf * hop:].any()}")
    assert not bad, "\n".join(bad)
