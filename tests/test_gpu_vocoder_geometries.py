"""-m gpu: the vocoder on checkpoints whose residual-block convs have other tap counts than 3 / 7 / 11 (synth.RESBLOCK_GEOMETRIES).

The checkpoint format stores one tensor per conv and the reference reads every conv's K from its shape (src/hifigan.cpp:125,164);
so does the loader, which packs fused weights per pair where both convs share a K that pair_supported takes.  Per geometry
(stages of 256, 128, 64 and 32 channels):
  * medium_rb357 (3 / 5 / 7): 5 taps are not pair-fusable at 32 channels, 3 and 7 are — that stage runs unfused as a whole;
    5 taps on resblock_pair64 / resblock_block64 at 64 channels;
  * medium_rb_wide (15 / 9 / 1): 15-tap pair kernels at 256 and 128 channels (14 halo rows: TMmin and LDS sizing with MT = 2,
    3 and 4), no whole-block kernel at 32 channels (triple_supported), a 1-tap conv fusable at 128 / 256 channels only;
  * medium_rb_dilk: the 11-tap branch's last dilation pair has 7 taps — no whole-block / block64 launch may run it with one K;
  * medium_rb_c1c2: convs1 / convs2 of 7 / 3 and 11 / 13 taps in one pair (never fused), a convs2 wider than every convs1;
  * medium_rb_c2wide: every convs2 of the 11-tap branch has 25 taps (never fused): a receptive radius of 25 frames, which a halo
    that left out convs2 (23) would not cover.
Not reached by any geometry: the one-K guard on the block64 path (two pairs of different K at dilations 0 and 1 of a 64-channel
branch).  A checkpoint that reaches it safely on a library without the guard would need dilation 1 wider than dilation 0 in every
stage, with the 32-channel whole-block kernel kept off; the guard is plain host arithmetic (csrc/voc_plan.h) and
tests/test_voc_plan_cpu.py checks it there.
Checked: every residual block alone against the oracle (default and batch kernels, same bits), the whole vocoder against the
oracle, every kernel regime's bits, the halo against the exact receptive radius with bit-exact streaming, and ragged batches
(eager, graph capture, replay) against stand-alone calls.  Also: the loader refuses what the reference would run differently."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WAV_RMS_GATE = 1e-4                 # tests/test_gpu_vocoder.py
ZV_ERR_SHAPE = 4


def _geoms():
    from zerovox_cpp_amd import synth
    return synth.RESBLOCK_GEOMETRIES


_M = {}


def _model(ckpt, gname):
    """one model per geometry: it serves every regime (every switch is read at the call)"""
    from zerovox_cpp_amd import capi
    if gname not in _M:
        _M[gname] = capi.Model(ckpt(gname)[0], 0)
    return _M[gname]


def _close(gname=None):
    for k in [k for k in _M if gname is None or k == gname]:
        _M.pop(k).close()


def teardown_module(module):
    _close()


def _rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))


@pytest.mark.parametrize("gname", _geoms())
def test_every_residual_block(ckpt, gname):
    """all 12 residual blocks through zv_debug_layer against the oracle (32 frames at the stage's rate), under the default switches and
    once more, the lane poisoned in between, under BATCH_REGIME (resblock_pair<256> on 96-row tiles, pair64's weight ring, block64
    at every tap count, the whole-block kernel's 512-row tiles), which must give the default's bits"""
    from zerovox_cpp_amd import capi
    from oracle import zvoracle
    from parity_helpers import BATCH_REGIME, layer_gate, oracle_pair
    _, g, tensors = ckpt(gname)
    m = _model(ckpt, gname)
    o = zvoracle.Oracle(tensors)
    for block in range(12):
        stage = block // 3
        C, rate = m.voc_channels(stage), m.voc_rate(stage)
        x = (0.5 * np.random.default_rng(100 + block).standard_normal((32 * rate, C))).astype(np.float32)
        got = m.debug_layer(m.LAYER_VOC_RESBLOCK, block, x, C)
        m.poison()
        with capi.switches(**BATCH_REGIME):
            gotb = m.debug_layer(m.LAYER_VOC_RESBLOCK, block, x, C)
        ref, alt = oracle_pair(o, "layer", o.LAYER_VOC_RESBLOCK, block, x, C)
        ks = [(g.resblock_k(block % 3, d, 1), g.resblock_k(block % 3, d, 2)) for d in range(3)]
        layer_gate(f"{gname} block {block} (C={C}, K={ks})", got, ref, alt, 2e-4)
        assert np.array_equal(gotb, got), (gname, block)


@pytest.mark.parametrize("gname", _geoms())
def test_vocoder_matches_oracle(ckpt, gname):
    """the whole vocoder against the oracle at 1, 37 and 384 frames: waveform RMS error <= 1e-4"""
    from zerovox_cpp_amd import synth
    from oracle import zvoracle
    _, g, tensors = ckpt(gname)
    m = _model(ckpt, gname)
    o = zvoracle.Oracle(tensors)
    for T in (1, 37, 384):
        mel = synth.vocoder_mel(g, tensors, 7, T)
        wav, ref = m.vocode(mel), o.vocoder(mel)
        assert wav.shape == ref.shape == (T * g.hop_size,) and np.isfinite(wav).all()
        err = _rms(wav - ref)
        print(f"{gname} T={T}: wav rms err {err:.3e}, signal rms {_rms(ref):.3f}")
        assert err <= WAV_RMS_GATE, (gname, T)


def _regimes():
    from parity_helpers import VOCODER_REGIMES
    return list(VOCODER_REGIMES) + [("block64_0", {"ZV_BLOCK64": 0}), ("block64_-3", {"ZV_BLOCK64": -3}),
                                    ("block64_-11", {"ZV_BLOCK64": -11})]


@pytest.mark.parametrize("gname", _geoms())
def test_kernel_regimes_give_the_same_bits(ckpt, gname):
    """every entry of VOCODER_REGIMES and ZV_BLOCK64 = 0 / -3 / -11 at 384 frames: the default's bits (as
    tests/test_gpu_full_size.py::test_kernel_regimes_give_the_same_bits).  One model, the switches set around each call and the lane
    poisoned before it: a stage with an unfusable pair runs unfused in every regime, a branch whose K changes over its dilations
    never runs on the whole-block / block64 kernels"""
    from zerovox_cpp_amd import capi, synth
    _, g, tensors = ckpt(gname)
    mel = synth.vocoder_mel(g, tensors, 51, 384)
    m = _model(ckpt, gname)
    want = m.vocode(mel)
    for name, env in _regimes():
        m.poison()
        with capi.switches(**{k: int(v) for k, v in env.items()}):
            got = m.vocode(mel)
        assert np.array_equal(got, want), (gname, name)


@pytest.mark.parametrize("gname", _geoms())
def test_halo_covers_every_conv_and_streaming_is_bit_exact(ckpt, gname):
    """zv_vocoder_halo_frames() against the exact receptive radius: at least the radius, at most 4 frames more — the halo sums
    fractional frames per layer (each upsample's whole 3-row polyphase window: 3.75 frames over the 4 stages, where the exact walk
    reaches at most 2.25 and rounds down), rounds up and adds a spare frame (medium: 23 against 20; the 11-tap branch's
    dilation pair of 7 taps in medium_rb_dilk takes it from 23 to 20, against 17).  medium_rb_c2wide reaches 25 frames: a halo
    that counted only the convs1 of dilation 0 (23) would be too small there, and streaming inexact.  And zv_vocode_stream with
    64-, 100- and 511-frame chunks gives zv_vocode's bits at 512 frames"""
    from zerovox_cpp_amd import synth
    from parity_helpers import receptive_radius
    _, g, tensors = ckpt(gname)
    m = _model(ckpt, gname)
    r = receptive_radius(g, tensors)
    H = m.vocoder_halo_frames()
    print(f"{gname}: receptive radius {r} frames, halo {H}")
    assert r <= H <= r + 4, (r, H)
    T = 512
    mel = synth.vocoder_mel(g, tensors, 52, T)
    full = m.vocode(mel)
    for chunk in (64, 100, 511):
        chunks = m.vocode_stream(mel, chunk)
        assert [c[0] for c in chunks] == [a * g.hop_size for a in range(0, T, chunk)]
        got = np.concatenate([c[1] for c in chunks])
        assert got.shape == full.shape and np.array_equal(got, full), (gname, chunk)


# (N, T) per utterance: T from 1 to 1 500, one utterance with more than 1 024 frames
BATCH = [(1, 1), (3, 7), (40, 100), (90, 333), (400, 1100), (120, 1500)]


@pytest.mark.parametrize("gname", _geoms())
def test_ragged_batch_equals_standalone(ckpt, gname):
    """zv_synthesize_batch of 6 utterances (T 1 .. 1 500, one over 1 024 frames: block64, the merged MRF sum and the fused
    256-channel stage engage by length): eager, graph capture and graph replay each give every utterance's stand-alone bits"""
    from zerovox_cpp_amd import synth
    _, g, tensors = ckpt(gname)
    m = _model(ckpt, gname)
    utts = [(*synth.encoder_inputs(g, 7000 + 13 * i + N, N), T) for i, (N, T) in enumerate(BATCH)]
    got = m.synthesize_batch(utts)
    m.set_graph_mode(True)
    try:
        got_c = m.synthesize_batch(utts)          # capture
        got_r = m.synthesize_batch(utts)          # replay
    finally:
        m.set_graph_mode(False)
    assert max(nf for _, nf in got) >= 1024
    for i, ((ids, puncts, style, T), (w, nf), (wc, nfc), (wr, nfr)) in enumerate(zip(utts, got, got_c, got_r)):
        ref, nf_ref = m.synthesize(ids, puncts, style, T)
        assert nf == nfc == nfr == nf_ref and 0 < nf <= T and np.isfinite(w).all(), (gname, i)
        assert np.array_equal(w, ref) and np.array_equal(wc, ref) and np.array_equal(wr, ref), (gname, i)
    _close(gname)


@pytest.mark.parametrize("gname,tensor", [("medium_up4553", "_meldec.upsamples.0.1.w"), ("medium_vock5", "_meldec.input_conv.w")])
def test_loader_refuses_what_the_reference_runs_differently(ckpt, gname, tensor):
    """the reference hard-codes 4 upsample stages of strides 5, 5, 4, 3 (src/zerovox.cpp:127-129) and pads the input and output
    convs for 7 taps (src/hifigan.cpp:261,338): a file with strides 4, 5, 5, 3 (kernels 8, 10, 10, 6: still a hop of 300) or with
    5-tap input / output convs is refused at load with ZV_ERR_SHAPE naming the tensor"""
    from zerovox_cpp_amd import capi
    path, g, _ = ckpt(gname)
    with pytest.raises(capi.ZvError) as ei:
        capi.Model(path, 0)
    print(ei.value)
    assert ei.value.status == ZV_ERR_SHAPE and tensor in str(ei.value)


@pytest.mark.parametrize("case,tensor", [("output_conv_k5", "_meldec.output_conv.1.w"), ("3_stages", "_meldec.upsamples.3.1.w"),
                                         ("5_stages", "_meldec.upsamples.4.1.w")])
def test_loader_refuses_other_output_convs_and_stage_counts(tmp_path, case, tensor):
    """the checks the two geometries above do not reach: a 5-tap output conv behind a 7-tap input conv, and 3 or 5 upsample stages
    instead of the reference's 4 (synth.TINY's tensors, edited): ZV_ERR_SHAPE naming the tensor"""
    from zerovox_cpp_amd import capi, gguf, synth
    g = synth.TINY
    tensors = synth.make_tensors(g, 7)
    if case == "output_conv_k5":
        tensors = [(n, a[:, :, 1:6].copy() if n == tensor else a) for n, a in tensors]
    elif case == "3_stages":
        tensors = [(n, a) for n, a in tensors if not n.startswith("_meldec.upsamples.3.")]
    else:
        up3 = dict(tensors)
        tensors = tensors + [(tensor, up3["_meldec.upsamples.3.1.w"]), ("_meldec.upsamples.4.1.b", up3["_meldec.upsamples.3.1.b"])]
    path = str(tmp_path / f"{case}.gguf")
    gguf.write_gguf(path, g.kv(), tensors, arch=synth.ARCH)
    with pytest.raises(capi.ZvError) as ei:
        capi.Model(path, 0)
    print(ei.value)
    assert ei.value.status == ZV_ERR_SHAPE and tensor in str(ei.value)
