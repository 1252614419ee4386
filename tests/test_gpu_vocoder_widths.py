"""-m gpu: the vocoder at other channel widths than 512, 128 and 48 (synth.VOC_WIDTH_GEOMETRIES: 256, 496, 768, 1 024).

The schedule picks a stage's kernels by its padded channel count (csrc/voc_plan.h, csrc/conv_plan.h), the loader takes the width from
`_meldec.input_conv.w`; medium, small and tiny put every specialised kernel at one fixed place.  Per width (stages at 5 / 25 / 100 /
300 rows per frame; tests/native/voc_plan_check.cpp pins the plan of each):
  * small_v256 (128 / 64 / 32 / 16): resblock_pair_kernel<128> at rate 5, pair64 / block64 at rate 25, the whole-block kernel at rate
    100 — its three outputs enter the next upsample conv's three-input prologue — and a generic 16-channel last stage; tail groups
    split a last stage that is not the whole-block kernel;
  * small_v496 (248 / 124 / 62 / 31 in 256 / 128 / 64 / 32): pad channels in every fused kernel, every upsample conv (padded Cout), the
    output conv (C = 31) and the input conv (15.5 output tiles);
  * small_v768 (384 / 192 / 96 / 48): no fused kernel; the generic kernel over a 256 + 128 channel split, conv_gemm_kernel with 4 and
    6 leftover tiles on conv1d_mfma_kernel from nt_begin, stages of 1.5 output tiles;
  * small_v1024 (512 / 256 / 128 / 64): an unfused 512-channel stage, resblock_pair_kernel<256> at rate 25 and <128> at rate 100, a
    64-channel last stage whose merged MRF sum the output conv reads in its one-input form, block64 inside a tail group.
Checked: every layer alone against the oracle (default and batch kernels: the same bits), the whole vocoder against the oracle, every
kernel regime's bits, the merged sum into the output conv, streaming and the halo, run shortening and fitted mode, ragged batches
(eager, graph capture, replays) against stand-alone calls, tail groups, and one end-to-end call with waveform stages.

The oracle's own re-association noise (sequential f32 against the AVX2 order, relative rms, measured on the CPU for the inputs used
here) is at most 2.2e-5 for a residual block (the 384- and 512-channel ones: 1.7e-5 .. 2.1e-5) and 8.2e-7 for a single conv (the
1 024 -> 512 transposed conv): twice that stays below the caps of tests/test_gpu_layers.py (2e-4 / 1e-4), which therefore hold as they
are."""
import numpy as np
import pytest

import contour_rule as CR
import filter_rule as FR
import level_rule as LR

pytestmark = pytest.mark.gpu

WAV_RMS_GATE = 1e-4                 # tests/test_gpu_vocoder.py
RESBLOCK_CAP, CONV_CAP = 2e-4, 1e-4       # tests/test_gpu_layers.py
F = np.float32


def _geoms():
    from zerovox_cpp_amd import synth
    return synth.VOC_WIDTH_GEOMETRIES


_M, _O = {}, {}


def _model(ckpt, gname):
    """one model per geometry: it serves every regime (every switch is read at the call)"""
    from zerovox_cpp_amd import capi
    if gname not in _M:
        _M[gname] = capi.Model(ckpt(gname)[0], 0)
    _M[gname].set_graph_mode(False)
    return _M[gname]


def _oracle(ckpt, gname):
    from oracle import zvoracle
    if gname not in _O:
        _O[gname] = zvoracle.Oracle(ckpt(gname)[2])
    return _O[gname]


def teardown_module(module):
    for k in list(_M):
        _M.pop(k).close()
    _O.clear()


def _rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))


def _bits(w):
    return np.ascontiguousarray(w, dtype=F).view(np.uint32)


def _same(what, got, want):
    assert got.shape == want.shape, what
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert bad.size == 0, (what, bad.size, bad[:8])


# ---- 1. every layer alone ---------------------------------------------------------------------------------------------------------

def _layer(ckpt, gname, name, kind, index, x, cols, cap, **kw):
    """zv_debug_layer against the oracle's layer under the default switches; once more, the lane poisoned in between, under
    BATCH_REGIME (the kernels only batches pick by themselves), which must give the same bits"""
    from zerovox_cpp_amd import capi
    from parity_helpers import BATCH_REGIME, layer_gate, oracle_pair
    m, o = _model(ckpt, gname), _oracle(ckpt, gname)
    got = m.debug_layer(kind, index, x, cols, **kw)
    m.poison()
    with capi.switches(**BATCH_REGIME):
        gotb = m.debug_layer(kind, index, x, cols, **kw)
    okind = {m.LAYER_VOC_RESBLOCK: o.LAYER_VOC_RESBLOCK, m.LAYER_VOC_UPSAMPLE: o.LAYER_VOC_UPSAMPLE, m.LAYER_VOC_INPUT: o.LAYER_VOC_INPUT,
             m.LAYER_VOC_OUTPUT: o.LAYER_VOC_OUTPUT}[kind]
    ref, alt = oracle_pair(o, "layer", okind, index, x, cols, **kw)
    layer_gate(f"{gname} {name}", got, ref, alt, cap)
    _same((gname, name, "batch kernels"), gotb, got)


@pytest.mark.parametrize("block", list(range(12)))
@pytest.mark.parametrize("gname", _geoms())
def test_every_residual_block(ckpt, gname, block):
    """all 12 residual blocks, 32 frames at the stage's rate"""
    m = _model(ckpt, gname)
    stage = block // 3
    C, rate = m.voc_channels(stage), m.voc_rate(stage)
    x = (0.5 * np.random.default_rng(100 + block).standard_normal((32 * rate, C))).astype(F)
    _layer(ckpt, gname, f"block {block} (C={C})", m.LAYER_VOC_RESBLOCK, block, x, C, RESBLOCK_CAP)


@pytest.mark.parametrize("idx", [0, 1, 2, 3])
@pytest.mark.parametrize("gname", _geoms())
def test_every_transposed_conv(ckpt, gname, idx):
    """leaky_relu(0.1) + conv_transpose1d, 48 frames at the stage's input rate"""
    _, g, _ = ckpt(gname)
    m = _model(ckpt, gname)
    cin = g.voc_channels >> idx
    cout, s = cin // 2, g.upsample_scales[idx]
    rate_in = 1 if idx == 0 else m.voc_rate(idx - 1)
    x = (0.7 * np.random.default_rng(400 + idx).standard_normal((48 * rate_in, cin))).astype(F)
    _layer(ckpt, gname, f"conv_transpose1d {idx} ({cin}->{cout}, x{s})", m.LAYER_VOC_UPSAMPLE, idx, x, cout, CONV_CAP, out_rows=x.shape[0] * s)


@pytest.mark.parametrize("gname", _geoms())
def test_input_conv_and_output_conv(ckpt, gname):
    """(mel - mean) / scale + input conv k7 on 96 frames; leaky_relu(0.01) + conv k7 (C -> 1) + tanh on 16 frames of a given MRF mean"""
    from zerovox_cpp_amd import synth
    _, g, t = ckpt(gname)
    m = _model(ckpt, gname)
    _layer(ckpt, gname, "input conv", m.LAYER_VOC_INPUT, 0, synth.vocoder_mel(g, t, 41, 96), g.voc_channels, CONV_CAP)
    C = g.voc_channels >> len(g.upsample_scales)
    x = (0.6 * np.random.default_rng(43).standard_normal((16 * g.hop_size, C))).astype(F)
    _layer(ckpt, gname, f"output conv + tanh (C={C})", m.LAYER_VOC_OUTPUT, 0, x, 0, CONV_CAP)


# ---- 2. the whole vocoder ---------------------------------------------------------------------------------------------------------

def _vocoder_gate(what, wav, ref, alt):
    """waveform rms error <= 1e-4 (tests/test_gpu_vocoder.py) and <= twice the oracle's own re-association noise on this input"""
    assert wav.shape == ref.shape and np.isfinite(wav).all(), what
    err, floor = _rms(wav - ref), _rms(alt - ref)
    print(f"{what}: wav rms err {err:.3e} (oracle self-noise {floor:.3e}), signal rms {_rms(ref):.3f}")
    assert err <= WAV_RMS_GATE, what
    assert err <= 2.0 * floor, what


@pytest.mark.parametrize("gname", _geoms())
def test_vocoder_matches_oracle(ckpt, gname):
    """the whole vocoder against the oracle at 1, 24 and 37 frames"""
    from zerovox_cpp_amd import synth
    from parity_helpers import oracle_pair
    _, g, tensors = ckpt(gname)
    m, o = _model(ckpt, gname), _oracle(ckpt, gname)
    for T in (1, 24, 37):
        mel = synth.vocoder_mel(g, tensors, 7, T)
        m.poison()
        wav = m.vocode(mel)
        assert wav.shape == (T * g.hop_size,)
        ref, alt = oracle_pair(o, "vocoder", mel)
        _vocoder_gate(f"{gname} T={T}", wav, ref, alt)


# ---- 3. every kernel regime ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gname", _geoms())
def test_kernel_regimes_give_the_same_bits(ckpt, gname):
    """every entry of VOCODER_REGIMES on one utterance of 41 frames: the default's bits, the lane poisoned before each call — also
    where the width cannot enter the regime"""
    from zerovox_cpp_amd import capi, synth
    from parity_helpers import BATCH_REGIME, VOCODER_REGIMES
    _, g, tensors = ckpt(gname)
    mel = synth.vocoder_mel(g, tensors, 51, 41)
    m = _model(ckpt, gname)
    want = m.vocode(mel)
    for name, env in list(VOCODER_REGIMES) + [("batch_regime", BATCH_REGIME)]:
        m.poison()
        with capi.switches(**{k: int(v) for k, v in env.items()}):
            got = m.vocode(mel)
        _same((gname, name), got, want)


# ---- 4. the merged sum into the output conv -------------------------------------------------------------------------------------------

def _merge_cases():
    from parity_helpers import WIDTH_MERGE_CASES
    return [pytest.param(*c, id=f"{c[0]}-{'-'.join(f'{k}={v}' for k, v in c[1].items())}") for c in WIDTH_MERGE_CASES]


@pytest.mark.parametrize("gname,sw,plan,out_merged", _merge_cases())
def test_merged_sum_into_the_output_conv(ckpt, gname, sw, plan, out_merged):
    """under ZV_MERGE_ALWAYS (with and without ZV_MERGE_SEQ = 0) the waveform has the bits of the ZV_NO_MERGE = 1 run and passes the
    oracle gates.  Which form ran is the plan tests/test_voc_plan_cpu.py holds csrc/voc_plan.h to for these switches at this length
    (parity_helpers.WIDTH_MERGE_CASES): a last stage that ends in '1' stores the MRF sum alone and the output conv reads one tensor
    (out_conv_tanh_kernel's one-input branch); small_v1024 does by itself, small_v496 (a whole-block last stage) with that kernel off"""
    from zerovox_cpp_amd import capi, synth
    from parity_helpers import WIDTH_MERGE_T, oracle_pair
    stages = plan.split()[2:]
    assert len(stages) == 4 and (stages[3][-1] == "1") == out_merged and any(s[-1] in "13" for s in stages)
    assert gname != "small_v1024" or out_merged
    _, g, tensors = ckpt(gname)
    m, o = _model(ckpt, gname), _oracle(ckpt, gname)
    mel = synth.vocoder_mel(g, tensors, 53, WIDTH_MERGE_T)
    with capi.switches(**{**sw, "ZV_MERGE_ALWAYS": 0, "ZV_NO_MERGE": 1}):
        apart = m.vocode(mel)
    m.poison()
    with capi.switches(**sw):
        got = m.vocode(mel)
    _same((gname, sw), got, apart)
    ref, alt = oracle_pair(o, "vocoder", mel)
    _vocoder_gate(f"{gname} {sw}", got, ref, alt)


# ---- 5. streaming ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gname", _geoms())
def test_halo_and_streaming(ckpt, gname):
    """the width changes no tap count: the exact receptive radius is medium's 20 frames and zv_vocoder_halo_frames() medium's 23 (it
    sums fractional frames per layer, rounds up and adds a spare frame: tests/test_gpu_vocoder_geometries.py, which holds it to
    radius <= halo <= radius + 4).  zv_vocode_stream in chunks of 16 (shorter than the halo) and 50 frames gives zv_vocode's bits at
    120 frames"""
    from zerovox_cpp_amd import synth
    from parity_helpers import receptive_radius
    _, g, tensors = ckpt(gname)
    m = _model(ckpt, gname)
    r, H = receptive_radius(g, tensors), m.vocoder_halo_frames()
    assert (r, H) == (20, 23) and r <= H <= r + 4, (r, H)
    T = 120
    mel = synth.vocoder_mel(g, tensors, 52, T)
    full = m.vocode(mel)
    for chunk in (16, 50):
        m.poison()
        chunks = m.vocode_stream(mel, chunk)
        assert [c[0] for c in chunks] == [a * g.hop_size for a in range(0, T, chunk)]
        _same((gname, chunk), np.concatenate([c[1] for c in chunks]), full)


# ---- 6. run shortening and fitted mode ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gname", _geoms())
def test_run_shortening_and_fitted_mode(ckpt, gname):
    """30 frames of speech in a capacity of 200: ZV_VOC_RUNS = 2 (the 170 constant frames vocoded as one run: the table says so)
    gives the bits of ZV_VOC_RUNS = 0; the fitted call gives, over the speech, the bits of the unfitted call at T = 30, and +0.0
    behind it"""
    from zerovox_cpp_amd import capi, synth
    _, g, _ = ckpt(gname)
    m = _model(ckpt, gname)
    hop, T, nf = g.hop_size, 200, 30
    ids, puncts, style = synth.encoder_inputs(g, 61, 12)
    with capi.switches(ZV_VOC_RUNS=0):
        w0, n0 = m.synthesize(ids, puncts, style, T, target_frames=nf)
        assert n0 == nf and m.voc_runs().shape[0] == 0
    with capi.switches(ZV_VOC_RUNS=2):
        m.poison()
        w2, n2 = m.synthesize(ids, puncts, style, T, target_frames=nf)
        tab = m.voc_runs()
        assert n2 == nf and tab.shape == (1, 4) and tab[0, 3] > 0 and tab[0, 1] + tab[0, 3] == T, tab
    _same((gname, "runs"), w2, w0)
    # fitted mode's contract (tests/test_gpu_fitted.py): the unfitted call at T = n_frames — decoder and vocoder run over the speech alone
    wu, nu = m.synthesize(ids, puncts, style, nf, target_frames=nf)
    m.poison()
    wf, nff = m.synthesize(ids, puncts, style, T, fitted=True, target_frames=nf)
    assert nff == nu == nf and wu.shape == (nf * hop,) and wf.shape == (T * hop,)
    _same((gname, "fitted speech"), wf[:nf * hop], wu)
    assert not _bits(wf[nf * hop:]).any(), gname


# ---- 7. ragged batches ---------------------------------------------------------------------------------------------------------

RAGGED = [(9, 40), (33, 64), (70, 96), (51, 131)]          # (phonemes, capacity): no capacity a multiple of a tile height x rate


@pytest.mark.parametrize("regime", ["default", "batch_kernels_merged"])
@pytest.mark.parametrize("gname", _geoms())
def test_ragged_batch_equals_standalone(ckpt, gname, regime):
    """four utterances through one prepared batch: eager, graph capture and two replays, the lane poisoned and the outputs prefilled
    with a sentinel before each run, give every utterance's stand-alone bits; under the default switches and under BATCH_REGIME with
    ZV_MERGE_ALWAYS = 1"""
    from zerovox_cpp_amd import capi, synth
    from parity_helpers import BATCH_REGIME
    _, g, _ = ckpt(gname)
    m = _model(ckpt, gname)
    utts = [(*synth.encoder_inputs(g, 7100 + 13 * i, N), T) for i, (N, T) in enumerate(RAGGED)]
    alone = [m.synthesize(*u) for u in utts]
    assert all(0 < n <= u[3] and np.isfinite(w).all() for (w, n), u in zip(alone, utts))
    sw = {} if regime == "default" else {**BATCH_REGIME, "ZV_MERGE_ALWAYS": 1}
    try:
        with capi.switches(**sw):
            bc = m.prepare_batch(utts)
            for what, graph, poison in [("eager", False, 0xFF), ("graph capture", True, 0x00), ("graph replay", True, 0xFF), ("second replay", True, 0x00)]:
                m.set_graph_mode(graph)
                m.poison(poison)
                for w in bc.wavs:
                    w.fill(7.0)
                bc.run()
                for i, ((w, n), (w0, n0)) in enumerate(zip(bc.results(), alone)):
                    assert n == n0, (gname, what, i)
                    _same((gname, regime, what, i), w, w0)
    finally:
        m.set_graph_mode(False)


# ---- 8. tail groups ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gname", ["small_v256", "small_v1024"])
def test_batch_split_into_tail_groups(ckpt, gname):
    """the smallest batch that splits into tail groups (16 utterances at T = 900: 16 MiB of waveform), fitted, target frames from 1
    to 900: ZV_TAIL_GROUPS = 2 and 8 give the bits of the one-group run, eagerly and under a graph replayed twice; one utterance of
    the one-group run equals its stand-alone call.  small_v256: a generic last stage inside a group; small_v1024: a 64-channel one
    (block64 and the merged sum into the output conv, tests/native/voc_plan_check.cpp)"""
    from zerovox_cpp_amd import capi, synth
    _, g, _ = ckpt(gname)
    m = _model(ckpt, gname)
    hop, T = g.hop_size, 900
    tfs = [900, 500, 250, 37, 899, 1, 640, 333, 65, 700, 31, 32, 33, 450, 820, 128]
    utts = [(*synth.encoder_inputs(g, 700 + i, 40 + 9 * i), T, None, None, tf) for i, tf in enumerate(tfs)]
    assert len(utts) * T * hop * 4 >= 16 << 20 and len(utts) // 2 >= 8
    try:
        with capi.switches(ZV_TAIL_GROUPS=1):
            bc = m.prepare_batch(utts, fitted=True)
            for w in bc.wavs:
                w.fill(7.0)
            bc.run()
            one = [(w.copy(), n) for w, n in bc.results()]
            assert [n for _, n in one] == tfs and not any((w == 7.0).any() for w, _ in one)      # every sample was written
            w3, n3 = m.synthesize(*utts[3][:4], fitted=True, target_frames=tfs[3])
            assert n3 == tfs[3]
            _same((gname, "one group against alone"), one[3][0], w3)
        for groups in (2, 8):
            with capi.switches(ZV_TAIL_GROUPS=groups):
                for graph in (False, True):
                    m.set_graph_mode(graph)
                    bc = m.prepare_batch(utts, fitted=True)
                    for rep in range(3 if graph else 1):                  # graph: capture, then two replays
                        m.poison(0x00 if rep == 1 else 0xFF)
                        for w in bc.wavs:
                            w.fill(7.0)
                        bc.run()
                        for i, ((w, n), (w0, n0)) in enumerate(zip(bc.results(), one)):
                            assert n == n0, (gname, groups, graph, rep, i)
                            _same((gname, groups, graph, rep, i), w, w0)
                m.set_graph_mode(False)
    finally:
        m.set_graph_mode(False)


# ---- 9. one end-to-end call with waveform stages --------------------------------------------------------------------------------------

@pytest.mark.parametrize("gname", _geoms())
def test_synthesize_with_waveform_stages(ckpt, gname):
    """zv_synthesize with a one-tap filter, a volume and a level contour equals the plain call taken through the Python rules
    (tests/filter_rule.py, level_rule.py, contour_rule.py; the per-stage tests hold every stage to them at medium): the stages find the
    waveform where this width's layout puts it"""
    from zerovox_cpp_amd import capi, synth
    _, g, _ = ckpt(gname)
    m = _model(ckpt, gname)
    hop, T = g.hop_size, 64
    ids, puncts, style = synth.encoder_inputs(g, 81, 21)
    plain, nf, dur = m.synthesize(ids, puncts, style, T, return_durations=True)
    assert 0 < nf <= T
    vol = capi.Volume(0.8, 0.07, 0.5)
    taps = np.array([0.5], F)
    m.poison()
    w, n, d, level, contour = m.synthesize(ids, puncts, style, T, return_durations=True, volume=vol, return_levels=True,
                                           return_contour=True, filter=taps)
    assert n == nf and np.array_equal(d, dur)
    v = LR.rule(FR.apply(plain, taps, T * hop), nf * hop, (vol.gain, vol.target_rms, vol.peak_ceiling))
    _same((gname, "waveform"), w, v["out"])
    assert LR.level_bits(level) == LR.level_bits(v["level"]), (gname, level, v["level"])
    c = CR.rule(w, T, hop, dur)
    assert np.array_equal(CR.bits(contour.frames), CR.bits(c["frames"])) and np.array_equal(CR.bits(contour.phonemes), CR.bits(c["phonemes"])), gname
