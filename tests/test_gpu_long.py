"""-m gpu: the sizes the C-ABI promises and nothing else ran — one utterance of zv_max_frames() frames, launch groups of 64
utterances / 64 Ki frames of capacity, zv_vocode_stream beyond the limit — at the production geometry (synth.MEDIUM), on models
of this module's own that are closed when it ends (an arena of tens of GB does not ride along in a session-wide fixture).

Where the arithmetic is least forgiving (include/zerovox_amd.h is the specification; csrc/vocoder.cpp, capi.cpp, model.cpp):
  * Tmax = 32 768 frames.  The last vocoder stage's tensor is 32 768 x 300 rows x 32 channels x 4 B = 1.26 GB, addressed by the
    ResBlock kernels through a buffer descriptor with a signed 32-bit byte offset: byte 2^30 falls into frame 27 962 (so does row
    2^23), stage 2's byte 2^29 and stage 1's byte 2^28 into frame 20 971, stage 1's 2^27 and stage 2's 2^28 into frame 10 485
    (parity_helpers.offset_crossing_frames lists every such frame from 2^27 on; tests/test_long_cpu.py checks the list);
  * in a group of 65 536 frames the last stage's tensor is 2.5 GB: the segments of utterances 55 ... 63 of 64 x 1 024 start past
    2^31 bytes, row numbers pass 2^24;
  * one long utterance selects by its row count the kernels that otherwise only batches use: resblock_block64_kernel from
    T = 2 499 (T x 100 / 244 >= 4 x 256 compute units), the f16 operand pass + conv_gemm_kernel for the second upsample conv from
    T = 3 277 (5 T >= 16 384 rows) and for the first from T = 16 384, the merged MRF sum, the fused 256-channel stage;
  * the decoder's InstanceNorm / AdaIN statistics run over all 32 768 rows (1 024 partial blocks per channel).

Checked.  Vocoder at Tmax: every sample against chunked vocoding (each chunk a call of a size the suite pins to the reference),
64-frame windows against the oracle at the start, the end and around every crossing frame, every kernel regime, graph replay,
lengths either side of the self-selected thresholds (prefix consistency + the launch counts zv_profile_end reports), 40 000
frames through zv_vocode_stream.  Decoder at Tmax: the whole output and every block of 256 frames against the oracle, every conv
regime, AdaIN and asr_res alone on 32 768 rows against float64 numpy.  Encoder: the length regulator as an exact gather up to
and beyond Tmax frames; the chain and fitted synthesis at capacity Tmax.  Launch groups: 64 x 1 024, 2 x 32 768, 4 x 16 384,
3 x 21 824 as one group each, 3 x 21 825, 64 x 1 025 and 65 x 1 008 split (and refused by _begin), against stand-alone calls —
eager, captured, replayed, on two lanes in flight, fitted.  zv_model_reserve(1501, Tmax) first.

Every gate is a ratio to the oracle's own re-association noise on the same input (2.0 rms, 1.5 max-abs, 4.0 for AdaIN alone) or
the suite's absolute waveform gate (rms <= 1e-4); the measured ratios are printed (-s).

Measured on an MI355X (16 CPUs for the oracle): the module's 64 tests take 94 s of wall time (vocoder 26 s, launch groups
16 s, encoder / chain / reserve 5 s, decoder 47 s of which the oracle's decoder pair at T = 32 768 is 35 s); the rest of the
-m gpu suite has not been timed beside it yet.  The first T = Tmax call takes 13.82 GiB of device memory (zv_model_reserve(1501, Tmax):
13.74 GiB), the first 64 x 1 024 group 27.73 GiB.  Worst oracle window: 0.990 x the oracle's own noise (frames [13 949, 14 013),
the last stage's byte 2^29).  Decoder at Tmax: rms 0.971 x and max-abs 1.037 x the floor; worst block 0.998 x its own rms floor
(block 82), 1.230 x its own max-abs floor (block 20).  AdaIN on 32 768 rows: error 3.1e-6 ... 3.4e-6, equal to the oracle's own
f32 distance from float64; asr_res 1.43e-4 (oracle 8.5e-5).  Launch counts: voc_resblock_s2 3 -> 4 at T = 2 499, voc_upsample
4 -> 5 at T = 3 277, equal at 16 383 / 16 384.
"""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ZV_OK, ZV_ERR_ARG = 0, 5
WAV_RMS_GATE = 1e-4                 # tests/test_gpu_full_size.py, tests/test_gpu_vocoder.py
TMAX_MEDIUM = 32768
T_STREAM = 40000                    # zv_vocode_stream "has no such limit on the total"
N_CU = 256                          # compute units of an MI355X (voc_plan.h compares workgroup counts with n_cu)
THRESHOLD_LENGTHS = (2498, 2499, 3276, 3277, 16383, 16384, TMAX_MEDIUM - 1, TMAX_MEDIUM)


def _rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))


def _free_bytes():
    """free device memory (reading only)"""
    import torch
    return int(torch.cuda.mem_get_info()[0])


@pytest.fixture(scope="module")
def env(ckpt):
    """the module's own default-regime model with the vocoder's output at Tmax, closed when the module ends"""
    from zerovox_cpp_amd import capi, synth
    path, g, tensors = ckpt("medium")
    _free_bytes()
    m = capi.Model(path, 0)
    try:
        Tmax = m.max_frames()
        assert Tmax == TMAX_MEDIUM          # Model::max_frames_per_utterance: a changed formula is noticed here
        H = m.vocoder_halo_frames()
        mel_long = synth.vocoder_mel(g, tensors, 61, T_STREAM)
        mel = mel_long[:Tmax]
        assert np.array_equal(mel, synth.vocoder_mel(g, tensors, 61, Tmax))
        before = _free_bytes()
        t0 = time.time()
        full = m.vocode(mel)
        print(f"\nvocode at T = {Tmax}: first call {time.time() - t0:.2f} s, device memory taken {(before - _free_bytes()) / 2 ** 30:.2f} GiB")
        assert full.shape == (Tmax * g.hop_size,) and np.isfinite(full).all()
        yield dict(m=m, path=path, g=g, tensors=tensors, Tmax=Tmax, H=H, mel_long=mel_long, mel=mel, full=full)
    finally:
        m.close()


# ---- 1. vocoder at Tmax ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chunk", [2048, 1500])
def test_vocoder_at_tmax_equals_chunked_vocoding_on_every_sample(env, chunk):
    """every chunk is a call of at most chunk + 2 H frames; every vocoder kernel sums in an order that depends neither on the
    tile nor on T, so the concatenation is the whole utterance bit for bit: a tile multiple and a chunk that is none"""
    m, g, Tmax = env["m"], env["g"], env["Tmax"]
    chunks = m.vocode_stream(env["mel"], chunk)
    assert [c[0] for c in chunks] == [a * g.hop_size for a in range(0, Tmax, chunk)]
    got = np.concatenate([c[1] for c in chunks])
    assert got.shape == env["full"].shape
    diff = np.flatnonzero(got != env["full"])
    assert not len(diff), f"chunk {chunk}: {len(diff)} samples differ, first at frame {diff[0] // g.hop_size}, last at frame {diff[-1] // g.hop_size}"


def test_vocoder_at_tmax_against_the_oracle_where_offsets_cross_powers_of_two(env):
    from oracle import zvoracle
    import parity_helpers as ph
    m, g, Tmax, H, mel, full = env["m"], env["g"], env["Tmax"], env["H"], env["mel"], env["full"]
    hop = g.hop_size
    assert H >= ph.receptive_radius(g, env["tensors"])
    assert [m.voc_rate(i) for i in range(4)] == [5, 25, 100, 300] and [m.voc_channels(i) for i in range(4)] == [256, 128, 64, 32]
    bpf = ph.voc_stage_bytes_per_frame([m.hp.voc_upsample_scales[i] for i in range(m.hp.voc_num_upsamples)], m.hp.voc_channels)
    cross = ph.offset_crossing_frames(bpf, Tmax)
    # the last stage's 2^30 (and its row 2^23), stage 2's 2^29, stage 1's 2^28 and 2^27
    assert (3, 30) in cross[27962] and (2 ** 23) // m.voc_rate(3) == 27962
    assert (2, 29) in cross[20971] and (1, 28) in cross[20971] and (1, 27) in cross[10485]
    windows = ph.oracle_windows(cross, Tmax)
    for f in cross:
        assert any(a <= f < b for a, b in windows), f
    o = zvoracle.Oracle(env["tensors"])
    worst = (0.0, None)
    for a, b in windows:
        lo, hi = max(0, a - H), min(Tmax, b + H)
        ref, alt = (w[(a - lo) * hop:(b - lo) * hop] for w in ph.oracle_pair(o, "vocoder", mel[lo:hi]))
        got = full[a * hop:b * hop]
        what = f"frames [{a}, {b})" + "".join(f" s{i}:2^{k}" for f in cross if a <= f < b for i, k in cross[f])
        ph.layer_gate(what, got, ref, alt, float("inf"))
        err, floor = _rms(got - ref), _rms(alt - ref)
        assert err <= WAV_RMS_GATE, (what, err)
        if floor > 0 and err / floor > worst[0]:
            worst = (err / floor, what)
    print(f"worst window: error {worst[0]:.3f} x the oracle's own noise, {worst[1]}")


def test_vocoder_at_tmax_graph_capture_and_replay(env):
    m = env["m"]
    m.set_graph_mode(True)
    try:
        assert np.array_equal(m.vocode(env["mel"]), env["full"]), "capture"
        assert np.array_equal(m.vocode(env["mel"]), env["full"]), "replay"
    finally:
        m.set_graph_mode(False)


def _vocoder_regimes():
    from parity_helpers import VOCODER_REGIMES
    return VOCODER_REGIMES


@pytest.mark.parametrize("regime", _vocoder_regimes(), ids=lambda r: r[0])
def test_vocoder_at_tmax_in_every_kernel_regime(env, regime):
    """a fresh model per regime, its call inside the regime's switches (read at the call): the default's bits"""
    from zerovox_cpp_amd import capi
    name, sw = regime
    with capi.switches(**sw):
        m = capi.Model(env["path"], 0)
        try:
            got = m.vocode(env["mel"])
        finally:
            m.close()
    diff = np.flatnonzero(got != env["full"])
    assert not len(diff), f"{name}: {len(diff)} samples differ, frames {diff[0] // 300} .. {diff[-1] // 300}"


def test_threshold_lengths_are_the_ones_the_schedule_switches_at():
    """csrc/voc_plan.h for one utterance (t_max = T, nseg = 1; tests/test_voc_plan_cpu.py asks the header itself): resblock_block64_kernel when T x 100 / 244 >= 4 n_cu (integer
    division), the f16 operand pass + conv_gemm_kernel for upsample conv i when its input rows T x rate >= 16 384 (i = 1: rate 5,
    i = 0: rate 1)"""
    first = lambda cond: next(T for T in range(1, TMAX_MEDIUM + 1) if cond(T))
    assert first(lambda T: T * 100 // 244 >= 4 * N_CU) == 2499
    assert first(lambda T: T * 5 >= 16384) == 3277
    assert first(lambda T: T >= 16384) == 16384
    assert THRESHOLD_LENGTHS == (2498, 2499, 3276, 3277, 16383, 16384, TMAX_MEDIUM - 1, TMAX_MEDIUM)


def test_vocoder_lengths_around_the_self_selected_thresholds(env):
    """prefix consistency against the Tmax run on either side of every threshold, and the launch counts zv_profile_end reports
    show that the kernel family changed: voc_resblock_s2 gains a launch at T = 2 499 (resblock_block64_kernel runs the 3-tap
    branch's first two pairs, the other branches keep their three pair launches), voc_upsample gains one at T = 3 277 (the f16
    operand pass).  At T = 16 384 the first upsample conv moves to conv_gemm_kernel with NO launch of its own (the input conv
    writes its f16 operand): the names cannot tell 16 383 from 16 384, so there the counts must be equal and the bits decide"""
    m, g, H, mel, full = env["m"], env["g"], env["H"], env["mel"], env["full"]
    hop = g.hop_size
    counts = {}
    for T in THRESHOLD_LENGTHS:
        m.profile_begin()
        w = m.vocode(mel[:T])
        stats = {p["name"]: p["launches"] for p in m.profile_end()}
        counts[T] = stats
        print(f"T = {T}: " + ", ".join(f"{k} {v}" for k, v in sorted(stats.items())))
        n = (T - H) * hop if T < env["Tmax"] else T * hop
        assert w.shape == (T * hop,) and np.isfinite(w).all(), T
        assert np.array_equal(w[:n], full[:n]), T
    assert counts[2499]["voc_resblock_s2"] == counts[2498]["voc_resblock_s2"] + 1
    assert counts[3277]["voc_upsample"] == counts[3276]["voc_upsample"] + 1
    assert counts[3276]["voc_upsample"] == counts[2499]["voc_upsample"] and counts[3276]["voc_resblock_s2"] == counts[2499]["voc_resblock_s2"]
    assert counts[16384]["voc_upsample"] == counts[16383]["voc_upsample"] == counts[3277]["voc_upsample"]
    assert counts[env["Tmax"]] == counts[env["Tmax"] - 1]


def test_vocode_stream_beyond_the_frame_limit(env):
    m, g, Tmax, H, full = env["m"], env["g"], env["Tmax"], env["H"], env["full"]
    hop, chunk, mel = g.hop_size, 4096, env["mel_long"]
    with pytest.raises(Exception) as ei:
        m.vocode(mel)
    assert getattr(ei.value, "status", None) == ZV_ERR_ARG
    chunks = m.vocode_stream(mel, chunk)
    assert [c[0] for c in chunks] == [a * hop for a in range(0, T_STREAM, chunk)]
    got = np.concatenate([c[1] for c in chunks])
    assert got.shape == (T_STREAM * hop,) and np.isfinite(got).all()
    n = (Tmax - H) * hop
    assert np.array_equal(got[:n], full[:n])
    tail = m.vocode(mel[T_STREAM - chunk:])
    k = (chunk - H) * hop
    assert np.array_equal(got[-k:], tail[-k:])


# ---- 2. decoder at Tmax ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dec(env):
    from zerovox_cpp_amd import synth
    g = env["g"]
    hid = synth.decoder_hidden(g, 42, env["Tmax"])
    _, _, style = synth.encoder_inputs(g, 7, 16)
    t0 = time.time()
    mel = env["m"].decode(hid, style)
    print(f"\ndecode at T = {env['Tmax']}: first call {time.time() - t0:.2f} s")
    assert mel.shape == (env["Tmax"], g.num_mels) and np.isfinite(mel).all()
    return hid, style, mel


def test_decoder_at_tmax_against_the_oracle_whole_and_per_block(env, dec):
    """statistics over all T rows: nothing can be windowed, so the full oracle in both orders; then 128 blocks of 256 frames each
    gated on its own (a misaddressed tile of 64 rows does not move a global rms)"""
    from oracle import zvoracle
    import parity_helpers as ph
    hid, style, got = dec
    o = zvoracle.Oracle(env["tensors"])
    t0 = time.time()
    ref, alt = ph.oracle_pair(o, "decoder", hid, style)
    print(f"oracle decoder pair at T = {env['Tmax']}: {time.time() - t0:.0f} s")
    assert np.isfinite(ref).all() and np.isfinite(alt).all()
    e_rms, f_rms = _rms(got - ref), _rms(alt - ref)
    e_max, f_max = float(np.max(np.abs(got - ref))), float(np.max(np.abs(alt - ref)))
    print(f"decoder T = {env['Tmax']}: rms err {e_rms:.3e} (floor {f_rms:.3e}, ratio {e_rms / f_rms:.3f}), max {e_max:.3e} "
          f"(floor {f_max:.3e}, ratio {e_max / f_max:.3f}), mel rms {_rms(ref):.3f}")
    assert e_rms <= 2.0 * f_rms and e_max <= 1.5 * f_max
    ph.block_gates(f"decoder T = {env['Tmax']}", got, ref, alt, block=256)


DEC_REGIMES = (("prepass_0", {"ZV_DEC_PREPASS": 0}), ("prepass_1", {"ZV_DEC_PREPASS": 1}), ("gemm_0", {"ZV_CONV_GEMM": 0}),
               ("gemm_2", {"ZV_CONV_GEMM": 2}), ("single_0", {"ZV_CONV_SINGLE": 0}), ("single_2", {"ZV_CONV_SINGLE": 2}),
               ("nt_1", {"ZV_CONV_NT": 1}), ("nt_2", {"ZV_CONV_NT": 2}), ("plain_grid", {"ZV_CONV_XCD": 0}),
               ("gemm_order_0", {"ZV_GEMM_ORDER": 0}))


@pytest.mark.parametrize("regime", DEC_REGIMES, ids=lambda r: r[0])
def test_decoder_at_tmax_in_every_conv_regime(env, dec, regime):
    from zerovox_cpp_amd import capi
    hid, style, mel = dec
    with capi.switches(**regime[1]):
        got = env["m"].decode(hid, style)
    rows = np.flatnonzero(np.any(got != mel, axis=1))
    assert not len(rows), f"{regime[0]}: {len(rows)} rows differ, {rows[0]} .. {rows[-1]}"


def _adain_f64(tensors, idx, x, style):
    """AdaIN1d in float64: ((x - mean) / sqrt(var + eps)) (1 + gamma) + beta, mean and biased variance over all rows, gamma and
    beta from the f32 fc weights"""
    from parity_helpers import EPS
    fw = tensors[f"_mel_decoder.decode.{idx // 2}.norm{1 + (idx & 1)}.fc.w"].astype(np.float64)
    fb = tensors[f"_mel_decoder.decode.{idx // 2}.norm{1 + (idx & 1)}.fc.b"].astype(np.float64)
    C = x.shape[1]
    h = fw.reshape(2 * C, -1) @ style.astype(np.float64) + fb
    x = x.astype(np.float64)
    return (x - x.mean(axis=0)) / np.sqrt(x.var(axis=0) + EPS) * (1.0 + h[:C]) + h[C:]


def test_adain_and_asr_res_alone_on_tmax_rows(env):
    """one layer through zv_debug_layer at rows = Tmax against float64 numpy, the input's channel means far from zero
    (parity_helpers.offset) so that a statistic lost among 1 024 partial sums shows; the floor is the oracle's f32 result
    against the same float64 reference"""
    from oracle import zvoracle
    import parity_helpers as ph
    m, g, t, Tmax = env["m"], env["g"], env["tensors"], env["Tmax"]
    o = zvoracle.Oracle(t)
    E, R = g.E, g.residual_dim
    style = (0.05 * np.random.default_rng(8).standard_normal(E)).astype(np.float32)
    for idx in range(10):
        C = ((2 * E, 2 * E, E, E, E) if idx & 1 else (2 * E + R, 2 * E + R, 2 * E + R, E, E))[idx // 2]
        x, _ = ph.offset(3000 + idx, Tmax, C)
        got = m.debug_layer(m.LAYER_DEC_ADAIN, idx, x, C, style=style)
        ref = _adain_f64(t, idx, x, style)
        alt = o.layer(o.LAYER_DEC_ADAIN, idx, x, C, style=style)
        ph.layer_gate(f"AdaIN {idx} (C={C}) rows={Tmax}", got, ref, alt, 1e-5, floor_mult=4.0)
    # asr_res = InstanceNorm(conv1x1(x)): the conv's operands are f16 (x rounded as the kernel rounds it, the weights are f16)
    x, _ = ph.offset(3100, Tmax, E, common_ratio=1e3)
    w = t["_mel_decoder.asr_res.0.w"].astype(np.float64).reshape(R, E)
    y = x.astype(np.float16).astype(np.float64) @ w.T + t["_mel_decoder.asr_res.0.b"].astype(np.float64)
    ref = (y - y.mean(axis=0)) / np.sqrt(y.var(axis=0) + ph.EPS) * t["_mel_decoder.asr_res.1.w"].astype(np.float64) + \
        t["_mel_decoder.asr_res.1.b"].astype(np.float64)
    got = m.debug_layer(m.LAYER_DEC_ASR_RES, 0, x, R)
    alt = o.layer(o.LAYER_DEC_ASR_RES, 0, x, R)
    ph.layer_gate(f"asr_res rows={Tmax}", got, ref, alt, 1e-3)


# ---- 3. encoder and the chain at Tmax ----------------------------------------------------------------------------------------

def _forced(N, total):
    """duration_frames [N] that sum to `total`, as even as integers allow"""
    return (total // N + (np.arange(N) < total % N)).astype(np.int32)


def _one_phoneme(N, i, frames):
    d = np.zeros(N, np.int32)
    d[i] = frames
    return d


@pytest.mark.parametrize("N", [1501, 340])
def test_length_regulator_is_an_exact_gather_up_to_tmax(env, N):
    from zerovox_cpp_amd import synth
    from test_gpu_phoneme_controls import restate_durations, restated_hidden, timings
    m, g, Tmax = env["m"], env["g"], env["Tmax"]
    assert N <= g.max_seq_len + 1
    ids, puncts, style = synth.encoder_inputs(g, 800 + N, N)
    cases = [("sum == Tmax", dict(phonemes=dict(duration_frames=_forced(N, Tmax))), Tmax),
             ("sum == Tmax + 1", dict(phonemes=dict(duration_frames=_forced(N, Tmax + 1))), Tmax),
             ("one phoneme of Tmax", dict(phonemes=dict(duration_frames=_one_phoneme(N, N // 3, Tmax))), Tmax),
             ("duration_scale 16", dict(prosody=dict(duration_scale=16.0)), None)]
    for what, kw, want_nf in cases:
        e = m.encode(ids, puncts, style, Tmax, return_durations=True, **kw)
        fr = kw.get("phonemes", {}).get("duration_frames")
        d = restate_durations(e["logdur"], N, Tmax, kw.get("prosody", {}).get("duration_scale", 1.0), fr)
        if fr is not None:
            assert np.array_equal(d, fr)
        hid, nf = restated_hidden(e["features"], d, Tmax)
        print(f"N = {N}, {what}: {e['n_frames']} frames")
        assert e["n_frames"] == nf == min(int(d.sum()), Tmax) and (want_nf is None or nf == want_nf), (N, what)
        assert np.array_equal(e["durations"], timings(d, Tmax)), (N, what)
        # a gather: np.repeat of the features tap, zero behind
        rep = np.repeat(e["features"], timings(d, Tmax), axis=0)
        assert rep.shape[0] == nf and np.array_equal(e["hidden"][:nf], rep) and not e["hidden"][nf:].any(), (N, what)
        assert np.array_equal(e["hidden"], hid), (N, what)


@pytest.fixture(scope="module")
def chain(env):
    """synthesize at T = Tmax, 340 phonemes at duration_scale 16 (the regulator fills a good part of the capacity)"""
    from zerovox_cpp_amd import synth
    m, g, Tmax = env["m"], env["g"], env["Tmax"]
    ids, puncts, style = synth.encoder_inputs(g, 5, 340)
    pr = dict(duration_scale=16.0)
    wav, nf = m.synthesize(ids, puncts, style, Tmax, prosody=pr)
    assert wav.shape == (Tmax * g.hop_size,) and np.isfinite(wav).all() and 0 < nf <= Tmax
    return ids, puncts, style, pr, wav, nf


def test_chain_at_tmax_equals_its_stages(env, chain):
    m, Tmax = env["m"], env["Tmax"]
    ids, puncts, style, pr, wav, nf = chain
    e = m.encode(ids, puncts, style, Tmax, prosody=pr)
    print(f"chain at T = {Tmax}: {nf} frames filled")
    assert e["n_frames"] == nf
    assert np.array_equal(m.vocode(m.decode(e["hidden"], style)), wav)
    m.set_graph_mode(True)
    try:
        for rep in ("capture", "replay"):
            w, n = m.synthesize(ids, puncts, style, Tmax, prosody=pr)
            assert n == nf and np.array_equal(w, wav), rep
    finally:
        m.set_graph_mode(False)


def test_fitted_synthesis_at_capacity_tmax(env):
    """capacity Tmax, the forced durations fill (a) 5 000, (b) Tmax - 1, (c) Tmax, (d) 0 frames: the live samples are the unfitted
    call's at T = n_frames, the rest is 0.0f"""
    from zerovox_cpp_amd import synth
    m, g, Tmax = env["m"], env["g"], env["Tmax"]
    hop, N = g.hop_size, 340
    ids, puncts, style = synth.encoder_inputs(g, 811, N)
    for nf in (5000, Tmax - 1, Tmax, 0):
        pc = dict(duration_frames=_forced(N, nf))
        w, n, d = m.synthesize(ids, puncts, style, Tmax, phonemes=pc, return_durations=True, fitted=True)
        assert n == nf and int(d.sum()) == nf and w.shape == (Tmax * hop,), nf
        assert not np.isnan(w[nf * hop:]).any() and not w[nf * hop:].any(), (nf, "tail is not zero")
        if nf:
            wr, nr, dr = m.synthesize(ids, puncts, style, nf, phonemes=pc, return_durations=True)
            assert nr == nf and np.array_equal(w[: nf * hop], wr) and np.array_equal(d, dr), nf


# ---- 4. launch groups at their limits ----------------------------------------------------------------------------------------

def _mixed_n(n_utt):
    """1 ... 340 phonemes, the first two the extremes"""
    return [1, 340] + [1 + (53 * i) % 340 for i in range(2, n_utt)]


# name: ((N, T, duration_scale) per utterance, launch group sizes)
def _compositions():
    long_n = [340, 200, 1, 250]
    return {
        "64x1024": ([(N, 1024, 1.0) for N in _mixed_n(64)], [64]),
        "2x32768": ([(N, 32768, 16.0 if i == 0 else 1.0) for i, N in enumerate(long_n[:2])], [2]),
        "4x16384": ([(N, 16384, 16.0 if i == 0 else 1.0) for i, N in enumerate(long_n)], [4]),
        "3x21824": ([(N, 21824, 16.0 if i == 0 else 1.0) for i, N in enumerate(long_n[:3])], [3]),
        "3x21825": ([(N, 21825, 16.0 if i == 0 else 1.0) for i, N in enumerate(long_n[:3])], [2, 1]),
        "64x1025": ([(N, 1025, 1.0) for N in _mixed_n(64)], [60, 4]),
        "65x1008": ([(N, 1008, 1.0) for N in _mixed_n(65)], [64, 1]),
    }


ONE_GROUP = ("64x1024", "2x32768", "4x16384", "3x21824")


def _utterances(g, comp):
    from zerovox_cpp_amd import synth
    return [(*synth.encoder_inputs(g, 7000 + 31 * i + N, N), T, dict(duration_scale=ds)) for i, (N, T, ds) in enumerate(_compositions()[comp][0])]


@pytest.fixture(scope="module")
def stand_alone(env):
    """every utterance of every composition alone, once, in the default regime: (wav, n_frames, durations)"""
    import parity_helpers as ph
    m, g = env["m"], env["g"]
    refs = {}
    for comp, (nts, groups) in _compositions().items():
        assert ph.launch_groups([T for _, T, _ in nts]) == groups, comp
        utts = _utterances(g, comp)
        refs[comp] = (utts, [m.synthesize(*u[:4], prosody=u[4], return_durations=True) for u in utts])
    utts, ref = refs["64x1024"]
    assert any(nf == 1024 for _, nf, _ in ref), "no utterance fills its T"
    assert any(0 < nf < 256 for _, nf, _ in ref), "no utterance fills under a quarter of its T"
    assert {len(u[0]) for u in utts} >= {1, 340}
    # utterances 55 ... 63 of 64 x 1 024 start past 2^31 bytes of the last stage's tensor, whose rows pass 2^24
    bpf = ph.voc_stage_bytes_per_frame((5, 5, 4, 3), 512)[-1]
    assert [u for u in range(64) if u * 1024 * bpf >= 2 ** 31] == list(range(55, 64)) and 65536 * 300 > 2 ** 24
    print("\nframes filled: " + ", ".join(f"{c} {[nf for _, nf, _ in r]}" for c, (_, r) in refs.items() if c != "64x1025" and c != "65x1008"))
    return refs


def _check_batch(bc, ref, what):
    assert bc.n == len(ref)
    for i, ((w, nf), d, (rw, rnf, rd)) in enumerate(zip(bc.results(), bc.durations, ref)):
        assert nf == rnf and np.array_equal(d, rd), (what, i, nf, rnf)
        assert np.array_equal(w, rw), (what, i)


def _nan_fill(bc):
    for w in bc.wavs:
        w[:] = np.nan


def _group_regimes():
    from parity_helpers import BATCH_REGIME
    return (("default", {}), ("tail_groups_1", {"ZV_TAIL_GROUPS": 1}), ("tail_groups_8", {"ZV_TAIL_GROUPS": 8}), ("batch_regime", BATCH_REGIME))


@pytest.mark.parametrize("regime", _group_regimes(), ids=lambda r: r[0])
def test_launch_groups_at_their_limits_equal_stand_alone_calls(env, stand_alone, regime):
    """eager, graph capture, replay, replay after other content with the same capacities (the utterances rotated by one)"""
    from zerovox_cpp_amd import capi
    name, sw = regime
    with capi.switches(**sw):
        m = capi.Model(env["path"], 0)
        try:
            for comp, (utts, ref) in stand_alone.items():
                bc = m.prepare_batch(utts, durations=True)
                rot = m.prepare_batch(utts[1:] + utts[:1], durations=True)
                before = _free_bytes()
                t0 = time.time()
                bc.run()
                if name == "default" and comp == "64x1024":
                    print(f"\nfirst batch of 64 x 1 024 frames: {time.time() - t0:.2f} s, device memory taken {(before - _free_bytes()) / 2 ** 30:.2f} GiB")
                _check_batch(bc, ref, (name, comp, "eager"))
                m.set_graph_mode(True)
                try:
                    for step, call, r in (("capture", bc, ref), ("replay", bc, ref), ("other content", rot, ref[1:] + ref[:1]),
                                          ("replay after other content", bc, ref)):
                        _nan_fill(call)
                        call.run()
                        _check_batch(call, r, (name, comp, step))
                finally:
                    m.set_graph_mode(False)
        finally:
            m.close()


def test_launch_groups_on_two_lanes_and_refused_splits(env, stand_alone):
    """_begin / _end: the one-group compositions on two lanes in flight (the utterances and their rotation), eager and replayed;
    a batch that needs two groups is refused with ZV_ERR_ARG and leaves no lane in flight"""
    from zerovox_cpp_amd import capi
    m = capi.Model(env["path"], 0)
    try:
        for comp, (utts, ref) in stand_alone.items():
            if comp in ONE_GROUP:
                continue
            bc = m.prepare_batch(utts, durations=True)
            for lane in (0, 1):
                with pytest.raises(capi.ZvError) as ei:
                    bc.begin(lane)
                assert ei.value.status == ZV_ERR_ARG and "launch group" in str(ei.value), (comp, str(ei.value))
                with pytest.raises(capi.ZvError) as ei:
                    bc.end(lane)
                assert ei.value.status == ZV_ERR_ARG and "no batch in flight" in str(ei.value), (comp, str(ei.value))
            bc.run()                                   # the synchronous call splits it, lane 0 is free
            _check_batch(bc, ref, (comp, "synchronous after the refusal"))
        for graph in (False, True):
            m.set_graph_mode(graph)
            for comp in ONE_GROUP:
                utts, ref = stand_alone[comp]
                a, b = m.prepare_batch(utts, durations=True), m.prepare_batch(utts[1:] + utts[:1], durations=True)
                for rep in range(2 if graph else 1):
                    _nan_fill(a)
                    _nan_fill(b)
                    a.begin(0)
                    b.begin(1)
                    a.end(0)
                    b.end(1)
                    _check_batch(a, ref, (comp, "lane 0", graph, rep))
                    _check_batch(b, ref[1:] + ref[:1], (comp, "lane 1", graph, rep))
        m.set_graph_mode(False)
    finally:
        m.close()


def test_fitted_full_group(env, stand_alone):
    """64 utterances of capacity 1 024, fitted, as one group: each its stand-alone fitted call, synchronous and on a lane"""
    from zerovox_cpp_amd import capi
    utts, ref = stand_alone["64x1024"]
    fit = [env["m"].synthesize(*u[:4], prosody=u[4], return_durations=True, fitted=True) for u in utts]
    hop = env["g"].hop_size
    for (w, nf, d), (rw, rnf, rd) in zip(fit, ref):      # fitted alone: the frames the unfitted call filled, silence behind
        assert nf == rnf and np.array_equal(d, rd) and not w[nf * hop:].any()
    assert any(nf < 1024 for _, nf, _ in fit)
    m = capi.Model(env["path"], 0)
    try:
        for graph in (False, True):
            m.set_graph_mode(graph)
            bc = m.prepare_batch(utts, durations=True, fitted=True)
            for rep in range(2 if graph else 1):
                _nan_fill(bc)
                bc.run()
                _check_batch(bc, fit, ("fitted", graph, rep))
                _nan_fill(bc)
                bc.begin(1)
                bc.end(1)
                _check_batch(bc, fit, ("fitted on lane 1", graph, rep))
        m.set_graph_mode(False)
    finally:
        m.close()


# ---- 5. zv_model_reserve first -----------------------------------------------------------------------------------------------

def test_reserve_for_the_limits_then_the_tmax_calls(env, dec, chain):
    from zerovox_cpp_amd import capi
    g, Tmax = env["g"], env["Tmax"]
    m = capi.Model(env["path"], 0)
    try:
        before = _free_bytes()
        m.reserve(g.max_seq_len + 1, Tmax)           # raises unless ZV_OK
        taken = before - _free_bytes()
        print(f"\nzv_model_reserve({g.max_seq_len + 1}, {Tmax}): device memory taken {taken / 2 ** 30:.2f} GiB")
        assert np.array_equal(m.vocode(env["mel"]), env["full"])
        hid, style, mel = dec
        assert np.array_equal(m.decode(hid, style), mel)
        ids, puncts, sty, pr, wav, nf = chain
        w, n = m.synthesize(ids, puncts, sty, Tmax, prosody=pr)
        assert n == nf and np.array_equal(w, wav)
        print(f"after the three calls: {(before - _free_bytes()) / 2 ** 30:.2f} GiB (the I/O blocks are not part of the reservation)")
    finally:
        m.close()
