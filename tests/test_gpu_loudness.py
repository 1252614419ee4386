"""-m gpu: loudness (include/zerovox_amd.h "loudness") on the tiny synthetic checkpoint (22 050 Hz, hop 300, so a 100 ms step is 2 205
samples; the kernels depend on the rate, the hop, the lengths and the asks alone).  This file stays at ONE rate, below 3.1 s (27
momentary blocks, 33 true-peak tiles: one round of 64 of each of the gate kernel's loops), at five utterances in one launch group and
at n_frames >= 1; other rates, longer spans, wider batches, n_frames = 0, a batch across a launch group's end and the ceiling's
round-down step are tests/test_gpu_loudness_shapes.py.

Every expectation is the rule restated in numpy (tests/loudness_rule.py) on the design the library itself returns (the design is data to
the kernels): there is no tolerance anywhere but in the last test, the bits must match — every field of the result and every sample.
  * the single call with N = n_frames * hop on both sides of four steps (29 / 30 frames: no block / the first block) and of thirty steps
    (220 / 221 frames: no short-term block / the first), at N a whole number of chunks (64 frames = 75 chunks) and not, always with
    n_frames < T: the tail behind N is scaled and not measured.  221 frames are 259 chunks and 33 true-peak tiles: five workgroups of the
    chunk passes and 33 of the peak pass over one utterance (the gate pass stays within its first round);
  * a ragged batch of five with an utterance below four steps, a silent one and one with a NaN and an infinity, under mixed asks (none,
    a target, a ceiling, both with the ceiling winning): every utterance has the bits of its single call;
  * the same batch after zv_debug_poison of lane 0 with both bytes;
  * the ceiling's promise recomputed from the result; out = NULL changes nothing in the result;
  * a synthesised waveform metered, brought to -16 LUFS and metered again;
  * the command line: --lufs / --true-peak-dbtp on a synthesis run, --loudness on the file it wrote."""
import math

import numpy as np
import pytest

import loudness_rule as LR

pytestmark = pytest.mark.gpu

_M = {}
F = np.float32
SR, HOP = 22050, 300
STEP = 2205


@pytest.fixture(scope="module")
def env(ckpt):
    from zerovox_cpp_amd import capi
    if "m" not in _M:
        path, g, tensors = ckpt("tiny")
        _M.update(m=capi.Model(path, 0), g=g, D=capi.loudness_design(SR), path=path)
    assert _M["g"].sampling_rate == SR and _M["g"].hop_size == HOP and _M["D"].step == STEP
    _M["m"].set_graph_mode(False)
    yield _M["m"], _M["D"]


def teardown_module(module):
    if "m" in _M:
        _M["m"].close()
    _M.clear()


def _speech(seed, T, amp=0.1):
    """harmonics and noise under a slow swell, so that blocks differ and the relative gate has something to drop"""
    rng = np.random.default_rng(seed)
    t = np.arange(T * HOP)
    f0 = rng.uniform(90, 250) / SR
    x = sum(np.sin(2 * np.pi * h * f0 * t + rng.uniform(0, 6)) / h for h in range(1, 9))
    swell = 0.02 + np.abs(np.sin(2 * np.pi * t / SR * rng.uniform(0.4, 0.9)))
    return ((x * 0.4 + rng.standard_normal(t.size) * 0.05) * swell * amp).astype(F)


def _ask(q):
    """a capi.Loudness (or None) as the rule's ask"""
    if q is None:
        return LR.ask()
    s = q.struct
    return LR.ask(s.gain, s.target_lufs, s.true_peak_ceiling, s.flags)


def _same(what, got, want):
    (res, out), (wres, wout) = got, want
    assert LR.key(res) == LR.key(wres), (what, res, wres)
    if wout is None:
        assert out is None, what
    else:
        assert out.shape == wout.shape and out.dtype == F, what
        bad = np.flatnonzero(out.view(np.uint32) != wout.view(np.uint32))
        assert bad.size == 0, (what, bad.size, bad[:6], out[bad[0]], wout[bad[0]])


# ---- 1. the single call ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nf", [29, 30, 64, 220, 221])
def test_single_call_around_the_block_edges(env, nf):
    from zerovox_cpp_amd import capi
    m, D = env
    T = nf + 3
    x = _speech(nf, T)
    N = nf * HOP
    assert (N // STEP >= 4) == (nf >= 30) and (N // STEP >= 30) == (nf >= 221) and (N % 256 == 0) == (nf == 64)
    for q in (None, capi.Loudness.from_lufs(-16.0, true_peak_dbtp=-1.0), capi.Loudness(0.5, -23.0, None)):
        want = LR.rule(D, x, N, _ask(q))
        got = m.loudness_wave(x, q, n_frames=nf)
        _same((nf, q), got, want)
        assert got[0].blocks == max(N // STEP - 3, 0)
        if q is not None and got[0].blocks_gated:
            assert got[0].gain != F(q.gain)                       # the target moved the gain
    # the tail behind N is scaled, not measured: another tail, the same result
    y = x.copy()
    y[N:] = F(0.9)
    a, b = m.loudness_wave(x, None, n_frames=nf), m.loudness_wave(y, None, n_frames=nf)
    assert LR.key(a[0]) == LR.key(b[0]) and (b[1][N:] == F(0.9) * a[0].gain).all()
    # n_frames beyond T counts as T
    _same((nf, "beyond"), m.loudness_wave(x, None, n_frames=T + 9), LR.rule(D, x, T * HOP, LR.ask()))


# ---- 2. a ragged batch ------------------------------------------------------------------------------------------------------------------

def _batch():
    from zerovox_cpp_amd import capi
    xs = [_speech(31, 20), np.zeros(40 * HOP, F), _speech(33, 50), _speech(34, 230, 0.5), _speech(35, 75)]
    xs[2][1234] = np.nan
    xs[2][7000] = np.inf
    xs[2][7001] = -np.inf
    xs[4][:35 * HOP] *= F(0.05)                                                 # a quiet half: the relative gate drops its blocks
    nfs = [20, 40, 47, 226, 75]
    asks = [None, capi.Loudness(1.0, -16.0, None), capi.Loudness(2.0, None, 0.25), capi.Loudness(1.0, -6.0, 0.125), capi.Loudness(1.0, -20.0, 1.0)]
    return xs, nfs, asks


def test_ragged_batch_equals_single_calls_and_the_rule(env):
    m, D = env
    xs, nfs, asks = _batch()
    want = [LR.rule(D, x, nf * HOP, _ask(q)) for x, nf, q in zip(xs, nfs, asks)]
    assert want[0][0].blocks == 0 and want[1][0].blocks > 0 and want[1][0].blocks_absolute == 0 and math.isinf(want[1][0].integrated_lufs)
    assert 0 < want[4][0].blocks_gated < want[4][0].blocks_absolute == want[4][0].blocks
    assert want[1][0].gain == F(1.0)                                            # a target does nothing without a gated block
    r3 = want[3][0]
    assert r3.gain < F(math.sqrt(_ask(asks[3]).zt / r3.integrated_ms))          # the ceiling won
    single = [m.loudness_wave(x, q, n_frames=nf) for x, nf, q in zip(xs, nfs, asks)]
    for u in range(5):
        _same(("single", u), single[u], want[u])
    batch = m.loudness_wave_batch(xs, asks, nfs)
    for u in range(5):
        _same(("batch", u), batch[u], single[u])
    # asks == NULL and n_frames == NULL: the identity over the whole capacity; a NULL entry of out meters only
    plain = m.loudness_wave_batch(xs, None, None, apply=[True, False, True, False, True])
    for u in range(5):
        _same(("plain", u), plain[u], LR.rule(D, xs[u], xs[u].size, LR.ask(), out=u % 2 == 0))


def test_poisoned_lane_leaves_the_bits_unchanged(env):
    m, D = env
    xs, nfs, asks = _batch()
    first = m.loudness_wave_batch(xs, asks, nfs)
    for byte in (0x00, 0xFF):
        m.poison(byte, 0)
        for u, got in enumerate(m.loudness_wave_batch(xs, asks, nfs)):
            _same(("poison", byte, u), got, first[u])
        m.poison(byte, 0)
        _same(("poison, single", byte), m.loudness_wave(xs[3], asks[3], n_frames=nfs[3]), first[3])


# ---- 3. the promises ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ceiling", [0.125, 0.3, 0.70710677, 1.0])
def test_the_scaled_true_peak_stays_under_the_ceiling(env, ceiling):
    from zerovox_cpp_amd import capi
    m, D = env
    for seed in range(4):
        x = _speech(50 + seed, 60, 0.6)
        q = capi.Loudness(3.0, -10.0, ceiling)
        res, out = m.loudness_wave(x, q)
        _same((ceiling, seed), (res, out), LR.rule(D, x, x.size, _ask(q)))
        assert F(float(res.gain) * res.true_peak) <= F(ceiling), (ceiling, seed, res)
        assert np.abs(out).max() <= F(ceiling)


def test_meter_only_changes_nothing_in_the_result(env):
    from zerovox_cpp_amd import capi
    m, D = env
    x = _speech(60, 64)
    q = capi.Loudness.from_lufs(-19.0, true_peak_dbtp=-3.0)
    a, b = m.loudness_wave(x, q), m.loudness_wave(x, q, apply=False)
    assert b[1] is None and LR.key(a[0]) == LR.key(b[0])
    _same("meter only", b, LR.rule(D, x, x.size, _ask(q), out=False))


# ---- 4. a synthesised waveform to -16 LUFS ------------------------------------------------------------------------------------------------

def test_a_synthesised_waveform_reaches_its_target(env):
    from zerovox_cpp_amd import capi, synth
    m, D = env
    ids, puncts, style = synth.encoder_inputs(_M["g"], 9, 12)
    T = 64
    wav, nf = m.synthesize(ids, puncts, style, T)[:2]
    q = capi.Loudness.from_lufs(-16.0, true_peak_dbtp=-1.0)
    first, out = m.loudness_wave(wav, q, n_frames=nf)
    print("synthesised:", nf, "frames,", first)
    assert first.blocks_gated > 0 and np.isfinite(first.integrated_lufs)
    second, _ = m.loudness_wave(out, None, n_frames=nf, apply=False)
    print("normalised:", second)
    by_target = F(math.sqrt(_ask(q).zt / first.integrated_ms))
    if first.gain == by_target:
        assert abs(float(second.integrated_lufs) + 16.0) <= 0.01, (first, second)
    else:                                                                       # the ceiling applied: quieter than the target, under -1 dBTP
        assert first.gain < by_target and float(second.integrated_lufs) < -16.0
        assert float(second.true_peak_dbtp) <= -1.0 + 1e-3


# ---- 5. the command line ------------------------------------------------------------------------------------------------------------------

def test_command_line_normalises_and_meters(env, tmp_path):
    import os
    import re
    import subprocess
    import wave
    from zerovox_cpp_amd import capi, synth
    m, D = env
    g = _M["g"]
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zerovox.cpp_amd", "zerovox")
    ids, puncts, _ = synth.encoder_inputs(g, 9, 12)
    out, utt = str(tmp_path / "out.wav"), str(tmp_path / "utt.txt")
    open(utt, "w").write(" ".join(map(str, ids)) + "\n" + " ".join(map(str, puncts)) + "\n0\n")
    r = subprocess.run([cli, "-m", _M["path"], "-u", utt, "-o", out, "--fit", "--lufs", "-16", "--true-peak-dbtp", "-1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    wav, nf = m.synthesize(ids, puncts, np.zeros(g.E, F), g.max_seq_len, fitted=True)[:2]
    want, scaled = m.loudness_wave(wav[:nf * HOP], capi.Loudness.from_lufs(-16.0, true_peak_dbtp=-1.0))
    got = re.search(r"loudness before the gain: integrated (\S+) LUFS, .* true peak (\S+) dBTP .* blocks (\d+) / (\d+) / (\d+), gain (\S+)", r.stdout)
    assert got, r.stdout
    assert got.group(1) == "%.2f" % want.integrated_lufs and got.group(2) == "%.2f" % want.true_peak_dbtp and got.group(6) == "%.6f" % want.gain
    assert tuple(map(int, got.group(3, 4, 5))) == (want.blocks, want.blocks_absolute, want.blocks_gated)
    with wave.open(out, "rb") as w:
        assert w.getnchannels() == 1 and w.getframerate() == SR and w.getnframes() == nf * HOP
        pcm = np.frombuffer(w.readframes(nf * HOP), "<i2").astype(F) / F(32768.0)
    assert np.abs(pcm - np.clip(scaled, -1, 1)).max() <= 1.0 / 32768.0 + 1e-7                  # PCM16 of the scaled waveform
    r = subprocess.run([cli, "-m", _M["path"], "--loudness", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    again = m.loudness_wave(pcm, None, apply=False)[0]
    got = re.search(r"integrated (\S+) LUFS, momentary max (\S+) LUFS, short-term max (\S+) LUFS, true peak (\S+) dBTP", r.stdout)
    assert got and got.groups() == tuple("%.2f" % v for v in (again.integrated_lufs, again.momentary_max_lufs, again.short_term_max_lufs,
                                                               again.true_peak_dbtp)), (r.stdout, again)
