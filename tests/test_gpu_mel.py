"""-m gpu: mel analysis (include/zerovox_amd.h "mel analysis") at the production geometry (the "medium" synthetic checkpoint, 22 050 Hz,
hop 300, 80 channels; the two kernels depend on the hop, the lengths, the channel count and the call's parameters alone).

Every expectation is the rule restated in Python (tests/mel_rule.py): there is no tolerance anywhere, the bits must match.
  * lengths 1 and around one tile of the frames kernel;
  * a ragged batch: every utterance has the bits of its single call, whatever constant its neighbours hold;
  * the operand map of the i8 matrix instruction with two digits on both operands: impulses whose two digits differ, at seven offsets,
    read through 64 one-bin weight rows (which lane holds which row, column and digit plane, cos against sin included);
  * span edges: both pads at both ends, centres 0, hop / 2 and hop - 1; non-finite samples; a silent frame between loud ones; the three
    log modes and a floor;
  * vocode_batch(mel_wave_batch(w)) runs and equals vocode of the same rows;
  * the error messages."""
import numpy as np
import pytest

import mel_rule as MR

pytestmark = pytest.mark.gpu

_M = {}
F = np.float32
SR, HOP, NM = 22050, 300, 80
TILE = MR.tile_frames()


@pytest.fixture(scope="module")
def env(ckpt):
    from zerovox_cpp_amd import capi
    if "m" not in _M:
        path, g, tensors = ckpt("medium")
        _M.update(m=capi.Model(path, 0), g=g, W=capi.mel_design(SR, NM), path=path)
    assert _M["g"].sampling_rate == SR and _M["g"].hop_size == HOP and _M["g"].num_mels == NM
    _M["m"].set_graph_mode(False)
    yield _M["m"], _M["W"]


def teardown_module(module):
    if "m" in _M:
        _M["m"].close()
    _M.clear()


def _speech(seed, T, amp=0.3):
    rng = np.random.default_rng(seed)
    t = np.arange(T * HOP)
    f0 = rng.uniform(80, 300) / SR
    x = sum(np.sin(2 * np.pi * h * f0 * t + rng.uniform(0, 6)) / h for h in range(1, 12))
    return ((x * 0.3 + rng.standard_normal(t.size) * 0.05) * amp).astype(F)


def _same(what, have, want):
    assert have.shape == want.shape and have.dtype == F, what
    bad = np.argwhere(MR.bits(have) != MR.bits(want))
    assert bad.size == 0, (what, len(bad), bad[:6], have[tuple(bad[0])], want[tuple(bad[0])])


def _rule(x, W, p=None):
    kw = {} if p is None else dict(centre=p.centre, pad=p.pad, log=p.log, floor=p.floor)
    return MR.rule(x, x.size // HOP, HOP, W if p is None or p.weights is None else p.weights, **kw)


# ---- 1. lengths -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", [1, TILE - 1, TILE, TILE + 1])
def test_lengths_around_a_tile(env, T):
    m, W = env
    x = _speech(T, T)
    _same(("defaults", T), m.mel_wave(x), _rule(x, W))


# ---- 2. a ragged batch ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pad,Ts", [("zero", (1, TILE + 1, 2 * TILE + 3)), ("reflect", (2, TILE + 1, 2 * TILE + 3))])
def test_ragged_batch_equals_single_calls_whatever_the_neighbours_hold(env, pad, Ts):
    from zerovox_cpp_amd import capi
    m, W = env
    p = capi.MelAnalysis(pad=pad, centre=7, log="ln")
    xs = [_speech(100 + u, T) for u, T in enumerate(Ts)]
    single = [m.mel_wave(x, p) for x in xs]
    for u, x in enumerate(xs):
        _same((pad, "single", u), single[u], _rule(x, W, p))
    batch = m.mel_wave_batch(xs, p)
    for u in range(len(xs)):
        _same((pad, "batch", u), batch[u], single[u])
    # an utterance's rows do not move when its neighbours' samples do: no span crosses a segment
    for u in range(len(xs)):
        other = [x if v == u else np.full_like(x, 0.25 * (v + 1) * (-1) ** v) for v, x in enumerate(xs)]
        _same((pad, "neighbours", u), m.mel_wave_batch(other, p)[u], single[u])


# ---- 3. the operand map -----------------------------------------------------------------------------------------------------------

def test_impulses_through_one_bin_rows(env):
    """an impulse of 8 229 / 8 192 * 2^-1 quantises to 4 115 = 128 * 32 + 19: both digits non-zero and unequal.  Its spectrum is a column
    of the tables, so every one-bin row reads sqrt(C[k][t]^2 + S[k][t]^2) of one (bin, sample): a swapped lane, row, column, digit plane
    or cos / sin changes it"""
    from zerovox_cpp_amd import capi
    m, _ = env
    bins = sorted(set([0, 1, 15, 16, 17, 31, 255, 256, 257, 495, 496, 511, 512] + list(range(3, 512, 10))))[:64]
    assert len(bins) == 64 and bins[0] == 0 and 512 in bins
    W = np.zeros((NM, MR.BINS), F)
    W[np.arange(64), bins] = 1.0
    p = capi.MelAnalysis(W, centre=150, log="linear", floor=1e-30)
    amp, T = F(8229.0 / 8192.0 * 0.5), 5
    offsets = (0, 1, 163, 700, 701, 1499 - 64, 1499)
    xs = []
    for o in offsets:
        x = np.zeros(T * HOP, F)
        x[o] = amp if o % 2 else -amp
        xs.append(x)
    a, k = MR.quantise(MR.spans(xs[3], T, HOP, 150, 0)[2])
    assert k == 13 and sorted(np.abs(a[a != 0]).tolist()) == [4115] and MR.digits(np.array([4115]))[0][0] == 32
    out = m.mel_wave_batch(xs, p)
    for o, x, rows in zip(offsets, xs, out):
        want = _rule(x, W, p)
        assert (want[:, :64] > 1e-30).any() and (want[:, 64:] == F(1e-30)).all()
        _same(("impulse", o), rows, want)


# ---- 4. span edges and sample handling --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pad", ["zero", "reflect"])
@pytest.mark.parametrize("centre", [0, HOP // 2, HOP - 1])
def test_span_edges(env, pad, centre):
    from zerovox_cpp_amd import capi
    m, W = env
    T = 6
    x = _speech(31 + centre, T)
    x[:5] = [0.9, -0.8, 0.7, -0.6, 0.5]                 # loud first and last samples: a reflection that repeats the edge, or reads past it, shows
    x[-5:] = [0.5, -0.6, 0.7, -0.8, 0.9]
    p = capi.MelAnalysis(centre=centre, pad=pad, log=("log10", "ln", "linear")[centre % 3], floor=(0.0, 1e-4)[pad == "zero"])
    _same((pad, centre), m.mel_wave(x, p), _rule(x, W, p))


def test_non_finite_samples_and_a_silent_frame(env):
    from zerovox_cpp_amd import capi
    m, W = env
    rng = np.random.default_rng(9)
    specials = np.array([0x7fc00000, 0x7f800000, 0xff800000, 0x80000000], np.uint32).view(F)
    x = _speech(77, 12)
    x[rng.integers(0, x.size, 60)] = rng.choice(specials, 60)
    x[3 * HOP:3 * HOP + 1024 + 2 * HOP] = 0.0
    x[3 * HOP + 700] = F(2.0 ** -25)                     # inside frames 5 and 6, below the silence threshold: they stay silent
    x[-HOP:] *= F(5.0)                                   # an overload behind it
    for p in (None, capi.MelAnalysis(pad="reflect", log="linear", floor=0.125)):
        want = _rule(x, W, p)
        silent = [f for f in range(12) if (want[f] == want[f, 0]).all()]
        assert silent and (want[silent[0], 0] == (F(-10.0) if p is None else F(0.125)))
        _same(("specials", p), m.mel_wave(x, p), want)


# ---- 5. the round trip ------------------------------------------------------------------------------------------------------------

def test_round_trip_through_the_vocoder(env):
    from zerovox_cpp_amd import capi
    m, _ = env
    p = capi.MelAnalysis(log="ln", pad="reflect", floor=1e-5)
    xs = [_speech(200 + u, T, 0.5) for u, T in enumerate((3, 17, 40))]
    rows = m.mel_wave_batch(xs, p)
    wavs = m.vocode_batch(rows)
    for u, (r, w) in enumerate(zip(rows, wavs)):
        assert w.shape == (r.shape[0] * HOP,) and np.isfinite(w).all(), u
        assert np.array_equal(MR.bits(w), MR.bits(m.vocode(r))), u
    assert np.array_equal(MR.bits(m.resynthesize(xs[1], p)), MR.bits(wavs[1]))


def test_cli_analyzes_the_files_the_library_writes(env, tmp_path):
    """zerovox --analyze on a file zv_write_wav wrote: the rows of mel_wave on the PCM16 samples, the vocoder's waveform of them, and a
    file at another rate refused by name"""
    import os
    import subprocess
    import wave
    from zerovox_cpp_amd import capi
    m, _ = env
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zerovox.cpp_amd", "zerovox")
    x = _speech(55, 9, 0.5)
    src, rows_path, out = str(tmp_path / "in.wav"), str(tmp_path / "rows.f32"), str(tmp_path / "out.wav")
    assert m.lib.zv_write_wav(src.encode(), x.ctypes.data, x.size, SR) == 0
    with wave.open(src, "rb") as w:
        pcm = np.frombuffer(w.readframes(x.size), "<i2")
    r = subprocess.run([cli, "-m", _M["path"], "--analyze", src, "--mel-out", rows_path, "--resynth", out, "--mel-fmax", "8000", "--mel-centre", "150",
                        "--mel-pad", "zero"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = np.fromfile(rows_path, "<f4").reshape(9, NM)
    want = m.mel_wave((pcm.astype(F) / F(32768.0)), capi.MelAnalysis(fmax_hz=8000.0, centre=150, pad="zero", log="ln"))
    _same("cli rows", rows, want)
    with wave.open(out, "rb") as w:
        assert w.getnchannels() == 1 and w.getframerate() == SR and w.getnframes() == 9 * HOP
    other = str(tmp_path / "rate.wav")
    assert m.lib.zv_write_wav(other.encode(), x.ctypes.data, x.size, 16000) == 0
    r = subprocess.run([cli, "-m", _M["path"], "--analyze", other, "--mel-out", rows_path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "16000 Hz" in r.stderr and "nothing is resampled" in r.stderr, r.stderr[-500:]


# ---- 6. errors --------------------------------------------------------------------------------------------------------------------

def test_error_messages(env):
    import ctypes as C
    from zerovox_cpp_amd import capi
    m, W = env
    x = _speech(1, 4)
    bad_w = W.copy()
    bad_w[5, 100] = np.nan
    for p, words in ((capi.MelAnalysis(centre=HOP), ("mel centre = 300", "300")), (capi.MelAnalysis(pad=2), ("mel pad = 2",)),
                     (capi.MelAnalysis(log=3), ("mel log = 3",)), (capi.MelAnalysis(floor=-1.0), ("mel floor",)),
                     (capi.MelAnalysis(floor=float("inf")), ("mel floor",)), (capi.MelAnalysis(bad_w), ("mel weights",)),
                     (capi.MelAnalysis(fmin_hz=4000.0, fmax_hz=3000.0), ("mel fmin_hz",)), (capi.MelAnalysis(fmax_hz=12000.0), ("mel fmax_hz",))):
        for call, name in ((lambda: m.mel_wave(x, p), "zv_mel_wave:"), (lambda: m.mel_wave_batch([x, x], p), "zv_mel_wave_batch:")):
            with pytest.raises(capi.ZvError) as e:
                call()
            assert e.value.status == 5 and name in str(e.value) and all(w in str(e.value) for w in words), str(e.value)
    with pytest.raises(capi.ZvError) as e:
        m.mel_wave_batch([x, _speech(2, 1)], capi.MelAnalysis(pad="reflect"))
    assert "zv_mel_wave_batch: utterance 1: T = 1" in str(e.value) and "reflect" in str(e.value)
    out, st, P = np.zeros((4, NM), F), capi.MelC(), C.c_void_p * 2
    assert m.lib.zv_mel_wave(m.h, x.ctypes.data, 0, C.byref(st), out.ctypes.data) == 5 and b"zv_mel_wave: T must be > 0" in m.lib.zv_last_error()
    big = m.lib.zv_max_frames(m.h) + 1
    assert m.lib.zv_mel_wave(m.h, x.ctypes.data, big, C.byref(st), out.ctypes.data) == 5 and b"zv_mel_wave: T = " in m.lib.zv_last_error()
    assert m.lib.zv_mel_wave(m.h, x.ctypes.data, 4, None, out.ctypes.data) == 5 and b"zv_mel_wave: mel is NULL" in m.lib.zv_last_error()
    Ts = (C.c_uint32 * 2)(4, 0)
    assert m.lib.zv_mel_wave_batch(m.h, 2, P(x.ctypes.data, x.ctypes.data), Ts, C.byref(st), P(out.ctypes.data, out.ctypes.data)) == 5
    assert b"zv_mel_wave_batch: utterance 1: T must be > 0" in m.lib.zv_last_error()
    assert m.lib.zv_mel_wave_batch(m.h, 2, P(x.ctypes.data, None), (C.c_uint32 * 2)(4, 4), C.byref(st), P(out.ctypes.data, out.ctypes.data)) == 5
    assert b"zv_mel_wave_batch: utterance 1: wav is NULL" in m.lib.zv_last_error()
    with pytest.raises(ValueError):
        m.mel_wave(x, capi.MelAnalysis(np.zeros((64, 513), F)))
    with pytest.raises(TypeError):
        m.mel_wave(x, dict(pad=1))
    _same("a call after the refusals", m.mel_wave(x), _rule(x, W))
