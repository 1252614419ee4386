"""-m gpu: the waveform filter (include/zerovox_amd.h "waveform filter") at the production geometry (the "medium" synthetic checkpoint,
22 050 Hz, hop 300; the kernel depends on the hop, the lengths and the taps alone).

filter_kernel runs behind the vocoder's last convolution and ahead of the envelope, the volume passes and every meter, so every
expectation is the rule restated in numpy (tests/filter_rule.py) applied to the waveform of the call WITHOUT the filter: there is no
tolerance anywhere, the bits must match.
  * zv_filter_wave against the rule: capacities of 1, 2 and 5 frames (511 taps are longer than the signal), the lengths on either
    side of one and of two of the kernel's tiles (the hop is 300 and the tile 2 048, so no T * hop equals it), every length class of
    non-symmetric taps, impulses that read the taps back, special values, out == wav;
  * zv_synthesize_filter = the rule on the plain call's waveform, fitted and unfitted, at every speech length of a small utterance;
    the fitted tail is zero and the fitted result is the unfitted filtered call at T = n_frames;
  * the order: filter, envelope, loudness target and peak ceiling in one call, and the meters on what is returned;
  * nothing else moves: NULL, all-NULL structs and NULL taps with a nonsense count give the _bands call's bits; voc_filter appears in
    the profile once and only with a request, in its place;
  * a ragged batch with a tap count per utterance, unfiltered utterances and loud neighbours (eager, graph capture, replay on poisoned
    lanes, new taps on replay, two lanes in flight) = the stand-alone calls; tail groups;
  * validation messages; the CLI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bands_rule as BR
import contour_rule as CR
import envelope_rule as ER
import filter_rule as FR
import level_rule as LR
import pitch_rule as PR

pytestmark = pytest.mark.gpu

_M = {}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SR = 22050
LENGTHS = (1, 3, 33, 255, 511)
SPECIALS = np.array([0x7fc00000, 0x7f800000, 0xff800000, 0x80000000, 0x00000001, 0x807fffff, 0x7f7fffff, 0xffc12345], np.uint32).view(F)


@pytest.fixture(scope="module")
def env(ckpt):
    from zerovox_cpp_amd import capi
    if "m" not in _M:
        path, g, tensors = ckpt("medium")
        _M.update(m=capi.Model(path, 0), g=g, t=tensors, path=path)
    assert _M["g"].sampling_rate == SR and _M["g"].hop_size == 300
    _M["m"].set_graph_mode(False)
    yield _M["m"], _M["g"], _M["t"]
    _M["m"].set_graph_mode(False)


def teardown_module(module):
    if "m" in _M:
        _M["m"].close()
    _M.clear()


def _utt(g, seed, N):
    from zerovox_cpp_amd import synth
    return synth.encoder_inputs(g, seed, N)


def _taps(seed, L, scale=1.0):
    """non-symmetric"""
    return (np.random.default_rng(1000 + seed).standard_normal(L) * scale / np.sqrt(L)).astype(F)


def _gains(N, seed):
    g = np.random.default_rng(seed).random(N) * 4.0
    g[::5] = 0.0
    g[3::7] = 16.0
    return g.astype(F)


def _eq(what, got, want):
    bad = np.flatnonzero(FR.bits(got) != FR.bits(want))
    assert bad.size == 0, (what, bad.size, bad[:8], np.asarray(got)[bad[:4]], np.asarray(want)[bad[:4]])


# ---- 1. zv_filter_wave against the rule -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", LENGTHS)
def test_filter_wave_equals_the_rule(env, L):
    m, g, _ = env
    hop = g.hop_size
    below, above = FR.TILE // hop, FR.TILE // hop + 1                # 1 800 and 2 100 samples around the 2 048 of one tile
    assert below * hop < FR.TILE < above * hop and (2 * FR.TILE // hop) * hop < 2 * FR.TILE
    rng = np.random.default_rng(L)
    h = _taps(L, L)
    for T in (1, 2, 5, below, above, 2 * FR.TILE // hop, 2 * FR.TILE // hop + 1):
        x = (rng.standard_normal(T * hop) * 0.3).astype(F)
        _eq((L, T), m.filter_wave(x, h), FR.apply(x, h))
    # special values: NaN and the infinities are +0.0 to their neighbours, -0.0 and subnormals are themselves
    x = (rng.standard_normal(above * hop) * 0.3).astype(F)
    x[rng.choice(x.size, 4 * SPECIALS.size, replace=False)] = np.tile(SPECIALS, 4)
    x[:2], x[-2:] = SPECIALS[:2], SPECIALS[2:4]
    _eq((L, "specials"), m.filter_wave(x, h), FR.apply(x, h))
    # out == wav
    want, buf = FR.apply(x, h), x.copy()
    from zerovox_cpp_amd import capi
    st = capi.Filter(h).struct                                   # (the binding allocates its own output: the library is called directly)
    m._chk(m.lib.zv_filter_wave(m.h, buf.ctypes.data, above, C.byref(st), buf.ctypes.data))
    _eq((L, "in place"), buf, want)
    # no taps: a copy, bit for bit
    st = capi.FilterC(None, 12)
    out = np.zeros_like(x)
    m._chk(m.lib.zv_filter_wave(m.h, x.ctypes.data, above, C.byref(st), out.ctypes.data))
    _eq((L, "copy"), out, x)


def test_impulses_read_the_taps_back_and_sums_overflow(env):
    m, g, _ = env
    hop, T = g.hop_size, 8
    S = T * hop
    for L in (3, 33, 255, 511):
        h, c = _taps(50 + L, L), (L - 1) // 2
        for at in (0, 1, c - 1, c, S - 1):
            x = np.zeros(S, F)
            x[at] = 1.0
            y = m.filter_wave(x, h)
            want = np.zeros(S, F)
            lo, hi = max(at - c, 0), min(at + c + 1, S)
            want[lo:hi] = h[lo - at + c: hi - at + c]               # y[n] = h[n - at + c]: the centre tap lands on the impulse
            _eq((L, at), y, want)
            _eq((L, at, "rule"), y, FR.apply(x, h))
    # L = 1, h = {1}: x with -0.0 as +0.0 and the non-finite samples as +0.0
    x = np.tile(SPECIALS, S // SPECIALS.size)
    y = m.filter_wave(x, np.ones(1, F))
    _eq("identity", y, np.where(np.isfinite(x), x, F(0)) + F(0))
    # a result beyond the f32 range becomes infinite by the conversion; tiny ones become subnormal
    big = np.full(S, 3.0e38, F)
    big[::7] = -3.0e38
    y = m.filter_wave(big, np.full(33, 1.5, F))
    assert np.isinf(y).any()
    _eq("overflow", y, FR.apply(big, np.full(33, 1.5, F)))
    tiny, ht = np.full(S, 1.0e-30, F), np.array([1.0e-10, 3.0e-12, -1.0e-10], F)
    y = m.filter_wave(tiny, ht)
    assert ((np.abs(y) < np.finfo(F).tiny) & (y != 0)).any()
    _eq("subnormal", y, FR.apply(tiny, ht))


# ---- 2. zv_synthesize_filter ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fitted", [False, True])
def test_every_speech_length_of_a_small_utterance(env, fitted):
    m, g, _ = env
    N, T, hop = 16, 64, g.hop_size
    ids, puncts, style = _utt(g, 21, N)
    h = _taps(3, 33)
    for nf in range(0, T + 1):
        kw = dict(phonemes=dict(duration_frames=np.zeros(N, np.int32))) if nf == 0 else dict(target_frames=nf)
        plain, n0 = m.synthesize(ids, puncts, style, T, fitted=fitted, **kw)
        w, n = m.synthesize(ids, puncts, style, T, fitted=fitted, filter=h, **kw)
        assert n == n0 == nf
        _eq((fitted, nf), w, FR.apply(plain, h, nf * hop if fitted else T * hop))
        if fitted:
            assert not FR.bits(w[nf * hop:]).any(), nf
            if nf in (1, 2, 7, 33, 64):                          # the fitted promise: the unfitted filtered call at T = nf, then zeros
                u, _ = m.synthesize(ids, puncts, style, nf, target_frames=nf, filter=h)
                _eq((nf, "T = nf"), w[:nf * hop], u)


@pytest.mark.parametrize("L", [1, 255, 511])
def test_synthesize_filter_equals_the_rule_on_the_plain_calls_wave(env, L):
    m, g, _ = env
    N, T, hop = 30, 150, g.hop_size
    ids, puncts, style = _utt(g, 22, N)
    h = _taps(4, L)
    for fitted in (False, True):
        plain, nf = m.synthesize(ids, puncts, style, T, fitted=fitted, target_frames=101)
        for graph in (False, True, True):
            m.set_graph_mode(graph)
            w, n = m.synthesize(ids, puncts, style, T, fitted=fitted, target_frames=101, filter=h)
            assert n == nf == 101
            _eq((L, fitted, graph), w, FR.apply(plain, h, nf * hop if fitted else T * hop))
        m.set_graph_mode(False)


# ---- 3. the order -----------------------------------------------------------------------------------------------------------------

def test_filter_then_envelope_then_volume_then_the_meters(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    N, T, hop = 40, 100, g.hop_size
    ids, puncts, style = _utt(g, 61, N)
    h = capi.Filter.from_band_gains_db([6.0] * 8 + [12.0] * 8).taps              # a boost: the ceiling must hold behind it
    e = capi.Envelope(_gains(N, 7), 2, 5 * hop, 7 * hop + 3)
    vol = capi.Volume(0.8, 0.07, 0.5)
    for fitted in (False, True):
        plain, nf0, dur0 = m.synthesize(ids, puncts, style, T, fitted=fitted, target_frames=80, return_durations=True)
        x = FR.apply(plain, h, 80 * hop if fitted else T * hop)
        r = ER.rule(x, dur0, T, hop, ER.as_tuple(e))
        v = LR.rule(r["out"], r["nf"] * hop, (vol.gain, vol.target_rms, vol.peak_ceiling))
        for graph in (False, True, True):
            m.set_graph_mode(graph)
            w, n, dur, lv, c, p, b = m.synthesize(ids, puncts, style, T, fitted=fitted, target_frames=80, envelope=e, volume=vol, filter=h,
                                                  return_durations=True, return_levels=True, return_contour=True, return_pitch=True, return_bands=True)
            assert n == 80 and dur.tolist() == dur0.tolist()
            _eq((fitted, graph, "wave"), w, v["out"])
            assert LR.level_bits(lv) == LR.level_bits(v["level"])
            assert np.abs(w[np.isfinite(w)]).max() <= F(0.5)
            if not graph:
                cr, pr, br = CR.rule(w, T, hop, dur), PR.rule(w, T, SR, hop, dur), BR.rule(w, T, hop, dur)
            for got, want in ((c.frames, cr["frames"]), (c.phonemes, cr["phonemes"]), (p.frames, pr["frames"]), (p.phonemes, pr["phonemes"]),
                              (b.frames, br["frames"]), (b.phonemes, br["phonemes"])):
                assert np.array_equal(FR.bits(got), FR.bits(want)), (fitted, graph)
        m.set_graph_mode(False)


# ---- 4. nothing else moves ----------------------------------------------------------------------------------------------------------

def test_no_filter_gives_the_bands_calls_bits(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    N, T, hop = 24, 60, g.hop_size
    ids, puncts, style = _utt(g, 31, N)
    e, vol = capi.Envelope(_gains(N, 2), 1, 30, 40), capi.Volume(1.1, 0.06, 0.45)
    kw = dict(target_frames=50, envelope=e, volume=vol, return_levels=True, return_bands=True)
    for graph in (False, True):
        m.set_graph_mode(graph)
        w0, n0, lv0, b0 = m.synthesize(ids, puncts, style, T, **kw)
        w0 = w0.copy()
        for flt in (capi.Filter(None), capi.Filter(None, n_taps=1 << 30), capi.Filter(None, n_taps=4)):
            w, n, lv, b = m.synthesize(ids, puncts, style, T, filter=flt, **kw)
            assert n == n0 and LR.level_bits(lv) == LR.level_bits(lv0)
            _eq((graph, flt), w, w0)
            assert np.array_equal(FR.bits(b.frames), FR.bits(b0.frames)) and np.array_equal(FR.bits(b.phonemes), FR.bits(b0.phonemes))
    m.set_graph_mode(False)
    # the _filter entry points with filter == NULL, single and batch
    plain = m.synthesize(ids, puncts, style, T)[0].copy()
    wav, nf = np.full(T * hop, 7.0, F), C.c_uint32(0)
    a, b_, c = np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(puncts, np.int32), np.ascontiguousarray(style, F)
    m._chk(m.lib.zv_synthesize_filter(m.h, a.ctypes.data, b_.ctypes.data, c.ctypes.data, N, T, wav.ctypes.data, C.byref(nf), None, None, None, 0, 0,
                                      None, None, None, None, None, None, None))
    _eq("single NULL", wav, plain)
    utts = [(ids, puncts, style, T), (*_utt(g, 32, 9), 33)]
    plains = [w.copy() for w, _ in m.synthesize_batch(utts)]
    null = m.prepare_batch(utts)
    args = (m.h, null.n, null.ids_p, null.pun_p, null.sty_p, null.Ns, null.Ts, null.wav_p, null.nf)
    bad = (capi.FilterC * 2)(capi.FilterC(None, 99), capi.FilterC(None, 2))
    for flt in (None, (capi.FilterC * 2)(), bad):
        for w in null.wavs:
            w.fill(7.0)
        m._chk(m.lib.zv_synthesize_batch_filter(*args, None, None, None, None, 0, None, None, None, None, None, None, flt))
        for i, (w, n) in enumerate(null.results()):
            _eq(("batch", i), w, plains[i])


def test_the_launch_appears_only_with_a_request_and_in_its_place(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    N, T = 30, 150
    ids, puncts, style = _utt(g, 42, N)
    kw = dict(target_frames=100, volume=capi.Volume(1.0, 0.1, 0.5), envelope=capi.Envelope(_gains(N, 6), 1, 10, 10), return_contour=True,
              return_pitch=True, return_bands=True)
    for fitted in (False, True):
        m.profile_begin()
        m.synthesize(ids, puncts, style, T, fitted=fitted, **kw)
        without = {s["name"]: s for s in m.profile_end()}
        m.profile_begin()
        m.synthesize(ids, puncts, style, T, fitted=fitted, filter=capi.Filter(None, n_taps=7), **kw)
        none = {s["name"]: s for s in m.profile_end()}
        m.profile_begin()
        m.synthesize(ids, puncts, style, T, fitted=fitted, filter=_taps(1, 255), **kw)
        with_f = {s["name"]: s for s in m.profile_end()}
        assert "voc_filter" not in without and list(none) == list(without)
        assert set(with_f) == set(without) | {"voc_filter"}
        for k in without:
            assert with_f[k]["launches"] == without[k]["launches"] == none[k]["launches"], k
        names = list(with_f)
        before = "voc_zero_tail" if fitted else ("voc_run_fill" if "voc_run_fill" in names else "voc_output_conv")
        assert names[names.index("voc_filter") - 1] == before and names[names.index("voc_filter") + 1] == "voc_env_knots", names
        assert with_f["voc_filter"]["launches"] == 1


# ---- 5. batches ---------------------------------------------------------------------------------------------------------------------

def _ragged(g):
    # (N, T, target frames): a short quiet utterance between loud neighbours, capacities that are no multiple of anything
    nt = [(40, 150, 101), (30, 140, 140), (3, 9, 2), (60, 130, 130), (1, 11, 5), (100, 160, 97)]
    return [(*_utt(g, 500 + i, N), T, None, None, tf) for i, (N, T, tf) in enumerate(nt)]


def _filters():
    return [_taps(10, 255), _taps(11, 511, 40.0), _taps(12, 33, 1e-3), _taps(13, 3, 40.0), None, _taps(15, 1)]


def _volumes():
    from zerovox_cpp_amd import capi
    return [None, capi.Volume(30.0, 0.0, 0.0), capi.Volume(1e-3, 0.0, 0.0), capi.Volume(30.0, 0.0, 0.0), None, None]


@pytest.mark.parametrize("fitted", [False, True])
def test_ragged_batch_replay_and_poison(env, fitted):
    m, g, _ = env
    hop = g.hop_size
    utts, flts = _ragged(g), _filters()
    m.set_graph_mode(False)
    plains = [(w.copy(), n) for w, n in m.synthesize_batch(utts, fitted=fitted)]
    alone = [m.synthesize(*u[:4], fitted=fitted, target_frames=u[6], filter=flts[i])[0].copy() for i, u in enumerate(utts)]
    for i, (w, n) in enumerate(plains):                          # the stand-alone calls are the rule; the batches are held to them
        _eq(("alone", i), alone[i], FR.apply(w, flts[i], n * hop if fitted else None))
    _eq("unfiltered", alone[4], plains[4][0])
    bc = m.prepare_batch(utts, fitted=fitted, filter=flts)
    steps = [("eager", False, None), ("graph capture", True, None), ("graph replay on a lane poisoned with 0xFF", True, 0xFF),
             ("graph replay on a lane poisoned with 0x00", True, 0x00)]
    for what, graph, poison in steps:
        m.set_graph_mode(graph)
        if poison is not None:
            m.poison(poison)
        for w in bc.wavs:
            w.fill(7.0)
        bc.run()
        for i, (w, n) in enumerate(bc.results()):
            assert n == plains[i][1]
            _eq((what, i), w, alone[i])
    # a replay with new taps and new tap counts picks them up: the filters move one utterance on
    moved = flts[1:] + flts[:1]
    want = [FR.apply(w, moved[i], n * hop if fitted else None) for i, (w, n) in enumerate(plains)]
    for i, f in enumerate(moved):
        bc.set_filter(i, f)
    m.poison(0xFF)
    bc.run()
    for i, (w, n) in enumerate(bc.results()):
        _eq(("new taps", i), w, want[i])
    bc.begin(2)
    bc.end(2)
    for i, (w, n) in enumerate(bc.results()):
        _eq(("lane 2", i), w, want[i])
    # loud and quiet neighbours through the whole chain: volume behind the filter, per utterance as alone
    vols = _volumes()
    m.set_graph_mode(False)
    loud = m.synthesize_batch(utts, fitted=fitted, volume=vols, filter=flts)
    for i, u in enumerate(utts):
        _eq(("loud", i), loud[i][0], m.synthesize(*u[:4], fitted=fitted, target_frames=u[6], volume=vols[i], filter=flts[i])[0])
    # the plain batch next to it keeps its bits
    for i, (w, n) in enumerate(m.synthesize_batch(utts, fitted=fitted)):
        _eq(("plain", i), w, plains[i][0])


def test_two_lanes_in_flight(env):
    m, g, _ = env
    hop = g.hop_size
    sets = [[(*_utt(g, 600 + 10 * k + i, 20 + 5 * i), 40 + 10 * k + 9 * i, None, None, 20 + 10 * k + 7 * i) for i in range(3)] for k in range(3)]
    flts = [[_taps(20, 255), None, _taps(21, 33)], [None, _taps(22, 511), _taps(23, 1)], [_taps(24, 3), _taps(25, 255), None]]
    m.set_graph_mode(False)
    want = []
    for k, utts in enumerate(sets):
        want.append([FR.apply(w, flts[k][i]) for i, (w, n) in enumerate(m.synthesize_batch(utts))])
    batches = [m.prepare_batch(utts, filter=flts[k]) for k, utts in enumerate(sets)]
    for graph in (False, True):
        m.set_graph_mode(graph)
        for bc in batches:
            for w in bc.wavs:
                w.fill(7.0)
        for k, bc in enumerate(batches):                 # _begin k, _end k - 1
            bc.begin(k % 2)
            if k:
                batches[k - 1].end((k - 1) % 2)
        batches[-1].end((len(batches) - 1) % 2)
        for k, bc in enumerate(batches):
            for i, (w, n) in enumerate(bc.results()):
                _eq((graph, k, i), w, want[k][i])
    m.set_graph_mode(False)


def test_batch_split_into_tail_groups(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    hop, T = g.hop_size, 900                                  # 16 utterances: 2 and 8 groups are different schedules (two utterances per group at least)
    tfs = [900, 500, 250, 37, 899, 1, 640, 333, 65, 700, 31, 32, 33, 450, 820, 128]
    utts = [(*_utt(g, 700 + i, 40 + 9 * i), T, None, None, tf) for i, tf in enumerate(tfs)]
    assert len(utts) * T * hop * 4 >= 16 << 20 and len(utts) // 2 >= 8
    flts = [[_taps(30 + i, 255), None, _taps(30 + i, 511), _taps(30 + i, 33)][i % 4] for i in range(len(utts))]
    m.set_graph_mode(False)
    with capi.switches(ZV_TAIL_GROUPS=1):
        plains = [w.copy() for w, _ in m.synthesize_batch(utts, fitted=True)]
        bc = m.prepare_batch(utts, fitted=True, filter=flts)
        bc.run()
        assert [n for _, n in bc.results()] == tfs
        for i in (1, 2, 7):                                   # two filtered utterances and an unfiltered one of the one-group run against the rule
            _eq(("one group", i), bc.results()[i][0], FR.apply(plains[i], flts[i], tfs[i] * hop))
        one = [w.copy() for w, _ in bc.results()]
    for groups in (2, 8):
        with capi.switches(ZV_TAIL_GROUPS=groups):
            for graph in (False, True):
                m.set_graph_mode(graph)
                bc = m.prepare_batch(utts, fitted=True, filter=flts)
                for rep in range(2 if graph else 1):
                    m.poison(0x00 if rep else 0xFF)
                    for w in bc.wavs:
                        w.fill(7.0)
                    bc.run()
                    for i, (w, n) in enumerate(bc.results()):
                        assert n == tfs[i] and np.array_equal(FR.bits(w), FR.bits(one[i])), (groups, graph, rep, i)
            m.set_graph_mode(False)


# ---- 6. validation; the CLI -----------------------------------------------------------------------------------------------------------

def test_validation_names_the_entry_point_the_utterance_and_the_field(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    utts = _ragged(g)[:2]
    bad_count = [capi.Filter(np.ones(4, F)), capi.Filter(np.ones(8, F), n_taps=0), capi.Filter(np.ones(600, F), n_taps=513)]
    nan, inf = np.ones(33, F), np.ones(3, F)
    nan[20], inf[0] = np.nan, -np.inf
    for flt, field in [(f, "n_taps") for f in bad_count] + [(capi.Filter(nan), "taps"), (capi.Filter(inf), "taps")]:
        with pytest.raises(capi.ZvError, match=r"zv_synthesize_batch_filter: utterance 1: filter %s" % field):
            m.synthesize_batch(utts, filter=[None, flt])
        with pytest.raises(capi.ZvError, match=r"zv_synthesize_filter: utterance 0: filter %s" % field):
            m.synthesize(*utts[0][:4], filter=flt)
        with pytest.raises(capi.ZvError, match=r"zv_filter_wave: filter %s" % field):
            m.filter_wave(np.zeros(g.hop_size, F), flt)
        bc = m.prepare_batch(utts, filter=[flt, None])
        with pytest.raises(capi.ZvError, match=r"zv_synthesize_batch_begin_filter: utterance 0: filter %s" % field):
            bc.begin(1)
    with pytest.raises(capi.ZvError, match="zv_filter_wave: T = "):
        m.filter_wave(np.zeros(g.hop_size * (m.max_frames() + 1), F), [1.0])
    # a refused call has enqueued nothing: the next one is as ever
    w, n = m.synthesize(*utts[0][:4], filter=[1.0])
    _eq("after", w, FR.apply(m.synthesize(*utts[0][:4])[0], [1.0]))


def test_cli_round_trip(env, tmp_path):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    N, hop = 40, g.hop_size
    ids, puncts, style = _utt(g, 71, N)
    utt = tmp_path / "utt.txt"
    utt.write_text(" ".join(map(str, ids.tolist())) + "\n" + " ".join(map(str, puncts.tolist())) + "\n" +
                   " ".join(repr(float(x)) for x in style.tolist()) + "\n")
    out = tmp_path / "filter.wav"
    cli = os.path.join(ROOT, "zerovox.cpp_amd", "zerovox")
    base = [cli, "-m", _M["path"], "-u", str(utt), "-o", str(out), "--fit", "--target-frames", "123", "--peak-dbfs", "-3"]
    vol = capi.Volume.from_db(peak_dbfs=-3)

    def pcm_of(w, nf):
        return np.clip(np.rint(w[:nf * hop] * F(32767.0)), -32768, 32767).astype(np.int16)

    hz, db = [300, 1000, 3400, 8000], [6.0, 0.0, -12.0]
    r = subprocess.run(base + ["--eq-gain-db", ",".join(map(str, db)), "--eq-edges-hz", ",".join(map(str, hz)), "--eq-taps", "127"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    edges = capi.BandLevels.from_hz(SR, hz).edges.tolist()
    f = capi.Filter.from_band_gains_db(db, edges, 127)
    w, nf = m.synthesize(ids, puncts, style, g.max_seq_len, fitted=True, target_frames=123, volume=vol, filter=f)
    assert nf == 123
    pcm = np.frombuffer(out.read_bytes()[44:], "<i2")
    assert np.array_equal(pcm, pcm_of(w, nf)) and pcm.any()
    plain = m.synthesize(ids, puncts, style, g.max_seq_len, fitted=True, target_frames=123, volume=vol)[0]
    assert not np.array_equal(pcm, pcm_of(plain, nf))
    # the default bands and tap count
    r = subprocess.run(base + ["--eq-gain-db", ",".join(["-6"] * 8 + ["3"] * 8)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    w, nf = m.synthesize(ids, puncts, style, g.max_seq_len, fitted=True, target_frames=123, volume=vol,
                         filter=capi.Filter.from_band_gains_db([-6.0] * 8 + [3.0] * 8))
    assert np.array_equal(np.frombuffer(out.read_bytes()[44:], "<i2"), pcm_of(w, nf))
    # taps from a file
    h = _taps(77, 33)
    taps = tmp_path / "taps.txt"
    taps.write_text("".join("%.9g\n" % float(t) for t in h))
    r = subprocess.run(base + ["--filter-taps", str(taps)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    w, nf = m.synthesize(ids, puncts, style, g.max_seq_len, fitted=True, target_frames=123, volume=vol, filter=h)
    assert np.array_equal(np.frombuffer(out.read_bytes()[44:], "<i2"), pcm_of(w, nf))
    taps.write_text("0.5\n0.5\n")
    r = subprocess.run(base + ["--filter-taps", str(taps)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "filter n_taps" in r.stderr
