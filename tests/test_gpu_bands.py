"""-m gpu: band levels (include/zerovox_amd.h "band levels") at the production geometry (the "medium" synthetic checkpoint, 22 050 Hz,
hop 300; the two kernels depend on the hop, the lengths, the band count and the edges alone).

bands_frames_kernel and bands_phonemes_kernel run behind the vocoder's last step, the envelope, the volume passes, the contour and the
pitch track, so every expectation is the rule restated in Python (tests/bands_rule.py) applied to the waveform and the durations[] THE
SAME CALL returned: there is no tolerance anywhere, the bits must match.
  * band levels are a meter: waveform, n_frames, durations, levels, contour rows and pitch rows of plain, fitted, target, volume,
    envelope, contour and pitch calls keep their bits with them (eager, graph capture, replay);
  * a replayed graph picks up new edges and a new band count;
  * every speech length 0 .. 64 of a small utterance, fitted and unfitted; capacities 1 .. 4 (shorter than the window) and around one
    and two of the frames kernel's tiles;
  * the operand map of the i8 matrix instruction: impulses read back single columns of both tables, through 64 one-bin bands at several
    offsets; the digit combination at the quantiser's ceiling (hi = 64) and on negative samples;
  * edges: one band, 64 bands, a band touching bin 0, a band touching bin 512, the defaults; bands strictly inside one 16-bin block
    of the kernel's, whose first and last bins have no band; random edge sets;
  * a forced phoneme longer than a tile between phonemes of 0 and 1 frames; a capacity that cuts a phoneme;
  * batches (ragged with mixed wishes and edges, graph replay on poisoned lanes, begin / end with two lanes in flight, tail groups)
    = the rule and the stand-alone calls;
  * the two launches appear in the profile only with a request; envelope, volume, contour, pitch and bands in one call; validation; the
    CLI's files."""
import os
import subprocess

import numpy as np
import pytest

import bands_rule as BR
import level_rule as LR

pytestmark = pytest.mark.gpu

_M = {}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SR = 22050


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


def _gains(N, seed):
    g = np.random.default_rng(seed).random(N) * 4.0
    g[::5] = 0.0
    g[3::7] = 16.0
    return g.astype(F)


def _kw(spec):
    if spec is None:
        return {}
    return dict(n_bands=spec.n_bands, edges=None if spec.edges is None else spec.edges.tolist())


def _check(what, bands, wav, dur, T, hop, frames=True, phonemes=True, spec=None):
    """the tables of a call against the rule applied to the waveform and the durations the same call returned"""
    r = BR.rule(wav, T, hop, dur if phonemes else None, **_kw(spec))
    nb = r["n_bands"]
    assert (bands.frames is not None) == frames and (bands.phonemes is not None) == phonemes, what
    if frames:
        assert bands.frames.shape == (T, nb) and bands.frames.dtype == F
        bad = np.flatnonzero((BR.bits(bands.frames) != BR.bits(r["frames"])).any(axis=1))
        assert bad.size == 0, (what, "frames", bad.size, bad[:8], bands.frames[bad[:2]], r["frames"][bad[:2]])
    if phonemes:
        assert bands.phonemes.shape == (len(dur), nb) and bands.phonemes.dtype == F
        bad = np.flatnonzero((BR.bits(bands.phonemes) != BR.bits(r["phonemes"])).any(axis=1))
        assert bad.size == 0, (what, "phonemes", bad.size, bad[:8], bands.phonemes[bad[:2]], r["phonemes"][bad[:2]], np.asarray(dur)[bad[:4]])
    return r


def _same(a, b):
    return (a is None and b is None) or np.array_equal(BR.bits(a), BR.bits(b))


def _spec(wish):
    from zerovox_cpp_amd import capi
    return wish if isinstance(wish, capi.BandLevels) else None


# ---- 1. band levels are a meter -------------------------------------------------------------------------------------------------------

def test_band_levels_change_no_other_result(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    N, T, hop = 40, 100, g.hop_size
    ids, puncts, style = _utt(g, 11, N)
    kinds = dict(plain={}, fitted=dict(fitted=True), target=dict(target_frames=77), volume=dict(target_frames=60, volume=capi.Volume(1.3, 0.05, 0.4)),
                 envelope=dict(fitted=True, target_frames=66, envelope=capi.Envelope(_gains(N, 1), 2, 37, 53)))
    m.set_graph_mode(False)
    refs = {}
    for kind, kw in kinds.items():
        w, nf, dur, lv, c, p = m.synthesize(ids, puncts, style, T, return_durations=True, return_levels=True, return_contour=True, return_pitch=True, **kw)
        refs[kind] = (w.copy(), nf, dur.copy(), LR.level_bits(lv), c.frames.copy(), c.phonemes.copy(), p.frames.copy(), p.phonemes.copy())
    plain = m.synthesize(ids, puncts, style, T)[0].copy()
    assert np.array_equal(LR.bits(plain), LR.bits(refs["plain"][0]))
    first = {}
    for graph in (False, True):
        m.set_graph_mode(graph)
        for rep in range(2 if graph else 1):               # capture, then replay
            for kind, kw in kinds.items():
                for wish in (True, "frames", "phonemes"):
                    w, nf, dur, lv, c, p, b = m.synthesize(ids, puncts, style, T, return_durations=True, return_levels=True, return_contour=True,
                                                           return_pitch=True, return_bands=wish, **kw)
                    w0, nf0, dur0, lv0, cf0, cp0, pf0, pp0 = refs[kind]
                    assert nf == nf0 and dur.tolist() == dur0.tolist() and LR.level_bits(lv) == lv0, (kind, wish, graph, rep)
                    assert np.array_equal(LR.bits(w), LR.bits(w0)), (kind, wish, graph, rep)
                    assert _same(c.frames, cf0) and _same(c.phonemes, cp0) and _same(p.frames, pf0) and _same(p.phonemes, pp0), (kind, wish, graph, rep)
                    if (kind, wish) not in first:          # the rule once per waveform; every other run is held to these bits
                        _check((kind, wish), b, w, dur, T, hop, wish != "phonemes", wish != "frames")
                        first[kind, wish] = (b.frames, b.phonemes)
                    assert _same(b.frames, first[kind, wish][0]) and _same(b.phonemes, first[kind, wish][1]), (kind, wish, graph, rep)
                assert _same(first[kind, True][0], first[kind, "frames"][0]) and _same(first[kind, True][1], first[kind, "phonemes"][1])
            # the plain call keeps its bits next to graphs captured with band levels, and return_bands=False asks for nothing
            res = m.synthesize(ids, puncts, style, T, return_bands=False)
            assert len(res) == 2 and np.array_equal(LR.bits(res[0]), LR.bits(plain)), (graph, rep)
    # bands alone, without contour or pitch: the same rows
    w, nf, dur, b = m.synthesize(ids, puncts, style, T, return_durations=True, return_bands=True)
    assert np.array_equal(LR.bits(w), LR.bits(plain)) and _same(b.frames, first["plain", True][0]) and _same(b.phonemes, first["plain", True][1])
    m.set_graph_mode(False)


def test_a_replayed_graph_picks_up_new_edges_and_band_counts(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    N, T, hop = 24, 48, g.hop_size
    utts = [(*_utt(g, 12, N), T, None, None, 40), (*_utt(g, 13, N), T, None, None, 48)]
    specs = [capi.BandLevels(), capi.BandLevels(edges=[0, 513]), capi.BandLevels(edges=list(range(3, 68))), capi.BandLevels(edges=[2, 9, 100, 300, 512])]
    m.set_graph_mode(True)
    bc = m.prepare_batch(utts, durations=True, return_bands=[specs[0], specs[1]])
    bc.run()
    seen = set()
    for k in range(1, 5):                                     # replays: band count and edges of both utterances change every time
        ta, tb = specs[k % 4], specs[(k + 2) % 4]
        bc.set_bands(0, ta)
        bc.set_bands(1, tb)
        bc.run()
        for i, t in enumerate((ta, tb)):
            w, n = bc.results()[i]
            _check((k, i), bc.bands[i], w, bc.durations[i], T, hop, spec=t)
            seen.add(BR.bits(bc.bands[i].frames).tobytes())
    assert len(seen) >= 4
    m.set_graph_mode(False)


# ---- 2. every length, the tile edges --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fitted", [False, True])
def test_every_speech_length_of_a_small_utterance(env, fitted):
    m, g, _ = env
    N, T, hop = 16, 64, g.hop_size
    ids, puncts, style = _utt(g, 21, N)
    for nf in range(0, T + 1):
        kw = dict(phonemes=dict(duration_frames=np.zeros(N, np.int32))) if nf == 0 else dict(target_frames=nf)
        w, n, dur, b = m.synthesize(ids, puncts, style, T, fitted=fitted, return_durations=True, return_bands=True, **kw)
        assert n == nf == int(dur.sum())
        _check((fitted, nf), b, w, dur, T, hop)
        if fitted:
            assert not BR.bits(b.frames[nf + 2:]).any(), nf        # fitted zeros give zero rows (a span two frames behind the speech sees none of it)
        else:
            assert BR.bits(b.frames).any(axis=1).all(), nf         # an unfitted tail is measured like the speech


def test_capacities_below_the_window_and_around_the_frames_kernels_tile(env):
    m, g, _ = env
    hop, c = g.hop_size, BR.tile_frames()
    N = 16
    ids, puncts, style = _utt(g, 22, N)
    assert 4 * hop > BR.N > 3 * hop
    for T in (1, 2, 3, 4, c - 1, c, c + 1, 2 * c - 1, 2 * c, 2 * c + 1):
        for fitted in (False, True):
            w, n, dur, b = m.synthesize(ids, puncts, style, T, fitted=fitted, target_frames=max(T - 3, 1), return_durations=True, return_bands=True)
            assert n == max(T - 3, 1)
            _check((T, fitted), b, w, dur, T, hop)


# ---- 3. the operand map, the digits, the edges --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("t0", [0, 1, 63, 64, 511, 1023])
def test_an_impulse_reads_back_one_column_of_both_tables(env, t0):
    """y = delta[t0] in frame 4's span: Re(k) = 4096 C[k][t0], Im(k) = 4096 S[k][t0] (an impulse of 0.5 quantises to 4 096 at k = 13), so a
    one-bin band reads sqrt(((4096^2 (C^2 + S^2)) >> 6) / 48774928) * 2^-13 exactly: every column of the i8 operand map, asymmetric in k"""
    from zerovox_cpp_amd import capi
    m, g, _ = env
    T, hop = 8, g.hop_size
    s0 = 4 * hop + hop // 2 - BR.N // 2
    x = np.zeros(T * hop, F)
    x[s0 + t0] = 0.5
    C_, S_ = BR.tables()
    for off in (0, 1, 15, 16, 17, 200, 449):
        spec = capi.BandLevels(edges=list(range(off, off + 65)))
        b = m.band_levels(x, spec)
        r = _check((t0, off), b, x, None, T, hop, phonemes=False, spec=spec)
        for j in (0, 1, 31, 63):
            kbin = off + j
            want = BR.band_row(((4096 * int(C_[kbin, t0])) ** 2 + (4096 * int(S_[kbin, t0])) ** 2) >> 6, 13)[0]
            assert BR.bits(b.frames[4, j]) == BR.bits(want) == BR.bits(r["frames"][4, j]), (t0, off, j)


def test_digit_combination_at_the_ceiling_and_on_negative_samples(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    T, hop = 8, g.hop_size
    rng = np.random.default_rng(3)
    spec = capi.BandLevels(edges=[0, 1, 2, 5, 100, 512, 513])
    for name, x in (("ceiling", np.full(T * hop, F(8191.0 / 8192.0), F)), ("negative ceiling", np.full(T * hop, F(-8191.0 / 8192.0), F)),
                    ("negative", -np.abs(rng.standard_normal(T * hop) * 0.3)), ("alternating ceiling", np.tile(np.array([8191.0, -8191.0], F) / F(8192), T * hop // 2)),
                    ("noise", rng.standard_normal(T * hop) * 0.3)):
        x = np.asarray(x, F)
        _check(name, m.band_levels(x, spec), x, None, T, hop, phonemes=False, spec=spec)
        _check(name, m.band_levels(x), x, None, T, hop, phonemes=False)
    a, k = BR.quantise(BR.spans(np.full(T * hop, F(8191.0 / 8192.0), F), T, hop)[3])
    assert k == 13 and (a == 8191).all()                     # hi = (8191 + 64) >> 7 = 64, lo = -1


@pytest.mark.parametrize("edges", [[0, 513], list(range(0, 512, 8)) + [513], [0, 1, 7], [500, 512, 513], [512, 513], None, list(range(449, 514))])
def test_edges(env, edges):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    N, T, hop = 16, 37, g.hop_size
    ids, puncts, style = _utt(g, 30, N)
    spec = capi.BandLevels(edges=edges)
    w, n, dur, b = m.synthesize(ids, puncts, style, T, target_frames=30, return_durations=True, return_bands=spec)
    _check(edges, b, w, dur, T, hop, spec=spec)
    specials = np.array([0x7fc00000, 0x7f800000, 0xff800000, 0x80000000, 0x00000001, 0x7f7fffff], np.uint32).view(F)
    rng = np.random.default_rng(5)
    x = np.where(rng.random(w.size) < 0.02, rng.choice(specials, w.size), w).astype(F)
    _check((edges, "specials"), m.band_levels(x, spec), x, None, T, hop, phonemes=False, spec=spec)


INSIDE = [[3, 5], [17, 20], [1, 3, 5, 8, 12], [500, 505], [83, 90], [1, 2], [14, 15], [2, 3, 4, 5, 6], [18, 20, 45], [30, 33, 40, 47], [497, 500, 511],
          [510, 512], [7, 9, 300, 310]]


@pytest.mark.parametrize("edges", INSIDE)
def test_bands_that_leave_both_ends_of_a_bin_block_unassigned(env, edges):
    """the frames kernel adds a 16-bin block up in one step where its first and last bin lie in one band, and skips a block none of whose
    bins has a band: bands strictly inside a block, whose first and last bin have none, must take neither shortcut"""
    from zerovox_cpp_amd import capi
    m, g, _ = env
    N, T, hop = 16, 37, g.hop_size
    ids, puncts, style = _utt(g, 33, N)
    spec = capi.BandLevels(edges=edges)
    w, n, dur, b = m.synthesize(ids, puncts, style, T, target_frames=30, return_durations=True, return_bands=spec)
    _check(edges, b, w, dur, T, hop, spec=spec)
    assert b.frames[:30].all() and b.phonemes[dur > 0].all()
    x = (np.random.default_rng(9).standard_normal(T * hop) * 0.3).astype(F)
    b = m.band_levels(x, spec)
    _check((edges, "noise"), b, x, None, T, hop, phonemes=False, spec=spec)
    assert b.frames.all()


def test_random_edges(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    T, hop = 6, g.hop_size
    rng = np.random.default_rng(10)
    x = (rng.standard_normal(T * hop) * 0.3).astype(F)
    for k in range(60):
        nb = int(rng.integers(1, 65)) if k % 2 else int(rng.integers(1, 5))
        lo = int(rng.integers(0, BR.BINS - nb))
        hi = BR.BINS + 1 if k % 3 else min(lo + nb + int(rng.integers(1, 40)), BR.BINS + 1)      # every third set lies in a narrow range
        edges = np.sort(rng.choice(np.arange(lo, hi), size=nb + 1, replace=False)).tolist()
        spec = capi.BandLevels(edges=edges)
        _check(("random", k, edges), m.band_levels(x, spec), x, None, T, hop, phonemes=False, spec=spec)


def test_band_levels_of_silence_and_of_a_long_waveform(env):
    m, g, _ = env
    T, hop = 8, g.hop_size
    rng = np.random.default_rng(6)
    x = (rng.standard_normal(T * hop) * 0.2).astype(F)
    for name, w in (("zeros", np.zeros_like(x)), ("-0.0", np.full_like(x, -0.0)), ("below 2^-24", x * F(2.0 ** -26)), ("1e30", x * F(1e30))):
        b = m.band_levels(w)
        _check(name, b, w, None, T, hop, phonemes=False)
        assert name == "1e30" or not BR.bits(b.frames).any()
    c = BR.tile_frames()
    w = (rng.standard_normal((2 * c + 3) * hop) * 0.1 + np.sin(np.arange((2 * c + 3) * hop) * 2 * np.pi / 90.5)).astype(F)
    _check("two tiles and a bit", m.band_levels(w), w, None, 2 * c + 3, hop, phonemes=False)


# ---- 4. phonemes -------------------------------------------------------------------------------------------------------------------------

def test_a_forced_phoneme_longer_than_a_tile(env):
    m, g, _ = env
    N, T, hop = 16, 200, g.hop_size
    ids, puncts, style = _utt(g, 31, N)
    forced = np.array([3, 0, 100, 1, 0, 0, 7, 1, 0, 2, 40, 0, 1, 5, 0, 9], np.int32)          # 169 frames
    assert forced[2] > 3 * BR.tile_frames() and int(forced.sum()) < T
    w, nf, dur, b = m.synthesize(ids, puncts, style, T, fitted=True, phonemes=dict(duration_frames=forced), return_durations=True, return_bands=True)
    assert nf == int(forced.sum()) and dur.tolist() == forced.tolist()
    _check("long", b, w, dur, T, hop)
    assert not BR.bits(b.phonemes[forced == 0]).any() and BR.bits(b.phonemes[forced > 0]).any(axis=1).all()


def test_a_capacity_that_cuts_a_phoneme_in_two(env):
    m, g, _ = env
    N, T, hop = 16, 64, g.hop_size
    ids, puncts, style = _utt(g, 32, N)
    forced = np.array([0, 9, 0, 0, 3, 1, 12, 0, 7, 40, 0, 5, 9, 0, 2, 4], np.int32)          # 92 frames: phoneme 9 is cut by T = 64
    for fitted in (False, True):
        w, nf, dur, b = m.synthesize(ids, puncts, style, T, fitted=fitted, phonemes=dict(duration_frames=forced), return_durations=True,
                                     return_bands=True)
        assert nf == T and dur.tolist() == forced[:9].tolist() + [64 - int(forced[:9].sum())] + [0] * 6
        _check(("cut", fitted), b, w, dur, T, hop)
        assert not BR.bits(b.phonemes[10:]).any()           # the rest of the utterance has no frame


# ---- 5. batches = the rule and the stand-alone calls --------------------------------------------------------------------------------

def _ragged(g):
    nt = [(40, 150, 101), (7, 60, 0), (60, 130, 130), (1, 11, 5), (100, 160, 97)]
    return [(*_utt(g, 500 + i, N), T, None, None, tf) for i, (N, T, tf) in enumerate(nt)]


def _wishes():
    from zerovox_cpp_amd import capi
    return [capi.BandLevels(edges=[1, 40, 200, 513], frames=True, phonemes=False), "phonemes", capi.BandLevels(edges=list(range(0, 512, 8)) + [513]), False, True]


def _same_as_the_rule(bc, wishes, hop, what, want_wav=None):
    for i, (w, n) in enumerate(bc.results()):
        if want_wav is not None:
            assert np.array_equal(LR.bits(w), LR.bits(want_wav[i])), (what, i)
        if bc.bands[i] is None:
            assert wishes[i] is False
            continue
        b = bc.bands[i]
        _check((what, i), b, w, bc.durations[i], len(w) // hop, hop, b.frames is not None, b.phonemes is not None, _spec(wishes[i]))


def _scrub(bc):
    """overwrite the tables so that a run that wrote nothing cannot pass"""
    for b in bc.bands:
        for a in ([] if b is None else [b.frames, b.phonemes]):
            if a is not None:
                a.fill(-7.0)


def _copy(bc):
    return [None if b is None else tuple(None if a is None else a.copy() for a in (b.frames, b.phonemes)) for b in bc.bands]


@pytest.mark.parametrize("fitted", [False, True])
def test_ragged_batch_replay_and_poison(env, fitted):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    hop = g.hop_size
    utts, wishes = _ragged(g), _wishes()
    m.set_graph_mode(False)
    plains = [w.copy() for w, _ in m.synthesize_batch(utts, fitted=fitted)]
    alone = []
    for i, u in enumerate(utts):
        res = m.synthesize(*u[:4], fitted=fitted, target_frames=u[6], return_durations=True, return_bands=wishes[i])
        assert np.array_equal(LR.bits(res[0]), LR.bits(plains[i])), i
        alone.append(res[3] if wishes[i] is not False else None)
    bc = m.prepare_batch(utts, durations=True, fitted=fitted, return_bands=wishes)
    steps = [("eager", False, None), ("graph capture", True, None), ("graph replay on a lane poisoned with 0xFF", True, 0xFF),
             ("graph replay on a lane poisoned with 0x00", True, 0x00)]
    for k, (what, graph, poison) in enumerate(steps):
        m.set_graph_mode(graph)
        if poison is not None:
            m.poison(poison)
        _scrub(bc)
        bc.run()
        if k == 0:
            _same_as_the_rule(bc, wishes, hop, what, plains)     # the rule once; the stand-alone calls and the other runs are held to these bits
            first = _copy(bc)
        for i, a in enumerate(alone):
            assert np.array_equal(LR.bits(bc.results()[i][0]), LR.bits(plains[i])), (what, i)
            for j, name in enumerate(("frames", "phonemes")):
                if a is None:
                    assert bc.bands[i] is None
                    continue
                assert _same(getattr(bc.bands[i], name), getattr(a, name)), (what, i, name)
                assert _same(getattr(bc.bands[i], name), first[i][j]), (what, i, name)
    _scrub(bc)
    bc.begin(2)
    bc.end(2)
    for i, b in enumerate(bc.bands):
        assert b is None or (_same(b.frames, first[i][0]) and _same(b.phonemes, first[i][1])), i
    # the plain batch next to it, and the _bands entry point with bands NULL / no table asked for
    for i, (w, n) in enumerate(m.synthesize_batch(utts, fitted=fitted)):
        assert np.array_equal(LR.bits(w), LR.bits(plains[i])), i
    null = m.prepare_batch(utts, fitted=fitted)
    args = (m.h, null.n, null.ids_p, null.pun_p, null.sty_p, null.Ns, null.Ts, null.wav_p, null.nf)
    bad = (capi.BandsC * len(utts))(*[capi.BandsC(None, None, 99, None)] * len(utts))      # no table: the parameters are not looked at
    for bnd in (None, (capi.BandsC * len(utts))(), bad):
        for w in null.wavs:
            w.fill(7.0)
        m._chk(m.lib.zv_synthesize_batch_bands(*args, None, None, None, null.targets, int(fitted), None, None, None, None, None, bnd))
        for i, (w, n) in enumerate(null.results()):
            assert np.array_equal(LR.bits(w), LR.bits(plains[i])), i
    m.set_graph_mode(False)


def test_validation_names_the_utterance_and_the_field(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    utts = _ragged(g)[:2]
    for spec, field in ((capi.BandLevels(n_bands=65), "n_bands"), (capi.BandLevels(n_bands=5), "edges"), (capi.BandLevels(edges=[5, 5, 9]), "edges"),
                        (capi.BandLevels(edges=[9, 5]), "edges"), (capi.BandLevels(edges=[1, 100, 514]), "edges")):
        with pytest.raises(capi.ZvError, match=r"zv_synthesize_batch_bands: utterance 1: bands %s" % field):
            m.synthesize_batch(utts, return_bands=[True, spec])
        with pytest.raises(capi.ZvError, match=r"zv_synthesize_bands: utterance 0: bands %s" % field):
            m.synthesize(*utts[0][:4], return_bands=spec)
        with pytest.raises(capi.ZvError, match=r"zv_band_levels: bands %s" % field):
            m.band_levels(np.zeros(g.hop_size, F), spec)
    with pytest.raises(capi.ZvError, match="zv_band_levels: T = "):
        m.band_levels(np.zeros(g.hop_size * (m.max_frames() + 1), F))


def test_two_lanes_in_flight(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    hop = g.hop_size
    sets = [[(*_utt(g, 600 + 10 * k + i, 20 + 5 * i), 40 + 10 * k + 9 * i, None, None, 20 + 10 * k + 7 * i) for i in range(3)] for k in range(3)]
    wishes = [["frames", True, "phonemes"], [capi.BandLevels(edges=[0, 3, 513]), False, True], ["phonemes", "frames", capi.BandLevels(edges=list(range(100, 165)))]]
    batches = [m.prepare_batch(utts, durations=True, return_bands=wishes[k]) for k, utts in enumerate(sets)]
    for graph in (False, True):
        m.set_graph_mode(graph)
        for bc in batches:
            _scrub(bc)
        for k, bc in enumerate(batches):                 # _begin k, _end k - 1
            bc.begin(k % 2)
            if k:
                batches[k - 1].end((k - 1) % 2)
        batches[-1].end((len(batches) - 1) % 2)
        for k, bc in enumerate(batches):
            if not graph:
                _same_as_the_rule(bc, wishes[k], hop, f"lanes, batch {k}")
                bc.first = _copy(bc)
            for i, b in enumerate(bc.bands):
                assert b is None or (_same(b.frames, bc.first[i][0]) and _same(b.phonemes, bc.first[i][1])), (k, i, graph)
    m.set_graph_mode(False)


def test_batch_split_into_tail_groups(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    hop, T = g.hop_size, 900                                  # 16 utterances: 2 and 8 groups are different schedules (two utterances per group at least)
    tfs = [900, 500, 250, 37, 899, 1, 640, 333, 65, 700, 31, 32, 33, 450, 820, 128]
    utts = [(*_utt(g, 700 + i, 40 + 9 * i), T, None, None, tf) for i, tf in enumerate(tfs)]
    assert len(utts) * T * hop * 4 >= 16 << 20 and len(utts) // 2 >= 8
    # frames of two utterances and the phonemes of all but four are held to the rule; every table to the one-group run
    wishes = [[capi.BandLevels(edges=[1, 30, 513], phonemes=False), "phonemes", "phonemes", False][i % 4] for i in range(len(utts))]
    wishes[-1] = capi.BandLevels(edges=list(range(0, 512, 8)) + [513])
    m.set_graph_mode(False)
    with capi.switches(ZV_TAIL_GROUPS=1):
        bc = m.prepare_batch(utts, durations=True, fitted=True, return_bands=wishes)
        bc.run()
        assert [n for _, n in bc.results()] == tfs
        for i in (0, 1, 5, 15):
            b, (w, n) = bc.bands[i], bc.results()[i]
            _check(("one group", i), b, w, bc.durations[i], T, hop, b.frames is not None, b.phonemes is not None, _spec(wishes[i]))
        one = _copy(bc)
        wavs = [w.copy() for w, _ in bc.results()]
    for groups in (2, 8):
        with capi.switches(ZV_TAIL_GROUPS=groups):
            for graph in (False, True):
                m.set_graph_mode(graph)
                bc = m.prepare_batch(utts, durations=True, fitted=True, return_bands=wishes)
                for rep in range(2 if graph else 1):
                    m.poison(0x00 if rep else 0xFF)
                    _scrub(bc)
                    bc.run()
                    for i, (w, n) in enumerate(bc.results()):
                        assert n == tfs[i] and np.array_equal(LR.bits(w), LR.bits(wavs[i])), (groups, graph, rep, i)
                        if one[i] is None:
                            assert bc.bands[i] is None
                            continue
                        for a, b in zip((bc.bands[i].frames, bc.bands[i].phonemes), one[i]):
                            assert _same(a, b), (groups, graph, rep, i)
            m.set_graph_mode(False)


# ---- 6. the profile; with everything else; the CLI ---------------------------------------------------------------------------------------

def test_the_two_launches_appear_only_with_a_request(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    N = 30
    ids, puncts, style = _utt(g, 42, N)
    T = 150
    kw = dict(target_frames=100, volume=capi.Volume(1.0, 0.1, 0.5), envelope=capi.Envelope(_gains(N, 6), 1, 10, 10), return_contour=True, return_pitch=True)
    m.profile_begin()
    m.synthesize(ids, puncts, style, T, **kw)
    without = {s["name"]: s for s in m.profile_end()}
    m.profile_begin()
    m.synthesize(ids, puncts, style, T, return_bands="phonemes", **kw)
    with_b = {s["name"]: s for s in m.profile_end()}
    assert "voc_bands_frames" not in without and "voc_bands_phonemes" not in without
    assert set(with_b) == set(without) | {"voc_bands_frames", "voc_bands_phonemes"}
    for k in without:
        assert with_b[k]["launches"] == without[k]["launches"], k
    names = list(with_b)
    assert names.index("voc_pitch_phonemes") < names.index("voc_bands_frames") == names.index("voc_bands_phonemes") - 1
    assert with_b["voc_bands_frames"]["launches"] == 1 and with_b["voc_bands_phonemes"]["launches"] == 1


def test_envelope_volume_contour_pitch_and_bands_in_one_call(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    N, T, hop = 40, 100, g.hop_size
    ids, puncts, style = _utt(g, 61, N)
    e = capi.Envelope(_gains(N, 7), 2, 5 * hop, 7 * hop + 3)
    vol = capi.Volume(0.8, 0.07, 0.5)
    for fitted in (False, True):
        ref, _, lv0, c0, p0 = m.synthesize(ids, puncts, style, T, fitted=fitted, target_frames=80, envelope=e, volume=vol, return_levels=True,
                                           return_contour=True, return_pitch=True)
        ref = ref.copy()
        rows = None
        for graph in (False, True, True):
            m.set_graph_mode(graph)
            w, n, dur, lv, c, p, b = m.synthesize(ids, puncts, style, T, fitted=fitted, target_frames=80, envelope=e, volume=vol, return_durations=True,
                                                  return_levels=True, return_contour=True, return_pitch=True, return_bands=True)
            assert n == 80 and np.array_equal(LR.bits(w), LR.bits(ref)) and LR.level_bits(lv) == LR.level_bits(lv0)
            assert _same(c.frames, c0.frames) and _same(c.phonemes, c0.phonemes) and _same(p.frames, p0.frames) and _same(p.phonemes, p0.phonemes)
            if rows is None:
                _check((fitted, graph), b, w, dur, T, hop)
                rows = (b.frames, b.phonemes)
            assert _same(b.frames, rows[0]) and _same(b.phonemes, rows[1]), (fitted, graph)
        m.set_graph_mode(False)


def _read_tsv(path, edges):
    lines = open(path).read().splitlines()
    assert lines[0] == "index\t" + "\t".join(f"{a}-{b}" for a, b in zip(edges, edges[1:]))
    rows = [l.split("\t") for l in lines[1:]]
    assert [int(r[0]) for r in rows] == list(range(len(rows)))
    return np.array([[F(v) for v in r[1:]] for r in rows], F).reshape(len(rows), len(edges) - 1)


def test_cli_round_trip(env, tmp_path):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    N, hop = 40, g.hop_size
    ids, puncts, style = _utt(g, 71, N)
    utt = tmp_path / "utt.txt"
    utt.write_text(" ".join(map(str, ids.tolist())) + "\n" + " ".join(map(str, puncts.tolist())) + "\n" +
                   " ".join(repr(float(x)) for x in style.tolist()) + "\n")
    out, ff, pf = tmp_path / "bands.wav", tmp_path / "bands.tsv", tmp_path / "phonemes.tsv"
    cli = os.path.join(ROOT, "zerovox.cpp_amd", "zerovox")
    base = [cli, "-m", _M["path"], "-u", str(utt), "-o", str(out), "--fit", "--target-frames", "123", "--bands", str(ff), "--phoneme-bands", str(pf)]
    hz = [100, 300, 1000, 3000, 8000, 11025]
    r = subprocess.run(base + ["--band-edges-hz", ",".join(map(str, hz))], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    spec = capi.BandLevels.from_hz(SR, hz)
    assert spec.edges.tolist() == [5, 14, 46, 139, 372, 512]
    w, nf, dur, b = m.synthesize(ids, puncts, style, g.max_seq_len, fitted=True, target_frames=123, return_durations=True, return_bands=spec)
    assert nf == 123
    _check("cli", b, w, dur, g.max_seq_len, hop, spec=spec)
    frames, phonemes = _read_tsv(ff, spec.edges.tolist()), _read_tsv(pf, spec.edges.tolist())
    assert frames.shape == (g.max_seq_len, 5) and phonemes.shape == (N, 5)
    assert np.array_equal(BR.bits(frames), BR.bits(b.frames)) and np.array_equal(BR.bits(phonemes), BR.bits(b.phonemes))
    # the defaults, and edges that fall on one bin once the rate is known
    r = subprocess.run(base, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    d = m.synthesize(ids, puncts, style, g.max_seq_len, fitted=True, target_frames=123, return_bands=True)[2]
    assert np.array_equal(BR.bits(_read_tsv(ff, list(BR.DEFAULT_EDGES))), BR.bits(d.frames))
    r = subprocess.run(base + ["--band-edges-hz", "100,105,1000"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "fall on the same bin" in r.stderr
