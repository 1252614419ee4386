"""-m gpu: the pitch track (include/zerovox_amd.h "pitch track") at the production geometry (the "medium" synthetic checkpoint, 22 050 Hz,
hop 300; the two kernels depend on the rate, the hop, the lengths and the parameters alone).

pitch_frames_kernel and pitch_phonemes_kernel run behind the vocoder's last step, the envelope, the volume passes and the contour, so
every expectation is the rule restated in Python (tests/pitch_rule.py) applied to the waveform and the durations[] THE SAME CALL
returned: there is no tolerance anywhere, the bits must match.
  * a pitch track is a meter: waveform, n_frames, durations, levels and contour rows of plain, fitted, target, volume, envelope and
    contour calls keep their bits with it (eager, graph capture, replay), and the plain call keeps its bits next to them;
  * a replayed graph picks up new lags, window and threshold;
  * every speech length 0 .. 64 of a small utterance, fitted and unfitted; capacities around one and two of the frames kernel's chunks;
  * the parameters at their bounds; a forced phoneme of 1 100 frames between phonemes of 0 and 1 frames; a capacity that cuts a phoneme;
  * zv_pitch_track on signals of known period, on NaN, inf and 1e30 samples and on silence;
  * batches (ragged with mixed wishes and parameters, the first and last frames of every utterance, graph replay on poisoned lanes,
    begin / end with two lanes in flight, tail groups) = the rule and the stand-alone calls;
  * the two launches appear in the profile only with a pitch request; envelope, volume, contour and pitch in one call; the CLI's files."""
import os
import subprocess

import numpy as np
import pytest

import level_rule as LR
import pitch_rule as PR

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


def _kw(track):
    return {} if track is None else dict(min_lag=track.min_lag, max_lag=track.max_lag, window=track.window, threshold=track.voiced_threshold)


def _check(what, pitch, wav, dur, T, hop, frames=True, phonemes=True, track=None):
    """the tables of a call against the rule applied to the waveform and the durations the same call returned"""
    r = PR.rule(wav, T, SR, hop, dur if phonemes else None, **_kw(track))
    assert (pitch.frames is not None) == frames and (pitch.phonemes is not None) == phonemes, what
    if frames:
        assert pitch.frames.shape == (T, 2) and pitch.frames.dtype == F
        bad = np.flatnonzero((PR.bits(pitch.frames) != PR.bits(r["frames"])).any(axis=1))
        assert bad.size == 0, (what, "frames", bad.size, bad[:8], pitch.frames[bad[:4]], r["frames"][bad[:4]])
    if phonemes:
        assert pitch.phonemes.shape == (len(dur), 2) and pitch.phonemes.dtype == F
        bad = np.flatnonzero((PR.bits(pitch.phonemes) != PR.bits(r["phonemes"])).any(axis=1))
        assert bad.size == 0, (what, "phonemes", bad.size, bad[:8], pitch.phonemes[bad[:4]], r["phonemes"][bad[:4]], np.asarray(dur)[bad[:4]])
    return r


def _same(a, b):
    return (a is None and b is None) or np.array_equal(PR.bits(a), PR.bits(b))


# ---- 1. a pitch track is a meter ------------------------------------------------------------------------------------------------------

def test_a_pitch_track_changes_no_other_result(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    N, T, hop = 40, 100, g.hop_size
    ids, puncts, style = _utt(g, 11, N)
    kinds = dict(plain={}, fitted=dict(fitted=True), target=dict(target_frames=77), volume=dict(target_frames=60, volume=capi.Volume(1.3, 0.05, 0.4)),
                 envelope=dict(fitted=True, target_frames=66, envelope=capi.Envelope(_gains(N, 1), 2, 37, 53)),
                 contour=dict(target_frames=90, return_contour=True))
    m.set_graph_mode(False)
    refs = {}
    for kind, kw in kinds.items():
        kw = dict(kw, return_contour=True)
        w, nf, dur, lv, c = m.synthesize(ids, puncts, style, T, return_durations=True, return_levels=True, **kw)
        refs[kind] = (w.copy(), nf, dur.copy(), LR.level_bits(lv), c.frames.copy(), c.phonemes.copy())
    plain = m.synthesize(ids, puncts, style, T)[0].copy()
    assert np.array_equal(LR.bits(plain), LR.bits(refs["plain"][0]))
    first = {}
    for graph in (False, True):
        m.set_graph_mode(graph)
        for rep in range(2 if graph else 1):               # capture, then replay
            for kind, kw in kinds.items():
                kw = dict(kw, return_contour=True)
                for wish in (True, "frames", "phonemes"):
                    w, nf, dur, lv, c, p = m.synthesize(ids, puncts, style, T, return_durations=True, return_levels=True, return_pitch=wish, **kw)
                    w0, nf0, dur0, lv0, cf0, cp0 = refs[kind]
                    assert nf == nf0 and dur.tolist() == dur0.tolist() and LR.level_bits(lv) == lv0, (kind, wish, graph, rep)
                    assert np.array_equal(LR.bits(w), LR.bits(w0)), (kind, wish, graph, rep)
                    assert _same(c.frames, cf0) and _same(c.phonemes, cp0), (kind, wish, graph, rep)
                    if (kind, wish) not in first:          # the rule once per waveform; every other run is held to these bits
                        _check((kind, wish), p, w, dur, T, hop, wish != "phonemes", wish != "frames")
                        first[kind, wish] = (p.frames, p.phonemes)
                    assert _same(p.frames, first[kind, wish][0]) and _same(p.phonemes, first[kind, wish][1]), (kind, wish, graph, rep)
                assert _same(first[kind, True][0], first[kind, "frames"][0]) and _same(first[kind, True][1], first[kind, "phonemes"][1])
            # the plain call keeps its bits next to graphs captured with a pitch track, and return_pitch=False asks for nothing
            res = m.synthesize(ids, puncts, style, T, return_pitch=False)
            assert len(res) == 2 and np.array_equal(LR.bits(res[0]), LR.bits(plain)), (graph, rep)
    m.set_graph_mode(False)


def test_a_replayed_graph_picks_up_new_parameters(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    N, T, hop = 24, 48, g.hop_size
    utts = [(*_utt(g, 12, N), T, None, None, 40), (*_utt(g, 13, N), T, None, None, 48)]
    tracks = [capi.PitchTrack(), capi.PitchTrack(40, 300, 512, 0.3), capi.PitchTrack(8, 64, 64, 0.9), capi.PitchTrack(64, 512, 1024, 0.05)]
    m.set_graph_mode(True)
    bc = m.prepare_batch(utts, durations=True, return_pitch=[tracks[0], tracks[1]])
    bc.run()
    seen = set()
    for k in range(1, 5):                                     # replays: the parameters of both utterances change every time
        ta, tb = tracks[k % 4], tracks[(k + 2) % 4]
        bc.set_pitch(0, ta)
        bc.set_pitch(1, tb)
        bc.run()
        for i, t in enumerate((ta, tb)):
            w, n = bc.results()[i]
            _check((k, i), bc.pitches[i], w, bc.durations[i], T, hop, track=t)
            seen.add(PR.bits(bc.pitches[i].frames).tobytes())
    assert len(seen) >= 4
    m.set_graph_mode(False)


# ---- 2. every length, the chunk edges -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fitted", [False, True])
def test_every_speech_length_of_a_small_utterance(env, fitted):
    m, g, _ = env
    N, T, hop = 16, 64, g.hop_size
    ids, puncts, style = _utt(g, 21, N)
    for nf in range(0, T + 1):
        kw = dict(phonemes=dict(duration_frames=np.zeros(N, np.int32))) if nf == 0 else dict(target_frames=nf)
        w, n, dur, p = m.synthesize(ids, puncts, style, T, fitted=fitted, return_durations=True, return_pitch=True, **kw)
        assert n == nf == int(dur.sum())
        _check((fitted, nf), p, w, dur, T, hop)
        if fitted:
            assert not PR.bits(p.frames[nf + 2:]).any(), nf        # fitted zeros give {0, 0} (a span two frames behind the speech sees none of it)
        else:
            assert PR.bits(p.frames[:, 1]).any(), nf               # an unfitted tail is measured like the speech


def test_capacities_around_the_frames_kernels_chunk(env):
    m, g, _ = env
    hop, c = g.hop_size, PR.chunk_frames(ROOT)
    N = 16
    ids, puncts, style = _utt(g, 22, N)
    for T in (1, c - 1, c, c + 1, 2 * c - 1, 2 * c, 2 * c + 1):
        for fitted in (False, True):
            w, n, dur, p = m.synthesize(ids, puncts, style, T, fitted=fitted, target_frames=max(T - 3, 1), return_durations=True, return_pitch=True)
            assert n == max(T - 3, 1)
            _check((T, fitted), p, w, dur, T, hop)


# ---- 3. parameters at their bounds, long forced phonemes, a truncating capacity -----------------------------------------------------------

@pytest.mark.parametrize("lo,hi,window", [(8, 64, 64), (64, 512, 1024), (8, 9, 1024), (511, 512, 64), (50, 400, 601)])
def test_parameters_at_their_bounds(env, lo, hi, window):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    N, T, hop = 16, 37, g.hop_size
    ids, puncts, style = _utt(g, 30, N)
    for thr in (1.0, 1e-6):
        t = capi.PitchTrack(lo, hi, window, thr)
        w, n, dur, p = m.synthesize(ids, puncts, style, T, target_frames=30, return_durations=True, return_pitch=t)
        _check((lo, hi, window, thr), p, w, dur, T, hop, track=t)


def test_a_forced_phoneme_longer_than_a_wave_can_stride_once(env):
    m, g, _ = env
    N, T, hop = 16, 1200, g.hop_size
    ids, puncts, style = _utt(g, 31, N)
    forced = np.array([3, 0, 1100, 1, 0, 0, 7, 1, 0, 2, 64, 0, 1, 5, 0, 9], np.int32)          # 1 193 frames
    assert forced[2] > 64 * 16 and int(forced.sum()) < T
    w, nf, dur, p = m.synthesize(ids, puncts, style, T, fitted=True, phonemes=dict(duration_frames=forced), return_durations=True, return_pitch=True)
    assert nf == int(forced.sum()) and dur.tolist() == forced.tolist()
    _check("long", p, w, dur, T, hop)
    assert not PR.bits(p.phonemes[forced == 0]).any()


def test_a_capacity_that_cuts_a_phoneme_in_two(env):
    m, g, _ = env
    N, T, hop = 16, 64, g.hop_size
    ids, puncts, style = _utt(g, 32, N)
    forced = np.array([0, 9, 0, 0, 3, 1, 12, 0, 7, 40, 0, 5, 9, 0, 2, 4], np.int32)          # 92 frames: phoneme 9 is cut by T = 64
    for fitted in (False, True):
        w, nf, dur, p = m.synthesize(ids, puncts, style, T, fitted=fitted, phonemes=dict(duration_frames=forced), return_durations=True,
                                     return_pitch=True)
        assert nf == T and dur.tolist() == forced[:9].tolist() + [64 - int(forced[:9].sum())] + [0] * 6
        _check(("cut", fitted), p, w, dur, T, hop)
        assert not PR.bits(p.phonemes[10:]).any()           # the rest of the utterance has no frame


# ---- 4. zv_pitch_track on known signals ---------------------------------------------------------------------------------------------------

def _signals(P, T, hop):
    t = np.arange(T * hop)
    return dict(pulses=((t % P) == 0) * 0.7, harmonics=sum(np.sin(2 * np.pi * h * t / P) / h for h in range(1, 9)) * 0.1)


@pytest.mark.parametrize("P", [50, 51, 127, 128, 349, 350])
def test_pitch_track_of_known_periods(env, P):
    m, g, _ = env
    T, hop = 8, g.hop_size
    for name, x in _signals(P, T, hop).items():
        x = x.astype(F)
        p = m.pitch_track(x)
        assert p.phonemes is None
        _check((name, P), p, x, None, T, hop, phonemes=False)
        f0, strength = p.frames[3]                          # frame 3's span [575, 1526) lies inside the waveform
        assert abs(SR / float(f0) - P) <= 0.5 and strength >= 0.9, (name, P, f0, strength)


def test_pitch_track_of_special_samples_and_silence(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    T, hop = 8, g.hop_size
    rng = np.random.default_rng(5)
    x = _signals(100, T, hop)["harmonics"].astype(F)
    specials = np.array([0x7fc00000, 0x7f800000, 0xff800000, 0x80000000, 0x00000001, 0x7f7fffff], np.uint32).view(F)
    for name, w in (("NaN and inf", np.where(rng.random(x.size) < 0.02, rng.choice(specials[:4], x.size), x)),
                    ("1e30", np.where(rng.random(x.size) < 0.02, F(1e30), x)), ("scaled by 1e30", x * F(1e30)),
                    ("all specials", rng.choice(specials, x.size)), ("zeros", np.zeros_like(x)), ("-0.0", np.full_like(x, -0.0)),
                    ("below 2^-24", x * F(2.0 ** -24)), ("noise", (rng.standard_normal(x.size) * 0.1))):
        w = np.asarray(w, F)
        for t in (None, capi.PitchTrack(8, 64, 64, 0.2), capi.PitchTrack(64, 512, 1024, 1.0)):
            p = m.pitch_track(w, t)
            _check((name, t), p, w, None, T, hop, phonemes=False, track=t)
        if name in ("zeros", "-0.0"):
            assert not PR.bits(p.frames).any()
    assert not m.pitch_track((rng.standard_normal(x.size) * 0.1).astype(F)).frames[:, 0].any()       # white noise is unvoiced at the default threshold
    # the longest waveform of one segment that still fits a test: more than one workgroup, a chunk that is not full
    c = PR.chunk_frames(ROOT)
    w = (rng.standard_normal((2 * c + 3) * hop) * 0.1 + np.sin(np.arange((2 * c + 3) * hop) * 2 * np.pi / 90.5)).astype(F)
    _check("two chunks and a bit", m.pitch_track(w), w, None, 2 * c + 3, hop, phonemes=False)


# ---- 5. batches = the rule and the stand-alone calls --------------------------------------------------------------------------------

def _ragged(g):
    nt = [(40, 150, 101), (7, 60, 0), (60, 130, 130), (1, 11, 5), (100, 160, 97)]
    return [(*_utt(g, 500 + i, N), T, None, None, tf) for i, (N, T, tf) in enumerate(nt)]


def _wishes():
    from zerovox_cpp_amd import capi
    return [capi.PitchTrack(30, 200, 300, 0.4, frames=True, phonemes=False), "phonemes", capi.PitchTrack(64, 512, 1024, 0.2), False, True]


def _track(wish):
    from zerovox_cpp_amd import capi
    return wish if isinstance(wish, capi.PitchTrack) else None


def _same_as_the_rule(bc, wishes, hop, what, want_wav=None, edges_only=False):
    for i, (w, n) in enumerate(bc.results()):
        if want_wav is not None:
            assert np.array_equal(LR.bits(w), LR.bits(want_wav[i])), (what, i)
        if bc.pitches[i] is None:
            assert wishes[i] is False
            continue
        p = bc.pitches[i]
        _check((what, i), p, w, bc.durations[i], len(w) // hop, hop, p.frames is not None, p.phonemes is not None, _track(wishes[i]))


def _scrub(bc):
    """overwrite the tables so that a run that wrote nothing cannot pass"""
    for p in bc.pitches:
        for a in ([] if p is None else [p.frames, p.phonemes]):
            if a is not None:
                a.fill(-7.0)


@pytest.mark.parametrize("fitted", [False, True])
def test_ragged_batch_replay_and_poison(env, fitted):
    m, g, _ = env
    hop = g.hop_size
    utts, wishes = _ragged(g), _wishes()
    m.set_graph_mode(False)
    plains = [w.copy() for w, _ in m.synthesize_batch(utts, fitted=fitted)]
    alone = []
    for i, u in enumerate(utts):
        res = m.synthesize(*u[:4], fitted=fitted, target_frames=u[6], return_durations=True, return_pitch=wishes[i])
        assert np.array_equal(LR.bits(res[0]), LR.bits(plains[i])), i
        alone.append(res[3] if wishes[i] is not False else None)
    bc = m.prepare_batch(utts, durations=True, fitted=fitted, return_pitch=wishes)
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
            first = [None if p is None else tuple(None if a is None else a.copy() for a in (p.frames, p.phonemes)) for p in bc.pitches]
            # the first and the last three frames of every utterance, explicitly: their spans must not see the neighbour's samples
            for i, (w, n) in enumerate(bc.results()):
                p, T = bc.pitches[i], len(w) // hop
                if p is not None and p.frames is not None:
                    params = PR.resolve(SR, hop, **_kw(_track(wishes[i])))
                    for f in sorted(set(list(range(min(3, T))) + list(range(max(T - 3, 0), T)))):
                        want = PR.frame(w, T * hop, f, SR, hop, params)[0]
                        assert PR.bits(p.frames[f]).tolist() == PR.bits(np.array(want, F)).tolist(), (i, f)
        for i, a in enumerate(alone):
            assert np.array_equal(LR.bits(bc.results()[i][0]), LR.bits(plains[i])), (what, i)
            for j, name in enumerate(("frames", "phonemes")):
                if a is None:
                    assert bc.pitches[i] is None
                    continue
                assert _same(getattr(bc.pitches[i], name), getattr(a, name)), (what, i, name)
                assert _same(getattr(bc.pitches[i], name), first[i][j]), (what, i, name)
    _scrub(bc)
    bc.begin(2)
    bc.end(2)
    for i, p in enumerate(bc.pitches):
        assert p is None or (_same(p.frames, first[i][0]) and _same(p.phonemes, first[i][1])), i
    # the plain batch next to it, and the _pitch entry point with pitch NULL / no table asked for
    for i, (w, n) in enumerate(m.synthesize_batch(utts, fitted=fitted)):
        assert np.array_equal(LR.bits(w), LR.bits(plains[i])), i
    from zerovox_cpp_amd import capi
    null = m.prepare_batch(utts, fitted=fitted)
    args = (m.h, null.n, null.ids_p, null.pun_p, null.sty_p, null.Ns, null.Ts, null.wav_p, null.nf)
    bad = (capi.PitchC * len(utts))(*[capi.PitchC(None, None, 1, 2, 3, -1.0)] * len(utts))      # no table: the parameters are not looked at
    for pit in (None, (capi.PitchC * len(utts))(), bad):
        for w in null.wavs:
            w.fill(7.0)
        m._chk(m.lib.zv_synthesize_batch_pitch(*args, None, None, None, null.targets, int(fitted), None, None, None, None, pit))
        for i, (w, n) in enumerate(null.results()):
            assert np.array_equal(LR.bits(w), LR.bits(plains[i])), i
    m.set_graph_mode(False)


def test_validation_names_the_utterance_and_the_field(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    utts = _ragged(g)[:2]
    for track, field in ((capi.PitchTrack(7, 50), "min_lag"), (capi.PitchTrack(50, 401), "max_lag"), (capi.PitchTrack(50, 50), "max_lag"),
                         (capi.PitchTrack(window=63), "window"), (capi.PitchTrack(window=1025), "window"),
                         (capi.PitchTrack(voiced_threshold=1.5), "voiced_threshold"), (capi.PitchTrack(voiced_threshold=float("nan")), "voiced_threshold")):
        with pytest.raises(capi.ZvError, match=r"zv_synthesize_batch_pitch: utterance 1: pitch %s" % field):
            m.synthesize_batch(utts, return_pitch=[True, track])
        with pytest.raises(capi.ZvError, match=r"zv_pitch_track: pitch %s" % field):
            m.pitch_track(np.zeros(g.hop_size, F), track)
    with pytest.raises(capi.ZvError, match="zv_pitch_track: T = "):
        m.pitch_track(np.zeros(g.hop_size * (m.max_frames() + 1), F))


def test_two_lanes_in_flight(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    hop = g.hop_size
    sets = [[(*_utt(g, 600 + 10 * k + i, 20 + 5 * i), 40 + 10 * k + 9 * i, None, None, 20 + 10 * k + 7 * i) for i in range(3)] for k in range(3)]
    wishes = [["frames", True, "phonemes"], [capi.PitchTrack(20, 100, 200, 0.3), False, True], ["phonemes", "frames", capi.PitchTrack(100, 500)]]
    batches = [m.prepare_batch(utts, durations=True, return_pitch=wishes[k]) for k, utts in enumerate(sets)]
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
                bc.first = [None if p is None else tuple(None if a is None else a.copy() for a in (p.frames, p.phonemes)) for p in bc.pitches]
            for i, p in enumerate(bc.pitches):
                assert p is None or (_same(p.frames, bc.first[i][0]) and _same(p.phonemes, bc.first[i][1])), (k, i, graph)
    m.set_graph_mode(False)


def test_batch_split_into_tail_groups(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    hop, T = g.hop_size, 900                                  # 16 utterances: 2 and 8 groups are different schedules (two utterances per group at least)
    tfs = [900, 500, 250, 37, 899, 1, 640, 333, 65, 700, 31, 32, 33, 450, 820, 128]
    utts = [(*_utt(g, 700 + i, 40 + 9 * i), T, None, None, tf) for i, tf in enumerate(tfs)]
    assert len(utts) * T * hop * 4 >= 16 << 20 and len(utts) // 2 >= 8
    # frames of two utterances and the phonemes of all but four are held to the rule; every table to the one-group run
    wishes = [[capi.PitchTrack(8, 64, 64, 0.3, phonemes=False), "phonemes", "phonemes", False][i % 4] for i in range(len(utts))]
    wishes[-1] = capi.PitchTrack(60, 120, 100, 0.5)
    m.set_graph_mode(False)
    with capi.switches(ZV_TAIL_GROUPS=1):
        bc = m.prepare_batch(utts, durations=True, fitted=True, return_pitch=wishes)
        bc.run()
        assert [n for _, n in bc.results()] == tfs
        for i in (0, 1, 5, 15):
            p, (w, n) = bc.pitches[i], bc.results()[i]
            _check(("one group", i), p, w, bc.durations[i], T, hop, p.frames is not None, p.phonemes is not None, _track(wishes[i]))
        one = [None if p is None else tuple(None if a is None else a.copy() for a in (p.frames, p.phonemes)) for p in bc.pitches]
        wavs = [w.copy() for w, _ in bc.results()]
    for groups in (2, 8):
        with capi.switches(ZV_TAIL_GROUPS=groups):
            for graph in (False, True):
                m.set_graph_mode(graph)
                bc = m.prepare_batch(utts, durations=True, fitted=True, return_pitch=wishes)
                for rep in range(2 if graph else 1):
                    m.poison(0x00 if rep else 0xFF)
                    _scrub(bc)
                    bc.run()
                    for i, (w, n) in enumerate(bc.results()):
                        assert n == tfs[i] and np.array_equal(LR.bits(w), LR.bits(wavs[i])), (groups, graph, rep, i)
                        if one[i] is None:
                            assert bc.pitches[i] is None
                            continue
                        for a, b in zip((bc.pitches[i].frames, bc.pitches[i].phonemes), one[i]):
                            assert _same(a, b), (groups, graph, rep, i)
            m.set_graph_mode(False)


# ---- 6. the profile; with envelope, volume and contour; the CLI -------------------------------------------------------------------------

def test_the_two_launches_appear_only_with_a_pitch_request(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    N = 30
    ids, puncts, style = _utt(g, 42, N)
    hop, T = g.hop_size, 150
    kw = dict(target_frames=100, volume=capi.Volume(1.0, 0.1, 0.5), envelope=capi.Envelope(_gains(N, 6), 1, 10, 10), return_contour=True)
    m.profile_begin()
    m.synthesize(ids, puncts, style, T, **kw)
    without = {s["name"]: s for s in m.profile_end()}
    m.profile_begin()
    m.synthesize(ids, puncts, style, T, return_pitch="phonemes", **kw)
    with_p = {s["name"]: s for s in m.profile_end()}
    assert "voc_pitch_frames" not in without and "voc_pitch_phonemes" not in without
    assert set(with_p) == set(without) | {"voc_pitch_frames", "voc_pitch_phonemes"}
    for k in without:
        assert with_p[k]["launches"] == without[k]["launches"], k
    names = list(with_p)
    assert names.index("voc_contour_phonemes") < names.index("voc_pitch_frames") == names.index("voc_pitch_phonemes") - 1
    assert with_p["voc_pitch_frames"]["launches"] == 1 and with_p["voc_pitch_phonemes"]["launches"] == 1
    assert with_p["voc_pitch_frames"]["algo_bytes"] == 4.0 * T * hop + 16.0 * T and with_p["voc_pitch_phonemes"]["algo_bytes"] == 8.0 * T + 8.0 * N


def test_envelope_volume_contour_and_pitch_in_one_call(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    N, T, hop = 40, 100, g.hop_size
    ids, puncts, style = _utt(g, 61, N)
    e = capi.Envelope(_gains(N, 7), 2, 5 * hop, 7 * hop + 3)
    vol = capi.Volume(0.8, 0.07, 0.5)
    for fitted in (False, True):
        ref, _, lv0, c0 = m.synthesize(ids, puncts, style, T, fitted=fitted, target_frames=80, envelope=e, volume=vol, return_levels=True,
                                       return_contour=True)
        ref = ref.copy()
        rows = None
        for graph in (False, True, True):
            m.set_graph_mode(graph)
            w, n, dur, lv, c, p = m.synthesize(ids, puncts, style, T, fitted=fitted, target_frames=80, envelope=e, volume=vol, return_durations=True,
                                               return_levels=True, return_contour=True, return_pitch=True)
            assert n == 80 and np.array_equal(LR.bits(w), LR.bits(ref)) and LR.level_bits(lv) == LR.level_bits(lv0)
            assert _same(c.frames, c0.frames) and _same(c.phonemes, c0.phonemes)
            if rows is None:
                _check((fitted, graph), p, w, dur, T, hop)
                rows = (p.frames, p.phonemes)
            assert _same(p.frames, rows[0]) and _same(p.phonemes, rows[1]), (fitted, graph)
        m.set_graph_mode(False)


def _read_tsv(path, last):
    lines = open(path).read().splitlines()
    assert lines[0] == "index\tf0_hz\t" + last
    rows = [l.split("\t") for l in lines[1:]]
    assert [int(r[0]) for r in rows] == list(range(len(rows)))
    return np.array([[F(r[1]), F(r[2])] for r in rows], F).reshape(len(rows), 2)


def test_cli_round_trip(env, tmp_path):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    N, hop = 40, g.hop_size
    ids, puncts, style = _utt(g, 71, N)
    utt = tmp_path / "utt.txt"
    utt.write_text(" ".join(map(str, ids.tolist())) + "\n" + " ".join(map(str, puncts.tolist())) + "\n" +
                   " ".join(repr(float(x)) for x in style.tolist()) + "\n")
    out, ff, pf = tmp_path / "pitch.wav", tmp_path / "pitch.tsv", tmp_path / "phonemes.tsv"
    cli = os.path.join(ROOT, "zerovox.cpp_amd", "zerovox")
    r = subprocess.run([cli, "-m", _M["path"], "-u", str(utt), "-o", str(out), "--fit", "--target-frames", "123", "--pitch", str(ff),
                        "--phoneme-pitch", str(pf), "--pitch-min-hz", "80", "--pitch-max-hz", "500", "--pitch-threshold", "0.25"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    track = capi.PitchTrack.from_hz(SR, 80, 500, voiced_threshold=0.25)
    assert (track.min_lag, track.max_lag) == (44, 275)
    w, nf, dur, p = m.synthesize(ids, puncts, style, g.max_seq_len, fitted=True, target_frames=123, return_durations=True, return_pitch=track)
    assert nf == 123
    _check("cli", p, w, dur, g.max_seq_len, hop, track=track)
    frames, phonemes = _read_tsv(ff, "strength"), _read_tsv(pf, "voiced")
    assert frames.shape == (g.max_seq_len, 2) and phonemes.shape == (N, 2)
    assert np.array_equal(PR.bits(frames), PR.bits(p.frames)) and np.array_equal(PR.bits(phonemes), PR.bits(p.phonemes))
