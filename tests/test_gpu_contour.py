"""-m gpu: the level contour (include/zerovox_amd.h "level contour") at the production geometry (the "medium" synthetic checkpoint,
hop 300; the two kernels depend on the hop and the lengths alone).

contour_frames_kernel and contour_phonemes_kernel run behind the vocoder's last step, the envelope and the volume passes, so every
expectation is the rule restated in Python (tests/contour_rule.py) applied to the waveform and the durations[] THE SAME CALL returned:
there is no tolerance anywhere, the bits must match.
  * a contour is a meter: waveform, n_frames, durations and level of plain, fitted, target, volume and envelope calls keep their bits
    with it (eager, graph capture, replay), and the plain call keeps its bits next to them;
  * every speech length 0 .. 64 of a small utterance, fitted (tails {0, 0}) and unfitted (tails measured like the speech);
  * capacities around one and two of the frames kernel's chunks;
  * a forced phoneme of 1 100 frames between phonemes of 0 and 1 frames; a capacity that cuts a phoneme in two;
  * the two launches appear in the profile only with a contour; the frame peaks' maximum is the zv_level peak;
  * batches (ragged with mixed wishes, graph replay on poisoned lanes, begin / end, two lanes in flight, tail groups) = the rule and
    the stand-alone calls; envelope, volume and contour in one call; the CLI's two files."""
import os
import subprocess

import numpy as np
import pytest

import contour_rule as CR
import level_rule as LR

pytestmark = pytest.mark.gpu

_M = {}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def env(ckpt):
    from zerovox_cpp_amd import capi
    if "m" not in _M:
        path, g, tensors = ckpt("medium")
        _M.update(m=capi.Model(path, 0), g=g, t=tensors, path=path)
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


def _check(what, contour, wav, dur, T, hop, frames=True, phonemes=True):
    """the tables of a call against the rule applied to the waveform and the durations the same call returned"""
    r = CR.rule(wav, T, hop, dur)
    assert (contour.frames is not None) == frames and (contour.phonemes is not None) == phonemes, what
    if frames:
        assert contour.frames.shape == (T, 2) and contour.frames.dtype == F
        bad = np.flatnonzero((CR.bits(contour.frames) != CR.bits(r["frames"])).any(axis=1))
        assert bad.size == 0, (what, "frames", bad.size, bad[:8], contour.frames[bad[:4]], r["frames"][bad[:4]])
    if phonemes:
        assert contour.phonemes.shape == (len(dur), 2) and contour.phonemes.dtype == F
        bad = np.flatnonzero((CR.bits(contour.phonemes) != CR.bits(r["phonemes"])).any(axis=1))
        assert bad.size == 0, (what, "phonemes", bad.size, bad[:8], contour.phonemes[bad[:4]], r["phonemes"][bad[:4]], np.asarray(dur)[bad[:4]])
    return r


# ---- 1. a contour is a meter ------------------------------------------------------------------------------------------------------

def test_a_contour_changes_no_other_result(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    N, T, hop = 40, 200, g.hop_size
    assert hop % 4 == 0
    ids, puncts, style = _utt(g, 11, N)
    kinds = dict(plain={}, fitted=dict(fitted=True), target=dict(target_frames=151), volume=dict(target_frames=120, volume=capi.Volume(1.3, 0.05, 0.4)),
                 envelope=dict(fitted=True, target_frames=133, envelope=capi.Envelope(_gains(N, 1), 2, 37, 53)))
    m.set_graph_mode(False)
    refs = {}
    for kind, kw in kinds.items():
        w, nf, dur, lv = m.synthesize(ids, puncts, style, T, return_durations=True, return_levels=True, **kw)
        refs[kind] = (w.copy(), nf, dur.copy(), LR.level_bits(lv))
    plain = m.synthesize(ids, puncts, style, T)[0].copy()
    assert np.array_equal(LR.bits(plain), LR.bits(refs["plain"][0]))
    for graph in (False, True):
        m.set_graph_mode(graph)
        for rep in range(2 if graph else 1):               # capture, then replay
            for kind, kw in kinds.items():
                for wish in (True, "frames", "phonemes"):
                    w, nf, dur, lv, c = m.synthesize(ids, puncts, style, T, return_durations=True, return_levels=True, return_contour=wish, **kw)
                    w0, nf0, dur0, lv0 = refs[kind]
                    assert nf == nf0 and dur.tolist() == dur0.tolist() and LR.level_bits(lv) == lv0, (kind, wish, graph, rep)
                    assert np.array_equal(LR.bits(w), LR.bits(w0)), (kind, wish, graph, rep)
                    _check((kind, wish, graph, rep), c, w, dur, T, hop, wish != "phonemes", wish != "frames")
                # without levels and durations the contour still describes the returned waveform
                w, nf, c = m.synthesize(ids, puncts, style, T, return_contour=True, **kw)
                assert np.array_equal(LR.bits(w), LR.bits(refs[kind][0])), (kind, graph, rep)
                _check((kind, "no levels", graph, rep), c, w, refs[kind][2], T, hop)
            # the plain call keeps its bits next to graphs captured with a contour, and return_contour=False asks for nothing
            res = m.synthesize(ids, puncts, style, T, return_contour=False)
            assert len(res) == 2 and np.array_equal(LR.bits(res[0]), LR.bits(plain)), (graph, rep)
    m.set_graph_mode(False)


# ---- 2. every length, the chunk edges -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fitted", [False, True])
def test_every_speech_length_of_a_small_utterance(env, fitted):
    m, g, _ = env
    N, T, hop = 16, 64, g.hop_size
    ids, puncts, style = _utt(g, 21, N)
    seen = set()
    for nf in range(0, T + 1):
        kw = dict(phonemes=dict(duration_frames=np.zeros(N, np.int32))) if nf == 0 else dict(target_frames=nf)
        w, n, dur, c = m.synthesize(ids, puncts, style, T, fitted=fitted, return_durations=True, return_contour=True, **kw)
        assert n == nf == int(dur.sum())
        _check((fitted, nf), c, w, dur, T, hop)
        tail = CR.bits(c.frames[nf:])
        if fitted:
            assert not tail.any(), nf                          # fitted zeros give {0, 0}
        else:
            assert tail[:, 1].all(), nf                        # an unfitted tail is measured like the speech: no frame of it is silent
        seen.add(CR.bits(c.phonemes).tobytes())
    assert len(seen) > 60


def test_capacities_around_the_frames_kernels_chunk(env):
    m, g, _ = env
    hop, c = g.hop_size, CR.chunk_frames(ROOT)
    assert c * hop == LR.chunk_samples(ROOT)
    N = 16
    ids, puncts, style = _utt(g, 22, N)
    for k in (1, 2):
        for T in (c * k - 1, c * k, c * k + 1):
            for fitted in (False, True):
                for tf in (T, T - 3):
                    w, n, dur, ct = m.synthesize(ids, puncts, style, T, fitted=fitted, target_frames=tf, return_durations=True, return_contour=True)
                    assert n == tf
                    _check((T, fitted, tf), ct, w, dur, T, hop)
                    assert CR.bits(ct.frames[:tf, 1]).all()
                    if tf < T:
                        assert CR.bits(ct.frames[tf:, 1]).all() != fitted and CR.bits(ct.frames[tf:]).any() != fitted


# ---- 3. long forced phonemes, a truncating capacity ---------------------------------------------------------------------------------

def test_a_forced_phoneme_longer_than_a_wave_can_stride_once(env):
    m, g, _ = env
    N, T, hop = 16, 1200, g.hop_size
    ids, puncts, style = _utt(g, 31, N)
    forced = np.array([3, 0, 1100, 1, 0, 0, 7, 1, 0, 2, 64, 0, 1, 5, 0, 9], np.int32)          # 1 193 frames
    assert forced[2] > 64 * 16 and int(forced.sum()) < T
    for fitted in (False, True):
        w, nf, dur, c = m.synthesize(ids, puncts, style, T, fitted=fitted, phonemes=dict(duration_frames=forced), return_durations=True,
                                     return_contour=True)
        assert nf == int(forced.sum()) and dur.tolist() == forced.tolist()
        r = _check(("long", fitted), c, w, dur, T, hop)
        assert not CR.bits(c.phonemes[forced == 0]).any() and CR.bits(c.phonemes[forced > 0, 1]).all()
        assert sum(r["pS"]) == sum(r["S"][:nf]) and r["pS"][2] == sum(r["S"][3:1103])


def test_a_capacity_that_cuts_a_phoneme_in_two(env):
    m, g, _ = env
    N, T, hop = 16, 64, g.hop_size
    ids, puncts, style = _utt(g, 32, N)
    forced = np.array([0, 9, 0, 0, 3, 1, 12, 0, 7, 40, 0, 5, 9, 0, 2, 4], np.int32)          # 92 frames: phoneme 9 is cut by T = 64
    for fitted in (False, True):
        w, nf, dur, c = m.synthesize(ids, puncts, style, T, fitted=fitted, phonemes=dict(duration_frames=forced), return_durations=True,
                                     return_contour=True)
        assert nf == T and dur.tolist() == forced[:9].tolist() + [64 - int(forced[:9].sum())] + [0] * 6
        _check(("cut", fitted), c, w, dur, T, hop)
        assert CR.bits(c.phonemes[9, 1]) and not CR.bits(c.phonemes[10:]).any()           # the rest of the utterance has no frame


# ---- 4. the profile, the peak -----------------------------------------------------------------------------------------------------------

def test_the_two_launches_appear_only_with_a_contour(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    N = 30
    ids, puncts, style = _utt(g, 42, N)
    hop, T = g.hop_size, 150
    kw = dict(target_frames=100, volume=capi.Volume(1.0, 0.1, 0.5), envelope=capi.Envelope(_gains(N, 6), 1, 10, 10))
    m.profile_begin()
    m.synthesize(ids, puncts, style, T, **kw)
    without = {s["name"]: s for s in m.profile_end()}
    m.profile_begin()
    m.synthesize(ids, puncts, style, T, return_contour="phonemes", **kw)
    with_c = {s["name"]: s for s in m.profile_end()}
    assert "voc_contour_frames" not in without and "voc_contour_phonemes" not in without
    assert set(with_c) == set(without) | {"voc_contour_frames", "voc_contour_phonemes"}
    for k in without:
        assert with_c[k]["launches"] == without[k]["launches"], k
    names = list(with_c)
    assert names.index("voc_level_apply") < names.index("voc_contour_frames") == names.index("voc_contour_phonemes") - 1
    assert with_c["voc_contour_frames"]["launches"] == 1 and with_c["voc_contour_phonemes"]["launches"] == 1
    assert with_c["voc_contour_frames"]["algo_bytes"] == 4.0 * T * hop and with_c["voc_contour_phonemes"]["algo_bytes"] == 16.0 * T + 8.0 * N


def test_the_frame_peaks_maximum_is_the_level_meters_peak(env):
    m, g, _ = env
    N, T, hop = 40, 200, g.hop_size
    ids, puncts, style = _utt(g, 43, N)
    for fitted in (False, True):
        for nf in (1, 77, 200):
            w, n, lv, c = m.synthesize(ids, puncts, style, T, fitted=fitted, target_frames=nf, return_levels=True, return_contour="frames")
            assert n == nf and lv.gain == 1.0
            assert CR.bits(c.frames[:nf, 1].max())[()] == LR.level_bits(lv)[1]
            S, P = CR.frame_totals(w, T, hop)
            assert LR.level_bits(LR.report(sum(S[:nf]), nf * hop, max(P[:nf]))[1]) == LR.level_bits(lv)


# ---- 5. batches = the rule and the stand-alone calls --------------------------------------------------------------------------------

def _ragged(g):
    nt = [(40, 300, 201), (7, 60, 0), (60, 257, 257), (1, 11, 5), (100, 310, 97)]
    return [(*_utt(g, 500 + i, N), T, None, None, tf) for i, (N, T, tf) in enumerate(nt)]


WISHES = ["frames", "phonemes", True, False, True]


def _same_as_the_rule(bc, wishes, hop, what, want_wav=None):
    for i, (w, n) in enumerate(bc.results()):
        if want_wav is not None:
            assert np.array_equal(LR.bits(w), LR.bits(want_wav[i])), (what, i)
        f, p = wishes[i] in (True, "frames"), wishes[i] in (True, "phonemes")
        if not (f or p):
            assert bc.contours[i] is None
            continue
        assert int(bc.durations[i].sum()) == n
        _check((what, i), bc.contours[i], w, bc.durations[i], len(w) // hop, hop, f, p)


def _scrub(bc):
    """overwrite the tables so that a run that wrote nothing cannot pass"""
    for c in bc.contours:
        for a in ([] if c is None else [c.frames, c.phonemes]):
            if a is not None:
                a.fill(-7.0)


@pytest.mark.parametrize("fitted", [False, True])
def test_ragged_batch_replay_and_poison(env, fitted):
    m, g, _ = env
    hop = g.hop_size
    utts = _ragged(g)
    m.set_graph_mode(False)
    plains = [w.copy() for w, _ in m.synthesize_batch(utts, fitted=fitted)]
    alone = []
    for i, u in enumerate(utts):
        res = m.synthesize(*u[:4], fitted=fitted, target_frames=u[6], return_durations=True, return_contour=WISHES[i])
        assert np.array_equal(LR.bits(res[0]), LR.bits(plains[i])), i
        if WISHES[i]:
            _check(("alone", i), res[3], res[0], res[2], u[3], hop, WISHES[i] != "phonemes", WISHES[i] != "frames")
        alone.append(res[3] if WISHES[i] else None)
    bc = m.prepare_batch(utts, durations=True, fitted=fitted, return_contour=WISHES)
    steps = [("eager", False, None), ("graph capture", True, None), ("graph replay on a lane poisoned with 0xFF", True, 0xFF),
             ("graph replay on a lane poisoned with 0x00", True, 0x00)]
    for what, graph, poison in steps:
        m.set_graph_mode(graph)
        if poison is not None:
            m.poison(poison)
        _scrub(bc)
        bc.run()
        _same_as_the_rule(bc, WISHES, hop, what, plains)
        for i, a in enumerate(alone):                        # the batch equals the stand-alone calls
            for name in ("frames", "phonemes"):
                if a is not None and getattr(a, name) is not None:
                    assert np.array_equal(CR.bits(getattr(bc.contours[i], name)), CR.bits(getattr(a, name))), (what, i, name)
    _scrub(bc)
    bc.begin(2)
    bc.end(2)
    _same_as_the_rule(bc, WISHES, hop, "begin / end on lane 2, graph", plains)
    # the plain batch next to it, and the _contour entry point with contour NULL / no table asked for
    for i, (w, n) in enumerate(m.synthesize_batch(utts, fitted=fitted)):
        assert np.array_equal(LR.bits(w), LR.bits(plains[i])), i
    from zerovox_cpp_amd import capi
    null = m.prepare_batch(utts, fitted=fitted)
    args = (m.h, null.n, null.ids_p, null.pun_p, null.sty_p, null.Ns, null.Ts, null.wav_p, null.nf)
    for ctr in (None, (capi.ContourC * len(utts))()):
        for w in null.wavs:
            w.fill(7.0)
        m._chk(m.lib.zv_synthesize_batch_contour(*args, None, None, None, null.targets, int(fitted), None, None, None, ctr))
        for i, (w, n) in enumerate(null.results()):
            assert np.array_equal(LR.bits(w), LR.bits(plains[i])), i
    m.set_graph_mode(False)


def test_two_lanes_in_flight(env):
    m, g, _ = env
    hop = g.hop_size
    sets = [[(*_utt(g, 600 + 10 * k + i, 20 + 5 * i), 120 + 40 * k + 9 * i, None, None, 60 + 30 * k + 7 * i) for i in range(3)] for k in range(3)]
    wishes = [["frames", True, "phonemes"], [True, False, True], ["phonemes", "frames", True]]
    batches = [m.prepare_batch(utts, durations=True, return_contour=wishes[k]) for k, utts in enumerate(sets)]
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
            _same_as_the_rule(bc, wishes[k], hop, f"lanes, batch {k}, graph={graph}")
    m.set_graph_mode(False)


def test_batch_split_into_tail_groups(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    hop, T = g.hop_size, 900                                  # 16 utterances: 2 and 8 groups are different schedules (two utterances per group at least)
    tfs = [900, 500, 250, 37, 899, 1, 640, 333, 65, 700, 31, 32, 33, 450, 820, 128]
    utts = [(*_utt(g, 700 + i, 40 + 9 * i), T, None, None, tf) for i, tf in enumerate(tfs)]
    assert len(utts) * T * hop * 4 >= 16 << 20 and len(utts) // 2 >= 8
    wishes = [[True, "frames", "phonemes", False][i % 4] for i in range(len(utts))]
    wishes[-1] = True
    m.set_graph_mode(False)
    with capi.switches(ZV_TAIL_GROUPS=1):
        bc = m.prepare_batch(utts, durations=True, return_contour=wishes)
        bc.run()
        assert [n for _, n in bc.results()] == tfs
        _same_as_the_rule(bc, wishes, hop, "one group")          # the rule, once; the grouped runs are held to these bits
        one = [None if c is None else tuple(None if a is None else a.copy() for a in (c.frames, c.phonemes)) for c in bc.contours]
        wavs = [w.copy() for w, _ in bc.results()]
    for groups in (2, 8):
        with capi.switches(ZV_TAIL_GROUPS=groups):
            for graph in (False, True):
                m.set_graph_mode(graph)
                bc = m.prepare_batch(utts, durations=True, return_contour=wishes)
                for rep in range(2 if graph else 1):
                    m.poison(0x00 if rep else 0xFF)
                    _scrub(bc)
                    bc.run()
                    for i, (w, n) in enumerate(bc.results()):
                        assert n == tfs[i] and np.array_equal(LR.bits(w), LR.bits(wavs[i])), (groups, graph, rep, i)
                        if one[i] is None:
                            assert bc.contours[i] is None
                            continue
                        for a, b in zip((bc.contours[i].frames, bc.contours[i].phonemes), one[i]):
                            assert (a is None) == (b is None) and (a is None or np.array_equal(CR.bits(a), CR.bits(b))), (groups, graph, rep, i)
            m.set_graph_mode(False)


# ---- 6. with envelope and volume; the CLI ---------------------------------------------------------------------------------------------

def test_the_contour_is_that_of_the_scaled_waveform(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    N, T, hop = 40, 200, g.hop_size
    ids, puncts, style = _utt(g, 61, N)
    e = capi.Envelope(_gains(N, 7), 2, 5 * hop, 7 * hop + 3)
    vol = capi.Volume(0.8, 0.07, 0.5)
    for fitted in (False, True):
        plain, nf = m.synthesize(ids, puncts, style, T, fitted=fitted, target_frames=150)
        plain = plain.copy()
        ref, _, lv0 = m.synthesize(ids, puncts, style, T, fitted=fitted, target_frames=150, envelope=e, volume=vol, return_levels=True)
        ref = ref.copy()
        assert not np.array_equal(LR.bits(ref), LR.bits(plain))
        for graph in (False, True, True):
            m.set_graph_mode(graph)
            w, n, dur, lv, c = m.synthesize(ids, puncts, style, T, fitted=fitted, target_frames=150, envelope=e, volume=vol, return_durations=True,
                                            return_levels=True, return_contour=True)
            assert n == nf == 150 and np.array_equal(LR.bits(w), LR.bits(ref)) and LR.level_bits(lv) == LR.level_bits(lv0)
            _check((fitted, graph), c, w, dur, T, hop)
            # what the meter sees is what the ceiling promised: no frame of the speech peaks above it, and the ceiling was reached
            assert c.frames[:nf, 1].max() <= F(0.5) and c.phonemes[:, 1].max() == c.frames[:nf, 1].max() > F(0.49)
        m.set_graph_mode(False)


def _read_tsv(path):
    lines = open(path).read().splitlines()
    assert lines[0] == "index\trms\tpeak"
    rows = [l.split("\t") for l in lines[1:]]
    assert [int(r[0]) for r in rows] == list(range(len(rows)))
    return np.array([[F(r[1]), F(r[2])] for r in rows], F).reshape(len(rows), 2)


def test_cli_round_trip(env, tmp_path):
    m, g, _ = env
    N, hop = 40, g.hop_size
    ids, puncts, style = _utt(g, 71, N)
    utt = tmp_path / "utt.txt"
    utt.write_text(" ".join(map(str, ids.tolist())) + "\n" + " ".join(map(str, puncts.tolist())) + "\n" +
                   " ".join(repr(float(x)) for x in style.tolist()) + "\n")
    out, cf, pf = tmp_path / "contour.wav", tmp_path / "contour.tsv", tmp_path / "phonemes.tsv"
    cli = os.path.join(ROOT, "zerovox.cpp_amd", "zerovox")
    r = subprocess.run([cli, "-m", _M["path"], "-u", str(utt), "-o", str(out), "--fit", "--target-frames", "123", "--contour", str(cf),
                        "--phoneme-levels", str(pf)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    w, nf, dur, c = m.synthesize(ids, puncts, style, g.max_seq_len, fitted=True, target_frames=123, return_durations=True, return_contour=True)
    assert nf == 123
    _check("cli", c, w, dur, g.max_seq_len, hop)
    frames, phonemes = _read_tsv(cf), _read_tsv(pf)
    assert frames.shape == (g.max_seq_len, 2) and phonemes.shape == (N, 2)
    assert np.array_equal(CR.bits(frames), CR.bits(c.frames)) and np.array_equal(CR.bits(phonemes), CR.bits(c.phonemes))
    assert CR.bits(frames[:nf, 1]).all() and not CR.bits(frames[nf:]).any()
