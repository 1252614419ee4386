"""-m gpu: the amplitude envelope (include/zerovox_amd.h "amplitude envelope") at the production geometry.

env_knots_kernel and env_apply_kernel run behind the vocoder's last step, ahead of the volume passes, so every expectation comes from
the GPU's own waveform and durations[] of the same call WITHOUT an envelope, pushed through the rule restated in Python
(tests/envelope_rule.py) and, where the call carries a volume, then through tests/level_rule.py: waveform and level must match bit
for bit.  These tests are also the check that gfx950's f64 quotient and products round as the host's do.
  * identity: envelope = NULL, a zeroed struct and all-ones gains give the _volume call's bits (eager, graph capture and replay);
  * every speech length 0 .. 64 of a small utterance, fitted and unfitted; r in {0, 1, 7, 64} x fades of 0, 1, hop - 1, n, n + 5;
  * forced durations with zeros and a truncating T; prosody, per-phoneme controls, a target, an envelope and a volume in one call;
  * run-shortened vocoding / decoding on and off; the two launches appear in the profile only with an envelope;
  * batches (ragged, graph replay with new values, poisoned lanes, two lanes in flight, tail groups) = the rule and the stand-alone calls;
  * validation messages and the CLI flags.
A segment whose first sample is not 16-byte aligned cannot occur here: a segment starts row0 * hop floats behind a 256-byte aligned
base and every synthetic checkpoint's hop is 300, a multiple of 4 (asserted below), so the kernels' 4-byte path — row0 * hop or a
length that is no multiple of 4 — is reached by no call the library can make on these checkpoints; envelope.h's arithmetic for it is the
same function, held to the restatement at hops 1, 3, 5 and 7 on the CPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import envelope_rule as ER
import level_rule as LR

pytestmark = pytest.mark.gpu

ZV_ERR_ARG = 5
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


def _vt(v):
    return LR.IDENTITY if v is None else (v.gain, v.target_rms, v.peak_ceiling)


def _check(what, w, level, plain, dur, T, hop, envelope, vol=None):
    """waveform (and level, where the call measured one) against the two rules applied to the plain call's waveform and timings"""
    r = ER.rule(plain, dur, T, hop, ER.as_tuple(envelope))
    want = r["out"]
    if level is not None:
        v = LR.rule(want, r["nf"] * hop, _vt(vol))
        want = v["out"]
        assert LR.level_bits(level) == LR.level_bits(v["level"]) and level.reserved == 0, (what, "level", level, v["level"])
    bad = np.flatnonzero(LR.bits(w) != LR.bits(want))
    assert bad.size == 0, (what, "waveform", bad.size, bad[:8], w[bad[:4]], want[bad[:4]], r["nf"])
    return r


def _gains(N, seed, lo=0.0, hi=4.0):
    g = np.random.default_rng(seed).random(N) * (hi - lo) + lo
    g[::5] = 0.0
    g[3::7] = 16.0
    return g.astype(F)


# ---- 1. identity ------------------------------------------------------------------------------------------------------------

def test_identities_give_the_volume_calls_bits(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    N, T, hop = 16, 64, g.hop_size
    assert hop % 4 == 0                                          # see the module's docstring
    ids, puncts, style = _utt(g, 11, N)
    vol = capi.Volume(1.3, 0.05, 0.4)
    for fitted in (False, True):
        m.set_graph_mode(False)
        ref, nf = m.synthesize(ids, puncts, style, T, fitted=fitted, target_frames=41)
        ref = ref.copy()
        refv, _, lvv = m.synthesize(ids, puncts, style, T, fitted=fitted, target_frames=41, volume=vol, return_levels=True)
        refv = refv.copy()
        for graph in (False, True):
            m.set_graph_mode(graph)
            for _ in range(2 if graph else 1):               # capture, then replay
                # the _envelope entry point itself with envelope NULL, without and with a volume
                a, b, c = (np.ascontiguousarray(x) for x in (ids, puncts, style))
                w, n, lv = np.full(T * hop, 7.0, F), C.c_uint32(0), capi.Level()
                m._chk(m.lib.zv_synthesize_envelope(m.h, capi._ptr(a), capi._ptr(b), capi._ptr(c), N, T, capi._ptr(w), C.byref(n), None, None,
                                                    None, 41, int(fitted), None, None, None))
                assert n.value == nf and np.array_equal(LR.bits(w), LR.bits(ref)), (fitted, graph)
                m._chk(m.lib.zv_synthesize_envelope(m.h, capi._ptr(a), capi._ptr(b), capi._ptr(c), N, T, capi._ptr(w), C.byref(n), None, None,
                                                    None, 41, int(fitted), C.byref(vol), C.byref(lv), None))
                assert np.array_equal(LR.bits(w), LR.bits(refv)) and LR.level_bits(lv) == LR.level_bits(lvv), (fitted, graph)
                for what, e in (("zeroed struct", capi.Envelope()), ("all-ones gains", capi.Envelope(np.ones(N, F))),
                                ("all-ones gains, r = 5", capi.Envelope(np.ones(N, F), 5)), ("no gains, r = 64", capi.Envelope(None, 64))):
                    w, n = m.synthesize(ids, puncts, style, T, fitted=fitted, target_frames=41, envelope=e)
                    assert n == nf and np.array_equal(LR.bits(w), LR.bits(ref)), (what, fitted, graph)
                    w, n, lv = m.synthesize(ids, puncts, style, T, fitted=fitted, target_frames=41, envelope=e, volume=vol, return_levels=True)
                    assert np.array_equal(LR.bits(w), LR.bits(refv)) and LR.level_bits(lv) == LR.level_bits(lvv), (what, fitted, graph)
                # and the plain call still gives its bits next to graphs captured with an envelope
                w, n = m.synthesize(ids, puncts, style, T, fitted=fitted, target_frames=41)
                assert n == nf and np.array_equal(LR.bits(w), LR.bits(ref)), (fitted, graph)
    m.set_graph_mode(False)


# ---- 2. every length, the parameter sweep -----------------------------------------------------------------------------------

@pytest.mark.parametrize("fitted", [False, True])
def test_every_speech_length_of_a_small_utterance(env, fitted):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    N, T, hop = 16, 64, g.hop_size
    ids, puncts, style = _utt(g, 21, N)
    e = capi.Envelope(_gains(N, 1), 2, 37, 53)
    vol = capi.Volume(1.3, 0.05, 0.4)
    seen = set()
    for nf in range(0, T + 1):
        kw = dict(phonemes=dict(duration_frames=np.zeros(N, np.int32))) if nf == 0 else dict(target_frames=nf)
        plain, n0, dur = m.synthesize(ids, puncts, style, T, fitted=fitted, return_durations=True, **kw)
        plain = plain.copy()
        assert n0 == nf == int(dur.sum())
        if nf % 2:
            w, n, lv = m.synthesize(ids, puncts, style, T, fitted=fitted, envelope=e, volume=vol, return_levels=True, **kw)
        else:
            (w, n), lv = m.synthesize(ids, puncts, style, T, fitted=fitted, envelope=e, **kw), None
        assert n == nf
        r = _check((fitted, nf), w, lv, plain, dur, T, hop, e, vol)
        seen.add(tuple(r["B"]))
        if fitted or nf == 0:
            assert not w[nf * hop:].any()                      # fitted zeros stay zero; a fade-out silences what follows the speech
        if nf == 0 and not fitted:
            w0, _ = m.synthesize(ids, puncts, style, T, envelope=capi.Envelope(_gains(N, 1), 2, 37, 0), **kw)
            assert np.array_equal(LR.bits(w0), LR.bits(plain)) and plain.any()      # nothing to fade: the bits stay
    assert len(seen) > 60


def test_ramp_and_fade_sweep(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    N, T, nf, hop = 16, 64, 50, g.hop_size
    ids, puncts, style = _utt(g, 22, N)
    plain, n0, dur = m.synthesize(ids, puncts, style, T, target_frames=nf, return_durations=True)
    plain = plain.copy()
    n = nf * hop
    assert n0 == nf and plain[n:].any()
    gains = _gains(N, 2)
    for r in (0, 1, 7, 64):
        for Fi in (0, 1, hop - 1, n, n + 5):
            for Fo in (0, 1, hop - 1, n, n + 5):
                e = capi.Envelope(gains, r, Fi, Fo)
                w, n1 = m.synthesize(ids, puncts, style, T, target_frames=nf, envelope=e)
                assert n1 == nf
                res = _check((r, Fi, Fo), w, None, plain, dur, T, hop, e)
                if Fo == 0:                                    # an unfitted tail is scaled by the last knot, like the end of the speech
                    last = F(np.float64(res["B"][nf] * hop) / np.float64(2 * (2 * r + 1) * hop * 65536))
                    t0 = max(n, Fi)                            # (a fade-in longer than the speech is still rising behind it)
                    assert np.array_equal(LR.bits(w[t0:]), LR.bits(plain[t0:] * last))
                else:
                    assert not w[n - 1:].any()


# ---- 3. forced durations, every control at once -----------------------------------------------------------------------------

def test_forced_durations_with_zeros_and_a_truncating_capacity(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    N, T, hop = 16, 64, g.hop_size
    ids, puncts, style = _utt(g, 31, N)
    forced = np.array([0, 9, 0, 0, 3, 1, 12, 0, 7, 40, 0, 5, 9, 0, 2, 4], np.int32)          # 92 frames: phoneme 9 is cut by T = 64
    for fitted in (False, True):
        plain, nf, dur = m.synthesize(ids, puncts, style, T, fitted=fitted, phonemes=dict(duration_frames=forced), return_durations=True)
        plain = plain.copy()
        assert nf == T and dur.tolist() == forced[:9].tolist() + [64 - int(forced[:9].sum())] + [0] * 6
        for r in (0, 3, 64):
            e = capi.Envelope(_gains(N, 3 + r), r, 100, 2 * hop + 1)
            w, n, lv = m.synthesize(ids, puncts, style, T, fitted=fitted, phonemes=dict(duration_frames=forced), envelope=e,
                                    volume=capi.Volume(1.0, 0.0, 0.3), return_levels=True)
            assert n == nf
            _check((fitted, r), w, lv, plain, dur, T, hop, e, capi.Volume(1.0, 0.0, 0.3))


def test_every_control_in_one_call(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    N, T, hop = 16, 64, g.hop_size
    ids, puncts, style = _utt(g, 32, N)
    pc = dict(duration_frames=np.where(np.arange(N) % 4 == 1, 3, -1).astype(np.int32), duration_scale=np.linspace(0.5, 2.0, N).astype(F),
              pitch_shift=np.linspace(-0.5, 0.5, N).astype(F), energy_shift=np.linspace(0.3, -0.3, N).astype(F))
    kw = dict(prosody=capi.Prosody(1.2, 0.9, 0.1, 1.1, -0.1), phonemes=pc, target_frames=57)
    vol = capi.Volume(0.8, 0.07, 0.5)
    e = capi.Envelope(_gains(N, 4), 1, 2 * hop, 3 * hop + 7)
    for fitted in (False, True):
        for graph in (False, True, True):
            m.set_graph_mode(False)
            plain, nf, dur = m.synthesize(ids, puncts, style, T, fitted=fitted, return_durations=True, **kw)
            plain = plain.copy()
            assert nf == 57
            m.set_graph_mode(graph)
            w, n, dur2, lv = m.synthesize(ids, puncts, style, T, fitted=fitted, return_durations=True, envelope=e, volume=vol, return_levels=True, **kw)
            assert n == nf and dur2.tolist() == dur.tolist()
            _check((fitted, graph), w, lv, plain, dur, T, hop, e, vol)
    m.set_graph_mode(False)


# ---- 4. run-shortened paths, the profile ------------------------------------------------------------------------------------

def test_unfitted_with_run_shortening_on_and_off(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    N, T, nf, hop = 30, 600, 100, g.hop_size
    ids, puncts, style = _utt(g, 41, N)
    e = capi.Envelope(_gains(N, 5), 3, 480, 480)
    vol = capi.Volume(1.5, 0.06, 0.5)
    plain, n0, dur = m.synthesize(ids, puncts, style, T, target_frames=nf, return_durations=True)
    plain = plain.copy()
    assert n0 == nf and plain[nf * hop:].any()
    for voc_runs in (2, 0):                                    # 2: at any size (1, the default, takes batches only)
        for dec_runs in (2, 0):
            with capi.switches(ZV_VOC_RUNS=voc_runs, ZV_DEC_RUNS=dec_runs):
                for graph in (False, True):
                    m.set_graph_mode(graph)
                    w, n, lv = m.synthesize(ids, puncts, style, T, target_frames=nf, envelope=e, volume=vol, return_levels=True)
                    assert n == nf
                    _check((voc_runs, dec_runs, graph), w, lv, plain, dur, T, hop, e, vol)
                    tab = m.voc_runs()
                    assert (tab.shape[0] == 1 and tab[0, 3] > 0) if voc_runs else tab.shape[0] == 0      # the run was taken, or not
                m.set_graph_mode(False)


def test_the_two_launches_appear_only_with_an_envelope(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    N = 30
    ids, puncts, style = _utt(g, 42, N)
    hop, T = g.hop_size, 150
    vol = capi.Volume(1.0, 0.1, 0.5)
    m.profile_begin()
    m.synthesize(ids, puncts, style, T, target_frames=100, volume=vol)
    plain = {s["name"]: s for s in m.profile_end()}
    m.profile_begin()
    m.synthesize(ids, puncts, style, T, target_frames=100, volume=vol, envelope=capi.Envelope(_gains(N, 6), 1, 10, 10))
    with_env = {s["name"]: s for s in m.profile_end()}
    assert "voc_env_knots" not in plain and "voc_env_apply" not in plain
    assert set(with_env) == set(plain) | {"voc_env_knots", "voc_env_apply"}
    for k in plain:
        assert with_env[k]["launches"] == plain[k]["launches"], k
    names = list(with_env)
    assert names.index("voc_env_knots") + 1 == names.index("voc_env_apply") < names.index("voc_level_measure")
    assert with_env["voc_env_knots"]["launches"] == 1 and with_env["voc_env_apply"]["launches"] == 1
    assert with_env["voc_env_apply"]["algo_bytes"] == 8.0 * T * hop and with_env["voc_env_knots"]["algo_bytes"] == 4.0 * (T + 1) + 8.0 * N


# ---- 5. batches = the rule and the stand-alone calls ------------------------------------------------------------------------

def _ragged(g):
    nt = [(40, 300, 201), (7, 60, 0), (60, 257, 257), (1, 11, 5), (100, 310, 97)]
    return [(*_utt(g, 500 + i, N), T, None, None, tf) for i, (N, T, tf) in enumerate(nt)]


def _batch_controls(utts, hop, salt):
    """per-utterance envelopes and volumes, some None"""
    from zerovox_cpp_amd import capi
    envs, vols = [], []
    for i, u in enumerate(utts):
        N = len(u[0])
        k = i + salt
        envs.append(None if k % 4 == 1 else capi.Envelope(None if k % 4 == 3 else _gains(N, 10 * salt + i), [0, 2, 64, 1, 7][k % 5],
                                                          [0, 150, hop - 1, 5000][k % 4], [977, 0, 1, 40000][k % 4]))
        vols.append(None if k % 3 == 0 else capi.Volume(1.0 + 0.25 * k, 0.05 if k % 2 else 0.0, 0.5))
    return envs, vols


def _same_as(bc, plains, envs, vols, hop, what):
    for i, ((w, n), lv) in enumerate(zip(bc.results(), bc.levels)):
        wav, nf, dur = plains[i]
        assert n == nf, (what, i)
        _check((what, i), w, lv, wav, dur, len(wav) // hop, hop, envs[i], vols[i])


@pytest.mark.parametrize("fitted", [False, True])
def test_ragged_batch_replay_and_poison(env, fitted):
    m, g, _ = env
    hop = g.hop_size
    utts = _ragged(g)
    m.set_graph_mode(False)
    plains = [(w.copy(), n, d) for w, n, d in m.synthesize_batch(utts, return_durations=True, fitted=fitted)]
    envs1, vols1 = _batch_controls(utts, hop, 0)
    envs2, vols2 = _batch_controls(utts, hop, 1)
    assert any(e is None for e in envs1) and any(v is None for v in vols1)
    # the stand-alone envelope calls follow the rule, and so does the batch: the batch equals the stand-alone calls
    alone = []
    for i, u in enumerate(utts):
        if vols1[i] is None:
            (w, n), lv = m.synthesize(*u[:4], fitted=fitted, target_frames=u[6], envelope=envs1[i]), None
        else:
            w, n, lv = m.synthesize(*u[:4], fitted=fitted, target_frames=u[6], envelope=envs1[i], volume=vols1[i], return_levels=True)
        assert n == plains[i][1]
        _check(("alone", i), w, lv, plains[i][0], plains[i][2], u[3], hop, envs1[i], vols1[i])
        alone.append(w.copy())
    bc = m.prepare_batch(utts, fitted=fitted, volume=vols1, envelope=envs1)
    bc.run()
    _same_as(bc, plains, envs1, vols1, hop, "eager")
    for i, (w, _) in enumerate(bc.results()):
        if vols1[i] is not None:
            assert np.array_equal(LR.bits(w), LR.bits(alone[i])), i
    m.set_graph_mode(True)
    bc.run()
    _same_as(bc, plains, envs1, vols1, hop, "graph capture")
    m.poison(0xFF)
    bc.run()
    _same_as(bc, plains, envs1, vols1, hop, "graph replay on a lane poisoned with 0xFF")
    for i in range(len(utts)):
        bc.set_envelope(i, envs2[i])
        bc.set_volume(i, vols2[i])
    m.poison(0x00)
    bc.run()
    _same_as(bc, plains, envs2, vols2, hop, "graph replay with new gains and fades on a lane poisoned with 0x00")
    bc.begin(2)
    bc.end(2)
    _same_as(bc, plains, envs2, vols2, hop, "begin / end, graph")
    # an envelope batch without volume, and the plain batch next to it
    eo = m.prepare_batch(utts, fitted=fitted, envelope=envs1)
    eo.run()
    for i, (w, n) in enumerate(eo.results()):
        _check(("envelope only", i), w, None, plains[i][0], plains[i][2], utts[i][3], hop, envs1[i])
    for i, (w, n) in enumerate(m.synthesize_batch(utts, fitted=fitted)):
        assert n == plains[i][1] and np.array_equal(LR.bits(w), LR.bits(plains[i][0])), i
    # the _envelope entry point with envelope NULL is the _volume call
    null = m.prepare_batch(utts, fitted=fitted)
    args = (m.h, null.n, null.ids_p, null.pun_p, null.sty_p, null.Ns, null.Ts, null.wav_p, null.nf)
    m._chk(m.lib.zv_synthesize_batch_envelope(*args, None, None, None, null.targets, int(fitted), None, None, None))
    for i, (w, n) in enumerate(null.results()):
        assert n == plains[i][1] and np.array_equal(LR.bits(w), LR.bits(plains[i][0])), i
    m.set_graph_mode(False)


def test_two_lanes_in_flight(env):
    m, g, _ = env
    hop = g.hop_size
    sets = [[(*_utt(g, 600 + 10 * k + i, 20 + 5 * i), 120 + 40 * k + 9 * i, None, None, 60 + 30 * k + 7 * i) for i in range(3)] for k in range(3)]
    m.set_graph_mode(False)
    plains = [[(w.copy(), n, d) for w, n, d in m.synthesize_batch(utts, return_durations=True)] for utts in sets]
    ctl = [_batch_controls(utts, hop, k) for k, utts in enumerate(sets)]
    batches = [m.prepare_batch(utts, volume=ctl[k][1], envelope=ctl[k][0]) for k, utts in enumerate(sets)]
    for graph in (False, True):
        m.set_graph_mode(graph)
        for k, bc in enumerate(batches):                 # _begin k, _end k - 1
            bc.begin(k % 2)
            if k:
                batches[k - 1].end((k - 1) % 2)
        batches[-1].end((len(batches) - 1) % 2)
        for k, bc in enumerate(batches):
            _same_as(bc, plains[k], ctl[k][0], ctl[k][1], hop, f"lanes, batch {k}, graph={graph}")
    m.set_graph_mode(False)


def test_batch_split_into_tail_groups(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    hop, T = g.hop_size, 900                                  # 16 utterances: 2 and 8 groups are different schedules (two utterances per group at least)
    tfs = [900, 500, 250, 37, 899, 1, 640, 333, 65, 700, 31, 32, 33, 450, 820, 128]
    utts = [(*_utt(g, 700 + i, 40 + 9 * i), T, None, None, tf) for i, tf in enumerate(tfs)]
    assert len(utts) * T * hop * 4 >= 16 << 20 and len(utts) // 2 >= 8
    envs, vols = _batch_controls(utts, hop, 2)
    m.set_graph_mode(False)
    with capi.switches(ZV_TAIL_GROUPS=1):
        plains = [(w.copy(), n, d) for w, n, d in m.synthesize_batch(utts, return_durations=True)]
        assert [n for _, n, _ in plains] == tfs
        bc = m.prepare_batch(utts, volume=vols, envelope=envs)
        bc.run()
        _same_as(bc, plains, envs, vols, hop, "one group")      # the rule, once; the grouped runs are held to these bits
        one = [(w.copy(), capi.Level.from_buffer_copy(lv)) for (w, _), lv in zip(bc.results(), bc.levels)]
    for groups in (2, 8):
        with capi.switches(ZV_TAIL_GROUPS=groups):
            for graph in (False, True):
                m.set_graph_mode(graph)
                bc = m.prepare_batch(utts, volume=vols, envelope=envs)
                for rep in range(2 if graph else 1):
                    m.poison(0x00 if rep else 0xFF)
                    bc.run()
                    for i, ((w, n), lv) in enumerate(zip(bc.results(), bc.levels)):
                        assert n == tfs[i] and np.array_equal(LR.bits(w), LR.bits(one[i][0])), (groups, graph, rep, i)
                        assert LR.level_bits(lv) == LR.level_bits(one[i][1]), (groups, graph, rep, i)
            m.set_graph_mode(False)


# ---- 6. validation, CLI -----------------------------------------------------------------------------------------------------

def test_bad_fields_are_refused_and_the_lane_stays_usable(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    hop = g.hop_size
    utts = [(*_utt(g, 62 + i, 20 + i), 100) for i in range(3)]
    good = [capi.Envelope(_gains(20, 7), 2, 100, 100), None, capi.Envelope(_gains(22, 8), 64, 0, 7)]
    bc = m.prepare_batch(utts, envelope=good)
    bc.run()
    want = [(w.copy(), n) for w, n in bc.results()]
    ids, puncts, style = (np.ascontiguousarray(x) for x in utts[0][:3])

    def refused(field, index):
        for call, name in ((bc.run, "zv_synthesize_batch_envelope"), (lambda: bc.begin(1), "zv_synthesize_batch_begin_envelope")):
            with pytest.raises(capi.ZvError) as ei:
                call()
            msg = str(ei.value)
            assert ei.value.status == ZV_ERR_ARG and name in msg and "utterance 2" in msg and field in msg, msg
            assert index is None or f"[{index}]" in msg, msg
        with pytest.raises(capi.ZvError):
            bc.end(1)                                    # nothing was left in flight

    def refused_alone(e, field, index):
        w, n = np.zeros(100 * hop, F), C.c_uint32(0)
        st = m.lib.zv_synthesize_envelope(m.h, capi._ptr(ids), capi._ptr(puncts), capi._ptr(style), len(ids), 100, capi._ptr(w), C.byref(n),
                                          None, None, None, 0, 0, None, None, C.byref(e))
        msg = m.lib.zv_last_error().decode()
        assert st == ZV_ERR_ARG and "zv_synthesize_envelope" in msg and "utterance 0" in msg and field in msg, msg
        assert index is None or f"[{index}]" in msg, msg

    for value in (float("nan"), float("inf"), -0.5, 16.5):           # past the binding's own check: the array the struct points into
        old = float(bc.ekeep[2].phoneme_gain[13])
        bc.ekeep[2].phoneme_gain[13] = value
        refused("phoneme_gain", 13)
        bc.ekeep[2].phoneme_gain[13] = old
        gains = np.ones(len(ids), F)
        gains[5] = value
        refused_alone(capi.EnvelopeC(gains.ctypes.data, 0, 0, 0), "phoneme_gain", 5)
    for field, value in (("ramp_frames", 65), ("fade_in_samples", 0x80000000), ("fade_out_samples", 0xffffffff)):
        old = getattr(bc.envelope[2], field)
        setattr(bc.envelope[2], field, value)
        refused(field, None)
        setattr(bc.envelope[2], field, old)
        e = capi.EnvelopeC()
        setattr(e, field, value)
        refused_alone(e, field, None)
    bc.run()                                             # lane 0 and lane 1 work as before
    for (w, n), (w0, n0) in zip(bc.results(), want):
        assert n == n0 and np.array_equal(LR.bits(w), LR.bits(w0))
    bc.begin(1)
    bc.end(1)
    for (w, n), (w0, n0) in zip(bc.results(), want):
        assert n == n0 and np.array_equal(LR.bits(w), LR.bits(w0))


def test_cli_round_trip(env, tmp_path):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    N, hop = 40, g.hop_size
    ids, puncts, style = _utt(g, 71, N)
    utt = tmp_path / "utt.txt"
    utt.write_text(" ".join(map(str, ids.tolist())) + "\n" + " ".join(map(str, puncts.tolist())) + "\n" +
                   " ".join(repr(float(x)) for x in style.tolist()) + "\n")
    db = [round(float(d), 2) for d in np.random.default_rng(9).uniform(-30.0, 12.0, N)]
    gains = tmp_path / "gains.txt"
    gains.write_text("".join(f"{d}\n" for d in db))
    out = tmp_path / "envelope.wav"
    cli = os.path.join(ROOT, "zerovox.cpp_amd", "zerovox")
    r = subprocess.run([cli, "-m", _M["path"], "-u", str(utt), "-o", str(out), "--fit", "--target-frames", "123", "--phoneme-gain-db", str(gains),
                        "--ramp-frames", "2", "--fade-in-ms", "20", "--fade-out-ms", "0.4761904761", "--peak-dbfs", "-3"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    e = capi.Envelope.from_db(phoneme_gain_db=db, ramp_frames=2, fade_in_ms=20, fade_out_ms=0.4761904761, rate=g.sampling_rate)
    assert e.fade_in_samples == int(np.floor(20 * g.sampling_rate / 1000 + 0.5)) > 0
    # 0.4761904761 ms at 22 050 Hz are 10.499999998 samples as a double and 10.50000003 once rounded to f32: the CLI must convert the double
    assert g.sampling_rate == 22050 and e.fade_out_samples == 10 and int(np.floor(float(F(0.4761904761)) * 22.05 + 0.5)) == 11
    w, nf = m.synthesize(ids, puncts, style, g.max_seq_len, fitted=True, target_frames=123, envelope=e, volume=capi.Volume.from_db(peak_dbfs=-3))
    assert nf == 123
    pcm = np.frombuffer(out.read_bytes()[44:], "<i2")
    want = np.clip(np.rint(w[:nf * hop] * F(32767.0)), -32768, 32767).astype(np.int16)
    assert np.array_equal(pcm, want) and pcm[0] == 0 and pcm[-1] == 0 and pcm.any()
