"""-m gpu: target durations (include/zerovox_amd.h "target durations") at the production geometry.

fit_durations_kernel sits between the duration predictor and the length regulator and hands the regulator forced frame counts, so
everything is checked against the existing forced-duration calls and against the rule restated in Python integers
(tests/fit_durations_rule.py) from the GPU's own raw logdur tap:
  * target 0 / None / a NULL array give the bits of the calls without a target (eager, graph capture and replay, both LayerNorm forms);
  * n_frames == target == sum of durations, durations == the rule, raw taps and buckets untouched, on both sides of the fused
    regulator's 1 024-token limit and of the kernel's own 1 024-wide passes;
  * the returned durations fed back as duration_frames give the same hidden, n_frames and wav, unfitted and fitted;
  * forced + free + per-phoneme scales, Fs > target, no free phoneme, num_phonemes < n, all weights 0;
  * batches (ragged, graph replay with new targets, poisoned lanes, tail groups, two lanes in flight) = stand-alone calls;
  * validation and the CLI flags."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from fit_durations_rule import fit, scaled_dur

pytestmark = pytest.mark.gpu

ZV_ERR_ARG = 5
_M = {}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROSODIES = [None, dict(duration_scale=1.3, pitch_scale=0.9, pitch_shift=0.05, energy_scale=1.1, energy_shift=-0.03)]
TAPS = ("logdur", "pitch", "energy", "pitch_bucket", "energy_bucket")


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


def _uscale(pr):
    from zerovox_cpp_amd import capi
    return None if pr is None else capi.Prosody(**pr).duration_scale


def mixed_controls(rng, n):
    """forced, per-phoneme-scaled and predicted durations side by side, local pitch / energy shifts (test_gpu_phoneme_controls.py's)"""
    frames = np.full(n, -1, np.int32)
    forced = rng.random(n) < 0.3
    frames[forced] = rng.integers(0, 9, forced.sum())
    scale = np.where(rng.random(n) < 0.5, rng.uniform(0.3, 3.0, n), 1.0).astype(np.float32)
    return dict(duration_frames=frames, duration_scale=scale, pitch_shift=rng.uniform(-0.2, 0.2, n).astype(np.float32),
                energy_shift=rng.uniform(-0.2, 0.2, n).astype(np.float32))


def _rule(e, num_phonemes, T, target, pr=None, pc=None):
    """the rule from the call's own raw logdur tap and its controls"""
    pc = pc or {}
    return fit(scaled_dur(e["logdur"], _uscale(pr), pc.get("duration_scale")), pc.get("duration_frames"), num_phonemes, T, target)


# ---- 1. identity ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ln_tail", [1, 0])
def test_target_zero_is_the_call_without_a_target(env, ln_tail):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    T = 700
    rng = np.random.default_rng(3)
    with capi.switches(ZV_LN_TAIL=ln_tail):
        for seed, N in ((11, 200), (12, 1100)):
            ids, puncts, style = _utt(g, seed, N)
            for pr, pc in ((None, None), (PROSODIES[1], mixed_controls(rng, N))):
                m.set_graph_mode(False)
                a = m.encode(ids, puncts, style, T, prosody=pr, phonemes=pc, return_durations=True)
                b = m.encode(ids, puncts, style, T, prosody=pr, phonemes=pc, return_durations=True, target_frames=0)
                for k in a:
                    assert np.array_equal(a[k], b[k]), (N, pr, k)
                ref = {f: m.synthesize(ids, puncts, style, T, prosody=pr, phonemes=pc, return_durations=True, fitted=f) for f in (False, True)}
                for graph in (False, True):
                    m.set_graph_mode(graph)
                    for _ in range(2 if graph else 1):       # capture, then replay
                        for f in (False, True):
                            w, n, d = m.synthesize(ids, puncts, style, T, prosody=pr, phonemes=pc, return_durations=True, fitted=f,
                                                   target_frames=0)
                            assert n == ref[f][1] and np.array_equal(w, ref[f][0]) and np.array_equal(d, ref[f][2]), (N, pr, graph, f)
                m.set_graph_mode(False)


def _ragged(g):
    nt = [(200, 1500), (7, 60), (300, 1200), (1, 11), (1100, 1437)]
    return [(*_utt(g, 300 + i, N), T) for i, (N, T) in enumerate(nt)]


@pytest.mark.parametrize("ln_tail", [1, 0])
def test_batch_without_targets_is_the_plain_batch(env, ln_tail):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    utts = _ragged(g)
    with capi.switches(ZV_LN_TAIL=ln_tail):
        for fitted in (False, True):
            m.set_graph_mode(False)
            ref = [(w.copy(), n) for w, n in m.synthesize_batch(utts, fitted=fitted)]
            for graph in (False, True):
                m.set_graph_mode(graph)
                zeros = m.prepare_batch([u + (None, None, 0) for u in utts], fitted=fitted)
                null = m.prepare_batch(utts, fitted=fitted)
                assert zeros.targets is not None and null.targets is None
                for _ in range(2 if graph else 1):
                    zeros.run()
                    # the _target entry point itself with a NULL array
                    args = (m.h, null.n, null.ids_p, null.pun_p, null.sty_p, null.Ns, null.Ts, null.wav_p, null.nf)
                    m._chk(m.lib.zv_synthesize_batch_target(*args, None, None, None, None, int(fitted)))
                    for i, (wr, nr) in enumerate(ref):
                        for what, bc in (("zeros", zeros), ("NULL", null)):
                            w, n = bc.results()[i]
                            assert n == nr and np.array_equal(w, wr), (what, fitted, graph, i)
            m.set_graph_mode(False)


# ---- 2. exact sums and the rule ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [1, 2, 7, 200, 1024, 1025, 1100, "max_phonemes"])
def test_exact_sums_and_the_rule(env, N):
    m, g, _ = env
    T = g.max_seq_len
    if N == "max_phonemes":
        N = T + 1                        # the sinusoid table's rows (synth.py), one more than the frame capacity
    ids, puncts, style = _utt(g, 40 + N, N)
    seen = 0
    for pr in PROSODIES:
        e0 = m.encode(ids, puncts, style, T, prosody=pr, return_durations=True)
        for target in sorted({1, N - 1, e0["n_frames"], T}):
            if not 0 < target <= T:
                continue                  # (N - 1 = 0 at N = 1, an utterance the predictor gives no frame: 0 means "no target")
            e = m.encode(ids, puncts, style, T, prosody=pr, return_durations=True, target_frames=target)
            what = (N, pr is not None, target)
            assert e["n_frames"] == target == int(e["durations"].sum()), (what, e["n_frames"], int(e["durations"].sum()))
            assert np.array_equal(e["durations"], _rule(e, N, T, target, pr)), what
            for k in TAPS + ("features",):
                assert np.array_equal(e[k], e0[k]), (what, k)
            seen += 1
    assert seen >= 4


# ---- 3. equivalence with forced durations, independent of any host exp ----------------------------------------------------------

@pytest.mark.parametrize("N,T,target", [(200, 900, 333), (1100, 1500, 1277), (1100, 1500, 1500), (7, 64, 12)])
def test_durations_fed_back_as_forced_frames_give_the_same_bits(env, N, T, target):
    m, g, _ = env
    hop = g.hop_size
    ids, puncts, style = _utt(g, 60 + N, N)
    pr = PROSODIES[1]
    e = m.encode(ids, puncts, style, T, prosody=pr, return_durations=True, target_frames=target)
    d = e["durations"]
    assert int(d.sum()) == target == e["n_frames"]
    forced = dict(duration_frames=d)
    ef = m.encode(ids, puncts, style, T, prosody=pr, phonemes=forced, return_durations=True)
    for k in e:
        assert np.array_equal(e[k], ef[k]), k
    w, nf, dw = m.synthesize(ids, puncts, style, T, prosody=pr, return_durations=True, target_frames=target)
    wf, nff, dwf = m.synthesize(ids, puncts, style, T, prosody=pr, phonemes=forced, return_durations=True)
    assert nf == nff == target and np.array_equal(dw, d) and np.array_equal(dwf, d)
    assert np.array_equal(w, wf), "unfitted wav"
    # fitted: the forced fitted call's bits; target * hop samples of audio — those of the unfitted forced call at T = target — then zeros
    v, nv, dv = m.synthesize(ids, puncts, style, T, prosody=pr, return_durations=True, target_frames=target, fitted=True)
    vf, nvf = m.synthesize(ids, puncts, style, T, prosody=pr, phonemes=forced, fitted=True)
    assert nv == nvf == target and np.array_equal(dv, d)
    assert np.array_equal(v, vf), "fitted wav"
    assert not np.isnan(v[target * hop:]).any() and not v[target * hop:].any(), "tail is not zero"
    short, ns = m.synthesize(ids, puncts, style, target, prosody=pr, phonemes=forced)
    assert ns == target and np.array_equal(v[:target * hop], short), "fitted audio = the unfitted forced call at T = target"


# ---- 4. mixed controls --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [200, 1100])
def test_mixed_controls(env, N):
    m, g, _ = env
    T = g.max_seq_len
    rng = np.random.default_rng(N)
    ids, puncts, style = _utt(g, 80 + N, N)
    e0 = m.encode(ids, puncts, style, T)
    # forced + free + per-phoneme scales, with and without an utterance scale
    for pr in PROSODIES:
        pc = mixed_controls(rng, N)
        Fs = int(pc["duration_frames"][pc["duration_frames"] >= 0].sum())
        assert Fs + 1 < T
        for target in sorted({Fs + 1, min(Fs + N, T - 1), T}):
            e = m.encode(ids, puncts, style, T, prosody=pr, phonemes=pc, return_durations=True, target_frames=target)
            want = _rule(e, N, T, target, pr, pc)
            assert np.array_equal(e["durations"], want), (pr is not None, target)
            assert e["n_frames"] == target == int(want.sum())
            held = pc["duration_frames"] >= 0
            assert np.array_equal(e["durations"][held], pc["duration_frames"][held])
            ep = m.encode(ids, puncts, style, T, prosody=pr, phonemes=pc)
            for k in TAPS:                            # pitch and energy decisions do not depend on durations
                assert np.array_equal(e[k], ep[k]), k
            assert np.array_equal(e["logdur"], e0["logdur"])
    # Fs > target: forced durations win, the free phonemes get 0
    pc = dict(duration_frames=np.where(np.arange(N) % 3 == 0, 6, -1).astype(np.int32))
    Fs = 6 * len(range(0, N, 3))
    e = m.encode(ids, puncts, style, T, phonemes=pc, return_durations=True, target_frames=Fs // 2)
    d = np.where(pc["duration_frames"] >= 0, 6, 0)
    want_t = np.diff(np.concatenate([[0], np.minimum(np.cumsum(d), T)]))
    assert e["n_frames"] == min(Fs, T) and np.array_equal(e["durations"], want_t)
    assert np.array_equal(_rule(e, N, T, Fs // 2, None, pc), d)
    # Fs == target: the same
    if Fs <= T:
        e = m.encode(ids, puncts, style, T, phonemes=pc, return_durations=True, target_frames=Fs)
        assert e["n_frames"] == Fs and np.array_equal(e["durations"], d)
    # no free phoneme: the forced durations, whatever the target
    pc = dict(duration_frames=rng.integers(0, T // N + 1, N).astype(np.int32))
    e = m.encode(ids, puncts, style, T, phonemes=pc, return_durations=True, target_frames=T)
    assert np.array_equal(e["durations"], pc["duration_frames"]) and e["n_frames"] == int(pc["duration_frames"].sum())
    # num_phonemes = n - 10: nothing lands past it, also where a duration is forced there
    k = N - 10
    pc = dict(duration_frames=np.full(N, -1, np.int32))
    pc["duration_frames"][[2, N - 3]] = 4
    for target in (k + 5, T):
        e = m.encode(ids, puncts, style, T, num_phonemes=k, phonemes=pc, return_durations=True, target_frames=target)
        assert np.array_equal(e["durations"], _rule(e, k, T, target, None, pc)), target
        assert e["n_frames"] == target and not e["durations"][k:].any() and e["durations"][2] == 4
    # every weight 0 (duration_scale = 1e-30 on the utterance): equal shares, the first three take the three frames left over
    e = m.encode(ids, puncts, style, T, prosody=dict(duration_scale=1e-30), return_durations=True, target_frames=N + 3)
    assert e["durations"].tolist() == [2, 2, 2] + [1] * (N - 3) and e["n_frames"] == N + 3


# ---- 5. batches -------------------------------------------------------------------------------------------------------------

def _alone(m, utts, prs, pcs, tgs, fitted=False):
    return [m.synthesize(*u, prosody=p, phonemes=c, return_durations=True, fitted=fitted, target_frames=t or None)
            for u, p, c, t in zip(utts, prs, pcs, tgs)]


def _same(bc, alone, what):
    for i, ((w, n), d, (wr, nr, dr)) in enumerate(zip(bc.results(), bc.durations, alone)):
        assert n == nr, (what, i, n, nr)
        assert np.array_equal(d, dr), (what, i, "durations")
        assert np.array_equal(w, wr), (what, i)


@pytest.mark.parametrize("fitted", [False, True])
def test_ragged_batch_graph_replay_with_new_targets_and_poisoned_lane(env, fitted):
    m, g, _ = env
    base = _ragged(g)
    rng = np.random.default_rng(17 + fitted)
    prs = [PROSODIES[i % 2] for i in range(len(base))]
    pcs = [mixed_controls(rng, len(u[0])) if i == 2 else None for i, u in enumerate(base)]
    tg1 = [900, 0, 1200, 11, 0]                  # targets on some utterances, none on the others
    tg2 = [0, 60, 777, 3, 1437]
    m.set_graph_mode(False)
    alone1, alone2 = _alone(m, base, prs, pcs, tg1, fitted), _alone(m, base, prs, pcs, tg2, fitted)
    for al, tg in ((alone1, tg1), (alone2, tg2)):
        for (w, n, d), t, u in zip(al, tg, base):
            assert not t or (n == t == int(d.sum())), (n, t)
    bc = m.prepare_batch([u + (p, c, t) for u, p, c, t in zip(base, prs, pcs, tg1)], durations=True, fitted=fitted)
    bc.run()
    _same(bc, alone1, "eager")
    m.set_graph_mode(True)
    bc.run()
    _same(bc, alone1, "graph capture")
    m.poison(0xFF)
    bc.run()
    _same(bc, alone1, "graph replay on a poisoned lane")
    for i, t in enumerate(tg2):
        bc.set_target_frames(i, t)
    m.poison(0x3C)
    bc.run()
    _same(bc, alone2, "graph replay with new targets")
    bc.begin(2)
    bc.end(2)
    _same(bc, alone2, "begin / end, graph")
    for i, t in enumerate(tg1):
        bc.set_target_frames(i, t)
    bc.run()
    _same(bc, alone1, "graph replay, back to the first targets")
    m.set_graph_mode(False)


def test_batch_split_into_tail_groups(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    utts = [(*_utt(g, 500 + i, N), T) for i, (N, T) in enumerate([(150 + 13 * i, 1500 - 7 * i) for i in range(10)])]
    assert sum(u[3] for u in utts) * g.hop_size * 4 >= 16 << 20 and capi.debug_get("ZV_TAIL_GROUPS") > 1
    tgs = [0 if i % 4 == 3 else 700 + 61 * i for i in range(10)]
    none = [None] * 10
    alone = _alone(m, utts, none, none, tgs)
    for graph in (False, True):
        m.set_graph_mode(graph)
        bc = m.prepare_batch([u + (None, None, t) for u, t in zip(utts, tgs)], durations=True)
        for rep in range(2 if graph else 1):
            m.poison(0x3C if rep else 0xFF)
            bc.run()
            _same(bc, alone, f"tail groups, graph={graph}, rep={rep}")
    m.set_graph_mode(False)


def test_two_lanes_in_flight_with_different_targets(env):
    m, g, _ = env
    batches, alones = [], []
    none = [None] * 3
    for k in range(4):
        utts = [(*_utt(g, 700 + 10 * k + i, 60 + 40 * i + 7 * k), 900) for i in range(3)]
        tgs = [300 + 100 * k + 7 * i for i in range(3)]
        alones.append(_alone(m, utts, none, none, tgs))
        batches.append(m.prepare_batch([u + (None, None, t) for u, t in zip(utts, tgs)], durations=True))
    for graph in (False, True):
        m.set_graph_mode(graph)
        for bc in batches:
            for d in bc.durations:
                d[:] = -7
        for k, bc in enumerate(batches):                 # _begin k, _end k - 1
            bc.begin(k % 2)
            if k:
                batches[k - 1].end((k - 1) % 2)
        batches[-1].end((len(batches) - 1) % 2)
        for k, bc in enumerate(batches):
            _same(bc, alones[k], f"lanes, batch {k}, graph={graph}")
            assert [n for _, n in bc.results()] == [300 + 100 * k + 7 * i for i in range(3)]
    m.set_graph_mode(False)


# ---- 6. validation and the CLI ------------------------------------------------------------------------------------------------

def test_target_above_the_capacity_is_refused_before_any_work(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    N, T = 40, 400
    ids, puncts, style = _utt(g, 61, N)
    wav, nf = np.zeros(T * g.hop_size, np.float32), C.c_uint32(0)
    st = m.lib.zv_synthesize_target(m.h, capi._ptr(ids), capi._ptr(puncts), capi._ptr(style), N, T, capi._ptr(wav), C.byref(nf), None, None,
                                    None, T + 1, 0)
    msg = m.lib.zv_last_error().decode()
    assert st == ZV_ERR_ARG and "zv_synthesize_target" in msg and "utterance 0" in msg and "target_frames" in msg, msg
    hid = np.zeros((T, m.E), np.float32)
    st = m.lib.zv_encode_taps_target(m.h, capi._ptr(ids), capi._ptr(puncts), capi._ptr(style), N, N, T, capi._ptr(hid), C.byref(nf), None,
                                     None, None, None, None, None, None, None, None, T + 1)
    msg = m.lib.zv_last_error().decode()
    assert st == ZV_ERR_ARG and "zv_encode_taps_target" in msg and "utterance 0" in msg and "target_frames" in msg, msg
    utts = [(*_utt(g, 62 + i, 20 + i), 300, None, None, 100) for i in range(3)]
    bc = m.prepare_batch(utts)
    bc.targets[2] = 301                                # past the binding's own check
    for call, name in ((bc.run, "zv_synthesize_batch_target"), (lambda: bc.begin(1), "zv_synthesize_batch_begin_target")):
        with pytest.raises(capi.ZvError) as ei:
            call()
        msg = str(ei.value)
        assert ei.value.status == ZV_ERR_ARG and name in msg and "utterance 2" in msg and "target_frames" in msg, msg
    with pytest.raises(capi.ZvError):
        bc.end(1)                                      # nothing was left in flight
    bc.targets[2] = 300
    bc.run()
    assert [n for _, n in bc.results()] == [100, 100, 300]


def _cli(args, code=0):
    cli = os.path.join(ROOT, "zerovox.cpp_amd", "zerovox")
    r = subprocess.run([cli, "-m", _M["path"]] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == code, (r.returncode, r.stderr)
    return r


def test_cli_target_flags(env, tmp_path):
    m, g, _ = env
    N, F = 40, 123
    hop = g.hop_size
    ids, puncts, style = _utt(g, 71, N)
    utt = tmp_path / "utt.txt"
    utt.write_text(" ".join(map(str, ids.tolist())) + "\n" + " ".join(map(str, puncts.tolist())) + "\n" +
                   " ".join(repr(float(x)) for x in style.tolist()) + "\n")
    out, tsv = tmp_path / "fit.wav", tmp_path / "align.tsv"
    _cli(["-u", str(utt), "-o", str(out), "--fit", "--target-frames", str(F), "--alignment", str(tsv)])
    assert os.path.getsize(out) == 44 + 2 * F * hop
    rows = [line.split("\t") for line in tsv.read_text().splitlines()]
    got = np.array([[int(v) for v in r] for r in rows[1:]], np.int64)
    assert len(got) == N and int(got[:, 3].sum()) == F
    w, nf, dur = m.synthesize(ids, puncts, style, g.max_seq_len, return_durations=True, fitted=True, target_frames=F)
    assert nf == F and np.array_equal(got[:, 3], dur)
    # seconds: floor(S * rate / hop + 0.5) frames; without --fit the file keeps the capacity, with --trim it is cut to the target
    S = 1.003
    Fs = int(np.floor(S * g.sampling_rate / hop + 0.5))
    out2 = tmp_path / "sec.wav"
    _cli(["-u", str(utt), "-o", str(out2), "--trim", "--target-seconds", repr(S), "--duration-scale", "1.2"])
    assert os.path.getsize(out2) == 44 + 2 * Fs * hop
    # a target above the checkpoint's capacity is a usage error
    r = _cli(["-u", str(utt), "-o", str(out2), "--target-frames", str(g.max_seq_len + 1)], code=2)
    assert "max_seq_len" in r.stderr
