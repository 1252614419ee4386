"""-m gpu: volume controls (include/zerovox_amd.h "volume controls") at the production geometry.

level_measure_kernel and level_apply_kernel run behind the vocoder's last step, so every expectation comes from the GPU's own
waveform of the same call WITHOUT volume, pushed through the rule restated in Python (tests/level_rule.py): the waveform must be
plain * float32(g) and the level the rule's, bit for bit.  These tests are also the check that gfx950's f64 conversion, product,
quotient and square root round as the host's do.
  * identity: no volume and no levels = the _target call; a meter-only call and the identity volume leave the waveform's bits alone
    (eager, graph capture and replay);
  * every speech length 0 .. 64 of a small utterance, fitted and unfitted, and lengths around one and two chunks of the kernels;
  * what the three fields mean, alone and together; the launches appear in the profile only with volume;
  * unfitted with run-shortened vocoding / decoding on and off;
  * batches (ragged, graph replay with new values, poisoned lanes, two lanes in flight, tail groups) = stand-alone calls;
  * validation and the CLI flags."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

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
    """a capi.Volume (or None: the identity) as the rule's tuple"""
    return LR.IDENTITY if v is None else (v.gain, v.target_rms, v.peak_ceiling)


def _check(what, w, level, plain, nf, hop, vol):
    """waveform and level of a volume call against the rule applied to the plain call's waveform"""
    r = LR.rule(plain, nf * hop, _vt(vol))
    assert np.array_equal(LR.bits(w), LR.bits(r["out"])), (what, "waveform", r["level"], level)
    assert LR.level_bits(level) == LR.level_bits(r["level"]) and level.reserved == 0, (what, "level", level, r["level"], r["S"])
    return r


def _volumes_for(plain, nf, hop):
    """volumes that mean something at this utterance's own level: (name, Volume) pairs"""
    from zerovox_cpp_amd import capi
    S, pk = LR.measure(plain[:nf * hop])
    rms = float(LR.rms_of(S, nf * hop))
    peak = float(np.array([pk], np.uint32).view(F)[0])
    if not (rms > 0 and peak > 0):                           # nothing to relate to (no speech): any volume does
        rms, peak = 0.1, 0.5
    up = min(1.0, rms * 1.7)
    return [("target alone", capi.Volume(1.0, up, 0.0)), ("gain alone", capi.Volume(0.37, 0.0, 0.0)),
            ("ceiling binds", capi.Volume(1.0, 0.0, min(1.0, peak * 0.5))), ("ceiling does not bind", capi.Volume(1.0, 0.0, min(1.0, peak * 1.01))),
            ("target and gain", capi.Volume(0.5, up, 0.0)), ("all three", capi.Volume(2.0, rms * 0.9, min(1.0, peak * 0.8))),
            ("all three, ceiling free", capi.Volume(0.5, rms * 0.5, 1.0))]


# ---- 1. identity ------------------------------------------------------------------------------------------------------------

def test_no_volume_is_the_target_call_and_meters_leave_the_bits_alone(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    N, T, hop = 40, 200, g.hop_size
    ids, puncts, style = _utt(g, 11, N)
    for fitted in (False, True):
        for tf in (0, 120):
            m.set_graph_mode(False)
            ref, nf = m.synthesize(ids, puncts, style, T, fitted=fitted, target_frames=tf)
            ref = ref.copy()
            for graph in (False, True):
                m.set_graph_mode(graph)
                for _ in range(2 if graph else 1):       # capture, then replay
                    # the _volume entry point itself with both NULL
                    a, b, c = (np.ascontiguousarray(x) for x in (ids, puncts, style))
                    w, n = np.full(T * hop, 7.0, F), C.c_uint32(0)
                    m._chk(m.lib.zv_synthesize_volume(m.h, capi._ptr(a), capi._ptr(b), capi._ptr(c), N, T, capi._ptr(w), C.byref(n), None, None,
                                                      None, tf, int(fitted), None, None))
                    assert n.value == nf and np.array_equal(LR.bits(w), LR.bits(ref)), (fitted, tf, graph)
                    for what, vol in (("meter only", None), ("identity volume", capi.Volume())):
                        w, n, lv = m.synthesize(ids, puncts, style, T, fitted=fitted, target_frames=tf, volume=vol, return_levels=True)
                        assert n == nf and np.array_equal(LR.bits(w), LR.bits(ref)) and lv.gain == 1.0, (what, fitted, tf, graph)
                        _check((what, fitted, tf, graph), w, lv, ref, nf, hop, vol)
                    # and the plain call still gives its bits next to graphs captured with volume
                    w, n = m.synthesize(ids, puncts, style, T, fitted=fitted, target_frames=tf)
                    assert n == nf and np.array_equal(LR.bits(w), LR.bits(ref)), (fitted, tf, graph)
    m.set_graph_mode(False)


# ---- 2. every length --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fitted", [False, True])
def test_every_speech_length_of_a_small_utterance(env, fitted):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    N, T, hop = 16, 64, g.hop_size
    ids, puncts, style = _utt(g, 21, N)
    vol = capi.Volume(1.3, 0.05, 0.4)
    gains = set()
    for nf in range(0, T + 1):
        kw = dict(phonemes=dict(duration_frames=np.zeros(N, np.int32))) if nf == 0 else dict(target_frames=nf)
        plain, n0 = m.synthesize(ids, puncts, style, T, fitted=fitted, **kw)
        plain = plain.copy()
        w, n, lv = m.synthesize(ids, puncts, style, T, fitted=fitted, volume=vol, return_levels=True, **kw)
        assert n0 == nf == n
        r = _check((fitted, nf), w, lv, plain, nf, hop, vol)
        gains.add(float(r["level"][2]))
        if fitted:
            assert not w[nf * hop:].any()                      # fitted zeros stay zero
        elif nf < T:
            assert w[nf * hop:].any() and lv.gain != 1.0       # an unfitted tail is scaled like the speech
    assert len(gains) > 32, gains                              # the lengths were told apart


@pytest.mark.parametrize("fitted", [False, True])
def test_lengths_around_one_and_two_chunks(env, fitted):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    hop, chunk = g.hop_size, LR.chunk_samples(ROOT)
    nfs = sorted({max(1, (k * chunk) // hop + d) for k in (1, 2) for d in (-1, 0, 1)} | {-(-k * chunk // hop) for k in (1, 2)})
    N, T = 50, max(nfs) + 37
    assert T * hop > 2 * chunk + hop and any(nf * hop % chunk == 0 for nf in nfs) == (chunk % hop == 0)
    ids, puncts, style = _utt(g, 22, N)
    vol = capi.Volume(0.9, 0.07, 0.6)
    for nf in nfs:
        plain, n0 = m.synthesize(ids, puncts, style, T, fitted=fitted, target_frames=nf)
        plain = plain.copy()
        w, n, lv = m.synthesize(ids, puncts, style, T, fitted=fitted, target_frames=nf, volume=vol, return_levels=True)
        assert n0 == nf == n
        _check((fitted, nf), w, lv, plain, nf, hop, vol)


# ---- 3. what the fields mean ------------------------------------------------------------------------------------------------

def test_target_gain_and_ceiling(env):
    m, g, _ = env
    N, T, hop = 60, 300, g.hop_size
    ids, puncts, style = _utt(g, 31, N)
    for fitted in (False, True):
        plain, nf = m.synthesize(ids, puncts, style, T, fitted=fitted, target_frames=211)
        plain = plain.copy()
        n = nf * hop
        for name, vol in _volumes_for(plain, nf, hop):
            w, n1, lv = m.synthesize(ids, puncts, style, T, fitted=fitted, target_frames=211, volume=vol, return_levels=True)
            assert n1 == nf
            r = _check((name, fitted), w, lv, plain, nf, hop, vol)
            rms_out = float(np.sqrt(np.mean(w[:n].astype(np.float64) ** 2)))
            if name == "gain alone":
                assert lv.gain == vol.gain
            if name in ("target alone", "target and gain"):
                want = vol.target_rms * vol.gain
                if float(r["rms"]) >= 0.01:              # the bound tests/test_level_cpu.py derives, where it was derived
                    assert abs(rms_out - want) <= want * (2.0 ** -20 / float(r["rms"]) + 2.0 ** -22), (name, rms_out, want)
            if name in ("ceiling binds", "all three"):
                assert lv.gain < (vol.gain if name == "ceiling binds" else 2.0 * vol.target_rms / lv.rms)
                top = int((LR.bits(w[:n]) & np.uint32(0x7fffffff)).max())
                assert top <= int(LR.bits(F(vol.peak_ceiling))[0]), (name, top)          # at or under the ceiling, by bits
                assert top >= int(LR.bits(F(vol.peak_ceiling * 0.999))[0]), (name, top)  # and it reaches it
            if name == "ceiling does not bind":
                assert lv.gain == 1.0


def test_the_two_launches_appear_only_with_volume(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    ids, puncts, style = _utt(g, 32, 30)
    hop, T = g.hop_size, 150
    m.profile_begin()
    m.synthesize(ids, puncts, style, T, target_frames=100)
    plain = {s["name"]: s for s in m.profile_end()}
    m.profile_begin()
    m.synthesize(ids, puncts, style, T, target_frames=100, volume=capi.Volume(1.0, 0.1, 0.5))
    vol = {s["name"]: s for s in m.profile_end()}
    assert "voc_level_measure" not in plain and "voc_level_apply" not in plain
    assert set(vol) == set(plain) | {"voc_level_measure", "voc_level_apply"}
    for k in plain:
        assert vol[k]["launches"] == plain[k]["launches"], k
    assert vol["voc_level_measure"]["launches"] == 1 and vol["voc_level_apply"]["launches"] == 1
    assert vol["voc_level_measure"]["algo_bytes"] == 4.0 * 100 * hop and vol["voc_level_apply"]["algo_bytes"] == 8.0 * T * hop


# ---- 4. unfitted forms ------------------------------------------------------------------------------------------------------

def test_unfitted_with_run_shortening_on_and_off(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    N, T, nf, hop = 30, 600, 100, g.hop_size
    ids, puncts, style = _utt(g, 41, N)
    vol = capi.Volume(1.5, 0.06, 0.5)
    plain, n0 = m.synthesize(ids, puncts, style, T, target_frames=nf)
    plain = plain.copy()
    assert n0 == nf and plain[nf * hop:].any()
    for voc_runs in (2, 0):                                    # 2: at any size (1, the default, takes batches only)
        for dec_runs in (2, 0):
            with capi.switches(ZV_VOC_RUNS=voc_runs, ZV_DEC_RUNS=dec_runs):
                for graph in (False, True):
                    m.set_graph_mode(graph)
                    w, n, lv = m.synthesize(ids, puncts, style, T, target_frames=nf, volume=vol, return_levels=True)
                    assert n == nf
                    _check((voc_runs, dec_runs, graph), w, lv, plain, nf, hop, vol)
                    tab = m.voc_runs()
                    assert (tab.shape[0] == 1 and tab[0, 3] > 0) if voc_runs else tab.shape[0] == 0      # the run was taken, or not
                m.set_graph_mode(False)


# ---- 5. batches = stand-alone calls -----------------------------------------------------------------------------------------

def _ragged(g):
    nt = [(40, 300, 201), (7, 60, 0), (60, 257, 257), (1, 11, 5), (100, 310, 97)]
    return [(*_utt(g, 500 + i, N), T, None, None, tf) for i, (N, T, tf) in enumerate(nt)]


def _batch_volumes(m, utts, fitted, hop, salt):
    """per-utterance volumes chosen at each utterance's own level, some None"""
    plains = [(w.copy(), n) for w, n in m.synthesize_batch(utts, fitted=fitted)]
    vols = []
    for i, (w, n) in enumerate(plains):
        cands = _volumes_for(w, n, hop)
        vols.append(None if (i + salt) % 3 == 1 else cands[(2 * i + salt) % len(cands)][1])
    return plains, vols


def _same_as(bc, plains, vols, hop, what):
    for i, ((w, n), lv) in enumerate(zip(bc.results(), bc.levels)):
        assert n == plains[i][1], (what, i)
        _check((what, i), w, lv, plains[i][0], n, hop, vols[i])


@pytest.mark.parametrize("fitted", [False, True])
def test_ragged_batch_replay_and_poison(env, fitted):
    m, g, _ = env
    hop = g.hop_size
    utts = _ragged(g)
    m.set_graph_mode(False)
    plains, vols1 = _batch_volumes(m, utts, fitted, hop, 0)
    _, vols2 = _batch_volumes(m, utts, fitted, hop, 1)
    # the plain batch is the stand-alone calls (test_gpu_fit_durations.py); here: the volume batch = the stand-alone volume calls
    for i, u in enumerate(utts):
        w, n, lv = m.synthesize(*u[:4], fitted=fitted, target_frames=u[6], volume=vols1[i], return_levels=True)
        assert n == plains[i][1]
        _check(("alone", i), w, lv, plains[i][0], n, hop, vols1[i])
    bc = m.prepare_batch(utts, fitted=fitted, volume=vols1)
    bc.run()
    _same_as(bc, plains, vols1, hop, "eager")
    m.set_graph_mode(True)
    bc.run()
    _same_as(bc, plains, vols1, hop, "graph capture")
    m.poison(0xFF)
    bc.run()
    _same_as(bc, plains, vols1, hop, "graph replay on a lane poisoned with 0xFF")
    for i, v in enumerate(vols2):
        bc.set_volume(i, v)
    m.poison(0x00)
    bc.run()
    _same_as(bc, plains, vols2, hop, "graph replay with new values on a lane poisoned with 0x00")
    bc.begin(2)
    bc.end(2)
    _same_as(bc, plains, vols2, hop, "begin / end, graph")
    # a meter-only batch and the plain batch next to it
    meter = m.prepare_batch(utts, fitted=fitted, return_levels=True)
    meter.run()
    _same_as(meter, plains, [None] * len(utts), hop, "meter only")
    for i, (w, n) in enumerate(m.synthesize_batch(utts, fitted=fitted)):
        assert n == plains[i][1] and np.array_equal(LR.bits(w), LR.bits(plains[i][0])), i
    # the _volume entry point with both NULL is the _target call
    null = m.prepare_batch(utts, fitted=fitted)
    args = (m.h, null.n, null.ids_p, null.pun_p, null.sty_p, null.Ns, null.Ts, null.wav_p, null.nf)
    m._chk(m.lib.zv_synthesize_batch_volume(*args, None, None, None, null.targets, int(fitted), None, None))
    for i, (w, n) in enumerate(null.results()):
        assert n == plains[i][1] and np.array_equal(LR.bits(w), LR.bits(plains[i][0])), i
    m.set_graph_mode(False)


def test_two_lanes_in_flight(env):
    m, g, _ = env
    hop = g.hop_size
    sets = [[(*_utt(g, 600 + 10 * k + i, 20 + 5 * i), 120 + 40 * k + 9 * i, None, None, 60 + 30 * k + 7 * i) for i in range(3)] for k in range(3)]
    m.set_graph_mode(False)
    prep = [_batch_volumes(m, utts, False, hop, k) for k, utts in enumerate(sets)]
    batches = [m.prepare_batch(utts, volume=prep[k][1]) for k, utts in enumerate(sets)]
    for graph in (False, True):
        m.set_graph_mode(graph)
        for bc in batches:
            for lv in bc.levels:
                lv.rms = lv.peak = lv.gain = -7.0
        for k, bc in enumerate(batches):                 # _begin k, _end k - 1
            bc.begin(k % 2)
            if k:
                batches[k - 1].end((k - 1) % 2)
        batches[-1].end((len(batches) - 1) % 2)
        for k, bc in enumerate(batches):
            _same_as(bc, prep[k][0], prep[k][1], hop, f"lanes, batch {k}, graph={graph}")
    m.set_graph_mode(False)


def test_batch_split_into_tail_groups(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    hop, T = g.hop_size, 900                                  # 16 utterances: 2 and 8 groups are different schedules (two utterances per group at least)
    tfs = [900, 500, 250, 37, 899, 1, 640, 333, 65, 700, 31, 32, 33, 450, 820, 128]
    utts = [(*_utt(g, 700 + i, 40 + 9 * i), T, None, None, tf) for i, tf in enumerate(tfs)]
    assert len(utts) * T * hop * 4 >= 16 << 20 and len(utts) // 2 >= 8
    m.set_graph_mode(False)
    with capi.switches(ZV_TAIL_GROUPS=1):
        plains = [(w.copy(), n) for w, n in m.synthesize_batch(utts)]
        assert [n for _, n in plains] == tfs
        vols = [capi.Volume(1.0, 0.05, 0.5), None, capi.Volume(0.5, 0.0, 0.0), capi.Volume(3.0, 0.1, 0.3)] * 4
        bc = m.prepare_batch(utts, volume=vols)
        bc.run()
        _same_as(bc, plains, vols, hop, "one group")            # the rule, once; the grouped runs are held to these bits
        one = [(w.copy(), capi.Level.from_buffer_copy(lv)) for (w, _), lv in zip(bc.results(), bc.levels)]
    for groups in (2, 8):
        with capi.switches(ZV_TAIL_GROUPS=groups):
            for graph in (False, True):
                m.set_graph_mode(graph)
                bc = m.prepare_batch(utts, volume=vols)
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
    good = [capi.Volume(1.0, 0.1, 0.5), None, capi.Volume(2.0, 0.0, 0.9)]
    bc = m.prepare_batch(utts, volume=good)
    bc.run()
    want = [(w.copy(), n, capi.Level.from_buffer_copy(lv)) for (w, n), lv in zip(bc.results(), bc.levels)]
    bad = [("gain", float("nan")), ("gain", float("inf")), ("gain", -1.0), ("gain", 1000.5), ("target_rms", float("nan")),
           ("target_rms", -0.25), ("target_rms", 1.5), ("peak_ceiling", float("-inf")), ("peak_ceiling", -0.5), ("peak_ceiling", 1.25)]
    for field, value in bad:
        old = getattr(bc.volume[2], field)
        setattr(bc.volume[2], field, value)              # past the binding's own check
        for call, name in ((bc.run, "zv_synthesize_batch_volume"), (lambda: bc.begin(1), "zv_synthesize_batch_begin_volume")):
            with pytest.raises(capi.ZvError) as ei:
                call()
            msg = str(ei.value)
            assert ei.value.status == ZV_ERR_ARG and name in msg and "utterance 2" in msg and field in msg, msg
        with pytest.raises(capi.ZvError):
            bc.end(1)                                    # nothing was left in flight
        v = capi.Volume()
        setattr(v, field, value)
        ids, puncts, style = (np.ascontiguousarray(x) for x in utts[0][:3])
        w, n, lv = np.zeros(100 * hop, F), C.c_uint32(0), capi.Level()
        st = m.lib.zv_synthesize_volume(m.h, capi._ptr(ids), capi._ptr(puncts), capi._ptr(style), len(ids), 100, capi._ptr(w), C.byref(n),
                                        None, None, None, 0, 0, C.byref(v), C.byref(lv))
        msg = m.lib.zv_last_error().decode()
        assert st == ZV_ERR_ARG and "zv_synthesize_volume" in msg and "utterance 0" in msg and field in msg, msg
        setattr(bc.volume[2], field, old)
    bc.run()                                             # lane 0 and lane 1 work as before
    bc.begin(1)
    bc.end(1)
    for (w, n), lv, (w0, n0, lv0) in zip(bc.results(), bc.levels, want):
        assert n == n0 and np.array_equal(LR.bits(w), LR.bits(w0)) and LR.level_bits(lv) == LR.level_bits(lv0)


def test_cli_volume_flags(env, tmp_path):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    N, hop = 40, g.hop_size
    ids, puncts, style = _utt(g, 71, N)
    utt = tmp_path / "utt.txt"
    utt.write_text(" ".join(map(str, ids.tolist())) + "\n" + " ".join(map(str, puncts.tolist())) + "\n" +
                   " ".join(repr(float(x)) for x in style.tolist()) + "\n")
    out = tmp_path / "level.wav"
    cli = os.path.join(ROOT, "zerovox.cpp_amd", "zerovox")
    r = subprocess.run([cli, "-m", _M["path"], "-u", str(utt), "-o", str(out), "--fit", "--target-frames", "123", "--loudness-dbfs", "-20",
                        "--peak-dbfs", "-1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    vol = capi.Volume.from_db(target_dbfs=-20, peak_dbfs=-1)
    w, nf, lv = m.synthesize(ids, puncts, style, g.max_seq_len, fitted=True, target_frames=123, volume=vol, return_levels=True)
    assert nf == 123
    pcm = np.frombuffer(out.read_bytes()[44:], "<i2")
    want = np.clip(np.rint(w[:nf * hop] * F(32767.0)), -32768, 32767).astype(np.int16)
    assert np.array_equal(pcm, want)
    assert np.abs(pcm.astype(np.int32)).max() == int(np.rint(np.abs(w[:nf * hop]).max() * F(32767.0))) <= int(np.rint(vol.peak_ceiling * F(32767.0)))
    got = re.search(r"level: rms (\S+) peak (\S+) gain (\S+)", r.stdout)
    assert got and [F(float(v)) for v in got.groups()] == [F(lv.rms), F(lv.peak), F(lv.gain)], r.stdout
