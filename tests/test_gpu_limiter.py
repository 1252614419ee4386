"""-m gpu: the look-ahead peak limiter (include/zerovox_amd.h "limiter") on the tiny synthetic checkpoint (22 050 Hz, hop 300; the kernels
depend on the rate, the hop, the lengths and the asks alone).

Every expectation is the rule restated in numpy (tests/limiter_rule.py) on the interpolator the library itself returns
(capi.loudness_design: the design is data to the kernels).  There is no tolerance anywhere: every field of the result and every sample
has the rule's bits.  Every case first asserts, FROM THE RESTATEMENT's intermediates, that it reaches the branch it is there for
(tests/limiter_shapes.py, which tests/test_limiter_cpu.py runs without a device too), and holds s_n <= q_n and the promise — every
finite |out_n|, n < N, at most the ceiling — on the device's output as well.
  * the single call on every shape of limiter_shapes.CASES: W = 3 and W = 8 192, N < W, N < attack, n_frames = 0, n_frames < T, peaks in
    sample 0 and N - 1, peaks closer than W and exactly W apart, peaks on either side of a tile's end in each pass's own index over
    spans of one tile and of three, a full-scale square wave, silence, a NaN and infinities, gain 0, the identity;
  * a ragged batch of five under mixed asks against the single calls; the same batch after zv_debug_poison of lane 0 with both bytes;
  * one batch in two launch groups;
  * a call beside a batch in flight, and after a much longer and a much shorter call;
  * true_peak_before against Model.loudness_wave, bit for bit; Model.deliver on a synthesised waveform; the two command-line forms;
  * arguments refused by name."""
import os
import re
import subprocess
import types
import wave

import numpy as np
import pytest

import limiter_rule as LM
import limiter_shapes as LH
import loudness_rule as LR
import loudness_shapes as LS

pytestmark = pytest.mark.gpu

_M = {}
F = np.float32
SR, HOP = LH.SR, LH.HOP


@pytest.fixture
def tiny(ckpt):
    from zerovox_cpp_amd import capi
    if "e" not in _M:
        path, g, _ = ckpt("tiny")
        _M["e"] = types.SimpleNamespace(m=capi.Model(path, 0), g=g, path=path, D=capi.loudness_design(g.sampling_rate))
    e = _M["e"]
    assert e.g.sampling_rate == SR and e.g.hop_size == HOP and capi.limit_design(SR) == (LH.ATTACK, LH.RELEASE)
    e.m.set_graph_mode(False)
    return e


def teardown_module(module):
    if "e" in _M:
        _M["e"].m.close()
    _M.clear()


def _limiter(q):
    """the rule's ask (or None) as a capi.Limiter"""
    from zerovox_cpp_amd import capi
    return None if q is None else capi.Limiter(float(q.gain), float(q.ceiling), q.attack, q.release)


def _same(what, got, want):
    (res, out), (wres, wout) = got, want
    assert LM.key(res) == LM.key(wres), (what, res, wres)
    assert out.shape == wout.shape and out.dtype == F, what
    bad = np.flatnonzero(out.view(np.uint32) != wout.view(np.uint32))
    assert bad.size == 0, (what, bad.size, bad[:6], out[bad[0]], wout[bad[0]])


def _promise(what, out, N, ceiling):
    head = out[:N]
    fin = np.isfinite(head)
    assert (np.abs(head[fin]) <= F(ceiling)).all(), what


# ---- 1. the single call on every shape ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(LH.CASES))
def test_single_call_has_the_rules_bits(tiny, name):
    m, D = tiny.m, tiny.D
    c = LH.CASES[name]()
    res, out, I = LH.check(D, c)
    got = m.limit_wave(c.x, _limiter(c.ask), n_frames=c.nf)
    _same(name, got, (res, out))
    _promise(name, got[1], c.N, I.ask.ceiling)
    loud = m.loudness_wave(c.x, None, n_frames=c.nf, apply=False)[0]          # the same span through the true-peak meter
    assert LR.dbits(loud.true_peak) == LR.dbits(got[0].true_peak_before) and LR.fbits(loud.sample_peak) == LR.fbits(got[0].sample_peak_before)
    after = m.loudness_wave(got[1], None, n_frames=c.nf, apply=False)[0]
    assert LR.dbits(after.true_peak) == LR.dbits(got[0].true_peak_after) and LR.fbits(after.sample_peak) == LR.fbits(got[0].sample_peak_after)


def test_n_frames_beyond_T_counts_as_T(tiny):
    m, D = tiny.m, tiny.D
    c = LH.CASES["w3"]()
    _same("beyond", m.limit_wave(c.x, _limiter(c.ask), n_frames=c.x.size // HOP + 9), LM.rule(D, c.x, c.x.size, c.ask, SR)[:2])


# ---- 2. a ragged batch ------------------------------------------------------------------------------------------------------------------------

def test_ragged_batch_equals_single_calls_and_the_rule(tiny):
    m, D = tiny.m, tiny.D
    xs, nfs, asks = LH.ragged_batch()
    want = [LM.rule(D, x, nf * HOP, q, SR)[:2] for x, nf, q in zip(xs, nfs, asks)]
    assert all(w[0].limited_samples > 0 for u, w in enumerate(want) if u != 1) and want[1][0].limited_samples == 0
    single = [m.limit_wave(x, _limiter(q), n_frames=nf) for x, nf, q in zip(xs, nfs, asks)]
    for u in range(5):
        _same(("single", u), single[u], want[u])
    batch = m.limit_wave_batch(xs, [_limiter(q) for q in asks], nfs)
    for u in range(5):
        _same(("batch", u), batch[u], single[u])
        _promise(("batch", u), batch[u][1], nfs[u] * HOP, asks[u].ceiling)
    # asks == NULL and n_frames == NULL: the identity over the whole capacity
    plain = m.limit_wave_batch(xs, None, None)
    for u in range(5):
        _same(("plain", u), plain[u], LM.rule(D, xs[u], xs[u].size, None, SR)[:2])


def test_poisoned_lane_leaves_the_bits_unchanged(tiny):
    m = tiny.m
    xs, nfs, asks = LH.ragged_batch()
    qs = [_limiter(q) for q in asks]
    first = m.limit_wave_batch(xs, qs, nfs)
    for byte in (0x00, 0xFF):
        m.poison(byte, 0)
        for u, got in enumerate(m.limit_wave_batch(xs, qs, nfs)):
            _same(("poison", byte, u), got, first[u])
        m.poison(byte, 0)
        _same(("poison, single", byte), m.limit_wave(xs[3], qs[3], n_frames=nfs[3]), first[3])


# ---- 3. one batch, two launch groups ---------------------------------------------------------------------------------------------------------

def test_a_batch_across_a_launch_groups_end(tiny):
    """Capacities that cross 2^26 padded samples: utterances 0 .. 5 are one launch group, 6 .. 9 the next, whose segment offsets start
    at 0 again in an I/O block that is reused.  A kernel that ignores x0, q0, m0, tile0 or stat0 fails the utterances behind the head
    of their group."""
    m, D = tiny.m, tiny.D
    Ts = [32768] * 7 + [50, 50, 1]
    assert m.max_frames() >= max(Ts) and LS.group_ends(Ts, HOP) == [6, 10]
    nfs = [400, 40, 0, 7, 300, 1, 0, 50, 45, 1]
    block = LS.speech(SR, 600, 1 << 20, 0.3)
    xs = [np.resize(np.roll(block, 4099 * u), T * HOP) * F(0.5 + 0.1 * u) for u, T in enumerate(Ts)]
    a = [LM.ask(2.0, 0.1, LH.ATTACK, LH.RELEASE), LM.ask(3.0, 0.05, 1, 1), LM.ask(1.5, 0.1, 2047, 6144), LM.ask(4.0, 0.2, 100, 900)]
    asks = [a[0], a[1], a[2], a[3], a[2], a[0], a[1], a[0], a[3], a[1]]
    want = [LM.rule(D, x, nf * HOP, q, SR)[:2] for x, nf, q in zip(xs, nfs, asks)]
    assert all(want[u][0].limited_samples > 0 for u in (0, 1, 3, 4, 7, 8))
    batch = m.limit_wave_batch(xs, [_limiter(q) for q in asks], nfs)
    for u in range(len(Ts)):
        _same(("batch", u), batch[u], want[u])


# ---- 4. history -------------------------------------------------------------------------------------------------------------------------------

def _utterances(g):
    from zerovox_cpp_amd import synth
    return [(*synth.encoder_inputs(g, 8300 + i, N), T) for i, (N, T) in enumerate(((6, 40), (3, 17), (9, 64)))]


def test_calls_around_it_leave_the_bits_unchanged(tiny):
    m, D, g = tiny.m, tiny.D, tiny.g
    xs, nfs, asks = LH.ragged_batch()
    qs = [_limiter(q) for q in asks]
    want = [LM.rule(D, x, nf * HOP, q, SR)[:2] for x, nf, q in zip(xs, nfs, asks)]

    def check(what):
        for u, got in enumerate(m.limit_wave_batch(xs, qs, nfs)):
            _same((what, "batch", u), got, want[u])
        _same((what, "single"), m.limit_wave(xs[3], qs[3], n_frames=nfs[3]), want[3])

    check("quiescent")
    utts = _utterances(g)
    plain = m.synthesize_batch(utts)
    for graph in (False, True, True):                                          # eager, graph capture, graph replay
        m.set_graph_mode(graph)
        bc = m.prepare_batch(utts)
        bc.begin(1)
        check(("beside a batch in flight on lane 1", graph))
        bc.end(1)
        for (w0, n0), (w1, n1) in zip(plain, bc.results()):                     # and the batch beside it is what it is alone
            assert n0 == n1 and np.array_equal(w0.view(np.uint32), w1.view(np.uint32)), graph
        check(("after the batch", graph))
    m.set_graph_mode(False)
    long = LS.speech(SR, 710, 3000 * HOP, 0.4)                                  # the I/O block grows ...
    first = m.limit_wave(long, qs[0], n_frames=2990)
    check("after a much longer call")
    m.limit_wave(xs[0][:HOP], None)                                             # ... and is reused by a call of one frame
    check("after a much shorter call")
    _same("the long call again", m.limit_wave(long, qs[0], n_frames=2990), first)


# ---- 5. the delivery chain ----------------------------------------------------------------------------------------------------------------------

def test_deliver_meets_target_and_ceiling_on_a_synthesised_waveform(tiny):
    from zerovox_cpp_amd import capi, synth
    m, D, g = tiny.m, tiny.D, tiny.g
    ids, puncts, style = synth.encoder_inputs(g, 9, 12)
    wav, nf = m.synthesize(ids, puncts, style, 64)[:2]
    ceiling = F(10.0 ** (-1.0 / 20.0))
    before, lim, after, out = m.deliver(wav, -16.0, -1.0, n_frames=nf)
    print("deliver:", before, lim, after)
    assert before.blocks_gated > 0
    want = LM.rule(D, wav, nf * HOP, LM.ask(before.gain, ceiling, LH.ATTACK, LH.RELEASE), SR)
    _same("deliver", (lim, out), want[:2])
    _promise("deliver", out, nf * HOP, ceiling)
    assert LR.key(after) == LR.key(LR.rule(D, out, nf * HOP, out=False)[0])
    assert LR.dbits(after.true_peak) == LR.dbits(lim.true_peak_after)
    if lim.limited_samples == 0:                                                # nothing to limit: the target is met as by the gain alone
        assert abs(float(after.integrated_lufs) + 16.0) <= 0.01, (before, after)
    else:
        assert float(after.integrated_lufs) <= -16.0 + 0.01 and after.sample_peak <= ceiling


# ---- 6. the command line ------------------------------------------------------------------------------------------------------------------------

def _pcm(path):
    with wave.open(path, "rb") as w:
        assert w.getnchannels() == 1 and w.getframerate() == SR
        return np.frombuffer(w.readframes(w.getnframes()), "<i2").astype(F) / F(32768.0)


def test_command_line_limits_a_file_and_a_synthesis_run(tiny, tmp_path):
    from zerovox_cpp_amd import capi, synth
    m, D, g = tiny.m, tiny.D, tiny.g
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zerovox.cpp_amd", "zerovox")
    ids, puncts, _ = synth.encoder_inputs(g, 9, 12)
    out, utt, lim = str(tmp_path / "out.wav"), str(tmp_path / "utt.txt"), str(tmp_path / "lim.wav")
    open(utt, "w").write(" ".join(map(str, ids)) + "\n" + " ".join(map(str, puncts)) + "\n0\n")
    # a synthesis run: --limit with --lufs and --true-peak-dbtp
    r = subprocess.run([cli, "-m", tiny.path, "-u", utt, "-o", out, "--fit", "--limit", "--lufs", "-16", "--true-peak-dbtp", "-1"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    wav, nf = m.synthesize(ids, puncts, np.zeros(g.E, F), g.max_seq_len, fitted=True)[:2]
    before, want, after, limited = m.deliver(wav[:nf * HOP], -16.0, -1.0)
    got = re.search(r"limiter: true peak (\S+) dBTP before, (\S+) dBTP after .* least gain (\S+) \((\S+) dB\), limited samples (\d+)", r.stdout)
    assert got, r.stdout
    assert got.groups() == ("%.2f" % want.true_peak_before_dbtp, "%.2f" % want.true_peak_after_dbtp, "%.6f" % want.min_gain,
                            "%.2f" % want.reduction_db, str(want.limited_samples)), (r.stdout, want)
    assert re.search(r"loudness before the gain: .* gain %s" % re.escape("%.6f" % before.gain), r.stdout), r.stdout
    assert re.search(r"loudness after the limiter: integrated %s LUFS" % re.escape("%.2f" % after.integrated_lufs), r.stdout), r.stdout
    pcm = _pcm(out)
    assert pcm.size == nf * HOP and np.abs(pcm - np.clip(limited, -1, 1)).max() <= 1.0 / 32768.0 + 1e-7       # PCM16 of the limited waveform
    # a file: --limit IN.wav
    r = subprocess.run([cli, "-m", tiny.path, "--limit", out, "-o", lim, "--limit-dbtp", "-9", "--limit-gain-db", "6", "--limit-attack-ms", "1",
                        "--limit-release-ms", "20"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    q = capi.Limiter.from_dbtp(-9.0, gain_db=6.0, attack_ms=1.0, release_ms=20.0, sampling_rate=SR)
    assert (q.attack, q.release) == (22, 441)
    want, limited = m.limit_wave(pcm, q)
    got = re.search(r"true peak (\S+) dBTP before, (\S+) dBTP after .* least gain (\S+) \((\S+) dB\), limited samples (\d+)", r.stdout)
    assert got and got.groups() == ("%.2f" % want.true_peak_before_dbtp, "%.2f" % want.true_peak_after_dbtp, "%.6f" % want.min_gain,
                                    "%.2f" % want.reduction_db, str(want.limited_samples)), (r.stdout, want)
    assert want.limited_samples > 0
    assert np.abs(_pcm(lim) - np.clip(limited, -1, 1)).max() <= 1.0 / 32768.0 + 1e-7
    # usage errors
    for bad in (["--limit", out, "-o", lim], ["--limit"], ["--limit-dbtp", "-1"], ["--limit", out, "--limit-dbtp", "1"]):
        r = subprocess.run([cli, "-m", tiny.path] + bad, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2, (bad, r.returncode, r.stderr[-500:])


# ---- 7. arguments -------------------------------------------------------------------------------------------------------------------------------

def test_arguments_are_refused_by_name(tiny):
    from zerovox_cpp_amd import capi
    m = tiny.m
    x = LH.speech(50, 4, 0.3)
    for q, word in ((capi.Limiter(-1.0, 0.5, 1, 1), "gain"), (capi.Limiter(1.0, 0.0, 1, 1), "ceiling"), (capi.Limiter(1.0, 1.5, 1, 1), "ceiling"),
                    (capi.Limiter(1.0, 0.5, 0, 1), "attack"), (capi.Limiter(1.0, 0.5, 2048, 1), "attack"), (capi.Limiter(1.0, 0.5, 1, 0), "release"),
                    (capi.Limiter(1.0, 0.5, 1, 6145), "release"), (capi.Limiter(float("nan"), 0.5, 1, 1), "gain")):
        with pytest.raises(capi.ZvError) as e:
            m.limit_wave(x, q)
        assert ("limiter " + word) in str(e.value) and "zv_limit_wave" in str(e.value), (word, str(e.value))
        with pytest.raises(capi.ZvError) as e:
            m.limit_wave_batch([x, x], [capi.Limiter(1.0, 0.5, 1, 1), q])
        assert "utterance 1: limiter " + word in str(e.value), (word, str(e.value))
    with pytest.raises(capi.ZvError) as e:
        capi.limit_design(3999)
    assert "sampling_rate" in str(e.value)
    with pytest.raises(capi.ZvError) as e:
        capi.limit_design(SR, -1.0)
    assert "attack_ms" in str(e.value)
    _same("after the refusals", m.limit_wave(x, None), LM.rule(tiny.D, x, x.size, None, SR)[:2])
