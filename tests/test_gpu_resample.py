"""-m gpu: sample-rate conversion and PCM16 delivery (include/zerovox_amd.h "resampling") on the tiny synthetic checkpoint (22 050 Hz, hop
300; the kernels depend on the table, the ratio, the lengths and the flags alone).

Every expectation is the rule restated in numpy (tests/resample_rule.py) on a table that is data: random entries, or what the library
itself returns (capi.resample_design).  There is no tolerance anywhere: every f32 sample, every int16 sample and every field of the
report has the rule's bits.  The shapes and the assertions that they reach their branches are tests/resample_shapes.py's, which
tests/test_resample_cpu.py runs without a device too.
  * caller's tables with random entries, (L, M, P) from (1, 1, 2) to (1 280, 441, 2), (1, 1, 512) and (1, 8, 4): inputs of 1, 2, half - 1 and
    half samples, output counts on either side of one and of two of the table's own tiles (R = 8, 4, 2, 1), last outputs whose base is and is not the last sample; NaN, +-inf
    and -0.0 in the first and last sample and just either side of a tile's staged span; silence;
  * dither off and on under the seeds 0, 1 and 0xFFFFFFFF; only out, only pcm, both;
  * designed tables for 22050 -> 48000, 8000, 16000 and 48000 -> 22050 on a speech-like signal; a full-scale square wave that clips;
  * a ragged batch of seven against its single calls under seed + u; the same batch after zv_debug_poison of lane 0 with both bytes;
  * one batch in two launch groups;
  * calls beside a batch in flight, around synthesis calls, after a much longer and a much shorter call;
  * Model.deliver with and without the new keywords; the two command-line forms;
  * arguments refused by name."""
import os
import re
import subprocess
import types
import wave

import numpy as np
import pytest

import resample_rule as RR
import resample_shapes as RH

pytestmark = pytest.mark.gpu

_M = {}
F = np.float32
SR, HOP = 22050, 300


@pytest.fixture
def tiny(ckpt):
    from zerovox_cpp_amd import capi
    if "e" not in _M:
        path, g, _ = ckpt("tiny")
        _M["e"] = types.SimpleNamespace(m=capi.Model(path, 0), g=g, path=path, designs={})
    e = _M["e"]
    assert e.g.sampling_rate == SR and e.g.hop_size == HOP
    e.m.set_graph_mode(False)
    return e


def teardown_module(module):
    if "e" in _M:
        _M["e"].m.close()
    _M.clear()


def _design(e, rate_in, rate_out):
    """the library's table for a pair of rates, as data to the rule -> (L, M, table)"""
    from zerovox_cpp_amd import capi
    if (rate_in, rate_out) not in e.designs:
        e.designs[(rate_in, rate_out)] = capi.resample_design(rate_in, rate_out)
    return e.designs[(rate_in, rate_out)]


def _ask(h, M, dither=False, seed=0):
    from zerovox_cpp_amd import capi
    return capi.Resample(table=h, M=M, dither=dither, seed=seed)


def _same(what, got, want, out=True, pcm=True):
    (res, y, q), (wres, wy, wq) = got, want
    assert (res.n_out, fb(res.sample_peak)) == (wres.n_out, fb(wres.sample_peak)), (what, res, wres)
    assert res.clipped == (wres.clipped if pcm else 0), (what, res, wres)
    if out:
        assert y.shape == wy.shape and y.dtype == F, what
        bad = np.flatnonzero(y.view(np.uint32) != wy.view(np.uint32))
        assert bad.size == 0, (what, bad.size, bad[:6], y[bad[0]], wy[bad[0]])
    else:
        assert y is None, what
    if pcm:
        assert q.shape == wq.shape and q.dtype == np.int16, what
        bad = np.flatnonzero(q != wq)
        assert bad.size == 0, (what, bad.size, bad[:6], q[bad[0]], wq[bad[0]])
    else:
        assert q is None, what


def fb(v):
    return RR.fbits(v)


def _want(h, M, x, dither=False, seed=0):
    return RR.rule(h, M, x, dither, seed)[:3]


# ---- 1. caller's tables -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", RH.TABLES, ids=lambda s: "%d_%d_%d" % s)
def test_callers_table_has_the_rules_bits(tiny, shape):
    m = tiny.m
    mine = [c for c in RH.cases() if (c.L, c.M, c.table.shape[1]) == shape]
    assert mine
    RH.check_targets()
    for i, c in enumerate(mine):
        _same(c.name, m.resample_wave(c.x, _ask(c.table, c.M), out=True, pcm=True), _want(c.table, c.M, c.x))
        seed = RH.SEEDS[i % 3]
        want = _want(c.table, c.M, c.x, True, seed)
        _same((c.name, "dither", seed), m.resample_wave(c.x, _ask(c.table, c.M, True, seed), out=True, pcm=True), want)
        if i % 3 == 0:                                                          # the three selections of outputs
            _same((c.name, "out"), m.resample_wave(c.x, _ask(c.table, c.M, True, seed), out=True, pcm=False), want, pcm=False)
            _same((c.name, "pcm"), m.resample_wave(c.x, _ask(c.table, c.M, True, seed), out=False, pcm=True), want, out=False)


def test_every_seed_on_one_shape(tiny):
    m = tiny.m
    h, x = RH.table(320, 147, 8), RH.noise(5, 700, 0.9)
    got = []
    for seed in RH.SEEDS:
        want = _want(h, 147, x, True, seed)
        got.append(m.resample_wave(x, _ask(h, 147, True, seed), pcm=True))
        _same(("seed", seed), got[-1], want)
    assert (got[0][2] != got[1][2]).any() and (got[1][2] != got[2][2]).any()     # the seeds dither differently
    plain = m.resample_wave(x, _ask(h, 147, False, 7), pcm=True)                 # without the flag the seed is not looked at
    _same("no dither", plain, _want(h, 147, x))
    assert (plain[1].view(np.uint32) == got[0][1].view(np.uint32)).all()         # the f32 output never sees the dither


# ---- 2. designed tables -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pair", RH.DESIGNED, ids=lambda p: "%d_%d" % p)
def test_designed_table_on_a_speech_like_signal(tiny, pair):
    from zerovox_cpp_amd import capi
    m = tiny.m
    L, M, h = _design(tiny, *pair)
    assert (L, M, h.shape[1]) == RR.sizes(*pair) and h.dtype == F
    assert float(np.abs(h.astype(np.float64) - RR.design(*pair)[2]).max()) <= 2.0 ** -23      # the library's table is the header's formula
    x = RH.speech(70, 3000)
    for dither, seed in ((False, 0), (True, 3)):
        want = _want(h, M, x, dither, seed)
        ask = capi.Resample(pair[0], pair[1], dither=dither, seed=seed)
        _same((pair, dither, "designed"), m.resample_wave(x, ask, pcm=True), want)
        _same((pair, dither, "as a caller's table"), m.resample_wave(x, _ask(h, M, dither, seed), pcm=True), want)
    assert capi.resample_count(3000, L, M) == want[0].n_out


def test_full_scale_square_wave_clips(tiny):
    from zerovox_cpp_amd import capi
    L, M, h = _design(tiny, 22050, 48000)
    x = RH.square()
    want = _want(h, M, x)
    assert want[0].clipped > 0 and want[0].sample_peak > F(1)                    # on the rule first
    _same("square", tiny.m.resample_wave(x, capi.Resample(22050, 48000), pcm=True), want)
    same = tiny.m.resample_wave(x, capi.Resample(22050, 22050), pcm=True)        # rate_in == rate_out is no special case: a low-pass
    L1, M1, h1 = _design(tiny, 22050, 22050)
    assert (L1, M1) == (1, 1)
    _same("square at the same rate", same, _want(h1, 1, x))


# ---- 3. batches -----------------------------------------------------------------------------------------------------------------------------------

def _batch_want(h, M, xs, dither, seed):
    return [_want(h, M, x, dither, (seed + u) & 0xFFFFFFFF) for u, x in enumerate(xs)]


def test_ragged_batch_equals_single_calls_and_the_rule(tiny):
    from zerovox_cpp_amd import capi
    m = tiny.m
    xs = RH.ragged_batch()
    assert len(xs) == 7
    L, M, h = _design(tiny, 22050, 8000)
    for dither, seed in ((False, 0), (True, 0xFFFFFFFD)):                        # seed + u wraps past 2^32
        want = _batch_want(h, M, xs, dither, seed)
        single = [m.resample_wave(x, capi.Resample(22050, 8000, dither=dither, seed=(seed + u) & 0xFFFFFFFF), pcm=True) for u, x in enumerate(xs)]
        batch = m.resample_wave_batch(xs, capi.Resample(22050, 8000, dither=dither, seed=seed), pcm=True)
        for u in range(7):
            _same(("single", dither, u), single[u], want[u])
            _same(("batch", dither, u), batch[u], want[u])
    g = RH.table(3, 2, 4)
    want = _batch_want(g, 2, xs, True, 5)
    for u, got in enumerate(m.resample_wave_batch(xs, _ask(g, 2, True, 5), out=False, pcm=True)):
        _same(("batch, pcm only", u), got, want[u], out=False)
    for u, got in enumerate(m.resample_wave_batch(xs, _ask(g, 2, True, 5), out=True, pcm=False)):
        _same(("batch, out only", u), got, want[u], pcm=False)


def test_poisoned_lane_leaves_the_bits_unchanged(tiny):
    from zerovox_cpp_amd import capi
    m = tiny.m
    xs = RH.ragged_batch()
    ask = capi.Resample(22050, 16000, dither=True, seed=11)
    first = m.resample_wave_batch(xs, ask, pcm=True)
    for byte in (0x00, 0xFF):
        m.poison(byte, 0)
        for u, got in enumerate(m.resample_wave_batch(xs, ask, pcm=True)):
            _same(("poison", byte, u), got, first[u])
        m.poison(byte, 0)
        _same(("poison, single", byte), m.resample_wave(xs[3], capi.Resample(22050, 16000, dither=True, seed=14), pcm=True), first[3])


def test_a_batch_across_a_launch_groups_end(tiny):
    """Input plus output samples that cross 2^26: utterances 0 .. 5 are one launch group, 6 .. 10 the next, whose segment offsets start at
    0 again in an I/O block that is reused.  A caller's two-tap table keeps the rule cheap."""
    m = tiny.m
    S, L, M, h = RH.group_batch(m.max_frames() * HOP)                            # (the cut is asserted there)
    block = RH.noise(600, 1 << 20, 0.9)
    xs = [np.resize(np.roll(block, 4099 * u), s) for u, s in enumerate(S)]
    want = _batch_want(h, M, xs, True, 21)
    assert all(w[0].clipped > 0 for w in want[:7])
    for u, got in enumerate(m.resample_wave_batch(xs, _ask(h, M, True, 21), out=True, pcm=True)):
        _same(("batch", u), got, want[u])


# ---- 4. history -------------------------------------------------------------------------------------------------------------------------------------

def _utterances(g):
    from zerovox_cpp_amd import synth
    return [(*synth.encoder_inputs(g, 8300 + i, N), T) for i, (N, T) in enumerate(((6, 40), (3, 17), (9, 64)))]


def test_calls_around_it_leave_the_bits_unchanged(tiny):
    from zerovox_cpp_amd import capi
    m, g = tiny.m, tiny.g
    xs = RH.ragged_batch()
    L, M, h = _design(tiny, 22050, 48000)
    ask = capi.Resample(22050, 48000, dither=True, seed=2)
    want = _batch_want(h, M, xs, True, 2)

    def check(what):
        for u, got in enumerate(m.resample_wave_batch(xs, ask, pcm=True)):
            _same((what, "batch", u), got, want[u])
        _same((what, "single"), m.resample_wave(xs[3], capi.Resample(22050, 48000, dither=True, seed=5), pcm=True), want[3])

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
    long = RH.speech(710, 3000 * HOP, 0.4)                                      # the I/O block grows ...
    first = m.resample_wave(long, ask, pcm=True)
    check("after a much longer call")
    m.resample_wave(xs[0], ask)                                                 # ... and is reused by a call of one sample
    check("after a much shorter call")
    _same("the long call again", m.resample_wave(long, ask, pcm=True), first)
    other = m.resample_wave(xs[3], capi.Resample(22050, 8000), pcm=True)        # another design in between: the kept tables do not mix
    _same("another design", other, _want(_design(tiny, 22050, 8000)[2], 441, xs[3]))
    check("after another design")


# ---- 5. the delivery chain ------------------------------------------------------------------------------------------------------------------------

def test_deliver_with_and_without_the_new_keywords(tiny):
    from zerovox_cpp_amd import capi, synth
    m, g = tiny.m, tiny.g
    ids, puncts, style = synth.encoder_inputs(g, 9, 12)
    wav, nf = m.synthesize(ids, puncts, style, 64)[:2]
    # one by one: loudness -> limiter -> resample
    before, _ = m.loudness_wave(wav, capi.Loudness.from_lufs(-16.0), nf, apply=False)
    a, r = capi.limit_design(SR)
    lim, limited = m.limit_wave(wav, capi.Limiter(float(before.gain), float(F(10.0 ** (-1.0 / 20.0))), a, r), nf)
    rs, _, pcm = m.resample_wave(limited, capi.Resample(SR, 8000), out=False, pcm=True)
    got = m.deliver(wav, -16.0, -1.0, n_frames=nf, rate=8000, pcm16=True)
    assert len(got) == 6
    assert (got[3].view(np.uint32) == limited.view(np.uint32)).all() and got[1].limited_samples == lim.limited_samples
    assert (got[4].n_out, got[4].clipped, fb(got[4].sample_peak)) == (rs.n_out, rs.clipped, fb(rs.sample_peak))
    assert got[5].dtype == np.int16 and (got[5] == pcm).all()
    L, M, h = _design(tiny, SR, 8000)
    _same("deliver against the rule", (got[4], None, got[5]), _want(h, M, limited), out=False)
    assert got[4].n_out == RR.count(limited.size, L, M) == -(-limited.size * 160 // 441)
    dithered = m.deliver(wav, -16.0, -1.0, n_frames=nf, rate=8000, pcm16=True, dither=True)
    _same("deliver, dithered", (dithered[4], None, dithered[5]), _want(h, M, limited, True, 0), out=False)
    f32 = m.deliver(wav, -16.0, -1.0, n_frames=nf, rate=48000)
    L, M, h = _design(tiny, SR, 48000)
    _same("deliver, f32 at 48 kHz", (f32[4], f32[5], None), _want(h, M, limited), pcm=False)
    # without the new keywords: what it gave
    old = m.deliver(wav, -16.0, -1.0, n_frames=nf)
    assert len(old) == 4 and (old[3].view(np.uint32) == limited.view(np.uint32)).all() and old[1].limited_samples == lim.limited_samples
    assert fb(old[0].gain) == fb(before.gain)


# ---- 6. the command line --------------------------------------------------------------------------------------------------------------------------

def _pcm(path):
    with wave.open(path, "rb") as w:
        assert w.getnchannels() == 1 and w.getsampwidth() == 2
        return w.getframerate(), np.frombuffer(w.readframes(w.getnframes()), "<i2")


def test_command_line_resamples_a_file_and_a_synthesis_run(tiny, tmp_path):
    from zerovox_cpp_amd import capi, synth
    m, g = tiny.m, tiny.g
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zerovox.cpp_amd", "zerovox")
    # a 48 kHz recording -> the model's rate -> --analyze accepts it
    rec, at_model, mel = str(tmp_path / "rec48.wav"), str(tmp_path / "rec22.wav"), str(tmp_path / "rec.mel")
    x16 = np.round(RH.LS.speech(48000, 90, 30000, 0.4).astype(np.float64) * 32768.0).astype(np.int16)
    capi.write_wav_pcm16(rec, x16, 48000)
    assert _pcm(rec)[0] == 48000 and (_pcm(rec)[1] == x16).all()
    r = subprocess.run([cli, "-m", tiny.path, "--analyze", rec, "--mel-out", mel], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "48000 Hz" in r.stderr                          # the refusal stays
    r = subprocess.run([cli, "-m", tiny.path, "--resample", rec, "-o", at_model, "--rate", str(SR)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    L, M, h = _design(tiny, 48000, SR)
    x = x16.astype(F) / F(32768.0)
    want = _want(h, M, x)
    rate, got = _pcm(at_model)
    assert rate == SR and got.size == want[0].n_out and (got == want[2]).all()
    assert re.search(r"48000 -> 22050 Hz \(L 147, M 320, %d taps per phase\), 30000 -> %d samples, sample peak %s, clipped %d" %
                     (h.shape[1], want[0].n_out, re.escape("%.6f" % want[0].sample_peak), want[0].clipped), r.stdout), r.stdout
    r = subprocess.run([cli, "-m", tiny.path, "--analyze", at_model, "--mel-out", mel], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and os.path.getsize(mel) == (want[0].n_out // HOP) * g.num_mels * 4, (r.stderr[-2000:], r.stdout)
    # other design parameters and dither
    r = subprocess.run([cli, "-m", tiny.path, "--resample", rec, "-o", at_model, "--rate", "16000", "--resample-zeros", "12", "--resample-beta", "6.5",
                        "--resample-cutoff", "0.8", "--dither", "--dither-seed", "77"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    L, M, h = capi.resample_design(48000, 16000, 12, 6.5, 0.8)
    assert (_pcm(at_model)[1] == _want(h, M, x, True, 77)[2]).all() and _pcm(at_model)[0] == 16000
    # a synthesis run: --out-rate 8000 --dither
    ids, puncts, _ = synth.encoder_inputs(g, 9, 12)
    out, utt = str(tmp_path / "out.wav"), str(tmp_path / "utt.txt")
    open(utt, "w").write(" ".join(map(str, ids)) + "\n" + " ".join(map(str, puncts)) + "\n0\n")
    r = subprocess.run([cli, "-m", tiny.path, "-u", utt, "-o", out, "--fit", "--limit", "--lufs", "-16", "--true-peak-dbtp", "-1", "--out-rate", "8000",
                        "--dither"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    wav, nf = m.synthesize(ids, puncts, np.zeros(g.E, F), g.max_seq_len, fitted=True)[:2]
    limited = m.deliver(wav[:nf * HOP], -16.0, -1.0)[3]
    L, M, h = _design(tiny, SR, 8000)
    want = _want(h, M, limited, True, 0)
    rate, got = _pcm(out)
    assert rate == 8000 and got.size == want[0].n_out and (got == want[2]).all()
    r = subprocess.run([cli, "-m", tiny.path, "-u", utt, "-o", out, "--fit", "--out-rate", "48000"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    L, M, h = _design(tiny, SR, 48000)
    assert _pcm(out)[0] == 48000 and (_pcm(out)[1] == _want(h, M, wav[:nf * HOP])[2]).all()
    # usage errors
    for bad in (["--resample", rec, "-o", out], ["--rate", "8000"], ["--resample", rec, "--rate", "3999"], ["--resample", rec, "--rate", "8000", "--out-rate", "8000"],
                ["--dither"], ["--resample-zeros", "12"], ["--resample", rec, "--rate", "8000", "--resample-zeros", "3"],
                ["--resample", rec, "--rate", "8000", "--resample-beta", "21"], ["--resample", rec, "--rate", "8000", "--resample-cutoff", "0"],
                ["--resample", rec, "--rate", "8000", "--analyze", rec, "--mel-out", mel], ["--resample"]):
        r = subprocess.run([cli, "-m", tiny.path] + bad, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2, (bad, r.returncode, r.stderr[-500:])
    # a ratio the design refuses is an error by name, not a usage error
    r = subprocess.run([cli, "-m", tiny.path, "--resample", rec, "-o", out, "--rate", "44099"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "resample L" in r.stderr, r.stderr[-500:]


# ---- 7. arguments ---------------------------------------------------------------------------------------------------------------------------------

def test_arguments_are_refused_by_name(tiny):
    from zerovox_cpp_amd import capi
    m = tiny.m
    x = RH.noise(50, 400)
    R = capi.Resample
    h = RH.table(3, 2, 4)
    nan = h.copy()
    nan[1, 2] = np.nan
    for q, word in ((R(3999, 8000), "resample rate_in"), (R(SR, 768001), "resample rate_out"), (R(SR, 22051), "resample L"), (R(5132, 4000), "resample M"),
                    (R(4000, 36000), "resample ratio"), (R(SR, 8000, zeros=3), "resample zeros"), (R(SR, 8000, zeros=65), "resample zeros"),
                    (R(SR, 8000, beta=-1.0), "resample beta"), (R(SR, 8000, beta=20.5), "resample beta"), (R(SR, 8000, cutoff=1.5), "resample cutoff"),
                    (R(SR, 8000, cutoff=float("nan")), "resample cutoff"), (R(48000, 8000, zeros=64), "resample P"), (R(6390, 6400, zeros=64), "resample table size"),
                    (R(SR, 8000, flags=2), "resample flags"), (R(table=np.tile(h, (2, 1)), M=4), "common divisor"), (R(table=nan, M=2), "resample table holds"),
                    (R(table=h, M=0), "resample M"), (R(table=h, M=25), "resample ratio"), (R(table=h[:, :3], M=2), "resample P"),
                    (R(table=np.zeros((129, 512), F), M=128), "resample table size"), (R(table=np.zeros((1281, 2), F), M=1280), "resample L")):
        with pytest.raises(capi.ZvError) as e:
            m.resample_wave(x, q, pcm=True)
        assert word in str(e.value) and "zv_resample_wave:" in str(e.value), (word, str(e.value))
        with pytest.raises(capi.ZvError) as e:
            m.resample_wave_batch([x, x], q)
        assert word in str(e.value) and "zv_resample_wave_batch:" in str(e.value), (word, str(e.value))
    with pytest.raises(capi.ZvError) as e:
        m.resample_wave(x, R(SR, 8000), out=False, pcm=False)
    assert "out and pcm are both NULL" in str(e.value)
    with pytest.raises(capi.ZvError) as e:
        m.resample_wave(np.zeros(0, F), R(SR, 8000))
    assert "S_in = 0" in str(e.value)
    with pytest.raises(capi.ZvError) as e:
        m.resample_wave_batch([x, np.zeros(0, F)], R(SR, 8000))
    assert "utterance 1: S_in = 0" in str(e.value)
    with pytest.raises(capi.ZvError) as e:
        m.resample_wave(np.zeros(m.max_frames() * HOP + 1, F), R(table=np.ones((1, 2), F), M=1))
    assert "S_in" in str(e.value) and "zv_max_frames" in str(e.value)
    with pytest.raises(TypeError):
        m.resample_wave(x, None)
    for args, word in (((3999, 8000), "rate_in"), ((SR, 8000, 3), "zeros"), ((SR, 8000, 0, 25.0), "beta"), ((SR, 8000, 0, 0.0, 2.0), "cutoff")):
        with pytest.raises(capi.ZvError) as e:
            capi.resample_design(*args)
        assert word in str(e.value) and "zv_resample_design" in str(e.value)
    L, M, t = _design(tiny, SR, 8000)
    _same("after the refusals", m.resample_wave(x, R(SR, 8000), pcm=True), _want(t, M, x))
