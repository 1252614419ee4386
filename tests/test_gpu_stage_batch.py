"""-m gpu: the three stage calls over a batch (include/zerovox_amd.h "stages in batches": zv_encode_batch, zv_decode_batch,
zv_vocode_batch, zv_vocode_batch_begin / _end) on the synthetic `small` and `tiny` checkpoints.

Every comparison is bit for bit (uint32 views) against the single calls on the same arguments, or against zv_synthesize_batch, and lane
0's arena, I/O block and pinned block are poisoned (zv_debug_poison, 0xFF bytes: NaN as f32, -1 as int32) between the two sides of a
comparison and between the single calls, so that a write that never happened cannot pass on what the call before it left behind.
 1 encode   n = (5, 16, 9), T = (24, 40, 17): a prosody, forced per-phoneme frames, a target; hidden, n_frames, durations
 2 decode   those hiddens and one of T = 1
 3 vocode   T = (1, 24, 65, 37), one mel with a constant padded tail; eager, graph mode (capture, then a replay with other values and
            another length under the same key), ZV_VOC_RUNS=0
 4 chain    vocode_batch(decode_batch(encode_batch)) against synthesize_batch
 5 plan     the planning call's n_frames as capacities, against synthesize_batch(fitted=True)
 6 groups   65 utterances (two launch groups) through all three stages; 4 long mels whose waveforms pass 16 MiB (tail groups)
 7 lanes    two vocode batches in flight, ended in both orders; the calls a busy, mismatched or idle lane refuses
 8 errors   every rejected argument: ZV_ERR_ARG, a message naming entry point, utterance and argument, no launch, no graph lookup
 9 cli      zerovox --plan prints the planning call's frame counts for every utterance of the -u file"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ERR_ARG = 5
NS, TS = (5, 16, 9), (24, 40, 17)
_M = {}


@pytest.fixture(scope="module")
def small(ckpt):
    from zerovox_cpp_amd import capi
    path, g, tensors = ckpt("small")
    if "small" not in _M:
        _M["small"] = capi.Model(path, 0)
    _M["small"].set_graph_mode(False)
    return _M["small"], g, tensors


@pytest.fixture(scope="module")
def tiny(ckpt):
    from zerovox_cpp_amd import capi
    path, g, tensors = ckpt("tiny")
    if "tiny" not in _M:
        _M["tiny"] = capi.Model(path, 0)
    _M["tiny"].set_graph_mode(False)
    return _M["tiny"], g, tensors


def teardown_module(module):
    for v in _M.values():
        if hasattr(v, "close"):
            v.close()
    _M.clear()


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _same(got, want, what):
    a, b = _bits(got), _bits(want)
    assert a.shape == b.shape and np.array_equal(a, b), (what, int((a != b).sum()) if a.shape == b.shape else (a.shape, b.shape))


def _poison(m, lane=0):
    return m.poison(0xFF, lane)      # (arena, I/O block, pinned block) bytes filled: 0 for a block the lane does not have yet


def _utts(g):
    """test 1's utterances as synthesize_batch's tuples: a prosody, forced per-phoneme frames (30 of the 40), a target (12 of the 17)"""
    from zerovox_cpp_amd import synth
    base = [synth.encoder_inputs(g, 9101 + k, n) + (T,) for k, (n, T) in enumerate(zip(NS, TS))]
    forced = (30 // 16 + (np.arange(16) < 30 % 16)).astype(np.int32)
    return [base[0] + ((1.25, 1.0, 0.1, 1.0, -0.1), None, None), base[1] + (None, dict(duration_frames=forced), None), base[2] + (None, None, 12)]


def _encode_singles(m, utts, Ts=None):
    """the reference of tests 1, 2, 4: encode per utterance, a poison ahead of each; shared by the tests of a module run"""
    key = ("enc", tuple(Ts or ()))
    if key not in _M:
        out = []
        for k, (ids, puncts, style, T, prosody, phonemes, target) in enumerate(utts):
            _poison(m)
            out.append(m.encode(ids, puncts, style, Ts[k] if Ts else T, prosody=prosody, phonemes=phonemes, return_durations=True, target_frames=target))
        _M[key] = out
    return _M[key]


# ---- 1. encode ------------------------------------------------------------------------------------------------------------------

def test_encode_batch_equals_encode_and_the_chains_frame_counts(small):
    m, g, _ = small
    utts = _utts(g)
    want = _encode_singles(m, utts)
    assert want[1]["n_frames"] == 30 and want[2]["n_frames"] == 12 and all(w["n_frames"] > 0 for w in want)
    _poison(m)
    got = m.encode_batch(utts, return_durations=True)
    filled = _poison(m)
    assert filled[0] > 0 and filled[1] >= sum(TS) * g.E * 4 and filled[2] >= sum(TS) * g.E * 4, filled      # the hook covers what the batch used
    plan = m.encode_batch(utts, return_hidden=False, return_durations=True)
    _poison(m)
    chain = m.synthesize_batch(utts, return_durations=True)
    for u, (a, b, p, c) in enumerate(zip(got, want, plan, chain)):
        assert a["hidden"].shape == (TS[u], g.E) and a["durations"].shape == (NS[u],)
        _same(a["hidden"], b["hidden"], ("hidden", u))
        assert a["n_frames"] == b["n_frames"] == p["n_frames"] == c[1], (u, a["n_frames"], b["n_frames"], p["n_frames"], c[1])
        for d, who in ((a["durations"], "batch"), (p["durations"], "planning"), (c[2], "chain")):
            assert np.array_equal(d, b["durations"]), (u, who, d, b["durations"])
        assert "hidden" not in p
    # a batch without options is the plain encode
    plain = [u[:4] for u in utts]
    _poison(m)
    got = m.encode_batch(plain)
    for u, (ids, puncts, style, T) in enumerate(plain):
        _poison(m)
        ref = m.encode(ids, puncts, style, T)
        _same(got[u]["hidden"], ref["hidden"], ("plain hidden", u))
        assert got[u]["n_frames"] == ref["n_frames"] and "durations" not in got[u]


# ---- 2. decode ------------------------------------------------------------------------------------------------------------------

def test_decode_batch_equals_decode(small):
    from zerovox_cpp_amd import synth
    m, g, _ = small
    utts = _utts(g)
    hid = [e["hidden"] for e in _encode_singles(m, utts)] + [synth.decoder_hidden(g, 9150, 1)]
    sty = [u[2] for u in utts] + [synth.encoder_inputs(g, 9151, 2)[2]]
    assert [h.shape[0] for h in hid] == [24, 40, 17, 1]
    want = []
    for h, s in zip(hid, sty):
        _poison(m)
        want.append(m.decode(h, s))
    _poison(m)
    got = m.decode_batch(hid, sty)
    assert len(got) == 4
    for u in range(4):
        assert np.isfinite(got[u]).all()
        _same(got[u], want[u], ("mel", u))


# ---- 3. vocode ------------------------------------------------------------------------------------------------------------------

def _mels(g, tensors, Ts, seed):
    from zerovox_cpp_amd import synth
    mels = [synth.vocoder_mel(g, tensors, seed + k, T) for k, T in enumerate(Ts)]
    k = int(np.argmax(Ts))
    mels[k][Ts[k] // 2:] = mels[k][Ts[k] // 2]            # a constant padded tail: a batch builds a run table for it
    return mels


def _vocode_singles(m, mels):
    out = []
    for mel in mels:
        _poison(m)
        out.append(m.vocode(mel))
    return out


@pytest.mark.parametrize("mode", ["eager", "graph", "runs_off"])
def test_vocode_batch_equals_vocode(small, mode):
    from zerovox_cpp_amd import capi
    m, g, tensors = small
    first, second = _mels(g, tensors, (1, 24, 65, 37), 9300), _mels(g, tensors, (1, 24, 65, 30), 9400)
    with capi.switches(**(dict(ZV_VOC_RUNS=0) if mode == "runs_off" else {})):
        if ("voc", mode == "runs_off") not in _M:
            _M[("voc", mode == "runs_off")] = [_vocode_singles(m, first), _vocode_singles(m, second)]
        want = _M[("voc", mode == "runs_off")]
        m.set_graph_mode(mode == "graph")
        _poison(m)
        s0 = m.graph_cache_stats()
        got = m.vocode_batch(first)
        s1 = m.graph_cache_stats()
        _poison(m)
        again = m.vocode_batch(second)              # other values, 37 -> 30 frames: the same capacities, the same graph
        s2 = m.graph_cache_stats()
        m.set_graph_mode(False)
    for u in range(4):
        _same(got[u], want[0][u], (mode, "first", u))
        _same(again[u], want[1][u], (mode, "second", u))
    if mode == "graph":
        assert (s1.lookups - s0.lookups, s1.captures - s0.captures) == (1, 1), (s0, s1)
        assert (s2.lookups - s1.lookups, s2.hits - s1.hits, s2.captures - s1.captures) == (1, 1, 0), (s1, s2)
    else:
        assert s2.lookups == s0.lookups


# ---- 4. chain -------------------------------------------------------------------------------------------------------------------

def test_the_three_stage_batches_in_sequence_equal_synthesize_batch(small):
    m, g, _ = small
    utts = _utts(g)
    _poison(m)
    want = m.synthesize_batch(utts, return_durations=True)
    _poison(m)
    enc = m.encode_batch(utts, return_durations=True)
    _poison(m)
    mels = m.decode_batch([e["hidden"] for e in enc], [u[2] for u in utts])
    _poison(m)
    wavs = m.vocode_batch(mels)
    for u in range(3):
        assert enc[u]["n_frames"] == want[u][1] and np.array_equal(enc[u]["durations"], want[u][2])
        _same(wavs[u], want[u][0], ("wav", u))


# ---- 5. the plan story ----------------------------------------------------------------------------------------------------------

def test_planned_capacities_give_the_fitted_batch(small):
    m, g, _ = small
    utts = _utts(g)
    hop = g.hop_size
    _poison(m)
    fitted = m.synthesize_batch(utts, fitted=True)
    _poison(m)
    nf = [p["n_frames"] for p in m.encode_batch(utts, return_hidden=False)]
    assert nf == [f[1] for f in fitted] and all(0 < n <= T for n, T in zip(nf, TS)) and nf[1:] == [30, 12]
    exact = [u[:3] + (n,) + u[4:] for u, n in zip(utts, nf)]                # T[u] = n_frames[u]: the capacities fit exactly
    _poison(m)
    enc = m.encode_batch(exact)
    assert [e["n_frames"] for e in enc] == nf
    _poison(m)
    mels = m.decode_batch([e["hidden"] for e in enc], [u[2] for u in utts])
    _poison(m)
    wavs = m.vocode_batch(mels)
    for u in range(3):
        assert wavs[u].shape == (nf[u] * hop,)
        _same(wavs[u], fitted[u][0][:nf[u] * hop], ("fitted wav", u))
        assert not fitted[u][0][nf[u] * hop:].any()


# ---- 6. groups ------------------------------------------------------------------------------------------------------------------

def test_two_launch_groups_equal_the_single_calls_in_every_stage(tiny):
    from zerovox_cpp_amd import synth
    m, g, tensors = tiny
    utts = [synth.encoder_inputs(g, 9500 + k, 2) + (3,) for k in range(65)]      # 65 utterances: groups of 64 and 1
    _poison(m)
    enc = m.encode_batch(utts)
    hid = [synth.decoder_hidden(g, 9600 + k, 3) for k in range(65)]
    sty = [u[2] for u in utts]
    _poison(m)
    mels = m.decode_batch(hid, sty)
    mel_in = [synth.vocoder_mel(g, tensors, 9700 + k, 3) for k in range(65)]
    _poison(m)
    wavs = m.vocode_batch(mel_in)
    for k in range(65):
        _poison(m)
        e = m.encode(*utts[k])
        assert enc[k]["n_frames"] == e["n_frames"], k
        _same(enc[k]["hidden"], e["hidden"], ("hidden", k))
        _same(mels[k], m.decode(hid[k], sty[k]), ("mel", k))
        _same(wavs[k], m.vocode(mel_in[k]), ("wav", k))


def test_a_vocode_batch_with_tail_groups_equals_vocode(tiny):
    m, g, tensors = tiny
    Ts = (3500, 3497, 3600, 3503)
    assert min(Ts) <= m.max_frames() and sum(Ts) * g.hop_size * 4 > 16 << 20 > (sum(Ts) - 200) * g.hop_size * 4      # just over TAIL_GROUPS_MIN_BYTES
    mels = _mels(g, tensors, Ts, 9800)
    want = _vocode_singles(m, mels)
    _poison(m)
    got = m.vocode_batch(mels)
    for u in range(4):
        _same(got[u], want[u], ("wav", u))


# ---- 7. lanes -------------------------------------------------------------------------------------------------------------------

def test_vocode_batches_in_flight_on_two_lanes(small):
    from zerovox_cpp_amd import capi
    m, g, tensors = small
    a, b = _mels(g, tensors, (1, 24, 65, 37), 9300), _mels(g, tensors, (33, 5, 64), 9900)
    _poison(m)
    want_a = m.vocode_batch(a)
    _poison(m)
    want_b = m.vocode_batch(b)
    for order in ((0, 1), (1, 0)):
        _poison(m, 0)
        m.vocode_batch_begin(0, a)
        m.vocode_batch_begin(1, b)
        got = {lane: m.vocode_batch_end(lane) for lane in order}
        for u in range(4):
            _same(got[0][u], want_a[u], (order, "lane 0", u))
        for u in range(3):
            _same(got[1][u], want_b[u], (order, "lane 1", u))
    # what a busy lane, the other kind's _end and an idle lane refuse; the batch in flight still finishes with the right bits
    m.vocode_batch_begin(1, b)
    with pytest.raises(capi.ZvError, match="lane 1 already has a batch in flight") as e:
        m.vocode_batch_begin(1, a)
    assert e.value.status == ERR_ARG
    assert m.lib.zv_synthesize_batch_end(m.h, 1) == ERR_ARG and b"zv_vocode_batch_end" in m.lib.zv_last_error()
    with pytest.raises(capi.ZvError, match="lane 2 has no batch in flight") as e:
        m.vocode_batch_end(2)
    assert e.value.status == ERR_ARG
    got = m.vocode_batch_end(1)
    for u in range(3):
        _same(got[u], want_b[u], ("after the refusals", u))
    # ... and the reverse: a synthesize batch is not finished by zv_vocode_batch_end
    utts = [u[:4] for u in _utts(g)]
    bc = m.prepare_batch(utts)
    bc.run()
    want = [w.copy() for w in bc.wavs]
    for w in bc.wavs:
        w[:] = 0
    bc.begin(1)
    assert m.lib.zv_vocode_batch_end(m.h, 1) == ERR_ARG and b"zv_synthesize_batch_end" in m.lib.zv_last_error()
    bc.end(1)
    for u in range(3):
        _same(bc.wavs[u], want[u], ("synthesize batch", u))


# ---- 8. errors ------------------------------------------------------------------------------------------------------------------

def _ptrs(arrays):
    return (C.c_void_p * len(arrays))(*[None if a is None else a.ctypes.data for a in arrays])


def test_every_rejected_argument_is_err_arg_and_launches_nothing(small):
    m, g, tensors = small
    lib, h = m.lib, m.h
    utts = _utts(g)
    ids, pun, sty = ([u[k] for u in utts] for k in range(3))
    n, T = (C.c_uint32 * 3)(*NS), (C.c_uint32 * 3)(*TS)
    hid = [np.zeros((t, g.E), np.float32) for t in TS]
    mel = [np.zeros((t, g.num_mels), np.float32) for t in TS]
    wav = [np.zeros(t * g.hop_size, np.float32) for t in TS]
    nf = (C.c_uint32 * 3)()
    big = m.max_frames() + 1

    def Tv(u, v):
        t = list(TS)
        t[u] = v
        return (C.c_uint32 * 3)(*t)

    def drop(arrays, u):
        return _ptrs([None if k == u else a for k, a in enumerate(arrays)])

    bad_id = [a.copy() for a in ids]
    bad_id[1][2] = 9999
    from zerovox_cpp_amd import capi
    pro = (capi.Prosody * 3)(capi.Prosody(), capi.Prosody(), capi.Prosody(duration_scale=0.0))
    tgt = (C.c_uint32 * 3)(0, 41, 0)
    enc = lambda **kw: lib.zv_encode_batch(h, kw.get("n_utt", 3), kw.get("ids", _ptrs(ids)), kw.get("pun", _ptrs(pun)), kw.get("sty", _ptrs(sty)),
                                           kw.get("n", n), kw.get("T", T), kw.get("hid", _ptrs(hid)), kw.get("nf", nf), kw.get("pro"), None, None,
                                           kw.get("tgt"))
    dec = lambda **kw: lib.zv_decode_batch(h, kw.get("n_utt", 3), kw.get("hid", _ptrs(hid)), kw.get("sty", _ptrs(sty)), kw.get("T", T),
                                           kw.get("mel", _ptrs(mel)))
    voc = lambda **kw: lib.zv_vocode_batch(h, kw.get("n_utt", 3), kw.get("mel", _ptrs(mel)), kw.get("T", T), kw.get("wav", _ptrs(wav)))
    beg = lambda **kw: lib.zv_vocode_batch_begin(h, kw.get("lane", 1), kw.get("n_utt", 3), kw.get("mel", _ptrs(mel)), kw.get("T", T),
                                                 kw.get("wav", _ptrs(wav)))
    cases = [
        (enc, dict(ids=None), "zv_encode_batch: ids is NULL"),
        (enc, dict(pun=drop(pun, 1)), "zv_encode_batch: utterance 1: puncts is NULL"),
        (enc, dict(sty=drop(sty, 2)), "zv_encode_batch: utterance 2: styles is NULL"),
        (enc, dict(n=None), "zv_encode_batch: n_phonemes is NULL"),
        (enc, dict(nf=None), "zv_encode_batch: n_frames is NULL"),
        (enc, dict(T=None), "zv_encode_batch: T is NULL"),
        (enc, dict(n_utt=0), "zv_encode_batch: n_utt must be > 0"),
        (enc, dict(n=(C.c_uint32 * 3)(5, 0, 9)), "zv_encode_batch: utterance 1: n_phonemes must be > 0"),
        (enc, dict(T=Tv(0, 0)), "zv_encode_batch: utterance 0: T must be > 0"),
        (enc, dict(T=Tv(2, big)), "zv_encode_batch: utterance 2: T = %d exceeds zv_max_frames()" % big),
        (enc, dict(ids=_ptrs(bad_id)), "zv_encode_batch: utterance 1: phoneme id 9999 at position 2"),
        (enc, dict(pro=pro), "zv_encode_batch: utterance 2: prosody duration_scale = 0"),
        (enc, dict(tgt=tgt), "zv_encode_batch: utterance 1: target_frames = 41 exceeds the capacity T = 40"),
        (dec, dict(hid=None), "zv_decode_batch: hidden is NULL"),
        (dec, dict(hid=drop(hid, 0)), "zv_decode_batch: utterance 0: hidden is NULL"),
        (dec, dict(sty=drop(sty, 1)), "zv_decode_batch: utterance 1: styles is NULL"),
        (dec, dict(mel=drop(mel, 2)), "zv_decode_batch: utterance 2: mel is NULL"),
        (dec, dict(n_utt=0), "zv_decode_batch: n_utt must be > 0"),
        (dec, dict(T=Tv(1, 0)), "zv_decode_batch: utterance 1: T must be > 0"),
        (dec, dict(T=Tv(1, big)), "zv_decode_batch: utterance 1: T = %d exceeds zv_max_frames()" % big),
        (voc, dict(mel=None), "zv_vocode_batch: mel is NULL"),
        (voc, dict(mel=drop(mel, 1)), "zv_vocode_batch: utterance 1: mel is NULL"),
        (voc, dict(wav=None), "zv_vocode_batch: wav is NULL"),
        (voc, dict(wav=drop(wav, 2)), "zv_vocode_batch: utterance 2: wav is NULL"),
        (voc, dict(n_utt=0), "zv_vocode_batch: n_utt must be > 0"),
        (voc, dict(T=Tv(2, 0)), "zv_vocode_batch: utterance 2: T must be > 0"),
        (voc, dict(T=Tv(0, big)), "zv_vocode_batch: utterance 0: T = %d exceeds zv_max_frames()" % big),
        (beg, dict(mel=drop(mel, 0)), "zv_vocode_batch_begin: utterance 0: mel is NULL"),
        (beg, dict(wav=None), "zv_vocode_batch_begin: wav is NULL"),
        (beg, dict(n_utt=0), "zv_vocode_batch_begin: n_utt must be > 0"),
        (beg, dict(T=Tv(1, 0)), "zv_vocode_batch_begin: utterance 1: T must be > 0"),
        (beg, dict(lane=4), "zv_vocode_batch_begin: lane out of range"),
    ]
    m.set_graph_mode(True)
    m.vocode_batch(mel)                             # something is captured: a failed call must not even look it up
    before = m.graph_cache_stats()
    filled = _poison(m)
    for fn, kw, msg in cases:
        assert fn(**kw) == ERR_ARG, msg
        assert lib.zv_last_error().decode().startswith(msg), (msg, lib.zv_last_error().decode())
    after = m.graph_cache_stats()
    m.set_graph_mode(False)
    assert (after.lookups, after.captures, after.entries) == (before.lookups, before.captures, before.entries)
    assert lib.zv_vocode_batch_end(h, 1) == ERR_ARG            # nothing was left in flight by the refused _begin calls
    assert m.poison(0xFF, 0) == filled                          # and no block has grown: nothing was staged
    # a 65-utterance batch does not fit the one launch group of a _begin
    many = [np.zeros((3, g.num_mels), np.float32)] * 65
    with pytest.raises(capi.ZvError, match="zv_vocode_batch_begin: an asynchronous batch must fit one launch group") as e:
        m.vocode_batch_begin(1, many)
    assert e.value.status == ERR_ARG


# ---- 9. the command line: zerovox --plan ------------------------------------------------------------------------------------------

def test_the_cli_plans_every_utterance_of_the_file(small, ckpt, tmp_path):
    import os
    import subprocess
    m, g, _ = small
    path = ckpt("small")[0]
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zerovox.cpp_amd", "zerovox")
    utts = [u[:3] + (g.max_seq_len,) for u in _utts(g)]
    with open(tmp_path / "utts.txt", "w") as f:
        for ids, puncts, style, _T in utts:
            f.write(" ".join(map(str, ids)) + "\n" + " ".join(map(str, puncts)) + "\n" + " ".join(repr(float(x)) for x in style) + "\n\n")
    for flags, prosody in (([], None), (["--duration-scale", "1.5"], (1.5, 1.0, 0.0, 1.0, 0.0))):
        want = [e["n_frames"] for e in m.encode_batch([u + (prosody,) for u in utts], return_hidden=False)]
        r = subprocess.run([cli, "-m", path, "-u", str(tmp_path / "utts.txt"), "--plan"] + flags, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-1000:]
        rows = [line.split() for line in r.stdout.strip().splitlines()]
        assert [(int(a), int(b), int(c)) for a, b, c, _ in rows] == [(u, NS[u], want[u]) for u in range(3)], (rows, want)
        assert [s for *_, s in rows] == ["%.3f" % (n * g.hop_size / g.sampling_rate) for n in want]
