"""-m gpu: per-phoneme controls and phoneme timings (include/zerovox_amd.h zv_phoneme_controls) at the production geometry.

The controls reach the same three device decisions as the per-utterance prosody: the length regulator (lr_fused16_kernel for
utterances of at most 1 024 tokens, lr_scan_kernel beyond: N = 200 and N = 1100 below) and both forms of the pitch / energy bucket
step (the tail of add_layernorm_kernel<true>, or bucket_embed_add_kernel with ZV_LN_TAIL=0).  Checked here:
  * identity controls (NULL struct, NULL fields, explicit identity arrays) give the bits of the _prosody calls;
  * teacher-forced decisions: a numpy float32 restatement of the header's arithmetic from the GPU's own raw taps gives the
    buckets, hidden rows, n_frames and durations exactly;
  * the reference composed layer by layer with the pitch embedding at the GPU's controlled buckets;
  * batches (ragged, graph replay with new values, tail groups, two lanes in flight) = stand-alone calls, timings included;
  * validation and the CLI flags."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ZV_ERR_ARG = 5
_M = {}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


# ---- numpy float32 restatement of include/zerovox_amd.h §per-phoneme controls ----------------------------------------------

def _trunc_int(x64):
    return np.trunc(np.clip(x64, -2.0 ** 31, 2.0 ** 31 - 1)).astype(np.int64)


def restate_buckets(pred, scale, shift, pshift, nbins):
    p = np.asarray(pred, np.float32)
    p = (p * np.float32(scale)).astype(np.float32)
    p = (p + np.float32(shift)).astype(np.float32)
    if pshift is not None:
        p = (p + np.asarray(pshift, np.float32)).astype(np.float32)
    p = (p * np.float32(nbins - 1)).astype(np.float32)
    return np.clip(_trunc_int(p.astype(np.float64) + 0.5), 0, nbins - 1)


def restate_durations(logdur, num_phonemes, T, uscale=1.0, frames=None, scale=None):
    dur = (np.exp(np.asarray(logdur, np.float32).astype(np.float64)) - 1.0).astype(np.float32)
    dur = (dur * np.float32(uscale)).astype(np.float32)
    if scale is not None:
        dur = (dur * np.asarray(scale, np.float32)).astype(np.float32)
    d = np.clip(_trunc_int(dur.astype(np.float64) + 0.5), 0, T)
    if frames is not None:
        fr = np.asarray(frames, np.int64)
        d = np.where(fr >= 0, np.minimum(fr, T), d)
    d[num_phonemes:] = 0
    return d


def timings(d, T):
    c = np.minimum(np.cumsum(d), T)
    return np.diff(np.concatenate([[0], c])).astype(np.int32)


def restated_hidden(features, d, T):
    cum = np.cumsum(d)
    idx = np.searchsorted(cum, np.arange(T), side="right")
    live = idx < len(d)
    out = np.zeros((T, features.shape[1]), np.float32)
    out[live] = features[idx[live]]
    return out, int(min(int(cum[-1]), T))


def identity_arrays(n):
    return dict(duration_frames=np.full(n, -1, np.int32), duration_scale=np.ones(n, np.float32),
                pitch_shift=np.zeros(n, np.float32), energy_shift=np.zeros(n, np.float32))


def check_decisions(e, e0, T, nbins, num_phonemes, prosody=None, pc=None):
    """e: encode with controls, e0: the same utterance uncontrolled; every controlled decision restated from e's raw taps"""
    from zerovox_cpp_amd import capi
    pr = capi._prosody(prosody) or capi.Prosody()
    pc = pc or {}
    for k in ("logdur", "pitch"):
        assert np.array_equal(e[k], e0[k]), k
    assert np.array_equal(e["pitch_bucket"], restate_buckets(e["pitch"], pr.pitch_scale, pr.pitch_shift, pc.get("pitch_shift"), nbins))
    assert np.array_equal(e["energy_bucket"],
                          restate_buckets(e["energy"], pr.energy_scale, pr.energy_shift, pc.get("energy_shift"), nbins))
    d = restate_durations(e["logdur"], num_phonemes, T, pr.duration_scale, pc.get("duration_frames"), pc.get("duration_scale"))
    hid, nf = restated_hidden(e["features"], d, T)
    assert e["n_frames"] == nf, (e["n_frames"], nf)
    assert np.array_equal(e["hidden"], hid), "hidden rows"
    assert np.array_equal(e["durations"], timings(d, T)), "durations"
    assert int(e["durations"].sum()) == e["n_frames"]
    return d


PROSODIES = [None, dict(duration_scale=1.3, pitch_scale=0.9, pitch_shift=0.05, energy_scale=1.1, energy_shift=-0.03)]


def mixed_controls(rng, n):
    """forced, per-phoneme-scaled and predicted durations side by side, local pitch / energy shifts"""
    frames = np.full(n, -1, np.int32)
    forced = rng.random(n) < 0.3
    frames[forced] = rng.integers(0, 9, forced.sum())
    scale = np.where(rng.random(n) < 0.5, rng.uniform(0.3, 3.0, n), 1.0).astype(np.float32)
    return dict(duration_frames=frames, duration_scale=scale, pitch_shift=rng.uniform(-0.2, 0.2, n).astype(np.float32),
                energy_shift=rng.uniform(-0.2, 0.2, n).astype(np.float32))


# ---- 1. identity ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ln_tail", [1, 0])
def test_identity_encode(env, ln_tail):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    T = g.max_seq_len
    with capi.switches(ZV_LN_TAIL=ln_tail):
        for seed, N in ((11, 200), (12, 1100)):
            ids, puncts, style = _utt(g, seed, N)
            for pr in PROSODIES:
                a = m.encode(ids, puncts, style, T, prosody=pr)
                for how in (dict(return_durations=True), dict(phonemes={}), dict(phonemes=identity_arrays(N))):
                    b = m.encode(ids, puncts, style, T, prosody=pr, **how)
                    for k in a:
                        assert np.array_equal(a[k], b[k]), (N, pr, how, k)
                    assert int(b["durations"].sum()) == a["n_frames"]


@pytest.mark.parametrize("ln_tail", [1, 0])
def test_identity_synthesize_eager_and_graph(env, ln_tail):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    T = g.max_seq_len
    with capi.switches(ZV_LN_TAIL=ln_tail):
        for seed, N in ((21, 200), (22, 1100)):
            ids, puncts, style = _utt(g, seed, N)
            for pr in PROSODIES:
                m.set_graph_mode(False)
                ref, nf = m.synthesize(ids, puncts, style, T, prosody=pr)
                dref = m.encode(ids, puncts, style, T, prosody=pr, return_durations=True)["durations"]
                for graph in (False, True):
                    m.set_graph_mode(graph)
                    for _ in range(2 if graph else 1):       # capture, then replay
                        for how in (dict(), dict(phonemes={}), dict(phonemes=identity_arrays(N))):
                            w, n, d = m.synthesize(ids, puncts, style, T, prosody=pr, return_durations=True, **how)
                            assert n == nf and np.array_equal(w, ref), (N, pr, graph, how)
                            assert np.array_equal(d, dref), (N, pr, graph, how)
                m.set_graph_mode(False)


def _ragged(g, with_scan=True):
    nt = [(200, 1500), (7, 60), (300, 1200), (1, 11)]
    if with_scan:
        nt.append((1100, 1437))
    return [(*_utt(g, 300 + i, N), T) for i, (N, T) in enumerate(nt)]


@pytest.mark.parametrize("ln_tail", [1, 0])
def test_identity_batch_eager_and_graph(env, ln_tail):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    pr = capi.Prosody(**PROSODIES[1])
    with capi.switches(ZV_LN_TAIL=ln_tail):
        for with_scan in (True, False):
            utts = _ragged(g, with_scan)
            m.set_graph_mode(False)
            ref = [(w.copy(), n) for w, n in m.synthesize_batch([u + (pr,) for u in utts])]
            for graph in (False, True):
                m.set_graph_mode(graph)
                for ctl in (None, {}, "ident"):
                    bc = m.prepare_batch([u + (pr, identity_arrays(len(u[0])) if ctl == "ident" else ctl) for u in utts],
                                         durations=True)
                    for _ in range(2 if graph else 1):
                        bc.run()
                        for i, ((w, n), (wr, nr)) in enumerate(zip(bc.results(), ref)):
                            assert n == nr and np.array_equal(w, wr), (with_scan, graph, ctl, i)
                            assert int(bc.durations[i].sum()) == n
            m.set_graph_mode(False)


# ---- 2. teacher-forced decisions --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ln_tail", [1, 0])
@pytest.mark.parametrize("N", [200, 1100])
def test_teacher_forced_decisions(env, ln_tail, N):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    T, nb = g.max_seq_len, g.ve_n_bins
    rng = np.random.default_rng(N + ln_tail)
    ids, puncts, style = _utt(g, 31 + N, N)
    with capi.switches(ZV_LN_TAIL=ln_tail):
        e0 = m.encode(ids, puncts, style, T)
        # all durations forced (a total below T)
        pc = dict(duration_frames=rng.integers(0, T // N + 1, N).astype(np.int32))
        e = m.encode(ids, puncts, style, T, phonemes=pc)
        d = check_decisions(e, e0, T, nb, N, None, pc)
        assert np.array_equal(d, pc["duration_frames"])
        # forced, per-phoneme scaled and predicted, with an utterance scale and shifts
        for pr in PROSODIES:
            pc = mixed_controls(rng, N)
            check_decisions(m.encode(ids, puncts, style, T, prosody=pr, phonemes=pc), e0, T, nb, N, pr, pc)
        # a forced 0: that phoneme's features never appear in hidden
        pc = dict(duration_frames=np.full(N, -1, np.int32))
        zero = [3, N // 2]
        pc["duration_frames"][zero] = 0
        pc["duration_frames"][4] = 5
        e = m.encode(ids, puncts, style, T, phonemes=pc)
        check_decisions(e, e0, T, nb, N, None, pc)
        assert all(e["durations"][i] == 0 for i in zero)
        for i in zero:
            assert not np.any(np.all(e["hidden"][:e["n_frames"]] == e["features"][i], axis=1)), i
        # forced totals above T: durations clipped to T, summing to n_frames = T
        pc = dict(duration_frames=np.full(N, 2 * T // N + 3, np.int32))
        e = m.encode(ids, puncts, style, T, phonemes=pc)
        check_decisions(e, e0, T, nb, N, None, pc)
        assert e["n_frames"] == T and int(e["durations"].sum()) == T and e["durations"][-1] == 0
        # num_phonemes < n: durations forced past it are ignored, shifts still act on all n tokens
        k = N - 10
        e0k = m.encode(ids, puncts, style, T, num_phonemes=k)
        pc = dict(duration_frames=np.full(N, 4, np.int32), pitch_shift=np.full(N, 0.3, np.float32),
                  energy_shift=np.full(N, -0.3, np.float32))
        e = m.encode(ids, puncts, style, T, num_phonemes=k, phonemes=pc)
        check_decisions(e, e0k, T, nb, k, None, pc)
        assert not np.any(e["durations"][k:])
        assert not np.array_equal(e["pitch_bucket"][k:], e0k["pitch_bucket"][k:])


# ---- 3. oracle parity ---------------------------------------------------------------------------------------------------

def test_energy_and_features_match_composed_reference(env):
    from oracle import zvoracle
    from parity_helpers import layer_gate
    m, g, tensors = env
    o = zvoracle.Oracle(tensors)
    N, T = 64, 600
    ids, puncts, style = _utt(g, 41, N)
    rng = np.random.default_rng(41)
    pr = dict(duration_scale=1.2, pitch_scale=0.9, pitch_shift=0.1, energy_scale=0.8, energy_shift=-0.05)
    pc = mixed_controls(rng, N)
    e = m.encode(ids, puncts, style, T, prosody=pr, phonemes=pc)
    pemb = np.asarray(tensors["_pe._var_adapt.pitch_embedding.w"], np.float32).reshape(g.ve_n_bins, g.E)
    eemb = np.asarray(tensors["_pe._var_adapt.energy_embedding.w"], np.float32).reshape(g.ve_n_bins, g.E)
    x_in = np.stack([ids, puncts], axis=1).astype(np.float32)

    def compose():
        x = o.layer(o.LAYER_ENC_EMBED, 0, x_in, g.E)
        for layer in range(g.encoder_layer):
            x = o.layer(o.LAYER_ENC_FFT, layer, x, g.E, heads=g.encoder_head, ksz=g.conv_kernel_size)
        x = (x + style[None, :]).astype(np.float32)
        x = (x + pemb[e["pitch_bucket"]]).astype(np.float32)
        energy = o.layer(o.LAYER_VAR_PRED, 2, x, 0, ksz=(g.vp_kernel_size,))
        feats = (x + eemb[e["energy_bucket"]]).astype(np.float32)
        return energy, feats

    o.set_order(zvoracle.ORDER_GGML_AVX2)
    ref_e, ref_f = compose()
    o.set_order(zvoracle.ORDER_SEQ_F32)
    alt_e, alt_f = compose()
    o.set_order(zvoracle.ORDER_GGML_AVX2)
    # the gate of test_gpu_prosody.py's composed check (absolute bound scaled to the chain, the noise gate decides)
    layer_gate("energy (per-phoneme pitch)", e["energy"], ref_e, alt_e, 1e-3)
    layer_gate("features (per-phoneme)", e["features"], ref_f, alt_f, 1e-3)
    assert np.array_equal(e["pitch_bucket"], restate_buckets(e["pitch"], 0.9, 0.1, pc["pitch_shift"], g.ve_n_bins))
    assert np.array_equal(e["energy_bucket"], restate_buckets(e["energy"], 0.8, -0.05, pc["energy_shift"], g.ve_n_bins))


# ---- 4. batch and graph ---------------------------------------------------------------------------------------------------

def _alone(m, utts, prs, pcs):
    return [m.synthesize(*u, prosody=p, phonemes=c, return_durations=True) for u, p, c in zip(utts, prs, pcs)]


def _same(bc, alone, what):
    for i, ((w, n), d, (wr, nr, dr)) in enumerate(zip(bc.results(), bc.durations, alone)):
        assert n == nr and np.array_equal(w, wr), (what, i)
        assert np.array_equal(d, dr), (what, i, "durations")


@pytest.mark.parametrize("with_scan", [True, False])
def test_batch_matches_standalone_graph_and_replay(env, with_scan):
    m, g, _ = env
    base = _ragged(g, with_scan)
    rng = np.random.default_rng(7 + with_scan)
    prs = [PROSODIES[i % 2] for i in range(len(base))]
    pc1 = [mixed_controls(rng, len(u[0])) if i != 1 else None for i, u in enumerate(base)]
    pc2 = [mixed_controls(rng, len(u[0])) if i != 3 else None for i, u in enumerate(base)]
    m.set_graph_mode(False)
    alone1, alone2 = _alone(m, base, prs, pc1), _alone(m, base, prs, pc2)
    bc = m.prepare_batch([u + (p, c) for u, p, c in zip(base, prs, pc1)])
    bc.run()
    _same(bc, alone1, "eager")
    m.set_graph_mode(True)
    bc.run()
    _same(bc, alone1, "graph capture")
    bc.run()
    _same(bc, alone1, "graph replay")
    for i, c in enumerate(pc2):
        bc.set_phoneme_controls(i, c)
    bc.run()
    _same(bc, alone2, "graph replay with new control values")
    bc.begin(2)
    bc.end(2)
    _same(bc, alone2, "begin / end, graph")
    m.set_graph_mode(False)


def test_batch_split_into_tail_groups(env):
    """16 utterances of up to 1 500 frames: the last vocoder stage runs in utterance groups (G > 1); timings still come back"""
    m, g, _ = env
    rng = np.random.default_rng(99)
    utts = [(*_utt(g, 500 + i, N), T) for i, (N, T) in enumerate([(150 + 13 * i, 1500 - 7 * i) for i in range(16)])]
    prs = [None] * 16
    pcs = [mixed_controls(rng, len(u[0])) if i % 3 else None for i, u in enumerate(utts)]
    alone = _alone(m, utts, prs, pcs)
    for graph in (False, True):
        m.set_graph_mode(graph)
        bc = m.prepare_batch([u + (None, c) for u, c in zip(utts, pcs)])
        for rep in range(2 if graph else 1):
            m.poison(0x3C if rep else 0xFF)              # the lane's blocks hold the previous call's waveforms (zv_debug_poison)
            bc.run()
            _same(bc, alone, f"tail groups, graph={graph}")
    m.set_graph_mode(False)


def test_two_lanes_in_flight_fill_their_own_durations(env):
    m, g, _ = env
    rng = np.random.default_rng(5)
    batches, alones = [], []
    for k in range(4):
        utts = [(*_utt(g, 700 + 10 * k + i, 60 + 40 * i + 7 * k), 900) for i in range(3)]
        pcs = [mixed_controls(rng, len(u[0])) for u in utts]
        alones.append(_alone(m, utts, [None] * 3, pcs))
        batches.append(m.prepare_batch([u + (None, c) for u, c in zip(utts, pcs)]))
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
    m.set_graph_mode(False)


# ---- 5. validation ----------------------------------------------------------------------------------------------------------

def test_validation_rejects_bad_controls_before_any_work(env, ckpt):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    N, T = 40, 400
    ids, puncts, style = _utt(g, 61, N)
    utts = [(*_utt(g, 62 + i, 20 + i), 300) for i in range(3)]
    fmax = min(32768, m.max_frames())
    bad = [("duration_frames", -2), ("duration_frames", fmax + 1), ("duration_scale", 0.0), ("duration_scale", -1.0),
           ("duration_scale", 16.5), ("duration_scale", float("nan")), ("duration_scale", float("inf")),
           ("pitch_shift", float("nan")), ("pitch_shift", float("inf")), ("energy_shift", float("-inf"))]
    good = mixed_controls(np.random.default_rng(1), N)
    for field, val in bad:
        def with_bad(n, at):
            c = identity_arrays(n)
            c[field] = c[field].copy()
            c[field][at] = val
            return c
        for call in (lambda: m.encode(ids, puncts, style, T, phonemes=with_bad(N, 17)),
                     lambda: m.synthesize(ids, puncts, style, T, phonemes=with_bad(N, 17))):
            with pytest.raises(capi.ZvError) as ei:
                call()
            msg = str(ei.value)
            assert ei.value.status == ZV_ERR_ARG and "utterance 0" in msg and f"{field}[17]" in msg, msg
        bc = m.prepare_batch([u + (None, with_bad(len(u[0]), 5) if i == 2 else None) for i, u in enumerate(utts)])
        for call in (bc.run, lambda: bc.begin(1)):
            with pytest.raises(capi.ZvError) as ei:
                call()
            msg = str(ei.value)
            assert ei.value.status == ZV_ERR_ARG and "utterance 2" in msg and f"{field}[5]" in msg, msg
    with pytest.raises(capi.ZvError):
        bc.end(1)                                      # nothing was left in flight
    w, n, d = m.synthesize(ids, puncts, style, T, phonemes=good, return_durations=True)
    e = m.encode(ids, puncts, style, T, phonemes=good)
    path, _, _ = ckpt("medium")
    fresh = capi.Model(path, 0)
    try:
        wf, nf, df = fresh.synthesize(ids, puncts, style, T, phonemes=good, return_durations=True)
        ef = fresh.encode(ids, puncts, style, T, phonemes=good)
    finally:
        fresh.close()
    assert n == nf and np.array_equal(w, wf) and np.array_equal(d, df)
    for k in e:
        assert np.array_equal(e[k], ef[k]), k


# ---- 6. CLI -----------------------------------------------------------------------------------------------------------------

def _cli(args):
    cli = os.path.join(ROOT, "zerovox.cpp_amd", "zerovox")
    r = subprocess.run([cli, "-m", _M["path"]] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r


def test_cli_phoneme_controls_and_alignment(env, tmp_path):
    m, g, _ = env
    N = 40
    ids, puncts, style = _utt(g, 71, N)
    utt = tmp_path / "utt.txt"
    utt.write_text(" ".join(map(str, ids.tolist())) + "\n" + " ".join(map(str, puncts.tolist())) + "\n" +
                   " ".join(repr(float(x)) for x in style.tolist()) + "\n")
    plain, ident = tmp_path / "plain.wav", tmp_path / "ident.wav"
    _cli(["-u", str(utt), "-o", str(plain)])
    pcf = tmp_path / "ident.txt"
    pcf.write_text("-1 1 0 0\n" * N)
    _cli(["-u", str(utt), "-o", str(ident), "--phoneme-controls", str(pcf)])
    assert ident.read_bytes() == plain.read_bytes()
    # forced durations with --trim: sum(frames) * hop samples; the alignment rows = the library's durations
    frames = np.random.default_rng(3).integers(0, 12, N).astype(np.int32)
    pcf = tmp_path / "forced.txt"
    pcf.write_text("".join(f"{f} 1 0.05 -0.05\n" for f in frames))
    out, tsv = tmp_path / "forced.wav", tmp_path / "align.tsv"
    _cli(["-u", str(utt), "-o", str(out), "--trim", "--phoneme-controls", str(pcf), "--alignment", str(tsv)])
    hop = g.hop_size
    assert os.path.getsize(out) == 44 + 2 * int(frames.sum()) * hop
    rows = [line.split("\t") for line in tsv.read_text().splitlines()]
    assert rows[0] == ["index", "phoneme_id", "start_frame", "frames", "start_sample", "samples"]
    got = np.array([[int(v) for v in r] for r in rows[1:]], np.int64)
    _, _, dur = m.synthesize(ids, puncts, style, g.max_seq_len, return_durations=True,
                             phonemes=dict(duration_frames=frames, pitch_shift=np.full(N, 0.05, np.float32),
                                           energy_shift=np.full(N, -0.05, np.float32)))
    start = np.concatenate([[0], np.cumsum(dur)[:-1]])
    assert np.array_equal(got[:, 0], np.arange(N)) and np.array_equal(got[:, 1], ids)
    assert np.array_equal(got[:, 3], dur) and np.array_equal(got[:, 2], start)
    assert np.array_equal(got[:, 4], start * hop) and np.array_equal(got[:, 5], dur.astype(np.int64) * hop)
    assert np.array_equal(dur, frames)
