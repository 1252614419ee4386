"""-m gpu: per-utterance prosody controls (include/zerovox_amd.h zv_prosody) at the production geometry (synth.MEDIUM).

The controls steer the variance adaptor's three decisions on the device: the length regulator scales every duration before it
is rounded (lr_fused16_kernel for utterances of at most 1 024 tokens, lr_scan_kernel beyond), and the pitch / energy bucket
steps scale and shift the prediction before it is quantised (the tail of add_layernorm_kernel<true>, or bucket_embed_add_kernel
with ZV_LN_TAIL=0).  Checked here:
  * identity controls (and prosody=None) give the bits of the uncontrolled entry points, eager and graph, both regulator forms,
    both bucket forms;
  * teacher-forced decisions: with controls, the raw taps stay raw and every controlled decision equals a numpy float32
    restatement of the header's arithmetic from the GPU's own raw taps;
  * the reference semantics composed from Oracle.layer (the pitch embedding at the GPU's controlled bucket) against the GPU's
    energy tap and features;
  * batches with a different setting per utterance = stand-alone calls; graph replay after changing only the control values;
  * validation (ZV_ERR_ARG before any work) and the CLI flags."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ZV_ERR_ARG = 5
_M = {}

SETTINGS = [
    dict(duration_scale=0.5),
    dict(duration_scale=1.37, pitch_shift=0.1),
    dict(duration_scale=2.0, pitch_shift=-0.1, energy_scale=0.8),
    dict(pitch_scale=1.3, pitch_shift=-0.05, energy_scale=0.8, energy_shift=0.07),
]


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


# ---- numpy float32 restatement of include/zerovox_amd.h §prosody ---------------------------------------------------------

def _trunc_int(x64):
    """(int)(double) of the kernels: truncation toward zero (values far outside int range saturate; the clamps follow)"""
    return np.trunc(np.clip(x64, -2.0 ** 31, 2.0 ** 31 - 1)).astype(np.int64)


def restate_buckets(pred, scale, shift, nbins):
    p = np.asarray(pred, np.float32)
    p = (p * np.float32(scale)).astype(np.float32)
    p = (p + np.float32(shift)).astype(np.float32)
    p = (p * np.float32(nbins - 1)).astype(np.float32)
    return np.clip(_trunc_int(p.astype(np.float64) + 0.5), 0, nbins - 1)


def restate_durations(logdur, scale, T):
    dur = (np.exp(np.asarray(logdur, np.float32).astype(np.float64)) - 1.0).astype(np.float32)
    dur = (dur * np.float32(scale)).astype(np.float32)
    return np.clip(_trunc_int(dur.astype(np.float64) + 0.5), 0, T)


def restated_hidden(features, d, T):
    """frame f holds the features row of the first token whose cumulative duration exceeds f; zero past the total"""
    cum = np.cumsum(d)
    idx = np.searchsorted(cum, np.arange(T), side="right")
    live = idx < len(d)
    out = np.zeros((T, features.shape[1]), np.float32)
    out[live] = features[idx[live]]
    return out, int(min(int(cum[-1]), T))


def _full(p):
    from zerovox_cpp_amd import capi
    return capi._prosody(p) if p is not None else capi.Prosody()


def check_decisions(e, e0, p, nbins, T):
    """e: encode with controls p, e0: the uncontrolled encode of the same utterance"""
    pr = _full(p)
    for k in ("logdur", "pitch"):                        # predicted before any controlled decision: unchanged
        assert np.array_equal(e[k], e0[k]), k
    pb = restate_buckets(e["pitch"], pr.pitch_scale, pr.pitch_shift, nbins)
    eb = restate_buckets(e["energy"], pr.energy_scale, pr.energy_shift, nbins)
    assert np.array_equal(e["pitch_bucket"], pb), "pitch buckets"
    assert np.array_equal(e["energy_bucket"], eb), "energy buckets"
    d = restate_durations(e["logdur"], pr.duration_scale, T)
    hid, nf = restated_hidden(e["features"], d, T)
    assert e["n_frames"] == nf, (e["n_frames"], nf)
    assert np.array_equal(e["hidden"], hid), "hidden rows"
    assert not np.any(e["hidden"][nf:]), "rows past n_frames"


# ---- 1. identity is free ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ln_tail", [1, 0])
def test_identity_encode_taps(env, ln_tail):
    """prosody=None (zv_encode_taps) and the explicit identity (zv_encode_taps_prosody): every tap, fused and scan regulator"""
    from zerovox_cpp_amd import capi
    m, g, _ = env
    T = g.max_seq_len
    with capi.switches(ZV_LN_TAIL=ln_tail):
        for seed, N in ((11, 64), (12, 1024), (13, 1100)):
            ids, puncts, style = _utt(g, seed, N)
            a = m.encode(ids, puncts, style, T)
            b = m.encode(ids, puncts, style, T, prosody=capi.Prosody())
            c = m.encode(ids, puncts, style, T, prosody=(1.0, 1.0, 0.0, 1.0, 0.0))
            for k in a:
                assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), (N, k)


@pytest.mark.parametrize("ln_tail", [1, 0])
def test_identity_synthesize_eager_and_graph(env, ln_tail):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    T = g.max_seq_len
    with capi.switches(ZV_LN_TAIL=ln_tail):
        for seed, N in ((21, 1024), (22, 1100)):
            ids, puncts, style = _utt(g, seed, N)
            m.set_graph_mode(False)
            ref, nf = m.synthesize(ids, puncts, style, T)
            for graph in (False, True):
                m.set_graph_mode(graph)
                for _ in range(2 if graph else 1):       # capture, then replay
                    w, n = m.synthesize(ids, puncts, style, T, prosody=capi.Prosody())
                    assert n == nf and np.array_equal(w, ref), (N, graph)
                    w, n = m.synthesize(ids, puncts, style, T)
                    assert n == nf and np.array_equal(w, ref), (N, graph)
            m.set_graph_mode(False)


def _ragged(g, with_scan=True):
    nt = [(1024, 1500), (7, 60), (300, 1200), (1, 11)]
    if with_scan:
        nt.append((1100, 1437))
    return [(*_utt(g, 300 + i, N), T) for i, (N, T) in enumerate(nt)]


@pytest.mark.parametrize("ln_tail", [1, 0])
def test_identity_batch_eager_graph_and_lanes(env, ln_tail):
    """a ragged batch with a 1 024-token and a 1 100-token utterance (the scan regulator) and one without the latter (the fused
    regulator): run() and begin() / end(), eager and graph, identity controls = no controls"""
    from zerovox_cpp_amd import capi
    m, g, _ = env
    with capi.switches(ZV_LN_TAIL=ln_tail):
        for with_scan in (True, False):
            utts = _ragged(g, with_scan)
            m.set_graph_mode(False)
            ref = [(w.copy(), n) for w, n in m.synthesize_batch(utts)]
            ident = [u + (capi.Prosody(),) for u in utts]
            for graph in (False, True):
                m.set_graph_mode(graph)
                bc = m.prepare_batch(ident)
                assert bc.prosody is not None
                for _ in range(2 if graph else 1):
                    bc.run()
                    for (w, n), (wr, nr) in zip(bc.results(), ref):
                        assert n == nr and np.array_equal(w, wr), (with_scan, graph, "run")
                    bc.begin(1)
                    bc.end(1)
                    for (w, n), (wr, nr) in zip(bc.results(), ref):
                        assert n == nr and np.array_equal(w, wr), (with_scan, graph, "begin/end")
            m.set_graph_mode(False)


# ---- 2. teacher-forced decisions --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ln_tail", [1, 0])
def test_teacher_forced_decisions(env, ln_tail):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    T = g.max_seq_len
    with capi.switches(ZV_LN_TAIL=ln_tail):
        for seed, N in ((31, 200), (32, 1100)):          # fused regulator, scan regulator
            ids, puncts, style = _utt(g, seed, N)
            e0 = m.encode(ids, puncts, style, T)
            for p in SETTINGS:
                e = m.encode(ids, puncts, style, T, prosody=p)
                check_decisions(e, e0, p, g.ve_n_bins, T)
            # the uncontrolled run is its own restatement under the identity
            check_decisions(e0, e0, None, g.ve_n_bins, T)


# ---- 3. oracle parity ---------------------------------------------------------------------------------------------------

def test_energy_and_features_match_composed_reference(env):
    """the reference semantics composed layer by layer (embedding, FFT blocks, + style, + pitch embedding at the GPU's
    controlled bucket, energy predictor), gated like test_gpu_layers.py's variance predictors"""
    from oracle import zvoracle
    from parity_helpers import layer_gate
    m, g, tensors = env
    o = zvoracle.Oracle(tensors)
    N, T = 64, 600
    ids, puncts, style = _utt(g, 41, N)
    p = dict(duration_scale=1.2, pitch_scale=0.9, pitch_shift=0.1, energy_scale=0.8, energy_shift=-0.05)
    e = m.encode(ids, puncts, style, T, prosody=p)
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
    # test_gpu_layers.py's variance-predictor gate: no worse than 2 x the oracle's own re-association noise on the same input.  Its
    # absolute bound (1e-4) is for ONE layer; composed over the embedding, four FFT blocks and the predictor the oracle's two
    # summation orders already differ by ~3e-4, so the absolute bound is scaled to the chain (1e-3) and the noise gate decides
    layer_gate("energy (controlled pitch)", e["energy"], ref_e, alt_e, 1e-3)
    layer_gate("features (controlled)", e["features"], ref_f, alt_f, 1e-3)
    assert np.array_equal(e["energy_bucket"], restate_buckets(e["energy"], 0.8, -0.05, g.ve_n_bins))


# ---- 4. batch and graph ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_scan", [True, False])
def test_batch_per_utterance_prosody_graph_and_replay(env, with_scan):
    """each utterance with its own setting = its stand-alone zv_synthesize_prosody; graph = eager; replaying the same BatchCall
    after changing only the control values = the eager result for the new values (controls are not baked into the graph)"""
    from zerovox_cpp_amd import capi
    m, g, _ = env
    base = _ragged(g, with_scan)
    p1 = [SETTINGS[i % len(SETTINGS)] for i in range(len(base))]
    p2 = [SETTINGS[(i + 1) % len(SETTINGS)] for i in range(len(base))]
    m.set_graph_mode(False)
    alone1 = [m.synthesize(*u, prosody=p) for u, p in zip(base, p1)]
    alone2 = [m.synthesize(*u, prosody=p) for u, p in zip(base, p2)]
    uncontrolled = [w.copy() for w, _ in m.synthesize_batch(base)]

    def same(bc, alone, what):
        for i, ((w, n), (wr, nr)) in enumerate(zip(bc.results(), alone)):
            assert n == nr and np.array_equal(w, wr), (what, i)

    bc = m.prepare_batch([u + (p,) for u, p in zip(base, p1)])
    bc.run()
    same(bc, alone1, "eager")
    assert any(not np.array_equal(w, u) for (w, _), u in zip(bc.results(), uncontrolled))
    m.set_graph_mode(True)
    bc.run()                                            # capture
    same(bc, alone1, "graph capture")
    bc.run()                                            # replay
    same(bc, alone1, "graph replay")
    for i, p in enumerate(p2):
        bc.set_prosody(i, p)
    bc.run()                                            # replay, new values only
    same(bc, alone2, "graph replay with new control values")
    bc.begin(2)
    bc.end(2)
    same(bc, alone2, "begin / end, graph")
    # an uncontrolled batch on the same capacities does not pick up the controlled graph, and the reverse
    for (w, _), u in zip(m.synthesize_batch(base), uncontrolled):
        assert np.array_equal(w, u)
    bc.run()
    same(bc, alone2, "controlled again after an uncontrolled batch")
    m.set_graph_mode(False)
    bc.begin(3)
    bc.end(3)
    same(bc, alone2, "begin / end, eager")


# ---- 5. the controls act ------------------------------------------------------------------------------------------------

def test_controls_act(env):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    N, T = 48, g.max_seq_len
    ids, puncts, style = _utt(g, 51, N)
    e0 = m.encode(ids, puncts, style, T)
    e2 = m.encode(ids, puncts, style, T, prosody=dict(duration_scale=2.0))
    d = restate_durations(e0["logdur"], 2.0, T)
    assert e2["n_frames"] == min(int(d.sum()), T)
    assert 0 < e0["n_frames"] and 2 * e0["n_frames"] < T
    assert abs(e2["n_frames"] - 2 * e0["n_frames"]) <= N, (e0["n_frames"], e2["n_frames"])
    w0, n0 = m.synthesize(ids, puncts, style, T)
    w2, n2 = m.synthesize(ids, puncts, style, T, prosody=capi.Prosody(duration_scale=2.0))
    assert n0 == e0["n_frames"] and n2 == e2["n_frames"] and not np.array_equal(w0, w2)
    hi = m.encode(ids, puncts, style, T, prosody=dict(pitch_shift=100.0))
    assert np.all(hi["pitch_bucket"] == g.ve_n_bins - 1)
    lo = m.encode(ids, puncts, style, T, prosody=dict(energy_shift=-100.0))
    assert np.all(lo["energy_bucket"] == 0)
    # the raw predictions stay raw (energy: the pitch buckets of `lo` are the uncontrolled ones)
    assert np.array_equal(hi["pitch"], e0["pitch"]) and np.array_equal(lo["energy"], e0["energy"])


# ---- 6. validation ----------------------------------------------------------------------------------------------------------

BAD = [("duration_scale", float("nan")), ("duration_scale", float("inf")), ("duration_scale", 0.0), ("duration_scale", -1.0),
       ("duration_scale", 16.5), ("pitch_scale", float("nan")), ("pitch_shift", float("inf")), ("pitch_shift", float("-inf")),
       ("energy_scale", float("-inf")), ("energy_shift", float("nan"))]


def test_validation_rejects_bad_controls_before_any_work(env, ckpt):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    N, T = 40, 400
    ids, puncts, style = _utt(g, 61, N)
    utts = [(*_utt(g, 62 + i, 20 + i), 300) for i in range(3)]
    good = capi.Prosody(duration_scale=1.5, pitch_shift=0.05)
    for field, val in BAD:
        bad = capi.Prosody(**{field: val})
        for call in (lambda: m.encode(ids, puncts, style, T, prosody=bad),
                     lambda: m.synthesize(ids, puncts, style, T, prosody=bad)):
            with pytest.raises(capi.ZvError) as ei:
                call()
            assert ei.value.status == ZV_ERR_ARG and "utterance 0" in str(ei.value) and field in str(ei.value), str(ei.value)
        bc = m.prepare_batch([u + (good if i != 2 else bad,) for i, u in enumerate(utts)])
        for call in (bc.run, lambda: bc.begin(1)):
            with pytest.raises(capi.ZvError) as ei:
                call()
            assert ei.value.status == ZV_ERR_ARG and "utterance 2" in str(ei.value) and field in str(ei.value), str(ei.value)
    # a null pointer: the message names the entry point that was called
    wav, nf = np.empty(T * g.hop_size, np.float32), ctypes.c_uint32(0)
    st = m.lib.zv_synthesize(m.h, None, capi._ptr(puncts), capi._ptr(style), N, T, capi._ptr(wav), ctypes.byref(nf))
    msg = m.lib.zv_last_error().decode()
    assert st == ZV_ERR_ARG and msg.startswith("zv_synthesize: "), msg
    # nothing was left in flight: lane 1 is idle, and the next valid call gives a fresh model's bits
    with pytest.raises(capi.ZvError):
        bc.end(1)
    w, n = m.synthesize(ids, puncts, style, T, prosody=good)
    e = m.encode(ids, puncts, style, T, prosody=good)
    path, _, _ = ckpt("medium")
    fresh = capi.Model(path, 0)
    try:
        wf, nf = fresh.synthesize(ids, puncts, style, T, prosody=good)
        ef = fresh.encode(ids, puncts, style, T, prosody=good)
    finally:
        fresh.close()
    assert n == nf and np.array_equal(w, wf)
    for k in e:
        assert np.array_equal(e[k], ef[k]), k


# ---- 8. CLI -----------------------------------------------------------------------------------------------------------------

def test_cli_prosody_flags_write_the_same_samples(env, tmp_path):
    from zerovox_cpp_amd import capi
    m, g, _ = env
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zerovox.cpp_amd", "zerovox")
    N = 40
    ids, puncts, style = _utt(g, 71, N)
    utt = tmp_path / "utt.txt"
    utt.write_text(" ".join(map(str, ids.tolist())) + "\n" + " ".join(map(str, puncts.tolist())) + "\n" +
                   " ".join(repr(float(x)) for x in style.tolist()) + "\n")
    out = tmp_path / "cli.wav"
    r = subprocess.run([cli, "-m", _M["path"], "-u", str(utt), "-o", str(out), "--duration-scale", "1.5", "--pitch-shift", "0.05"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    T = g.max_seq_len
    wav, nf = m.synthesize(ids, puncts, style, T, prosody=capi.Prosody(duration_scale=1.5, pitch_shift=0.05))
    ref = tmp_path / "ref.wav"
    capi.write_wav(str(ref), wav, g.sampling_rate)
    assert out.read_bytes() == ref.read_bytes()
    plain, _ = m.synthesize(ids, puncts, style, T)
    assert not np.array_equal(plain, wav)
