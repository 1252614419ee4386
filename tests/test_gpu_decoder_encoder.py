"""-m gpu: StyleTTS decoder and FastSpeech2 encoder through the C-ABI vs the CPU oracle.

Noise-aware gates (Appx D): every conv rounds its input activations to f16, which makes
the reference's own semantics chaotic at the 1e-3 level under f32 re-association.  The floor is measured
here, per case, as the distance between two runs of the oracle that differ only in summation order; the
GPU must land within 1.5x of it.  Discrete decisions (durations, buckets) are compared with near-tie
accounting: a flip is accepted only where the oracle's pre-rounding value sits within the noise band of a
rounding boundary."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))


@pytest.fixture(scope="module")
def models(ckpt):
    from zerovox_cpp_amd import capi
    cache = {}

    def get(name):
        if name not in cache:
            path, g, tensors = ckpt(name)
            cache[name] = (capi.Model(path, 0), g, tensors)
        return cache[name]

    yield get
    for m, _, _ in cache.values():
        m.close()


@pytest.mark.parametrize("geom,T", [("tiny", 16), ("tiny", 50), ("small", 64), ("medium", 32)])
def test_decoder_matches_oracle(models, geom, T):
    from zerovox_cpp_amd import synth
    from oracle import zvoracle
    model, g, tensors = models(geom)
    hid = synth.decoder_hidden(g, 11, T)
    _, _, style = synth.encoder_inputs(g, 5, 8)
    mel = model.decode(hid, style)
    orc = zvoracle.Oracle(tensors)
    ref = orc.decoder(hid, style)
    orc.set_order(zvoracle.ORDER_SEQ_F32)
    alt = orc.decoder(hid, style)
    floor_max, floor_rms = float(np.max(np.abs(alt - ref))), _rms(alt - ref)
    err_max, err_rms = float(np.max(np.abs(mel - ref))), _rms(mel - ref)
    print(f"{geom} T={T}: mel err max {err_max:.3e} rms {err_rms:.3e} | floor max {floor_max:.3e} rms {floor_rms:.3e} "
          f"| ratio {err_rms / floor_rms:.2f} | mel rms {_rms(ref):.3f}")
    assert mel.shape == ref.shape and np.isfinite(mel).all()
    assert err_rms <= 1.5 * floor_rms + 1e-6
    assert err_max <= 2.0 * floor_max + 1e-6


def _near_tie_ok(gpu_int, ref_int, pre, scale_fn, band):
    """every disagreement must sit where the oracle's pre-rounding value is within `band` of a .5 boundary"""
    bad = np.nonzero(gpu_int != ref_int)[0]
    for i in bad:
        x = scale_fn(pre[i])
        frac = abs((x + 0.5) - np.round(x + 0.5))
        if frac > band or abs(int(gpu_int[i]) - int(ref_int[i])) > 1:
            return False, i
    return True, len(bad)


@pytest.mark.parametrize("geom,N,T", [("tiny", 8, 40), ("tiny", 13, 64), ("small", 24, 128), ("medium", 32, 160)])
def test_encoder_matches_oracle(models, geom, N, T):
    from zerovox_cpp_amd import synth
    from oracle import zvoracle
    model, g, tensors = models(geom)
    ids, puncts, style = synth.encoder_inputs(g, 5, N)
    e = model.encode(ids, puncts, style, T)
    orc = zvoracle.Oracle(tensors)
    r = orc.encoder(g, ids, puncts, style, T)
    orc.set_order(zvoracle.ORDER_SEQ_F32)
    a = orc.encoder(g, ids, puncts, style, T)
    for k in ("logdur", "pitch", "energy"):
        floor = float(np.max(np.abs(a[k] - r[k])))
        err = float(np.max(np.abs(e[k] - r[k])))
        print(f"{geom} N={N}: {k} err {err:.3e} floor {floor:.3e}")
        assert err <= max(3.0 * floor, 5e-3)
    nb = g.ve_n_bins - 1
    band = 0.05 + 3e-3 * nb
    ok, info = _near_tie_ok(e["pitch_bucket"], r["pitch_bucket"], r["pitch"], lambda p: p * nb, band)
    assert ok, f"pitch bucket flip away from a rounding boundary at token {info}"
    same_pitch = np.array_equal(e["pitch_bucket"], r["pitch_bucket"])
    if same_pitch:
        ok, info = _near_tie_ok(e["energy_bucket"], r["energy_bucket"], r["energy"], lambda p: p * nb, band)
        assert ok, f"energy bucket flip away from a rounding boundary at token {info}"
    # features: rows whose buckets agree must agree to the conv noise level
    rows = np.nonzero((e["pitch_bucket"] == r["pitch_bucket"]) & (e["energy_bucket"] == r["energy_bucket"]))[0]
    ferr = float(np.max(np.abs(e["features"][rows] - r["features"][rows]))) if len(rows) else 0.0
    ffloor = float(np.max(np.abs(a["features"][rows] - r["features"][rows]))) if len(rows) else 0.0
    print(f"{geom} N={N}: features err {ferr:.3e} on {len(rows)}/{N} rows (floor {ffloor:.3e}); frames {e['n_frames']} vs {r['n_frames']}")
    assert ferr <= max(3.0 * ffloor, 5e-3)
    # length regulator: teacher-forced with the GPU's own features + log-durations it must be bit-exact
    hid, nf = orc.length_regulator(e["features"], e["logdur"], T)
    assert nf == e["n_frames"]
    assert np.array_equal(hid, e["hidden"])


def test_bad_ids_are_rejected(models):
    from zerovox_cpp_amd import capi, synth
    model, g, _ = models("tiny")
    ids, puncts, style = synth.encoder_inputs(g, 5, 8)
    ids = ids.copy()
    ids[3] = 155
    with pytest.raises(capi.ZvError) as ei:
        model.encode(ids, puncts, style, 32)
    assert ei.value.status == 5


def test_synthesize_end_to_end(models):
    """throughput path: encoder -> decoder -> vocoder with intermediates kept in HBM; coarse sanity only
    (bit-level end-to-end parity is impossible for any re-ordered implementation)"""
    from zerovox_cpp_amd import synth
    model, g, tensors = models("small")
    N, T = 24, 128
    ids, puncts, style = synth.encoder_inputs(g, 5, N)
    wav, nf = model.synthesize(ids, puncts, style, T)
    e = model.encode(ids, puncts, style, T)
    mel = model.decode(e["hidden"], style)
    wav2 = model.vocode(mel)
    assert nf == e["n_frames"] and wav.shape == (T * g.hop_size,)
    assert np.array_equal(wav, wav2)          # same kernels, same order: the fused path is deterministic


def test_synthesize_batch_equals_per_utterance(models):
    """configs[3]/[4]: mixed-length utterances run on several in-flight lanes; every utterance keeps its own (N, T)
    and must come out bit-identical to a stand-alone zv_synthesize call (no batch padding, deterministic kernels)"""
    from zerovox_cpp_amd import sharding, synth
    model, g, tensors = models("small")
    lens = [min(n, 96) for n in sharding.mixed_length_batch(11, 7)]
    utts = []
    for u, n in enumerate(lens):
        ids, puncts, style = synth.encoder_inputs(g, 100 + u, n)
        utts.append((ids, puncts, style, 64 + 32 * (u % 3)))
    got = model.synthesize_batch(utts)
    for (ids, puncts, style, T), (wav, nf) in zip(utts, got):
        ref, nf_ref = model.synthesize(ids, puncts, style, T)
        assert nf == nf_ref and wav.shape == ref.shape
        assert np.array_equal(wav, ref)
    assert model.synthesize_batch([]) == []


def test_cli_writes_the_same_wav(models, ckpt, tmp_path):
    """the `zerovox` binary (facade + C-ABI, like the reference's main) must write exactly the PCM16 samples that
    zv_synthesize + zv_write_wav produce for the same utterance; --trim cuts at the regulator's frame count"""
    import os
    import subprocess
    from zerovox_cpp_amd import capi, synth
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zerovox.cpp_amd", "zerovox")
    model, g, tensors = models("small")
    path, _, _ = ckpt("small")
    N = 24
    ids, puncts, style = synth.encoder_inputs(g, 5, N)
    utt = tmp_path / "utt.txt"
    utt.write_text(" ".join(map(str, ids.tolist())) + "\n" + " ".join(map(str, puncts.tolist())) + "\n" +
                   " ".join(repr(float(x)) for x in style.tolist()) + "\n")
    out = tmp_path / "cli.wav"
    r = subprocess.run([cli, "-m", path, "-u", str(utt), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    T = g.max_seq_len
    wav, nf = model.synthesize(ids, puncts, style, T)
    ref = tmp_path / "ref.wav"
    capi.write_wav(str(ref), wav, g.sampling_rate)
    assert out.read_bytes() == ref.read_bytes()
    assert f"{T * g.hop_size} samples" in r.stdout
    r = subprocess.run([cli, "-m", path, "-u", str(utt), "-o", str(out), "--trim"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    capi.write_wav(str(ref), wav[: nf * g.hop_size], g.sampling_rate)
    assert out.read_bytes() == ref.read_bytes() and 0 < nf <= T
    # the no-argument form of the reference's main: default model name in the working directory, foo.wav out
    os.symlink(path, tmp_path / "medium-ldec.gguf")
    r = subprocess.run([cli], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0 and (tmp_path / "foo.wav").stat().st_size == 44 + 2 * T * g.hop_size


def test_encoder_edge_cases(models):
    """ragged / extreme inputs the reference's eval handles (src/fs2encoder.cpp:594-656): a single phoneme, a frame
    budget smaller than the predicted durations (truncate at T), one far larger (zero-filled tail), as many phonemes
    as the position table has rows, one more than that (error), T = 0 (error)"""
    from zerovox_cpp_amd import capi, synth
    from oracle import zvoracle
    model, g, tensors = models("tiny")
    orc = zvoracle.Oracle(tensors)
    # one phoneme
    ids, puncts, style = synth.encoder_inputs(g, 9, 1)
    e = model.encode(ids, puncts, style, 16)
    r = orc.encoder(g, ids, puncts, style, 16)
    assert abs(float(e["logdur"][0]) - float(r["logdur"][0])) <= 5e-3
    hid, nf = orc.length_regulator(e["features"], e["logdur"], 16)
    assert nf == e["n_frames"] and np.array_equal(hid, e["hidden"])
    # truncation: 40 phonemes x ~4 frames into 8 frames; and a long zero tail
    ids, puncts, style = synth.encoder_inputs(g, 10, 40)
    for T in (8, 1, 64):
        e = model.encode(ids, puncts, style, T)
        hid, nf = orc.length_regulator(e["features"], e["logdur"], T)
        assert nf == e["n_frames"] and np.array_equal(hid, e["hidden"]) and e["hidden"].shape == (T, g.E)
        if T <= 8:
            assert nf == T                                  # every frame taken
    ids4, puncts4, style4 = synth.encoder_inputs(g, 11, 4)
    e = model.encode(ids4, puncts4, style4, 64)
    assert 0 < e["n_frames"] < 64 and not e["hidden"][e["n_frames"]:].any()
    # the position table has max_seq_len + 1 rows: that many phonemes run, one more is an argument error
    nmax = g.max_seq_len + 1
    ids, puncts, style = synth.encoder_inputs(g, 12, nmax)
    e = model.encode(ids, puncts, style, 32)
    assert np.isfinite(e["features"]).all() and e["features"].shape == (nmax, g.E)
    ids, puncts, style = synth.encoder_inputs(g, 12, nmax + 1)
    for call in (lambda: model.encode(ids, puncts, style, 32), lambda: model.synthesize(ids, puncts, style, 32)):
        with pytest.raises(capi.ZvError) as ei:
            call()                                          # refused before any upload, like a batch's utterance
        assert ei.value.status == 5 and "utterance 0" in str(ei.value) and "sinusoid" in str(ei.value), str(ei.value)
    with pytest.raises(capi.ZvError):
        model.encode(ids4, puncts4, style4, 0)
    # negative and too-large punctuation ids are rejected too
    bad = puncts4.copy()
    bad[0] = 7
    with pytest.raises(capi.ZvError):
        model.encode(ids4, bad, style4, 16)
    bad[0] = -1
    with pytest.raises(capi.ZvError):
        model.encode(ids4, bad, style4, 16)


def test_decoder_edge_cases(models):
    """T = 1 (InstanceNorm over a single frame: variance 0 -> output is the affine offset, src/stylettsdec.cpp:94-98)
    and an all-zero hidden sequence (the regulator's zero tail) stay finite and match the oracle"""
    from zerovox_cpp_amd import synth
    from oracle import zvoracle
    model, g, tensors = models("tiny")
    orc = zvoracle.Oracle(tensors)
    _, _, style = synth.encoder_inputs(g, 5, 4)
    for T, fill in ((1, 1.0), (2, 1.0), (8, 0.0)):
        hid = synth.decoder_hidden(g, 21, T, fill=fill) if fill else np.zeros((T, g.E), np.float32)
        mel = model.decode(hid, style)
        ref = orc.decoder(hid, style)
        assert mel.shape == (T, g.num_mels) and np.isfinite(mel).all()
        err = float(np.max(np.abs(mel - ref)))
        print(f"decoder T={T} fill={fill}: max err {err:.3e}")
        assert err <= 2e-2


def test_reference_style_call_site_runs(models, ckpt, tmp_path):
    """the reference-style C++ caller (stage objects built like src/zerovox.cpp:104-137, eval chain :326-334) must
    produce exactly what the C-ABI path produces for the same utterance"""
    import subprocess
    from test_boundary_cpu import _build_callsite
    from zerovox_cpp_amd import synth
    model, g, _ = models("small")
    path, _, _ = ckpt("small")
    exe = _build_callsite(tmp_path)
    n = 24
    out = tmp_path / "wav.f32"
    r = subprocess.run([exe, path, str(n), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    i = np.arange(n, dtype=np.uint64)
    ids = (1 + (i * 37 + 11) % 154).astype(np.int32)
    puncts = (i % 3).astype(np.int32)
    k = np.arange(g.E, dtype=np.uint64)
    style = (np.float32(0.05) * (((k * np.uint64(2654435761)) % np.uint64(2 ** 32) % np.uint64(201)).astype(np.int64) - 100).astype(np.float32)
             / np.float32(100.0)).astype(np.float32)
    T = g.max_seq_len
    e = model.encode(ids, puncts, style, T)
    wav = model.vocode(model.decode(e["hidden"], style))
    got = np.fromfile(out, np.float32)
    assert got.shape == wav.shape and f"frames {e['n_frames']} " in r.stdout
    assert np.array_equal(got, wav)


def test_medium_geometry_length_sweep(models):
    """decoder and encoder at the full-size channel counts (256-channel chunks, split-K kernel, 1 056-channel concat)
    for lengths around the 32-row tile boundaries; gates as in the golden tests (the reference's own re-association
    noise at this geometry is ~1e-3 rms / 4e-3 max on mel, 5e-4 on log-durations)"""
    from zerovox_cpp_amd import synth
    from oracle import zvoracle
    model, g, tensors = models("medium")
    orc = zvoracle.Oracle(tensors)
    _, _, style = synth.encoder_inputs(g, 5, 4)
    for T in (1, 2, 3, 31, 32, 33, 63, 65):
        # distinct frames: InstanceNorm over a few (nearly) identical frames divides rounding noise by sqrt(eps) and
        # says nothing about the kernels; the gate is relative to the oracle's own re-association noise for the case
        hid = synth.decoder_hidden(g, 60 + T, T, frames_per_phoneme=1, fill=1.0)
        mel = model.decode(hid, style)
        orc.set_order(zvoracle.ORDER_GGML_AVX2)
        ref = orc.decoder(hid, style)
        orc.set_order(zvoracle.ORDER_SEQ_F32)
        alt = orc.decoder(hid, style)
        orc.set_order(zvoracle.ORDER_GGML_AVX2)
        d, floor = mel - ref, alt - ref
        print(f"decoder medium T={T}: rms {_rms(d):.3e} max {np.max(np.abs(d)):.3e} (floor rms {_rms(floor):.3e} max {np.max(np.abs(floor)):.3e})")
        assert np.isfinite(mel).all(), T
        assert _rms(d) <= max(3.0 * _rms(floor), 3e-3) and np.max(np.abs(d)) <= max(3.0 * np.max(np.abs(floor)), 2e-2), T
    for N in (1, 2, 31, 33, 65):
        ids, puncts, sty = synth.encoder_inputs(g, 70 + N, N)
        T = 4 * N + 8
        e = model.encode(ids, puncts, sty, T)
        r = orc.encoder(g, ids, puncts, sty, T)
        ld = float(np.max(np.abs(e["logdur"] - r["logdur"])))
        print(f"encoder medium N={N}: logdur err {ld:.3e}, frames {e['n_frames']} vs {r['n_frames']}")
        assert ld <= 5e-3, N
        hid, nf = orc.length_regulator(e["features"], e["logdur"], T)
        assert nf == e["n_frames"] and np.array_equal(hid, e["hidden"]), N


def test_nothing_depends_on_fresh_arena_contents(models, ckpt, tmp_path):
    """ZV_ARENA_FILL=255 makes every new activation arena start as NaN patterns instead of zeros: the whole chain must
    give the same bits as in this process (no kernel may read activation memory that it or a predecessor did not write)"""
    import subprocess
    import sys
    from zerovox_cpp_amd import synth
    model, g, _ = models("small")
    path, _, _ = ckpt("small")
    ids, puncts, style = synth.encoder_inputs(g, 77, 40)
    wav, nf = model.synthesize(ids, puncts, style, 160)
    out = tmp_path / "poison.npy"
    code = (
        "import sys, numpy as np\n"
        f"sys.path.insert(0, {os.path.dirname(os.path.dirname(os.path.abspath(__file__)))!r})\n"
        "from __graft_entry__ import load_package\nload_package()\n"
        "from zerovox_cpp_amd import capi, synth\n"
        f"m = capi.Model({path!r}, 0)\n"
        "ids, puncts, style = synth.encoder_inputs(synth.SMALL, 77, 40)\n"
        "b = m.synthesize_batch([(ids, puncts, style, 160)] * 5)\n"
        "w, nf = m.synthesize(ids, puncts, style, 160)\n"
        "assert all(np.array_equal(x[0], w) and x[1] == nf for x in b)\n"
        f"np.save({str(out)!r}, w)\n")
    env = dict(os.environ, ZV_ARENA_FILL="255")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal(np.load(out), wav)


def test_batch_regime_kernels_do_not_depend_on_fresh_arena_contents(ckpt, tmp_path):
    """the same poison test with the kernels only batches pick forced on (conv_gemm_kernel reads "finite neighbours" past Cin_p
    against zero weights, the operand passes convert whole capacities, xr16 / the f16 c0 are arena tenants of their own): a NaN
    pattern in a row nobody wrote, times a zero weight, would be a NaN — the NaN-filled run must give the zero-filled run's bits"""
    import subprocess
    import sys
    from zerovox_cpp_amd import capi, synth
    regime = dict(ZV_CONV_GEMM=2, ZV_UP_GEMM=2, ZV_CONV_STREAM=2, ZV_BLOCK64=-3, ZV_DEC_PREPASS=1, ZV_PAIR64_RING=2, ZV_TRIPLE_V2=3,
                  ZV_FUSE256=1, ZV_MERGE_ALWAYS=1)
    path, g, _ = ckpt("medium")
    ids, puncts, style = synth.encoder_inputs(g, 78, 24)
    T = 96
    with capi.switches(**regime):
        m = capi.Model(path, 0)
        wav, nf = m.synthesize(ids, puncts, style, T)
        m.close()
    assert np.isfinite(wav).all()
    out = tmp_path / "poison_batch.npy"
    code = (
        "import sys, numpy as np\n"
        f"sys.path.insert(0, {os.path.dirname(os.path.dirname(os.path.abspath(__file__)))!r})\n"
        "from __graft_entry__ import load_package\nload_package()\n"
        "from zerovox_cpp_amd import capi, synth\n"
        f"m = capi.Model({path!r}, 0)\n"
        "ids, puncts, style = synth.encoder_inputs(synth.MEDIUM, 78, 24)\n"
        f"b = m.synthesize_batch([(ids, puncts, style, {T})] * 3)\n"
        f"w, nf = m.synthesize(ids, puncts, style, {T})\n"
        "assert all(np.array_equal(x[0], w) and x[1] == nf for x in b)\n"
        f"np.save({str(out)!r}, w)\n")
    env = dict(os.environ, ZV_ARENA_FILL="255", **{k: str(v) for k, v in regime.items()})
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal(np.load(out), wav)
