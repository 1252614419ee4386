"""CPU: the "trained" weight family of synth.make_tensors (heavy-tailed f16 conv weights with channel gains spread over octaves,
exact zeros, f16 subnormals and pruned channels; norm gains that include 0 and negatives) has the properties it claims — measured
in f64 on the stored f16 / f32 values, as parity_helpers.ln_rows_reached does for its rows — leaves the "uniform" family's bytes
alone, and keeps the oracle finite at a useful level in all three summation orders."""
import hashlib

import numpy as np
import pytest

# sha256 over (name, dtype, shape, bytes) of every tensor, recorded from make_tensors as it was before it took a `family`
UNIFORM_SHA256 = {("tiny", 1234): "e262c1d28a06f4bddd33077bfe5278bd643e831f4969096d2d852eddb72d272a",
                  ("tiny", 99): "0ca80041a37bc2d6a40826b38cb9a69a4d087cca6a955ba73d893310264ba210"}

F16_MIN_NORMAL, F16_MIN_SUBNORMAL = 2.0 ** -14, 2.0 ** -24
BIG = 4096          # elements from which a tensor's shares are gated (2 % of 4 096: 82 +- 9)


def _sha(tensors):
    s = hashlib.sha256()
    for name, a in tensors:
        s.update(name.encode())
        s.update(str(a.dtype).encode())
        s.update(str(a.shape).encode())
        s.update(a.tobytes())
    return s.hexdigest()


def _rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))


def _is_norm_gain(name):
    return name.endswith(("layer_norm.w", "layer_norm_1.w", "layer_norm_2.w", "norm1.w", "norm2.w", "asr_res.1.w"))


@pytest.fixture(scope="module")
def families():
    from zerovox_cpp_amd import synth
    out = {}
    for gname in ("tiny", "small"):
        g = synth.GEOMETRIES[gname]
        out[gname] = (g, synth.make_tensors(g, 1234), synth.make_tensors(g, 1234, family="trained"))
    return out


@pytest.mark.parametrize("seed", [1234, 99])
def test_uniform_family_keeps_its_bytes(seed):
    """the default family is the generator every fixture under tests/golden/ was made from: not a byte may move"""
    from zerovox_cpp_amd import synth
    assert _sha(synth.make_tensors(synth.TINY, seed)) == UNIFORM_SHA256[("tiny", seed)]
    assert _sha(synth.make_tensors(synth.TINY, seed, family="uniform")) == UNIFORM_SHA256[("tiny", seed)]
    with pytest.raises(ValueError):
        synth.make_tensors(synth.TINY, seed, family="real")


def test_trained_family_is_a_pure_function_of_geometry_seed_and_family(tmp_path):
    from zerovox_cpp_amd import gguf, synth
    a, b = synth.make_tensors(synth.TINY, 7, family="trained"), synth.make_tensors(synth.TINY, 7, family="trained")
    assert _sha(a) == _sha(b) != _sha(synth.make_tensors(synth.TINY, 8, family="trained"))
    path = str(tmp_path / "t.gguf")
    synth.write_checkpoint(path, synth.TINY, 7, family="trained")
    _, t = gguf.read_gguf(path)
    for name, arr in a:                      # the file carries the family's values bit for bit, signed zeros and subnormals included
        assert t[name].dtype == arr.dtype and t[name].tobytes() == arr.tobytes(), name


@pytest.mark.parametrize("gname", ["tiny", "small"])
def test_same_names_shapes_and_dtypes(families, gname):
    g, uni, tr = families[gname]
    assert [(n, a.shape, a.dtype) for n, a in uni] == [(n, a.shape, a.dtype) for n, a in tr]
    for (n, a), (_, b) in zip(uni, tr):
        assert np.isfinite(b.astype(np.float64)).all(), n
        if n == "sinusoid_encoding_table" or n.endswith("linear_layer.b"):       # the predictors' linear bias sets the durations
            assert np.array_equal(a, b), n
        else:
            assert not np.array_equal(a, b), n


@pytest.mark.parametrize("gname", ["tiny", "small"])
def test_conv_weights_have_the_marks_of_trained_ones(families, gname):
    from zerovox_cpp_amd import synth
    g, uni, tr = families[gname]
    uni = dict(uni)
    n_big = n_pruned_out = n_pruned_in = n_chains = 0
    spans, worst_sub = [], 0.0
    for name, w16 in tr:
        if w16.dtype != np.float16:
            continue
        assert w16.ndim == 3, name
        oc, ic, k = w16.shape
        w = w16.astype(np.float64)
        po, pi = synth.trained_pruned(1234, name, oc, ic)
        assert (po >= 0) == (oc >= 32) and (pi >= 0) == (ic >= 32), name
        live = np.ones(w.shape, bool)
        if po >= 0:
            assert not w[po].any(), f"{name}: output channel {po} is not pruned"
            live[po] = False
            n_pruned_out += 1
        if pi >= 0:
            assert not w[:, pi].any(), f"{name}: input channel {pi} is not pruned"
            live[:, pi] = False
            n_pruned_in += 1
        v, bits = w[live], w16[live].view(np.uint16)
        zero = v == 0.0
        sub = (~zero) & (np.abs(v) < F16_MIN_NORMAL)
        assert np.all(np.abs(v[sub]) >= F16_MIN_SUBNORMAL)
        rms = _rms(w)
        assert np.max(np.abs(w)) < 65504.0
        if w.size >= BIG:
            assert np.max(np.abs(w)) >= 4.0 * rms, f"{name}: no element at 4 x the RMS"
            n_big += 1
            zs, ss = float(zero.mean()), float(sub.mean())
            assert 0.01 <= zs <= 0.03, f"{name}: zero share {zs:.4f}"
            # 1 % are set subnormal; the octave gains' own lower tail adds more where the RMS is small (convs2, gain 0.2: 7 %)
            assert 0.005 <= ss <= 0.25, f"{name}: subnormal share {ss:.4f}"
            worst_sub = max(worst_sub, ss)
            neg = (bits[zero] >> 15).astype(bool)
            assert neg.any() and (~neg).any(), f"{name}: zeros of one sign only"
            r = rms / _rms(uni[name])
            assert 0.8 <= r <= 1.15, f"{name}: RMS {r:.3f} x the uniform family's"
        # one output channel is one chain of the conv: the span of the magnitudes it adds up
        for c in range(oc):
            a = np.abs(w[c])
            a = a[a > 0]
            if len(a) >= 256:
                lo, hi = np.percentile(a, [1, 99])
                spans.append(hi / lo)
                n_chains += 1
    print(f"{gname}: {n_big} conv tensors of >= {BIG} elements, {n_pruned_out} pruned output / {n_pruned_in} input channels, "
          f"{n_chains} chains of >= 256 nonzero weights, 99th / 1st percentile span: smallest 2^{np.log2(min(spans)):.2f}, median 2^{np.log2(np.median(spans)):.2f}; largest subnormal share {worst_sub:.4f}")
    assert n_big and n_pruned_out and n_pruned_in and n_chains
    # log2 |w| of a chain is a sum of log2 |normal| (sd 1.6 bits) and the uniform octave gains over +-2 and +-3 (sd 1.15 and 1.73): sd
    # 2.6 bits, so the 1st and 99th percentile lie 2 x 2.33 x 2.6 = 12 bits apart in the typical chain (the subnormals sit at the 1st
    # percentile's edge and pull it further); the narrowest of thousands of chains is a tail draw, gated at the claimed 2^10
    assert np.median(spans) >= 2.0 ** 12
    assert min(spans) >= 2.0 ** 10


@pytest.mark.parametrize("gname", ["tiny", "small"])
def test_norm_gains_biases_statistics_embeddings_and_linears(families, gname):
    g, uni, tr = families[gname]
    uni = dict(uni)
    n_gain = n_lin = 0
    for name, a in tr:
        v = a.astype(np.float64)
        if _is_norm_gain(name):
            n_gain += 1
            assert v.min() >= -1.5 and v.max() <= 3.0, name
            assert (v == 0.0).any() and v.min() < 0.0, f"{name}: no exact 0 / no negative gain"
            assert v.max() - v.min() >= 3.0, name
        elif a.ndim == 1 and name.endswith(".b") and not name.endswith("linear_layer.b"):
            assert np.max(np.abs(v)) <= 1.0, name
            if not name.startswith("_meldec.") and len(v) >= 16:
                assert np.max(np.abs(v)) >= 0.5, name
        elif a.ndim == 2 and a.dtype == np.float32 and name.endswith((".w",)) and "emb" not in name and min(a.shape) >= 32:
            n_lin += 1                       # f32 linear weights: the convs' octave structure over rows (outputs) and columns (inputs)
            rows, cols = np.sqrt(np.mean(v * v, axis=1)), np.sqrt(np.mean(v * v, axis=0))
            assert rows.max() / rows.min() >= 2.0 ** 1.5 and cols.max() / cols.min() >= 2.0 ** 3, name
            assert 0.95 <= _rms(v) / _rms(uni[name]) <= 1.05, name          # the uniform sample's own RMS is within a few per cent of its amplitude / sqrt 3
    assert n_gain and n_lin
    t = dict(tr)
    mean, scale = t["hifigan.mean"].astype(np.float64), t["hifigan.scale"].astype(np.float64)
    assert -7.0 <= mean.min() and mean.max() <= -3.0 and abs(mean.mean() + 5.0) < 1.0
    assert 0.05 <= scale.min() and scale.max() <= 3.0 and scale.max() / scale.min() >= 10.0
    for name in ("_pe._enc.src_word_emb.w", "_pe._enc.punct_embed.w"):
        assert not t[name][0].any() and all(r.any() for r in t[name][1:]), f"{name}: row 0 is the padding row"


# (geometry, weights seed) of every "trained" checkpoint the suite uses at (N, T) = (16, 64): the property tests' own, and the golden
# fixture's (tests/golden/make_golden.py TRAINED_SEED)
UNIFORM_SEED = 1234         # the yardstick: the uniform checkpoints every other test and fixture of the suite runs on
LEVEL_CASES = [("tiny", 1234), ("small", 1234), ("small", 2719)]


@pytest.mark.parametrize("gname,seed", LEVEL_CASES)
def test_oracle_is_finite_and_at_a_useful_level_on_the_trained_family(gname, seed):
    """(N, T) = (16, 64), all three summation orders: nothing non-finite anywhere, the waveform inside tanh's useful range (RMS
    within 2 x the uniform family's at its seed 1234, no sample at +-1); the oracle's own re-association noise printed next to the uniform family's.
    The level moves with the seed (the gains are drawn, not fitted: over seeds 2718 .. 2729 of `small` the ratio runs from 0.31 to
    2.57), so it is asserted for every seed a checkpoint of the suite is made from."""
    from zerovox_cpp_amd import synth
    from oracle import zvoracle
    g = synth.GEOMETRIES[gname]
    N, T = 16, 64
    ids, puncts, style = synth.encoder_inputs(g, 5, N)
    hid = synth.decoder_hidden(g, 11, T)
    level, noise = {}, {}
    for fam in ("uniform", "trained"):
        tensors = dict(synth.make_tensors(g, seed if fam == "trained" else UNIFORM_SEED, family=fam))
        mel = synth.vocoder_mel(g, tensors, 7, T)
        o = zvoracle.Oracle(tensors)
        out = {}
        for order in (zvoracle.ORDER_GGML_AVX2, zvoracle.ORDER_SEQ_F32, zvoracle.ORDER_SEQ_F64):
            o.set_order(order)
            e = o.encoder(g, ids, puncts, style, T)
            out[order] = (o.vocoder(mel), o.decoder(hid, style), e["hidden"], e["features"], e["logdur"])
            for a in out[order]:
                assert np.isfinite(a).all(), (fam, order)
            assert 0 < e["n_frames"] <= T
        ref, alt = out[zvoracle.ORDER_GGML_AVX2], out[zvoracle.ORDER_SEQ_F32]
        level[fam] = (_rms(ref[0]), float(np.max(np.abs(ref[0]))), _rms(ref[1]))
        noise[fam] = (_rms(alt[0] - ref[0]) / _rms(ref[0]), _rms(alt[1] - ref[1]) / _rms(ref[1]))
    for fam in ("uniform", "trained"):
        print(f"{gname} seed {seed if fam == 'trained' else UNIFORM_SEED} {fam:8s}: wav rms {level[fam][0]:.3f} peak {level[fam][1]:.2f}, mel rms {level[fam][2]:.3f}; AVX2 vs "
              f"sequential self-noise: vocoder {noise[fam][0]:.1e}, decoder {noise[fam][1]:.1e}")
    assert 0.5 <= level["trained"][0] / level["uniform"][0] <= 2.0
    assert level["trained"][1] < 0.999


def test_the_fixture_seed_is_the_one_whose_level_is_asserted():
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trained_small_seed2719_T72_N18.npz"))
    assert (str(z["geometry"]), int(z["seed_w"])) in LEVEL_CASES and str(z["family"]) == "trained"
    w = z["wav"].astype(np.float64)
    assert np.isfinite(w).all() and float(np.max(np.abs(w))) < 0.999


def test_vocoder_level_of_the_medium_checkpoint_of_the_gpu_tests():
    """tests/test_gpu_trained_weights.py runs on medium, seed 5150: its vocoder's level on 16 frames, the oracle in the reference's
    order, against the uniform family's (the vocoder alone: it has no norm, so it is the stage whose level the weights set)"""
    from zerovox_cpp_amd import synth
    from oracle import zvoracle
    import test_gpu_mfma_chain as chain
    import test_gpu_trained_weights as gpu
    g = synth.MEDIUM
    level = {}
    for fam in ("uniform", "trained"):
        everything = dict(synth.make_tensors(g, gpu.SEED_W if fam == "trained" else UNIFORM_SEED, family=fam))
        if fam == "trained":        # the chains tests/test_gpu_mfma_chain.py cuts for its family (c) are this checkpoint's tensors
            assert chain.CHAIN_SEED == gpu.SEED_W
            for name, oc, ic, k, gain in chain.CHAIN_TENSORS.values():
                assert everything[name].tobytes() == synth.trained_conv_weight(chain.CHAIN_SEED, name, oc, ic, k, gain).tobytes(), name
        tensors = {n: a for n, a in everything.items() if n.startswith(("_meldec.", "hifigan."))}
        w = zvoracle.Oracle(tensors).vocoder(synth.vocoder_mel(g, tensors, 7, 16))
        assert np.isfinite(w).all()
        level[fam] = (_rms(w), float(np.max(np.abs(w))))
        print(f"medium seed {gpu.SEED_W if fam == 'trained' else UNIFORM_SEED} {fam:8s}: wav rms {level[fam][0]:.3f} peak {level[fam][1]:.2f}")
    assert 0.5 <= level["trained"][0] / level["uniform"][0] <= 2.0
    assert level["trained"][1] < 0.999
