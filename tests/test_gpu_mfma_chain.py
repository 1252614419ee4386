"""GPU: the matrix-core accumulation chain at instruction level (zv_debug_mfma_chain: one wave, out = c0 + a[32][K] . b[K][32]).

Every "same bits" promise of the product (batch == stand-alone, zv_vocode_stream == zv_vocode, run-shortening on == off, all
VOCODER_REGIMES) mixes kernels on v_mfma_f32_32x32x16_f16 (form 0) with kernels on v_mfma_f32_16x16x32_f16 (form 1) and rests on
the two giving the same bits for one k-ordered chain; the f32 linear layers and the attention rest on v_mfma_f32_32x32x2_f32
(form 2) being a k-ordered fmaf chain.  scripts/mfma_shape_bits.hip measured the first once, by hand, on operands of one magnitude
per chain.  Here both are asserted on chains whose products span the f16 range, cancel, are subnormal or meet an accumulator out
of scale, and the accuracy of forms 0 / 1 is gated against the reference's own accumulation, a sequential f32 fmaf chain.

The table of measured figures (profiles/mfma_chain.txt) is printed, and written to $ZV_MFMA_CHAIN_TABLE when that is set."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K_ALL = (32, 96, 1152, 3360)        # one and three instructions of form 1; a 3-tap 384-channel and a 3-tap 1 120-channel chain
FINITE = ("a", "b", "c", "d", "e", "f")
FMAF = ("a", "b", "d", "e")         # the families form 2 runs (as f32 operands with full mantissas)
NAMES = {"a": "script's uniform operands", "b": "exponent sweep", "c": "trained-family weights x sparse activations",
         "d": "cancelling pair", "e": "accumulator out of scale", "f": "signed zeros", "g": "non-finite"}
# family (c): (tensor, oc, ic, k, gain) as synth.make_tensors builds it for the medium geometry, per chain depth K: a 7-tap and a
# 3-tap conv of the last vocoder stage (K = 32 cut from 224, K = 96 whole), the 528-channel and the 1 120-channel 3-tap decoder
# convs (K = 1 152 = 384 channels x 3 taps cut from 1 584, K = 3 360 whole).  tests/test_trained_weights_cpu.py checks that these
# are the checkpoint's tensors bit for bit
CHAIN_SEED = 5150
CHAIN_TENSORS = {32: ("_meldec.blocks.10.convs1.0.1.w", 32, 32, 7, 1.0), 96: ("_meldec.blocks.9.convs1.0.1.w", 32, 32, 3, 1.0),
                 1152: ("_mel_decoder.decode.3.conv1.w", 528, 528, 3, 1.4), 3360: ("_mel_decoder.decode.0.conv1.w", 1056, 1120, 3, 1.4)}
ACC_MARGIN = 4.0     # x the fmaf chain's own worst error: truncating instead of rounding doubles it, aligning a group of
                     # products to its largest doubles it again


def _sweep(rng, shape, lo=-24, hi=15):
    """sign x 2^e x (1 + u), e uniform over the whole f16 range (e < -14: f16 subnormals), clipped to the largest finite f16"""
    e = rng.integers(lo, hi + 1, shape)
    v = np.where(rng.random(shape) < 0.5, -1.0, 1.0) * np.exp2(e.astype(np.float64)) * (1.0 + rng.random(shape))
    return np.clip(v, -65504.0, 65504.0)


def _cases(K):
    """[(family, label, a [32][K] f64, b [K][32] f64, c0 [32][32] f32)], every case seeded"""
    import parity_helpers as ph
    from zerovox_cpp_amd import synth
    out = []
    # (a) scripts/mfma_shape_bits.hip: integers in +-1000 over 1000, A at three scales, C0 a hundred times larger
    for i, scale in enumerate((100.0, 1e-3, 1.0)):
        rng = np.random.default_rng(1000 + 10 * i + K)
        a = rng.integers(-1000, 1001, (32, K)) / 1000.0 * scale
        b = rng.integers(-1000, 1001, (K, 32)) / 1000.0
        c0 = (rng.integers(-1000, 1001, (32, 32)) / 10.0 * scale).astype(np.float32)
        out.append(("a", f"scale {scale:g}", a, b, c0))
    # (b) exponents uniform over the f16 range in both operands and in the accumulator: products from 2^-48 to 2^32 in one chain
    for i in range(2):
        rng = np.random.default_rng(2000 + 10 * i + K)
        out.append(("b", f"seed {i}", _sweep(rng, (32, K)), _sweep(rng, (K, 32)), _sweep(rng, (32, 32)).astype(np.float32)))
    # (c) b: the first 32 output channels of a conv tensor of the medium "trained" checkpoint of tests/test_gpu_trained_weights.py,
    # cut to K weights (CHAIN_TENSORS); a: heavy-tailed activations, 90 % and 50 % zeros, each case with its own seeds
    name, oc, ic, k, gain = CHAIN_TENSORS[K]
    w = synth.trained_conv_weight(CHAIN_SEED, name, oc, ic, k, gain)[:32].reshape(32, ic * k)[:, :K].astype(np.float64)
    for i, zf in enumerate((0.9, 0.5)):
        rng = np.random.default_rng(3000 + 100 * i + K)
        out.append(("c", f"{name} zeros {zf:g}", ph.sparse(3050 + 100 * i + K, 32, K, zero_frac=zf)[0].astype(np.float64), w.T.copy(),
                    (0.1 * rng.standard_normal((32, 32))).astype(np.float32)))
    # (d) +x and -x at k1 < k2 among products 2^-12 .. 2^-20 as large: what survives depends on the order and the width of
    # whatever the matrix core adds up inside one instruction
    base = 32 * ((K // 32) // 2)
    places = [("inside one group of 8", 1, 6), ("across two groups of 8", 3, 12), ("across the 16-k boundary", 12, 19)]
    if base + 35 < K:
        places.append(("across the 32-k boundary", 28, 35))
    for i, (label, d1, d2) in enumerate(places):
        rng = np.random.default_rng(4000 + 10 * i + K)
        x = np.exp2(rng.uniform(0, 6, (32, 1))) * (1.0 + rng.random((32, 1)))
        small = np.exp2(-rng.integers(12, 21, (32, K)).astype(np.float64)) * (1.0 + rng.random((32, K)))
        a = x * small * np.where(rng.random((32, K)) < 0.5, -1.0, 1.0)
        b = rng.uniform(-1, 1, (K, 32))
        a[:, base + d1], a[:, base + d2] = x[:, 0], -x[:, 0]
        b[base + d1] = b[base + d2] = rng.uniform(0.5, 1.0, 32) * np.where(rng.random(32) < 0.5, -1.0, 1.0)
        out.append(("d", label, a, b, np.zeros((32, 32), np.float32)))
    # (e) the accumulator 2^20 larger / smaller than the products
    for i, s in enumerate((20, -20)):
        rng = np.random.default_rng(5000 + 10 * i + K)
        c0 = (np.exp2(s) * rng.uniform(0.5, 1.0, (32, 32)) * np.where(rng.random((32, 32)) < 0.5, -1.0, 1.0)).astype(np.float32)
        out.append(("e", f"c0 x 2^{s:+d}", rng.uniform(-1, 1, (32, K)), rng.uniform(-1, 1, (K, 32)), c0))
    # (f) every product a zero, of both signs; c0 = +0 / -0
    for i, c in enumerate((0.0, -0.0)):
        rng = np.random.default_rng(6000 + 10 * i + K)
        a = np.where(rng.random((32, K)) < 0.5, -0.0, 0.0)
        out.append(("f", f"c0 {'-0' if i else '+0'}, a zero", a, rng.uniform(-1, 1, (K, 32)), np.full((32, 32), c, np.float32)))
        b = np.where(rng.random((K, 32)) < 0.5, -0.0, 0.0)
        out.append(("f", f"c0 {'-0' if i else '+0'}, b zero", rng.uniform(-1, 1, (32, K)), b, np.full((32, 32), c, np.float32)))
    # (g) the only non-finite inputs: one +inf, one NaN, inf x 0 — one element of a each
    for i, label in enumerate(("one +inf", "one NaN", "inf x 0")):
        rng = np.random.default_rng(7000 + 10 * i + K)
        a, b = rng.uniform(-1, 1, (32, K)), rng.uniform(-1, 1, (K, 32))
        r, kk = int(rng.integers(32)), int(rng.integers(K))
        a[r, kk] = np.nan if i == 1 else np.inf
        if i == 2:
            b[kk] = 0.0
        out.append(("g", label, a, b, rng.uniform(-1, 1, (32, 32)).astype(np.float32)))
    return out


def _fma32(a, b, c):
    """fmaf on arrays, exactly: round_f32(a * b + c) with one rounding.  a * b is exact in f64 (two 24-bit significands); the sum is
    formed in f64 with its rounding error (TwoSum), rounded TO ODD, and only then to f32 — f64 keeps 29 bits more than f32, so
    the second rounding sees exactly what a single one would"""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.uint64) & np.uint64(1)) == 0
    fix = (err != 0.0) & even & np.isfinite(s)
    s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def _fmaf_chains(a, b, c0):
    """out[n][i][j] = fmaf chain over k = 0 .. K - 1 from c0, operands f32: a [n][32][K], b [n][K][32], c0 [n][32][32]"""
    acc = c0.astype(np.float32).copy()
    for k in range(a.shape[2]):
        acc = _fma32(a[:, :, k, None], b[:, k, None, :], acc)
    return acc


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def test_fma32_is_a_single_rounding():
    """the host model itself against exact rational arithmetic, on operands that make f64 round the sum (it needs no GPU; it
    stands here because only the tests below use the model)"""
    from fractions import Fraction
    rng = np.random.default_rng(5)
    a = _sweep(rng, 4000, -40, 40).astype(np.float32)
    b = _sweep(rng, 4000, -40, 40).astype(np.float32)
    c = (a.astype(np.float64) * b * -(1.0 + np.exp2(-rng.integers(20, 60, 4000).astype(np.float64)))).astype(np.float32)
    c[::3] = _sweep(rng, len(c[::3]), -60, 60).astype(np.float32)
    # halfway cases of the final rounding that f64 rounds first: c = 1, a * b = 2^-24 + 2^-80
    a[:2], b[:2], c[:2] = [2.0 ** -12, -2.0 ** -12], [2.0 ** -12 * (1 + 2.0 ** -23), 2.0 ** -12 * (1 + 2.0 ** -23)], [1.0, -1.0]
    got = _fma32(a, b, c)
    for i in range(len(a)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.float32(exact)                                   # Fraction -> float rounds once to f64; refine exactly below
        cands = [lo, np.nextafter(lo, np.float32(np.inf)), np.nextafter(lo, np.float32(-np.inf))]
        best = min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), int(np.float32(v).view(np.uint32)) & 1))
        assert got[i] == best, (i, float(a[i]), float(b[i]), float(c[i]))


@pytest.fixture(scope="module")
def model(ckpt):
    from zerovox_cpp_amd import capi
    m = capi.Model(ckpt("tiny")[0], 0)
    yield m
    m.close()


def test_bad_arguments_are_errors(model):
    """K no multiple of 32, K above 4 096, an unknown form: ZV_ERR_ARG"""
    from zerovox_cpp_amd import capi
    c0 = np.zeros((32, 32), np.float32)
    for form, K in ((0, 48), (1, 48), (2, 48), (0, 4128), (2, 4128), (3, 32)):
        dt = np.float32 if form == 2 else np.float16
        with pytest.raises(capi.ZvError) as ei:
            model.debug_mfma_chain(form, np.zeros((32, K), dt), np.zeros((K, 32), dt), c0)
        assert ei.value.status == 5, (form, K, str(ei.value))
    out = model.debug_mfma_chain(0, np.zeros((32, 4096), np.float16), np.zeros((4096, 32), np.float16), c0)      # the largest K
    assert not out.any()


@pytest.fixture(scope="module")
def table(model):
    """every case at every K through the three forms and the host models, once: {(family, K): [case dict]}"""
    m = model
    res = {}
    for K in K_ALL:
        cases = _cases(K)
        a16 = np.stack([c[2] for c in cases]).astype(np.float16)
        b16 = np.stack([c[3] for c in cases]).astype(np.float16)
        a32 = np.stack([c[2] for c in cases]).astype(np.float32)
        b32 = np.stack([c[3] for c in cases]).astype(np.float32)
        c0 = np.stack([c[4] for c in cases])
        with np.errstate(invalid="ignore", over="ignore"):
            seq16 = _fmaf_chains(a16.astype(np.float32), b16.astype(np.float32), c0)     # the yardstick of forms 0 / 1
            seq32 = _fmaf_chains(a32, b32, c0)                                           # what form 2 must be
        for n, (fam, label, _, _, _) in enumerate(cases):
            r = dict(label=label, K=K, a16=a16[n], b16=b16[n], c0=c0[n], seq16=seq16[n], seq32=seq32[n],
                     f0=m.debug_mfma_chain(m.MFMA_32X32X16_F16, a16[n], b16[n], c0[n]),
                     f1=m.debug_mfma_chain(m.MFMA_16X16X32_F16, a16[n], b16[n], c0[n]))
            if fam in FMAF:
                r["f2"] = m.debug_mfma_chain(m.MFMA_32X32X2_F32, a32[n], b32[n], c0[n])
            res.setdefault((fam, K), []).append(r)
    lines = ["family K cases elements | forms 0 vs 1 differ | form 2 vs fmaf chain differ | worst err / sum|a b|: form 0, form 1, fmaf chain"]
    for fam in FINITE:
        for K in K_ALL:
            rs = res[(fam, K)]
            d01 = sum(int((_bits(r["f0"]) != _bits(r["f1"])).sum()) for r in rs)
            d2 = sum(int((_bits(r["f2"]) != _bits(r["seq32"])).sum()) for r in rs) if fam in FMAF else None
            q = _ratios(rs)
            lines.append(f"({fam}) {NAMES[fam]:44s} K={K:5d} {len(rs)} {1024 * len(rs):5d} | {d01:5d} | "
                         f"{'-' if d2 is None else d2:>5} | " + (f"{q[0]:.3e} {q[1]:.3e} {q[2]:.3e}" if q else "- (every product is zero)"))
    n01 = sum(1024 * len(res[(fam, K)]) for fam in FINITE for K in K_ALL)
    n2 = sum(1024 * len(res[(fam, K)]) for fam in FMAF for K in K_ALL)
    lines.append(f"total: forms 0 vs 1 on {n01} elements of the finite families, form 2 vs the fmaf chain on {n2}")
    text = "\n".join(lines)
    print("\n" + text)
    if os.environ.get("ZV_MFMA_CHAIN_TABLE"):
        with open(os.environ["ZV_MFMA_CHAIN_TABLE"], "w") as f:
            f.write(text + "\n")
    return res


def _ratios(rs):
    """worst |x - exact| / sum_k |a_k b_k| over the elements of the cases rs for x = form 0, form 1 and the f32 fmaf chain; exact =
    the f64 dot product of the same f16 operands"""
    worst = np.zeros(3)
    seen = False
    for r in rs:
        a, b = r["a16"].astype(np.float64), r["b16"].astype(np.float64)
        exact = r["c0"].astype(np.float64) + a @ b
        den = np.abs(a) @ np.abs(b)
        ok = den > 0
        if not ok.any():
            continue
        seen = True
        for i, key in enumerate(("f0", "f1", "seq16")):
            worst[i] = max(worst[i], float(np.max(np.abs(r[key].astype(np.float64) - exact)[ok] / den[ok])))
    return tuple(worst) if seen else None


@pytest.mark.parametrize("family", FINITE)
def test_the_two_f16_shapes_give_the_same_bits(table, family):
    """v_mfma_f32_32x32x16_f16 and v_mfma_f32_16x16x32_f16 on one k-ordered chain: the same 32 bits, the signs of zeros included"""
    bad = []
    for K in K_ALL:
        for r in table[(family, K)]:
            ne = np.flatnonzero(_bits(r["f0"]).ravel() != _bits(r["f1"]).ravel())
            if len(ne):
                i = int(ne[0])
                bad.append(f"K={K} [{r['label']}]: {len(ne)} of 1024 differ, first at [{i // 32}][{i % 32}]: "
                           f"{r['f0'].ravel()[i]!r} vs {r['f1'].ravel()[i]!r}")
    assert not bad, f"family ({family}) {NAMES[family]}:\n" + "\n".join(bad)


def test_the_two_f16_shapes_are_non_finite_at_the_same_elements(table):
    for K in K_ALL:
        for r in table[("g", K)]:
            n0, n1 = ~np.isfinite(r["f0"]), ~np.isfinite(r["f1"])
            print(f"(g) K={K} [{r['label']}]: non-finite {int(n0.sum())} / {int(n1.sum())}, NaN {int(np.isnan(r['f0']).sum())} / "
                  f"{int(np.isnan(r['f1']).sum())}")
            assert n0.any() and np.array_equal(n0, n1), f"K={K} [{r['label']}]: {int((n0 != n1).sum())} elements differ"


@pytest.mark.parametrize("family", FMAF)
def test_the_f32_shape_is_a_k_ordered_fmaf_chain(table, family):
    """v_mfma_f32_32x32x2_f32 against fmaf(a_k, b_k, acc) over k = 0, 1, ... on the host, bit for bit (the property
    linear_mfma_kernel and the attention kernels state), on f32 operands with full significands"""
    bad = []
    for K in K_ALL:
        for r in table[(family, K)]:
            ne = np.flatnonzero(_bits(r["f2"]).ravel() != _bits(r["seq32"]).ravel())
            if len(ne):
                i = int(ne[0])
                bad.append(f"K={K} [{r['label']}]: {len(ne)} of 1024 differ, first at [{i // 32}][{i % 32}]: "
                           f"{r['f2'].ravel()[i]!r} vs {r['seq32'].ravel()[i]!r}")
    assert not bad, f"family ({family}) {NAMES[family]}:\n" + "\n".join(bad)


@pytest.mark.parametrize("family", [f for f in FINITE if f != "f"])
def test_the_f16_shapes_are_as_accurate_as_the_fmaf_chain(table, family):
    """err / sum |a_k b_k| against the f64 dot product, worst element of the family at each K: at most ACC_MARGIN x the same figure
    of a sequential f32 fmaf chain on the same operands (the reference's accumulation)"""
    for K in K_ALL:
        q0, q1, qs = _ratios(table[(family, K)])
        print(f"({family}) K={K}: form 0 {q0:.3e}, form 1 {q1:.3e}, fmaf chain {qs:.3e}")
        assert q0 <= ACC_MARGIN * qs and q1 <= ACC_MARGIN * qs, f"family ({family}) {NAMES[family]}, K={K}"
