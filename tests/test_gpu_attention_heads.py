"""-m gpu: the encoder at `encoder.head` = 1, 3, 4, 8 (synth.MEDIUM_H*: MEDIUM with only the head count changed; every other
test runs H = 2).  E = 528, so the head dim dk = E / H is 528, 176, 132 or 66, and launch_attention (encoder_kernels.hip; the rule:
stage_plan.h att_plan, restated once in parity_helpers.mfma_max_tokens) picks:
  * attention_mfma_kernel only for dk % 4 == 0 and dk <= 2 x ATT_NS_MAX = 288 (H = 3, 4) while its LDS,
    (64 (dk | 1) + 1 + 64 round_up(n, 32)) x 4 bytes, fits ATT_LDS_MAX = 156 KiB: n <= 416 tokens at dk = 176, n <= 480 at dk = 132
    (and by default only with >= 48 workgroups, i.e. for batches; ZV_ATT_MFMA = 1 forces it where it is legal).  dk = 176 is
    not a multiple of 64; dk = 132 gives ns = dk / 2 = 66 MFMA steps, the loop's last group of two;
  * attention_kernel (scalar) otherwise: dk = 528 > 288 (H = 1), dk = 66 with dk % 4 != 0 (H = 8), and n past the LDS limit.
Gates: LAYER_ENC_MHA against the oracle's layer at heads = H with N on both sides of the LDS limit, under ZV_ATT_SCALAR = 1 and
ZV_ATT_MFMA = 1, the two bit-equal; the whole encoder against the reference's outputs in tests/golden/medium_heads.npz (37 / 300 /
450 tokens) with parity_helpers.encoder_decisions_vs_reference, every tap bit-equal between the two attention kernels; a batch of
the three utterances (>= 48 workgroups: the matrix-core kernel by itself where legal) equal to the stand-alone calls."""
import os

import numpy as np
import pytest

from parity_helpers import mfma_max_tokens as _mfma_max_tokens

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HEADS = {"medium_h1": 1, "medium_h3": 3, "medium_h4": 4, "medium_h8": 8}


def test_mfma_token_limits_at_these_head_dims():
    assert _mfma_max_tokens(264) == 352 and _mfma_max_tokens(176) == 416 and _mfma_max_tokens(132) == 480
    assert _mfma_max_tokens(528) == 0 and _mfma_max_tokens(66) == 0


@pytest.mark.parametrize("geom", list(HEADS))
def test_attention_sublayer_at_other_head_counts(ckpt, geom):
    from zerovox_cpp_amd import capi
    from oracle import zvoracle
    from parity_helpers import layer_gate, oracle_pair
    path, g, tensors = ckpt(geom)
    H = HEADS[geom]
    assert g.encoder_head == H
    dk = g.E // H
    lim = _mfma_max_tokens(dk)
    Ns = (1, 33, 96) + ((lim, lim + 1) if lim else (340, 400))
    m = capi.Model(path, 0)
    try:
        o = zvoracle.Oracle(tensors)
        for layer in (0, 3):
            for N in Ns:
                x = np.random.default_rng(700 + 10 * layer + N).standard_normal((N, g.E)).astype(np.float32)
                ref, alt = oracle_pair(o, "layer", o.LAYER_ENC_MHA, layer, x, g.E, heads=H, ksz=g.conv_kernel_size)
                outs = {}
                for sw in ({"ZV_ATT_SCALAR": 1}, {"ZV_ATT_MFMA": 1}):
                    with capi.switches(**sw):
                        outs[list(sw)[0]] = got = m.debug_layer(m.LAYER_ENC_MHA, layer, x, g.E)
                    layer_gate(f"H={H} dk={dk} layer {layer} N={N} {list(sw)[0]}", got, ref, alt, 1e-4)
                assert np.array_equal(outs["ZV_ATT_SCALAR"], outs["ZV_ATT_MFMA"]), (H, layer, N)
    finally:
        m.close()


@pytest.mark.parametrize("geom", list(HEADS))
def test_encoder_at_other_head_counts_vs_reference_golden(ckpt, geom):
    from zerovox_cpp_amd import capi, synth
    from parity_helpers import encoder_decisions_vs_reference
    z = np.load(os.path.join(GOLD, "medium_heads.npz"))
    path, g, tensors = ckpt(geom, int(z["seed_w"]))
    m = capi.Model(path, 0)
    try:
        utts = []
        for N, T in z["cases"]:
            N, T = int(N), int(T)
            k = "%s_N%d_" % (geom, N)
            zc = {n[len(k):]: z[n] for n in z.files if n.startswith(k)}
            ids, puncts, style = synth.encoder_inputs(g, int(z["seed_enc"]), N)
            e = m.encode(ids, puncts, style, T)
            print(f"{geom} N={N} T={T}")
            encoder_decisions_vs_reference(e, zc, g.ve_n_bins - 1, T)
            assert not e["hidden"][e["n_frames"]:].any()
            taps = {}
            for sw in ({"ZV_ATT_SCALAR": 1}, {"ZV_ATT_MFMA": 1}):
                with capi.switches(**sw):
                    taps[list(sw)[0]] = m.encode(ids, puncts, style, T)
            for name, v in e.items():
                assert np.array_equal(np.asarray(taps["ZV_ATT_SCALAR"][name]), np.asarray(v)), (N, name)
                assert np.array_equal(np.asarray(taps["ZV_ATT_MFMA"][name]), np.asarray(v)), (N, name)
            utts.append((ids, puncts, style, T))
        ref = [m.synthesize(*u) for u in utts]
        for (w, nf), (rw, rnf) in zip(m.synthesize_batch(utts), ref):
            assert nf == rnf and np.array_equal(w, rw), geom
    finally:
        m.close()
