"""-m gpu: ragged batches at the production geometry (synth.MEDIUM) against stand-alone calls, under every kernel regime.

A batch is one launch per kernel over segment tables (one Seg per utterance + one spanning the batch, capi.cpp); the kernels that
only batches select are chosen from the rows a launch covers, Lbatch = t_max x rate x nseg (voc_plan.h, t_max = the longest T
rounded up to 64), with n_cu = 256.  Composition (a) has 18 utterances, T from 1 to 1 500 (t_max = 1 536), so:
  * conv_gemm_kernel for the two deep upsample convs (ZV_UP_GEMM): L = t_max x nseg = 27 648 >= 16 384 input rows;
  * resblock_block64_kernel (64 channels, rate 100): Lbatch / 244 = 11 331 >= 4 x 256;
  * the merged MRF sum (ZV_MERGE_MAXC = 256): Lbatch / 54 = 2 560 (256 ch, rate 5), / 118 = 5 857 (128 ch, rate 25),
    / 246 = 11 239 (64 ch) >= 4 x 256; the fused 256-channel stage (floor(Lbatch / 54) x 3 >= 256) and its 96-row tiles
    (pair<256> MT = 3: ceil(7 680 / 86) x 18 >= 4 x 256); pair64's LDS weight ring (>= 6 x 256 workgroups);
  * the whole-block kernel on 512-row tiles (32 channels) and conv_stream_kernel for the memory-bound upsample convs (batches);
  * the utterance-grouped vocoder tail (capi.cpp: nseg >= 4 and >= 16 MB of waveform: 14 789 frames x 300 x 4 B = 17.7 MB);
  * the decoder's f16 operand pre-pass (t_max x nseg >= 256) and conv_gemm_kernel for its wide convs;
  * the encoder's per-token layers over one dense segment (ZV_LINEAR_MERGED: the extra table entry d_tok[nseg]);
  * attention_mfma_kernel (dk = 264: n_max = round_up(340, 32) = 352 tokens fit its LDS; ceil(352 / 64) x 2 x 18 >= 48
    workgroups) and the one-launch regulator lr_fused16_kernel (longest utterance <= 1 024 tokens).
Ts 1, 2, 11, 54, 55, 255, 256, 257, 1 024 and 1 500 sit next to each other in the tables; at least one utterance fills its T
(n_frames == T), one fills under a quarter of it; N from 1 to 340.  Composition (b) is (a) with one utterance of N = 1 025 and
one of N = max_seq_len + 1 = 1 501: scalar attention_kernel for the whole batch and the scan + gather regulator.  Composition (c)
is (a) with a longest utterance of exactly N = 1 024: the last size of the fused regulator, scalar attention.
Every utterance of every batch must equal its stand-alone zv_synthesize (default regime) bit for bit, waveform and frame count,
in every regime (a fresh model per regime, every call inside the regime's switches, which are read at the call): eager, graph capture + replay, and replay after a
batch of other content with the same capacities (the utterances rotated by one)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (N, T) per utterance
BASE = [(1, 1), (340, 2), (5, 11), (60, 54), (1, 55), (64, 255), (33, 256), (97, 257), (200, 1024), (340, 1500), (20, 1500),
        (300, 1437), (128, 1300), (2, 1499), (250, 1388), (31, 1450), (180, 1320), (65, 1480)]
COMPOSITIONS = {
    "a_short_tokens": BASE,
    "b_long_tokens": [(1025, 1437) if i == 11 else (1501, 1388) if i == 14 else nt for i, nt in enumerate(BASE)],
    "c_1024_tokens": [(1024, 1437) if i == 11 else nt for i, nt in enumerate(BASE)],
}


def _regimes():
    from parity_helpers import VOCODER_REGIMES
    nseg = len(BASE)
    batch_side = [("no_linear_merged", {"ZV_LINEAR_MERGED": 0}),
                  ("conv_gemm_0", {"ZV_CONV_GEMM": 0}), ("conv_gemm_2", {"ZV_CONV_GEMM": 2}),
                  ("up_gemm_0", {"ZV_UP_GEMM": 0}), ("up_gemm_2", {"ZV_UP_GEMM": 2}),
                  ("conv_stream_0", {"ZV_CONV_STREAM": 0}), ("conv_stream_2", {"ZV_CONV_STREAM": 2}),
                  ("block64_0", {"ZV_BLOCK64": 0}), ("block64_-3", {"ZV_BLOCK64": -3}), ("block64_-11", {"ZV_BLOCK64": -11}),
                  ("merge_maxc_64", {"ZV_MERGE_MAXC": 64}), ("merge_maxc_512", {"ZV_MERGE_MAXC": 512}), ("merge_seq_0", {"ZV_MERGE_SEQ": 0}),
                  ("tail_groups_1", {"ZV_TAIL_GROUPS": 1}), ("tail_groups_5", {"ZV_TAIL_GROUPS": 5}),
                  ("tail_groups_nseg", {"ZV_TAIL_GROUPS": nseg}), ("tail_groups_above_nseg", {"ZV_TAIL_GROUPS": 2 * nseg + 3}),
                  ("dec_prepass_0", {"ZV_DEC_PREPASS": 0}), ("dec_prepass_1", {"ZV_DEC_PREPASS": 1}), ("ln_tail_0", {"ZV_LN_TAIL": 0}),
                  ("att_scalar", {"ZV_ATT_SCALAR": 1}), ("att_mfma", {"ZV_ATT_MFMA": 1}),
                  ("conv_nt_1", {"ZV_CONV_NT": 1}), ("conv_nt_2", {"ZV_CONV_NT": 2})]
    return list(VOCODER_REGIMES) + batch_side


def _utterances(g, synth, comp):
    return [(*synth.encoder_inputs(g, 5000 + 37 * i + N, N), T) for i, (N, T) in enumerate(COMPOSITIONS[comp])]


def test_regime_list_covers_the_batch_switches():
    names = [n for n, _ in _regimes()]
    assert len(names) == len(set(names))
    keys = {k for _, sw in _regimes() for k in sw}
    for k in ("ZV_LINEAR_MERGED", "ZV_CONV_GEMM", "ZV_UP_GEMM", "ZV_CONV_STREAM", "ZV_BLOCK64", "ZV_MERGE_MAXC", "ZV_MERGE_SEQ",
              "ZV_TAIL_GROUPS", "ZV_DEC_PREPASS", "ZV_LN_TAIL", "ZV_ATT_SCALAR", "ZV_ATT_MFMA", "ZV_CONV_NT"):
        assert k in keys, k
    # the compositions' arithmetic of the module docstring
    for comp, nt in COMPOSITIONS.items():
        t_max = (max(T for _, T in nt) + 63) // 64 * 64
        assert len(nt) == 18 and t_max * len(nt) >= 16384 and sum(T for _, T in nt) * 300 * 4 >= 16 << 20, comp
        assert {1, 2, 11, 54, 55, 255, 256, 257, 1024, 1500} <= {T for _, T in nt}, comp
    assert max(N for N, _ in COMPOSITIONS["a_short_tokens"]) == 340 and min(N for N, _ in COMPOSITIONS["a_short_tokens"]) == 1
    assert {1025, 1501} <= {N for N, _ in COMPOSITIONS["b_long_tokens"]}
    assert max(N for N, _ in COMPOSITIONS["c_1024_tokens"]) == 1024


@pytest.fixture(scope="module")
def stand_alone(ckpt):
    """the stand-alone references, once, in the default regime"""
    from zerovox_cpp_amd import capi, synth
    path, g, _ = ckpt("medium")
    m = capi.Model(path, 0)
    try:
        refs = {}
        for comp in COMPOSITIONS:
            utts = _utterances(g, synth, comp)
            refs[comp] = (utts, [m.synthesize(*u) for u in utts])
    finally:
        m.close()
    a = refs["a_short_tokens"]
    assert any(nf == u[3] for u, (_, nf) in zip(*a)), "no utterance fills its T"
    assert any(0 < nf < u[3] // 4 for u, (_, nf) in zip(*a)), "no utterance fills well under its T"
    assert refs["b_long_tokens"][1][14][1] == 1388            # N = 1 501 saturates its T
    return path, refs


def _check(got, ref, what):
    assert len(got) == len(ref)
    for i, ((w, nf), (rw, rnf)) in enumerate(zip(got, ref)):
        assert nf == rnf and np.array_equal(w, rw), (what, i)


@pytest.mark.parametrize("regime", _regimes(), ids=lambda r: r[0])
def test_ragged_medium_batches_equal_stand_alone_calls(stand_alone, regime):
    from zerovox_cpp_amd import capi
    path, refs = stand_alone
    name, sw = regime
    with capi.switches(**sw):
        m = capi.Model(path, 0)
        try:
            for comp, (utts, ref) in refs.items():
                _check(m.synthesize_batch(utts), ref, (name, comp, "eager"))
                rot = utts[1:] + utts[:1]                 # other content in every segment, the same capacities
                m.set_graph_mode(True)
                try:
                    _check(m.synthesize_batch(utts), ref, (name, comp, "capture"))
                    _check(m.synthesize_batch(utts), ref, (name, comp, "replay"))
                    _check(m.synthesize_batch(rot), ref[1:] + ref[:1], (name, comp, "other content"))
                    _check(m.synthesize_batch(utts), ref, (name, comp, "replay after other content"))
                finally:
                    m.set_graph_mode(False)
        finally:
            m.close()
