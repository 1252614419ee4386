"""-m gpu: the vocoder and the decoder at the production geometry (synth.MEDIUM: 512 vocoder channels, E = 528) on lengths
that put each kernel's row count on both sides of its tile heights, every length against the CPU oracle.

Vocoder stages: 256 / 128 / 64 / 32 channels at 5 / 25 / 100 / 300 rows per mel frame (rows = T x rate).  Output rows per
tile (TM = rows a workgroup stores, from the launch_* functions of conv1d_mfma.hip; K = 3 / 7 / 11 taps, Kmax = 11 sizes the grid):
  * resblock_pair_kernel<256>: BM = 32 MT (4 / 4) rows less K - 1 halo rows -> 62 / 58 / 54 (MT = 2, ZV_FUSE256 or
    T >= 929 by itself: enough_rows of csrc/voc_plan.h, both sides checked on the host by tests/test_voc_plan_cpu.py) and
    94 / 90 / 86 (the batches' 96-row tiles, MT = 3);
  * resblock_pair_kernel<128>: 62 / 58 / 54 (MT = 2) and 126 / 122 / 118 (MT = 4; the merged MRF sum's 118-row tile);
  * resblock_pair_kernel<64>: 126 / 122 / 118; resblock_pair64_kernel (LDS weight ring): 257 - K = 254 / 250 / 246 (the merged
    sum's 246-row tile); resblock_block64_kernel (two dilation pairs, dil 1 and 3): 256 - 2 h (1 + 3 + 2) = 244 at K = 3;
  * resblock_triple_kernel / resblock_block32 (all three pairs, dil 1 3 5): R - 24 h, h = (K - 1) / 2 -> 232 / 184 / 136
    (R = 256) and 488 / 440 / 392 (the batches' 512-row tiles).
Lengths 1 2 3 4 5 (stage 1: 25 .. 125 rows around 54 .. 126; stage 2: 100 .. 500 rows around 118 .. 254 and 244 / 488;
stage 3: one 512-row tile or two), 9 10 (stage 1 around two 118-row tiles), 10 .. 13 (stage 0 around 54 / 58 / 62), 17 .. 19
(around 86 / 90 / 94), 21 22 (around two 54-row tiles), and 928 / 929 (either side of the fused-256 threshold; 4 640 rows:
many tiles at every stage).  ~2 000 frames in all.
Per length: the waveform against the oracle (WAV_RMS_GATE and three times the oracle's own re-association noise: ggml AVX2
order vs sequential f32); the same bits from calls under the batch regime (parity_helpers.BATCH_REGIME), with the 96-row
pair<256> tiles (ZV_PAIR_MT = 3) and with the merged MRF sum (ZV_MERGE_ALWAYS), on the same model with its lane poisoned before
each (every switch is read at the call); and the prefix property (the first T frames of
vocode(mel[:T + H]) are those of the long utterance).

Decoder at T = 255 / 256 / 257 / 513: the operand pre-pass threshold (t_max x nseg >= 256, decoder.cpp) and conv_gemm_kernel's
256-row tiles (one tile, one tile + 1 row, two tiles + 1 row), against the oracle with the gate of
test_gpu_decoder_encoder.py::test_medium_geometry_length_sweep, and the same bits under ZV_CONV_GEMM = 2, ZV_GEMM_ORDER = 0 and
ZV_DEC_PREPASS = 0 / 1."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WAV_RMS_GATE = 1e-4
LENGTHS = (1, 2, 3, 4, 5, 9, 10, 11, 12, 13, 17, 18, 19, 21, 22, 928, 929)


def _rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))


def test_medium_vocoder_length_sweep_vs_oracle(ckpt):
    from zerovox_cpp_amd import capi, synth
    from oracle import zvoracle
    from parity_helpers import BATCH_REGIME, oracle_pair
    path, g, tensors = ckpt("medium")
    regimes = (("batch", BATCH_REGIME), ("batch_pair256_96_rows", dict(BATCH_REGIME, ZV_PAIR_MT=3)),
               ("batch_merged_sum", dict(BATCH_REGIME, ZV_MERGE_ALWAYS=1)))
    m = capi.Model(path, 0)
    try:
        orc = zvoracle.Oracle(tensors)
        H = m.vocoder_halo_frames()
        mel = synth.vocoder_mel(g, tensors, 19, max(LENGTHS) + H + 8)
        full = m.vocode(mel)
        hop = g.hop_size
        for T in LENGTHS:
            wav = m.vocode(mel[:T])
            ref, alt = oracle_pair(orc, "vocoder", mel[:T])
            assert wav.shape == ref.shape == (T * hop,) and np.isfinite(wav).all(), T
            err, floor, sig = _rms(wav - ref), _rms(alt - ref), _rms(ref)
            print(f"T={T}: wav rms err {err:.3e} (oracle self-noise {floor:.3e}), max {np.max(np.abs(wav - ref)):.3e}, signal rms {sig:.3f}")
            assert err <= WAV_RMS_GATE, T
            assert err <= max(3.0 * floor, 3e-7 * sig), T
            for name, sw in regimes:
                m.poison()          # no regime finds another's values in the lane
                with capi.switches(**sw):
                    assert np.array_equal(m.vocode(mel[:T]), wav), (name, T)
            ctx = m.vocode(mel[: T + H])
            assert np.array_equal(ctx[: T * hop], full[: T * hop]), T
    finally:
        m.close()


def test_medium_decoder_pre_pass_and_gemm_tile_edges_vs_oracle(ckpt):
    from zerovox_cpp_amd import capi, synth
    from oracle import zvoracle
    from parity_helpers import oracle_pair
    path, g, tensors = ckpt("medium")
    m = capi.Model(path, 0)
    try:
        orc = zvoracle.Oracle(tensors)
        _, _, style = synth.encoder_inputs(g, 5, 4)
        for T in (255, 256, 257, 513):
            hid = synth.decoder_hidden(g, 80 + T, T, frames_per_phoneme=1, fill=1.0)
            mel = m.decode(hid, style)
            ref, alt = oracle_pair(orc, "decoder", hid, style)
            d, floor = mel - ref, alt - ref
            print(f"decoder medium T={T}: rms {_rms(d):.3e} max {np.max(np.abs(d)):.3e} (floor rms {_rms(floor):.3e} max {np.max(np.abs(floor)):.3e})")
            assert np.isfinite(mel).all(), T
            assert _rms(d) <= max(3.0 * _rms(floor), 3e-3) and np.max(np.abs(d)) <= max(3.0 * np.max(np.abs(floor)), 2e-2), T
            for sw in (dict(ZV_DEC_PREPASS=0), dict(ZV_DEC_PREPASS=1), dict(ZV_CONV_GEMM=2), dict(ZV_CONV_GEMM=2, ZV_DEC_PREPASS=1),
                       dict(ZV_CONV_GEMM=2, ZV_DEC_PREPASS=1, ZV_GEMM_ORDER=0), dict(ZV_CONV_GEMM=2, ZV_GEMM_ORDER=0)):
                with capi.switches(**sw):
                    assert np.array_equal(m.decode(hid, style), mel), (T, sw)
    finally:
        m.close()
