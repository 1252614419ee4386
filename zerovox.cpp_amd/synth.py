"""Deterministic synthetic ZeroVox checkpoints with the reference's exact weight contract.

No real checkpoint exists offline, so every parity case runs on a synthetic GGUF
whose tensor names / shapes / dtypes are those the reference's stage classes look up
(src/fs2encoder.cpp:29-62,152-171,344-382,504-505; src/stylettsdec.cpp:33-66,163-168,220-239,
334-340; src/hifigan.cpp:34-39,84-95,208-218) and whose KV keys are those of src/zerovox.h:17-33.

Values come from a counter-based integer hash (splitmix64) -> float, so a (geometry, seed) pair
produces bit-identical files on every machine: the GPU box regenerates the checkpoints the golden
fixtures were made from instead of shipping 193 MB files.

Two value families (make_tensors(..., family=)): "uniform", the default every fixture but one was made from, and "trained",
the same tensors with the value distribution of a trained checkpoint (heavy tails, channel gains spread over octaves, exact zeros,
f16 subnormals, pruned channels, norm gains that include 0 and negatives) — a statistical stand-in, not a trained model.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import numpy as np

ARCH = "zerovox-resnet-fs2-styletts"
NUM_PHONEMES = 154          # reference src/zerovox.h:35
NUM_PUNCTS = 6              # reference src/zerovox.h:36

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _fnv1a64(s: str) -> int:
    h = 0xCBF29CE484222325
    for b in s.encode():
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def _splitmix64(x: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        z = x
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def u01(seed: int, name: str, n: int) -> np.ndarray:
    """n uniform doubles in [0,1) that depend only on (seed, name, index)."""
    base = np.uint64((_fnv1a64(name) ^ (seed * 0x2545F4914F6CDD1D)) & 0xFFFFFFFFFFFFFFFF)
    with np.errstate(over="ignore"):
        idx = np.arange(n, dtype=np.uint64) * np.uint64(0xD1342543DE82EF95) + base
    return (_splitmix64(idx) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def sym(seed: int, name: str, shape, amp: float) -> np.ndarray:
    n = int(np.prod(shape))
    return ((u01(seed, name, n) * 2.0 - 1.0) * amp).astype(np.float32).reshape(shape)


def normal(seed: int, name: str, shape, std: float = 1.0) -> np.ndarray:
    """Box-Muller on two hashed uniforms (float64 math, cast to f32)."""
    n = int(np.prod(shape))
    a = u01(seed, name + "/a", n)
    b = u01(seed, name + "/b", n)
    z = np.sqrt(-2.0 * np.log(1.0 - a)) * np.cos(2.0 * np.pi * b)
    return (z * std).astype(np.float32).reshape(shape)


@dataclass
class Geometry:
    name: str = "medium"
    emb_dim: int = 512
    punct_emb_dim: int = 16
    conv_filter_size: int = 1024            # encoder FFN width (KV key says "decoder.", src/zerovox.cpp:111)
    conv_kernel_size: Tuple[int, int] = (9, 1)
    encoder_layer: int = 4
    encoder_head: int = 2
    vp_filter_size: int = 256
    vp_kernel_size: int = 3
    ve_n_bins: int = 256
    decoder_n_head: int = 2                 # read by the reference, unused
    max_seq_len: int = 1500
    num_mels: int = 80
    hop_size: int = 300
    sampling_rate: int = 22050
    residual_dim: int = 64                  # hard-coded in the reference (src/zerovox.cpp:124)
    voc_channels: int = 512
    voc_kernel_size: int = 7
    upsample_scales: Tuple[int, ...] = (5, 5, 4, 3)        # hard-coded, src/zerovox.cpp:129
    upsample_kernels: Tuple[int, ...] = (10, 10, 8, 6)
    resblock_kernels: Tuple[int, ...] = (3, 7, 11)
    resblock_dilations: Tuple[int, ...] = (1, 3, 5)        # hard-coded, src/zerovox.cpp:132
    # per-conv tap counts that differ from resblock_kernels[branch]: (branch, dilation, conv (1 or 2), K), in every stage
    # (the file stores one tensor per conv, and the reference reads each one's K from its shape, src/hifigan.cpp:125,164)
    resblock_overrides: Tuple[Tuple[int, int, int, int], ...] = ()

    def resblock_k(self, branch: int, dilation: int, conv: int) -> int:
        k = self.resblock_kernels[branch]
        for b, d, c, kk in self.resblock_overrides:
            if (b, d, c) == (branch, dilation, conv):
                k = kk
        return k

    @property
    def E(self) -> int:
        return self.emb_dim + self.punct_emb_dim

    def kv(self) -> Dict[str, int]:
        p = ARCH + "."
        return {
            p + "max_seq_len": self.max_seq_len,
            p + "emb_dim": self.emb_dim,
            p + "punct_emb_dim": self.punct_emb_dim,
            p + "decoder.n_head": self.decoder_n_head,
            p + "encoder.layer": self.encoder_layer,
            p + "encoder.head": self.encoder_head,
            p + "encoder.vp_filter_size": self.vp_filter_size,
            p + "encoder.vp_kernel_size": self.vp_kernel_size,
            p + "encoder.ve_n_bins": self.ve_n_bins,
            p + "decoder.conv_filter_size": self.conv_filter_size,
            p + "decoder.conv_kernel_size.0": self.conv_kernel_size[0],
            p + "decoder.conv_kernel_size.1": self.conv_kernel_size[1],
            p + "audio.sampling_rate": self.sampling_rate,
            p + "audio.num_mels": self.num_mels,
            p + "audio.hop_size": self.hop_size,
        }


MEDIUM = Geometry()
# Same topology, every width shrunk; channel counts deliberately NOT multiples of 16/32 so the
# kernels' padding paths are exercised (SURVEY.md §8c "tiny-geometry GGUF with identical topology").
TINY = Geometry(name="tiny", emb_dim=48, punct_emb_dim=16, conv_filter_size=72, encoder_layer=2,
                encoder_head=2, vp_filter_size=40, ve_n_bins=16, max_seq_len=64, voc_channels=48)
# A mid-size geometry: big enough that every MFMA tile shape is hit, small enough for quick CPU runs.
SMALL = Geometry(name="small", emb_dim=112, punct_emb_dim=16, conv_filter_size=256, encoder_layer=2,
                 encoder_head=2, vp_filter_size=64, ve_n_bins=64, max_seq_len=256, voc_channels=128)

# MEDIUM with 8 pitch / energy bins (`encoder.ve_n_bins` is a free KV of the checkpoint format): a bin is 1/7 wide, 300 times
# the summation-order noise of the predictions, so an utterance whose predictions all sit >= 0.1 bin from a boundary makes
# the same integer decisions under any re-association — the un-forced end-to-end golden (tests/golden/make_golden.py)
MEDIUM8 = Geometry(name="medium8", ve_n_bins=8)

# MEDIUM with another `encoder.head` (a free KV of the checkpoint format, read by the reference and the loader alike): head dims
# dk = E / H = 528 (H = 1: above the matrix-core attention's 288), 176 (H = 3: a matrix-core head dim that is not a multiple of 64),
# 132 (H = 4: ns = dk / 2 = 66, the MFMA loop's last group of two steps) and 66 (H = 8: dk % 4 != 0, the scalar kernel only)
MEDIUM_H1 = Geometry(name="medium_h1", encoder_head=1)
MEDIUM_H3 = Geometry(name="medium_h3", encoder_head=3)
MEDIUM_H4 = Geometry(name="medium_h4", encoder_head=4)
MEDIUM_H8 = Geometry(name="medium_h8", encoder_head=8)
# MEDIUM with E = 1024 > 64 x LN_MAXE = 768: the encoder's LayerNorm rows take add_layernorm_kernel's path for wide rows; 4 heads
# of dk = 256 keep both attention kernels legal
MEDIUM_E1024 = Geometry(name="medium_e1024", emb_dim=1008, encoder_head=4)

# MEDIUM with other residual-block tap counts (every conv's K is a free shape of the checkpoint format).  Stages of 256, 128, 64 and
# 32 channels reach every fused kernel:
#  * rb357: K = 5 is not pair-fusable at 32 channels (an odd number of 4-step MFMA bodies) while 3 and 7 are; at 64 channels
#    K = 5 runs resblock_pair64 and resblock_block64;
#  * rb_wide: 15 taps (no whole-block kernel at 32 channels: the halo leaves too few rows; 256- and 128-channel tiles with 14 halo
#    rows), 9 (fusable at 64 channels and up) and 1 (a 'same' 1-tap conv, fusable at 128 and 256 channels only);
#  * rb_dilk: the 11-tap branch's last dilation pair has 7 taps (a branch whose K changes over its dilations);
#  * rb_c1c2: convs1 and convs2 of one pair differ (7 / 3 in branch 1, 11 / 13 in branch 2, dilation 0), a convs2 wider than
#    every convs1 of the stage;
#  * rb_c2wide: every convs2 of the 11-tap branch has 25 taps — a receptive radius of 25 frames, beyond the 23 of a halo that
#    counts convs1 of dilation 0 alone (such pairs are never fused: convs1 and convs2 differ)
MEDIUM_RB357 = Geometry(name="medium_rb357", resblock_kernels=(3, 5, 7))
MEDIUM_RB_WIDE = Geometry(name="medium_rb_wide", resblock_kernels=(15, 9, 1))
MEDIUM_RB_DILK = Geometry(name="medium_rb_dilk", resblock_overrides=((2, 2, 1, 7), (2, 2, 2, 7)))
MEDIUM_RB_C1C2 = Geometry(name="medium_rb_c1c2", resblock_overrides=((1, 0, 2, 3), (2, 0, 2, 13)))
MEDIUM_RB_C2WIDE = Geometry(name="medium_rb_c2wide", resblock_overrides=((2, 0, 2, 25), (2, 1, 2, 25), (2, 2, 2, 25)))
RESBLOCK_GEOMETRIES = ("medium_rb357", "medium_rb_wide", "medium_rb_dilk", "medium_rb_c1c2", "medium_rb_c2wide")

# checkpoints the loader refuses (the reference hard-codes what these change, src/zerovox.cpp:127-129, src/hifigan.cpp:261,338):
# upsample strides (4, 5, 5, 3) — still a hop of 300 — and 5-tap input / output convs
MEDIUM_UP4553 = Geometry(name="medium_up4553", upsample_scales=(4, 5, 5, 3), upsample_kernels=(8, 10, 10, 6))
MEDIUM_VOCK5 = Geometry(name="medium_vock5", voc_kernel_size=5)

# other encoder / decoder widths, FFN tap counts and mel counts (emb_dim + punct_emb_dim, decoder.conv_kernel_size.{0,1},
# encoder.vp_filter_size, encoder.layer and audio.num_mels are free KVs of the checkpoint format).  A decoder conv of Cout
# channels has ceil(Cout / 32) output tiles: batches run whole groups of 8 on conv_gemm_kernel (plus one leftover tile), two
# or more leftovers on conv1d_mfma_kernel from tile nt_begin = 8 x groups on (conv.hip launch_conv):
#  * e576: decoder convs of 18 / 36 tiles (GEMM 16 / 32 + 2 / 4 at nt_begin); dk = 288 = 2 x ATT_NS_MAX, the matrix-core
#    attention's widest head, whose LDS takes at most 320 tokens (the scalar kernel above); 128 mels; a 3-tap FFN w_2 over
#    F = 1 024 f16 channels, run per utterance;
#  * e720: 23 / 45 tiles (7 / 5 leftover; the last tile half padding, 720 = 22.5 x 32); dk = 240; 272 mels: the vocoder input
#    conv stages two 256-channel chunks under its (mel - mean) / scale prologue, to_out has 8.5 tiles; V = 784 > 768 turns the
#    LayerNorm tails off by V alone; a 17-tap FFN w_1 (16 halo rows);
#  * small_e304: 10 / 19 tiles (GEMM 8 / 16 + 2 / 3); one encoder layer; 16 mels; the FFN's f16 operand has padded columns
#    (200 -> 208) and a 1-tap w_1 / 5-tap w_2
MEDIUM_E576 = Geometry(name="medium_e576", emb_dim=560, encoder_head=2, num_mels=128, conv_kernel_size=(3, 3))
MEDIUM_E720 = Geometry(name="medium_e720", emb_dim=704, encoder_head=3, num_mels=272, conv_kernel_size=(17, 1), vp_filter_size=784)
SMALL_E304 = Geometry(name="small_e304", emb_dim=272, punct_emb_dim=32, conv_filter_size=200, conv_kernel_size=(1, 5),
                      encoder_layer=1, encoder_head=2, vp_filter_size=64, ve_n_bins=32, max_seq_len=256, voc_channels=128,
                      num_mels=16)
# (medium_e1024 above: the whole encoder with the tails off by E; decoder convs of 2 048 / 2 112 channels, GEMM groups with no
# leftover)
ENCDEC_GEOMETRIES = ("medium_e576", "medium_e720", "small_e304", "medium_e1024")

# checkpoints the loader refuses: 100 mels (the loader requires num_mels % 16 == 0; the reference does not) and an 8-tap FFN
# conv (not a 'same' conv)
MEDIUM_M100 = Geometry(name="medium_m100", num_mels=100)
MEDIUM_FFN8 = Geometry(name="medium_ffn8", conv_kernel_size=(8, 1))

# SMALL with other vocoder widths (the width is the shape of `_meldec.input_conv.w`; it halves per upsample stage).  The schedule
# picks a stage's kernels by its padded channel count Cp (csrc/voc_plan.h, csrc/conv_plan.h), not by its position, so each width
# puts the kernels at other rates (5 / 25 / 100 / 300 rows per frame) than medium (256 / 128 / 64 / 32), small (64 / 32 / 16 / 16)
# and tiny (32 / 16 / 16 / 16) do; tests/native/voc_plan_check.cpp pins the plan of each:
#  * small_v256: 128 / 64 / 32 / 16 — resblock_pair_kernel<128> at rate 5 (behind it an upsample of stride 5), pair64 / block64 at
#    rate 25, the whole-block 32-channel kernel at rate 100, its three outputs read by the next upsample conv's three-input
#    prologue; the last stage (16 channels) on the generic conv kernel, as is the 16-channel output conv; tail groups split a last
#    stage that is not the whole-block kernel;
#  * small_v496: 248 / 124 / 62 / 31 real channels in 256 / 128 / 64 / 32 padded ones — every fused kernel, every upsample conv
#    (padded Cout) and the output conv (C = 31) with pad channels; the input conv has 15.5 output tiles;
#  * small_v768: 384 / 192 / 96 / 48 — no fused kernel anywhere: the generic kernel's 11-tap dilation-5 convs over a 256 + 128
#    channel split and over 192 / 96 / 48 channels in one chunk, a 768 -> 5 x 384 upsample conv on conv_gemm_kernel (7 groups of 8
#    tiles, 4 leftover tiles on conv1d_mfma_kernel from nt_begin = 56), stages of 1.5 output tiles;
#  * small_v1024: 512 / 256 / 128 / 64 — an unfused 512-channel stage (two 256-channel chunks), resblock_pair_kernel<256> at rate
#    25, <128> at rate 100, and a 64-channel last stage at rate 300: pair64 / block64 there, whose merged MRF sum the output conv
#    reads, alone, in its one-input form (also inside a tail group)
SMALL_V256 = Geometry(name="small_v256", emb_dim=112, punct_emb_dim=16, conv_filter_size=256, encoder_layer=2, encoder_head=2,
                      vp_filter_size=64, ve_n_bins=64, max_seq_len=256, voc_channels=256)
SMALL_V496 = Geometry(name="small_v496", emb_dim=112, punct_emb_dim=16, conv_filter_size=256, encoder_layer=2, encoder_head=2,
                      vp_filter_size=64, ve_n_bins=64, max_seq_len=256, voc_channels=496)
SMALL_V768 = Geometry(name="small_v768", emb_dim=112, punct_emb_dim=16, conv_filter_size=256, encoder_layer=2, encoder_head=2,
                      vp_filter_size=64, ve_n_bins=64, max_seq_len=256, voc_channels=768)
SMALL_V1024 = Geometry(name="small_v1024", emb_dim=112, punct_emb_dim=16, conv_filter_size=256, encoder_layer=2, encoder_head=2,
                       vp_filter_size=64, ve_n_bins=64, max_seq_len=256, voc_channels=1024)
VOC_WIDTH_GEOMETRIES = ("small_v256", "small_v496", "small_v768", "small_v1024")

# TINY at other sampling rates (`audio.sampling_rate` is a free KV of the checkpoint format; the hop stays 300).  Loudness takes
# its 100 ms gating step from the rate, (rate + 5) / 10 samples, and cuts the signal into chunks of 256 (csrc/loudness.h):
#  * tiny_sr4000: step 400, the lowest rate the design takes — most chunks meet two steps, a step spans two or three chunks;
#  * tiny_sr5120: step 512, exactly two chunks — no chunk ever holds a step edge, its second run stays empty;
#  * tiny_sr48000: step 4 800, the rate of the standard's own coefficient table;
#  * tiny_sr3999: the loader takes it, loudness refuses it (a chunk could meet three steps)
TINY_SR4000 = Geometry(name="tiny_sr4000", emb_dim=48, punct_emb_dim=16, conv_filter_size=72, encoder_layer=2, encoder_head=2,
                       vp_filter_size=40, ve_n_bins=16, max_seq_len=64, voc_channels=48, sampling_rate=4000)
TINY_SR5120 = Geometry(name="tiny_sr5120", emb_dim=48, punct_emb_dim=16, conv_filter_size=72, encoder_layer=2, encoder_head=2,
                       vp_filter_size=40, ve_n_bins=16, max_seq_len=64, voc_channels=48, sampling_rate=5120)
TINY_SR48000 = Geometry(name="tiny_sr48000", emb_dim=48, punct_emb_dim=16, conv_filter_size=72, encoder_layer=2, encoder_head=2,
                        vp_filter_size=40, ve_n_bins=16, max_seq_len=64, voc_channels=48, sampling_rate=48000)
TINY_SR3999 = Geometry(name="tiny_sr3999", emb_dim=48, punct_emb_dim=16, conv_filter_size=72, encoder_layer=2, encoder_head=2,
                       vp_filter_size=40, ve_n_bins=16, max_seq_len=64, voc_channels=48, sampling_rate=3999)
RATE_GEOMETRIES = ("tiny_sr4000", "tiny_sr5120", "tiny_sr48000")

GEOMETRIES = {g.name: g for g in (MEDIUM, TINY, SMALL, MEDIUM8, MEDIUM_H1, MEDIUM_H3, MEDIUM_H4, MEDIUM_H8, MEDIUM_E1024,
                                  MEDIUM_RB357, MEDIUM_RB_WIDE, MEDIUM_RB_DILK, MEDIUM_RB_C1C2, MEDIUM_RB_C2WIDE, MEDIUM_UP4553,
                                  MEDIUM_VOCK5, MEDIUM_E576, MEDIUM_E720, SMALL_E304, MEDIUM_M100, MEDIUM_FFN8, SMALL_V256,
                                  SMALL_V496, SMALL_V768, SMALL_V1024, TINY_SR4000, TINY_SR5120, TINY_SR48000, TINY_SR3999)}


def sinusoid_table(n_position: int, d_hid: int) -> np.ndarray:
    """Same formula as utils/zv2gguf.py:41-62 (angles evaluated in float64, table cast to f32
    BEFORE sin/cos are applied in f32 — the converter builds the angle array with dtype=float32
    and then overwrites slices with np.sin/np.cos of those f32 angles)."""
    pos = np.arange(n_position, dtype=np.float64)[:, None]
    j = np.arange(d_hid)[None, :]
    ang = (pos / np.power(10000.0, 2 * (j // 2) / d_hid)).astype(np.float32)
    ang[:, 0::2] = np.sin(ang[:, 0::2])
    ang[:, 1::2] = np.cos(ang[:, 1::2])
    return ang


FAMILIES = ("uniform", "trained")

# the "trained" family: octave ranges of the three gains a weight carries (per input channel, per element, per output channel),
# the shares of exact zeros and of f16 subnormals, the count and size (in tensor RMS) of the outliers, and the fewest channels
# an axis needs before one of them is pruned
TRAINED_OCT_IN, TRAINED_OCT_ELEM, TRAINED_OCT_OUT = 3.0, 2.0, 1.5
TRAINED_ZERO_SHARE, TRAINED_SUBNORMAL_SHARE = 0.02, 0.01
TRAINED_OUTLIERS, TRAINED_OUTLIER_RMS = 6, (4.0, 8.0)
TRAINED_PRUNE_MIN = 32
TRAINED_GAIN_RANGE = (-1.5, 3.0)                 # norm gains
TRAINED_BIAS_MULT = 10.0                         # biases: ten times the uniform family's (+-0.1 -> +-1)
# the vocoder has no norm between its convs and ends in tanh: biases of +-1 there saturate the waveform (RMS 0.87), +-0.15 keep
# its RMS within 2 x the uniform family's
TRAINED_VOC_BIAS_MULT = 1.5
F16_SUBNORMAL_STEP = 2.0 ** -24                  # f16 subnormals are 1 .. 1023 of these


def _octaves(seed: int, name: str, n: int, span: float) -> np.ndarray:
    """n gains 2^U(-span, span)"""
    return np.exp2((u01(seed, name, n) * 2.0 - 1.0) * span)


def trained_pruned(seed: int, name: str, oc: int, ic: int) -> Tuple[int, int]:
    """(output channel, input channel) of a "trained" conv tensor that are all zero; -1 where the axis has fewer than
    TRAINED_PRUNE_MIN channels"""
    u = u01(seed, name + "#t/prune", 2)
    return (int(u[0] * oc) if oc >= TRAINED_PRUNE_MIN else -1, int(u[1] * ic) if ic >= TRAINED_PRUNE_MIN else -1)


def _trained_matrix(seed: int, name: str, shape, rms: float) -> np.ndarray:
    """normal x per-input-channel x per-element x per-output-channel octave gain, renormalised to `rms` (float64);
    shape = (out, in) or (out, in, k)"""
    n = int(np.prod(shape))
    oc, ic = shape[0], shape[1]
    ax = (slice(None), None) + (None,) * (len(shape) - 2)
    w = normal(seed, name + "#t/z", shape).astype(np.float64)
    w = w * _octaves(seed, name + "#t/ge", n, TRAINED_OCT_ELEM).reshape(shape)
    w = w * _octaves(seed, name + "#t/gi", ic, TRAINED_OCT_IN)[(None,) + ax[:-1]]
    w = w * _octaves(seed, name + "#t/go", oc, TRAINED_OCT_OUT)[ax]
    return w * (rms / np.sqrt(np.mean(w * w)))


def trained_conv_weight(seed: int, name: str, oc: int, ic: int, k: int, gain: float) -> np.ndarray:
    """an f16 conv weight [oc][ic][k] with the marks of a trained one: heavy tails and channel gains spread over octaves
    (_trained_matrix, at the uniform family's RMS gain / sqrt(ic k)), a few outliers at 4-8 x the RMS, ~1 % f16 subnormals,
    ~2 % exact zeros of both signs, and one all-zero output and input channel where the axis has >= TRAINED_PRUNE_MIN channels"""
    shape, n = (oc, ic, k), oc * ic * k
    rms = gain / np.sqrt(ic * k)
    w = _trained_matrix(seed, name, shape, rms).reshape(n)
    sign = np.where(u01(seed, name + "#t/sign", n) < 0.5, -1.0, 1.0)
    kind = u01(seed, name + "#t/kind", n)
    sub = kind < TRAINED_SUBNORMAL_SHARE
    steps = np.clip(np.rint(np.exp2(u01(seed, name + "#t/sub", n) * 10.0)), 1, 1023)       # 2^-24 .. 1023 x 2^-24
    w = np.where(sub, sign * steps * F16_SUBNORMAL_STEP, w)
    zero = (kind >= TRAINED_SUBNORMAL_SHARE) & (kind < TRAINED_SUBNORMAL_SHARE + TRAINED_ZERO_SHARE)
    w = np.where(zero, sign * 0.0, w)
    n_out = max(1, min(TRAINED_OUTLIERS, n // 1024))                  # one per 1 024 elements, so that they do not set the RMS
    u_out = u01(seed, name + "#t/outlier", 2 * n_out)
    at = np.minimum((u_out[:n_out] * n).astype(np.int64), n - 1)
    lo, hi = TRAINED_OUTLIER_RMS
    w[at] = sign[at] * rms * (lo + (hi - lo) * u_out[n_out:])
    w = w.reshape(shape)
    po, pi = trained_pruned(seed, name, oc, ic)
    if po >= 0:
        w[po] = 0.0
    if pi >= 0:
        w[:, pi] = 0.0
    return w.astype(np.float16)


def make_tensors(g: Geometry, seed: int, family: str = "uniform") -> List[Tuple[str, np.ndarray]]:
    """All tensors of SURVEY.md Appx A in numpy (C-order) shape = reversed ggml ne.

    family "uniform": every weight uniform in +-sqrt(3 / fan-in), norm gains 1 +- 0.1, biases +-0.1.  family "trained": the same
    names, shapes and dtypes with the value distribution of a trained checkpoint (DESIGN.md "The trained-like weight family"):
    a statistical stand-in, not a trained model."""
    if family not in FAMILIES:
        raise ValueError(f"unknown weight family {family!r}")
    trained = family == "trained"
    E, F = g.E, g.conv_filter_size
    T: List[Tuple[str, np.ndarray]] = []

    def add(name, arr):
        T.append((name, np.ascontiguousarray(arr)))

    def conv_w(name, oc, ic, k, gain=1.0):           # f16, ggml ne [k, ic, oc]
        if trained:
            return add(name, trained_conv_weight(seed, name, oc, ic, k, gain))
        amp = gain * np.sqrt(3.0 / (ic * k))
        add(name, sym(seed, name, (oc, ic, k), amp).astype(np.float16))

    def lin_w(name, out, inp, gain=1.0):             # f32, ggml ne [in, out]
        if trained:
            return add(name, _trained_matrix(seed, name, (out, inp), gain / np.sqrt(inp)).astype(np.float32))
        add(name, sym(seed, name, (out, inp), gain * np.sqrt(3.0 / inp)))

    def vec(name, n, amp=0.1, center=0.0):
        if trained and center == 1.0:                # a norm gain: spread over TRAINED_GAIN_RANGE, one exact 0, one forced negative
            lo, hi = TRAINED_GAIN_RANGE
            v = (lo + (hi - lo) * u01(seed, name + "#t", n)).astype(np.float32)
            at = np.minimum((u01(seed, name + "#t/at", 2) * n).astype(np.int64), n - 1)
            v[at[0]] = 0.0
            if n > 1:
                i = at[1] if at[1] != at[0] else (at[1] + 1) % n
                v[i] = np.float32(lo)
            return add(name, v)
        if trained:
            amp = amp * (TRAINED_VOC_BIAS_MULT if name.startswith("_meldec.") else TRAINED_BIAS_MULT)
        add(name, (sym(seed, name, (n,), amp) + np.float32(center)).astype(np.float32))

    def emb(name, key, shape, amp, padding_row=False):
        if trained:                                  # normal at the uniform family's RMS; row 0 is padding_idx
            e = normal(seed, key + "#t", shape, amp / np.sqrt(3.0))
            if padding_row:
                e[0] = 0.0
            return add(name, e)
        add(name, sym(seed, key, shape, amp))

    # ---- vocoder statistics
    if trained:
        add("hifigan.mean", (sym(seed, "hifigan.mean#t", (g.num_mels,), 2.0) + np.float32(-5.0)).astype(np.float32))
        u = u01(seed, "hifigan.scale#t", g.num_mels)
        add("hifigan.scale", (0.05 * np.exp(u * np.log(3.0 / 0.05))).astype(np.float32))
    else:
        vec("hifigan.mean", g.num_mels, amp=1.0, center=-1.0)
        vec("hifigan.scale", g.num_mels, amp=0.5, center=1.0)

    # ---- FastSpeech2 encoder
    add("sinusoid_encoding_table", sinusoid_table(g.max_seq_len + 1, E))
    emb("_pe._enc.src_word_emb.w", "_pe._enc.src_word_emb.w", (NUM_PHONEMES + 1, g.emb_dim), 1.0, padding_row=True)
    emb("_pe._enc.punct_embed.w", "_pe._enc.punct_embed.w", (NUM_PUNCTS + 1, g.punct_emb_dim), 1.0, padding_row=True)
    for i in range(g.encoder_layer):
        p = f"_pe._enc.laystk.{i}."
        for nm in ("w_qs", "w_ks", "w_vs", "fc"):
            lin_w(p + f"slf_attn.{nm}.w", E, E)
            vec(p + f"slf_attn.{nm}.b", E)
        vec(p + "slf_attn.layer_norm.w", E, center=1.0)
        vec(p + "slf_attn.layer_norm.b", E)
        conv_w(p + "pos_ffn.w_1.w", F, E, g.conv_kernel_size[0], gain=1.4)
        vec(p + "pos_ffn.w_1.b", F)
        conv_w(p + "pos_ffn.w_2.w", E, F, g.conv_kernel_size[1], gain=1.4)
        vec(p + "pos_ffn.w_2.b", E)
        vec(p + "pos_ffn.layer_norm.w", E, center=1.0)
        vec(p + "pos_ffn.layer_norm.b", E)
    V = g.vp_filter_size
    for pred, lin_gain, lin_bias in (("duration_predictor", 0.25, 1.6), ("pitch_predictor", 0.15, 0.5),
                                     ("engy_pred", 0.15, 0.5)):
        p = f"_pe._var_adapt.{pred}."
        conv_w(p + "conv_layer.conv1d_1.conv.w", V, E, g.vp_kernel_size, gain=1.4)
        vec(p + "conv_layer.conv1d_1.conv.b", V)
        vec(p + "conv_layer.layer_norm_1.w", V, center=1.0)
        vec(p + "conv_layer.layer_norm_1.b", V)
        conv_w(p + "conv_layer.conv1d_2.conv.w", V, V, g.vp_kernel_size, gain=1.4)
        vec(p + "conv_layer.conv1d_2.conv.b", V)
        vec(p + "conv_layer.layer_norm_2.w", V, center=1.0)
        vec(p + "conv_layer.layer_norm_2.b", V)
        lin_w(p + "linear_layer.w", 1, V, gain=lin_gain)
        add(p + "linear_layer.b", np.array([lin_bias], dtype=np.float32))
    emb("_pe._var_adapt.pitch_embedding.w", "pitch_embedding", (g.ve_n_bins, E), 0.5)
    emb("_pe._var_adapt.energy_embedding.w", "energy_embedding", (g.ve_n_bins, E), 0.5)

    # ---- StyleTTS mel decoder
    R = g.residual_dim
    for i, (ci, co) in enumerate(((E, 2 * E), (2 * E, 2 * E))):
        p = f"_mel_decoder.encode.{i}."
        conv_w(p + "conv1.w", ci, ci, 3, gain=1.4)
        vec(p + "conv1.b", ci)
        conv_w(p + "conv2.w", co, ci, 3, gain=1.4)
        vec(p + "conv2.b", co)
        if ci != co:
            conv_w(p + "conv1x1.w", co, ci, 1)
        for n in ("norm1", "norm2"):
            vec(p + n + ".w", ci, center=1.0)
            vec(p + n + ".b", ci)
    conv_w("_mel_decoder.asr_res.0.w", R, E, 1)
    vec("_mel_decoder.asr_res.0.b", R)
    vec("_mel_decoder.asr_res.1.w", R, center=1.0)
    vec("_mel_decoder.asr_res.1.b", R)
    dims = ((2 * E + R, 2 * E), (2 * E + R, 2 * E), (2 * E + R, E), (E, E), (E, E))
    for i, (ci, co) in enumerate(dims):
        p = f"_mel_decoder.decode.{i}."
        lin_w(p + "norm1.fc.w", 2 * ci, E)
        vec(p + "norm1.fc.b", 2 * ci)
        lin_w(p + "norm2.fc.w", 2 * co, E)
        vec(p + "norm2.fc.b", 2 * co)
        conv_w(p + "conv1.w", co, ci, 3, gain=1.4)
        vec(p + "conv1.b", co)
        conv_w(p + "conv2.w", co, co, 3, gain=1.4)
        vec(p + "conv2.b", co)
        if ci != co:
            conv_w(p + "conv1x1.w", co, ci, 1)
    conv_w("_mel_decoder.to_out.0.w", g.num_mels, E, 1)
    vec("_mel_decoder.to_out.0.b", g.num_mels)

    # ---- HiFi-GAN vocoder (channels halve per upsample stage).  Gains are chosen so that the waveform has a
    # speech-like level (RMS ~0.1, peaks ~0.35): the reference's re-association noise floor is a fixed
    # *relative* ~4.5e-4 of the signal (f16 operand rounding, SURVEY.md Appx D), so the absolute 1e-4 RMS
    # gate only means something at a realistic amplitude.
    C = g.voc_channels
    conv_w("_meldec.input_conv.w", C, g.num_mels, g.voc_kernel_size)
    vec("_meldec.input_conv.b", C)
    for i, (s, k) in enumerate(zip(g.upsample_scales, g.upsample_kernels)):
        ci, co = C >> i, C >> (i + 1)
        # stored already flipped + permuted to (out, in, k) (utils/zv2gguf.py:175-178); a transposed
        # conv of stride s uses k/s taps per output sample, hence fan-in ci*k/s
        amp_gain = np.sqrt(s)
        conv_w(f"_meldec.upsamples.{i}.1.w", co, ci, k, gain=1.0 * amp_gain)
        vec(f"_meldec.upsamples.{i}.1.b", co)
        for j in range(len(g.resblock_kernels)):
            n = i * len(g.resblock_kernels) + j
            for d in range(len(g.resblock_dilations)):
                conv_w(f"_meldec.blocks.{n}.convs1.{d}.1.w", co, co, g.resblock_k(j, d, 1), gain=1.0)
                vec(f"_meldec.blocks.{n}.convs1.{d}.1.b", co)
                conv_w(f"_meldec.blocks.{n}.convs2.{d}.1.w", co, co, g.resblock_k(j, d, 2), gain=0.2)
                vec(f"_meldec.blocks.{n}.convs2.{d}.1.b", co)
    cl = C >> len(g.upsample_scales)
    conv_w("_meldec.output_conv.1.w", 1, cl, g.voc_kernel_size, gain=0.5)
    vec("_meldec.output_conv.1.b", 1, amp=0.01)
    return T


def write_checkpoint(path: str, g: Geometry, seed: int, trim_dims: bool = False, family: str = "uniform") -> None:
    from .gguf import write_gguf
    write_gguf(path, g.kv(), make_tensors(g, seed, family), arch=ARCH, trim_dims=trim_dims)


# ---- seeded synthetic inputs -----------------------------------------

def encoder_inputs(g: Geometry, seed: int, n_phonemes: int):
    ids = 1 + (u01(seed, "ids", n_phonemes) * NUM_PHONEMES).astype(np.int32)          # U{1..154}
    puncts = (u01(seed, "puncts", n_phonemes) * (NUM_PUNCTS + 1)).astype(np.int32)    # U{0..6}
    style = normal(seed, "style", (g.E,), 0.05)
    return np.minimum(ids, NUM_PHONEMES).astype(np.int32), np.minimum(puncts, NUM_PUNCTS).astype(np.int32), style


def vocoder_mel(g: Geometry, tensors: Dict[str, np.ndarray], seed: int, T: int) -> np.ndarray:
    """mel[T, num_mels] = mean + scale * N(0,1) so the normalised vocoder input is N(0,1)."""
    z = normal(seed, "mel", (T, g.num_mels), 1.0)
    return (tensors["hifigan.mean"][None, :] + tensors["hifigan.scale"][None, :] * z).astype(np.float32)


def decoder_hidden(g: Geometry, seed: int, T: int, frames_per_phoneme: int = 4, fill: float = 0.8) -> np.ndarray:
    """Piece-wise constant hidden[T, E] (what the length regulator emits) with a zero-padded tail."""
    n_used = int(T * fill)
    n_ph = (n_used + frames_per_phoneme - 1) // frames_per_phoneme
    feat = normal(seed, "hidden", (n_ph, g.E), 1.5)
    h = np.zeros((T, g.E), dtype=np.float32)
    h[:n_used] = np.repeat(feat, frames_per_phoneme, axis=0)[:n_used]
    return h
