"""CPU: the identity behind run-shortened vocoding (include/zerovox_amd.h zv_vocode), checked on the oracle.

The vocoder has no normalisation over time and a finite reach of H frames, so over a run [a, b) of bit-identical mel rows its
output is one hop-long frame, repeated.  With Rmin = 2H + 1: vocode rows [0, a + Rmin) ++ [b, T) instead of all T, keep the
waveform up to frame a + H, move the rest b - a - Rmin frames further on, fill the gap with copies of frame a + H — and the full
waveform comes back BIT FOR BIT.  The helpers here are the model the GPU tests (tests/test_gpu_voc_runs.py) check the device's
run table against: the FIRST longest run of rows equal as 32-bit patterns, taken when it saves at least MARGIN frames."""
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 16            # VOC_RUN_MARGIN of csrc/kernels.h


def halo_frames(g):
    """Model::vocoder_halo_frames() (csrc/vocoder.cpp) from a geometry: input conv, per stage the polyphase upsample conv's taps at
    the stage's input rate and the widest residual block, the output conv; in frames, rounded up, + 1"""
    frames = float((g.voc_kernel_size - 1) // 2)
    rate = 1.0
    for i, s in enumerate(g.upsample_scales):
        K = g.upsample_kernels[i]
        off = (K - 1) - (s // 2 + s % 2)
        ds = [(k - off + r) // s for r in range(s) for k in range(K) if (k - off + r) % s == 0]
        frames += (2 * max(-min(ds + [0]), max(ds + [0])) + 1) / rate
        rate *= s
        reach = max(sum((g.resblock_k(j, d, 1) - 1) // 2 * dil + (g.resblock_k(j, d, 2) - 1) // 2
                        for d, dil in enumerate(g.resblock_dilations)) for j in range(len(g.resblock_kernels)))
        frames += reach / rate
    frames += ((g.voc_kernel_size - 1) // 2) / rate
    return int(math.ceil(frames)) + 1


def longest_run(mel):
    """[a, b): the first longest run of consecutive rows with the same BITS (-0 != +0, equal NaN patterns are equal)"""
    bits = np.ascontiguousarray(mel, dtype=np.float32).view(np.uint32)
    eq = np.concatenate([[False], (bits[1:] == bits[:-1]).all(axis=1)])
    best, a, cur = 1, 0, 1
    for t in range(1, len(eq)):
        cur = cur + 1 if eq[t] else 1
        if cur > best:
            best, a = cur, t - cur + 1
    return a, a + best


def run_entry(mel, H):
    """(frames vocoded, split frame, frames skipped) of the run table for one utterance"""
    T = mel.shape[0]
    a, b = longest_run(mel)
    if b - a >= 2 * H + 1 + MARGIN:
        return T - (b - a) + 2 * H + 1, a + H, b - a - (2 * H + 1)
    return T, T, 0


def shorten(mel, H):
    rows, split, shift = run_entry(mel, H)
    keep = split + H + 1
    return np.concatenate([mel[:keep], mel[keep + shift:]]) if shift else mel


def stretch(wav_short, mel, H, hop):
    """the full waveform from the short one: head copied, one frame replicated, tail shifted"""
    rows, split, shift = run_entry(mel, H)
    assert wav_short.shape == (rows * hop,)
    out = np.empty(mel.shape[0] * hop, np.float32)
    cut = (split + 1) * hop
    out[:cut] = wav_short[:cut]
    out[cut:cut + shift * hop] = np.tile(wav_short[split * hop:cut], shift)
    out[cut + shift * hop:] = wav_short[cut:]
    return out


def test_longest_run_compares_bits_and_takes_the_first_longest():
    rng = np.random.default_rng(5)
    mel = rng.standard_normal((40, 8)).astype(np.float32)
    assert longest_run(mel) == (0, 1)
    mel[5:12] = mel[5]
    mel[20:27] = mel[20]
    assert longest_run(mel) == (5, 12)                      # two runs of 7: the first
    mel[20:28] = mel[20]
    assert longest_run(mel) == (20, 28)                     # the longer one
    z = np.zeros((10, 8), np.float32)
    z[1::2, 3] = -0.0
    assert (z[1:] == z[:-1]).all() and longest_run(z) == (0, 1)      # equal as floats, not as bits
    n = np.full((10, 8), np.nan, np.float32)
    assert longest_run(n) == (0, 10)                        # NaN == NaN is false; the patterns are equal
    assert run_entry(np.zeros((200, 8), np.float32), 20) == (41, 20, 159)
    assert run_entry(np.zeros((56, 8), np.float32), 20) == (56, 56, 0) and run_entry(np.zeros((57, 8), np.float32), 20) == (41, 20, 16)


def test_oracle_waveform_of_the_run_shortened_mel_stretches_to_the_full_one(ckpt):
    from zerovox_cpp_amd import synth
    from oracle import zvoracle
    path, g, tensors = ckpt("medium")
    orc = zvoracle.Oracle(tensors)
    H, hop, T = halo_frames(g), g.hop_size, 320
    taken = 0
    for seed, N in ((200, 40), (201, 22)):
        ids, puncts, style = synth.encoder_inputs(g, seed, N)
        e = orc.encoder(g, ids, puncts, style, T)
        mel = orc.decoder(e["hidden"], style)
        a, b = longest_run(mel)
        rows, split, shift = run_entry(mel, H)
        print(f"N={N}: n_frames {e['n_frames']}, run [{a}, {b}), H {H}, vocoded rows {rows} of {T}")
        # the decoder's 3-tap convs reach 14 frames behind the utterance and 15 in front of the end
        assert a <= e["n_frames"] + 14 and b >= T - 15
        assert shift > 0 and rows == T - (b - a) + 2 * H + 1
        full = orc.vocoder(mel, hop)
        short = orc.vocoder(shorten(mel, H), hop)
        got = stretch(short, mel, H, hop)
        assert np.array_equal(got.view(np.uint32), full.view(np.uint32)), (seed, N)
        taken += 1
    assert taken == 2
