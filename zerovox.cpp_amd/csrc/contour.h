// contour.h — level contour (include/zerovox_amd.h "level contour"): the level of an utterance as it runs, per frame and per phoneme,
// in the measure of level.h.  Plain arithmetic shared by contour_frames_kernel / contour_phonemes_kernel (contour_kernels.hip) and the
// host-side test (tests/native/contour_check.cpp): nothing here needs HIP.
//
// A frame's totals are level.h's: S_f, the sum of the squared 1.19 magnitudes (level_quant) of its hop samples as a u64, and P_f, the
// largest level_abs_bits among them.  A phoneme's totals are the sum and the maximum of its frames' totals.  Integers and maxima of
// bit patterns: any split over loads, lanes and waves gives the same totals.  Behind them a row is level_rms (every f64 step ONE IEEE
// operation) and one f64 -> f32 conversion.
#pragma once

#include "level.h"

#if !defined(__HIP_DEVICE_COMPILE__)
#include <vector>
#endif

namespace zv
{

// frames one workgroup of contour_frames_kernel covers (four waves, eight frames each).  At the 300-sample hop of the shipped
// checkpoints that is LEVEL_CHUNK_SAMPLES samples, the chunk and hence the grid of the level passes; a workgroup then starts a
// multiple of 38 400 bytes = 300 lines of 128 bytes behind its segment's first sample, so no two workgroups of a segment share a
// line, and as the hop is a multiple of 4 every frame starts on a 16-byte boundary (contour_kernels.hip)
constexpr int CONTOUR_CHUNK_FRAMES = 32;
static_assert(CONTOUR_CHUNK_FRAMES * 300 == LEVEL_CHUNK_SAMPLES, "a contour chunk is a level chunk at hop 300");

// a row of either table; the layout of include/zerovox_amd.h zv_frame_level
struct ContourRow
{
    float rms, peak;
};

// the row of `samples` samples whose squares sum to S and whose largest magnitude has the bits `peak_bits`; no samples have the
// totals {0, 0} and so the row {0, 0} (level_rms returns 0 for S == 0 ahead of its quotient)
ZV_LV_FN ContourRow contour_row(uint64_t S, uint64_t samples, uint32_t peak_bits)
{
    ContourRow r;
    r.rms = (float)level_rms(S, samples);
    r.peak = level_from_bits(peak_bits);
    return r;
}

// frames [start, start + d) of phoneme i from the length regulator's inclusive scan `cum` [n], clipped to the capacity T exactly as the
// phoneme timings are (durations[i] = min(cum[i], T) - min(cum[i - 1], T)); d <= 0 where there is nothing to measure
ZV_LV_FN void contour_extent(const int32_t *cum, int i, int T, int &start, int &d)
{
    int a = i > 0 ? cum[i - 1] : 0, b = cum[i];
    a = a < 0 ? 0 : (a < T ? a : T);
    b = b < 0 ? 0 : (b < T ? b : T);
    start = a;
    d = b - a;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// Host reference of the whole rule for one utterance: w[0 .. T * hop) is the waveform of its capacity, durations [n] its phoneme
// timings.  frames [T] and phonemes [n] receive the rows (either may be null); S_out [T] and P_out [T] (may be null) the frames' totals.
inline void contour_reference(const float *w, uint32_t T, uint32_t hop, const int32_t *durations, uint32_t n, ContourRow *frames,
                              ContourRow *phonemes, uint64_t *S_out, uint32_t *P_out)
{
    std::vector<uint64_t> S(T, 0);
    std::vector<uint32_t> P(T, 0);
    for (uint32_t f = 0; f < T; f++)
    {
        for (uint32_t j = 0; j < hop; j++)
        {
            const float x = w[(size_t)f * hop + j];
            const uint64_t q = level_quant(x);
            S[f] += q * q;
            const uint32_t a = level_abs_bits(x);
            P[f] = a > P[f] ? a : P[f];
        }
        if (frames) frames[f] = contour_row(S[f], hop, P[f]);
        if (S_out) S_out[f] = S[f];
        if (P_out) P_out[f] = P[f];
    }
    uint64_t start = 0;
    for (uint32_t i = 0; phonemes && i < n; i++)
    {
        const uint64_t d = durations[i] > 0 ? (uint64_t)durations[i] : 0;
        uint64_t Sp = 0;
        uint32_t Pp = 0;
        for (uint64_t f = start; f < start + d && f < T; f++)
        {
            Sp += S[f];
            Pp = P[f] > Pp ? P[f] : Pp;
        }
        phonemes[i] = contour_row(Sp, d * hop, Pp);
        start += d;
    }
}
#endif

}  // namespace zv
