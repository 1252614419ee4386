// pitch.h — pitch track (include/zerovox_amd.h "pitch track"): the fundamental frequency and the voicing of an utterance as it runs,
// per frame and per phoneme.  Plain arithmetic shared by pitch_frames_kernel / pitch_phonemes_kernel (pitch_kernels.hip) and the
// host-side test (tests/native/pitch_check.cpp): nothing here needs HIP.
//
// A frame is a normalised cross-correlation of its span with itself over the lags [min_lag - 1, max_lag + 1].  The span is block
// scaled to integers of at most 1023 in magnitude (pitch_quant: one exact f64 product by a power of two, one f64 sum, a truncation),
// so the correlation sums c(L) and the energies E(L) are integers below 2^30: any split over lanes, loads and instructions gives the
// same sums.  Behind the sums every f64 step is ONE IEEE operation (a conversion, *, /, +, - or sqrt), written as a statement of its
// own; the library builds with -ffp-contract=off.  The pick takes maxima and smallest lags, which no order changes either.
#pragma once

#include <math.h>
#include <stdint.h>

#include "contour.h"       // ZV_LV_FN, level_bits, contour_extent

#if !defined(__HIP_DEVICE_COMPILE__)
#include <vector>
#endif

namespace zv
{

constexpr uint32_t PITCH_LAG_LO = 8, PITCH_LAG_HI = 512;           // 8 <= min_lag < max_lag <= 512
constexpr uint32_t PITCH_LAG_RATIO = 8;                            // max_lag <= 8 * min_lag: three octaves
constexpr uint32_t PITCH_WINDOW_LO = 64, PITCH_WINDOW_HI = 1024;   // 64 <= window <= 1024
constexpr int      PITCH_MAX_SPAN = (int)(PITCH_WINDOW_HI + PITCH_LAG_HI + 1);      // M = window + max_lag + 1 <= 1 537 samples
constexpr int      PITCH_MAX_LAGS = (int)(PITCH_LAG_HI - PITCH_LAG_HI / PITCH_LAG_RATIO + 3);      // lags min_lag - 1 .. max_lag + 1: <= 451
constexpr uint32_t PITCH_SILENT_BITS = 0x33800000u;                // 2^-24: a span whose peak is below it is silent
constexpr int32_t  PITCH_Q_MAX = 1023;
constexpr double   PITCH_PICK_SHARE = 0.875;                       // the first lag within 1/8 of the best one starts the search
// a parameter row in HBM, uint32 [segment][PITCH_PARAM_STRIDE]: min_lag, max_lag, window, the bits of voiced_threshold — resolved
constexpr int PITCH_PARAM_STRIDE = 4;
// frames one workgroup of pitch_frames_kernel covers (four waves, four frames each, a wave per frame at a time)
constexpr int PITCH_CHUNK_FRAMES = 16;

// rows of the two tables; the layouts of include/zerovox_amd.h zv_pitch_frame / zv_pitch_phoneme
struct PitchFrameRow
{
    float f0_hz, strength;
};
struct PitchPhonemeRow
{
    float f0_hz, voiced;
};
// what the frames pass keeps per frame for the phonemes pass: Fq = f0 in 1/256 Hz (0 unless voiced) and the voiced flag
struct PitchSlabRow
{
    uint32_t fq, voiced;
};
struct PitchParams
{
    uint32_t min_lag, max_lag, window;
    float    voiced_threshold;
};

// Defaults (a field at 0) and validation.  Returns null when `p` is usable, else the name of the first field that is not;
// *defaulted then tells whether that field's value was the default (the checkpoint's rate needs explicit lags).
ZV_LV_FN const char *pitch_params_resolve(uint32_t sr, uint32_t hop, PitchParams &p, bool *defaulted)
{
    const bool d_min = p.min_lag == 0, d_max = p.max_lag == 0, d_win = p.window == 0, d_thr = p.voiced_threshold == 0.0f;
    if (d_min) p.min_lag = sr / 441u;
    if (d_max) p.max_lag = sr / 63u;
    if (d_win) p.window = 2u * hop;
    if (d_thr) p.voiced_threshold = 0.5f;
    if (defaulted) *defaulted = false;
    if (!(p.min_lag >= PITCH_LAG_LO && p.min_lag < PITCH_LAG_HI))
    {
        if (defaulted) *defaulted = d_min;
        return "min_lag";
    }
    if (!(p.max_lag > p.min_lag && p.max_lag <= PITCH_LAG_HI && p.max_lag <= PITCH_LAG_RATIO * p.min_lag))
    {
        if (defaulted) *defaulted = d_max;
        return "max_lag";
    }
    if (!(p.window >= PITCH_WINDOW_LO && p.window <= PITCH_WINDOW_HI))
    {
        if (defaulted) *defaulted = d_win;
        return "window";
    }
    const uint32_t tb = level_bits(p.voiced_threshold);
    if (!(tb < 0x7f800000u && p.voiced_threshold > 0.0f && p.voiced_threshold <= 1.0f)) return "voiced_threshold";
    return nullptr;
}

// the span of frame f: its first sample s0 (signed; the span is w[s0 .. s0 + M), zeros outside the utterance) for M = window + max_lag + 1
ZV_LV_FN int64_t pitch_span(uint32_t f, uint32_t hop, uint32_t M) { return (int64_t)f * hop + hop / 2u - M / 2u; }

// a sample of the span as the peak sees it: its sign-cleared bits when it is finite, else 0 (the sample then counts as +0.0)
ZV_LV_FN uint32_t pitch_abs_bits(float x) { return level_abs_bits(x); }

// 2^k for the span whose peak has the bits pk >= PITCH_SILENT_BITS: e = (pk >> 23) - 127, k = 9 - e, so that the peak lands in 512 .. 1023
ZV_LV_FN double pitch_scale(uint32_t pk)
{
    const int k = 9 - ((int)(pk >> 23) - 127);                     // -118 <= k <= 33
    const uint64_t b = (uint64_t)(1023 + k) << 52;
    double s;
    __builtin_memcpy(&s, &b, 8);
    return s;
}

// the block-scaled sample: sign(y) * min((int64)(|y| * 2^k + 0.5), 1023); a NaN or infinite sample is 0
ZV_LV_FN int32_t pitch_quant(float y, double scale)
{
    const uint32_t b = level_bits(y), ab = pitch_abs_bits(y);
    double d = (double)level_from_bits(ab);
    d = d * scale;
    d = d + 0.5;
    int32_t q = (int32_t)d;                                        // 0.5 <= d < 1025: the conversion truncates, as the rule's (int64) does
    q = q < PITCH_Q_MAX ? q : PITCH_Q_MAX;
    return (b >> 31) ? -q : q;
}

// r(L) from the integer sums
ZV_LV_FN double pitch_corr(int64_t c, int64_t E0, int64_t EL)
{
    if (!(c > 0 && E0 > 0 && EL > 0)) return 0.0;
    const uint64_t prod = (uint64_t)E0 * (uint64_t)EL;
    double den = (double)prod;
    den = sqrt(den);
    double r = (double)c;
    r = r / den;
    return r < 1.0 ? r : 1.0;
}

// f0 from the three correlations around the picked lag (step 6)
ZV_LV_FN double pitch_refine(double rm, double r0, double rp, uint32_t lag, uint32_t sr)
{
    const double p = rm - r0, n = rp - r0, den = p + n;
    double delta = 0.0;
    if (den < 0.0)
    {
        delta = rm - rp;
        delta = delta / den;
        delta = delta * 0.5;
        if (!(delta >= -0.5 && delta <= 0.5)) delta = 0.0;
    }
    double l = (double)lag;
    l = l + delta;
    return (double)sr / l;
}

// the row and the slab entry of a frame from f0 and the strength (step 7); a silent frame or rmax == 0 is pitch_frame_none
ZV_LV_FN PitchFrameRow pitch_frame_row(double f0, double strength, float threshold, PitchSlabRow &slab)
{
    const bool voiced = strength >= (double)threshold;
    PitchFrameRow row;
    row.f0_hz = voiced ? (float)f0 : 0.0f;
    row.strength = (float)strength;
    double q = f0 * 256.0;
    q = q + 0.5;
    slab.fq = voiced ? (uint32_t)q : 0u;
    slab.voiced = voiced ? 1u : 0u;
    return row;
}
ZV_LV_FN PitchFrameRow pitch_frame_none(PitchSlabRow &slab)
{
    slab.fq = 0u;
    slab.voiced = 0u;
    PitchFrameRow row;
    row.f0_hz = 0.0f;
    row.strength = 0.0f;
    return row;
}

// steps 5 to 7 from the correlations r[L - (min_lag - 1)] of the lags min_lag - 1 .. max_lag + 1
ZV_LV_FN PitchFrameRow pitch_pick(const double *r, const PitchParams &p, uint32_t sr, PitchSlabRow &slab)
{
    const uint32_t lo = p.min_lag - 1u;
    double rmax = 0.0;
    for (uint32_t L = p.min_lag; L <= p.max_lag; L++) rmax = r[L - lo] > rmax ? r[L - lo] : rmax;
    if (rmax == 0.0) return pitch_frame_none(slab);
    const double gate = PITCH_PICK_SHARE * rmax;
    uint32_t L = p.min_lag;
    while (!(r[L - lo] >= gate)) L++;                              // ends at the lag of rmax at the latest
    while (L < p.max_lag && !(r[L + 1u - lo] <= r[L - lo])) L++;
    const double f0 = pitch_refine(r[L - 1u - lo], r[L - lo], r[L + 1u - lo], L, sr);
    return pitch_frame_row(f0, r[L - lo], p.voiced_threshold, slab);
}

// a phoneme's row from the sum of Fq over its voiced frames, their number and the phoneme's frames
ZV_LV_FN PitchPhonemeRow pitch_phoneme_row(uint64_t SF, uint64_t nv, uint64_t d)
{
    PitchPhonemeRow row;
    row.f0_hz = 0.0f;
    row.voiced = 0.0f;
    if (nv > 0)
    {
        double den = (double)nv;
        den = den * 256.0;
        double m = (double)SF;
        m = m / den;
        row.f0_hz = (float)m;
    }
    if (d > 0)
    {
        double s = (double)nv;
        s = s / (double)d;
        row.voiced = (float)s;
    }
    return row;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// Host reference of one frame: w[0 .. n) is the utterance's waveform, p is resolved.
inline PitchFrameRow pitch_frame_reference(const float *w, uint64_t n, uint32_t f, uint32_t sr, uint32_t hop, const PitchParams &p,
                                           PitchSlabRow &slab)
{
    const uint32_t W = p.window, M = W + p.max_lag + 1u, lo = p.min_lag - 1u, nl = p.max_lag + 1u - lo + 1u;
    const int64_t s0 = pitch_span(f, hop, M);
    std::vector<float> y(M, 0.0f);
    uint32_t pk = 0;
    for (uint32_t t = 0; t < M; t++)
    {
        const int64_t s = s0 + (int64_t)t;
        if (s >= 0 && (uint64_t)s < n && pitch_abs_bits(w[s]) == (level_bits(w[s]) & 0x7fffffffu)) y[t] = w[s];
        const uint32_t a = pitch_abs_bits(y[t]);
        pk = a > pk ? a : pk;
    }
    if (pk < PITCH_SILENT_BITS) return pitch_frame_none(slab);
    const double scale = pitch_scale(pk);
    std::vector<int32_t> a(M);
    for (uint32_t t = 0; t < M; t++) a[t] = pitch_quant(y[t], scale);
    int64_t E0 = 0;
    for (uint32_t t = 0; t < W; t++) E0 += (int64_t)a[t] * a[t];
    std::vector<double> r(nl);
    for (uint32_t L = lo; L <= p.max_lag + 1u; L++)
    {
        int64_t c = 0, E = 0;
        for (uint32_t t = 0; t < W; t++)
        {
            c += (int64_t)a[t] * a[t + L];
            E += (int64_t)a[t + L] * a[t + L];
        }
        r[L - lo] = pitch_corr(c, E0, E);
    }
    return pitch_pick(r.data(), p, sr, slab);
}

// Host reference of the whole rule for one utterance: w[0 .. T * hop) is the waveform of its capacity, durations [n] its phoneme
// timings, p resolved.  frames [T] and phonemes [n] receive the rows (either may be null).
inline void pitch_reference(const float *w, uint32_t T, uint32_t sr, uint32_t hop, const PitchParams &p, const int32_t *durations, uint32_t n,
                            PitchFrameRow *frames, PitchPhonemeRow *phonemes)
{
    std::vector<PitchSlabRow> slab(T);
    for (uint32_t f = 0; f < T; f++)
    {
        const PitchFrameRow row = pitch_frame_reference(w, (uint64_t)T * hop, f, sr, hop, p, slab[f]);
        if (frames) frames[f] = row;
    }
    uint64_t start = 0;
    for (uint32_t i = 0; phonemes && i < n; i++)
    {
        const uint64_t d = durations[i] > 0 ? (uint64_t)durations[i] : 0;
        uint64_t SF = 0, nv = 0;
        for (uint64_t f = start; f < start + d && f < T; f++)
        {
            SF += slab[f].fq;
            nv += slab[f].voiced;
        }
        phonemes[i] = pitch_phoneme_row(SF, nv, d);
        start += d;
    }
}
#endif

}  // namespace zv
