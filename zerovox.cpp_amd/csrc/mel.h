// mel.h — mel analysis (include/zerovox_amd.h "mel analysis"): a waveform's log-mel rows, the domain zv_vocode* reads.  Plain
// arithmetic shared by mel_frames_kernel / mel_rows_kernel (mel_kernels.hip), the C-ABI (capi.cpp) and the host-side test
// (tests/native/mel_check.cpp): nothing here needs HIP.
//
// A frame is the band levels' 1 024-point DFT (bands.h) at twice the digits on BOTH operands.  The span is block scaled by the band
// levels' quantiser (bands_exponent, bands_quant: |a| <= 8 191) and split into two signed base-128 digits (bands_digits); the windowed
// twiddles are integers of at most 8 188 in magnitude, split the same way.  Four digit-plane products give three i32 sums per (frame,
// bin, cos / sin), each below 2^23, so any split over lanes, waves and matrix instructions gives the same Re and Im (int64, below 2^37).
// Behind the sums every f64 step is ONE IEEE operation, written as a statement of its own; the library builds with -ffp-contract=off.
// The logarithm is NOT libm's: mel_ln is a fixed sequence of such steps, so the device and every host give the same bits.
#pragma once

#include <math.h>
#include <stdint.h>

#include "bands.h"         // BANDS_N, BANDS_BINS, the block quantiser, the digits, the table's fragment order

#if !defined(__HIP_DEVICE_COMPILE__)
#include <vector>
#endif

namespace zv
{

constexpr int      MEL_SCALE = 8188;                               // twiddle scale: at 8 188 no table product is near a tie (mel_twiddle)
constexpr uint32_t MEL_MAX_MELS = 256;                             // channels per row
constexpr uint32_t MEL_FLOOR_BITS = 0x2edbe6ffu;                   // 1e-10f: what floor = 0 means
constexpr int      MEL_TILE_FRAMES = 32;                           // frames one workgroup of mel_frames_kernel covers: two 16-row matrix tiles
constexpr int      MEL_ROWS_FRAMES = 4;                            // frames one workgroup of mel_rows_kernel covers
constexpr int      MEL_SLAB_STRIDE = BANDS_BINS;                   // f64 magnitudes per frame row of the slab between the two kernels
// The table on the device: two digit planes (0: the high digits, 1: the low ones), each in the band levels' fragment order
constexpr size_t MEL_TABLE_BYTES = 2 * BANDS_TABLE_BYTES;
ZV_LV_FN size_t mel_table_index(int plane, int trig, int bin, int t) { return (size_t)plane * BANDS_TABLE_BYTES + bands_table_index(trig, bin, t); }
// The parameter block in HBM, 32-bit words: [centre, pad, log, the floor's bits (resolved), num_mels, 0, 0, 0], then per channel
// [first bin, end bin) of its non-zero weights (MEL_MAX_MELS pairs), then the weights, f32 [num_mels][513]
constexpr int MEL_PAR_HEAD = 8, MEL_PAR_WEIGHTS = MEL_PAR_HEAD + 2 * (int)MEL_MAX_MELS;
ZV_LV_FN size_t mel_par_words(uint32_t num_mels) { return (size_t)MEL_PAR_WEIGHTS + (size_t)num_mels * BANDS_BINS; }

// (the launches' grids: stage_plan.h mel_plan)

// ---- span: frame f covers the samples f * hop + centre - 512 + t, t = 0 .. 1023 ----
ZV_LV_FN int64_t mel_span(uint32_t f, uint32_t hop, uint32_t centre) { return (int64_t)f * hop + centre - BANDS_N / 2; }
// where sample s of the utterance x[0 .. S) is read, or -1: +0.0.  pad 0: zeros outside; pad 1: reflected without repeating the edge
// (-j -> j, S - 1 + j -> S - 1 - j), which stays inside for S >= 513 (checked by the caller; an index that does not reads +0.0)
ZV_LV_FN int64_t mel_sample_index(int64_t s, int64_t S, uint32_t pad)
{
    if (s >= 0 && s < S) return s;
    if (!pad) return -1;
    const int64_t r = s < 0 ? -s : 2 * (S - 1) - s;
    return r >= 0 && r < S ? r : -1;
}

// ---- magnitude: the three digit sums of cos and of sin -> |X(k)| re full scale ----
ZV_LV_FN int64_t mel_combine(int32_t a2, int32_t a1, int32_t a0) { return 16384 * (int64_t)a2 + 128 * (int64_t)a1 + (int64_t)a0; }
ZV_LV_FN double mel_magnitude(int64_t re, int64_t im, int k)
{
    const double r = (double)re, i = (double)im;
    double p = r * r;
    const double q = i * i;
    p = p + q;
    double g = sqrt(p);
    g = g * bands_pow2(-k);
    g = g / (double)MEL_SCALE;
    return g;
}

// ---- level: v = max(acc, floor); log 0: log10, 1: ln, 2: linear ----
ZV_LV_FN double mel_from_bits(uint64_t b)
{
    double d;
    __builtin_memcpy(&d, &b, 8);
    return d;
}
// ln of a positive normal f64: v = m * 2^e with m in [sqrt(1/2), sqrt(2)), s = (m - 1) / (m + 1), ln m = 2 s (1 + z/3 + ... + z^6/13),
// z = s * s.  |s| <= 0.1716, so what is cut off is below 4.4e-13.  The constants are the f64 nearest to 1/13 ... 1/3, ln 2 and log10 e.
ZV_LV_FN double mel_ln(double v)
{
    uint64_t b;
    __builtin_memcpy(&b, &v, 8);
    int e = (int)((b >> 52) & 0x7ffu) - 1022;                      // frexp: v = m * 2^e, 0.5 <= m < 1
    double m = mel_from_bits((b & 0x000fffffffffffffull) | 0x3fe0000000000000ull);
    if (m < mel_from_bits(0x3fe6a09e667f3bcdull))                  // sqrt(1/2)
    {
        m = m * 2.0;
        e = e - 1;
    }
    const double num = m - 1.0, den = m + 1.0;
    const double s = num / den;
    const double z = s * s;
    double poly = mel_from_bits(0x3fb3b13b13b13b14ull);           // 1/13
    poly = poly * z;
    poly = poly + mel_from_bits(0x3fb745d1745d1746ull);            // 1/11
    poly = poly * z;
    poly = poly + mel_from_bits(0x3fbc71c71c71c71cull);            // 1/9
    poly = poly * z;
    poly = poly + mel_from_bits(0x3fc2492492492492ull);            // 1/7
    poly = poly * z;
    poly = poly + mel_from_bits(0x3fc999999999999aull);            // 1/5
    poly = poly * z;
    poly = poly + mel_from_bits(0x3fd5555555555555ull);            // 1/3
    poly = poly * z;
    poly = poly + 1.0;
    double lnm = 2.0 * s;
    lnm = lnm * poly;
    double r = (double)e * mel_from_bits(0x3fe62e42fefa39efull);   // ln 2
    r = r + lnm;
    return r;
}
ZV_LV_FN float mel_floor(float floor) { return floor == 0.0f ? level_from_bits(MEL_FLOOR_BITS) : floor; }
// the row entry from the channel's sum; floor: resolved (mel_floor), positive and finite
ZV_LV_FN float mel_level(double acc, float floor, uint32_t log)
{
    const double fl = (double)floor;
    const double v = acc > fl ? acc : fl;
    if (log == 2u) return (float)v;
    double r = mel_ln(v);
    if (log == 0u) r = r * mel_from_bits(0x3fdbcb7b1526e50eull);   // log10 e
    return (float)r;
}
// one channel of one frame: acc = +0.0, then ascending bins, one multiply and one add each; bins outside [lo, hi) carry zero weights,
// which cannot change acc (a product of a zero weight and a finite magnitude is a zero, and acc is never -0.0)
ZV_LV_FN double mel_channel(const float *w, const double *g, uint32_t lo, uint32_t hi)
{
    double acc = 0.0;
    for (uint32_t k = lo; k < hi; k++)
    {
        const double t = (double)w[k] * g[k];
        acc = acc + t;
    }
    return acc;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- host side only: the table, the design, the parameter block and the reference; a device pass sees none of it ----
// one table entry: trig 0 is C[k][t], trig 1 is S[k][t], floor(8188 * w[t] * trig(2 pi k t / 1024) + 0.5) with the periodic Hann window
// (bands_window).  At scale 8 188 no product lies within 1.4e-5 of a half-integer (odd scales meet exact ties where w * cos = 1/2), so
// any libm gives the same integer.
inline int mel_twiddle(int trig, int k, int t)
{
    const double ang = 2.0 * M_PI * (double)((k * t) % BANDS_N) / (double)BANDS_N;
    const double x = (double)MEL_SCALE * bands_window(t) * (trig ? sin(ang) : cos(ang));
    return (int)floor(x + 0.5);
}
// the plain tables [2][513][1024] and the kernel's image of them (mel_table_index)
inline std::vector<int16_t> mel_tables()
{
    std::vector<int16_t> tab((size_t)2 * BANDS_BINS * BANDS_N);
    for (int trig = 0; trig < 2; trig++)
        for (int k = 0; k < BANDS_BINS; k++)
            for (int t = 0; t < BANDS_N; t++) tab[((size_t)trig * BANDS_BINS + k) * BANDS_N + t] = (int16_t)mel_twiddle(trig, k, t);
    return tab;
}
inline std::vector<int8_t> mel_table_fragments(const std::vector<int16_t> &tab)
{
    std::vector<int8_t> img(MEL_TABLE_BYTES, 0);
    for (int trig = 0; trig < 2; trig++)
        for (int k = 0; k < BANDS_BINS; k++)
            for (int t = 0; t < BANDS_N; t++)
            {
                int32_t hi, lo;
                bands_digits(tab[((size_t)trig * BANDS_BINS + k) * BANDS_N + t], hi, lo);
                img[mel_table_index(0, trig, k, t)] = (int8_t)hi;
                img[mel_table_index(1, trig, k, t)] = (int8_t)lo;
            }
    return img;
}

// The design (zv_mel_design): Slaney-scale triangular filters with Slaney area normalisation on the 513 bin centres k * rate / 1024,
// in f64, each weight rounded to f32 once.
//   mel(f) = 3 f / 200 below 1 000 Hz, else 15 + 27 ln(f / 1000) / ln 6.4; hz() is its inverse;
//   p[i] = hz(mel(fmin) + i (mel(fmax) - mel(fmin)) / (num_mels + 1)), i = 0 .. num_mels + 1;
//   W[c][k] = max(0, min((f_k - p[c]) / (p[c+1] - p[c]), (p[c+2] - f_k) / (p[c+2] - p[c+1]))) * 2 / (p[c+2] - p[c]).
// fmax 0 = Nyquist.  Returns null, else the name of the field that is wrong.
inline double mel_hz_to_mel(double f) { return f < 1000.0 ? 3.0 * f / 200.0 : 15.0 + 27.0 * log(f / 1000.0) / log(6.4); }
inline double mel_mel_to_hz(double m) { return m < 15.0 ? 200.0 * m / 3.0 : 1000.0 * exp(log(6.4) * (m - 15.0) / 27.0); }
inline const char *mel_design(uint32_t rate, uint32_t num_mels, float fmin_hz, float fmax_hz, float *weights)
{
    if (rate == 0) return "sampling_rate";
    if (num_mels == 0 || num_mels > MEL_MAX_MELS) return "num_mels";
    const double nyq = 0.5 * (double)rate;
    if (!isfinite(fmin_hz) || fmin_hz < 0.0f) return "fmin_hz";
    if (!isfinite(fmax_hz) || fmax_hz < 0.0f) return "fmax_hz";
    const double lo = (double)fmin_hz, hi = fmax_hz == 0.0f ? nyq : (double)fmax_hz;
    if (hi > nyq) return "fmax_hz";
    if (!(lo < hi)) return "fmin_hz";
    const double m0 = mel_hz_to_mel(lo), m1 = mel_hz_to_mel(hi);
    std::vector<double> p(num_mels + 2);
    for (uint32_t i = 0; i < num_mels + 2; i++) p[i] = mel_mel_to_hz(m0 + (double)i * (m1 - m0) / (double)(num_mels + 1));
    for (uint32_t c = 0; c < num_mels; c++)
        for (int k = 0; k < BANDS_BINS; k++)
        {
            const double f = (double)k * (double)rate / (double)BANDS_N;
            const double up = (f - p[c]) / (p[c + 1] - p[c]), down = (p[c + 2] - f) / (p[c + 2] - p[c + 1]);
            double w = up < down ? up : down;
            w = w > 0.0 ? w : 0.0;
            weights[(size_t)c * BANDS_BINS + k] = (float)(w * (2.0 / (p[c + 2] - p[c])));
        }
    return nullptr;
}

// A zv_mel as plain values.  weights: [num_mels * 513] or null = the design.
struct MelParams
{
    const float *weights;
    float        fmin_hz, fmax_hz;
    uint32_t     centre, pad, log;
    float        floor;
};
// Validation and the parameter block (mel_par_words(num_mels) words).  S: the shortest utterance's samples (pad 1 needs 513).  Returns
// null, else the name of the field that is wrong.
inline const char *mel_resolve(const MelParams &q, uint32_t rate, uint32_t hop, uint32_t num_mels, uint64_t S, std::vector<uint32_t> &par)
{
    if (num_mels == 0 || num_mels > MEL_MAX_MELS) return "num_mels";
    if (q.centre >= hop) return "centre";
    if (q.pad > 1u) return "pad";
    if (q.pad == 1u && S < (uint64_t)BANDS_BINS) return "pad (T)";
    if (q.log > 2u) return "log";
    if (!isfinite(q.floor) || q.floor < 0.0f) return "floor";
    par.assign(mel_par_words(num_mels), 0u);
    float *w = (float *)(par.data() + MEL_PAR_WEIGHTS);
    if (q.weights)
    {
        for (size_t i = 0; i < (size_t)num_mels * BANDS_BINS; i++)
        {
            if (!isfinite(q.weights[i])) return "weights";
            w[i] = q.weights[i];
        }
    }
    else if (const char *field = mel_design(rate, num_mels, q.fmin_hz, q.fmax_hz, w))
        return field;
    par[0] = q.centre;
    par[1] = q.pad;
    par[2] = q.log;
    par[3] = level_bits(mel_floor(q.floor));
    par[4] = num_mels;
    for (uint32_t c = 0; c < num_mels; c++)
    {
        uint32_t lo = 0, hi = 0;
        for (uint32_t k = 0; k < (uint32_t)BANDS_BINS; k++)
            if (w[(size_t)c * BANDS_BINS + k] != 0.0f)
            {
                if (hi == 0) lo = k;
                hi = k + 1;
            }
        par[MEL_PAR_HEAD + 2 * c] = lo;
        par[MEL_PAR_HEAD + 2 * c + 1] = hi;
    }
    return nullptr;
}

// Host reference of one frame's 513 magnitudes: x[0 .. S) is the utterance's waveform, tab the plain tables
inline void mel_frame_magnitudes(const float *x, uint64_t S, uint32_t f, uint32_t hop, uint32_t centre, uint32_t pad, const int16_t *tab, double *g)
{
    const int64_t s0 = mel_span(f, hop, centre);
    float y[BANDS_N];
    uint32_t pk = 0;
    for (int t = 0; t < BANDS_N; t++)
    {
        const int64_t s = mel_sample_index(s0 + t, (int64_t)S, pad);
        y[t] = 0.0f;
        if (s >= 0 && level_abs_bits(x[s]) == (level_bits(x[s]) & 0x7fffffffu)) y[t] = x[s];
        const uint32_t a = level_abs_bits(y[t]);
        pk = a > pk ? a : pk;
    }
    for (int k = 0; k < BANDS_BINS; k++) g[k] = 0.0;
    if (pk < BANDS_SILENT_BITS) return;
    const int k2 = bands_exponent(pk);
    const double scale = bands_pow2(k2);
    int32_t hi[BANDS_N], lo[BANDS_N];
    for (int t = 0; t < BANDS_N; t++) bands_digits(bands_quant(y[t], scale), hi[t], lo[t]);
    for (int bin = 0; bin < BANDS_BINS; bin++)
    {
        int64_t sum[2];
        for (int trig = 0; trig < 2; trig++)
        {
            const int16_t *c = tab + ((size_t)trig * BANDS_BINS + bin) * BANDS_N;
            int32_t a2 = 0, a1 = 0, a0 = 0;
            for (int t = 0; t < BANDS_N; t++)
            {
                int32_t chi, clo;
                bands_digits(c[t], chi, clo);
                a2 += hi[t] * chi;
                a1 += hi[t] * clo + lo[t] * chi;
                a0 += lo[t] * clo;
            }
            sum[trig] = mel_combine(a2, a1, a0);
        }
        g[bin] = mel_magnitude(sum[0], sum[1], k2);
    }
}

// Host reference of the whole rule for one utterance: x[0 .. T * hop), par a resolved parameter block, out [T][num_mels]
inline void mel_reference(const float *x, uint32_t T, uint32_t hop, const uint32_t *par, const int16_t *tab, float *out)
{
    const uint32_t M = par[4];
    const float *w = (const float *)(par + MEL_PAR_WEIGHTS);
    std::vector<double> g(BANDS_BINS);
    for (uint32_t f = 0; f < T; f++)
    {
        mel_frame_magnitudes(x, (uint64_t)T * hop, f, hop, par[0], par[1], tab, g.data());
        for (uint32_t c = 0; c < M; c++)
            out[(size_t)f * M + c] = mel_level(mel_channel(w + (size_t)c * BANDS_BINS, g.data(), par[MEL_PAR_HEAD + 2 * c], par[MEL_PAR_HEAD + 2 * c + 1]),
                                               level_from_bits(par[3]), par[2]);
    }
}

#endif

}  // namespace zv
