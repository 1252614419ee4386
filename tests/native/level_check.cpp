// Host-side driver of csrc/level.h for tests/test_level_cpu.py (no GPU, no HIP).
// Reads cases from stdin until it ends.  Every number that is a float travels as the hexadecimal bit pattern of its f32 value, so that
// inf, NaN and -0.0 arrive unchanged.  Two kinds of case:
//     0 n cap gain target_rms peak_ceiling          then a line of cap samples: the whole rule (zv::level_reference) over a waveform
//                                                    of cap samples whose first n are speech
//     1 S n peak gain target_rms peak_ceiling       the level and the gain from given totals (zv::level_report): S and n decimal
// and prints one line per case:
//     S  peak bits  rms as the bits of the f64  the three floats of the report as bits (rms, peak, gain)  reserved  hash
// hash = sum over the scaled samples of bits_i * (i + 1), modulo 2^64 (0 for a case of kind 1).
#include "level.h"

#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

static float from_bits(unsigned b)
{
    float f;
    memcpy(&f, &b, 4);
    return f;
}

int main()
{
    int kind;
    long cases = 0;
    while (scanf("%d", &kind) == 1)
    {
        uint64_t S = 0, n = 0, cap = 0, hash = 0;
        unsigned peak = 0, g = 0, t = 0, c = 0;
        zv::LevelRow r;
        if (kind == 0)
        {
            if (scanf("%" SCNu64 " %" SCNu64 " %x %x %x", &n, &cap, &g, &t, &c) != 5 || n > cap || cap > (1u << 26))
                return fprintf(stderr, "case %ld: bad header\n", cases), 2;
            std::vector<float> x(cap), out(cap);
            for (uint64_t i = 0; i < cap; i++)
            {
                unsigned b = 0;
                if (scanf("%x", &b) != 1) return fprintf(stderr, "case %ld: short sample line\n", cases), 2;
                x[i] = from_bits(b);
            }
            r = zv::level_reference(x.data(), n, cap, from_bits(g), from_bits(t), from_bits(c), out.data(), &S);
            for (uint64_t i = 0; i < cap; i++) hash += (uint64_t)zv::level_bits(out[i]) * (i + 1);
        }
        else if (kind == 1)
        {
            if (scanf("%" SCNu64 " %" SCNu64 " %x %x %x %x", &S, &n, &peak, &g, &t, &c) != 6) return fprintf(stderr, "case %ld: bad header\n", cases), 2;
            r = zv::level_report(S, n, peak, from_bits(g), from_bits(t), from_bits(c));
        }
        else
            return fprintf(stderr, "case %ld: bad kind %d\n", cases, kind), 2;
        const double rms = zv::level_rms(S, n);
        uint64_t rms_bits;
        memcpy(&rms_bits, &rms, 8);
        printf("%" PRIu64 " %x %" PRIx64 " %x %x %x %u %" PRIu64 "\n", S, zv::level_bits(r.peak), rms_bits, zv::level_bits(r.rms), zv::level_bits(r.peak),
               zv::level_bits(r.gain), r.reserved, hash);
        cases++;
    }
    return 0;
}
