// Host-side driver of csrc/contour.h for tests/test_contour_cpu.py (no GPU, no HIP).
// Reads cases from stdin until it ends.  Every float travels as the hexadecimal bit pattern of its f32 value, so that inf, NaN and
// -0.0 arrive unchanged.  A case:
//     T hop n                    the capacity in frames, the hop, the tokens
//     n decimal integers         the length regulator's scan `cum` (not clipped to T: contour_extent does that, as the kernel does)
//     T * hop floats             the waveform
// and prints one line per case:
//     the n durations contour_extent gives | per frame S:P:rms:peak | per phoneme rms:peak
// S decimal, everything else hexadecimal bit patterns.
#include "contour.h"

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
    long cases = 0;
    int T, hop, n;
    while (scanf("%d %d %d", &T, &hop, &n) == 3)
    {
        if (T < 1 || hop < 1 || n < 1 || (int64_t)T * hop > (1 << 26)) return fprintf(stderr, "case %ld: bad header\n", cases), 2;
        std::vector<int32_t> cum(n), dur(n);
        std::vector<float> w((size_t)T * hop);
        for (int i = 0; i < n; i++)
            if (scanf("%d", &cum[i]) != 1) return fprintf(stderr, "case %ld: short scan\n", cases), 2;
        for (size_t i = 0; i < w.size(); i++)
        {
            unsigned b = 0;
            if (scanf("%x", &b) != 1) return fprintf(stderr, "case %ld: short sample line\n", cases), 2;
            w[i] = from_bits(b);
        }
        int at = 0;
        for (int i = 0; i < n; i++)
        {
            int start = 0;
            zv::contour_extent(cum.data(), i, T, start, dur[i]);
            if (start != at) return fprintf(stderr, "case %ld: phoneme %d starts at %d, not %d\n", cases, i, start, at), 2;
            at += dur[i];
            printf("%d ", dur[i]);
        }
        std::vector<zv::ContourRow> frames(T), phonemes(n);
        std::vector<uint64_t> S(T);
        std::vector<uint32_t> P(T);
        zv::contour_reference(w.data(), (uint32_t)T, (uint32_t)hop, dur.data(), (uint32_t)n, frames.data(), phonemes.data(), S.data(), P.data());
        printf("|");
        for (int f = 0; f < T; f++)
            printf(" %" PRIu64 ":%x:%x:%x", S[f], P[f], zv::level_bits(frames[f].rms), zv::level_bits(frames[f].peak));
        printf(" |");
        for (int i = 0; i < n; i++) printf(" %x:%x", zv::level_bits(phonemes[i].rms), zv::level_bits(phonemes[i].peak));
        printf("\n");
        cases++;
    }
    if (!feof(stdin)) return fprintf(stderr, "case %ld: malformed header\n", cases), 2;
    return 0;
}
