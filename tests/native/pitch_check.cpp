// Host-side driver of csrc/pitch.h for tests/test_pitch_cpu.py (no GPU, no HIP).
// Reads cases from stdin until it ends.  Every float travels as the hexadecimal bit pattern of its f32 value, so that inf, NaN and
// -0.0 arrive unchanged.  A case:
//     T sr hop n min_lag max_lag window threshold     the capacity in frames, the rate, the hop, the tokens, the zv_pitch parameters (0 = default)
//     n decimal integers                              the phoneme timings (n may be 0)
//     T * hop floats                                  the waveform
// and prints one line per case:
//     the resolved parameters | per frame f0:strength:Fq:voiced | per phoneme f0:voiced
// Fq and the flag decimal, everything else hexadecimal bit patterns; or "refused FIELD DEFAULTED" where pitch_params_resolve refuses.
#include "pitch.h"

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
    int T, sr, hop, n;
    unsigned lo, hi, win, thr;
    while (scanf("%d %d %d %d %u %u %u %x", &T, &sr, &hop, &n, &lo, &hi, &win, &thr) == 8)
    {
        if (T < 1 || hop < 1 || sr < 1 || n < 0 || (int64_t)T * hop > (1 << 26)) return fprintf(stderr, "case %ld: bad header\n", cases), 2;
        std::vector<int32_t> dur(n);
        std::vector<float> w((size_t)T * hop);
        for (int i = 0; i < n; i++)
            if (scanf("%d", &dur[i]) != 1) return fprintf(stderr, "case %ld: short timings\n", cases), 2;
        for (size_t i = 0; i < w.size(); i++)
        {
            unsigned b = 0;
            if (scanf("%x", &b) != 1) return fprintf(stderr, "case %ld: short sample line\n", cases), 2;
            w[i] = from_bits(b);
        }
        zv::PitchParams p = {lo, hi, win, from_bits(thr)};
        bool defaulted = false;
        if (const char *field = zv::pitch_params_resolve((uint32_t)sr, (uint32_t)hop, p, &defaulted))
        {
            printf("refused %s %d\n", field, defaulted ? 1 : 0);
            cases++;
            continue;
        }
        printf("%u %u %u %x |", p.min_lag, p.max_lag, p.window, zv::level_bits(p.voiced_threshold));
        std::vector<zv::PitchFrameRow> frames(T);
        std::vector<zv::PitchPhonemeRow> phonemes(n);
        zv::pitch_reference(w.data(), (uint32_t)T, (uint32_t)sr, (uint32_t)hop, p, dur.data(), (uint32_t)n, frames.data(),
                            n ? phonemes.data() : nullptr);
        for (int f = 0; f < T; f++)
        {
            zv::PitchSlabRow s;
            const zv::PitchFrameRow row = zv::pitch_frame_reference(w.data(), w.size(), (uint32_t)f, (uint32_t)sr, (uint32_t)hop, p, s);
            if (memcmp(&row, &frames[f], sizeof(row)) != 0) return fprintf(stderr, "case %ld: frame %d differs between the two references\n", cases, f), 2;
            printf(" %x:%x:%u:%u", zv::level_bits(row.f0_hz), zv::level_bits(row.strength), s.fq, s.voiced);
        }
        printf(" |");
        for (int i = 0; i < n; i++) printf(" %x:%x", zv::level_bits(phonemes[i].f0_hz), zv::level_bits(phonemes[i].voiced));
        printf("\n");
        cases++;
    }
    if (!feof(stdin)) return fprintf(stderr, "case %ld: malformed header\n", cases), 2;
    return 0;
}
