// Host-side driver of csrc/envelope.h (and, for the combined cases, csrc/level.h) for tests/test_envelope_cpu.py (no GPU, no HIP).
// Reads cases from stdin until it ends.  Every number that is a float travels as the hexadecimal bit pattern of its f32 value, so that
// inf, NaN and -0.0 arrive unchanged.  A case:
//     T hop n r Fi Fo have_gain have_volume      the capacity in frames, the hop, the tokens, the three scalars of the envelope, flags
//     n decimal integers                         the length regulator's scan `cum`
//     n floats                                   the gains, only with have_gain
//     3 floats                                   gain target_rms peak_ceiling, only with have_volume
//     T * hop floats                             the waveform
// and prints one line per case:
//     nf  the nf + 1 knots (none when nf == 0)  hash of the enveloped samples  [S  rms peak gain as bits  hash of the final samples]
// hash = sum over the samples of bits_i * (i + 1), modulo 2^64.
#include "envelope.h"
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

static uint64_t hash_of(const std::vector<float> &v)
{
    uint64_t h = 0;
    for (size_t i = 0; i < v.size(); i++) h += (uint64_t)zv::level_bits(v[i]) * (i + 1);
    return h;
}

int main()
{
    long cases = 0;
    int T, hop, n, r, have_gain, have_volume;
    unsigned Fi, Fo;
    while (scanf("%d %d %d %d %u %u %d %d", &T, &hop, &n, &r, &Fi, &Fo, &have_gain, &have_volume) == 8)
    {
        if (T < 1 || hop < 1 || n < 1 || r < 0 || r > zv::ENV_MAX_RAMP || (int64_t)T * hop > (1 << 26))
            return fprintf(stderr, "case %ld: bad header\n", cases), 2;
        std::vector<int32_t> cum(n);
        std::vector<float> gain(n), x((size_t)T * hop), y(x.size());
        for (int i = 0; i < n; i++)
            if (scanf("%d", &cum[i]) != 1) return fprintf(stderr, "case %ld: short scan\n", cases), 2;
        for (int i = 0; have_gain && i < n; i++)
        {
            unsigned b = 0;
            if (scanf("%x", &b) != 1) return fprintf(stderr, "case %ld: short gains\n", cases), 2;
            gain[i] = from_bits(b);
        }
        unsigned vb[3] = {0, 0, 0};
        if (have_volume && scanf("%x %x %x", &vb[0], &vb[1], &vb[2]) != 3) return fprintf(stderr, "case %ld: bad volume\n", cases), 2;
        for (size_t i = 0; i < x.size(); i++)
        {
            unsigned b = 0;
            if (scanf("%x", &b) != 1) return fprintf(stderr, "case %ld: short sample line\n", cases), 2;
            x[i] = from_bits(b);
        }
        const int total = cum[n - 1] < 0 ? 0 : cum[n - 1], nf = total < T ? total : T;
        std::vector<uint32_t> B((size_t)nf + 1);
        zv::envelope_reference(x.data(), T, hop, cum.data(), n, nf, have_gain ? gain.data() : nullptr, r, Fi, Fo, y.data(), B.data());
        printf("%d", nf);
        for (int f = 0; nf > 0 && f <= nf; f++) printf(" %u", B[f]);
        printf(" %" PRIu64, hash_of(y));
        if (have_volume)
        {
            uint64_t S = 0;
            std::vector<float> w(y.size());
            const zv::LevelRow lv = zv::level_reference(y.data(), (uint64_t)nf * hop, y.size(), from_bits(vb[0]), from_bits(vb[1]), from_bits(vb[2]),
                                                        w.data(), &S);
            printf(" %" PRIu64 " %x %x %x %" PRIu64, S, zv::level_bits(lv.rms), zv::level_bits(lv.peak), zv::level_bits(lv.gain), hash_of(w));
        }
        printf("\n");
        cases++;
    }
    return 0;
}
