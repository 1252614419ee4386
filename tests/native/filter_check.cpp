// Host-side driver of csrc/filter.h for tests/test_filter_cpu.py (no GPU, no HIP).
// It reads cases from stdin until it ends.  Every float travels as the hexadecimal bit pattern of its f32 value, so that inf, NaN and
// -0.0 arrive unchanged.  The cases:
//     constants                         prints FILTER_TILE FILTER_MAX_TAPS FILTER_PARAM_STRIDE and the default edges
//     apply S cap L                     S span samples, cap >= S samples of capacity, L taps (0: taps == NULL, a copy)
//       L floats, cap floats            the taps, the waveform
//                                       prints cap floats, or "refused FIELD" where filter_check refuses; the parameter row must
//                                       give the taps back
//     design n_bands ne L               zv_filter_design's n_bands, the edges given (0: NULL), n_taps
//       ne integers, ng floats          the edges, the gains (ng = n_bands, or 16 where it is 0)
//                                       prints L floats, or "refused FIELD"
#include "filter.h"

#include <cstdio>
#include <cstring>
#include <vector>

static float from_bits(unsigned b)
{
    float f;
    memcpy(&f, &b, 4);
    return f;
}

static bool read_floats(std::vector<float> &v)
{
    for (float &f : v)
    {
        unsigned b = 0;
        if (scanf("%x", &b) != 1) return false;
        f = from_bits(b);
    }
    return true;
}

int main()
{
    char word[32];
    long cases = 0;
    while (scanf("%31s", word) == 1)
    {
        if (!strcmp(word, "constants"))
        {
            printf("%d %u %d", zv::FILTER_TILE, zv::FILTER_MAX_TAPS, zv::FILTER_PARAM_STRIDE);
            for (uint32_t e : zv::FILTER_DEFAULT_EDGES) printf(" %u", e);
            printf("\n");
        }
        else if (!strcmp(word, "apply"))
        {
            long S, cap;
            unsigned L;
            if (scanf("%ld %ld %u", &S, &cap, &L) != 3 || S < 0 || cap < S || cap > (1 << 24) || L > 4096) return fprintf(stderr, "case %ld: bad header\n", cases), 2;
            std::vector<float> h(L), x((size_t)cap), y((size_t)cap);
            if (!read_floats(h) || !read_floats(x)) return fprintf(stderr, "case %ld: short case\n", cases), 2;
            if (const char *field = zv::filter_check(L ? h.data() : nullptr, L))
            {
                printf("refused %s\n", field);
                cases++;
                continue;
            }
            uint32_t row[zv::FILTER_PARAM_STRIDE];
            zv::filter_pack(L ? h.data() : nullptr, L, row);
            if (row[0] != L || (L && memcmp(row + 1, h.data(), (size_t)L * 4) != 0)) return fprintf(stderr, "case %ld: the parameter row differs\n", cases), 2;
            zv::filter_reference(x.data(), (uint64_t)S, (uint64_t)cap, L ? h.data() : nullptr, L, y.data());
            for (float v : y) printf("%x ", zv::level_bits(v));
            printf("\n");
        }
        else if (!strcmp(word, "design"))
        {
            unsigned nb, ne, L;
            if (scanf("%u %u %u", &nb, &ne, &L) != 3 || ne > 4096) return fprintf(stderr, "case %ld: bad header\n", cases), 2;
            std::vector<uint32_t> edges(ne);
            for (uint32_t &e : edges)
                if (scanf("%u", &e) != 1) return fprintf(stderr, "case %ld: short edges\n", cases), 2;
            std::vector<float> g(nb && nb <= 4096 ? nb : zv::FILTER_BANDS_DEFAULT), taps(L ? L : 1);
            if (!read_floats(g)) return fprintf(stderr, "case %ld: short gains\n", cases), 2;
            // (the test sends as many edges and gains as the count asks for; a count the design refuses reads none of them)
            if (const char *field = zv::filter_design(nb, ne ? edges.data() : nullptr, g.data(), L, taps.data()))
                printf("refused %s\n", field);
            else
            {
                for (unsigned k = 0; k < L; k++) printf("%x ", zv::level_bits(taps[k]));
                printf("\n");
            }
        }
        else
            return fprintf(stderr, "case %ld: unknown case %s\n", cases, word), 2;
        cases++;
    }
    return 0;
}
