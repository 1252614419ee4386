// Host-side driver of csrc/bands.h for tests/test_bands_cpu.py (no GPU, no HIP).
// `bands_check table FILE` writes the plain tables [cos, sin][513][1024] as signed bytes to FILE, after checking that the kernel's
// image of them (bands_table_fragments) holds every entry at bands_table_index and zeros elsewhere, that no two entries share a place,
// and that the digits of every quantised value give it back.
// Without arguments it reads cases from stdin until it ends.  Every float travels as the hexadecimal bit pattern of its f32 value,
// so that inf, NaN and -0.0 arrive unchanged.  A case:
//     T hop n n_bands ne            the capacity in frames, the hop, the tokens, zv_bands' n_bands, the edges given (0: NULL)
//     ne decimal integers           the edges
//     n decimal integers            the phoneme timings (n may be 0)
//     T * hop floats                the waveform
// and prints one line per case:
//     n_bands and the edges | per frame and band level:Eq | per phoneme and band level
// Eq decimal, the levels hexadecimal bit patterns; or "refused FIELD" where bands_resolve refuses.
#include "bands.h"

#include <cstdio>
#include <cstring>
#include <vector>

static float from_bits(unsigned b)
{
    float f;
    memcpy(&f, &b, 4);
    return f;
}

static int table_mode(const char *path)
{
    const std::vector<int8_t> tab = zv::bands_tables();
    const std::vector<int8_t> img = zv::bands_table_fragments(tab);
    if (img.size() != zv::BANDS_TABLE_BYTES) return fprintf(stderr, "image size\n"), 2;
    std::vector<uint8_t> seen(img.size(), 0);
    for (int trig = 0; trig < 2; trig++)
        for (int k = 0; k < zv::BANDS_BINS; k++)
            for (int t = 0; t < zv::BANDS_N; t++)
            {
                const size_t at = zv::bands_table_index(trig, k, t);
                if (at >= img.size() || seen[at]) return fprintf(stderr, "index %d %d %d out of range or taken twice\n", trig, k, t), 2;
                seen[at] = 1;
                if (img[at] != tab[((size_t)trig * zv::BANDS_BINS + k) * zv::BANDS_N + t]) return fprintf(stderr, "image differs at %d %d %d\n", trig, k, t), 2;
            }
    for (size_t i = 0; i < img.size(); i++)
        if (!seen[i] && img[i] != 0) return fprintf(stderr, "image not zero at %zu\n", i), 2;
    for (int32_t a = -zv::BANDS_Q_MAX; a <= zv::BANDS_Q_MAX; a++)
    {
        int32_t hi, lo;
        zv::bands_digits(a, hi, lo);
        if (128 * hi + lo != a || hi < -64 || hi > 64 || lo < -64 || lo > 64) return fprintf(stderr, "digits of %d: %d %d\n", a, hi, lo), 2;
    }
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(tab.data(), 1, tab.size(), f) != tab.size() || fclose(f) != 0) return fprintf(stderr, "cannot write %s\n", path), 2;
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 3 && !strcmp(argv[1], "table")) return table_mode(argv[2]);
    const std::vector<int8_t> tab = zv::bands_tables();
    long cases = 0;
    int T, hop, n;
    unsigned n_bands, ne;
    while (scanf("%d %d %d %u %u", &T, &hop, &n, &n_bands, &ne) == 5)
    {
        if (T < 1 || hop < 1 || n < 0 || ne > 4096 || (int64_t)T * hop > (1 << 26)) return fprintf(stderr, "case %ld: bad header\n", cases), 2;
        std::vector<uint32_t> edges(ne);
        std::vector<int32_t> dur(n);
        std::vector<float> w((size_t)T * hop);
        for (unsigned i = 0; i < ne; i++)
            if (scanf("%u", &edges[i]) != 1) return fprintf(stderr, "case %ld: short edges\n", cases), 2;
        for (int i = 0; i < n; i++)
            if (scanf("%d", &dur[i]) != 1) return fprintf(stderr, "case %ld: short timings\n", cases), 2;
        for (size_t i = 0; i < w.size(); i++)
        {
            unsigned b = 0;
            if (scanf("%x", &b) != 1) return fprintf(stderr, "case %ld: short sample line\n", cases), 2;
            w[i] = from_bits(b);
        }
        // (a caller's edges array holds n_bands + 1 entries, or 17 with n_bands 0; the test sends exactly what the count asks for)
        const unsigned need = (n_bands ? n_bands : zv::BANDS_DEFAULT) + 1;
        if (ne && n_bands <= zv::BANDS_MAX && ne != need) return fprintf(stderr, "case %ld: %u edges for n_bands %u\n", cases, ne, n_bands), 2;
        uint32_t par[zv::BANDS_PARAM_STRIDE];
        if (const char *field = zv::bands_resolve(n_bands, ne ? edges.data() : nullptr, par))
        {
            printf("refused %s\n", field);
            cases++;
            continue;
        }
        const uint32_t nb = par[0];
        printf("%u", nb);
        for (uint32_t b = 0; b <= nb; b++) printf(" %u", par[1 + b]);
        printf(" |");
        std::vector<float> frames((size_t)T * nb), phonemes((size_t)n * nb), row(nb);
        std::vector<uint64_t> eq(nb);
        zv::bands_reference(w.data(), (uint32_t)T, (uint32_t)hop, par, tab.data(), dur.data(), (uint32_t)n, frames.data(), n ? phonemes.data() : nullptr);
        for (int f = 0; f < T; f++)
        {
            zv::bands_frame_reference(w.data(), w.size(), (uint32_t)f, (uint32_t)hop, par, tab.data(), row.data(), eq.data());
            if (memcmp(row.data(), &frames[(size_t)f * nb], nb * 4) != 0) return fprintf(stderr, "case %ld: frame %d differs between the two references\n", cases, f), 2;
            for (uint32_t b = 0; b < nb; b++) printf(" %x:%llu", zv::level_bits(row[b]), (unsigned long long)eq[b]);
        }
        printf(" |");
        for (size_t i = 0; i < phonemes.size(); i++) printf(" %x", zv::level_bits(phonemes[i]));
        printf("\n");
        cases++;
    }
    if (!feof(stdin)) return fprintf(stderr, "case %ld: malformed header\n", cases), 2;
    return 0;
}
