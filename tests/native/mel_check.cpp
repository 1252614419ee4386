// Host-side driver of csrc/mel.h for tests/test_mel_cpu.py (no GPU, no HIP).
// `mel_check table FILE` writes the plain tables [cos, sin][513][1024] as little-endian int16 to FILE, after checking that the kernel's
// image of them (mel_table_fragments) holds the high digit of every entry at mel_table_index(0, ...), the low digit at
// mel_table_index(1, ...) and zeros elsewhere, that no two entries share a place, and that the digits of every entry give it back.
// `mel_check ln` reads f64 bit patterns (hexadecimal) from stdin and prints the bit pattern of mel_ln of each.
// `mel_check design RATE M FMIN FMAX` (the floats as f32 bit patterns) prints "refused FIELD" or the M * 513 weights' bit patterns.
// `mel_check plan` reads lines "max_rows nseg hop num_mels" and prints "ok frames_gx rows_gx gy" of stage_plan.h's mel_plan for each.
// Without arguments it reads cases from stdin until it ends.  Every float travels as the hexadecimal bit pattern of its f32 value, so
// that inf, NaN and -0.0 arrive unchanged.  A case:
//     T hop M rate centre pad log floor fmin fmax nw     (nw: 0 = weights NULL, the design; else M * 513)
//     nw floats                                           the weights
//     T * hop floats                                      the waveform
// and prints one line per case: the T * M row entries' bit patterns, or "refused FIELD" where mel_resolve refuses.
#include "mel.h"
#include "stage_plan.h"

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
    const std::vector<int16_t> tab = zv::mel_tables();
    const std::vector<int8_t> img = zv::mel_table_fragments(tab);
    if (img.size() != zv::MEL_TABLE_BYTES) return fprintf(stderr, "image size\n"), 2;
    std::vector<uint8_t> seen(img.size(), 0);
    for (int trig = 0; trig < 2; trig++)
        for (int k = 0; k < zv::BANDS_BINS; k++)
            for (int t = 0; t < zv::BANDS_N; t++)
            {
                const int v = tab[((size_t)trig * zv::BANDS_BINS + k) * zv::BANDS_N + t];
                int32_t hi, lo;
                zv::bands_digits(v, hi, lo);
                if (v < -zv::MEL_SCALE || v > zv::MEL_SCALE || 128 * hi + lo != v || hi < -64 || hi > 64 || lo < -64 || lo > 64)
                    return fprintf(stderr, "entry %d %d %d = %d: digits %d %d\n", trig, k, t, v, hi, lo), 2;
                for (int plane = 0; plane < 2; plane++)
                {
                    const size_t at = zv::mel_table_index(plane, trig, k, t);
                    if (at >= img.size() || seen[at]) return fprintf(stderr, "index %d %d %d %d out of range or taken twice\n", plane, trig, k, t), 2;
                    seen[at] = 1;
                    if (img[at] != (plane ? lo : hi)) return fprintf(stderr, "image differs at %d %d %d %d\n", plane, trig, k, t), 2;
                }
            }
    for (size_t i = 0; i < img.size(); i++)
        if (!seen[i] && img[i] != 0) return fprintf(stderr, "image not zero at %zu\n", i), 2;
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(tab.data(), 2, tab.size(), f) != tab.size() || fclose(f) != 0) return fprintf(stderr, "cannot write %s\n", path), 2;
    return 0;
}

static int ln_mode()
{
    unsigned long long b;
    while (scanf("%llx", &b) == 1)
    {
        const double r = zv::mel_ln(zv::mel_from_bits(b));
        unsigned long long o;
        memcpy(&o, &r, 8);
        printf("%llx\n", o);
    }
    return 0;
}

static int design_mode(char **argv)
{
    const unsigned rate = (unsigned)strtoul(argv[0], nullptr, 10), M = (unsigned)strtoul(argv[1], nullptr, 10);
    const float fmin = from_bits((unsigned)strtoul(argv[2], nullptr, 16)), fmax = from_bits((unsigned)strtoul(argv[3], nullptr, 16));
    std::vector<float> w((size_t)(M && M <= zv::MEL_MAX_MELS ? M : 1) * zv::BANDS_BINS);
    if (const char *field = zv::mel_design(rate, M, fmin, fmax, w.data())) return printf("refused %s\n", field), 0;
    for (float v : w) printf("%x ", zv::level_bits(v));
    printf("\n");
    return 0;
}

static int plan_mode()
{
    int rows, nseg, hop, M;
    while (scanf("%d %d %d %d", &rows, &nseg, &hop, &M) == 4)
    {
        const zv::MelPlan p = zv::mel_plan(rows, nseg, hop, M);
        printf("%d %d %d %d\n", (int)p.ok, p.frames_gx, p.rows_gx, p.gy);
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 3 && !strcmp(argv[1], "table")) return table_mode(argv[2]);
    if (argc == 2 && !strcmp(argv[1], "ln")) return ln_mode();
    if (argc == 6 && !strcmp(argv[1], "design")) return design_mode(argv + 2);
    if (argc == 2 && !strcmp(argv[1], "plan")) return plan_mode();
    const std::vector<int16_t> tab = zv::mel_tables();
    long cases = 0;
    int T, hop;
    unsigned M, rate, centre, pad, log, floor, fmin, fmax, nw;
    while (scanf("%d %d %u %u %u %u %u %x %x %x %u", &T, &hop, &M, &rate, &centre, &pad, &log, &floor, &fmin, &fmax, &nw) == 11)
    {
        if (T < 1 || hop < 1 || (int64_t)T * hop > (1 << 26) || (nw && (M > zv::MEL_MAX_MELS || nw != M * (unsigned)zv::BANDS_BINS)))
            return fprintf(stderr, "case %ld: bad header\n", cases), 2;
        std::vector<float> W(nw), x((size_t)T * hop);
        for (std::vector<float> *v : {&W, &x})
            for (float &e : *v)
            {
                unsigned b = 0;
                if (scanf("%x", &b) != 1) return fprintf(stderr, "case %ld: short line\n", cases), 2;
                e = from_bits(b);
            }
        const zv::MelParams q{nw ? W.data() : nullptr, from_bits(fmin), from_bits(fmax), centre, pad, log, from_bits(floor)};
        std::vector<uint32_t> par;
        if (const char *field = zv::mel_resolve(q, rate, (uint32_t)hop, M, x.size(), par))
        {
            printf("refused %s\n", field);
            cases++;
            continue;
        }
        if (par.size() != zv::mel_par_words(M)) return fprintf(stderr, "case %ld: block size\n", cases), 2;
        std::vector<float> out((size_t)T * M);
        zv::mel_reference(x.data(), (uint32_t)T, (uint32_t)hop, par.data(), tab.data(), out.data());
        for (float v : out) printf("%x ", zv::level_bits(v));
        printf("\n");
        cases++;
    }
    if (!feof(stdin)) return fprintf(stderr, "case %ld: malformed header\n", cases), 2;
    return 0;
}
