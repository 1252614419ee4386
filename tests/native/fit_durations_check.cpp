// Host-side driver of csrc/fit_durations.h for tests/test_fit_durations_cpu.py (no GPU, no HIP).
// Reads cases from stdin until it ends, each three lines:
//     n num_phonemes T target has_forced
//     n durations as the hexadecimal bit patterns of their f32 values (so that inf and NaN travel unchanged)
//     n forced frame counts (-1 = free); the line is empty when has_forced is 0 (the reference then gets forced == NULL)
// and prints one line per case: the n frame counts d[i] of zv::fit_durations.
#include "fit_durations.h"

#include <cstdio>
#include <cstring>
#include <vector>

int main()
{
    int n, num_phonemes, T, target, has_forced;
    long cases = 0;
    while (scanf("%d %d %d %d %d", &n, &num_phonemes, &T, &target, &has_forced) == 5)
    {
        if (n < 0 || n > (1 << 20)) return fprintf(stderr, "case %ld: bad n %d\n", cases, n), 2;
        std::vector<float> dur(n);
        std::vector<int32_t> forced(n), d(n, -7);
        for (int i = 0; i < n; i++)
        {
            unsigned bits = 0;
            if (scanf("%x", &bits) != 1) return fprintf(stderr, "case %ld: short duration line\n", cases), 2;
            memcpy(&dur[i], &bits, 4);
        }
        for (int i = 0; has_forced && i < n; i++)
            if (scanf("%d", &forced[i]) != 1) return fprintf(stderr, "case %ld: short forced line\n", cases), 2;
        zv::fit_durations(dur.data(), has_forced ? forced.data() : nullptr, n, num_phonemes, T, target, d.data());
        for (int i = 0; i < n; i++) printf("%d%c", d[i], i + 1 == n ? '\n' : ' ');
        if (n == 0) printf("\n");
        cases++;
    }
    return 0;
}
