// Host-side driver of csrc/conv_xcd.h for tests/test_conv_xcd_cpu.py (no GPU, no HIP).
//   conv_xcd_check NY_LO NY_HI NX_LO NX_HI
//       for every (ny, nx), with the spread map on and off:
//         * grid.x is a multiple of 8; every (bx, by) of the nx x ny space is produced exactly once, every other workgroup is dead
//           (also past the grid: a dead workgroup stays dead);
//         * ny >= 8, or the spread map off: the map is the closed form the kernel had before the header existed, written out below;
//         * ny < 8, spread on: channel group g sits on the p XCDs g p .. g p + p - 1 (p = 8 / 4 / 2 / 1 for ny = 1 / 2 / 3-4 / 5-7)
//           and on no other, the XCDs with live work number ny min(p, nx) — which is min(8, ny p) as soon as a group has p row
//           tiles — and the live counts of a group's XCDs differ by at most one;
//         * (part, nparts) numbers the row tiles a group has on one XCD 0 .. nparts - 1, each once.
//       Prints "ok <cases>".
#include "conv_xcd.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace zv;

#define FAIL(...) return printf(__VA_ARGS__), printf(" at ny %d nx %d spread %d\n", ny, nx, spread), 1

static int check(int ny, int nx, int spread)
{
    const int grid = conv_xcd_grid(nx, ny, spread);
    if (grid <= 0 || grid % 8) FAIL("grid %d", grid);
    const bool fresh = spread && ny < 8;
    const int p = ny <= 1 ? 8 : (ny == 2 ? 4 : (ny <= 4 ? 2 : 1));
    if (conv_xcd_spread(ny) != p) FAIL("p %d, expected %d", conv_xcd_spread(ny), p);
    if (!fresh && grid != 8 * nx * ((ny + 7) / 8)) FAIL("grid %d differs from the group map's", grid);
    if (fresh && grid != 8 * ((nx + p - 1) / p)) FAIL("grid %d differs from 8 ceil(nx / p)", grid);
    std::vector<int> seen((size_t)nx * ny, 0), parts;
    std::vector<long> live(8 * (size_t)ny, 0);          // [group][xcd]
    for (int b = 0; b < grid + 64; b++)
    {
        ConvXcdSlot s = {-1, -1, -1, -1};
        const bool ok = conv_xcd_slot(b, nx, ny, spread, s);
        if (!fresh)
        {
            // the closed form of the group map: q = b >> 3, g = q / nx, by = (b & 7) + 8 g, bx = q - g nx, dead when by >= ny
            const int q = b >> 3, g = q / nx, by = (b & 7) + 8 * g, bx = q - g * nx;
            if (ok != (by < ny) || (ok && (s.bx != bx || s.by != by))) FAIL("workgroup %d: (%d, %d) %d, closed form (%d, %d) %d", b, s.bx, s.by, ok, bx, by, by < ny);
        }
        if (!ok) continue;
        if (b >= grid) FAIL("live workgroup %d beyond the grid %d", b, grid);
        if (s.bx < 0 || s.bx >= nx || s.by < 0 || s.by >= ny) FAIL("workgroup %d: (%d, %d) out of range", b, s.bx, s.by);
        seen[(size_t)s.by * nx + s.bx]++;
        live[(size_t)s.by * 8 + (b & 7)]++;
        if (s.nparts < 1 || s.part < 0 || s.part >= s.nparts) FAIL("workgroup %d: part %d of %d", b, s.part, s.nparts);
        if (fresh)
        {
            if ((b & 7) != s.by * p + s.bx % p) FAIL("workgroup %d: row tile %d of group %d on XCD %d", b, s.bx, s.by, b & 7);
            if ((b >> 3) != s.bx / p) FAIL("workgroup %d: row tile %d in slot %d", b, s.bx, b >> 3);
        }
    }
    for (size_t i = 0; i < seen.size(); i++)
        if (seen[i] != 1) FAIL("(%d, %d) produced %d times", (int)(i % nx), (int)(i / nx), seen[i]);
    // parts: per (group, XCD) the parts 0 .. nparts - 1 once each and nparts = the live count there
    std::vector<size_t> base(live.size() + 1, 0);
    for (size_t k = 0; k < live.size(); k++) base[k + 1] = base[k] + (size_t)live[k];
    parts.assign(base.back(), 0);
    for (int b = 0; b < grid; b++)
    {
        ConvXcdSlot s;
        if (!conv_xcd_slot(b, nx, ny, spread, s)) continue;
        const size_t k = (size_t)s.by * 8 + (b & 7);
        if (s.nparts != live[k]) FAIL("workgroup %d: nparts %d, its group has %ld row tiles on XCD %d", b, s.nparts, live[k], b & 7);
        if (parts[base[k] + s.part]++) FAIL("part %d of group %d on XCD %d taken twice", s.part, s.by, b & 7);
    }
    if (fresh)
    {
        int used = 0;
        for (int x = 0; x < 8; x++)
        {
            long any = 0;
            for (int g = 0; g < ny; g++) any += live[(size_t)g * 8 + x];
            used += any > 0;
        }
        const int want = ny * (p < nx ? p : nx);
        if (used != want) FAIL("%d XCDs with live work, expected %d", used, want);
        if (nx >= p && used != (8 < ny * p ? 8 : ny * p)) FAIL("%d XCDs with live work, expected min(8, ny p)", used);
        for (int g = 0; g < ny; g++)
        {
            long lo = nx, hi = 0;
            for (int x = 0; x < 8; x++)
            {
                const long n = live[(size_t)g * 8 + x];
                const bool own = x >= g * p && x < g * p + p;
                if (!own && n) FAIL("group %d has %ld row tiles on XCD %d", g, n, x);
                if (own) lo = n < lo ? n : lo, hi = n > hi ? n : hi;
            }
            if (hi - lo > 1) FAIL("group %d: %ld .. %ld row tiles per XCD", g, lo, hi);
        }
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 5)
    {
        fprintf(stderr, "usage: see the head of tests/native/conv_xcd_check.cpp\n");
        return 2;
    }
    long cases = 0;
    for (int ny = atoi(argv[1]); ny <= atoi(argv[2]); ny++)
        for (int nx = atoi(argv[3]); nx <= atoi(argv[4]); nx++)
            for (int spread = 0; spread < 2; spread++, cases++)
                if (check(ny, nx, spread)) return 1;
    printf("ok %ld\n", cases);
    return 0;
}
