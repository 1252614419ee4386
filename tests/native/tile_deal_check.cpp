// Host-side driver of csrc/tile_deal.h for tests/test_tile_deal_cpu.py (no GPU, no HIP).
//   tile_deal_check cover C NSEG_LO NSEG_HI TPS_LO TPS_HI
//       for every (nseg, tps): the launcher's grid gives every tile exactly once, every other workgroup a dead index, the tiles
//       of one chunk one XCD; a grid sized for a job with more tiles per segment only adds dead workgroups.  Prints "ok <cases>".
//   tile_deal_check load new|old C TM RATE T NSEG ROWS...
//       live tiles (ceil(rows * RATE / TM) of the ceil(T * RATE / TM) each segment has room for) per XCD, 8 numbers;
//       old = one contiguous eighth of the capacity per XCD, the map launches with one segment keep.
#include "tile_deal.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace zv;

static int cover(int c, int nlo, int nhi, int tlo, int thi)
{
    long cases = 0;
    std::vector<int> seen, xcd;
    for (int nseg = nlo; nseg <= nhi; nseg++)
        for (int tps = tlo; tps <= thi; tps++, cases++)
        {
            const int ntiles = nseg * tps, grid = tile_deal_grid(tps, nseg, c);
            const int grid_big = tile_deal_grid(tps + 1 + tps / 9, nseg, c);      // another job of the launch has more tiles
            if (grid % 8 || grid_big < grid) return printf("grid %d / %d at nseg %d tps %d\n", grid, grid_big, nseg, tps), 1;
            seen.assign(ntiles, 0);
            xcd.assign(ntiles, -1);
            for (int b = 0; b < grid_big; b++)
            {
                const int v = tile_deal(b, tps, nseg, c);
                if (v < 0 || v > ntiles) return printf("index %d out of range at nseg %d tps %d b %d\n", v, nseg, tps, b), 1;
                if (v == ntiles) continue;
                if (b >= grid) return printf("live workgroup %d beyond the job's grid %d at nseg %d tps %d\n", b, grid, nseg, tps), 1;
                seen[v]++;
                xcd[v] = b & 7;
            }
            for (int v = 0; v < ntiles; v++)
            {
                if (seen[v] != 1) return printf("tile %d seen %d times at nseg %d tps %d\n", v, seen[v], nseg, tps), 1;
                const int t = v % tps;
                if (nseg > 1 && t % c && xcd[v] != xcd[v - 1]) return printf("chunk of tile %d split at nseg %d tps %d\n", v, nseg, tps), 1;
            }
        }
    printf("ok %ld\n", cases);
    return 0;
}

static int load(bool fresh, int c, int TM, int rate, int T, int nseg, char **rows)
{
    std::vector<int> live(nseg);
    const int tps = (T * rate + TM - 1) / TM;
    for (int u = 0; u < nseg; u++) live[u] = (atoi(rows[u]) * rate + TM - 1) / TM;
    const int ntiles = nseg * tps, grid = fresh ? tile_deal_grid(tps, nseg, c) : (ntiles + 7) / 8 * 8;
    long per[8] = {0};
    for (int b = 0; b < grid; b++)
    {
        const int v = fresh ? tile_deal(b, tps, nseg, c) : tile_deal_contiguous(b, ntiles);
        if (v < ntiles && v % tps < live[v / tps]) per[b & 7]++;
    }
    for (int x = 0; x < 8; x++) printf("%ld%c", per[x], x == 7 ? '\n' : ' ');
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 7 && !strcmp(argv[1], "cover")) return cover(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]));
    if (argc > 8 && !strcmp(argv[1], "load") && argc == 8 + atoi(argv[7]))
        return load(!strcmp(argv[2], "new"), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), atoi(argv[7]), argv + 8);
    fprintf(stderr, "usage: see the head of tests/native/tile_deal_check.cpp\n");
    return 2;
}
