// conv_xcd.h — which (row tile, channel group) a workgroup of conv1d_mfma_kernel's loader-wave form (conv.hip) works on when the
// launch is dealt over the XCDs.  Plain integer arithmetic shared by the kernel, its launch plan (conv_plan.h) and the host-side
// test (tests/native/conv_xcd_check.cpp): nothing here needs HIP.
#pragma once

#if defined(__HIPCC__)
#define ZV_CX_FN __host__ __device__ static inline
#else
#define ZV_CX_FN static inline
#endif

namespace zv
{

// As in tile_deal.h: with grid.x a multiple of 8, workgroup b runs on XCD b & 7 (observed, not promised: only the speed depends
// on it), each XCD has its own L2, and a launch lasts as long as its busiest XCD.
//
// A launch has nx row tiles (all segments' capacity) x ny channel groups.  Every row tile of a channel group walks the same
// weight stream, so a group wants ONE L2 to hold it:
//
//   group map (spread = 0, or ny >= 8): XCD k holds the groups k, k + 8, ...; slot q = b >> 3 of XCD k is
//       (row tile q % nx, group k + 8 (q / nx)).  grid.x = 8 nx ceil(ny / 8).  With ny < 8 the XCDs ny .. 7 get dead workgroups
//       only: right for one utterance (a handful of row tiles per group, latency-bound on the weights), wrong for a batch, whose
//       hundreds of row tiles then queue on ny XCDs.
//   spread map (spread = 1 and ny < 8): group g owns the p = conv_xcd_spread(ny) XCDs g p .. g p + p - 1 and its row tile t
//       goes to XCD g p + t % p, slot t / p.  grid.x = 8 ceil(nx / p).  The group's weights then sit in p L2s instead of one;
//       the XCDs ny p .. 7 (ny = 3, 5, 6, 7) stay empty as before.
// The launcher asks for the spread map where a launch has several segments.

// XCDs a channel group is dealt over: 8 / 4 / 2 / 1 for ny = 1 / 2 / 3-4 / 5 and more
ZV_CX_FN int conv_xcd_spread(int ny) { return ny <= 1 ? 8 : (ny == 2 ? 4 : (ny <= 4 ? 2 : 1)); }

// grid.x of the launch
ZV_CX_FN int conv_xcd_grid(int nx, int ny, int spread)
{
    if (!spread || ny >= 8) return 8 * nx * ((ny + 7) / 8);
    const int p = conv_xcd_spread(ny);
    return 8 * ((nx + p - 1) / p);
}

// What a workgroup works on: row tile bx of nx, channel group by of ny; on its XCD it is row tile `part` of the `nparts` its
// group has there (l2_warm: together they touch the group's weights once per L2).
struct ConvXcdSlot
{
    int bx, by, part, nparts;
};

// workgroup b -> slot; false for a workgroup with nothing to do
ZV_CX_FN bool conv_xcd_slot(int b, int nx, int ny, int spread, ConvXcdSlot &s)
{
    const int x = b & 7, q = b >> 3;
    if (!spread || ny >= 8)
    {
        const int g = q / nx;
        s.by = x + 8 * g;
        s.bx = q - g * nx;
        s.part = s.bx;
        s.nparts = nx;
        return s.by < ny;
    }
    const int p = conv_xcd_spread(ny), g = x / p, r = x - g * p;
    s.by = g;
    s.bx = q * p + r;
    s.part = q;
    s.nparts = (nx - r + p - 1) / p;        // row tiles t < nx with t % p == r
    return g < ny && s.bx < nx;
}

}  // namespace zv
