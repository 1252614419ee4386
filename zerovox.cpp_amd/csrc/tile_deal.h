// tile_deal.h — which time tile a workgroup of the ResBlock kernels (conv1d_mfma.hip) works on.  Plain integer arithmetic
// shared by the kernels, their launchers and the host-side test (tests/native/tile_deal_check.cpp): nothing here needs HIP.
#pragma once

#if defined(__HIPCC__)
#define ZV_TD_FN __host__ __device__ static inline
#else
#define ZV_TD_FN static inline
#endif

namespace zv
{

// Workgroups are dealt round-robin over the 8 XCDs (observed, not promised: only the speed depends on it) and each XCD has
// its own L2: with grid.x a multiple of 8, workgroup b runs on XCD b & 7, and dispatch is in order — a launch lasts as long as
// its busiest XCD.

// One segment: XCD x gets the x-th contiguous eighth of the ntiles time tiles, so that neighbouring tiles — which share
// their halo rows — sit behind the same L2.  Workgroups beyond the tiles get ntiles (dead).  grid.x = round_up(ntiles, 8).
ZV_TD_FN int tile_deal_contiguous(int b, int ntiles)
{
#ifdef ZV_NO_XCD_MAP
    return b < ntiles ? b : ntiles;
#else
    const int per = (ntiles + 7) >> 3, idx = b >> 3;
    return idx < per ? (b & 7) * per + idx : ntiles;
#endif
}

// Several segments.  A launch's tile space is sized by capacity (nseg x tps tiles, tps from the segments' max_rows) but only
// the first tiles of each segment are live (run table, fitted mode: Seg::rows), so contiguous eighths of the capacity give
// some XCDs whole long utterances and others mostly dead tiles.  Instead every segment is dealt over all 8 XCDs in chunks of
// c consecutive tiles (a chunk shares its halo rows behind one L2), chunk k of segment u to XCD (k + u * ROT) & 7: live
// tiles are a prefix of every segment, so each XCD gets its share of them whatever the segments' lengths, and the rotation
// keeps the remainder chunks of equal-length segments from piling onto the same XCDs.  A segment's capacity is padded to
// S = ceil(tps / 8c) * c slots per XCD, which makes the inverse closed-form: workgroup b = (idx, x), idx = b >> 3,
// x = b & 7, works on segment idx / S, and with r = idx % S on chunk (r / c) * 8 + ((x - rot) & 7), tile chunk * c + r % c.
constexpr int TILE_DEAL_ROT = 3;      // odd: 8 consecutive segments start on 8 different XCDs

ZV_TD_FN int tile_deal_slots(int tps, int c) { return (tps + 8 * c - 1) / (8 * c) * c; }

// grid.x of a launch whose job with the most tiles per segment has tps of them
ZV_TD_FN int tile_deal_grid(int tps, int nseg, int c) { return nseg == 1 ? (tps + 7) / 8 * 8 : 8 * tile_deal_slots(tps, c) * nseg; }

// workgroup b -> tile index in [0, nseg * tps) (segment = index / tps), or nseg * tps for a workgroup with nothing to do
ZV_TD_FN int tile_deal(int b, int tps, int nseg, int c)
{
    const int ntiles = tps * nseg;
    if (nseg == 1) return tile_deal_contiguous(b, ntiles);
#ifdef ZV_NO_XCD_MAP
    return b < ntiles ? b : ntiles;
#else
    const int S = tile_deal_slots(tps, c), x = b & 7, idx = b >> 3;
    const int useg = idx / S;
    if (useg >= nseg) return ntiles;
    const int r = idx - useg * S;
    const int tile = ((r / c) * 8 + ((x - useg * TILE_DEAL_ROT) & 7)) * c + r % c;
    return tile < tps ? useg * tps + tile : ntiles;
#endif
}

// Chunk length per stage, by the stage's (padded) channel count: measured on the batch of 32 x 1 024 frames, candidates
// 1, 2, 4, 8 (DESIGN.md "Tiles dealt by live rows").  A longer chunk keeps more halo rows behind one L2, a shorter one
// balances better where an utterance has only a few dozen tiles (256 channels).
#ifndef ZV_DEAL_C256
#define ZV_DEAL_C256 4
#endif
#ifndef ZV_DEAL_C128
#define ZV_DEAL_C128 8
#endif
#ifndef ZV_DEAL_C64
#define ZV_DEAL_C64 1
#endif
#ifndef ZV_DEAL_C32
#define ZV_DEAL_C32 4
#endif
ZV_TD_FN int tile_deal_chunk(int Cp) { return Cp >= 256 ? ZV_DEAL_C256 : (Cp == 128 ? ZV_DEAL_C128 : (Cp == 64 ? ZV_DEAL_C64 : ZV_DEAL_C32)); }

}  // namespace zv
