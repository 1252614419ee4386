// wave_stages.h — the waveform stages behind the vocoder's output convolution (volume, envelope, contour, pitch track, band levels,
// filter) as the host plumbs them: which stages a request turns on, the regions each owns in the I/O blocks, and the device pointers a
// Batch carries for them.  Pure (no HIP, no model): tests/native/wave_stages_check.cpp checks every decision on the CPU.
// ADDING A STAGE: a WaveStageId, its WaveArgs member and rule in ask(), its pointers in WaveStages, its rows in WAVE_REGIONS; then its
// own check and pack (capi.cpp), its launch block (wave_stages.cpp) and its public entry points.  Nothing else names a stage.
#pragma once

#include <array>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <type_traits>

#include "../../include/zerovox_amd.h"
#include "bands.h"
#include "contour.h"
#include "envelope.h"
#include "filter.h"
#include "level.h"
#include "pitch.h"

namespace zv
{

// every region of an arena or an I/O block starts on a 256-byte boundary (DeviceArena::take, Layout::at)
constexpr size_t region_align(size_t off) { return (off + 255) & ~(size_t)255; }

// the layout of an I/O block (io_scratch, pinned_scratch): regions in the order they are carved; size() covers every region handed out
struct Layout
{
    size_t end = 0;
    size_t at(size_t bytes)
    {
        const size_t o = region_align(end);
        end = o + bytes;
        return o;
    }
    size_t size() const { return region_align(end); }
};

enum WaveStageId { WS_VOLUME, WS_ENVELOPE, WS_CONTOUR, WS_PITCH, WS_BANDS, WS_FILTER, WS_COUNT };      // in the order of their regions

// what a request wants: which stages are on and, for the stages that hand tables back, whether any utterance asks for its frame rows /
// its phoneme rows (a staging table exists only then)
struct WaveAsk
{
    bool on[WS_COUNT] = {}, frames[WS_COUNT] = {}, phonemes[WS_COUNT] = {};
    // an envelope's knots pass and a table stage's phonemes pass read the regulator's scan behind the vocoder: Batch::d_cum must be set
    bool needs_scan() const { return on[WS_ENVELOPE] || on[WS_CONTOUR] || on[WS_PITCH] || on[WS_BANDS]; }
};

// A request's stage arguments, [count] each or null (include/zerovox_amd.h), in the entry points' argument order: a Request's positional
// initialiser runs on into this aggregate.
struct WaveArgs
{
    const zv_volume   *volume = nullptr;        // or null with levels: a meter, every gain 1
    zv_level          *levels = nullptr;
    const zv_envelope *envelope = nullptr;      // each phoneme_gain is [n[u]] or null
    const zv_contour  *contour = nullptr;       // each struct's tables are [T[u]] and [n[u]] or null
    const zv_pitch    *pitch = nullptr;         // likewise; parameters 0 = default
    const zv_bands    *bands = nullptr;         // tables [T[u]][n_bands] and [n[u]][n_bands] or null
    const zv_filter   *filter = nullptr;        // taps [n_taps] or null = no filter for that utterance

    WaveArgs slice(uint32_t a) const      // the arguments of utterances a, a + 1, ...
    {
        return WaveArgs{volume ? volume + a : volume,       levels ? levels + a : levels,    envelope ? envelope + a : envelope,
                        contour ? contour + a : contour,    pitch ? pitch + a : pitch,       bands ? bands + a : bands,
                        filter ? filter + a : filter};
    }
    // Each feature's own rule.  Volume: the call measures levels (every utterance gets a volume row, the identity where none is given).
    // Envelope: the call carries the array.  Contour, pitch, bands: some utterance asks for a table (the rows of both tables are written,
    // the host downloads what was asked for).  Filter: some utterance has taps (the others get n_taps = 0: their bits are copied).
    WaveAsk ask(uint32_t count) const
    {
        WaveAsk a;
        for (uint32_t u = 0; u < count; u++)
        {
            if (contour && contour[u].frames) a.frames[WS_CONTOUR] = true;
            if (contour && contour[u].phonemes) a.phonemes[WS_CONTOUR] = true;
            if (pitch && pitch[u].frames) a.frames[WS_PITCH] = true;
            if (pitch && pitch[u].phonemes) a.phonemes[WS_PITCH] = true;
            if (bands && bands[u].frames) a.frames[WS_BANDS] = true;
            if (bands && bands[u].phonemes) a.phonemes[WS_BANDS] = true;
            if (filter && filter[u].taps) a.on[WS_FILTER] = true;
        }
        for (int s : {WS_CONTOUR, WS_PITCH, WS_BANDS}) a.on[s] = a.frames[s] || a.phonemes[s];
        a.on[WS_VOLUME] = volume || levels;
        a.on[WS_ENVELOPE] = envelope != nullptr;
        return a;
    }
};

// The device pointers a Batch carries for the stages (HBM outside the arena), a stage's all set or none.  Every one keys a captured
// graph: its presence changes the launches, its value is a kernel argument; the VALUES behind them are read at run time, so a replay
// picks up new ones.  Pointers only, compared bytewise: a field added here is part of the key without another line anywhere.
struct WaveStages
{
    // volume controls (level.h): the volume rows, f32 [nseg][LEVEL_VOL_STRIDE], the level rows [nseg], the regulator's frame counts [nseg]
    const float   *d_vol = nullptr;
    LevelRow      *d_levels = nullptr;
    const int32_t *d_nframes = nullptr;
    // amplitude envelope (envelope.h): the per-phoneme gains, f32 [n_rows] by absolute token row, and the rows, int32 [nseg][ENV_CTL_STRIDE]
    const float   *d_env_gain = nullptr;
    const int32_t *d_env = nullptr;
    // level contour (contour.h): the frame rows [t_rows] and the phoneme rows [n_rows], by absolute frame row / token row, all written
    ContourRow *d_ctr_frames = nullptr, *d_ctr_phonemes = nullptr;
    // pitch track (pitch.h): the two tables likewise, and the parameter rows, uint32 [nseg][PITCH_PARAM_STRIDE], resolved on the host
    PitchFrameRow   *d_pit_frames = nullptr;
    PitchPhonemeRow *d_pit_phonemes = nullptr;
    const uint32_t  *d_pit_par = nullptr;
    // band levels (bands.h): the two tables likewise, f32 [..][BANDS_ROW_STRIDE], the kept powers the frames pass leaves for the phonemes
    // pass, u64 [t_rows][BANDS_ROW_STRIDE], the parameter rows, uint32 [nseg][BANDS_PARAM_STRIDE], and the twiddle table (Model::bands_table)
    float              *d_bnd_frames = nullptr, *d_bnd_phonemes = nullptr;
    unsigned long long *d_bnd_slab = nullptr;
    const uint32_t     *d_bnd_par = nullptr;
    const void         *d_bnd_table = nullptr;
    // waveform filter (filter.h): the parameter rows, uint32 [nseg][FILTER_PARAM_STRIDE]; with it VocLayout::filter_in is carved
    const uint32_t *d_flt_par = nullptr;

    bool operator==(const WaveStages &o) const { return memcmp(this, &o, sizeof(*this)) == 0; }
    bool needs_scan() const { return d_env || d_ctr_frames || d_pit_frames || d_bnd_frames; }
    // the "all set or none" rules the launches rest on, given the batch's scan (Batch::d_cum): null, or what is missing
    const char *inconsistent(const void *d_cum) const
    {
        if (d_env && (!d_cum || !d_nframes || !d_env_gain)) return "internal: an envelope without the scan, the frame counts or the gains";
        if (d_ctr_frames && (!d_cum || !d_ctr_phonemes)) return "internal: a contour without the scan or the phoneme rows";
        if (d_pit_frames && (!d_cum || !d_pit_phonemes || !d_pit_par))
            return "internal: a pitch track without the scan, the phoneme rows or the parameters";
        if (d_bnd_frames && (!d_cum || !d_bnd_phonemes || !d_bnd_slab || !d_bnd_par || !d_bnd_table))
            return "internal: band levels without the scan, the phoneme rows, the slab, the parameters or the table";
        return nullptr;
    }
    WaveStages group(int g0) const;      // the pointers of a tail sub-batch that starts at segment g0 (Model::vocode_tail): below
};
static_assert(std::is_trivially_copyable<WaveStages>::value && std::has_unique_object_representations<WaveStages>::value,
              "WaveStages is pointers only, without padding: its bytes are the graph key");

// ---- the region plan: a region holds one row per utterance, per token row or per frame row of its block's row space
enum WaveRowKind { ROWS_UTTERANCE, ROWS_TOKEN, ROWS_FRAME };
// WR_INPUT: packed on the host and uploaded with the call's input.  WR_DEVICE: written on the device.  WR_HOST: the host's staging of a
// device region's rows in a batch's pinned block (a single utterance's rows go straight to the caller); per-utterance rows are staged
// with their stage, frame rows / phoneme rows only where some utterance asks for that table.
enum WaveRole { WR_INPUT = 1, WR_DEVICE = 2, WR_HOST = 4 };
enum WaveRegionId
{
    R_VOL, R_LEVELS, R_LEVELS_HOST, R_ENV_GAIN, R_ENV, R_CTR_FRAMES, R_CTR_PHONEMES, R_CTR_FRAMES_HOST, R_CTR_PHONEMES_HOST,
    R_PIT_FRAMES, R_PIT_PHONEMES, R_PIT_FRAMES_HOST, R_PIT_PHONEMES_HOST, R_PIT_PAR,
    R_BND_FRAMES, R_BND_PHONEMES, R_BND_SLAB, R_BND_FRAMES_HOST, R_BND_PHONEMES_HOST, R_BND_PAR, R_FLT_PAR, R_COUNT
};
// member: offsetof the WaveStages pointer that names an input or device region; device: the device region a staging region stages
struct WaveRegion { WaveStageId stage; WaveRowKind rows; size_t row_bytes; WaveRole role; size_t member; int device; };

// The regions in carving order: a block takes the ones of its roles, in this order (the order the features were added in, so no offset
// has moved since).  A region of a stage that is off is still carved, with zero bytes.
inline constexpr WaveRegion WAVE_REGIONS[R_COUNT] = {
    {WS_VOLUME, ROWS_UTTERANCE, LEVEL_VOL_STRIDE * 4, WR_INPUT, offsetof(WaveStages, d_vol), -1},
    {WS_VOLUME, ROWS_UTTERANCE, sizeof(LevelRow), WR_DEVICE, offsetof(WaveStages, d_levels), -1},
    {WS_VOLUME, ROWS_UTTERANCE, sizeof(LevelRow), WR_HOST, 0, R_LEVELS},
    {WS_ENVELOPE, ROWS_TOKEN, 4, WR_INPUT, offsetof(WaveStages, d_env_gain), -1},
    {WS_ENVELOPE, ROWS_UTTERANCE, ENV_CTL_STRIDE * 4, WR_INPUT, offsetof(WaveStages, d_env), -1},
    {WS_CONTOUR, ROWS_FRAME, sizeof(ContourRow), WR_DEVICE, offsetof(WaveStages, d_ctr_frames), -1},
    {WS_CONTOUR, ROWS_TOKEN, sizeof(ContourRow), WR_DEVICE, offsetof(WaveStages, d_ctr_phonemes), -1},
    {WS_CONTOUR, ROWS_FRAME, sizeof(ContourRow), WR_HOST, 0, R_CTR_FRAMES},
    {WS_CONTOUR, ROWS_TOKEN, sizeof(ContourRow), WR_HOST, 0, R_CTR_PHONEMES},
    {WS_PITCH, ROWS_FRAME, sizeof(PitchFrameRow), WR_DEVICE, offsetof(WaveStages, d_pit_frames), -1},
    {WS_PITCH, ROWS_TOKEN, sizeof(PitchPhonemeRow), WR_DEVICE, offsetof(WaveStages, d_pit_phonemes), -1},
    {WS_PITCH, ROWS_FRAME, sizeof(PitchFrameRow), WR_HOST, 0, R_PIT_FRAMES},
    {WS_PITCH, ROWS_TOKEN, sizeof(PitchPhonemeRow), WR_HOST, 0, R_PIT_PHONEMES},
    {WS_PITCH, ROWS_UTTERANCE, PITCH_PARAM_STRIDE * 4, WR_INPUT, offsetof(WaveStages, d_pit_par), -1},
    {WS_BANDS, ROWS_FRAME, BANDS_ROW_STRIDE * 4, WR_DEVICE, offsetof(WaveStages, d_bnd_frames), -1},
    {WS_BANDS, ROWS_TOKEN, BANDS_ROW_STRIDE * 4, WR_DEVICE, offsetof(WaveStages, d_bnd_phonemes), -1},
    {WS_BANDS, ROWS_FRAME, BANDS_ROW_STRIDE * 8, WR_DEVICE, offsetof(WaveStages, d_bnd_slab), -1},
    {WS_BANDS, ROWS_FRAME, BANDS_ROW_STRIDE * 4, WR_HOST, 0, R_BND_FRAMES},
    {WS_BANDS, ROWS_TOKEN, BANDS_ROW_STRIDE * 4, WR_HOST, 0, R_BND_PHONEMES},
    {WS_BANDS, ROWS_UTTERANCE, BANDS_PARAM_STRIDE * 4, WR_INPUT, offsetof(WaveStages, d_bnd_par), -1},
    {WS_FILTER, ROWS_UTTERANCE, FILTER_PARAM_STRIDE * 4, WR_INPUT, offsetof(WaveStages, d_flt_par), -1},
};

// the rows of a block's row space, by WaveRowKind: a batch's device blocks go by capacity {nseg, n_rows, t_rows}, its staging block by
// what the utterances hold {their count, the sum of their phonemes, the sum of their frames}; a single utterance's block is {1, n, T}
using WaveRows = std::array<size_t, 3>;

inline bool wave_region_exists(const WaveRegion &g, const WaveAsk &ask)
{
    const bool asked = g.role != WR_HOST || g.rows == ROWS_UTTERANCE || (g.rows == ROWS_FRAME ? ask.frames[g.stage] : ask.phonemes[g.stage]);
    return ask.on[g.stage] && asked;
}
inline size_t wave_region_bytes(int id, const WaveAsk &ask, const WaveRows &rows)
{
    const WaveRegion &g = WAVE_REGIONS[id];
    return wave_region_exists(g, ask) ? rows[g.rows] * g.row_bytes : 0;
}

// where the regions start in the blocks that hold them: each block's carve fills in the regions of its roles
struct WaveOffsets { size_t at[R_COUNT] = {}; };
// Appends the regions of `roles` to a block's layout, in order: a batch's input, device and staging blocks one role each; a single
// utterance's one block WR_INPUT | WR_DEVICE, which is the batch's two at nseg = 1, n_rows = n, t_rows = T.
inline void wave_carve(Layout &L, const WaveAsk &ask, const WaveRows &rows, int roles, WaveOffsets &o)
{
    for (int id = 0; id < R_COUNT; id++)
        if (WAVE_REGIONS[id].role & roles) o.at[id] = L.at(wave_region_bytes(id, ask, rows));
}

// The pointers of a call: every input region of an on stage at `in` + its offset, every device region at `dev` + its offset (a single
// utterance: the same block twice), the frame counts for the stages that read them and the twiddle table for the one that does.
inline WaveStages wave_bind(const WaveAsk &ask, const WaveOffsets &o, char *in, char *dev, const int32_t *d_nframes, const void *bands_table)
{
    WaveStages w;
    for (int id = 0; id < R_COUNT; id++)
    {
        const WaveRegion &g = WAVE_REGIONS[id];
        if (g.role == WR_HOST || !ask.on[g.stage]) continue;
        const char *p = (g.role == WR_INPUT ? in : dev) + o.at[id];
        memcpy((char *)&w + g.member, &p, sizeof(p));
    }
    if (ask.on[WS_VOLUME] || ask.on[WS_ENVELOPE]) w.d_nframes = d_nframes;
    if (ask.on[WS_BANDS]) w.d_bnd_table = bands_table;
    return w;
}

// Per-utterance tables (the frame counts among them) advance by g0 rows of their stride; tables indexed by absolute frame row or
// token row do not move, nor does the twiddle table.
inline WaveStages WaveStages::group(int g0) const
{
    WaveStages s = *this;
    for (int id = 0; id < R_COUNT; id++)
    {
        const WaveRegion &g = WAVE_REGIONS[id];
        if (g.role == WR_HOST || g.rows != ROWS_UTTERANCE) continue;
        const char *p;
        memcpy(&p, (const char *)&s + g.member, sizeof(p));
        if (p) p += (size_t)g0 * g.row_bytes;
        memcpy((char *)&s + g.member, &p, sizeof(p));
    }
    if (d_nframes) s.d_nframes = d_nframes + g0;
    return s;
}

}  // namespace zv
