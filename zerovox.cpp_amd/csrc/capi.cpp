// capi.cpp — the extern "C" boundary declared in include/zerovox_amd.h.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <optional>
#include <string>
#include <thread>
#include <vector>

#include "common.h"
#include "model.h"
#include "knobs.h"
#include "stage_range.h"

using zv::Model;

struct PendingBatch;
struct zv_model
{
    Model        *m;
    PendingBatch *pending;       // [ZV_BATCH_LANES], see zv_synthesize_batch_begin
};

static void free_pending(zv_model *m);
static void lane0_select(zv_model *m);   // selects lane 0 without the busy check (copies, waits, profiling)
static void use_lane0(zv_model *m);      // selects lane 0 (the lane of every synchronous entry point); fails when lane 0 has a batch in flight

static thread_local std::string g_last_error;

template <typename F> static zv_status guarded(F &&f)
{
    try
    {
        f();
        return ZV_OK;
    }
    catch (const zv::Error &e)
    {
        g_last_error = e.what();
        return e.status;
    }
    catch (const std::bad_alloc &)
    {
        g_last_error = "out of host memory";
        return ZV_ERR_OOM;
    }
    catch (const std::exception &e)
    {
        g_last_error = e.what();
        return ZV_ERR_DEVICE;
    }
}

#define ZV_NEED(cond, what) \
    if (!(cond)) zv::fail(ZV_ERR_ARG, "%s: %s", __func__, what)

extern "C" {

const char *zv_last_error(void) { return g_last_error.c_str(); }
const char *zv_version(void) { return "zerovox.cpp_amd 0.1 (gfx950)"; }

zv_status zv_model_load(const char *gguf_path, int device, zv_model **out)
{
    return guarded([&] {
        ZV_NEED(gguf_path && out, "null argument");
        *out = nullptr;
        Model *m = new Model(gguf_path, device);
        *out = new zv_model{m, nullptr};
    });
}

void zv_model_free(zv_model *m)
{
    if (!m) return;
    free_pending(m);
    delete m->m;
    delete m;
}

zv_status zv_model_get_hparams(const zv_model *m, zv_hparams *out)
{
    return guarded([&] {
        ZV_NEED(m && out, "null argument");
        *out = m->m->hp;
    });
}

zv_status zv_model_reserve(zv_model *m, uint32_t max_phonemes, uint32_t max_frames)
{
    return guarded([&] {
        ZV_NEED(m, "null model");
        ZV_HIP(hipSetDevice(m->m->device));
        m->m->reserve(max_phonemes, max_frames);
    });
}

// ---- host-buffer entry points -------------------------------------------------------------------

static void check_ids(const Model &M, const int32_t *ids, const int32_t *puncts, uint32_t n)
{
    // the reference aborts inside ggml_get_rows on a bad id (ggml-cpu.c:8456); the tables have 155 / 7 rows in the
    // reference's checkpoints (src/zerovox.h:35-36) — the limit is what the loaded file holds
    const int wmax = M.wemb_rows() - 1, pmax = M.pemb_rows() - 1;
    for (uint32_t i = 0; i < n; i++)
    {
        if (ids[i] < 0 || ids[i] > wmax) zv::fail(ZV_ERR_ARG, "phoneme id %d at position %u is outside [0, %d]", ids[i], i, wmax);
        if (puncts[i] < 0 || puncts[i] > pmax) zv::fail(ZV_ERR_ARG, "punctuation id %d at position %u is outside [0, %d]", puncts[i], i, pmax);
    }
}

#include "demo_utterance.inc"

void zv_demo_utterance(const int32_t **ids, const int32_t **puncts, const float **style, uint32_t *n_phonemes, uint32_t *style_len)
{
    if (ids) *ids = kDemoIds;
    if (puncts) *puncts = kDemoPuncts;
    if (style) *style = kDemoStyle;
    if (n_phonemes) *n_phonemes = 120;
    if (style_len) *style_len = 528;
}

uint32_t zv_max_frames(const zv_model *m) { return m ? m->m->max_frames_per_utterance() : 0; }

static void check_T(const Model &M, uint32_t T)
{
    if (T == 0) zv::fail(ZV_ERR_ARG, "T must be > 0");
    if (T > M.max_frames_per_utterance())
        zv::fail(ZV_ERR_ARG, "T = %u exceeds zv_max_frames() = %u frames per utterance (32-bit offsets inside a segment); use zv_vocode_stream for longer audio",
                 T, M.max_frames_per_utterance());
}

using zv::Layout;      // wave_stages.h

// One call's utterances, in the form the batch entry points take them; a single-utterance entry point makes a request of one
// that points at its own arguments.  out[u] receives utterance u's waveform (zv_encode_taps*: its hidden frames); n_frames,
// prosody and phonemes are [count] or null; durations is [count] or null, and its entries may be null.
// A batch request runs the stages of `range` (stage_range.h): out[u] receives what the last stage writes (an encoder-only request:
// hidden, or null = not downloaded), src[u] is what the first stage reads where that is not the encoder (hidden, mel); what the range
// does not read (ids, puncts, n, num_phonemes without the encoder; styles with the vocoder alone) is null.
struct Request
{
    const char                *fn;                     // the C entry point, for messages
    uint32_t                   count;
    const int32_t *const      *ids, *const *puncts;
    const float *const        *styles;
    const uint32_t            *n, *num_phonemes, *T;   // num_phonemes[u] <= n[u]: the tokens the length regulator walks
    float *const              *out;
    uint32_t                  *n_frames = nullptr;
    const zv_prosody          *prosody = nullptr;
    const zv_phoneme_controls *phonemes = nullptr;
    int32_t *const            *durations = nullptr;
    // fitted (zv_synthesize_fitted): decode and vocode each utterance as the n_frames the length regulator fills, not as T
    bool                       fitted = false;
    // target durations (zv_*_target): [count] or null, 0 = no target for that utterance
    const uint32_t            *target_frames = nullptr;
    // the waveform stages' arguments (wave_stages.h), in the entry points' order: volume, levels, envelope, contour, pitch, bands, filter
    zv::WaveArgs               wave;
    zv::StageRange             range;
    const float *const        *src = nullptr;

    // any utterance with a target: then every utterance gets a ctl row and pctl rows (the identity where it has no controls), which
    // the device step between the duration predictor and the length regulator reads and rewrites (kernels.h launch_fit_durations)
    bool targets() const
    {
        for (uint32_t u = 0; target_frames && u < count; u++)
            if (target_frames[u]) return true;
        return false;
    }
    // any utterance with per-phoneme controls: then every utterance gets rows (the identity where it has none)
    bool phoneme_controls() const
    {
        for (uint32_t u = 0; phonemes && u < count; u++)
            if (phonemes[u].duration_frames || phonemes[u].duration_scale || phonemes[u].pitch_shift || phonemes[u].energy_shift)
                return true;
        return false;
    }
    // any utterance that asks for its phoneme timings
    bool timings() const
    {
        for (uint32_t u = 0; durations && u < count; u++)
            if (durations[u]) return true;
        return false;
    }
    // utterances [a, b)
    Request slice(uint32_t a, uint32_t b) const
    {
        Request s = *this;
        s.count = b - a;
        if (ids) s.ids += a;
        if (puncts) s.puncts += a;
        if (styles) s.styles += a;
        if (n) s.n += a;
        if (num_phonemes) s.num_phonemes += a;
        if (src) s.src += a;
        s.T += a;
        s.out += a;
        if (n_frames) s.n_frames += a;
        if (prosody) s.prosody += a;
        if (phonemes) s.phonemes += a;
        if (durations) s.durations += a;
        if (target_frames) s.target_frames += a;
        s.wave = wave.slice(a);
        return s;
    }
};

static void check_prosody(const zv_prosody &p)
{
    static const char *const names[5] = {"duration_scale", "pitch_scale", "pitch_shift", "energy_scale", "energy_shift"};
    const float f[5] = {p.duration_scale, p.pitch_scale, p.pitch_shift, p.energy_scale, p.energy_shift};
    for (int k = 0; k < 5; k++)
        if (!std::isfinite(f[k])) zv::fail(ZV_ERR_ARG, "prosody %s = %g is not finite", names[k], (double)f[k]);
    if (!(f[0] > 0.0f && f[0] <= 16.0f)) zv::fail(ZV_ERR_ARG, "prosody duration_scale = %g is outside (0, 16]", (double)f[0]);
}

static void check_volume(const zv_volume &v)
{
    static const char *const names[3] = {"gain", "target_rms", "peak_ceiling"};
    const float f[3] = {v.gain, v.target_rms, v.peak_ceiling};
    const float hi[3] = {1000.0f, 1.0f, 1.0f};
    for (int k = 0; k < 3; k++)
    {
        if (!std::isfinite(f[k])) zv::fail(ZV_ERR_ARG, "volume %s = %g is not finite", names[k], (double)f[k]);
        if (!(f[k] >= 0.0f && f[k] <= hi[k])) zv::fail(ZV_ERR_ARG, "volume %s = %g is outside [0, %g]", names[k], (double)f[k], (double)hi[k]);
    }
}

// a request's volume rows in the kernels' layout (level.h LEVEL_VOL_STRIDE), the identity {1, 0, 0} where the call only meters
static void pack_volume(const Request &r, float *vol)
{
    static const zv_volume identity = {1.0f, 0.0f, 0.0f};
    for (uint32_t u = 0; u < r.count; u++)
    {
        const zv_volume &v = r.wave.volume ? r.wave.volume[u] : identity;
        float *c = vol + (size_t)u * zv::LEVEL_VOL_STRIDE;
        c[0] = v.gain;
        c[1] = v.target_rms;
        c[2] = v.peak_ceiling;
        c[3] = 0.0f;
    }
}
static_assert(sizeof(zv_level) == sizeof(zv::LevelRow) && sizeof(zv_level) == 16, "zv_level is the kernels' LevelRow");
static_assert(sizeof(zv_frame_level) == sizeof(zv::ContourRow) && sizeof(zv_frame_level) == 8, "zv_frame_level is the kernels' ContourRow");

static_assert(zv::SEG_BYTES == sizeof(zv::Seg) && zv::CTL_ROW_BYTES == zv::CTL_STRIDE * 4 && zv::PCTL_ROW_BYTES == zv::PCTL_STRIDE * 4,
              "stage_range.h sizes the tables and control rows without kernels.h");
static_assert(sizeof(zv_pitch_frame) == sizeof(zv::PitchFrameRow) && sizeof(zv_pitch_frame) == 8, "zv_pitch_frame is the kernels' PitchFrameRow");
static_assert(sizeof(zv_pitch_phoneme) == sizeof(zv::PitchPhonemeRow) && sizeof(zv_pitch_phoneme) == 8, "zv_pitch_phoneme is the kernels' PitchPhonemeRow");

// a zv_pitch's parameters with their defaults filled in (pitch.h pitch_params_resolve), or ZV_ERR_ARG naming the field
static zv::PitchParams resolve_pitch(const Model &M, const zv_pitch &p)
{
    zv::PitchParams q = {p.min_lag, p.max_lag, p.window, p.voiced_threshold};
    bool defaulted = false;
    if (const char *field = zv::pitch_params_resolve(M.hp.audio_sampling_rate, M.hp.audio_hop_size, q, &defaulted))
    {
        const double v = !strcmp(field, "min_lag") ? q.min_lag : !strcmp(field, "max_lag") ? q.max_lag : !strcmp(field, "window") ? q.window
                                                                                                         : (double)q.voiced_threshold;
        zv::fail(ZV_ERR_ARG, "pitch %s = %g breaks 8 <= min_lag < max_lag <= 512, max_lag <= 8 * min_lag, 64 <= window <= 1024, 0 < voiced_threshold <= 1%s",
                 field, v, defaulted ? " (the default at this checkpoint's rate and hop: it needs explicit lags and window)" : "");
    }
    return q;
}

// a request's pitch parameters in the kernels' layout (pitch.h PITCH_PARAM_STRIDE), resolved; an utterance that asks for no table
// gets the cheapest valid row (its rows are written and never downloaded)
static void pack_pitch(const Model &M, const Request &r, uint32_t *par)
{
    for (uint32_t u = 0; u < r.count; u++)
    {
        zv::PitchParams q = {zv::PITCH_LAG_LO, zv::PITCH_LAG_LO + 1, zv::PITCH_WINDOW_LO, 0.5f};
        if (r.wave.pitch[u].frames || r.wave.pitch[u].phonemes) q = resolve_pitch(M, r.wave.pitch[u]);
        uint32_t *c = par + (size_t)u * zv::PITCH_PARAM_STRIDE;
        c[0] = q.min_lag;
        c[1] = q.max_lag;
        c[2] = q.window;
        c[3] = zv::level_bits(q.voiced_threshold);
    }
}

// a zv_bands' resolved parameter row (bands.h bands_resolve), or ZV_ERR_ARG naming the field
static void resolve_bands(const zv_bands &b, uint32_t *row)
{
    if (const char *field = zv::bands_resolve(b.n_bands, b.edges, row))
    {
        if (!strcmp(field, "n_bands")) zv::fail(ZV_ERR_ARG, "bands n_bands = %u exceeds %u", b.n_bands, zv::BANDS_MAX);
        if (!b.edges) zv::fail(ZV_ERR_ARG, "bands edges = NULL (the default edges) needs n_bands 0 or %u, got %u", zv::BANDS_DEFAULT, b.n_bands);
        zv::fail(ZV_ERR_ARG, "bands edges must ascend strictly and end at or below %d (edges[n_bands] = %u)", zv::BANDS_BINS,
                 b.edges[b.n_bands ? b.n_bands : zv::BANDS_DEFAULT]);
    }
}

// a request's band parameters in the kernels' layout (bands.h BANDS_PARAM_STRIDE), resolved; an utterance that asks for no table gets
// n_bands = 0, which both passes skip.  A row's first word is the utterance's band count
static void pack_bands(const Request &r, uint32_t *par)
{
    for (uint32_t u = 0; u < r.count; u++)
    {
        uint32_t *c = par + (size_t)u * zv::BANDS_PARAM_STRIDE;
        memset(c, 0, zv::BANDS_PARAM_STRIDE * 4);
        if (r.wave.bands[u].frames || r.wave.bands[u].phonemes) resolve_bands(r.wave.bands[u], c);
    }
}

// a zv_filter's checks (filter.h filter_check), or ZV_ERR_ARG naming the field
static void check_filter(const zv_filter &f)
{
    if (const char *field = zv::filter_check(f.taps, f.n_taps))
    {
        if (!strcmp(field, "n_taps"))
            zv::fail(ZV_ERR_ARG, "filter n_taps = %u must be odd and in 1 .. %u", f.n_taps, zv::FILTER_MAX_TAPS);
        zv::fail(ZV_ERR_ARG, "filter taps holds a value that is not finite");
    }
}

// a request's filter rows in the kernel's layout (filter.h FILTER_PARAM_STRIDE); an utterance without a filter gets n_taps = 0
static void pack_filter(const Request &r, uint32_t *par)
{
    for (uint32_t u = 0; u < r.count; u++) zv::filter_pack(r.wave.filter[u].taps, r.wave.filter[u].n_taps, par + (size_t)u * zv::FILTER_PARAM_STRIDE);
}

static void check_envelope(const zv_envelope &e, uint32_t n)
{
    for (uint32_t i = 0; e.phoneme_gain && i < n; i++)
    {
        const float v = e.phoneme_gain[i];
        if (!std::isfinite(v)) zv::fail(ZV_ERR_ARG, "envelope phoneme_gain[%u] = %g is not finite", i, (double)v);
        if (!(v >= 0.0f && v <= zv::ENV_MAX_GAIN))
            zv::fail(ZV_ERR_ARG, "envelope phoneme_gain[%u] = %g is outside [0, %g]", i, (double)v, (double)zv::ENV_MAX_GAIN);
    }
    if (e.ramp_frames > (uint32_t)zv::ENV_MAX_RAMP)
        zv::fail(ZV_ERR_ARG, "envelope ramp_frames = %u exceeds %d", e.ramp_frames, zv::ENV_MAX_RAMP);
    if (e.fade_in_samples > 0x7fffffffu) zv::fail(ZV_ERR_ARG, "envelope fade_in_samples = %u exceeds 2147483647", e.fade_in_samples);
    if (e.fade_out_samples > 0x7fffffffu) zv::fail(ZV_ERR_ARG, "envelope fade_out_samples = %u exceeds 2147483647", e.fade_out_samples);
}

// a request's envelopes in the kernels' layouts: gain, one f32 per token packed like the token table (1 where an utterance gives
// none), and env, one zv::ENV_CTL_STRIDE row of integers per utterance
static void pack_envelope(const Request &r, float *gain, int32_t *env)
{
    for (uint32_t u = 0, row = 0; u < r.count; row += r.n[u], u++)
    {
        const zv_envelope &e = r.wave.envelope[u];
        for (uint32_t i = 0; i < r.n[u]; i++) gain[row + i] = e.phoneme_gain ? e.phoneme_gain[i] : 1.0f;
        int32_t *c = env + (size_t)u * zv::ENV_CTL_STRIDE;
        c[0] = (int32_t)e.ramp_frames;
        c[1] = (int32_t)e.fade_in_samples;
        c[2] = (int32_t)e.fade_out_samples;
        c[3] = 0;
    }
}

// ---- the waveform stages as a group (wave_stages.h): what run_single and batch_enqueue share.  Besides check_request's lines only
// pack_wave and wave_tables name the stages; nothing behind them does.
// a request's stage rows in the kernels' layouts, in a host block at the planned offsets of its input regions (a batch's pinned input
// block, a single utterance's host staging); token rows past the utterances are never read
static void pack_wave(const Model &M, const Request &r, const zv::WaveAsk &ask, char *h, const zv::WaveOffsets &o)
{
    if (ask.on[zv::WS_VOLUME]) pack_volume(r, (float *)(h + o.at[zv::R_VOL]));
    if (ask.on[zv::WS_ENVELOPE]) pack_envelope(r, (float *)(h + o.at[zv::R_ENV_GAIN]), (int32_t *)(h + o.at[zv::R_ENV]));
    if (ask.on[zv::WS_PITCH]) pack_pitch(M, r, (uint32_t *)(h + o.at[zv::R_PIT_PAR]));
    if (ask.on[zv::WS_BANDS]) pack_bands(r, (uint32_t *)(h + o.at[zv::R_BND_PAR]));
    if (ask.on[zv::WS_FILTER]) pack_filter(r, (uint32_t *)(h + o.at[zv::R_FLT_PAR]));
}

// an utterance's table at the caller (null: not asked for) and the bytes of a row there
struct RowDst { void *p; size_t row; };

// One table a stage hands back: the device rows, the bytes of a device row (and of a staging row), the staging rows in a batch's pinned
// block or null (a single utterance's rows go straight to the caller), and whether there is a row per utterance, token row or frame row
struct RowTable { const char *dev; size_t dev_row; char *host; zv::WaveRowKind rows; };

// The tables of a request, one per staging region that exists for it, and what each utterance receives of them, dst[k * count + u].
// dev: the block of the device regions; host: the pinned block of the staging regions, or null; h, ho: the packed input regions and
// their offsets, where a band table's n_bands is read (a band row at the caller is the first n_bands entries of the device's).
static void wave_tables(const Request &r, const zv::WaveAsk &ask, const zv::WaveOffsets &o, const char *dev, char *host, const char *h,
                        const zv::WaveOffsets &ho, std::vector<RowTable> &tabs, std::vector<RowDst> &dst)
{
    const zv::WaveArgs &w = r.wave;
    tabs.clear();
    dst.clear();
    for (int id = 0; id < zv::R_COUNT; id++)
    {
        const zv::WaveRegion &g = zv::WAVE_REGIONS[id];
        if (g.role != zv::WR_HOST || !zv::wave_region_exists(g, ask)) continue;
        tabs.push_back(RowTable{dev + o.at[g.device], g.row_bytes, host ? host + o.at[id] : nullptr, g.rows});
        for (uint32_t u = 0; u < r.count; u++)
        {
            const size_t band_row = ask.on[zv::WS_BANDS] ? 4 * (size_t)((const uint32_t *)(h + ho.at[zv::R_BND_PAR]))[(size_t)u * zv::BANDS_PARAM_STRIDE] : 0;
            dst.push_back(id == zv::R_LEVELS_HOST         ? RowDst{w.levels ? w.levels + u : nullptr, sizeof(zv_level)}
                          : id == zv::R_CTR_FRAMES_HOST   ? RowDst{w.contour[u].frames, sizeof(zv_frame_level)}
                          : id == zv::R_CTR_PHONEMES_HOST ? RowDst{w.contour[u].phonemes, sizeof(zv_frame_level)}
                          : id == zv::R_PIT_FRAMES_HOST   ? RowDst{w.pitch[u].frames, sizeof(zv_pitch_frame)}
                          : id == zv::R_PIT_PHONEMES_HOST ? RowDst{w.pitch[u].phonemes, sizeof(zv_pitch_phoneme)}
                          : id == zv::R_BND_FRAMES_HOST   ? RowDst{w.bands[u].frames, band_row}
                                                          : RowDst{w.bands[u].phonemes, band_row});
        }
    }
}

// rows [first, first + count) of a table to dst on stream st, dst_row bytes of each: whole rows, or the leading part of each
static void rows_download(const RowTable &t, size_t first, size_t count, void *dst, size_t dst_row, hipStream_t st)
{
    if (!count) return;
    const char *src = t.dev + first * t.dev_row;
    if (dst_row == t.dev_row)
        ZV_HIP(hipMemcpyAsync(dst, src, count * t.dev_row, hipMemcpyDeviceToHost, st));
    else
        ZV_HIP(hipMemcpy2DAsync(dst, dst_row, src, t.dev_row, dst_row, count, hipMemcpyDeviceToHost, st));
}

static void check_phoneme_controls(const Model &M, const zv_phoneme_controls &p, uint32_t n)
{
    const int64_t fmax = std::min<int64_t>(32768, M.max_frames_per_utterance());      // forced frames travel as exact f32 integers
    for (uint32_t i = 0; i < n; i++)
    {
        if (p.duration_frames && (p.duration_frames[i] < -1 || p.duration_frames[i] > fmax))
            zv::fail(ZV_ERR_ARG, "duration_frames[%u] = %d is outside [-1, %lld]", i, p.duration_frames[i], (long long)fmax);
        if (p.duration_scale)
        {
            const float v = p.duration_scale[i];
            if (!std::isfinite(v)) zv::fail(ZV_ERR_ARG, "duration_scale[%u] = %g is not finite", i, (double)v);
            if (!(v > 0.0f && v <= 16.0f)) zv::fail(ZV_ERR_ARG, "duration_scale[%u] = %g is outside (0, 16]", i, (double)v);
        }
        if (p.pitch_shift && !std::isfinite(p.pitch_shift[i]))
            zv::fail(ZV_ERR_ARG, "pitch_shift[%u] = %g is not finite", i, (double)p.pitch_shift[i]);
        if (p.energy_shift && !std::isfinite(p.energy_shift[i]))
            zv::fail(ZV_ERR_ARG, "energy_shift[%u] = %g is not finite", i, (double)p.energy_shift[i]);
    }
}

// Every check of a request, utterance by utterance, before the caller enqueues anything.  ZV_ERR_ARG; the message names the
// entry point, the utterance and what is wrong (for per-phoneme controls the field and the phoneme).
static void check_request(zv_model *m, const Request &r)
{
    const bool enc = r.range.has(zv::ST_ENCODER);      // without it a request has no tokens: what it reads is src, frames by T
    if (!(m && r.T && r.out && (enc ? r.ids && r.puncts && r.n && r.num_phonemes : r.src != nullptr) && (r.styles || r.range.first == zv::ST_VOCODER)))
        zv::fail(ZV_ERR_ARG, "%s: null argument", r.fn);
    const Model &M = *m->m;
    const bool tg = r.targets();
    // the one limit of the envelope that is the checkpoint's, not an utterance's (kernels.h env_hop_supported)
    if (r.wave.envelope && !zv::env_hop_supported(M.hp.audio_hop_size))
        zv::fail(ZV_ERR_ARG, "%s: an envelope needs audio_hop_size >= 10, the checkpoint has %d", r.fn, (int)M.hp.audio_hop_size);
    for (uint32_t u = 0; u < r.count; u++)
    {
        try
        {
            if (!enc)
            {
                if (!(r.src[u] && r.out[u] && (!r.styles || r.styles[u]))) zv::fail(ZV_ERR_ARG, "null argument");
                check_T(M, r.T[u]);
                continue;
            }
            // (an encoder-only request may leave an utterance's hidden where it is: the planning call)
            if (!(r.ids[u] && r.puncts[u] && r.styles[u] && (r.out[u] || r.range.last == zv::ST_ENCODER))) zv::fail(ZV_ERR_ARG, "null argument");
            if (!(r.n[u] > 0 && r.T[u] > 0)) zv::fail(ZV_ERR_ARG, "n and T must be > 0");
            check_T(M, r.T[u]);
            if (r.num_phonemes[u] > r.n[u]) zv::fail(ZV_ERR_ARG, "num_phonemes exceeds n");
            if (r.n[u] > M.max_phonemes())
                zv::fail(ZV_ERR_ARG, "%u phonemes exceed the %u rows of the sinusoid table", r.n[u], M.max_phonemes());
            check_ids(M, r.ids[u], r.puncts[u], r.n[u]);
            if (r.prosody) check_prosody(r.prosody[u]);
            if (r.phonemes) check_phoneme_controls(M, r.phonemes[u], r.n[u]);
            const zv::WaveArgs &w = r.wave;
            if (w.volume) check_volume(w.volume[u]);
            if (w.envelope) check_envelope(w.envelope[u], r.n[u]);
            if (w.pitch && (w.pitch[u].frames || w.pitch[u].phonemes)) resolve_pitch(M, w.pitch[u]);
            if (w.bands && (w.bands[u].frames || w.bands[u].phonemes))
            {
                uint32_t row[zv::BANDS_PARAM_STRIDE];
                resolve_bands(w.bands[u], row);
            }
            if (w.filter) check_filter(w.filter[u]);
            if (r.target_frames && r.target_frames[u] > r.T[u])
                zv::fail(ZV_ERR_ARG, "target_frames = %u exceeds the capacity T = %u", r.target_frames[u], r.T[u]);
            if (tg && r.n[u] > (uint32_t)zv::FIT_MAX_TOKENS)      // one launch covers the request's utterances, with or without a target
                zv::fail(ZV_ERR_ARG, "target_frames needs n <= %d phonemes, got %u", zv::FIT_MAX_TOKENS, r.n[u]);
        }
        catch (const zv::Error &e)
        {
            zv::fail(e.status, "%s: utterance %u: %s", r.fn, u, e.what());
        }
    }
}

// A request's controls in the kernels' layouts (kernels.h CTL_*, PCTL_*), written where the caller says: a batch's pinned input
// block, or a single utterance's host staging.  ctl: with prosody, one zv::CTL_STRIDE row per utterance.  pctl: with per-phoneme
// controls, one zv::PCTL_STRIDE row per token, packed like the token table; absent fields get the identity {-1, 1, 0, 0}.
// With a target on any utterance both are written: the identity prosody {1, 1, 0, 1, 0} where none is given, identity rows for an
// utterance without per-phoneme controls, and each utterance's target in CTL_TARGET (frame counts up to 32 768 are exact in f32).
static void pack_controls(const Request &r, float *ctl, float *pctl)
{
    const bool tg = r.targets(), pc = r.phoneme_controls() || tg;
    static const zv_prosody identity = {1.0f, 1.0f, 0.0f, 1.0f, 0.0f};
    static const zv_phoneme_controls none = {nullptr, nullptr, nullptr, nullptr};
    for (uint32_t u = 0, row = 0; u < r.count; row += r.n[u], u++)
    {
        if (r.prosody || tg)
        {
            const zv_prosody &p = r.prosody ? r.prosody[u] : identity;
            float *c = ctl + (size_t)u * zv::CTL_STRIDE;
            std::fill(c, c + zv::CTL_STRIDE, 0.0f);
            c[zv::CTL_DURATION] = p.duration_scale;
            c[zv::CTL_PITCH] = p.pitch_scale;
            c[zv::CTL_PITCH + 1] = p.pitch_shift;
            c[zv::CTL_ENERGY] = p.energy_scale;
            c[zv::CTL_ENERGY + 1] = p.energy_shift;
            if (tg) c[zv::CTL_TARGET] = (float)r.target_frames[u];
        }
        for (uint32_t i = 0; pc && i < r.n[u]; i++)
        {
            const zv_phoneme_controls &p = r.phonemes ? r.phonemes[u] : none;
            float *c = pctl + (size_t)(row + i) * zv::PCTL_STRIDE;
            c[zv::PCTL_FRAMES] = p.duration_frames ? (float)p.duration_frames[i] : -1.0f;
            c[zv::PCTL_DURATION] = p.duration_scale ? p.duration_scale[i] : 1.0f;
            c[zv::PCTL_PITCH] = p.pitch_shift ? p.pitch_shift[i] : 0.0f;
            c[zv::PCTL_ENERGY] = p.energy_shift ? p.energy_shift[i] : 0.0f;
        }
    }
}

// The phoneme timings from the length regulator's scan, packed like the token table: durations[u][i] = min(cum[i], T[u]) -
// min(cum[i - 1], T[u]), the frames token i of utterance u occupies in hidden (null entries are skipped)
static void durations_from_cum(const int32_t *cum, uint32_t count, const uint32_t *n, const uint32_t *T, int32_t *const *durations)
{
    for (uint32_t u = 0; u < count; cum += n[u], u++)
    {
        int64_t prev = 0;
        for (uint32_t i = 0; durations[u] && i < n[u]; i++)
        {
            const int64_t c = std::min<int64_t>(cum[i], T[u]);
            durations[u][i] = (int32_t)(c - prev);
            prev = c;
        }
    }
}

// the taps zv_encode_taps* returns beside hidden, each [n] (features [n][E]) or null
struct Taps
{
    float   *features, *logdur, *pitch, *energy;
    int32_t *pitch_bucket, *energy_bucket;
};

// One utterance on lane 0, host buffers in and out: the encoder with its taps (taps given, r.out[0] is hidden) or the whole chain
// (r.out[0] is the waveform).  The schedule of one utterance (Batch::single, inline segments), not a batch of one.
static zv_status run_single(zv_model *m, const Request &r, std::optional<Taps> taps = std::nullopt)
{
    return guarded([&] {
        check_request(m, r);
        Model &M = *m->m;
        use_lane0(m);
        const uint32_t n = r.n[0], T = r.T[0];
        const bool tg = r.targets(), pc = r.phoneme_controls() || tg, dur = r.timings();
        const size_t E = M.E(), b_ids = (size_t)n * 4, b_hid = (size_t)T * E * 4, b_wav = (size_t)T * M.hp.audio_hop_size * 4;
        const size_t b_ctl = r.prosody || tg ? zv::CTL_STRIDE * 4 : 0, b_pctl = pc ? (size_t)n * zv::PCTL_STRIDE * 4 : 0;
        const zv::WaveAsk ask = taps ? zv::WaveAsk{} : r.wave.ask(1);      // (an encoder-taps call has no waveform)
        const void *bands_table = ask.on[zv::WS_BANDS] ? M.bands_table() : nullptr;      // (allocates and copies on first use: ahead of everything enqueued)
        if (!taps) M.reserve(n, T);
        // [frame count][ids][puncts][style][controls][phoneme controls][hidden], and for the chain [mel][wav][scan] (scan: only when
        // timings are asked for, the length regulator's `cum`, which the decoder and vocoder would otherwise overwrite in the arena)
        // [live frame table] (fitted: one entry, written on the device) [decoder run table] (run-shortened decoding: one entry, likewise)
        Layout L;
        const size_t o_nf = L.at(4), o_ids = L.at(b_ids), o_pun = L.at(b_ids), o_sty = L.at(E * 4), o_ctl = L.at(b_ctl),
                     o_pctl = L.at(b_pctl), o_hid = L.at(b_hid);
        const size_t o_mel = taps ? 0 : L.at((size_t)T * M.hp.audio_num_mels * 4), o_wav = taps ? 0 : L.at(b_wav),
                     o_cum = taps ? 0 : L.at(dur || ask.needs_scan() ? b_ids : 0), o_live = L.at(r.fitted && !taps ? sizeof(zv::Seg) : 0),
                     o_runs = L.at(!r.fitted && !taps ? sizeof(zv::Seg) : 0);
        // the waveform stages' regions (wave_stages.h), uploaded or written on the device; the last regions, so no other offset moves
        const zv::WaveRows rows{1, n, T};
        zv::WaveOffsets wo;
        zv::wave_carve(L, ask, rows, zv::WR_INPUT | zv::WR_DEVICE, wo);
        char *io = (char *)M.io_scratch(L.size());
        int32_t *d_nf = (int32_t *)(io + o_nf), *d_ids = (int32_t *)(io + o_ids), *d_pun = (int32_t *)(io + o_pun);
        float *d_sty = (float *)(io + o_sty), *d_hid = (float *)(io + o_hid);
        std::vector<float> ctl(b_ctl / 4), pctl(b_pctl / 4);         // host staging: lives until the M.sync() below
        std::vector<int32_t> cum(dur ? n : 0);
        pack_controls(r, ctl.data(), pctl.data());
        zv::Batch bt = zv::Batch::single(n, T, r.num_phonemes[0]);
        bt.has_targets = tg;
        if (r.fitted && !taps) bt.d_frm_live = (zv::Seg *)(io + o_live);
        if (!taps && M.dec_plan(bt).runs) bt.d_dec_runs = (zv::Seg *)(io + o_runs);
        ZV_HIP(hipMemcpyAsync(d_ids, r.ids[0], b_ids, hipMemcpyHostToDevice, M.stream()));
        ZV_HIP(hipMemcpyAsync(d_pun, r.puncts[0], b_ids, hipMemcpyHostToDevice, M.stream()));
        ZV_HIP(hipMemcpyAsync(d_sty, r.styles[0], E * 4, hipMemcpyHostToDevice, M.stream()));
        if (b_ctl)
        {
            bt.d_ctl = (const float *)(io + o_ctl);
            ZV_HIP(hipMemcpyAsync(io + o_ctl, ctl.data(), b_ctl, hipMemcpyHostToDevice, M.stream()));
        }
        if (b_pctl)
        {
            bt.d_pctl = (const float *)(io + o_pctl);
            ZV_HIP(hipMemcpyAsync(io + o_pctl, pctl.data(), b_pctl, hipMemcpyHostToDevice, M.stream()));
        }
        // the stages' rows: host staging like ctl, at the offsets of a block of the input regions alone
        Layout S;
        zv::WaveOffsets so;
        zv::wave_carve(S, ask, rows, zv::WR_INPUT, so);
        std::vector<char> stage(S.size());
        pack_wave(M, r, ask, stage.data(), so);
        bt.wave = zv::wave_bind(ask, wo, io, io, d_nf, bands_table);
        for (int id = 0; id < zv::R_COUNT; id++)
            if (const size_t bytes = zv::WAVE_REGIONS[id].role == zv::WR_INPUT ? zv::wave_region_bytes(id, ask, rows) : 0)
                ZV_HIP(hipMemcpyAsync(io + wo.at[id], stage.data() + so.at[id], bytes, hipMemcpyHostToDevice, M.stream()));
        std::vector<RowTable> tabs;      // the stages' tables and where each goes: straight to the caller, like the waveform
        std::vector<RowDst> dst;
        wave_tables(r, ask, wo, io, nullptr, stage.data(), so, tabs, dst);
        int32_t nf = 0;
        if (taps)
        {
            const Model::EncoderTaps t = M.encode_dev(bt, d_ids, d_pun, d_sty, d_hid, d_nf);
            ZV_HIP(hipMemcpyAsync(r.out[0], d_hid, b_hid, hipMemcpyDeviceToHost, M.stream()));
            ZV_HIP(hipMemcpyAsync(&nf, d_nf, 4, hipMemcpyDeviceToHost, M.stream()));
            if (taps->features) ZV_HIP(hipMemcpyAsync(taps->features, t.features, (size_t)n * E * 4, hipMemcpyDeviceToHost, M.stream()));
            if (taps->logdur) ZV_HIP(hipMemcpyAsync(taps->logdur, t.logdur, b_ids, hipMemcpyDeviceToHost, M.stream()));
            if (taps->pitch) ZV_HIP(hipMemcpyAsync(taps->pitch, t.pitch, b_ids, hipMemcpyDeviceToHost, M.stream()));
            if (taps->energy) ZV_HIP(hipMemcpyAsync(taps->energy, t.energy, b_ids, hipMemcpyDeviceToHost, M.stream()));
            if (taps->pitch_bucket) ZV_HIP(hipMemcpyAsync(taps->pitch_bucket, t.pitch_bucket, b_ids, hipMemcpyDeviceToHost, M.stream()));
            if (taps->energy_bucket) ZV_HIP(hipMemcpyAsync(taps->energy_bucket, t.energy_bucket, b_ids, hipMemcpyDeviceToHost, M.stream()));
            if (dur) ZV_HIP(hipMemcpyAsync(cum.data(), t.cum, b_ids, hipMemcpyDeviceToHost, M.stream()));
        }
        else
        {
            float *d_mel = (float *)(io + o_mel), *d_wav = (float *)(io + o_wav);
            // an envelope's knots pass and a table stage's phonemes pass read the scan behind the vocoder
            if (dur || bt.wave.needs_scan()) bt.d_cum = (int32_t *)(io + o_cum);
            M.chain_dev(bt, d_ids, d_pun, d_sty, d_hid, d_mel, d_wav, d_nf);
            ZV_HIP(hipMemcpyAsync(&nf, d_nf, 4, hipMemcpyDeviceToHost, M.stream()));
            if (dur) ZV_HIP(hipMemcpyAsync(cum.data(), bt.d_cum, b_ids, hipMemcpyDeviceToHost, M.stream()));
            ZV_HIP(hipMemcpyAsync(r.out[0], d_wav, b_wav, hipMemcpyDeviceToHost, M.stream()));
            for (size_t k = 0; k < tabs.size(); k++)
                if (dst[k].p)
                    rows_download(tabs[k], 0, rows[tabs[k].rows], dst[k].p, dst[k].row, M.stream());
        }
        M.sync();
        if (r.n_frames) r.n_frames[0] = (uint32_t)nf;
        if (dur) durations_from_cum(cum.data(), 1, r.n, r.T, r.durations);
    });
}

// The plain and _prosody forms are the _phonemes form with NULLs: the same request, the same code path, the same bits.
zv_status zv_encode_taps(zv_model *m, const int32_t *ids, const int32_t *puncts, const float *style, uint32_t n,
                         uint32_t num_phonemes, uint32_t T, float *hidden, uint32_t *n_frames, float *features, float *logdur,
                         float *pitch, float *energy, int32_t *pitch_bucket, int32_t *energy_bucket)
{
    return run_single(m, {__func__, 1, &ids, &puncts, &style, &n, &num_phonemes, &T, &hidden, n_frames},
                      Taps{features, logdur, pitch, energy, pitch_bucket, energy_bucket});
}

zv_status zv_encode_taps_prosody(zv_model *m, const int32_t *ids, const int32_t *puncts, const float *style, uint32_t n,
                                 uint32_t num_phonemes, uint32_t T, float *hidden, uint32_t *n_frames, float *features, float *logdur,
                                 float *pitch, float *energy, int32_t *pitch_bucket, int32_t *energy_bucket, const zv_prosody *prosody)
{
    return run_single(m, {__func__, 1, &ids, &puncts, &style, &n, &num_phonemes, &T, &hidden, n_frames, prosody},
                      Taps{features, logdur, pitch, energy, pitch_bucket, energy_bucket});
}

zv_status zv_encode_taps_phonemes(zv_model *m, const int32_t *ids, const int32_t *puncts, const float *style, uint32_t n,
                                  uint32_t num_phonemes, uint32_t T, float *hidden, uint32_t *n_frames, float *features, float *logdur,
                                  float *pitch, float *energy, int32_t *pitch_bucket, int32_t *energy_bucket, const zv_prosody *prosody,
                                  const zv_phoneme_controls *phonemes, int32_t *durations)
{
    return run_single(m, {__func__, 1, &ids, &puncts, &style, &n, &num_phonemes, &T, &hidden, n_frames, prosody, phonemes, &durations},
                      Taps{features, logdur, pitch, energy, pitch_bucket, energy_bucket});
}

zv_status zv_encode(zv_model *m, const int32_t *ids, const int32_t *puncts, const float *style, uint32_t n, uint32_t T,
                    float *hidden, uint32_t *n_frames)
{
    return zv_encode_taps(m, ids, puncts, style, n, n, T, hidden, n_frames, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}

zv_status zv_decode(zv_model *m, const float *hidden, const float *style, uint32_t T, float *mel)
{
    return guarded([&] {
        ZV_NEED(m && hidden && style && mel, "null argument");
        Model &M = *m->m;
        use_lane0(m);
        check_T(M, T);
        const size_t E = M.E(), b_hid = (size_t)T * E * 4, b_mel = (size_t)T * M.hp.audio_num_mels * 4;
        Layout L;
        const size_t o_sty = L.at(E * 4), o_hid = L.at(b_hid), o_mel = L.at(b_mel);
        char *io = (char *)M.io_scratch(L.size());
        float *d_sty = (float *)(io + o_sty), *d_hid = (float *)(io + o_hid), *d_mel = (float *)(io + o_mel);
        ZV_HIP(hipMemcpyAsync(d_hid, hidden, b_hid, hipMemcpyHostToDevice, M.stream()));
        ZV_HIP(hipMemcpyAsync(d_sty, style, E * 4, hipMemcpyHostToDevice, M.stream()));
        M.decode_dev(zv::Batch::single(1, T, 1), d_hid, d_sty, d_mel);
        ZV_HIP(hipMemcpyAsync(mel, d_mel, b_mel, hipMemcpyDeviceToHost, M.stream()));
        M.sync();
    });
}

zv_status zv_vocode(zv_model *m, const float *mel, uint32_t T, float *wav)
{
    return guarded([&] {
        ZV_NEED(m && mel && wav, "null argument");
        Model &M = *m->m;
        use_lane0(m);
        check_T(M, T);
        const size_t b_mel = (size_t)T * M.hp.audio_num_mels * 4, b_wav = (size_t)T * M.hp.audio_hop_size * 4;
        Layout L;
        const size_t o_mel = L.at(b_mel), o_wav = L.at(b_wav);
        char *io = (char *)M.io_scratch(L.size());
        float *d_mel = (float *)(io + o_mel), *d_wav = (float *)(io + o_wav);
        ZV_HIP(hipMemcpyAsync(d_mel, mel, b_mel, hipMemcpyHostToDevice, M.stream()));
        M.vocode_dev_graph(zv::Batch::single(1, T, 1), d_mel, d_wav);
        ZV_HIP(hipMemcpyAsync(wav, d_wav, b_wav, hipMemcpyDeviceToHost, M.stream()));
        M.sync();
    });
}

uint32_t zv_vocoder_halo_frames(zv_model *m) { return m ? m->m->vocoder_halo_frames() : 0; }

zv_status zv_vocode_stream(zv_model *m, const float *mel, uint32_t T, uint32_t chunk_frames, zv_wav_sink sink, void *user)
{
    return guarded([&] {
        ZV_NEED(m && mel && sink, "null argument");
        ZV_NEED(T > 0 && chunk_frames > 0, "T and chunk_frames must be > 0");
        Model &M = *m->m;
        use_lane0(m);
        const size_t Mm = M.hp.audio_num_mels, hop = M.hp.audio_hop_size;
        const uint32_t H = M.vocoder_halo_frames();
        const uint32_t ctx_max = std::min<uint64_t>(T, (uint64_t)chunk_frames + 2 * H);
        check_T(M, ctx_max);                          // only a chunk plus its context is ever vocoded at once
        // the chunks are the schedule here: no run-shortening inside a chunk
        struct RunsOff { Model &M; ~RunsOff() { M.voc_runs_off = false; } } runs_off{M};
        M.voc_runs_off = true;
        M.reserve(1, ctx_max);
        Layout L;
        const size_t o_mel = L.at((size_t)T * Mm * 4), o_wav = L.at((size_t)ctx_max * hop * 4);
        char *io = (char *)M.io_scratch(L.size());
        float *d_mel = (float *)(io + o_mel), *d_wav = (float *)(io + o_wav);
        // two pinned slots: chunk c is copied out and delivered while chunk c + 1 is being computed
        Layout P;
        const size_t slot[2] = {P.at((size_t)chunk_frames * hop * 4), P.at((size_t)chunk_frames * hop * 4)};
        char *pin = (char *)M.pinned_scratch(P.size());
        hipEvent_t done[2] = {nullptr, nullptr};
        ZV_HIP(hipEventCreateWithFlags(&done[0], hipEventDisableTiming));
        ZV_HIP(hipEventCreateWithFlags(&done[1], hipEventDisableTiming));
        struct Pending { bool live; uint64_t first, n; } pend[2] = {{false, 0, 0}, {false, 0, 0}};
        auto deliver = [&](int k) {
            if (!pend[k].live) return;
            ZV_HIP(hipEventSynchronize(done[k]));
            sink(user, (const float *)(pin + slot[k]), pend[k].first, pend[k].n);
            pend[k].live = false;
        };
        try
        {
            ZV_HIP(hipMemcpyAsync(d_mel, mel, (size_t)T * Mm * 4, hipMemcpyHostToDevice, M.stream()));
            int k = 0;
            for (uint32_t a = 0; a < T; a += chunk_frames, k ^= 1)
            {
                const uint32_t b = std::min<uint64_t>(T, (uint64_t)a + chunk_frames);
                const uint32_t c0 = a > H ? a - H : 0, c1 = std::min<uint64_t>(T, (uint64_t)b + H);
                deliver(k);                                   // the slot we are about to overwrite
                M.vocode_dev(zv::Batch::single(1, c1 - c0, 1), d_mel + (size_t)c0 * Mm, d_wav);
                ZV_HIP(hipMemcpyAsync(pin + slot[k], d_wav + (size_t)(a - c0) * hop, (size_t)(b - a) * hop * 4, hipMemcpyDeviceToHost, M.stream()));
                ZV_HIP(hipEventRecord(done[k], M.stream()));
                pend[k] = {true, (uint64_t)a * hop, (uint64_t)(b - a) * hop};
                deliver(k ^ 1);                               // the previous chunk, while this one runs
            }
            deliver(k);
            deliver(k ^ 1);
        }
        catch (...)
        {
            hipStreamSynchronize(M.stream());
            hipEventDestroy(done[0]);
            hipEventDestroy(done[1]);
            throw;
        }
        M.sync();
        hipEventDestroy(done[0]);
        hipEventDestroy(done[1]);
    });
}

zv_status zv_synthesize(zv_model *m, const int32_t *ids, const int32_t *puncts, const float *style, uint32_t n, uint32_t T,
                        float *wav, uint32_t *n_frames)
{
    return run_single(m, {__func__, 1, &ids, &puncts, &style, &n, &n, &T, &wav, n_frames});
}

zv_status zv_synthesize_prosody(zv_model *m, const int32_t *ids, const int32_t *puncts, const float *style, uint32_t n, uint32_t T,
                                float *wav, uint32_t *n_frames, const zv_prosody *prosody)
{
    return run_single(m, {__func__, 1, &ids, &puncts, &style, &n, &n, &T, &wav, n_frames, prosody});
}

zv_status zv_synthesize_phonemes(zv_model *m, const int32_t *ids, const int32_t *puncts, const float *style, uint32_t n, uint32_t T,
                                 float *wav, uint32_t *n_frames, const zv_prosody *prosody, const zv_phoneme_controls *phonemes,
                                 int32_t *durations)
{
    return run_single(m, {__func__, 1, &ids, &puncts, &style, &n, &n, &T, &wav, n_frames, prosody, phonemes, &durations});
}

// copies the finished waveforms out of the pinned staging block, on a few threads when there is enough to move
// (utterances [a, b) of a launch group; off[], wav[] and T[] are indexed from the group's first utterance)
static void scatter_out(const char *pin_wav, const size_t *off, float *const *wav, const uint32_t *T, size_t hop, uint32_t a, uint32_t b)
{
    // (hop: the floats of a frame of what the batch hands back, the waveform's hop for every batch that ends with the vocoder; an
    // utterance without a destination, an encoder batch's planning entries, has nothing staged)
    size_t total = 0;
    for (uint32_t u = a; u < b; u++) total += wav[u] ? (size_t)T[u] * hop * 4 : 0;
    // (a group of the 8-group tail is 5 MB: with the old 8 MB threshold every group went out on one thread, 4 ms per batch between
    // a batch's end and the next batch's start on that lane)
    const unsigned nth = total > ((size_t)1 << 20) ? 4u : 1u;
    auto work = [&](unsigned k) {
        for (uint32_t u = a + k; u < b; u += nth)
            if (wav[u]) memcpy(wav[u], pin_wav + off[u], (size_t)T[u] * hop * 4);
    };
    if (nth == 1)
    {
        work(0);
        return;
    }
    std::vector<std::thread> th;
    for (unsigned k = 1; k < nth; k++) th.emplace_back(work, k);
    work(0);
    for (auto &t : th) t.join();
}

// ---- batches.  One launch group (up to 64 utterances / 64 Ki frames) is enqueued on a lane — input block built in the
// lane's pinned memory, the chain as one hipGraph, the last vocoder stage in utterance groups with each group's download
// behind it on the lane's copy stream — and finished later: wait for the downloads, copy the waveforms out.  The
// synchronous entry point is enqueue + finish on lane 0; zv_synthesize_batch_begin / _end expose the two halves so that a
// caller can keep a batch in flight per lane (the next batch's upload and kernels run while this one's tail downloads).
struct PendingBatch
{
    bool                  active = false;
    zv::StageRange        range;       // what is in flight: the chain, or one stage (zv_vocode_batch_begin); its _end must match
    uint32_t              n_utt = 0;
    int                   G = 1;
    std::vector<uint32_t> gb;          // group boundaries (utterance indices), G + 1 entries
    std::vector<size_t>   woff;        // byte offset of each utterance's waveform in the pinned block
    std::vector<uint32_t> T;
    std::vector<float *>  wav;         // (a batch that ends ahead of the vocoder: its mel or hidden rows; null = that utterance wants none)
    uint32_t             *n_frames = nullptr;
    const char           *h_wav = nullptr;
    const int32_t        *h_nf = nullptr;      // null for a batch without the encoder: no frame counts, no scan
    size_t                hop = 0;             // floats of a frame of `wav`
    // phoneme timings (zv_synthesize_batch_begin_phonemes): the regulator's scan lands in h_cum, packed utterance after utterance
    std::vector<uint32_t> N;
    std::vector<int32_t *> dur;
    const int32_t        *h_cum = nullptr;
    // the waveform stages' tables: the rows land in each table's staging — frame rows packed like the waveforms, phoneme rows like the
    // tokens (noff[u] rows ahead of utterance u) — and are handed out to dst[k * n_utt + u], the table utterance u asked for (or null)
    std::vector<size_t>   noff;
    std::vector<RowTable> tables;
    std::vector<RowDst>   dst;
    // utterance u's rows in a table of this row kind: the first, and how many
    size_t first_row(zv::WaveRowKind k, uint32_t u) const { return k == zv::ROWS_UTTERANCE ? u : k == zv::ROWS_TOKEN ? noff[u] : woff[u] / (hop * 4); }
    size_t row_count(zv::WaveRowKind k, uint32_t u) const { return k == zv::ROWS_UTTERANCE ? 1 : k == zv::ROWS_TOKEN ? N[u] : T[u]; }
};
static PendingBatch &pending_slot(zv_model *m, int lane)
{
    if (!m->pending) m->pending = new PendingBatch[ZV_BATCH_LANES];
    return m->pending[lane];
}
static void free_pending(zv_model *m)
{
    delete[] m->pending;
    m->pending = nullptr;
}
static void lane0_select(zv_model *m)
{
    if (hipSetDevice(m->m->device) != hipSuccess) zv::fail(ZV_ERR_DEVICE, "hipSetDevice(%d) failed", m->m->device);
    m->m->select_lane(0);
}
static void use_lane0(zv_model *m)
{
    // the synchronous and device-resident entry points run on lane 0's stream, arena and I/O block whatever lane was
    // touched last: select it FIRST, then refuse the call while a batch of that lane is still reading those buffers
    if (m->pending && m->pending[0].active)
        zv::fail(ZV_ERR_ARG, "lane 0 has a batch in flight (zv_synthesize_batch_begin): finish it with zv_synthesize_batch_end first");
    if (hipSetDevice(m->m->device) != hipSuccess) zv::fail(ZV_ERR_DEVICE, "hipSetDevice(%d) failed", m->m->device);
    m->m->select_lane(0);
}

// one launch group of a checked request, enqueued on `lane`
static void batch_enqueue(zv_model *m, int lane, const Request &r)
{
    Model &M = *m->m;
    PendingBatch &pb = pending_slot(m, lane);
    if (pb.active) zv::fail(ZV_ERR_ARG, "lane %d already has a batch in flight", lane);
    if (!r.range.valid() || (r.fitted && !r.range.full())) zv::fail(ZV_ERR_ARG, "internal: bad stage range");
    M.select_lane(lane);
    const size_t E = M.E(), Mm = M.hp.audio_num_mels, hop = M.hp.audio_hop_size;
    // the stages this request runs (stage_range.h): the chain, or one stage over the batch.  Without the encoder there are no tokens:
    // the capacities are those of one token per utterance, as a stand-alone decode or vocode of one utterance has them
    const zv::StageRange sr = r.range;
    const bool enc = sr.has(zv::ST_ENCODER), voc = sr.has(zv::ST_VOCODER);
    const bool tg = r.targets(), pc = r.phoneme_controls() || tg, ctl = r.prosody || tg, dur = r.timings();
    const zv::WaveAsk ask = r.wave.ask(r.count);
    const void *bands_table = ask.on[zv::WS_BANDS] ? M.bands_table() : nullptr;      // (allocates and copies on first use: ahead of everything enqueued)
    uint32_t nmax = enc ? 0 : 1, tmax = 0, ntot = 0;
    for (uint32_t u = 0; u < r.count; u++)
    {
        if (enc) nmax = std::max(nmax, r.n[u]);
        tmax = std::max(tmax, r.T[u]);
        if (enc) ntot += r.n[u];
    }
    zv::Batch bt;
    bt.nseg = (int)r.count;
    bt.n_max = zv::round_up((int)nmax, 32);
    bt.n_real = (int)nmax;
    bt.t_max = zv::round_up((int)tmax, 64);
    bt.n_rows = (size_t)bt.nseg * bt.n_max;
    bt.t_rows = (size_t)bt.nseg * bt.t_max;
    // input block, uploaded in one copy from its pinned mirror: [token table][frame table][ids][puncts][styles][controls]
    // [phoneme controls][the waveform stages' input regions] (tables: one entry per utterance + one that spans all of them, see
    // Batch::tokens_merged; controls: only with prosody or a target, one zv::CTL_STRIDE row per utterance; phoneme controls: only with
    // per-phoneme controls or a target, one zv::PCTL_STRIDE row per token row — uploaded with the rest, so a replayed graph reads the
    // values of this call, also where the previous run's fit_durations_kernel has rewritten the rows' frame column)
    // The three blocks are carved by stage_range.h's batch_carve, the chain's as they always were; a region the range does not touch
    // takes no bytes (a stage batch has no token table without the encoder, no waveform without the vocoder, ...)
    // device block: [frame counts][input block][hidden][mel][wav][scan] (scan: only when timings are asked for, the length
    // regulator's `cum`, which the decoder and vocoder would otherwise overwrite in the arena) [live frame table][decoder run table]
    // [the waveform stages' device regions]
    // pinned block: [input block][frame counts][waveforms, utterance after utterance][scan][the waveform stages' staging regions] (a
    // table only where some utterance asks for it; the rows packed like the waveforms / the tokens) [source rows] (a range that starts
    // behind the encoder: the caller's hidden or mel rows, utterance after utterance, uploaded ahead of the schedule)
    // What the batch hands back are the rows of its last stage (hidden, mel, waveform), staged for the utterances that want them.
    zv::BatchShape q;
    q.nseg = (size_t)bt.nseg, q.n_rows = bt.n_rows, q.t_rows = bt.t_rows, q.E = E, q.mels = Mm, q.hop = hop;
    q.ctl = ctl, q.pctl = pc, q.timings = dur, q.fitted = r.fitted, q.n_tokens = ntot;
    const size_t out_row = zv::stage_row_floats(sr.result(), q) * 4, src_row = enc ? 0 : zv::stage_row_floats(sr.source(), q) * 4;
    size_t wav_bytes = 0;
    pb.hop = out_row / 4;
    pb.woff.assign(r.count, 0);
    pb.noff.assign(r.count + 1, 0);
    std::vector<size_t> frm0(r.count + 1, 0);      // an utterance's first frame row in the concatenated tensors
    for (uint32_t u = 0; u < r.count; u++)
    {
        pb.woff[u] = wav_bytes;
        if (r.out[u]) wav_bytes += (size_t)r.T[u] * out_row;
        frm0[u + 1] = frm0[u] + r.T[u];
        pb.noff[u + 1] = pb.noff[u] + (enc ? r.n[u] : 0);
    }
    const size_t frame_rows = frm0[r.count];
    q.n_frames = frame_rows, q.result_bytes = wav_bytes, q.source_bytes = frame_rows * src_row;
    const zv::BatchOffsets bo = zv::batch_carve(sr, q, ask);
    const zv::WaveOffsets &wo = bo.wave;
    const size_t i_tok = bo.at[zv::BI_TOK], i_frm = bo.at[zv::BI_FRM], i_ids = bo.at[zv::BI_IDS], i_pun = bo.at[zv::BI_PUN],
                 i_sty = bo.at[zv::BI_STY], i_ctl = bo.at[zv::BI_CTL], i_pctl = bo.at[zv::BI_PCTL], b_in = bo.in_bytes;
    const size_t o_nf = bo.at[zv::BD_NF], o_in = bo.at[zv::BD_IN], o_hid = bo.at[zv::BD_HID], o_mel = bo.at[zv::BD_MEL],
                 o_wav = bo.at[zv::BD_WAV], o_cum = bo.at[zv::BD_CUM], o_live = bo.at[zv::BD_LIVE], o_runs = bo.at[zv::BD_RUNS];
    const size_t p_in = bo.at[zv::BP_IN], p_nf = bo.at[zv::BP_NF], p_wav = bo.at[zv::BP_OUT], p_cum = bo.at[zv::BP_CUM], p_src = bo.at[zv::BP_SRC];
    char *io = (char *)M.io_scratch(bo.dev_bytes);
    char *pin = (char *)M.pinned_scratch(bo.pin_bytes);
    char *d_in = io + o_in, *h_in = pin + p_in;
    {
        zv::Seg *h_tok = (zv::Seg *)(h_in + i_tok), *h_frm = (zv::Seg *)(h_in + i_frm);
        int32_t *h_ids = (int32_t *)(h_in + i_ids), *h_pun = (int32_t *)(h_in + i_pun);
        float *h_sty = (float *)(h_in + i_sty);
        int32_t n0 = 0, t0 = 0;
        for (uint32_t u = 0; u < r.count; u++)
        {
            const int32_t n = enc ? (int32_t)r.n[u] : 0, t = (int32_t)r.T[u];
            h_frm[u] = zv::Seg{t0, t, 0, 0};
            if (enc)
            {
                h_tok[u] = zv::Seg{n0, n, n, 0};
                memcpy(h_ids + n0, r.ids[u], (size_t)n * 4);
                memcpy(h_pun + n0, r.puncts[u], (size_t)n * 4);
            }
            if (r.styles) memcpy(h_sty + (size_t)u * E, r.styles[u], E * 4);
            if (!enc) memcpy(pin + p_src + frm0[u] * src_row, r.src[u], (size_t)t * src_row);
            n0 += n;
            t0 += t;
        }
        if (enc) h_tok[r.count] = zv::Seg{0, n0, n0, 0};
        h_frm[r.count] = zv::Seg{0, t0, 0, 0};
        if (enc) pack_controls(r, (float *)(h_in + i_ctl), (float *)(h_in + i_pctl));      // (phoneme rows past the utterances are never read)
        pack_wave(M, r, ask, h_in, wo);
    }
    if (enc) bt.d_tok = (const zv::Seg *)(d_in + i_tok);
    bt.d_frm = (const zv::Seg *)(d_in + i_frm);
    if (ctl) bt.d_ctl = (const float *)(d_in + i_ctl);
    bt.has_targets = tg;
    if (pc) bt.d_pctl = (const float *)(d_in + i_pctl);
    bt.wave = zv::wave_bind(ask, wo, d_in, io, (const int32_t *)(io + o_nf), bands_table);
    // the arena, ahead of everything enqueued: with the stages bound (a filter adds its input region to the vocoder's layout) and the scan
    // not yet (without Batch::d_cum the encoder's layout keeps it in the arena), so one reservation asks for the largest of each
    M.reserve_batch(bt);
    // an envelope's knots pass and a table stage's phonemes pass read the scan behind the vocoder
    if (enc && (dur || bt.wave.needs_scan())) bt.d_cum = (int32_t *)(io + o_cum);
    if (r.fitted) bt.d_frm_live = (zv::Seg *)(io + o_live);
    // (a run table is the chain's: a stand-alone decode's hidden comes from the caller, Model::dec_plan)
    if (enc && sr.has(zv::ST_DECODER) && M.dec_plan(bt).runs) bt.d_dec_runs = (zv::Seg *)(io + o_runs);
    int32_t *d_nf = (int32_t *)(io + o_nf), *d_ids = (int32_t *)(d_in + i_ids), *d_pun = (int32_t *)(d_in + i_pun);
    float *d_sty = (float *)(d_in + i_sty), *d_hid = (float *)(io + o_hid), *d_mel = (float *)(io + o_mel), *d_wav = (float *)(io + o_wav);
    int32_t *h_nf = enc ? (int32_t *)(pin + p_nf) : nullptr, *h_cum = dur ? (int32_t *)(pin + p_cum) : nullptr;
    char *h_wav = pin + p_wav;
    // what the range reads from the caller and what it hands back, in the device block
    float *d_src = sr.first == zv::ST_DECODER ? d_hid : sr.first == zv::ST_VOCODER ? d_mel : nullptr;
    const char *d_out = (const char *)(sr.last == zv::ST_VOCODER ? d_wav : sr.last == zv::ST_DECODER ? d_mel : d_hid);
    // the rows of the utterances that want them, one copy per run of neighbours (the chain: every utterance, one copy)
    auto out_download = [&](hipStream_t st) {
        for (uint32_t u = 0, v; u < r.count; u = v)
        {
            for (v = u + 1; r.out[u] && v < r.count && r.out[v]; v++) {}
            if (r.out[u])
                ZV_HIP(hipMemcpyAsync(h_wav + pb.woff[u], d_out + frm0[u] * out_row, (frm0[v] - frm0[u]) * out_row, hipMemcpyDeviceToHost, st));
        }
    };
    wave_tables(r, ask, wo, io, pin, h_in, wo, pb.tables, pb.dst);      // (the struct arrays are read here, the tables are written in batch_finish)
    // the table rows of utterances [u0, u1) travel behind their waveforms on stream `st`; the per-utterance tables (whole) follow the last kernel
    auto tables_download = [&](uint32_t u0, uint32_t u1, hipStream_t st, bool whole) {
        for (const RowTable &t : pb.tables)
        {
            if ((t.rows == zv::ROWS_UTTERANCE) != whole) continue;
            const size_t a = pb.first_row(t.rows, u0), b = u1 < r.count ? pb.first_row(t.rows, u1) : zv::WaveRows{r.count, ntot, frame_rows}[t.rows];
            rows_download(t, a, b - a, t.host + a * t.dev_row, t.dev_row, st);
        }
    };
    // Large batches: the last vocoder stage (two thirds of a waveform's bytes are produced there) runs in G groups of
    // utterances; a finished group's waveforms travel to the host on the lane's copy stream while the next group's kernels
    // run.  Same kernels on the same rows: same bits.
    const int G = voc ? zv::voc_tail_groups(bt.nseg, wav_bytes, M.profiling, M.dbg_layer.kind >= 0) : 1;
    // from here on work is queued that reads the lane's pinned input block and writes its I/O block: if anything fails the
    // lane's streams are drained before the error leaves, so an idle-looking lane never has work in flight
    try
    {
        hipStream_t cs = M.copy_stream();
        pb.gb.assign(G + 1, r.count);
        pb.gb[0] = 0;
        // Batches in flight on different lanes share the GPU kernel by kernel (worth 1.4 ms per batch: the latency-bound encoder /
        // decoder launches of one fill the other's vocoder).  Every batch owns a (start, done) pair of timing events on its lane's
        // stream — zv_batch_timeline reports from them when the GPU had no batch to work on.  (Round 4 measured that number
        // without a profiler: 0.00 ms per step with two batches in flight; a device-side limit of two concurrent batches with a
        // third queued behind them, built to close gaps a kernel trace had shown, changed nothing and was removed again.)
        const uint64_t seq = M.next_batch_seq();
        ZV_HIP(hipEventRecord(M.batch_event(seq, 0), M.stream()));
        // the caller's hidden or mel, by its real size and ahead of the schedule (whose first node uploads the input block by capacity)
        if (d_src) ZV_HIP(hipMemcpyAsync(d_src, pin + p_src, q.source_bytes, hipMemcpyHostToDevice, M.stream()));
        if (G <= 1)
        {
            M.chain_dev(bt, d_ids, d_pun, d_sty, d_hid, d_mel, d_wav, d_nf, h_in, d_in, b_in, 0, sr);
            ZV_HIP(hipEventRecord(M.batch_event(seq, 1), M.stream()));
            if (enc) ZV_HIP(hipMemcpyAsync(h_nf, d_nf, (size_t)bt.nseg * 4, hipMemcpyDeviceToHost, M.stream()));
            if (dur) ZV_HIP(hipMemcpyAsync(h_cum, bt.d_cum, (size_t)ntot * 4, hipMemcpyDeviceToHost, M.stream()));
            out_download(M.stream());
            tables_download(0, r.count, M.stream(), true);
            tables_download(0, r.count, M.stream(), false);
            ZV_HIP(hipEventRecord(M.tail_event(1), M.stream()));
        }
        else
        {
            M.chain_dev(bt, d_ids, d_pun, d_sty, d_hid, d_mel, d_wav, d_nf, h_in, d_in, b_in, 1, sr);
            if (enc) ZV_HIP(hipMemcpyAsync(h_nf, d_nf, (size_t)bt.nseg * 4, hipMemcpyDeviceToHost, M.stream()));
            if (dur) ZV_HIP(hipMemcpyAsync(h_cum, bt.d_cum, (size_t)ntot * 4, hipMemcpyDeviceToHost, M.stream()));
            for (int g = 1; g < G; g++)               // contiguous groups of about wav_bytes / G each
            {
                uint32_t u = pb.gb[g - 1] + 1;
                while (u < r.count && pb.woff[u] < wav_bytes * g / G) u++;
                pb.gb[g] = std::min(u, r.count - (uint32_t)(G - g));
            }
            for (int g = 0; g < G; g++)
            {
                const uint32_t u0 = pb.gb[g], u1 = pb.gb[g + 1];
                M.vocode_tail(bt, d_mel, d_wav, (int)u0, (int)(u1 - u0));
                const size_t o0 = pb.woff[u0], o1 = u1 < r.count ? pb.woff[u1] : wav_bytes;
                ZV_HIP(hipEventRecord(M.tail_event(2 * g), M.stream()));
                ZV_HIP(hipStreamWaitEvent(cs, M.tail_event(2 * g), 0));
                ZV_HIP(hipMemcpyAsync(h_wav + o0, (const char *)d_wav + o0, o1 - o0, hipMemcpyDeviceToHost, cs));
                tables_download(u0, u1, cs, false);
                ZV_HIP(hipEventRecord(M.tail_event(2 * g + 1), cs));
            }
            ZV_HIP(hipEventRecord(M.batch_event(seq, 1), M.stream()));
            // the per-utterance rows of every group, behind the last group's kernels (batch_finish waits for the lane's stream)
            tables_download(0, r.count, M.stream(), true);
        }
    }
    catch (...)
    {
        hipStreamSynchronize(M.stream());
        if (M.copy_stream()) hipStreamSynchronize(M.copy_stream());
        throw;
    }
    pb.active = true;
    pb.range = sr;
    pb.n_utt = r.count;
    pb.G = G;
    pb.T.assign(r.T, r.T + r.count);
    pb.wav.assign(r.out, r.out + r.count);
    pb.n_frames = enc ? r.n_frames : nullptr;
    pb.h_wav = h_wav;
    pb.h_nf = h_nf;
    pb.h_cum = h_cum;
    if (enc) pb.N.assign(r.n, r.n + r.count);
    else pb.N.assign(r.count, 0);
    if (dur) pb.dur.assign(r.durations, r.durations + r.count);
    else pb.dur.clear();
}

static void batch_finish(zv_model *m, int lane)
{
    Model &M = *m->m;
    PendingBatch &pb = pending_slot(m, lane);
    if (!pb.active) zv::fail(ZV_ERR_ARG, "lane %d has no batch in flight", lane);
    M.select_lane(lane);
    try
    {
        for (int g = 0; g < pb.G; g++)
        {
            ZV_HIP(hipEventSynchronize(M.tail_event(2 * g + 1)));
            scatter_out(pb.h_wav, pb.woff.data(), pb.wav.data(), pb.T.data(), pb.hop, pb.gb[g], pb.gb[g + 1]);
        }
        M.sync();                                 // the frame counts (and, unsplit, the waveforms) travel on the lane's stream
    }
    catch (...)
    {
        // a failed wait: drain what can be drained, then give the lane up as idle (its buffers are no longer in use)
        hipStreamSynchronize(M.stream());
        if (M.copy_stream()) hipStreamSynchronize(M.copy_stream());
        pb.active = false;
        throw;
    }
    pb.active = false;
    if (pb.n_frames)
        for (uint32_t u = 0; u < pb.n_utt; u++) pb.n_frames[u] = (uint32_t)pb.h_nf[u];
    if (pb.h_cum) durations_from_cum(pb.h_cum, pb.n_utt, pb.N.data(), pb.T.data(), pb.dur.data());
    for (size_t k = 0; k < pb.tables.size(); k++)
        for (uint32_t u = 0; u < pb.n_utt; u++)
        {
            const RowTable &t = pb.tables[k];
            const RowDst &d = pb.dst[k * pb.n_utt + u];
            if (!d.p) continue;
            const char *src = t.host + pb.first_row(t.rows, u) * t.dev_row;
            const size_t count = pb.row_count(t.rows, u);
            if (d.row == t.dev_row) memcpy(d.p, src, count * d.row);
            else for (size_t i = 0; i < count; i++) memcpy((char *)d.p + i * d.row, src + i * t.dev_row, d.row);
        }
}

// how many utterances from `a` on form one launch group: up to 64 utterances / 64 Ki frames of capacity
static uint32_t batch_group_end(uint32_t a, uint32_t n_utt, const uint32_t *T)
{
    uint32_t b = a, tmax = 0;
    while (b < n_utt && b - a < 64)
    {
        const uint32_t tm = std::max(tmax, T[b]);
        if (b > a && (uint64_t)(b - a + 1) * zv::round_up((int)tm, 64) > 65536) break;
        tmax = tm;
        b++;
    }
    return b;
}

// zv_synthesize_batch*: every launch group enqueued and finished on lane 0
static zv_status synthesize_batch(zv_model *m, const Request &r)
{
      return guarded([&] {
        check_request(m, r);
        use_lane0(m);                             // refused like every synchronous call while lane 0 has a batch in flight, in the same words
        // Groups of up to 64 utterances / 64 Ki frames go through the chain as ONE launch per kernel: every tensor is
        // the row concatenation of the group, the segment tables tell the kernels where each utterance starts and ends.
        // Capacities are rounded up so that batches of similar shape replay the same captured graph.
        for (uint32_t a = 0, b; a < r.count; a = b)
        {
            b = batch_group_end(a, r.count, r.T);
            batch_enqueue(m, 0, r.slice(a, b));
            batch_finish(m, 0);
        }
    });
}

// zv_synthesize_batch_begin*: one launch group, left in flight on `lane`
static zv_status begin_batch(zv_model *m, uint32_t lane, const Request &r)
{
    return guarded([&] {
        check_request(m, r);
        if (!(lane < ZV_BATCH_LANES)) zv::fail(ZV_ERR_ARG, "%s: lane out of range", r.fn);
        if (!(r.count > 0)) zv::fail(ZV_ERR_ARG, "%s: empty batch", r.fn);
        if (batch_group_end(0, r.count, r.T) != r.count)
            zv::fail(ZV_ERR_ARG, "%s: an asynchronous batch must fit one launch group (64 utterances, 64 Ki frames of capacity)", r.fn);
        ZV_HIP(hipSetDevice(m->m->device));
        batch_enqueue(m, (int)lane, r);
    });
}

zv_status zv_synthesize_batch(zv_model *m, uint32_t n_utt, const int32_t *const *ids, const int32_t *const *puncts,
                              const float *const *styles, const uint32_t *n_phonemes, const uint32_t *T, float *const *wav,
                              uint32_t *n_frames)
{
    return synthesize_batch(m, {__func__, n_utt, ids, puncts, styles, n_phonemes, n_phonemes, T, wav, n_frames});
}

zv_status zv_synthesize_batch_prosody(zv_model *m, uint32_t n_utt, const int32_t *const *ids, const int32_t *const *puncts,
                                      const float *const *styles, const uint32_t *n_phonemes, const uint32_t *T, float *const *wav,
                                      uint32_t *n_frames, const zv_prosody *prosody)
{
    return synthesize_batch(m, {__func__, n_utt, ids, puncts, styles, n_phonemes, n_phonemes, T, wav, n_frames, prosody});
}

zv_status zv_synthesize_batch_phonemes(zv_model *m, uint32_t n_utt, const int32_t *const *ids, const int32_t *const *puncts,
                                       const float *const *styles, const uint32_t *n_phonemes, const uint32_t *T, float *const *wav,
                                       uint32_t *n_frames, const zv_prosody *prosody, const zv_phoneme_controls *phonemes,
                                       int32_t *const *durations)
{
    return synthesize_batch(m, {__func__, n_utt, ids, puncts, styles, n_phonemes, n_phonemes, T, wav, n_frames, prosody, phonemes,
                                durations});
}

zv_status zv_synthesize_batch_begin(zv_model *m, uint32_t lane, uint32_t n_utt, const int32_t *const *ids, const int32_t *const *puncts,
                                    const float *const *styles, const uint32_t *n_phonemes, const uint32_t *T, float *const *wav,
                                    uint32_t *n_frames)
{
    return begin_batch(m, lane, {__func__, n_utt, ids, puncts, styles, n_phonemes, n_phonemes, T, wav, n_frames});
}

zv_status zv_synthesize_batch_begin_prosody(zv_model *m, uint32_t lane, uint32_t n_utt, const int32_t *const *ids,
                                            const int32_t *const *puncts, const float *const *styles, const uint32_t *n_phonemes,
                                            const uint32_t *T, float *const *wav, uint32_t *n_frames, const zv_prosody *prosody)
{
    return begin_batch(m, lane, {__func__, n_utt, ids, puncts, styles, n_phonemes, n_phonemes, T, wav, n_frames, prosody});
}

zv_status zv_synthesize_batch_begin_phonemes(zv_model *m, uint32_t lane, uint32_t n_utt, const int32_t *const *ids,
                                             const int32_t *const *puncts, const float *const *styles, const uint32_t *n_phonemes,
                                             const uint32_t *T, float *const *wav, uint32_t *n_frames, const zv_prosody *prosody,
                                             const zv_phoneme_controls *phonemes, int32_t *const *durations)
{
    return begin_batch(m, lane, {__func__, n_utt, ids, puncts, styles, n_phonemes, n_phonemes, T, wav, n_frames, prosody, phonemes,
                                 durations});
}

// The fitted forms: the _phonemes requests with the flag set (NULL prosody / phonemes / durations as there).
zv_status zv_synthesize_fitted(zv_model *m, const int32_t *ids, const int32_t *puncts, const float *style, uint32_t n, uint32_t T,
                               float *wav, uint32_t *n_frames, const zv_prosody *prosody, const zv_phoneme_controls *phonemes,
                               int32_t *durations)
{
    return run_single(m, {__func__, 1, &ids, &puncts, &style, &n, &n, &T, &wav, n_frames, prosody, phonemes, &durations, true});
}

zv_status zv_synthesize_batch_fitted(zv_model *m, uint32_t n_utt, const int32_t *const *ids, const int32_t *const *puncts,
                                     const float *const *styles, const uint32_t *n_phonemes, const uint32_t *T, float *const *wav,
                                     uint32_t *n_frames, const zv_prosody *prosody, const zv_phoneme_controls *phonemes,
                                     int32_t *const *durations)
{
    return synthesize_batch(m, {__func__, n_utt, ids, puncts, styles, n_phonemes, n_phonemes, T, wav, n_frames, prosody, phonemes,
                                durations, true});
}

zv_status zv_synthesize_batch_begin_fitted(zv_model *m, uint32_t lane, uint32_t n_utt, const int32_t *const *ids,
                                           const int32_t *const *puncts, const float *const *styles, const uint32_t *n_phonemes,
                                           const uint32_t *T, float *const *wav, uint32_t *n_frames, const zv_prosody *prosody,
                                           const zv_phoneme_controls *phonemes, int32_t *const *durations)
{
    return begin_batch(m, lane, {__func__, n_utt, ids, puncts, styles, n_phonemes, n_phonemes, T, wav, n_frames, prosody, phonemes,
                                 durations, true});
}

// The target forms: the _phonemes / _fitted requests plus the targets (NULL / 0 = none: the request of the call without them).
zv_status zv_encode_taps_target(zv_model *m, const int32_t *ids, const int32_t *puncts, const float *style, uint32_t n,
                                uint32_t num_phonemes, uint32_t T, float *hidden, uint32_t *n_frames, float *features, float *logdur,
                                float *pitch, float *energy, int32_t *pitch_bucket, int32_t *energy_bucket, const zv_prosody *prosody,
                                const zv_phoneme_controls *phonemes, int32_t *durations, uint32_t target_frames)
{
    return run_single(m, {__func__, 1, &ids, &puncts, &style, &n, &num_phonemes, &T, &hidden, n_frames, prosody, phonemes, &durations,
                          false, &target_frames},
                      Taps{features, logdur, pitch, energy, pitch_bucket, energy_bucket});
}

zv_status zv_synthesize_target(zv_model *m, const int32_t *ids, const int32_t *puncts, const float *style, uint32_t n, uint32_t T,
                               float *wav, uint32_t *n_frames, const zv_prosody *prosody, const zv_phoneme_controls *phonemes,
                               int32_t *durations, uint32_t target_frames, int fitted)
{
    return run_single(m, {__func__, 1, &ids, &puncts, &style, &n, &n, &T, &wav, n_frames, prosody, phonemes, &durations, fitted != 0,
                          &target_frames});
}

zv_status zv_synthesize_batch_target(zv_model *m, uint32_t n_utt, const int32_t *const *ids, const int32_t *const *puncts,
                                     const float *const *styles, const uint32_t *n_phonemes, const uint32_t *T, float *const *wav,
                                     uint32_t *n_frames, const zv_prosody *prosody, const zv_phoneme_controls *phonemes,
                                     int32_t *const *durations, const uint32_t *target_frames, int fitted)
{
    return synthesize_batch(m, {__func__, n_utt, ids, puncts, styles, n_phonemes, n_phonemes, T, wav, n_frames, prosody, phonemes,
                                durations, fitted != 0, target_frames});
}

zv_status zv_synthesize_batch_begin_target(zv_model *m, uint32_t lane, uint32_t n_utt, const int32_t *const *ids,
                                           const int32_t *const *puncts, const float *const *styles, const uint32_t *n_phonemes,
                                           const uint32_t *T, float *const *wav, uint32_t *n_frames, const zv_prosody *prosody,
                                           const zv_phoneme_controls *phonemes, int32_t *const *durations,
                                           const uint32_t *target_frames, int fitted)
{
    return begin_batch(m, lane, {__func__, n_utt, ids, puncts, styles, n_phonemes, n_phonemes, T, wav, n_frames, prosody, phonemes,
                                 durations, fitted != 0, target_frames});
}

// The volume forms: the _target requests plus the volumes and the levels (both NULL: the request of the _target call).
zv_status zv_synthesize_volume(zv_model *m, const int32_t *ids, const int32_t *puncts, const float *style, uint32_t n, uint32_t T,
                               float *wav, uint32_t *n_frames, const zv_prosody *prosody, const zv_phoneme_controls *phonemes,
                               int32_t *durations, uint32_t target_frames, int fitted, const zv_volume *volume, zv_level *levels)
{
    return run_single(m, {__func__, 1, &ids, &puncts, &style, &n, &n, &T, &wav, n_frames, prosody, phonemes, &durations, fitted != 0,
                          &target_frames, volume, levels});
}

zv_status zv_synthesize_batch_volume(zv_model *m, uint32_t n_utt, const int32_t *const *ids, const int32_t *const *puncts,
                                     const float *const *styles, const uint32_t *n_phonemes, const uint32_t *T, float *const *wav,
                                     uint32_t *n_frames, const zv_prosody *prosody, const zv_phoneme_controls *phonemes,
                                     int32_t *const *durations, const uint32_t *target_frames, int fitted, const zv_volume *volume,
                                     zv_level *levels)
{
    return synthesize_batch(m, {__func__, n_utt, ids, puncts, styles, n_phonemes, n_phonemes, T, wav, n_frames, prosody, phonemes,
                                durations, fitted != 0, target_frames, volume, levels});
}

zv_status zv_synthesize_batch_begin_volume(zv_model *m, uint32_t lane, uint32_t n_utt, const int32_t *const *ids,
                                           const int32_t *const *puncts, const float *const *styles, const uint32_t *n_phonemes,
                                           const uint32_t *T, float *const *wav, uint32_t *n_frames, const zv_prosody *prosody,
                                           const zv_phoneme_controls *phonemes, int32_t *const *durations,
                                           const uint32_t *target_frames, int fitted, const zv_volume *volume, zv_level *levels)
{
    return begin_batch(m, lane, {__func__, n_utt, ids, puncts, styles, n_phonemes, n_phonemes, T, wav, n_frames, prosody, phonemes,
                                 durations, fitted != 0, target_frames, volume, levels});
}

// The envelope forms: the _volume requests plus the envelopes (NULL: the request of the _volume call).
zv_status zv_synthesize_envelope(zv_model *m, const int32_t *ids, const int32_t *puncts, const float *style, uint32_t n, uint32_t T,
                                 float *wav, uint32_t *n_frames, const zv_prosody *prosody, const zv_phoneme_controls *phonemes,
                                 int32_t *durations, uint32_t target_frames, int fitted, const zv_volume *volume, zv_level *levels,
                                 const zv_envelope *envelope)
{
    return run_single(m, {__func__, 1, &ids, &puncts, &style, &n, &n, &T, &wav, n_frames, prosody, phonemes, &durations, fitted != 0,
                          &target_frames, volume, levels, envelope});
}

zv_status zv_synthesize_batch_envelope(zv_model *m, uint32_t n_utt, const int32_t *const *ids, const int32_t *const *puncts,
                                       const float *const *styles, const uint32_t *n_phonemes, const uint32_t *T, float *const *wav,
                                       uint32_t *n_frames, const zv_prosody *prosody, const zv_phoneme_controls *phonemes,
                                       int32_t *const *durations, const uint32_t *target_frames, int fitted, const zv_volume *volume,
                                       zv_level *levels, const zv_envelope *envelope)
{
    return synthesize_batch(m, {__func__, n_utt, ids, puncts, styles, n_phonemes, n_phonemes, T, wav, n_frames, prosody, phonemes,
                                durations, fitted != 0, target_frames, volume, levels, envelope});
}

zv_status zv_synthesize_batch_begin_envelope(zv_model *m, uint32_t lane, uint32_t n_utt, const int32_t *const *ids,
                                             const int32_t *const *puncts, const float *const *styles, const uint32_t *n_phonemes,
                                             const uint32_t *T, float *const *wav, uint32_t *n_frames, const zv_prosody *prosody,
                                             const zv_phoneme_controls *phonemes, int32_t *const *durations,
                                             const uint32_t *target_frames, int fitted, const zv_volume *volume, zv_level *levels,
                                             const zv_envelope *envelope)
{
    return begin_batch(m, lane, {__func__, n_utt, ids, puncts, styles, n_phonemes, n_phonemes, T, wav, n_frames, prosody, phonemes,
                                 durations, fitted != 0, target_frames, volume, levels, envelope});
}

// The contour forms: the _envelope requests plus the contours (NULL, or no table asked for: the request of the _envelope call).
zv_status zv_synthesize_contour(zv_model *m, const int32_t *ids, const int32_t *puncts, const float *style, uint32_t n, uint32_t T,
                                float *wav, uint32_t *n_frames, const zv_prosody *prosody, const zv_phoneme_controls *phonemes,
                                int32_t *durations, uint32_t target_frames, int fitted, const zv_volume *volume, zv_level *levels,
                                const zv_envelope *envelope, const zv_contour *contour)
{
    return run_single(m, {__func__, 1, &ids, &puncts, &style, &n, &n, &T, &wav, n_frames, prosody, phonemes, &durations, fitted != 0,
                          &target_frames, volume, levels, envelope, contour});
}

zv_status zv_synthesize_batch_contour(zv_model *m, uint32_t n_utt, const int32_t *const *ids, const int32_t *const *puncts,
                                      const float *const *styles, const uint32_t *n_phonemes, const uint32_t *T, float *const *wav,
                                      uint32_t *n_frames, const zv_prosody *prosody, const zv_phoneme_controls *phonemes,
                                      int32_t *const *durations, const uint32_t *target_frames, int fitted, const zv_volume *volume,
                                      zv_level *levels, const zv_envelope *envelope, const zv_contour *contour)
{
    return synthesize_batch(m, {__func__, n_utt, ids, puncts, styles, n_phonemes, n_phonemes, T, wav, n_frames, prosody, phonemes,
                                durations, fitted != 0, target_frames, volume, levels, envelope, contour});
}

zv_status zv_synthesize_batch_begin_contour(zv_model *m, uint32_t lane, uint32_t n_utt, const int32_t *const *ids,
                                            const int32_t *const *puncts, const float *const *styles, const uint32_t *n_phonemes,
                                            const uint32_t *T, float *const *wav, uint32_t *n_frames, const zv_prosody *prosody,
                                            const zv_phoneme_controls *phonemes, int32_t *const *durations,
                                            const uint32_t *target_frames, int fitted, const zv_volume *volume, zv_level *levels,
                                            const zv_envelope *envelope, const zv_contour *contour)
{
    return begin_batch(m, lane, {__func__, n_utt, ids, puncts, styles, n_phonemes, n_phonemes, T, wav, n_frames, prosody, phonemes,
                                 durations, fitted != 0, target_frames, volume, levels, envelope, contour});
}

// The pitch forms: the _contour requests plus the pitch tracks (NULL, or no table asked for: the request of the _contour call).
zv_status zv_synthesize_pitch(zv_model *m, const int32_t *ids, const int32_t *puncts, const float *style, uint32_t n, uint32_t T,
                              float *wav, uint32_t *n_frames, const zv_prosody *prosody, const zv_phoneme_controls *phonemes,
                              int32_t *durations, uint32_t target_frames, int fitted, const zv_volume *volume, zv_level *levels,
                              const zv_envelope *envelope, const zv_contour *contour, const zv_pitch *pitch)
{
    return run_single(m, {__func__, 1, &ids, &puncts, &style, &n, &n, &T, &wav, n_frames, prosody, phonemes, &durations, fitted != 0,
                          &target_frames, volume, levels, envelope, contour, pitch});
}

zv_status zv_synthesize_batch_pitch(zv_model *m, uint32_t n_utt, const int32_t *const *ids, const int32_t *const *puncts,
                                    const float *const *styles, const uint32_t *n_phonemes, const uint32_t *T, float *const *wav,
                                    uint32_t *n_frames, const zv_prosody *prosody, const zv_phoneme_controls *phonemes,
                                    int32_t *const *durations, const uint32_t *target_frames, int fitted, const zv_volume *volume,
                                    zv_level *levels, const zv_envelope *envelope, const zv_contour *contour, const zv_pitch *pitch)
{
    return synthesize_batch(m, {__func__, n_utt, ids, puncts, styles, n_phonemes, n_phonemes, T, wav, n_frames, prosody, phonemes,
                                durations, fitted != 0, target_frames, volume, levels, envelope, contour, pitch});
}

zv_status zv_synthesize_batch_begin_pitch(zv_model *m, uint32_t lane, uint32_t n_utt, const int32_t *const *ids,
                                          const int32_t *const *puncts, const float *const *styles, const uint32_t *n_phonemes,
                                          const uint32_t *T, float *const *wav, uint32_t *n_frames, const zv_prosody *prosody,
                                          const zv_phoneme_controls *phonemes, int32_t *const *durations,
                                          const uint32_t *target_frames, int fitted, const zv_volume *volume, zv_level *levels,
                                          const zv_envelope *envelope, const zv_contour *contour, const zv_pitch *pitch)
{
    return begin_batch(m, lane, {__func__, n_utt, ids, puncts, styles, n_phonemes, n_phonemes, T, wav, n_frames, prosody, phonemes,
                                 durations, fitted != 0, target_frames, volume, levels, envelope, contour, pitch});
}

// The stand-alone passes (zv_pitch_track, zv_band_levels, zv_filter_wave): a host waveform wav[T * hop] in, one pass over it as one
// inline segment, eagerly, on lane 0, rows out.  I/O block: [waveform][rows][slab][parameter row]; of each of the T device rows of
// dev_row bytes the caller receives the first out_row.  launch(d_wav, d_rows, d_slab, d_par, segment) enqueues the pass.
extern "C++" template <typename Launch>
static void wave_pass(Model &M, const float *wav, uint32_t T, const void *par, size_t b_par, size_t dev_row, size_t slab_row, void *out,
                      size_t out_row, Launch launch)
{
    const size_t hop = M.hp.audio_hop_size, b_wav = (size_t)T * hop * 4;
    Layout L;
    const size_t o_wav = L.at(b_wav), o_rows = L.at(T * dev_row), o_slab = L.at(T * slab_row), o_par = L.at(b_par);
    char *io = (char *)M.io_scratch(L.size());
    ZV_HIP(hipMemcpyAsync(io + o_wav, wav, b_wav, hipMemcpyHostToDevice, M.stream()));
    ZV_HIP(hipMemcpyAsync(io + o_par, par, b_par, hipMemcpyHostToDevice, M.stream()));
    ZV_HIP(launch((const float *)(io + o_wav), io + o_rows, io + o_slab, (const uint32_t *)(io + o_par), zv::Segs{nullptr, 1, (int)T, zv::Seg{0, (int32_t)T, 0, 0}}));
    rows_download(RowTable{io + o_rows, dev_row, nullptr, zv::ROWS_FRAME}, 0, T, out, out_row, M.stream());
    M.sync();
}

// The stand-alone meter: a host waveform through the frames pass (wave_pass).
zv_status zv_pitch_track(zv_model *m, const float *wav, uint32_t T, const zv_pitch *pitch)
{
    return guarded([&] {
        if (!(m && wav && pitch)) zv::fail(ZV_ERR_ARG, "zv_pitch_track: null argument");
        if (!pitch->frames) zv::fail(ZV_ERR_ARG, "zv_pitch_track: pitch->frames is required");
        if (pitch->phonemes) zv::fail(ZV_ERR_ARG, "zv_pitch_track: pitch->phonemes must be NULL (a waveform has no phoneme timings)");
        Model &M = *m->m;
        zv::PitchParams q;
        try
        {
            check_T(M, T);
            q = resolve_pitch(M, *pitch);
        }
        catch (const zv::Error &e)
        {
            zv::fail(e.status, "zv_pitch_track: %s", e.what());
        }
        use_lane0(m);
        const uint32_t prow[zv::PITCH_PARAM_STRIDE] = {q.min_lag, q.max_lag, q.window, zv::level_bits(q.voiced_threshold)};
        wave_pass(M, wav, T, prow, sizeof(prow), sizeof(zv::PitchFrameRow), sizeof(zv::PitchSlabRow), pitch->frames, sizeof(zv_pitch_frame),
                  [&](const float *d_wav, char *rows, char *slab, const uint32_t *d_par, const zv::Segs &one) {
                      return zv::launch_pitch_frames(M.stream(), d_wav, slab, (zv::PitchFrameRow *)rows, d_par, one, (int)M.hp.audio_hop_size, (int)M.hp.audio_sampling_rate);
                  });
    });
}

// The bands forms: the _pitch requests plus the band levels (NULL, or no table asked for: the request of the _pitch call).
zv_status zv_synthesize_bands(zv_model *m, const int32_t *ids, const int32_t *puncts, const float *style, uint32_t n, uint32_t T,
                              float *wav, uint32_t *n_frames, const zv_prosody *prosody, const zv_phoneme_controls *phonemes,
                              int32_t *durations, uint32_t target_frames, int fitted, const zv_volume *volume, zv_level *levels,
                              const zv_envelope *envelope, const zv_contour *contour, const zv_pitch *pitch, const zv_bands *bands)
{
    return run_single(m, {__func__, 1, &ids, &puncts, &style, &n, &n, &T, &wav, n_frames, prosody, phonemes, &durations, fitted != 0,
                          &target_frames, volume, levels, envelope, contour, pitch, bands});
}

zv_status zv_synthesize_batch_bands(zv_model *m, uint32_t n_utt, const int32_t *const *ids, const int32_t *const *puncts,
                                    const float *const *styles, const uint32_t *n_phonemes, const uint32_t *T, float *const *wav,
                                    uint32_t *n_frames, const zv_prosody *prosody, const zv_phoneme_controls *phonemes,
                                    int32_t *const *durations, const uint32_t *target_frames, int fitted, const zv_volume *volume,
                                    zv_level *levels, const zv_envelope *envelope, const zv_contour *contour, const zv_pitch *pitch,
                                    const zv_bands *bands)
{
    return synthesize_batch(m, {__func__, n_utt, ids, puncts, styles, n_phonemes, n_phonemes, T, wav, n_frames, prosody, phonemes,
                                durations, fitted != 0, target_frames, volume, levels, envelope, contour, pitch, bands});
}

zv_status zv_synthesize_batch_begin_bands(zv_model *m, uint32_t lane, uint32_t n_utt, const int32_t *const *ids,
                                          const int32_t *const *puncts, const float *const *styles, const uint32_t *n_phonemes,
                                          const uint32_t *T, float *const *wav, uint32_t *n_frames, const zv_prosody *prosody,
                                          const zv_phoneme_controls *phonemes, int32_t *const *durations,
                                          const uint32_t *target_frames, int fitted, const zv_volume *volume, zv_level *levels,
                                          const zv_envelope *envelope, const zv_contour *contour, const zv_pitch *pitch,
                                          const zv_bands *bands)
{
    return begin_batch(m, lane, {__func__, n_utt, ids, puncts, styles, n_phonemes, n_phonemes, T, wav, n_frames, prosody, phonemes,
                                 durations, fitted != 0, target_frames, volume, levels, envelope, contour, pitch, bands});
}

// The filter forms: the _bands requests plus the waveform filter (NULL, or no taps anywhere: the request of the _bands call).
zv_status zv_synthesize_filter(zv_model *m, const int32_t *ids, const int32_t *puncts, const float *style, uint32_t n, uint32_t T,
                               float *wav, uint32_t *n_frames, const zv_prosody *prosody, const zv_phoneme_controls *phonemes,
                               int32_t *durations, uint32_t target_frames, int fitted, const zv_volume *volume, zv_level *levels,
                               const zv_envelope *envelope, const zv_contour *contour, const zv_pitch *pitch, const zv_bands *bands,
                               const zv_filter *filter)
{
    return run_single(m, {__func__, 1, &ids, &puncts, &style, &n, &n, &T, &wav, n_frames, prosody, phonemes, &durations, fitted != 0,
                          &target_frames, volume, levels, envelope, contour, pitch, bands, filter});
}

zv_status zv_synthesize_batch_filter(zv_model *m, uint32_t n_utt, const int32_t *const *ids, const int32_t *const *puncts,
                                     const float *const *styles, const uint32_t *n_phonemes, const uint32_t *T, float *const *wav,
                                     uint32_t *n_frames, const zv_prosody *prosody, const zv_phoneme_controls *phonemes,
                                     int32_t *const *durations, const uint32_t *target_frames, int fitted, const zv_volume *volume,
                                     zv_level *levels, const zv_envelope *envelope, const zv_contour *contour, const zv_pitch *pitch,
                                     const zv_bands *bands, const zv_filter *filter)
{
    return synthesize_batch(m, {__func__, n_utt, ids, puncts, styles, n_phonemes, n_phonemes, T, wav, n_frames, prosody, phonemes,
                                durations, fitted != 0, target_frames, volume, levels, envelope, contour, pitch, bands, filter});
}

zv_status zv_synthesize_batch_begin_filter(zv_model *m, uint32_t lane, uint32_t n_utt, const int32_t *const *ids,
                                           const int32_t *const *puncts, const float *const *styles, const uint32_t *n_phonemes,
                                           const uint32_t *T, float *const *wav, uint32_t *n_frames, const zv_prosody *prosody,
                                           const zv_phoneme_controls *phonemes, int32_t *const *durations,
                                           const uint32_t *target_frames, int fitted, const zv_volume *volume, zv_level *levels,
                                           const zv_envelope *envelope, const zv_contour *contour, const zv_pitch *pitch,
                                           const zv_bands *bands, const zv_filter *filter)
{
    return begin_batch(m, lane, {__func__, n_utt, ids, puncts, styles, n_phonemes, n_phonemes, T, wav, n_frames, prosody, phonemes,
                                 durations, fitted != 0, target_frames, volume, levels, envelope, contour, pitch, bands, filter});
}

// The stand-alone filter: a host waveform through the filter pass (wave_pass); out may be wav.
zv_status zv_filter_wave(zv_model *m, const float *wav, uint32_t T, const zv_filter *filter, float *out)
{
    return guarded([&] {
        if (!(m && wav && filter && out)) zv::fail(ZV_ERR_ARG, "zv_filter_wave: null argument");
        Model &M = *m->m;
        try
        {
            check_T(M, T);
            check_filter(*filter);
        }
        catch (const zv::Error &e)
        {
            zv::fail(e.status, "zv_filter_wave: %s", e.what());
        }
        use_lane0(m);
        std::vector<uint32_t> frow(zv::FILTER_PARAM_STRIDE);
        zv::filter_pack(filter->taps, filter->n_taps, frow.data());
        const size_t b_frame = (size_t)M.hp.audio_hop_size * 4;      // the rows of this pass: the filtered waveform, a frame each
        wave_pass(M, wav, T, frow.data(), frow.size() * 4, b_frame, 0, out, b_frame, [&](const float *d_wav, char *rows, char *, const uint32_t *d_par, const zv::Segs &one) {
            return zv::launch_filter(M.stream(), d_wav, (float *)rows, d_par, one, one, (int)M.hp.audio_hop_size);
        });
    });
}

// The design: host only, no model, no device (filter.h filter_design).
zv_status zv_filter_design(uint32_t n_bands, const uint32_t *edges, const float *gains, uint32_t n_taps, float *taps)
{
    return guarded([&] {
        if (!(gains && taps)) zv::fail(ZV_ERR_ARG, "zv_filter_design: null argument");
#if !defined(__HIP_DEVICE_COMPILE__)      // (filter.h keeps its host half out of device passes)
        if (const char *field = zv::filter_design(n_bands, edges, gains, n_taps, taps))
        {
            if (!strcmp(field, "n_bands")) zv::fail(ZV_ERR_ARG, "zv_filter_design: n_bands = %u exceeds %u", n_bands, zv::FILTER_BANDS_MAX);
            if (!strcmp(field, "n_taps")) zv::fail(ZV_ERR_ARG, "zv_filter_design: n_taps = %u must be odd and in 1 .. %u", n_taps, zv::FILTER_MAX_TAPS);
            if (!strcmp(field, "gains")) zv::fail(ZV_ERR_ARG, "zv_filter_design: gains holds a value that is negative or not finite");
            if (!edges)
                zv::fail(ZV_ERR_ARG, "zv_filter_design: edges = NULL (the default edges) needs n_bands 0 or %u, got %u", zv::FILTER_BANDS_DEFAULT, n_bands);
            zv::fail(ZV_ERR_ARG, "zv_filter_design: edges must ascend strictly and end at or below %d (edges[n_bands] = %u)", zv::FILTER_DFT / 2 + 1,
                     edges[n_bands ? n_bands : zv::FILTER_BANDS_DEFAULT]);
        }
#endif
    });
}

// The stand-alone meter: a host waveform through the frames pass (wave_pass).
zv_status zv_band_levels(zv_model *m, const float *wav, uint32_t T, const zv_bands *bands)
{
    return guarded([&] {
        if (!(m && wav && bands)) zv::fail(ZV_ERR_ARG, "zv_band_levels: null argument");
        if (!bands->frames) zv::fail(ZV_ERR_ARG, "zv_band_levels: bands->frames is required");
        if (bands->phonemes) zv::fail(ZV_ERR_ARG, "zv_band_levels: bands->phonemes must be NULL (a waveform has no phoneme timings)");
        Model &M = *m->m;
        uint32_t brow[zv::BANDS_PARAM_STRIDE];
        try
        {
            check_T(M, T);
            resolve_bands(*bands, brow);
        }
        catch (const zv::Error &e)
        {
            zv::fail(e.status, "zv_band_levels: %s", e.what());
        }
        use_lane0(m);
        const void *table = M.bands_table();
        wave_pass(M, wav, T, brow, sizeof(brow), zv::BANDS_ROW_STRIDE * 4, zv::BANDS_ROW_STRIDE * 8, bands->frames, (size_t)brow[0] * 4,
                  [&](const float *d_wav, char *rows, char *slab, const uint32_t *d_par, const zv::Segs &one) {
                      return zv::launch_bands_frames(M.stream(), d_wav, table, slab, (float *)rows, d_par, one, (int)M.hp.audio_hop_size);
                  });
    });
}

// ---- mel analysis (zv_mel_wave, zv_mel_wave_batch, zv_mel_design; the rule: mel.h): host waveforms in, their log-mel rows out,
// eagerly, on lane 0.  I/O block: [waveforms][rows][slab][parameter block][segment table], every utterance at its absolute frame row;
// one launch per kernel whatever the batch (stage_plan.h mel_plan).
struct StageArg { const char *name; const void *array; bool entries; };      // entries: a [n_utt] array of pointers, none of which may be null
static void check_stage_args(const char *fn, const zv_model *m, uint32_t n_utt, std::initializer_list<StageArg> args, const uint32_t *n_phonemes,
                             const uint32_t *T);      // (with the stage batches, below)

[[maybe_unused]] static void mel_fail(const char *fn, const char *field, const zv_mel &q, uint32_t hop, uint32_t num_mels, uint32_t rate)
{
    if (!strcmp(field, "centre")) zv::fail(ZV_ERR_ARG, "%s: mel centre = %u must be below the hop, %u", fn, q.centre, hop);
    if (!strcmp(field, "pad")) zv::fail(ZV_ERR_ARG, "%s: mel pad = %u must be 0 (zeros) or 1 (reflect)", fn, q.pad);
    if (!strcmp(field, "pad (T)")) zv::fail(ZV_ERR_ARG, "%s: mel pad = 1 (reflect) needs at least %d samples in every utterance", fn, zv::BANDS_BINS);      // (mel_run names the utterance first)
    if (!strcmp(field, "log")) zv::fail(ZV_ERR_ARG, "%s: mel log = %u must be 0 (log10), 1 (ln) or 2 (linear)", fn, q.log);
    if (!strcmp(field, "floor")) zv::fail(ZV_ERR_ARG, "%s: mel floor must be finite and >= 0", fn);
    if (!strcmp(field, "weights")) zv::fail(ZV_ERR_ARG, "%s: mel weights holds a value that is not finite", fn);
    if (!strcmp(field, "num_mels")) zv::fail(ZV_ERR_ARG, "%s: num_mels = %u must be in 1 .. %u", fn, num_mels, zv::MEL_MAX_MELS);
    if (!strcmp(field, "sampling_rate")) zv::fail(ZV_ERR_ARG, "%s: sampling_rate must be > 0", fn);
    if (!strcmp(field, "fmin_hz"))
        zv::fail(ZV_ERR_ARG, "%s: mel fmin_hz = %g must be finite, >= 0 and below fmax_hz = %g (0 = Nyquist, %g)", fn, (double)q.fmin_hz, (double)q.fmax_hz, 0.5 * rate);
    zv::fail(ZV_ERR_ARG, "%s: mel fmax_hz = %g must be finite, >= 0 and at most Nyquist, %g", fn, (double)q.fmax_hz, 0.5 * rate);
}

static void mel_run(zv_model *m, const char *fn, uint32_t n_utt, const float *const *wav, const uint32_t *T, const zv_mel *mel, float *const *out)
{
#if !defined(__HIP_DEVICE_COMPILE__)      // (mel.h keeps its host half out of device passes)
    Model &M = *m->m;
    const uint32_t hop = M.hp.audio_hop_size, nm = M.hp.audio_num_mels, rate = M.hp.audio_sampling_rate;
    if (!mel) zv::fail(ZV_ERR_ARG, "%s: mel is NULL", fn);
    if (hop < 4 || hop % 4) zv::fail(ZV_ERR_ARG, "%s: audio_hop_size = %u must be a multiple of 4", fn, hop);
    uint64_t rows = 0;
    uint32_t t_min = T[0], t_max = 0;
    for (uint32_t u = 0; u < n_utt; u++)
    {
        rows += T[u];
        t_min = std::min(t_min, T[u]);
        t_max = std::max(t_max, T[u]);
        if (mel->pad == 1u && (uint64_t)T[u] * hop < (uint64_t)zv::BANDS_BINS)
            zv::fail(ZV_ERR_ARG, "%s: utterance %u: T = %u gives %llu samples, mel pad = 1 (reflect) needs at least %d", fn, u, T[u],
                     (unsigned long long)T[u] * hop, zv::BANDS_BINS);
    }
    if (rows > (uint64_t)INT32_MAX) zv::fail(ZV_ERR_ARG, "%s: the batch holds %llu frames, more than %d", fn, (unsigned long long)rows, INT32_MAX);
    std::vector<uint32_t> par;
    const zv::MelParams q{mel->weights, mel->fmin_hz, mel->fmax_hz, mel->centre, mel->pad, mel->log, mel->floor};
    if (const char *field = zv::mel_resolve(q, rate, hop, nm, (uint64_t)t_min * hop, par)) mel_fail(fn, field, *mel, hop, nm, rate);
    use_lane0(m);
    M.mel_table();                        // (allocates and copies on first use: ahead of everything enqueued)
    std::vector<zv::Seg> segs(n_utt);
    int32_t row0 = 0;
    for (uint32_t u = 0; u < n_utt; u++)
    {
        segs[u] = zv::Seg{row0, (int32_t)T[u], 0, 0};
        row0 += (int32_t)T[u];
    }
    Layout L;
    const size_t o_wav = L.at(rows * hop * 4), o_rows = L.at(rows * nm * 4), o_slab = L.at(rows * zv::MEL_SLAB_STRIDE * 8), o_par = L.at(par.size() * 4),
                 o_seg = L.at(segs.size() * sizeof(zv::Seg));
    char *io = (char *)M.io_scratch(L.size());
    for (uint32_t u = 0; u < n_utt; u++)
        ZV_HIP(hipMemcpyAsync(io + o_wav + (size_t)segs[u].row0 * hop * 4, wav[u], (size_t)T[u] * hop * 4, hipMemcpyHostToDevice, M.stream()));
    ZV_HIP(hipMemcpyAsync(io + o_par, par.data(), par.size() * 4, hipMemcpyHostToDevice, M.stream()));
    ZV_HIP(hipMemcpyAsync(io + o_seg, segs.data(), segs.size() * sizeof(zv::Seg), hipMemcpyHostToDevice, M.stream()));
    const zv::Segs frames{n_utt > 1 ? (const zv::Seg *)(io + o_seg) : nullptr, (int)n_utt, (int)t_max, segs[0]};
    M.mel_launches((const float *)(io + o_wav), (double *)(io + o_slab), (float *)(io + o_rows), (const uint32_t *)(io + o_par), frames, (size_t)rows);
    for (uint32_t u = 0; u < n_utt; u++)
        ZV_HIP(hipMemcpyAsync(out[u], io + o_rows + (size_t)segs[u].row0 * nm * 4, (size_t)T[u] * nm * 4, hipMemcpyDeviceToHost, M.stream()));
    M.sync();                             // (par and segs are pageable: the uploads have read them by now)
#endif
}

zv_status zv_mel_wave(zv_model *m, const float *wav, uint32_t T, const zv_mel *mel, float *out)
{
    const char *fn = __func__;      // (inside the lambda __func__ is the lambda's)
    return guarded([&] {
        if (!m) zv::fail(ZV_ERR_ARG, "%s: m is NULL", fn);
        if (!wav) zv::fail(ZV_ERR_ARG, "%s: wav is NULL", fn);
        if (!out) zv::fail(ZV_ERR_ARG, "%s: out is NULL", fn);
        try
        {
            check_T(*m->m, T);
        }
        catch (const zv::Error &e)
        {
            zv::fail(e.status, "%s: %s", fn, e.what());
        }
        mel_run(m, fn, 1, &wav, &T, mel, &out);
    });
}

zv_status zv_mel_wave_batch(zv_model *m, uint32_t n_utt, const float *const *wav, const uint32_t *T, const zv_mel *mel, float *const *out)
{
    const char *fn = __func__;      // (inside the lambda __func__ is the lambda's)
    return guarded([&] {
        check_stage_args(fn, m, n_utt, {{"wav", wav, true}, {"out", out, true}}, nullptr, T);
        mel_run(m, fn, n_utt, wav, T, mel, out);
    });
}

// The design: host only, no model, no device (mel.h mel_design).
zv_status zv_mel_design(uint32_t sampling_rate, uint32_t num_mels, float fmin_hz, float fmax_hz, float *weights)
{
    const char *fn = __func__;      // (inside the lambda __func__ is the lambda's)
    return guarded([&] {
        if (!weights) zv::fail(ZV_ERR_ARG, "%s: weights is NULL", fn);
#if !defined(__HIP_DEVICE_COMPILE__)      // (mel.h keeps its host half out of device passes)
        zv_mel q{};
        q.fmin_hz = fmin_hz;
        q.fmax_hz = fmax_hz;
        if (const char *field = zv::mel_design(sampling_rate, num_mels, fmin_hz, fmax_hz, weights)) mel_fail(fn, field, q, 0, num_mels, sampling_rate);
#endif
    });
}

// ---- mel alignment (zv_mel_align, zv_mel_align_batch, zv_align_durations; the rule: align.h): host rows in, per pair the path's total,
// distance, length and maps out, eagerly, on lane 0.  A batch runs as launch groups of consecutive pairs (align_group_end), each ONE
// launch per kernel.  I/O block of a group: [rows f32][means][two digit planes][norms][cost u32][choice u8][totals][pair table], then
// [result rows][maps], which come back as ONE download.
static_assert(sizeof(zv_alignment) == sizeof(zv::AlignRow) && ZV_ALIGN_MAX_FRAMES == zv::ALIGN_MAX_FRAMES, "zv_alignment is align.h's AlignRow");

static void align_run(zv_model *m, const char *fn, bool batch, uint32_t n_pairs, const float *const *a, const uint32_t *Ta, const float *const *b,
                      const uint32_t *Tb, uint32_t Mm, const zv_align *params, zv_alignment *out, int32_t *const *map_a, int32_t *const *map_b)
{
    if (!m) zv::fail(ZV_ERR_ARG, "%s: m is NULL", fn);
    if (!a) zv::fail(ZV_ERR_ARG, "%s: a is NULL", fn);
    if (!Ta) zv::fail(ZV_ERR_ARG, "%s: Ta is NULL", fn);
    if (!b) zv::fail(ZV_ERR_ARG, "%s: b is NULL", fn);
    if (!Tb) zv::fail(ZV_ERR_ARG, "%s: Tb is NULL", fn);
    if (!params) zv::fail(ZV_ERR_ARG, "%s: params is NULL", fn);
    if (!out) zv::fail(ZV_ERR_ARG, "%s: out is NULL", fn);
    if (!n_pairs) zv::fail(ZV_ERR_ARG, "%s: n_pairs must be > 0", fn);
    if (Mm < 1 || Mm > zv::ALIGN_MAX_MELS) zv::fail(ZV_ERR_ARG, "%s: M = %u must be in 1 .. %u", fn, Mm, zv::ALIGN_MAX_MELS);
    char who[32] = "";
    for (uint32_t p = 0; p < n_pairs; p++)
    {
        if (batch) snprintf(who, sizeof who, "pair %u: ", p);
        if (!a[p]) zv::fail(ZV_ERR_ARG, "%s: %sa is NULL", fn, who);
        if (!b[p]) zv::fail(ZV_ERR_ARG, "%s: %sb is NULL", fn, who);
        if (Ta[p] < 1 || Ta[p] > zv::ALIGN_MAX_FRAMES)
            zv::fail(ZV_ERR_ARG, "%s: %sTa = %u must be in 1 .. ZV_ALIGN_MAX_FRAMES = %u", fn, who, Ta[p], zv::ALIGN_MAX_FRAMES);
        if (Tb[p] < 1 || Tb[p] > zv::ALIGN_MAX_FRAMES)
            zv::fail(ZV_ERR_ARG, "%s: %sTb = %u must be in 1 .. ZV_ALIGN_MAX_FRAMES = %u", fn, who, Tb[p], zv::ALIGN_MAX_FRAMES);
    }
    float scale = params->scale;
    if (const char *field = zv::align_resolve(scale, params->normalise))
    {
        if (!strcmp(field, "scale")) zv::fail(ZV_ERR_ARG, "%s: align scale = %g must be finite and positive (0 = %g)", fn, (double)params->scale, (double)zv::ALIGN_SCALE);
        zv::fail(ZV_ERR_ARG, "%s: align normalise = %u must be 0 or 1", fn, params->normalise);
    }
    Model &M = *m->m;
    use_lane0(m);
    const size_t K = (size_t)zv::align_k((int)Mm);
    std::vector<zv::AlignPair> pairs;
    std::vector<char> back;
    for (uint32_t g0 = 0; g0 < n_pairs;)
    {
        const uint32_t g1 = zv::align_group_end(g0, n_pairs, Ta, Tb), n = g1 - g0;
        pairs.resize(n);
        size_t rows = 0, cells = 0, maps = 0;
        uint32_t max_ta = 0, max_tb = 0;
        for (uint32_t k = 0; k < n; k++)
        {
            const uint32_t ta = Ta[g0 + k], tb = Tb[g0 + k];
            pairs[k] = zv::AlignPair{(int32_t)ta, (int32_t)tb, (int32_t)rows, (int32_t)(rows + ta), (int32_t)maps, 0, (uint64_t)cells};
            rows += (size_t)ta + tb;
            maps += (size_t)ta + tb;
            cells += (size_t)ta * tb;
            max_ta = std::max(max_ta, ta);
            max_tb = std::max(max_tb, tb);
        }
        Layout L;
        const size_t o_x = L.at(rows * Mm * 4), o_mean = L.at((size_t)2 * n * zv::ALIGN_MAX_MELS * 4), o_hi = L.at(rows * K), o_lo = L.at(rows * K),
                     o_norm = L.at(rows * 4), o_cost = L.at(cells * 4), o_ch = L.at(cells), o_tot = L.at((size_t)n * 8),
                     o_pair = L.at((size_t)n * sizeof(zv::AlignPair)), o_row = L.at((size_t)n * sizeof(zv::AlignRow)), o_map = L.at(maps * 4);
        const size_t b_back = o_map + maps * 4 - o_row;
        char *io = (char *)M.io_scratch(L.size());
        for (uint32_t k = 0; k < n; k++)
        {
            ZV_HIP(hipMemcpyAsync(io + o_x + (size_t)pairs[k].row_a * Mm * 4, a[g0 + k], (size_t)pairs[k].Ta * Mm * 4, hipMemcpyHostToDevice, M.stream()));
            ZV_HIP(hipMemcpyAsync(io + o_x + (size_t)pairs[k].row_b * Mm * 4, b[g0 + k], (size_t)pairs[k].Tb * Mm * 4, hipMemcpyHostToDevice, M.stream()));
        }
        ZV_HIP(hipMemcpyAsync(io + o_pair, pairs.data(), (size_t)n * sizeof(zv::AlignPair), hipMemcpyHostToDevice, M.stream()));
        const zv::AlignJob job{(const float *)(io + o_x), (int32_t *)(io + o_mean), (int8_t *)(io + o_hi), (int8_t *)(io + o_lo), (int32_t *)(io + o_norm),
                               (uint32_t *)(io + o_cost), (uint8_t *)(io + o_ch), (int64_t *)(io + o_tot), (zv::AlignRow *)(io + o_row),
                               (int32_t *)(io + o_map), (const zv::AlignPair *)(io + o_pair), (int)n, (int)max_ta, (int)max_tb, (int)Mm, scale,
                               params->normalise};
        M.align_launches(job, rows, cells);
        back.resize(b_back);
        ZV_HIP(hipMemcpyAsync(back.data(), io + o_row, b_back, hipMemcpyDeviceToHost, M.stream()));
        M.sync();                             // (pairs and back are pageable and reused by the next group)
        const zv::AlignRow *res = (const zv::AlignRow *)back.data();
        const int32_t *mp = (const int32_t *)(back.data() + (o_map - o_row));
        for (uint32_t k = 0; k < n; k++)
        {
            out[g0 + k] = zv_alignment{res[k].total, res[k].distance, res[k].path_len, 0};
            if (map_a && map_a[g0 + k]) memcpy(map_a[g0 + k], mp + pairs[k].map0, (size_t)pairs[k].Ta * 4);
            if (map_b && map_b[g0 + k]) memcpy(map_b[g0 + k], mp + pairs[k].map0 + pairs[k].Ta, (size_t)pairs[k].Tb * 4);
        }
        g0 = g1;
    }
}

zv_status zv_mel_align(zv_model *m, const float *a, uint32_t Ta, const float *b, uint32_t Tb, uint32_t M, const zv_align *params,
                       zv_alignment *out, int32_t *map_a, int32_t *map_b)
{
    const char *fn = __func__;      // (inside the lambda __func__ is the lambda's)
    return guarded([&] {
        if (!a) zv::fail(ZV_ERR_ARG, "%s: a is NULL", fn);
        if (!b) zv::fail(ZV_ERR_ARG, "%s: b is NULL", fn);
        align_run(m, fn, false, 1, &a, &Ta, &b, &Tb, M, params, out, &map_a, &map_b);
    });
}

zv_status zv_mel_align_batch(zv_model *m, uint32_t n_pairs, const float *const *a, const uint32_t *Ta, const float *const *b, const uint32_t *Tb,
                             uint32_t M, const zv_align *params, zv_alignment *out, int32_t *const *map_a, int32_t *const *map_b)
{
    const char *fn = __func__;      // (inside the lambda __func__ is the lambda's)
    return guarded([&] { align_run(m, fn, true, n_pairs, a, Ta, b, Tb, M, params, out, map_a, map_b); });
}

// The timing transfer: host only, no model, no device (align.h align_durations).
zv_status zv_align_durations(uint32_t n, const int32_t *durations_a, uint32_t Ta, const int32_t *map_a, uint32_t Tb, int32_t *durations_b)
{
    const char *fn = __func__;      // (inside the lambda __func__ is the lambda's)
    return guarded([&] {
        if (!durations_a) zv::fail(ZV_ERR_ARG, "%s: durations_a is NULL", fn);
        if (!map_a) zv::fail(ZV_ERR_ARG, "%s: map_a is NULL", fn);
        if (!durations_b) zv::fail(ZV_ERR_ARG, "%s: durations_b is NULL", fn);
        if (!n) zv::fail(ZV_ERR_ARG, "%s: n must be > 0", fn);
        if (!Ta || !Tb) zv::fail(ZV_ERR_ARG, "%s: Ta = %u and Tb = %u must be > 0", fn, Ta, Tb);
        const char *field = zv::align_durations(n, durations_a, Ta, map_a, Tb, durations_b);
        if (!field) return;
        if (!strcmp(field, "durations_a")) zv::fail(ZV_ERR_ARG, "%s: durations_a holds a negative duration", fn);
        if (!strcmp(field, "sum")) zv::fail(ZV_ERR_ARG, "%s: the sum of durations_a must be Ta = %u", fn, Ta);
        zv::fail(ZV_ERR_ARG, "%s: map_a must be non-decreasing inside [0, Tb = %u)", fn, Tb);
    });
}

// ---- loudness (zv_loudness_wave, zv_loudness_wave_batch, zv_loudness_design; the rule: loudness.h): host waveforms in, per utterance
// the BS.1770 result and (where asked) the scaled waveform out, eagerly, on lane 0.  A batch runs as launch groups of consecutive
// utterances (loud_group_end), each ONE launch per kernel.  I/O block of a group: [samples, every utterance on whole chunks][states][runs]
// [step energies][blocks][peaks][segment table][asks][design][result rows].
static_assert(sizeof(zv_loudness_result) == sizeof(zv::LoudRow) && sizeof(zv_loudness_filter) == sizeof(zv::LoudFilter) &&
                  offsetof(zv_loudness_filter, interp) == offsetof(zv::LoudFilter, c) && offsetof(zv_loudness_result, gain) == offsetof(zv::LoudRow, gain) &&
                  ZV_LOUDNESS_TARGET == zv::LOUD_FLAG_TARGET && ZV_LOUDNESS_CEILING == zv::LOUD_FLAG_CEILING,
              "zv_loudness_result is loudness.h's LoudRow, zv_loudness_filter its LoudFilter");

static void check_loudness(const char *fn, const char *who, const zv_loudness &q)
{
    const char *field = zv::loud_check(q.gain, q.target_lufs, q.true_peak_ceiling, q.flags);
    if (!field) return;
    if (!strcmp(field, "flags")) zv::fail(ZV_ERR_ARG, "%s: %sloudness flags = %u holds bits other than 0 (target) and 1 (ceiling)", fn, who, q.flags);
    const float v = !strcmp(field, "gain") ? q.gain : !strcmp(field, "target_lufs") ? q.target_lufs : q.true_peak_ceiling;
    if (!std::isfinite(v)) zv::fail(ZV_ERR_ARG, "%s: %sloudness %s = %g is not finite", fn, who, field, (double)v);
    if (!strcmp(field, "gain")) zv::fail(ZV_ERR_ARG, "%s: %sloudness gain = %g is outside [0, 1000]", fn, who, (double)v);
    if (!strcmp(field, "target_lufs")) zv::fail(ZV_ERR_ARG, "%s: %sloudness target_lufs = %g is outside [-70, 0]", fn, who, (double)v);
    zv::fail(ZV_ERR_ARG, "%s: %sloudness true_peak_ceiling = %g is outside (0, 1]", fn, who, (double)v);
}

// the checks that need no model: res, then every utterance's ask by field
static void check_loud_args(const char *fn, bool batch, uint32_t n_utt, const zv_loudness *ask, const zv_loudness_result *res)
{
    if (!res) zv::fail(ZV_ERR_ARG, "%s: res is NULL", fn);
    char who[32] = "";
    for (uint32_t u = 0; ask && u < n_utt; u++)
    {
        if (batch) snprintf(who, sizeof who, "utterance %u: ", u);
        check_loudness(fn, who, ask[u]);
    }
}

static void loud_run(zv_model *m, const char *fn, uint32_t n_utt, const float *const *wav, const uint32_t *T, const uint32_t *n_frames,
                     const zv_loudness *ask, zv_loudness_result *res, float *const *out)
{
#if !defined(__HIP_DEVICE_COMPILE__)      // (loudness.h keeps its host half out of device passes)
    Model &M = *m->m;
    const uint32_t hop = M.hp.audio_hop_size, rate = M.hp.audio_sampling_rate;
    zv::LoudFilter F;
    if (zv::loud_design(rate, &F))
        zv::fail(ZV_ERR_ARG, "%s: audio_sampling_rate = %u must be in %u .. %u", fn, rate, zv::LOUD_MIN_RATE, zv::LOUD_MAX_RATE);
    use_lane0(m);
    static const zv_loudness identity = {1.0f, 0.0f, 0.0f, 0u};
    std::vector<zv::LoudSeg> segs;
    std::vector<zv::LoudAsk> asks;
    std::vector<zv::LoudRow> rows;
    for (uint32_t g0 = 0; g0 < n_utt;)
    {
        const uint32_t g1 = zv::loud_group_end(g0, n_utt, T, hop), n = g1 - g0;
        segs.resize(n);
        asks.resize(n);
        rows.resize(n);
        int64_t x0 = 0, max_N = 0, max_total = 0;
        size_t chunks = 0, steps = 0, tiles = 0, measured = 0, capacity = 0;
        bool apply = false;
        for (uint32_t k = 0; k < n; k++)
        {
            const uint32_t u = g0 + k, nf = n_frames ? std::min(n_frames[u], T[u]) : T[u];
            const int64_t N = (int64_t)nf * hop, total = (int64_t)T[u] * hop;
            segs[k] = zv::LoudSeg{x0, N, total, (int32_t)chunks, (int32_t)steps, (int32_t)tiles, 0};
            const zv_loudness &q = ask ? ask[u] : identity;
            asks[k] = zv::loud_ask(q.gain, q.target_lufs, q.true_peak_ceiling, q.flags);
            x0 += (int64_t)zv::loud_padded((uint64_t)total);
            chunks += (size_t)zv::loud_chunks(N);
            steps += (size_t)(N / F.step);
            tiles += (size_t)zv::loud_tp_tiles(N);
            max_N = std::max(max_N, N);
            max_total = std::max(max_total, total);
            measured += (size_t)N;
            capacity += (size_t)total;
            apply = apply || (out && out[u]);
        }
        Layout L;
        const size_t o_wav = L.at((size_t)x0 * 4), o_state = L.at(chunks * 32), o_runs = L.at(chunks * 16 + 16), o_energy = L.at(steps * 8 + 8),
                     o_blocks = L.at(steps * 8 + 8), o_peaks = L.at(tiles * 16), o_seg = L.at((size_t)n * sizeof(zv::LoudSeg)),
                     o_ask = L.at((size_t)n * sizeof(zv::LoudAsk)), o_des = L.at(sizeof(zv::LoudFilter)), o_row = L.at((size_t)n * sizeof(zv::LoudRow));
        char *io = (char *)M.io_scratch(L.size());
        for (uint32_t k = 0; k < n; k++)
            ZV_HIP(hipMemcpyAsync(io + o_wav + (size_t)segs[k].x0 * 4, wav[g0 + k], (size_t)segs[k].total * 4, hipMemcpyHostToDevice, M.stream()));
        ZV_HIP(hipMemcpyAsync(io + o_seg, segs.data(), (size_t)n * sizeof(zv::LoudSeg), hipMemcpyHostToDevice, M.stream()));
        ZV_HIP(hipMemcpyAsync(io + o_ask, asks.data(), (size_t)n * sizeof(zv::LoudAsk), hipMemcpyHostToDevice, M.stream()));
        ZV_HIP(hipMemcpyAsync(io + o_des, &F, sizeof F, hipMemcpyHostToDevice, M.stream()));
        const zv::LoudJob job{(float *)(io + o_wav), (double *)(io + o_state), (double *)(io + o_runs), (double *)(io + o_energy), (double *)(io + o_blocks),
                              (uint64_t *)(io + o_peaks), (zv::LoudRow *)(io + o_row), (const zv::LoudSeg *)(io + o_seg), (const zv::LoudAsk *)(io + o_ask),
                              (const zv::LoudFilter *)(io + o_des), (int)n, max_N, max_total, F.step};
        M.loud_launches(job, apply, measured, capacity);
        ZV_HIP(hipMemcpyAsync(rows.data(), io + o_row, (size_t)n * sizeof(zv::LoudRow), hipMemcpyDeviceToHost, M.stream()));
        for (uint32_t k = 0; k < n; k++)
            if (out && out[g0 + k])
                ZV_HIP(hipMemcpyAsync(out[g0 + k], io + o_wav + (size_t)segs[k].x0 * 4, (size_t)segs[k].total * 4, hipMemcpyDeviceToHost, M.stream()));
        M.sync();                             // (segs, asks, rows and F are pageable and reused by the next group)
        for (uint32_t k = 0; k < n; k++) memcpy(&res[g0 + k], &rows[k], sizeof(zv::LoudRow));
        g0 = g1;
    }
#endif
}

zv_status zv_loudness_wave(zv_model *m, const float *wav, uint32_t T, uint32_t n_frames, const zv_loudness *ask, zv_loudness_result *res, float *out)
{
    const char *fn = __func__;      // (inside the lambda __func__ is the lambda's)
    return guarded([&] {
        if (!m) zv::fail(ZV_ERR_ARG, "%s: m is NULL", fn);
        if (!wav) zv::fail(ZV_ERR_ARG, "%s: wav is NULL", fn);
        check_loud_args(fn, false, 1, ask, res);
        try
        {
            check_T(*m->m, T);
        }
        catch (const zv::Error &e)
        {
            zv::fail(e.status, "%s: %s", fn, e.what());
        }
        loud_run(m, fn, 1, &wav, &T, &n_frames, ask, res, &out);
    });
}

zv_status zv_loudness_wave_batch(zv_model *m, uint32_t n_utt, const float *const *wav, const uint32_t *T, const uint32_t *n_frames,
                                 const zv_loudness *ask, zv_loudness_result *res, float *const *out)
{
    const char *fn = __func__;      // (inside the lambda __func__ is the lambda's)
    return guarded([&] {
        if (!m) zv::fail(ZV_ERR_ARG, "%s: m is NULL", fn);
        check_loud_args(fn, true, n_utt, ask, res);
        check_stage_args(fn, m, n_utt, {{"wav", wav, true}}, nullptr, T);
        loud_run(m, fn, n_utt, wav, T, n_frames, ask, res, out);
    });
}

// The design: host only, no model, no device (loudness.h loud_design).
zv_status zv_loudness_design(uint32_t sampling_rate, zv_loudness_filter *out)
{
    const char *fn = __func__;      // (inside the lambda __func__ is the lambda's)
    return guarded([&] {
        if (!out) zv::fail(ZV_ERR_ARG, "%s: out is NULL", fn);
#if !defined(__HIP_DEVICE_COMPILE__)      // (loudness.h keeps its host half out of device passes)
        zv::LoudFilter F;
        if (zv::loud_design(sampling_rate, &F))
            zv::fail(ZV_ERR_ARG, "%s: sampling_rate = %u must be in %u .. %u", fn, sampling_rate, zv::LOUD_MIN_RATE, zv::LOUD_MAX_RATE);
        memcpy(out, &F, sizeof F);
#endif
    });
}

// ---- limiter (zv_limit_wave, zv_limit_wave_batch, zv_limit_design; the rule: limiter.h): host waveforms in, per utterance the limited
// waveform and the report out, eagerly, on lane 0.  A batch runs as launch groups of consecutive utterances (loud_group_end), each ONE
// launch per kernel.  I/O block of a group: [samples, every utterance on whole chunks][limited samples, likewise][q, every utterance on
// whole tiles][m][peaks before][peaks after][statistics][segment table][asks][design][result rows].
static_assert(sizeof(zv_limit_result) == sizeof(zv::LimitRow) && offsetof(zv_limit_result, min_gain) == offsetof(zv::LimitRow, min_gain) &&
                  offsetof(zv_limit_result, limited_samples) == offsetof(zv::LimitRow, limited_samples),
              "zv_limit_result is limiter.h's LimitRow");

static void check_limiter(const char *fn, const char *who, const zv_limiter &q)
{
    const char *field = zv::limit_check(q.gain, q.ceiling, q.attack, q.release, q.flags);
    if (!field) return;
    if (!strcmp(field, "flags")) zv::fail(ZV_ERR_ARG, "%s: %slimiter flags = %u must be 0", fn, who, q.flags);
    if (!strcmp(field, "attack")) zv::fail(ZV_ERR_ARG, "%s: %slimiter attack = %u is outside [1, %u] samples", fn, who, q.attack, zv::LIMIT_MAX_ATTACK);
    if (!strcmp(field, "release")) zv::fail(ZV_ERR_ARG, "%s: %slimiter release = %u is outside [1, %u] samples", fn, who, q.release, zv::LIMIT_MAX_RELEASE);
    const float v = !strcmp(field, "gain") ? q.gain : q.ceiling;
    if (!std::isfinite(v)) zv::fail(ZV_ERR_ARG, "%s: %slimiter %s = %g is not finite", fn, who, field, (double)v);
    if (!strcmp(field, "gain")) zv::fail(ZV_ERR_ARG, "%s: %slimiter gain = %g is outside [0, 1000]", fn, who, (double)v);
    zv::fail(ZV_ERR_ARG, "%s: %slimiter ceiling = %g is outside (0, 1]", fn, who, (double)v);
}

// the checks that need no model: res, then every utterance's ask by field
static void check_limit_args(const char *fn, bool batch, uint32_t n_utt, const zv_limiter *ask, const zv_limit_result *res)
{
    if (!res) zv::fail(ZV_ERR_ARG, "%s: res is NULL", fn);
    char who[32] = "";
    for (uint32_t u = 0; ask && u < n_utt; u++)
    {
        if (batch) snprintf(who, sizeof who, "utterance %u: ", u);
        check_limiter(fn, who, ask[u]);
    }
}

static void limit_run(zv_model *m, const char *fn, uint32_t n_utt, const float *const *wav, const uint32_t *T, const uint32_t *n_frames,
                      const zv_limiter *ask, zv_limit_result *res, float *const *out)
{
#if !defined(__HIP_DEVICE_COMPILE__)      // (loudness.h keeps its host half out of device passes)
    Model &M = *m->m;
    const uint32_t hop = M.hp.audio_hop_size, rate = M.hp.audio_sampling_rate;
    zv::LoudFilter F;
    zv::LimitAsk identity{1.0f, 1.0f, 0u, 0u};
    if (zv::loud_design(rate, &F) || zv::limit_design(rate, 0.0f, 0.0f, &identity.attack, &identity.release))
        zv::fail(ZV_ERR_ARG, "%s: audio_sampling_rate = %u must be in %u .. %u", fn, rate, zv::LOUD_MIN_RATE, zv::LOUD_MAX_RATE);
    use_lane0(m);
    std::vector<zv::LimitSeg> segs;
    std::vector<zv::LimitAsk> asks;
    std::vector<zv::LimitRow> rows;
    for (uint32_t g0 = 0; g0 < n_utt;)
    {
        const uint32_t g1 = zv::loud_group_end(g0, n_utt, T, hop), n = g1 - g0;
        segs.resize(n);
        asks.resize(n);
        rows.resize(n);
        int64_t x0 = 0, q0 = 0, m0 = 0, max_qlen = 0, max_total = 0, max_halo = 0;
        size_t tiles = 0, stats = 0, measured = 0, capacity = 0;
        for (uint32_t k = 0; k < n; k++)
        {
            const uint32_t u = g0 + k, nf = n_frames ? std::min(n_frames[u], T[u]) : T[u];
            const int64_t N = (int64_t)nf * hop, total = (int64_t)T[u] * hop;
            asks[k] = ask ? zv::LimitAsk{ask[u].gain, ask[u].ceiling, ask[u].attack, ask[u].release} : identity;
            const int64_t H = zv::limit_halo(asks[k]), qlen = zv::limit_qlen(total, H);
            segs[k] = zv::LimitSeg{x0, N, total, q0, m0, (int32_t)tiles, (int32_t)stats};
            x0 += (int64_t)zv::loud_padded((uint64_t)total);
            q0 += zv::limit_tiles(qlen) * zv::LIMIT_TILE;
            m0 += (zv::limit_mlen(total, H) + 3) / 4 * 4;
            tiles += (size_t)zv::limit_tiles(qlen);
            stats += (size_t)zv::limit_tiles(total);
            max_qlen = std::max(max_qlen, qlen);
            max_total = std::max(max_total, total);
            max_halo = std::max(max_halo, H);
            measured += (size_t)N;
            capacity += (size_t)total;
        }
        Layout L;
        const size_t o_wav = L.at((size_t)x0 * 4), o_out = L.at((size_t)x0 * 4), o_q = L.at((size_t)q0 * 4), o_m = L.at((size_t)m0 * 4),
                     o_pb = L.at(tiles * 16), o_pa = L.at(tiles * 16), o_st = L.at(stats * 8), o_seg = L.at((size_t)n * sizeof(zv::LimitSeg)),
                     o_ask = L.at((size_t)n * sizeof(zv::LimitAsk)), o_des = L.at(sizeof(zv::LoudFilter)), o_row = L.at((size_t)n * sizeof(zv::LimitRow));
        char *io = (char *)M.io_scratch(L.size());
        for (uint32_t k = 0; k < n; k++)
            ZV_HIP(hipMemcpyAsync(io + o_wav + (size_t)segs[k].x0 * 4, wav[g0 + k], (size_t)segs[k].total * 4, hipMemcpyHostToDevice, M.stream()));
        ZV_HIP(hipMemcpyAsync(io + o_seg, segs.data(), (size_t)n * sizeof(zv::LimitSeg), hipMemcpyHostToDevice, M.stream()));
        ZV_HIP(hipMemcpyAsync(io + o_ask, asks.data(), (size_t)n * sizeof(zv::LimitAsk), hipMemcpyHostToDevice, M.stream()));
        ZV_HIP(hipMemcpyAsync(io + o_des, &F, sizeof F, hipMemcpyHostToDevice, M.stream()));
        const zv::LimitJob job{(const float *)(io + o_wav), (float *)(io + o_out), (uint32_t *)(io + o_q), (uint32_t *)(io + o_m), (uint64_t *)(io + o_pb),
                               (uint64_t *)(io + o_pa), (uint32_t *)(io + o_st), (zv::LimitRow *)(io + o_row), (const zv::LimitSeg *)(io + o_seg),
                               (const zv::LimitAsk *)(io + o_ask), (const zv::LoudFilter *)(io + o_des), (int)n, (int)max_halo, max_qlen, max_total};
        M.limit_launches(job, measured, capacity, (size_t)q0);
        ZV_HIP(hipMemcpyAsync(rows.data(), io + o_row, (size_t)n * sizeof(zv::LimitRow), hipMemcpyDeviceToHost, M.stream()));
        for (uint32_t k = 0; k < n; k++)
            ZV_HIP(hipMemcpyAsync(out[g0 + k], io + o_out + (size_t)segs[k].x0 * 4, (size_t)segs[k].total * 4, hipMemcpyDeviceToHost, M.stream()));
        M.sync();                             // (segs, asks, rows and F are pageable and reused by the next group)
        for (uint32_t k = 0; k < n; k++) memcpy(&res[g0 + k], &rows[k], sizeof(zv::LimitRow));
        g0 = g1;
    }
#endif
}

zv_status zv_limit_wave(zv_model *m, const float *wav, uint32_t T, uint32_t n_frames, const zv_limiter *ask, zv_limit_result *res, float *out)
{
    const char *fn = __func__;      // (inside the lambda __func__ is the lambda's)
    return guarded([&] {
        if (!m) zv::fail(ZV_ERR_ARG, "%s: m is NULL", fn);
        if (!wav) zv::fail(ZV_ERR_ARG, "%s: wav is NULL", fn);
        if (!out) zv::fail(ZV_ERR_ARG, "%s: out is NULL (a limiter without an output is zv_loudness_wave's true-peak meter)", fn);
        check_limit_args(fn, false, 1, ask, res);
        try
        {
            check_T(*m->m, T);
        }
        catch (const zv::Error &e)
        {
            zv::fail(e.status, "%s: %s", fn, e.what());
        }
        limit_run(m, fn, 1, &wav, &T, &n_frames, ask, res, &out);
    });
}

zv_status zv_limit_wave_batch(zv_model *m, uint32_t n_utt, const float *const *wav, const uint32_t *T, const uint32_t *n_frames,
                              const zv_limiter *ask, zv_limit_result *res, float *const *out)
{
    const char *fn = __func__;      // (inside the lambda __func__ is the lambda's)
    return guarded([&] {
        if (!m) zv::fail(ZV_ERR_ARG, "%s: m is NULL", fn);
        check_limit_args(fn, true, n_utt, ask, res);
        check_stage_args(fn, m, n_utt, {{"wav", wav, true}, {"out", out, true}}, nullptr, T);
        limit_run(m, fn, n_utt, wav, T, n_frames, ask, res, out);
    });
}

// The window lengths: host only, no model, no device (limiter.h limit_design).
zv_status zv_limit_design(uint32_t sampling_rate, float attack_ms, float release_ms, uint32_t *attack, uint32_t *release)
{
    const char *fn = __func__;      // (inside the lambda __func__ is the lambda's)
    return guarded([&] {
        if (!attack) zv::fail(ZV_ERR_ARG, "%s: attack is NULL", fn);
        if (!release) zv::fail(ZV_ERR_ARG, "%s: release is NULL", fn);
        const char *field = zv::limit_design(sampling_rate, attack_ms, release_ms, attack, release);
        if (!field) return;
        if (!strcmp(field, "sampling_rate"))
            zv::fail(ZV_ERR_ARG, "%s: sampling_rate = %u must be in %u .. %u", fn, sampling_rate, zv::LOUD_MIN_RATE, zv::LOUD_MAX_RATE);
        zv::fail(ZV_ERR_ARG, "%s: %s = %g must be finite and >= 0 (0: the default)", fn, field, (double)(!strcmp(field, "attack_ms") ? attack_ms : release_ms));
    });
}

// ---- resampling (zv_resample_wave, zv_resample_wave_batch, zv_resample_design, zv_resample_count; the rule: resample.h): host waveforms
// in, per utterance the waveform at the other rate (f32, PCM16 or both) and the report out, eagerly, on lane 0.  A batch runs as launch
// groups of consecutive utterances (resample_group_end), each ONE launch per kernel.  I/O block of a group: [inputs, every utterance on
// whole chunks][f32 outputs, likewise][PCM16 outputs][table][statistics][segment table][result rows].
static_assert(sizeof(zv_resample_result) == sizeof(zv::ResampleRow) && offsetof(zv_resample_result, sample_peak) == offsetof(zv::ResampleRow, sample_peak),
              "zv_resample_result is resample.h's ResampleRow");

[[maybe_unused]] static void resample_design_fail(const char *fn, const char *field, uint32_t rate_in, uint32_t rate_out, uint32_t zeros, float beta, float cutoff)
{
    const uint32_t g = zv::resample_gcd(rate_in, rate_out), L = g ? rate_out / g : 0, M = g ? rate_in / g : 0;
    if (!strcmp(field, "rate_in") || !strcmp(field, "rate_out"))
        zv::fail(ZV_ERR_ARG, "%s: resample %s = %u must be in %u .. %u", fn, field, !strcmp(field, "rate_in") ? rate_in : rate_out, zv::RESAMPLE_MIN_RATE,
                 zv::RESAMPLE_MAX_RATE);
    if (!strcmp(field, "L") || !strcmp(field, "M"))
        zv::fail(ZV_ERR_ARG, "%s: resample %s = %u exceeds %u (rates %u -> %u: L = %u, M = %u)", fn, field, !strcmp(field, "L") ? L : M, zv::RESAMPLE_MAX_L,
                 rate_in, rate_out, L, M);
    if (!strcmp(field, "ratio")) zv::fail(ZV_ERR_ARG, "%s: resample ratio %u : %u exceeds %u", fn, L, M, zv::RESAMPLE_MAX_RATIO);
    if (!strcmp(field, "zeros")) zv::fail(ZV_ERR_ARG, "%s: resample zeros = %u is outside %u .. %u (0: the default)", fn, zeros, zv::RESAMPLE_MIN_ZEROS, zv::RESAMPLE_MAX_ZEROS);
    if (!strcmp(field, "beta")) zv::fail(ZV_ERR_ARG, "%s: resample beta = %g is outside (0, 20] (0: the default)", fn, (double)beta);
    if (!strcmp(field, "cutoff")) zv::fail(ZV_ERR_ARG, "%s: resample cutoff = %g is outside (0, 1] (0: the default)", fn, (double)cutoff);
    if (!strcmp(field, "P")) zv::fail(ZV_ERR_ARG, "%s: resample P exceeds %u taps per phase at zeros = %u and ratio %u : %u", fn, zv::RESAMPLE_MAX_P, zeros, L, M);
    zv::fail(ZV_ERR_ARG, "%s: resample table size L * P exceeds %u entries (L = %u)", fn, zv::RESAMPLE_MAX_TABLE, L);
}

// the checks of an ask that need no model
static void check_resample_ask(const char *fn, const zv_resample *q, const zv_resample_result *res)
{
    if (!q) zv::fail(ZV_ERR_ARG, "%s: ask is NULL", fn);
    if (!res) zv::fail(ZV_ERR_ARG, "%s: res is NULL", fn);
    if (q->flags & ~zv::RESAMPLE_FLAG_DITHER) zv::fail(ZV_ERR_ARG, "%s: resample flags = %u holds bits other than bit 0 (dither)", fn, q->flags);
    if (!q->table) return;
    const char *field = zv::resample_check_table(q->table, q->L, q->M, q->P);
    if (!field) return;
    if (!strcmp(field, "gcd")) zv::fail(ZV_ERR_ARG, "%s: resample L = %u and M = %u have a common divisor (gcd must be 1)", fn, q->L, q->M);
    if (!strcmp(field, "table")) zv::fail(ZV_ERR_ARG, "%s: resample table holds an entry that is not finite", fn);
    if (!strcmp(field, "ratio")) zv::fail(ZV_ERR_ARG, "%s: resample ratio %u : %u exceeds %u", fn, q->L, q->M, zv::RESAMPLE_MAX_RATIO);
    if (!strcmp(field, "table size")) zv::fail(ZV_ERR_ARG, "%s: resample table size L * P = %u exceeds %u entries", fn, q->L * q->P, zv::RESAMPLE_MAX_TABLE);
    if (!strcmp(field, "P")) zv::fail(ZV_ERR_ARG, "%s: resample P = %u must be even and in 2 .. %u", fn, q->P, zv::RESAMPLE_MAX_P);
    zv::fail(ZV_ERR_ARG, "%s: resample %s = %u is outside 1 .. %u", fn, field, !strcmp(field, "L") ? q->L : q->M, zv::RESAMPLE_MAX_L);
}

static void resample_run(zv_model *m, const char *fn, bool batch, uint32_t n_utt, const float *const *wav, const uint64_t *S_in, const zv_resample *ask,
                         zv_resample_result *res, float *const *out, int16_t *const *pcm)
{
#if !defined(__HIP_DEVICE_COMPILE__)      // (resample.h keeps its host half out of device passes)
    Model &M = *m->m;
    const uint64_t smax = (uint64_t)M.max_frames_per_utterance() * M.hp.audio_hop_size;
    char who[32] = "";
    for (uint32_t u = 0; u < n_utt; u++)
    {
        if (batch) snprintf(who, sizeof who, "utterance %u: ", u);
        if (S_in[u] < 1 || S_in[u] > smax)
            zv::fail(ZV_ERR_ARG, "%s: %sS_in = %llu is outside 1 .. zv_max_frames() * hop = %llu samples", fn, who, (unsigned long long)S_in[u], (unsigned long long)smax);
    }
    uint32_t L = ask->L, Mq = ask->M, P = ask->P;
    const float *table = ask->table;
    if (!table)
    {
        const Model::ResampleDesign *found = nullptr;
        for (const Model::ResampleDesign &d : M.resample_designs)
            if (d.rate_in == ask->rate_in && d.rate_out == ask->rate_out && d.zeros == ask->zeros && !memcmp(&d.beta, &ask->beta, 4) && !memcmp(&d.cutoff, &ask->cutoff, 4))
                found = &d;
        if (!found)
        {
            Model::ResampleDesign d{ask->rate_in, ask->rate_out, ask->zeros, ask->beta, ask->cutoff, 0, 0, 0, {}};
            const char *field = zv::resample_design(d.rate_in, d.rate_out, d.zeros, d.beta, d.cutoff, &d.L, &d.M, &d.P, nullptr);
            if (field) resample_design_fail(fn, field, d.rate_in, d.rate_out, d.zeros, d.beta, d.cutoff);
            d.table.resize((size_t)d.L * d.P);
            zv::resample_design(d.rate_in, d.rate_out, d.zeros, d.beta, d.cutoff, &d.L, &d.M, &d.P, d.table.data());
            if (M.resample_designs.size() >= 16) M.resample_designs.erase(M.resample_designs.begin());
            M.resample_designs.push_back(std::move(d));
            found = &M.resample_designs.back();
        }
        L = found->L, Mq = found->M, P = found->P, table = found->table.data();
    }
    use_lane0(m);
    std::vector<zv::ResampleSeg> segs;
    std::vector<zv::ResampleRow> rows;
    for (uint32_t g0 = 0; g0 < n_utt;)
    {
        const uint32_t g1 = zv::resample_group_end(g0, n_utt, S_in, L, Mq), n = g1 - g0;
        segs.resize(n);
        rows.resize(n);
        int64_t x0 = 0, y0 = 0, max_n_out = 0;
        size_t tiles = 0;
        const int tile = zv::resample_tile_outputs(zv::resample_tile(L, Mq, P));
        for (uint32_t k = 0; k < n; k++)
        {
            const uint32_t u = g0 + k;
            const int64_t n_out = (int64_t)zv::resample_count(S_in[u], L, Mq);
            segs[k] = zv::ResampleSeg{x0, (int64_t)S_in[u], y0, n_out, (int32_t)tiles, ask->seed + u};
            x0 += (int64_t)zv::loud_padded(S_in[u]);
            y0 += (int64_t)zv::loud_padded((uint64_t)n_out);
            tiles += (size_t)zv::resample_tiles(n_out, tile);
            max_n_out = std::max(max_n_out, n_out);
        }
        Layout Lo;
        const size_t o_wav = Lo.at((size_t)x0 * 4), o_out = Lo.at(out ? (size_t)y0 * 4 : 0), o_pcm = Lo.at(pcm ? (size_t)y0 * 2 : 0),
                     o_tab = Lo.at((size_t)L * P * 4), o_st = Lo.at(tiles * 8), o_seg = Lo.at((size_t)n * sizeof(zv::ResampleSeg)),
                     o_row = Lo.at((size_t)n * sizeof(zv::ResampleRow));
        char *io = (char *)M.io_scratch(Lo.size());
        for (uint32_t k = 0; k < n; k++)
            ZV_HIP(hipMemcpyAsync(io + o_wav + (size_t)segs[k].x0 * 4, wav[g0 + k], (size_t)segs[k].S_in * 4, hipMemcpyHostToDevice, M.stream()));
        ZV_HIP(hipMemcpyAsync(io + o_tab, table, (size_t)L * P * 4, hipMemcpyHostToDevice, M.stream()));
        ZV_HIP(hipMemcpyAsync(io + o_seg, segs.data(), (size_t)n * sizeof(zv::ResampleSeg), hipMemcpyHostToDevice, M.stream()));
        const zv::ResampleJob job{(const float *)(io + o_wav), out ? (float *)(io + o_out) : nullptr, pcm ? (int16_t *)(io + o_pcm) : nullptr,
                                  (const float *)(io + o_tab), (uint32_t *)(io + o_st), (zv::ResampleRow *)(io + o_row), (const zv::ResampleSeg *)(io + o_seg),
                                  (int)n, L, Mq, P, ask->flags, max_n_out};
        M.resample_launches(job, (size_t)x0, (size_t)y0);
        ZV_HIP(hipMemcpyAsync(rows.data(), io + o_row, (size_t)n * sizeof(zv::ResampleRow), hipMemcpyDeviceToHost, M.stream()));
        for (uint32_t k = 0; k < n; k++)
        {
            if (out) ZV_HIP(hipMemcpyAsync(out[g0 + k], io + o_out + (size_t)segs[k].y0 * 4, (size_t)segs[k].n_out * 4, hipMemcpyDeviceToHost, M.stream()));
            if (pcm) ZV_HIP(hipMemcpyAsync(pcm[g0 + k], io + o_pcm + (size_t)segs[k].y0 * 2, (size_t)segs[k].n_out * 2, hipMemcpyDeviceToHost, M.stream()));
        }
        M.sync();                             // (segs and rows are pageable and reused by the next group)
        for (uint32_t k = 0; k < n; k++) memcpy(&res[g0 + k], &rows[k], sizeof(zv::ResampleRow));
        g0 = g1;
    }
#endif
}

uint64_t zv_resample_count(uint64_t S_in, uint32_t L, uint32_t M) { return zv::resample_count(S_in, L, M); }

zv_status zv_resample_wave(zv_model *m, const float *wav, uint64_t S_in, const zv_resample *ask, zv_resample_result *res, float *out, int16_t *pcm)
{
    const char *fn = __func__;      // (inside the lambda __func__ is the lambda's)
    return guarded([&] {
        if (!m) zv::fail(ZV_ERR_ARG, "%s: m is NULL", fn);
        if (!wav) zv::fail(ZV_ERR_ARG, "%s: wav is NULL", fn);
        if (!out && !pcm) zv::fail(ZV_ERR_ARG, "%s: out and pcm are both NULL (give at least one)", fn);
        check_resample_ask(fn, ask, res);
        resample_run(m, fn, false, 1, &wav, &S_in, ask, res, out ? &out : nullptr, pcm ? &pcm : nullptr);
    });
}

zv_status zv_resample_wave_batch(zv_model *m, uint32_t n_utt, const float *const *wav, const uint64_t *S_in, const zv_resample *ask,
                                 zv_resample_result *res, float *const *out, int16_t *const *pcm)
{
    const char *fn = __func__;      // (inside the lambda __func__ is the lambda's)
    return guarded([&] {
        if (!m) zv::fail(ZV_ERR_ARG, "%s: m is NULL", fn);
        if (!wav) zv::fail(ZV_ERR_ARG, "%s: wav is NULL", fn);
        if (!S_in) zv::fail(ZV_ERR_ARG, "%s: S_in is NULL", fn);
        if (!n_utt) zv::fail(ZV_ERR_ARG, "%s: n_utt must be > 0", fn);
        if (!out && !pcm) zv::fail(ZV_ERR_ARG, "%s: out and pcm are both NULL (give at least one)", fn);
        check_resample_ask(fn, ask, res);
        for (uint32_t u = 0; u < n_utt; u++)
        {
            if (!wav[u]) zv::fail(ZV_ERR_ARG, "%s: utterance %u: wav is NULL", fn, u);
            if (out && !out[u]) zv::fail(ZV_ERR_ARG, "%s: utterance %u: out is NULL", fn, u);
            if (pcm && !pcm[u]) zv::fail(ZV_ERR_ARG, "%s: utterance %u: pcm is NULL", fn, u);
        }
        resample_run(m, fn, true, n_utt, wav, S_in, ask, res, out, pcm);
    });
}

// The table: host only, no model, no device (resample.h resample_design).
zv_status zv_resample_design(uint32_t rate_in, uint32_t rate_out, uint32_t zeros, float beta, float cutoff, uint32_t *L, uint32_t *M, uint32_t *P,
                             float *table)
{
    const char *fn = __func__;      // (inside the lambda __func__ is the lambda's)
    return guarded([&] {
        if (!L) zv::fail(ZV_ERR_ARG, "%s: L is NULL", fn);
        if (!M) zv::fail(ZV_ERR_ARG, "%s: M is NULL", fn);
        if (!P) zv::fail(ZV_ERR_ARG, "%s: P is NULL", fn);
#if !defined(__HIP_DEVICE_COMPILE__)      // (resample.h keeps its host half out of device passes)
        const char *field = zv::resample_design(rate_in, rate_out, zeros, beta, cutoff, L, M, P, table);
        if (field) resample_design_fail(fn, field, rate_in, rate_out, zeros, beta, cutoff);
#endif
    });
}

zv_status zv_synthesize_batch_end(zv_model *m, uint32_t lane)
{
    return guarded([&] {
        ZV_NEED(m, "null argument");
        ZV_NEED(lane < ZV_BATCH_LANES, "lane out of range");
        if (m->pending && m->pending[lane].active && !m->pending[lane].range.full())
            zv::fail(ZV_ERR_ARG, "zv_synthesize_batch_end: lane %u holds a vocode batch (zv_vocode_batch_begin): finish it with zv_vocode_batch_end", lane);
        ZV_HIP(hipSetDevice(m->m->device));
        batch_finish(m, (int)lane);
    });
}

// ---- the stages in batches (zv_encode_batch, zv_decode_batch, zv_vocode_batch*): the batch request path with a stage range of one
// stage.  A call's own checks name the argument as the header does; check_request follows with the ids and the controls.
static void check_stage_args(const char *fn, const zv_model *m, uint32_t n_utt, std::initializer_list<StageArg> args, const uint32_t *n_phonemes,
                             const uint32_t *T)
{
    if (!m) zv::fail(ZV_ERR_ARG, "%s: m is NULL", fn);
    for (const StageArg &a : args)
        if (!a.array) zv::fail(ZV_ERR_ARG, "%s: %s is NULL", fn, a.name);
    if (!T) zv::fail(ZV_ERR_ARG, "%s: T is NULL", fn);
    if (!n_utt) zv::fail(ZV_ERR_ARG, "%s: n_utt must be > 0", fn);
    const uint32_t tmax = m->m->max_frames_per_utterance();
    for (uint32_t u = 0; u < n_utt; u++)
    {
        for (const StageArg &a : args)
            if (a.entries && !((const void *const *)a.array)[u]) zv::fail(ZV_ERR_ARG, "%s: utterance %u: %s is NULL", fn, u, a.name);
        if (n_phonemes && !n_phonemes[u]) zv::fail(ZV_ERR_ARG, "%s: utterance %u: n_phonemes must be > 0", fn, u);
        if (!T[u]) zv::fail(ZV_ERR_ARG, "%s: utterance %u: T must be > 0", fn, u);
        if (T[u] > tmax) zv::fail(ZV_ERR_ARG, "%s: utterance %u: T = %u exceeds zv_max_frames() = %u frames per utterance", fn, u, T[u], tmax);
    }
}

zv_status zv_encode_batch(zv_model *m, uint32_t n_utt, const int32_t *const *ids, const int32_t *const *puncts,
                          const float *const *styles, const uint32_t *n_phonemes, const uint32_t *T, float *const *hidden,
                          uint32_t *n_frames, const zv_prosody *prosody, const zv_phoneme_controls *phonemes,
                          int32_t *const *durations, const uint32_t *target_frames)
{
    const char *fn = __func__;      // (inside the lambda __func__ is the lambda's)
    std::vector<float *> none;      // hidden == NULL: the planning call, no utterance's hidden leaves the device
    zv_status st = guarded([&] {
        check_stage_args(fn, m, n_utt, {{"ids", ids, true}, {"puncts", puncts, true}, {"styles", styles, true}, {"n_phonemes", n_phonemes, false},
                                              {"n_frames", n_frames, false}}, n_phonemes, T);
        if (!hidden) none.assign(n_utt, nullptr);
    });
    if (st != ZV_OK) return st;
    Request r{__func__, n_utt, ids, puncts, styles, n_phonemes, n_phonemes, T, hidden ? hidden : none.data(), n_frames, prosody, phonemes,
              durations, false, target_frames};
    r.range = zv::StageRange{zv::ST_ENCODER, zv::ST_ENCODER};
    return synthesize_batch(m, r);
}

zv_status zv_decode_batch(zv_model *m, uint32_t n_utt, const float *const *hidden, const float *const *styles, const uint32_t *T,
                          float *const *mel)
{
    const char *fn = __func__;      // (inside the lambda __func__ is the lambda's)
    zv_status st = guarded([&] { check_stage_args(fn, m, n_utt, {{"hidden", hidden, true}, {"styles", styles, true}, {"mel", mel, true}}, nullptr, T); });
    if (st != ZV_OK) return st;
    Request r{__func__, n_utt, nullptr, nullptr, styles, nullptr, nullptr, T, mel};
    r.range = zv::StageRange{zv::ST_DECODER, zv::ST_DECODER};
    r.src = hidden;
    return synthesize_batch(m, r);
}

static Request vocode_request(const char *fn, uint32_t n_utt, const float *const *mel, const uint32_t *T, float *const *wav)
{
    Request r{fn, n_utt, nullptr, nullptr, nullptr, nullptr, nullptr, T, wav};
    r.range = zv::StageRange{zv::ST_VOCODER, zv::ST_VOCODER};
    r.src = mel;
    return r;
}

zv_status zv_vocode_batch(zv_model *m, uint32_t n_utt, const float *const *mel, const uint32_t *T, float *const *wav)
{
    const char *fn = __func__;      // (inside the lambda __func__ is the lambda's)
    zv_status st = guarded([&] { check_stage_args(fn, m, n_utt, {{"mel", mel, true}, {"wav", wav, true}}, nullptr, T); });
    return st != ZV_OK ? st : synthesize_batch(m, vocode_request(__func__, n_utt, mel, T, wav));
}

zv_status zv_vocode_batch_begin(zv_model *m, uint32_t lane, uint32_t n_utt, const float *const *mel, const uint32_t *T, float *const *wav)
{
    const char *fn = __func__;      // (inside the lambda __func__ is the lambda's)
    zv_status st = guarded([&] { check_stage_args(fn, m, n_utt, {{"mel", mel, true}, {"wav", wav, true}}, nullptr, T); });
    return st != ZV_OK ? st : begin_batch(m, lane, vocode_request(__func__, n_utt, mel, T, wav));
}

zv_status zv_vocode_batch_end(zv_model *m, uint32_t lane)
{
    return guarded([&] {
        ZV_NEED(m, "null argument");
        ZV_NEED(lane < ZV_BATCH_LANES, "lane out of range");
        if (m->pending && m->pending[lane].active && !m->pending[lane].range.only(zv::ST_VOCODER))
            zv::fail(ZV_ERR_ARG, "zv_vocode_batch_end: lane %u holds a synthesize batch (zv_synthesize_batch_begin): finish it with zv_synthesize_batch_end", lane);
        ZV_HIP(hipSetDevice(m->m->device));
        batch_finish(m, (int)lane);
    });
}

zv_status zv_batch_timeline(zv_model *m, uint32_t cap, double *start_ms, double *end_ms, uint32_t *n)
{
    return guarded([&] {
        ZV_NEED(m && start_ms && end_ms && n, "null argument");
        Model &M = *m->m;
        ZV_HIP(hipSetDevice(M.device));
        M.sync_all_lanes();
        const uint64_t total = M.batch_seq();
        const uint64_t cnt = std::min<uint64_t>(std::min<uint64_t>(cap, total), (uint64_t)Model::BATCH_RING);
        *n = (uint32_t)cnt;
        if (!cnt) return;
        const uint64_t first = total - cnt;
        hipEvent_t base = M.batch_event(first, 0);
        for (uint64_t i = 0; i < cnt; i++)
        {
            float a = 0.f, b = 0.f;
            ZV_HIP(hipEventElapsedTime(&a, base, M.batch_event(first + i, 0)));
            ZV_HIP(hipEventElapsedTime(&b, base, M.batch_event(first + i, 1)));
            start_ms[i] = a;
            end_ms[i] = b;
        }
    });
}

// ---- one layer at a time (tests: teacher-forced per-layer parity) -------------------------------------------------

zv_status zv_debug_layer(zv_model *m, int kind, int index, const float *x, uint32_t rows, const float *style, float *out)
{
    return guarded([&] {
        ZV_NEED(m && x && out, "null argument");
        ZV_NEED(rows > 0, "rows must be > 0");
        Model &M = *m->m;
        use_lane0(m);
        ZV_NEED(!M.graph_mode, "zv_debug_layer runs eagerly: turn graph mode off");
        const size_t E = M.E(), Mm = M.hp.audio_num_mels, hop = M.hp.audio_hop_size;
        std::vector<float> zsty(E, 0.f);
        const float *sty = style ? style : zsty.data();
        M.dbg_layer = Model::DebugLayer();
        M.dbg_layer.kind = kind;
        M.dbg_layer.index = index;
        M.dbg_layer.x = x;
        M.dbg_layer.out = out;
        struct Reset { Model &M; ~Reset() { M.dbg_layer = Model::DebugLayer(); } } reset{M};
        if (kind == ZV_LAYER_VOC_RESBLOCK || kind == ZV_LAYER_VOC_UPSAMPLE || kind == ZV_LAYER_VOC_INPUT || kind == ZV_LAYER_VOC_OUTPUT)
        {
            // rows are rows at the layer's INPUT rate: frames x samples per frame of the stage the layer reads
            uint32_t rate = 1;
            if (kind == ZV_LAYER_VOC_RESBLOCK)
            {
                const int stage = index / (int)M.hp.voc_num_resblocks;
                ZV_NEED(index >= 0 && stage < (int)M.hp.voc_num_upsamples, "residual block index out of range");
                rate = (uint32_t)M.voc_stage_rate(stage);
            }
            else if (kind == ZV_LAYER_VOC_UPSAMPLE)
            {
                ZV_NEED(index >= 0 && index < (int)M.hp.voc_num_upsamples, "upsample index out of range");
                rate = index == 0 ? 1u : (uint32_t)M.voc_stage_rate(index - 1);
            }
            else if (kind == ZV_LAYER_VOC_OUTPUT)
                rate = (uint32_t)hop;
            ZV_NEED(rows % rate == 0, "rows must be a multiple of the layer's samples per frame");
            const uint32_t T = rows / rate;
            check_T(M, T);
            Layout L;
            const size_t b_mel = (size_t)T * Mm * 4, o_mel = L.at(b_mel), o_wav = L.at((size_t)T * hop * 4);
            char *io = (char *)M.io_scratch(L.size());
            if (kind == ZV_LAYER_VOC_INPUT)
                ZV_HIP(hipMemcpyAsync(io + o_mel, x, b_mel, hipMemcpyHostToDevice, M.stream()));      // the layer's input IS the mel
            else
                ZV_HIP(hipMemsetAsync(io + o_mel, 0, b_mel, M.stream()));
            M.vocode_dev(zv::Batch::single(1, T, 1), (const float *)(io + o_mel), (float *)(io + o_wav));
        }
        else if (kind == ZV_LAYER_ENC_FFT || kind == ZV_LAYER_VAR_PRED || kind == ZV_LAYER_ENC_EMBED || kind == ZV_LAYER_ENC_MHA ||
                 kind == ZV_LAYER_ENC_FFN)
        {
            const uint32_t n = rows, T = 8;
            Layout L;
            const size_t o_nf = L.at(4), o_ids = L.at((size_t)n * 4), o_pun = L.at((size_t)n * 4), o_sty = L.at(E * 4),
                         o_hid = L.at((size_t)T * E * 4);
            char *io = (char *)M.io_scratch(L.size());
            int32_t *d_nf = (int32_t *)(io + o_nf), *d_ids = (int32_t *)(io + o_ids), *d_pun = (int32_t *)(io + o_pun);
            float *d_sty = (float *)(io + o_sty), *d_hid = (float *)(io + o_hid);
            ZV_HIP(hipMemsetAsync(io, 0, o_sty, M.stream()));                 // frame count, ids and puncts: all in front of the style
            std::vector<int32_t> hid, hpu;
            if (kind == ZV_LAYER_ENC_EMBED)
            {
                // x[n] = (phoneme id, punctuation id) as floats
                hid.resize(n);
                hpu.resize(n);
                for (uint32_t i = 0; i < n; i++)
                {
                    hid[i] = (int32_t)x[2 * i];
                    hpu[i] = (int32_t)x[2 * i + 1];
                }
                check_ids(M, hid.data(), hpu.data(), n);
                ZV_HIP(hipMemcpyAsync(d_ids, hid.data(), (size_t)n * 4, hipMemcpyHostToDevice, M.stream()));
                ZV_HIP(hipMemcpyAsync(d_pun, hpu.data(), (size_t)n * 4, hipMemcpyHostToDevice, M.stream()));
                ZV_HIP(hipStreamSynchronize(M.stream()));            // the staging vectors go out of scope below
            }
            ZV_HIP(hipMemcpyAsync(d_sty, sty, E * 4, hipMemcpyHostToDevice, M.stream()));
            M.encode_dev(zv::Batch::single(n, T, n), d_ids, d_pun, d_sty, d_hid, d_nf);
        }
        else if (kind == ZV_LAYER_DEC_BLOCK || kind == ZV_LAYER_DEC_ASR_RES || kind == ZV_LAYER_DEC_TO_OUT || kind == ZV_LAYER_DEC_ADAIN)
        {
            const uint32_t T = rows;
            check_T(M, T);
            Layout L;
            const size_t o_sty = L.at(E * 4), o_hid = L.at((size_t)T * E * 4), o_mel = L.at((size_t)T * Mm * 4);
            char *io = (char *)M.io_scratch(L.size());
            float *d_sty = (float *)(io + o_sty), *d_hid = (float *)(io + o_hid), *d_mel = (float *)(io + o_mel);
            if (kind == ZV_LAYER_DEC_ASR_RES)
                ZV_HIP(hipMemcpyAsync(d_hid, x, (size_t)T * E * 4, hipMemcpyHostToDevice, M.stream()));     // asr_res reads the stage input itself
            else
                ZV_HIP(hipMemsetAsync(d_hid, 0, o_mel - o_hid, M.stream()));                               // the region, padding included
            ZV_HIP(hipMemcpyAsync(d_sty, sty, E * 4, hipMemcpyHostToDevice, M.stream()));
            M.decode_dev(zv::Batch::single(1, T, 1), d_hid, d_sty, d_mel);
        }
        else if (kind == ZV_LAYER_ENC_LN)
            M.debug_layernorm(index, rows);
        else
            zv::fail(ZV_ERR_ARG, "unknown layer kind %d", kind);
        M.sync();
        if (!M.dbg_layer.done) zv::fail(ZV_ERR_ARG, "layer (%d, %d) does not exist in this model", kind, index);
    });
}

zv_status zv_debug_mfma_chain(zv_model *m, int form, const void *a, const void *b, const float *c0, uint32_t K, float *out)
{
    return guarded([&] {
        ZV_NEED(m && a && b && c0 && out, "null argument");
        ZV_NEED(form >= 0 && form <= 2, "form must be 0 (32x32x16 f16), 1 (16x16x32 f16) or 2 (32x32x2 f32)");
        ZV_NEED(K >= 32 && K % 32 == 0 && K <= 4096, "K must be a multiple of 32, at most 4096");
        Model &M = *m->m;
        use_lane0(m);
        const size_t elem = form == 2 ? 4 : 2, b_op = (size_t)32 * K * elem, b_c = 32 * 32 * 4;
        Layout L;
        const size_t o_a = L.at(b_op), o_b = L.at(b_op), o_c0 = L.at(b_c), o_out = L.at(b_c);
        char *io = (char *)M.io_scratch(L.size());
        ZV_HIP(hipMemcpyAsync(io + o_a, a, b_op, hipMemcpyHostToDevice, M.stream()));
        ZV_HIP(hipMemcpyAsync(io + o_b, b, b_op, hipMemcpyHostToDevice, M.stream()));
        ZV_HIP(hipMemcpyAsync(io + o_c0, c0, b_c, hipMemcpyHostToDevice, M.stream()));
        ZV_HIP(zv::launch_mfma_chain(M.stream(), form, io + o_a, io + o_b, (const float *)(io + o_c0), (int)K, (float *)(io + o_out)));
        ZV_HIP(hipMemcpyAsync(out, io + o_out, b_c, hipMemcpyDeviceToHost, M.stream()));
        M.sync();
    });
}

zv_status zv_debug_set(const char *name, int value)
{
    return guarded([&] {
        if (!name)
        {
            zv::knob_reset();
            return;
        }
        if (!zv::knob_set(name, value)) zv::fail(ZV_ERR_ARG, "unknown switch '%s'", name);
    });
}

zv_status zv_debug_get(const char *name, int *value)
{
    return guarded([&] {
        ZV_NEED(name && value, "null argument");
        if (!zv::knob_get(name, value)) zv::fail(ZV_ERR_ARG, "unknown switch '%s'", name);
    });
}

zv_status zv_debug_voc_runs(zv_model *m, uint32_t lane, int32_t *table, uint32_t cap, uint32_t *n)
{
    return guarded([&] {
        ZV_NEED(m && n && (table || !cap), "null argument");
        ZV_NEED(lane < ZV_BATCH_LANES, "lane out of range");
        Model &M = *m->m;
        ZV_HIP(hipSetDevice(M.device));
        struct Restore { Model &M; int was; ~Restore() { M.select_lane(was); } } restore{M, M.selected_lane()};
        M.select_lane((int)lane);
        M.sync();
        int cnt = 0;
        const zv::Seg *tab = M.voc_runs_last(&cnt);      // null again once the lane's arena was reallocated
        *n = tab ? (uint32_t)cnt : 0;
        const size_t k = std::min<size_t>(*n, cap);
        if (k) ZV_HIP(hipMemcpy(table, tab, k * sizeof(zv::Seg), hipMemcpyDeviceToHost));
    });
}

zv_status zv_debug_poison(zv_model *m, uint32_t lane, int byte, size_t filled[3])
{
    return guarded([&] {
        ZV_NEED(m, "null model");
        ZV_NEED(lane < ZV_BATCH_LANES, "lane out of range");
        ZV_NEED(byte >= 0 && byte <= 255, "byte must be 0..255");
        ZV_NEED(!(m->pending && m->pending[lane].active), "the lane has a batch in flight: finish it with zv_synthesize_batch_end first");
        ZV_HIP(hipSetDevice(m->m->device));
        size_t f[3];
        m->m->poison_lane((int)lane, byte, f);       // the selected lane stays selected: nothing is selected
        for (int k = 0; filled && k < 3; k++) filled[k] = f[k];
    });
}

// ---- device-resident entry points ---------------------------------------------------------------

void *zv_device_alloc(zv_model *m, size_t bytes)
{
    if (!m) return nullptr;
    void *p = nullptr;
    if (hipSetDevice(m->m->device) != hipSuccess) return nullptr;
    if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess)
    {
        g_last_error = "hipMalloc failed";
        return nullptr;
    }
    return p;
}

void zv_device_free(zv_model *m, void *p)
{
    if (!m || !p) return;
    hipSetDevice(m->m->device);
    try { m->m->sync_all_lanes(); } catch (...) {}
    hipFree(p);
}

zv_status zv_memcpy_h2d(zv_model *m, void *dst, const void *src, size_t bytes)
{
    return guarded([&] {
        ZV_NEED(m && dst && src, "null argument");
        // lane 0's stream, the one zv_vocode_device / zv_decode_device run on, whatever lane was touched last (the lanes' streams
        // are not ordered with each other); no busy check: the copy only queues behind what lane 0 already holds
        lane0_select(m);
        ZV_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, m->m->stream()));
        m->m->sync();
    });
}

zv_status zv_memcpy_d2h(zv_model *m, void *dst, const void *src, size_t bytes)
{
    return guarded([&] {
        ZV_NEED(m && dst && src, "null argument");
        lane0_select(m);
        ZV_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, m->m->stream()));
        m->m->sync();
    });
}

zv_status zv_vocode_device(zv_model *m, const float *d_mel, uint32_t T, float *d_wav)
{
    return guarded([&] {
        ZV_NEED(m && d_mel && d_wav, "null argument");
        check_T(*m->m, T);
        use_lane0(m);
        m->m->vocode_dev_graph(zv::Batch::single(1, T, 1), d_mel, d_wav);
    });
}

zv_status zv_decode_device(zv_model *m, const float *d_hidden, const float *d_style, uint32_t T, float *d_mel)
{
    return guarded([&] {
        ZV_NEED(m && d_hidden && d_style && d_mel, "null argument");
        check_T(*m->m, T);
        use_lane0(m);
        m->m->decode_dev(zv::Batch::single(1, T, 1), d_hidden, d_style, d_mel);
    });
}

zv_status zv_synchronize(zv_model *m)
{
    return guarded([&] {
        ZV_NEED(m, "null model");
        ZV_HIP(hipSetDevice(m->m->device));
        // every lane: whatever entry point enqueued it, the work is done when this returns (a batch begun with
        // zv_synthesize_batch_begin still needs its _end: that is where its waveforms leave the staging block)
        m->m->sync_all_lanes();
    });
}

zv_status zv_set_graph_mode(zv_model *m, int on)
{
    return guarded([&] {
        ZV_NEED(m, "null model");
        m->m->graph_mode = on != 0;
    });
}

zv_status zv_set_graph_cache(zv_model *m, uint32_t capacity)
{
    return guarded([&] {
        ZV_NEED(m, "null model");
        ZV_NEED(zv::graph_capacity_ok(capacity), "graph cache capacity must be 1 .. 1024");
        ZV_HIP(hipSetDevice(m->m->device));
        m->m->set_graph_cache(capacity);
    });
}

zv_status zv_graph_cache_stats(zv_model *m, zv_graph_stats *out)
{
    return guarded([&] {
        ZV_NEED(m && out, "null argument");
        m->m->graph_stats(out);
    });
}

// ---- measurement -----------------------------------------------------------------------------

zv_status zv_profile_begin(zv_model *m)
{
    return guarded([&] {
        ZV_NEED(m, "null model");
        lane0_select(m);                      // the synchronous entry points, which are what gets profiled, run on lane 0
        m->m->sync();
        m->m->prof_clear();
        m->m->profiling = true;
    });
}

zv_status zv_profile_end(zv_model *m, zv_kernel_stat *stats, uint32_t cap, uint32_t *n)
{
    return guarded([&] {
        ZV_NEED(m && n, "null argument");
        Model &M = *m->m;
        lane0_select(m);
        M.sync();
        M.profiling = false;
        std::map<std::string, zv_kernel_stat> agg;
        std::vector<std::string> order;
        for (auto &p : M.prof)
        {
            float ms = 0.f;
            ZV_HIP(hipEventElapsedTime(&ms, p.e0, p.e1));
            auto it = agg.find(p.name);
            if (it == agg.end())
            {
                zv_kernel_stat s;
                memset(&s, 0, sizeof(s));
                strncpy(s.name, p.name, sizeof(s.name) - 1);
                it = agg.emplace(p.name, s).first;
                order.push_back(p.name);
            }
            it->second.launches += (uint32_t)p.launches;
            it->second.total_ms += ms;
            it->second.algo_bytes += p.bytes;
            it->second.algo_flops += p.flops;
        }
        M.prof_clear();
        uint32_t k = 0;
        for (auto &name : order)
        {
            if (stats && k < cap) stats[k] = agg[name];
            k++;
        }
        *n = k;
    });
}

zv_status zv_gguf_inspect(const char *gguf_path, uint32_t *n_tensors, uint32_t *max_seq_len, int tensor_index,
                          char *name_out, uint32_t *type_out, int64_t *ne_out)
{
    return guarded([&] {
        ZV_NEED(gguf_path, "null path");
        zv::GgufFile g;
        g.open(gguf_path);
        if (n_tensors) *n_tensors = (uint32_t)g.tensors().size();
        if (max_seq_len) *max_seq_len = g.get_u32("zerovox-resnet-fs2-styletts.max_seq_len");
        if (tensor_index >= 0)
        {
            if ((size_t)tensor_index >= g.tensors().size()) zv::fail(ZV_ERR_ARG, "tensor index %d out of range", tensor_index);
            const zv::GgufTensor &t = g.tensors()[tensor_index];
            if (name_out) { strncpy(name_out, t.name.c_str(), 63); name_out[63] = 0; }
            if (type_out) *type_out = t.type;
            if (ne_out) for (int i = 0; i < 4; i++) ne_out[i] = t.ne[i];
        }
    });
}

// ---- WAV writer (reference src/zerovox.cpp:337-391 uses libsndfile SF_FORMAT_WAV | SF_FORMAT_PCM_16) ----

zv_status zv_write_wav(const char *path, const float *wav, size_t n_samples, uint32_t sampling_rate)
{
    return guarded([&] {
        ZV_NEED(path && wav, "null argument");
        FILE *f = fopen(path, "wb");
        if (!f) zv::fail(ZV_ERR_IO, "cannot open '%s' for writing", path);
        if (n_samples > (size_t)0x7FFFFFE0u / 2) zv::fail(ZV_ERR_ARG, "%zu samples do not fit a RIFF/WAVE file (32-bit sizes)", n_samples);
        const uint32_t data_bytes = (uint32_t)(n_samples * 2);
        uint8_t hdr[44];
        auto put32 = [&](int o, uint32_t v) { for (int i = 0; i < 4; i++) hdr[o + i] = (uint8_t)(v >> (8 * i)); };
        auto put16 = [&](int o, uint16_t v) { hdr[o] = (uint8_t)v; hdr[o + 1] = (uint8_t)(v >> 8); };
        memcpy(hdr, "RIFF", 4);
        put32(4, 36 + data_bytes);
        memcpy(hdr + 8, "WAVEfmt ", 8);
        put32(16, 16);
        put16(20, 1);                 // PCM
        put16(22, 1);                 // mono
        put32(24, sampling_rate);
        put32(28, sampling_rate * 2);
        put16(32, 2);
        put16(34, 16);
        memcpy(hdr + 36, "data", 4);
        put32(40, data_bytes);
        bool ok = fwrite(hdr, 1, 44, f) == 44;
        std::vector<int16_t> pcm(n_samples);
        for (size_t i = 0; i < n_samples; i++)
        {
            // libsndfile float -> PCM16: scale by 0x7FFF (normalisation on), round to nearest, clip
            float v = wav[i] * 32767.0f;
            long q = lrintf(v);
            if (q > 32767) q = 32767;
            if (q < -32768) q = -32768;
            pcm[i] = (int16_t)q;
        }
        ok = ok && fwrite(pcm.data(), 2, n_samples, f) == n_samples;
        ok = (fclose(f) == 0) && ok;
        if (!ok) zv::fail(ZV_ERR_IO, "short write to '%s'", path);
    });
}

// int16 samples as they are (zv_resample_wave's pcm): nothing is scaled or rounded here
zv_status zv_write_wav_pcm16(const char *path, const int16_t *pcm, size_t n, uint32_t sampling_rate)
{
    return guarded([&] {
        ZV_NEED(path && pcm, "null argument");
        if (n > (size_t)0x7FFFFFE0u / 2) zv::fail(ZV_ERR_ARG, "%zu samples do not fit a RIFF/WAVE file (32-bit sizes)", n);
        FILE *f = fopen(path, "wb");
        if (!f) zv::fail(ZV_ERR_IO, "cannot open '%s' for writing", path);
        const uint32_t data_bytes = (uint32_t)(n * 2);
        uint8_t hdr[44];
        auto put32 = [&](int o, uint32_t v) { for (int i = 0; i < 4; i++) hdr[o + i] = (uint8_t)(v >> (8 * i)); };
        auto put16 = [&](int o, uint16_t v) { hdr[o] = (uint8_t)v; hdr[o + 1] = (uint8_t)(v >> 8); };
        memcpy(hdr, "RIFF", 4);
        put32(4, 36 + data_bytes);
        memcpy(hdr + 8, "WAVEfmt ", 8);
        put32(16, 16);
        put16(20, 1);                 // PCM
        put16(22, 1);                 // mono
        put32(24, sampling_rate);
        put32(28, sampling_rate * 2);
        put16(32, 2);
        put16(34, 16);
        memcpy(hdr + 36, "data", 4);
        put32(40, data_bytes);
        bool ok = fwrite(hdr, 1, 44, f) == 44;
        std::vector<uint8_t> le(n * 2);
        for (size_t i = 0; i < n; i++) le[2 * i] = (uint8_t)(uint16_t)pcm[i], le[2 * i + 1] = (uint8_t)((uint16_t)pcm[i] >> 8);
        ok = ok && fwrite(le.data(), 2, n, f) == n;
        ok = (fclose(f) == 0) && ok;
        if (!ok) zv::fail(ZV_ERR_IO, "short write to '%s'", path);
    });
}

}  // extern "C"
