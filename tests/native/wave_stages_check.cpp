// Host-side driver of csrc/wave_stages.h for tests/test_wave_stages_cpu.py (no GPU, no HIP).
//   wave_stages_check cases
//       every subset of the six stages x the frame / phoneme asks of the three table stages x three row spaces: the carves against the
//       layout as it stood inline in capi.cpp's run_single and batch_enqueue before the header existed (restated below, region by
//       region, in that code's order), every region aligned, disjoint, inside its block and empty where its stage is off; the bind;
//       the tail group's pointers against Model::vocode_tail's arithmetic as it stood; the graph key; needs_scan; the ask's rules.
//       Prints "ok <checks>".
#include "wave_stages.h"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace zv;

static long g_checks = 0;
#define CHECK(cond, ...)                                   \
    do                                                     \
    {                                                      \
        g_checks++;                                        \
        if (!(cond))                                       \
        {                                                  \
            printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); \
            printf(__VA_ARGS__);                           \
            printf("\n");                                  \
            exit(1);                                       \
        }                                                  \
    } while (0)

struct Span { size_t off, bytes; };

// the regions of one block: 256-aligned, in ascending order without overlap, inside size()
static void check_block(const Layout &L, const std::vector<Span> &spans, size_t first, const char *what)
{
    size_t end = first;
    for (size_t k = 0; k < spans.size(); k++)
    {
        CHECK(spans[k].off % 256 == 0, "%s region %zu at %zu", what, k, spans[k].off);
        CHECK(spans[k].off >= end, "%s region %zu at %zu overlaps the one before (ends %zu)", what, k, spans[k].off, end);
        end = spans[k].off + spans[k].bytes;
        CHECK(end <= L.size(), "%s region %zu ends at %zu past size %zu", what, k, end, L.size());
    }
}

// The layout as it stood inline (capi.cpp before wave_stages.h), behind whatever the block already holds.  vol ... flt: the stages;
// xf / xp: some utterance asks for the frame rows / phoneme rows of contour, pitch, bands.
struct Old
{
    bool vol, env, ctr, pit, bnd, flt, cf, cp, pf, pp, bf, bp;
};
static Old old_of(const WaveAsk &a)
{
    return Old{a.on[WS_VOLUME], a.on[WS_ENVELOPE], a.on[WS_CONTOUR], a.on[WS_PITCH], a.on[WS_BANDS], a.on[WS_FILTER],
               a.on[WS_CONTOUR] && a.frames[WS_CONTOUR], a.on[WS_CONTOUR] && a.phonemes[WS_CONTOUR], a.on[WS_PITCH] && a.frames[WS_PITCH],
               a.on[WS_PITCH] && a.phonemes[WS_PITCH], a.on[WS_BANDS] && a.frames[WS_BANDS], a.on[WS_BANDS] && a.phonemes[WS_BANDS]};
}
// run_single: one block
static void old_single(Layout &L, const Old &q, size_t n, size_t T, size_t *o)
{
    const size_t b_ids = n * 4;
    o[R_VOL] = L.at(q.vol ? LEVEL_VOL_STRIDE * 4 : 0), o[R_LEVELS] = L.at(q.vol ? sizeof(LevelRow) : 0);
    o[R_ENV_GAIN] = L.at(q.env ? b_ids : 0), o[R_ENV] = L.at(q.env ? ENV_CTL_STRIDE * 4 : 0);
    const size_t b_cfr = T * sizeof(ContourRow), b_cph = n * sizeof(ContourRow);
    o[R_CTR_FRAMES] = L.at(q.ctr ? b_cfr : 0), o[R_CTR_PHONEMES] = L.at(q.ctr ? b_cph : 0);
    const size_t b_pfr = T * sizeof(PitchFrameRow), b_pph = n * sizeof(PitchPhonemeRow);
    o[R_PIT_FRAMES] = L.at(q.pit ? b_pfr : 0), o[R_PIT_PHONEMES] = L.at(q.pit ? b_pph : 0), o[R_PIT_PAR] = L.at(q.pit ? PITCH_PARAM_STRIDE * 4 : 0);
    const size_t b_bfr = T * BANDS_ROW_STRIDE * 4, b_bph = n * BANDS_ROW_STRIDE * 4;
    o[R_BND_FRAMES] = L.at(q.bnd ? b_bfr : 0), o[R_BND_PHONEMES] = L.at(q.bnd ? b_bph : 0), o[R_BND_SLAB] = L.at(q.bnd ? 2 * b_bfr : 0),
    o[R_BND_PAR] = L.at(q.bnd ? BANDS_PARAM_STRIDE * 4 : 0);
    o[R_FLT_PAR] = L.at(q.flt ? FILTER_PARAM_STRIDE * 4 : 0);
}
// batch_enqueue: the input block, the device block, the pinned block
static void old_batch(Layout &in, Layout &dev, Layout &host, const Old &q, size_t nseg, size_t n_rows, size_t t_rows, size_t ntot, size_t frame_rows,
                      size_t *o)
{
    o[R_VOL] = in.at(q.vol ? nseg * LEVEL_VOL_STRIDE * 4 : 0);
    o[R_ENV_GAIN] = in.at(q.env ? n_rows * 4 : 0);
    o[R_ENV] = in.at(q.env ? nseg * ENV_CTL_STRIDE * 4 : 0);
    o[R_PIT_PAR] = in.at(q.pit ? nseg * PITCH_PARAM_STRIDE * 4 : 0);
    o[R_BND_PAR] = in.at(q.bnd ? nseg * BANDS_PARAM_STRIDE * 4 : 0);
    o[R_FLT_PAR] = in.at(q.flt ? nseg * FILTER_PARAM_STRIDE * 4 : 0);
    o[R_LEVELS] = dev.at(q.vol ? nseg * sizeof(LevelRow) : 0);
    o[R_CTR_FRAMES] = dev.at(q.ctr ? t_rows * sizeof(ContourRow) : 0);
    o[R_CTR_PHONEMES] = dev.at(q.ctr ? n_rows * sizeof(ContourRow) : 0);
    o[R_PIT_FRAMES] = dev.at(q.pit ? t_rows * sizeof(PitchFrameRow) : 0);
    o[R_PIT_PHONEMES] = dev.at(q.pit ? n_rows * sizeof(PitchPhonemeRow) : 0);
    o[R_BND_FRAMES] = dev.at(q.bnd ? t_rows * BANDS_ROW_STRIDE * 4 : 0);
    o[R_BND_PHONEMES] = dev.at(q.bnd ? n_rows * BANDS_ROW_STRIDE * 4 : 0);
    o[R_BND_SLAB] = dev.at(q.bnd ? t_rows * BANDS_ROW_STRIDE * 8 : 0);
    o[R_LEVELS_HOST] = host.at(q.vol ? nseg * sizeof(zv_level) : 0);
    o[R_CTR_FRAMES_HOST] = host.at(q.cf ? frame_rows * sizeof(zv_frame_level) : 0), o[R_CTR_PHONEMES_HOST] = host.at(q.cp ? ntot * sizeof(zv_frame_level) : 0);
    o[R_PIT_FRAMES_HOST] = host.at(q.pf ? frame_rows * sizeof(zv_pitch_frame) : 0), o[R_PIT_PHONEMES_HOST] = host.at(q.pp ? ntot * sizeof(zv_pitch_phoneme) : 0);
    o[R_BND_FRAMES_HOST] = host.at(q.bf ? frame_rows * BANDS_ROW_STRIDE * 4 : 0), o[R_BND_PHONEMES_HOST] = host.at(q.bp ? ntot * BANDS_ROW_STRIDE * 4 : 0);
}

// Model::vocode_tail's arithmetic as it stood
static WaveStages old_group(const WaveStages &bt, int g0)
{
    WaveStages sub = bt;
    if (bt.d_vol)
    {
        sub.d_vol = bt.d_vol + (size_t)g0 * LEVEL_VOL_STRIDE;
        sub.d_levels = bt.d_levels + g0;
    }
    if (bt.d_nframes) sub.d_nframes = bt.d_nframes + g0;
    if (bt.d_pit_par) sub.d_pit_par = bt.d_pit_par + (size_t)g0 * PITCH_PARAM_STRIDE;
    if (bt.d_bnd_par) sub.d_bnd_par = bt.d_bnd_par + (size_t)g0 * BANDS_PARAM_STRIDE;
    if (bt.d_flt_par) sub.d_flt_par = bt.d_flt_par + (size_t)g0 * FILTER_PARAM_STRIDE;
    if (bt.d_env) sub.d_env = bt.d_env + (size_t)g0 * ENV_CTL_STRIDE;
    return sub;
}

static void one_case(const WaveAsk &ask, size_t nseg, size_t n_rows, size_t t_rows)
{
    const Old q = old_of(ask);
    const WaveRegion *R = WAVE_REGIONS;
    const size_t lead[3] = {0, 100, 4096 + 7};       // what the block holds in front of the stages' regions
    for (size_t pre : lead)
    {
        // a batch's three blocks; the staging block by what the utterances hold (less than the capacity)
        const size_t ntot = n_rows - n_rows / 3, frame_rows = t_rows - t_rows / 5;
        Layout in, dev, host, oin, odev, ohost;
        for (Layout *L : {&in, &dev, &host, &oin, &odev, &ohost}) L->at(pre);
        WaveOffsets o;
        size_t old[R_COUNT];
        wave_carve(in, ask, WaveRows{nseg, n_rows, t_rows}, WR_INPUT, o);
        wave_carve(dev, ask, WaveRows{nseg, n_rows, t_rows}, WR_DEVICE, o);
        wave_carve(host, ask, WaveRows{nseg, ntot, frame_rows}, WR_HOST, o);
        old_batch(oin, odev, ohost, q, nseg, n_rows, t_rows, ntot, frame_rows, old);
        CHECK(in.end == oin.end && dev.end == odev.end && host.end == ohost.end, "block ends differ from the inline layout's");
        std::vector<Span> spans[3];
        for (int id = 0; id < R_COUNT; id++)
        {
            CHECK(o.at[id] == old[id], "region %d at %zu, the inline layout had %zu", id, o.at[id], old[id]);
            const WaveRows rows = R[id].role == WR_HOST ? WaveRows{nseg, ntot, frame_rows} : WaveRows{nseg, n_rows, t_rows};
            const size_t bytes = wave_region_bytes(id, ask, rows);
            if (!ask.on[R[id].stage]) CHECK(bytes == 0, "region %d of an off stage takes %zu bytes", id, bytes);
            else if (R[id].role != WR_HOST) CHECK(bytes == rows[R[id].rows] * R[id].row_bytes && bytes > 0, "region %d takes %zu bytes", id, bytes);
            spans[R[id].role == WR_INPUT ? 0 : R[id].role == WR_DEVICE ? 1 : 2].push_back(Span{o.at[id], bytes});
        }
        check_block(in, spans[0], pre, "input");
        check_block(dev, spans[1], pre, "device");
        check_block(host, spans[2], pre, "staging");

        // the bind: every region of an on stage at its block's base + offset, everything of an off stage null
        char *const bin = (char *)0x10000000, *const bdev = (char *)0x70000000;
        const int32_t *const nf = (const int32_t *)0x5000;
        const void *const table = (const void *)0x6000;
        const WaveStages w = wave_bind(ask, o, bin, bdev, nf, table);
        WaveStages e;
        if (q.vol) e.d_vol = (const float *)(bin + old[R_VOL]), e.d_levels = (LevelRow *)(bdev + old[R_LEVELS]), e.d_nframes = nf;
        if (q.env) e.d_env_gain = (const float *)(bin + old[R_ENV_GAIN]), e.d_env = (const int32_t *)(bin + old[R_ENV]), e.d_nframes = nf;
        if (q.ctr) e.d_ctr_frames = (ContourRow *)(bdev + old[R_CTR_FRAMES]), e.d_ctr_phonemes = (ContourRow *)(bdev + old[R_CTR_PHONEMES]);
        if (q.pit)
            e.d_pit_frames = (PitchFrameRow *)(bdev + old[R_PIT_FRAMES]), e.d_pit_phonemes = (PitchPhonemeRow *)(bdev + old[R_PIT_PHONEMES]),
            e.d_pit_par = (const uint32_t *)(bin + old[R_PIT_PAR]);
        if (q.bnd)
            e.d_bnd_frames = (float *)(bdev + old[R_BND_FRAMES]), e.d_bnd_phonemes = (float *)(bdev + old[R_BND_PHONEMES]),
            e.d_bnd_slab = (unsigned long long *)(bdev + old[R_BND_SLAB]), e.d_bnd_par = (const uint32_t *)(bin + old[R_BND_PAR]), e.d_bnd_table = table;
        if (q.flt) e.d_flt_par = (const uint32_t *)(bin + old[R_FLT_PAR]);
        CHECK(w == e, "the bind differs from the inline bind blocks");
        const bool scan = q.env || q.ctr || q.pit || q.bnd;      // (capi.cpp: `env || ctr || pit || bnd`)
        CHECK(w.needs_scan() == scan && ask.needs_scan() == scan, "needs_scan");
        CHECK(w.inconsistent((const void *)0x7000) == nullptr, "a bound group is consistent: %s", w.inconsistent((const void *)0x7000));
        CHECK((w.inconsistent(nullptr) != nullptr) == scan, "without the scan exactly the stages that read it are inconsistent");
        for (int g0 : {0, 1, 63})
        {
            const WaveStages g = w.group(g0), eg = old_group(w, g0);
            CHECK(g == eg, "group(%d) differs from vocode_tail's arithmetic", g0);
            CHECK(g0 != 0 || g == w, "group(0) moves something");
        }
        // the graph key: any one pointer changed compares unequal
        for (size_t k = 0; k < sizeof(WaveStages) / sizeof(void *); k++)
        {
            WaveStages c = w;
            char *p;
            memcpy(&p, (char *)&c + k * sizeof(void *), sizeof(p));
            p += 4;
            memcpy((char *)&c + k * sizeof(void *), &p, sizeof(p));
            CHECK(!(c == w), "pointer %zu is not part of the key", k);
        }
        CHECK(sizeof(WaveStages) % sizeof(void *) == 0, "pointers only");

        // a single utterance's one block: the inline layout of run_single, and the batch's input and device carves at nseg = 1
        if (nseg == 1)
        {
            Layout L, oL, i1, d1;
            L.at(pre), oL.at(pre);
            WaveOffsets so, bo;
            size_t sold[R_COUNT] = {};
            wave_carve(L, ask, WaveRows{1, n_rows, t_rows}, WR_INPUT | WR_DEVICE, so);
            old_single(oL, q, n_rows, t_rows, sold);
            wave_carve(i1, ask, WaveRows{1, n_rows, t_rows}, WR_INPUT, bo);
            wave_carve(d1, ask, WaveRows{1, n_rows, t_rows}, WR_DEVICE, bo);
            CHECK(L.end == oL.end, "the single block ends at %zu, inline at %zu", L.end, oL.end);
            std::vector<Span> sp;
            size_t sum = 0;
            for (int id = 0; id < R_COUNT; id++)
            {
                if (R[id].role == WR_HOST) continue;
                CHECK(so.at[id] == sold[id], "single: region %d at %zu, inline %zu", id, so.at[id], sold[id]);
                sp.push_back(Span{so.at[id], wave_region_bytes(id, ask, WaveRows{1, n_rows, t_rows})});
                sum += region_align(sp.back().bytes);
            }
            check_block(L, sp, pre, "single");
            CHECK(sum == i1.size() + d1.size(), "the single block holds %zu bytes of regions, the batch's two at nseg = 1 hold %zu", sum, i1.size() + d1.size());
        }
    }
}

// the ask's rules from the public structs (count = 3; `who` asks, the others do not)
static void ask_rules()
{
    zv_frame_level fl[4];
    zv_pitch_frame pf[4];
    zv_pitch_phoneme pp[4];
    float rows[4], taps[1] = {1.0f};
    zv_level lv[3];
    zv_volume vol[3] = {};
    zv_envelope env[3] = {};
    for (int who = 0; who < 3; who++)
        for (int mask = 0; mask < 128; mask++)
        {
            zv_contour c[3] = {};
            zv_pitch p[3] = {};
            zv_bands b[3] = {};
            zv_filter f[3] = {};
            WaveArgs a;
            if (mask & 1) a.contour = c, c[who].frames = fl;
            if (mask & 2) a.contour = c, c[who].phonemes = fl;
            if (mask & 4) a.pitch = p, p[who].frames = pf;
            if (mask & 8) a.pitch = p, p[who].phonemes = pp;
            if (mask & 16) a.bands = b, b[who].frames = rows;
            if (mask & 32) a.bands = b, b[who].phonemes = rows;
            if (mask & 64) a.filter = f, f[who].taps = taps, f[who].n_taps = 1;
            const WaveAsk k = a.ask(3);
            CHECK(!k.on[WS_VOLUME] && !k.on[WS_ENVELOPE], "volume and envelope go by their arrays");
            CHECK(k.on[WS_CONTOUR] == ((mask & 3) != 0) && k.frames[WS_CONTOUR] == ((mask & 1) != 0) && k.phonemes[WS_CONTOUR] == ((mask & 2) != 0), "contour");
            CHECK(k.on[WS_PITCH] == ((mask & 12) != 0) && k.frames[WS_PITCH] == ((mask & 4) != 0) && k.phonemes[WS_PITCH] == ((mask & 8) != 0), "pitch");
            CHECK(k.on[WS_BANDS] == ((mask & 48) != 0) && k.frames[WS_BANDS] == ((mask & 16) != 0) && k.phonemes[WS_BANDS] == ((mask & 32) != 0), "bands");
            CHECK(k.on[WS_FILTER] == ((mask & 64) != 0), "filter");
            // a slice that leaves the asking utterance out asks for nothing; one that starts at it does
            const WaveAsk none = a.slice(who + 1).ask(2 - who), some = a.slice(who).ask(1);
            for (int s = 0; s < WS_COUNT; s++) CHECK(!none.on[s] && some.on[s] == k.on[s], "slice, stage %d", s);
        }
    // arrays that are there but ask for nothing: tables off, the filter off; an envelope array alone is on; levels alone is a meter
    zv_contour c[3] = {};
    zv_pitch p[3] = {};
    zv_bands b[3] = {};
    zv_filter f[3] = {};
    WaveArgs a;
    a.contour = c, a.pitch = p, a.bands = b, a.filter = f;
    WaveAsk k = a.ask(3);
    for (int s = 0; s < WS_COUNT; s++) CHECK(!k.on[s], "stage %d on without an ask", s);
    a.envelope = env;
    CHECK(a.ask(3).on[WS_ENVELOPE] && !a.ask(3).on[WS_VOLUME], "the envelope array turns the envelope on");
    a.levels = lv;
    CHECK(a.ask(3).on[WS_VOLUME], "levels alone: a meter");
    a.levels = nullptr, a.volume = vol;
    CHECK(a.ask(3).on[WS_VOLUME], "volume alone");
    CHECK(a.slice(2).volume == vol + 2 && a.slice(2).levels == nullptr && a.slice(2).envelope == env + 2 && a.slice(2).contour == c + 2, "slice");
    CHECK(!WaveAsk{}.needs_scan() && !WaveStages{}.needs_scan() && WaveStages{}.inconsistent(nullptr) == nullptr, "an encoder-taps call has none");
}

int main(int argc, char **argv)
{
    if (argc != 2 || std::string(argv[1]) != "cases")
    {
        fprintf(stderr, "usage: wave_stages_check cases\n");
        return 2;
    }
    const size_t shapes[3][3] = {{1, 9, 40}, {3, 96, 192}, {64, 2048, 65536}};
    for (const auto &sh : shapes)
        for (int subset = 0; subset < 64; subset++)
            for (int asks = 0; asks < 27; asks++)        // per table stage: frames, phonemes, both
            {
                WaveAsk a;
                for (int s = 0; s < WS_COUNT; s++) a.on[s] = (subset >> s) & 1;
                int code = asks;
                bool repeat = false;
                for (int s : {WS_CONTOUR, WS_PITCH, WS_BANDS})
                {
                    const int m = code % 3 + 1;
                    code /= 3;
                    if (!a.on[s]) repeat = repeat || m != 1;      // an off stage has one ask: none
                    a.frames[s] = a.on[s] && (m & 1);
                    a.phonemes[s] = a.on[s] && (m & 2);
                }
                if (!repeat) one_case(a, sh[0], sh[1], sh[2]);
            }
    ask_rules();
    printf("ok %ld\n", g_checks);
    return 0;
}
