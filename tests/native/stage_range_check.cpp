// Host-side driver of csrc/stage_range.h for tests/test_stage_range_cpu.py (no GPU, no HIP).
//   stage_range_check cases
//       every stage range [first, last] x the request's options (controls, phoneme controls, timings, fitted, a few asks of the waveform
//       stages) x three shapes x all / some / none of the utterances wanting their rows back: every region 256-aligned, the regions of
//       a block in ascending order without overlap and inside the block's size, a region the range does not touch empty, the regions
//       the range needs present with the bytes written out below; and for the full range every offset and size of the three blocks as
//       capi.cpp's batch_enqueue carved them inline before the header existed (restated below in that code's order).
//       Prints "ok <checks>".
#include "stage_range.h"

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

// batch_enqueue's layout as it stood: the chain's three blocks.  SEG = sizeof(zv::Seg) = 16, CTL_STRIDE = 8, PCTL_STRIDE = 4.
struct Old
{
    size_t i_tok, i_frm, i_ids, i_pun, i_sty, i_ctl, i_pctl, b_in;
    size_t o_nf, o_in, o_hid, o_mel, o_wav, o_cum, o_live, o_runs, dev_size;
    size_t p_in, p_nf, p_wav, p_cum, host_size;
    WaveOffsets wo;
};
static Old old_batch(const BatchShape &q, const WaveAsk &ask)
{
    Old o;
    const size_t SEG = 16, CTL_STRIDE = 8, PCTL_STRIDE = 4, E = q.E, Mm = q.mels, hop = q.hop;
    const bool   ctl = q.ctl, pc = q.pctl, dur = q.timings, fitted = q.fitted;
    Layout in;
    const size_t b_tab = (q.nseg + 1) * SEG;
    o.i_tok = in.at(b_tab), o.i_frm = in.at(b_tab), o.i_ids = in.at(q.n_rows * 4), o.i_pun = in.at(q.n_rows * 4);
    o.i_sty = in.at(q.nseg * E * 4), o.i_ctl = in.at(ctl ? q.nseg * CTL_STRIDE * 4 : 0), o.i_pctl = in.at(pc ? q.n_rows * PCTL_STRIDE * 4 : 0);
    const WaveRows cap_rows{q.nseg, q.n_rows, q.t_rows};
    wave_carve(in, ask, cap_rows, WR_INPUT, o.wo);
    o.b_in = in.size();
    Layout dev;
    o.o_nf = dev.at(q.nseg * 4), o.o_in = dev.at(o.b_in), o.o_hid = dev.at(q.t_rows * E * 4), o.o_mel = dev.at(q.t_rows * Mm * 4);
    o.o_wav = dev.at(q.t_rows * hop * 4), o.o_cum = dev.at(dur || ask.needs_scan() ? q.n_rows * 4 : 0);
    o.o_live = dev.at(fitted ? q.nseg * SEG : 0), o.o_runs = dev.at(!fitted ? (q.nseg + 1) * SEG : 0);
    wave_carve(dev, ask, cap_rows, WR_DEVICE, o.wo);
    o.dev_size = dev.size();
    Layout host;
    const size_t wav_bytes = q.n_frames * hop * 4;      // every utterance's waveform, T[u] * hop * 4 each
    o.p_in = host.at(o.b_in), o.p_nf = host.at(q.nseg * 4), o.p_wav = host.at(wav_bytes), o.p_cum = host.at(dur ? q.n_rows * 4 : 0);
    wave_carve(host, ask, WaveRows{q.nseg, q.n_tokens, q.n_frames}, WR_HOST, o.wo);
    o.host_size = host.size();
    return o;
}

// the regions [a, b] of one block, with the waveform stages' regions of `role` where they are carved (behind region `wave_after`):
// aligned, ascending, disjoint, inside `size`
static void check_block(const BatchOffsets &o, const StageRange &r, const BatchShape &q, const WaveAsk &ask, int a, int b, int wave_after, int role,
                        const WaveRows &rows, size_t size, const char *what)
{
    size_t end = 0;
    auto span = [&](size_t off, size_t bytes, int id) {
        CHECK(off % 256 == 0, "%s region %d at %zu", what, id, off);
        CHECK(off >= end, "%s region %d at %zu overlaps the one before (ends %zu)", what, id, off, end);
        end = off + bytes;
        CHECK(end <= size, "%s region %d ends at %zu past the block's %zu", what, id, end, size);
    };
    const WaveAsk voc_ask = r.has(ST_VOCODER) ? ask : WaveAsk{};
    for (int id = a; id <= b; id++)
    {
        span(o.at[id], batch_region_bytes(id, r, q, voc_ask, o.in_bytes), id);
        if (id == wave_after)
            for (int w = 0; w < R_COUNT; w++)
                if (WAVE_REGIONS[w].role == role) span(o.wave.at[w], wave_region_bytes(w, voc_ask, rows), 100 + w);
    }
    CHECK(size % 256 == 0 && size >= end, "%s size %zu", what, size);
}

int main(int argc, char **argv)
{
    if (argc < 2 || std::string(argv[1]) != "cases") return 2;
    struct Shape { size_t nseg, n_rows, t_rows, n_tokens, n_frames; };
    const Shape shapes[] = {{1, 32, 64, 9, 40}, {3, 96, 192, 30, 81}, {64, 2048, 65536, 1000, 60000}};
    const size_t E = 528, Mm = 80, hop = 256;
    std::vector<WaveAsk> asks(4);
    asks[1].on[WS_VOLUME] = true;
    asks[2].on[WS_ENVELOPE] = asks[2].on[WS_FILTER] = true;
    for (int s : {WS_CONTOUR, WS_PITCH, WS_BANDS}) asks[3].on[s] = asks[3].frames[s] = asks[3].phonemes[s] = true;
    static_assert(StageRange().full() && StageRange().key() == 0, "a request is the chain unless it says otherwise");
    int keys[ST_COUNT * ST_COUNT + 1] = {};
    for (int first = 0; first < ST_COUNT; first++)
        for (int last = first; last < ST_COUNT; last++)
        {
            const StageRange r{first, last};
            CHECK(r.valid() && r.key() >= 0 && r.key() <= ST_COUNT * ST_COUNT && keys[r.key()]++ == 0, "range %d..%d key %d", first, last, r.key());
            CHECK((r.key() == 0) == r.full(), "only the chain has key 0");
            const bool enc = first == ST_ENCODER, dec = first <= ST_DECODER && last >= ST_DECODER, voc = last == ST_VOCODER;
            CHECK(r.has(ST_ENCODER) == enc && r.has(ST_DECODER) == dec && r.has(ST_VOCODER) == voc, "has");
            for (const Shape &sh : shapes)
                for (int opt = 0; opt < 16; opt++)
                    for (const WaveAsk &ask : asks)
                        for (int want = 0; want < 3; want++)      // the rows of all, half, none of the frames travel back
                        {
                            BatchShape q;
                            q.nseg = sh.nseg, q.n_rows = sh.n_rows, q.t_rows = sh.t_rows, q.E = E, q.mels = Mm, q.hop = hop;
                            q.ctl = opt & 1, q.pctl = opt & 2, q.timings = opt & 4, q.fitted = (opt & 8) && r.full();
                            q.n_tokens = enc ? sh.n_tokens : 0, q.n_frames = sh.n_frames;
                            const size_t out_row = stage_row_floats(r.result(), q) * 4;
                            CHECK(out_row == (last == ST_ENCODER ? E : last == ST_DECODER ? Mm : hop) * 4, "result row");
                            q.result_bytes = (want == 0 ? sh.n_frames : want == 1 ? sh.n_frames / 2 : 0) * out_row;
                            q.source_bytes = enc ? 0 : sh.n_frames * stage_row_floats(r.source(), q) * 4;
                            CHECK(enc || q.source_bytes == sh.n_frames * (first == ST_DECODER ? E : Mm) * 4, "source row");
                            const BatchOffsets o = batch_carve(r, q, ask);
                            check_block(o, r, q, ask, BI_TOK, BI_PCTL, BI_PCTL, WR_INPUT, WaveRows{q.nseg, q.n_rows, q.t_rows}, o.in_bytes, "input");
                            check_block(o, r, q, ask, BD_NF, BD_RUNS, BD_RUNS, WR_DEVICE, WaveRows{q.nseg, q.n_rows, q.t_rows}, o.dev_bytes, "device");
                            check_block(o, r, q, ask, BP_IN, BP_SRC, BP_CUM, WR_HOST, WaveRows{q.nseg, q.n_tokens, q.n_frames}, o.pin_bytes, "pinned");
                            // what the range touches is there with its bytes, what it does not touch is empty
                            const WaveAsk va = voc ? ask : WaveAsk{};
                            auto bytes = [&](int id) { return batch_region_bytes(id, r, q, va, o.in_bytes); };
                            const size_t tab = (q.nseg + 1) * 16;
                            CHECK(bytes(BI_FRM) == tab && bytes(BI_TOK) == (enc ? tab : 0), "tables");
                            CHECK(bytes(BI_IDS) == (enc ? q.n_rows * 4 : 0) && bytes(BI_PUN) == bytes(BI_IDS), "ids");
                            CHECK(bytes(BI_STY) == (enc || dec ? q.nseg * E * 4 : 0), "styles");
                            CHECK(bytes(BI_CTL) == (enc && q.ctl ? q.nseg * 32 : 0) && bytes(BI_PCTL) == (enc && q.pctl ? q.n_rows * 16 : 0), "controls");
                            CHECK(bytes(BD_NF) == (enc ? q.nseg * 4 : 0) && bytes(BP_NF) == bytes(BD_NF), "frame counts");
                            CHECK(bytes(BD_IN) == o.in_bytes && bytes(BP_IN) == o.in_bytes, "input block");
                            CHECK(bytes(BD_HID) == (first <= ST_DECODER ? q.t_rows * E * 4 : 0), "hidden");
                            CHECK(bytes(BD_MEL) == (last >= ST_DECODER ? q.t_rows * Mm * 4 : 0), "mel");
                            CHECK(bytes(BD_WAV) == (voc ? q.t_rows * hop * 4 : 0), "wav");
                            CHECK(bytes(BD_CUM) == (enc && (q.timings || (voc && ask.needs_scan())) ? q.n_rows * 4 : 0), "scan");
                            CHECK(bytes(BP_CUM) == (enc && q.timings ? q.n_rows * 4 : 0), "scan staging");
                            CHECK(bytes(BD_LIVE) == (q.fitted ? q.nseg * 16 : 0), "live table");
                            CHECK(bytes(BD_RUNS) == (enc && dec && !q.fitted ? tab : 0), "run table");
                            CHECK(bytes(BP_OUT) == q.result_bytes && bytes(BP_SRC) == q.source_bytes, "what travels");
                            for (int w = 0; w < R_COUNT; w++)
                                CHECK(voc || wave_region_bytes(w, va, WaveRows{q.nseg, q.n_rows, q.t_rows}) == 0, "a waveform stage without the vocoder");
                            if (!voc)      // ... so its blocks are those of a request that asks for none
                            {
                                const BatchOffsets plain = batch_carve(r, q, WaveAsk{});
                                CHECK(o.in_bytes == plain.in_bytes && o.dev_bytes == plain.dev_bytes && o.pin_bytes == plain.pin_bytes &&
                                          o.at[BP_SRC] == plain.at[BP_SRC],
                                      "blocks of %d..%d grow with the waveform stages", first, last);
                            }
                            if (!r.full() || want != 0) continue;
                            // the chain: the layout as it stood, offset by offset
                            const Old old = old_batch(q, ask);
                            CHECK(o.at[BI_TOK] == old.i_tok && o.at[BI_FRM] == old.i_frm && o.at[BI_IDS] == old.i_ids && o.at[BI_PUN] == old.i_pun &&
                                      o.at[BI_STY] == old.i_sty && o.at[BI_CTL] == old.i_ctl && o.at[BI_PCTL] == old.i_pctl && o.in_bytes == old.b_in,
                                  "the chain's input block");
                            CHECK(o.at[BD_NF] == old.o_nf && o.at[BD_IN] == old.o_in && o.at[BD_HID] == old.o_hid && o.at[BD_MEL] == old.o_mel &&
                                      o.at[BD_WAV] == old.o_wav && o.at[BD_CUM] == old.o_cum && o.at[BD_LIVE] == old.o_live &&
                                      o.at[BD_RUNS] == old.o_runs && o.dev_bytes == old.dev_size,
                                  "the chain's device block");
                            CHECK(o.at[BP_IN] == old.p_in && o.at[BP_NF] == old.p_nf && o.at[BP_OUT] == old.p_wav && o.at[BP_CUM] == old.p_cum &&
                                      o.pin_bytes == old.host_size,
                                  "the chain's pinned block");
                            for (int w = 0; w < R_COUNT; w++) CHECK(o.wave.at[w] == old.wo.at[w], "the chain's waveform region %d", w);
                        }
        }
    printf("ok %ld\n", g_checks);
    return 0;
}
