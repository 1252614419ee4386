// model.h — the model object behind zv_model: GGUF weights re-laid-out in HBM, a static activation
// arena and the fixed kernel schedule of the three stages.
//
// Replaces ZeroVOXModel's loader (reference src/zerovox.cpp:21-179) and the three ggml graphs built in
// the stage constructors (src/fs2encoder.cpp:477-586, src/stylettsdec.cpp:306-449, src/hifigan.cpp:187-356).
#pragma once

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "common.h"
#include "gguf_reader.h"
#include "graph_cache.h"
#include "kernels.h"
#include "stage_range.h"
#include "wave_stages.h"

namespace zv
{

// one Conv1d layer resident in HBM: weights in MFMA fragment order, bias padded with zeros
struct ConvW
{
    void  *w = nullptr;
    void  *w8 = nullptr;        // conv_gemm_kernel's stream order (wide decoder convs), or null
    float *bias = nullptr;
    int    K = 0, Cin = 0, Cout = 0, Cin_p = 0, Cout_p = 0, ck = 0;
};

struct DeviceArena
{
    char  *base = nullptr;
    size_t cap = 0, used = 0;
    // an arena that only counts: no memory behind it, take() hands out null and `used` ends up as the bytes a layout needs
    static DeviceArena counter() { return DeviceArena{nullptr, SIZE_MAX, 0}; }
    void  *take(size_t bytes)
    {
        const size_t a = region_align(used);      // every region starts on a 256-byte boundary (wave_stages.h)
        if (a + bytes > cap) fail(ZV_ERR_OOM, "device arena overflow (%zu + %zu > %zu)", a, bytes, cap);
        used = a + bytes;
        return base ? base + a : nullptr;
    }
    template <typename T> T *take_n(size_t n) { return (T *)take(n * sizeof(T)); }
};

struct ProfEntry
{
    const char *name;
    hipEvent_t  e0, e1;
    double      bytes, flops;
    int         launches;       // consecutive launches of the same family bracketed by this event pair
};

// One call's utterances (host side).  Tensors of a batch are row-concatenated: utterance u owns the token rows /
// frame rows its table entries name (kernels.h: Seg / Segs).  `nseg`, `n_max`, `t_max`, `n_rows`, `t_rows` are
// CAPACITIES: they size grids and the arena, the real extents are read from the tables on the device, so one captured
// graph serves every batch that fits.  A single utterance needs no table (inline segment).
// A NEW FIELD: decide in same_schedule() below whether it keys a captured graph; whatever changes a grid, an arena offset or a kernel
// argument does.  A pointer of a waveform stage belongs in the group (`wave`, wave_stages.h), which is keyed as a whole.  Deliberately not keyed: n_real (only host-side checks read it, the kernels take the real extents from the tables);
// the destination and size of chain_dev's input upload (they follow from the keyed buffers).
struct Batch
{
    int        nseg = 1;
    int        n_max = 0, t_max = 0;        // >= every utterance's phonemes / frames
    int        n_real = 0;                  // the longest utterance's real phoneme count (checks)
    size_t     n_rows = 0, t_rows = 0;      // >= sum of phonemes / frames (rows of the concatenated buffers)
    const Seg *d_tok = nullptr, *d_frm = nullptr;
    Seg        tok1{0, 0, 0, 0}, frm1{0, 0, 0, 0};
    // prosody controls, f32 [nseg][CTL_STRIDE] in HBM (kernels.h CTL_*), or null: the uncontrolled schedule.  Part of a graph's
    // key (the kernels' arguments differ); the VALUES are read at run time, so a replay picks up new ones.
    const float *d_ctl = nullptr;
    // per-phoneme controls, f32 [n_rows][PCTL_STRIDE] in HBM indexed by absolute token row (kernels.h PCTL_*), or null; keyed and read
    // like d_ctl
    const float *d_pctl = nullptr;
    // where the length regulator stores its scan (the `cum` tap, int32 [n_rows]) when it must outlive the encoder (phoneme timings of a
    // chain: the decoder and the vocoder reuse the arena), or null: the arena
    int32_t *d_cum = nullptr;
    // Fitted mode: the LIVE frame table, Seg [nseg] in HBM outside the arena, or null.  The encoder writes it behind the length
    // regulator (live[u] = {d_frm[u].row0, n_frames[u], 0, 0}, kernels.h launch_live_frames) and everything after the regulator —
    // decoder, vocoder — takes its extents from it, so an utterance is decoded and vocoded as exactly n_frames[u] frames; buffers,
    // grids and the regulator itself stay by capacity.  A single utterance has a one-entry table.  Keyed like d_ctl: a fitted and
    // an unfitted schedule are different graphs, and a fitted graph replays for new lengths.
    Seg *d_frm_live = nullptr;
    // Run-shortened decoding (dec_runs.h, kernels.h launch_dec_runs): the decoder's run table, Seg [nseg] in HBM outside the arena, or
    // null.  The encoder writes it behind the length regulator from the frame counts and the decoder takes every extent from it; the
    // entry points set it where Model::dec_plan's `runs` says so.  A single utterance has a one-entry table.  Keyed like d_frm_live.
    // A batch's block holds nseg + 1 entries: densely packed decoding (dec_runs.h, Model::dec_plan's `pack`) writes the packed rows as one
    // segment into the last.
    Seg *d_dec_runs = nullptr;
    // Target durations (include/zerovox_amd.h "target durations"): some utterance's ctl row carries a target frame count, so the
    // encoder launches fit_durations_kernel ahead of the length regulator (d_ctl and d_pctl are then both set).  Keyed: one launch
    // more.  WHICH utterances have a target, and its value, is read at run time: a replay picks up new targets.
    bool has_targets = false;
    // The waveform stages behind the vocoder's output convolution (wave_stages.h: volume, envelope, contour, pitch track, band levels,
    // filter): their device pointers, all null where a stage is off.  Keyed as a whole, bytewise; a sub-batch takes its group().
    WaveStages wave;

    static Batch single(uint32_t N, uint32_t T, uint32_t num_phonemes)
    {
        Batch b;
        b.n_max = (int)N;
        b.n_real = (int)N;
        b.t_max = (int)T;
        b.n_rows = N;
        b.t_rows = T;
        b.tok1 = Seg{0, (int32_t)N, (int32_t)num_phonemes, 0};
        b.frm1 = Seg{0, (int32_t)T, 0, 0};
        return b;
    }
    Segs tokens() const { return Segs{d_tok, nseg, n_max, tok1}; }
    // every token row of the batch as ONE segment (table entry nseg: rows [0, sum of phonemes)) — for the per-token layers, whose row
    // tiles then pack the utterances densely instead of padding every utterance to a tile
    Segs tokens_merged() const { return d_tok ? Segs{d_tok + nseg, 1, (int)n_rows, tok1} : tokens(); }
    // the frames by capacity: buffer layout, the length regulator's clamps and zero fill
    Segs frames_cap() const { return Segs{d_frm, nseg, t_max, frm1}; }
    // the frames the decoder and the vocoder run over: the live table in fitted mode, else the capacity
    Segs frames() const { return d_frm_live ? Segs{d_frm_live, nseg, t_max, frm1} : frames_cap(); }
    // what of a Batch a captured schedule depends on: the capacities (grids, arena layout), the table pointers, the inline segments
    // where there is no table, the optional pointers that change the kernels' arguments, the flag that adds a launch and the waveform
    // stages' group
    bool same_schedule(const Batch &o) const
    {
        return nseg == o.nseg && n_max == o.n_max && t_max == o.t_max && n_rows == o.n_rows && t_rows == o.t_rows && d_tok == o.d_tok &&
               d_frm == o.d_frm && (d_tok || memcmp(&tok1, &o.tok1, sizeof(Seg)) == 0) && (d_frm || memcmp(&frm1, &o.frm1, sizeof(Seg)) == 0) &&
               d_ctl == o.d_ctl && d_pctl == o.d_pctl && d_cum == o.d_cum && d_frm_live == o.d_frm_live && has_targets == o.has_targets &&
               d_dec_runs == o.d_dec_runs && wave == o.wave;
    }
};

// a captured schedule: replayed when the same entry point is called with the same Batch (same_schedule) and buffers
struct CapturedGraph
{
    static constexpr int NKEY = 8;         // the buffers of a call that are not part of its Batch (chain_dev)
    int            kind = 0;               // 0 vocoder, 1 chain, 2 chain up to the vocoder's tail; + 4 * StageRange::key() for a stage batch
    int            lane = 0;               // the lane that captured it
    unsigned       epoch = 0;              // knob_epoch() at capture
    Batch          b;
    const void    *p[NKEY] = {};
    hipGraphExec_t exec = nullptr;
    const Seg     *runs_tab = nullptr;     // the run table its vocoder writes (Model::voc_runs_last), or null
    int            runs_n = 0;
};

class Model
{
  public:
    Model(const std::string &gguf_path, int device);
    ~Model();

    zv_hparams hp{};
    int        device = 0;
    int        n_cu = 256;
    hipStream_t stream() const { return lanes_[cur_lane_].stream; }      // the selected lane's

    // ---- stages (device pointers in, device pointers out; everything enqueued on stream()) ----
    // every tensor is the row concatenation over the batch: mel [t_rows][M], wav [t_rows * hop], hidden [t_rows][E],
    // ids / puncts [n_rows], styles [nseg][E]
    void vocode_dev(const Batch &b, const float *d_mel, float *d_wav);
    // part: 0 = the whole schedule, 1 = everything up to and including the last stage's upsample conv, 2 = the last
    // stage's residual blocks + the output conv
    // seg0: the batch's first segment is entry seg0 of the head's run table (vocode_tail)
    void vocode_group(const Batch &b, const float *d_mel, float *d_wav, int part = 0, int seg0 = 0);
    // the tail (part 2) of segments [g0, g0 + cnt) of a batch whose head chain_dev(..., voc_part = 1) has enqueued: same
    // arena layout, same row ranges, same bits as the unsplit schedule
    void vocode_tail(const Batch &b, const float *d_mel, float *d_wav, int g0, int cnt);
    // second stream + events for the waveform download of a finished group under the next group's kernels
    hipStream_t copy_stream();
    hipEvent_t  tail_event(int i);
    // Batches in flight (zv_synthesize_batch_begin) are numbered in the order they are enqueued; each owns a (start, done) pair
    // of timing events on its lane's stream: `start` ahead of its upload, `done` behind its last kernel (zv_batch_timeline).
    static constexpr int BATCH_RING = 64;
    uint64_t    next_batch_seq() { return batch_seq_++; }
    uint64_t    batch_seq() const { return batch_seq_; }
    hipEvent_t  batch_event(uint64_t seq, int which);          // which: 0 start, 1 done
    void decode_dev(const Batch &b, const float *d_hidden, const float *d_styles, float *d_mel);
    // taps are device pointers inside the arena (token rows as in ids), valid until the next call;
    // n_frames [nseg] is written to d_nframes (outside the arena)
    struct EncoderTaps
    {
        float   *features = nullptr, *logdur = nullptr, *pitch = nullptr, *energy = nullptr;
        int32_t *pitch_bucket = nullptr, *energy_bucket = nullptr, *cum = nullptr;
    };
    EncoderTaps encode_dev(const Batch &b, const int32_t *d_ids, const int32_t *d_puncts, const float *d_styles,
                           float *d_hidden, int32_t *d_nframes);

    // One layer at a time (the counterpart of the reference's tensor_dbg, src/utils.cpp:19-44; tests only): while
    // `dbg_layer.kind >= 0` the stage that owns the layer replaces the layer's input with dbg_layer.x (host, time-major,
    // unpadded) right before it runs, copies the layer's output to dbg_layer.out right after it and returns.
    // kinds (include/zerovox_amd.h zv_layer_kind): 0 HiFi-GAN residual block n, 1 encoder FFT block l,
    // 2 decoder residual block b (0,1 encode; 2..6 decode), 3 variance predictor p (0 duration, 1 pitch, 2 energy)
    struct DebugLayer
    {
        int          kind = -1, index = 0;
        const float *x = nullptr;
        float       *out = nullptr;
        bool         done = false;
    } dbg_layer;

    // rows of the sinusoid table = the longest utterance the encoder takes (reference src/fs2encoder.cpp:306-324)
    uint32_t max_phonemes() const { return (uint32_t)enc_.posenc_rows; }
    void reserve(uint32_t max_phonemes, uint32_t max_frames);
    void reserve_batch(const Batch &b);
    int  voc_stage_rate(int stage) const;       // samples per frame after upsample stage `stage`
    int  voc_stage_channels(int stage) const;
    // largest frame count one segment may have: byte offsets inside a segment are 32-bit in the buffer descriptors
    uint32_t max_frames_per_utterance() const;
    int wemb_rows() const { return enc_.wemb_rows; }
    int pemb_rows() const { return enc_.pemb_rows; }
    // receptive field of the vocoder in mel frames per side (input conv + per stage: transposed-conv taps and the widest
    // residual block, converted from the stage's sample rate), rounded up, + 1
    uint32_t vocoder_halo_frames() const;
    // Run-shortened vocoding of the unfitted path (vocoder.cpp): off in fitted mode, under a dbg_layer tap, where the caller asks
    // (zv_vocode_stream: its chunks are the schedule) and by ZV_VOC_RUNS.  voc_runs_last: the selected lane's most recent run table
    // (device, in the lane's arena, valid until the lane's next call) and its entries, or null / 0 when that call ran without one
    bool voc_runs_off = false;
    bool voc_runs_on(const Batch &b) const;
    const Seg *voc_runs_last(int *n) { *n = lane().runs_n; return lane().runs_tab; }
    // The decoder's regime over b (stage_plan.h dec_plan).  runs: whether a chain over b gets a run table (Batch::d_dec_runs) — the
    // unfitted synthesize paths; never a stand-alone decode, whose hidden comes from the caller.  pack: a chain with a run table packs
    // the utterances' compact rows into one row space, which the decoder's convs then run over as one segment (dec_runs.h).
    DecPlan dec_plan(const Batch &b) const
    {
        return zv::dec_plan(b.nseg, b.t_max, b.t_rows, b.d_frm_live != nullptr, dbg_layer.kind >= 0, b.d_dec_runs != nullptr);
    }
    // frames the decoder's 3-tap convs reach to either side, from the loaded layers (the longest path through its blocks)
    int  dec_reach_frames() const;
    void sync();

    // Lanes: independent (stream, activation arena, I/O scratch) triples so that several utterances are in flight at
    // once (zv_synthesize_batch): a single short utterance cannot fill 256 CUs in its narrow stages, four can.
    // stream(), the arena and the scratch blocks are the selected lane's (lanes_ may grow: an index, not a reference); lane 0 is the default.
    void select_lane(int i);
    int  selected_lane() const { return cur_lane_; }
    void sync_all_lanes();
    // Tests (zv_debug_poison): fills the whole capacity of lane i's arena, I/O scratch and pinned staging block with `byte` after
    // waiting for the lane's streams, and forgets its run table (it lay in the arena).  filled[3] = the bytes of each block, 0 for
    // one that is not allocated (all three for a lane never selected).  Allocates nothing, selects nothing, drops no graph.
    void poison_lane(int i, int byte, size_t filled[3]);

    // band levels: the twiddle table in the frames pass's fragment order (bands.h bands_table_fragments, BANDS_TABLE_BYTES of device
    // memory outside the arenas), built on the host and uploaded at the first request, then kept for the model's life.  It allocates
    // and copies synchronously, so the entry points call it before anything is enqueued or captured.
    const void *bands_table();
    // mel analysis: both digit planes of its table likewise (mel.h mel_table_fragments, MEL_TABLE_BYTES)
    const void *mel_table();
    // the two launches of mel analysis on the lane's stream (wave_stages.cpp; kernels.h launch_mel_frames / launch_mel_rows), eager:
    // d_wav the utterances' samples by absolute frame row, d_par the call's parameter block, total_rows the rows of all segments
    void mel_launches(const float *d_wav, double *d_slab, float *d_rows, const uint32_t *d_par, const Segs &frames, size_t total_rows);
    // the five launches of mel alignment over one launch group of pairs, likewise (kernels.h launch_align_*); rows and cells: the group's
    // sequence rows and matrix cells, for the profile's byte and operation counts
    void align_launches(const AlignJob &job, size_t rows, size_t cells);
    // the launches of loudness over one launch group of utterances, likewise (kernels.h launch_loud_*): five of them measure, the sixth
    // scales (apply: the caller wants the waveform back); samples: the group's measured samples, capacity: the samples it scales
    void loud_launches(const LoudJob &job, bool apply, size_t samples, size_t capacity);
    // the launches of the limiter over one launch group of utterances, likewise (kernels.h launch_limit_*); entries: the group's q entries
    void limit_launches(const LimitJob &job, size_t samples, size_t capacity, size_t entries);
    // the launches of resampling over one launch group of utterances, likewise (kernels.h launch_resample*); in, out: the group's samples
    void resample_launches(const ResampleJob &job, size_t in, size_t out);
    // the designed tables of resampling, built on the host at the first request for their (rates, zeros, beta, cutoff) and kept
    struct ResampleDesign
    {
        uint32_t rate_in, rate_out, zeros;
        float beta, cutoff;
        uint32_t L, M, P;
        std::vector<float> table;
    };
    std::vector<ResampleDesign> resample_designs;

    // scratch for host-buffer entry points (grows on demand)
    void *io_scratch(size_t bytes);
    // pinned host staging for batched D2H copies (an async copy into pageable memory blocks the host and would
    // serialise the lanes)
    void *pinned_scratch(size_t bytes);

    // graph replay of the vocoder schedule
    bool graph_mode = false;
    // The cache of captured graphs (graph_cache.h holds the policy, DESIGN.md "Serving under changing shapes" the lifetime rule).
    // set_graph_cache: 1 .. 1024 slots, shrinking evicts by the victim rule and waits for no lane; false for a capacity out of range.
    // graph_stats: the counters since load; queries nothing on the device.
    bool set_graph_cache(uint64_t capacity);
    void graph_stats(zv_graph_stats *out) const;
    void vocode_dev_graph(const Batch &b, const float *d_mel, float *d_wav);
    // encoder -> decoder -> vocoder back to back (graph replay keyed by (capacities, buffers) when graph_mode is on).
    // h2d_src / h2d_dst / h2d_bytes (optional): an input upload that becomes the first node of the schedule
    // range (stage_range.h): the stages that are enqueued, the full chain by default; a shorter range reads d_hidden / d_mel as the
    // caller filled them, ignores the pointers of the stages it leaves out, and keys its graphs apart from the chain's
    void chain_dev(const Batch &b, const int32_t *d_ids, const int32_t *d_puncts, const float *d_styles, float *d_hidden,
                   float *d_mel, float *d_wav, int32_t *d_nframes, const void *h2d_src = nullptr, void *h2d_dst = nullptr,
                   size_t h2d_bytes = 0, int voc_part = 0, StageRange range = StageRange());

    // profiling (HIP events around every launch while enabled)
    bool profiling = false;
    std::vector<ProfEntry> prof;
    void prof_clear();

    uint32_t E() const { return hp.emb_dim + hp.punct_emb_dim; }
    // ZV_LAYER_ENC_LN (zv_debug_layer): one encoder LayerNorm alone on dbg_layer.x, outside the encoder's schedule
    void debug_layernorm(int index, uint32_t n);

  private:
    // ---- weights ----
    std::vector<void *> allocs_;
    void  *bands_table_ = nullptr, *mel_table_ = nullptr;
    void  *dev_alloc(size_t bytes);
    float *upload_f32(const GgufTensor &t, int pad_to = 0, float pad_value = 0.f);
    float *upload_vec(const GgufFile &g, const std::string &name, int expect_n, int pad_to = 0, float pad_value = 0.f);
    ConvW  load_conv(const GgufFile &g, const std::string &wname, const std::string &bname, int expect_cin = -1, bool gemm_pack = false);
    ConvW  load_upsample(const GgufFile &g, int idx, int stride, int expect_cin);

    // p1/p2: 32 x 32 x 16 fragment order (resblock_triple_kernel), x1/x2: 16 x 16 x 32 order (pair kernel, block32), r1/r2: LDS-ring stream (64 channels)
    struct ResPair { ConvW c1, c2; void *p1 = nullptr, *p2 = nullptr, *r1 = nullptr, *r2 = nullptr, *x1 = nullptr, *x2 = nullptr; };
    struct Voc
    {
        float *mean = nullptr, *scale = nullptr;
        ConvW  in_conv;
        int    n_up = 0;
        int    scales[8] = {0};
        ConvW  ups[8];
        int    n_rb = 0, n_dil = 3;
        int    dil[8] = {1, 3, 5};
        std::vector<ResPair> pairs;       // [(stage*n_rb + j)*n_dil + d]
        uint16_t *out_w = nullptr;        // f16 [K][Cp]
        float  out_b = 0.f;
        int    out_K = 0, out_C = 0;
    } voc_;
    // what of voc_ the schedule's decisions read (voc_plan.h), and a call's numbers; vocode_group issues what voc_plan says of the two
    VocGeom voc_geom_{};
    VocCall voc_call(const Batch &b) const;
    // vocode_group's job filling: a branch's first n_dil dilation pairs as one whole-block job (ring: launch_block64's weights), and
    // one dilation pair as the two convs' jobs and as the fused kernel's
    TripleJob block_job(const ResPair *rp, int n_dil, bool ring, const float *y, float *out) const;
    struct DilPairJobs { ConvJob c1, c2; PairJob p; };
    DilPairJobs pair_jobs(const ResPair &rp, int dil, const float *yin, float *yout, _Float16 *xt, float *y) const;

    struct DecBlk
    {
        ConvW  conv1, conv2, sc;
        bool   learned_sc = false;
        int    cin = 0, cout = 0;
        float *n1w = nullptr, *n1b = nullptr, *n2w = nullptr, *n2b = nullptr;   // encode blocks: affine IN
        int    g1 = 0, g2 = 0;                                                   // decode blocks: offsets into adain h
    };
    struct Dec
    {
        DecBlk enc[2], dec[5];
        ConvW  asr0, to_out;
        float *asr1w = nullptr, *asr1b = nullptr;
        float *fcW = nullptr, *fcB = nullptr, *fcExtra = nullptr;   // all 10 AdaIN fc layers concatenated
        int    fc_out = 0;
        int    R = 64, M = 80;
    } dec_;

    struct EncLayer
    {
        float *qkvW = nullptr, *qkvB = nullptr, *fcW = nullptr, *fcB = nullptr;
        float *ln1w = nullptr, *ln1b = nullptr, *ln2w = nullptr, *ln2b = nullptr;
        ConvW  w1, w2;
    };
    struct VarPred
    {
        ConvW  c1, c2;
        float *l1w = nullptr, *l1b = nullptr, *l2w = nullptr, *l2b = nullptr, *lw = nullptr, *lb = nullptr;
        int    V = 0;
    };
    struct Enc
    {
        float *wemb = nullptr, *pemb = nullptr, *posenc = nullptr, *pitch_emb = nullptr, *energy_emb = nullptr;
        int    posenc_rows = 0, wemb_rows = 0, pemb_rows = 0;
        std::vector<EncLayer> layers;
        VarPred dur, pitch, energy;
    } enc_;

    // ---- activations ----
    // One layout per stage states the stage's buffers in the arena, in carving order.  The stage calls it on the lane's arena for its
    // pointers; arena_bytes_for calls the very same function on DeviceArena::counter() and reads the bytes used.  Invariants:
    //   * every stage asks for the largest of the three layouts + ARENA_TAIL, so a chain never regrows the arena between stages;
    //   * run_captured reserves before capture begins (hipMalloc cannot be captured) with the Batch the stages size by, so the
    //     arena_require a stage issues inside the capture asks for the same bytes; no layout shrinks when a capacity grows, so a
    //     sub-batch (vocode_tail) or a Batch that has gained d_cum never asks for more than the reservation did;
    //   * vocode_tail (part 2 of a split batch) sees the layout the head (part 1) carved: voc_layout reads t_rows alone, but for the
    //     size of its last carve (the run table) and whether the batch carries a filter, which a sub-batch keeps.
    struct VocLayout
    {
        float *c0;
        struct Stage { float *ub, *y[3]; _Float16 *xt[3]; } st[8];      // stage i: ping-pong pool i & 1
        // run-shortened schedule (kernels.h launch_voc_runs), behind the pools so that a sub-batch finds them where the head put them:
        // the compacted mel, the row flags, the run table (one entry per segment: the only carve that reads nseg, hence the last)
        // volume controls (kernels.h launch_level_measure): the partial totals, 16 bytes per (segment, chunk).  Sized by t_rows alone
        // (level_slab_entries) and carved in front of the run table, so that a sub-batch finds the table where the head put it
        void *level_slab;
        // amplitude envelope (kernels.h launch_env_knots): the knots, one uint32 per frame and one more per segment.  Sized by t_rows
        // alone (env_knot_entries) and carved in front of the run table like the slab
        uint32_t *env_knots;
        // level contour (kernels.h launch_contour_frames): the frames' totals, 16 bytes per frame row, t_rows entries, carved in front
        // of the run table like the slab
        void *contour_slab;
        // pitch track (kernels.h launch_pitch_frames): {Fq, voiced} per frame row, 8 bytes each, t_rows entries, carved likewise
        void *pitch_slab;
        // waveform filter (kernels.h launch_filter): the vocoder's waveform ahead of the filter, t_rows * hop floats indexed like the
        // waveform, carved likewise and only where the batch carries a filter (WaveStages::d_flt_par); null otherwise
        float *filter_in;
        float *mel_c; int32_t *eq; Seg *runs;
    };
    // entries of VocLayout::level_slab: >= nseg * level_chunks(t_max, hop) for every Batch with nseg * t_max <= t_rows, a sub-batch included
    size_t level_slab_entries(const Batch &b) const;
    // entries of VocLayout::env_knots: >= t_rows + nseg for every Batch with nseg * t_max <= t_rows, a sub-batch included
    size_t env_knot_entries(const Batch &b) const;
    struct DecLayout
    {
        int    nblk, hs, ss;        // per segment: statistics blocks, floats of AdaIN vectors, floats of (mean, rstd) pairs
        int    rows, nblk_all;      // rows of every [rows] buffer (dec_pack_rows_cap: the packed rows fit whatever the lengths), statistics blocks of part_t / part_o
        float *h, *st_x, *st_t, *st_y, *st_a, *cat, *t1, *sc, *x0, *xa, *asr_t;
        double *part_t, *part_o; _Float16 *xa16, *t16, *xr16;
        float *mel_c;       // run-shortened decoding: the compact mel the last conv writes (launch_dec_run_expand reads it)
    };
    struct EncLayout { int Vp; float *x, *y, *qkv, *o, *f, *va, *vb; _Float16 *hh; EncoderTaps t; };
    VocLayout voc_layout(DeviceArena &a, const Batch &b) const;
    // the launches of the waveform stages over a (sub-)batch's finished waveform (wave_stages.cpp), behind vocode_group's output conv
    void wave_stage_launches(const Batch &b, const VocLayout &lay, float *d_wav, int rate, int seg0);
    DecLayout dec_layout(DeviceArena &a, const Batch &b) const;
    EncLayout enc_layout(DeviceArena &a, const Batch &b) const;
    // the arena's one margin, behind the largest layout: reads that run past a stage's last buffer stay inside the allocation
    static constexpr size_t ARENA_TAIL = (size_t)1 << 20;
    size_t arena_bytes_for(const Batch &b) const;
    void  arena_require(size_t bytes);
    DeviceArena &stage_arena(const Batch &b);       // the selected lane's arena, large enough for every stage of b, rewound

    // ---- launch helpers ----
    void conv(const ConvJob *jobs, int n, const Segs &segs, int rate, const char *name, double bytes, double flops);
    void dbg_inject(void *dev, int ld, int cols, size_t rows);
    void dbg_extract(const void *dev, int ld, int cols, size_t rows);
    ConvJob job(const ConvW &w) const;
    void tick(hipEvent_t *e0);
    void tock(hipEvent_t e0, const char *name, double bytes, double flops);
    void group_begin();
    void group_end(const char *name);
    bool       in_group_ = false;
    hipEvent_t group_e0_ = nullptr;
    double     group_bytes_ = 0.0, group_flops_ = 0.0;
    int        group_n_ = 0;

    struct Lane
    {
        hipStream_t stream = nullptr;
        DeviceArena arena;
        void       *io = nullptr;
        size_t      io_cap = 0;
        // host staging block, download stream and events of the lane (a batch in flight per lane: zv_synthesize_batch_begin)
        void       *pinned = nullptr;
        size_t      pinned_cap = 0;
        hipStream_t copy_stream = nullptr;
        std::vector<hipEvent_t> tail_events;
        const Seg  *runs_tab = nullptr;      // voc_runs_last
        int         runs_n = 0;
    };
    std::vector<Lane> lanes_;
    int  cur_lane_ = 0;
    Lane &lane() { return lanes_[cur_lane_]; }
    uint64_t   batch_seq_ = 0;
    hipEvent_t batch_events_[2 * BATCH_RING] = {};

    bool skip_launch_ = false;    // vocode_group: the launches of the part that is not asked for are skipped
    // A slot belongs to the lane that captured it: its graph names that lane's arena, I/O block and pinned block, the caller's own
    // device buffers (zv_vocode_device, lane 0) and model-lifetime blocks (weights, bands_table), nothing of another lane, and only
    // that lane's stream ever replays it (the lane is part of the key).
    GraphCache<CapturedGraph> graphs_;
    // an exec that has left the cache while its lane's stream may still be replaying it, and the event recorded on that stream then
    struct RetiredExec { hipGraphExec_t exec; hipEvent_t done; };
    RetireList<RetiredExec> retired_;
    void retire_graph(CapturedGraph &&g, int lane);     // destroys the exec once its lane has passed it; waits for no lane
    void sweep_retired();                               // destroys what has finished (a query per entry)
    void drop_lane_graphs();                            // the selected lane's slots; its stream has just been synchronised
    void drop_graphs();                                 // every slot and the retire list, after synchronising every lane (teardown)
    template <typename F> void run_captured(int kind, const Batch &b, const void *const (&key)[CapturedGraph::NKEY], F &&enqueue);
};

}  // namespace zv
