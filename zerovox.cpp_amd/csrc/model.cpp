// model.cpp — the runtime: lanes, scratch blocks, the activation arena, launch and profiling helpers, the graph cache (see model.h).
#include "schedule.h"

#include <algorithm>

namespace zv
{

Model::~Model()
{
    hipSetDevice(device);
    for (Lane &l : lanes_) hipStreamSynchronize(l.stream);       // (a lane is never without its stream)
    drop_graphs();
    prof_clear();
    for (void *p : allocs_) hipFree(p);
    for (hipEvent_t e : batch_events_)
        if (e) hipEventDestroy(e);
    for (Lane &l : lanes_)
    {
        if (l.copy_stream) hipStreamSynchronize(l.copy_stream);
        if (l.arena.base) hipFree(l.arena.base);
        if (l.io) hipFree(l.io);
        if (l.pinned) hipHostFree(l.pinned);
        for (hipEvent_t e : l.tail_events) hipEventDestroy(e);
        if (l.copy_stream) hipStreamDestroy(l.copy_stream);
        if (l.stream) hipStreamDestroy(l.stream);
    }
}

void Model::sync() { ZV_HIP(hipStreamSynchronize(stream())); }

hipStream_t Model::copy_stream()
{
    Lane &l = lane();
    if (!l.copy_stream) ZV_HIP(hipStreamCreateWithFlags(&l.copy_stream, hipStreamNonBlocking));
    return l.copy_stream;
}

hipEvent_t Model::batch_event(uint64_t seq, int which)
{
    hipEvent_t &e = batch_events_[2 * (seq % BATCH_RING) + which];
    if (!e) ZV_HIP(hipEventCreate(&e));
    return e;
}

hipEvent_t Model::tail_event(int i)
{
    std::vector<hipEvent_t> &ev = lane().tail_events;
    while ((int)ev.size() <= i)
    {
        hipEvent_t e;
        ZV_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        ev.push_back(e);
    }
    return ev[i];
}

void Model::select_lane(int i)
{
    if (i < 0 || i >= 16) fail(ZV_ERR_ARG, "lane %d out of range", i);
    while ((int)lanes_.size() <= i)
    {
        Lane l;
        ZV_HIP(hipStreamCreateWithFlags(&l.stream, hipStreamNonBlocking));
        lanes_.push_back(l);
    }
    cur_lane_ = i;
}

void Model::sync_all_lanes() { for (Lane &l : lanes_) ZV_HIP(hipStreamSynchronize(l.stream)); }

void Model::poison_lane(int i, int byte, size_t filled[3])
{
    filled[0] = filled[1] = filled[2] = 0;
    if (i < 0 || i >= (int)lanes_.size()) return;        // never selected: no stream, no blocks
    Lane &l = lanes_[i];
    ZV_HIP(hipStreamSynchronize(l.stream));
    if (l.copy_stream) ZV_HIP(hipStreamSynchronize(l.copy_stream));
    // on the lane's own stream, as arena_require's fill: the null stream is not ordered with the lane's kernels
    if (l.arena.base) ZV_HIP(hipMemsetAsync(l.arena.base, byte, l.arena.cap, l.stream));
    if (l.io) ZV_HIP(hipMemsetAsync(l.io, byte, l.io_cap, l.stream));
    ZV_HIP(hipStreamSynchronize(l.stream));
    if (l.pinned) memset(l.pinned, byte, l.pinned_cap);
    l.runs_tab = nullptr;                        // the last run table lay in the arena just overwritten (voc_runs_last)
    l.runs_n = 0;
    filled[0] = l.arena.base ? l.arena.cap : 0;
    filled[1] = l.io ? l.io_cap : 0;
    filled[2] = l.pinned ? l.pinned_cap : 0;
}

void *Model::pinned_scratch(size_t bytes)
{
    Lane &l = lane();
    if (bytes <= l.pinned_cap) return l.pinned;
    ZV_HIP(hipStreamSynchronize(l.stream));              // the block belongs to this lane: only its streams use it
    if (l.copy_stream) ZV_HIP(hipStreamSynchronize(l.copy_stream));
    drop_lane_graphs();                                  // a batch graph's first node uploads from this block
    if (l.pinned) hipHostFree(l.pinned);
    l.pinned = nullptr;
    l.pinned_cap = 0;
    if (hipHostMalloc(&l.pinned, bytes, hipHostMallocDefault) != hipSuccess) fail(ZV_ERR_OOM, "hipHostMalloc(%zu) failed", bytes);
    l.pinned_cap = bytes;
    return l.pinned;
}

void *Model::io_scratch(size_t bytes)
{
    Lane &l = lane();
    if (bytes <= l.io_cap) return l.io;
    ZV_HIP(hipStreamSynchronize(l.stream));
    drop_lane_graphs();                                  // the lane's graphs name the block about to be freed
    if (l.io) hipFree(l.io);
    l.io = nullptr;
    l.io_cap = 0;
    if (hipMalloc(&l.io, bytes) != hipSuccess) fail(ZV_ERR_OOM, "hipMalloc(%zu) for I/O scratch failed", bytes);
    l.io_cap = bytes;
    return l.io;
}

// activation arena

uint32_t Model::max_frames_per_utterance() const
{
    // buffer descriptors address a segment with 32-bit byte offsets: rows * channels * 4 < 2^31 at every stage
    // (rows * channels peaks at the first upsample stages: T * hop * C_last <= T * s0 * C0 / 2 ...)
    uint64_t worst = (uint64_t)round_up(hp.voc_channels, 16);
    uint64_t rate = 1, C = hp.voc_channels;
    for (uint32_t i = 0; i < hp.voc_num_upsamples; i++)
    {
        rate *= hp.voc_upsample_scales[i];
        C >>= 1;
        worst = std::max<uint64_t>(worst, rate * (uint64_t)round_up((int)C, 16));
    }
    worst = std::max<uint64_t>(worst, (uint64_t)(2 * E() + dec_.R));
    const uint64_t lim = ((uint64_t)1 << 31) / (4 * worst) - 64;
    return (uint32_t)std::min<uint64_t>(lim, 32768);
}

// the largest of the three stage layouts for b's capacities, measured by the carves themselves (model.h)
size_t Model::arena_bytes_for(const Batch &b) const
{
    DeviceArena v = DeviceArena::counter(), d = DeviceArena::counter(), e = DeviceArena::counter();
    voc_layout(v, b);
    dec_layout(d, b);
    enc_layout(e, b);
    return std::max(v.used, std::max(d.used, e.used)) + ARENA_TAIL;
}

DeviceArena &Model::stage_arena(const Batch &b) { reserve_batch(b); lane().arena.used = 0; return lane().arena; }

void Model::arena_require(size_t bytes)
{
    if (bytes <= lane().arena.cap) return;
    ZV_HIP(hipStreamSynchronize(stream()));
    // captured graphs hold pointers into the arena they were captured on, and only a lane's own graphs name its arena (model.h
    // graphs_): the lane's slots go, the other lanes keep theirs and are not waited for
    drop_lane_graphs();
    DeviceArena &ar = lane().arena;
    if (ar.base) hipFree(ar.base);
    ar = DeviceArena();
    lane().runs_tab = nullptr;                   // the last run table lay in the arena just freed (voc_runs_last)
    lane().runs_n = 0;
    void *p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) fail(ZV_ERR_OOM, "hipMalloc(%zu) for the activation arena failed", bytes);
    // on the lane's own stream: the streams are non-blocking, so a memset on the null stream is NOT ordered with the
    // kernels that follow on the lane's and could zero an arena they have already started to fill
    // ZV_ARENA_FILL=255 fills it with NaN patterns instead: no kernel may depend on what a fresh arena holds (test hook)
    const int fill = knob(ZV_ARENA_FILL);
    ZV_HIP(hipMemsetAsync(p, fill, bytes, stream()));
    ar = DeviceArena{(char *)p, bytes, 0};
}

void Model::reserve(uint32_t max_phonemes, uint32_t max_frames) { reserve_batch(Batch::single(std::max(1u, max_phonemes), std::max(1u, max_frames), 1)); }

void Model::reserve_batch(const Batch &b) { arena_require(arena_bytes_for(b)); }

// launch helpers

void Model::prof_clear()
{
    for (auto &p : prof)
    {
        hipEventDestroy(p.e0);
        hipEventDestroy(p.e1);
    }
    prof.clear();
}

void Model::tick(hipEvent_t *e0)
{
    *e0 = nullptr;
    if (!profiling || in_group_) return;
    ZV_HIP(hipEventCreate(e0));
    ZV_HIP(hipEventRecord(*e0, stream()));
}

void Model::tock(hipEvent_t e0, const char *name, double bytes, double flops)
{
    if (!profiling) return;
    if (in_group_)
    {
        group_bytes_ += bytes;
        group_flops_ += flops;
        group_n_++;
        return;
    }
    hipEvent_t e1;
    ZV_HIP(hipEventCreate(&e1));
    ZV_HIP(hipEventRecord(e1, stream()));
    prof.push_back({name, e0, e1, bytes, flops, group_n_ > 0 ? group_n_ : 1});
}

// the ResBlock launches of one stage run back to back: one event pair brackets the whole run so that the per-launch
// average is not inflated by ~2 us of event-record overhead per launch
void Model::group_begin()
{
    if (!profiling) return;
    ZV_HIP(hipEventCreate(&group_e0_));
    ZV_HIP(hipEventRecord(group_e0_, stream()));
    in_group_ = true;
    group_bytes_ = group_flops_ = 0.0;
    group_n_ = 0;
}

void Model::group_end(const char *name)
{
    if (!profiling || !in_group_) return;
    in_group_ = false;
    tock(group_e0_, name, group_bytes_, group_flops_);
    group_n_ = 0;
}

ConvJob Model::job(const ConvW &w) const
{
    ConvJob j;
    memset(&j, 0, sizeof(j));
    j.Cin_p = w.Cin_p;
    j.Cout_p = w.Cout_p;
    j.K = w.K;
    j.dil = 1;
    j.pad = (w.K - 1) / 2;
    j.ck = w.ck;
    j.w = w.w;
    j.w8 = w.w8;
    j.bias = w.bias;
    j.pro = PRO_ACT;
    j.slope = 1.0f;
    j.pscale = 1.0f;
    j.escale = 1.0f;
    j.ldx = w.Cin_p;
    j.ldo = w.Cout_p;
    return j;
}

void Model::dbg_inject(void *dev, int ld, int cols, size_t rows)
{
    ZV_HIP(hipMemcpy2DAsync(dev, (size_t)ld * 4, dbg_layer.x, (size_t)cols * 4, (size_t)cols * 4, rows, hipMemcpyHostToDevice, stream()));
}

void Model::dbg_extract(const void *dev, int ld, int cols, size_t rows)
{
    ZV_HIP(hipMemcpy2DAsync(dbg_layer.out, (size_t)cols * 4, dev, (size_t)ld * 4, (size_t)cols * 4, rows, hipMemcpyDeviceToHost, stream()));
    ZV_HIP(hipStreamSynchronize(stream()));
    dbg_layer.done = true;
}

void Model::conv(const ConvJob *jobs, int n, const Segs &segs, int rate, const char *name, double bytes, double flops)
{
    ZV_LAUNCH(name, bytes, flops, launch_conv(stream(), jobs, n, n_cu, segs, rate));
}

// ---- the graph cache: graph_cache.h decides, this part owns the execs ----
// No exec is destroyed with work of its own in flight, and no lane is synchronised to evict a graph.

static void destroy_retired(hipGraphExec_t exec, hipEvent_t done)
{
    if (exec) hipGraphExecDestroy(exec);
    if (done) hipEventDestroy(done);
}

void Model::drop_graphs()
{
    sync_all_lanes();                            // an exec of another lane may still be running
    graphs_.drop_all([](CapturedGraph &&g, int) { destroy_retired(g.exec, nullptr); });
    retired_.clear([](RetiredExec &&r) { destroy_retired(r.exec, r.done); });
}

void Model::drop_lane_graphs()
{
    graphs_.drop_lane(cur_lane_, [](CapturedGraph &&g, int) { destroy_retired(g.exec, nullptr); });
}

void Model::sweep_retired()
{
    retired_.sweep([](const RetiredExec &r) { return hipEventQuery(r.done) == hipSuccess; },
                   [](RetiredExec &&r) { destroy_retired(r.exec, r.done); });
    (void)hipGetLastError();                     // "not ready" is an answer, not an error for the next launch to report
}

// The slot has left the cache.  Everything its lane's stream was given so far, the exec's last replay included, lies ahead of an event
// recorded on that stream now: the exec goes when the event has completed (sweep_retired), or at once where the stream is already idle.
void Model::retire_graph(CapturedGraph &&g, int lane)
{
    hipStream_t s = lanes_[(size_t)lane].stream;
    const hipError_t idle = hipStreamQuery(s);
    (void)hipGetLastError();
    if (idle == hipSuccess) return destroy_retired(g.exec, nullptr);
    hipEvent_t done = nullptr;
    if (hipEventCreateWithFlags(&done, hipEventDisableTiming) != hipSuccess || hipEventRecord(done, s) != hipSuccess)
    {
        hipStreamSynchronize(s);                 // no event to be had: the one stream the exec ran on, then the exec
        return destroy_retired(g.exec, done);
    }
    // bounded by the cache's capacity: a full list waits for its oldest event alone
    retired_.push(RetiredExec{g.exec, done}, graphs_.capacity(), [](const RetiredExec &r) { hipEventSynchronize(r.done); },
                  [](RetiredExec &&r) { destroy_retired(r.exec, r.done); });
}

bool Model::set_graph_cache(uint64_t capacity)
{
    if (!graph_capacity_ok(capacity)) return false;
    sweep_retired();
    return graphs_.set_capacity(capacity, knob_epoch(), [this](CapturedGraph &&g, int lane) { retire_graph(std::move(g), lane); });
}

void Model::graph_stats(zv_graph_stats *out) const
{
    const GraphCounters &n = graphs_.counters();
    memset(out, 0, sizeof(*out));
    out->capacity = graphs_.capacity();
    out->entries = (uint32_t)graphs_.entries();
    out->retired = (uint32_t)retired_.size();
    out->lookups = n.lookups;
    out->hits = n.hits;
    out->captures = n.captures;
    out->evictions = n.evictions;
    out->stale_evictions = n.stale_evictions;
    out->lane_drops = n.lane_drops;
    out->full_drops = n.full_drops;
}

// the hash of a graph's key: every field the full comparison reads (run_captured), field by field (a Batch has padding).  A keyed
// field that is missing here costs a collision, which the full comparison settles; a field hashed but not keyed would cost hits
static uint64_t graph_key_hash(int kind, int lane, unsigned epoch, const Batch &b, const void *const *key, size_t key_bytes)
{
    uint64_t h = GRAPH_HASH_SEED;
    auto add = [&h](const auto &v) { h = graph_hash(h, &v, sizeof(v)); };
    add(kind), add(lane), add(epoch);
    add(b.nseg), add(b.n_max), add(b.t_max), add(b.n_rows), add(b.t_rows), add(b.d_tok), add(b.d_frm);
    if (!b.d_tok) add(b.tok1);
    if (!b.d_frm) add(b.frm1);
    add(b.d_ctl), add(b.d_pctl), add(b.d_cum), add(b.d_frm_live), add(b.has_targets), add(b.d_dec_runs), add(b.wave);
    return graph_hash(h, key, key_bytes);
}

// Replays the captured schedule for (kind, capacities, buffers) or captures it first.  The capacities decide grids and
// arena layout; the segment tables are read by the kernels at run time, so a batch graph does not depend on the
// utterances' lengths.  A replay is a hash, a scan of the slots and a launch: no event, no wait, no allocation.
template <typename F> void Model::run_captured(int kind, const Batch &b, const void *const (&key)[CapturedGraph::NKEY], F &&enqueue)
{
    const unsigned epoch = knob_epoch();
    const int      ln = cur_lane_;
    const uint64_t hash = graph_key_hash(kind, ln, epoch, b, key, sizeof(key));
    const int at = graphs_.find(hash, [&](const CapturedGraph &g) {
        return g.kind == kind && g.lane == ln && g.epoch == epoch && b.same_schedule(g.b) && memcmp(g.p, key, sizeof(key)) == 0;
    });
    if (at >= 0)
    {
        const CapturedGraph &g = graphs_.hit(at);
        ZV_HIP(hipGraphLaunch(g.exec, stream()));
        lane().runs_tab = g.runs_tab;
        lane().runs_n = g.runs_n;
        return;
    }
    sweep_retired();
    reserve_batch(b);                            // hipMalloc is not capturable
    hipGraph_t graph = nullptr;
    lane().runs_tab = nullptr;
    lane().runs_n = 0;
    ZV_HIP(hipStreamBeginCapture(stream(), hipStreamCaptureModeThreadLocal));
    try
    {
        enqueue();
    }
    catch (...)
    {
        hipStreamEndCapture(stream(), &graph);
        if (graph) hipGraphDestroy(graph);
        throw;
    }
    ZV_HIP(hipStreamEndCapture(stream(), &graph));
    CapturedGraph cg;
    cg.kind = kind;
    cg.lane = ln;
    cg.epoch = epoch;              // a graph replays the kernel regime it was captured in: a later zv_debug_set captures anew
    cg.b = b;
    memcpy(cg.p, key, sizeof(key));
    cg.runs_tab = lane().runs_tab;
    cg.runs_n = lane().runs_n;
    hipError_t e = hipGraphInstantiate(&cg.exec, graph, nullptr, nullptr, 0);
    hipGraphDestroy(graph);
    if (e != hipSuccess) fail(ZV_ERR_DEVICE, "hipGraphInstantiate failed: %s", hipGetErrorString(e));
    hipGraphExec_t exec = cg.exec;
    // a full cache gives up exactly one slot (graph_cache.h victim), whose exec may still be running on its own lane
    graphs_.insert(hash, epoch, ln, std::move(cg), [this](CapturedGraph &&g, int lane) { retire_graph(std::move(g), lane); });
    ZV_HIP(hipGraphLaunch(exec, stream()));
}

void Model::chain_dev(const Batch &b, const int32_t *d_ids, const int32_t *d_puncts, const float *d_styles, float *d_hidden,
                      float *d_mel, float *d_wav, int32_t *d_nframes, const void *h2d_src, void *h2d_dst, size_t h2d_bytes, int voc_part,
                      StageRange range)
{
    auto run = [&]() {
        if (h2d_bytes) ZV_HIP(hipMemcpyAsync(h2d_dst, h2d_src, h2d_bytes, hipMemcpyHostToDevice, stream()));
        if (range.has(ST_ENCODER)) encode_dev(b, d_ids, d_puncts, d_styles, d_hidden, d_nframes);
        if (range.has(ST_DECODER)) decode_dev(b, d_hidden, d_styles, d_mel);        // the reference vocodes all T frames (src/zerovox.cpp:326-334)
        if (!range.has(ST_VOCODER)) return;
        if (voc_part == 1) vocode_group(b, d_mel, d_wav, 1);      // the caller runs the last stage in utterance groups
        else vocode_dev(b, d_mel, d_wav);
    };
    if (!graph_mode || profiling) return run();
    // the buffers that are not part of the Batch (what of the Batch keys a graph: Batch::same_schedule)
    const void *key[CapturedGraph::NKEY] = {d_ids, d_puncts, d_styles, d_hidden, d_mel, d_wav, d_nframes, h2d_src};
    // the stage range is part of the kind: the chain keeps 1 and 2, a stage batch's graphs are 4 * range.key() above them
    run_captured((voc_part == 1 ? 2 : 1) + 4 * range.key(), b, key, run);
}

void Model::vocode_dev_graph(const Batch &b, const float *d_mel, float *d_wav)
{
    if (!graph_mode || profiling) return vocode_dev(b, d_mel, d_wav);
    const void *key[CapturedGraph::NKEY] = {d_mel, d_wav};
    run_captured(0, b, key, [&]() { vocode_dev(b, d_mel, d_wav); });
}

}  // namespace zv
