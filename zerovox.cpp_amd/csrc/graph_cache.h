// graph_cache.h — the policy of the captured-graph cache (DESIGN.md "Serving under changing shapes"): which slot a call hits, which
// slot goes when the cache is full, what a lane's regrow removes, what a capacity change evicts, when a retired exec may be
// destroyed, and the arithmetic of the counters of zv_graph_cache_stats.  Pure host code: no HIP, no Model, no device pointer is
// dereferenced.  The cache stores a payload P per slot (model.cpp: the CapturedGraph with its exec) and the retire list an R per
// entry (model.cpp: exec + event); what "same key", "ready", "wait" and "destroy" mean is handed in by the caller.  Shared by
// Model::run_captured and the host-side test (tests/native/graph_cache_check.cpp), which replays it against a written-out model.
#pragma once

#include <cstddef>
#include <cstdint>
#include <deque>
#include <utility>
#include <vector>

namespace zv
{

constexpr uint32_t GRAPH_CACHE_DEFAULT = 16, GRAPH_CACHE_MIN = 1, GRAPH_CACHE_MAX = 1024;

inline bool graph_capacity_ok(uint64_t capacity) { return capacity >= GRAPH_CACHE_MIN && capacity <= GRAPH_CACHE_MAX; }

// FNV-1a over the bytes of a key's fields, chained: h = graph_hash(h, &field, sizeof(field)).  A hit is never decided by it alone.
constexpr uint64_t GRAPH_HASH_SEED = 1469598103934665603ull;
inline uint64_t graph_hash(uint64_t h, const void *p, size_t n)
{
    const unsigned char *c = (const unsigned char *)p;
    for (size_t i = 0; i < n; i++) h = (h ^ c[i]) * 1099511628211ull;
    return h;
}

// what the policy knows of a slot
struct GraphSlot
{
    uint64_t hash = 0;      // of the whole key (kind, lane, epoch, Batch::same_schedule's fields, the buffers)
    uint64_t tick = 0;      // last use: the cache's counter at the capture or the most recent hit
    unsigned epoch = 0;     // knob epoch at capture: a slot of another epoch than the current one can never hit again
    int      lane = 0;      // the lane that captured it, the only one that replays it
};

// include/zerovox_amd.h zv_graph_stats without `capacity`, `entries` and `retired`, which the containers hold.  Invariants, after
// every operation: lookups = hits + captures, captures = entries + evictions + stale_evictions + lane_drops + full_drops.
struct GraphCounters
{
    uint64_t lookups = 0, hits = 0, captures = 0, evictions = 0, stale_evictions = 0;
    uint64_t lane_drops = 0, full_drops = 0;      // SLOTS removed by lane drops / full drops, not the drops
};

template <typename P> class GraphCache
{
  public:
    uint32_t capacity() const { return capacity_; }
    size_t   entries() const { return slots_.size(); }
    const GraphCounters &counters() const { return n_; }
    const GraphSlot &slot(size_t i) const { return slots_[i]; }
    const P &item(size_t i) const { return items_[i]; }

    // the slot of this key or -1: by hash first, then confirmed by same(item) — the caller's full comparison
    template <typename Same> int find(uint64_t hash, Same &&same) const
    {
        for (size_t i = 0; i < slots_.size(); i++)
            if (slots_[i].hash == hash && same(items_[i])) return (int)i;
        return -1;
    }
    // a call that found slot i: counts it and makes the slot the most recently used.  Never changes the slot set.
    const P &hit(int i)
    {
        n_.lookups++;
        n_.hits++;
        slots_[(size_t)i].tick = ++tick_;
        return items_[(size_t)i];
    }
    bool full() const { return slots_.size() >= capacity_; }
    // the slot that goes when one must: of the slots of another epoch than `epoch` the least recently used, else of all slots the
    // least recently used; -1 for an empty cache
    int victim(unsigned epoch) const
    {
        int best = -1;
        bool best_stale = false;
        for (size_t i = 0; i < slots_.size(); i++)
        {
            const bool stale = slots_[i].epoch != epoch;
            if (best < 0 || (stale && !best_stale) || (stale == best_stale && slots_[i].tick < slots_[(size_t)best].tick))
            {
                best = (int)i;
                best_stale = stale;
            }
        }
        return best;
    }
    // removes the victim and hands its payload to out(P &&, lane); the cache must not be empty
    template <typename Out> void evict(unsigned epoch, Out &&out)
    {
        const int v = victim(epoch);
        if (slots_[(size_t)v].epoch != epoch) n_.stale_evictions++;
        else n_.evictions++;
        remove((size_t)v, out);
    }
    // a call that missed and captured: evicts exactly one slot when the cache is full, then holds the new one as the most recent
    template <typename Out> void insert(uint64_t hash, unsigned epoch, int lane, P &&item, Out &&out)
    {
        if (full()) evict(epoch, out);
        n_.lookups++;
        n_.captures++;
        GraphSlot s;
        s.hash = hash;
        s.tick = ++tick_;
        s.epoch = epoch;
        s.lane = lane;
        slots_.push_back(s);
        items_.push_back(std::move(item));
    }
    // removes exactly the slots of `lane` (its arena or one of its blocks is about to be freed)
    template <typename Out> size_t drop_lane(int lane, Out &&out)
    {
        size_t k = 0;
        for (size_t i = slots_.size(); i-- > 0;)
            if (slots_[i].lane == lane)
            {
                remove(i, out);
                k++;
            }
        n_.lane_drops += k;
        return k;
    }
    // removes every slot (teardown)
    template <typename Out> size_t drop_all(Out &&out)
    {
        const size_t k = slots_.size();
        while (!slots_.empty()) remove(slots_.size() - 1, out);
        n_.full_drops += k;
        return k;
    }
    // shrinking evicts by the victim rule until the cache fits; false (and nothing changes) for a capacity out of range
    template <typename Out> bool set_capacity(uint64_t capacity, unsigned epoch, Out &&out)
    {
        if (!graph_capacity_ok(capacity)) return false;
        capacity_ = (uint32_t)capacity;
        while (slots_.size() > capacity_) evict(epoch, out);
        return true;
    }

  private:
    template <typename Out> void remove(size_t i, Out &&out)
    {
        P   gone = std::move(items_[i]);
        int lane = slots_[i].lane;
        if (i + 1 != slots_.size())
        {
            slots_[i] = slots_.back();
            items_[i] = std::move(items_.back());
        }
        slots_.pop_back();
        items_.pop_back();
        out(std::move(gone), lane);
    }
    uint32_t               capacity_ = GRAPH_CACHE_DEFAULT;
    uint64_t               tick_ = 0;
    GraphCounters          n_;
    std::vector<GraphSlot> slots_;       // scanned by find: 24 bytes a slot, the payloads apart
    std::vector<P>         items_;
};

// Execs that have left the cache and wait for their last replay to finish.  ready(R): the entry's event has completed (a query,
// never a wait); wait(R): blocks on that one event; destroy(R &&): frees the exec and the event.  Never longer than `bound`.
template <typename R> class RetireList
{
  public:
    size_t size() const { return list_.size(); }
    // destroys every entry that is ready, in any position (the lanes finish in any order)
    template <typename Ready, typename Destroy> size_t sweep(Ready &&ready, Destroy &&destroy)
    {
        size_t k = 0;
        for (size_t i = 0; i < list_.size();)
            if (ready(list_[i]))
            {
                destroy(std::move(list_[i]));
                list_.erase(list_.begin() + (std::ptrdiff_t)i);
                k++;
            }
            else i++;
        return k;
    }
    // appends r; while the list holds `bound` entries or more, waits for its OLDEST alone and destroys it first
    template <typename Wait, typename Destroy> void push(R &&r, size_t bound, Wait &&wait, Destroy &&destroy)
    {
        if (bound < 1) bound = 1;
        while (list_.size() >= bound)
        {
            wait(list_.front());
            destroy(std::move(list_.front()));
            list_.pop_front();
        }
        list_.push_back(std::move(r));
    }
    // teardown, everything has been waited for: destroys all
    template <typename Destroy> void clear(Destroy &&destroy)
    {
        for (R &r : list_) destroy(std::move(r));
        list_.clear();
    }

  private:
    std::deque<R> list_;
};

}  // namespace zv
