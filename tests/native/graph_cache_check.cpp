// graph_cache_check.cpp — csrc/graph_cache.h against a written-out model of the policy (tests/test_graph_cache_cpu.py builds and runs
// it, once more under -fsanitize=address,undefined).  A seeded stream of operations — lookup (hit or capture), epoch bump, lane drop,
// capacity change, sweep of the retire list, full drop — runs through GraphCache / RetireList and through the model below, which
// states the rules the slow way: plain vectors, a sort for the victim.  After every step the two must agree.
//
//   graph_cache_check cases     prints "ok <checks>" and exits 0, or "FAILED <what>" lines and exits 1
//   graph_cache_check lookup    prints the host time of a lookup at 1 024 slots, hit and miss
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <ctime>
#include <deque>
#include <set>
#include <tuple>
#include <vector>

#include "graph_cache.h"

using namespace zv;

static long g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                                   \
    do                                                     \
    {                                                      \
        g_checks++;                                        \
        if (!(cond))                                       \
        {                                                  \
            if (g_failed++ < 20)                           \
            {                                              \
                printf("FAILED %s:%d: ", __FILE__, __LINE__); \
                printf(__VA_ARGS__);                       \
                printf("\n");                              \
            }                                              \
        }                                                  \
    } while (0)

// a key as run_captured sees it: what the call is (shape), the lane and the epoch.  The hash keeps 3 bits of the shape alone, so keys
// that differ in shape, lane or epoch collide all the time and only the full comparison tells them apart.
struct Key
{
    int      shape, lane;
    unsigned epoch;
    bool operator==(const Key &o) const { return shape == o.shape && lane == o.lane && epoch == o.epoch; }
    bool operator<(const Key &o) const { return std::tie(shape, lane, epoch) < std::tie(o.shape, o.lane, o.epoch); }
    uint64_t hash() const { return (uint64_t)(shape & 7); }
};
struct Payload { Key key; int exec; };                  // exec: a serial number, "destroyed" exactly once
struct Retired { int exec; long done_at; };              // the event completes at time done_at

struct Rng
{
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    int below(int n) { return (int)(next() % (uint32_t)n); }
};

// ---- the model ----
struct MSlot { Key key; uint64_t tick; };
struct ModelCache
{
    uint32_t capacity = 16;
    uint64_t tick = 0;
    std::vector<MSlot> slots;
    uint64_t lookups = 0, hits = 0, captures = 0, evictions = 0, stale = 0, lane_drops = 0, full_drops = 0;

    int find(const Key &k) const
    {
        for (size_t i = 0; i < slots.size(); i++)
            if (slots[i].key == k) return (int)i;
        return -1;
    }
    // stale slots first, then by last use: the front of the sorted order
    Key take_victim(unsigned epoch)
    {
        std::vector<std::tuple<int, uint64_t, size_t>> order;
        for (size_t i = 0; i < slots.size(); i++) order.emplace_back(slots[i].key.epoch != epoch ? 0 : 1, slots[i].tick, i);
        std::sort(order.begin(), order.end());
        const size_t at = std::get<2>(order[0]);
        const Key k = slots[at].key;
        (std::get<0>(order[0]) == 0 ? stale : evictions)++;
        slots.erase(slots.begin() + (std::ptrdiff_t)at);
        return k;
    }
};

struct Run
{
    GraphCache<Payload> cache;
    RetireList<Retired> retire;
    ModelCache          model;
    std::deque<Retired> mretire;
    Rng                 rng{1};
    unsigned            epoch = 0;
    long                now = 0;
    int                 next_exec = 0;
    std::set<int>       live_execs, destroyed;
    std::vector<Key>    evicted;          // what the cache handed out during the current operation
    long                collisions = 0, waits = 0, swept = 0;

    void destroy(int exec, long done_at)
    {
        CHECK(done_at <= now, "exec %d destroyed at %ld with its lane only passing it at %ld", exec, now, done_at);
        CHECK(live_execs.erase(exec) == 1, "exec %d destroyed but not alive", exec);
        CHECK(destroyed.insert(exec).second, "exec %d destroyed twice", exec);
    }
    // an evicted slot: its lane may still be replaying it
    void retire_out(Payload &&p, int lane)
    {
        CHECK(lane == p.key.lane, "payload of lane %d handed out as lane %d", p.key.lane, lane);
        evicted.push_back(p.key);
        Retired r{p.exec, now + rng.below(24)};
        const size_t bound = cache.capacity();
        // model: the oldest alone is waited for, and only while the list is full; a wait lasts until that event completes
        long expect_now = now;
        while (mretire.size() >= bound)
        {
            expect_now = std::max(expect_now, mretire.front().done_at);
            mretire.pop_front();
        }
        mretire.push_back(r);
        retire.push(std::move(r), bound, [&](const Retired &x) { waits++; now = std::max(now, x.done_at); },
                    [&](Retired &&x) { destroy(x.exec, x.done_at); });
        CHECK(now == expect_now, "retire: waited until %ld, the oldest entries alone last until %ld", now, expect_now);
        CHECK(retire.size() <= bound, "retire list %zu over its bound %zu", retire.size(), bound);
        CHECK(retire.size() == mretire.size(), "retire list %zu, model %zu", retire.size(), mretire.size());
    }
    // a dropped slot: its lane has just been synchronised
    void direct_out(Payload &&p, int lane)
    {
        CHECK(lane == p.key.lane, "payload of lane %d handed out as lane %d", p.key.lane, lane);
        evicted.push_back(p.key);
        destroy(p.exec, now);
    }

    void compare(const char *what)
    {
        const GraphCounters &n = cache.counters();
        CHECK(cache.entries() == model.slots.size(), "%s: %zu entries, model %zu", what, cache.entries(), model.slots.size());
        CHECK(cache.entries() <= cache.capacity(), "%s: %zu entries over capacity %u", what, cache.entries(), cache.capacity());
        CHECK(cache.capacity() == model.capacity, "%s: capacity %u, model %u", what, cache.capacity(), model.capacity);
        std::vector<std::tuple<Key, uint64_t>> a, b;
        for (size_t i = 0; i < cache.entries(); i++)
        {
            const GraphSlot &s = cache.slot(i);
            const Key &k = cache.item(i).key;
            CHECK(s.lane == k.lane && s.epoch == k.epoch && s.hash == k.hash(), "%s: slot %zu does not describe its payload", what, i);
            a.emplace_back(k, s.tick);
        }
        for (const MSlot &s : model.slots) b.emplace_back(s.key, s.tick);
        std::sort(a.begin(), a.end());
        std::sort(b.begin(), b.end());
        CHECK(a == b, "%s: the slot sets differ", what);
        CHECK(n.lookups == n.hits + n.captures, "%s: lookups %llu != hits %llu + captures %llu", what, (unsigned long long)n.lookups,
              (unsigned long long)n.hits, (unsigned long long)n.captures);
        CHECK(n.captures == cache.entries() + n.evictions + n.stale_evictions + n.lane_drops + n.full_drops, "%s: captures %llu do not add up", what,
              (unsigned long long)n.captures);
        CHECK(n.lookups == model.lookups && n.hits == model.hits && n.captures == model.captures && n.evictions == model.evictions &&
                  n.stale_evictions == model.stale && n.lane_drops == model.lane_drops && n.full_drops == model.full_drops,
              "%s: the counters differ from the model's", what);
        CHECK(live_execs.size() == cache.entries() + retire.size(), "%s: %zu execs alive, %zu held + %zu retired", what, live_execs.size(),
              cache.entries(), retire.size());
    }

    void lookup()
    {
        const Key k{rng.below(40), rng.below(3), epoch};
        // another key with this hash in the cache?  Then only the full comparison keeps it from being replayed
        bool collides = false;
        for (size_t i = 0; i < cache.entries(); i++) collides |= cache.slot(i).hash == k.hash() && !(cache.item(i).key == k);
        collisions += collides;
        const int at = cache.find(k.hash(), [&](const Payload &p) { return p.key == k; });
        const int mat = model.find(k);
        CHECK((at >= 0) == (mat >= 0), "lookup: cache says %d, model %d", at, mat);
        if (at >= 0) CHECK(cache.item((size_t)at).key == k, "lookup: a colliding hash replayed another key");
        evicted.clear();
        if (at >= 0 && mat >= 0)
        {
            std::vector<Key> before, after;
            for (size_t i = 0; i < cache.entries(); i++) before.push_back(cache.item(i).key);
            const Payload &p = cache.hit(at);
            CHECK(p.key == k, "hit: the payload of another key");
            for (size_t i = 0; i < cache.entries(); i++) after.push_back(cache.item(i).key);
            CHECK(before == after, "hit: the slot set changed");
            model.slots[(size_t)mat].tick = ++model.tick;
            model.lookups++, model.hits++;
            return compare("hit");
        }
        if (at >= 0 || mat >= 0) return;
        // a capture: the model first
        bool had_stale = false;
        for (const MSlot &s : model.slots) had_stale |= s.key.epoch != epoch;
        std::vector<Key> mvictims;
        if (model.slots.size() >= model.capacity) mvictims.push_back(model.take_victim(epoch));
        model.slots.push_back(MSlot{k, ++model.tick});
        model.lookups++, model.captures++;
        const int v = cache.full() ? cache.victim(epoch) : -1;
        const Key announced = v >= 0 ? cache.item((size_t)v).key : Key{-1, -1, 0};
        live_execs.insert(next_exec);
        cache.insert(k.hash(), epoch, k.lane, Payload{k, next_exec++}, [&](Payload &&p, int lane) { retire_out(std::move(p), lane); });
        CHECK(evicted.size() == mvictims.size() && evicted.size() <= 1, "capture: %zu slots went, model %zu", evicted.size(), mvictims.size());
        if (evicted.size() == 1 && mvictims.size() == 1)
        {
            CHECK(evicted[0] == mvictims[0], "capture: victim (%d, %d, %u), model (%d, %d, %u)", evicted[0].shape, evicted[0].lane, evicted[0].epoch,
                  mvictims[0].shape, mvictims[0].lane, mvictims[0].epoch);
            CHECK(evicted[0] == announced, "capture: victim() named another slot than the one that went");
            CHECK(!had_stale || evicted[0].epoch != epoch, "capture: a live slot went while a stale one was held");
        }
        compare("capture");
    }

    void lane_drop()
    {
        const int lane = rng.below(3);
        size_t expect = 0;
        for (size_t i = model.slots.size(); i-- > 0;)
            if (model.slots[i].key.lane == lane)
            {
                model.slots.erase(model.slots.begin() + (std::ptrdiff_t)i);
                expect++;
            }
        model.lane_drops += expect;
        evicted.clear();
        const size_t k = cache.drop_lane(lane, [&](Payload &&p, int l) { direct_out(std::move(p), l); });
        CHECK(k == expect && evicted.size() == expect, "lane drop: %zu slots went, model %zu", k, expect);
        for (const Key &e : evicted) CHECK(e.lane == lane, "lane drop of %d removed a slot of lane %d", lane, e.lane);
        compare("lane drop");
    }

    void set_capacity()
    {
        static const uint64_t asks[] = {1, 2, 3, 5, 8, 16, 16, 24, 64, 1024, 0, 1025, 70000, (uint64_t)1 << 32};
        const uint64_t c = asks[rng.below((int)(sizeof(asks) / sizeof(asks[0])))];
        std::vector<Key> mvictims;
        const bool ok = c >= 1 && c <= 1024;
        if (ok)
        {
            model.capacity = (uint32_t)c;
            while (model.slots.size() > model.capacity) mvictims.push_back(model.take_victim(epoch));
        }
        evicted.clear();
        const bool got = cache.set_capacity(c, epoch, [&](Payload &&p, int lane) { retire_out(std::move(p), lane); });
        CHECK(got == ok && graph_capacity_ok(c) == ok, "capacity %llu: accepted %d, expected %d", (unsigned long long)c, (int)got, (int)ok);
        CHECK(evicted == mvictims, "capacity %llu: other victims (or another order) than the model's", (unsigned long long)c);
        // the retire list's bound follows the capacity at the next push only: it never waits here for more than it pushed
        compare("capacity");
    }

    void sweep()
    {
        now += rng.below(12);
        size_t expect = 0;
        for (size_t i = 0; i < mretire.size();)
            if (mretire[i].done_at <= now)
            {
                mretire.erase(mretire.begin() + (std::ptrdiff_t)i);
                expect++;
            }
            else i++;
        const size_t k = retire.sweep([&](const Retired &r) { return r.done_at <= now; }, [&](Retired &&r) { destroy(r.exec, r.done_at); });
        swept += (long)k;
        CHECK(k == expect && retire.size() == mretire.size(), "sweep: %zu destroyed, model %zu", k, expect);
        compare("sweep");
    }

    void full_drop()
    {
        // drop_graphs: every lane synchronised first, so everything has finished
        for (const Retired &r : mretire) now = std::max(now, r.done_at);
        model.full_drops += model.slots.size();
        model.slots.clear();
        mretire.clear();
        cache.drop_all([&](Payload &&p, int l) { direct_out(std::move(p), l); });
        retire.clear([&](Retired &&r) { destroy(r.exec, r.done_at); });
        CHECK(cache.entries() == 0 && retire.size() == 0 && live_execs.empty(), "full drop left %zu + %zu, %zu execs alive", cache.entries(),
              retire.size(), live_execs.size());
        compare("full drop");
    }

    void run(uint64_t seed, int steps)
    {
        rng.s = seed;
        for (int i = 0; i < steps && g_failed == 0; i++)
        {
            const int op = rng.below(100);
            if (op < 70) lookup();
            // (the library's epoch only grows, so there a stale slot is also an old one; here it comes back to earlier values, as a
            // counter that wraps would, so that "stale first" and "least recent first" name different slots)
            else if (op < 78) { epoch = (epoch + 1 + (unsigned)rng.below(3)) % 4; compare("epoch"); }
            else if (op < 84) lane_drop();
            else if (op < 90) set_capacity();
            else if (op < 99) sweep();
            else full_drop();
        }
        full_drop();
        CHECK((int)destroyed.size() == next_exec, "%zu of %d execs destroyed at the end", destroyed.size(), next_exec);
    }
};

static void fixed_cases()
{
    // the default, the limits, the hash
    GraphCache<Payload> c;
    CHECK(c.capacity() == 16 && c.entries() == 0 && c.victim(0) == -1, "a fresh cache");
    CHECK(!graph_capacity_ok(0) && graph_capacity_ok(1) && graph_capacity_ok(1024) && !graph_capacity_ok(1025), "capacity limits");
    const int a = 1, b = 2;
    CHECK(graph_hash(GRAPH_HASH_SEED, &a, sizeof(a)) != graph_hash(GRAPH_HASH_SEED, &b, sizeof(b)), "graph_hash tells 1 from 2");
    CHECK(graph_hash(graph_hash(GRAPH_HASH_SEED, &a, 4), &b, 4) != graph_hash(graph_hash(GRAPH_HASH_SEED, &b, 4), &a, 4), "graph_hash sees the order");
    // the 17th graph evicts one graph, the least recently used, not all
    std::vector<int> gone;
    auto out = [&](Payload &&p, int) { gone.push_back(p.key.shape); };
    for (int i = 0; i < 16; i++) c.insert((uint64_t)i, 0, 0, Payload{Key{i, 0, 0}, i}, out);
    c.hit(c.find(0, [](const Payload &p) { return p.key.shape == 0; }));
    c.insert(16, 0, 0, Payload{Key{16, 0, 0}, 16}, out);
    CHECK(c.entries() == 16 && gone == std::vector<int>{1}, "the 17th graph evicts the least recently used alone");
    // a stale slot goes before an older live one
    gone.clear();
    c.insert(17, 1, 0, Payload{Key{17, 0, 1}, 17}, out);      // epoch 1: all sixteen held are stale, shape 2 the oldest of them
    c.insert(18, 1, 0, Payload{Key{18, 0, 1}, 18}, out);
    CHECK(gone == (std::vector<int>{2, 3}) && c.counters().stale_evictions == 2 && c.counters().evictions == 1, "stale slots go first, oldest first");
    CHECK(c.set_capacity(2, 1, out) && c.entries() == 2, "shrinking to 2");
    std::set<int> left{c.item(0).key.shape, c.item(1).key.shape};
    CHECK(left == (std::set<int>{17, 18}), "shrinking keeps the live, most recently used slots");
}

// `lookup`: the host time of what a call adds ahead of its launch at 1 024 slots — the hash of a key as long as the library's
// (about 300 bytes) and the scan — for a key held in the last slot (hit) and for one not held (miss).  A measurement, not a check.
static int lookup_times()
{
    struct Big { unsigned char key[304]; void *exec; };
    GraphCache<Big> c;
    c.set_capacity(1024, 0, [](Big &&, int) {});
    auto key_of = [](int i) { Big b{}; for (size_t k = 0; k < sizeof(b.key); k++) b.key[k] = (unsigned char)(i * 131 + (int)k * 7 + (i >> 8)); return b; };
    for (int i = 0; i < 1024; i++)
    {
        Big b = key_of(i);
        c.insert(graph_hash(GRAPH_HASH_SEED, b.key, sizeof(b.key)), 0, 0, std::move(b), [](Big &&, int) {});
    }
    const int reps = 20000;
    for (int which = 0; which < 2; which++)
    {
        const Big probe = key_of(which == 0 ? 1023 : 5000);
        long found = 0;
        timespec t0, t1;
        clock_gettime(CLOCK_MONOTONIC, &t0);
        for (int r = 0; r < reps; r++)
        {
            volatile unsigned char salt = probe.key[r % 304];      // keeps the loop's work from being hoisted
            (void)salt;
            const uint64_t h = graph_hash(GRAPH_HASH_SEED, probe.key, sizeof(probe.key));
            const int at = c.find(h, [&](const Big &b) { return memcmp(b.key, probe.key, sizeof(b.key)) == 0; });
            if (at >= 0)
            {
                c.hit(at);
                found++;
            }
        }
        clock_gettime(CLOCK_MONOTONIC, &t1);
        const double ns = ((double)(t1.tv_sec - t0.tv_sec) * 1e9 + (double)(t1.tv_nsec - t0.tv_nsec)) / reps;
        printf("lookup at 1024 slots, %s: %.0f ns (hash of 304 bytes + scan%s), %ld of %d found\n", which == 0 ? "hit in the last slot" : "miss", ns,
               which == 0 ? " + full comparison" : "", found, reps);
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && strcmp(argv[1], "lookup") == 0) return lookup_times();
    if (argc != 2 || strcmp(argv[1], "cases") != 0)
    {
        fprintf(stderr, "usage: %s cases | lookup\n", argv[0]);
        return 2;
    }
    fixed_cases();
    long collisions = 0, waits = 0, swept = 0;
    for (uint64_t seed = 1; seed <= 6 && g_failed == 0; seed++)
    {
        Run r;
        r.run(seed * 7919, 4000);
        collisions += r.collisions;
        waits += r.waits;
        swept += r.swept;
    }
    // the stream must have reached what it is there to reach
    CHECK(collisions > 1000, "only %ld lookups met a colliding hash", collisions);
    CHECK(waits > 0 && swept > 100, "the retire list waited %ld times and swept %ld entries", waits, swept);
    if (g_failed)
    {
        printf("FAILED %ld of %ld checks\n", g_failed, g_checks);
        return 1;
    }
    printf("ok %ld\n", g_checks);
    return 0;
}
