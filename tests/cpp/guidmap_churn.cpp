// guidmap_churn — include/nfgpu_guidmap.hpp on the CPU (no GPU, no library): GuidMap against a
// std::map over long random churn, probe runs that wrap past the table's last entry with erases inside
// them, growth from empty through its rehashes, and the mirror protocol of nfgpu_host.hip's
// guid_mirror_update (the whole table after a rebuild, else the logged entries) with lookups on the
// mirror done the way k_guid_find probes.  Prints one summary line; exit 0 = every check held.
//
//   guidmap_churn [seed]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <utility>
#include <vector>

#include "nfgpu_guidmap.hpp"

using nfgpu_detail::GuidMap;
using Key = std::pair<int64_t, int64_t>;

#define CHECK(c, ...)                                   \
    do {                                                \
        if (!(c)) {                                     \
            fprintf(stderr, "%s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);               \
            fprintf(stderr, "\n");                      \
            exit(1);                                    \
        }                                               \
    } while (0)

// the device's entry and hash (nfgpu_kernels.hip GuidEntry / guid_home), restated
struct GuidEntry {
    int64_t h, d;
    int32_t v;
};
static uint64_t guid_home(int64_t h, int64_t d, uint64_t mask) {
    uint64_t x = (uint64_t)h * 0x9E3779B97F4A7C15ull ^ (uint64_t)d;
    x ^= x >> 31;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 29;
    return x & mask;
}
// k_guid_find's probe over a mirror
static int32_t mirror_find(const std::vector<GuidEntry>& t, int64_t h, int64_t d) {
    if (t.empty()) return -1;
    const uint64_t mask = t.size() - 1;
    size_t steps = 0;
    for (uint64_t s = guid_home(h, d, mask);; s = (s + 1) & mask) {
        const GuidEntry e = t[s];
        if (e.v < 0) return -1;
        if (e.h == h && e.d == d) return e.v;
        CHECK(++steps <= t.size(), "mirror probe does not end");
    }
}

// A GuidMap, the std::map it must agree with, and a mirror kept as guid_mirror_update keeps the device's
struct Harness {
    GuidMap m;
    std::map<Key, int32_t> ref;
    std::vector<uint32_t> log;
    std::vector<GuidEntry> mirror;
    bool synced = false;
    size_t n_full = 0, n_patch = 0, n_patched = 0, n_dropped = 0;
    std::mt19937_64 rng;

    explicit Harness(uint64_t seed) : rng(seed) { m.set_log(&log); }

    void insert(Key k, int32_t v) {
        m.insert(k.first, k.second, v);
        ref[k] = v;
    }
    void erase(Key k) {
        m.erase(k.first, k.second);
        ref.erase(k);
    }
    void check_find(Key k) {
        auto it = ref.find(k);
        const int32_t want = it == ref.end() ? -1 : it->second;
        const int32_t got = m.find(k.first, k.second);
        CHECK(got == want, "find(%lld, %lld) = %d, std::map holds %d", (long long)k.first, (long long)k.second, got, want);
        CHECK(m.count(k.first, k.second) == (want >= 0), "count");
    }
    // find_many_par's host branch: a long log is dropped and the mirror marked stale
    void host_batch() {
        if (log.size() > m.capacity() / 8) {
            log.clear();
            synced = false;
            n_dropped++;
        }
    }
    // guid_mirror_update, then the mirror must be the table
    void sync() {
        const size_t cap = m.capacity();
        bool full = m.take_rebuilt() || !synced || mirror.size() != cap;
        size_t np = full ? 0 : log.size();
        if (np > cap / 8) {
            full = true;
            np = 0;
        }
        const GuidMap::E* t = m.entries();
        if (full) {
            mirror.resize(cap);
            for (size_t i = 0; i < cap; i++) mirror[i] = GuidEntry{t[i].h, t[i].d, t[i].v};
            synced = true;
            n_full++;
        } else if (np) {
            for (size_t i = 0; i < np; i++) {
                CHECK(log[i] < cap, "logged index %u outside the table of %zu", log[i], cap);
                mirror[log[i]] = GuidEntry{t[log[i]].h, t[log[i]].d, t[log[i]].v};
            }
            n_patch++;
            n_patched += np;
        }
        log.clear();
        CHECK(mirror.size() == cap, "mirror size");
        size_t live = 0;
        for (size_t i = 0; i < cap; i++) {
            // (an erased entry keeps its stale NFGUID on both sides: every field is compared)
            CHECK(mirror[i].h == t[i].h && mirror[i].d == t[i].d && mirror[i].v == t[i].v,
                  "mirror entry %zu of %zu differs after a %s update", i, cap, full ? "whole" : "logged");
            live += t[i].v >= 0;
        }
        CHECK(live == ref.size() && m.size() == ref.size(), "table holds %zu live entries, size() %zu, std::map %zu", live,
              m.size(), ref.size());
        CHECK(cap == 0 || ref.size() * 2 <= cap, "table more than half full");
    }
    void check_mirror_find(Key k) {
        auto it = ref.find(k);
        const int32_t want = it == ref.end() ? -1 : it->second;
        const int32_t got = mirror_find(mirror, k.first, k.second);
        CHECK(got == want, "mirror lookup (%lld, %lld) = %d, std::map holds %d", (long long)k.first, (long long)k.second, got,
              want);
    }
    void check_all() {
        for (auto& kv : ref) {
            check_find(kv.first);
            check_mirror_find(kv.first);
        }
    }
};

static Key random_key(std::mt19937_64& rng) {
    const int64_t head = (rng() % 10 < 9) ? 7 : 9;   // (one draw a statement: the same run under every compiler)
    const int64_t data = (int64_t)(rng() >> 24) + 1;
    return Key(head, data);
}

// 1. random insert / overwrite / erase / find over a pool of NFGUIDs, the mirror brought up to date
//    after batches of 1..96 operations (now and then a host batch drops a long log first)
static size_t random_churn(uint64_t seed, size_t n_ops, size_t pool_size) {
    Harness H(seed);
    std::vector<Key> pool;
    for (size_t i = 0; i < pool_size; i++) pool.push_back(random_key(H.rng));
    H.sync();   // (an empty table: nothing to mirror, lookups miss)
    H.check_mirror_find(pool[0]);
    size_t done = 0, next_sync = 1;
    int32_t v = 0;
    while (done < n_ops) {
        const Key k = pool[H.rng() % pool.size()];
        switch (H.rng() % 8) {
        case 0: case 1: case 2: H.insert(k, v++ & 0x3FFFFFFF); break;   // (new or overwrite)
        case 3: case 4: H.erase(k); break;                              // (present or not)
        default: H.check_find(k); break;
        }
        done++;
        if (done == next_sync) {
            if (H.rng() % 16 == 0) H.host_batch();
            H.sync();
            for (int i = 0; i < 24; i++) H.check_mirror_find(pool[H.rng() % pool.size()]);
            H.check_mirror_find(random_key(H.rng));   // (nearly always absent)
            const uint64_t longest = H.rng() % 8 == 0 ? 96 : 12;
            next_sync = done + 1 + H.rng() % longest;
        }
    }
    H.sync();
    H.check_all();
    // (a small pool keeps the table small, so its batches outgrow capacity / 8 all the time)
    CHECK(H.n_full >= 3 && H.n_patch > 1000 && (pool_size > 100 || H.n_dropped > 0),
          "mirror paths: %zu whole, %zu logged, %zu dropped logs", H.n_full, H.n_patch, H.n_dropped);
    printf("churn: %zu ops over %zu NFGUIDs, capacity %zu, %zu live; mirror %zu whole / %zu logged (%zu entries) / %zu logs dropped\n",
           done, pool.size(), H.m.capacity(), H.ref.size(), H.n_full, H.n_patch, H.n_patched, H.n_dropped);
    return done;
}

// 2. probe runs across the wrap: at each capacity, NFGUIDs whose home is one of the last 4 entries
//    (more of them than entries there, so their run goes on at entry 0) and of the first 4 (pushed
//    behind the wrapped run), erased and put back in random order, the mirror checked after every call
static size_t wrap_runs(uint64_t seed) {
    size_t wrapped_shifts = 0;
    for (size_t cap = 64; cap <= 4096; cap *= 2) {
        Harness H(seed + cap);
        // fill to the capacity wanted: GuidMap doubles when n + 1 > cap / 2
        std::vector<Key> filler, tail, head;
        while (H.m.capacity() < cap) {
            filler.push_back(random_key(H.rng));
            H.insert(filler.back(), (int32_t)filler.size());
        }
        for (const Key& k : filler) H.erase(k);
        CHECK(H.m.capacity() == cap && H.m.size() == 0, "capacity %zu wanted, %zu", cap, H.m.capacity());
        const size_t mask = cap - 1;
        while (tail.size() < 10 || head.size() < 6) {
            const Key k = random_key(H.rng);
            const size_t hm = GuidMap::home(k.first, k.second, mask);
            CHECK(hm == guid_home(k.first, k.second, mask), "home() differs from the device's hash");
            if (hm >= cap - 4 && tail.size() < 10) tail.push_back(k);
            else if (hm < 4 && head.size() < 6) head.push_back(k);
        }
        std::vector<Key> keys(tail);
        keys.insert(keys.end(), head.begin(), head.end());
        H.sync();
        for (int round = 0; round < 40; round++) {
            // in: a random order, so the wrapped run interleaves both kinds
            for (size_t i = keys.size(); i > 1; i--) std::swap(keys[i - 1], keys[H.rng() % i]);
            for (size_t i = 0; i < keys.size(); i++) {
                H.insert(keys[i], (int32_t)(round * 100 + i));
                H.sync();
            }
            CHECK(H.m.capacity() == cap, "the table grew");
            // the run does wrap: an entry among the first ones whose home is among the last
            const GuidMap::E* t = H.m.entries();
            size_t over = 0;
            for (size_t i = 0; i < 16; i++)
                over += t[i].v >= 0 && GuidMap::home(t[i].h, t[i].d, mask) >= cap - 4;
            CHECK(over >= 6, "capacity %zu: %zu entries wrapped", cap, over);
            CHECK(t[cap - 1].v >= 0 && t[0].v >= 0, "the run does not cross the last entry");
            H.check_all();
            // out: a random order; every erase inside the run shifts later members back, some across the wrap
            for (size_t i = keys.size(); i > 1; i--) std::swap(keys[i - 1], keys[H.rng() % i]);
            for (size_t i = 0; i < keys.size(); i++) {
                const size_t at_front = t[0].v >= 0 ? (size_t)t[0].v : (size_t)-1;
                H.erase(keys[i]);
                wrapped_shifts += t[cap - 1].v >= 0 && (size_t)t[cap - 1].v == at_front;   // entry 0 moved to the last entry
                H.sync();
                for (const Key& k : keys) {
                    H.check_find(k);
                    H.check_mirror_find(k);
                }
            }
            CHECK(H.m.size() == 0, "entries left");
        }
        CHECK(H.n_patch > 100, "the wrap phase must go through the log");
    }
    CHECK(wrapped_shifts > 50, "only %zu erases shifted an entry back across the wrap", wrapped_shifts);
    printf("wrap: capacities 64..4096, %zu erases moved entry 0 back to the last entry\n", wrapped_shifts);
    return wrapped_shifts;
}

// 3. growth from empty through its rehashes with the mirror live, then erased down to nothing
static void growth(uint64_t seed, size_t n) {
    Harness H(seed);
    std::vector<Key> keys;
    size_t rehashes = 0, cap = 0;
    for (size_t i = 0; i < n; i++) {
        Key k = random_key(H.rng);
        if (H.ref.count(k)) continue;
        keys.push_back(k);
        H.insert(k, (int32_t)i);
        if (H.m.capacity() != cap) {
            cap = H.m.capacity();
            rehashes++;
            H.sync();   // (right after the rebuild: the flag, not the log, must carry it)
            H.check_all();
        } else if (i % 257 == 0) {
            H.sync();
            H.check_mirror_find(keys[H.rng() % keys.size()]);
        }
    }
    CHECK(rehashes >= 8, "%zu rehashes", rehashes);
    H.sync();
    H.check_all();
    for (size_t i = 0; i < keys.size(); i++) {
        H.erase(keys[i]);
        if (i % 509 == 0) {
            H.sync();
            H.check_mirror_find(keys[i]);
            H.check_mirror_find(keys[keys.size() - 1]);
        }
    }
    H.sync();
    CHECK(H.m.size() == 0 && H.m.capacity() == cap, "after erasing everything");
    printf("growth: %zu NFGUIDs, %zu rehashes to capacity %zu\n", keys.size(), rehashes, cap);
}

int main(int argc, char** argv) {
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 20261021;
    const size_t ops = random_churn(seed, 240000, 3000) + random_churn(seed + 1, 60000, 40);
    wrap_runs(seed + 2);
    growth(seed + 3, 20000);
    printf("guidmap_churn ok: %zu random operations\n", ops);
    return 0;
}
