// nfgpu_tick.hpp — k_tick, the frame kernel, and its helpers, written over a SCHEMA POLICY:
// DynSchema reads the programs and the working set from Dev / Tables at run time (the kernels
// compiled into libnfgpu.so); a world's own policy, generated from its schema at commit
// (nfgpu_host.hip, jit_*), bakes them in as constants and straight-line code and is compiled
// with this same header by hipRTC.
#pragma once
#include "nfgpu_device.hpp"

namespace nfgpu {

// The next "standalone" dirty Set group of slot e at or after g: a queued Set of a property that
// no program writes, whose value changed over the frame (x_old != x_new).  Returns n_x when none.
__device__ __forceinline__ int next_standalone(const Dev& d, int g, int e) {
    for (; g < d.n_x && d.x_slot[g] == (uint32_t)e; g++)
        if (d.tab->w_slot[d.x_pid[g]] == kNoU &&
            (d.x_old[g] != d.x_new[g] || ((int)d.x_pid[g] >= d.n_if && d.x_old_h[g] != d.x_new_h[g])))
            return g;
    return d.n_x;
}
// recipients of a property event (GetBroadCastObject, AOI:531-593) of slot e's class
struct EvFan {
    uint32_t n;    // messages
    bool pub;      // to the scene group's players but self (else to self)
};
__device__ __forceinline__ EvFan ev_fan(const Dev& d, uint64_t desc, uint32_t pid) {
    const uint8_t fl = d.tab->pflags[desc >> 60][pid];
    return EvFan{event_msgs(desc, fl), (fl & NFK_PUBLIC) != 0};
}

// ---------------------------------------------------------------------------------
// Frame working set (k_tick).  A thread keeps its entity's values of the U slots in registers;
// program operands are addressed by wave-uniform slot numbers (Tables::opu), so a program runs
// without searching a written-property list.
#define NFK_U16(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15)
static_assert(kMaxU == 16, "NFK_U16 enumerates kMaxU slots");

// A frame's U slots: the writable ones [0, n_w), then the read-only ones [n_w, n_w + n_r).  The
// kind tables name a read-only operand by its index r as 0x80 | r, so one table serves every
// frame; kU (template) = the register slots a k_tick variant keeps (n_w + n_r <= kU).
__device__ __forceinline__ uint32_t uslot(uint32_t raw, uint32_t n_w) {
    return (raw & 0x80u) ? n_w + (raw & 0x7Fu) : raw;
}
// j wave-uniform: a scalar branch to one register move
template <int kU>
__device__ __forceinline__ uint64_t uget(const uint64_t (&v)[kU], uint32_t j) {
    switch (__builtin_amdgcn_readfirstlane(j)) {
#define NFK_C(i) \
    case i:      \
        return v[(i) < kU ? (i) : 0];
        NFK_U16(NFK_C)
#undef NFK_C
    }
    return 0;
}
template <int kU>
__device__ __forceinline__ void uput(uint64_t (&v)[kU], uint32_t j, uint64_t x) {
    switch (__builtin_amdgcn_readfirstlane(j)) {
#define NFK_C(i)                   \
    case i:                        \
        v[(i) < kU ? (i) : 0] = x; \
        break;
        NFK_U16(NFK_C)
#undef NFK_C
    }
}
// An accepted Set of a program op, as (kind, op index, U slot, old bits, new bits): k_chain_u's log
// hook; k_tick passes this empty one, which compiles away.
struct NoSetLog {
    __device__ __forceinline__ void operator()(int, int, uint32_t, uint64_t, uint64_t) const {}
};
// The fired kinds' programs in schedule-name order on the register working set.  A Set that
// fails the reference's change predicate leaves the value as it was; wm collects the slots a
// Set changed at least once.  Bit 16 + j of wm, set by the caller: U slot j holds a guard cell whose
// row the record uses (cell_loads); such a slot takes the RIADD_CLAMP ops the walk passes on its
// column, so a later guard reads NFCRecord::GetInt as the walk has left it (an unused row reads 0
// before and after, RC:616-635).  The cell itself, its write-back and events are k_records'.
template <int kU, bool kCells = false, class Log = NoSetLog>
__device__ __forceinline__ void run_programs_u(uint64_t (&v)[kU], uint32_t& wm, const Tables* __restrict__ tab_,
                                               uint32_t fired, int n_kind, uint32_t n_w, const Log& log = Log()) {
    CTables* tab = ctab(tab_);
    for (int k = 0; k < n_kind; k++) {
        if (!((fired >> k) & 1)) continue;
        const int n = tab->nops[k];
        for (int i = 0; i < n; i++) {
            const uint32_t cfd = tab->opx[k][i].cfd, sl = tab->opx[k][i].slots;
            const uint32_t code = cfd & 0xFF, flags = (cfd >> 8) & 0xFF;
            const uint32_t u0 = uslot(sl & 0xFF, n_w), u1 = uslot((sl >> 8) & 0xFF, n_w);
            const uint32_t u2 = uslot((sl >> 16) & 0xFF, n_w), u3 = uslot(sl >> 24, n_w);
            const uint32_t gd = tab->opx[k][i].gd;
            if (gd && !guard_ok((gd >> 8) & 3u, (int64_t)uget(v, uslot(gd & 0xFF, n_w)),
                                (gd & 0x40000000u) ? (int64_t)uget(v, uslot((gd >> 16) & 0xFF, n_w))
                                                   : (int64_t)((int32_t)(gd << 3) >> 19)))  // the constant, bits 16..28
                continue;  // NFK_GUARD
            if (code == NFK_OP_IADD_CLAMP) {
                const int64_t cur = (int64_t)uget(v, u0);
                const int64_t a = (flags & NFK_A_PROP) ? (int64_t)uget(v, u1) : tab->opx[k][i].a;
                const int64_t lo = (flags & NFK_LO_PROP) ? (int64_t)uget(v, u2) : tab->opx[k][i].b;
                const int64_t hi = (flags & NFK_HI_PROP) ? (int64_t)uget(v, u3) : tab->opx[k][i].c;
                int64_t r = (int64_t)((uint64_t)cur + (uint64_t)a);
                r = r < lo ? lo : r;
                r = r > hi ? hi : r;
                uput(v, u0, (uint64_t)r);  // NFCProperty::SetInt (PR:273): r == cur changes nothing
                wm |= (r != cur) ? (1u << u0) : 0u;
                if (r != cur) log(k, i, u0, (uint64_t)cur, (uint64_t)r);
            } else if (code == NFK_OP_FLERP || code == NFK_OP_FAFFINE) {
                const uint64_t xb = uget(v, u0);
                const double x = __longlong_as_double((long long)xb);
                double r;
                if (code == NFK_OP_FLERP) {
                    const double tg = __longlong_as_double((long long)uget(v, u1));
                    const double dd = tg - x;
                    const double m = dd * __longlong_as_double(tab->opx[k][i].b);
                    r = x + m;
                    if (r != r) r = flerp_nan(x, tg, __longlong_as_double(tab->opx[k][i].b));
                } else {
                    const double m = x * __longlong_as_double(tab->opx[k][i].a);
                    r = m + __longlong_as_double(tab->opx[k][i].b);
                    if (r != r) r = faffine_nan(x, __longlong_as_double(tab->opx[k][i].a), __longlong_as_double(tab->opx[k][i].b));
                }
                const bool set = !(fabs(r - x) <= 1e-15);  // NFCProperty::SetFloat (PR:314): IsZeroDouble(v - cur)
                uput(v, u0, set ? (uint64_t)__double_as_longlong(r) : xb);
                wm |= set ? (1u << u0) : 0u;
                if (set) log(k, i, u0, xb, (uint64_t)__double_as_longlong(r));
            } else if (code == NFK_OP_ISET) {
                const uint64_t cur = uget(v, u0);
                const uint64_t r = (flags & NFK_A_PROP) ? uget(v, u1) : (uint64_t)tab->opx[k][i].a;
                uput(v, u0, r);  // NFCProperty::SetInt (PR:273): r == cur changes nothing
                wm |= (r != cur) ? (1u << u0) : 0u;
                if (r != cur) log(k, i, u0, cur, r);
            } else if (code == NFK_OP_FSET) {
                const uint64_t xb = uget(v, u0);
                const uint64_t rb = (flags & NFK_A_PROP) ? uget(v, u1) : (uint64_t)tab->opx[k][i].a;
                const double x = __longlong_as_double((long long)xb), r = __longlong_as_double((long long)rb);
                const bool set = !(fabs(r - x) <= 1e-15);  // NFCProperty::SetFloat (PR:314)
                uput(v, u0, set ? rb : xb);
                wm |= set ? (1u << u0) : 0u;
                if (set) log(k, i, u0, xb, rb);
            } else if (kCells && code == NFK_OP_RIADD_CLAMP) {
                // (kCells: a world with guard cells, DynSchemaT<true>.  The op runs in k_records; sl: the read-only indices of the guard cells on its column)
                for (uint32_t m = sl; m; m &= m - 1) {
                    const uint32_t j = n_w + (uint32_t)__builtin_ctz(m);
                    if ((wm >> (16 + j)) & 1)
                        uput(v, j, (uint64_t)riadd_clamp((int64_t)uget(v, j), tab->opx[k][i].a, tab->opx[k][i].b, tab->opx[k][i].c));
                }
            }
            // record ops run in k_records
        }
    }
}

// Block-wide exclusive scan of a packed 64-bit value (fields must not overflow into each other).
__device__ __forceinline__ unsigned long long block_excl_scan(unsigned long long v, unsigned long long* s_w,
                                                              unsigned long long& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long inc = wave_incl_scan(v);
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    unsigned long long before = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < kTPB / 64; i++) {
        const unsigned long long x = s_w[i];
        before += (i < w) ? x : 0ull;
        total += x;
    }
    return before + inc - v;
}

// Element i (stride str elements) of a wave-uniform array.  A policy with kOff32 (its world's arrays
// are all under 4 GiB from their bases: nfgpu_jit.hpp) addresses it as the scalar base plus a 32-bit
// byte offset, so a column access is one saddr load on an offset shared by every column of the same
// stride, with no 64-bit address arithmetic or 64-bit address registers per lane.
// (The base goes through readfirstlane, which the compiler cannot see through: otherwise it
// re-associates base_k = s_word + k * stride with the lane offset into one 64-bit lane address per
// kind.  Every base here is wave-uniform, so the first lane's is the base.)
template <class S, typename T>
__device__ __forceinline__ T* elem(T* base, uint32_t i, uint32_t str = 1) {
    if constexpr (S::kOff32) {
        const uint64_t p = (uint64_t)base;
        const uint64_t b = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)p) |
                           ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(p >> 32)) << 32);
        typedef __attribute__((address_space(1))) char GChar;  // (global: the saddr forms)
        return (T*)((GChar*)b + i * (uint32_t)(sizeof(T) * str));
    } else
        return base + (size_t)i * str;
}

// The schema k_tick runs: the heartbeat kinds, the programs' working set (U slots) and its event
// order and fan-out classes.  DynSchema reads it at run time (Dev, kernel-argument scalars, and
// Tables through the constant address space); a generated policy (nfgpu_host.hip, jit_source)
// has the same members as constants and the programs as straight-line code on the registers.
// kCells: the instantiations for a world whose programs guard on record cells (NFK_GUARD_CELL); a
// world without such a guard launches DynSchemaT<false>, which has none of that code (its loops
// and register allocation are what they were before the flag existed).
template <bool kCells>
struct DynSchemaT {
    static constexpr bool kStatic = false;
    static constexpr bool kOff32 = false;  // 64-bit element addresses (any world size)
    // non-temporal hints (kNt* bits): none in the library's instantiations
    static constexpr uint32_t kNt = 0;
    // k_tick may rank the frame's tiles itself (Dev::lb_rank: the tiles publish their counts, rank
    // workgroups scan them); a policy of a world that never does (record ops, kAblScanKernel) compiles
    // that code out (kLb = false) and its frames rank by k_scan_tiles
    static constexpr bool kLb = true;
    static constexpr int kNK = NFK_MAX_KINDS;  // (an upper bound only)
    // guard cells (NFK_GUARD_CELL): any U slot may hold one, told by its Dev::u_pid at run time
    static constexpr uint32_t kCellMask = kCells ? 0xFFFFu : 0u;
    __device__ static uint32_t u_cell(const Dev& d, int j) {
        return d.u_pid[j] >= kCellPid ? (uint32_t)d.u_pid[j] & 0x1FFFu : kNoCell;
    }
    __device__ static int rec_rows(const Dev& d, uint32_t rec) { return ctab(d.tab)->rec_rows[rec]; }
    __device__ static int n_kind(const Dev& d) { return d.n_kind; }
    __device__ static int n_w(const Dev& d) { return d.n_w; }
    __device__ static uint32_t u_lower(const Dev& d, int j) { return d.u_lower[j]; }
    __device__ static int u_pid(const Dev& d, int j) { return d.u_pid[j]; }
    __device__ static int u_order(const Dev& d, int i) { return d.u_order[i]; }
    __device__ static uint32_t u_str(const Dev& d, int j) { return (uint32_t)d.u_str[j]; }
    // the event masks of the entity's class (Dev::u_cmask): a select over kernel-argument scalars,
    // no indexed copy and no barrier
    __device__ static uint32_t class_mask(const Dev& d, unsigned cls) {
        uint32_t cm = 0;
#pragma unroll
        for (int i = 0; i < NFK_MAX_CLASSES; i++) cm = cls == (unsigned)i ? d.u_cmask[i] : cm;
        return cm;
    }
    // the U slots the fired kinds read or write
    __device__ static uint32_t need(const Dev& d, uint32_t fired) {
        uint32_t need = 0;
        for (int k = 0; k < d.n_kind; k++)
            if ((fired >> k) & 1) {
                const uint32_t um = ctab(d.tab)->umask[k];  // writable bits | read-only bits << 16
                need |= (um & 0xFFFFu) | ((um >> 16) << d.n_w);
            }
        return need;
    }
    template <int kU, class Log = NoSetLog>
    __device__ static void run(uint64_t (&v)[kU], uint32_t& wm, const Dev& d, uint32_t fired, const Log& log = Log()) {
        run_programs_u<kU, kCells>(v, wm, d.tab, fired, d.n_kind, d.n_w, log);
    }
};

// ---- guard cells (NFK_GUARD_CELL) ----
// A policy names the U slots that may hold a record cell in kCellMask, with u_cell(d, j) = the
// slot's NFK_GUARD_CELL_ID (kNoCell: a property) and rec_rows(d, rec).  A generated policy of a
// world without cell guards has no such members and none of this code is instantiated for it.
template <class S>
constexpr auto cell_slots(int) -> decltype(S::kCellMask) {
    return S::kCellMask;
}
template <class S>
constexpr uint32_t cell_slots(long) {
    return 0u;
}
template <class S>
__device__ __forceinline__ bool slot_is_cell(const Dev& d, int j) {
    if constexpr (cell_slots<S>(0) != 0)
        return ((cell_slots<S>(0) >> j) & 1u) && S::u_cell(d, j) != kNoCell;
    else
        return false;
}
// The guard cells among the needed slots of entity e (e < N, a live slot): the record's used-row
// mask, then — when the record uses the row — the cell at rec_pos(used, rowm, row) of the slot's
// (entity, column) vector; an unused row leaves the register 0 and loads no cell.  row < rows and
// col < cols (checked at commit), so the place is inside the entity's [cols][rows] cells.  Returns
// the slots whose row is used.
template <int kU, class S>
__device__ __forceinline__ uint32_t cell_loads(const Dev& d, int e, uint32_t need, uint64_t (&v)[kU], unsigned& bytes) {
    uint32_t cu = 0;
    constexpr uint32_t km = cell_slots<S>(0);
    if constexpr (km != 0) {
#pragma unroll
        for (int j = 0; j < kU; j++) {
            if (!((km >> j) & 1u)) continue;
            const uint32_t c = S::u_cell(d, j);
            if (c == kNoCell || !((need >> j) & 1u)) continue;
            const uint32_t rec = cell_rec(c), row = cell_row(c);
            const int rows = S::rec_rows(d, rec);
            const uint64_t used = *elem<S>(d.rused[rec], (uint32_t)e);
            bytes += 8;
            if ((used >> row) & 1ull) {
                const uint32_t at = cell_col(c) * (uint32_t)rows + rec_pos(used, rec_rowm(rows), (int)row);
                v[j] = *(elem<S>(d.u_col[j], (uint32_t)e, S::u_str(d, j)) + at);
                cu |= 1u << j;
                bytes += 8;
            }
        }
    }
    return cu;
}

typedef DynSchemaT<false> DynSchema;
typedef DynSchemaT<true> DynSchemaCells;

constexpr int kKindChunk = 8;  // schedule hot records loaded together per chunk
// non-temporal hint bits of a schema policy's kNt (NFGPU_JIT_NT for the hipRTC specialisation)
// kNtFanStore: the fan-out's LDS-window stores (16-byte aligned runs); kNtFanGroupStore: its lane-group
// stores (runs of 16 or more recipients, 16-byte stores at any dword)
constexpr uint32_t kNtSchedLoad = 1, kNtColLoad = 2, kNtEventStore = 4, kNtStateStore = 8, kNtFanStore = 16,
                   kNtFanGroupStore = 32;

// k_tick register budgets (waves per SIMD) by the frame's U slot count
constexpr int kWavesU8 = 8, kWavesU12 = 7;
constexpr int kWavesJit = 5;  // the hipRTC specialisation (nfgpu_jit.hpp; profiles/r11j_jit_waves_ab.txt)
constexpr long long kMsgStrideLimit = 1ll << 30;  // fixed-stride message runs: at most 4 GiB reserved

template <class S>
__device__ __forceinline__ void sched_load(const Dev& d, int e, int k0, uint64_t (&h)[kKindChunk]) {
    // kinds past n_kind re-read the chunk's first word (a cache hit); a static schema loads
    // exactly its kinds
    const int nk = S::n_kind(d) - k0;
#pragma unroll
    for (int j = 0; j < kKindChunk; j++)
        if (!S::kStatic || j < nk)
            h[j] = ld_nt<(S::kNt & kNtSchedLoad) != 0>(elem<S>(d.s_word + (size_t)(k0 + (j < nk ? j : 0)) * d.s_wstr, (uint32_t)e));
}
// One due-test and fire of a WIDE record (the word has kScWide): NFCScheduleModule::Execute's
// reschedule on the 16-byte hot record, the cold record where the hot one cannot give the next
// time.  Returns whether it fired; gone: the fire removed the schedule (the caller clears the word).
template <class S, bool kStore>
__device__ __forceinline__ bool sched_fire_wide(const Dev& d, int e, int k, unsigned& bytes, bool& taken, int32_t& remain,
                                                bool& gone) {
    SchedHot* const at = elem<S>(d.s_wide + (size_t)k * d.s_kstr, (uint32_t)e);
    SchedHot h = *at;
    bytes += 16;
    if (!(d.now > h.next)) return false;
    const bool forever = h.state & kStForever;
    if (!(h.remain > 0 || forever)) return false;
    h.remain -= 1;
    const uint32_t st = h.state;
    if (h.remain <= 0 && !forever) {
        if (!taken) {  // insert into the remove list succeeds for the first one only
            h.state = 0;
            taken = true;
            gone = true;
        }
    } else {
        const bool first = !(st & kStFired);
        if ((st & kStStep) && (first || !forever || h.remain < 0)) {
            // next = start + step * (all - remain) without the cold record (see kSt*)
            if (!first) h.next += st_step(st);
        } else {
            const SchedCold c = *elem<S>(d.s_cold + (size_t)k * d.s_kstr, (uint32_t)e);
            bytes += 16;
            const int64_t step = (int64_t)(c.interval * 1000.0f);
            const int32_t done = (int32_t)((uint32_t)c.all - (uint32_t)h.remain);
            h.next = c.start + step * (int64_t)done;
        }
        h.state = st | kStFired;
    }
    remain = h.remain;
    bytes += 16;
    if (kStore && !(d.ablate & kAblNoSchedStore)) *at = h;
    return true;
}
// NFCScheduleModule::Execute (SM:51-81) for one object: its schedules in name order (kind id
// order).  The 8-byte words of a chunk of kinds are loaded together (independent loads).
// Rescheduled / removed records are stored back.  Every load of the compact path is issued without
// a branch and before the first use of any of them: a load under a branch is followed by a wait at
// the join, and a first use after the record stores would make the wave wait for the stores too
// (the vector memory counter retires in order), i.e. one round trip per kind or per store batch.
// (A wide record is such a load under a branch: the price of the fallback.)
// kStore = false: the fire test only (k_chain re-runs it before k_tick; nothing is stored).
template <class S, bool kFirst, bool kStore = true>
__device__ __forceinline__ void sched_chunk(const Dev& d, int e, int k0, unsigned& bytes, uint64_t& desc,
                                            bool& dead, bool& taken, uint32_t& fired, int32_t* s_rem,
                                            bool oob) {
    uint64_t h[kKindChunk];
    uint8_t ef = 0;
    sched_load<S>(d, e, k0, h);
    if constexpr (kFirst) {
        desc = ld_nt<(S::kNt & kNtSchedLoad) != 0>(elem<S>(d.fan_desc, (uint32_t)e));
        ef = *elem<S>(d.e_flags, (uint32_t)e);  // (always allocated)
        __builtin_amdgcn_sched_barrier(0);  // the scheduler would hoist the first use and its wait
    }
    if constexpr (kFirst) {
        dead = oob || desc_dead(desc);  // a slack slot has no schedules; dead slots store nothing
        taken = d.has_pre && (ef & 1);  // std::map remove-list key already owned (SM:68)
        bytes += d.has_pre ? 1 : 0;
    }
#pragma unroll
    for (int j = 0; j < kKindChunk; j++) {
        const int k = k0 + j;
        if (k >= S::n_kind(d)) break;
        bytes += 8;
        bool fire = false;
        uint64_t w = h[j];
        int32_t remain = 0;
        if (!dead && (w & kStPresent)) {
            if (w & kScWide) {
                bool gone = false;
                fire = sched_fire_wide<S, kStore>(d, e, k, bytes, taken, remain, gone);
                if (fire) fired |= 1u << k;
                if (fire && s_rem) s_rem[k * kTPB + threadIdx.x] = remain;  // for the fired list
                fire = gone;  // the word changes only when the schedule is removed
                w = 0;
            } else if (d.now > d.s_epoch + sc_off(w)) {  // (a compact word exists only once the epoch is fixed)
                const bool forever = w & kStForever;
                remain = sc_remain(w);
                if (remain > 0 || forever) {
                    fire = true;
                    remain -= 1;
                    fired |= 1u << k;
                    if (remain <= 0 && !forever) {
                        if (!taken) {  // insert into the remove list succeeds for the first one only
                            w = 0;
                            taken = true;
                        } else
                            w = sc_word((uint32_t)w, sc_off(w), remain);
                    } else {
                        // next = start + step * (all - remain): the first fire leaves next, later ones add the step
                        const int64_t off = sc_off(w) + ((w & kStFired) ? (int64_t)d.s_step[k] : 0ll);
                        const uint32_t fl = (uint32_t)w | kStFired;
                        if (sc_fits(off, remain))
                            w = sc_word(fl, off, remain);
                        else {  // out of the word's fields: the record goes wide, for good
                            SchedHot x;
                            x.next = d.s_epoch + off;
                            x.remain = remain;
                            x.state = (fl & 7u) | st_pack_step((int64_t)d.s_step[k]);
                            if (kStore && !(d.ablate & kAblNoSchedStore)) *elem<S>(d.s_wide + (size_t)k * d.s_kstr, (uint32_t)e) = x;
                            bytes += 16;
                            w = sc_wide_word(x.state);
                        }
                    }
                    if (s_rem) s_rem[k * kTPB + threadIdx.x] = remain;  // for the fired list
                }
            }
        }
        if (fire) bytes += 8;
        if (kStore && fire && !(d.ablate & kAblNoSchedStore))
            st_nt<(S::kNt & kNtStateStore) != 0>(elem<S>(d.s_word + (size_t)k * d.s_wstr, (uint32_t)e), w);
    }
}
// Loads desc = fan_desc[e] with the first chunk; returns the fired-kind mask.  oob: a slot past N
// (e is then a valid slot re-read, treated as dead).
template <class S = DynSchema, bool kStore = true>
__device__ __forceinline__ uint32_t sched_scan(const Dev& d, int e, unsigned& bytes, uint64_t& desc,
                                               int32_t* s_rem = nullptr, bool oob = false) {
    uint32_t fired = 0;
    bool dead = true, taken = false;
    sched_chunk<S, true, kStore>(d, e, 0, bytes, desc, dead, taken, fired, s_rem, oob);
    for (int k0 = kKindChunk; k0 < S::n_kind(d); k0 += kKindChunk)
        sched_chunk<S, false, kStore>(d, e, k0, bytes, desc, dead, taken, fired, s_rem, oob);
    return fired;
}

// ---- dense ranks in k_tick (Dev::lb_rank) ----
// What k_scan_tiles computes, without its launch.  Every tile publishes its counts once its events
// are written and before its fan-out (a store at the block scan itself, where the counts are first
// known, splits the emission's code there and costs config[1]'s k_tick 9 us even when it never runs:
// profiles/r19a_rank_workgroups_ab.txt): two words, (fired << 16 | events) and messages, each
// tagged with the launch's epoch (lb_st word: epoch << 32 | value; plane q of the array holds word q
// of every tile), stored as relaxed agent-scope atomics.  A tile reads nothing back and waits for
// nothing.  kRankWgs extra workgroups of the same launch (blockIdx.x >= n_tiles) own no tile: rank
// workgroup q polls plane q until every word carries this launch's epoch, scans the counts and writes
// ev_base / fi_base (q = 0) or msg_base (q = 1) and the frame totals.  The word polled is the
// payload, so the result does not depend on when or where a rank workgroup is dispatched: one
// that starts early sleeps between polls in its slot, and no tile ever waits for it.  Nothing is
// cleared between launches (the epoch changes).
constexpr int kRankWgs = 2;
constexpr int kRankPer = 16;  // counts per thread and pass (Dev::lb_rank; 4096 tiles in one pass)
// a poll that has not seen its epoch after this long raises kErrRankWait (constant 100 MHz clock: 1 s)
constexpr unsigned long long kRankWaitTicks = 100000000ull;

__device__ __forceinline__ void lb_store(const Dev& d, int tile, int q, uint32_t v) {
    __hip_atomic_store(d.lb_st + (size_t)q * (size_t)(d.cap / kTile) + tile, ((uint64_t)d.lb_epoch << 32) | v,
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// threads 0 and 1 publish the tile's counts (events and fired fit 16 bits each: the block scan's fields)
__device__ __forceinline__ void lb_publish(const Dev& d, int tile, uint32_t ev, uint32_t fi, uint32_t msg) {
    if (threadIdx.x < 2) lb_store(d, tile, threadIdx.x, threadIdx.x == 0 ? (fi << 16) | ev : msg);
}
// One rank workgroup: passes of kTPB * kPer tiles with a carry.  Every load of a poll round is issued
// before any is checked; stale words are polled again after a sleep.
template <int kPer>
__device__ void lb_rank_wg(const Dev& d, const int q, unsigned long long* s_w, unsigned& s_late) {
    const int n = d.n_tiles, t = (int)threadIdx.x;
    if (t == 0) s_late = 0;
    __syncthreads();
    const uint64_t* const p = d.lb_st + (size_t)q * (size_t)(d.cap / kTile);
    unsigned long long carry = 0;
    for (int c0 = 0; c0 < n; c0 += kTPB * kPer) {
        const int i0 = c0 + t * kPer;
        uint64_t x[kPer];
        uint32_t stale = 0;
#pragma unroll
        for (int j = 0; j < kPer; j++) {
            x[j] = (uint64_t)d.lb_epoch << 32;  // (a tile past n_tiles: count 0)
            if (i0 + j < n) stale |= 1u << j;
        }
        bool late = false;
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        while (stale) {
#pragma unroll
            for (int j = 0; j < kPer; j++)
                if ((stale >> j) & 1u) x[j] = __hip_atomic_load(p + i0 + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
            for (int j = 0; j < kPer; j++)
                if ((uint32_t)(x[j] >> 32) == d.lb_epoch) stale &= ~(1u << j);
            if (!stale) break;
            if (__builtin_amdgcn_s_memrealtime() - t0 > kRankWaitTicks) {
                late = true;
                break;
            }
            __builtin_amdgcn_s_sleep(8);
        }
        // (a barrier every thread reaches: a wave that gave up takes the workgroup out, no rank written)
        if (late) s_late = 1;
        __syncthreads();
        if (s_late) {
            if (late) dev_error(d, kErrRankWait);
            return;
        }
        unsigned long long sum = 0;
#pragma unroll
        for (int j = 0; j < kPer; j++) {
            const uint32_t v = (uint32_t)x[j];
            x[j] = q == 0 ? ((unsigned long long)(v >> 16) << 32) | (v & 0xFFFFu) : v;
            sum += x[j];
        }
        unsigned long long tot;
        unsigned long long run = carry + block_excl_scan(sum, s_w, tot);
#pragma unroll
        for (int j = 0; j < kPer; j++) {
            if (i0 + j < n) {
                if (q == 0) {
                    d.ev_base[i0 + j] = (uint32_t)run;
                    d.fi_base[i0 + j] = (uint32_t)(run >> 32);
                } else {
                    d.msg_base[i0 + j] = (uint32_t)(i0 + j) * d.msg_tcap;  // (fixed-stride runs)
                }
            }
            run += x[j];
        }
        carry += tot;
        __syncthreads();  // (s_w is reused by the next pass)
    }
    if (t == 0) {  // (k_scan_tiles' totals; no record tiles in such a frame)
        if (q == 0) {
            d.ev_base[n] = (uint32_t)carry;
            d.fi_base[n] = (uint32_t)(carry >> 32);
            d.re_base[0] = 0;
            d.ctrl->n_ev = (uint32_t)carry;
            d.ctrl->n_fi = (uint32_t)(carry >> 32);
            d.ctrl->n_re = 0;
        } else {
            const unsigned long long ext = (unsigned long long)n * d.msg_tcap;
            d.msg_base[n] = (uint32_t)ext;
            d.ctrl->msg_extent = ext;
            d.ctrl->n_msgs_ptiles = carry;
            if (ext > (unsigned long long)d.msg_cap || (d.ablate & kAblForceMsgCap)) dev_error(d, kErrMsgCap);
        }
    }
}

// ---- fan-out pieces shared by k_tick's tail and k_fanout (nfgpu_kernels.hip) ----
// An event of a fan-out chunk in LDS, three words: its first message; the first player of its
// group's pl_slot run (a public event) or the entity's own slot (a private one); and
// count | r1 << 14 | public << 31, r1 = 1 + the entity's rank among its group's players (0: not one).
struct FanEv {
    uint32_t ms, a, n, r1;
    bool pub;
};
__device__ __forceinline__ void fan_ev_put(uint32_t* x, uint32_t ms, uint32_t a, uint32_t n, uint32_t r1, bool pub) {
    x[0] = ms;
    x[1] = a;
    x[2] = n | (r1 << 14) | (pub ? 0x80000000u : 0u);
}
__device__ __forceinline__ FanEv fan_ev_get(const uint32_t* x) {
    const uint32_t b = x[2];
    return FanEv{x[0], x[1], b & 0x3FFFu, (b >> 14) & 0x3FFFu, (b >> 31) != 0};
}
// every player of the group but self: recipient p of an entity that is the group's r1-th player
// (r1 = 0: not a player) is player skip_self(p, r1) of the group's run
__device__ __forceinline__ uint32_t skip_self(uint32_t p, uint32_t r1) { return p + ((r1 && p + 1 >= r1) ? 1u : 0u); }
// A thread's part of the pl_slot run [lo, hi) of the groups with messages (hi = 0: none) and its
// largest recipient count, reduced over the wave.  Merging them into s_pb is the caller's: k_tick
// raises the largest count for a wave with a run, k_fanout for every wave.
__device__ __forceinline__ void fan_run_reduce(uint32_t& lo, uint32_t& hi, uint32_t& nmax) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        lo = min(lo, (uint32_t)__shfl_xor((int)lo, m, 64));
        hi = max(hi, (uint32_t)__shfl_xor((int)hi, m, 64));
        nmax = max(nmax, (uint32_t)__shfl_xor((int)nmax, m, 64));
    }
}
// n words of LDS to a 16-byte aligned run of global memory: 16-byte stores and a tail of up to 3 words
template <bool NT>
__device__ __forceinline__ void lds_flush16(uint32_t* dst, const uint32_t* src, uint32_t n) {
    const uint32_t n4 = n >> 2;
    uint4* dst4 = (uint4*)dst;
    const uint4* src4 = (const uint4*)src;
    for (uint32_t i = threadIdx.x; i < n4; i += kTPB) st_nt<NT>(dst4 + i, src4[i]);
    if (threadIdx.x < (n & 3u)) dst[4 * n4 + threadIdx.x] = src[4 * n4 + threadIdx.x];
}

// k_tick: one thread per slot, one workgroup per 256-slot tile, on the programs' working set
// (Dev::u_*, fixed at commit).  Every value the entity's frame touches is loaded in ONE batch of
// independent loads into registers; the fired kinds' programs run on those registers with
// wave-uniform slot numbers; the slots a program or a queued Set changed are diffed against their
// frame-start values (kept in LDS).  Queued SetProperty calls were applied by k_sets: a Set of a
// program destination joins that slot's diff (frame-start value = the group's x_old), a Set of any
// other property is a "standalone" event (x_old -> x_new) merged into the entity's events in
// property-id order.  Outputs of tile t are written densely at [t * tile_cap, t * tile_cap + count);
// k_scan_tiles, or this kernel's rank workgroups (Dev::lb_rank), turn the counts into global ranks.
// kWPE: waves per SIMD the register allocation aims at.  The LDS image of the frame-start values
// is dynamic: n_w writable slots x kTPB.
// Workgroup b (dealt to XCD b mod 8) runs a tile of that XCD's contiguous range: the workgroups of
// one XCD take neighbouring tiles, which its L2 holds (profiles/r11o_ktick_xcd_map_ab.txt)
__device__ __forceinline__ int xcd_tile(int b, int n) {
    const int x = b & 7, i = b >> 3, q = n >> 3, r = n & 7;
    return x * q + min(x, r) + i;
}

// A thread's state of its tile's frame, handed from phase to phase of tick_tile (the working set's
// registers v[kU] travel beside it).
struct TickSt {
    int e;                 // the thread's slot
    uint64_t desc;         // its fan-out descriptor (kDeadDesc past N and for a slack slot)
    uint32_t fired;        // kinds that fired
    uint32_t xh;           // 1 + the slot's first queued Set group (0: none)
    uint32_t xset;         // writable slots that are destinations of a queued Set
    uint32_t wm, dm;       // slots a Set changed at least once (bits 16+: used guard cells); dirty slots
    uint32_t pubm, privm;  // the class's public / private-only writable slots (Dev::u_cmask)
    uint32_t npub, r1;     // recipients of a public event; 1 + rank among the group's players (0: not one)
    unsigned nsd;          // standalone Set events
    unsigned nd, nmsg;     // events and messages
    unsigned nmax;         // largest recipient count of one event
    unsigned pev0, pfi, pmsg0;  // the block scan's prefixes: first event, fired heartbeat, message in the tile
    unsigned bytes;        // algorithmic bytes (the tally)
};

// (block-uniform) a calls-only pass and no Set group in this tile: nothing fires, nothing is dirty
template <class S>
__device__ __forceinline__ void tick_idle_tile(const Dev& d, const int tile, const int e) {
    if (d.has_recops && e < d.N) d.fired_mask[e] = 0;
    if (threadIdx.x == 0) {
        d.t_ev[tile] = 0;
        d.t_fi[tile] = 0;
        d.t_msg[tile] = 0;
    }
    if (S::kLb && d.lb_rank) lb_publish(d, tile, 0u, 0u, 0u);
}

// Load and run: the schedule scan, the slot's queued Set groups, one batch of operand and cell loads,
// the frame-start image (s_o), the fired kinds' programs, the dirty diff, and the write-back of the
// Sets a program undid.
template <int kU, class S>
__device__ __forceinline__ void tick_load_run(const Dev& d, TickSt& t, uint64_t (&v)[kU], uint64_t* s_o, int32_t* s_rem) {
    constexpr int kW = kU < kMaxW ? kU : kMaxW;  // writable register slots
    const int e = t.e;
    {
        // descriptor and schedule records in one round trip, without a branch: slots past N (the
        // last tile) re-read slot N-1 and count as dead; a dead slot stores nothing
        const int ec = e < d.N ? e : d.N - 1;
        t.fired = sched_scan<S>(d, ec, t.bytes, t.desc, s_rem, e >= d.N);  // NFCScheduleModule::Execute (SM:51-81)
        t.desc = e < d.N ? t.desc : kDeadDesc;
        t.bytes = e < d.N ? t.bytes + 8 : 0u;
    }
    const bool live = !desc_dead(t.desc);
    // queued Set groups of this slot (k_sets ran them): program destinations among them
    // (queued Sets are the rare case, here and below: most frames have none, and few entities of a
    // frame that has; the hints keep that code off the programs' path, which the library's 8- and
    // 16-slot instantiations pay for in spills otherwise: profiles/r20a_tick_phases.txt)
    if (live && __builtin_expect(d.n_x != 0, 0)) {
        t.xh = *elem<S>(d.ext_head, (uint32_t)e);
        t.bytes += 4;
        if (t.xh)
            for (int g = (int)t.xh - 1; g < d.n_x && d.x_slot[g] == (uint32_t)e; g++) {
                const uint32_t j = d.tab->w_slot[d.x_pid[g]];
                t.xset |= j != kNoU ? 1u << j : 0u;
                t.bytes += 8;
            }
    }
    uint32_t need = 0, cu = 0;  // cu: the guard-cell slots whose row is used
    if (live) {
        need = t.xset;
        if (!(d.ablate & kAblPrograms)) need |= S::need(d, t.fired);
        // one batch of independent loads: every value this entity's frame reads or writes
#pragma unroll
        for (int j = 0; j < kU; j++)
            if (((need >> j) & 1) && !slot_is_cell<S>(d, j) && !(d.ablate & kAblNoLoads)) {
                v[j] = ld_nt<(S::kNt & kNtColLoad) != 0>(elem<S>(d.u_col[j], (uint32_t)e, S::u_str(d, j)));
                t.bytes += 8;
            }
        if (!(d.ablate & kAblNoLoads)) cu = cell_loads<kU, S>(d, e, need, v, t.bytes);
    }
    if (live) {
#pragma unroll
        for (int j = 0; j < kW; j++)
            if (j < S::n_w(d) && ((need >> j) & 1)) s_o[j * kTPB + threadIdx.x] = v[j];
        // a Set program destination: its frame-start value is the value before the Set group
        if (t.xset) {
            for (int g = (int)t.xh - 1; g < d.n_x && d.x_slot[g] == (uint32_t)e; g++) {
                const uint32_t j = d.tab->w_slot[d.x_pid[g]];
                if (j != kNoU) s_o[j * kTPB + threadIdx.x] = d.x_old[g];
                t.bytes += j != kNoU ? 8 : 0;
            }
            t.wm = t.xset;
        }
        // the fired heartbeats' effect programs, in schedule-name order
        t.wm |= cu << 16;  // (run_programs_u: the used guard cells take the walk's record ops)
        if (!(d.ablate & (kAblPrograms | kAblNoRun)) && t.fired) S::run(v, t.wm, d, t.fired);
    }
    // dirty diff against the frame-start values
#pragma unroll
    for (int j = 0; j < kW; j++)
        if (((t.wm >> j) & 1) && v[j] != s_o[j * kTPB + threadIdx.x]) t.dm |= 1u << j;
    // a Set program destination that a program moved back to its frame-start value has no event,
    // but k_sets changed its column: write it back here (the dirty slots are written with their
    // events)
    if (__builtin_expect((t.xset & ~t.dm) != 0, 0))
#pragma unroll
        for (int j = 0; j < kW; j++)
            if (j < S::n_w(d) && ((t.xset & ~t.dm) >> j) & 1) {
                *elem<S>(d.u_col[j], (uint32_t)e, S::u_str(d, j)) = v[j];
                t.bytes += 8;
            }
}

// Counts.  Fan-out message counts (event_msgs): a public property's event goes to every player of the
// group but the entity itself, a private & !upload one to the entity only.  The message offset
// of a slot's event = the counts of the dirty slots with lower property ids (Dev::u_lower).
template <class S>
__device__ __forceinline__ void tick_counts(const Dev& d, TickSt& t) {
    // the entity's class's event masks (Dev::u_cmask; class 15, a free slot: no slots): a select
    // over kernel-argument scalars, no indexed copy and no barrier
    const uint32_t cm = S::class_mask(d, (unsigned)(t.desc >> 60));
    t.pubm = cm & 0xFFFFu;
    t.privm = cm >> 16;
    t.r1 = (uint32_t)((t.desc >> 46) & 0x3FFF);
    t.npub = (uint32_t)((t.desc >> 32) & 0x3FFF) - (t.r1 ? 1u : 0u);
    t.nmsg = t.npub * __builtin_popcount(t.dm & t.pubm) + __builtin_popcount(t.dm & t.privm);
    t.nmax = (t.dm & t.pubm) ? t.npub : ((t.dm & t.privm) ? 1u : 0u);
    t.nd = __builtin_popcount(t.dm);
    // standalone Set events (properties no program writes): counted here, merged in property-id
    // order with the slots' events by walk_events
    if (t.xh) {
        for (int g = next_standalone(d, (int)t.xh - 1, t.e); g < d.n_x; g = next_standalone(d, g + 1, t.e)) {
            const EvFan f = ev_fan(d, t.desc, d.x_pid[g]);
            t.nsd++;
            t.nmsg += f.n;
            t.nmax = max(t.nmax, f.n);
            t.bytes += 8;
        }
        t.nd += t.nsd;
    }
}

// the entity's events in property-id order: dirty slots (u_order) merged with the standalone
// groups; emit(rank, message offset, pid, slot or -1, group, recipients) per event
template <class S, class Emit>
__device__ __forceinline__ void walk_events(const Dev& d, const TickSt& t, Emit&& emit) {
    int g = next_standalone(d, (int)t.xh - 1, t.e);
    unsigned at = 0, m = 0;
#pragma unroll 1
    for (int i = 0; i <= S::n_w(d); i++) {
        const int j = i < S::n_w(d) ? S::u_order(d, i) : -1;
        const uint32_t pj = j >= 0 ? (uint32_t)S::u_pid(d, j) : 0xFFFFFFFFu;
        while (g < d.n_x && d.x_pid[g] < pj) {
            const EvFan f = ev_fan(d, t.desc, d.x_pid[g]);
            emit(at, m, d.x_pid[g], -1, g, f);
            at++;
            m += f.n;
            g = next_standalone(d, g + 1, t.e);
        }
        if (j >= 0 && ((t.dm >> j) & 1)) {
            const bool pub = (t.pubm >> j) & 1;
            const EvFan f{pub ? t.npub : ((t.privm >> j) & 1u), pub};
            emit(at, m, pj, j, 0, f);
            at++;
            m += f.n;
        }
    }
}

// Write back the changed values; their events in property-id order (rank among the entity's dirty
// slots by Dev::u_lower) at the tile's output run ev0.  !fuse: the events' tile-local message offsets
// too (k_fanout adds the tile's message base).
template <int kU, class S>
__device__ __forceinline__ void emit_events(const Dev& d, TickSt& t, const uint64_t (&v)[kU], const uint64_t* s_o,
                                            const size_t ev0, const bool fuse) {
    constexpr int kW = kU < kMaxW ? kU : kMaxW;
    const int e = t.e;
    const uint32_t dm = t.dm, pubm = t.pubm, privm = t.privm, npub = t.npub;
    const unsigned pev0 = t.pev0, pmsg0 = t.pmsg0;
    uint32_t* const t_evm = d.ev_moff + ev0;
    uint32_t* const t_evs = d.ev_slot + ev0;
    uint32_t* const t_evp = d.ev_pid + ev0;
    uint64_t* const t_evo = d.ev_old + ev0;
    uint64_t* const t_evn = d.ev_new + ev0;
    if (!t.nsd) {
        // A thread's events sit at consecutive ranks, so two consecutive ones are stored
        // together (8-byte stores of the slot and pid words, 16-byte stores of the old and
        // new values, at any dword): one store per array covers most of a wave's run instead
        // of one per event slot with the lanes ~2.4 events apart
        // (tools/event_store_probe.hip: 22.4 -> 18.8 us for config[1]'s 2.5M events)
        constexpr bool kNE = (S::kNt & kNtEventStore) != 0;
        bool pend = false;  // an event held back to be stored with the next one
        uint32_t pa = 0, pp = 0;
        uint64_t po = 0, pn = 0;
#pragma unroll
        for (int j = 0; j < kW; j++) {
            if (j >= S::n_w(d) || !((dm >> j) & 1)) continue;
            const uint32_t below = dm & S::u_lower(d, j);
            const uint32_t at = pev0 + __builtin_popcount(below);
            const uint64_t nv = v[j], ov = s_o[j * kTPB + threadIdx.x];
            const uint32_t pid = (uint32_t)S::u_pid(d, j);
            if (!(d.ablate & kAblNoWriteBack)) st_nt<(S::kNt & kNtStateStore) != 0>(elem<S>(d.u_col[j], (uint32_t)e, S::u_str(d, j)), nv);
            if (!fuse)  // tile-local; k_fanout adds the tile's message base
                st_off(t_evm, at, pmsg0 + npub * __builtin_popcount(below & pubm) +
                                      __builtin_popcount(below & privm));
            if (d.ablate & kAblNoEvStore) {
            } else if (pend && at == pa + 1) {  // (the writable slots are in property-id order)
                st_vec<kNE>(t_evs, 4u * pa, u32x2_a4{(uint32_t)e, (uint32_t)e});
                st_vec<kNE>(t_evp, 4u * pa, u32x2_a4{pp, pid});
                st_vec<kNE>(t_evo, 8u * pa, u32x4_a4{(uint32_t)po, (uint32_t)(po >> 32), (uint32_t)ov, (uint32_t)(ov >> 32)});
                st_vec<kNE>(t_evn, 8u * pa, u32x4_a4{(uint32_t)pn, (uint32_t)(pn >> 32), (uint32_t)nv, (uint32_t)(nv >> 32)});
                pend = false;
            } else {
                if (pend) {
                    st_off_nt<kNE>(t_evs, pa, (uint32_t)e);
                    st_off_nt<kNE>(t_evp, pa, pp);
                    st_off_nt<kNE>(t_evo, pa, po);
                    st_off_nt<kNE>(t_evn, pa, pn);
                }
                pend = true;
                pa = at;
                pp = pid;
                po = ov;
                pn = nv;
            }
            t.bytes += 8 + 24;
        }
        if (pend && !(d.ablate & kAblNoEvStore)) {
            st_off_nt<kNE>(t_evs, pa, (uint32_t)e);
            st_off_nt<kNE>(t_evp, pa, pp);
            st_off_nt<kNE>(t_evo, pa, po);
            st_off_nt<kNE>(t_evn, pa, pn);
        }
    } else {
        // (rare: an entity with standalone Set events) write back the slots, then every
        // event by the merged walk, which reads the slots' new values back from their
        // columns so that no register of the working set stays live in it
#pragma unroll
        for (int j = 0; j < kW; j++)
            if (j < S::n_w(d) && ((dm >> j) & 1)) {
                *elem<S>(d.u_col[j], (uint32_t)e, S::u_str(d, j)) = v[j];
                t.bytes += 8;
            }
        unsigned& bytes = t.bytes;
        walk_events<S>(d, t, [&](unsigned at, unsigned m, uint32_t pid, int j, int g, EvFan) {
            uint64_t ov, nv;
            if (j >= 0) {
                ov = s_o[j * kTPB + threadIdx.x];
                nv = __hip_atomic_load(elem<S>(d.u_col[j], (uint32_t)e, S::u_str(d, j)), __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_WAVEFRONT);
            } else {  // (k_sets wrote the column)
                ov = d.x_old[g];
                nv = d.x_new[g];
                if ((int)pid >= d.n_if) {  // an object property: its head halves beside
                    st_off(d.ev_old_h + ev0, pev0 + at, d.x_old_h[g]);
                    st_off(d.ev_new_h + ev0, pev0 + at, d.x_new_h[g]);
                    bytes += 16;
                }
            }
            st_off(t_evs, pev0 + at, (uint32_t)e);
            st_off(t_evp, pev0 + at, pid);
            st_off(t_evo, pev0 + at, ov);
            st_off(t_evn, pev0 + at, nv);
            if (!fuse) st_off(t_evm, pev0 + at, pmsg0 + m);
            bytes += 24;
        });
    }
}

// the thread's fired heartbeats into the tile's fired list at fi0: (slot, kind, remain after the fire)
template <class S>
__device__ __forceinline__ void emit_fired(const Dev& d, TickSt& t, const int32_t* s_rem, const size_t fi0) {
    const int e = t.e;
    uint32_t* const t_fis = d.fi_slot + fi0;
    uint32_t* const t_fik = d.fi_kind + fi0;
    int32_t* const t_fir = d.fi_remain + fi0;
    unsigned pfi = t.pfi;
    uint32_t fl = t.fired;
    while (fl) {
        const int k = __builtin_ctz(fl);
        fl &= fl - 1;
        constexpr bool kNE = (S::kNt & kNtEventStore) != 0;
        const int32_t rem = s_rem[k * kTPB + threadIdx.x];
        // (a forever heartbeat's remain may be any int32, the sentinel too: sched_edges worlds
        // wrap it through INT32_MIN; a counted one is >= 0 after a fire.  The forever bit is the
        // same before and after the scan, in a compact word and in a wide one's, so the word is read
        // whatever the L1 holds)
        if ((d.ablate & kAblCheckRem) && rem == kRemUnset &&
            !(*elem<S>(d.s_word + (size_t)k * d.s_wstr, (uint32_t)e) & kStForever))
            dev_error(d, kErrRemain);
        if (!(d.ablate & kAblNoFiStore)) {
            st_off_nt<kNE>(t_fis, pfi, (uint32_t)e);
            st_off_nt<kNE>(t_fik, pfi, (uint32_t)k);
            st_off_nt<kNE>(t_fir, pfi, rem);
        }
        pfi++;
        t.bytes += 12;
    }
}

// ---- k_tick's fan-out (GetBroadCastObject, AOI:531-593; see k_fanout) ----
// A tile's recipients go into its fixed-stride run `out` (msg_rcpt + tile * msg_tcap) in event order.
// The LDS region of the frame-start image (R words at s_o) is reused, in one of three forms that
// fan_out chooses for the whole tile: fan_direct, or chunks of event triples (fan_fill) expanded by
// fan_lane_groups or fan_window.
// What the three forms share: the region's layout and the groups' player run.
struct FanLds {
    uint32_t* s_ev;    // a chunk's event triples (FanEv)
    uint32_t* s_win;   // the message window behind them (fan_window)
    uint32_t* s_pl;    // the staged player run at the region's end (staged)
    uint32_t pb_lo;    // its first index in pl_slot
    bool staged;       // else the players are read from pl_slot
};
// player p of the run that starts at pl_slot[a], from the staged run when there is one
__device__ __forceinline__ uint32_t fan_player(const Dev& d, const FanLds& f, uint32_t a, uint32_t p) {
    return f.staged ? f.s_pl[a - f.pb_lo + p] : (uint32_t)d.pl_slot[a + p];
}

// Short runs whose tile's whole run fits beside the staged players: no triples, no event loop and
// no window passes.  A thread knows its own events and their message offsets, so it writes their
// recipients straight into the window [0, tmsg) at s_run (tile-local offsets), and the window is
// stored once.  The players are read from pl_slot through L1 (a group's run is read by its ~250
// neighbouring threads), which saves the staging and its barrier.  nm: the tile's largest run.
template <int kU, class S>
__device__ __forceinline__ void fan_direct(const Dev& d, const TickSt& t, uint32_t* const s_run, uint32_t* out,
                                           const unsigned tmsg, const uint32_t nm) {
    constexpr int kW = kU < kMaxW ? kU : kMaxW;
    const int e = t.e;
    const uint64_t desc = t.desc;
    const uint32_t dm = t.dm, pubm = t.pubm, privm = t.privm, npub = t.npub, r1 = t.r1;
    const unsigned pmsg0 = t.pmsg0;
    if (t.nsd) {  // (rare) the merged walk gives each event's offset and recipients
        walk_events<S>(d, t, [&](unsigned, unsigned m, uint32_t, int, int, EvFan f) {
            uint32_t* w = s_run + pmsg0 + m;
            if (!f.pub) {
                if (f.n) w[0] = (uint32_t)e;
                return;
            }
            const auto* pl = d.pl_slot + (uint32_t)desc;
            for (uint32_t k = 0; k < f.n; k++) w[k] = (uint32_t)pl[skip_self(k, r1)];
        });
    } else if (t.nmsg) {
        // public events with recipients: the q-th one's run starts npub * q + (the
        // private events before it: 4 bits each in pk) words after the thread's first
        const uint32_t dpub = npub ? dm & pubm : 0u, dprv = dm & privm;
        unsigned long long pk = 0;
        if (dprv) {  // a private event goes to the entity itself
#pragma unroll
            for (int j = 0; j < kW; j++) {
                if (j >= S::n_w(d)) continue;
                const uint32_t below = dm & S::u_lower(d, j);
                const uint32_t q = __builtin_popcount(below & pubm), pv = __builtin_popcount(below & privm);
                if ((dprv >> j) & 1) s_run[pmsg0 + npub * q + pv] = (uint32_t)e;
                pk |= ((dpub >> j) & 1) ? (unsigned long long)pv << (4u * q) : 0ull;
            }
        }
        const uint32_t npe = __builtin_popcount(dpub);
        if (npe) {
            // eight recipients at a time, read once and written to every public event's
            // run: a store past a run's end repeats its last word (the same value at the
            // same place), so only the event loop's trip count differs between lanes
            const auto* pl = d.pl_slot + (uint32_t)desc;
#pragma unroll 1
            for (uint32_t k0 = 0; k0 < nm; k0 += 8) {  // uniform
                uint32_t x[8], o[8];
#pragma unroll
                for (int k = 0; k < 8; k++) {  // every player of the group but self
                    o[k] = min(k0 + (uint32_t)k, npub - 1u);
                    x[k] = (uint32_t)pl[skip_self(o[k], r1)];
                }
                uint32_t* w = s_run + pmsg0;
                unsigned long long pq = pk;
                for (uint32_t q = 0; q < npe; q++) {
                    uint32_t* wq = w + ((uint32_t)pq & 15u);
#pragma unroll
                    for (int k = 0; k < 8; k++) wq[o[k]] = x[k];
                    w += npub;
                    pq >>= 4;
                }
            }
        }
    }
    __syncthreads();
    // out is 16-byte aligned (msg_tcap is a multiple of 4); nothing refills the window
    lds_flush16<(S::kNt & kNtFanStore) != 0>(out, s_run, tmsg);
}

// The thread's events of the chunk [c0, c1) of the tile's events as triples at f.s_ev.
template <class S>
__device__ __forceinline__ void fan_fill(const Dev& d, const TickSt& t, const FanLds& f, const unsigned c0, const unsigned c1) {
    const int e = t.e;
    const uint64_t desc = t.desc;
    const uint32_t dm = t.dm, pubm = t.pubm, privm = t.privm, npub = t.npub, r1 = t.r1;
    const unsigned pev0 = t.pev0, pmsg0 = t.pmsg0;
    if (!(t.nd && pev0 < c1 && pev0 + t.nd > c0)) return;
    if (t.nsd) {
        walk_events<S>(d, t, [&](unsigned at, unsigned m, uint32_t, int, int, EvFan ef) {
            const unsigned a = pev0 + at;
            if (a < c0 || a >= c1) return;
            fan_ev_put(f.s_ev + 3u * (a - c0), pmsg0 + m, ef.pub ? (uint32_t)desc : (uint32_t)e, ef.n, r1, ef.pub);
        });
    } else {
        // a runtime loop over the slots (an unrolled one gets hoisted out of the chunk loop
        // and spills: 12 slots x 4 values)
#pragma unroll 1
        for (int j = 0; j < S::n_w(d); j++) {
            if (!((dm >> j) & 1)) continue;
            const uint32_t below = dm & S::u_lower(d, j);
            const uint32_t at = pev0 + __builtin_popcount(below);
            if (at < c0 || at >= c1) continue;
            const bool pub = (pubm >> j) & 1;
            const uint32_t m = pmsg0 + npub * __builtin_popcount(below & pubm) +
                               __builtin_popcount(below & privm);
            const uint32_t n = pub ? npub : ((privm >> j) & 1u);
            fan_ev_put(f.s_ev + 3u * (at - c0), m, pub ? (uint32_t)desc : (uint32_t)e, n, r1, pub);
        }
    }
}

// Runs of 16 or more recipients, straight to HBM: n events of a chunk by lane groups of L/4 lanes
// (L = the tile's largest recipient count rounded up to a power of two), four consecutive recipients
// per lane in one 16-byte store (dword-aligned: runs start anywhere); consecutive events' runs are
// adjacent, so a wave writes 64 x 16 B of one contiguous stretch
template <class S>
__device__ __forceinline__ void fan_lane_groups(const Dev& d, const FanLds& f, uint32_t* out, const uint32_t n_ev, const uint32_t L) {
    const uint32_t L4 = L >= 4 ? L / 4 : 1u, sub4 = threadIdx.x & (L4 - 1);
    for (uint32_t i = threadIdx.x / L4; i < n_ev; i += kTPB / L4) {
        const FanEv ev = fan_ev_get(f.s_ev + 3 * i);
        const uint32_t ms = ev.ms, n = ev.n;
        if (!ev.pub) {  // private & !upload: the entity itself (n is 0 or 1)
            if (sub4 == 0 && n) out[ms] = ev.a;
            continue;
        }
        for (uint32_t p = 4 * sub4; p < n; p += 4 * L4) {  // every player of the group but self
            uint32_t x[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint32_t pq = p + (uint32_t)q;
                x[q] = pq < n ? fan_player(d, f, ev.a, skip_self(pq, ev.r1)) : 0u;
            }
            if (p + 4 <= n) {
                if constexpr ((S::kNt & kNtFanGroupStore) != 0)
                    __builtin_nontemporal_store(u32x4_a4{x[0], x[1], x[2], x[3]}, (u32x4_a4*)(out + ms + p));
                else
                    *(u32x4_a4*)(out + ms + p) = u32x4_a4{x[0], x[1], x[2], x[3]};
            } else {
#pragma unroll
                for (int q = 0; q < 3; q++)
                    if (p + (uint32_t)q < n) out[ms + p + q] = x[q];
            }
        }
    }
}

// Shorter runs: n events of a chunk written one thread per event into an LDS message window of W
// words that is stored with 16-byte stores, in as many passes as the chunk's messages need (short
// runs stored directly leave lines partly written by several waves, and lane groups would re-read
// each event's triple once per lane).
template <class S>
__device__ __forceinline__ void fan_window(const Dev& d, const FanLds& f, uint32_t* out, const uint32_t n_ev, const unsigned W) {
    const FanEv last = fan_ev_get(f.s_ev + 3u * (n_ev - 1u));
    const unsigned m_lo = f.s_ev[0], m_hi = last.ms + last.n;
    for (unsigned w0 = m_lo; w0 < m_hi; w0 += W) {  // uniform
        const unsigned w1 = min(m_hi, w0 + W);
        // short runs: one thread per event (fewer LDS reads than lane groups)
        for (uint32_t i = threadIdx.x; i < n_ev; i += kTPB) {
            const FanEv ev = fan_ev_get(f.s_ev + 3 * i);
            const uint32_t ms = ev.ms, n = ev.n, r1 = ev.r1;
            if (n == 0 || ms >= w1 || ms + n <= w0) continue;
            if (!ev.pub) {
                f.s_win[ms - w0] = ev.a;
                continue;
            }
            const uint32_t np = n + (r1 ? 1u : 0u);
            uint32_t k = ms;
            for (uint32_t p = 0; p < np; p++) {
                if (p + 1 == r1) continue;
                if (k >= w0 && k < w1) f.s_win[k - w0] = fan_player(d, f, ev.a, p);
                k++;
            }
        }
        __syncthreads();
        const uint32_t n = w1 - w0;
        if ((w0 & 3u) == 0) {  // out is 16-byte aligned (msg_tcap is a multiple of 4): 16-byte stores
            lds_flush16<(S::kNt & kNtFanStore) != 0>(out + w0, f.s_win, n);
        } else {
            for (uint32_t i = threadIdx.x; i < n; i += kTPB) out[w0 + i] = f.s_win[i];
        }
        __syncthreads();
    }
}

// The tile's fan-out: the block-uniform choice of its form.  tev / tmsg: the tile's events and
// messages; s_pb: the groups' player run [lo, hi) and the largest recipient count (tick_tile).
template <int kU, class S>
__device__ __forceinline__ void fan_out(const Dev& d, TickSt& t, const int tile, const unsigned tev, const unsigned tmsg,
                                        const uint32_t* s_pb, uint64_t* s_o) {
    const unsigned R = (unsigned)d.lds_words;
    const uint32_t pb_lo = s_pb[0], npl = s_pb[1] > s_pb[0] ? s_pb[1] - s_pb[0] : 0u;
    const uint32_t nm = s_pb[2];
    const uint32_t L = nm <= 1 ? 1u : nm >= 64 ? 64u : 1u << (32 - __builtin_clz(nm - 1));
    const bool win = L < ((d.ablate & kAblFanWin32) ? 64u : (d.ablate & kAblFanWin16) ? 32u : 16u);
    const bool staged = npl <= R / 4;
    const unsigned room = R - (staged ? npl : 0u);
    // events per chunk: all of them, or what leaves the window half of the room
    const unsigned ecap = (min(tev, win ? room / 6u : room / 3u) + 3u) & ~3u;
    const unsigned W = win ? (room - 3u * ecap) & ~3u : 0u;  // window entries
    FanLds f;
    f.s_ev = (uint32_t*)s_o;
    f.s_win = f.s_ev + 3u * ecap;
    f.s_pl = f.s_ev + (R - npl);
    f.pb_lo = pb_lo;
    f.staged = staged;
    uint32_t* out = d.msg_rcpt + (unsigned)tile * d.msg_tcap;
    // NFGPU_ABLATE kAblFanTriples keeps the triples for every tile
    const bool direct = win && staged && !(d.ablate & kAblFanTriples) && tmsg <= ((R - npl) & ~3u);
    if (staged) {  // (the tally counts the run once for a direct tile too: summaries do not depend on the path)
        if (!direct)
            for (uint32_t i = threadIdx.x; i < npl; i += kTPB) f.s_pl[i] = (uint32_t)d.pl_slot[pb_lo + i];
        t.bytes += 4 * ((npl + kTPB - 1 - threadIdx.x) / kTPB);
    }
    t.bytes += 4 * t.nmsg;
    if (direct) {
        fan_direct<kU, S>(d, t, (uint32_t*)s_o, out, tmsg, nm);
        return;
    }
    for (unsigned c0 = 0; c0 < tev; c0 += ecap) {  // uniform: chunks of event triples
        const unsigned c1 = min(tev, c0 + ecap);
        fan_fill<S>(d, t, f, c0, c1);
        __syncthreads();
        if (win)
            fan_window<S>(d, f, out, c1 - c0, W);
        else
            fan_lane_groups<S>(d, f, out, c1 - c0, L);
        if (c1 < tev) __syncthreads();  // s_ev is refilled
    }
}

// One tile of k_tick (the workgroup's; its LDS passed in).
template <int kU, class S>
__device__ __forceinline__ void tick_tile(const Dev& d, const int tile, unsigned long long* s_w, unsigned& s_bytes,
                                          uint32_t* s_pb, uint64_t* s_o) {
    const int e = tile * kTile + (int)threadIdx.x;
    if (d.tile_work && !d.tile_work[tile]) {
        tick_idle_tile<S>(d, tile, e);
        return;
    }
    const bool fuse = d.msg_tcap != 0;  // this tile's fan-out is written here, at tile * msg_tcap
    if (threadIdx.x == 0) {
        s_bytes = 0;
        s_pb[0] = 0xFFFFFFFFu;
        s_pb[1] = 0;
        s_pb[2] = 1;
    }
    int32_t* s_rem = (int32_t*)(s_o + (size_t)S::n_w(d) * kTPB);  // [n_kind][kTPB] remain after a fire
    if (d.ablate & kAblCheckRem)  // (this thread's own column: read back only by this thread)
        for (int k = 0; k < S::n_kind(d); k++) s_rem[k * kTPB + threadIdx.x] = kRemUnset;
    TickSt t{};
    t.e = e;
    t.desc = kDeadDesc;
    uint64_t v[kU];
#pragma unroll
    for (int j = 0; j < kU; j++) v[j] = 0;
    tick_load_run<kU, S>(d, t, v, s_o, s_rem);
    tick_counts<S>(d, t);
    // tile-local compaction: one block scan of (fired:16 | events:16 | messages:32)
    const unsigned nf = __builtin_popcount(t.fired);
    unsigned long long tot;
    const unsigned long long excl =
        block_excl_scan(((unsigned long long)nf << 48) | ((unsigned long long)t.nd << 32) | t.nmsg, s_w, tot);
    t.pev0 = (unsigned)((excl >> 32) & 0xFFFF);
    t.pfi = (unsigned)(excl >> 48);
    t.pmsg0 = (unsigned)excl;
    const unsigned tmsg = (unsigned)tot;
    // (after the scan: its barrier orders thread 0's s_pb initialisation before these atomics, and
    // the barrier before the fan-out orders them before its reads)
    if (fuse) {  // the pl_slot run of the groups whose members have messages (they are contiguous)
        const uint32_t np = (uint32_t)((t.desc >> 32) & 0x3FFF);
        uint32_t lo = t.nmsg ? (uint32_t)t.desc : 0xFFFFFFFFu, hi = t.nmsg ? (uint32_t)t.desc + np : 0u;
        fan_run_reduce(lo, hi, t.nmax);
        if ((threadIdx.x & 63) == 0 && hi) {
            atomicMin(&s_pb[0], lo);
            atomicMax(&s_pb[1], hi);
            atomicMax(&s_pb[2], t.nmax);
        }
    }
    // this tile's output runs (wave-uniform bases, tile-local 32-bit offsets)
    const size_t ev0 = (size_t)tile * d.ev_tcap, fi0 = (size_t)tile * d.fi_tcap;
    if (!desc_dead(t.desc)) {
        // (the three are independent: the slot's Set groups were read through t.xh, the fired list
        // reads s_rem, the events read v and s_o.  This order is the one that spills least in the
        // library's instantiations: profiles/r20a_tick_phases.txt)
        if (t.xh) *elem<S>(d.ext_head, (uint32_t)e) = 0;
        emit_fired<S>(d, t, s_rem, fi0);
        if (t.nd && !(d.ablate & kAblNoEmit)) emit_events<kU, S>(d, t, v, s_o, ev0, fuse);
    }
    if (d.has_recops && e < d.N) {  // slack slots too: a slot's previous occupant left a mask
        *elem<S>(d.fired_mask, (uint32_t)e) = t.fired;
        t.bytes += 4;
    }
    if (!fuse && !(d.ablate & kAblNoEmit)) t.bytes += 4 * t.nd;  // ev_moff
    if (fuse) {
        __syncthreads();  // s_pb; every read of s_o and s_rem is done: the region is reused
        const unsigned tev = (unsigned)((tot >> 32) & 0xFFFF);
        if (tmsg > d.msg_tcap && threadIdx.x == 0) dev_error(d, kErrFanBound);  // (host bound)
        // this tile's counts for the dense ranks (the rank workgroups poll them while the fan-out runs)
        if (S::kLb && d.lb_rank) lb_publish(d, tile, tev, (unsigned)(tot >> 48), tmsg);
        // No per-event message offsets: the tile's run holds its events' recipients in event order
        // (the readers count through it: k_counted_moff)
        if (tmsg && tmsg <= d.msg_tcap) fan_out<kU, S>(d, t, tile, tev, tmsg, s_pb, s_o);
    }
    // tile counts and algorithmic-byte tally
    const unsigned wb = (unsigned)wave_sum(t.bytes);
    if ((threadIdx.x & 63) == 0) atomicAdd(&s_bytes, wb);
    __syncthreads();
    if (threadIdx.x == 0) {
        d.t_ev[tile] = (unsigned)((tot >> 32) & 0xFFFF);
        d.t_fi[tile] = (unsigned)(tot >> 48);
        d.t_msg[tile] = (unsigned)tot;
        tally_add(d, kTallyTick, (unsigned long long)(s_bytes + 12 + (fuse ? 16 : 0)));
    }
}

template <int kWPE, int kU, class S = DynSchema>
__global__ __launch_bounds__(kTPB) __attribute__((amdgpu_waves_per_eu(kWPE, 8))) void k_tick(Dev d) {
    __shared__ unsigned long long s_w[kTPB / 64];
    __shared__ unsigned s_bytes;
    __shared__ uint32_t s_pb[3];   // pl_slot run of the groups with dirty events [lo, hi), most recipients
    extern __shared__ __align__(16) uint64_t s_o[];  // [n_w][kTPB] frame-start values of the writable slots
    if constexpr (S::kLb) {
        if ((int)blockIdx.x >= d.n_tiles) {  // a rank workgroup (Dev::lb_rank counts per thread and pass)
            const int q = (int)blockIdx.x - d.n_tiles;
            if (d.lb_rank == 1) lb_rank_wg<1>(d, q, s_w, s_bytes);  // (s_bytes: a tile's tally, free here)
            else lb_rank_wg<kRankPer>(d, q, s_w, s_bytes);
            return;
        }
    }
    tick_tile<kU, S>(d, xcd_tile((int)blockIdx.x, d.n_tiles), s_w, s_bytes, s_pb, s_o);
}


// ---------------------------------------------------------------------------------
// The per-Set log of the watched properties (nfk_watch_props; see k_chain in nfgpu_kernels.hip) on
// the frame's register working set, under the world's schema policy: the fire test without its
// stores, the operand loads and the fired kinds' programs exactly as k_tick runs them (its hipRTC
// specialisation's straight-line programs, or the library's tables), on the values k_sets left,
// before k_tick.  The programs run twice on register copies — count the watched Sets, then write
// them at their places from a block scan — so the log is tile-staged in (slot, kind, op) order with
// no atomics: tile t's entries at t * tcap, t_cnt[t] of them.
struct ChainEnt {
    uint32_t slot;
    uint16_t pid;
    uint8_t kind, op;
    uint64_t old_bits, new_bits;
};
static_assert(sizeof(ChainEnt) == 24, "ChainEnt is read back as 24-byte records");

template <int kU, class S>
__global__ __launch_bounds__(kTPB) void k_chain_u(Dev d, ChainEnt* __restrict__ out, uint32_t* __restrict__ t_cnt,
                                                  uint32_t tcap, uint32_t kinds, uint64_t watch0, uint64_t watch1) {
    __shared__ unsigned long long s_w[kTPB / 64];
    const int e = blockIdx.x * kTPB + (int)threadIdx.x;
    uint32_t fired = 0;
    uint64_t v[kU];
#pragma unroll
    for (int j = 0; j < kU; j++) v[j] = 0;
    if (e < d.N) {
        unsigned bytes = 0;
        uint64_t desc = kDeadDesc;
        fired = sched_scan<S, false>(d, e, bytes, desc) & kinds;
        if (desc_dead(desc)) fired = 0;
    }
    uint32_t cu = 0;  // the guard-cell slots whose row is used (cell_loads)
    if (fired) {
        const uint32_t need = S::need(d, fired);
#pragma unroll
        for (int j = 0; j < kU; j++)
            if (((need >> j) & 1) && !slot_is_cell<S>(d, j)) v[j] = *elem<S>(d.u_col[j], (uint32_t)e, S::u_str(d, j));
        unsigned bytes = 0;
        cu = cell_loads<kU, S>(d, e, need, v, bytes);
    }
    const auto watched = [&](uint32_t u) {
        const uint32_t p = (uint32_t)S::u_pid(d, (int)u);
        return ((p < 64 ? watch0 >> p : watch1 >> (p - 64)) & 1ull) != 0;
    };
    uint32_t cnt = 0;
    if (fired) {
        uint64_t c[kU];
#pragma unroll
        for (int j = 0; j < kU; j++) c[j] = v[j];
        uint32_t wm = cu << 16;
        S::run(c, wm, d, fired, [&](int, int, uint32_t u, uint64_t, uint64_t) { cnt += watched(u) ? 1u : 0u; });
    }
    unsigned long long tot;
    uint32_t at = (uint32_t)block_excl_scan(cnt, s_w, tot);
    if (cnt) {
        ChainEnt* t_out = out + (size_t)blockIdx.x * tcap;
        uint32_t wm = cu << 16;
        S::run(v, wm, d, fired, [&](int k, int i, uint32_t u, uint64_t o, uint64_t n) {
            if (watched(u) && at < tcap)
                t_out[at++] = ChainEnt{(uint32_t)e, (uint16_t)S::u_pid(d, (int)u), (uint8_t)k, (uint8_t)i, o, n};
        });
    }
    if (threadIdx.x == 0) t_cnt[blockIdx.x] = (uint32_t)tot;
}

}  // namespace nfgpu
