// nfgpu_host.hip — C-ABI implementation (include/nfgpu.h): world lifetime, schema,
// membership layout, queued SetProperty / schedule calls, frame launch, readback.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <numeric>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include <mutex>
#include <thread>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "nfgpu_jit.hpp"
#include "nfgpu_kernels.hip"
#include "../../include/nfgpu_guidmap.hpp"
#include "nfgpu_pool.hpp"

using namespace nfgpu;

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define HIPCHK(x)                                                                          \
    do {                                                                                   \
        hipError_t _e = (x);                                                               \
        if (_e != hipSuccess)                                                              \
            return fail(NFK_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(_e));     \
    } while (0)

using nfgpu_detail::GuidMap;
using nfgpu_detail::HostPool;

template <typename T>
int dalloc(T** p, size_t n) {
    *p = nullptr;
    if (n == 0) n = 1;
    hipError_t e = hipMalloc((void**)p, n * sizeof(T));
    if (e != hipSuccess) return fail(NFK_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
    return NFK_OK;
}

enum { KT_TICK = 0, KT_REC = 1, KT_FAN = 2, KT_AUX = 3, KT_SCAN = 4, KT_MEM = 5, KT_CHAIN = 6, KT_N = 7 };
static_assert(KT_N == NFK_N_KERNEL_TIMERS, "nfk_kernel_times' arrays");

struct PendingTiming {
    int kind;
    hipEvent_t a, b;
    int64_t bytes_before;
};

struct MemPlan;

struct World {
    nfk_config cfg{};
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int32_t n_obj = 0;
    bool committed = false;
    int n_prop = 0;  // properties: int [0, n_int), f64 [n_int, n_if), object (NFGUID) [n_if, n_prop)
    int n_if = 0;    // n_int + n_flt
    int n_pw = 0;    // property words of a row: n_if + 2 object halves per object property
    // host-mapped error word (Dev::err_host): device error bits, seen without a device read
    unsigned* err_host = nullptr;
    unsigned* err_host_d = nullptr;

    std::vector<int64_t> gh, gd;
    struct Guid { int64_t h, d; };
    std::vector<Guid> guid;  // (gh, gd) side by side: one cache line per NFGUID comparison
    std::vector<int32_t> scene, group;
    std::vector<uint8_t> cls, isplayer;
    GuidMap obj_of;
    std::vector<int32_t> slot_of_obj, obj_of_slot;  // -1: not resident / slack slot
    std::vector<uint8_t> alive;                       // object exists (not destroyed / exported)
    std::vector<int64_t> src_row;                     // >= 0: arrives from row src_row of ins_rows
    std::vector<uint8_t> m_flag;                      // membership changed in this window
    std::vector<int32_t> touched;                     // objects with m_flag set
    // scene-group segments in (scene, group) order; slot range [base, base + cap)
    struct Seg {
        int32_t scene, group, base, cap;
        int32_t np = 0;             // players among objs (set by seg_meta)
        std::vector<int32_t> objs;  // live objects, NFGUID order
        // their NFGUIDs, beside them: a joiner's place is binary-searched in this contiguous array
        // instead of through guid[objs[i]] (one random host read per probe, ~8 per joiner)
        std::vector<Guid> keys;
    };
    std::vector<Seg> segs;
    std::vector<uint64_t> seg_key;  // each segment's (scene, group) as seg_key_of gives it: ascending
    int32_t slack = 16;  // slack slots per 256 live (nfk_config::slack_per_256)
    int32_t pid_scene = -1, pid_group = -1, pid_x = -1, pid_y = -1, pid_z = -1;  // nfk_set_scene_props
    int32_t row_words = 0;
    uint64_t* ins_rows = nullptr;  // rows of entities imported this window
    size_t ins_cap = 0, ins_n = 0;
    uint64_t* mv_rows = nullptr;   // rows of entities moving inside this shard
    size_t mv_cap = 0;
    void* mlist = nullptr;         // device copy of the membership lists
    size_t mlist_cap = 0;
    std::vector<char> mhost;       // host staging of the membership lists
    // pinned double buffer the lists are uploaded from, so no upload waits for the stream
    char* mpin[2] = {nullptr, nullptr};
    size_t mpin_cap[2] = {0, 0};
    hipEvent_t mpin_done[2] = {nullptr, nullptr};
    bool mpin_pending[2] = {false, false};
    int mpin_slot = 0;
    // nfk_export_objects' slot list, read by k_pack straight from pinned host memory (a few
    // hundred rows: no copy, which behind a busy stream could wait for it)
    int32_t* xpin = nullptr;
    int32_t* xpin_dev = nullptr;
    size_t xpin_cap = 0;
    hipEvent_t xpin_done = nullptr;
    bool xpin_pending = false;
    uint64_t* fan_desc_w = nullptr;
    int32_t* pl_slot_w = nullptr;
    int64_t n_relayout_full = 0, n_relayout_seg = 0;
    double ms_relayout_full = 0, ms_relayout_seg = 0;  // host time in plan/commit_membership
    std::unique_ptr<MemPlan> mplan;            // the window's membership plan (scratch kept)
    void* glist = nullptr;  // device-generated membership lists (untouched segments of a full re-layout)
    size_t glist_cap = 0;
    std::vector<std::vector<uint64_t>> init_props;
    std::vector<std::vector<uint64_t>> init_rcells, init_rused;
    std::vector<bool> rec_defined;
    uint8_t rec_ctype[NFK_MAX_RECORDS][NFK_MAX_REC_COLS] = {};  // NFK_REC_*
    // property links (nfk_link_record): per record the rows summed (0: no link) and each column's
    // int property (-1: none), the linked properties as a mask, and the frame's hit masks and sums
    // (LinkDev, the third argument of k_rrows and k_links' own)
    int8_t lk_rows[NFK_MAX_RECORDS] = {};
    int8_t lk_pid[NFK_MAX_RECORDS][NFK_MAX_REC_COLS];
    uint64_t lk_pids[2] = {0, 0};
    void* lk_buf = nullptr;
    size_t lk_cap = 0;
    int16_t lk_of_pid[128];  // a linked property's rec << 4 | col (link_pid_mask keeps it), else -1
    bool linked_pid(int32_t p) const { return p >= 0 && p < 128 && ((lk_pids[p >> 6] >> (p & 63)) & 1); }

    Tables tab{};
    bool kind_defined[NFK_MAX_KINDS] = {};
    uint64_t dst_union_mask[2] = {0, 0};  // properties written by any program (bit per pid)
    // frame working set of k_tick (Dev::u_*): program destinations / read-only operands
    bool u_ok = false;
    std::vector<int> u_wp, u_rp;
    int n_dst_union = 0;

    Dev d{};
    Tables* tab_d = nullptr;
    Ctrl* ctrl = nullptr;
    int32_t* slot_obj_d = nullptr;
    int32_t nseg = 0;
    std::vector<void*> allocs;
    // dense readback scratch (nfk_read_*), grown on demand
    void* dense = nullptr;
    size_t dense_cap = 0;
    // nfk_read_frame: the dense region on the device and its pinned host copy, device scratch, and
    // the NFGUID order of the objects (guid_sorted; rank_d[object] on the device for rank_n objects)
    void* fr_dev = nullptr;
    char* fr_pin = nullptr;
    size_t fr_cap = 0;
    void* fr_scr = nullptr;
    size_t fr_scap = 0;
    std::vector<int32_t> guid_sorted;
    int32_t* rank_d = nullptr;
    size_t rank_cap = 0;
    int32_t rank_n = 0;

    // queued calls
    // queued calls; `slot` holds the object index until nfk_execute resolves it after the
    // window's membership changes
    struct XOp { uint32_t slot, pid; uint64_t bits; };
    std::vector<XOp> xops;
    std::vector<uint64_t> xops_h;  // the NFGUID head half of each queued call (worlds with object properties)
    // the SetProperty groups are folded on the device (k_xkeys, radix sort, k_scan_heads,
    // k_xgroups): object -> slot after the window's membership changes (rebuilt by k_obj_slots
    // when the membership changed), and the fold's scratch
    int32_t* obj_slot_d = nullptr;
    size_t obj_slot_cap = 0;
    bool obj_slot_dirty = true;
    void* xf_buf = nullptr;
    size_t xf_cap = 0;
    // SetProperty calls of large batches queued on the device (set_props_dev), in two buffers used
    // by alternate windows: the window's first xq_n calls are xq[xq_b][0, xq_n) (XOp records), the
    // host xops the calls queued after them; xq_ev[b]: the frame that folded buffer b read it
    void* xq[2] = {nullptr, nullptr};
    size_t xq_cap[2] = {0, 0};  // records
    hipEvent_t xq_ev[2] = {nullptr, nullptr};
    bool xq_ev_set[2] = {false, false};
    int xq_b = 0;
    size_t xq_n = 0;
    uint8_t* tile_work_d = nullptr;  // a calls-only pass's tiles with SetProperty groups (Dev::tile_work)
    size_t tile_work_cap = 0;
    std::vector<int32_t> look;           // GUID lookups of one batched call
    // GUID lookups of large call batches on the device (find_many_dev): obj_of's device mirror
    // (guid_d, same entries and hash), the log of the entries the host table wrote since the
    // mirror was last brought up to date, the batch's pinned and device buffers, and a stream of
    // their own (the world's stream may be running the previous frame)
    std::vector<uint32_t> guid_log;
    void* guid_d = nullptr;
    size_t guid_dcap = 0;       // bytes
    size_t guid_dmask = 0;      // capacity - 1 of the mirrored table
    bool guid_synced = false;
    hipStream_t look_stream = nullptr;
    char* look_pin = nullptr;
    size_t look_pin_cap = 0;
    void* look_dev = nullptr;
    size_t look_dev_cap = 0;
    size_t dev_look_min = 4096;  // batches from this size on (NFGPU_DEV_LOOKUP; 0 = never)
    // the window's SetProperty calls of properties no program writes, and those properties: they
    // bound a tile's standalone events (nfk_execute)
    int64_t sa_calls = 0;
    uint64_t sa_pids[2] = {0, 0};
    // GetProperty* (nfk_get_props): device values read since the last frame, and the queued
    // SetProperty chain of each (object, property): ov_last[key] = its last xop, ov_prev links back
    std::unordered_map<uint64_t, uint64_t> dcache;
    std::unordered_map<uint64_t, uint32_t> ov_last;
    std::vector<uint32_t> ov_prev;
    uint64_t* gat = nullptr;             // device scratch of gathered reads
    size_t gat_cap = 0;
    uint32_t* moff_tmp = nullptr;        // device scratch of nfk_read_fanout's counted offsets
    size_t moff_tmp_cap = 0;
    // host worker threads for large call batches (NFGPU_HOST_THREADS, default 1 = none)
    std::unique_ptr<HostPool> pool;
    size_t par_calls = 16384;  // batches from this size on use the pool (NFGPU_PAR_CALLS: tests)
    // queued SetRecordInt / SetRecordFloat calls (obj: object index until nfk_execute resolves it;
    // rrc = rec << 16 | row << 8 | col) and their folding scratch
    // op 0 SetRecord*, 1 AddRow (row 0xFF: -1; aux = its values' index in rvals, or 0xFFFFFFFF),
    // 2 Remove, 3 ClearRecord, 4 SwapRowInfo (row the origin, the col field the target row)
    struct RSOp { uint32_t obj, rrc; uint64_t bits; uint32_t op, aux; };
    std::vector<RSOp> rsq;
    // the NFGUID head halves of the queued SetRecordObject calls (bits: the data halves), parallel
    // to rsq and filled up lazily: shorter than rsq until the window's first such call (rsq_head)
    std::vector<uint64_t> rsq_h;
    uint64_t rsq_head(size_t k) const { return k < rsq_h.size() ? rsq_h[k] : 0ull; }
    bool rec_obj = false;  // a record has an object column (fixed at nfk_commit)
    // the head halves of the object cells' Update events, tile-staged beside Dev::re_old / re_new
    // (rec_obj), and the frame's RecHeads (the SetRecord kernels' second argument)
    uint64_t* re_old_h = nullptr;
    uint64_t* re_new_h = nullptr;
    RecHeads rheads{};
    std::vector<uint64_t> rvals;  // AddRow values, NFK_MAX_REC_COLS words each
    std::unordered_map<uint64_t, std::vector<uint32_t>> rq_index;  // (object << 3 | record) -> its queued calls
    std::unordered_map<uint64_t, uint64_t> ucache;  // (object << 3 | record) -> used mask read this window
    // (object << 7 | linked property) -> its column's cells in row order, read this window (current_props)
    std::unordered_map<uint64_t, std::vector<uint64_t>> lcache;
    std::vector<uint64_t> rowpairs;  // (slot << 3 | record) with row operations this window (nfk_execute)
    void* rl_buf = nullptr;          // rs_has / rl_cnt / rl_ev
    size_t rl_cap = 0;
    std::vector<uint64_t> rpk, rpk_t;
    std::vector<uint32_t> rs_slot_h, rs_rrc_h, rs_first_h, rss_slot_h, rss_g0_h;
    void* rs_buf = nullptr;   // rs_old / rs_new
    size_t rs_cap = 0;
    void* rss_buf = nullptr;  // rss_ev / rss_msg / rss_pos / rss_pmsg
    size_t rss_cap = 0;
    // the device fold of the schedule calls (hf_buf: keys, counts, pre / post entries, added flags);
    // the last pass's post entries (hf_post, count at *hf_npost) stay for nfk_read_added
    void* hf_buf = nullptr;
    size_t hf_cap = 0;
    bool hf_pending = false;
    size_t hf_max = 0;         // post entries' room (2 per call)
    const uint32_t* hf_npost = nullptr;
    const uint32_t* hf_pslot = nullptr;
    const uint32_t* hf_pkind = nullptr;
    const uint32_t* hf_pop = nullptr;
    const uint8_t* hf_added = nullptr;
    void* xs_buf = nullptr;  // x_old / x_new (/ x_old_h / x_new_h)
    size_t xs_cap = 0;
    struct HOp { int32_t code; uint32_t slot, kind; float interval; int32_t count; int64_t time; };
    std::vector<HOp> hops;
    // schedule words (nfgpu_device.hpp): the kinds still without a common step, and whether the
    // epoch is fixed (fix_schedule_steps)
    uint32_t s_unfixed = 0;
    bool s_epoch_set = false;

    // pinned upload arena + device staging
    void* pin = nullptr;
    size_t pin_cap = 0;
    hipEvent_t pin_done = nullptr;
    bool pin_pending = false;
    void* stage = nullptr;
    size_t stage_cap = 0;

    // k_tick specialised to this world's schema (nfgpu_jit.hpp); null: the generic instantiations
    hipFunction_t jit_fn = nullptr;
    hipFunction_t jit_chain_fn = nullptr;  // k_chain_u on the same policy
    int jit_waves = 0, jit_u = 0;
    bool jit_lb = false;  // the specialisation has k_tick's rank workgroups compiled in (JitSchema::kLb)
    std::string jit_msg = "not compiled";

    int32_t ticks = 0;
    uint32_t last_tcap = 0;  // Dev::msg_tcap of the last launched frame
    uint32_t last_rtcap = 0; // Dev::msg_rtcap of the last launched frame (0: records not fused)
    uint32_t lb_epoch = 0;       // k_tick's own ranks: the last launch's epoch (Dev::lb_epoch)
    bool scan_pending = false;  // the last frame's dense ranks (k_scan_tiles) are built on first read
    Dev scan_dev;               // ... with that frame's Dev
    int64_t last_rec_msgs = 0;  // record-tile messages of the last summarised frame (capacity hint)
    // the last frame ran k_fanout: its error word is copied to err_pin (event err_done) and
    // checked before anything reads or replaces that frame's fan-out (check_fanout)
    bool fan_unchecked = false;
    unsigned* err_pin = nullptr;
    // pinned landing area of the frame's control block and byte tallies (read_ctrl / read_ctrl_tallies:
    // asynchronous copies behind the frame and one stream synchronisation, not two synchronous copies)
    char* ctrl_pin = nullptr;
    hipEvent_t err_done = nullptr;
    int32_t max_np = 0;    // most players in one scene group (an upper bound between full re-layouts)
    // per-Set chains of the watched properties (nfk_watch_props, k_chain): the watch mask, the log
    // of the last nfk_execute (ChainEnt records, its count on the device) and whether that frame ran it
    // (k_chain stages it per tile: chain_tcap records per tile, chain_cnt_d the tiles' counts; the
    // read-back's device scratch and pinned copy are the chain's own, so nfk_read_frame's stay valid)
    uint64_t chain_watch[2] = {0, 0};
    ChainEnt* chain_d = nullptr;
    uint32_t* chain_cnt_d = nullptr;
    size_t chain_cap = 0;  // records
    uint32_t chain_tcap = 0;
    int32_t chain_tiles = 0;
    bool chain_ran = false;
    void* chain_scr = nullptr;
    size_t chain_scap = 0;
    char* chain_pin = nullptr;
    size_t chain_pcap = 0;
    // scene queries (nfk_query_objects): the batch's device scratch (descriptors, tile counts and
    // bases, offsets and hits) and the pinned host buffer of the uploaded descriptors and the
    // result, both grown on demand; q_mark[object]: affected in this window (set and cleared per call)
    void* q_dev = nullptr;
    size_t q_dcap = 0;
    char* q_pin = nullptr;
    size_t q_pcap = 0;
    std::vector<uint8_t> q_mark;
    // the scenes and (scene, group) pairs (seg_key_of) whose emptied segment a re-layout dropped: such
    // a group still exists for the reference (its NFCSceneGroupInfo stays until ReleaseGroupScene).
    // Written only there, so a world whose groups never empty keeps both sets empty
    std::unordered_set<uint64_t> known_groups;
    std::unordered_set<int32_t> known_scenes;
    hipEvent_t q_ev[2] = {nullptr, nullptr};
    // view changes (nfk_view_changes): the window's membership log (appended by the membership calls,
    // cleared where the window's membership is applied), the resident per-slot departure instants
    // (all 0xFFFFFFFF between calls: a call scatters the window's leavers and restores them with the
    // same list; vc_dirty: a failed call left some behind), the batch's device scratch and the pinned
    // buffer of the upload and the result, both grown on demand; vc_last[object]: its open stint
    std::vector<nfk_vc_entry> vc_log;
    uint32_t* vc_tout = nullptr;
    int32_t vc_tout_cap = 0;
    bool vc_dirty = false;
    void* vc_dev = nullptr;
    size_t vc_dcap = 0;
    char* vc_pin = nullptr;
    size_t vc_pcap = 0;
    std::vector<int32_t> vc_last;
    hipEvent_t vc_ev[2] = {nullptr, nullptr};
    // record finds (nfk_find_rows): the batch's descriptors and row masks on the device and in
    // pinned host memory (descriptors first, masks behind them), both grown on demand; the last
    // call's figures for nfk_find_stats
    void* f_dev = nullptr;
    size_t f_dcap = 0;
    char* f_pin = nullptr;
    size_t f_pcap = 0;
    hipEvent_t f_ev[2] = {nullptr, nullptr};
    double f_kernel_ms = 0;
    int64_t f_bytes = 0;
    int32_t f_host = 0;
    // resource calls (nfk_adjust_props): the batch's descriptors and results on the device and in
    // pinned host memory (descriptors, new values, result bytes), both grown on demand; the last
    // call's figures for nfk_adjust_stats
    void* a_dev = nullptr;
    size_t a_dcap = 0;
    char* a_pin = nullptr;
    size_t a_pcap = 0;
    hipEvent_t a_ev[2] = {nullptr, nullptr};
    nfk_adjust_stats_t a_stats{};
    // enter snapshots (nfk_snapshot_objects): the walk's order (empty: id order), its table on the
    // device (rebuilt when flags or order change), the batch's scratch (requests, counts, bases) and
    // result region on the device, and the pinned buffer the nfk_snapshot pointers index
    std::vector<int32_t> s_porder, s_rorder;
    SnapTab s_tab{};
    uint32_t s_cells_ub[NFK_MAX_CLASSES][2] = {};  // most cells of a request of (class, view)
    SnapTab* s_tab_d = nullptr;
    bool s_tab_dirty = true;
    void* s_dev = nullptr;
    size_t s_dcap = 0;
    void* s_out = nullptr;
    size_t s_ocap = 0;
    char* s_pin = nullptr;
    size_t s_pcap = 0;
    hipEvent_t s_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    std::vector<uint8_t> s_mark;

    bool profiling = false;
    std::vector<PendingTiming> pend;
    std::vector<hipEvent_t> evpool;
    double kt_ms[KT_N] = {};
    int64_t kt_n[KT_N] = {};
    int64_t kt_bytes[KT_N] = {};
    uint64_t last_bytes[3] = {0, 0, 0};
};

// the device error bits in the host-mapped words (dev_error: one word per bit)
inline unsigned err_host_bits(const World* w) {
    unsigned e = 0;
    for (int i = 0; i < kErrHostWords; i++) e |= ((volatile const unsigned*)w->err_host)[i] ? 1u << i : 0u;
    return e;
}
inline void clear_err_host(World* w) {
    for (int i = 0; i < kErrHostWords; i++) ((volatile unsigned*)w->err_host)[i] = 0;
}

constexpr uint32_t kNoKind = 0xFFFFFFFFu;  // HOp::kind of a RemoveSchedule(self, name) with no device program
// a queued SetProperty of a property no program writes: a standalone event (see nfk_execute)
inline void count_standalone(World* w, uint32_t pid) {
    if (w->tab.w_slot[pid] == kNoU) {
        w->sa_calls++;
        w->sa_pids[pid >> 6] |= 1ull << (pid & 63);
    }
}
static_assert(sizeof(World::HOp) == sizeof(HCall) && offsetof(World::HOp, time) == offsetof(HCall, time),
              "k_hkeys / k_hfold read the queued schedule calls as uploaded");
static_assert(sizeof(World::XOp) == sizeof(XCall) && offsetof(World::XOp, bits) == offsetof(XCall, bits),
              "k_xkeys reads the queued SetProperty calls as uploaded");

// word of property pid (its data half for an object property) in an entity row
inline int64_t prop_word(const World* w, int32_t pid) {
    return pid < w->n_if ? pid : w->n_if + 2 * (int64_t)(pid - w->n_if);
}

// Every failure of nfk_execute after the window's membership changes are applied drops the
// window's remaining queued calls (SetProperty / SetObject, SetRecord, schedule calls) with it: the
// membership part cannot be undone, so none of the window's calls is applied out of its order in
// a later frame.  (A failure before that keeps every queue.)
int drop_window(World* w, int r) {
    w->xq_n = 0;
    w->xops.clear();
    w->xops_h.clear();
    w->sa_calls = 0;
    w->sa_pids[0] = w->sa_pids[1] = 0;
    w->hops.clear();
    w->rsq.clear();
    w->rsq_h.clear();
    w->rvals.clear();
    w->rq_index.clear();
    w->ucache.clear();
    w->lcache.clear();
    w->dcache.clear();
    w->ov_last.clear();
    w->ov_prev.clear();
    return r;
}

int alloc_track(World* w, void** p, size_t bytes) {
    *p = nullptr;
    hipError_t e = hipMalloc(p, bytes ? bytes : 16);
    if (e != hipSuccess) return fail(NFK_ERR_HIP, std::string("hipMalloc ") + std::to_string(bytes) + ": " + hipGetErrorString(e));
    w->allocs.push_back(*p);
    return NFK_OK;
}
#define ALLOC(ptr, bytes)                                                    \
    do {                                                                     \
        void* _p;                                                            \
        int _r = alloc_track(w, &_p, (size_t)(bytes));                       \
        if (_r) return _r;                                                   \
        ptr = reinterpret_cast<decltype(ptr)>(_p);                           \
    } while (0)

hipEvent_t get_event(World* w) {
    if (!w->evpool.empty()) {
        hipEvent_t e = w->evpool.back();
        w->evpool.pop_back();
        return e;
    }
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

int drain_timings(World* w) {
    for (auto& p : w->pend) {
        HIPCHK(hipEventSynchronize(p.b));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, p.a, p.b));
        w->kt_ms[p.kind] += ms;
        w->kt_n[p.kind] += 1;
        w->evpool.push_back(p.a);
        w->evpool.push_back(p.b);
    }
    w->pend.clear();
    return NFK_OK;
}

struct TimeScope {
    World* w;
    int kind;
    hipEvent_t a = nullptr, b = nullptr;
    TimeScope(World* ww, int k) : w(ww), kind(k) {
        if (w->profiling) {
            a = get_event(w);
            b = get_event(w);
            if (a) (void)hipEventRecord(a, w->stream);
        }
    }
    ~TimeScope() {
        if (w->profiling && a && b) {
            (void)hipEventRecord(b, w->stream);
            w->pend.push_back({kind, a, b, 0});
        }
    }
};

// reserve a pinned host arena (waits for the previous upload to finish reading it)
int pin_reserve(World* w, size_t bytes) {
    if (w->pin_pending) {
        HIPCHK(hipEventSynchronize(w->pin_done));
        w->pin_pending = false;
    }
    if (bytes > w->pin_cap) {
        if (w->pin) HIPCHK(hipHostFree(w->pin));
        w->pin = nullptr;
        size_t cap = std::max(bytes, w->pin_cap * 2);
        w->pin_cap = 0;  // (until the new buffer exists)
        HIPCHK(hipHostMalloc(&w->pin, cap, hipHostMallocDefault));
        w->pin_cap = cap;
    }
    if (bytes > w->stage_cap) {
        // kernels of earlier frames may still read the old staging buffer
        HIPCHK(hipStreamSynchronize(w->stream));
        if (w->stage) HIPCHK(hipFree(w->stage));
        w->stage = nullptr;
        size_t cap = std::max(bytes, w->stage_cap * 2);
        w->stage_cap = 0;  // (until the new buffer exists)
        HIPCHK(hipMalloc(&w->stage, cap));
        w->stage_cap = cap;
    }
    return NFK_OK;
}

size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

int lookup(World* w, int64_t h, int64_t d, int32_t* obj) {
    *obj = w->obj_of.find(h, d);
    if (*obj < 0) return fail(NFK_ERR_NOTFOUND, "no object " + std::to_string(h) + "-" + std::to_string(d));
    return NFK_OK;
}

// accumulated algorithmic-byte tallies of k_tick, k_records, k_fanout
constexpr size_t kTallyBytes = (size_t)3 * kTallyN * 8 * 8;  // (the tallies' 64-byte spread slots)
constexpr size_t kCtrlPinTally = (sizeof(Ctrl) + 255) & ~(size_t)255;
constexpr size_t kCtrlPinBytes = kCtrlPinTally + kTallyBytes;
int read_tallies(World* w, uint64_t out[3]) {
    std::vector<unsigned long long> t((size_t)3 * kTallyN * 8);
    HIPCHK(hipMemcpy(t.data(), w->d.tally, t.size() * 8, hipMemcpyDeviceToHost));
    for (int k = 0; k < 3; k++) {
        out[k] = 0;
        for (int i = 0; i < kTallyN; i++) out[k] += t[((size_t)k * kTallyN + i) * 8];
    }
    return NFK_OK;
}

// dense scratch for readback, at least `bytes`
int dense_reserve(World* w, size_t bytes) {
    if (bytes <= w->dense_cap) return NFK_OK;
    HIPCHK(hipStreamSynchronize(w->stream));
    if (w->dense) HIPCHK(hipFree(w->dense));
    w->dense = nullptr;
    HIPCHK(hipMalloc(&w->dense, bytes));
    w->dense_cap = bytes;
    return NFK_OK;
}

// tile-staged src -> host array in global order (n entries)
template <typename T>
int gather_tiles(World* w, const T* src, const uint32_t* base, int n_tiles, int tcap, size_t n, T* host) {
    if (n == 0 || n_tiles == 0) return NFK_OK;
    int r = dense_reserve(w, n * sizeof(T));
    if (r) return r;
    const unsigned nb = (unsigned)std::min(n_tiles, 4096);
    hipLaunchKernelGGL(k_compact<T>, dim3(nb), dim3(kTPB), 0, w->stream, src, (T*)w->dense, base, n_tiles, tcap);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(host, w->dense, n * sizeof(T), hipMemcpyDeviceToHost, w->stream));
    HIPCHK(hipStreamSynchronize(w->stream));
    return NFK_OK;
}
#define GATHER(...)                    \
    do {                               \
        int _r = gather_tiles(__VA_ARGS__); \
        if (_r) return _r;             \
    } while (0)

// ---------------- membership layout ----------------
// Slots are grouped in scene-group segments in (scene, group) order.  Inside a segment the live
// entities sit in NFGUID order, followed by slack slots (fan_desc = kDeadDesc) that absorb
// arrivals without moving other segments.  NFCSceneGroupInfo keeps its member maps as
// std::map<NFGUID, ...>, so slot order is both the reference's dirty-sync order and
// GetBroadCastObject's recipient order (AOI:572, KM:1270-1294).
bool guid_less(const World* w, int32_t a, int32_t b) {
    const World::Guid x = w->guid[a], y = w->guid[b];
    return x.h != y.h ? x.h < y.h : x.d < y.d;
}

// (scene, group) as one word whose unsigned order is the pair's signed order
uint64_t seg_key_of(int32_t scene, int32_t group) {
    return ((uint64_t)((uint32_t)scene ^ 0x80000000u) << 32) | ((uint32_t)group ^ 0x80000000u);
}

// the segment of (scene, group), or -1
int32_t find_seg(const World* w, int32_t scene, int32_t group) {
    const uint64_t k = seg_key_of(scene, group);
    const auto it = std::lower_bound(w->seg_key.begin(), w->seg_key.end(), k);
    return it != w->seg_key.end() && *it == k ? (int32_t)(it - w->seg_key.begin()) : -1;
}

void index_segs(World* w) {
    w->seg_key.resize(w->segs.size());
    for (size_t g = 0; g < w->segs.size(); g++) w->seg_key[g] = seg_key_of(w->segs[g].scene, w->segs[g].group);
}

int32_t seg_slack(int32_t slack, int32_t len) {
    return slack <= 0 ? 0 : std::max<int32_t>(2, (int32_t)(((int64_t)len * slack + 255) / 256));
}

// segments of every live object with `slack` slots per 256; returns the slot total
int64_t plan_segments(World* w, int32_t slack, std::vector<World::Seg>& segs) {
    std::vector<int32_t> objs;
    for (int32_t o = 0; o < w->n_obj; o++)
        if (w->alive[o]) objs.push_back(o);
    std::sort(objs.begin(), objs.end(), [w](int32_t a, int32_t b) {
        if (w->scene[a] != w->scene[b]) return w->scene[a] < w->scene[b];
        if (w->group[a] != w->group[b]) return w->group[a] < w->group[b];
        return guid_less(w, a, b);
    });
    segs.clear();
    int64_t base = 0;
    for (size_t i = 0; i < objs.size();) {
        size_t j = i;
        const int32_t o = objs[i];
        while (j < objs.size() && w->scene[objs[j]] == w->scene[o] && w->group[objs[j]] == w->group[o]) j++;
        World::Seg g;
        g.scene = w->scene[o];
        g.group = w->group[o];
        g.base = (int32_t)std::min<int64_t>(base, INT32_MAX);
        g.objs.assign(objs.begin() + i, objs.begin() + j);
        g.keys.resize(g.objs.size());
        for (size_t k = 0; k < g.objs.size(); k++) g.keys[k] = w->guid[g.objs[k]];
        g.cap = (int32_t)g.objs.size() + seg_slack(slack, (int32_t)g.objs.size());
        base += g.cap;
        segs.push_back(std::move(g));
        i = j;
    }
    return base;
}

// per-slot metadata of one segment: slot -> object, fan-out descriptor, and the player run
// pl_slot[base, base + players) in NFGUID order (NFCSceneGroupInfo::mxPlayerList)
struct MetaLists {
    std::vector<int32_t> slot, obj, pl;
    std::vector<uint64_t> desc;
};

int seg_meta(World* w, World::Seg& g, MetaLists& m) {
    int32_t np = 0;
    for (int32_t o : g.objs) np += w->isplayer[o] ? 1 : 0;
    if (np > 0x3FFF) return fail(NFK_ERR_ARG, "more than 16383 players in one scene group");
    g.np = np;
    w->max_np = std::max(w->max_np, np);
    const size_t at = m.slot.size();
    int32_t rank = 0;
    for (int32_t i = 0; i < g.cap; i++) {
        m.slot.push_back(g.base + i);
        m.pl.push_back(0);
        if (i < (int32_t)g.objs.size()) {
            const int32_t o = g.objs[i];
            const bool pl = w->isplayer[o];
            m.obj.push_back(o);
            m.desc.push_back((uint64_t)(uint32_t)g.base | ((uint64_t)np << 32) |
                             ((uint64_t)(pl ? rank + 1 : 0) << 46) | ((uint64_t)w->cls[o] << 60));
            if (pl) m.pl[at + rank++] = g.base + i;
        } else {
            m.obj.push_back(-1);
            m.desc.push_back(kDeadDesc);
        }
    }
    return NFK_OK;
}

void set_tiles(Dev& d, int32_t n_slots) {
    d.N = n_slots;
    d.n_tiles = (n_slots + kTile - 1) / kTile;
    d.n_rtiles = (n_slots + kRTile - 1) / kRTile;
}

// grow a device buffer (contents dropped; callers only grow between uses)
int dev_reserve(World* w, void** p, size_t* cap, size_t bytes) {
    if (bytes <= *cap) return NFK_OK;
    HIPCHK(hipStreamSynchronize(w->stream));
    if (*p) HIPCHK(hipFree(*p));
    *p = nullptr;
    const size_t c = std::max(bytes, *cap + *cap / 2);
    *cap = 0;  // (until the new buffer exists)
    HIPCHK(hipMalloc(p, c));
    *cap = c;
    return NFK_OK;
}

// stable LSD radix sort of packed words key << shift | index on the key's low `key_bits` bits
// (11-bit digits, a digit that every key shares is skipped): one array, 8 bytes per element and
// pass instead of a key and a value array
void radix_sort_packed(std::vector<uint64_t>& a, std::vector<uint64_t>& t, int shift, int key_bits) {
    const size_t n = a.size();
    if (n < 2) return;
    t.resize(n);
    uint32_t cnt[2048];
    for (int sh = shift; sh < shift + key_bits; sh += 11) {
        memset(cnt, 0, sizeof cnt);
        for (size_t i = 0; i < n; i++) cnt[(a[i] >> sh) & 2047]++;
        if (cnt[(a[0] >> sh) & 2047] == n) continue;
        uint32_t acc = 0;
        for (int b = 0; b < 2048; b++) {
            const uint32_t c = cnt[b];
            cnt[b] = acc;
            acc += c;
        }
        for (size_t i = 0; i < n; i++) t[cnt[(a[i] >> sh) & 2047]++] = a[i];
        a.swap(t);
    }
}
int bits_for(uint64_t x) { return x ? 64 - __builtin_clzll(x) : 1; }


// look_pin / look_dev (the device lookups' pinned and device staging) hold at least `bytes`
int look_reserve(World* w, size_t bytes) {
    if (bytes > w->look_pin_cap) {
        if (w->look_pin) HIPCHK(hipHostFree(w->look_pin));
        w->look_pin = nullptr;
        w->look_pin_cap = 0;
        HIPCHK(hipHostMalloc((void**)&w->look_pin, bytes + bytes / 2, hipHostMallocDefault));
        w->look_pin_cap = bytes + bytes / 2;
    }
    if (bytes > w->look_dev_cap) {
        if (w->look_dev) HIPCHK(hipFree(w->look_dev));
        w->look_dev = nullptr;
        w->look_dev_cap = 0;
        HIPCHK(hipMalloc(&w->look_dev, bytes + bytes / 2));
        w->look_dev_cap = bytes + bytes / 2;
    }
    return NFK_OK;
}

// Brings the device mirror of obj_of up to date on look_stream (the whole table after a rebuild,
// else the entries written since the last batch) and reserves the staging: the mirror's patch takes
// [0, *used) of look_pin / look_dev, the caller's batch (batch_bytes) follows.
int guid_mirror_update(World* w, size_t batch_bytes, size_t* used) {
    if (!w->look_stream) HIPCHK(hipStreamCreateWithFlags(&w->look_stream, hipStreamNonBlocking));
    using E = GuidMap::E;
    static_assert(sizeof(E) == sizeof(GuidEntry) && offsetof(E, v) == offsetof(GuidEntry, v), "mirror layout");
    const size_t cap = w->obj_of.capacity();
    const size_t tbytes = cap * sizeof(E);
    bool full = w->obj_of.take_rebuilt() || !w->guid_synced || w->guid_dmask != cap - 1;
    size_t np = full ? 0 : w->guid_log.size();
    if (np > cap / 8) {  // (many writes since: the whole table is the smaller upload)
        full = true;
        np = 0;
    }
    const size_t o_pi = 0, o_pe = align16(np * 4), u = align16(o_pe + np * sizeof(E));
    if (int r = look_reserve(w, u + batch_bytes)) return r;
    char* P = w->look_pin;
    char* D = (char*)w->look_dev;
    if (full) {
        if (tbytes > w->guid_dcap) {
            if (w->guid_d) HIPCHK(hipFree(w->guid_d));
            w->guid_d = nullptr;
            w->guid_dcap = 0;
            HIPCHK(hipMalloc(&w->guid_d, tbytes));
            w->guid_dcap = tbytes;
        }
        HIPCHK(hipMemcpyAsync(w->guid_d, w->obj_of.entries(), tbytes, hipMemcpyHostToDevice, w->look_stream));
        w->guid_dmask = cap - 1;
        w->guid_synced = true;
    } else if (np) {
        const E* t = w->obj_of.entries();
        uint32_t* pi = (uint32_t*)(P + o_pi);
        E* pe = (E*)(P + o_pe);
        for (size_t i = 0; i < np; i++) {  // (an entry logged twice is written twice with its final value)
            pi[i] = w->guid_log[i];
            pe[i] = t[w->guid_log[i]];
        }
        HIPCHK(hipMemcpyAsync(D, P, u, hipMemcpyHostToDevice, w->look_stream));
        hipLaunchKernelGGL(k_guid_patch, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, w->look_stream,
                           (GuidEntry*)w->guid_d, (const uint32_t*)(D + o_pi), (const GuidEntry*)(D + o_pe), (int32_t)np);
        HIPCHK(hipGetLastError());
    }
    w->guid_log.clear();
    *used = u;
    return NFK_OK;
}

// n lookups of a large batch on the device mirror of obj_of: one H2D copy of the GUIDs,
// k_guid_find, one D2H copy of the object indices
static bool trace_calls() {
    static const bool t = getenv("NFGPU_TRACE_CALLS") != nullptr;  // call batches' host phases to stderr
    return t;
}
static double ms_since(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
    return std::chrono::duration<double, std::milli>(b - a).count();
}

int find_many_dev(World* w, int32_t n, const int64_t* gh, const int64_t* gd, int32_t* out) {
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    const size_t cap = w->obj_of.capacity();
    if (cap == 0 || n <= 0) {
        for (int32_t i = 0; i < n; i++) out[i] = -1;
        return NFK_OK;
    }
    const size_t o_q = 0, o_r = align16((size_t)n * 16), tot = align16(o_r + (size_t)n * 4);
    size_t u = 0;
    if (int r = guid_mirror_update(w, tot, &u)) return r;
    char* P = w->look_pin + u;
    char* D = (char*)w->look_dev + u;
    memcpy(P + o_q, gh, (size_t)n * 8);
    memcpy(P + o_q + (size_t)n * 8, gd, (size_t)n * 8);
    const auto t1 = clk::now();
    HIPCHK(hipMemcpyAsync(D, P, o_r, hipMemcpyHostToDevice, w->look_stream));
    hipLaunchKernelGGL(k_guid_find, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, w->look_stream,
                       (const GuidEntry*)w->guid_d, (uint64_t)(cap - 1), (const int64_t*)(D + o_q), n,
                       (int32_t*)(D + o_r));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(P + o_r, D + o_r, (size_t)n * 4, hipMemcpyDeviceToHost, w->look_stream));
    const auto t2 = clk::now();
    HIPCHK(hipStreamSynchronize(w->look_stream));
    const auto t3 = clk::now();
    memcpy(out, P + o_r, (size_t)n * 4);
    if (trace_calls())
        fprintf(stderr, "find_many_dev n=%d: mirror+stage %.3f ms, enqueue %.3f ms, wait %.3f ms, copy-out %.3f ms\n", n,
                ms_since(t0, t1), ms_since(t1, t2), ms_since(t2, t3), ms_since(t3, clk::now()));
    return NFK_OK;
}

// the window's device queue of SetProperty calls (xq[xq_b]) holds at least `recs` records; grown
// on look_stream with its first xq_n records copied (the frame that last read the buffer is done:
// look_stream waited for xq_ev at the window's first device batch)
int xq_reserve(World* w, size_t recs) {
    const int b = w->xq_b;
    if (recs <= w->xq_cap[b]) return NFK_OK;
    const size_t c = std::max<size_t>({recs, w->xq_cap[b] + w->xq_cap[b] / 2, 65536});
    void* nb = nullptr;
    HIPCHK(hipMalloc(&nb, c * sizeof(World::XOp)));
    if (w->xq_n) HIPCHK(hipMemcpyAsync(nb, w->xq[b], w->xq_n * sizeof(World::XOp), hipMemcpyDeviceToDevice, w->look_stream));
    HIPCHK(hipStreamSynchronize(w->look_stream));
    if (w->xq[b]) HIPCHK(hipFree(w->xq[b]));
    w->xq[b] = nb;
    w->xq_cap[b] = c;
    return NFK_OK;
}

// the same at nfk_execute, on the world's stream (the host calls queued after the last device batch
// are appended there): a new buffer gets the device queue's calls, the old one is freed after
int xq_reserve_exec(World* w, size_t recs) {
    const int b = w->xq_b;
    if (recs <= w->xq_cap[b]) return NFK_OK;
    const size_t c = std::max<size_t>({recs, w->xq_cap[b] + w->xq_cap[b] / 2, 65536});
    void* nb = nullptr;
    HIPCHK(hipMalloc(&nb, c * sizeof(World::XOp)));
    HIPCHK(hipMemcpyAsync(nb, w->xq[b], w->xq_n * sizeof(World::XOp), hipMemcpyDeviceToDevice, w->stream));
    HIPCHK(hipStreamSynchronize(w->stream));
    HIPCHK(hipFree(w->xq[b]));
    w->xq[b] = nb;
    w->xq_cap[b] = c;
    return NFK_OK;
}

// A large batch of SetProperty* calls queued on the device (worlds without object properties):
// the lookups run on the device mirror and each call is written straight into the window's device
// queue (k_guid_queue), so the host touches the batch once, to stage it.  The host calls queued
// since the last device batch go in front of it (call order); a GUID that is no object rejects the
// whole batch, as nfk_set_props does.
int set_props_dev(World* w, int32_t n, const int64_t* gh, const int64_t* gd, const int32_t* pid, const uint64_t* bits) {
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    // the ids checked and the standalone calls counted without a branch per call (a batch's
    // properties follow no order a branch predictor learns: 3.4 ns per call with the branches on
    // the GPU boxes' hosts): one bit per property without a writable slot
    uint64_t nos[2] = {0, 0};
    for (int p = 0; p < w->n_if; p++)
        if (w->tab.w_slot[p] == kNoU) nos[p >> 6] |= 1ull << (p & 63);
    const uint32_t nif = (uint32_t)w->n_if;
    uint32_t bad = 0;
    int64_t sa = 0;
    uint64_t u0 = 0, u1 = 0;
    for (int32_t i = 0; i < n; i++) {
        const uint32_t p = (uint32_t)pid[i];
        bad |= (uint32_t)(p >= nif);
        const uint64_t bit = 1ull << (p & 63);
        const uint64_t hi = 0 - (uint64_t)((p >> 6) & 1);  // all ones for ids 64..127
        sa += (((nos[0] & ~hi) | (nos[1] & hi)) & bit) != 0;
        u0 |= bit & ~hi;
        u1 |= bit & hi;
    }
    if (bad)
        for (int32_t i = 0; i < n; i++)
            if (pid[i] < 0 || pid[i] >= w->n_if)
                return fail(NFK_ERR_ARG, pid[i] >= w->n_if && pid[i] < w->n_prop ? "object property: use nfk_set_objects"
                                                                                  : "bad property id");
    const uint64_t sp[2] = {u0 & nos[0], u1 & nos[1]};
    const auto t1 = clk::now();
    if (!w->look_stream) HIPCHK(hipStreamCreateWithFlags(&w->look_stream, hipStreamNonBlocking));
    const int b = w->xq_b;
    if (w->xq_n == 0 && w->xq_ev_set[b]) HIPCHK(hipStreamWaitEvent(w->look_stream, w->xq_ev[b], 0));
    const size_t tail = w->xops.size();
    if (int r = xq_reserve(w, w->xq_n + tail + (size_t)n)) return r;
    const size_t o_t = 0, o_b = align16(tail * sizeof(World::XOp)), o_p = align16(o_b + (size_t)n * 24),
                 o_m = align16(o_p + (size_t)n * 4), tot = o_m + 16;
    size_t u = 0;
    if (int r = guid_mirror_update(w, tot, &u)) return r;
    char* P = w->look_pin + u;
    char* D = (char*)w->look_dev + u;
    if (tail) memcpy(P + o_t, w->xops.data(), tail * sizeof(World::XOp));
    memcpy(P + o_b, gh, (size_t)n * 8);
    memcpy(P + o_b + (size_t)n * 8, gd, (size_t)n * 8);
    memcpy(P + o_b + (size_t)n * 16, bits, (size_t)n * 8);
    memcpy(P + o_p, pid, (size_t)n * 4);
    *(int32_t*)(P + o_m) = INT32_MAX;
    const auto t2 = clk::now();
    HIPCHK(hipMemcpyAsync(D, P, tot, hipMemcpyHostToDevice, w->look_stream));
    World::XOp* q = (World::XOp*)w->xq[b] + w->xq_n;
    if (tail) HIPCHK(hipMemcpyAsync(q, D + o_t, tail * sizeof(World::XOp), hipMemcpyDeviceToDevice, w->look_stream));
    hipLaunchKernelGGL(k_guid_queue, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, w->look_stream,
                       (const GuidEntry*)w->guid_d, (uint64_t)(w->obj_of.capacity() - 1), (const int64_t*)(D + o_b),
                       (const int32_t*)(D + o_p), n, (XCall*)(q + tail), (int32_t*)(D + o_m));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(P + o_m, D + o_m, 4, hipMemcpyDeviceToHost, w->look_stream));
    const auto t3 = clk::now();
    HIPCHK(hipStreamSynchronize(w->look_stream));
    if (trace_calls())
        fprintf(stderr, "set_props_dev n=%d: validate %.3f ms, mirror+reserve+stage %.3f ms, enqueue %.3f ms, wait %.3f ms\n",
                n, ms_since(t0, t1), ms_since(t1, t2), ms_since(t2, t3), ms_since(t3, clk::now()));
    const int32_t miss = *(const int32_t*)(P + o_m);
    if (miss >= 0 && miss < n)  // NFCKernelModule logs "There is no object" and returns false (KM:331)
        return fail(NFK_ERR_NOTFOUND, "no object " + std::to_string(gh[miss]) + "-" + std::to_string(gd[miss]));
    w->xq_n += tail + (size_t)n;
    w->xops.clear();
    w->ov_last.clear();  // (the overlay index is rebuilt from the whole queue at the next read)
    w->ov_prev.clear();
    w->sa_calls += sa;
    w->sa_pids[0] |= sp[0];
    w->sa_pids[1] |= sp[1];
    return NFK_OK;
}

// the window's device queue back in the host xops, in front of the calls queued after it (a read
// of queued values — GetProperty* — needs them all on the host)
int pull_device_queue(World* w) {
    if (!w->xq_n) return NFK_OK;
    std::vector<World::XOp> dq(w->xq_n);
    HIPCHK(hipMemcpy(dq.data(), w->xq[w->xq_b], w->xq_n * sizeof(World::XOp), hipMemcpyDeviceToHost));
    w->xops.insert(w->xops.begin(), dq.begin(), dq.end());
    w->xq_n = 0;
    w->ov_last.clear();
    w->ov_prev.clear();
    return NFK_OK;
}

// A batch's lookups: on the device from dev_look_min calls on, else GuidMap::find_many (split
// over the host pool for a large batch when the pool has workers)
int find_many_par(World* w, int32_t n, const int64_t* gh, const int64_t* gd, int32_t* out) {
    if (w->dev_look_min && (size_t)n >= w->dev_look_min) return find_many_dev(w, n, gh, gd, out);
    if (w->guid_log.size() > w->obj_of.capacity() / 8) {  // (the mirror is rewritten at its next use)
        w->guid_log.clear();
        w->guid_synced = false;
    }
    if ((size_t)n < w->par_calls || w->pool->threads() < 2) {
        w->obj_of.find_many(n, gh, gd, out);
        return NFK_OK;
    }
    const int P = w->pool->threads();
    w->pool->run(P, [&](int c) {
        const int32_t a = (int32_t)((int64_t)n * c / P), b = (int32_t)((int64_t)n * (c + 1) / P);
        w->obj_of.find_many(b - a, gh + a, gd + a, out + a);
    });
    return NFK_OK;
}


// replace a tracked device allocation by a bigger one (contents dropped)
int regrow(World* w, void** p, size_t bytes) {
    if (*p) {
        HIPCHK(hipFree(*p));
        w->allocs.erase(std::remove(w->allocs.begin(), w->allocs.end(), *p), w->allocs.end());
        *p = nullptr;
    }
    return alloc_track(w, p, bytes);
}

// the property-event tiles with room for `per_tile` events each (a frame with many standalone
// SetProperty groups in one tile); the previous frame's events are dropped
int grow_event_tiles(World* w, int64_t per_tile) {
    Dev& d = w->d;
    const int64_t tcap = (per_tile + kTile - 1) / kTile * kTile;
    if (tcap > 0xFFFF) return fail(NFK_ERR_CAPACITY, "more than 65535 property events in one 256-slot tile");
    HIPCHK(hipStreamSynchronize(w->stream));
    const size_t n = (size_t)(d.cap / kTile) * (size_t)tcap;
    int r;
    if ((r = regrow(w, (void**)&d.ev_slot, n * 4)) || (r = regrow(w, (void**)&d.ev_pid, n * 4)) ||
        (r = regrow(w, (void**)&d.ev_old, n * 8)) || (r = regrow(w, (void**)&d.ev_new, n * 8)) ||
        (r = regrow(w, (void**)&d.ev_moff, n * 4)) ||
        (d.n_obj && ((r = regrow(w, (void**)&d.ev_old_h, n * 8)) || (r = regrow(w, (void**)&d.ev_new_h, n * 8))))) {
        d.ev_tcap = 0;
        return r;
    }
    d.ev_tcap = (int32_t)tcap;
    w->scan_pending = false;
    return NFK_OK;
}

// the record-event tiles grown for a frame whose SetRecord groups add events beside the record
// programs' (contents dropped: called before the frame writes them)
int grow_rec_tiles(World* w, int64_t per_tile) {
    Dev& d = w->d;
    const int64_t tcap = (per_tile + 63) / 64 * 64;
    if (tcap > INT32_MAX / 2) return fail(NFK_ERR_CAPACITY, "too many record events in one record tile");
    HIPCHK(hipStreamSynchronize(w->stream));
    const size_t n = (size_t)(d.cap / kRTile) * (size_t)tcap;
    int r;
    if ((r = regrow(w, (void**)&d.re_rrc, n * 4)) ||
        (r = regrow(w, (void**)&d.re_old, n * 8)) || (r = regrow(w, (void**)&d.re_new, n * 8)) ||
        (r = regrow(w, (void**)&d.re_moff, n * 4)) ||
        (w->rec_obj && ((r = regrow(w, (void**)&w->re_old_h, n * 8)) || (r = regrow(w, (void**)&w->re_new_h, n * 8))))) {
        d.re_tcap = 0;
        return r;
    }
    d.re_tcap = (int32_t)tcap;
    w->scan_pending = false;
    return NFK_OK;
}

// the property ops (a program's Get + Set on a property column; record ops run in k_records)
static bool prop_op(int code) {
    return code == NFK_OP_IADD_CLAMP || code == NFK_OP_FLERP || code == NFK_OP_FAFFINE || code == NFK_OP_ISET ||
           code == NFK_OP_FSET;
}

// The programs' working set: program destinations -> writable U slots [0, n_w) and the operands
// programs only read -> slots [n_w, n_u), each group in property-id order; the tables name
// read-only operand r as 0x80 | r.  Fills the kinds' U-slot tables (opu, umask, opx, w_slot);
// false when the set does not fit k_tick's register slots (k_tick_touch runs instead).
bool build_u_tables(Tables& tab, int NK, std::vector<int>& wp, std::vector<int>& rp) {
    bool u_ok = false;
    {
        std::vector<int> W, R;
        for (int k = 0; k < NK; k++)
            for (int i = 0; i < tab.nops[k]; i++) {
                const nfk_op& op = tab.ops[k][i];
                if (prop_op(op.code)) W.push_back(op.dst);
            }
        std::sort(W.begin(), W.end());
        W.erase(std::unique(W.begin(), W.end()), W.end());
        auto is_w = [&](int64_t p) { return std::binary_search(W.begin(), W.end(), (int)p); };
        for (int k = 0; k < NK; k++)
            for (int i = 0; i < tab.nops[k]; i++) {
                const nfk_op& op = tab.ops[k][i];
                if (op.code == NFK_OP_IADD_CLAMP) {
                    if ((op.flags & NFK_A_PROP) && !is_w(op.a)) R.push_back((int)op.a);
                    if ((op.flags & NFK_LO_PROP) && !is_w(op.b)) R.push_back((int)op.b);
                    if ((op.flags & NFK_HI_PROP) && !is_w(op.c)) R.push_back((int)op.c);
                } else if (op.code == NFK_OP_FLERP && !is_w(op.a)) {
                    R.push_back((int)op.a);
                } else if ((op.code == NFK_OP_ISET || op.code == NFK_OP_FSET) && (op.flags & NFK_A_PROP) && !is_w(op.a)) {
                    R.push_back((int)op.a);
                }
                // (a guard cell, NFK_GUARD_CELL: its pseudo-id, behind every property; never writable)
                if ((op.flags & NFK_GUARD) && !is_w(guard_id(op))) R.push_back(guard_id(op));
                if ((op.flags & NFK_GUARD) && (op.guard & NFK_GUARD_PROP) && !is_w(op.guard >> 19))
                    R.push_back((int)(op.guard >> 19));
            }
        std::sort(R.begin(), R.end());
        R.erase(std::unique(R.begin(), R.end()), R.end());
        u_ok = (int)W.size() <= kMaxW && (int)(W.size() + R.size()) <= kMaxU;
        wp.assign(W.begin(), W.end());
        rp.assign(R.begin(), R.end());
        memset(tab.w_slot, kNoU, sizeof tab.w_slot);
        for (size_t i = 0; i < W.size() && i < (size_t)kMaxW; i++) tab.w_slot[W[i]] = (uint8_t)i;
        auto slot = [&](int64_t p) -> uint8_t {
            auto it = std::lower_bound(W.begin(), W.end(), (int)p);
            if (it != W.end() && *it == p) return (uint8_t)(it - W.begin());
            it = std::lower_bound(R.begin(), R.end(), (int)p);
            return (uint8_t)(0x80 | (it - R.begin()));
        };
        for (int k = 0; k < NK && u_ok; k++) {
            tab.umask[k] = 0;
            for (int i = 0; i < tab.nops[k]; i++) {
                const nfk_op& op = tab.ops[k][i];
                uint8_t* u = tab.opu[k][i];
                u[0] = u[1] = u[2] = u[3] = kNoU;
                if (op.code == NFK_OP_IADD_CLAMP) {
                    u[0] = slot(op.dst);
                    if (op.flags & NFK_A_PROP) u[1] = slot(op.a);
                    if (op.flags & NFK_LO_PROP) u[2] = slot(op.b);
                    if (op.flags & NFK_HI_PROP) u[3] = slot(op.c);
                } else if (op.code == NFK_OP_FLERP) {
                    u[0] = slot(op.dst);
                    u[1] = slot(op.a);
                } else if (op.code == NFK_OP_FAFFINE) {
                    u[0] = slot(op.dst);
                } else if (op.code == NFK_OP_ISET || op.code == NFK_OP_FSET) {
                    u[0] = slot(op.dst);
                    if (op.flags & NFK_A_PROP) u[1] = slot(op.a);
                }
                tab.opg[k][i] = (op.flags & NFK_GUARD) ? slot(guard_id(op)) : kNoU;
                tab.opg2[k][i] = ((op.flags & NFK_GUARD) && (op.guard & NFK_GUARD_PROP)) ? slot(op.guard >> 19) : kNoU;
                for (int q = 0; q < 6; q++) {  // writable bits | read-only bits << 16
                    const uint8_t uq = q < 4 ? u[q] : q == 4 ? tab.opg[k][i] : tab.opg2[k][i];
                    if (uq != kNoU) tab.umask[k] |= (uq & 0x80) ? 1u << (16 + (uq & 0x7F)) : 1u << uq;
                }
                OpX& x = tab.opx[k][i];
                x.cfd = (uint32_t)op.code | ((uint32_t)op.flags << 8) | ((uint32_t)op.dst << 16);
                x.slots = (uint32_t)u[0] | ((uint32_t)u[1] << 8) | ((uint32_t)u[2] << 16) | ((uint32_t)u[3] << 24);
                if (op.code == NFK_OP_RIADD_CLAMP) {
                    // a record op has no U slots: the word holds the read-only indices of the guard
                    // cells on its column, which take the op in the walk (run_programs_u)
                    x.slots = 0;
                    for (size_t r = 0; r < R.size(); r++)
                        if (R[r] >= kCellPid && (cell_rec((uint32_t)R[r]) << 8 | cell_col((uint32_t)R[r])) == op.dst)
                            x.slots |= 1u << r;
                }
                x.a = op.a;
                x.b = op.b;
                x.c = op.c;
                x.gd = (op.flags & NFK_GUARD) ? 0x80000000u | (((op.guard >> 16) & 3u) << 8) | tab.opg[k][i] : 0u;
                if (tab.opg2[k][i] != kNoU) x.gd |= 0x40000000u | ((uint32_t)tab.opg2[k][i] << 16);
                else if (op.flags & NFK_GUARD) x.gd |= ((op.guard >> 19) & 0x1FFFu) << 16;  // NFK_GUARD_K
            }
        }
    }
    return u_ok;
}

// Dev::u_* from the working set: slot properties, event order and fan-out classes of the
// writable slots (all read by k_tick as scalars); columns only once the world has property memory
void fill_u_dev(Dev& d, const Tables& tab, const std::vector<int>& wp, const std::vector<int>& rp, bool u_ok) {
    const int n_w = (int)wp.size(), n_r = (int)rp.size();
    for (int j = 0; j < kMaxU; j++) d.u_pid[j] = -1;
    d.n_w = d.n_u = 0;
    if (!u_ok) return;
    for (int i = 0; i < n_w; i++) d.u_pid[i] = wp[i];
    for (int i = 0; i < n_r; i++) d.u_pid[n_w + i] = rp[i];
    d.n_w = n_w;
    d.n_u = n_w + n_r;
    for (int i = 0; i < kMaxW; i++) d.u_order[i] = i < n_w ? i : 0;  // (wp is in property-id order)
    for (int j = 0; j < kMaxU; j++) {
        const int p = d.u_pid[j];
        if (p >= kCellPid) {  // a guard cell: its record's cells, cols x rows per entity
            const uint32_t r = cell_rec((uint32_t)p);
            d.u_col[j] = d.rcells[r];
            d.u_str[j] = tab.rec_rows[r] * tab.rec_cols[r];
            continue;
        }
        d.u_col[j] = (p < 0 || !d.pmem) ? nullptr : d.pmem + tab.p_off[p];
        d.u_str[j] = p < 0 ? 0 : tab.p_str[p];
    }
    for (int j = 0; j < kMaxW; j++) {
        d.u_lower[j] = 0;
        for (int i = 0; i < n_w && j < n_w; i++)
            if (d.u_pid[i] < d.u_pid[j]) d.u_lower[j] |= 1u << i;
    }
    for (int c = 0; c < NFK_MAX_CLASSES; c++) {
        uint32_t pub = 0, priv = 0;
        for (int j = 0; j < n_w && c != 15; j++) {  // (class 15 marks a free slot)
            const uint8_t f = tab.pflags[c][d.u_pid[j]];
            if (f & NFK_PUBLIC) pub |= 1u << j;
            else if ((f & NFK_PRIVATE) && !(f & NFK_UPLOAD)) priv |= 1u << j;
        }
        d.u_cmask[c] = pub | (priv << 16);
    }
}

void set_working_set(World* w) { fill_u_dev(w->d, w->tab, w->u_wp, w->u_rp, w->u_ok); }

// waves per SIMD k_tick's register budget aims at, by the working set's size
int tick_waves(int n_u, uint32_t ablate) {
    if (n_u <= 8) return kWavesU8;
    if (n_u <= 12) return (ablate & kAblWaves8) ? 8 : kWavesU12;
    return 6;
}

// the non-temporal hints the specialised k_tick is built with (A/B: NFGPU_JIT_NT): the schedule
// records / descriptor loads and the fan-out's LDS-window recipient stores stream past the caches
// (config[1]: 90 vs 115 us with none, 102 with the fan-out stores alone; event-array stores
// non-temporal run 160 us; profiles/r07a_ntab.txt).  Not the lane-group recipient stores
// (kNtFanGroupStore: config[3] 377 vs 415 us, config[4] 94 vs 107 us; profiles/r08i_*)
constexpr uint32_t kJitNtDefault = kNtSchedLoad | kNtFanStore;

// What the hipRTC build of a world's k_tick is made with, from the environment and the world (d: its
// Dev once committed; nfk_jit_preview's has no record ops and no NFGPU_ABLATE).
struct JitOptions {
    int waves;    // waves per SIMD of the register budget
    uint32_t nt;  // non-temporal hints (kNt* bits of nfgpu_tick.hpp)
    bool lb;      // the rank workgroups' code compiled in
};
JitOptions jit_options(const Dev& d) {
    JitOptions o;
    // The specialised kernel gets the register budget of 5 waves per SIMD (round 4: no spills, and
    // the fan-out's LDS window grows with the budget): config[1] 82.7-83.7 vs 83.7-84.1 us at 6
    // (12 VGPRs spilled), 97 at 7, 122 at 8; config[3] 342-344 vs 347-348 us
    // (profiles/r11j_jit_waves_ab.txt; round 2's r02t_ab_waves.txt chose 6 over 7).
    o.waves = (d.ablate & kAblWaves8) ? tick_waves(d.n_u, d.ablate) : kWavesJit;
    if (const char* ew = getenv("NFGPU_JIT_WAVES")) o.waves = std::max(1, std::min(8, atoi(ew)));
    // NFGPU_JIT_NT overrides the default hints
    o.nt = kJitNtDefault;
    if (const char* en = getenv("NFGPU_JIT_NT")) o.nt = (uint32_t)strtoul(en, nullptr, 0);
    // a world whose frames never rank in k_tick (record ops: their counts come from k_records too; dense
    // ranks by k_scan_tiles asked for with kAblScanKernel) has that code compiled out of its
    // specialisation (NFGPU_JIT_LB=0 / 1 overrides, for A/B; Dev::lb_rank is decided per frame)
    o.lb = !d.has_recops && !(d.ablate & kAblScanKernel);
    if (const char* el = getenv("NFGPU_JIT_LB")) o.lb = el[0] == '1';
    return o;
}

// Specialised k_tick kernels built in this process, by (device, variant, policy source): a
// schema compiles once however many worlds use it.
std::mutex g_jit_mu;
std::map<std::string, std::pair<hipFunction_t, hipFunction_t>> g_jit;  // (k_tick, k_chain_u)

void build_jit(World* w) {
    w->jit_fn = nullptr;
    w->jit_chain_fn = nullptr;
    const char* env = getenv("NFGPU_JIT");
    if (env && env[0] == '0') {
        w->jit_msg = "disabled (NFGPU_JIT=0)";
        return;
    }
    if (!w->u_ok) {
        w->jit_msg = "working set does not fit k_tick (k_tick_touch runs)";
        return;
    }
    const int u = std::max(w->d.n_u, 1);
    const JitOptions jo = jit_options(w->d);
    const int waves = jo.waves;
    const bool lb = jo.lb;
    const std::string src = jit_schema_source(w->tab, w->d, jo.nt, lb);
    int dev = 0;
    (void)hipGetDevice(&dev);
    const std::string key = std::to_string(dev) + "|" + std::to_string(waves) + "|" + std::to_string(u) + "|" + src;
    std::lock_guard<std::mutex> lk(g_jit_mu);
    auto it = g_jit.find(key);
    if (it == g_jit.end()) {
        JitBuild b = jit_compile(src, waves, u);
        hipModule_t mod = nullptr;
        hipFunction_t fn = nullptr, cfn = nullptr;
        if (!b.ok || hipModuleLoadData(&mod, b.code.data()) != hipSuccess ||
            hipModuleGetFunction(&fn, mod, b.lowered.c_str()) != hipSuccess ||
            hipModuleGetFunction(&cfn, mod, b.lowered_chain.c_str()) != hipSuccess) {
            w->jit_msg = "hipRTC build failed: " + b.log.substr(0, 2000);
            return;
        }
        it = g_jit.emplace(key, std::make_pair(fn, cfn)).first;
    }
    w->jit_fn = it->second.first;
    w->jit_chain_fn = it->second.second;
    w->jit_lb = lb;
    w->jit_waves = waves;
    w->jit_u = u;
    w->jit_msg = jit_kernel_name(waves, u);
}

// w->mhost -> w->mlist, asynchronously on the world's stream (through a pinned double buffer:
// a buffer is refilled only once the copy from it two uploads ago has completed)
int upload_mhost(World* w) {
    int r = dev_reserve(w, &w->mlist, &w->mlist_cap, w->mhost.size() + 16);
    if (r) return r;
    const int s = w->mpin_slot;
    w->mpin_slot ^= 1;
    if (w->mpin_pending[s]) {
        HIPCHK(hipEventSynchronize(w->mpin_done[s]));
        w->mpin_pending[s] = false;
    }
    if (w->mhost.size() > w->mpin_cap[s]) {
        if (w->mpin[s]) HIPCHK(hipHostFree(w->mpin[s]));
        w->mpin[s] = nullptr;
        const size_t c = std::max(w->mhost.size(), 2 * w->mpin_cap[s]);
        w->mpin_cap[s] = 0;  // (until the new buffer exists)
        HIPCHK(hipHostMalloc((void**)&w->mpin[s], c, hipHostMallocDefault));
        w->mpin_cap[s] = c;
    }
    if (w->mhost.empty()) return NFK_OK;
    memcpy(w->mpin[s], w->mhost.data(), w->mhost.size());
    HIPCHK(hipMemcpyAsync(w->mlist, w->mpin[s], w->mhost.size(), hipMemcpyHostToDevice, w->stream));
    HIPCHK(hipEventRecord(w->mpin_done[s], w->stream));
    w->mpin_pending[s] = true;
    return NFK_OK;
}

template <typename T>
size_t stage_list(World* w, const std::vector<T>& v) {
    const size_t off = align16(w->mhost.size());
    w->mhost.resize(off + v.size() * sizeof(T));
    if (!v.empty()) memcpy(w->mhost.data() + off, v.data(), v.size() * sizeof(T));
    return off;
}

unsigned grid_for(size_t work) { return (unsigned)std::max<size_t>(1, std::min<size_t>((work + kTPB - 1) / kTPB, 8192)); }

// per affected segment: its new member list, the old ranks its leavers had and its joiners
// with their new ranks (ins, sorted by rank)
struct EdInfo {
    World::Seg seg;
    std::vector<int32_t> rem, join;
    std::vector<std::pair<int32_t, int32_t>> ins;  // (new rank, object)
};

// A window's membership changes, planned on the host (plan_membership: the new member lists and
// the device's edit / move plans; it changes nothing of the world) and then applied
// (commit_membership: uploads and launches, then the host maps while the device rewrites the
// slots).  nfk_execute plans while the previous frame still runs on the GPU and waits for that
// frame before the commit, which rewrites slots the previous frame's fan-out recovery
// (regrow_fanout) reads.
struct MemPlan {
    bool active = false, full = false;
    int32_t max_np0 = 0;
    std::vector<int32_t> aff, epos;
    // einfo[0, n_einfo): this plan's affected segments; the entries (and their lists' buffers)
    // are kept from plan to plan, so a window's edits allocate nothing once they have been seen
    std::vector<EdInfo> einfo;
    size_t n_einfo = 0;
    std::vector<SegEdit> edits;
    std::vector<int32_t> ins_rank, ins_obj, rem_rank;
    std::vector<uint64_t> ins_meta;
    std::vector<int64_t> ins_src;
    std::vector<SegMove> moves;
    std::vector<World::Seg> nsegs;  // full: the new segment table
    std::vector<int32_t> nsrc;      // full: nsegs[i] is untouched segment nsrc[i] (members kept), or -1
    int32_t mv_rows_dev = 0, mv_list_dev = 0, ed_rows = 0, ed_list = 0;
    std::chrono::steady_clock::time_point t_host, t_edit, t_lists;
    std::chrono::steady_clock::time_point t_leave, t_join;  // (trace) the edit phase's parts
};

// Apply this window's membership changes (SwitchScene across groups, DestroyObject, exports,
// imports) before the frame: only the scene-group segments that changed are rewritten (the
// entities behind the first change shift by one slot each); a new (scene, group) or a segment
// whose slack ran out rebuilds the whole layout.
int plan_membership(World* w, MemPlan& p) {
    p.active = false;
    if (w->touched.empty()) return NFK_OK;
    using clk = std::chrono::steady_clock;
    p.t_host = clk::now();
    p.full = false;
    p.aff.clear();
    p.n_einfo = 0;
    p.edits.clear();
    p.ins_rank.clear();
    p.ins_obj.clear();
    p.rem_rank.clear();
    p.ins_meta.clear();
    p.ins_src.clear();
    p.moves.clear();
    p.mv_rows_dev = p.mv_list_dev = p.ed_rows = p.ed_list = 0;
    p.nsegs.clear();
    p.nsrc.clear();
    Dev& d = w->d;
    const auto cmp = [w](int32_t a, int32_t b) { return guid_less(w, a, b); };
    // The new member lists are built on copies of the affected segments; nothing of the world
    // changes before every check has passed (a failure leaves the window's calls queued).
    bool& full = p.full;
    std::vector<int32_t>& aff = p.aff;  // affected segments, in first-touch order
    auto seg_at = [&](int32_t slot) {
        int32_t lo = 0, hi = (int32_t)w->segs.size() - 1;
        while (lo < hi) {
            const int32_t mid = (lo + hi + 1) / 2;
            if (w->segs[mid].base <= slot) lo = mid;
            else hi = mid - 1;
        }
        return lo;
    };
    std::vector<int32_t>& epos = p.epos;
    epos.assign(w->segs.size(), -1);
    std::vector<EdInfo>& einfo = p.einfo;
    einfo.reserve(2 * w->touched.size() + 1);
    auto ed = [&](int32_t g) -> EdInfo& {
        if (epos[g] < 0) {
            if (p.n_einfo == einfo.size()) einfo.emplace_back();
            EdInfo& x = einfo[p.n_einfo];
            x.rem.clear();
            x.join.clear();
            x.ins.clear();
            x.seg.objs.clear();
            x.seg.keys.clear();
            epos[g] = (int32_t)p.n_einfo++;
            aff.push_back(g);
        }
        return einfo[epos[g]];
    };
    for (int32_t o : w->touched) {
        const int32_t s = w->slot_of_obj[o];
        if (s < 0) continue;
        const int32_t gi = seg_at(s);
        ed(gi).rem.push_back(s - w->segs[gi].base);  // members occupy [base, base + n) in NFGUID order
    }
    p.t_leave = clk::now();
    for (int32_t o : w->touched) {
        if (!w->alive[o]) continue;
        const int32_t gi = find_seg(w, w->scene[o], w->group[o]);
        if (gi < 0) {
            full = true;
            continue;
        }
        ed(gi).join.push_back(o);
    }
    p.t_join = clk::now();
    // each new member list in one pass: the old list without its leavers (known by rank, no
    // NFGUID comparison), the joiners (sorted) spliced in at their binary-searched places
    for (int32_t g : aff) {
        EdInfo& x = einfo[epos[g]];
        const World::Seg& old = w->segs[g];
        x.seg.scene = old.scene;
        x.seg.group = old.group;
        x.seg.base = old.base;
        x.seg.cap = old.cap;
        x.seg.np = old.np;
        std::sort(x.rem.begin(), x.rem.end());
        std::sort(x.join.begin(), x.join.end(), cmp);
        std::vector<int32_t>& v = x.seg.objs;
        std::vector<World::Guid>& kv = x.seg.keys;
        v.reserve(old.objs.size() - x.rem.size() + x.join.size());
        kv.reserve(v.capacity());
        // (a joiner's place is searched in the old list, leavers included: they are still in
        // NFGUID order, and one that rejoins compares equal to itself and is skipped below)
        size_t r = 0, at = 0;
        auto copy_to = [&](size_t p) {  // old ranks [at, p) without the leavers, as runs (memcpy-speed copies)
            while (at < p) {
                if (r < x.rem.size() && x.rem[r] == (int32_t)at) {
                    r++;
                    at++;
                    continue;
                }
                const size_t e = (r < x.rem.size() && (size_t)x.rem[r] < p) ? (size_t)x.rem[r] : p;
                v.insert(v.end(), old.objs.begin() + (std::ptrdiff_t)at, old.objs.begin() + (std::ptrdiff_t)e);
                kv.insert(kv.end(), old.keys.begin() + (std::ptrdiff_t)at, old.keys.begin() + (std::ptrdiff_t)e);
                at = e;
            }
        };
        const auto key_less = [](const World::Guid& a, const World::Guid& b) { return a.h != b.h ? a.h < b.h : a.d < b.d; };
        for (int32_t o : x.join) {
            const World::Guid go = w->guid[o];
            copy_to((size_t)(std::lower_bound(old.keys.begin() + at, old.keys.end(), go, key_less) - old.keys.begin()));
            x.ins.push_back({(int32_t)v.size(), o});
            v.push_back(o);
            kv.push_back(go);
        }
        copy_to(old.objs.size());
        if ((int32_t)v.size() > old.cap) full = true;
    }
    // edited and new segments: their slot lists are generated on the device (k_seg_edit) from the
    // removed ranks and the inserted objects at their new ranks
    std::vector<SegEdit>& edits = p.edits;
    std::vector<int32_t>&ins_rank = p.ins_rank, &ins_obj = p.ins_obj, &rem_rank = p.rem_rank;
    std::vector<uint64_t>& ins_meta = p.ins_meta;
    std::vector<int64_t>& ins_src = p.ins_src;
    int32_t &ed_rows = p.ed_rows, &ed_list = p.ed_list;
    // ob: the old segment (-1: a new (scene, group) pair; its members are all inserted)
    auto add_edit = [&](World::Seg& g, int32_t ob_seg, const std::vector<std::pair<int32_t, int32_t>>* ins,
                        const std::vector<int32_t>* rem, bool all) -> int {
        SegEdit e{};
        const World::Seg* old = ob_seg >= 0 ? &w->segs[ob_seg] : nullptr;
        e.ob = old ? old->base : -1;
        e.nb = g.base;
        e.on = old ? (int32_t)old->objs.size() : 0;
        e.nn = (int32_t)g.objs.size();
        e.nc = g.cap;
        int32_t np = old ? old->np : 0;
        e.io = (int32_t)ins_rank.size();
        if (ins) {  // (new rank, object), in rank order
            for (const auto& x : *ins) {
                const int32_t o = x.second;
                np += w->isplayer[o] ? 1 : 0;
                ins_rank.push_back(x.first);
                ins_obj.push_back(o);
                ins_meta.push_back(((uint64_t)w->cls[o] << 60) | (w->isplayer[o] ? 1u : 0u));
                ins_src.push_back(w->src_row[o] >= 0 ? -1 - w->src_row[o] : (int64_t)w->slot_of_obj[o]);
            }
        }
        e.ni = (int32_t)ins_rank.size() - e.io;
        e.ro = (int32_t)rem_rank.size();
        if (rem) {
            const size_t r0 = rem_rank.size();
            for (int32_t rk : *rem) {
                rem_rank.push_back(rk);
                np -= w->isplayer[old->objs[rk]] ? 1 : 0;
            }
            std::sort(rem_rank.begin() + r0, rem_rank.end());
        }
        e.nr = (int32_t)rem_rank.size() - e.ro;
        if (np > 0x3FFF) return fail(NFK_ERR_ARG, "more than 16383 players in one scene group");
        e.np = np;
        e.all = all ? 1 : 0;
        g.np = np;
        w->max_np = std::max(w->max_np, np);
        edits.push_back(e);
        return NFK_OK;
    };
    std::vector<World::Seg>& nsegs = p.nsegs;
    std::vector<int32_t>& nsrc = p.nsrc;
    std::vector<int32_t> nold;   // full: nsegs[i] is edited segment nold[i], or -1 (untouched / new)
    std::vector<SegMove>& moves = p.moves;  // full: untouched segments whose slot range changes
    int32_t &mv_rows_dev = p.mv_rows_dev, &mv_list_dev = p.mv_list_dev;
    const int32_t max_np0 = p.max_np0 = w->max_np;
    p.t_edit = clk::now();
    if (full) {
        // The (scene, group)-ordered segment table is rebuilt from the member lists: untouched
        // segments keep theirs, edited ones take their edit copies, the objects of new (scene,
        // group) pairs form new NFGUID-sorted segments, empty segments are dropped, and every
        // segment gets a fresh base and slack.  Nothing of the world is sorted — the result is
        // the layout a sort of every live object by (scene, group, NFGUID) would give.  The slot
        // lists of edited and new segments are built here; those of the untouched segments (the
        // bulk of the world) are generated on the device from their old and new ranges.
        std::map<std::pair<int32_t, int32_t>, std::vector<int32_t>> fresh;
        for (int32_t o : w->touched)
            if (w->alive[o] && find_seg(w, w->scene[o], w->group[o]) < 0)
                fresh[{w->scene[o], w->group[o]}].push_back(o);
        for (auto& f : fresh) std::sort(f.second.begin(), f.second.end(), cmp);
        auto fit = fresh.begin();
        auto push_fresh = [&]() {
            World::Seg g;
            g.scene = fit->first.first;
            g.group = fit->first.second;
            g.objs = std::move(fit->second);
            g.keys.resize(g.objs.size());
            for (size_t k = 0; k < g.objs.size(); k++) g.keys[k] = w->guid[g.objs[k]];
            nsegs.push_back(std::move(g));
            nsrc.push_back(-1);
            nold.push_back(-1);
            ++fit;
        };
        for (int32_t gi = 0; gi < (int32_t)w->segs.size(); gi++) {
            const World::Seg& old = w->segs[gi];
            const std::pair<int32_t, int32_t> key{old.scene, old.group};
            while (fit != fresh.end() && fit->first < key) push_fresh();
            const bool edited = epos[gi] >= 0;
            if ((edited ? einfo[epos[gi]].seg.objs : old.objs).empty()) {
                // (the group stays for the scene queries: NFCSceneGroupInfo until ReleaseGroupScene)
                w->known_scenes.insert(old.scene);
                w->known_groups.insert(seg_key_of(old.scene, old.group));
                continue;
            }
            World::Seg g;
            g.scene = old.scene;
            g.group = old.group;
            if (edited) {
                g.objs = std::move(einfo[epos[gi]].seg.objs);
                g.keys = std::move(einfo[epos[gi]].seg.keys);
            }
            nsegs.push_back(std::move(g));
            nsrc.push_back(edited ? -1 : gi);
            nold.push_back(edited ? gi : -1);
        }
        while (fit != fresh.end()) push_fresh();
        auto members = [&](size_t i) -> const std::vector<int32_t>& {
            return nsrc[i] >= 0 ? w->segs[nsrc[i]].objs : nsegs[i].objs;
        };
        auto assign = [&](int32_t sl) {
            int64_t base = 0;
            for (size_t i = 0; i < nsegs.size(); i++) {
                const int32_t n = (int32_t)members(i).size();
                nsegs[i].base = (int32_t)std::min<int64_t>(base, INT32_MAX);
                nsegs[i].cap = n + seg_slack(sl, n);
                base += nsegs[i].cap;
            }
            return base;
        };
        int64_t total = assign(w->slack);
        if (total > d.cap) total = assign(0);
        if (total > d.cap) return fail(NFK_ERR_CAPACITY, "entity capacity exceeded (nothing of the window applied)");
        w->max_np = 0;  // recomputed over every segment below
        for (size_t i = 0; i < nsegs.size(); i++) {
            World::Seg& g = nsegs[i];
            if (nsrc[i] >= 0) {
                const World::Seg& old = w->segs[nsrc[i]];
                g.np = old.np;
                w->max_np = std::max(w->max_np, g.np);
                if (old.base == g.base && old.cap == g.cap) continue;  // stays where it is
                moves.push_back({old.base, g.base, (int32_t)old.objs.size(), g.cap, old.np, mv_rows_dev, mv_list_dev, 0});
                mv_rows_dev += (int32_t)old.objs.size();
                mv_list_dev += g.cap;
                continue;
            }
            int r;
            if (nold[i] >= 0) {
                const EdInfo& x = einfo[epos[nold[i]]];
                r = add_edit(g, nold[i], &x.ins, &x.rem, true);
            } else {  // a new (scene, group) pair: every member joins, at its rank
                std::vector<std::pair<int32_t, int32_t>> all_in(g.objs.size());
                for (size_t k = 0; k < g.objs.size(); k++) all_in[k] = {(int32_t)k, g.objs[k]};
                r = add_edit(g, -1, &all_in, nullptr, true);
            }
            if (r) {
                w->max_np = max_np0;
                return r;
            }
        }
    } else {
        for (int32_t gi : aff) {
            EdInfo& x = einfo[epos[gi]];
            int r = add_edit(x.seg, gi, &x.ins, &x.rem, false);
            if (r) {
                w->max_np = max_np0;
                return r;
            }
        }
    }
    for (SegEdit& e : edits) {  // their lists follow the untouched segments' (device-generated too)
        e.po = mv_rows_dev + ed_rows;
        e.lo = mv_list_dev + ed_list;
        ed_rows += e.nn;
        ed_list += e.nc;
    }

    p.t_lists = clk::now();
    p.active = true;
    return NFK_OK;
}

// the device phase of a planned window (after the previous frame has been waited for)
int commit_membership(World* w, MemPlan& p) {
    if (!p.active) return NFK_OK;
    p.active = false;
    w->obj_slot_dirty = true;  // (k_obj_slots before the next device fold)
    using clk = std::chrono::steady_clock;
    const auto t_dev = clk::now();
    Dev& d = w->d;
    const bool full = p.full;
    const std::vector<SegEdit>& edits = p.edits;
    const std::vector<int32_t>&ins_rank = p.ins_rank, &ins_obj = p.ins_obj, &rem_rank = p.rem_rank;
    const std::vector<uint64_t>& ins_meta = p.ins_meta;
    const std::vector<int64_t>& ins_src = p.ins_src;
    const std::vector<SegMove>& moves = p.moves;
    const int32_t mv_rows_dev = p.mv_rows_dev, mv_list_dev = p.mv_list_dev, ed_rows = p.ed_rows, ed_list = p.ed_list;
    std::vector<int32_t> pack_src, un_dst;  // (host-built lists: none since k_seg_edit)
    std::vector<int64_t> un_src;
    MetaLists m;
    // device: pack movers (old slots), then unpack into the new layout, then the metadata.  The
    // untouched segments' lists (full re-layout) are generated first, from the old metadata.
    const int32_t rw = w->row_words;
    w->mhost.clear();
    const size_t o_ps = stage_list(w, pack_src), o_ud = stage_list(w, un_dst), o_us = stage_list(w, un_src);
    const size_t o_ms = stage_list(w, m.slot), o_mo = stage_list(w, m.obj), o_md = stage_list(w, m.desc);
    const size_t o_mp = stage_list(w, m.pl), o_mv = stage_list(w, moves);
    const size_t o_ed = stage_list(w, edits), o_ir = stage_list(w, ins_rank), o_io = stage_list(w, ins_obj);
    const size_t o_im = stage_list(w, ins_meta), o_is = stage_list(w, ins_src), o_rr = stage_list(w, rem_rank);
    const size_t hp = pack_src.size();
    const size_t nd = (size_t)mv_list_dev + ed_list, npk = (size_t)mv_rows_dev + ed_rows;
    int r = dev_reserve(w, (void**)&w->mv_rows, &w->mv_cap, std::max<size_t>(hp + npk, 1) * rw * 8);
    if (r) return r;
    // device-generated lists (untouched segments that move, then edited / new segments):
    // pack_src | un_dst | un_src | m_slot | m_obj | m_desc | m_pl
    const size_t g_ps = 0, g_ud = align16(g_ps + npk * 4), g_us = align16(g_ud + nd * 4), g_ms = align16(g_us + nd * 8),
                 g_mo = align16(g_ms + nd * 4), g_md = align16(g_mo + nd * 4), g_mp = align16(g_md + nd * 8),
                 g_end = align16(g_mp + nd * 4);
    if (nd) {
        r = dev_reserve(w, (void**)&w->glist, &w->glist_cap, g_end);
        if (r) return r;
    }
    r = upload_mhost(w);
    if (r) return r;
    {
        TimeScope ts(w, KT_MEM);
        char* L = (char*)w->mlist;
        char* G = (char*)w->glist;
        if (!moves.empty())
            hipLaunchKernelGGL(k_seg_lists, dim3((unsigned)std::min<size_t>(moves.size(), 8192)), dim3(kTPB), 0,
                               w->stream, (const SegMove*)(L + o_mv), (int32_t)moves.size(),
                               (const int32_t*)w->slot_obj_d, (const uint64_t*)w->fan_desc_w,
                               (const int32_t*)w->pl_slot_w, (int32_t*)(G + g_ps), (int32_t*)(G + g_ud),
                               (int64_t*)(G + g_us), (int32_t*)(G + g_ms), (int32_t*)(G + g_mo), (uint64_t*)(G + g_md),
                               (int32_t*)(G + g_mp));
        if (!edits.empty())
            hipLaunchKernelGGL(k_seg_edit, dim3((unsigned)std::min<size_t>(edits.size(), 8192)), dim3(kTPB), 0,
                               w->stream, (const SegEdit*)(L + o_ed), (int32_t)edits.size(), (const int32_t*)(L + o_ir),
                               (const int32_t*)(L + o_io), (const uint64_t*)(L + o_im), (const int64_t*)(L + o_is),
                               (const int32_t*)(L + o_rr), (const int32_t*)w->slot_obj_d, (const uint64_t*)w->fan_desc_w,
                               (int32_t*)(G + g_ps), (int32_t*)(G + g_ud), (int64_t*)(G + g_us), (int32_t*)(G + g_ms),
                               (int32_t*)(G + g_mo), (uint64_t*)(G + g_md), (int32_t*)(G + g_mp));
        if (hp)
            hipLaunchKernelGGL(k_pack, dim3(grid_for(hp * rw)), dim3(kTPB), 0, w->stream, d,
                               (const int32_t*)(L + o_ps), (int32_t)hp, rw, w->mv_rows);
        if (npk)
            hipLaunchKernelGGL(k_pack, dim3(grid_for(npk * rw)), dim3(kTPB), 0, w->stream, d,
                               (const int32_t*)(G + g_ps), (int32_t)npk, rw, w->mv_rows + hp * rw);
        if (!un_dst.empty())
            hipLaunchKernelGGL(k_unpack, dim3(grid_for(un_dst.size() * rw)), dim3(kTPB), 0, w->stream, d,
                               (const int32_t*)(L + o_ud), (const int64_t*)(L + o_us), (int32_t)un_dst.size(), rw,
                               (const uint64_t*)w->mv_rows, (const uint64_t*)w->ins_rows);
        if (nd)
            hipLaunchKernelGGL(k_unpack, dim3(grid_for(nd * rw)), dim3(kTPB), 0, w->stream, d,
                               (const int32_t*)(G + g_ud), (const int64_t*)(G + g_us), (int32_t)nd, rw,
                               (const uint64_t*)(w->mv_rows + hp * rw), (const uint64_t*)w->ins_rows);
        if (!m.slot.empty())
            hipLaunchKernelGGL(k_meta, dim3(grid_for(m.slot.size())), dim3(kTPB), 0, w->stream,
                               (const int32_t*)(L + o_ms), (const int32_t*)(L + o_mo), (const uint64_t*)(L + o_md),
                               (const int32_t*)(L + o_mp), (int32_t)m.slot.size(), w->slot_obj_d, w->fan_desc_w,
                               w->pl_slot_w);
        if (nd)
            hipLaunchKernelGGL(k_meta, dim3(grid_for(nd)), dim3(kTPB), 0, w->stream, (const int32_t*)(G + g_ms),
                               (const int32_t*)(G + g_mo), (const uint64_t*)(G + g_md), (const int32_t*)(G + g_mp),
                               (int32_t)nd, w->slot_obj_d, w->fan_desc_w, w->pl_slot_w);
        HIPCHK(hipGetLastError());
    }
    const auto t_launched = clk::now();
    const size_t n_touched = w->touched.size();
    // host maps (while the device rewrites the slots)
    std::vector<int32_t>& aff = p.aff;
    const std::vector<int32_t>& epos = p.epos;
    std::vector<EdInfo>& einfo = p.einfo;
    std::vector<World::Seg>& nsegs = p.nsegs;
    const std::vector<int32_t>& nsrc = p.nsrc;
    if (full) {
        w->n_relayout_full++;
        std::vector<int32_t> seg_base0(nsegs.size(), -1), seg_cap0(nsegs.size(), -1);
        for (size_t i = 0; i < nsegs.size(); i++)
            if (nsrc[i] >= 0) {
                seg_base0[i] = w->segs[nsrc[i]].base;
                seg_cap0[i] = w->segs[nsrc[i]].cap;
                nsegs[i].objs = std::move(w->segs[nsrc[i]].objs);
                nsegs[i].keys = std::move(w->segs[nsrc[i]].keys);
            }
        w->segs = std::move(nsegs);
        index_segs(w);
        int64_t total = 0;
        for (const auto& g : w->segs) total = (int64_t)g.base + g.cap;
        // slots past the new end held entities before; every slot below it belongs to a segment
        for (int64_t sl = total; sl < std::min<int64_t>(d.N, (int64_t)w->obj_of_slot.size()); sl++)
            w->obj_of_slot[sl] = -1;
        set_tiles(d, (int32_t)total);
        // the host maps change for the segments whose slots or members changed
        aff.clear();
        for (size_t g = 0; g < w->segs.size(); g++)
            if (nsrc[g] < 0 || w->segs[g].base != seg_base0[g] || w->segs[g].cap != seg_cap0[g]) aff.push_back((int32_t)g);
    } else {
        w->n_relayout_seg++;
        for (int32_t gi : aff) {  // (the old list's buffer goes back to the plan, for the next window)
            std::swap(w->segs[gi].objs, einfo[epos[gi]].seg.objs);
            std::swap(w->segs[gi].keys, einfo[epos[gi]].seg.keys);
            w->segs[gi].np = einfo[epos[gi]].seg.np;
        }
    }
    // the ranks whose slot <-> object pairs change: [first leaver / joiner, the longer of the two
    // lists), or only up to the last leaver / joiner when as many join as leave (the members
    // behind it keep their ranks)
    std::vector<int32_t> mlo(aff.size(), 0), mhi(aff.size());
    for (size_t k = 0; k < aff.size(); k++) {
        mhi[k] = w->segs[aff[k]].cap;
        if (full) continue;
        const EdInfo& x = einfo[epos[aff[k]]];
        const int32_t nn = (int32_t)w->segs[aff[k]].objs.size(), no = nn - (int32_t)x.ins.size() + (int32_t)x.rem.size();
        int32_t lo = INT32_MAX, last = -1;
        if (!x.rem.empty()) lo = x.rem.front(), last = x.rem.back();
        if (!x.ins.empty()) lo = std::min(lo, x.ins.front().first), last = std::max(last, x.ins.back().first);
        mlo[k] = std::min(lo, mhi[k]);
        mhi[k] = nn != no ? std::max(nn, no) : last + 1;
    }
    for (int32_t o : w->touched)
        if (!w->alive[o]) w->slot_of_obj[o] = -1;
    // slot <-> object of the changed segments (disjoint slots and objects per segment: split over
    // threads when large)
    auto maps = [w, &aff, &mlo, &mhi](size_t a, size_t b) {
        for (size_t k = a; k < b; k++) {
            const World::Seg& g = w->segs[aff[k]];
            for (int32_t i = mlo[k]; i < mhi[k]; i++) {
                const int32_t ns = g.base + i;
                const int32_t o = i < (int32_t)g.objs.size() ? g.objs[i] : -1;
                w->obj_of_slot[ns] = o;
                if (o >= 0) w->slot_of_obj[o] = ns;
            }
        }
    };
    {
        int64_t work = 0;
        for (size_t k = 0; k < aff.size(); k++) work += mhi[k] - mlo[k];
        const int nt = work >= (1 << 17) ? (int)std::min<size_t>(8, aff.size()) : 1;
        if (nt <= 1) {
            maps(0, aff.size());
        } else {
            std::vector<std::thread> th;
            for (int t = 0; t < nt; t++) th.emplace_back(maps, aff.size() * t / nt, aff.size() * (t + 1) / nt);
            for (auto& x : th) x.join();
        }
    }
    for (int32_t o : w->touched) {
        w->m_flag[o] = 0;
        w->src_row[o] = -1;
    }
    w->touched.clear();
    w->vc_log.clear();
    w->ins_n = 0;
    const auto t_end = clk::now();
    auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    (full ? w->ms_relayout_full : w->ms_relayout_seg) += ms(p.t_host, p.t_lists) + ms(t_dev, t_end);
    if (getenv("NFGPU_TRACE_MEMBERSHIP"))
        fprintf(stderr, "apply_membership %s: %zu touched, edit %.3f ms (leavers %.3f, joiners %.3f, member lists %.3f), "
                "lists %.3f ms (%zu edited segments, %zu moves; "
                "before the previous frame is waited for), upload+launch %.3f ms, host maps %.3f ms\n",
                full ? "full" : "seg", n_touched, ms(p.t_host, p.t_edit), ms(p.t_host, p.t_leave), ms(p.t_leave, p.t_join),
                ms(p.t_join, p.t_edit), ms(p.t_edit, p.t_lists), edits.size(),
                moves.size(), ms(t_dev, t_launched), ms(t_launched, t_end));
    return NFK_OK;
}

// a new object index (creation order in this world)
int32_t add_object(World* w, int64_t gh, int64_t gd, int32_t scene, int32_t group, uint8_t cls, uint8_t pl) {
    const int32_t o = w->n_obj++;
    w->obj_of.insert(gh, gd, o);
    w->gh.push_back(gh);
    w->guid.push_back({gh, gd});
    w->gd.push_back(gd);
    w->scene.push_back(scene);
    w->group.push_back(group);
    w->cls.push_back(cls);
    w->isplayer.push_back(pl ? 1 : 0);
    w->alive.push_back(1);
    w->src_row.push_back(-1);
    w->m_flag.push_back(0);
    w->slot_of_obj.push_back(-1);
    return o;
}

void touch(World* w, int32_t o) {
    if (!w->m_flag[o]) {
        w->m_flag[o] = 1;
        w->touched.push_back(o);
    }
}

}  // namespace

extern "C" {

static int check_fanout(World* w);

const char* nfk_last_error(void) { return g_err.c_str(); }

int nfk_create(const nfk_config* cfg, void** out) {
    if (!cfg || !out) return fail(NFK_ERR_ARG, "null argument");
    if (cfg->capacity <= 0 || cfg->n_int < 0 || cfg->n_int > NFK_MAX_INT_PROPS || cfg->n_flt < 0 ||
        cfg->n_flt > NFK_MAX_FLT_PROPS || cfg->n_class <= 0 || cfg->n_class > NFK_MAX_CLASSES - 1 ||
        cfg->n_kind < 0 || cfg->n_kind > NFK_MAX_KINDS || cfg->n_rec < 0 || cfg->n_rec > NFK_MAX_RECORDS ||
        cfg->n_obj < 0 || cfg->n_obj > NFK_MAX_OBJ_PROPS || cfg->n_int + cfg->n_flt + cfg->n_obj > NFK_MAX_PROPS)
        return fail(NFK_ERR_ARG, "config out of range");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) return fail(NFK_ERR_HIP, "no HIP device available");
    World* w = new World();
    {
        // host threads for large call batches (the caller and nt - 1 workers).  Default 1: on the
        // GPU boxes the workers made the host work slower, not faster (schedule-call fold 0.85 vs
        // 0.31 ms, the SetProperty fold 3-6 vs 0.67 ms before it moved to the device;
        // profiles/r08b_hostprof*.log)
        int nt = 1;
        if (const char* e = getenv("NFGPU_HOST_THREADS")) nt = std::max(1, std::min(64, atoi(e)));
        w->pool.reset(new HostPool(nt - 1));
        if (const char* e = getenv("NFGPU_PAR_CALLS")) w->par_calls = (size_t)std::max(1, atoi(e));
        if (const char* e = getenv("NFGPU_DEV_LOOKUP")) w->dev_look_min = (size_t)std::max(0, atoi(e));
        w->obj_of.set_log(&w->guid_log);
    }
    w->cfg = *cfg;
    w->n_if = cfg->n_int + cfg->n_flt;
    w->n_prop = w->n_if + cfg->n_obj;
    w->n_pw = w->n_if + 2 * cfg->n_obj;
    w->slack = cfg->slack_per_256 == 0 ? 16 : std::max(cfg->slack_per_256, 0);
    if (cfg->stream) {
        w->stream = (hipStream_t)cfg->stream;
    } else {
        if (hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking) != hipSuccess) {
            delete w;
            return fail(NFK_ERR_HIP, "hipStreamCreate failed");
        }
        w->own_stream = true;
    }
    if (hipEventCreateWithFlags(&w->pin_done, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&w->mpin_done[0], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&w->mpin_done[1], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&w->err_done, hipEventDisableTiming) != hipSuccess ||
        hipHostMalloc((void**)&w->err_pin, 64, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void**)&w->ctrl_pin, kCtrlPinBytes, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void**)&w->err_host, 64, hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer((void**)&w->err_host_d, w->err_host, 0) != hipSuccess) {
        delete w;
        return fail(NFK_ERR_HIP, "hipEventCreate failed");
    }
    clear_err_host(w);
    w->init_props.resize(w->n_prop);
    w->init_rcells.resize(cfg->n_rec);
    w->init_rused.resize(cfg->n_rec);
    w->rec_defined.assign(cfg->n_rec, false);
    memset(w->lk_pid, 0xFF, sizeof(w->lk_pid));
    memset(w->lk_of_pid, 0xFF, sizeof(w->lk_of_pid));
    *out = w;
    return NFK_OK;
}

int nfk_destroy(void* world) {
    World* w = (World*)world;
    if (!w) return NFK_OK;
    (void)hipStreamSynchronize(w->stream);
    for (void* p : w->allocs) (void)hipFree(p);
    if (w->pin) (void)hipHostFree(w->pin);
    if (w->stage) (void)hipFree(w->stage);
    if (w->dense) (void)hipFree(w->dense);
    if (w->fr_dev) (void)hipFree(w->fr_dev);
    if (w->fr_pin) (void)hipHostFree(w->fr_pin);
    if (w->fr_scr) (void)hipFree(w->fr_scr);
    if (w->rank_d) (void)hipFree(w->rank_d);
    if (w->ins_rows) (void)hipFree(w->ins_rows);
    if (w->mv_rows) (void)hipFree(w->mv_rows);
    if (w->mlist) (void)hipFree(w->mlist);
    if (w->glist) (void)hipFree(w->glist);
    if (w->xs_buf) (void)hipFree(w->xs_buf);
    if (w->xf_buf) (void)hipFree(w->xf_buf);
    if (w->tile_work_d) (void)hipFree(w->tile_work_d);
    for (int b = 0; b < 2; b++) {
        if (w->xq[b]) (void)hipFree(w->xq[b]);
        if (w->xq_ev[b]) (void)hipEventDestroy(w->xq_ev[b]);
    }
    if (w->obj_slot_d) (void)hipFree(w->obj_slot_d);
    if (w->rs_buf) (void)hipFree(w->rs_buf);
    if (w->rss_buf) (void)hipFree(w->rss_buf);
    if (w->rl_buf) (void)hipFree(w->rl_buf);
    if (w->lk_buf) (void)hipFree(w->lk_buf);
    if (w->look_stream) (void)hipStreamSynchronize(w->look_stream);
    if (w->guid_d) (void)hipFree(w->guid_d);
    if (w->look_dev) (void)hipFree(w->look_dev);
    if (w->look_pin) (void)hipHostFree(w->look_pin);
    if (w->look_stream) (void)hipStreamDestroy(w->look_stream);
    if (w->gat) (void)hipFree(w->gat);
    if (w->moff_tmp) (void)hipFree(w->moff_tmp);
    if (w->hf_buf) (void)hipFree(w->hf_buf);
    if (w->chain_d) (void)hipFree(w->chain_d);
    if (w->chain_cnt_d) (void)hipFree(w->chain_cnt_d);
    if (w->chain_scr) (void)hipFree(w->chain_scr);
    if (w->chain_pin) (void)hipHostFree(w->chain_pin);
    if (w->q_dev) (void)hipFree(w->q_dev);
    if (w->q_pin) (void)hipHostFree(w->q_pin);
    if (w->vc_tout) (void)hipFree(w->vc_tout);
    if (w->vc_dev) (void)hipFree(w->vc_dev);
    if (w->vc_pin) (void)hipHostFree(w->vc_pin);
    for (auto e : w->vc_ev)
        if (e) (void)hipEventDestroy(e);
    if (w->f_dev) (void)hipFree(w->f_dev);
    if (w->f_pin) (void)hipHostFree(w->f_pin);
    for (auto e : w->f_ev)
        if (e) (void)hipEventDestroy(e);
    if (w->a_dev) (void)hipFree(w->a_dev);
    if (w->a_pin) (void)hipHostFree(w->a_pin);
    for (auto e : w->a_ev)
        if (e) (void)hipEventDestroy(e);
    if (w->s_tab_d) (void)hipFree(w->s_tab_d);
    if (w->s_dev) (void)hipFree(w->s_dev);
    if (w->s_out) (void)hipFree(w->s_out);
    if (w->s_pin) (void)hipHostFree(w->s_pin);
    for (auto e : w->s_ev)
        if (e) (void)hipEventDestroy(e);
    for (auto e : w->q_ev)
        if (e) (void)hipEventDestroy(e);
    for (auto& p : w->pend) {
        (void)hipEventDestroy(p.a);
        (void)hipEventDestroy(p.b);
    }
    for (auto e : w->evpool) (void)hipEventDestroy(e);
    if (w->pin_done) (void)hipEventDestroy(w->pin_done);
    if (w->err_done) (void)hipEventDestroy(w->err_done);
    if (w->err_pin) (void)hipHostFree(w->err_pin);
    if (w->ctrl_pin) (void)hipHostFree(w->ctrl_pin);
    if (w->err_host) (void)hipHostFree(w->err_host);
    for (int i = 0; i < 2; i++) {
        if (w->mpin_done[i]) (void)hipEventDestroy(w->mpin_done[i]);
        if (w->mpin[i]) (void)hipHostFree(w->mpin[i]);
    }
    if (w->xpin_done) (void)hipEventDestroy(w->xpin_done);
    if (w->xpin) (void)hipHostFree(w->xpin);
    if (w->own_stream) (void)hipStreamDestroy(w->stream);
    delete w;
    return NFK_OK;
}

int nfk_set_prop_flags(void* world, int32_t c, const uint8_t* flags) {
    World* w = (World*)world;
    if (!w || !flags || c < 0 || c >= w->cfg.n_class) return fail(NFK_ERR_ARG, "bad class");
    for (int p = 0; p < w->n_prop; p++) w->tab.pflags[c][p] = flags[p];
    w->s_tab_dirty = true;  // (the snapshots' view masks)
    return NFK_OK;
}

int nfk_define_record(void* world, int32_t rec, int32_t rows, int32_t cols, const uint8_t* col_types,
                      const uint8_t* flags_per_class) {
    World* w = (World*)world;
    if (!w || rec < 0 || rec >= w->cfg.n_rec || rows <= 0 || rows > NFK_MAX_REC_ROWS || cols <= 0 ||
        cols > NFK_MAX_REC_COLS || !flags_per_class)
        return fail(NFK_ERR_ARG, "bad record definition");
    if (w->committed) return fail(NFK_ERR_STATE, "schema is fixed after commit");
    // an object column is a data half with its head half right behind it (checked before anything
    // is changed)
    for (int c = 0; col_types && c < cols; c++) {
        const int t = col_types[c];
        if (t > NFK_REC_OBJ_HEAD)
            return fail(NFK_ERR_ARG, "record column type must be 0 (int64), 1 (f64) or 2, 3 (an NFGUID's halves)");
        if (t == NFK_REC_OBJ_DATA && (c + 1 >= cols || col_types[c + 1] != NFK_REC_OBJ_HEAD))
            return fail(NFK_ERR_ARG, "record column " + std::to_string(c) + ": a data half (2) without its head half (3) behind it");
        if (t == NFK_REC_OBJ_HEAD && (c == 0 || col_types[c - 1] != NFK_REC_OBJ_DATA))
            return fail(NFK_ERR_ARG, "record column " + std::to_string(c) + ": a head half (3) without its data half (2) before it");
    }
    w->tab.rec_rows[rec] = rows;
    w->tab.rec_cols[rec] = cols;
    for (int c = 0; c < w->cfg.n_class; c++) w->tab.rflags[c][rec] = flags_per_class[c];
    for (int c = 0; c < NFK_MAX_REC_COLS; c++) w->rec_ctype[rec][c] = col_types && c < cols ? col_types[c] : 0;
    w->rec_defined[rec] = true;
    return NFK_OK;
}

// the linked properties of every record but `skip` (-1: of all of them)
static void link_pid_mask(World* w, int skip, uint64_t m[2]) {
    m[0] = m[1] = 0;
    if (skip < 0) {
        memset(w->lk_of_pid, 0xFF, sizeof(w->lk_of_pid));
        for (int r = 0; r < w->cfg.n_rec; r++)
            for (int c = 0; w->lk_rows[r] && c < NFK_MAX_REC_COLS; c++)
                if (w->lk_pid[r][c] >= 0) w->lk_of_pid[w->lk_pid[r][c]] = (int16_t)(r << 4 | c);
    }
    for (int r = 0; r < w->cfg.n_rec; r++)
        for (int c = 0; r != skip && w->lk_rows[r] && c < NFK_MAX_REC_COLS; c++)
            if (w->lk_pid[r][c] >= 0) m[w->lk_pid[r][c] >> 6] |= 1ull << (w->lk_pid[r][c] & 63);
}

// NFCPropertyModule::OnRecordPropertyEvent (PM:127-149) as part of the schema: after every record
// event of record rec, the int property col_pid[nCol] takes the 32-bit sum of column nCol over the
// record's first `rows` rows (nfgpu.h states the events' nCol).  Applied by k_rrows / k_links.
int nfk_link_record(void* world, int32_t rec, int32_t rows, const int32_t* col_pid, int32_t mode) {
    World* w = (World*)world;
    if (!w) return fail(NFK_ERR_ARG, "null world");
    if (w->committed) return fail(NFK_ERR_STATE, "schema is fixed after commit");
    if (rec < 0 || rec >= w->cfg.n_rec || !w->rec_defined[rec]) return fail(NFK_ERR_ARG, "nfk_link_record: bad record");
    if (col_pid) {
        if (mode != NFK_LINK_SUM32) return fail(NFK_ERR_ARG, "nfk_link_record: mode must be NFK_LINK_SUM32");
        if (rows < 1 || rows > w->tab.rec_rows[rec])
            return fail(NFK_ERR_ARG, "nfk_link_record: rows outside [1, the record's rows]");
    }
    uint64_t other[2], mine[2] = {0, 0};
    link_pid_mask(w, rec, other);
    const int cols = w->tab.rec_cols[rec];
    for (int c = 0; col_pid && c < cols; c++) {
        const int32_t p = col_pid[c];
        if (p == -1) continue;
        if (p < 0 || p >= w->cfg.n_int)
            return fail(NFK_ERR_ARG, "nfk_link_record: column " + std::to_string(c) + " links something that is not an int property");
        if (w->rec_ctype[rec][c] != NFK_REC_INT)
            return fail(NFK_ERR_ARG, "nfk_link_record: column " + std::to_string(c) + " is not an int column");
        if (((other[p >> 6] | mine[p >> 6]) >> (p & 63)) & 1)
            return fail(NFK_ERR_ARG, "nfk_link_record: property " + std::to_string(p) + " is linked from two places");
        if (p == w->pid_scene || p == w->pid_group)
            return fail(NFK_ERR_ARG, "nfk_link_record: property " + std::to_string(p) + " is one of nfk_set_scene_props' properties");
        mine[p >> 6] |= 1ull << (p & 63);
    }
    // (checked before anything is changed; a link without a linked column is no link)
    memset(w->lk_pid[rec], 0xFF, sizeof(w->lk_pid[rec]));
    w->lk_rows[rec] = (mine[0] | mine[1]) ? (int8_t)rows : (int8_t)0;
    for (int c = 0; w->lk_rows[rec] && c < cols; c++) w->lk_pid[rec][c] = (int8_t)col_pid[c];
    link_pid_mask(w, -1, w->lk_pids);
    return NFK_OK;
}

// an NFK_GUARD_CELL op's cell: a defined record, a row and column inside its shape, an int column
static int check_guard_cell(World* w, const nfk_op& op) {
    if (op.guard & 0xE000u) return fail(NFK_ERR_ARG, "NFK_GUARD_CELL: guard bits 13..15 must be 0 (NFK_GUARD_CELL_ID)");
    const uint32_t c = op.guard & 0x1FFFu;
    const int r = (int)cell_rec(c), row = (int)cell_row(c), col = (int)cell_col(c);
    if (r >= w->cfg.n_rec || !w->rec_defined[r]) return fail(NFK_ERR_ARG, "NFK_GUARD_CELL: undefined record " + std::to_string(r));
    if (row >= w->tab.rec_rows[r])
        return fail(NFK_ERR_ARG, "NFK_GUARD_CELL: row " + std::to_string(row) + " outside record " + std::to_string(r) + "'s rows");
    if (col >= w->tab.rec_cols[r])
        return fail(NFK_ERR_ARG, "NFK_GUARD_CELL: column " + std::to_string(col) + " outside record " + std::to_string(r) + "'s columns");
    if (w->rec_ctype[r][col] != NFK_REC_INT)  // (f64, or a half of an object column)
        return fail(NFK_ERR_ARG, "NFK_GUARD_CELL: the guard's column is not an int column");
    return NFK_OK;
}

int nfk_define_kind(void* world, int32_t kind, const nfk_op* ops, int32_t n_ops) {
    World* w = (World*)world;
    if (!w || kind < 0 || kind >= w->cfg.n_kind || n_ops < 0 || n_ops > NFK_MAX_OPS || (n_ops && !ops))
        return fail(NFK_ERR_ARG, "bad kind definition");
    if (w->committed) return fail(NFK_ERR_STATE, "schema is fixed after commit");
    for (int i = 0; i < n_ops; i++) {
        const nfk_op& op = ops[i];
        const int np = w->n_if, ni = w->cfg.n_int;  // (object properties are no program operands)
        auto isint = [&](int64_t p) { return p >= 0 && p < ni; };
        auto isflt = [&](int64_t p) { return p >= ni && p < np; };
        if (op.flags & NFK_GUARD) {
            const bool rec = op.code == NFK_OP_RIADD_CLAMP || op.code == NFK_OP_RFAFFINE;
            // (NFK_GUARD_PROP: compared to the int property guard >> 19; otherwise to the constant
            // NFK_GUARD_KVAL(guard) in bits 19..31, any value)
            const bool vs = (op.guard & NFK_GUARD_PROP) != 0, cell = (op.flags & NFK_GUARD_CELL) != 0;
            if (rec) return fail(NFK_ERR_ARG, "NFK_GUARD: a record op takes no guard");
            if (op.code == NFK_OP_NOP || (!cell && !isint(op.guard & 0xFFFF)) || (vs && !isint(op.guard >> 19)))
                return fail(NFK_ERR_ARG, "NFK_GUARD: a property op guarded by an int property");
            if (cell) {
                const int r = check_guard_cell(w, op);
                if (r) return r;
            }
        } else if (op.flags & NFK_GUARD_CELL) {
            return fail(NFK_ERR_ARG, "NFK_GUARD_CELL without NFK_GUARD");
        } else if (op.guard) {
            return fail(NFK_ERR_ARG, "nfk_op.guard without NFK_GUARD");
        }
        switch (op.code) {
        case NFK_OP_IADD_CLAMP:
            if (!isint(op.dst) || ((op.flags & NFK_A_PROP) && !isint(op.a)) ||
                ((op.flags & NFK_LO_PROP) && !isint(op.b)) || ((op.flags & NFK_HI_PROP) && !isint(op.c)))
                return fail(NFK_ERR_ARG, "IADD_CLAMP operands must be int properties");
            break;
        case NFK_OP_FLERP:
            if (!isflt(op.dst) || !isflt(op.a)) return fail(NFK_ERR_ARG, "FLERP operands must be float properties");
            break;
        case NFK_OP_FAFFINE:
            if (!isflt(op.dst)) return fail(NFK_ERR_ARG, "FAFFINE dst must be a float property");
            break;
        case NFK_OP_ISET:
            if (!isint(op.dst) || ((op.flags & NFK_A_PROP) && !isint(op.a)))
                return fail(NFK_ERR_ARG, "ISET operands must be int properties");
            break;
        case NFK_OP_FSET:
            if (!isflt(op.dst) || ((op.flags & NFK_A_PROP) && !isflt(op.a)))
                return fail(NFK_ERR_ARG, "FSET operands must be float properties");
            break;
        case NFK_OP_RIADD_CLAMP:
        case NFK_OP_RFAFFINE: {
            int r = op.dst >> 8, col = op.dst & 255;
            if (r >= w->cfg.n_rec || !w->rec_defined[r] || col >= w->tab.rec_cols[r])
                return fail(NFK_ERR_ARG, "record op on undefined record/col");
            // NFCRecord::SetInt / SetFloat refuse a cell of the other type (RC:189, RC:250): such
            // an op could never change a cell, so it is rejected with the kind
            // (a half of an object column is neither)
            if (w->rec_ctype[r][col] != (op.code == NFK_OP_RFAFFINE ? NFK_REC_F64 : NFK_REC_INT))
                return fail(NFK_ERR_ARG, "record op type does not match the column type");
            break;
        }
        case NFK_OP_NOP:
            break;
        default:
            return fail(NFK_ERR_ARG, "unknown op code");
        }
        w->tab.ops[kind][i] = op;
    }
    w->tab.nops[kind] = n_ops;
    w->kind_defined[kind] = true;
    return NFK_OK;
}

int nfk_create_objects(void* world, int32_t n, const int64_t* gh, const int64_t* gd, const int32_t* scene,
                       const int32_t* group, const uint8_t* cls, const uint8_t* isplayer) {
    World* w = (World*)world;
    if (!w || n < 0 || (n && (!gh || !gd || !scene || !group || !cls || !isplayer)))
        return fail(NFK_ERR_ARG, "null argument");
    if (w->committed) return fail(NFK_ERR_STATE, "after commit, create objects with nfk_import_objects / nfk_spawn_objects");
    if ((int64_t)w->n_obj + n > w->cfg.capacity) return fail(NFK_ERR_CAPACITY, "entity capacity exceeded");
    for (int32_t i = 0; i < n; i++) {
        if (cls[i] >= w->cfg.n_class) return fail(NFK_ERR_ARG, "class id out of range");
        if (group[i] < 0) return fail(NFK_ERR_ARG, "negative group");
        if (w->obj_of.count(gh[i], gd[i])) return fail(NFK_ERR_ARG, "The object has Exists");  // KM:131
    }
    for (int32_t i = 0; i < n; i++) add_object(w, gh[i], gd[i], scene[i], group[i], cls[i], isplayer[i]);
    return NFK_OK;
}

int nfk_load_prop(void* world, int32_t pid, const uint64_t* bits) {
    World* w = (World*)world;
    if (!w || pid < 0 || pid >= w->n_if || !bits) return fail(NFK_ERR_ARG, "bad property (object properties: nfk_load_object)");
    if (w->committed) return fail(NFK_ERR_STATE, "load before commit");
    w->init_props[pid].assign(bits, bits + w->n_obj);
    return NFK_OK;
}

int nfk_load_object(void* world, int32_t pid, const int64_t* head, const int64_t* data) {
    World* w = (World*)world;
    if (!w || pid < w->n_if || pid >= w->n_prop || !head || !data) return fail(NFK_ERR_ARG, "bad object property");
    if (w->committed) return fail(NFK_ERR_STATE, "load before commit");
    std::vector<uint64_t>& v = w->init_props[pid];  // (data, head) per object
    v.resize((size_t)2 * w->n_obj);
    for (int32_t o = 0; o < w->n_obj; o++) {
        v[2 * (size_t)o] = (uint64_t)data[o];
        v[2 * (size_t)o + 1] = (uint64_t)head[o];
    }
    return NFK_OK;
}

int nfk_load_record(void* world, int32_t rec, const uint64_t* cells, const uint64_t* used) {
    World* w = (World*)world;
    if (!w || rec < 0 || rec >= w->cfg.n_rec || !w->rec_defined[rec] || !cells || !used)
        return fail(NFK_ERR_ARG, "bad record");
    if (w->committed) return fail(NFK_ERR_STATE, "load before commit");
    size_t per = (size_t)w->tab.rec_rows[rec] * w->tab.rec_cols[rec];
    w->init_rcells[rec].assign(cells, cells + per * w->n_obj);
    w->init_rused[rec].assign(used, used + w->n_obj);
    return NFK_OK;
}

int nfk_commit(void* world) {
    World* w = (World*)world;
    if (!w) return fail(NFK_ERR_ARG, "null world");
    if (w->committed) return fail(NFK_ERR_STATE, "already committed");
    const int32_t cfg_cap = w->cfg.capacity;
    int32_t cap = 0;
    const int NI = w->cfg.n_int, NF = w->cfg.n_flt, NK = w->cfg.n_kind, NR = w->cfg.n_rec;
    for (int r = 0; r < NR; r++)
        if (!w->rec_defined[r]) return fail(NFK_ERR_ARG, "record " + std::to_string(r) + " not defined");

    // guard cells against the records' final shapes (a record may have been redefined after the kind)
    for (int k = 0; k < NK; k++)
        for (int i = 0; i < w->tab.nops[k]; i++)
            if (w->tab.ops[k][i].flags & NFK_GUARD_CELL) {
                const int r = check_guard_cell(w, w->tab.ops[k][i]);
                if (r) return r;
            }
    // property links against the records' final shapes, and against the programs: a linked property
    // belongs to its link (no program writes it), and no record op feeds a linked column
    for (int r = 0; r < NR; r++) {
        if (!w->lk_rows[r]) continue;
        if (w->lk_rows[r] > w->tab.rec_rows[r])
            return fail(NFK_ERR_ARG, "record " + std::to_string(r) + " was redefined with fewer rows than its link sums");
        for (int c = 0; c < NFK_MAX_REC_COLS; c++)
            if (w->lk_pid[r][c] >= 0 && (c >= w->tab.rec_cols[r] || w->rec_ctype[r][c] != NFK_REC_INT))
                return fail(NFK_ERR_ARG, "record " + std::to_string(r) + " was redefined: linked column " + std::to_string(c) +
                                             " is not an int column");
    }
    if (w->lk_pids[0] | w->lk_pids[1]) {
        if (w->linked_pid(w->pid_scene) || w->linked_pid(w->pid_group))
            return fail(NFK_ERR_ARG, "a linked property is one of nfk_set_scene_props' properties");
        for (int k = 0; k < NK; k++)
            for (int i = 0; i < w->tab.nops[k]; i++) {
                const nfk_op& op = w->tab.ops[k][i];
                if (op.code == NFK_OP_RIADD_CLAMP || op.code == NFK_OP_RFAFFINE) {
                    const int r = op.dst >> 8, c = op.dst & 255;  // (in range: nfk_define_kind)
                    if (r < NR && c < NFK_MAX_REC_COLS && w->lk_rows[r] && w->lk_pid[r][c] >= 0)
                        return fail(NFK_ERR_ARG, "kind " + std::to_string(k) + ": a record op targets a linked (record, column)");
                } else if (prop_op(op.code) && w->linked_pid(op.dst)) {
                    return fail(NFK_ERR_ARG, "kind " + std::to_string(k) + " writes linked property " + std::to_string(op.dst));
                }
            }
    }
    // record ops: compiled list sorted by (rec, col); distinct (rec, col) required
    int nro = 0;
    for (int k = 0; k < NK; k++)
        for (int i = 0; i < w->tab.nops[k]; i++) {
            const nfk_op& op = w->tab.ops[k][i];
            if (op.code == NFK_OP_RIADD_CLAMP || op.code == NFK_OP_RFAFFINE) {
                if (nro == NFK_MAX_REC_OPS) return fail(NFK_ERR_ARG, "at most NFK_MAX_REC_OPS record ops across all kinds");
                RecOp ro{k, op.dst >> 8, op.dst & 255, op.code, op.a, op.b, op.c};
                w->tab.recops[nro++] = ro;
                w->tab.kind_has_recop |= 1u << k;
            } else if (prop_op(op.code)) {
                w->dst_union_mask[op.dst >> 6] |= 1ull << (op.dst & 63);
            }
        }
    std::sort(w->tab.recops, w->tab.recops + nro, [](const RecOp& a, const RecOp& b) {
        return a.rec != b.rec ? a.rec < b.rec : a.col < b.col;
    });
    for (int i = 1; i < nro; i++)
        if (w->tab.recops[i].rec == w->tab.recops[i - 1].rec && w->tab.recops[i].col == w->tab.recops[i - 1].col)
            return fail(NFK_ERR_ARG, "two record ops on the same (record, col)");
    w->tab.n_recops = nro;
    // the programs' working set (k_tick): program destinations -> writable U slots, read-only
    // operands after them (build_u_tables)
    w->u_ok = build_u_tables(w->tab, NK, w->u_wp, w->u_rp);
    w->n_dst_union = __builtin_popcountll(w->dst_union_mask[0]) + __builtin_popcountll(w->dst_union_mask[1]);
    if (w->n_dst_union > NFK_MAX_TOUCH)
        return fail(NFK_ERR_TOUCH, "programs write more than NFK_MAX_TOUCH distinct properties");

    // property columns (Tables::p_off / p_str): one plain column per int / float property, laid out
    // below.  Interleaved layouts (the properties one heartbeat program touches, or those with the
    // same access signature, stored together) measured slower on config[1]
    // (profiles/r01zo_ablate.log: 99.8 us vs 110.7 grouped, 104.8 by signature; again in
    // r14f_sparse_groups_ab.txt): a dense kind's strided 8-byte accesses cost twice the L2 requests
    // per load and its write-backs cover half lines, while a sparse kind's extra lines are few.

    // membership layout: scene-group segments, NFGUID order inside (see plan_membership)
    const int64_t n_slots = plan_segments(w, w->slack, w->segs);
    index_segs(w);
    MetaLists meta;
    w->max_np = 0;
    for (auto& g : w->segs) {
        int r = seg_meta(w, g, meta);
        if (r) return r;
    }
    {
        // slot capacity: the population plus slack, and at least the configured capacity plus slack
        const int64_t want = std::max<int64_t>(n_slots, (int64_t)cfg_cap + (int64_t)cfg_cap * w->slack / 256);
        const int64_t c = (want + kTile - 1) / kTile * kTile;
        if (c > INT32_MAX / 2) return fail(NFK_ERR_CAPACITY, "slot capacity too large");
        cap = (int32_t)c;
    }
    w->obj_of_slot.assign(cap, -1);
    for (size_t i = 0; i < meta.slot.size(); i++) {
        w->obj_of_slot[meta.slot[i]] = meta.obj[i];
        if (meta.obj[i] >= 0) w->slot_of_obj[meta.obj[i]] = meta.slot[i];
    }
    w->row_words = w->n_pw + 4 * NK;
    for (int r = 0; r < NR; r++) w->row_words += w->tab.rec_rows[r] * w->tab.rec_cols[r] + 1;

    // device allocation
    Dev& d = w->d;
    d.cap = cap;
    set_tiles(d, (int32_t)n_slots);
    d.n_int = NI;
    d.n_flt = NF;
    d.n_if = NI + NF;
    d.n_obj = w->cfg.n_obj;
    d.err_host = w->err_host_d;
    d.n_kind = NK;
    d.n_rec = NR;
    d.n_class = w->cfg.n_class;
    // the record pipeline (fired masks, k_records, record tiles) runs in a world with record
    // programs or with records that SetRecord* calls can change
    bool any_rec = false;
    for (int r = 0; r < NR; r++) any_rec = any_rec || w->rec_defined[r];
    d.has_recops = nro > 0 || any_rec;
    memcpy(w->tab.rec_ctype, w->rec_ctype, sizeof(w->tab.rec_ctype));
    w->rec_obj = false;
    for (int r = 0; r < NR; r++)
        for (int c = 0; w->rec_defined[r] && c < w->tab.rec_cols[r]; c++) w->rec_obj = w->rec_obj || w->rec_ctype[r][c] == NFK_REC_OBJ_DATA;
    ALLOC(w->tab_d, sizeof(Tables));
    ALLOC(d.tally, (size_t)3 * kTallyN * 8 * 8);
    ALLOC(w->ctrl, sizeof(Ctrl));
    {
        const char* ab = getenv("NFGPU_ABLATE");
        d.ablate = ab ? (uint32_t)strtoul(ab, nullptr, 0) : 0u;
    }
    w->s_unfixed = 0;
    w->s_epoch_set = false;
    for (int k = 0; k < NK; k++)
        if (w->kind_defined[k] && !(d.ablate & kAblSchedWide)) w->s_unfixed |= 1u << k;
    const int64_t cpad = kColPad / 8;  // column pad in values
    d.s_kstr = cap + (int32_t)(kColPad / (int64_t)sizeof(SchedHot));
    d.s_wstr = cap + (int32_t)cpad;
    d.s_epoch = 0;
    d.s_kvalid = 0;
    memset(d.s_step, 0, sizeof(d.s_step));
    ALLOC(d.pmem, ((size_t)cap + cpad) * (size_t)std::max(w->n_pw, 1) * 8);
    {
        int64_t off = 0;
        for (int p = 0; p < w->n_if; p++) {
            w->tab.p_off[p] = off;
            w->tab.p_str[p] = 1;
            off += (int64_t)cap + cpad;
        }
        // an object property is one 16-byte column: (data, head) of slot e at p_off + 2e
        for (int p = w->n_if; p < w->n_prop; p++) {
            w->tab.p_off[p] = off;
            w->tab.p_str[p] = 2;
            off += 2 * (int64_t)cap + cpad;
        }
    }
    ALLOC(d.s_word, (size_t)std::max(NK, 1) * d.s_wstr * 8);
    ALLOC(d.s_wide, (size_t)std::max(NK, 1) * d.s_kstr * sizeof(SchedHot));
    ALLOC(d.s_cold, (size_t)std::max(NK, 1) * d.s_kstr * sizeof(SchedCold));
    ALLOC(d.e_flags, cap);
    ALLOC(d.ext_head, (size_t)cap * 4);
    ALLOC(d.rs_head, (size_t)cap * 4);
    ALLOC(d.fired_mask, (size_t)cap * 4);
    size_t rec_events_per_ent = 0;
    for (int i = 0; i < nro; i++) rec_events_per_ent += w->tab.rec_rows[w->tab.recops[i].rec];
    for (int r = 0; r < NR; r++) {
        ALLOC(d.rcells[r], (size_t)cap * w->tab.rec_rows[r] * w->tab.rec_cols[r] * 8);
        ALLOC(d.rused[r], (size_t)cap * 8);
    }
    set_working_set(w);  // (after the records' arrays: a guard cell's slot points into them)
    ALLOC(w->pl_slot_w, (size_t)cap * 4);
    ALLOC(w->slot_obj_d, (size_t)cap * 4);
    ALLOC(w->fan_desc_w, (size_t)cap * 8);
    d.fan_desc = w->fan_desc_w;
    d.pl_slot = w->pl_slot_w;
    // output staging sized for every tile of the slot capacity
    d.ev_tcap = kTile * std::max(w->n_dst_union, 1);  // grows for frames with standalone SetProperty groups
    d.fi_tcap = kTile * std::max(NK, 1);
    d.re_tcap = (int32_t)(kRTile * std::max<size_t>(rec_events_per_ent, 1));
    const size_t nt = cap / kTile, nrt = cap / kRTile;
    const size_t ev_n = nt * d.ev_tcap, fi_n = nt * d.fi_tcap, re_n = d.has_recops ? nrt * d.re_tcap : 1;
    ALLOC(d.t_ev, nt * 4);
    ALLOC(d.t_fi, nt * 4);
    ALLOC(d.t_re, nrt * 4);
    ALLOC(d.t_msg, (nt + nrt) * 4);
    ALLOC(d.ev_base, (nt + 1) * 4);
    ALLOC(d.fi_base, (nt + 1) * 4);
    ALLOC(d.re_base, (nrt + 1) * 4);
    ALLOC(d.msg_base, (nt + nrt + 1) * 4);
    ALLOC(d.lb_st, std::max<size_t>(nt, 1) * kRankWgs * 8);
    d.msg_cap = w->cfg.msg_capacity > 0 ? w->cfg.msg_capacity : (int64_t)cap * 32;
    if (d.msg_cap > 0xFFFFFFFFll) return fail(NFK_ERR_ARG, "msg_capacity must fit 32-bit offsets");
    ALLOC(d.ev_slot, ev_n * 4);
    ALLOC(d.ev_pid, ev_n * 4);
    ALLOC(d.ev_old, ev_n * 8);
    ALLOC(d.ev_new, ev_n * 8);
    ALLOC(d.ev_moff, ev_n * 4);
    if (w->cfg.n_obj) {
        ALLOC(d.ev_old_h, ev_n * 8);
        ALLOC(d.ev_new_h, ev_n * 8);
    }
    ALLOC(d.fi_slot, fi_n * 4);
    ALLOC(d.fi_kind, fi_n * 4);
    ALLOC(d.fi_remain, fi_n * 4);
    ALLOC(d.re_rrc, re_n * 4);
    ALLOC(d.re_old, re_n * 8);
    ALLOC(d.re_new, re_n * 8);
    ALLOC(d.re_moff, re_n * 4);
    if (w->rec_obj) {
        ALLOC(w->re_old_h, re_n * 8);
        ALLOC(w->re_new_h, re_n * 8);
    }
    ALLOC(d.msg_rcpt, d.msg_cap * 4);
    d.tab = w->tab_d;
    d.ctrl = w->ctrl;
    // record ops with their record's arrays and op span (k_records reads them as scalars)
    d.n_rops = nro;
    d.rop_kinds = w->tab.kind_has_recop;
    for (int i = 0; i < nro; i++) {
        const RecOp& ro = w->tab.recops[i];
        RecOpX& x = d.rops[i];
        x.cells = d.rcells[ro.rec];
        x.used = d.rused[ro.rec];
        x.a = ro.a;
        x.b = ro.b;
        x.c = ro.c;
        x.kind = ro.kind;
        x.rec = ro.rec;
        x.col = ro.col;
        x.code = ro.code;
        x.rows = w->tab.rec_rows[ro.rec];
        x.cols = w->tab.rec_cols[ro.rec];
        int f = i, l = i;
        while (f > 0 && w->tab.recops[f - 1].rec == ro.rec) f--;
        while (l + 1 < nro && w->tab.recops[l + 1].rec == ro.rec) l++;
        x.gfirst = f;
        x.glast = l;
    }

    // uploads (synchronous: commit is control plane)
    HIPCHK(hipMemcpy(w->tab_d, &w->tab, sizeof(Tables), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(w->ctrl, 0, sizeof(Ctrl)));
    HIPCHK(hipMemset(d.tally, 0, (size_t)3 * kTallyN * 8 * 8));
    for (int p = 0; p < w->n_if; p++) {
        std::vector<uint64_t> blk((size_t)cap, 0);
        if (!w->init_props[p].empty())
            for (int32_t s = 0; s < d.N; s++)
                if (w->obj_of_slot[s] >= 0) blk[(size_t)s] = w->init_props[p][w->obj_of_slot[s]];
        HIPCHK(hipMemcpy(d.pmem + w->tab.p_off[p], blk.data(), blk.size() * 8, hipMemcpyHostToDevice));
    }
    for (int p = w->n_if; p < w->n_prop; p++) {
        std::vector<uint64_t> blk((size_t)cap * 2, 0);
        if (!w->init_props[p].empty())
            for (int32_t s = 0; s < d.N; s++)
                if (w->obj_of_slot[s] >= 0) {
                    blk[(size_t)s * 2] = w->init_props[p][(size_t)w->obj_of_slot[s] * 2];
                    blk[(size_t)s * 2 + 1] = w->init_props[p][(size_t)w->obj_of_slot[s] * 2 + 1];
                }
        HIPCHK(hipMemcpy(d.pmem + w->tab.p_off[p], blk.data(), blk.size() * 8, hipMemcpyHostToDevice));
    }
    for (int r = 0; r < NR; r++) {
        size_t per = (size_t)w->tab.rec_rows[r] * w->tab.rec_cols[r];
        std::vector<uint64_t> cells(per * cap, 0), used(cap, 0);
        if (!w->init_rcells[r].empty())
            for (int32_t s = 0; s < d.N; s++) {
                int32_t o = w->obj_of_slot[s];
                if (o < 0) continue;
                used[s] = w->init_rused[r][o];
                // each column's vector in packed row order (rec_pos)
                const int rows = w->tab.rec_rows[r], cols = w->tab.rec_cols[r];
                const uint64_t rowm = rec_rowm(rows);
                const uint64_t* src = &w->init_rcells[r][(size_t)o * per];
                uint64_t* dst = &cells[(size_t)s * per];
                for (int c = 0; c < cols; c++)
                    for (int q = 0; q < rows; q++) dst[(size_t)c * rows + rec_pos(used[s], rowm, q)] = src[(size_t)c * rows + q];
            }
        HIPCHK(hipMemcpy(d.rcells[r], cells.data(), cells.size() * 8, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d.rused[r], used.data(), used.size() * 8, hipMemcpyHostToDevice));
    }
    HIPCHK(hipMemset(d.s_word, 0, (size_t)std::max(NK, 1) * d.s_wstr * 8));
    HIPCHK(hipMemset(d.s_wide, 0, (size_t)std::max(NK, 1) * d.s_kstr * sizeof(SchedHot)));
    HIPCHK(hipMemset(d.s_cold, 0, (size_t)std::max(NK, 1) * d.s_kstr * sizeof(SchedCold)));
    {
        std::vector<uint64_t> fd(cap, kDeadDesc);
        std::vector<int32_t> pls(cap, 0), so(cap, -1);
        for (size_t i = 0; i < meta.slot.size(); i++) {
            fd[meta.slot[i]] = meta.desc[i];
            pls[meta.slot[i]] = meta.pl[i];
            so[meta.slot[i]] = meta.obj[i];
        }
        HIPCHK(hipMemcpy(w->fan_desc_w, fd.data(), (size_t)cap * 8, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(w->pl_slot_w, pls.data(), (size_t)cap * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(w->slot_obj_d, so.data(), (size_t)cap * 4, hipMemcpyHostToDevice));
    }
    HIPCHK(hipMemset(d.e_flags, 0, cap));
    HIPCHK(hipMemset(d.ext_head, 0, (size_t)cap * 4));
    HIPCHK(hipMemset(d.rs_head, 0, (size_t)cap * 4));
    HIPCHK(hipMemset(d.fired_mask, 0, (size_t)cap * 4));
    HIPCHK(hipMemset(d.t_ev, 0, nt * 4));
    HIPCHK(hipMemset(d.t_fi, 0, nt * 4));
    HIPCHK(hipMemset(d.t_re, 0, nrt * 4));
    HIPCHK(hipMemset(d.t_msg, 0, (nt + nrt) * 4));
    HIPCHK(hipMemset(d.ev_base, 0, (nt + 1) * 4));
    HIPCHK(hipMemset(d.fi_base, 0, (nt + 1) * 4));
    HIPCHK(hipMemset(d.re_base, 0, (nrt + 1) * 4));
    HIPCHK(hipMemset(d.msg_base, 0, (nt + nrt + 1) * 4));
    HIPCHK(hipMemset(d.lb_st, 0, std::max<size_t>(nt, 1) * kRankWgs * 8));
    w->lb_epoch = 0;
    // creation-time values are now on the device
    for (auto& v : w->init_props) std::vector<uint64_t>().swap(v);
    for (auto& v : w->init_rcells) std::vector<uint64_t>().swap(v);
    build_jit(w);  // k_tick for this schema (hipRTC); the generic kernel stays when it cannot be built
    // room for objects created or imported after commit (every arrival takes a new object index):
    // the per-object vectors and the arrivals' row buffer grow in the background of a frame only
    // after a quarter of the world has arrived, not on the first SwitchScene into this shard
    {
        const size_t room = (size_t)w->n_obj + (size_t)w->n_obj / 4 + 4096;
        w->gh.reserve(room);
        w->gd.reserve(room);
        w->guid.reserve(room);
        w->scene.reserve(room);
        w->group.reserve(room);
        w->cls.reserve(room);
        w->isplayer.reserve(room);
        w->slot_of_obj.reserve(room);
        w->alive.reserve(room);
        w->src_row.reserve(room);
        w->m_flag.reserve(room);
        if (!w->ins_rows) {
            const size_t c = 1024;
            HIPCHK(hipMalloc((void**)&w->ins_rows, c * (size_t)w->row_words * 8));
            w->ins_cap = c;
        }
    }
    w->committed = true;
    return NFK_OK;
}

// the SetProperty* calls of a batch, their objects resolved (obj[i] < 0: no such object; gh / gd
// name it in the error when given): every call is checked before any is queued
static int queue_sets(World* w, int32_t n, const int32_t* obj, const int32_t* pid, const uint64_t* bits,
                      const int64_t* gh, const int64_t* gd) {
    for (int32_t i = 0; i < n; i++) {
        if (obj[i] < 0)  // NFCKernelModule logs "There is no object" and returns false (KM:331)
            return fail(NFK_ERR_NOTFOUND, gh ? "no object " + std::to_string(gh[i]) + "-" + std::to_string(gd[i])
                                             : "no object index " + std::to_string(obj[i]));
        if (pid[i] < 0 || pid[i] >= w->n_if)
            return fail(NFK_ERR_ARG, pid[i] >= w->n_if && pid[i] < w->n_prop ? "object property: use nfk_set_objects"
                                                                              : "bad property id");
        if (w->linked_pid(pid[i]))  // (the batch queues nothing)
            return fail(NFK_ERR_ARG, "property " + std::to_string(pid[i]) + " is linked to a record column (nfk_link_record): "
                                     "its value is its link's");
    }
    const size_t at = w->xops.size();
    w->xops.resize(at + (size_t)n);
    World::XOp* x = w->xops.data() + at;
    for (int32_t i = 0; i < n; i++) {
        x[i] = World::XOp{(uint32_t)obj[i], (uint32_t)pid[i], bits[i]};
        count_standalone(w, (uint32_t)pid[i]);
    }
    if (w->cfg.n_obj) w->xops_h.resize(w->xops.size(), 0);
    return NFK_OK;
}

// object indices as the caller holds them (nfk's creation order, the outputs' ev_obj / fi_obj):
// -1 for one that is not a live object of this world
static const int32_t* live_objects(World* w, int32_t n, const int32_t* obj) {
    w->look.resize(n);
    for (int32_t i = 0; i < n; i++) {
        const int32_t o = obj[i];
        w->look[i] = (o >= 0 && o < w->n_obj && w->alive[o]) ? o : -1;
    }
    return w->look.data();
}

int nfk_set_props(void* world, int32_t n, const int64_t* gh, const int64_t* gd, const int32_t* pid,
                  const uint64_t* bits) {
    World* w = (World*)world;
    if (!w || n < 0 || (n && (!gh || !gd || !pid || !bits))) return fail(NFK_ERR_ARG, "null argument");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    if (w->lk_pids[0] | w->lk_pids[1])  // a direct Set of a linked property: refused, nothing queued
        for (int32_t i = 0; i < n; i++)
            if (w->linked_pid(pid[i]))
                return fail(NFK_ERR_ARG, "property " + std::to_string(pid[i]) + " is linked to a record column (nfk_link_record): "
                                         "its value is its link's");
    // a large batch in a world without object properties: looked up and queued on the device
    if (w->dev_look_min && (size_t)n >= w->dev_look_min && w->cfg.n_obj == 0) return set_props_dev(w, n, gh, gd, pid, bits);
    w->look.resize(n);  // one GUID lookup per call
    if (int rl = find_many_par(w, n, gh, gd, w->look.data())) return rl;
    return queue_sets(w, n, w->look.data(), pid, bits, gh, gd);
}

int nfk_set_props_obj(void* world, int32_t n, const int32_t* obj, const int32_t* pid, const uint64_t* bits) {
    World* w = (World*)world;
    if (!w || n < 0 || (n && (!obj || !pid || !bits))) return fail(NFK_ERR_ARG, "null argument");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    return queue_sets(w, n, live_objects(w, n, obj), pid, bits, nullptr, nullptr);
}

int nfk_set_objects(void* world, int32_t n, const int64_t* gh, const int64_t* gd, const int32_t* pid,
                    const int64_t* vh, const int64_t* vd) {
    World* w = (World*)world;
    if (!w || n < 0 || (n && (!gh || !gd || !pid || !vh || !vd))) return fail(NFK_ERR_ARG, "null argument");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    w->look.resize(n);
    if (int rl = find_many_par(w, n, gh, gd, w->look.data())) return rl;
    for (int32_t i = 0; i < n; i++) {
        if (w->look[i] < 0)  // "There is no object" (KM:370)
            return fail(NFK_ERR_NOTFOUND, "no object " + std::to_string(gh[i]) + "-" + std::to_string(gd[i]));
        if (pid[i] < w->n_if || pid[i] >= w->n_prop) return fail(NFK_ERR_ARG, "not an object property");
    }
    // one queue with the int / f64 Sets: the call order across properties is kept
    w->xops_h.resize(w->xops.size(), 0);
    for (int32_t i = 0; i < n; i++) {
        w->xops.push_back(World::XOp{(uint32_t)w->look[i], (uint32_t)pid[i], (uint64_t)vd[i]});
        w->xops_h.push_back((uint64_t)vh[i]);
        count_standalone(w, (uint32_t)pid[i]);
    }
    return NFK_OK;
}

int nfk_set_records(void* world, int32_t n, const int64_t* gh, const int64_t* gd, const int32_t* rec,
                    const int32_t* row, const int32_t* col, const uint8_t* is_float, const uint64_t* bits) {
    World* w = (World*)world;
    if (!w || n < 0 || (n && (!gh || !gd || !rec || !row || !col || !bits))) return fail(NFK_ERR_ARG, "null argument");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    // every call is checked before any is queued; one GUID lookup per call
    w->look.resize(n);
    if (int rl = find_many_par(w, n, gh, gd, w->look.data())) return rl;
    for (int32_t i = 0; i < n; i++) {
        if (w->look[i] < 0)  // NFCKernelModule logs "There is no object" and returns false (KM:505)
            return fail(NFK_ERR_NOTFOUND, "no object " + std::to_string(gh[i]) + "-" + std::to_string(gd[i]));
        const int32_t r = rec[i];
        if (r < 0 || r >= w->cfg.n_rec || !w->rec_defined[r] || row[i] < 0 || row[i] >= w->tab.rec_rows[r] ||
            col[i] < 0 || col[i] >= w->tab.rec_cols[r])
            return fail(NFK_ERR_ARG, "record cell out of range");
    }
    w->rsq.reserve(w->rsq.size() + n);
    for (int32_t i = 0; i < n; i++) {
        // NFCRecord::SetInt / SetFloat on a column of the other type write nothing (RC:189 / RC:250)
        // a half of an object column takes neither (nothing writes one half of a pair alone)
        const int ct = w->rec_ctype[rec[i]][col[i]];
        if (ct >= NFK_REC_OBJ_DATA || (is_float && (is_float[i] != 0) != (ct == NFK_REC_F64))) continue;
        w->rq_index[((uint64_t)w->look[i] << 3) | (uint32_t)rec[i]].push_back((uint32_t)w->rsq.size());
        w->rsq.push_back(World::RSOp{(uint32_t)w->look[i], ((uint32_t)rec[i] << 16) | ((uint32_t)row[i] << 8) | (uint32_t)col[i],
                                     bits[i], 0u, 0u});
    }
    return NFK_OK;
}

int nfk_set_record_objects(void* world, int32_t n, const int64_t* gh, const int64_t* gd, const int32_t* rec,
                           const int32_t* row, const int32_t* col, const int64_t* vh, const int64_t* vd) {
    World* w = (World*)world;
    if (!w || n < 0 || (n && (!gh || !gd || !rec || !row || !col || !vh || !vd))) return fail(NFK_ERR_ARG, "null argument");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    w->look.resize(n);
    if (int rl = find_many_par(w, n, gh, gd, w->look.data())) return rl;
    for (int32_t i = 0; i < n; i++) {
        if (w->look[i] < 0)  // "There is no object" (KM: SetRecordObject)
            return fail(NFK_ERR_NOTFOUND, "no object " + std::to_string(gh[i]) + "-" + std::to_string(gd[i]));
        const int32_t r = rec[i];
        if (r < 0 || r >= w->cfg.n_rec || !w->rec_defined[r] || row[i] < 0 || row[i] >= w->tab.rec_rows[r] ||
            col[i] < 0 || col[i] >= w->tab.rec_cols[r])
            return fail(NFK_ERR_ARG, "record cell out of range");
        if (w->rec_ctype[r][col[i]] != NFK_REC_OBJ_DATA)
            return fail(NFK_ERR_ARG, "not the data half of an object column");
    }
    // one queue with the int / f64 Sets and the row operations: the call order on a record is kept
    w->rsq.reserve(w->rsq.size() + n);
    w->rsq_h.resize(w->rsq.size(), 0);
    for (int32_t i = 0; i < n; i++) {
        w->rq_index[((uint64_t)w->look[i] << 3) | (uint32_t)rec[i]].push_back((uint32_t)w->rsq.size());
        w->rsq.push_back(World::RSOp{(uint32_t)w->look[i], ((uint32_t)rec[i] << 16) | ((uint32_t)row[i] << 8) | (uint32_t)col[i],
                                     (uint64_t)vd[i], 0u, 0u});
        w->rsq_h.push_back((uint64_t)vh[i]);
    }
    return NFK_OK;
}

int nfk_record_rows(void* world, int32_t n, const int64_t* gh, const int64_t* gd, const int32_t* rec, const int32_t* op,
                    const int32_t* row, const uint64_t* values) {
    World* w = (World*)world;
    if (!w || n < 0 || (n && (!gh || !gd || !rec || !op || !row))) return fail(NFK_ERR_ARG, "null argument");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    w->look.resize(n);
    if (int rl = find_many_par(w, n, gh, gd, w->look.data())) return rl;
    for (int32_t i = 0; i < n; i++) {
        if (w->look[i] < 0)  // FindRecord: "There is no object" (KM:487)
            return fail(NFK_ERR_NOTFOUND, "no object " + std::to_string(gh[i]) + "-" + std::to_string(gd[i]));
        const int32_t r = rec[i];
        if (r < 0 || r >= w->cfg.n_rec || !w->rec_defined[r] || op[i] < 1 || op[i] > 3)
            return fail(NFK_ERR_ARG, "bad record or row operation");
        if ((op[i] == 1 && (row[i] < -1 || row[i] >= w->tab.rec_rows[r])) ||
            (op[i] == 2 && (row[i] < 0 || row[i] >= w->tab.rec_rows[r])))
            return fail(NFK_ERR_ARG, "row out of range");
    }
    for (int32_t i = 0; i < n; i++) {
        uint32_t aux = 0;
        const uint32_t rr = op[i] == 3 ? 0u : (row[i] < 0 ? 0xFFu : (uint32_t)row[i]);
        if (op[i] == 1) {
            aux = 0xFFFFFFFFu;
            if (values) {
                aux = (uint32_t)(w->rvals.size() / NFK_MAX_REC_COLS);
                w->rvals.insert(w->rvals.end(), values + (size_t)i * NFK_MAX_REC_COLS,
                                values + (size_t)(i + 1) * NFK_MAX_REC_COLS);
            }
        }
        w->rq_index[((uint64_t)w->look[i] << 3) | (uint32_t)rec[i]].push_back((uint32_t)w->rsq.size());
        w->rsq.push_back(World::RSOp{(uint32_t)w->look[i], ((uint32_t)rec[i] << 16) | (rr << 8), 0ull, (uint32_t)op[i], aux});
    }
    return NFK_OK;
}

// NFCRecord::SwapRowInfo (RC:1219-1253), queued with the record's other calls (World::rsq, op 4: the
// row field the origin, the col field the target row)
int nfk_swap_rows(void* world, int32_t n, const int64_t* gh, const int64_t* gd, const int32_t* rec,
                  const int32_t* row_origin, const int32_t* row_target) {
    World* w = (World*)world;
    if (!w || n < 0 || (n && (!gh || !gd || !rec || !row_origin || !row_target))) return fail(NFK_ERR_ARG, "null argument");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    w->look.resize(n);
    if (int rl = find_many_par(w, n, gh, gd, w->look.data())) return rl;
    for (int32_t i = 0; i < n; i++) {
        if (w->look[i] < 0)  // FindRecord: "There is no object" (KM:487)
            return fail(NFK_ERR_NOTFOUND, "no object " + std::to_string(gh[i]) + "-" + std::to_string(gd[i]));
        const int32_t r = rec[i];
        if (r < 0 || r >= w->cfg.n_rec || !w->rec_defined[r]) return fail(NFK_ERR_ARG, "bad record");
        if (row_origin[i] < 0 || row_origin[i] >= w->tab.rec_rows[r] || row_target[i] < 0 ||
            row_target[i] >= w->tab.rec_rows[r])
            return fail(NFK_ERR_ARG, "row out of range");
    }
    w->rsq.reserve(w->rsq.size() + n);
    for (int32_t i = 0; i < n; i++) {
        w->rq_index[((uint64_t)w->look[i] << 3) | (uint32_t)rec[i]].push_back((uint32_t)w->rsq.size());
        w->rsq.push_back(World::RSOp{(uint32_t)w->look[i],
                                     ((uint32_t)rec[i] << 16) | ((uint32_t)row_origin[i] << 8) | (uint32_t)row_target[i], 0ull,
                                     4u, 0u});
    }
    return NFK_OK;
}

// device address of object o's used-row mask of record r (its import row in this window, or its slot)
static int used_addr(World* w, int32_t o, int32_t r, const uint64_t** used) {
    const int rows = w->tab.rec_rows[r], cols = w->tab.rec_cols[r];
    if (w->src_row[o] >= 0) {
        int64_t off = w->n_pw + 4 * w->cfg.n_kind;
        for (int x = 0; x < r; x++) off += (int64_t)w->tab.rec_rows[x] * w->tab.rec_cols[x] + 1;
        *used = w->ins_rows + (size_t)w->src_row[o] * w->row_words + off + (size_t)rows * cols;
    } else if (w->slot_of_obj[o] >= 0) {
        *used = w->d.rused[r] + w->slot_of_obj[o];
    } else {
        return fail(NFK_ERR_STATE, "object without a slot");
    }
    return NFK_OK;
}

// 8-byte device words at absolute addresses (waits for the world's stream)
static int read_abs(World* w, const std::vector<uint64_t>& addr, uint64_t* got) {
    if (addr.empty()) return NFK_OK;
    HIPCHK(hipStreamSynchronize(w->stream));
    if (addr.size() <= 4) {
        for (size_t q = 0; q < addr.size(); q++)
            HIPCHK(hipMemcpy(&got[q], (const void*)(uintptr_t)addr[q], 8, hipMemcpyDeviceToHost));
        return NFK_OK;
    }
    int r = dev_reserve(w, (void**)&w->gat, &w->gat_cap, addr.size() * 16);
    if (r) return r;
    HIPCHK(hipMemcpy(w->gat, addr.data(), addr.size() * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_gather_abs, dim3((unsigned)((addr.size() + kTPB - 1) / kTPB)), dim3(kTPB), 0, w->stream,
                       (const uint64_t*)w->gat, (int32_t)addr.size(), w->gat + addr.size());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(got, w->gat + addr.size(), addr.size() * 8, hipMemcpyDeviceToHost, w->stream));
    HIPCHK(hipStreamSynchronize(w->stream));
    return NFK_OK;
}

// the queued row operations of (object o, record r) replayed on a used-row mask
static uint64_t replay_rows(const World* w, int32_t o, int32_t r, uint64_t u) {
    auto it = w->rq_index.find(((uint64_t)o << 3) | (uint32_t)r);
    if (it == w->rq_index.end()) return u;
    const int rows = w->tab.rec_rows[r];
    for (uint32_t k : it->second) {
        const World::RSOp& x = w->rsq[k];
        const int xr = (int)((x.rrc >> 8) & 0xFF);
        if (x.op == 1) {
            if (xr == 0xFF) {
                const uint64_t fr = ~u & (rows >= 64 ? ~0ull : ((1ull << rows) - 1));
                if (fr) u |= fr & (~fr + 1);
            } else {
                u |= 1ull << xr;
            }
        } else if (x.op == 2) {
            u &= ~(1ull << xr);
        } else if (x.op == 3) {
            u = 0;
        } else if (x.op == 4) {  // SwapRowInfo: a used origin's bit and the target's change places
            const int xt = (int)(x.rrc & 0xFF);
            if ((u >> xr) & 1) u = (u & ~(1ull << xr)) | (((u >> xt) & 1) << xr) | (1ull << xt);
        }
    }
    return u;
}

int nfk_get_used_rows(void* world, int32_t n, const int64_t* gh, const int64_t* gd, const int32_t* rec, uint64_t* masks) {
    World* w = (World*)world;
    if (!w || n < 0 || (n && (!gh || !gd || !rec || !masks))) return fail(NFK_ERR_ARG, "null argument");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    std::vector<int32_t> obj(n);
    if (int rl = find_many_par(w, n, gh, gd, obj.data())) return rl;
    std::vector<uint64_t> addr;
    std::vector<int32_t> miss;
    for (int32_t i = 0; i < n; i++) {
        if (obj[i] < 0) return fail(NFK_ERR_NOTFOUND, "There is no object " + std::to_string(gh[i]) + "-" + std::to_string(gd[i]));
        if (rec[i] < 0 || rec[i] >= w->cfg.n_rec || !w->rec_defined[rec[i]]) return fail(NFK_ERR_ARG, "bad record");
        auto it = w->ucache.find(((uint64_t)obj[i] << 3) | (uint32_t)rec[i]);
        if (it != w->ucache.end()) {
            masks[i] = it->second;
            continue;
        }
        const uint64_t* u;
        int r = used_addr(w, obj[i], rec[i], &u);
        if (r) return r;
        addr.push_back((uint64_t)(uintptr_t)u);
        miss.push_back(i);
    }
    std::vector<uint64_t> got(addr.size());
    int r = read_abs(w, addr, got.data());
    if (r) return r;
    for (size_t q = 0; q < miss.size(); q++) {
        masks[miss[q]] = got[q];
        w->ucache[((uint64_t)obj[miss[q]] << 3) | (uint32_t)rec[miss[q]]] = got[q];
    }
    for (int32_t i = 0; i < n; i++) masks[i] = replay_rows(w, obj[i], rec[i], masks[i]);
    return NFK_OK;
}

// This window's queued calls on (object o, record r) replayed in call order on its used-row mask u
// and on column col's cells c[rows] in ROW order: SetRecord* through RC:182 / RC:243 on the row's
// used state at that call, AddRow / Remove / ClearRecord on the mask (RC:111, RC:1086, RC:1109).  A
// Remove leaves the cell's value behind (RC:1086-1107); an AddRow without values writes 0.  A
// SwapRowInfo of a used origin exchanges the two rows' cells and used bits (RC:1219-1253), so a
// row's result depends on other rows' cells: a caller hands in the cells of every row the device
// holds as used whenever the list holds a Swap (list_swaps).  Shared by nfk_get_records and
// nfk_find_rows.
// The pair form (ch != null, col the data half of an object column): c the data halves, ch the head
// halves; SetRecordObject writes both (RC:367-421), AddRow both words of its values.  Without ch a
// half column replays as the word it is (nfk_get_records): a queued SetRecordObject is named by its
// data half's column and writes the head column's word too.
static void replay_column(const World* w, int32_t o, int32_t r, int32_t col, uint64_t& u, uint64_t* c,
                          uint64_t* ch = nullptr) {
    auto it = w->rq_index.find(((uint64_t)o << 3) | (uint32_t)r);
    if (it == w->rq_index.end()) return;
    const int32_t rows = w->tab.rec_rows[r];
    const int ct = w->rec_ctype[r][col];
    const int setc = ct == NFK_REC_OBJ_HEAD ? col - 1 : col;  // the column a Set of this cell names
    for (uint32_t k : it->second) {
        const World::RSOp& x = w->rsq[k];
        const int xr = (int)((x.rrc >> 8) & 0xFF), xc = (int)(x.rrc & 0xFF);
        if (x.op == 0) {
            if (xc != setc || !((u >> xr) & 1)) continue;
            const uint64_t b = x.bits;
            if (ct >= NFK_REC_OBJ_DATA) {
                c[xr] = ct == NFK_REC_OBJ_HEAD ? w->rsq_head(k) : b;
                if (ch) ch[xr] = w->rsq_head(k);
            } else if (ct == NFK_REC_F64) {
                double bd, cd;
                memcpy(&bd, &b, 8);
                memcpy(&cd, &c[xr], 8);
                const double df = bd - cd;
                if (!(df < 0.001 && df > -0.001)) c[xr] = b;
            } else {
                c[xr] = b;
            }
        } else if (x.op == 1) {
            int rr = xr;
            if (xr == 0xFF) {
                const uint64_t fr = ~u & (rows >= 64 ? ~0ull : ((1ull << rows) - 1));
                if (!fr) continue;
                rr = __builtin_ctzll(fr);
            }
            u |= 1ull << rr;
            c[rr] = x.aux == 0xFFFFFFFFu ? 0ull : w->rvals[(size_t)x.aux * NFK_MAX_REC_COLS + col];
            if (ch) ch[rr] = x.aux == 0xFFFFFFFFu ? 0ull : w->rvals[(size_t)x.aux * NFK_MAX_REC_COLS + col + 1];
        } else if (x.op == 2) {
            u &= ~(1ull << xr);
        } else if (x.op == 3) {
            u = 0;
        } else if ((u >> xr) & 1) {  // SwapRowInfo (the col field: the target row)
            std::swap(c[xr], c[xc]);
            if (ch) std::swap(ch[xr], ch[xc]);
            u = (u & ~(1ull << xr)) | (((u >> xc) & 1) << xr) | (1ull << xc);
        }
    }
}

// The link of column col of record r (nfk_link_record) over this window's queued calls on (object
// o, record r), as k_rrows takes it: the calls replayed in call order on the used mask u and the
// column's int cells c[rows] in ROW order; every record event whose nCol names the column — an
// accepted Set of one of its cells; with col 0 an AddRow, a Remove (before the row goes) and each step
// of a ClearRecord; a Swap whose target row's index is col — takes the sum of the column over the
// link's rows, each cell truncated to int32, unused rows 0.  True when an event named the column:
// *sum is the last one's.
static bool replay_link(const World* w, int32_t o, int32_t r, int32_t col, uint64_t u, uint64_t* c, uint32_t* sum) {
    auto it = w->rq_index.find(((uint64_t)o << 3) | (uint32_t)r);
    if (it == w->rq_index.end()) return false;
    const int32_t rows = w->tab.rec_rows[r], rows_l = std::min<int32_t>(w->lk_rows[r], rows);
    bool hit = false;
    auto event = [&]() {
        uint32_t s = 0;
        for (int i = 0; i < rows_l; i++) s += ((u >> i) & 1) ? (uint32_t)c[i] : 0u;
        *sum = s;
        hit = true;
    };
    for (uint32_t k : it->second) {
        const World::RSOp& x = w->rsq[k];
        const int xr = (int)((x.rrc >> 8) & 0xFF), xc = (int)(x.rrc & 0xFF);
        if (x.op == 0) {
            if (xc != col || !((u >> xr) & 1) || c[xr] == x.bits) continue;  // RC:194, RC:209
            c[xr] = x.bits;
            event();
        } else if (x.op == 1) {
            int rr = xr;
            if (xr == 0xFF) {
                const uint64_t fr = ~u & rec_rowm(rows);
                if (!fr) continue;
                rr = __builtin_ctzll(fr);
            }
            u |= 1ull << rr;
            c[rr] = x.aux == 0xFFFFFFFFu ? 0ull : w->rvals[(size_t)x.aux * NFK_MAX_REC_COLS + col];
            if (col == 0) event();
        } else if (x.op == 2) {
            if (!((u >> xr) & 1)) continue;
            if (col == 0) event();
            u &= ~(1ull << xr);
        } else if (x.op == 3) {
            for (int q = rows - 1; q >= 0; q--)
                if ((u >> q) & 1) {
                    if (col == 0) event();
                    u &= ~(1ull << q);
                }
        } else if ((u >> xr) & 1) {  // SwapRowInfo (the col field: the target row)
            std::swap(c[xr], c[xc]);
            u = (u & ~(1ull << xr)) | (((u >> xc) & 1) << xr) | (1ull << xc);
            if (xc == col) event();
        }
    }
    return hit;
}

// whether the window's queued calls on (object o, record r) hold a SwapRowInfo
static bool list_swaps(const World* w, int32_t o, int32_t r) {
    auto it = w->rq_index.find(((uint64_t)o << 3) | (uint32_t)r);
    if (it == w->rq_index.end()) return false;
    for (uint32_t k : it->second)
        if (w->rsq[k].op == 4) return true;
    return false;
}

// nfk_get_records (heads null: the cells as the words they are) and nfk_get_record_objects (heads:
// the cells' head halves, bits their data halves; col names the data half, checked before anything
// is read): one lookup per query, the masks in one gather, both words of a pair in the second
static int get_record_cells(World* w, int32_t n, const int64_t* gh, const int64_t* gd, const int32_t* rec,
                            const int32_t* row, const int32_t* col, uint64_t* bits, uint64_t* heads) {
    std::vector<int32_t> obj(n);
    if (int rl = find_many_par(w, n, gh, gd, obj.data())) return rl;
    for (int32_t i = 0; i < n; i++) {
        if (obj[i] < 0) return fail(NFK_ERR_NOTFOUND, "There is no object " + std::to_string(gh[i]) + "-" + std::to_string(gd[i]));
        const int32_t r = rec[i];
        if (r < 0 || r >= w->cfg.n_rec || !w->rec_defined[r] || row[i] < 0 || row[i] >= w->tab.rec_rows[r] ||
            col[i] < 0 || col[i] >= w->tab.rec_cols[r])
            return fail(NFK_ERR_ARG, "record cell out of range");
        if (heads && w->rec_ctype[r][col[i]] != NFK_REC_OBJ_DATA)
            return fail(NFK_ERR_ARG, "not the data half of an object column");
    }
    // every query's used-row mask (this window's cache, else one gather), then the cells of the
    // rows the device holds as used in a second: a cell's place in its vector follows from the
    // mask (rec_pos); a row the device holds unused reads 0 unless a queued AddRow writes it
    std::vector<uint64_t> um(n), cv(n, 0), hv(heads ? n : 0, 0), swv;
    std::vector<uint8_t> swl(n, 0);   // the query's list holds a SwapRowInfo (list_swaps)
    std::vector<size_t> sw_at(n, 0);  // such a query's cells in swv
    for (int32_t i = 0; i < n; i++) swl[i] = list_swaps(w, obj[i], rec[i]);
    {
        std::vector<uint64_t> addr;
        std::vector<int32_t> miss;
        for (int32_t i = 0; i < n; i++) {
            auto it = w->ucache.find(((uint64_t)obj[i] << 3) | (uint32_t)rec[i]);
            if (it != w->ucache.end()) {
                um[i] = it->second;
                continue;
            }
            const uint64_t* u;
            if (int r = used_addr(w, obj[i], rec[i], &u)) return r;
            addr.push_back((uint64_t)(uintptr_t)u);
            miss.push_back(i);
        }
        std::vector<uint64_t> got(addr.size());
        if (int r = read_abs(w, addr, got.data())) return r;
        for (size_t q = 0; q < miss.size(); q++) {
            um[miss[q]] = got[q];
            w->ucache[((uint64_t)obj[miss[q]] << 3) | (uint32_t)rec[miss[q]]] = got[q];
        }
    }
    {
        std::vector<uint64_t> addr;
        std::vector<int32_t> at;
        for (int32_t i = 0; i < n; i++) {
            const int32_t o = obj[i], r = rec[i], rows = w->tab.rec_rows[r], cols = w->tab.rec_cols[r];
            // a list with a SwapRowInfo: the cell may come from any row, so every used row's is read
            const bool sw = swl[i];
            if (sw ? !(um[i] & rec_rowm(rows)) : !((um[i] >> row[i]) & 1)) continue;
            const size_t place = (size_t)col[i] * rows + (sw ? 0 : rec_pos(um[i], rec_rowm(rows), row[i]));
            const uint64_t* cell;
            if (w->src_row[o] >= 0) {  // entered in this window: its row of the import buffer
                int64_t off = w->n_pw + 4 * w->cfg.n_kind;
                for (int x = 0; x < r; x++) off += (int64_t)w->tab.rec_rows[x] * w->tab.rec_cols[x] + 1;
                cell = w->ins_rows + (size_t)w->src_row[o] * w->row_words + off + place;
            } else if (w->slot_of_obj[o] >= 0) {
                cell = w->d.rcells[r] + (size_t)w->slot_of_obj[o] * cols * rows + place;
            } else {
                return fail(NFK_ERR_STATE, "object without a slot");
            }
            // (the used rows first, in row order: rec_pos; a pair's head half at the same place of the next vector)
            const int np = sw ? __builtin_popcountll(um[i] & rec_rowm(rows)) : 1;
            for (int p = 0; p < np; p++) {
                addr.push_back((uint64_t)(uintptr_t)(cell + p));
                if (heads) addr.push_back((uint64_t)(uintptr_t)(cell + p + rows));
            }
            at.push_back(i);
        }
        std::vector<uint64_t> got(addr.size());
        if (int r = read_abs(w, addr, got.data())) return r;
        size_t g = 0;
        for (size_t q = 0; q < at.size(); q++) {
            const int32_t i = at[q];
            if (swl[i]) {
                sw_at[i] = g;
                g += (size_t)__builtin_popcountll(um[i] & rec_rowm(w->tab.rec_rows[rec[i]])) * (heads ? 2 : 1);
                continue;
            }
            cv[i] = got[g++];
            if (heads) hv[i] = got[g++];
        }
        swv.swap(got);
    }
    for (int32_t i = 0; i < n; i++) {
        uint64_t u = um[i], c[64] = {}, ch[64] = {};
        if (swl[i]) {
            size_t g = sw_at[i];
            for (int rr = 0; rr < w->tab.rec_rows[rec[i]]; rr++)
                if ((u >> rr) & 1) {
                    c[rr] = swv[g++];
                    if (heads) ch[rr] = swv[g++];
                }
        } else {
            c[row[i]] = cv[i];
            if (heads) ch[row[i]] = hv[i];
        }
        replay_column(w, obj[i], rec[i], col[i], u, c, heads ? ch : nullptr);
        // NFCRecord::GetInt / GetFloat / GetObject of an unused row (RC:623, RC:704): 0 / NULL_OBJECT
        bits[i] = ((u >> row[i]) & 1) ? c[row[i]] : 0;
        if (heads) heads[i] = ((u >> row[i]) & 1) ? ch[row[i]] : 0;
    }
    return NFK_OK;
}

int nfk_get_records(void* world, int32_t n, const int64_t* gh, const int64_t* gd, const int32_t* rec,
                    const int32_t* row, const int32_t* col, uint64_t* bits) {
    World* w = (World*)world;
    if (!w || n < 0 || (n && (!gh || !gd || !rec || !row || !col || !bits))) return fail(NFK_ERR_ARG, "null argument");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    return get_record_cells(w, n, gh, gd, rec, row, col, bits, nullptr);
}

int nfk_get_record_objects(void* world, int32_t n, const int64_t* gh, const int64_t* gd, const int32_t* rec,
                           const int32_t* row, const int32_t* col, int64_t* vh, int64_t* vd) {
    World* w = (World*)world;
    if (!w || n < 0 || (n && (!gh || !gd || !rec || !row || !col || !vh || !vd))) return fail(NFK_ERR_ARG, "null argument");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    return get_record_cells(w, n, gh, gd, rec, row, col, (uint64_t*)vd, (uint64_t*)vh);
}

// ---- record finds (nfk_find_rows): NFCRecord::FindInt / FindFloat (RC:830-899) ----
// device addresses of object o's record r: its cells [cols][rows] and its used-row mask (its row of
// the import buffer when it entered in this window, else its slot; used_addr)
static int rec_addrs(World* w, int32_t o, int32_t r, const uint64_t** cells, const uint64_t** used) {
    const size_t rows = (size_t)w->tab.rec_rows[r], cols = (size_t)w->tab.rec_cols[r];
    if (w->src_row[o] >= 0) {
        int64_t off = w->n_pw + 4 * w->cfg.n_kind;
        for (int x = 0; x < r; x++) off += (int64_t)w->tab.rec_rows[x] * w->tab.rec_cols[x] + 1;
        *cells = w->ins_rows + (size_t)w->src_row[o] * w->row_words + off;
        *used = *cells + rows * cols;
    } else if (w->slot_of_obj[o] >= 0) {
        *cells = w->d.rcells[r] + (size_t)w->slot_of_obj[o] * cols * rows;
        *used = w->d.rused[r] + w->slot_of_obj[o];
    } else {
        return fail(NFK_ERR_STATE, "object without a slot");
    }
    return NFK_OK;
}

// the finds of resolved objects (obj[i] < 0: unknown; gh / gd for the message, or null); heads: the
// arguments' NFGUID head halves (bits: the data halves) of a FindObject batch (k_find_objects), null
// for FindInt / FindFloat (k_find_rows)
static int find_rows(World* w, int32_t n, const int32_t* obj, const int64_t* gh, const int64_t* gd, const int32_t* rec,
                     const int32_t* col, const uint64_t* bits, uint64_t* masks, const uint64_t* heads = nullptr) {
    w->f_kernel_ms = 0;
    w->f_bytes = 0;
    w->f_host = 0;
    int max_rows = 1;
    for (int32_t i = 0; i < n; i++) {
        if (obj[i] < 0)
            return fail(NFK_ERR_NOTFOUND, gh ? "There is no object " + std::to_string(gh[i]) + "-" + std::to_string(gd[i])
                                             : "no object index");
        const int32_t r = rec[i];
        if (r < 0 || r >= w->cfg.n_rec || !w->rec_defined[r]) return fail(NFK_ERR_ARG, "bad record");
        if (col[i] < 0 || col[i] >= w->tab.rec_cols[r]) return fail(NFK_ERR_ARG, "record column out of range");
        const int ct = w->rec_ctype[r][col[i]];
        if (heads ? ct != NFK_REC_OBJ_DATA : ct >= NFK_REC_OBJ_DATA)
            return fail(NFK_ERR_ARG, heads ? "not the data half of an object column"
                                           : "a half of an object column (nfk_find_objects finds NFGUIDs)");
        max_rows = std::max(max_rows, (int)w->tab.rec_rows[r]);
    }
    if (n == 0) return NFK_OK;
    int lg = 0;
    while ((1 << lg) < max_rows) lg++;  // (rows <= 64: lg <= 6)

    // descriptors in pinned memory, the masks behind them; a query whose record has queued calls
    // in this window is left out of the batch (host: below)
    const size_t dsz = heads ? sizeof(FindObjDev) : sizeof(FindDev);
    const size_t o_m = align16((size_t)n * dsz), tot = o_m + (size_t)n * 8;
    if (int r = dev_reserve(w, &w->f_dev, &w->f_dcap, tot)) return r;
    if (tot > w->f_pcap) {
        if (w->f_pin) HIPCHK(hipHostFree(w->f_pin));
        w->f_pin = nullptr;
        const size_t c = std::max(tot, w->f_pcap + w->f_pcap / 2);
        w->f_pcap = 0;  // (until the new buffer exists)
        HIPCHK(hipHostMalloc((void**)&w->f_pin, c, hipHostMallocDefault));
        w->f_pcap = c;
    }
    FindDev* hq = (FindDev*)w->f_pin;
    FindObjDev* hqo = (FindObjDev*)w->f_pin;
    const uint64_t* hm = (const uint64_t*)(w->f_pin + o_m);
    std::vector<int32_t> host;  // queries answered on the host
    const bool queued = !w->rq_index.empty();
    int32_t nd = 0;
    for (int32_t i = 0; i < n; i++) {
        const int32_t o = obj[i], r = rec[i];
        if (queued && w->rq_index.count(((uint64_t)o << 3) | (uint32_t)r)) {
            host.push_back(i);
            continue;
        }
        const uint64_t *cells, *used;
        if (int e = rec_addrs(w, o, r, &cells, &used)) return e;
        if (heads) {
            FindObjDev f;
            f.used = (uint64_t)(uintptr_t)used;
            f.colv = (uint64_t)(uintptr_t)(cells + (size_t)col[i] * w->tab.rec_rows[r]);
            f.arg_d = bits[i];
            f.arg_h = heads[i];
            f.rows = w->tab.rec_rows[r];
            f.pad = 0;
            hqo[nd++] = f;
            continue;
        }
        FindDev f;
        f.used = (uint64_t)(uintptr_t)used;
        f.colv = (uint64_t)(uintptr_t)(cells + (size_t)col[i] * w->tab.rec_rows[r]);
        f.rows = w->tab.rec_rows[r];
        f.flt = w->rec_ctype[r][col[i]] == NFK_REC_F64 ? 1 : 0;
        f.arg = bits[i];
        hq[nd++] = f;
    }
    if (nd) {
        char* D = (char*)w->f_dev;
        const bool timed = w->profiling;
        if (timed)
            for (auto& e : w->f_ev)
                if (!e) HIPCHK(hipEventCreate(&e));
        HIPCHK(hipMemcpyAsync(D, w->f_pin, (size_t)nd * dsz, hipMemcpyHostToDevice, w->stream));
        if (timed) HIPCHK(hipEventRecord(w->f_ev[0], w->stream));
        const int64_t threads = (int64_t)nd << lg;
        if (heads)
            hipLaunchKernelGGL(k_find_objects, dim3((unsigned)((threads + kTPB - 1) / kTPB)), dim3(kTPB), 0, w->stream,
                               (const FindObjDev*)D, nd, lg, (uint64_t*)(D + o_m));
        else
            hipLaunchKernelGGL(k_find_rows, dim3((unsigned)((threads + kTPB - 1) / kTPB)), dim3(kTPB), 0, w->stream,
                               (const FindDev*)D, nd, lg, (uint64_t*)(D + o_m));
        HIPCHK(hipGetLastError());
        if (timed) HIPCHK(hipEventRecord(w->f_ev[1], w->stream));
        HIPCHK(hipMemcpyAsync(w->f_pin + o_m, D + o_m, (size_t)nd * 8, hipMemcpyDeviceToHost, w->stream));
        HIPCHK(hipStreamSynchronize(w->stream));
        w->f_bytes = (int64_t)nd * 8;
        if (timed) {
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, w->f_ev[0], w->f_ev[1]));
            w->f_kernel_ms = ms;
        }
        if (host.empty()) {
            memcpy(masks, hm, (size_t)n * 8);
        } else {
            size_t h = 0;
            int32_t k = 0;
            for (int32_t i = 0; i < n; i++) {
                if (h < host.size() && host[h] == i) h++;
                else masks[i] = hm[k++];
            }
        }
    }
    if (host.empty()) return NFK_OK;

    // read-your-writes: the device's mask and the column's used cells (two gathers for all of
    // them), the cells put in row order, the queued calls replayed, then the comparison
    w->f_host = (int32_t)host.size();
    std::vector<uint64_t> addr(host.size()), um(host.size());
    std::vector<const uint64_t*> colv(host.size());
    for (size_t j = 0; j < host.size(); j++) {
        const int32_t i = host[j];
        const uint64_t *cells, *used;
        if (int e = rec_addrs(w, obj[i], rec[i], &cells, &used)) return e;
        addr[j] = (uint64_t)(uintptr_t)used;
        colv[j] = cells + (size_t)col[i] * w->tab.rec_rows[rec[i]];
    }
    if (int e = read_abs(w, addr, um.data())) return e;
    addr.clear();
    for (size_t j = 0; j < host.size(); j++) {
        const int rows = w->tab.rec_rows[rec[host[j]]];
        um[j] &= rec_rowm(rows);
        const int np = __builtin_popcountll(um[j]);
        for (int p = 0; p < np; p++) addr.push_back((uint64_t)(uintptr_t)(colv[j] + p));
        // (an object find: the head halves, the same places of the next column vector)
        for (int p = 0; heads && p < np; p++) addr.push_back((uint64_t)(uintptr_t)(colv[j] + rows + p));
    }
    std::vector<uint64_t> cv(addr.size());
    if (int e = read_abs(w, addr, cv.data())) return e;
    size_t at = 0;
    for (size_t j = 0; j < host.size(); j++) {
        const int32_t i = host[j], r = rec[i], rows = w->tab.rec_rows[r];
        uint64_t u = um[j], c[64] = {};
        for (int row = 0; row < rows; row++)
            if ((u >> row) & 1) c[row] = cv[at++];  // (the used rows first, in row order: rec_pos)
        if (heads) {  // NFCRecord::FindObject (RC:957-987): both halves, on the used rows
            uint64_t ch[64] = {};
            for (int row = 0; row < rows; row++)
                if ((u >> row) & 1) ch[row] = cv[at++];
            replay_column(w, obj[i], r, col[i], u, c, ch);
            uint64_t m = 0;
            for (int row = 0; row < rows; row++)
                m |= (uint64_t)(((u >> row) & 1) && c[row] == bits[i] && ch[row] == heads[i]) << row;
            masks[i] = m;
            continue;
        }
        replay_column(w, obj[i], r, col[i], u, c);
        uint64_t m = 0;
        double a;
        memcpy(&a, &bits[i], 8);
        for (int row = 0; row < rows; row++) {
            if (!((u >> row) & 1)) continue;
            bool hit = c[row] == bits[i];
            if (w->rec_ctype[r][col[i]] == NFK_REC_F64) {
                double v;
                memcpy(&v, &c[row], 8);
                hit = v == a;
            }
            m |= (uint64_t)hit << row;
        }
        masks[i] = m;
    }
    return NFK_OK;
}

int nfk_find_rows(void* world, int32_t n, const int64_t* gh, const int64_t* gd, const int32_t* rec, const int32_t* col,
                  const uint64_t* bits, uint64_t* masks) {
    World* w = (World*)world;
    if (!w || n < 0 || (n && (!gh || !gd || !rec || !col || !bits || !masks))) return fail(NFK_ERR_ARG, "null argument");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    std::vector<int32_t> obj(n);
    if (int rl = find_many_par(w, n, gh, gd, obj.data())) return rl;
    return find_rows(w, n, obj.data(), gh, gd, rec, col, bits, masks);
}

int nfk_find_rows_obj(void* world, int32_t n, const int32_t* obj, const int32_t* rec, const int32_t* col,
                      const uint64_t* bits, uint64_t* masks) {
    World* w = (World*)world;
    if (!w || n < 0 || (n && (!obj || !rec || !col || !bits || !masks))) return fail(NFK_ERR_ARG, "null argument");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    return find_rows(w, n, live_objects(w, n, obj), nullptr, nullptr, rec, col, bits, masks);
}

int nfk_find_objects(void* world, int32_t n, const int64_t* gh, const int64_t* gd, const int32_t* rec, const int32_t* col,
                     const int64_t* vh, const int64_t* vd, uint64_t* masks) {
    World* w = (World*)world;
    if (!w || n < 0 || (n && (!gh || !gd || !rec || !col || !vh || !vd || !masks))) return fail(NFK_ERR_ARG, "null argument");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    std::vector<int32_t> obj(n);
    if (int rl = find_many_par(w, n, gh, gd, obj.data())) return rl;
    return find_rows(w, n, obj.data(), gh, gd, rec, col, (const uint64_t*)vd, masks, (const uint64_t*)vh);
}

int nfk_find_objects_obj(void* world, int32_t n, const int32_t* obj, const int32_t* rec, const int32_t* col,
                         const int64_t* vh, const int64_t* vd, uint64_t* masks) {
    World* w = (World*)world;
    if (!w || n < 0 || (n && (!obj || !rec || !col || !vh || !vd || !masks))) return fail(NFK_ERR_ARG, "null argument");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    return find_rows(w, n, live_objects(w, n, obj), nullptr, nullptr, rec, col, (const uint64_t*)vd, masks,
                     (const uint64_t*)vh);
}

int nfk_find_stats(void* world, double* kernel_ms, int64_t* bytes, int32_t* n_host) {
    World* w = (World*)world;
    if (!w) return fail(NFK_ERR_ARG, "null world");
    if (kernel_ms) *kernel_ms = w->f_kernel_ms;
    if (bytes) *bytes = w->f_bytes;
    if (n_host) *n_host = w->f_host;
    return NFK_OK;
}

int nfk_add_schedules(void* world, int32_t n, const int64_t* gh, const int64_t* gd, const int32_t* kind,
                      const float* interval, const int32_t* count, const int64_t* now_ms) {
    World* w = (World*)world;
    if (!w || n < 0 || (n && (!gh || !gd || !kind || !interval || !count || !now_ms)))
        return fail(NFK_ERR_ARG, "null argument");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    std::vector<int32_t> obj(n);
    for (int32_t i = 0; i < n; i++) {
        int r = lookup(w, gh[i], gd[i], &obj[i]);
        if (r) return r;
        if (kind[i] < 0 || kind[i] >= w->cfg.n_kind || !w->kind_defined[kind[i]])
            return fail(NFK_ERR_ARG, "undefined heartbeat kind");
    }
    for (int32_t i = 0; i < n; i++)
        w->hops.push_back({1, (uint32_t)obj[i], (uint32_t)kind[i], interval[i], count[i], now_ms[i]});
    return NFK_OK;
}

int nfk_remove_schedule(void* world, int64_t gh, int64_t gd, int32_t kind) {
    World* w = (World*)world;
    if (!w) return fail(NFK_ERR_ARG, "null world");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    int32_t obj;
    int r = lookup(w, gh, gd, &obj);
    if (r) return r;
    if (kind < -1 || kind >= w->cfg.n_kind) return fail(NFK_ERR_ARG, "bad kind");
    w->hops.push_back({2, (uint32_t)obj, kind < 0 ? kNoKind : (uint32_t)kind, 0.f, 0, 0});
    return NFK_OK;
}

int nfk_remove_all_schedules(void* world, int64_t gh, int64_t gd) {
    World* w = (World*)world;
    if (!w) return fail(NFK_ERR_ARG, "null world");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    int32_t obj;
    int r = lookup(w, gh, gd, &obj);
    if (r) return r;
    w->hops.push_back({3, (uint32_t)obj, 0u, 0.f, 0, 0});
    return NFK_OK;
}

// The schedule words' epoch and the kinds' common steps (nfgpu_device.hpp), taken from the queued
// AddSchedule calls of the first window that has any for the kind: the epoch from the world's first
// call, a kind's step the most frequent one among the window's calls for that kind (a majority
// vote; the calls of a commit come in no particular order, and a rare odd interval among them
// should not make every other record of the kind wide).  They are fixed here, before the frame
// whose k_post_hostops writes the first record that uses them, and never change afterwards.  A
// step that does not fit the hot record's 28 bits leaves its kind without one (its records are wide).
static void fix_schedule_steps(World* w) {
    Dev& d = w->d;
    int64_t cand[NFK_MAX_KINDS] = {};
    int64_t votes[NFK_MAX_KINDS] = {};
    uint32_t seen = 0;
    for (const auto& h : w->hops) {
        if (h.code != 1 || !((w->s_unfixed >> h.kind) & 1u)) continue;
        if (!w->s_epoch_set) {
            d.s_epoch = (int64_t)((uint64_t)h.time - (uint64_t)kScEpochBack);
            w->s_epoch_set = true;
        }
        const int64_t step = (int64_t)(h.interval * 1000.0f);
        seen |= 1u << h.kind;
        if (votes[h.kind] == 0) cand[h.kind] = step;
        votes[h.kind] += cand[h.kind] == step ? 1 : -1;
    }
    for (int k = 0; k < NFK_MAX_KINDS; k++) {
        if (!((seen >> k) & 1u)) continue;
        w->s_unfixed &= ~(1u << k);
        if (st_pack_step(cand[k])) {
            d.s_step[k] = (int32_t)cand[k];
            d.s_kvalid |= 1u << k;
        }
    }
}

// a batch of schedule calls, their objects resolved (see queue_sets)
static int queue_schedule_calls(World* w, int32_t n, const int32_t* op, const int32_t* obj, const int32_t* kind,
                                const float* interval, const int32_t* count, const int64_t* now_ms, const int64_t* gh,
                                const int64_t* gd) {
    // appended and checked in one pass without a branch per check (the ops of a batch come in no
    // predictable order); a batch with a bad call is taken back out and walked again for the first
    // one's error
    const int32_t nk = w->cfg.n_kind;
    const size_t base = w->hops.size();
    if (w->hops.capacity() < base + (size_t)n)  // (geometric: single calls append one by one)
        w->hops.reserve(std::max(base + (size_t)n, 2 * w->hops.capacity()));
    uint32_t bad = 0;
    for (int32_t i = 0; i < n; i++) {
        const int32_t o = op[i], k = kind[i];
        const bool add = o == 1;
        const bool kin = (uint32_t)k < (uint32_t)nk;
        const bool def = w->kind_defined[kin ? k : 0] && kin;
        bad |= (uint32_t)(obj[i] < 0) | (uint32_t)((uint32_t)(o - 1) > 2u) | (uint32_t)(add && !def) |
               (uint32_t)(o == 2 && (k < -1 || k >= nk));
        w->hops.push_back({o, (uint32_t)obj[i], o == 3 ? 0u : (k < 0 ? kNoKind : (uint32_t)k), add ? interval[i] : 0.f,
                           add ? count[i] : 0, add ? now_ms[i] : 0});
    }
    if (bad) {
        w->hops.resize(base);
        for (int32_t i = 0; i < n; i++) {
            if (obj[i] < 0)
                return fail(NFK_ERR_NOTFOUND, gh ? "no object " + std::to_string(gh[i]) + "-" + std::to_string(gd[i])
                                                 : "no object index " + std::to_string(obj[i]));
            if (op[i] < 1 || op[i] > 3) return fail(NFK_ERR_ARG, "schedule call op must be 1, 2 or 3");
            if (op[i] == 1 && (kind[i] < 0 || kind[i] >= w->cfg.n_kind || !w->kind_defined[kind[i]]))
                return fail(NFK_ERR_ARG, "undefined heartbeat kind");
            if (op[i] == 2 && (kind[i] < -1 || kind[i] >= w->cfg.n_kind)) return fail(NFK_ERR_ARG, "bad kind");
        }
        return fail(NFK_ERR_ARG, "bad schedule call");
    }
    return NFK_OK;
}

int nfk_schedule_calls(void* world, int32_t n, const int32_t* op, const int64_t* gh, const int64_t* gd,
                       const int32_t* kind, const float* interval, const int32_t* count, const int64_t* now_ms) {
    World* w = (World*)world;
    if (!w || n < 0 || (n && (!op || !gh || !gd || !kind || !interval || !count || !now_ms)))
        return fail(NFK_ERR_ARG, "null argument");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    w->look.resize(n);
    const auto t0 = std::chrono::steady_clock::now();
    if (int rl = find_many_par(w, n, gh, gd, w->look.data())) return rl;
    const auto t1 = std::chrono::steady_clock::now();
    const int r = queue_schedule_calls(w, n, op, w->look.data(), kind, interval, count, now_ms, gh, gd);
    if (trace_calls())
        fprintf(stderr, "schedule_calls n=%d: lookups %.3f ms, queue %.3f ms\n", n, ms_since(t0, t1),
                ms_since(t1, std::chrono::steady_clock::now()));
    return r;
}

int nfk_schedule_calls_obj(void* world, int32_t n, const int32_t* op, const int32_t* obj, const int32_t* kind,
                           const float* interval, const int32_t* count, const int64_t* now_ms) {
    World* w = (World*)world;
    if (!w || n < 0 || (n && (!op || !obj || !kind || !interval || !count || !now_ms)))
        return fail(NFK_ERR_ARG, "null argument");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    return queue_schedule_calls(w, n, op, live_objects(w, n, obj), kind, interval, count, now_ms, nullptr, nullptr);
}

// The world's values of property words after the last frame (waits for the world's stream): src
// entries are pmem word offsets, or (1 << 63 | word index in ins_rows) for an object that entered
// in this window; at most 8 single-element reads, else one gather kernel
static int read_words(World* w, const std::vector<uint64_t>& src, uint64_t* got) {
    if (src.empty()) return NFK_OK;
    HIPCHK(hipStreamSynchronize(w->stream));
    if (src.size() <= 8) {
        for (size_t q = 0; q < src.size(); q++) {
            const uint64_t* a = (src[q] >> 63) ? w->ins_rows + (src[q] & ~(1ull << 63)) : w->d.pmem + src[q];
            HIPCHK(hipMemcpy(&got[q], a, 8, hipMemcpyDeviceToHost));
        }
        return NFK_OK;
    }
    int r = dev_reserve(w, (void**)&w->gat, &w->gat_cap, src.size() * 16);
    if (r) return r;
    HIPCHK(hipMemcpy(w->gat, src.data(), src.size() * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_gather_words, dim3((unsigned)((src.size() + kTPB - 1) / kTPB)), dim3(kTPB), 0, w->stream,
                       (const uint64_t*)w->gat, (int32_t)src.size(), (const uint64_t*)w->d.pmem,
                       (const uint64_t*)w->ins_rows, w->gat + src.size());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(got, w->gat + src.size(), src.size() * 8, hipMemcpyDeviceToHost, w->stream));
    HIPCHK(hipStreamSynchronize(w->stream));
    return NFK_OK;
}

// where property word `half` (0 data, 1 head) of pid of object o is read from (see read_words)
static int word_src(World* w, int32_t o, int32_t pid, int half, uint64_t* src) {
    const int32_t sl = w->slot_of_obj[o];
    if (w->src_row[o] >= 0)  // entered in this window: its row of the import buffer
        *src = (1ull << 63) | ((uint64_t)w->src_row[o] * w->row_words + (uint64_t)(prop_word(w, pid) + half));
    else if (sl >= 0)
        *src = (uint64_t)(w->tab.p_off[pid] + (int64_t)sl * w->tab.p_str[pid] + half);
    else
        return fail(NFK_ERR_STATE, "object without a slot");
    return NFK_OK;
}

// index the queued Set calls by (object, property) (ov_last / ov_prev chains, call order)
static int index_queued_sets(World* w) {
    if (int r = pull_device_queue(w)) return r;
    for (size_t i = w->ov_prev.size(); i < w->xops.size(); i++) {
        const uint64_t key = ((uint64_t)w->xops[i].slot << 7) | w->xops[i].pid;
        auto it = w->ov_last.find(key);
        w->ov_prev.push_back(it == w->ov_last.end() ? 0xFFFFFFFFu : it->second);
        w->ov_last[key] = (uint32_t)i;
    }
    return NFK_OK;
}

// NFCProperty::GetObject of n (object, object property) pairs as the reference holds them now: the
// device's value after the last frame, then this window's queued SetObject calls (the last one
// stays).  Shared by nfk_get_objects and the host side of nfk_query_objects.
static int current_objects(World* w, int32_t n, const int32_t* obj, const int32_t* pid, int64_t* vh, int64_t* vd) {
    std::vector<uint64_t> src(2 * (size_t)n), got(2 * (size_t)n);
    for (int32_t i = 0; i < n; i++)
        for (int h = 0; h < 2; h++) {
            int r = word_src(w, obj[i], pid[i], h, &src[2 * (size_t)i + h]);
            if (r) return r;
        }
    int r = read_words(w, src, got.data());
    if (r) return r;
    // this window's queued SetObject calls on top: NFCProperty::SetObject keeps the last value
    if (int r = index_queued_sets(w)) return r;
    for (int32_t i = 0; i < n; i++) {
        vd[i] = (int64_t)got[2 * (size_t)i];
        vh[i] = (int64_t)got[2 * (size_t)i + 1];
        auto it = w->ov_last.find(((uint64_t)obj[i] << 7) | (uint32_t)pid[i]);
        if (it == w->ov_last.end()) continue;
        vd[i] = (int64_t)w->xops[it->second].bits;
        vh[i] = (int64_t)w->xops_h[it->second];
    }
    return NFK_OK;
}

int nfk_get_objects(void* world, int32_t n, const int64_t* gh, const int64_t* gd, const int32_t* pid, int64_t* vh,
                    int64_t* vd) {
    World* w = (World*)world;
    if (!w || n < 0 || (n && (!gh || !gd || !pid || !vh || !vd))) return fail(NFK_ERR_ARG, "null argument");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    std::vector<int32_t> obj(n);
    if (int rl = find_many_par(w, n, gh, gd, obj.data())) return rl;
    for (int32_t i = 0; i < n; i++) {
        if (obj[i] < 0) return fail(NFK_ERR_NOTFOUND, "There is no object " + std::to_string(gh[i]) + "-" + std::to_string(gd[i]));
        if (pid[i] < w->n_if || pid[i] >= w->n_prop) return fail(NFK_ERR_ARG, "not an object property");
    }
    return current_objects(w, n, obj.data(), pid, vh, vd);
}

// NFCProperty::GetInt / GetFloat of n (object, int / f64 property) pairs as the reference holds them
// now (raw bits).  Shared by nfk_get_props and the host side of nfk_query_objects.
static int current_props(World* w, int32_t n, const int32_t* obj, const int32_t* pid, uint64_t* bits) {
    // 1. the world's values after the last frame (a per-window cache of device reads)
    std::vector<uint64_t> src;
    std::vector<int32_t> miss;
    for (int32_t i = 0; i < n; i++) {
        const uint64_t key = ((uint64_t)obj[i] << 7) | (uint32_t)pid[i];
        auto it = w->dcache.find(key);
        if (it != w->dcache.end()) {
            bits[i] = it->second;
            continue;
        }
        uint64_t a;
        int r = word_src(w, obj[i], pid[i], 0, &a);
        if (r) return r;
        src.push_back(a);
        miss.push_back(i);
    }
    if (!miss.empty()) {
        std::vector<uint64_t> got(miss.size());
        int r = read_words(w, src, got.data());
        if (r) return r;
        for (size_t q = 0; q < miss.size(); q++) {
            const int32_t i = miss[q];
            bits[i] = got[q];
            w->dcache[((uint64_t)obj[i] << 7) | (uint32_t)pid[i]] = got[q];
        }
    }
    // 2. this window's queued writes of the property on top, in call order (PR:254 / PR:295)
    if (int r = index_queued_sets(w)) return r;
    std::vector<uint32_t> chain;
    for (int32_t i = 0; i < n; i++) {
        auto it = w->ov_last.find(((uint64_t)obj[i] << 7) | (uint32_t)pid[i]);
        if (it == w->ov_last.end()) continue;
        chain.clear();
        for (uint32_t x = it->second; x != 0xFFFFFFFFu; x = w->ov_prev[x]) chain.push_back(x);
        uint64_t v = bits[i];
        for (size_t c = chain.size(); c-- > 0;) {
            const uint64_t b = w->xops[chain[c]].bits;
            if (pid[i] < w->cfg.n_int) {
                v = b;
            } else {
                double bd, vd;
                memcpy(&bd, &b, 8);
                memcpy(&vd, &v, 8);
                if (!(fabs(bd - vd) <= 1e-15)) v = b;
            }
        }
        bits[i] = v;
    }
    // 3. a linked property (nfk_link_record) whose (object, record) has queued calls: the list
    //    replayed on the device's used mask and the one column; the sum at the last event that names
    //    the column stays (none: the stored value)
    if (w->lk_pids[0] | w->lk_pids[1]) {
        // (the device's used mask and the column are read once per window and (object, property): ucache / lcache)
        struct LEnt { int32_t i, r, c; const uint64_t* cells; uint64_t um; bool have_um, have_col; };
        std::vector<LEnt> ent;
        std::vector<uint64_t> addr;
        for (int32_t i = 0; i < n; i++) {
            if (!w->linked_pid(pid[i])) continue;
            const int r = w->lk_of_pid[pid[i]] >> 4, c = w->lk_of_pid[pid[i]] & 15;
            if (w->rq_index.find(((uint64_t)obj[i] << 3) | (uint32_t)r) == w->rq_index.end()) continue;
            LEnt e{i, r, c, nullptr, 0, false, w->lcache.count(((uint64_t)obj[i] << 7) | (uint32_t)pid[i]) != 0};
            auto it = w->ucache.find(((uint64_t)obj[i] << 3) | (uint32_t)r);
            if (it != w->ucache.end()) {
                e.um = it->second;
                e.have_um = true;
            }
            const uint64_t* used;
            if (int er = rec_addrs(w, obj[i], r, &e.cells, &used)) return er;
            if (!e.have_um) addr.push_back((uint64_t)(uintptr_t)used);
            ent.push_back(e);
        }
        if (!ent.empty()) {
            std::vector<uint64_t> um(addr.size());
            if (int e = read_abs(w, addr, um.data())) return e;
            addr.clear();
            size_t q = 0;
            for (LEnt& e : ent) {
                if (!e.have_um) {
                    e.um = um[q++];
                    w->ucache[((uint64_t)obj[e.i] << 3) | (uint32_t)e.r] = e.um;
                }
                const int rows = w->tab.rec_rows[e.r];
                e.um &= rec_rowm(rows);
                if (e.have_col) continue;
                for (int p = 0, nu = __builtin_popcountll(e.um); p < nu; p++)  // (the used rows first: rec_pos)
                    addr.push_back((uint64_t)(uintptr_t)(e.cells + (size_t)e.c * rows + p));
            }
            std::vector<uint64_t> cv(addr.size());
            if (int e = read_abs(w, addr, cv.data())) return e;
            size_t a = 0;
            for (const LEnt& e : ent) {
                const int rows = w->tab.rec_rows[e.r];
                std::vector<uint64_t>& col = w->lcache[((uint64_t)obj[e.i] << 7) | (uint32_t)pid[e.i]];
                if (col.empty()) {  // (two queries of one pair in this batch: the first fills it)
                    col.assign(64, 0);
                    if (!e.have_col)
                        for (int row = 0; row < rows; row++)
                            if ((e.um >> row) & 1) col[row] = cv[a++];
                } else if (!e.have_col) {
                    a += (size_t)__builtin_popcountll(e.um);
                }
                uint64_t c[64];
                memcpy(c, col.data(), sizeof c);
                uint32_t sum;
                if (replay_link(w, obj[e.i], e.r, e.c, e.um, c, &sum)) bits[e.i] = (uint64_t)(int64_t)(int32_t)sum;
            }
        }
    }
    return NFK_OK;
}

int nfk_get_props(void* world, int32_t n, const int64_t* gh, const int64_t* gd, const int32_t* pid, uint64_t* bits) {
    World* w = (World*)world;
    if (!w || n < 0 || (n && (!gh || !gd || !pid || !bits))) return fail(NFK_ERR_ARG, "null argument");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    std::vector<int32_t> obj(n);
    if (int rl = find_many_par(w, n, gh, gd, obj.data())) return rl;
    for (int32_t i = 0; i < n; i++) {
        if (obj[i] < 0) return fail(NFK_ERR_NOTFOUND, "There is no object " + std::to_string(gh[i]) + "-" + std::to_string(gd[i]));
        if (pid[i] < 0 || pid[i] >= w->n_if) return fail(NFK_ERR_ARG, "bad property id (object properties: nfk_get_objects)");
    }
    return current_props(w, n, obj.data(), pid, bits);
}

// ---- resource calls (nfk_adjust_props): NFCPropertyModule's Add* / Consume* / Enough* / Full* (PM:215-472) ----
// the calls of resolved objects (obj[i] < 0: unknown; gh / gd for the message, or null)
static int adjust_props(World* w, int32_t n, const int32_t* obj, const int64_t* gh, const int64_t* gd, const uint8_t* op,
                        const int32_t* dst, const int32_t* bound, const int64_t* value, uint8_t* ret) {
    w->a_stats = nfk_adjust_stats_t{};
    // the whole batch is checked before anything is read or queued
    for (int32_t i = 0; i < n; i++) {
        if (obj[i] < 0)
            return fail(NFK_ERR_NOTFOUND, gh ? "There is no object " + std::to_string(gh[i]) + "-" + std::to_string(gd[i])
                                             : "no object index");
        if (op[i] > NFK_ADJ_FILL) return fail(NFK_ERR_ARG, "unknown resource call op " + std::to_string(op[i]));
        if (dst[i] < 0 || dst[i] >= w->n_if)
            return fail(NFK_ERR_ARG, dst[i] >= w->n_if && dst[i] < w->n_prop ? "object property: use nfk_set_objects"
                                                                              : "bad property id");
        if (dst[i] >= w->cfg.n_int) return fail(NFK_ERR_ARG, "a resource call's dst is an int property");
        if (w->linked_pid(dst[i]))
            return fail(NFK_ERR_ARG, "property " + std::to_string(dst[i]) + " is linked to a record column (nfk_link_record): "
                                     "its value is its link's");
        const bool takes = op[i] == NFK_ADJ_GAIN_ALIVE || op[i] == NFK_ADJ_GAIN_CAP || op[i] == NFK_ADJ_FILL;
        if (takes ? (bound[i] < 0 || bound[i] >= w->cfg.n_int) : bound[i] != -1)
            return fail(NFK_ERR_ARG, takes ? "this resource call's bound is an int property" : "this resource call takes no bound (-1)");
        if (w->src_row[obj[i]] < 0 && w->slot_of_obj[obj[i]] < 0) return fail(NFK_ERR_STATE, "object without a slot");
    }
    if (n == 0) return NFK_OK;

    // the calls grouped stably by (object, dst): ord[] lists them group by group in call order,
    // gkey[] the groups' keys ascending, gat[] where each group starts in ord[].  (A batch whose
    // keys ascend strictly, distinct objects in index order, is its own grouping.)
    // (keys as ov_last's / dcache's: object << 7 | pid; the int and f64 properties are at most 128)
    static_assert(NFK_MAX_PROPS <= 128, "(object << 7 | pid) keys and the two-word dst_pids hold 128 property ids");
    auto key_of = [&](int32_t i, int32_t pid) { return ((uint64_t)(uint32_t)obj[i] << 7) | (uint32_t)pid; };
    bool ascending = true;
    uint64_t dst_pids[2] = {0, 0};
    for (int32_t i = 0; i < n; i++) {
        dst_pids[dst[i] >> 6] |= 1ull << (dst[i] & 63);
        if (i && key_of(i, dst[i]) <= key_of(i - 1, dst[i - 1])) ascending = false;
    }
    std::vector<uint32_t> ord(n);
    if (ascending) {
        for (int32_t i = 0; i < n; i++) ord[i] = (uint32_t)i;
    } else {
        const int ib = bits_for((uint64_t)n - 1), kb = bits_for((uint64_t)w->n_obj) + 7;
        if (ib + kb <= 64) {
            std::vector<uint64_t> a(n), t;
            for (int32_t i = 0; i < n; i++) a[i] = (key_of(i, dst[i]) << ib) | (uint32_t)i;
            radix_sort_packed(a, t, ib, kb);
            for (int32_t i = 0; i < n; i++) ord[i] = (uint32_t)(a[i] & ((1ull << ib) - 1));
        } else {
            for (int32_t i = 0; i < n; i++) ord[i] = (uint32_t)i;
            std::stable_sort(ord.begin(), ord.end(),
                             [&](uint32_t x, uint32_t y) { return key_of((int32_t)x, dst[x]) < key_of((int32_t)y, dst[y]); });
        }
    }
    std::vector<uint64_t> gkey;
    std::vector<uint32_t> gat;
    for (int32_t k = 0; k < n; k++) {
        const uint64_t key = key_of((int32_t)ord[k], dst[ord[k]]);
        if (gkey.empty() || gkey.back() != key) {
            gkey.push_back(key);
            gat.push_back((uint32_t)k);
        }
    }
    gat.push_back((uint32_t)n);
    const size_t ng = gkey.size();

    // the groups answered on the host: a call with pending state in this window on its (object,
    // dst), its (object, bound) or its object, and a call whose bound is a dst of this batch — with
    // that dst's group, so that the device's groups depend on no host call and the reverse
    if (int r = index_queued_sets(w)) return r;
    const bool queued = !w->ov_last.empty(), recq = !w->rq_index.empty() && (w->lk_pids[0] | w->lk_pids[1]);
    std::vector<uint8_t> ghost(ng, 0);
    auto group_of = [&](uint64_t key) -> int64_t {
        auto it = std::lower_bound(gkey.begin(), gkey.end(), key);
        return it != gkey.end() && *it == key ? (int64_t)(it - gkey.begin()) : -1;
    };
    int32_t n_host = 0;
    for (size_t g = 0; g < ng; g++)
        for (uint32_t k = gat[g]; k < gat[g + 1]; k++) {
            const int32_t i = (int32_t)ord[k], o = obj[i], b = bound[i];
            bool pend = w->src_row[o] >= 0 || (queued && w->ov_last.count(gkey[g]));
            if (b >= 0) {
                const uint64_t bk = key_of(i, b);
                pend = pend || (queued && w->ov_last.count(bk));
                if (recq && w->linked_pid(b))
                    pend = pend || w->rq_index.count(((uint64_t)o << 3) | (uint32_t)(w->lk_of_pid[b] >> 4));
                if ((dst_pids[b >> 6] >> (b & 63)) & 1) {
                    const int64_t bg = group_of(bk);
                    if (bg >= 0) {
                        ghost[bg] = 1;
                        pend = true;
                    }
                }
            }
            if (pend) ghost[g] = 1;
        }
    for (size_t g = 0; g < ng; g++)
        if (ghost[g]) n_host += (int32_t)(gat[g + 1] - gat[g]);
    const int32_t nd = n - n_host;

    // the device's calls: descriptors in pinned memory, the new values and result bytes behind them
    const size_t o_v = align16((size_t)nd * sizeof(AdjDev)), o_r = o_v + (size_t)n * 8, tot = align16(o_r + (size_t)n);
    std::vector<int64_t> newv_h;  // (the host's calls' new values, by place)
    const int64_t* newv = nullptr;
    if (nd) {
        if (int r = dev_reserve(w, &w->a_dev, &w->a_dcap, tot)) return r;
        if (tot > w->a_pcap) {
            if (w->a_pin) HIPCHK(hipHostFree(w->a_pin));
            w->a_pin = nullptr;
            const size_t c = std::max(tot, w->a_pcap + w->a_pcap / 2);
            w->a_pcap = 0;  // (until the new buffer exists)
            HIPCHK(hipHostMalloc((void**)&w->a_pin, c, hipHostMallocDefault));
            w->a_pcap = c;
        }
        AdjDev* hq = (AdjDev*)w->a_pin;
        int32_t q = 0;
        for (size_t g = 0; g < ng; g++) {
            if (ghost[g]) continue;
            for (uint32_t k = gat[g]; k < gat[g + 1]; k++) {
                const int32_t i = (int32_t)ord[k], o = obj[i];
                const int64_t sl = w->slot_of_obj[o];  // (not entered in this window: it has a slot)
                AdjDev f;
                f.dst = (uint64_t)(uintptr_t)(w->d.pmem + w->tab.p_off[dst[i]] + sl * w->tab.p_str[dst[i]]);
                f.bound = bound[i] < 0 ? 0 : (uint64_t)(uintptr_t)(w->d.pmem + w->tab.p_off[bound[i]] + sl * w->tab.p_str[bound[i]]);
                f.v = value[i];
                f.place = (uint32_t)i;
                f.len = k == gat[g] ? gat[g + 1] - gat[g] : 0;
                f.op = op[i];
                f.pad = 0;
                hq[q++] = f;
            }
        }
        char* D = (char*)w->a_dev;
        const bool timed = w->profiling;
        if (timed)
            for (auto& e : w->a_ev)
                if (!e) HIPCHK(hipEventCreate(&e));
        HIPCHK(hipMemcpyAsync(D, w->a_pin, (size_t)nd * sizeof(AdjDev), hipMemcpyHostToDevice, w->stream));
        // (a place no lane stores to keeps 0xFF: a descriptor k_adjust refused is an error, not a stale result)
        HIPCHK(hipMemsetAsync(D + o_r, 0xFF, (size_t)n, w->stream));
        if (timed) HIPCHK(hipEventRecord(w->a_ev[0], w->stream));
        hipLaunchKernelGGL(k_adjust, dim3((unsigned)((nd + kTPB - 1) / kTPB)), dim3(kTPB), 0, w->stream, (const AdjDev*)D, nd,
                           n, (int64_t*)(D + o_v), (uint8_t*)(D + o_r));
        HIPCHK(hipGetLastError());
        if (timed) HIPCHK(hipEventRecord(w->a_ev[1], w->stream));
        HIPCHK(hipMemcpyAsync(w->a_pin + o_v, D + o_v, tot - o_v, hipMemcpyDeviceToHost, w->stream));
        HIPCHK(hipStreamSynchronize(w->stream));
        w->a_stats.bytes = (int64_t)(tot - o_v);
        if (timed) {
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, w->a_ev[0], w->a_ev[1]));
            w->a_stats.kernel_ms = ms;
        }
        newv = (const int64_t*)(w->a_pin + o_v);
        const uint8_t* hr = (const uint8_t*)(w->a_pin + o_r);
        uint8_t unset = 0;
        for (size_t g = 0; g < ng; g++)
            if (!ghost[g])
                for (uint32_t k = gat[g]; k < gat[g + 1]; k++) {
                    ret[ord[k]] = hr[ord[k]];
                    unset |= hr[ord[k]] & 0xFC;
                }
        if (unset) return fail(NFK_ERR_DEVICE, "k_adjust left a call unanswered (nothing of the batch queued)");
    }

    // the host's calls, in batch order over the values nfk_get_props answers (read once per cell)
    if (n_host) {
        std::vector<uint8_t> chost(n, 0);
        for (size_t g = 0; g < ng; g++)
            if (ghost[g])
                for (uint32_t k = gat[g]; k < gat[g + 1]; k++) chost[ord[k]] = 1;
        std::unordered_map<uint64_t, int64_t> cell;
        std::vector<int32_t> ro, rp;
        for (int32_t i = 0; i < n; i++) {
            if (!chost[i]) continue;
            for (int32_t p : {dst[i], bound[i]})
                if (p >= 0 && cell.emplace(key_of(i, p), 0).second) {
                    ro.push_back(obj[i]);
                    rp.push_back(p);
                }
        }
        std::vector<uint64_t> got(ro.size());
        if (int r = current_props(w, (int32_t)ro.size(), ro.data(), rp.data(), got.data())) return r;
        for (size_t q = 0; q < ro.size(); q++) cell[((uint64_t)(uint32_t)ro[q] << 7) | (uint32_t)rp[q]] = (int64_t)got[q];
        newv_h.assign(n, 0);
        if (newv) memcpy(newv_h.data(), newv, (size_t)n * 8);
        for (int32_t i = 0; i < n; i++) {
            if (!chost[i]) continue;
            int64_t& cur = cell[key_of(i, dst[i])];
            const int64_t mx = bound[i] < 0 ? 0 : cell[key_of(i, bound[i])];
            int64_t nv = cur;
            const uint32_t r = adj_rule(op[i], cur, mx, value[i], &nv);
            if (r & NFK_ADJ_SET) cur = nv;
            newv_h[i] = nv;
            ret[i] = (uint8_t)r;
        }
        newv = newv_h.data();
    }

    // the accepted Sets join the window's SetProperty stream in batch order
    std::vector<int32_t> so, sp;
    std::vector<uint64_t> sb;
    for (int32_t i = 0; i < n; i++)
        if (ret[i] & NFK_ADJ_SET) {
            so.push_back(obj[i]);
            sp.push_back(dst[i]);
            sb.push_back((uint64_t)newv[i]);
        }
    w->a_stats.n_dev = nd;
    w->a_stats.n_host = n_host;
    w->a_stats.n_set = (int32_t)so.size();
    return queue_sets(w, (int32_t)so.size(), so.data(), sp.data(), sb.data(), nullptr, nullptr);
}

int nfk_adjust_props(void* world, int32_t n, const int64_t* gh, const int64_t* gd, const uint8_t* op, const int32_t* dst,
                     const int32_t* bound, const int64_t* value, uint8_t* ret) {
    World* w = (World*)world;
    if (!w || n < 0 || (n && (!gh || !gd || !op || !dst || !bound || !value || !ret))) return fail(NFK_ERR_ARG, "null argument");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    w->look.resize(n);  // one GUID lookup per call
    if (int rl = find_many_par(w, n, gh, gd, w->look.data())) return rl;
    return adjust_props(w, n, w->look.data(), gh, gd, op, dst, bound, value, ret);
}

int nfk_adjust_props_obj(void* world, int32_t n, const int32_t* obj, const uint8_t* op, const int32_t* dst,
                         const int32_t* bound, const int64_t* value, uint8_t* ret) {
    World* w = (World*)world;
    if (!w || n < 0 || (n && (!obj || !op || !dst || !bound || !value || !ret))) return fail(NFK_ERR_ARG, "null argument");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    return adjust_props(w, n, live_objects(w, n, obj), nullptr, nullptr, op, dst, bound, value, ret);
}

int nfk_adjust_stats(void* world, nfk_adjust_stats_t* out) {
    World* w = (World*)world;
    if (!w || !out) return fail(NFK_ERR_ARG, "null argument");
    *out = w->a_stats;
    return NFK_OK;
}

// ---- enter snapshots (nfk_snapshot_objects): OnPropertyEnter / OnRecordEnter payloads ----
int nfk_set_snapshot_order(void* world, const int32_t* prop_order, const int32_t* rec_order) {
    World* w = (World*)world;
    if (!w) return fail(NFK_ERR_ARG, "null world");
    auto perm = [](const int32_t* o, int n) {
        uint8_t seen[kMaxProps] = {};
        for (int i = 0; i < n; i++) {
            if (o[i] < 0 || o[i] >= n || seen[o[i]]) return false;
            seen[o[i]] = 1;
        }
        return true;
    };
    // (both lists are checked before either is taken)
    if (prop_order && !perm(prop_order, w->n_prop)) return fail(NFK_ERR_ARG, "prop_order is no permutation of the property ids");
    if (rec_order && !perm(rec_order, w->cfg.n_rec)) return fail(NFK_ERR_ARG, "rec_order is no permutation of the record ids");
    w->s_porder.clear();
    w->s_rorder.clear();
    if (prop_order) w->s_porder.assign(prop_order, prop_order + w->n_prop);
    if (rec_order) w->s_rorder.assign(rec_order, rec_order + w->cfg.n_rec);
    w->s_tab_dirty = true;
    return NFK_OK;
}

// the walk table from the flags and the order, on the host and (uploaded) on the device
static int snap_table(World* w) {
    if (!w->s_tab_dirty && w->s_tab_d) return NFK_OK;
    SnapTab& t = w->s_tab;
    t = SnapTab{};
    t.n_int = w->cfg.n_int;
    t.n_if = w->n_if;
    memset(w->s_cells_ub, 0, sizeof(w->s_cells_ub));
    for (int pos = 0; pos < w->n_prop; pos++) {
        const int pid = w->s_porder.empty() ? pos : w->s_porder[pos];
        t.p_pid[pos] = pid;
        t.p_off[pos] = w->tab.p_off[pid];
        for (int c = 0; c < w->cfg.n_class; c++)
            for (int v = 0; v < 2; v++)
                if (w->tab.pflags[c][pid] & (v ? NFK_PRIVATE : NFK_PUBLIC)) t.pmask[c][v][pos >> 6] |= 1ull << (pos & 63);
    }
    for (int pos = 0; pos < w->cfg.n_rec; pos++) {
        const int r = w->s_rorder.empty() ? pos : w->s_rorder[pos];
        SnapRec sr{w->d.rcells[r], w->d.rused[r], r, w->tab.rec_rows[r], w->tab.rec_cols[r], 0};
        t.rec[pos] = sr;
        t.rec_of[r] = sr;
        for (int c = 0; c < w->cfg.n_class; c++)
            for (int v = 0; v < 2; v++)
                if (w->tab.rflags[c][r] & (v ? NFK_PRIVATE : NFK_PUBLIC)) {
                    t.rmask[c][v] |= 1u << pos;
                    w->s_cells_ub[c][v] += (uint32_t)(sr.rows * sr.cols);
                }
    }
    if (!w->s_tab_d) HIPCHK(hipMalloc((void**)&w->s_tab_d, sizeof(SnapTab)));
    HIPCHK(hipStreamSynchronize(w->stream));  // (control plane: flags or order changed)
    HIPCHK(hipMemcpy(w->s_tab_d, &t, sizeof(SnapTab), hipMemcpyHostToDevice));
    w->s_tab_dirty = false;
    return NFK_OK;
}

// the result region's layout for n requests, P property entries, R record entries, C cells
struct SnapLayout {
    size_t hdr, p_pid, r_rec, r_cell, p_bits, p_head, r_used, cells, end, r_slot, dev_end;
    SnapLayout(size_t n, size_t P, size_t R, size_t C, bool heads) {
        hdr = 0;
        p_pid = align16(16 * n);
        r_rec = p_pid + align16(4 * P);
        r_cell = r_rec + align16(4 * R);
        p_bits = r_cell + align16(4 * R);
        p_head = p_bits + align16(8 * P);
        r_used = p_head + (heads ? align16(8 * P) : 0);
        cells = r_used + align16(8 * R);
        end = cells + align16(8 * C);
        r_slot = end;  // (device only)
        dev_end = r_slot + align16(4 * R);
    }
};

static int snap_pin_reserve(World* w, size_t bytes) {
    if (bytes <= w->s_pcap) return NFK_OK;
    if (w->s_pin) HIPCHK(hipHostFree(w->s_pin));
    w->s_pin = nullptr;
    const size_t c = std::max(bytes, w->s_pcap + w->s_pcap / 2);
    w->s_pcap = 0;  // (until the new buffer exists)
    HIPCHK(hipHostMalloc((void**)&w->s_pin, c, hipHostMallocDefault));
    w->s_pcap = c;
    return NFK_OK;
}

// NFIDataList::IsNullValue of an f64 (NFIDataList.h:160-221), as k_snap tests it
static bool snap_f64_set_host(uint64_t b) {
    double v;
    memcpy(&v, &b, 8);
    return v > 0.001 || v < -0.001;
}

// the three count arrays are scanned end to end with int indices: 3 n fits an int (tested before an
// array of the call is read)
constexpr int32_t kSnapMaxRequests = INT32_MAX / 3;

// the snapshots of resolved objects (obj[i] < 0: unknown; gh / gd for the message, or null)
static int snapshot(World* w, int32_t n, const int32_t* obj, const int64_t* gh, const int64_t* gd, const uint8_t* view,
                    nfk_snapshot* out) {
    *out = nfk_snapshot{};
    for (int32_t i = 0; i < n; i++) {
        if (view[i] != NFK_VIEW_PUBLIC && view[i] != NFK_VIEW_PRIVATE) return fail(NFK_ERR_ARG, "bad view");
        if (obj[i] < 0)
            return fail(NFK_ERR_NOTFOUND, gh ? "There is no object " + std::to_string(gh[i]) + "-" + std::to_string(gd[i])
                                             : "no object index");
    }
    if (n == 0) return NFK_OK;
    if (int r = snap_table(w)) return r;
    const SnapTab& t = w->s_tab;
    const bool heads = w->cfg.n_obj > 0;

    // the window's objects with queued Set / record calls (marks set and cleared in this call);
    // bounds of the totals
    if (int r = index_queued_sets(w)) return r;
    if (w->s_mark.size() < (size_t)w->n_obj) w->s_mark.resize(w->n_obj, 0);
    for (const auto& kv : w->ov_last) w->s_mark[kv.first >> 7] = 1;
    for (const auto& kv : w->rq_index) w->s_mark[kv.first >> 3] = 1;
    std::vector<int32_t> host;
    uint64_t ub_p = 0, ub_r = 0, ub_c = 0;
    for (int32_t i = 0; i < n; i++) {
        const int32_t o = obj[i];
        const int c = w->cls[o], v = view[i] == NFK_VIEW_PRIVATE;
        ub_p += (uint64_t)(__builtin_popcountll(t.pmask[c][v][0]) + __builtin_popcountll(t.pmask[c][v][1]));
        ub_r += (uint64_t)__builtin_popcount(t.rmask[c][v]);
        ub_c += w->s_cells_ub[c][v];
        if (w->s_mark[o] || w->src_row[o] >= 0) host.push_back(i);
    }
    for (const auto& kv : w->ov_last) w->s_mark[kv.first >> 7] = 0;
    for (const auto& kv : w->rq_index) w->s_mark[kv.first >> 3] = 0;
    // the totals are bounded from the views alone (every property in view an entry, every row of
    // every record in view used), before anything is allocated or launched: a batch within the
    // bound cannot wrap the device's 32-bit counts, so the totals themselves need no second test
    if (ub_p > 0xFFFFFFFFull || ub_r > 0xFFFFFFFFull || ub_c > 0xFFFFFFFFull)
        return fail(NFK_ERR_CAPACITY, "snapshot: the bound of the batch's entries or cells does not fit 32 bits");
    for (int32_t i = 0; i < n; i++)
        if (w->src_row[obj[i]] < 0 && w->slot_of_obj[obj[i]] < 0) return fail(NFK_ERR_STATE, "object without a slot");

    // ---- the host's answers (read-your-writes): nfk_get_props / nfk_get_objects / nfk_get_records' code
    std::vector<int32_t> hp_pid, hr_rec;
    std::vector<uint64_t> hp_bits, hp_head, hr_used, hcells;
    std::vector<uint32_t> hr_cell, h_np(host.size(), 0), h_nr(host.size(), 0);
    if (!host.empty()) {
        std::vector<int32_t> ro, rp, oo, op;
        for (int32_t i : host) {
            const int c = w->cls[obj[i]], v = view[i] == NFK_VIEW_PRIVATE;
            for (int pos = 0; pos < w->n_prop; pos++) {
                if (!((t.pmask[c][v][pos >> 6] >> (pos & 63)) & 1)) continue;
                const int pid = t.p_pid[pos];
                (pid < w->n_if ? ro : oo).push_back(obj[i]);
                (pid < w->n_if ? rp : op).push_back(pid);
            }
        }
        std::vector<uint64_t> pb(ro.size());
        std::vector<int64_t> vh(oo.size()), vd(oo.size());
        if (!ro.empty())
            if (int r = current_props(w, (int32_t)ro.size(), ro.data(), rp.data(), pb.data())) return r;
        if (!oo.empty())
            if (int r = current_objects(w, (int32_t)oo.size(), oo.data(), op.data(), vh.data(), vd.data())) return r;
        // the records in view: masks in one gather, the used rows' cells of every column in a second
        struct HEnt { int32_t o, r; const uint64_t* cells; };
        std::vector<HEnt> ent;
        std::vector<uint64_t> addr;
        for (int32_t i : host) {
            const int c = w->cls[obj[i]], v = view[i] == NFK_VIEW_PRIVATE;
            for (uint32_t m = t.rmask[c][v]; m; m &= m - 1) {
                const int r = t.rec[__builtin_ctz(m)].rec;
                const uint64_t *cells, *used;
                if (int e = rec_addrs(w, obj[i], r, &cells, &used)) return e;
                ent.push_back(HEnt{obj[i], r, cells});
                addr.push_back((uint64_t)(uintptr_t)used);
            }
        }
        std::vector<uint64_t> um(ent.size());
        if (int e = read_abs(w, addr, um.data())) return e;
        addr.clear();
        for (size_t j = 0; j < ent.size(); j++) {
            const int rows = w->tab.rec_rows[ent[j].r], cols = w->tab.rec_cols[ent[j].r];
            um[j] &= rec_rowm(rows);
            const int nu = __builtin_popcountll(um[j]);
            for (int c = 0; c < cols; c++)
                for (int p = 0; p < nu; p++) addr.push_back((uint64_t)(uintptr_t)(ent[j].cells + (size_t)c * rows + p));
        }
        std::vector<uint64_t> cv(addr.size());
        if (int e = read_abs(w, addr, cv.data())) return e;
        size_t ai = 0, oi = 0, ej = 0, ca = 0;
        for (size_t h = 0; h < host.size(); h++) {
            const int32_t i = host[h];
            const int c = w->cls[obj[i]], v = view[i] == NFK_VIEW_PRIVATE;
            for (int pos = 0; pos < w->n_prop; pos++) {
                if (!((t.pmask[c][v][pos >> 6] >> (pos & 63)) & 1)) continue;
                const int pid = t.p_pid[pos];
                uint64_t bits, head = 0;
                bool keep;
                if (pid < w->n_if) {
                    bits = pb[ai++];
                    keep = pid < w->cfg.n_int ? bits != 0 : snap_f64_set_host(bits);
                } else {
                    bits = (uint64_t)vd[oi];
                    head = (uint64_t)vh[oi++];
                    keep = (bits | head) != 0;
                }
                if (!keep) continue;
                hp_pid.push_back(pid);
                hp_bits.push_back(bits);
                hp_head.push_back(head);
                h_np[h]++;
            }
            for (uint32_t m = t.rmask[c][v]; m; m &= m - 1, ej++) {
                const int r = ent[ej].r, rows = w->tab.rec_rows[r], cols = w->tab.rec_cols[r];
                const int nu = __builtin_popcountll(um[ej]);
                uint64_t u_now = um[ej];
                hr_rec.push_back(r);
                hr_cell.push_back((uint32_t)hcells.size());
                for (int col = 0; col < cols; col++) {
                    uint64_t u = um[ej], cr[64] = {};
                    for (int row = 0, p = 0; row < rows; row++)
                        if ((u >> row) & 1) cr[row] = cv[ca + (size_t)col * nu + p++];  // (used rows first: rec_pos)
                    replay_column(w, ent[ej].o, r, col, u, cr);
                    u_now = u;
                    for (int row = 0; row < rows; row++)
                        if ((u >> row) & 1) hcells.push_back(cr[row]);
                }
                ca += (size_t)cols * nu;
                hr_used.push_back(u_now);
                h_nr[h]++;
            }
        }
    }
    out->n_host = (int32_t)host.size();

    // ---- the kernels' answers: every request keeps its place in the batch, a host request as slot -1
    const size_t nn = (size_t)n;
    const size_t o_tot = align16(8 * nn), o_res = o_tot + 16;  // pinned: requests, the three totals, the result
    uint32_t Pd = 0, Rd = 0, Cd = 0;
    const bool launch = host.size() < nn;
    const size_t a_req = 0, a_cnt = align16(8 * nn), a_base = a_cnt + align16(12 * nn), a_tot = a_base + align16(12 * nn + 4),
                 a_end = a_tot + 16;
    char* A = nullptr;
    const bool timed = w->profiling && launch;
    if (launch) {
        if (int r = snap_pin_reserve(w, o_res + SnapLayout(nn, 0, 0, 0, heads).end)) return r;
        if (int r = dev_reserve(w, &w->s_dev, &w->s_dcap, a_end)) return r;
        A = (char*)w->s_dev;
        SnapReq* hq = (SnapReq*)w->s_pin;
        for (int32_t i = 0; i < n; i++) hq[i] = SnapReq{w->slot_of_obj[obj[i]], view[i] == NFK_VIEW_PRIVATE ? 1u : 0u};
        for (int32_t i : host) hq[i].slot = -1;
        if (timed)
            for (auto& e : w->s_ev)
                if (!e) HIPCHK(hipEventCreate(&e));
        HIPCHK(hipMemcpyAsync(A + a_req, hq, 8 * nn, hipMemcpyHostToDevice, w->stream));
        if (timed) HIPCHK(hipEventRecord(w->s_ev[0], w->stream));
        hipLaunchKernelGGL(k_snap<false>, dim3((unsigned)((nn + kTPB - 1) / kTPB)), dim3(kTPB), 0, w->stream,
                           (const SnapTab*)w->s_tab_d, (const uint64_t*)w->d.pmem, w->d.fan_desc,
                           (const SnapReq*)(A + a_req), n, (uint32_t*)(A + a_cnt), (const uint32_t*)nullptr,
                           (uint32_t*)nullptr, (int32_t*)nullptr, (uint64_t*)nullptr, (uint64_t*)nullptr,
                           (int32_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr, (int32_t*)nullptr, 0u, 0u);
        hipLaunchKernelGGL(k_snap_scan, dim3(1), dim3(1024), 0, w->stream, (const uint32_t*)(A + a_cnt),
                           (uint32_t*)(A + a_base), (int)(3 * n), n, (uint32_t*)(A + a_tot));
        HIPCHK(hipGetLastError());
        if (timed) HIPCHK(hipEventRecord(w->s_ev[1], w->stream));
        uint32_t* tot = (uint32_t*)(w->s_pin + o_tot);
        HIPCHK(hipMemcpyAsync(tot, A + a_tot, 12, hipMemcpyDeviceToHost, w->stream));
        HIPCHK(hipStreamSynchronize(w->stream));
        Pd = tot[0];
        Rd = tot[1] - tot[0];
        Cd = tot[2] - tot[1];
        // (an invariant, not a state a batch can reach: the counts are sums of what the bounds bound)
        if (Pd > ub_p || Rd > ub_r || Cd > ub_c) return fail(NFK_ERR_DEVICE, "snapshot: more entries than the views hold");
    }
    const uint64_t P = (uint64_t)Pd + hp_pid.size(), R = (uint64_t)Rd + hr_rec.size(), C = (uint64_t)Cd + hcells.size();
    const SnapLayout L(nn, (size_t)P, (size_t)R, (size_t)C, heads);
    if (int r = snap_pin_reserve(w, o_res + L.end)) return r;  // (the requests are on the device by now)
    char* H = w->s_pin + o_res;
    if (launch) {
        if (int r = dev_reserve(w, &w->s_out, &w->s_ocap, L.dev_end)) return r;
        char* B = (char*)w->s_out;
        if (timed) HIPCHK(hipEventRecord(w->s_ev[2], w->stream));
        hipLaunchKernelGGL(k_snap<true>, dim3((unsigned)((nn + kTPB - 1) / kTPB)), dim3(kTPB), 0, w->stream,
                           (const SnapTab*)w->s_tab_d, (const uint64_t*)w->d.pmem, w->d.fan_desc,
                           (const SnapReq*)(A + a_req), n, (uint32_t*)nullptr, (const uint32_t*)(A + a_base),
                           (uint32_t*)(B + L.hdr), (int32_t*)(B + L.p_pid), (uint64_t*)(B + L.p_bits),
                           heads ? (uint64_t*)(B + L.p_head) : (uint64_t*)nullptr, (int32_t*)(B + L.r_rec),
                           (uint64_t*)(B + L.r_used), (uint32_t*)(B + L.r_cell), (int32_t*)(B + L.r_slot), Pd, Rd);
        if (Rd && Cd) {
            const uint64_t blocks = ((uint64_t)Rd * 64 + kTPB - 1) / kTPB;
            hipLaunchKernelGGL(k_snap_cells, dim3((unsigned)blocks), dim3(kTPB), 0, w->stream, (const SnapTab*)w->s_tab_d,
                               (const int32_t*)(B + L.r_rec), (const int32_t*)(B + L.r_slot),
                               (const uint64_t*)(B + L.r_used), (const uint32_t*)(B + L.r_cell), Rd,
                               (uint64_t*)(B + L.cells), Cd);
        }
        HIPCHK(hipGetLastError());
        if (timed) HIPCHK(hipEventRecord(w->s_ev[3], w->stream));
        HIPCHK(hipMemcpyAsync(H, B, L.end, hipMemcpyDeviceToHost, w->stream));
        HIPCHK(hipStreamSynchronize(w->stream));
        out->bytes = (int64_t)L.end;
        if (timed) {
            float m0 = 0, m1 = 0;
            HIPCHK(hipEventElapsedTime(&m0, w->s_ev[0], w->s_ev[1]));
            HIPCHK(hipEventElapsedTime(&m1, w->s_ev[2], w->s_ev[3]));
            out->kernel_ms = (double)m0 + (double)m1;
        }
    }
    uint32_t* hdr = (uint32_t*)(H + L.hdr);
    int32_t* p_pid = (int32_t*)(H + L.p_pid);
    uint64_t* p_bits = (uint64_t*)(H + L.p_bits);
    uint64_t* p_head = heads ? (uint64_t*)(H + L.p_head) : nullptr;
    int32_t* r_rec = (int32_t*)(H + L.r_rec);
    uint64_t* r_used = (uint64_t*)(H + L.r_used);
    uint32_t* r_cell = (uint32_t*)(H + L.r_cell);
    uint64_t* cells = (uint64_t*)(H + L.cells);
    // the host's runs behind the kernels': nothing is moved
    uint32_t pa = Pd, ra = Rd;
    for (size_t h = 0; h < host.size(); h++) {
        const size_t i = (size_t)host[h];
        hdr[i] = pa;
        hdr[nn + i] = h_np[h];
        hdr[2 * nn + i] = ra;
        hdr[3 * nn + i] = h_nr[h];
        pa += h_np[h];
        ra += h_nr[h];
    }
    for (size_t k = 0; k < hp_pid.size(); k++) {
        p_pid[Pd + k] = hp_pid[k];
        p_bits[Pd + k] = hp_bits[k];
        if (p_head) p_head[Pd + k] = hp_head[k];
    }
    for (size_t k = 0; k < hr_rec.size(); k++) {
        r_rec[Rd + k] = hr_rec[k];
        r_used[Rd + k] = hr_used[k];
        r_cell[Rd + k] = Cd + hr_cell[k];
    }
    if (!hcells.empty()) memcpy(cells + Cd, hcells.data(), hcells.size() * 8);
    out->p_first = hdr;
    out->p_count = hdr + nn;
    out->r_first = hdr + 2 * nn;
    out->r_count = hdr + 3 * nn;
    out->p_pid = p_pid;
    out->p_bits = p_bits;
    out->p_head = p_head;
    out->r_rec = r_rec;
    out->r_used = r_used;
    out->r_cell = r_cell;
    out->cells = cells;
    return NFK_OK;
}

int nfk_snapshot_objects(void* world, int32_t n, const int64_t* gh, const int64_t* gd, const uint8_t* view,
                         nfk_snapshot* out) {
    World* w = (World*)world;
    if (!w) return fail(NFK_ERR_ARG, "null world");
    if (!out || n < 0 || (n && (!gh || !gd || !view))) return fail(NFK_ERR_ARG, "null argument");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    if (n > kSnapMaxRequests) return fail(NFK_ERR_CAPACITY, "snapshot: too many requests in one batch");
    std::vector<int32_t> obj(n);
    if (int rl = find_many_par(w, n, gh, gd, obj.data())) return rl;
    return snapshot(w, n, obj.data(), gh, gd, view, out);
}

int nfk_snapshot_objects_obj(void* world, int32_t n, const int32_t* obj, const uint8_t* view, nfk_snapshot* out) {
    World* w = (World*)world;
    if (!w) return fail(NFK_ERR_ARG, "null world");
    if (!out || n < 0 || (n && (!obj || !view))) return fail(NFK_ERR_ARG, "null argument");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    if (n > kSnapMaxRequests) return fail(NFK_ERR_CAPACITY, "snapshot: too many requests in one batch");
    const int32_t* lo = live_objects(w, n, obj);
    const std::vector<int32_t> o(lo, lo + n);  // (w->look is the lookups' scratch)
    return snapshot(w, n, o.data(), nullptr, nullptr, view, out);
}

int nfk_exist_schedule(void* world, int64_t gh, int64_t gd, int32_t kind, int32_t* exists) {
    World* w = (World*)world;
    if (!w || !exists) return fail(NFK_ERR_ARG, "null argument");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    if (kind < 0 || kind >= w->cfg.n_kind) return fail(NFK_ERR_ARG, "bad kind");
    *exists = 0;
    const int32_t o = w->obj_of.find(gh, gd);
    if (o < 0) return NFK_OK;  // no schedule map for the object
    for (const auto& h : w->hops)
        if (h.code == 3 && h.slot == (uint32_t)o) return NFK_OK;  // RemoveSchedule(self) erased it
    uint64_t word = 0;
    HIPCHK(hipStreamSynchronize(w->stream));
    if (w->src_row[o] >= 0) {
        HIPCHK(hipMemcpy(&word, w->ins_rows + (size_t)w->src_row[o] * w->row_words + w->n_pw + 4 * kind + 1, 8,
                         hipMemcpyDeviceToHost));
    } else if (w->slot_of_obj[o] >= 0) {
        // (the slot's schedule word: the present bit is bit 0 in either form)
        HIPCHK(hipMemcpy(&word, w->d.s_word + (size_t)kind * w->d.s_wstr + w->slot_of_obj[o], 8, hipMemcpyDeviceToHost));
        word <<= 32;
    }
    *exists = (int32_t)((word >> 32) & kStPresent);
    return NFK_OK;
}

int nfk_watch_props(void* world, int32_t n, const int32_t* pid) {
    World* w = (World*)world;
    if (!w || n < 0 || (n && !pid)) return fail(NFK_ERR_ARG, "null argument");
    uint64_t m[2] = {0, 0};
    for (int32_t i = 0; i < n; i++) {
        if (pid[i] < 0 || pid[i] >= w->n_if) return fail(NFK_ERR_ARG, "nfk_watch_props: not an int / f64 property");
        m[pid[i] >> 6] |= 1ull << (pid[i] & 63);
    }
    w->chain_watch[0] = m[0];
    w->chain_watch[1] = m[1];
    return NFK_OK;
}

static int update_guid_ranks(World* w);

int nfk_read_chain(void* world, int32_t cap, int32_t* n, int32_t* obj, int32_t* kind, int32_t* op, int32_t* pid,
                   uint64_t* old_bits, uint64_t* new_bits) {
    World* w = (World*)world;
    if (!w || !n || cap < 0) return fail(NFK_ERR_ARG, "null argument");
    *n = 0;
    if (!w->chain_ran) return NFK_OK;
    // the tiles' counts -> dense bases (and the total), on the world's stream after the frame
    const int32_t nt = w->chain_tiles;
    const size_t s_db = 0, s_k1 = (((size_t)nt + 1) * 4 + 255) & ~(size_t)255;
    if (s_k1 > w->chain_scap) {
        HIPCHK(hipStreamSynchronize(w->stream));
        if (w->chain_scr) HIPCHK(hipFree(w->chain_scr));
        w->chain_scr = nullptr;
        w->chain_scap = s_k1 + 4096;
        HIPCHK(hipMalloc(&w->chain_scr, w->chain_scap));
    }
    uint32_t* db = (uint32_t*)((char*)w->chain_scr + s_db);
    hipLaunchKernelGGL(k_scan_counts, dim3(1), dim3(1024), 0, w->stream, w->chain_cnt_d, db, nt);
    uint32_t cnt = 0;
    HIPCHK(hipMemcpyAsync(&cnt, db + nt, sizeof(cnt), hipMemcpyDeviceToHost, w->stream));
    HIPCHK(hipStreamSynchronize(w->stream));
    *n = (int32_t)cnt;
    const uint32_t m = std::min<uint32_t>(cnt, (uint32_t)cap);
    if (!m) return NFK_OK;
    if (!obj || !kind || !op || !pid || !old_bits || !new_bits) return fail(NFK_ERR_ARG, "null argument");
    // walk order: (NFGUID rank of the object, kind, op) keys sorted on the device, the entries
    // gathered in that order as object-index columns, one copy back
    int r = update_guid_ranks(w);
    if (r) return r;
    int key_bits = 8;
    while ((1ll << (key_bits - 8)) < (long long)std::max(w->n_obj, 1)) key_bits++;
    size_t sort_bytes = 0;
    HIPCHK(rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr,
                                     (uint32_t*)nullptr, cnt, 0, key_bits, w->stream));
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t s_k2 = s_k1 + al((size_t)cnt * 8), s_i1 = s_k2 + al((size_t)cnt * 8), s_i2 = s_i1 + al((size_t)cnt * 4);
    const size_t s_out = s_i2 + al((size_t)cnt * 4), s_tmp = s_out + al((size_t)cnt * 32);
    const size_t need = s_tmp + sort_bytes + 256, pin = (size_t)cnt * 32;
    if (need > w->chain_scap || pin > w->chain_pcap) {
        // (db survives: the scan is redone into the new scratch)
        HIPCHK(hipStreamSynchronize(w->stream));
        if (need > w->chain_scap) {
            HIPCHK(hipFree(w->chain_scr));
            w->chain_scr = nullptr;
            w->chain_scap = need + need / 4 + 4096;
            HIPCHK(hipMalloc(&w->chain_scr, w->chain_scap));
            db = (uint32_t*)((char*)w->chain_scr + s_db);
            hipLaunchKernelGGL(k_scan_counts, dim3(1), dim3(1024), 0, w->stream, w->chain_cnt_d, db, nt);
        }
        if (pin > w->chain_pcap) {
            if (w->chain_pin) HIPCHK(hipHostFree(w->chain_pin));
            w->chain_pin = nullptr;
            w->chain_pcap = pin + pin / 4 + 4096;
            HIPCHK(hipHostMalloc((void**)&w->chain_pin, w->chain_pcap, hipHostMallocDefault));
        }
    }
    char* S = (char*)w->chain_scr;
    uint64_t* k1 = (uint64_t*)(S + s_k1);
    uint64_t* k2 = (uint64_t*)(S + s_k2);
    uint32_t* i1 = (uint32_t*)(S + s_i1);
    uint32_t* i2 = (uint32_t*)(S + s_i2);
    const unsigned gt = (unsigned)std::max(1, std::min(nt, 4096));
    hipLaunchKernelGGL(k_chain_keys, dim3(gt), dim3(kTPB), 0, w->stream, (const ChainEnt*)w->chain_d, (const uint32_t*)db, nt,
                       w->chain_tcap, (const int32_t*)w->slot_obj_d, (const int32_t*)w->rank_d, k1, i1);
    size_t sb = sort_bytes;
    if (cnt <= (uint32_t)kSmallPairs)
        hipLaunchKernelGGL(k_sort_small_pairs, dim3((cnt + kTPB - 1) / kTPB), dim3(kTPB), 0, w->stream, (const uint64_t*)k1,
                           k2, (const uint32_t*)i1, i2, (int)cnt);
    else
        HIPCHK(rocprim::radix_sort_pairs(S + s_tmp, sb, k1, k2, i1, i2, cnt, 0, key_bits, w->stream));
    int32_t* oi = (int32_t*)(S + s_out);
    uint64_t* ou = (uint64_t*)(S + s_out + (size_t)cnt * 16);
    hipLaunchKernelGGL(k_chain_gather, dim3((cnt + kTPB - 1) / kTPB), dim3(kTPB), 0, w->stream, (const ChainEnt*)w->chain_d,
                       (const uint32_t*)i2, (int)cnt, (const int32_t*)w->slot_obj_d, oi, ou);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(w->chain_pin, S + s_out, (size_t)cnt * 32, hipMemcpyDeviceToHost, w->stream));
    HIPCHK(hipStreamSynchronize(w->stream));
    const int32_t* hi = (const int32_t*)w->chain_pin;
    const uint64_t* hu = (const uint64_t*)(w->chain_pin + (size_t)cnt * 16);
    memcpy(obj, hi, (size_t)m * 4);
    memcpy(kind, hi + cnt, (size_t)m * 4);
    memcpy(op, hi + 2 * (size_t)cnt, (size_t)m * 4);
    memcpy(pid, hi + 3 * (size_t)cnt, (size_t)m * 4);
    memcpy(old_bits, hu, (size_t)m * 8);
    memcpy(new_bits, hu + cnt, (size_t)m * 8);
    return NFK_OK;
}

int nfk_read_added(void* world, int32_t cap, int32_t* n, int64_t* gh, int64_t* gd, int32_t* kind) {
    World* w = (World*)world;
    if (!w || !n || cap < 0 || (cap && (!gh || !gd || !kind))) return fail(NFK_ERR_ARG, "null argument");
    *n = 0;
    if (!w->hf_pending) return NFK_OK;
    // the last pass's post-scan entries (the device fold's): which AddSchedule created a schedule
    HIPCHK(hipStreamSynchronize(w->stream));
    uint32_t np = 0;
    HIPCHK(hipMemcpy(&np, w->hf_npost, 4, hipMemcpyDeviceToHost));
    np = std::min<uint32_t>(np, (uint32_t)w->hf_max);
    if (np == 0) return NFK_OK;
    std::vector<uint32_t> sl(np), kd(np), op(np);
    std::vector<uint8_t> added(np);
    HIPCHK(hipMemcpy(sl.data(), w->hf_pslot, np * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(kd.data(), w->hf_pkind, np * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(op.data(), w->hf_pop, np * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(added.data(), w->hf_added, np, hipMemcpyDeviceToHost));
    int32_t k = 0;
    for (uint32_t i = 0; i < np; i++) {
        if (!added[i] || !(op[i] & 2u) || sl[i] >= w->obj_of_slot.size()) continue;
        const int32_t o = w->obj_of_slot[sl[i]];
        if (o < 0) continue;
        if (k < cap) {
            gh[k] = w->gh[o];
            gd[k] = w->gd[o];
            kind[k] = (int32_t)kd[i];
        }
        k++;
    }
    *n = k;
    return NFK_OK;
}

int nfk_set_scene_props(void* world, int32_t pid_scene, int32_t pid_group, int32_t pid_x, int32_t pid_y,
                        int32_t pid_z) {
    World* w = (World*)world;
    if (!w) return fail(NFK_ERR_ARG, "null world");
    const int NI = w->cfg.n_int;
    auto ok_i = [&](int32_t p) { return p == -1 || (p >= 0 && p < NI); };
    auto ok_f = [&](int32_t p) { return p == -1 || (p >= NI && p < w->n_if); };
    if (!ok_i(pid_scene) || !ok_i(pid_group) || !ok_f(pid_x) || !ok_f(pid_y) || !ok_f(pid_z))
        return fail(NFK_ERR_ARG, "SceneID/GroupID must be int properties, X/Y/Z float properties");
    if (w->linked_pid(pid_scene) || w->linked_pid(pid_group))
        return fail(NFK_ERR_ARG, "SceneID/GroupID must not be linked properties (nfk_link_record)");
    w->pid_scene = pid_scene;
    w->pid_group = pid_group;
    w->pid_x = pid_x;
    w->pid_y = pid_y;
    w->pid_z = pid_z;
    return NFK_OK;
}

int nfk_switch_scene(void* world, int64_t gh, int64_t gd, int32_t scene, int32_t group, float x, float y, float z) {
    World* w = (World*)world;
    if (!w) return fail(NFK_ERR_ARG, "null world");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    int32_t o;
    int r = lookup(w, gh, gd, &o);
    if (r) return r;  // "There is no object" (KM:948)
    if (group < 0) return fail(NFK_ERR_ARG, "negative group");
    // the property writes of KM:931-942, in call order (queued like SetProperty*)
    auto put = [&](int32_t pid, uint64_t bits) {
        if (pid >= 0) {
            w->xops.push_back({(uint32_t)o, (uint32_t)pid, bits});
            count_standalone(w, (uint32_t)pid);
        }
    };
    auto dbits = [](double v) {
        uint64_t u;
        memcpy(&u, &v, 8);
        return u;
    };
    if (scene != w->scene[o]) {
        put(w->pid_group, 0);
        put(w->pid_scene, (uint64_t)(int64_t)scene);
    }
    put(w->pid_x, dbits((double)x));
    put(w->pid_y, dbits((double)y));
    put(w->pid_z, dbits((double)z));
    put(w->pid_group, (uint64_t)(int64_t)group);
    // RemoveObjectFromGroup + AddObjectToGroup (KM:928, 944): a new slot in the target group
    if (scene != w->scene[o] || group != w->group[o]) {
        w->vc_log.push_back({o, NFK_VC_SWITCH, w->scene[o], w->group[o], scene, group});
        w->scene[o] = scene;
        w->group[o] = group;
        touch(w, o);
    }
    return NFK_OK;
}

int nfk_destroy_objects(void* world, int32_t n, const int64_t* gh, const int64_t* gd) {
    World* w = (World*)world;
    if (!w || n < 0 || (n && (!gh || !gd))) return fail(NFK_ERR_ARG, "null argument");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    for (int32_t i = 0; i < n; i++) {
        int32_t o;
        int r = lookup(w, gh[i], gd[i], &o);
        if (r) return r;
    }
    for (int32_t i = 0; i < n; i++) {
        const int32_t o = w->obj_of.find(gh[i], gd[i]);
        w->obj_of.erase(gh[i], gd[i]);
        w->alive[o] = 0;
        w->vc_log.push_back({o, NFK_VC_DESTROY, w->scene[o], w->group[o], 0, 0});
        touch(w, o);
    }
    return NFK_OK;
}

int nfk_object_count(void* world, int32_t* n) {
    World* w = (World*)world;
    if (!w || !n) return fail(NFK_ERR_ARG, "null argument");
    *n = w->n_obj;
    return NFK_OK;
}

int nfk_row_words(void* world, int32_t* words) {
    World* w = (World*)world;
    if (!w || !words) return fail(NFK_ERR_ARG, "null argument");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    *words = w->row_words;
    return NFK_OK;
}

int nfk_export_objects(void* world, int32_t n, const int64_t* gh, const int64_t* gd, uint64_t* rows_dev) {
    World* w = (World*)world;
    if (!w || n < 0 || (n && (!gh || !gd || !rows_dev))) return fail(NFK_ERR_ARG, "null argument");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    if (n == 0) return NFK_OK;
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    std::vector<int32_t> src(n), objs(n);
    for (int32_t i = 0; i < n; i++) {
        int r = lookup(w, gh[i], gd[i], &objs[i]);
        if (r) return r;
        if (w->m_flag[objs[i]] || w->slot_of_obj[objs[i]] < 0)
            return fail(NFK_ERR_STATE, "export of an object whose membership already changed in this window");
        src[i] = w->slot_of_obj[objs[i]];
    }
    const auto t1 = clk::now();
    // the slot list from pinned host memory (the last export's k_pack has read its copy)
    if (!w->xpin_done) HIPCHK(hipEventCreateWithFlags(&w->xpin_done, hipEventDisableTiming));
    if (w->xpin_pending) {
        HIPCHK(hipEventSynchronize(w->xpin_done));
        w->xpin_pending = false;
    }
    if ((size_t)n > w->xpin_cap) {
        if (w->xpin) HIPCHK(hipHostFree(w->xpin));
        w->xpin = nullptr;
        const size_t c = std::max<size_t>((size_t)n, 2 * w->xpin_cap);
        w->xpin_cap = 0;  // (until the new buffer exists)
        HIPCHK(hipHostMalloc((void**)&w->xpin, c * sizeof(int32_t), hipHostMallocDefault));
        HIPCHK(hipHostGetDevicePointer((void**)&w->xpin_dev, w->xpin, 0));
        w->xpin_cap = c;
    }
    memcpy(w->xpin, src.data(), (size_t)n * sizeof(int32_t));
    const auto t2 = clk::now();
    hipLaunchKernelGGL(k_pack, dim3(grid_for((size_t)n * w->row_words)), dim3(kTPB), 0, w->stream, w->d,
                       (const int32_t*)w->xpin_dev, n, w->row_words, rows_dev);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(w->xpin_done, w->stream));
    w->xpin_pending = true;
    const auto t3 = clk::now();
    for (int32_t i = 0; i < n; i++) {
        w->obj_of.erase(gh[i], gd[i]);
        w->alive[objs[i]] = 0;
        w->vc_log.push_back({objs[i], NFK_VC_EXPORT, w->scene[objs[i]], w->group[objs[i]], 0, 0});
        touch(w, objs[i]);
    }
    if (getenv("NFGPU_TRACE_MEMBERSHIP")) {
        auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        fprintf(stderr, "nfk_export_objects: %d rows, lookup %.3f ms, upload %.3f ms, launch %.3f ms, unmap %.3f ms\n", n,
                ms(t0, t1), ms(t1, t2), ms(t2, t3), ms(t3, clk::now()));
    }
    return NFK_OK;
}

static int import_common(World* w, int32_t n, const int64_t* gh, const int64_t* gd, const int32_t* scene,
                         const int32_t* group, const uint8_t* cls, const uint8_t* isplayer, const void* rows,
                         hipMemcpyKind kind) {
    if (n < 0 || (n && (!gh || !gd || !scene || !group || !cls || !isplayer || !rows)))
        return fail(NFK_ERR_ARG, "null argument");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first (before it, use nfk_create_objects)");
    if (n == 0) return NFK_OK;
    for (int32_t i = 0; i < n; i++) {
        if (cls[i] >= w->cfg.n_class) return fail(NFK_ERR_ARG, "class id out of range");
        if (group[i] < 0) return fail(NFK_ERR_ARG, "negative group");
        if (w->obj_of.count(gh[i], gd[i])) return fail(NFK_ERR_ARG, "The object has Exists");  // KM:131
        for (int32_t j = 0; j < i; j++)
            if (gh[j] == gh[i] && gd[j] == gd[i]) return fail(NFK_ERR_ARG, "The object has Exists");
    }
    const size_t rb = (size_t)w->row_words * 8;
    if (w->ins_n + n > w->ins_cap) {
        // grow, keeping this window's earlier rows
        const size_t c = std::max(w->ins_n + n, w->ins_cap * 2);
        uint64_t* p = nullptr;
        HIPCHK(hipMalloc((void**)&p, c * rb));
        if (w->ins_n) HIPCHK(hipMemcpyAsync(p, w->ins_rows, w->ins_n * rb, hipMemcpyDeviceToDevice, w->stream));
        HIPCHK(hipStreamSynchronize(w->stream));
        if (w->ins_rows) HIPCHK(hipFree(w->ins_rows));
        w->ins_rows = p;
        w->ins_cap = c;
    }
    HIPCHK(hipMemcpyAsync(w->ins_rows + w->ins_n * w->row_words, rows, (size_t)n * rb, kind, w->stream));
    if (kind == hipMemcpyHostToDevice) HIPCHK(hipStreamSynchronize(w->stream));
    for (int32_t i = 0; i < n; i++) {
        const int32_t o = add_object(w, gh[i], gd[i], scene[i], group[i], cls[i], isplayer[i]);
        w->src_row[o] = (int64_t)(w->ins_n + i);
        w->vc_log.push_back({o, NFK_VC_CREATE, 0, 0, scene[i], group[i]});
        touch(w, o);
    }
    w->ins_n += n;
    return NFK_OK;
}

int nfk_import_objects(void* world, int32_t n, const int64_t* gh, const int64_t* gd, const int32_t* scene,
                       const int32_t* group, const uint8_t* cls, const uint8_t* isplayer, const uint64_t* rows_dev) {
    World* w = (World*)world;
    if (!w) return fail(NFK_ERR_ARG, "null world");
    return import_common(w, n, gh, gd, scene, group, cls, isplayer, rows_dev, hipMemcpyDeviceToDevice);
}

int nfk_spawn_objects(void* world, int32_t n, const int64_t* gh, const int64_t* gd, const int32_t* scene,
                      const int32_t* group, const uint8_t* cls, const uint8_t* isplayer, const uint64_t* props) {
    World* w = (World*)world;
    if (!w || (n > 0 && !props)) return fail(NFK_ERR_ARG, "null argument");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first (before it, use nfk_create_objects)");
    std::vector<uint64_t> rows((size_t)std::max(n, 0) * w->row_words, 0);
    for (int32_t i = 0; i < n; i++)
        memcpy(&rows[(size_t)i * w->row_words], props + (size_t)i * w->n_pw, (size_t)w->n_pw * 8);
    return import_common(w, n, gh, gd, scene, group, cls, isplayer, rows.data(), hipMemcpyHostToDevice);
}

// one device pass over the window's queued calls; calls_only: nfk_execute_calls (nothing fires,
// k_tick runs only the tiles with SetProperty groups)
static int execute_frame(World* w, int64_t now_ms, bool calls_only) {
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    // a device error of an earlier frame (host-mapped, no device read): that frame's outputs are
    // incomplete, so no further frame runs until nfk_summary_get has reported and cleared it
    if (const unsigned e = err_host_bits(w); e & (kErrFanBound | kErrTouch | kErrRankWait))
        return fail(NFK_ERR_DEVICE, std::string("device error of an earlier frame: ") +
                                        ((e & kErrFanBound) ? "a tile's fan-out exceeded its bound"
                                         : (e & kErrTouch)  ? "touch list overflow"
                                                            : "k_tick's rank workgroups gave up waiting") +
                                        " (nfk_summary_get reports and clears it)");
    using clk = std::chrono::steady_clock;
    const bool trace = getenv("NFGPU_TRACE_EXEC") != nullptr;  // host phases to stderr
    clk::time_point tp[6];
    tp[0] = clk::now();
    // ---- membership changes of this window ----
    {
        // the window's host plan overlaps the previous frame still on the GPU; its device phase
        // follows the wait for that frame
        if (!w->mplan) w->mplan.reset(new MemPlan());
        MemPlan& mp = *w->mplan;
        int r = plan_membership(w, mp);
        if (r) return r;  // nothing of the window applied; its calls stay queued
        const int rf = check_fanout(w);  // the last frame's fan-out is complete before it is replaced
        r = commit_membership(w, mp);    // (a planned window is applied either way)
        if (rf) return drop_window(w, rf);
        if (r) return drop_window(w, r);
    }
    // test hook: a failure right after the window's membership changes (tests/test_gpu_parity.py)
    if (const char* inj = getenv("NFGPU_INJECT_EXEC_FAIL"); inj && inj[0] == '1')
        return drop_window(w, fail(NFK_ERR_CAPACITY, "injected failure after the membership changes"));
    // property links: one placeholder SetProperty call per (object, linked property that a record
    // call of the window can hit), so that the slot's group of that property exists for k_links
    // (and the tile counts as one with SetProperty work).  An event names the cell's column (Set),
    // column 0 (AddRow / Remove / ClearRecord) or the column whose index is a Swap's target row.
    bool lk_on = false;
    if ((w->lk_pids[0] | w->lk_pids[1]) && !w->rsq.empty())
        for (const auto& kv : w->rq_index) {
            const uint32_t rec = (uint32_t)(kv.first & 7), o = (uint32_t)(kv.first >> 3);
            if (!w->lk_rows[rec] || w->slot_of_obj[o] < 0) continue;
            lk_on = true;
            uint32_t colm = 0;
            for (uint32_t i : kv.second) {
                const World::RSOp& x = w->rsq[i];
                const uint32_t c = x.op == 0 ? (x.rrc & 0xFF) : x.op == 4 ? (x.rrc & 0xFF) : 0u;
                if (c < NFK_MAX_REC_COLS) colm |= 1u << c;
            }
            for (; colm; colm &= colm - 1) {
                const int pid = w->lk_pid[rec][__builtin_ctz(colm)];
                if (pid < 0) continue;
                w->xops.push_back(World::XOp{o, (uint32_t)pid, 0ull});
                count_standalone(w, (uint32_t)pid);
            }
        }
    if (w->cfg.n_obj) w->xops_h.resize(w->xops.size(), 0);
    if (w->s_unfixed && !w->hops.empty()) fix_schedule_steps(w);
    Dev d = w->d;
    d.now = now_ms;

    tp[1] = clk::now();
    // ---- host-side preparation of queued calls ----
    // Queued calls hold object indices; each resolves to its slot after the window's membership
    // changes (a destroyed / exported object's calls are dropped: "There is no object").  Calls
    // are folded by a stable radix sort of packed words (key << ib | call index), ib = the bits
    // of the largest call index, so the sort moves one array and keeps call order within a key.
    //
    // SetProperty*: (slot, property) groups, each group's calls in call order, folded on the
    // device (k_xkeys, radix sort, k_scan_heads, k_xgroups below): the host hands the calls over as
    // queued.  A tile's events are its slots' program destinations plus its standalone groups
    // (properties no program writes); those are bounded here without the slots: at most one per
    // standalone call, and at most one per slot and standalone property the window sets.
    // (the window's SetProperty calls: xq_n on the device queue, then the host's)
    const size_t n_xdev = w->xq_n, n_xq = n_xdev + w->xops.size(), n_hq = w->hops.size();
    const int64_t max_sa = n_xq ? std::min<int64_t>(w->sa_calls, (int64_t)kTile * (__builtin_popcountll(w->sa_pids[0]) +
                                                                                   __builtin_popcountll(w->sa_pids[1])))
                                : 0;
    // a tile's events: its slots' program destinations plus its standalone Set groups
    {
        const int64_t need_ev = (int64_t)kTile * std::max(w->n_dst_union, 1) + max_sa;
        if (need_ev > w->d.ev_tcap) {
            int r = grow_event_tiles(w, need_ev);
            if (r) return drop_window(w, r);
            d.ev_tcap = w->d.ev_tcap;
            d.ev_slot = w->d.ev_slot; d.ev_pid = w->d.ev_pid; d.ev_old = w->d.ev_old;
            d.ev_new = w->d.ev_new; d.ev_moff = w->d.ev_moff;
            d.ev_old_h = w->d.ev_old_h; d.ev_new_h = w->d.ev_new_h;
        }
    }
    // SetRecordInt / SetRecordFloat: (slot, cell) groups, each group's calls in call order (key
    // slot << 19 | rec << 16 | row << 8 | col).  Record row operations (AddRow / Remove /
    // ClearRecord): one list per (slot, record) that has any, with every call on that pair (its
    // SetRecord calls too, whose groups k_rsets then leaves to k_rrows: rs_rrc bit 31) in call
    // order.  The slots with groups or lists, in slot order, are each run by k_rset_slots; a record
    // tile's extra events are bounded by its groups plus its lists' row events.
    const size_t n_rq = w->rsq.size();
    std::vector<uint32_t>& rs_slot = w->rs_slot_h;
    std::vector<uint32_t>& rs_rrc = w->rs_rrc_h;
    std::vector<uint32_t>& rs_first = w->rs_first_h;
    std::vector<uint32_t>& rss_slot = w->rss_slot_h;
    std::vector<uint32_t>& rss_g0 = w->rss_g0_h;
    rs_slot.clear();
    rs_rrc.clear();
    rs_first.clear();
    rss_slot.clear();
    rss_g0.clear();
    std::vector<uint32_t> rss_l0, rl_slot, rl_rec, rl_c0, rl_ev0, rc_code, rc_aux;
    std::vector<uint64_t> rc_bits, rc_bits_h;
    std::vector<uint64_t>& rowpairs = w->rowpairs;
    rowpairs.clear();
    std::vector<uint64_t>& rpk = w->rpk;
    rpk.clear();
    const int rib = bits_for(n_rq);
    const uint64_t rim = (1ull << rib) - 1;
    int64_t max_rs_tile = 0;
    size_t n_rev = 0;  // row-event bound of the window
    bool any_swap = false;
    std::vector<uint32_t> rs_swap;  // the group pairs the window's Swaps exchange (RecHeads::rs_swap)
    if (n_rq) {
        for (size_t i = 0; i < n_rq; i++)
            if (w->rsq[i].op) {
                const int32_t sl = w->slot_of_obj[w->rsq[i].obj];
                if (sl >= 0) rowpairs.push_back(((uint64_t)(uint32_t)sl << 3) | (w->rsq[i].rrc >> 16));
                any_swap = any_swap || (sl >= 0 && w->rsq[i].op == 4);
            }
        if (lk_on)  // a linked record's calls always form a list: one pair per (object, record), not per call
            for (const auto& kv : w->rq_index) {
                const int32_t sl = w->slot_of_obj[kv.first >> 3];
                if (sl >= 0 && w->lk_rows[kv.first & 7]) rowpairs.push_back(((uint64_t)(uint32_t)sl << 3) | (kv.first & 7));
            }
        std::sort(rowpairs.begin(), rowpairs.end());
        rowpairs.erase(std::unique(rowpairs.begin(), rowpairs.end()), rowpairs.end());
        auto pair_of = [&](uint32_t sl, uint32_t rec) -> int64_t {
            if (rowpairs.empty()) return -1;
            const uint64_t key = ((uint64_t)sl << 3) | rec;
            auto it = std::lower_bound(rowpairs.begin(), rowpairs.end(), key);
            return (it != rowpairs.end() && *it == key) ? (int64_t)(it - rowpairs.begin()) : -1;
        };
        rpk.resize(n_rq);
        uint64_t kor = 0;
        size_t k = 0;
        for (size_t i = 0; i < n_rq; i++) {
            if (w->rsq[i].op) continue;
            const int32_t sl = w->slot_of_obj[w->rsq[i].obj];
            if (sl < 0) continue;  // destroyed / exported in this window
            const uint64_t key = ((uint64_t)(uint32_t)sl << 19) | w->rsq[i].rrc;
            kor |= key;
            rpk[k++] = (key << rib) | i;
        }
        rpk.resize(k);
        if (bits_for(kor) + rib > 64) return drop_window(w, fail(NFK_ERR_CAPACITY, "too many queued SetRecord calls"));
        radix_sort_packed(rpk, w->rpk_t, rib, bits_for(kor));
        uint64_t prev = ~0ull;
        for (size_t i = 0; i < k; i++) {
            const uint64_t key = rpk[i] >> rib;
            if (key == prev) continue;
            prev = key;
            const uint32_t sl = (uint32_t)(key >> 19), rrc = (uint32_t)(key & 0x7FFFF);
            rs_slot.push_back(sl);
            rs_rrc.push_back(rrc | (pair_of(sl, rrc >> 16) >= 0 ? 0x80000000u : 0u));
            rs_first.push_back((uint32_t)i);
        }
        // SwapRowInfo: the window's Update log follows the row, so k_rrows exchanges the two rows'
        // groups with their cells.  A cell without a queued Set gets a group (no calls, rs_rrc bit
        // 31) when a Swap can hand it the other row's log: per list in call order, whenever one of
        // (origin, c) and (target, c) has a group the other gets one, closed over chains of swaps.
        // (The groups a list starts from are those of every Set of its window: a superset of the
        // Sets before the Swap, and a group without a log raises nothing.)
        if (any_swap) {
            std::vector<uint64_t> extra;
            std::vector<uint32_t> cellset;
            for (const auto& kv : w->rq_index) {
                const int32_t sl = w->slot_of_obj[kv.first >> 3];
                if (sl < 0) continue;
                bool sw = false;
                for (uint32_t i : kv.second) sw = sw || w->rsq[i].op == 4;
                if (!sw) continue;
                const uint32_t rec = (uint32_t)(kv.first & 7);
                const int cols = w->tab.rec_cols[rec];
                cellset.clear();  // row << 8 | col, sorted
                for (uint32_t i : kv.second)
                    if (w->rsq[i].op == 0) cellset.push_back(w->rsq[i].rrc & 0xFFFF);
                std::sort(cellset.begin(), cellset.end());
                cellset.erase(std::unique(cellset.begin(), cellset.end()), cellset.end());
                auto has = [&](uint32_t key) { return std::binary_search(cellset.begin(), cellset.end(), key); };
                auto add = [&](uint32_t key) {
                    cellset.insert(std::lower_bound(cellset.begin(), cellset.end(), key), key);
                    extra.push_back(((uint64_t)(uint32_t)sl << 19) | (rec << 16) | key);
                };
                for (uint32_t i : kv.second) {
                    if (w->rsq[i].op != 4) continue;
                    const uint32_t a = (w->rsq[i].rrc >> 8) & 0xFF, b = w->rsq[i].rrc & 0xFF;
                    for (uint32_t c = 0; a != b && c < (uint32_t)cols; c++) {
                        const bool ha = has((a << 8) | c), hb = has((b << 8) | c);
                        if (ha && !hb) add((b << 8) | c);
                        if (hb && !ha) add((a << 8) | c);
                    }
                }
            }
            if (!extra.empty()) {
                std::sort(extra.begin(), extra.end());
                std::vector<uint32_t> s2, r2, f2;
                const size_t ng0 = rs_slot.size();
                for (size_t gi = 0, xi = 0; gi < ng0 || xi < extra.size();) {
                    const uint64_t kg = gi < ng0 ? ((uint64_t)rs_slot[gi] << 19) | (rs_rrc[gi] & 0x7FFFF) : ~0ull;
                    const uint64_t kx = xi < extra.size() ? extra[xi] : ~0ull;
                    if (kx < kg) {
                        s2.push_back((uint32_t)(kx >> 19));
                        r2.push_back((uint32_t)(kx & 0x7FFFF) | 0x80000000u);
                        f2.push_back(gi < ng0 ? rs_first[gi] : (uint32_t)k);
                        xi++;
                    } else {
                        s2.push_back(rs_slot[gi]);
                        r2.push_back(rs_rrc[gi]);
                        f2.push_back(rs_first[gi]);
                        gi++;
                    }
                }
                rs_slot.swap(s2);
                rs_rrc.swap(r2);
                rs_first.swap(f2);
            }
        }
        rs_first.push_back((uint32_t)k);
        // the group of (slot, rec << 16 | row << 8 | col), or -1
        auto group_of = [&](uint32_t sl, uint32_t rrc) -> int64_t {
            const uint64_t key = ((uint64_t)sl << 19) | (rrc & 0x7FFFF);
            size_t lo = 0, hi = rs_slot.size();
            while (lo < hi) {
                const size_t m = (lo + hi) / 2;
                const uint64_t km = ((uint64_t)rs_slot[m] << 19) | (rs_rrc[m] & 0x7FFFF);
                if (km < key) lo = m + 1;
                else hi = m;
            }
            return lo < rs_slot.size() && (((uint64_t)rs_slot[lo] << 19) | (rs_rrc[lo] & 0x7FFFF)) == key ? (int64_t)lo : -1;
        };
        // the row-operation lists (one per pair, pair order), their calls in call order
        const size_t npair = rowpairs.size();
        if (npair) {
            std::vector<uint32_t> cnt(npair + 1, 0);
            std::vector<int64_t> call_pair(n_rq, -1);
            for (size_t i = 0; i < n_rq; i++) {
                const int32_t sl = w->slot_of_obj[w->rsq[i].obj];
                if (sl < 0) continue;
                call_pair[i] = pair_of((uint32_t)sl, w->rsq[i].rrc >> 16);
                if (call_pair[i] >= 0) cnt[call_pair[i]]++;
            }
            rl_c0.assign(npair + 1, 0);
            for (size_t q = 0; q < npair; q++) rl_c0[q + 1] = rl_c0[q] + cnt[q];
            rc_code.assign(rl_c0[npair], 0);
            rc_aux.assign(rl_c0[npair], 0);
            rc_bits.assign(rl_c0[npair], 0);
            if (w->rec_obj) rc_bits_h.assign(rl_c0[npair], 0);
            rl_ev0.assign(npair, 0);
            std::vector<uint32_t> fill(rl_c0.begin(), rl_c0.end() - 1), evb(npair, 0);
            for (size_t i = 0; i < n_rq; i++) {
                if (call_pair[i] < 0) continue;
                const World::RSOp& x = w->rsq[i];
                const int64_t q = call_pair[i];
                const uint32_t at = fill[q]++;
                const uint32_t rec = x.rrc >> 16, row = (x.rrc >> 8) & 0xFF, col = x.rrc & 0xFF;
                rc_code[at] = x.op | (row << 8) | (col << 16);
                rc_bits[at] = x.bits;
                if (w->rec_obj) rc_bits_h[at] = w->rsq_head(i);
                if (x.op == 0) {  // its cell's group (binary search over the sorted groups)
                    rc_aux[at] = (uint32_t)group_of((uint32_t)(rowpairs[q] >> 3), x.rrc);
                } else if (x.op == 4) {  // the columns in which both rows have a group: their logs change places
                    rc_aux[at] = (uint32_t)(rs_swap.size() / 2);
                    const uint32_t sl = (uint32_t)(rowpairs[q] >> 3);
                    for (uint32_t c = 0; row != col && c < (uint32_t)w->tab.rec_cols[rec]; c++) {
                        const int64_t ga = group_of(sl, (rec << 16) | (row << 8) | c);
                        const int64_t gb = group_of(sl, (rec << 16) | (col << 8) | c);
                        if (ga < 0 || gb < 0) continue;
                        rs_swap.push_back((uint32_t)ga);
                        rs_swap.push_back((uint32_t)gb);
                    }
                    rc_bits[at] = rs_swap.size() / 2 - rc_aux[at];
                    evb[q] += 1u;
                } else {
                    rc_aux[at] = x.aux;
                    evb[q] += x.op == 3 ? (uint32_t)w->tab.rec_rows[rec] : 1u;
                }
            }
            for (size_t q = 0; q < npair; q++) {
                rl_slot.push_back((uint32_t)(rowpairs[q] >> 3));
                rl_rec.push_back((uint32_t)(rowpairs[q] & 7));
                rl_ev0[q] = (uint32_t)n_rev;
                n_rev += evb[q];
            }
            // the tile bound: per record tile, its groups plus its lists' row-event bounds
            // (the groups and the lists are both in slot order: one merge, no sort of an entry per group)
            for (size_t g = 0, q = 0; g < rs_slot.size() || q < npair;) {
                const uint32_t tg = g < rs_slot.size() ? rs_slot[g] / kRTile : 0xFFFFFFFFu;
                const uint32_t tq = q < npair ? rl_slot[q] / kRTile : 0xFFFFFFFFu;
                const uint32_t tile = std::min(tg, tq);
                int64_t t = 0;
                for (; g < rs_slot.size() && rs_slot[g] / kRTile == tile; g++) t += 1;
                for (; q < npair && rl_slot[q] / kRTile == tile; q++) t += evb[q];
                max_rs_tile = std::max(max_rs_tile, t);
            }
        } else {
            uint32_t cur_rt = 0xFFFFFFFFu;
            int64_t tile_groups = 0;
            for (size_t g = 0; g < rs_slot.size(); g++) {
                if (rs_slot[g] / kRTile != cur_rt) {
                    cur_rt = rs_slot[g] / kRTile;
                    tile_groups = 0;
                }
                max_rs_tile = std::max(max_rs_tile, ++tile_groups);
            }
        }
        // the slots with record work: groups or lists, in slot order
        for (size_t gi = 0, pi = 0; gi < rs_slot.size() || pi < rl_slot.size();) {
            const uint32_t sl = std::min(gi < rs_slot.size() ? rs_slot[gi] : 0xFFFFFFFFu,
                                         pi < rl_slot.size() ? rl_slot[pi] : 0xFFFFFFFFu);
            rss_slot.push_back(sl);
            rss_g0.push_back((uint32_t)gi);
            rss_l0.push_back((uint32_t)pi);
            while (gi < rs_slot.size() && rs_slot[gi] == sl) gi++;
            while (pi < rl_slot.size() && rl_slot[pi] == sl) pi++;
        }
        // a record tile's events: its slots' record-program cells plus its SetRecord groups
        int64_t cells = 0;
        for (int j = 0; j < d.n_rops; j++) cells += d.rops[j].rows;
        const int64_t need_re = (int64_t)kRTile * std::max<int64_t>(cells, 1) + max_rs_tile;
        if (need_re > w->d.re_tcap) {
            int r = grow_rec_tiles(w, need_re);
            if (r) return drop_window(w, r);
            d.re_tcap = w->d.re_tcap;
            d.re_rrc = w->d.re_rrc; d.re_old = w->d.re_old;
            d.re_new = w->d.re_new; d.re_moff = w->d.re_moff;
        }
    }
    const size_t ngr = rs_slot.size(), nrss = rss_slot.size(), nrc = rpk.size();
    tp[2] = clk::now();
    // schedule calls: pre-scan entries (remove-list key owner, RemoveSchedule(self)) and post-scan
    // (slot, kind) entries (remove, add), folded on the device (k_hkeys, radix sort, k_hfold;
    // nfgpu_kernels.hip states the reference's rules).  Their counts stay on the device: k_pre_hostops
    // and k_post_hostops read them, nfk_read_added reads them back.

    // k_tick runs the programs on the working set fixed at commit (Dev::u_*); a schema whose
    // working set does not fit the register slots runs k_tick_touch
    const bool use_u = w->u_ok && !(d.ablate & kAblPerKind);
    // a calls-only pass runs k_tick on the tiles with SetProperty groups only (k_xgroups marks them)
    d.tile_work = nullptr;
    if (calls_only && use_u && d.n_tiles) {
        int r = dev_reserve(w, (void**)&w->tile_work_d, &w->tile_work_cap, (size_t)d.n_tiles);
        if (r) return drop_window(w, r);
        if (hipMemsetAsync(w->tile_work_d, 0, (size_t)d.n_tiles, w->stream) != hipSuccess)
            return drop_window(w, fail(NFK_ERR_HIP, "hipMemsetAsync (tile_work)"));
        d.tile_work = w->tile_work_d;
    }

    tp[3] = clk::now();
    // ---- uploads through the pinned arena ----
    // (the SetProperty calls as queued: (object, property, bits) and the head halves)
    // (schedule calls: staged as queued; pre / post entries at most 2 per call, counted on the device)
    const size_t ng = n_xq, nhq = n_hq, npre = 2 * n_hq, npost = 2 * n_hq;
    const size_t n_xhost = ng - n_xdev;  // (uploaded; the device queue's calls are there already)
    size_t off_xc = 0;
    size_t off_hc = align16(off_xc + n_xhost * sizeof(World::XOp));
    size_t off_rs = align16(off_hc + nhq * sizeof(World::HOp)), off_rr = align16(off_rs + ngr * 4);
    size_t off_rf = align16(off_rr + ngr * 4), off_rb = align16(off_rf + (ngr + 1) * 4);
    size_t off_ss = align16(off_rb + nrc * 8), off_sg = align16(off_ss + nrss * 4);
    const bool objs = w->cfg.n_obj > 0;
    size_t off_xh = align16(off_sg + nrss * 4);  // head halves of the calls (object properties)
    // record row-operation lists
    const size_t nrl = rl_slot.size(), nrcall = rc_code.size(), nval = w->rvals.size();
    size_t off_l0 = align16(off_xh + (objs ? ng * 8 : 0)), off_ls = align16(off_l0 + (nrl ? nrss * 4 : 0));
    size_t off_lr = align16(off_ls + nrl * 4), off_lc = align16(off_lr + nrl * 4);
    size_t off_le = align16(off_lc + (nrl ? (nrl + 1) * 4 : 0)), off_cc = align16(off_le + nrl * 4);
    size_t off_ca = align16(off_cc + nrcall * 4), off_cb = align16(off_ca + nrcall * 4);
    size_t off_rv = align16(off_cb + nrcall * 8);
    // the SetRecordObject calls' head halves, beside rs_bits and rc_bits (a world with an object column)
    const bool robj = w->rec_obj;
    size_t off_rbh = align16(off_rv + (nrl ? nval * 8 : 0)), off_cbh = align16(off_rbh + (robj ? nrc * 8 : 0));
    const size_t off_sw = align16(off_cbh + (robj ? nrcall * 8 : 0));  // the Swaps' group pairs
    size_t total = align16(off_sw + rs_swap.size() * 4);
    // device fold scratch: keys, sorted keys, call indices, sorted indices, group starts [ng + 1],
    // the groups (slot, property, first call [ng + 1]), the sorted values (and head halves), then
    // the radix sort's temporary storage
    const int xkey_bits = bits_for((uint64_t)std::max(w->d.cap, 1)) + 8;  // (~0: no slot, sorts last)
    size_t xf_sort = 0;
    const size_t xa = (ng * 8 + 255) & ~(size_t)255, xa4 = ((ng + 1) * 4 + 255) & ~(size_t)255;
    const size_t xo_k1 = 0, xo_k2 = xo_k1 + xa, xo_i1 = xo_k2 + xa, xo_i2 = xo_i1 + xa4, xo_gi = xo_i2 + xa4,
                 xo_xs = xo_gi + xa4, xo_xp = xo_xs + xa4, xo_xf = xo_xp + xa4, xo_xb = xo_xf + xa4,
                 xo_xh = xo_xb + xa, xo_tmp = xo_xh + (objs ? xa : 0);
    if (ng) {
        int r = dev_reserve(w, (void**)&w->xs_buf, &w->xs_cap, ng * (objs ? 32 : 16));
        if (r) return drop_window(w, r);
        HIPCHK(rocprim::radix_sort_pairs(nullptr, xf_sort, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr,
                                         (uint32_t*)nullptr, ng, 0, xkey_bits, w->stream));
        r = dev_reserve(w, &w->xf_buf, &w->xf_cap, xo_tmp + xf_sort + 256);
        if (r) return drop_window(w, r);
    }
    // the schedule-call fold's scratch: keys, sorted keys, indices, sorted indices, per-slot counts
    // and their scans, pre entries, post entries (slot, kind, op, interval, count, time), added
    // flags, the sort's temporary storage
    const int hkey_bits = bits_for((uint64_t)std::max(w->d.cap, 1)) + 6;  // (~0: no slot, sorts last)
    size_t hf_sort = 0;
    const size_t hn8 = (nhq * 8 + 255) & ~(size_t)255, hn4 = ((nhq + 1) * 4 + 255) & ~(size_t)255;
    const size_t hm4 = (npost * 4 + 255) & ~(size_t)255, hm8 = (npost * 8 + 255) & ~(size_t)255;
    const size_t ho_k1 = 0, ho_k2 = hn8, ho_i1 = 2 * hn8, ho_i2 = ho_i1 + hn4, ho_cp = ho_i2 + hn4, ho_cq = ho_cp + hn4,
                 ho_op = ho_cq + hn4, ho_oq = ho_op + hn4, ho_ps = ho_oq + hn4, ho_po = ho_ps + hm4,
                 ho_qs = ho_po + hm4, ho_qk = ho_qs + hm4, ho_qo = ho_qk + hm4, ho_qi = ho_qo + hm4, ho_qc = ho_qi + hm4,
                 ho_qt = ho_qc + hm4, ho_ad = ho_qt + hm8, ho_tmp = ho_ad + hm4;
    if (nhq) {
        HIPCHK(rocprim::radix_sort_pairs(nullptr, hf_sort, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr,
                                         (uint32_t*)nullptr, nhq, 0, hkey_bits, w->stream));
        size_t scan_b = 0;  // (the per-slot count scans: device-wide, n + 1 counts, the last 0)
        HIPCHK(rocprim::exclusive_scan(nullptr, scan_b, (const uint32_t*)nullptr, (uint32_t*)nullptr, 0u, nhq + 1,
                                       rocprim::plus<uint32_t>(), w->stream));
        hf_sort = std::max(hf_sort, scan_b);
        int r = dev_reserve(w, &w->hf_buf, &w->hf_cap, ho_tmp + hf_sort + 256);
        if (r) return drop_window(w, r);
    }
    if (ng || nhq) {  // object -> slot after the window's membership changes
        if (w->obj_slot_dirty || (size_t)w->n_obj * 4 > w->obj_slot_cap) {
            int r = dev_reserve(w, (void**)&w->obj_slot_d, &w->obj_slot_cap, ((size_t)w->n_obj + 1) * 4);
            if (r) return drop_window(w, r);
            HIPCHK(hipMemsetAsync(w->obj_slot_d, 0xFF, (size_t)w->n_obj * 4, w->stream));
            if (d.N > 0)
                hipLaunchKernelGGL(k_obj_slots, dim3((unsigned)((d.N + 255) / 256)), dim3(256), 0, w->stream,
                                   (const int32_t*)w->slot_obj_d, (const uint64_t*)w->fan_desc_w, (int32_t)d.N,
                                   w->obj_slot_d);
            HIPCHK(hipGetLastError());
            w->obj_slot_dirty = false;
        }
    }
    if (nrss) {
        int r = dev_reserve(w, (void**)&w->rs_buf, &w->rs_cap, std::max<size_t>(ngr, 1) * (robj ? 32 : 16));
        if (r) return drop_window(w, r);
        r = dev_reserve(w, (void**)&w->rss_buf, &w->rss_cap, nrss * 16);
        if (r) return drop_window(w, r);
        // rs_has [ngr] bytes, then (with lists) rl_cnt [nrl] and rl_ev [row-event bound]
        r = dev_reserve(w, &w->rl_buf, &w->rl_cap, align16(std::max<size_t>(ngr, 1)) + (nrl + n_rev + 1) * 4);
        if (r) return drop_window(w, r);
    }
    LinkDev lkd{};  // (hit / sum null: this window has no call on a linked record)
    if (lk_on && nrl) {
        int r = dev_reserve(w, &w->lk_buf, &w->lk_cap, nrl * 4 * (1 + NFK_MAX_REC_COLS));
        if (r) return drop_window(w, r);
        memcpy(lkd.rows, w->lk_rows, sizeof(lkd.rows));
        memcpy(lkd.pid, w->lk_pid, sizeof(lkd.pid));
        lkd.hit = (uint32_t*)w->lk_buf;
        lkd.sum = lkd.hit + nrl;
    }
    if (total > 0 && (ng || nhq || nrss)) {
        int r = pin_reserve(w, total);
        if (r) return drop_window(w, r);
        char* P = (char*)w->pin;
        if (ng) {
            if (n_xhost) memcpy(P + off_xc, w->xops.data(), n_xhost * sizeof(World::XOp));
            if (objs) memcpy(P + off_xh, w->xops_h.data(), ng * 8);
        }
        if (nhq) memcpy(P + off_hc, w->hops.data(), nhq * sizeof(World::HOp));
        if (nrss) {
            memcpy(P + off_rs, rs_slot.data(), ngr * 4);
            memcpy(P + off_rr, rs_rrc.data(), ngr * 4);
            memcpy(P + off_rf, rs_first.data(), (ngr + 1) * 4);
            uint64_t* rb = (uint64_t*)(P + off_rb);
            for (size_t i = 0; i < nrc; i++) rb[i] = w->rsq[rpk[i] & rim].bits;
            if (robj) {
                uint64_t* rbh = (uint64_t*)(P + off_rbh);
                for (size_t i = 0; i < nrc; i++) rbh[i] = w->rsq_head(rpk[i] & rim);
            }
            memcpy(P + off_ss, rss_slot.data(), nrss * 4);
            memcpy(P + off_sg, rss_g0.data(), nrss * 4);
        }
        if (nrl) {
            memcpy(P + off_l0, rss_l0.data(), nrss * 4);
            memcpy(P + off_ls, rl_slot.data(), nrl * 4);
            memcpy(P + off_lr, rl_rec.data(), nrl * 4);
            memcpy(P + off_lc, rl_c0.data(), (nrl + 1) * 4);
            memcpy(P + off_le, rl_ev0.data(), nrl * 4);
            memcpy(P + off_cc, rc_code.data(), nrcall * 4);
            memcpy(P + off_ca, rc_aux.data(), nrcall * 4);
            memcpy(P + off_cb, rc_bits.data(), nrcall * 8);
            if (robj) memcpy(P + off_cbh, rc_bits_h.data(), nrcall * 8);
            if (nval) memcpy(P + off_rv, w->rvals.data(), nval * 8);
            if (!rs_swap.empty()) memcpy(P + off_sw, rs_swap.data(), rs_swap.size() * 4);
        }
        HIPCHK(hipMemcpyAsync(w->stage, w->pin, total, hipMemcpyHostToDevice, w->stream));
        HIPCHK(hipEventRecord(w->pin_done, w->stream));
        w->pin_pending = true;
    }
    tp[4] = clk::now();
    char* S = (char*)w->stage;
    // the groups as k_xgroups lays them out: n_x = the call count bounds the groups (entries past
    // the frame's groups hold kNoGroupSlot)
    char* XF = (char*)w->xf_buf;
    d.n_x = (int32_t)ng;
    d.x_slot = ng ? (const uint32_t*)(XF + xo_xs) : nullptr;
    d.x_pid = ng ? (const uint32_t*)(XF + xo_xp) : nullptr;
    d.x_first = ng ? (const uint32_t*)(XF + xo_xf) : nullptr;
    d.x_bits = ng ? (const uint64_t*)(XF + xo_xb) : nullptr;
    d.x_old = ng ? (uint64_t*)w->xs_buf : nullptr;
    d.x_new = ng ? (uint64_t*)w->xs_buf + ng : nullptr;
    d.x_bits_h = ng && objs ? (const uint64_t*)(XF + xo_xh) : nullptr;
    d.x_old_h = ng && objs ? (uint64_t*)w->xs_buf + 2 * ng : nullptr;
    d.x_new_h = ng && objs ? (uint64_t*)w->xs_buf + 3 * ng : nullptr;
    d.n_rs = (int32_t)ngr;
    d.n_rss = (int32_t)nrss;
    d.rs_slot = nrss ? (const uint32_t*)(S + off_rs) : nullptr;
    d.rs_rrc = nrss ? (const uint32_t*)(S + off_rr) : nullptr;
    d.rs_first = nrss ? (const uint32_t*)(S + off_rf) : nullptr;
    d.rs_bits = nrss ? (const uint64_t*)(S + off_rb) : nullptr;
    d.rss_slot = nrss ? (const uint32_t*)(S + off_ss) : nullptr;
    d.rss_g0 = nrss ? (const uint32_t*)(S + off_sg) : nullptr;
    d.rs_old = nrss ? (uint64_t*)w->rs_buf : nullptr;
    d.rs_new = nrss ? (uint64_t*)w->rs_buf + ngr : nullptr;
    d.rs_has = nrss ? (uint8_t*)w->rl_buf : nullptr;
    RecHeads& rh = w->rheads;  // (re_old_h / re_new_h: after grow_rec_tiles, above)
    rh.rs_bits_h = nrss && robj ? (const uint64_t*)(S + off_rbh) : nullptr;
    rh.rs_old_h = nrss && robj ? (uint64_t*)w->rs_buf + 2 * ngr : nullptr;
    rh.rs_new_h = nrss && robj ? (uint64_t*)w->rs_buf + 3 * ngr : nullptr;
    rh.rc_bits_h = nrl && robj ? (const uint64_t*)(S + off_cbh) : nullptr;
    rh.rs_swap = rs_swap.empty() ? nullptr : (const uint32_t*)(S + off_sw);
    rh.re_old_h = w->re_old_h;
    rh.re_new_h = w->re_new_h;
    d.rss_ev = nrss ? (uint32_t*)w->rss_buf : nullptr;
    d.rss_msg = nrss ? (uint32_t*)w->rss_buf + nrss : nullptr;
    d.rss_pos = nrss ? (uint32_t*)w->rss_buf + 2 * nrss : nullptr;
    d.rss_pmsg = nrss ? (uint32_t*)w->rss_buf + 3 * nrss : nullptr;
    d.n_rl = (int32_t)nrl;
    d.rss_l0 = nrl ? (const uint32_t*)(S + off_l0) : nullptr;
    d.rl_slot = nrl ? (const uint32_t*)(S + off_ls) : nullptr;
    d.rl_rec = nrl ? (const uint32_t*)(S + off_lr) : nullptr;
    d.rl_c0 = nrl ? (const uint32_t*)(S + off_lc) : nullptr;
    d.rl_ev0 = nrl ? (const uint32_t*)(S + off_le) : nullptr;
    d.rc_code = nrl ? (const uint32_t*)(S + off_cc) : nullptr;
    d.rc_aux = nrl ? (const uint32_t*)(S + off_ca) : nullptr;
    d.rc_bits = nrl ? (const uint64_t*)(S + off_cb) : nullptr;
    d.rvals = nrl ? (const uint64_t*)(S + off_rv) : nullptr;
    d.rl_cnt = nrl ? (uint32_t*)((char*)w->rl_buf + align16(std::max<size_t>(ngr, 1))) : nullptr;
    d.rl_ev = nrl ? d.rl_cnt + nrl : nullptr;
    w->rsq.clear();
    w->rsq_h.clear();
    w->rvals.clear();
    w->rq_index.clear();
    w->ucache.clear();
    w->lcache.clear();
    w->xops.clear();
    w->xq_n = 0;
    w->xops_h.clear();
    w->sa_calls = 0;
    w->sa_pids[0] = w->sa_pids[1] = 0;
    w->hops.clear();
    w->dcache.clear();
    w->ov_last.clear();
    w->ov_prev.clear();

    // (schedule calls queued: e_flags may be set by k_pre_hostops; they are 0 wherever it sets none)
    d.has_pre = nhq > 0;
    char* HF = (char*)w->hf_buf;
    HPost hpost{};
    if (nhq) {
        hpost = HPost{(uint32_t*)(HF + ho_qs), (uint32_t*)(HF + ho_qk), (uint32_t*)(HF + ho_qo), (float*)(HF + ho_qi),
                      (int32_t*)(HF + ho_qc), (int64_t*)(HF + ho_qt)};
        w->hf_pending = true;
        w->hf_max = npost;
        w->hf_npost = (const uint32_t*)(HF + ho_oq) + nhq;
        w->hf_pslot = hpost.slot;
        w->hf_pkind = hpost.kind;
        w->hf_pop = hpost.op;
        w->hf_added = (const uint8_t*)(HF + ho_ad);
    } else {
        w->hf_pending = false;
    }
    if (ng || nhq || nrss) {
        TimeScope ts(w, KT_AUX);
        if (nrss) {
            hipLaunchKernelGGL(k_rs_scatter, dim3((unsigned)((nrss + 255) / 256)), dim3(256), 0, w->stream,
                               d.rss_slot, (int32_t)nrss, d.rs_head);
            if (ngr)
                hipLaunchKernelGGL(k_rsets, dim3((unsigned)((ngr + kTPB - 1) / kTPB)), dim3(kTPB), 0, w->stream, d, rh);
            if (nrl)  // after k_rsets: it clears the has-flags of the lists' groups
                hipLaunchKernelGGL(lkd.hit ? k_rrows<true> : k_rrows<false>, dim3((unsigned)((nrl + kTPB - 1) / kTPB)), dim3(kTPB), 0,
                                   w->stream, d, rh, lkd);
        }
        if (ng) {
            // the device fold: keys (slot << 7 | property) -> stable radix sort -> groups
            const unsigned gx = (unsigned)((ng + 255) / 256);
            // the calls in call order: the device queue's, then the host's appended to it
            const XCall* xc = (const XCall*)(S + off_xc);
            if (n_xdev) {
                if (int r = xq_reserve_exec(w, ng)) return drop_window(w, r);
                World::XOp* q = (World::XOp*)w->xq[w->xq_b];
                if (n_xhost)
                    HIPCHK(hipMemcpyAsync(q + n_xdev, S + off_xc, n_xhost * sizeof(World::XOp), hipMemcpyDeviceToDevice,
                                          w->stream));
                xc = (const XCall*)q;
            }
            uint64_t* k1 = (uint64_t*)(XF + xo_k1);
            uint64_t* k2 = (uint64_t*)(XF + xo_k2);
            uint32_t* i1 = (uint32_t*)(XF + xo_i1);
            uint32_t* i2 = (uint32_t*)(XF + xo_i2);
            uint32_t* gi = (uint32_t*)(XF + xo_gi);
            hipLaunchKernelGGL(k_xkeys, dim3(gx), dim3(256), 0, w->stream, xc, (int32_t)ng,
                               (const int32_t*)w->obj_slot_d, k1, i1, (uint32_t*)d.x_slot);
            size_t sb = xf_sort;
            if (ng <= (size_t)kSmallPairs)  // (a window's few calls: one launch instead of the radix passes)
                hipLaunchKernelGGL(k_sort_small_pairs, dim3((unsigned)((ng + kTPB - 1) / kTPB)), dim3(kTPB), 0, w->stream,
                                   (const uint64_t*)k1, k2, (const uint32_t*)i1, i2, (int)ng);
            else
                HIPCHK(rocprim::radix_sort_pairs(XF + xo_tmp, sb, k1, k2, i1, i2, ng, 0, xkey_bits, w->stream));
            hipLaunchKernelGGL(k_scan_heads, dim3(1), dim3(1024), 0, w->stream, (const uint64_t*)k2, (int)ng, gi);
            hipLaunchKernelGGL(k_xgroups, dim3(gx), dim3(256), 0, w->stream, (const uint64_t*)k2, (const uint32_t*)i2,
                               (const uint32_t*)gi, xc, objs ? (const uint64_t*)(S + off_xh) : nullptr, (int32_t)ng,
                               (uint32_t*)d.x_slot, (uint32_t*)d.x_pid, (uint32_t*)d.x_first, (uint64_t*)d.x_bits,
                               (uint64_t*)d.x_bits_h, d.ext_head, (uint8_t*)d.tile_work);
            if (n_xdev) {  // the buffer is free again once the fold has read it; the next window takes the other
                const int b = w->xq_b;
                if (!w->xq_ev[b]) HIPCHK(hipEventCreateWithFlags(&w->xq_ev[b], hipEventDisableTiming));
                HIPCHK(hipEventRecord(w->xq_ev[b], w->stream));
                w->xq_ev_set[b] = true;
                w->xq_b ^= 1;
            }
            if (lk_on) {  // the linked properties' groups keep their values; k_links gives them the window's sums
                LinkPids lp{{w->lk_pids[0], w->lk_pids[1]}};
                hipLaunchKernelGGL(k_sets<true>, dim3((unsigned)((ng + kTPB - 1) / kTPB)), dim3(kTPB), 0, w->stream, d, lp);
                if (lkd.hit)
                    hipLaunchKernelGGL(k_links, dim3((unsigned)((nrl * NFK_MAX_REC_COLS + kTPB - 1) / kTPB)), dim3(kTPB), 0,
                                       w->stream, d, lkd);
            } else {
                hipLaunchKernelGGL(k_sets<false>, dim3((unsigned)((ng + kTPB - 1) / kTPB)), dim3(kTPB), 0, w->stream, d,
                                   LinkPids{});
            }
        }
        if (nhq) {
            // the device fold of the schedule calls: keys -> stable radix sort -> per-slot counts ->
            // scans -> pre / post entries; then the pre-scan effects
            const unsigned gh_ = (unsigned)((nhq + 255) / 256);
            const HCall* hc = (const HCall*)(S + off_hc);
            uint64_t* k1 = (uint64_t*)(HF + ho_k1);
            uint64_t* k2 = (uint64_t*)(HF + ho_k2);
            uint32_t* i1 = (uint32_t*)(HF + ho_i1);
            uint32_t* i2 = (uint32_t*)(HF + ho_i2);
            uint32_t* cp = (uint32_t*)(HF + ho_cp);
            uint32_t* cq = (uint32_t*)(HF + ho_cq);
            uint32_t* op = (uint32_t*)(HF + ho_op);
            uint32_t* oq = (uint32_t*)(HF + ho_oq);
            uint32_t* ps = (uint32_t*)(HF + ho_ps);
            uint32_t* po = (uint32_t*)(HF + ho_po);
            hipLaunchKernelGGL(k_hkeys, dim3(gh_), dim3(256), 0, w->stream, hc, (int32_t)nhq,
                               (const int32_t*)w->obj_slot_d, k1, i1);
            size_t sb = hf_sort;
            if (nhq <= (size_t)kSmallPairs)
                hipLaunchKernelGGL(k_sort_small_pairs, dim3((unsigned)((nhq + kTPB - 1) / kTPB)), dim3(kTPB), 0, w->stream,
                                   (const uint64_t*)k1, k2, (const uint32_t*)i1, i2, (int)nhq);
            else
                HIPCHK(rocprim::radix_sort_pairs(HF + ho_tmp, sb, k1, k2, i1, i2, nhq, 0, hkey_bits, w->stream));
            hipLaunchKernelGGL(k_hfold<false>, dim3((unsigned)((nhq + 1 + 255) / 256)), dim3(256), 0, w->stream,
                               (const uint64_t*)k2, (const uint32_t*)i2,
                               hc, (int32_t)nhq, cp, cq, (const uint32_t*)nullptr, (const uint32_t*)nullptr, ps, po, hpost);
            size_t tb = hf_sort;  // (a mass AddSchedule at start: millions of calls, so a device-wide scan)
            HIPCHK(rocprim::exclusive_scan(HF + ho_tmp, tb, (const uint32_t*)cp, op, 0u, nhq + 1, rocprim::plus<uint32_t>(),
                                           w->stream));
            tb = hf_sort;
            HIPCHK(rocprim::exclusive_scan(HF + ho_tmp, tb, (const uint32_t*)cq, oq, 0u, nhq + 1, rocprim::plus<uint32_t>(),
                                           w->stream));
            hipLaunchKernelGGL(k_hfold<true>, dim3(gh_), dim3(256), 0, w->stream, (const uint64_t*)k2, (const uint32_t*)i2,
                               hc, (int32_t)nhq, cp, cq, (const uint32_t*)op, (const uint32_t*)oq, ps, po, hpost);
            hipLaunchKernelGGL(k_pre_hostops, dim3((unsigned)((npre + 255) / 256)), dim3(256), 0, w->stream,
                               (const uint32_t*)ps, (const uint32_t*)po, (int32_t)npre, d.e_flags, d.s_word, d.n_kind,
                               d.s_wstr, (const uint32_t*)op + nhq);
        }
        HIPCHK(hipGetLastError());
    }
    // k_tick writes its tiles' fan-out itself (its LDS image is reused for the events): property
    // tile t's messages sit at t * msg_tcap, msg_tcap = writable properties x slots x most
    // recipients of one event, so no tile waits for another tile's count.  Worlds whose bound
    // would reserve more than kMsgStrideLimit run k_fanout after k_scan_tiles instead.
    // With the property tiles at a fixed stride, k_records fans out its record tiles the same way
    // after them: msg_rtcap = slots x cells the record ops may change x most recipients of one
    // record event (the scene group's players for a public record, 1 for a private one).
    d.msg_tcap = 0;
    d.fuse_rec = 0;
    d.msg_rb0 = d.msg_rtcap = 0;
    if (use_u && d.n_tiles && !(d.ablate & (kAblNoFuse | kAblNoEmit))) {
        int64_t tcap = (((int64_t)std::max(d.n_w, 1) * kTile + max_sa) * std::max(w->max_np, 1) + 3) & ~(int64_t)3;
        if (d.ablate & kAblTinyTcap) tcap = 4;  // test hook: a bound every busy tile exceeds (kErrFanBound)
        int64_t rtcap = 0;
        bool rfuse = false;
        if (d.has_recops && d.n_rtiles) {
            int64_t cells = 0, per = 0;
            for (int j = 0; j < d.n_rops; j++) cells += d.rops[j].rows;
            auto rper = [&](int rec) {
                for (int c = 0; c < NFK_MAX_CLASSES; c++) {
                    const uint8_t f = w->tab.rflags[c][rec];
                    per = std::max<int64_t>(per, (f & NFK_PUBLIC) ? std::max(w->max_np, 1)
                                                 : ((f & NFK_PRIVATE) && !(f & NFK_UPLOAD)) ? 1 : 0);
                }
            };
            for (int j = 0; j < d.n_rops; j++) rper(d.rops[j].rec);
            if (nrss)  // SetRecord groups and row operations may hit any record
                for (int r = 0; r < d.n_rec; r++)
                    if (w->rec_defined[r]) rper(r);
            rtcap = (((int64_t)kRTile * cells + max_rs_tile) * per + 3) & ~(int64_t)3;  // (16-byte aligned runs)
            rfuse = tcap * d.n_tiles + rtcap * d.n_rtiles <= kMsgStrideLimit;
        }
        const int64_t need = tcap * d.n_tiles + (rfuse ? rtcap * d.n_rtiles
                                                       : w->last_rec_msgs + w->last_rec_msgs / 4) + 1024;
        if (tcap * d.n_tiles <= kMsgStrideLimit) {
            if (need > w->d.msg_cap) {  // grow before the frame (the previous frame's messages are dropped)
                HIPCHK(hipStreamSynchronize(w->stream));
                int r = regrow(w, (void**)&w->d.msg_rcpt, (size_t)need * 4);
                if (r) {
                    w->d.msg_cap = 0;
                    return drop_window(w, r);
                }
                w->d.msg_cap = need;
                d.msg_rcpt = w->d.msg_rcpt;
                d.msg_cap = need;
            }
            d.msg_tcap = (uint32_t)tcap;
            if (rfuse) {
                d.fuse_rec = 1;
                d.msg_rb0 = (uint32_t)(tcap * d.n_tiles);
                d.msg_rtcap = (uint32_t)rtcap;
            }
        }
    }
    d.fuse_fan = d.msg_tcap != 0;
    // a world whose programs guard on record cells (the cells are the last read-only slots): its
    // library kernels are the DynSchemaCells instantiations
    const bool cells = d.n_u > 0 && d.u_pid[d.n_u - 1] >= kCellPid;
    // No record pipeline after k_tick: kRankWgs extra workgroups of its launch rank the frame's tiles
    // and the frame has no k_scan_tiles launch (profiles/r19a_rank_workgroups_ab.txt).  Dev::lb_rank =
    // the counts a rank thread takes per pass: one while a pass of one each covers the world
    if (d.fuse_fan && !d.has_recops && d.n_tiles && !(d.ablate & kAblScanKernel) && (!(use_u && w->jit_fn) || w->jit_lb))
        d.lb_rank = (d.n_tiles <= kTPB || (d.ablate & kAblRankPer1)) ? 1 : kRankPer;
    else
        d.lb_rank = 0;
    if (d.lb_rank) {
        if (++w->lb_epoch == 0xFFFFFFFFu) {  // (clear the tags before they could repeat)
            HIPCHK(hipMemsetAsync(w->d.lb_st, 0, std::max<size_t>((size_t)d.cap / kTile, 1) * kRankWgs * 8, w->stream));
            w->lb_epoch = 1;
        }
        d.lb_epoch = w->lb_epoch;
    }
    w->last_tcap = d.msg_tcap;
    w->last_rtcap = d.fuse_rec ? d.msg_rtcap : 0u;
    // per-Set chains of the watched properties: the programs re-run read-only before k_tick
    // (k_chain); a calls-only pass fires nothing and keeps the frame's log
    if (!calls_only) w->chain_ran = false;
    if (!calls_only && (w->chain_watch[0] | w->chain_watch[1]) && d.N) {
        uint32_t kinds = 0;
        int64_t wops = 0;  // (kind, op) pairs whose destination is watched: a bound of the log per slot
        for (int k = 0; k < d.n_kind; k++)
            for (int i = 0; i < w->tab.nops[k]; i++) {
                const nfk_op& op = w->tab.ops[k][i];
                const bool prop_op = op.code == NFK_OP_IADD_CLAMP || op.code == NFK_OP_FLERP ||
                                     op.code == NFK_OP_FAFFINE || op.code == NFK_OP_ISET || op.code == NFK_OP_FSET;
                if (prop_op && op.dst < 128 && ((w->chain_watch[op.dst >> 6] >> (op.dst & 63)) & 1)) {
                    kinds |= 1u << k;
                    wops++;
                }
            }
        // ... and every kind before one of those whose program writes a property a later re-run kind
        // reads (an operand, a guard, or a destination's current value): the reference's functors run
        // in name order on what the earlier ones left (SM:52-80), so the logged (old, new) of a watched
        // Set depend on them.  Closed transitively, latest kind first.  (NFGPU_CHAIN_NO_CLOSURE=1: test
        // hook, the watched kinds only — the round-5 form, which logged wrong (old, new) for such Sets)
        static const bool no_closure = getenv("NFGPU_CHAIN_NO_CLOSURE") && getenv("NFGPU_CHAIN_NO_CLOSURE")[0] == '1';
        if (kinds && !no_closure) {
            auto bit = [](uint64_t (&m)[2], uint32_t p) {
                if (p < 128) m[p >> 6] |= 1ull << (p & 63);
            };
            uint64_t rd[NFK_MAX_KINDS][2] = {}, wr[NFK_MAX_KINDS][2] = {};
            // ... and the record columns: a RIADD_CLAMP writes its (record, column), which the guard
            // cells on that column read as the walk has left it (bit rec * 16 + col)
            uint64_t rdc[NFK_MAX_KINDS][2] = {}, wrc[NFK_MAX_KINDS][2] = {};
            for (int k = 0; k < d.n_kind; k++)
                for (int i = 0; i < w->tab.nops[k]; i++) {
                    const nfk_op& op = w->tab.ops[k][i];
                    if (op.code == NFK_OP_RIADD_CLAMP) bit(wrc[k], (uint32_t)(op.dst >> 8) * 16u + (op.dst & 255u));
                    if (op.code != NFK_OP_IADD_CLAMP && op.code != NFK_OP_FLERP && op.code != NFK_OP_FAFFINE &&
                        op.code != NFK_OP_ISET && op.code != NFK_OP_FSET)
                        continue;
                    bit(wr[k], op.dst);
                    bit(rd[k], op.dst);
                    if (op.flags & NFK_GUARD) {
                        if (op.flags & NFK_GUARD_CELL) bit(rdc[k], cell_rec(op.guard) * 16u + cell_col(op.guard));
                        else bit(rd[k], op.guard & 0xFFFFu);
                        if (op.guard & NFK_GUARD_PROP) bit(rd[k], op.guard >> 19);
                    }
                    if (op.code == NFK_OP_FLERP || ((op.code == NFK_OP_ISET || op.code == NFK_OP_FSET) && (op.flags & NFK_A_PROP)))
                        bit(rd[k], (uint32_t)op.a);
                    if (op.code == NFK_OP_IADD_CLAMP) {
                        if (op.flags & NFK_A_PROP) bit(rd[k], (uint32_t)op.a);
                        if (op.flags & NFK_LO_PROP) bit(rd[k], (uint32_t)op.b);
                        if (op.flags & NFK_HI_PROP) bit(rd[k], (uint32_t)op.c);
                    }
                }
            uint64_t need[2] = {0, 0}, needc[2] = {0, 0};  // what the re-run kinds after position k read
            for (int k = d.n_kind - 1; k >= 0; k--) {
                if (!((kinds >> k) & 1) &&
                    ((wr[k][0] & need[0]) | (wr[k][1] & need[1]) | (wrc[k][0] & needc[0]) | (wrc[k][1] & needc[1])))
                    kinds |= 1u << k;
                if ((kinds >> k) & 1) {
                    need[0] |= rd[k][0];
                    need[1] |= rd[k][1];
                    needc[0] |= rdc[k][0];
                    needc[1] |= rdc[k][1];
                }
            }
        }
        if (kinds) {
            // tile-staged: kTPB slots x the watched (kind, op) pairs per tile (each logs at most once)
            const int32_t nt = (int32_t)((d.N + kTPB - 1) / kTPB);
            const uint32_t tcap = (uint32_t)(kTPB * wops);
            const size_t need = (size_t)nt * tcap;
            if (need > w->chain_cap || nt > w->chain_tiles) {
                HIPCHK(hipStreamSynchronize(w->stream));
                if (need > w->chain_cap) {
                    if (w->chain_d) HIPCHK(hipFree(w->chain_d));
                    w->chain_d = nullptr;
                    w->chain_cap = 0;
                    if (hipMalloc(&w->chain_d, need * sizeof(ChainEnt)) != hipSuccess)
                        return drop_window(w, fail(NFK_ERR_CAPACITY, "hipMalloc (per-Set chain log)"));
                    w->chain_cap = need;
                }
                if (nt > w->chain_tiles) {
                    if (w->chain_cnt_d) HIPCHK(hipFree(w->chain_cnt_d));
                    w->chain_cnt_d = nullptr;
                    w->chain_tiles = 0;
                    HIPCHK(hipMalloc(&w->chain_cnt_d, ((size_t)nt + 1) * sizeof(uint32_t)));
                    w->chain_tiles = nt;
                }
            }
            w->chain_tcap = tcap;
            TimeScope ts(w, KT_CHAIN);
            // on the frame's register working set (the world's hipRTC policy, or the library's tables),
            // else on k_tick_touch's written-property list (NFGPU_CHAIN_U=0 forces that one, for A/B)
            static const bool chain_u = !getenv("NFGPU_CHAIN_U") || getenv("NFGPU_CHAIN_U")[0] != '0';
            ChainEnt* cd = (ChainEnt*)w->chain_d;
            uint32_t* cc = w->chain_cnt_d;
            uint64_t w0 = w->chain_watch[0], w1 = w->chain_watch[1];
            if (chain_u && use_u && w->jit_chain_fn) {
                void* args[] = {&d, &cd, &cc, (void*)&tcap, &kinds, &w0, &w1};
                HIPCHK(hipModuleLaunchKernel(w->jit_chain_fn, (unsigned)nt, 1, 1, kTPB, 1, 1, 0, w->stream, args, nullptr));
            } else if (chain_u && use_u && d.n_u <= 8) {
                if (cells) hipLaunchKernelGGL((k_chain_u<8, DynSchemaCells>), dim3((unsigned)nt), dim3(kTPB), 0, w->stream, d, cd, cc, tcap, kinds, w0, w1);
                else hipLaunchKernelGGL((k_chain_u<8, DynSchema>), dim3((unsigned)nt), dim3(kTPB), 0, w->stream, d, cd, cc, tcap, kinds, w0, w1);
            } else if (chain_u && use_u && d.n_u <= 12) {
                if (cells) hipLaunchKernelGGL((k_chain_u<12, DynSchemaCells>), dim3((unsigned)nt), dim3(kTPB), 0, w->stream, d, cd, cc, tcap, kinds, w0, w1);
                else hipLaunchKernelGGL((k_chain_u<12, DynSchema>), dim3((unsigned)nt), dim3(kTPB), 0, w->stream, d, cd, cc, tcap, kinds, w0, w1);
            } else if (chain_u && use_u) {
                if (cells) hipLaunchKernelGGL((k_chain_u<16, DynSchemaCells>), dim3((unsigned)nt), dim3(kTPB), 0, w->stream, d, cd, cc, tcap, kinds, w0, w1);
                else hipLaunchKernelGGL((k_chain_u<16, DynSchema>), dim3((unsigned)nt), dim3(kTPB), 0, w->stream, d, cd, cc, tcap, kinds, w0, w1);
            } else {
                hipLaunchKernelGGL(k_chain, dim3((unsigned)nt), dim3(kTPB), 0, w->stream, d, w->chain_d, w->chain_cnt_d, tcap,
                                   kinds, w->chain_watch[0], w->chain_watch[1]);
            }
            HIPCHK(hipGetLastError());
            w->chain_ran = true;
            w->chain_tiles = nt;
        }
    }
    if (d.n_tiles) {
        TimeScope ts(w, KT_TICK);
        size_t lds = (size_t)std::max(d.n_w, 1) * kTPB * 8 + (size_t)std::max(d.n_kind, 1) * kTPB * 4;
        const bool jit = use_u && w->jit_fn;
        if (d.fuse_fan) {  // the fan-out's message window takes what LDS the variant's occupancy
                           // leaves (waves per SIMD = workgroups per CU; ~2.3 KB static each)
            const int waves = jit ? w->jit_waves : tick_waves(d.n_u, d.ablate);
            lds = std::max(lds, (size_t)(163840 / waves - 2560) & ~(size_t)1023);
        }
        d.lds_words = (int32_t)(lds / 4);
        // (k_tick deals its tiles XCD-contiguous, xcd_tile: config[3] 342 -> 331 us against round-robin,
        // config[1] unchanged, profiles/r11o_ktick_xcd_map_ab.txt)
        // the variant whose register slots hold the frame's working set (no spills at 6 or more
        // waves per SIMD): this schema's own k_tick, else a generic instantiation
        // (... and the rank workgroups after the tiles': Dev::lb_rank)
        const dim3 g((unsigned)(d.n_tiles + (d.lb_rank ? kRankWgs : 0))), b(kTPB);
        if (jit) {
            void* args[] = {&d};
            HIPCHK(hipModuleLaunchKernel(w->jit_fn, g.x, 1, 1, kTPB, 1, 1, (unsigned)lds, w->stream,
                                         args, nullptr));
        } else if (use_u && cells) {  // the library's instantiations with the guard-cell loads and replay
            if (d.n_u <= 8)
                hipLaunchKernelGGL((k_tick<kWavesU8, 8, DynSchemaCells>), g, b, lds, w->stream, d);
            else if (d.n_u <= 12)
                hipLaunchKernelGGL((k_tick<kWavesU12, 12, DynSchemaCells>), g, b, lds, w->stream, d);
            else
                hipLaunchKernelGGL((k_tick<6, 16, DynSchemaCells>), g, b, lds, w->stream, d);
        } else if (use_u && d.n_u <= 8)
            hipLaunchKernelGGL((k_tick<kWavesU8, 8>), g, b, lds, w->stream, d);
        else if (use_u && d.n_u <= 12)
            hipLaunchKernelGGL((k_tick<kWavesU12, 12>), g, b, lds, w->stream, d);
        else if (use_u)
            hipLaunchKernelGGL((k_tick<6, 16>), g, b, lds, w->stream, d);
        else
            hipLaunchKernelGGL(k_tick_touch, dim3((unsigned)d.n_tiles), dim3(kTPB), 0, w->stream, d);
        HIPCHK(hipGetLastError());
    }
    if (d.has_recops && d.n_rtiles) {
        TimeScope ts(w, KT_REC);
        constexpr int kWpb = kTPB / 64;  // record tiles (waves) per workgroup
        const dim3 g((unsigned)((d.n_rtiles + kWpb - 1) / kWpb)), b(kTPB);
        if (nrss)  // the SetRecord slots' events and messages, for k_records to reserve
            hipLaunchKernelGGL((k_rset_slots<false>), dim3((unsigned)((nrss + kWpb - 1) / kWpb)), b, 0, w->stream, d,
                               w->rheads);
        // (the SetRecord slots' instantiation, and the unfused one: the fast path stays lean)
        auto launch = [&](auto sets, auto fuse) {
            constexpr bool kS = decltype(sets)::value, kF = decltype(fuse)::value;
            if (d.n_rops <= 1)
                hipLaunchKernelGGL((k_records<1, 4, kS, kF>), g, b, 0, w->stream, d);
            else if (d.n_rops <= 2) {
                // two known op codes (the fast path's common shape): compiled in
                const unsigned c0 = d.rops[0].code == NFK_OP_RIADD_CLAMP ? 1u : 2u;
                const unsigned c1 = d.rops[1].code == NFK_OP_RIADD_CLAMP ? 1u : 2u;
                if (kS || !kF || d.n_rops != 2)
                    hipLaunchKernelGGL((k_records<2, 4, kS, kF>), g, b, 0, w->stream, d);
                else if (c0 == 1 && c1 == 1)
                    hipLaunchKernelGGL((k_records<2, 4, kS, kF, 5u>), g, b, 0, w->stream, d);
                else if (c0 == 1 && c1 == 2)
                    hipLaunchKernelGGL((k_records<2, 4, kS, kF, 9u>), g, b, 0, w->stream, d);
                else if (c0 == 2 && c1 == 1)
                    hipLaunchKernelGGL((k_records<2, 4, kS, kF, 6u>), g, b, 0, w->stream, d);
                else
                    hipLaunchKernelGGL((k_records<2, 4, kS, kF, 10u>), g, b, 0, w->stream, d);
            }
            else
                hipLaunchKernelGGL((k_records<NFK_MAX_REC_OPS, 2, kS, kF>), g, b, 0, w->stream, d);
        };
        using T = std::true_type;
        using F = std::false_type;
        if (nrss)
            d.fuse_rec ? launch(T{}, T{}) : launch(T{}, F{});
        else
            d.fuse_rec ? launch(F{}, T{}) : launch(F{}, F{});
        if (nrss)  // ... and written into the room k_records left
            hipLaunchKernelGGL((k_rset_slots<true>), dim3((unsigned)((nrss + kWpb - 1) / kWpb)), b, 0, w->stream, d,
                               w->rheads);
        HIPCHK(hipGetLastError());
    }
    if (nhq) {  // the post-scan entries (their count is the fold's, on the device)
        TimeScope ts(w, KT_AUX);
        hipLaunchKernelGGL(k_post_hostops, dim3((unsigned)((npost + 255) / 256)), dim3(256), 0, w->stream,
                           (const uint32_t*)hpost.slot, (const uint32_t*)hpost.kind, (const uint32_t*)hpost.op,
                           (const float*)hpost.interval, (const int32_t*)hpost.count, (const int64_t*)hpost.time,
                           (int32_t)npost, (uint8_t*)(HF + ho_ad), d, w->hf_npost);
        HIPCHK(hipGetLastError());
    }
    // Dense global ranks of the tile-staged outputs (ev_base, fi_base, totals): the frame's own
    // work needs them only when k_fanout runs after it (record tiles, unfused property tiles).
    // Otherwise the frame's outputs are complete as tiles + per-tile counts, and the ranks are
    // built on the first read (nfk_summary_get, nfk_outputs_get, nfk_read_*).
    w->scan_pending = false;
    if (d.lb_rank) {
        // (written by k_tick's rank workgroups)
    } else if (d.fuse_fan && (!d.has_recops || d.fuse_rec)) {
        w->scan_pending = true;
        w->scan_dev = d;
    } else {
        TimeScope ts(w, KT_SCAN);
        hipLaunchKernelGGL(k_scan_tiles, dim3(4), dim3(kScanTPB), 0, w->stream, d);
        HIPCHK(hipGetLastError());
    }
    // the tiles k_tick / k_records did not fan out: record tiles, and property tiles after
    // k_tick_touch
    const int fan0 = d.fuse_fan ? d.n_tiles : 0;
    const int nfan = d.n_tiles + (d.has_recops && !d.fuse_rec ? d.n_rtiles : 0) - fan0;
    if (nfan > 0 && !(d.ablate & kAblNoEmit)) {  // (timing ablation: events were not written)
        {
            TimeScope ts(w, KT_FAN);
            hipLaunchKernelGGL(k_fanout, dim3((unsigned)nfan), dim3(kTPB), 0, w->stream, d, (int32_t)fan0);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipMemcpyAsync(w->err_pin, &w->ctrl->err, sizeof(unsigned), hipMemcpyDeviceToHost, w->stream));
        HIPCHK(hipEventRecord(w->err_done, w->stream));
        w->fan_unchecked = true;
    }
    w->ticks++;
    if (trace) {
        tp[5] = clk::now();
        auto ms = [&](int a, int b) { return std::chrono::duration<double, std::milli>(tp[b] - tp[a]).count(); };
        fprintf(stderr, "nfk_execute: membership %.3f ms, SetProperty groups %.3f ms (%zu calls), schedule "
                "calls %.3f ms (%zu), upload %.3f ms, launches %.3f ms\n", ms(0, 1), ms(1, 2), n_xq, ms(2, 3),
                n_hq, ms(3, 4), ms(4, 5));
    }
    return NFK_OK;
}

int nfk_execute(void* world, int64_t now_ms) {
    World* w = (World*)world;
    if (!w) return fail(NFK_ERR_ARG, "null world");
    return execute_frame(w, now_ms, false);
}

int nfk_execute_calls(void* world) {
    // a frame at the earliest time: `now > next` holds for no schedule, so nothing fires and no
    // record is rescheduled; the queued calls run through the ordinary frame path, k_tick only on
    // the tiles their SetProperty groups touch
    World* w = (World*)world;
    if (!w) return fail(NFK_ERR_ARG, "null world");
    return execute_frame(w, INT64_MIN, true);
}

int nfk_sync(void* world) {
    World* w = (World*)world;
    if (!w) return fail(NFK_ERR_ARG, "null world");
    HIPCHK(hipStreamSynchronize(w->stream));
    return NFK_OK;
}

int nfk_get_stream(void* world, void** stream) {
    World* w = (World*)world;
    if (!w || !stream) return fail(NFK_ERR_ARG, "null argument");
    *stream = (void*)w->stream;
    return NFK_OK;
}

static int ensure_ranks(World* w) {
    if (!w->scan_pending) return NFK_OK;
    w->scan_pending = false;
    TimeScope ts(w, KT_SCAN);
    hipLaunchKernelGGL(k_scan_tiles, dim3(4), dim3(kScanTPB), 0, w->stream, w->scan_dev);
    HIPCHK(hipGetLastError());
    return NFK_OK;
}

static int read_ctrl(World* w, Ctrl* c) {
    int r = ensure_ranks(w);
    if (r) return r;
    HIPCHK(hipMemcpyAsync(w->ctrl_pin, w->ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, w->stream));
    HIPCHK(hipStreamSynchronize(w->stream));
    memcpy(c, w->ctrl_pin, sizeof(Ctrl));
    return NFK_OK;
}
// the control block and the byte tallies (read_tallies) behind the frame, one synchronisation
static int read_ctrl_tallies(World* w, Ctrl* c, uint64_t tb[3]) {
    int r = ensure_ranks(w);
    if (r) return r;
    char* tp = w->ctrl_pin + kCtrlPinTally;
    HIPCHK(hipMemcpyAsync(w->ctrl_pin, w->ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, w->stream));
    HIPCHK(hipMemcpyAsync(tp, w->d.tally, kTallyBytes, hipMemcpyDeviceToHost, w->stream));
    HIPCHK(hipStreamSynchronize(w->stream));
    memcpy(c, w->ctrl_pin, sizeof(Ctrl));
    const unsigned long long* t = (const unsigned long long*)tp;
    for (int k = 0; k < 3; k++) {
        tb[k] = 0;
        for (int i = 0; i < kTallyN; i++) tb[k] += t[((size_t)k * kTallyN + i) * 8];
    }
    return NFK_OK;
}

// entries of msg_rcpt reserved by the fixed-stride tiles of the last frame (property tiles, and
// record tiles when k_records fanned them out)
static int64_t fixed_msgs_reserved(const World* w) {
    return (int64_t)w->last_tcap * w->d.n_tiles + (int64_t)w->last_rtcap * (w->d.has_recops ? w->d.n_rtiles : 0);
}

// messages of the last frame: the runs are dense unless k_tick placed property tiles at a stride
static int64_t frame_msgs(const World* w, const Ctrl& c) {
    if (!w->last_tcap) return (int64_t)c.msg_extent;
    return (int64_t)c.n_msgs_ptiles + (int64_t)c.msg_extent - fixed_msgs_reserved(w);
}

// The last frame's k_fanout found msg_rcpt too small: it wrote nothing (it checks the scanned
// extent first) and only reads the event tiles and the membership CSR, so grow the message buffer
// (keeping what k_tick's / k_records' own fan-out wrote) and re-run it for that frame.
static int regrow_fanout(World* w, Ctrl& c) {
    const int64_t extent = (int64_t)c.msg_extent;
    const int64_t need = extent + extent / 4 + 1024;
    if (need > 0xFFFFFFFFll) return fail(NFK_ERR_CAPACITY, "fan-out exceeds 2^32 messages per frame");
    uint32_t* grown = nullptr;
    int r = alloc_track(w, (void**)&grown, (size_t)need * 4);
    if (r) return r;
    if (w->last_tcap)
        HIPCHK(hipMemcpy(grown, w->d.msg_rcpt, (size_t)fixed_msgs_reserved(w) * 4, hipMemcpyDeviceToDevice));
    HIPCHK(hipFree(w->d.msg_rcpt));
    w->allocs.erase(std::remove(w->allocs.begin(), w->allocs.end(), (void*)w->d.msg_rcpt), w->allocs.end());
    w->d.msg_rcpt = grown;
    w->d.msg_cap = need;
    HIPCHK(hipMemset(&w->ctrl->err, 0, sizeof(unsigned)));
    Dev d = w->d;
    const int fan0 = w->last_tcap ? d.n_tiles : 0;
    const int nfan = d.n_tiles + (d.has_recops && !w->last_rtcap ? d.n_rtiles : 0) - fan0;
    if (nfan > 0) hipLaunchKernelGGL(k_fanout, dim3((unsigned)nfan), dim3(kTPB), 0, w->stream, d, (int32_t)fan0);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(w->stream));
    HIPCHK(hipMemcpy(&c, w->ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost));
    return NFK_OK;
}

// Before anything reads or replaces the last frame's fan-out: if its k_fanout overflowed the
// message buffer, recover that frame now (whether or not nfk_summary_get was called).
static int check_fanout(World* w) {
    if (!w->fan_unchecked) return NFK_OK;
    HIPCHK(hipEventSynchronize(w->err_done));
    w->fan_unchecked = false;
    if (!(*w->err_pin & kErrMsgCap)) return NFK_OK;
    Ctrl c;
    int r = read_ctrl(w, &c);
    if (r) return r;
    if (c.err & ~kErrMsgCap) return NFK_OK;  // (another device error: reported by nfk_summary_get)
    return regrow_fanout(w, c);
}

int nfk_summary_get(void* world, nfk_summary* out) {
    World* w = (World*)world;
    if (!w || !out) return fail(NFK_ERR_ARG, "null argument");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    Ctrl c;
    uint64_t tb[3];
    {
        int r = check_fanout(w);
        if (r) return r;
    }
    {
        int r = read_ctrl_tallies(w, &c, tb);
        if (r) return r;
    }
    memset(out, 0, sizeof *out);
    {
        int64_t live = 0;
        for (const auto& g : w->segs) live += (int64_t)g.objs.size();
        out->n_entities = live;
    }
    out->n_prop_events = (int64_t)c.n_ev;
    out->n_rec_events = (int64_t)c.n_re;
    out->n_fired = (int64_t)c.n_fi;
    out->n_msgs = frame_msgs(w, c);
    {
        out->alg_bytes_tick = (int64_t)(tb[0] - w->last_bytes[0]);
        out->alg_bytes_rec = (int64_t)(tb[1] - w->last_bytes[1]);
        out->alg_bytes_fan = (int64_t)(tb[2] - w->last_bytes[2]);
        for (int k = 0; k < 3; k++) w->last_bytes[k] = tb[k];
    }
    if ((c.err & kErrMsgCap) && !(c.err & ~kErrMsgCap)) {
        int r = regrow_fanout(w, c);
        if (r) return r;
    }
    w->last_rec_msgs = frame_msgs(w, c) - (int64_t)c.n_msgs_ptiles;
    out->device_error = (int32_t)c.err;
    out->tick = w->ticks;
    if (c.err) HIPCHK(hipMemset(&w->ctrl->err, 0, sizeof(unsigned)));
    clear_err_host(w);  // (the stream is idle: read_ctrl synchronised it)
    if (c.err & kErrTouch) return fail(NFK_ERR_TOUCH, "device touch list overflow");
    if (c.err & kErrFanBound) return fail(NFK_ERR_STATE, "a tile's fan-out exceeded its bound");
    if (c.err & kErrRemain) return fail(NFK_ERR_STATE, "k_tick read a fired heartbeat's remain it never wrote");
    if (c.err & kErrRankWait) return fail(NFK_ERR_DEVICE, "k_tick's rank workgroups gave up waiting for a tile's counts: the frame has no ranks");
    if (c.err & kErrMsgCap)
        return fail(NFK_ERR_CAPACITY, "device output capacity exceeded (err=" + std::to_string(c.err) + ")");
    return NFK_OK;
}

int nfk_outputs_get(void* world, nfk_outputs* o) {
    World* w = (World*)world;
    if (!w || !o) return fail(NFK_ERR_ARG, "null argument");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    int r = check_fanout(w);  // (synchronises only after a frame that ran k_fanout)
    if (r) return r;
    // a device error of a frame that has completed (host-mapped word, no device read); a frame
    // still running reports through the next call that waits for it (nfk_execute, nfk_summary_get)
    if (const unsigned e = err_host_bits(w); e & (kErrFanBound | kErrTouch | kErrRankWait))
        return fail(NFK_ERR_DEVICE, (e & kErrFanBound) ? "a tile's fan-out exceeded its bound: the recipient lists are truncated"
                                    : (e & kErrTouch)  ? "touch list overflow: events are missing"
                                                       : "k_tick's rank workgroups gave up waiting: the frame has no ranks");
    r = ensure_ranks(w);  // (asynchronous, on the world's stream like the frame)
    if (r) return r;
    const Dev& d = w->d;
    o->n_tiles = d.n_tiles; o->tile_slots = kTile;
    o->n_rtiles = d.has_recops ? d.n_rtiles : 0; o->rtile_slots = kRTile;
    o->ev_tile_cap = d.ev_tcap; o->fi_tile_cap = d.fi_tcap; o->re_tile_cap = d.re_tcap;
    o->ev_base = d.ev_base; o->fi_base = d.fi_base; o->re_base = d.re_base; o->msg_base = d.msg_base;
    o->msg_cnt = d.t_msg;
    o->ev_slot = d.ev_slot; o->ev_pid = d.ev_pid; o->ev_old = d.ev_old; o->ev_new = d.ev_new;
    o->ev_moff = w->last_tcap ? nullptr : d.ev_moff;  // (tiles k_tick fanned out store none: nfgpu.h)
    o->re_slot = nullptr;  // (a record event's slot is in its word: nfgpu.h)
    o->re_rrc = d.re_rrc; o->re_old = d.re_old; o->re_new = d.re_new;
    o->re_moff = w->last_rtcap ? nullptr : d.re_moff;  // (fused record tiles store none: nfgpu.h)
    o->fi_slot = d.fi_slot; o->fi_kind = d.fi_kind; o->fi_remain = d.fi_remain;
    o->msg_rcpt = d.msg_rcpt;
    o->slot_obj = w->slot_obj_d;
    o->ev_old_h = d.ev_old_h;
    o->ev_new_h = d.ev_new_h;
    o->re_old_h = w->re_old_h;
    o->re_new_h = w->re_new_h;
    return NFK_OK;
}

int nfk_read_object(void* world, int32_t pid, int64_t* head, int64_t* data) {
    World* w = (World*)world;
    if (!w || !head || !data || pid < w->n_if || pid >= w->n_prop) return fail(NFK_ERR_ARG, "bad argument");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    HIPCHK(hipStreamSynchronize(w->stream));
    const Dev& d = w->d;
    std::vector<uint64_t> col(2 * (size_t)std::max(d.N, 1));
    if (d.N) HIPCHK(hipMemcpy(col.data(), d.pmem + w->tab.p_off[pid], (size_t)d.N * 16, hipMemcpyDeviceToHost));
    memset(head, 0, (size_t)w->n_obj * 8);  // objects no longer in this world read the null NFGUID
    memset(data, 0, (size_t)w->n_obj * 8);
    for (int32_t s = 0; s < d.N; s++)
        if (w->obj_of_slot[s] >= 0) {
            data[w->obj_of_slot[s]] = (int64_t)col[2 * (size_t)s];
            head[w->obj_of_slot[s]] = (int64_t)col[2 * (size_t)s + 1];
        }
    return NFK_OK;
}

int nfk_read_prop(void* world, int32_t pid, uint64_t* bits) {
    World* w = (World*)world;
    if (!w || !bits || pid < 0 || pid >= w->n_if) return fail(NFK_ERR_ARG, "bad argument (object properties: nfk_read_object)");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    HIPCHK(hipStreamSynchronize(w->stream));
    const Dev& d = w->d;
    std::vector<uint64_t> col(std::max(d.N, 1));
    if (d.N)
        HIPCHK(hipMemcpy2D(col.data(), 8, d.pmem + w->tab.p_off[pid], (size_t)w->tab.p_str[pid] * 8, 8, (size_t)d.N,
                           hipMemcpyDeviceToHost));
    memset(bits, 0, (size_t)w->n_obj * 8);  // objects no longer in this world read 0
    for (int32_t s = 0; s < d.N; s++)
        if (w->obj_of_slot[s] >= 0) bits[w->obj_of_slot[s]] = col[s];
    return NFK_OK;
}

int nfk_read_record(void* world, int32_t rec, uint64_t* cells) {
    World* w = (World*)world;
    if (!w || !cells || rec < 0 || rec >= w->cfg.n_rec) return fail(NFK_ERR_ARG, "bad argument");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    HIPCHK(hipStreamSynchronize(w->stream));
    const Dev& d = w->d;
    const int rows = w->tab.rec_rows[rec], cols = w->tab.rec_cols[rec];
    const uint64_t rowm = rec_rowm(rows);
    size_t per = (size_t)rows * cols;
    std::vector<uint64_t> buf(per * d.N), used(d.N);
    HIPCHK(hipMemcpy(buf.data(), d.rcells[rec], buf.size() * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(used.data(), d.rused[rec], used.size() * 8, hipMemcpyDeviceToHost));
    memset(cells, 0, (size_t)w->n_obj * per * 8);
    for (int32_t s = 0; s < d.N; s++) {
        if (w->obj_of_slot[s] < 0) continue;
        uint64_t* dst = cells + (size_t)w->obj_of_slot[s] * per;  // row order (from packed, rec_pos)
        const uint64_t* src = &buf[(size_t)s * per];
        for (int c = 0; c < cols; c++)
            for (int q = 0; q < rows; q++) dst[(size_t)c * rows + q] = src[(size_t)c * rows + rec_pos(used[s], rowm, q)];
    }
    return NFK_OK;
}

// the hot records [n_kind][n_objects] decoded from the schedule words, and which of them are wide
static int read_schedules(World* w, int64_t* next_ms, int32_t* remain, uint8_t* state, uint8_t* wide) {
    HIPCHK(hipStreamSynchronize(w->stream));
    const Dev& d = w->d;
    const int NK = d.n_kind;
    std::vector<uint64_t> word((size_t)NK * d.s_wstr);
    std::vector<SchedHot> hot((size_t)NK * d.s_kstr);
    if (NK) HIPCHK(hipMemcpy(word.data(), d.s_word, word.size() * 8, hipMemcpyDeviceToHost));
    if (NK) HIPCHK(hipMemcpy(hot.data(), d.s_wide, hot.size() * sizeof(SchedHot), hipMemcpyDeviceToHost));
    for (int k = 0; k < NK; k++)
        for (int32_t s = 0; s < d.N; s++) {
            if (w->obj_of_slot[s] < 0) continue;
            const size_t o = (size_t)k * w->n_obj + w->obj_of_slot[s];
            const uint64_t x = word[(size_t)k * d.s_wstr + s];
            if (!(x & kStPresent)) continue;
            const SchedHot h = (x & kScWide) ? hot[(size_t)k * d.s_kstr + s] : sc_decode(x, d.s_epoch, d.s_step[k]);
            if (state) {
                state[o] = (uint8_t)(h.state & (kStPresent | kStForever));
                next_ms[o] = h.next;
                remain[o] = h.remain;
            }
            if (wide) wide[o] = (x & kScWide) ? 1 : 0;
        }
    return NFK_OK;
}

int nfk_read_schedules(void* world, int64_t* next_ms, int32_t* remain, uint8_t* state) {
    World* w = (World*)world;
    if (!w || !next_ms || !remain || !state) return fail(NFK_ERR_ARG, "null argument");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    const size_t n = (size_t)w->d.n_kind * w->n_obj;
    memset(state, 0, n);
    memset(next_ms, 0, n * 8);
    memset(remain, 0, n * 4);
    return read_schedules(w, next_ms, remain, state, nullptr);
}

int nfk_read_schedule_forms(void* world, uint8_t* wide) {
    World* w = (World*)world;
    if (!w || !wide) return fail(NFK_ERR_ARG, "null argument");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    memset(wide, 0, (size_t)w->d.n_kind * w->n_obj);
    return read_schedules(w, nullptr, nullptr, nullptr, wide);
}

int nfk_read_events(void* world, int32_t* ev_obj, int32_t* ev_pid, uint64_t* ev_old, uint64_t* ev_new) {
    World* w = (World*)world;
    if (!w) return fail(NFK_ERR_ARG, "null world");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    Ctrl c;
    int r = read_ctrl(w, &c);
    if (r) return r;
    const Dev& d = w->d;
    const size_t n = c.n_ev;
    std::vector<uint32_t> sl(n);
    GATHER(w, d.ev_slot, d.ev_base, d.n_tiles, d.ev_tcap, n, sl.data());
    GATHER(w, d.ev_pid, d.ev_base, d.n_tiles, d.ev_tcap, n, (uint32_t*)ev_pid);
    GATHER(w, d.ev_old, d.ev_base, d.n_tiles, d.ev_tcap, n, ev_old);
    GATHER(w, d.ev_new, d.ev_base, d.n_tiles, d.ev_tcap, n, ev_new);
    for (size_t i = 0; i < n; i++) ev_obj[i] = w->obj_of_slot[sl[i]];
    return NFK_OK;
}

// whether a record event word in the host format (op << 24 | rec << 16 | row << 8 | col; rrc_host
// of a raw word) is the Update of an object cell: the events whose head halves the device writes
static bool rrc_obj_update(const World* w, uint32_t rrc) {
    return (rrc >> 24) == 0 && w->rec_ctype[(rrc >> 16) & 0xFF][rrc & 0xFF] == NFK_REC_OBJ_DATA;
}

int nfk_read_events_obj(void* world, uint64_t* ev_old_h, uint64_t* ev_new_h) {
    World* w = (World*)world;
    if (!w) return fail(NFK_ERR_ARG, "null world");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    Ctrl c;
    int r = read_ctrl(w, &c);
    if (r) return r;
    const Dev& d = w->d;
    const size_t n = c.n_ev;
    if (!d.n_obj) {
        memset(ev_old_h, 0, n * 8);
        memset(ev_new_h, 0, n * 8);
        return NFK_OK;
    }
    std::vector<uint32_t> pid(n);
    GATHER(w, d.ev_pid, d.ev_base, d.n_tiles, d.ev_tcap, n, pid.data());
    GATHER(w, d.ev_old_h, d.ev_base, d.n_tiles, d.ev_tcap, n, ev_old_h);
    GATHER(w, d.ev_new_h, d.ev_base, d.n_tiles, d.ev_tcap, n, ev_new_h);
    for (size_t i = 0; i < n; i++)
        if ((int)pid[i] < d.n_if) ev_old_h[i] = ev_new_h[i] = 0;  // (unwritten for other events)
    return NFK_OK;
}

int nfk_read_rec_events(void* world, int32_t* re_obj, uint32_t* re_rrc, uint64_t* re_old, uint64_t* re_new) {
    World* w = (World*)world;
    if (!w) return fail(NFK_ERR_ARG, "null world");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    Ctrl c;
    int r = read_ctrl(w, &c);
    if (r) return r;
    const Dev& d = w->d;
    const size_t n = c.n_re;
    GATHER(w, d.re_rrc, d.re_base, d.n_rtiles, d.re_tcap, n, re_rrc);
    GATHER(w, d.re_old, d.re_base, d.n_rtiles, d.re_tcap, n, re_old);
    GATHER(w, d.re_new, d.re_base, d.n_rtiles, d.re_tcap, n, re_new);
    // each event's slot: its record tile's first slot + the slot field of its word (kRrcHost)
    std::vector<uint32_t> rb((size_t)d.n_rtiles + 1, 0);
    if (n) HIPCHK(hipMemcpy(rb.data(), d.re_base, rb.size() * 4, hipMemcpyDeviceToHost));
    for (int t = 0; t < d.n_rtiles; t++)
        for (uint32_t i = rb[(size_t)t]; i < rb[(size_t)t + 1] && i < n; i++) {
            re_obj[i] = w->obj_of_slot[(size_t)t * kRTile + (re_rrc[i] >> kRrcSitShift)];
            re_rrc[i] = rrc_host(re_rrc[i]);
        }
    return NFK_OK;
}

int nfk_read_rec_events_obj(void* world, uint64_t* re_old_h, uint64_t* re_new_h) {
    World* w = (World*)world;
    if (!w) return fail(NFK_ERR_ARG, "null world");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    Ctrl c;
    int r = read_ctrl(w, &c);
    if (r) return r;
    const Dev& d = w->d;
    const size_t n = c.n_re;
    if (!w->rec_obj) {
        memset(re_old_h, 0, n * 8);
        memset(re_new_h, 0, n * 8);
        return NFK_OK;
    }
    std::vector<uint32_t> rrc(n);
    GATHER(w, d.re_rrc, d.re_base, d.n_rtiles, d.re_tcap, n, rrc.data());
    GATHER(w, w->re_old_h, d.re_base, d.n_rtiles, d.re_tcap, n, re_old_h);
    GATHER(w, w->re_new_h, d.re_base, d.n_rtiles, d.re_tcap, n, re_new_h);
    for (size_t i = 0; i < n; i++)  // (unwritten but for the Updates of object cells)
        if (!rrc_obj_update(w, rrc_host(rrc[i]))) re_old_h[i] = re_new_h[i] = 0;
    return NFK_OK;
}

int nfk_read_fired(void* world, int32_t* fi_obj, int32_t* fi_kind, int32_t* fi_remain) {
    World* w = (World*)world;
    if (!w) return fail(NFK_ERR_ARG, "null world");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    Ctrl c;
    int r = read_ctrl(w, &c);
    if (r) return r;
    const Dev& d = w->d;
    const size_t n = c.n_fi;
    std::vector<uint32_t> sl(n);
    GATHER(w, d.fi_slot, d.fi_base, d.n_tiles, d.fi_tcap, n, sl.data());
    GATHER(w, d.fi_kind, d.fi_base, d.n_tiles, d.fi_tcap, n, (uint32_t*)fi_kind);
    GATHER(w, d.fi_remain, d.fi_base, d.n_tiles, d.fi_tcap, n, fi_remain);
    for (size_t i = 0; i < n; i++) fi_obj[i] = w->obj_of_slot[sl[i]];
    return NFK_OK;
}

int nfk_read_fanout(void* world, uint32_t* msg_off, int32_t* msg_rcpt_obj) {
    World* w = (World*)world;
    if (!w) return fail(NFK_ERR_ARG, "null world");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    Ctrl c;
    int r = check_fanout(w);
    if (r) return r;
    r = read_ctrl(w, &c);
    if (r) return r;
    if (c.msg_extent > (unsigned long long)w->d.msg_cap) return fail(NFK_ERR_CAPACITY, "fan-out not recovered");
    const Dev& d = w->d;
    const size_t nm = (size_t)frame_msgs(w, c);
    // each tile's messages are one run at msg_base[tile]; the dense CSR walks tiles in order
    const int ntt = d.n_tiles + (d.has_recops ? d.n_rtiles : 0);
    std::vector<uint32_t> mb(ntt), mc(ntt), eb(d.n_tiles + 1), rb(d.n_rtiles + 1);
    std::vector<uint64_t> db(ntt);
    if (ntt) {
        HIPCHK(hipMemcpy(mb.data(), d.msg_base, (size_t)ntt * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(mc.data(), d.t_msg, (size_t)ntt * 4, hipMemcpyDeviceToHost));
    }
    HIPCHK(hipMemcpy(eb.data(), d.ev_base, eb.size() * 4, hipMemcpyDeviceToHost));
    if (d.has_recops) HIPCHK(hipMemcpy(rb.data(), d.re_base, rb.size() * 4, hipMemcpyDeviceToHost));
    uint64_t acc = 0;
    for (int t = 0; t < ntt; t++) {
        db[t] = acc;
        acc += mc[t];
    }
    if (acc != nm) return fail(NFK_ERR_STATE, "message cursor and tile counts disagree");
    // (tiles k_tick / k_records fanned out themselves store no offsets: counted on the device below)
    const bool ev_counted = w->last_tcap != 0, rec_counted = d.has_recops && w->last_rtcap;
    if (!ev_counted) GATHER(w, d.ev_moff, d.ev_base, d.n_tiles, d.ev_tcap, (size_t)c.n_ev, msg_off);
    if (d.has_recops && !rec_counted)
        GATHER(w, d.re_moff, d.re_base, d.n_rtiles, d.re_tcap, (size_t)c.n_re, msg_off + c.n_ev);
    if (!ev_counted)
        for (int t = 0; t < d.n_tiles; t++)
            for (uint32_t i = eb[t]; i < eb[t + 1]; i++) msg_off[i] = (uint32_t)(msg_off[i] - mb[t] + db[t]);
    if (d.has_recops && !rec_counted)
        for (int t = 0; t < d.n_rtiles; t++)
            for (uint32_t i = rb[t]; i < rb[t + 1]; i++) {
                const int tg = d.n_tiles + t;
                msg_off[c.n_ev + i] = (uint32_t)(msg_off[c.n_ev + i] - mb[tg] + db[tg]);
            }
    const size_t ncnt = (ev_counted ? (size_t)c.n_ev : 0) + (rec_counted ? (size_t)c.n_re : 0);
    if (ncnt) {  // counted on the device (k_counted_moff) from the dense bases
        std::vector<uint32_t> dbv(ntt);
        for (int t = 0; t < ntt; t++) dbv[t] = (uint32_t)db[t];
        // (a world-owned scratch, grown as needed: no allocation per call, nothing to free on errors)
        r = dev_reserve(w, (void**)&w->moff_tmp, &w->moff_tmp_cap, ((size_t)ntt + (size_t)c.n_ev + (size_t)c.n_re) * 4);
        if (r) return r;
        uint32_t* const tmp = w->moff_tmp;
        HIPCHK(hipMemcpy(tmp, dbv.data(), (size_t)ntt * 4, hipMemcpyHostToDevice));
        uint32_t* out = tmp + ntt;  // [n_ev ++ n_re], as msg_off
        hipError_t ce = hipSuccess;
        if (ev_counted && c.n_ev) {
            const unsigned g = (unsigned)std::max(1, std::min(d.n_tiles, 4096));
            hipLaunchKernelGGL(k_counted_moff, dim3(g), dim3(kTPB), 0, w->stream, d, 0, out, (const uint32_t*)tmp);
            ce = hipGetLastError();
            if (ce == hipSuccess)
                ce = hipMemcpyAsync(msg_off, out, (size_t)c.n_ev * 4, hipMemcpyDeviceToHost, w->stream);
        }
        if (ce == hipSuccess && rec_counted && c.n_re) {
            const unsigned g = (unsigned)std::max(1, std::min(d.n_rtiles, 4096));
            hipLaunchKernelGGL(k_counted_moff, dim3(g), dim3(kTPB), 0, w->stream, d, 1, out + c.n_ev, (const uint32_t*)tmp);
            ce = hipGetLastError();
            if (ce == hipSuccess)
                ce = hipMemcpyAsync(msg_off + c.n_ev, out + c.n_ev, (size_t)c.n_re * 4, hipMemcpyDeviceToHost, w->stream);
        }
        if (ce == hipSuccess) ce = hipStreamSynchronize(w->stream);
        if (ce != hipSuccess) return fail(NFK_ERR_HIP, std::string("k_counted_moff: ") + hipGetErrorString(ce));
    }
    msg_off[c.n_ev + c.n_re] = (uint32_t)nm;
    // the runs cover [0, extent) with gaps when property tiles sit at a stride
    const size_t ext = (size_t)c.msg_extent;
    std::vector<uint32_t> rc(ext);
    if (ext) HIPCHK(hipMemcpy(rc.data(), d.msg_rcpt, ext * 4, hipMemcpyDeviceToHost));
    for (int t = 0; t < ntt; t++)
        for (uint32_t i = 0; i < mc[t]; i++) msg_rcpt_obj[db[t] + i] = w->obj_of_slot[rc[(size_t)mb[t] + i]];
    return NFK_OK;
}

// The rank of every object's NFGUID among all objects of the world (rank_d, on the device), for
// ordering the fired list as mObjectScheduleMap does: the sorted order is kept and new objects are
// merged into it (an O(n) merge in frames that created objects).
static int update_guid_ranks(World* w) {
    if (w->rank_n == w->n_obj && w->rank_d) return NFK_OK;
    std::vector<int32_t> fresh(w->n_obj - w->rank_n);
    std::iota(fresh.begin(), fresh.end(), w->rank_n);
    auto less = [w](int32_t a, int32_t b) { return guid_less(w, a, b); };
    std::sort(fresh.begin(), fresh.end(), less);
    std::vector<int32_t> merged(w->n_obj);
    std::merge(w->guid_sorted.begin(), w->guid_sorted.end(), fresh.begin(), fresh.end(), merged.begin(), less);
    w->guid_sorted.swap(merged);
    std::vector<int32_t> rank(w->n_obj);
    for (int32_t i = 0; i < w->n_obj; i++) rank[w->guid_sorted[i]] = i;
    if ((size_t)w->n_obj > w->rank_cap) {
        HIPCHK(hipStreamSynchronize(w->stream));
        if (w->rank_d) HIPCHK(hipFree(w->rank_d));
        w->rank_d = nullptr;
        w->rank_cap = (size_t)w->n_obj + w->n_obj / 4 + 1024;
        HIPCHK(hipMalloc((void**)&w->rank_d, w->rank_cap * 4));
    }
    HIPCHK(hipMemcpy(w->rank_d, rank.data(), rank.size() * 4, hipMemcpyHostToDevice));
    w->rank_n = w->n_obj;
    return NFK_OK;
}

int nfk_read_frame(void* world, uint32_t what, nfk_frame_host* o) {
    World* w = (World*)world;
    if (!w || !o) return fail(NFK_ERR_ARG, "null argument");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    memset(o, 0, sizeof *o);
    int r = check_fanout(w);
    if (r) return r;
    Ctrl c;
    r = read_ctrl(w, &c);
    if (r) return r;
    if (c.err & (kErrFanBound | kErrTouch | kErrRankWait))
        return fail(NFK_ERR_DEVICE, "the frame's outputs are incomplete (device error " + std::to_string(c.err) + ")");
    if (c.msg_extent > (unsigned long long)w->d.msg_cap) return fail(NFK_ERR_CAPACITY, "fan-out not recovered");
    const Dev& d = w->d;
    const bool fired = what & NFK_READ_FIRED, order = fired && (what & NFK_READ_FIRED_GUID_ORDER);
    const bool events = what & NFK_READ_EVENTS, fan = events && (what & NFK_READ_FANOUT);
    const bool heads = events && d.n_obj > 0;
    const size_t ne = events ? c.n_ev : 0, nr = events && d.has_recops ? c.n_re : 0, nf = fired ? c.n_fi : 0;
    const size_t nm = fan ? (size_t)frame_msgs(w, c) : 0;
    const int ntt = d.n_tiles + (d.has_recops ? d.n_rtiles : 0);
    // one region, the same layout on the device and in pinned host memory
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t a = at;
        at += (bytes + 255) & ~(size_t)255;
        return a;
    };
    const size_t o_eo = take(ne * 4), o_ep = take(ne * 4), o_eold = take(ne * 8), o_enew = take(ne * 8);
    const size_t o_eoh = take(heads ? ne * 8 : 0), o_enh = take(heads ? ne * 8 : 0);
    const size_t o_ro = take(nr * 4), o_rr = take(nr * 4), o_rold = take(nr * 8), o_rnew = take(nr * 8);
    const bool rheads = events && w->rec_obj;  // (the object cells' head halves)
    const size_t o_roh = take(rheads ? nr * 8 : 0), o_rnh = take(rheads ? nr * 8 : 0);
    const size_t o_fo = take(nf * 4), o_fk = take(nf * 4), o_fr = take(nf * 4);
    const size_t o_mo = take(fan ? (ne + nr + 1) * 4 : 0), o_mr = take(nm * 4);
    const size_t total = at;
    // device scratch: dense message bases, and the fired sort's keys / indices / unsorted copies
    const size_t s_db = 0, s_keys = (((size_t)ntt + 1) * 4 + 255) & ~(size_t)255;
    const size_t s_k2 = s_keys + ((nf * 8 + 255) & ~(size_t)255), s_i1 = s_k2 + ((nf * 8 + 255) & ~(size_t)255);
    const size_t s_i2 = s_i1 + ((nf * 4 + 255) & ~(size_t)255), s_f = s_i2 + ((nf * 4 + 255) & ~(size_t)255);
    size_t s_tmp = s_f + 3 * ((nf * 4 + 255) & ~(size_t)255);
    size_t sort_bytes = 0;
    int key_bits = 5;
    if (order) {
        r = update_guid_ranks(w);
        if (r) return r;
        while ((1ll << (key_bits - 5)) < (long long)std::max(w->n_obj, 1)) key_bits++;
        HIPCHK(rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr,
                                         (uint32_t*)nullptr, (uint32_t*)nullptr, nf, 0, key_bits, w->stream));
    }
    const size_t scratch = s_tmp + sort_bytes + 256;
    if (total > w->fr_cap || scratch > w->fr_scap) {
        HIPCHK(hipStreamSynchronize(w->stream));
        if (total > w->fr_cap) {
            if (w->fr_dev) HIPCHK(hipFree(w->fr_dev));
            if (w->fr_pin) HIPCHK(hipHostFree(w->fr_pin));
            w->fr_dev = nullptr;
            w->fr_pin = nullptr;
            w->fr_cap = total + total / 4 + 4096;
            HIPCHK(hipMalloc(&w->fr_dev, w->fr_cap));
            HIPCHK(hipHostMalloc((void**)&w->fr_pin, w->fr_cap, hipHostMallocDefault));
        }
        if (scratch > w->fr_scap) {
            if (w->fr_scr) HIPCHK(hipFree(w->fr_scr));
            w->fr_scr = nullptr;
            w->fr_scap = scratch + scratch / 4 + 4096;
            HIPCHK(hipMalloc(&w->fr_scr, w->fr_scap));
        }
    }
    char* D = (char*)w->fr_dev;
    char* S = (char*)w->fr_scr;
    const unsigned gt = (unsigned)std::max(1, std::min(d.n_tiles, 4096));
    const unsigned grt = (unsigned)std::max(1, std::min(d.n_rtiles, 4096));
    const int32_t* so = w->slot_obj_d;
    // the fired list's destination: dense, or the sort's unsorted copies
    int32_t* const fo = (int32_t*)(order ? S + s_f : D + o_fo);
    int32_t* const fk = (int32_t*)(order ? S + s_f + ((nf * 4 + 255) & ~(size_t)255) : D + o_fk);
    int32_t* const fr = (int32_t*)(order ? S + s_f + 2 * ((nf * 4 + 255) & ~(size_t)255) : D + o_fr);
    // events and fired list of the property tiles in one launch (k_compact_frame)
    if (ne || nf)
        hipLaunchKernelGGL(k_compact_frame, dim3(gt), dim3(kTPB), 0, w->stream, d, so,
                           ne ? (int32_t*)(D + o_eo) : nullptr, (uint32_t*)(D + o_ep), (uint64_t*)(D + o_eold),
                           (uint64_t*)(D + o_enew), nf ? fo : nullptr, (uint32_t*)fk, fr);
    if (ne) {
        if (heads) {
            hipLaunchKernelGGL(k_compact_h, dim3(gt), dim3(kTPB), 0, w->stream, d.ev_old_h, (uint64_t*)(D + o_eoh),
                               d.ev_pid, d.ev_base, d.n_tiles, d.ev_tcap, d.n_if);
            hipLaunchKernelGGL(k_compact_h, dim3(gt), dim3(kTPB), 0, w->stream, d.ev_new_h, (uint64_t*)(D + o_enh),
                               d.ev_pid, d.ev_base, d.n_tiles, d.ev_tcap, d.n_if);
        }
    }
    if (nr) {
        hipLaunchKernelGGL(k_compact_rec, dim3(grt), dim3(kTPB), 0, w->stream, d.re_rrc, (int32_t*)(D + o_ro),
                           (uint32_t*)(D + o_rr), d.re_base, d.n_rtiles, d.re_tcap, so);
        hipLaunchKernelGGL(k_compact<uint64_t>, dim3(grt), dim3(kTPB), 0, w->stream, d.re_old, (uint64_t*)(D + o_rold),
                           d.re_base, d.n_rtiles, d.re_tcap);
        hipLaunchKernelGGL(k_compact<uint64_t>, dim3(grt), dim3(kTPB), 0, w->stream, d.re_new, (uint64_t*)(D + o_rnew),
                           d.re_base, d.n_rtiles, d.re_tcap);
        if (rheads) {
            hipLaunchKernelGGL(k_compact<uint64_t>, dim3(grt), dim3(kTPB), 0, w->stream, w->re_old_h,
                               (uint64_t*)(D + o_roh), d.re_base, d.n_rtiles, d.re_tcap);
            hipLaunchKernelGGL(k_compact<uint64_t>, dim3(grt), dim3(kTPB), 0, w->stream, w->re_new_h,
                               (uint64_t*)(D + o_rnh), d.re_base, d.n_rtiles, d.re_tcap);
        }
    }
    if (fan && ntt && nm == 0) {
        // (a frame without messages, e.g. Tutorial3's private World Sets: every offset is 0)
        HIPCHK(hipMemsetAsync(D + o_mo, 0, (ne + nr + 1) * 4, w->stream));
    } else if (fan && ntt) {
        uint32_t* db = (uint32_t*)(S + s_db);
        hipLaunchKernelGGL(k_scan_counts, dim3(1), dim3(1024), 0, w->stream, d.t_msg, db, ntt);
        // (tiles k_tick / k_records fanned out themselves store no offsets: counted here)
        if (ne && w->last_tcap)
            hipLaunchKernelGGL(k_counted_moff, dim3(gt), dim3(kTPB), 0, w->stream, d, 0, (uint32_t*)(D + o_mo), db);
        else if (ne)
            hipLaunchKernelGGL(k_compact_moff, dim3(gt), dim3(kTPB), 0, w->stream, d.ev_moff, (uint32_t*)(D + o_mo),
                               d.ev_base, d.n_tiles, d.ev_tcap, d.msg_base, db);
        if (nr && w->last_rtcap)
            hipLaunchKernelGGL(k_counted_moff, dim3(grt), dim3(kTPB), 0, w->stream, d, 1, (uint32_t*)(D + o_mo) + ne, db);
        else if (nr)
            hipLaunchKernelGGL(k_compact_moff, dim3(grt), dim3(kTPB), 0, w->stream, d.re_moff,
                               (uint32_t*)(D + o_mo) + ne, d.re_base, d.n_rtiles, d.re_tcap, d.msg_base + d.n_tiles,
                               db + d.n_tiles);
        // the CSR's last offset: the frame's message count
        HIPCHK(hipMemcpyAsync(D + o_mo + (ne + nr) * 4, db + ntt, 4, hipMemcpyDeviceToDevice, w->stream));
        if (nm)
            hipLaunchKernelGGL(k_runs_obj, dim3((unsigned)std::min(ntt, 8192)), dim3(kTPB), 0, w->stream, d.msg_rcpt,
                               (int32_t*)(D + o_mr), d.msg_base, d.t_msg, db, ntt, so);
    } else if (fan) {
        HIPCHK(hipMemsetAsync(D + o_mo, 0, 4, w->stream));
    }
    if (nf) {
        if (order && nf <= (size_t)kSmallSort) {
            hipLaunchKernelGGL(k_fired_small, dim3((unsigned)((nf + kTPB - 1) / kTPB)), dim3(kTPB), 0, w->stream, (const int32_t*)fo,
                               (const int32_t*)fk, (const int32_t*)fr, w->rank_d, (int32_t*)(D + o_fo),
                               (int32_t*)(D + o_fk), (int32_t*)(D + o_fr), (int)nf);
        } else if (order) {
            const unsigned g = (unsigned)((nf + kTPB - 1) / kTPB);
            uint64_t* k1 = (uint64_t*)(S + s_keys);
            uint64_t* k2 = (uint64_t*)(S + s_k2);
            uint32_t* i1 = (uint32_t*)(S + s_i1);
            uint32_t* i2 = (uint32_t*)(S + s_i2);
            hipLaunchKernelGGL(k_fired_keys, dim3(g), dim3(kTPB), 0, w->stream, fo, fk, w->rank_d, k1, i1, (int)nf);
            size_t sb = sort_bytes;
            HIPCHK(rocprim::radix_sort_pairs(S + s_tmp, sb, k1, k2, i1, i2, nf, 0, key_bits, w->stream));
            hipLaunchKernelGGL(k_permute3, dim3(g), dim3(kTPB), 0, w->stream, i2, fo, fk, fr, (int32_t*)(D + o_fo),
                               (int32_t*)(D + o_fk), (int32_t*)(D + o_fr), (int)nf);
        }
    }
    HIPCHK(hipGetLastError());
    if (total) HIPCHK(hipMemcpyAsync(w->fr_pin, D, total, hipMemcpyDeviceToHost, w->stream));
    HIPCHK(hipStreamSynchronize(w->stream));
    char* H = w->fr_pin;
    o->n_ev = (int64_t)ne;
    o->n_re = (int64_t)nr;
    o->n_fi = (int64_t)nf;
    o->n_msgs = (int64_t)nm;
    o->bytes = (int64_t)total;
    if (events) {
        o->ev_obj = (const int32_t*)(H + o_eo);
        o->ev_pid = (const int32_t*)(H + o_ep);
        o->ev_old = (const uint64_t*)(H + o_eold);
        o->ev_new = (const uint64_t*)(H + o_enew);
        if (heads) {
            o->ev_old_h = (const uint64_t*)(H + o_eoh);
            o->ev_new_h = (const uint64_t*)(H + o_enh);
        }
        o->re_obj = (const int32_t*)(H + o_ro);
        o->re_rrc = (const uint32_t*)(H + o_rr);
        o->re_old = (const uint64_t*)(H + o_rold);
        o->re_new = (const uint64_t*)(H + o_rnew);
        if (rheads) {  // (the device writes them for the Updates of object cells only: 0 elsewhere)
            uint64_t* oh = (uint64_t*)(H + o_roh);
            uint64_t* nh = (uint64_t*)(H + o_rnh);
            for (size_t i = 0; i < nr; i++)
                if (!rrc_obj_update(w, o->re_rrc[i])) oh[i] = nh[i] = 0;
            o->re_old_h = oh;
            o->re_new_h = nh;
        }
    }
    if (fired) {
        o->fi_obj = (const int32_t*)(H + o_fo);
        o->fi_kind = (const int32_t*)(H + o_fk);
        o->fi_remain = (const int32_t*)(H + o_fr);
    }
    if (fan) {
        o->msg_off = (const uint32_t*)(H + o_mo);
        o->msg_rcpt = (const int32_t*)(H + o_mr);
    }
    return NFK_OK;
}

// ---- scene queries (nfk_query_objects) ----
// the segments [s0, s1) of a scene (all: every group, in group-id order) or of one scene group
static void seg_range(const World* w, int32_t scene, bool all, int32_t group, size_t* s0, size_t* s1) {
    const uint64_t k0 = seg_key_of(scene, all ? INT32_MIN : group), k1 = seg_key_of(scene, all ? INT32_MAX : group);
    *s0 = (size_t)(std::lower_bound(w->seg_key.begin(), w->seg_key.end(), k0) - w->seg_key.begin());
    *s1 = (size_t)(std::upper_bound(w->seg_key.begin(), w->seg_key.end(), k1) - w->seg_key.begin());
}

static int query_check(const World* w, const nfk_query& q) {
    if (q.who != NFK_Q_PLAYERS && q.who != NFK_Q_OTHERS) return fail(NFK_ERR_ARG, "nfk_query: bad who");
    if (q.flags & ~NFK_Q_ALL_GROUPS) return fail(NFK_ERR_ARG, "nfk_query: bad flags");
    if (q.pid < -1 || q.pid >= w->n_prop) return fail(NFK_ERR_ARG, "nfk_query: bad property id");
    if (q.pid < 0) return NFK_OK;
    if (q.mode == NFK_Q_INT_EQ32) {
        if (q.pid >= w->cfg.n_int) return fail(NFK_ERR_ARG, "nfk_query: NFK_Q_INT_EQ32 on a property that is no int");
    } else if (q.mode == NFK_Q_OBJ_EQ) {
        if (q.pid < w->n_if) return fail(NFK_ERR_ARG, "nfk_query: NFK_Q_OBJ_EQ on a property that is no object");
    } else {
        return fail(NFK_ERR_ARG, "nfk_query: bad mode");
    }
    return NFK_OK;
}

int nfk_query_objects(void* world, int32_t n_q, const nfk_query* q, nfk_query_result* out) {
    World* w = (World*)world;
    if (!w || !out || n_q < 0 || (n_q && !q)) return fail(NFK_ERR_ARG, "null argument");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    if (n_q > NFK_MAX_QUERIES) return fail(NFK_ERR_ARG, "more than NFK_MAX_QUERIES queries in one batch");
    uint64_t pidmask[2] = {0, 0};
    for (int32_t i = 0; i < n_q; i++) {
        if (int r = query_check(w, q[i])) return r;
        if (q[i].pid >= 0) pidmask[q[i].pid >> 6] |= 1ull << (q[i].pid & 63);
    }
    *out = nfk_query_result{};
    static const uint32_t kNoOff = 0;
    out->off = &kNoOff;
    if (n_q == 0) return NFK_OK;

    // the window's affected objects: membership calls (touched), and per queried property the
    // untouched objects with a queued Set of it, as (pid, object) sorted
    std::vector<std::pair<int32_t, int32_t>> xaff;
    if (pidmask[0] | pidmask[1]) {
        if (int r = index_queued_sets(w)) return r;
        for (const auto& kv : w->ov_last) {
            const int32_t pid = (int32_t)(kv.first & 127), o = (int32_t)(kv.first >> 7);
            if (((pidmask[pid >> 6] >> (pid & 63)) & 1) && !w->m_flag[o]) xaff.push_back({pid, o});
        }
        // a queried linked property (nfk_link_record): queued calls on its record count as a queued Set
        if ((pidmask[0] & w->lk_pids[0]) | (pidmask[1] & w->lk_pids[1]))
            for (const auto& kv : w->rq_index) {
                const int32_t r = (int32_t)(kv.first & 7), o = (int32_t)(kv.first >> 3);
                if (!w->lk_rows[r] || w->m_flag[o] || !w->alive[o]) continue;
                for (int c = 0; c < NFK_MAX_REC_COLS; c++) {
                    const int32_t pid = w->lk_pid[r][c];
                    if (pid >= 0 && ((pidmask[pid >> 6] >> (pid & 63)) & 1)) xaff.push_back({pid, o});
                }
            }
        std::sort(xaff.begin(), xaff.end());
    }
    auto xaff_of = [&](int32_t pid) {
        const auto a = std::lower_bound(xaff.begin(), xaff.end(), std::make_pair(pid, INT32_MIN));
        const auto b = std::lower_bound(xaff.begin(), xaff.end(), std::make_pair(pid + 1, INT32_MIN));
        return std::make_pair((size_t)(a - xaff.begin()), (size_t)(b - xaff.begin()));
    };

    // slot ranges, tiles and the bound of each query's hits from the segments' bookkeeping
    struct Plan { size_t s0, s1; int32_t lo, hi, tiles; size_t ub, n_aff; };
    std::vector<Plan> pl(n_q);
    size_t nt = 0, ub = 0, fin = 0;
    int32_t max_tiles = 0;
    for (int32_t i = 0; i < n_q; i++) {
        Plan& p = pl[i];
        seg_range(w, q[i].scene, (q[i].flags & NFK_Q_ALL_GROUPS) != 0, q[i].group, &p.s0, &p.s1);
        p.lo = p.hi = 0;
        p.ub = 0;
        if (p.s0 < p.s1) {
            p.lo = w->segs[p.s0].base;
            p.hi = w->segs[p.s1 - 1].base + (int32_t)w->segs[p.s1 - 1].objs.size();
            for (size_t g = p.s0; g < p.s1; g++) {
                const World::Seg& sg = w->segs[g];
                p.ub += q[i].who == NFK_Q_PLAYERS ? (size_t)sg.np : sg.objs.size() - (size_t)sg.np;
            }
            if (p.lo < 0 || p.hi < p.lo || p.hi > w->d.cap) return fail(NFK_ERR_STATE, "segment table out of the slot range");
        }
        p.tiles = (p.hi - p.lo + kTile - 1) / kTile;
        max_tiles = std::max(max_tiles, p.tiles);
        nt += (size_t)p.tiles;
        ub += p.ub;
        p.n_aff = w->touched.size();
        if (q[i].pid >= 0) {
            const auto xr = xaff_of(q[i].pid);
            p.n_aff += xr.second - xr.first;
        }
        fin += p.ub + p.n_aff;
    }
    const bool correct = !w->touched.empty() || !xaff.empty();

    // one region uploaded (descriptors, first tiles), one region read back (offsets, hits)
    const size_t nq1 = (size_t)n_q + 1;
    const size_t u_q = 0, u_t0 = align16((size_t)n_q * sizeof(QDev)), u_end = align16(u_t0 + nq1 * 4);
    const size_t d_cnt = u_end, d_base = align16(d_cnt + nt * 4), d_off = align16(d_base + (nt + 1) * 4);
    const size_t r_obj = align16(nq1 * 4), r_bytes = r_obj + ub * 4;  // (within the read-back region)
    const size_t d_end = d_off + r_bytes;
    const size_t h_res = u_end, h_foff = align16(h_res + r_bytes), h_fobj = align16(h_foff + nq1 * 4);
    const size_t h_ex = align16(h_fobj + (correct ? fin : 0) * 4), h_end = h_ex + align16((size_t)n_q);
    if (int r = dev_reserve(w, &w->q_dev, &w->q_dcap, d_end)) return r;
    if (h_end > w->q_pcap) {
        if (w->q_pin) HIPCHK(hipHostFree(w->q_pin));
        w->q_pin = nullptr;
        const size_t c = std::max(h_end, w->q_pcap + w->q_pcap / 2);
        w->q_pcap = 0;  // (until the new buffer exists)
        HIPCHK(hipHostMalloc((void**)&w->q_pin, c, hipHostMallocDefault));
        w->q_pcap = c;
    }
    char* H = w->q_pin;
    char* D = (char*)w->q_dev;
    QDev* hq = (QDev*)(H + u_q);
    int32_t* ht0 = (int32_t*)(H + u_t0);
    uint8_t* exists = (uint8_t*)(H + h_ex);
    int32_t t0 = 0;
    for (int32_t i = 0; i < n_q; i++) {
        const Plan& p = pl[i];
        QDev x{};
        x.lo = p.lo;
        x.hi = p.hi;
        x.tile0 = ht0[i] = t0;
        t0 += p.tiles;
        x.who = q[i].who;
        x.cls_mask = q[i].cls_mask & 0x7FFFu;  // (class 15 marks a free slot)
        x.mode = q[i].pid < 0 ? -1 : q[i].mode;
        x.skip_slot = -1;
        const int32_t so = q[i].skip_obj;
        if (so >= 0 && so < w->n_obj && !w->m_flag[so]) x.skip_slot = w->slot_of_obj[so];
        if (q[i].pid >= 0) {
            x.p_off = w->tab.p_off[q[i].pid];
            x.p_str = w->tab.p_str[q[i].pid];
        }
        x.value = (uint64_t)q[i].value;
        x.value_head = (uint64_t)q[i].value_head;
        hq[i] = x;
        // it has a segment, or had one (an object of the window entering it: below)
        exists[i] = p.s0 < p.s1 || ((q[i].flags & NFK_Q_ALL_GROUPS)
                                        ? w->known_scenes.count(q[i].scene)
                                        : w->known_groups.count(seg_key_of(q[i].scene, q[i].group)))
                        ? 1
                        : 0;
    }
    ht0[n_q] = t0;
    uint32_t* roff = (uint32_t*)(H + h_res);
    int32_t* robj = (int32_t*)(H + h_res + r_obj);
    if (nt == 0) {
        memset(roff, 0, nq1 * 4);  // (no slot to look at: nothing is launched)
    } else {
        const bool timed = w->profiling;
        if (timed)
            for (auto& e : w->q_ev)
                if (!e) HIPCHK(hipEventCreate(&e));
        HIPCHK(hipMemcpyAsync(D, H, u_end, hipMemcpyHostToDevice, w->stream));
        if (timed) HIPCHK(hipEventRecord(w->q_ev[0], w->stream));
        const dim3 grid((unsigned)max_tiles, (unsigned)n_q);
        hipLaunchKernelGGL(k_query<false>, grid, dim3(kTPB), 0, w->stream, (const QDev*)(D + u_q), w->d.fan_desc,
                           (const uint64_t*)w->d.pmem, (const int32_t*)w->slot_obj_d, (uint32_t*)(D + d_cnt),
                           (const uint32_t*)nullptr, (int32_t*)nullptr, 0u);
        hipLaunchKernelGGL(k_query_scan, dim3(1), dim3(1024), 0, w->stream, (const uint32_t*)(D + d_cnt),
                           (uint32_t*)(D + d_base), (int)nt, (const int32_t*)(D + u_t0), (int)n_q, (uint32_t*)(D + d_off));
        hipLaunchKernelGGL(k_query<true>, grid, dim3(kTPB), 0, w->stream, (const QDev*)(D + u_q), w->d.fan_desc,
                           (const uint64_t*)w->d.pmem, (const int32_t*)w->slot_obj_d, (uint32_t*)nullptr,
                           (const uint32_t*)(D + d_base), (int32_t*)(D + d_off + r_obj), (uint32_t)ub);
        HIPCHK(hipGetLastError());
        if (timed) HIPCHK(hipEventRecord(w->q_ev[1], w->stream));
        HIPCHK(hipMemcpyAsync(H + h_res, D + d_off, r_bytes, hipMemcpyDeviceToHost, w->stream));
        HIPCHK(hipStreamSynchronize(w->stream));
        out->bytes = (int64_t)r_bytes;
        if (timed) {
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, w->q_ev[0], w->q_ev[1]));
            out->kernel_ms = ms;
        }
        if (roff[n_q] > ub) return fail(NFK_ERR_DEVICE, "scene query: more hits than the segments' members");
    }
    out->exists = exists;
    out->off = roff;
    out->obj = robj;
    if (!correct) return NFK_OK;

    // the window's calls on top: every affected object is evaluated on the host, from the membership
    // arrays as the calls have left them and its property as nfk_get_props / nfk_get_objects read it
    struct Cand { int32_t q, o; };
    std::vector<Cand> cand;                 // membership passed (in query order)
    std::vector<int32_t> ro, rp, rc;        // reads of int properties: object, pid, candidate
    std::vector<int32_t> oo, op, oc;        // ... of object properties
    for (int32_t i = 0; i < n_q; i++) {
        const bool all = (q[i].flags & NFK_Q_ALL_GROUPS) != 0;
        auto eval = [&](int32_t o) {
            if (!w->alive[o] || w->scene[o] != q[i].scene || (!all && w->group[o] != q[i].group)) return;
            if (w->m_flag[o]) exists[i] = 1;  // (a scene group the window's calls bring into being)
            if ((w->isplayer[o] != 0) != (q[i].who == NFK_Q_PLAYERS) || !((q[i].cls_mask >> w->cls[o]) & 1u) ||
                o == q[i].skip_obj)
                return;
            if (q[i].pid >= 0) {
                auto& xo = q[i].mode == NFK_Q_OBJ_EQ ? oo : ro;
                auto& xp = q[i].mode == NFK_Q_OBJ_EQ ? op : rp;
                auto& xc = q[i].mode == NFK_Q_OBJ_EQ ? oc : rc;
                xo.push_back(o);
                xp.push_back(q[i].pid);
                xc.push_back((int32_t)cand.size());
            }
            cand.push_back({i, o});
        };
        for (int32_t o : w->touched) eval(o);
        if (q[i].pid >= 0) {
            const auto xr = xaff_of(q[i].pid);
            for (size_t j = xr.first; j < xr.second; j++) eval(xaff[j].second);
        }
    }
    std::vector<uint8_t> keep(cand.size(), 1);
    if (!ro.empty()) {
        std::vector<uint64_t> bits(ro.size());
        if (int r = current_props(w, (int32_t)ro.size(), ro.data(), rp.data(), bits.data())) return r;
        for (size_t j = 0; j < ro.size(); j++)
            keep[rc[j]] = (int64_t)(int32_t)(uint32_t)bits[j] == q[cand[rc[j]].q].value;
    }
    if (!oo.empty()) {
        std::vector<int64_t> vh(oo.size()), vd(oo.size());
        if (int r = current_objects(w, (int32_t)oo.size(), oo.data(), op.data(), vh.data(), vd.data())) return r;
        for (size_t j = 0; j < oo.size(); j++) {
            const nfk_query& qq = q[cand[oc[j]].q];
            keep[oc[j]] = vd[j] == qq.value && vh[j] == qq.value_head;
        }
    }
    // each list without its affected objects, the re-evaluated ones merged in by (group, NFGUID)
    auto before = [&](int32_t a, int32_t b) { return w->group[a] != w->group[b] ? w->group[a] < w->group[b] : guid_less(w, a, b); };
    if (w->q_mark.size() < (size_t)w->n_obj) w->q_mark.resize(w->n_obj, 0);
    for (int32_t o : w->touched) w->q_mark[o] = 1;
    uint32_t* foff = (uint32_t*)(H + h_foff);
    int32_t* fobj = (int32_t*)(H + h_fobj);
    std::vector<int32_t> add;
    size_t c0 = 0;
    uint32_t at = 0;
    for (int32_t i = 0; i < n_q; i++) {
        foff[i] = at;
        add.clear();
        for (; c0 < cand.size() && cand[c0].q == i; c0++)
            if (keep[c0]) add.push_back(cand[c0].o);
        std::sort(add.begin(), add.end(), before);
        std::pair<size_t, size_t> xr{0, 0};
        if (q[i].pid >= 0) xr = xaff_of(q[i].pid);
        for (size_t j = xr.first; j < xr.second; j++) w->q_mark[xaff[j].second] = 1;
        size_t a = 0;
        for (uint32_t h = roff[i]; h < roff[i + 1]; h++) {
            const int32_t o = robj[h];
            if (w->q_mark[o]) continue;
            while (a < add.size() && before(add[a], o)) fobj[at++] = add[a++];
            fobj[at++] = o;
        }
        while (a < add.size()) fobj[at++] = add[a++];
        for (size_t j = xr.first; j < xr.second; j++) w->q_mark[xaff[j].second] = 0;
    }
    foff[n_q] = at;
    for (int32_t o : w->touched) w->q_mark[o] = 0;
    out->off = foff;
    out->obj = fobj;
    return NFK_OK;
}

int nfk_online_count(void* world, int32_t scene, int32_t group, int32_t* n) {
    World* w = (World*)world;
    if (!w || !n) return fail(NFK_ERR_ARG, "null argument");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    size_t s0 = 0, s1 = w->segs.size();
    if (scene >= 0) seg_range(w, scene, group < 0, group, &s0, &s1);
    int64_t c = 0;
    for (size_t g = s0; g < s1; g++) c += w->segs[g].np;
    // the window's membership calls: a touched player leaves the segment of its slot and, alive,
    // joins the scene group the calls have left it in
    for (int32_t o : w->touched) {
        if (!w->isplayer[o]) continue;
        const int32_t sl = w->slot_of_obj[o];
        if (sl >= 0 && w->src_row[o] < 0) {
            size_t a = 0, b = w->segs.size();  // the last segment whose base is <= sl
            while (b - a > 1) {
                const size_t m = (a + b) / 2;
                if (w->segs[m].base <= sl) a = m;
                else b = m;
            }
            if (a >= s0 && a < s1) c--;
        }
        if (w->alive[o] && (scene < 0 || (w->scene[o] == scene && (group < 0 || w->group[o] == group)))) c++;
    }
    *n = (int32_t)c;
    return NFK_OK;
}

// ---- view changes (nfk_view_changes) ----
// entry i's visits in the reference's order (AOI:292-529 under KM:929-945, 248-249, 291-294)
static void vc_visits(const nfk_vc_entry& e, std::vector<nfk_vc_visit>& out) {
    const int32_t s0 = e.from_scene, g0 = e.from_group, s1 = e.to_scene, g1 = e.to_group;
    switch (e.kind) {
    case NFK_VC_SWITCH:
        if (g0 > 0) out.push_back({NFK_VC_GROUP_LEAVE, s0, g0});
        if (s0 != s1) {
            out.push_back({NFK_VC_SCENE_LEAVE, s0, 0});
            out.push_back({NFK_VC_SCENE_ENTER, s1, 0});
        }
        if (g1 > 0) out.push_back({NFK_VC_GROUP_ENTER, s1, g1});
        break;
    case NFK_VC_DESTROY:
        if (s0 > 0) out.push_back({NFK_VC_WHY_DESTROY, s0, g0});
        break;
    case NFK_VC_CREATE:
        if (s1 != 0) out.push_back({NFK_VC_SCENE_ENTER, s1, 0});
        if (g1 > 0) out.push_back({NFK_VC_GROUP_ENTER, s1, g1});
        break;
    default:  // NFK_VC_EXPORT
        if (g0 > 0) out.push_back({NFK_VC_GROUP_LEAVE, s0, g0});
        out.push_back({NFK_VC_SCENE_LEAVE, s0, 0});
        break;
    }
}

int nfk_view_changes(void* world, nfk_view_changes_result* out) {
    World* w = (World*)world;
    if (!w || !out) return fail(NFK_ERR_ARG, "null argument");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    *out = nfk_view_changes_result{};
    static const uint32_t kNoOff[1] = {0};
    out->call_visit = out->visit_off = kNoOff;
    const size_t n = w->vc_log.size();
    if (n == 0) {
        HIPCHK(hipStreamSynchronize(w->stream));
        return NFK_OK;
    }
    constexpr uint32_t kNever = 0xFFFFFFFFu;
    std::vector<nfk_vc_visit> vis;
    std::vector<uint32_t> cv(n + 1);
    // the window's leavers (a frame-start member's first entry) and stints (every membership
    // interval that begins in the window)
    struct Stint { uint64_t key; int32_t obj, pos; uint32_t t_in, t_out; };
    std::vector<Stint> st;
    std::vector<int32_t> lv_slot;
    std::vector<uint32_t> lv_val;
    if (w->vc_last.size() < (size_t)w->n_obj) w->vc_last.resize(w->n_obj, -2);  // -2: no entry yet
    auto resident = [w](int32_t o) { return w->slot_of_obj[o] >= 0 && w->src_row[o] < 0; };
    for (size_t i = 0; i < n; i++) {
        const nfk_vc_entry& e = w->vc_log[i];
        cv[i] = (uint32_t)vis.size();
        vc_visits(e, vis);
        int32_t& last = w->vc_last[e.obj];
        if (last == -2) {
            if (e.kind != NFK_VC_CREATE && resident(e.obj)) {
                lv_slot.push_back(w->slot_of_obj[e.obj]);
                lv_val.push_back((uint32_t)i);
            }
        } else if (last >= 0) {
            st[last].t_out = (uint32_t)i;
        }
        last = -1;
        if (e.kind == NFK_VC_SWITCH || e.kind == NFK_VC_CREATE) {
            last = (int32_t)st.size();
            st.push_back({seg_key_of(e.to_scene, e.to_group), e.obj, 0, (uint32_t)i, kNever});
        }
    }
    cv[n] = (uint32_t)vis.size();
    for (size_t i = 0; i < n; i++) w->vc_last[w->vc_log[i].obj] = -2;
    std::sort(st.begin(), st.end(), [w](const Stint& a, const Stint& b) {
        if (a.key != b.key) return a.key < b.key;
        if (guid_less(w, a.obj, b.obj)) return true;
        if (guid_less(w, b.obj, a.obj)) return false;
        return a.t_in < b.t_in;
    });
    for (size_t a = 0; a < st.size();) {  // pos: the lower-bound slot in the group's frame-start segment
        size_t b = a;
        while (b < st.size() && st[b].key == st[a].key) b++;
        const auto it = std::lower_bound(w->seg_key.begin(), w->seg_key.end(), st[a].key);
        if (it != w->seg_key.end() && *it == st[a].key) {
            const World::Seg& sg = w->segs[it - w->seg_key.begin()];
            for (size_t j = a; j < b; j++) {
                const World::Guid k = w->guid[st[j].obj];
                const auto at = std::lower_bound(sg.keys.begin(), sg.keys.end(), k, [](const World::Guid& x, const World::Guid& y) {
                    return x.h != y.h ? x.h < y.h : x.d < y.d;
                });
                st[j].pos = sg.base + (int32_t)(at - sg.keys.begin());
            }
        }
        a = b;
    }
    const size_t n_v = vis.size(), n_st = st.size(), n_lv = lv_slot.size();

    // per visit: its slot range, its stints, its tiles and the bound of its two lists
    struct Plan { int32_t seg, lo, hi, st0, st_n, tiles; bool host; };
    std::vector<Plan> pl(n_v);
    size_t nt = 0, ub = 0, ub_host = 0, n_host = 0;
    int32_t max_tiles = 0;
    for (size_t i = 0; i < n; i++)
        for (uint32_t v = cv[i]; v < cv[i + 1]; v++) {
            Plan& p = pl[v];
            p.seg = find_seg(w, vis[v].scene, vis[v].group);
            p.lo = p.hi = 0;
            if (p.seg >= 0) {
                p.lo = w->segs[p.seg].base;
                p.hi = p.lo + (int32_t)w->segs[p.seg].objs.size();
                if (p.lo < 0 || p.hi > w->d.cap) return fail(NFK_ERR_STATE, "segment table out of the slot range");
            }
            const uint64_t key = seg_key_of(vis[v].scene, vis[v].group);
            const auto a = std::lower_bound(st.begin(), st.end(), key, [](const Stint& x, uint64_t k) { return x.key < k; });
            const auto b = std::upper_bound(a, st.end(), key, [](uint64_t k, const Stint& x) { return k < x.key; });
            p.st0 = (int32_t)(a - st.begin());
            p.st_n = (int32_t)(b - a);
            p.host = p.st_n > NFK_VC_STINT_CAP;
            const size_t bound = (size_t)(p.hi - p.lo) + (size_t)p.st_n;
            if (p.host) {
                p.tiles = 0;
                ub_host += bound;
                n_host++;
            } else {
                // (a visit with stints has the tile of `hi`: a stint's pos lies in [lo, hi])
                p.tiles = p.st_n ? (p.hi - p.lo) / kTile + 1 : (p.hi - p.lo + kTile - 1) / kTile;
                ub += bound;
            }
            max_tiles = std::max(max_tiles, p.tiles);
            nt += (size_t)p.tiles;
        }
    if (ub + ub_host > (size_t)NFK_VC_MAX_ENTRIES)
        return fail(NFK_ERR_CAPACITY, "view changes: the window's lists can hold " + std::to_string(ub + ub_host) +
                                          " entries, more than NFK_VC_MAX_ENTRIES (execute the window in parts)");

    // one region uploaded (visits, the lists' first tiles, stints, leavers), one read back (offsets, lists)
    const size_t nv2 = 2 * n_v + 1;
    const size_t u_v = 0, u_t0 = align16(n_v * sizeof(VDev)), u_st = align16(u_t0 + nv2 * 4);
    const size_t u_ls = align16(u_st + n_st * sizeof(VStint)), u_lv = align16(u_ls + n_lv * 4), u_end = align16(u_lv + n_lv * 4);
    const size_t d_cnt = u_end, d_base = align16(d_cnt + 2 * nt * 4), d_off = align16(d_base + (2 * nt + 1) * 4);
    const size_t r_obj = align16(nv2 * 4), r_bytes = r_obj + ub * 4;
    const size_t d_end = d_off + r_bytes;
    const size_t h_log = u_end, h_cv = align16(h_log + n * sizeof(nfk_vc_entry)), h_vis = align16(h_cv + (n + 1) * 4);
    const size_t h_res = align16(h_vis + n_v * sizeof(nfk_vc_visit)), h_foff = align16(h_res + r_bytes);
    const size_t h_fobj = align16(h_foff + nv2 * 4), h_end = h_fobj + (n_host ? (ub + ub_host) * 4 : 0);
    if (int r = dev_reserve(w, &w->vc_dev, &w->vc_dcap, d_end)) return r;
    if (h_end > w->vc_pcap) {
        if (w->vc_pin) HIPCHK(hipHostFree(w->vc_pin));
        w->vc_pin = nullptr;
        const size_t c = std::max(h_end, w->vc_pcap + w->vc_pcap / 2);
        w->vc_pcap = 0;  // (until the new buffer exists)
        HIPCHK(hipHostMalloc((void**)&w->vc_pin, c, hipHostMallocDefault));
        w->vc_pcap = c;
    }
    char* H = w->vc_pin;
    char* D = (char*)w->vc_dev;
    VDev* hv = (VDev*)(H + u_v);
    int32_t* ht0 = (int32_t*)(H + u_t0);
    VStint* hs = (VStint*)(H + u_st);
    int32_t t0 = 0;
    for (size_t i = 0; i < n; i++) {
        const int32_t self = w->vc_log[i].obj;
        for (uint32_t v = cv[i]; v < cv[i + 1]; v++) {
            const Plan& p = pl[v];
            VDev x{};
            x.lo = p.lo;
            x.hi = p.host ? p.lo : p.hi;
            x.tile0 = t0;
            x.tiles = p.tiles;
            x.t = (uint32_t)i;
            x.skip_slot = resident(self) ? w->slot_of_obj[self] : -1;
            x.st0 = p.st0;
            x.st_n = p.host ? 0 : p.st_n;
            hv[v] = x;
            ht0[2 * v] = 2 * t0;
            ht0[2 * v + 1] = 2 * t0 + p.tiles;
            t0 += p.tiles;
        }
    }
    ht0[2 * n_v] = 2 * t0;
    for (size_t j = 0; j < n_st; j++)
        hs[j] = VStint{(uint32_t)st[j].obj | (w->isplayer[st[j].obj] ? 0x80000000u : 0u), st[j].pos, st[j].t_in, st[j].t_out};
    if (n_lv) {
        memcpy(H + u_ls, lv_slot.data(), n_lv * 4);
        memcpy(H + u_lv, lv_val.data(), n_lv * 4);
    }
    memcpy(H + h_log, w->vc_log.data(), n * sizeof(nfk_vc_entry));
    memcpy(H + h_cv, cv.data(), (n + 1) * 4);
    if (n_v) memcpy(H + h_vis, vis.data(), n_v * sizeof(nfk_vc_visit));
    uint32_t* roff = (uint32_t*)(H + h_res);
    int32_t* robj = (int32_t*)(H + h_res + r_obj);
    if (nt == 0) {
        memset(roff, 0, nv2 * 4);  // (no slot and no stint to look at: nothing is launched)
        HIPCHK(hipStreamSynchronize(w->stream));
    } else {
        if (w->vc_tout_cap < w->d.cap) {
            HIPCHK(hipStreamSynchronize(w->stream));
            if (w->vc_tout) HIPCHK(hipFree(w->vc_tout));
            w->vc_tout = nullptr;
            w->vc_tout_cap = 0;
            HIPCHK(hipMalloc((void**)&w->vc_tout, (size_t)w->d.cap * 4));
            w->vc_tout_cap = w->d.cap;
            w->vc_dirty = true;
        }
        if (w->vc_dirty) HIPCHK(hipMemsetAsync(w->vc_tout, 0xFF, (size_t)w->vc_tout_cap * 4, w->stream));
        const bool timed = w->profiling;
        if (timed)
            for (auto& e : w->vc_ev)
                if (!e) HIPCHK(hipEventCreate(&e));
        HIPCHK(hipMemcpyAsync(D, H, u_end, hipMemcpyHostToDevice, w->stream));
        if (timed) HIPCHK(hipEventRecord(w->vc_ev[0], w->stream));
        w->vc_dirty = true;  // (until the restore below has run)
        if (n_lv)
            hipLaunchKernelGGL(k_view_scatter, dim3(grid_for(n_lv)), dim3(kTPB), 0, w->stream, (const int32_t*)(D + u_ls),
                               (const uint32_t*)(D + u_lv), (int)n_lv, w->vc_tout, w->vc_tout_cap);
        // (the grid's y is at most 65535: a longer batch goes in runs of visits)
        auto launch = [&](bool write) {
            for (size_t y0 = 0; y0 < n_v; y0 += 65535) {
                const dim3 grid((unsigned)max_tiles, (unsigned)std::min<size_t>(65535, n_v - y0));
                if (!write)
                    hipLaunchKernelGGL(k_view<false>, grid, dim3(kTPB), 0, w->stream, (const VDev*)(D + u_v) + y0,
                                       (const VStint*)(D + u_st), w->d.fan_desc, (const uint32_t*)w->vc_tout,
                                       (const int32_t*)w->slot_obj_d, (uint32_t*)(D + d_cnt), (const uint32_t*)nullptr,
                                       (int32_t*)nullptr, 0u);
                else
                    hipLaunchKernelGGL(k_view<true>, grid, dim3(kTPB), 0, w->stream, (const VDev*)(D + u_v) + y0,
                                       (const VStint*)(D + u_st), w->d.fan_desc, (const uint32_t*)w->vc_tout,
                                       (const int32_t*)w->slot_obj_d, (uint32_t*)nullptr, (const uint32_t*)(D + d_base),
                                       (int32_t*)(D + d_off + r_obj), (uint32_t)ub);
            }
        };
        launch(false);
        hipLaunchKernelGGL(k_query_scan, dim3(1), dim3(1024), 0, w->stream, (const uint32_t*)(D + d_cnt),
                           (uint32_t*)(D + d_base), (int)(2 * nt), (const int32_t*)(D + u_t0), (int)(2 * n_v),
                           (uint32_t*)(D + d_off));
        launch(true);
        if (n_lv)
            hipLaunchKernelGGL(k_view_scatter, dim3(grid_for(n_lv)), dim3(kTPB), 0, w->stream, (const int32_t*)(D + u_ls),
                               (const uint32_t*)nullptr, (int)n_lv, w->vc_tout, w->vc_tout_cap);
        HIPCHK(hipGetLastError());
        if (timed) HIPCHK(hipEventRecord(w->vc_ev[1], w->stream));
        HIPCHK(hipMemcpyAsync(H + h_res, D + d_off, r_bytes, hipMemcpyDeviceToHost, w->stream));
        HIPCHK(hipStreamSynchronize(w->stream));
        w->vc_dirty = false;
        out->bytes = (int64_t)r_bytes;
        if (timed) {
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, w->vc_ev[0], w->vc_ev[1]));
            out->kernel_ms = ms;
        }
        if (roff[2 * n_v] > ub) return fail(NFK_ERR_DEVICE, "view changes: more list entries than members and stints");
    }
    out->n_calls = (int32_t)n;
    out->n_visits = (int32_t)n_v;
    out->log = (const nfk_vc_entry*)(H + h_log);
    out->call_visit = (const uint32_t*)(H + h_cv);
    out->visit = (const nfk_vc_visit*)(H + h_vis);
    out->visit_off = roff;
    out->obj = robj;
    out->n_host = (int32_t)n_host;
    out->n_tiles = (int32_t)nt;
    if (!n_host) return NFK_OK;

    // groups past the stint cap: the same merge on the host, spliced between the device's lists
    std::unordered_map<int32_t, uint32_t> left;  // frame-start members that leave: object -> instant
    for (size_t i = n; i-- > 0;) {
        const nfk_vc_entry& e = w->vc_log[i];
        if (e.kind != NFK_VC_CREATE && resident(e.obj)) left[e.obj] = (uint32_t)i;  // (the first entry wins)
    }
    uint32_t* foff = (uint32_t*)(H + h_foff);
    int32_t* fobj = (int32_t*)(H + h_fobj);
    uint32_t at = 0;
    std::vector<int32_t> others;
    for (size_t i = 0; i < n; i++) {
        const uint32_t t = (uint32_t)i;
        const int32_t self = w->vc_log[i].obj;
        for (uint32_t v = cv[i]; v < cv[i + 1]; v++) {
            const Plan& p = pl[v];
            foff[2 * v] = at;
            if (!p.host) {
                const uint32_t a = roff[2 * v], m = roff[2 * v + 1], b = roff[2 * v + 2];
                memcpy(fobj + at, robj + a, (size_t)(b - a) * 4);
                foff[2 * v + 1] = at + (m - a);
                at += b - a;
                continue;
            }
            others.clear();
            auto emit = [&](int32_t o) {
                if (w->isplayer[o]) fobj[at++] = o;
                else others.push_back(o);
            };
            const World::Seg* sg = p.seg >= 0 ? &w->segs[p.seg] : nullptr;
            int32_t j = p.st0;
            const int32_t je = p.st0 + p.st_n;
            auto stints_to = [&](int32_t slot) {
                for (; j < je && st[j].pos <= slot; j++)
                    if (st[j].t_in < t && t < st[j].t_out) emit(st[j].obj);
            };
            for (int32_t k = 0; k < p.hi - p.lo; k++) {
                stints_to(p.lo + k);
                const int32_t o = sg->objs[k];
                if (o == self) continue;
                const auto it = left.find(o);
                if (it == left.end() || it->second > t) emit(o);
            }
            stints_to(INT32_MAX);
            foff[2 * v + 1] = at;
            for (int32_t o : others) fobj[at++] = o;
        }
    }
    foff[2 * n_v] = at;
    out->visit_off = foff;
    out->obj = fobj;
    return NFK_OK;
}

int nfk_rank_top(void* world, int32_t pid, int32_t k, int32_t* n_out, int64_t* guid_head, int64_t* guid_data,
                 double* score) {
    World* w = (World*)world;
    if (!w || !n_out || (k > 0 && (!guid_head || !guid_data || !score))) return fail(NFK_ERR_ARG, "null argument");
    if (!w->committed) return fail(NFK_ERR_STATE, "commit first");
    if (pid < 0 || pid >= w->n_if || k < 0) return fail(NFK_ERR_ARG, "bad property / k (int or float properties rank)");
    *n_out = 0;
    const Dev& d = w->d;
    if (k == 0 || d.N == 0) return NFK_OK;
    HIPCHK(hipStreamSynchronize(w->stream));
    unsigned* hist = nullptr;
    HIPCHK(hipMalloc((void**)&hist, 257 * 4));
    const unsigned grid = std::min<unsigned>((d.N + kTPB - 1) / kTPB, 2048);
    // radix select of the k-th largest key, 8 bits at a time
    uint64_t prefix = 0, pmask = 0;
    uint64_t above = 0;  // entities with a key above the current prefix range
    for (int shift = 56; shift >= 0; shift -= 8) {
        hipError_t e1 = hipMemsetAsync(hist, 0, 256 * 4, w->stream);
        hipLaunchKernelGGL(k_rank_hist, dim3(grid), dim3(kTPB), 0, w->stream, d, pid, prefix, pmask, shift, hist);
        unsigned h[256];
        hipError_t e2 = hipMemcpyAsync(h, hist, sizeof h, hipMemcpyDeviceToHost, w->stream);
        hipError_t e3 = hipStreamSynchronize(w->stream);
        if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) {
            (void)hipFree(hist);
            return fail(NFK_ERR_HIP, "rank histogram failed");
        }
        int dg = 255;
        for (; dg > 0; dg--) {
            if (above + h[dg] >= (uint64_t)k) break;
            above += h[dg];
        }
        prefix |= (uint64_t)dg << shift;
        pmask |= 0xFFull << shift;
    }
    // everything at or above the k-th key: fewer than k above it plus all its ties
    const uint64_t thr = prefix;
    unsigned cnt = 0;
    std::vector<int64_t> cand;  // (slot, raw property word) pairs
    for (int attempt = 0; attempt < 2; attempt++) {
        const unsigned cap = attempt == 0 ? (unsigned)std::min<int64_t>(4 * (int64_t)k + 1024, d.N) : cnt;
        int64_t* out = nullptr;
        HIPCHK(hipMalloc((void**)&out, (size_t)std::max(cap, 1u) * 16));
        HIPCHK(hipMemsetAsync(hist + 256, 0, 4, w->stream));
        hipLaunchKernelGGL(k_rank_collect, dim3(grid), dim3(kTPB), 0, w->stream, d, pid, thr, hist + 256, out, cap);
        HIPCHK(hipMemcpyAsync(&cnt, hist + 256, 4, hipMemcpyDeviceToHost, w->stream));
        HIPCHK(hipStreamSynchronize(w->stream));
        if (cnt <= cap) {
            cand.resize((size_t)cnt * 2);
            if (cnt) HIPCHK(hipMemcpy(cand.data(), out, (size_t)cnt * 16, hipMemcpyDeviceToHost));
            (void)hipFree(out);
            break;
        }
        (void)hipFree(out);
    }
    (void)hipFree(hist);
    // ZREVRANGE order: score desc, member (NFGUID::ToString, NFGUID.h:93) desc
    struct C { double s; int32_t o; std::string m; };
    std::vector<C> cs;
    cs.reserve(cand.size() / 2);
    for (size_t i = 0; i < cand.size(); i += 2) {
        const int32_t sl = (int32_t)cand[i];
        const uint64_t raw = (uint64_t)cand[i + 1];
        double sc;
        if (pid < d.n_int) sc = (double)(int64_t)raw;
        else memcpy(&sc, &raw, 8);
        const int32_t o = w->obj_of_slot[sl];
        cs.push_back({sc, o, std::to_string(w->gh[o]) + "-" + std::to_string(w->gd[o])});
    }
    std::sort(cs.begin(), cs.end(), [](const C& a, const C& b) { return a.s != b.s ? a.s > b.s : a.m > b.m; });
    const int32_t n = (int32_t)std::min<size_t>(cs.size(), (size_t)k);
    for (int32_t i = 0; i < n; i++) {
        guid_head[i] = w->gh[cs[i].o];
        guid_data[i] = w->gd[cs[i].o];
        score[i] = cs[i].s;
    }
    *n_out = n;
    return NFK_OK;
}

static void copy_msg(const std::string& m, char* out, int32_t cap) {
    if (!out || cap <= 0) return;
    const size_t n = std::min(m.size(), (size_t)cap - 1);
    memcpy(out, m.data(), n);
    out[n] = 0;
}

int nfk_jit_status(void* world, int32_t* on, char* msg, int32_t cap) {
    World* w = (World*)world;
    if (!w || !on) return fail(NFK_ERR_ARG, "null argument");
    *on = w->jit_fn != nullptr;
    copy_msg(w->jit_msg, msg, cap);
    return NFK_OK;
}

int nfk_jit_preview(int32_t n_int, int32_t n_flt, int32_t n_class, int32_t n_kind, const uint8_t* prop_flags,
                    const nfk_op* ops, const int32_t* n_ops, int32_t compile, int32_t* ok, char* src, int32_t src_cap,
                    char* msg, int32_t msg_cap) {
    return nfk_jit_preview_rec(n_int, n_flt, n_class, n_kind, prop_flags, ops, n_ops, 0, nullptr, nullptr, nullptr, compile,
                               ok, src, src_cap, msg, msg_cap);
}

int nfk_jit_preview_rec(int32_t n_int, int32_t n_flt, int32_t n_class, int32_t n_kind, const uint8_t* prop_flags,
                        const nfk_op* ops, const int32_t* n_ops, int32_t n_rec, const int32_t* rec_rows,
                        const int32_t* rec_cols, const uint8_t* col_types, int32_t compile, int32_t* ok, char* src,
                        int32_t src_cap, char* msg, int32_t msg_cap) {
    if (n_rec < 0 || n_rec > NFK_MAX_RECORDS || (n_rec && (!rec_rows || !rec_cols))) return fail(NFK_ERR_ARG, "bad records");
    if (!ok || !prop_flags || (n_kind && (!ops || !n_ops)) || n_int < 0 || n_flt < 0 || n_int > NFK_MAX_INT_PROPS ||
        n_flt > NFK_MAX_FLT_PROPS || n_class <= 0 || n_class >= NFK_MAX_CLASSES || n_kind < 0 || n_kind > NFK_MAX_KINDS)
        return fail(NFK_ERR_ARG, "bad schema");
    *ok = 0;
    std::unique_ptr<Tables> tab(new Tables());
    memset(tab.get(), 0, sizeof(Tables));
    const int np = n_int + n_flt;
    for (int c = 0; c < n_class; c++)
        for (int p = 0; p < np; p++) tab->pflags[c][p] = prop_flags[(size_t)c * np + p];
    for (int k = 0; k < n_kind; k++) {
        if (n_ops[k] < 0 || n_ops[k] > NFK_MAX_OPS) return fail(NFK_ERR_ARG, "bad op count");
        tab->nops[k] = n_ops[k];
        for (int i = 0; i < n_ops[k]; i++) tab->ops[k][i] = ops[(size_t)k * NFK_MAX_OPS + i];
    }
    for (int r = 0; r < n_rec; r++) {
        if (rec_rows[r] <= 0 || rec_rows[r] > NFK_MAX_REC_ROWS || rec_cols[r] <= 0 || rec_cols[r] > NFK_MAX_REC_COLS)
            return fail(NFK_ERR_ARG, "bad record shape");
        tab->rec_rows[r] = rec_rows[r];
        tab->rec_cols[r] = rec_cols[r];
        // the column types, as nfk_define_record checks them: an object column is a data half with
        // its head half right behind it
        for (int c = 0; col_types && c < rec_cols[r]; c++) {
            const uint8_t* ct = col_types + (size_t)r * NFK_MAX_REC_COLS;
            if (ct[c] > NFK_REC_OBJ_HEAD || (ct[c] == NFK_REC_OBJ_DATA && (c + 1 >= rec_cols[r] || ct[c + 1] != NFK_REC_OBJ_HEAD)) ||
                (ct[c] == NFK_REC_OBJ_HEAD && (c == 0 || ct[c - 1] != NFK_REC_OBJ_DATA)))
                return fail(NFK_ERR_ARG, "bad record column types");
            tab->rec_ctype[r][c] = ct[c];
        }
    }
    for (int k = 0; k < n_kind; k++)  // a record op on a half of an object column, as nfk_define_kind refuses it
        for (int i = 0; i < n_ops[k]; i++) {
            const nfk_op& op = tab->ops[k][i];
            if (op.code != NFK_OP_RIADD_CLAMP && op.code != NFK_OP_RFAFFINE) continue;
            const int r = op.dst >> 8, col = op.dst & 255;
            if (r < n_rec && col < rec_cols[r] && tab->rec_ctype[r][col] >= NFK_REC_OBJ_DATA)
                return fail(NFK_ERR_ARG, "record op on a half of an object column");
        }
    for (int k = 0; k < n_kind; k++)  // the guard cells, as nfk_define_kind checks them
        for (int i = 0; i < n_ops[k]; i++) {
            const nfk_op& op = tab->ops[k][i];
            if (!(op.flags & NFK_GUARD_CELL)) continue;
            const uint32_t c = op.guard & 0x1FFFu, r = cell_rec(c);
            if (!(op.flags & NFK_GUARD) || (op.guard & 0xE000u) || (int)r >= n_rec || (int)cell_row(c) >= rec_rows[r] ||
                (int)cell_col(c) >= rec_cols[r] || (col_types && col_types[(size_t)r * NFK_MAX_REC_COLS + cell_col(c)] != 0))
                return fail(NFK_ERR_ARG, "NFK_GUARD_CELL: not an int cell of a defined record");
        }
    std::vector<int> wp, rp;
    const bool u_ok = build_u_tables(*tab, n_kind, wp, rp);
    Dev d{};
    d.n_kind = n_kind;
    fill_u_dev(d, *tab, wp, rp, u_ok);
    if (!u_ok) {
        copy_msg("working set does not fit k_tick (k_tick_touch runs)", msg, msg_cap);
        return NFK_OK;
    }
    const JitOptions jo = jit_options(d);  // (rank workgroups compiled in, as for a world without record ops)
    const std::string s = jit_schema_source(*tab, d, jo.nt, jo.lb);
    copy_msg(s, src, src_cap);
    if (!compile) {
        *ok = 1;
        return NFK_OK;
    }
    const int u = std::max(d.n_u, 1);
    JitBuild b = jit_compile(s, jo.waves, u, true);  // (with the kernels' resource usage in the log)
    *ok = b.ok;
    if (b.ok) {
        // the compiler's log as before (its warnings), then the kernels' resource remarks, each cut to
        // "Function Name: ...", "VGPRs Spill: n", ... on a line of its own (a remark comes with its
        // source line, a caret line and location notes: those are dropped)
        std::istringstream in(b.log);
        std::string line, other, usage_lines;
        const std::string tag = " [-Rpass-analysis=kernel-resource-usage]";
        bool in_remark = false;  // inside a remark's own lines, until the next warning or error begins
        while (std::getline(in, line)) {
            const size_t r = line.find("remark: "), t = line.find(tag);
            if (r != std::string::npos && t != std::string::npos && t > r) {
                usage_lines += line.substr(r + 8, t - r - 8) + "\n";
                in_remark = true;
                continue;
            }
            if (line.find("warning:") != std::string::npos || line.find("error:") != std::string::npos) in_remark = false;
            if (!in_remark) other += line + "\n";
        }
        b.log = other + usage_lines;
    }
    copy_msg(b.ok ? b.lowered + " (" + std::to_string(b.code.size()) + " B code object)\n" + b.log : b.log, msg, msg_cap);
    return NFK_OK;
}

int nfk_set_profiling(void* world, int32_t on) {
    World* w = (World*)world;
    if (!w) return fail(NFK_ERR_ARG, "null world");
    w->profiling = on != 0;
    return NFK_OK;
}

int nfk_kernel_times(void* world, double* ms, int64_t* launches, int64_t* bytes) {
    World* w = (World*)world;
    if (!w || !ms || !launches || !bytes) return fail(NFK_ERR_ARG, "null argument");
    int r = drain_timings(w);
    if (r) return r;
    if (w->committed) {
        Ctrl c;
        r = read_ctrl(w, &c);
        if (r) return r;
        uint64_t tb[3];
        r = read_tallies(w, tb);
        if (r) return r;
        for (int k = 0; k < 3; k++) w->kt_bytes[k] = (int64_t)tb[k];
    }
    for (int i = 0; i < KT_N; i++) {
        ms[i] = w->kt_ms[i];
        launches[i] = w->kt_n[i];
        bytes[i] = w->kt_bytes[i];
    }
    return NFK_OK;
}

int nfk_membership_stats(void* world, int64_t* n_full, int64_t* n_seg, double* host_ms_full, double* host_ms_seg) {
    World* w = (World*)world;
    if (!w || !n_full || !n_seg || !host_ms_full || !host_ms_seg) return fail(NFK_ERR_ARG, "null argument");
    *n_full = w->n_relayout_full;
    *n_seg = w->n_relayout_seg;
    *host_ms_full = w->ms_relayout_full;
    *host_ms_seg = w->ms_relayout_seg;
    return NFK_OK;
}

int nfk_reset_kernel_times(void* world) {
    World* w = (World*)world;
    if (!w) return fail(NFK_ERR_ARG, "null world");
    int r = drain_timings(w);
    if (r) return r;
    for (int i = 0; i < KT_N; i++) {
        w->kt_ms[i] = 0;
        w->kt_n[i] = 0;
    }
    if (w->committed) {
        Ctrl c;
        r = read_ctrl(w, &c);
        if (r) return r;
        // byte tallies restart from zero
        HIPCHK(hipMemset(w->d.tally, 0, (size_t)3 * kTallyN * 8 * 8));
        w->last_bytes[0] = w->last_bytes[1] = w->last_bytes[2] = 0;
    }
    return NFK_OK;
}

}  // extern "C"
