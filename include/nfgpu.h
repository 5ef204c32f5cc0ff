/* nfgpu.h — C-ABI boundary of the MI355X-native NoahGameFrame per-tick entity
 * update path (heartbeat scan -> property/record mutation -> dirty diff ->
 * scene-group fan-out).  Plain pointers and sizes only.
 *
 * Every entry point names the reference interface it replaces.  Reference
 * paths are relative to flyish/NoahGameFrame:
 *   KM  = NFComm/NFKernelPlugin/NFCKernelModule.cpp
 *   SM  = NFComm/NFKernelPlugin/NFCScheduleModule.cpp
 *   AOI = NFComm/NFKernelPlugin/NFCSceneAOIModule.cpp
 *   PR  = NFComm/NFCore/NFCProperty.cpp
 *   RC  = NFComm/NFCore/NFCRecord.cpp
 *
 * Entities are addressed by NFGUID (head, data) exactly like NFIKernelModule.
 * Outputs address entities by "object index" = creation order in this world
 * (nfk_create_objects call order), which the host maps back to NFGUID.
 */
#ifndef NFGPU_H
#define NFGPU_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (every call returns one; nothing fails silently) ---- */
#define NFK_OK 0
#define NFK_ERR_ARG (-1)       /* bad argument / schema violation */
#define NFK_ERR_HIP (-2)       /* HIP runtime error (no GPU, OOM, launch failure) */
#define NFK_ERR_STATE (-3)     /* call out of order (e.g. execute before commit) */
#define NFK_ERR_CAPACITY (-4)  /* entity / event / message capacity exceeded */
#define NFK_ERR_TOUCH (-5)     /* > NFK_MAX_TOUCH distinct properties written per entity per tick */
#define NFK_ERR_DEVICE (-6)    /* device-side error word set (bounded spin expired) */
#define NFK_ERR_NOTFOUND (-7)  /* GUID not present */

#define NFK_MAX_INT_PROPS 64
#define NFK_MAX_FLT_PROPS 64
#define NFK_MAX_OBJ_PROPS 32 /* object (NFGUID) properties; n_int + n_flt + n_obj <= NFK_MAX_PROPS */
#define NFK_MAX_PROPS 128
#define NFK_MAX_CLASSES 16 /* class id 15 is reserved (marks a free slot on the device) */
#define NFK_MAX_KINDS 32
#define NFK_MAX_OPS 8     /* ops per heartbeat program */
#define NFK_MAX_REC_OPS 4 /* record ops across all programs (distinct record columns) */
#define NFK_MAX_RECORDS 8
#define NFK_MAX_REC_ROWS 64
#define NFK_MAX_REC_COLS 16
#define NFK_MAX_TOUCH 12

/* record column types (nfk_define_record).  An object (NFGUID) column is TWO adjacent physical
 * columns: its data half (nData64) at column c and its head half (nHead64) at column c + 1, "data,
 * then head" as an entity row stores an object property.  A cell of it is named by the column of its
 * data half.  Whatever moves whole rows or column vectors carries an object cell as its two words:
 * nfk_load_record / nfk_read_record, the AddRow values of nfk_record_rows, export / import rows
 * (nfk_row_words), nfk_snapshot_objects' cells, and nfk_get_records (a half is a word). */
#define NFK_REC_INT 0
#define NFK_REC_F64 1
#define NFK_REC_OBJ_DATA 2 /* an NFGUID's data half; the next column must be NFK_REC_OBJ_HEAD */
#define NFK_REC_OBJ_HEAD 3 /* its head half; the column before must be NFK_REC_OBJ_DATA */

/* property / record visibility flags, NFIProperty::GetPublic/GetPrivate/GetUpload */
#define NFK_PUBLIC 1
#define NFK_PRIVATE 2
#define NFK_UPLOAD 4

/* Heartbeat effect ops.  A reference game registers arbitrary C++ functors
 * with NFIScheduleModule::AddSchedule (SM:218); on the device a heartbeat
 * kind carries a program of these ops, each one a Get + Set through the
 * reference's change predicates (PR:254 SetInt, PR:295 SetFloat, RC:182
 * SetInt, RC:243 SetFloat).
 *   IADD_CLAMP  dst(int) = clamp(dst + A, LO, HI)        A/LO/HI imm or prop
 *   FLERP       dst(f64) = dst + (prop[a] - dst) * f64(b) (no FMA contraction)
 *   FAFFINE     dst(f64) = dst * f64(a) + f64(b)
 *   RIADD_CLAMP record cell(int) = clamp(cell + a, b, c) for every used row
 *   RFAFFINE    record cell(f64) = cell * f64(a) + f64(b) for every used row
 *   ISET        dst(int) = A                                  A imm or prop (NFK_A_PROP)
 *   FSET        dst(f64) = A                                  A f64(a) or f64 prop (NFK_A_PROP)
 * clamp(v, lo, hi): v < lo -> lo; then v > hi -> hi.  Integer adds wrap.
 * Record ops: dst = (rec << 8) | col.
 * NFK_GUARD (property ops only): the op runs only when int property (guard & 0xFFFF), as the
 * program has left it so far, compares to 0 as NFK_GUARD_* in (guard >> 16) & 3 says — a functor's
 * `if (GetPropertyInt(self, g) > 0) SetProperty...(...)`.  With NFK_GUARD_PROP in guard it compares
 * to int property (guard >> 19) instead of 0 (both as the program has left them):
 * `if (GetPropertyInt(self, g) > GetPropertyInt(self, h)) ...`.  Without it, bits 19..31 hold a
 * signed constant K in [-4096, 4095] (NFK_GUARD_K; 0 by default) that g is compared to instead:
 * `if (GetPropertyInt(self, g) > 10) ...` (>= K and < K are > K-1 and <= K-1).
 * NFK_GUARD_CELL (with NFK_GUARD, property ops only): bits 0..15 of guard name an int record cell
 * instead of the property g, NFK_GUARD_CELL_ID(rec, row, col) = rec << 10 | row << 4 | col (13 bits;
 * rec < NFK_MAX_RECORDS, row < NFK_MAX_REC_ROWS, col < NFK_MAX_REC_COLS); bits 16..31 keep their
 * meaning (the comparison, then NFK_GUARD_PROP and the compared int property, or NFK_GUARD_K) — a
 * functor's `if (GetRecordInt(self, "SkillTable", row, "CD") <= 0) SetPropertyInt(self, ...)`.  The
 * guard reads NFCRecord::GetInt(row, col) (RC:616-635): the cell's value, or 0 when the record does
 * not use the row, as the walk has left it so far — the cell after the window's queued SetRecordInt /
 * AddRow / Remove / ClearRecord calls, then every RIADD_CLAMP on that (record, column) of a kind that
 * fired for the entity earlier in schedule-name order or of an earlier op of the same program
 * (wrapping add, clamp lo, clamp hi; applied only when the row is used, RC:182: an unused row reads
 * 0 before and after).  The record ops themselves, their write-back and events stay with the record
 * pass; they take no guard.  Guards on f64 cells and cell-to-cell comparisons are not expressible.
 * The cell is checked against the record's shape at nfk_define_kind (the record must be defined
 * first, as for a record op) and again at nfk_commit (a record may be redefined in between). */
enum {
    NFK_OP_NOP = 0,
    NFK_OP_IADD_CLAMP = 1,
    NFK_OP_FLERP = 2,
    NFK_OP_FAFFINE = 3,
    NFK_OP_RIADD_CLAMP = 4,
    NFK_OP_RFAFFINE = 5,
    NFK_OP_ISET = 6,
    NFK_OP_FSET = 7
};
#define NFK_A_PROP 1
#define NFK_LO_PROP 2
#define NFK_HI_PROP 4
#define NFK_GUARD 8
#define NFK_GUARD_CELL 16 /* with NFK_GUARD: guard bits 0..15 name an int record cell (NFK_GUARD_CELL_ID) */
#define NFK_GUARD_CELL_ID(rec, row, col) (((uint32_t)(rec) << 10) | ((uint32_t)(row) << 4) | (uint32_t)(col))
#define NFK_GUARD_GT0 0 /* g > 0 */
#define NFK_GUARD_LE0 1 /* g <= 0 */
#define NFK_GUARD_NE0 2 /* g != 0 */
#define NFK_GUARD_EQ0 3 /* g == 0 */
#define NFK_GUARD_PROP (1u << 18) /* compare g to int property guard >> 19 (< 8192) instead of 0 */
#define NFK_GUARD_K(k) (((uint32_t)(k) & 0x1FFFu) << 19) /* compare g to the constant k (no NFK_GUARD_PROP) */
#define NFK_GUARD_KVAL(guard) ((int32_t)(guard) >> 19)   /* the constant of a guard word without NFK_GUARD_PROP */
#define NFK_GUARD_KMIN (-4096)
#define NFK_GUARD_KMAX 4095

typedef struct nfk_op {
    uint8_t code;
    uint8_t flags;
    uint16_t dst;
    uint32_t guard; /* with NFK_GUARD: property id (NFK_GUARD_CELL: NFK_GUARD_CELL_ID) | NFK_GUARD_* << 16
                       [| NFK_GUARD_PROP | h << 19 or | NFK_GUARD_K(k)]; else 0 */
    int64_t a, b, c;
} nfk_op; /* 32 bytes */

typedef struct nfk_config {
    int32_t capacity;     /* max entities resident on this GPU */
    int32_t n_int;        /* int64 property columns, prop ids [0, n_int) */
    int32_t n_flt;        /* f64 property columns, prop ids [n_int, n_int+n_flt) */
    int32_t n_class;      /* classes (NFIClassModule), flags per class */
    int32_t n_kind;       /* heartbeat kinds; id order MUST equal lexical name order */
    int32_t n_rec;        /* records */
    int64_t msg_capacity; /* fan-out messages per tick (0 = 32 x capacity) */
    void* stream;         /* hipStream_t to launch on, NULL = library-owned stream */
    int32_t slack_per_256; /* free slots kept per 256 members of a scene group for arrivals
                              (SwitchScene / imports) without a full re-layout:
                              0 = default 16, < 0 = none */
    int32_t n_obj;        /* object (NFGUID) property columns, prop ids [n_int+n_flt, +n_obj):
                             16 bytes per entity (data, head), TDATA_OBJECT (NFIDataList.h) */
} nfk_config;

typedef struct nfk_summary {
    int64_t n_entities;
    int64_t n_prop_events;  /* coalesced dirty (entity, property) pairs this tick */
    int64_t n_rec_events;   /* coalesced dirty (entity, record, row, col) cells */
    int64_t n_fired;        /* heartbeat callbacks fired (NFCScheduleElement::DoHeartBeatEvent) */
    int64_t n_msgs;         /* fan-out messages (event x recipient) */
    int64_t alg_bytes_tick; /* algorithmic HBM bytes of the tick kernel this tick */
    int64_t alg_bytes_rec;  /* ... of the record kernel */
    int64_t alg_bytes_fan;  /* ... of the fan-out kernel */
    int32_t device_error;   /* nonzero: device error word */
    int32_t tick;           /* ticks executed */
} nfk_summary;

/* Device-resident outputs of the last tick (valid until the next execute).
 *
 * Outputs are TILE-STAGED: property events and fired heartbeats are grouped by 256-slot tile
 * (tile t = slots [256t, 256t+256) in (scene, group, guid) order), record events by 64-slot
 * record tile.  The i-th output of tile t sits at index t * <x>_tile_cap + i, for
 * i < <x>_base[t+1] - <x>_base[t]; its rank in the global order is <x>_base[t] + i.  Walking
 * tiles in order and each tile's entries in order gives exactly the reference order:
 *   property events  (scene, group, guid, prop)
 *   record events    (scene, group, guid, rec, ...): per record its row events (AddRow / Remove /
 *                    ClearRecord, in call order) then its cell Updates in (row, col) order;
 *                    rrc = op<<24 | rec<<16 | row<<8 | col, op 0 = Update (RECORD_EVENT_DATA::Update,
 *                    old / new the cell), 1 = Add, 2 = Del, 3 = Cover (row events: col 0, old = new = 0),
 *                    4 = Swap (nfk_swap_rows; a row event: the row field the origin row, the col
 *                    field the TARGET ROW, old = new = 0).
 *                    In the raw tiles (nfk_outputs) the word also carries the event's slot: bits
 *                    26-31 = slot - tile * rtile_slots (the record tile the event sits in), op in
 *                    bits 24-25; re_slot is NULL.  A Swap's raw word has op bits 0 and bit 23 set
 *                    (rec needs bits 16-18 only): slot << 26 | 1 << 23 | rec << 16 | origin << 8 |
 *                    target.  The nfk_read_* arrays carry the word above (a Swap: 4 << 24 | ...).
 *   fired heartbeats (scene, group, guid, kind)
 * Fan-out (GetBroadCastObject recipients): the messages of tile t (property tiles, then record
 * tiles) are one run of msg_cnt[t] recipients at msg_rcpt[msg_base[t]], in event order.  Runs
 * follow each other in tile order; when the frame's k_tick fanned out its own tiles, property
 * tile runs start at a fixed stride (msg_base[t] = t x an upper bound of a tile's messages) and
 * the record tiles' runs follow, densely or (when k_records fanned them out too) at a fixed
 * stride of their own.  Always walk tiles by msg_base / msg_cnt.  ev_moff / re_moff hold the index in msg_rcpt of the
 * event's first recipient; its recipients end where the next event of its tile begins
 * (msg_base[t] + msg_cnt[t] after the tile's last).  When k_tick fanned the property tiles out
 * (fixed-stride runs) ev_moff is NULL, and when k_records fanned the record tiles out re_moff is
 * NULL: such a tile's run holds its events' recipients in event order, the count of each the
 * recipient count of its property's / record's flags for the entity's class (private & !upload: 1,
 * the entity itself; public: the players of its group but itself; else 0).
 * Recipients are slots; slot_obj maps slot -> object index.  nfk_read_fanout returns the dense
 * CSR over [property events ++ record events].
 * nfk_read_* return the same data as dense arrays in object-index terms. */
typedef struct nfk_outputs {
    int32_t n_tiles, tile_slots;     /* property / fired tiles (tile_slots = 256) */
    int32_t n_rtiles, rtile_slots;   /* record-event tiles (rtile_slots = 64) */
    int64_t ev_tile_cap, fi_tile_cap, re_tile_cap;
    const uint32_t* ev_base;   /* [n_tiles + 1]  exclusive scan of per-tile event counts */
    const uint32_t* fi_base;   /* [n_tiles + 1] */
    const uint32_t* re_base;   /* [n_rtiles + 1] */
    const uint32_t* msg_base;  /* [n_tiles + n_rtiles + 1] first message of each tile */
    const uint32_t* msg_cnt;   /* [n_tiles + n_rtiles] messages of each tile */
    const uint32_t* ev_slot; const uint32_t* ev_pid; const uint64_t* ev_old; const uint64_t* ev_new;
    const uint32_t* ev_moff;
    const uint32_t* re_slot; /* NULL: a record event's slot is in its re_rrc word (above) */
    const uint32_t* re_rrc; const uint64_t* re_old; const uint64_t* re_new;
    const uint32_t* re_moff;
    const uint32_t* fi_slot; const uint32_t* fi_kind; const int32_t* fi_remain;
    const uint32_t* msg_rcpt; /* one run per tile (see above) */
    const int32_t* slot_obj;  /* slot -> object index */
    /* object-property events (ev_pid >= n_int + n_flt): ev_old / ev_new hold the NFGUID's data
     * half (nData64), these its head half (nHead64); other events leave them unwritten.  NULL in a
     * world without object properties. */
    const uint64_t* ev_old_h; const uint64_t* ev_new_h;
    /* Update events of object record cells (rrc op 0 on an NFK_REC_OBJ_DATA column; one event per
     * cell, never one on the head column): re_old / re_new hold the data halves, these the head
     * halves; other record events leave them unwritten.  NULL in a world without object record columns. */
    const uint64_t* re_old_h; const uint64_t* re_new_h;
} nfk_outputs;

/* ---- lifetime: NFCKernelModule ctor/Init/AfterInit (KM:17,51,1490) ---- */
int nfk_create(const nfk_config* cfg, void** out_world);
int nfk_destroy(void* world);
/* human-readable description of the last error on this thread */
const char* nfk_last_error(void);

/* ---- schema: NFIClassModule property/record definitions (KM:137-189) ---- */
int nfk_set_prop_flags(void* world, int32_t cls, const uint8_t* flags /* [n_int+n_flt+n_obj]: the object
                                                                         properties' flags behind the others */);
int nfk_define_record(void* world, int32_t rec, int32_t rows, int32_t cols,
                      const uint8_t* col_types /* [cols] NFK_REC_*: 0=int64 1=f64, 2 then 3 = an NFGUID's
                                                   data and head halves (cols counts both; a 2 without
                                                   a 3 behind it or a 3 without a 2 before it:
                                                   NFK_ERR_ARG) */,
                      const uint8_t* flags_per_class /* [n_class] */);
/* heartbeat kind program; replaces the functor passed to AddSchedule (SM:218) */
int nfk_define_kind(void* world, int32_t kind, const nfk_op* ops, int32_t n_ops);

/* ---- objects: NFCKernelModule::CreateObject (KM:101) ---- */
int nfk_create_objects(void* world, int32_t n, const int64_t* guid_head, const int64_t* guid_data,
                       const int32_t* scene, const int32_t* group, const uint8_t* cls,
                       const uint8_t* is_player);
/* creation-time property values (CreateObject's config SetProperty, KM:193-208), creation order */
int nfk_load_prop(void* world, int32_t pid, const uint64_t* bits /* [n_objects] */);
/* creation-time object property values (NFGUID head / data halves), creation order */
int nfk_load_object(void* world, int32_t pid, const int64_t* head /* [n_objects] */, const int64_t* data);
/* creation-time record contents, cells [n_objects][cols][rows] as bit patterns, used-row masks */
int nfk_load_record(void* world, int32_t rec, const uint64_t* cells, const uint64_t* used_mask);
/* build the device layout: slots sorted by (scene, group, guid) (NFCSceneInfo group maps) */
int nfk_commit(void* world);

/* ---- runtime membership (after nfk_commit) ----
 * Queued like every other between-frame call and applied at the start of the next nfk_execute,
 * before the queued SetProperty calls, so an entity's events of that frame come from its new
 * scene group.  Slots stay sorted by (scene, group, guid); only the scene groups that changed
 * are rewritten. */
/* property ids SwitchScene writes: SceneID, GroupID (int), X, Y, Z (float); -1 = not in schema */
int nfk_set_scene_props(void* world, int32_t pid_scene, int32_t pid_group, int32_t pid_x, int32_t pid_y,
                        int32_t pid_z);
/* NFCKernelModule::SwitchScene (KM:901-951): leave the group, [GroupID = 0, SceneID = scene when
 * the scene changes], X/Y/Z = (double)x/y/z, GroupID = group, join the new group */
int nfk_switch_scene(void* world, int64_t guid_head, int64_t guid_data, int32_t scene, int32_t group, float x,
                     float y, float z);
/* NFCKernelModule::DestroyObject (KM:273-308): leaves its group, its schedules go with it */
int nfk_destroy_objects(void* world, int32_t n, const int64_t* guid_head, const int64_t* guid_data);
/* objects ever created in this world (creation-order indices of the nfk_read_* arrays) */
int nfk_object_count(void* world, int32_t* n);
/* An entity's state as a ROW of 64-bit words: properties (prop id order; an object property is two
 * words, data then head), per heartbeat kind its
 * schedule (next, remain|state, start, all|interval), per record its cells [cols][places] and its
 * used-row mask.  A column's cells are in the device's PACKED order, not row order: the used rows
 * first in row order, then the unused rows in row order (a stable partition by the used mask, so the
 * mask alone maps a row to its place and back: place = popcount(used & ((1 << row) - 1)) for a used
 * row, popcount(used) + popcount(~used & ((1 << row) - 1)) for an unused one).  nfk_import_objects
 * takes rows in the same form; a producer or consumer outside export / import must (un)pack by the
 * row's mask.  Rows let a scene shard hand entities to another (SwitchScene across GPUs). */
int nfk_row_words(void* world, int32_t* words);
/* source side: write the entities' rows to rows_dev (device memory, [n][row_words]) on the world's
 * stream, and remove the entities from this world (they must not have other membership calls
 * queued in this window) */
int nfk_export_objects(void* world, int32_t n, const int64_t* guid_head, const int64_t* guid_data,
                       uint64_t* rows_dev);
/* destination side: new entities with the given rows (device memory, copied on the world's
 * stream before the call returns); also CreateObject after commit (KM:101) */
int nfk_import_objects(void* world, int32_t n, const int64_t* guid_head, const int64_t* guid_data,
                       const int32_t* scene, const int32_t* group, const uint8_t* cls, const uint8_t* is_player,
                       const uint64_t* rows_dev);
/* CreateObject after commit with creation-time property values from host memory
 * (props [n][n_int + n_flt + 2 n_obj] words: int / f64 bit patterns, then each object property's
 * data and head halves; no schedules, empty records) */
int nfk_spawn_objects(void* world, int32_t n, const int64_t* guid_head, const int64_t* guid_data,
                      const int32_t* scene, const int32_t* group, const uint8_t* cls, const uint8_t* is_player,
                      const uint64_t* props);

/* ---- property mutation: NFIKernelModule::SetPropertyInt/Float (KM:323,336) ----
 * Queued in call order, applied at the start of the next nfk_execute with the
 * reference's change predicates.  bits = int64 or f64 bit pattern. */
int nfk_set_props(void* world, int32_t n, const int64_t* guid_head, const int64_t* guid_data,
                  const int32_t* pid, const uint64_t* bits);
/* the same with the objects as nfk's object indices (creation order in this world: the ev_obj /
 * fi_obj of the outputs) for a caller that already resolved the NFGUID (the C++ plugin checks the
 * object exists, KM:325, before it queues): no lookup here; NFK_ERR_NOTFOUND for an index that is
 * not a live object */
int nfk_set_props_obj(void* world, int32_t n, const int32_t* obj, const int32_t* pid, const uint64_t* bits);

/* ---- object properties: NFIKernelModule::SetPropertyObject (KM:362) -> NFCProperty::SetObject
 * (PR:377-416): queued in call order with the other Sets, applied at the start of the next
 * nfk_execute; a value equal to the current NFGUID (both halves) changes nothing and raises no
 * event.  pid must be an object property. */
int nfk_set_objects(void* world, int32_t n, const int64_t* guid_head, const int64_t* guid_data, const int32_t* pid,
                    const int64_t* val_head, const int64_t* val_data);
/* NFIKernelModule::GetPropertyObject (KM:440): read-your-writes like nfk_get_props */
int nfk_get_objects(void* world, int32_t n, const int64_t* guid_head, const int64_t* guid_data, const int32_t* pid,
                    int64_t* val_head, int64_t* val_data);

/* ---- record mutation: NFIKernelModule::SetRecordInt/Float (KM:505, KM:545) ----
 * Queued in call order, applied at the start of the next nfk_execute through NFCRecord::SetInt /
 * SetFloat (RC:182 / RC:243): refused on a row the record does not use (RC:194); an int cell
 * changes when the value differs, an f64 cell unless |new - cur| < 0.001 (TData::operator==).
 * The cell's event of the frame runs from its value before the window's Sets to its value after
 * the frame's record programs (coalesced, dropped when the bits are equal), in (rec, row, col)
 * order beside the programs' events.  is_float (nullable: typed by the column) marks
 * SetRecordFloat calls; a call of the other type than its column writes nothing (RC:189 /
 * RC:250).  NFK_ERR_NOTFOUND for an unknown GUID, NFK_ERR_ARG for a cell outside the record. */
int nfk_set_records(void* world, int32_t n, const int64_t* guid_head, const int64_t* guid_data, const int32_t* rec,
                    const int32_t* row, const int32_t* col, const uint8_t* is_float, const uint64_t* bits);
/* NFIKernelModule::SetRecordObject -> NFCRecord::SetObject (RC:367-421): queued in call order WITH the
 * window's nfk_set_records / nfk_record_rows calls on the same (object, record), applied at the start
 * of the next frame; refused on a row unused at that point of the call order; a value whose two halves
 * both equal the cell's changes nothing and logs nothing, otherwise both halves are written together.
 * col names the data half (NFK_REC_OBJ_DATA), else NFK_ERR_ARG; the other errors as nfk_set_records.
 * nfk_set_records on either half of an object column writes nothing (a call of another type than
 * its column, RC:189), with or without is_float: no call writes one half alone.  A cell that ends the
 * frame different from its frame-start value in either half raises ONE Update event at the data
 * half's column (re_old / re_new the data halves, re_old_h / re_new_h the head halves). */
int nfk_set_record_objects(void* world, int32_t n, const int64_t* guid_head, const int64_t* guid_data,
                           const int32_t* rec, const int32_t* row, const int32_t* col, const int64_t* val_head,
                           const int64_t* val_data);

/* ---- record row operations, queued in call order with the SetRecord calls:
 *   op 1  NFCRecord::AddRow(row, values) (RC:111-180): row -1 = the first unused row (none: nothing
 *         happens); a used row is covered (Cover event, else Add); values [n][NFK_MAX_REC_COLS] words
 *         (NULL or a call without values: the record's initial values, 0), written without Update events
 *   op 2  NFCRecord::Remove(row) (RC:1086-1107): a used row's Del event, then the row is unused (its
 *         cells keep their values)
 *   op 3  NFIKernelModule::ClearRecord (KM:492) -> NFCRecord::Clear (RC:1109): Remove of every row,
 *         the last row first
 * A Set on a row is accepted or refused by the row's used state at that call (RC:194).  The row
 * events are delivered with the frame's record events (rrc op bits, see nfk_outputs).
 * NFK_ERR_NOTFOUND for an unknown GUID, NFK_ERR_ARG for a row outside the record. */
int nfk_record_rows(void* world, int32_t n, const int64_t* guid_head, const int64_t* guid_data, const int32_t* rec,
                    const int32_t* op, const int32_t* row, const uint64_t* values);

/* NFCRecord::SwapRowInfo(origin, target) (RC:1219-1253), queued in call order WITH the window's
 * nfk_set_records / nfk_set_record_objects / nfk_record_rows calls on the same (object, record) and
 * applied at the start of the next frame.  An origin unused at that point of the call order: nothing
 * happens and no event is raised.  Otherwise the two rows' cells are exchanged in every physical
 * column (both halves of an object column; whatever an unused target still holds travels too) and
 * the two used bits are exchanged, so a used origin and an unused target is a move.  origin ==
 * target on a used row changes nothing and raises the event.  One Swap event per accepted call
 * (rrc = 4 << 24 | rec << 16 | origin << 8 | target, old = new = 0; see nfk_outputs), delivered with
 * the record's other row events in call order, ahead of its cell Updates, to the recipients of any
 * event of that record; no Update is raised for a moved cell.
 * Coalescing: the frame's one Update per cell (first logged old value to last logged new one) FOLLOWS
 * THE ROW: a Swap of rows a, b re-keys every log entry made before it on a row a cell to row b and
 * the other way round.  Set(a, c) v0 -> v1 then Swap(a, b) yields Swap(a, b), Update(b, c) v0 -> v1:
 * a client that applies the frame's events in order ends in the server's state.
 * NFK_ERR_STATE before commit, NFK_ERR_NOTFOUND for an unknown GUID, NFK_ERR_ARG for a bad record or
 * a row outside [0, rows); a failed batch queues nothing. */
int nfk_swap_rows(void* world, int32_t n, const int64_t* guid_head, const int64_t* guid_data, const int32_t* rec,
                  const int32_t* row_origin, const int32_t* row_target);

/* ---- property links: record columns summed into properties ----
 * NFCPropertyModule::OnRecordPropertyEvent (NFCPropertyModule.cpp:127-149) as part of the schema: the
 * reference's game server registers it on every player's CommPropertyValue record (one row per
 * property group, one column per combat property), and it is how MAXHP and its like change at all.
 * A link (rows, col_pid[cols]) on record rec says: after EVERY record event the reference raises on
 * rec for an object, with c the event's nCol field and col_pid[c] >= 0,
 *     sum = 0 (32 bits); for i in [0, min(rows, the record's rows)): sum += (int32) GetInt(i, c)
 *     SetPropertyInt(self, col_pid[c], sum)          (stored only when different, PR:254)
 * where GetInt is 0 for a row the record does not use at that instant (RC:616-635).  nCol and the
 * instant of each event:
 *   Update (an accepted nfk_set_records call; a refused or unchanged Set raises nothing, RC:194 /
 *           RC:209): nCol the cell's column; the sum after the store.
 *   Add / Cover (nfk_record_rows op 1, RC:111-180): nCol 0; after the row's values are written and the
 *           row is used.  The values AddRow writes to OTHER columns raise nothing, so those columns'
 *           properties go stale until an event names them: the reference's behaviour and this one's.
 *   Del (op 2, and each step of op 3 ClearRecord, last row first; RC:1086-1117): nCol 0; BEFORE the
 *           used bit is cleared, so the removed row still counts.
 *   Swap (nfk_swap_rows, RC:1219-1253): nCol is the TARGET ROW's index; the sum is over column number
 *           `target`, after the exchange; nothing when `target` is no column or that column has no link.
 *           (`target` counts PHYSICAL columns, as every column of this interface does; the reference counts
 *           logical ones, which differs in a record with an object column ahead of column `target`.)
 * Each cell is truncated to int32 before the add (2^32 + 5 counts as 5).  The reference's add is a
 * signed int add; the device's wraps modulo 2^32 and the result is sign-extended to the property's 64
 * bits.  (The two agree wherever the signed add does not overflow; the wrap is pinned on the tests'
 * model only.)
 * The links run on the device in the window's call order (k_rrows; k_links stores the sums): the
 * property's value after the window is the sum at the last such event, and the frame reports ONE
 * property event, frame-start value -> final value, dropped when equal, in the entity's events in
 * property-id order with the property's own flags and recipients, like a standalone queued Set.
 * A heartbeat program that reads the property (an operand, NFK_*_PROP, a guard) sees the window's
 * value in the same frame.  nfk_execute and nfk_execute_calls both apply links.
 * A linked property belongs to its link: nfk_load_prop, nfk_spawn_objects' values and imports set its
 * stored value as before, but a queued direct Set of it (nfk_set_props / nfk_set_props_obj) is
 * NFK_ERR_ARG and the batch queues nothing — the one difference from the reference, whose
 * SetPropertyValue(..., NPG_ALL, ...) writes the property directly.  nfk_get_props, nfk_query_objects
 * and nfk_snapshot_objects see the window's queued calls on the record (read-your-writes: the list
 * is replayed on the host from the device's used mask and the one column).
 * col_pid: [the record's cols], -1 for a column without a link; NULL removes the record's link.
 * Before nfk_commit only (NFK_ERR_STATE after).  NFK_ERR_ARG: a null world, a bad record, a mode that
 * is not NFK_LINK_SUM32, rows outside [1, the record's rows], a linked column that is not NFK_REC_INT,
 * a pid that is not an int property, a pid linked from two places, a pid that is one of
 * nfk_set_scene_props' properties (in whichever order the two calls come); nothing is changed then.
 * nfk_commit is NFK_ERR_ARG when a heartbeat program writes a linked property or a record op
 * (RIADD_CLAMP / RFAFFINE) targets a linked (record, column); NFK_GUARD_CELL guards on linked cells
 * stay legal. */
#define NFK_LINK_SUM32 0
int nfk_link_record(void* world, int32_t rec, int32_t rows, const int32_t* col_pid /* [cols], -1: none; NULL: unlink */,
                    int32_t mode /* NFK_LINK_SUM32 */);

/* NFCRecord::IsUsed (RC:1209) for n (object, record) pairs: the used-row masks as the reference holds
 * them now — the device's after the last frame (one read per pair per window, cached until the next
 * nfk_execute) with this window's queued row operations replayed in call order.  What AddRow(-1)
 * would take is the lowest clear bit below the record's rows. */
int nfk_get_used_rows(void* world, int32_t n, const int64_t* guid_head, const int64_t* guid_data, const int32_t* rec,
                      uint64_t* masks);

/* ---- record reads: NFIKernelModule::GetRecordInt/Float (NFIKernelModule.h:134-135) ----
 * NFCRecord::GetInt / GetFloat (RC:616): the cell after the last frame (waits for the world's
 * stream; the used-row masks and cells of all queries in one gather) with this window's queued
 * SetRecord* and row operations on the record replayed in call order (read-your-writes); 0 for a
 * row the record does not use.  NFK_ERR_NOTFOUND / NFK_ERR_ARG as nfk_set_records. */
int nfk_get_records(void* world, int32_t n, const int64_t* guid_head, const int64_t* guid_data, const int32_t* rec,
                    const int32_t* row, const int32_t* col, uint64_t* bits);
/* NFCRecord::GetObject (RC:697-716) of object cells (col: the data half's column, else NFK_ERR_ARG):
 * read-your-writes as nfk_get_records; (0, 0), NULL_OBJECT, for a row the record does not use */
int nfk_get_record_objects(void* world, int32_t n, const int64_t* guid_head, const int64_t* guid_data,
                           const int32_t* rec, const int32_t* row, const int32_t* col, int64_t* val_head,
                           int64_t* val_data);

/* ---- property reads: NFIKernelModule::GetPropertyInt/Float (KM:401-425) ----
 * The value the reference would return now: the world's value after the last frame (waits for
 * the world's stream) with this window's queued SetProperty* / SwitchScene writes to that
 * property applied on top in call order through the change predicates (read-your-writes).  One
 * 8-byte device read per (entity, property) not read since the last nfk_execute; n > 8 reads are
 * gathered by one kernel.  NFK_ERR_NOTFOUND for an unknown GUID ("There is no object", KM:411). */
int nfk_get_props(void* world, int32_t n, const int64_t* guid_head, const int64_t* guid_data, const int32_t* pid,
                  uint64_t* bits);

/* ---- heartbeats: NFIScheduleModule (SM:218,240,245,251) ---- */
int nfk_add_schedules(void* world, int32_t n, const int64_t* guid_head, const int64_t* guid_data,
                      const int32_t* kind, const float* interval_s, const int32_t* count,
                      const int64_t* now_ms);
/* kind -1: RemoveSchedule(self, name) of a name that has no device program — it removes nothing
 * but still takes the object's remove-list key for this frame (SM:245-249) */
int nfk_remove_schedule(void* world, int64_t guid_head, int64_t guid_data, int32_t kind);
int nfk_remove_all_schedules(void* world, int64_t guid_head, int64_t guid_data);
/* the three calls above batched, in call order: op 1 = AddSchedule(self, kind, interval_s, count)
 * made at now_ms, 2 = RemoveSchedule(self, kind), 3 = RemoveSchedule(self); every GUID and kind is
 * checked before any call is queued */
int nfk_schedule_calls(void* world, int32_t n, const int32_t* op, const int64_t* guid_head, const int64_t* guid_data,
                       const int32_t* kind, const float* interval_s, const int32_t* count, const int64_t* now_ms);
/* the same by object index (see nfk_set_props_obj) */
int nfk_schedule_calls_obj(void* world, int32_t n, const int32_t* op, const int32_t* obj, const int32_t* kind,
                           const float* interval_s, const int32_t* count, const int64_t* now_ms);
/* NFIScheduleModule::ExistSchedule(self, name) (SM:276-285): the object's schedule map as the
 * reference holds it between frames — schedules present after the last frame, minus a
 * RemoveSchedule(self) queued in this window (it erases at once, SM:240); AddSchedule and
 * RemoveSchedule(self, name) take effect in the next Execute.  An unknown GUID reads 0. */
int nfk_exist_schedule(void* world, int64_t guid_head, int64_t guid_data, int32_t kind, int32_t* exists);
/* the AddSchedule calls of the last frame that created a schedule — the (object, name) had none
 * after the frame's removals, so the call's functor is the one that fires from now on (SM:108-116);
 * at most cap entries, *n = how many there are */
int nfk_read_added(void* world, int32_t cap, int32_t* n, int64_t* guid_head, int64_t* guid_data, int32_t* kind);

/* ---- per-Set chains: NFCProperty::SetInt / SetFloat fire a property's per-object callbacks
 * (NFIKernelModule::AddPropertyCallBack, NFIKernelModule.h:40) once per accepted Set (PR:254-334),
 * in the order NFCScheduleModule::Execute runs the heartbeat functors (SM:52-80).  The frame's
 * events are coalesced per (entity, property); for the int / f64 properties named here each
 * nfk_execute also logs every Set its heartbeat programs make that the change predicates accept:
 * (object, kind, op index in the kind's program, property, old, new), so a host with per-object
 * callbacks fires one per Set.  The last Set of an (entity, property) ends at the frame event's new
 * value.  n = 0 watches nothing (no extra kernel runs). */
int nfk_watch_props(void* world, int32_t n, const int32_t* pid);
/* the last nfk_execute's log in the walk's order: objects in NFGUID order, then kind (name order),
 * then op (SM:52-80) — sorted on the device; at most cap entries copied, *n = how many there are
 * (nfk_execute_calls fires nothing and keeps it) */
int nfk_read_chain(void* world, int32_t cap, int32_t* n, int32_t* obj, int32_t* kind, int32_t* op, int32_t* pid,
                   uint64_t* old_bits, uint64_t* new_bits);

/* ---- one server frame: NFCScheduleModule::Execute (SM:49) + NFCKernelModule::Execute (KM:70)
 * + NFCSceneAOIModule::OnPropertyCommonEvent/GetBroadCastObject fan-out (AOI:227,260,531).
 * Asynchronous on the world's stream. */
int nfk_execute(void* world, int64_t now_ms);
/* The calls heartbeat functors made during a frame, applied within that frame: the queued
 * SetProperty / SwitchScene / Create / Destroy / AddSchedule / RemoveSchedule calls take effect
 * and their events and recipient lists replace the outputs, with no heartbeat scan (nothing is
 * due).  In NFCScheduleModule::Execute a functor's Sets land at once (SM:65) and its
 * Add/RemoveSchedule calls are applied at the end of the same walk (SM:83-119); the plugin calls
 * this after running the frame's functors.  Asynchronous like nfk_execute. */
int nfk_execute_calls(void* world);
/* wait for everything queued on the world's stream */
int nfk_sync(void* world);
/* the hipStream_t the world launches on (nfk_config.stream, or the library's own): a caller that
 * moves the world's rows (the scene shards' RCCL transport) orders its work on it */
int nfk_get_stream(void* world, void** stream);
/* synchronise and read the counters of the last tick */
int nfk_summary_get(void* world, nfk_summary* out);
int nfk_outputs_get(void* world, nfk_outputs* out);

/* ---- host copies (synchronising) ---- */
int nfk_read_prop(void* world, int32_t pid, uint64_t* bits /* [n_objects], creation order */);
/* an object property's values, creation order */
int nfk_read_object(void* world, int32_t pid, int64_t* head /* [n_objects] */, int64_t* data);
int nfk_read_record(void* world, int32_t rec, uint64_t* cells /* [n_objects][cols][rows] */);
/* schedule table in creation order: arrays [n_kind][n_objects] */
int nfk_read_schedules(void* world, int64_t* next_ms, int32_t* remain, uint8_t* state);
/* how the device holds each schedule, same shape: 1 = a 16-byte wide record behind its 8-byte scan
 * word, 0 = the compact word alone (or no schedule).  Both forms read the same through
 * nfk_read_schedules; the form only tells what the timer scan costs. */
int nfk_read_schedule_forms(void* world, uint8_t* wide);
int nfk_read_events(void* world, int32_t* ev_obj, int32_t* ev_pid, uint64_t* ev_old, uint64_t* ev_new);
/* the head halves of the object-property events, dense like nfk_read_events (0 for other events) */
int nfk_read_events_obj(void* world, uint64_t* ev_old_h, uint64_t* ev_new_h);
int nfk_read_rec_events(void* world, int32_t* re_obj, uint32_t* re_rrc, uint64_t* re_old, uint64_t* re_new);
/* the head halves of the object-cell Update events, dense like nfk_read_rec_events (0 for other events) */
int nfk_read_rec_events_obj(void* world, uint64_t* re_old_h, uint64_t* re_new_h);
int nfk_read_fired(void* world, int32_t* fi_obj, int32_t* fi_kind, int32_t* fi_remain);
/* dense CSR over [prop events ++ record events]: msg_off[n_ev + n_re + 1], recipients as objects */
int nfk_read_fanout(void* world, uint32_t* msg_off, int32_t* msg_rcpt_obj);

/* ---- the frame's outputs for a host consumer in ONE read-back ----
 * The host plugin's delivery path (heartbeat functors, common property / record callbacks, AOI
 * recipient lists): the selected outputs of the last frame are compacted on the device into dense
 * arrays in object-index terms (slot -> object, message offsets rebased to a dense CSR over
 * [property events ++ record events]), the fired list optionally ordered by (NFGUID, kind) — the
 * order NFCScheduleModule::Execute walks mObjectScheduleMap (SM:52-80) — with a device radix sort,
 * and copied with one asynchronous copy into a pinned host buffer owned by the world.  The
 * pointers stay valid until the next nfk_execute / nfk_execute_calls / nfk_read_frame.  Arrays not
 * selected are NULL; ev_old_h / ev_new_h are NULL in a world without object properties (0 for
 * the other events). */
#define NFK_READ_FIRED 1u
#define NFK_READ_FIRED_GUID_ORDER 2u /* with NFK_READ_FIRED: (NFGUID, kind) order; else frame order */
#define NFK_READ_EVENTS 4u           /* property and record events */
#define NFK_READ_FANOUT 8u           /* with NFK_READ_EVENTS: the recipient CSR */
/* nfk_read_frame clears and fills sizeof(nfk_frame_host) bytes, and the struct may grow at its end
 * (re_old_h / re_new_h did): a caller is built against the header of the library it loads. */
typedef struct nfk_frame_host {
    int64_t n_ev, n_re, n_fi, n_msgs;
    const int32_t* ev_obj; const int32_t* ev_pid; const uint64_t* ev_old; const uint64_t* ev_new;
    const uint64_t* ev_old_h; const uint64_t* ev_new_h;
    const int32_t* re_obj; const uint32_t* re_rrc; const uint64_t* re_old; const uint64_t* re_new;
    const int32_t* fi_obj; const int32_t* fi_kind; const int32_t* fi_remain;
    const uint32_t* msg_off;   /* [n_ev + n_re + 1] */
    const int32_t* msg_rcpt;   /* [n_msgs] object indices */
    int64_t bytes;             /* bytes copied to the host */
    /* head halves of the object record cells' Update events (re_old / re_new: the data halves), 0
     * for the other record events; NULL in a world without object record columns */
    const uint64_t* re_old_h; const uint64_t* re_new_h;
} nfk_frame_host;
int nfk_read_frame(void* world, uint32_t what, nfk_frame_host* out);

/* ---- leaderboards: NFIRankRedisModule::GetRange (NFCRankRedisModule.cpp:109, a Redis
 * ZREVRANGE 0..k-1 WITH SCORES) with the property as the rank value (SetRankValue takes a double):
 * the k entities of this world with the highest score, ties by NFGUID::ToString() descending
 * (Redis orders equal scores by member, reversed).  Across scene shards, every rank's top k is
 * gathered and merged with the same order (noahgameframe_amd/shard.py rank_top_global). */
int nfk_rank_top(void* world, int32_t pid, int32_t k, int32_t* n_out, int64_t* guid_head, int64_t* guid_data,
                 double* score);

/* ---- scene queries: NFCKernelModule::GetObjectByProperty (KM:1357-1405), the GetGroupObjectList
 * overloads (KM:1169-1294), GetSceneOnLineList / GetSceneOnLineCount (KM:1042-1102), GetOnLineCount
 * (KM:1015).  A batch of n_q <= NFK_MAX_QUERIES queries is answered in one call (more: NFK_ERR_ARG).  A query is a filtered, order-preserving
 * compaction over the slot range of one scene (NFK_Q_ALL_GROUPS: its groups in group-id order, the
 * std::map walk of NFCSceneInfo First / Next) or of one scene group:
 *   who        NFK_Q_PLAYERS: the group's mxPlayerList, NFK_Q_OTHERS: its mxOtherList.  "Players then
 *              others" (GetGroupObjectList(scene, group, list), KM:1169) is two queries of one batch
 *   cls_mask   bit c: objects of class c qualify (the classes that have the property, FindProperty
 *              KM:1365; the strClassName overloads, KM:1231)
 *   pid        the property compared, or -1: a pure membership list
 *   mode       NFK_Q_INT_EQ32 (int property): (int64_t)(int32_t)property == value — the reference reads
 *              the property into an int (KM:1372) and compares it with the argument's NFINT64, so a
 *              property of 2^32 + 5 matches the argument 5 and a property of 5 does not match 2^32 + 5;
 *              NFK_Q_OBJ_EQ (object property): both NFGUID halves equal value (data) / value_head (KM:1391)
 *   skip_obj   an object index left out (noSelf, KM:1270), or -1
 * The result is owned by the world, in pinned host memory, valid until the next nfk_query_objects /
 * nfk_execute / nfk_execute_calls: off[n_q + 1], obj[off[n_q]] (object indices, as ev_obj) with query
 * q's hits at obj[off[q] .. off[q + 1]) in the reference's order — group id ascending, then NFGUID
 * ascending (NFGUID::operator<) — and exists[n_q]: 0 for a scene (or scene group) that never held an
 * object of this world (the reference returns false / 0), whose list is empty; a group exists from its
 * first member on and stays when it is emptied (NFCSceneGroupInfo until ReleaseGroupScene).
 * An object is a player or an "other" by what nfk_create_objects / nfk_spawn_objects said (its class);
 * NFCKernelModule::SwitchScene itself moves every object between the groups' PLAYER lists (KM:929, 945
 * pass bPlayer = true, so an NPC it moves stays listed in its old group): that is not reproduced.
 * The answer is the reference's NOW: the device state after the last frame (the call waits for the
 * world's stream like nfk_rank_top, queues nothing and changes nothing a frame reads) with this
 * window's queued calls on top, by the read-your-writes rule of nfk_get_props — objects whose
 * membership changed in the window (SwitchScene, DestroyObject, spawn / import) or that have a queued
 * Set of the queried property are taken out of the device's hits, re-evaluated on the host and merged
 * back in order.  NFK_ERR_ARG: a bad pid / mode / who, or a mode that does not fit the property's
 * type; NFK_ERR_STATE before nfk_commit. */
#define NFK_MAX_QUERIES 4096 /* queries of one nfk_query_objects batch */
#define NFK_Q_PLAYERS 0
#define NFK_Q_OTHERS 1
#define NFK_Q_ALL_GROUPS 1u /* nfk_query::flags: every group of the scene (group is ignored) */
#define NFK_Q_INT_EQ32 0
#define NFK_Q_OBJ_EQ 1
typedef struct nfk_query {
    int32_t scene, group;
    uint32_t flags;    /* NFK_Q_ALL_GROUPS */
    int32_t who;       /* NFK_Q_PLAYERS / NFK_Q_OTHERS */
    uint32_t cls_mask; /* 16 bits, one per class id */
    int32_t pid;       /* -1: no property test */
    int32_t mode;      /* NFK_Q_INT_EQ32 / NFK_Q_OBJ_EQ (with pid >= 0) */
    int32_t skip_obj;  /* -1: none */
    int64_t value;      /* the int argument, or the NFGUID's data half (nData64) */
    int64_t value_head; /* the NFGUID's head half (nHead64) */
} nfk_query; /* 48 bytes */
typedef struct nfk_query_result {
    const uint32_t* off;   /* [n_q + 1] */
    const int32_t* obj;    /* [off[n_q]] */
    const uint8_t* exists; /* [n_q] */
    /* the launches' device time in ms (0 unless nfk_set_profiling is on) and the bytes read back */
    double kernel_ms;
    int64_t bytes;
} nfk_query_result;
int nfk_query_objects(void* world, int32_t n_q, const nfk_query* q, nfk_query_result* out);
/* GetSceneOnLineCount(scene) (KM:1083; group < 0) / GetSceneOnLineCount(scene, group) (KM:1090) /
 * GetOnLineCount (KM:1015; scene < 0: every scene): the players now, from the host's segment
 * bookkeeping corrected by the window's membership calls — no launch, no device read */
int nfk_online_count(void* world, int32_t scene, int32_t group, int32_t* n);

/* ---- view changes: the group lists NFCSceneAOIModule::OnGroupEvent / OnSceneEvent /
 * OnClassCommonEvent (AOI:292-529) read inside every SwitchScene, CreateObject and DestroyObject, each
 * as of ITS call.  The window is everything queued since the last nfk_execute / nfk_execute_calls.
 * nfk_switch_scene, nfk_destroy_objects, nfk_spawn_objects, nfk_import_objects and nfk_export_objects
 * append one log entry per object whose (scene, group) or existence changes, in call order (a batch call
 * in array order; a switch that changes neither scene nor group logs nothing); the log is cleared where
 * the window's membership is applied.  Entry i expands to 0-4 visits (why, scene, group), the groups the
 * reference reads, in its order:
 *   NFK_VC_SWITCH inside a scene (KM:943):  GROUP_LEAVE (s, g0) if g0 > 0, GROUP_ENTER (s, g1) if g1 > 0
 *   NFK_VC_SWITCH s0 -> s1 (KM:932-943):    GROUP_LEAVE (s0, g0) if g0 > 0, SCENE_LEAVE (s0, 0),
 *                                           SCENE_ENTER (s1, 0), GROUP_ENTER (s1, g1) if g1 > 0
 *   NFK_VC_DESTROY:                         DESTROY (s, g) when s > 0 (AOI:294-327)
 *   NFK_VC_CREATE (spawn / import):         SCENE_ENTER (s, 0) when s != 0, GROUP_ENTER (s, g) if g > 0
 *   NFK_VC_EXPORT:                          GROUP_LEAVE (s0, g0) if g0 > 0, SCENE_LEAVE (s0, 0)
 * A visit answers two lists of object indices, the group's players and its other objects, each in
 * NFGUID order (GetGroupObjectList's "players then others", KM:1169-1199), both without entry i's own
 * object, as the group stood at instant i: the frame-start membership with entries 0 .. i-1 applied.  A
 * switching or destroyed object is out of its old group at its own instant and not yet in its new one
 * (KM:929 precedes 945, KM:291 precedes 294); a created one is in its group (KM:146) and skipped as
 * self.  Player / other follows the class, as nfk_query_objects documents.  A group nobody has been in
 * gives two empty lists.
 * The result is owned by the world, in pinned host memory, valid until the next nfk_view_changes /
 * nfk_execute / nfk_execute_calls.  Calling it twice in a window gives the same answer plus whatever
 * was queued in between.  It waits for the world's stream, queues nothing and changes nothing a frame
 * reads.  A visit whose group has more than NFK_VC_STINT_CAP membership intervals begun in the window
 * is answered on the host (n_host counts them).  NFK_ERR_STATE before nfk_commit; NFK_ERR_CAPACITY when
 * the BOUND of the window's list entries (per visit: the members of its group's segment plus the
 * group's intervals of the window) exceeds NFK_VC_MAX_ENTRIES. */
#define NFK_VC_SWITCH 0
#define NFK_VC_DESTROY 1
#define NFK_VC_CREATE 2
#define NFK_VC_EXPORT 3
#define NFK_VC_GROUP_LEAVE 0
#define NFK_VC_GROUP_ENTER 1
#define NFK_VC_SCENE_LEAVE 2
#define NFK_VC_SCENE_ENTER 3
#define NFK_VC_WHY_DESTROY 4
#define NFK_VC_STINT_CAP 256           /* a group's intervals of one window merged on the device */
#define NFK_VC_MAX_ENTRIES (1 << 24)   /* bound of one window's list entries (64 MiB read back) */
typedef struct nfk_vc_entry {
    int32_t obj, kind; /* object index (as ev_obj), NFK_VC_SWITCH / DESTROY / CREATE / EXPORT */
    int32_t from_scene, from_group, to_scene, to_group; /* (CREATE: from = 0, 0; DESTROY / EXPORT: to = 0, 0) */
} nfk_vc_entry; /* 24 bytes */
typedef struct nfk_vc_visit {
    int32_t why, scene, group; /* NFK_VC_GROUP_LEAVE ... NFK_VC_WHY_DESTROY */
} nfk_vc_visit; /* 12 bytes */
typedef struct nfk_view_changes_result {
    int32_t n_calls, n_visits;
    const nfk_vc_entry* log;     /* [n_calls] */
    const uint32_t* call_visit;  /* [n_calls + 1]: entry i's visits are [call_visit[i], call_visit[i + 1]) */
    const nfk_vc_visit* visit;   /* [n_visits] */
    const uint32_t* visit_off;   /* [2 * n_visits + 1]: players of visit v at obj[off[2v], off[2v + 1]),
                                    others at obj[off[2v + 1], off[2v + 2]) */
    const int32_t* obj;          /* [visit_off[2 * n_visits]] */
    double kernel_ms;            /* the launches' device time in ms (0 unless nfk_set_profiling is on) */
    int64_t bytes;               /* read back from the device */
    int32_t n_host;              /* visits answered on the host (groups past NFK_VC_STINT_CAP) */
    int32_t n_tiles;             /* 256-slot tiles of the device batch */
} nfk_view_changes_result;
int nfk_view_changes(void* world, nfk_view_changes_result* out);

/* ---- record finds: NFCRecord::FindInt / FindFloat / FindRowByColValue (RC:778-910) ----
 * n (object, record, column, argument) finds answered in one call: masks[i] has bit r set when row
 * r of the record is used and its cell in column col[i] equals bits[i] under the column's type —
 * an int column by 64-bit equality (RC:850; 5 does not match 2^32 + 5, unlike NFK_Q_INT_EQ32), an
 * f64 column by the C == on doubles (RC:892: -0.0 finds 0.0, a NaN cell is never found, not by a
 * NaN argument either).  The reference's list (rows ascending) and count follow from the bits; a
 * Remove leaves a cell's value behind (RC:1086-1107), so only used rows are compared.
 * One launch for the batch (k_find_rows: a lane per row, the used rows' dense run of the column's
 * vector read, one ballot per query) on the world's stream, the masks back in one pinned copy; the
 * staging buffers are the world's and grow on demand.  The answer is the reference's NOW, by the
 * read-your-writes rule of nfk_get_records: a find whose (object, record) has queued SetRecord* /
 * AddRow / Remove / ClearRecord calls in this window is answered on the host — the device's mask
 * and column, the queued calls replayed in call order, then the comparison.  An object that
 * entered in this window is read from the import buffer.  Queues nothing, changes nothing.
 * nfk_find_rows_obj takes object indices (nfk_query_objects' hits, ev_obj) instead of NFGUIDs.
 * NFK_ERR_ARG: a null argument, n < 0, a bad record or column; NFK_ERR_STATE before nfk_commit;
 * NFK_ERR_NOTFOUND: an unknown (or destroyed) object.  The caller tests the column's type against
 * its argument's (the reference returns -1 there, RC:837 / RC:880); the bits are compared as the
 * column's type says. */
int nfk_find_rows(void* world, int32_t n, const int64_t* guid_head, const int64_t* guid_data, const int32_t* rec,
                  const int32_t* col, const uint64_t* bits, uint64_t* masks);
int nfk_find_rows_obj(void* world, int32_t n, const int32_t* obj, const int32_t* rec, const int32_t* col,
                      const uint64_t* bits, uint64_t* masks);
/* NFCRecord::FindObject (RC:957-987): bit r of masks[i] is set when row r is used and BOTH halves of
 * its cell in the object column col[i] (the data half's column, else NFK_ERR_ARG) equal the argument.
 * A find of NULL_OBJECT (0, 0) finds the used rows that hold it, as the reference does.  One launch
 * (k_find_objects: nfk_find_rows' shape, the head word read rows words behind the data word); the
 * read-your-writes rule, the import buffer, the errors and nfk_find_stats are nfk_find_rows'.
 * nfk_find_rows on either half of an object column is NFK_ERR_ARG. */
int nfk_find_objects(void* world, int32_t n, const int64_t* guid_head, const int64_t* guid_data, const int32_t* rec,
                     const int32_t* col, const int64_t* val_head, const int64_t* val_data, uint64_t* masks);
int nfk_find_objects_obj(void* world, int32_t n, const int32_t* obj, const int32_t* rec, const int32_t* col,
                         const int64_t* val_head, const int64_t* val_data, uint64_t* masks);
/* the last nfk_find_rows / nfk_find_objects (or their _obj forms) of the world: its launch's device
 * time in ms (0 unless nfk_set_profiling is on), the bytes read back and the finds answered on the
 * host (each pointer may be null) */
int nfk_find_stats(void* world, double* kernel_ms, int64_t* bytes, int32_t* n_host);

/* ---- resource calls: NFCPropertyModule's FullHPMP / AddHP / ConsumeHP / EnoughHP / AddMoney ...
 * (PM:215-472), each a read-modify-write of one int property dst, some against a second one, bound.
 * A batch of n calls applies in array order and returns, and leaves the world, exactly as this loop
 * over the entry points above would: cur = nfk_get_props(o, dst), max = nfk_get_props(o, bound),
 * the op's rule, nfk_set_props(o, dst, new) where the reference calls SetPropertyInt.  So a call
 * sees the device's values, the window's queued Sets and linked-record calls, the objects spawned
 * or imported in this window and every earlier call of its batch.  value is signed 64-bit; add and
 * subtract wrap (signed overflow is undefined in the reference).
 *   op                   reference                   rule (v = value[i])
 *   NFK_ADJ_GAIN_ALIVE   AddHP PM:232                v <= 0: ret 0, nothing.  Else ret 1, and if
 *                                                    cur > 0: n = cur + v, n = max if n > max, Set(n)
 *   NFK_ADJ_GAIN_CAP     AddMP / AddSP PM:281, 340   v <= 0: ret 0.  Else n = cur + v capped at max,
 *                                                    Set(n), ret 1 (no cur > 0 test)
 *   NFK_ADJ_GAIN         AddMoney / AddDiamond       v <= 0: ret 0.  Else Set(cur + v), ret 0 (the
 *                        PM:386, 430                 reference returns false on both branches)
 *   NFK_ADJ_SPEND_ALIVE  ConsumeHP/MP/SP             cur > 0 && cur - v >= 0: Set(cur - v), ret 1.
 *                        PM:267, 302, 361            Else ret 0.  v is not tested (v < 0 raises dst)
 *   NFK_ADJ_SPEND        ConsumeMoney / Diamond      v <= 0: ret 0.  Else n = cur - v; n >= 0:
 *                        PM:400, 444                 Set(n), ret 1; else ret 0
 *   NFK_ADJ_ENOUGH       every Enough* PM:256...     ret = cur > 0 && cur - v >= 0.  Never Sets
 *   NFK_ADJ_FILL         FullSP, each half of        max > 0: Set(max), ret 1.  Else ret 0.  v ignored
 *                        FullHPMP PM:215, 327
 * ret[i]: bit 0 the reference's return value, bit 1 a Set was queued (a Set of the value the
 * property already holds is queued too, as the reference still calls SetPropertyInt; the frame's
 * change predicate drops it).  The accepted Sets join the window's SetProperty stream in batch
 * order, exactly as nfk_set_props' would.
 * dst is an int property nfk_set_props accepts (a linked property or an object property is refused
 * with that call's NFK_ERR_ARG); bound is an int property (a linked one too) for GAIN_ALIVE,
 * GAIN_CAP and FILL and -1 for the four ops that read no maximum, else NFK_ERR_ARG.  An unknown or
 * destroyed object is NFK_ERR_NOTFOUND; before nfk_commit NFK_ERR_STATE.  The whole batch is
 * checked before anything is queued.
 * One launch for the batch (k_adjust, the world's stream) and one pinned copy back: the host groups
 * the calls stably by (object, dst), a group's first lane walks it with cur in a register.  A call
 * whose (object, dst), (object, bound) or object has pending state in this window — a queued Set,
 * a linked bound whose record has queued calls, an object spawned or imported in the window — or
 * whose bound is another call's dst in the batch, is answered on the host through nfk_get_props'
 * code, with the other calls on its dst (and on its bound).  After an adjust batch its (object, dst)
 * pairs have queued Sets, so later batches of the window on them run on the host.
 * nfk_adjust_props_obj takes object indices (nfk_query_objects' hits, ev_obj) instead of NFGUIDs. */
#define NFK_ADJ_GAIN_ALIVE 0
#define NFK_ADJ_GAIN_CAP 1
#define NFK_ADJ_GAIN 2
#define NFK_ADJ_SPEND_ALIVE 3
#define NFK_ADJ_SPEND 4
#define NFK_ADJ_ENOUGH 5
#define NFK_ADJ_FILL 6
#define NFK_ADJ_RET 1    /* ret bit 0: the reference's return value */
#define NFK_ADJ_SET 2    /* ret bit 1: a Set was queued */
int nfk_adjust_props(void* world, int32_t n, const int64_t* guid_head, const int64_t* guid_data, const uint8_t* op,
                     const int32_t* dst, const int32_t* bound, const int64_t* value, uint8_t* ret);
int nfk_adjust_props_obj(void* world, int32_t n, const int32_t* obj, const uint8_t* op, const int32_t* dst,
                         const int32_t* bound, const int64_t* value, uint8_t* ret);
/* the last nfk_adjust_props / nfk_adjust_props_obj of the world */
typedef struct nfk_adjust_stats_t {
    double kernel_ms;   /* the launch's device time (0 unless nfk_set_profiling is on) */
    int64_t bytes;      /* read back from the device */
    int32_t n_dev;      /* calls answered by k_adjust */
    int32_t n_host;     /* calls answered on the host */
    int32_t n_set;      /* Sets queued */
    int32_t pad;
} nfk_adjust_stats_t;
int nfk_adjust_stats(void* world, nfk_adjust_stats_t* out);

/* ---- enter snapshots: the payloads of NFCGameServerNet_ServerModule::OnPropertyEnter (:271-393) and
 * OnRecordEnter (:395-554), which NFCSceneAOIModule::OnGroupEvent / OnSceneEvent / OnClassCommonEvent
 * hand to the recipients of an object that comes into view ----
 * n (object, view) requests answered in one call.  NFK_VIEW_PRIVATE (the recipient is the object
 * itself) takes the entries whose flags have NFK_PRIVATE, NFK_VIEW_PUBLIC those with NFK_PUBLIC; an
 * entry with both is in both views, NFK_UPLOAD plays no part.  The flags are Tables::pflags[class][pid]
 * (nfk_set_prop_flags: all three property types) and the records' flags_per_class.
 * Properties: the walk's order (nfk_set_snapshot_order: the reference walks a std::map by name; the
 * default is id order); a property is an entry only when NFCProperty::Changed() holds, that is
 * !IsNullValue() (NFIDataList.h:160-221): an int != 0; an f64 v with v > 0.001 || v < -0.001 (0.001,
 * -0.001, -0.0, denormals and NaN are not entries); an object with either half non-zero.
 * Records: every record in view, in the walk's order, is one entry, also when it uses no row; its
 * cells are those of its used rows, no null test (a cell of an unused row is never in it).
 * Requests may repeat an object and come in any order; results are in request order.  The runs
 * answered by the kernels (k_snap, k_snap_scan, k_snap_cells on the world's stream, one pinned
 * copy back) are dense in request order; a request whose object has a queued SetProperty* /
 * SetPropertyObject call (SwitchScene's among them) or a queued record call in this window, or that
 * entered in this window (spawn / import), is answered on the host through the code of nfk_get_props /
 * nfk_get_objects / nfk_get_records, with the same predicates, and its runs are appended behind the
 * kernels' — hence (first, count) pairs, not a CSR.  The answer is the reference's NOW; the call
 * waits for the world's stream, queues nothing and changes nothing a frame reads.
 * NFK_ERR_ARG: a null argument (a null world's message says so), n < 0, a view that is neither
 * constant; NFK_ERR_NOTFOUND: an unknown or destroyed object; NFK_ERR_STATE before nfk_commit;
 * NFK_ERR_CAPACITY: the BOUND of the batch's property entries, record entries or cells does not fit
 * 32 bits — every property in view taken as an entry, every row of every record in view as used
 * (rows x cols cells), summed over the requests on the host before anything is allocated or
 * launched, so the device's 32-bit counts cannot wrap; a batch whose real totals would fit is
 * refused with its bound — or n > INT32_MAX / 3 (tested before an array is read).  NFK_ERR_DEVICE:
 * the kernels counted more than that bound, an invariant check no batch can reach.  n == 0 launches
 * nothing.  After any of these the world answers the next call. */
#define NFK_VIEW_PUBLIC 1u
#define NFK_VIEW_PRIVATE 2u
typedef struct nfk_snapshot { /* world-owned pinned memory, valid until the next nfk_snapshot_* /
                                 nfk_execute / nfk_execute_calls */
    const uint32_t *p_first, *p_count; /* [n] request i's property entries: p_pid/p_bits/p_head[p_first[i] .. +p_count[i]) */
    const int32_t* p_pid;              /* walk order */
    const uint64_t* p_bits;            /* the word; an object property's data half */
    const uint64_t* p_head;            /* an object property's head half, 0 otherwise; NULL when n_obj == 0 */
    const uint32_t *r_first, *r_count; /* [n] request i's record entries */
    const int32_t* r_rec;
    const uint64_t* r_used;            /* used-row mask (may be 0) */
    const uint32_t* r_cell;            /* first cell of the entry in cells[] */
    const uint64_t* cells;             /* entry e: cells[r_cell[e] + c * popcount(r_used[e]) + k] = column c of
                                          the k-th used row (column-major, as the device holds it) */
    double kernel_ms;                  /* the launches' device time (0 unless nfk_set_profiling is on) */
    int64_t bytes;                     /* read back */
    int32_t n_host;                    /* requests answered on the host */
} nfk_snapshot;
int nfk_snapshot_objects(void* world, int32_t n, const int64_t* guid_head, const int64_t* guid_data,
                         const uint8_t* view, nfk_snapshot* out);
/* by object index (nfk_query_objects' hits, ev_obj) instead of NFGUID */
int nfk_snapshot_objects_obj(void* world, int32_t n, const int32_t* obj, const uint8_t* view, nfk_snapshot* out);
/* the walk's order: prop_order a permutation of the property ids [0, n_int + n_flt + n_obj),
 * rec_order one of the record ids [0, n_rec); NULL: id order.  The world holds no names, so the
 * caller gives the byte-wise name order of the reference's NFMapEx walk.  Before or after
 * nfk_commit; NFK_ERR_ARG for anything that is not a permutation (nothing is changed then). */
int nfk_set_snapshot_order(void* world, const int32_t* prop_order, const int32_t* rec_order);

/* ---- schema specialisation ----
 * At nfk_commit k_tick is compiled for the world's schema (its heartbeat programs as straight-line
 * code, its working set and event tables as constants) with hipRTC for gfx950, from the same
 * device source as the library's generic k_tick; the results are bit-identical.  NFGPU_JIT=0 (or
 * a failed compile) keeps the generic kernel. */
/* whether this world's frames run the specialised k_tick; msg: its kernel name or why not */
int nfk_jit_status(void* world, int32_t* on, char* msg, int32_t cap);
/* the specialisation for a schema without a world or a GPU: the generated policy source, and with
 * compile != 0 the hipRTC build for gfx950 (*ok = 1 on success, msg = the kernel's name, the compiler
 * log, and after it the compiler's resource remarks of each kernel, one "name: value" per line after
 * its "Function Name: ..." line — VGPRs, SGPRs Spill, VGPRs Spill, ScratchSize [bytes/lane], ...:
 * the preview compiles with -Rpass-analysis=kernel-resource-usage, a world's commit does not) */
int nfk_jit_preview(int32_t n_int, int32_t n_flt, int32_t n_class, int32_t n_kind,
                    const uint8_t* prop_flags /* [n_class][n_int + n_flt] */,
                    const nfk_op* ops /* [n_kind][NFK_MAX_OPS] */, const int32_t* n_ops /* [n_kind] */,
                    int32_t compile, int32_t* ok, char* src, int32_t src_cap, char* msg, int32_t msg_cap);
/* the same for a schema whose programs guard on record cells (NFK_GUARD_CELL): the policy holds the
 * records' shapes as literals (col_types [n_rec][NFK_MAX_REC_COLS], nullable: all int64) */
int nfk_jit_preview_rec(int32_t n_int, int32_t n_flt, int32_t n_class, int32_t n_kind, const uint8_t* prop_flags,
                        const nfk_op* ops, const int32_t* n_ops, int32_t n_rec, const int32_t* rec_rows /* [n_rec] */,
                        const int32_t* rec_cols /* [n_rec] */, const uint8_t* col_types, int32_t compile, int32_t* ok,
                        char* src, int32_t src_cap, char* msg, int32_t msg_cap);

/* ---- measurement ---- */
int nfk_set_profiling(void* world, int32_t on);
/* accumulated device time (ms), launch count and algorithmic bytes per kernel:
 * 0 k_tick, 1 k_records, 2 k_fanout, 3 aux (queued host calls), 4 k_scan_tiles,
 * 5 membership changes (k_seg_lists / k_pack / k_unpack / k_meta), 6 k_chain (the per-Set log of
 * the watched properties, nfk_watch_props) */
#define NFK_N_KERNEL_TIMERS 7
int nfk_kernel_times(void* world, double* ms /* [7] */, int64_t* launches /* [7] */, int64_t* bytes /* [7] */);
/* membership changes applied so far: windows that rewrote only the changed scene-group segments
 * (n_seg) or rebuilt the segment table (n_full: a new scene group, or a segment out of slack), and
 * the host milliseconds nfk_execute spent planning them (the device part is timer 5 above) */
int nfk_membership_stats(void* world, int64_t* n_full, int64_t* n_seg, double* host_ms_full, double* host_ms_seg);
int nfk_reset_kernel_times(void* world);

#ifdef __cplusplus
}
#endif
#endif
