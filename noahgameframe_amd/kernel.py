"""Python host mirror of the reference plugin API over the C-ABI (include/nfgpu.h).

`NFKernelModule` keeps the names, argument meaning and failure behaviour of the
reference's NFIKernelModule / NFIScheduleModule calls on the tick path
(NFComm/NFPluginModule/NFIKernelModule.h, NFIScheduleModule.h):
CreateObject, SetPropertyInt/Float, GetPropertyInt/Float, AddSchedule,
RemoveSchedule, Execute.  The compute runs in libnfgpu.so (hand-written HIP
for gfx950).  There is no CPU fallback: constructing a module without the
library or without a GPU raises.
"""
import ctypes
import os

import numpy as np

from . import workload as wl

NFK_MAX_OPS = 8  # include/nfgpu.h: ops per heartbeat program

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NFGPU_LIB") or os.path.join(_HERE, "libnfgpu.so")  # (NFGPU_LIB: A/B timing of library builds)

NFK_OK = 0
_ERRS = {-1: "NFK_ERR_ARG", -2: "NFK_ERR_HIP", -3: "NFK_ERR_STATE", -4: "NFK_ERR_CAPACITY",
         -5: "NFK_ERR_TOUCH", -6: "NFK_ERR_DEVICE", -7: "NFK_ERR_NOTFOUND"}


class NFKError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{_ERRS.get(code, code)}: {msg}")
        self.code = code


class Config(ctypes.Structure):
    _fields_ = [("capacity", ctypes.c_int32), ("n_int", ctypes.c_int32), ("n_flt", ctypes.c_int32),
                ("n_class", ctypes.c_int32), ("n_kind", ctypes.c_int32), ("n_rec", ctypes.c_int32),
                ("msg_capacity", ctypes.c_int64), ("stream", ctypes.c_void_p), ("slack_per_256", ctypes.c_int32),
                ("n_obj", ctypes.c_int32)]


class Summary(ctypes.Structure):
    _fields_ = [("n_entities", ctypes.c_int64), ("n_prop_events", ctypes.c_int64),
                ("n_rec_events", ctypes.c_int64), ("n_fired", ctypes.c_int64), ("n_msgs", ctypes.c_int64),
                ("alg_bytes_tick", ctypes.c_int64), ("alg_bytes_rec", ctypes.c_int64),
                ("alg_bytes_fan", ctypes.c_int64), ("device_error", ctypes.c_int32), ("tick", ctypes.c_int32)]


class Outputs(ctypes.Structure):
    """nfk_outputs: tile-staged device outputs of the last frame (see include/nfgpu.h)."""
    _fields_ = ([("n_tiles", ctypes.c_int32), ("tile_slots", ctypes.c_int32), ("n_rtiles", ctypes.c_int32),
                 ("rtile_slots", ctypes.c_int32), ("ev_tile_cap", ctypes.c_int64), ("fi_tile_cap", ctypes.c_int64),
                 ("re_tile_cap", ctypes.c_int64)] +
                [(n, ctypes.c_void_p) for n in
                 ["ev_base", "fi_base", "re_base", "msg_base", "msg_cnt", "ev_slot", "ev_pid", "ev_old", "ev_new", "ev_moff",
                  "re_slot", "re_rrc", "re_old", "re_new", "re_moff", "fi_slot", "fi_kind", "fi_remain",
                  "msg_rcpt", "slot_obj", "ev_old_h", "ev_new_h", "re_old_h", "re_new_h"]])


class AdjustStats(ctypes.Structure):
    """nfk_adjust_stats_t"""
    _fields_ = [("kernel_ms", ctypes.c_double), ("bytes", ctypes.c_int64), ("n_dev", ctypes.c_int32),
                ("n_host", ctypes.c_int32), ("n_set", ctypes.c_int32), ("pad", ctypes.c_int32)]


class Query(ctypes.Structure):
    """nfk_query (include/nfgpu.h): one scene query of a nfk_query_objects batch."""
    _fields_ = [("scene", ctypes.c_int32), ("group", ctypes.c_int32), ("flags", ctypes.c_uint32),
                ("who", ctypes.c_int32), ("cls_mask", ctypes.c_uint32), ("pid", ctypes.c_int32),
                ("mode", ctypes.c_int32), ("skip_obj", ctypes.c_int32), ("value", ctypes.c_int64),
                ("value_head", ctypes.c_int64)]


class QueryResult(ctypes.Structure):
    _fields_ = [("off", ctypes.POINTER(ctypes.c_uint32)), ("obj", ctypes.POINTER(ctypes.c_int32)),
                ("exists", ctypes.POINTER(ctypes.c_uint8)), ("kernel_ms", ctypes.c_double),
                ("bytes", ctypes.c_int64)]


class ViewChanges(ctypes.Structure):
    """nfk_view_changes_result (include/nfgpu.h)"""
    _fields_ = [("n_calls", ctypes.c_int32), ("n_visits", ctypes.c_int32), ("log", ctypes.POINTER(ctypes.c_int32)),
                ("call_visit", ctypes.POINTER(ctypes.c_uint32)), ("visit", ctypes.POINTER(ctypes.c_int32)),
                ("visit_off", ctypes.POINTER(ctypes.c_uint32)), ("obj", ctypes.POINTER(ctypes.c_int32)),
                ("kernel_ms", ctypes.c_double), ("bytes", ctypes.c_int64), ("n_host", ctypes.c_int32),
                ("n_tiles", ctypes.c_int32)]


# nfk_vc_entry::kind, nfk_vc_visit::why
VC_SWITCH, VC_DESTROY, VC_CREATE, VC_EXPORT = 0, 1, 2, 3
VC_GROUP_LEAVE, VC_GROUP_ENTER, VC_SCENE_LEAVE, VC_SCENE_ENTER, VC_WHY_DESTROY = 0, 1, 2, 3, 4
VC_STINT_CAP = 256   # NFK_VC_STINT_CAP


class Snapshot(ctypes.Structure):
    _U32, _I32, _U64 = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint64)
    _fields_ = [("p_first", _U32), ("p_count", _U32), ("p_pid", _I32), ("p_bits", _U64), ("p_head", _U64),
                ("r_first", _U32), ("r_count", _U32), ("r_rec", _I32), ("r_used", _U64), ("r_cell", _U32),
                ("cells", _U64), ("kernel_ms", ctypes.c_double), ("bytes", ctypes.c_int64),
                ("n_host", ctypes.c_int32)]


VIEW_PUBLIC, VIEW_PRIVATE = 1, 2
# record column types (NFK_REC_*): an object (NFGUID) column is a data half and its head half behind it
REC_INT, REC_F64, REC_OBJ_DATA, REC_OBJ_HEAD = 0, 1, 2, 3
REC_OBJECT = (REC_OBJ_DATA, REC_OBJ_HEAD)   # col_types.extend(REC_OBJECT): one logical object column
MAX_RECORDS = 8   # NFK_MAX_RECORDS
LINK_SUM32 = 0    # NFK_LINK_SUM32 (nfk_link_record's mode)
Q_PLAYERS, Q_OTHERS = 0, 1
Q_ALL_GROUPS = 1
Q_INT_EQ32, Q_OBJ_EQ = 0, 1
# nfk_adjust_props' ops (NFK_ADJ_*) and result bits
ADJ_GAIN_ALIVE, ADJ_GAIN_CAP, ADJ_GAIN, ADJ_SPEND_ALIVE, ADJ_SPEND, ADJ_ENOUGH, ADJ_FILL = range(7)
ADJ_RET, ADJ_SET = 1, 2


def query(scene, group=None, who=Q_PLAYERS, cls_mask=0x7FFF, pid=-1, mode=Q_INT_EQ32, value=0, value_head=0,
          skip_obj=-1):
    """One nfk_query; group None = every group of the scene, in group-id order."""
    return Query(int(scene), 0 if group is None else int(group), Q_ALL_GROUPS if group is None else 0, int(who),
                 int(cls_mask), int(pid), int(mode), int(skip_obj), int(value), int(value_head))


N_KERNEL_TIMERS = 7
KERNEL_TIMER_NAMES = ["k_tick", "k_records", "k_fanout", "aux", "k_scan_tiles", "membership", "k_chain"]


_lib = None


def load_library(path=LIB_PATH):
    """Load libnfgpu.so; raises if it is missing (no silent fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise ImportError(f"{path} not built: run __graft_entry__.build() (hipcc --offload-arch=gfx950)")
    lib = ctypes.CDLL(path)
    P, I32, I64, VP = ctypes.POINTER, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    sig = {
        "nfk_create": [P(Config), P(VP)], "nfk_destroy": [VP], "nfk_last_error": [],
        "nfk_set_prop_flags": [VP, I32, VP], "nfk_define_record": [VP, I32, I32, I32, VP, VP],
        "nfk_define_kind": [VP, I32, VP, I32],
        "nfk_create_objects": [VP, I32, VP, VP, VP, VP, VP, VP], "nfk_load_prop": [VP, I32, VP],
        "nfk_load_record": [VP, I32, VP, VP], "nfk_commit": [VP],
        "nfk_set_props": [VP, I32, VP, VP, VP, VP], "nfk_set_props_obj": [VP, I32, VP, VP, VP], "nfk_set_records": [VP, I32, VP, VP, VP, VP, VP, VP, VP],
        "nfk_get_records": [VP, I32, VP, VP, VP, VP, VP, VP],
        "nfk_add_schedules": [VP, I32, VP, VP, VP, VP, VP, VP],
        "nfk_remove_schedule": [VP, I64, I64, I32], "nfk_remove_all_schedules": [VP, I64, I64],
        "nfk_schedule_calls": [VP, I32, VP, VP, VP, VP, VP, VP, VP], "nfk_schedule_calls_obj": [VP, I32, VP, VP, VP, VP, VP, VP],
        "nfk_get_props": [VP, I32, VP, VP, VP, VP], "nfk_exist_schedule": [VP, I64, I64, I32, VP],
        "nfk_execute": [VP, I64], "nfk_execute_calls": [VP], "nfk_summary_get": [VP, P(Summary)], "nfk_outputs_get": [VP, P(Outputs)],
        "nfk_read_prop": [VP, I32, VP], "nfk_read_record": [VP, I32, VP], "nfk_read_schedules": [VP, VP, VP, VP],
        "nfk_read_schedule_forms": [VP, VP],
        "nfk_read_events": [VP, VP, VP, VP, VP], "nfk_read_rec_events": [VP, VP, VP, VP, VP],
        "nfk_read_fired": [VP, VP, VP, VP], "nfk_read_fanout": [VP, VP, VP],
        "nfk_set_profiling": [VP, I32], "nfk_kernel_times": [VP, VP, VP, VP], "nfk_reset_kernel_times": [VP],
        "nfk_set_scene_props": [VP, I32, I32, I32, I32, I32],
        "nfk_switch_scene": [VP, I64, I64, I32, I32, ctypes.c_float, ctypes.c_float, ctypes.c_float],
        "nfk_destroy_objects": [VP, I32, VP, VP], "nfk_object_count": [VP, VP], "nfk_row_words": [VP, VP],
        "nfk_export_objects": [VP, I32, VP, VP, VP],
        "nfk_import_objects": [VP, I32, VP, VP, VP, VP, VP, VP, VP],
        "nfk_spawn_objects": [VP, I32, VP, VP, VP, VP, VP, VP, VP], "nfk_sync": [VP],
        "nfk_rank_top": [VP, I32, I32, VP, VP, VP, VP],
        "nfk_jit_status": [VP, VP, VP, I32], "nfk_membership_stats": [VP, VP, VP, VP, VP],
        "nfk_jit_preview": [I32, I32, I32, I32, VP, VP, VP, I32, VP, VP, I32, VP, I32],
        "nfk_jit_preview_rec": [I32, I32, I32, I32, VP, VP, VP, I32, VP, VP, VP, I32, VP, VP, I32, VP, I32],
        "nfk_watch_props": [VP, I32, VP], "nfk_read_chain": [VP, I32, VP, VP, VP, VP, VP, VP, VP],
        "nfk_load_object": [VP, I32, VP, VP], "nfk_set_objects": [VP, I32, VP, VP, VP, VP, VP],
        "nfk_get_objects": [VP, I32, VP, VP, VP, VP, VP], "nfk_read_object": [VP, I32, VP, VP],
        "nfk_read_events_obj": [VP, VP, VP], "nfk_record_rows": [VP, I32, VP, VP, VP, VP, VP, VP],
        "nfk_query_objects": [VP, I32, VP, P(QueryResult)], "nfk_online_count": [VP, I32, I32, VP],
        "nfk_find_rows": [VP, I32, VP, VP, VP, VP, VP, VP], "nfk_find_rows_obj": [VP, I32, VP, VP, VP, VP, VP],
        "nfk_find_stats": [VP, VP, VP, VP], "nfk_get_used_rows": [VP, I32, VP, VP, VP, VP],
        "nfk_snapshot_objects": [VP, I32, VP, VP, VP, P(Snapshot)],
        "nfk_snapshot_objects_obj": [VP, I32, VP, VP, P(Snapshot)], "nfk_set_snapshot_order": [VP, VP, VP],
        "nfk_set_record_objects": [VP, I32, VP, VP, VP, VP, VP, VP, VP],
        "nfk_get_record_objects": [VP, I32, VP, VP, VP, VP, VP, VP, VP],
        "nfk_find_objects": [VP, I32, VP, VP, VP, VP, VP, VP, VP],
        "nfk_find_objects_obj": [VP, I32, VP, VP, VP, VP, VP, VP], "nfk_read_rec_events_obj": [VP, VP, VP],
        "nfk_swap_rows": [VP, I32, VP, VP, VP, VP, VP],
        "nfk_link_record": [VP, I32, I32, VP, I32],
        "nfk_view_changes": [VP, P(ViewChanges)],
        "nfk_adjust_props": [VP, I32, VP, VP, VP, VP, VP, VP, VP],
        "nfk_adjust_props_obj": [VP, I32, VP, VP, VP, VP, VP, VP], "nfk_adjust_stats": [VP, P(AdjustStats)],
    }
    for name, args in sig.items():
        if not hasattr(lib, name) and os.environ.get("NFGPU_LIB"):
            continue   # (A/B timing of an older library build: entry points it predates stay unbound)
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = ctypes.c_char_p if name == "nfk_last_error" else ctypes.c_int
    _lib = lib
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


class NFKernelModule:
    """One GPU-resident world (the entities of one scene shard)."""

    def __init__(self, capacity, n_int=wl.N_INT, n_flt=wl.N_FLT, n_class=2, n_kind=len(wl.KINDS), n_rec=0,
                 msg_capacity=0, stream=None, slack_per_256=0, n_oprops=0):
        self.lib = load_library()
        cfg = Config(capacity, n_int, n_flt, n_class, n_kind, n_rec, msg_capacity, stream, slack_per_256, n_oprops)
        self.n_oprops = n_oprops
        h = ctypes.c_void_p()
        self._chk(self.lib.nfk_create(ctypes.byref(cfg), ctypes.byref(h)))
        self.h = h
        self.stream = stream
        self.n_int, self.n_flt, self.n_kind, self.n_rec = n_int, n_flt, n_kind, n_rec
        self.n_obj = 0
        self.rec_shape = {}

    def _chk(self, rc):
        if rc != NFK_OK:
            raise NFKError(rc, self.lib.nfk_last_error().decode())
        return rc

    def close(self):
        if getattr(self, "h", None):
            self.lib.nfk_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- schema (NFIClassModule) ----
    def set_prop_flags(self, cls, flags):
        flags = np.ascontiguousarray(flags, np.uint8)
        self._chk(self.lib.nfk_set_prop_flags(self.h, cls, _p(flags)))

    def define_record(self, rec, rows, cols, col_types, flags_per_class):
        ct = np.ascontiguousarray(col_types, np.uint8)
        fl = np.ascontiguousarray(flags_per_class, np.uint8)
        self._chk(self.lib.nfk_define_record(self.h, rec, rows, cols, _p(ct), _p(fl)))
        self.rec_shape[rec] = (cols, rows)
        self.rec_types = {**getattr(self, "rec_types", {}), rec: [int(t) for t in ct[:cols]]}
        # the reference's LOGICAL columns (an object column is one) as physical columns: the C-ABI and
        # the batch methods speak physical columns (an object cell named by its data half's), the
        # methods with the reference's names (FindInt, SetRecordObject, QueryRow, ...) logical ones
        self.rec_logical = {**getattr(self, "rec_logical", {}),
                            rec: [c for c in range(cols) if int(ct[c]) != REC_OBJ_HEAD]}
        self.rec_has_obj = getattr(self, "rec_has_obj", False) or REC_OBJ_DATA in self.rec_types[rec]

    def _phys(self, rec, col):
        """logical column -> (physical column, its type), or None for an unknown record / column"""
        lg = getattr(self, "rec_logical", {}).get(rec)
        if lg is None or col < 0 or col >= len(lg):
            return None
        return lg[col], self.rec_types[rec][lg[col]]

    def define_kind(self, kind, ops):
        ops = np.ascontiguousarray(ops)
        if ops.dtype != wl.OP_DTYPE:
            ops = ops.view(wl.OP_DTYPE).reshape(-1)
        self._chk(self.lib.nfk_define_kind(self.h, kind, _p(ops), len(ops)))

    # ---- objects (NFIKernelModule::CreateObject) ----
    def create_objects(self, guid_head, guid_data, scene, group, cls, is_player):
        a = [np.ascontiguousarray(x, t) for x, t in
             ((guid_head, np.int64), (guid_data, np.int64), (scene, np.int32), (group, np.int32),
              (cls, np.uint8), (is_player, np.uint8))]
        self._chk(self.lib.nfk_create_objects(self.h, len(a[0]), *[_p(x) for x in a]))
        self._keep = getattr(self, "_keep", []) + [a]
        self.n_obj += len(a[0])

    def load_prop(self, pid, values):
        v = np.ascontiguousarray(values)
        bits = v.view(np.uint64) if v.dtype.itemsize == 8 else v.astype(np.int64).view(np.uint64)
        self._chk(self.lib.nfk_load_prop(self.h, pid, _p(np.ascontiguousarray(bits))))

    def load_object(self, pid, head, data):
        h = np.ascontiguousarray(head, np.int64)
        d = np.ascontiguousarray(data, np.int64)
        self._chk(self.lib.nfk_load_object(self.h, pid, _p(h), _p(d)))

    def load_record(self, rec, cells, used):
        c = np.ascontiguousarray(cells, np.uint64)
        u = np.ascontiguousarray(used, np.uint64)
        self._chk(self.lib.nfk_load_record(self.h, rec, _p(c), _p(u)))

    # ---- NFCPropertyModule::OnRecordPropertyEvent (PM:127-149) as part of the schema ----
    def link_record(self, rec, rows, col_pid):
        """nfk_link_record, before commit: after every record event of `rec` the int property
        col_pid[nCol] takes the 32-bit sum of column nCol over the record's first `rows` rows
        (nCol: a Set's column; 0 for AddRow / Remove / ClearRecord; a Swap's target row).
        col_pid: one property id per column, -1 for none; None removes the record's link."""
        cp = None if col_pid is None else np.ascontiguousarray(col_pid, np.int32)
        if cp is not None and len(cp) != self.rec_shape.get(rec, (len(cp), 0))[0]:
            raise ValueError("link_record: one property id (or -1) per column of the record")
        self._chk(self.lib.nfk_link_record(self.h, rec, rows, None if cp is None else _p(cp), LINK_SUM32))

    def commit(self):
        self._chk(self.lib.nfk_commit(self.h))

    # ---- NFIKernelModule::SetProperty* (queued, applied at the next Execute) ----
    def set_props(self, guid_head, guid_data, pid, bits):
        a = [np.ascontiguousarray(x, t) for x, t in
             ((guid_head, np.int64), (guid_data, np.int64), (pid, np.int32), (bits, np.uint64))]
        self._chk(self.lib.nfk_set_props(self.h, len(a[0]), *[_p(x) for x in a]))

    def set_props_obj(self, obj, pid, bits):
        """nfk_set_props_obj: the same calls by nfk object index (creation order; the outputs' ev_obj)."""
        a = [np.ascontiguousarray(x, t) for x, t in ((obj, np.int32), (pid, np.int32), (bits, np.uint64))]
        self._chk(self.lib.nfk_set_props_obj(self.h, len(a[0]), *[_p(x) for x in a]))

    # ---- NFIKernelModule::SetPropertyObject / GetPropertyObject (KM:362 / KM:440) ----
    def set_objects(self, guid_head, guid_data, pid, val_head, val_data):
        a = [np.ascontiguousarray(x, t) for x, t in
             ((guid_head, np.int64), (guid_data, np.int64), (pid, np.int32), (val_head, np.int64),
              (val_data, np.int64))]
        self._chk(self.lib.nfk_set_objects(self.h, len(a[0]), *[_p(x) for x in a]))

    def get_objects(self, guid_head, guid_data, pid):
        a = [np.ascontiguousarray(x, t) for x, t in ((guid_head, np.int64), (guid_data, np.int64), (pid, np.int32))]
        vh = np.zeros(len(a[0]), np.int64)
        vd = np.zeros(len(a[0]), np.int64)
        self._chk(self.lib.nfk_get_objects(self.h, len(a[0]), *[_p(x) for x in a], _p(vh), _p(vd)))
        return vh, vd

    def SetPropertyObject(self, guid, pid, value):
        self.set_objects([guid[0]], [guid[1]], [pid], [value[0]], [value[1]])
        return True

    def GetPropertyObject(self, guid, pid):
        vh, vd = self.get_objects([guid[0]], [guid[1]], [pid])
        return int(vh[0]), int(vd[0])

    def read_object(self, pid):
        h = np.zeros(self.n_obj, np.int64)
        d = np.zeros(self.n_obj, np.int64)
        self._chk(self.lib.nfk_read_object(self.h, pid, _p(h), _p(d)))
        return h, d

    # ---- NFIKernelModule::SetRecordInt / SetRecordFloat ----
    def set_records(self, guid_head, guid_data, rec, row, col, bits, is_float=None):
        a = [np.ascontiguousarray(x, t) for x, t in
             ((guid_head, np.int64), (guid_data, np.int64), (rec, np.int32), (row, np.int32), (col, np.int32))]
        f = None if is_float is None else np.ascontiguousarray(is_float, np.uint8)
        b = np.ascontiguousarray(bits, np.uint64)
        self._chk(self.lib.nfk_set_records(self.h, len(a[0]), *[_p(x) for x in a], _p(f) if f is not None else None,
                                           _p(b)))

    def record_rows(self, guid_head, guid_data, rec, op, row, values=None):
        """NFCRecord::AddRow (op 1, row -1 = first unused, values [n][16] words) / Remove (op 2) /
        NFIKernelModule::ClearRecord (op 3), queued in call order with the SetRecord calls"""
        a = [np.ascontiguousarray(x, t) for x, t in
             ((guid_head, np.int64), (guid_data, np.int64), (rec, np.int32), (op, np.int32), (row, np.int32))]
        v = None if values is None else np.ascontiguousarray(values, np.uint64).reshape(len(a[0]), 16)
        self._chk(self.lib.nfk_record_rows(self.h, len(a[0]), *[_p(x) for x in a], _p(v)))

    def AddRow(self, guid, rec, row=-1, values=None):
        self.record_rows([guid[0]], [guid[1]], [rec], [1], [row], None if values is None else [values])
        return True

    def RemoveRow(self, guid, rec, row):
        self.record_rows([guid[0]], [guid[1]], [rec], [2], [row])
        return True

    def ClearRecord(self, guid, rec):
        self.record_rows([guid[0]], [guid[1]], [rec], [3], [0])
        return True

    # ---- NFCRecord::SwapRowInfo (RC:1219-1253) ----
    def swap_rows(self, guid_head, guid_data, rec, origin, target):
        """nfk_swap_rows: queued in call order with set_records / set_record_objects / record_rows;
        a used origin row changes places with the target row (cells of every column, used bits, the
        window's Update log) and raises one Swap event, rrc = 4 << 24 | rec << 16 | origin << 8 | target"""
        a = [np.ascontiguousarray(x, t) for x, t in
             ((guid_head, np.int64), (guid_data, np.int64), (rec, np.int32), (origin, np.int32), (target, np.int32))]
        self._chk(self.lib.nfk_swap_rows(self.h, len(a[0]), *[_p(x) for x in a]))

    def get_used_rows(self, guid_head, guid_data, rec):
        """nfk_get_used_rows -> uint64 used-row masks, this window's queued row calls replayed"""
        a = [np.ascontiguousarray(x, t) for x, t in ((guid_head, np.int64), (guid_data, np.int64), (rec, np.int32))]
        out = np.zeros(len(a[0]), np.uint64)
        self._chk(self.lib.nfk_get_used_rows(self.h, len(a[0]), *[_p(x) for x in a], _p(out)))
        return out

    def SwapRowInfo(self, guid, rec, origin, target):
        """NFCRecord::SwapRowInfo: False (nothing queued) for an unknown record, a row outside the
        record or an origin that is unused now (the window's queued calls replayed); else queued"""
        shape = self.rec_shape.get(rec)
        if shape is None or origin < 0 or origin >= shape[1] or target < 0 or target >= shape[1]:
            return False
        if not (int(self.get_used_rows([guid[0]], [guid[1]], [rec])[0]) >> origin) & 1:
            return False
        self.swap_rows([guid[0]], [guid[1]], [rec], [origin], [target])
        return True

    # ---- NFIKernelModule::SetRecordObject / NFCRecord::GetObject (RC:367-421 / RC:697-716) ----
    def set_record_objects(self, guid_head, guid_data, rec, row, col, val_head, val_data):
        """nfk_set_record_objects: queued with set_records / record_rows in call order; col is the
        physical column of the object cell's data half"""
        a = [np.ascontiguousarray(x, t) for x, t in
             ((guid_head, np.int64), (guid_data, np.int64), (rec, np.int32), (row, np.int32), (col, np.int32),
              (val_head, np.int64), (val_data, np.int64))]
        self._chk(self.lib.nfk_set_record_objects(self.h, len(a[0]), *[_p(x) for x in a]))

    def get_record_objects(self, guid_head, guid_data, rec, row, col):
        """nfk_get_record_objects -> (head, data) arrays, read-your-writes; (0, 0) for an unused row"""
        a = [np.ascontiguousarray(x, t) for x, t in
             ((guid_head, np.int64), (guid_data, np.int64), (rec, np.int32), (row, np.int32), (col, np.int32))]
        vh = np.zeros(len(a[0]), np.int64)
        vd = np.zeros(len(a[0]), np.int64)
        self._chk(self.lib.nfk_get_record_objects(self.h, len(a[0]), *[_p(x) for x in a], _p(vh), _p(vd)))
        return vh, vd

    def SetRecordObject(self, guid, rec, row, col, value):
        """NFIKernelModule::SetRecordObject (logical column): False for an unknown record, an invalid
        row or column, or a column that holds no NFGUID (RC:367-381); the refusal on an unused row and
        the equal-value test follow at the next frame, in call order"""
        pc = self._phys(rec, col)
        if pc is None or pc[1] != REC_OBJ_DATA or row < 0 or row >= self.rec_shape[rec][1]:
            return False
        self.set_record_objects([guid[0]], [guid[1]], [rec], [row], [pc[0]], [value[0]], [value[1]])
        return True

    def GetRecordObject(self, guid, rec, row, col):
        """NFCRecord::GetObject (logical column) -> (head, data); NULL_OBJECT (0, 0) for an invalid
        cell, a column of another type or an unused row"""
        pc = self._phys(rec, col)
        if pc is None or pc[1] != REC_OBJ_DATA or row < 0 or row >= self.rec_shape[rec][1]:
            return 0, 0
        vh, vd = self.get_record_objects([guid[0]], [guid[1]], [rec], [row], [pc[0]])
        return int(vh[0]), int(vd[0])

    def get_records(self, guid_head, guid_data, rec, row, col):
        """NFIKernelModule::GetRecordInt/Float for n cells: raw 64-bit patterns, read-your-writes"""
        a = [np.ascontiguousarray(x, t) for x, t in
             ((guid_head, np.int64), (guid_data, np.int64), (rec, np.int32), (row, np.int32), (col, np.int32))]
        out = np.zeros(len(a[0]), np.uint64)
        self._chk(self.lib.nfk_get_records(self.h, len(a[0]), *[_p(x) for x in a], _p(out)))
        return out

    # ---- NFCRecord::FindInt / FindFloat / QueryRow (RC:830-899, RC:554) ----
    def find_rows(self, guid_head, guid_data, rec, col, bits, stats=None):
        """nfk_find_rows: n (object, record, column, argument bits) finds -> uint64 row masks (bit r:
        row r is used and its cell equals the argument under the column's type), read-your-writes.
        stats: a dict that receives the launch's device time (kernel_ms, with set_profiling(True)),
        the bytes read back and the finds answered on the host (n_host)."""
        a = [np.ascontiguousarray(x, t) for x, t in
             ((guid_head, np.int64), (guid_data, np.int64), (rec, np.int32), (col, np.int32), (bits, np.uint64))]
        out = np.zeros(len(a[0]), np.uint64)
        self._chk(self.lib.nfk_find_rows(self.h, len(a[0]), *[_p(x) for x in a], _p(out)))
        self._find_stats(stats)
        return out

    def find_rows_obj(self, obj, rec, col, bits, stats=None):
        """nfk_find_rows_obj: find_rows by object index (query_objects' hits, the outputs' ev_obj)"""
        a = [np.ascontiguousarray(x, t) for x, t in
             ((obj, np.int32), (rec, np.int32), (col, np.int32), (bits, np.uint64))]
        out = np.zeros(len(a[0]), np.uint64)
        self._chk(self.lib.nfk_find_rows_obj(self.h, len(a[0]), *[_p(x) for x in a], _p(out)))
        self._find_stats(stats)
        return out

    def find_objects(self, guid_head, guid_data, rec, col, val_head, val_data, stats=None):
        """nfk_find_objects: n (object, record, object column, NFGUID) finds -> uint64 row masks (bit
        r: row r is used and both halves of its cell equal the argument); col is the physical column
        of the data half; read-your-writes and stats as find_rows"""
        a = [np.ascontiguousarray(x, t) for x, t in
             ((guid_head, np.int64), (guid_data, np.int64), (rec, np.int32), (col, np.int32), (val_head, np.int64),
              (val_data, np.int64))]
        out = np.zeros(len(a[0]), np.uint64)
        self._chk(self.lib.nfk_find_objects(self.h, len(a[0]), *[_p(x) for x in a], _p(out)))
        self._find_stats(stats)
        return out

    def find_objects_obj(self, obj, rec, col, val_head, val_data, stats=None):
        """nfk_find_objects_obj: find_objects by object index"""
        a = [np.ascontiguousarray(x, t) for x, t in
             ((obj, np.int32), (rec, np.int32), (col, np.int32), (val_head, np.int64), (val_data, np.int64))]
        out = np.zeros(len(a[0]), np.uint64)
        self._chk(self.lib.nfk_find_objects_obj(self.h, len(a[0]), *[_p(x) for x in a], _p(out)))
        self._find_stats(stats)
        return out

    def FindObject(self, guid, rec, col, value, result):
        """NFCRecord::FindObject (RC:957, logical column): rows whose cell equals the NFGUID value
        (head, data), appended to result; -1 as FindInt"""
        pc = self._phys(rec, col)
        if pc is None or pc[1] != REC_OBJ_DATA:
            return -1
        try:
            m = int(self.find_objects([guid[0]], [guid[1]], [rec], [pc[0]], [value[0]], [value[1]])[0])
        except NFKError as e:
            if e.code != -7:
                raise
            return -1
        result.extend(r for r in range(64) if (m >> r) & 1)
        return len(result)

    def _find_stats(self, stats):
        if stats is None:
            return
        ms, by, nh = ctypes.c_double(), ctypes.c_int64(), ctypes.c_int32()
        self._chk(self.lib.nfk_find_stats(self.h, ctypes.byref(ms), ctypes.byref(by), ctypes.byref(nh)))
        stats["kernel_ms"], stats["bytes"], stats["n_host"] = ms.value, by.value, nh.value

    def _find(self, guid, rec, col, bits, want_float, result):
        """the reference's return: -1 (nothing appended) for an unknown object or record, an invalid
        column or a column of another type; else the hits appended and result's total size (RC:856)"""
        pc = self._phys(rec, col)   # (logical column; an object column is a column of another type)
        if pc is None or pc[1] != (REC_F64 if want_float else REC_INT):
            return -1
        col = pc[0]
        try:
            m = int(self.find_rows([guid[0]], [guid[1]], [rec], [col], [bits])[0])
        except NFKError as e:
            if e.code != -7:   # (NFK_ERR_NOTFOUND: "There is no object", the reference's -1)
                raise
            return -1
        result.extend(r for r in range(64) if (m >> r) & 1)
        return len(result)

    def FindInt(self, guid, rec, col, value, result):
        """NFCRecord::FindInt (RC:830): rows whose int cell equals value, appended to result"""
        return self._find(guid, rec, col, np.int64(value).view(np.uint64), False, result)

    def FindFloat(self, guid, rec, col, value, result):
        """NFCRecord::FindFloat (RC:873): rows whose f64 cell == value, appended to result"""
        return self._find(guid, rec, col, np.float64(value).view(np.uint64), True, result)

    def QueryRow(self, guid, rec, row):
        """NFCRecord::QueryRow (RC:554): the row's cells as raw 64-bit patterns [cols], or None for
        an invalid or unused row (the reference's false).  A record with object columns answers a
        list over its logical columns, an object cell as its (head, data) pair."""
        shape = self.rec_shape.get(rec)
        if shape is None or row < 0 or row >= shape[1]:
            return None
        used = np.zeros(1, np.uint64)
        gh, gd = np.array([guid[0]], np.int64), np.array([guid[1]], np.int64)
        self._chk(self.lib.nfk_get_used_rows(self.h, 1, _p(gh), _p(gd), _p(np.array([rec], np.int32)), _p(used)))
        if not (int(used[0]) >> row) & 1:
            return None
        cols = shape[0]
        w = self.get_records([guid[0]] * cols, [guid[1]] * cols, [rec] * cols, [row] * cols, list(range(cols)))
        types = self.rec_types[rec]
        if REC_OBJ_DATA not in types:
            return w
        return [(int(w[c + 1].view(np.int64)), int(w[c].view(np.int64))) if types[c] == REC_OBJ_DATA else w[c]
                for c in self.rec_logical[rec]]

    # ---- enter snapshots: OnPropertyEnter / OnRecordEnter payloads (nfk_snapshot_objects) ----
    def set_snapshot_order(self, prop_order=None, rec_order=None):
        """nfk_set_snapshot_order: the walk's order as permutations of the property ids and of the
        record ids (the reference walks its maps by name); None: id order"""
        po = None if prop_order is None else np.ascontiguousarray(prop_order, np.int32)
        ro = None if rec_order is None else np.ascontiguousarray(rec_order, np.int32)
        if po is not None and len(po) != self.n_int + self.n_flt + self.n_oprops:
            raise NFKError(-1, "prop_order: one entry per property")
        if ro is not None and len(ro) != self.n_rec:
            raise NFKError(-1, "rec_order: one entry per record")
        self._chk(self.lib.nfk_set_snapshot_order(self.h, _p(po), _p(ro)))

    def _snapshot_arrays(self, res, n, stats):
        def arr(ptr, k, dt):
            return np.ctypeslib.as_array(ptr, (k,)).copy() if k else np.zeros(0, dt)
        out = {k: arr(getattr(res, k), n, np.uint32) for k in ("p_first", "p_count", "r_first", "r_count")}
        n_p = int((out["p_first"].astype(np.int64) + out["p_count"]).max()) if n else 0
        n_r = int((out["r_first"].astype(np.int64) + out["r_count"]).max()) if n else 0
        out["p_pid"] = arr(res.p_pid, n_p, np.int32)
        out["p_bits"] = arr(res.p_bits, n_p, np.uint64)
        out["p_head"] = arr(res.p_head, n_p, np.uint64) if res.p_head else None
        out["r_rec"] = arr(res.r_rec, n_r, np.int32)
        out["r_used"] = arr(res.r_used, n_r, np.uint64)
        out["r_cell"] = arr(res.r_cell, n_r, np.uint32)
        # the entries' used-row counts (one byte-table pass), and from them the cells' extent
        out["r_nused"] = np.unpackbits(out["r_used"].view(np.uint8)).reshape(n_r, 64).sum(1, dtype=np.int64)
        cols = np.array([self.rec_shape.get(r, (0, 0))[0] for r in range(MAX_RECORDS)], np.int64)
        n_c = int((out["r_cell"].astype(np.int64) + cols[out["r_rec"]] * out["r_nused"]).max()) if n_r else 0
        out["cells"] = arr(res.cells, n_c, np.uint64)
        if stats is not None:
            stats["kernel_ms"], stats["bytes"], stats["n_host"] = res.kernel_ms, res.bytes, res.n_host
        return out

    def snapshot_objects(self, guid_head, guid_data, view, stats=None):
        """nfk_snapshot_objects: n (object, view) requests (VIEW_PUBLIC / VIEW_PRIVATE) -> a dict of
        numpy copies of the nfk_snapshot arrays (p_first, p_count, p_pid, p_bits, p_head or None,
        r_first, r_count, r_rec, r_used, r_cell, cells; r_nused: the entries' used-row counts), the
        reference's now.  stats: a dict that receives kernel_ms (with set_profiling(True)), the bytes
        read back and the requests answered on the host (n_host)."""
        gh, gd = np.ascontiguousarray(guid_head, np.int64), np.ascontiguousarray(guid_data, np.int64)
        v = np.ascontiguousarray(view, np.uint8)
        res = Snapshot()
        self._chk(self.lib.nfk_snapshot_objects(self.h, len(gh), _p(gh), _p(gd), _p(v), ctypes.byref(res)))
        return self._snapshot_arrays(res, len(gh), stats)

    def snapshot_objects_obj(self, obj, view, stats=None):
        """nfk_snapshot_objects_obj: snapshot_objects by object index (query_objects' hits, ev_obj)"""
        o, v = np.ascontiguousarray(obj, np.int32), np.ascontiguousarray(view, np.uint8)
        res = Snapshot()
        self._chk(self.lib.nfk_snapshot_objects_obj(self.h, len(o), _p(o), _p(v), ctypes.byref(res)))
        return self._snapshot_arrays(res, len(o), stats)

    def _set_col(self, rec, col):
        """the physical column of a SetRecordInt / SetRecordFloat's logical column, or None when it is
        an object column (a column of another type: the reference returns false, RC:189)"""
        pc = self._phys(rec, col)
        if pc is None:
            return col   # (an unknown record or column: nfk_set_records reports it)
        return None if pc[1] >= REC_OBJ_DATA else pc[0]

    def SetRecordInt(self, guid, rec, row, col, value):
        col = self._set_col(rec, col)
        if col is None:
            return False
        self.set_records([guid[0]], [guid[1]], [rec], [row], [col], [np.int64(value).view(np.uint64)], [0])
        return True

    def SetRecordFloat(self, guid, rec, row, col, value):
        col = self._set_col(rec, col)
        if col is None:
            return False
        self.set_records([guid[0]], [guid[1]], [rec], [row], [col], [np.float64(value).view(np.uint64)], [1])
        return True

    def SetPropertyInt(self, guid, prop, value):
        pid = wl.PID[prop] if isinstance(prop, str) else prop
        self.set_props([guid[0]], [guid[1]], [pid], [np.int64(value).view(np.uint64)])
        return True

    def SetPropertyFloat(self, guid, prop, value):
        pid = wl.PID[prop] if isinstance(prop, str) else prop
        self.set_props([guid[0]], [guid[1]], [pid], [np.float64(value).view(np.uint64)])
        return True

    # ---- NFIScheduleModule ----
    def add_schedules(self, guid_head, guid_data, kind, interval_s, count, now_ms):
        a = [np.ascontiguousarray(x, t) for x, t in
             ((guid_head, np.int64), (guid_data, np.int64), (kind, np.int32), (interval_s, np.float32),
              (count, np.int32), (now_ms, np.int64))]
        self._chk(self.lib.nfk_add_schedules(self.h, len(a[0]), *[_p(x) for x in a]))

    def AddSchedule(self, guid, name, interval_s, count, now_ms):
        kind = wl.KID[name] if isinstance(name, str) else name
        self.add_schedules([guid[0]], [guid[1]], [kind], [interval_s], [count], [now_ms])
        return True

    def schedule_calls(self, op, guid_head, guid_data, kind, interval_s, count, now_ms):
        """AddSchedule (op 1) / RemoveSchedule(self, name) (op 2) / RemoveSchedule(self) (op 3)
        calls in call order, as one batch."""
        a = [np.ascontiguousarray(x, t) for x, t in
             ((op, np.int32), (guid_head, np.int64), (guid_data, np.int64), (kind, np.int32),
              (interval_s, np.float32), (count, np.int32), (now_ms, np.int64))]
        self._chk(self.lib.nfk_schedule_calls(self.h, len(a[0]), *[_p(x) for x in a]))

    def schedule_calls_obj(self, op, obj, kind, interval_s, count, now_ms):
        """nfk_schedule_calls_obj: schedule_calls by nfk object index."""
        a = [np.ascontiguousarray(x, t) for x, t in
             ((op, np.int32), (obj, np.int32), (kind, np.int32), (interval_s, np.float32), (count, np.int32),
              (now_ms, np.int64))]
        self._chk(self.lib.nfk_schedule_calls_obj(self.h, len(a[0]), *[_p(x) for x in a]))

    def RemoveSchedule(self, guid, name=None):
        if name is None:
            self._chk(self.lib.nfk_remove_all_schedules(self.h, int(guid[0]), int(guid[1])))
        else:
            kind = wl.KID[name] if isinstance(name, str) else name
            self._chk(self.lib.nfk_remove_schedule(self.h, int(guid[0]), int(guid[1]), kind))
        return True

    # ---- runtime membership (NFCKernelModule::SwitchScene / DestroyObject / CreateObject) ----
    def set_scene_props(self, pid_scene, pid_group, pid_x, pid_y, pid_z):
        self._chk(self.lib.nfk_set_scene_props(self.h, pid_scene, pid_group, pid_x, pid_y, pid_z))

    def SwitchScene(self, guid, scene, group, x, y, z):
        self._chk(self.lib.nfk_switch_scene(self.h, int(guid[0]), int(guid[1]), int(scene), int(group),
                                            float(x), float(y), float(z)))
        return True

    def destroy_objects(self, guid_head, guid_data):
        a = [np.ascontiguousarray(x, np.int64) for x in (guid_head, guid_data)]
        self._chk(self.lib.nfk_destroy_objects(self.h, len(a[0]), _p(a[0]), _p(a[1])))

    def DestroyObject(self, guid):
        self.destroy_objects([guid[0]], [guid[1]])
        return True

    def object_count(self):
        n = ctypes.c_int32()
        self._chk(self.lib.nfk_object_count(self.h, ctypes.byref(n)))
        return n.value

    def membership_stats(self):
        """{n_full, n_seg, host_ms_full, host_ms_seg}: membership windows applied by rebuilding the
        segment table / by rewriting only changed segments, and their host planning time"""
        nf, ns = ctypes.c_int64(), ctypes.c_int64()
        mf, ms = ctypes.c_double(), ctypes.c_double()
        self._chk(self.lib.nfk_membership_stats(self.h, ctypes.byref(nf), ctypes.byref(ns), ctypes.byref(mf),
                                                ctypes.byref(ms)))
        return {"n_full": nf.value, "n_seg": ns.value, "host_ms_full": mf.value, "host_ms_seg": ms.value}

    def jit_status(self):
        """(True, message) when k_tick runs the hipRTC specialisation built at commit"""
        on = ctypes.c_int32()
        msg = ctypes.create_string_buffer(4096)
        self._chk(self.lib.nfk_jit_status(self.h, ctypes.byref(on), msg, len(msg)))
        return bool(on.value), msg.value.decode()

    def row_words(self):
        n = ctypes.c_int32()
        self._chk(self.lib.nfk_row_words(self.h, ctypes.byref(n)))
        return n.value

    def export_objects(self, guid_head, guid_data, rows_dev_ptr):
        """Pack the entities' state rows into device memory at rows_dev_ptr ([n][row_words] u64)
        on the world's stream and remove them from this world."""
        a = [np.ascontiguousarray(x, np.int64) for x in (guid_head, guid_data)]
        self._chk(self.lib.nfk_export_objects(self.h, len(a[0]), _p(a[0]), _p(a[1]), ctypes.c_void_p(rows_dev_ptr)))

    def import_objects(self, guid_head, guid_data, scene, group, cls, is_player, rows_dev_ptr):
        a = [np.ascontiguousarray(x, t) for x, t in
             ((guid_head, np.int64), (guid_data, np.int64), (scene, np.int32), (group, np.int32),
              (cls, np.uint8), (is_player, np.uint8))]
        self._chk(self.lib.nfk_import_objects(self.h, len(a[0]), *[_p(x) for x in a], ctypes.c_void_p(rows_dev_ptr)))
        self.n_obj = self.object_count()

    def spawn_objects(self, guid_head, guid_data, scene, group, cls, is_player, props):
        a = [np.ascontiguousarray(x, t) for x, t in
             ((guid_head, np.int64), (guid_data, np.int64), (scene, np.int32), (group, np.int32),
              (cls, np.uint8), (is_player, np.uint8))]
        pr = np.ascontiguousarray(props, np.uint64)
        self._chk(self.lib.nfk_spawn_objects(self.h, len(a[0]), *[_p(x) for x in a], _p(pr)))
        self.n_obj = self.object_count()

    # ---- leaderboards (NFIRankRedisModule::GetRange) ----
    def rank_top(self, prop, k):
        """The k entities with the highest score (the property as a double), ties by
        NFGUID::ToString() descending: (guid_head, guid_data, score) arrays."""
        pid = wl.PID[prop] if isinstance(prop, str) else int(prop)
        gh = np.zeros(max(k, 1), np.int64)
        gd = np.zeros(max(k, 1), np.int64)
        sc = np.zeros(max(k, 1), np.float64)
        n = ctypes.c_int32()
        self._chk(self.lib.nfk_rank_top(self.h, pid, int(k), ctypes.byref(n), _p(gh), _p(gd), _p(sc)))
        return gh[:n.value], gd[:n.value], sc[:n.value]

    # ---- scene queries (NFCKernelModule::GetObjectByProperty / GetGroupObjectList, KM:1169-1405) ----
    def query_objects(self, queries, with_exists=False, stats=None):
        """nfk_query_objects: one batch of `query(...)` records -> a list of object-index arrays (the
        outputs' ev_obj indices) in the reference's order: group id, then NFGUID.  with_exists: also
        the per-query exists flags (False: this world holds no such scene / scene group).  stats: a
        dict that receives the launches' device time (kernel_ms, with set_profiling(True)) and the
        bytes read back."""
        qs = (Query * max(len(queries), 1))(*queries)
        res = QueryResult()
        self._chk(self.lib.nfk_query_objects(self.h, len(queries), qs, ctypes.byref(res)))
        n = len(queries)
        off = np.ctypeslib.as_array(res.off, (n + 1,)).copy() if n else np.zeros(1, np.uint32)
        tot = int(off[n])
        obj = np.ctypeslib.as_array(res.obj, (tot,)).copy() if tot else np.zeros(0, np.int32)
        out = [obj[int(off[i]):int(off[i + 1])] for i in range(n)]
        if stats is not None:
            stats["kernel_ms"], stats["bytes"] = res.kernel_ms, res.bytes
        if with_exists:
            ex = np.ctypeslib.as_array(res.exists, (n,)).astype(bool) if n else np.zeros(0, bool)
            return out, ex
        return out

    def _guids(self, obj, guid_head, guid_data):
        return [(int(guid_head[o]), int(guid_data[o])) for o in obj]

    def object_by_property(self, scene, prop, value):
        """NFCKernelModule::GetObjectByProperty (KM:1357-1405) over the scene's players, as object
        indices: `value` an int (compared as the reference does, through an int: KM:1372), a
        (head, data) NFGUID pair, or a float (matches nothing, KM:1398).  An argument of another type
        than the property reads the getter's null value (TData::GetInt 0 / GetObject the null NFGUID).
        Every class is taken to have the property (cls_mask 0x7FFF: this mirror keeps no per-class
        property list, and a workload's classes share one schema); the C++ plugin builds the mask
        from SetPropertyFlags.  A caller with classes that lack it passes its own mask to query()."""
        pid = wl.PID[prop] if isinstance(prop, str) else int(prop)
        n_if = self.n_int + self.n_flt
        if isinstance(value, float):
            return np.zeros(0, np.int32)
        is_obj = isinstance(value, tuple)
        if is_obj and pid >= n_if:
            q = query(scene, pid=pid, mode=Q_OBJ_EQ, value=value[1], value_head=value[0])
        elif not is_obj and pid < self.n_int:
            q = query(scene, pid=pid, mode=Q_INT_EQ32, value=value)
        else:   # the getter of the argument's type reads the null value from the property
            null = (tuple(value) == (0, 0)) if is_obj else (int(value) == 0)
            if not null:
                return np.zeros(0, np.int32)
            q = query(scene)
        return self.query_objects([q])[0]

    def group_object_list(self, scene, group, who=None, no_self=-1, cls=None):
        """NFCKernelModule::GetGroupObjectList (KM:1169-1294) as (found, object indices): who = True
        the group's players, False its other objects, None players then others (KM:1169); no_self: an
        object index left out (KM:1270); cls: only objects of that class id (the strClassName
        overloads)."""
        mask = 0x7FFF if cls is None else 1 << int(cls)
        whos = [Q_PLAYERS, Q_OTHERS] if who is None else [Q_PLAYERS if who else Q_OTHERS]
        lists, ex = self.query_objects([query(scene, group, w, mask, skip_obj=no_self) for w in whos], with_exists=True)
        return bool(ex[0]), np.concatenate(lists)

    def GetObjectByProperty(self, scene, prop, value, guid_head, guid_data):
        """object_by_property as NFGUIDs (head, data); guid_head / guid_data: the NFGUIDs by object
        index, which the caller holds"""
        return self._guids(self.object_by_property(scene, prop, value), guid_head, guid_data)

    def GetGroupObjectList(self, scene, group, who, guid_head, guid_data, no_self=-1, cls=None):
        """group_object_list's list as NFGUIDs (head, data)"""
        return self._guids(self.group_object_list(scene, group, who, no_self, cls)[1], guid_head, guid_data)

    def GetSceneOnLineList(self, scene, guid_head, guid_data):
        """NFCKernelModule::GetSceneOnLineList (KM:1042): the players of every group of the scene"""
        return self._guids(self.query_objects([query(scene)])[0], guid_head, guid_data)

    # ---- view changes (NFCSceneAOIModule::OnGroupEvent / OnSceneEvent / OnClassCommonEvent, AOI:292-529) ----
    def view_changes(self):
        """nfk_view_changes: the window's membership log and, per visit, the group's players and its
        other objects as of the visit's call.  A dict of numpy arrays: log [n_calls, 6] (object, kind,
        from scene, from group, to scene, to group), call_visit [n_calls + 1], visit [n_visits, 3]
        (why, scene, group), visit_off [2 n_visits + 1] into obj (players of visit v at
        obj[off[2v]:off[2v + 1]], others at obj[off[2v + 1]:off[2v + 2]]); and kernel_ms, bytes,
        n_host, n_tiles."""
        res = ViewChanges()
        self._chk(self.lib.nfk_view_changes(self.h, ctypes.byref(res)))
        n, nv = res.n_calls, res.n_visits
        arr = np.ctypeslib.as_array
        log = arr(res.log, (n, 6)).copy() if n else np.zeros((0, 6), np.int32)
        cv = arr(res.call_visit, (n + 1,)).copy() if n else np.zeros(1, np.uint32)
        vis = arr(res.visit, (nv, 3)).copy() if nv else np.zeros((0, 3), np.int32)
        off = arr(res.visit_off, (2 * nv + 1,)).copy() if nv else np.zeros(1, np.uint32)
        tot = int(off[-1])
        obj = arr(res.obj, (tot,)).copy() if tot else np.zeros(0, np.int32)
        return {"log": log, "call_visit": cv, "visit": vis, "visit_off": off, "obj": obj,
                "kernel_ms": res.kernel_ms, "bytes": res.bytes, "n_host": res.n_host, "n_tiles": res.n_tiles}

    def online_count(self, scene=-1, group=-1):
        n = ctypes.c_int32()
        self._chk(self.lib.nfk_online_count(self.h, int(scene), int(group), ctypes.byref(n)))
        return n.value

    def GetSceneOnLineCount(self, scene, group=-1):
        return self.online_count(scene, group)

    def GetOnLineCount(self):
        return self.online_count()

    # ---- one frame ----
    def Execute(self, now_ms):
        self._chk(self.lib.nfk_execute(self.h, int(now_ms)))
        return True

    def ExecuteCalls(self):
        """nfk_execute_calls: the queued calls applied in a pass where nothing fires (what heartbeat
        functors call inside NFCScheduleModule::Execute's walk, SM:65, SM:83-119)."""
        self._chk(self.lib.nfk_execute_calls(self.h))
        return True

    def synchronize(self):
        self._chk(self.lib.nfk_sync(self.h))

    def summary(self):
        s = Summary()
        self._chk(self.lib.nfk_summary_get(self.h, ctypes.byref(s)))
        return {f: getattr(s, f) for f, _ in Summary._fields_}

    def outputs(self):
        o = Outputs()
        self._chk(self.lib.nfk_outputs_get(self.h, ctypes.byref(o)))
        return {f: getattr(o, f) for f, _ in Outputs._fields_}

    def outputs_raw(self):
        """nfk_outputs_get into one reused struct (device pointers; the frame's dense ranks are
        built asynchronously on the world's stream) — what a consumer calls every frame."""
        if not hasattr(self, "_out"):
            self._out = Outputs()
        self._chk(self.lib.nfk_outputs_get(self.h, ctypes.byref(self._out)))
        return self._out

    # ---- readback ----
    def read_prop(self, pid):
        out = np.zeros(self.n_obj, np.uint64)
        self._chk(self.lib.nfk_read_prop(self.h, pid, _p(out)))
        return out.view(np.int64) if pid < self.n_int else out.view(np.float64)

    def get_props(self, guid_head, guid_data, pid):
        """NFIKernelModule::GetProperty* for n (entity, property) pairs: the value after the last
        frame with this window's queued writes applied (read-your-writes); raw 64-bit patterns."""
        a = [np.ascontiguousarray(x, t) for x, t in ((guid_head, np.int64), (guid_data, np.int64), (pid, np.int32))]
        out = np.zeros(len(a[0]), np.uint64)
        self._chk(self.lib.nfk_get_props(self.h, len(a[0]), *[_p(x) for x in a], _p(out)))
        return out

    # ---- NFCPropertyModule's resource calls (PM:215-472): AddHP / ConsumeHP / EnoughHP / AddMoney / FullHPMP ... ----
    def adjust_props(self, guid_head, guid_data, op, dst, bound, value, stats=None):
        """nfk_adjust_props: n (object, ADJ_* op, dst, bound or -1, int64 value) calls applied in array
        order as the loop get_props / the op's rule / set_props would -> uint8 results (ADJ_RET: the
        reference's return value, ADJ_SET: a Set was queued).  stats: a dict that receives the
        launch's device time (kernel_ms, with set_profiling(True)), the bytes read back, the calls
        answered by the kernel (n_dev) and on the host (n_host) and the Sets queued (n_set)."""
        a = [np.ascontiguousarray(x, t) for x, t in
             ((guid_head, np.int64), (guid_data, np.int64), (op, np.uint8), (dst, np.int32), (bound, np.int32),
              (value, np.int64))]
        out = np.zeros(len(a[0]), np.uint8)
        self._chk(self.lib.nfk_adjust_props(self.h, len(a[0]), *[_p(x) for x in a], _p(out)))
        self._adjust_stats(stats)
        return out

    def adjust_props_obj(self, obj, op, dst, bound, value, stats=None):
        """nfk_adjust_props_obj: adjust_props by object index (query_objects' hits, the outputs' ev_obj)"""
        a = [np.ascontiguousarray(x, t) for x, t in
             ((obj, np.int32), (op, np.uint8), (dst, np.int32), (bound, np.int32), (value, np.int64))]
        out = np.zeros(len(a[0]), np.uint8)
        self._chk(self.lib.nfk_adjust_props_obj(self.h, len(a[0]), *[_p(x) for x in a], _p(out)))
        self._adjust_stats(stats)
        return out

    def _adjust_stats(self, stats):
        if stats is None:
            return
        st = AdjustStats()
        self._chk(self.lib.nfk_adjust_stats(self.h, ctypes.byref(st)))
        stats.update(kernel_ms=st.kernel_ms, bytes=st.bytes, n_dev=st.n_dev, n_host=st.n_host, n_set=st.n_set)

    def GetPropertyInt(self, guid, prop):
        pid = wl.PID[prop] if isinstance(prop, str) else prop
        return int(self.get_props([guid[0]], [guid[1]], [pid]).view(np.int64)[0])

    def GetPropertyFloat(self, guid, prop):
        pid = wl.PID[prop] if isinstance(prop, str) else prop
        return float(self.get_props([guid[0]], [guid[1]], [pid]).view(np.float64)[0])

    def ExistSchedule(self, guid, name):
        kind = wl.KID[name] if isinstance(name, str) else name
        e = ctypes.c_int32()
        self._chk(self.lib.nfk_exist_schedule(self.h, int(guid[0]), int(guid[1]), int(kind), ctypes.byref(e)))
        return bool(e.value)

    def read_record(self, rec):
        cols, rows = self.rec_shape[rec]
        out = np.zeros((self.n_obj, cols, rows), np.uint64)
        self._chk(self.lib.nfk_read_record(self.h, rec, _p(out)))
        return out

    def read_schedules(self):
        nx = np.zeros((self.n_kind, self.n_obj), np.int64)
        rm = np.zeros((self.n_kind, self.n_obj), np.int32)
        st = np.zeros((self.n_kind, self.n_obj), np.uint8)
        self._chk(self.lib.nfk_read_schedules(self.h, _p(nx), _p(rm), _p(st)))
        return nx, rm, st

    def read_schedule_forms(self):
        """[n_kind][n_obj] uint8: 1 where the schedule's device record is wide, 0 compact or absent."""
        wide = np.zeros((self.n_kind, self.n_obj), np.uint8)
        self._chk(self.lib.nfk_read_schedule_forms(self.h, _p(wide)))
        return wide

    def read_tick(self):
        """All outputs of the last frame, entities as object (creation) indices."""
        s = self.summary()
        ne, nr, nf, nm = s["n_prop_events"], s["n_rec_events"], s["n_fired"], s["n_msgs"]
        ev = [np.zeros(ne, np.int32), np.zeros(ne, np.int32), np.zeros(ne, np.uint64), np.zeros(ne, np.uint64)]
        self._chk(self.lib.nfk_read_events(self.h, *[_p(x) for x in ev]))
        re = [np.zeros(nr, np.int32), np.zeros(nr, np.uint32), np.zeros(nr, np.uint64), np.zeros(nr, np.uint64)]
        self._chk(self.lib.nfk_read_rec_events(self.h, *[_p(x) for x in re]))
        fi = [np.zeros(nf, np.int32), np.zeros(nf, np.int32), np.zeros(nf, np.int32)]
        self._chk(self.lib.nfk_read_fired(self.h, *[_p(x) for x in fi]))
        mo = np.zeros(ne + nr + 1, np.uint32)
        mr = np.zeros(nm, np.int32)
        self._chk(self.lib.nfk_read_fanout(self.h, _p(mo), _p(mr)))
        out = dict(ev_obj=ev[0], ev_pid=ev[1], ev_old=ev[2], ev_new=ev[3],
                   re_obj=re[0], re_rrc=re[1], re_old=re[2], re_new=re[3],
                   fi_obj=fi[0], fi_kind=fi[1], fi_rem=fi[2], mo_off=mo, mr_obj=mr, summary=s)
        if self.n_oprops:
            oh = [np.zeros(ne, np.uint64), np.zeros(ne, np.uint64)]
            self._chk(self.lib.nfk_read_events_obj(self.h, *[_p(x) for x in oh]))
            out["ev_oldh"], out["ev_newh"] = oh
        if getattr(self, "rec_has_obj", False):   # the object cells' Update events: their head halves
            rh = [np.zeros(nr, np.uint64), np.zeros(nr, np.uint64)]
            self._chk(self.lib.nfk_read_rec_events_obj(self.h, *[_p(x) for x in rh]))
            out["re_oldh"], out["re_newh"] = rh
        return out

    # ---- per-Set chains (NFIKernelModule::AddPropertyCallBack) ----
    def watch_props(self, pids):
        """nfk_watch_props: the int / f64 properties whose accepted program Sets every Execute logs
        (an empty list watches nothing)"""
        p = np.ascontiguousarray(pids, np.int32)
        self._chk(self.lib.nfk_watch_props(self.h, len(p), _p(p)))

    def read_chain(self):
        """nfk_read_chain: the last Execute's per-Set log in the walk's order (NFGUID, kind, op) as a
        dict of arrays obj, kind, op, pid, old, new"""
        n = ctypes.c_int32()
        self._chk(self.lib.nfk_read_chain(self.h, 0, ctypes.byref(n), None, None, None, None, None, None))
        cap = n.value
        a = [np.zeros(cap, np.int32) for _ in range(4)] + [np.zeros(cap, np.uint64) for _ in range(2)]
        if cap:
            self._chk(self.lib.nfk_read_chain(self.h, cap, ctypes.byref(n), *[_p(x) for x in a]))
        return dict(zip(("obj", "kind", "op", "pid", "old", "new"), a))

    # ---- measurement ----
    def set_profiling(self, on):
        self._chk(self.lib.nfk_set_profiling(self.h, 1 if on else 0))

    def kernel_times(self):
        ms = np.zeros(N_KERNEL_TIMERS, np.float64)
        n = np.zeros(N_KERNEL_TIMERS, np.int64)
        b = np.zeros(N_KERNEL_TIMERS, np.int64)
        self._chk(self.lib.nfk_kernel_times(self.h, _p(ms), _p(n), _p(b)))
        return ms, n, b

    def reset_kernel_times(self):
        self._chk(self.lib.nfk_reset_kernel_times(self.h))


def jit_preview(w, compile=False):
    """nfk_jit_preview: the k_tick schema policy (JitSchema source) nfk_commit would generate for a
    workload's schema, and with compile=True whether hipRTC builds k_tick<.., JitSchema> for gfx950
    from it.  Needs no GPU.  Returns (source, ok, message)."""
    lib = load_library()
    _, n_int, n_flt, n_cls, n_kind = (int(x) for x in w["cfg"][:5])
    flags = np.ascontiguousarray(np.asarray(w["prop_flags"])[:n_cls], np.uint8)
    src_ops = np.asarray(w["ops"][:n_kind])
    if src_ops.dtype != wl.OP_DTYPE:  # (raw records from a workload file)
        src_ops = src_ops.view(wl.OP_DTYPE).reshape(n_kind, -1)
    ops = np.zeros((n_kind, NFK_MAX_OPS), wl.OP_DTYPE)  # [n_kind][NFK_MAX_OPS] (nfgpu.h)
    ops[:, :src_ops.shape[1]] = src_ops
    n_ops = np.ascontiguousarray(w["n_ops"][:n_kind], np.int32)
    ok = ctypes.c_int32()
    src = ctypes.create_string_buffer(1 << 20)
    msg = ctypes.create_string_buffer(1 << 16)
    n_rec = int(w["cfg"][5])
    if n_rec:  # the records' shapes: a policy with guard cells (NFK_GUARD_CELL) holds them as literals
        rows = np.ascontiguousarray(w["rec_rows"][:n_rec], np.int32)
        cols = np.ascontiguousarray(w["rec_cols"][:n_rec], np.int32)
        ct = np.zeros((n_rec, wl.MAX_REC_COLS), np.uint8)
        ct[:, :] = np.asarray(w["rec_ctype"], np.uint8).reshape(n_rec, -1)[:, :wl.MAX_REC_COLS]
        rc = lib.nfk_jit_preview_rec(n_int, n_flt, n_cls, n_kind, _p(flags), _p(ops), _p(n_ops), n_rec, _p(rows),
                                     _p(cols), _p(ct), int(compile), ctypes.byref(ok), src, len(src), msg, len(msg))
    else:
        rc = lib.nfk_jit_preview(n_int, n_flt, n_cls, n_kind, _p(flags), _p(ops), _p(n_ops), int(compile),
                                 ctypes.byref(ok), src, len(src), msg, len(msg))
    if rc != NFK_OK:
        raise NFKError(rc, lib.nfk_last_error().decode())
    return src.value.decode(), bool(ok.value), msg.value.decode()


def world_from_workload(w, capacity=None, msg_capacity=0, stream=None, slack_per_256=0):
    """Build an NFKernelModule from a workload dict (see workload.make_world): classes,
    kinds, objects, creation-time values, then the AddSchedule calls made before frame 0."""
    cfg = w["cfg"]
    n_obj, n_int, n_flt, n_cls, n_kind, n_rec = (int(x) for x in cfg[:6])
    n_op = int(w["n_oprops"][0]) if "n_oprops" in w else 0
    m = NFKernelModule(capacity or n_obj, n_int, n_flt, n_cls, n_kind, n_rec, msg_capacity, stream, slack_per_256,
                       n_op)
    if "scene_props" in w:
        m.set_scene_props(*(int(x) for x in w["scene_props"]))
    m.cur_scene = np.array(w["scene"], np.int32)   # membership as SwitchScene calls change it
    m.cur_group = np.array(w["group"], np.int32)
    for c in range(n_cls):
        m.set_prop_flags(c, w["prop_flags"][c])
    for r in range(n_rec):
        m.define_record(r, int(w["rec_rows"][r]), int(w["rec_cols"][r]), w["rec_ctype"][r],
                        w["rec_flags"][:, r])
    for k in range(n_kind):
        m.define_kind(k, w["ops"][k][: int(w["n_ops"][k])])
    # objects created before frame 0 (a workload's later objects, born[o] >= 0, are the last ones
    # and enter through nfk_spawn_objects in their window: run_workload)
    n0 = int(np.sum(w["born"] < 0)) if "born" in w else n_obj
    m.create_objects(w["guid_head"][:n0], w["guid_data"][:n0], w["scene"][:n0], w["group"][:n0], w["cls"][:n0],
                     w["is_player"][:n0])
    for p in range(n_int):
        m.load_prop(p, w["init_i"][p][:n0])
    for p in range(n_flt):
        m.load_prop(n_int + p, w["init_f"][p][:n0])
    for p in range(n_op):
        m.load_object(n_int + n_flt + p, w["init_oh"][p][:n0], w["init_od"][p][:n0])
    for r in range(n_rec):
        m.load_record(r, w[f"rec{r}_cells"][:n0], w[f"rec{r}_used"][:n0])
    m.commit()
    gh, gd = w["guid_head"], w["guid_data"]
    so = w["s_obj"]
    m.add_schedules(gh[so], gd[so], w["s_kind"], w["s_interval"], w["s_count"], w["s_time"])
    return m


def run_workload(m, w, tick, collect=True):
    """Replay the between-frame calls of frame `tick` in the oracle's window order — CreateObject
    (nfk_spawn_objects), SwitchScene, schedule calls, SetProperty calls, SetRecord calls,
    DestroyObject — then Execute it."""
    gh, gd = w["guid_head"], w["guid_data"]
    if "born" in w:
        new = np.nonzero(w["born"] == tick)[0]
        if len(new):
            parts = [w["init_i"][:, new].astype(np.int64).view(np.uint64),
                     w["init_f"][:, new].astype(np.float64).view(np.uint64)]
            if m.n_oprops:   # each object property as (data, head)
                od = w["init_od"][:, new].astype(np.int64).view(np.uint64)
                oh = w["init_oh"][:, new].astype(np.int64).view(np.uint64)
                parts.append(np.stack([od, oh], 1).reshape(-1, len(new)))
            props = np.concatenate(parts).T
            m.spawn_objects(gh[new], gd[new], w["scene"][new], w["group"][new], w["cls"][new], w["is_player"][new],
                            np.ascontiguousarray(props))
    if "sw_tick" in w:
        for i in np.nonzero(w["sw_tick"] == tick)[0]:
            o = int(w["sw_obj"][i])
            sc, gr = int(w["sw_scene"][i]), int(w["sw_group"][i])
            if sc < 0:   # the object's own cell
                sc, gr = int(m.cur_scene[o]), int(m.cur_group[o])
            m.SwitchScene((int(gh[o]), int(gd[o])), sc, gr, w["sw_x"][i], w["sw_y"][i], w["sw_z"][i])
            m.cur_scene[o], m.cur_group[o] = sc, gr
    # (by_object: the calls by nfk object index — nfk_set_props_obj / nfk_schedule_calls_obj — which
    # in a world without objects created after commit is the workload's object index)
    by_object = os.environ.get("NFGPU_TEST_BY_OBJECT") == "1" and "born" not in w
    hsel = np.nonzero(w["h_tick"] == tick)[0]
    if len(hsel):   # call order preserved
        ho = w["h_obj"][hsel]
        if by_object:
            m.schedule_calls_obj(w["h_op"][hsel], ho, w["h_kind"][hsel], w["h_interval"][hsel], w["h_count"][hsel],
                                 w["h_time"][hsel])
        else:
            m.schedule_calls(w["h_op"][hsel], gh[ho], gd[ho], w["h_kind"][hsel], w["h_interval"][hsel],
                             w["h_count"][hsel], w["h_time"][hsel])
    xsel = np.nonzero(w["x_tick"] == tick)[0]
    if len(xsel):
        mode = w["x_mode"][xsel] if "x_mode" in w else np.zeros(len(xsel), np.uint8)
        # runs of plain SetProperty calls go as one batch; a read-modify-write call (mode 1:
        # SetProperty(p, GetProperty(p) + delta)) reads through nfk_get_props first
        cut = np.nonzero(np.diff(np.concatenate([[2], mode, [2]])))[0]
        for a, b in zip(cut[:-1], cut[1:]):
            sel = xsel[a:b]
            xo = w["x_obj"][sel]
            if mode[a] == 0:
                pid = w["x_pid"][sel]
                isobj = pid >= m.n_int + m.n_flt
                # (calls on different properties never interact: the object calls go as their own batch)
                if (~isobj).any() and by_object:
                    m.set_props_obj(xo[~isobj], pid[~isobj], w["x_bits"][sel][~isobj])
                elif (~isobj).any():
                    m.set_props(gh[xo[~isobj]], gd[xo[~isobj]], pid[~isobj], w["x_bits"][sel][~isobj])
                if isobj.any():
                    m.set_objects(gh[xo[isobj]], gd[xo[isobj]], pid[isobj], w["x_bits_h"][sel][isobj].view(np.int64),
                                  w["x_bits"][sel][isobj].view(np.int64))
                continue
            for i in sel:
                o, p = int(w["x_obj"][i]), int(w["x_pid"][i])
                cur = m.get_props([gh[o]], [gd[o]], [p])
                d = w["x_bits"][i:i + 1]
                if p < m.n_int:
                    v = (cur.view(np.int64) + d.view(np.int64)).view(np.uint64)
                else:
                    v = (cur.view(np.float64) + d.view(np.float64)).view(np.uint64)
                m.set_props([gh[o]], [gd[o]], [p], v)
    if "r_tick" in w:   # SetRecordInt / SetRecordFloat calls (typed by their column), row operations
        rsel = np.nonzero(w["r_tick"] == tick)[0]
        if len(rsel):
            ops = w["r_op"][rsel] if "r_op" in w else np.zeros(len(rsel), np.uint8)
            cut = np.nonzero(np.diff(np.concatenate([[-1], (ops != 0).astype(np.int8), [-1]])))[0]
            for a, b in zip(cut[:-1], cut[1:]):   # runs of Sets / of row operations, in call order
                sel = rsel[a:b]
                ro = w["r_obj"][sel]
                if ops[a] == 0:
                    m.set_records(gh[ro], gd[ro], w["r_rec"][sel], w["r_row"][sel], w["r_col"][sel], w["r_bits"][sel])
                else:
                    m.record_rows(gh[ro], gd[ro], w["r_rec"][sel], ops[a:b].astype(np.int32), w["r_row"][sel],
                                  w["r_vals"][sel])
    if "d_tick" in w:
        dead = w["d_obj"][w["d_tick"] == tick]
        if len(dead):
            m.destroy_objects(gh[dead], gd[dead])
    now = int(w["tick_time"][tick])
    if now == np.iinfo(np.int64).min:  # a calls-only pass (nfk_execute_calls: nothing fires)
        m.ExecuteCalls()
    else:
        m.Execute(now)
    return m.read_tick() if collect else None
