"""CPU: synthetic world invariants the parity tests rely on."""
import numpy as np

from noahgameframe_amd import workload as wl


def test_kind_ids_follow_lexical_schedule_names():
    assert wl.KINDS == sorted(wl.KINDS)


def test_world_shapes_and_uniqueness():
    w = wl.make_world(n_obj=1000, n_scenes=2, groups_per_scene=5, players_per_group=3, n_ticks=4, seed=3,
                      records=True, rec_rows=32)
    n = 1000
    guid = set(zip(w["guid_head"].tolist(), w["guid_data"].tolist()))
    assert len(guid) == n
    assert w["init_i"].shape == (wl.N_INT, n) and w["init_f"].shape == (wl.N_FLT, n)
    assert w["rec0_cells"].shape == (n, 3, 32)
    assert np.all(w["rec0_used"] < (1 << 32))
    cells = set(zip(w["scene"].tolist(), w["group"].tolist()))
    assert len(cells) == 10
    for c in cells:
        m = (w["scene"] == c[0]) & (w["group"] == c[1])
        assert w["is_player"][m].sum() == min(3, m.sum())
    assert np.all(np.diff(w["x_tick"]) >= 0) and np.all(np.diff(w["h_tick"]) >= 0)


def _digest(w):
    import hashlib
    m = hashlib.sha256()
    for k in sorted(w):
        a = np.ascontiguousarray(w[k])
        for part in (k.encode(), str(a.dtype).encode(), str(a.shape).encode(), a.tobytes()):
            m.update(part)
    return m.hexdigest()


def test_destroy_only_world_generates_and_others_are_unchanged():
    """destroy_frac > 0 with spawn_frac == 0 (no late objects: their AddSchedule times have no minimum)
    generates; a world with both is byte for byte what it was before that case was handled (the digest
    was taken from the generator as it stood: test_oracle.py's seed 9)"""
    w = wl.make_world(n_obj=200, n_scenes=1, groups_per_scene=3, players_per_group=2, n_ticks=6, seed=2,
                      destroy_frac=0.1, switch_frac=0.05)
    assert len(w["d_obj"]) == 100 and not np.any(w["born"] >= 0) and int(w["cfg"][0]) == 200
    w = wl.make_world(n_obj=700, n_scenes=3, groups_per_scene=4, players_per_group=3, ext_frac=0.05, host_ops=True,
                      sched_edges=True, switch_frac=0.02, switch_new_groups=True, rmw_frac=0.02, spawn_frac=0.03,
                      destroy_frac=0.03, n_ticks=9, seed=9)
    assert _digest(w) == "993966de1374474364eba0a215d4c12b9663807d42a12f37f4985d0b157d0796"


def test_programs_only_write_declared_columns():
    ops, n = wl.programs(True)
    dst = {int(ops[k, i]["dst"]) for k in range(len(wl.KINDS)) for i in range(n[k])
           if ops[k, i]["code"] in (wl.OP_IADD_CLAMP, wl.OP_FLERP, wl.OP_FAFFINE)}
    assert len(dst) <= 8
