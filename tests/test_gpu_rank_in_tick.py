"""GPU: the frame's dense ranks (ev_base / fi_base / msg_base and the frame totals) written by k_tick's
rank workgroups — extra workgroups of the k_tick launch that poll the counts every tile publishes
before its fan-out (nfgpu_tick.hpp, Dev::lb_rank) — against the oracle and, array for array, against the
same world ranked by k_scan_tiles (NFGPU_ABLATE=1<<28), on the hipRTC and the library kernels."""
import ctypes

import numpy as np
import pytest

from noahgameframe_amd import kernel, workload
from tests.parity import compare_runs, run_oracle

pytestmark = pytest.mark.gpu

SCAN_KERNEL = 1 << 28   # kAblScanKernel: dense ranks by k_scan_tiles for every world (outputs exact)
RANK_PER_1 = 1 << 23    # kAblRankPer1: a rank thread takes one count per pass (outputs exact)
SMALL_TILES = 256       # worlds up to this many tiles ranked through an arrival counter before
JIT = pytest.mark.parametrize("jit", ["1", "0"], ids=["hiprtc", "library"])


def _dev(ptr, n, dtype):
    """n elements of a device array (the world's stream is idle)"""
    out = np.zeros(n, dtype)
    if n:
        rc = kernel.load_library().hipMemcpy(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(ptr),
                                             ctypes.c_size_t(out.nbytes), ctypes.c_int(2))
        assert rc == 0, f"hipMemcpy: {rc}"
    return out


def run_frames(w, slack_per_256=0):
    """tests.parity.run_gpu, with the consumer's read of every frame (nfk_outputs_get first, as the
    plugin and the benchmark do: that is the read k_scan_tiles was launched for) — its base arrays and
    per-tile message counts read back — and the frame's summary.  Returns (outputs, tile counts,
    k_scan_tiles launches)."""
    m = kernel.world_from_workload(w, slack_per_256=slack_per_256)
    m.set_profiling(True)   # (counts the launches of each kernel)
    out, tiles = {}, []
    for t in range(int(w["cfg"][7])):
        kernel.run_workload(m, w, t, collect=False)
        o = m.outputs()
        m.synchronize()
        nt, nrt = o["n_tiles"], o["n_rtiles"]
        tiles.append(nt)
        out[f"rk_t{t}_ev_base"] = _dev(o["ev_base"], nt + 1, np.uint32)
        out[f"rk_t{t}_fi_base"] = _dev(o["fi_base"], nt + 1, np.uint32)
        out[f"rk_t{t}_re_base"] = _dev(o["re_base"], nrt + 1, np.uint32)
        out[f"rk_t{t}_msg_base"] = _dev(o["msg_base"], nt + nrt + 1, np.uint32)
        out[f"rk_t{t}_msg_cnt"] = _dev(o["msg_cnt"], nt + nrt, np.uint32)
        r = m.read_tick()
        s = r.pop("summary")
        assert s["device_error"] == 0, s
        # (the byte tallies are sums of per-workgroup atomics: equal too, the tiles do the same work)
        out[f"rk_t{t}_summary"] = np.array([s[k] for k in sorted(s)], np.int64)
        for k in ("ev_obj", "ev_pid", "ev_old", "ev_new", "re_obj", "re_rrc", "re_old", "re_new",
                  "fi_obj", "fi_kind", "fi_rem"):
            pfx, nm = k.split("_", 1)
            out[f"{pfx}_t{t}_{nm}"] = r[k]
        out[f"mo_t{t}_off"] = r["mo_off"]
        out[f"mr_t{t}_obj"] = r["mr_obj"]
    n_int, n_flt, n_rec = int(w["cfg"][1]), int(w["cfg"][2]), int(w["cfg"][5])
    out["final_i"] = np.stack([m.read_prop(p) for p in range(n_int)])
    out["final_f"] = np.stack([m.read_prop(n_int + p) for p in range(n_flt)])
    for r in range(n_rec):
        out[f"final_rec{r}"] = m.read_record(r)
    nx, rm, st = m.read_schedules()
    out["final_s_next"] = nx
    out["final_s_remain"] = rm
    out["final_s_present"] = (st & 1).astype(np.uint8)
    scans = int(m.kernel_times()[1][kernel.KERNEL_TIMER_NAMES.index("k_scan_tiles")])
    m.close()
    return out, tiles, scans


def check(monkeypatch, w, jit, ablate=0, slack_per_256=0, large=True, ranked_in_tick=True):
    """the world equals the oracle, and equals itself ranked by k_scan_tiles in every array"""
    monkeypatch.setenv("NFGPU_JIT", jit)
    monkeypatch.setenv("NFGPU_ABLATE", str(ablate))
    got, tiles, scans = run_frames(w, slack_per_256)
    assert (scans == 0) if ranked_in_tick else (scans >= len(tiles)), scans
    assert all(t > SMALL_TILES for t in tiles) if large else all(0 < t <= SMALL_TILES for t in tiles), tiles
    compare_runs(got, run_oracle(w))
    monkeypatch.setenv("NFGPU_ABLATE", str(ablate | SCAN_KERNEL))
    ref, ref_tiles, ref_scans = run_frames(w, slack_per_256)
    assert ref_tiles == tiles and ref_scans >= len(tiles)
    assert sorted(ref) == sorted(got)
    compare_runs(got, ref)
    return got, tiles


@JIT
def test_just_over_the_small_world_bound(gpu_available, monkeypatch, jit):
    """257 or more tiles, the last one partial, 4 frames: one epoch's counts must not satisfy the next
    frame's poll (every frame's counts differ: the heartbeats' periods do)."""
    w = workload.make_world(n_obj=66_003, n_scenes=1, groups_per_scene=258, players_per_group=8, n_ticks=4, seed=41)
    got, _ = check(monkeypatch, w, jit)
    assert len({got[f"rk_t{t}_ev_base"][-1] for t in range(4)}) > 1


@JIT
def test_several_passes_with_a_carry(gpu_available, monkeypatch, jit):
    """about 600 tiles at one count per rank thread and pass: three passes, the last one partial"""
    w = workload.make_world(n_obj=150_000, n_scenes=2, groups_per_scene=290, players_per_group=6, n_ticks=3, seed=42)
    _, tiles = check(monkeypatch, w, jit, ablate=RANK_PER_1)
    assert all(2 * 256 < t < 3 * 256 for t in tiles), tiles


@JIT
def test_slack_slots_and_membership_rebuilds(gpu_available, monkeypatch, jit):
    """default slack and SwitchScene calls: dead slots, and rebuilds that change n_tiles between frames"""
    w = workload.make_world(n_obj=70_000, n_scenes=2, groups_per_scene=140, players_per_group=5, n_ticks=6, seed=43,
                            switch_frac=0.02, switch_new_groups=True)
    assert len(w["sw_tick"]) > 0
    check(monkeypatch, w, jit)


@JIT
def test_calls_only_pass_publishes_every_tile(gpu_available, monkeypatch, jit):
    """frames 1 and 3 are nfk_execute_calls passes: k_tick runs only the tiles with SetProperty groups,
    and the tiles it skips must still publish (zero) counts for the rank workgroups"""
    w = workload.make_world(n_obj=70_000, n_scenes=2, groups_per_scene=140, players_per_group=5, n_ticks=5, seed=44,
                            host_ops=True, ext_frac=0.05)
    tt = np.asarray(w["tick_time"]).copy()
    tt[[1, 3]] = np.iinfo(np.int64).min
    w["tick_time"] = tt
    check(monkeypatch, w, jit)


@pytest.mark.parametrize("path", ["k_tick", "k_tick_dyn", "k_tick_touch"])
def test_small_world(gpu_available, monkeypatch, path):
    """3,000 entities: a small world ranks through the same rank workgroups (one count per thread);
    equal to the oracle on all three k_tick paths (k_tick_touch frames rank by k_scan_tiles)"""
    w = workload.make_world(n_obj=3000, n_scenes=2, groups_per_scene=6, players_per_group=3, n_ticks=6, seed=45)
    check(monkeypatch, w, "0" if path == "k_tick_dyn" else "1", ablate=8 if path == "k_tick_touch" else 0, large=False,
          ranked_in_tick=path != "k_tick_touch")


@JIT
def test_record_world_ranks_by_the_scan_kernel(gpu_available, monkeypatch, jit):
    """a world with record ops: its counts come from k_records too, so its frames keep k_scan_tiles"""
    w = workload.make_world(n_obj=3000, n_scenes=2, groups_per_scene=6, players_per_group=3, n_ticks=6, seed=46,
                            records=True, rec_rows=16)
    check(monkeypatch, w, jit, large=False, ranked_in_tick=False)
