"""GPU: k_tick's direct window — a tile whose short recipient runs all fit in LDS beside its staged
players has every thread write its own events' recipients straight into the window, with no event
triples, no event loop and no window passes (nfgpu_tick.hpp) — against the oracle and, array for
array, against the same world with the triples forced for every tile (NFGPU_ABLATE=1<<16), on the
hipRTC and the library kernels."""
import numpy as np
import pytest

from noahgameframe_amd import workload
from tests.parity import compare_runs, run_oracle
from tests.test_gpu_rank_in_tick import run_frames

pytestmark = pytest.mark.gpu

FAN_TRIPLES = 1 << 16   # kAblFanTriples: the event triples and window passes for every tile (outputs exact)
FAN_WIN16 = 1 << 24     # kAblFanWin16: the LDS window for runs of up to 16 recipients
FAN_WIN32 = 1 << 25     # kAblFanWin32: ... of up to 32
WAVES8 = 32             # kAblWaves8: the library kernel at 8 waves per SIMD (a smaller LDS share)
JIT = pytest.mark.parametrize("jit", ["1", "0"], ids=["hiprtc", "library"])


def check(monkeypatch, w, jit, ablate=0):
    """the world equals the oracle, and equals itself fanned out through the triples in every array
    (mr_obj, mo_off, msg_cnt, msg_base, the summaries' byte tallies and the rest)"""
    monkeypatch.setenv("NFGPU_JIT", jit)
    monkeypatch.setenv("NFGPU_ABLATE", str(ablate))
    got, tiles, _ = run_frames(w)
    compare_runs(got, run_oracle(w))
    monkeypatch.setenv("NFGPU_ABLATE", str(ablate | FAN_TRIPLES))
    ref, ref_tiles, _ = run_frames(w)
    assert ref_tiles == tiles
    assert sorted(ref) == sorted(got)
    compare_runs(got, ref)
    return got, tiles


def msg_counts(got, tiles):
    """the property tiles' message counts of every frame"""
    return np.concatenate([got[f"rk_t{t}_msg_cnt"][:nt] for t, nt in enumerate(tiles)])


@JIT
def test_several_groups_per_tile_and_a_partial_last_tile(gpu_available, monkeypatch, jit):
    """700 entities in groups of about 30 with 3 players: a tile's threads sit at different places of
    its staged player run, players and NPCs mix, and a player is first, middle or last of its group's
    run (the skip-self rule at each place); 2 full tiles and a partial one"""
    w = workload.make_world(n_obj=700, n_scenes=1, groups_per_scene=23, players_per_group=3, n_ticks=4, seed=51)
    assert int(w["is_player"].sum()) == 3 * 23
    got, tiles = check(monkeypatch, w, jit)
    assert all(t >= 3 for t in tiles) and msg_counts(got, tiles).max() > 0


@JIT
def test_tiles_without_messages_beside_tiles_with(gpu_available, monkeypatch, jit):
    """frames 1 and 2 are calls-only passes with few Sets: most tiles have no message (or are not run at
    all), beside tiles with a handful"""
    w = workload.make_world(n_obj=3000, n_scenes=1, groups_per_scene=12, players_per_group=4, n_ticks=4, seed=52,
                            host_ops=True, ext_frac=0.004)
    tt = np.asarray(w["tick_time"]).copy()
    tt[[1, 2]] = np.iinfo(np.int64).min
    w["tick_time"] = tt
    got, tiles = check(monkeypatch, w, jit)
    for t in (1, 2):
        c = got[f"rk_t{t}_msg_cnt"][:tiles[t]]
        assert (c == 0).any() and (c > 0).any(), c


@JIT
def test_standalone_sets_beside_program_destinations(gpu_available, monkeypatch, jit):
    """queued Sets of program destinations, of other properties (standalone events, merged in
    property-id order by the walk) and read-modify-write Sets, in the same entities"""
    w = workload.make_world(n_obj=1500, n_scenes=1, groups_per_scene=10, players_per_group=5, n_ticks=4, seed=53,
                            host_ops=True, ext_frac=0.3, rmw_frac=0.1, ext_props="all")
    check(monkeypatch, w, jit)


@JIT
def test_direct_and_windowed_tiles_in_one_frame(gpu_available, monkeypatch, jit):
    """8 waves per SIMD leave 163840 / 8 - 2560 bytes (rounded down to 1 KiB: 4352 words) for the
    window and the staged players; some tiles' runs of a frame pass it, others stay below"""
    monkeypatch.setenv("NFGPU_JIT_WAVES", "8")
    w = workload.make_world(n_obj=6000, n_scenes=1, groups_per_scene=24, players_per_group=8, n_ticks=3, seed=54,
                            host_ops=True, ext_frac=0.02)
    got, tiles = check(monkeypatch, w, jit, ablate=WAVES8)
    R = ((163840 // 8 - 2560) & ~1023) // 4
    players = int(w["is_player"].sum())   # (no tile stages more players than the world has)
    c = msg_counts(got, tiles)
    print("window", R, "players", players, "tile messages", sorted(c))
    assert ((c > 0) & (c <= ((R - players) & ~3))).any(), "no tile fits the direct window"
    assert (c > R).any(), "no tile falls back to the window passes"
    # a chunk of triples holds at most R / 6 events (rounded up to 4) when the window takes the other half
    ev = np.concatenate([np.diff(got[f"rk_t{t}_ev_base"][:nt + 1].astype(np.int64)) for t, nt in enumerate(tiles)])
    print("tile events", sorted(ev)[-4:], "chunk capacity", (R // 6 + 3) & ~3)
    assert (ev > ((R // 6 + 3) & ~3)).any(), "no tile takes several chunks of triples"


@pytest.mark.parametrize("ablate", [0, FAN_WIN16], ids=["win8", "win16"])
@pytest.mark.parametrize("ppg", [8, 9, 10])
@JIT
def test_run_lengths_at_the_window_threshold(gpu_available, monkeypatch, jit, ppg, ablate):
    """8 and 9 players per group: runs of up to 8 recipients (L = 8), the window; 10: runs of 9
    (L = 16), lane groups by default and, under kAblFanWin16, a window run in two 8-recipient parts"""
    w = workload.make_world(n_obj=1200, n_scenes=1, groups_per_scene=6, players_per_group=ppg, n_ticks=3, seed=55)
    check(monkeypatch, w, jit, ablate=ablate)


@JIT
def test_long_runs_in_the_window(gpu_available, monkeypatch, jit):
    """20 players per group under kAblFanWin32: runs of 19 and 20 recipients, three 8-recipient parts"""
    w = workload.make_world(n_obj=600, n_scenes=1, groups_per_scene=3, players_per_group=20, n_ticks=3, seed=56)
    check(monkeypatch, w, jit, ablate=FAN_WIN32)


@JIT
def test_a_group_with_one_player(gpu_available, monkeypatch, jit):
    """the only player's public events have no recipient; the NPCs' go to that one player"""
    w = workload.make_world(n_obj=900, n_scenes=1, groups_per_scene=7, players_per_group=1, n_ticks=4, seed=57)
    check(monkeypatch, w, jit)


@JIT
def test_private_properties_only(gpu_available, monkeypatch, jit):
    """calls-only frames whose Sets change Camp alone: private for an NPC (one message, to itself),
    public for the group's only player (no recipient)"""
    w = workload.make_world(n_obj=900, n_scenes=1, groups_per_scene=7, players_per_group=1, n_ticks=3, seed=58,
                            host_ops=True, ext_frac=0.3, ext_props=[workload.PID["Camp"]])
    w["tick_time"] = np.full(len(w["tick_time"]), np.iinfo(np.int64).min, np.int64)
    got, tiles = check(monkeypatch, w, jit)
    assert msg_counts(got, tiles).max() > 0


NO_FUSE = 4096          # kAblNoFuse: the fan-out in k_fanout, after k_tick (outputs exact)
K_FAN_LDS = 2048        # kFanLds: the players k_fanout stages in LDS
R_MAX = 7424            # the largest LDS share of k_tick in words: (163840 / 5 - 2560 rounded down to 1 KiB) / 4


@JIT
def test_a_player_run_too_long_to_stage(gpu_available, monkeypatch, jit):
    """one group of 2100 players: above k_fanout's kFanLds = 2048 staged players and above a quarter of
    the largest LDS share k_tick gets at 5 waves per SIMD (7424 words: 1856), so every tile expands its
    runs from the players in global memory; once more with the fan-out in k_fanout"""
    w = workload.make_world(n_obj=2400, n_scenes=1, groups_per_scene=1, players_per_group=2100, n_ticks=2, seed=59)
    assert len(np.unique(w["scene"])) == 1 and len(np.unique(w["group"])) == 1   # the only group
    players = int(w["is_player"].sum())
    assert players == 2100 and players > K_FAN_LDS and players > R_MAX // 4
    ref = run_oracle(w)
    check(monkeypatch, w, jit)
    monkeypatch.setenv("NFGPU_ABLATE", str(NO_FUSE))
    got, _, _ = run_frames(w)
    compare_runs(got, ref)
