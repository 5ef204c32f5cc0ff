"""bench.py's own host bookkeeping (CPU): the migration harness's row queue."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("nf_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_row_queue_is_fifo():
    """RowQueue.take / append against a plain list model: the oldest rows leave first, arrivals
    queue behind them, short takes return what is left, an empty queue returns None."""
    RowQueue = _bench().RowQueue
    rng = np.random.default_rng(5)
    start = np.arange(1000 * 5, dtype=np.int64).reshape(1000, 5)
    q, model, nxt = RowQueue(start), [tuple(r) for r in start], 10 ** 6
    for _ in range(300):
        if rng.random() < 0.5:
            k = int(rng.integers(0, 40))
            rows = np.arange(nxt, nxt + 5 * k, dtype=np.int64).reshape(k, 5)
            nxt += 5 * k
            q.append(rows)
            model += [tuple(r) for r in rows]
        else:
            n = int(rng.integers(1, 90))
            got = q.take(n)
            want, model = model[:n], model[n:]
            if not want:
                assert got is None
            else:
                assert [tuple(r) for r in got] == want
        assert len(q) == len(model)
    assert q.take(len(model) + 5) is not None or not model
    assert len(q) == 0 and q.take(3) is None


class _FakeWorld:
    """What dump_outputs reads of a world: one frame's read_tick arrays and the property columns."""
    n_int, n_flt = 2, 1

    def __init__(self, n_obj, n_ev, n_msg):
        self.n_obj, self.n_ev, self.n_msg = n_obj, n_ev, n_msg

    def read_tick(self):
        ne, nm = self.n_ev, self.n_msg
        pid = (np.arange(ne) % 3).astype(np.int32)
        val = np.where(pid < 2, (np.arange(ne, dtype=np.int64) - 5).view(np.uint64),
                       (np.arange(ne) * 0.5).view(np.uint64))
        z32, z64 = np.zeros(0, np.int32), np.zeros(0, np.uint64)
        return dict(ev_obj=np.arange(ne, dtype=np.int32), ev_pid=pid, ev_old=val, ev_new=val,
                    re_obj=z32, re_rrc=z32.view(np.uint32), re_old=z64, re_new=z64,
                    fi_obj=np.arange(7, dtype=np.int32), fi_kind=np.zeros(7, np.int32), fi_rem=np.ones(7, np.int32),
                    mo_off=np.arange(ne + 1, dtype=np.uint32), mr_obj=np.arange(nm, dtype=np.int32), summary={})

    def read_prop(self, pid):
        a = np.arange(self.n_obj, dtype=np.int64) + pid
        return a if pid < self.n_int else a.astype(np.float64) / 4


def test_dump_outputs_writes_float64_arrays_within_the_size_limit(tmp_path):
    """--dump-outputs: every array of the frame as float64 DIR/<name>.npy, property values decoded by
    type; small outputs whole, large ones cut to the same seeded sample on every run, under 64 MB."""
    b = _bench()
    b.dump_outputs(str(tmp_path / "small"), _FakeWorld(100, 9, 40))
    got = {p.name[:-4]: np.load(p) for p in (tmp_path / "small").iterdir()}
    assert all(a.dtype == np.float64 and a.size for a in got.values())
    assert not any(k.startswith("re_") for k in got)   # no record events in the frame: no empty files
    assert {"ev_obj", "ev_pid", "ev_old", "ev_new", "fi_obj", "mo_off", "mr_obj", "prop_00", "prop_02"} <= set(got)
    assert got["ev_old"].tolist() == [-5.0, -4.0, 1.0, -2.0, -1.0, 2.5, 1.0, 2.0, 4.0]
    assert got["mr_obj"].tolist() == list(range(40)) and got["prop_02"][:3].tolist() == [0.5, 0.75, 1.0]
    big = _FakeWorld(1 << 20, 1 << 20, 6 << 20)   # 8 * (6 + 8) MiB of float64 and more: over the limit
    b.dump_outputs(str(tmp_path / "a"), big)
    b.dump_outputs(str(tmp_path / "b"), big)
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert files == sorted(p.name for p in (tmp_path / "b").iterdir())
    assert sum((tmp_path / "a" / f).stat().st_size for f in files) <= 64 * 10 ** 6
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
    mr = np.load(tmp_path / "a" / "mr_obj.npy")
    assert 0 < len(mr) < (6 << 20) and np.all(np.diff(mr) > 0)   # a sample, in order
    assert len(np.load(tmp_path / "a" / "fi_obj.npy")) == 7     # short arrays stay whole


def test_gpus_flag_starts_the_ranks(tmp_path):
    """`bench.py --gpus N` without a launcher starts N rank processes with the launcher's
    environment (RANK, LOCAL_RANK, WORLD_SIZE = N, rendezvous on 127.0.0.1); a launched rank
    whose WORLD_SIZE disagrees with --gpus refuses to run."""
    import json
    import pytest
    b = _bench()
    probe = tmp_path / "probe.py"
    probe.write_text("import json, os, sys\n"
                     "keys = ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT')\n"
                     "open(sys.argv[1] + os.environ['RANK'], 'w').write(json.dumps({k: os.environ[k] for k in keys}))\n")
    assert b.spawn_ranks(3, [str(tmp_path / "r")], script=str(probe)) == 0
    seen = [json.loads((tmp_path / f"r{i}").read_text()) for i in range(3)]
    assert [s["RANK"] for s in seen] == ["0", "1", "2"] and [s["LOCAL_RANK"] for s in seen] == ["0", "1", "2"]
    assert {s["WORLD_SIZE"] for s in seen} == {"3"} and {s["MASTER_ADDR"] for s in seen} == {"127.0.0.1"}
    assert len({s["MASTER_PORT"] for s in seen}) == 1
    os.environ.pop("WORLD_SIZE", None)
    assert b.world_from_env(1) == (1, 0, 0)
    try:
        os.environ["WORLD_SIZE"] = "2"
        with pytest.raises(SystemExit):
            b.world_from_env(4)
    finally:
        os.environ.pop("WORLD_SIZE", None)


def test_a_failing_rank_stops_the_others(tmp_path):
    """If one rank fails, bench.py stops the others (by PID) and exits with that rank's code
    instead of waiting for a collective that can never complete."""
    import time
    b = _bench()
    probe = tmp_path / "probe.py"
    probe.write_text("import os, sys, time\n"
                     "if os.environ['RANK'] == '1':\n    sys.exit(3)\n"
                     "time.sleep(120)\n")
    t = time.time()
    assert b.spawn_ranks(2, [], script=str(probe)) == 3
    assert time.time() - t < 60
