"""bench.py --dump-outputs on synthetic result arrays (no GPU): float32 / float64 files only, the 64 MB budget, the schedule
digest recoverable exactly, schedules masked past their length and for unsolved instances, and a fixed sample."""
import os

import numpy as np

import bench


def _results(n, na, cap, seed=1):
    rng = np.random.default_rng(seed)
    ra = dict(status=rng.integers(0, 3, n).astype(np.int32), cost=rng.integers(0, 500, n).astype(np.int64),
              makespan=rng.integers(0, 60, n).astype(np.int64), hl_expanded=rng.integers(0, 9, n).astype(np.int64),
              ll_expanded=rng.integers(0, 50000, n).astype(np.int64), ll_searches=rng.integers(0, 30, n).astype(np.int32),
              schedule_digest=rng.integers(0, 2 ** 63, n, dtype=np.uint64) * np.uint64(2) + np.uint64(1),
              path_len=rng.integers(0, cap + 3, (n, na)).astype(np.int32))
    pxy = rng.integers(0, 32, (n, na, cap, 2)).astype(np.int32)
    return ra, pxy


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_whole_batch(tmp_path):
    ra, pxy = _results(5000, 10, 128)
    bench.dump_outputs(str(tmp_path / "a"), ra, pxy, 0)
    bench.dump_outputs(str(tmp_path / "b"), ra, pxy, 0)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == sorted(b) and "instance_index" not in a
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), k
        assert np.array_equal(a[k], b[k]), k  # the same sample every time
    for k in ("status", "cost", "makespan", "hl_expanded", "ll_expanded", "ll_searches"):
        assert np.array_equal(a[k], ra[k])
    assert np.array_equal(a["path_len"], ra["path_len"])
    digest = (a["schedule_digest_hi"].astype(np.uint64) << np.uint64(32)) | a["schedule_digest_lo"].astype(np.uint64)
    assert np.array_equal(digest, ra["schedule_digest"])
    pick = a["paths_sample_index"].astype(np.int64)
    assert len(pick) == bench.DUMP_PATHS_SAMPLE and np.all(np.diff(pick) > 0)
    for j, i in enumerate(pick[:64]):
        for ag in range(10):
            got = a["paths_sample"][j, ag]
            if ra["status"][i] != 0:
                assert np.all(got == -1)
                continue
            m = min(ra["path_len"][i, ag], 128)
            assert np.array_equal(got[:m], pxy[i, ag, :m]) and np.all(got[m:] == -1)


def test_dump_stays_within_budget(tmp_path):
    n = 1 << 20
    ra, _ = _results(n, 4, 8)
    pxy = np.zeros((n, 4, 8, 2), dtype=np.int32)
    bench.dump_outputs(str(tmp_path), ra, pxy, 0)
    total = sum(os.path.getsize(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path))
    assert total <= bench.DUMP_BUDGET_BYTES
    a = _load(tmp_path)
    rows = a["instance_index"].astype(np.int64)
    assert 0 < len(rows) < n and np.all(np.diff(rows) > 0)
    assert np.array_equal(a["ll_expanded"], ra["ll_expanded"][rows])
    assert a["path_len"].shape == (len(rows), 4)
