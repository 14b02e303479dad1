"""bench.py --dump-outputs: the sample of the k-mer list is chosen by key alone (same arrays whatever the task split and order),
holds exact keys and counts, and stays within its size bound.  CPU only: a stand-in for the device-resident result."""
import ctypes as C
import os
import sys

import numpy as np

from tests import util

sys.path.insert(0, util.ROOT)
import bench  # noqa: E402
from hysortk_amd import _lib  # noqa: E402


class _FakeDeviceResult:
    """What dump_outputs reads of a DeviceResult: nw, ntasks, n, res (histogram, total_kmers) and fetch(t)."""

    def __init__(self, tasks, nw, histo):
        self.tasks, self.nw, self.ntasks = tasks, nw, len(tasks)
        self.n = sum(len(c) for _, c in tasks)
        self._histo = (C.c_uint64 * len(histo))(*histo)
        self.res = _lib.Result()
        self.res.histo, self.res.histo_len = C.cast(self._histo, C.POINTER(C.c_uint64)), len(histo)
        self.res.total_kmers = 987654321

    def fetch(self, t):
        k, c = self.tasks[t]
        return dict(n=len(c), kmers=k, cnt=c)


def _tasks(nw, ntasks, per_task, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(ntasks):
        k = rng.integers(0, 1 << 62, size=(per_task, nw), dtype=np.uint64)
        k = k[np.lexsort(tuple(k[:, w] for w in range(nw - 1, -1, -1)))]
        out.append((k, rng.integers(15, 41, size=per_task).astype(np.uint64)))
    return out


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_sample_is_exact_and_independent_of_task_layout(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_SAMPLE_BYTES", 24 << 10)
    for nw in (1, 2):
        tasks = _tasks(nw, 5, 20000, nw)
        histo = list(range(50))
        bench.dump_outputs(str(tmp_path / ("a%d" % nw)), _FakeDeviceResult(tasks, nw, histo))
        # the same entries split into other tasks, in another order
        allk = np.concatenate([k for k, _ in tasks]); allc = np.concatenate([c for _, c in tasks])
        perm = np.random.default_rng(7).permutation(len(allc))
        other = [(allk[perm[i::3]], allc[perm[i::3]]) for i in range(3)]
        bench.dump_outputs(str(tmp_path / ("b%d" % nw)), _FakeDeviceResult(other, nw, histo))
        a, b = _load(str(tmp_path / ("a%d" % nw))), _load(str(tmp_path / ("b%d" % nw)))
        assert sorted(a) == ["counts", "histogram", "kmers", "totals"]
        for name in a:
            assert a[name].dtype == np.float64 and np.array_equal(a[name], b[name]), name
        km, cnt = a["kmers"], a["counts"]
        assert km.shape == (len(cnt), 2 * nw) and 0 < len(cnt) <= (24 << 10) // (8 * (2 * nw + 1)) * 3 // 2
        keys = np.stack([(km[:, 2 * w].astype(np.uint64) << np.uint64(32)) | km[:, 2 * w + 1].astype(np.uint64) for w in range(nw)], axis=1)
        want = {tuple(k): c for k, c in zip(allk.tolist(), allc.tolist())}
        assert all(want[tuple(k)] == c for k, c in zip(keys.tolist(), cnt.tolist()))
        assert [tuple(k) for k in keys.tolist()] == sorted(tuple(k) for k in keys.tolist())
        assert np.array_equal(a["histogram"], np.arange(50, dtype=np.float64))
        assert a["totals"].tolist() == [len(allc), 987654321]


def test_dump_sample_cap(tmp_path, monkeypatch):
    """A threshold that lets every entry through (the count says the list is small) still writes at most 1.5 x the sample size:
    the entries with the smallest hashes."""
    monkeypatch.setattr(bench, "DUMP_SAMPLE_BYTES", 24 * 1000)
    dev = _FakeDeviceResult(_tasks(1, 3, 10000, 3), 1, [0, 1])
    dev.n = 1000
    bench.dump_outputs(str(tmp_path), dev)
    assert np.load(str(tmp_path / "kmers.npy")).shape == (1500, 2) and np.load(str(tmp_path / "counts.npy")).shape == (1500,)
