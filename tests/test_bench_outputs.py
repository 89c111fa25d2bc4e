"""bench.py --dump-outputs on CPU: the files hold exactly the scores and CIGAR runs of the pairs they name, as float64, within the size cap;
a batch too big for the cap is sampled the same way every time."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from gonomics_amd import _lib  # noqa: E402


def _results(seed, n, mean_runs):
    rng = np.random.default_rng(seed)
    runs = rng.integers(1, 2 * mean_runs, size=n)
    off = np.concatenate([[0], np.cumsum(runs)]).astype(np.int64)
    ops = np.zeros(int(off[-1]), dtype=_lib.CIGAR_DTYPE)
    ops["run_length"] = rng.integers(1, 100000, size=ops.shape[0])
    ops["op"] = rng.integers(0, 4, size=ops.shape[0])
    return rng.integers(-40000000, 200000, size=n).astype(np.int64), ops, off


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def _check(d, scores, ops, off):
    a = _load(d)
    assert sorted(a) == ["cigar_op", "cigar_run_length", "cigar_runs", "pairs", "scores"]
    assert all(v.dtype == np.float64 for v in a.values())
    assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64 * 1000 * 1000
    pick = a["pairs"].astype(np.int64)
    assert np.all(np.diff(pick) > 0) and np.array_equal(a["scores"], scores[pick])
    assert np.array_equal(a["cigar_runs"], off[pick + 1] - off[pick])
    seg = np.concatenate([ops[off[p]:off[p + 1]] for p in pick])
    assert np.array_equal(a["cigar_run_length"], seg["run_length"]) and np.array_equal(a["cigar_op"], seg["op"])
    return pick


def test_dump_holds_every_pair_when_it_fits(tmp_path):
    res = _results(1, 1000, 5)
    info = bench.dump_outputs(str(tmp_path), *res)
    assert np.array_equal(_check(str(tmp_path), *res), np.arange(1000))
    assert info["pairs"] == info["of_pairs"] == 1000 and info["runs"] == res[2][-1]


def test_dump_samples_a_batch_beyond_the_cap_the_same_way(tmp_path):
    res = _results(2, 2048, 30000)  # ~61 M runs: ~1 GB as float64
    picks = []
    for k in range(2):
        d = str(tmp_path / str(k))
        info = bench.dump_outputs(d, *res)
        picks.append(_check(d, *res))
        assert 0 < info["pairs"] < 2048
    assert np.array_equal(picks[0], picks[1])
