"""bench.py command line: --dump-outputs writes the last timed step's final
aggregate, a plain run leaves the CPU baseline leg out (--full brings it
back), and --steps sets the number of timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _batch(keys, sums, sum_valid, cnts):
    return [dict(dtype="int64", values=keys, valid=None),
            dict(dtype="float64", values=sums, valid=sum_valid),
            dict(dtype="int64", values=cnts, valid=None)]


def test_dump_outputs_columns_and_nulls(tmp_path):
    b0 = _batch(np.array([7, 3], np.int64), np.array([1.5, 99.0]),
                np.array([True, False]), np.array([2, 0], np.int64))
    b1 = _batch(np.array([5], np.int64), np.array([4.0]), None,
                np.array([1], np.int64))
    bench.dump_outputs(str(tmp_path), [b0, b1], rank=0, world=1)
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert sorted(got) == ["cnt", "cnt_valid", "key", "key_valid", "sum",
                           "sum_valid"]
    for name in ("key", "sum", "cnt"):
        assert got[name].dtype == np.float64
        assert got[name + "_valid"].dtype == np.float32
    np.testing.assert_array_equal(got["key"], [7, 3, 5])  # engine row order
    np.testing.assert_array_equal(got["sum"], [1.5, 0.0, 4.0])  # null -> 0
    np.testing.assert_array_equal(got["sum_valid"], [1, 0, 1])
    np.testing.assert_array_equal(got["cnt"], [2, 0, 1])
    np.testing.assert_array_equal(got["key_valid"], [1, 1, 1])


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path, monkeypatch):
    n = 1000
    keys = np.arange(n, dtype=np.int64)
    b = _batch(keys, keys * 2.0, None, keys + 1)
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 36 * 100)  # room for 100 rows
    bench.dump_outputs(str(tmp_path / "a"), [b], rank=0, world=1)
    bench.dump_outputs(str(tmp_path / "b"), [b], rank=0, world=1)
    total = 0
    for f in os.listdir(tmp_path / "a"):
        a = np.load(tmp_path / "a" / f)
        np.testing.assert_array_equal(a, np.load(tmp_path / "b" / f))
        total += a.nbytes
    assert total <= 36 * 100
    k = np.load(tmp_path / "a" / "key.npy")
    assert len(k) == 100 and (np.diff(k) > 0).all()  # same rows, order kept
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "sum.npy"), k * 2)
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "cnt.npy"), k + 1)


def _run_bench(*extra):
    p = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
         "--rows", "200000", "--warmup", "1", *extra],
        capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_dumps_last_step_and_skips_cpu_leg(tmp_path):
    out = _run_bench("--steps", "2", "--dump-outputs", str(tmp_path / "d"))
    assert out["steps"] == 2 and out["ms_per_step"] > 0
    assert out["unit"] == "rows/s" and out["higher_is_better"] is True
    assert out["dtype"] == "f64"
    assert out["value"] == pytest.approx(
        200000 / (out["ms_per_step"] / 1000), rel=1e-2)
    assert out["cpu_baseline"] is None  # only with --full
    d = tmp_path / "d"
    key, s, cnt = (np.load(d / f"{n}.npy") for n in ("key", "sum", "cnt"))
    ng = out["config"]["num_groups"]
    assert len(key) == len(s) == len(cnt) == ng == len(np.unique(key))
    assert np.load(d / "key_valid.npy").all()
    # every row lands in exactly one group; COUNT(val) leaves the nulls out
    assert 0.99 * 200000 <= cnt.sum() <= 200000
    assert (s[np.load(d / "sum_valid.npy") == 0] == 0).all()
    assert (s <= cnt * 999_999.0).all() and (s >= 0).all()
    # same arguments -> same inputs -> same outputs
    _run_bench("--steps", "1", "--dump-outputs", str(tmp_path / "e"))
    for f in os.listdir(d):
        np.testing.assert_array_equal(np.load(d / f),
                                      np.load(tmp_path / "e" / f))
