"""The key range that picks the packed 16-byte partition records is taken
from the first chunk's histogram pass. Each case is one two-phase chunk
(4 194 304 + 5 rows; the path needs 4 * 2^20) at an edge of the decision:
a small range below zero, the exact 2^32 - 1 boundary, one past it, the
extremes of int64, and a first chunk without a single normal key. The
assertion is parity with the oracle; whichever layout the engine picks, keys
outside the packed window must still arrive through the leftover list."""
import os

import numpy as np
import pytest

import blaze_amd
from blaze_amd import plan
from oracle import pywrap as oracle

pytestmark = pytest.mark.gpu

N = 4_194_304 + 5
I64_MIN = -2**63
I64_MAX = 2**63 - 1


def _run_and_check(batches, env=None):
    env = env or {}
    for k, v in env.items():
        os.environ[k] = v
    try:
        t = blaze_amd.Task(
            plan.plan_partial_final(),
            batches=[[(k, kv), (v, None)] for k, kv, v in batches],
            conf={"BATCH_SIZE": 1 << 22,
                  "AURON_HIP_AGG_TABLE_SLOTS": 1 << 20})
        outs = t.run()
        t.finalize()
    finally:
        for k in env:
            os.environ.pop(k, None)
    got_k = np.concatenate([o[0]["values"] for o in outs])
    got_s = np.concatenate([o[1]["values"] for o in outs])
    got_c = np.concatenate([o[2]["values"] for o in outs])
    orc = oracle.Agg()
    for k, kv, v in batches:
        orc.update(k, v, key_valid=kv)
    ref = orc.output()
    assert len(got_k) == orc.num_groups
    np.testing.assert_array_equal(got_k, ref["keys"])   # first-row order
    np.testing.assert_array_equal(got_c, ref["counts"])
    np.testing.assert_array_equal(got_s, ref["sums"])   # integer-valued


def _vals(rng, n):
    return rng.integers(0, 1000, n).astype(np.float64)


def test_keyrange_small_negative_base():
    rng = np.random.default_rng(71)
    keys = rng.integers(-3, 1000, N).astype(np.int64)
    _run_and_check([(keys, None, _vals(rng, N))])


def test_keyrange_exact_packed_boundary():
    """min 0, max 2^32 - 1: the widest range that still packs."""
    rng = np.random.default_rng(72)
    keys = rng.integers(0, 2**32, N).astype(np.int64) % 50_000 * 85_899
    assert keys.max() < 2**32
    keys[1000] = 0
    keys[2000] = 2**32 - 1
    keys[N - 1] = 2**32 - 1
    _run_and_check([(keys, None, _vals(rng, N))])


def test_keyrange_one_past_boundary():
    """min 0, max 2^32: one too wide, the 24-byte records stay."""
    rng = np.random.default_rng(73)
    keys = rng.integers(0, 50_000, N).astype(np.int64)
    keys[1000] = 0
    keys[2000] = 2**32
    keys[N - 1] = 2**32
    _run_and_check([(keys, None, _vals(rng, N))])


def test_keyrange_int64_extremes():
    """i64::MAX and i64::MIN + 1 are normal keys (i64::MIN itself is the
    special group, present too); the order-mapped range spans 2^64 - 2."""
    rng = np.random.default_rng(74)
    keys = rng.integers(-50_000, 50_000, N).astype(np.int64)
    keys[10] = I64_MAX
    keys[20] = I64_MIN + 1
    keys[30] = I64_MIN
    keys[N - 2] = I64_MAX
    keys[N - 1] = I64_MIN + 1
    _run_and_check([(keys, None, _vals(rng, N))])


def test_keyrange_first_chunk_without_normal_keys():
    """Chunk 1 holds only null and i64::MIN keys (an empty range: nothing to
    pack), chunk 2 is ordinary."""
    rng = np.random.default_rng(75)
    n = 4_194_304
    k1 = np.full(n, I64_MIN, dtype=np.int64)
    kv1 = np.ones(n, bool)
    kv1[::3] = False
    k2 = rng.integers(5_000_000_000, 5_000_200_000, n).astype(np.int64)
    keys = np.concatenate([k1, k2])
    kv = np.concatenate([kv1, np.ones(n, bool)])
    _run_and_check([(keys, kv, _vals(rng, 2 * n))],
                   env={"AURON_AGG2_CHUNK_M": "4"})
