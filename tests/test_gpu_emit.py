"""Host emit of the aggregation output: a Partial -> Final chain whose columns
come back through the engine's export buffers. Pins the compaction of the
slot table at its tile edges, bitmaps that do not end on a byte, the exported
Arrow null_count, results under buffer reuse across tasks, the emit byte
metrics and the group counter under growth. The engine grows a table to 2^21
slots before its first chunk, so in the plain cases the compaction sees the
two special slots alone in the tail tile of a grown table; the cases with a
capped memory budget keep the table at 64 / 1024 slots, smaller than one
tile, with the special slots inside it. The reference is the oracle
throughout."""
import numpy as np
import pytest

import blaze_amd
from blaze_amd import plan
from oracle import pywrap as oracle

pytestmark = pytest.mark.gpu

I64_MIN = -2**63


def _gen(groups, seed, specials=True, rows_per_group=4):
    """~rows_per_group rows per group in shuffled order. Every fifth regular
    group has only null values (SUM null, COUNT 0). With specials, an
    i64::MIN-key group and a null-key group are added; the null-key group's
    values are all null too."""
    rng = np.random.default_rng(seed)
    ids = rng.permutation(groups * 7 + 11)[:groups].astype(np.int64) - 5
    keys = np.repeat(ids, rows_per_group)
    kv = np.ones(len(keys), bool)
    vv = np.ones(len(keys), bool)
    vv[np.repeat(np.arange(groups) % 5 == 4, rows_per_group)] = False
    if specials:
        keys = np.concatenate([keys, np.full(3, I64_MIN), np.zeros(3, np.int64)])
        kv = np.concatenate([kv, np.ones(3, bool), np.zeros(3, bool)])
        vv = np.concatenate([vv, np.ones(3, bool), np.zeros(3, bool)])
    order = rng.permutation(len(keys))
    keys, kv, vv = keys[order], kv[order], vv[order]
    vals = rng.integers(0, 1000, len(keys)).astype(np.float64)
    return keys, kv, vals, vv


@pytest.fixture
def exported(monkeypatch):
    """The null_count of every exported child array, one list per batch, as
    the engine wrote it into the ArrowArray (the importer only looks at
    whether it is zero)."""
    seen = []
    orig = blaze_amd._import_output

    def spy(array_ptr, schema_fields):
        a = array_ptr.contents
        seen.append([int(a.children[i].contents.null_count)
                     for i in range(a.n_children)])
        return orig(array_ptr, schema_fields)

    monkeypatch.setattr(blaze_amd, "_import_output", spy)
    return seen


def _cat(outs, col):
    vals = np.concatenate([o[col]["values"] for o in outs])
    if all(o[col]["valid"] is None for o in outs):
        return vals, None
    valid = np.concatenate([
        o[col]["valid"] if o[col]["valid"] is not None
        else np.ones(len(o[col]["values"]), bool) for o in outs])
    return vals, valid


def _check_col(got_vals, got_valid, ref_vals, ref_valid):
    """A column without nulls comes back without a bitmap; one with nulls
    carries exactly the reference's validity."""
    if ref_valid.all():
        assert got_valid is None
        np.testing.assert_array_equal(got_vals, ref_vals)
    else:
        assert got_valid is not None
        np.testing.assert_array_equal(got_valid, ref_valid)
        np.testing.assert_array_equal(got_vals[got_valid], ref_vals[ref_valid])


def _check_outs(outs, ref, null_counts):
    """null_counts: the exported per-batch, per-column Arrow null_count of
    exactly these batches."""
    gk, gkv = _cat(outs, 0)
    gs, gsv = _cat(outs, 1)
    gc, gcv = _cat(outs, 2)
    assert len(gk) == len(ref["keys"])
    _check_col(gk, gkv, ref["keys"], ref["key_valid"])       # order included
    _check_col(gs, gsv, ref["sums"], ref["sum_valid"])
    assert gcv is None
    np.testing.assert_array_equal(gc, ref["counts"])
    # per batch: the exported null_count is the reference's number of nulls
    # in that batch's rows, and a bitmap is attached exactly when it is > 0
    assert len(null_counts) == len(outs)
    at = 0
    for o, nc in zip(outs, null_counts):
        n = len(o[0]["values"])
        for col, name in ((0, "key_valid"), (1, "sum_valid")):
            want = int((~ref[name][at:at + n]).sum())
            assert nc[col] == want
            assert (o[col]["valid"] is not None) == (want > 0)
        assert nc[2] == 0
        at += n


def _ref(keys, kv, vals, vv):
    orc = oracle.Agg()
    orc.update(keys, vals, key_valid=kv, val_valid=vv)
    return orc.output()


def _run_chain(keys, kv, vals, vv, conf):
    t = blaze_amd.Task(plan.plan_partial_final(),
                       batches=[[(keys, kv), (vals, vv)]], conf=conf)
    outs = t.run()
    t.finalize()
    return outs


@pytest.mark.parametrize("slots", [64, 4096])
@pytest.mark.parametrize("specials", [True, False])
@pytest.mark.parametrize("groups", [1, 7, 8, 9, 255, 256, 257, 2049])
def test_emit_group_counts(groups, specials, slots, exported):
    """With specials the two special groups ride on top of `groups` regular
    ones; without, the output is exactly `groups` rows, so the bitmaps end
    one short of, on and one past a byte."""
    keys, kv, vals, vv = _gen(groups, 1000 + groups, specials)
    outs = _run_chain(keys, kv, vals, vv,
                      {"AURON_HIP_AGG_TABLE_SLOTS": slots})
    ref = _ref(keys, kv, vals, vv)
    assert len(ref["keys"]) == groups + (2 if specials else 0)
    _check_outs(outs, ref, exported)


def test_emit_multi_batch_unaligned_bitmaps(exported):
    """257 groups at BATCH_SIZE=100: batches of 100/100/57, none of whose
    bitmaps ends on a byte."""
    keys, kv, vals, vv = _gen(255, 77, specials=True)
    outs = _run_chain(keys, kv, vals, vv, {"BATCH_SIZE": 100})
    assert [len(o[0]["values"]) for o in outs] == [100, 100, 57]
    ref = _ref(keys, kv, vals, vv)
    # key and SUM carry different null counts, in every batch that has any
    assert int((~ref["key_valid"]).sum()) == 1
    assert int((~ref["sum_valid"][:100]).sum()) > 1
    _check_outs(outs, ref, exported)


def test_emit_no_nulls_has_no_bitmaps(exported):
    rng = np.random.default_rng(5)
    keys = rng.integers(0, 300, 2000).astype(np.int64)
    vals = rng.integers(0, 1000, 2000).astype(np.float64)
    outs = _run_chain(keys, None, vals, None, {})
    for o in outs:
        assert o[0]["valid"] is None and o[1]["valid"] is None
        assert o[2]["valid"] is None
    ref = _ref(keys, None, vals, None)
    assert all(nc == [0, 0, 0] for nc in exported)
    _check_outs(outs, ref, exported)


def test_emit_buffers_reused_across_tasks(exported):
    """Three chains in one process. The importer copies every column and
    releases the export at once, so the later tasks get their buffers back
    from the pool with the earlier tasks' bytes in them: every result must
    still be right (a stale bitmap or tail would show), and the arrays kept
    from earlier runs, copies owned by Python, are unchanged at the end."""
    kept, snaps, refs, ncs = [], [], [], []
    for r in range(3):
        keys, kv, vals, vv = _gen(257, 300 + r, specials=True)
        outs = _run_chain(keys, kv, vals, vv, {"BATCH_SIZE": 100})
        kept.append(outs)
        snaps.append([[{k: (None if v is None else np.array(v, copy=True))
                        for k, v in c.items() if k in ("values", "valid")}
                       for c in o] for o in outs])
        refs.append(_ref(keys, kv, vals, vv))
        ncs.append(exported[-len(outs):])
    for outs, snap, ref, nc in zip(kept, snaps, refs, ncs):
        for o, so in zip(outs, snap):
            for c, sc in zip(o, so):
                np.testing.assert_array_equal(c["values"], sc["values"])
                assert (c["valid"] is None) == (sc["valid"] is None)
                if c["valid"] is not None:
                    np.testing.assert_array_equal(c["valid"], sc["valid"])
        _check_outs(outs, ref, nc)


def _frozen_batch(keys, kv, vals, vv):
    """One Partial task's output as the oracle writes it: (key, a8 buffer)."""
    orc = oracle.Agg()
    orc.update(keys, vals, key_valid=kv, val_valid=vv)
    g = orc.output()
    data, offs = orc.freeze()
    return g["keys"], g["key_valid"], data, offs


def test_emit_metrics_final_plan(exported):
    """(key, SUM, COUNT) final plan: every payload byte arrives by D2H in its
    export buffer (three 8-byte columns plus the key and SUM bitmaps per
    batch) and none is moved again on the host."""
    keys, kv, vals, vv = _gen(255, 91, specials=True)
    pk, pkv, data, offs = _frozen_batch(keys, kv, vals, vv)
    t = blaze_amd.Task(
        plan.plan_final_only(),
        batches=[[(pk, pkv), ("binary", data, offs.astype(np.int32), None)]],
        conf={"BATCH_SIZE": 100})
    outs = t.run()
    lens = [len(o[0]["values"]) for o in outs]
    assert lens == [100, 100, 57]
    want = sum(3 * 8 * n + 2 * ((n + 7) // 8) for n in lens)
    assert t.metric("emit_host_copy_bytes") == 0
    assert t.metric("emit_d2h_bytes") == want
    t.finalize()
    fin = oracle.Agg()
    fin.merge_frozen(pk, data, offs, key_valid=pkv)
    _check_outs(outs, fin.output(), exported)


def test_final_merge_group_counter_under_growth(exported):
    """Every key arrives twice, once per input batch; 50 000 groups into a
    table that starts at 1024 slots, so it grows and re-reads its group
    counter mid-stream. The counter and the results must match the oracle."""
    groups = 50_000
    batches, fin = [], oracle.Agg()
    for seed in (11, 12):
        rng = np.random.default_rng(seed)
        keys = rng.permutation(groups).astype(np.int64) * 3 - 7
        keys = np.concatenate([keys, [I64_MIN, 0]])
        kv = np.ones(len(keys), bool)
        kv[-1] = False
        vals = rng.integers(0, 1000, len(keys)).astype(np.float64)
        vv = rng.random(len(keys)) >= 0.1
        pk, pkv, data, offs = _frozen_batch(keys, kv, vals, vv)
        batches.append([(pk, pkv),
                        ("binary", data, offs.astype(np.int32), None)])
        fin.merge_frozen(pk, data, offs, key_valid=pkv)
    t = blaze_amd.Task(plan.plan_final_only(), batches=batches,
                       conf={"AURON_HIP_AGG_TABLE_SLOTS": 1024})
    outs = t.run()
    assert fin.num_groups == groups + 2
    assert t.metric("num_groups") == fin.num_groups
    t.finalize()
    _check_outs(outs, fin.output(), exported)


@pytest.mark.parametrize("budget,groups", [(4096, 257), (64 << 10, 2049)])
def test_emit_table_smaller_than_a_compaction_tile(budget, groups, exported):
    """AURON_HIP_MEM_BUDGET caps the table at budget / 64 slots (64 and
    1024), so it cannot grow: it spills instead, and every compaction runs on
    a table smaller than one tile whose special slots sit inside that tile.
    Output order is per spill bucket then, so rows are compared as a set;
    the exported null_count must equal the unset bits of each batch."""
    keys, kv, vals, vv = _gen(groups, 500 + groups, specials=True)
    t = blaze_amd.Task(plan.plan_partial_final(),
                       batches=[[(keys, kv), (vals, vv)]],
                       conf={"AURON_HIP_MEM_BUDGET": budget,
                             "AURON_HIP_AGG_TABLE_SLOTS": budget // 64})
    outs = t.run()
    assert t.metric("spill_count") > 0
    t.finalize()
    ref = _ref(keys, kv, vals, vv)

    def rows(k, kvalid, s, svalid, c):
        return sorted(zip(kvalid.tolist(), np.where(kvalid, k, 0).tolist(),
                          c.tolist(), svalid.tolist(),
                          np.where(svalid, s, 0.0).tolist()))

    gk, gkv = _cat(outs, 0)
    gs, gsv = _cat(outs, 1)
    gc, gcv = _cat(outs, 2)
    assert gcv is None and len(gk) == groups + 2
    ones = np.ones(len(gk), bool)
    assert rows(gk, ones if gkv is None else gkv, gs,
                ones if gsv is None else gsv, gc) == \
        rows(ref["keys"], ref["key_valid"], ref["sums"], ref["sum_valid"],
             ref["counts"])
    assert len(exported) == len(outs)
    for o, nc in zip(outs, exported):
        for col in (0, 1):
            v = o[col]["valid"]
            assert nc[col] == (0 if v is None else int((~v).sum()))
            assert v is None or nc[col] > 0
        assert nc[2] == 0


# ---- terminal Filter: the Runtime's own host emit ---------------------------

def _utf8(strings):
    raw = [s.encode() for s in strings]
    offs = np.zeros(len(raw) + 1, dtype=np.int32)
    offs[1:] = np.cumsum([len(r) for r in raw])
    return np.frombuffer(b"".join(raw), dtype=np.uint8).copy(), offs


def _filter_task():
    """Filter(b IS NOT NULL) as the plan's last stage over (a Int64, b Int32,
    s Utf8), all nullable."""
    reader = plan.ffi_reader([plan.field("a", plan.DT_INT64, True),
                              plan.field("b", plan.DT_INT32, True),
                              plan.field("s", plan.DT_UTF8, True)], "input0")
    return plan.task_definition(
        plan.filter_node(reader, [plan.is_not_null(plan.column("b", 1))]))


def _filter_input(m, splits):
    """Input batches of the given sizes in which exactly m rows pass. b is
    null on the dropped rows only, so its gathered bitmap has no zero bit; a
    and s carry nulls among the passing rows (s: empty strings too). With
    m == 1 the one passing row has a null a and a valid s."""
    n = sum(splits)
    rng = np.random.default_rng(4000 + m)
    sel = np.zeros(n, bool)
    sel[rng.permutation(n)[:m]] = True
    a = rng.integers(-1000, 1000, n).astype(np.int64)
    av = rng.random(n) >= 0.3
    b = rng.integers(-1000, 1000, n).astype(np.int32)
    vocab = ["", "x", "天地人", "row_0123456789"]
    strs = [vocab[i] for i in rng.integers(0, len(vocab), n)]
    sv = rng.random(n) >= 0.3
    if m == 1:
        av[sel], sv[sel] = False, True
    batches, parts, at = [], [], 0
    for k in splits:
        r = slice(at, at + k)
        data, offs = _utf8(strs[r])
        batches.append([(a[r], av[r]), (b[r], sel[r]),
                        ("binary", data, offs, sv[r])])
        parts.append(dict(sel=sel[r], a=a[r], av=av[r], b=b[r],
                          strs=strs[at:at + k], sv=sv[r]))
        at += k
    return batches, [p for p in parts if p["sel"].any()]


FILTER_CASES = [(1, [3]), (9, [20]), (1001, [130, 1500, 63])]


def _run_filter(m, splits):
    batches, parts = _filter_input(m, splits)
    assert sum(int(p["sel"].sum()) for p in parts) == m
    # every input batch has a dropped row, so b always arrives with a bitmap
    assert all(not p["sel"].all() for p in parts)
    t = blaze_amd.Task(_filter_task(), batches=batches)
    outs = t.run()
    metrics = (t.metric("emit_d2h_bytes"), t.metric("emit_host_copy_bytes"))
    t.finalize()
    return outs, parts, metrics


@pytest.mark.parametrize("m,splits", FILTER_CASES)
def test_terminal_filter_null_counts_and_bitmaps(m, splits, exported):
    """One output batch per input batch with a passing row; bitmaps of 1, 9
    and (over three unequal batches) 1 001 rows in all end mid-byte. Per
    batch: values, offsets and validity exact, the exported null_count of
    each child is the number of nulls among the selected rows, and a column
    whose selected rows have no nulls comes back without a bitmap."""
    outs, parts, _ = _run_filter(m, splits)
    assert len(outs) == len(parts) == len(exported)
    for o, p, nc in zip(outs, parts, exported):
        sel = p["sel"]
        k = int(sel.sum())
        want_valid = [p["av"][sel], np.ones(k, bool), p["sv"][sel]]
        for col in range(3):
            nulls = int((~want_valid[col]).sum())
            assert nc[col] == nulls
            if nulls == 0:
                assert o[col]["valid"] is None
            else:
                np.testing.assert_array_equal(o[col]["valid"],
                                              want_valid[col])
        assert o[1]["valid"] is None        # b: bitmap without a zero bit
        np.testing.assert_array_equal(o[0]["values"], p["a"][sel])
        assert o[1]["values"].dtype == np.int32
        np.testing.assert_array_equal(o[1]["values"], p["b"][sel])
        data, offs = _utf8([p["strs"][i] for i in np.flatnonzero(sel)])
        np.testing.assert_array_equal(o[2]["offsets"], offs)
        np.testing.assert_array_equal(o[2]["data"], data)
    if m == 1:
        assert exported[0] == [1, 0, 0]


@pytest.mark.parametrize("m,splits", FILTER_CASES)
def test_terminal_filter_byte_metric(m, splits):
    """Payload only: values, (k+1)*4 offsets and the data bytes of the Utf8
    column, and (k+7)//8 for every column that arrived with a bitmap. The
    gather carries an input bitmap along and the download happens before the
    null count is known, so b's all-ones bitmap counts. The input side drops
    the bitmap of a column without nulls in that batch."""
    outs, parts, (d2h, host_copy) = _run_filter(m, splits)
    want = 0
    for p in parts:
        sel = p["sel"]
        k = int(sel.sum())
        data, _ = _utf8([p["strs"][i] for i in np.flatnonzero(sel)])
        want += k * 8 + k * 4 + (k + 1) * 4 + len(data)
        carried = [not p["av"].all(), True, not p["sv"].all()]
        want += sum(carried) * ((k + 7) // 8)
    assert host_copy == 0
    assert d2h == want
