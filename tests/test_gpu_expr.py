"""k_expr_eval on the GPU through the operators that use it: terminal
Projection and Filter plans, the divide-by-zero error path, and computed Agg
inputs. Expected columns come from the numpy reference in expr_ref; every row
of every output is compared with assert_array_equal."""
import functools

import numpy as np
import pytest

import blaze_amd
import expr_ref as R
from blaze_amd import plan
from oracle import pywrap as oracle

pytestmark = pytest.mark.gpu

I32, I64, F64 = "int32", "int64", "float64"
I32_MIN, I32_MAX = -2**31, 2**31 - 1
I64_MIN, I64_MAX = -2**63, 2**63 - 1

FIELDS = [("a32", plan.DT_INT32), ("b32", plan.DT_INT32),
          ("a64", plan.DT_INT64), ("b64", plan.DT_INT64),
          ("af", plan.DT_FLOAT64), ("bf", plan.DT_FLOAT64),
          ("cf", plan.DT_FLOAT64)]
A32, B32, A64, B64, AF, BF, CF = (R.col(i, FIELDS[i][0]) for i in range(7))

# the validity-word tail and wave boundaries; 4099 spans several blocks
ROW_COUNTS = [1, 63, 64, 65, 130, 4099]


def _reader(fields=FIELDS):
    return plan.ffi_reader([plan.field(n, dt, True) for n, dt in fields],
                           "input0")


@functools.lru_cache(maxsize=None)
def _data(n, nulls):
    """Input columns (read-only, shared): wrap and cast edges planted where
    there is room, ~10% nulls per column or no validity buffers at all. No
    NaN and no -0.0 (the documented comparison caveat)."""
    rng = np.random.default_rng(1000 + n)
    a32 = rng.integers(I32_MIN, I32_MAX, n, dtype=np.int64).astype(np.int32)
    b32 = rng.integers(-40000, 40000, n).astype(np.int32)
    a64 = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64)
    b64 = rng.integers(-2**33, 2**33, n).astype(np.int64)
    af = rng.random(n) * 7 - 3          # fractional: a*b + c rounds twice
    bf = rng.random(n) * 5 - 2
    cf = rng.random(n) * 11 - 6
    for arr, edges in ((a32, [I32_MAX, I32_MIN, -1, 0]),
                       (b32, [1, -1, I32_MIN, 7]),
                       (a64, [I64_MAX, I64_MIN, 2**31, -2**31 - 1, 2**31 - 1,
                              -2**31]),
                       (b64, [1, -1, I64_MIN, 3, 5, -7]),
                       (af, [1e30, -1e30, 2147483647.5, -2147483648.5, 0.5,
                             9.3e18])):
        k = min(len(edges), n)
        arr[n - k:] = edges[:k]          # at the tail: the partial word
    cols = []
    for v in (a32, b32, a64, b64, af, bf, cf):
        v.setflags(write=False)
        valid = None
        if nulls:
            valid = rng.random(n) >= 0.1
            valid.setflags(write=False)
        cols.append((v, valid))
    return tuple(cols)


def _split(cols, sizes):
    out, lo = [], 0
    for sz in sizes:
        out.append([(v[lo:lo + sz], None if m is None else m[lo:lo + sz])
                    for v, m in cols])
        lo += sz
    return out


def _run(task, batches, ncols):
    """Run a terminal Filter / Projection task; concatenate its output
    batches into per-column (values, valid) with valid always materialised."""
    t = blaze_amd.Task(task, batches=batches)
    try:
        outs = t.run()
    finally:
        t.finalize()
    got = []
    for ci in range(ncols):
        vals = [ob[ci]["values"] for ob in outs]
        valid = [np.ones(len(ob[ci]["values"]), bool)
                 if ob[ci]["valid"] is None else ob[ci]["valid"]
                 for ob in outs]
        got.append((np.concatenate(vals) if vals else np.zeros(0),
                    np.concatenate(valid) if valid else np.zeros(0, bool)))
    return got, outs


ARITH_EXPRS = [
    R.binop("Plus", R.binop("Multiply", AF, BF), CF),      # FMA would differ
    R.binop("Multiply", A32, B32), R.binop("Plus", A32, B32),
    R.binop("Minus", A32, B32),
    R.binop("Multiply", A64, B64), R.binop("Plus", A64, A64),
    R.binop("Minus", A64, B64),
    ("neg", A32), ("neg", A64), ("neg", AF),
    R.binop("Divide", AF, BF), R.binop("Modulo", AF, BF),
    R.binop("Divide", A64, R.lit(7, I64)),
    R.binop("Modulo", A32, R.lit(-10, I32)),
    R.cast(A32, I64), R.cast(A32, F64), R.cast(A64, F64), R.cast(A64, I32),
    R.cast(AF, I64), R.cast(AF, I32), R.cast(A64, I32, try_=True),
    R.case([(R.binop("Gt", A32, R.lit(0, I32)), B64),
            (("is_null", A32), R.lit(-1, I64))], else_=R.lit(None, I64)),
    R.case([(R.binop("Or", R.binop("Lt", AF, BF), ("is_null", CF)), AF)]),
]


def _project_task(exprs):
    return plan.task_definition(plan.projection(
        _reader(), [R.to_plan(e) for e in exprs],
        [f"o{i}" for i in range(len(exprs))]))


def _check_projection(cols, n, sizes):
    got, _ = _run(_project_task(ARITH_EXPRS), _split(cols, sizes),
                  len(ARITH_EXPRS))
    for i, e in enumerate(ARITH_EXPRS):
        ref = R.evaluate(e, cols, n)
        assert not ref.poison.any()
        ref_v, ref_st = ref.canonical()
        gv, gm = got[i]
        assert gv.dtype == ref_v.dtype, (i, gv.dtype, ref_v.dtype)
        np.testing.assert_array_equal(gm, ref_st == 0, err_msg=f"expr {i}")
        # every row, null rows included (the kernel writes 0 there)
        np.testing.assert_array_equal(gv, ref_v, err_msg=f"expr {i}")


@pytest.mark.parametrize("nulls", [True, False], ids=["nulls", "novalidity"])
@pytest.mark.parametrize("n", ROW_COUNTS)
def test_terminal_projection_arithmetic(n, nulls):
    _check_projection(_data(n, nulls), n, [n])


def test_terminal_projection_three_unequal_batches():
    n = 4099
    _check_projection(_data(n, True), n, [65, 4000, 34])


def test_projection_keeps_column_views_and_order():
    n = 130
    cols = _data(n, True)
    exprs = [B64, R.binop("Plus", AF, CF), A32]
    got, outs = _run(_project_task(exprs), _split(cols, [n]), 3)
    for i, e in enumerate(exprs):
        ref_v, ref_st = R.evaluate(e, cols, n).canonical()
        np.testing.assert_array_equal(got[i][1], ref_st == 0)
        np.testing.assert_array_equal(
            np.where(got[i][1], got[i][0], 0), ref_v)
    assert len(outs) == 1


# ---- terminal Filter --------------------------------------------------------

FILTER_FIELDS = [("a", plan.DT_INT64), ("b", plan.DT_INT64),
                 ("c", plan.DT_INT64), ("s", plan.DT_UTF8)]
FA, FB, FC = (R.col(i, FILTER_FIELDS[i][0]) for i in range(3))
VOCAB = [f"row_{i:03d}" for i in range(40)] + ["", "天地人"]


def _utf8_col(strings):
    raw = [s.encode() for s in strings]
    offs = np.zeros(len(raw) + 1, dtype=np.int32)
    offs[1:] = np.cumsum([len(r) for r in raw])
    return np.frombuffer(b"".join(raw), dtype=np.uint8).copy(), offs


@functools.lru_cache(maxsize=None)
def _filter_data(n):
    rng = np.random.default_rng(2000 + n)
    cols = []
    for _ in range(3):
        v = rng.integers(-3, 4, n).astype(np.int64)   # many equal pairs
        m = rng.random(n) >= 0.1
        cols.append((v, m))
    strs = [VOCAB[i] for i in rng.integers(0, len(VOCAB), n)]
    return tuple(cols), strs


FILTER_PREDS = {
    "or_is_null": [R.binop("Or", R.binop("Gt", FA, FB), ("is_null", FC))],
    "not_eq": [("not", R.binop("Eq", FA, FB))],
    "null_predicate_drops": [R.binop("Gt", FA, FB)],   # null where a or b is
    "two_predicates": [R.binop("LtEq", FA, FC), ("not", ("is_null", FB))],
}


def _check_filter(name, n, sizes):
    cols, strs = _filter_data(n)
    preds = FILTER_PREDS[name]
    task = plan.task_definition(plan.filter_node(
        _reader(FILTER_FIELDS), [R.to_plan(p) for p in preds]))
    batches, lo = [], 0
    for sz in sizes:
        data, offs = _utf8_col(strs[lo:lo + sz])
        batches.append([(v[lo:lo + sz], m[lo:lo + sz]) for v, m in cols] +
                       [("binary", data, offs, None)])
        lo += sz
    t = blaze_amd.Task(task, batches=batches)
    try:
        outs = t.run()
    finally:
        t.finalize()
    both = preds[0]
    for p in preds[1:]:
        both = R.binop("And", both, p)
    ref = R.evaluate(both, list(cols), n)
    assert not ref.poison.any()
    keep = ref.valid & ref.values          # null predicate rows are dropped
    if name == "null_predicate_drops" and n >= 63:
        assert (~ref.valid).any()
    for ci in range(3):
        v, m = cols[ci]
        gv = np.concatenate([ob[ci]["values"] for ob in outs]) \
            if outs else np.zeros(0, np.int64)
        gm = np.concatenate(
            [np.ones(len(ob[ci]["values"]), bool) if ob[ci]["valid"] is None
             else ob[ci]["valid"] for ob in outs]) if outs \
            else np.zeros(0, bool)
        np.testing.assert_array_equal(gm, m[keep])
        np.testing.assert_array_equal(gv[gm], v[keep][m[keep]])
    got_strs = []
    for ob in outs:
        d, o = ob[3]["data"].tobytes(), ob[3]["offsets"]
        got_strs += [d[o[i]:o[i + 1]].decode() for i in range(len(o) - 1)]
    assert got_strs == [s for s, k in zip(strs, keep) if k]


@pytest.mark.parametrize("name", list(FILTER_PREDS))
@pytest.mark.parametrize("n", ROW_COUNTS)
def test_terminal_filter(name, n):
    _check_filter(name, n, [n])


def test_terminal_filter_three_unequal_batches():
    _check_filter("or_is_null", 4099, [130, 3906, 63])


# ---- divide by zero: an error return, dropped only where the table says -----

def _div_data(n=130):
    rng = np.random.default_rng(77)
    a = rng.integers(-1000, 1000, n).astype(np.int64)
    b = rng.integers(1, 9, n).astype(np.int64)
    b[[0, 63, 64, 129]] = 0              # zeros at chosen rows
    cols = [(np.zeros(n, np.int32), None)] * 2 + [(a, None), (b, None)] + \
        [(np.zeros(n), None)] * 3
    return cols, n


DIV = R.binop("Divide", A64, B64)
NONZERO = R.binop("NotEq", B64, R.lit(0, I64))


def test_divide_by_zero_fails_the_task():
    cols, n = _div_data()
    with pytest.raises(RuntimeError, match="Divide by zero"):
        _run(_project_task([DIV]), _split(cols, [n]), 1)


def test_case_guard_drops_the_poison():
    cols, n = _div_data()
    e = R.case([(NONZERO, DIV)], else_=R.lit(0, I64))
    got, _ = _run(_project_task([e]), _split(cols, [n]), 1)
    ref_v, ref_st = R.evaluate(e, cols, n).canonical()
    assert not ref_st.any()
    np.testing.assert_array_equal(got[0][1], ref_st == 0)
    np.testing.assert_array_equal(got[0][0], ref_v)


def _div_filter(pred):
    cols, n = _div_data()
    task = plan.task_definition(plan.filter_node(_reader(),
                                                 [R.to_plan(pred)]))
    got, _ = _run(task, _split(cols, [n]), len(FIELDS))
    return got, cols, n


def test_sc_and_drops_the_poison_plain_and_does_not():
    big = R.binop("Gt", DIV, R.lit(1, I64))
    pred = ("sc_and", NONZERO, big)
    got, cols, n = _div_filter(pred)
    ref = R.evaluate(pred, cols, n)
    assert not ref.poison.any()
    keep = ref.valid & ref.values
    assert keep.any() and not keep.all()
    np.testing.assert_array_equal(got[2][0], cols[2][0][keep])
    np.testing.assert_array_equal(got[3][0], cols[3][0][keep])
    with pytest.raises(RuntimeError, match="Divide by zero"):
        _div_filter(R.binop("And", NONZERO, big))


# ---- computed Agg inputs ----------------------------------------------------

def test_agg_over_computed_grouping_and_arguments():
    """SUM(price*qty), COUNT(CASE WHEN x > 0 THEN 1 END) GROUP BY k % 10 as a
    Partial -> Final chain; integer-valued data, so sums are bit-exact."""
    rng = np.random.default_rng(5)
    n = 4099
    k = rng.integers(-500, 500, n).astype(np.int64)    # negative remainders
    price = rng.integers(1, 1000, n).astype(np.float64)
    qty = rng.integers(1, 50, n).astype(np.float64)
    x = rng.integers(-5, 6, n).astype(np.int32)
    pv, xv = rng.random(n) >= 0.1, rng.random(n) >= 0.1
    fields = [("k", plan.DT_INT64), ("price", plan.DT_FLOAT64),
              ("qty", plan.DT_FLOAT64), ("x", plan.DT_INT32)]
    K, P, Q, X = (R.col(i, fields[i][0]) for i in range(4))
    group = R.binop("Modulo", K, R.lit(10, I64))
    revenue = R.binop("Multiply", P, Q)
    flag = R.case([(R.binop("Gt", X, R.lit(0, I32)), R.lit(1, I32))])
    aggs = [plan.agg_expr(plan.AGG_SUM, [R.to_plan(revenue)],
                          plan.DT_FLOAT64),
            plan.agg_expr(plan.AGG_COUNT, [R.to_plan(flag)], plan.DT_INT64)]
    partial = plan.agg(_reader(fields), [R.to_plan(group)], aggs,
                       [plan.MODE_PARTIAL] * 2, ["g"], ["rev", "pos"])
    final = plan.agg(partial, [plan.column("g", 0)], aggs,
                     [plan.MODE_FINAL] * 2, ["g"], ["rev", "pos"])
    cols = [(k, None), (price, pv), (qty, None), (x, xv)]
    t = blaze_amd.Task(plan.task_definition(final),
                       batches=_split(cols, [1000, 3000, 99]))
    outs = t.run()
    t.finalize()
    got_keys = np.concatenate([ob[0]["values"] for ob in outs])
    got_sums = np.concatenate([ob[1]["values"] for ob in outs])
    got_cnts = np.concatenate([ob[2]["values"] for ob in outs])

    g = R.evaluate(group, cols, n)
    rev = R.evaluate(revenue, cols, n)
    pos = R.evaluate(flag, cols, n)
    assert g.valid.all() and (g.values < 0).any()
    o_sum, o_cnt = oracle.Agg(), oracle.Agg()
    o_sum.update(g.values, rev.values, val_valid=rev.valid)
    o_cnt.update(g.values, pos.values.astype(np.float64), val_valid=pos.valid)
    rs, rc = o_sum.output(), o_cnt.output()
    np.testing.assert_array_equal(got_keys, rs["keys"])
    np.testing.assert_array_equal(got_keys, rc["keys"])
    np.testing.assert_array_equal(got_sums, rs["sums"])
    np.testing.assert_array_equal(got_cnts, rc["counts"])
    assert len(got_keys) == 19
