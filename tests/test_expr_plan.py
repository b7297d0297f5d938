"""Expression plan layer on the host: builder round trips, type and limit
errors at plan build, and the semantics of every op through the host
interpreter (which shares the kernel's per-row evaluator) against the numpy
reference in expr_ref. No GPU needed."""
import numpy as np
import pytest

import blaze_amd
import expr_ref as R
from blaze_amd import plan

I32, I64, F64 = "int32", "int64", "float64"
I32_MIN, I32_MAX = -2**31, 2**31 - 1
I64_MIN, I64_MAX = -2**63, 2**63 - 1

# input schema shared by the tests: two columns of each value type + a string
FIELDS = [("a32", plan.DT_INT32), ("b32", plan.DT_INT32),
          ("a64", plan.DT_INT64), ("b64", plan.DT_INT64),
          ("af", plan.DT_FLOAT64), ("bf", plan.DT_FLOAT64),
          ("s", plan.DT_UTF8)]
A32, B32, A64, B64, AF, BF = (R.col(i, FIELDS[i][0]) for i in range(6))
S = R.col(6, "s")


def _reader():
    return plan.ffi_reader([plan.field(n, dt, True) for n, dt in FIELDS],
                           "input0")


def project_plan(exprs):
    return plan.task_definition(plan.projection(
        _reader(), [R.to_plan(e) for e in exprs],
        [f"o{i}" for i in range(len(exprs))]))


def filter_plan(preds):
    return plan.task_definition(plan.filter_node(
        _reader(), [R.to_plan(p) for p in preds]))


def compile_text(task):
    return blaze_amd.debug_compile_expr(task)


# ---- round trip -------------------------------------------------------------

def test_new_builders_round_trip_through_decoder():
    exprs = [
        ("is_null", A32), ("not", R.binop("Eq", A32, B32)), ("neg", AF),
        R.cast(A32, I64), R.cast(AF, I32, try_=True),
        R.case([(R.binop("Gt", A64, R.lit(0, I64)), B64)],
               else_=R.lit(0, I64)),
        R.case([(R.lit(1, I32), R.lit(10, I32))], base=A32),
        ("sc_and", R.binop("NotEq", B64, R.lit(0, I64)), R.lit(True, "bool")),
        ("sc_or", ("is_null", AF), R.lit(None, "bool")),
        R.binop("Or", R.binop("Lt", A32, B32), ("is_not_null", S)),
    ]
    s = blaze_amd.debug_decode_plan(project_plan(exprs))
    assert "Project(ncols=10)->FFIReader(nfields=7,rid=input0)" in s
    for want in [
            "IsNull(Column(a32#0))",
            "Not(Eq(Column(a32#0),Column(b32#1)))",
            "Negative(Column(af#4))",
            "Cast(Column(a32#0) AS Int64)",
            "TryCast(Column(af#4) AS Int32)",
            "Case(when=Gt(Column(a64#2),Literal(Int64:0)),then=Column(b64#3),"
            "else=Literal(Int64:0))",
            "Case(base=Column(a32#0),when=Literal(Int32:1),"
            "then=Literal(Int32:10),else=none)",
            "SCAnd(NotEq(Column(b64#3),Literal(Int64:0)),Literal(Bool:1))",
            "SCOr(IsNull(Column(af#4)),Literal(Bool:null))",
            "Or(Lt(Column(a32#0),Column(b32#1)),IsNotNull(Column(s#6)))"]:
        assert want in s, (want, s)
    f = blaze_amd.debug_decode_plan(filter_plan(
        [R.binop("Gt", AF, BF), ("is_null", A64)]))
    assert "Filter(npred=2)->FFIReader" in f
    assert "Filter[Gt(Column(af#4),Column(bf#5)); IsNull(Column(a64#2))]" in f


def test_bool_literal_decodes():
    for v in (True, False):
        txt = compile_text(filter_plan([R.lit(v, "bool")]))
        assert f"LIT(Bool:{int(v)})" in txt, txt
    assert "LIT(Bool:null)" in compile_text(filter_plan([R.lit(None, "bool")]))


def test_compile_renders_postfix_program():
    txt = compile_text(project_plan(
        [A32, R.binop("Plus", R.binop("Multiply", AF, BF), AF)]))
    assert txt.strip() == ("expr1 root=Float64 n=5 poison=0 : "
                           "LOAD(col4:Float64) LOAD(col5:Float64) MUL.Float64 "
                           "LOAD(col4:Float64) ADD.Float64")
    # CASE base WHEN v desugars to Eq; integer Divide can poison
    txt = compile_text(project_plan([R.case(
        [(R.lit(3, I64), R.binop("Divide", A64, B64))], base=A64)]))
    assert "EQ.Int64" in txt and "SELECT" in txt and "poison=1" in txt


# ---- plan-build errors ------------------------------------------------------

def _chain(op, leaf, count, right_nested):
    e = leaf
    for _ in range(count - 1):
        e = R.binop(op, leaf, e) if right_nested else R.binop(op, e, leaf)
    return e


@pytest.mark.parametrize("case,task,needles", [
    ("type_mismatch",
     lambda: project_plan([R.binop("Plus", A32, A64)]),
     ["type mismatch", "Plus", "Int32", "Int64"]),
    ("cmp_mismatch",
     lambda: filter_plan([R.binop("Lt", A64, AF)]),
     ["type mismatch", "Lt", "Int64", "Float64"]),
    ("bad_cast",
     lambda: project_plan([R.cast(A32, "utf8")]),
     ["unsupported cast", "Int32", "Utf8"]),
    ("bool_cast",
     lambda: project_plan([R.cast(R.binop("Lt", A32, B32), I32)]),
     ["unsupported cast", "Bool"]),
    ("utf8_operand",
     lambda: filter_plan([R.binop("Eq", S, S)]),
     ["Utf8", "'s'", "computed expression"]),
    ("stack_depth_9",
     lambda: project_plan([_chain("Plus", A64, 9, right_nested=True)]),
     ["stack depth 9", "limit 8"]),
    ("instructions_65",
     lambda: project_plan([_chain("Plus", A64, 33, right_nested=False)]),
     ["65 instructions", "limit 64"]),
    ("bool_projection_root",
     lambda: project_plan([R.binop("Gt", A32, B32)]),
     ["Bool", "wrap in CASE"]),
    ("non_bool_predicate",
     lambda: filter_plan([R.binop("Plus", A32, B32)]),
     ["predicate", "Int32", "not Bool"]),
    ("unknown_binary_op",
     lambda: project_plan([R.binop("BitwiseXor", A32, B32)]),
     ["BitwiseXor"]),
    ("case_branch_mismatch",
     lambda: project_plan([R.case([(R.binop("Gt", A32, B32), A32)],
                                  else_=A64)]),
     ["CASE", "Int64", "Int32"]),
])
def test_plan_build_errors_name_their_cause(case, task, needles):
    txt = compile_text(task())
    assert txt.startswith("ERROR: "), txt
    for nd in needles:
        assert nd in txt, (nd, txt)


def test_limits_are_inclusive():
    """Depth 8 and 64 instructions still compile (the limits, not below)."""
    ok8 = compile_text(project_plan([_chain("Plus", A64, 8, True)]))
    assert ok8.startswith("expr0 root=Int64 n=15"), ok8
    # 32 loads + 31 adds = 63; a Negative on top makes 64
    ok64 = compile_text(project_plan(
        [("neg", _chain("Plus", A64, 32, False))]))
    assert ok64.startswith("expr0 root=Int64 n=64"), ok64


def test_unknown_expr_field_still_fails_decode():
    # PhysicalExprNode.in_list = 13 stays outside the surface
    bad = plan._len_field(13, b"")
    s = blaze_amd.debug_decode_plan(plan.task_definition(
        plan.filter_node(_reader(), [bad])))
    assert "ERROR" in s and "unsupported PhysicalExprNode field 13" in s


# ---- host semantics vs the numpy reference ----------------------------------

def _cols(n, seed, null_frac=0.15):
    """Seven input columns with nulls and every edge value planted."""
    rng = np.random.default_rng(seed)
    a32 = rng.integers(-50, 50, n).astype(np.int32)
    b32 = rng.integers(-5, 6, n).astype(np.int32)       # zeros included
    a64 = rng.integers(-10**12, 10**12, n).astype(np.int64)
    b64 = rng.integers(-4, 5, n).astype(np.int64)        # zeros included
    af = np.round(rng.normal(0, 100, n), 3)
    bf = np.round(rng.normal(0, 3, n), 1)                # zeros included
    edge32 = [I32_MIN, I32_MAX, -1, 0, 1]
    edge64 = [I64_MIN, I64_MAX, -1, 0, 1, 2**31, 2**31 - 1, -2**31,
              -2**31 - 1]
    edgef = [1e30, -1e30, np.nan, 2147483647.5, -2147483648.5, 0.5, -0.5,
             9.3e18, -9.3e18, 2.0**53 + 2]
    a32[:len(edge32)] = edge32
    b32[:len(edge32)] = [-1, 1, -1, 0, 0]
    a64[:len(edge64)] = edge64
    b64[:len(edge64)] = [-1, 1, I64_MIN, 0, 0, 2, -2, 3, -3]
    af[:len(edgef)] = edgef
    cols = []
    for v in (a32, b32, a64, b64, af, bf):
        valid = rng.random(n) >= null_frac
        valid[:10] = True  # the planted edges stay visible
        cols.append((v, valid))
    cols.append((np.zeros(n, np.int32), None))  # Utf8 slot: never read
    return cols


def _check(expr, cols, n, as_filter=False):
    task = filter_plan([expr]) if as_filter else project_plan([expr])
    got_v, got_st = blaze_amd.debug_eval_expr(task, cols)
    ref = R.evaluate(expr, cols, n)
    ref_v, ref_st = ref.canonical()
    np.testing.assert_array_equal(got_st, ref_st)
    assert got_v.dtype == ref_v.dtype, (got_v.dtype, ref_v.dtype)
    # bit-exact, NaN == NaN
    np.testing.assert_array_equal(got_v.view(np.uint8), ref_v.view(np.uint8))
    return ref


N = 300
ZERO = {I32: R.lit(0, I32), I64: R.lit(0, I64), F64: R.lit(0.0, F64)}
PAIRS = {I32: (A32, B32), I64: (A64, B64), F64: (AF, BF)}


@pytest.mark.parametrize("ty", [I32, I64, F64])
@pytest.mark.parametrize("op", ["Plus", "Minus", "Multiply", "Divide",
                                "Modulo"])
def test_arithmetic_matches_reference(op, ty):
    cols = _cols(N, 11)
    x, y = PAIRS[ty]
    # wrap in CASE so the value comes out as a column; poison shows as state 2
    ref = _check(R.binop(op, x, y), cols, N)
    if op in ("Divide", "Modulo") and ty != F64:
        assert (ref.state == 2).any()   # zero divisors and MIN op -1 planted
    else:
        assert not (ref.state == 2).any()
    # both operands the same column: exercises x op x (e.g. MIN * MIN wrap)
    if op in ("Plus", "Minus", "Multiply"):
        _check(R.binop(op, x, x), cols, N)


def test_integer_wrap_at_the_limits():
    cols = _cols(N, 12)
    one32, one64 = R.lit(1, I32), R.lit(1, I64)
    r = _check(R.binop("Plus", A32, one32), cols, N)
    assert r.values[1] == I32_MIN          # MAX + 1 wraps
    r = _check(R.binop("Minus", A64, one64), cols, N)
    assert r.values[0] == I64_MAX          # MIN - 1 wraps
    r = _check(("neg", A32), cols, N)
    assert r.values[0] == I32_MIN          # -MIN wraps to MIN
    r = _check(("neg", A64), cols, N)
    assert r.values[0] == I64_MIN
    _check(R.binop("Multiply", A64, R.lit(3, I64)), cols, N)
    _check(("neg", AF), cols, N)


def test_min_div_minus_one_and_zero_divisor_poison():
    cols = _cols(N, 13)
    for x, y in ((A32, B32), (A64, B64)):
        for op in ("Divide", "Modulo"):
            r = _check(R.binop(op, x, y), cols, N)
            assert r.state[0] == 2         # MIN op -1
            assert r.state[3] == 2 and r.state[4] == 2   # x op 0
            assert r.state[1] == 0
    # Float64 division by zero is IEEE, never poison
    r = _check(R.binop("Divide", AF, R.lit(0.0, F64)), cols, N)
    assert not (r.state == 2).any()


@pytest.mark.parametrize("ty", [I32, I64, F64])
@pytest.mark.parametrize("op", ["Eq", "NotEq", "Lt", "LtEq", "Gt", "GtEq"])
def test_comparisons_match_reference(op, ty):
    cols = _cols(N, 14)
    if ty == F64:  # the documented NaN / -0.0 rule is k_cmp_lit's; keep clear
        cols[4] = (np.nan_to_num(cols[4][0], nan=7.0), cols[4][1])
    x, y = PAIRS[ty]
    _check(R.binop(op, x, y), cols, N, as_filter=True)
    _check(R.binop(op, x, ZERO[ty]), cols, N, as_filter=True)


def _tri(n_rep=1):
    """Two Bool-valued operand columns covering {T, F, null} squared, built
    from Int32 inputs: x = (a32 > 0), null where a32 is null."""
    vals = [1, 0, 1]          # T, F, (null)
    ok = [True, True, False]
    a = np.array([vals[i] for i in range(3) for _ in range(3)] * n_rep,
                 np.int32)
    av = np.array([ok[i] for i in range(3) for _ in range(3)] * n_rep)
    b = np.array([vals[j] for _ in range(3) for j in range(3)] * n_rep,
                 np.int32)
    bv = np.array([ok[j] for _ in range(3) for j in range(3)] * n_rep)
    cols = [(a, av), (b, bv)] + [(np.zeros(len(a), np.int64), None)] * 2 + \
        [(np.zeros(len(a)), None)] * 2 + [(np.zeros(len(a), np.int32), None)]
    x = R.binop("Gt", A32, R.lit(0, I32))
    y = R.binop("Gt", B32, R.lit(0, I32))
    return cols, x, y, len(a)


def test_kleene_tables():
    cols, x, y, n = _tri()
    T, F, NULL = (True, 0), (False, 0), (False, 1)   # (value, state)
    want = {
        "And": [T, F, NULL, F, F, F, NULL, F, NULL],
        "Or": [T, T, T, T, F, NULL, T, NULL, NULL],
    }
    for name, node in (("And", R.binop("And", x, y)),
                       ("Or", R.binop("Or", x, y)),
                       ("And", ("sc_and", x, y)), ("Or", ("sc_or", x, y))):
        got_v, got_st = blaze_amd.debug_eval_expr(filter_plan([node]), cols)
        assert [(bool(v), int(s)) for v, s in zip(got_v, got_st)] == \
            want[name], name
        _check(node, cols, n, as_filter=True)
    # Not: null stays null; IsNull / IsNotNull never null
    got_v, got_st = blaze_amd.debug_eval_expr(filter_plan([("not", x)]), cols)
    assert list(got_st[[0, 3, 6]]) == [0, 0, 1]
    assert list(got_v[[0, 3]]) == [False, True]
    for node in (("not", x), ("is_null", x), ("is_not_null", x),
                 ("is_null", A32), ("is_not_null", R.binop("Plus", A32, B32))):
        r = _check(node, cols, n, as_filter=True)
        if node[0] != "not":
            assert not (r.state == 1).any()


def test_cast_table():
    cols = _cols(N, 15)
    _check(R.cast(A32, I64), cols, N)
    _check(R.cast(A32, F64), cols, N)
    r = _check(R.cast(A64, F64), cols, N)           # rounds to nearest
    assert r.values[1] == 2.0**63
    r = _check(R.cast(A64, I32), cols, N)           # out of range -> null
    assert list(r.state[:9]) == [1, 1, 0, 0, 0, 1, 0, 0, 1]
    assert r.values[6] == 2**31 - 1 and r.values[7] == -2**31
    r = _check(R.cast(AF, I64), cols, N)            # trunc, saturate, NaN->0
    assert list(r.values[:3]) == [I64_MAX, I64_MIN, 0]
    assert list(r.values[5:9]) == [0, 0, I64_MAX, I64_MIN]
    r = _check(R.cast(AF, I32), cols, N)
    assert list(r.values[:5]) == [I32_MAX, I32_MIN, 0, I32_MAX, I32_MIN]
    _check(R.cast(AF, I32, try_=True), cols, N)
    _check(R.cast(A64, I32, try_=True), cols, N)
    _check(R.cast(AF, F64), cols, N)                # identity


def test_case_semantics():
    cols = _cols(N, 16)
    pos = R.binop("Gt", A32, R.lit(0, I32))
    # null condition is not taken; no ELSE gives null
    r = _check(R.case([(pos, B32)]), cols, N)
    assert (r.state == 1).any() and (r.state == 0).any()
    _check(R.case([(pos, B32)], else_=R.lit(-7, I32)), cols, N)
    # first valid-and-true WHEN wins
    _check(R.case([(pos, R.lit(1, I64)),
                   (R.binop("Gt", B32, R.lit(0, I32)), R.lit(2, I64)),
                   (("is_null", A32), R.lit(3, I64))],
                  else_=R.lit(None, I64)), cols, N)
    # CASE base WHEN v
    _check(R.case([(R.lit(0, I64), R.lit(100, I64)),
                   (R.lit(1, I64), A64)], else_=B64, base=B64), cols, N)
    _check(R.case([(R.binop("Lt", AF, BF), AF)], else_=BF), cols, N)


def test_poison_dropped_by_case_and_sc_but_kept_by_and():
    cols = _cols(N, 17)
    nz = R.binop("NotEq", B64, R.lit(0, I64))
    div = R.binop("Divide", A64, B64)
    bare = _check(div, cols, N)
    assert (bare.state == 2).sum() >= 3
    # row 0 is MIN / -1: b != 0 holds there, so it stays poison under the guard
    guarded = _check(R.case([(nz, div)], else_=R.lit(0, I64)), cols, N)
    assert guarded.state[0] == 2 and guarded.state[3] == 0
    assert (guarded.state == 2).sum() < (bare.state == 2).sum()
    # poison in the ELSE of a taken WHEN is dropped too
    r = _check(R.case([(R.binop("Eq", B64, R.lit(0, I64)), R.lit(0, I64))],
                      else_=R.binop("Modulo", A64, B64)), cols, N)
    assert r.state[3] == 0 and r.state[0] == 2
    big = R.binop("Gt", div, R.lit(1, I64))
    sc = _check(("sc_and", nz, big), cols, N, as_filter=True)
    assert sc.state[3] == 0 and not sc.values[3]
    plain = _check(R.binop("And", nz, big), cols, N, as_filter=True)
    assert plain.state[3] == 2
    # poison on the LEFT of SCAnd is never dropped
    left = _check(("sc_and", big, nz), cols, N, as_filter=True)
    assert left.state[3] == 2
    z = R.binop("Eq", B64, R.lit(0, I64))
    sco = _check(("sc_or", z, big), cols, N, as_filter=True)
    assert sco.state[3] == 0 and sco.values[3]
    assert _check(R.binop("Or", z, big), cols, N,
                  as_filter=True).state[3] == 2
    # a poisoned operand outranks a null one, and IsNull does not absorb it
    assert _check(("is_null", div), cols, N, as_filter=True).state[3] == 2


def test_filter_predicates_are_anded():
    cols = _cols(N, 18)
    p1, p2 = R.binop("Gt", A32, B32), ("is_not_null", AF)
    got_v, got_st = blaze_amd.debug_eval_expr(filter_plan([p1, p2]), cols)
    ref_v, ref_st = R.evaluate(R.binop("And", p1, p2), cols, N).canonical()
    np.testing.assert_array_equal(got_st, ref_st)
    np.testing.assert_array_equal(got_v, ref_v)


def test_mul_then_add_rounds_twice_on_the_host():
    rng = np.random.default_rng(19)
    n = 2000
    a, b = rng.random(n) * 3, rng.random(n) * 3
    cols = [(np.zeros(n, np.int32), None)] * 2 + \
        [(np.zeros(n, np.int64), None)] * 2 + [(a, None), (b, None)]
    e = R.binop("Plus", R.binop("Multiply", AF, BF), R.binop("Minus", BF, AF))
    got, st = blaze_amd.debug_eval_expr(project_plan([e]), cols)
    assert not st.any()
    np.testing.assert_array_equal(got, a * b + (b - a))


# ---- the reference itself vs pyarrow.compute --------------------------------

def _pa(v, valid, dtype):
    import pyarrow as pa
    return pa.array(np.asarray(v), mask=~np.asarray(valid),
                    type={I32: pa.int32(), I64: pa.int64(),
                          F64: pa.float64(), "bool": pa.bool_()}[dtype])


def _same(val, arr):
    import pyarrow as pa
    zero = False if pa.types.is_boolean(arr.type) else 0
    got = arr.fill_null(zero).to_numpy(zero_copy_only=False)
    valid = ~np.asarray(arr.is_null())
    np.testing.assert_array_equal(val.valid, valid)
    a = np.asarray(val.values)[valid]
    b = np.asarray(got)[valid].astype(a.dtype)
    np.testing.assert_array_equal(a, b)
    assert not val.poison.any()


def test_reference_agrees_with_pyarrow_compute():
    import pyarrow as pa
    import pyarrow.compute as pc

    cols = _cols(N, 20)
    cols[4] = (np.nan_to_num(cols[4][0], nan=1.0), cols[4][1])
    for ty, (x, y) in PAIRS.items():
        xa = _pa(*cols[x[1]], ty)
        ya = _pa(*cols[y[1]], ty)
        for op, f in (("Plus", pc.add), ("Minus", pc.subtract),
                      ("Multiply", pc.multiply)):   # unchecked: ints wrap
            _same(R.evaluate(R.binop(op, x, y), cols, N), f(xa, ya))
        _same(R.evaluate(("neg", x), cols, N), pc.negate(xa))
        _same(R.evaluate(("is_null", x), cols, N), pc.is_null(xa))
    tcols, bx, by, n = _tri(3)
    ba = _pa(tcols[0][0] > 0, tcols[0][1], "bool")
    bb = _pa(tcols[1][0] > 0, tcols[1][1], "bool")
    _same(R.evaluate(R.binop("And", bx, by), tcols, n), pc.and_kleene(ba, bb))
    _same(R.evaluate(R.binop("Or", bx, by), tcols, n), pc.or_kleene(ba, bb))
    _same(R.evaluate(("not", bx), tcols, n), pc.invert(ba))
    # if_else(cond, then, else): a null cond gives null in arrow's if_else but
    # takes ELSE in CASE, so compare where the condition is not null
    t32, e32 = _pa(*tcols[1], I32), pa.array(np.full(n, -7, np.int32))
    got = R.evaluate(R.case([(bx, B32)], else_=R.lit(-7, I32)), tcols, n)
    want = pc.if_else(ba, t32, e32)
    known = tcols[0][1]
    np.testing.assert_array_equal(
        got.valid[known], ~np.asarray(want.is_null())[known])
    both = known & got.valid
    np.testing.assert_array_equal(
        got.values[both],
        want.fill_null(0).to_numpy(zero_copy_only=False)[both])
    # exact casts
    a32 = _pa(*cols[0], I32)
    _same(R.evaluate(R.cast(A32, I64), cols, N), pc.cast(a32, pa.int64()))
    _same(R.evaluate(R.cast(A32, F64), cols, N), pc.cast(a32, pa.float64()))
    small = (cols[2][0] % 10**6, cols[2][1])
    c2 = list(cols)
    c2[2] = small
    _same(R.evaluate(R.cast(A64, I32), c2, N),
          pc.cast(_pa(*small, I64), pa.int32()))
    _same(R.evaluate(R.cast(A64, F64), c2, N),
          pc.cast(_pa(*small, I64), pa.float64()))
