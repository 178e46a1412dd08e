"""Every expression opcode on every route a loaded row can take to the GPU, against the 50-digit reference of
tests/expr_reference.py (the law, the bounds and the tables are stated there).

Layer 1: `Engine.eval_expression` (the interpreter, fp64) on the regular and the special tables of every opcode.
Layer 2: the same values out of the rollout kernels -- interpreter and hiprtc-specialised, fp64 and fp32.  The rollout is a
one-step evaluator: generation-1 map with mean 0 and scale 1, vt_mode 0, Euler, N = 1, dt = 2^-6, all cost weights zero.  With
theta = -0.0 the first predicted theta times 64 IS f_theta(x) (the step 2^-6 f is exact but for a subnormal result, which
costs at most 32 of T's smallest subnormal: added to the bound; -0.0 keeps the sign of a zero result); with gamma = -0.0 the
same for f_gamma.  At node 0 the slots x0..x8 and x14..x17 are copies of the state.  A table row is one problem of a batched
launch (step_batch_device, 64 problems of K = 67 equal candidates: a ragged workgroup); each model's first row also goes through
rollout_costs, where every lane must return the record's bits.  The interpreter's routes build nothing and take every table as
a row of its own; a hiprtc model costs a build, so there the tables are terms of sum rows (MERGED)."""
from functools import lru_cache

import numpy as np
import pytest

import expr_reference as er

pytestmark = pytest.mark.gpu

K = 67
H = 2.0 ** -6
P1 = (1.0, 0.5, -0.75)                                       # x0..x2: a geometry with a finite cable solve (P0 = 0, L = 3)
ROUTES = [("interpreter", "f64"), ("interpreter", "f32"), ("jit", "f64"), ("jit", "f32")]
ROUTE_IDS = ["%s-%s" % r for r in ROUTES]
WORST = {}                                                   # (route, dtype, opcode) -> largest error / bound seen


@pytest.fixture(scope="module")
def rv():
    import rovmpc
    return rovmpc


@pytest.fixture(scope="module")
def orc():
    from oracle import rovmpc_oracle
    return rovmpc_oracle


def note(route, dtype, op, r):
    key = (route, dtype, op)
    WORST[key] = max(WORST.get(key, 0.0), float(np.max(r)) if len(r) else 0.0)


def one_step_cfg(rv, route, dtype, N=1, integrator=None):
    return rv.MPCConfig(N=N, K=K, dtype=dtype, jit=(route == "jit"), no_builtin=True, vt_mode=0, integrator=rv.EULER if integrator is None else integrator,
                        dt=H, w_theta=0.0, w_gamma=0.0, w_u=0.0, w_T=0.0, w_taut=0.0, w_floor=0.0)


def model_of(rv, f_theta, f_gamma):
    return rv.DynamicsModel(np.zeros(18), np.ones(18), f_theta, f_gamma)


def state_of(row, which):
    """The state whose node-0 slots are `row`; the integrated variable starts at -0.0."""
    assert tuple(row[0:3]) == P1 and (row[14] == 0 if which == 0 else row[15] == 0)
    th, ga = (-0.0, row[15]) if which == 0 else (row[14], -0.0)
    return np.concatenate([[0.0, 0.0, 0.0], row[0:3], row[3:6], row[6:9], [th, ga, row[16], row[17]]])


B = 64


def evaluate(e, which, X):
    """f_theta (which = 0) or f_gamma (1) of the engine's model on the rows of X: one row per problem of a batched launch
    (step_batch_device, 64 problems of K = 67 candidates), read off the first predicted node of each problem's record.  The
    candidates of a problem are equal, so the record is candidate 0's whatever the costs are (ties, and costs that are NaN
    behind a non-finite angle, take the lowest index).  The first row also goes through rollout_costs: all 67 lanes must
    return the record's bits."""
    import torch
    dev = torch.device("cuda", 0)
    N = e.cfg.N
    tdt = torch.float64 if e.cfg.dtype == "f64" else torch.float32
    d_U = torch.zeros((B, K, N, 3), dtype=tdt, device=dev)
    R = e.result_len
    out = np.empty(len(X))
    stream = torch.cuda.current_stream().cuda_stream
    for at in range(0, len(X), B):
        blk = X[at:at + B]
        states = np.stack([state_of(row, which) for row in blk] + [state_of(blk[0], which)] * (B - len(blk)))
        d_s = torch.tensor(states, device=dev)
        d_r = torch.full((B, R), 7.0, dtype=torch.float64, device=dev)
        e.step_batch_device(B, d_s.data_ptr(), d_U.data_ptr(), d_r.data_ptr(), stream)
        torch.cuda.synchronize()
        res = d_r.cpu().numpy()
        assert np.all(res[:len(blk), 1] == 0), ("winner", res[:len(blk), 1])
        out[at:at + len(blk)] = res[:len(blk), 5:].reshape(len(blk), N + 1, 2)[:, 1, which] * 64.0
    _, traj = e.rollout_costs(state_of(X[0], which), np.zeros((K, N, 3), dtype=e.cfg.np_dtype), return_traj=True)
    v = np.ascontiguousarray(traj[:, 1, which])
    bits = v.view(np.uint64 if v.dtype == np.float64 else np.uint32)
    assert np.all(bits == bits[0]), ("lanes differ", v)
    one = float(v[0]) * 64.0
    assert one == out[0] or (np.isnan(one) and np.isnan(out[0])), (one, out[0])
    return out


def rows(F, **cols):
    X = er._rows(F, **cols)
    X[:, 0:3] = P1
    return X


def check(case, got, route, dtype):
    F = er.FMT[dtype]
    r = case.ratios(got, extra=32 * F.tiny)
    note(route, dtype, case.op, r)
    bad = int(np.argmax(r))
    assert r.max() <= 1.0, (route, dtype, case.name, case.text, bad, case.X[bad][[3, 4, 5, 6, 14, 15, 16, 17]], got[bad], case.want[bad], r.max())
    return r


# ---- layer 2, first: the evaluator itself ------------------------------------------------------------------------------------------
# one pure identity model, and one whose rows are sums of slots of which one at a time is not zero (x + 0 + 0 + 0 is x, bit for bit)
IDENTITY = [("x15", "x14"), ("x3 + x15 + x16 + x17", "x14 + x16 + x17 + x8")]


@pytest.mark.parametrize("route,dtype", ROUTES, ids=ROUTE_IDS)
def test_identity_rows_return_the_input_bit_for_bit(rv, route, dtype):
    F = er.FMT[dtype]
    rng = np.random.default_rng(5)
    n = 12
    vals = lambda: np.concatenate([rng.standard_normal(n - 4) * 10.0 ** rng.integers(-6, 6, n - 4), [F.max, -F.max / 3, 2.0 ** -100, -1.0]])
    for ft, fg in IDENTITY:
        with rv.Engine(one_step_cfg(rv, route, dtype), model_of(rv, ft, fg)) as e:
            assert e.model_path == route
            for which, text in ((0, ft), (1, fg)):
                for slot in [int(t[1:]) for t in text.split(" + ")]:
                    X = rows(F, **{"x%d" % slot: vals()})
                    assert slot != (14 if which == 0 else 15)
                    got = evaluate(e, which, X)
                    assert np.array_equal(got, X[:, slot]), (route, dtype, text, slot, got, X[:, slot])


# ---- layer 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def interp64(rv):
    with rv.Engine(rv.MPCConfig(N=1, K=1, force_interpreter=True)) as e:
        yield e


def test_every_opcode_on_the_interpreter(rv, interp64):
    """eval_expression on the regular and special tables, fp64: regular points within bound; NaN where NumPy has NaN, +-inf and
    +-0 with NumPy's sign, everything else within bound."""
    cases = er.regular_cases("f64") + er.special_cases("f64") + [er.division_cases("f64")]
    assert {c.op for c in cases} == set(rv.expr.OP)
    F = er.F64
    extra = [er.Case("PUSH_C", "const", t, er._rows(F, x3=[1.5, -2.0, 0.0, -0.0], x4=[0.25, -1.0, 3.0, -0.0], x15=[0.5, -0.0, 7.0, 1e300]), "f64")
             for t in er.CONSTANT_ROWS]
    rng = np.random.default_rng(11)
    wide = rng.standard_normal((64, 18)) * 4
    extra += [er.Case("ADD", "depth 16", er.deep_expression(), wide, "f64"), er.Case("ADD", "256 instructions", er.long_expression(), wide, "f64")]
    for c in cases + extra:
        assert len(c.X) <= 4096
        consts = []
        prog = rv.expr.compile_expression(c.text, consts)
        got = interp64.eval_expression(prog.code, consts, c.X)
        r = c.ratios(got)
        note("eval_expression", "f64", c.op, r)
        bad = int(np.argmax(r))
        assert r.max() <= 1.0, (c.name, c.text, bad, c.X[bad][[0, 1, 3, 15]], got[bad], c.want[bad], r.max())


# ---- layer 2: the regular tables of every opcode out of the rollout kernels ----------------------------------------------------------------
def to_state_slots(text, which):
    """The table's x0 / x1 moved to slots the rollout copies from the state: x0 -> x15 (dtheta/dt row) or x14 (dgamma/dt), x1 -> x16."""
    import re
    return re.sub(r"\bx([01])\b", lambda m: {"0": "x15" if which == 0 else "x14", "1": "x16"}[m.group(1)], text)


N_REGULAR = 34                                               # len(er.regular_cases(.)), two tables per model
REGULAR_PAIRS = [(i, i + 1) for i in range(0, N_REGULAR, 2)]
INTERPRETER = [r for r in ROUTES if r[0] == "interpreter"]
HIPRTC = [r for r in ROUTES if r[0] == "jit"]


@pytest.mark.parametrize("route,dtype", INTERPRETER, ids=["%s-%s" % r for r in INTERPRETER])
@pytest.mark.parametrize("pair", REGULAR_PAIRS, ids=["tables-%d-%d" % p for p in REGULAR_PAIRS])
def test_regular_tables_through_the_rollout(rv, route, dtype, pair):
    """The interpreter's routes build nothing: every table is a row of its own, two tables per model (the hiprtc routes take
    the same tables as sums of terms: test_merged_tables_on_the_hiprtc_routes)."""
    F = er.FMT[dtype]
    assert len(er.regular_cases(dtype)) == N_REGULAR
    cases = [er.regular_cases(dtype)[i] for i in pair]
    texts = [to_state_slots(c.text, which) for which, c in enumerate(cases)]
    with rv.Engine(one_step_cfg(rv, route, dtype), model_of(rv, *texts)) as e:
        assert e.model_path == route
        for which, (c, text) in enumerate(zip(cases, texts)):
            X = c.X.copy()
            X[:, 15 if which == 0 else 14] = c.X[:, 0]
            X[:, 16] = c.X[:, 1]
            X[:, 0:3] = P1
            moved = er.Case(c.op, c.name, text, X, dtype)
            assert np.array_equal(moved.want, c.want, equal_nan=True)
            check(moved, evaluate(e, which, X), route, dtype)


# ---- layer 2: special operands through the rollout, the hiprtc route included ----------------------------------------------------------
POWI_E = (0, 1, 3, 5, 30, -1, -2, -3, -7, (1 << 22) - 1, -((1 << 22) - 1))
_POWI = [("POWI", "x15**(%d)" % e) for e in POWI_E] + [("POWI", "x15**(-5)")]
# (opcode, dtheta/dt row, opcode, dgamma/dt row): the state operand is x15 in the first row and x14 in the second
SPECIAL_MODELS = ([("DIV", "x15 / x3", "DIV", "x14 / x3"), ("POW", "x15**x3", "POW", "pow(x14, x3)"), ("LOG", "log(x15)", "SQRT", "sqrt(x14)"),
                   ("LOG", "log(x3)", "SQRT", "sqrt(x3)")]
                  + [(_POWI[i][0], _POWI[i][1], _POWI[i + 1][0], _POWI[i + 1][1].replace("x15", "x14")) for i in range(0, len(_POWI), 2)]
                  + [("SIN", "sin(x15)", "SAFE_SQRT", "safe_sqrt(x14)"), ("EXP", "exp(x15)", "TANH", "tanh(x14)"),
                     ("ABS", "abs(x15)", "NEG", "-x14"), ("SAFE_LOG", "safe_log(x15)", "COS", "cos(x14)")])
CONSTANT_MODELS = [("PUSH_C", "x15 + -1e999", "PUSH_C", "x3 * -0.0"), ("PUSH_C", "x15 * (1e999 - 1e999)", "PUSH_C", "x4 / 1e999")]
INF_NAN_MODEL = ("PUSH_C", "x15 + -1e999", "PUSH_C", "x14 * (1e999 - 1e999)")     # hiprtc: -0.0 and x / inf are terms of MERGED's signed-zero row
SPECIAL_RUNS = ([(m, r, d) for m in SPECIAL_MODELS + CONSTANT_MODELS for r, d in INTERPRETER] + [(INF_NAN_MODEL, r, d) for r, d in HIPRTC])


def special_columns(op, text, fmt):
    """(x3, state operand) columns of the special table that belongs to the row `text`."""
    F = er.FMT[fmt]
    sp = er.special_cases(fmt)
    table = lambda t: np.concatenate([c.X[:, 0] for c in sp if c.text == t])
    if op == "DIV":
        c = er.division_cases(fmt)
        return c.X[:, 3], c.X[:, 15]
    if op == "POW":
        c = [c for c in sp if c.text == "x0**x1"][0]
        return c.X[:, 1], c.X[:, 0]
    if op in ("LOG", "SQRT", "SIN", "SAFE_SQRT", "EXP", "TANH", "ABS", "SAFE_LOG", "COS") or text == "-x14":
        col = table("-x0" if text == "-x14" else text[:text.index("(")] + "(x0)")
        return (col, np.zeros(len(col))) if "x3" in text else (np.zeros(len(col)), col)
    if op == "POWI":
        e = text[text.index("**"):]
        col = table("x0" + e) if e != "**(-5)" else table("x0**(-7)")
        return np.zeros(len(col)), col
    col = np.array([1.5, -2.0, 0.0, -0.0, F.max])
    return col, col[::-1].copy()


@pytest.mark.parametrize("model,route,dtype", SPECIAL_RUNS, ids=["%s|%s-%s-%s" % (m[1], m[3], r, d) for m, r, d in SPECIAL_RUNS])
def test_special_operands_through_the_rollout(rv, route, dtype, model):
    """The special tables of / (the divisor in a stage-invariant slot: the reciprocal rewrite), pow, x**e, log and sqrt, and the
    non-finite and signed-zero constants, out of the rollout kernels."""
    F = er.FMT[dtype]
    with rv.Engine(one_step_cfg(rv, route, dtype), model_of(rv, model[1], model[3])) as e:
        assert e.model_path == route
        for which, (op, text) in enumerate((model[0:2], model[2:4])):
            x3, sv = special_columns(op, text, dtype)
            X = rows(F, x3=x3, x4=x3, **{"x15" if which == 0 else "x14": sv})
            e_powi = int(text[text.index("(") + 1:-1]) if op == "POWI" else None
            pinned = er.stated_pins(op, x3 if "x3" in text else sv, F, e_powi)          # the stated deviations (include/rovmpc.h)
            if op == "SIN":
                pinned = {i: 0.0 for i in range(len(sv)) if sv[i] == 0 and np.signbit(sv[i])}
            check(er.Case(op, "special", text, X, dtype, pinned), evaluate(e, which, X), route, dtype)


# ---- layer 2: the same tables on the hiprtc routes, as sums of terms ---------------------------------------------------------------------
# A hiprtc model costs a build, so there a row is a SUM of terms on disjoint slots and each term's table is run with the other
# terms at a neutral operand.  Where every neutral term is an exact zero the sum IS the active term (a row whose neutral terms are
# all -0 keeps the sign of a zero result too); the rows marked "offset" hold the opcodes with no such operand (cos, exp, safe_log,
# x**e with e <= 0): there the other terms add exact constants, a zero result shows as that constant, and the bound is the sum's.
# term: (opcode, text, table text, kind, slots, neutral operands[, table columns])
def T(op, text, table, kind, slots, neutral, src=(0, 1)):
    return (op, text, table, kind, slots, neutral, src)


MERGED = {
    "arithmetic": ([T("ADD", "(x15 + x3)", "x0 + x1", "reg", (15, 3), (0.0, 0.0)), T("SUB", "(x16 - x4)", "x0 - x1", "reg", (16, 4), (0.0, 0.0)),
                    T("MUL", "x17 * x5", "x0 * x1", "reg", (17, 5), (0.0, 0.0)), T("DIV", "x6 / x7", "x0 / x1", "reg", (6, 7), (0.0, 1.0))],
                   [T("NEG", "-(x14 + x3)", "-(x0 + x1)", "reg", (14, 3), (0.0, 0.0)), T("NEG", "neg(x16 * x4)", "neg(x0 * x1)", "reg", (16, 4), (0.0, 0.0)),
                    T("ABS", "abs(x17 - x5)", "abs(x0 - x1)", "reg", (17, 5), (0.0, 0.0)), T("ABS", "Abs(x6)", "Abs(x0)", "reg", (6,), (0.0,)),
                    T("SQUARE", "square(x7)", "square(x0)", "reg", (7,), (0.0,)), T("SQUARE", "x8**2", "x0**2", "reg", (8,), (0.0,))]),
    "functions": ([T("SIN", "sin(x15)", "sin(x0)", "reg", (15,), (0.0,)), T("TANH", "tanh(x16)", "tanh(x0)", "reg", (16,), (0.0,)),
                   T("SQRT", "sqrt(x17)", "sqrt(x0)", "reg", (17,), (0.0,)), T("SAFE_SQRT", "safe_sqrt(x3)", "safe_sqrt(x0)", "reg", (3,), (0.0,)),
                   T("LOG", "log(x4)", "log(x0)", "reg", (4,), (1.0,)), T("PUSH_F", "(x5 - x6)", "x17 - x3", "reg", (5, 6), (0.0, 0.0), (17, 3))],
                  [T("POW", "x14**x3", "x0**x1", "reg", (14, 3), (0.0, 1.0)), T("POW", "pow(x16, x4)", "pow(x0, x1)", "reg", (16, 4), (0.0, 1.0)),
                   T("POW", "x17**2.5", "x0**2.5", "reg", (17,), (0.0,))]),
    "offset|powers": ([T("COS", "cos(x15)", "cos(x0)", "reg", (15,), (0.0,)), T("EXP", "exp(x16)", "exp(x0)", "reg", (16,), (0.0,)),
                       T("SAFE_LOG", "safe_log(x17)", "safe_log(x0)", "reg", (17,), (1.0,)), T("POW", "x3^-0.5", "x0^-0.5", "reg", (3,), (1.0,)),
                       T("POW", "1.5**x4", "1.5**x0", "reg", (4,), (0.0,)),
                       T("PUSH_C", "(x5 * 0.1 + 1.0000000000000002)", "x0 * 0.1 + 1.0000000000000002", "reg", (5,), (0.0,)),
                       # special tables of the opcodes without a zero: 1 / sin(x) shows the sign of sin(-0.0) as the sign of an infinity
                       T("EXP", "exp(x6)", "exp(x0)", "spec", (6,), (0.0,)), T("SAFE_LOG", "safe_log(x7)", "safe_log(x0)", "spec", (7,), (1.0,)),
                       T("SIN", "1.0 / sin(x8)", "sin(x0)", "spec", (8,), (1.5,))],
                      [T("POWI", "x14**3", "x0**3", "reg", (14,), (0.0,)), T("POWI", "x16**5", "x0**5", "reg", (16,), (0.0,)),
                       T("POWI", "x17**30", "x0**30", "reg", (17,), (0.0,)), T("POWI", "x3**(-1)", "x0**(-1)", "reg", (3,), (1.0,)),
                       T("POWI", "x4**(-2)", "x0**(-2)", "reg", (4,), (1.0,)), T("POWI", "x5**(-3)", "x0**(-3)", "reg", (5,), (1.0,)),
                       T("POWI", "x6**(-7)", "x0**(-7)", "reg", (6,), (1.0,)), T("POWI", "x7**(0)", "x0**(0)", "spec", (7,), (0.0,))]),
    # special operands.  First model: every neutral term is -0, so +-0 results keep their sign; the divisor of / is stage-invariant
    "special|signed zeros": ([T("DIV", "x15 / x3", None, "div", (15, 3), (-0.0, 1.0)), T("POW", "x16**x4", "x0**x1", "spec", (16, 4), (-0.0, 1.0)),
                              T("SQRT", "sqrt(x17)", "sqrt(x0)", "spec", (17,), (-0.0,)), T("POWI", "x5**(1)", "x0**(1)", "spec", (5,), (-0.0,)),
                              T("POWI", "x6**(3)", "x0**(3)", "spec", (6,), (-0.0,)), T("POWI", "x7**(5)", "x0**(5)", "spec", (7,), (-0.0,)),
                              T("POWI", "x8**(4194303)", "x0**(4194303)", "spec", (8,), (-0.0,))],
                             [T("DIV", "x14 / x3", None, "div", (14, 3), (-0.0, 1.0)), T("POW", "pow(x16, x4)", "pow(x0, x1)", "spec", (16, 4), (-0.0, 1.0)),
                              T("SQRT", "sqrt(x5)", "sqrt(x0)", "spec", (5,), (-0.0,)), T("PUSH_C", "x6 * -0.0", "x3 * -0.0", "const", (6,), (1.0,)),
                              T("PUSH_C", "x7 / 1e999", "x4 / 1e999", "const", (7,), (-1.0,)),
                              # odd negative powers: 1 / (-inf)**|e| = -0 is their neutral value, so the sign of their zeros shows
                              T("POWI", "x17**(-1)", "x0**(-1)", "spec", (17,), (-np.inf,)), T("POWI", "x8**(-3)", "x0**(-3)", "spec", (8,), (-np.inf,))]),
    # every neutral term is +0: a zero result shows against a subnormal one (the stated x**e, e < 0, and fp32 safe_sqrt)
    "special|zeros": ([T("LOG", "log(x15)", "log(x0)", "spec", (15,), (1.0,)), T("POWI", "x16**(30)", "x0**(30)", "spec", (16,), (0.0,)),
                       T("SIN", "sin(x17)", "sin(x0)", "spec", (17,), (0.0,)), T("SAFE_SQRT", "safe_sqrt(x3)", "safe_sqrt(x0)", "spec", (3,), (0.0,)),
                       T("LOG", "log(x4)", "log(x0)", "spec", (4,), (1.0,)), T("TANH", "tanh(x5)", "tanh(x0)", "spec", (5,), (0.0,)),
                       T("ABS", "abs(x6)", "abs(x0)", "spec", (6,), (0.0,)), T("NEG", "-x7", "-x0", "spec", (7,), (0.0,))],
                      [T("POWI", "x14**(-1)", "x0**(-1)", "spec", (14,), (np.inf,)), T("POWI", "x16**(-2)", "x0**(-2)", "spec", (16,), (np.inf,)),
                       T("POWI", "x17**(-3)", "x0**(-3)", "spec", (17,), (np.inf,)), T("POWI", "x3**(-7)", "x0**(-7)", "spec", (3,), (np.inf,)),
                       T("POWI", "x4**(-4194303)", "x0**(-4194303)", "spec", (4,), (np.inf,))]),
}


def term_table(term, fmt):
    """(columns of the term's operands, surrogate operand per pinned row) from the term's table."""
    op, text, table, kind, slots, neutral, src = term
    F = er.FMT[fmt]
    if kind == "div":
        c = er.division_cases(fmt)
        return [c.X[:, 15], c.X[:, 3]], {}
    if kind == "const":                     # a non-finite or signed-zero constant against ordinary and zero operands
        return [np.array([1.5, -2.0, 0.0, -0.0, F.max])], {}
    cases = [c for c in (er.regular_cases(fmt) if kind == "reg" else er.special_cases(fmt)) if c.text == table]
    assert cases, table
    cols = [np.concatenate([c.X[:, j] for c in cases]) for j in src[:len(slots)]]
    # a stated deviation of the term (include/rovmpc.h) enters the row through an operand that gives the stated value exactly:
    # 1 / x**|e| = +-0 at x = +-inf, sqrt(+-0) = +-0, sin(+0) = +0
    e = int(table[table.index("(") + 1:-1]) if op == "POWI" and "(" in table else None
    pins = er.stated_pins(op, cols[0], F, e)
    if op == "SIN":
        pins = {i: 0.0 for i in range(len(cols[0])) if cols[0][i] == 0 and np.signbit(cols[0][i])}
    sur = {}
    for i, v in pins.items():
        if op == "POWI":
            sur[i] = np.copysign(np.inf, cols[0][i]) if e % 2 else np.inf
        else:
            sur[i] = v
    return cols, sur


@pytest.mark.parametrize("route,dtype", HIPRTC, ids=["%s-%s" % r for r in HIPRTC])
@pytest.mark.parametrize("name", list(MERGED))
def test_merged_tables_on_the_hiprtc_routes(rv, route, dtype, name):
    F = er.FMT[dtype]
    texts = [" + ".join(t[1] for t in terms) for terms in MERGED[name]]
    with rv.Engine(one_step_cfg(rv, route, dtype), model_of(rv, *texts)) as e:
        assert e.model_path == route
        for which, (terms, text) in enumerate(zip(MERGED[name], texts)):
            for term in terms:
                op, _, _, kind, slots, _, _ = term
                cols, sur = term_table(term, dtype)
                n = len(cols[0])
                base = {"x%d" % s: np.full(n, v) for t in terms for s, v in zip(t[4], t[5])}
                X = rows(F, **{**base, **{"x%d" % s: c for s, c in zip(slots, cols)}})
                pinned = {}
                if sur:
                    Xs = X.copy()
                    for i, v in sur.items():
                        Xs[i, slots[0]] = v
                    ws = er.numpy_values(text, Xs, F)
                    pinned = {i: float(ws[i]) for i in sur}
                if kind == "div":           # stated: the generator's a * (1 / D) where 1 / D is not a normal number (the other terms are -0)
                    with np.errstate(all="ignore"):
                        a, r = cols[0].astype(F.np), F.np(1) / cols[1].astype(F.np)
                        odd = ~(np.isfinite(r) & (np.abs(r) >= np.finfo(F.np).tiny))
                        pinned = {int(i): float(a[i] * r[i]) for i in np.flatnonzero(odd)}
                check(er.Case(op, name, text, X, dtype, pinned), evaluate(e, which, X), route, dtype)


# ---- layer 2: the code generator's structure -------------------------------------------------------------------------------------------
# (three opcodes in a row ask for 9 e[k] and 3 g[k], four for 12 and 4: the last ones stay inline, which is a case of its own)
HEAVY_GROUPS = [("exp", "log", "sqrt"), ("tanh", "safe_sqrt", "sin"), ("pow", "safe_log", "cos", "powi_neg")]


def group_rows(group):
    return " + ".join(er.composite_theta(op) for op in group), " + ".join(er.composite_gamma(op) for op in group)


COMPOSITES = {"+".join(g): group_rows(g) for g in HEAVY_GROUPS}
# more hoistable subtrees than e[] and g[] hold (the gamma row keeps the gamma path candidate-invariant, so g[] exists), a
# constant that needs all 17 digits; a row of exactly 256 instructions and one of stack depth exactly 16
COMPOSITES["lists-overflow|17-digits"] = (er.OVERFLOW_THETA, "x17 * 0.12345678901234568 + 0.30000000000000004 - x15 * 0.25 + abs(x17 - 1.0) * 0.5"
                                                             " - square(x17) * 0.125 + -(x15 + x17) * 0.0625")
COMPOSITES["256-instructions|depth-16"] = (er.long_expression(), er.deep_expression())
GAMMA_INVARIANT = set(COMPOSITES) - {"256-instructions|depth-16"}
NPTS = 24


def composite_points(F, which, seed):
    """Positive, moderate slots: every heavy opcode is inside its domain in each dependency class."""
    rng = np.random.default_rng(seed)
    cols = {"x%d" % j: rng.uniform(0.3, 1.7, NPTS) for j in (3, 4, 5, 6, 7, 8, 14, 15, 16, 17)}
    cols["x14" if which == 0 else "x15"] = np.zeros(NPTS)
    return rows(F, **cols)


@lru_cache(maxsize=None)
def composite_case(name, which, dtype):
    """The reference of a composite row: built once, shared by the routes and the two generator settings."""
    return er.Case("composite", name, COMPOSITES[name][which], composite_points(er.FMT[dtype], which, 40 + which), dtype)


COMPOSITE_RUNS = [(r, d, True) for r, d in ROUTES] + [(r, d, False) for r, d in ROUTES if r == "jit"]     # ROVMPC_JIT_NO_HOIST acts on the generator alone


@pytest.mark.parametrize("route,dtype,hoist", COMPOSITE_RUNS, ids=["%s-%s%s" % (r, d, "" if h else "-no-hoist") for r, d, h in COMPOSITE_RUNS])
@pytest.mark.parametrize("name", list(COMPOSITES))
def test_composites_on_every_route(rv, monkeypatch, name, route, dtype, hoist):
    """Each heavy opcode once in each dependency class the code generator distinguishes (tests/expr_reference.py:
    composite_theta), within bound of the 50-digit value on all four routes, with and without the hoisting."""
    if not hoist:
        monkeypatch.setenv("ROVMPC_JIT_NO_HOIST", "1")
    F = er.FMT[dtype]
    ft, fg = COMPOSITES[name]
    with rv.Engine(one_step_cfg(rv, route, dtype), model_of(rv, ft, fg)) as e:
        assert e.model_path == route
        if route == "jit" and name in GAMMA_INVARIANT:
            assert e.model_structure == {"gamma_invariant"}           # the x17-only subtrees of dtheta/dt become g[k]
        for which, text in ((0, ft), (1, fg)):
            X = composite_points(F, which, 40 + which)
            case = composite_case(name, which, dtype)
            assert np.all(np.isfinite(case.want)) and all(r is not None for r in case.ref), name
            r = check(case, evaluate(e, which, X), route, dtype)
            note(route + ("" if hoist else "/no-hoist"), dtype, name, r)


ORACLE_RK4 = {}


def oracle_cfg(orc, cfg):
    return orc.MPCConfig(N=cfg.N, dt=cfg.dt, v_scale=cfg.v_scale, L=cfg.L, cable_wet_weight=cfg.cable_wet_weight, c_lo=cfg.c_lo, c_hi=cfg.c_hi,
                         n_shape_pts=cfg.n_shape_pts, up=1.0, vt_mode=cfg.vt_mode, prev_mode=cfg.prev_mode, integrator=cfg.integrator,
                         w_theta=cfg.w_theta, w_gamma=cfg.w_gamma, w_u=cfg.w_u, w_T=cfg.w_T, w_taut=cfg.w_taut, rho_taut=cfg.rho_taut,
                         w_floor=cfg.w_floor, z_floor=cfg.z_floor, theta_ref=cfg.theta_ref, gamma_ref=cfg.gamma_ref, U_ref=tuple(cfg.U_ref),
                         feature_map=cfg.feature_map)


@pytest.mark.parametrize("route", ["interpreter", "jit"])
@pytest.mark.parametrize("name", list(COMPOSITES))
def test_composites_in_a_small_rk4_rollout(rv, orc, name, route):
    """N = 3, RK4, fp64, against the oracle at the suite's 1e-8: the stage loop, the midpoint rows and the g[k] table see every
    opcode too."""
    ft, fg = COMPOSITES[name]
    cfg = one_step_cfg(rv, route, "f64", N=3, integrator=rv.RK4)
    cfg.w_theta, cfg.w_gamma = 1.0, 1.0
    rng = np.random.default_rng(3)
    U = 1.0 + 0.02 * (np.arange(3)[None, :, None] + 1) + 0.005 * rng.uniform(0, 1, (K, 3, 3))      # rising: the acceleration slots stay positive
    state = np.concatenate([[0.0, 0.0, 0.0], P1, [1.0, 1.0, 1.0], [0.5, 0.6, 0.7], [0.4, 0.9, 0.45, 0.85]])
    model = model_of(rv, ft, fg)
    with rv.Engine(cfg, model) as e:
        assert e.model_path == route
        J, traj = e.rollout_costs(state, U, return_traj=True)
    if name not in ORACLE_RK4:               # computed once, shared by both routes, left unchanged
        omodel = orc.DynamicsModel(model.mean, model.scale, orc.SymbolicModel(ft), orc.SymbolicModel(fg))
        ORACLE_RK4[name] = orc.rollout_vec(oracle_cfg(orc, cfg), omodel, orc.MPCState.from_array(state), U)[:2]
    Jo, trajo = ORACLE_RK4[name]
    assert np.all(np.isfinite(trajo))
    np.testing.assert_allclose(traj, trajo, rtol=1e-8)
    np.testing.assert_allclose(J, Jo, rtol=1e-8)


@pytest.fixture(scope="module", autouse=True)
def report():
    """When the module is through: the largest error / bound per route, type and opcode (the figures of DESIGN.md section 3)."""
    yield
    import sys
    lines = ["", "largest error / bound per route, type and opcode"] + ["  %-22s %s %-28s %.3f" % (k + (v,)) for k, v in sorted(WORST.items())]
    sys.__stdout__.write("\n".join(lines) + "\n")


def test_the_loaded_models_hold_every_opcode(rv):
    """All 19 opcodes are in the rows this file loads on the four routes."""
    texts = [t for m in COMPOSITES.values() for t in m] + [t for m in SPECIAL_MODELS for t in (m[1], m[3])]
    texts += [to_state_slots(c.text, 0) for c in er.regular_cases("f64")]
    merged = [" + ".join(t[1] for t in terms) for m in MERGED.values() for terms in m]
    hiprtc = set()
    for t in merged + [t for m in COMPOSITES.values() for t in m]:
        hiprtc |= {w & 0xFF for w in rv.expr.compile_expression(t, []).code}
    assert hiprtc == set(rv.expr.OP.values())
    seen = set()
    for t in texts:
        seen |= {w & 0xFF for w in rv.expr.compile_expression(t, []).code}
    assert seen == set(rv.expr.OP.values()) and len(seen) == 19
