"""tests/expr_reference.py on the CPU: NumPy's evaluation of every table stays within the bounds the GPU tests assert, the
bounds notice a wrong interpreter, and the compiler emits what the device decodes."""
import numpy as np
import pytest

import expr_reference as er

FMTS = ("f64", "f32")


@pytest.fixture(scope="module")
def expr():
    from rovmpc import expr
    return expr


def all_cases(fmt):
    return er.regular_cases(fmt) + er.special_cases(fmt) + [er.division_cases(fmt)]


# ---- NumPy mirror of interp_eval (csrc/rollout_kernels.h) over the product's bytecode, with the mutations of the test below ---
def mirror(expr, text, X, fmt, mutant=None):
    F = er.FMT[fmt]
    T = F.np
    consts = []
    prog = expr.compile_expression(text, consts)
    ck = np.asarray(consts if consts else [0.0], dtype=np.float64).astype(T)
    X = np.asarray(X, dtype=np.float64).astype(T)
    n = X.shape[0]
    inv = {v: k for k, v in expr.OP.items()}
    st = []
    with np.errstate(all="ignore"):
        for ins in prog.code:
            op, arg = inv[ins & 0xFF], ins >> 8
            if op == "PUSH_C":
                st.append(np.full(n, ck[arg], dtype=T)); continue
            if op == "PUSH_F":
                st.append(X[:, arg].copy()); continue
            if op in ("ADD", "SUB", "MUL", "DIV", "POW"):
                b = st.pop(); a = st.pop()
                if mutant == "swap_" + op:
                    a, b = b, a
                st.append({"ADD": np.add, "SUB": np.subtract, "MUL": np.multiply, "DIV": np.divide, "POW": np.power}[op](a, b).astype(T))
                continue
            x = st.pop()
            if op == "NEG":
                r = -x
            elif op == "SIN":
                r = np.where((x == 0) & np.signbit(x), T(0), np.sin(x))          # the stated deviation
            elif op == "COS":
                r = np.cos(x)
            elif op == "TANH":
                r = np.tanh(x)
                if mutant == "tanh_small":
                    r = np.where(np.abs(x) < 2.0 ** -20, x, r)
            elif op == "ABS":
                r = np.abs(x)
            elif op == "SQUARE":
                r = x + x if mutant == "square_2x" else x * x
            elif op == "EXP":
                r = np.exp(x)
            elif op == "LOG":
                r = np.log(x)
            elif op == "SQRT":
                r = np.sqrt(sqrt_operand(x))
            elif op == "POWI":
                e = arg - (1 << 24) if arg >= (1 << 23) else arg
                e += {"powi_plus": 1, "powi_minus": -1}.get(mutant, 0)
                if mutant == "powi_sign":
                    e = abs(e)
                ae, b, r = abs(e), x.copy(), np.ones(n, dtype=T)
                while ae:
                    if ae & 1:
                        r = r * b
                    b = b * b
                    ae >>= 1
                r = T(1) / r if e < 0 else r
            elif op == "SAFE_LOG":
                r = np.log(np.abs(x) + T(1e-6 if mutant == "safe_log_eps" else 1e-5))
            elif op == "SAFE_SQRT":
                r = np.sqrt(sqrt_operand(x if mutant == "safe_sqrt_noabs" else np.abs(x)))
            else:
                raise AssertionError(op)
            st.append(np.asarray(r, dtype=T))
    assert len(st) == 1
    return st[0].astype(np.float64)


def sqrt_operand(x):
    """m_sqrt(float) is v_sqrt_f32, which reads a subnormal operand as a zero of its sign (the stated deviation)."""
    if x.dtype != np.float32:
        return x
    return np.where((x != 0) & (np.abs(x) < np.finfo(np.float32).tiny), np.copysign(np.float32(0), x), x)


MUTANTS = {"swap_SUB": "SUB", "swap_DIV": "DIV", "swap_POW": "POW", "powi_plus": "POWI", "powi_minus": "POWI", "powi_sign": "POWI",
           "safe_log_eps": "SAFE_LOG", "safe_sqrt_noabs": "SAFE_SQRT", "square_2x": "SQUARE", "tanh_small": "TANH"}
# Mutants the tables of one format cannot see, with the size at which they can: tanh(x) = x below 2^-20 is wrong by x^2 / 3
# relative, under fp32's u there; taken below 2^-10 instead it shows (fp64 sees it at 2^-20).
UNDETECTED = {("tanh_small", "f32"): 2.0 ** -10}


@pytest.mark.parametrize("fmt", FMTS)
def test_numpy_stays_within_the_bounds(fmt, capsys):
    """The condition the reference passes alone: the oracle's NumPy evaluation of every case is within bound -- exact on the
    special values -- on every table (the pinned rows are the stated deviations from NumPy and are left out here)."""
    worst = {}
    for c in all_cases(fmt):
        r = c.ratios(c.numpy)
        keep = np.ones(len(r), bool); keep[c.pinned] = False
        worst[c.op] = max(worst.get(c.op, 0.0), float(r[keep].max()))
        assert r[keep].max() <= 1.0, (c.name, c.text, int(np.argmax(np.where(keep, r, 0))), r.max())
    with capsys.disabled():
        print("\n[%s] NumPy error / bound per opcode: %s" % (fmt, "  ".join("%s %.2f" % kv for kv in sorted(worst.items()))))
    assert set(worst) == set(er_ops())                             # all 19 opcodes have a table


def er_ops():
    return ["PUSH_C", "PUSH_F", "ADD", "SUB", "MUL", "DIV", "NEG", "SIN", "COS", "TANH", "ABS", "SQUARE", "EXP", "LOG", "SQRT", "POW",
            "POWI", "SAFE_LOG", "SAFE_SQRT"]


@pytest.mark.parametrize("fmt", FMTS)
def test_recorded_numpy_model_still_holds(fmt, capsys):
    """NP_MODEL is NumPy's own error over the regular tables; the bound of tanh, exp, log, sqrt and pow is NP_MODEL + 1."""
    got = er.measure_numpy(fmt)
    with capsys.disabled():
        print("\n[%s] NumPy model: %s" % (fmt, "  ".join("%s %.3f (recorded %.2f)" % (k, v, er.NP_MODEL[(k, fmt)]) for k, v in got.items())))
    for fn, v in got.items():
        assert v <= er.NP_MODEL[(fn, fmt)] + 0.05, (fn, v)         # the record reproduces (slack: another NumPy build may round elsewhere)


@pytest.mark.parametrize("fmt", FMTS)
def test_the_mirror_of_the_interpreter_is_within_bound(expr, fmt):
    for c in all_cases(fmt):
        r = c.ratios(mirror(expr, c.text, c.X, fmt))
        assert r.max() <= 1.0, (c.name, c.text, int(np.argmax(r)), c.X[int(np.argmax(r))][[0, 1, 3, 15]], r.max())


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_the_bounds_notice_a_wrong_interpreter(expr, mutant):
    """Each mutation of the interpreter's mirror fails at least one case of the tables, in every format that can see it."""
    for fmt in FMTS:
        caught = [c.name for c in all_cases(fmt) if c.op == MUTANTS[mutant] and c.ratios(mirror(expr, c.text, c.X, fmt, mutant)).max() > 1.0]
        if (mutant, fmt) in UNDETECTED:
            assert not caught, (mutant, fmt, "is detected: take it out of UNDETECTED")
            continue
        assert caught, (mutant, fmt)
    assert any((mutant, f) not in UNDETECTED for f in FMTS)


def test_the_undetected_mutant_shows_at_its_named_size(expr):
    F = er.F32
    x = np.float32(UNDETECTED[("tanh_small", "f32")]) * np.float32(0.99)
    c = er.Case("TANH", "tanh at the named size", "tanh(x0)", er._rows(F, x0=[x, -x]), "f32")
    assert c.ratios(c.X[:, 0]).max() > 1.0 and c.ratios(c.numpy).max() <= 1.0


# ---- compiler facts ------------------------------------------------------------------------------------------------------------
def test_every_program_is_a_valid_int32_array(expr):
    """(arg << 8) | opcode as a SIGNED int32: what Engine.set_model / eval_expression hand to the C ABI."""
    texts = er.all_texts()
    assert any("**(-" in t for t in texts)
    for t in texts:
        prog = expr.compile_expression(t, [])
        code = np.asarray(prog.code, dtype=np.int32)
        assert code.dtype == np.int32 and len(code) <= er.MAX_CODE and prog.max_stack <= er.MAX_STACK, t
        assert all(-(1 << 31) <= w < (1 << 31) for w in prog.code), t
        for w in code.tolist():                                                  # the device's decode: arithmetic shift
            op, arg = w & 0xFF, w >> 8
            assert 0 <= op < 19
            if op != expr.OP["POWI"]:
                assert 0 <= arg < 256, t


@pytest.mark.parametrize("e", [0, 1, 3, 5, 30, -1, -2, -3, -7, (1 << 22) - 1, -((1 << 22) - 1)])
def test_powi_exponent_round_trips(expr, e):
    for text in ("x0**(%d)" % e, "x0^(%d)" % e, "x0**(%d.0)" % e):
        prog = expr.compile_expression(text, [])
        word = int(np.asarray(prog.code, dtype=np.int32)[-1])
        assert word & 0xFF == expr.OP["POWI"]
        arg = word >> 8
        assert (arg - (1 << 24) if arg >= (1 << 23) else arg) == e                 # interp_eval / bytecode_to_cxx
        assert expr.disassemble(prog, []).splitlines()[-1] == "POWI %d" % e


def test_the_power_forms(expr):
    last = lambda t: expr.disassemble(expr.compile_expression(t, []), [0.0] * 4).splitlines()[-1]
    assert last("x0**2") == "SQUARE" and last("x0^2") == "SQUARE"
    assert last("x0**4194303") == "POWI 4194303" and last("x0**-4194303") == "POWI -4194303"
    assert last("x0**4194304") == "POW" and last("x0**-4194304") == "POW" and last("x0**4194304.0") == "POW"
    assert last("x0**2.5") == "POW" and last("x0**x1") == "POW" and last("pow(x0, 3)") == "POW"
    assert expr.compile_expression("x0 ^ 3 + x1", []).code == expr.compile_expression("x0 ** 3 + x1", []).code


def test_limits_are_exact(expr):
    assert expr.compile_expression(er.deep_expression(16), []).max_stack == 16
    assert len(expr.compile_expression(er.long_expression(256), []).code) == 256
    with pytest.raises(expr.ExpressionError):
        expr.compile_expression(er.deep_expression(17), [])
    with pytest.raises(expr.ExpressionError):
        expr.compile_expression(er.long_expression(257), [])


def test_composites_have_the_structure_they_are_chosen_for():
    """More distinct hoistable subtrees than the generator's lists hold, and every heavy opcode in each dependency class."""
    assert er.OVERFLOW_THETA.count("exp(") > er.MAX_SUBS and sum(er.OVERFLOW_THETA.count(f) for f in ("tanh(x17", "sqrt(x17", "log(x17")) > er.MAX_GSUBS
    for op in er.HEAVY:
        t = er.composite_theta(op)
        assert all(s in t for s in ("x3 + x4", "x17", "x15 + x4", "x16"))
