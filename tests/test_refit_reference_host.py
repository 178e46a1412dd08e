"""The references of rovmpc_refit_rows on the CPU (tests/refit_reference.py): the NumPy restatement of the law against the
50-digit minimisers, the records of those minimisers, expr.rewrite_constants on every shipped row, and what scoring.refit_rows
refuses before it reaches the library."""
import json
import os
import sys

import mpmath as mp
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refit_reference as rr  # noqa: E402

sys.path.insert(0, rr.ROOT)
import rovmpc  # noqa: E402
from rovmpc import expr  # noqa: E402

from rovmpc.model import DATA_DIR as DATA  # noqa: E402


@pytest.fixture(scope="module")
def numpy_fits():
    return {p.name: rr.refit_np(p.text, p.recs, p.c0, p.free) for p in rr.all_problems()}


# ---- the NumPy restatement -------------------------------------------------------------------------------------------------------
def test_every_fit_of_fixture_a_converges_within_16_trial_steps(numpy_fits):
    probs = rr.fixture_a()
    assert len(probs) == 36
    for p in probs:
        o = numpy_fits[p.name]
        code, consts = rr.compile_row(p.text)
        F_true = rr.sums_np(code, p.c_true, rr.free_indices(code, consts), p.recs)[0]
        assert o["status"] == rr.CONVERGED and o["iters"] <= 16, (p.name, o["status"], o["iters"])
        assert o["loss"] <= o["loss0"] and o["loss"] <= F_true / len(p.recs[0][1]), p.name


def test_numpy_against_50_digits(numpy_fits):
    """Measures M and M_c of the module text of refit_reference and holds the recorded values to them."""
    M, Mc, where, n_cmp = 0.0, 0.0, (None, None), 0
    for p in rr.all_problems():
        o, rec = numpy_fits[p.name], rr.minimisers()[p.name]
        if o["status"] != rr.CONVERGED or rec["P"] == 0 or not rec["orth"] <= rr.REF_ORTH:
            continue
        n_cmp += 1
        _, derived, E = rr.loss_bound(rec, M=0.0)
        with mp.workdps(rr.DPS):
            excess = float(mp.mpf(o["loss"]) - mp.mpf(rec["F"]) / rec["n"])
            dc = [float(abs(mp.mpf(float(o["consts"][k])) - rr.star_consts(rec)[k])) for k in rec["free_idx"]]
        if E > 0 and np.isfinite(derived) and (excess - derived) / E > M:
            M, where = (excess - derived) / E, (p.name, where[1])
        for d, (_, dj, Ej) in zip(dc, rr.const_bounds(rec, Mc=0.0) if p.name.startswith("B/") else []):
            if np.isfinite(Ej) and Ej > 0 and (d - dj) / Ej > Mc:
                Mc, where = (d - dj) / Ej, (where[0], p.name)
    print("NumPy against 50 digits on %d converged problems: M = %.3g, M_c = %.3g at %s" % (n_cmp, M, Mc, where))
    assert n_cmp >= 45
    assert M <= rr.MEASURED_M <= 2 * M and Mc <= rr.MEASURED_MC <= 2 * Mc, (M, Mc)


def test_numpy_losses_and_constants_are_within_the_bound(numpy_fits):
    for p in rr.all_problems():
        o, rec = numpy_fits[p.name], rr.minimisers()[p.name]
        if o["status"] != rr.CONVERGED or rec["P"] == 0 or not rec["orth"] <= rr.REF_ORTH:
            continue
        assert o["loss"] <= rr.loss_bound(rec)[0], p.name
        with mp.workdps(rr.DPS):
            for k, (b, _, _) in zip(rec["free_idx"], rr.const_bounds(rec) if p.name.startswith("B/") else []):
                assert float(abs(mp.mpf(float(o["consts"][k])) - rr.star_consts(rec)[k])) <= b, (p.name, k)


# ---- the records ------------------------------------------------------------------------------------------------------------------
def test_every_record_is_stationary_at_50_digits():
    recs = rr.minimisers()
    probs = rr.all_problems()
    assert sorted(recs) == sorted(p.name for p in probs)
    for p in probs:
        rec = recs[p.name]
        code, consts = rr.compile_row(p.text)
        idx = rr.free_indices(code, consts, p.free)
        assert idx == rec["free_idx"] and rec["P"] == len(idx)
        with mp.workdps(rr.DPS):
            F, A, g, ok, p2 = rr.sums_mp(code, rr.star_consts(rec), idx, p.recs)
            # (c* is kept to 40 digits: the values move by some 1e-38 |p|, and F by 2 |r| times that)
            assert ok and abs(F - mp.mpf(rec["F"])) <= mp.mpf("1e-36") * (2 * mp.sqrt(F * p2) + F) + mp.mpf("1e-70"), p.name
            if rec["orth"] <= rr.REF_ORTH:
                # the orthogonality test with room for the 40 digits of the record: a residual of 1e-35 |p| cannot be told from 0
                for j in range(len(idx)):
                    if A[j][j] > 0:
                        assert abs(g[j]) / mp.sqrt(A[j][j]) <= rr.REF_ORTH * mp.sqrt(F) + mp.mpf("1e-35") * mp.sqrt(p2), (p.name, j)


def test_a_sample_of_records_is_recomputed_from_the_start():
    by_name = {p.name: p for p in rr.all_problems()}
    for name in ("A/dtheta_dt[3]", "A/dgamma_dt[11]", "B/frozen_sine"):
        assert rr.record_of(by_name[name]) == rr.minimisers()[name], name


# ---- expr.rewrite_constants --------------------------------------------------------------------------------------------------------
def _shipped_rows():
    out = []
    for gen in ("gen1", "gen2", "gen3"):
        eqs = json.load(open(os.path.join(DATA, "%s_equations.json" % gen)))
        names = eqs.get("variable_names")
        for key, front in eqs.items():
            if isinstance(front, dict) and "rows" in front:
                for row in front["rows"]:
                    for col in ("sympy_format", "equation"):
                        if row.get(col):
                            out.append((gen, row[col], names))
    return out


def _resolved(code, consts):
    """The program with every PUSH_C carrying its value's bits: two programs evaluate alike when these are equal."""
    return [("C", np.float64(consts[ins >> 8]).tobytes()) if ins & 0xFF == expr.OP["PUSH_C"] else ins for ins in code]


def test_rewrite_constants_round_trip_on_every_shipped_row():
    rows = _shipped_rows()
    assert len(rows) > 100
    rng = np.random.default_rng(11)
    most = 0
    for gen, text, names in rows:
        F = 32
        consts = []
        prog = expr.compile_expression(text, consts, F, names)
        most = max(most, len(consts))
        same = expr.rewrite_constants(text, consts, names)
        c2 = []
        assert _resolved(expr.compile_expression(same, c2, F, names).code, c2) == _resolved(prog.code, consts), text
        new = [float(c) * float(rng.uniform(0.5, 1.5)) * float(rng.choice([-1.0, 1.0])) + float(rng.normal()) * 1e-3 for c in consts]
        if new:
            new[0] = -0.0 if len(new) % 2 else 1e300
        from rovmpc.scoring import exponent_roles
        for k, (n_exp, _) in enumerate(exponent_roles(prog.code, len(consts))):
            if n_exp:
                new[k] = consts[k]                  # an exponent keeps its value: an integer one would compile to POWI
        text2 = expr.rewrite_constants(text, new, names)
        c3 = []
        assert _resolved(expr.compile_expression(text2, c3, F, names).code, c3) == _resolved(prog.code, new), (text, text2)
    assert most <= 7
    with pytest.raises(expr.ExpressionError):
        expr.rewrite_constants("0.5*x0 + 2.5", [1.0])
    with pytest.raises(expr.ExpressionError):
        expr.rewrite_constants("0.5*x0", [float("nan")])
    assert expr.rewrite_constants("x0**2 + x1**(-3) + 2*x2", [7.0]) == "x0 ** 2 + x1 ** (-3) + 7.0 * x2"
    assert expr.rewrite_constants("0.5**x0 - -0.25", [-1.5, 1e999]) == "(-1.5) ** x0 - 1e309"


# ---- what scoring.refit_rows refuses before the library ---------------------------------------------------------------------------
def test_python_refusals():
    X, g = np.zeros((2, 5, 18)), np.zeros((2, 5))
    ok = dict(rows=["0.5*x3 + 1.5"], X=X, target=g)
    bad = [dict(rows=[]), dict(rows="0.5*x3"), dict(target=None), dict(target=np.zeros((2, 4))), dict(X=np.zeros(5)),
           dict(lengths=[5, 0]), dict(lengths=[5, 6]), dict(groups="some"), dict(groups=[0, 1]), dict(groups=[0, 2, 2]), dict(groups=[1, 2]),
           dict(groups=[0.0, 2.0]), dict(free=[[True]]), dict(free=[[True, True], [True]]), dict(max_iter=0), dict(max_iter=1001),
           dict(max_iter=2.5), dict(gtol=-1.0), dict(xtol=float("nan")),
           dict(rows=[" + ".join("%d.5*x%d" % (k + 1, k) for k in range(9))]),                  # nine free constants
           dict(rows=["x3**2.5 + 2.5*x4"])]                                                      # 2.5: an exponent and a factor
    for change in bad:
        with pytest.raises(ValueError):
            rovmpc.refit_rows(**dict(ok, **change))
    from rovmpc.scoring import default_free
    code, consts = rr.compile_row("1.5*x3**2.5 + x4**0.5")
    assert list(default_free(code, len(consts))) == [1, 0, 0]
    assert [s.name for s in rovmpc.RefitStatus] == ["CONVERGED", "MAX_ITER", "STALLED", "NONFINITE", "NO_PARAMS"]
