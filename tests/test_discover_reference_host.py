"""The reference of rovmpc_discover_rows (tests/discover_reference.py) checked against itself on the CPU: the NumPy restatement
of stage 2 against an independent selection by np.linalg.lstsq and against the exact solve at 50 digits, the decided picks of
fixture A, the measured constant, the degenerate libraries, and three deliberately wrong laws that the checks must reject.
These tests validate the reference alone: they need no library and pass without the feature."""
import os
import sys

import mpmath as mp
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import discover_reference as dr  # noqa: E402


def cases_ab():
    out = [(c, 0) for c in dr.fixture_a().values()]
    for c in dr.fixture_b().values():
        out += [(c, g) for g in range(len(c.group_ranges()))]
    return out


@pytest.fixture(scope="module")
def fronts():
    """Per (case, group): select_np on the correctly rounded exact Gram, the exact Gram, the columns and the decided steps."""
    out = {}
    for case, g in cases_ab():
        res, grams, V = dr.reference_front(case, g)
        picks = [int(p) for p in res["picks"][:res["n_sel"]]]
        out[(case.name, g)] = (case, res, grams, V, dr.decided_steps(grams[0], grams[1], len(case.terms), picks, len(V)))
    return out


def decided_prefix(decided):
    """The steps before the first undecided one: after it the two selections may hold different sets."""
    k = 0
    while k < len(decided) and decided[k][0]:
        k += 1
    return k


def test_select_np_picks_what_lstsq_picks_on_every_decided_step(fronts):
    seen = 0
    for (name, g), (case, res, grams, V, decided) in fronts.items():
        k = decided_prefix(decided)
        assert dr.greedy_lstsq(V, k) == [int(p) for p in res["picks"][:k]], (name, g)
        seen += k
    assert seen >= 40


def test_fixture_a_is_decided_up_to_the_reference_rows(fronts):
    """Every step of the theta front up to size 4 and of the gamma front up to size 2, at both noise levels, and the terms are
    the reference's; at noise 0 the front ends there on the relative stop rule."""
    for (name, noise), case in dr.fixture_a().items():
        _, res, grams, V, decided = fronts[(case.name, 0)]
        k = dr.A_SIZES[name]
        assert res["n_sel"] >= k
        for s in range(k):
            ok, gap, bound = decided[s]
            print("%s step %d: gap %.3g bound %.3g" % (case.name, s, gap, bound))
            assert ok and gap > bound, (case.name, s, gap, bound)
        assert {case.terms[int(p)] for p in res["picks"][:k]} == set(dr.A_EXPECT[name])
        if noise == 0.0:
            assert res["n_sel"] == k and res["status"] == dr.MIN_GAIN
    assert min(fronts[(c.name, 0)][4][s][1] for (nm, _), c in dr.fixture_a().items() for s in range(dr.A_SIZES[nm])) > 2e-3


def test_coefficients_and_losses_within_the_bound_of_the_exact_solve(fronts):
    worst_a = worst_f = 0.0
    for (name, g), (case, res, (hi, lo, _), V, _) in fronts.items():
        n, M = len(V), len(case.terms)
        eps = dr.eps_total(n)
        for s in range(res["n_sel"]):
            picked = [int(p) for p in res["picks"][:s + 1]]
            st = dr.exact_state(hi, lo, M, picked)
            with mp.workdps(dr.DPS):
                for i, b in enumerate(dr.coef_bounds(st, picked, eps)):
                    r = float(abs(mp.mpf(float(res["coef"][s, i])) - st["a"][i])) / b
                    worst_a = max(worst_a, r)
                    assert r <= 1, (name, g, s, i, r)
                exact_loss = max(st["F"], 0) / n
                r = float(abs(mp.mpf(float(res["loss"][s + 1])) - exact_loss)) / (dr.f_bound(st, picked, eps) / n + dr.U * float(exact_loss))
                worst_f = max(worst_f, r)
                assert r <= 1, (name, g, s, r)
    print("largest error / bound: coefficients %.3g, losses %.3g" % (worst_a, worst_f))


def test_recovered_coefficients_of_fixture_a(fronts):
    for (name, noise), case in dr.fixture_a().items():
        _, res, (hi, lo, _), V, _ = fronts[(case.name, 0)]
        k = dr.A_SIZES[name]
        picked = [int(p) for p in res["picks"][:k]]
        st = dr.exact_state(hi, lo, len(case.terms), picked)
        bounds = dr.coef_bounds(st, picked, dr.eps_total(len(V)))
        e = np.linalg.norm(case.target[0] - dr.fixture_a()[(name, 0.0)].target[0])
        for i, p in enumerate(picked):
            want = dr.A_EXPECT[name][case.terms[p]]
            # noise e moves the least-squares solution itself: a = pinv(Phi) g, |pinv(Phi D^-1)| = 1 / sqrt(lmin), so by at most
            # |e| / sqrt(G_ii lmin); 1e-8 relative: the digits the reference's file gives its constant
            slack = e / np.sqrt(float(st["diag"][p]) * st["lmin"]) + 1e-8 * abs(want)
            assert abs(res["coef"][k - 1, i] - want) <= bounds[i] + slack, (case.name, case.terms[p])


def test_measured_constant_is_what_the_module_records():
    worst, where = 0.0, ""
    for case, g in cases_ab():
        k, at = dr.measure_k((case.columns(g), len(case.terms), case.max_terms))
        if k > worst:
            worst, where = k, "%s group %d, %s" % (case.name, g, at)
    print("K measured %.4g at %s (recorded %.4g)" % (worst, where, dr.MEASURED_K))
    assert dr.MEASURED_K / 2 <= worst <= dr.MEASURED_K


def test_degenerate_libraries():
    c = dr.fixture_c()
    res, grams, V = dr.reference_front(c["duplicate"])
    picks = [int(p) for p in res["picks"][:res["n_sel"]]]
    assert not (0 in picks and 2 in picks) and 0 in picks and res["status"] == dr.EXHAUSTED and res["n_sel"] == 3
    # the twin's residual is a rounding of its own square sum: far below dep_tol
    st = dr.exact_state(grams[0], grams[1], 4, [0])
    assert float(st["rho"][2] / st["diag"][2]) < 1e-20
    res, _, _ = dr.reference_front(c["zero_term"])
    assert 1 not in res["picks"] and res["n_sel"] == 2 and res["status"] == dr.EXHAUSTED
    with_log, _, V = dr.reference_front(c["with_log"])
    without, _, _ = dr.reference_front(c["without_log"])
    assert np.isnan(V[:, 1]).any() and 1 not in with_log["picks"]
    remap = {0: 0, 2: 1, 3: 2, -1: -1}
    assert [remap[int(p)] for p in with_log["picks"]] == [int(p) for p in without["picks"]]
    assert dr.same(with_log["coef"], without["coef"]) and dr.same(with_log["loss"], without["loss"]) and with_log["status"] == without["status"]
    res, _, _ = dr.reference_front(c["nan_target"])
    assert res["status"] == dr.NONFINITE and res["n_sel"] == 0 and np.isnan(res["loss"]).all() and (res["picks"] == -1).all()
    res, _, _ = dr.reference_front(c["zero_target"])
    assert res["status"] == dr.MIN_GAIN and res["n_sel"] == 0 and res["loss"][0] == 0.0 and np.isnan(res["loss"][1:]).all()
    res, _, _ = dr.reference_front(c["few_terms"])
    assert res["status"] == dr.EXHAUSTED and res["n_sel"] == 2


def test_three_broken_laws_are_rejected(fronts):
    """gain without the division by rho: the picks leave lstsq's on a decided step; no dependence test: a term and its near twin
    are both picked;
    ties to the highest index: the second twin is picked where the law picks the first."""
    wrong = 0
    for (name, g), (case, res, grams, V, decided) in fronts.items():
        k = decided_prefix(decided)
        bad = dr.select_np(grams[0], len(case.terms), len(V), max_terms=case.max_terms, mutant="no_division")
        wrong += [int(p) for p in bad["picks"][:k]] != dr.greedy_lstsq(V, k)
    assert wrong >= 3
    near = dr.fixture_c()["near_twin"]                                         # x0 and x0 + 1e-9 x5: rho / G = 1e-18 after x0
    V = near.columns()
    hi = dr.gram_exact(V)[0]
    good, bad = dr.select_np(hi, 4, len(V)), dr.select_np(hi, 4, len(V), mutant="no_dep_test")
    assert [int(p) for p in good["picks"][:3]] == [0, 1, 3] and good["n_sel"] == 3 and good["status"] == dr.EXHAUSTED
    assert 0 in bad["picks"] and 2 in bad["picks"]
    V = dr.fixture_c()["duplicate"].columns()
    hi = dr.gram_exact(V)[0]
    good = dr.select_np(hi, 4, len(V))
    assert good["steps"][0][0] == good["steps"][0][2] == np.nanmax(good["steps"][0])     # an exact tie between the twins, the largest gain
    assert int(good["picks"][0]) == 0 and 2 not in good["picks"]
    assert int(dr.select_np(hi, 4, len(V), mutant="ties_high")["picks"][0]) == 2
