"""rovmpc_discover_rows / rovmpc_discover_rows_device on the GPU (law in include/rovmpc.h) on the fixtures of
tests/discover_reference.py: the Gram against the exact Gram of the device's own term values, the selection bit for bit
against the NumPy restatement on the returned Gram, the recovery of the reference's rows, independence to the bit, the loss
against rovmpc_score_rows within the derived bound, the front through refit_rows and select_model, and the refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import discover_reference as dr  # noqa: E402
import score_reference as sr  # noqa: E402
from score_reference import same  # noqa: E402
from plan_controller_helpers import rv  # noqa: E402,F401

pytestmark = pytest.mark.gpu


def discover(rv, case, **kw):
    kw = dict(dict(lengths=case.lengths, groups=case.groups, max_terms=case.max_terms, return_gram=True), **kw)
    return rv.discover_rows(case.terms, case.X, case.target, **kw)


def device_values(rv, case):
    """(M, B, T): every term on every row as the device evaluates it (the `pred` of rovmpc_score_rows)."""
    zeros = np.zeros(case.target.shape)
    return rv.score_rows(case.terms, case.X, zeros, zeros, integrator="euler", lengths=case.lengths, return_pred=True).pred


@pytest.fixture(scope="module")
def runs(rv):
    """name -> (case, front) for every case of A, B and C, each run once through the host entry."""
    cases = list(dr.fixture_a().values()) + list(dr.fixture_b().values()) + list(dr.fixture_c().values())
    return {c.name: (c, discover(rv, c)) for c in cases}


@pytest.fixture(scope="module")
def exact(rv, runs):
    """(case name, group) -> (V, (hi, lo, absum)): the device's own term values and their exact Gram, on A and B."""
    out = {}
    for case in list(dr.fixture_a().values()) + list(dr.fixture_b().values()):
        vals = device_values(rv, case)
        for g in range(len(case.group_ranges())):
            V = case.columns(g, term_values=vals)
            out[(case.name, g)] = (V, dr.gram_exact(V))
    return out


# ---- 1. the Gram -------------------------------------------------------------------------------------------------------------
def test_gram_within_the_bound_of_the_exact_gram(runs, exact):
    worst = 0.0
    for (name, g), (V, (hi, lo, ab)) in exact.items():
        case, front = runs[name]
        assert front.n[g] == len(V) and front.gram.shape == (len(case.group_ranges()), (len(case.terms) + 1) * (len(case.terms) + 2) // 2)
        got = front.gram[g]
        n = len(V)
        err = np.abs((got - hi) - lo)
        with np.errstate(all="ignore"):
            ratio = np.where(err == 0, 0.0, err / (dr._gamma(n + 1) * ab))
        print("%s group %d: n = %d, largest |G^ - G| / (gamma_{n+1} sum |v_j v_k|) = %.3g" % (name, g, n, ratio.max()))
        worst = max(worst, float(ratio.max()))
        assert ratio.max() <= 1, (name, g)
    print("largest ratio over A and B: %.3g" % worst)


# ---- 2. the selection --------------------------------------------------------------------------------------------------------
def test_selection_is_the_numpy_restatement_on_the_returned_gram_bit_for_bit(runs):
    for name, (case, front) in runs.items():
        M = len(case.terms)
        for g in range(len(case.group_ranges())):
            ref = dr.select_np(front.gram[g], M, int(front.n[g]), max_terms=case.max_terms)
            assert front.n_sel[g] == ref["n_sel"] and front.status[g] == ref["status"], (name, g, front.n_sel[g], front.status[g], ref["n_sel"], ref["status"])
            assert np.array_equal(front.picks[g], ref["picks"]), (name, g, front.picks[g], ref["picks"])
            assert same(front.coef[g], ref["coef"]) and same(front.loss[g], ref["loss"]), (name, g)
            assert len(front.expressions[g]) == ref["n_sel"]


def test_degenerate_libraries(runs):
    S = dr.FULL, dr.MIN_GAIN, dr.EXHAUSTED, dr.NONFINITE
    front = runs["C/duplicate"][1]
    picks = list(front.picks[0][:front.n_sel[0]])
    assert 0 in picks and 2 not in picks and front.n_sel[0] == 3 and front.status[0] == S[2]
    front = runs["C/near_twin"][1]
    assert list(front.picks[0][:3]) == [0, 1, 3] and front.n_sel[0] == 3 and front.status[0] == S[2]
    front = runs["C/zero_term"][1]
    assert 1 not in front.picks[0] and front.n_sel[0] == 2 and front.status[0] == S[2]
    a, b = runs["C/with_log"][1], runs["C/without_log"][1]
    remap = {0: 0, 2: 1, 3: 2, -1: -1}
    assert [remap[int(p)] for p in a.picks[0]] == [int(p) for p in b.picks[0]] and 1 not in a.picks[0]
    assert same(a.coef, b.coef) and same(a.loss, b.loss) and a.status[0] == b.status[0] and a.n_sel[0] == b.n_sel[0] == 3
    front = runs["C/nan_target"][1]
    assert front.status[0] == S[3] and front.n_sel[0] == 0 and np.isnan(front.loss).all() and (front.picks == -1).all() and (front.coef == 0).all()
    assert front.expressions == [[]] and front.rows() == []
    front = runs["C/zero_target"][1]
    assert front.status[0] == S[1] and front.n_sel[0] == 0 and front.loss[0, 0] == 0.0 and np.isnan(front.loss[0, 1:]).all()
    front = runs["C/few_terms"][1]
    assert front.status[0] == S[2] and front.n_sel[0] == 2 and (front.picks[0, 2:] == -1).all() and (front.coef[0, 2:] == 0).all()
    front = runs["B/one"][1]
    assert front.n_sel[0] == 1 and front.status[0] == S[2] and front.coef[0, 0, 0] == 1.5 and front.loss[0, 0] == 9.0 and front.loss[0, 1] == 0.0


# ---- 3. recovery -------------------------------------------------------------------------------------------------------------
def test_the_reference_rows_are_recovered_on_fixture_a(runs, exact):
    for (name, noise), case in dr.fixture_a().items():
        front = runs[case.name][1]
        k = dr.A_SIZES[name]
        picked = [int(p) for p in front.picks[0][:k]]
        assert {case.terms[p] for p in picked} == set(dr.A_EXPECT[name]), (case.name, picked)
        V, (hi, lo, _) = exact[(case.name, 0)]
        st = dr.exact_state(hi, lo, len(case.terms), picked)
        bounds = dr.coef_bounds(st, picked, dr.eps_total(len(V)))
        e = np.linalg.norm(case.target[0] - dr.fixture_a()[(name, 0.0)].target[0])
        for i, p in enumerate(picked):
            want = dr.A_EXPECT[name][case.terms[p]]
            slack = e / np.sqrt(float(st["diag"][p]) * st["lmin"]) + 1e-8 * abs(want)         # (test_discover_reference_host derives it)
            got = front.coef[0, k - 1, i]
            print("%s %s: %.17g (want %.9g, bound %.3g + %.3g)" % (case.name, case.terms[p], got, want, bounds[i], slack))
            assert abs(got - want) <= bounds[i] + slack, (case.name, case.terms[p], got)
        if noise == 0.0:
            assert front.n_sel[0] == k and front.status[0] == dr.MIN_GAIN, (case.name, front.n_sel, front.status)


# ---- 4. independence, to the bit ------------------------------------------------------------------------------------------------
def front_bits(front, g):
    return front.picks[g], front.coef[g], front.loss[g], front.n_sel[g], front.status[g], front.n[g], front.gram[g]


def same_front(a, ga, b, gb):
    return all(same(x, y) for x, y in zip(front_bits(a, ga), front_bits(b, gb)))


def test_a_group_does_not_feel_the_rest_of_the_call(rv, runs):
    case, each = runs["B/ragged_each"]
    B = len(case.X)
    for b in range(B):
        n = int(case.lengths[b])
        alone = dr.Case("alone", case.terms, case.X[b:b + 1], case.target[b:b + 1], case.lengths[b:b + 1])
        assert same_front(discover(rv, alone), 0, each, b), b
        trimmed = dr.Case("trimmed", case.terms, case.X[b:b + 1, :n], case.target[b:b + 1, :n])          # another T, no lengths
        assert same_front(discover(rv, trimmed), 0, each, b), b
    order = [2, 0, 1]
    moved = dr.Case("moved", case.terms, case.X[order], case.target[order], case.lengths[order], "each")
    front = discover(rv, moved)
    for g, b in enumerate(order):
        assert same_front(front, g, each, b), (g, b)
    # the groups of "offsets" are recordings (0, 1) and (2): the second is recording 2 alone, the first a pooled pair
    off = runs["B/ragged_offsets"][1]
    assert same_front(off, 1, each, 2)
    pair = dr.Case("pair", case.terms, case.X[:2], case.target[:2], case.lengths[:2])
    assert same_front(discover(rv, pair), 0, off, 0)


def test_the_device_entry_gives_the_host_entry_bits(rv, runs):
    for name in ("B/M64", "B/ragged_offsets", "B/one", "A/theta/noise0.001", "C/with_log"):
        case, host = runs[name]
        dev = discover(rv, case, device=True)
        for g in range(len(case.group_ranges())):
            assert same_front(dev, g, host, g), (name, g)
        assert dev.expressions == host.expressions
    nogram = discover(rv, runs["B/M64"][0], return_gram=False)
    assert nogram.gram is None and same(nogram.coef, runs["B/M64"][1].coef)


def test_a_terms_place_in_the_library_does_not_matter_without_ties(rv, runs):
    case, front = runs["B/M64"]
    M = len(case.terms)
    perm = np.random.default_rng(11).permutation(M)                           # new place k holds old term perm[k]
    moved = dr.Case("permuted", [case.terms[p] for p in perm], case.X, case.target)
    got = discover(rv, moved)
    assert [int(perm[p]) for p in got.picks[0]] == [int(p) for p in front.picks[0]]
    assert same(got.coef, front.coef) and same(got.loss, front.loss) and got.status[0] == front.status[0]
    for s in range(int(front.n_sel[0])):                                      # (no ties: the gains of every step are distinct)
        gains = dr.select_np(front.gram[0], M, int(front.n[0]))["steps"][s]
        gains = gains[gains == gains]
        assert len(set(gains.tolist())) == len(gains)


def test_smaller_fronts_are_prefixes(rv, runs):
    case, front = runs["B/M64"]
    for S in (1, 3):
        small = discover(rv, case, max_terms=S)
        assert small.picks.shape == (1, S) and small.coef.shape == (1, S, S) and small.loss.shape == (1, S + 1)
        assert np.array_equal(small.picks[0], front.picks[0, :S]) and same(small.coef[0], front.coef[0, :S, :S]) and same(small.loss[0], front.loss[0, :S + 1])
        assert small.status[0] == dr.FULL


# ---- 5. the loss -------------------------------------------------------------------------------------------------------------
def test_loss_is_the_scores_loss_within_the_derived_bound(rv, runs, exact):
    worst = 0.0
    for (name, g), (V, (hi, lo, _)) in exact.items():
        case, front = runs[name]
        k_sel = int(front.n_sel[g])
        if k_sel == 0:
            continue
        b0, b1 = case.group_ranges()[g]
        X, target = case.X[b0:b1], case.target[b0:b1]
        lens = None if case.lengths is None else case.lengths[b0:b1]
        zeros = np.zeros(target.shape)
        scored = rv.score_rows(front.rows(g), X, zeros, zeros, integrator="euler", target=target, lengths=lens).loss       # (sizes, recordings)
        nb = np.full(b1 - b0, X.shape[1]) if lens is None else lens
        n = int(nb.sum())
        pooled = (scored * nb).sum(axis=1) / n
        for s in range(k_sel):
            picked = [int(p) for p in front.picks[g][:s + 1]]
            st = dr.exact_state(hi, lo, len(case.terms), picked)
            bound = dr.loss_bound(st, picked, n) + dr._gamma(len(nb) + 3) * pooled[s]      # (the pooling here: B products, quotients, sums)
            r = abs(front.loss[g, s + 1] - pooled[s]) / bound
            worst = max(worst, r)
            assert r <= 1, (name, g, s, front.loss[g, s + 1], pooled[s], bound)
    print("largest |front loss - score loss| / bound: %.3g" % worst)


# ---- 6. downstream -----------------------------------------------------------------------------------------------------------
def test_the_front_goes_through_refit_and_select_model(rv, runs, scaler):
    fronts = {}
    for name in ("theta", "gamma"):
        case, front = runs[dr.fixture_a()[(name, 1e-3)].name]
        rows = front.rows()
        assert len(rows) == front.n_sel[0] >= dr.A_SIZES[name]
        fit = rv.refit_rows(rows, case.X, case.target)
        print(name, "refit status", fit.status[:, 0], "loss0", fit.loss0[:, 0], "loss", fit.loss[:, 0])
        assert (fit.status[:, 0] == rv.RefitStatus.CONVERGED).all(), fit.status[:, 0]
        assert (fit.loss[:, 0] <= fit.loss0[:, 0]).all()
        fronts[name] = rows
    mean, scale = scaler
    a = sr.fixture_a()
    rt, rg = a["theta"][1], a["gamma"][1]
    model, s_th, s_ga = rv.select_model(fronts["theta"], fronts["gamma"], rt.X * scale + mean, rt.time, rt.truth, rg.truth, mean, scale)
    assert model.expr_theta in [r["equation"] for r in fronts["theta"]] and model.expr_gamma in [r["equation"] for r in fronts["gamma"]]
    assert s_th.r2.shape == (len(fronts["theta"]), 1) and s_ga.r2.shape == (len(fronts["gamma"]), 1)
    sk = rv.score_pairs(fronts["theta"][:2], fronts["gamma"][:2], rt.X, rt.time, rt.truth, rg.truth, mean, scale, horizon=5)
    assert sk.skill.shape == (4, 1, 5)


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_anything_is_launched(rv):
    from rovmpc import _lib
    from rovmpc.engine import _ptr
    from rovmpc.expr import OP
    PUSH_F, PUSH_C, ADD = (OP[n] for n in ("PUSH_F", "PUSH_C", "ADD"))
    T, B, F, G, S = 6, 2, 4, 2, 8
    X = np.random.default_rng(3).standard_normal((B, T, F))
    good = dict(code=np.array([PUSH_F, (0 << 8) | PUSH_C, ADD, (1 << 8) | PUSH_F], np.int32), code_off=np.array([0, 3, 4], np.int32),
                consts=np.array([0.5]), const_off=np.array([0, 1, 1], np.int32), M=2, X=X, F=F, len=np.array([T, 3], np.int64), T=T, B=B,
                target=X[..., 1] + 1.0, group_off=np.array([0, 1, 2], np.int32), G=G, params=_lib.DiscoverParams.make())
    e = rv.default_engine()
    order = ("code", "code_off", "consts", "const_off", "M", "X", "F", "len", "T", "B", "target", "group_off", "G", "params")
    outs = ("picks", "coef", "loss", "info", "gram")

    def call(entry="rovmpc_discover_rows", **change):
        a = dict(good, **change)
        bufs = dict(picks=np.full(64, -7, np.int32), coef=np.full(1024, -7.0), loss=np.full(64, -7.0), info=np.full(16, -7, np.int64),
                    gram=np.full(64, -7.0))
        args = [_ptr(a[k]) if isinstance(a[k], np.ndarray) or a[k] is None else (C.byref(a[k]) if k == "params" else a[k]) for k in order]
        rc = getattr(e.lib, entry)(e._h, *args, *[None if k in change and change[k] is None else _ptr(bufs[k]) for k in outs])
        return rc, e.lib.rovmpc_last_error(e._h).decode(), bufs

    rc, _, bufs = call()
    assert rc == 0 and list(bufs["info"][:6]) == [2, dr.EXHAUSTED, T, 2, dr.EXHAUSTED, 3] and (bufs["picks"][G * S:] == -7).all()
    assert not (bufs["loss"][:G * (S + 1)] == -7.0).any() and (bufs["loss"][G * (S + 1):] == -7.0).all() and not (bufs["gram"][:12] == -7.0).any()
    rc, _, bufs = call(gram=None, params=None)
    assert rc == 0 and (bufs["gram"] == -7.0).all() and bufs["info"][0] == 2

    def p(**kw):
        q = _lib.DiscoverParams.make()
        for k, v in kw.items():
            setattr(q, k, v)
        return q
    big = 65
    bad = [dict(M=0), dict(M=big, code=np.full(big, (1 << 8) | PUSH_F, np.int32), code_off=np.arange(big + 1, dtype=np.int32), const_off=np.zeros(big + 1, np.int32)),
           dict(B=0), dict(T=0), dict(len=np.array([T, 0], np.int64)), dict(len=np.array([T + 1, 1], np.int64)), dict(F=0),
           dict(F=_lib.MAX_FEATURES + 1), dict(code_off=np.array([0, 4, 3], np.int32)), dict(const_off=np.array([0, 1, 0], np.int32)),
           dict(code_off=np.array([1, 3, 4], np.int32)), dict(code=None), dict(code_off=None), dict(consts=None), dict(const_off=None),
           dict(X=None), dict(target=None), dict(picks=None), dict(coef=None), dict(loss=None), dict(info=None), dict(G=0), dict(G=-1),
           dict(group_off=None), dict(group_off=np.array([1, 1, 2], np.int32)), dict(group_off=np.array([0, 1, 1], np.int32)),
           dict(group_off=np.array([0, 2, 2], np.int32)), dict(group_off=np.array([0, 2, 1], np.int32)), dict(group_off=np.array([0, 1, 3], np.int32)),
           dict(params=p(struct_size=16)), dict(params=p(max_terms=0)), dict(params=p(max_terms=9)), dict(params=p(dep_tol=-1.0)),
           dict(params=p(dep_tol=float("nan"))), dict(params=p(min_gain=-1e-300)), dict(params=p(min_gain=float("nan")))]
    for entry in ("rovmpc_discover_rows", "rovmpc_discover_rows_device"):
        for change in bad:
            rc, msg, bufs = call(entry, **change)
            assert rc == -1 and entry in msg, (entry, change, rc, msg)
            assert all((b == -7).all() for b in bufs.values()), (entry, change)
    rc, msg, bufs = call(F=1, X=np.zeros((B, T, 1)))                         # term 1 reads feature 1, which F = 1 does not have
    assert rc == -1 and "row 1" in msg and all((b == -7).all() for b in bufs.values()), msg
