"""CPU checks of tests/score_reference.py (the NumPy restatement of rovmpc_score_rows' metric law, the 50-digit values and
the derived bounds) and of the host side of rovmpc.score_rows: ranking and argument errors.  No GPU."""
import numpy as np
import pytest

import rovmpc
import score_reference as sr


def _cases():
    """(name, est, pred, Recording) on fixtures A (RK4, every row) and B (every length, integrator and row)."""
    for name, (texts, rec, _) in sr.fixture_a().items():
        for r, text in enumerate(texts):
            est, pred = sr.replay_np(text, rec.X, rec.time, rec.y0, sr.RK4)
            yield "A/%s/%d" % (name, r), est, pred, rec
    for T in sr.B_LENGTHS:
        rec = sr.fixture_b(T)
        for integ in sr.INTEGRATORS:
            for r, text in enumerate(sr.B_ROWS):
                est, pred = sr.replay_np(text, rec.X, rec.time, rec.y0, integ)
                yield "B/%d/%d/%d" % (T, integ, r), est, pred, rec


def test_score_np_is_within_the_bound_on_every_fixture():
    worst, where = 0.0, None
    for name, est, pred, rec in _cases():
        got = sr.score_np(est, rec.truth, pred, rec.target)
        ratios = sr.score_ratios(got, est, rec.truth, pred, rec.target)
        assert not np.isnan(ratios).any(), name            # (no fixture has SS_tot exactly 0)
        if ratios.max() > worst:
            worst, where = float(ratios.max()), name
    print("score_np: largest error / bound = %.3g at %s" % (worst, where))
    assert worst <= 1.0, where


def test_fixture_a_is_what_the_issue_describes():
    """Every row finite, the reference's chosen rows win, and the gaps between rows are far above the bound."""
    for name, (texts, rec, chosen) in sr.fixture_a().items():
        r2 = np.array([sr.score_np(*sr.replay_np(t, rec.X, rec.time, rec.y0, sr.RK4)[:1], rec.truth)[0] for t in texts])
        assert np.isfinite(r2).all()
        assert int(np.argmax(r2)) == chosen
        assert abs(r2[chosen] - 0.99999914) < 5e-9
        gap = np.min(np.diff(np.sort(r2)))
        print("%s: best R2 %.8f, smallest gap %.2g" % (name, r2[chosen], gap))
        assert gap > 1e-6


@pytest.mark.parametrize("mutant", ["one_pass", "about_zero"])
def test_a_wrong_variance_fails_the_bound(mutant):
    """A truth series offset by 1e6: the one-pass variance (and SS_tot about 0) miss the bound, the two-pass law holds it."""
    rng = np.random.default_rng(11)
    n = 300
    truth = 1e6 + rng.standard_normal(n)
    est = truth + 0.1 * rng.standard_normal(n)
    good = sr.score_ratios(sr.score_np(est, truth), est, truth)
    bad = sr.score_ratios(sr.score_np(est, truth, mutant=mutant), est, truth)
    assert good.max() <= 1.0
    assert bad[0] > 1.0


def test_r2_agrees_with_sklearn():
    skm = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(5)
    for n in (2, 3, sr.TILE, sr.TILE + 1, 300):
        y = rng.standard_normal(n) + 3.0
        e = y + 0.2 * rng.standard_normal(n)
        got = sr.score_np(e, y)[0]
        _, bnd = sr.score_true(e, y)
        assert abs(got - skm.r2_score(y, e)) <= 2 * bnd[0]
    # SS_tot = 0: 1 for a perfect fit, 0 otherwise (force_finite); the constant is summed exactly
    for n in (2, 5, sr.TILE + 1):
        y = np.full(n, 0.5)
        assert sr.score_np(y.copy(), y)[0] == skm.r2_score(y, y.copy()) == 1.0
        e = y + 0.25
        assert sr.score_np(e, y)[0] == skm.r2_score(y, e) == 0.0
    assert np.isnan(sr.score_np(np.ones(1), np.ones(1))[0])            # n < 2 (sklearn warns and returns NaN too)


def _scores(r2):
    t = np.zeros((len(r2), np.shape(r2)[1], 8))
    t[..., 0] = r2
    t[..., 1] = -np.asarray(r2)
    return rovmpc.RowScores.from_table(t)


def test_rank_puts_nan_last_and_breaks_ties_to_the_lower_index():
    s = _scores([[0.5, 0.5], [np.nan, 0.9], [0.9, 0.9], [0.5, 0.5], [-np.inf, 0.0], [0.9, 0.9]])
    assert list(s.rank("r2")) == [2, 5, 0, 3, 4, 1]
    assert list(s.rank("rmse")) == [2, 5, 0, 3, 4, 1]                  # smaller is better, same order by construction
    assert list(s.rank("r2", reduce="min")) == [2, 5, 0, 3, 4, 1]
    assert s.best() == 2
    with pytest.raises(ValueError):
        s.rank("r3")
    with pytest.raises(ValueError):
        s.rank("r2", reduce="sum")


def test_bad_shapes_and_options_raise_before_the_library_is_called(monkeypatch):
    from rovmpc import engine as eng_mod
    monkeypatch.setattr(eng_mod, "default_engine", lambda: pytest.fail("the library was reached"))
    X, t, y = np.zeros((10, 18)), np.arange(10.0), np.zeros(10)
    bad = [
        dict(rows=["x0"], X=np.zeros(10), time=t, truth=y),                       # X not 2-D / 3-D
        dict(rows=["x0"], X=X, time=t[:9], truth=y),                              # time length
        dict(rows=["x0"], X=X, time=t, truth=np.zeros((2, 10))),                  # truth shape
        dict(rows=["x0"], X=X, time=t, truth=y, target=np.zeros(9)),
        dict(rows=["x0"], X=np.zeros((10, 33)), time=t, truth=y),                 # more than ROVMPC_MAX_FEATURES
        dict(rows=["x0"], X=np.zeros((0, 18)), time=t[:0], truth=y[:0]),          # T < 1
        dict(rows=[], X=X, time=t, truth=y),
        dict(rows="x0", X=X, time=t, truth=y),                                    # a single row is not a sequence of rows
        dict(rows=[3.0], X=X, time=t, truth=y),
        dict(rows=["x0"], X=X, time=t, truth=y, integrator="rk5"),
        dict(rows=["x0"], X=X, time=t, truth=y, integrator=7),
        dict(rows=["x0"], X=X, time=t, truth=y, lengths=[11]),
        dict(rows=["x0"], X=X, time=t, truth=y, lengths=[0]),
        dict(rows=["x0"], X=X, time=t, truth=y, lengths=[5, 5]),
        dict(rows=["x0"], X=X, time=t, truth=y, lengths=[2.5]),
        dict(rows=["x0"], X=X, time=t, truth=y, y0=[0.0, 1.0]),
        dict(rows=["x18"], X=X, time=t, truth=y),                                 # feature index beyond F
        dict(rows=["x0 +"], X=X, time=t, truth=y),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            rovmpc.score_rows(**kw)
    with pytest.raises(ValueError):
        rovmpc.select_model(["x0"], ["x1"], X, t, y, y, np.zeros(17), np.ones(17))
    with pytest.raises(ValueError):
        rovmpc.RowScores.from_table(np.zeros((3, 8)))
