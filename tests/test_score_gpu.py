"""rovmpc_score_rows / rovmpc_score_rows_device on the GPU (law in include/rovmpc.h) on the fixtures of tests/score_reference.py:
est bit for bit against rovmpc_replay and pred against rovmpc_eval_expression, the scores against 50 digits from the GPU's own
est / pred bits, the ranking and select_model, independence of the batch, the non-finite law, the device entry, the refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_reference as sr  # noqa: E402
from score_reference import same  # noqa: E402
from plan_controller_helpers import rv  # noqa: E402,F401

pytestmark = pytest.mark.gpu

INTEG_NAMES = {sr.RK4: "rk4", sr.EULER: "euler", sr.DOUBLE_EULER: "double_euler", sr.TRAPEZOID: "trapezoid"}
OTHER_ROWS = (0, 7, -1)                     # the rows the three other integrators are replayed on, per front


class Replayer:
    """rovmpc_replay / rovmpc_eval_expression of single rows: one interpreter handle per expression, kept for the module."""

    def __init__(self, rv):
        self.rv, self.engines = rv, {}

    def engine(self, text, F=18):
        if text not in self.engines:
            m = self.rv.DynamicsModel(np.zeros(F), np.ones(F), text, text)
            self.engines[text] = (self.rv.Engine(self.rv.MPCConfig(N=1, K=1, force_interpreter=True), m), m)
        return self.engines[text]

    def replay(self, text, rec, integ, n=None):
        e, _ = self.engine(text, rec.X.shape[1])
        return e.replay(rec.X[:n], rec.time[:n], rec.y0, rec.y0, integ)[0]

    def predict(self, text, rec, n=None):
        e, m = self.engine(text, rec.X.shape[1])
        return e.eval_expression(m.prog_theta.code, m.consts, rec.X[:n])

    def close(self):
        for e, _ in self.engines.values():
            e.close()


@pytest.fixture(scope="module")
def replayer(rv):
    r = Replayer(rv)
    yield r
    r.close()


def score(rv, texts, rec, integ, **kw):
    kw.setdefault("target", rec.target)
    kw.setdefault("y0", rec.y0)
    return rv.score_rows(list(texts), rec.X, rec.time, rec.truth, integrator=INTEG_NAMES[integ], return_est=True, return_pred=True, **kw)


@pytest.fixture(scope="module")
def gpu_a(rv):
    """Fixture A: {(front, integrator): RowScores of all the front's rows}."""
    return {(name, integ): score(rv, texts, rec, integ) for name, (texts, rec, _) in sr.fixture_a().items() for integ in sr.INTEGRATORS}


@pytest.fixture(scope="module")
def gpu_b(rv):
    """Fixture B: {(T, integrator): RowScores of the three rows}."""
    return {(T, integ): score(rv, sr.B_ROWS, sr.fixture_b(T), integ) for T in sr.B_LENGTHS for integ in sr.INTEGRATORS}


# ---- 1. the bit law ------------------------------------------------------------------------------------------------------------
def test_est_is_replay_and_pred_is_eval_expression_on_the_recorded_table(gpu_a, replayer):
    for name, (texts, rec, _) in sr.fixture_a().items():
        for integ in sr.INTEGRATORS:
            s = gpu_a[(name, integ)]
            rows = range(len(texts)) if integ == sr.RK4 else [r % len(texts) for r in OTHER_ROWS]
            for r in rows:
                assert same(s.est[r, 0], replayer.replay(texts[r], rec, integ)), (name, integ, r)
        for r, text in enumerate(texts):
            assert same(gpu_a[(name, sr.RK4)].pred[r, 0], replayer.predict(text, rec)), (name, r)


def test_est_is_replay_across_the_tile_carries(gpu_b, replayer):
    for T in sr.B_LENGTHS:
        rec = sr.fixture_b(T)
        for integ in sr.INTEGRATORS:
            s = gpu_b[(T, integ)]
            for r, text in enumerate(sr.B_ROWS):
                assert same(s.est[r, 0], replayer.replay(text, rec, integ)), (T, integ, r)
                assert same(s.pred[r, 0], replayer.predict(text, rec)), (T, integ, r)


# ---- 2. the scores against 50 digits ----------------------------------------------------------------------------------------------
def test_scores_are_within_the_derived_bound(gpu_a, gpu_b):
    cases = [((name, integ), s, sr.fixture_a()[name][1]) for (name, integ), s in gpu_a.items()]
    cases += [(key, s, sr.fixture_b(key[0])) for key, s in gpu_b.items()]
    worst, where = 0.0, None
    for key, s, rec in cases:
        table = s.table()
        for r in range(table.shape[0]):
            ratios = sr.score_ratios(table[r, 0], s.est[r, 0], rec.truth, s.pred[r, 0], rec.target)
            assert not np.isnan(ratios).any(), (key, r)
            if ratios.max() > worst:
                worst, where = float(ratios.max()), (key, r)
            assert ratios.max() <= 1.0, (key, r, ratios)
    print("GPU: largest error / bound = %.3g at %s" % (worst, where))


# ---- 3. ranking and selection -----------------------------------------------------------------------------------------------------
def test_ranking_matches_numpy_and_selects_the_reference_rows(rv, gpu_a, scaler):
    fronts = sr.fixture_a()
    for name, (texts, rec, chosen) in fronts.items():
        ref = np.array([sr.score_np(sr.replay_np(t, rec.X, rec.time, rec.y0, sr.RK4)[0], rec.truth) for t in texts])
        want = rv.RowScores.from_table(ref[:, None, :]).rank("r2")
        got = gpu_a[(name, sr.RK4)].rank("r2")
        assert list(got) == list(want)
        assert got[0] == chosen
    mean, scale = scaler
    (tt, rt, _), (tg, rg, _) = fronts["theta"], fronts["gamma"]
    model, s_th, s_ga = rv.select_model(tt, tg, rt.X * scale + mean, rt.time, rt.truth, rg.truth, mean, scale, integrator="rk4")
    dm = rv.default_model()
    assert (model.expr_theta, model.expr_gamma) == (dm.expr_theta, dm.expr_gamma)
    assert s_th.r2.shape == (len(tt), 1) and s_ga.r2.shape == (len(tg), 1)
    state, _ = rv.synthetic_problem(64, 8)
    mppi = rv.MPPI(rv.MPCConfig(N=8, K=64), model)
    u = mppi.step(state)
    mppi.engine.close()
    assert u.shape == (3,) and np.isfinite(u).all()


# ---- 4. independence ---------------------------------------------------------------------------------------------------------------
def test_a_row_alone_equals_the_row_among_all(rv, gpu_a):
    texts, rec, _ = sr.fixture_a()["theta"]
    whole = gpu_a[("theta", sr.RK4)]
    for r in (0, 11, len(texts) - 1):
        alone = score(rv, [texts[r]], rec, sr.RK4)
        assert same(alone.table()[0], whole.table()[r])
        assert same(alone.est[0], whole.est[r]) and same(alone.pred[0], whole.pred[r])
    again = score(rv, texts, rec, sr.RK4)
    assert same(again.table(), whole.table()) and same(again.est, whole.est)


def test_a_recording_of_a_ragged_batch_equals_the_truncated_recording_alone(rv):
    T = 2 * sr.TILE + 3
    rec = sr.fixture_b(T)
    lengths = [T, sr.TILE + 1, 1]
    stack = lambda a: np.stack([a, a, a])
    for integ in sr.INTEGRATORS:
        s = rv.score_rows(list(sr.B_ROWS), stack(rec.X), stack(rec.time), stack(rec.truth), integrator=INTEG_NAMES[integ],
                          target=stack(rec.target), lengths=lengths, return_est=True, return_pred=True)
        for b, n in enumerate(lengths):
            cut = sr.Recording(rec.X[:n], rec.time[:n], rec.truth[:n], rec.target[:n], rec.truth[0])
            alone = score(rv, sr.B_ROWS, cut, integ)
            assert same(s.table()[:, b], alone.table()[:, 0]), (integ, b)
            assert same(s.est[:, b, :n], alone.est[:, 0]) and same(s.pred[:, b, :n], alone.pred[:, 0])
            assert np.isnan(s.est[:, b, n:]).all() and np.isnan(s.pred[:, b, n:]).all()


# ---- 5. the non-finite law ---------------------------------------------------------------------------------------------------------
def test_a_row_that_turns_non_finite(rv, gpu_b):
    T = 2 * sr.TILE + 3
    rec = sr.fixture_b(T)
    for integ in sr.INTEGRATORS:
        s = gpu_b[(T, integ)]
        table = s.table()
        ref = sr.score_np(sr.replay_np(sr.B_ROWS[2], rec.X, rec.time, rec.y0, integ)[0], rec.truth)
        assert 0 < ref[3] < T
        assert table[2, 0, 3] == ref[3] == s.n_finite[2, 0]
        assert np.isnan(table[2, 0, [0, 1, 2, 6, 7]]).all()
        assert np.isnan(table[2, 0, [4, 5]]).all()                       # log(x3) itself is non-finite among the rows
        assert s.rank("r2")[-1] == 2 and s.rank("rmse")[-1] == 2
        assert np.isfinite(table[:2]).all()
        without = score(rv, sr.B_ROWS[:2], rec, integ)                   # the other rows are untouched by the bad one
        assert same(without.table(), table[:2])
        no_target = score(rv, sr.B_ROWS, rec, integ, target=None)
        assert np.isnan(no_target.table()[..., [4, 5]]).all()
        assert same(no_target.table()[..., [0, 1, 2, 3, 6, 7]], table[..., [0, 1, 2, 3, 6, 7]])


# ---- 6. the device entry -----------------------------------------------------------------------------------------------------------
def test_device_entry_gives_the_host_entry_bits(rv, gpu_b):
    T = sr.TILE + 1
    rec = sr.fixture_b(T)
    for integ in (sr.RK4, sr.TRAPEZOID):
        dev = score(rv, sr.B_ROWS, rec, integ, device=True)
        host = gpu_b[(T, integ)]
        assert same(dev.table(), host.table()) and same(dev.est, host.est) and same(dev.pred, host.pred)
    rec = sr.fixture_b(2 * sr.TILE + 3)
    dev = rv.score_rows(list(sr.B_ROWS), np.stack([rec.X, rec.X]), np.stack([rec.time] * 2), np.stack([rec.truth] * 2), integrator="euler",
                        lengths=[sr.TILE, 2], device=True)
    host = rv.score_rows(list(sr.B_ROWS), np.stack([rec.X, rec.X]), np.stack([rec.time] * 2), np.stack([rec.truth] * 2), integrator="euler",
                         lengths=[sr.TILE, 2])
    assert same(dev.table(), host.table())


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_anything_is_launched(rv):
    from rovmpc import _lib
    from rovmpc.engine import _ptr
    OP_PUSH_F, OP_PUSH_C, OP_ADD = (_lib_op(rv, n) for n in ("PUSH_F", "PUSH_C", "ADD"))
    T, B, F = 6, 2, 4
    good = dict(code=np.array([OP_PUSH_F, (0 << 8) | OP_PUSH_C, OP_ADD, (1 << 8) | OP_PUSH_F], np.int32), code_off=np.array([0, 3, 4], np.int32),
                consts=np.array([0.5]), const_off=np.array([0, 1, 1], np.int32), R=2, X=np.zeros((B, T, F)), F=F, time=np.tile(np.arange(T) * 0.1, (B, 1)),
                len=np.array([T, 3], np.int64), T=T, B=B, truth=np.zeros((B, T)), target=None, y0=None, integrator=0)
    e = rv.default_engine()
    order = ("code", "code_off", "consts", "const_off", "R", "X", "F", "time", "len", "T", "B", "truth", "target", "y0", "integrator")

    def call(**change):
        a = dict(good, **change)
        scores = np.full((a["R"] if a["R"] > 0 else 1, max(a["B"], 1), 8), -7.0)
        args = [_ptr(a[k]) if isinstance(a[k], np.ndarray) or a[k] is None else a[k] for k in order]
        rc = e.lib.rovmpc_score_rows(e._h, *args, _ptr(scores) if change.get("scores", 1) is not None else None, None, None)
        msg = e.lib.rovmpc_last_error(e._h).decode()
        return rc, msg, scores

    rc, _, scores = call()
    assert rc == 0 and not (scores == -7.0).any()
    bad = [dict(R=0), dict(B=0), dict(T=0), dict(len=np.array([T, 0], np.int64)), dict(len=np.array([T + 1, 1], np.int64)), dict(F=0),
           dict(F=_lib.MAX_FEATURES + 1), dict(code_off=np.array([0, 4, 3], np.int32)), dict(const_off=np.array([0, 1, 0], np.int32)),
           dict(code_off=np.array([1, 3, 4], np.int32)), dict(code=None), dict(code_off=None), dict(consts=None), dict(const_off=None),
           dict(X=None), dict(time=None), dict(truth=None), dict(scores=None), dict(integrator=4), dict(integrator=-1)]
    for change in bad:
        rc, msg, scores = call(**change)
        assert rc == -1 and "rovmpc_score_rows" in msg, (change, rc, msg)
        assert (scores == -7.0).all(), change
    # a bad row is named: row 1 reads feature 1, which F = 1 does not have; row 0 underflows the stack
    rc, msg, scores = call(F=1, X=np.zeros((B, T, 1)))
    assert rc == -1 and "row 1" in msg and (scores == -7.0).all(), msg
    rc, msg, scores = call(code=np.array([OP_ADD, OP_PUSH_F, OP_PUSH_F, OP_PUSH_F], np.int32))
    assert rc == -1 and "row 0" in msg and (scores == -7.0).all(), msg
    assert e.lib.rovmpc_score_rows(None, *[None] * 4, 1, None, 1, None, None, 1, 1, None, None, None, 0, None, None, None) == -1


def _lib_op(rv, name):
    from rovmpc import expr
    return expr.OP[name]
