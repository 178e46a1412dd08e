"""CPU checks of tests/horizon_reference.py (the NumPy restatement of rovmpc_score_pairs' law, the 50-digit run and the
measured error figure) and of the host side of rovmpc.score_pairs / select_model(horizon=...): the pair logic through a stand-in
engine that answers with horizon_np, the argument errors, the struct mirror.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rovmpc
import horizon_reference as hr
import score_reference as sr
from rovmpc import _lib
from rovmpc.expr import compile_expression


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def test_horizon_np_is_within_the_recorded_figure_on_every_fixture():
    worst, where = hr.measure(lambda fx, q, b: fx.np_pair(q, b)[1])
    b = hr.bounds()
    print("horizon_np: largest |error| / (u S) = %.4g at %s (recorded figure %g)" % (worst, where, b["np_figure"]))
    assert worst <= b["np_figure"], where
    assert worst >= b["np_figure"] / 4, "the recorded figure is stale: measure it again"


@pytest.mark.parametrize("mutant", ["k3_state", "prev_unshifted"])
def test_a_wrong_stage_fails_the_gpu_margin(mutant):
    worst, where = hr.measure(lambda fx, q, b: fx.np_pair(q, b, mutant)[1])
    assert worst > hr.GPU_MARGIN * hr.bounds()["np_figure"], (mutant, worst, where)


def test_law_sum_is_the_tile_and_tree_order():
    rng = np.random.default_rng(3)
    t = rng.standard_normal(2 * hr.TILE + 5) * 10.0 ** rng.integers(-8, 8, 2 * hr.TILE + 5)
    tiles = [np.concatenate([t[k:k + hr.TILE], np.zeros(max(0, k + hr.TILE - len(t)))]) for k in range(0, len(t), hr.TILE)]

    def tree(v):
        v = list(v)
        s = hr.TILE // 2
        while s:
            for l in range(s):
                v[l] = v[l] + v[l + s]
            s //= 2
        return v[0]
    want = 0.0
    for v in tiles:
        want = want + tree(v)
    assert hr.law_sum(t) == want
    assert hr.law_sum(t[:3]) == tree(list(t[:3]) + [0.0] * (hr.TILE - 3))


def test_single_window_without_named_slots_is_the_replay():
    """The tie to rovmpc_replay's law, in NumPy: rows that read no named slot, one window from row 0."""
    rec = sr.fixture_b(40)
    text_t, text_g = "x3*x5 - 0.5*x2", "sin(x1) + x7"
    mean, scale = np.zeros(18), np.ones(18)
    for integ in (hr.RK4, hr.EULER):
        _, pred = hr.horizon_np(text_t, text_g, rec.X, rec.time, np.full(40, 0.3), np.full(40, -0.2), mean, scale, 39, integrator=integ)
        for c, (text, y0) in enumerate(((text_t, 0.3), (text_g, -0.2))):
            est, _ = sr.replay_np(text, rec.X, rec.time, y0, integ)
            assert hr.same(pred[0, :, c], est[1:]), (integ, c)


# ---- fixture A and the pair logic --------------------------------------------------------------------------------------------------
class StandInEngine:
    """Answers Engine.score_rows and Engine.score_pairs with the NumPy restatements, for the rows of fixture A."""

    def __init__(self, fx):
        self.fx, self.texts, self.calls = fx, {}, []
        for text in fx.theta_rows + fx.gamma_rows:
            consts = []
            prog = compile_expression(text, consts, fx.X.shape[2], None)
            self.texts[(tuple(prog.code), tuple(consts))] = text

    def text(self, program):
        return self.texts[(tuple(program[0]), tuple(program[1]))]

    def score_rows(self, programs, X, time, truth, integrator, target, lengths, y0, return_est, return_pred, device):
        table = np.empty((len(programs), X.shape[0], 8))
        for r, prog in enumerate(programs):
            for b in range(X.shape[0]):
                est, pred = sr.replay_np(self.text(prog), X[b], time[b], truth[b, 0] if y0 is None else y0[b], integrator)
                table[r, b] = sr.score_np(est, truth[b], pred, None if target is None else target[b])
        return table, None, None

    def score_pairs(self, theta_programs, gamma_programs, pairs, X, time, theta, gamma, mean, scale, params, lengths, return_pred, device):
        self.calls.append(np.array(pairs))
        out = np.empty((len(pairs), X.shape[0], params.H, 9))
        for q, (it, ig) in enumerate(pairs):
            for b in range(X.shape[0]):
                out[q, b], _ = hr.horizon_np(self.text(theta_programs[it]), self.text(gamma_programs[ig]), X[b], time[b], theta[b], gamma[b],
                                            mean, scale, params.H, params.stride, params.integrator, params.prev_mode, params.slots(),
                                            n=None if lengths is None else lengths[b])
        return out, None


@pytest.fixture(scope="module")
def skill_a():
    fx = hr.fixture_a()
    eng = StandInEngine(fx)
    return eng, rovmpc.score_pairs(fx.theta_rows, fx.gamma_rows, fx.X[0], fx.time[0], fx.theta[0], fx.gamma[0], fx.mean, fx.scale, fx.H, engine=eng)


def test_fixture_a_is_what_the_issue_describes(skill_a):
    fx = hr.fixture_a()
    _, sk = skill_a
    assert fx.X.shape == (1, 200, 18) and len(fx.theta_rows) == 23 and len(fx.gamma_rows) == 14 and len(fx.pairs) == 322
    assert (np.diff(fx.time[0]) > 0).all() and np.ptp(np.diff(fx.time[0])) > 0
    assert hr.n_windows(200, fx.H, 1) == 192 == sk.windows[0] and 192 == hr.TILE + 64
    assert [tuple(p) for p in sk.pairs] == fx.pairs                       # "product" is theta-major
    assert sk.n_ok.shape == (322, 1, 8)
    assert (sk.n_ok[fx.chosen] == 192).all() and (sk.coverage[fx.chosen] == 1.0).all()
    assert sk.best() == fx.chosen == sk.rank("skill")[0]
    assert sk.expressions[fx.chosen] == (fx.theta_rows[fx.pairs[fx.chosen][0]], fx.gamma_rows[fx.pairs[fx.chosen][1]])
    dm = rovmpc.default_model()
    assert sk.expressions[fx.chosen] == (dm.expr_theta, dm.expr_gamma)
    assert 0.9 < sk.skill_theta[fx.chosen, 0, -1] <= 1 and 0.9 < sk.skill_gamma[fx.chosen, 0, -1] <= 1


def test_rank_puts_nan_last_and_takes_the_step_asked_for(skill_a):
    _, sk = skill_a
    t = sk.table()[:3].copy()
    t[..., 4] = 10
    t[..., 5:7] = np.array([1.0, 2.0])
    t[..., 7:9] = 4.0
    t[1, :, -1, 5] = 0.5                       # pair 1 is best at the last step only
    t[2, :, :, 7] = 0.0                        # ss_hold = 0: skill NaN
    p = rovmpc.PairSkill.from_table(t, sk.pairs[:3], sk.expressions[:3], sk.windows)
    assert list(p.rank()) == [1, 0, 2] and list(p.rank(at=1)) == [0, 1, 2] and p.best() == 1
    assert np.isnan(p.skill_theta[2]).all() and p.skill_theta[0, 0, 0] == 0.75 and p.skill_gamma[0, 0, 0] == 0.5
    assert list(p.rank("rmse_theta", at=8)) == list(np.lexsort((np.arange(3), p.rmse_theta[:, 0, 7])))
    for kw in (dict(metric="r2"), dict(at=0), dict(at=9), dict(reduce="sum")):
        with pytest.raises(ValueError):
            p.rank(**kw)
    with pytest.raises(ValueError):
        rovmpc.PairSkill.from_table(np.zeros((3, 1, 8)), sk.pairs[:3], (), sk.windows)


def test_select_model_with_a_horizon_loads_the_best_pair_of_the_shortlists(skill_a):
    fx = hr.fixture_a()
    eng = StandInEngine(fx)
    X_raw = fx.X[0] * fx.scale + fx.mean
    args = (fx.theta_rows, fx.gamma_rows, X_raw, fx.time[0], fx.theta[0], fx.gamma[0], fx.mean, fx.scale)
    model3 = rovmpc.select_model(*args, engine=eng)
    assert len(model3) == 3 and not eng.calls
    model, s_th, s_ga, sk = rovmpc.select_model(*args, engine=eng, horizon=8, shortlist=3)
    assert len(eng.calls) == 1 and len(eng.calls[0]) == 9
    top_t, top_g = s_th.rank("r2")[:3], s_ga.rank("r2")[:3]
    assert [tuple(p) for p in sk.pairs] == [(it, ig) for it in top_t for ig in top_g]
    it, ig = sk.pairs[sk.best()]
    assert (model.expr_theta, model.expr_gamma) == (fx.theta_rows[it], fx.gamma_rows[ig]) == sk.expressions[sk.best()]
    assert (it, ig) == fx.pairs[fx.chosen]
    whole = skill_a[1]
    q = fx.pairs.index((it, ig))
    np.testing.assert_allclose(sk.table()[sk.best()], whole.table()[q], rtol=1e-6)      # (X_raw scaled back is X to a rounding)
    for kw in (dict(shortlist=0), dict(shortlist=1.5), dict(horizon=0), dict(horizon=8, stride=0), dict(horizon=8, integrator="trapezoid")):
        with pytest.raises(ValueError):
            rovmpc.select_model(*args, engine=eng, **{"horizon": 8, **kw})


# ---- argument errors ---------------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise_before_the_library_is_called(monkeypatch):
    from rovmpc import engine as eng_mod
    monkeypatch.setattr(eng_mod, "default_engine", lambda: pytest.fail("the library was reached"))
    X, t, y = np.zeros((10, 18)), np.arange(10.0), np.zeros(10)
    good = dict(theta_rows=["x0"], gamma_rows=["x1", "x2"], X=X, time=t, theta=y, gamma=y, mean=np.zeros(18), scale=np.ones(18), horizon=3)
    bad = [dict(horizon=0), dict(horizon=2.5), dict(horizon=True), dict(stride=0), dict(integrator="trapezoid"), dict(integrator=2),
           dict(prev_mode="lag"), dict(prev_mode=2), dict(feature_map="gen3"), dict(feature_map={"theta": 14}), dict(feature_map={"gamma": 15}),
           dict(feature_map={"theta": 14, "gamma": 14}), dict(feature_map={"theta": 14, "gamma": 18}), dict(feature_map={"theta": 14, "gamma": 15, "phi": 3}),
           dict(feature_map={"theta": -2, "gamma": 15}), dict(feature_map=3), dict(pairs="all"), dict(pairs="zip"), dict(pairs=[(0, 2)]),
           dict(pairs=[(1, 0)]), dict(pairs=[(0, -1)]), dict(pairs=[]), dict(pairs=[(0.0, 1.0)]), dict(pairs=[(0, 1, 1)]), dict(theta_rows=[]),
           dict(gamma_rows="x1"), dict(theta_rows=["x18"]), dict(gamma_rows=["x0 +"]), dict(X=np.zeros(10)), dict(X=np.zeros((10, 33))),
           dict(time=t[:9]), dict(theta=np.zeros((2, 10))), dict(gamma=np.zeros(9)), dict(mean=np.zeros(17)), dict(scale=np.ones((18, 1))),
           dict(scale=np.where(np.arange(18) == 15, 0.0, 1.0)), dict(scale=np.where(np.arange(18) == 16, np.inf, 1.0)),
           dict(mean=np.where(np.arange(18) == 14, np.nan, 0.0)), dict(lengths=[11]), dict(lengths=[0]), dict(lengths=[2.5]),
           dict(feature_map="gen2", X=np.zeros((10, 14)), mean=np.zeros(14), scale=np.ones(14))]
    for change in bad:
        with pytest.raises(ValueError):
            rovmpc.score_pairs(**dict(good, **change))
    # a scale that is zero at a slot no name points to is nobody's business
    eng = type("E", (), {"score_pairs": lambda self, *a: (np.zeros((2, 1, 3, 9)), None)})()
    sk = rovmpc.score_pairs(**dict(good, scale=np.where(np.arange(18) == 3, 0.0, 1.0), engine=eng))
    assert sk.n_ok.shape == (2, 1, 3) and list(sk.windows) == [7]


# ---- header and mirror --------------------------------------------------------------------------------------------------------------
def test_header_and_struct_mirror_agree():
    hdr = open(os.path.join(hr.ROOT, "include", "rovmpc.h")).read()
    assert sr.header_define("ROVMPC_HORIZON_COLS") == _lib.HORIZON_COLS == len(_lib.HORIZON_NAMES) == len(hr.COLS)
    assert sr.header_define("ROVMPC_HORIZON_TILE") == _lib.HORIZON_TILE == hr.TILE
    assert _lib.HORIZON_NAMES == hr.COLS
    body = re.search(r"typedef struct rovmpc_horizon_params \{(.*?)\} rovmpc_horizon_params;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.replace("int32_t", "").split(",")]
    assert fields == [n for n, _ in _lib.HorizonParams._fields_]
    assert all(t is C.c_int32 for _, t in _lib.HorizonParams._fields_) and C.sizeof(_lib.HorizonParams) == 4 * len(fields)
    p = _lib.HorizonParams.make()
    assert (p.struct_size, p.integrator, p.prev_mode, p.H, p.stride) == (44, _lib.RK4, _lib.PREV_INTERP, 20, 1)
    assert p.slots() == (14, 15, 16, 17, -1, -1) == _lib.FEATURE_MAPS["gen1"] == hr.GEN1 and _lib.FEATURE_MAPS["gen2"] == hr.GEN2
    for name in ("rovmpc_default_horizon_params", "rovmpc_score_pairs", "rovmpc_score_pairs_device"):
        assert name in _lib.exported_symbols() and re.search(name + r"\(", hdr)
    assert "the rollout's law) is rovmpc_score_pairs" in hdr
