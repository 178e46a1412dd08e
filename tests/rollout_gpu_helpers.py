"""What the GPU tests of the rollout trajectories share (tests/test_rollout_steps_gpu.py, tests/test_rollout_dd_gpu.py): the
oracle's configuration and model of a product configuration and model, a seeded rotation table, one rollout_costs call with
the trajectory (and a step()), and the check of step()'s record against that call."""
import numpy as np


def oracle_cfg(orc, cfg):
    return orc.MPCConfig(N=cfg.N, dt=cfg.dt, v_scale=cfg.v_scale, L=cfg.L, cable_wet_weight=cfg.cable_wet_weight, c_lo=cfg.c_lo,
                         c_hi=cfg.c_hi, n_shape_pts=cfg.n_shape_pts, up=1.0 if cfg.frame == "ENU" else -1.0, vt_mode=cfg.vt_mode,
                         prev_mode=cfg.prev_mode, integrator=cfg.integrator, w_theta=cfg.w_theta, w_gamma=cfg.w_gamma, w_u=cfg.w_u,
                         w_T=cfg.w_T, w_taut=cfg.w_taut, rho_taut=cfg.rho_taut, w_floor=cfg.w_floor, z_floor=cfg.z_floor,
                         theta_ref=cfg.theta_ref, gamma_ref=cfg.gamma_ref, U_ref=tuple(cfg.U_ref), feature_map=cfg.feature_map)


def oracle_model(orc, model):
    return orc.DynamicsModel(model.mean, model.scale, orc.SymbolicModel(model.expr_theta), orc.SymbolicModel(model.expr_gamma))


def rand_rtab(N, seed=7):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(N):
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] *= -1
        out.append(q)
    return np.stack(out)


def rollout(rv, cfg, model, state, U, Rtab=None, with_step=False, path=None):
    U = np.ascontiguousarray(U, dtype=cfg.np_dtype)
    with rv.Engine(cfg, model) as e:
        if path is not None:
            assert e.model_path == path
        if Rtab is not None:
            e.set_rotation_table(Rtab)
        J, traj = e.rollout_costs(state, U, return_traj=True)
        res = e.step(state, U) if with_step else None
    return U, J, traj, res


def record_is_the_best_row(res, U, J, traj):
    k = int(np.argmin(J))
    assert res.index == k and res.cost == float(J[k])
    assert np.array_equal(res.u, U[k, 0].astype(np.float64)) and np.array_equal(res.traj, traj[k].astype(np.float64))


def oracle_model_named(orc, model):
    """The oracle's model of a product model whose text names its variables (the second-order generation)."""
    return orc.DynamicsModel(model.mean, model.scale, orc.SymbolicModel(model.expr_theta, len(model.mean), model.variable_names),
                             orc.SymbolicModel(model.expr_gamma, len(model.mean), model.variable_names))
