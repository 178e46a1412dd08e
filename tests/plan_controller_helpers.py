"""Helpers shared by the MPPI and CEM GPU tests: the oracle's view of a configuration and a model, and the default plan."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def rv():
    import rovmpc
    return rovmpc


@pytest.fixture(scope="module")
def orc():
    from oracle import rovmpc_oracle
    return rovmpc_oracle


def oracle_cfg(orc, cfg):
    return orc.MPCConfig(N=cfg.N, dt=cfg.dt, v_scale=cfg.v_scale, L=cfg.L, cable_wet_weight=cfg.cable_wet_weight,
                         c_lo=cfg.c_lo, c_hi=cfg.c_hi, n_shape_pts=cfg.n_shape_pts,
                         up=1.0 if cfg.frame == "ENU" else -1.0, vt_mode=cfg.vt_mode, prev_mode=cfg.prev_mode,
                         integrator=cfg.integrator, w_theta=cfg.w_theta, w_gamma=cfg.w_gamma, w_u=cfg.w_u,
                         w_T=cfg.w_T, w_taut=cfg.w_taut, rho_taut=cfg.rho_taut, w_floor=cfg.w_floor,
                         z_floor=cfg.z_floor, theta_ref=cfg.theta_ref, gamma_ref=cfg.gamma_ref, U_ref=tuple(cfg.U_ref),
                         feature_map=cfg.feature_map)


def oracle_model(orc, model):
    return orc.DynamicsModel(model.mean, model.scale, orc.SymbolicModel(model.expr_theta),
                             orc.SymbolicModel(model.expr_gamma))


def oracle_J(orc, cfg, model, state, U):
    J, traj, _ = orc.rollout_vec(oracle_cfg(orc, cfg), oracle_model(orc, model), orc.MPCState.from_array(state),
                                 np.asarray(U, dtype=np.float64))
    return J, traj


def defaults(rv, N):
    m = rv.default_model()
    return np.tile(m.mean[3:6], (N, 1)), np.asarray(m.scale[3:6], dtype=np.float64)


def colmax(U, shape):
    K = U.shape[0]
    return np.abs(np.asarray(U, dtype=np.float64)).reshape(K, -1).max(axis=0).reshape(shape)


def batch_costs_after_step_batch(engine, state, U):
    """rovmpc_step_batch_device with B = 2 on the engine, then where rovmpc_batch_costs_device says its costs lie."""
    import torch
    dev = torch.device("cuda", engine.cfg.device)
    st = torch.tensor(np.tile(state, (2, 1)), device=dev)
    dU = torch.tensor(np.stack([U, U]).astype(engine.cfg.np_dtype), device=dev)
    res = torch.empty((2, engine.result_len), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    engine.step_batch_device(2, st.data_ptr(), dU.data_ptr(), res.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    return engine.batch_costs_ptr()
