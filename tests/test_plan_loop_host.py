"""The device-resident MPPI / CEM loops on the host side: the header declares the four entries and the two row-length
functions, the binding has the header's argument order, the parameter and configuration structs are unchanged, ``run``
rejects bad shapes, batch sizes and feedback values before any library call, rows split into their parts, and the NumPy
plant rule the GPU tests use agrees with closed_loop.state_of_step.  No compute call into the library happens here."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import rovmpc
from rovmpc import closed_loop
from rovmpc.mpc import loop_feedback, loop_rows, loop_rows_batch, split_rows

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from plan_loop_helpers import next_state  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I32, I64, U64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64
MP, CP = ctypes.POINTER(rovmpc.MPPIParams), ctypes.POINTER(rovmpc.CEMParams)
# name -> (result, argument types, the header's parameter names in order)
SIGNATURES = {
    "rovmpc_mppi_row_len": (I32, [P], ["h"]),
    "rovmpc_cem_row_len": (I32, [P, I32], ["h", "n_elite"]),
    "rovmpc_mppi_closed_loop_device": (ctypes.c_int, [P, P, I64, I32, U64, U64, MP, P],
                                       ["h", "d_exo", "T", "feedback", "seed", "step0", "p", "d_rows"]),
    "rovmpc_cem_closed_loop_device": (ctypes.c_int, [P, P, I64, I32, U64, U64, CP, P],
                                      ["h", "d_exo", "T", "feedback", "seed", "step0", "p", "d_rows"]),
    "rovmpc_mppi_closed_loop_batch_device": (ctypes.c_int, [P, I32, P, I64, I32, P, U64, MP, P],
                                             ["h", "B", "d_exo", "T", "feedback", "seeds", "step0", "p", "d_rows"]),
    "rovmpc_cem_closed_loop_batch_device": (ctypes.c_int, [P, I32, P, I64, I32, P, U64, CP, P],
                                            ["h", "B", "d_exo", "T", "feedback", "seeds", "step0", "p", "d_rows"]),
}
C_TYPES = {"int32_t": I32, "int64_t": I64, "uint64_t": U64}


def _header():
    return open(os.path.join(ROOT, "include", "rovmpc.h")).read()


def test_header_declares_the_loop_entries_in_the_bound_order():
    hdr = _header()
    for name, (res, args, names) in SIGNATURES.items():
        m = re.search(r"\b(int|int32_t) " + name + r"\s*\(([^;]*?)\);", hdr, re.S)
        assert m, name
        assert (m.group(1) == "int32_t") == name.endswith("_row_len"), name
        params = [" ".join(p.split()) for p in m.group(2).split(",")]
        assert [p.split()[-1].lstrip("*") for p in params] == names, name
        for p, t in zip(params, args):                       # pointers bind as void* / POINTER(params), scalars by width
            if "*" in p:
                assert t in (P, MP, CP), (name, p)
                assert (t is MP) == ("rovmpc_mppi_params" in p) and (t is CP) == ("rovmpc_cem_params" in p), (name, p)
            else:
                assert C_TYPES[p.split()[0]] is t, (name, p)
        assert name in rovmpc.exported_symbols(), name
    assert "bit for bit what rovmpc_<ctl>_step(state_i, seed, step0 + i, p) publishes" in hdr
    assert "first predicted node of the cheapest candidate" in hdr and "each call starts" in hdr
    for m in re.finditer(r"Not provided:(.*?)\*/", hdr, re.S):
        if "pipelined" not in m.group(1):                    # (the loops' own list names the pipelined and sharded forms)
            assert "closed-loop" not in m.group(1) and "closed loop" not in m.group(1)


def test_symbols_resolve_with_the_declared_types():
    lib = rovmpc.load_library()
    raw = ctypes.CDLL(rovmpc.LIB_PATH)
    for name, (res, args, _) in SIGNATURES.items():
        assert getattr(raw, name)                            # exported by the built library itself
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert lib.rovmpc_mppi_row_len(None) == 0 and lib.rovmpc_cem_row_len(None, 4) == 0


def test_structs_unchanged():
    """Sizes and field order of the parameter and configuration structs (the loops add no field)."""
    from rovmpc._lib import Config
    assert ctypes.sizeof(rovmpc.MPPIParams) == 40 and [f[0] for f in rovmpc.MPPIParams._fields_] == ["struct_size", "n_iter", "lambda_", "std"]
    assert ctypes.sizeof(rovmpc.CEMParams) == 120
    assert [f[0] for f in rovmpc.CEMParams._fields_] == ["struct_size", "n_iter", "n_elite", "reserved", "alpha", "std", "std_min", "lo", "hi"]
    assert ctypes.sizeof(Config) == 17 * 4 + 4 + 19 * 8
    assert [f[0] for f in Config._fields_] == [
        "struct_size", "device", "dtype", "N", "K", "n_shape_pts", "vt_mode", "prev_mode", "integrator", "frame", "force_interpreter",
        "candidates_per_block", "debug_flags", "jit_off", "feature_map", "threads_per_block", "no_builtin", "dt", "v_scale", "L",
        "cable_wet_weight", "c_lo", "c_hi", "w_theta", "w_gamma", "w_u", "w_T", "w_taut", "rho_taut", "w_floor", "z_floor",
        "theta_ref", "gamma_ref", "U_ref"]
    hdr = _header()
    for struct, fields in (("rovmpc_mppi_params", ["struct_size", "n_iter", "lambda", "std[3]"]),
                           ("rovmpc_cem_params", ["struct_size", "n_iter", "n_elite", "reserved", "alpha", "std[3]", "std_min[3]", "lo[3], hi[3]"])):
        body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", hdr, re.S).group(1)
        decl = [re.sub(r"^\s*(int32_t|double)\s+", "", ln.split(";")[0]) for ln in body.splitlines() if ";" in ln]
        assert decl == fields, struct
    assert "/* 120 bytes */" in hdr


def test_exports():
    assert rovmpc.PlanLoopResult is rovmpc.mpc.PlanLoopResult and rovmpc.run_plan_closed_loop is closed_loop.run_plan_closed_loop
    for cls in (rovmpc.MPPI, rovmpc.CEM, rovmpc.BatchedMPPI, rovmpc.BatchedCEM):
        assert callable(cls.run)
    for name in ("mppi_row_len", "cem_row_len", "mppi_closed_loop_device", "cem_closed_loop_device", "mppi_closed_loop_batch_device",
                 "cem_closed_loop_batch_device"):
        assert callable(getattr(rovmpc.Engine, name)), name


# ---- ``run`` checks its arguments before any library call ---------------------------------------------------------------------
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the library was reached")


def _controller(cls, **attrs):
    c = object.__new__(cls)                                  # no handle: every use of the engine says so
    c.engine = _NoLibrary()
    for k, v in attrs.items():
        setattr(c, k, v)
    return c


GOOD = np.zeros((5, 16))
BAD_ROWS = [np.zeros((5, 15)), np.zeros(16), np.zeros((0, 16)), np.zeros((2, 5, 16)), [[1.0, 2.0]]]
BAD_FEEDBACK = [2, -1, 0.5, "yes", None]


@pytest.mark.parametrize("cls", [rovmpc.MPPI, rovmpc.CEM])
def test_run_rejects_before_the_library(cls):
    c = _controller(cls)
    for rows in BAD_ROWS:
        with pytest.raises(ValueError):
            c.run(rows)
    for fb in BAD_FEEDBACK:
        with pytest.raises(ValueError):
            c.run(GOOD, fb)
    with pytest.raises(AssertionError, match="the library was reached"):
        c.run(GOOD, True)


@pytest.mark.parametrize("cls", [rovmpc.BatchedMPPI, rovmpc.BatchedCEM])
def test_batched_run_rejects_before_the_library(cls):
    c = _controller(cls, B=3)
    for rows in (np.zeros((2, 5, 16)), np.zeros((4, 5, 16)), np.zeros((3, 5, 15)), np.zeros((3, 0, 16)), np.zeros((5, 15)), np.zeros(16),
                 np.zeros((1, 3, 5, 16))):
        with pytest.raises(ValueError):
            c.run(rows)
    for fb in BAD_FEEDBACK:
        with pytest.raises(ValueError):
            c.run(np.zeros((3, 5, 16)), fb)
    for rows in (np.zeros((3, 5, 16)), GOOD):
        with pytest.raises(AssertionError, match="the library was reached"):
            c.run(rows, 1)


def test_rows_and_feedback_helpers():
    r = np.arange(32.0).reshape(2, 16)
    assert loop_rows(r.tolist()).dtype == np.float64 and np.array_equal(loop_rows(r), r)
    b = loop_rows_batch(r, 3)
    assert b.shape == (3, 2, 16) and b.flags.c_contiguous and b.flags.writeable and all(np.array_equal(b[i], r) for i in range(3))
    full = np.arange(96.0).reshape(3, 2, 16)
    assert np.array_equal(loop_rows_batch(full, 3), full)
    assert [loop_feedback(v) for v in (False, True, 0, 1, np.bool_(True), np.int64(0))] == [False, True, False, True, True, False]


def test_split_rows():
    R, N, E = 5 + 2 * 3, 2, 3
    mppi = np.arange(2 * (R + 6 + 4), dtype=np.float64).reshape(2, -1)
    s = split_rows(mppi, R, N)
    assert np.array_equal(s.records, mppi[:, :R]) and np.array_equal(s.plans.reshape(2, -1), mppi[:, R:R + 6])
    assert np.array_equal(s.stats, mppi[:, R + 6:]) and s.spreads is None and s.elites is None
    assert np.array_equal(s.u, mppi[:, 2:5]) and np.array_equal(s.cost, mppi[:, 0])
    cem = np.arange(4 * (R + 12 + 4 + E), dtype=np.float64).reshape(2, 2, -1)             # (T, B, W)
    cem[..., -E:] = np.array([7, 1, -1], dtype=np.int64).view(np.float64)
    s = split_rows(cem, R, N, E)
    assert s.records.shape == (2, 2, R) and s.plans.shape == s.spreads.shape == (2, 2, N, 3) and s.stats.shape == (2, 2, 4)
    assert np.array_equal(s.spreads.reshape(2, 2, -1), cem[..., R + 6:R + 12]) and np.array_equal(s.stats, cem[..., R + 12:R + 16])
    assert s.elites.dtype == np.int64 and s.elites.shape == (2, 2, E) and (s.elites == [7, 1, -1]).all()


# ---- the plant rule ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("feedback", [False, True])
def test_plant_rule_agrees_with_state_of_step(feedback):
    """next_state, step by step on made-up records, against closed_loop.state_of_step on the report of the same records."""
    rng = np.random.default_rng(5)
    T, N = 7, 4
    rows = rng.standard_normal((T, 16))
    rec = rng.standard_normal((T, 5 + 2 * (N + 1)))
    st, states = None, []
    for i in range(T):
        st = next_state(rows[i], st, rec[i - 1] if i else None, feedback)
        rec[i, 5:7] = st[12:14]                                # a record's node 0 is the state its step started from
        states.append(st)
    tg = np.vstack([rec[0, 5:7], rec[:, 7:9]])
    rep = closed_loop.ClosedLoopReport(T, 1.0, 1.0, 1.0, 1.0, rec[:, 2:5], tg, rec[:, 0])
    for i in range(T):
        assert np.array_equal(states[i], closed_loop.state_of_step(rows, rep, i, feedback)), i
    assert np.array_equal(states[0], rows[0])
    if feedback:
        assert np.array_equal(states[3][:12], rows[3][:12]) and np.array_equal(states[3][12:14], rec[2, 7:9])
        assert np.array_equal(states[3][14:16], states[2][12:14])
    else:
        assert np.array_equal(np.stack(states), rows)
