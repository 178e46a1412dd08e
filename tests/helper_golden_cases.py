"""The cases of tests/golden/helper_entries.npz, shared by tools/make_helper_golden.py (which records them) and
test_helper_entries_gpu.py (which compares): fixed seeded inputs for every host-pointer helper entry of include/rovmpc.h at the
smallest shapes that use every copy, ``call``, which runs one case through the C ABI, and the handle they run on.

A case lists the entry's arguments after the handle, in order: ``In(array)``, ``Val(ctype, value)`` or ``Out(name, shape,
dtype, optional)``.  ``empty`` names the argument set to 0 for the empty-input call (None: the entry does not allow one),
``bad`` the argument and value of a call that must be refused."""
import ctypes as C
from collections import namedtuple

import numpy as np

In = namedtuple("In", "array")
Val = namedtuple("Val", "ctype value")
Out = namedtuple("Out", "name shape dtype optional")
Case = namedtuple("Case", "name fn args empty bad")

POISON = 0xA5          # every byte of an output array before the call

OK, ERR_INVALID = 0, -1


def handle(rv):
    """The engine the cases run on: the default model (18 features), everything else as configured by default."""
    return rv.Engine(rv.MPCConfig(N=20, K=256, device=0), rv.default_model())


def _rng(tag):
    return np.random.default_rng(20240 + tag)


def _i64(v):
    return Val(C.c_int64, v)


def _i32(v):
    return Val(C.c_int32, v)


def _f64(v):
    return Val(C.c_double, v)


def _programs(rv, texts, n_features):
    from rovmpc.expr import compile_expression
    consts = []
    codes = [np.asarray(compile_expression(t, consts, n_features).code, dtype=np.int32) for t in texts]
    return codes, np.asarray(consts, dtype=np.float64)


def _endpoints(tag, n):
    r = _rng(tag)
    A = r.uniform(-0.3, 0.3, (n, 3))
    B = A + np.column_stack([r.uniform(0.8, 1.6, n), r.uniform(-0.6, 0.6, n), r.uniform(-0.5, 0.5, n)])
    return A, B


def _track(tag, T):
    """Marker positions, velocity, time and angles of T rows (the estimation entries' inputs)."""
    r = _rng(tag)
    time = np.cumsum(r.uniform(0.015, 0.02, T))
    P0 = r.uniform(-0.2, 0.2, (T, 3)) + np.linspace(0.0, 0.3, T)[:, None]
    P1 = P0 + r.uniform(0.5, 1.5, (T, 3))
    V = r.uniform(-0.4, 0.4, (T, 3))
    return P0, P1, V, time, r.uniform(-0.5, 0.5, T), r.uniform(-0.5, 0.5, T)


def cases(rv):
    from rovmpc import _lib
    out = []
    n = 3
    r = _rng(1)
    Xs = r.standard_normal((n, 18))
    for which, nm in ((0, "theta"), (1, "gamma")):
        out.append(Case(f"predict_{nm}", "rovmpc_predict", [In(Xs), _i64(n), _i32(which), Out("out", (n,), "f8", False)],
                        1, (2, 2)))

    (code,), consts = _programs(rv, ["sin(x0) * 1.5 + x1 / (x2 + 3.25)"], 3)
    X3 = _rng(2).uniform(-1.0, 1.0, (n, 3))
    out.append(Case("eval_expression", "rovmpc_eval_expression",
                    [In(code), _i32(len(code)), In(consts), _i32(len(consts)), In(X3), _i32(3), _i64(n), Out("out", (n,), "f8", False)],
                    6, (5, 0)))

    x = np.array([0.3, 1.7, -2.5, 10.25, 1e-3])
    y = np.array([3.0, -0.7, 1.25, 1e-2, 7.0])
    for dt, dn in ((_lib.F64, "f64"), (_lib.F32, "f32")):
        for fn, second_in, second_out in (("SQRT", False, False), ("DIV", True, False), ("SINCOS", False, True)):
            args = [_i32(_lib.PROBE_FN[fn]), _i32(dt), In(x), In(y) if second_in else Val(C.c_void_p, None), _i64(5),
                    Out("out0", (5,), "f8", False),
                    Out("out1", (5,), "f8", True) if second_out else Val(C.c_void_p, None)]
            out.append(Case(f"math_probe_{fn.lower()}_{dn}", "rovmpc_math_probe", args, 4, (0, -1)))

    T, B = 3, 2
    (cth, cga), k = _programs(rv, ["-1.5 * sin(x0) - 0.1 * x2", "cos(x0) - 0.7 * x1 - 0.2 * x3"], 4)
    time = np.array([0.0, 0.02, 0.045])
    y0 = _rng(3).uniform(-0.5, 0.5, (B, 4))
    out.append(Case("lagrangian_rollout", "rovmpc_lagrangian_rollout",
                    [In(cth), _i32(len(cth)), In(cga), _i32(len(cga)), In(k), _i32(len(k)), In(time), _i64(T), In(y0), _i64(B),
                     Out("out", (4, B, T), "f8", False)], None, (7, 0)))

    Xr = _rng(4).standard_normal((T, 18))
    for integ, nm in ((_lib.RK4, "rk4"), (_lib.DOUBLE_EULER, "double_euler")):
        out.append(Case(f"replay_{nm}", "rovmpc_replay",
                        [In(Xr), In(time), _i64(T), _f64(0.1), _f64(-0.2), _i32(integ), Out("theta", (T,), "f8", True),
                         Out("gamma", (T,), "f8", True)], None, (5, 7)))

    ell = np.array([1.2, 2.0, 2.9])
    dH = np.array([0.3, -0.5, 0.0])
    out.append(Case("solve_catenary", "rovmpc_solve_catenary",
                    [In(ell), In(dH), _f64(3.0), _i64(n), Out("C", (n,), "f8", False), Out("T", (n,), "f8", True)], 3, (3, -1)))

    r = _rng(5)
    out.append(Case("rodrigues", "rovmpc_rodrigues",
                    [In(r.standard_normal((n, 3))), In(r.standard_normal((n, 3))), In(r.uniform(-3.0, 3.0, n)), _i64(n),
                     Out("out", (n, 3), "f8", False)], 3, (3, -1)))

    M = 4
    A, Bp = _endpoints(6, n)
    out.append(Case("catenary_points", "rovmpc_catenary_points",
                    [In(A), In(Bp), _f64(3.0), _i64(n), _i32(M), Out("pts", (n, M, 3), "f8", False), Out("valid", (n,), "i4", False),
                     Out("params", (n, 3), "f8", True)], 3, (4, 1)))
    out.append(Case("compute_catenary_3d", "rovmpc_compute_catenary_3d",
                    [In(A), In(Bp), _f64(3.0), _i64(n), _i32(M), Out("pts", (n, M, 3), "f8", False), Out("a", (n,), "f8", True)],
                    3, (4, 1)))
    r = _rng(7)
    out.append(Case("transform_catenary", "rovmpc_transform_catenary",
                    [In(A), In(Bp), In(r.uniform(-0.6, 0.6, n)), In(r.uniform(-0.6, 0.6, n)), _f64(3.0), _i64(n), _i32(M),
                     Out("out", (4, n, M, 3), "f8", False), Out("npts", (n, 2), "i4", False), Out("z_low", (n,), "f8", True)],
                    5, (6, 1)))
    r = _rng(8)
    out.append(Case("velocity_transform", "rovmpc_velocity_transform",
                    [In(r.standard_normal((n, 9))), In(r.standard_normal((n, 3))), _i64(n), Out("out", (n, 3), "f8", False)],
                    2, (2, -1)))

    tr = _track(9, 2)
    out.append(Case("extract_features", "rovmpc_extract_features",
                    [In(a) for a in tr] + [_i64(2), _i32(1), Out("out", (2, 18), "f8", False)], None, (6, 1)))
    tr = _track(10, 11)
    out.append(Case("features_dd", "rovmpc_features_dd",
                    [In(tr[0] * 1e3), In(tr[1] * 1e3), In(tr[2] * 1e3)] + [In(a) for a in tr[3:]] +
                    [_i64(11), _i32(11), _i32(3), Out("features", (11, 14), "f8", False), Out("targets", (11, 2), "f8", True)],
                    None, (7, 4)))
    out.append(Case("gaussian_filter1d", "rovmpc_gaussian_filter1d",
                    [In(_rng(11).standard_normal(5)), _i64(5), _f64(1.0), _f64(4.0), Out("out", (5,), "f8", False)], None, (2, 0.0)))
    Tk, Mk = 2, 3
    r = _rng(12)
    P = r.standard_normal((Tk, Mk, 3))
    Q = P + 0.05 * r.standard_normal((Tk, Mk, 3))
    out.append(Case("kabsch", "rovmpc_kabsch_velocity_transform",
                    [In(P), In(Q), In(r.standard_normal((Tk, 3))), _i64(Tk), _i32(Mk), _i32(1), Out("v", (Tk, 3), "f8", False),
                     Out("R", (Tk, 9), "f8", True)], 3, (4, 0)))
    return out


def call(eng, case, null=(), replace=None):
    """One call of the entry: outputs start poisoned, the optional ones named in ``null`` are passed as null pointers,
    ``replace`` = (argument index, value) overrides one scalar.  Returns (status, {output name: array})."""
    keep, outs, argv = [], {}, [eng._h]
    for i, a in enumerate(case.args):
        if isinstance(a, In):
            buf = np.ascontiguousarray(a.array)
            keep.append(buf)
            argv.append(C.c_void_p(buf.ctypes.data))
        elif isinstance(a, Out):
            if a.name in null:
                assert a.optional, a.name
                argv.append(C.c_void_p(None))
                continue
            buf = np.frombuffer(bytes([POISON]) * (int(np.prod(a.shape)) * np.dtype(a.dtype).itemsize), dtype=a.dtype).reshape(a.shape).copy()
            outs[a.name] = buf
            argv.append(C.c_void_p(buf.ctypes.data))
        else:
            v = replace[1] if replace is not None and replace[0] == i else a.value
            argv.append(a.ctype(v))
    rc = getattr(eng.lib, case.fn)(*argv)
    return rc, outs


def last_error(eng):
    msg = eng.lib.rovmpc_last_error(eng._h)
    return msg.decode() if msg else ""


def optional_outputs(case):
    return [a.name for a in case.args if isinstance(a, Out) and a.optional]


def save_fixture(path, arrays):
    np.savez_compressed(path, **{k.replace("/", "__"): v for k, v in arrays.items()})


def load_fixture(path):
    with np.load(path) as z:
        return {k.replace("__", "/"): z[k] for k in z.files}
