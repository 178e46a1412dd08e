"""Helpers of the plan-loop tests (MPPI / CEM device-resident closed loops): the plant rule restated in NumPy, the
host-stepped reference loops over the existing step entries, and exact comparison."""
import numpy as np


def same(a, b):
    """Bit for bit, NaN payloads included."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    bits = {8: np.uint64, 4: np.uint32}[a.dtype.itemsize]
    return np.array_equal(a.view(bits), b.view(bits))


def next_state(row, prev_state, prev_record, feedback):
    """The plant rule of rovmpc_closed_loop_device for one step: the measured row; with feedback (theta_prev, gamma_prev) =
    the (theta, gamma) the previous step started from and (theta, gamma) = record[7], record[8] of the previous step."""
    st = np.array(row, dtype=np.float64)
    if feedback and prev_state is not None:
        st[14:16] = prev_state[12:14]
        st[12:14] = prev_record[7:9]
    return st


def record_of(result):
    return np.concatenate([[result.cost, float(result.index)], result.u, result.traj.ravel()])


MPPI_STATS = ("rho", "eta", "ess", "J0")
CEM_STATS = ("J_best", "J_worst_elite", "n_finite", "J0")


def stats_of(ctl, keys):
    s = ctl.last_stats
    return np.stack([np.atleast_1d(s[k]).astype(np.float64) for k in keys], axis=-1)


def host_loop(ctl, rows, feedback, cem=False):
    """T host steps of a single controller (``ctl.step``), the states by ``next_state`` from the records the loop itself
    returned.  Returns dict(records (T, R), plans (T, N, 3), stats (T, 4)[, spreads, elites]) and the states it used."""
    out = {k: [] for k in ("records", "plans", "stats", "spreads", "elites")}
    st, rec, states = None, None, []
    for i in range(len(rows)):
        st = next_state(rows[i], st, rec, feedback)
        ctl.step(st)
        rec = record_of(ctl.last)
        states.append(st)
        out["records"].append(rec)
        out["plans"].append((ctl.mean if cem else ctl.nominal).copy())
        out["stats"].append(stats_of(ctl, CEM_STATS if cem else MPPI_STATS)[0])
        if cem:
            out["spreads"].append(ctl.std.copy()); out["elites"].append(ctl.elites.copy())
    return {k: np.stack(v) for k, v in out.items() if v}, np.stack(states)


def host_loop_batch(ctl, rows, feedback, cem=False):
    """The same for a batched controller: rows (B, T, 16), ``ctl.step(states (B, 16))``; arrays (T, B, ...)."""
    out = {k: [] for k in ("records", "plans", "stats", "spreads", "elites")}
    B, T = rows.shape[:2]
    st, rec = [None] * B, [None] * B
    for i in range(T):
        st = [next_state(rows[b, i], st[b], rec[b], feedback) for b in range(B)]
        ctl.step(np.stack(st))
        rec = [r.copy() for r in ctl.records]
        out["records"].append(ctl.records.copy())
        out["plans"].append((ctl.mean if cem else ctl.nominal).copy())
        out["stats"].append(stats_of(ctl, CEM_STATS if cem else MPPI_STATS))
        if cem:
            out["spreads"].append(ctl.std.copy()); out["elites"].append(ctl.elites.copy())
    return {k: np.stack(v) for k, v in out.items() if v}


PARTS = ("records", "plans", "stats", "spreads", "elites")


def parts_of(res, index=None):
    """A PlanLoopResult (or a dict of its parts) as a dict, each part indexed by ``index`` (e.g. np.s_[:, b]: problem b)."""
    d = res if isinstance(res, dict) else {k: getattr(res, k) for k in PARTS if getattr(res, k) is not None}
    return d if index is None else {k: v[index] for k, v in d.items()}


def assert_rows_equal(got, ref, what=""):
    """The rows of two loops (PlanLoopResult or dict of parts), every part of every step bit for bit."""
    got, ref = parts_of(got), parts_of(ref)
    assert sorted(got) == sorted(ref), (what, sorted(got), sorted(ref))
    for name in got:
        a, b = got[name], ref[name]
        assert a.shape == b.shape and a.dtype == b.dtype, (what, name, a.shape, b.shape, a.dtype, b.dtype)
        bad = [i for i in range(len(a)) if not same(a[i], b[i])]
        assert not bad, (what, name, "first differing step", bad[0])
