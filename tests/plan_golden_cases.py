"""The cases of tests/golden/plan_controllers.npz, shared by tools/make_plan_golden.py (which records them) and
test_plan_golden_gpu.py (which compares): the inputs of the batched controller tests (``problems``, ``plans_for``,
``seeds_for``), the case table, ``run_case``, which runs one case on the GPU and returns its arrays by name, and the file
format (``save_fixture`` / ``load_fixture``)."""
import hashlib
import json
from collections import namedtuple

import numpy as np

from plan_controller_helpers import defaults
from plan_loop_helpers import CEM_STATS, MPPI_STATS, PARTS, parts_of, record_of, stats_of

STEPS = 3          # warm-started control steps of a step case
LOOP_T = 4         # control steps of a device loop, followed by one host step


def problems(rv, B, K, N, s):
    """States (B, 16) of control step s: every problem and every step its own."""
    base, _ = rv.synthetic_problem(K, N)
    st = np.tile(base, (B, 1))
    b = np.arange(B, dtype=np.float64)
    st[:, 12] += 0.01 * s + 0.003 * b
    st[:, 13] -= 0.005 * s + 0.002 * b
    st[:, 3:6] *= (1.0 + 0.05 * s + 0.02 * b)[:, None]
    st[:, 14:16] = st[:, 12:14] - 1e-3 * (1.0 + b)[:, None]
    return st


def plans_for(rv, B, N):
    mean, std = defaults(rv, N)
    rng = np.random.default_rng(B * 1000 + N)
    return mean[None] + 0.05 * std * rng.standard_normal((B, N, 3)), std


def seeds_for(B):
    return [1000003 * (b + 1) + 17 for b in range(B)]


# kind: "mppi" | "cem" | "update"; B None: the single-problem controller; feedback None: steps, else a device loop;
# nan: problem 1 of the batch starts every step from theta = NaN
Case = namedtuple("Case", "name kind N K n_iter dtype n_elite B feedback nan")


def _cases():
    out = []

    def add(kind, N, K, n_iter, dtype="f64", n_elite=None, B=None, feedback=None, nan=False):
        name = "-".join([kind, f"N{N}", f"K{K}", f"I{n_iter}", dtype] + ([f"E{n_elite}"] if n_elite else [])
                        + ["single" if B is None else f"B{B}"] + ([] if feedback is None else [f"loop-fb{feedback}"])
                        + (["nan"] if nan else []))
        out.append(Case(name, kind, N, K, n_iter, dtype, n_elite, B, feedback, nan))

    for kind, E in (("mppi", None), ("cem", 24)):
        for dtype in ("f64", "f32"):            # the base law, the n_iter counter, half flipping; 8 MPPI update workgroups
            for B in (None, 1, 3):
                add(kind, 12, 512, 2, dtype, E, B)
    for kind, E in (("mppi", None), ("cem", 16)):
        for B in (None, 2):                     # 3 N > 256: the QC = 4 instantiations
            add(kind, 90, 384, 2, "f64", E, B)
    for B in (None, 2):                         # two CEM update workgroups: slab rows and a ticket per problem
        add("cem", 20, 8192, 2, "f64", 96, B)
    for kind, E in (("mppi", None), ("cem", 24)):
        for B in (None, 3):                     # PlanHandoff rows, the state hand-off, publication at the last step only
            for feedback in (0, 1):
                add(kind, 12, 512, 2, "f64", E, B, feedback)
    add("update", 12, 512, 2, n_elite=24)       # rovmpc_*_update_device on the U and J the first case ends with
    add("cem", 12, 512, 2, "f64", 24, 3, nan=True)      # the keep-the-plan branch through the batched copy-out
    return out


CASES = _cases()


def lam_key(c):
    return f"lam/N{c.N}-K{c.K}-{c.dtype}"


def measure_lam(rv, c):
    """A temperature on the scale of the spread of one draw's costs, so that the weights neither collapse nor flatten.
    Measured when the fixture is recorded and kept in it as an input of the MPPI cases."""
    plans, std = plans_for(rv, 1, c.N)
    m = rv.MPPI(rv.MPCConfig(N=c.N, K=c.K, dtype=c.dtype), lam=1.0, std=std, n_iter=1, nominal=plans[0])
    m.step(problems(rv, 1, c.K, c.N, 0)[0])
    J = np.asarray(m.engine.mppi_last()[1], dtype=np.float64)
    m.close()
    J = J[np.isfinite(J)]
    return float(max(np.median(J - J.min()), 1e-12))


def cem_kw(rv, c):
    mean0, std = defaults(rv, c.N)
    return dict(n_elite=c.n_elite, n_iter=c.n_iter, alpha=0.15, std=std, std_min=0.02 * std, lo=mean0[0] - 1.2 * std,
                hi=mean0[0] + 0.9 * std)


def make_controller(rv, c, lam):
    cfg = rv.MPCConfig(N=c.N, K=c.K, dtype=c.dtype)
    B = c.B or 1
    plans, std = plans_for(rv, B, c.N)
    seeds = seeds_for(B)
    if c.kind == "cem":
        if c.B is None:
            return rv.CEM(cfg, seed=seeds[0], mean=plans[0], **cem_kw(rv, c))
        return rv.BatchedCEM(cfg, B=B, seeds=seeds, mean=plans, **cem_kw(rv, c))
    if c.B is None:
        return rv.MPPI(cfg, lam=lam, std=std, n_iter=c.n_iter, seed=seeds[0], nominal=plans[0])
    return rv.BatchedMPPI(cfg, B=B, lam=lam, std=std, n_iter=c.n_iter, seeds=seeds, nominal=plans)


def states_of(rv, c, s):
    st = problems(rv, c.B or 1, c.K, c.N, s)
    if c.nan:
        st[1, 12] = np.nan
    return st if c.B is not None else st[0]


def sha256(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def last_digests(ctl, c):
    e = ctl.engine
    U, J = ctl.candidates() if c.B is not None else (e.cem_last() if c.kind == "cem" else e.mppi_last())
    return {"U_sha256": sha256(U), "J_sha256": sha256(J)}


def snapshot(ctl, c):
    """What a control step left behind: record(s), plan (and spread), stats, elite lists, digests of the last U and J."""
    cem = c.kind == "cem"
    out = {"records": ctl.records if c.B is not None else record_of(ctl.last),
           "plans": ctl.mean if cem else ctl.nominal,
           "stats": stats_of(ctl, CEM_STATS if cem else MPPI_STATS)}
    if cem:
        out.update(spreads=ctl.std, elites=ctl.elites)
    out.update(last_digests(ctl, c))
    return {k: np.array(v) for k, v in out.items()}


def run_update_case(rv, c, lam):
    """rovmpc_mppi_update_device and rovmpc_cem_update_device, once each, on the last U and J of CASES[0]."""
    import torch
    first = CASES[0]
    ctl = make_controller(rv, first, lam)
    for s in range(STEPS):
        ctl.step(states_of(rv, first, s))
    U, J = ctl.engine.mppi_last()
    plans, std = plans_for(rv, 1, c.N)
    dev = torch.device("cuda", ctl.cfg.device)
    dU, dJ = torch.tensor(U, device=dev), torch.tensor(J, device=dev)
    d_in, d_sg = torch.tensor(plans[0], device=dev), torch.tensor(np.tile(std, (c.N, 1)), device=dev)
    nu, mu, sg = (torch.empty((c.N, 3), dtype=torch.float64, device=dev) for _ in range(3))
    st_m, st_c = (torch.empty(4, dtype=torch.float64, device=dev) for _ in range(2))
    el = torch.empty(c.n_elite, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    torch.cuda.synchronize(dev)
    ctl.engine.mppi_update_device(dJ.data_ptr(), dU.data_ptr(), lam, d_in.data_ptr(), nu.data_ptr(), st_m.data_ptr(), stream)
    kw = cem_kw(rv, c)
    p = rv.CEMParams.make(kw["n_iter"], kw["n_elite"], kw["alpha"], kw["std"], kw["std_min"], kw["lo"], kw["hi"])
    with rv.Engine(rv.MPCConfig(N=c.N, K=c.K, dtype=c.dtype)) as e:
        e.cem_update_device(dJ.data_ptr(), dU.data_ptr(), p, d_in.data_ptr(), d_sg.data_ptr(), mu.data_ptr(), sg.data_ptr(),
                            el.data_ptr(), st_c.data_ptr(), stream)
        torch.cuda.synchronize(dev)
    ctl.close()
    return {"mppi_plan": nu.cpu().numpy(), "mppi_stats": st_m.cpu().numpy(), "cem_plan": mu.cpu().numpy(),
            "cem_spread": sg.cpu().numpy(), "cem_elites": el.cpu().numpy(), "cem_stats": st_c.cpu().numpy()}


def run_case(rv, c, lam):
    """The arrays of case c by name.  Step cases: every part stacked over the STEPS steps.  Loop cases: the loop's rows split
    into their parts (``loop_*``), the digests after the loop, then one host step (``next_*``)."""
    if c.kind == "update":
        return run_update_case(rv, c, lam)
    ctl = make_controller(rv, c, lam)
    if c.feedback is None:
        steps = []
        for s in range(STEPS):
            ctl.step(states_of(rv, c, s))
            steps.append(snapshot(ctl, c))
        out = {k: np.stack([s[k] for s in steps]) for k in steps[0]}
    else:
        rows = np.stack([states_of(rv, c, s) for s in range(LOOP_T)], axis=-2)         # (T, 16) or (B, T, 16)
        res = parts_of(ctl.run(rows, bool(c.feedback)))
        out = {"loop_" + k: res[k] for k in PARTS if k in res}
        out.update({"loop_" + k: v for k, v in last_digests(ctl, c).items()})
        ctl.step(states_of(rv, c, LOOP_T))
        out.update({"next_" + k: v for k, v in snapshot(ctl, c).items()})
    ctl.close()
    return out


def save_fixture(path, arrays):
    """All arrays as one byte string and an index of (name, dtype, shape): most of them are smaller than a zip member's
    own headers, and a single controller and its batch of one repeat each other, which only one stream can fold."""
    index = [(k, a.dtype.str, list(a.shape)) for k, a in arrays.items()]
    data = b"".join(np.ascontiguousarray(a).tobytes() for a in arrays.values())
    np.savez_compressed(path, index=np.array(json.dumps(index)), data=np.frombuffer(data, dtype=np.uint8))


def load_fixture(path):
    with np.load(path) as z:
        index, data = json.loads(str(z["index"])), z["data"].tobytes()
    out, off = {}, 0
    for k, dtype, shape in index:
        n = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
        out[k] = np.frombuffer(data[off:off + n], dtype=dtype).reshape(shape)
        off += n
    assert off == len(data)
    return out
