"""CPU tests of the navigation cost (rovmpc_set_nav_cost): the 50-digit reference of tests/nav_reference.py against closed
forms, the clamp of the track row, and the argument checks of rovmpc.NavCost / _lib.nav_cost, which come before any library
call."""
import ctypes as C
import os
import re

import mpmath as mp
import numpy as np
import pytest

import rovmpc
from rovmpc import _lib
import nav_reference as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
c = 1e-3 / 60.0


def test_constant_control_is_a_straight_line_and_its_track_costs_nothing():
    N, u, P0 = 7, np.array([300.0, -120.0, 45.0]), np.array([0.5, -0.25, -0.75])
    U = np.tile(u, (1, N, 1))
    Pk = nr.path(P0, U[0], c)
    for n in range(1, N + 1):
        for ch in range(3):
            assert abs(Pk[n - 1][ch] - (mp.mpf(float(P0[ch])) + n * mp.mpf(c) * mp.mpf(float(u[ch])))) < mp.mpf(10) ** -45
    # the track through that path (rounded to double): C is zero to the rounding of the rows, and the rate term is zero
    track = np.array([[float(v) for v in Pk[n]] for n in range(N)])
    Cs, b = nr.nav_cost_ref(P0, U, 0, c, track, w_pos=(1e6,) * 3, w_term=(1e6,) * 3, w_du=(1.0,) * 3, origin=1)
    assert float(Cs[0]) <= 1e6 * 6 * N * (2.0 ** -53) ** 2
    assert b[0] > 0
    # one metre off on x: N + 1 squared metres with unit weights
    Cs, _ = nr.nav_cost_ref(P0, U, 0, c, track + [1.0, 0, 0], w_pos=(1.0,) * 3, w_term=(1.0,) * 3, origin=1)
    assert abs(float(Cs[0]) - (N + 1)) < 1e-9


def test_track_row_clamps_and_wraps():
    Tr = 5
    assert [nr.track_row(0, 3, n, Tr) for n in (1, 2, 3, 4, 5)] == [0, 0, 0, 1, 2]             # before the origin
    assert [nr.track_row(10, 3, n, Tr) for n in (1, 2)] == [4, 4]                               # past the end
    assert nr.track_row(2, 2 ** 64 - 1, 1, Tr) == 4                                             # step - origin wraps to +3
    assert nr.track_row(2 ** 64 - 2, 1, 1, Tr) == 0                                             # ... to -3, read as signed
    assert nr.track_row(2 ** 63, 0, 1, Tr) == 0 and nr.track_row(2 ** 63 - 1, 0, 1, Tr) == 4    # the sign boundary
    # the reference reads the rows it says it reads
    U = np.zeros((1, 3, 3))
    track = np.arange(15.0).reshape(5, 3)
    for step, origin, rows in ((0, 3, (0, 0, 0)), (4, 3, (2, 3, 4)), (9, 3, (4, 4, 4)), (1, 2 ** 64 - 1, (3, 4, 4))):
        Cs, _ = nr.nav_cost_ref(np.zeros(3), U, step, c, track, w_pos=(1, 0, 0), origin=origin)
        assert float(Cs[0]) == sum(track[r, 0] ** 2 for r in rows), (step, origin)


def test_single_node_has_no_rate_term():
    U = np.array([[[100.0, 200.0, -50.0]]])
    Cs, b = nr.nav_cost_ref(np.zeros(3), U, 0, c, np.zeros((1, 3)), w_du=(5.0,) * 3)
    assert Cs[0] == 0 and b[0] == 0
    U2 = np.array([[[100.0, 200.0, -50.0], [101.0, 198.0, -50.0]]])
    Cs, _ = nr.nav_cost_ref(np.zeros(3), U2, 0, c, np.zeros((1, 3)), w_du=(5.0,) * 3)
    assert float(Cs[0]) == 5.0 * (1 + 4)


def test_sphere_touched_on_its_boundary_costs_nothing():
    # the path runs along x from the origin; a sphere of radius 1 centred one radius off the path touches it at P_2
    N, step_len = 4, 1.0
    U = np.tile([step_len / c, 0.0, 0.0], (1, N, 1))
    P2 = float(nr.path(np.zeros(3), U[0], c)[1][0])
    Cs, _ = nr.nav_cost_ref(np.zeros(3), U, 0, c, np.zeros((1, 3)), w_sphere=10.0, spheres=[[P2, 1.0, 0.0, 1.0]])
    assert Cs[0] == 0
    Cs, _ = nr.nav_cost_ref(np.zeros(3), U, 0, c, np.zeros((1, 3)), w_sphere=10.0, spheres=[[P2, 0.75, 0.0, 1.0]])
    assert abs(float(Cs[0]) - 10.0 * 0.25 ** 2) < 1e-9       # only P_2 is inside: its neighbours are 1.25 away


def test_struct_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "rovmpc.h")).read()
    body = re.search(r"typedef struct rovmpc_nav_cost \{(.*?)\} rovmpc_nav_cost;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.sub(r"\[.*", "", d.strip()) for stmt in body.split(";") if stmt.strip()
             for d in re.sub(r"^\s*(int32_t|uint64_t|double)\s+", "", stmt.strip()).split(",")]
    assert names == [f[0] for f in _lib.NavCost._fields_]
    assert C.sizeof(_lib.NavCost) == 8 + 8 * 10 + 8 * 32 + 8
    assert int(re.search(r"#define ROVMPC_NAV_MAX_SPHERES (\d+)", hdr).group(1)) == _lib.NAV_MAX_SPHERES


BAD = [
    dict(w_pos=-1.0), dict(w_pos=(1.0, np.nan, 0.0)), dict(w_term=np.inf), dict(w_du=(0.0, 0.0)), dict(w_du=(0.0, 0.0, -1e-300)),
    dict(w_sphere=-0.5), dict(w_sphere=np.nan),
    dict(spheres=np.zeros((9, 4))), dict(spheres=[[0.0, 0.0, 0.0, -1.0]]), dict(spheres=[[0.0, np.inf, 0.0, 1.0]]),
    dict(spheres=[[0.0, 0.0, 1.0]]), dict(origin=1.5),
    dict(track=[[0.0, np.nan, 0.0]]), dict(track=np.zeros((4, 2))), dict(track=np.zeros(3)), dict(track=np.zeros((0, 3))),
    dict(track=np.zeros((2, 2, 2, 3))),
]


@pytest.mark.parametrize("kw", BAD, ids=[next(iter(k)) + str(i) for i, k in enumerate(BAD)])
def test_bad_arguments_raise_before_the_library_is_called(kw, monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load_library", no_library)
    kw = dict(kw)
    track = kw.pop("track", np.zeros((3, 3)))
    with pytest.raises(ValueError):
        _lib.nav_cost(track, **kw)
    with pytest.raises(ValueError):
        rovmpc.NavCost(track, **kw)


def test_navcost_fills_the_struct():
    nav = rovmpc.NavCost(np.arange(6.0).reshape(2, 3), w_pos=2.0, w_term=(1.0, 2.0, 3.0), w_sphere=4.0,
                         spheres=[[1.0, 2.0, 3.0, 0.5]], origin=-1)
    n = nav.c_nav
    assert n.struct_size == C.sizeof(_lib.NavCost) and n.n_spheres == 1 and n.origin == 2 ** 64 - 1
    assert list(n.w_pos) == [2.0] * 3 and list(n.w_term) == [1.0, 2.0, 3.0] and list(n.w_du) == [0.0] * 3 and n.w_sphere == 4.0
    assert list(n.spheres[0]) == [1.0, 2.0, 3.0, 0.5]
    assert nav.tracks.shape == (1, 2, 3) and nav.tracks.flags.c_contiguous and nav.spheres.shape == (1, 4)
    assert rovmpc.NavCost(np.zeros((3, 5, 3))).tracks.shape == (3, 5, 3)


def test_controllers_check_the_track_count_before_an_engine_exists(monkeypatch):
    from rovmpc import mpc

    def no_engine(*a, **k):
        raise AssertionError("an engine was made")
    monkeypatch.setattr(mpc, "Engine", no_engine)
    three = rovmpc.NavCost(np.zeros((3, 5, 3)))
    with pytest.raises(ValueError):
        rovmpc.MPPI(N=4, K=8, nav=three)
    with pytest.raises(ValueError):
        rovmpc.CEM(N=4, K=8, nav=three)
    with pytest.raises(ValueError):
        rovmpc.BatchedMPPI(B=2, N=4, K=8, nav=three)
    with pytest.raises(ValueError):
        rovmpc.BatchedCEM(B=4, N=4, K=8, nav=three)
    with pytest.raises(TypeError):
        rovmpc.MPPI(N=4, K=8, nav=np.zeros((5, 3)))
