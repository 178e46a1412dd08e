"""rovmpc_discover_rows without a GPU: the header and the library's exports, the params mirror and its defaults, the enum, the
refusals that need no handle (a handle needs a device: the refusals of the entries themselves, with their messages, are in
tests/test_discover_gpu.py), term_library, and the texts of a RowFront compiled back."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rovmpc
from rovmpc import _lib, scoring
from rovmpc.expr import compile_expression

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "rovmpc.h")).read()


def test_header_declares_both_entries_and_the_library_exports_them():
    hdr = _header()
    declared = set(re.findall(r"\b(rovmpc_[a-z_0-9]+)\s*\(", hdr))
    lib = rovmpc.load_library()
    for name in ("rovmpc_discover_rows", "rovmpc_discover_rows_device", "rovmpc_default_discover_params"):
        assert name in declared and name in rovmpc.exported_symbols() and hasattr(lib, name), name
    for phrase in ("forward orthogonal least squares", "one fused multiply-add per row", "lowest j on ties", "loss comes by subtraction",
                   "not of G, B, T, the group's place in the call, or the entry"):
        assert phrase in hdr, phrase
    define = lambda n: int(re.search(r"#define %s (\d+)" % n, hdr).group(1))
    assert define("ROVMPC_DISCOVER_MAX_TERMS") == _lib.DISCOVER_MAX_TERMS == 64
    assert define("ROVMPC_DISCOVER_MAX_SIZE") == _lib.DISCOVER_MAX_SIZE == define("ROVMPC_REFIT_MAX_PARAMS") == 8
    assert define("ROVMPC_DISCOVER_CHUNK") == _lib.DISCOVER_CHUNK == 1024
    assert len(lib.rovmpc_discover_rows.argtypes) == len(lib.rovmpc_discover_rows_device.argtypes) == 20


def test_params_mirror_size_and_defaults():
    body = re.search(r"typedef struct rovmpc_discover_params \{(.*?)\} rovmpc_discover_params;", _header(), re.S).group(1)
    fields = re.findall(r"^\s*(int32_t|double)\s+([a-z_]+)\s*;", body, re.M)
    assert [f[1] for f in fields] == [n for n, _ in _lib.DiscoverParams._fields_] == ["struct_size", "max_terms", "dep_tol", "min_gain"]
    assert C.sizeof(_lib.DiscoverParams) == sum({"int32_t": 4, "double": 8}[t] for t, _ in fields) == 24
    p = _lib.DiscoverParams()
    rovmpc.load_library().rovmpc_default_discover_params(C.byref(p))
    assert (p.struct_size, p.max_terms, p.dep_tol, p.min_gain) == (24, 8, 1e-10, 1e-12)
    q = _lib.DiscoverParams.make()
    assert bytes(p) == bytes(q)
    assert rovmpc.DiscoverParams is _lib.DiscoverParams
    rovmpc.load_library().rovmpc_default_discover_params(None)                  # (a null pointer is ignored)


def test_enum_matches_the_header():
    body = re.search(r"typedef enum rovmpc_discover_status \{(.*?)\} rovmpc_discover_status;", _header(), re.S).group(1)
    values = {n: int(v) for n, v in re.findall(r"ROVMPC_DISCOVER_([A-Z_]+) = (\d+)", body)}
    assert values == {m.name: int(m) for m in rovmpc.DiscoverStatus} == {"FULL": 0, "MIN_GAIN": 1, "EXHAUSTED": 2, "NONFINITE": 3}


def test_refusals_that_need_no_handle(monkeypatch):
    lib = rovmpc.load_library()
    for entry in (lib.rovmpc_discover_rows, lib.rovmpc_discover_rows_device):
        assert entry(None, *[None] * 4, 1, None, 1, None, 1, 1, None, None, 1, None, *[None] * 5) == -1
    for kw in (dict(max_terms=0), dict(max_terms=9), dict(max_terms=2.5), dict(max_terms=True), dict(dep_tol=-1e-300), dict(dep_tol=float("nan")),
               dict(min_gain=-1.0), dict(min_gain=float("nan"))):
        with pytest.raises(ValueError):
            _lib.DiscoverParams.make(**kw)

    def no_engine():
        raise AssertionError("the engine was created before the check")
    from rovmpc import engine
    monkeypatch.setattr(engine, "default_engine", no_engine)
    X, g = np.zeros((2, 5, 3)), np.zeros((2, 5))
    for args, kw in ((([], X, g), {}), ((["x0"] * 65, X, g), {}), (("x0", X, g), {}), ((["x0"], X, None), {}), ((["x3"], X, g), {}),
                     ((["x0"], X, g[:, :4]), {}), ((["x0"], X, g), dict(max_terms=9)), ((["x0"], X, g), dict(dep_tol=-1.0)),
                     ((["x0"], X, g), dict(groups="some")), ((["x0"], X, g), dict(groups=[0, 1])), ((["x0"], X, g), dict(lengths=[5, 6])),
                     ((["x0"], np.zeros((2, 5, 33)), g), {})):
        with pytest.raises(ValueError):
            rovmpc.discover_rows(*args, **kw)


def test_term_library_counts_order_and_refusal():
    lib = rovmpc.term_library(18)
    assert len(lib) == 55 and lib[0] == "1.0" and lib[1:19] == ["x%d" % i for i in range(18)]
    assert lib[19:37] == ["sin(x%d)" % i for i in range(18)] and lib[37:] == ["cos(x%d)" % i for i in range(18)]
    assert rovmpc.term_library(2, unary=("cos", "id"), intercept=False, products=[(0, 1), (1, 1)]) == ["cos(x0)", "cos(x1)", "x0", "x1", "x0*x1", "x1*x1"]
    assert rovmpc.term_library(2, unary=("id",), variable_names=["th", "ga"], products=[(0, 1)]) == ["1.0", "th", "ga", "th*ga"]
    assert len(rovmpc.term_library(18, products=[(i, i) for i in range(9)])) == 64
    for text in lib:
        compile_expression(text, [], 18)
    with pytest.raises(ValueError, match="at most 64"):
        rovmpc.term_library(18, products=[(i, i) for i in range(10)])
    with pytest.raises(ValueError, match="at most 64"):
        rovmpc.term_library(32)
    for bad in (dict(F=0), dict(F=33), dict(F=3, unary=("sinh",)), dict(F=3, products=[(0, 3)]), dict(F=3, variable_names=["a"])):
        with pytest.raises(ValueError):
            rovmpc.term_library(**bad)


def test_row_front_texts_compile_back_to_the_returned_coefficients():
    terms = rovmpc.term_library(18)
    picks = np.array([[22, 17, 36, 4], [3, -1, -1, -1]], np.int32)
    coef = np.zeros((2, 4, 4))
    coef[0] = np.tril(np.array([[-0.0481, 0, 0, 0], [-0.048, -1.5e-300, 0, 0], [0.25, 0.25, -0.1, 0], [1 / 3, -2 / 3, 5e300, 1e-5]]))
    coef[1, 0, 0] = -7.0
    n_sel = np.array([4, 1])
    texts, counts = scoring._front_texts(picks, coef, n_sel, terms, 18, None)
    assert [len(t) for t in texts] == [4, 1] and texts[1] == ["-7.0*(x2)"]
    assert texts[0][1] == "-0.048*(sin(x3)) + -1.5e-300*(x16)"
    for g in range(2):
        for s, text in enumerate(texts[g]):
            pool = []
            prog = compile_expression(text, pool, 18)
            assert sorted(set(pool)) == sorted(set(coef[g, s, :s + 1])), text          # (equal coefficients share a pool slot)
            assert len(prog.code) == counts[g][s]
            assert sorted(prog.features_used) == sorted({(int(p) - 1) % 18 for p in picks[g, :s + 1]})
    front = rovmpc.RowFront(picks, coef, np.array([[1.0, 0.5, 0.25, 0.1, 0.05], [2.0, 1.0] + [np.nan] * 3]), n_sel, np.array([0, 1]),
                            np.array([200, 200]), tuple(terms), None, texts, counts)
    rows = front.rows(0)
    assert [set(r) for r in rows] == [{"complexity", "loss", "equation", "sympy_format"}] * 4
    assert [r["loss"] for r in rows] == [0.5, 0.25, 0.1, 0.05] and [r["complexity"] for r in rows] == counts[0]
    assert [scoring.row_text(r) for r in rows] == texts[0] and len(front.rows(1)) == 1
    assert "not pysr's complexity" in " ".join(rovmpc.RowFront.rows.__doc__.lower().split())
    # a front that cannot be written as text names the size
    bad = coef.copy(); bad[0, 2, 1] = np.inf
    with pytest.raises(ValueError, match="size-3 row of group 0"):
        scoring._front_texts(picks, bad, n_sel, terms, 18, None)
    deep = "x0"
    for i in range(1, 40):
        deep = "x%d - (%s)" % (i % 18, deep)
    with pytest.raises(ValueError, match="size-1 row"):
        scoring._front_texts(np.array([[0]], np.int32), np.ones((1, 1, 1)), np.array([1]), [deep], 18, None)
