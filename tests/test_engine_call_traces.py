"""CPU: what engine.py hands to libtclip.so, pinned call by call.  The few-shot families of engine.py (PADDLE, BD-CSPN,
LaplacianShot, ALPHA_TIM, TIM_GD, EM-Dirichlet; dense, table-fed and swept) are positional pointer lists of 10-14 entries that
ctypes cannot tell apart, so every call of their 24 public functions is replayed against a recording fake library
(tests/helpers/engine_trace.py) and compared with tests/golden/engine_call_traces.json: the ordered library calls with every
argument resolved to the input or output it points at, the type, text and order of every Python-level refusal (none may come
after an entry call), and the names, signatures and docstrings of engine's public surface.  The fixture was recorded once, before
the families were folded into one runner per method, and is never regenerated."""
import json
import os

import pytest

from conftest import GOLDEN
from helpers import engine_trace
from tclip_amd import engine

with open(os.path.join(GOLDEN, "engine_call_traces.json")) as f:
    FIXTURE = json.load(f)
CASES = {c[0]: c for c in engine_trace.cases()}
FUNCTIONS = {c[1] for c in CASES.values()}


def test_the_cases_cover_the_24_functions():
    swept = ("paddle", "bdcspn", "laplacian_shot", "alpha_tim")
    kinds = ("run_%s", "run_%s_visual", "run_%s_tasks", "run_%s_visual_tasks", "sweep_%s_tasks")
    assert FUNCTIONS == {k % m for m in swept for k in kinds} | {"run_tim_gd", "run_tim_gd_tasks", "run_em_dirichlet", "run_em_dirichlet_tasks"}
    assert len(FUNCTIONS) == 24 and FUNCTIONS <= set(FIXTURE["public"])
    assert sorted(CASES) == sorted(FIXTURE["traces"])
    with_cols = {fn for fn in FUNCTIONS if "cols" in FIXTURE["public"][fn]["signature"]}
    assert len(with_cols) == 10 and {fn + "+cols" for fn in with_cols if fn != "run_em_dirichlet_tasks"} <= set(CASES)
    for case in ("", "+support", "_tasks", "_tasks+cols", "_tasks+support", "_tasks+support+cols"):       # zero-shot and few-shot
        assert "run_em_dirichlet" + case in CASES


def test_public_surface():
    got = engine_trace.public_surface(engine)
    assert sorted(got) == sorted(FIXTURE["public"])
    for name in got:
        assert got[name] == FIXTURE["public"][name], name


@pytest.mark.parametrize("case", sorted(CASES))
def test_library_calls(case, monkeypatch):
    _, fn, width, tables, pos, kw, _ = CASES[case]
    rec = engine_trace.install(monkeypatch, engine)
    got = engine_trace.run(rec, engine, fn, engine_trace.inputs(width, tables), pos, dict(kw))
    assert got == FIXTURE["traces"][case]


def test_refusals(monkeypatch):
    """each refusal alone, and every pair of them: which comes first"""
    got = engine_trace.record(monkeypatch, engine)["refusals"]
    assert sorted(got) == sorted(FIXTURE["refusals"])
    for case in got:
        assert got[case] == FIXTURE["refusals"][case], case


def test_recording_is_the_fixture_byte_for_byte(monkeypatch):
    with open(os.path.join(GOLDEN, "engine_call_traces.json")) as f:
        assert engine_trace.dumps(engine_trace.record(monkeypatch, engine)) == f.read()
