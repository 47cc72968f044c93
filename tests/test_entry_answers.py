"""CPU: the 26 workspace queries and 29 run entries of the k-means and few-shot methods answer what they answered before their
host drivers were folded onto one check path per method.  tests/golden/method_entry_answers.json was recorded once from the
library of the commit before that change (tests/helpers/entry_answers.py, loaded through TCLIP_LIB) and is never regenerated.

Queries: the size, or the refusal's message, for every problem of the grid.  Run entries: code and message of every single
fault; for two faults at once the code, and a message that is the recorded one or the one either fault gives alone - the order
of a method's checks is one order for all its call forms now, and this is the whole freedom it gets.  The two-fault cases that
use it are counted per method and printed.  Every call is refused before any HIP call, so none needs a GPU."""
import itertools
import json
import os

import pytest

from conftest import GOLDEN
from helpers import entry_answers as ea
from tclip_amd import _capi

with open(os.path.join(GOLDEN, "method_entry_answers.json")) as f:
    FIXTURE = json.load(f)
MESSAGES = FIXTURE["messages"]


def test_the_cases_cover_every_entry_and_query():
    entries = {n.split("|")[0] for n in ea.RUNS}
    assert len(entries) == 29 and len(ea.QUERIES) == 26 and len(ea.METHODS) == 10
    assert entries | set(ea.QUERIES) <= set(_capi.EXPORTS)
    stems = ("soft_kmeans", "em_gaussian", "hard_kmeans", "kl_kmeans", "kmeans_visual", "paddle", "bdcspn", "alpha_tim", "tim_gd",
             "laplacian_shot")
    assert entries == {e for e in _capi.EXPORTS if e.startswith(tuple("tclip_" + s for s in stems)) and not e.endswith("_bytes")}
    assert sorted(FIXTURE["runs"]) == sorted(ea.RUNS) and sorted(FIXTURE["queries"]) == ea.QUERIES
    for name in ea.RUNS:
        assert len(_capi._SIGNATURES[name.split("|")[0]][1]) == 1 + len(ea.RUNS[name][2].split()), name
        assert FIXTURE["runs"][name]["faults"] == [f[0] for f in ea.faults(name)], name


@pytest.mark.parametrize("query", ea.QUERIES)
def test_queries(query):
    lib = _capi.lib()
    grid, want = ea.query_grid(query), FIXTURE["queries"][query]
    assert len(grid) == len(want)
    for moves, w in zip(grid, want):
        assert ea.ask(lib, query, moves) == (w if w > 0 else MESSAGES[-1 - w]), moves


@pytest.mark.parametrize("method", ea.METHODS)
def test_run_entries(method):
    lib = _capi.lib()
    freedom = cases = 0
    for name in (n for n in ea.RUNS if ea.RUNS[n][0] == method):
        fl, rec = ea.faults(name), FIXTURE["runs"][name]
        alone = {}
        for (what, m), (rc, text) in zip(fl, rec["single"]):
            assert ea.call(lib, name, [m]) == (rc, MESSAGES[text]), (name, what)
            alone[what] = MESSAGES[text]
        for (a, b), (rc, text) in zip(itertools.combinations(fl, 2), rec["pairs"]):
            got = ea.call(lib, name, [a[1], b[1]])
            assert got[0] == rc, (name, a[0], b[0], got)
            assert got[1] in (MESSAGES[text], alone[a[0]], alone[b[0]]), (name, a[0], b[0], got)
            freedom += got[1] != MESSAGES[text]
            cases += 1
    print(f"{method}: {freedom} of {cases} two-fault cases report the other fault than the recording")
