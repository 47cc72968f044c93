"""CPU: what the task-batch loops (Evaluator_zero_shot, Evaluator_few_shot) hand to the engine, pinned call by call.  Which
engine function a (method, feature kind, options) triple reaches - the tables in place, the fused task builder or the gathered
and relabelled tensors -, with which rows, labels and parameter, on which rank, in how many groups, from which method object,
and what is logged, returned, left behind and written, is replayed against recording stubs (tests/helpers/evaluator_trace.py) and
compared with tests/golden/evaluator_call_traces.json.  The fixture was recorded once, before the two evaluators were folded
onto one shared base, and is never regenerated."""
import json
import os

import pytest

from conftest import GOLDEN
from helpers import evaluator_trace

with open(os.path.join(GOLDEN, "evaluator_call_traces.json")) as f:
    TEXT = f.read()
FIXTURE = json.loads(TEXT)
NAMES = [name for name, _ in evaluator_trace.cases()]


@pytest.fixture(scope="module")
def recording():
    """every case, replayed once for the whole module"""
    return evaluator_trace.record(pytest.MonkeyPatch())


def test_the_cases_are_the_recorded_ones():
    assert sorted(NAMES) == sorted(FIXTURE["cases"]) and len(set(NAMES)) == len(NAMES)
    ran = {n for n, c in FIXTURE["cases"].items() if "returned" in c}
    for method in evaluator_trace.ZERO_SHOT:
        assert f"zero {method} softmax" in ran
    for method, feat in evaluator_trace.FEW_SHOT:
        for route in ("", " materialise_tasks=True", " in_place_support=True", " in_place_loop=True"):
            for per_call in (0, 1, 2):
                assert f"few {method} {feat}{route} batches_per_call={per_call}" in ran
    assert os.path.getsize(os.path.join(GOLDEN, "evaluator_call_traces.json")) < os.path.getsize(os.path.join(GOLDEN, "engine_call_traces.json"))


def test_public_names_and_signatures():
    assert evaluator_trace.public_surface() == FIXTURE["public"]


@pytest.mark.parametrize("case", NAMES)
def test_case(case, recording):
    got = evaluator_trace.expand(recording["cases"][case], recording["pool"])
    want = evaluator_trace.expand(FIXTURE["cases"][case], FIXTURE["pool"])
    for part in sorted(set(got) | set(want)):
        assert got.get(part) == want.get(part), part


def test_recording_is_the_fixture_byte_for_byte(recording):
    assert evaluator_trace.dumps(recording) == TEXT
