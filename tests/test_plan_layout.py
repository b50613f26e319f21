"""The plan's host-side layout against tests/golden/plan_layout.json (tests/golden/gen/make_plan_layout.py): parameter names, numels
and order, workspace and mask sizes, DropPath call count, logits layout and the backward segment of every parameter, for every
configuration of tests/plan_layout_cases.py.  Integers only: equality, no tolerance.  No GPU."""
import json
import os

import pytest

from tests.plan_layout_cases import CONFIGS, measure

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_layout.json")


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_holds_exactly_the_configurations(golden):
    assert sorted(golden) == sorted(CONFIGS)
    assert "params" in golden["base"]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_plan_layout(golden, name):
    assert name in golden, f"{name} is missing from {FIXTURE}"
    got, want = measure(name), golden[name]
    assert sorted(got) == sorted(want)
    for key in want:  # key by key: a failure names the value that moved
        assert got[key] == want[key], (name, key)


def test_segments_partition_the_parameters(golden):
    for name, g in golden.items():
        assert sorted(i for seg in g["segments"] for i in seg) == list(range(g["num_params"])), name
