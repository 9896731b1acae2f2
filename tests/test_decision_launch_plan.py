"""DecisionPicture's launch plan, launch for launch, against the record kept in tests/golden/decision_launch_plan.json (tests/launch_plan_tools.py: a recording
stand-in for the Havoc context -- no device).  The step after the searches is a captured graph: a launch that moves, an argument, a byte of a job table or the aliasing
of two buffers that changes is a change of what the device runs, and shows here as the first launch that differs.  The check is exact.

The configurations are the smallest pictures that reach every branch of the tables: 56 x 56 holds units of 32, 16 and 8; 136 x 72 is 3 x 2 CTUs cut by both edges.
"""
import json

import pytest

import launch_plan_tools as T

pytestmark = pytest.mark.skipif(not T.library_built(), reason="libhavoc_mi355x.so is not built (its host entry points size the workspaces)")


@pytest.fixture(scope="module")
def golden():
    with open(T.GOLDEN) as f:
        return json.load(f)


def test_golden_holds_every_configuration(golden):
    assert sorted(golden) == sorted(T.CONFIGS)


@pytest.mark.parametrize("name", list(T.CONFIGS))
def test_launch_plan_is_the_recorded_one(golden, name):
    got = T.record(name)
    assert len(got["names"]) > 0
    assert T.first_difference(got, golden[name]) is None
    assert got == golden[name]


def test_record_does_not_depend_on_the_run():
    assert T.record("tree_rates_56x56") == T.record("tree_rates_56x56")
