"""The host-side layout of the step plan against tests/golden/plan_layout.json (tests/helpers/plan_layout_dump.py): sizes, the tensor
table, the gradient buckets and every view of thirteen configurations, exactly.  Host only: nothing is dereferenced."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import plan_layout_dump as D  # noqa: E402

with open(D.GOLDEN) as f:
    GOLDEN = json.load(f)


def test_the_fixture_covers_every_configuration():
    assert sorted(GOLDEN) == sorted(c["name"] for c in D.CONFIGS)


@pytest.mark.parametrize("cfg", D.CONFIGS, ids=lambda c: c["name"])
def test_plan_layout_matches_the_golden(cfg):
    got = json.loads(json.dumps(D.layout_of(cfg)))          # (tuples -> lists, as the file has them)
    want = GOLDEN[cfg["name"]]
    assert got["sizes"] == want["sizes"]
    assert got["tensors"] == want["tensors"]
    assert got["grad_buckets"] == want["grad_buckets"]
    assert sorted(got["views"]) == sorted(want["views"])
    for name in want["views"]:
        assert got["views"][name] == want["views"][name], name
