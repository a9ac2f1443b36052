"""What the library enqueues for one eager pass against tests/golden/step_launches.json (tests/helpers/step_launch_dump.py): per case and
operation the rows of dmvae_prof_collect -- names, launch counts and order exactly; flops and bytes are host-computed doubles from the same
integer shapes, so exactly too.  A change that alters the launch structure on purpose regenerates the file and shows the diff."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import step_launch_dump as D  # noqa: E402

pytestmark = pytest.mark.gpu

with open(D.GOLDEN) as f:
    GOLDEN = json.load(f)


def test_the_fixture_covers_every_case():
    assert sorted(GOLDEN) == sorted(c["name"] for c in D.CASES)


@pytest.mark.parametrize("case", D.CASES, ids=lambda c: c["name"])
def test_step_launches_match_the_golden(case):
    import torch
    torch.cuda.set_device(0)
    got = json.loads(json.dumps(D.run_case(case)))
    want = GOLDEN[case["name"]]
    assert [op for op, _ in got] == [op for op, _ in want]
    for (op, rows), (_, wrows) in zip(got, want):
        assert [r[:3] for r in rows] == [r[:3] for r in wrows], "%s: names / launches / kernel launches, in order" % op
        assert rows == wrows, "%s: flops / bytes" % op
