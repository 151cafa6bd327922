"""The launch policy (word2vec_amd/csrc/device/w2v_policy.cpp) decides what it
decided before it was separated from the launch code: every case of
tests/policy_cases.py gives the plan recorded in tests/golden/launch_plans.json,
which was captured on the commit named there (its launch code carrying a
read-back of its locals) on an MI355X. Integers, the doubles and the float32
bit patterns of the flush scales are all compared for equality: the arithmetic
is double precision without contraction on both sides."""
import base64
import json
from pathlib import Path

import numpy as np
import pytest

from tests.policy_cases import CASES, run_case, to_json

GOLDEN = json.loads((Path(__file__).parent / "golden" / "launch_plans.json").read_text())


def test_golden_covers_the_case_matrix():
    assert sorted(GOLDEN["cases"]) == sorted(CASES)
    for name, c in CASES.items():
        assert GOLDEN["cases"][name]["params"] == json.loads(json.dumps(c)), name


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_launch_plan_equals_parent(name, monkeypatch):
    import torch

    assert torch.cuda.get_device_properties(0).multi_processor_count == GOLDEN["n_cu"]
    want = GOLDEN["cases"][name]["plan"]
    got = json.loads(json.dumps(to_json(run_case(name, monkeypatch.setenv))))
    assert sorted(got) == sorted(want)
    for k in sorted(want):
        if k in ("priv_sc", "ctx_sc") and got[k] != want[k]:  # which scales differ, and by how much
            g, w = (np.frombuffer(base64.b64decode(x[k]), "<f4") for x in (got, want))
            assert g.size == w.size, (name, k, g.size, w.size)
            bad = np.flatnonzero(g.view(np.uint32) != w.view(np.uint32))
            assert bad.size == 0, (name, k, bad[:8].tolist(), g[bad[:8]].tolist(), w[bad[:8]].tolist())
        assert got[k] == want[k], (name, k, got[k], want[k])
