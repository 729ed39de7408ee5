"""The launch plans that off-table image shapes reach (tools/offtable_plan_sweep.py), on the host: the committed fixture
tests/golden/offtable_conv_problems.json is exactly what the sweep gives with today's planner (a planner change forces a
conscious refresh with `python tools/offtable_plan_sweep.py --write`), every plan signature the sweep reaches is either
one the plan table's own pairs show (tests/test_gpu_plan_table.py runs those) or has a representative in the fixture
(tests/test_gpu_offtable_plans.py runs those), the enumeration gives back each config's table problems at its benchmark
frame, and the read-only plan query agrees with the two older queries on every swept problem. No GPU."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("offtable_plan_sweep", os.path.join(ROOT, "tools", "offtable_plan_sweep.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def tool():
    return _tool()


@pytest.fixture(scope="module")
def result(tool):
    return tool.sweep()


def test_enumeration_reproduces_the_table_at_the_benchmark_frames(tool):
    import __graft_entry__ as g
    g.build()
    counts = tool.self_check()
    assert len(counts) == 4 and all(n > 0 for n in counts.values()), counts


def test_fixture_is_what_the_sweep_gives(tool, result):
    committed = json.load(open(tool.FIXTURE))
    fresh = json.loads(json.dumps(tool.fixture_of(result)))
    assert fresh["counts"] == committed["counts"], "planner changed: python tools/offtable_plan_sweep.py --write"
    assert fresh == committed, "planner changed: python tools/offtable_plan_sweep.py --write"


def test_every_reached_signature_is_covered_or_represented(tool, result):
    left_out = [s for s in result["reached"] if s not in result["covered"] and s not in result["representatives"]]
    assert len(left_out) == 0, left_out[:5]
    assert len(result["reached"]) > 0 and len(result["queried"]) > 1000
    for sig, (prob, mode) in result["representatives"].items():
        assert sig not in result["covered"] and sig[0] == mode
        # the representative is the cheapest problem with its signature
        assert tool.macs(prob) == min(tool.macs(p) for p, m, s, _ in result["queried"] if s == sig)
    # the table's problems at the benchmark frames are part of the sweep: all their signatures count as covered
    table = tool.table_problems()
    swept_table = {s for p, m, s, _ in result["queried"] if p in table and m in table[p]}
    assert swept_table and swept_table <= result["covered"]


def test_plan_query_agrees_with_tile_config_and_num_dispatches(result):
    assert result["queried"]
    for prob, mode, sig, (code, cfg, disp, nd, tail_rows) in result["queried"]:
        assert code == cfg, (prob, mode, code, cfg)
        assert disp == nd, (prob, mode, disp, nd)
        if sig[1] == "direct" and mode != 2:
            assert (nd == 2) == (tail_rows > 0), (prob, mode, nd, tail_rows)
