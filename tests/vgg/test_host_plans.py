"""The launch plans of the Faster R-CNN VGG-16 configuration (tools/vgg16_plan_sweep.py), on the host: the committed fixture
tests/golden/vgg16_conv_problems.json is exactly what the sweep gives with today's planner and today's model (a change of
either forces a conscious refresh with `python tools/vgg16_plan_sweep.py --write`), every plan signature the sweep reaches
is one the plan table's pairs or the off-table fixture show (tests/test_gpu_plan_table.py and
tests/test_gpu_offtable_plans.py run those) or is in one of the fixture's two lists (tests/vgg/test_gpu_fullsize_plans.py
runs those), each representative is the cheapest problem of its signature, the read-only plan query agrees with the two
older queries on every swept pair, and the two problems no other configuration comes near — the 3-channel first
convolution on the VALU fallback and the 25 088-term FC reductions — are in the production list. No GPU."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _tool():
    spec = importlib.util.spec_from_file_location("vgg16_plan_sweep", os.path.join(ROOT, "tools", "vgg16_plan_sweep.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def tool():
    return _tool()


@pytest.fixture(scope="module")
def result(tool):
    return tool.sweep()


def test_fixture_is_what_the_sweep_gives(tool, result):
    committed = json.load(open(tool.FIXTURE))
    fresh = json.loads(json.dumps(tool.fixture_of(result)))
    assert fresh["counts"] == committed["counts"], "planner or model changed: python tools/vgg16_plan_sweep.py --write"
    assert fresh == committed, "planner or model changed: python tools/vgg16_plan_sweep.py --write"


def test_every_reached_signature_is_covered_or_listed(tool, result):
    prod_sigs = {rec[0] for rec in result["production"].values()}
    left_out = [s for s in result["reached"]
                if s not in result["covered"] and s not in prod_sigs and s not in result["representatives"]]
    assert len(left_out) == 0, left_out[:5]
    # 84 frames x 2 batches x 2 freeze settings of ~50 pairs each, most of them shared between frames
    assert len(result["reached"]) > 0 and len(result["queried"]) > 1000
    assert {s for _, _, s, _ in result["queried"]} == result["reached"]
    for sig, (prob, mode) in result["representatives"].items():
        assert sig not in result["covered"] and sig not in prod_sigs and sig[0] == mode
        assert (prob, mode) not in result["production"]
        # the representative is the cheapest problem with its signature
        assert tool.macs(prob) == min(tool.macs(p) for p, m, s, _ in result["queried"] if s == sig)
    # the production pairs are part of the sweep
    swept = {(p, m): s for p, m, s, _ in result["queried"]}
    for (prob, mode), (sig, freeze, names) in result["production"].items():
        assert swept[(prob, mode)] == sig and sig[0] == mode
        assert freeze and set(freeze) <= set(tool.FREEZE_SETTINGS) and names


def test_plan_query_agrees_with_tile_config_and_num_dispatches(result):
    assert result["queried"]
    for prob, mode, sig, (code, cfg, disp, nd, tail_rows) in result["queried"]:
        assert code == cfg, (prob, mode, code, cfg)
        assert disp == nd, (prob, mode, disp, nd)
        if sig[1] == "direct" and mode != 2:
            assert (nd == 2) == (tail_rows > 0), (prob, mode, nd, tail_rows)


def test_production_list_is_one_step_at_the_benchmark_frame(tool, result):
    prod = result["production"]
    assert result["frames"][0] == tool.BENCH_FRAME == (600, 1024)
    # the image-level problems are at batch 1 on the frame and its floor-halved levels 300x512, 150x256, 75x128, 37x64
    maps = {(p[1], p[2]) for p, _ in prod if p[1] > 1}
    assert maps == {(600, 1024), (300, 512), (150, 256), (75, 128), (37, 64)}, maps
    assert all(p[0] == 1 for p, _ in prod if p[1] > 1)
    # conv1_1 forward: the one shipped layer whose production plan is the VALU fallback's 3x3 on a whole frame
    conv1_1 = ((1, 600, 1024, 3, 64, 3, 3, 600, 1024, 1, 1, 1, 1), 0)
    assert conv1_1 in prod and prod[conv1_1][0][1] == "valu_fallback", prod.get(conv1_1)
    assert set(prod[conv1_1][1]) == set(tool.FREEZE_SETTINGS) and prod[conv1_1][2][0].endswith("conv1/conv1_1")
    # the FC layers on the flattened 7x7x512 crops: 25 088-term reductions, in all three modes
    fc = {m for p, m in prod if p[3] == 25088 and p[4] == 4096 and p[5:9] == (1, 1, 1, 1)}
    assert fc == {0, 1, 2}, fc
    # freeze_layer 'conv2' trains conv3 and above: conv1 / conv2 forward only, conv3_1 without a dgrad; '' adds the rest
    def modes_of(scope_end, fz):
        return {m for (p, m), (s, freeze, names) in prod.items() if fz in freeze and any(n.endswith(scope_end) for n in names)}
    for name in ("conv1_1", "conv1_2", "conv2_1", "conv2_2"):
        assert modes_of(name, "conv2") == {0}, name
    assert modes_of("conv3_1", "conv2") == {0, 2} and modes_of("conv3_2", "conv2") == {0, 1, 2}
    assert modes_of("conv1_1", "") == {0, 2} and modes_of("conv1_2", "") == {0, 1, 2}
    assert modes_of("conv3_1", "") == {0, 1, 2}
    # the refiner's window pass is forward only: its 4 * 64 + 8 rows never reach a dgrad or a wgrad
    rows = tool.refiner_window_rois(tool.load_models()["conv2"][1])
    assert rows == 264 and {m for p, m in prod if p[0] == rows} == {0}
