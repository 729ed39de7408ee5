"""Integrity of the committed plan table (mtl_ssl_amd/conv_plans.json): every key is a descriptor the model can build,
every value a plan code the library knows, and a pinned code takes effect through the path production uses
(ops._autotune on the first call of a (problem, mode)). A stale or hand-edited entry fails here, on a CPU, instead of
silently running the planner's choice on the GPU. tests/test_gpu_plan_table.py runs the same entries on an MI355X."""
import ctypes
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_FILE = os.path.join(ROOT, "mtl_ssl_amd", "conv_plans.json")


def _table():
    return json.load(open(PLAN_FILE))["plans"]


def _parse(key):
    vals = tuple(int(v) for v in key.split(","))
    assert len(vals) == 14 and ",".join(str(v) for v in vals) == key, key
    return vals


@pytest.fixture(scope="module")
def ops():
    from mtl_ssl_amd import ops
    return ops


def test_table_covers_the_four_configs():
    keys = [_parse(k) for k in _table()]
    assert len(keys) == 359
    assert len({k[1:] for k in keys}) == 150


def test_keys_and_values_are_well_formed(ops):
    for key, val in _table().items():
        mode = _parse(key)[0]
        assert mode in (0, 1, 2), key
        assert isinstance(val, int) and (val == -1 or val in ops.PLAN_CODES), (key, val)


def test_every_key_is_a_descriptor_conv_desc_builds(ops):
    """The key is exactly ops._plan_key of what ops.conv_desc makes for SAME, VALID or RESNET_SAME padding: a key with
    a wrong output size or pad can never match a call, and its pin would be dead."""
    for key in _table():
        mode, N, H, W, C, K, R, S, OH, OW, stride, dil, pt, pl = _parse(key)
        assert min(N, H, W, C, K, R, S, OH, OW, stride, dil) >= 1 and min(pt, pl) >= 0, key
        built = [ops._plan_key(ops.conv_desc((N, H, W, C), (R, S, C, K), stride, dil, pad), mode)
                 for pad in ("SAME", "VALID", "RESNET_SAME")]
        assert _parse(key) in built, (key, built)


def test_pinned_winograd_codes_only_on_3x3_stride1_problems(ops):
    for key, val in _table().items():
        if val >= 0 and ops.plan_code_algorithm(val) in (1, 2):
            mode, N, H, W, C, K, R, S, OH, OW, stride, dil, pt, pl = _parse(key)
            assert (R, S, stride, dil) == (3, 3, 1, 1), (key, val)


def test_pinned_codes_take_effect_through_the_first_call_path(ops):
    """ops._autotune is what the first conv2d_fwd / _dgrad / _wgrad call of a (problem, mode) runs; with the on-line
    tuner off it hands a pinned code to the library's plan registry. Host-side planning only (no launch), so this runs
    without a GPU. The plan a -1 entry keeps must be a code the library reports for the problem."""
    import __graft_entry__ as g
    g.build()
    from mtl_ssl_amd.lib import ConvDesc, lib
    ops.reset_tuning(use_plan_db=True, autotune=False)
    try:
        for key, val in _table().items():
            vals = _parse(key)
            mode, d = vals[0], ConvDesc(*vals[1:], 0)
            ops._autotune(d, mode, None)        # the tuner is off: the run callback is never used
            got = lib().conv2d_tile_config(ctypes.byref(d), mode)
            if val >= 0:
                assert got == val, (key, val, got)
            else:
                assert got == -1 or got in ops.PLAN_CODES, (key, got)
    finally:
        ops.reset_tuning()
