"""CPU half of tests/footprint: the instrument's self-test on CPU tensors, and the coverage pin — every size query of the
C ABI has a guarded case in this sub-suite, so a sixteenth query fails here until it gets one."""
import ast
import os
import re

import pytest
import torch

from tests.footprint import guarded as G

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HERE = os.path.dirname(os.path.abspath(__file__))

# size query -> the tests of this sub-suite that run the launch it sizes inside a guarded buffer of exactly that size
COVERAGE = {
    "mtlssl_conv2d_workspace_bytes": ["test_gpu_conv_ops.py::test_every_plan_family_stays_inside_its_workspace",
                                      "test_gpu_conv_ops.py::test_store_mask_of_the_last_tile",
                                      "test_gpu_conv_ops.py::test_ksplit_forward_folds",
                                      "test_gpu_conv_ops.py::test_fp32_engine_modes_share_one_workspace_size",
                                      "test_gpu_conv_ops.py::test_strided_slice_of_a_guarded_wide_map"],
    "mtlssl_conv2d_wgrad_workspace_bytes": ["test_gpu_conv_ops.py::test_filter_gradient_families",
                                            "test_gpu_conv_ops.py::test_row_group_flags_keep_the_list_inside_the_workspace",
                                            "test_gpu_conv_ops.py::test_fp32_engine_modes_share_one_workspace_size"],
    "mtlssl_conv2d_wgrad_grouped_workspace_bytes": ["test_gpu_conv_ops.py::test_grouped_filter_gradient_three_problems"],
    "mtlssl_conv2d_filter_xf_bytes": ["test_gpu_conv_ops.py::test_kept_transforms_stay_inside_their_queries"],
    "mtlssl_conv2d_input_xf_bytes": ["test_gpu_conv_ops.py::test_kept_transforms_stay_inside_their_queries"],
    "mtlssl_depthwise_wgrad_workspace_bytes": ["test_gpu_conv_ops.py::test_depthwise_filter_gradient"],
    "mtlssl_bn_param_grads_workspace_bytes": ["test_gpu_conv_ops.py::test_bn_param_grads"],
    "mtlssl_rpn_proposals_workspace_bytes": ["test_gpu_detection.py::test_rpn_proposals"],
    "mtlssl_nms_workspace_bytes": ["test_gpu_detection.py::test_nms"],
    "mtlssl_batch_multiclass_nms_workspace_bytes": ["test_gpu_detection.py::test_batch_multiclass_nms"],
    "mtlssl_assign_targets_workspace_bytes": ["test_gpu_detection.py::test_assign_targets"],
    "mtlssl_roi_crop_pool_bwd_workspace_bytes": ["test_gpu_detection.py::test_roi_crop_pool_bwd"],
    "mtlssl_sgd_workspace_bytes": ["test_gpu_detection.py::test_sgd_momentum_clip"],
    "mtlssl_prepare_images_aug_workspace": ["test_gpu_detection.py::test_prepare_images_aug_with_a_contrast_and_a_pad_slot"],
    "mtlssl_variable_histograms_workspace_bytes": ["test_gpu_detection.py::test_variable_histograms"],
}


def _size_queries():
    text = open(os.path.join(ROOT, "include", "mtlssl_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = re.findall(r"\bint64_t\s+(mtlssl_\w+)\s*\(", text)
    return {n for n in names if re.search(r"_workspace_bytes$|_xf_bytes$|_workspace$", n)}


def test_every_size_query_has_a_guarded_case():
    queries = _size_queries()
    assert len(queries) >= 15
    assert queries == set(COVERAGE), ("size queries without a guarded case: %s; table entries without a query: %s"
                                      % (sorted(queries - set(COVERAGE)), sorted(set(COVERAGE) - queries)))
    # every test the table names exists, and its module really goes through the query's wrapper or the query itself
    defined = {}
    for mod in {t.split("::")[0] for ts in COVERAGE.values() for t in ts}:
        src = open(os.path.join(HERE, mod)).read()
        defined[mod] = ({n.name for n in ast.walk(ast.parse(src)) if isinstance(n, ast.FunctionDef)}, src)
    for query, tests in COVERAGE.items():
        assert tests, query
        for t in tests:
            mod, name = t.split("::")
            assert name in defined[mod][0], t
    for query in ("conv2d_wgrad_workspace_bytes", "conv2d_wgrad_grouped_workspace_bytes", "conv2d_filter_xf_bytes",
                  "conv2d_input_xf_bytes", "depthwise_wgrad_workspace_bytes", "bn_param_grads_workspace_bytes"):
        assert query + "(" in defined["test_gpu_conv_ops.py"][1], query
    for query in sorted(set(COVERAGE) - {q for q in COVERAGE if "conv2d" in q or "depthwise" in q or "bn_param" in q}):
        assert query[len("mtlssl_"):] + "(" in defined["test_gpu_detection.py"][1], query


def test_guard_band_geometry():
    assert G.GUARD_BYTES == 512 * 1024 == 2 * (256 * 256 * 4) and G.GUARD_BYTES % 256 == 0
    for nbytes in (0, 1, 3, 4, 1000, 4096):
        t = G.guarded(nbytes, torch.uint8, None, "cpu")
        g = t.guard
        assert t.numel() == nbytes and g.parent.numel() == nbytes + 2 * G.GUARD_BYTES
        assert nbytes == 0 or (t.is_contiguous() and t.data_ptr() == g.parent.data_ptr() + G.GUARD_BYTES and bool((t == 255).all()))
        # every aligned 32-bit word of both bands holds the pattern, compared as integers
        assert bool((g.lo().view(torch.int32) == G.PATTERN).all())
        start = (G.GUARD_BYTES + nbytes + 3) // 4 * 4
        hi = g.parent[start:start + (g.parent.numel() - start) // 4 * 4]
        assert bool((hi.view(torch.int32) == G.PATTERN).all())
    assert torch.isfinite(torch.tensor([G.PATTERN], dtype=torch.int32).view(torch.float32)).all()
    x = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    gx = G.guarded(None, fill=x, device="cpu")
    assert torch.equal(gx, x) and gx.is_contiguous()
    assert bool(torch.isnan(gx.guard.lo().view(torch.float32)).all()) and bool(torch.isnan(gx.guard.hi().view(torch.float32)).all())
    out = G.guarded((2, 5), torch.float32, float("nan"), "cpu")
    assert out.shape == (2, 5) and bool(torch.isnan(out).all()) and bool((out.guard.hi().view(torch.int32) == G.PATTERN).all())


def _three_handouts():
    gw = G.GuardedWorkspaces()
    bufs = [gw._hand_out(n, key, torch.device("cpu")) for n, key in ((1000, "a"), (4096, "b"), (7, "a"))]
    return gw, bufs


def test_an_untouched_set_passes_and_is_counted():
    gw, bufs = _three_handouts()
    for b in bufs:
        b.fill_(3)                                         # writing the whole payload is what a kernel may do
    gw.check()
    assert [(k, n) for k, n, _ in gw.handouts] == [("a", 1000), ("b", 4096), ("a", 7)]
    assert gw.stats == {"a": [2, 1007], "b": [1, 4096]} and gw.bytes_of("a") == [1000, 7]
    assert all(b.numel() == n for (_, n, _), b in zip(gw.handouts, bufs))


@pytest.mark.parametrize("which,side,offset", [(1, "before", -1), (1, "after", 4096), (2, "after", 7), (0, "before", -G.GUARD_BYTES),
                                               (0, "after", 1000 + G.GUARD_BYTES - 1)])
def test_one_damaged_guard_byte_is_named(which, side, offset):
    """One byte just before / just after a payload (and the outermost byte of each band), written through the parent."""
    gw, bufs = _three_handouts()
    g = bufs[which].guard
    g.parent[G.GUARD_BYTES + offset] ^= 0x40
    key, nbytes = gw.handouts[which][0], gw.handouts[which][1]
    with pytest.raises(AssertionError) as e:
        gw.check()
    msg = str(e.value)
    assert "workspace %r, %d bytes: guard %s the payload damaged, first at byte offset %d" % (key, nbytes, side, offset) in msg
    assert "1 of 3 buffers" in msg
    g.parent[G.GUARD_BYTES + offset] ^= 0x40                # put it back: the set passes again
    gw.check()


def test_an_input_guard_that_was_written_is_caught_too():
    gs = G.GuardSet("cpu")
    x = gs.input(torch.ones(5), "x")
    y = gs.output((5,), "y")
    gs.check()
    assert bool(torch.isnan(y).all())
    x.guard.parent[G.GUARD_BYTES + 20] = 1                  # the first byte past the five floats
    with pytest.raises(AssertionError, match=r"x, 20 bytes: guard after the payload damaged, first at byte offset 20"):
        gs.check()


def test_the_context_manager_swaps_ops_workspace_and_puts_it_back():
    from mtl_ssl_amd import ops
    before = ops.workspace
    with G.GuardedWorkspaces() as gw:
        assert ops.workspace == gw._hand_out
        with pytest.raises(AssertionError):
            gw.__enter__()                                  # not re-entrant
    assert ops.workspace is before
    try:
        with G.GuardedWorkspaces():
            raise KeyError("x")
    except KeyError:
        pass
    assert ops.workspace is before
    with G.GuardedOutputs() as go:
        assert ops.torch is not torch and ops.torch.float32 is torch.float32
        t = ops.torch.empty((2, 3), dtype=torch.float32, device="cpu")        # host allocations pass through
        assert not hasattr(t, "guard") and not go.tensors
    assert ops.torch is torch
