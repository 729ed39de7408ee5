"""Which launch plans does the Faster R-CNN VGG-16 configuration reach, and which of them does nothing else show?

configs/vgg16/frcnn_vgg16_voc_mtl.config was merged after the plan table (mtl_ssl_amd/conv_plans.json) was tuned and after
tools/offtable_plan_sweep.py swept the four tabled configurations, so none of its convolutions is in either. This sibling
of that tool enumerates them on the host and writes tests/golden/vgg16_conv_problems.json, which
tests/vgg/test_gpu_fullsize_plans.py runs against float64 on an MI355X and tests/vgg/test_host_plans.py regenerates on a CPU.

    python tools/vgg16_plan_sweep.py [--write]        counts; --write refreshes the fixture

Layers: the model as model_builder constructs it on the host (variables registered, nothing allocated); every layer's
(filter shape, stride, dilation, padding) is its own Layer.geometry(). The 13 trunk convolutions (fe.groups), the RPN
convolution and its two heads, the edge-mask convolution, every nn.Conv / nn.FCStack layer of the box, window and
closeness predictors and of the refiner.
Maps: the trunk shrinks through 2x2 / 2 VALID max-pools, so the input of group g is the frame floor-halved g times (vgg.py
extract_proposal_features) — not the SAME-style chain of the tabled extractors.
Head rows do not depend on the data: SAMPLED_ROIS per image for the box and closeness predictors and the refiner, DRAWN_WINDOWS
per image for the window head, REFINER_WINDOW_ROIS per image (forward only) for the refiner's window crops.
Modes are what one training step runs (frcnn.py backward, vgg.py backward_proposal_features, the predictors' backward):
every layer forward, a trainable layer wgrad, dgrad wherever the step propagates — all heads, and the trunk down to, but
not through, the first convolution of the first trainable group. Both freeze settings the README quotes a step rate for
are enumerated: the configuration's own 'conv2' and '' (everything trains).
Frames: the configuration's resizer over the source sizes of offtable_plan_sweep.frames, 600x1024 first; batches 1 (the
configuration's) and 2 (the step-rate figure's).

The fixture holds two lists. `production`: every (problem, mode) of the 600x1024 frame at batch 1 under either freeze
setting — these run at their own size whether or not their signature is shown elsewhere, like the plan table's pairs.
`representatives`: for every signature reached at the other frames or at batch 2 that neither the plan table's pairs, the
off-table fixture nor `production` shows, the cheapest problem that has it.
"""
import argparse
import ctypes
import inspect
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from offtable_plan_sweep import (FIXTURE as OFFTABLE_FIXTURE, PLANNING_SWITCHES, SIGNATURE_FIELDS, desc_of, frames,  # noqa: E402
                                 macs, signature, table_problems)

FIXTURE = os.path.join(ROOT, "tests", "golden", "vgg16_conv_problems.json")
CONFIG = os.path.join(ROOT, "configs", "vgg16", "frcnn_vgg16_voc_mtl.config")
OWN_FREEZE = "freeze_layer: 'conv2'"
FREEZE_SETTINGS = ("conv2", "")         # the configuration's own, and the other one the README quotes a step rate for
BENCH_FRAME = (600, 1024)
BATCHES = (1, 2)                        # train_config.batch_size, and tools/vgg16_step_rate.py's
MODE_NAMES = ("fwd", "dgrad", "wgrad")


def sampled_rois(model):
    """RoIs per image through the box predictor, the closeness predictor and the refiner: max_num_proposals, which is
    second_stage_batch_size while training without a hard example miner (frcnn.py _predict_second_stage)."""
    assert model._is_training and model._hard_miner is None
    return int(model.cfg.second_stage_batch_size)


def drawn_windows():
    """Windows per image through the window head (frcnn.py predict_with_window): the num_windows that
    provide_generated_labels draws, which is also what synthetic.make_batch and the records carry."""
    from mtl_ssl_amd.frcnn import FasterRCNNMetaArch
    return int(inspect.signature(FasterRCNNMetaArch.provide_generated_labels).parameters["num_windows"].default)


def refiner_window_rois(model):
    """RoIs per image of the refiner's window pass (frcnn.py _refine_window_predictions), forward only: the N_EXPAND - 1
    windows of every proposal that differ between proposals plus the DEDUP_SLOTS distinct whole-image ones."""
    assert model.DEDUP_SLOTS > 0
    return (model.N_EXPAND - 1) * sampled_rois(model) + model.DEDUP_SLOTS


def load_models():
    """{freeze setting: (cfg, model constructed on the host)}."""
    from mtl_ssl_amd import config, model_builder
    text = open(CONFIG).read()
    assert text.count(OWN_FREEZE) == 1, CONFIG
    out = {}
    for fz in FREEZE_SETTINGS:
        cfg = config.parse_pipeline_config(text.replace(OWN_FREEZE, "freeze_layer: '%s'" % fz))
        assert str(cfg.model.faster_rcnn.feature_extractor.freeze_layer) == fz
        out[fz] = (cfg, model_builder._construct(cfg.model, True, 0)[0])
    return out


def _add(out, ops, layer, shape, modes):
    d = ops.conv_desc(shape, *layer.geometry())
    prob = (d.N, d.H, d.W, d.C, d.K, d.R, d.S, d.OH, d.OW, d.stride, d.dilation, d.pad_t, d.pad_l)
    modes = set(modes) - (set() if layer.trainable else {2})
    names, have = out.setdefault(prob, ([], set()))
    have |= modes
    names.append(layer.scope)
    return (d.N, d.OH, d.OW, d.K)


def _predictor(out, ops, pred, rows, backward):
    """MaskRCNNBoxPredictor.predict / .backward (need_feat_grad: the identity tower hands the gradient on to the crops)."""
    for l in pred.layers():
        _add(out, ops, l, (rows, 1, 1, l.cin), (0, 1, 2) if backward else (0,))


def problems_of(ops, model, n, frame):
    """{problem: ([layer scopes], {modes})} of one training step at batch n on the given frame."""
    from mtl_ssl_amd import nn
    mtl, fe = model._mtl, model._feature_extractor
    # what the mode rules below restate (frcnn.py backward, the branch without shared classifier features)
    assert not model._shared_classifier and not model._first_stage_only and not mtl.stop_gradient_for_aux_tasks
    assert model.tower.layers() == [] and model.window_tower.layers() == [] and model.closeness_tower.layers() == []
    out = {}
    h, w = frame
    shape = (n, h, w, 3)
    for g, convs in enumerate(fe.groups):
        for i, l in enumerate(convs):
            assert isinstance(l, nn.Conv) and l.trainable == fe.group_trainable[g]
            # backward_proposal_features: groups below the first trainable one get nothing; its first layer no dgrad
            back = g >= fe.first_trainable
            modes = (0,) + ((2,) if back else ()) + ((1,) if back and not (i == 0 and g == fe.first_trainable) else ())
            shape = _add(out, ops, l, shape, modes)
        if g < len(fe.groups) - 1:
            shape = (n, shape[1] // 2, shape[2] // 2, shape[3])            # ops.maxpool_fwd(x, 2, 2, "VALID")
    F = shape
    rpn_feat = _add(out, ops, model.rpn_conv, F, (0, 1, 2))                # _backward_first_stage
    _add(out, ops, model.rpn_box, rpn_feat, (0, 1, 2))
    _add(out, ops, model.rpn_cls, rpn_feat, (0, 1, 2))
    if mtl.edgemask:
        _add(out, ops, model.edgemask_conv, F, (0, 1, 2))
    n2 = sampled_rois(model)
    _predictor(out, ops, model.box_predictor, n2 * n, True)
    if mtl.closeness:
        _predictor(out, ops, model.closeness_predictor, n2 * n, True)
    if mtl.window:
        _predictor(out, ops, model.window_predictor, drawn_windows() * n, True)
    if mtl.refine:
        if mtl.window:
            _predictor(out, ops, model.window_predictor, refiner_window_rois(model) * n, False)
        stack = model.refine_stack.layers if model.refine_stack is not None else []
        for i, l in enumerate(stack):                                      # FCStack.backward(need_input_grad=False)
            _add(out, ops, l, (n2 * n, 1, 1, l.cin), (0, 2) + ((1,) if i > 0 else ()))
        # the refiner's input is a stop_gradient: its last layer sends a gradient back only into a hidden stack
        _add(out, ops, model.refine_fc, (n2 * n, 1, 1, model.refine_fc.cin), (0, 2) + ((1,) if stack else ()))
    return {p: (names, tuple(sorted(m))) for p, (names, m) in out.items()}


def _query(ops, L, prob, mode):
    sig = signature(ops, prob, mode)
    d, info = desc_of(prob), ops.conv_plan_info(desc_of(prob), mode)
    return sig, (info["code"], int(L.conv2d_tile_config(ctypes.byref(d), mode)), info["dispatches"],
                 int(L.conv2d_num_dispatches(ctypes.byref(d), mode)), info["tail_rows"])


def sweep():
    """-> dict(reached, covered, production, representatives, queried, frames): reached / covered are sets of
    signatures (covered: shown by the plan table's pairs or the off-table fixture), production {(problem, mode):
    (signature, [freeze settings], [layer scopes])}, representatives {signature: (problem, mode)}, queried as in
    offtable_plan_sweep.sweep."""
    set_switches = [k for k in PLANNING_SWITCHES if k in os.environ]
    if set_switches:
        raise RuntimeError("planning switches are set: %s" % ", ".join(set_switches))
    import __graft_entry__ as g
    g.build()
    from mtl_ssl_amd import ops
    from mtl_ssl_amd.lib import lib
    L = lib()
    ops.reset_tuning(use_plan_db=True, autotune=False)
    try:
        covered = {signature(ops, p, m) for p, modes in sorted(table_problems().items()) for m in modes}
        covered |= {signature(ops, tuple(e["descriptor"]), e["mode"]) for e in json.load(open(OFFTABLE_FIXTURE))["problems"]}
        models = load_models()
        cfg = models[FREEZE_SETTINGS[0]][0]
        all_frames = frames(cfg.model.faster_rcnn.image_resizer, BENCH_FRAME)
        assert all_frames[0] == BENCH_FRAME and BATCHES[0] == int(cfg.train_config.batch_size)
        production, others, queried, reached = {}, {}, {}, set()
        for fz in FREEZE_SETTINGS:
            model = models[fz][1]
            for frame in all_frames:
                for n in BATCHES:
                    prod = frame == BENCH_FRAME and n == BATCHES[0]
                    for prob, (names, modes) in sorted(problems_of(ops, model, n, frame).items()):
                        for mode in modes:
                            if (prob, mode) not in queried:
                                queried[(prob, mode)] = _query(ops, L, prob, mode)
                            sig = queried[(prob, mode)][0]
                            reached.add(sig)
                            if prod:
                                rec = production.setdefault((prob, mode), (sig, [], []))
                                rec[1].append(fz)
                                rec[2].extend(s for s in names if s not in rec[2])
                            else:
                                others[(prob, mode)] = sig
        shown = covered | {rec[0] for rec in production.values()}
        reps = {}
        for (prob, mode), sig in sorted(others.items()):
            if sig not in shown:
                best = reps.get(sig)
                if best is None or (macs(prob), prob) < (macs(best[0]), best[0]):
                    reps[sig] = (prob, mode)
    finally:
        ops.reset_tuning()
    return dict(reached=reached, covered=covered, production=production, representatives=reps, frames=all_frames,
                queried=[(p, m, sig, rest) for (p, m), (sig, rest) in sorted(queried.items())])


def fixture_of(result):
    """The JSON document of the fixture: counts and both lists in a fixed order."""
    plain = lambda sig: json.loads(json.dumps(sig))
    prod = sorted(result["production"].items(), key=lambda kv: (kv[0][1], kv[0][0]))
    reps = sorted(result["representatives"].items(), key=lambda kv: (kv[1][1], kv[1][0]))
    prod_sigs = {rec[0] for rec in result["production"].values()}
    return {
        "comment": "launch plans of configs/vgg16/frcnn_vgg16_voc_mtl.config: every (problem, mode) of one training step at "
                   "600x1024, batch 1, under freeze_layer 'conv2' and '' (production), and one cheapest representative per "
                   "plan signature that other frames or batch 2 reach and nothing else shows (representatives) "
                   "(tools/vgg16_plan_sweep.py --write regenerates this file)",
        "signature_fields": list(SIGNATURE_FIELDS),
        "descriptor_fields": ["N", "H", "W", "C", "K", "R", "S", "OH", "OW", "stride", "dilation", "pad_t", "pad_l"],
        "frames": [list(f) for f in result["frames"]],
        "batches": list(BATCHES),
        "counts": {"pairs_queried": len(result["queried"]),
                   "signatures_reached": len(result["reached"]),
                   "signatures_covered_by_table_or_offtable": len(result["reached"] & result["covered"]),
                   "signatures_first_shown_by_production": len(prod_sigs - result["covered"]),
                   "production": len(prod),
                   "representatives": len(reps)},
        "production": [{"descriptor": list(prob), "mode": mode, "signature": plain(sig), "freeze_layers": list(fz),
                        "layers": list(names)} for (prob, mode), (sig, fz, names) in prod],
        "representatives": [{"descriptor": list(prob), "mode": mode, "signature": plain(sig)}
                            for sig, (prob, mode) in reps],
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--write", action="store_true", help="refresh tests/golden/vgg16_conv_problems.json")
    a = ap.parse_args()
    res = sweep()
    doc = fixture_of(res)
    c = doc["counts"]
    print("%d frames x batches %s x freeze_layer %s: %d (problem, mode) pairs queried" % (
        len(res["frames"]), list(BATCHES), list(FREEZE_SETTINGS), c["pairs_queried"]))
    print("signatures reached %d, covered by the plan table or the off-table fixture %d, first shown by production %d" % (
        c["signatures_reached"], c["signatures_covered_by_table_or_offtable"], c["signatures_first_shown_by_production"]))
    print("production %d pairs (%s), representatives %d" % (
        c["production"], ", ".join("%r: %d" % (fz, sum(fz in e["freeze_layers"] for e in doc["production"]))
                                   for fz in FREEZE_SETTINGS), c["representatives"]))
    for name in ("production", "representatives"):
        fams = {}
        for e in doc[name]:
            key = (MODE_NAMES[e["mode"]], e["signature"][1])
            fams[key] = fams.get(key, 0) + 1
        for key, n in sorted(fams.items()):
            print("    %-16s %-6s %-16s %d" % (name, key[0], key[1], n))
    if a.write:
        with open(FIXTURE, "w") as f:
            json.dump(doc, f, indent=0, sort_keys=True)
            f.write("\n")
        print("wrote", FIXTURE)


if __name__ == "__main__":
    main()
