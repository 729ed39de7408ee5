"""Which launch plans do the image shapes of real training reach that the committed plan table does not?

mtl_ssl_amd/conv_plans.json pins every convolution of the four shipped configurations at ONE frame, the benchmark's. The
keep-aspect-ratio resizer and the bucketing of input_reader.batches / InputPipeline hand the model other frames and
smaller batches, and every such problem is planned by the library's time models (csrc/conv.hip route: plan_gemm,
wgrad_plan, choose_wino). This tool enumerates those problems on the host, asks the planner what each would launch
(ops.conv_plan_info: no GPU), reduces the answer to a signature and keeps, for every signature the table's own 359 pairs do
not already show, the cheapest problem that has it: tests/golden/offtable_conv_problems.json, which
tests/test_gpu_offtable_plans.py runs against float64 on an MI355X and tests/test_offtable_plans.py regenerates on a CPU.

    python tools/offtable_plan_sweep.py [--write]        counts; --write refreshes the fixture

Frames: each config's own image_resizer (FasterRCNNMetaArch.resized_shape) applied to sources with a long side of 500 and
640, a short side of 160 .. long side in steps of 20, both orientations, plus the benchmark's frame. Batches: 1 .. the
config's per-GPU batch. Layer problems of a frame: the model's forward launches device kernels throughout (proposals, NMS,
RoI crops), so it cannot be recorded without a GPU; instead every image-derived problem of the table is carried to the new
frame along its (H, W) -> (OH, OW) chain. The extractors of this build reduce the map by SAME-style stride-2 steps only,
so a table problem whose input map is the frame halved k times (ops.same_pad) becomes the new frame halved k times, and
ops.conv_desc with the layer's own padding rule gives the rest of the descriptor. Head layers on RoI crops do not depend
on the frame and are skipped. The one image-level layer the table does not hold, the extractor's 3-channel stem, is
taken from the model as model_builder constructs it on the host (its space-to-depth forward is a planned launch too).
At a config's benchmark frame and batch the enumeration must give back that config's table problems exactly (self_check).
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, "tests", "golden", "offtable_conv_problems.json")
PLAN_FILE = os.path.join(ROOT, "mtl_ssl_amd", "conv_plans.json")
# (pipeline config, benchmark frame H, W): the runs of tools/tune_plans.py that made the table
CONFIGS = (("frcnn_resnet101_coco_mtl.config", 600, 1024), ("rfcn_resnet101_voc_mtl.config", 600, 1024),
           ("frcnn_mobilenet_v1_voc_mtl.config", 600, 1024), ("frcnn_inception_resnet_v2_coco_mtl.config", 800, 1333))
LONG_SIDES, SHORT_MIN, SHORT_STEP = (500, 640), 160, 20
LEVELS = 6                      # halvings of the frame looked at (the extractors stop at 4)
PLANNING_SWITCHES = ("MTLSSL_FORCE_CFG", "MTLSSL_WINOGRAD", "MTLSSL_PLAN_FILE", "MTLSSL_PLAN_DB", "MTLSSL_FP32_ENGINE")
SIGNATURE_FIELDS = ("mode", "family", "code", "tile", "nsplit", "ragged_last_split", "tail", "tail_nsplit", "M_mod_BM",
                    "NG_mod_BN", "NG_mod_4", "pointwise", "stride", "wino_ragged_frame", "parity_classes")


def table_problems():
    """{problem (N, H, W, C, K, R, S, OH, OW, stride, dilation, pad_t, pad_l): sorted modes} of the plan table."""
    probs = {}
    for key in json.load(open(PLAN_FILE))["plans"]:
        v = tuple(int(t) for t in key.split(","))
        probs.setdefault(v[1:], []).append(v[0])
    return {p: sorted(m) for p, m in probs.items()}


def _levels(ops, h, w):
    out = [(h, w)]
    for _ in range(LEVELS):
        out.append((ops.same_pad(out[-1][0], 3, 2)[1], ops.same_pad(out[-1][1], 3, 2)[1]))
    return out


def _padding_rule(ops, prob):
    """The conv_desc padding rule that builds this table problem (as tests/test_plan_table.py checks every key has one)."""
    N, H, W, C, K, R, S, OH, OW, stride, dil, pt, pl = prob
    for pad in ("SAME", "VALID", "RESNET_SAME"):
        d = ops.conv_desc((N, H, W, C), (R, S, C, K), stride, dil, pad)
        if (d.OH, d.OW, d.pad_t, d.pad_l) == (OH, OW, pt, pl):
            return pad
    raise ValueError("no padding rule of ops.conv_desc builds %r" % (prob,))


def load_configs():
    """[(name, per-GPU batch, resizer message, (Hb, Wb))]."""
    return [c[:4] for c in _configs()]


def _configs():
    from mtl_ssl_amd import config
    out = []
    for name, hb, wb in CONFIGS:
        cfg = config.parse_pipeline_config(open(os.path.join(ROOT, "configs", name)).read())
        out.append((name, int(cfg.train_config.batch_size), cfg.model.faster_rcnn.image_resizer, (hb, wb), cfg))
    return out


def stem_templates(cfg):
    """The extractor's 3-channel first convolution, which reads the frame itself (level 0), as a template like
    layer_templates': taken from the model as model_builder constructs it on the host (variables registered, nothing
    allocated). The table does not hold it (it is off the MFMA path: mtlssl_conv2d_tile_config = -1) but its forward is a
    planned launch all the same — the space-to-depth form runs plan_gemm on the frame's rows. Forward only: the input
    is the image, and the filter gradient of a stem is a VALU kernel no planner touches."""
    from mtl_ssl_amd import model_builder, nn
    model, _ = model_builder._construct(cfg.model, True, 0)
    stems = [l for l in model._feature_extractor.layers() if isinstance(l, nn.ConvBN) and int(l.w.shape[2]) == 3]
    assert len(stems) == 1, len(stems)
    l = stems[0]
    R, S, C, K = (int(v) for v in l.w.shape)
    return [(0, (C, K, R, S, int(l.stride), int(l.dilation)), l.padding, (0,))]


def frames(resizer, bench_frame):
    """Resized frames of the source sizes above under this config's resizer, the benchmark's own frame first."""
    from mtl_ssl_amd.frcnn import FasterRCNNMetaArch
    out = [tuple(bench_frame)]
    for long_side in LONG_SIDES:
        for short in range(SHORT_MIN, long_side + 1, SHORT_STEP):
            for h, w in ((short, long_side), (long_side, short)):
                f = tuple(FasterRCNNMetaArch.resized_shape(h, w, resizer))
                if f not in out:
                    out.append(f)
    return out


def layer_templates(ops, table, batch, bench_frame):
    """The table's image-derived problems of one config: [(level k, (C, K, R, S, stride, dilation), padding rule, modes)]
    for every table problem with N = the config's batch whose input map is the benchmark frame halved k times."""
    lv = _levels(ops, *bench_frame)
    out = []
    for prob, modes in sorted(table.items()):
        N, H, W, C, K, R, S, OH, OW, stride, dil, pt, pl = prob
        if N == batch and (H, W) in lv[1:]:
            out.append((lv.index((H, W)), (C, K, R, S, stride, dil), _padding_rule(ops, prob), tuple(modes)))
    return out


def problems_at(ops, templates, n, frame):
    """{problem: modes} of the templates at batch n and the given frame."""
    lv = _levels(ops, *frame)
    out = {}
    for k, (C, K, R, S, stride, dil), pad, modes in templates:
        h, w = lv[k]
        d = ops.conv_desc((n, h, w, C), (R, S, C, K), stride, dil, pad)
        prob = (d.N, d.H, d.W, d.C, d.K, d.R, d.S, d.OH, d.OW, d.stride, d.dilation, d.pad_t, d.pad_l)
        out[prob] = tuple(sorted(set(out.get(prob, ())) | set(modes)))
    return out


def self_check(ops=None):
    """At each config's benchmark frame and batch the enumeration reproduces that config's image-derived table problems
    (with their modes) exactly, every image-derived table problem belongs to a config, and every stride-2 one of them
    maps a level of the frame onto the next. -> {config: number of problems}."""
    if ops is None:
        from mtl_ssl_amd import ops
    table = table_problems()
    claimed, counts = set(), {}
    for name, batch, _, bench_frame, cfg in _configs():
        lv = _levels(ops, *bench_frame)
        want = {p: tuple(m) for p, m in table.items() if p[0] == batch and (p[1], p[2]) in lv[1:]}
        got = problems_at(ops, layer_templates(ops, table, batch, bench_frame), batch, bench_frame)
        assert got == want, (name, sorted(set(got) ^ set(want))[:5])
        assert want, name
        for p in want:
            assert p[9] in (1, 2), (name, p)
            assert (p[7], p[8]) == lv[lv.index((p[1], p[2])) + p[9] - 1], (name, p)
        assert not (claimed & set(want)), name
        assert not (set(problems_at(ops, stem_templates(cfg), batch, bench_frame)) & set(table)), name    # off the table
        claimed |= set(want)
        counts[name] = len(want)
    # what is left are head layers on RoI crops: many crops of at most 17 x 17, never a config's batch of image maps
    for p in set(table) - claimed:
        assert p[0] >= 64 and max(p[1], p[2]) <= 17, p
    return counts


def enumerate_problems(ops):
    """{problem: modes} over every config, frame and batch 1 .. the per-GPU batch."""
    table = table_problems()
    out = {}
    for name, batch, resizer, bench_frame, cfg in _configs():
        templates = layer_templates(ops, table, batch, bench_frame) + stem_templates(cfg)
        for frame in frames(resizer, bench_frame):
            for n in range(1, batch + 1):
                for prob, modes in problems_at(ops, templates, n, frame).items():
                    out[prob] = tuple(sorted(set(out.get(prob, ())) | set(modes)))
    return out


def desc_of(prob):
    from mtl_ssl_amd.lib import ConvDesc
    return ConvDesc(*prob, 0)


def _gemm_sig(info):
    """(tile, nsplit, ragged last split, tail present, tail_nsplit, M % BM != 0, NG % BN != 0, NG % 4 != 0) of one GEMM plan."""
    if info["tile"] < 0 or info["nsplit"] == 0:
        return (info["tile"], 0, 0, 0, 0, 0, 0, 0)
    if info["pix_per_split"]:                                   # wgrad: the pixel range is what is split
        ragged = info["nsplit"] > 1 and info["ksteps"] % info["ks_per_split"] != 0
    else:
        ragged = ((info["nsplit"] > 1 and info["ksteps"] % info["ks_per_split"] != 0)
                  or (info["tail_rows"] > 0 and info["ksteps"] % info["tail_ks"] != 0))
    return (info["tile"], info["nsplit"], int(ragged), int(info["tail_rows"] > 0), info["tail_nsplit"],
            int(info["M"] % info["BM"] != 0), int(info["NG"] % info["BN"] != 0), int(info["NG"] % 4 != 0))


def signature(ops, prob, mode):
    """The plan of (problem, mode) as production would run it (the table's pin applied through ops._autotune like the first
    call of the pair does), reduced to SIGNATURE_FIELDS. The input-parity dgrad lists its four sub-plans."""
    d = desc_of(prob)
    ops._autotune(d, mode, None)
    info = ops.conv_plan_info(d, mode)
    fam = info["family"]
    classes = ()
    if fam == "input_parity":
        subs = [_gemm_sig(ops.conv_plan_info(d, mode, c)) for c in range(4)]
        classes = tuple(sorted(set(subs)))
        g = max(subs, key=lambda s: (s[3], s[1], s))            # headline: the class with a tail, else the widest split
    else:
        g = _gemm_sig(info)
    wino_ragged = 0
    if fam.startswith("winograd"):
        t = 4 if fam == "winograd_F43" else 7
        hs, ws = (prob[1], prob[2]) if mode == 1 else (prob[7], prob[8])
        wino_ragged = int(hs % t != 0 or ws % t != 0)
        g = (g[0], 1, 0, 0, 0) + g[5:]
    return (mode, fam, info["code"]) + g + (int(ops.desc_is_pointwise(d)), prob[9], wino_ragged, classes)


def macs(prob):
    N, H, W, C, K, R, S, OH, OW = prob[:9]
    return N * OH * OW * K * C * R * S


def sweep():
    """-> dict(reached, covered, representatives, queried): reached / covered are sets of signatures, representatives
    {signature: (problem, mode)} for the reached signatures the table does not show, queried [(problem, mode, signature,
    (plan_info's code, conv2d_tile_config, plan_info's dispatches, conv2d_num_dispatches, tail_rows))]."""
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
        reps, reached, queried = {}, set(), []
        for prob, modes in sorted(enumerate_problems(ops).items()):
            for mode in modes:
                sig = signature(ops, prob, mode)
                d, info = desc_of(prob), ops.conv_plan_info(desc_of(prob), mode)
                queried.append((prob, mode, sig, (info["code"], int(L.conv2d_tile_config(ctypes.byref(d), mode)),
                                                  info["dispatches"], int(L.conv2d_num_dispatches(ctypes.byref(d), mode)),
                                                  info["tail_rows"])))
                reached.add(sig)
                if sig not in covered:
                    best = reps.get(sig)
                    if best is None or (macs(prob), prob) < (macs(best[0]), best[0]):
                        reps[sig] = (prob, mode)
    finally:
        ops.reset_tuning()
    return dict(reached=reached, covered=covered, representatives=reps, queried=queried)


def fixture_of(result):
    """The JSON document of the fixture: counts and the representatives in a fixed order."""
    reps = sorted(result["representatives"].items(), key=lambda kv: (kv[1][1], kv[1][0]))
    return {
        "comment": "off-table launch plans training can reach: one cheapest representative per plan signature the plan "
                   "table's own pairs do not show (tools/offtable_plan_sweep.py --write regenerates this file)",
        "signature_fields": list(SIGNATURE_FIELDS),
        "descriptor_fields": ["N", "H", "W", "C", "K", "R", "S", "OH", "OW", "stride", "dilation", "pad_t", "pad_l"],
        "counts": {"signatures_reached": len(result["reached"]),
                   "signatures_covered_by_table": len(result["reached"] & result["covered"]),
                   "representatives": len(reps)},
        "problems": [{"descriptor": list(prob), "mode": mode, "signature": json.loads(json.dumps(sig))}
                     for sig, (prob, mode) in reps],
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--write", action="store_true", help="refresh tests/golden/offtable_conv_problems.json")
    a = ap.parse_args()
    print("self-check at the benchmark frames:", self_check())
    res = sweep()
    doc = fixture_of(res)
    print("%d (problem, mode) pairs queried; signatures reached %d, covered by the table %d, representatives %d" % (
        len(res["queried"]), doc["counts"]["signatures_reached"], doc["counts"]["signatures_covered_by_table"],
        doc["counts"]["representatives"]))
    fams = {}
    for e in doc["problems"]:
        key = (("fwd", "dgrad", "wgrad")[e["mode"]], e["signature"][1])
        fams[key] = fams.get(key, 0) + 1
    for key, n in sorted(fams.items()):
        print("    %-6s %-16s %d" % (key[0], key[1], n))
    if a.write:
        with open(FIXTURE, "w") as f:
            json.dump(doc, f, indent=0, sort_keys=True)
            f.write("\n")
        print("wrote", FIXTURE)


if __name__ == "__main__":
    main()
