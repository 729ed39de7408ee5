"""CPU-only tests of the host logic: pipeline-config parsing and proto defaults, parameter store
layout, learning-rate schedule, label generators, and the data-parallel gradient reduction
(world_size 2 over gloo)."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(name):
    from mtl_ssl_amd import config
    return config.parse_pipeline_config(open(os.path.join(ROOT, "configs", name)).read())


def test_pipeline_config_parses_with_proto_defaults():
    cfg = _cfg("frcnn_resnet101_coco_mtl.config")
    fr, mtl, tc = cfg.model.faster_rcnn, cfg.model.mtl, cfg.train_config
    assert fr.num_classes == 90 and fr.feature_extractor.type == "faster_rcnn_resnet101"
    assert fr.first_stage_anchor_generator.grid_anchor_generator.scales == [0.25, 0.5, 1.0, 2.0]
    # unset fields fall back to the .proto defaults (protos/faster_rcnn.proto:20-146, model.proto:27-58)
    assert fr.first_stage_minibatch_size == 256 and fr.first_stage_box_predictor_depth == 512
    assert fr.second_stage_balance_fraction == 0.25 and fr.feature_extractor.freeze_layer == "block1"
    assert fr.first_stage_clip_window is False
    assert mtl.shared_feature == "proposal_feature_maps" and mtl.global_closeness is True
    assert mtl.stop_gradient_for_aux_tasks is True and mtl.refine_num_fc_layers == 0
    assert tc.gradient_clipping_by_norm == 10.0 and tc.optimizer.use_moving_average is False
    sched = tc.optimizer.momentum_optimizer.learning_rate.manual_step_learning_rate.schedule
    assert [s.step for s in sched] == [820000, 950000]
    assert fr.second_stage_box_predictor.which_oneof(["mask_rcnn_box_predictor", "rfcn_box_predictor"]) \
        == "mask_rcnn_box_predictor"


def test_text_format_corner_cases():
    from mtl_ssl_amd import config
    m = config.parse_pipeline_config("""
      # comment
      model { faster_rcnn { num_classes: 3  feature_extractor { type: "x" } } }
      train_config: { batch_size: 4 data_augmentation_options { random_horizontal_flip { } }
                      data_augmentation_options { random_horizontal_flip { } } }
      train_input_reader: { tf_record_input_reader { input_path: "a" input_path: 'b' } }
    """)
    assert m.model.faster_rcnn.num_classes == 3
    assert len(m.train_config.data_augmentation_options) == 2
    assert m.train_input_reader.tf_record_input_reader.input_path == ["a", "b"]
    with pytest.raises(ValueError):
        config.parse_pipeline_config("model { faster_rcnn { ")
    with pytest.raises(AttributeError):
        m.model.faster_rcnn.no_such_field


def test_model_builder_rejects_unknown_types():
    from mtl_ssl_amd import config, model_builder
    cfg = config.parse_pipeline_config("model { faster_rcnn { num_classes: 3 feature_extractor { type: 'nope' } } }")
    with pytest.raises(ValueError, match="Unknown Faster R-CNN feature_extractor"):
        model_builder.build(cfg.model, True, "cpu")
    cfg = config.parse_pipeline_config("model { ssd { num_classes: 3 } }")
    with pytest.raises(ValueError, match="ssd"):
        model_builder.build(cfg.model, True, "cpu")


def test_batch_norm_trainable_by_extractor_family():
    """ResNet: gamma / beta of every BatchNorm — frozen root conv and frozen block1 included — become trainable variables
    on the moving statistics (models/faster_rcnn_resnet_v1_feature_extractor.py:131,169; slim/nets/resnet_utils.py:203-237).
    MobileNet: the flag means batch-statistics BatchNorm there (…mobilenet…:89,127,168): a clear error, never a silently
    different model. Inception-ResNet-v2 ignores it (next test)."""
    from mtl_ssl_amd import config, model_builder
    from mtl_ssl_amd.params import ParamStore
    text = open(os.path.join(ROOT, "configs", "frcnn_resnet101_coco_mtl.config")).read()
    assert "type: 'faster_rcnn_resnet101'" in text
    cfg = config.parse_pipeline_config(text.replace("type: 'faster_rcnn_resnet101'",
                                                    "type: 'faster_rcnn_resnet101' batch_norm_trainable: true"))
    fe_cfg = cfg.model.faster_rcnn.feature_extractor
    ps = ParamStore()
    fe = model_builder.FASTER_RCNN_FEATURE_EXTRACTOR_CLASS_MAP["faster_rcnn_resnet101"](ps, fe_cfg, True)
    tower = fe.box_classifier_tower("SecondStageFeatureExtractor", True)
    by = {sp.name: sp for sp in ps.specs}
    p = "FirstStageFeatureExtractor/resnet_v1_101/"
    assert by[p + "conv1/BatchNorm/gamma"].trainable and by[p + "block1/unit_2/bottleneck_v1/conv2/BatchNorm/beta"].trainable
    assert not by[p + "conv1/weights"].trainable and not by[p + "block1/unit_2/bottleneck_v1/conv2/weights"].trainable
    assert by[p + "block3/unit_23/bottleneck_v1/conv3/BatchNorm/gamma"].trainable
    assert by["SecondStageFeatureExtractor/resnet_v1_101/block4/unit_3/bottleneck_v1/conv3/BatchNorm/beta"].trainable
    assert not any(sp.trainable for sp in ps.specs if "moving_" in sp.name)
    assert fe.first_trainable == 0 and tower.stack.units[0].bn_trainable
    ps2 = ParamStore()                                   # inference replica: nothing trains
    model_builder.FASTER_RCNN_FEATURE_EXTRACTOR_CLASS_MAP["faster_rcnn_resnet101"](ps2, fe_cfg, False)
    assert not any(sp.trainable for sp in ps2.specs)
    t = open(os.path.join(ROOT, "configs", "frcnn_mobilenet_v1_voc_mtl.config")).read()
    assert "type: 'frcnn_mobilenet_v1'" in t
    c = config.parse_pipeline_config(t.replace("type: 'frcnn_mobilenet_v1'", "type: 'frcnn_mobilenet_v1' batch_norm_trainable: true"))
    with pytest.raises(ValueError, match="batch-statistics"):       # MobileNet: the flag means batch statistics (:127,168)
        model_builder.build(c.model, True, "cpu")


def test_inception_batch_norm_trainable_is_accepted_and_ignored():
    """The reference's Inception-ResNet-v2 extractor stores `batch_norm_trainable` and never reads it: both arg scopes
    force slim.batch_norm(is_training=False) (models/faster_rcnn_inception_resnet_v2_feature_extractor.py:59, 105-106,
    136-137). A config with the flag must build, with the same variables (names, shapes, trainability, initial values)
    as the config without it."""
    from mtl_ssl_amd import config, model_builder
    from mtl_ssl_amd.params import ParamStore
    typ = "faster_rcnn_inception_resnet_v2"
    t = open(os.path.join(ROOT, "configs", "frcnn_inception_resnet_v2_coco_mtl.config")).read()
    assert "type: '%s'" % typ in t
    stores = []
    for text in (t, t.replace("type: '%s'" % typ, "type: '%s' batch_norm_trainable: true" % typ)):
        fe_cfg = config.parse_pipeline_config(text).model.faster_rcnn.feature_extractor
        ps = ParamStore()
        fe = model_builder.FASTER_RCNN_FEATURE_EXTRACTOR_CLASS_MAP[typ](ps, fe_cfg, True)
        fe.box_classifier_tower("SecondStageFeatureExtractor", True)
        stores.append(ps)
    assert bool(config.parse_pipeline_config(text).model.faster_rcnn.feature_extractor.batch_norm_trainable)
    a, b = stores
    assert [(s.name, tuple(s.shape), s.trainable, s.init) for s in a.specs] == \
        [(s.name, tuple(s.shape), s.trainable, s.init) for s in b.specs]
    assert not any(s.trainable for s in b.specs if "moving_" in s.name)
    a.finalize("cpu", seed=3)
    b.finalize("cpu", seed=3)
    assert torch.equal(a.weights, b.weights)


def test_param_store_layout_and_reference_names():
    from mtl_ssl_amd import frcnn, model_builder
    from mtl_ssl_amd.params import ParamStore
    cfg = _cfg("frcnn_resnet101_coco_mtl.config")
    ps = ParamStore()
    fe = model_builder.FASTER_RCNN_FEATURE_EXTRACTOR_CLASS_MAP["faster_rcnn_resnet101"](
        ps, cfg.model.faster_rcnn.feature_extractor, True)
    frcnn.FasterRCNNMetaArch(ps, True, cfg.model.faster_rcnn, cfg.model.mtl, fe)
    names = set(ps.by_name)
    for n in ("FirstStageFeatureExtractor/resnet_v1_101/conv1/weights",
              "FirstStageFeatureExtractor/resnet_v1_101/block3/unit_23/bottleneck_v1/conv2/BatchNorm/moving_variance",
              "SecondStageFeatureExtractor/resnet_v1_101/block4/unit_1/bottleneck_v1/shortcut/weights",
              "ClosenessBoxPredictor/resnet_v1_101/block4/unit_3/bottleneck_v1/conv3/weights",
              "WindowBoxPredictor/ClassPredictor/biases", "FirstStageBoxPredictor/Conv/weights",
              "SecondStageBoxPredictor/BoxEncodingPredictor/weights",
              "EdgeMaskPredictor/BoxEncodingPredictor/weights", "MTLClassRefiner/fc1/weights"):
        assert n in names, n
    tr = {s.name for s in ps.specs if s.trainable}
    assert not any("BatchNorm" in n for n in tr)              # BN is frozen
    assert not any("/conv1/weights" in n and "block" not in n for n in tr)   # root conv never trains
    assert not any("block1" in n for n in tr)                 # freeze_layer default 'block1'
    assert ps.by_name["MTLClassRefiner/fc1/weights"].shape == (7 * 91, 91)
    assert ps.by_name["SecondStageBoxPredictor/BoxEncodingPredictor/weights"].shape == (2048, 360)


def test_mobilenet_variables_follow_slim_names_and_trainability():
    """slim/nets/mobilenet_v1.py:120-266,376-413 + models/faster_rcnn_mobilenet_v1_feature_extractor.py:
    145-184: BatchNorm gamma/beta train (moving stats do not); depthwise filters and the second-stage
    separable convs carry no L2 regulariser, conv / pointwise filters carry `weight_decay`."""
    from mtl_ssl_amd import frcnn, model_builder
    from mtl_ssl_amd.params import ParamStore
    cfg = _cfg("frcnn_mobilenet_v1_voc_mtl.config")
    ps = ParamStore()
    fe = model_builder.FASTER_RCNN_FEATURE_EXTRACTOR_CLASS_MAP["frcnn_mobilenet_v1"](
        ps, cfg.model.faster_rcnn.feature_extractor, True)
    frcnn.FasterRCNNMetaArch(ps, True, cfg.model.faster_rcnn, cfg.model.mtl, fe)
    by = ps.by_name
    p = "FirstStageFeatureExtractor/MobilenetV1/"
    assert by[p + "Conv2d_0/weights"].shape == (3, 3, 3, 32) and by[p + "Conv2d_0/weights"].weight_decay == 1e-4
    assert by[p + "Conv2d_11_pointwise/weights"].shape == (1, 1, 512, 512)
    assert by[p + "Conv2d_6_depthwise/depthwise_weights"].shape == (3, 3, 256, 1)
    assert by[p + "Conv2d_6_depthwise/depthwise_weights"].weight_decay == 0.0
    assert by[p + "Conv2d_3_pointwise/BatchNorm/gamma"].trainable
    assert not by[p + "Conv2d_3_pointwise/BatchNorm/moving_mean"].trainable
    for scope in ("SecondStageFeatureExtractor", "ClosenessBoxPredictor", "WindowBoxPredictor"):
        q = scope + "/MobilenetV1/"
        assert by[q + "Conv2d_12_pointwise/depthwise_weights"].shape == (3, 3, 512, 1)
        assert by[q + "Conv2d_13_pointwise/pointwise_weights"].shape == (1, 1, 1024, 1024)
        assert by[q + "Conv2d_13_pointwise/pointwise_weights"].weight_decay == 0.0
        assert q + "Conv2d_12_pointwise/BatchNorm/beta" in by
        assert q + "Conv2d_12_depthwise/depthwise_weights" not in by
    assert by["SecondStageBoxPredictor/ClassPredictor/weights"].shape == (1024, 21)
    with pytest.raises(ValueError, match="must be 8 or 16"):
        from mtl_ssl_amd import mobilenet
        mobilenet.FasterRCNNMobilenetV1FeatureExtractor(ParamStore(), True, first_stage_features_stride=4)


def test_resize_to_range_shapes_match_reference_known_answers():
    """core/preprocessor_test.py:1398-1409 testResizeToRangePreservesStaticSpatialShape."""
    from mtl_ssl_amd import config, frcnn
    r = config.parse_pipeline_config(
        "model { faster_rcnn { image_resizer { keep_aspect_ratio_resizer { min_dimension: 50 max_dimension: 100 } } } }"
    ).model.faster_rcnn.image_resizer
    for (h, w), want in zip([(60, 40), (15, 30), (15, 50)], [(75, 50), (50, 100), (30, 100)]):
        assert frcnn.FasterRCNNMetaArch.resized_shape(h, w, r) == want
    r = config.parse_pipeline_config(
        "model { faster_rcnn { image_resizer { fixed_shape_resizer { height: 320 width: 200 } } } }"
    ).model.faster_rcnn.image_resizer
    assert frcnn.FasterRCNNMetaArch.resized_shape(60, 40, r) == (320, 200)
    d = _cfg("frcnn_resnet101_coco_mtl.config").model.faster_rcnn.image_resizer
    assert frcnn.FasterRCNNMetaArch.resized_shape(600, 1024, d) == (600, 1024)       # bench inputs: identity
    assert frcnn.FasterRCNNMetaArch.resized_shape(480, 640, d) == (600, 800)
    assert frcnn.FasterRCNNMetaArch.resized_shape(375, 1242, d) == (309, 1024)


def test_checkpoint_maps_follow_reference_restore_rules(tmp_path):
    """faster_rcnn_meta_arch.py:167-205,1947-2013; models/...inception_resnet_v2...:173-248;
    trainer.py:309-356."""
    from mtl_ssl_amd import checkpoint, frcnn, model_builder
    from mtl_ssl_amd.params import ParamStore
    cfg = _cfg("frcnn_resnet101_coco_mtl.config")
    ps = ParamStore()
    fe = model_builder.FASTER_RCNN_FEATURE_EXTRACTOR_CLASS_MAP["faster_rcnn_resnet101"](
        ps, cfg.model.faster_rcnn.feature_extractor, True)
    frcnn.FasterRCNNMetaArch(ps, True, cfg.model.faster_rcnn, cfg.model.mtl, fe)
    ps.finalize("cpu", seed=1)
    # classification checkpoint: scopes stripped, first and second stage only
    m = checkpoint.restore_map(ps, from_detection_checkpoint=False)
    assert m["resnet_v1_101/conv1/weights"] == "FirstStageFeatureExtractor/resnet_v1_101/conv1/weights"
    assert m["resnet_v1_101/block4/unit_3/bottleneck_v1/conv3/weights"] == \
        "SecondStageFeatureExtractor/resnet_v1_101/block4/unit_3/bottleneck_v1/conv3/weights"
    assert not any(v.startswith(("WindowBoxPredictor", "FirstStageBoxPredictor", "MTLClassRefiner")) for v in m.values())
    # aux towers share the classification init (share_second_stage_init, trainer.py:337-346)
    aux = checkpoint.mtl_init_maps(ps, cfg.model.mtl, from_detection_checkpoint=False)
    assert len(aux) == 3
    assert aux[0]["resnet_v1_101/block4/unit_1/bottleneck_v1/shortcut/weights"].startswith("WindowBoxPredictor/")
    assert checkpoint.mtl_init_maps(ps, cfg.model.mtl, from_detection_checkpoint=True) == []
    # detection checkpoint: feature extractors always, heads on request
    d = checkpoint.restore_map(ps, True)
    assert all(k == v for k, v in d.items())
    assert not any(k.startswith(("SecondStageBoxPredictor", "WindowBoxPredictor")) for k in d)
    d = checkpoint.restore_map(ps, True, restore_box_predictor=True, restore_window=True, restore_mtl_refine=True)
    assert "SecondStageBoxPredictor/ClassPredictor/weights" in d and "MTLClassRefiner/fc1/biases" in d
    assert any(k.startswith("WindowBoxPredictor/") for k in d) and not any(k.startswith("ClosenessBoxPredictor/") for k in d)
    # import: shape-checked like variables_helper.get_variables_available_in_checkpoint
    name = "FirstStageFeatureExtractor/resnet_v1_101/block2/unit_1/bottleneck_v1/conv1/weights"
    shape = ps.by_name[name].shape
    ck = {"resnet_v1_101/block2/unit_1/bottleneck_v1/conv1/weights": np.full(shape, 0.5, np.float32),
          "resnet_v1_101/conv1/weights": np.zeros((3, 3, 3, 64), np.float32),      # wrong shape: skipped
          "resnet_v1_101/logits/weights": np.zeros((1, 1, 2048, 1000), np.float32)}  # not in the model: skipped
    done = checkpoint.assign(ps, m, ck)
    assert done == [name] and float(ps.value(name).mean()) == 0.5
    # save / load round trip incl. momentum slots and step
    ps.accum.uniform_(-1, 1)
    w0, a0 = ps.weights.clone(), ps.accum.clone()
    path = str(tmp_path / "state.npz")
    checkpoint.save(path, ps, global_step=1234)
    ps.weights.zero_(); ps.accum.zero_(); ps.frozen.zero_()
    assert checkpoint.load(path, ps) == 1234
    for sp in ps.trainable_specs:
        assert torch.equal(ps._view(ps.weights, sp), ps._view(w0, sp)) and torch.equal(ps._view(ps.accum, sp), ps._view(a0, sp))
    # Inception-ResNet-v2: the second-stage `Repeat` scope is `Repeat_2` in the classification graph
    icfg = _cfg("frcnn_inception_resnet_v2_coco_mtl.config")
    ips = ParamStore()
    ife = model_builder.FASTER_RCNN_FEATURE_EXTRACTOR_CLASS_MAP["faster_rcnn_inception_resnet_v2"](
        ips, icfg.model.faster_rcnn.feature_extractor, True)
    frcnn.FasterRCNNMetaArch(ips, True, icfg.model.faster_rcnn, icfg.model.mtl, ife)
    im = checkpoint.restore_map(ips, False, inception_resnet_v2=True)
    assert im["InceptionResnetV2/Repeat_2/block8_3/Branch_0/Conv2d_1x1/weights"] == \
        "SecondStageFeatureExtractor/InceptionResnetV2/Repeat/block8_3/Branch_0/Conv2d_1x1/weights"
    assert im["InceptionResnetV2/Repeat/block35_1/Conv2d_1x1/biases"] == \
        "FirstStageFeatureExtractor/InceptionResnetV2/Repeat/block35_1/Conv2d_1x1/biases"


def test_every_shipped_pipeline_config_builds():
    """Every pipeline config under configs/ (ResNet-50 / ResNet-101 / MobileNet-v1 / Inception-ResNet-v2,
    Faster R-CNN and R-FCN heads, full-size and smoke) parses and builds its full variable set through the
    plugin registry."""
    from mtl_ssl_amd import config, frcnn, model_builder, rfcn
    from mtl_ssl_amd.params import ParamStore
    cdir = os.path.join(ROOT, "configs")
    names = sorted(f for f in os.listdir(cdir) if f.endswith(".config"))
    assert len(names) == 8
    kinds = set()
    for f in names:
        cfg = config.parse_pipeline_config(open(os.path.join(cdir, f)).read())
        fr = cfg.model.faster_rcnn
        ps = ParamStore()
        fe = model_builder.FASTER_RCNN_FEATURE_EXTRACTOR_CLASS_MAP[fr.feature_extractor.type](
            ps, fr.feature_extractor, True)
        arch = rfcn.RFCNMetaArch if fr.second_stage_box_predictor.has("rfcn_box_predictor") else frcnn.FasterRCNNMetaArch
        arch(ps, True, fr, cfg.model.mtl, fe)
        assert len(ps.specs) > 100 and any(s.trainable for s in ps.specs)
        from mtl_ssl_amd import trainer
        f_lr, mom = trainer.learning_rate_fn(cfg.train_config.optimizer)
        assert f_lr(0) > 0 and mom == 0.9
        kinds.add((fr.feature_extractor.type, arch.__name__))
    assert len(kinds) >= 4, kinds


def test_manual_step_learning_rate():
    from mtl_ssl_amd import trainer
    f, mom = trainer.learning_rate_fn(_cfg("smoke_resnet50_mtl.config").train_config.optimizer)
    assert mom == 0.9 and f(0) == 0.001 and f(4) == 0.001 and f(5) == 0.0001 and f(10 ** 6) == 0.0001


def test_label_generators_match_the_reference_functions():
    """labels.py against outputs of the reference's own label functions (create_pascal_tf_record.py:120-421,
    lifted with ast and run by tests/golden/make_aux_label_golden.py in the authoring container): window
    boxes + soft labels of both branches (random windows driven by the same random.random() stream,
    and the expanding windows), closeness labels, edge masks, and the union-area helper."""
    import json
    from mtl_ssl_amd import labels
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "aux_labels_golden.json")))
    assert len(gold["cases"]) >= 10
    for c in gold["cases"]:
        K, W, H = c["K"], c["width"], c["height"]
        boxes, classes = np.asarray(c["boxes"], float).reshape(-1, 4), c["classes"]
        if c["random_windows"]:
            wb, wl = labels.random_windows(boxes, classes, W, H, K, labels.PyRandom(c["seed"]))
            if not len(boxes):                  # the reference emits ONE window, this build repeats it 64x
                wb, wl = wb[:1], wl[:1]
        else:
            wb, wl = labels.expanding_windows(boxes, classes, W, H, K)
        assert wb.shape == (len(c["window_boxes"]), 4), (wb.shape, len(c["window_boxes"]))
        np.testing.assert_allclose(wb, np.asarray(c["window_boxes"]), rtol=0, atol=1e-6)
        # labels are stored as 3-decimal text; the union area comes from a different algorithm (coordinate
        # compression vs inclusion-exclusion), so a value sitting on a rounding boundary may move by one unit
        got, want = wl.astype(np.float64), np.asarray(c["window_labels"])
        assert np.abs(got - want).max() <= 1.0001e-3 and (np.abs(got - want) < 1e-6).mean() > 0.995
        if len(boxes):
            clo = labels.closeness_labels(boxes, classes, W, H, K).astype(np.float64)
            cw = np.asarray(c["closeness"])
            assert np.abs(clo - cw).max() <= 1.0001e-3 and (np.abs(clo - cw) < 1e-6).mean() > 0.995
            frac = labels._window_area_fraction(boxes, [0, 0, H, W])
            assert abs(frac - c["union_area_fraction"]) < 1e-9
        em = labels.edgemask(boxes, W, H)
        np.testing.assert_array_equal(em[0].astype(int), np.asarray(c["edgemask_fg"]))
        np.testing.assert_allclose(em[1].astype(np.float64).sum(1), c["edgemask_weight_sum_rows"], rtol=1e-5)
        np.testing.assert_allclose(em[1].astype(np.float64)[::7, ::5], c["edgemask_weight_probe"], rtol=1e-5)


def test_label_generator_properties():
    """Property checks of the label generators (a Monte-Carlo estimate of the union area; distributions)."""
    from mtl_ssl_amd import labels
    rng = np.random.RandomState(0)
    boxes = rng.uniform(0, 1, (6, 4))
    boxes = np.stack([np.minimum(boxes[:, 0], boxes[:, 2]), np.minimum(boxes[:, 1], boxes[:, 3]),
                      np.maximum(boxes[:, 0], boxes[:, 2]), np.maximum(boxes[:, 1], boxes[:, 3])], 1)
    # Monte-Carlo check of the exact union area
    pts = rng.uniform(0, 1, (200000, 2))
    inside = np.zeros(len(pts), bool)
    for b in boxes:
        inside |= (pts[:, 0] > b[0]) & (pts[:, 0] < b[2]) & (pts[:, 1] > b[1]) & (pts[:, 1] < b[3])
    assert abs(labels.union_area(boxes) - inside.mean()) < 5e-3
    assert labels.union_area(np.zeros((0, 4))) == 0.0
    # window labels are a distribution; a window disjoint from every object is pure background
    abs_b = np.array([[10, 10, 60, 60], [40, 40, 100, 120]], float)
    lab, bg = labels.window_label(abs_b, [1, 3], [0, 0, 200, 300], 5)
    assert abs(lab.sum() - 1) < 2e-3 and lab[2] == 0 and lab[1] > 0 and lab[3] > 0
    lab, bg = labels.window_label(abs_b, [1, 3], [150, 150, 200, 300], 5)
    assert bg == 1.0 and lab[0] == 1.0
    clo = labels.closeness_labels(abs_b, [1, 3], 300, 200, 5)
    assert clo.shape == (2, 6) and abs(clo[0].sum() - 1) < 2e-3 and clo[0, 3] > 0 and clo[0, 1] == 0
    assert labels.closeness_labels(abs_b[:1], [1], 300, 200, 5)[0, 0] == 1
    em = labels.edgemask(abs_b, 300, 200)
    assert em.shape == (2, 64, 64) and abs(em[1].mean() - 1) < 1e-5 and em[0].max() == 1


def _dp_worker(rank, world, port, out):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from mtl_ssl_amd import trainer
    from mtl_ssl_amd.params import ParamStore
    ps = ParamStore()
    names = ["a/weights", "b/weights", "b/biases", "c/weights", "d/weights", "e/weights"]
    for n, shape in zip(names, [(300, 7), (1000,), (10,), (40, 40), (3, 3, 16, 16), (700,)]):
        ps.add(n, shape, ("truncated_normal", 0.1))
    ps.add("c/frozen", (5,), ("zeros",), trainable=False)
    ps.finalize("cpu", seed=0)
    from mtl_ssl_amd.comm import GlooComm
    red = trainer.GradientReducer(ps, GlooComm(), bucket_bytes=4096)       # several variable-aligned buckets
    assert len(red.buckets) > 2 and red.buckets[0][0] == 0 and red.buckets[-1][1] == ps.n_train
    assert all(red.buckets[i][1] == red.buckets[i + 1][0] for i in range(len(red.buckets) - 1))
    g = torch.arange(ps.n_train, dtype=torch.float32) * (rank + 1) / world   # clone loss is scaled 1/N
    ps.grads.copy_(g)
    red.all_reduce()
    res = {"flat": ps.grads.clone().numpy()}
    # overlapped form: variables report in backward order (last created first); a bucket is reduced
    # the moment its last variable has reported, the rest at finish()
    ps.grads.copy_(g)
    red.begin_step()
    for n in reversed(names[2:]):
        ps.grad_ready(ps.by_name[n])
        ps.grad_ready(ps.by_name[n])                           # a repeated report is ignored
    early = list(red.launch_order)
    red.finish()
    res["overlap"] = ps.grads.clone().numpy()
    res["order"] = list(red.launch_order)
    # per-bucket form (the optimizer runs bucket by bucket behind each bucket's all-reduce): the same reports, then the
    # generator yields every bucket exactly once, in issue order, and a bucket's slice holds the cross-replica SUM at
    # the moment it is yielded — while it is being "updated" the later buckets may still be on the wire
    ps.grads.copy_(g)
    red.begin_step()
    for n in reversed(names[2:]):
        ps.grad_ready(ps.by_name[n])
    yielded, summed_at_yield = [], []
    expect = torch.arange(ps.n_train, dtype=torch.float32) * (1 + 2) / 2
    for b in red.finish_by_bucket():
        s0, e0 = red.buckets[b]
        yielded.append(b)
        summed_at_yield.append(bool(torch.allclose(ps.grads[s0:e0], expect[s0:e0], rtol=1e-6)))
        ps.grads[s0:e0].zero_()                                  # the update consumes (and zeroes) its slice
    res["by_bucket"] = (yielded, list(red.launch_order), summed_at_yield, float(ps.grads.abs().max()))
    # the per-bucket tables partition the variables in order; a per-variable clip + momentum update applied bucket by
    # bucket (in ANY order) gives the bits of the update applied to all variables at once
    tabs = trainer.bucket_update_tables(ps, red.buckets)
    res["tabs_cover"] = [(v0, v1) for v0, v1, _, _ in tabs]
    from oracle import optimizer as OO
    rng = np.random.RandomState(7)
    vals = {sp.name: rng.randn(*sp.shape).astype(np.float32) for sp in ps.trainable_specs}
    grads = {k: (rng.randn(*v.shape) * 3).astype(np.float32) for k, v in vals.items()}
    acc = {k: rng.randn(*v.shape).astype(np.float32) for k, v in vals.items()}
    mono_v, mono_a = {k: v.copy() for k, v in vals.items()}, {k: v.copy() for k, v in acc.items()}
    OO.momentum_update(mono_v, grads, mono_a, 0.01, 0.9, 10.0)
    bk_v, bk_a = {k: v.copy() for k, v in vals.items()}, {k: v.copy() for k, v in acc.items()}
    for b in reversed(range(len(tabs))):
        v0, v1, rel, mx = tabs[b]
        nm = [sp.name for sp in ps.trainable_specs[v0:v1]]
        assert rel[0] == 0 and rel[-1] == red.buckets[b][1] - red.buckets[b][0] and mx == max(np.diff(rel))
        sub_v, sub_a = {k: bk_v[k] for k in nm}, {k: bk_a[k] for k in nm}
        OO.momentum_update(sub_v, {k: grads[k] for k in nm}, sub_a, 0.01, 0.9, 10.0)
        bk_v.update(sub_v); bk_a.update(sub_a)
    res["bucket_update_identical"] = all(np.array_equal(mono_v[k], bk_v[k]) and np.array_equal(mono_a[k], bk_a[k]) for k in vals)
    # the step loop's collective failure verdict: rank 1 alone sees a problem, both ranks learn of it
    res["verdict"] = trainer.collective_verdict(GlooComm(), 2 if rank == 1 else 0, "cpu")
    res["verdict_ok"] = trainer.collective_verdict(GlooComm(), 0, "cpu")
    # default_comm's fallback: the library's RCCL wrapper fails on ONE rank -> both ranks agree over the host channel,
    # the rank that did get a communicator closes it, and both continue on a torch.distributed group
    from mtl_ssl_amd import comm as C

    class _Fake:
        closed = False

        def __init__(self, device, r, w):
            if r == 1:
                raise RuntimeError("simulated: librccl.so cannot be loaded")
            _Fake.last = self

        def close(self):
            _Fake.closed = True
    real, C.RcclComm, C._FALLBACK_BACKEND = C.RcclComm, _Fake, "gloo"
    fb = C.default_comm(torch.device("cuda", 0))
    C.RcclComm = real
    t = torch.full((5,), float(rank + 1))
    fb.allreduce(t)
    res["fallback"] = (type(fb).__name__, fb.info()["backend"], t.tolist(), _Fake.closed if rank == 0 else None)
    # RcclComm's precondition agreement (before the collective mtlssl_comm_init): one rank that cannot load RCCL or see
    # its device makes EVERY rank raise, nobody is left inside ncclCommInitRank; and the wrapper reports its group's backend
    res["agree"] = (C._dist_agree(rank == 1), C._dist_agree(False), fb.backend, GlooComm().backend)
    res["early"] = early
    res["nb"] = len(red.buckets)
    out[rank] = res
    dist.destroy_process_group()


def test_data_parallel_gradient_sum_gloo_world2():
    """slim/deployment/model_deploy.py:414-444: gradients of the (1/N-scaled) clone losses are
    summed across replicas. Two CPU processes over gloo, bucketed all-reduce of the flat buffer."""
    import torch.multiprocessing as mp
    mgr = mp.Manager()
    out = mgr.dict()
    port = 29500 + (os.getpid() % 1000)
    mp.spawn(_dp_worker, args=(2, port, out), nprocs=2, join=True)
    n = len(out[0]["flat"])
    expect = np.arange(n, dtype=np.float32) * (1 + 2) / 2
    for key in ("flat", "overlap"):
        np.testing.assert_allclose(out[0][key], expect, rtol=1e-6)
        np.testing.assert_array_equal(out[0][key], out[1][key])
    # buckets holding only late variables were reduced before finish(), highest offsets first;
    # every bucket exactly once overall
    assert len(out[0]["early"]) >= 1 and out[0]["early"] == sorted(out[0]["early"], reverse=True)
    assert sorted(out[0]["order"]) == list(range(out[0]["nb"]))
    for r in (0, 1):
        yielded, issued, summed, left = out[r]["by_bucket"]
        assert yielded == issued and sorted(yielded) == list(range(out[r]["nb"])) and all(summed) and left == 0.0
        cover = out[r]["tabs_cover"]
        assert cover[0][0] == 0 and cover[-1][1] == 6 and all(cover[i][1] == cover[i + 1][0] for i in range(len(cover) - 1))
        assert out[r]["bucket_update_identical"]
    # trainer.collective_verdict: a failure seen by one rank stops every rank (none is left waiting in an all-reduce)
    assert out[0]["verdict"] == 2 and out[1]["verdict"] == 2 and out[0]["verdict_ok"] == 0 and out[1]["verdict_ok"] == 0
    # comm.default_comm: one rank's RCCL init failure moves BOTH ranks to the torch.distributed fallback
    assert out[0]["fallback"] == ("GlooComm", "torch-gloo (fallback)", [3.0] * 5, True)
    assert out[1]["fallback"] == ("GlooComm", "torch-gloo (fallback)", [3.0] * 5, None)
    assert out[0]["agree"] == (False, True, "gloo", "gloo") and out[1]["agree"] == (False, True, "gloo", "gloo")


def test_rccl_channel_and_priority_knobs(monkeypatch):
    """MTLSSL_COMM_MAX_CHANNELS / _MIN_CHANNELS reach RCCL as NCCL_MAX_NCHANNELS / NCCL_MIN_NCHANNELS unless those are set
    explicitly; MTLSSL_COMM_STREAM_PRIORITY picks the all-reduce stream's priority (default 0: tools/cu_thief_probe.py
    measured a resident kernel on a HIGH-priority stream starving the three compute streams, 55 -> 75 ms/step)."""
    from mtl_ssl_amd import comm as C
    for k in ("NCCL_MAX_NCHANNELS", "NCCL_MIN_NCHANNELS", "MTLSSL_COMM_MAX_CHANNELS", "MTLSSL_COMM_MIN_CHANNELS",
              "MTLSSL_COMM_STREAM_PRIORITY"):
        monkeypatch.delenv(k, raising=False)
    C._apply_rccl_knobs()
    assert "NCCL_MAX_NCHANNELS" not in os.environ and C.comm_stream_priority() == 0
    monkeypatch.setenv("MTLSSL_COMM_MAX_CHANNELS", "8")
    monkeypatch.setenv("NCCL_MIN_NCHANNELS", "2")
    monkeypatch.setenv("MTLSSL_COMM_MIN_CHANNELS", "4")
    monkeypatch.setenv("MTLSSL_COMM_STREAM_PRIORITY", "-1")
    C._apply_rccl_knobs()
    assert os.environ["NCCL_MAX_NCHANNELS"] == "8" and os.environ["NCCL_MIN_NCHANNELS"] == "2"     # explicit NCCL_* wins
    assert C.comm_stream_priority() == -1
    monkeypatch.delenv("NCCL_MAX_NCHANNELS", raising=False)


def test_random_horizontal_flip_known_answers_and_fork_extras():
    """core/preprocessor_test.py:63-66,181-184,357-383 (boxes after mirroring) + the fork's window
    boxes and its edge-mask axis quirk (core/preprocessor.py:340-342)."""
    from mtl_ssl_amd import config, preprocessor
    boxes = np.array([[0.0, 0.25, 0.75, 1.0], [0.25, 0.5, 0.75, 1.0]], np.float32)
    np.testing.assert_allclose(preprocessor.flip_boxes(boxes), [[0.0, 0.0, 0.75, 0.75], [0.25, 0.0, 0.75, 0.5]])
    img = np.arange(2 * 3 * 3, dtype=np.float32).reshape(2, 3, 3)
    wins = np.array([[0.1, 0.0, 0.2, 0.4]], np.float32)
    em = np.arange(2 * 4 * 4, dtype=np.float32).reshape(2, 4, 4)
    i2, b2, w2, e2 = preprocessor.random_horizontal_flip(img, boxes, wins, em, do_flip=True)
    np.testing.assert_array_equal(i2, img[:, ::-1])
    np.testing.assert_allclose(w2, [[0.1, 0.6, 0.2, 1.0]])
    np.testing.assert_array_equal(e2, em[:, ::-1])                      # rows reversed, like the reference
    e3 = preprocessor.random_horizontal_flip(img, boxes, wins, em, do_flip=True, reference_edgemask_axis=False)[3]
    np.testing.assert_array_equal(e3, em[:, :, ::-1])
    same = preprocessor.random_horizontal_flip(img, boxes, wins, em, do_flip=False)
    assert same[0] is not None and np.array_equal(same[0], img) and np.array_equal(same[1], boxes)
    # no boxes -> never flipped (:302-304)
    noflip = preprocessor.random_horizontal_flip(img, np.zeros((0, 4), np.float32), do_flip=True)
    np.testing.assert_array_equal(noflip[0], img)
    # ~half of the draws flip; driven by the parsed config options
    cfg = _cfg("frcnn_resnet101_coco_mtl.config")
    rng = np.random.RandomState(0)
    ex = dict(image=img, groundtruth_boxes=boxes, window_boxes=wins, groundtruth_edgemask=em)
    flips = sum(not np.array_equal(preprocessor.preprocess(ex, cfg.train_config.data_augmentation_options, rng)["image"], img)
                for _ in range(400))
    assert 150 < flips < 250
    with pytest.raises(ValueError, match="not supported"):
        preprocessor.preprocess(ex, [{"random_crop_image": {}}])


def test_train_launcher_reads_the_reference_flag_forms(tmp_path):
    """object_detection/train.py:101-155: one pipeline file, or --model/--train/--input config files; record
    globs of tf_record_input_reader.input_path; clone / parameter-server flags are refused, not ignored."""
    from mtl_ssl_amd import train
    text = open(os.path.join(ROOT, "configs", "smoke_resnet50_mtl.config")).read()
    for i in range(3):
        (tmp_path / ("voc-%05d-of-00003.record" % i)).write_bytes(b"")
    reader = 'tf_record_input_reader { input_path: "%s" }' % str(tmp_path / "voc-?????-of-00003.record")
    pipe = tmp_path / "pipeline.config"
    pipe.write_text(text + "\ntrain_input_reader { %s }\n" % reader)
    f = train._flags(["--logtostderr", "--train_dir=/x", "--pipeline_config_path=%s" % pipe])
    model_cfg, train_cfg, input_cfg = train.read_configs(f)
    assert model_cfg.faster_rcnn.num_classes == 5 and int(train_cfg.batch_size) == 2
    assert [os.path.basename(p) for p in train.record_paths(input_cfg)] == ["voc-%05d-of-00003.record" % i for i in range(3)]
    # the three-file form gives the same messages
    from mtl_ssl_amd import config
    whole = config.parse_pipeline_config(pipe.read_text())

    def body(field):
        s = pipe.read_text()
        a = s.index(field) + len(field)
        a = s.index("{", a) + 1
        depth, i = 1, a
        while depth:
            depth += {"{": 1, "}": -1}.get(s[i], 0)
            i += 1
        return s[a:i - 1]
    for name, field in (("m.cfg", "model"), ("t.cfg", "train_config"), ("i.cfg", "train_input_reader")):
        (tmp_path / name).write_text(body(field))
    f3 = train._flags(["--train_dir", "/x", "--model_config_path", str(tmp_path / "m.cfg"),
                       "--train_config_path", str(tmp_path / "t.cfg"), "--input_config_path", str(tmp_path / "i.cfg")])
    m3, t3, i3 = train.read_configs(f3)
    assert m3 == whole.model and t3 == whole.train_config and train.record_paths(i3) == train.record_paths(input_cfg)
    with pytest.raises(FileNotFoundError):
        train.record_paths(config.parse_pipeline_config('train_input_reader { tf_record_input_reader { input_path: "/nowhere/*.rec" } }').train_input_reader)
    with pytest.raises(ValueError):
        train.record_paths(config.Msg())
    for bad in (["--num_clones=8"], ["--ps_tasks=1"], ["--worker_replicas=2"]):
        with pytest.raises(SystemExit) as e:
            train.main(["--train_dir=/x", "--pipeline_config_path=%s" % pipe] + bad)
        assert "torch.distributed.run" in str(e.value)


def test_optimizer_builder_covers_the_three_optimizers_and_learning_rates():
    """builders/optimizer_builder.py:24-118 + protos/optimizer.proto defaults: momentum / rms_prop / adam with
    constant, manual-step and exponential-decay rates (tf.train.exponential_decay, staircase on by default)."""
    from mtl_ssl_amd import config, trainer

    def opt(text):
        return trainer.optimizer_from_config(config.parse_pipeline_config("train_config { optimizer { %s } }" % text).train_config.optimizer)
    o = opt("rms_prop_optimizer { learning_rate { exponential_decay_learning_rate { initial_learning_rate: 0.004 decay_steps: 100 decay_factor: 0.5 } } }")
    assert o["kind"] == "rms_prop" and (o["decay"], o["momentum"], o["epsilon"]) == (0.9, 0.9, 1.0)
    assert [o["lr_fn"](s) for s in (0, 99, 100, 250)] == [0.004, 0.004, 0.002, 0.001]           # staircase
    o = opt("adam_optimizer { beta2: 0.99 learning_rate { exponential_decay_learning_rate { decay_steps: 100 decay_factor: 0.5 staircase: false } } }")
    assert o["kind"] == "adam" and (o["beta1"], o["beta2"], o["epsilon"]) == (0.9, 0.99, 1e-8)
    assert abs(o["lr_fn"](50) - 0.002 * 0.5 ** 0.5) < 1e-12
    o = opt("momentum_optimizer { momentum_optimizer_value: 0.8 learning_rate { constant_learning_rate { learning_rate: 0.01 } } }")
    assert o["kind"] == "momentum" and o["momentum"] == 0.8 and o["lr_fn"](12345) == 0.01
    with pytest.raises(ValueError):
        opt("")


def test_oracle_rmsprop_and_adam_known_answers():
    """Hand-computed single steps of tf.train.RMSPropOptimizer (mean square starts at one) and AdamOptimizer."""
    from oracle import optimizer as O
    v, ms, mom = {"w": np.array([1.0, -2.0], np.float32)}, {}, {}
    O.rmsprop_update(v, {"w": np.array([0.5, -1.0], np.float32)}, ms, mom, lr=0.1, decay=0.9, momentum=0.0, epsilon=1.0, clip_norm=0.0)
    s = 0.9 + 0.1 * np.array([0.25, 1.0])
    np.testing.assert_allclose(ms["w"], s, rtol=1e-6)
    np.testing.assert_allclose(v["w"], np.array([1.0, -2.0]) - 0.1 * np.array([0.5, -1.0]) / np.sqrt(s + 1.0), rtol=1e-6)
    v, m, vv = {"w": np.array([1.0, -2.0], np.float32)}, {}, {}
    O.adam_update(v, {"w": np.array([0.5, -1.0], np.float32)}, m, vv, step=1, lr=0.1, beta1=0.9, beta2=0.999, epsilon=1e-8, clip_norm=0.0)
    np.testing.assert_allclose(v["w"], np.array([0.9, -1.9]), rtol=1e-5)      # the first Adam step moves every weight by lr


def _reference_vectors():
    import json
    with open(os.path.join(ROOT, "tests", "golden", "reference_vectors.json")) as f:
        return json.load(f)


def test_manual_stepping_on_the_reference_vector():
    """utils/learning_schedules_test.py:42-56: boundaries [2, 3, 7], rates [1, 2, 3, 4], steps 0..9."""
    from mtl_ssl_amd import trainer
    v = _reference_vectors()["manual_stepping"]
    got = [trainer.manual_stepping(s, v["boundaries"], v["rates"]) for s in range(len(v["expected"]))]
    assert got == v["expected"]


def test_variable_filters_on_the_reference_vectors():
    """utils/variables_helper_test.py:32-126: filter_variables with and without `invert` (empty patterns ignored),
    multiply_gradients_matching_regex and freeze_gradients_matching_regex — as name filters and as the per-variable
    multiplier table the fused update takes (negative = left out of the update)."""
    from mtl_ssl_amd import config, trainer
    from mtl_ssl_amd.params import ParamStore
    v = _reference_vectors()["variables_helper"]
    names = v["names"]
    for c in v["filter"]:
        assert trainer.filter_variable_names(names, c["regex"], invert=c["invert"]) == [names[i] for i in c["kept"]]
    for c in v["multiply"]:
        hit = trainer.filter_variable_names(names, c["regex"], invert=True)
        got = [g * (c["multiplier"] if n in hit else 1.0) for g, n in zip(v["grads"], names)]
        assert got == c["expected"]
    ps = ParamStore()
    for n in names:
        ps.add(n, (2,), ("zeros",))
    ps.finalize("cpu")
    assert [sp.name for sp in ps.trainable_specs] == names
    fz = v["freeze"]
    tc = config.parse_pipeline_config("train_config { batch_size: 1 %s }" % " ".join(
        "freeze_variables: '%s'" % r for r in fz["regex"])).train_config
    m = trainer.gradient_multipliers(ps, tc).numpy()
    assert [i for i in range(len(names)) if m[i] >= 0] == fz["kept"]
    # the second multiply case is trainer.py:399-403's bias multiplier ('.*/biases'); 0.0 means "unset" there
    # (a proto float tested for truth), so the selection is checked with another factor
    tc = config.parse_pipeline_config("train_config { batch_size: 1 bias_grad_multiplier: 2.0 }").train_config
    m = trainer.gradient_multipliers(ps, tc).numpy()
    want_hit = [e == 0.0 for e in v["multiply"][1]["expected"]]
    assert [x == 2.0 for x in m] == want_hit
    # an empty pattern in freeze_variables freezes nothing (filter(None, ...) at variables_helper.py:45)
    tc = config.parse_pipeline_config("train_config { batch_size: 1 freeze_variables: '' }").train_config
    assert trainer.gradient_multipliers(ps, tc) is None


def test_gpu_suite_order_keeps_kernel_parity_ahead_of_whole_model_cases():
    """tests/conftest.py pytest_collection_modifyitems: under `-x` one failing whole-model case must not hide the
    kernel-level parity evidence of any SURVEY §8 row (172 tests never ran). Collected order of the
    GPU suite: every kernel-level test before the first whole-model step test, every small-model test before the
    first full-size case, configs[1] (the benchmark) first among the full-size cases, properties / e2e / bench last."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests"), "-m", "gpu", "--collect-only", "-q"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    ids = [l.strip() for l in r.stdout.splitlines() if "::" in l]
    assert len(ids) > 390, r.stdout[-2000:]
    mod = lambda i: i.split("::")[0].split("/")[-1][:-3]
    whole = lambda i: any(w in i.split("::")[1] for w in ("_step", "detector_inference", "trainer_"))
    kernel_modules = {"test_gpu_detection", "test_gpu_conv_ops", "test_gpu_winograd", "test_gpu_mobilenet", "test_gpu_inception",
                      "test_gpu_postprocess", "test_gpu_comm", "test_gpu_split_engine"}
    small_model = {"test_gpu_model", "test_gpu_rfcn", "test_gpu_switches", "test_gpu_multi_rank", "test_gpu_data_parallel"}
    last = {"test_gpu_fullsize_configs", "test_gpu_fullsize", "test_gpu_determinism", "test_gpu_end_to_end", "test_gpu_bench_contract"}
    unnamed = {"test_gpu_plan_table", "test_gpu_head_kernels", "test_gpu_spatial_kernels", "test_gpu_offtable_plans",
               "test_gpu_option_kernels", "test_gpu_fullsize_plans"}   # not in conftest's _ORDER: the slot after the small models
    assert {mod(i) for i in ids} == kernel_modules | small_model | last | {"test_gpu_fullsize_parity"} | unnamed
    first = lambda pred: next(n for n, i in enumerate(ids) if pred(i))
    lastidx = lambda pred: max(n for n, i in enumerate(ids) if pred(i))
    kernel_last = lastidx(lambda i: mod(i) in kernel_modules and not whole(i))
    first_whole = first(lambda i: whole(i) or mod(i) in small_model)
    assert kernel_last < first_whole, (ids[kernel_last], ids[first_whole])
    # the PS-RoI kernel tests of test_gpu_rfcn (row a17) come before any full-size case as well
    full_first = first(lambda i: mod(i) == "test_gpu_fullsize_parity")
    assert lastidx(lambda i: mod(i) in small_model or mod(i) in kernel_modules) < full_first
    assert lastidx(lambda i: mod(i) in small_model) < first(lambda i: mod(i) in unnamed)
    assert lastidx(lambda i: mod(i) in unnamed) < full_first
    assert "configs1_frcnn_resnet101_coco]" in ids[full_first]
    assert lastidx(lambda i: mod(i) == "test_gpu_fullsize_parity") < first(lambda i: mod(i) in last)
