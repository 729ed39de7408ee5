"""Random crop / pad augmentation end to end on the GPU: the asynchronous pipeline's device batches against its host
preparer on the records and options of tests/test_geometric_augmentation.py, bit for bit; and a model with every
auxiliary head trained for three steps with aux_labels="generate" from the asynchronous feed and from the host feed,
with the same losses and an edge mask made from the boxes AFTER the crop, at the resized size.

The module shares its name with tests/test_gpu_end_to_end.py on purpose: tests/conftest.py orders the GPU suite by
module name, and these run with the end-to-end stage."""
import os

import numpy as np
import pytest
import torch

from tests.aux_labels.test_gpu_end_to_end import SHAPES, _setup, _write_plain_records
from tests.test_geometric_augmentation import FEED_OPTIONS, K, _opts, assert_same_batches, resized, write_records

pytestmark = pytest.mark.gpu
GEOMETRIC = ["random_horizontal_flip { }", "random_crop_pad_image { min_object_covered: 0.5 max_padded_size_ratio: [1.5, 1.5] }"]


def test_device_batches_equal_the_host_preparer(tmp_path):
    import __graft_entry__ as g
    g.build()
    from mtl_ssl_amd import input_pipeline as IP
    rec = write_records(str(tmp_path / "geo.record"))
    opts = _opts(FEED_OPTIONS)
    out = {}
    for device in ("cpu", "cuda"):
        with IP.InputPipeline([rec], K, 2, opts, rng=np.random.RandomState(9), resized_shape=resized, max_pending=4,
                              device=device, num_workers=2, geometric=True) as pipe:
            out[device] = list(pipe)
    assert all(b["images"].is_cuda for b in out["cuda"])
    assert_same_batches(out["cuda"], out["cpu"])


def test_every_head_trains_on_cropped_and_padded_images_from_both_feeds(tmp_path):
    cfg = _setup("smoke_resnet50_mtl.config")
    from mtl_ssl_amd import labels, model_builder, train, trainer
    from mtl_ssl_amd.frcnn import FasterRCNNMetaArch as M
    Kc = int(cfg.model.faster_rcnn.num_classes)
    rec = str(tmp_path / "plain.record")
    _write_plain_records(rec, SHAPES, Kc, np.random.RandomState(6))
    opts = _opts(GEOMETRIC)
    assert train.geometric_augmentation(opts, cfg.model, "generate")
    with pytest.raises(ValueError, match="--aux_labels=generate"):
        train.geometric_augmentation(opts, cfg.model, "record")
    rz = cfg.model.faster_rcnn.image_resizer
    recorded = {}                                # source id -> the boxes as the record holds them
    for b in train.record_batches("host", [rec], Kc, 2, (), np.random.RandomState(1), torch.device("cuda"), {},
                                  shuffle_buffer=0, resized_shape=lambda h, w: M.resized_shape(h, w, rz)):
        recorded.update(zip(b["source_id"], b["groundtruth_boxes"]))
    assert len(recorded) == len(SHAPES)

    def run(kind):
        model = model_builder.build(cfg.model, True, "cuda", seed=3)
        tr = trainer.Trainer(model, cfg.train_config, 1, aux_labels="generate", aux_num_windows=8)
        stream = train.record_batches(kind, [rec], Kc, 2, opts, np.random.RandomState(1), torch.device("cuda"), {},
                                      loop=True, shuffle_buffer=0, resized_shape=lambda h, w: M.resized_shape(h, w, rz),
                                      prefetch=2, geometric=True)
        try:
            out, first = [], None
            for s in range(3):
                batch = next(stream)
                losses = tr.step(batch)
                torch.cuda.synchronize()
                if first is None:
                    first = batch
                    B, H, W = (int(v) for v in batch["images"].shape[:3])
                    H, W = model.resized_shape(H, W, model.cfg.image_resizer)
                    em = model._edgemask.cpu().numpy()
                    for i in range(B):
                        ex = labels.edgemask_exact(np.asarray(batch["groundtruth_boxes"][i]), H, W)
                        np.testing.assert_array_equal(em[i, 0], ex[0])
                        np.testing.assert_allclose(em[i, 1], ex[1], rtol=1e-6, atol=0)
                out.append({k: float(v.item()) for k, v in losses.items()})
            return out, first
        finally:
            if hasattr(stream, "close"):
                stream.close()

    a, first = run("async")
    b, _ = run("host")
    for losses in a:
        assert all(np.isfinite(v) for v in losses.values()), losses
        assert losses["edgemask_loss"] != 0.0 and losses["window_class_loss"] != 0.0
    assert a == b
    # the boxes the labels were made from are the cropped and padded ones, not the record's (the batches are bucketed
    # by the final frames, so the images are looked up by their source id)
    for sid, boxes in zip(first["source_id"], first["groundtruth_boxes"]):
        assert len(boxes) and not np.array_equal(boxes, recorded[sid]), sid
    assert not any(k in first for k in ("window_boxes", "groundtruth_edgemask", "groundtruth_closeness"))
