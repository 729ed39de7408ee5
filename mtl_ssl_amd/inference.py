"""Detections from a trained checkpoint: the inference side of object_detection/exporter.py.

    det = Detector.from_export("exported_model")                 # python -m mtl_ssl_amd.export_inference_graph ...
    det = Detector("pipeline.config", "train_dir/model.ckpt")     # or straight from a training directory
    out = det.detect_images([img0, img1])        # uint8 [H,W,3] of any sizes -> one dict per image, in input order
    out = det.detect_encoded([jpeg_bytes])       # JPEG / PNG bytes
    out = det.detect_examples([serialized])      # tf.Example records (only image/encoded is read)
    out = det(inputs)                            # dispatch on the export's input_type

Per call: host decode (PIL, the decoder of input_reader), resized shapes from the configured image resizer, then per
group of images with the same resized shape one pinned uint8 pack, one H2D copy, mtlssl_prepare_images (the legacy
bilinear resize, bit-identical to the host path), preprocess -> predict -> (predict_edgemask) ->
(predict_with_mtl_results) -> postprocess at is_training=False — the program of exporter.py:345-353 and of eval.py.

Each result follows exporter.py:185-233: detection_boxes [max_total_detections, 4] normalised to the image,
detection_scores, detection_classes (the postprocess class + 1, label_id_offset) and num_detections, all float32.
"""
import io
import json
import os

import numpy as np

INPUT_TYPES = ("image_tensor", "encoded_image_string_tensor", "tf_example")
OUTPUT_KEYS = ("detection_boxes", "detection_scores", "detection_classes", "num_detections")
LABEL_ID_OFFSET = 1                                   # exporter.py:214


def decode_image(encoded):
    """JPEG / PNG bytes -> uint8 [H,W,3]: PIL with .convert("RGB") like input_reader.decode_example_uint8, so a
    grayscale image gets 3 equal channels and RGBA loses its alpha (tf.image.decode_image(channels=3),
    exporter.py:153-171). Other formats are refused."""
    from PIL import Image
    try:
        im = Image.open(io.BytesIO(encoded))
    except Exception as e:                             # PIL.UnidentifiedImageError and truncated headers
        raise ValueError("cannot decode image (%d bytes): JPEG or PNG expected (%s)" % (len(encoded), e)) from None
    if im.format not in ("JPEG", "PNG"):
        raise ValueError("image format %s is not supported: JPEG or PNG expected" % im.format)
    return np.asarray(im.convert("RGB"))


def image_from_example(serialized):
    """The decoded `image/encoded` of a serialized tf.Example (exporter.py:132-150); no other feature is read."""
    from .input_reader import parse_example
    enc = parse_example(serialized).get("image/encoded")
    if not enc:
        raise ValueError("tf.Example without image/encoded")
    return decode_image(enc[0])


def output_tensors(post):
    """exporter.py:185-233 on the host arrays of model.postprocess: float32 boxes, scores, classes + 1 and counts."""
    if "detection_classes" not in post:
        raise ValueError("the model's postprocess gives no detection_classes (first_stage_only)")
    return {"detection_boxes": np.asarray(post["detection_boxes"], np.float32),
            "detection_scores": np.asarray(post["detection_scores"], np.float32),
            "detection_classes": np.asarray(post["detection_classes"], np.float32) + np.float32(LABEL_ID_OFFSET),
            "num_detections": np.asarray(post["num_detections"]).astype(np.float32)}


def split_outputs(batched):
    """[B, ...] output tensors -> B per-image dicts (num_detections a float32 scalar)."""
    B = batched["num_detections"].shape[0]
    return [{k: (np.float32(v[i]) if k == "num_detections" else v[i]) for k, v in batched.items()} for i in range(B)]


def stack_outputs(results):
    """Per-image dicts -> [B, ...] tensors, the exporter's output nodes for one batch."""
    return {k: np.stack([np.asarray(r[k], np.float32) for r in results]) for k in OUTPUT_KEYS}


def run_grouped(keys, run_group):
    """Calls run_group(indices, key) once per distinct key, in order of first appearance, with the input indices of
    that key; run_group returns one result per index. Returns the results in input order."""
    groups = {}
    for i, k in enumerate(keys):
        groups.setdefault(k, []).append(i)
    out = [None] * len(keys)
    for k, idx in groups.items():
        res = run_group(idx, k)
        if len(res) != len(idx):
            raise RuntimeError("group %s: %d results for %d images" % (k, len(res), len(idx)))
        for i, r in zip(idx, res):
            out[i] = r
    return out


def _check_image(a, i):
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("image %d: uint8 [H,W,3] expected, got %s %s" % (i, a.dtype, a.shape))
    return np.ascontiguousarray(a)


class Detector:
    """A trained model at is_training=False on one GPU. Nothing here moves the model's training state: no step
    counter, no dropout draw, no gradient buffer."""

    _ALIGN = 256

    def __init__(self, pipeline_config, checkpoint, use_moving_averages=None, input_type="image_tensor", device=None,
                 float32_matmul_precision=None):
        """pipeline_config: path of the pipeline text; checkpoint: a state file of this build (`model.ckpt.npz` or
        its prefix) or a TensorFlow V1 / V2 checkpoint. use_moving_averages None = eval_config.use_moving_averages.
        float32_matmul_precision: a name of ops.FP32_ENGINES ("highest", "split", "high", "medium") sets the level of the
        large fp32 GEMMs for the whole PROCESS (ops.set_float32_matmul_precision: it is not a property of this detector,
        and it stays after the detector is gone); None leaves the process's setting alone."""
        if input_type not in INPUT_TYPES:
            raise ValueError("Unknown input type: {}".format(input_type))
        import torch
        import __graft_entry__ as ge
        ge.build()
        from . import checkpoint as ckpt
        from . import config, model_builder
        if float32_matmul_precision is not None:
            from . import ops
            ops.set_float32_matmul_precision(float32_matmul_precision)
        self.torch = torch
        cfg = config.parse_pipeline_config(open(pipeline_config).read())
        if cfg.model.faster_rcnn.first_stage_only:
            raise ValueError("first_stage_only models give proposals without classes; exporter.py:214 needs "
                             "detection_classes")
        if use_moving_averages is None:
            use_moving_averages = bool(cfg.get("eval_config", config.Msg("EvalConfig")).get("use_moving_averages", False))
        self.device = torch.device(device) if device is not None else torch.device("cuda", 0)
        if self.device.type != "cuda":
            raise ValueError("Detector runs on a GPU, got device %s" % self.device)
        specs = model_builder.variable_specs(cfg.model, is_training=False)
        values, self.moving_averages_applied = ckpt.inference_values(specs, checkpoint, use_moving_averages)
        self.model = model_builder.build(cfg.model, False, self.device, seed=0, values=values)
        self.config, self.input_type, self.checkpoint = cfg, input_type, checkpoint
        mtl = cfg.model.get("mtl")
        self._edgemask = mtl is not None and bool(mtl.get("edgemask", False))
        self._refine = mtl is not None and bool(mtl.get("refine", False))
        self._pinned = None

    @classmethod
    def from_export(cls, directory, device=None, float32_matmul_precision=None):
        """The output directory of mtl_ssl_amd.export_inference_graph (its moving averages are already applied).
        float32_matmul_precision: as in the constructor (process-global; None leaves the setting alone)."""
        from .export_inference_graph import FORMAT_VERSION
        with open(os.path.join(directory, "export.json")) as fh:
            meta = json.load(fh)
        if int(meta.get("format_version", -1)) != FORMAT_VERSION:
            raise ValueError("%s: export format %s, this build reads %d"
                             % (directory, meta.get("format_version"), FORMAT_VERSION))
        return cls(os.path.join(directory, "pipeline.config"), os.path.join(directory, "model.ckpt"),
                   use_moving_averages=False, input_type=meta["input_type"], device=device,
                   float32_matmul_precision=float32_matmul_precision)

    def resized_shape(self, height, width):
        return self.model.resized_shape(int(height), int(width), self.config.model.faster_rcnn.image_resizer)

    # ---------------------------------------------------------------- entry points
    def __call__(self, inputs, **kw):
        fn = {"image_tensor": self.detect_images, "encoded_image_string_tensor": self.detect_encoded,
              "tf_example": self.detect_examples}[self.input_type]
        return fn(inputs, **kw)

    def detect_images(self, images, batched=False):
        """images: one uint8 [B,H,W,3] array or a list of uint8 [H,W,3] arrays of any sizes -> one dict per image,
        in input order. batched=True (a [B,H,W,3] array only): the exporter's [B, ...] output tensors instead."""
        if batched and not (isinstance(images, np.ndarray) and images.ndim == 4):
            raise ValueError("batched=True takes one uint8 [B,H,W,3] array")
        res = self._detect([_check_image(a, i) for i, a in enumerate(images)])
        return stack_outputs(res) if batched else res

    def detect_encoded(self, strings):
        """JPEG / PNG bytes (encoded_image_string_tensor)."""
        return self._detect([decode_image(s) for s in strings])

    def detect_examples(self, strings):
        """Serialized tf.Example records (tf_example)."""
        return self._detect([image_from_example(s) for s in strings])

    # ---------------------------------------------------------------- device path
    def _detect(self, images):
        shapes = [self.resized_shape(a.shape[0], a.shape[1]) for a in images]
        return run_grouped(shapes, lambda idx, hw: self._run_group([images[i] for i in idx], *hw))

    def _stage(self, images, OH, OW):
        """One pinned pack [descriptors | pixels] -> one H2D copy -> (device pixels, device descriptors)."""
        torch = self.torch
        from . import ops
        desc, nbytes = ops.image_descs([a.shape[:2] for a in images], [False] * len(images), OH, OW)
        head = -(-desc.nbytes // self._ALIGN) * self._ALIGN
        total = head + nbytes
        if self._pinned is None or self._pinned.numel() < total:
            self._pinned = torch.empty(total + total // 4, dtype=torch.uint8, pin_memory=True)
        host = self._pinned.numpy()
        host[:desc.nbytes] = desc.view(np.uint8)
        off = head
        for a in images:
            host[off:off + a.size] = a.reshape(-1)
            off += a.size
        assert off == total
        dev = torch.empty(total, dtype=torch.uint8, device=self.device)
        dev.copy_(self._pinned[:total], non_blocking=True)
        return dev[head:], dev[:desc.nbytes]

    def _run_group(self, images, OH, OW):
        from . import ops
        m = self.model
        with self.torch.cuda.device(self.device):
            pixels, desc = self._stage(images, OH, OW)
            x = ops.prepare_images(pixels, desc, len(images), OH, OW)
            pd = m.predict(m.preprocess(x))
            if self._edgemask:
                pd = m.predict_edgemask(pd)
            if self._refine:
                pd = m.predict_with_mtl_results(pd)
            post = {k: v.cpu().numpy() for k, v in m.postprocess(pd).items()}    # synchronises: the pack is free
            m.check_device_flags()
        return split_outputs(output_tensors(post))
