"""Training launcher with the flags of object_detection/train.py:65-98 — what a user of the reference runs:

    python -m mtl_ssl_amd.train --train_dir=/runs/a --pipeline_config_path=configs/frcnn_resnet101_coco_mtl.config
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m mtl_ssl_amd.train --train_dir=... ...

One process per GPU; data parallelism comes from the launcher's WORLD_SIZE (RCCL all-reduce of the gradient buckets,
trainer.GradientReducer), not from --num_clones / parameter servers: those flags are accepted so existing command
lines keep working, and a value that asks for the reference's in-process clones is refused with the torchrun line
that does the same job."""
import argparse
import glob
import os
import sys

import numpy as np

FLOAT32_MATMUL_PRECISIONS = ("highest", "split", "high", "medium")     # the names of ops.FP32_ENGINES


def _flags(argv):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--master", default="")
    ap.add_argument("--task", type=int, default=0)
    ap.add_argument("--num_clones", type=int, default=1)
    ap.add_argument("--clone_on_cpu", default="false")
    ap.add_argument("--worker_replicas", type=int, default=1)
    ap.add_argument("--ps_tasks", type=int, default=0)
    ap.add_argument("--train_dir", default="")
    ap.add_argument("--train_tag", default="")
    ap.add_argument("--pipeline_config_path", default="")
    ap.add_argument("--train_config_path", default="")
    ap.add_argument("--input_config_path", default="")
    ap.add_argument("--model_config_path", default="")
    ap.add_argument("--logtostderr", action="store_true")
    ap.add_argument("--num_steps", type=int, default=None, help="overrides train_config.num_steps")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--input_pipeline", choices=("async", "host"), default="async",
                    help="async: decode workers + on-device flip / resize (mtl_ssl_amd.input_pipeline); host: the serial "
                         "generator input_reader.batches (the same batches, bit for bit)")
    ap.add_argument("--aux_labels", choices=("record", "generate"), default="record",
                    help="record: window / closeness / edge-mask labels are read from the records (frozen when they were "
                         "written); generate: they are made on the device at every step from the boxes and classes "
                         "alone, with fresh windows per step, so plain detection records train the auxiliary heads")
    ap.add_argument("--save_summaries_secs", type=float, default=None,
                    help="overrides train_config.save_summaries_secs (default 120): seconds between two summaries in "
                         "train_dir's TensorBoard event file; 0 writes none")
    ap.add_argument("--input_state", choices=("resume", "restart"), default="resume",
                    help="resume: a run that continues from train_dir's state file also continues its input stream where "
                         "that file left it (shuffle buffer, draws, waiting images; --input_pipeline=async only); restart: "
                         "the stream starts at the first record again")
    ap.add_argument("--log_every", type=int, default=10, help="steps between two printed loss lines")
    ap.add_argument("--float32_matmul_precision", choices=FLOAT32_MATMUL_PRECISIONS, default=None,
                    help="how the large fp32 GEMMs multiply, for the whole process (ops.set_float32_matmul_precision): "
                         "highest = native fp32 MFMA; split = exact three-piece bf16 split, six products; high = 16 "
                         "significant bits, three products; medium = one bf16 (round-to-nearest-even), one product. "
                         "Not given: the process's setting stays (highest unless MTLSSL_FP32_ENGINE=split)")
    return ap.parse_args(argv)


def read_configs(f):
    """train.py:101-155: one TrainEvalPipelineConfig, or the three separate files."""
    from . import config
    if f.pipeline_config_path:
        return config.get_configs_from_pipeline_file(f.pipeline_config_path)
    if not (f.train_config_path and f.input_config_path and f.model_config_path):
        raise SystemExit("give --pipeline_config_path, or all of --model_config_path --train_config_path --input_config_path")
    parts = []
    for field, path in (("model", f.model_config_path), ("train_config", f.train_config_path),
                        ("train_input_reader", f.input_config_path)):
        parts.append("%s {\n%s\n}" % (field, open(path).read()))
    cfg = config.parse_pipeline_config("\n".join(parts))
    return cfg.model, cfg.train_config, cfg.train_input_reader


def record_paths(input_config):
    """input_reader_builder.py:34-65: tf_record_input_reader.input_path (repeated, glob patterns allowed)."""
    paths = []
    reader = input_config.get("tf_record_input_reader")
    if reader is None:
        raise ValueError("the configuration has no train_input_reader { tf_record_input_reader { input_path: ... } }")
    for pat in reader.input_path:
        hits = sorted(glob.glob(pat))
        if not hits:
            raise FileNotFoundError("train_input_reader: nothing matches %r" % pat)
        paths += hits
    if not paths:
        raise ValueError("train_input_reader.tf_record_input_reader.input_path is empty")
    return paths


def geometric_augmentation(augmentation_options, model_config, aux_labels):
    """Whether the input path may run the options that move the frame (random_crop_image, random_pad_image,
    random_crop_pad_image, ssd_random_crop): they deliver the image and the boxes in the new frame, so the window,
    closeness and edge-mask labels must be made from those boxes (aux_labels="generate") or not be needed at all.
    A config that lists such an option while a head reads its labels from the records is refused here."""
    from . import preprocessor
    mtl = model_config.mtl
    heads = [h for h in ("window", "closeness", "edgemask") if getattr(mtl, h)]
    ok = aux_labels == "generate" or not heads
    listed = [k for k, _ in preprocessor._entries(augmentation_options or ()) if k in preprocessor.GEOMETRIC_KIND]
    if listed and not ok:
        raise ValueError("data augmentation %s moves the image and the boxes, but mtl.%s read%s the labels frozen into the "
                         "records, which would stay in the old frame: train with --aux_labels=generate "
                         "(aux_labels=\"generate\") to make them from the boxes at every step"
                         % (", ".join(repr(k) for k in listed), " / mtl.".join(heads), "s" if len(heads) == 1 else ""))
    return ok


class HostBatches:
    """The serial generator input_reader.batches with `images` copied to `device` at hand-out. With follow_state, a
    pipeline that builds no batches (InputPipeline(device=None), one decode worker) follows the same stream from a
    copy of the RandomState, batch for batch, so that state() is the state the asynchronous pipeline would report
    after as many batches: a state file written by a host-fed run can be continued with --input_pipeline=async. The
    generator itself cannot be continued (there is no restore())."""

    def __init__(self, paths, num_classes, batch_size, augmentation_options, rng, device, follow_state=False,
                 geometric=False, **kw):
        from . import input_pipeline, input_reader
        self.device = device
        self._shadow = None
        if follow_state:
            twin = np.random.RandomState(0)
            twin.set_state((rng if rng is not None else twin).get_state())
            self._shadow = input_pipeline.InputPipeline(paths, num_classes, batch_size, augmentation_options, twin,
                                                        device=None, num_workers=1, prefetch=2, geometric=geometric, **kw)
        self._batches = input_reader.batches(paths, num_classes, batch_size, augmentation_options, rng,
                                             geometric=geometric, **kw)

    def __iter__(self):
        return self

    def __next__(self):
        b = next(self._batches)
        if self._shadow is not None and next(self._shadow) != int(b["images"].shape[0]):
            raise RuntimeError("the pipeline following the host generator's stream has left it")
        b["images"] = b["images"].to(self.device, non_blocking=True)
        return b

    def state(self):
        """InputPipeline.state() of the stream as of the last batch handed out; None without follow_state."""
        return None if self._shadow is None else self._shadow.state()

    def close(self):
        if self._shadow is not None:
            self._shadow.close()


def record_batches(kind, paths, num_classes, batch_size, augmentation_options, rng, device, input_config,
                   prefetch=10, geometric=False, follow_state=False, **kw):
    """The batches of input_reader.batches with `images` on `device`: 'async' = mtl_ssl_amd.input_pipeline
    (input_reader.proto num_readers decode workers, train.proto prefetch_queue_capacity batches ahead), 'host' = the
    serial generator, images copied at hand-out (follow_state: see HostBatches). geometric: see
    geometric_augmentation."""
    from . import input_pipeline, input_reader
    if kind == "async":
        local = int(os.environ.get("LOCAL_WORLD_SIZE", "1"))
        workers = input_pipeline.default_num_workers(int(input_config.get("num_readers", 8) or 8), local)
        return input_pipeline.InputPipeline(paths, num_classes, batch_size, augmentation_options, rng, device=device,
                                            num_workers=workers, prefetch=max(1, prefetch), geometric=geometric, **kw)
    if kind != "host":
        raise ValueError("input pipeline %r: async or host" % kind)

    return HostBatches(paths, num_classes, batch_size, augmentation_options, rng, device, follow_state, geometric, **kw)


def main(argv=None):
    f = _flags(sys.argv[1:] if argv is None else argv)
    if f.num_clones != 1 or f.worker_replicas != 1 or f.ps_tasks != 0:
        raise SystemExit("clones / parameter servers are replaced by one process per GPU:\n  python -m torch.distributed.run "
                         "--nproc-per-node %d --master-addr 127.0.0.1 -m mtl_ssl_amd.train --train_dir=%s ..."
                         % (max(f.num_clones * f.worker_replicas, 2), f.train_dir or "DIR"))
    if not f.train_dir:
        raise SystemExit("--train_dir is required")
    import torch
    import torch.distributed as dist
    import __graft_entry__ as ge
    from . import model_builder, trainer
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if rank == 0:
        ge.build()
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        dist.init_process_group("gloo")            # bootstrap + barriers; gradients travel over RCCL (mtl_ssl_amd.comm)
        dist.barrier()
    torch.cuda.set_device(local % max(torch.cuda.device_count(), 1))
    dev = torch.device("cuda", torch.cuda.current_device())
    model_config, train_config, input_config = read_configs(f)
    total_configs = (model_config, train_config, input_config)        # train.py:200-204: five with a pipeline file
    if f.pipeline_config_path:
        from . import config
        whole = config.parse_pipeline_config(open(f.pipeline_config_path).read())
        total_configs += (whole.get("eval_config"), whole.get("eval_input_reader"))
    K = int(model_config.faster_rcnn.num_classes)
    B = int(train_config.batch_size)
    if world > 1:                                    # train_config.batch_size is the GLOBAL batch: every clone of the
        if B % world:                                # reference takes batch_size // num_clones images (trainer.py:270)
            raise SystemExit("train_config.batch_size %d does not divide over %d ranks" % (B, world))
        B //= world
    try:
        geometric = geometric_augmentation(train_config.data_augmentation_options, model_config, f.aux_labels)
    except ValueError as e:
        raise SystemExit(str(e))
    probe = model_builder.build(model_config, True, dev, seed=f.seed)
    rz = model_config.faster_rcnn.image_resizer
    stream = record_batches(f.input_pipeline, record_paths(input_config), K, B, train_config.data_augmentation_options,
                            np.random.RandomState(f.seed + rank), dev, input_config, loop=True, rank=rank, world=world,
                            # protos/input_reader.proto: shuffle (default true) draws from a queue that holds
                            # at least min_after_dequeue (default 1000) serialized records
                            shuffle_buffer=int(input_config.get("min_after_dequeue", 1000) or 0)
                            if input_config.get("shuffle", True) else 0,
                            resized_shape=lambda h, w: probe.resized_shape(h, w, rz),
                            max_pending=64 if world == 1 else 256,
                            prefetch=int(train_config.prefetch_queue_capacity), geometric=geometric,
                            follow_state=True)

    def next_batch():
        return next(stream)
    os.makedirs(f.train_dir, exist_ok=True)
    if (rank == 0 and f.input_pipeline == "host" and f.input_state == "resume"
            and os.path.exists(os.path.join(f.train_dir, "model.ckpt.npz"))):
        print("warning: --input_pipeline=host cannot continue its input stream: weights and step are resumed, the "
              "records restart at the first one (--input_pipeline=async continues it)")
    if rank == 0 and f.pipeline_config_path:          # train.py:235-247 keeps the configuration beside the checkpoints
        with open(os.path.join(f.train_dir, "pipeline.config"), "w") as out:
            out.write(open(f.pipeline_config_path).read())
    try:
        trainer.train(next_batch, lambda: probe, train_config, master=f.master, task=rank, num_clones=1,
                      worker_replicas=world, is_chief=rank == 0, train_dir=f.train_dir, model_config=model_config,
                      num_steps=f.num_steps, aux_labels=f.aux_labels, save_summaries_secs=f.save_summaries_secs,
                      total_configs=total_configs, input_queue=stream, input_state=f.input_state,
                      log_every=max(1, f.log_every), float32_matmul_precision=f.float32_matmul_precision)
    finally:
        if hasattr(stream, "close"):
            stream.close()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
