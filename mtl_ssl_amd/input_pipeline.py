"""Asynchronous TFRecord input: the batches of `input_reader.batches`, decoded in worker processes a few batches
ahead of the step, augmented and resized on the device.

The reference overlaps its input with the step through parallel readers and prefetch / batch queues
(protos/input_reader.proto:39 `num_readers`, protos/train.proto:57-63 `prefetch_queue_capacity`). Here:

* The consuming process replays the record stream of `input_reader.examples` exactly (rank sharding, the shuffle
  buffer, the fixed number of uniform draws of every listed augmentation option (`preprocessor.Step.draws`), the
  same RandomState in the same order). Only the framing of a TFRecord is read here; the draws do not depend on
  pixels or boxes.
* Worker processes (the `spawn` context: a process that has initialised HIP is never forked, and a worker never
  imports torch) read the record, parse the tf.Example, decode the image to uint8, turn the consumer's draws into
  the image's float32 op parameters (`preprocessor.plan`: flip flags, jitter, colour deltas, patch corners, seeds)
  and apply the label side (flips, box jitter, crops and pads); they return the image, its parameters and the size
  of the frame the program ends in.
* The consumer buckets the decoded examples by the resized shape of that final frame exactly like `batches` (same
  flushes, same remainder).
* On a GPU, a batch is packed into a pinned staging slot (descriptors + op parameters + uint8 pixels), copied in one
  H2D copy and turned into the float32 [B,OH,OW,3] batch on a stream of its own: `ops.prepare_images` when the
  options are flips only, `ops.prepare_images_aug` (the op program before the resize, crops and pads included)
  otherwise. The consumer's stream waits on the batch's event at hand-out. Copies and kernels are launched from the
  consumer's thread, so no second Python thread competes with the step's launch thread. On the CPU, the host preparer
  runs the numpy path (`preprocessor.apply_program`, then `resize_bilinear_legacy`).
"""
import collections
import multiprocessing
import os
import queue
import struct
import time
import traceback

import numpy as np

from . import input_reader, preprocessor


def option_draw_counts(augmentation_options, geometric=False):
    """The uniform draws `preprocessor.preprocess` makes per example for each listed option, in config order
    (refusing what preprocess refuses)."""
    return [s.draws for s in preprocessor.parse_options(augmentation_options, warn=False, geometric=geometric)]


def default_num_workers(num_readers=8, local_ranks=1):
    """`num_readers` decode workers, capped by the CPUs this process may run on shared among the node's local ranks
    (one CPU per rank kept for its launch thread)."""
    cpus = len(os.sched_getaffinity(0))
    return max(1, min(int(num_readers), cpus // max(1, int(local_ranks)) - 1))


def record_spans(path):
    """(payload offset, payload length) of every record of a TFRecord file, from the framing alone. Raises the
    errors `input_reader.read_tfrecord` raises for a truncated file."""
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        pos = 0
        while True:
            f.seek(pos)
            hdr = f.read(8)
            if not hdr:
                return
            if len(hdr) < 8:
                raise IOError("truncated record header in %s" % path)
            (n,) = struct.unpack("<Q", hdr)
            if n > size - (pos + 8):
                raise IOError("truncated or corrupted record (length %d) in %s" % (n, path))
            if pos + 16 + n > size:
                raise IOError("truncated record in %s" % path)
            yield pos + 12, n
            pos += 16 + n


def decode_record(serialized, num_classes, steps, draws, timings=None, geometric=False):
    """-> (example with the uint8 image as decoded and augmented labels, float32 op parameters of the image, the
    (height, width) of the frame after the program). `steps`: the parsed options (preprocessor.parse_options); `draws`:
    the consumer's uniform draws of this record (preprocessor.preprocess takes the same ones up front). The labels are
    flipped / jittered / cropped / padded one action after the other, like the host path (1 - (1 - x) need not be x).
    geometric=True drops the record's frozen auxiliary labels, like preprocess."""
    ex = input_reader.decode_example_uint8(serialized, num_classes, timings)
    image = ex.pop("image")
    params, actions, frame = preprocessor.plan(steps, draws, image.shape[0], image.shape[1],
                                               np.asarray(ex["groundtruth_boxes"], np.float32).reshape(-1, 4),
                                               frame=True)
    ex = preprocessor.apply_labels(preprocessor.drop_aux_fields(ex) if geometric else ex, actions)
    ex["image"] = image
    return ex, params, frame


def _worker_main(tasks, results, num_classes, steps, geometric=False):
    files = {}
    while True:
        task = tasks.get()
        if task is None:
            return
        seq, path, index, offset, length, draws = task
        timings = {}
        try:
            f = files.get(path)
            if f is None:
                f = files[path] = open(path, "rb")
            f.seek(offset)
            data = f.read(length)
            if len(data) != length:
                raise IOError("truncated record")
            ex, params, frame = decode_record(data, num_classes, steps, draws, timings, geometric)
            results.put((seq, ex, (params, frame), timings, None))
        except Exception as e:
            results.put((seq, None, None, timings, "record %d of %s: %s: %s\n%s" % (
                index, path, type(e).__name__, e, traceback.format_exc())))


class InputPipelineError(RuntimeError):
    pass


class _HostPreparer:
    """The host path on the decoded uint8 images: float32 cast, the op program (flips, colour ops, patches),
    resize_bilinear_legacy, collate."""

    def __init__(self, codes):
        self.codes = codes

    def prepare(self, items, OH, OW):
        exs = []
        for ex, (params, _) in items:
            img = preprocessor.apply_program(np.asarray(ex["image"], np.float32), self.codes, params)
            exs.append(dict(ex, image=preprocessor.resize_bilinear_legacy(img, OH, OW)))
        return input_reader.collate(exs)

    def hand_out(self, batch):
        return batch


class _DevicePreparer:
    """Pinned staging ring -> one H2D copy + one mtlssl_prepare_images launch per batch on a dedicated stream (a
    program of flips only: the net flip goes into the descriptor), or mtlssl_prepare_images_aug with the batch's
    [B, P] op parameters staged between the descriptors and the pixels and the scales of each image's final frame (the
    source size unless the program crops or pads) in its descriptor. The whole decoded image is copied even when a crop
    keeps a part of it."""

    _ALIGN = 256

    def __init__(self, device, slots, codes, profile=False):
        import torch
        self.torch = torch
        self.codes = list(codes)
        self.P = preprocessor.num_params(self.codes)
        self.flips_only = all(c == preprocessor.OP_FLIP for c in self.codes)
        self.device = device
        self.stream = torch.cuda.Stream(device)
        self.slots = [None] * slots          # pinned uint8 staging buffers
        self.events = [None] * slots         # the event of the batch that last used the slot
        self.k = 0
        self.profile = profile
        self.timed = []                      # (copy start, copy end / prepare start, prepare end, bytes, pixels)

    def prepare(self, items, OH, OW):
        torch = self.torch
        from . import ops
        if self.flips_only:      # the net mirror of the listed flips (the flip flag is each op's one parameter)
            flips, P = [int(np.count_nonzero(p)) % 2 == 1 for _, (p, _) in items], 0
        else:
            flips, P = [False] * len(items), self.P
        desc, nbytes = ops.image_descs([ex["image"].shape[:2] for ex, _ in items], flips, OH, OW,
                                       [frame for _, (_, frame) in items])
        align = lambda n: -(-n // self._ALIGN) * self._ALIGN
        poff = align(desc.nbytes)
        head = poff + align(len(items) * P * 4)
        total = head + nbytes
        s = self.k % len(self.slots)
        self.k += 1
        if self.events[s] is not None:
            self.events[s].synchronize()     # the slot's previous copy has completed
        buf = self.slots[s]
        if buf is None or buf.numel() < total:
            buf = self.slots[s] = torch.empty(total + total // 4, dtype=torch.uint8, pin_memory=True)
        host = buf.numpy()
        host[:desc.nbytes] = desc.view(np.uint8)
        if P:
            host[poff:poff + len(items) * P * 4] = np.stack([p for _, (p, _) in items]).astype(np.float32).view(np.uint8).reshape(-1)
        off = head
        for ex, _ in items:
            a = np.ascontiguousarray(ex["image"], np.uint8).reshape(-1)
            host[off:off + a.size] = a
            off += a.size
        with torch.cuda.stream(self.stream):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)] if self.profile else None
            dev = torch.empty(total, dtype=torch.uint8, device=self.device)
            if ev:
                ev[0].record(self.stream)
            dev.copy_(buf[:total], non_blocking=True)
            if ev:
                ev[1].record(self.stream)
            if self.flips_only:
                out = ops.prepare_images(dev[head:], dev[:desc.nbytes], len(items), OH, OW)
            else:
                max_H = max(h for ex, (p, _) in items
                            for h, _ in preprocessor.stage_frames(self.codes, p, *ex["image"].shape[:2]))
                out = ops.prepare_images_aug(dev[head:], dev[:desc.nbytes], len(items), OH, OW, self.codes,
                                             dev[poff:head], P, max_H)
            done = torch.cuda.Event(enable_timing=self.profile)
            done.record(self.stream)
        self.events[s] = done
        if ev:
            self.timed.append((ev[0], ev[1], done, total, out.numel() // 3))
        batch = {"images": out}
        batch.update(input_reader.collate_labels([ex for ex, _ in items]))
        return batch, done

    def hand_out(self, staged):
        batch, done = staged
        cur = self.torch.cuda.current_stream(self.device)
        cur.wait_event(done)
        batch["images"].record_stream(cur)
        return batch

    def device_times(self):
        """(seconds of H2D copies, seconds of prepare kernels, bytes copied, output pixels) of the profiled batches."""
        self.torch.cuda.synchronize(self.device)
        c = sum(a.elapsed_time(b) for a, b, _, _, _ in self.timed) / 1e3
        p = sum(b.elapsed_time(d) for _, b, d, _, _ in self.timed) / 1e3
        return c, p, sum(t[3] for t in self.timed), sum(t[4] for t in self.timed)


class InputPipeline:
    """Iterator (and context manager) over the batches `input_reader.batches(...)` yields for the same arguments, with
    `images` already on `device` (ready on the consumer's current stream at hand-out); on a CPU device, the host
    preparer yields exactly batches()'s dicts.

    num_workers: decode processes (default: `default_num_workers()` of 8 readers); local_ranks: ranks on this node
    sharing its CPUs; prefetch: batches decoded / staged ahead of the consumer (train.proto prefetch_queue_capacity);
    geometric: as in input_reader.batches (random crop / pad options run, no frozen auxiliary labels).
    """

    def __init__(self, paths, num_classes, batch_size, augmentation_options=(), rng=None, loop=False, rank=0,
                 world=1, shuffle_buffer=0, resized_shape=None, max_pending=64, drop_remainder=False, device="cpu",
                 num_workers=None, prefetch=10, local_ranks=1, profile=False, geometric=False):
        self.paths = list(paths)
        self.num_classes = int(num_classes)
        self.batch_size = int(batch_size)
        self.options = list(augmentation_options or ())
        self.geometric = bool(geometric)
        self.steps = preprocessor.parse_options(self.options, geometric=self.geometric)
        self.codes = preprocessor.program(self.steps)
        self.n_draws = preprocessor.draw_count(self.steps)
        self.rng = rng if rng is not None else np.random.RandomState(0)
        self.loop, self.rank, self.world, self.shuffle_buffer = loop, rank, world, int(shuffle_buffer)
        self.resized_shape, self.max_pending, self.drop_remainder = resized_shape, int(max_pending), drop_remainder
        self.prefetch = max(1, int(prefetch))
        self.num_workers = int(num_workers) if num_workers else default_num_workers(8, local_ranks)
        self.timings = collections.Counter()          # worker seconds per stage, consumer seconds of packing
        self._records = self._record_stream()
        self._exhausted = False
        self._seq_next = 0                            # next task sequence number
        self._seq_want = 0                            # next result to bucket
        self._done = {}                               # out-of-order results
        self._buckets, self._pending = {}, 0
        self._ready = collections.deque()             # assembled batches: (items, OH, OW)
        self._staged = collections.deque()            # prepared batches awaiting hand-out
        self._procs = []
        self._closed = False
        import torch
        dev = torch.device(device)
        self._preparer = (_HostPreparer(self.codes) if dev.type == "cpu"
                          else _DevicePreparer(dev, self.prefetch + 1, self.codes, profile))
        ctx = multiprocessing.get_context("spawn")
        self._tasks, self._results = ctx.Queue(), ctx.Queue()
        try:
            for _ in range(self.num_workers):
                p = ctx.Process(target=_worker_main, args=(self._tasks, self._results, self.num_classes, self.steps, self.geometric),
                                daemon=True)
                p.start()
                self._procs.append(p)
        except BaseException:
            self.close()
            raise

    # ---------------------------------------------------------------- the record stream of input_reader.examples
    def _record_stream(self):
        rng, world, rank, paths = self.rng, self.world, self.rank, self.paths

        def records():
            i = 0
            while True:
                for p in paths:
                    for k, span in enumerate(record_spans(p)):
                        mine = (i % world) == rank
                        i += 1
                        if mine:
                            yield (p, k) + span
                if not self.loop:
                    return

        def shuffled():
            if self.shuffle_buffer <= 0:
                yield from records()
                return
            buf = []
            for rec in records():
                buf.append(rec)
                if len(buf) > self.shuffle_buffer:
                    j = int(rng.randint(len(buf)))
                    buf[j], buf[-1] = buf[-1], buf[j]
                    yield buf.pop()
            while buf:
                j = int(rng.randint(len(buf)))
                buf[j], buf[-1] = buf[-1], buf[j]
                yield buf.pop()

        for rec in shuffled():
            # preprocessor.preprocess: a fixed number of rng.uniform() per listed option, whatever the pixels or boxes
            yield rec, [float(rng.uniform()) for _ in range(self.n_draws)]

    def _submit(self):
        depth = self.prefetch * self.batch_size + self.num_workers
        while not self._exhausted and self._seq_next - self._seq_want < depth:     # decoded or in flight
            try:
                (path, index, offset, length), draws = next(self._records)
            except StopIteration:
                self._exhausted = True
                break
            self._tasks.put((self._seq_next, path, index, offset, length, draws))
            self._seq_next += 1

    # ---------------------------------------------------------------- bucketing of input_reader.batches
    def _bucket(self, ex, params):
        """`params`: the worker's (op parameters, final frame); the frame is the source size unless a crop / pad moved it."""
        H, W = params[1]
        key = tuple(self.resized_shape(H, W)) if self.resized_shape is not None else (H, W)
        self._buckets.setdefault(key, []).append((ex, params))
        self._pending += 1
        if len(self._buckets[key]) == self.batch_size:
            self._pending -= self.batch_size
            self._ready.append((self._buckets.pop(key), key))
        elif self._pending > self.max_pending:
            key = max(self._buckets, key=lambda k: len(self._buckets[k]))
            self._pending -= len(self._buckets[key])
            self._ready.append((self._buckets.pop(key), key))

    def _next_ready(self, block):
        """The next assembled batch: None at the end of the stream, or (block=False) when none is assembled yet."""
        while not self._ready:
            while self._seq_want in self._done:              # bucket what has arrived, in stream order
                ex, params = self._done.pop(self._seq_want)
                self._seq_want += 1
                self._bucket(ex, params)
            if self._ready:
                break
            self._submit()
            if self._exhausted and self._seq_want == self._seq_next:
                if not self.drop_remainder:
                    for key in sorted(self._buckets):
                        self._ready.append((self._buckets[key], key))
                self._buckets, self._pending = {}, 0
                break
            try:
                seq, ex, params, timings, err = self._results.get(timeout=0.5) if block else self._results.get_nowait()
            except queue.Empty:
                if not block:
                    return None
                dead = [p for p in self._procs if not p.is_alive()]
                if dead:
                    raise InputPipelineError("input worker %d exited with code %s" % (dead[0].pid, dead[0].exitcode))
                continue
            self.timings.update(timings)
            if err is not None:
                raise InputPipelineError("decoding failed: " + err)
            self._done[seq] = (ex, params)
        return self._ready.popleft() if self._ready else None

    def _stage(self, ready):
        items, (OH, OW) = ready
        t0 = time.perf_counter()
        staged = self._preparer.prepare(items, OH, OW)
        self.timings["stage"] += time.perf_counter() - t0
        self._staged.append(staged)

    # ---------------------------------------------------------------- iterator
    def __iter__(self):
        return self

    def __next__(self):
        if self._closed:
            raise StopIteration
        try:
            if not self._staged:
                ready = self._next_ready(block=True)
                if ready is None:
                    self.close()
                    raise StopIteration
                self._stage(ready)
            batch = self._preparer.hand_out(self._staged.popleft())
            # stage what has already been decoded, so that its copy and kernel overlap the step about to run
            while len(self._staged) < self.prefetch:
                ready = self._next_ready(block=False)
                if ready is None:
                    break
                self._stage(ready)
            return batch
        except StopIteration:
            raise
        except BaseException:
            self.close()
            raise

    def queue_fill(self):
        """(batches staged ahead of the consumer, capacity): the prefetch queue's fill for the training summaries
        (the reference's queue/fraction_of_<capacity>_full of its prefetch queue)."""
        return len(self._staged), self.prefetch

    def device_times(self):
        return self._preparer.device_times() if isinstance(self._preparer, _DevicePreparer) else None

    def close(self):
        """Stops the workers (idempotent); no child process outlives it."""
        if getattr(self, "_closed", True) and not getattr(self, "_procs", None):
            return
        self._closed = True
        self._staged.clear()
        self._ready.clear()
        for p in self._procs:
            if p.is_alive():
                p.terminate()
        for p in self._procs:
            p.join(5)
            if p.is_alive():
                p.kill()
                p.join()
        self._procs = []
        for q in (getattr(self, "_tasks", None), getattr(self, "_results", None)):
            if q is None:
                continue
            q.cancel_join_thread()
            q.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
