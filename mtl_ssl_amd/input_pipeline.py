"""Asynchronous TFRecord input: the batches of `input_reader.batches`, decoded in worker processes a few batches
ahead of the step, augmented and resized on the device.

The reference overlaps its input with the step through parallel readers and prefetch / batch queues
(protos/input_reader.proto:39 `num_readers`, protos/train.proto:57-63 `prefetch_queue_capacity`). Here:

* The consuming process replays the record stream of `input_reader.examples` exactly (rank sharding, the shuffle
  buffer, the fixed number of uniform draws of every listed augmentation option (`preprocessor.Step.draws`), the
  same RandomState in the same order). Only the framing of a TFRecord is read here; the draws do not depend on
  pixels or boxes. That stream is small references and numbers, so `InputPipeline.state()` can describe it as of the
  last batch handed out in a few kilobytes of JSON, and `restore()` continues it in another process.
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
import itertools
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


class InputStateMismatch(ValueError):
    """A stream state was taken by a pipeline defined differently from the one asked to continue it; `field` names the
    first entry of the definition that differs."""

    def __init__(self, field, was, now):
        ValueError.__init__(self, "the input state was taken with another %s (%r, this pipeline has %r)" % (field, was, now))
        self.field = field


STATE_VERSION = 1


def _plain(v):
    """Parsed option arguments as JSON would give them back: lists for tuples, Python scalars for numpy's."""
    if hasattr(v, "keys"):
        return {str(k): _plain(v[k]) for k in v.keys()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    return v.item() if isinstance(v, np.generic) else v


def _rng_to_json(st):
    name, key, pos, has_gauss, cached = st
    return [str(name), [int(x) for x in key], int(pos), int(has_gauss), float(cached)]


def _rng_from_json(st):
    return (str(st[0]), np.asarray(st[1], np.uint32), int(st[2]), int(st[3]), float(st[4]))


class _RecordStream:
    """The record stream of `input_reader.examples` as an object whose whole state is plain data: rank sharding over
    the files, the shuffle buffer, then the fixed number of uniform draws per record, from the same RandomState in the
    same order. An item is (path, index, offset, length) and its draws. `cursor()` is the state outside the shuffle
    buffer and the RandomState; every item also comes with the numbers that undo its step on the buffer and repeat its
    calls of the RandomState (`undo`), so a consumer that lets the stream run ahead can still name the state after any
    recent item without copying the buffer or the RandomState's 624 words per item."""

    def __init__(self, paths, rng, loop, rank, world, shuffle_buffer, n_draws):
        self.paths, self.rng, self.loop, self.rank, self.world = paths, rng, loop, rank, world
        self.shuffle_buffer, self.n_draws = shuffle_buffer, n_draws
        self.epoch, self.file, self.record, self.i = 0, 0, 0, 0     # pass over the files; the next record; stream counter
        self.buf, self.draining = [], False
        self._spans = None                                          # open iterator over paths[file], at `record`

    def _next_record(self):
        """records() of input_reader.examples: the next record of this rank, None at the end of a non-looping stream."""
        while True:
            if self._spans is None:
                if self.file >= len(self.paths):
                    if not self.loop:
                        return None
                    self.epoch, self.file, self.record = self.epoch + 1, 0, 0
                    if not self.paths:
                        return None
                self._spans = itertools.islice(record_spans(self.paths[self.file]), self.record, None)
            span = next(self._spans, None)
            if span is None:
                self._spans, self.file, self.record = None, self.file + 1, 0
                continue
            k, mine = self.record, (self.i % self.world) == self.rank
            self.record += 1
            self.i += 1
            if mine:
                return (self.paths[self.file], k) + span

    def next(self):
        """-> (record, draws, undo) or None. undo = (records appended to the buffer, index drawn, the buffer's length
        then), None without a buffer."""
        undo = None
        if self.shuffle_buffer <= 0:
            rec = self._next_record()
        else:
            buf, grown, rec = self.buf, 0, None
            while not self.draining and rec is None:
                new = self._next_record()
                if new is None:
                    self.draining = True
                    break
                buf.append(new)
                grown += 1
                if len(buf) > self.shuffle_buffer:
                    rec = self._draw()
            if rec is None and buf:
                rec = self._draw()
            if rec is not None:
                undo = (grown,) + rec[1:]
                rec = rec[0]
        if rec is None:
            return None
        # preprocessor.preprocess: a fixed number of rng.uniform() per listed option, whatever the pixels or boxes
        return rec, [float(self.rng.uniform()) for _ in range(self.n_draws)], undo

    def _draw(self):
        buf = self.buf
        n = len(buf)
        j = int(self.rng.randint(n))
        buf[j], buf[-1] = buf[-1], buf[j]
        return buf.pop(), j, n

    def cursor(self):
        return (self.epoch, self.file, self.record, self.i, self.draining)

    def repeat_calls(self, rng, undo):
        """Advance `rng` (a copy of the RandomState as it was before an item) by the calls that item made."""
        if undo is not None:
            rng.randint(undo[2])
        for _ in range(self.n_draws):
            rng.uniform()

    def rewound(self, items):
        """A copy of the shuffle buffer as it was before `items` (the latest (record, undo) pairs, oldest first)."""
        buf = list(self.buf)
        for rec, undo in reversed(items):
            if undo is None:
                continue
            grown, j, _ = undo
            buf.append(rec)
            buf[j], buf[-1] = buf[-1], buf[j]
            if grown:
                del buf[-grown:]
        return buf

    def restore(self, cursor, rng_state, buf):
        self.epoch, self.file, self.record, self.i, self.draining = cursor
        self.rng.set_state(rng_state)
        self.buf, self._spans = list(buf), None


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


class _NoPreparer:
    """device=None: the pipeline only follows the stream and hands out each batch's size. The training launcher runs
    one beside the serial host generator, batch for batch, to know that generator's stream state."""

    def prepare(self, items, OH, OW):
        return len(items)

    def hand_out(self, size):
        return size


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
    preparer yields exactly batches()'s dicts; with device=None no batch is built and the batch's size is yielded.

    num_workers: decode processes (default: `default_num_workers()` of 8 readers); local_ranks: ranks on this node
    sharing its CPUs; prefetch: batches decoded / staged ahead of the consumer (train.proto prefetch_queue_capacity);
    geometric: as in input_reader.batches (random crop / pad options run, no frozen auxiliary labels).

    `state()` describes the stream as of the last batch handed out, as plain JSON data; a pipeline built with the same
    arguments and given that dict (`state=`, or `restore()` before the first batch) continues with exactly the
    batches this one would have handed out next. The description does not depend on num_workers, prefetch or timing.
    """

    def __init__(self, paths, num_classes, batch_size, augmentation_options=(), rng=None, loop=False, rank=0,
                 world=1, shuffle_buffer=0, resized_shape=None, max_pending=64, drop_remainder=False, device="cpu",
                 num_workers=None, prefetch=10, local_ranks=1, profile=False, geometric=False, state=None):
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
        self._records = _RecordStream(self.paths, self.rng, self.loop, self.rank, self.world, self.shuffle_buffer,
                                      self.n_draws)
        self._exhausted = False
        self._seq_next = 0                            # next task sequence number = stream items drawn so far
        self._seq_want = 0                            # next result to bucket
        self._done = {}                               # out-of-order results
        self._buckets, self._pending = {}, 0          # key -> [(example, worker's parameters, item's log entry)]
        self._ready = collections.deque()             # assembled batches: (items, key, stream mark)
        self._staged = collections.deque()            # prepared batches awaiting hand-out, each with its mark
        # what state() needs, as references to small tuples: the stream items from `_log_base` on, each (record, draws,
        # undo, the stream's cursor after it); the cursor before the first of them and a RandomState that has made the
        # calls of every item before it; a pipeline continued from a state re-decodes that state's bucket contents
        # first, under the sequence numbers below `_refill[0]` (log entries without a cursor: they move nothing)
        self._log, self._log_base = collections.deque(), 0
        self._cursor_base = self._records.cursor()
        self._rng_base = np.random.RandomState(0)
        self._rng_base.set_state(self.rng.get_state())
        self._refill = (0, {})
        self._resend = collections.deque()            # the log entries of those, until they are sent to the workers
        self._started = False
        # the mark of the last batch handed out: (items bucketed, ((key, log entries in the bucket), ...), exhausted)
        self._mark = (0, (), False)
        self._handed = 0
        self._definition = None
        self._procs = []
        self._closed = False
        if device is None:
            self._preparer = _NoPreparer()
        else:
            import torch
            dev = torch.device(device)
            self._preparer = (_HostPreparer(self.codes) if dev.type == "cpu"
                              else _DevicePreparer(dev, self.prefetch + 1, self.codes, profile))
        ctx = multiprocessing.get_context("spawn")
        self._tasks, self._results = ctx.Queue(), ctx.Queue()
        try:
            if state is not None:
                self.restore(state)
            for _ in range(self.num_workers):
                p = ctx.Process(target=_worker_main, args=(self._tasks, self._results, self.num_classes, self.steps, self.geometric),
                                daemon=True)
                p.start()
                self._procs.append(p)
        except BaseException:
            self.close()
            raise

    def _submit(self):
        depth = self.prefetch * self.batch_size + self.num_workers
        while (self._resend or not self._exhausted) and self._seq_next - self._seq_want < depth:   # decoded or in flight
            if self._resend:
                entry = self._resend.popleft()
            else:
                item = self._records.next()
                if item is None:
                    self._exhausted = True
                    break
                entry = item + (self._records.cursor(),)
            self._log.append(entry)
            self._tasks.put((self._seq_next,) + entry[0] + (entry[1],))
            self._seq_next += 1

    # ---------------------------------------------------------------- bucketing of input_reader.batches
    def _key(self, frame):
        H, W = frame
        return tuple(self.resized_shape(H, W)) if self.resized_shape is not None else (H, W)

    def _passed(self, entry, cursor, rng):
        """The stream's cursor after a log entry, `rng` advanced by the entry's calls."""
        if entry[3] is None:
            return cursor
        self._records.repeat_calls(rng, entry[2])
        return entry[3]

    def _marked(self, exhausted=False):
        """The stream mark of a batch assembled now: where bucketing stands and who waits in which bucket."""
        return (self._seq_want, self._waiting(self._buckets, self._buckets), exhausted)

    @staticmethod
    def _waiting(buckets, keys):
        """((key, ((log entry, final frame) of every example in that bucket, in order)), ...): references, no copies."""
        return tuple((k, tuple((e, p[1]) for _, p, e in buckets[k])) for k in keys)

    def _bucket(self, seq, ex, params):
        """`params`: the worker's (op parameters, final frame); the frame is the source size unless a crop / pad moved it."""
        entry = self._log[seq - self._log_base]
        if seq < self._refill[0]:                    # a restored state's bucket content goes back where it waited
            self._buckets[self._refill[1][seq]].append((ex, params, entry))
            self._pending += 1
            return
        key = self._key(params[1])
        self._buckets.setdefault(key, []).append((ex, params, entry))
        self._pending += 1
        if len(self._buckets[key]) == self.batch_size:
            self._pending -= self.batch_size
            self._ready.append((self._buckets.pop(key), key, self._marked()))
        elif self._pending > self.max_pending:
            key = max(self._buckets, key=lambda k: len(self._buckets[k]))
            self._pending -= len(self._buckets[key])
            self._ready.append((self._buckets.pop(key), key, self._marked()))

    def _next_ready(self, block):
        """The next assembled batch: None at the end of the stream, or (block=False) when none is assembled yet."""
        while not self._ready:
            while self._seq_want in self._done:              # bucket what has arrived, in stream order
                ex, params = self._done.pop(self._seq_want)
                self._seq_want += 1
                self._bucket(self._seq_want - 1, ex, params)
            if self._ready:
                break
            self._submit()
            if self._exhausted and not self._resend and self._seq_want == self._seq_next:
                left = self._buckets if not self.drop_remainder else {}
                self._buckets, self._pending = {}, 0
                keys = sorted(left)
                for n, key in enumerate(keys):       # the mark of a remainder batch: the remainder batches after it
                    self._ready.append((left[key], key, (self._seq_want, self._waiting(left, keys[n + 1:]), True)))
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
        items, (OH, OW), mark = ready
        t0 = time.perf_counter()
        staged = self._preparer.prepare([it[:2] for it in items], OH, OW)
        self.timings["stage"] += time.perf_counter() - t0
        self._staged.append((staged, mark))

    # ---------------------------------------------------------------- iterator
    def __iter__(self):
        return self

    def __next__(self):
        self._started = True
        if self._closed:
            raise StopIteration
        try:
            if not self._staged:
                ready = self._next_ready(block=True)
                if ready is None:
                    self.close()
                    raise StopIteration
                self._stage(ready)
            staged, self._mark = self._staged.popleft()
            self._handed += 1
            while self._log_base < self._mark[0]:    # state() starts from the mark: forget the items before it
                self._cursor_base = self._passed(self._log.popleft(), self._cursor_base, self._rng_base)
                self._log_base += 1
            batch = self._preparer.hand_out(staged)
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

    # ---------------------------------------------------------------- stopping and continuing
    DEFINITION = ("paths", "file_sizes", "num_classes", "batch_size", "options", "geometric", "loop", "rank", "world",
                  "shuffle_buffer", "max_pending", "drop_remainder")

    def definition(self):
        """What two pipelines must share for one to continue the other's stream, as JSON data. The resize rule is a
        function and cannot be listed: it is checked through the bucket keys a state records."""
        if self._definition is None:
            self._definition = {
                "paths": list(self.paths), "file_sizes": [os.path.getsize(p) for p in self.paths],
                "num_classes": self.num_classes, "batch_size": self.batch_size,
                "options": [[s.kind, _plain(s.args)] for s in self.steps], "geometric": self.geometric,
                "loop": bool(self.loop), "rank": int(self.rank), "world": int(self.world),
                "shuffle_buffer": self.shuffle_buffer, "max_pending": self.max_pending,
                "drop_remainder": bool(self.drop_remainder)}
        return self._definition

    def state(self):
        """The stream as of the last batch handed out (the start of the stream if none was), as a JSON-serialisable
        dict: where the record cursor, the RandomState and the shuffle buffer stood when that batch was assembled, and
        which records waited in which bucket with which draws. Nothing decoded, staged or in flight is part of it: the
        record stream runs ahead of bucketing, so the cursor is the one logged with the last item bucketed, the
        RandomState is a second one that repeats each item's calls as batches are handed out, and the shuffle buffer
        is wound back over the items drawn since. `replay` (items drawn but not bucketed) is therefore always empty."""
        m, waiting, exhausted = self._mark
        log = list(self._log)
        cursor, rng = self._cursor_base, np.random.RandomState(0)
        rng.set_state(self._rng_base.get_state())
        for entry in log[:max(0, m - self._log_base)]:         # none once a batch was handed out: the log starts at its mark
            cursor = self._passed(entry, cursor, rng)
        epoch, file, record, i, draining = cursor
        index = {}
        for n, p in enumerate(self.paths):
            index.setdefault(p, n)
        ref = lambda rec: [index[rec[0]], int(rec[1]), int(rec[2]), int(rec[3])]
        buf = self._records.rewound([(e[0], e[2]) for e in log[max(0, m - self._log_base):]])
        return {
            "version": STATE_VERSION, "definition": dict(self.definition()), "batches": self._handed, "items": m,
            "cursor": {"pass": epoch, "file": file, "record": record, "i": i},
            "rng": _rng_to_json(rng.get_state()), "shuffle": [ref(r) for r in buf], "draining": bool(draining),
            "buckets": [{"key": [int(v) for v in key],
                         "items": [{"record": ref(e[0]), "draws": list(e[1]), "frame": [int(v) for v in frame]}
                                   for e, frame in items]} for key, items in waiting],
            "replay": [], "pending": sum(len(items) for _, items in waiting), "exhausted": bool(exhausted)}

    def restore(self, state):
        """Continue the stream a `state()` dict describes. Only before the first batch is asked for. Raises
        InputStateMismatch (naming the field) when the state was taken by a differently defined pipeline, and leaves
        this one untouched then."""
        if self._started or self._closed:
            raise RuntimeError("InputPipeline.restore() must be called before the first batch is asked for")
        if state.get("version") != STATE_VERSION:
            raise InputStateMismatch("version", state.get("version"), STATE_VERSION)
        mine, theirs = self.definition(), state["definition"]
        for field in self.DEFINITION:
            if theirs.get(field) != mine[field]:
                raise InputStateMismatch(field, theirs.get(field), mine[field])
        if state["replay"]:
            raise ValueError("the input state lists replay items, which this version never writes")
        for b in state["buckets"]:
            for it in b["items"]:
                if list(self._key(it["frame"])) != list(b["key"]):
                    raise InputStateMismatch("resized_shape", b["key"], list(self._key(it["frame"])))
        ref = lambda r: (self.paths[r[0]], int(r[1]), int(r[2]), int(r[3]))
        c = state["cursor"]
        cursor = (int(c["pass"]), int(c["file"]), int(c["record"]), int(c["i"]), bool(state["draining"]))
        self._records.restore(cursor, _rng_from_json(state["rng"]), [ref(r) for r in state["shuffle"]])
        self._rng_base.set_state(self.rng.get_state())
        m = int(state["items"])
        first = m - sum(len(b["items"]) for b in state["buckets"])
        self._log.clear()
        self._log_base = self._seq_want = self._seq_next = first
        self._cursor_base = cursor
        self._buckets, self._pending, where, waiting = {}, 0, {}, []
        self._resend.clear()
        for b in state["buckets"]:
            key = tuple(int(v) for v in b["key"])
            self._buckets[key] = []
            entries = [(ref(it["record"]), [float(u) for u in it["draws"]], None, None) for it in b["items"]]
            for e in entries:
                where[first + len(self._resend)] = key
                self._resend.append(e)
            waiting.append((key, tuple((e, tuple(it["frame"])) for e, it in zip(entries, b["items"]))))
        self._refill = (m, where)
        self._exhausted = bool(state["exhausted"])
        self._mark = (m, tuple(waiting), self._exhausted)
        self._handed = int(state["batches"])

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
