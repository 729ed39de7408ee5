"""TensorBoard event files without TensorFlow: what the reference leaves in train_dir and eval_dir
(object_detection/trainer.py:440-445 variable histograms, loss scalars and TotalLoss; builders/optimizer_builder.py:117
Learning_Rate; trainer.py:570-574 the config texts; eval_util.py:58-80 one scalar per metric, :660-669 one image per
visualisation).

* The histogram semantics of TensorFlow 1.7's HistogramSummary op (tensorflow/core/lib/histogram/histogram.cc):
  default bucket limits, bucket = first limit strictly greater than double(x), EncodeToProto without zero buckets.
  `histogram_numpy` is the float64 restatement that the device kernel (ops.variable_histograms) is tested against bit
  for bit, and what ParamStore.histograms() runs on a store that lives on the CPU.
* The container: TFRecord framing around serialized Event protos (tensorflow/core/util/event.proto,
  framework/summary.proto), written and read with input_reader's CRC-32C and wire-format helpers.
"""
import os
import socket
import struct
import sys
import time

import numpy as np

from .input_reader import _enc_varint, _fields, _ld, masked_crc

FILE_VERSION = "brain.Event:2"
DT_STRING = 7
MOMENTS = ("min", "max", "num", "sum", "sum_squares", "nonfinite")

_limits = None


def default_bucket_limits():
    """histogram.cc InitDefaultBucketsInner: 1e-12 growing by 1.1 up to 1e20, then DBL_MAX; mirrored around 0.0.
    float64 [1551], 0.0 at index 775."""
    global _limits
    if _limits is None:
        pos, v = [], 1e-12
        while v < 1e20:
            pos.append(v)
            v *= 1.1
        pos.append(sys.float_info.max)
        _limits = np.array([-x for x in reversed(pos)] + [0.0] + pos, np.float64)
        _limits.setflags(write=False)
    return _limits


def histogram_numpy(values, limits=None):
    """Histogram::Add over every value, in float64: -> (moments float64 [6] = min, max, num, sum, sum_squares,
    nonfinite; counts uint32 [len(limits)]). NaN and +-inf are only counted in nonfinite; no finite value (or no value)
    leaves min = DBL_MAX, max = -DBL_MAX, num = 0."""
    limits = default_bucket_limits() if limits is None else np.asarray(limits, np.float64)
    x = np.asarray(values).reshape(-1).astype(np.float64)
    finite = np.isfinite(x)
    bad = int(x.size - finite.sum())
    x = x[finite]
    idx = np.minimum(np.searchsorted(limits, x, side="right"), len(limits) - 1)
    counts = np.bincount(idx, minlength=len(limits)).astype(np.uint32)
    big = sys.float_info.max
    moments = np.array([x.min() if x.size else big, x.max() if x.size else -big, float(x.size), x.sum(),
                        (x * x).sum(), float(bad)], np.float64)
    return moments, counts


def encode_histogram(counts, limits=None):
    """Histogram::EncodeToProto(preserve_zero_buckets=false): every run of empty buckets becomes ONE entry that carries
    the run's last limit and count 0. -> (bucket_limit list, bucket list), equally long."""
    limits = np.asarray(default_bucket_limits() if limits is None else limits, np.float64)
    c = np.asarray(counts)
    empty = c <= 0
    run_ends = np.ones(len(c), bool)              # an empty bucket stays when the next one is occupied or there is none
    run_ends[:-1] = ~empty[1:]
    keep = ~empty | run_ends
    return limits[keep].tolist(), c[keep].astype(np.float64).tolist()


# ------------------------------------------------------------------------------ config texts
def _pbtxt(msg, indent, depth, out):
    import re
    pad = " " * (indent * depth)
    for name, val in msg.items():
        for v in (val if isinstance(val, list) else [val]):
            if isinstance(v, dict):
                out.append("%s%s {" % (pad, name))
                _pbtxt(v, indent, depth + 1, out)
                out.append(pad + "}")
            elif isinstance(v, bool):
                out.append("%s%s: %s" % (pad, name, "true" if v else "false"))
            elif isinstance(v, float):
                out.append("%s%s: %s" % (pad, name, format(v, ".2g")))
            elif isinstance(v, str) and not re.fullmatch(r"[A-Z][A-Z0-9_]*", v):
                out.append('%s%s: "%s"' % (pad, name, v))
            else:
                out.append("%s%s: %s" % (pad, name, v))


def config_md_text(msg, indent=2):
    """object_detection/trainer.py:494-498 config_to_md_text: the message in protobuf text format (floats as %.2g) with
    line breaks and spaces made visible to TensorBoard's markdown; "" for a config that is not there."""
    if msg is None:
        return ""
    out = []
    _pbtxt(msg, indent, 0, out)
    return ("\n".join(out) + "\n").replace("\n", "<br>").replace(" ", "&nbsp;")


# ------------------------------------------------------------------------------ protobuf encoding
def _f64(fn, v):
    return _enc_varint((fn << 3) | 1) + struct.pack("<d", float(v))


def _f32(fn, v):
    return _enc_varint((fn << 3) | 5) + struct.pack("<f", float(v))


def _int(fn, v):
    return _enc_varint(fn << 3) + _enc_varint(int(v))


def _value(tag, payload):
    """Summary{value=1: Value{tag=1, ...}}"""
    return _ld(1, _ld(1, tag.encode("utf-8")) + payload)


class SummaryWriter:
    """Appends Event records to <logdir>/events.out.tfevents.<unix time>.<hostname> (tf.summary.FileWriter's name);
    the first record carries the file version."""

    def __init__(self, logdir):
        os.makedirs(logdir, exist_ok=True)
        now = time.time()
        self.path = os.path.join(logdir, "events.out.tfevents.%010d.%s" % (int(now), socket.gethostname()))
        self._f = open(self.path, "ab")
        if self._f.tell() == 0:
            self._record(_f64(1, now) + _ld(3, FILE_VERSION.encode("ascii")))
            self._f.flush()

    def _record(self, payload):
        hdr = struct.pack("<Q", len(payload))
        self._f.write(hdr + struct.pack("<I", masked_crc(hdr)) + payload + struct.pack("<I", masked_crc(payload)))

    def _event(self, step, summary):
        self._record(_f64(1, time.time()) + _int(2, step) + _ld(5, summary))

    def add_scalar(self, tag, value, step):
        self._event(step, _value(tag, _f32(2, value)))

    def add_histogram(self, tag, moments, counts, limits, step):
        """moments / counts: one variable's rows of ops.variable_histograms or histogram_numpy. A variable that holds
        a NaN or an infinity raises FloatingPointError like the HistogramSummary op ("Nan in summary histogram for")."""
        if moments[5] > 0:
            raise FloatingPointError("Nan in summary histogram for: %s" % tag)
        bl, bc = encode_histogram(counts, limits)
        histo = b"".join(_f64(i + 1, moments[i]) for i in range(5))
        histo += _ld(6, np.asarray(bl, "<f8").tobytes()) + _ld(7, np.asarray(bc, "<f8").tobytes())
        self._event(step, _value(tag, _ld(5, histo)))

    def add_text(self, tag, text, step):
        """tf.summary.text: a scalar DT_STRING tensor with the text plugin's metadata."""
        if isinstance(text, str):
            text = text.encode("utf-8")
        tensor = _int(1, DT_STRING) + _ld(2, b"") + _ld(8, text)
        meta = _ld(1, _ld(1, b"text"))
        self._event(step, _value(tag, _ld(8, tensor) + _ld(9, meta)))

    def add_image(self, tag, png_bytes, height, width, step, colorspace=3):
        image = _int(1, height) + _int(2, width) + _int(3, colorspace) + _ld(4, bytes(png_bytes))
        self._event(step, _value(tag, _ld(4, image)))

    def flush(self):
        self._f.flush()

    def close(self):
        if not self._f.closed:
            self._f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


# ------------------------------------------------------------------------------ reading
def _d(v):
    return struct.unpack("<d", bytes(v))[0]


def _decode_value(buf):
    out = {}
    for fn, wt, v in _fields(buf):
        if fn == 1:
            out["tag"] = bytes(v).decode("utf-8")
        elif fn == 2 and wt == 5:
            out["simple_value"] = struct.unpack("<f", bytes(v))[0]
        elif fn == 4:
            img = {}
            for f2, _, x in _fields(v):
                if f2 in (1, 2, 3):
                    img[("height", "width", "colorspace")[f2 - 1]] = int(x)
                elif f2 == 4:
                    img["encoded_image_string"] = bytes(x)
            out["image"] = img
        elif fn == 5:
            h = {"bucket_limit": [], "bucket": []}
            for f2, w2, x in _fields(v):
                if 1 <= f2 <= 5:
                    h[MOMENTS[f2 - 1]] = _d(x)
                elif f2 in (6, 7):
                    vals = np.frombuffer(bytes(x), "<f8").tolist() if w2 == 2 else [_d(x)]
                    h["bucket_limit" if f2 == 6 else "bucket"] += vals
            out["histo"] = h
        elif fn == 8:
            t = {"string_val": []}
            for f2, _, x in _fields(v):
                if f2 == 1:
                    t["dtype"] = int(x)
                elif f2 == 8:
                    t["string_val"].append(bytes(x))
            out["tensor"] = t
        elif fn == 9:
            for f2, _, x in _fields(v):
                if f2 == 1:
                    for f3, _, y in _fields(x):
                        if f3 == 1:
                            out["plugin_name"] = bytes(y).decode("utf-8")
    return out


def decode_event(payload):
    """One serialized Event -> {wall_time, step, file_version?, values: [{tag, simple_value | histo | image | tensor}]}."""
    ev = {"step": 0, "values": []}
    for fn, wt, v in _fields(memoryview(payload)):
        if fn == 1 and wt == 1:
            ev["wall_time"] = _d(v)
        elif fn == 2 and wt == 0:
            ev["step"] = int(v)
        elif fn == 3:
            ev["file_version"] = bytes(v).decode("utf-8")
        elif fn == 5:
            for f2, _, x in _fields(v):
                if f2 == 1:
                    ev["values"].append(_decode_value(x))
    return ev


def read_records(path):
    """The serialized records of an event file, both CRCs of each verified (IOError on a mismatch or a short file)."""
    with open(path, "rb") as f:
        data = f.read()
    pos, out = 0, []
    while pos < len(data):
        if pos + 12 > len(data):
            raise IOError("truncated record header in %s" % path)
        hdr = data[pos:pos + 8]
        (n,) = struct.unpack("<Q", hdr)
        if struct.unpack("<I", data[pos + 8:pos + 12])[0] != masked_crc(hdr):
            raise IOError("corrupted record (length CRC mismatch) in %s" % path)
        if pos + 16 + n > len(data):
            raise IOError("truncated record (length %d) in %s" % (n, path))
        payload = data[pos + 12:pos + 12 + n]
        if struct.unpack("<I", data[pos + 12 + n:pos + 16 + n])[0] != masked_crc(payload):
            raise IOError("corrupted record (data CRC mismatch) in %s" % path)
        out.append(payload)
        pos += 16 + n
    return out


def read_events(path):
    """An event file -> list of decode_event dicts, CRCs verified."""
    return [decode_event(p) for p in read_records(path)]


def event_files(logdir):
    return sorted(os.path.join(logdir, n) for n in os.listdir(logdir) if n.startswith("events.out.tfevents."))
