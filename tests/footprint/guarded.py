"""Guard bands around device buffers: the instrument of tests/footprint.

Every workspace, output and input of a guarded call lives in an allocation of its own, exactly as large as the size
query (or the tensor shape) says, with GUARD_BYTES on each side. A kernel that stores past its buffer then writes into
memory this test owns — an ordinary assertion failure of `check()`, not a fault and not a silent hit on somebody
else's tensor, which is what the grow-only ops.workspace cache and torch's caching allocator turn such a store into.

GUARD_BYTES is 512 KiB: the largest block one workgroup stores is a 256 x 256 fp32 tile of the split engine (256 KiB);
the band is twice that, and a multiple of 256 bytes, so a payload keeps the 256-byte alignment the library assumes of
the buffers it is handed (the parent comes from torch's allocator, which aligns to 512).

Guards of workspaces and outputs hold PATTERN, a finite 32-bit value; guards of inputs hold quiet NaNs, so a read past
an input that enters arithmetic makes the result non-finite. Both kinds are compared afterwards as integers, bit for
bit (an input must not be written at all). Payloads: workspaces 0xFF bytes (as ops.workspace under MTLSSL_POISON_WS),
outputs without ACCUM NaN, inputs their data.

A plain module: no fixtures, not a conftest."""
import torch

GUARD_BYTES = 512 << 10
PATTERN = 0x5AC3A53C            # finite as a float (3.1e16), positive as an int32; no byte repeats
NAN_BITS = 0x7FC00000           # quiet NaN
assert GUARD_BYTES % 256 == 0 and GUARD_BYTES == 2 * 256 * 256 * 4

_expected = {}


def _guard_bytes(bits, phase, device):
    """GUARD_BYTES bytes of the little-endian 32-bit value `bits`, for a band that starts `phase` bytes past a 4-byte
    boundary of the parent: every aligned word of the parent's guard regions holds `bits`."""
    key = (bits, phase, str(device))
    t = _expected.get(key)
    if t is None:
        four = torch.tensor([(bits >> (8 * ((i + phase) % 4))) & 255 for i in range(4)], dtype=torch.uint8)
        t = four.repeat(GUARD_BYTES // 4).to(device)
        _expected[key] = t
    return t


class Guard:
    """One allocation: [guard | payload of exactly nbytes | guard]."""

    def __init__(self, nbytes, device, bits, key=None):
        self.nbytes, self.bits, self.key = int(nbytes), bits, key
        self.parent = torch.empty(2 * GUARD_BYTES + self.nbytes, dtype=torch.uint8, device=device)
        assert self.parent.data_ptr() % 256 == 0 or not self.parent.is_cuda      # (host memory: the CPU self-tests)
        self.phase = (GUARD_BYTES + self.nbytes) % 4
        self.lo().copy_(_guard_bytes(bits, 0, self.parent.device))
        self.hi().copy_(_guard_bytes(bits, self.phase, self.parent.device))
        self.payload = self.parent[GUARD_BYTES:GUARD_BYTES + self.nbytes]

    def lo(self):
        return self.parent[:GUARD_BYTES]

    def hi(self):
        return self.parent[GUARD_BYTES + self.nbytes:]

    def damage_counts(self):
        """Two 0-d tensors on the buffer's device: damaged bytes before / after the payload (no synchronisation)."""
        dev = self.parent.device
        return ((self.lo() != _guard_bytes(self.bits, 0, dev)).sum(), (self.hi() != _guard_bytes(self.bits, self.phase, dev)).sum())

    def first_damage(self):
        """None, or (side, offset): the damaged guard byte at the lowest address, `offset` counted from the payload's
        first byte (-1 is the byte just before the payload, nbytes the byte just after it)."""
        dev = self.parent.device
        bad = (self.lo() != _guard_bytes(self.bits, 0, dev)).nonzero()
        if bad.numel():
            return "before", int(bad[0]) - GUARD_BYTES
        bad = (self.hi() != _guard_bytes(self.bits, self.phase, dev)).nonzero()
        if bad.numel():
            return "after", self.nbytes + int(bad[0])
        return None

    def describe(self):
        what = "%s, %d bytes" % (self.key if self.key is not None else "buffer", self.nbytes)
        d = self.first_damage()
        return None if d is None else "%s: guard %s the payload damaged, first at byte offset %d" % (what, d[0], d[1])


def guarded(shape_or_nbytes, dtype=torch.uint8, fill=None, device="cuda", guards=None, key=None):
    """A contiguous tensor of exactly the requested size between two guard bands; `.guard` is its Guard.
    shape_or_nbytes: an int (that many elements of dtype; bytes for uint8) or a shape.
    fill: None -> 0xFF bytes (a poisoned workspace; NaN as floats, -1 as ints); a number -> that value; a tensor -> its
    data (an input: NaN guards unless `guards` says otherwise, dtype and shape taken from the tensor).
    guards: "pattern" | "nan"."""
    if isinstance(fill, torch.Tensor):
        shape, dtype = tuple(fill.shape), fill.dtype
        guards = guards or "nan"
    else:
        shape = (int(shape_or_nbytes),) if isinstance(shape_or_nbytes, int) else tuple(int(s) for s in shape_or_nbytes)
        guards = guards or "pattern"
    n = 1
    for s in shape:
        n *= s
    item = torch.empty(0, dtype=dtype).element_size()
    g = Guard(n * item, torch.device(device), PATTERN if guards == "pattern" else NAN_BITS, key)
    assert g.payload.data_ptr() % 256 == 0 or not g.parent.is_cuda
    view = g.payload.view(dtype).view(shape) if n else torch.empty(shape, dtype=dtype, device=g.parent.device)
    if isinstance(fill, torch.Tensor):
        view.copy_(fill)
    elif fill is None:
        g.payload.fill_(255)
    else:
        view.fill_(fill)
    view.guard = g
    return view


def check_guards(guards, what="guard bands"):
    """Synchronise, then assert every Guard of `guards` intact; the message names key, size, side and first offset."""
    guards = [g for g in guards if g is not None]
    if any(g.parent.is_cuda for g in guards):
        torch.cuda.synchronize()
    if not guards:
        return
    by_device = {}
    for g in guards:
        by_device.setdefault(g.parent.device, []).append(g)
    bad = []
    for gs in by_device.values():                    # one device-to-host copy per device, not one per guard
        counts = torch.stack([sum(g.damage_counts()) for g in gs]).cpu()
        bad += [gs[i].describe() for i in counts.nonzero().flatten().tolist()]
    assert not bad, "%s: %d of %d buffers written outside their bytes — %s" % (what, len(bad), len(guards), "; ".join(bad[:8]))


class GuardSet:
    """The guarded operands of one test case: inputs (data + NaN guards), outputs (NaN or given prefill + pattern
    guards); check() asserts all of them intact."""

    def __init__(self, device="cuda"):
        self.device, self.guards = device, []

    def _keep(self, t, key):
        t.guard.key = key
        self.guards.append(t.guard)
        return t

    def input(self, t, key="input"):
        return self._keep(guarded(None, fill=t, device=self.device), key)

    def output(self, shape, key="output", dtype=torch.float32, fill=float("nan")):
        """An output the call must overwrite (NaN prefill), or one it accumulates into (fill = a tensor of old values)."""
        if isinstance(fill, torch.Tensor):
            return self._keep(guarded(None, fill=fill, device=self.device, guards="pattern"), key)
        return self._keep(guarded(shape, dtype, fill, self.device), key)

    def check(self):
        check_guards(self.guards, "operands")


class GuardedWorkspaces:
    """Context manager: for its duration mtl_ssl_amd.ops.workspace — the one name every wrapper allocates its scratch
    through — hands out a fresh guarded buffer of exactly the bytes asked for (0xFF-filled, as under MTLSSL_POISON_WS),
    on the stream current at the call, and keeps every hand-out alive as (key, nbytes, buffer) until check()."""

    def __init__(self):
        self.handouts = []
        self.stats = {}           # key -> [hand-outs, total bytes]
        self._saved = None

    def __enter__(self):
        from mtl_ssl_amd import ops
        assert self._saved is None
        self._saved = ops.workspace
        ops.workspace = self._hand_out
        return self

    def __exit__(self, *exc):
        from mtl_ssl_amd import ops
        ops.workspace = self._saved
        self._saved = None
        return False

    def _hand_out(self, nbytes, key="default", device=None):
        device = device or torch.device("cuda", torch.cuda.current_device())
        buf = guarded(int(nbytes), torch.uint8, None, device, key="workspace %r" % (key,))
        assert buf.numel() == int(nbytes)
        self.handouts.append((key, int(nbytes), buf))
        s = self.stats.setdefault(key, [0, 0])
        s[0] += 1
        s[1] += int(nbytes)
        return buf

    def bytes_of(self, key):
        return [n for k, n, _ in self.handouts if k == key]

    def check(self):
        check_guards([b.guard for _, _, b in self.handouts], "workspaces")

    def report(self):
        return ", ".join("%s %d x / %d B" % (k, c, n) for k, (c, n) in sorted(self.stats.items()))


class _TorchShim:
    """Stands in for the `torch` name of mtl_ssl_amd.ops: device allocations come back guarded, the rest is torch."""

    def __init__(self, owner):
        self._owner = owner

    def __getattr__(self, name):
        return getattr(torch, name)

    def _alloc(self, args, kw, fill):
        device = kw.get("device")
        if device is None or torch.device(device).type != "cuda":
            return None
        shape = args[0] if len(args) == 1 and not isinstance(args[0], int) else args
        t = guarded(tuple(shape), kw.get("dtype", torch.float32), fill, device, key="output of the wrapper")
        self._owner.guards.append(t.guard)
        self._owner.tensors.append(t)
        return t

    def empty(self, *args, **kw):
        t = self._alloc(args, kw, None)
        return t if t is not None else torch.empty(*args, **kw)

    def zeros(self, *args, **kw):
        t = self._alloc(args, kw, 0)
        return t if t is not None else torch.zeros(*args, **kw)


class GuardedOutputs:
    """Context manager: the tensors an ops.* wrapper allocates for its results (torch.empty / torch.zeros on the device,
    inside mtl_ssl_amd.ops only) are guarded buffers of exactly their shape, prefilled with 0xFF bytes (NaN as floats,
    -1 as int32) where the wrapper asked for uninitialised memory."""

    def __init__(self):
        self.guards, self.tensors = [], []

    def __enter__(self):
        from mtl_ssl_amd import ops
        self._saved = ops.torch
        ops.torch = _TorchShim(self)
        return self

    def __exit__(self, *exc):
        from mtl_ssl_amd import ops
        ops.torch = self._saved
        return False

    def check(self):
        check_guards(self.guards, "wrapper outputs")
