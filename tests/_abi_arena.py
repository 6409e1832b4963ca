"""Guard-band arena for the C-ABI's memory contract (include/ddrl.h, "Memory contract"): where a call writes, what it leaves alone,
and whether its result depends on what lies next to its inputs.  No GPU code here: one torch.uint8 tensor per call (on the GPU for
the library, on the CPU for the stand-in kernels of tests/test_abi_table_cpu.py), filled with sentinels, out of which a case carves
its inputs and outputs at chosen byte offsets; the library gets raw addresses (arena.data_ptr() + offset).

    P1  nothing outside   every guard word around every input and output still holds its sentinel
    P2  everything inside no sentinel word is left inside an output's documented extent, the extent is bit-equal to what the plain twin
                          (exact-size torch tensors, handles built from the same seeds) wrote, and an output the header says is left
                          alone still holds the sentinel
    P3  inputs intact     every input is bit-identical before and after (the one the header documents as modified equals the twin's)
    P4  surroundings      three arena runs — input guards filled with NaN, 1e30, zeros — give bit-identical outputs
    ALIGN                 a run with pointers offset by one float (where the contract allows it) is bit-equal to the aligned run

A case is a function fn(ctx) that builds its handles, declares its buffers through ctx.inp / ctx.out and returns the closure that makes
the call under test; run_case drives it once on a PlainCtx and several times on ArenaCtx and collects every failed comparison before
raising anything.  The closure hands the call ctx.stream_arg as its stream — NULL in all of these runs; run_stream_case (second half
of this file, "S") runs the same case once more on a side stream, for the header's stream contract."""
import contextlib
import ctypes

import numpy as np
import torch

SENT_WORD = 0x7FC0DEAD           # float / double regions: a quiet NaN with a payload
SENT_BYTE = 0xA5                 # uint8 / int32 / int64 outputs: neither 0 nor 1 as `ended`, negative or out of range as an index
SENT_BYTE_WORD = 0xA5A5A5A5
FILLS = {"nan": SENT_WORD, "big": int(np.float32(1e30).view(np.uint32)), "zeros": 0}
MIN_GUARD = 4096
_FLOATS = (torch.float32, torch.float64)


def _i32(word):
    return int(np.uint32(word).view(np.int32))


def _as_tensor(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
    return t.contiguous() if dtype is None else t.to(dtype).contiguous()


class Region:
    def __init__(self, name, off, nbytes, lo, hi, dtype, word):
        self.name, self.off, self.nbytes, self.lo, self.hi, self.dtype, self.word = name, off, nbytes, lo, hi, dtype, word


class Arena:
    """One sentinel-filled byte tensor.  carve() places a buffer with a guard of max(4096 bytes, its own size) on BOTH sides (a one-row
    overrun and a wrong-stride write of the whole extent both land in it); guards are never shared between buffers."""

    def __init__(self, device, capacity=48 << 20):
        raw = torch.empty(capacity + 256, dtype=torch.uint8, device=device)   # carve() fills what it hands out, guards included
        skip = -raw.data_ptr() % 256                                           # (the CPU allocator aligns to 64 bytes only)
        self.buf = raw[skip:skip + capacity]
        self.base = self.buf.data_ptr()
        assert self.base % 256 == 0
        self.cursor = 0
        self.regions = []
        self.pristine = None

    def carve(self, nbytes, align=256, misalign_floats=0, name="", dtype=torch.float32, word=SENT_WORD):
        """A buffer of nbytes whose address is `align`-aligned plus misalign_floats * 4 bytes; buffer and guards are filled with the
        32-bit pattern `word`."""
        guard = max(MIN_GUARD, nbytes)
        lo = self.cursor
        off = -(-(lo + guard) // align) * align + 4 * misalign_floats
        hi = -(-(off + nbytes + guard) // 4) * 4
        assert hi <= self.buf.numel(), "arena too small for this case"
        assert off - lo >= guard and hi - (off + nbytes) >= guard                      # the condition the guards are held to
        self.buf[lo:hi].view(torch.int32).fill_(_i32(word))
        self.cursor = -(-hi // 256) * 256
        r = Region(name, off, nbytes, lo, hi, dtype, word)
        self.regions.append(r)
        return r

    def ptr(self, r):
        return self.base + r.off

    def region(self, r, view_dtype=torch.uint8):
        return self.buf[r.off:r.off + r.nbytes].view(view_dtype)

    def write(self, r, t):
        src = _as_tensor(t).reshape(-1).view(torch.uint8)
        assert src.numel() == r.nbytes, (r.name, src.numel(), r.nbytes)
        self.buf[r.off:r.off + r.nbytes].copy_(src)

    def arm(self):
        """Call after every buffer is carved and every input written, right before the call under test."""
        self.pristine = self.buf[:self.cursor].clone()

    def guards_intact(self):
        """Names of the buffers with a changed guard byte ([] = intact).  The guards were filled with the region's sentinel word; they
        are compared with their image at arm() time through an int32 view."""
        bad = []
        for r in self.regions:
            a, b = -(-(r.off + r.nbytes) // 4) * 4, r.off // 4 * 4
            ok = (torch.equal(self.buf[r.lo:b].view(torch.int32), self.pristine[r.lo:b].view(torch.int32))
                  and torch.equal(self.buf[b:r.off], self.pristine[b:r.off])
                  and torch.equal(self.buf[r.off + r.nbytes:a], self.pristine[r.off + r.nbytes:a])
                  and torch.equal(self.buf[a:r.hi].view(torch.int32), self.pristine[a:r.hi].view(torch.int32)))
            if not ok:
                bad.append(r.name)
        return bad

    def unchanged(self, r):
        return torch.equal(self.region(r), self.pristine[r.off:r.off + r.nbytes])

    def all_overwritten(self, r):
        """No sentinel left inside the extent: no 32-bit word of a float / double buffer is the NaN word, no element of an integer
        buffer is made of 0xA5 bytes."""
        if r.nbytes == 0:
            return True
        if r.dtype in _FLOATS:
            return not bool((self.region(r, torch.int32) == _i32(SENT_WORD)).any())
        v = self.region(r, torch.uint8).reshape(-1, r.dtype.itemsize)
        return not bool((v == SENT_BYTE).all(dim=1).any())


class Checks:
    """Every comparison of a case is collected before anything is raised (tests/test_gpu_acting.py's _Checks)."""

    def __init__(self, case):
        self.case, self.failed = case, []

    def add(self, prop, ok, what):
        if not ok:
            self.failed.append((prop, what))

    def props(self):
        return sorted(set(p for p, _ in self.failed))

    def report(self):
        assert not self.failed, "%s: %d memory-contract check(s) failed:\n  %s" % (
            self.case, len(self.failed), "\n  ".join("%s %s" % f for f in self.failed))


class _Ctx:
    def __init__(self, device, lib=None, stream=None):
        self.device, self.lib = torch.device(device), lib
        self.bufs, self._keep, self._defer = {}, [], []
        self.expect_rc = 0
        self.stream = stream       # None: the null stream (PlainCtx, ArenaCtx on the GPU); StreamCtx: the side stream of its run

    @property
    def stream_arg(self):
        """What a closure hands the call under test as `void *stream`: NULL, the side stream's hipStream_t, or — for the CPU
        stand-ins of tests/test_abi_table_cpu.py — the model stream itself."""
        if self.stream is None:
            return None
        return ctypes.c_void_p(self.stream.cuda_stream) if hasattr(self.stream, "cuda_stream") else self.stream

    def host(self, name, n, ctype):
        """A HOST output of n elements (the *_h scalars of counts / mt_state / opt_steps / opt_state_get / env_stats): a ctypes array
        filled with 0xA5 bytes; read when the call returns — such a call is documented to synchronise its stream — and compared
        with the plain twin's."""
        arr = (ctype * int(n))()
        ctypes.memset(arr, SENT_BYTE, ctypes.sizeof(arr))
        self.bufs[name] = dict(kind="host", arr=arr)
        return arr

    def read_host(self):
        """Called as soon as the call under test has returned, before anything else synchronises."""
        for b in self.bufs.values():
            if b["kind"] == "host":
                b["got"] = bytes(b["arr"])

    # -- what a case uses -------------------------------------------------------------------------------------------------------
    def tmp(self, x, dtype=None):
        """A plain device tensor for the case's SETUP calls (never part of the arena); returns the tensor (kept alive)."""
        t = _as_tensor(x, dtype).to(self.device)
        self._keep.append(t)
        return t

    def keep(self, *objs):
        self._keep.extend(objs)
        return objs[0]

    def defer(self, fn):
        """Run fn() after the case's results are read (handle destruction)."""
        self._defer.append(fn)

    def sync(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def finish(self):
        self.sync()
        for fn in reversed(self._defer):
            fn()
        self._defer = []


class PlainCtx(_Ctx):
    """The twin: exact-size tensors of the caching allocator, what every other test of the suite passes."""
    arena = None

    def inp(self, name, x, dtype=None, ma=False, modified=False, align=256):
        t = _as_tensor(x, dtype)
        d = torch.zeros(t.numel() * t.element_size() + 64, dtype=torch.uint8, device=self.device)   # zero slack: the stand-ins' "neighbour"
        d[:t.numel() * t.element_size()].copy_(t.reshape(-1).view(torch.uint8))
        self.bufs[name] = dict(kind="in", t=d, nbytes=t.numel() * t.element_size(), dtype=t.dtype, modified=modified)
        return d.data_ptr()

    def out(self, name, nelem, dtype=torch.float32, ma=False, untouched=False, align=256):
        nbytes = int(nelem) * dtype.itemsize
        d = torch.empty(nbytes + 64, dtype=torch.uint8, device=self.device)
        self.bufs[name] = dict(kind="out", t=d, nbytes=nbytes, dtype=dtype, untouched=untouched)
        return d.data_ptr()

    def view(self, name, extra=0):
        b = self.bufs[name]
        return b["t"][:b["nbytes"] + extra * b["dtype"].itemsize].view(b["dtype"]).numpy()

    def tensor(self, name):
        """The buffer's extent as a tensor of its dtype (for a case that copies a handle's internal array out itself)."""
        b = self.bufs[name]
        return b["t"][:b["nbytes"]].view(b["dtype"])

    def arm(self):
        self.sync()

    def result(self, name):
        b = self.bufs[name]
        return b["t"][:b["nbytes"]].clone()


class ArenaCtx(_Ctx):
    """The same case inside the arena.  in_fill: what surrounds the inputs ("nan" / "big" / "zeros"); the outputs' side is always the
    sentinel.  misalign: names of the pointers to offset by one float (only those the case declares ma=True take the offset)."""
    capacity = 48 << 20

    def __init__(self, device, lib=None, in_fill="nan", misalign=(), capacity=None, stream=None):
        super().__init__(device, lib, stream)
        self.arena, self.in_fill, self.misalign = Arena(device, capacity or self.capacity), in_fill, set(misalign)
        self.ma_names = []

    def _mis(self, name, ma):
        if ma:
            self.ma_names.append(name)
        return 1 if (ma and name in self.misalign) else 0

    def inp(self, name, x, dtype=None, ma=False, modified=False, align=256):
        t = _as_tensor(x, dtype)
        r = self.arena.carve(t.numel() * t.element_size(), align, self._mis(name, ma), name, t.dtype, FILLS[self.in_fill])
        self.arena.write(r, t.to(self.device))
        self.bufs[name] = dict(kind="in", r=r, dtype=t.dtype, modified=modified)
        return self.arena.ptr(r)

    def out(self, name, nelem, dtype=torch.float32, ma=False, untouched=False, align=256):
        word = SENT_WORD if dtype in _FLOATS else SENT_BYTE_WORD
        r = self.arena.carve(int(nelem) * dtype.itemsize, align, self._mis(name, ma), name, dtype, word)
        self.bufs[name] = dict(kind="out", r=r, dtype=dtype, untouched=untouched)
        return self.arena.ptr(r)

    def view(self, name, extra=0):
        b = self.bufs[name]
        r = b["r"]
        return self.arena.buf[r.off:r.off + r.nbytes + extra * b["dtype"].itemsize].view(b["dtype"]).numpy()

    def tensor(self, name):
        b = self.bufs[name]
        return self.arena.region(b["r"], b["dtype"])

    def arm(self):
        self.sync()
        self.arena.arm()

    def result(self, name):
        return self.arena.region(self.bufs[name]["r"]).clone()


def _run(fn, ctx, checks, tag):
    call = fn(ctx)
    ctx.arm()
    rc = call()
    ctx.read_host()
    ctx.sync()
    rcs = list(rc) if isinstance(rc, (list, tuple)) else [rc]
    for v in rcs:
        checks.add("RC", v is None or v == ctx.expect_rc, "%s: call returned %r, expected %r" % (tag, v, ctx.expect_rc))
    return ctx


def _check_arena(ctx, plain, checks, tag):
    ar = ctx.arena
    for name in ar.guards_intact():
        checks.add("P1", False, "%s: a guard word around `%s` was overwritten" % (tag, name))
    res = {}
    for name, b in ctx.bufs.items():
        if b["kind"] == "host":
            checks.add("S-sync", b["got"] == plain.bufs[name]["got"], "%s: host output `%s` differs from the plain twin's" % (tag, name))
            continue
        r = b["r"]
        if b["kind"] == "out":
            if b["untouched"]:
                checks.add("P2", ar.unchanged(r), "%s: output `%s` must be left untouched and was written" % (tag, name))
                continue
            checks.add("P2", ar.all_overwritten(r), "%s: a sentinel is left inside the extent of output `%s`" % (tag, name))
            res[name] = ctx.result(name)
            checks.add("P2", torch.equal(res[name].cpu(), plain.result(name).cpu()), "%s: output `%s` differs from the plain twin's" % (tag, name))
        elif b["modified"]:
            res[name] = ctx.result(name)
            checks.add("P3", torch.equal(res[name].cpu(), plain.result(name).cpu()),
                       "%s: input `%s` (documented as modified) differs from the plain twin's" % (tag, name))
        else:
            checks.add("P3", ar.unchanged(r), "%s: input `%s` was written" % (tag, name))
    return res


def run_case(name, fn, device, lib=None, misaligned=True, capacity=None):
    """P1-P4 of one case, plus its misaligned variants (each pointer the case declares ma=True offset by one float on its own, then all
    of them together).  Returns the Checks; the caller reports."""
    checks = Checks(name)
    plain = _run(fn, PlainCtx(device, lib), checks, "plain")
    runs = {}
    ma_names = []
    for fill in ("nan", "big", "zeros"):
        ctx = _run(fn, ArenaCtx(device, lib, fill, capacity=capacity), checks, fill)
        runs[fill] = _check_arena(ctx, plain, checks, fill)
        ma_names = ctx.ma_names
        ctx.finish()
    for fill in ("big", "zeros"):
        for k, v in runs[fill].items():
            checks.add("P4", torch.equal(v, runs["nan"][k]),
                       "`%s` differs between input guards of NaN and of %s: the call reads beyond its inputs" % (k, fill))
    if misaligned and ma_names:
        variants = [(n,) for n in ma_names] + ([tuple(ma_names)] if len(ma_names) > 1 else [])
        for mis in variants:
            tag = "misaligned(%s)" % ",".join(mis)
            ctx = _run(fn, ArenaCtx(device, lib, "nan", mis, capacity), checks, tag)
            got = _check_arena(ctx, plain, checks, tag)
            for k, v in got.items():
                checks.add("ALIGN", torch.equal(v, runs["nan"][k]), "%s: `%s` differs from the aligned run" % (tag, k))
            ctx.finish()
    plain.finish()
    return checks


# ---- S: the stream contract (include/ddrl.h, "Conventions": all device work is enqueued on `stream`) ------------------------------------
# One more arena run (`nan` fill, aligned) on a non-blocking side stream s.  Every device input is carved holding a DECOY — its own
# elements rotated by one position: an index, mask or flag array stays in range, weights and observations stay valid values that give
# another result — while the true value waits in a device-side staging image.  On s, in this order: a bounded GATE that holds the
# stream, the LATE WRITES (the true value of every input over its decoy, the sentinel over every output extent), the closure called with
# s.  Then s.synchronize() — not a device sync — and the arena is read.  P1 / P2 / P3 hold as they stand against the plain twin, and
#     S-early  work that did not go to s ran during the gate: it read decoys and the late sentinel erased what it wrote — a sentinel is
#              left or the output differs from the twin's, and still does once the whole device has drained
#     S-late   work left unjoined on another stream had not landed at s.synchronize(): the same failures, gone after a device sync
#     S-sync   a host output read behind a sync of the wrong stream is stale (ctx.host, read when the call returns)
#     VOID     the gate, measured with events in every run, came out shorter than intended, or it held the null stream as well (streams
#              that share a hardware queue run one behind the other: side_stream picks one that is seen to run beside the null stream,
#              and every run checks with a marker on the null stream): the run proves nothing and fails
# The side a run uses is an object with stream / on() / gate() / enqueue(fn) / synchronize() / drain() / measured_ms() / gate_ms:
# TorchSide on the GPU, ModelSide for the NumPy stand-ins of tests/test_abi_table_cpu.py (a stream is a deferred queue there).
_CYCLES_PER_MS = {}


def cycles_per_ms(device):
    """torch.cuda._sleep's cycles per millisecond, measured once per process with two events (a few bounded sleeps)."""
    key = str(device)
    if key not in _CYCLES_PER_MS:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n, ms = 100000, 0.0
        for _ in range(16):
            torch.cuda.synchronize(device)
            e0.record()
            torch.cuda._sleep(n)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            if ms >= 2.0:
                break
            n *= 4
        assert ms >= 2.0, "torch.cuda._sleep(%d) took %.3f ms: no usable gate on this device" % (n, ms)
        _CYCLES_PER_MS[key] = n / ms
    return _CYCLES_PER_MS[key]


def runs_beside(gated, other, device):
    """Does work on stream `other` run while a gate holds stream `gated`?  Two non-blocking streams have no ORDER between them, but the
    runtime maps its streams onto a few hardware queues, and two streams that share one run one behind the other: a gate on one of
    them then holds the other as well, and whatever the gate is meant to expose waits politely.  One bounded probe (a 5 ms gate)."""
    device = torch.device(device)
    torch.cuda.synchronize(device)
    end, mark = torch.cuda.Event(), torch.cuda.Event()
    with torch.cuda.stream(gated):
        torch.cuda._sleep(int(cycles_per_ms(device) * 5.0))
        end.record()
    with torch.cuda.stream(other):
        torch.zeros(1, device=device)
        mark.record()
    mark.synchronize()
    beside = not end.query()
    torch.cuda.synchronize(device)
    return beside


_SIDE_STREAM = {}


def side_stream(device):
    """A stream of torch's pool that is seen to run beside the null stream, both ways (found once per process; at most 16 probes)."""
    device = torch.device(device)
    if str(device) not in _SIDE_STREAM:
        null = torch.cuda.default_stream(device)
        for _ in range(16):
            s = torch.cuda.Stream(device)
            if runs_beside(s, null, device) and runs_beside(null, s, device):
                _SIDE_STREAM[str(device)] = s
                break
        else:
            raise AssertionError("no stream of the pool runs beside the null stream on %s: the gate cannot expose anything" % device)
    return _SIDE_STREAM[str(device)]


class TorchSide:
    def __init__(self, device, gate_ms):
        self.device, self.gate_ms = torch.device(device), float(gate_ms)
        self.cycles = int(cycles_per_ms(self.device) * self.gate_ms * 1.1)
        self.stream = side_stream(self.device)                # torch's pool streams are non-blocking: no implicit order against NULL
        self.e0, self.e1, self.mark = (torch.cuda.Event(enable_timing=True) for _ in range(3))

    def on(self):
        return torch.cuda.stream(self.stream)

    def gate(self):
        self.e0.record(self.stream)
        torch.cuda._sleep(self.cycles)
        self.e1.record(self.stream)
        null = torch.cuda.default_stream(self.device)         # a marker on the null stream: it must pass while the gate still holds
        with torch.cuda.stream(null):
            torch.zeros(1, device=self.device)
            self.mark.record()

    def beside_ms(self):
        """How long before the gate's end the null stream's marker passed (what a launch misplaced there would have had)."""
        return self.mark.elapsed_time(self.e1)

    def enqueue(self, fn):
        fn()                                                   # torch work issued under on() lands on the stream

    def synchronize(self):
        self.stream.synchronize()

    def drain(self):
        torch.cuda.synchronize(self.device)

    def measured_ms(self):
        return self.e0.elapsed_time(self.e1)


class ModelDevice:
    """The CPU model of a device: its streams are deferred queues; eager=True is the twin's device, on which everything runs at once."""

    def __init__(self, eager=False):
        self.eager, self.streams = eager, []

    def new_stream(self):
        s = ModelStream(self, not self.eager)
        self.streams.append(s)
        return s

    def null_stream(self):
        return ModelStream(self, False)

    def synchronize(self):
        for s in self.streams:
            s.synchronize()


class ModelStream:
    def __init__(self, device, deferred):
        self.device, self.deferred, self.q = device, deferred, []

    def enqueue(self, fn):
        if self.deferred:
            self.q.append(fn)
        else:
            fn()

    def synchronize(self):
        while self.q:
            self.q.pop(0)()


class ModelSide:
    def __init__(self, gate_ms=10.0, measured_ms=None):
        self.dev = ModelDevice()
        self.stream, self.gate_ms, self._measured = self.dev.new_stream(), gate_ms, gate_ms if measured_ms is None else measured_ms

    def on(self):
        return contextlib.nullcontext()

    def gate(self):
        pass        # whatever bypasses a deferred queue has run before the queue does: the gate is the model itself

    def enqueue(self, fn):
        self.stream.enqueue(fn)

    def synchronize(self):
        self.stream.synchronize()

    def drain(self):
        self.dev.synchronize()

    def measured_ms(self):
        return self._measured

    def beside_ms(self):
        return self._measured


class StreamCtx(ArenaCtx):
    """The S run.  The case's setup (fn(ctx): handles, setup calls, the carving) runs on the null stream as in every other run and
    arm() drains the device; from the gate on everything is issued under side.on()."""

    def __init__(self, device, lib, side, capacity=None):
        super().__init__(device, lib, "nan", (), capacity, stream=side.stream)
        self.side, self._true = side, []

    def inp(self, name, x, dtype=None, ma=False, modified=False, align=256):
        t = _as_tensor(x, dtype)
        r = self.arena.carve(t.numel() * t.element_size(), align, 0, name, t.dtype, FILLS[self.in_fill])
        true = t.to(self.device).reshape(-1)
        self.arena.write(r, torch.roll(true, 1))                 # the decoy
        self._true.append((r, true.clone()))
        self.bufs[name] = dict(kind="in", r=r, dtype=t.dtype, modified=modified)
        return self.arena.ptr(r)

    def arm(self):
        """pristine becomes the staging image: the true value of every input (what P3 compares with), the sentinel in every output."""
        self.sync()
        ar = self.arena
        ar.arm()
        for r, true in self._true:
            ar.pristine[r.off:r.off + r.nbytes].copy_(true.view(torch.uint8))
        self.sync()

    def late_writes(self):
        ar = self.arena
        for b in self.bufs.values():
            if b["kind"] != "host":
                r = b["r"]
                ar.buf[r.off:r.off + r.nbytes].copy_(ar.pristine[r.off:r.off + r.nbytes])

    def image(self):
        return self.arena.buf[:self.arena.cursor].to("cpu", copy=True)


def _check_image(ctx, image, pristine, plain, checks, tag):
    """_check_arena on a host image of the arena (what was there at s.synchronize(); what was there once the device had drained)."""
    ar = ctx.arena
    keep = ar.buf, ar.pristine
    ar.buf, ar.pristine = image, pristine
    try:
        return _check_arena(ctx, plain, checks, tag)
    finally:
        ar.buf, ar.pristine = keep


def run_stream_case(name, fn, device, lib, side, plain_stream=None, capacity=None):
    """The plain twin (null stream) and ONE S run of the case on `side`.  Returns the Checks; the caller reports."""
    checks = Checks(name)
    plain = _run(fn, PlainCtx(device, lib, plain_stream), checks, "plain")
    ctx = StreamCtx(device, lib, side, capacity)
    call = fn(ctx)
    ctx.arm()
    pristine = ctx.arena.pristine.to("cpu", copy=True)
    with side.on():
        side.gate()
        side.enqueue(ctx.late_writes)
        rc = call()
        ctx.read_host()
        side.synchronize()
        first = ctx.image()
    side.drain()
    drained = ctx.image()
    for v in (list(rc) if isinstance(rc, (list, tuple)) else [rc]):
        checks.add("RC", v is None or v == ctx.expect_rc, "S: call returned %r, expected %r" % (v, ctx.expect_rc))
    got, want = side.measured_ms(), side.gate_ms
    checks.add("VOID", got >= want, "S: the gate held the stream for %.2f ms, %.2f ms intended: the run is void" % (got, want))
    got = side.beside_ms()
    checks.add("VOID", got >= 0.5 * want, "S: the null stream passed its marker %.2f ms before the gate's end (%.2f ms intended): the gate "
               "held the null stream too, the run is void" % (got, want))
    c1 = Checks(name)
    _check_image(ctx, first, pristine, plain, c1, "S")
    checks.failed += c1.failed
    if any(p in ("P2", "P3") for p, _ in c1.failed):
        c2 = Checks(name)
        _check_image(ctx, drained, pristine, plain, c2, "drained")
        if any(p in ("P2", "P3") for p, _ in c2.failed):
            checks.add("S-early", False, "S: the failures above remain after a device sync: work that did not go to the caller's "
                       "stream ran during the gate (it read decoys, or the late sentinel erased its output)")
        else:
            checks.add("S-late", False, "S: the failures above are gone after a device sync: work left on another stream had not "
                       "landed when the caller's stream was synchronised")
    ctx.finish()
    plain.finish()
    return checks
