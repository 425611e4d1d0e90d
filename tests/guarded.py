"""A guarded arena for the C ABI: does an entry point stay inside the memory it was given?

Every device buffer of one call is cut from ONE uint8 tensor, each as  guard | buffer | guard :
  * a buffer's base is a multiple of ALIGN = 256 bytes (what torch's allocator gives; smaller alignments are not examined here);
  * the guard before it ends exactly at the base and the guard after it begins exactly at base + nbytes: nbytes is never
    rounded, so the first byte a call writes past a buffer is a guard byte;
  * the arena ends with a guard: everything behind the last buffer, GUARD bytes at least.
GUARD = 64 KiB on each side.  The condition it satisfies: it is at least one whole workgroup tile of the widest output of the
hot-path ABI, the results tile of 256 rows x 22 columns x 8 B = 45 056 B, so a workgroup that stores a full padded tile at a
buffer's last row lands wholly in memory this arena owns and reads back.  A wider tile added later must raise GUARD
(WIDEST_TILE_BYTES states the tile; the assertion below holds the two together).

Fill: guards, `out` and `scratch` buffers are 0xFF bytes -- a NaN in float32 and float64, -1 in every integer type -- so a read
past an input that reaches a result shows as a NaN or a changed byte, and a stray store of anything else shows in the guard.
check() -- after the call and a synchronise -- wants every guard byte still 0xFF and every `in` buffer byte-equal to what was
put in; its message names the buffer, the side, the first and last changed offset relative to the buffer and the count.
This is ordinary device memory inside one allocation: nothing here can fault that could not fault with separate tensors.

Plain is the same interface on ordinary tensors, one allocation per buffer, for the call the guarded one is compared with.
Nothing here carries a tolerance.  The layout arithmetic needs neither torch nor a GPU."""

ALIGN = 256
GUARD = 64 * 1024
WIDEST_TILE_BYTES = 256 * 22 * 8          # pinn_results_assemble: 256 rows of 22 doubles per workgroup
assert GUARD >= WIDEST_TILE_BYTES and GUARD % ALIGN == 0
FILL = 0xFF
ROLES = ("in", "out", "inout", "scratch")


def round_up(v, a=ALIGN):
    return -(-v // a) * a


def next_base(prev_end):
    """Base of the buffer that follows one ending at prev_end (0: the arena's start): room for the guard after the previous
    buffer and for this one's own, then up to the alignment."""
    return round_up(prev_end + (2 * GUARD if prev_end else GUARD))


def layout(sizes):
    """sizes: byte counts in the order taken -> (bases, total bytes of an arena that holds exactly these)."""
    bases, end = [], 0
    for nb in sizes:
        assert nb >= 0
        bases.append(next_base(end))
        end = bases[-1] + nb
    return bases, (end if bases else 0) + GUARD


def capacity_for(sizes):
    return layout(sizes)[1]


class GuardError(AssertionError):
    pass


class Buf:
    """One buffer: .ptr (an integer address, what ctypes' c_void_p takes), .view(dtype), .bytes() (a host copy)."""

    def __init__(self, name, role, nbytes, tensor, base=0):
        self.name, self.role, self.nbytes, self.base, self._t = name, role, nbytes, base, tensor

    @property
    def ptr(self):
        return self._t.data_ptr() if self.nbytes else self._base_ptr

    def view(self, dtype):
        return self._t.view(dtype)

    def bytes(self):
        return self._t.cpu().numpy().tobytes()


def _as_bytes(init, nbytes, name):
    """init (a torch tensor or a numpy array of any type, or bytes) -> a host uint8 tensor of exactly nbytes."""
    import numpy as np
    import torch
    if isinstance(init, torch.Tensor):
        init = init.detach().cpu().contiguous().numpy()
    if isinstance(init, (bytes, bytearray)):
        a = np.frombuffer(bytes(init), dtype=np.uint8)
    else:
        a = np.ascontiguousarray(init).reshape(-1).view(np.uint8)
    assert a.size == nbytes, "%s: init holds %d bytes, the buffer %d" % (name, a.size, nbytes)
    return torch.from_numpy(a.copy())


class Arena:
    def __init__(self, device="cpu", capacity=1 << 20):
        import torch
        self.device = torch.device(device)
        self.capacity = round_up(capacity)
        self._raw = torch.full((self.capacity + ALIGN,), FILL, dtype=torch.uint8, device=self.device)
        skip = -self._raw.data_ptr() % ALIGN          # 0 on the device; the host allocator aligns to 64 bytes only
        self.mem = self._raw[skip:skip + self.capacity]
        assert self.mem.data_ptr() % ALIGN == 0
        self.bufs = []          # in address order
        self._init = {}         # name -> host uint8 copy of what was put in (in, inout)
        self._end = 0

    def take(self, name, nbytes, role, init=None):
        assert role in ROLES, role
        assert all(b.name != name for b in self.bufs), name
        assert (init is not None) == (role in ("in", "inout")), "%s: in / inout buffers need an init, the others take none" % name
        nbytes = int(nbytes)
        base = next_base(self._end)
        assert base + nbytes + GUARD <= self.capacity, "arena of %d bytes is too small for %s (%d bytes at %d)" % (self.capacity, name, nbytes, base)
        b = Buf(name, role, nbytes, self.mem[base:base + nbytes], base)
        b._base_ptr = self.mem.data_ptr() + base
        if init is not None:
            host = _as_bytes(init, nbytes, name)
            self._init[name] = host
            b._t.copy_(host)
        self.bufs.append(b)
        self._end = base + nbytes
        return b

    def __getitem__(self, name):
        return next(b for b in self.bufs if b.name == name)

    # -- the check ----------------------------------------------------------------------------------------------------------
    def _regions(self):
        """(buffer, side, start, stop, origin): every byte outside the buffers, attributed to the nearer buffer; offsets in a
        message are relative to origin -- the buffer's base for `before` (negative), its end for `after` (0 = first byte past)."""
        out, prev = [], None
        for b in self.bufs:
            if prev is None:
                out.append((b, "before", 0, b.base, b.base))
            else:
                pe = prev.base + prev.nbytes
                out.append((prev, "after", pe, pe + GUARD, pe))
                out.append((b, "before", pe + GUARD, b.base, b.base))
            prev = b
        if prev is not None:
            pe = prev.base + prev.nbytes
            out.append((prev, "after", pe, self.capacity, pe))
        return out

    @staticmethod
    def _changed(diff):
        """diff: bool tensor -> None or (first, last, count)."""
        if not bool(diff.any()):
            return None
        idx = diff.nonzero().reshape(-1)
        return int(idx[0]), int(idx[-1]), int(idx.numel())

    def findings(self, untouched=False):
        """Every violation as (buffer name, kind, first, last, count).  kind: `before` / `after` (a guard; offsets relative to the
        base / to the end), `input` (an `in` buffer changed; offsets from the base).  untouched: the call was refused, so `out`
        and `scratch` buffers must still be the fill and `inout` buffers what was put in (kind `written`)."""
        found = []
        for b, side, lo, hi, origin in self._regions():
            c = self._changed(self.mem[lo:hi] != FILL) if hi > lo else None
            if c:
                found.append((b.name, side, lo + c[0] - origin, lo + c[1] - origin, c[2]))
        for b in self.bufs:
            if b.role == "in" or (untouched and b.role == "inout"):
                c = self._changed(b._t.cpu() != self._init[b.name])
                if c:
                    found.append((b.name, "input" if b.role == "in" else "written") + c)
            elif untouched and b.role in ("out", "scratch"):
                c = self._changed(b._t != FILL)
                if c:
                    found.append((b.name, "written") + c)
        return found

    def check(self, what="", untouched=False):
        found = self.findings(untouched)
        print("GUARD %s: %d buffers, %d bytes, %d guard bytes, %s" % (
            what, len(self.bufs), sum(b.nbytes for b in self.bufs), self.capacity - sum(b.nbytes for b in self.bufs),
            "intact" if not found else "%d findings" % len(found)))
        if found:
            raise GuardError("%s: " % what + "; ".join(describe(f) for f in found))


def describe(f):
    name, kind, first, last, count = f
    where = {"before": "guard before %s", "after": "guard after %s", "input": "input %s", "written": "refused call wrote %s"}[kind] % name
    return "%s: %d bytes changed, offsets %d..%d %s" % (
        where, count, first, last, {"before": "from the base", "after": "past the end"}.get(kind, "from the base"))


class Plain:
    """Arena's interface on ordinary tensors: one allocation per buffer, out / scratch filled like the arena's."""

    def __init__(self, device="cpu"):
        import torch
        self.device = torch.device(device)
        self.bufs = []

    def take(self, name, nbytes, role, init=None):
        import torch
        assert role in ROLES, role
        assert (init is not None) == (role in ("in", "inout"))
        nbytes = int(nbytes)
        t = torch.full((nbytes,), FILL, dtype=torch.uint8, device=self.device)
        if init is not None:
            t.copy_(_as_bytes(init, nbytes, name))
        b = Buf(name, role, nbytes, t)
        b._base_ptr = t.data_ptr()
        self.bufs.append(b)
        return b

    def __getitem__(self, name):
        return next(b for b in self.bufs if b.name == name)


def differing_outputs(a, b):
    """Names of the out / inout buffers of two allocators (the same takes) whose bytes differ."""
    assert [(x.name, x.role, x.nbytes) for x in a.bufs] == [(x.name, x.role, x.nbytes) for x in b.bufs]
    return [x.name for x, y in zip(a.bufs, b.bufs) if x.role in ("out", "inout") and x.bytes() != y.bytes()]
