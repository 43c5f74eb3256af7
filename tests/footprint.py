"""Guard-band audit of an op's memory footprint (works on CPU and device tensors).

Every case is written once, as `run(alloc) -> {name: result tensor}`, and takes ALL its tensors from `alloc`.  audit(run) runs it with
Plain (ordinary fresh tensors), then with an Arena, and compares the two result dicts bit for bit.

Arena: ONE uint8 allocation filled with 0xFF bytes - NaN as bf16 / fp32 / fp64, 255 as uint8, -1 as int32.  Tensors are contiguous views
at 256-byte multiples or, offset16=True, at 256 k + 16: where the engines' flat parameter buffers put a layer's w / b / gamma / beta,
their gradients and optimizer moments (offsets rounded to 4 floats, the neighbour is the next layer's parameters).  On both sides of every
tensor lies a guard band of at least max(64 KiB, one outermost-dimension slice of the tensor) bytes, so a store one vector, one row, one
workgroup slot or one plane out of bounds lands in memory the test owns and check() finds it; a load from there yields NaN, which reaches
a result and makes it differ from the plain run's.

Roles: "input" (bit-identical after the call), "output" (pre-filled with NaN: every element must have been written), "accumulate"
(pre-filled with given values, the same in both runs), "inout" (documented in-place ops); workspace(nbytes) is EXACTLY nbytes long and,
zero=True, zero before the call and all zero after it; slot(view, full) declares that only the columns `view` of the wider tensor `full`
belong to the op: the other columns keep the 0xFF sentinel bit for bit.
"""
import torch

GUARD_MIN = 64 * 1024
ALIGN = 256
ROLES = ("input", "output", "accumulate", "inout")
_INT_FILL_PLAIN = 0x55      # integer outputs cannot hold a NaN: the two runs start from different bytes, an unwritten element differs


def _round_up(n, m):
    return (n + m - 1) // m * m


def _nbytes(shape, dtype):
    n = 1
    for s in shape:
        n *= int(s)
    return n * torch.empty((), dtype=dtype).element_size()


def guard_bytes(shape, dtype):
    """max(64 KiB, bytes of one outermost-dimension slice), rounded up to 256"""
    shape = tuple(int(s) for s in shape)
    one = _nbytes(shape[1:], dtype) if len(shape) > 1 else 0
    return _round_up(max(GUARD_MIN, one), ALIGN)


def _bytes_of(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


class _Base:
    """what Plain and Arena share: the roles' fills and the bookkeeping of the checks"""

    def __init__(self, device):
        self.device = torch.device(device)
        self.recs = []

    def _raw(self, nbytes, guard, offset16, name):
        raise NotImplementedError

    def _new(self, shape, dtype, guard, offset16, name):
        shape = tuple(int(s) for s in shape)
        raw = self._raw(_nbytes(shape, dtype), guard, offset16, name)
        return raw.view(dtype).view(shape)

    def take(self, shape, dtype, role, fill=None, offset16=False, name=None):
        assert role in ROLES, role
        if isinstance(shape, int):
            shape = (shape,)
        name = name or "%s%d" % (role, len(self.recs))
        t = self._new(shape, dtype, guard_bytes(shape, dtype), offset16, name)
        rec = {"name": name, "role": role, "t": t, "cols": None}
        if role == "output":
            assert fill is None, "an output starts as NaN"
            if not t.dtype.is_floating_point and isinstance(self, Plain):
                _bytes_of(t).fill_(_INT_FILL_PLAIN)
            else:
                _bytes_of(t).fill_(0xFF)
        else:
            assert fill is not None and tuple(fill.shape) == tuple(t.shape) and fill.dtype == dtype, (name, role, "needs its values")
            t.copy_(fill)
            if role == "input":
                rec["keep"] = t.clone()
        self.recs.append(rec)
        return t

    # the four roles by name
    def input(self, fill, offset16=False, name=None):
        return self.take(fill.shape, fill.dtype, "input", fill, offset16, name)

    def output(self, shape, dtype, offset16=False, name=None):
        return self.take(shape, dtype, "output", None, offset16, name)

    def accumulate(self, fill, offset16=False, name=None):
        return self.take(fill.shape, fill.dtype, "accumulate", fill, offset16, name)

    def inout(self, fill, offset16=False, name=None):
        return self.take(fill.shape, fill.dtype, "inout", fill, offset16, name)

    def workspace(self, nbytes, zero=False, dtype=torch.uint8, name=None, keep_front=0):
        """exactly nbytes; zero=True: zeroed now and all zero at check(), else left as 0xFF bytes (a workspace the op need not find cleared).
        keep_front: that many bytes in front hold the op's result at exit (the totals of a statistics tail) and are not asked to be zero."""
        nbytes = int(nbytes)
        name = name or "workspace%d" % len(self.recs)
        es = torch.empty((), dtype=dtype).element_size()
        assert nbytes > 0 and nbytes % es == 0, (name, nbytes, dtype)
        t = self._raw(nbytes, _round_up(GUARD_MIN, ALIGN), False, name).view(dtype)
        _bytes_of(t).fill_(0 if zero else 0xFF)
        assert 0 <= keep_front <= nbytes
        self.recs.append({"name": name, "role": "workspace", "t": t, "zero": bool(zero), "cols": None, "keep_front": int(keep_front)})
        return t

    def slot(self, view, full):
        """view = full[..., lo:hi] of a tensor taken here: only these columns are the op's, the others are set to the sentinel (0xFF bytes)
        now and must hold it at check().  Returns full (the op gets the wide tensor, its row length and the column offset)."""
        rec = next(r for r in self.recs if r["t"] is full)
        ld = full.shape[-1]
        lo = view.storage_offset() - full.storage_offset()
        hi = lo + view.shape[-1]
        assert 0 <= lo < hi <= ld and tuple(view.shape[:-1]) == tuple(full.shape[:-1]) and view.stride() == full.stride(), "a column slice of `full`"
        rec["cols"] = (lo, hi)
        sent = torch.ones(ld, dtype=torch.bool, device=full.device)
        sent[lo:hi] = False
        rec["sent"] = sent
        flat = full.view(-1, ld)
        es = full.element_size()
        bytes2d = flat.view(torch.uint8).view(flat.shape[0], ld, es)
        bytes2d[:, sent] = 0xFF
        if "keep" in rec:
            rec["keep"] = full.clone()
        return full

    def _own(self, rec):
        """the part of a tensor that belongs to the op"""
        t = rec["t"]
        return t if rec["cols"] is None else t[..., rec["cols"][0]:rec["cols"][1]]

    def check_contents(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        for rec in self.recs:
            t, name = rec["t"], rec["name"]
            if rec["cols"] is not None:
                ld, es = t.shape[-1], t.element_size()
                b = t.view(-1, ld).view(torch.uint8).view(-1, ld, es)[:, rec["sent"]]
                bad = b != 0xFF
                if bool(bad.any()):
                    row, col = torch.nonzero(bad.any(dim=2))[0].tolist()
                    cols = torch.nonzero(rec["sent"]).reshape(-1).tolist()
                    raise AssertionError("%s: sentinel column %d (row %d) outside the slot [%d, %d) was written (%d sentinel bytes changed)" % (
                        name, cols[col], row, rec["cols"][0], rec["cols"][1], int(bad.sum())))
            if rec["role"] == "input":
                a, k = _bytes_of(t), _bytes_of(rec["keep"])
                if not torch.equal(a, k):
                    i = int(torch.nonzero(a != k)[0])
                    raise AssertionError("%s: input modified (%d bytes differ, the first in element %d)" % (name, int((a != k).sum()), i // t.element_size()))
            elif rec["role"] == "output" and t.dtype.is_floating_point:
                own = self._own(rec)
                nan = torch.isnan(own)
                if bool(nan.any()):
                    raise AssertionError("%s: output not fully written: %d of %d elements are still NaN, the first at %s" % (
                        name, int(nan.sum()), own.numel(), torch.nonzero(nan)[0].tolist()))
            elif rec["role"] == "workspace" and rec["zero"]:
                b = _bytes_of(t)[rec["keep_front"]:]
                if bool(b.any()):
                    raise AssertionError("%s: zero-on-exit workspace left nonzero (%d bytes, the first at byte %d of %d)" % (
                        name, int((b != 0).sum()), rec["keep_front"] + int(torch.nonzero(b)[0]), t.numel() * t.element_size()))


class Plain(_Base):
    """ordinary fresh tensors, one allocation each (with the 512 bytes of slack on either side that a caching allocator's rounding leaves a
    neighbour-free tensor anyway, zero-filled).  Keeps what an Arena for the same sequence of calls needs."""
    SLACK = 512

    def __init__(self, device):
        super().__init__(device)
        self.need = 0
        self._last_guard = 0

    def _raw(self, nbytes, guard, offset16, name):
        self.need = _round_up(self.need + max(guard, self._last_guard), ALIGN) + (16 if offset16 else 0) + nbytes
        self._last_guard = guard
        buf = torch.zeros(self.SLACK + _round_up(nbytes, 512) + self.SLACK, dtype=torch.uint8, device=self.device)
        return buf[self.SLACK:self.SLACK + nbytes]

    def required_bytes(self):
        """size of an Arena that holds the tensors taken so far, guards included"""
        return _round_up(self.need + self._last_guard, ALIGN) + ALIGN

    def check(self):
        self.check_contents()


class Arena(_Base):
    def __init__(self, device, nbytes):
        super().__init__(device)
        nbytes = int(nbytes)
        self.buf = torch.empty(nbytes + ALIGN, dtype=torch.uint8, device=self.device)
        self.base = (-self.buf.data_ptr()) % ALIGN            # CPU allocations are not 256-byte aligned
        self.size = nbytes
        self.buf.fill_(0xFF)
        self.cur = 0
        self._last_guard = 0
        self.spans = []                                        # (name, start, end) in arena bytes, ascending

    def _raw(self, nbytes, guard, offset16, name):
        start = _round_up(self.cur + max(guard, self._last_guard), ALIGN) + (16 if offset16 else 0)
        end = start + nbytes
        if end + guard > self.size:
            raise MemoryError("arena of %d bytes is too small for %s (%d bytes + two guards of %d)" % (self.size, name, nbytes, guard))
        self.cur, self._last_guard = end, guard
        self.spans.append((name, start, end))
        return self.buf[self.base + start:self.base + end]

    def guard_before(self, i):
        """bytes of guard in front of the i-th tensor / behind it"""
        return self.spans[i][1] - (self.spans[i - 1][2] if i else 0)

    def guard_behind(self, i):
        return (self.spans[i + 1][1] if i + 1 < len(self.spans) else self.size) - self.spans[i][2]

    def check_guards(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        edges = [(None, 0, 0)] + self.spans + [(None, self.size, self.size)]
        for (pn, _, pe), (nn, ns, _) in zip(edges[:-1], edges[1:]):
            gap = self.buf[self.base + pe:self.base + ns]
            bad = gap != 0xFF
            if not bool(bad.any()):
                continue
            where = torch.nonzero(bad).reshape(-1)
            first, last, n = int(where[0]), int(where[-1]), int(where.numel())
            behind, before = first + 1, (ns - pe) - last               # byte distances from the two tensors' edges
            if nn is None or (pn is not None and behind <= before):
                raise AssertionError("guard band changed: %d bytes BEHIND %s, the nearest %d bytes past its end (the farthest %d)" % (
                    n, pn, behind, last + 1))
            raise AssertionError("guard band changed: %d bytes IN FRONT OF %s, the nearest %d bytes before its start (the farthest %d)" % (
                n, nn, before, (ns - pe) - first))

    def check(self):
        self.check_guards()
        self.check_contents()


def assert_same(got, ref, what=""):
    """bit-for-bit equality (gpu_util.assert_same; restated so that this module needs nothing else)"""
    assert got.dtype == ref.dtype and tuple(got.shape) == tuple(ref.shape), (what, got.dtype, ref.dtype, tuple(got.shape), tuple(ref.shape))
    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[got.element_size()]
    a, b = got.contiguous().view(view), ref.contiguous().view(view)
    if not torch.equal(a, b):
        bad = a != b
        idx = torch.nonzero(bad)[:5].tolist()
        raise AssertionError("%s: %d/%d elements differ between the arena run and the plain run; first idx %s arena %s plain %s" % (
            what, int(bad.sum()), bad.numel(), idx, [float(got[tuple(i)]) for i in idx], [float(ref[tuple(i)]) for i in idx]))


def audit(run, device="cuda", loose=()):
    """run(alloc) with Plain, then with an Arena of the size that needs; arena.check(); every result the same bits in both runs, except the
    names in `loose` (sums that meet in floating-point atomics), which the caller compares with the op's own reference and bar.
    Returns (plain results, arena results)."""
    plain = Plain(device)
    r0 = run(plain)
    arena = Arena(device, plain.required_bytes())
    r1 = run(arena)
    arena.check()
    assert r0.keys() == r1.keys() and len(r0) > 0
    for k in r0:
        if k not in loose:
            assert_same(r1[k], r0[k], k)
    return r0, r1
