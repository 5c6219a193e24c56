"""Guard bands around caller buffers.

The kernels are handed ordinary torch tensors everywhere else in the suite; the caching allocator rounds each of them up and places it
between unrelated blocks, so a store or a load that runs past a buffer's end is invisible there.  An Arena is ONE uint8 allocation that
holds every buffer of a case as [guard | payload | guard]:

    a = Arena("cuda", 0x00)
    a.request("obs", (B, C, H, W), torch.uint8, align=1, init=obs)   # an input: copied in, inputs_unchanged() compares it
    a.request("q", (B, A), torch.float32, align=4)                   # an output: prefilled with 0x77
    a.request("ring", (S, n), torch.uint8, align=1, init=ring, inout=True)   # read and written: copied in, exempt from inputs_unchanged(),
                                                                     # part of outputs() -- the caller compares ALL of it with the reference
    q = a.take("q")                                                  # the first take() sizes and fills the allocation
    ... launch ...
    a.check(); a.inputs_unchanged()

Every guard is GUARD (64 KiB) bytes of `fill` -- a store one whole row or sample off still lands in it.  A payload starts at a 256-byte
boundary plus `align` bytes (aligned to `align` and to nothing coarser) and its ragged end touches the next guard directly.  A case runs
once with fill 0x00 and once with 0xFF: the two differ in every bit, as uint8 (0 / 255), int32 (0 / -1), f32 and f16 (0.0 / NaN), so an
output that depends on a guard byte cannot have equal bits in both runs.

take(name, shape, dtype, align, init, inout) requests and takes in one call while the arena is still unsized."""
import numpy as np
import torch

GUARD = 64 * 1024
OUT_FILL = 0x77
FILLS = (0x00, 0xFF)


def _itemsize(dtype):
    return torch.empty((), dtype=dtype).element_size()


class _Buf:
    __slots__ = ("name", "shape", "dtype", "align", "init", "inout", "lo", "start", "nbytes", "hi_end")


class Arena:
    def __init__(self, device, fill):
        assert 0 <= int(fill) <= 255
        self.device = torch.device(device)
        self.fill = int(fill)
        self._bufs = {}
        self._raw = None
        self._mem = None

    # ---- layout ------------------------------------------------------------------------------------------------------------
    def request(self, name, shape, dtype, align, init=None, inout=False):
        assert self._mem is None, "the arena is already sized: request every buffer before the first take()"
        assert name not in self._bufs, f"buffer {name!r} requested twice"
        align = int(align)
        assert align >= 1 and 256 % align == 0, "align must be a power of two up to 256"
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        isz = _itemsize(dtype)
        assert align % isz == 0 or isz == 1, f"{name}: a {dtype} payload cannot sit at {align}-byte alignment"
        b = _Buf()
        b.name, b.shape, b.dtype, b.align = name, shape, dtype, align
        b.nbytes = int(np.prod(shape, dtype=np.int64)) * isz
        b.init, b.inout = None, bool(inout)
        assert init is not None or not inout, f"{name}: an in/out buffer starts from its init"
        if init is not None:
            t = torch.as_tensor(init).detach().to("cpu").contiguous()
            assert t.dtype == dtype and tuple(t.shape) == shape, f"{name}: init is {t.dtype} {tuple(t.shape)}, wanted {dtype} {shape}"
            b.init = t.reshape(-1).view(torch.uint8).clone() if t.numel() else torch.empty(0, dtype=torch.uint8)
        self._bufs[name] = b

    def _build(self):
        cur = 0
        for b in self._bufs.values():
            b.lo = cur                                               # the low guard starts where the previous high guard ended
            b.start = -(-(cur + GUARD) // 256) * 256 + b.align
            b.hi_end = b.start + b.nbytes + GUARD
            cur = b.hi_end
        total = -(-max(cur, 1) // 256) * 256
        if self._bufs:
            list(self._bufs.values())[-1].hi_end = total             # the last guard runs to the end of the allocation
        self.total = total
        self._raw = torch.empty(total + 256, dtype=torch.uint8, device=self.device)
        base = (-self._raw.data_ptr()) % 256
        self._mem = self._raw[base:base + total]
        assert self._mem.data_ptr() % 256 == 0 and self._mem.numel() % 256 == 0
        self._mem.fill_(self.fill)
        for b in self._bufs.values():
            p = self._mem[b.start:b.start + b.nbytes]
            if b.init is None:
                p.fill_(OUT_FILL)
            else:
                p.copy_(b.init)

    def take(self, name, shape=None, dtype=None, align=None, init=None, inout=False):
        if name not in self._bufs:
            self.request(name, shape, dtype, align, init, inout)
        if self._mem is None:
            self._build()
        b = self._bufs[name]
        t = self._mem[b.start:b.start + b.nbytes]
        if b.dtype != torch.uint8:
            t = t.view(b.dtype)
        t = t.view(b.shape)
        a = t.data_ptr()
        assert a % b.align == 0 and (b.align == 256 or a % (2 * b.align) != 0), (name, a, b.align)
        return t

    def ptr(self, name):
        return self.take(name).data_ptr()

    def raw(self):
        """The whole allocation as bytes (tests of the helper itself write strays through it)."""
        if self._mem is None:
            self._build()
        return self._mem

    def span(self, name):
        """(low guard start, payload start, payload end, high guard end) as byte offsets into raw()."""
        if self._mem is None:
            self._build()
        b = self._bufs[name]
        return b.lo, b.start, b.start + b.nbytes, b.hi_end

    # ---- checks ------------------------------------------------------------------------------------------------------------
    def check(self):
        """Every guard still holds `fill` (compared on the device); names the buffer, the side and the first changed offset
        (relative to the payload: negative below it, >= nbytes above it)."""
        if self._mem is None:
            self._build()
        sides = []
        for b in self._bufs.values():
            sides.append((b, "low", b.lo, b.start))
            sides.append((b, "high", b.start + b.nbytes, b.hi_end))
        bad = torch.stack([(self._mem[s:e] != self.fill).any() for (_, _, s, e) in sides]).cpu().numpy()
        for hit, (b, side, s, e) in zip(bad, sides):
            if hit:
                idx = int(torch.nonzero(self._mem[s:e] != self.fill)[0, 0])
                off = s + idx - b.start
                val = int(self._mem[s + idx])
                raise AssertionError(f"guard of buffer {b.name!r} changed on its {side} side: first at payload offset {off} "
                                     f"(payload is {b.nbytes} bytes), holds 0x{val:02x}, guard byte 0x{self.fill:02x}")

    def inputs_unchanged(self):
        if self._mem is None:
            self._build()
        for b in self._bufs.values():
            if b.init is None or b.inout:
                continue
            now = self._mem[b.start:b.start + b.nbytes].cpu()
            if not torch.equal(now, b.init):
                idx = int(torch.nonzero(now != b.init)[0, 0])
                raise AssertionError(f"input buffer {b.name!r} changed: first at byte {idx} of {b.nbytes}")

    def bytes_of(self, name):
        """The payload's bytes on the host (comparison between the two fills)."""
        b = self._bufs[name]
        return self.take(name).reshape(-1).view(torch.uint8).cpu().numpy().copy() if b.nbytes else np.zeros(0, np.uint8)

    def outputs(self):
        """{name: payload bytes} of every buffer that had no init, and of every in/out buffer."""
        return {n: self.bytes_of(n) for n, b in self._bufs.items() if b.init is None or b.inout}

    def verify(self):
        """(a) and (b) of the rule; returns outputs() for (c) and (d)."""
        if self.device.type == "cuda":
            torch.cuda.synchronize()
        self.check()
        self.inputs_unchanged()
        return self.outputs()


def same_bits(out0, out1):
    """(c): the outputs of the 0x00 run and of the 0xFF run are bit-identical."""
    assert out0.keys() == out1.keys()
    for k in out0:
        if not np.array_equal(out0[k], out1[k]):
            idx = int(np.nonzero(out0[k] != out1[k])[0][0])
            raise AssertionError(f"output {k!r} depends on the guard bytes: first difference at byte {idx}")
