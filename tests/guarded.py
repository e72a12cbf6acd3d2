"""Guard-banded buffers for the bounds tests of the C ABI (tests/test_gpu_bounds.py).

Every buffer a launch is given lives inside one uint8 tensor of ``guard + pad + n_bytes + guard`` bytes; the callee gets a
pointer to the inner part.  torch's caching allocator carves small tensors out of shared segments, so a kernel that writes past
its output corrupts a neighbour without any fault, and one that reads past its input picks up a neighbour's bytes without any
sign.  Here the neighbours are the guards:

  * write check: the guards are filled with a known byte before the call and compared byte for byte after it
    (``Arena.check``: synchronise, the library's last HIP error must be 0, every guard unchanged);
  * read check: a case runs once with guards (and scratch, and the outputs before the call) filled with 0x00 and once with
    0xFF - 0xFF...FF reads as NaN in float32 and float64 - and its outputs must be bit-identical (``twice``).  With the
    outputs pre-filled the same way this also checks that every output byte is written, and with the workspace filled the same
    way that nothing is read from it before it is written.

The module works on any torch device; its self-test (tests/test_guarded.py) plants overruns in CPU memory.
"""
import numpy as np
import torch

GUARD = 64 * 1024          # bytes on each side: more than any tile or vector body can overrun by
ALIGN = 256                # the inner pointer's alignment before the optional byte offset


class GuardError(AssertionError):
    pass


class GuardedBuffer:
    """``n_bytes`` of device memory between two guards.  ``offset``: bytes added to the 256-byte aligned inner start (4, 8, 12:
    the unaligned and scalar paths of the element-wise kernels)."""

    def __init__(self, name, n_bytes, device, offset=0, guard=GUARD):
        self.name, self.n_bytes, self.offset, self.guard = name, int(n_bytes), int(offset), int(guard)
        self.raw = torch.empty(self.guard + ALIGN + self.n_bytes + ALIGN + self.guard, dtype=torch.uint8, device=device)
        pad = (-(self.raw.data_ptr() + self.guard)) % ALIGN
        self.start = self.guard + pad + self.offset                 # index of the first inner byte in ``raw``
        self.end = self.start + self.n_bytes
        self.fill_byte = None

    @property
    def ptr(self):
        return self.raw.data_ptr() + self.start

    @property
    def inner(self):
        return self.raw[self.start:self.end]

    def view(self, dtype, shape=None):
        """The inner bytes as a tensor of ``dtype`` (the inner start must be aligned to its size)."""
        t = self.inner.view(dtype)
        return t if shape is None else t.view(shape)

    def fill(self, byte, guards=True, inner=True):
        """Guards (and inner bytes) to ``byte``; the guards are compared against it by ``check``."""
        if guards:
            self.raw[:self.start].fill_(byte)
            self.raw[self.end:].fill_(byte)
            self.fill_byte = int(byte)
        if inner:
            self.inner.fill_(byte)

    def put(self, data):
        """Copy ``data`` (array or tensor; its bytes, C order) into the inner part; it must be exactly n_bytes long."""
        if isinstance(data, torch.Tensor):
            b = data.detach().contiguous().reshape(-1).view(torch.uint8)
        else:
            b = torch.from_numpy(np.ascontiguousarray(data).reshape(-1).view(np.uint8))
        if b.numel() != self.n_bytes:
            raise ValueError(f'{self.name}: {b.numel()} bytes for a buffer of {self.n_bytes}')
        self.inner.copy_(b)

    def get(self, dtype=np.uint8):
        """A host copy of the inner bytes as ``dtype``."""
        return self.inner.cpu().numpy().view(dtype).copy()

    def damage(self):
        """None, or (side, offset, length) of the first damaged guard.  'after': offset of the first changed byte counted from
        the end of the buffer (0 = the byte at n_bytes); 'before': how far before the start the farthest changed byte lies
        (1 = the byte just before it).  length: from the first to the last changed byte of that guard."""
        if self.fill_byte is None:
            raise GuardError(f'{self.name}: guards were never filled')
        for side, part in (('before', self.raw[:self.start]), ('after', self.raw[self.end:])):
            bad = torch.nonzero(part != self.fill_byte).reshape(-1)
            if bad.numel():
                lo, hi = int(bad[0]), int(bad[-1])
                return side, (self.start - lo) if side == 'before' else lo, hi - lo + 1
        return None

    def check(self):
        d = self.damage()
        if d is not None:
            side, off, n = d
            where = f'{off} bytes before its start' if side == 'before' else f'at offset {off} past its end'
            raise GuardError(f'buffer {self.name!r} ({self.n_bytes} bytes, offset {self.offset}): guard {side} changed, '
                             f'first change {where}, {n} bytes changed span')


class Arena:
    """The guarded buffers of one case.  ``lib``: the HIP library (its last error is checked); None on the CPU."""

    def __init__(self, device, lib=None):
        self.device, self.lib, self.buffers = torch.device(device), lib, {}

    def alloc(self, name, n_bytes, offset=0):
        b = self.buffers[name] = GuardedBuffer(name, n_bytes, self.device, offset)
        return b

    def __getitem__(self, name):
        return self.buffers[name]

    def fill(self, byte, inner=()):
        """Every guard to ``byte``; the inner parts of the buffers named in ``inner`` (outputs, scratch) too."""
        for name, b in self.buffers.items():
            b.fill(byte, inner=name in inner)

    def check(self):
        if self.device.type == 'cuda':
            torch.cuda.synchronize(self.device)
        if self.lib is not None:
            err = self.lib.dexct_last_hip_error()
            assert err == 0, f'HIP error {err} after the launch'
        for b in self.buffers.values():
            b.check()


def twice(arena, launch, outputs, scratch=(), fills=(0x00, 0xFF)):
    """Run ``launch()`` once per fill: guards, ``outputs`` and ``scratch`` (names) filled with it before, guards checked after.
    The outputs must be bit-identical across the fills; returns their host bytes (dict name -> uint8 array) of the last run."""
    got = []
    for byte in fills:
        arena.fill(byte, inner=tuple(outputs) + tuple(scratch))
        launch()
        arena.check()
        got.append({n: arena[n].get() for n in outputs})
    for n in outputs:
        for k in range(1, len(got)):
            if not np.array_equal(got[0][n], got[k][n]):
                i = int(np.flatnonzero(got[0][n] != got[k][n])[0])
                raise GuardError(f'output {n!r} depends on bytes outside the inputs: fills 0x{fills[0]:02x} and 0x{fills[k]:02x} '
                                 f'differ first at byte {i} of {got[0][n].size}')
    return got[-1]
