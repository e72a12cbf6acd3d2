"""Self-test of the guard-band helper (tests/guarded.py) in CPU memory: it must see a planted overrun and underrun, say where
they are, and see a read of bytes outside the buffer.  This tests the test; nothing here touches a GPU."""
import numpy as np
import pytest
import torch

from guarded import ALIGN, GUARD, Arena, GuardError, GuardedBuffer, twice


@pytest.mark.parametrize('offset', [0, 4, 8, 12])
@pytest.mark.parametrize('fill', [0x00, 0xFF])
def test_planted_overrun_and_underrun_are_found_at_their_offset(offset, fill):
    b = GuardedBuffer('out', 1000, 'cpu', offset)
    assert b.ptr % ALIGN == offset and b.start >= GUARD and b.raw.numel() - b.end >= GUARD
    b.fill(fill)
    b.inner.fill_(0x5A)                       # the callee may write all of its own bytes
    b.check()
    b.raw[b.end + 5:b.end + 9] = fill ^ 0x01  # 4 bytes, 5 past the end
    with pytest.raises(GuardError, match=r"'out'.*guard after.*offset 5 past its end, 4 bytes"):
        b.check()
    assert b.damage() == ('after', 5, 4)
    b.fill(fill, inner=False)
    b.raw[b.end] = fill ^ 0x80               # the first byte past the end; one more far out in the guard
    b.raw[b.end + GUARD - 1] = fill ^ 0x80
    assert b.damage() == ('after', 0, GUARD)
    b.fill(fill, inner=False)
    b.raw[b.start - 16:b.start - 8] = fill ^ 0x10       # 8 bytes, ending 8 before the start
    with pytest.raises(GuardError, match=r'guard before.*16 bytes before its start, 8 bytes'):
        b.check()
    assert b.damage() == ('before', 16, 8)
    b.fill(fill, inner=False)
    b.raw[b.start - 1] = fill ^ 0x01
    assert b.damage() == ('before', 1, 1)
    b.fill(fill, inner=False)
    b.check()


def test_inner_views_and_copies():
    a = Arena('cpu')
    x = a.alloc('x', 8 * 7)
    a.alloc('y', 4 * 7, offset=4)
    x.put(np.arange(7, dtype=np.float64))
    assert np.array_equal(x.get(np.float64), np.arange(7.0))
    assert torch.equal(x.view(torch.float64, (7,)), torch.arange(7, dtype=torch.float64))
    a['y'].put(torch.arange(7, dtype=torch.float32))
    assert np.array_equal(a['y'].get(np.float32), np.arange(7, dtype=np.float32))
    with pytest.raises(ValueError):
        x.put(np.zeros(8))


def test_twice_sees_writes_and_reads_outside_the_buffer():
    a = Arena('cpu')
    src, dst = a.alloc('src', 4 * 65, offset=4), a.alloc('dst', 4 * 65, offset=8)
    data = np.linspace(1.0, 2.0, 65, dtype=np.float32)

    def copy():
        src.put(data)
        dst.inner.copy_(src.inner)

    got = twice(a, copy, ['dst'])
    assert np.array_equal(got['dst'].view(np.float32), data)
    with pytest.raises(GuardError, match="'dst'.*guard after.*offset 0 past its end, 4 bytes"):
        twice(a, lambda: (copy(), dst.raw[dst.end:dst.end + 4].fill_(0x5A)), ['dst'])
    # reads one float past the end of src and writes it inside dst (dst one longer than src says): only the fills see it
    a2 = Arena('cpu')
    src, dst = a2.alloc('src', 4 * 64), a2.alloc('dst', 4 * 65)

    def over_read():
        src.put(data[:64])
        dst.inner.copy_(src.raw[src.start:src.end + 4])

    with pytest.raises(GuardError, match="output 'dst' depends on bytes outside the inputs.*byte 256"):
        twice(a2, over_read, ['dst'])
    # an output byte the callee never writes keeps the fill: seen the same way
    with pytest.raises(GuardError, match="output 'dst'.*byte 256"):
        twice(a2, lambda: (src.put(data[:64]), dst.raw[dst.start:dst.end - 4].copy_(src.inner)), ['dst'])
