"""dexct_reduce_max with 16-byte loads: any pointer and length.  Lengths around the vector, the wave and the block, one
past what the capped grid covers with one vector per thread; the pointer 0-3 elements into a larger allocation (the
elements before the first 16-byte boundary and after the last whole vector go one by one); the maximum, and a NaN, at
the first, the last and an unaligned middle element; all -inf.  Against torch.max on the same slice: the same value,
NaN where torch gives NaN."""
import math

import pytest
import torch

from grid_caps import CAPS

pytestmark = pytest.mark.gpu

CAP_BLOCKS = CAPS['kReduceMaxBlocks'][1]
# the last two: one vector per thread of the capped grid and a little more (a second trip of the one-vector loop), and
# past four float4 per thread (the loop with four loads in flight runs, then the one-vector loop, then the tail)
LENGTHS = [1, 3, 4, 5, 255, 256, 257, 1023, 1025, CAP_BLOCKS * 256 * 4 + 5, CAP_BLOCKS * 256 * 4 * 5 + 7]


def reduce_max(lib, x, out):
    from dex_ct_sim_amd._device import ptr, stream_ptr
    assert lib.dexct_reduce_max(ptr(x), int(x.dtype == torch.float64), x.numel(), ptr(out), stream_ptr()) == 0
    return float(out.item())


@pytest.mark.parametrize('offset', [0, 1, 2, 3])
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_reduce_max_any_pointer_and_length(hip, dtype, offset):
    dev = torch.device('cuda:0')
    gen = torch.Generator(device='cpu').manual_seed(offset + 10 * int(dtype == torch.float64))
    big = (torch.rand(max(LENGTHS) + 8, generator=gen, dtype=torch.float64) * 1e4 - 5e3).to(dtype).to(dev)
    out = torch.zeros(1, dtype=torch.float64, device=dev)
    for n in LENGTHS:
        x = big[offset:offset + n]
        assert x.data_ptr() == big.data_ptr() + offset * big.element_size()
        assert reduce_max(hip, x, out) == float(torch.max(x)), n
        for pos in sorted({0, n - 1, min(n - 1, (n // 2) | 1)}):
            keep = x[pos].clone()
            x[pos] = 1e30                                   # the maximum sits here
            assert reduce_max(hip, x, out) == float(torch.max(x)) == float(x[pos]), (n, pos)
            x[pos] = float('nan')
            assert math.isnan(float(torch.max(x))) and math.isnan(reduce_max(hip, x, out)), (n, pos)
            x[pos] = keep
        assert reduce_max(hip, x, out) == float(torch.max(x)), n      # (restored)
    x = big[offset:offset + 1025]
    x.fill_(float('-inf'))
    assert reduce_max(hip, x, out) == float('-inf')
