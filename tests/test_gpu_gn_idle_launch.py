"""The Newton launch that finds its queue used up (csrc/gn.hip gn_queue_used_up): on the dedup route the pass is launched twice,
on the list and on the sinograms, the device decides which of the two has work, and the other one's blocks leave at their first
line.  Nothing a caller sees may depend on that:

  * small sinograms of 1 - 3 views x 33 channels x 64 and 130 rows through the route WITH repeats (use = 1: the direct launch
    is the idle one), WITHOUT (the probe votes no: the launch on the list is the idle one) and with dedup=False (no second
    launch: the queue starts at 0 and the test at the top only costs its load);
  * the one-step short cut, the two-step short cut and pass 0 (gn_shortcut_kernel<1>, <2>, gn_refill_kernel<false>), with and
    without the mask;
  * a_out is the direct route's, byte for byte, between guard bands, with a_out and the dedup workspace pre-filled with 0x00 and
    with 0xFF;
  * every word last_gn_stats() reports - executed steps, stalls, launches, mode, the residual's rows - equals the direct route's
    where the direct launch worked, and where the list's launch worked that of a plain call on the list's own entries: the launch
    with work wrote the diagnostic words, the idle one added nothing; the finished-pixel word is n_pix either way.
"""
import numpy as np
import pytest
import torch

from gn_route_cases import MODES, call, route_equals_direct
from test_gpu_gn_dedup import LIGHT, pool, sinogram  # noqa: F401  (pool: the fixture)

pytestmark = pytest.mark.gpu

SHAPES = ((1, 33, 64), (2, 33, 130), (3, 33, 64), (3, 33, 130))


@pytest.mark.parametrize('mask', [False, True], ids=['plain', 'mask'])
@pytest.mark.parametrize('how', list(MODES))
def test_the_idle_launch_changes_nothing(hip, pool, how, mask):
    for V, C, R in SHAPES:
        for dtype in ((np.float32,) if R == 64 else (np.float32, np.float64)):
            seed = 100 * V + R
            repeats = sinogram(pool, V, C, R, dtype, patterns=LIGHT, seed=seed)
            assert route_equals_direct(hip, pool, repeats, how, mask)['use'] == 1, (V, C, R)
            none = sinogram(pool, V, C, R, dtype, patterns=('different',), seed=seed + 1)
            assert route_equals_direct(hip, pool, none, how, mask) == {'use': 0, 'F': 0, 'cap': V * C * R // 8 // 64 * 64, 'launches': 1}


@pytest.mark.parametrize('how', list(MODES))
def test_without_the_route_the_queue_starts_at_zero(hip, pool, how):
    """dedup=False twice: the same bytes, the same words, every pixel finished."""
    for V, C, R in SHAPES[1:3]:
        t = torch.from_numpy(sinogram(pool, V, C, R, np.float32, patterns=LIGHT, seed=V + R)).cuda()
        for mask in (False, True):
            a, st, dd, done = call(pool, t, how, mask, False)
            b, st2, dd2, done2 = call(pool, t, how, mask, False)
            assert dd is None and dd2 is None and done == done2 == V * C * R
            assert st == st2 and st['pixel_iterations'] > 0
            assert torch.equal(a.view(torch.int64), b.view(torch.int64))
