"""Guard-banded bounds and per-stage value tests of the reconstruction kernels (csrc/fbp.hip) through the bare C ABI.

Method of tests/test_gpu_bounds.py (tests/guarded.py): every buffer between two 64 KiB guards, each case under a 0x00 and a
0xFF fill of guards and outputs, outputs bit-identical under both, no guard changed, dexct_last_hip_error() == 0.  Every buffer
has exactly the size include/dexct.h promises:
  dexct_fbp_parker       sino, out: 4 n_views n_rows n_ch (out = sino in the in-place cases)
  dexct_fbp_filter       sino, q: 4 lines n_ch; taps: 4 (2 n_ch - 1); weight: 4 n_ch
  dexct_fbp_backproject  q: 4 n_views n_rows n_ch; view_cs: 16 n_views; image: 4 n_rows N^2
  dexct_fdk_backproject  q, view_cs as above; row_weight: 4 n_rows; image: 4 n_slices N^2
  dexct_vmi              m1, m2, out: 4 n
  dexct_label_moments    m1, m2: 4 n; labels: n; out: 48 n_labels
Values: the kernel and a float64 NumPy reference are fed the same float32 arrays; the bounds are derived from the kernel's
arithmetic in tests/bounds_refs.py (its docstring has the derivations; tests/test_bounds_refs.py shows on the CPU that each
comparison rejects a dropped view, a shifted channel and a tap scaled by 1 + 4 n_ch u, and that the edge-pixel cap of 1 % holds
for every geometry used here).

Kernel -> test (fbp.hip):
  parker_kernel                    test_parker
  fbp_filter_kernel                test_filter (n_ch 5000 = the LDS limit), test_filter_refuses_more_than_5000_channels
  fbp_backproject_kernel<1>        test_backproject (rows 1, 7)
  fbp_backproject_kernel<8>        test_backproject (rows 8, 9, 17: a partial last group)
  fdk_backproject_kernel<4>        test_fdk_backproject (slices 1, 3, 4, 5; rows 2, 3, 9)
  vmi_kernel                       test_vmi
  label_moments_kernel             test_label_moments

Outcome and wall time: see the end of tests/test_gpu_bounds_projection.py's docstring (one record for both modules).
"""
import numpy as np
import pytest

import bounds_refs as br
from bounds_refs import F32, F64
from guarded import Arena, twice
from test_gpu_bounds import ok

pytestmark = pytest.mark.gpu

CHANNELS = [2, 3, 255, 256, 257, 5000]


def sp():
    from dex_ct_sim_amd._device import stream_ptr
    return stream_ptr()


@pytest.mark.parametrize('n_ch', CHANNELS)
@pytest.mark.parametrize('in_place', [False, True])
def test_parker(hip, n_ch, in_place):
    """A shard of a short scan (view_offset > 0, 3 rows, the views ragged against the 256-thread blocks): 2 w sino within
    2 u |ref|; in place the input is the output."""
    n_views, n_rows, view_offset, n_total = 5, 3, 6, 11
    dgamma = br.FAN / n_ch
    theta_tot = np.pi + br.FAN + 0.3
    rng = np.random.default_rng(n_ch)
    sino = (rng.uniform(0.1, 6.0, (n_views, n_rows, n_ch)) * rng.choice([-1.0, 1.0], (n_views, n_rows, n_ch))).astype(F32)
    ref, bound = br.parker_ref(sino, theta_tot, dgamma, view_offset, n_total)
    ar = Arena('cuda', hip)
    ar.alloc('sino', sino.nbytes)
    out = 'sino' if in_place else 'out'
    if not in_place:
        ar.alloc('out', sino.nbytes)

    def launch():
        ar['sino'].put(sino)
        ok(hip.dexct_fbp_parker(ar['sino'].ptr, n_views, n_rows, n_ch, theta_tot, dgamma, view_offset, n_total, ar[out].ptr, sp()))

    got = twice(ar, launch, [out])[out].view(F32).reshape(sino.shape)
    print('parker worst err / bound', br.worst(got, ref, bound))
    assert br.within(got, ref, bound), br.worst(got, ref, bound)
    assert np.any(np.abs(ref) < 0.5 * np.abs(sino)) and np.any(ref == 2.0 * sino.astype(F64))    # both ramps and the plateau


def filter_problem(n_ch, lines):
    from oracle import fbp_oracle as fo
    dgamma = br.FAN / n_ch
    rng = np.random.default_rng(n_ch + lines)
    gam = (np.arange(n_ch) - 0.5 * (n_ch - 1)) * dgamma
    taps = fo.ramp_taps(n_ch, dgamma).astype(F32)
    weight = (br.SID * np.cos(gam)).astype(F32)
    sino = rng.uniform(0.0, 8.0, (lines, n_ch)).astype(F32)
    sino[0, :] = 1.0                                                     # a flat line: the taps cancel almost completely
    return sino, taps, weight, dgamma


@pytest.mark.parametrize('n_ch', CHANNELS)
def test_filter(hip, n_ch):
    sino, taps, weight, dgamma = filter_problem(n_ch, 3)
    ref, bound = br.filter_ref(sino, taps, weight, dgamma)
    ar = Arena('cuda', hip)
    ar.alloc('sino', sino.nbytes).put(sino)
    ar.alloc('taps', 4 * (2 * n_ch - 1)).put(taps)
    ar.alloc('weight', 4 * n_ch).put(weight)
    ar.alloc('q', sino.nbytes)
    got = twice(ar, lambda: ok(hip.dexct_fbp_filter(ar['sino'].ptr, ar['taps'].ptr, ar['weight'].ptr, 3, n_ch, dgamma, ar['q'].ptr,
                                                    sp())), ['q'])['q'].view(F32).reshape(sino.shape)
    print('filter worst err / bound', br.worst(got, ref, bound))
    assert br.within(got, ref, bound), br.worst(got, ref, bound)


def test_filter_refuses_more_than_5000_channels(hip):
    """5001 channels: DEXCT_ERANGE, and nothing was launched - q still holds its fill."""
    n_ch = 5001
    ar = Arena('cuda', hip)
    ar.alloc('sino', 4 * 2 * n_ch)
    ar.alloc('taps', 4 * (2 * n_ch - 1))
    ar.alloc('weight', 4 * n_ch)
    ar.alloc('q', 4 * 2 * n_ch)
    for byte in (0x00, 0xFF):
        ar.fill(byte, inner=('sino', 'taps', 'weight', 'q'))
        assert hip.dexct_fbp_filter(ar['sino'].ptr, ar['taps'].ptr, ar['weight'].ptr, 2, n_ch, 1e-4, ar['q'].ptr, sp()) == -2
        ar.check()
        assert np.all(ar['q'].get() == byte)


@pytest.mark.parametrize('case', br.BACKPROJECT, ids=lambda c: '-'.join(str(v) for v in c))
def test_backproject(hip, case):
    p = br.backproject_problem(case)
    n_views, n_ch, n_rows, N, fov = case
    ref, bound, keep = br.backproject_ref(**p)
    assert (~keep).mean() <= 0.01
    ar = Arena('cuda', hip)
    ar.alloc('q', p['q'].nbytes).put(p['q'])
    ar.alloc('view_cs', 16 * n_views).put(p['view_cs'])
    ar.alloc('image', 4 * n_rows * N * N)
    got = twice(ar, lambda: ok(hip.dexct_fbp_backproject(ar['q'].ptr, ar['view_cs'].ptr, n_views, n_ch, n_rows, p['sid'], p['dgamma'],
                                                         p['dbeta'], N, fov, ar['image'].ptr, sp())),
                ['image'])['image'].view(F32).reshape(ref.shape)
    print('backproject worst err / bound', br.worst(got[keep], ref[keep], bound[keep]))
    assert br.within(got[keep], ref[keep], bound[keep]), br.worst(got[keep], ref[keep], bound[keep])
    assert np.all(np.isfinite(got))


@pytest.mark.parametrize('case', br.FDK, ids=lambda c: '-'.join(str(v) for v in c))
def test_fdk_backproject(hip, case):
    p = br.fdk_problem(case)
    n_views, n_ch, n_rows, N, fov, n_slices = case
    ref, bound, keep = br.fdk_ref(**p)
    assert (~keep).mean() <= 0.01
    ar = Arena('cuda', hip)
    ar.alloc('q', p['q'].nbytes).put(p['q'])
    ar.alloc('view_cs', 16 * n_views).put(p['view_cs'])
    ar.alloc('row_weight', 4 * n_rows).put(p['row_weight'])
    ar.alloc('image', 4 * n_slices * N * N)
    got = twice(ar, lambda: ok(hip.dexct_fdk_backproject(
        ar['q'].ptr, ar['view_cs'].ptr, ar['row_weight'].ptr, n_views, n_ch, n_rows, p['sid'], p['sdd'], p['dgamma'], p['dbeta'],
        p['row_z0'], p['row_dz'], p['src_z'], N, fov, n_slices, p['z0'], p['dz'], ar['image'].ptr, sp())),
        ['image'])['image'].view(F32).reshape(ref.shape)
    print('fdk worst err / bound', br.worst(got[keep], ref[keep], bound[keep]))
    assert br.within(got[keep], ref[keep], bound[keep]), br.worst(got[keep], ref[keep], bound[keep])
    assert np.all(np.isfinite(got)) and np.any(ref != 0.0)


ELEMENTS = [1, 255, 256, 257, 4099]


@pytest.mark.parametrize('n', ELEMENTS)
@pytest.mark.parametrize('hu', [0, 1])
def test_vmi(hip, n, hu):
    rng = np.random.default_rng(n)
    m1, m2 = rng.uniform(-0.2, 1.5, n).astype(F32), rng.uniform(-0.1, 2.0, n).astype(F32)
    u1, u2, uw = 0.2059, 0.5731, 0.2269
    ar = Arena('cuda', hip)
    ar.alloc('m1', 4 * n).put(m1)
    ar.alloc('m2', 4 * n).put(m2)
    ar.alloc('out', 4 * n)
    got = twice(ar, lambda: ok(hip.dexct_vmi(ar['m1'].ptr, ar['m2'].ptr, n, u1, u2, uw, hu, ar['out'].ptr, sp())),
                ['out'])['out'].view(F32)
    assert np.array_equal(got, br.vmi_ref(m1, m2, u1, u2, uw, hu))


@pytest.mark.parametrize('n', ELEMENTS)
@pytest.mark.parametrize('n_labels,with_m2,with_labels', [(1, True, False), (1, False, True), (64, True, True), (64, False, False),
                                                          (5, True, True)])
def test_label_moments(hip, n, n_labels, with_m2, with_labels):
    """Counts exact, sums within 1e-12 of the longdouble sums.  The images are positive (densities), so every sum equals the sum
    of its absolute terms and the relative tolerance is one against the terms, not against a cancelled result.  Labels run up
    to n_labels + 2: pixels with a label >= n_labels are skipped."""
    rng = np.random.default_rng(n * 64 + n_labels)
    m1, m2 = rng.uniform(0.05, 2.0, n).astype(F32), rng.uniform(0.05, 3.0, n).astype(F32)
    labels = rng.integers(0, n_labels + 3, n, dtype=np.uint8)
    ar = Arena('cuda', hip)
    ar.alloc('m1', 4 * n).put(m1)
    if with_m2:
        ar.alloc('m2', 4 * n).put(m2)
    if with_labels:
        ar.alloc('labels', n).put(labels)
    ar.alloc('out', 48 * n_labels)
    ref = br.moments_ref(m1, m2 if with_m2 else None, labels if with_labels else None, n_labels)
    for byte in (0x00, 0xFF):             # (float64 atomics in unspecified order: the sums of the two fills may differ in the last bits)
        got = twice(ar, lambda: ok(hip.dexct_label_moments(ar['m1'].ptr, ar['m2'].ptr if with_m2 else None,
                                                           ar['labels'].ptr if with_labels else None, n, n_labels, ar['out'].ptr, sp())),
                    ['out'], fills=(byte,))['out'].view(F64).reshape(n_labels, 6)
        assert np.array_equal(got[:, 0], ref[:, 0].astype(F64))
        np.testing.assert_allclose(got[:, 1:], ref[:, 1:].astype(F64), rtol=1e-12, atol=0.0)
