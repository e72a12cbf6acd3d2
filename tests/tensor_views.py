"""Layout and dtype variants of one conforming array, for the tensor-contract tests (tests/test_tensor_views.py on the CPU,
tests/test_gpu_tensor_contract.py on the device).

``variants(x)`` yields recipes; ``recipe.build(device)`` makes a tensor whose LOGICAL content equals ``x`` but whose strides,
storage offset or dtype differ from the dense tensor an entry point documents.  A wrapper that hands ``data_ptr()`` to a kernel
without looking at the layout then computes from other bytes - the parent's filler - and the result differs.

THE IN-BOUNDS RULE.  Every view is carved out of a parent allocation of this module, padded so that a reader that ignores the
layout and takes ``numel`` elements of up to 8 bytes from the data pointer stays inside the parent: with off = storage_offset x
itemsize, the parent holds at least off + max(span of the view, numel x 8) bytes and, for good measure, off more.  ``in_bounds``
asserts exactly that from the tensor's metadata before ``build`` returns, so no case built here can make a kernel touch memory
the test does not own, whichever way the code under test is wrong.  It is arithmetic, not a measurement: the CPU test runs it for
every recipe at every shape the GPU module uses.
"""
import numpy as np
import torch

FILL = 3.0                  # what the parent holds outside the view: finite, positive (counts), exact in every dtype used
WIDEST = 8                  # bytes of the widest element a kernel may assume (float64)


# every shape tests/test_gpu_tensor_contract.py builds a variant at (tests/test_tensor_views.py checks the in-bounds rule at each)
GPU_SHAPES = [(), (4, 16, 8), (4, 15, 6), (197,), (2, 48), (3, 48), (2, 60), (4, 8, 16, 2), (4, 6, 15, 2), (197, 2),      # Newton
              (3, 4, 16, 8), (3, 197), (4, 16, 8, 2), (4, 16, 8, 3),                                                    # K x M, covariance
              (12, 16), (12, 9, 16), (12, 4, 16), (12, 16, 3), (12, 9, 16, 3),                                          # FBP
              (3, 5), (2, 5), (2, 6, 16, 53), (2, 6, 53, 16), (2, 6, 10, 53), (2, 6, 53, 10),                           # projection
              (2, 52, 16, 2), (2, 37, 16, 2), (2, 52, 2, 16), (2, 37, 2, 16),                                           # transpose_log
              (3, 9, 13), (7, 2, 53), (2, 7, 2, 53), (3, 7, 2, 53), (2, 3, 9, 13)]                                      # the matched pair


def _dense_strides(shape):
    st, n = [], 1
    for d in reversed(shape):
        st.append(n)
        n *= d
    return tuple(reversed(st))


def _span(shape, strides):
    """elements from the first to one past the last element a view addresses"""
    return 0 if 0 in shape else 1 + sum((d - 1) * s for d, s in zip(shape, strides))


def in_bounds(t, itemsize=WIDEST):
    """Assert the in-bounds rule for tensor ``t`` (``itemsize``: the widest element a reader or writer may assume); returns t."""
    off = t.storage_offset() * t.element_size()
    have = t.untyped_storage().nbytes()
    need = off + max(_span(tuple(t.shape), tuple(t.stride())) * t.element_size(), t.numel() * itemsize)
    assert have >= need + off, (tuple(t.shape), tuple(t.stride()), t.storage_offset(), str(t.dtype), have, need + off)
    return t


class Recipe:
    """One variant: ``name``, the torch ``dtype``, element ``strides`` and ``offset`` of the view in a flat parent.  ``conforms``:
    dense and of the array's own dtype (the offset variants) - a call given it must compute what it computes from the plain
    tensor, refusal is not accepted."""

    def __init__(self, name, x, dtype, strides, offset, conforms=False):
        self.name, self.x, self.dtype, self.strides, self.offset, self.conforms = name, x, dtype, tuple(strides), int(offset), conforms
        self.shape = tuple(x.shape)
        itemsize = torch.empty((), dtype=dtype).element_size()
        n = int(np.prod(self.shape))
        need = self.offset * itemsize + max(_span(self.shape, self.strides) * itemsize, n * WIDEST) + self.offset * itemsize
        self.parent_numel = -(-need // itemsize)

    def build(self, device):
        parent = torch.full((self.parent_numel,), FILL, dtype=self.dtype, device=device)
        view = parent.as_strided(self.shape, self.strides, self.offset)
        src = torch.from_numpy(np.array(self.x)).to(device=device, dtype=self.dtype)
        if 0 in self.strides and view.numel():         # a broadcast axis: one copy of the data serves every index along it
            keep = tuple(slice(0, 1) if s == 0 else slice(None) for s in self.strides)
            view[keep].copy_(src[keep])
        else:
            view.copy_(src)
        return in_bounds(view)

    def __repr__(self):
        return self.name


def torch_dtype(x):
    return torch.from_numpy(np.empty(0, x.dtype)).dtype


def variants(x, dtypes=True):
    """The recipes of the conforming host array ``x`` (float32 or float64; integer-valued and below 2048 where the dtype variants
    are to reproduce it exactly).  ``dtypes=False`` leaves the dtype variants out; ``'exact'`` keeps the one that reproduces any
    float32 array exactly, its float64 copy."""
    x = np.asarray(x)
    dt, shape, dense = torch_dtype(x), tuple(x.shape), _dense_strides(x.shape)
    out = [Recipe('offset1', x, dt, dense, 1, conforms=True), Recipe('offset3', x, dt, dense, 3, conforms=True)]
    if x.ndim >= 1 and shape[-1] > 1:
        doubled = _dense_strides(shape[:-1] + (2 * shape[-1],))
        out.append(Recipe('every_other', x, dt, doubled[:-1] + (2,), 0))
    if x.ndim >= 2 and shape[-1] > 1 and shape[-2] > 1:
        swapped = _dense_strides(shape[:-2] + (shape[-1], shape[-2]))
        out.append(Recipe('transposed', x, dt, swapped[:-2] + (swapped[-1], swapped[-2]), 0))
    if x.size > 1:
        out.append(Recipe('plane_of_pair', x, dt, tuple(2 * s for s in dense), 1))
    if x.ndim >= 2 and shape[0] > 1 and np.array_equal(x, np.broadcast_to(x[:1], shape)):
        out.append(Recipe('broadcast', x, dt, (0,) + dense[1:], 0))
    if dtypes == 'exact':
        return out + ([Recipe('float64', x, torch.float64, dense, 0)] if dt == torch.float32 else [])
    if dtypes:
        other = torch.float64 if dt == torch.float32 else torch.float32
        for d in (other, torch.float16, torch.int32):
            out.append(Recipe(str(d).replace('torch.', ''), x, d, dense, 0))
    return out


def plain(x, device):
    """The conforming tensor itself: dense, of x's dtype, at the start of its own allocation."""
    return torch.from_numpy(np.array(x)).to(device)


def written_variants(shape, dtype):
    """Named constructors ``f(device) -> tensor`` of outputs a call must refuse, all inside the in-bounds rule for ``dtype``:
    the wrong dtype (of at least the documented byte count) and a non-dense view of the right element count.  Outputs of the
    wrong SIZE and host tensors cannot meet the rule: the CPU tests alone build them, and nothing is launched there."""
    n = int(np.prod(shape))
    size = torch.empty((), dtype=dtype).element_size()
    wrong = torch.float32 if dtype == torch.float64 else torch.float64

    def wrong_dtype(device):
        parent = torch.zeros(2 * n, dtype=wrong, device=device)
        return in_bounds(parent[:n].view(shape), WIDEST)

    def non_dense(device):
        parent = torch.zeros(2 * n * max(1, WIDEST // size), dtype=dtype, device=device)
        return in_bounds(parent.as_strided(tuple(shape), tuple(2 * s for s in _dense_strides(shape)), 0), WIDEST)

    return {'wrong_dtype': wrong_dtype, 'non_dense': non_dense}


def same_bytes(a, b):
    """byte-identical, NaN for NaN: same shape, dtype and bit pattern"""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8)))
