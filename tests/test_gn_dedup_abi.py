"""The additive entry points of the dedup route (include/dexct_gn_dedup.h): declared there and not in include/dexct.h, which
includes that header; exported by the library; required and typed by the binding; the size query is that of
csrc/gn_dedup_index.h and returns int64."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_library_and_binding_agree():
    from dex_ct_sim_amd import _native
    ext = open(os.path.join(ROOT, 'include', 'dexct_gn_dedup.h')).read()
    main = open(os.path.join(ROOT, 'include', 'dexct.h')).read()
    declared = sorted(set(re.findall(r'^(?:int|int64_t)\s+(dexct_[a-z_0-9]+)\s*\(', ext, re.M)))
    assert declared == sorted(_native.GN_DEDUP_SYMBOLS) and not set(declared) & set(_native.SYMBOLS)
    assert '#include "dexct_gn_dedup.h"' in main and '#include "dexct.h"' in ext
    for macro, value in (('DEXCT_GN_DEDUP_USE', _native.GN_DEDUP_USE), ('DEXCT_GN_DEDUP_FRESH', _native.GN_DEDUP_FRESH),
                         ('DEXCT_GN_DEDUP_CAP', _native.GN_DEDUP_CAP)):
        assert re.search(rf'#define {macro} {value}\b', ext), macro
    raw = ctypes.CDLL(_native.LIB_PATH)
    assert all(hasattr(raw, name) for name in declared)
    lib = _native.load()
    assert lib.dexct_gn_decompose_dedup.restype is ctypes.c_int and lib.dexct_gn_dedup_workspace_bytes.restype is ctypes.c_int64
    assert len(lib.dexct_gn_decompose_dedup.argtypes) == len(lib.dexct_gn_decompose.argtypes) + 1


def test_workspace_size():
    from dex_ct_sim_amd import _native
    size = _native.load().dexct_gn_dedup_workspace_bytes
    assert size(0, 512, 0) == 0 and size(1024, 0, 0) == 0 and size(1000, 512, 0) == 0        # not whole lines
    n, rows = 409600000, 512
    cap = n // 8 // 64 * 64
    up = lambda b: -(-b // 256) * 256
    for is64, elem in ((0, 4), (1, 8)):
        want = up(64) + up(n // 8) + 2 * up(4 * (n // rows)) + up(4 * -(-(n // rows) // 1024)) + 2 * up(cap * elem) + up(cap * 16)
        assert size(n, rows, is64) == want
    assert 1.25e9 < size(n, rows, 0) < 1.35e9
    big = size(2 ** 31 - 512, 512, 1)
    assert big > 2 ** 31                                                                     # comes back whole
