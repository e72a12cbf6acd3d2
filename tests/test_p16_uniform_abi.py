"""The additive entry points of the column-class map (include/dexct_p16_uniform.h): declared there and not in include/dexct.h,
which includes that header; exported by the library; required and typed by the binding; the class encoding of the header is the
one of csrc/uniform_count.h and of the binding."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_library_and_binding_agree():
    from dex_ct_sim_amd import _native
    ext = open(os.path.join(ROOT, 'include', 'dexct_p16_uniform.h')).read()
    main = open(os.path.join(ROOT, 'include', 'dexct.h')).read()
    declared = sorted(set(re.findall(r'^(?:int|int64_t)\s+(dexct_[a-z_0-9]+)\s*\(', ext, re.M)))
    assert declared == sorted(_native.P16_UNIFORM_SYMBOLS)
    assert not set(declared) & set(_native.SYMBOLS) and not set(declared) & set(_native.GN_DEDUP_SYMBOLS)
    assert '#include "dexct_p16_uniform.h"' in main and '#include "dexct.h"' in ext
    assert re.search(rf'#define DEXCT_COL_UNIFORM {_native.COL_UNIFORM}u\b', ext)
    assert re.search(rf'#define DEXCT_COL_CLASS_BITS {_native.COL_CLASS_BITS}\b', ext)
    pure = open(os.path.join(ROOT, 'dex-ct-sim_amd', 'csrc', 'uniform_count.h')).read()
    assert re.search(rf'constexpr uint32_t kUniform = {_native.COL_UNIFORM}u;', pure)
    assert 'MapKind{3u, 7u, 2u, 7u}' in pure                 # eight columns per word, four bits apart: DEXCT_COL_CLASS_BITS
    raw = ctypes.CDLL(_native.LIB_PATH)
    assert all(hasattr(raw, name) for name in declared)
    lib = _native.load()
    assert lib.dexct_volume_column_classes.restype is ctypes.c_int and lib.dexct_siddon_project_packed_uniform.restype is ctypes.c_int
    assert len(lib.dexct_volume_column_classes.argtypes) == len(lib.dexct_volume_air_columns.argtypes)
    assert len(lib.dexct_siddon_project_packed_uniform.argtypes) == len(lib.dexct_siddon_project_packed_skip.argtypes) + 2


def test_refusals_need_no_device():
    """Null pointers and impossible shapes are refused before anything touches the device."""
    from dex_ct_sim_amd import _native
    lib = _native.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    assert lib.dexct_volume_column_classes(None, 4, 4, 16, p, p, None) == -1
    assert lib.dexct_volume_column_classes(p, 4, 4, 16, None, p, None) == -1
    assert lib.dexct_volume_column_classes(p, 4, 4, 16, p, None, None) == -1
    assert lib.dexct_volume_column_classes(p, 0, 4, 16, p, p, None) == -1
    assert lib.dexct_volume_column_classes(p, 4, 4, 18, p, p, None) == -1
    assert lib.dexct_volume_column_classes(p, 65536, 32768, 16, p, p, None) == -2
