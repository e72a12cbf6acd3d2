"""ctypes binding of libdexct_hip.so (include/dexct.h).  No fallback: if the library is missing or
does not export the ABI the import of the compute modules fails loudly."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, 'libdexct_hip.so')
ABI_VERSION = 6

# every entry point include/dexct.h declares
SYMBOLS = ['dexct_strerror', 'dexct_abi_version', 'dexct_last_hip_error', 'dexct_volume_layouts', 'dexct_fan_plan',
           'dexct_siddon_project', 'dexct_siddon_trace', 'dexct_gn_decompose', 'dexct_gn_apply_mask', 'dexct_gn_model_sums',
           'dexct_reduce_max', 'dexct_transpose_batched', 'dexct_fbp_filter', 'dexct_fbp_backproject',
           'dexct_add_noise', 'dexct_volume_groups', 'dexct_siddon_project_grouped', 'dexct_cone_project',
           'dexct_cone_layout', 'dexct_cone_project_rows', 'dexct_volume_pack2', 'dexct_siddon_project_packed', 'dexct_volume_groups_pack2',
           'dexct_siddon_project_grouped_packed', 'dexct_poisson_detect', 'dexct_vmi', 'dexct_label_moments', 'dexct_fdk_backproject', 'dexct_sino_allgather', 'dexct_sino_gather', 'dexct_transpose_log', 'dexct_host_pin', 'dexct_host_touch', 'dexct_host_unpin', 'dexct_download',
           'dexct_volume_ids', 'dexct_volume_remap', 'dexct_fbp_parker', 'dexct_sino_log', 'dexct_cone_layout_groups', 'dexct_cone_project_grouped',
           'dexct_bhc_linearize', 'dexct_image_project', 'dexct_image_backproject', 'dexct_sirt_residual', 'dexct_sirt_update',
           'dexct_gn_reduced_rows', 'dexct_gn_decompose_multi', 'dexct_gn_covariance', 'dexct_cov_quadform',
           'dexct_fbp_var_filter', 'dexct_fbp_var_backproject', 'dexct_fdk_var_backproject',
           'dexct_cov_precision', 'dexct_pwls_majorizer', 'dexct_pwls_residual', 'dexct_pwls_update',
           'dexct_volume_air_columns', 'dexct_siddon_project_packed_skip',
           'dexct_cone_layout_bytes', 'dexct_gn_workspace_bytes', 'dexct_gn_multi_workspace_bytes', 'dexct_gn_cov_workspace_bytes']
# the size queries return int64_t; dexct_strerror a string; every other entry point an int status
SIZE_QUERIES = ['dexct_cone_layout_bytes', 'dexct_gn_workspace_bytes', 'dexct_gn_multi_workspace_bytes',
                'dexct_gn_cov_workspace_bytes']
# what include/dexct_gn_dedup.h declares (additive to ABI 6: the lists above are those of include/dexct.h): the entry point
# (int status) and its size query (int64_t); load() requires and types them like the others
GN_DEDUP_SYMBOLS = ['dexct_gn_decompose_dedup', 'dexct_gn_dedup_workspace_bytes']
# what include/dexct_p16_uniform.h declares (additive to ABI 6 in the same way): the column-class map of a packed volume and the
# packed projection that takes it (both int status)
P16_UNIFORM_SYMBOLS = ['dexct_volume_column_classes', 'dexct_siddon_project_packed_uniform']
COL_UNIFORM, COL_CLASS_BITS = 1, 4   # DEXCT_COL_UNIFORM, DEXCT_COL_CLASS_BITS: a column's class is COL_UNIFORM | id << 1, or 0 (mixed)
# what include/dexct_p16_tiles.h declares (additive to ABI 6 in the same way): the tile map of a column-class map, its size query
# (int64_t) and the packed projection that takes it (int status)
P16_TILES_SYMBOLS = ['dexct_volume_tile_map_words', 'dexct_volume_tile_classes', 'dexct_siddon_project_packed_tiles']
TILE_SIDE = 8                        # DEXCT_TILE_SIDE


class FanGeom(C.Structure):
    """dexct_fan_geom"""
    _fields_ = [('n_views', C.c_int32), ('n_channels', C.c_int32), ('n_rows', C.c_int32), ('z_first', C.c_int32),
                ('nx', C.c_int32), ('ny', C.c_int32), ('nz', C.c_int32), ('pad_', C.c_int32),
                ('dx', C.c_double), ('dy', C.c_double), ('dz', C.c_double), ('sid', C.c_double), ('sdd', C.c_double)]


class LogOut(C.Structure):
    """dexct_log_out: the optional second output of get_sino, sino_log = ln(air / counts)"""
    _fields_ = [('sino_log', C.c_void_p), ('air', C.c_float * 4)]


def log_out(sino_log_ptr, air):
    """byref-able dexct_log_out, or None when no log sinogram is wanted."""
    if sino_log_ptr is None:
        return None
    lo = LogOut()
    lo.sino_log = sino_log_ptr
    for k in range(4):
        lo.air[k] = float(air[k]) if k < len(air) else 1.0
    return C.byref(lo)


class Noise(C.Structure):
    """dexct_noise (ABI 6): quantum noise drawn by the projection kernel itself"""
    _fields_ = [('seed', C.c_uint64), ('sample', C.c_int32), ('reserved_', C.c_int32)]


def noise(seed, sample=True):
    """byref-able dexct_noise, or None (``seed`` None): the kernel samples counts = max(signal + sqrt(variance) z, 1e-20)."""
    if seed is None:
        return None
    return C.byref(Noise(int(seed) & (2 ** 64 - 1), 1 if sample else 0, 0))


class GnOptions(C.Structure):
    """dexct_gn_options (ABI 5)"""
    _fields_ = [('stop_tol', C.c_double), ('out_rows', C.c_int32), ('out_channels', C.c_int32), ('kernel', C.c_int32),
                ('gn_pass', C.c_int32), ('iterations', C.c_void_p), ('start', C.c_void_p), ('flags', C.c_int32),
                ('blocks_per_cu', C.c_int32)]


GN_PASS_COUNT, GN_PASS_SHORTCUT = 1, 2
GN_FLAG_FULL_LOOP, GN_FLAG_NATURAL_ORDER, GN_FLAG_ONE_STEP, GN_FLAG_FULL_RESIDUAL = 1, 2, 4, 8
GN_REDUCED_HEADER = 16   # DEXCT_GN_REDUCED_HEADER
GN_WS_EXECUTED, GN_WS_PROGRESS, GN_WS_QUEUE_HEAD, GN_WS_STALLS, GN_WS_RESIDUAL_ROWS = 72, 80, 88, 96, 104   # DEXCT_GN_WS_*: byte offsets
GN_WS_WORDS = slice(GN_WS_EXECUTED, GN_WS_RESIDUAL_ROWS + 8)   # ... of the workspace's diagnostic uint64 words; the span of all five
GN_DEDUP_USE, GN_DEDUP_FRESH, GN_DEDUP_CAP = 0, 8, 16   # DEXCT_GN_DEDUP_*: byte offsets of the dedup workspace's descriptor words
GN_TABLE_ROW = 14        # doubles per energy row of the Newton tables (csrc/gn.hip, kTab)
GN_MAX_MEAS, GN_MAX_MATS = 4, 3   # DEXCT_GN_MAX_MEAS, DEXCT_GN_MAX_MATS (dexct_gn_decompose_multi)
GN_MULTI_FULL_LOOP = 1   # DEXCT_GN_MULTI_FULL_LOOP
FBP_VAR_MAX_CHANNELS = 2730   # DEXCT_FBP_VAR_MAX_CHANNELS (dexct_fbp_var_filter)
COV_ESTIMATOR, COV_CRLB = 0, 1   # DEXCT_COV_* (dexct_gn_covariance)


def gn_options(stop_tol=None, out_rows=0, out_channels=0, kernel=0, gn_pass=0, iterations=None, start=None, flags=0,
               blocks_per_cu=0):
    """byref-able dexct_gn_options; ``stop_tol=None`` asks for the library default (a negative value in the struct).
    ``gn_pass`` / ``iterations`` (device address of n_pix bytes: the step counts of GN_PASS_COUNT) / ``start`` (device address of
    the table of the reference's fixed points: GN_PASS_SHORTCUT): the Newton short cut; ``flags``: GN_FLAG_*;
    ``blocks_per_cu``: workgroups per CU of the queue kernels, 0 = default (include/dexct.h)."""
    o = GnOptions(-1.0 if stop_tol is None else float(stop_tol), int(out_rows), int(out_channels), int(kernel), int(gn_pass),
                  iterations, start, int(flags), int(blocks_per_cu))
    return C.byref(o)


def gn_reduced_rows(mus, nodes, w):
    """dexct_gn_reduced_rows on host arrays: the block (NumPy float64) a reduced residual rule adds to the device copy of a start
    array - header of GN_REDUCED_HEADER doubles, then the kept rows in the format of the Newton tables."""
    import numpy as np
    lib = load()
    mus = np.ascontiguousarray(mus, dtype=np.float64)
    nodes = np.ascontiguousarray(nodes, dtype=np.int32)
    w = np.ascontiguousarray(w, dtype=np.float64)
    if mus.ndim != 2 or mus.shape[0] != 2 or w.shape != (2, nodes.size):
        raise ValueError('mus must be [2, nE] and w [2, len(nodes)]')
    block = np.zeros(GN_REDUCED_HEADER + GN_TABLE_ROW * nodes.size)
    w0, w1 = np.ascontiguousarray(w[0]), np.ascontiguousarray(w[1])
    check(lib.dexct_gn_reduced_rows(mus.ctypes.data, mus.shape[1], nodes.ctypes.data, nodes.size, w0.ctypes.data, w1.ctypes.data,
                                    block.ctypes.data, block.size), 'dexct_gn_reduced_rows')
    return block[:int(block[9])]


PLAN_BYTES = 40   # sizeof(dexct_ray_plan)


class DexctError(RuntimeError):
    pass


_lib = None


def load():
    """Load the HIP library; raises if it is absent (build with __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DexctError(f'{LIB_PATH} not found: the HIP extension is not built '
                         f'(run `python -c "import __graft_entry__ as g; g.build()"` or `make -C dex-ct-sim_amd/csrc`). '
                         f'There is no CPU fallback.')
    lib = C.CDLL(LIB_PATH)
    for name in SYMBOLS + GN_DEDUP_SYMBOLS + P16_UNIFORM_SYMBOLS + P16_TILES_SYMBOLS:
        if not hasattr(lib, name):
            raise DexctError(f'{LIB_PATH} does not export {name}')
    lib.dexct_strerror.restype = C.c_char_p
    lib.dexct_strerror.argtypes = [C.c_int]
    if lib.dexct_abi_version() != ABI_VERSION:
        raise DexctError(f'ABI version mismatch: library {lib.dexct_abi_version()}, binding {ABI_VERSION}')
    vp, i32, i64, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    lib.dexct_volume_layouts.argtypes = [vp, i32, i32, i32, vp, vp, vp]
    lib.dexct_volume_ids.argtypes = [vp, i64, vp, vp]
    lib.dexct_volume_remap.argtypes = [vp, i64, C.POINTER(C.c_uint8), vp]
    lib.dexct_fan_plan.argtypes = [C.POINTER(FanGeom), vp, vp, i32, i32, vp, vp]
    lib.dexct_siddon_project.argtypes = [C.POINTER(FanGeom), vp, i32, i32, vp, vp, vp, i32, i32, i32, vp, vp, vp,
                                         vp, i32, i32, vp, vp, vp, vp]
    lib.dexct_sino_log.argtypes = [vp, C.POINTER(C.c_float), i32, i64, vp, vp]
    lib.dexct_add_noise.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, C.c_uint64, vp]
    lib.dexct_volume_groups.argtypes = [vp, i64, i32, vp, vp]
    lib.dexct_vmi.argtypes = [vp, vp, i64, f64, f64, f64, i32, vp, vp]
    lib.dexct_bhc_linearize.argtypes = [vp, i64, vp, i32, i32, i32, i32, vp, vp]
    lib.dexct_image_project.argtypes = [C.POINTER(FanGeom), vp, i32, i32, i32, vp, vp, vp, vp]
    lib.dexct_image_backproject.argtypes = [C.POINTER(FanGeom), vp, i32, i32, i32, vp, vp, vp, i32, vp]
    lib.dexct_sirt_residual.argtypes = [vp, vp, vp, i32, i32, i64, vp, vp, vp]
    lib.dexct_sirt_update.argtypes = [vp, vp, vp, i64, f64, i32, vp]
    lib.dexct_cov_precision.argtypes = [vp, i64, i32, f64, vp, vp]
    lib.dexct_pwls_majorizer.argtypes = [vp, vp, i64, i32, vp, vp]
    lib.dexct_pwls_residual.argtypes = [vp, vp, vp, vp, i64, i32, i32, i32, i64, vp, vp, vp]
    lib.dexct_pwls_update.argtypes = [vp, vp, vp, i32, i32, i32, i32, f64, C.POINTER(f64), C.POINTER(f64), i32, vp, vp, vp]
    lib.dexct_label_moments.argtypes = [vp, vp, vp, i64, i32, vp, vp]
    lib.dexct_sino_allgather.argtypes = [vp, vp, i64, vp, vp]
    lib.dexct_sino_gather.argtypes = [vp, vp, C.POINTER(i64), C.POINTER(i64), i32, i32, i32, vp, vp]
    lib.dexct_host_pin.argtypes = [vp, i64, i32]
    lib.dexct_host_unpin.argtypes = [vp, i32]
    lib.dexct_host_touch.argtypes = [vp, i64, i32]
    lib.dexct_download.argtypes = [vp, vp, i64, vp]
    lib.dexct_fdk_backproject.argtypes = [vp, vp, vp, i32, i32, i32, f64, f64, f64, f64, f64, f64, f64, i32, f64, i32,
                                          f64, f64, vp, vp]
    lib.dexct_poisson_detect.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, C.c_uint64, vp, vp]
    lib.dexct_cone_project.argtypes = [C.POINTER(FanGeom), vp, vp, vp, vp, f64, f64, i32, i32, vp, vp, i32, i32, i32, vp, vp,
                                       vp, vp, vp, vp, vp, vp, vp]
    lib.dexct_volume_pack2.argtypes = [vp, i64, vp, vp]
    lib.dexct_volume_groups_pack2.argtypes = [vp, i64, i32, vp, vp]
    lib.dexct_siddon_project_packed.argtypes = [C.POINTER(FanGeom), vp, i32, i32, vp, i32, i32, i32, vp, vp, vp, vp, i32, vp, vp,
                                                vp, vp, vp]
    lib.dexct_volume_air_columns.argtypes = [vp, i32, i32, i32, vp, vp, vp]
    lib.dexct_siddon_project_packed_skip.argtypes = lib.dexct_siddon_project_packed.argtypes[:-1] + [vp, i64, vp]
    lib.dexct_volume_column_classes.argtypes = [vp, i32, i32, i32, vp, vp, vp]
    lib.dexct_siddon_project_packed_uniform.argtypes = lib.dexct_siddon_project_packed.argtypes[:-1] + [vp, i64, vp, C.POINTER(i64), vp]
    lib.dexct_volume_column_classes.restype = lib.dexct_siddon_project_packed_uniform.restype = C.c_int
    lib.dexct_volume_tile_map_words.argtypes = [i32, i32]
    lib.dexct_volume_tile_classes.argtypes = [vp, i32, i32, vp, vp, vp]
    lib.dexct_siddon_project_packed_tiles.argtypes = lib.dexct_siddon_project_packed_uniform.argtypes[:-1] + [vp, C.POINTER(i64), vp]
    lib.dexct_volume_tile_classes.restype = lib.dexct_siddon_project_packed_tiles.restype = C.c_int
    lib.dexct_volume_tile_map_words.restype = i64
    lib.dexct_cone_layout.argtypes = [vp, i32, i32, i32, vp, vp]
    lib.dexct_cone_project_rows.argtypes = [C.POINTER(FanGeom), vp, vp, vp, vp, f64, f64, i32, i32, vp, i32, i32, i32, vp, vp, vp,
                                            vp, vp, vp, vp, vp, vp]
    lib.dexct_cone_layout_groups.argtypes = [vp, i32, i32, i32, i32, vp, vp]
    lib.dexct_cone_project_grouped.argtypes = [C.POINTER(FanGeom), vp, vp, vp, vp, f64, f64, i32, i32, vp, i32, i32, i32, vp, vp, vp,
                                               vp, vp, vp, vp, vp, vp, vp]
    lib.dexct_cone_layout_bytes.argtypes = [i32, i32, i32]
    lib.dexct_siddon_project_grouped.argtypes = [C.POINTER(FanGeom), vp, i32, i32, vp, i32, i32, i32, vp, vp, vp, vp, vp,
                                                 i32, vp, vp, vp, vp, vp]
    lib.dexct_siddon_project_grouped_packed.argtypes = lib.dexct_siddon_project_grouped.argtypes
    lib.dexct_transpose_batched.argtypes = [vp, vp, i64, i32, i32, i32, vp]
    lib.dexct_transpose_log.argtypes = [vp, vp, vp, C.POINTER(C.c_float), i32, i64, i32, i32, vp]
    lib.dexct_fbp_filter.argtypes = [vp, vp, vp, i64, i32, f64, vp, vp]
    lib.dexct_fbp_parker.argtypes = [vp, i32, i32, i32, f64, f64, i32, i32, vp, vp]
    lib.dexct_fbp_backproject.argtypes = [vp, vp, i32, i32, i32, f64, f64, f64, i32, f64, vp, vp]
    lib.dexct_fbp_var_filter.argtypes = [vp, i32, i32, i32, i32, vp, vp, f64, f64, i32, i32, vp, vp, vp]
    lib.dexct_fbp_var_backproject.argtypes = [vp, vp, vp, i32, i32, i32, i32, f64, f64, f64, i32, f64, vp, vp]
    lib.dexct_fdk_var_backproject.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, f64, f64, f64, f64, f64, f64, f64, i32, f64, i32,
                                              f64, f64, vp, vp]
    lib.dexct_siddon_trace.argtypes = [C.POINTER(FanGeom), vp, vp, i32, i32, vp, vp, vp, vp]
    lib.dexct_gn_decompose.argtypes = [vp, vp, i32, i64, vp, vp, i32, i32, i32, i32, i32, i32, vp, f64, vp, C.POINTER(GnOptions), vp, vp]
    lib.dexct_gn_workspace_bytes.argtypes = [i32, i32]
    lib.dexct_gn_decompose_dedup.argtypes = lib.dexct_gn_decompose.argtypes[:-1] + [vp, vp]
    lib.dexct_gn_dedup_workspace_bytes.argtypes = [i64, i32, i32]
    lib.dexct_gn_apply_mask.argtypes = [vp, i32, i64, f64, vp, vp]
    lib.dexct_gn_model_sums.argtypes = [vp, i64, vp, vp, i32, vp, vp, vp, vp]
    lib.dexct_reduce_max.argtypes = [vp, i32, i64, vp, vp]
    lib.dexct_gn_reduced_rows.argtypes = [vp, i32, vp, i32, vp, vp, vp, i64]
    lib.dexct_gn_decompose_multi.argtypes = [vp, i32, i64, i32, i32, vp, vp, i32, i32, vp, f64, i32, vp, vp, vp]
    lib.dexct_gn_multi_workspace_bytes.argtypes = [i32, i32, i32]
    lib.dexct_gn_covariance.argtypes = [vp, i64, i32, i32, vp, vp, vp, i32, i32, vp, i32, vp, f64, vp, vp, vp]
    lib.dexct_cov_quadform.argtypes = [vp, i64, i32, vp, vp, vp]
    lib.dexct_gn_cov_workspace_bytes.argtypes = [i32, i32, i32]
    for name in SYMBOLS[1:]:
        getattr(lib, name).restype = i64 if name in SIZE_QUERIES else C.c_int
    lib.dexct_gn_decompose_dedup.restype, lib.dexct_gn_dedup_workspace_bytes.restype = C.c_int, i64
    _lib = lib
    return lib


def check(code, what):
    if code != 0:
        lib = load()
        msg = lib.dexct_strerror(code).decode()
        extra = f' (hipError {lib.dexct_last_hip_error()})' if code == -3 else ''
        raise DexctError(f'{what}: {msg}{extra}')
