"""ctypes mirror of include/sz.h and include/szhip.h (sz_amd/csrc/libszhip.so)."""
import ctypes
import dataclasses
import os
import subprocess

import numpy as np

ABS, REL, VR_REL, ABS_AND_REL, ABS_OR_REL, PSNR, NORM, PW_REL = 0, 1, 1, 2, 3, 4, 5, 10
SZ_FLOAT, SZ_DOUBLE = 0, 1
SZ_BEST_SPEED, SZ_BEST_COMPRESSION, SZ_DEFAULT_COMPRESSION = 0, 1, 2
SZ_SCES, SZ_NSCS = 0, -1

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")


def lib_path():
    """The product library; SZ_AMD_LIB names another build of it (variants)."""
    return os.environ.get("SZ_AMD_LIB") or os.path.join(_CSRC, "libszhip.so")


class SZError(RuntimeError):
    pass


class sz_params(ctypes.Structure):  # include/sz.h (reference sz/include/sz.h:164-198)
    _fields_ = [("dataType", ctypes.c_int), ("max_quant_intervals", ctypes.c_uint),
                ("quantization_intervals", ctypes.c_uint), ("maxRangeRadius", ctypes.c_uint),
                ("sol_ID", ctypes.c_int), ("losslessCompressor", ctypes.c_int), ("sampleDistance", ctypes.c_int),
                ("predThreshold", ctypes.c_float), ("szMode", ctypes.c_int), ("gzipMode", ctypes.c_int),
                ("errorBoundMode", ctypes.c_int), ("absErrBound", ctypes.c_double), ("relBoundRatio", ctypes.c_double),
                ("psnr", ctypes.c_double), ("normErr", ctypes.c_double), ("pw_relBoundRatio", ctypes.c_double),
                ("segment_size", ctypes.c_int), ("pwr_type", ctypes.c_int), ("protectValueRange", ctypes.c_int),
                ("fmin", ctypes.c_float), ("fmax", ctypes.c_float), ("dmin", ctypes.c_double), ("dmax", ctypes.c_double),
                ("snapshotCmprStep", ctypes.c_int), ("predictionMode", ctypes.c_int),
                ("accelerate_pw_rel_compression", ctypes.c_int), ("plus_bits", ctypes.c_int),
                ("randomAccess", ctypes.c_int), ("withRegression", ctypes.c_int)]


class szhip_params(ctypes.Structure):  # include/szhip.h
    _fields_ = [("sample_distance", ctypes.c_int), ("pred_threshold", ctypes.c_float),
                ("max_quant_intervals", ctypes.c_uint), ("quantization_intervals", ctypes.c_uint), ("flags", ctypes.c_uint)]


class szhip_stats(ctypes.Structure):  # include/szhip.h
    _fields_ = [("ms_total", ctypes.c_double), ("ms_prequant", ctypes.c_double), ("ms_quant", ctypes.c_double),
                ("ms_entropy", ctypes.c_double), ("ms_host", ctypes.c_double),
                ("n_elements", ctypes.c_uint64), ("n_blocks", ctypes.c_uint64), ("n_reg_blocks", ctypes.c_uint64),
                ("n_unpred", ctypes.c_uint64), ("intervals", ctypes.c_uint), ("use_mean", ctypes.c_int),
                ("out_bytes", ctypes.c_uint64), ("quant_kernel_launches", ctypes.c_uint64), ("vmin", ctypes.c_double), ("vmax", ctypes.c_double), ("chain_overlapped", ctypes.c_int), ("quant_kernel", ctypes.c_int), ("packing", ctypes.c_int),
                ("book_on_device", ctypes.c_int)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class szhip_batch_item(ctypes.Structure):  # include/szhip.h: one array of szhip_compress_omp_batch / szhip_decompress_omp_batch
    _fields_ = [("data", ctypes.c_void_p), ("out", ctypes.c_void_p), ("eb", ctypes.c_double), ("meta", ctypes.c_void_p), ("stream", ctypes.c_void_p),
                ("stream_len", ctypes.c_size_t), ("body_off", ctypes.c_size_t),
                ("offset", ctypes.c_size_t), ("size", ctypes.c_size_t), ("rc", ctypes.c_int), ("intervals", ctypes.c_uint), ("n_unpred", ctypes.c_uint64),
                ("quant_kernel", ctypes.c_int), ("batched", ctypes.c_int)]


class szhip_batch_shape(ctypes.Structure):  # include/szhip.h: the shape (dim 0 slowest) and box count of one array of the *_batch_shapes calls
    _fields_ = [("r0", ctypes.c_size_t), ("r1", ctypes.c_size_t), ("r2", ctypes.c_size_t), ("thread_num", ctypes.c_int)]


class szhip_batch_region(ctypes.Structure):  # include/szhip.h: the sub-box and destination pitches of one item of szhip_decompress_omp_batch_region
    _fields_ = [("lo", ctypes.c_size_t * 3), ("hi", ctypes.c_size_t * 3), ("pitch0", ctypes.c_size_t), ("pitch1", ctypes.c_size_t),
                ("n_boxes", ctypes.c_uint64), ("shares", ctypes.c_int)]


class szhip_book_record(ctypes.Structure):  # include/szhip.h
    _fields_ = [("n_nodes", ctypes.c_uint32), ("tree_bytes", ctypes.c_uint32), ("max_len", ctypes.c_uint32), ("status", ctypes.c_uint32),
                ("total_bits", ctypes.c_uint64), ("total_unpred", ctypes.c_uint64)]


class szhip_quality(ctypes.Structure):  # include/szhip.h: what szhip_compare / szhip_compare_view fill
    _fields_ = [(k, ctypes.c_uint64) for k in ("n", "n_excluded", "n_excluded_diff", "n_zero_changed", "n_over_abs", "n_over_pwr", "n_over_both",
                                               "max_abs_idx", "first_over_idx")] + \
               [(k, ctypes.c_double) for k in ("vmin", "vmax", "max_abs_err", "max_pw_rel_err", "sum_ori", "sum_dec", "sum_dec_sq", "sum_err_sq",
                                               "cov", "var_ori", "var_dec", "range", "mse", "psnr", "nrmse", "norm_err", "ac_eff")]


SZHIP_Q_CORR = 1
NO_INDEX = 2 ** 64 - 1              # max_abs_idx / first_over_idx when there is no such point
# the fields of szhip_quality as Python numbers, and the struct's bytes (`raw`: two calls on the same input give the same bytes)
Quality = dataclasses.make_dataclass("Quality", [(k, int if t is ctypes.c_uint64 else float) for k, t in szhip_quality._fields_] + [("raw", bytes)], frozen=True)


def _quality(q):
    return Quality(**{k: getattr(q, k) for k, _ in szhip_quality._fields_}, raw=bytes(q))


class szhost_meta(ctypes.Structure):  # sz_amd/csrc/szhost.h
    _fields_ = [("data_type", ctypes.c_int), ("err_mode", ctypes.c_int), ("abs_bound", ctypes.c_double),
                ("rel_ratio", ctypes.c_double), ("psnr", ctypes.c_double), ("pwr_ratio", ctypes.c_double), ("vmin", ctypes.c_double),
                ("vmax", ctypes.c_double), ("opt_quant_mode", ctypes.c_int), ("data_endian", ctypes.c_int),
                ("sz_mode", ctypes.c_int), ("gzip_mode", ctypes.c_int), ("sample_distance", ctypes.c_int),
                ("pred_threshold", ctypes.c_float), ("sol_id", ctypes.c_int), ("max_quant_intervals", ctypes.c_uint),
                ("quantization_intervals", ctypes.c_uint), ("protect_value_range", ctypes.c_int)]


def build_library(force=False):
    """Compile every HIP/C source for gfx950 into sz_amd/csrc/libszhip.so (hipcc cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-s", "-C", _CSRC, "clean"])
    subprocess.check_call(["make", "-s", "-C", _CSRC])
    return lib_path()


_lib = None


def lib():
    """Load the product library; raises (loudly) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    p = lib_path()
    if not os.path.exists(p):
        raise SZError(f"{p} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    _lib = _bind(ctypes.CDLL(p))
    return _lib


def _bind(L):
    """Declare the C prototypes on a loaded library object."""
    sz = ctypes.c_size_t
    L.SZ_Init.argtypes = [ctypes.c_char_p]; L.SZ_Init.restype = ctypes.c_int
    L.SZ_Init_Params.argtypes = [ctypes.POINTER(sz_params)]; L.SZ_Init_Params.restype = ctypes.c_int
    L.SZ_Finalize.argtypes = []; L.SZ_Finalize.restype = None
    L.SZ_compress.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(sz)] + [sz] * 5
    L.SZ_compress.restype = ctypes.c_void_p
    L.SZ_compress_args.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(sz), ctypes.c_int,
                                   ctypes.c_double, ctypes.c_double, ctypes.c_double] + [sz] * 5
    L.SZ_compress_args.restype = ctypes.c_void_p
    L.SZ_decompress.argtypes = [ctypes.c_int, ctypes.c_void_p, sz] + [sz] * 5
    L.SZ_decompress.restype = ctypes.c_void_p
    L.SZ_hip_last_stats.argtypes = [ctypes.POINTER(szhip_stats)]; L.SZ_hip_last_stats.restype = ctypes.c_int
    L.SZ_hip_set_device.argtypes = [ctypes.c_int]
    L.szhip_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int]; L.szhip_create.restype = ctypes.c_int
    L.szhip_destroy.argtypes = [ctypes.c_void_p]; L.szhip_destroy.restype = None
    L.szhip_last_error.argtypes = [ctypes.c_void_p]; L.szhip_last_error.restype = ctypes.c_char_p
    L.szhip_minmax.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, sz,
                               ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    L.szhip_minmax.restype = ctypes.c_int
    L.szhip_compress.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, sz, sz, sz, ctypes.c_double,
                                 ctypes.POINTER(szhip_params), ctypes.c_char_p, sz, ctypes.c_int,
                                 ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(sz), ctypes.POINTER(szhip_stats)]
    L.szhip_compress.restype = ctypes.c_int
    if hasattr(L, "szhip_pool_create"):
        L.szhip_pool_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int]; L.szhip_pool_create.restype = ctypes.c_int
        L.szhip_pool_destroy.argtypes = [ctypes.c_void_p]; L.szhip_pool_destroy.restype = None
        L.szhip_pool_submit.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, sz, sz, sz, ctypes.c_double,
                                        ctypes.POINTER(szhip_params), ctypes.c_char_p, sz, ctypes.c_int, ctypes.c_void_p, sz, ctypes.POINTER(ctypes.c_int)]
        L.szhip_pool_submit.restype = ctypes.c_int
        L.szhip_pool_wait.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(sz), ctypes.POINTER(szhip_stats)]
        L.szhip_pool_wait.restype = ctypes.c_int
    L.szhip_decompress.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, sz, sz, sz, sz, sz,
                                   ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(szhip_stats)]
    L.szhip_decompress.restype = ctypes.c_int
    L.szhip_compress_sz14.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, sz, sz, sz, ctypes.c_double,
                                      ctypes.c_double, ctypes.c_double, ctypes.POINTER(szhip_params), ctypes.c_char_p, sz, ctypes.c_int,
                                      ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(sz), ctypes.POINTER(szhip_stats)]
    L.szhip_compress_sz14.restype = ctypes.c_int
    L.szhip_decompress_sz14.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, sz, sz, sz, sz, sz,
                                        ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(szhip_stats)]
    L.szhip_decompress_sz14.restype = ctypes.c_int
    L.szhip_debug_fetch.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, sz]; L.szhip_debug_fetch.restype = ctypes.c_int
    if hasattr(L, "szhip_compress_omp"):
        L.szhip_compress_omp.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, sz, sz, sz, ctypes.c_double, ctypes.c_int,
                                         ctypes.POINTER(szhip_params), ctypes.c_char_p, sz, ctypes.c_int,
                                         ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(sz), ctypes.POINTER(szhip_stats)]
        L.szhip_compress_omp.restype = ctypes.c_int
        L.szhip_decompress_omp.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, sz, sz, sz, sz, sz,
                                           ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(szhip_stats)]
        L.szhip_decompress_omp.restype = ctypes.c_int
    if hasattr(L, "szhip_decompress_omp_region"):
        L.szhip_decompress_omp_region.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, sz, sz, sz, sz, sz,
                                                  ctypes.POINTER(sz), ctypes.POINTER(sz), ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(szhip_stats)]
        L.szhip_decompress_omp_region.restype = ctypes.c_int
    if hasattr(L, "szhip_compress_omp_view"):
        L.szhip_compress_omp_view.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, sz, sz, sz, sz, sz, ctypes.c_double, ctypes.c_int,
                                              ctypes.POINTER(szhip_params), ctypes.c_char_p, sz, ctypes.c_int,
                                              ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(sz), ctypes.POINTER(szhip_stats)]
        L.szhip_compress_omp_view.restype = ctypes.c_int
        L.szhip_decompress_omp_view.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, sz, sz, sz, sz, sz,
                                                ctypes.c_void_p, ctypes.c_int, sz, sz, ctypes.POINTER(szhip_stats)]
        L.szhip_decompress_omp_view.restype = ctypes.c_int
        L.szhip_pack_view.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, sz, sz, sz, sz, sz, ctypes.POINTER(ctypes.c_void_p)]
        L.szhip_pack_view.restype = ctypes.c_int
        L.szhip_scatter_view.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, sz, sz, sz, ctypes.c_void_p, ctypes.c_int, sz, sz]
        L.szhip_scatter_view.restype = ctypes.c_int
    if hasattr(L, "szhip_compress_omp_batch"):
        L.szhip_compress_omp_batch.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(szhip_batch_item), ctypes.c_int, ctypes.c_int, sz, sz, sz, ctypes.c_int,
                                               ctypes.POINTER(szhip_params), sz, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(sz), ctypes.POINTER(szhip_stats)]
        L.szhip_compress_omp_batch.restype = ctypes.c_int
        L.szhip_decompress_omp_batch.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(szhip_batch_item), ctypes.c_int, ctypes.c_int, sz, sz, sz, ctypes.c_int,
                                                 ctypes.POINTER(szhip_stats)]
        L.szhip_decompress_omp_batch.restype = ctypes.c_int
    if hasattr(L, "szhip_compress_omp_batch_shapes"):
        L.szhip_compress_omp_batch_shapes.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(szhip_batch_item), ctypes.POINTER(szhip_batch_shape), ctypes.c_int, ctypes.c_int,
                                                      ctypes.POINTER(szhip_params), sz, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(sz), ctypes.POINTER(szhip_stats)]
        L.szhip_compress_omp_batch_shapes.restype = ctypes.c_int
        L.szhip_decompress_omp_batch_shapes.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(szhip_batch_item), ctypes.POINTER(szhip_batch_shape), ctypes.c_int, ctypes.c_int,
                                                        ctypes.c_int, ctypes.POINTER(szhip_stats)]
        L.szhip_decompress_omp_batch_shapes.restype = ctypes.c_int
        L.szhip_minmax_batch_lens.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(sz), ctypes.c_int, ctypes.c_int,
                                              ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(szhip_stats)]
        L.szhip_minmax_batch_lens.restype = ctypes.c_int
    if hasattr(L, "szhip_decompress_omp_batch_region"):
        L.szhip_decompress_omp_batch_region.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(szhip_batch_item), ctypes.POINTER(szhip_batch_shape),
                                                        ctypes.POINTER(szhip_batch_region), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(szhip_stats)]
        L.szhip_decompress_omp_batch_region.restype = ctypes.c_int
        L.SZ_hip_decompress_batch_regions.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(sz), ctypes.POINTER(sz), ctypes.POINTER(sz),
                                                      ctypes.POINTER(sz), ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.POINTER(sz)]
        L.SZ_hip_decompress_batch_regions.restype = ctypes.c_int
    if hasattr(L, "SZ_hip_compress_args_batch_shapes"):
        L.SZ_hip_compress_args_batch_shapes.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                                        ctypes.POINTER(sz), ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(sz), ctypes.POINTER(ctypes.c_int)]
        L.SZ_hip_compress_args_batch_shapes.restype = ctypes.c_int
        L.SZ_hip_decompress_batch_shapes.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(sz), ctypes.POINTER(ctypes.c_void_p), ctypes.c_int,
                                                     ctypes.POINTER(sz)]
        L.SZ_hip_decompress_batch_shapes.restype = ctypes.c_int
    if hasattr(L, "SZ_hip_compress_openmp_batch"):
        L.SZ_hip_compress_openmp_batch.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.POINTER(ctypes.c_double), sz, sz, sz,
                                                   ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(sz)]
        L.SZ_hip_compress_openmp_batch.restype = ctypes.c_int
        L.SZ_hip_decompress_openmp_batch.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(sz), ctypes.POINTER(ctypes.c_void_p),
                                                     ctypes.c_int, sz, sz, sz]
        L.SZ_hip_decompress_openmp_batch.restype = ctypes.c_int
    if hasattr(L, "SZ_hip_compress_region"):
        L.SZ_hip_compress_region.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(sz), ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double] + [sz] * 5 + \
                                            [ctypes.POINTER(sz), ctypes.POINTER(sz)]
        L.SZ_hip_compress_region.restype = ctypes.c_void_p
        L.SZ_hip_decompress_into_region.argtypes = [ctypes.c_int, ctypes.c_void_p, sz, ctypes.c_void_p] + [sz] * 5 + [ctypes.POINTER(sz), ctypes.POINTER(sz)]
        L.SZ_hip_decompress_into_region.restype = ctypes.c_int
    if hasattr(L, "szhip_huff_book"):
        L.szhip_huff_book.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p, sz, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.POINTER(szhip_book_record)]
        L.szhip_huff_book.restype = ctypes.c_int
    if hasattr(L, "SZ_hip_decompress_region"):
        L.SZ_hip_decompress_region.argtypes = [ctypes.c_int, ctypes.c_void_p, sz] + [sz] * 5 + [ctypes.POINTER(sz), ctypes.POINTER(sz)]
        L.SZ_hip_decompress_region.restype = ctypes.c_void_p
        L.sz_slab_compress.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(sz), ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double, sz, sz, sz, ctypes.c_int]
        L.sz_slab_compress.restype = ctypes.c_void_p
        L.sz_slab_decompress.argtypes = [ctypes.c_void_p, sz, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(sz * 3)]
        L.sz_slab_decompress.restype = ctypes.c_void_p
        L.sz_slab_decompress_region.argtypes = [ctypes.c_void_p, sz, ctypes.POINTER(sz), ctypes.POINTER(sz), ctypes.POINTER(ctypes.c_int)]
        L.sz_slab_decompress_region.restype = ctypes.c_void_p
    if hasattr(L, "SZ_hip_compress_device"):
        L.SZ_hip_compress_device.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(sz), ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double] + [sz] * 5
        L.SZ_hip_compress_device.restype = ctypes.c_void_p
        L.SZ_hip_compress_device_into.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, sz, ctypes.POINTER(sz), ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                                  ctypes.c_double] + [sz] * 5
        L.SZ_hip_compress_device_into.restype = ctypes.c_int
        L.SZ_hip_decompress_device.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, sz, ctypes.c_void_p] + [sz] * 5
        L.SZ_hip_decompress_device.restype = ctypes.c_int
        L.szhip_store_be.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, sz, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        L.szhip_store_be.restype = ctypes.c_int
        L.szhip_load_be.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, sz, ctypes.c_void_p]
        L.szhip_load_be.restype = ctypes.c_int
        L.szhip_fill.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, sz, ctypes.c_void_p]
        L.szhip_fill.restype = ctypes.c_int
        L.szhip_clamp.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, sz, ctypes.c_double, ctypes.c_double]
        L.szhip_clamp.restype = ctypes.c_int
    if hasattr(L, "szhip_compare"):
        L.szhip_compare.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, sz, ctypes.c_double, ctypes.c_double,
                                    ctypes.c_uint, ctypes.POINTER(szhip_quality)]
        L.szhip_compare.restype = ctypes.c_int
        L.szhip_compare_view.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, sz, sz, ctypes.c_void_p, ctypes.c_int, sz, sz, sz, sz, sz,
                                         ctypes.c_double, ctypes.c_double, ctypes.c_uint, ctypes.POINTER(szhip_quality)]
        L.szhip_compare_view.restype = ctypes.c_int
        for f in (L.SZ_hip_compare, L.SZ_hip_compare_device):
            f.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p] + [sz] * 5 + [ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.POINTER(szhip_quality)]
            f.restype = ctypes.c_int
        L.SZ_hip_print_quality.argtypes = [ctypes.POINTER(szhip_quality), sz, ctypes.c_int]; L.SZ_hip_print_quality.restype = None
    if hasattr(L, "szhip_minmax_batch"):
        vpp, dp = ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_double)
        L.szhip_minmax_batch.argtypes = [ctypes.c_void_p, ctypes.c_int, vpp, ctypes.c_int, ctypes.c_int, sz, dp, dp, ctypes.POINTER(szhip_stats)]
        L.szhip_minmax_batch.restype = ctypes.c_int
        L.szhip_compare_batch.argtypes = [ctypes.c_void_p, ctypes.c_int, vpp, vpp, ctypes.c_int, ctypes.c_int, sz, dp, dp, ctypes.c_uint,
                                          ctypes.POINTER(szhip_quality), ctypes.POINTER(szhip_stats)]
        L.szhip_compare_batch.restype = ctypes.c_int
    if hasattr(L, "szhip_compress_omp_batch_view"):
        vpp, dp = ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_double)
        L.szhip_compress_omp_batch_view.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(szhip_batch_item), ctypes.c_int, ctypes.c_int, sz, sz, sz, sz, sz, ctypes.c_int,
                                                    ctypes.POINTER(szhip_params), sz, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(sz),
                                                    ctypes.POINTER(szhip_stats)]
        L.szhip_compress_omp_batch_view.restype = ctypes.c_int
        L.szhip_decompress_omp_batch_view.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(szhip_batch_item), ctypes.c_int, ctypes.c_int, sz, sz, sz, ctypes.c_int,
                                                      sz, sz, ctypes.POINTER(szhip_stats)]
        L.szhip_decompress_omp_batch_view.restype = ctypes.c_int
        L.szhip_minmax_batch_view.argtypes = [ctypes.c_void_p, ctypes.c_int, vpp, ctypes.c_int, ctypes.c_int, sz, sz, sz, sz, sz, dp, dp, ctypes.POINTER(szhip_stats)]
        L.szhip_minmax_batch_view.restype = ctypes.c_int
        L.szhip_compare_batch_view.argtypes = [ctypes.c_void_p, ctypes.c_int, vpp, sz, sz, vpp, sz, sz, ctypes.c_int, ctypes.c_int, sz, sz, sz, dp, dp, ctypes.c_uint,
                                               ctypes.POINTER(szhip_quality), ctypes.POINTER(szhip_stats)]
        L.szhip_compare_batch_view.restype = ctypes.c_int
    if hasattr(L, "SZ_hip_compress_args_batch_region"):
        vpp, dp, szp = ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(sz)
        L.SZ_hip_compress_args_batch_region.argtypes = [ctypes.c_int, ctypes.c_int, vpp, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double, sz, sz, sz, szp, szp,
                                                        vpp, szp, ctypes.POINTER(ctypes.c_int)]
        L.SZ_hip_compress_args_batch_region.restype = ctypes.c_int
        L.SZ_hip_decompress_batch_into_region.argtypes = [ctypes.c_int, ctypes.c_int, vpp, szp, vpp, ctypes.c_int, sz, sz, sz, szp, szp]
        L.SZ_hip_decompress_batch_into_region.restype = ctypes.c_int
        L.SZ_hip_compare_batch_region.argtypes = [ctypes.c_int, ctypes.c_int, vpp, vpp, ctypes.c_int, sz, sz, sz, szp, szp, dp, dp, ctypes.c_int, ctypes.POINTER(szhip_quality)]
        L.SZ_hip_compare_batch_region.restype = ctypes.c_int
    if hasattr(L, "SZ_hip_compress_args_batch"):
        vpp, dp = ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_double)
        L.SZ_hip_compress_args_batch.argtypes = [ctypes.c_int, ctypes.c_int, vpp, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double, sz, sz, sz,
                                                 vpp, ctypes.POINTER(sz), ctypes.POINTER(ctypes.c_int)]
        L.SZ_hip_compress_args_batch.restype = ctypes.c_int
        L.SZ_hip_decompress_batch.argtypes = [ctypes.c_int, ctypes.c_int, vpp, ctypes.POINTER(sz), vpp, ctypes.c_int, sz, sz, sz]
        L.SZ_hip_decompress_batch.restype = ctypes.c_int
        L.SZ_hip_compare_batch.argtypes = [ctypes.c_int, ctypes.c_int, vpp, vpp, ctypes.c_int, sz, sz, sz, dp, dp, ctypes.c_int, ctypes.POINTER(szhip_quality)]
        L.SZ_hip_compare_batch.restype = ctypes.c_int
    L.szhost_write_meta.argtypes = [ctypes.POINTER(szhost_meta), ctypes.c_ubyte, ctypes.c_char_p]
    L.szhost_write_meta.restype = sz
    L.free.argtypes = [ctypes.c_void_p]
    return L


def _dims5(shape):
    """numpy shape (slowest..fastest) -> (r5, r4, r3, r2, r1), r1 fastest, unused = 0 (reference convention)."""
    d = list(shape)[::-1] + [0] * (5 - len(shape))
    return d[4], d[3], d[2], d[1], d[0]


def _dtype_code(a):
    if a.dtype == np.float32:
        return SZ_FLOAT
    if a.dtype == np.float64:
        return SZ_DOUBLE
    raise SZError("only float32 / float64 arrays")


def SZ_Init(config_path=None):
    return lib().SZ_Init(config_path.encode() if config_path else None)


def SZ_Init_Params(params):
    return lib().SZ_Init_Params(ctypes.byref(params))


def SZ_Finalize():
    lib().SZ_Finalize()


def conf_params():
    """The live `confparams_cpr` struct (callers of the reference poke it directly)."""
    p = ctypes.POINTER(sz_params).in_dll(lib(), "confparams_cpr")
    if not p:
        raise SZError("SZ_Init has not been called")
    return p.contents


def SZ_compress_args(data, errBoundMode, absErrBound=0.0, relBoundRatio=0.0, pwrBoundRatio=0.0):
    """SZ_compress_args(dataType, data, &outSize, mode, abs, rel, pwr, r5..r1); returns the stream as bytes."""
    a = np.ascontiguousarray(data)
    n = ctypes.c_size_t(0)
    p = lib().SZ_compress_args(_dtype_code(a), a.ctypes.data, ctypes.byref(n), errBoundMode, absErrBound, relBoundRatio,
                               pwrBoundRatio, *_dims5(a.shape))
    if not p:
        raise SZError("SZ_compress_args returned NULL")
    out = ctypes.string_at(p, n.value)
    lib().free(p)
    return out


def SZ_compress(data):
    a = np.ascontiguousarray(data)
    n = ctypes.c_size_t(0)
    p = lib().SZ_compress(_dtype_code(a), a.ctypes.data, ctypes.byref(n), *_dims5(a.shape))
    if not p:
        raise SZError("SZ_compress returned NULL")
    out = ctypes.string_at(p, n.value)
    lib().free(p)
    return out


def SZ_decompress(stream, shape, dtype):
    dt = SZ_FLOAT if np.dtype(dtype) == np.float32 else SZ_DOUBLE
    buf = ctypes.create_string_buffer(bytes(stream), len(stream))
    p = lib().SZ_decompress(dt, buf, len(stream), *_dims5(shape))
    if not p:
        raise SZError("SZ_decompress returned NULL")
    n = int(np.prod(shape))
    ct = ctypes.c_float if dt == SZ_FLOAT else ctypes.c_double
    arr = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ct)), shape=(n,)).copy().reshape(shape)
    lib().free(p)
    return arr


def _take(p, shape, dt):
    """a malloc'd array of the library as a numpy array of its own; the library's memory is freed"""
    ct = ctypes.c_float if dt == SZ_FLOAT else ctypes.c_double
    arr = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ct)), shape=(int(np.prod(shape)),)).copy().reshape(shape)
    lib().free(p)
    return arr


def _box(lo, hi):
    return (ctypes.c_size_t * 3)(*[int(v) for v in lo]), (ctypes.c_size_t * 3)(*[int(v) for v in hi])


def SZ_hip_decompress_region(stream, shape, dtype, lo, hi):
    """The sub-box [lo, hi) (per dimension, slowest first, hi exclusive) of a 3-D array out of the stream SZ_compress_args wrote for it under SZ_HIP_MODE=omp
    (include/sz.h): only the boxes of the OpenMP container that meet the region are decoded.  Any other stream raises."""
    dt = SZ_FLOAT if np.dtype(dtype) == np.float32 else SZ_DOUBLE
    buf = ctypes.create_string_buffer(bytes(stream), len(stream))
    c_lo, c_hi = _box(lo, hi)
    p = lib().SZ_hip_decompress_region(dt, buf, len(stream), *_dims5(shape), c_lo, c_hi)
    if not p:
        raise SZError("SZ_hip_decompress_region returned NULL")
    return _take(p, tuple(int(h) - int(l) for l, h in zip(lo, hi)), dt)


def _parent3(parent):
    if not (isinstance(parent, np.ndarray) and parent.flags["C_CONTIGUOUS"]):
        raise SZError("the parent must be a C-contiguous numpy array (it is read / written where it lies)")
    return _dtype_code(parent)


def SZ_hip_compress_region(parent, lo, hi, errBoundMode, absErrBound=0.0, relBoundRatio=0.0, pwrBoundRatio=0.0):
    """The sub-box [lo, hi) of a 3-D host array compressed where it lies (include/sz.h): the bytes SZ_compress_args returns for np.ascontiguousarray(parent[lo:hi])."""
    dt = _parent3(parent)
    n = ctypes.c_size_t(0)
    c_lo, c_hi = _box(lo, hi)
    p = lib().SZ_hip_compress_region(dt, parent.ctypes.data, ctypes.byref(n), errBoundMode, absErrBound, relBoundRatio, pwrBoundRatio, *_dims5(parent.shape), c_lo, c_hi)
    if not p:
        raise SZError("SZ_hip_compress_region returned NULL")
    out = ctypes.string_at(p, n.value)
    lib().free(p)
    return out


def SZ_hip_decompress_into_region(stream, parent, lo, hi):
    """A stream of the extents hi - lo decoded into the sub-box [lo, hi) of a 3-D host array (include/sz.h); nothing else of the parent is written."""
    dt = _parent3(parent)
    buf = ctypes.create_string_buffer(bytes(stream), len(stream))
    c_lo, c_hi = _box(lo, hi)
    if lib().SZ_hip_decompress_into_region(dt, buf, len(stream), parent.ctypes.data, *_dims5(parent.shape), c_lo, c_hi) != SZ_SCES:
        raise SZError("SZ_hip_decompress_into_region failed")


def SZ_hip_compress_device(ptr, shape, dtype, errBoundMode, absErrBound=0.0, relBoundRatio=0.0, pwrBoundRatio=0.0):
    """SZ_compress_args for the array of `shape` / `dtype` at the DEVICE address ptr (include/sz.h): the stream as bytes, byte for byte what SZ_compress_args returns
    for a host copy of the array.  The array is never copied to the host."""
    dt = SZ_FLOAT if np.dtype(dtype) == np.float32 else SZ_DOUBLE
    n = ctypes.c_size_t(0)
    p = lib().SZ_hip_compress_device(dt, ptr, ctypes.byref(n), errBoundMode, absErrBound, relBoundRatio, pwrBoundRatio, *_dims5(shape))
    if not p:
        raise SZError("SZ_hip_compress_device returned NULL")
    out = ctypes.string_at(p, n.value)
    lib().free(p)
    return out


def SZ_hip_compress_device_into(ptr, shape, dtype, out_ptr, cap, errBoundMode, absErrBound=0.0, relBoundRatio=0.0, pwrBoundRatio=0.0):
    """The same stream into the caller's DEVICE buffer of `cap` bytes at out_ptr (any alignment); returns its length.  Raises when the library refuses: a capacity
    below the stream's length, or a configuration whose szMode is not SZ_BEST_SPEED (the reason is printed by the library)."""
    dt = SZ_FLOAT if np.dtype(dtype) == np.float32 else SZ_DOUBLE
    n = ctypes.c_size_t(0)
    rc = lib().SZ_hip_compress_device_into(dt, ptr, out_ptr, cap, ctypes.byref(n), errBoundMode, absErrBound, relBoundRatio, pwrBoundRatio, *_dims5(shape))
    if rc != SZ_SCES:
        raise SZError(f"SZ_hip_compress_device_into failed ({rc})")
    return n.value


def SZ_hip_decompress_device(stream_or_ptr, on_device, length, out_ptr, shape, dtype):
    """SZ_decompress into the DEVICE array at out_ptr (include/sz.h).  The stream: a bytes object (on_device = False) or a device address (on_device = True) of
    `length` bytes.  Exactly prod(shape) values are written."""
    dt = SZ_FLOAT if np.dtype(dtype) == np.float32 else SZ_DOUBLE
    if on_device:
        src = stream_or_ptr
    else:
        keep = ctypes.create_string_buffer(bytes(stream_or_ptr), length)
        src = ctypes.addressof(keep)
    rc = lib().SZ_hip_decompress_device(dt, src, 1 if on_device else 0, length, out_ptr, *_dims5(shape))
    if rc != SZ_SCES:
        raise SZError(f"SZ_hip_decompress_device failed ({rc})")


def SZ_hip_compare(ori, dec, absBound=-1.0, pwRelBound=-1.0, corr=False):
    """include/sz.h: the numpy array `ori` against its decoded copy `dec` (same shape and dtype), compared on the device: a Quality."""
    ori, dec = np.ascontiguousarray(ori), np.ascontiguousarray(dec)
    if ori.shape != dec.shape or ori.dtype != dec.dtype:
        raise SZError("SZ_hip_compare: two arrays of one shape and dtype")
    q = szhip_quality()
    if lib().SZ_hip_compare(_dtype_code(ori), ori.ctypes.data, dec.ctypes.data, *_dims5(ori.shape), absBound, pwRelBound, SZHIP_Q_CORR if corr else 0, ctypes.byref(q)) != SZ_SCES:
        raise SZError("SZ_hip_compare failed")
    return _quality(q)


def SZ_hip_compare_device(ori_ptr, dec_ptr, shape, dtype, absBound=-1.0, pwRelBound=-1.0, corr=False):
    """include/sz.h: the same for two arrays of `shape` / `dtype` at DEVICE addresses; neither is copied to the host."""
    dt = SZ_FLOAT if np.dtype(dtype) == np.float32 else SZ_DOUBLE
    q = szhip_quality()
    if lib().SZ_hip_compare_device(dt, ori_ptr, dec_ptr, *_dims5(shape), absBound, pwRelBound, SZHIP_Q_CORR if corr else 0, ctypes.byref(q)) != SZ_SCES:
        raise SZError("SZ_hip_compare_device failed")
    return _quality(q)


def SZ_hip_print_quality(q, cmp_bytes=0, is_double=False):
    """include/sz.h: the lines of the reference's `-a` report for a Quality, on the process's stdout."""
    lib().SZ_hip_print_quality(ctypes.byref(szhip_quality.from_buffer_copy(q.raw)), cmp_bytes, int(is_double))


def SZ_hip_compress_openmp_batch(ptrs, on_device, shape, dtype, bounds):
    """include/sz.h: `len(ptrs)` arrays of one 3-D `shape` / `dtype` at the addresses ptrs (host, or device with on_device) into OpenMP-container streams, array i with
    the absolute bound bounds[i]: a list of bytes objects, stream i byte for byte what SZ_compress_{float,double}_3D_MDQ_openmp returns for array i."""
    dt = SZ_FLOAT if np.dtype(dtype) == np.float32 else SZ_DOUBLE
    count = len(ptrs)
    c_ptrs = (ctypes.c_void_p * count)(*ptrs)
    c_eb = (ctypes.c_double * count)(*bounds)
    streams, sizes = (ctypes.c_void_p * count)(), (ctypes.c_size_t * count)()
    rc = lib().SZ_hip_compress_openmp_batch(dt, count, c_ptrs, 1 if on_device else 0, c_eb, shape[0], shape[1], shape[2], streams, sizes)
    if rc != SZ_SCES:
        raise SZError(f"SZ_hip_compress_openmp_batch failed ({rc})")
    out = [ctypes.string_at(streams[i], sizes[i]) for i in range(count)]
    for i in range(count):
        lib().free(streams[i])
    return out


def SZ_hip_decompress_openmp_batch(streams, out_ptrs, out_on_device, shape, dtype):
    """include/sz.h: the inverse -- streams[i] (bytes, as returned: the parameter bytes in front) into the array at out_ptrs[i] (host, or device with out_on_device)."""
    dt = SZ_FLOAT if np.dtype(dtype) == np.float32 else SZ_DOUBLE
    count = len(streams)
    keep = [ctypes.create_string_buffer(bytes(s), len(s)) for s in streams]
    c_streams = (ctypes.c_void_p * count)(*[ctypes.addressof(k) for k in keep])
    c_sizes = (ctypes.c_size_t * count)(*[len(s) for s in streams])
    c_out = (ctypes.c_void_p * count)(*out_ptrs)
    rc = lib().SZ_hip_decompress_openmp_batch(dt, count, c_streams, c_sizes, c_out, 1 if out_on_device else 0, shape[0], shape[1], shape[2])
    if rc != SZ_SCES:
        raise SZError(f"SZ_hip_decompress_openmp_batch failed ({rc})")


def SZ_hip_compress_args_batch(ptrs, on_device, shape, dtype, errBoundMode, absErrBound=0.0, relBoundRatio=0.0, raise_on_error=True):
    """include/sz.h: SZ_compress_args over `len(ptrs)` arrays of one 3-D `shape` / `dtype` at the addresses ptrs (host, or device with on_device) in one call.
    Returns (rc, streams, batched): stream i (bytes, or None when the item failed) is byte for byte what SZ_compress_args returns for array i alone under
    SZ_HIP_MODE=omp; batched[i] is 1 for the items that went through the shared launches."""
    dt = SZ_FLOAT if np.dtype(dtype) == np.float32 else SZ_DOUBLE
    count = len(ptrs)
    c_ptrs = (ctypes.c_void_p * max(count, 1))(*ptrs)
    streams, sizes, batched = (ctypes.c_void_p * max(count, 1))(), (ctypes.c_size_t * max(count, 1))(), (ctypes.c_int * max(count, 1))()
    rc = lib().SZ_hip_compress_args_batch(dt, count, c_ptrs, 1 if on_device else 0, errBoundMode, absErrBound, relBoundRatio, shape[0], shape[1], shape[2],
                                          streams, sizes, batched)
    out = [ctypes.string_at(streams[i], sizes[i]) if streams[i] else None for i in range(count)]
    for i in range(count):
        if streams[i]:
            lib().free(streams[i])
    if rc != SZ_SCES and raise_on_error:
        raise SZError(f"SZ_hip_compress_args_batch failed ({rc})")
    return rc, out, [batched[i] for i in range(count)]


def SZ_hip_decompress_batch(streams, out_ptrs, out_on_device, shape, dtype, raise_on_error=True):
    """include/sz.h: streams[i] (bytes, as SZ_hip_compress_args_batch or SZ_compress_args returned it) into the array at out_ptrs[i] (host, or device with
    out_on_device), bit for bit what SZ_decompress returns for it.  Returns rc: SZ_NSCS when any item failed (the others are decoded)."""
    dt = SZ_FLOAT if np.dtype(dtype) == np.float32 else SZ_DOUBLE
    count = len(streams)
    keep = [ctypes.create_string_buffer(bytes(s), len(s)) for s in streams]
    c_streams = (ctypes.c_void_p * max(count, 1))(*[ctypes.addressof(k) for k in keep])
    c_sizes = (ctypes.c_size_t * max(count, 1))(*[len(s) for s in streams])
    c_out = (ctypes.c_void_p * max(count, 1))(*out_ptrs)
    rc = lib().SZ_hip_decompress_batch(dt, count, c_streams, c_sizes, c_out, 1 if out_on_device else 0, shape[0], shape[1], shape[2])
    if rc != SZ_SCES and raise_on_error:
        raise SZError(f"SZ_hip_decompress_batch failed ({rc})")
    return rc


def SZ_hip_compress_args_batch_shapes(ptrs, on_device, shapes, dtype, errBoundMode, absErrBound=0.0, relBoundRatio=0.0, raise_on_error=True):
    """include/sz.h: SZ_hip_compress_args_batch over arrays of DIFFERENT 3-D shapes, shapes[i] = (r1, r2, r3) of array i, r1 slowest.  Returns (rc, streams, batched)."""
    dt = SZ_FLOAT if np.dtype(dtype) == np.float32 else SZ_DOUBLE
    count = len(ptrs)
    c_ptrs = (ctypes.c_void_p * max(count, 1))(*ptrs)
    c_dims = (ctypes.c_size_t * max(3 * count, 3))(*[int(v) for s in shapes for v in s])
    streams, sizes, batched = (ctypes.c_void_p * max(count, 1))(), (ctypes.c_size_t * max(count, 1))(), (ctypes.c_int * max(count, 1))()
    rc = lib().SZ_hip_compress_args_batch_shapes(dt, count, c_ptrs, 1 if on_device else 0, errBoundMode, absErrBound, relBoundRatio, c_dims, streams, sizes, batched)
    out = [ctypes.string_at(streams[i], sizes[i]) if streams[i] else None for i in range(count)]
    for i in range(count):
        if streams[i]:
            lib().free(streams[i])
    if rc != SZ_SCES and raise_on_error:
        raise SZError(f"SZ_hip_compress_args_batch_shapes failed ({rc})")
    return rc, out, [batched[i] for i in range(count)]


def SZ_hip_decompress_batch_shapes(streams, out_ptrs, out_on_device, shapes, dtype, raise_on_error=True):
    """include/sz.h: SZ_hip_decompress_batch with the extents per item, shapes[i] = (r1, r2, r3).  Returns rc: SZ_NSCS when any item failed (the others are decoded)."""
    dt = SZ_FLOAT if np.dtype(dtype) == np.float32 else SZ_DOUBLE
    count = len(streams)
    keep = [ctypes.create_string_buffer(bytes(s), len(s)) for s in streams]
    c_streams = (ctypes.c_void_p * max(count, 1))(*[ctypes.addressof(k) for k in keep])
    c_sizes = (ctypes.c_size_t * max(count, 1))(*[len(s) for s in streams])
    c_out = (ctypes.c_void_p * max(count, 1))(*out_ptrs)
    c_dims = (ctypes.c_size_t * max(3 * count, 3))(*[int(v) for s in shapes for v in s])
    rc = lib().SZ_hip_decompress_batch_shapes(dt, count, c_streams, c_sizes, c_out, 1 if out_on_device else 0, c_dims)
    if rc != SZ_SCES and raise_on_error:
        raise SZError(f"SZ_hip_decompress_batch_shapes failed ({rc})")
    return rc


def SZ_hip_decompress_batch_regions(streams, shapes, los, his, out_ptrs, out_on_device, dtype, pitches=None, raise_on_error=True):
    """include/sz.h: the sub-box [los[i], his[i]) of the array of shapes[i] = (r1, r2, r3) in streams[i] (bytes; the SAME bytes object given twice is one stream) into
    out_ptrs[i] (host, or device with out_on_device); pitches: None (contiguous destinations) or pitches[i] = (pitch0, pitch1) in elements.  Returns rc: SZ_NSCS when
    any item failed (the others are delivered)."""
    dt = SZ_FLOAT if np.dtype(dtype) == np.float32 else SZ_DOUBLE
    count = len(streams)
    keep = {}
    for s in streams:
        if id(s) not in keep:
            keep[id(s)] = ctypes.create_string_buffer(bytes(s), len(s))
    c_streams = (ctypes.c_void_p * max(count, 1))(*[ctypes.addressof(keep[id(s)]) for s in streams])
    c_sizes = (ctypes.c_size_t * max(count, 1))(*[len(s) for s in streams])
    c_out = (ctypes.c_void_p * max(count, 1))(*out_ptrs)
    flat = lambda rows, k: (ctypes.c_size_t * max(k * count, k))(*[int(v) for r in rows for v in r])
    c_pitches = flat(pitches, 2) if pitches is not None else None
    rc = lib().SZ_hip_decompress_batch_regions(dt, count, c_streams, c_sizes, flat(shapes, 3), flat(los, 3), flat(his, 3), c_out, 1 if out_on_device else 0, c_pitches)
    if rc != SZ_SCES and raise_on_error:
        raise SZError(f"SZ_hip_decompress_batch_regions failed ({rc})")
    return rc


def SZ_hip_compare_batch(ori_ptrs, dec_ptrs, on_device, shape, dtype, absBounds, pwRelBounds=None, corr=False):
    """include/sz.h: `len(ori_ptrs)` pairs of arrays of `shape` / `dtype` (host, or device with on_device), pair i against absBounds[i] (and pwRelBounds[i]): a list
    of Quality, record i byte for byte SZ_hip_compare's for pair i."""
    dt = SZ_FLOAT if np.dtype(dtype) == np.float32 else SZ_DOUBLE
    count = len(ori_ptrs)
    c_ori, c_dec = (ctypes.c_void_p * max(count, 1))(*ori_ptrs), (ctypes.c_void_p * max(count, 1))(*dec_ptrs)
    c_abs = (ctypes.c_double * max(count, 1))(*[float(b) for b in absBounds])
    c_pwr = (ctypes.c_double * max(count, 1))(*[float(b) for b in pwRelBounds]) if pwRelBounds is not None else None
    out = (szhip_quality * max(count, 1))()
    if lib().SZ_hip_compare_batch(dt, count, c_ori, c_dec, 1 if on_device else 0, shape[0], shape[1], shape[2], c_abs, c_pwr, SZHIP_Q_CORR if corr else 0, out) != SZ_SCES:
        raise SZError("SZ_hip_compare_batch failed")
    return [_quality(out[i]) for i in range(count)]


def _box3(lo, hi):
    return (ctypes.c_size_t * 3)(*[int(v) for v in lo]), (ctypes.c_size_t * 3)(*[int(v) for v in hi])


def SZ_hip_compress_args_batch_region(parent_ptrs, on_device, parent_shape, dtype, lo, hi, errBoundMode, absErrBound=0.0, relBoundRatio=0.0, raise_on_error=True):
    """include/sz.h: SZ_hip_compress_args_batch on the box [lo, hi) common to `len(parent_ptrs)` 3-D parents of `parent_shape` / `dtype` (patches with ghost layers;
    the pointers are the parents' first values).  Returns (rc, streams, batched): stream i is byte for byte that of a contiguous copy of sub-box i."""
    dt = SZ_FLOAT if np.dtype(dtype) == np.float32 else SZ_DOUBLE
    count = len(parent_ptrs)
    c_ptrs = (ctypes.c_void_p * max(count, 1))(*parent_ptrs)
    c_lo, c_hi = _box3(lo, hi)
    streams, sizes, batched = (ctypes.c_void_p * max(count, 1))(), (ctypes.c_size_t * max(count, 1))(), (ctypes.c_int * max(count, 1))()
    rc = lib().SZ_hip_compress_args_batch_region(dt, count, c_ptrs, 1 if on_device else 0, errBoundMode, absErrBound, relBoundRatio, parent_shape[0], parent_shape[1],
                                                 parent_shape[2], c_lo, c_hi, streams, sizes, batched)
    out = [ctypes.string_at(streams[i], sizes[i]) if streams[i] else None for i in range(count)]
    for i in range(count):
        if streams[i]:
            lib().free(streams[i])
    if rc != SZ_SCES and raise_on_error:
        raise SZError(f"SZ_hip_compress_args_batch_region failed ({rc})")
    return rc, out, [batched[i] for i in range(count)]


def SZ_hip_decompress_batch_into_region(streams, parent_ptrs, out_on_device, parent_shape, dtype, lo, hi, raise_on_error=True):
    """include/sz.h: streams[i] into the box [lo, hi) of the parent at parent_ptrs[i] (host, or device with out_on_device); no other byte of a parent is written.
    Returns rc: SZ_NSCS when any item failed (the others are decoded)."""
    dt = SZ_FLOAT if np.dtype(dtype) == np.float32 else SZ_DOUBLE
    count = len(streams)
    keep = [ctypes.create_string_buffer(bytes(s), len(s)) for s in streams]
    c_streams = (ctypes.c_void_p * max(count, 1))(*[ctypes.addressof(k) for k in keep])
    c_sizes = (ctypes.c_size_t * max(count, 1))(*[len(s) for s in streams])
    c_out = (ctypes.c_void_p * max(count, 1))(*parent_ptrs)
    c_lo, c_hi = _box3(lo, hi)
    rc = lib().SZ_hip_decompress_batch_into_region(dt, count, c_streams, c_sizes, c_out, 1 if out_on_device else 0, parent_shape[0], parent_shape[1], parent_shape[2],
                                                   c_lo, c_hi)
    if rc != SZ_SCES and raise_on_error:
        raise SZError(f"SZ_hip_decompress_batch_into_region failed ({rc})")
    return rc


def SZ_hip_compare_batch_region(ori_parent_ptrs, dec_parent_ptrs, on_device, parent_shape, dtype, lo, hi, absBounds, pwRelBounds=None, corr=False):
    """include/sz.h: the boxes [lo, hi) of `len(ori_parent_ptrs)` pairs of parents against each other, pair i against absBounds[i] (and pwRelBounds[i]): a list of
    Quality, record i byte for byte SZ_hip_compare's for contiguous copies of pair i."""
    dt = SZ_FLOAT if np.dtype(dtype) == np.float32 else SZ_DOUBLE
    count = len(ori_parent_ptrs)
    c_ori, c_dec = (ctypes.c_void_p * max(count, 1))(*ori_parent_ptrs), (ctypes.c_void_p * max(count, 1))(*dec_parent_ptrs)
    c_abs = (ctypes.c_double * max(count, 1))(*[float(b) for b in absBounds])
    c_pwr = (ctypes.c_double * max(count, 1))(*[float(b) for b in pwRelBounds]) if pwRelBounds is not None else None
    c_lo, c_hi = _box3(lo, hi)
    out = (szhip_quality * max(count, 1))()
    if lib().SZ_hip_compare_batch_region(dt, count, c_ori, c_dec, 1 if on_device else 0, parent_shape[0], parent_shape[1], parent_shape[2], c_lo, c_hi, c_abs, c_pwr,
                                         SZHIP_Q_CORR if corr else 0, out) != SZ_SCES:
        raise SZError("SZ_hip_compare_batch_region failed")
    return [_quality(out[i]) for i in range(count)]


def sz_slab_compress(data, slabs, errBoundMode, absErrBound=0.0, relBoundRatio=0.0, pwrBoundRatio=0.0):
    """include/sz_slab.h: a 3-D array as `slabs` slabs in one container (bytes)."""
    a = np.ascontiguousarray(data)
    n = ctypes.c_size_t(0)
    p = lib().sz_slab_compress(_dtype_code(a), a.ctypes.data, ctypes.byref(n), errBoundMode, absErrBound, relBoundRatio, pwrBoundRatio, *a.shape, slabs)
    if not p:
        raise SZError("sz_slab_compress returned NULL")
    out = ctypes.string_at(p, n.value)
    lib().free(p)
    return out


def sz_slab_decompress(blob):
    """include/sz_slab.h: the whole array of a slab container."""
    dt, dims = ctypes.c_int(0), (ctypes.c_size_t * 3)()
    p = lib().sz_slab_decompress(bytes(blob), len(blob), ctypes.byref(dt), ctypes.byref(dims))
    if not p:
        raise SZError("sz_slab_decompress returned NULL")
    return _take(p, tuple(dims), dt.value)


def sz_slab_decompress_region(blob, lo, hi):
    """include/sz_slab_region.h (part of sz_slab.h): the sub-box [lo, hi) of a slab container's array; only the slabs that meet it are touched, and of a slab that is an OpenMP container only
    the boxes that do."""
    dt = ctypes.c_int(0)
    c_lo, c_hi = _box(lo, hi)
    p = lib().sz_slab_decompress_region(bytes(blob), len(blob), c_lo, c_hi, ctypes.byref(dt))
    if not p:
        raise SZError("sz_slab_decompress_region returned NULL")
    return _take(p, tuple(int(h) - int(l) for l, h in zip(lo, hi)), dt.value)


def SZ_hip_last_stats():
    s = szhip_stats()
    lib().SZ_hip_last_stats(ctypes.byref(s))
    return s


def make_meta(dtype, err_mode=ABS, abs_bound=0.0, rel_ratio=0.0, vmin=0.0, vmax=0.0, sz_mode=SZ_BEST_SPEED, gzip_mode=1,
              sample_distance=100, pred_threshold=0.99, max_quant_intervals=65536, quantization_intervals=0,
              protect_value_range=0):
    """Version + flag + parameter bytes an SZ 2.1 regression-type stream starts with (szhost_write_meta)."""
    m = szhost_meta()
    m.data_type = SZ_FLOAT if np.dtype(dtype) == np.float32 else SZ_DOUBLE
    m.err_mode, m.abs_bound, m.rel_ratio, m.psnr = err_mode, abs_bound, rel_ratio, 0.0
    m.vmin, m.vmax = vmin, vmax
    m.opt_quant_mode = 1 if quantization_intervals == 0 else 0
    m.data_endian, m.sz_mode, m.gzip_mode = 0, sz_mode, gzip_mode
    m.sample_distance, m.pred_threshold, m.sol_id = sample_distance, pred_threshold, 101
    m.max_quant_intervals, m.quantization_intervals, m.protect_value_range = max_quant_intervals, quantization_intervals, protect_value_range
    buf = ctypes.create_string_buffer(64)
    flags = 0x80 | 0x40 | (0x04 if protect_value_range else 0)
    n = lib().szhost_write_meta(ctypes.byref(m), flags, buf)
    return buf.raw[:n]


def sz14_range(vmin, vmax, dtype):
    """(value_range, median) as szhip_compress_sz14 takes them: max - min and min + range / 2, both computed in the data's type
    (include/szhip.h; the reference's range scan, dataCompression.c:102-119)."""
    T = np.dtype(dtype).type
    lo, hi = T(vmin), T(vmax)
    rng = T(hi - lo)
    return float(rng), float(T(lo + T(rng / T(2))))


BOOK_CAP = 1024                      # distinct symbols k_huff_book's heap holds (SZH_BOOK_CAP, sz_amd/csrc/szh_book.h)


def szhip_huff_book_tree_cap():
    """Bytes of the largest tree szhip_huff_book serialises (two-byte node indices)."""
    return 1 + 9 * (2 * BOOK_CAP - 1)


def parse_book_record(raw):
    """The 32 bytes of a szhip_book_record as a dict (the layout the library copies from the device)."""
    rec = szhip_book_record.from_buffer_copy(bytes(raw)[:ctypes.sizeof(szhip_book_record)])
    return {k: getattr(rec, k) for k, _ in rec._fields_}


class HipPool:
    """szhip_pool (include/szhip.h): `lanes` contexts and host threads on one GPU; submit() queues one szhip_compress call and returns
    a ticket, wait() blocks for it.  The arguments of a call (input, parameter bytes, output buffer) must stay alive until its wait()."""

    def __init__(self, device=0, lanes=2):
        self._h = ctypes.c_void_p()
        self.lanes = lanes
        rc = lib().szhip_pool_create(ctypes.byref(self._h), device, lanes)
        if rc != 0:
            raise SZError(f"szhip_pool_create failed ({rc})")
        self._keep = {}

    def close(self):
        if self._h:
            lib().szhip_pool_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def submit(self, ptr, on_device, shape3, dtype, eb, meta, params, out_ptr, out_cap):
        """Stream into the caller's device buffer (out_ptr, out_cap).  Returns the ticket."""
        t = ctypes.c_int(-1)
        p = params or szhip_params(100, 0.99, 65536, 0)
        rc = lib().szhip_pool_submit(self._h, 0 if np.dtype(dtype) == np.float32 else 1, ptr, int(on_device), shape3[0], shape3[1], shape3[2], eb,
                                     ctypes.byref(p), meta, len(meta), 2, out_ptr, out_cap, ctypes.byref(t))
        if rc != 0:
            raise SZError(f"szhip_pool_submit failed ({rc})")
        self._keep[t.value] = (p, meta)
        return t.value

    def wait(self, ticket):
        """Returns (size, stats); raises if the call failed.  SZHIP_CONSTANT (1: the array lies within the bound of one value -- the caller
        writes the reference's constant stream, as SZ_compress_args does) is a result, not a failure: size 0, stats with the range."""
        out = ctypes.c_void_p(); n = ctypes.c_size_t(0); st = szhip_stats()
        rc = lib().szhip_pool_wait(self._h, ticket, ctypes.byref(out), ctypes.byref(n), ctypes.byref(st))
        self._keep.pop(ticket, None)
        if rc == 1:
            return 0, st
        if rc != 0:
            raise SZError(f"pooled szhip_compress failed ({rc})")
        return n.value, st


class HipContext:
    """Thin owner of one szhip_ctx (one HIP stream + device workspaces).  Device-resident entry points for bench.py."""

    def __init__(self, device=0):
        self._h = ctypes.c_void_p()
        rc = lib().szhip_create(ctypes.byref(self._h), device)
        if rc != 0:
            raise SZError(f"szhip_create failed ({rc}): no usable HIP device; there is no CPU fallback")

    def close(self):
        if self._h:
            lib().szhip_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _err(self, rc, what):
        raise SZError(f"{what} failed ({rc}): {lib().szhip_last_error(self._h).decode(errors='replace')}")

    def minmax(self, ptr, on_device, n, dtype):
        lo, hi = ctypes.c_double(), ctypes.c_double()
        rc = lib().szhip_minmax(self._h, 0 if np.dtype(dtype) == np.float32 else 1, ptr, int(on_device), n,
                                ctypes.byref(lo), ctypes.byref(hi))
        if rc:
            self._err(rc, "szhip_minmax")
        return lo.value, hi.value

    def compress(self, ptr, on_device, shape3, dtype, eb, meta, params=None, out_on_device=False, out_ptr=None, out_cap=0):
        """Returns (bytes | device pointer int, size, stats).  out_ptr / out_cap: the caller's device buffer and its capacity in bytes
        (out_on_device = 2 of include/szhip.h); the stream is written there and out_ptr comes back."""
        p = params or szhip_params(100, 0.99, 65536, 0)
        out = ctypes.c_void_p()
        n = ctypes.c_size_t(0)
        st = szhip_stats()
        if out_ptr is not None:
            out, n, out_on_device = ctypes.c_void_p(out_ptr), ctypes.c_size_t(out_cap), 2
        rc = lib().szhip_compress(self._h, 0 if np.dtype(dtype) == np.float32 else 1, ptr, int(on_device), shape3[0], shape3[1],
                                  shape3[2], eb, ctypes.byref(p), meta, len(meta), int(out_on_device), ctypes.byref(out),
                                  ctypes.byref(n), ctypes.byref(st))
        if rc == 1:                      # SZHIP_CONSTANT (range-from-data): nothing encoded, st.vmin / st.vmax say why
            return None, 0, st
        if rc:
            self._err(rc, "szhip_compress")
        if out_on_device:
            return out.value, n.value, st
        b = ctypes.string_at(out.value, n.value)
        lib().free(out)
        return b, n.value, st

    def compress_sz14(self, ptr, on_device, shape3, dtype, eb, value_range, median, meta, params=None, out_on_device=False, out_ptr=None, out_cap=0):
        """The SZ 1.4 container (szhip_compress_sz14).  shape3: (r0, r1, r2), r0 == 0 a 2-D array, r0 == r1 == 0 a 1-D array; value_range / median: see
        sz14_range.  Returns (bytes | device pointer int, size, stats)."""
        p = params or szhip_params(100, 0.99, 65536, 0)
        out = ctypes.c_void_p()
        n = ctypes.c_size_t(0)
        st = szhip_stats()
        if out_ptr is not None:
            out, n, out_on_device = ctypes.c_void_p(out_ptr), ctypes.c_size_t(out_cap), 2
        rc = lib().szhip_compress_sz14(self._h, 0 if np.dtype(dtype) == np.float32 else 1, ptr, int(on_device), shape3[0], shape3[1], shape3[2], eb,
                                       value_range, median, ctypes.byref(p), meta, len(meta), int(out_on_device), ctypes.byref(out), ctypes.byref(n),
                                       ctypes.byref(st))
        if rc:
            self._err(rc, "szhip_compress_sz14")
        if out_on_device:
            return out.value, n.value, st
        b = ctypes.string_at(out.value, n.value)
        lib().free(out)
        return b, n.value, st

    def decompress_sz14(self, stream_ptr, stream_on_device, stream_len, body_off, shape3, dtype, out_ptr, out_on_device):
        st = szhip_stats()
        rc = lib().szhip_decompress_sz14(self._h, 0 if np.dtype(dtype) == np.float32 else 1, stream_ptr, int(stream_on_device), stream_len,
                                         body_off, shape3[0], shape3[1], shape3[2], out_ptr, int(out_on_device), ctypes.byref(st))
        if rc:
            self._err(rc, "szhip_decompress_sz14")
        return st

    def compress_omp(self, ptr, on_device, shape3, dtype, eb, thread_num, meta, params=None, out_on_device=False):
        """The reference's OpenMP container (szhip_compress_omp; sz/src/sz_omp.c:63-358).  Returns (bytes | device pointer int, size, stats)."""
        p = params or szhip_params(100, 0.99, 65536, 0)
        out = ctypes.c_void_p()
        n = ctypes.c_size_t(0)
        st = szhip_stats()
        rc = lib().szhip_compress_omp(self._h, 0 if np.dtype(dtype) == np.float32 else 1, ptr, int(on_device), shape3[0], shape3[1], shape3[2],
                                      eb, thread_num, ctypes.byref(p), meta, len(meta), int(out_on_device), ctypes.byref(out), ctypes.byref(n),
                                      ctypes.byref(st))
        if rc:
            self._err(rc, "szhip_compress_omp")
        if out_on_device:
            return out.value, n.value, st
        b = ctypes.string_at(out.value, n.value)
        lib().free(out)
        return b, n.value, st

    def decompress_omp(self, stream_ptr, stream_on_device, stream_len, body_off, shape3, dtype, out_ptr, out_on_device):
        st = szhip_stats()
        rc = lib().szhip_decompress_omp(self._h, 0 if np.dtype(dtype) == np.float32 else 1, stream_ptr, int(stream_on_device), stream_len,
                                        body_off, shape3[0], shape3[1], shape3[2], out_ptr, int(out_on_device), ctypes.byref(st))
        if rc:
            self._err(rc, "szhip_decompress_omp")
        return st

    def compress_omp_batch(self, ptrs, on_device, shape3, dtype, bounds, thread_num, metas, params=None, out_on_device=False, raise_on_error=True):
        """szhip_compress_omp_batch: len(ptrs) arrays of one shape3 / dtype in one call, array i with the absolute bound bounds[i] and the parameter bytes metas[i] (all of
        one length).  Returns (rc, blob, blob_size, items, stats): blob a bytes object, or the context's device pointer with out_on_device; items[i].offset / .size place
        stream i in it, items[i].rc / .intervals / .n_unpred / .quant_kernel / .batched say how it went.  rc: the first non-zero items[i].rc."""
        count = len(ptrs)
        items = (szhip_batch_item * max(count, 1))()
        keep = [ctypes.create_string_buffer(bytes(m), len(m)) for m in metas]
        for i in range(count):
            items[i].data, items[i].eb, items[i].meta = ptrs[i], bounds[i], ctypes.addressof(keep[i]) if metas[i] is not None else None
        p = params or szhip_params(100, 0.99, 65536, 0)
        out, n, st = ctypes.c_void_p(), ctypes.c_size_t(0), szhip_stats()
        rc = lib().szhip_compress_omp_batch(self._h, 0 if np.dtype(dtype) == np.float32 else 1, items, count, int(on_device), shape3[0], shape3[1], shape3[2], thread_num,
                                            ctypes.byref(p), len(metas[0]) if count else 0, int(out_on_device), ctypes.byref(out), ctypes.byref(n), ctypes.byref(st))
        if rc and raise_on_error:
            self._err(rc, "szhip_compress_omp_batch")
        if out_on_device or not out.value:
            return rc, out.value, n.value, items, st
        b = ctypes.string_at(out.value, n.value)
        lib().free(out)
        return rc, b, n.value, items, st

    def decompress_omp_batch(self, streams, stream_on_device, body_off, shape3, dtype, out_ptrs, out_on_device, raise_on_error=True):
        """szhip_decompress_omp_batch: streams[i] = (address, length) of an OpenMP-container stream (host, or device with stream_on_device) into the array at out_ptrs[i].
        Returns (rc, items, stats); an item whose rc is non-zero failed alone."""
        count = len(streams)
        items = (szhip_batch_item * max(count, 1))()
        for i in range(count):
            items[i].stream, items[i].stream_len, items[i].body_off, items[i].out = streams[i][0], streams[i][1], body_off, out_ptrs[i]
        st = szhip_stats()
        rc = lib().szhip_decompress_omp_batch(self._h, 0 if np.dtype(dtype) == np.float32 else 1, items, count, int(stream_on_device), shape3[0], shape3[1], shape3[2],
                                              int(out_on_device), ctypes.byref(st))
        if rc and raise_on_error:
            self._err(rc, "szhip_decompress_omp_batch")
        return rc, items, st

    def compress_omp_batch_shapes(self, ptrs, on_device, shapes, dtype, bounds, metas, params=None, out_on_device=False, raise_on_error=True):
        """szhip_compress_omp_batch_shapes: compress_omp_batch on arrays of DIFFERENT shapes, shapes[i] = (r0, r1, r2, thread_num) of array i (None: a null table).
        Returns (rc, blob, blob_size, items, stats) as compress_omp_batch; stats.quant_kernel_launches grows with the kinds of item, not with their number."""
        count = len(ptrs)
        items = (szhip_batch_item * max(count, 1))()
        keep = [ctypes.create_string_buffer(bytes(m), len(m)) for m in metas]
        for i in range(count):
            items[i].data, items[i].eb, items[i].meta = ptrs[i], bounds[i], ctypes.addressof(keep[i]) if metas[i] is not None else None
        c_shapes = (szhip_batch_shape * max(count, 1))(*[szhip_batch_shape(*s) for s in shapes]) if shapes is not None else None
        p = params or szhip_params(100, 0.99, 65536, 0)
        out, n, st = ctypes.c_void_p(), ctypes.c_size_t(0), szhip_stats()
        rc = lib().szhip_compress_omp_batch_shapes(self._h, 0 if np.dtype(dtype) == np.float32 else 1, items, c_shapes, count, int(on_device), ctypes.byref(p),
                                                   len(metas[0]) if count else 0, int(out_on_device), ctypes.byref(out), ctypes.byref(n), ctypes.byref(st))
        if rc and raise_on_error:
            self._err(rc, "szhip_compress_omp_batch_shapes")
        if out_on_device or not out.value:
            return rc, out.value, n.value, items, st
        b = ctypes.string_at(out.value, n.value)
        lib().free(out)
        return rc, b, n.value, items, st

    def decompress_omp_batch_shapes(self, streams, stream_on_device, body_off, shapes, dtype, out_ptrs, out_on_device, raise_on_error=True):
        """szhip_decompress_omp_batch_shapes: streams[i] = (address, length) into the array of shapes[i] = (r0, r1, r2[, anything]) at out_ptrs[i]; the box count is read
        from each stream.  Returns (rc, items, stats); an item whose rc is non-zero failed alone."""
        count = len(streams)
        items = (szhip_batch_item * max(count, 1))()
        for i in range(count):
            items[i].stream, items[i].stream_len, items[i].body_off, items[i].out = streams[i][0], streams[i][1], body_off, out_ptrs[i]
        c_shapes = (szhip_batch_shape * max(count, 1))(*[szhip_batch_shape(s[0], s[1], s[2], 0) for s in shapes]) if shapes is not None else None
        st = szhip_stats()
        rc = lib().szhip_decompress_omp_batch_shapes(self._h, 0 if np.dtype(dtype) == np.float32 else 1, items, c_shapes, count, int(stream_on_device), int(out_on_device),
                                                     ctypes.byref(st))
        if rc and raise_on_error:
            self._err(rc, "szhip_decompress_omp_batch_shapes")
        return rc, items, st

    def decompress_omp_batch_region(self, streams, stream_on_device, body_off, shapes, dtype, regions, out_ptrs, out_on_device, raise_on_error=True):
        """szhip_decompress_omp_batch_region: the sub-box regions[i] = (lo, hi[, (pitch0, pitch1)]) of the array of shapes[i] = (r0, r1, r2) in streams[i] = (address,
        length) into out_ptrs[i]; pitches in elements, absent or (0, 0): a contiguous destination.  Items that name the same (address, length) share the stream's header
        work.  Returns (rc, items, regions, stats): regions[i].n_boxes the boxes decoded, regions[i].shares the first item of the same stream."""
        count = len(streams)
        items = (szhip_batch_item * max(count, 1))()
        for i in range(count):
            items[i].stream, items[i].stream_len, items[i].body_off, items[i].out = streams[i][0], streams[i][1], body_off, out_ptrs[i]
        c_shapes = (szhip_batch_shape * max(count, 1))(*[szhip_batch_shape(s[0], s[1], s[2], 0) for s in shapes]) if shapes is not None else None
        c_regions = None
        if regions is not None:
            c_regions = (szhip_batch_region * max(count, 1))()
            for i, r in enumerate(regions):
                c_regions[i].lo[:] = [int(v) for v in r[0]]
                c_regions[i].hi[:] = [int(v) for v in r[1]]
                c_regions[i].pitch0, c_regions[i].pitch1 = (int(r[2][0]), int(r[2][1])) if len(r) > 2 and r[2] is not None else (0, 0)
        st = szhip_stats()
        rc = lib().szhip_decompress_omp_batch_region(self._h, 0 if np.dtype(dtype) == np.float32 else 1, items, c_shapes, c_regions, count, int(stream_on_device),
                                                     int(out_on_device), ctypes.byref(st))
        if rc and raise_on_error:
            self._err(rc, "szhip_decompress_omp_batch_region")
        return rc, items, c_regions, st

    def compress_omp_batch_view(self, ptrs, on_device, shape3, pitches, dtype, bounds, thread_num, metas, params=None, out_on_device=False, raise_on_error=True):
        """szhip_compress_omp_batch_view: compress_omp_batch on len(ptrs) sub-boxes of shape3 values, ptrs[i] the first value of sub-box i inside its parent array,
        pitches = (pitch0, pitch1) in elements, common to all (patches with ghost layers).  Stream i is byte for byte that of a contiguous copy of sub-box i.
        Returns (rc, blob, blob_size, items, stats) as compress_omp_batch; stats.packing counts the gather launches (0 or 1)."""
        count = len(ptrs)
        items = (szhip_batch_item * max(count, 1))()
        keep = [ctypes.create_string_buffer(bytes(m), len(m)) for m in metas]
        for i in range(count):
            items[i].data, items[i].eb, items[i].meta = ptrs[i], bounds[i], ctypes.addressof(keep[i]) if metas[i] is not None else None
        p = params or szhip_params(100, 0.99, 65536, 0)
        out, n, st = ctypes.c_void_p(), ctypes.c_size_t(0), szhip_stats()
        rc = lib().szhip_compress_omp_batch_view(self._h, 0 if np.dtype(dtype) == np.float32 else 1, items, count, int(on_device), shape3[0], shape3[1], shape3[2],
                                                 int(pitches[0]), int(pitches[1]), thread_num, ctypes.byref(p), len(metas[0]) if count else 0, int(out_on_device),
                                                 ctypes.byref(out), ctypes.byref(n), ctypes.byref(st))
        if rc and raise_on_error:
            self._err(rc, "szhip_compress_omp_batch_view")
        if out_on_device or not out.value:
            return rc, out.value, n.value, items, st
        b = ctypes.string_at(out.value, n.value)
        lib().free(out)
        return rc, b, n.value, items, st

    def decompress_omp_batch_view(self, streams, stream_on_device, body_off, shape3, dtype, out_ptrs, out_on_device, pitches, raise_on_error=True):
        """szhip_decompress_omp_batch_view: decompress_omp_batch into len(streams) sub-boxes of shape3 values, out_ptrs[i] the first value of sub-box i inside its parent,
        pitches = (pitch0, pitch1) in elements, common to all; no other byte of a parent is written.  Returns (rc, items, stats)."""
        count = len(streams)
        items = (szhip_batch_item * max(count, 1))()
        for i in range(count):
            items[i].stream, items[i].stream_len, items[i].body_off, items[i].out = streams[i][0], streams[i][1], body_off, out_ptrs[i]
        st = szhip_stats()
        rc = lib().szhip_decompress_omp_batch_view(self._h, 0 if np.dtype(dtype) == np.float32 else 1, items, count, int(stream_on_device), shape3[0], shape3[1], shape3[2],
                                                   int(out_on_device), int(pitches[0]), int(pitches[1]), ctypes.byref(st))
        if rc and raise_on_error:
            self._err(rc, "szhip_decompress_omp_batch_view")
        return rc, items, st

    def minmax_batch_view(self, ptrs, on_device, shape3, pitches, dtype, raise_on_error=True):
        """szhip_minmax_batch_view: the value ranges of len(ptrs) sub-boxes of shape3 values (ptrs[i]: the first value; pitches = (pitch0, pitch1) in elements) in one
        launch.  Returns (rc, [(vmin, vmax), ...], stats); pair i is bit for bit minmax of a contiguous copy of sub-box i."""
        count = len(ptrs)
        c_ptrs = (ctypes.c_void_p * max(count, 1))(*ptrs)
        lo, hi, st = (ctypes.c_double * max(count, 1))(), (ctypes.c_double * max(count, 1))(), szhip_stats()
        rc = lib().szhip_minmax_batch_view(self._h, 0 if np.dtype(dtype) == np.float32 else 1, c_ptrs, count, int(on_device), shape3[0], shape3[1], shape3[2],
                                           int(pitches[0]), int(pitches[1]), lo, hi, ctypes.byref(st))
        if rc and raise_on_error:
            self._err(rc, "szhip_minmax_batch_view")
        return rc, [(lo[i], hi[i]) for i in range(count)], st

    def compare_batch_view(self, ori_ptrs, ori_pitches, dec_ptrs, dec_pitches, on_device, shape3, dtype, abs_bounds, pw_rel_bounds=None, corr=False, raise_on_error=True):
        """szhip_compare_batch_view: len(ori_ptrs) pairs of boxes of shape3 values, the originals with ori_pitches, the decoded ones with dec_pitches (each (pitch0,
        pitch1) in elements, common to the batch).  Returns (rc, [Quality, ...], stats); record i is byte for byte compare_view of pair i alone."""
        count = len(ori_ptrs)
        c_ori, c_dec = (ctypes.c_void_p * max(count, 1))(*ori_ptrs), (ctypes.c_void_p * max(count, 1))(*dec_ptrs)
        c_abs = (ctypes.c_double * max(count, 1))(*[float(b) for b in abs_bounds])
        c_pwr = (ctypes.c_double * max(count, 1))(*[float(b) for b in pw_rel_bounds]) if pw_rel_bounds is not None else None
        out, st = (szhip_quality * max(count, 1))(), szhip_stats()
        rc = lib().szhip_compare_batch_view(self._h, 0 if np.dtype(dtype) == np.float32 else 1, c_ori, int(ori_pitches[0]), int(ori_pitches[1]), c_dec,
                                            int(dec_pitches[0]), int(dec_pitches[1]), count, int(on_device), shape3[0], shape3[1], shape3[2], c_abs, c_pwr,
                                            SZHIP_Q_CORR if corr else 0, out, ctypes.byref(st))
        if rc and raise_on_error:
            self._err(rc, "szhip_compare_batch_view")
        return rc, [_quality(out[i]) for i in range(count)], st

    def decompress_omp_region(self, stream_ptr, stream_on_device, stream_len, body_off, shape3, dtype, lo, hi, out_ptr, out_on_device):
        """The sub-box [lo, hi) (per dimension, dim 0 slowest, hi exclusive) of an OpenMP-container stream (szhip_decompress_omp_region): only the boxes that
        meet it are decoded.  out_ptr receives prod(hi - lo) values, contiguous.  Returns the stats (n_blocks: the boxes decoded)."""
        st = szhip_stats()
        c_lo, c_hi = (ctypes.c_size_t * 3)(*[int(v) for v in lo]), (ctypes.c_size_t * 3)(*[int(v) for v in hi])
        rc = lib().szhip_decompress_omp_region(self._h, 0 if np.dtype(dtype) == np.float32 else 1, stream_ptr, int(stream_on_device), stream_len,
                                               body_off, shape3[0], shape3[1], shape3[2], c_lo, c_hi, out_ptr, int(out_on_device), ctypes.byref(st))
        if rc:
            self._err(rc, "szhip_decompress_omp_region")
        return st

    def compress_omp_view(self, ptr, on_device, shape3, pitches, dtype, eb, thread_num, meta, params=None, out_on_device=False):
        """szhip_compress_omp_view: the OpenMP container of the sub-box of shape3 values at ptr inside a larger array, pitches = (pitch0, pitch1) in elements (planes,
        rows).  Byte for byte the stream compress_omp makes of a contiguous copy.  Returns (bytes | device pointer int, size, stats)."""
        p = params or szhip_params(100, 0.99, 65536, 0)
        out = ctypes.c_void_p()
        n = ctypes.c_size_t(0)
        st = szhip_stats()
        rc = lib().szhip_compress_omp_view(self._h, 0 if np.dtype(dtype) == np.float32 else 1, ptr, int(on_device), shape3[0], shape3[1], shape3[2],
                                           int(pitches[0]), int(pitches[1]), eb, thread_num, ctypes.byref(p), meta, len(meta), int(out_on_device),
                                           ctypes.byref(out), ctypes.byref(n), ctypes.byref(st))
        if rc:
            self._err(rc, "szhip_compress_omp_view")
        if out_on_device:
            return out.value, n.value, st
        b = ctypes.string_at(out.value, n.value)
        lib().free(out)
        return b, n.value, st

    def decompress_omp_view(self, stream_ptr, stream_on_device, stream_len, body_off, shape3, dtype, out_ptr, out_on_device, pitches):
        """szhip_decompress_omp_view: a stream of shape3 values decoded into the sub-box at out_ptr of a larger array (pitches as above); nothing else of it is written."""
        st = szhip_stats()
        rc = lib().szhip_decompress_omp_view(self._h, 0 if np.dtype(dtype) == np.float32 else 1, stream_ptr, int(stream_on_device), stream_len,
                                             body_off, shape3[0], shape3[1], shape3[2], out_ptr, int(out_on_device), int(pitches[0]), int(pitches[1]), ctypes.byref(st))
        if rc:
            self._err(rc, "szhip_decompress_omp_view")
        return st

    def pack_view(self, ptr, on_device, shape3, pitches, dtype):
        """szhip_pack_view: the view gathered into the context's input buffer; returns its device pointer (shape3[0] == 0: a 2-D view, pitches[0] ignored)."""
        out = ctypes.c_void_p()
        rc = lib().szhip_pack_view(self._h, 0 if np.dtype(dtype) == np.float32 else 1, ptr, int(on_device), shape3[0], shape3[1], shape3[2],
                                   int(pitches[0]), int(pitches[1]), ctypes.byref(out))
        if rc:
            self._err(rc, "szhip_pack_view")
        return out.value

    def scatter_view(self, packed_ptr, shape3, dtype, out_ptr, out_on_device, pitches):
        """szhip_scatter_view: the contiguous device array at packed_ptr into the view at out_ptr."""
        rc = lib().szhip_scatter_view(self._h, 0 if np.dtype(dtype) == np.float32 else 1, packed_ptr, shape3[0], shape3[1], shape3[2], out_ptr, int(out_on_device),
                                      int(pitches[0]), int(pitches[1]))
        if rc:
            self._err(rc, "szhip_scatter_view")

    def compare(self, ori_ptr, dec_ptr, on_device, n, dtype, abs_bound=-1.0, pw_rel_bound=-1.0, corr=False):
        """szhip_compare: the n values at ori_ptr against the n at dec_ptr (on_device: one flag for both, or a pair), in one read of the two arrays on the device;
        corr: the correlation too, a second read.  Returns a Quality (include/szhip.h describes the fields); neither array is written."""
        od, dd = on_device if isinstance(on_device, (tuple, list)) else (on_device, on_device)
        q = szhip_quality()
        rc = lib().szhip_compare(self._h, 0 if np.dtype(dtype) == np.float32 else 1, ori_ptr, int(od), dec_ptr, int(dd), n, float(abs_bound), float(pw_rel_bound),
                                 SZHIP_Q_CORR if corr else 0, ctypes.byref(q))
        if rc:
            self._err(rc, "szhip_compare")
        return _quality(q)

    def minmax_batch(self, ptrs, on_device, n, dtype, raise_on_error=True):
        """szhip_minmax_batch: the value ranges of len(ptrs) arrays of n values each (host, or device with on_device) in one launch and one read-back.
        Returns (rc, [(vmin, vmax), ...], stats); pair i is bit for bit what minmax returns for array i alone."""
        count = len(ptrs)
        c_ptrs = (ctypes.c_void_p * max(count, 1))(*ptrs)
        lo, hi, st = (ctypes.c_double * max(count, 1))(), (ctypes.c_double * max(count, 1))(), szhip_stats()
        rc = lib().szhip_minmax_batch(self._h, 0 if np.dtype(dtype) == np.float32 else 1, c_ptrs, count, int(on_device), n, lo, hi, ctypes.byref(st))
        if rc and raise_on_error:
            self._err(rc, "szhip_minmax_batch")
        return rc, [(lo[i], hi[i]) for i in range(count)], st

    def minmax_batch_lens(self, ptrs, on_device, lens, dtype, raise_on_error=True):
        """szhip_minmax_batch_lens: minmax_batch with a length per array, lens[i] values at ptrs[i].  Returns (rc, [(vmin, vmax), ...], stats)."""
        count = len(ptrs)
        c_ptrs = (ctypes.c_void_p * max(count, 1))(*ptrs)
        c_lens = (ctypes.c_size_t * max(count, 1))(*lens)
        lo, hi, st = (ctypes.c_double * max(count, 1))(), (ctypes.c_double * max(count, 1))(), szhip_stats()
        rc = lib().szhip_minmax_batch_lens(self._h, 0 if np.dtype(dtype) == np.float32 else 1, c_ptrs, c_lens, count, int(on_device), lo, hi, ctypes.byref(st))
        if rc and raise_on_error:
            self._err(rc, "szhip_minmax_batch_lens")
        return rc, [(lo[i], hi[i]) for i in range(count)], st

    def compare_batch(self, ori_ptrs, dec_ptrs, on_device, n, dtype, abs_bounds, pw_rel_bounds=None, corr=False, raise_on_error=True):
        """szhip_compare_batch: len(ori_ptrs) pairs of contiguous arrays of n values each, pair i against abs_bounds[i] (and pw_rel_bounds[i]; None: not asked), in a
        number of launches that does not grow with the count.  Returns (rc, [Quality, ...], stats); record i is byte for byte what compare returns for pair i alone."""
        count = len(ori_ptrs)
        c_ori, c_dec = (ctypes.c_void_p * max(count, 1))(*ori_ptrs), (ctypes.c_void_p * max(count, 1))(*dec_ptrs)
        c_abs = (ctypes.c_double * max(count, 1))(*[float(b) for b in abs_bounds])
        c_pwr = (ctypes.c_double * max(count, 1))(*[float(b) for b in pw_rel_bounds]) if pw_rel_bounds is not None else None
        out, st = (szhip_quality * max(count, 1))(), szhip_stats()
        rc = lib().szhip_compare_batch(self._h, 0 if np.dtype(dtype) == np.float32 else 1, c_ori, c_dec, count, int(on_device), n, c_abs, c_pwr,
                                       SZHIP_Q_CORR if corr else 0, out, ctypes.byref(st))
        if rc and raise_on_error:
            self._err(rc, "szhip_compare_batch")
        return rc, [_quality(out[i]) for i in range(count)], st

    def compare_view(self, ori_ptr, ori_pitches, dec_ptr, dec_pitches, on_device, shape3, dtype, abs_bound=-1.0, pw_rel_bound=-1.0, corr=False):
        """szhip_compare_view: two boxes of shape3 values, each inside a larger array with its own (pitch0, pitch1) in elements.  The Quality of compare on contiguous
        copies of the two boxes, sums included."""
        od, dd = on_device if isinstance(on_device, (tuple, list)) else (on_device, on_device)
        q = szhip_quality()
        rc = lib().szhip_compare_view(self._h, 0 if np.dtype(dtype) == np.float32 else 1, ori_ptr, int(od), int(ori_pitches[0]), int(ori_pitches[1]),
                                      dec_ptr, int(dd), int(dec_pitches[0]), int(dec_pitches[1]), shape3[0], shape3[1], shape3[2], float(abs_bound),
                                      float(pw_rel_bound), SZHIP_Q_CORR if corr else 0, ctypes.byref(q))
        if rc:
            self._err(rc, "szhip_compare_view")
        return _quality(q)

    def store_be(self, src_ptr, n, dtype, dst_ptr, dst_on_device=True, zero_replacement=None):
        """szhip_store_be: the n values of the device array at src_ptr as big-endian bytes at dst_ptr (a device byte address of any alignment, or host memory);
        zero_replacement: a value stored in place of every value equal to zero."""
        T = np.dtype(dtype)
        z = None if zero_replacement is None else np.array([zero_replacement], dtype=T)
        rc = lib().szhip_store_be(self._h, 0 if T == np.float32 else 1, src_ptr, n, None if z is None else z.ctypes.data, dst_ptr, int(dst_on_device))
        if rc:
            self._err(rc, "szhip_store_be")

    def load_be(self, src_ptr, src_on_device, n, dtype, out_ptr):
        """szhip_load_be: n big-endian values at the byte address src_ptr (device, any alignment; or host) into the device array at out_ptr."""
        rc = lib().szhip_load_be(self._h, 0 if np.dtype(dtype) == np.float32 else 1, src_ptr, int(src_on_device), n, out_ptr)
        if rc:
            self._err(rc, "szhip_load_be")

    def fill(self, value, n, dtype, out_ptr):
        """szhip_fill: n copies of `value` into the device array at out_ptr."""
        v = np.array([value], dtype=np.dtype(dtype))
        rc = lib().szhip_fill(self._h, 0 if v.dtype == np.float32 else 1, v.ctypes.data, n, out_ptr)
        if rc:
            self._err(rc, "szhip_fill")

    def clamp(self, ptr, n, dtype, vmin, vmax):
        """szhip_clamp: the device array at ptr clamped to [vmin, vmax] in place with the reference's comparisons (a NaN stays)."""
        rc = lib().szhip_clamp(self._h, 0 if np.dtype(dtype) == np.float32 else 1, ptr, n, float(vmin), float(vmax))
        if rc:
            self._err(rc, "szhip_clamp")

    def huff_book(self, hist, on_device=False, intervals=None, tree_cap=None):
        """The device's code book of a histogram (szhip_huff_book; k_huff_book alone).  hist: a numpy uint32 array, or a device pointer with `intervals`.
        Returns (record, tree bytes, code words uint64[intervals], lengths uint8[intervals]); the arrays hold the fill byte 0xA5 when record.status != 0."""
        if on_device:
            ptr, k = hist, int(intervals)
        else:
            h = np.ascontiguousarray(hist, dtype=np.uint32)
            ptr, k = h.ctypes.data, h.size
        cap = szhip_huff_book_tree_cap() if tree_cap is None else tree_cap
        tree = np.zeros(max(cap, 1), dtype=np.uint8); code = np.zeros(k, dtype=np.uint64); ln = np.zeros(k, dtype=np.uint8)
        rec = szhip_book_record()
        rc = lib().szhip_huff_book(self._h, ptr, k, tree.ctypes.data, cap, code.ctypes.data, ln.ctypes.data, ctypes.byref(rec))
        if rc:
            self._err(rc, "szhip_huff_book")
        return rec, (tree[:rec.tree_bytes].tobytes() if rec.status == 0 else tree.tobytes()), code, ln

    def debug_fetch(self, which, count, dtype):
        """Copy an internal workspace of the last call to host (tests only; see szhip_debug_fetch)."""
        a = np.zeros(count, dtype=dtype)
        rc = lib().szhip_debug_fetch(self._h, which, a.ctypes.data, a.nbytes)
        if rc:
            self._err(rc, "szhip_debug_fetch")
        return a

    def decompress(self, stream_ptr, stream_on_device, stream_len, body_off, shape3, dtype, out_ptr, out_on_device):
        st = szhip_stats()
        rc = lib().szhip_decompress(self._h, 0 if np.dtype(dtype) == np.float32 else 1, stream_ptr, int(stream_on_device), stream_len,
                                    body_off, shape3[0], shape3[1], shape3[2], out_ptr, int(out_on_device), ctypes.byref(st))
        if rc:
            self._err(rc, "szhip_decompress")
        return st
