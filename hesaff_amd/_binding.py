"""ctypes binding of libhesaff_amd.so (C ABI in include/hesaff_amd.h)."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))


class HesaffError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("hesaff_amd error %d: %s" % (code, msg))
        self.code = code


class Params(C.Structure):
    """hesaff_params (include/hesaff_amd.h): reference defaults + capacity knobs."""
    _fields_ = [
        ("threshold", C.c_float),
        ("edgeEigenValueRatio", C.c_float),
        ("initialSigma", C.c_float),
        ("maxIterations", C.c_int),
        ("convergenceThreshold", C.c_float),
        ("mrSize", C.c_float),
        ("maxBinValue", C.c_float),
        ("upscaleInputImage", C.c_int),
        ("max_batch", C.c_int),
        ("max_kpts_per_mpx", C.c_int),
        ("fast", C.c_int),
    ]


class _Result(C.Structure):
    _fields_ = [("count_hessian", C.c_int32), ("count_desc", C.c_int32), ("keys", C.c_void_p)]


class Timings(C.Structure):
    _fields_ = [
        ("pyramid_ms", C.c_float), ("detect_ms", C.c_float), ("affine_ms", C.c_float), ("patch_ms", C.c_float),
        ("sift_ms", C.c_float), ("pack_ms", C.c_float), ("total_ms", C.c_float), ("blur_hess_ms", C.c_float), ("blur_hess_launches", C.c_int32),
        ("blur_hess_bytes", C.c_double), ("pyramid_bytes", C.c_double),
        ("extrema_ms", C.c_float), ("extrema_launches", C.c_int32), ("extrema_bytes", C.c_double),
        ("export_ms", C.c_float), ("export_rows", C.c_int32),
    ]


# struct Keypoint of hesaff.cpp:41-48 == hesaff_keypoint, 164 bytes
KEYPOINT_DTYPE = np.dtype([
    ("x", "<f4"), ("y", "<f4"), ("s", "<f4"), ("a11", "<f4"), ("a12", "<f4"), ("a21", "<f4"), ("a22", "<f4"),
    ("response", "<f4"), ("type", "<i4"), ("desc", "u1", (128,)),
])
assert KEYPOINT_DTYPE.itemsize == 164


class Region(C.Structure):
    """hesaff_region: one onHessianKeypointDetected call (pyramid.h:43-47) and what hesaff.cpp:66-105 made of it, 64 bytes."""
    _fields_ = [
        ("x", C.c_float), ("y", C.c_float), ("s", C.c_float), ("pixelDistance", C.c_float), ("response", C.c_float),
        ("type", C.c_int32), ("octave", C.c_int32), ("level", C.c_int32),
        ("a11", C.c_float), ("a12", C.c_float), ("a21", C.c_float), ("a22", C.c_float),
        ("iters", C.c_int32), ("outcome", C.c_int32), ("key", C.c_int32), ("reserved", C.c_int32),
    ]


# the same record as a numpy structured dtype (field offsets = Region's)
REGION_DTYPE = np.dtype({
    "names": [n for n, _ in Region._fields_],
    "formats": ["<f4" if t is C.c_float else "<i4" for _, t in Region._fields_],
    "offsets": [getattr(Region, n).offset for n, _ in Region._fields_],
    "itemsize": C.sizeof(Region),
})
assert REGION_DTYPE.itemsize == 64
REGION_NOT_CONVERGED, REGION_REJECTED, REGION_DESCRIBED = 0, 1, 2   # hesaff_region.outcome


class _RegionResult(C.Structure):
    _fields_ = [("count_hessian", C.c_int32), ("count_desc", C.c_int32), ("regions", C.c_void_p), ("keys", C.c_void_p)]

_f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
_i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
_u8p = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")

ABI_VERSION = 8   # HESAFF_ABI_VERSION of the include/hesaff_amd.h these ctypes structs mirror


class JpegLayout(C.Structure):
    """hesaff_jpeg_layout: what the JPEG images of one device chunk share."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("channels", C.c_int32)] + \
               [(n, C.c_int32 * 3) for n in ("h", "v", "hx", "vx", "bw", "bh", "cw", "chgt")]


class HostPlan(C.Structure):
    """hesaff_host_plan: one device's share of the host (hesaff_host_plan_for)"""
    _fields_ = [("cpus", C.c_int), ("decode_threads", C.c_int), ("write_threads", C.c_int), ("stage_threads", C.c_int)]


def host_plan(devices_sharing_host=1):
    """The library's one rule for host threads per device: dict(cpus, decode_threads, write_threads, stage_threads)."""
    hp = HostPlan()
    rc = load_library().hesaff_host_plan_for(int(devices_sharing_host), C.byref(hp))
    if rc != 0:
        raise HesaffError(rc, "hesaff_host_plan_for(%r)" % (devices_sharing_host,))
    return {k: int(getattr(hp, k)) for k, _ in HostPlan._fields_}


class FileStatus(C.Structure):
    """hesaff_file_status"""
    _fields_ = [("rc", C.c_int32), ("stage", C.c_int32), ("count_hessian", C.c_int32), ("count_desc", C.c_int32)]


CHUNK_SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(_Result))

_lib = None


def lib_path():
    # HESAFF_AMD_LIB: another build of the same library (the tuning build, or another commit's for a comparison)
    return os.environ.get("HESAFF_AMD_LIB") or os.path.join(_HERE, "libhesaff_amd.so")


def load_library():
    """Load libhesaff_amd.so; fails loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch bundles its own HIP runtime (torch/lib/libamdhip64.so).  Two HIP runtimes in one
    # process cannot both see the GPU, so when torch is installed it is imported FIRST and
    # libhesaff_amd.so binds to the runtime torch already loaded (same SONAME).  Without torch
    # (e.g. the hesaff CLI) the library uses the system ROCm runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    p = lib_path()
    if not os.path.exists(p):
        raise HesaffError(-1, "%s not built: run `make -C hesaff_amd/csrc` (or __graft_entry__.build())" % p)
    L = C.CDLL(p)
    vp = C.c_void_p
    L.hesaff_version.restype = C.c_char_p
    L.hesaff_abi_version.argtypes = []
    L.hesaff_sizeof_params.argtypes = []; L.hesaff_sizeof_params.restype = C.c_size_t
    L.hesaff_sizeof_timings.argtypes = []; L.hesaff_sizeof_timings.restype = C.c_size_t
    abi = L.hesaff_abi_version()
    sizeof_region = 0
    if abi >= 8:   # (older libraries lack the symbol: the version check below reports them)
        L.hesaff_sizeof_region.argtypes = []; L.hesaff_sizeof_region.restype = C.c_size_t
        sizeof_region = L.hesaff_sizeof_region()
    if (abi != ABI_VERSION or L.hesaff_sizeof_params() != C.sizeof(Params)
            or L.hesaff_sizeof_timings() != C.sizeof(Timings) or sizeof_region != C.sizeof(Region)):
        raise HesaffError(-2, "%s has ABI version %d (params %d bytes, timings %d bytes, region %d bytes); this binding mirrors version %d (%d, %d, %d)"
                          % (p, abi, L.hesaff_sizeof_params(), L.hesaff_sizeof_timings(), sizeof_region, ABI_VERSION,
                             C.sizeof(Params), C.sizeof(Timings), C.sizeof(Region)))
    L.hesaff_default_params.argtypes = [C.POINTER(Params)]
    L.hesaff_create.argtypes = [C.POINTER(vp), C.POINTER(Params), C.c_int]
    L.hesaff_destroy.argtypes = [vp]; L.hesaff_destroy.restype = None
    L.hesaff_last_error.argtypes = [vp]; L.hesaff_last_error.restype = C.c_char_p
    L.hesaff_detect_batch.argtypes = [vp, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                      C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(_Result)]
    L.hesaff_detect_regions.argtypes = [vp, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                        C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(_RegionResult)]
    L.hesaff_detect_batch_cb.argtypes = [vp, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                         C.POINTER(C.c_int), C.POINTER(C.c_int), CHUNK_SINK, vp]
    L.hesaff_process_files.argtypes = [vp, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_int, C.c_int, C.POINTER(FileStatus)]
    L.hesaff_write_sift_mt.argtypes = [C.c_char_p, vp, C.c_int, C.c_float, C.c_int]
    L.hesaff_write_bin.argtypes = [C.c_char_p, vp, C.c_int, C.c_float]
    L.hesaff_set_output_format.argtypes = [vp, C.c_int]
    L.hesaff_set_resume.argtypes = [vp, C.c_int]
    L.hesaff_output_is_complete.argtypes = [C.c_char_p, C.c_int]
    L.hesaff_set_pinned_read_budget.argtypes = [vp, C.c_size_t, C.c_size_t]
    L.hesaff_set_pool_priority.argtypes = [vp, C.c_int]
    L.hesaff_set_keypoint_limit.argtypes = [vp, C.c_int]
    L.hesaff_get_keypoint_limit.argtypes = [vp, C.POINTER(C.c_int)]
    if hasattr(L, "hesaff_set_keypoint_grid"):   # (absent from an older build loaded through HESAFF_AMD_LIB for a comparison)
        L.hesaff_set_keypoint_grid.argtypes = [vp, C.c_int, C.c_int]
        L.hesaff_get_keypoint_grid.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    # per-image detection masks for the next detecting call (found by name, like hesaff_describe_regions)
    if hasattr(L, "hesaff_set_next_masks"):
        L.hesaff_set_next_masks.argtypes = [vp, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
        L.hesaff_set_next_masks_device.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int64]
    L.hesaff_stage_threads_for_pool.argtypes = [C.c_int]
    L.hesaff_detect_batch_device.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, _i32p, _i32p, C.POINTER(vp), C.POINTER(C.c_int64)]
    # float grey planes (CV_32FC1, pyramid.h:73): the twins above with float images
    L.hesaff_detect_batch_f32.argtypes = [vp, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                          C.POINTER(_Result)]
    L.hesaff_detect_regions_f32.argtypes = [vp, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                            C.POINTER(_RegionResult)]
    L.hesaff_detect_batch_cb_f32.argtypes = [vp, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                             CHUNK_SINK, vp]
    L.hesaff_detect_batch_device_f32.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int64, _i32p, _i32p, C.POINTER(vp),
                                                 C.POINTER(C.c_int64)]
    L.hesaff_stage_pyramid_f32.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.POINTER(C.c_int), C.POINTER(C.c_size_t)]
    # describe caller-supplied keypoints (found by name: a library of ABI version 8 built before them lacks the two symbols)
    if hasattr(L, "hesaff_describe_regions"):
        L.hesaff_describe_regions.argtypes = [vp, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                              C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int, C.POINTER(_RegionResult)]
        L.hesaff_describe_regions_f32.argtypes = [vp, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                                  C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int, C.POINTER(_RegionResult)]
    L.hesaff_set_profiling.argtypes = [vp, C.c_int]
    L.hesaff_get_timings.argtypes = [vp, C.POINTER(Timings)]
    L.hesaff_ellipse.argtypes = [vp, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.hesaff_ellipse.restype = None
    L.hesaff_write_sift.argtypes = [C.c_char_p, vp, C.c_int, C.c_float]
    L.hesaff_format_sift.argtypes = [vp, C.c_int, C.c_float, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.hesaff_format_sift_mt.argtypes = [vp, C.c_int, C.c_float, C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.hesaff_host_threads.argtypes = []
    L.hesaff_host_threads.restype = C.c_int
    L.hesaff_host_plan_for.argtypes = [C.c_int, C.POINTER(HostPlan)]
    L.hesaff_host_plan_for.restype = C.c_int
    L.hesaff_write_sift_batch.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(_Result), C.c_float, C.c_int]
    L.hesaff_test_fmt_g.argtypes = [_f32p, C.c_int]
    L.hesaff_free.argtypes = [vp]; L.hesaff_free.restype = None
    L.hesaff_read_pnm.argtypes = [C.c_char_p, C.POINTER(vp), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.hesaff_read_png.argtypes = L.hesaff_read_pnm.argtypes
    L.hesaff_read_image.argtypes = L.hesaff_read_pnm.argtypes
    L.hesaff_read_bmp.argtypes = L.hesaff_read_pnm.argtypes
    L.hesaff_read_tiff.argtypes = L.hesaff_read_pnm.argtypes
    L.hesaff_read_jpeg.argtypes = L.hesaff_read_pnm.argtypes
    L.hesaff_stage_gaussian_blur.argtypes = [vp, _f32p, C.c_int, C.c_int, C.c_float, _f32p]
    L.hesaff_stage_hessian_response.argtypes = [vp, _f32p, C.c_int, C.c_int, C.c_float, _f32p]
    L.hesaff_stage_half_image.argtypes = [vp, _f32p, C.c_int, C.c_int, _f32p]
    L.hesaff_stage_pyramid.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.POINTER(C.c_int), C.POINTER(C.c_size_t)]
    L.hesaff_stage_hessian_keypoints.argtypes = [vp, _u8p, C.c_int, C.c_int, C.c_int, _f32p, _i32p, C.POINTER(C.c_int)]
    L.hesaff_stage_detect_planes.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, vp, vp, vp, C.POINTER(C.c_int)]
    L.hesaff_stage_find_affine_shape.argtypes = [vp, _f32p, C.c_int, C.c_int, C.c_int, _f32p, _i32p, _f32p, _i32p]
    L.hesaff_stage_rectify.argtypes = [vp, C.c_int, _f32p]
    if hasattr(L, "hesaff_stage_affine_tail"):   # (absent from an older build loaded through HESAFF_AMD_LIB for a comparison)
        L.hesaff_stage_affine_tail.argtypes = [vp, C.c_int, _f32p, _f32p, _f32p, _f32p, _i32p]
    L.hesaff_stage_normalize_affine.argtypes = [vp, _f32p, C.c_int, C.c_int, C.c_int, _f32p, _f32p, _i32p, _f32p]
    L.hesaff_stage_sift.argtypes = [vp, C.c_int, _f32p, _u8p]
    L.hesaff_stage_sift_parts.argtypes = [vp, C.c_int, _f32p, _f32p, _f32p, _u8p]
    if hasattr(L, "hesaff_stage_sift_alive"):   # (absent from an older build loaded through HESAFF_AMD_LIB for a comparison)
        L.hesaff_stage_sift_alive.argtypes = [vp, C.c_int, _f32p, _i32p, _u8p]
    if hasattr(L, "hesaff_set_orientation"):   # (likewise)
        L.hesaff_set_orientation.argtypes = [vp, C.c_int]
        L.hesaff_get_orientation.argtypes = [vp, C.POINTER(C.c_int)]
        L.hesaff_stage_orientation.argtypes = [vp, C.c_int, _f32p, _f32p, _f32p, _f32p]
    if hasattr(L, "hesaff_set_orientation_count"):   # (likewise)
        L.hesaff_set_orientation_count.argtypes = [vp, C.c_int]
        L.hesaff_get_orientation_count.argtypes = [vp, C.POINTER(C.c_int)]
        L.hesaff_stage_orientation_peaks.argtypes = [vp, C.c_int, _f32p, C.c_int, _i32p, _i32p, _f32p]
    if hasattr(L, "hesaff_set_descriptor"):   # (likewise)
        L.hesaff_set_descriptor.argtypes = [vp, C.c_int]
        L.hesaff_get_descriptor.argtypes = [vp, C.POINTER(C.c_int)]
        L.hesaff_stage_sift_mode.argtypes = [vp, C.c_int, _f32p, C.c_void_p, C.c_int, _u8p]
    if hasattr(L, "hesaff_set_vocabulary"):   # (likewise)
        L.hesaff_set_vocabulary.argtypes = [vp, C.c_int, vp]
        L.hesaff_get_vocabulary_size.argtypes = [vp, C.POINTER(C.c_int)]
        L.hesaff_get_words.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_int)]
        L.hesaff_get_words_device.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int64)]
        L.hesaff_assign_words_device.argtypes = [vp, C.c_int64, vp, C.c_int64, C.c_int64, vp]
        L.hesaff_stage_assign_words.argtypes = [vp, C.c_int, vp, vp]
        L.hesaff_get_assign_ms.argtypes = [vp, C.POINTER(C.c_float)]
        L.hesaff_write_words.argtypes = [C.c_char_p, vp, vp, C.c_int, C.c_float, C.c_int]
        L.hesaff_read_vocabulary.argtypes = [C.c_char_p, C.POINTER(vp), C.POINTER(C.c_int)]
        L.hesaff_write_vocabulary.argtypes = [C.c_char_p, vp, C.c_int]
    if hasattr(L, "hesaff_train_vocabulary"):   # (likewise)
        L.hesaff_train_vocabulary_device.argtypes = [vp, C.c_int64, vp, C.c_int64, C.c_int64, C.c_int, vp, C.c_int, vp, vp, vp, C.POINTER(C.c_int)]
        L.hesaff_train_vocabulary.argtypes = [vp, C.c_int64, vp, C.c_int, vp, C.c_int, vp, vp, vp, C.POINTER(C.c_int)]
        L.hesaff_stage_accumulate_words.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, vp]
        L.hesaff_get_training_ms.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]
    if hasattr(L, "hesaff_set_vocabulary_cells"):   # (likewise)
        L.hesaff_set_vocabulary_cells.argtypes = [vp, C.c_int, vp, vp]
        L.hesaff_get_vocabulary_cells.argtypes = [vp, C.POINTER(C.c_int)]
        L.hesaff_get_assign_cells_ms.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.hesaff_build_vocabulary_cells.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp, vp, vp, vp, C.POINTER(C.c_int)]
        L.hesaff_train_vocabulary_cells_device.argtypes = [vp, C.c_int64, vp, C.c_int64, C.c_int64, C.c_int, vp, C.c_int, vp, vp, C.c_int, vp, vp, vp,
                                                           C.POINTER(C.c_int)]
        L.hesaff_train_vocabulary_cells.argtypes = [vp, C.c_int64, vp, C.c_int, vp, C.c_int, vp, vp, C.c_int, vp, vp, vp, C.POINTER(C.c_int)]
        L.hesaff_read_vocabulary_cells.argtypes = [C.c_char_p, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.hesaff_write_vocabulary_cells.argtypes = [C.c_char_p, C.c_int, vp, vp]
    if hasattr(L, "hesaff_set_vocabulary_probes"):   # (likewise)
        L.hesaff_set_vocabulary_probes.argtypes = [vp, C.c_int]
        L.hesaff_get_vocabulary_probes.argtypes = [vp, C.POINTER(C.c_int)]
        L.hesaff_stage_probe_cells.argtypes = [vp, C.c_int, vp, vp, vp]
    if hasattr(L, "hesaff_set_vocabulary_neighbours"):   # (likewise)
        L.hesaff_set_vocabulary_neighbours.argtypes = [vp, C.c_int]
        L.hesaff_get_vocabulary_neighbours.argtypes = [vp, C.POINTER(C.c_int)]
        L.hesaff_get_neighbours.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.hesaff_get_neighbours_device.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int64), C.POINTER(C.c_int)]
        L.hesaff_assign_neighbours_device.argtypes = [vp, C.c_int64, vp, C.c_int64, C.c_int64, vp]
        L.hesaff_stage_assign_neighbours.argtypes = [vp, C.c_int, vp, vp]
    if hasattr(L, "hesaff_index_build"):   # (likewise)
        L.hesaff_index_build.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.c_int]
        L.hesaff_index_build_device.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.c_int]
        L.hesaff_index_query.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, C.POINTER(C.c_int)]
        L.hesaff_index_query_device.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, C.POINTER(C.c_int)]
        L.hesaff_index_get_scores.argtypes = [vp, vp, vp, vp]
        L.hesaff_index_get_tables.argtypes = [vp, vp, vp, vp]
        L.hesaff_index_get_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.hesaff_index_clear.argtypes = [vp]
        L.hesaff_get_index_ms.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.hesaff_read_words.argtypes = [C.c_char_p, C.POINTER(vp), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    if hasattr(L, "hesaff_verify_matches"):   # (likewise)
        L.hesaff_verify_matches.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_float, vp, vp, vp]
        L.hesaff_verify_matches_device.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_float, vp, vp, vp]
        L.hesaff_verify_get_pairs.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_int)]
        L.hesaff_verify_get_query_inert.argtypes = [vp, C.POINTER(C.c_int)]
        L.hesaff_stage_verify_pairs.argtypes = [vp, C.c_int, vp, C.c_float, vp, C.POINTER(C.c_int32)]
        L.hesaff_get_verify_ms.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.hesaff_read_words_rows.argtypes = [C.c_char_p, C.POINTER(vp), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    if hasattr(L, "hesaff_expand_query"):   # (likewise)
        L.hesaff_expand_query.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, C.POINTER(C.c_int), vp]
        L.hesaff_expand_query_device.argtypes = L.hesaff_expand_query.argtypes
        L.hesaff_get_expand_ms.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    if hasattr(L, "hesaff_set_embedding"):   # (likewise)
        i64 = C.c_int64
        L.hesaff_embedding_projection.argtypes = [C.c_uint64, vp]
        L.hesaff_set_embedding.argtypes = [vp, vp, vp]
        L.hesaff_get_embedding.argtypes = [vp, C.POINTER(C.c_int), vp, vp]
        L.hesaff_get_signatures.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_int)]
        L.hesaff_get_signatures_device.argtypes = [vp, C.POINTER(vp), C.POINTER(i64)]
        L.hesaff_embed_device.argtypes = [vp, i64, vp, i64, i64, vp, C.c_int, vp]
        L.hesaff_stage_embed.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp]
        L.hesaff_stage_project.argtypes = [vp, C.c_int, vp, vp, vp]
        L.hesaff_train_embedding.argtypes = [vp, i64, vp, vp, C.c_int, C.c_int, vp, vp, vp]
        L.hesaff_train_embedding_device.argtypes = [vp, i64, vp, i64, i64, vp, C.c_int, C.c_int, vp, vp, vp]
        L.hesaff_get_embedding_ms.argtypes = [vp] + [C.POINTER(C.c_float)] * 4
        L.hesaff_index_build_embedded.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, C.c_int]
        L.hesaff_index_build_embedded_device.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, C.c_int]
        L.hesaff_index_query_embedded.argtypes = [vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, C.POINTER(C.c_int)]
        L.hesaff_index_query_embedded_device.argtypes = [vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, C.POINTER(C.c_int)]
        L.hesaff_index_get_embedded.argtypes = [vp, C.POINTER(C.c_int), vp, vp, vp]
        L.hesaff_write_embedding.argtypes = [C.c_char_p, C.c_int, vp, vp]
        L.hesaff_read_embedding.argtypes = [C.c_char_p, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int)]
        L.hesaff_write_signatures.argtypes = [C.c_char_p, vp, C.c_int]
        L.hesaff_read_signatures.argtypes = [C.c_char_p, C.POINTER(vp), C.POINTER(C.c_int)]
        L.hesaff_signatures_is_complete.argtypes = [C.c_char_p]
    if hasattr(L, "hesaff_index_add"):   # (likewise)
        L.hesaff_index_add.argtypes = [vp, C.c_int, vp, vp, C.c_int]
        L.hesaff_index_add_device.argtypes = [vp, C.c_int, vp, vp, C.c_int]
        L.hesaff_index_add_embedded.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp]
        L.hesaff_index_add_embedded_device.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp]
        L.hesaff_index_get_postings.argtypes = [vp, vp, vp, vp]
        L.hesaff_index_save.argtypes = [vp, C.c_char_p]
        L.hesaff_index_load.argtypes = [vp, C.c_char_p]
        L.hesaff_get_index_growth_ms.argtypes = [vp] + [C.POINTER(C.c_float)] * 5
        L.hesaff_write_index_file.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, i64, i64, vp, vp, vp, vp, vp]
        L.hesaff_read_index_file.argtypes = [C.c_char_p] + [C.POINTER(C.c_int)] * 3 + [C.POINTER(i64)] * 2 + [C.POINTER(vp)] * 5
    if hasattr(L, "hesaff_index_remove"):   # (likewise)
        L.hesaff_index_remove.argtypes = [vp, C.c_int, vp, vp]
        L.hesaff_get_index_remove_ms.argtypes = [vp] + [C.POINTER(C.c_float)] * 4
    if hasattr(L, "hesaff_index_query_batch"):   # (likewise)
        L.hesaff_index_query_batch.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.c_int, vp, vp, C.POINTER(C.c_int)]
        L.hesaff_index_query_batch_device.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.c_int, vp, vp, C.POINTER(C.c_int)]
        L.hesaff_index_query_batch_embedded.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, C.POINTER(C.c_int)]
        L.hesaff_index_query_batch_embedded_device.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, C.POINTER(C.c_int)]
        L.hesaff_index_set_batch_budget.argtypes = [vp, C.c_size_t]
        L.hesaff_index_get_batch_budget.argtypes = [vp, C.POINTER(C.c_size_t)]
        L.hesaff_index_get_batch_chunks.argtypes = [vp, C.POINTER(C.c_int)]
        L.hesaff_get_index_batch_ms.argtypes = [vp] + [C.POINTER(C.c_float)] * 3
    L.hesaff_stage_math_sift_general.argtypes = [vp, C.c_int, _f32p, _f32p, _f32p, _f32p, _f32p]
    L.hesaff_stage_math.argtypes = [vp, C.c_int, _f32p, _f32p, _f32p, _f32p]
    L.hesaff_stage_math_sift.argtypes = [vp, C.c_int, _f32p, _f32p, _f32p, _f32p, _f32p, _f32p]
    L.hesaff_stage_export.argtypes = [vp, vp, C.c_int, C.c_float, C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.hesaff_stage_fmt_g.argtypes = [vp, C.c_int, _f32p, vp, _i32p]
    L.hesaff_read_jpeg_coefficients.argtypes = [C.c_char_p, C.POINTER(JpegLayout), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.hesaff_stage_jpeg_pixels.argtypes = [vp, C.POINTER(JpegLayout), C.c_int, vp, C.c_size_t, vp]
    L.hesaff_write_sift_rows.argtypes = [C.c_char_p, vp, C.c_size_t, C.c_int]
    L.hesaff_write_bin_rows.argtypes = [C.c_char_p, vp, C.c_int]
    L.hesaff_shard_range.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.hesaff_table_gauss_mask.argtypes = [C.c_int, _f32p]
    L.hesaff_table_circ_gauss_mask.argtypes = [C.c_int, _f32p]
    L.hesaff_table_sift_bins.argtypes = [_i32p, _i32p, _f32p, _f32p]
    L.hesaff_table_gauss_kernel.argtypes = [C.c_float, C.c_int, vp, C.POINTER(C.c_int)]
    _lib = L
    return L


# every symbol include/hesaff_amd.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "hesaff_version", "hesaff_default_params", "hesaff_create", "hesaff_destroy", "hesaff_last_error",
    "hesaff_detect_batch", "hesaff_detect_batch_device", "hesaff_set_profiling", "hesaff_get_timings", "hesaff_ellipse",
    "hesaff_write_sift", "hesaff_format_sift", "hesaff_free", "hesaff_read_pnm", "hesaff_stage_gaussian_blur",
    "hesaff_stage_hessian_response", "hesaff_stage_half_image", "hesaff_stage_pyramid", "hesaff_stage_hessian_keypoints",
    "hesaff_stage_find_affine_shape", "hesaff_stage_rectify", "hesaff_stage_affine_tail", "hesaff_stage_normalize_affine", "hesaff_stage_sift",
    "hesaff_stage_math", "hesaff_stage_math_sift", "hesaff_stage_sift_parts", "hesaff_stage_sift_alive", "hesaff_stage_math_sift_general", "hesaff_table_gauss_mask", "hesaff_table_circ_gauss_mask", "hesaff_table_sift_bins",
    "hesaff_table_gauss_kernel", "hesaff_format_sift_mt", "hesaff_write_sift_batch", "hesaff_test_fmt_g",
    "hesaff_read_png", "hesaff_read_image", "hesaff_device_count", "hesaff_shard_range", "hesaff_read_jpeg",
    "hesaff_host_threads", "hesaff_host_plan_for", "hesaff_abi_version", "hesaff_sizeof_params", "hesaff_sizeof_timings", "hesaff_detect_batch_cb",
    "hesaff_process_files", "hesaff_write_sift_mt", "hesaff_write_bin", "hesaff_set_output_format",
    "hesaff_write_sift_rows", "hesaff_write_bin_rows", "hesaff_stage_export", "hesaff_stage_fmt_g", "hesaff_set_resume",
    "hesaff_output_is_complete", "hesaff_read_jpeg_coefficients", "hesaff_read_jpeg_coefficients_alloc", "hesaff_stage_jpeg_pixels",
    "hesaff_read_pnm_alloc", "hesaff_read_image_alloc", "hesaff_set_pinned_read_budget", "hesaff_set_pool_priority",
    "hesaff_stage_threads_for_pool", "hesaff_read_bmp", "hesaff_read_tiff", "hesaff_detect_regions", "hesaff_sizeof_region",
    "hesaff_detect_batch_f32", "hesaff_detect_batch_cb_f32", "hesaff_detect_regions_f32", "hesaff_detect_batch_device_f32",
    "hesaff_stage_pyramid_f32", "hesaff_describe_regions", "hesaff_describe_regions_f32",
    "hesaff_set_keypoint_limit", "hesaff_get_keypoint_limit", "hesaff_set_next_masks", "hesaff_set_next_masks_device",
    "hesaff_set_orientation", "hesaff_get_orientation", "hesaff_stage_orientation",
    "hesaff_set_keypoint_grid", "hesaff_get_keypoint_grid", "hesaff_stage_detect_planes",
    "hesaff_set_descriptor", "hesaff_get_descriptor", "hesaff_stage_sift_mode",
    "hesaff_set_orientation_count", "hesaff_get_orientation_count", "hesaff_stage_orientation_peaks",
    "hesaff_set_vocabulary", "hesaff_get_vocabulary_size", "hesaff_get_words", "hesaff_get_words_device",
    "hesaff_assign_words_device", "hesaff_stage_assign_words", "hesaff_get_assign_ms", "hesaff_write_words",
    "hesaff_read_vocabulary", "hesaff_write_vocabulary",
    "hesaff_train_vocabulary", "hesaff_train_vocabulary_device", "hesaff_stage_accumulate_words", "hesaff_get_training_ms",
    "hesaff_set_vocabulary_cells", "hesaff_get_vocabulary_cells", "hesaff_get_assign_cells_ms", "hesaff_build_vocabulary_cells",
    "hesaff_train_vocabulary_cells", "hesaff_train_vocabulary_cells_device", "hesaff_read_vocabulary_cells", "hesaff_write_vocabulary_cells",
    "hesaff_set_vocabulary_probes", "hesaff_get_vocabulary_probes", "hesaff_stage_probe_cells",
    "hesaff_index_build", "hesaff_index_build_device", "hesaff_index_query", "hesaff_index_query_device", "hesaff_index_get_scores",
    "hesaff_index_get_tables", "hesaff_index_get_info", "hesaff_index_clear", "hesaff_get_index_ms", "hesaff_read_words",
    "hesaff_verify_matches", "hesaff_verify_matches_device", "hesaff_verify_get_pairs", "hesaff_verify_get_query_inert",
    "hesaff_stage_verify_pairs", "hesaff_get_verify_ms", "hesaff_read_words_rows",
    "hesaff_embedding_projection", "hesaff_set_embedding", "hesaff_get_embedding", "hesaff_get_signatures", "hesaff_get_signatures_device",
    "hesaff_embed_device", "hesaff_stage_embed", "hesaff_stage_project", "hesaff_train_embedding", "hesaff_train_embedding_device",
    "hesaff_get_embedding_ms", "hesaff_index_build_embedded", "hesaff_index_build_embedded_device", "hesaff_index_query_embedded",
    "hesaff_index_query_embedded_device", "hesaff_index_get_embedded", "hesaff_write_embedding", "hesaff_read_embedding",
    "hesaff_write_signatures", "hesaff_read_signatures", "hesaff_signatures_is_complete",
    "hesaff_index_add", "hesaff_index_add_device", "hesaff_index_add_embedded", "hesaff_index_add_embedded_device", "hesaff_index_get_postings",
    "hesaff_index_save", "hesaff_index_load", "hesaff_get_index_growth_ms", "hesaff_write_index_file", "hesaff_read_index_file",
    "hesaff_index_query_batch", "hesaff_index_query_batch_device", "hesaff_index_query_batch_embedded", "hesaff_index_query_batch_embedded_device",
    "hesaff_index_set_batch_budget", "hesaff_index_get_batch_budget", "hesaff_index_get_batch_chunks", "hesaff_get_index_batch_ms",
    "hesaff_set_vocabulary_neighbours", "hesaff_get_vocabulary_neighbours", "hesaff_get_neighbours", "hesaff_get_neighbours_device",
    "hesaff_assign_neighbours_device", "hesaff_stage_assign_neighbours",
    "hesaff_index_remove", "hesaff_get_index_remove_ms",
    "hesaff_expand_query", "hesaff_expand_query_device", "hesaff_get_expand_ms",
]

# hesaff_set_output_format's bits
OUT_TEXT = 1
OUT_BIN = 2
OUT_WORDS = 4   # <image>.hesaff.words (needs a vocabulary)

# hesaff_set_descriptor's modes
DESC_SIFT = 0       # the reference's SIFT bytes (default)
DESC_ROOTSIFT = 1   # the vector L1-normalised and square-rooted before it is quantised
_DESC_NAMES = {"sift": DESC_SIFT, "rootsift": DESC_ROOTSIFT}

# hesaff_set_orientation's modes
ORI_UP = 0         # the reference's "up is up" frame (default)
ORI_DOMINANT = 1   # the frame turned by the dominant gradient angle of the keypoint's own patch
_ORI_NAMES = {"up": ORI_UP, "dominant": ORI_DOMINANT}

class _OrientationMode(int):
    """What HesaffContext.orientation returns: the mode, an int.  It is a subclass only so that the spelling
    ctx.orientation(patches) works beside the property; the operator itself is HesaffContext.orientation_of, which is what new
    code should call.  The object keeps a reference to its context, and compares, hashes and pickles as the plain int."""

    def __reduce__(self):
        return (int, (int(self),))


    def __new__(cls, value, ctx):
        self = super().__new__(cls, value)
        self._ctx = ctx
        return self

    def __call__(self, patches, parts=False):
        return self._ctx.orientation_of(patches, parts)


# hesaff_describe_regions' `from`: which of the reference's two public callback members each record enters the chain through
FROM_POINTS = 1   # onHessianKeypointDetected (hesaff.cpp:66-71): findAffineShape, then the rest when it converges
FROM_SHAPES = 2   # onAffineShapeFound (hesaff.cpp:73-105): rectify, normalizeAffine, SIFT


def default_params():
    p = Params()
    load_library().hesaff_default_params(C.byref(p))
    return p


def table_gauss_mask(size):
    m = np.zeros((size, size), np.float32)
    load_library().hesaff_table_gauss_mask(size, m)
    return m


def table_circ_gauss_mask(size):
    m = np.zeros((size, size), np.float32)
    load_library().hesaff_table_circ_gauss_mask(size, m)
    return m


def table_sift_bins():
    b0 = np.zeros(41, np.int32); b1 = np.zeros(41, np.int32); w0 = np.zeros(41, np.float32); w1 = np.zeros(41, np.float32)
    load_library().hesaff_table_sift_bins(b0, b1, w0, w1)
    return b0, b1, w0, w1


def table_gauss_kernel(sigma):
    L = load_library()
    k = C.c_int()
    L.hesaff_table_gauss_kernel(sigma, 0, None, C.byref(k))
    taps = np.zeros(k.value, np.float32)
    L.hesaff_table_gauss_kernel(sigma, k.value, taps.ctypes.data, C.byref(k))
    return taps


def ellipse(keys, mr_size):
    """(a,b,c) of each record, hesaff.cpp:115-123 in closed form."""
    L = load_library()
    keys = np.ascontiguousarray(keys, dtype=KEYPOINT_DTYPE)
    out = np.zeros((len(keys), 3), np.float32)
    a = C.c_float(); b = C.c_float(); c = C.c_float()
    base = keys.ctypes.data
    for i in range(len(keys)):
        L.hesaff_ellipse(base + i * 164, mr_size, C.byref(a), C.byref(b), C.byref(c))
        out[i] = (a.value, b.value, c.value)
    return out


def format_sift(keys, mr_size):
    """exportKeypoints hesaff.cpp:107-130 -> bytes of the .hesaff.sift file."""
    L = load_library()
    keys = np.ascontiguousarray(keys, dtype=KEYPOINT_DTYPE)
    buf = C.c_void_p(); n = C.c_size_t()
    rc = L.hesaff_format_sift(keys.ctypes.data, len(keys), mr_size, C.byref(buf), C.byref(n))
    if rc != 0:
        raise HesaffError(rc, "hesaff_format_sift")
    try:
        return C.string_at(buf.value, n.value)
    finally:
        L.hesaff_free(buf)


def format_sift_mt(keys, mr_size, threads=0):
    """Same bytes as format_sift, rows formatted by `threads` host threads (0 = auto)."""
    L = load_library()
    keys = np.ascontiguousarray(keys, dtype=KEYPOINT_DTYPE)
    buf = C.c_void_p(); n = C.c_size_t()
    rc = L.hesaff_format_sift_mt(keys.ctypes.data, len(keys), C.c_float(mr_size), threads, C.byref(buf), C.byref(n))
    if rc != 0:
        raise HesaffError(rc, "hesaff_format_sift_mt")
    try:
        return C.string_at(buf.value, n.value)
    finally:
        L.hesaff_free(buf)


def write_sift_batch(paths, key_arrays, mr_size, threads=0):
    """One .hesaff.sift per image: key_arrays[i] (KEYPOINT_DTYPE) -> paths[i], images spread over host threads."""
    L = load_library()
    n = len(paths)
    arrs = [np.ascontiguousarray(k, dtype=KEYPOINT_DTYPE) for k in key_arrays]
    res = (_Result * n)()
    for i, a in enumerate(arrs):
        res[i].count_hessian = len(a); res[i].count_desc = len(a); res[i].keys = a.ctypes.data
    cp = (C.c_char_p * n)(*[os.fsencode(p) for p in paths])
    rc = L.hesaff_write_sift_batch(n, cp, res, C.c_float(mr_size), threads)
    if rc != 0:
        raise HesaffError(rc, "hesaff_write_sift_batch")


def write_sift(path, keys, mr_size):
    keys = np.ascontiguousarray(keys, dtype=KEYPOINT_DTYPE)
    rc = load_library().hesaff_write_sift(os.fsencode(path), keys.ctypes.data, len(keys), mr_size)
    if rc != 0:
        raise HesaffError(rc, "hesaff_write_sift(%s)" % path)


BIN_ROW_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("a", "<f4"), ("b", "<f4"), ("c", "<f4"), ("desc", "u1", (128,))])


def write_bin(path, keys, mr_size):
    keys = np.ascontiguousarray(keys, dtype=KEYPOINT_DTYPE)
    rc = load_library().hesaff_write_bin(os.fsencode(path), keys.ctypes.data, len(keys), mr_size)
    if rc != 0:
        raise HesaffError(rc, "hesaff_write_bin(%s)" % path)


def read_bin(path):
    """.hesaff.bin (hesaff_write_bin) -> structured array of BIN_ROW_DTYPE."""
    with open(path, "rb") as f:
        head = f.read(16)
        if len(head) != 16 or head[:8] != b"HESAFFB1":
            raise HesaffError(-4, "%s is not a .hesaff.bin file" % path)
        dim, n = np.frombuffer(head[8:], "<u4")
        if dim != 128:
            raise HesaffError(-4, "descriptor dimension %d" % dim)
        rows = np.frombuffer(f.read(), dtype=BIN_ROW_DTYPE)
    if len(rows) != n:
        raise HesaffError(-4, "%s is truncated" % path)
    return rows


WORDS_ROW_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("a", "<f4"), ("b", "<f4"), ("c", "<f4"), ("word", "<u4")])


def _vocabulary_array(words):
    """uint8 [K, 128], C-contiguous, 1 <= K <= 2^20 - anything else is a ValueError"""
    if not isinstance(words, np.ndarray) or words.dtype != np.uint8 or words.ndim != 2 or words.shape[1] != 128:
        raise ValueError("a vocabulary is a uint8 array of shape [K, 128]")
    if not words.flags["C_CONTIGUOUS"]:
        raise ValueError("a vocabulary must be C-contiguous")
    if not 1 <= words.shape[0] <= (1 << 20):
        raise ValueError("a vocabulary has 1 .. 2^20 rows, not %d" % words.shape[0])
    return words


def write_vocabulary(path, words):
    """hesaff_write_vocabulary: uint8 [K, 128] -> a vocabulary file ("HESAFFV1")."""
    words = _vocabulary_array(words)
    rc = load_library().hesaff_write_vocabulary(os.fsencode(path), words.ctypes.data, words.shape[0])
    if rc != 0:
        raise HesaffError(rc, "hesaff_write_vocabulary(%s)" % path)


def read_vocabulary(path):
    """hesaff_read_vocabulary: a vocabulary file -> uint8 [K, 128]."""
    L = load_library()
    data = C.c_void_p(); k = C.c_int()
    rc = L.hesaff_read_vocabulary(os.fsencode(path), C.byref(data), C.byref(k))
    if rc != 0:
        raise HesaffError(rc, "hesaff_read_vocabulary(%s): not a readable, whole vocabulary file" % path)
    try:
        arr = np.frombuffer(C.string_at(data.value, k.value * 128), dtype=np.uint8).copy()
    finally:
        L.hesaff_free(data)
    return arr.reshape(k.value, 128)


def _cells_arrays(coarse, first):
    """(coarse uint8 [C, 128], first uint32 [C + 1]), C-contiguous - anything else is a ValueError; the rules of `first` are the library's"""
    coarse = _vocabulary_array(coarse)
    first = np.ascontiguousarray(first)
    if first.dtype.kind not in "iu" or first.shape != (coarse.shape[0] + 1,) or (first < 0).any() or (first > (1 << 20)).any():
        raise ValueError("first is an integer array of C + 1 = %d row indices" % (coarse.shape[0] + 1))
    return coarse, np.ascontiguousarray(first, dtype=np.uint32)


def write_vocabulary_cells(path, coarse, first):
    """hesaff_write_vocabulary_cells: coarse uint8 [C, 128], first [C + 1] -> a cells file ("HESAFFC1"), kept beside the vocabulary
    file of the same first[C] rows."""
    coarse, first = _cells_arrays(coarse, first)
    rc = load_library().hesaff_write_vocabulary_cells(os.fsencode(path), coarse.shape[0], coarse.ctypes.data, first.ctypes.data)
    if rc != 0:
        raise HesaffError(rc, "hesaff_write_vocabulary_cells(%s)" % path)


def read_vocabulary_cells(path):
    """hesaff_read_vocabulary_cells: a cells file -> (coarse uint8 [C, 128], first uint32 [C + 1]); first[C] is the number of rows."""
    L = load_library()
    coarse = C.c_void_p(); first = C.c_void_p(); c = C.c_int(); k = C.c_int()
    rc = L.hesaff_read_vocabulary_cells(os.fsencode(path), C.byref(coarse), C.byref(first), C.byref(c), C.byref(k))
    if rc != 0:
        raise HesaffError(rc, "hesaff_read_vocabulary_cells(%s): not a readable, whole cells file" % path)
    try:
        g = np.frombuffer(C.string_at(coarse.value, c.value * 128), dtype=np.uint8).copy()
        f = np.frombuffer(C.string_at(first.value, (c.value + 1) * 4), dtype="<u4").astype(np.uint32)
    finally:
        L.hesaff_free(coarse)
        L.hesaff_free(first)
    return g.reshape(c.value, 128), f


def write_words(path, keys, words, mr_size, vocabulary_size):
    """hesaff_write_words: keys[KEYPOINT_DTYPE] and their int32 [n, 2] (word, dist2) rows -> a words file ("HESAFFW1")."""
    keys = np.ascontiguousarray(keys, dtype=KEYPOINT_DTYPE)
    words = np.ascontiguousarray(words, dtype=np.int32).reshape(-1, 2)
    if len(words) != len(keys):
        raise ValueError("one (word, dist2) row per key")
    rc = load_library().hesaff_write_words(os.fsencode(path), keys.ctypes.data, words.ctypes.data, len(keys), mr_size, int(vocabulary_size))
    if rc != 0:
        raise HesaffError(rc, "hesaff_write_words(%s)" % path)


def read_words(path):
    """.hesaff.words (hesaff_write_words) -> (vocabulary_size, structured array of WORDS_ROW_DTYPE)."""
    with open(path, "rb") as f:
        head = f.read(16)
        if len(head) != 16 or head[:8] != b"HESAFFW1":
            raise HesaffError(-4, "%s is not a .hesaff.words file" % path)
        vocabulary_size, n = (int(v) for v in np.frombuffer(head[8:], "<u4"))
        body = f.read()
    if len(body) != n * WORDS_ROW_DTYPE.itemsize:
        raise HesaffError(-4, "%s is truncated" % path)
    return vocabulary_size, np.frombuffer(body, dtype=WORDS_ROW_DTYPE).copy()


def expand_rows(rows, neighbours, signatures=None):
    """The rows a words file holds under a neighbour count R > 1 (hesaff_set_vocabulary_neighbours), built in numpy: for every key in
    key order one row per present rank in ascending rank - the key's five floats, that rank's word; a rank with word -1 (fewer than R
    rows in the vocabulary) gives no row.  rows: WORDS_ROW_DTYPE [n], one per key (their word column is not read); neighbours:
    int32 [n, R, 2]; signatures: None, or uint64 [n, R], a signature per (key, rank).  -> the expanded rows, or (rows, signatures
    row for row with them): what query_index and verify_matches take."""
    rows = np.asarray(rows)
    if rows.dtype != WORDS_ROW_DTYPE or rows.ndim != 1:
        raise ValueError("rows are a 1-d array of WORDS_ROW_DTYPE (what read_words returns)")
    neighbours = np.asarray(neighbours, dtype=np.int32)
    if neighbours.ndim != 3 or neighbours.shape[0] != len(rows) or neighbours.shape[2] != 2:
        raise ValueError("neighbours are an int32 array of shape [n, R, 2], a row per row of `rows`")
    words = neighbours[:, :, 0]
    key, rank = np.nonzero(words >= 0)   # (row-major: key order, ascending rank within a key)
    out = rows[key].copy()
    out["word"] = words[key, rank].astype(np.uint32)
    if signatures is None:
        return out
    signatures = np.asarray(signatures, dtype=np.uint64)
    if signatures.shape != words.shape:
        raise ValueError("signatures are a uint64 array of shape [n, R], one per (key, rank)")
    return out, np.ascontiguousarray(signatures[key, rank])


EMBED_BITS = 64   # HESAFF_EMBED_BITS


def embedding_projection(seed):
    """The default projection of hesaff_embedding_projection in numpy: int8 [64, 128], entry e = i * 128 + j the e-th output of
    splitmix64 from `seed`, its top byte less 128, with -128 raised to -127."""
    with np.errstate(over="ignore"):
        s = np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) + np.arange(1, EMBED_BITS * 128 + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        x = (s ^ (s >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    v = (x >> np.uint64(56)).astype(np.int32) - 128
    return np.maximum(v, -127).astype(np.int8).reshape(EMBED_BITS, 128)


def _projection_array(P):
    """int8 [64, 128], C-contiguous, no entry -128 - anything else is a ValueError"""
    if not isinstance(P, np.ndarray) or P.dtype != np.int8 or P.shape != (EMBED_BITS, 128):
        raise ValueError("a projection is an int8 array of shape [64, 128]")
    if (P == -128).any():
        raise ValueError("a projection has entries in -127 .. 127")
    return np.ascontiguousarray(P)


def _thresholds_array(tau, k=None):
    """int32 [K, 64], C-contiguous"""
    if not isinstance(tau, np.ndarray) or tau.dtype != np.int32 or tau.ndim != 2 or tau.shape[1] != EMBED_BITS or (k is not None and tau.shape[0] != k):
        raise ValueError("thresholds are an int32 array of shape [K, 64]%s" % ("" if k is None else ", K = %d" % k))
    return np.ascontiguousarray(tau)


def _signature_array(sigs, n):
    sigs = np.ascontiguousarray(sigs, dtype=np.uint64)
    if sigs.shape != (n,):
        raise ValueError("one uint64 signature per key: shape [%d], not %s" % (n, sigs.shape))
    return sigs


def write_embedding(path, P, tau):
    """hesaff_write_embedding: P int8 [64, 128], tau int32 [K, 64] -> an embedding file ("HESAFFE1")."""
    P = _projection_array(P)
    tau = _thresholds_array(tau)
    rc = load_library().hesaff_write_embedding(os.fsencode(path), tau.shape[0], P.ctypes.data, tau.ctypes.data)
    if rc != 0:
        raise HesaffError(rc, "hesaff_write_embedding(%s)" % path)


def read_embedding(path):
    """hesaff_read_embedding: an embedding file -> (P int8 [64, 128], tau int32 [K, 64])."""
    L = load_library()
    P = C.c_void_p(); tau = C.c_void_p(); k = C.c_int()
    rc = L.hesaff_read_embedding(os.fsencode(path), C.byref(P), C.byref(tau), C.byref(k))
    if rc != 0:
        raise HesaffError(rc, "hesaff_read_embedding(%s): not a readable, whole embedding file" % path)
    try:
        p = np.frombuffer(C.string_at(P.value, EMBED_BITS * 128), dtype=np.int8).copy()
        t = np.frombuffer(C.string_at(tau.value, k.value * EMBED_BITS * 4), dtype="<i4").astype(np.int32)
    finally:
        L.hesaff_free(P)
        L.hesaff_free(tau)
    return p.reshape(EMBED_BITS, 128), t.reshape(k.value, EMBED_BITS)


def write_index_file(path, n_images, n_keys, df, postings, key_count=None, key_image=None, key_sig=None):
    """hesaff_write_index_file: an index file ("HESAFFI1") from host arrays - df uint32 [K], postings uint32 [n_postings, 2] = (image, tf)
    word-major, and for an embedded index key_count uint32 [K], key_image uint32 [n_keys], key_sig uint64 [n_keys]."""
    df = np.ascontiguousarray(df, dtype=np.uint32).reshape(-1)
    postings = np.ascontiguousarray(postings, dtype=np.uint32).reshape(-1, 2)
    embedded = key_count is not None
    kc = ki = ks = None
    if embedded:
        kc = np.ascontiguousarray(key_count, dtype=np.uint32).reshape(-1)
        ki = np.ascontiguousarray(key_image, dtype=np.uint32).reshape(-1)
        ks = np.ascontiguousarray(key_sig, dtype=np.uint64).reshape(-1)
        if len(kc) != len(df) or len(ki) != n_keys or len(ks) != n_keys:
            raise ValueError("key_count has K entries, key_image and key_sig n_keys")
    rc = load_library().hesaff_write_index_file(os.fsencode(path), int(embedded), len(df), int(n_images), int(n_keys), len(postings), df.ctypes.data,
                                                postings.ctypes.data if len(postings) else None, kc.ctypes.data if embedded else None,
                                                ki.ctypes.data if embedded and n_keys else None, ks.ctypes.data if embedded and n_keys else None)
    if rc != 0:
        raise HesaffError(rc, "hesaff_write_index_file(%s)" % path)


def read_index_file(path):
    """hesaff_read_index_file: an index file -> a dict of embedded, k, n_images, n_keys, n_postings, df, postings [n_postings, 2] and, for an
    embedded index, key_count, key_image, key_sig (None otherwise)."""
    L = load_library()
    e, k, n = C.c_int(), C.c_int(), C.c_int()
    t, p = C.c_int64(), C.c_int64()
    ptr = [C.c_void_p() for _ in range(5)]
    rc = L.hesaff_read_index_file(os.fsencode(path), C.byref(e), C.byref(k), C.byref(n), C.byref(t), C.byref(p), *[C.byref(q) for q in ptr])
    if rc != 0:
        raise HesaffError(rc, "hesaff_read_index_file(%s): not a readable, whole index file" % path)
    try:
        def take(q, count, dtype):
            return np.frombuffer(C.string_at(q.value, count * np.dtype(dtype).itemsize), dtype=dtype).copy() if count else np.zeros(0, dtype)
        out = dict(embedded=bool(e.value), k=k.value, n_images=n.value, n_keys=t.value, n_postings=p.value, df=take(ptr[0], k.value, np.uint32),
                   postings=take(ptr[1], 2 * p.value, np.uint32).reshape(-1, 2), key_count=None, key_image=None, key_sig=None)
        if e.value:
            out.update(key_count=take(ptr[2], k.value, np.uint32), key_image=take(ptr[3], t.value, np.uint32), key_sig=take(ptr[4], t.value, np.uint64))
    finally:
        for q in ptr:
            L.hesaff_free(q)
    return out


def write_signatures(path, sigs):
    """hesaff_write_signatures: uint64 [n] -> a signatures file ("HESAFFS1")."""
    sigs = np.ascontiguousarray(sigs, dtype=np.uint64).reshape(-1)
    rc = load_library().hesaff_write_signatures(os.fsencode(path), sigs.ctypes.data if len(sigs) else None, len(sigs))
    if rc != 0:
        raise HesaffError(rc, "hesaff_write_signatures(%s)" % path)


def read_signatures(path):
    """hesaff_read_signatures: a signatures file -> uint64 [n]."""
    L = load_library()
    p = C.c_void_p(); n = C.c_int()
    rc = L.hesaff_read_signatures(os.fsencode(path), C.byref(p), C.byref(n))
    if rc != 0:
        raise HesaffError(rc, "hesaff_read_signatures(%s): not a readable, whole signatures file" % path)
    try:
        out = np.frombuffer(C.string_at(p.value, n.value * 8), dtype="<u8").astype(np.uint64) if n.value else np.zeros(0, np.uint64)
    finally:
        L.hesaff_free(p)
    return out


def _verify_rows(rows):
    """the rows of an image (or of a query) for verification: a 1-d array of WORDS_ROW_DTYPE, C-contiguous"""
    if not isinstance(rows, np.ndarray) or rows.dtype != WORDS_ROW_DTYPE or rows.ndim != 1:
        raise ValueError("rows are a 1-d array of WORDS_ROW_DTYPE (what read_words returns)")
    return np.ascontiguousarray(rows)


def _live_rows(rows):
    """the LIVE rule of hesaff_verify_matches (include/hesaff_amd.h, step 1) on an array of WORDS_ROW_DTYPE -> bool [n]"""
    F = np.float32
    x, y, a, b, c = (rows[f].astype(F) for f in "xyabc")
    lo, hi = F(2.0 ** -20), F(2.0 ** 20)
    with np.errstate(all="ignore"):
        r = np.sqrt(c); q = b / r; t = a - q * q; p = np.sqrt(t)
        return (c > 0) & (t > 0) & (p >= lo) & (p <= hi) & (r >= lo) & (r <= hi) & (a <= F(2.0 ** 40)) & (np.abs(x) <= hi) & (np.abs(y) <= hi)


def _expand_roi(roi, rows):
    """the region of an expansion as float32 [4] = x0, y0, x1, y1; None: the bounding box of the query's live keys (zeros without one)"""
    if roi is None:
        if rows is None:
            raise ValueError("rows in device memory need a roi")
        k = rows[_live_rows(rows)]
        roi = (k["x"].min(), k["y"].min(), k["x"].max(), k["y"].max()) if len(k) else (0, 0, 0, 0)
    roi = np.ascontiguousarray(roi, dtype=np.float32)
    if roi.shape != (4,):
        raise ValueError("roi is (x0, y0, x1, y1)")
    return roi


def _expand_hypotheses(out, hyp, n_candidates):
    out = np.ascontiguousarray(out, dtype=np.int32); hyp = np.ascontiguousarray(hyp, dtype=np.float32)
    if out.shape != (n_candidates, 6) or hyp.shape != (n_candidates, 3):
        raise ValueError("out is int32 [R, 6] and hyp float32 [R, 3], as verify_matches returns them for the same candidates")
    return out, hyp


def _index_words(w):
    """an image's (or a query's) words for the index: int32 [n] or (word, dist2) rows [n, 2], C-contiguous"""
    if not isinstance(w, np.ndarray) or w.dtype != np.int32 or not (w.ndim == 1 or (w.ndim == 2 and w.shape[1] == 2)):
        raise ValueError("words are an int32 array of shape [n] or [n, 2]")
    return np.ascontiguousarray(w)


def _index_stride(arrays):
    kinds = {a.ndim for a in arrays}
    if len(kinds) > 1:
        raise ValueError("the word arrays are all [n] or all [n, 2]")
    return 2 if kinds == {2} else 1


def read_image(path):
    """PGM/PPM or PNG by magic number -> uint8 array HxW (grey) or HxWx3."""
    return read_pnm(path, _fn="hesaff_read_image")


def read_jpeg_coefficients(path):
    """The host half of the JPEG reader (entropy decoding only) -> (JpegLayout, blob as a uint8 array)."""
    L = load_library()
    lay = JpegLayout(); blob = C.c_void_p(); nb = C.c_size_t()
    rc = L.hesaff_read_jpeg_coefficients(os.fsencode(path), C.byref(lay), C.byref(blob), C.byref(nb))
    if rc != 0:
        raise HesaffError(rc, "hesaff_read_jpeg_coefficients(%s)" % path)
    try:
        arr = np.frombuffer(C.string_at(blob.value, nb.value), dtype=np.uint8).copy()
    finally:
        L.hesaff_free(blob)
    return lay, arr


def read_pnm(path, _fn="hesaff_read_pnm"):
    L = load_library()
    data = C.c_void_p(); w = C.c_int(); h = C.c_int(); ch = C.c_int()
    rc = getattr(L, _fn)(os.fsencode(path), C.byref(data), C.byref(w), C.byref(h), C.byref(ch))
    if rc != 0:
        raise HesaffError(rc, "%s(%s)" % (_fn, path))
    try:
        n = w.value * h.value * ch.value
        arr = np.frombuffer(C.string_at(data.value, n), dtype=np.uint8).copy()
    finally:
        L.hesaff_free(data)
    return arr.reshape((h.value, w.value) if ch.value == 1 else (h.value, w.value, 3))


class HesaffContext:
    """One device context (hesaff_create / hesaff_destroy)."""

    def __init__(self, params=None, device=0):
        self.L = load_library()
        self.params = params if params is not None else default_params()
        self.device = int(device)   # HIP device ordinal = torch's cuda index (detect_batch_device_f32 checks its tensor against it)
        self.h = C.c_void_p()
        rc = self.L.hesaff_create(C.byref(self.h), C.byref(self.params), device)
        if rc != 0:
            raise HesaffError(rc, self.L.hesaff_last_error(None).decode())

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self.L.hesaff_destroy(self.h)
            self.h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise HesaffError(rc, self.L.hesaff_last_error(self.h).decode())

    # ---- whole path ----
    def _arm_masks(self, masks, imgs):
        """hesaff_set_next_masks for the call that follows: masks is None (nothing armed) or a list with, per image, None or an H x W
        uint8 / bool array (non-zero: detect here; any positive row stride with unit pixel stride is passed as it is).  -> the arrays,
        which the caller keeps alive across the detecting call: the library copies the pointers, not the pixels."""
        if masks is None:
            return None
        if len(masks) != len(imgs):
            raise ValueError("masks: one entry (an array or None) per image (%d images, %d masks)" % (len(imgs), len(masks)))
        keep = []
        for i, (m, im) in enumerate(zip(masks, imgs)):
            if m is None:
                keep.append(None)
                continue
            m = np.asarray(m)
            if m.dtype == np.bool_:
                m = m.view(np.uint8)
            if m.dtype != np.uint8 or m.ndim != 2 or m.shape != tuple(im.shape[:2]):
                raise ValueError("mask %d: an H x W uint8 or bool array of the image's size %s is expected, got %s %s"
                                 % (i, tuple(im.shape[:2]), m.dtype, m.shape))
            if (m.shape[1] > 1 and m.strides[1] != 1) or (m.shape[0] > 1 and m.strides[0] < m.shape[1]):
                m = np.ascontiguousarray(m)
            keep.append(m)
        n = len(keep)
        ptrs = (C.c_void_p * n)(*[None if m is None else m.ctypes.data for m in keep])
        st = (C.c_int * n)(*[0 if m is None else (m.strides[0] if m.shape[0] > 1 else m.shape[1]) for m in keep])
        self._check(self.L.hesaff_set_next_masks(self.h, n, ptrs, st))
        return keep

    def detect_batch(self, images, masks=None):
        """images: list of uint8 arrays HxW (grey) or HxWx3.  -> list of (count_hessian, keys[KEYPOINT_DTYPE]).
        masks (here and in the other detect_* methods): per-image detection masks for this call (hesaff_set_next_masks): a list
        with, per image, None or an H x W uint8 / bool array; keypoints whose pixel is zero are dropped on the device."""
        imgs, n, ptrs, ws, hs, st, chs = self._u8_list(images)
        keep = self._arm_masks(masks, imgs)  # noqa: F841  (alive until the call has returned)
        res = (_Result * n)()
        self._check(self.L.hesaff_detect_batch(self.h, n, ptrs, ws, hs, st, chs, res))
        # one copy out of the library-owned (pinned) result buffer, valid until the next call
        return [(r.count_hessian, self._keys_at(r.keys, r.count_desc)) for r in res]

    def detect_regions(self, images, masks=None):
        """hesaff_detect_regions: images as for detect_batch.  -> list of (regions[REGION_DTYPE], keys[KEYPOINT_DTYPE]) per image:
        one record per Hessian keypoint in the reference's callback order (pyramid.h:43-47, affine.h:48-58), and the same keys as
        detect_batch.  regions[i]["key"] is the row of keys that keypoint became (-1 when it got no descriptor)."""
        imgs, n, ptrs, ws, hs, st, chs = self._u8_list(images)
        keep = self._arm_masks(masks, imgs)  # noqa: F841
        res = (_RegionResult * n)()
        self._check(self.L.hesaff_detect_regions(self.h, n, ptrs, ws, hs, st, chs, res))
        # copies out of the library-owned (pinned) result buffer, valid until the next call
        return [(self._regions_at(r.regions, r.count_hessian), self._keys_at(r.keys, r.count_desc)) for r in res]

    @staticmethod
    def _region_lists(regions, n):
        """one REGION_DTYPE array per image -> (arrays, pointers, counts)"""
        if len(regions) != n:
            raise ValueError("describe_regions takes one record array per image (%d images, %d arrays)" % (n, len(regions)))
        recs = [np.ascontiguousarray(r, dtype=REGION_DTYPE).reshape(-1) for r in regions]
        ptrs = (C.c_void_p * n)(*[r.ctypes.data if r.size else None for r in recs])
        counts = (C.c_int * n)(*[r.size for r in recs])
        return recs, ptrs, counts

    def describe_regions(self, images, regions, from_):
        """hesaff_describe_regions: the rest of the chain for the caller's records.  images as for detect_batch; regions: one
        REGION_DTYPE array per image (what detect_regions returned, whole, filtered or reordered, or keypoints of the caller's own);
        from_: FROM_POINTS (findAffineShape on the plane (octave, level), then rectify / normalizeAffine / SIFT) or FROM_SHAPES
        (a11..a22 given: rectify / normalizeAffine / SIFT only).  -> what detect_regions returns, records and keys in the caller's order."""
        imgs, n, ptrs, ws, hs, st, chs = self._u8_list(images)
        recs, rptrs, counts = self._region_lists(regions, n)
        res = (_RegionResult * n)()
        self._check(self.L.hesaff_describe_regions(self.h, n, ptrs, ws, hs, st, chs, rptrs, counts, int(from_), res))
        return [(self._regions_at(r.regions, r.count_hessian), self._keys_at(r.keys, r.count_desc)) for r in res]

    def describe_regions_f32(self, images, regions, from_):
        """hesaff_describe_regions_f32: describe_regions for 2-D float32 grey planes."""
        imgs, ptrs, ws, hs, st = self._f32_list(images)
        recs, rptrs, counts = self._region_lists(regions, len(imgs))
        res = (_RegionResult * len(imgs))()
        self._check(self.L.hesaff_describe_regions_f32(self.h, len(imgs), ptrs, ws, hs, st, rptrs, counts, int(from_), res))
        return [(self._regions_at(r.regions, r.count_hessian), self._keys_at(r.keys, r.count_desc)) for r in res]

    @staticmethod
    def _u8_list(images):
        """arrays HxW (grey) or HxWx3, cast to uint8 -> (arrays, n, ptrs, widths, heights, strides, channels)"""
        n = len(images)
        imgs = [np.ascontiguousarray(im, dtype=np.uint8) for im in images]
        ptrs = (C.c_void_p * n)(*[im.ctypes.data for im in imgs])
        ws = (C.c_int * n)(*[im.shape[1] for im in imgs])
        hs = (C.c_int * n)(*[im.shape[0] for im in imgs])
        chs = (C.c_int * n)(*[1 if im.ndim == 2 else 3 for im in imgs])
        st = (C.c_int * n)(*[im.shape[1] * (1 if im.ndim == 2 else 3) for im in imgs])
        return imgs, n, ptrs, ws, hs, st, chs

    # ---- float grey planes (CV_32FC1, pyramid.h:73) ----
    @staticmethod
    def _f32_list(images):
        """2-D float32 arrays -> (arrays, ptrs, widths, heights, strides); no cast: any other dtype or shape is a TypeError."""
        for i, im in enumerate(images):
            if not isinstance(im, np.ndarray) or im.dtype != np.float32 or im.ndim != 2:
                raise TypeError("image %d: the _f32 methods take 2-D float32 arrays, got %s" % (
                    i, "%s %s" % (im.dtype, im.shape) if isinstance(im, np.ndarray) else type(im).__name__))
        imgs = []
        for im in images:
            if im.strides[1] != 4 or im.strides[0] < 4 * im.shape[1] or im.strides[0] % 4:
                im = np.ascontiguousarray(im)   # (same dtype: a layout copy, not a cast)
            imgs.append(im)
        n = len(imgs)
        ptrs = (C.c_void_p * n)(*[im.ctypes.data for im in imgs])
        ws = (C.c_int * n)(*[im.shape[1] for im in imgs])
        hs = (C.c_int * n)(*[im.shape[0] for im in imgs])
        st = (C.c_int * n)(*[im.strides[0] for im in imgs])
        return imgs, ptrs, ws, hs, st

    def detect_batch_f32(self, images, masks=None):
        """hesaff_detect_batch_f32: 2-D float32 grey planes (padded rows allowed) -> list of (count_hessian, keys[KEYPOINT_DTYPE])."""
        imgs, ptrs, ws, hs, st = self._f32_list(images)
        keep = self._arm_masks(masks, imgs)  # noqa: F841
        res = (_Result * len(imgs))()
        self._check(self.L.hesaff_detect_batch_f32(self.h, len(imgs), ptrs, ws, hs, st, res))
        return [(r.count_hessian, self._keys_at(r.keys, r.count_desc)) for r in res]

    def detect_regions_f32(self, images, masks=None):
        """hesaff_detect_regions_f32: detect_regions for 2-D float32 grey planes."""
        imgs, ptrs, ws, hs, st = self._f32_list(images)
        keep = self._arm_masks(masks, imgs)  # noqa: F841
        res = (_RegionResult * len(imgs))()
        self._check(self.L.hesaff_detect_regions_f32(self.h, len(imgs), ptrs, ws, hs, st, res))
        return [(self._regions_at(r.regions, r.count_hessian), self._keys_at(r.keys, r.count_desc)) for r in res]

    def detect_batch_cb_f32(self, images, sink, masks=None):
        """hesaff_detect_batch_cb_f32: detect_batch_cb for 2-D float32 grey planes."""
        imgs, ptrs, ws, hs, st = self._f32_list(images)
        keep = self._arm_masks(masks, imgs)  # noqa: F841
        self._check(self.L.hesaff_detect_batch_cb_f32(self.h, len(imgs), ptrs, ws, hs, st, self._chunk_sink(sink), None))

    def set_next_masks_device(self, masks_ptr, n, row_stride=0, img_stride=0):
        """hesaff_set_next_masks_device: n mask planes in device memory (raw device pointer) for the next device-resident call;
        strides in bytes, 0 = tightly packed.  masks_ptr None or n = 0 disarms."""
        if masks_ptr is None:
            n = 0
        self._check(self.L.hesaff_set_next_masks_device(self.h, int(n), C.c_void_p(masks_ptr), int(row_stride), int(img_stride)))

    def detect_batch_device_f32(self, t, masks_ptr=None, mask_row_stride=0, mask_img_stride=0):
        """hesaff_detect_batch_device_f32 on a torch tensor on this context's device: float32, [n, H, W] or [H, W], unit stride
        along W, any positive row and image stride.  A tensor that repeats images or rows through a zero stride (expand, broadcast)
        is made contiguous first: the C entry point reads a stride of 0 as "tightly packed".  torch's current stream on that device
        is synchronised before the call.  masks_ptr: n uint8 mask planes [n, H, W] in device memory (raw device pointer, complete
        before the call; strides in bytes, 0 = tightly packed), armed for this call.
        -> (count_hessian[n], count_desc[n], d_keys, total) as detect_batch_device returns them."""
        import torch
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() not in (2, 3):
            raise TypeError("detect_batch_device_f32 takes a float32 torch tensor [n, H, W] or [H, W]")
        if t.dim() == 2:
            t = t.unsqueeze(0)
        if t.device.type != "cuda":
            raise ValueError("detect_batch_device_f32: the tensor is not in device memory")
        if t.device.index != self.device:
            raise ValueError("detect_batch_device_f32: the tensor is on %s, this context on cuda:%d" % (t.device, self.device))
        if t.stride(2) != 1 and t.shape[2] > 1:
            raise ValueError("detect_batch_device_f32: the tensor needs unit stride along W")
        n, H, W = t.shape
        if (n > 1 and t.stride(0) == 0) or (H > 1 and t.stride(1) == 0):
            t = t.contiguous()   # (on torch's current stream, which is synchronised below)
        torch.cuda.current_stream(t.device).synchronize()
        ch = np.zeros(n, np.int32); cd = np.zeros(n, np.int32)
        dk = C.c_void_p(); tot = C.c_int64()
        row, img = t.stride(1) * 4, t.stride(0) * 4
        if H == 1:
            row = 0   # (the stride of a single row is never used: tightly packed)
        if n == 1:
            img = 0
        if masks_ptr is not None:
            self.set_next_masks_device(masks_ptr, n, mask_row_stride, mask_img_stride)
        self._check(self.L.hesaff_detect_batch_device_f32(self.h, n, C.c_void_p(t.data_ptr()), W, H, row, img, ch, cd, C.byref(dk),
                                                          C.byref(tot)))
        return ch, cd, dk.value, tot.value

    def pyramid_f32(self, img):
        """hesaff_stage_pyramid_f32: pyramid() for a 2-D float32 grey plane."""
        if not isinstance(img, np.ndarray) or img.dtype != np.float32 or img.ndim != 2:
            raise TypeError("pyramid_f32 takes a 2-D float32 array")
        g = np.ascontiguousarray(img)
        return self._pyramid(self.L.hesaff_stage_pyramid_f32, g)

    @staticmethod
    def _records_at(addr, count, dtype):
        """a copy of `count` records at a library-owned address"""
        if count <= 0:
            return np.zeros(0, dtype)
        return np.frombuffer((C.c_char * (count * dtype.itemsize)).from_address(addr), dtype=dtype).copy()

    @classmethod
    def _keys_at(cls, addr, count):
        return cls._records_at(addr, count, KEYPOINT_DTYPE)

    @classmethod
    def _regions_at(cls, addr, count):
        return cls._records_at(addr, count, REGION_DTYPE)

    def _chunk_sink(self, sink):
        """the hesaff_chunk_sink that hands a chunk's image indices and copies of its records to sink(indices, [(count_hessian, keys), ...])"""
        def _sink(_user, m, idx, res):
            out = [(res[i].count_hessian, self._keys_at(res[i].keys, res[i].count_desc)) for i in range(m)]
            return 1 if sink([idx[i] for i in range(m)], out) else 0
        return CHUNK_SINK(_sink)

    def detect_batch_raw(self, images):
        """hesaff_detect_batch without copying the records out: -> ctypes array of hesaff_result whose `keys` point into
        library-owned pinned memory (valid until the next call on this context)."""
        imgs, n, ptrs, ws, hs, st, chs = self._u8_list(images)
        res = (_Result * n)()
        self._check(self.L.hesaff_detect_batch(self.h, n, ptrs, ws, hs, st, chs, res))
        return res

    def detect_batch_cb(self, images, sink, masks=None):
        """hesaff_detect_batch_cb: sink(image_indices, [(count_hessian, keys copy), ...]) is called once per chunk with
        records that are valid only during the call (bounded pinned memory); a truthy return value stops the run."""
        imgs, n, ptrs, ws, hs, st, chs = self._u8_list(images)
        keep = self._arm_masks(masks, imgs)  # noqa: F841
        self._check(self.L.hesaff_detect_batch_cb(self.h, n, ptrs, ws, hs, st, chs, self._chunk_sink(sink), None))

    def set_output_format(self, fmt):
        """OUT_TEXT = 1 (.hesaff.sift, default), OUT_BIN = 2 (binary sidecar .hesaff.bin), OUT_WORDS = 4 (.hesaff.words, with a
        vocabulary set), or-ed as wanted."""
        self._check(self.L.hesaff_set_output_format(self.h, fmt))

    def set_resume(self, on=True, strict=False):
        """hesaff_process_files skips images whose complete output exists (strict: the rows of an existing text file are counted too)."""
        self._check(self.L.hesaff_set_resume(self.h, (2 if strict else 1) if on else 0))

    def set_pinned_read_budget(self, max_bytes, keep_bytes):
        """page-locked read buffers of process_files: at most max_bytes at any time, keep_bytes kept from call to call"""
        self._check(self.L.hesaff_set_pinned_read_budget(self.h, max_bytes, keep_bytes))

    def set_pool_priority(self, mode):
        """-1: the pool of process_files steps down (nice 10) when the host plan is CPU-starved (default); 0 never; 1 always"""
        self._check(self.L.hesaff_set_pool_priority(self.h, mode))

    def set_keypoint_limit(self, n):
        """hesaff_set_keypoint_limit: every detecting call keeps, per image, the n Hessian keypoints of greatest |response| (ties at
        the cut to the earlier one), in the reference's order; 0 = no limit (default).  n bounds Hessian keypoints, not descriptors.
        describe_regions* and the stage operators are not limited."""
        self._check(self.L.hesaff_set_keypoint_limit(self.h, int(n)))

    @property
    def keypoint_limit(self):
        n = C.c_int()
        self._check(self.L.hesaff_get_keypoint_limit(self.h, C.byref(n)))
        return n.value

    @keypoint_limit.setter
    def keypoint_limit(self, n):
        self.set_keypoint_limit(n)

    def set_keypoint_grid(self, rows, cols):
        """hesaff_set_keypoint_grid: with a keypoint limit n, every detecting call keeps the n // (rows * cols) strongest Hessian
        keypoints of every cell of a rows x cols grid over the image (OpenCV's GridAdaptedFeatureDetector; the rule in
        include/hesaff_amd.h), in the reference's order; (1, 1) = no grid (default).  rows * cols <= 64, and not more cells than a
        set limit."""
        self._check(self.L.hesaff_set_keypoint_grid(self.h, int(rows), int(cols)))

    @property
    def keypoint_grid(self):
        r, c = C.c_int(), C.c_int()
        self._check(self.L.hesaff_get_keypoint_grid(self.h, C.byref(r), C.byref(c)))
        return r.value, c.value

    @keypoint_grid.setter
    def keypoint_grid(self, rows_cols):
        self.set_keypoint_grid(*rows_cols)

    def set_orientation(self, mode):
        """hesaff_set_orientation: ORI_UP / "up" (default: the reference's upright frame, bit for bit) or ORI_DOMINANT / "dominant":
        every keypoint's frame is turned by the dominant gradient angle of its patch before it is described, so descriptors follow
        an in-plane rotation of the image (one orientation per keypoint; definition in include/hesaff_amd.h).  Applies to every
        detecting call, process_files and describe_regions*; not to the stage operators."""
        if isinstance(mode, str):
            if mode not in _ORI_NAMES:
                raise ValueError("orientation is 'up' or 'dominant', not %r" % (mode,))
            mode = _ORI_NAMES[mode]
        self._check(self.L.hesaff_set_orientation(self.h, int(mode)))

    @property
    def orientation(self):
        """The mode, an int (ORI_UP / ORI_DOMINANT) - and, called with patches, the stage operator: ctx.orientation(patches) is
        ctx.orientation_of(patches)."""
        m = C.c_int()
        self._check(self.L.hesaff_get_orientation(self.h, C.byref(m)))
        return _OrientationMode(m.value, self)

    @orientation.setter
    def orientation(self, mode):
        self.set_orientation(mode)

    def set_orientation_count(self, k):
        """hesaff_set_orientation_count: up to k keys per region, k in 1..4 (default 1), one per peak of the orientation histogram
        within 80 % of the highest (definition in include/hesaff_amd.h).  Read in ORI_DOMINANT only; inert in ORI_UP.  With k > 1 a
        region's keys are adjacent rows in ascending rank, REGION_DTYPE's `key` is the first and `reserved` their number, and an image
        may have more keys than Hessian keypoints."""
        self._check(self.L.hesaff_set_orientation_count(self.h, int(k)))

    @property
    def orientation_count(self):
        k = C.c_int(0)
        self._check(self.L.hesaff_get_orientation_count(self.h, C.byref(k)))
        return k.value

    @orientation_count.setter
    def orientation_count(self, k):
        self.set_orientation_count(k)

    def set_descriptor(self, mode):
        """hesaff_set_descriptor: DESC_SIFT / "sift" (default: the reference's bytes, bit for bit) or DESC_ROOTSIFT / "rootsift": the
        descriptor vector is L1-normalised and square-rooted on the device before it is quantised (definition in
        include/hesaff_amd.h); only `desc` of the keys changes.  Applies to every detecting call, process_files and
        describe_regions*; not to the stage operators."""
        if isinstance(mode, str):
            if mode not in _DESC_NAMES:
                raise ValueError("descriptor is 'sift' or 'rootsift', not %r" % (mode,))
            mode = _DESC_NAMES[mode]
        self._check(self.L.hesaff_set_descriptor(self.h, int(mode)))

    @property
    def descriptor(self):
        m = C.c_int()
        self._check(self.L.hesaff_get_descriptor(self.h, C.byref(m)))
        return m.value

    @descriptor.setter
    def descriptor(self, mode):
        self.set_descriptor(mode)

    # ---- visual words (hesaff_set_vocabulary, include/hesaff_amd.h) ----
    def set_vocabulary(self, words):
        """hesaff_set_vocabulary: words is a C-contiguous uint8 [K, 128] array (copied to the device) or None (no vocabulary, the
        default).  With one set, every call that produces keys also assigns each key the lowest row of least squared distance to
        its descriptor bytes; words(image) hands them out."""
        if words is None:
            self._check(self.L.hesaff_set_vocabulary(self.h, 0, None))
            return
        words = _vocabulary_array(words)
        self._check(self.L.hesaff_set_vocabulary(self.h, words.shape[0], words.ctypes.data))

    @property
    def vocabulary_size(self):
        k = C.c_int()
        self._check(self.L.hesaff_get_vocabulary_size(self.h, C.byref(k)))
        return k.value

    def words(self, image):
        """hesaff_get_words: int32 [count, 2] = (word, dist2), row for row the keys of image `image` of the last host call (a copy)."""
        p = C.c_void_p(); n = C.c_int()
        if self.L.hesaff_get_words(self.h, int(image), C.byref(p), C.byref(n)) != 0:
            raise HesaffError(-1, "hesaff_get_words(%d): no vocabulary is set, or no such image in the last host call" % image)
        if n.value == 0:
            return np.zeros((0, 2), np.int32)
        return np.frombuffer((C.c_char * (n.value * 8)).from_address(p.value), dtype=np.int32).copy().reshape(n.value, 2)

    def assign_words(self, desc):
        """hesaff_stage_assign_words: desc uint8 [n, 128] -> int32 [n, 2] = (word, dist2) against the context's vocabulary."""
        desc = np.ascontiguousarray(desc, dtype=np.uint8)
        if desc.ndim != 2 or desc.shape[1] != 128:
            raise ValueError("descriptors are a uint8 array of shape [n, 128]")
        out = np.zeros((desc.shape[0], 2), np.int32)
        rc = self.L.hesaff_stage_assign_words(self.h, desc.shape[0], desc.ctypes.data if desc.shape[0] else None,
                                              out.ctypes.data if desc.shape[0] else None)
        if rc != 0 and desc.shape[0] == 0:
            raise HesaffError(rc, "hesaff_stage_assign_words: no vocabulary is set")
        self._check(rc)
        return out

    def assign_words_device(self, ptr, n, stride, offset, out_ptr):
        """hesaff_assign_words_device: n descriptors in device memory, descriptor i at ptr + i * stride + offset (164 / 36: a key array;
        128 / 0: a packed tensor) -> n x 2 int32 at out_ptr (raw device pointers)."""
        self._check(self.L.hesaff_assign_words_device(self.h, int(n), C.c_void_p(ptr), int(stride), int(offset), C.c_void_p(out_ptr)))

    def words_device(self):
        """hesaff_get_words_device: (device pointer, rows) of the int32 [total, 2] array parallel to the keys of the last device-resident call."""
        p = C.c_void_p(); tot = C.c_int64()
        if self.L.hesaff_get_words_device(self.h, C.byref(p), C.byref(tot)) != 0:
            raise HesaffError(-1, "hesaff_get_words_device: no vocabulary is set, or the last call was not device-resident")
        return p.value, tot.value

    @property
    def assign_ms(self):
        """HIP-event time of the last batch's word assignment (profiling level >= 1), in ms"""
        ms = C.c_float()
        self._check(self.L.hesaff_get_assign_ms(self.h, C.byref(ms)))
        return ms.value

    # ---- vocabulary neighbours (hesaff_set_vocabulary_neighbours, include/hesaff_amd.h) ----
    def set_vocabulary_neighbours(self, neighbours):
        """hesaff_set_vocabulary_neighbours: every key's R nearest rows of the vocabulary, not just the nearest (1..8, default 1).  With
        R > 1 every call that assigns words also leaves neighbours(image), int32 [n, R, 2]; words(image) stays rank 0, byte for byte.
        Does not combine with a cell layer."""
        self._check(self.L.hesaff_set_vocabulary_neighbours(self.h, int(neighbours)))

    def vocabulary_neighbours(self):
        """hesaff_get_vocabulary_neighbours: the neighbour count that is set"""
        r = C.c_int()
        self._check(self.L.hesaff_get_vocabulary_neighbours(self.h, C.byref(r)))
        return r.value

    def neighbours(self, image):
        """hesaff_get_neighbours: int32 [count, R, 2] = (word, dist2) per rank, row for row the keys of image `image` of the last host
        call (a copy); a rank the vocabulary is too small for is (-1, 2^31 - 1)."""
        p = C.c_void_p(); n = C.c_int(); r = C.c_int()
        if self.L.hesaff_get_neighbours(self.h, int(image), C.byref(p), C.byref(n), C.byref(r)) != 0:
            raise HesaffError(-1, "hesaff_get_neighbours(%d): no vocabulary is set, or no such image in the last host call" % image)
        if n.value == 0:
            return np.zeros((0, r.value, 2), np.int32)
        return np.frombuffer((C.c_char * (n.value * r.value * 8)).from_address(p.value), dtype=np.int32).copy().reshape(n.value, r.value, 2)

    def assign_neighbours(self, desc):
        """hesaff_stage_assign_neighbours: desc uint8 [n, 128] -> int32 [n, R, 2] with the context's R (1 as well)."""
        desc = np.ascontiguousarray(desc, dtype=np.uint8)
        if desc.ndim != 2 or desc.shape[1] != 128:
            raise ValueError("descriptors are a uint8 array of shape [n, 128]")
        out = np.zeros((desc.shape[0], self.vocabulary_neighbours(), 2), np.int32)
        rc = self.L.hesaff_stage_assign_neighbours(self.h, desc.shape[0], desc.ctypes.data if desc.shape[0] else None,
                                                   out.ctypes.data if desc.shape[0] else None)
        if rc != 0 and desc.shape[0] == 0:
            raise HesaffError(rc, "hesaff_stage_assign_neighbours: no vocabulary is set")
        self._check(rc)
        return out

    def assign_neighbours_device(self, ptr, n, stride, offset, out_ptr):
        """hesaff_assign_neighbours_device: n descriptors in device memory, addressed as in assign_words_device -> n x R x 2 int32 at
        out_ptr (raw device pointers)."""
        self._check(self.L.hesaff_assign_neighbours_device(self.h, int(n), C.c_void_p(ptr), int(stride), int(offset), C.c_void_p(out_ptr)))

    def neighbours_device(self):
        """hesaff_get_neighbours_device: (device pointer, rows, R) of the int32 [total, R, 2] array the last assignment left."""
        p = C.c_void_p(); tot = C.c_int64(); r = C.c_int()
        if self.L.hesaff_get_neighbours_device(self.h, C.byref(p), C.byref(tot), C.byref(r)) != 0:
            raise HesaffError(-1, "hesaff_get_neighbours_device: no vocabulary is set, or no assignment on the device was the last call")
        return p.value, tot.value, r.value

    # ---- vocabulary training (hesaff_train_vocabulary, include/hesaff_amd.h) ----
    def _train(self, call, k, iterations, init):
        k, iterations = int(k), int(iterations)
        if init is not None:
            init = _vocabulary_array(init)
            if init.shape[0] != k:
                raise ValueError("init has %d rows, k is %d" % (init.shape[0], k))
        words = np.zeros((max(k, 0), 128), np.uint8)
        distortion = np.zeros(max(iterations, 0), np.int64)
        empty = np.zeros(max(iterations, 0), np.int32)
        done = C.c_int(0)
        self._check(call(k, init.ctypes.data if init is not None else None, iterations, words.ctypes.data, distortion.ctypes.data,
                         empty.ctypes.data, C.byref(done)))
        return words, distortion[:done.value].copy(), empty[:done.value].copy()

    def train_vocabulary(self, desc, k, iterations, init=None):
        """hesaff_train_vocabulary: exact integer k-means over desc uint8 [n, 128] -> (words uint8 [k, 128], distortion int64 [done],
        empty int32 [done]); done <= iterations is the number of iterations that ran (fewer: a fixed point was reached).  init: the
        initial vocabulary uint8 [k, 128], or None for row r = desc[r * n // k].  The context's own vocabulary is not touched."""
        if not isinstance(desc, np.ndarray) or desc.dtype != np.uint8 or desc.ndim != 2 or desc.shape[1] != 128:
            raise ValueError("descriptors are a uint8 array of shape [n, 128]")
        desc = np.ascontiguousarray(desc)
        n = desc.shape[0]
        return self._train(lambda *a: self.L.hesaff_train_vocabulary(self.h, n, desc.ctypes.data if n else None, *a), k, iterations, init)

    def train_vocabulary_device(self, ptr, n, stride, offset, k, iterations, init=None):
        """hesaff_train_vocabulary_device: the same on n descriptors in device memory, descriptor i at ptr + i * stride + offset
        (164 / 36: a key array; 128 / 0: a packed tensor; a raw device pointer)."""
        return self._train(lambda *a: self.L.hesaff_train_vocabulary_device(self.h, int(n), C.c_void_p(ptr), int(stride), int(offset), *a),
                           k, iterations, init)

    def accumulate_words(self, desc, words, k):
        """hesaff_stage_accumulate_words: desc uint8 [n, 128], words int32 [n] in 0 .. k - 1 -> (sums uint32 [k, 128], counts uint32 [k])."""
        desc = np.ascontiguousarray(desc, dtype=np.uint8)
        words = np.ascontiguousarray(words, dtype=np.int32)
        if desc.ndim != 2 or desc.shape[1] != 128 or words.shape != (desc.shape[0],):
            raise ValueError("descriptors are uint8 [n, 128], words int32 [n]")
        k = int(k)
        sums = np.zeros((max(k, 0), 128), np.uint32)
        counts = np.zeros(max(k, 0), np.uint32)
        n = desc.shape[0]
        self._check(self.L.hesaff_stage_accumulate_words(self.h, n, desc.ctypes.data if n else None, words.ctypes.data if n else None, k,
                                                         sums.ctypes.data, counts.ctypes.data))
        return sums, counts

    @property
    def training_ms(self):
        """HIP-event times (assignment, accumulation, update) of the last training call, summed over its iterations (profiling >= 1), in ms"""
        a, b, u = C.c_float(), C.c_float(), C.c_float()
        self._check(self.L.hesaff_get_training_ms(self.h, C.byref(a), C.byref(b), C.byref(u)))
        return a.value, b.value, u.value

    # ---- vocabulary cells (hesaff_set_vocabulary_cells, include/hesaff_amd.h) ----
    def set_vocabulary_cells(self, coarse, first=None):
        """hesaff_set_vocabulary_cells: coarse uint8 [C, 128] and first [C + 1] (first[0] = 0, first[C] = K, strictly increasing: cell c
        owns rows first[c] .. first[c + 1] - 1 of the vocabulary that is set), or None to remove the layer.  With a layer every
        assignment takes the lowest nearest coarse row, then the lowest nearest row of that cell."""
        if coarse is None:
            self._check(self.L.hesaff_set_vocabulary_cells(self.h, 0, None, None))
            return
        coarse, first = _cells_arrays(coarse, first)
        self._check(self.L.hesaff_set_vocabulary_cells(self.h, coarse.shape[0], coarse.ctypes.data, first.ctypes.data))

    def vocabulary_cells(self):
        """hesaff_get_vocabulary_cells: the number of cells of the layer that is set, 0 without one"""
        c = C.c_int()
        self._check(self.L.hesaff_get_vocabulary_cells(self.h, C.byref(c)))
        return c.value

    def set_vocabulary_probes(self, probes):
        """hesaff_set_vocabulary_probes: with a cell layer set, search a key's `probes` nearest cells (1..8, default 1 = its one cell;
        at least as many as the layer has cells = the flat assignment).  A context setting: set_vocabulary and set_vocabulary_cells
        keep it, and without a layer it has no effect."""
        self._check(self.L.hesaff_set_vocabulary_probes(self.h, int(probes)))

    def vocabulary_probes(self):
        """hesaff_get_vocabulary_probes: the probe count that is set"""
        p = C.c_int()
        self._check(self.L.hesaff_get_vocabulary_probes(self.h, C.byref(p)))
        return p.value

    def probe_cells(self, desc):
        """hesaff_stage_probe_cells: desc uint8 [n, 128] -> (cells int32 [n, P'], dist2 int32 [n, P']), the P' = min(probes, cells)
        nearest cells of every key through the layer that is set, nearest first, equal distances in ascending cell."""
        desc = np.ascontiguousarray(desc, dtype=np.uint8)
        if desc.ndim != 2 or desc.shape[1] != 128:
            raise ValueError("descriptors are a uint8 array of shape [n, 128]")
        n, used = desc.shape[0], min(self.vocabulary_probes(), self.vocabulary_cells())
        cells = np.zeros((n, used), np.int32)
        dist2 = np.zeros((n, used), np.int32)
        rc = self.L.hesaff_stage_probe_cells(self.h, n, desc.ctypes.data if n else None, cells.ctypes.data if n else None, dist2.ctypes.data if n else None)
        if rc != 0 and used == 0:
            raise HesaffError(rc, "hesaff_stage_probe_cells: no cell layer is set")
        self._check(rc)
        return cells, dist2

    @property
    def assign_cells_ms(self):
        """HIP-event times (coarse assignment, grouping, assignment inside the cells) of the last assignment through a layer
        (profiling level >= 1), in ms"""
        a, b, f = C.c_float(), C.c_float(), C.c_float()
        self._check(self.L.hesaff_get_assign_cells_ms(self.h, C.byref(a), C.byref(b), C.byref(f)))
        return a.value, b.value, f.value

    def build_vocabulary_cells(self, words, coarse):
        """hesaff_build_vocabulary_cells: a layer for words uint8 [K, 128] given coarse uint8 [C, 128] -> (words in cell order uint8
        [K, 128], order int32 [K] with order[new] = old row, coarse uint8 [C', 128], first uint32 [C' + 1]); C' <= C: coarse rows that
        attract no row are dropped.  The context's own vocabulary is not touched."""
        words = _vocabulary_array(words)
        coarse = _vocabulary_array(coarse)
        k, c = words.shape[0], coarse.shape[0]
        words_out = np.zeros((k, 128), np.uint8); order = np.zeros(k, np.int32)
        coarse_out = np.zeros((c, 128), np.uint8); first = np.zeros(c + 1, np.uint32)
        kept = C.c_int(0)
        self._check(self.L.hesaff_build_vocabulary_cells(self.h, k, words.ctypes.data, c, coarse.ctypes.data, words_out.ctypes.data, order.ctypes.data,
                                                         coarse_out.ctypes.data, first.ctypes.data, C.byref(kept)))
        return words_out, order, coarse_out[:kept.value].copy(), first[:kept.value + 1].copy()

    def train_vocabulary_cells(self, desc, words, coarse, first, iterations):
        """hesaff_train_vocabulary_cells: Lloyd iterations over desc uint8 [n, 128] on the rows `words` uint8 [K, 128] of a layer
        (coarse, first), which stays fixed: every iteration assigns inside the cells -> (words, distortion, empty) as train_vocabulary."""
        if not isinstance(desc, np.ndarray) or desc.dtype != np.uint8 or desc.ndim != 2 or desc.shape[1] != 128:
            raise ValueError("descriptors are a uint8 array of shape [n, 128]")
        desc = np.ascontiguousarray(desc)
        coarse, first = _cells_arrays(coarse, first)
        n, c = desc.shape[0], coarse.shape[0]
        return self._train(lambda k, init, it, *a: self.L.hesaff_train_vocabulary_cells(self.h, n, desc.ctypes.data if n else None, k, init, c,
                                                                                      coarse.ctypes.data, first.ctypes.data, it, *a),
                           np.shape(words)[0], iterations, words)

    def train_vocabulary_cells_device(self, ptr, n, stride, offset, words, coarse, first, iterations):
        """hesaff_train_vocabulary_cells_device: the same on n descriptors in device memory, descriptor i at ptr + i * stride + offset"""
        coarse, first = _cells_arrays(coarse, first)
        c = coarse.shape[0]
        return self._train(lambda k, init, it, *a: self.L.hesaff_train_vocabulary_cells_device(self.h, int(n), C.c_void_p(ptr), int(stride), int(offset), k,
                                                                                             init, c, coarse.ctypes.data, first.ctypes.data, it, *a),
                           np.shape(words)[0], iterations, words)

    def train_cell_vocabulary(self, desc, k, cells, iterations, coarse_iterations):
        """The composite: G = train_vocabulary(desc, cells, coarse_iterations); V0 = the rows desc[r * n // k]; build_vocabulary_cells(V0,
        G); train_vocabulary_cells -> (words uint8 [k, 128], coarse uint8 [C', 128], first uint32 [C' + 1], distortion, empty).
        Needs n >= k >= cells."""
        if not isinstance(desc, np.ndarray) or desc.dtype != np.uint8 or desc.ndim != 2 or desc.shape[1] != 128:
            raise ValueError("descriptors are a uint8 array of shape [n, 128]")
        n, k, cells = desc.shape[0], int(k), int(cells)
        if not n >= k >= cells >= 1:
            raise ValueError("a cell vocabulary needs n >= k >= cells >= 1, not n = %d, k = %d, cells = %d" % (n, k, cells))
        coarse = self.train_vocabulary(desc, cells, coarse_iterations)[0]
        v0 = np.ascontiguousarray(desc[(np.arange(k, dtype=np.int64) * n) // k])
        v0, _, coarse, first = self.build_vocabulary_cells(v0, coarse)
        words, distortion, empty = self.train_vocabulary_cells(desc, v0, coarse, first, iterations)
        return words, coarse, first, distortion, empty

    # ---- Hamming embedding (hesaff_set_embedding, include/hesaff_amd.h) ----
    def set_embedding(self, projection, thresholds=None):
        """hesaff_set_embedding: projection int8 [64, 128] (entries in -127 .. 127) and thresholds int32 [K, 64], K the rows of the
        vocabulary that is set (both copied), or None to remove the embedding.  With one set, every call that assigns words also
        makes a 64-bit signature per key; signatures(image) hands them out."""
        if projection is None:
            self._check(self.L.hesaff_set_embedding(self.h, None, None))
            return
        P = _projection_array(projection)
        tau = _thresholds_array(thresholds, self.vocabulary_size)
        self._check(self.L.hesaff_set_embedding(self.h, P.ctypes.data, tau.ctypes.data))

    def embedding(self):
        """hesaff_get_embedding: (P int8 [64, 128], tau int32 [K, 64]), or None when no embedding is set"""
        k = C.c_int()
        self._check(self.L.hesaff_get_embedding(self.h, C.byref(k), None, None))
        if k.value == 0:
            return None
        P = np.zeros((EMBED_BITS, 128), np.int8); tau = np.zeros((k.value, EMBED_BITS), np.int32)
        self._check(self.L.hesaff_get_embedding(self.h, C.byref(k), P.ctypes.data, tau.ctypes.data))
        return P, tau

    def signatures(self, image):
        """hesaff_get_signatures: uint64 [count], row for row the keys (and words) of image `image` of the last host call (a copy)."""
        p = C.c_void_p(); n = C.c_int()
        if self.L.hesaff_get_signatures(self.h, int(image), C.byref(p), C.byref(n)) != 0:
            raise HesaffError(-2, "hesaff_get_signatures(%d): no embedding is set, or no such image in the last host call" % image)
        if n.value == 0:
            return np.zeros(0, np.uint64)
        return np.frombuffer((C.c_char * (n.value * 8)).from_address(p.value), dtype=np.uint64).copy()

    def signatures_device(self):
        """hesaff_get_signatures_device: (device pointer, rows) of the uint64 [total] array parallel to the keys of the last device-resident call."""
        p = C.c_void_p(); tot = C.c_int64()
        if self.L.hesaff_get_signatures_device(self.h, C.byref(p), C.byref(tot)) != 0:
            raise HesaffError(-2, "hesaff_get_signatures_device: no embedding is set, or the last call was not device-resident")
        return p.value, tot.value

    @staticmethod
    def _desc_words(desc, words):
        desc = np.ascontiguousarray(desc, dtype=np.uint8)
        words = _index_words(words)
        if desc.ndim != 2 or desc.shape[1] != 128 or len(words) != desc.shape[0]:
            raise ValueError("descriptors are uint8 [n, 128], words int32 [n] or [n, 2]")
        return desc, words, words.ndim

    def embed(self, desc, words):
        """hesaff_stage_embed: desc uint8 [n, 128] and their words int32 [n] or (word, dist2) rows [n, 2] -> uint64 [n] signatures under
        the context's embedding."""
        desc, words, stride = self._desc_words(desc, words)
        n = desc.shape[0]
        out = np.zeros(n, np.uint64)
        rc = self.L.hesaff_stage_embed(self.h, n, desc.ctypes.data if n else None, words.ctypes.data if n else None, stride, out.ctypes.data if n else None)
        self._check(rc)
        return out

    def embed_device(self, ptr, n, stride, offset, words_ptr, word_stride, out_ptr):
        """hesaff_embed_device: n descriptors in device memory (descriptor i at ptr + i * stride + offset), their words at words_ptr
        (key i's the int32 at + 4 i word_stride) -> n uint64 at out_ptr (raw device pointers)."""
        self._check(self.L.hesaff_embed_device(self.h, int(n), C.c_void_p(ptr), int(stride), int(offset), C.c_void_p(words_ptr), int(word_stride), C.c_void_p(out_ptr)))

    def project(self, desc, projection):
        """hesaff_stage_project: desc uint8 [n, 128] -> z int32 [n, 64] = projection . desc, by the kernel that makes the signatures."""
        desc = np.ascontiguousarray(desc, dtype=np.uint8)
        if desc.ndim != 2 or desc.shape[1] != 128:
            raise ValueError("descriptors are a uint8 array of shape [n, 128]")
        P = _projection_array(projection)
        n = desc.shape[0]
        z = np.zeros((n, EMBED_BITS), np.int32)
        self._check(self.L.hesaff_stage_project(self.h, n, desc.ctypes.data if n else None, P.ctypes.data, z.ctypes.data if n else None))
        return z

    def train_embedding(self, desc, words, projection, k=None):
        """hesaff_train_embedding: desc uint8 [n, 128], their words, projection int8 [64, 128] -> (tau int32 [k, 64], counts uint32 [k]):
        per word and bit the lower median of the word's projections, 0 for a word without keys.  k defaults to the vocabulary that
        is set.  The context's own embedding is not touched."""
        desc, words, stride = self._desc_words(desc, words)
        P = _projection_array(projection)
        k = self.vocabulary_size if k is None else int(k)
        n = desc.shape[0]
        tau = np.zeros((max(k, 0), EMBED_BITS), np.int32); counts = np.zeros(max(k, 0), np.uint32)
        self._check(self.L.hesaff_train_embedding(self.h, n, desc.ctypes.data if n else None, words.ctypes.data if n else None, stride, k, P.ctypes.data,
                                                  tau.ctypes.data, counts.ctypes.data))
        return tau, counts

    def train_embedding_device(self, ptr, n, stride, offset, words_ptr, word_stride, k, projection):
        """hesaff_train_embedding_device: the same on n descriptors and words in device memory (raw pointers)."""
        P = _projection_array(projection)
        k = int(k)
        tau = np.zeros((max(k, 0), EMBED_BITS), np.int32); counts = np.zeros(max(k, 0), np.uint32)
        self._check(self.L.hesaff_train_embedding_device(self.h, int(n), C.c_void_p(ptr), int(stride), int(offset), C.c_void_p(words_ptr), int(word_stride), k,
                                                         P.ctypes.data, tau.ctypes.data, counts.ctypes.data))
        return tau, counts

    @property
    def embedding_ms(self):
        """HIP-event times (the last signature launch; projection, grouping, medians of the last threshold training) at profiling >= 1, in ms"""
        v = [C.c_float() for _ in range(4)]
        self._check(self.L.hesaff_get_embedding_ms(self.h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    # ---- image index (hesaff_index_build, include/hesaff_amd.h) ----
    def build_index(self, images, vocabulary_size, signatures=None):
        """hesaff_index_build: images is a list with, per image, an int32 array of words [n] or of (word, dist2) rows [n, 2] (what
        words(i) returns), all of one kind; vocabulary_size is K.  Replaces the context's index.  signatures: per image a uint64
        array [n] (what signatures(i) returns) - hesaff_index_build_embedded: the same index with key lists for query_index(hamming=)."""
        arrays = [_index_words(w) for w in images]
        stride = _index_stride(arrays)
        counts = np.array([len(a) for a in arrays], np.int32)
        flat = np.ascontiguousarray(np.concatenate(arrays) if arrays else np.zeros((0,), np.int32))
        if signatures is not None:
            if len(signatures) != len(arrays):
                raise ValueError("one signature array per image")
            sg = [_signature_array(g, len(a)) for g, a in zip(signatures, arrays)]
            sflat = np.ascontiguousarray(np.concatenate(sg) if sg else np.zeros(0, np.uint64))
            self._check(self.L.hesaff_index_build_embedded(self.h, len(arrays), counts.ctypes.data, flat.ctypes.data if flat.size else None, stride,
                                                           sflat.ctypes.data if sflat.size else None, int(vocabulary_size)))
            return
        self._check(self.L.hesaff_index_build(self.h, len(arrays), counts.ctypes.data, flat.ctypes.data if flat.size else None, stride, int(vocabulary_size)))

    def build_embedded_index(self, images, signatures, vocabulary_size):
        """hesaff_index_build_embedded: build_index with a signature per key"""
        self.build_index(images, vocabulary_size, signatures=signatures)

    def build_embedded_index_device(self, ptr, sigs_ptr, counts, word_stride, vocabulary_size):
        """hesaff_index_build_embedded_device: words and signatures of all images one after the other in device memory (raw pointers)"""
        counts = np.ascontiguousarray(counts, dtype=np.int32)
        self._check(self.L.hesaff_index_build_embedded_device(self.h, len(counts), counts.ctypes.data, C.c_void_p(ptr), int(word_stride), C.c_void_p(sigs_ptr),
                                                              int(vocabulary_size)))

    def index_embedded(self):
        """hesaff_index_get_embedded: None for a plain index, otherwise (offsets uint32 [K + 1], images uint32 [T], sigs uint64 [T]): word
        w's keys are entries offsets[w] .. offsets[w + 1] - 1, in no particular order"""
        n, k, t, _ = self._need_index()
        flag = C.c_int()
        self._check(self.L.hesaff_index_get_embedded(self.h, C.byref(flag), None, None, None))
        if not flag.value:
            return None
        offsets = np.zeros(k + 1, np.uint32); images = np.zeros(t, np.uint32); sigs = np.zeros(t, np.uint64)
        self._check(self.L.hesaff_index_get_embedded(self.h, C.byref(flag), offsets.ctypes.data, images.ctypes.data if t else None, sigs.ctypes.data if t else None))
        return offsets, images, sigs

    # ---- the growing, durable index (hesaff_index_add, hesaff_index_save, hesaff_index_load) ----
    def add_to_index(self, images, signatures=None):
        """hesaff_index_add: appends the images (as build_index takes them) to the context's index; they take the numbers N .. N + m - 1.
        signatures: per image a uint64 array [n] - hesaff_index_add_embedded, on an index built with signatures."""
        arrays = [_index_words(w) for w in images]
        stride = _index_stride(arrays)
        counts = np.array([len(a) for a in arrays], np.int32)
        flat = np.ascontiguousarray(np.concatenate(arrays) if arrays else np.zeros((0,), np.int32))
        if signatures is not None:
            if len(signatures) != len(arrays):
                raise ValueError("one signature array per image")
            sg = [_signature_array(g, len(a)) for g, a in zip(signatures, arrays)]
            sflat = np.ascontiguousarray(np.concatenate(sg) if sg else np.zeros(0, np.uint64))
            self._check(self.L.hesaff_index_add_embedded(self.h, len(arrays), counts.ctypes.data, flat.ctypes.data if flat.size else None, stride,
                                                         sflat.ctypes.data if sflat.size else None))
            return
        self._check(self.L.hesaff_index_add(self.h, len(arrays), counts.ctypes.data, flat.ctypes.data if flat.size else None, stride))

    def add_to_index_device(self, ptr, counts, word_stride, sigs_ptr=None):
        """hesaff_index_add_device: the words of the new images one after the other in device memory (a raw pointer), counts the keys per
        image (host); with sigs_ptr hesaff_index_add_embedded_device."""
        counts = np.ascontiguousarray(counts, dtype=np.int32)
        if sigs_ptr is not None:
            self._check(self.L.hesaff_index_add_embedded_device(self.h, len(counts), counts.ctypes.data, C.c_void_p(ptr), int(word_stride), C.c_void_p(sigs_ptr)))
            return
        self._check(self.L.hesaff_index_add_device(self.h, len(counts), counts.ctypes.data, C.c_void_p(ptr), int(word_stride)))

    def index_postings(self):
        """hesaff_index_get_postings: (offsets uint32 [K + 1], images uint32 [n_postings], tf uint32 [n_postings]): word w's postings are
        entries offsets[w] .. offsets[w + 1] - 1, in no particular order"""
        n, k, t, p = self._need_index()
        offsets = np.zeros(k + 1, np.uint32); images = np.zeros(p, np.uint32); tf = np.zeros(p, np.uint32)
        self._check(self.L.hesaff_index_get_postings(self.h, offsets.ctypes.data, images.ctypes.data if p else None, tf.ctypes.data if p else None))
        return offsets, images, tf

    def save_index(self, path):
        """hesaff_index_save: the context's index to an index file ("HESAFFI1")"""
        self._check(self.L.hesaff_index_save(self.h, os.fsencode(path)))

    def load_index(self, path):
        """hesaff_index_load: replaces the context's index by an index file's; a file that is refused leaves the index as it was"""
        self._check(self.L.hesaff_index_load(self.h, os.fsencode(path)))

    @property
    def index_growth_ms(self):
        """HIP-event times (insert, tables, merge, scatter) of the last add and (load) of the last load's device pass (profiling >= 1), in ms"""
        v = [C.c_float() for _ in range(5)]
        self._check(self.L.hesaff_get_index_growth_ms(self.h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    # ---- removal from the index (hesaff_index_remove) ----
    def remove_from_index(self, images):
        """hesaff_index_remove: removes the images with the given numbers (distinct, in any order, at least one and not all) from the
        context's index; the images that stay keep their order and are renumbered densely.  -> remap int32 [N]: the new number of
        every old image, -1 for a removed one."""
        n = self._need_index()[0]
        gone = np.ascontiguousarray(np.asarray(images).reshape(-1), dtype=np.int32)
        remap = np.zeros(n, np.int32)
        self._check(self.L.hesaff_index_remove(self.h, len(gone), gone.ctypes.data if gone.size else None, remap.ctypes.data))
        return remap

    def index_remove_ms(self):
        """HIP-event times (count, tables, compact, keys) of the last removal (profiling >= 1), in ms"""
        v = [C.c_float() for _ in range(4)]
        self._check(self.L.hesaff_get_index_remove_ms(self.h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def build_index_device(self, ptr, counts, word_stride, vocabulary_size):
        """hesaff_index_build_device: the words of all images one after the other in device memory (a raw pointer; key j's word is the
        int32 at ptr + 4 j word_stride), counts the keys per image (host)."""
        counts = np.ascontiguousarray(counts, dtype=np.int32)
        self._check(self.L.hesaff_index_build_device(self.h, len(counts), counts.ctypes.data, C.c_void_p(ptr), int(word_stride), int(vocabulary_size)))

    def _query(self, call, top):
        top = int(top)
        images = np.zeros(max(min(top, 1024), 1), np.int32)
        scores = np.zeros(len(images), np.float64)
        n = C.c_int(0)
        self._check(call(top, images.ctypes.data, scores.ctypes.data, C.byref(n)))
        return images[:n.value].copy(), scores[:n.value].copy()

    def query_index(self, words, top, signatures=None, hamming=None):
        """hesaff_index_query: words int32 [n] or [n, 2] -> (images int32 [min(top, N)], scores float64), best first, ties by index.
        With signatures uint64 [n] and hamming = T in 0 .. 64 - hesaff_index_query_embedded, on an index built with signatures: a
        word match counts only where the two signatures differ in at most T bits."""
        w = _index_words(words)
        stride = _index_stride([w])
        if (signatures is None) != (hamming is None):
            raise ValueError("signatures and hamming go together")
        if signatures is not None:
            g = _signature_array(signatures, len(w))
            return self._query(lambda *a: self.L.hesaff_index_query_embedded(self.h, len(w), w.ctypes.data if len(w) else None, stride,
                                                                             g.ctypes.data if len(w) else None, int(hamming), *a), top)
        return self._query(lambda *a: self.L.hesaff_index_query(self.h, len(w), w.ctypes.data if len(w) else None, stride, *a), top)

    def query_embedded_index_device(self, ptr, sigs_ptr, n, word_stride, hamming, top):
        """hesaff_index_query_embedded_device: the same on n words and signatures in device memory (raw pointers)."""
        return self._query(lambda *a: self.L.hesaff_index_query_embedded_device(self.h, int(n), C.c_void_p(ptr), int(word_stride), C.c_void_p(sigs_ptr),
                                                                                int(hamming), *a), top)

    def query_index_device(self, ptr, n, word_stride, top):
        """hesaff_index_query_device: the same on n words in device memory (a raw pointer)."""
        return self._query(lambda *a: self.L.hesaff_index_query_device(self.h, int(n), C.c_void_p(ptr), int(word_stride), *a), top)

    # ---- batched index queries (hesaff_index_query_batch, include/hesaff_amd.h) ----
    def _query_batch(self, call, n_queries, top):
        top = int(top)
        rows = max(min(top, 1024), 1)
        images = np.zeros((max(n_queries, 1), rows), np.int32)
        scores = np.zeros(images.shape, np.float64)
        n = C.c_int(0)
        self._check(call(top, images.ctypes.data, scores.ctypes.data, C.byref(n)))
        return images[:n_queries, :n.value].copy(), scores[:n_queries, :n.value].copy()

    def query_index_batch(self, queries, top, signatures=None, hamming=None):
        """hesaff_index_query_batch: queries is a list with, per query, an int32 array of words [n] or [n, 2], all of one kind ->
        (images int32 [Q, min(top, N)], scores float64 [Q, min(top, N)]); row q is what query_index returns for queries[q].  With
        signatures (per query a uint64 array [n]) and hamming = T in 0 .. 64 - hesaff_index_query_batch_embedded."""
        arrays = [_index_words(w) for w in queries]
        stride = _index_stride(arrays)
        if (signatures is None) != (hamming is None):
            raise ValueError("signatures and hamming go together")
        counts = np.array([len(a) for a in arrays], np.int32)
        flat = np.ascontiguousarray(np.concatenate(arrays) if arrays else np.zeros((0,), np.int32))
        if signatures is not None:
            if len(signatures) != len(arrays):
                raise ValueError("one signature array per query")
            sg = [_signature_array(g, len(a)) for g, a in zip(signatures, arrays)]
            sflat = np.ascontiguousarray(np.concatenate(sg) if sg else np.zeros(0, np.uint64))
            return self._query_batch(lambda *a: self.L.hesaff_index_query_batch_embedded(self.h, len(arrays), counts.ctypes.data, flat.ctypes.data if flat.size else None,
                                                                                         stride, sflat.ctypes.data if sflat.size else None, int(hamming), *a),
                                     len(arrays), top)
        return self._query_batch(lambda *a: self.L.hesaff_index_query_batch(self.h, len(arrays), counts.ctypes.data, flat.ctypes.data if flat.size else None, stride, *a),
                                 len(arrays), top)

    def query_index_batch_device(self, ptr, counts, word_stride, top, sigs_ptr=None, hamming=None):
        """hesaff_index_query_batch_device: the words of all queries one after the other in device memory (a raw pointer), counts the
        words per query (host); with sigs_ptr and hamming hesaff_index_query_batch_embedded_device."""
        counts = np.ascontiguousarray(counts, dtype=np.int32)
        if counts.ndim != 1:
            raise ValueError("counts is a 1-d array: the words per query")
        if (sigs_ptr is None) != (hamming is None):
            raise ValueError("sigs_ptr and hamming go together")
        if sigs_ptr is not None:
            return self._query_batch(lambda *a: self.L.hesaff_index_query_batch_embedded_device(self.h, len(counts), counts.ctypes.data, C.c_void_p(ptr), int(word_stride),
                                                                                                C.c_void_p(sigs_ptr), int(hamming), *a), len(counts), top)
        return self._query_batch(lambda *a: self.L.hesaff_index_query_batch_device(self.h, len(counts), counts.ctypes.data, C.c_void_p(ptr), int(word_stride), *a),
                                 len(counts), top)

    def set_index_batch_budget(self, nbytes):
        """hesaff_index_set_batch_budget: the device scratch a chunk of a batch may hold, in bytes (0: the default); results do not
        depend on it.  Releases what earlier batches allocated."""
        nbytes = int(nbytes)
        if nbytes < 0:
            raise ValueError("a budget is a number of bytes, 0 for the default")
        self._check(self.L.hesaff_index_set_batch_budget(self.h, C.c_size_t(nbytes)))

    @property
    def index_batch_budget(self):
        """hesaff_index_get_batch_budget: the budget in force, in bytes"""
        v = C.c_size_t(0)
        self._check(self.L.hesaff_index_get_batch_budget(self.h, C.byref(v)))
        return v.value

    @property
    def index_batch_chunks(self):
        """hesaff_index_get_batch_chunks: the chunks the last batch ran in"""
        v = C.c_int(0)
        self._check(self.L.hesaff_index_get_batch_chunks(self.h, C.byref(v)))
        return v.value

    @property
    def index_batch_ms(self):
        """HIP-event times (group, score, select) summed over the chunks of the last batch (profiling >= 1), in ms"""
        v = [C.c_float() for _ in range(3)]
        self._check(self.L.hesaff_get_index_batch_ms(self.h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    @property
    def index_info(self):
        """hesaff_index_get_info: (n_images, vocabulary_size, n_keys, n_postings), or None when no index is built"""
        n, k, t, p = C.c_int(), C.c_int(), C.c_int64(), C.c_int64()
        if self.L.hesaff_index_get_info(self.h, C.byref(n), C.byref(k), C.byref(t), C.byref(p)) != 0:
            return None
        return n.value, k.value, t.value, p.value

    def _need_index(self):
        info = self.index_info
        if info is None:
            raise HesaffError(-2, "no index is built (build_index)")
        return info

    def index_scores(self):
        """hesaff_index_get_scores: (dot uint64 [N], score float64 [N], nq2) of the last query, for every image"""
        n = self._need_index()[0]
        dot = np.zeros(n, np.uint64); score = np.zeros(n, np.float64); nq2 = C.c_uint64()
        self._check(self.L.hesaff_index_get_scores(self.h, dot.ctypes.data, score.ctypes.data, C.addressof(nq2)))
        return dot, score, nq2.value

    def index_tables(self):
        """hesaff_index_get_tables: (df uint32 [K], idf uint32 [K], norm2 uint64 [N])"""
        n, k = self._need_index()[:2]
        df = np.zeros(k, np.uint32); idf = np.zeros(k, np.uint32); norm2 = np.zeros(n, np.uint64)
        self._check(self.L.hesaff_index_get_tables(self.h, df.ctypes.data, idf.ctypes.data, norm2.ctypes.data))
        return df, idf, norm2

    def clear_index(self):
        self._check(self.L.hesaff_index_clear(self.h))

    @property
    def index_ms(self):
        """HIP-event times (build, query) of the last build and the last query (profiling >= 1), in ms"""
        b, q = C.c_float(), C.c_float()
        self._check(self.L.hesaff_get_index_ms(self.h, C.byref(b), C.byref(q)))
        return b.value, q.value

    # ---- spatial verification (hesaff_verify_matches, include/hesaff_amd.h) ----
    def _verify(self, call, n_candidates):
        out = np.zeros((n_candidates, 6), np.int32); hyp = np.zeros((n_candidates, 3), np.float32); order = np.zeros(n_candidates, np.int32)
        self._check(call(out.ctypes.data, hyp.ctypes.data, order.ctypes.data))
        return out, hyp, order

    def verify_matches(self, query_rows, candidates, vocabulary_size, tolerance, max_pairs=1):
        """hesaff_verify_matches: query_rows and every entry of the list `candidates` are arrays of WORDS_ROW_DTYPE (what read_words
        returns) -> (out int32 [R, 6] = inliers, used, found, query_key, candidate_key, inert_keys; hyp float32 [R, 3] = L11, L21,
        L22 of the best hypothesis; order int32 [R], the candidates by (inliers descending, position ascending))."""
        q = _verify_rows(query_rows)
        arrays = [_verify_rows(c) for c in candidates]
        counts = np.array([len(a) for a in arrays], np.int32)
        flat = np.ascontiguousarray(np.concatenate(arrays) if arrays else np.zeros(0, WORDS_ROW_DTYPE))
        return self._verify(lambda *a: self.L.hesaff_verify_matches(self.h, len(q), q.ctypes.data if len(q) else None, len(arrays), counts.ctypes.data,
                                                                     flat.ctypes.data if len(flat) else None, int(vocabulary_size), int(max_pairs),
                                                                     float(tolerance), *a), len(arrays))

    def verify_matches_device(self, query_ptr, nq, candidates_ptr, counts, vocabulary_size, tolerance, max_pairs=1):
        """hesaff_verify_matches_device: the same on rows in device memory (raw pointers, 24 bytes per row, the candidates' rows one
        image after the other), counts the rows per candidate (host)."""
        counts = np.ascontiguousarray(counts, dtype=np.int32)
        return self._verify(lambda *a: self.L.hesaff_verify_matches_device(self.h, int(nq), C.c_void_p(query_ptr), len(counts), counts.ctypes.data,
                                                                            C.c_void_p(candidates_ptr), int(vocabulary_size), int(max_pairs), float(tolerance),
                                                                            *a), len(counts))

    def verify_pairs(self, candidate):
        """hesaff_verify_get_pairs: the used correspondences int32 [M, 2] = (query key, candidate key) of one candidate of the last call"""
        p, n = C.c_void_p(), C.c_int()
        self._check(self.L.hesaff_verify_get_pairs(self.h, int(candidate), C.byref(p), C.byref(n)))
        if n.value == 0:
            return np.zeros((0, 2), np.int32)
        return np.frombuffer(C.string_at(p.value, n.value * 8), np.int32).reshape(-1, 2).copy()

    @property
    def verify_query_inert(self):
        """hesaff_verify_get_query_inert: the inert keys of the last call's query"""
        n = C.c_int()
        self._check(self.L.hesaff_verify_get_query_inert(self.h, C.byref(n)))
        return n.value

    def stage_verify_pairs(self, pairs, tolerance):
        """hesaff_stage_verify_pairs: pairs float32 [m, 10] -> (inl int32 [m], best h or -1)"""
        c = np.ascontiguousarray(pairs, dtype=np.float32).reshape(-1, 10)
        inl = np.zeros(len(c), np.int32); best = C.c_int32(-2)
        self._check(self.L.hesaff_stage_verify_pairs(self.h, len(c), c.ctypes.data if len(c) else None, float(tolerance), inl.ctypes.data if len(c) else None,
                                                     C.byref(best)))
        return inl, best.value

    @property
    def verify_ms(self):
        """HIP-event times (pairs, hypotheses) of the last verify call (profiling >= 1), in ms"""
        a, b = C.c_float(), C.c_float()
        self._check(self.L.hesaff_get_verify_ms(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    # ---- query expansion (hesaff_expand_query, include/hesaff_amd.h) ----
    def expand_query(self, query_rows, candidates, out, hyp, vocabulary_size, min_inliers, max_images=1024, roi=None, max_rows=2 ** 18,
                     query_signatures=None, candidate_signatures=None):
        """hesaff_expand_query: the query's rows followed by the keys of the selected candidates (out[r][0] >= min_inliers, the best
        max_images of them), back-projected by hyp[r] and kept where they fall into roi = (x0, y0, x1, y1) - None: the bounding box
        of the query's live keys.  out and hyp are what verify_matches returned for the same query and candidates.
        -> (rows of WORDS_ROW_DTYPE [n_out], info int32 [R, 4] = rank or -1, live, kept, written keys) and, with query_signatures
        uint64 [nq] and candidate_signatures (a uint64 array per candidate), the signatures uint64 [n_out] as a third entry."""
        q = _verify_rows(query_rows)
        arrays = [_verify_rows(c) for c in candidates]
        counts = np.array([len(a) for a in arrays], np.int32)
        flat = np.ascontiguousarray(np.concatenate(arrays) if arrays else np.zeros(0, WORDS_ROW_DTYPE))
        out, hyp = _expand_hypotheses(out, hyp, len(arrays))
        roi = _expand_roi(roi, q)
        if (query_signatures is None) != (candidate_signatures is None):
            raise ValueError("signatures of the query and of the candidates go together")
        qs = cs = sigs = None
        cap = max(min(int(max_rows), len(q) + len(flat)), 1)
        if query_signatures is not None:
            if len(candidate_signatures) != len(arrays):
                raise ValueError("one signature array per candidate")
            qs = _signature_array(query_signatures, len(q))
            sg = [_signature_array(g, len(a)) for g, a in zip(candidate_signatures, arrays)]
            cs = np.ascontiguousarray(np.concatenate(sg) if sg else np.zeros(0, np.uint64))
            sigs = np.zeros(cap, np.uint64)
        rows = np.zeros(cap, WORDS_ROW_DTYPE); words = np.zeros(cap, np.int32); info = np.zeros((len(arrays), 4), np.int32); n = C.c_int(0)
        self._check(self.L.hesaff_expand_query(self.h, len(q), q.ctypes.data if len(q) else None, qs.ctypes.data if qs is not None and len(q) else None,
                                               len(arrays), counts.ctypes.data, flat.ctypes.data if len(flat) else None,
                                               cs.ctypes.data if cs is not None and len(flat) else None, out.ctypes.data, hyp.ctypes.data, int(min_inliers),
                                               int(max_images), roi.ctypes.data, int(vocabulary_size), int(max_rows), rows.ctypes.data, words.ctypes.data,
                                               sigs.ctypes.data if sigs is not None else None, C.byref(n), info.ctypes.data))
        if sigs is not None:
            return rows[:n.value].copy(), info, sigs[:n.value].copy()
        return rows[:n.value].copy(), info

    def expand_query_device(self, query_ptr, nq, candidates_ptr, counts, out, hyp, vocabulary_size, min_inliers, roi, rows_out_ptr, words_out_ptr,
                            max_images=1024, max_rows=2 ** 18, query_sigs_ptr=None, candidate_sigs_ptr=None, sigs_out_ptr=None):
        """hesaff_expand_query_device: the same on rows (24 bytes each), signatures and outputs in device memory (raw pointers; the
        outputs hold min(max_rows, nq + sum(counts)) entries); counts, out, hyp and roi on the host -> (n_out, info int32 [R, 4])."""
        counts = np.ascontiguousarray(counts, dtype=np.int32)
        out, hyp = _expand_hypotheses(out, hyp, len(counts))
        roi = _expand_roi(roi, None)
        info = np.zeros((len(counts), 4), np.int32); n = C.c_int(0)
        opt = lambda p: None if p is None else C.c_void_p(p)
        self._check(self.L.hesaff_expand_query_device(self.h, int(nq), opt(query_ptr), opt(query_sigs_ptr), len(counts), counts.ctypes.data, opt(candidates_ptr),
                                                      opt(candidate_sigs_ptr), out.ctypes.data, hyp.ctypes.data, int(min_inliers), int(max_images), roi.ctypes.data,
                                                      int(vocabulary_size), int(max_rows), opt(rows_out_ptr), opt(words_out_ptr), opt(sigs_out_ptr), C.byref(n),
                                                      info.ctypes.data))
        return n.value, info

    @property
    def expand_ms(self):
        """HIP-event times (flags with its scan, scatter) of the last expand call (profiling >= 1), in ms"""
        a, b = C.c_float(), C.c_float()
        self._check(self.L.hesaff_get_expand_ms(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def query_index_expanded(self, query_rows, image_rows, top, tolerance, min_inliers, max_images=1024, max_pairs=1, roi=None, max_rows=2 ** 18):
        """query -> verify -> expand -> query in one call.  image_rows[i] are the rows of index image i: the index keeps no geometry,
        so the caller supplies it.  -> ((images, scores, out, order) of the first query and its verification, (images, scores) of the
        query with the expanded rows, the expanded rows, info)."""
        q = _verify_rows(query_rows)
        k = self._need_index()[1]
        images, scores = self.query_index(np.ascontiguousarray(q["word"].astype(np.int32)), top)
        cands = [image_rows[int(i)] for i in images]
        if not cands:
            return (images, scores, np.zeros((0, 6), np.int32), np.zeros(0, np.int32)), (images, scores), q.copy(), np.zeros((0, 4), np.int32)
        out, hyp, order = self.verify_matches(q, cands, k, tolerance, max_pairs)
        rows, info = self.expand_query(q, cands, out, hyp, k, min_inliers, max_images=max_images, roi=roi, max_rows=max_rows)
        second = self.query_index(np.ascontiguousarray(rows["word"].astype(np.int32)), top)
        return (images, scores, out, order), second, rows, info

    def process_files(self, paths, out_paths=None, decode_threads=0, write_threads=0):
        """hesaff_process_files: image files -> <name>.hesaff.sift through the decode / device / write pipeline.
        -> list of (rc, stage, count_hessian, count_desc) per file."""
        n = len(paths)
        cp = (C.c_char_p * n)(*[os.fsencode(q) for q in paths])
        op = None
        if out_paths is not None:
            op = (C.c_char_p * n)(*[None if q is None else os.fsencode(q) for q in out_paths])
        st = (FileStatus * n)()
        self._check(self.L.hesaff_process_files(self.h, n, cp, op, decode_threads, write_threads, st))
        return [(s.rc, s.stage, s.count_hessian, s.count_desc) for s in st]

    def write_sift_batch_raw(self, paths, results, mr_size, threads=0):
        """hesaff_write_sift_batch on hesaff_result records (e.g. a slice of detect_batch_raw's return value)."""
        n = len(paths)
        arr = (_Result * n)(*[results[i] for i in range(n)])
        cp = (C.c_char_p * n)(*[os.fsencode(q) for q in paths])
        rc = self.L.hesaff_write_sift_batch(n, cp, arr, C.c_float(mr_size), threads)
        if rc != 0:
            raise HesaffError(rc, "hesaff_write_sift_batch")

    def detect_batch_device(self, d_ptr, n, width, height, masks_ptr=None, mask_row_stride=0, mask_img_stride=0):
        """Inputs resident in HBM (uint8 [n,H,W], raw device pointer).  -> (count_hessian[n], count_desc[n], d_keys, total).
        masks_ptr: n uint8 mask planes in device memory (raw device pointer; strides in bytes, 0 = tightly packed) for this call."""
        if masks_ptr is not None:
            self.set_next_masks_device(masks_ptr, n, mask_row_stride, mask_img_stride)
        ch = np.zeros(n, np.int32); cd = np.zeros(n, np.int32)
        dk = C.c_void_p(); tot = C.c_int64()
        self._check(self.L.hesaff_detect_batch_device(self.h, n, C.c_void_p(d_ptr), width, height, ch, cd, C.byref(dk), C.byref(tot)))
        return ch, cd, dk.value, tot.value

    def set_profiling(self, level):
        self._check(self.L.hesaff_set_profiling(self.h, level))

    def timings(self):
        t = Timings()
        self._check(self.L.hesaff_get_timings(self.h, C.byref(t)))
        return t

    # ---- stage entry points (one reference operator each) ----
    def gaussian_blur(self, img, sigma):
        img = np.ascontiguousarray(img, np.float32); out = np.empty_like(img)
        self._check(self.L.hesaff_stage_gaussian_blur(self.h, img, img.shape[0], img.shape[1], sigma, out))
        return out

    def hessian_response(self, img, norm):
        img = np.ascontiguousarray(img, np.float32); out = np.empty_like(img)
        self._check(self.L.hesaff_stage_hessian_response(self.h, img, img.shape[0], img.shape[1], norm, out))
        return out

    def half_image(self, img):
        img = np.ascontiguousarray(img, np.float32)
        out = np.empty((img.shape[0] // 2, img.shape[1] // 2), np.float32)
        self._check(self.L.hesaff_stage_half_image(self.h, img, img.shape[0], img.shape[1], out))
        return out

    def _pyramid(self, entry, g):
        """hesaff_stage_pyramid or its float twin on the contiguous image g: sizes first, then the planes, cut into octaves"""
        no = C.c_int(); nf = C.c_size_t()
        self._check(entry(self.h, None, g.shape[0], g.shape[1], None, C.byref(no), C.byref(nf)))
        buf = np.empty(max(nf.value, 1), np.float32)
        self._check(entry(self.h, g.ctypes.data, g.shape[0], g.shape[1], buf.ctypes.data, C.byref(no), C.byref(nf)))
        up = 1 if self.params.upscaleInputImage > 0 else 0   # (the first octave is the 2x up-sampled image: pyramid.cpp:267-271)
        out = []; off = 0; r, c = g.shape[0] << up, g.shape[1] << up
        for _ in range(no.value):
            n = r * c
            Ls = buf[off:off + 5 * n].reshape(5, r, c); off += 5 * n
            Rs = buf[off:off + 5 * n].reshape(5, r, c); off += 5 * n
            out.append((Ls, Rs))
            r //= 2; c //= 2
        return out

    def pyramid(self, gray_u8):
        """-> list over octaves of (L[5,rows,cols], R[5,rows,cols])."""
        g = np.ascontiguousarray(gray_u8, np.uint8)
        return self._pyramid(self.L.hesaff_stage_pyramid, g)

    def hessian_keypoints(self, gray_u8, cap=None):
        """-> f[n,5] = x,y,s,pd,response ; i[n,5] = type,octave,level,r0,c0 (reference order)."""
        g = np.ascontiguousarray(gray_u8, np.uint8)
        if cap is None:
            cap = max(4096, int(g.size * 0.05))
        f = np.zeros((cap, 5), np.float32); i = np.zeros((cap, 5), np.int32); cnt = C.c_int()
        self._check(self.L.hesaff_stage_hessian_keypoints(self.h, g, g.shape[0], g.shape[1], cap, f, i, C.byref(cnt)))
        n = min(cnt.value, cap)
        return f[:n].copy(), i[:n].copy(), cnt.value

    def detect_planes(self, L, R, band=0, cap=None):
        """hesaff_stage_detect_planes: the detection chain on the blur planes L and response planes R of one octave, [5, rows, cols] or
        [n_images, 5, rows, cols] (finite values).  band: 0 = the batch path's choice, or 32, 64, 128.
        -> f[n,5], i[n,5] as hessian_keypoints (octave 0), image[n], count."""
        L = np.ascontiguousarray(L, np.float32); R = np.ascontiguousarray(R, np.float32)
        if L.ndim == 3:
            L = L[None]; R = R[None]
        if L.ndim != 4 or L.shape[1] != 5 or R.shape != L.shape:
            raise ValueError("L and R must both be [n_images, 5, rows, cols]")
        nimg, _, rows, cols = L.shape
        if cap is None:
            cap = max(4096, int(nimg * rows * cols * 0.05))
        f = np.zeros((cap, 5), np.float32); i = np.zeros((cap, 5), np.int32); im = np.zeros(cap, np.int32); cnt = C.c_int()
        self._check(self.L.hesaff_stage_detect_planes(self.h, nimg, rows, cols, L.ctypes.data, R.ctypes.data, int(band), cap,
                                                      f.ctypes.data, i.ctypes.data, im.ctypes.data, C.byref(cnt)))
        n = min(cnt.value, cap)
        return f[:n].copy(), i[:n].copy(), im[:n].copy(), cnt.value

    def find_affine_shape(self, blur, kp):
        blur = np.ascontiguousarray(blur, np.float32); kp = np.ascontiguousarray(kp, np.float32).reshape(-1, 4)
        n = len(kp)
        conv = np.zeros(n, np.int32); U = np.zeros((n, 4), np.float32); it = np.zeros(n, np.int32)
        self._check(self.L.hesaff_stage_find_affine_shape(self.h, blur, blur.shape[0], blur.shape[1], n, kp, conv, U, it))
        return conv, U, it

    def rectify(self, A):
        A = np.ascontiguousarray(A, np.float32).reshape(-1, 4).copy()
        self._check(self.L.hesaff_stage_rectify(self.h, len(A), A))
        return A

    def affine_tail(self, abc, U, ratio_bef):
        """One pass of findAffineShape's tail (affine.cpp:72-97) per row, with the context's convergenceThreshold.
        -> abc'[n,3], U'[n,4], ratio[n], l[n,4] (l1, l2 of invSqrt, then of getEigenvalues), state[n] (0 continue, 1 break, 2 converged)"""
        abc = np.ascontiguousarray(abc, np.float32).reshape(-1, 3).copy(); U = np.ascontiguousarray(U, np.float32).reshape(-1, 4).copy()
        ratio = np.ascontiguousarray(ratio_bef, np.float32).reshape(-1).copy()
        n = len(abc)
        if len(U) != n or len(ratio) != n:
            raise ValueError("affine_tail: abc, U and ratio_bef must have one row per operand set")
        l = np.zeros((n, 4), np.float32); state = np.zeros(n, np.int32)
        self._check(self.L.hesaff_stage_affine_tail(self.h, n, abc, U, ratio, l, state))
        return abc, U, ratio, l, state

    def normalize_affine(self, img, kp, A):
        img = np.ascontiguousarray(img, np.float32); kp = np.ascontiguousarray(kp, np.float32).reshape(-1, 3)
        A = np.ascontiguousarray(A, np.float32).reshape(-1, 4)
        n = len(kp)
        rej = np.zeros(n, np.int32); patches = np.zeros((n, 41 * 41), np.float32)
        self._check(self.L.hesaff_stage_normalize_affine(self.h, img, img.shape[0], img.shape[1], n, kp, A, rej, patches))
        return rej, patches.reshape(n, 41, 41)

    def sift(self, patches):
        p = np.ascontiguousarray(patches, np.float32).reshape(-1, 41 * 41)
        d = np.zeros((len(p), 128), np.uint8)
        self._check(self.L.hesaff_stage_sift(self.h, len(p), p, d))
        return d

    def sift_parts(self, patches):
        """-> meanvar [n, 2], hist [n, 128] (un-normalised), desc [n, 128] u8 (hesaff_stage_sift_parts)."""
        p = np.ascontiguousarray(patches, np.float32).reshape(-1, 41 * 41)
        n = len(p)
        mv = np.zeros((n, 2), np.float32); hist = np.zeros((n, 128), np.float32); d = np.zeros((n, 128), np.uint8)
        self._check(self.L.hesaff_stage_sift_parts(self.h, n, p, mv, hist, d))
        return mv, hist, d

    def orientation_of(self, patches, parts=False):
        """hesaff_stage_orientation on [n, 41, 41] patches -> theta [n]; parts=True: (theta, hist [n, 36] after smoothing,
        cs [n, 2] = (cos theta, sin theta))."""
        p = np.ascontiguousarray(patches, np.float32).reshape(-1, 41 * 41)
        n = len(p)
        theta = np.zeros(n, np.float32); hist = np.zeros((n, 36), np.float32); cs = np.zeros((n, 2), np.float32)
        self._check(self.L.hesaff_stage_orientation(self.h, n, p, theta, hist, cs))
        return (theta, hist, cs) if parts else theta

    def orientation_peaks_of(self, patches, k=4):
        """hesaff_stage_orientation_peaks on [n, 41, 41] patches with orientation count k -> (n_ori [n] int32, bins [n, 4] int32,
        theta [n, 4] float32); beyond n_ori a bin is -1 and an angle 0."""
        p = np.ascontiguousarray(patches, np.float32).reshape(-1, 41 * 41)
        n = len(p)
        n_ori = np.zeros(n, np.int32); bins = np.zeros((n, 4), np.int32); theta = np.zeros((n, 4), np.float32)
        self._check(self.L.hesaff_stage_orientation_peaks(self.h, n, p, int(k), n_ori, bins, theta))
        return n_ori, bins, theta

    def sift_alive(self, patches, alive, fill=0):
        """-> desc [n, 128] u8, every byte `fill` before the call: rows of keypoints with alive == 0 keep it (hesaff_stage_sift_alive)."""
        p = np.ascontiguousarray(patches, np.float32).reshape(-1, 41 * 41)
        a = np.ascontiguousarray(alive, np.int32).reshape(-1)
        assert len(a) == len(p)
        d = np.full((len(p), 128), fill, np.uint8)
        self._check(self.L.hesaff_stage_sift_alive(self.h, len(p), p, a, d))
        return d

    def sift_mode(self, patches, mode, alive=None, fill=0):
        """-> desc [n, 128] u8 in descriptor mode `mode` (DESC_SIFT / DESC_ROOTSIFT), whatever the context's mode is
        (hesaff_stage_sift_mode).  alive=None: every keypoint; otherwise rows of keypoints with alive == 0 keep `fill`."""
        p = np.ascontiguousarray(patches, np.float32).reshape(-1, 41 * 41)
        d = np.full((len(p), 128), fill, np.uint8)
        a = None
        if alive is not None:
            a = np.ascontiguousarray(alive, np.int32).reshape(-1)
            assert len(a) == len(p)
        self._check(self.L.hesaff_stage_sift_mode(self.h, len(p), p, None if a is None else a.ctypes.data, int(mode), d))
        return d

    def export(self, keys, mr_size=None, fmt=1):
        """exportKeypoints on the device (hesaff_stage_export): bytes of the .hesaff.sift file (fmt 1) or of the sidecar (fmt 2)."""
        keys = np.ascontiguousarray(keys, dtype=KEYPOINT_DTYPE)
        buf = C.c_void_p(); n = C.c_size_t()
        mr = self.params.mrSize if mr_size is None else mr_size
        self._check(self.L.hesaff_stage_export(self.h, keys.ctypes.data, len(keys), C.c_float(mr), fmt, C.byref(buf), C.byref(n)))
        try:
            return C.string_at(buf.value, n.value)
        finally:
            self.L.hesaff_free(buf)

    def fmt_g(self, v):
        """The device's "%g" print of float32 values -> list of bytes."""
        v = np.ascontiguousarray(v, np.float32).reshape(-1)
        text = np.zeros((len(v), 16), np.uint8); lens = np.zeros(len(v), np.int32)
        self._check(self.L.hesaff_stage_fmt_g(self.h, len(v), v, text.ctypes.data, lens))
        return text, lens

    def jpeg_pixels(self, layout, blobs):
        """The device half of the JPEG reader: blobs [n, blob_bytes] uint8 of one layout -> pixels [n, H, W(, 3)] uint8."""
        blobs = np.ascontiguousarray(blobs, np.uint8)
        if blobs.ndim == 1:
            blobs = blobs[None]
        n = blobs.shape[0]
        shape = (n, layout.height, layout.width) + ((3,) if layout.channels == 3 else ())
        out = np.zeros(shape, np.uint8)
        self._check(self.L.hesaff_stage_jpeg_pixels(self.h, C.byref(layout), n, blobs.ctypes.data, blobs.shape[1], out.ctypes.data))
        return out

    def math(self, a, b):
        a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
        at = np.zeros_like(a); pw = np.zeros_like(a)
        self._check(self.L.hesaff_stage_math(self.h, a.size, a.reshape(-1), b.reshape(-1), at.reshape(-1), pw.reshape(-1)))
        return at, pw

    def math_sift(self, gy, gx):
        """-> ori_general, ori_nd, grad_general, grad_nd (hesaff_stage_math_sift)."""
        gy = np.ascontiguousarray(gy, np.float32).reshape(-1); gx = np.ascontiguousarray(gx, np.float32).reshape(-1)
        outs = [np.zeros_like(gy) for _ in range(4)]
        self._check(self.L.hesaff_stage_math_sift(self.h, gy.size, gy, gx, *outs))
        return outs

    def math_sift_general(self, gy, gx):
        """-> ori, grad, coord: the flat-patch forms of the descriptor gradient (hesaff_stage_math_sift_general)."""
        gy = np.ascontiguousarray(gy, np.float32).reshape(-1); gx = np.ascontiguousarray(gx, np.float32).reshape(-1)
        outs = [np.zeros_like(gy) for _ in range(3)]
        self._check(self.L.hesaff_stage_math_sift_general(self.h, gy.size, gy, gx, *outs))
        return outs
