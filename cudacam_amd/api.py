"""ctypes binding of libhipcanny.so plus Python mirrors of the reference operator classes.

`CannyEdge` and `cvPipeline` keep the names, argument meaning and error behaviour of
cvp::cuda::CannyEdge (src/cvp/cannyEdgeH.hpp:17-32) and cvp::cvPipeline (src/cvp/cvPipeline.hpp:20-39)
so the parity tests read like tests of the reference.  numpy arrays play the role of cv::Mat:
(H, W) uint8 == CV_8UC1, (H, W, 3) uint8 == CV_8UC3 (BGR).

There is no CPU fallback: if the shared library or a GPU is missing, construction raises.
"""
import ctypes as C
import enum
import math
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HIPCANNY_LIB") or os.path.join(_HERE, "libhipcanny.so")  # override: kernel experiments only


class CannyStage(enum.IntEnum):
    """cvp::CannyStage, src/cvp/define.hpp:9-17"""
    MONO = 0
    GAUSSIAN = 1
    GRADIENT = 2
    NMS = 3
    THRESH = 4
    HYSTER = 5


# cvp::CANNY_STAGES, src/cvp/define.hpp:27-34 (display strings double as timer names)
CANNY_STAGES = {
    CannyStage.MONO: "1/6 Mono Conversion",
    CannyStage.GAUSSIAN: "2/6 Gaussian Noise Removal",
    CannyStage.GRADIENT: "3/6 Gradient Computation",
    CannyStage.NMS: "4/6 Non Maximum Suppression",
    CannyStage.THRESH: "5/6 Double Threshold",
    CannyStage.HYSTER: "6/6 Hysteresis",
}

MODE_R, MODE_O = 0, 1
OPT_NMS_SATURATE = 1
OPT_PIPELINE = 2
OPT_PER_CHANNEL = 3
OPT_FRONT_SPLIT = 4
OPT_L2_GRADIENT = 5
OPT_DEBUG_TAPS = 6
OPT_FRONT_HALF = 7
OPT_FRONT_DENSE = 8
OPT_COPY_STREAMS = 9
OPT_PIPELINE_SLOTS = 10
OPT_FRONT_WPB = 11
OPT_FRONT_MX = 12
OPT_APERTURE = 13   # mode O: cv::Canny's apertureSize, 3 (default) or 5
OPT_TEST_HYST_LATE_GRID, OPT_TEST_HYST_LOOP, OPT_TEST_HYST_DIAG, OPT_TEST_HYST_GEOM, OPT_TEST_DENSE_ENTER, OPT_TEST_DENSE_LEAVE = 100, 101, 102, 103, 104, 105   # test / diagnostic hooks
OPT_TEST_HOUGH_ROWS = 107      # angles per workgroup of k_hough_vote (measurements; 0: by the plan's rule)
OPT_TEST_HOUGH_SCRATCH = 106   # bytes: the bound of hough_lines_device's scratch (tests: several passes on a small batch)
TAP_BLUR, TAP_THRESH = 1, 2
# front forms hc_last_run_info reports for canny_device at apertures 7 / -1 (the header's HC_FORM_O_APERTURE7 / HC_FORM_O_SCHARR)
FORM_O_APERTURE7, FORM_O_SCHARR = 8, 9
# rules of hc_auto_thresholds_device (the header's HC_AUTO_MEDIAN / HC_AUTO_OTSU)
AUTO_MEDIAN, AUTO_OTSU = 0, 1
# borders of hc_gaussian_blur_device (the header's HC_BORDER_REFLECT_101 / HC_BORDER_REPLICATE)
BORDER_REFLECT_101, BORDER_REPLICATE = 0, 1
# words of a statistics row of hc_connected_components_device (the header's HC_CC_STAT_*)
CC_STAT_LEFT, CC_STAT_TOP, CC_STAT_WIDTH, CC_STAT_HEIGHT, CC_STAT_AREA, CC_STAT_WORDS = 0, 1, 2, 3, 4, 5
# operations and element shapes of hc_morphology_device / hc_structuring_element (the header's HC_MORPH_*)
MORPH_ERODE, MORPH_DILATE, MORPH_OPEN, MORPH_CLOSE, MORPH_GRADIENT = 0, 1, 2, 3, 4
MORPH_RECT, MORPH_CROSS, MORPH_ELLIPSE = 0, 1, 2
# targets and distance types of hc_distance_transform_device, and the squared distance of a frame without a feature pixel (the
# header's HC_DT_*)
DT_TO_NONZERO, DT_TO_ZERO = 0, 1
DT_SQUARED_I32, DT_F32 = 0, 1
DT_NONE = 2147483647
# methods of hc_thinning_device (the header's HC_THIN_*) and the names Context.thinning takes for them
THIN_ZHANGSUEN, THIN_GUOHALL = 0, 1
THIN_METHODS = {"zhangsuen": THIN_ZHANGSUEN, "guohall": THIN_GUOHALL}
# methods of hc_corner_response_device (the header's HC_CORNER_*) and the names Context.corner_response takes for them
CORNER_MIN_EIGEN, CORNER_HARRIS = 0, 1
CORNER_METHODS = {"min_eigen": CORNER_MIN_EIGEN, "harris": CORNER_HARRIS}
# words of hc_last_hysteresis_schedule, in the order of the header's HC_SCHED_* indices
SCHEDULE_FIELDS = ("launches", "lists", "loop", "hist_grid", "longest", "overflows", "tiles", "tile_rows", "waves", "panels", "frames")

# every symbol include/hipcanny.h declares
ABI_SYMBOLS = [
    "hc_create", "hc_destroy", "hc_set_thresholds", "hc_get_thresholds", "hc_upload", "hc_run", "hc_run_device",
    "hc_hysteresis_device", "hc_download", "hc_sync", "hc_set_stream", "hc_enable_profiling", "hc_stage_time_ms", "hc_profile_get",
    "hc_device_ptrs", "hc_last_hysteresis_info", "hc_hysteresis_stats", "hc_set_tuning", "hc_set_option", "hc_selftest", "hc_last_error", "hc_version",
    "hc_host_alloc", "hc_host_free", "hc_profile_get_front", "hc_debug_tap", "hc_use_own_stream", "hc_profile_get_intervals", "hc_last_run_info", "hc_pipeline_depth", "hc_pipeline_slots_in_use", "hc_front_waves_per_workgroup",
    "hc_profile_get_front_each", "hc_hysteresis_totals", "hc_last_hysteresis_schedule", "hc_download_begin", "hc_download_end", "hc_run_gradients_device",
    "hc_derivatives_device", "hc_canny_device", "hc_frame_thresholds_device", "hc_histogram_device", "hc_auto_thresholds_device",
    "hc_edge_points_device", "hc_gaussian_blur_device", "hc_hough_lines_device", "hc_hough_tables",
    "hc_hough_segments_device", "hc_hough_walk_tables", "hc_hough_circles_device", "hc_hough_circle_geometry",
    "hc_connected_components_device", "hc_morphology_device", "hc_structuring_element", "hc_distance_transform_device",
    "hc_thinning_device", "hc_corner_response_device", "hc_good_features_device", "hc_pyr_down_device", "hc_lk_flow_device",
]
# ... and the one whose name ends in a digit, which the name pattern of tests/test_abi_cpu.py does not read from the header
ABI_SYMBOLS_HOST = ["hc_gaussian_taps_q8"]

_lib = None
_lib_legacy = None
LEGACY_LIB_PATH = os.path.join(_HERE, "libhipcanny_legacy.so")


class HipCannyError(RuntimeError):
    pass


def preload_hip_runtime():
    """One HIP runtime per process.  The PyTorch wheel bundles its own libamdhip64 (file name
    libamdhip64.so, SONAME libamdhip64.so.7 -- the same SONAME as /opt/rocm's).  If libhipcanny
    pulled in /opt/rocm's copy first, a later `import torch` would load the bundled one as well and
    the second runtime finds no GPU.  Loading torch's copy first (without importing torch) makes
    every later user -- this library, torch, oracle/_ref -- resolve to that single instance."""
    import importlib.util
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.origin:
        return None
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        return C.CDLL(cand, mode=C.RTLD_GLOBAL)
    return None


def load_library(legacy=False):
    """Loads libhipcanny.so (fails loudly when it has not been built).  legacy: libhipcanny_legacy.so instead -- the same
    sources plus the round-1 front kernels of Mode R (HC_OPT_FRONT_SPLIT 1 / 0), which the product library no longer
    contains; parity tests run every case through them as independent implementations."""
    global _lib, _lib_legacy
    if legacy and _lib_legacy is not None:
        return _lib_legacy
    if not legacy and _lib is not None:
        return _lib
    preload_hip_runtime()
    path = LEGACY_LIB_PATH if legacy else LIB_PATH
    if not os.path.exists(path):
        raise HipCannyError(f"{path} is missing: run `python -m cudacam_amd.build` (hipcc, gfx950). There is no CPU fallback.")
    L = C.CDLL(path)
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    L.hc_create.restype = vp
    L.hc_create.argtypes = [i, i, i, i, i, i]
    L.hc_destroy.restype = None
    L.hc_destroy.argtypes = [vp]
    L.hc_set_thresholds.argtypes = [vp, i, i]
    L.hc_get_thresholds.argtypes = [vp, C.POINTER(i), C.POINTER(i)]
    L.hc_upload.argtypes = [vp, vp, sz, sz, i]
    L.hc_run.argtypes = [vp, i, i]
    L.hc_run_device.argtypes = [vp, vp, sz, sz, vp, sz, sz, i, i]
    L.hc_hysteresis_device.argtypes = [vp, vp, sz, sz, vp, sz, sz, i]
    L.hc_run_gradients_device.argtypes = [vp, vp, vp, sz, sz, vp, sz, sz, i]
    L.hc_derivatives_device.argtypes = [vp, vp, sz, sz, vp, vp, sz, sz, i, i]
    L.hc_canny_device.argtypes = [vp, vp, sz, sz, vp, sz, sz, i, C.c_double, C.c_double, i, i]
    L.hc_frame_thresholds_device.argtypes = [vp, vp, i]
    L.hc_histogram_device.argtypes = [vp, vp, sz, sz, i, vp]
    L.hc_auto_thresholds_device.argtypes = [vp, vp, sz, sz, i, i, C.c_double, vp]
    L.hc_edge_points_device.argtypes = [vp, vp, sz, sz, i, vp, vp, sz]
    L.hc_gaussian_blur_device.argtypes = [vp, vp, sz, sz, vp, sz, sz, i, i, C.POINTER(C.c_uint16), i]
    L.hc_gaussian_taps_q8.argtypes = [i, C.c_double, C.POINTER(C.c_uint16)]
    d, fp = C.c_double, C.POINTER(C.c_float)
    L.hc_hough_lines_device.argtypes = [vp, vp, vp, sz, i, d, d, i, d, d, vp, vp, sz]
    L.hc_hough_tables.argtypes = [i, i, d, d, d, d, C.POINTER(i), C.POINTER(i), fp, fp, fp, sz]
    L.hc_hough_segments_device.argtypes = [vp, vp, sz, sz, vp, vp, sz, i, d, d, d, d, i, i, vp, vp, sz]
    L.hc_hough_walk_tables.argtypes = [i, i, d, d, d, d, C.POINTER(i), C.POINTER(C.c_int32), fp, fp, sz]
    L.hc_hough_circles_device.argtypes = [vp, vp, vp, sz, vp, vp, sz, sz, i, d, d, i, i, i, sz, vp, vp, sz]
    L.hc_connected_components_device.argtypes = [vp, vp, sz, sz, i, i, vp, sz, sz, vp, vp, vp, sz]
    L.hc_morphology_device.argtypes = [vp, vp, sz, sz, vp, sz, sz, i, i, i, i, C.POINTER(C.c_int8)]
    L.hc_structuring_element.argtypes = [i, i, C.POINTER(C.c_int8)]
    L.hc_distance_transform_device.argtypes = [vp, vp, sz, sz, i, i, i, vp, sz, sz, vp, sz, sz]
    L.hc_thinning_device.argtypes = [vp, vp, sz, sz, vp, sz, sz, i, i, i, vp]
    L.hc_corner_response_device.argtypes = [vp, vp, vp, sz, sz, vp, sz, sz, i, i, i, d]
    L.hc_good_features_device.argtypes = [vp, vp, sz, sz, i, d, d, sz, vp, vp, vp, sz]
    L.hc_pyr_down_device.argtypes = [vp, vp, sz, sz, i, i, vp, sz, sz, i]
    L.hc_lk_flow_device.argtypes = [vp, vp, vp, sz, sz, i, i, i, i, vp, vp, vp, sz, i, i, d, d, i, vp, vp]
    L.hc_hough_circle_geometry.argtypes = [i, i, d, d, i, i, C.POINTER(i), C.POINTER(i), C.POINTER(C.c_longlong)]
    L.hc_download.argtypes = [vp, vp, sz, sz, i]
    L.hc_download_begin.argtypes = [vp, vp, sz, sz, i]
    L.hc_download_end.argtypes = [vp]
    L.hc_sync.argtypes = [vp]
    L.hc_set_stream.argtypes = [vp, vp]
    L.hc_use_own_stream.argtypes = [vp]
    L.hc_enable_profiling.argtypes = [vp, i]
    L.hc_stage_time_ms.argtypes = [vp, i, C.POINTER(C.c_float)]
    L.hc_profile_get.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_long), i]
    L.hc_profile_get_front.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_long)]
    L.hc_device_ptrs.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(sz), C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]
    L.hc_last_hysteresis_info.argtypes = [vp, C.POINTER(i), C.POINTER(i)]
    L.hc_hysteresis_stats.argtypes = [vp, C.POINTER(C.c_uint), i]
    L.hc_set_tuning.argtypes = [vp, i, i]
    L.hc_set_option.argtypes = [vp, i, i]
    L.hc_selftest.argtypes = [i]
    L.hc_debug_tap.argtypes = [vp, i, vp, sz, sz, i]
    L.hc_last_run_info.argtypes = [vp, C.POINTER(i), C.POINTER(i), C.POINTER(i)]
    L.hc_pipeline_depth.argtypes = [vp, i]
    L.hc_pipeline_slots_in_use.argtypes = [vp]
    L.hc_front_waves_per_workgroup.argtypes = [vp]
    L.hc_profile_get_intervals.argtypes = [vp, C.POINTER(C.c_float), i, C.POINTER(i)]
    L.hc_profile_get_front_each.argtypes = [vp, C.POINTER(C.c_float), i, C.POINTER(i)]
    L.hc_hysteresis_totals.argtypes = [vp, C.POINTER(C.c_ulonglong), i]
    L.hc_last_hysteresis_schedule.argtypes = [vp, C.POINTER(i), i]
    L.hc_host_alloc.restype = vp
    L.hc_host_alloc.argtypes = [sz]
    L.hc_host_free.restype = None
    L.hc_host_free.argtypes = [vp]
    L.hc_last_error.restype = C.c_char_p
    L.hc_version.restype = C.c_char_p
    for name in ABI_SYMBOLS + ABI_SYMBOLS_HOST:
        getattr(L, name)
    if legacy:
        _lib_legacy = L
    else:
        _lib = L
    return L


def last_error():
    msg = load_library().hc_last_error().decode()
    if _lib_legacy is not None:   # (a context of the test library keeps its error text there)
        other = _lib_legacy.hc_last_error().decode()
        if other and other != msg:
            msg = (msg + " | " if msg else "") + other
    return msg


def _ck(rc):
    if rc != 0:
        raise HipCannyError(f"hipcanny error {rc}: {last_error()}")


_FIXED_TAPS_Q8 = {3: [64, 128, 64], 5: [16, 64, 96, 64, 16], 7: [8, 28, 56, 72, 56, 28, 8]}


def gaussian_taps_q8(ksize, sigma=0.0):
    """The Q8 taps (256 = 1.0) of a ksize Gaussian for gaussian_blur_device, by the rule include/hipcanny.h states for
    hc_gaussian_taps_q8 -- pure Python, the same result: ksize 3, 5 or 7; sigma <= 0 gives OpenCV's small fixed kernels."""
    import math
    ksize, sigma = int(ksize), float(sigma)
    if ksize not in _FIXED_TAPS_Q8:
        raise HipCannyError("gaussian_taps_q8: ksize 3, 5 or 7")
    if not math.isfinite(sigma):
        raise HipCannyError("gaussian_taps_q8: sigma must be finite")
    if sigma <= 0:
        return list(_FIXED_TAPS_Q8[ksize])
    r = ksize // 2
    den = 2.0 * sigma * sigma
    g = [1.0 if i == r else math.exp(-float((i - r) * (i - r)) / den) if den > 0 else 0.0 for i in range(ksize)]
    total = 0.0
    for v in g:   # (added in index order, as the C function adds them: the built-in sum compensates)
        total += v
    taps, err = [0] * ksize, 0.0
    for i in range(r):
        x = 256.0 * (g[i] / total) + err
        v = round(x)   # half to even, as nearbyint
        err = x - v
        taps[i] = taps[ksize - 1 - i] = int(v)
    taps[r] = 256 - sum(taps)
    if min(taps) < 0 or max(taps) > 256:
        raise HipCannyError("gaussian_taps_q8: sigma gives taps outside 0 .. 256")
    return taps


def structuring_element(shape, ksize):
    """The ksize half-widths of cv::getStructuringElement(shape, Size(ksize, ksize)) for morphology_device (hc_structuring_element:
    the host function; no context, no GPU): shape MORPH_RECT, MORPH_CROSS or MORPH_ELLIPSE, ksize 3, 5 or 7.  Row j of the element
    covers the columns -spans[j] .. +spans[j] around the anchor."""
    spans = (C.c_int8 * 8)()
    _ck(load_library().hc_structuring_element(int(shape), int(ksize), spans))
    return [int(v) for v in spans[:int(ksize)]]


def hough_tables(width, height, rho, theta, min_theta=0.0, max_theta=math.pi):
    """Geometry and tables of hough_lines_device for width x height frames (hc_hough_tables: the host function the device entry
    itself uses; no context, no GPU).  Returns (numangle, numrho, tab_cos, tab_sin, tab_theta), the tables float32 [numangle]."""
    L = load_library()
    na, nr = C.c_int(0), C.c_int(0)
    args = (int(width), int(height), float(rho), float(theta), float(min_theta), float(max_theta))
    _ck(L.hc_hough_tables(*args, C.byref(na), C.byref(nr), None, None, None, 0))
    tabs = [np.empty(na.value, np.float32) for _ in range(3)]
    fp = C.POINTER(C.c_float)
    _ck(L.hc_hough_tables(*args, C.byref(na), C.byref(nr), *[t.ctypes.data_as(fp) for t in tabs], na.value))
    return (na.value, nr.value, *tabs)


def hough_walk_tables(width, height, rho, theta, min_theta=0.0, max_theta=math.pi):
    """The walk tables of hough_segments_device for width x height frames (hc_hough_walk_tables: the host function the device
    entry itself uses; no context, no GPU).  Returns (numangle, major int32, slope float32, scale float32), [numangle] each."""
    L = load_library()
    na = C.c_int(0)
    args = (int(width), int(height), float(rho), float(theta), float(min_theta), float(max_theta))
    _ck(L.hc_hough_walk_tables(*args, C.byref(na), None, None, None, 0))
    major, slope, scale = np.empty(na.value, np.int32), np.empty(na.value, np.float32), np.empty(na.value, np.float32)
    fp = C.POINTER(C.c_float)
    _ck(L.hc_hough_walk_tables(*args, C.byref(na), major.ctypes.data_as(C.POINTER(C.c_int32)), slope.ctypes.data_as(fp), scale.ctypes.data_as(fp), na.value))
    return na.value, major, slope, scale


def hough_circle_geometry(width, height, dp, min_dist, min_radius, max_radius):
    """The geometry of hough_circles_device for width x height frames (hc_hough_circle_geometry: the host function the device
    entry itself uses; no context, no GPU).  Returns (acc_width, acc_height, min_d2): the accumulator's cells and the smallest
    squared distance of two kept centres, in cells."""
    L = load_library()
    aw, ah, d2 = C.c_int(0), C.c_int(0), C.c_longlong(0)
    _ck(L.hc_hough_circle_geometry(int(width), int(height), float(dp), float(min_dist), int(min_radius), int(max_radius), C.byref(aw), C.byref(ah), C.byref(d2)))
    return aw.value, ah.value, d2.value


class Context:
    """Thin RAII wrapper of hc_ctx (one device, one stream)."""

    def __init__(self, width, height, channels=1, max_batch=1, mode=MODE_R, device=0, front_split=None):
        """front_split: HC_OPT_FRONT_SPLIT for the context's whole life (None: the library's default, k_front8 / k_front8o).
        The round-1 front kernels of Mode R (1: k_blur + k_nms, 0: the 4-px k_front) are not part of the product library:
        such a context is created in libhipcanny_legacy.so (parity tests, bench.py --front split / fused4)."""
        self.lib = load_library(legacy=front_split in (0, 1) and int(mode) == MODE_R)
        self.w, self.h, self.c, self.max_batch = int(width), int(height), int(channels), int(max_batch)
        self.device = int(device)
        self.handle = self.lib.hc_create(int(device), self.w, self.h, self.c, self.max_batch, int(mode))
        if not self.handle:
            raise HipCannyError(f"hc_create failed: {last_error()}")
        if front_split is not None:
            self.set_option(OPT_FRONT_SPLIT, front_split)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.hc_destroy(self.handle)
            self.handle = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_thresholds(self, low, high):
        _ck(self.lib.hc_set_thresholds(self.handle, int(low), int(high)))

    def get_thresholds(self):
        lo, hi = C.c_int(), C.c_int()
        _ck(self.lib.hc_get_thresholds(self.handle, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def set_tuning(self, chunk_rows=0, hyst_launches=0):
        _ck(self.lib.hc_set_tuning(self.handle, int(chunk_rows), int(hyst_launches)))

    def set_option(self, option, value):
        _ck(self.lib.hc_set_option(self.handle, int(option), int(value)))
        if int(option) == OPT_PER_CHANNEL:
            self._maps_per_frame = 3 if value else 1

    def set_stream(self, stream_handle):
        """Run on the caller's hipStream_t (0 = the null stream, e.g. torch's default current stream)."""
        _ck(self.lib.hc_set_stream(self.handle, C.c_void_p(stream_handle)))

    def use_own_stream(self):
        _ck(self.lib.hc_use_own_stream(self.handle))

    def enable_profiling(self, on):
        _ck(self.lib.hc_enable_profiling(self.handle, int(bool(on))))

    def stage_time_ms(self, stage):
        ms = C.c_float()
        _ck(self.lib.hc_stage_time_ms(self.handle, int(stage), C.byref(ms)))
        return ms.value

    def profile_get(self, reset=True):
        """(sum_ms[3], nruns) over all profiled runs since the last reset: stage 0 / front / hysteresis+expand."""
        sums = (C.c_double * 3)()
        n = C.c_long()
        _ck(self.lib.hc_profile_get(self.handle, sums, C.byref(n), int(bool(reset))))
        return [sums[0], sums[1], sums[2]], n.value

    def profile_intervals(self, cap=4096):
        """End-of-run to end-of-run times (ms) of consecutive profiled runs since the last reset."""
        buf = (C.c_float * cap)()
        n = C.c_int()
        _ck(self.lib.hc_profile_get_intervals(self.handle, buf, cap, C.byref(n)))
        return [buf[k] for k in range(min(cap, n.value))]

    def profile_front_each(self, cap=4096):
        """The front kernels' time (ms) of every profiled HYSTER run since the last reset, in run order."""
        buf = (C.c_float * cap)()
        n = C.c_int()
        _ck(self.lib.hc_profile_get_front_each(self.handle, buf, cap, C.byref(n)))
        return [buf[k] for k in range(min(cap, n.value))]

    def hysteresis_totals(self, reset=False):
        """(runs, runs continued from the host, launches with work, launches queued) since creation / the last reset."""
        t = (C.c_ulonglong * 4)()
        _ck(self.lib.hc_hysteresis_totals(self.handle, t, int(bool(reset))))
        return tuple(int(v) for v in t)

    def hysteresis_schedule(self):
        """The schedule the most recent completed run got (hc_last_hysteresis_schedule), as a dict: launches queued,
        lists (0 none / 1 from launch 1 / 2 mixed), loop, hist_grid (smallest grid sized from the previous run's lists, 0 if
        none), longest (list a launch had to serve), overflows (launches whose list was longer than such a grid), tiles,
        tile_rows, waves, panels, frames."""
        v = (C.c_int * len(SCHEDULE_FIELDS))()
        _ck(self.lib.hc_last_hysteresis_schedule(self.handle, v, len(SCHEDULE_FIELDS)))
        return dict(zip(SCHEDULE_FIELDS, (int(x) for x in v)))

    def profile_get_front(self):
        """([k_blur_ms_sum, k_nms_ms_sum], nruns) of the profiled runs that took the split front path; call before
        profile_get(reset=True)."""
        sums = (C.c_double * 2)()
        n = C.c_long()
        _ck(self.lib.hc_profile_get_front(self.handle, sums, C.byref(n)))
        return [sums[0], sums[1]], n.value

    def upload(self, frames):
        """frames: (n,H,W) / (n,H,W,3) uint8, or a single frame."""
        a = np.ascontiguousarray(frames, dtype=np.uint8)
        if a.ndim == (2 if self.c == 1 else 3):
            a = a[None]
        exp = (self.h, self.w) if self.c == 1 else (self.h, self.w, 3)
        if a.shape[1:] != exp:
            raise HipCannyError(f"Cannot load image to GPU, specs different since initialization: {a.shape[1:]} vs {exp}")
        row = self.w * self.c
        _ck(self.lib.hc_upload(self.handle, a.ctypes.data, row, row * self.h, a.shape[0]))
        self._keep = a
        return a.shape[0]

    def run(self, final_stage=CannyStage.HYSTER, nframes=1):
        _ck(self.lib.hc_run(self.handle, int(final_stage), int(nframes)))

    def download(self, nframes=1):
        """nframes output images (in per-channel mode: 3 per input frame)."""
        out = np.empty((nframes, self.h, self.w), np.uint8)
        _ck(self.lib.hc_download(self.handle, out.ctypes.data, self.w, self.w * self.h, nframes))
        return out

    def sync(self):
        _ck(self.lib.hc_sync(self.handle))

    def run_device(self, d_in, in_pitch, in_fs, d_out, out_pitch, out_fs, nframes, final_stage=CannyStage.HYSTER):
        _ck(self.lib.hc_run_device(self.handle, C.c_void_p(d_in), in_pitch, in_fs, C.c_void_p(d_out), out_pitch, out_fs,
                                   int(nframes), int(final_stage)))

    def run_gradients_device(self, d_dx, d_dy, pitch, fs, d_out, out_pitch, out_fs, nframes):
        """cv::Canny(dx, dy, edges, low, high, L2gradient) on device memory (mode O): int16 dx / dy planes with the same
        pitch / frame stride in bytes -> u8 edge maps (hc_run_gradients_device).  Asynchronous, as run_device."""
        _ck(self.lib.hc_run_gradients_device(self.handle, C.c_void_p(d_dx), C.c_void_p(d_dy), pitch, fs, C.c_void_p(d_out),
                                             out_pitch, out_fs, int(nframes)))

    def process_gradients(self, dx, dy):
        """cv::Canny(dx, dy, ...) convenience (mode O): numpy int16 (n,H,W) / (n,H,W,3) -- or one frame -- in, uint8
        (n,H,W) edge maps out, through device tensors."""
        tx, n, pitch, fs = self._device_view(dx, "process_gradients: dx", np.int16)
        ty, ny, _, _ = self._device_view(dy, "process_gradients: dy", np.int16)
        if ny != n:
            raise HipCannyError(f"process_gradients: {n} dx planes, {ny} dy planes")
        out = self._device_maps(n)
        self._wait_for_torch()
        self.run_gradients_device(tx.data_ptr(), ty.data_ptr(), pitch, fs, out.data_ptr(), self.w, self.w * self.h, n)
        self.sync()
        return out.cpu().numpy()

    def derivatives_device(self, d_in, in_pitch, in_fs, d_dx, d_dy, pitch, fs, nframes, ksize):
        """The derivatives cv::Canny computes before its NMS (hc_derivatives_device): u8 frames on the device -> int16 dx / dy
        planes with the same channel interleave; ksize 3, 5, 7 (scaled by 1/16, half to even) or -1 (Scharr).  Pitches and
        frame strides in bytes.  Asynchronous on the context stream; not a run."""
        _ck(self.lib.hc_derivatives_device(self.handle, C.c_void_p(d_in), in_pitch, in_fs, C.c_void_p(d_dx), C.c_void_p(d_dy),
                                           pitch, fs, int(nframes), int(ksize)))

    def _frames_u8(self, frames, who, dtype=np.uint8):
        """(n,H,W) / (n,H,W,3) frames -- or one frame -- of the context's shape.  uint8: converted; int16: required as they come."""
        shape = (self.h, self.w) if self.c == 1 else (self.h, self.w, 3)
        a = np.ascontiguousarray(frames, dtype=np.uint8 if dtype == np.uint8 else None)
        if a.dtype != dtype:
            raise HipCannyError(f"{who}: must be int16 (CV_16SC1 / CV_16SC3), not {a.dtype}")
        if a.ndim == len(shape):
            a = a[None]
        if a.shape[1:] != shape:
            raise HipCannyError(f"{who}: frames {a.shape} do not match the context's {shape}")
        return a

    def _device_view(self, frames, who, dtype=np.uint8):
        """Host frames as a tight device view: (torch tensor, n, row bytes, frame stride in bytes)."""
        import torch
        a = self._frames_u8(frames, who, dtype)
        row = self.c * self.w * a.itemsize
        return torch.from_numpy(a).to(torch.device("cuda", self.device)), a.shape[0], row, row * self.h

    def _device_maps(self, n):
        """Uninitialised uint8 (n,H,W) maps on the device: pitch W, frame stride W * H."""
        import torch
        return torch.empty((n, self.h, self.w), dtype=torch.uint8, device=torch.device("cuda", self.device))

    @staticmethod
    def _wait_for_torch():   # the context stream does not wait for torch's: uploads and allocations first, then its calls
        import torch
        torch.cuda.current_stream().synchronize()

    def _maps_on_device(self, maps, who):
        """Host or torch u8 maps [n, H, W] (or one map) as a contiguous u8 tensor [n, H, W] on the context's device."""
        import torch
        dev = torch.device("cuda", self.device)
        if isinstance(maps, torch.Tensor):
            d = maps.to(device=dev, dtype=torch.uint8).contiguous()
            if d.ndim == 2:
                d = d[None]
        else:
            a = np.ascontiguousarray(maps, dtype=np.uint8)
            d = torch.from_numpy(a[None] if a.ndim == 2 else a).to(dev)
        if d.ndim != 3 or tuple(d.shape[1:]) != (self.h, self.w):
            raise HipCannyError(f"{who}: maps {tuple(d.shape)} do not match the context's {(self.h, self.w)}")
        return d

    def _largest_count(self, counts):
        """The largest of the uint32 counts a counts pass queued on the context stream writes into a device tensor: they size
        the buffer of the pass that follows."""
        self.sync()
        return int(counts.cpu().numpy().view(np.uint32).max())

    def _again_if_continued(self, fn):
        """fn(), once more if the last run was continued from the host (adversarial content): its maps changed after fn read them."""
        result = fn()
        return fn() if self.hysteresis_info()[1] else result

    @staticmethod
    def _count_or_error(r):   # the getters that return a non-negative int or an error code
        if r < 0:
            _ck(r)
        return r

    def derivatives(self, frames, ksize):
        """numpy u8 (n,H,W) / (n,H,W,3) -- or one frame -- in, (dx, dy) numpy int16 of the same shape out, through device
        tensors (either mode)."""
        import torch
        src, n, row, fs = self._device_view(frames, "derivatives")
        dx, dy = torch.empty_like(src, dtype=torch.int16), torch.empty_like(src, dtype=torch.int16)
        self._wait_for_torch()
        self.derivatives_device(src.data_ptr(), row, fs, dx.data_ptr(), dy.data_ptr(), 2 * row, 2 * fs, n, ksize)
        self.sync()
        return dx.cpu().numpy(), dy.cpu().numpy()

    def process_aperture(self, frames, ksize):
        """cv::Canny(img, low, high, ksize, L2gradient) for any of its apertures (mode O): frames -> derivatives ->
        run_gradients_device -> uint8 (n,H,W) edge maps, with no host round trip in between.  Uses the context's thresholds
        as they are (at 7 they are in the units of the scaled derivatives: see hc_derivatives_device)."""
        import torch
        src, n, row, fs = self._device_view(frames, "process_aperture")
        dx, dy = torch.empty_like(src, dtype=torch.int16), torch.empty_like(src, dtype=torch.int16)
        out = self._device_maps(n)
        self._wait_for_torch()
        self.derivatives_device(src.data_ptr(), row, fs, dx.data_ptr(), dy.data_ptr(), 2 * row, 2 * fs, n, ksize)
        self.run_gradients_device(dx.data_ptr(), dy.data_ptr(), 2 * row, 2 * fs, out.data_ptr(), self.w, self.w * self.h, n)
        self.sync()
        return out.cpu().numpy()

    def gaussian_blur_device(self, d_in, in_pitch, in_fs, d_out, out_pitch, out_fs, nframes, ksize, taps, border=BORDER_REFLECT_101):
        """cv::GaussianBlur's fixed-point path for u8 frames on device memory (hc_gaussian_blur_device, either mode): ksize 3, 5
        or 7, `taps` ksize Q8 values (256 = 1.0, sum 256: gaussian_taps_q8), the same along x and y.  Pitches and frame strides
        in bytes, any alignment; the views must not overlap.  Asynchronous on the context stream; not a run."""
        vals = [int(v) for v in taps]
        if any(v < 0 or v > 0xFFFF for v in vals) or (int(ksize) in _FIXED_TAPS_Q8 and len(vals) != int(ksize)):
            raise HipCannyError(f"hc_gaussian_blur_device: `taps` must hold ksize = {int(ksize)} uint16 values, not {vals}")
        t = (C.c_uint16 * max(len(vals), 1))(*vals)
        _ck(self.lib.hc_gaussian_blur_device(self.handle, C.c_void_p(d_in), in_pitch, in_fs, C.c_void_p(d_out), out_pitch, out_fs,
                                             int(nframes), int(ksize), t, int(border)))

    def gaussian_blur(self, frames, ksize, sigma=0.0, border=BORDER_REFLECT_101, taps=None):
        """numpy u8 (n,H,W) / (n,H,W,3) -- or one frame -- in, the blurred frames of the same shape out, through device tensors
        (either mode).  taps: ksize Q8 values instead of gaussian_taps_q8(ksize, sigma)."""
        import torch
        src, n, row, fs = self._device_view(frames, "gaussian_blur")
        out = torch.empty_like(src)
        self._wait_for_torch()
        self.gaussian_blur_device(src.data_ptr(), row, fs, out.data_ptr(), row, fs, n, ksize,
                                  gaussian_taps_q8(ksize, sigma) if taps is None else taps, border)
        self.sync()
        return out.cpu().numpy()

    def _blurred(self, src, n, row, fs, blur, border=BORDER_REFLECT_101):
        """Queues the blur = (ksize, sigma) of a tight device view into a scratch tensor on the context stream and returns the
        tensor; blur None: src itself, nothing queued.  The caller has waited for torch's stream."""
        import torch
        if blur is None:
            return src
        ksize, sigma = blur
        taps = gaussian_taps_q8(ksize, sigma)
        tmp = torch.empty_like(src)
        self._wait_for_torch()
        self.gaussian_blur_device(src.data_ptr(), row, fs, tmp.data_ptr(), row, fs, n, ksize, taps, border)
        return tmp

    def blur_canny(self, frames, ksize, sigma, low, high, aperture=3, l2gradient=False, border=BORDER_REFLECT_101):
        """cv::GaussianBlur(.., Size(ksize, ksize), sigma) followed by cv::Canny(.., low, high, aperture, l2gradient) (mode O):
        gaussian_blur_device into a scratch tensor, then canny_device, queued back to back on the context stream with no
        synchronisation in between.  numpy u8 frames in, uint8 (n,H,W) edge maps out."""
        src, n, row, fs = self._device_view(frames, "blur_canny")
        out = self._device_maps(n)
        self._wait_for_torch()
        tmp = self._blurred(src, n, row, fs, (ksize, sigma), border)
        self.canny_device(tmp.data_ptr(), row, fs, out.data_ptr(), self.w, self.w * self.h, n, low, high, aperture, l2gradient)
        self.sync()
        return out.cpu().numpy()

    def canny_device(self, d_in, in_pitch, in_fs, d_out, out_pitch, out_fs, nframes, low, high, aperture=3, l2gradient=False):
        """cv::Canny(img, edges, low, high, aperture, l2gradient) on device memory (mode O, hc_canny_device): thresholds in
        cv::Canny's units, aperture 3, 5, 7 or -1 (Scharr), all per call -- the context's thresholds and options are neither
        read nor changed.  Apertures 7 / -1 run one fused kernel (FORM_O_APERTURE7 / FORM_O_SCHARR).  Asynchronous, as run_device."""
        _ck(self.lib.hc_canny_device(self.handle, C.c_void_p(d_in), in_pitch, in_fs, C.c_void_p(d_out), out_pitch, out_fs,
                                     int(nframes), float(low), float(high), int(aperture), int(bool(l2gradient))))

    def canny(self, frames, low, high, aperture=3, l2gradient=False):
        """cv::Canny convenience (mode O): numpy u8 (n,H,W) / (n,H,W,3) -- or one frame -- in, uint8 (n,H,W) edge maps out,
        through device tensors and canny_device."""
        src, n, row, fs = self._device_view(frames, "canny")
        out = self._device_maps(n)
        self._wait_for_torch()
        self.canny_device(src.data_ptr(), row, fs, out.data_ptr(), self.w, self.w * self.h, n, low, high, aperture, l2gradient)
        self.sync()
        return out.cpu().numpy()

    def frame_thresholds_device(self, d_thr, nframes=0):
        """Per-frame thresholds for the runs that follow (mode O, hc_frame_thresholds_device): d_thr is device memory, int32
        [nframes][2] = (low, high) per frame, read by each run's front kernel on the context stream.  None / 0: back to the
        context's pair."""
        _ck(self.lib.hc_frame_thresholds_device(self.handle, C.c_void_p(d_thr or None), int(nframes)))

    def histogram_device(self, d_in, in_pitch, in_fs, nframes, d_hist):
        """256-bin histograms of u8 frames on the device (hc_histogram_device): d_hist is uint32 [nframes][256], the channels
        of 3-channel frames pooled.  Any alignment of the input view.  Asynchronous on the context stream; not a run."""
        _ck(self.lib.hc_histogram_device(self.handle, C.c_void_p(d_in), in_pitch, in_fs, int(nframes), C.c_void_p(d_hist)))

    def auto_thresholds_device(self, d_in, in_pitch, in_fs, nframes, rule, param, d_thr):
        """Automatic (low, high) per frame on the device (hc_auto_thresholds_device): rule AUTO_MEDIAN with param = sigma, or
        AUTO_OTSU with param = ratio; d_thr is int32 [nframes][2], as frame_thresholds_device reads it.  Asynchronous on the
        context stream; not a run."""
        _ck(self.lib.hc_auto_thresholds_device(self.handle, C.c_void_p(d_in), in_pitch, in_fs, int(nframes), int(rule), float(param),
                                               C.c_void_p(d_thr)))

    def histogram(self, frames):
        """numpy u8 (n,H,W) / (n,H,W,3) -- or one frame -- in, uint32 (n,256) histograms out, through device tensors."""
        import torch
        src, n, row, fs = self._device_view(frames, "histogram")
        hist = torch.empty((n, 256), dtype=torch.int32, device=src.device)
        self._wait_for_torch()
        self.histogram_device(src.data_ptr(), row, fs, n, hist.data_ptr())
        self.sync()
        return hist.cpu().numpy().view(np.uint32)

    def canny_auto(self, frames, rule="median", param=0.33, blur=None):
        """cv::Canny with thresholds chosen per frame on the device (mode O): auto thresholds -> per-frame table -> run, queued
        back to back on the context stream with no host synchronisation in between.  rule: "median" (param = sigma) or "otsu"
        (param = ratio), or AUTO_MEDIAN / AUTO_OTSU.  Returns (uint8 (n,H,W) edge maps, int32 (n,2) thresholds).  The
        context's aperture and L2 options apply; the table is taken off the context again before returning.
        blur = (ksize, sigma): the frames are blurred first (gaussian_blur_device, chained on the device too); thresholds and
        maps are those of the blurred frames."""
        import torch
        rule = {"median": AUTO_MEDIAN, "otsu": AUTO_OTSU}.get(rule, rule)
        raw, n, row, fs = self._device_view(frames, "canny_auto")
        thr = torch.empty((n, 2), dtype=torch.int32, device=raw.device)
        out = self._device_maps(n)
        self._wait_for_torch()
        src = self._blurred(raw, n, row, fs, blur)
        self.auto_thresholds_device(src.data_ptr(), row, fs, n, rule, param, thr.data_ptr())
        self.frame_thresholds_device(thr.data_ptr(), n)
        try:
            self.run_device(src.data_ptr(), row, fs, out.data_ptr(), self.w, self.w * self.h, n)
        finally:
            self.frame_thresholds_device(None)
        self.sync()
        return out.cpu().numpy(), thr.cpu().numpy()

    def edge_points_device(self, d_map, pitch, fs, nframes, d_counts, d_points, capacity):
        """cv::findNonZero / cv::countNonZero per frame on the device (hc_edge_points_device): d_map holds one-channel u8 maps
        (any alignment), d_counts is uint32 [nframes] (always the full counts), d_points int32 [nframes][capacity][2] = (x, y)
        in raster order, the first min(count, capacity) of each frame; capacity 0 (d_points None / 0): counts only.
        Asynchronous on the context stream; not a run, but a pipelined run in flight that writes the map is completed first."""
        _ck(self.lib.hc_edge_points_device(self.handle, C.c_void_p(d_map), pitch, fs, int(nframes), C.c_void_p(d_counts),
                                           C.c_void_p(d_points or None), int(capacity)))

    def _edge_points_of(self, d_maps, n, capacity):
        """(counts, lists) of n tight maps on the device (a torch u8 tensor [n, H, W] the context stream may read)."""
        import torch
        counts = torch.empty((n,), dtype=torch.int32, device=d_maps.device)
        fs = self.w * self.h
        if capacity is None:   # two passes: the counts size the list buffer
            self.edge_points_device(d_maps.data_ptr(), self.w, fs, n, counts.data_ptr(), None, 0)
            capacity = self._largest_count(counts)
        capacity = int(capacity)
        pts = torch.empty((n, max(capacity, 1), 2), dtype=torch.int32, device=d_maps.device)
        self._wait_for_torch()
        self.edge_points_device(d_maps.data_ptr(), self.w, fs, n, counts.data_ptr(), pts.data_ptr() if capacity else None, capacity)
        self.sync()
        cnt = counts.cpu().numpy().view(np.uint32)
        host = pts.cpu().numpy()
        return cnt, [host[f, :min(int(cnt[f]), capacity)].copy() for f in range(n)]

    def edge_points(self, maps, capacity=None):
        """Host or torch u8 maps [n, H, W] (or one map) in; (uint32 counts [n], [int32 array of shape (min(count_f, capacity), 2)
        = (x, y) per frame]) out.  capacity=None: two passes, counts first, then a list buffer sized by the largest count."""
        d = self._maps_on_device(maps, "edge_points")
        self._wait_for_torch()
        return self._edge_points_of(d, d.shape[0], capacity)

    def canny_points(self, frames, low, high, aperture=3, l2gradient=False, capacity=None, blur=None):
        """cv::Canny followed by cv::findNonZero (mode O): canny_device and edge_points_device chained on the device, with no
        host copy of the maps in between.  Returns (uint8 (n,H,W) edge maps, uint32 counts, lists as edge_points gives them).
        blur = (ksize, sigma): the frames are blurred first (gaussian_blur_device, chained on the device too)."""
        raw, n, row, fs = self._device_view(frames, "canny_points")
        out = self._device_maps(n)
        self._wait_for_torch()
        src = self._blurred(raw, n, row, fs, blur)   # (raw stays referenced until the call has synchronised)
        self.canny_device(src.data_ptr(), row, fs, out.data_ptr(), self.w, self.w * self.h, n, low, high, aperture, l2gradient)
        counts, lists = self._again_if_continued(lambda: self._edge_points_of(out, n, capacity))
        return out.cpu().numpy(), counts, lists

    def hough_lines_device(self, d_points, d_point_counts, point_capacity, nframes, rho, theta, threshold, min_theta, max_theta,
                           d_line_counts, d_lines, line_capacity):
        """cv::HoughLines' standard transform per frame on the device (hc_hough_lines_device, either mode), from what
        edge_points_device wrote: d_points int32 [nframes][point_capacity][2], d_point_counts uint32 [nframes].  d_line_counts is
        uint32 [nframes] (always the full number of peaks), d_lines float32 [nframes][line_capacity][3] = (rho, theta, votes),
        the strongest min(count, line_capacity) of each frame in cv::HoughLines' order; line_capacity 0 (d_lines None / 0):
        counts only.  Asynchronous on the context stream; not a run."""
        _ck(self.lib.hc_hough_lines_device(self.handle, C.c_void_p(d_points), C.c_void_p(d_point_counts), int(point_capacity), int(nframes),
                                           float(rho), float(theta), int(threshold), float(min_theta), float(max_theta),
                                           C.c_void_p(d_line_counts), C.c_void_p(d_lines or None), int(line_capacity)))

    def _lines_on_device(self, d_maps, n, rho, theta, threshold, min_theta, max_theta, max_lines, point_capacity):
        """Edge points, then lines, of n tight maps on the device, chained on the context stream and not waited for: (uint32
        line counts as an int32 tensor [n], float32 lines [n, max(capacity, 1), 3], capacity, the point lists)."""
        import torch
        dev, fs = d_maps.device, self.w * self.h
        pcounts = torch.empty((n,), dtype=torch.int32, device=dev)
        lcounts = torch.empty((n,), dtype=torch.int32, device=dev)
        if point_capacity is None:   # the counts size the list buffer
            self._wait_for_torch()
            self.edge_points_device(d_maps.data_ptr(), self.w, fs, n, pcounts.data_ptr(), None, 0)
            point_capacity = self._largest_count(pcounts)
        pcap = max(int(point_capacity), 1)
        pts = torch.empty((n, pcap, 2), dtype=torch.int32, device=dev)
        geo = (float(rho), float(theta), int(threshold), float(min_theta), float(max_theta))
        self._wait_for_torch()
        self.edge_points_device(d_maps.data_ptr(), self.w, fs, n, pcounts.data_ptr(), pts.data_ptr(), pcap)
        if max_lines is None:        # likewise: a counts pass first
            self.hough_lines_device(pts.data_ptr(), pcounts.data_ptr(), pcap, n, *geo, lcounts.data_ptr(), None, 0)
            max_lines = self._largest_count(lcounts)
        cap = int(max_lines)
        lines = torch.empty((n, max(cap, 1), 3), dtype=torch.float32, device=dev)
        self._wait_for_torch()
        self.hough_lines_device(pts.data_ptr(), pcounts.data_ptr(), pcap, n, *geo, lcounts.data_ptr(), lines.data_ptr() if cap else None, cap)
        return lcounts, lines, cap, (pts, pcounts)   # (the queued kernels read the lists: referenced until the caller has synchronised)

    def _hough_lines_of(self, d_maps, n, rho, theta, threshold, min_theta, max_theta, max_lines, point_capacity):
        """(counts, lines) of n tight maps on the device: edge points, then lines, chained on the context stream."""
        lcounts, lines, cap, _lists = self._lines_on_device(d_maps, n, rho, theta, threshold, min_theta, max_theta, max_lines, point_capacity)
        self.sync()
        cnt = lcounts.cpu().numpy().view(np.uint32)
        host = lines.cpu().numpy()
        return cnt, [host[f, :min(int(cnt[f]), cap)].copy() for f in range(n)]

    def hough_lines(self, maps, rho, theta, threshold, min_theta=0.0, max_theta=math.pi, max_lines=None, point_capacity=None):
        """cv::HoughLines(map, lines, rho, theta, threshold, 0, 0, min_theta, max_theta) per map: host or torch u8 maps [n, H, W]
        (or one map) in; (uint32 counts [n], [float32 (min(count_f, max_lines), 3) = (rho, theta, votes) per frame]) out --
        edge_points_device then hough_lines_device on the device.  max_lines=None: a counts pass first, then a buffer sized by the
        largest count; point_capacity=None likewise for the point lists (a smaller one cuts them: the lines are then those of
        the cut lists)."""
        d = self._maps_on_device(maps, "hough_lines")
        return self._hough_lines_of(d, d.shape[0], rho, theta, threshold, min_theta, max_theta, max_lines, point_capacity)

    def canny_lines(self, frames, low, high, rho, theta, threshold, aperture=3, l2gradient=False, blur=None, min_theta=0.0, max_theta=math.pi,
                    max_lines=None, point_capacity=None):
        """cv::GaussianBlur (blur = (ksize, sigma), optional), cv::Canny, cv::findNonZero and cv::HoughLines chained on the device
        (mode O), with no host copy of maps or point lists in between.  Returns (uint8 (n,H,W) edge maps, uint32 line counts,
        lines as hough_lines gives them)."""
        raw, n, row, fs = self._device_view(frames, "canny_lines")
        out = self._device_maps(n)
        self._wait_for_torch()
        src = self._blurred(raw, n, row, fs, blur)   # (raw stays referenced until the call has synchronised)
        self.canny_device(src.data_ptr(), row, fs, out.data_ptr(), self.w, self.w * self.h, n, low, high, aperture, l2gradient)
        tail = (rho, theta, threshold, min_theta, max_theta, max_lines, point_capacity)
        counts, lines = self._again_if_continued(lambda: self._hough_lines_of(out, n, *tail))
        return out.cpu().numpy(), counts, lines

    def hough_segments_device(self, d_map, pitch, fs, d_lines, d_line_counts, line_capacity, nframes, rho, theta, min_theta, max_theta,
                              min_length, max_gap, d_seg_counts, d_segs, seg_capacity):
        """Line segments per frame on the device (hc_hough_segments_device, either mode): the lines hough_lines_device wrote
        (d_lines float32 [nframes][line_capacity][3], d_line_counts uint32 [nframes], made with the same rho, theta, min_theta,
        max_theta) walked over the one-channel u8 maps d_map (any alignment) and cut by max_gap and min_length.  d_seg_counts is
        uint32 [nframes] (always the full counts), d_segs int32 [nframes][seg_capacity][4] = (x0, y0, x1, y1) by line, then along
        the line, the first min(count, seg_capacity) of each frame; seg_capacity 0 (d_segs None / 0): counts only.  Asynchronous
        on the context stream; not a run, but a pipelined run in flight that writes the map is completed first."""
        _ck(self.lib.hc_hough_segments_device(self.handle, C.c_void_p(d_map), pitch, fs, C.c_void_p(d_lines), C.c_void_p(d_line_counts),
                                              int(line_capacity), int(nframes), float(rho), float(theta), float(min_theta), float(max_theta),
                                              int(min_length), int(max_gap), C.c_void_p(d_seg_counts), C.c_void_p(d_segs or None), int(seg_capacity)))

    def _hough_segments_of(self, d_maps, n, rho, theta, threshold, min_length, max_gap, min_theta, max_theta, max_lines, max_segments, point_capacity):
        """(counts, segments) of n tight maps on the device: edge points, lines, then segments, chained on the context stream."""
        import torch
        lcounts, lines, lcap, _lists = self._lines_on_device(d_maps, n, rho, theta, threshold, min_theta, max_theta, max_lines, point_capacity)
        scounts = torch.zeros((n,), dtype=torch.int32, device=d_maps.device)
        segs = None
        cap = 0
        if lcap:   # (max_lines 0: no line is walked, no segment found)
            walk = (d_maps.data_ptr(), self.w, self.w * self.h, lines.data_ptr(), lcounts.data_ptr(), lcap, n, float(rho), float(theta), float(min_theta),
                    float(max_theta), int(min_length), int(max_gap), scounts.data_ptr())
            self._wait_for_torch()
            if max_segments is None:     # a counts pass first, as for the lines
                self.hough_segments_device(*walk, None, 0)
                max_segments = self._largest_count(scounts)
            cap = int(max_segments)
            segs = torch.empty((n, max(cap, 1), 4), dtype=torch.int32, device=d_maps.device)
            self._wait_for_torch()
            self.hough_segments_device(*walk, segs.data_ptr() if cap else None, cap)
        self.sync()
        cnt = scounts.cpu().numpy().view(np.uint32)
        host = segs.cpu().numpy() if cap else np.empty((n, 0, 4), np.int32)
        return cnt, [host[f, :min(int(cnt[f]), cap)].copy() for f in range(n)]

    def hough_segments(self, maps, rho, theta, threshold, min_length, max_gap, min_theta=0.0, max_theta=math.pi, max_lines=None, max_segments=None,
                       point_capacity=None):
        """Line segments per map: host or torch u8 maps [n, H, W] (or one map) in; (uint32 counts [n], [int32 (min(count_f,
        max_segments), 4) = (x0, y0, x1, y1) per frame]) out -- edge_points_device, hough_lines_device (rho, theta, threshold,
        min_theta, max_theta) and hough_segments_device (min_length, max_gap) on the device.  max_segments=None: a counts pass
        first, then a buffer sized by the largest count; max_lines and point_capacity likewise, as in hough_lines (smaller ones
        cut the lists: the segments are then those of the cut lists)."""
        d = self._maps_on_device(maps, "hough_segments")
        return self._hough_segments_of(d, d.shape[0], rho, theta, threshold, min_length, max_gap, min_theta, max_theta, max_lines, max_segments, point_capacity)

    def canny_segments(self, frames, low, high, rho, theta, threshold, min_length, max_gap, aperture=3, l2gradient=False, blur=None, min_theta=0.0,
                       max_theta=math.pi, max_lines=None, max_segments=None, point_capacity=None):
        """cv::GaussianBlur (blur = (ksize, sigma), optional), cv::Canny, cv::findNonZero, cv::HoughLines and the segment walk
        chained on the device (mode O), with no host copy of maps, point lists or lines in between.  Returns (uint8 (n,H,W) edge
        maps, uint32 segment counts, segments as hough_segments gives them)."""
        raw, n, row, fs = self._device_view(frames, "canny_segments")
        out = self._device_maps(n)
        self._wait_for_torch()
        src = self._blurred(raw, n, row, fs, blur)   # (raw stays referenced until the call has synchronised)
        self.canny_device(src.data_ptr(), row, fs, out.data_ptr(), self.w, self.w * self.h, n, low, high, aperture, l2gradient)
        tail = (rho, theta, threshold, min_length, max_gap, min_theta, max_theta, max_lines, max_segments, point_capacity)
        counts, segs = self._again_if_continued(lambda: self._hough_segments_of(out, n, *tail))
        return out.cpu().numpy(), counts, segs

    def hough_circles_device(self, d_points, d_point_counts, point_capacity, d_dx, d_dy, pitch, fs, nframes, dp, min_dist, votes_threshold,
                             min_radius, max_radius, centre_capacity, d_circle_counts, d_circles, circle_capacity):
        """Circles per frame on the device (hc_hough_circles_device, either mode; the form of cv::cuda::HoughCirclesDetector), from
        what edge_points_device wrote (d_points int32 [nframes][point_capacity][2], d_point_counts uint32 [nframes]) and the
        one-channel int16 gradient planes d_dx / d_dy (pitch and frame stride in bytes: derivatives_device on a 1-channel
        context).  d_circle_counts is uint32 [nframes] (always the full counts), d_circles float32 [nframes][circle_capacity][4] =
        (x, y, radius, votes) by centre (votes descending), then by radius, the first min(count, circle_capacity) of each frame;
        circle_capacity 0 (d_circles None / 0): counts only.  Asynchronous on the context stream; not a run."""
        _ck(self.lib.hc_hough_circles_device(self.handle, C.c_void_p(d_points), C.c_void_p(d_point_counts), int(point_capacity), C.c_void_p(d_dx),
                                             C.c_void_p(d_dy), pitch, fs, int(nframes), float(dp), float(min_dist), int(votes_threshold), int(min_radius),
                                             int(max_radius), int(centre_capacity), C.c_void_p(d_circle_counts), C.c_void_p(d_circles or None),
                                             int(circle_capacity)))

    def _hough_circles_of(self, d_maps, d_dx, d_dy, n, dp, min_dist, votes_threshold, min_radius, max_radius, max_centres, max_circles, point_capacity):
        """(counts, circles) of n tight maps and tight int16 planes on the device: edge points, then circles, chained on the
        context stream."""
        import torch
        dev, fs = d_maps.device, self.w * self.h
        pcounts = torch.empty((n,), dtype=torch.int32, device=dev)
        ccounts = torch.empty((n,), dtype=torch.int32, device=dev)
        self._wait_for_torch()
        if point_capacity is None:   # the counts size the list buffer
            self.edge_points_device(d_maps.data_ptr(), self.w, fs, n, pcounts.data_ptr(), None, 0)
            point_capacity = self._largest_count(pcounts)
        pcap = max(int(point_capacity), 1)
        pts = torch.empty((n, pcap, 2), dtype=torch.int32, device=dev)
        self._wait_for_torch()
        self.edge_points_device(d_maps.data_ptr(), self.w, fs, n, pcounts.data_ptr(), pts.data_ptr(), pcap)
        call = (pts.data_ptr(), pcounts.data_ptr(), pcap, d_dx.data_ptr(), d_dy.data_ptr(), 2 * self.w, 2 * fs, n, dp, min_dist, votes_threshold, min_radius,
                max_radius, max_centres, ccounts.data_ptr())
        if max_circles is None:      # likewise: a counts pass first
            self.hough_circles_device(*call, None, 0)
            max_circles = self._largest_count(ccounts)
        cap = int(max_circles)
        circles = torch.empty((n, max(cap, 1), 4), dtype=torch.float32, device=dev)
        self._wait_for_torch()
        self.hough_circles_device(*call, circles.data_ptr() if cap else None, cap)
        self.sync()
        cnt = ccounts.cpu().numpy().view(np.uint32)
        host = circles.cpu().numpy()
        return cnt, [host[f, :min(int(cnt[f]), cap)].copy() for f in range(n)]

    def _planes_on_device(self, planes, n, who):
        """Host or torch int16 planes [n, H, W] (or one plane) as a contiguous int16 tensor [n, H, W] on the context's device."""
        import torch
        dev = torch.device("cuda", self.device)
        if isinstance(planes, torch.Tensor):
            d = planes if planes.ndim == 3 else planes[None]
            if d.dtype != torch.int16:
                raise HipCannyError(f"{who}: must be int16 (CV_16SC1), not {d.dtype}")
            d = d.to(dev).contiguous()
        else:
            a = np.ascontiguousarray(planes)
            if a.dtype != np.int16:
                raise HipCannyError(f"{who}: must be int16 (CV_16SC1), not {a.dtype}")
            d = torch.from_numpy(a[None] if a.ndim == 2 else a).to(dev)
        if tuple(d.shape) != (n, self.h, self.w):
            raise HipCannyError(f"{who}: planes {tuple(d.shape)} do not match the maps' {(n, self.h, self.w)}")
        return d

    def hough_circles(self, maps, dx, dy, dp, min_dist, votes_threshold, min_radius, max_radius, max_centres=4096, max_circles=None, point_capacity=None):
        """Circles per map (the form of cv::cuda::HoughCirclesDetector): host or torch u8 edge maps [n, H, W] (or one map) and the
        int16 gradient planes dx, dy of the same shape in; (uint32 counts [n], [float32 (min(count_f, max_circles), 4) = (x, y,
        radius, votes) per frame]) out -- edge_points_device then hough_circles_device on the device.  max_centres: the strongest
        centres that go on to the smallest-distance rule (1 .. 4096).  max_circles=None: a counts pass first, then a buffer sized
        by the largest count; point_capacity=None likewise for the point lists (a smaller one cuts them: the circles are then
        those of the cut lists)."""
        d = self._maps_on_device(maps, "hough_circles")
        n = d.shape[0]
        gx, gy = self._planes_on_device(dx, n, "hough_circles: dx"), self._planes_on_device(dy, n, "hough_circles: dy")
        return self._hough_circles_of(d, gx, gy, n, dp, min_dist, votes_threshold, min_radius, max_radius, max_centres, max_circles, point_capacity)

    def canny_circles(self, frames, low, high, dp, min_dist, votes_threshold, min_radius, max_radius, aperture=3, l2gradient=False, blur=None,
                      max_centres=4096, max_circles=None, point_capacity=None):
        """cv::GaussianBlur (blur = (ksize, sigma), optional), the derivatives of cv::Canny's aperture, cv::Canny, cv::findNonZero
        and the circle transform chained on the device (mode O, 1-channel contexts), with no host copy of maps, planes or point
        lists in between.  Returns (uint8 (n,H,W) edge maps, uint32 circle counts, circles as hough_circles gives them)."""
        import torch
        if self.c != 1:
            raise ValueError("canny_circles: a 1-channel context is required (the derivative planes of 3-channel frames are interleaved)")
        raw, n, row, fs = self._device_view(frames, "canny_circles")
        out = self._device_maps(n)
        gx, gy = torch.empty_like(raw, dtype=torch.int16), torch.empty_like(raw, dtype=torch.int16)
        self._wait_for_torch()
        src = self._blurred(raw, n, row, fs, blur)   # (raw stays referenced until the call has synchronised)
        self.derivatives_device(src.data_ptr(), row, fs, gx.data_ptr(), gy.data_ptr(), 2 * row, 2 * fs, n, aperture)
        self.canny_device(src.data_ptr(), row, fs, out.data_ptr(), self.w, self.w * self.h, n, low, high, aperture, l2gradient)
        tail = (dp, min_dist, votes_threshold, min_radius, max_radius, max_centres, max_circles, point_capacity)
        counts, circles = self._again_if_continued(lambda: self._hough_circles_of(out, gx, gy, n, *tail))
        return out.cpu().numpy(), counts, circles

    def connected_components_device(self, d_map, pitch, fs, nframes, connectivity, d_labels, label_pitch, label_fs, d_counts, d_stats=None,
                                    d_centroids=None, capacity=0):
        """cv::connectedComponentsWithStats per frame on the device (hc_connected_components_device): d_map holds one-channel u8
        maps (any alignment), d_labels receives int32 [H][W] per frame (pitch and frame stride in bytes, multiples of 4), d_counts
        uint32 [nframes] = components + 1, d_stats int32 [nframes][capacity][5] and d_centroids float64 [nframes][capacity][2] the
        rows 0 .. min(N, capacity) - 1 of each frame (row 0: the background).  Components are numbered in raster order of their
        first pixels.  capacity 0 (d_stats, d_centroids None / 0): labels and counts only.  Asynchronous on the context stream;
        not a run, but a pipelined run in flight that writes the map or the label plane is completed first."""
        _ck(self.lib.hc_connected_components_device(self.handle, C.c_void_p(d_map), pitch, fs, int(nframes), int(connectivity), C.c_void_p(d_labels),
                                                    label_pitch, label_fs, C.c_void_p(d_counts), C.c_void_p(d_stats or None),
                                                    C.c_void_p(d_centroids or None), int(capacity)))

    def _components_of(self, d_maps, n, connectivity, max_components):
        """(labels, counts, stats, centroids) of n tight maps on the device (a torch u8 tensor [n, H, W] the context stream may read)."""
        import torch
        dev = d_maps.device
        labels = torch.empty((n, self.h, self.w), dtype=torch.int32, device=dev)
        counts = torch.empty((n,), dtype=torch.int32, device=dev)
        fs = self.w * self.h
        self._wait_for_torch()
        if max_components is None:   # two passes: the counts size the rows
            self.connected_components_device(d_maps.data_ptr(), self.w, fs, n, connectivity, labels.data_ptr(), 4 * self.w, 4 * fs, counts.data_ptr())
            max_components = self._largest_count(counts)
        cap = int(max_components)
        stats = torch.empty((n, max(cap, 1), CC_STAT_WORDS), dtype=torch.int32, device=dev)
        cent = torch.empty((n, max(cap, 1), 2), dtype=torch.float64, device=dev)
        self._wait_for_torch()
        self.connected_components_device(d_maps.data_ptr(), self.w, fs, n, connectivity, labels.data_ptr(), 4 * self.w, 4 * fs, counts.data_ptr(),
                                         stats.data_ptr() if cap else None, cent.data_ptr() if cap else None, cap)
        self.sync()
        cnt = counts.cpu().numpy().view(np.uint32)
        hs, hc = stats.cpu().numpy(), cent.cpu().numpy()
        rows = [min(int(cnt[f]), cap) for f in range(n)]
        return labels.cpu().numpy(), cnt, [hs[f, :rows[f]].copy() for f in range(n)], [hc[f, :rows[f]].copy() for f in range(n)]

    def connected_components(self, maps, connectivity=8, max_components=None):
        """Host or torch u8 maps [n, H, W] (or one map) in; (int32 labels [n, H, W], uint32 counts [n] = components + 1, [int32
        array (min(N_f, max_components), 5) = (left, top, width, height, area) per frame], [float64 array (.., 2) = centroid (x, y)
        per frame]) out; row 0 is the background.  max_components=None: two passes, counts first, then rows sized by the largest."""
        d = self._maps_on_device(maps, "connected_components")
        return self._components_of(d, d.shape[0], connectivity, max_components)

    def morphology_device(self, d_in, in_pitch, in_fs, d_out, out_pitch, out_fs, nframes, channels, op, ksize, spans):
        """cv::erode / cv::dilate / cv::morphologyEx (open, close, gradient) for u8 frames on device memory (hc_morphology_device,
        either mode): op MORPH_ERODE .. MORPH_GRADIENT, ksize 3, 5 or 7, `spans` the ksize half-widths of the element's rows (-1: an
        empty row; structuring_element gives OpenCV's shapes), channels 1 or 3 (3: a 3-channel context).  Constant border that never
        takes part.  Pitches and frame strides in bytes, any alignment; the views must not overlap.  Asynchronous on the context
        stream; not a run, but a pipelined run in flight that writes either view is completed first."""
        vals = [int(v) for v in spans]
        if any(v < -128 or v > 127 for v in vals) or (int(ksize) in _FIXED_TAPS_Q8 and len(vals) != int(ksize)):
            raise HipCannyError(f"hc_morphology_device: `spans` must hold ksize = {int(ksize)} int8 values, not {vals}")
        t = (C.c_int8 * max(len(vals), 1))(*vals)
        _ck(self.lib.hc_morphology_device(self.handle, C.c_void_p(d_in), in_pitch, in_fs, C.c_void_p(d_out), out_pitch, out_fs, int(nframes),
                                          int(channels), int(op), int(ksize), t))

    def _morphed(self, src, op, ksize, spans, iterations=1):
        """Queues `op` on a contiguous u8 device tensor (n,H,W) / (n,H,W,3) on the context stream, `iterations` times as
        cv::morphologyEx counts them, and returns the result tensor.  Every tensor the queued kernels touch is appended to
        self._morph_keep, which the caller clears once it has synchronised.  The caller has waited for torch's stream."""
        import torch
        n = src.shape[0]
        ch = 3 if src.ndim == 4 else 1
        row = ch * self.w
        fs = row * self.h
        if int(iterations) < 1:
            raise HipCannyError("morphology: iterations must be at least 1")
        if int(iterations) == 1:
            chain = [op]
        elif op in (MORPH_ERODE, MORPH_DILATE):
            chain = [op] * int(iterations)
        elif op == MORPH_OPEN:
            chain = [MORPH_ERODE] * int(iterations) + [MORPH_DILATE] * int(iterations)
        elif op == MORPH_CLOSE:
            chain = [MORPH_DILATE] * int(iterations) + [MORPH_ERODE] * int(iterations)
        elif op == MORPH_GRADIENT:   # dilate^n - erode^n: both chains, then the difference on torch's stream
            bufs = [self._morphed(src, o, ksize, spans, iterations) for o in (MORPH_DILATE, MORPH_ERODE)]
            self.sync()
            return (bufs[0].to(torch.int16) - bufs[1].to(torch.int16)).clamp_(min=0).to(torch.uint8)   # (saturated, as cv::subtract)
        else:
            raise HipCannyError("hc_morphology_device: op must be one of HC_MORPH_ERODE .. HC_MORPH_GRADIENT")
        keep = getattr(self, "_morph_keep", None)
        if keep is None:
            keep = self._morph_keep = []
        keep.append(src)
        cur = src
        for o in chain:
            dst = torch.empty_like(src)
            self._wait_for_torch()
            self.morphology_device(cur.data_ptr(), row, fs, dst.data_ptr(), row, fs, n, ch, o, ksize, spans)
            keep.append(dst)
            cur = dst
        return cur

    def morphology(self, frames_or_maps, op, shape=MORPH_RECT, ksize=3, iterations=1, spans=None):
        """numpy or torch u8 (n,H,W) / (n,H,W,3) -- or one frame -- in, the result of the same shape out (numpy), through device
        tensors (either mode).  spans: ksize half-widths instead of structuring_element(shape, ksize).  iterations > 1 chains the
        primitive calls on the device with no synchronisation in between, as cv::morphologyEx does: OPEN is `iterations` erosions
        then as many dilations, CLOSE the reverse, GRADIENT the difference of the iterated dilation and erosion."""
        import torch
        dev = torch.device("cuda", self.device)
        if isinstance(frames_or_maps, torch.Tensor):
            d = frames_or_maps.to(device=dev, dtype=torch.uint8)
        else:
            d = torch.from_numpy(np.ascontiguousarray(frames_or_maps, dtype=np.uint8)).to(dev)
        if d.ndim == 2 or (d.ndim == 3 and tuple(d.shape) == (self.h, self.w, 3)):
            d = d[None]
        d = d.contiguous()
        if d.ndim not in (3, 4) or tuple(d.shape[1:3]) != (self.h, self.w) or (d.ndim == 4 and d.shape[3] != 3):
            raise HipCannyError(f"morphology: frames {tuple(d.shape)} do not match the context's {(self.h, self.w)}")
        sp = structuring_element(shape, ksize) if spans is None else spans
        self._wait_for_torch()
        out = self._morphed(d, int(op), ksize, sp, iterations)
        self.sync()
        res = out.cpu().numpy()
        self._morph_keep = None
        return res

    def canny_components(self, frames, low, high, connectivity=8, aperture=3, l2gradient=False, blur=None, max_components=None, close=None, thin=None):
        """cv::Canny followed by cv::connectedComponentsWithStats (mode O): canny_device and connected_components_device chained on
        the device, with no host copy of the maps in between.  Returns (uint8 (n,H,W) edge maps, labels, counts, stats, centroids as
        connected_components gives them).  blur = (ksize, sigma): the frames are blurred first (gaussian_blur_device).
        close = (shape, ksize): cv::morphologyEx(MORPH_CLOSE) with that element runs between the two on the device
        (morphology_device), the components are those of the closed maps, and the closed maps are what the call returns.
        thin = a method name of thinning ("zhangsuen" / "guohall"): thinning_device (16 iterations at most) runs after the closing,
        and the components and the returned maps are those of the skeletons."""
        raw, n, row, fs = self._device_view(frames, "canny_components")
        out = self._device_maps(n)
        self._wait_for_torch()
        src = self._blurred(raw, n, row, fs, blur)   # (raw stays referenced until the call has synchronised)
        self.canny_device(src.data_ptr(), row, fs, out.data_ptr(), self.w, self.w * self.h, n, low, high, aperture, l2gradient)
        if close is None and thin is None:
            labels, counts, stats, cent = self._again_if_continued(lambda: self._components_of(out, n, connectivity, max_components))
            return out.cpu().numpy(), labels, counts, stats, cent
        spans = structuring_element(*close) if close is not None else None
        method = self._thin_method(thin) if thin is not None else None
        closed = self._device_maps(n) if close is not None else out
        last = self._device_maps(n) if thin is not None else closed

        def later_components():
            self._wait_for_torch()
            if close is not None:
                self.morphology_device(out.data_ptr(), self.w, self.w * self.h, closed.data_ptr(), self.w, self.w * self.h, n, 1, MORPH_CLOSE, close[1], spans)
            if thin is not None:
                self.thinning_device(closed.data_ptr(), self.w, self.w * self.h, last.data_ptr(), self.w, self.w * self.h, n, method, 16)
            return self._components_of(last, n, connectivity, max_components)
        labels, counts, stats, cent = self._again_if_continued(later_components)
        return last.cpu().numpy(), labels, counts, stats, cent

    def distance_transform_device(self, d_map, pitch, fs, nframes, target, dist_type, d_dist, dist_pitch, dist_fs, d_nearest=None, nearest_pitch=0,
                                  nearest_fs=0):
        """The exact Euclidean distance transform per frame on the device (hc_distance_transform_device): d_map holds one-channel
        u8 maps (any alignment); the feature pixels are its non-zero bytes (target DT_TO_NONZERO) or its zero bytes (DT_TO_ZERO).
        d_dist receives [H][W] per frame, the squared distance to the nearest feature pixel as int32 (dist_type DT_SQUARED_I32;
        DT_NONE in a frame without one) or its float32 root (DT_F32; +inf); d_nearest, when given, int32 [H][W] = y' * W + x' of
        that pixel (-1 in a frame without one), ties to the smallest x', then the smallest y'.  Output pitches and frame strides
        in bytes, multiples of 4.  Asynchronous on the context stream; not a run, but a pipelined run in flight that writes any
        of the views is completed first."""
        _ck(self.lib.hc_distance_transform_device(self.handle, C.c_void_p(d_map), pitch, fs, int(nframes), int(target), int(dist_type), C.c_void_p(d_dist),
                                                  dist_pitch, dist_fs, C.c_void_p(d_nearest or None), nearest_pitch, nearest_fs))

    def _distances_of(self, d_maps, n, target, squared, nearest):
        """(dist[, nearest]) of n tight maps on the device (a torch u8 tensor [n, H, W] the context stream may read), as numpy."""
        import torch
        dist = torch.empty((n, self.h, self.w), dtype=torch.int32 if squared else torch.float32, device=d_maps.device)
        near = torch.empty((n, self.h, self.w), dtype=torch.int32, device=d_maps.device) if nearest else None
        fs = self.w * self.h
        self._wait_for_torch()
        self.distance_transform_device(d_maps.data_ptr(), self.w, fs, n, target, DT_SQUARED_I32 if squared else DT_F32, dist.data_ptr(), 4 * self.w, 4 * fs,
                                       near.data_ptr() if nearest else None, 4 * self.w if nearest else 0, 4 * fs if nearest else 0)
        self.sync()
        return (dist.cpu().numpy(), near.cpu().numpy()) if nearest else dist.cpu().numpy()

    def distance_transform(self, maps, target=DT_TO_NONZERO, squared=False, nearest=False):
        """Host or torch u8 maps [n, H, W] (or one map) in; float32 distances [n, H, W] out (squared=True: the exact int32 squared
        distances), with nearest=True the pair (distances, int32 [n, H, W] indices y' * W + x' of the nearest feature pixel)."""
        d = self._maps_on_device(maps, "distance_transform")
        return self._distances_of(d, d.shape[0], target, squared, nearest)

    def canny_distance(self, frames, low, high, aperture=3, l2gradient=False, blur=None, squared=False, nearest=False):
        """cv::Canny followed by the distance of every pixel to the nearest edge pixel (mode O): canny_device and
        distance_transform_device chained on the device, with no host copy of the maps and no synchronisation in between.
        blur = (ksize, sigma): the frames are blurred first (gaussian_blur_device).  Returns (uint8 (n,H,W) edge maps, distances
        [, nearest]) as distance_transform gives them."""
        raw, n, row, fs = self._device_view(frames, "canny_distance")
        out = self._device_maps(n)
        self._wait_for_torch()
        src = self._blurred(raw, n, row, fs, blur)   # (raw stays referenced until the call has synchronised)
        self.canny_device(src.data_ptr(), row, fs, out.data_ptr(), self.w, self.w * self.h, n, low, high, aperture, l2gradient)
        res = self._again_if_continued(lambda: self._distances_of(out, n, DT_TO_NONZERO, squared, nearest))
        return (out.cpu().numpy(),) + (res if nearest else (res,))

    def thinning_device(self, d_map, pitch, fs, d_out, out_pitch, out_fs, nframes, method=THIN_ZHANGSUEN, max_iterations=16, d_status=None):
        """Zhang-Suen / Guo-Hall thinning of one-channel u8 maps on device memory (hc_thinning_device, either mode): a pixel is
        foreground iff its byte is non-zero, the output is 0 / 255; method THIN_ZHANGSUEN or THIN_GUOHALL; at most max_iterations
        (1..1024) iterations, every one of which is queued -- a cost, 16 suits closed Canny maps.  d_status, when given, receives
        uint32 [nframes][2] = (iterations that removed a pixel, 1 iff the output is known to be the fixed point).  Pitches and frame
        strides in bytes, any alignment; the views must not overlap.  Asynchronous on the context stream; not a run, but a
        pipelined run in flight that writes either view is completed first."""
        _ck(self.lib.hc_thinning_device(self.handle, C.c_void_p(d_map), pitch, fs, C.c_void_p(d_out), out_pitch, out_fs, int(nframes), int(method),
                                        int(max_iterations), C.c_void_p(d_status or None)))

    @staticmethod
    def _thin_method(method):
        if isinstance(method, str):
            if method.lower() not in THIN_METHODS:
                raise HipCannyError(f"thinning: method must be one of {sorted(THIN_METHODS)}, not {method!r}")
            return THIN_METHODS[method.lower()]
        return int(method)

    def thinning(self, maps, method="zhangsuen", max_iterations=16):
        """Host or torch u8 maps [n, H, W] (or one map) in; (uint8 0 / 255 skeleton maps [n, H, W], uint32 iterations [n], uint32
        converged [n]) out, as hc_thinning_device states them.  max_iterations=None: the call is repeated in chunks of 16
        iterations between two device buffers until every frame reports convergence -- one host synchronisation per chunk;
        `iterations` is then the sum over the chunks.  Every chunk is a whole call on the whole batch: frames that converged in
        an earlier chunk are packed and unpacked again (their step launches exit at once), so a batch pays a pack and an unpack
        per chunk of its slowest frame."""
        import torch
        d = self._maps_on_device(maps, "thinning")
        n, fs = d.shape[0], self.w * self.h
        m = self._thin_method(method)
        bufs = [self._device_maps(n), self._device_maps(n)]   # (the caller's tensor is never written)
        status = torch.empty((n, 2), dtype=torch.int32, device=d.device)
        total = np.zeros(n, np.uint32)
        src, k = d, 0
        while True:
            dst = bufs[k & 1]
            self._wait_for_torch()
            self.thinning_device(src.data_ptr(), self.w, fs, dst.data_ptr(), self.w, fs, n, m, 16 if max_iterations is None else max_iterations, status.data_ptr())
            self.sync()
            st = status.cpu().numpy().view(np.uint32)
            total += st[:, 0]
            if max_iterations is not None or st[:, 1].all():
                return dst.cpu().numpy(), total, st[:, 1].copy()
            src, k = dst, k + 1

    def canny_skeleton(self, frames, low, high, close=(MORPH_RECT, 3), method="zhangsuen", max_iterations=16, aperture=3, l2gradient=False, blur=None):
        """cv::Canny, cv::morphologyEx(MORPH_CLOSE) with the element close = (shape, ksize) and the thinning of the closed maps
        (mode O): canny_device, morphology_device and thinning_device chained on the device with no host copy and no
        synchronisation in between.  blur = (ksize, sigma): the frames are blurred first (gaussian_blur_device).  Returns (uint8
        (n,H,W) skeleton maps, uint32 iterations [n], uint32 converged [n]) as thinning gives them."""
        import torch
        raw, n, row, fs = self._device_view(frames, "canny_skeleton")
        m = self._thin_method(method)
        spans = structuring_element(*close)
        edges, closed, skel = self._device_maps(n), self._device_maps(n), self._device_maps(n)
        status = torch.empty((n, 2), dtype=torch.int32, device=edges.device)
        mfs = self.w * self.h
        self._wait_for_torch()
        src = self._blurred(raw, n, row, fs, blur)   # (raw stays referenced until the call has synchronised)
        self.canny_device(src.data_ptr(), row, fs, edges.data_ptr(), self.w, mfs, n, low, high, aperture, l2gradient)

        def skeleton():
            self._wait_for_torch()
            self.morphology_device(edges.data_ptr(), self.w, mfs, closed.data_ptr(), self.w, mfs, n, 1, MORPH_CLOSE, close[1], spans)
            self.thinning_device(closed.data_ptr(), self.w, mfs, skel.data_ptr(), self.w, mfs, n, m, max_iterations, status.data_ptr())
            self.sync()
            return skel.cpu().numpy(), status.cpu().numpy().view(np.uint32)
        maps, st = self._again_if_continued(skeleton)
        return maps, st[:, 0].copy(), st[:, 1].copy()

    def corner_response_device(self, d_dx, d_dy, pitch, fs, d_response, out_pitch, out_fs, nframes, block_size=3, method=CORNER_MIN_EIGEN, k=0.04):
        """cv::cornerMinEigenVal / cv::cornerHarris on given one-channel int16 derivative planes on device memory
        (hc_corner_response_device, either mode): block_size 3, 5 or 7 with a replicated border, exact integer window sums, no
        normalisation; float32 planes of W x H out.  Pitches and frame strides in bytes (input even, output multiples of 4); the
        views must not overlap.  Asynchronous on the context stream; not a run."""
        _ck(self.lib.hc_corner_response_device(self.handle, C.c_void_p(d_dx), C.c_void_p(d_dy), pitch, fs, C.c_void_p(d_response), out_pitch, out_fs,
                                               int(nframes), int(block_size), int(method), float(k)))

    def good_features_device(self, d_response, pitch, fs, nframes, quality_level, min_distance, candidate_capacity, d_corner_counts, d_corners,
                             d_quality, corner_capacity):
        """cv::goodFeaturesToTrack on float32 response planes of W x H on device memory (hc_good_features_device, either mode; the
        form of cv::cuda::CornersDetector): d_corner_counts uint32 [nframes] (always the full counts), d_corners float32
        [nframes][corner_capacity][2] = (x, y) by descending response, d_quality (or None) float32 [nframes][corner_capacity]
        their responses; corner_capacity 0 (d_corners None): counts only.  Only the strongest candidate_capacity (1 .. 4096) local
        maxima go on to the smallest-distance rule.  Asynchronous on the context stream; not a run."""
        _ck(self.lib.hc_good_features_device(self.handle, C.c_void_p(d_response), pitch, fs, int(nframes), float(quality_level), float(min_distance),
                                             int(candidate_capacity), C.c_void_p(d_corner_counts), C.c_void_p(d_corners or None), C.c_void_p(d_quality or None),
                                             int(corner_capacity)))

    @staticmethod
    def _corner_method(method):
        if isinstance(method, str):
            if method.lower() not in CORNER_METHODS:
                raise HipCannyError(f"corner_response: method must be one of {sorted(CORNER_METHODS)}, not {method!r}")
            return CORNER_METHODS[method.lower()]
        return int(method)

    def _feature_buffers(self, n, max_corners, candidate_capacity, dev):
        """(capacity, counts, corners, qualities): the output tensors of one good_features_device call"""
        import torch
        cap = int(candidate_capacity) if max_corners is None else int(max_corners)
        return (cap, torch.empty((n,), dtype=torch.int32, device=dev), torch.empty((n, max(cap, 1), 2), dtype=torch.float32, device=dev),
                torch.empty((n, max(cap, 1)), dtype=torch.float32, device=dev))

    def _queue_response(self, gx, gy, resp, n, block_size, method, k):
        """Queues the corner measure of tight int16 planes [n, H, W] into the tight float32 tensor resp; no host wait."""
        self.corner_response_device(gx.data_ptr(), gy.data_ptr(), 2 * self.w, 2 * self.w * self.h, resp.data_ptr(), 4 * self.w, 4 * self.w * self.h, n,
                                    block_size, method, k)

    def _queue_features(self, resp, n, quality_level, min_distance, candidate_capacity, bufs):
        """Queues the selection on a tight float32 tensor [n, H, W] into the tensors of _feature_buffers; no host wait."""
        cap, counts, corners, quality = bufs
        self.good_features_device(resp.data_ptr(), 4 * self.w, 4 * self.w * self.h, n, quality_level, min_distance, candidate_capacity, counts.data_ptr(),
                                  corners.data_ptr() if cap else None, quality.data_ptr() if cap else None, cap)

    def _features_from(self, n, bufs):
        """Waits for the context stream; ([float32 (count_f, 2) = (x, y)], [float32 (count_f,) responses]) of the tensors."""
        cap, counts, corners, quality = bufs
        self.sync()
        cnt = counts.cpu().numpy().view(np.uint32)
        xy, q = corners.cpu().numpy(), quality.cpu().numpy()
        keep = [min(int(cnt[f]), cap) for f in range(n)]
        return [xy[f, :keep[f]].copy() for f in range(n)], [q[f, :keep[f]].copy() for f in range(n)]

    def corner_response(self, dx, dy, block_size=3, method="min_eigen", k=0.04):
        """Host or torch int16 planes dx, dy [n, H, W] (or one plane each) in, the float32 corner measure [n, H, W] out as a torch
        tensor on the device (hc_corner_response_device): method "min_eigen" or "harris" (k: the Harris constant)."""
        import torch
        n = 1 if (dx.ndim if isinstance(dx, torch.Tensor) else np.asarray(dx).ndim) == 2 else len(dx)
        gx, gy = self._planes_on_device(dx, n, "corner_response: dx"), self._planes_on_device(dy, n, "corner_response: dy")
        resp = torch.empty((n, self.h, self.w), dtype=torch.float32, device=gx.device)
        self._wait_for_torch()
        self._queue_response(gx, gy, resp, n, block_size, self._corner_method(method), k)
        self.sync()
        return resp

    def good_features(self, response, quality_level, min_distance, max_corners=None, candidate_capacity=4096):
        """Host or torch float32 response planes [n, H, W] (or one plane) in; per frame the corners float32 (count, 2) = (x, y) by
        descending response and their responses float32 (count,) out, as hc_good_features_device states them: at most
        max_corners a frame (None: all that are kept)."""
        import torch
        dev = torch.device("cuda", self.device)
        if isinstance(response, torch.Tensor):
            d = response
        else:
            d = torch.from_numpy(np.ascontiguousarray(response))
        if d.dtype != torch.float32:
            raise HipCannyError(f"good_features: the response must be float32, not {d.dtype}")
        d = (d if d.ndim == 3 else d[None]).to(dev).contiguous()
        if d.ndim != 3 or tuple(d.shape[1:]) != (self.h, self.w):
            raise HipCannyError(f"good_features: planes {tuple(d.shape)} do not match the context's {(self.h, self.w)}")
        n = d.shape[0]
        bufs = self._feature_buffers(n, max_corners, candidate_capacity, dev)
        self._wait_for_torch()
        self._queue_features(d, n, quality_level, min_distance, candidate_capacity, bufs)
        return self._features_from(n, bufs)

    def features(self, frames, ksize=3, block_size=3, method="min_eigen", k=0.04, quality_level=0.01, min_distance=10, max_corners=1000, blur=None,
                 candidate_capacity=4096):
        """cv::goodFeaturesToTrack of u8 frames (1-channel contexts): cv::GaussianBlur (blur = (ksize, sigma), optional), the
        derivatives of aperture ksize (derivatives_device), the corner measure and the selection chained on the device with no
        host copy and no synchronisation in between.  Returns (corners, responses) per frame as good_features gives them."""
        import torch
        if self.c != 1:
            raise ValueError("features: a 1-channel context is required (the derivative planes of 3-channel frames are interleaved)")
        raw, n, row, fs = self._device_view(frames, "features")
        m = self._corner_method(method)
        # every tensor first, then one wait for torch's stream (_blurred waits once more, before anything of the chain is queued)
        gx, gy = torch.empty_like(raw, dtype=torch.int16), torch.empty_like(raw, dtype=torch.int16)
        resp = torch.empty((n, self.h, self.w), dtype=torch.float32, device=raw.device)
        bufs = self._feature_buffers(n, max_corners, candidate_capacity, raw.device)
        self._wait_for_torch()
        src = self._blurred(raw, n, row, fs, blur)   # (raw stays referenced until the call has synchronised)
        self.derivatives_device(src.data_ptr(), row, fs, gx.data_ptr(), gy.data_ptr(), 2 * row, 2 * fs, n, ksize)
        self._queue_response(gx, gy, resp, n, block_size, m, k)
        self._queue_features(resp, n, quality_level, min_distance, candidate_capacity, bufs)
        return self._features_from(n, bufs)

    def pyr_down_device(self, d_src, pitch, fs, src_width, src_height, d_dst, dst_pitch, dst_fs, nframes):
        """cv::pyrDown of one-channel u8 planes of src_width x src_height on device memory (hc_pyr_down_device, either mode): planes of
        ((src_width + 1) // 2) x ((src_height + 1) // 2) out.  Pitches and frame strides in bytes, any alignment; the views must not
        overlap.  Asynchronous on the context stream; not a run."""
        _ck(self.lib.hc_pyr_down_device(self.handle, C.c_void_p(d_src), pitch, fs, int(src_width), int(src_height), C.c_void_p(d_dst), dst_pitch, dst_fs,
                                        int(nframes)))

    def lk_flow_device(self, d_prev, d_next, pitch, fs, width, height, level, nframes, d_counts, d_prev_pts, d_next_pts, capacity, win, max_iterations,
                       epsilon, min_eig_threshold, use_initial, d_status, d_err):
        """One pyramid level of cv::calcOpticalFlowPyrLK on device memory (hc_lk_flow_device, either mode): u8 levels of width x
        height, points in level-0 units, d_next_pts in / out; d_status and d_err (or None) are written at level 0 only.
        Asynchronous on the context stream; not a run."""
        _ck(self.lib.hc_lk_flow_device(self.handle, C.c_void_p(d_prev), C.c_void_p(d_next), pitch, fs, int(width), int(height), int(level), int(nframes),
                                       C.c_void_p(d_counts), C.c_void_p(d_prev_pts), C.c_void_p(d_next_pts), int(capacity), int(win), int(max_iterations),
                                       float(epsilon), float(min_eig_threshold), int(use_initial), C.c_void_p(d_status), C.c_void_p(d_err or None)))

    def _u8_planes(self, frames, who, width=None, height=None):
        """Host or torch u8 planes [n, h, w] (or one plane) as a contiguous tensor on the context's device; (h, w) is (height, width)
        where given, else the planes' own, and no larger than the context's frame."""
        import torch
        dev = torch.device("cuda", self.device)
        if isinstance(frames, torch.Tensor):
            d = frames.to(device=dev, dtype=torch.uint8)
        else:
            d = torch.from_numpy(np.ascontiguousarray(frames, dtype=np.uint8)).to(dev)
        d = (d[None] if d.ndim == 2 else d).contiguous()
        if d.ndim != 3 or (width is not None and d.shape[2] != int(width)) or (height is not None and d.shape[1] != int(height)):
            raise HipCannyError(f"{who}: planes {tuple(d.shape)} do not match (n, {height}, {width})")
        if d.shape[1] > self.h or d.shape[2] > self.w:
            raise HipCannyError(f"{who}: planes {tuple(d.shape)} exceed the context's {(self.h, self.w)}")
        return d

    def _queue_pyr_down(self, src):
        """Queues cv::pyrDown of a tight u8 tensor [n, h, w] into a new tight tensor and returns it; no host wait (the caller has
        waited for torch's stream after its own allocations; this one's memory is not written by torch)."""
        import torch
        n, h, w = src.shape
        dst = torch.empty((n, (h + 1) // 2, (w + 1) // 2), dtype=torch.uint8, device=src.device)
        self._wait_for_torch()
        self.pyr_down_device(src.data_ptr(), w, w * h, w, h, dst.data_ptr(), dst.shape[2], dst.shape[2] * dst.shape[1], n)
        return dst

    def pyr_down(self, frames, width=None, height=None):
        """Host or torch u8 planes [n, h, w] (or one plane) in, cv::pyrDown of them [n, (h + 1) // 2, (w + 1) // 2] out as a torch
        tensor on the device (hc_pyr_down_device).  width, height: what the planes must measure (None: their own size)."""
        src = self._u8_planes(frames, "pyr_down", width, height)
        self._wait_for_torch()
        dst = self._queue_pyr_down(src)
        self.sync()
        return dst

    def lk_level(self, prev, nxt, level, counts, prev_pts, next_pts, win=21, max_iterations=30, epsilon=0.01, min_eig_threshold=1e-4, use_initial=False,
                 status=None, err=None):
        """One level call on torch tensors of the context's device, queued on the context stream with no host wait: prev, nxt tight u8
        [n, h, w]; counts int32 / uint32 [n]; prev_pts, next_pts float32 [n, capacity, 2] (next_pts in / out); status u8
        [n, capacity]; err float32 [n, capacity] or None.  A thin wrapper of hc_lk_flow_device."""
        n, h, w = prev.shape
        if tuple(nxt.shape) != (n, h, w) or not (prev.is_contiguous() and nxt.is_contiguous() and prev_pts.is_contiguous() and next_pts.is_contiguous()):
            raise HipCannyError("lk_level: prev and next must be contiguous tensors of one shape, the points contiguous")
        self.lk_flow_device(prev.data_ptr(), nxt.data_ptr(), w, w * h, w, h, level, n, counts.data_ptr(), prev_pts.data_ptr(), next_pts.data_ptr(),
                            prev_pts.shape[1], win, max_iterations, epsilon, min_eig_threshold, use_initial, status.data_ptr() if status is not None else None,
                            err.data_ptr() if err is not None else None)

    def _queue_flow(self, a, b, pts, counts, nxt, status, err, win, levels, max_iterations, epsilon, min_eig_threshold, use_initial):
        """Queues both pyramids and the level calls, from the coarsest level down; returns the pyramids (they must outlive the
        calls).  The pyramid stops at the last level whose sides are still at least 3."""
        pa, pb = [a], [b]
        for _ in range(int(levels)):
            h, w = pa[-1].shape[1:]
            if (h + 1) // 2 < 3 or (w + 1) // 2 < 3:
                break
            pa.append(self._queue_pyr_down(pa[-1]))
            pb.append(self._queue_pyr_down(pb[-1]))
        top = len(pa) - 1
        for lv in range(top, -1, -1):
            self.lk_level(pa[lv], pb[lv], lv, counts, pts, nxt, win, max_iterations, epsilon, min_eig_threshold, use_initial or lv < top, status, err)
        return pa, pb

    def optical_flow(self, prev, next, points, counts, win=21, levels=3, max_iterations=30, epsilon=0.01, min_eig_threshold=1e-4, initial=None):
        """cv::calcOpticalFlowPyrLK of u8 frames [n, H, W] (or one frame) of the context's size: points float32 [n, capacity, 2] =
        (x, y) and counts [n] as hc_good_features_device writes them (host or torch); initial: a guess of the same shape.  Both
        pyramids and the levels + 1 level calls are chained on the context stream.  Returns torch tensors on the device:
        (next_pts [n, capacity, 2], status u8 [n, capacity], err float32 [n, capacity]); slots at or beyond a frame's count hold the
        points (or the guess) they were given, status 0 and err 0."""
        import torch
        dev = torch.device("cuda", self.device)
        a, b = self._u8_planes(prev, "optical_flow: prev", self.w, self.h), self._u8_planes(next, "optical_flow: next", self.w, self.h)
        n = a.shape[0]
        as_dev = lambda v, dt: (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v))).to(device=dev, dtype=dt).contiguous()
        pts = as_dev(points, torch.float32)
        pts = pts[None] if pts.ndim == 2 else pts
        cnt = as_dev(np.asarray(counts).astype(np.int64) if not isinstance(counts, torch.Tensor) else counts, torch.int32).reshape(-1)
        if b.shape[0] != n or pts.ndim != 3 or pts.shape[0] != n or pts.shape[2] != 2 or cnt.shape[0] != n:
            raise HipCannyError(f"optical_flow: {n} prev frames, {b.shape[0]} next frames, points {tuple(pts.shape)}, {cnt.shape[0]} counts")
        nxt = (pts if initial is None else as_dev(initial, torch.float32).reshape(pts.shape)).clone()
        status = torch.zeros(pts.shape[:2], dtype=torch.uint8, device=dev)
        err = torch.zeros(pts.shape[:2], dtype=torch.float32, device=dev)
        self._wait_for_torch()
        keep = self._queue_flow(a, b, pts, cnt, nxt, status, err, win, levels, max_iterations, epsilon, min_eig_threshold, initial is not None)
        self.sync()
        del keep
        return nxt, status, err

    def track(self, prev, next, ksize=3, block_size=3, method="min_eigen", k=0.04, quality_level=0.01, min_distance=10, max_corners=1000, blur=None,
              candidate_capacity=4096, win=21, levels=3, max_iterations=30, epsilon=0.01, min_eig_threshold=1e-4):
        """Detect and follow (1-channel contexts): the chain of `features` on prev -- blur, derivatives, corner measure, selection --
        and then the flow of those corners into next, all on the context stream with no host copy in between.  Returns torch tensors
        on the device: (counts int32 [n] = min(kept, max_corners), points [n, max_corners, 2], next_pts likewise, status u8
        [n, max_corners], err float32 [n, max_corners]); slots at or beyond a frame's count hold zeros."""
        import torch
        if self.c != 1:
            raise ValueError("track: a 1-channel context is required")
        raw, n, row, fs = self._device_view(prev, "track: prev")
        nx = self._u8_planes(next, "track: next", self.w, self.h)
        if nx.shape[0] != n:
            raise HipCannyError(f"track: {n} prev frames, {nx.shape[0]} next frames")
        m = self._corner_method(method)
        gx, gy = torch.empty_like(raw, dtype=torch.int16), torch.empty_like(raw, dtype=torch.int16)
        resp = torch.empty((n, self.h, self.w), dtype=torch.float32, device=raw.device)
        cap = int(max_corners)
        counts = torch.zeros((n,), dtype=torch.int32, device=raw.device)
        pts = torch.zeros((n, cap, 2), dtype=torch.float32, device=raw.device)
        nxt = torch.zeros_like(pts)
        status = torch.zeros((n, cap), dtype=torch.uint8, device=raw.device)
        err = torch.zeros((n, cap), dtype=torch.float32, device=raw.device)
        self._wait_for_torch()
        src = self._blurred(raw, n, row, fs, blur)
        self.derivatives_device(src.data_ptr(), row, fs, gx.data_ptr(), gy.data_ptr(), 2 * row, 2 * fs, n, ksize)
        self._queue_response(gx, gy, resp, n, block_size, m, k)
        self.good_features_device(resp.data_ptr(), 4 * self.w, 4 * self.w * self.h, n, quality_level, min_distance, candidate_capacity, counts.data_ptr(),
                                  pts.data_ptr(), None, cap)
        keep = self._queue_flow(raw.reshape(n, self.h, self.w), nx, pts, counts, nxt, status, err, win, levels, max_iterations, epsilon, min_eig_threshold, False)
        self.sync()
        del keep
        return torch.clamp(counts, max=cap), pts, nxt, status, err

    def hysteresis_device(self, d_thr, in_pitch, in_fs, d_out, out_pitch, out_fs, nframes):
        _ck(self.lib.hc_hysteresis_device(self.handle, C.c_void_p(d_thr), in_pitch, in_fs, C.c_void_p(d_out), out_pitch,
                                          out_fs, int(nframes)))

    def front_waves_per_workgroup(self):
        """Waves per workgroup of the most recent k_front8 launch (hc_front_waves_per_workgroup): 4, 1 or 3."""
        return self._count_or_error(self.lib.hc_front_waves_per_workgroup(self.handle))

    def pipeline_slots_in_use(self):
        """Slots of the ring the most recent pipelined run used (hc_pipeline_slots_in_use)."""
        return self._count_or_error(self.lib.hc_pipeline_slots_in_use(self.handle))

    def pipeline_depth(self, nframes):
        """Runs of `nframes` frames kept in flight in pipelined mode (hc_pipeline_depth): the size of the output-buffer ring."""
        return self._count_or_error(self.lib.hc_pipeline_depth(self.handle, int(nframes)))

    def last_run_info(self):
        """(input_staged, output_staged, front_form) of the last run: see hc_last_run_info."""
        a, b, f = C.c_int(), C.c_int(), C.c_int()
        _ck(self.lib.hc_last_run_info(self.handle, C.byref(a), C.byref(b), C.byref(f)))
        return bool(a.value), bool(b.value), f.value

    def hysteresis_info(self):
        a, b = C.c_int(), C.c_int()
        _ck(self.lib.hc_last_hysteresis_info(self.handle, C.byref(a), C.byref(b)))
        return a.value, b.value

    def hysteresis_stats(self, launches=6):
        """[(sweeps_sum, sweeps_max, active_tiles)] per queued hysteresis launch of the last run."""
        buf = (C.c_uint * (3 * launches))()
        _ck(self.lib.hc_hysteresis_stats(self.handle, buf, 3 * launches))
        return [(buf[3 * k], buf[3 * k + 1], buf[3 * k + 2]) for k in range(launches)]

    def debug_tap(self, what, nframes=1):
        """The FAST path's own intermediate (TAP_BLUR / TAP_THRESH) of the last HYSTER run; needs OPT_DEBUG_TAPS."""
        out = np.empty((nframes, self.h, self.w), np.uint8)
        _ck(self.lib.hc_debug_tap(self.handle, int(what), out.ctypes.data, self.w, self.w * self.h, int(nframes)))
        return out

    def process(self, frames, final_stage=CannyStage.HYSTER):
        """upload -> run -> download convenience."""
        n = self.upload(frames)
        self.run(final_stage, n)
        return self.download(n * getattr(self, "_maps_per_frame", 1))   # per-channel mode: three maps per input frame


def selftest(device=0):
    _ck(load_library().hc_selftest(int(device)))


class TimerManager:
    """timerManager singleton, src/utils/timer.hpp:13-67 (running averages keyed by stage name)."""
    _inst = None

    def __init__(self):
        self._timers = {}

    @classmethod
    def Get(cls):
        if cls._inst is None:
            cls._inst = cls()
        return cls._inst

    def createTimer(self, name):
        self._timers.setdefault(name, [0.0, 0])

    def addTime(self, name, t):
        if name in self._timers:
            self._timers[name][0] += t
            self._timers[name][1] += 1
        else:
            print(f"Timer {name} unknown", file=sys.stderr)

    def getAverageTime(self, name):
        t = self._timers.get(name)
        if t and t[1] > 0:
            return t[0] / t[1]
        print(f"Timer {name} unknown", file=sys.stderr)
        return 0.0

    def timers(self):
        return dict(self._timers)


def _mat_type(mat):
    if not isinstance(mat, np.ndarray) or mat.dtype != np.uint8:
        return None
    if mat.ndim == 2:
        return "CV_8UC1"
    if mat.ndim == 3 and mat.shape[2] == 3:
        return "CV_8UC3"
    return None


class CannyEdge:
    """Mirror of cvp::cuda::CannyEdge (src/cvp/cannyEdgeH.hpp:17-32).

    pbo: the reference's OpenGL pixel-buffer id; a headless MI355X has no GL, so it must be 0 and
    the result is read with output() instead.
    """

    def __init__(self, pbo, imageWidth, imageHeight, imageNbChannels, mode=MODE_R, device=0):
        if pbo != 0:
            raise HipCannyError("GL interop is not available on MI355X: pass pbo=0 and read output()")
        self._ctx = Context(imageWidth, imageHeight, imageNbChannels, 1, mode, device)
        self.m_inputW, self.m_inputH, self.m_inputNbChannels = imageWidth, imageHeight, imageNbChannels
        self._ctx.set_thresholds(10, 40) if mode == MODE_R else None  # cannyEdgeH.cu:22-23
        self._profiling = True                                          # cannyEdgeH.cu:24
        self._ctx.enable_profiling(True)
        self._out = None
        tm = TimerManager.Get()
        for name in CANNY_STAGES.values():                              # cannyEdgeH.cu:35-37
            tm.createTimer(name)

    def run(self, input, finalStage):
        """cannyEdgeH.cu:49-120.  Size/channel mismatch: logged, frame not processed (:124-130)."""
        exp = (self.m_inputH, self.m_inputW) if self.m_inputNbChannels == 1 else (self.m_inputH, self.m_inputW, 3)
        if input.shape != exp:
            print("Cannot load image to GPU, specs different since initialization", file=sys.stderr)
            return
        try:
            stage = CannyStage(int(finalStage))
        except ValueError:
            print("Canny Stage Not Recognized", file=sys.stderr)
            return
        self._ctx.upload(input)
        self._ctx.run(stage, 1)
        self._out = self._ctx.download(1)[0]
        if self._profiling:
            tm = TimerManager.Get()
            for st in CannyStage:  # one sample per stage that ran (cannyEdgeH.cu:415-430); -1 = the run did not execute it
                ms = self._ctx.stage_time_ms(st)
                if ms >= 0:
                    tm.addTime(CANNY_STAGES[st], ms)

    def output(self):
        return self._out

    def setLowThreshold(self, low):
        lo, hi = self._ctx.get_thresholds()
        self._ctx.set_thresholds(min(int(low) & 0xFF, hi), hi)     # cannyEdgeH.hpp:25

    def getLowThreshold(self):
        return self._ctx.get_thresholds()[0]

    def setHighThreshold(self, high):
        lo, hi = self._ctx.get_thresholds()
        self._ctx.set_thresholds(lo, max(int(high) & 0xFF, lo))    # cannyEdgeH.hpp:28

    def getHighThreshold(self):
        return self._ctx.get_thresholds()[1]

    def enableKernelProfiling(self, profiling):
        self._profiling = bool(profiling)
        self._ctx.enable_profiling(self._profiling)

    def isKernelProfilingEnabled(self):
        return self._profiling


class cvPipeline:
    """Mirror of cvp::cvPipeline (src/cvp/cvPipeline.hpp:20-39, cvPipeline.cpp:9-96)."""

    def __init__(self, pbo, inputImageCols, inputImageRows, inputImageNbChannels, mode=MODE_R, device=0):
        self.m_cudaCannyEdge = CannyEdge(pbo, inputImageCols, inputImageRows, inputImageNbChannels, mode, device)

    def process(self, inputImage, finalStage):
        if self.m_cudaCannyEdge is None:
            print("Cannot process the webcam stream, Cuda is not ready.", file=sys.stderr)
            return False
        if inputImage is None or getattr(inputImage, "size", 0) == 0:
            print("Blank frame grabbed", file=sys.stderr)                       # cvPipeline.cpp:27-31
            return False
        if _mat_type(inputImage) is None:
            print("Only supporting CV_8UC3 and CV_8UC1 input types for now", file=sys.stderr)  # :32-36
            return False
        self.m_cudaCannyEdge.run(inputImage, finalStage)
        return True

    def output(self):
        return self.m_cudaCannyEdge.output()

    def setLowThreshold(self, low):
        self.m_cudaCannyEdge.setLowThreshold(low)

    def getLowThreshold(self):
        return self.m_cudaCannyEdge.getLowThreshold()

    def setHighThreshold(self, high):
        self.m_cudaCannyEdge.setHighThreshold(high)

    def getHighThreshold(self):
        return self.m_cudaCannyEdge.getHighThreshold()

    def enableCudaProfiling(self, profiling):
        self.m_cudaCannyEdge.enableKernelProfiling(profiling)

    def isCudaProfilingEnabled(self):
        return self.m_cudaCannyEdge.isKernelProfilingEnabled() if self.m_cudaCannyEdge else False
