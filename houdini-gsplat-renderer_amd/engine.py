"""ctypes binding of libgsplat_hip.so: the C ABI (include/gsplat_hip.h) and the flat wrappers
of the GSplatRenderer host shim (include/GSplatRenderer.h).

There is NO CPU fallback: if the library is missing or no GPU is visible, every
render path raises ``GsrError``.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import build as _build

_LIB = None


class GsrError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"gsplat_hip error {code}: {msg}")
        self.code = code


class gsr_camera(C.Structure):
    _fields_ = [("obj_view", C.c_float * 16), ("object", C.c_float * 16), ("inv_object", C.c_float * 16),
                ("view", C.c_float * 16), ("proj", C.c_float * 16), ("cam_pos", C.c_float * 3),
                ("width", C.c_int32), ("height", C.c_int32), ("sh_order", C.c_int32)]


class gsr_stats(C.Structure):
    _fields_ = [("n_splats", C.c_int64), ("n_visible", C.c_int64), ("pairs_total", C.c_int64),
                ("pairs_consumed", C.c_int64), ("tiles_x", C.c_int32), ("tiles_y", C.c_int32),
                ("record_bytes", C.c_int32), ("pair_bytes", C.c_int32),
                ("ms_preprocess", C.c_float), ("ms_depth_sort", C.c_float), ("ms_emit", C.c_float),
                ("ms_tile_sort", C.c_float), ("ms_blend", C.c_float), ("ms_total", C.c_float),
                ("blend_ms_total", C.c_double), ("blend_launches", C.c_int64),
                ("blend_pairs_consumed_total", C.c_int64), ("frame_ms_total", C.c_double), ("frames", C.c_int64),
                ("entries_scanned", C.c_int64), ("blend_entries_scanned_total", C.c_int64),
                ("super_tile", C.c_int32), ("stiles_x", C.c_int32), ("stiles_y", C.c_int32), ("reserved_", C.c_int32),
                ("blend_wave_evals_total", C.c_int64), ("stage_ms_total", C.c_double * 5),
                ("stage_frames", C.c_int64), ("sorts_skipped", C.c_int64), ("frames_requeued", C.c_int64),
                ("lazy_redo_tiles", C.c_int64), ("lazy_colours_total", C.c_int64), ("frames_truncated", C.c_int64),
                ("frames_culled", C.c_int64), ("frames_repaired", C.c_int64),
                ("clusters_total", C.c_int64), ("clusters_kept", C.c_int64),
                ("policy_bits", C.c_int32), ("cull_dilate", C.c_int32), ("cull_holdoff", C.c_int32), ("reserved2_", C.c_int32),
                ("frames_resorted", C.c_int64), ("frames_slab", C.c_int64), ("frames_jumped", C.c_int64), ("frames_lazy", C.c_int64),
                ("uploads", C.c_int64), ("upload_ms", C.c_double * 6),
                ("moves", C.c_int64), ("move_ms", C.c_double * 4)]

    def as_dict(self) -> dict:
        d = {n: getattr(self, n) for n, _ in self._fields_}
        d["stage_ms_total"] = list(self.stage_ms_total)
        d["upload_ms"] = list(self.upload_ms)
        d["move_ms"] = list(self.move_ms)
        return d


class gsr_debug_record(C.Structure):
    _fields_ = [(n, C.c_float) for n in
                ("cx", "cy", "a1x", "a1y", "b1x", "b1y", "hx", "hy", "r", "g", "b", "la", "key")] + \
               [("visible", C.c_int32)]


DEBUG_RECORD_DTYPE = np.dtype([(n, np.float32) for n in
                               ("cx", "cy", "a1x", "a1y", "b1x", "b1y", "hx", "hy", "r", "g", "b", "la", "key")]
                              + [("visible", np.int32)])


class GSplatRenderContext(C.Structure):
    _fields_ = [("obj_view", C.c_float * 16), ("object", C.c_float * 16), ("inv_object", C.c_float * 16),
                ("view", C.c_float * 16), ("proj", C.c_float * 16), ("width", C.c_int32), ("height", C.c_int32),
                ("target", C.c_void_p), ("target_is_device", C.c_int32),
                ("depth", C.c_void_p), ("depth_is_device", C.c_int32)]


class gsr_raw_attrs(C.Structure):
    _fields_ = [("P", C.c_void_p), ("Cd", C.c_void_p), ("alpha", C.c_void_p), ("scale", C.c_void_p), ("orient", C.c_void_p),
                ("sh_scheme", C.c_int32), ("sh_vec3_per_point", C.c_int32), ("sh_array", C.c_void_p), ("sh_ptr", C.POINTER(C.c_void_p))]


class gsr_background(C.Structure):
    """include/gsplat_hip.h: what gsr_render_over composites the frame over (premultiplied; kind 0 = nothing)"""
    _fields_ = [("kind", C.c_int32), ("format", C.c_int32), ("rgba", C.c_float * 4), ("image", C.c_void_p),
                ("image_is_device", C.c_int32), ("reserved_", C.c_int32)]


class gsr_attr_update(C.Structure):
    """include/gsplat_hip.h: the arrays gsr_update rewrites in place (NULL = leave as is)"""
    _fields_ = [("Cd", C.c_void_p), ("alpha", C.c_void_p), ("scale", C.c_void_p), ("orient", C.c_void_p),
                ("shx", C.c_void_p), ("shy", C.c_void_p), ("shz", C.c_void_p)]


class gsr_device_attrs(C.Structure):
    """include/gsplat_hip.h: float32 point attributes in DEVICE memory (NULL has the meaning the verb gives it)"""
    _fields_ = [("P", C.c_void_p), ("Cd", C.c_void_p), ("alpha", C.c_void_p), ("scale", C.c_void_p), ("orient", C.c_void_p),
                ("sh", C.c_void_p), ("sh_vec3_per_point", C.c_int32), ("reserved_", C.c_int32)]


class gsr_read_arrays(C.Structure):
    """include/gsplat_hip.h: the HOST destinations of gsr_read, in gsr_upload_append's layout (NULL = not wanted)"""
    _fields_ = [("P", C.c_void_p), ("Cd", C.c_void_p), ("alpha", C.c_void_p), ("scale", C.c_void_p), ("orient", C.c_void_p),
                ("shx", C.c_void_p), ("shy", C.c_void_p), ("shz", C.c_void_p)]


class gsr_device_out(C.Structure):
    """include/gsplat_hip.h: the float32 DEVICE destinations of gsr_read_device, in gsr_device_attrs' layout (NULL = not wanted)"""
    _fields_ = [("P", C.c_void_p), ("Cd", C.c_void_p), ("alpha", C.c_void_p), ("scale", C.c_void_p), ("orient", C.c_void_p),
                ("sh", C.c_void_p), ("sh_vec3_per_point", C.c_int32), ("reserved_", C.c_int32)]


class gsr_crop_volume(C.Structure):
    """include/gsplat_hip.h: one crop volume -- a 3x4 affine map (rows) from upload space onto the unit box / unit ball"""
    _fields_ = [("kind", C.c_int32), ("invert", C.c_int32), ("to_unit", C.c_float * 12)]


class gsr_visibility(C.Structure):
    """include/gsplat_hip.h: what gsr_set_visibility hides by -- up to four volumes (a splat must pass every one) and a HOST bit mask"""
    _fields_ = [("n_volumes", C.c_int32), ("reserved_", C.c_int32), ("volume", gsr_crop_volume * 4),
                ("mask", C.c_void_p), ("mask_splats", C.c_int64)]


class gsr_select_region(C.Structure):
    """include/gsplat_hip.h: the screen region of gsr_select -- a rect, and optionally a bit image and a depth buffer (host or device)"""
    _fields_ = [("x0", C.c_float), ("y0", C.c_float), ("x1", C.c_float), ("y1", C.c_float),
                ("image", C.c_void_p), ("image_is_device", C.c_int32), ("depth", C.c_void_p), ("depth_is_device", C.c_int32),
                ("depth_bias", C.c_float), ("op", C.c_int32), ("flags", C.c_int32), ("reserved_", C.c_int32)]


class gsr_mark_style(C.Structure):
    """include/gsplat_hip.h: how gsr_render_marks draws a selection -- dots or outlines, a fixed colour or Cd, an optional depth test"""
    _fields_ = [("shape", C.c_int32), ("radius", C.c_int32), ("colour_mode", C.c_int32), ("flags", C.c_int32), ("rgba", C.c_float * 4),
                ("depth", C.c_void_p), ("depth_is_device", C.c_int32), ("depth_bias", C.c_float), ("reserved_", C.c_int32)]


class gsr_attr_rule(C.Structure):
    """include/gsplat_hip.h: the rule of gsr_select_attrs -- clauses on the true alpha, the scale halves, the base colour and crop volumes"""
    _fields_ = [("clauses", C.c_int32), ("flags", C.c_int32), ("op", C.c_int32), ("n_volumes", C.c_int32),
                ("alpha_lo", C.c_float), ("alpha_hi", C.c_float), ("scale_max_lo", C.c_float), ("scale_max_hi", C.c_float),
                ("scale_min_lo", C.c_float), ("scale_min_hi", C.c_float), ("anisotropy", C.c_float),
                ("colour_lo", C.c_float * 3), ("colour_hi", C.c_float * 3), ("reserved_", C.c_int32), ("volume", gsr_crop_volume * 4)]


class gsr_density_rule(C.Structure):
    """include/gsplat_hip.h: the rule of gsr_select_density -- a grid of 1024^3 cells, a reach, a range of neighbour counts, an alpha floor"""
    _fields_ = [("cell", C.c_float), ("origin", C.c_float * 3), ("reach", C.c_int32), ("flags", C.c_int32), ("op", C.c_int32),
                ("reserved_", C.c_int32), ("count_lo", C.c_uint32), ("count_hi", C.c_uint32), ("alpha_min", C.c_float)]


class gsr_density_result(C.Structure):
    """include/gsplat_hip.h: what gsr_select_density reports beside the mask.  hist() -> count_hist as an int64 array"""
    _fields_ = [("n_population", C.c_int64), ("n_outside", C.c_int64), ("n_cells", C.c_int64), ("count_hist", C.c_int64 * 64)]

    def hist(self) -> np.ndarray:
        """int64 (64,): bin b < 63 holds the population splats with N == b + 1, bin 63 those with N >= 64"""
        return np.array(self.count_hist[:], np.int64)

    def fields(self) -> tuple:
        """(n_population, n_outside, n_cells, count_hist as a tuple): what two results are compared by"""
        return (self.n_population, self.n_outside, self.n_cells, tuple(self.count_hist[:]))


class gsr_connect_rule(C.Structure):
    """include/gsplat_hip.h: the rule of gsr_select_connected -- the density rule's grid, reach, alpha floor and flags, and a range of
    component sizes in the place of the count range"""
    _fields_ = [("cell", C.c_float), ("origin", C.c_float * 3), ("reach", C.c_int32), ("flags", C.c_int32), ("op", C.c_int32),
                ("reserved_", C.c_int32), ("size_lo", C.c_uint32), ("size_hi", C.c_uint32), ("alpha_min", C.c_float)]


class gsr_connect_result(C.Structure):
    """include/gsplat_hip.h: what gsr_select_connected reports beside the mask.  hists() -> (comp_hist, splat_hist) as int64 arrays"""
    _fields_ = [("n_population", C.c_int64), ("n_outside", C.c_int64), ("n_cells", C.c_int64), ("n_components", C.c_int64),
                ("n_seeded", C.c_int64), ("largest", C.c_int64), ("comp_hist", C.c_int64 * 32), ("splat_hist", C.c_int64 * 32)]

    def hists(self) -> tuple:
        """(int64 (32,), int64 (32,)): bin b holds the components with floor(log2(size)) == b, and the population splats in them"""
        return np.array(self.comp_hist[:], np.int64), np.array(self.splat_hist[:], np.int64)

    def fields(self) -> tuple:
        """(n_population, n_outside, n_cells, n_components, n_seeded, largest, comp_hist, splat_hist as tuples): what two results are
        compared by"""
        return (self.n_population, self.n_outside, self.n_cells, self.n_components, self.n_seeded, self.largest,
                tuple(self.comp_hist[:]), tuple(self.splat_hist[:]))


class gsr_hist_spec(C.Structure):
    """include/gsplat_hip.h: one histogram of gsr_measure -- a channel, [lo, hi) in `bins` bins, and what gsr_hist_prepare derives"""
    _fields_ = [("channel", C.c_int32), ("flags", C.c_int32), ("bins", C.c_int32), ("lo", C.c_float), ("hi", C.c_float), ("inv_w", C.c_float)]


class gsr_measure_request(C.Structure):
    """include/gsplat_hip.h: what gsr_measure computes -- bounds, extent, moments about ref, up to four histograms"""
    _fields_ = [("what", C.c_int32), ("flags", C.c_int32), ("ref", C.c_float * 3), ("extent_k", C.c_float), ("n_hist", C.c_int32),
                ("hist", gsr_hist_spec * 4), ("reserved_", C.c_int32)]


class gsr_measure_result(C.Structure):
    """include/gsplat_hip.h: what gsr_measure reports.  The Python door also sets .ref (float32 (3,), the request's) and .hist (one
    uint32 array of bins + 3 counts per spec: the bins, then under, over, nan)"""
    _fields_ = [("n_selected", C.c_int64), ("n_measured", C.c_int64), ("n_extent", C.c_int64),
                ("lo", C.c_float * 3), ("hi", C.c_float * 3), ("lo_e", C.c_float * 3), ("hi_e", C.c_float * 3), ("sum", C.c_double * 9)]
    ref = (0.0, 0.0, 0.0)
    hist = ()

    def centroid(self) -> np.ndarray:
        """float64 (3,): ref + sum(d) / n_measured, formed on the host (NaN where nothing was measured; needs MEASURE_MOMENTS)"""
        s = np.array(self.sum[:3], np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.asarray(self.ref, np.float64) + s / np.float64(self.n_measured)

    def covariance(self) -> np.ndarray:
        """float64 (3, 3): E[d d^T] - E[d] E[d]^T over the measured splats (the population covariance), formed on the host"""
        xx, xy, xz, yy, yz, zz = [float(v) for v in self.sum[3:]]
        with np.errstate(invalid="ignore", divide="ignore"):
            m = np.array(self.sum[:3], np.float64) / np.float64(self.n_measured)
            return np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]], np.float64) / np.float64(self.n_measured) - np.outer(m, m)


class gsr_xform(C.Structure):
    """include/gsplat_hip.h: the similarity of gsr_transform -- p' = s R (p - pivot) + pivot + translate"""
    _fields_ = [("rotate", C.c_float * 4), ("scale", C.c_float), ("translate", C.c_float * 3), ("pivot", C.c_float * 3), ("reserved_", C.c_int32)]


class gsr_xform_rule(C.Structure):
    """include/gsplat_hip.h: what gsr_xform_prepare derives from a gsr_xform (100 float32)"""
    _fields_ = [("A", C.c_float * 9), ("t", C.c_float * 3), ("s", C.c_float), ("q", C.c_float * 4),
                ("D1", C.c_float * 9), ("D2", C.c_float * 25), ("D3", C.c_float * 49)]


class gsr_grade_params(C.Structure):
    """include/gsplat_hip.h: what a user turns to grade a selection (grade_params() has the neutral defaults)"""
    _fields_ = [("exposure", C.c_float), ("gain", C.c_float * 3), ("saturation", C.c_float), ("contrast", C.c_float), ("pivot", C.c_float),
                ("offset", C.c_float * 3), ("alpha_gain", C.c_float), ("alpha_offset", C.c_float)]


class gsr_grade_rule(C.Structure):
    """include/gsplat_hip.h: what gsr_grade evaluates -- c' = M c + b, alpha' = clamp(ag alpha + ab, 0, 1), and which of the two run"""
    _fields_ = [("M", C.c_float * 9), ("b", C.c_float * 3), ("ag", C.c_float), ("ab", C.c_float), ("flags", C.c_uint32)]


GRADE_COLOUR, GRADE_ALPHA = 1, 2


class gsplat_attrs(C.Structure):
    _fields_ = [("count", C.c_int64), ("P", C.c_void_p), ("Cd", C.c_void_p), ("opacity", C.c_void_p), ("Alpha", C.c_void_p),
                ("scale", C.c_void_p), ("orient", C.c_void_p), ("sh_coefficients", C.c_void_p),
                ("sh_coefficients_len", C.c_int32), ("sh", C.POINTER(C.c_void_p)), ("f_rest", C.POINTER(C.c_void_p)),
                ("sh_order", C.POINTER(C.c_int32)), ("explicit_camera_pos", C.POINTER(C.c_float))]


TRANSPORT_AUTO, TRANSPORT_RCCL, TRANSPORT_COPY = 0, 1, 2
MAX_DIM = 16384         # GSR_MAX_DIM (include/gsplat_hip.h): largest framebuffer width / height
MISSING_CD, MISSING_OPACITY, MISSING_SCALE, MISSING_ORIENT, MISSING_SH, BAD_SH_ORDER = 1, 2, 4, 8, 16, 32
OPT_XCD_SWIZZLE, OPT_STAGE_TIMING, OPT_SORT_CACHE, OPT_SUPER_TILE, OPT_DEBUG_FLAGS, OPT_FRAMES_IN_FLIGHT, OPT_DEFERRED_CHECK, OPT_LAZY_COLOUR, OPT_SHARD_LAYOUT = 1, 2, 3, 4, 5, 6, 7, 8, 9
OPT_OCCLUSION_CULL = 10
OPT_TIMING_EVERY = 11
OPT_CLUSTER_CULL = 12
OPT_STORAGE_ORDER = 13
OPT_CULL_DILATE = 14
OPT_LOCAL_SORT = 15
OPT_FRONT_SLAB = 16
OPT_ROW_WORK = 17
TILE = 16               # GSR_TILE

# target formats (gsr_set_target_format): what one pixel of every target is
TARGET_RGBA32F = 0
TARGET_RGBA16F = 1
TARGET_RGBA8 = 2
AOV_DEPTH = 1          # gsr_render_aov: the plane {zsum, cov}, two float32 per pixel whatever the target format
BG_COLOUR = 1          # gsr_background.kind
BG_IMAGE = 2
VIS_MAX_VOLUMES = 4    # GSR_VIS_MAX_VOLUMES
VOL_BOX = 1            # gsr_crop_volume.kind: inside iff max(|q|) <= 1
VOL_ELLIPSOID = 2      # ... iff |q|^2 <= 1
REMOVE_HIDDEN = 1      # GSR_REMOVE_HIDDEN: gsr_remove also removes what the visibility in force hides
REMOVE_BLOCK = 4096    # GSR_REMOVE_BLOCK: upload indices one workgroup of the compaction kernels spans
COPY_BLOCK = REMOVE_BLOCK      # ... and of k_copy.h's, which keep that shape
SELECT_REPLACE, SELECT_ADD, SELECT_SUBTRACT, SELECT_INTERSECT, SELECT_TOGGLE = range(5)     # GSR_SELECT_*: what gsr_select does to the mask
SELECT_ANY_OPACITY = 1 # GSR_SELECT_ANY_OPACITY (flags): no opacity test, so hidden splats can be hit
SELECT_BLOCK = 256     # GSR_SELECT_BLOCK: upload indices one workgroup of the selection kernel spans
# GSR_ATTR_* (gsr_attr_rule.clauses): what gsr_select_attrs looks at; ATTR_SKIP_HIDDEN (flags): hidden splats are never hit
ATTR_ALPHA, ATTR_SCALE_MAX, ATTR_SCALE_MIN, ATTR_ANISOTROPY, ATTR_COLOUR, ATTR_VOLUME = 1, 2, 4, 8, 16, 32
ATTR_SKIP_HIDDEN = 1
# GSR_DENSITY_* (gsr_density_rule.flags, and the limits of the rule): what gsr_select_density counts and hits
DENSITY_SKIP_HIDDEN, DENSITY_HIT_OUTSIDE = 1, 2
DENSITY_CELLS = 1024       # GSR_DENSITY_CELLS: cells per axis
DENSITY_MAX_REACH = 2      # GSR_DENSITY_MAX_REACH
DENSITY_HIST_BINS = 64     # GSR_DENSITY_HIST_BINS
# GSR_CONNECT_* (gsr_connect_rule.flags, and the limits of the rule): what gsr_select_connected links and hits
CONNECT_SKIP_HIDDEN, CONNECT_HIT_OUTSIDE = 1, 2
CONNECT_CELLS = 1024       # GSR_CONNECT_CELLS: cells per axis
CONNECT_MAX_REACH = 2      # GSR_CONNECT_MAX_REACH
CONNECT_HIST_BINS = 32     # GSR_CONNECT_HIST_BINS
CONNECT_NO_LABEL = 0xffffffff  # GSR_CONNECT_NO_LABEL: labels_out of a splat that is not population
# GSR_MEASURE_* (gsr_measure_request.what / .flags) and GSR_HIST_* (gsr_hist_spec.channel / .flags): what gsr_measure computes
MEASURE_BOUNDS, MEASURE_EXTENT, MEASURE_MOMENTS = 1, 2, 4
MEASURE_SKIP_HIDDEN = 1
HIST_X, HIST_Y, HIST_Z, HIST_ALPHA, HIST_SCALE_MAX, HIST_SCALE_MIN, HIST_CD_R, HIST_CD_G, HIST_CD_B = range(9)
HIST_LOG2 = 1
HIST_MAX_BINS = 256    # GSR_HIST_MAX_BINS
MEASURE_MAX_HIST = 4   # GSR_MEASURE_MAX_HIST
MARK_DOT, MARK_OUTLINE = 1, 2                  # GSR_MARK_*: gsr_mark_style.shape
MARK_COLOUR_FIXED, MARK_COLOUR_CD = 0, 1       # ... .colour_mode
MARK_ANY_OPACITY = 1                           # ... .flags: also splats below 1/255 and the ones a visibility hides
MARK_MAX_RADIUS = 8                            # GSR_MARK_MAX_RADIUS: a dot is at most 17 x 17 pixels
TARGET_DTYPES = {TARGET_RGBA32F: np.dtype(np.float32), TARGET_RGBA16F: np.dtype(np.float16), TARGET_RGBA8: np.dtype(np.uint8)}

# every symbol include/gsplat_hip.h and include/GSplatRenderer.h declare
C_ABI_SYMBOLS = [
    "gsr_device_count", "gsr_create", "gsr_destroy", "gsr_last_error", "gsr_version", "gsr_set_stream",
    "gsr_upload_begin", "gsr_upload_append", "gsr_upload_append_raw", "gsr_upload_end", "gsr_upload_abort", "gsr_upload", "gsr_set_row_shard", "gsr_band_rows",
    "gsr_stitch_bands", "gsr_render", "gsr_render_depth", "gsr_render_wire", "gsr_render_wire_over", "gsr_synchronize", "gsr_get_stats", "gsr_stats_reset", "gsr_set_option",
    "gsr_debug_read_records", "gsr_debug_read_depth_order", "gsr_debug_read_storage_order", "gsr_debug_read_tile_lists", "gsr_debug_sort_pairs", "gsr_debug_sort_pairs_local", "gsr_debug_policy", "gsr_debug_policy_state", "gsr_debug_frame_plan",
    "gsr_debug_read_tile_work", "gsr_debug_read_horizons", "gsr_debug_read_horizon_pyramid", "gsr_debug_read_cull",
    "gsr_multi_create", "gsr_multi_destroy", "gsr_multi_count", "gsr_multi_transport", "gsr_multi_context",
    "gsr_multi_set_stream", "gsr_multi_set_option", "gsr_multi_upload_begin", "gsr_multi_upload_append",
    "gsr_multi_upload_end", "gsr_multi_upload_abort", "gsr_multi_upload", "gsr_multi_render", "gsr_multi_render_depth",
    "gsr_multi_synchronize", "gsr_multi_get_stats", "gsr_multi_comm_info", "gsr_multi_gather_stats",
    "gsr_comm_available", "gsr_comm_get_unique_id", "gsr_comm_init", "gsr_comm_info", "gsr_comm_destroy", "gsr_comm_render",
    "gsplat_renderer_create_multi", "gsplat_renderer_multi",
    "gsplat_prim_create", "gsplat_prim_destroy", "gsplat_prim_update", "gsplat_prim_render", "gsplat_prim_missing",
    "gsplat_prim_sh_order", "gsplat_prim_has_sh", "gsplat_prim_array",
    "gsplat_renderer_create", "gsplat_renderer_get_instance", "gsplat_renderer_destroy",
    "gsplat_renderer_register_update", "gsplat_renderer_include_in_render_pass",
    "gsplat_renderer_flush_entries_for_matching_detail", "gsplat_renderer_generate_render_geometry",
    "gsplat_renderer_render", "gsplat_renderer_post_render", "gsplat_renderer_redraw", "gsplat_renderer_set_rendering_enabled",
    "gsplat_renderer_set_explicit_camera_pos", "gsplat_renderer_set_spherical_harmonics_order",
    "gsplat_renderer_query", "gsplat_renderer_get_origin", "gsplat_renderer_get_last_camera_pos",
    "gsplat_renderer_engine", "gsplat_closest_sqrt_power_of_2", "gsplat_quantize_half",
    "gsplat_pack_sh_from_vec3", "gsplat_pack_sh_from_frest", "gsplat_pack_sh_from_array",
    "gsr_target_pixel_bytes", "gsr_set_target_format", "gsr_get_target_format", "gsr_multi_set_target_format", "gsr_convert_pixels",
    "gsplat_renderer_set_target_format", "gsplat_renderer_get_target_format",
    "gsr_render_aov", "gsr_resolve_depth", "gsr_resolve_depth_device", "gsplat_renderer_set_aov_target",
    "gsr_render_over", "gsr_composite_over", "gsplat_renderer_set_background",
    "gsr_update", "gsr_multi_update", "gsr_debug_read_resident", "gsplat_renderer_update_attributes", "gsplat_renderer_row_array",
    "gsr_move", "gsr_multi_move", "gsplat_renderer_move_splats",
    "gsr_upload_append_device", "gsr_update_device", "gsr_move_device", "gsr_debug_check_device_source",
    "gsr_set_row_band", "gsr_read_row_work", "gsr_debug_balance_rows", "gsr_multi_get_bands",
    "gsr_set_visibility", "gsr_get_visibility", "gsr_visibility_eval", "gsr_multi_set_visibility", "gsplat_renderer_set_visibility",
    "gsr_remove", "gsr_remove_map", "gsr_get_removal", "gsr_multi_remove",
    "gsr_add", "gsr_add_device", "gsr_add_capacity", "gsr_get_add", "gsr_multi_add",
    "gsr_read_info", "gsr_read", "gsr_read_device", "gsr_get_read", "gsr_multi_read",
    "gsr_copy_map", "gsr_read_masked", "gsr_read_masked_device", "gsr_duplicate", "gsr_get_duplicate", "gsr_multi_read_masked", "gsr_multi_duplicate",
    "gsr_debug_replica_verdict",
    "gsr_select", "gsr_select_eval", "gsr_get_select", "gsr_multi_select",
    "gsr_select_attrs", "gsr_select_attrs_eval", "gsr_get_select_attrs", "gsr_multi_select_attrs",
    "gsr_select_density", "gsr_select_density_eval", "gsr_get_select_density", "gsr_multi_select_density",
    "gsr_select_connected", "gsr_select_connected_eval", "gsr_get_select_connected", "gsr_debug_select_connected_stages",
    "gsr_multi_select_connected",
    "gsr_render_marks", "gsr_get_marks",
    "gsr_measure", "gsr_measure_eval", "gsr_hist_prepare", "gsr_get_measure", "gsr_multi_measure",
    "gsr_xform_prepare", "gsr_transform_eval", "gsr_transform", "gsr_get_transform", "gsr_multi_transform",
    "gsr_grade_prepare", "gsr_grade_eval", "gsr_grade", "gsr_get_grade", "gsr_multi_grade",
    "gsr_debug_live_handles", "gsr_debug_sort_frame", "gsr_debug_last_plan", "gsr_debug_stage_bytes",
]


def live_handles():
    """gsr_debug_live_handles (no context, no GPU): what the library's host code holds in this process right now, as
    (device buffers, pinned host buffers, events, streams).  Four zeros before the first context, and again after the last close()"""
    out = (C.c_int64 * 4)()
    _check(load_library().gsr_debug_live_handles(out))
    return tuple(int(v) for v in out)


def balance_rows(row_work, count: int, cur_first=None, min_gain_permille: int = 0):
    """gsr_debug_balance_rows (host only, no GPU): uint32 row_work[tiles_y] -> (changed: bool, int32 boundaries[count + 1]) of the
    contiguous partition into `count` bands with the smallest largest band sum; with cur_first the proposal is adopted only if it cuts
    the largest sum by min_gain_permille.  Raises GsrError on a bad argument"""
    L = load_library()
    w = np.ascontiguousarray(row_work, dtype=np.uint32).reshape(-1)
    cur = None if cur_first is None else np.ascontiguousarray(cur_first, dtype=np.int32).reshape(-1)
    if cur is not None and cur.size != count + 1:
        raise ValueError("cur_first holds count + 1 boundaries")
    out = np.zeros(max(int(count), 0) + 1, np.int32)
    rc = L.gsr_debug_balance_rows(_ptr(w) if w.size else None, int(w.size), int(count), _ptr(cur), int(min_gain_permille), out.ctypes.data)
    _check(rc if rc < 0 else 0)
    return bool(rc), out


REPLICA_KEEP_REFUSAL, REPLICA_AGREED, REPLICA_DROP_ALL = range(3)     # GSR_REPLICA_*: gsr_debug_replica_verdict


def replica_verdict(rc: int, counts) -> int:
    """gsr_debug_replica_verdict (host only, no GPU): the agreement rule of gsr_multi_remove, _add, _duplicate, _transform and _grade.
    rc: what the ranks returned together; counts: int64 (ranks, per_rank), -1 where a rank did not return GSR_OK -> REPLICA_*.
    Raises GsrError on a bad argument"""
    a = np.ascontiguousarray(counts, dtype=np.int64)
    if a.ndim != 2:
        raise ValueError("counts is (ranks, per_rank)")
    out = C.c_int(-1)
    _check(load_library().gsr_debug_replica_verdict(int(rc), a.shape[0], a.shape[1], _ptr(a) if a.size else None, C.byref(out)))
    return out.value


# gsr_debug_sort_frame's modes (include/gsplat_hip.h)
SORT_GLOBAL, SORT_GLOBAL_MID, SORT_LOCAL_GATHER, SORT_LOCAL_K1, SORT_LOCAL_DIRECT, SORT_ORDERED = range(6)
# GSR_PLAN_OUT_FIELDS of csrc/gsr_frame_plan.h, in their order (gsr_debug_last_plan)
PLAN_FIELDS = ("deferred", "lazy", "cull", "jumped", "cull_dilate", "phase", "timing", "timing_all", "dcull", "cache_hit", "want_pos",
               "ordered", "key_bits", "n_slots", "held", "local", "local_phase", "k1_scatters", "bk_lo", "bk_shift", "scatter_direct",
               "mid_sort", "k1_grid", "bn_items", "bn_blocks", "bn_grid")

# the int32 words of gsr_debug_read_horizon_pyramid, in their order (the six level offsets are one entry)
PYRAMID_LEVELS = 6
PYRAMID_META_FIELDS = ("tiles_x", "tiles_y", "pyr_off", "rect_shift", "super_shift", "key_min", "key_max", "hpyr_re", "horizon_valid", "stiles_x",
                       "list_cap", "stat_in_use", "depth_culled", "culled", "shard_index", "shard_count", "shard_rpb", "shard_first", "local_tiles_y")

POLICY_FIELDS = ("cull_pays", "cull_weak", "vis_unculled", "cull_holdoff", "cull_backoff", "cull_streak", "cull_dilate", "opt_dilate",
                 "slab_holdoff", "local_fails", "local_holdoff")


def lib_path() -> str:
    """the in-tree library; GSR_LIBRARY names another build of the same sources (the sanitizer builds of tools/build_sanitized.sh)"""
    return os.environ.get("GSR_LIBRARY") or _build.LIB


def load_library() -> C.CDLL:
    """dlopen the in-tree libgsplat_hip.so (never builds implicitly on a GPU box: the .so travels)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise GsrError(-100, f"{path} is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950) first")
    L = C.CDLL(path)
    vp, i32, i64, f32p = C.c_void_p, C.c_int, C.c_int64, C.POINTER(C.c_float)
    L.gsr_device_count.restype = i32
    L.gsr_last_error.restype = C.c_char_p
    L.gsr_version.restype = C.c_char_p
    L.gsr_create.argtypes = [i32, C.POINTER(vp)]
    L.gsr_destroy.argtypes = [vp]
    L.gsr_destroy.restype = None
    L.gsr_set_stream.argtypes = [vp, vp]
    L.gsr_upload_begin.argtypes = [vp, i64, i32, f32p]
    L.gsr_upload_append.argtypes = [vp, i64] + [vp] * 8
    L.gsr_upload_append_raw.argtypes = [vp, i64, C.POINTER(gsr_raw_attrs)]
    L.gsr_upload_end.argtypes = [vp]
    L.gsr_update.argtypes = [vp, i64, i64, C.POINTER(gsr_attr_update)]
    L.gsr_multi_update.argtypes = [vp, i64, i64, C.POINTER(gsr_attr_update)]
    L.gsr_move.argtypes = [vp, i64, i64, vp, f32p, C.POINTER(gsr_attr_update)]
    L.gsr_multi_move.argtypes = [vp, i64, i64, vp, f32p, C.POINTER(gsr_attr_update)]
    L.gsplat_renderer_move_splats.argtypes = [vp, C.c_char_p, vp, f32p] + [vp] * 7 + [C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.gsr_upload_append_device.argtypes = [vp, i64, C.POINTER(gsr_device_attrs)]
    L.gsr_update_device.argtypes = [vp, i64, i64, C.POINTER(gsr_device_attrs)]
    L.gsr_move_device.argtypes = [vp, i64, i64, f32p, C.POINTER(gsr_device_attrs)]
    L.gsr_debug_check_device_source.argtypes = [vp, vp, i64]
    L.gsr_debug_live_handles.argtypes = [C.POINTER(C.c_int64)]
    L.gsr_debug_stage_bytes.argtypes = [vp]
    L.gsr_debug_stage_bytes.restype = i64
    L.gsr_debug_read_resident.argtypes = [vp, i32, vp, i64]
    L.gsr_set_visibility.argtypes = [vp, C.POINTER(gsr_visibility)]
    L.gsr_get_visibility.argtypes = [vp, C.POINTER(gsr_visibility), C.POINTER(C.c_int64)]
    L.gsr_visibility_eval.argtypes = [C.POINTER(gsr_visibility), vp, i64, i64, vp]
    L.gsr_multi_set_visibility.argtypes = [vp, C.POINTER(gsr_visibility)]
    L.gsplat_renderer_set_visibility.argtypes = [vp, C.POINTER(gsr_visibility)]
    L.gsr_remove.argtypes = [vp, vp, i32, i32, C.POINTER(C.c_int64)]
    L.gsr_remove_map.argtypes = [vp, i64, vp, C.POINTER(C.c_int64)]
    L.gsr_get_removal.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    L.gsr_multi_remove.argtypes = [vp, vp, i32, C.POINTER(C.c_int64)]
    L.gsr_add.argtypes = [vp, i64] + [vp] * 8 + [C.POINTER(C.c_int64)]
    L.gsr_add_device.argtypes = [vp, i64, C.POINTER(gsr_device_attrs), C.POINTER(C.c_int64)]
    L.gsr_add_capacity.argtypes = [i64, i64]
    L.gsr_add_capacity.restype = i64
    L.gsr_get_add.argtypes = [vp] + [C.POINTER(C.c_int64)] * 4 + [C.POINTER(C.c_double)]
    L.gsr_multi_add.argtypes = [vp, i64] + [vp] * 8 + [C.POINTER(C.c_int64)]
    L.gsr_read_info.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int), f32p]
    L.gsr_read.argtypes = [vp, i64, i64, C.POINTER(gsr_read_arrays)]
    L.gsr_read_device.argtypes = [vp, i64, i64, C.POINTER(gsr_device_out)]
    L.gsr_get_read.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    L.gsr_multi_read.argtypes = [vp, i64, i64, C.POINTER(gsr_read_arrays)]
    L.gsr_copy_map.argtypes = [vp, i64, vp, C.POINTER(C.c_int64)]
    L.gsr_read_masked.argtypes = [vp, vp, i32, i64, C.POINTER(gsr_read_arrays), C.POINTER(C.c_int64)]
    L.gsr_read_masked_device.argtypes = [vp, vp, i32, i64, C.POINTER(gsr_device_out), C.POINTER(C.c_int64)]
    L.gsr_duplicate.argtypes = [vp, vp, i32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.gsr_get_duplicate.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    L.gsr_multi_read_masked.argtypes = [vp, vp, i64, C.POINTER(gsr_read_arrays), C.POINTER(C.c_int64)]
    L.gsr_multi_duplicate.argtypes = [vp, vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.gsr_select.argtypes = [vp, C.POINTER(gsr_camera), C.POINTER(gsr_select_region), vp, i32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.gsr_select_eval.argtypes = [C.POINTER(gsr_camera), f32p, C.POINTER(gsr_select_region), vp, vp, i64, vp, vp]
    L.gsr_get_select.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    L.gsr_multi_select.argtypes = [vp, C.POINTER(gsr_camera), C.POINTER(gsr_select_region), vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.gsr_select_attrs.argtypes = [vp, C.POINTER(gsr_attr_rule), vp, i32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.gsr_select_attrs_eval.argtypes = [C.POINTER(gsr_attr_rule), C.POINTER(gsr_visibility), i64, vp, vp, vp, vp, vp]
    L.gsr_get_select_attrs.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    L.gsr_multi_select_attrs.argtypes = [vp, C.POINTER(gsr_attr_rule), vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.gsr_select_density.argtypes = [vp, C.POINTER(gsr_density_rule), vp, i32, vp, i32, C.POINTER(gsr_density_result), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.gsr_select_density_eval.argtypes = [C.POINTER(gsr_density_rule), C.POINTER(gsr_visibility), i64, vp, vp, vp, vp, C.POINTER(gsr_density_result)]
    L.gsr_get_select_density.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    L.gsr_multi_select_density.argtypes = [vp, C.POINTER(gsr_density_rule), vp, vp, C.POINTER(gsr_density_result), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.gsr_select_connected.argtypes = [vp, C.POINTER(gsr_connect_rule), vp, i32, vp, i32, vp, vp, i32, C.POINTER(gsr_connect_result),
                                       C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.gsr_select_connected_eval.argtypes = [C.POINTER(gsr_connect_rule), C.POINTER(gsr_visibility), i64, vp, vp, vp, vp, vp, vp, C.POINTER(gsr_connect_result)]
    L.gsr_get_select_connected.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    L.gsr_debug_select_connected_stages.argtypes = [vp, C.POINTER(C.c_double)]
    L.gsr_multi_select_connected.argtypes = [vp, C.POINTER(gsr_connect_rule), vp, vp, vp, vp, C.POINTER(gsr_connect_result), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.gsr_measure.argtypes = [vp, vp, i32, C.POINTER(gsr_measure_request), C.POINTER(gsr_measure_result), vp]
    L.gsr_measure_eval.argtypes = [C.POINTER(gsr_measure_request), C.POINTER(gsr_visibility), i64, vp, vp, vp, vp, vp, C.POINTER(gsr_measure_result), vp]
    L.gsr_hist_prepare.argtypes = [i32, i32, C.c_double, C.c_double, i32, C.POINTER(gsr_hist_spec)]
    L.gsr_get_measure.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    L.gsr_multi_measure.argtypes = [vp, vp, C.POINTER(gsr_measure_request), C.POINTER(gsr_measure_result), vp]
    L.gsr_xform_prepare.argtypes =[C.POINTER(gsr_xform), C.POINTER(gsr_xform_rule)]
    L.gsr_transform_eval.argtypes = [C.POINTER(gsr_xform), i64] + [vp] * 7
    L.gsr_transform.argtypes = [vp, vp, i32, C.POINTER(gsr_xform), C.POINTER(C.c_int64)]
    L.gsr_get_transform.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    L.gsr_multi_transform.argtypes = [vp, vp, C.POINTER(gsr_xform), C.POINTER(C.c_int64)]
    L.gsr_grade_prepare.argtypes = [C.POINTER(gsr_grade_params), C.POINTER(gsr_grade_rule)]
    L.gsr_grade_eval.argtypes = [C.POINTER(gsr_grade_rule), i64, vp, i32] + [vp] * 5
    L.gsr_grade.argtypes = [vp, vp, i32, C.POINTER(gsr_grade_rule), C.POINTER(C.c_int64)]
    L.gsr_get_grade.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    L.gsr_multi_grade.argtypes = [vp, vp, C.POINTER(gsr_grade_rule), C.POINTER(C.c_int64)]
    L.gsplat_renderer_update_attributes.argtypes = [vp, C.c_char_p] + [vp] * 7 + [C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.gsplat_renderer_row_array.argtypes = [vp, C.c_char_p, i32]
    L.gsplat_renderer_row_array.restype = vp
    L.gsr_upload_abort.argtypes = [vp]
    L.gsr_upload.argtypes = [vp, i64] + [vp] * 8 + [f32p]
    L.gsr_set_row_shard.argtypes = [vp, i32, i32]
    L.gsr_band_rows.argtypes = [i32, i32, i32]
    L.gsr_stitch_bands.argtypes = [vp, vp, i32, i32, i32, vp]
    L.gsr_render.argtypes = [vp, C.POINTER(gsr_camera), vp, i32]
    L.gsr_render_depth.argtypes = [vp, C.POINTER(gsr_camera), vp, i32, vp, i32]
    L.gsr_render_aov.argtypes = [vp, C.POINTER(gsr_camera), vp, i32, vp, i32, i32, vp]
    L.gsr_resolve_depth.argtypes = [vp, i64, C.c_float, vp]
    L.gsr_resolve_depth_device.argtypes = [vp, vp, i64, C.c_float, vp]
    L.gsplat_renderer_set_aov_target.argtypes = [vp, i32, vp]
    L.gsr_render_over.argtypes = [vp, C.POINTER(gsr_camera), vp, i32, C.POINTER(gsr_background), vp, i32]
    L.gsr_composite_over.argtypes = [vp, i64, C.POINTER(gsr_background), i32, vp]
    L.gsplat_renderer_set_background.argtypes = [vp, C.POINTER(gsr_background)]
    L.gsr_render_wire.argtypes = [vp, C.POINTER(gsr_camera), vp, i32]
    L.gsr_render_wire_over.argtypes = [vp, C.POINTER(gsr_camera), vp, i32]
    L.gsr_render_marks.argtypes = [vp, C.POINTER(gsr_camera), vp, i32, C.POINTER(gsr_mark_style), vp, i32, C.POINTER(C.c_int64)]
    L.gsr_get_marks.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    L.gsr_synchronize.argtypes = [vp]
    L.gsr_get_stats.argtypes = [vp, C.POINTER(gsr_stats)]
    L.gsr_stats_reset.argtypes = [vp]
    L.gsr_set_option.argtypes = [vp, i32, i32]
    L.gsr_debug_read_records.argtypes = [vp, vp, i64]
    L.gsr_debug_read_depth_order.argtypes = [vp, vp, i64, C.POINTER(C.c_int64)]
    L.gsr_debug_read_cull.argtypes = [vp, vp, i64, vp, i64, C.POINTER(C.c_int64)]
    L.gsr_debug_read_tile_lists.argtypes = [vp, vp, vp, i64, vp, i64]
    L.gsr_debug_read_storage_order.argtypes = [vp, vp, i64]
    L.gsr_debug_sort_pairs.argtypes = [vp, vp, vp, i64, i32]
    L.gsr_debug_sort_pairs_local.argtypes = [vp, vp, vp, i64, i32, C.c_uint32, i32]
    L.gsr_debug_sort_frame.argtypes = [vp, i32, vp, vp, vp, i64, i64, i32, i32, C.c_uint32, i32, i32, i32, C.POINTER(C.c_int64), C.POINTER(C.c_uint32)]
    L.gsr_debug_last_plan.argtypes = [vp, vp]
    L.gsr_debug_policy.argtypes = [vp, i32, C.c_longlong, C.c_longlong]
    L.gsr_debug_policy_state.argtypes = [vp, vp]
    L.gsr_debug_frame_plan.argtypes = [i32, vp, vp, vp]
    L.gsr_debug_read_tile_work.argtypes = [vp, vp, i64]
    L.gsr_debug_read_horizons.argtypes = [vp, vp, i64]
    L.gsr_debug_read_horizon_pyramid.argtypes = [vp, vp, i64, vp]
    L.gsr_target_pixel_bytes.argtypes = [i32]
    L.gsr_set_target_format.argtypes = [vp, i32]
    L.gsr_get_target_format.argtypes = [vp]
    L.gsr_multi_set_target_format.argtypes = [vp, i32]
    L.gsr_convert_pixels.argtypes = [vp, i64, i32, vp]
    L.gsplat_renderer_set_target_format.argtypes = [vp, i32]
    L.gsplat_renderer_get_target_format.argtypes = [vp]
    # host shim wrappers
    L.gsplat_renderer_create.restype = vp
    L.gsplat_renderer_create.argtypes = [i32]
    L.gsplat_renderer_get_instance.restype = vp
    L.gsplat_renderer_destroy.argtypes = [vp]
    L.gsplat_renderer_destroy.restype = None
    L.gsplat_renderer_register_update.argtypes = [vp, C.c_uint64, C.POINTER(C.c_int64), i64, i64, f32p] + [vp] * 8 + \
                                                 [i64, C.c_char_p, i32]
    L.gsplat_renderer_include_in_render_pass.argtypes = [vp, C.c_char_p]
    L.gsplat_renderer_include_in_render_pass.restype = None
    L.gsplat_renderer_flush_entries_for_matching_detail.argtypes = [vp, C.c_char_p]
    L.gsplat_renderer_flush_entries_for_matching_detail.restype = None
    L.gsplat_renderer_generate_render_geometry.argtypes = [vp, C.POINTER(GSplatRenderContext)]
    L.gsplat_renderer_generate_render_geometry.restype = None
    L.gsplat_renderer_render.argtypes = [vp, C.POINTER(GSplatRenderContext), i32]
    L.gsplat_renderer_render.restype = None
    L.gsplat_renderer_post_render.argtypes = [vp]
    L.gsplat_renderer_post_render.restype = None
    L.gsplat_renderer_redraw.argtypes = [vp, C.POINTER(C.c_char_p), i32, C.POINTER(GSplatRenderContext), i32]
    L.gsplat_renderer_redraw.restype = None
    L.gsplat_renderer_set_rendering_enabled.argtypes = [vp, i32]
    L.gsplat_renderer_set_rendering_enabled.restype = None
    L.gsplat_renderer_set_explicit_camera_pos.argtypes = [vp, f32p]
    L.gsplat_renderer_set_explicit_camera_pos.restype = None
    L.gsplat_renderer_set_spherical_harmonics_order.argtypes = [vp, i32]
    L.gsplat_renderer_set_spherical_harmonics_order.restype = None
    L.gsplat_renderer_query.argtypes = [vp, i32, C.c_char_p]
    L.gsplat_renderer_query.restype = i64
    L.gsplat_renderer_get_origin.argtypes = [vp, f32p]
    L.gsplat_renderer_get_origin.restype = None
    L.gsplat_renderer_get_last_camera_pos.argtypes = [vp, f32p]
    L.gsplat_renderer_get_last_camera_pos.restype = None
    L.gsplat_renderer_engine.argtypes = [vp]
    L.gsplat_renderer_engine.restype = vp
    L.gsplat_closest_sqrt_power_of_2.argtypes = [i32]
    L.gsplat_closest_sqrt_power_of_2.restype = C.c_uint
    L.gsplat_quantize_half.argtypes = [vp, vp, i64]
    L.gsplat_quantize_half.restype = None
    L.gsplat_pack_sh_from_vec3.argtypes = [C.POINTER(vp), i64, vp, vp, vp]
    L.gsplat_pack_sh_from_vec3.restype = None
    L.gsplat_pack_sh_from_frest.argtypes = [C.POINTER(vp), i64, vp, vp, vp]
    L.gsplat_pack_sh_from_frest.restype = None
    L.gsplat_pack_sh_from_array.argtypes = [vp, i64, i32, vp, vp, vp]
    L.gsplat_pack_sh_from_array.restype = None
    # several GPUs
    L.gsr_multi_create.argtypes = [C.POINTER(C.c_int), i32, i32, C.POINTER(vp)]
    L.gsr_multi_destroy.argtypes = [vp]
    L.gsr_multi_destroy.restype = None
    L.gsr_multi_count.argtypes = [vp]
    L.gsr_multi_transport.argtypes = [vp]
    L.gsr_multi_context.argtypes = [vp, i32]
    L.gsr_multi_context.restype = vp
    L.gsr_multi_set_stream.argtypes = [vp, vp]
    L.gsr_multi_set_option.argtypes = [vp, i32, i32]
    L.gsr_multi_upload_begin.argtypes = [vp, i64, i32, f32p]
    L.gsr_multi_upload_append.argtypes = [vp, i64] + [vp] * 8
    L.gsr_multi_upload_end.argtypes = [vp]
    L.gsr_multi_upload_abort.argtypes = [vp]
    L.gsr_multi_upload.argtypes = [vp, i64] + [vp] * 8 + [f32p]
    L.gsr_multi_render.argtypes = [vp, C.POINTER(gsr_camera), vp, i32]
    L.gsr_multi_render_depth.argtypes = [vp, C.POINTER(gsr_camera), vp, i32, vp, i32]
    L.gsr_multi_synchronize.argtypes = [vp]
    L.gsr_multi_get_stats.argtypes = [vp, i32, C.POINTER(gsr_stats)]
    L.gsr_multi_comm_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.gsr_set_row_band.argtypes = [vp, i32, i32]
    L.gsr_read_row_work.argtypes = [vp, vp, i32, C.POINTER(C.c_int64)]
    L.gsr_debug_balance_rows.argtypes = [vp, i32, i32, vp, i32, vp]
    L.gsr_debug_replica_verdict.argtypes = [i32, i32, i32, vp, C.POINTER(C.c_int)]
    L.gsr_multi_get_bands.argtypes = [vp, vp, C.POINTER(C.c_int64)]
    L.gsr_multi_gather_stats.argtypes = [vp, i32, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    L.gsr_comm_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.gsr_comm_get_unique_id.argtypes = [vp]
    L.gsr_comm_init.argtypes = [vp, vp, i32, i32]
    L.gsr_comm_destroy.argtypes = [vp]
    L.gsr_comm_render.argtypes = [vp, C.POINTER(gsr_camera), vp, i32, vp]
    L.gsplat_renderer_create_multi.argtypes = [C.POINTER(C.c_int), i32, i32]
    L.gsplat_renderer_create_multi.restype = vp
    L.gsplat_renderer_multi.argtypes = [vp]
    L.gsplat_renderer_multi.restype = vp
    # the viewport primitive's part (N1 ingest)
    L.gsplat_prim_create.argtypes = [vp]
    L.gsplat_prim_create.restype = vp
    L.gsplat_prim_destroy.argtypes = [vp]
    L.gsplat_prim_destroy.restype = None
    L.gsplat_prim_update.argtypes = [vp, C.c_uint64, C.POINTER(C.c_int64), i64, C.POINTER(gsplat_attrs), f32p, C.c_char_p, i32]
    L.gsplat_prim_render.argtypes = [vp, i32]
    L.gsplat_prim_render.restype = None
    L.gsplat_prim_missing.argtypes = [vp]
    L.gsplat_prim_missing.restype = C.c_uint
    L.gsplat_prim_sh_order.argtypes = [vp]
    L.gsplat_prim_has_sh.argtypes = [vp]
    L.gsplat_prim_array.argtypes = [vp, i32]
    L.gsplat_prim_array.restype = vp
    _LIB = L
    return L


def _check(rc: int):
    if rc != 0:
        raise GsrError(rc, load_library().gsr_last_error().decode("utf-8", "replace"))


def _ptr(a):
    return None if a is None else a.ctypes.data


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def target_dtype(fmt: int) -> np.dtype:
    """the numpy channel type of a target format (float32 / float16 / uint8)"""
    if fmt not in TARGET_DTYPES:
        raise GsrError(-1, f"unknown target format {fmt}")
    return TARGET_DTYPES[fmt]


def convert_pixels(rgba: np.ndarray, fmt: int) -> np.ndarray:
    """gsr_convert_pixels: float32 [..., 4] pixels -> the same shape in the target format's channel type, on the host, by the
    rule the kernels store with (RGBA16F: round to nearest even; RGBA8: clamp, one fma rounding, truncate)"""
    a = np.ascontiguousarray(rgba, dtype=np.float32)
    if a.ndim == 0 or a.shape[-1] != 4:
        raise GsrError(-1, "convert_pixels: the last axis must hold the four channels")
    out = np.empty(a.shape, dtype=target_dtype(fmt))
    _check(load_library().gsr_convert_pixels(a.ctypes.data, a.size // 4, int(fmt), out.ctypes.data))
    return out


def background_struct(bg, shape=None):
    """a background as gsr_background: None (kind 0), a premultiplied colour (r, g, b, a), or an ndarray [..., 4] of float32 / float16 /
    uint8 -- the image format is inferred from the dtype -- which must hold shape[0] x shape[1] pixels if `shape` is given.  Returns
    (struct, the array the struct points into: keep it alive as long as the struct is used)"""
    b = gsr_background()
    if bg is None:
        return b, None
    if isinstance(bg, np.ndarray) and bg.ndim >= 2:
        fmt = {np.dtype(np.float32): TARGET_RGBA32F, np.dtype(np.float16): TARGET_RGBA16F, np.dtype(np.uint8): TARGET_RGBA8}.get(bg.dtype)
        if fmt is None or bg.shape[-1] != 4:
            raise GsrError(-1, "a background image is float32, float16 or uint8 [..., 4]")
        img = np.ascontiguousarray(bg)
        if shape is not None and img.size != int(shape[0]) * int(shape[1]) * 4:
            raise GsrError(-1, f"the background image must hold {shape[0]} x {shape[1]} pixels")
        b.kind, b.format, b.image, b.image_is_device = BG_IMAGE, fmt, img.ctypes.data, 0
        return b, img
    col = [float(x) for x in np.asarray(bg, dtype=np.float32).reshape(-1)]
    if len(col) != 4:
        raise GsrError(-1, "a background colour is (r, g, b, a), premultiplied")
    b.kind = BG_COLOUR
    b.rgba[:] = col
    return b, None


def composite_over(rgba32f: np.ndarray, bg, fmt: int = TARGET_RGBA32F) -> np.ndarray:
    """gsr_composite_over: float32 [..., 4] pixels over `bg` (a colour, or an image of as many pixels: background_struct) -> the same
    shape in the channel type of `fmt`, on the host, by the rule k_blend_over composites and stores with"""
    a = np.ascontiguousarray(rgba32f, dtype=np.float32)
    if a.ndim == 0 or a.shape[-1] != 4:
        raise GsrError(-1, "composite_over: the last axis must hold the four channels")
    b, keep = background_struct(bg)
    if keep is not None and keep.size != a.size:
        raise GsrError(-1, "composite_over: the background image must hold as many pixels as the frame")
    out = np.empty(a.shape, dtype=target_dtype(fmt))
    _check(load_library().gsr_composite_over(a.ctypes.data, a.size // 4, C.byref(b), int(fmt), out.ctypes.data))
    return out


def resolve_depth(aov: np.ndarray, cov_min: float = 0.5) -> np.ndarray:
    """gsr_resolve_depth: a depth-AOV plane [..., 2] = {zsum, cov} -> float32 window depth [...], on the host:
    cov >= cov_min ? min(zsum / cov, 1) : 1.  What gsr_render_depth (or GL) accepts as a depth buffer."""
    a = np.ascontiguousarray(aov, dtype=np.float32)
    if a.ndim == 0 or a.shape[-1] != 2:
        raise GsrError(-1, "resolve_depth: the last axis must hold {zsum, cov}")
    out = np.empty(a.shape[:-1], dtype=np.float32)
    _check(load_library().gsr_resolve_depth(a.ctypes.data, a.size // 2, float(cov_min), out.ctypes.data))
    return out


def _crop_to_unit(centre, half_extents, rotation3x3):
    """to_unit[12] (rows of a 3x4 map, float32) of a volume with the given centre, half extents and orientation (the columns of
    rotation3x3 are the volume's axes in upload space; None = axis-aligned): q = diag(1 / h) R^T (P - centre), formed in float64 and
    rounded once.  Dyadic extents and an axis-aligned volume give dyadic entries, so centre +- h lands on +-1 exactly."""
    c = np.asarray(centre, dtype=np.float64).reshape(3)
    h = np.asarray(half_extents, dtype=np.float64).reshape(-1)
    h = np.repeat(h, 3) if h.size == 1 else h.reshape(3)
    R = np.eye(3) if rotation3x3 is None else np.asarray(rotation3x3, dtype=np.float64).reshape(3, 3)
    A = R.T / h[:, None]
    return np.concatenate([A, -(A @ c)[:, None]], axis=1).astype(np.float32).reshape(12)


def crop_box(centre, half_extents, rotation3x3=None, invert: bool = False):
    """a box volume (kind, invert, to_unit12) for visibility_struct: centre + R diag(half_extents) [-1, 1]^3"""
    return (VOL_BOX, int(bool(invert)), _crop_to_unit(centre, half_extents, rotation3x3))


def crop_ellipsoid(centre, half_extents, rotation3x3=None, invert: bool = False):
    """an ellipsoid volume (kind, invert, to_unit12) for visibility_struct: semi-axes half_extents along the columns of rotation3x3"""
    return (VOL_ELLIPSOID, int(bool(invert)), _crop_to_unit(centre, half_extents, rotation3x3))


def pack_mask(hidden) -> np.ndarray:
    """a boolean array (True = hidden, upload order) -> the uint32 words gsr_visibility.mask takes: bit (i & 31) of word (i >> 5)"""
    h = np.asarray(hidden, dtype=bool).reshape(-1)
    bits = np.zeros((h.size + 31) // 32 * 32, np.uint8)
    bits[:h.size] = h
    return np.packbits(bits, bitorder="little").view("<u4").astype(np.uint32)


def visibility_struct(volumes=(), mask=None):
    """gsr_visibility from volumes = [(kind, invert, to_unit12), ...] (crop_box / crop_ellipsoid build them) and mask = a boolean array,
    True = hidden, one entry per resident splat in upload order (or None) -> (struct, the words it points into: keep them alive
    during the call).  The counts and kinds are the library's to refuse."""
    v, keep = gsr_visibility(), None
    volumes = list(volumes)
    v.n_volumes = len(volumes)
    for k, (kind, invert, to_unit) in enumerate(volumes[:VIS_MAX_VOLUMES]):
        v.volume[k].kind, v.volume[k].invert = int(kind), int(invert)
        v.volume[k].to_unit[:] = np.asarray(to_unit, dtype=np.float32).reshape(12).tolist()
    if mask is not None:
        m = np.asarray(mask).reshape(-1)
        keep = pack_mask(m)
        if keep.size == 0:
            keep = np.zeros(1, np.uint32)
        v.mask, v.mask_splats = keep.ctypes.data, m.size
    return v, keep


def visibility_eval(vis, P, first: int = 0) -> np.ndarray:
    """gsr_visibility_eval: the rule of gsr_set_visibility on the host, through the function the kernel evaluates.  vis: a gsr_visibility
    (visibility_struct) or None; P: float32 (n, 3) = the splats [first, first + n) as far as a mask is concerned -> bool (n,), True = visible"""
    P = np.ascontiguousarray(P, dtype=np.float32).reshape(-1, 3)
    out = np.zeros(P.shape[0], np.uint8)
    _check(load_library().gsr_visibility_eval(C.byref(vis) if vis is not None else None, P.ctypes.data if P.size else None, int(first),
                                              P.shape[0], out.ctypes.data if P.size else None))
    return out.astype(bool)


def removal_mask(mask) -> np.ndarray:
    """what gsr_remove takes from a caller's mask: a boolean array (True = the splat goes, upload order) is packed with pack_mask; an
    array of uint32 is taken as the packed words it already is.  Never empty (a cloud of no splats still hands a word over)."""
    m = np.asarray(mask)
    if m.dtype == np.uint32:
        words = np.ascontiguousarray(m).reshape(-1)
    elif m.dtype == np.bool_:
        words = pack_mask(m)
    else:
        raise GsrError(-1, f"remove: the mask is {m.dtype}, neither bool (one entry per splat) nor uint32 (packed words)")
    return words if words.size else np.zeros(1, np.uint32)


def removal_words(mask, n: int):
    """removal_mask for a cloud of n resident splats: a boolean mask must hold n entries and packed words must cover n bits -- the
    library reads ceil(n / 32) words and cannot know how many the caller has"""
    m = None if mask is None else np.asarray(mask)
    if m is None:
        return None
    if m.dtype == np.bool_ and m.size != int(n):
        raise GsrError(-1, f"remove: the mask holds {m.size} entries, {int(n)} splats are resident")
    words = removal_mask(m)
    if words.size * 32 < int(n):
        raise GsrError(-1, f"remove: {words.size} mask words do not cover the {int(n)} resident splats")
    return words


def remove_map(mask, n=None):
    """gsr_remove_map (host only, no GPU): where gsr_remove puts the survivors.  mask as removal_mask takes it; n = the splat count
    (from a boolean mask's length when None) -> (int32 new_index[n]: the new upload index, -1 for a removed splat; the splats left)"""
    m = np.asarray(mask)
    if n is None:
        if m.dtype != np.bool_:
            raise GsrError(-1, "remove_map: packed words do not say how many splats they cover: n must be given")
        n = m.size
    words = removal_mask(m)
    if words.size * 32 < int(n):
        raise GsrError(-1, f"remove_map: {words.size} words do not cover {int(n)} splats")
    out, left = np.zeros(max(int(n), 0), np.int32), C.c_int64(0)
    _check(load_library().gsr_remove_map(words.ctypes.data, int(n), out.ctypes.data if out.size else None, C.byref(left)))
    return out, left.value


def copy_map(mask, n=None):
    """gsr_copy_map (host only, no GPU): the rows gsr_read_masked returns and gsr_duplicate copies.  mask as removal_mask takes it (True =
    selected); n = the splat count (from a boolean mask's length when None) -> (int32 rows[m]: the upload indices of the selected splats,
    ascending; m)"""
    m = np.asarray(mask)
    if n is None:
        if m.dtype != np.bool_:
            raise GsrError(-1, "copy_map: packed words do not say how many splats they cover: n must be given")
        n = m.size
    words = removal_mask(m)
    if words.size * 32 < int(n):
        raise GsrError(-1, f"copy_map: {words.size} words do not cover {int(n)} splats")
    out, cnt = np.zeros(max(int(n), 0), np.int32), C.c_int64(0)
    _check(load_library().gsr_copy_map(words.ctypes.data, int(n), out.ctypes.data if out.size else None, C.byref(cnt)))
    return out[:cnt.value].copy(), cnt.value


def range_mask(first: int, count: int, n: int) -> np.ndarray:
    """the packed mask words over n splats with the bits [first, first + count) set: after duplicate() -> (m, n_total) the mask of the
    fresh copies is range_mask(n_total - m, m, n_total), what a following transform or grade takes"""
    first, count, n = int(first), int(count), int(n)
    if first < 0 or count < 0 or n < 0 or first + count > n:
        raise GsrError(-1, f"range_mask: [{first}, {first} + {count}) is not within the {n} splats")
    bits = np.zeros(n, bool)
    bits[first:first + count] = True
    return removal_mask(bits)


def _device_mask_ptr(mask, who: str) -> int:
    """a device mask as the *_device verbs take it: an int (a device pointer) or an object with data_ptr() -> the pointer"""
    if isinstance(mask, (bool, np.bool_)) or mask is None:
        raise GsrError(-1, f"{who}: the mask is neither a device pointer (int) nor an object with data_ptr()")
    if isinstance(mask, (int, np.integer)):
        return int(mask)
    if hasattr(mask, "data_ptr"):
        return int(mask.data_ptr())
    raise GsrError(-1, f"{who}: the mask is neither a device pointer (int) nor an object with data_ptr()")


def _read_masked_splats(verb, info, mask, names):
    """Engine.read_masked / MultiEngine.read_masked behind their handles: verb(mask pointer, max_rows, struct, &m); info = (resident
    count, has_sh).  A count call sizes the arrays."""
    from .scenes import Splats
    total, has_sh = info
    words = removal_words(mask, total)
    ptr = None if words is None else words.ctypes.data
    if names is None:
        names = [name for name, _, _ in READ_ARRAYS if has_sh or not name.startswith("sh")]
    unknown = set(names) - {name for name, _, _ in READ_ARRAYS}
    if unknown:
        raise GsrError(-1, f"read_masked: unknown array(s) {sorted(unknown)}")
    m = C.c_int64(0)
    _check(verb(ptr, 0, None, C.byref(m)))
    r, arrays = read_arrays_struct(m.value, tuple(names))
    if m.value and names:
        _check(verb(ptr, m.value, C.byref(r), C.byref(m)))
    return Splats(*[arrays.get(name) for name, _, _ in READ_ARRAYS])


def pack_image(painted) -> np.ndarray:
    """a boolean image (height, width), row 0 at the BOTTOM (GL window coordinates), True = painted -> the uint32 words
    gsr_select_region.image takes: one bit per pixel, packed across rows without padding"""
    words = pack_mask(np.asarray(painted, dtype=bool).reshape(-1))
    return words if words.size else np.zeros(1, np.uint32)


def select_region(rect=None, image=None, depth=None, depth_bias: float = 0.0, op: int = SELECT_REPLACE, any_opacity: bool = False,
                  image_device: int | None = None, depth_device: int | None = None):
    """gsr_select_region -> (struct, the arrays it points into: keep them alive during the call).  rect = (x0, y0, x1, y1) in GL window
    coordinates, half-open (None: everywhere); image = a boolean (height, width) array, row 0 at the bottom, or packed uint32 words
    (pack_image); depth = float32 (height, width) window depths; image_device / depth_device = raw device pointers in their place.
    What the sizes must be is the camera's to say: Engine.select and select_eval check them."""
    r, keep = gsr_select_region(), []
    inf = float("inf")
    r.x0, r.y0, r.x1, r.y1 = (-inf, -inf, inf, inf) if rect is None else [float(v) for v in rect]
    if image is not None and image_device is not None or depth is not None and depth_device is not None:
        raise GsrError(-1, "select_region: a source is given both as an array and as a device pointer")
    if image is not None:
        m = np.asarray(image)
        words = np.ascontiguousarray(m).reshape(-1) if m.dtype == np.uint32 else pack_image(m)
        keep.append(words)
        r.image, r.image_is_device = words.ctypes.data, 0
    elif image_device is not None:
        r.image, r.image_is_device = int(image_device), 1
    if depth is not None:
        d = np.ascontiguousarray(depth, dtype=np.float32).reshape(-1)
        keep.append(d)
        r.depth, r.depth_is_device = d.ctypes.data, 0
    elif depth_device is not None:
        r.depth, r.depth_is_device = int(depth_device), 1
    r.depth_bias, r.op, r.flags = float(depth_bias), int(op), SELECT_ANY_OPACITY if any_opacity else 0
    return r, keep


def _region_fits(cam, keep, who):
    """the host arrays of a select_region against the camera's size: the library reads ceil(w h / 32) words and w h floats"""
    px = int(cam.width) * int(cam.height)
    for a in keep:
        need = (px + 31) // 32 if a.dtype == np.uint32 else px
        if 1 <= int(cam.width) <= MAX_DIM and 1 <= int(cam.height) <= MAX_DIM and a.size < need:
            raise GsrError(-1, f"{who}: the region's {'image' if a.dtype == np.uint32 else 'depth'} holds {a.size} entries, {cam.width}x{cam.height} needs {need}")


def select_eval(cam, origin, region, P, opacity=None, centres: bool = False):
    """gsr_select_eval (host only, no GPU): the rule of gsr_select through the function the kernel evaluates.  region: a gsr_select_region
    or the (struct, keep) pair select_region returns, with HOST sources; P: float32 (n, 3) raw positions; opacity: float32 (n,) RESIDENT
    opacities (None = 1) -> bool (n,) hit, and with centres also float32 (n, 3) = cx, cy, zw of every selectable splat, else NaN"""
    r, keep = region if isinstance(region, tuple) else (region, [])
    _region_fits(cam, keep, "select_eval")
    P = np.ascontiguousarray(P, dtype=np.float32).reshape(-1, 3)
    n = P.shape[0]
    a = None if opacity is None else np.ascontiguousarray(opacity, dtype=np.float32).reshape(-1)
    if a is not None and a.size != n:
        raise GsrError(-1, f"select_eval: {a.size} opacities for {n} positions")
    hit, c = np.zeros(max(n, 1), np.uint8), np.zeros((max(n, 1), 3), np.float32) if centres else None
    cs = cam if isinstance(cam, gsr_camera) else camera_struct(cam)
    _check(load_library().gsr_select_eval(C.byref(cs), _f3(origin), C.byref(r), P.ctypes.data if n else None, _ptr(a) if n else None, n,
                                          hit.ctypes.data, _ptr(c)))
    return (hit[:n].astype(bool), c[:n]) if centres else hit[:n].astype(bool)


def mark_style(shape: int = MARK_DOT, radius: int = 0, colour=(1.0, 1.0, 0.0, 1.0), any_opacity: bool = False, depth=None,
               depth_bias: float = 0.0, depth_device: int | None = None):
    """gsr_mark_style -> (struct, the arrays it points into: keep them alive during the call).  shape = MARK_DOT (radius 0..8 pixels
    around the centre's pixel) or MARK_OUTLINE (radius 0); colour = a premultiplied (r, g, b, a), finite, 0 <= a <= 1, or "cd": each
    splat's own (Cd, 1); depth = float32 (height, width) window depths, depth_device = a raw device pointer in its place.  What the
    depth buffer's size must be is the camera's to say: Engine.render_marks checks it."""
    st, keep = gsr_mark_style(), []
    if shape not in (MARK_DOT, MARK_OUTLINE):
        raise GsrError(-1, f"mark_style: unknown shape {shape!r}")
    if isinstance(radius, (bool, np.bool_)) or not isinstance(radius, (int, np.integer)) or not 0 <= radius <= (MARK_MAX_RADIUS if shape == MARK_DOT else 0):
        raise GsrError(-1, f"mark_style: radius {radius!r} is not within 0..{MARK_MAX_RADIUS} (dots) or not 0 (outlines)")
    st.shape, st.radius = int(shape), int(radius)
    if isinstance(colour, str):
        if colour.lower() != "cd":
            raise GsrError(-1, f"mark_style: colour {colour!r} is neither (r, g, b, a) nor \"cd\"")
        st.colour_mode = MARK_COLOUR_CD
    else:
        col = np.asarray(colour, dtype=np.float32).reshape(-1)
        if col.size != 4 or not np.isfinite(col).all() or not 0.0 <= col[3] <= 1.0:
            raise GsrError(-1, "mark_style: a colour is a finite premultiplied (r, g, b, a) with 0 <= a <= 1")
        st.colour_mode = MARK_COLOUR_FIXED
        st.rgba[:] = [float(x) for x in col]
    if depth is not None and depth_device is not None:
        raise GsrError(-1, "mark_style: the depth buffer is given both as an array and as a device pointer")
    if depth is not None:
        d = np.ascontiguousarray(depth, dtype=np.float32).reshape(-1)
        keep.append(d)
        st.depth, st.depth_is_device = d.ctypes.data, 0
    elif depth_device is not None:
        st.depth, st.depth_is_device = int(depth_device), 1
    st.depth_bias, st.flags = float(depth_bias), MARK_ANY_OPACITY if any_opacity else 0
    return st, keep


def attr_rule(alpha=None, scale_max=None, scale_min=None, anisotropy=None, colour=None, volumes=(), op: int = SELECT_REPLACE,
              skip_hidden: bool = False) -> gsr_attr_rule:
    """gsr_attr_rule: every argument that is not None (volumes: not empty) sets its clause.  alpha, scale_max, scale_min = (lo, hi)
    ranges, inclusive; anisotropy = k (hit iff smax > 0 and smax >= k smin); colour = (lo, hi) with each a scalar or (r, g, b);
    volumes = [(kind, invert, to_unit12), ...] as crop_box / crop_ellipsoid build them; op = SELECT_*; skip_hidden: a splat the
    visibility in force hides is never hit.  What the fields may hold is the library's to refuse."""
    r = gsr_attr_rule()
    r.op, r.flags = int(op), ATTR_SKIP_HIDDEN if skip_hidden else 0
    for bit, rng, lo, hi in ((ATTR_ALPHA, alpha, "alpha_lo", "alpha_hi"), (ATTR_SCALE_MAX, scale_max, "scale_max_lo", "scale_max_hi"),
                             (ATTR_SCALE_MIN, scale_min, "scale_min_lo", "scale_min_hi")):
        if rng is not None:
            r.clauses |= bit
            setattr(r, lo, float(rng[0]))
            setattr(r, hi, float(rng[1]))
    if anisotropy is not None:
        r.clauses |= ATTR_ANISOTROPY
        r.anisotropy = float(anisotropy)
    if colour is not None:
        r.clauses |= ATTR_COLOUR
        r.colour_lo[:] = np.broadcast_to(np.asarray(colour[0], np.float32), (3,)).tolist()
        r.colour_hi[:] = np.broadcast_to(np.asarray(colour[1], np.float32), (3,)).tolist()
    volumes = list(volumes)
    if volumes:
        r.clauses |= ATTR_VOLUME
        r.n_volumes = len(volumes)
        for k, (kind, invert, to_unit) in enumerate(volumes[:VIS_MAX_VOLUMES]):
            r.volume[k].kind, r.volume[k].invert = int(kind), int(invert)
            r.volume[k].to_unit[:] = np.asarray(to_unit, dtype=np.float32).reshape(12).tolist()
    return r


def select_attrs_eval(rule, P=None, alpha=None, scale=None, Cd=None, vis=None) -> np.ndarray:
    """gsr_select_attrs_eval (host only, no GPU): the rule of gsr_select_attrs through the function the kernel evaluates.  Arrays in
    read()'s layout: P float32 (n, 3), alpha float32 (n,) TRUE alphas, scale and Cd uint16 halves (n, 3); an array no set clause looks
    at may be None (at least one array says n).  vis: the gsr_visibility (visibility_struct) that skip_hidden hides by, or None
    -> bool (n,) hit"""
    arrs = [None if a is None else np.ascontiguousarray(a, dtype=t).reshape(-1, w) for a, t, w in
            ((P, np.float32, 3), (alpha, np.float32, 1), (scale, np.uint16, 3), (Cd, np.uint16, 3))]
    sizes = {a.shape[0] for a in arrs if a is not None}
    if len(sizes) != 1:
        raise GsrError(-1, f"select_attrs_eval: the arrays hold {sorted(sizes)} rows")
    n = sizes.pop()
    hit = np.zeros(max(n, 1), np.uint8)
    _check(load_library().gsr_select_attrs_eval(C.byref(rule), C.byref(vis) if vis is not None else None, n,
                                                *[a.ctypes.data if a is not None and n else None for a in arrs], hit.ctypes.data))
    return hit[:n].astype(bool)


def density_rule(cell, origin, reach: int = 1, count=(1, 0xffffffff), alpha_min: float = float("-inf"), op: int = SELECT_REPLACE,
                 skip_hidden: bool = False, hit_outside: bool = False) -> gsr_density_rule:
    """gsr_density_rule: a grid of 1024^3 cells of edge `cell` whose low corner is `origin` (upload space; density_grid makes both
    from a bounding box); reach = how many cells around a splat's own count as its neighbourhood (0..2); count = (lo, hi), hit iff
    lo <= N <= hi ((1, k - 1): the floaters); alpha_min: only splats with a true alpha >= it are counted and hit; op = SELECT_*;
    skip_hidden: a splat the visibility in force hides is not counted; hit_outside: what lies outside the grid is hit.  What the
    fields may hold is the library's to refuse."""
    r = gsr_density_rule()
    r.cell = float(cell)
    r.origin[:] = [float(x) for x in np.asarray(origin, np.float32).reshape(3)]
    r.reach, r.op = int(reach), int(op)
    r.flags = (DENSITY_SKIP_HIDDEN if skip_hidden else 0) | (DENSITY_HIT_OUTSIDE if hit_outside else 0)
    r.count_lo, r.count_hi = int(count[0]), int(count[1])
    r.alpha_min = float(alpha_min)
    return r


def density_grid(lo, hi, cell):
    """(origin float32 (3,), cell float32) of a gsr_density_rule for the bounding box lo .. hi (measure()'s bounds, say): the origin
    lies one cell below lo, so every splat of the box has all its neighbour cells inside the grid.  The box must fit 1022 cells per
    axis at that cell: ValueError otherwise, naming the smallest cell that does.  Pure host arithmetic."""
    lo64, hi64 = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
    c = np.float32(cell)
    if not (np.isfinite(lo64).all() and np.isfinite(hi64).all() and (hi64 >= lo64).all()):
        raise ValueError("density_grid: the box is not finite, or hi is below lo")
    if not (np.isfinite(c) and c > 0):
        raise ValueError(f"density_grid: cell {cell!r} is not a finite positive number")
    extent = float((hi64 - lo64).max())
    smallest = np.float32(extent / (DENSITY_CELLS - 2))
    while float(smallest) * (DENSITY_CELLS - 2) <= extent:         # (strictly more than the extent: hi itself lies inside a cell)
        smallest = np.nextafter(smallest, np.float32(np.inf))
    if float(c) < float(smallest):
        raise ValueError(f"density_grid: a box of extent {extent:g} does not fit {DENSITY_CELLS - 2} cells of {float(c):g}; "
                         f"the smallest cell that fits is {float(smallest):.9g}")
    return (lo64 - float(c)).astype(np.float32), c


def select_density_eval(rule, P, alpha=None, vis=None, counts: bool = False, result: bool = False):
    """gsr_select_density_eval (host only, no GPU): the rule of gsr_select_density through the functions the kernels evaluate.  P
    float32 (n, 3) and alpha float32 (n,) TRUE alphas in read()'s layout (None: every alpha 1); vis: the gsr_visibility
    (visibility_struct) that skip_hidden hides by, or None -> bool (n,) hit; with counts / result also the uint32 (n,) neighbour
    counts / the gsr_density_result, in that order"""
    P = np.ascontiguousarray(P, dtype=np.float32).reshape(-1, 3)
    n = P.shape[0]
    a = None if alpha is None else np.ascontiguousarray(alpha, dtype=np.float32).reshape(-1)
    if a is not None and a.shape[0] != n:
        raise GsrError(-1, f"select_density_eval: the arrays hold {sorted({n, a.shape[0]})} rows")
    hit, cnt, res = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint32), gsr_density_result()
    _check(load_library().gsr_select_density_eval(C.byref(rule), C.byref(vis) if vis is not None else None, n, P.ctypes.data if n else None,
                                                  a.ctypes.data if a is not None and n else None, hit.ctypes.data,
                                                  cnt.ctypes.data if counts else None, C.byref(res) if result else None))
    out = (hit[:n].astype(bool),) + ((cnt[:n],) if counts else ()) + ((res,) if result else ())
    return out[0] if len(out) == 1 else out


def connect_rule(cell, origin, reach: int = 1, size=(1, 0xffffffff), alpha_min: float = float("-inf"), flags: int = 0,
                 op: int = SELECT_REPLACE) -> gsr_connect_rule:
    """gsr_connect_rule: density_rule's grid (cell and origin: density_grid makes both from a bounding box), reach = how far apart two
    occupied cells may be and still be adjacent (0..2); size = (lo, hi), hit iff lo <= the population of the splat's connected
    component <= hi ((1, k - 1): every clump of fewer than k splats); alpha_min: only splats with a true alpha >= it are population;
    flags = CONNECT_SKIP_HIDDEN | CONNECT_HIT_OUTSIDE; op = SELECT_*.  What the fields may hold is the library's to refuse."""
    r = gsr_connect_rule()
    r.cell = float(cell)
    r.origin[:] = [float(x) for x in np.asarray(origin, np.float32).reshape(3)]
    r.reach, r.op, r.flags = int(reach), int(op), int(flags)
    r.size_lo, r.size_hi = int(size[0]), int(size[1])
    r.alpha_min = float(alpha_min)
    return r


def select_connected_eval(rule, P, alpha=None, seed=None, vis=None, labels: bool = False, sizes: bool = False, result: bool = False):
    """gsr_select_connected_eval (host only, no GPU): the rule of gsr_select_connected through the functions the kernels evaluate.  P
    float32 (n, 3) and alpha float32 (n,) TRUE alphas in read()'s layout (None: every alpha 1); seed: a boolean array over the splats
    or packed uint32 words (None: no seed clause); vis: the gsr_visibility that CONNECT_SKIP_HIDDEN hides by, or None -> bool (n,) hit;
    with labels / sizes / result also the uint32 (n,) labels / the uint32 (n,) sizes / the gsr_connect_result, in that order"""
    P = np.ascontiguousarray(P, dtype=np.float32).reshape(-1, 3)
    n = P.shape[0]
    a = None if alpha is None else np.ascontiguousarray(alpha, dtype=np.float32).reshape(-1)
    if a is not None and a.shape[0] != n:
        raise GsrError(-1, f"select_connected_eval: the arrays hold {sorted({n, a.shape[0]})} rows")
    sw = None if seed is None else np.concatenate([removal_words(seed, n), np.zeros(1, np.uint32)])
    hit, lab, siz, res = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32), gsr_connect_result()
    _check(load_library().gsr_select_connected_eval(C.byref(rule), C.byref(vis) if vis is not None else None, n, P.ctypes.data if n else None,
                                                    a.ctypes.data if a is not None and n else None, sw.ctypes.data if sw is not None else None,
                                                    hit.ctypes.data, lab.ctypes.data if labels else None, siz.ctypes.data if sizes else None,
                                                    C.byref(res) if result else None))
    out = (hit[:n].astype(bool),) + ((lab[:n],) if labels else ()) + ((siz[:n],) if sizes else ()) + ((res,) if result else ())
    return out[0] if len(out) == 1 else out


def hist_spec(channel: int, lo: float, hi: float, bins: int, log2: bool = False) -> gsr_hist_spec:
    """gsr_hist_prepare (host only, no GPU): the histogram of `channel` (HIST_*) over [lo, hi) in `bins` bins; log2: of the
    piecewise-linear log2 of the value (lo and hi are then exponents).  Raises GsrError on what the library refuses"""
    s = gsr_hist_spec()
    _check(load_library().gsr_hist_prepare(int(channel), HIST_LOG2 if log2 else 0, float(lo), float(hi), int(bins), C.byref(s)))
    return s


def measure_request(bounds: bool = False, extent=None, moments: bool = False, ref=(0.0, 0.0, 0.0), hists=(), skip_hidden: bool = False) -> gsr_measure_request:
    """gsr_measure_request: bounds -> lo / hi; extent = k -> lo_e / hi_e (P -+ k smax) and n_extent; moments -> the nine sums about
    ref (float32, upload space); hists = up to four gsr_hist_spec (hist_spec); skip_hidden: a splat the visibility in force hides is
    not selected.  What the fields may hold is the library's to refuse."""
    r = gsr_measure_request()
    r.what = (MEASURE_BOUNDS if bounds else 0) | (MEASURE_EXTENT if extent is not None else 0) | (MEASURE_MOMENTS if moments else 0)
    r.flags = MEASURE_SKIP_HIDDEN if skip_hidden else 0
    r.ref[:] = [float(x) for x in np.asarray(ref, np.float32).reshape(3)]
    r.extent_k = float(extent) if extent is not None else 0.0
    hists = list(hists)
    r.n_hist = len(hists)
    for k, s in enumerate(hists[:MEASURE_MAX_HIST]):
        r.hist[k] = s
    return r


def _measure_hist_words(request) -> int:
    """the uint32 words the request's histograms take (bins + 3 per spec); the library refuses an n_hist out of range"""
    return sum(max(int(request.hist[k].bins), 0) + 3 for k in range(min(max(int(request.n_hist), 0), MEASURE_MAX_HIST)))


def _measure_result(request, res, words):
    """the result as the Python door returns it: the struct with .ref and .hist (one array per spec) set"""
    res.ref = np.array(list(request.ref), np.float32)
    out, at = [], 0
    for k in range(min(max(int(request.n_hist), 0), MEASURE_MAX_HIST)):
        size = max(int(request.hist[k].bins), 0) + 3
        out.append(words[at:at + size].copy())
        at += size
    res.hist = out
    return res


def measure_eval(request, P=None, alpha=None, scale=None, Cd=None, mask=None, vis=None, n=None) -> gsr_measure_result:
    """gsr_measure_eval (host only, no GPU): what gsr_measure computes, through the functions the kernels evaluate.  Arrays in read()'s
    layout: P float32 (n, 3), alpha float32 (n,) TRUE alphas, scale and Cd uint16 halves (n, 3); an array the request does not look at
    may be None (at least one array, or n, says how many splats).  mask: a boolean array over the splats or packed uint32 words
    (None: every splat); vis: the gsr_visibility (visibility_struct) that skip_hidden hides by, or None -> the result"""
    arrs = [None if a is None else np.ascontiguousarray(a, dtype=t).reshape(-1, w) for a, t, w in
            ((P, np.float32, 3), (alpha, np.float32, 1), (scale, np.uint16, 3), (Cd, np.uint16, 3))]
    sizes = {a.shape[0] for a in arrs if a is not None} | ({int(n)} if n is not None else set())
    if len(sizes) != 1:
        raise GsrError(-1, f"measure_eval: the arrays hold {sorted(sizes)} rows")
    n = sizes.pop()
    words = removal_words(mask, n)
    res = gsr_measure_result()
    hist = np.zeros(max(_measure_hist_words(request), 1), np.uint32)
    _check(load_library().gsr_measure_eval(C.byref(request), C.byref(vis) if vis is not None else None, n, _ptr(words),
                                           *[a.ctypes.data if a is not None and n else None for a in arrs], C.byref(res),
                                           hist.ctypes.data if request.n_hist > 0 else None))
    return _measure_result(request, res, hist)


def unpack_mask(words, n: int) -> np.ndarray:
    """the first n bits of packed uint32 mask words -> bool (n,): pack_mask the other way round"""
    w = np.ascontiguousarray(words, dtype="<u4").reshape(-1)
    return np.unpackbits(w.view(np.uint8), bitorder="little")[:int(n)].astype(bool)


def xform(rotate=(0.0, 0.0, 0.0, 1.0), scale: float = 1.0, translate=(0.0, 0.0, 0.0), pivot=(0.0, 0.0, 0.0), axis_angle=None) -> gsr_xform:
    """gsr_xform: p' = scale * R (p - pivot) + pivot + translate.  rotate = a quaternion (x, y, z, w), orient's order, of any length;
    axis_angle = ((ax, ay, az), degrees) instead: the quaternion of that turn about that axis (formed in double).  What the fields may
    hold is the library's to refuse (xform_prepare, transform_eval, Engine.transform)."""
    x = gsr_xform()
    if axis_angle is not None:
        axis, deg = axis_angle
        a = np.asarray(axis, dtype=np.float64).reshape(3)
        half = np.deg2rad(float(deg)) / 2.0
        rotate = tuple(a / np.linalg.norm(a) * np.sin(half)) + (np.cos(half),)
    x.rotate[:] = [float(v) for v in np.asarray(rotate, dtype=np.float32).reshape(4)]
    x.scale = float(np.float32(scale))
    x.translate[:] = [float(v) for v in np.asarray(translate, dtype=np.float32).reshape(3)]
    x.pivot[:] = [float(v) for v in np.asarray(pivot, dtype=np.float32).reshape(3)]
    return x


def xform_prepare(x: gsr_xform) -> dict:
    """gsr_xform_prepare (host only, no GPU): the float32 rule of a transform -> {A (3, 3) = s R, t (3,), s, q (4,) = the unit
    quaternion (i, j, k, r), D1 (3, 3), D2 (5, 5), D3 (7, 7): the SH band matrices}"""
    r = gsr_xform_rule()
    _check(load_library().gsr_xform_prepare(C.byref(x) if x is not None else None, C.byref(r)))
    arr = lambda field, *shape: np.array(list(field), dtype=np.float32).reshape(*shape)
    return {"A": arr(r.A, 3, 3), "t": arr(r.t, 3), "s": np.float32(r.s), "q": arr(r.q, 4), "D1": arr(r.D1, 3, 3), "D2": arr(r.D2, 5, 5), "D3": arr(r.D3, 7, 7)}


def transform_eval(x: gsr_xform, splats, mask=None):
    """gsr_transform_eval (host only, no GPU): the arrays of a Splats-like object with the transform baked into the rows the mask
    selects (a boolean array over the splats or packed uint32 words; None: every row), through the functions the kernel evaluates
    -> a new scenes.Splats; Cd and alpha are copies, the input is not written"""
    from .scenes import Splats
    a = _Arrays(splats)
    P, scale, orient = a.P.copy(), a.scale.copy(), a.orient.copy()
    sh = [None if v is None else v.copy() for v in (a.shx, a.shy, a.shz)]
    words = removal_words(mask, a.n)
    _check(load_library().gsr_transform_eval(C.byref(x) if x is not None else None, a.n, None if words is None else words.ctypes.data,
                                             _ptr(P), _ptr(scale), _ptr(orient), *[_ptr(v) for v in sh]))
    return Splats(P, a.Cd.copy(), a.alpha.copy(), scale, orient, *sh)


def grade_params(exposure: float = 0.0, gain=(1.0, 1.0, 1.0), saturation: float = 1.0, contrast: float = 1.0, pivot: float = 0.5,
                 offset=(0.0, 0.0, 0.0), alpha_gain: float = 1.0, alpha_offset: float = 0.0) -> gsr_grade_params:
    """gsr_grade_params with the neutral defaults: colour x 2^exposure x gain per channel, saturation about the Rec.709 luma,
    contrast about pivot, offset added last; opacity -> clamp(alpha_gain alpha + alpha_offset, 0, 1).  What the fields may hold is the
    library's to refuse (grade_prepare)."""
    p = gsr_grade_params()
    p.exposure, p.saturation, p.contrast, p.pivot = float(exposure), float(saturation), float(contrast), float(pivot)
    p.gain[:] = [float(v) for v in np.asarray(gain, dtype=np.float32).reshape(3)]
    p.offset[:] = [float(v) for v in np.asarray(offset, dtype=np.float32).reshape(3)]
    p.alpha_gain, p.alpha_offset = float(alpha_gain), float(alpha_offset)
    return p


def _grade_rule_struct(rule) -> gsr_grade_rule:
    """a gsr_grade_rule as it is, or the struct of a dict grade_prepare / grade_rule returned (its arrays may have been edited)"""
    if rule is None or isinstance(rule, gsr_grade_rule):
        return rule
    r = gsr_grade_rule()
    r.M[:] = [float(v) for v in np.asarray(rule["M"], dtype=np.float32).reshape(9)]
    r.b[:] = [float(v) for v in np.asarray(rule["b"], dtype=np.float32).reshape(3)]
    r.ag, r.ab, r.flags = float(rule["ag"]), float(rule["ab"]), int(rule["flags"])
    return r


def _grade_rule_dict(r: gsr_grade_rule) -> dict:
    return {"M": np.array(list(r.M), dtype=np.float32).reshape(3, 3), "b": np.array(list(r.b), dtype=np.float32),
            "ag": np.float32(r.ag), "ab": np.float32(r.ab), "flags": int(r.flags)}


def grade_prepare(params: gsr_grade_params) -> dict:
    """gsr_grade_prepare (host only, no GPU): the float32 rule of a grade -> {M (3, 3), b (3,), ag, ab, flags: GRADE_COLOUR |
    GRADE_ALPHA, which of the two steps run}; what Engine.grade and grade_eval take"""
    r = gsr_grade_rule()
    _check(load_library().gsr_grade_prepare(C.byref(params) if params is not None else None, C.byref(r)))
    return _grade_rule_dict(r)


def grade_rule(M, b=(0.0, 0.0, 0.0), alpha_gain: float = 1.0, alpha_offset: float = 0.0) -> dict:
    """the rule of a caller's own colour matrix (rows; a colour-space change, a hue rotation, a channel swap): c' = M c + b, rounded to
    float32; the colour step runs unless M is the identity and b zero, the opacity step unless (alpha_gain, alpha_offset) == (1, 0)"""
    r = gsr_grade_rule()
    r.M[:] = [float(v) for v in np.asarray(M, dtype=np.float32).reshape(9)]
    r.b[:] = [float(v) for v in np.asarray(b, dtype=np.float32).reshape(3)]
    r.ag, r.ab = float(alpha_gain), float(alpha_offset)
    identity = list(r.M) == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0] and list(r.b) == [0.0, 0.0, 0.0]
    r.flags = (0 if identity else GRADE_COLOUR) | (0 if (r.ag == 1.0 and r.ab == 0.0) else GRADE_ALPHA)
    return _grade_rule_dict(r)


def grade_eval(rule, splats, mask=None):
    """gsr_grade_eval (host only, no GPU): the arrays of a Splats-like object with the rule (grade_prepare / grade_rule, or a
    gsr_grade_rule) baked into the rows the mask selects (a boolean array over the splats or packed uint32 words; None: every row),
    through the functions the kernel evaluates -> a new scenes.Splats; P, scale and orient are copies, the input is not written"""
    from .scenes import Splats
    a = _Arrays(splats)
    Cd, alpha = a.Cd.copy(), a.alpha.copy()
    sh = [None if v is None else v.copy() for v in (a.shx, a.shy, a.shz)]
    words = removal_words(mask, a.n)
    r = _grade_rule_struct(rule)
    _check(load_library().gsr_grade_eval(C.byref(r) if r is not None else None, a.n, None if words is None else words.ctypes.data,
                                         1 if sh[0] is not None else 0, _ptr(Cd), _ptr(alpha), *[_ptr(v) for v in sh]))
    return Splats(a.P.copy(), Cd, alpha, a.scale.copy(), a.orient.copy(), *sh)


def add_capacity(cap: int, need: int) -> int:
    """gsr_add_capacity (host only, no GPU): the capacity a context of capacity cap has after an add that brings it to need splats --
    cap while need fits, else need + need // 4, clamped to 0x7fffffff"""
    cap, need = int(cap), int(need)
    if not (-2 ** 63 <= cap < 2 ** 63 and -2 ** 63 <= need < 2 ** 63):
        raise GsrError(-1, f"add_capacity: ({cap}, {need}) are not 64-bit counts")
    out = load_library().gsr_add_capacity(cap, need)
    if out < 0:
        _check(int(out))
    return int(out)


def add_arrays(splats, has_sh=None):
    """the arrays of gsr_add from a Splats-like object -> _Arrays; has_sh (None: not known here) = whether the resident cloud has SH,
    which the new rows must match"""
    for name in ("P", "Cd", "alpha", "scale", "orient"):
        if getattr(splats, name, None) is None:
            raise GsrError(-1, f"add: the new splats have no {name}")
    a = _Arrays(splats)
    if has_sh is not None and bool(has_sh) != (a.shx is not None) and a.n:
        raise GsrError(-1, "add: the new splats " + ("have no SH and the resident cloud has" if has_sh else "have SH and the resident cloud has none"))
    return a


def camera_struct(cam) -> gsr_camera:
    s = gsr_camera()
    for name in ("obj_view", "object", "inv_object", "view", "proj"):
        getattr(s, name)[:] = np.asarray(getattr(cam, name), dtype=np.float32).reshape(16).tolist()
    s.cam_pos[:] = np.asarray(cam.cam_pos, dtype=np.float32).tolist()
    s.width, s.height, s.sh_order = int(cam.width), int(cam.height), int(cam.sh_order)
    return s


UPDATE_ATTRS = (("Cd", np.uint16, 3), ("alpha", np.float32, 1), ("scale", np.uint16, 3), ("orient", np.uint16, 4),
                ("shx", np.uint16, 16), ("shy", np.uint16, 16), ("shz", np.uint16, 16))
RESIDENT_GEOA, RESIDENT_GEOB, RESIDENT_COL, RESIDENT_COLROW, RESIDENT_CLUSA, RESIDENT_CLUSB = range(6)


def attr_update_struct(**arrays):
    """gsr_attr_update from keyword arrays (Cd, alpha, scale, orient, shx, shy, shz; None = leave as is) -> (struct, n, the typed
    contiguous arrays it points into: keep them alive during the call).  n comes from the arrays; mismatched lengths raise."""
    u, keep, n = gsr_attr_update(), [], None
    for name, dtype, width in UPDATE_ATTRS:
        a = arrays.get(name)
        if a is None:
            continue
        a = np.ascontiguousarray(a, dtype=dtype)
        if a.size % width:
            raise GsrError(-1, f"update_attrs: {name} holds {a.size} values, not a multiple of {width}")
        if n is not None and a.size // width != n:
            raise GsrError(-1, f"update_attrs: {name} holds {a.size // width} splats, the arrays before it {n}")
        n = a.size // width
        keep.append(a)
        setattr(u, name, a.ctypes.data)
    return u, (n or 0), keep


def move_arrays(P, **attrs):
    """the arguments of gsr_move from P (float32, (n, 3)) and update_attrs' keyword arrays -> (P, n, gsr_attr_update, the arrays to keep
    alive during the call); the attribute arrays must hold n rows"""
    P = np.ascontiguousarray(P, dtype=np.float32)
    if P.size % 3:
        raise GsrError(-1, f"move: P holds {P.size} values, not a multiple of 3")
    n = P.size // 3
    u, nu, keep = attr_update_struct(**attrs)
    if keep and nu != n:
        raise GsrError(-1, f"move: the attribute arrays hold {nu} splats, P {n}")
    return P, n, u, keep


DEVICE_ATTRS = (("P", 3), ("Cd", 3), ("alpha", 1), ("scale", 3), ("orient", 4), ("sh", None))     # (name, float32 values per splat)


def device_attrs_struct(n=None, sh_vec3_per_point=None, **arrays):
    """gsr_device_attrs from keyword arrays in DEVICE memory (P, Cd, alpha, scale, orient, sh; None = NULL) -> (struct, n, the objects it
    points into: keep them alive during the call).  An array is an int -- a device pointer; then n must be given, and sh_vec3_per_point
    with sh -- or an object with data_ptr() (a torch tensor): float32, contiguous, on a GPU, its first axis the splats; n and
    sh_vec3_per_point come from the shapes and are cross-checked.  Nothing is copied and nothing is synchronised."""
    unknown = set(arrays) - {name for name, _ in DEVICE_ATTRS}
    if unknown:
        raise GsrError(-1, f"device_attrs_struct: unknown attribute(s) {sorted(unknown)}")
    a, keep = gsr_device_attrs(), []
    n = None if n is None else int(n)
    vpp = None if sh_vec3_per_point is None else int(sh_vec3_per_point)
    for name, width in DEVICE_ATTRS:
        v = arrays.get(name)
        if v is None:
            continue
        if isinstance(v, (int, np.integer)):
            if n is None:
                raise GsrError(-1, f"device_attrs_struct: {name} is a raw device pointer: n must be given")
            setattr(a, name, int(v))
            continue
        if not hasattr(v, "data_ptr"):
            raise GsrError(-1, f"device_attrs_struct: {name} is neither a device pointer (int) nor an object with data_ptr()")
        if not str(v.dtype).endswith("float32"):
            raise GsrError(-1, f"device_attrs_struct: {name} is {v.dtype}, not float32")
        if not v.is_contiguous():
            raise GsrError(-1, f"device_attrs_struct: {name} is not contiguous")
        if not getattr(v, "is_cuda", False):
            raise GsrError(-1, f"device_attrs_struct: {name} lives on {getattr(v, 'device', 'the host')}, not on a GPU")
        shape = tuple(int(x) for x in v.shape)
        if not shape:
            raise GsrError(-1, f"device_attrs_struct: {name} has no splat axis")
        rows, per = shape[0], int(np.prod(shape[1:], dtype=np.int64))
        if n is not None and rows != n:
            raise GsrError(-1, f"device_attrs_struct: {name} holds {rows} splats, not {n}")
        n = rows
        if width is None:                           # sh: (n, vpp, 3)
            if per % 3 or (len(shape) > 2 and shape[-1] != 3) or (vpp is not None and per != 3 * vpp):
                raise GsrError(-1, f"device_attrs_struct: sh holds {per} values per splat, not {'3 x vec3 per point' if vpp is None else 3 * vpp}")
            vpp = per // 3
        elif per != width:
            raise GsrError(-1, f"device_attrs_struct: {name} holds {per} values per splat, not {width}")
        keep.append(v)
        setattr(a, name, int(v.data_ptr()))
    if a.sh:
        if vpp is None:
            raise GsrError(-1, "device_attrs_struct: sh is a raw device pointer: sh_vec3_per_point must be given")
        a.sh_vec3_per_point = vpp
    return a, (n or 0), keep


def device_out_struct(n=None, sh_vec3_per_point=None, **arrays):
    """gsr_device_out from keyword DESTINATIONS in device memory (P, Cd, alpha, scale, orient, sh; None = not wanted) -> (struct, n, the
    objects it points into: keep them alive during the call).  Built like device_attrs_struct: an array is an int -- a device pointer;
    then n must be given, and sh_vec3_per_point with sh -- or an object with data_ptr() (a torch tensor): float32, contiguous, on a
    GPU, its first axis the rows; n and sh_vec3_per_point (1..16) come from the shapes and are cross-checked.  Nothing is written here."""
    a, n, keep = device_attrs_struct(n, sh_vec3_per_point, **arrays)       # (the same rules for what an array may be)
    out = gsr_device_out()
    for name, _ in DEVICE_ATTRS:
        setattr(out, name, getattr(a, name))
    if out.sh:
        if not 1 <= a.sh_vec3_per_point <= 16:
            raise GsrError(-1, f"device_out_struct: sh_vec3_per_point = {a.sh_vec3_per_point} is not within 1..16")
        out.sh_vec3_per_point = a.sh_vec3_per_point
    return out, n, keep


READ_ARRAYS = (("P", np.float32, 3), ("Cd", np.uint16, 3), ("alpha", np.float32, 1), ("scale", np.uint16, 3), ("orient", np.uint16, 4),
               ("shx", np.uint16, 16), ("shy", np.uint16, 16), ("shz", np.uint16, 16))     # gsr_read_arrays: (name, dtype, values per row)


def read_arrays_struct(n: int, names):
    """gsr_read_arrays for n rows of the arrays `names` -> (struct, {name: the fresh array it points into})"""
    unknown = set(names) - {name for name, _, _ in READ_ARRAYS}
    if unknown:
        raise GsrError(-1, f"read: unknown array(s) {sorted(unknown)}")
    r, arrays = gsr_read_arrays(), {}
    for name, dtype, width in READ_ARRAYS:
        if name in names:
            arrays[name] = np.zeros((n, width) if width > 1 else (n,), dtype)
            setattr(r, name, arrays[name].ctypes.data)
    return r, arrays


def _read_splats(L, verb, handle, info, first, n, names):
    """Engine.read / MultiEngine.read behind their handles: info = (resident count, has_sh)"""
    from .scenes import Splats
    total, has_sh = info
    first = int(first)
    n = total - first if n is None else int(n)
    if names is None:
        names = [name for name, _, _ in READ_ARRAYS if has_sh or not name.startswith("sh")]
    r, arrays = read_arrays_struct(max(n, 0), tuple(names))
    _check(verb(handle, first, n, C.byref(r)))
    return Splats(*[arrays.get(name) for name, _, _ in READ_ARRAYS])


class _Arrays:
    """contiguous, correctly typed views of a Splats-like object (kept alive during the call)"""

    def __init__(self, s):
        self.P = np.ascontiguousarray(s.P, dtype=np.float32).reshape(-1, 3)
        n = self.n = self.P.shape[0]
        self.Cd = np.ascontiguousarray(s.Cd, dtype=np.uint16).reshape(n, 3)
        self.alpha = np.ascontiguousarray(s.alpha, dtype=np.float32).reshape(n)
        self.scale = np.ascontiguousarray(s.scale, dtype=np.uint16).reshape(n, 3)
        self.orient = np.ascontiguousarray(s.orient, dtype=np.uint16).reshape(n, 4)
        sh = getattr(s, "shx", None) is not None
        self.shx = np.ascontiguousarray(s.shx, dtype=np.uint16).reshape(n, 16) if sh else None
        self.shy = np.ascontiguousarray(s.shy, dtype=np.uint16).reshape(n, 16) if sh else None
        self.shz = np.ascontiguousarray(s.shz, dtype=np.uint16).reshape(n, 16) if sh else None

    def ptrs(self):
        return [_ptr(a) for a in (self.P, self.Cd, self.alpha, self.scale, self.orient, self.shx, self.shy, self.shz)]


class Engine:
    """One libgsplat_hip context = one GPU.  Thin, 1:1 over the gsr_* C ABI."""

    def __init__(self, device: int = 0):
        self.L = load_library()
        h = C.c_void_p()
        _check(self.L.gsr_create(int(device), C.byref(h)))
        self.h = h
        self.device = device
        self.shard = (0, 1)
        self.target_format = TARGET_RGBA32F

    def close(self):
        if getattr(self, "h", None):
            self.L.gsr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- staging
    def upload(self, splats, origin=(0.0, 0.0, 0.0)):
        a = _Arrays(splats)
        _check(self.L.gsr_upload(self.h, a.n, *a.ptrs(), _f3(origin)))
        return a.n

    def upload_parts(self, parts, origin=(0.0, 0.0, 0.0)):
        arrs = [_Arrays(p) for p in parts]
        has_sh = bool(arrs) and all(a.shx is not None for a in arrs)
        _check(self.L.gsr_upload_begin(self.h, sum(a.n for a in arrs), int(has_sh), _f3(origin)))
        for a in arrs:
            p = a.ptrs()
            if not has_sh:
                p[5:] = [None, None, None]
            _check(self.L.gsr_upload_append(self.h, a.n, *p))
        _check(self.L.gsr_upload_end(self.h))

    def upload_raw(self, attrs: dict, origin=(0.0, 0.0, 0.0)):
        """raw float32 point attributes (dict keyed like a Houdini detail: P, Cd, opacity / Alpha resolved by the caller into
        'alpha', scale, orient, and ONE of sh_coefficients / sh1..sh15 / f_rest_0..44): quantised and packed on the GPU"""
        f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
        keep = {k: f32(v) for k, v in attrs.items()}
        n = int(keep["P"].reshape(-1, 3).shape[0])
        a = gsr_raw_attrs()
        for name in ("P", "Cd", "alpha", "scale", "orient"):
            setattr(a, name, keep[name].ctypes.data if name in keep else None)
        ptrs = None
        if "sh_coefficients" in keep:
            a.sh_scheme, a.sh_array = 1, keep["sh_coefficients"].ctypes.data
            a.sh_vec3_per_point = int(keep["sh_coefficients"].size // max(n, 1) // 3)
        elif "sh1" in keep:
            ptrs = (C.c_void_p * 15)(*[keep[f"sh{k + 1}"].ctypes.data if f"sh{k + 1}" in keep else None for k in range(15)])
            a.sh_scheme, a.sh_ptr = 2, ptrs
        elif "f_rest_0" in keep:
            ptrs = (C.c_void_p * 45)(*[keep[f"f_rest_{k}"].ctypes.data if f"f_rest_{k}" in keep else None for k in range(45)])
            a.sh_scheme, a.sh_ptr = 3, ptrs
        _check(self.L.gsr_upload_begin(self.h, n, int(a.sh_scheme != 0), _f3(origin)))
        try:
            _check(self.L.gsr_upload_append_raw(self.h, n, C.byref(a)))
            _check(self.L.gsr_upload_end(self.h))
        except GsrError:
            self.L.gsr_upload_abort(self.h)
            raise
        return n

    def update_attrs(self, first: int, Cd=None, alpha=None, scale=None, orient=None, shx=None, shy=None, shz=None) -> int:
        """gsr_update: new attribute values for the resident splats [first, first + n) (upload order) written in place, no re-upload;
        arrays in the registerUpdate() layout (halves as uint16 bits), None = leave as is, n from the arrays.  No P: that is an upload."""
        u, n, keep = attr_update_struct(Cd=Cd, alpha=alpha, scale=scale, orient=orient, shx=shx, shy=shy, shz=shz)
        _check(self.L.gsr_update(self.h, int(first), n, C.byref(u)))
        return n

    def move(self, first: int, P, origin=None, **attrs) -> int:
        """gsr_move: new positions P (float32, (n, 3)) for the resident splats [first, first + n) (upload order), re-ordered on the GPU
        with no re-upload; origin = the new GSplatOrigin (None: it stays); attrs = update_attrs' arrays for the same rows, applied in
        the same call.  The context keeps a second copy of the resident planes from the first move on (include/gsplat_hip.h)."""
        P, n, u, keep = move_arrays(P, **attrs)
        _check(self.L.gsr_move(self.h, int(first), n, P.ctypes.data, None if origin is None else _f3(origin), C.byref(u)))
        return n

    # ---- device sources: float32 arrays that already sit in device memory (device_attrs_struct says what an array may be)
    def upload_device(self, attrs: dict, origin=(0.0, 0.0, 0.0), n=None, sh_vec3_per_point=None):
        """gsr_upload_append_device as a whole upload: attrs = {P, and optionally Cd, alpha, scale, orient, sh}, quantised and packed on
        the GPU with nothing crossing the link; missing arrays take upload_raw's defaults, and the cloud has SH exactly when sh is given"""
        a, n, keep = device_attrs_struct(n, sh_vec3_per_point, **attrs)
        _check(self.L.gsr_upload_begin(self.h, n, int(bool(a.sh)), _f3(origin)))
        try:
            _check(self.L.gsr_upload_append_device(self.h, n, C.byref(a)))
            _check(self.L.gsr_upload_end(self.h))
        except GsrError:
            self.L.gsr_upload_abort(self.h)
            raise
        return n

    def update_attrs_device(self, first: int, n=None, sh_vec3_per_point=None, **attrs) -> int:
        """gsr_update_device: update_attrs from float32 arrays in device memory (Cd, alpha, scale, orient, sh; no P), quantised on the GPU.
        Waits for the work queued on the stream given to set_stream, then for the frames in flight; synchronous."""
        a, n, keep = device_attrs_struct(n, sh_vec3_per_point, **attrs)
        _check(self.L.gsr_update_device(self.h, int(first), n, C.byref(a)))
        return n

    def move_device(self, first: int, P, origin=None, n=None, sh_vec3_per_point=None, **attrs) -> int:
        """gsr_move_device: move from a float32 P (n, 3) in device memory, with update_attrs_device's arrays for the same rows"""
        a, n, keep = device_attrs_struct(n, sh_vec3_per_point, P=P, **attrs)
        _check(self.L.gsr_move_device(self.h, int(first), n, None if origin is None else _f3(origin), C.byref(a)))
        return n

    def check_device_source(self, ptr: int, nbytes: int) -> bool:
        """gsr_debug_check_device_source: would the device-source verbs take [ptr, ptr + nbytes) as a source array?  A pure query."""
        rc = self.L.gsr_debug_check_device_source(self.h, C.c_void_p(int(ptr)), int(nbytes))
        if rc not in (0, -1):
            _check(rc)
        return rc == 0

    def set_visibility(self, vis=None, volumes=None, mask=None):
        """gsr_set_visibility: hide the resident splats that fail the volumes or whose mask entry is True, with no re-upload.  Either a
        gsr_visibility (its mask words must stay alive during the call), or volumes / mask as visibility_struct takes them; nothing
        given = everything visible again.  Volumes persist across updates, moves and uploads; the mask is dropped by an upload."""
        keep = None
        if vis is None and (volumes is not None or mask is not None):
            vis, keep = visibility_struct(volumes or (), mask)
        _check(self.L.gsr_set_visibility(self.h, C.byref(vis) if vis is not None else None))

    def get_visibility(self):
        """gsr_get_visibility -> (the gsr_visibility in force, mask pointer always NULL; how many splats the last application hid)"""
        v, hidden = gsr_visibility(), C.c_int64(0)
        _check(self.L.gsr_get_visibility(self.h, C.byref(v), C.byref(hidden)))
        return v, hidden.value

    def remove(self, mask=None, hidden: bool = False) -> int:
        """gsr_remove: the resident splats whose mask entry is True (a boolean array over the resident splats in upload order, or the
        packed uint32 words) leave the cloud, compacted and re-ordered on the GPU with no re-upload; hidden = also everything the
        visibility in force hides (mask may then be None).  The survivors keep their relative upload order (remove_map) -> the splats
        left.  The context keeps a second copy of the resident planes from the first removal on (include/gsplat_hip.h)."""
        words = removal_words(mask, self.stats()["n_splats"])
        left = C.c_int64(0)
        _check(self.L.gsr_remove(self.h, None if words is None else words.ctypes.data, 0, REMOVE_HIDDEN if hidden else 0, C.byref(left)))
        return left.value

    def remove_device(self, mask, hidden: bool = False) -> int:
        """gsr_remove from packed uint32 mask words in DEVICE memory: an int (a device pointer) or an object with data_ptr() (a torch
        tensor of 32-bit integers, contiguous, on the context's GPU), ceil(n / 32) words.  Waits for the work queued on the stream
        given to set_stream first -> the splats left"""
        if isinstance(mask, (int, np.integer)):
            ptr = int(mask)
        elif hasattr(mask, "data_ptr"):
            if not str(mask.dtype).endswith(("int32", "uint32")):
                raise GsrError(-1, f"remove_device: the mask is {mask.dtype}, not packed 32-bit words")
            if not mask.is_contiguous() or not getattr(mask, "is_cuda", False):
                raise GsrError(-1, "remove_device: the mask is not a contiguous tensor on a GPU")
            ptr = int(mask.data_ptr())
        else:
            raise GsrError(-1, "remove_device: the mask is neither a device pointer (int) nor an object with data_ptr()")
        left = C.c_int64(0)
        _check(self.L.gsr_remove(self.h, C.c_void_p(ptr), 1, REMOVE_HIDDEN if hidden else 0, C.byref(left)))
        return left.value

    # ---- transform: selected resident splats rotated, scaled, translated (include/gsplat_hip.h, "transform")
    def transform(self, x: gsr_xform, mask=None) -> int:
        """gsr_transform from a HOST mask: the transform (xform) is baked into the resident splats whose mask entry is True (a boolean
        array over the resident splats in upload order, or the packed uint32 words; None: every splat) -- positions, scales, orients
        and SH rows -- and the cloud is re-ordered on the GPU with no re-upload, bit for bit a fresh upload of transform_eval of what
        read returns -> the splats moved"""
        words = removal_words(mask, self.stats()["n_splats"])
        moved = C.c_int64(0)
        _check(self.L.gsr_transform(self.h, None if words is None else words.ctypes.data, 0, C.byref(x) if x is not None else None, C.byref(moved)))
        return moved.value

    def transform_device(self, x: gsr_xform, mask_ptr) -> int:
        """gsr_transform from packed uint32 mask words in DEVICE (or pinned) memory: a raw pointer or an object with data_ptr(),
        ceil(n / 32) words, as select_device writes them; never written.  Waits for the work queued on the stream given to set_stream
        first -> the splats moved"""
        ptr = int(mask_ptr.data_ptr()) if hasattr(mask_ptr, "data_ptr") else int(mask_ptr)
        moved = C.c_int64(0)
        _check(self.L.gsr_transform(self.h, C.c_void_p(ptr), 1, C.byref(x) if x is not None else None, C.byref(moved)))
        return moved.value

    def get_transform(self) -> dict:
        """gsr_get_transform -> {transforms: the calls, moved_last, ms: the last call's stage clock [mask copy, kernel .. sort,
        repack, wall]}"""
        return self._tally(self.L.gsr_get_transform, "transforms", "moved_last")

    # ---- grade: the colour and the opacity of selected resident splats (include/gsplat_hip.h, "grade")
    def grade(self, rule, mask=None) -> int:
        """gsr_grade from a HOST mask: the rule (grade_prepare / grade_rule, or a gsr_grade_rule) is baked into the Cd, the SH rows and
        the opacity of the resident splats whose mask entry is True (a boolean array over the resident splats in upload order, or the
        packed uint32 words; None: every splat), in place on the GPU, bit for bit a fresh upload of grade_eval of what read returns
        -> the splats graded"""
        words = removal_words(mask, self.stats()["n_splats"])
        r = _grade_rule_struct(rule)
        graded = C.c_int64(0)
        _check(self.L.gsr_grade(self.h, None if words is None else words.ctypes.data, 0, C.byref(r) if r is not None else None, C.byref(graded)))
        return graded.value

    def grade_device(self, rule, mask_ptr) -> int:
        """gsr_grade from packed uint32 mask words in DEVICE (or pinned) memory: a raw pointer or an object with data_ptr(),
        ceil(n / 32) words, as select_device writes them; never written.  Waits for the work queued on the stream given to set_stream
        first -> the splats graded"""
        ptr = int(mask_ptr.data_ptr()) if hasattr(mask_ptr, "data_ptr") else int(mask_ptr)
        r = _grade_rule_struct(rule)
        graded = C.c_int64(0)
        _check(self.L.gsr_grade(self.h, C.c_void_p(ptr), 1, C.byref(r) if r is not None else None, C.byref(graded)))
        return graded.value

    def get_grade(self) -> dict:
        """gsr_get_grade -> {grades: the calls, graded_last, ms: the stage clock of the last call that wrote [mask copy and count,
        kernel, visibility, wall]}"""
        return self._tally(self.L.gsr_get_grade, "grades", "graded_last")

    def get_removal(self) -> dict:
        """gsr_get_removal -> {removals: calls that removed something, removed_last, ms: the last call's stage clock
        [mask copy, mark .. sort, repack, wall]}"""
        return self._tally(self.L.gsr_get_removal, "removals", "removed_last")

    def add(self, splats) -> int:
        """gsr_add: the splats (a Splats-like object, arrays in upload's layout) join the resident cloud behind its last upload index,
        ordered and packed on the GPU with no re-upload; with SH exactly when the resident cloud has SH -> the splats resident now.
        An add that does not fit grows the context (add_capacity; include/gsplat_hip.h)."""
        a = add_arrays(splats)
        total = C.c_int64(0)
        _check(self.L.gsr_add(self.h, a.n, *a.ptrs(), C.byref(total)))
        return total.value

    def add_device(self, attrs: dict, n=None, sh_vec3_per_point=None) -> int:
        """gsr_add_device: add from float32 arrays in device memory, attrs = {P, and optionally Cd, alpha, scale, orient, sh} as
        upload_device takes them; sh exactly when the resident cloud has SH -> the splats resident now"""
        if not isinstance(attrs, dict):
            raise GsrError(-1, "add_device: attrs is not a dict of device arrays")
        if attrs.get("P") is None:
            raise GsrError(-1, "add_device: P is missing")
        a, n, keep = device_attrs_struct(n, sh_vec3_per_point, **attrs)
        total = C.c_int64(0)
        _check(self.L.gsr_add_device(self.h, n, C.byref(a), C.byref(total)))
        return total.value

    def get_add(self) -> dict:
        """gsr_get_add -> {adds: calls that added something, added_last, capacity: splats the context has room for, grows: adds that
        grew it, ms: the last call's stage clock [new rows over the link, positions .. sort, pack, wall]}"""
        return self._tally(self.L.gsr_get_add, "adds", "added_last", "capacity", "grows")

    # ---- reading back: the resident cloud in upload order (include/gsplat_hip.h, "reading back")
    def read_info(self) -> dict:
        """gsr_read_info -> {n_splats: resident now, has_sh, origin: the GSplatOrigin in force}; no kernel, no synchronisation"""
        n, sh, origin = C.c_int64(0), C.c_int(0), (C.c_float * 3)()
        _check(self.L.gsr_read_info(self.h, C.byref(n), C.byref(sh), origin))
        return {"n_splats": n.value, "has_sh": bool(sh.value), "origin": tuple(float(x) for x in origin)}

    def read(self, first: int = 0, n=None, names=None):
        """gsr_read: the attributes of the resident splats [first, first + n) (upload order; n = None: to the end) as a scenes.Splats
        in upload's layout, bit for bit what a fresh upload would have to be given: raw P bits, TRUE alphas also under a visibility,
        the resident halves.  names = the arrays wanted (the others are None); default: all, SH only when the cloud has it.  Changes
        and invalidates nothing."""
        info = self.read_info()
        return _read_splats(self.L, self.L.gsr_read, self.h, (info["n_splats"], info["has_sh"]), first, n, names)

    def read_device(self, dst: dict, first: int = 0, n=None, sh_vec3_per_point=None) -> int:
        """gsr_read_device: the same rows into float32 arrays in DEVICE memory, dst = {P, Cd, alpha, scale, orient, sh} (any subset) of
        raw device pointers (then n must be given, and sh_vec3_per_point with sh) or torch tensors (device_out_struct); every half
        arrives as the float32 of exactly that value; SH slots >= sh_vec3_per_point are not written out.  Waits for the work queued on
        the stream given to set_stream first; synchronous -> the rows read"""
        if not isinstance(dst, dict):
            raise GsrError(-1, "read_device: dst is not a dict of device arrays")
        out, n, keep = device_out_struct(n, sh_vec3_per_point, **dst)
        _check(self.L.gsr_read_device(self.h, int(first), n, C.byref(out)))
        return n

    # ---- copying: the selection read out, or duplicated (include/gsplat_hip.h, "copying")
    def read_masked(self, mask, names=None):
        """gsr_read_masked from a HOST mask (a boolean array over the resident splats in upload order, or the packed uint32 words;
        None: every splat): read's rows for the selected splats, in ascending upload order (copy_map), as a scenes.Splats of m rows.
        Changes and invalidates nothing."""
        info = self.read_info()
        verb = lambda ptr, max_rows, r, m: self.L.gsr_read_masked(self.h, ptr, 0, max_rows, r, m)     # noqa: E731
        return _read_masked_splats(verb, (info["n_splats"], info["has_sh"]), mask, names)

    def read_masked_device(self, dst: dict, mask, max_rows=None, sh_vec3_per_point=None, mask_is_device: bool = True) -> int:
        """gsr_read_masked_device: the same rows into float32 arrays in DEVICE memory, dst as read_device takes it, each array holding
        max_rows rows (from the tensors' shapes when None); mask = packed uint32 words in device (or pinned) memory -- a raw pointer or
        an object with data_ptr(), as select_device writes them -- or, with mask_is_device = False, a host mask as read_masked takes it;
        None: every splat.  A selection of more than max_rows rows raises (GSR_E_INVALID) and writes nothing; an empty dst is a count
        -> the rows of the selection"""
        if not isinstance(dst, dict):
            raise GsrError(-1, "read_masked_device: dst is not a dict of device arrays")
        keep_words = None
        if mask is None:
            ptr, dev = None, 0
        elif mask_is_device:
            ptr, dev = C.c_void_p(_device_mask_ptr(mask, "read_masked_device")), 1
        else:
            keep_words = removal_words(mask, self.read_info()["n_splats"])
            ptr, dev = keep_words.ctypes.data, 0
        m = C.c_int64(0)
        if not any(v is not None for v in dst.values()):
            _check(self.L.gsr_read_masked_device(self.h, ptr, dev, 0, None, C.byref(m)))
            return m.value
        out, max_rows, keep = device_out_struct(max_rows, sh_vec3_per_point, **dst)
        _check(self.L.gsr_read_masked_device(self.h, ptr, dev, max_rows, C.byref(out), C.byref(m)))
        return m.value

    def duplicate(self, mask=None):
        """gsr_duplicate from a HOST mask (a boolean array over the resident splats in upload order, or the packed uint32 words; None:
        every splat): a copy of each selected splat joins the cloud behind its last upload index, in the ascending upload order of the
        originals, on the GPU with no re-upload -- bit for bit a fresh upload of concat(read(), read()[copy_map]) -> (m: the copies,
        n_total: the splats resident now).  range_mask(n_total - m, m, n_total) selects the copies."""
        words = removal_words(mask, self.stats()["n_splats"])
        m, total = C.c_int64(0), C.c_int64(0)
        _check(self.L.gsr_duplicate(self.h, None if words is None else words.ctypes.data, 0, C.byref(m), C.byref(total)))
        return m.value, total.value

    def duplicate_device(self, mask_ptr):
        """gsr_duplicate from packed uint32 mask words in DEVICE (or pinned) memory: a raw pointer or an object with data_ptr(),
        ceil(n / 32) words, as select_device writes them; never written.  Waits for the work queued on the stream given to set_stream
        first -> (m, n_total)"""
        ptr = _device_mask_ptr(mask_ptr, "duplicate_device")
        m, total = C.c_int64(0), C.c_int64(0)
        _check(self.L.gsr_duplicate(self.h, C.c_void_p(ptr), 1, C.byref(m), C.byref(total)))
        return m.value, total.value

    def debug_stage_bytes(self) -> int:
        """gsr_debug_stage_bytes: the bytes the context's staging arena answers for right now"""
        return int(self.L.gsr_debug_stage_bytes(self.h))

    def get_duplicate(self) -> dict:
        """gsr_get_duplicate -> {duplicates: calls that copied something, copied_last, ms: the last call's stage clock [mask copy,
        mark .. sort, repack, wall]}"""
        return self._tally(self.L.gsr_get_duplicate, "duplicates", "copied_last")

    def get_read(self) -> dict:
        """gsr_get_read -> {reads: calls that read something, rows_last, ms: the last call's clock [kernel, device -> host copies, 0, wall]}"""
        return self._tally(self.L.gsr_get_read, "reads", "rows_last")

    # ---- selection: resident splats by screen region (include/gsplat_hip.h, "selection")
    def select(self, cam, region, mask=None):
        """gsr_select into a HOST mask: the resident splats whose centre projects into the region (a gsr_select_region, or the
        (struct, keep) pair select_region returns) -> (bool (n,) mask in upload order, n_hit, n_set).  mask = the prior selection the
        region's op combines with (a boolean array over the resident splats or packed uint32 words; None: nothing selected).  The
        result feeds set_visibility(mask=...) and remove(...) as it is.  Changes and invalidates nothing."""
        r, keep = region if isinstance(region, tuple) else (region, [])
        _region_fits(cam, keep, "select")
        n = self.read_info()["n_splats"]
        words = removal_words(np.zeros(n, bool) if mask is None else mask, n).copy()
        hit, nset = C.c_int64(0), C.c_int64(0)
        cs = cam if isinstance(cam, gsr_camera) else camera_struct(cam)
        _check(self.L.gsr_select(self.h, C.byref(cs), C.byref(r), words.ctypes.data, 0, C.byref(hit), C.byref(nset)))
        return unpack_mask(words, n), hit.value, nset.value

    def select_device(self, cam, region, mask_ptr: int):
        """gsr_select into packed uint32 mask words in DEVICE memory (a raw pointer or an object with data_ptr(); ceil(n / 32) words,
        read first by every op but SELECT_REPLACE); the region's image / depth may be device pointers too (select_region's
        image_device / depth_device).  Waits for the work queued on the stream given to set_stream first; synchronous
        -> (n_hit, n_set).  The mask goes straight into remove_device."""
        r, keep = region if isinstance(region, tuple) else (region, [])
        _region_fits(cam, keep, "select_device")
        ptr = int(mask_ptr.data_ptr()) if hasattr(mask_ptr, "data_ptr") else int(mask_ptr)
        hit, nset = C.c_int64(0), C.c_int64(0)
        cs = cam if isinstance(cam, gsr_camera) else camera_struct(cam)
        _check(self.L.gsr_select(self.h, C.byref(cs), C.byref(r), C.c_void_p(ptr), 1, C.byref(hit), C.byref(nset)))
        return hit.value, nset.value

    def get_select(self) -> dict:
        """gsr_get_select -> {selects: calls that selected, hit_last, ms: the last call's clock [kernel, copies, 0, wall]}"""
        return self._tally(self.L.gsr_get_select, "selects", "hit_last")

    # ---- selection by attribute (include/gsplat_hip.h, "selection by attribute")
    def select_attrs(self, rule: gsr_attr_rule, mask=None):
        """gsr_select_attrs into a HOST mask: the resident splats the rule (attr_rule) hits -> (bool (n,) mask in upload order, n_hit,
        n_set).  mask = the prior selection the rule's op combines with (a boolean array over the resident splats or packed uint32 words;
        None: nothing selected).  Changes and invalidates nothing."""
        n = self.read_info()["n_splats"]
        words = removal_words(np.zeros(n, bool) if mask is None else mask, n).copy()
        hit, nset = C.c_int64(0), C.c_int64(0)
        _check(self.L.gsr_select_attrs(self.h, C.byref(rule), words.ctypes.data, 0, C.byref(hit), C.byref(nset)))
        return unpack_mask(words, n), hit.value, nset.value

    def select_attrs_device(self, rule: gsr_attr_rule, mask_ptr):
        """gsr_select_attrs into packed uint32 mask words in DEVICE memory (a raw pointer or an object with data_ptr(); ceil(n / 32)
        words, read first by every op but SELECT_REPLACE).  Waits for the work queued on the stream given to set_stream first;
        synchronous -> (n_hit, n_set).  The mask goes straight into remove_device (a prune: nothing crosses the link)."""
        ptr = _device_mask_ptr(mask_ptr, "select_attrs_device")
        hit, nset = C.c_int64(0), C.c_int64(0)
        _check(self.L.gsr_select_attrs(self.h, C.byref(rule), C.c_void_p(ptr), 1, C.byref(hit), C.byref(nset)))
        return hit.value, nset.value

    def get_select_attrs(self) -> dict:
        """gsr_get_select_attrs -> {selects: calls that selected, hit_last, ms: the last call's clock [kernel, copies, 0, wall]}"""
        return self._tally(self.L.gsr_get_select_attrs, "selects", "hit_last")

    # ---- selection by density (include/gsplat_hip.h, "selection by density")
    def select_density(self, rule: gsr_density_rule, mask=None, counts: bool = False):
        """gsr_select_density into a HOST mask: the resident splats whose neighbour count the rule (density_rule) hits -> (bool (n,)
        mask in upload order, n_hit, n_set, the gsr_density_result[, the uint32 (n,) neighbour counts]).  mask = the prior selection the
        rule's op combines with (a boolean array over the resident splats or packed uint32 words; None: nothing selected).  Waits for the
        frames in flight; changes and invalidates nothing."""
        n = self.read_info()["n_splats"]
        words = removal_words(np.zeros(n, bool) if mask is None else mask, n).copy()
        cnt = np.zeros(max(n, 1), np.uint32)
        hit, nset, res = C.c_int64(0), C.c_int64(0), gsr_density_result()
        _check(self.L.gsr_select_density(self.h, C.byref(rule), words.ctypes.data, 0, cnt.ctypes.data if counts else None, 0, C.byref(res),
                                         C.byref(hit), C.byref(nset)))
        return (unpack_mask(words, n), hit.value, nset.value, res) + ((cnt[:n],) if counts else ())

    def select_density_device(self, rule: gsr_density_rule, mask_ptr, counts_ptr=None):
        """gsr_select_density into packed uint32 mask words in DEVICE memory (a raw pointer or an object with data_ptr(); ceil(n / 32)
        words, read first by every op but SELECT_REPLACE) and, with counts_ptr, n uint32 neighbour counts in device memory.  Waits for
        the frames in flight and the work queued on the stream given to set_stream first; synchronous -> (n_hit, n_set, the
        gsr_density_result).  The mask goes straight into remove_device: the floaters go and nothing crosses the link."""
        ptr = _device_mask_ptr(mask_ptr, "select_density_device")
        cptr = None if counts_ptr is None else C.c_void_p(_device_mask_ptr(counts_ptr, "select_density_device"))
        hit, nset, res = C.c_int64(0), C.c_int64(0), gsr_density_result()
        _check(self.L.gsr_select_density(self.h, C.byref(rule), C.c_void_p(ptr), 1, cptr, 1, C.byref(res), C.byref(hit), C.byref(nset)))
        return hit.value, nset.value, res

    def get_select_density(self) -> dict:
        """gsr_get_select_density -> {selects: calls that selected, hit_last, ms: the last call's clock [the verb's kernels, copies,
        the sort, wall]}"""
        return self._tally(self.L.gsr_get_select_density, "selects", "hit_last")

    # ---- selection by connectivity (include/gsplat_hip.h, "selection by connectivity")
    def select_connected(self, rule: gsr_connect_rule, mask=None, seed=None, outputs: bool = False):
        """gsr_select_connected into a HOST mask: the resident splats whose connected component the rule (connect_rule) hits -> (bool
        (n,) mask in upload order, n_hit, n_set, the gsr_connect_result[, the uint32 (n,) labels, the uint32 (n,) sizes]).  mask = the
        prior selection the rule's op combines with, seed = the selection a component must touch (each a boolean array over the resident
        splats or packed uint32 words; None: nothing selected / no seed clause).  Waits for the frames in flight; changes and invalidates
        nothing."""
        n = self.read_info()["n_splats"]
        words = removal_words(np.zeros(n, bool) if mask is None else mask, n).copy()
        sw = None if seed is None else removal_words(seed, n).copy()
        lab, siz = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
        hit, nset, res = C.c_int64(0), C.c_int64(0), gsr_connect_result()
        _check(self.L.gsr_select_connected(self.h, C.byref(rule), sw.ctypes.data if sw is not None and n else None, 0, words.ctypes.data, 0,
                                           lab.ctypes.data if outputs else None, siz.ctypes.data if outputs else None, 0, C.byref(res),
                                           C.byref(hit), C.byref(nset)))
        return (unpack_mask(words, n), hit.value, nset.value, res) + ((lab[:n], siz[:n]) if outputs else ())

    def select_connected_device(self, rule: gsr_connect_rule, mask_ptr, seed_ptr=None, labels_ptr=None, sizes_ptr=None):
        """gsr_select_connected into packed uint32 mask words in DEVICE memory (a raw pointer or an object with data_ptr(); ceil(n / 32)
        words, read first by every op but SELECT_REPLACE); seed_ptr: the seed words in device memory (None: no seed clause; it may be
        mask_ptr: SELECT_ADD then grows the selection in place); labels_ptr / sizes_ptr: n uint32 each in device memory.  Waits for
        the frames in flight and the work queued on the stream given to set_stream first; synchronous -> (n_hit, n_set, the
        gsr_connect_result).  The mask goes straight into remove_device, transform, grade or duplicate: nothing crosses the link."""
        who = "select_connected_device"
        ptr = _device_mask_ptr(mask_ptr, who)
        opt = lambda p: None if p is None else C.c_void_p(_device_mask_ptr(p, who))
        hit, nset, res = C.c_int64(0), C.c_int64(0), gsr_connect_result()
        _check(self.L.gsr_select_connected(self.h, C.byref(rule), opt(seed_ptr), 1, C.c_void_p(ptr), 1, opt(labels_ptr), opt(sizes_ptr), 1,
                                           C.byref(res), C.byref(hit), C.byref(nset)))
        return hit.value, nset.value, res

    def get_select_connected(self) -> dict:
        """gsr_get_select_connected -> {selects: calls that selected, hit_last, ms: the last call's clock [the verb's kernels, copies,
        the sort, wall]}"""
        return self._tally(self.L.gsr_get_select_connected, "selects", "hit_last")

    def select_connected_stages(self) -> list:
        """gsr_debug_select_connected_stages -> the last call's kernels, ms: [keys, sort, cell table, link, flatten + stats, scatter + hit]"""
        ms = (C.c_double * 6)()
        _check(self.L.gsr_debug_select_connected_stages(self.h, ms))
        return list(ms)

    # ---- measuring a selection (include/gsplat_hip.h, "measuring a selection")
    def measure(self, request: gsr_measure_request, mask=None) -> gsr_measure_result:
        """gsr_measure from a HOST mask (a boolean array over the resident splats or packed uint32 words; None: every splat): counts,
        bounds, extent, moments and histograms of the selected splats as `request` (measure_request) asks -> the result, with
        .centroid(), .covariance() and .hist.  Changes and invalidates nothing."""
        n = self.read_info()["n_splats"]
        words = removal_words(mask, n)
        return self._measure(request, _ptr(words), 0)

    def measure_device(self, request: gsr_measure_request, mask_ptr) -> gsr_measure_result:
        """gsr_measure from packed uint32 mask words in DEVICE (or pinned) memory (a raw pointer or an object with data_ptr(); ceil(n /
        32) words, as select_device writes them; never written).  Waits for the work queued on the stream given to set_stream first;
        synchronous -> the result.  Only the result crosses the link."""
        return self._measure(request, C.c_void_p(_device_mask_ptr(mask_ptr, "measure_device")), 1)

    def _measure(self, request, mask_arg, is_device):
        res = gsr_measure_result()
        hist = np.zeros(max(_measure_hist_words(request), 1), np.uint32)
        _check(self.L.gsr_measure(self.h, mask_arg, is_device, C.byref(request), C.byref(res), hist.ctypes.data if request.n_hist > 0 else None))
        return _measure_result(request, res, hist)

    def get_measure(self) -> dict:
        """gsr_get_measure -> {measures: calls that measured, measured_last, ms: the last call's clock [k_measure, the launches that
        finish the sums, copies, wall]}"""
        return self._tally(self.L.gsr_get_measure, "measures", "measured_last")

    # ---- selection overlay (include/gsplat_hip.h, "selection overlay")
    def render_marks(self, cam, mask, style, under: np.ndarray):
        """gsr_render_marks over a HOST frame: the splats `mask` selects (a boolean array over the resident splats or packed uint32
        words; None: every splat) drawn on top of `under` (a finished frame [H, W, 4] in the target format) as `style` (a
        gsr_mark_style, or the (struct, keep) pair mark_style returns) says -> (the combined image, the pixels written).  Changes and
        invalidates nothing."""
        st, keep = style if isinstance(style, tuple) else (style, [])
        _region_fits(cam, keep, "render_marks")
        n = self.read_info()["n_splats"]
        words = None if mask is None else removal_words(mask, n)
        out = np.ascontiguousarray(under, dtype=target_dtype(self.target_format)).reshape(cam.height, cam.width, 4).copy()
        cs = cam if isinstance(cam, gsr_camera) else camera_struct(cam)
        wrote = C.c_int64(0)
        _check(self.L.gsr_render_marks(self.h, C.byref(cs), None if words is None else words.ctypes.data, 0, C.byref(st), out.ctypes.data, 0, C.byref(wrote)))
        return out, wrote.value

    def render_marks_device(self, cam, mask_ptr, style, ptr: int) -> int:
        """gsr_render_marks with the mask words and the frame in DEVICE memory (raw pointers or objects with data_ptr(); mask_ptr None:
        every splat); the style's depth buffer may be a device pointer too (mark_style's depth_device).  Waits for the frames in flight
        and the work queued on the stream given to set_stream first; synchronous -> the pixels written.  Nothing crosses the link."""
        st, keep = style if isinstance(style, tuple) else (style, [])
        _region_fits(cam, keep, "render_marks_device")
        mptr = None if mask_ptr is None else C.c_void_p(_device_mask_ptr(mask_ptr, "render_marks_device"))
        cs = cam if isinstance(cam, gsr_camera) else camera_struct(cam)
        wrote = C.c_int64(0)
        _check(self.L.gsr_render_marks(self.h, C.byref(cs), mptr, 1, C.byref(st), C.c_void_p(_device_mask_ptr(ptr, "render_marks_device")), 1, C.byref(wrote)))
        return wrote.value

    def get_marks(self) -> dict:
        """gsr_get_marks -> {calls: calls that drew, pixels_last, ms: the last call's clock [clear + k_mark, k_mark_resolve, copies, wall]}"""
        return self._tally(self.L.gsr_get_marks, "calls", "pixels_last")

    def _tally(self, get, *keys) -> dict:
        """a gsr_get_* of the resident-edit family: its int64 outputs (the calls, the last count, and what else the verb reports) under
        `keys`, in their order, then "ms": the last call's clock"""
        v, ms = [C.c_int64(0) for _ in keys], (C.c_double * 4)()
        _check(get(self.h, *[C.byref(x) for x in v], ms))
        return {**{k: x.value for k, x in zip(keys, v)}, "ms": [float(x) for x in ms]}

    def debug_resident(self, which: int) -> np.ndarray:
        """gsr_debug_read_resident: the bytes of one plane of the resident geometry (RESIDENT_*), in storage order"""
        size = self.L.gsr_debug_read_resident(self.h, int(which), None, 0)
        if size < 0:
            _check(size)
        out = np.zeros(size, np.uint8)
        rc = self.L.gsr_debug_read_resident(self.h, int(which), out.ctypes.data, size)
        if rc < 0:
            _check(rc)
        return out

    # ---- configuration
    def set_stream(self, hip_stream: int | None):
        _check(self.L.gsr_set_stream(self.h, C.c_void_p(hip_stream or 0)))

    def set_option(self, option: int, value: int):
        _check(self.L.gsr_set_option(self.h, option, value))

    def set_target_format(self, fmt: int):
        """what a pixel of every target is from the next frame on (TARGET_*): the host-returning render* methods return arrays of
        target_dtype(fmt); the device-pointer methods write pixels of gsr_target_pixel_bytes(fmt) bytes"""
        _check(self.L.gsr_set_target_format(self.h, int(fmt)))
        self.target_format = int(fmt)

    def set_row_shard(self, index: int, count: int):
        _check(self.L.gsr_set_row_shard(self.h, index, count))
        self.shard = (index, count)
        self.band = None

    def set_row_band(self, first_tile_row: int, tile_rows: int):
        """gsr_set_row_band: render only the tile rows [first_tile_row, first_tile_row + tile_rows); the render* methods then return
        the band image, tile_rows * 16 pixel rows (row 0 = the bottom pixel row of tile row first_tile_row)"""
        _check(self.L.gsr_set_row_band(self.h, int(first_tile_row), int(tile_rows)))
        self.shard = (0, 1)
        self.band = (int(first_tile_row), int(tile_rows))

    def band_rows(self, height: int) -> int:
        if getattr(self, "band", None) is not None:
            return self.band[1] * TILE
        return height if self.shard[1] == 1 else int(self.L.gsr_band_rows(height, self.shard[0], self.shard[1]))

    def read_row_work(self, height: int):
        """gsr_read_row_work (OPT_ROW_WORK = 1): (uint32 [ceil(height / 16)] blend work per GLOBAL tile row of the newest frame, 0 for
        rows this context does not own; the frame's ordinal).  Synchronises"""
        n = (int(height) + TILE - 1) // TILE
        out = np.zeros(n, np.uint32)
        frame = C.c_int64(0)
        _check(self.L.gsr_read_row_work(self.h, out.ctypes.data, n, C.byref(frame)))
        return out, frame.value

    # ---- per frame
    def render(self, cam) -> np.ndarray:
        """synchronous render to a host array [rows, W, 4] of the target format's channel type (float32 by default; row 0 = bottom)"""
        rows = self.band_rows(cam.height)
        out = np.empty((rows, cam.width, 4), dtype=target_dtype(self.target_format))
        cs = camera_struct(cam)
        _check(self.L.gsr_render(self.h, C.byref(cs), out.ctypes.data, 0))
        return out

    def render_depth(self, cam, depth: np.ndarray) -> np.ndarray:
        """depth-tested frame; depth = float32 [H, W] window depth of the opaque pass (row 0 = bottom)"""
        rows = self.band_rows(cam.height)
        out = np.empty((rows, cam.width, 4), dtype=target_dtype(self.target_format))
        d = np.ascontiguousarray(depth, dtype=np.float32).reshape(cam.height, cam.width)
        cs = camera_struct(cam)
        _check(self.L.gsr_render_depth(self.h, C.byref(cs), d.ctypes.data, 0, out.ctypes.data, 0))
        return out

    def render_aov(self, cam, depth: np.ndarray | None = None, aov: int = AOV_DEPTH):
        """the frame of render / render_depth plus the depth AOV: (rgba [rows, W, 4] in the target format, plane float32 [rows, W, 2] =
        {zsum, cov}: the alpha-weighted sum of window depths and the coverage 1 - T, row 0 = bottom)"""
        rows = self.band_rows(cam.height)
        out = np.empty((rows, cam.width, 4), dtype=target_dtype(self.target_format))
        plane = np.empty((rows, cam.width, 2), dtype=np.float32)
        d = None if depth is None else np.ascontiguousarray(depth, dtype=np.float32).reshape(cam.height, cam.width)
        cs = camera_struct(cam)
        _check(self.L.gsr_render_aov(self.h, C.byref(cs), _ptr(d), 0, out.ctypes.data, 0, int(aov), plane.ctypes.data))
        return out, plane

    def render_aov_struct_to_device(self, cam_struct: gsr_camera, device_ptr: int, aov_device_ptr: int, depth_device_ptr: int = 0, aov: int = AOV_DEPTH):
        """gsr_render_aov with every buffer in device memory (the plane: 8 bytes per pixel, 8-byte aligned)"""
        _check(self.L.gsr_render_aov(self.h, C.byref(cam_struct), C.c_void_p(depth_device_ptr or None), 1, C.c_void_p(device_ptr), 1, int(aov),
                                     C.c_void_p(aov_device_ptr or None)))

    def render_over(self, cam, bg, depth: np.ndarray | None = None) -> np.ndarray:
        """the frame of render / render_depth composited over `bg` inside the blend kernel: a premultiplied colour (r, g, b, a), or an
        ndarray [H, W, 4] of float32 / float16 / uint8 (the FULL image also when row-sharded; the format is inferred from the dtype,
        independent of the target format); None = the plain frame.  [rows, W, 4] in the target format, row 0 = bottom"""
        rows = self.band_rows(cam.height)
        out = np.empty((rows, cam.width, 4), dtype=target_dtype(self.target_format))
        d = None if depth is None else np.ascontiguousarray(depth, dtype=np.float32).reshape(cam.height, cam.width)
        b, keep = background_struct(bg, (cam.height, cam.width))
        cs = camera_struct(cam)
        _check(self.L.gsr_render_over(self.h, C.byref(cs), _ptr(d), 0, C.byref(b), out.ctypes.data, 0))
        return out

    def render_over_struct_to_device(self, cam_struct: gsr_camera, bg: gsr_background | None, device_ptr: int, depth_device_ptr: int = 0):
        """gsr_render_over into a device target with a device depth buffer; bg: a gsr_background whose image may live on either side
        (image_is_device) -- a device image must stay valid until the frame completes on the public stream"""
        _check(self.L.gsr_render_over(self.h, C.byref(cam_struct), C.c_void_p(depth_device_ptr or None), 1,
                                      C.byref(bg) if bg is not None else None, C.c_void_p(device_ptr), 1))

    def render_over_struct_to_host(self, cam_struct: gsr_camera, bg: gsr_background | None, host_ptr: int):
        """gsr_render_over into a HOST buffer of the band's pixels in the target format; bg as for render_over_struct_to_device (a
        device image under a host target is the one route render_over cannot take)"""
        _check(self.L.gsr_render_over(self.h, C.byref(cam_struct), None, 0, C.byref(bg) if bg is not None else None, C.c_void_p(host_ptr), 0))

    def resolve_depth(self, aov: np.ndarray, cov_min: float = 0.5) -> np.ndarray:
        """the module's resolve_depth (host, no GPU work): plane [..., 2] -> window depth [...]"""
        return resolve_depth(aov, cov_min)

    def resolve_depth_device(self, aov_device_ptr: int, n_pixels: int, cov_min: float, depth_device_ptr: int):
        """gsr_resolve_depth_device: the same rule as one kernel on the context's public stream"""
        _check(self.L.gsr_resolve_depth_device(self.h, C.c_void_p(aov_device_ptr), int(n_pixels), float(cov_min), C.c_void_p(depth_device_ptr)))

    def policy_state(self) -> dict:
        """the live state of the host-side policies (csrc/gsr_policy.h)"""
        st = np.zeros(16, np.int32)
        _check(self.L.gsr_debug_policy_state(self.h, st.ctypes.data))
        return dict(zip(POLICY_FIELDS, (int(x) for x in st[:11])))

    def render_wire(self, cam) -> np.ndarray:
        """wireframe overlay (outlines of the +-2 quads, colour Cd), [H, W, 4] in the target format"""
        out = np.empty((cam.height, cam.width, 4), dtype=target_dtype(self.target_format))
        cs = camera_struct(cam)
        _check(self.L.gsr_render_wire(self.h, C.byref(cs), out.ctypes.data, 0))
        return out

    def render_wire_over(self, cam, frame: np.ndarray) -> np.ndarray:
        """wire-over display: the outlines on top of `frame` (a finished beauty frame [H, W, 4]); returns the combined image"""
        out = np.ascontiguousarray(frame, dtype=target_dtype(self.target_format)).reshape(cam.height, cam.width, 4).copy()
        cs = camera_struct(cam)
        _check(self.L.gsr_render_wire_over(self.h, C.byref(cs), out.ctypes.data, 0))
        return out

    def render_wire_over_device(self, cam, device_ptr: int):
        cs = camera_struct(cam)
        _check(self.L.gsr_render_wire_over(self.h, C.byref(cs), C.c_void_p(device_ptr), 1))

    def render_to_device(self, cam, device_ptr: int):
        cs = camera_struct(cam)
        _check(self.L.gsr_render(self.h, C.byref(cs), C.c_void_p(device_ptr), 1))

    def render_struct_to_device(self, cam_struct: gsr_camera, device_ptr: int):
        _check(self.L.gsr_render(self.h, C.byref(cam_struct), C.c_void_p(device_ptr), 1))

    def render_struct_to_host(self, cam_struct: gsr_camera, host_ptr: int):
        """gsr_render into a HOST buffer of height x width pixels of the target format (what a caller without GL interop hands over)"""
        _check(self.L.gsr_render(self.h, C.byref(cam_struct), C.c_void_p(host_ptr), 0))

    def render_struct_depth_to_device(self, cam_struct: gsr_camera, depth_device_ptr: int, device_ptr: int):
        """depth-tested frame, both buffers in device memory: what the viewport hook issues on every redraw (hdk/DM_GSplatHook_hip.C)"""
        _check(self.L.gsr_render_depth(self.h, C.byref(cam_struct), C.c_void_p(depth_device_ptr), 1, C.c_void_p(device_ptr), 1))

    def stitch_bands(self, gathered_ptr: int, count: int, width: int, height: int, out_ptr: int):
        _check(self.L.gsr_stitch_bands(self.h, C.c_void_p(gathered_ptr), count, width, height, C.c_void_p(out_ptr)))

    # ---- one process per GPU: the frame's gather inside the library (gsr_comm_*)
    def comm_unique_id(self) -> bytes:
        buf = C.create_string_buffer(128)
        _check(self.L.gsr_comm_get_unique_id(buf))
        return buf.raw

    def comm_init(self, unique_id: bytes, rank: int, world: int):
        _check(self.L.gsr_comm_init(self.h, C.c_char_p(unique_id), int(rank), int(world)))
        self.shard = (rank, world)

    def comm_render(self, cam_struct: gsr_camera, out_ptr: int, depth_ptr: int = 0):
        _check(self.L.gsr_comm_render(self.h, C.byref(cam_struct), C.c_void_p(depth_ptr or None), 1, C.c_void_p(out_ptr or None)))

    def comm_info(self):
        """(rank, ranks) as RCCL itself reports them for this context's communicator"""
        r, n = C.c_int(-1), C.c_int(0)
        _check(self.L.gsr_comm_info(self.h, C.byref(r), C.byref(n)))
        return r.value, n.value

    def comm_destroy(self):
        _check(self.L.gsr_comm_destroy(self.h))
        self.shard = (0, 1)

    def synchronize(self):
        _check(self.L.gsr_synchronize(self.h))

    def stats(self) -> dict:
        st = gsr_stats()
        _check(self.L.gsr_get_stats(self.h, C.byref(st)))
        return st.as_dict()

    def stats_reset(self):
        _check(self.L.gsr_stats_reset(self.h))

    # ---- debug access
    def debug_records(self, n: int) -> np.ndarray:
        out = np.zeros(n, dtype=DEBUG_RECORD_DTYPE)
        _check(self.L.gsr_debug_read_records(self.h, out.ctypes.data, n))
        return out

    def debug_cull(self, n: int):
        """(rect[n] uint32: the packed tile rect K1 gave each splat, by upload index, 0xffffffff = it left no sort entry; the ordered list
        of the clusters k_cluster_cull kept, cluster k = storage slots [64 k, 64 k + 64)) of the last frame"""
        rect = np.zeros(n, dtype=np.uint32)
        nclus = (n + 63) // 64
        clus = np.zeros(max(nclus, 1), dtype=np.uint32)
        cnt = C.c_int64()
        _check(self.L.gsr_debug_read_cull(self.h, rect.ctypes.data, n, clus.ctypes.data, nclus, C.byref(cnt)))
        assert cnt.value <= nclus
        return rect, clus[:cnt.value]

    def debug_depth_order(self, n: int) -> np.ndarray:
        """indices of the splats that survived culling, nearest first"""
        out = np.zeros(n, dtype=np.int32)
        cnt = C.c_int64()
        _check(self.L.gsr_debug_read_depth_order(self.h, out.ctypes.data, n, C.byref(cnt)))
        return out[:cnt.value]

    def debug_storage_order(self, n: int) -> np.ndarray:
        """perm[j] = upload index of the splat in storage slot j (Morton order of the positions by default): what breaks ties in
        the depth sort"""
        out = np.zeros(n, dtype=np.int32)
        _check(self.L.gsr_debug_read_storage_order(self.h, out.ctypes.data, n))
        return out

    def debug_tile_lists(self):
        """per-SUPER-tile [start, end) + the depth-ordered splat list of the last frame"""
        st = self.stats()
        nt = st["stiles_x"] * st["stiles_y"]
        npairs = st["pairs_total"]
        ts = np.zeros(nt, np.int32)
        te = np.zeros(nt, np.int32)
        pv = np.zeros(max(npairs, 1), np.int32)
        _check(self.L.gsr_debug_read_tile_lists(self.h, ts.ctypes.data, te.ctypes.data, nt, pv.ctypes.data, npairs))
        return ts, te, pv[:npairs]

    def debug_tile_work(self) -> np.ndarray:
        """[tiles_y, tiles_x, 4] uint32: list entries scanned / records gathered / wave-record evaluations / saturated flag
        per tile (last frame; the fourth word: bit 0 = went opaque, the rest = the 1024-entry scan step that held its first hit)"""
        st = self.stats()
        nt = st["tiles_x"] * st["tiles_y"]
        out = np.zeros((nt, 4), np.uint32)
        _check(self.L.gsr_debug_read_tile_work(self.h, out.ctypes.data, nt))
        return out.reshape(st["tiles_y"], st["tiles_x"], 4)

    def debug_horizons(self, tiles_x: int, tiles_y: int) -> np.ndarray:
        """[4, tiles_y, tiles_x] float32: dilated horizons / raw horizons (sign = status) / dilated status / covered depths (whole image)"""
        out = np.zeros((4, tiles_y, tiles_x), np.float32)
        _check(self.L.gsr_debug_read_horizons(self.h, out.ctypes.data, tiles_x * tiles_y))
        return out

    def debug_horizon_pyramid(self):
        """(levels, meta): the six levels of the max pyramid the slot's next frame would be culled against, level l a float32 array
        [((tiles_y - 1) >> l) + 1, ((tiles_x - 1) >> l) + 1] over the whole image of the last frame, and the dict of
        PYRAMID_META_FIELDS (pyr_off: the six level offsets; key_min / key_max as unsigned)"""
        words = np.zeros(24, np.int32)
        _check(self.L.gsr_debug_read_horizon_pyramid(self.h, None, 0, words.ctypes.data))      # (the sizes)
        tx, ty = int(words[0]), int(words[1])
        dims = [(((ty - 1) >> l) + 1, ((tx - 1) >> l) + 1) for l in range(PYRAMID_LEVELS)]
        flat = np.zeros(sum(h * w for h, w in dims), np.float32)
        _check(self.L.gsr_debug_read_horizon_pyramid(self.h, flat.ctypes.data, flat.size, words.ctypes.data))
        w = [int(x) for x in words]
        vals = w[:2] + [w[2:2 + PYRAMID_LEVELS]] + w[2 + PYRAMID_LEVELS:]
        meta = dict(zip(PYRAMID_META_FIELDS, vals))
        meta["key_min"] &= 0xffffffff
        meta["key_max"] &= 0xffffffff
        levels = [flat[o:o + h * w_].reshape(h, w_).copy() for o, (h, w_) in zip(meta["pyr_off"], dims)]
        return levels, meta

    def debug_sort_pairs(self, keys: np.ndarray, vals: np.ndarray, key_bits: int = 32, local=None):
        """the pipeline's stable radix sort on host arrays; local = (bucket_lo, bucket_shift): the small-frame form (BK_BUCKETS = 1024 buckets of
        width 2^shift from lo globally, then every bucket on its own)"""
        k = np.ascontiguousarray(keys, dtype=np.uint32).copy()
        v = np.ascontiguousarray(vals, dtype=np.uint32).copy()
        if local is None:
            _check(self.L.gsr_debug_sort_pairs(self.h, k.ctypes.data, v.ctypes.data, k.shape[0], key_bits))
        else:
            _check(self.L.gsr_debug_sort_pairs_local(self.h, k.ctypes.data, v.ctypes.data, k.shape[0], key_bits, int(local[0]), int(local[1])))
        return k, v

    def debug_sort_frame(self, mode: int, keys: np.ndarray, vals: np.ndarray, blk_cnt: np.ndarray, n_slots_dev=None, key_bits: int = 32,
                         allow9: bool = True, lo: int = 0, shift: int = 0, range_dev: bool = False, k1_grid: int = 1 << 30):
        """gsr_debug_sort_frame: a frame's own depth sort (mode = SORT_*) on K1's block-compacted layout -- keys[n_slots] uint32,
        vals[n_slots, 2] uint32, blk_cnt[n_slots / 256] items at the head of every 256 slots, n_slots_dev of the slots filled as far as
        the device knows.  Returns (sorted keys[kept], their payloads [kept, 2], failed: the local sort's "gave up" word)"""
        k = np.ascontiguousarray(keys, dtype=np.uint32).reshape(-1).copy()
        v = np.ascontiguousarray(vals, dtype=np.uint32).reshape(-1).copy()
        c = np.ascontiguousarray(blk_cnt, dtype=np.uint32).reshape(-1)
        if v.shape[0] != 2 * k.shape[0] or c.shape[0] * 256 < k.shape[0]:
            raise ValueError("debug_sort_frame: vals holds one pair per slot and blk_cnt one count per 256 slots")
        kept, failed = C.c_int64(), C.c_uint32()
        _check(self.L.gsr_debug_sort_frame(self.h, int(mode), k.ctypes.data, v.ctypes.data, c.ctypes.data if c.size else None, k.shape[0],
                                           k.shape[0] if n_slots_dev is None else int(n_slots_dev), int(key_bits), int(bool(allow9)),
                                           int(lo), int(shift), int(bool(range_dev)), int(min(k1_grid, 1 << 30)), C.byref(kept), C.byref(failed)))
        return k[:kept.value], v.reshape(-1, 2)[:kept.value], int(failed.value)

    def debug_last_plan(self) -> dict:
        """the plan of the attempt queued last (csrc/gsr_frame_plan.h): which sort the frame really took"""
        out = np.zeros(32, np.int32)
        _check(self.L.gsr_debug_last_plan(self.h, out.ctypes.data))
        return {k: int(x) & 0xffffffff for k, x in zip(PLAN_FIELDS, out)}


class GSplatRenderer:
    """Python face of the C++ GSplatRenderer host shim -- the reference's nine verbs
    (include/GSplatRenderer.h:34-56 of the reference).  ``device=-1`` gives a dry
    instance (registry/staging logic only, no GPU)."""

    Q_REGISTRY_SIZE, Q_ACTIVE_STAGED, Q_SPLAT_COUNT, Q_CAN_RENDER, Q_STAGING_COUNT, Q_RENDER_COUNT, Q_SH_PRESENT, \
        Q_LAST_STATUS, Q_ENTRY_AGE, Q_ENTRY_AGE_SINCE_ACTIVE = range(10)

    def __init__(self, device=0, transport: int = TRANSPORT_AUTO):
        """device: an int (one GPU; -1 = dry) or a sequence of device ordinals (tile rows sharded over them)"""
        self.L = load_library()
        if isinstance(device, (list, tuple)):
            arr = (C.c_int * len(device))(*[int(d) for d in device])
            self.h = self.L.gsplat_renderer_create_multi(arr, len(device), int(transport))
        else:
            self.h = self.L.gsplat_renderer_create(int(device))
        if not self.h:
            raise GsrError(-3, self.L.gsr_last_error().decode("utf-8", "replace") or "gsplat_renderer_create failed")
        self._keep = {}
        self._updates = {}      # rid -> {attribute: the array updateAttributes gave the row last}

    def close(self):
        if getattr(self, "h", None):
            self.L.gsplat_renderer_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def registerUpdate(self, gdp: int, gversion, gVtxOffset: int, splats, splatOrigin=None) -> str:
        a = _Arrays(splats)
        origin = splats.barycenter() if splatOrigin is None else splatOrigin
        ver = (C.c_int64 * 4)(*[int(x) for x in gversion])
        buf = C.create_string_buffer(256)
        p = a.ptrs()
        n = self.L.gsplat_renderer_register_update(self.h, int(gdp), ver, int(gVtxOffset), a.n, _f3(origin), *p,
                                                   a.n if a.shx is not None else 0, buf, 256)
        if n < 0:
            raise GsrError(n, "registerUpdate failed")
        rid = buf.value.decode()
        self._keep[rid] = a  # the shim BORROWS the arrays, as the reference does
        # the new registration replaced every pointer of the row, and retired the rows of older versions of its detail
        detail = rid.split("__", 1)[0] + "__"
        for k in [k for k in self._updates if k == rid or (k.startswith(detail) and k.rsplit("__", 1)[-1] != rid.rsplit("__", 1)[-1])]:
            del self._updates[k]
        return rid

    def updateAttributes(self, rid: str, Cd=None, alpha=None, scale=None, orient=None, shx=None, shy=None, shz=None):
        """GSplatRenderer::updateAttributes: new arrays for a registered primitive whose positions did not change -> (rc, first, n):
        rc 1 = its resident splats [first, first + n) were edited in place, 0 = not resident (staged when next shown), < 0 = GSR_E_*.
        The shim BORROWS the arrays: each is kept alive here, one per attribute of the row, in place of the one it replaces."""
        given = dict(Cd=Cd, alpha=alpha, scale=scale, orient=orient, shx=shx, shy=shy, shz=shz)
        u, n, keep = attr_update_struct(**given)
        first, cnt = C.c_int64(0), C.c_int64(0)
        rc = int(self.L.gsplat_renderer_update_attributes(self.h, rid.encode(), u.Cd, u.alpha, u.scale, u.orient, u.shx, u.shy, u.shz,
                                                          C.byref(first), C.byref(cnt)))
        # keep what the row holds NOW: a refused call may or may not have replaced its pointers (an unknown id or bad SH arrays: not;
        # an engine's refusal: yes), so ask the row
        what = {"Cd": 1, "alpha": 2, "scale": 3, "orient": 4, "shx": 5, "shy": 6, "shz": 7}
        names = [k for k, _, _ in UPDATE_ATTRS if given[k] is not None]
        for k, a in zip(names, keep):
            if self.rowArray(rid, what[k]) == a.ctypes.data:
                self._updates.setdefault(rid, {})[k] = a
        return rc, first.value, cnt.value

    def moveSplats(self, rid: str, P, origin=None, Cd=None, alpha=None, scale=None, orient=None, shx=None, shy=None, shz=None):
        """GSplatRenderer::moveSplats: new positions (and optionally a new origin and new attribute arrays) for a registered primitive
        whose point count did not change -> (rc, first, n) as updateAttributes returns them.  The arrays are BORROWED and kept alive
        here, P included, in place of the ones they replace."""
        given = dict(Cd=Cd, alpha=alpha, scale=scale, orient=orient, shx=shx, shy=shy, shz=shz)
        P, n, u, keep = move_arrays(P, **given)
        first, cnt = C.c_int64(0), C.c_int64(0)
        rc = int(self.L.gsplat_renderer_move_splats(self.h, rid.encode(), P.ctypes.data, None if origin is None else _f3(origin),
                                                    u.Cd, u.alpha, u.scale, u.orient, u.shx, u.shy, u.shz, C.byref(first), C.byref(cnt)))
        what = {"P": 0, "Cd": 1, "alpha": 2, "scale": 3, "orient": 4, "shx": 5, "shy": 6, "shz": 7}
        names = ["P"] + [k for k, _, _ in UPDATE_ATTRS if given[k] is not None]
        for k, a in zip(names, [P] + keep):
            if self.rowArray(rid, what[k]) == a.ctypes.data:
                self._updates.setdefault(rid, {})[k] = a
        return rc, first.value, cnt.value

    def rowArray(self, rid: str, what: int) -> int:
        """address of the array a registered row holds now (0 P, 1 Cd, 2 alpha, 3 scale, 4 orient, 5..7 shx / shy / shz); 0 = none"""
        return int(self.L.gsplat_renderer_row_array(self.h, rid.encode(), int(what)) or 0)

    def includeInRenderPass(self, rid: str):
        self.L.gsplat_renderer_include_in_render_pass(self.h, rid.encode())

    def flushEntriesForMatchingDetail(self, rid: str):
        self.L.gsplat_renderer_flush_entries_for_matching_detail(self.h, rid.encode())
        # the rows of that detail are gone: ids are "<detail>__<vertex offset>__<version>"
        detail = rid.split("__", 1)[0] + "__"
        for k in [k for k in self._updates if k.startswith(detail)]:
            del self._updates[k]

    @staticmethod
    def context(cam, target=None, target_is_device=False) -> GSplatRenderContext:
        r = GSplatRenderContext()
        for name in ("obj_view", "object", "inv_object", "view", "proj"):
            getattr(r, name)[:] = np.asarray(getattr(cam, name), dtype=np.float32).reshape(16).tolist()
        r.width, r.height = int(cam.width), int(cam.height)
        r.target = target
        r.target_is_device = int(bool(target_is_device))
        return r

    def generateRenderGeometry(self, r: GSplatRenderContext):
        self.L.gsplat_renderer_generate_render_geometry(self.h, C.byref(r))

    def render(self, r: GSplatRenderContext, isObjectLevel: bool = False):
        self.L.gsplat_renderer_render(self.h, C.byref(r), int(isObjectLevel))

    def postRender(self):
        self.L.gsplat_renderer_post_render(self.h)

    def redraw(self, rids, r: GSplatRenderContext, isObjectLevel: bool = False):
        """one redraw as the reference drives it (includeInRenderPass x N -> generateRenderGeometry -> render -> postRender) in ONE foreign call"""
        key = tuple(rids)
        if getattr(self, "_ids_key", None) != key:
            self._ids_key = key
            self._ids_arr = (C.c_char_p * len(rids))(*[x.encode() for x in rids])
        self.L.gsplat_renderer_redraw(self.h, self._ids_arr, len(rids), C.byref(r), int(isObjectLevel))

    def engine_stats(self) -> dict:
        """gsr_stats of the context behind the verbs (one GPU)"""
        st = gsr_stats()
        _check(self.L.gsr_get_stats(self.L.gsplat_renderer_engine(self.h), C.byref(st)))
        return st.as_dict()

    def setRenderingEnabled(self, enabled: bool):
        self.L.gsplat_renderer_set_rendering_enabled(self.h, int(enabled))

    def setExplicitCameraPos(self, pos):
        self.L.gsplat_renderer_set_explicit_camera_pos(self.h, _f3(pos))

    def setSphericalHarmonicsOrder(self, order: int):
        self.L.gsplat_renderer_set_spherical_harmonics_order(self.h, int(order))

    def setTargetFormat(self, fmt: int) -> int:
        """what a pixel of GSplatRenderContext.target is (TARGET_*); 0, or a negative GSR_E_* code for an unknown format"""
        return int(self.L.gsplat_renderer_set_target_format(self.h, int(fmt)))

    def targetFormat(self) -> int:
        return int(self.L.gsplat_renderer_get_target_format(self.h))

    def setAovTarget(self, aov: int, plane_ptr: int | None) -> int:
        """from the next render() on every frame also writes the depth AOV {zsum, cov} (height x width x 2 float32) to plane_ptr, which
        lives where GSplatRenderContext.target lives and must stay alive; aov = 0 or no pointer switches it off.  0 or a GSR_E_* code"""
        return int(self.L.gsplat_renderer_set_aov_target(self.h, int(aov), C.c_void_p(plane_ptr or None)))

    def setBackground(self, bg: gsr_background | None) -> int:
        """from the next render() on every frame is composited over *bg (copied; an image it names is borrowed and must stay alive);
        None or kind 0 clears it.  0 or a GSR_E_* code"""
        return int(self.L.gsplat_renderer_set_background(self.h, C.byref(bg) if bg is not None else None))

    def setVisibility(self, vis: gsr_visibility | None) -> int:
        """crop volumes (visibility_struct; no mask: the shim refuses one) that hide resident splats from the next render() on and
        through every re-stage; None or no volume clears them.  0 or a GSR_E_* code"""
        return int(self.L.gsplat_renderer_set_visibility(self.h, C.byref(vis) if vis is not None else None))

    def query(self, what: int, rid: str | None = None) -> int:
        return int(self.L.gsplat_renderer_query(self.h, what, rid.encode() if rid else None))

    def origin(self) -> np.ndarray:
        o = (C.c_float * 3)()
        self.L.gsplat_renderer_get_origin(self.h, o)
        return np.array(list(o), dtype=np.float32)

    def lastCameraPos(self) -> np.ndarray:
        o = (C.c_float * 3)()
        self.L.gsplat_renderer_get_last_camera_pos(self.h, o)
        return np.array(list(o), dtype=np.float32)

    def frame(self, cam, rids, height=None) -> np.ndarray:
        """one redraw exactly as the reference drives it: N x GR_PrimGsplat::render marks entries
        active, then the scene hook runs generate -> render -> postRender (src/DM_GSplatHook.C:30-39)"""
        for rid in rids:
            self.includeInRenderPass(rid)
        out = np.zeros((cam.height, cam.width, 4), dtype=target_dtype(self.targetFormat()))
        r = self.context(cam, out.ctypes.data, False)
        self.generateRenderGeometry(r)
        self.render(r, False)
        self.postRender()
        return out


def quantize_half(a: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.float32)
    out = np.empty(a.shape, dtype=np.uint16)
    load_library().gsplat_quantize_half(a.ctypes.data, out.ctypes.data, a.size)
    return out


class MultiEngine:
    """gsr_multi_*: several GPUs (or several contexts on one GPU, transport COPY) driven from this one thread."""

    def __init__(self, devices, transport: int = TRANSPORT_AUTO):
        self.L = load_library()
        arr = (C.c_int * len(devices))(*[int(d) for d in devices])
        h = C.c_void_p()
        _check(self.L.gsr_multi_create(arr, len(devices), int(transport), C.byref(h)))
        self.h = h
        self.count = len(devices)
        self.target_format = TARGET_RGBA32F

    def close(self):
        if getattr(self, "h", None):
            self.L.gsr_multi_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def transport(self) -> int:
        return int(self.L.gsr_multi_transport(self.h))

    def set_stream(self, hip_stream):
        _check(self.L.gsr_multi_set_stream(self.h, C.c_void_p(hip_stream or 0)))

    def set_option(self, option: int, value: int):
        _check(self.L.gsr_multi_set_option(self.h, option, value))

    def set_target_format(self, fmt: int):
        """every rank renders, and the gather moves, pixels of this format (TARGET_*) from the next frame on"""
        _check(self.L.gsr_multi_set_target_format(self.h, int(fmt)))
        self.target_format = int(fmt)

    def upload(self, splats, origin=(0.0, 0.0, 0.0)):
        a = _Arrays(splats)
        _check(self.L.gsr_multi_upload(self.h, a.n, *a.ptrs(), _f3(origin)))

    def update_attrs(self, first: int, Cd=None, alpha=None, scale=None, orient=None, shx=None, shy=None, shz=None) -> int:
        """gsr_multi_update: Engine.update_attrs on every rank"""
        u, n, keep = attr_update_struct(Cd=Cd, alpha=alpha, scale=scale, orient=orient, shx=shx, shy=shy, shz=shz)
        _check(self.L.gsr_multi_update(self.h, int(first), n, C.byref(u)))
        return n

    def move(self, first: int, P, origin=None, **attrs) -> int:
        """gsr_multi_move: Engine.move on every rank"""
        P, n, u, keep = move_arrays(P, **attrs)
        _check(self.L.gsr_multi_move(self.h, int(first), n, P.ctypes.data, None if origin is None else _f3(origin), C.byref(u)))
        return n

    def set_visibility(self, vis=None, volumes=None, mask=None):
        """gsr_multi_set_visibility: Engine.set_visibility on every rank"""
        keep = None
        if vis is None and (volumes is not None or mask is not None):
            vis, keep = visibility_struct(volumes or (), mask)
        _check(self.L.gsr_multi_set_visibility(self.h, C.byref(vis) if vis is not None else None))

    def remove(self, mask=None, hidden: bool = False) -> int:
        """gsr_multi_remove: Engine.remove on every rank, from a host mask -> the splats left (the ranks agree, or none keeps geometry)"""
        words = removal_words(mask, self.stats(0)["n_splats"])
        left = C.c_int64(0)
        _check(self.L.gsr_multi_remove(self.h, None if words is None else words.ctypes.data, REMOVE_HIDDEN if hidden else 0, C.byref(left)))
        return left.value

    def add(self, splats) -> int:
        """gsr_multi_add: Engine.add on every rank, from host arrays -> the splats resident now (the ranks agree, or none keeps geometry)"""
        a = add_arrays(splats)
        total = C.c_int64(0)
        _check(self.L.gsr_multi_add(self.h, a.n, *a.ptrs(), C.byref(total)))
        return total.value

    def transform(self, x: gsr_xform, mask=None) -> int:
        """gsr_multi_transform: Engine.transform on every rank, from a host mask -> the splats moved (the ranks agree, or none keeps
        geometry)"""
        words = removal_words(mask, self.stats(0)["n_splats"])
        moved = C.c_int64(0)
        _check(self.L.gsr_multi_transform(self.h, None if words is None else words.ctypes.data, C.byref(x) if x is not None else None, C.byref(moved)))
        return moved.value

    def grade(self, rule, mask=None) -> int:
        """gsr_multi_grade: Engine.grade on every rank, from a host mask -> the splats graded (the ranks agree, or none keeps
        geometry)"""
        words = removal_words(mask, self.stats(0)["n_splats"])
        r = _grade_rule_struct(rule)
        graded = C.c_int64(0)
        _check(self.L.gsr_multi_grade(self.h, None if words is None else words.ctypes.data, C.byref(r) if r is not None else None, C.byref(graded)))
        return graded.value

    def read(self, first: int = 0, n=None, names=None):
        """gsr_multi_read: Engine.read of rank 0's copy (the cloud is replicated) -> scenes.Splats"""
        cnt, sh = C.c_int64(0), C.c_int(0)
        _check(self.L.gsr_read_info(self.L.gsr_multi_context(self.h, 0), C.byref(cnt), C.byref(sh), None))
        return _read_splats(self.L, self.L.gsr_multi_read, self.h, (cnt.value, bool(sh.value)), first, n, names)

    def read_masked(self, mask, names=None):
        """gsr_multi_read_masked: Engine.read_masked of rank 0's copy (the cloud is replicated), from a host mask -> scenes.Splats"""
        cnt, sh = C.c_int64(0), C.c_int(0)
        _check(self.L.gsr_read_info(self.L.gsr_multi_context(self.h, 0), C.byref(cnt), C.byref(sh), None))
        verb = lambda ptr, max_rows, r, m: self.L.gsr_multi_read_masked(self.h, ptr, max_rows, r, m)     # noqa: E731
        return _read_masked_splats(verb, (cnt.value, bool(sh.value)), mask, names)

    def duplicate(self, mask=None):
        """gsr_multi_duplicate: Engine.duplicate on every rank, from a host mask -> (the copies, the splats resident now) (the ranks
        agree, or none keeps geometry)"""
        words = removal_words(mask, self.stats(0)["n_splats"])
        m, total = C.c_int64(0), C.c_int64(0)
        _check(self.L.gsr_multi_duplicate(self.h, None if words is None else words.ctypes.data, C.byref(m), C.byref(total)))
        return m.value, total.value

    def select(self, cam, region, mask=None):
        """gsr_multi_select: Engine.select on rank 0's copy (the cloud is replicated), into a host mask -> (bool mask, n_hit, n_set)"""
        r, keep = region if isinstance(region, tuple) else (region, [])
        _region_fits(cam, keep, "select")
        cnt = C.c_int64(0)
        _check(self.L.gsr_read_info(self.L.gsr_multi_context(self.h, 0), C.byref(cnt), None, None))
        n = cnt.value
        words = removal_words(np.zeros(n, bool) if mask is None else mask, n).copy()
        hit, nset = C.c_int64(0), C.c_int64(0)
        cs = cam if isinstance(cam, gsr_camera) else camera_struct(cam)
        _check(self.L.gsr_multi_select(self.h, C.byref(cs), C.byref(r), words.ctypes.data, C.byref(hit), C.byref(nset)))
        return unpack_mask(words, n), hit.value, nset.value

    def select_attrs(self, rule: gsr_attr_rule, mask=None):
        """gsr_multi_select_attrs: Engine.select_attrs on rank 0's copy (the cloud is replicated), into a host mask -> (bool mask, n_hit,
        n_set)"""
        cnt = C.c_int64(0)
        _check(self.L.gsr_read_info(self.L.gsr_multi_context(self.h, 0), C.byref(cnt), None, None))
        n = cnt.value
        words = removal_words(np.zeros(n, bool) if mask is None else mask, n).copy()
        hit, nset = C.c_int64(0), C.c_int64(0)
        _check(self.L.gsr_multi_select_attrs(self.h, C.byref(rule), words.ctypes.data, C.byref(hit), C.byref(nset)))
        return unpack_mask(words, n), hit.value, nset.value

    def select_density(self, rule: gsr_density_rule, mask=None, counts: bool = False):
        """gsr_multi_select_density: Engine.select_density on rank 0's copy (the cloud is replicated), into a host mask -> (bool mask,
        n_hit, n_set, the gsr_density_result[, the neighbour counts])"""
        c64 = C.c_int64(0)
        _check(self.L.gsr_read_info(self.L.gsr_multi_context(self.h, 0), C.byref(c64), None, None))
        n = c64.value
        words = removal_words(np.zeros(n, bool) if mask is None else mask, n).copy()
        cnt = np.zeros(max(n, 1), np.uint32)
        hit, nset, res = C.c_int64(0), C.c_int64(0), gsr_density_result()
        _check(self.L.gsr_multi_select_density(self.h, C.byref(rule), words.ctypes.data, cnt.ctypes.data if counts else None, C.byref(res),
                                               C.byref(hit), C.byref(nset)))
        return (unpack_mask(words, n), hit.value, nset.value, res) + ((cnt[:n],) if counts else ())

    def select_connected(self, rule: gsr_connect_rule, mask=None, seed=None, outputs: bool = False):
        """gsr_multi_select_connected: Engine.select_connected on rank 0's copy (the cloud is replicated), everything in host memory ->
        (bool mask, n_hit, n_set, the gsr_connect_result[, the labels, the sizes])"""
        c64 = C.c_int64(0)
        _check(self.L.gsr_read_info(self.L.gsr_multi_context(self.h, 0), C.byref(c64), None, None))
        n = c64.value
        words = removal_words(np.zeros(n, bool) if mask is None else mask, n).copy()
        sw = None if seed is None else removal_words(seed, n).copy()
        lab, siz = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
        hit, nset, res = C.c_int64(0), C.c_int64(0), gsr_connect_result()
        _check(self.L.gsr_multi_select_connected(self.h, C.byref(rule), sw.ctypes.data if sw is not None and n else None, words.ctypes.data,
                                                 lab.ctypes.data if outputs else None, siz.ctypes.data if outputs else None, C.byref(res),
                                                 C.byref(hit), C.byref(nset)))
        return (unpack_mask(words, n), hit.value, nset.value, res) + ((lab[:n], siz[:n]) if outputs else ())

    def measure(self, request: gsr_measure_request, mask=None) -> gsr_measure_result:
        """gsr_multi_measure: Engine.measure on rank 0's copy (the cloud is replicated), from a host mask (None: every splat)"""
        cnt = C.c_int64(0)
        _check(self.L.gsr_read_info(self.L.gsr_multi_context(self.h, 0), C.byref(cnt), None, None))
        words = removal_words(mask, cnt.value)
        res = gsr_measure_result()
        hist = np.zeros(max(_measure_hist_words(request), 1), np.uint32)
        _check(self.L.gsr_multi_measure(self.h, _ptr(words), C.byref(request), C.byref(res), hist.ctypes.data if request.n_hist > 0 else None))
        return _measure_result(request, res, hist)

    def render(self, cam, depth=None) -> np.ndarray:
        out = np.empty((cam.height, cam.width, 4), dtype=target_dtype(self.target_format))
        cs = camera_struct(cam)
        if depth is None:
            _check(self.L.gsr_multi_render(self.h, C.byref(cs), out.ctypes.data, 0))
        else:
            d = np.ascontiguousarray(depth, dtype=np.float32).reshape(cam.height, cam.width)
            _check(self.L.gsr_multi_render_depth(self.h, C.byref(cs), d.ctypes.data, 0, out.ctypes.data, 0))
        return out

    def render_struct_to_device(self, cam_struct: gsr_camera, device_ptr: int, depth_ptr: int = 0):
        _check(self.L.gsr_multi_render_depth(self.h, C.byref(cam_struct), C.c_void_p(depth_ptr or None), 1,
                                             C.c_void_p(device_ptr), 1))

    def synchronize(self):
        _check(self.L.gsr_multi_synchronize(self.h))

    def comm_info(self):
        """([ncclCommUserRank of every rank's communicator], ncclCommCount); ([-1, ...], 0) with the COPY transport"""
        ranks = (C.c_int * self.count)()
        n = C.c_int(0)
        _check(self.L.gsr_multi_comm_info(self.h, ranks, C.byref(n)))
        return list(ranks), n.value

    def gather_stats(self, enable: int = -1):
        """(milliseconds, gathers) measured on the root's transfer stream so far; enable = 1 / 0 switches the measurement"""
        ms, k = C.c_double(0.0), C.c_int64(0)
        _check(self.L.gsr_multi_gather_stats(self.h, int(enable), C.byref(ms), C.byref(k)))
        return ms.value, k.value

    def stats(self, rank: int = 0) -> dict:
        st = gsr_stats()
        _check(self.L.gsr_multi_get_stats(self.h, rank, C.byref(st)))
        return st.as_dict()

    def get_bands(self):
        """gsr_multi_get_bands: ([count + 1] boundaries of the last frame's bands in tile rows, how often they have changed)"""
        first = np.zeros(self.count + 1, np.int32)
        n = C.c_int64(0)
        _check(self.L.gsr_multi_get_bands(self.h, first.ctypes.data, C.byref(n)))
        return first, n.value


class GSplatPrim:
    """Python face of the GSplatPrim mirror of GR_PrimGsplat (include/GSplatPrim.h): attribute ingest + the
    per-redraw verbs.  attrs: dict of float32 arrays keyed by Houdini attribute names
    (P, Cd, opacity, Alpha, scale, orient, sh_coefficients, sh1..sh15, f_rest_0..44) plus the detail attributes
    gsplat__sh_order (int) and gsplat__explicit_camera_pos (3 floats)."""

    def __init__(self, renderer: GSplatRenderer):
        self.L = load_library()
        self.R = renderer
        self.h = self.L.gsplat_prim_create(renderer.h)
        if not self.h:
            raise GsrError(-1, "gsplat_prim_create failed")
        self.id = ""
        self._keep = None

    def close(self):
        if getattr(self, "h", None):
            self.L.gsplat_prim_destroy(self.h)
            self.h = None

    def update(self, detail: int, version, vtx_offset: int, attrs: dict, barycenter=None) -> str:
        f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
        keep = {k: f32(v) for k, v in attrs.items() if not k.startswith("gsplat__")}
        a = gsplat_attrs()
        a.count = int(keep["P"].reshape(-1, 3).shape[0]) if "P" in keep else 0
        for name in ("P", "Cd", "opacity", "Alpha", "scale", "orient"):
            setattr(a, name, keep[name].ctypes.data if name in keep else None)
        if "sh_coefficients" in keep:
            a.sh_coefficients = keep["sh_coefficients"].ctypes.data
            a.sh_coefficients_len = int(keep["sh_coefficients"].size // max(a.count, 1))
        sh_ptrs = (C.c_void_p * 15)(*[keep[f"sh{k + 1}"].ctypes.data if f"sh{k + 1}" in keep else None for k in range(15)])
        fr_ptrs = (C.c_void_p * 45)(*[keep[f"f_rest_{k}"].ctypes.data if f"f_rest_{k}" in keep else None for k in range(45)])
        a.sh = sh_ptrs
        a.f_rest = fr_ptrs
        order = C.c_int32(int(attrs["gsplat__sh_order"])) if "gsplat__sh_order" in attrs else None
        a.sh_order = C.pointer(order) if order is not None else None
        eye = _f3(attrs["gsplat__explicit_camera_pos"]) if "gsplat__explicit_camera_pos" in attrs else None
        a.explicit_camera_pos = eye
        ver = (C.c_int64 * 4)(*[int(x) for x in version])
        buf = C.create_string_buffer(256)
        bc = _f3(barycenter) if barycenter is not None else None
        n = self.L.gsplat_prim_update(self.h, int(detail), ver, int(vtx_offset), C.byref(a), bc, buf, 256)
        if n < 0:
            raise GsrError(n, "gsplat_prim_update failed")
        self._keep = (keep, sh_ptrs, fr_ptrs, order, eye)
        self.id = buf.value.decode()
        return self.id

    def render(self, beauty_mode: bool = True):
        self.L.gsplat_prim_render(self.h, int(beauty_mode))

    @property
    def missing(self) -> int:
        return int(self.L.gsplat_prim_missing(self.h))

    @property
    def sh_order(self) -> int:
        return int(self.L.gsplat_prim_sh_order(self.h))

    @property
    def has_sh(self) -> bool:
        return bool(self.L.gsplat_prim_has_sh(self.h))

    def arrays(self, n: int):
        """the quantised registerUpdate-layout arrays (copies) as a scenes.Splats-like namespace"""
        import types
        def grab(what, dtype, width):
            p = self.L.gsplat_prim_array(self.h, what)
            if not p:
                return None
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(n * width * np.dtype(dtype).itemsize,)) \
                .view(dtype).reshape(n, width).copy()
        return types.SimpleNamespace(P=grab(0, np.float32, 3), Cd=grab(1, np.uint16, 3), alpha=grab(2, np.float32, 1).reshape(n),
                                     scale=grab(3, np.uint16, 3), orient=grab(4, np.uint16, 4), shx=grab(5, np.uint16, 16),
                                     shy=grab(6, np.uint16, 16), shz=grab(7, np.uint16, 16), n=n)
