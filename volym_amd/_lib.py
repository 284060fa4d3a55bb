"""ctypes binding of libvolym_hip.so (include/volym_hip.h + include/volym_host.h).

There is no CPU fallback: if the shared library is missing or a call fails, this raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VOLYM_HIP_LIB") or os.path.join(_HERE, "libvolym_hip.so")   # the override is for A/B builds during development

OK, E_INVALID, E_HIP, E_NO_DEVICE, E_NOMEM, E_STATE = 0, -1, -2, -3, -4, -5
FILTER_NEAREST, FILTER_LINEAR = 0, 1
OPT_KERNEL, OPT_WRITE_F32, OPT_MACRO_CELLS = 1, 2, 3
OPT_VOLUME_LAYOUT, OPT_CULLING, OPT_COST_FEEDBACK, OPT_DEPTH_PARALLEL, OPT_XCD_BANDS, OPT_REBALANCE_ROUNDS = 4, 5, 6, 7, 8, 9
OPT_SETUP_IEEE = 10
OPT_FRAMES_IN_FLIGHT = 11
OPT_BOUNDS_CELLS = 12
OPT_TEXEL_BYTES = 13


class VolymError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("volym error %d: %s" % (code, msg))
        self.code = code


class CameraUniforms(C.Structure):
    """src/gpu_resources/camera.rs:56-64"""
    _fields_ = [
        ("view_matrix", (C.c_float * 4) * 4),
        ("projection_matrix", (C.c_float * 4) * 4),
        ("inverse_view_proj", (C.c_float * 4) * 4),
        ("camera_position", C.c_float * 3),
        ("_padding", C.c_float),
    ]


class ParameterUniforms(C.Structure):
    """src/gpu_resources/parameters.rs:55-66"""
    _fields_ = [
        ("density_threshold", C.c_float),
        ("use_cone_importance_check", C.c_uint32),
        ("use_importance_coloring", C.c_uint32),
        ("use_opacity", C.c_uint32),
        ("use_importance_rendering", C.c_uint32),
        ("use_gaussian_smoothing", C.c_uint32),
        ("importance_check_ahead_steps", C.c_uint32),
        ("raymarching_step_size", C.c_float),
    ]


class Stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_vol", "n_imp", "n_steps", "n_dense", "n_hit", "n_rays")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class Pick(C.Structure):
    """volym_pick (include/volym_hip.h): the record of one picked pixel, 16 bytes"""
    _fields_ = [
        ("t", C.c_float),
        ("x", C.c_uint16), ("y", C.c_uint16), ("z", C.c_uint16),
        ("label", C.c_uint8), ("density", C.c_uint8), ("status", C.c_uint8), ("alpha8", C.c_uint8),
        ("has_labels", C.c_uint8), ("reserved", C.c_uint8),
    ]


# the same record as a NumPy structured dtype (GpuContext.read_picks)
PICK_DTYPE = np.dtype([("t", "<f4"), ("x", "<u2"), ("y", "<u2"), ("z", "<u2"), ("label", "u1"), ("density", "u1"), ("status", "u1"),
                       ("alpha8", "u1"), ("has_labels", "u1"), ("reserved", "u1")])
PICK_MISS, PICK_NONE, PICK_HIT = 0, 1, 2      # volym_pick.status


class Outline(C.Structure):
    """volym_outline (include/volym_hip.h): selection, colours and radius of one outline pass, 268 bytes"""
    _fields_ = [
        ("selected", C.c_uint8 * 256),
        ("ring_rgba", C.c_uint8 * 4),
        ("fill_rgba", C.c_uint8 * 4),
        ("radius", C.c_uint32),
    ]


SLICE_DENSITY, SLICE_TF, SLICE_IMPORTANCE = 0, 1, 2           # volym_slice.mode
SLICE_UNCUT, SLICE_LABELS, SLICE_MARK_CUT = 1, 2, 4            # volym_slice.flags


class Slice(C.Structure):
    """volym_slice (include/volym_hip.h): geometry, mode, flags and colours of one slice pass, 1084 bytes"""
    _fields_ = [
        ("origin", C.c_int32 * 3),
        ("du", C.c_int32 * 3),
        ("dv", C.c_int32 * 3),
        ("width", C.c_uint32), ("height", C.c_uint32),
        ("mode", C.c_uint32), ("flags", C.c_uint32),
        ("background", C.c_uint8 * 4),
        ("cut_rgba", C.c_uint8 * 4),
        ("palette", (C.c_uint8 * 4) * 256),
    ]


PROJECT_MAX, PROJECT_MEAN = 0, 1                               # volym_project.mode
PROJECT_TF, PROJECT_LABELS, PROJECT_NO_SKIP = 1, 2, 4          # volym_project.flags


class Project(C.Structure):
    """volym_project (include/volym_hip.h): step, mode, flags and colours of one projection pass, 1040 bytes"""
    _fields_ = [
        ("step", C.c_float),
        ("mode", C.c_uint32), ("flags", C.c_uint32),
        ("background", C.c_uint8 * 4),
        ("palette", (C.c_uint8 * 4) * 256),
    ]


class Projection(C.Structure):
    """volym_projection (include/volym_hip.h): the record of one projected ray, 16 bytes"""
    _fields_ = [
        ("t", C.c_float),
        ("x", C.c_uint16), ("y", C.c_uint16), ("z", C.c_uint16),
        ("max", C.c_uint8), ("mean", C.c_uint8), ("label", C.c_uint8), ("status", C.c_uint8),
        ("n_samples", C.c_uint16),
    ]


# the same record as a NumPy structured dtype (GpuContext.read_projection)
PROJECTION_DTYPE = np.dtype([("t", "<f4"), ("x", "<u2"), ("y", "<u2"), ("z", "<u2"), ("max", "u1"), ("mean", "u1"), ("label", "u1"),
                             ("status", "u1"), ("n_samples", "<u2")])
PROJECTION_MISS, PROJECTION_EMPTY, PROJECTION_HIT = 0, 1, 2   # volym_projection.status


MEASURE_UNCUT = 1                                              # volym_measure.flags
MEASURE_GROUPS, MEASURE_NO_GROUP = 8, 255


class Measure(C.Structure):
    """volym_measure (include/volym_hip.h): box, flags and group table of one measure pass, 284 bytes"""
    _fields_ = [
        ("box", C.c_uint32 * 6),
        ("flags", C.c_uint32),
        ("group", C.c_uint8 * 256),
    ]


class SegmentStats(C.Structure):
    """volym_segment_stats (include/volym_hip.h): the record of one label value, 80 bytes"""
    _fields_ = [
        ("count", C.c_uint64), ("sum", C.c_uint64), ("sum_sq", C.c_uint64),
        ("sum_x", C.c_uint64), ("sum_y", C.c_uint64), ("sum_z", C.c_uint64),
        ("box", C.c_int32 * 6),
        ("min", C.c_uint32), ("max", C.c_uint32),
    ]


class Measurement(C.Structure):
    """volym_measurement (include/volym_hip.h): 256 records and 8 histograms of 256 bins, 36864 bytes"""
    _fields_ = [
        ("seg", SegmentStats * 256),
        ("hist", (C.c_uint64 * 256) * 8),
    ]


# the record as a NumPy structured dtype (GpuContext.read_measure, scene.measure_volume)
SEGMENT_STATS_DTYPE = np.dtype([("count", "<u8"), ("sum", "<u8"), ("sum_sq", "<u8"), ("sum_x", "<u8"), ("sum_y", "<u8"), ("sum_z", "<u8"),
                                ("box", "<i4", (6,)), ("min", "<u4"), ("max", "<u4")])


SURFACE_UNCUT = 1                                              # volym_surface.flags
SURFACE_SCAN_ROWS = 256                                        # rows of a request's box per workgroup of the offset scan


class Surface(C.Structure):
    """volym_surface (include/volym_hip.h): box, flags, min_byte and select table of one surface pass, 288 bytes"""
    _fields_ = [
        ("box", C.c_uint32 * 6),
        ("flags", C.c_uint32),
        ("min_byte", C.c_uint32),
        ("select", C.c_uint8 * 256),
    ]


class SurfaceSummary(C.Structure):
    """volym_surface_summary (include/volym_hip.h): faces per label and direction, their total and the divergence sums, 24584 bytes"""
    _fields_ = [
        ("faces", (C.c_uint64 * 6) * 256),
        ("total", C.c_uint64),
        ("pos", (C.c_uint64 * 3) * 256),
        ("neg", (C.c_uint64 * 3) * 256),
    ]


class SurfaceFace(C.Structure):
    """volym_surface_face (include/volym_hip.h): one boundary face, 8 bytes"""
    _fields_ = [("x", C.c_uint16), ("y", C.c_uint16), ("z", C.c_uint16), ("dir", C.c_uint8), ("label", C.c_uint8)]


# the summary and the face record as NumPy structured dtypes (GpuContext.read_surface / read_surface_faces, scene.surface_volume)
SURFACE_SUMMARY_DTYPE = np.dtype([("faces", "<u8", (256, 6)), ("total", "<u8"), ("pos", "<u8", (256, 3)), ("neg", "<u8", (256, 3))])
SURFACE_FACE_DTYPE = np.dtype([("x", "<u2"), ("y", "<u2"), ("z", "<u2"), ("dir", "u1"), ("label", "u1")])


COMPONENTS_UNCUT, COMPONENTS_SPLIT_LABELS = 1, 2               # volym_components.flags
COMPONENTS_DEFAULT_MAX = 65536                                 # max_components == 0
COMPONENTS_TABLE_MAX = 1 << 24                                 # largest max_components
COMPONENTS_BOX_MAX = 2 ** 31 - 2                               # most texels of a request's box
COMPONENT_NONE = 0xFFFFFFFF                                    # id of a texel that is not solid


class Components(C.Structure):
    """volym_components (include/volym_hip.h): box, flags, min_byte, select table and table capacity of one components pass, 292 bytes"""
    _fields_ = [
        ("box", C.c_uint32 * 6),
        ("flags", C.c_uint32),
        ("min_byte", C.c_uint32),
        ("select", C.c_uint8 * 256),
        ("max_components", C.c_uint32),
    ]


class ComponentsSummary(C.Structure):
    """volym_components_summary (include/volym_hip.h): components, solid texels, records kept and components per root label, 2072 bytes"""
    _fields_ = [("n_components", C.c_uint64), ("n_solid", C.c_uint64), ("recorded", C.c_uint64), ("per_label", C.c_uint64 * 256)]


class Component(C.Structure):
    """volym_component (include/volym_hip.h): the record of one component, 24 bytes"""
    _fields_ = [("x", C.c_uint16), ("y", C.c_uint16), ("z", C.c_uint16), ("label", C.c_uint8), ("flags", C.c_uint8), ("count", C.c_uint32),
                ("box", C.c_uint16 * 6)]


# the summary and the record as NumPy structured dtypes (GpuContext.read_components / read_component_table, scene.components_volume)
COMPONENTS_SUMMARY_DTYPE = np.dtype([("n_components", "<u8"), ("n_solid", "<u8"), ("recorded", "<u8"), ("per_label", "<u8", (256,))])
COMPONENT_DTYPE = np.dtype([("x", "<u2"), ("y", "<u2"), ("z", "<u2"), ("label", "u1"), ("flags", "u1"), ("count", "<u4"), ("box", "<u2", (6,))])


DISTANCE_UNCUT, DISTANCE_INSIDE = 1, 2                          # volym_distance.flags
DISTANCE_WEIGHT_MAX = 64                                       # each weight is 1..64
DISTANCE_BOX_MAX = 2 ** 31 - 2                                 # most texels of a request's box
DISTANCE_NONE = 0xFFFFFFFF                                     # no seed in the box
DISTANCE_BINS = 256


class Distance(C.Structure):
    """volym_distance (include/volym_hip.h): box, flags, min_byte, select table and axis weights of one distance pass, 300 bytes"""
    _fields_ = [
        ("box", C.c_uint32 * 6),
        ("flags", C.c_uint32),
        ("min_byte", C.c_uint32),
        ("select", C.c_uint8 * 256),
        ("weight", C.c_uint32 * 3),
    ]


class DistanceSummary(C.Structure):
    """volym_distance_summary (include/volym_hip.h): counters, the deepest texel, the nearest texel per label and the histogram, 6184 bytes"""
    _fields_ = [("n_solid", C.c_uint64), ("n_present", C.c_uint64), ("n_finite", C.c_uint64), ("max_d2", C.c_uint32), ("max_at", C.c_uint32 * 3),
                ("near_d2", C.c_uint32 * 256), ("near_at", (C.c_uint32 * 3) * 256), ("hist", C.c_uint64 * 256)]


# the summary as a NumPy structured dtype (GpuContext.read_distance, scene.distance_volume)
DISTANCE_SUMMARY_DTYPE = np.dtype([("n_solid", "<u8"), ("n_present", "<u8"), ("n_finite", "<u8"), ("max_d2", "<u4"), ("max_at", "<u4", (3,)),
                                   ("near_d2", "<u4", (256,)), ("near_at", "<u4", (256, 3)), ("hist", "<u8", (256,))])


RELABEL_UNCUT, RELABEL_IDS, RELABEL_IDS_EXCEPT, RELABEL_DISTANCE, RELABEL_DRY_RUN = 1, 2, 4, 8, 16   # volym_relabel.flags


class Relabel(C.Structure):
    """volym_relabel (include/volym_hip.h): box, flags, density window, label table, id range and distance band of one edit, 308 bytes"""
    _fields_ = [
        ("box", C.c_uint32 * 6),
        ("flags", C.c_uint32),
        ("min_byte", C.c_uint32),
        ("max_byte", C.c_uint32),
        ("to", C.c_uint8 * 256),
        ("id_lo", C.c_uint32),
        ("id_hi", C.c_uint32),
        ("d2_lo", C.c_uint32),
        ("d2_hi", C.c_uint32),
    ]


class RelabelResult(C.Structure):
    """volym_relabel_result (include/volym_hip.h): texels changed, per label those that left and arrived, and their hull, 4128 bytes"""
    _fields_ = [("changed", C.c_uint64), ("left", C.c_uint64 * 256), ("arrived", C.c_uint64 * 256), ("box", C.c_uint32 * 6)]


# the result as a NumPy structured dtype (GpuContext.edit_labels, scene.relabel_volume)
RELABEL_RESULT_DTYPE = np.dtype([("changed", "<u8"), ("left", "<u8", (256,)), ("arrived", "<u8", (256,)), ("box", "<u4", (6,))])

BRUSH_UNCUT, BRUSH_DRY_RUN = 1, 16                            # volym_brush.flags: the values of their RELABEL counterparts
BRUSH_LIFT = 1                                                # volym_brush_point.flags
BRUSH_MAX_POINTS = 256


class BrushPoint(C.Structure):
    """volym_brush_point (include/volym_hip.h): a texel of the stroke and its flags, 8 bytes"""
    _fields_ = [("x", C.c_uint16), ("y", C.c_uint16), ("z", C.c_uint16), ("flags", C.c_uint16)]


class Brush(C.Structure):
    """volym_brush (include/volym_hip.h): box, flags, density window, label table, axis weights, squared radius and the points of one
    stroke, 2360 bytes"""
    _fields_ = [
        ("box", C.c_uint32 * 6),
        ("flags", C.c_uint32),
        ("min_byte", C.c_uint32),
        ("max_byte", C.c_uint32),
        ("to", C.c_uint8 * 256),
        ("weight", C.c_uint32 * 3),
        ("r2", C.c_uint32),
        ("n_points", C.c_uint32),
        ("points", BrushPoint * BRUSH_MAX_POINTS),
    ]


LASSO_UNCUT, LASSO_DRY_RUN, LASSO_OUTSIDE = 1, 16, 32         # volym_lasso.flags: UNCUT and DRY_RUN carry the values of their RELABEL counterparts
LASSO_MAX_POINTS = 1024
LASSO_MAX_FRAME = 16384
LASSO_VERTEX_MAX = 1 << 20


SMOOTH_UNCUT, SMOOTH_DRY_RUN = 1, 16                           # volym_smooth.flags: they carry the values of their RELABEL counterparts
SMOOTH_MAX_RADIUS = 3


class Smooth(C.Structure):
    """volym_smooth (include/volym_hip.h): box, flags, density window, radii and the give and take tables, 560 bytes"""
    _fields_ = [
        ("box", C.c_uint32 * 6),
        ("flags", C.c_uint32),
        ("min_byte", C.c_uint32),
        ("max_byte", C.c_uint32),
        ("radius", C.c_uint32 * 3),
        ("give", C.c_uint8 * 256),
        ("take", C.c_uint8 * 256),
    ]


NEAREST_NONE = 0xFFFFFFFF                                      # no solid texel in the box
FILL_UNCUT, FILL_DRY_RUN = 1, 2                                # volym_fill.flags


class NearestSummary(C.Structure):
    """volym_nearest_summary (include/volym_hip.h): counters and the cells per label, 4120 bytes"""
    _fields_ = [("n_solid", C.c_uint64), ("n_present", C.c_uint64), ("n_finite", C.c_uint64), ("cell", C.c_uint64 * 256), ("cell_present", C.c_uint64 * 256)]


class NearestSite(C.Structure):
    """volym_nearest_site (include/volym_hip.h): the site of one texel in volume coordinates, its d2 and its label, 20 bytes"""
    _fields_ = [("at", C.c_uint32 * 3), ("d2", C.c_uint32), ("label", C.c_uint32)]


# the summary as a NumPy structured dtype (GpuContext.read_nearest, scene.nearest_volume)
NEAREST_SUMMARY_DTYPE = np.dtype([("n_solid", "<u8"), ("n_present", "<u8"), ("n_finite", "<u8"), ("cell", "<u8", (256,)), ("cell_present", "<u8", (256,))])


class Fill(C.Structure):
    """volym_fill (include/volym_hip.h): box, flags, density window, the give and take tables and the band of one fill, 556 bytes"""
    _fields_ = [
        ("box", C.c_uint32 * 6),
        ("flags", C.c_uint32),
        ("min_byte", C.c_uint32),
        ("max_byte", C.c_uint32),
        ("give", C.c_uint8 * 256),
        ("take", C.c_uint8 * 256),
        ("d2_lo", C.c_uint32),
        ("d2_hi", C.c_uint32),
    ]


INTERPOLATE_UNCUT, INTERPOLATE_KEYS = 1, 2                      # volym_interpolate.flags
INTERPOLATE_SHAPE, INTERPOLATE_INSIDE, INTERPOLATE_GAP = 1, 2, 4   # bits of a state byte
INTERPOLATE_SLICE_OUTSIDE, INTERPOLATE_SLICE_KEY, INTERPOLATE_SLICE_GAP, INTERPOLATE_SLICE_REFUSED = 0, 1, 2, 3
INTERPOLATE_NONE = 0xFFFFFFFF                                  # no key slice, or a key slice without SHAPE
INTERPOLATE_SLICES = 4096
INTERPOLATE_EDIT_UNCUT, INTERPOLATE_EDIT_DRY_RUN = 1, 2        # volym_interpolate_edit.flags


class Interpolate(C.Structure):
    """volym_interpolate (include/volym_hip.h): box, flags, min_byte, select, weights, axis, max_gap and the key bits, 820 bytes"""
    _fields_ = [
        ("box", C.c_uint32 * 6),
        ("flags", C.c_uint32),
        ("min_byte", C.c_uint32),
        ("select", C.c_uint8 * 256),
        ("weight", C.c_uint32 * 3),
        ("axis", C.c_uint32),
        ("max_gap", C.c_uint32),
        ("keys", C.c_uint32 * (INTERPOLATE_SLICES // 32)),
    ]


class InterpolateSlice(C.Structure):
    """volym_interpolate_slice (include/volym_hip.h): the kind of one slice, the keys about it and its count, 16 bytes"""
    _fields_ = [("kind", C.c_uint32), ("key_lo", C.c_uint32), ("key_hi", C.c_uint32), ("count", C.c_uint32)]


class InterpolateSummary(C.Structure):
    """volym_interpolate_summary (include/volym_hip.h): the slice and gap counts, the texel counts and the slice records, 65592 bytes"""
    _fields_ = [("n_slices", C.c_uint32), ("n_keys", C.c_uint32), ("n_gaps", C.c_uint32), ("n_gap_slices", C.c_uint32), ("n_refused", C.c_uint32),
                ("reserved", C.c_uint32), ("n_shape", C.c_uint64), ("n_inside", C.c_uint64), ("n_new", C.c_uint64), ("n_stale", C.c_uint64),
                ("slice", InterpolateSlice * INTERPOLATE_SLICES)]


# the summary as a NumPy structured dtype (GpuContext.read_interpolate, scene.interpolate_volume)
INTERPOLATE_SLICE_DTYPE = np.dtype([("kind", "<u4"), ("key_lo", "<u4"), ("key_hi", "<u4"), ("count", "<u4")])
INTERPOLATE_SUMMARY_DTYPE = np.dtype([("n_slices", "<u4"), ("n_keys", "<u4"), ("n_gaps", "<u4"), ("n_gap_slices", "<u4"), ("n_refused", "<u4"), ("reserved", "<u4"),
                                      ("n_shape", "<u8"), ("n_inside", "<u8"), ("n_new", "<u8"), ("n_stale", "<u8"),
                                      ("slice", INTERPOLATE_SLICE_DTYPE, (INTERPOLATE_SLICES,))])


class InterpolateEdit(C.Structure):
    """volym_interpolate_edit (include/volym_hip.h): box, flags, density window and the to and out tables of one edit, 548 bytes"""
    _fields_ = [
        ("box", C.c_uint32 * 6),
        ("flags", C.c_uint32),
        ("min_byte", C.c_uint32),
        ("max_byte", C.c_uint32),
        ("to", C.c_uint8 * 256),
        ("out", C.c_uint8 * 256),
    ]


GEODESIC_UNCUT = 1                                             # volym_geodesic.flags
GEODESIC_POINTS_MAX = 64
GEODESIC_STEPS_MAX = 0xFFFFFD                                  # 2^24 - 3: the largest step count a key holds
GEODESIC_BOX_MAX = 0x7FFFFFFE
GEODESIC_NONE = 0xFFFFFFFF                                     # not reached
FLOOD_UNCUT, FLOOD_DRY_RUN = 1, 2                              # volym_flood.flags


class Geodesic(C.Structure):
    """volym_geodesic (include/volym_hip.h): box, flags, window, the seed and through tables, the step limit and the points, 1324 bytes"""
    _fields_ = [
        ("box", C.c_uint32 * 6),
        ("flags", C.c_uint32),
        ("min_byte", C.c_uint32),
        ("max_byte", C.c_uint32),
        ("seed", C.c_uint8 * 256),
        ("through", C.c_uint8 * 256),
        ("max_steps", C.c_uint32),
        ("n_points", C.c_uint32),
        ("points", (C.c_uint32 * 3) * GEODESIC_POINTS_MAX),
    ]


class GeodesicSummary(C.Structure):
    """volym_geodesic_summary (include/volym_hip.h): counters, the maximum, the cells per label and the histogram of steps, 6184 bytes"""
    _fields_ = [("n_seed", C.c_uint64), ("n_medium", C.c_uint64), ("n_reached", C.c_uint64), ("max_steps", C.c_uint32), ("max_at", C.c_uint32 * 3),
                ("cell", C.c_uint64 * 256), ("cell_medium", C.c_uint64 * 256), ("hist", C.c_uint64 * 256)]


class GeodesicSite(C.Structure):
    """volym_geodesic_site (include/volym_hip.h): the key of one texel taken apart, 8 bytes"""
    _fields_ = [("steps", C.c_uint32), ("label", C.c_uint32)]


# the summary as a NumPy structured dtype (GpuContext.read_geodesic, scene.geodesic_volume)
GEODESIC_SUMMARY_DTYPE = np.dtype([("n_seed", "<u8"), ("n_medium", "<u8"), ("n_reached", "<u8"), ("max_steps", "<u4"), ("max_at", "<u4", (3,)),
                                   ("cell", "<u8", (256,)), ("cell_medium", "<u8", (256,)), ("hist", "<u8", (256,))])


class Flood(C.Structure):
    """volym_flood (include/volym_hip.h): box, flags, density window, the give, take and to tables and the band of one flood, 812 bytes"""
    _fields_ = [
        ("box", C.c_uint32 * 6),
        ("flags", C.c_uint32),
        ("min_byte", C.c_uint32),
        ("max_byte", C.c_uint32),
        ("give", C.c_uint8 * 256),
        ("take", C.c_uint8 * 256),
        ("to", C.c_uint8 * 256),
        ("steps_lo", C.c_uint32),
        ("steps_hi", C.c_uint32),
    ]


COST_UNCUT = 1                                                 # volym_cost.flags
COST_POINTS_MAX = 64
COST_MAX = 0xFFFFFD                                            # 2^24 - 3: the largest cost a key holds
COST_STEP_MAX = 65280                                          # 255 + 255 * 255: the most one step costs
COST_BOX_MAX = 0x7FFFFFFE
COST_NONE = 0xFFFFFFFF                                         # not reached
COST_HIST_SHIFT_MAX = 16
SPREAD_UNCUT, SPREAD_DRY_RUN = 1, 2                            # volym_spread.flags


class Cost(C.Structure):
    """volym_cost (include/volym_hip.h): box, flags, window, the seed and through tables, the cost limit, the points, the two weights
    and the histogram's shift, 1336 bytes"""
    _fields_ = [
        ("box", C.c_uint32 * 6),
        ("flags", C.c_uint32),
        ("min_byte", C.c_uint32),
        ("max_byte", C.c_uint32),
        ("seed", C.c_uint8 * 256),
        ("through", C.c_uint8 * 256),
        ("max_cost", C.c_uint32),
        ("n_points", C.c_uint32),
        ("points", (C.c_uint32 * 3) * COST_POINTS_MAX),
        ("step_cost", C.c_uint32),
        ("contrast_cost", C.c_uint32),
        ("hist_shift", C.c_uint32),
    ]


class CostSummary(C.Structure):
    """volym_cost_summary (include/volym_hip.h): counters, the maximum, the cells per label and the histogram of costs, 6184 bytes"""
    _fields_ = [("n_seed", C.c_uint64), ("n_medium", C.c_uint64), ("n_reached", C.c_uint64), ("max_cost", C.c_uint32), ("max_at", C.c_uint32 * 3),
                ("cell", C.c_uint64 * 256), ("cell_medium", C.c_uint64 * 256), ("hist", C.c_uint64 * 256)]


class CostSite(C.Structure):
    """volym_cost_site (include/volym_hip.h): the key of one texel taken apart, 8 bytes"""
    _fields_ = [("cost", C.c_uint32), ("label", C.c_uint32)]


# the summary as a NumPy structured dtype (GpuContext.read_cost, scene.cost_volume)
COST_SUMMARY_DTYPE = np.dtype([("n_seed", "<u8"), ("n_medium", "<u8"), ("n_reached", "<u8"), ("max_cost", "<u4"), ("max_at", "<u4", (3,)),
                               ("cell", "<u8", (256,)), ("cell_medium", "<u8", (256,)), ("hist", "<u8", (256,))])


class Spread(C.Structure):
    """volym_spread (include/volym_hip.h): box, flags, density window, the give, take and to tables and the band of one spread, 812 bytes"""
    _fields_ = [
        ("box", C.c_uint32 * 6),
        ("flags", C.c_uint32),
        ("min_byte", C.c_uint32),
        ("max_byte", C.c_uint32),
        ("give", C.c_uint8 * 256),
        ("take", C.c_uint8 * 256),
        ("to", C.c_uint8 * 256),
        ("cost_lo", C.c_uint32),
        ("cost_hi", C.c_uint32),
    ]


class LassoView(C.Structure):
    """volym_lasso_view (include/volym_hip.h): the integer view texel -> (X, Y, D), 88 bytes"""
    _fields_ = [
        ("m", (C.c_int32 * 3) * 3),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("scale_log2", C.c_int32),
        ("c", C.c_int64 * 3),
        ("depth", C.c_int64 * 2),
    ]


class LassoPoint(C.Structure):
    """volym_lasso_point (include/volym_hip.h): a vertex of the polygon in pixels, 8 bytes"""
    _fields_ = [("x", C.c_int32), ("y", C.c_int32)]


class Lasso(C.Structure):
    """volym_lasso (include/volym_hip.h): box, flags, density window, label table, the integer view and the polygon, 8576 bytes"""
    _fields_ = [
        ("box", C.c_uint32 * 6),
        ("flags", C.c_uint32),
        ("min_byte", C.c_uint32),
        ("max_byte", C.c_uint32),
        ("to", C.c_uint8 * 256),
        ("n_points", C.c_uint32),
        ("view", LassoView),
        ("points", LassoPoint * LASSO_MAX_POINTS),
    ]


JOURNAL_RECORD_BYTES = 20     # what one journalled chunk costs of the history's budget: its index and its 16 bytes


class LabelHistoryInfo(C.Structure):
    """volym_label_history_info (include/volym_hip.h): budget and use of the label history, its steps and counters, 56 bytes"""
    _fields_ = [("budget_bytes", C.c_uint64), ("used_bytes", C.c_uint64), ("undo_steps", C.c_uint32), ("redo_steps", C.c_uint32),
                ("next_undo_records", C.c_uint64), ("next_redo_records", C.c_uint64), ("dropped_steps", C.c_uint64), ("lost", C.c_uint64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class CCamera(C.Structure):
    """src/camera.rs:5-19"""
    _fields_ = [
        ("position", C.c_float * 3),
        ("target", C.c_float * 3),
        ("up", C.c_float * 3),
        ("aspect", C.c_float),
        ("fovy", C.c_float),
        ("znear", C.c_float),
        ("zfar", C.c_float),
        ("horizontal_angle", C.c_float),
        ("vertical_angle", C.c_float),
        ("distance", C.c_float),
        ("max_distance", C.c_float),
        ("min_distance", C.c_float),
    ]


class CCameraController(C.Structure):
    """src/camera.rs:76-83"""
    _fields_ = [(n, C.c_float) for n in
                ("rotate_horizontal", "rotate_vertical", "scroll", "sensitivity", "zoom_sensitivity")]


class CStateParameters(C.Structure):
    """src/state.rs:28-39"""
    _fields_ = [
        ("camera_position", C.c_float * 3),
        ("density_trheshold", C.c_float),
        ("use_cone_importance_check", C.c_uint32),
        ("use_importance_coloring", C.c_uint32),
        ("use_opacity", C.c_uint32),
        ("use_importance_rendering", C.c_uint32),
        ("use_gaussian_smoothing", C.c_uint32),
        ("importance_check_ahead_steps", C.c_uint32),
        ("raymarching_step_size", C.c_float),
    ]


class CState(C.Structure):
    """src/state.rs:11-26 (parameter half)"""
    _fields_ = [
        ("camera", CCamera),
        ("camera_controller", CCameraController),
        ("density_threshold", C.c_float),
        ("use_importance_coloring", C.c_uint32),
        ("use_cone_importance_check", C.c_uint32),
        ("use_opacity", C.c_uint32),
        ("use_importance_rendering", C.c_uint32),
        ("use_gaussian_smoothing", C.c_uint32),
        ("importance_check_ahead_steps", C.c_uint32),
        ("raymarching_step_size", C.c_float),
    ]


_u8p = C.POINTER(C.c_uint8)
_f32p = C.POINTER(C.c_float)
_ctx = C.c_void_p

# name -> (restype, argtypes): every symbol the two headers declare
SIGNATURES = {
    # include/volym_hip.h
    "volym_create": (C.c_int, [C.POINTER(_ctx), C.c_uint32, C.c_uint32, C.c_int]),
    "volym_destroy": (None, [_ctx]),
    "volym_last_error": (C.c_char_p, [_ctx]),
    "volym_abi_version": (C.c_int, []),
    "volym_set_stream": (C.c_int, [_ctx, C.c_void_p]),
    "volym_set_option": (C.c_int, [_ctx, C.c_int, C.c_int]),
    "volym_set_shard": (C.c_int, [_ctx, C.c_uint32, C.c_uint32]),
    "volym_set_volume": (C.c_int, [_ctx, _u8p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]),
    "volym_set_importances": (C.c_int, [_ctx, _u8p, C.c_uint32, C.c_uint32, C.c_uint32]),
    "volym_set_transfer_function": (C.c_int, [_ctx, _u8p, C.c_uint32]),
    "volym_set_labels": (C.c_int, [_ctx, _u8p, C.c_uint32, C.c_uint32, C.c_uint32]),
    "volym_set_segment_importances": (C.c_int, [_ctx, _u8p]),
    "volym_label_counts": (C.c_int, [_ctx, C.POINTER(C.c_uint64)]),
    "volym_set_crop_box": (C.c_int, [_ctx, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "volym_get_crop_box": (C.c_int, [_ctx, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "volym_set_clip_plane": (C.c_int, [_ctx, C.POINTER(C.c_int32), C.c_int32]),
    "volym_get_clip_plane": (C.c_int, [_ctx, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "volym_clip_plane_box": (C.c_int, [C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                       C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "volym_set_segment_visibility": (C.c_int, [_ctx, _u8p]),
    "volym_get_segment_visibility": (C.c_int, [_ctx, _u8p]),
    "volym_visibility_boxes": (C.c_int, [_u8p, C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                         C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "volym_crop_slabs": (C.c_int, [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                   C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "volym_update": (C.c_int, [_ctx, C.POINTER(CameraUniforms), C.POINTER(ParameterUniforms)]),
    "volym_view_eye_displacement": (C.c_int, [C.POINTER(CameraUniforms), C.c_uint32, C.c_uint32, C.c_double, C.POINTER(C.c_double)]),
    "volym_compute_pass": (C.c_int, [_ctx]),
    "volym_sync": (C.c_int, [_ctx]),
    "volym_settle": (C.c_int, [_ctx]),
    "volym_throttle": (C.c_int, [_ctx, C.c_uint32]),
    "volym_blit": (C.c_int, [_ctx, C.c_void_p, C.c_uint32, C.c_uint32]),
    "volym_read_blit": (C.c_int, [_ctx, _u8p]),
    "volym_read_rgba8": (C.c_int, [_ctx, _u8p]),
    "volym_read_rgba32f": (C.c_int, [_ctx, _f32p]),
    "volym_local_tiles": (C.c_uint32, [_ctx]),
    "volym_shard_bytes": (C.c_size_t, [_ctx]),
    "volym_shard_device_ptr": (C.c_void_p, [_ctx]),
    "volym_frame_device_ptr": (C.c_void_p, [_ctx]),
    "volym_bind_output": (C.c_int, [_ctx, C.c_void_p, C.c_void_p]),
    "volym_assemble": (C.c_int, [_ctx, C.c_void_p]),
    "volym_packed_shard_bytes": (C.c_size_t, [_ctx, C.c_uint32]),
    "volym_pack_shard": (C.c_int, [_ctx, C.c_void_p, C.c_size_t]),
    "volym_packed_tiles": (C.c_int, [_ctx, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "volym_assemble_packed": (C.c_int, [_ctx, C.c_void_p, C.c_size_t]),
    "volym_read_shard": (C.c_int, [_ctx, _u8p]),
    "volym_assemble_host": (C.c_int, [_ctx, _u8p]),
    "volym_pick_pass": (C.c_int, [_ctx, C.POINTER(C.c_uint32), C.c_float]),
    "volym_read_picks": (C.c_int, [_ctx, C.POINTER(Pick)]),
    "volym_pick_device_ptr": (C.c_void_p, [_ctx]),
    "volym_pick": (C.c_int, [_ctx, C.c_uint32, C.c_uint32, C.c_float, C.POINTER(Pick)]),
    "volym_outline_pass": (C.c_int, [_ctx, C.POINTER(Outline), C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p]),
    "volym_cells_meeting_box": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "volym_bounds_cells_for": (C.c_uint32, [C.POINTER(C.c_uint32), C.c_uint32]),
    "volym_tile_bounds_size": (C.c_int, [_ctx, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "volym_read_tile_bounds": (C.c_int, [_ctx, C.POINTER(C.c_uint32), _f32p, _f32p]),
    "volym_read_outline": (C.c_int, [_ctx, _u8p]),
    "volym_outline_device_ptr": (C.c_void_p, [_ctx]),
    "volym_slice_pass": (C.c_int, [_ctx, C.POINTER(Slice), C.c_void_p]),
    "volym_read_slice": (C.c_int, [_ctx, _u8p]),
    "volym_slice_device_ptr": (C.c_void_p, [_ctx]),
    "volym_slice_check": (C.c_int, [C.POINTER(Slice)]),
    "volym_slice_axis": (C.c_int, [C.c_int, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(Slice)]),
    "volym_slice_texel": (C.c_int, [C.POINTER(Slice), C.c_uint32, C.c_uint32, C.POINTER(C.c_int32)]),
    "volym_project_pass": (C.c_int, [_ctx, C.POINTER(Project), C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p]),
    "volym_project_image_pass": (C.c_int, [_ctx, C.POINTER(Project), C.POINTER(C.c_uint32)]),
    "volym_read_projection": (C.c_int, [_ctx, C.POINTER(Projection)]),
    "volym_read_projection_image": (C.c_int, [_ctx, _u8p]),
    "volym_projection_device_ptr": (C.c_void_p, [_ctx]),
    "volym_projection_image_device_ptr": (C.c_void_p, [_ctx]),
    "volym_projection_size": (C.c_int, [_ctx, C.POINTER(C.c_uint32)]),
    "volym_projection_image_size": (C.c_int, [_ctx, C.POINTER(C.c_uint32)]),
    "volym_project_at": (C.c_int, [_ctx, C.c_uint32, C.c_uint32, C.c_float, C.POINTER(Projection)]),
    "volym_project_check": (C.c_int, [C.POINTER(Project)]),
    "volym_project_samples": (C.c_int, [C.c_float, C.c_float, C.c_float, C.POINTER(C.c_uint32)]),
    "volym_measure_pass": (C.c_int, [_ctx, C.POINTER(Measure)]),
    "volym_read_measure": (C.c_int, [_ctx, C.POINTER(Measurement)]),
    "volym_measure_device_ptr": (C.c_void_p, [_ctx]),
    "volym_measure_check": (C.c_int, [C.POINTER(Measure), C.POINTER(C.c_uint32)]),
    "volym_surface_pass": (C.c_int, [_ctx, C.POINTER(Surface)]),
    "volym_read_surface": (C.c_int, [_ctx, C.POINTER(SurfaceSummary)]),
    "volym_surface_device_ptr": (C.c_void_p, [_ctx]),
    "volym_surface_faces_pass": (C.c_int, [_ctx, C.c_void_p, C.c_uint64]),
    "volym_read_surface_faces": (C.c_int, [_ctx, C.POINTER(SurfaceFace), C.c_uint64]),
    "volym_surface_check": (C.c_int, [C.POINTER(Surface), C.POINTER(C.c_uint32)]),
    "volym_components_pass": (C.c_int, [_ctx, C.POINTER(Components)]),
    "volym_components_check": (C.c_int, [C.POINTER(Components), C.POINTER(C.c_uint32)]),
    "volym_read_components": (C.c_int, [_ctx, C.POINTER(ComponentsSummary)]),
    "volym_read_component_table": (C.c_int, [_ctx, C.POINTER(Component), C.c_uint64]),
    "volym_read_component_ids": (C.c_int, [_ctx, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "volym_component_of": (C.c_int, [_ctx, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]),
    "volym_components_device_ptr": (C.c_void_p, [_ctx]),
    "volym_component_ids_device_ptr": (C.c_void_p, [_ctx]),
    "volym_component_table_device_ptr": (C.c_void_p, [_ctx]),
    "volym_distance_pass": (C.c_int, [_ctx, C.POINTER(Distance)]),
    "volym_distance_check": (C.c_int, [C.POINTER(Distance), C.POINTER(C.c_uint32)]),
    "volym_read_distance": (C.c_int, [_ctx, C.POINTER(DistanceSummary)]),
    "volym_read_distance_map": (C.c_int, [_ctx, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "volym_distance_at": (C.c_int, [_ctx, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]),
    "volym_distance_device_ptr": (C.c_void_p, [_ctx]),
    "volym_distance_map_device_ptr": (C.c_void_p, [_ctx]),
    "volym_edit_labels": (C.c_int, [_ctx, C.POINTER(Relabel), C.POINTER(RelabelResult)]),
    "volym_relabel_check": (C.c_int, [C.POINTER(Relabel), C.POINTER(C.c_uint32)]),
    "volym_read_labels": (C.c_int, [_ctx, C.POINTER(C.c_uint32), _u8p]),
    "volym_label_history": (C.c_int, [_ctx, C.c_uint64]),
    "volym_undo_labels": (C.c_int, [_ctx, C.POINTER(RelabelResult)]),
    "volym_redo_labels": (C.c_int, [_ctx, C.POINTER(RelabelResult)]),
    "volym_label_history_info": (C.c_int, [_ctx, C.POINTER(LabelHistoryInfo)]),
    "volym_brush_labels": (C.c_int, [_ctx, C.POINTER(Brush), C.POINTER(RelabelResult)]),
    "volym_brush_check": (C.c_int, [C.POINTER(Brush), C.POINTER(C.c_uint32)]),
    "volym_brush_box": (C.c_int, [C.POINTER(Brush), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "volym_lasso_labels": (C.c_int, [_ctx, C.POINTER(Lasso), C.POINTER(RelabelResult)]),
    "volym_lasso_check": (C.c_int, [C.POINTER(Lasso), C.POINTER(C.c_uint32)]),
    "volym_lasso_rect": (C.c_int, [C.POINTER(Lasso), C.POINTER(C.c_uint32)]),
    "volym_read_lasso_mask": (C.c_int, [_ctx, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint64]),
    "volym_lasso_view_from_camera": (C.c_int, [C.POINTER(CameraUniforms), C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.c_double, C.POINTER(LassoView)]),
    "volym_lasso_view_depth": (C.c_int, [C.POINTER(LassoView), C.c_double, C.c_double]),
    "volym_smooth_labels": (C.c_int, [_ctx, C.POINTER(Smooth), C.POINTER(RelabelResult)]),
    "volym_smooth_check": (C.c_int, [C.POINTER(Smooth), C.POINTER(C.c_uint32)]),
    "volym_nearest_pass": (C.c_int, [_ctx, C.POINTER(Distance)]),
    "volym_nearest_check": (C.c_int, [C.POINTER(Distance), C.POINTER(C.c_uint32)]),
    "volym_read_nearest": (C.c_int, [_ctx, C.POINTER(NearestSummary)]),
    "volym_read_nearest_sites": (C.c_int, [_ctx, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "volym_read_nearest_labels": (C.c_int, [_ctx, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)]),
    "volym_nearest_at": (C.c_int, [_ctx, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(NearestSite)]),
    "volym_nearest_device_ptr": (C.c_void_p, [_ctx]),
    "volym_nearest_sites_device_ptr": (C.c_void_p, [_ctx]),
    "volym_nearest_labels_device_ptr": (C.c_void_p, [_ctx]),
    "volym_fill_labels": (C.c_int, [_ctx, C.POINTER(Fill), C.POINTER(RelabelResult)]),
    "volym_fill_check": (C.c_int, [C.POINTER(Fill), C.POINTER(C.c_uint32)]),
    "volym_geodesic_pass": (C.c_int, [_ctx, C.POINTER(Geodesic)]),
    "volym_geodesic_check": (C.c_int, [C.POINTER(Geodesic), C.POINTER(C.c_uint32)]),
    "volym_read_geodesic": (C.c_int, [_ctx, C.POINTER(GeodesicSummary)]),
    "volym_read_geodesic_map": (C.c_int, [_ctx, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "volym_geodesic_at": (C.c_int, [_ctx, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(GeodesicSite)]),
    "volym_geodesic_device_ptr": (C.c_void_p, [_ctx]),
    "volym_geodesic_map_device_ptr": (C.c_void_p, [_ctx]),
    "volym_flood_labels": (C.c_int, [_ctx, C.POINTER(Flood), C.POINTER(RelabelResult)]),
    "volym_flood_check": (C.c_int, [C.POINTER(Flood), C.POINTER(C.c_uint32)]),
    "volym_cost_pass": (C.c_int, [_ctx, C.POINTER(Cost)]),
    "volym_cost_check": (C.c_int, [C.POINTER(Cost), C.POINTER(C.c_uint32)]),
    "volym_read_cost": (C.c_int, [_ctx, C.POINTER(CostSummary)]),
    "volym_read_cost_map": (C.c_int, [_ctx, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "volym_cost_at": (C.c_int, [_ctx, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(CostSite)]),
    "volym_cost_device_ptr": (C.c_void_p, [_ctx]),
    "volym_cost_map_device_ptr": (C.c_void_p, [_ctx]),
    "volym_spread_labels": (C.c_int, [_ctx, C.POINTER(Spread), C.POINTER(RelabelResult)]),
    "volym_spread_check": (C.c_int, [C.POINTER(Spread), C.POINTER(C.c_uint32)]),
    "volym_interpolate_pass": (C.c_int, [_ctx, C.POINTER(Interpolate)]),
    "volym_interpolate_check": (C.c_int, [C.POINTER(Interpolate), C.POINTER(C.c_uint32)]),
    "volym_read_interpolate": (C.c_int, [_ctx, C.POINTER(InterpolateSummary)]),
    "volym_read_interpolate_map": (C.c_int, [_ctx, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "volym_read_interpolate_state": (C.c_int, [_ctx, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)]),
    "volym_interpolate_at": (C.c_int, [_ctx, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)]),
    "volym_interpolate_device_ptr": (C.c_void_p, [_ctx]),
    "volym_interpolate_map_device_ptr": (C.c_void_p, [_ctx]),
    "volym_interpolate_state_device_ptr": (C.c_void_p, [_ctx]),
    "volym_interpolate_labels": (C.c_int, [_ctx, C.POINTER(InterpolateEdit), C.POINTER(RelabelResult)]),
    "volym_interpolate_labels_check": (C.c_int, [C.POINTER(InterpolateEdit), C.POINTER(C.c_uint32)]),
    "volym_stats_pass": (C.c_int, [_ctx, C.POINTER(Stats)]),
    "volym_time_passes": (C.c_int, [_ctx, C.c_uint32, _f32p]),
    "volym_time_batch": (C.c_int, [_ctx, C.c_uint32, _f32p]),
    "volym_selftest_ray_setup": (C.c_int, [_ctx, C.POINTER(C.c_ulonglong)]),
    "volym_selftest_texel256": (C.c_int, [_ctx, C.POINTER(C.c_ulonglong)]),
    "volym_texel_bytes_in_use": (C.c_int, [_ctx]),
    # include/volym_host.h
    "volym_camera_default_with_aspect_and_pos": (None, [C.POINTER(CCamera), C.c_float, _f32p]),
    "volym_camera_orbit": (None, [C.POINTER(CCamera), C.c_float, C.c_float, C.c_float]),
    "volym_camera_view_matrix": (None, [C.POINTER(CCamera), _f32p]),
    "volym_camera_projection_matrix": (None, [C.POINTER(CCamera), _f32p]),
    "volym_camera_uniforms_from": (C.c_int, [C.POINTER(CCamera), C.POINTER(CameraUniforms)]),
    "volym_camera_controller_new": (None, [C.POINTER(CCameraController), C.c_float, C.c_float]),
    "volym_camera_controller_process_mouse": (None, [C.POINTER(CCameraController), C.c_double, C.c_double]),
    "volym_camera_controller_process_scroll": (None, [C.POINTER(CCameraController), C.c_float]),
    "volym_camera_controller_update_camera": (None, [C.POINTER(CCameraController), C.POINTER(CCamera)]),
    "volym_state_parameters_default": (None, [C.POINTER(CStateParameters)]),
    "volym_state_parameters_benchmark": (None, [C.POINTER(CStateParameters)]),
    "volym_state_with_parameters": (None, [C.POINTER(CState), C.c_float, C.POINTER(CStateParameters)]),
    "volym_state_update": (None, [C.POINTER(CState)]),
    "volym_parameter_uniforms_from": (C.c_int, [C.POINTER(CState), C.POINTER(ParameterUniforms)]),
    "volym_transfer_function_default_lut": (None, [_u8p]),
    "volym_transfer_function_bake": (C.c_int, [_f32p, C.c_uint32, _f32p, C.c_uint32, _u8p]),
    "volym_prepare_volume": (C.c_int, [_u8p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, _u8p]),
    "volym_map_segments_to_importance": (C.c_int, [_u8p, C.c_size_t, _u8p, _u8p, C.c_uint32]),
    "volym_synth_bonsai": (C.c_int, [C.c_uint32, C.c_uint32, _u8p, _u8p]),
    "volym_synth_teapot": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _u8p, _u8p]),
}

_lib = None


def lib():
    """Load libvolym_hip.so.  Fails loudly when it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C volym_amd/csrc` (hipcc --offload-arch=gfx950)" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)       # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc, ctx=None):
    if rc != OK:
        msg = lib().volym_last_error(ctx)
        raise VolymError(rc, msg.decode() if msg else "")
    return rc
