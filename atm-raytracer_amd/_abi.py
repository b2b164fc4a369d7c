"""ctypes mirror of include/atmrt.h (the C ABI of the HIP library).

Field order and types must match the header exactly; tests/test_abi.py checks sizeof() of every
struct against the compiled library (atmrt_abi_sizeof).
"""
import ctypes as C

TEMP_LINEAR, TEMP_SPLINE = 0, 1
SPLINE_BOUNDARY = {"Natural": 0, "Derivatives": 1, "SecondDerivatives": 2}

# atmrt_status
OK, ERR_INVALID_ARGUMENT, ERR_NO_DEVICE, ERR_HIP, ERR_IO, ERR_FORMAT, ERR_STATE, ERR_UNSUPPORTED = 0, -1, -2, -3, -4, -5, -6, -7

# atmrt_earth_kind  (EarthModel, src/utils/earth_model/mod.rs:19-28)
EARTH_KINDS = {
    "SimpleSphere": 0, "Spherical": 1, "Ellipsoid": 2, "Wgs84": 3,
    "AzimuthalEquidistant": 4, "FlatDistorted": 5, "ObserverAe": 6, "SimpleObserverAe": 7,
}
ALT_ABSOLUTE, ALT_RELATIVE = 0, 1
# atmrt_generator_kind (GeneratorDef, params.rs:387-392)
GENERATORS = {"Fast": 0, "InterpolatingRectilinear": 1, "Rectilinear": 2}
OBJ_FRUSTUM, OBJ_BILLBOARD = 0, 1
COLOR_TERRAIN, COLOR_RGBA = 0, 1


class EarthModel(C.Structure):
    _fields_ = [("kind", C.c_int32), ("_pad", C.c_int32), ("radius", C.c_double), ("a", C.c_double), ("b", C.c_double)]


class Position(C.Structure):
    _fields_ = [("latitude", C.c_double), ("longitude", C.c_double), ("altitude_kind", C.c_int32), ("_pad", C.c_int32),
                ("altitude", C.c_double)]


class Frame(C.Structure):
    _fields_ = [("direction", C.c_double), ("tilt", C.c_double), ("fov", C.c_double), ("max_distance", C.c_double)]


class Params(C.Structure):
    _fields_ = [("position", Position), ("frame", Frame), ("earth", EarthModel), ("wavelength", C.c_double),
                ("simulation_step", C.c_double), ("terrain_alpha", C.c_double), ("straight_rays", C.c_int32),
                ("generator", C.c_int32), ("width", C.c_uint16), ("height", C.c_uint16), ("col_begin", C.c_uint16),
                ("col_end", C.c_uint16)]


class TempFunction(C.Structure):
    """atmrt_temp_function_t.  The spline points are borrowed pointers: set them with set_points(), which keeps the arrays alive
    on the owning Atmosphere."""
    _fields_ = [("kind", C.c_int32), ("boundary", C.c_int32), ("altitude", C.c_double), ("gradient", C.c_double),
                ("bc", C.c_double * 2), ("n_points", C.c_int32), ("_pad", C.c_int32),
                ("point_altitude", C.POINTER(C.c_double)), ("point_temperature", C.POINTER(C.c_double))]


class Atmosphere(C.Structure):
    """atmrt_atmosphere_t: any number of temperature functions, any number of spline points (pointer + count, like the `Vec`s
    of AtmosphereDef).  Build with Atmosphere.new(n): the function table and the point arrays are owned by the Python object."""
    _fields_ = [("pressure_altitude", C.c_double), ("pressure", C.c_double), ("temperature_altitude", C.c_double),
                ("temperature", C.c_double), ("has_temperature_fixed_point", C.c_int32), ("n_functions", C.c_int32),
                ("functions", C.POINTER(TempFunction))]

    @classmethod
    def new(cls, n_functions):
        a = cls()
        a._table = (TempFunction * max(1, n_functions))()
        a._points = []
        a.functions = C.cast(a._table, C.POINTER(TempFunction))
        a.n_functions = n_functions
        return a

    def set_points(self, k, altitudes, temperatures):
        n = len(altitudes)
        xa, ya = (C.c_double * n)(*[float(v) for v in altitudes]), (C.c_double * n)(*[float(v) for v in temperatures])
        self._points.append((xa, ya))
        fn = self.functions[k]
        fn.n_points = n
        fn.point_altitude, fn.point_temperature = C.cast(xa, C.POINTER(C.c_double)), C.cast(ya, C.POINTER(C.c_double))


class Object(C.Structure):
    _fields_ = [("kind", C.c_int32), ("_pad", C.c_int32), ("position", Position), ("r1", C.c_double), ("r2", C.c_double),
                ("height", C.c_double), ("width", C.c_double), ("color", C.c_double * 4),
                ("texture_rgba", C.POINTER(C.c_uint8)), ("texture_width", C.c_uint32), ("texture_height", C.c_uint32)]


class Result(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("n_pixels", C.c_uint64), ("n_hits", C.c_uint64),
                ("azimuth", C.POINTER(C.c_double)), ("elevation_angle", C.POINTER(C.c_double)),
                ("hit_count", C.POINTER(C.c_uint32)), ("hit_offset", C.POINTER(C.c_uint64)),
                ("lat", C.POINTER(C.c_double)), ("lon", C.POINTER(C.c_double)), ("distance", C.POINTER(C.c_double)),
                ("elevation", C.POINTER(C.c_double)), ("path_length", C.POINTER(C.c_double)),
                ("normal", C.POINTER(C.c_double)), ("color_tag", C.POINTER(C.c_uint32)), ("rgba", C.POINTER(C.c_double)),
                ("ray_steps", C.c_uint64), ("device_ms", C.c_double)]


class DevicePlanes(C.Structure):
    _fields_ = [("azimuth", C.c_void_p), ("elevation_angle", C.c_void_p), ("hit_count", C.c_void_p), ("lat", C.c_void_p),
                ("lon", C.c_void_p), ("distance", C.c_void_p), ("elevation", C.c_void_p), ("path_length", C.c_void_p),
                ("normal", C.c_void_p)]


class DeviceHits(C.Structure):
    _fields_ = [("capacity", C.c_uint64), ("hit_offset", C.c_void_p), ("lat", C.c_void_p), ("lon", C.c_void_p), ("distance", C.c_void_p),
                ("elevation", C.c_void_p), ("path_length", C.c_void_p), ("normal", C.c_void_p), ("color_tag", C.c_void_p),
                ("rgba", C.c_void_p)]


class Coloring(C.Structure):
    _fields_ = [("kind", C.c_int32), ("palette", C.c_int32), ("water_level", C.c_double), ("max_distance", C.c_double),
                ("ambient_light", C.c_double), ("light_dir", C.c_double * 3), ("has_fog", C.c_int32), ("_pad", C.c_int32),
                ("fog_distance", C.c_double)]


COLORING_SIMPLE, COLORING_SHADING = 0, 1
PALETTES = {"Legacy": 0, "Improved": 1}

# atmrt_tick_kind
TICK_SINGLE, TICK_MULTIPLE = 0, 1
TICK_LABEL_BYTES = 32


class Tick(C.Structure):
    _fields_ = [("kind", C.c_int32), ("size", C.c_uint32), ("angle", C.c_double), ("bias", C.c_double), ("step", C.c_double),
                ("labelled", C.c_int32), ("_pad", C.c_int32)]


class Overlay(C.Structure):
    """atmrt_overlay_t.  The tick arrays are borrowed pointers: build with Overlay.new(), which keeps them alive on the object."""
    _fields_ = [("ticks", C.POINTER(Tick)), ("vertical_ticks", C.POINTER(Tick)), ("n_ticks", C.c_uint32), ("n_vertical_ticks", C.c_uint32),
                ("show_eye_level", C.c_int32), ("show_flat_horizon", C.c_int32)]

    @classmethod
    def new(cls, ticks=(), vertical_ticks=(), show_eye_level=False, show_flat_horizon=False):
        o = cls()
        o._arrays = ((Tick * max(1, len(ticks)))(*ticks), (Tick * max(1, len(vertical_ticks)))(*vertical_ticks))
        o.ticks, o.vertical_ticks = C.cast(o._arrays[0], C.POINTER(Tick)), C.cast(o._arrays[1], C.POINTER(Tick))
        o.n_ticks, o.n_vertical_ticks = len(ticks), len(vertical_ticks)
        o.show_eye_level, o.show_flat_horizon = int(bool(show_eye_level)), int(bool(show_flat_horizon))
        return o


class DrawnTick(C.Structure):
    _fields_ = [("pos", C.c_uint32), ("size", C.c_uint32), ("labelled", C.c_int32), ("vertical", C.c_int32),
                ("label", C.c_char * TICK_LABEL_BYTES)]


# atmrt_visibility_mode
VIS_FIRST, VIS_ALL = 0, 1
VIS_MODES = {"first": VIS_FIRST, "all": VIS_ALL}


class GeoGrid(C.Structure):
    """atmrt_geo_grid_t: cell (i, j) covers [lat0 + i cell_lat, + cell_lat) x [lon0 + j cell_lon, + cell_lon), plain degrees."""
    _fields_ = [("lat0", C.c_double), ("lon0", C.c_double), ("cell_lat", C.c_double), ("cell_lon", C.c_double),
                ("n_lat", C.c_uint32), ("n_lon", C.c_uint32)]


class VisibilityStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("n_points", "n_binned", "n_outside", "n_skipped", "n_updates")]


class Landmark(C.Structure):
    """atmrt_landmark_t: degrees, and what a degree of longitude is worth against a degree of latitude there (1e-6 .. 1)."""
    _fields_ = [("lat", C.c_double), ("lon", C.c_double), ("lon_scale", C.c_double)]


class LandmarkHit(C.Structure):
    _fields_ = [("n_within", C.c_uint32), ("x", C.c_uint32), ("y", C.c_uint32), ("point", C.c_uint32), ("d2", C.c_double),
                ("distance", C.c_double), ("elevation", C.c_double)]


class LandmarkStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("n_points", "n_skipped", "n_tested", "n_within")]


# atmrt_sight_status
SIGHT_SEEN, SIGHT_HIDDEN, SIGHT_ABOVE_FAN, SIGHT_BELOW_FAN = 0, 1, 2, 3
SIGHT_STATUS = {SIGHT_SEEN: "seen", SIGHT_HIDDEN: "hidden", SIGHT_ABOVE_FAN: "above_fan", SIGHT_BELOW_FAN: "below_fan"}


class SightTarget(C.Structure):
    """atmrt_sight_target_t: azimuth [deg], surface distance [m] (> 0), metres above the ground at the target (>= 0)."""
    _fields_ = [("azimuth_deg", C.c_double), ("distance", C.c_double), ("height", C.c_double)]


class Sight(C.Structure):
    _fields_ = [("status", C.c_int32), ("rounds_done", C.c_int32), ("m", C.c_int32), ("block_index", C.c_int32)] + \
        [(k, C.c_double) for k in ("angle", "arrival", "ground", "hidden", "resolution", "block_distance", "block_lat", "block_lon",
                                   "block_elevation")]


class SightRay(C.Structure):
    _fields_ = [("block_index", C.c_int32), ("min_index", C.c_int32), ("arrival", C.c_double), ("min_clearance", C.c_double)]


class ViewshedSpec(C.Structure):
    """atmrt_viewshed_spec_t: the azimuths, the reach [m], the height above the ground [m], the fan [deg] and its rays."""
    _fields_ = [(k, C.c_double) for k in ("az_lo_deg", "az_step_deg", "reach", "height", "fan_lo_deg", "fan_hi_deg")] + \
        [("n_az", C.c_int32), ("fan_rays", C.c_int32)]


class ViewshedMapStats(C.Structure):
    """atmrt_viewshed_map_stats_t: n_samples = n_binned + n_outside + n_skipped, of one call."""
    _fields_ = [(k, C.c_uint64) for k in ("n_samples", "n_binned", "n_outside", "n_skipped", "n_seen")]


# atmrt_horizon_status: the last two have the values of the sight statuses of the same meaning
HORIZON_FOUND, HORIZON_ABOVE_FAN, HORIZON_BELOW_FAN = 0, SIGHT_ABOVE_FAN, SIGHT_BELOW_FAN
HORIZON_STATUS = {HORIZON_FOUND: "found", HORIZON_ABOVE_FAN: "above_fan", HORIZON_BELOW_FAN: "below_fan"}


class HorizonSpec(C.Structure):
    """atmrt_horizon_spec_t: the azimuths, the reach [m], the first fan [deg] and its rays, and the rounds."""
    _fields_ = [(k, C.c_double) for k in ("az_lo_deg", "az_step_deg", "reach", "fan_lo_deg", "fan_hi_deg")] + \
        [("n_az", C.c_int32), ("fan_rays", C.c_int32), ("rounds", C.c_int32)]


# atmrt_shadow_status
SHADOW_NONE, SHADOW_LIT, SHADOW_SHADOWED = 0, 1, 2


class ShadowSpec(C.Structure):
    """atmrt_shadow_spec_t: the direction toward the light and the shadow ray's launch elevation [deg], the reach and the lift [m]."""
    _fields_ = [(k, C.c_double) for k in ("azimuth_deg", "elevation_deg", "reach", "lift")]


class ShadowStats(C.Structure):
    """atmrt_shadow_stats_t: none + lit + shadowed = the pixels; the stepper steps taken and the rays that escaped, of one call."""
    _fields_ = [(k, C.c_uint64) for k in ("none", "lit", "shadowed", "integrated_steps", "escaped_rays")]


class ShadowLightsSpec(C.Structure):
    """atmrt_shadow_lights_spec_t: the lights (world-frame vectors [n_lights][3], host memory), the reach and the lift [m]."""
    _fields_ = [("dir", C.POINTER(C.c_double)), ("n_lights", C.c_uint32), ("_pad", C.c_uint32), ("reach", C.c_double), ("lift", C.c_double)]


# atmrt_sky_status
SKY_NONE, SKY_EXIT, SKY_GROUND, SKY_INSIDE, SKY_LOST = 0, 1, 2, 3, 4
SKY_STATUS = {SKY_NONE: "none", SKY_EXIT: "exit", SKY_GROUND: "ground", SKY_INSIDE: "inside", SKY_LOST: "lost"}
SKY_M_MAX, SKY_BODIES_MAX = 1048575, 32


class SkySpec(C.Structure):
    """atmrt_sky_spec_t: the step [m] (0: the context's simulation_step), the top and the floor [m], the step cap."""
    _fields_ = [("step", C.c_double), ("top", C.c_double), ("floor", C.c_double), ("m", C.c_int32), ("_pad", C.c_int32)]


class SkyRay(C.Structure):
    """atmrt_sky_ray_t: status (SKY_*), the deciding step, the true elevation [deg] (NaN unless EXIT)."""
    _fields_ = [("status", C.c_int32), ("steps", C.c_uint32), ("true_elevation", C.c_double)]


class SkyStats(C.Structure):
    """atmrt_sky_stats_t: none + exit + ground + inside + lost = the pixels; the stepper steps taken, of one call."""
    _fields_ = [(k, C.c_uint64) for k in ("none", "exit", "ground", "inside", "lost", "integrated_steps")]


class SkyBody(C.Structure):
    """atmrt_sky_body_t: the body's true direction and angular radius [deg], its colour."""
    _fields_ = [("azimuth_deg", C.c_double), ("elevation_deg", C.c_double), ("radius_deg", C.c_double), ("rgb", C.c_uint8 * 3),
                ("_pad", C.c_uint8 * 5)]


class SkyLightSpec(C.Structure):
    """atmrt_sky_light_spec_t: the sky spec of the march, the altitude whose zenith is air mass 1 [m], the node spacing of the zenith
    column [m] (0: the step of the march)."""
    _fields_ = [("sky", SkySpec), ("ref_alt", C.c_double), ("column_dz", C.c_double)]


class SkyShade(C.Structure):
    """atmrt_sky_shade_t: the zenith column [m], the zenith optical depth and the limb-darkening coefficient per channel, the
    exposure and the colour of the airlight."""
    _fields_ = [("zenith_column", C.c_double), ("tau", C.c_double * 3), ("limb", C.c_double * 3), ("exposure", C.c_double),
                ("airlight", C.c_uint8 * 3), ("_pad", C.c_uint8 * 5)]


SKY_COLUMN_NODES_MAX = 1048575
SKY_TABLE_ALT_MAX, SKY_TABLE_EL_MAX, SKY_TABLE_ENTRIES_MAX = 1024, 65536, 1 << 24


class SkyTableSpec(C.Structure):
    """atmrt_sky_table_spec_t: the sky spec of the table's rays, its altitudes [m] and launch elevations [deg], its shape."""
    _fields_ = [("sky", SkySpec)] + [(k, C.c_double) for k in ("alt_lo", "alt_hi", "el_lo", "el_hi")] + [("n_alt", C.c_uint32), ("n_el", C.c_uint32)]


class Horizon(C.Structure):
    _fields_ = [("status", C.c_int32), ("rounds_done", C.c_int32), ("k_star", C.c_int32), ("block_index", C.c_int32)] + \
        [(k, C.c_double) for k in ("angle_clear", "angle_blocked", "resolution", "block_distance", "block_lat", "block_lon", "block_elevation")]


class InterpLattice(C.Structure):
    """atmrt_interp_lattice_t: the lattice atmrt_debug_interp_blend blends, host arrays (borrowed: build with interp_lattice())."""
    _fields_ = [("ne", C.c_int32), ("nd", C.c_int32), ("n_hits", C.c_uint64),
                ("hit_count", C.POINTER(C.c_uint32)), ("azimuth", C.POINTER(C.c_double)), ("elevation_angle", C.POINTER(C.c_double)),
                ("px_steps", C.POINTER(C.c_uint32)),
                ("lat", C.POINTER(C.c_double)), ("lon", C.POINTER(C.c_double)), ("distance", C.POINTER(C.c_double)),
                ("elevation", C.POINTER(C.c_double)), ("path_length", C.POINTER(C.c_double)), ("normal", C.POINTER(C.c_double)),
                ("color_tag", C.POINTER(C.c_uint32)), ("rgba", C.POINTER(C.c_double))]


def interp_lattice(lat):
    """An atmrt_interp_lattice_t over the arrays of the dict `lat` (hit_count, azimuth, elevation_angle, px_steps: [ne][nd]; lat, lon,
    distance, elevation, path_length [n], normal [n][3], color_tag [n], rgba [n][4]) and the arrays it borrows (keep them alive)."""
    import numpy as np
    r = InterpLattice()
    keep = {}

    def ptr(key, dtype, ctype):
        a = np.ascontiguousarray(lat[key], dtype=dtype)
        if a.size == 0:
            a = np.zeros(1, dtype=dtype)
        keep[key] = a
        return a.ctypes.data_as(C.POINTER(ctype))

    r.ne, r.nd = np.shape(lat["hit_count"])
    r.n_hits = int(np.size(lat["distance"]))
    for k in ("hit_count", "px_steps", "color_tag"):
        setattr(r, k, ptr(k, np.uint32, C.c_uint32))
    for k in ("azimuth", "elevation_angle", "lat", "lon", "distance", "elevation", "path_length", "normal", "rgba"):
        setattr(r, k, ptr(k, np.float64, C.c_double))
    return r, keep


def numpy_to_result(res):
    """Inverse of result_to_numpy: an atmrt_result_t whose pointers borrow the numpy arrays (keep `res` alive)."""
    import numpy as np
    r = Result()
    keep = {}

    def ptr(key, dtype, ctype):
        a = np.ascontiguousarray(res[key], dtype=dtype)
        if a.size == 0:
            a = np.zeros(1, dtype=dtype)
        keep[key] = a
        return a.ctypes.data_as(C.POINTER(ctype))

    r.width, r.height = int(res["width"]), int(res["height"])
    r.n_pixels, r.n_hits = r.width * r.height, int(res["n_hits"])
    r.azimuth, r.elevation_angle = ptr("azimuth", np.float64, C.c_double), ptr("elevation_angle", np.float64, C.c_double)
    r.hit_count, r.hit_offset = ptr("hit_count", np.uint32, C.c_uint32), ptr("hit_offset", np.uint64, C.c_uint64)
    for k in ("lat", "lon", "distance", "elevation", "path_length", "normal", "rgba"):
        setattr(r, k, ptr(k, np.float64, C.c_double))
    r.color_tag = ptr("color_tag", np.uint32, C.c_uint32)
    r.ray_steps = int(res["ray_steps"])
    return r, keep


class CommTimings(C.Structure):
    _fields_ = [("gather_ms", C.c_double), ("assemble_ms", C.c_double), ("tile_ms_max", C.c_double), ("tile_ms_min", C.c_double),
                ("bytes_per_rank", C.c_uint64), ("world", C.c_int32), ("route", C.c_int32), ("collectives", C.c_int32), ("_pad", C.c_int32)]


ROUTES = {0: "none", 1: "rccl", 2: "peer", 3: "external", 4: "host", 5: "external-device"}
COMM_ID_BYTES = 128
# atmrt_all_gather_fn(user, send_host, recv_host, bytes_per_rank) -> int
ALL_GATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)


class Timings(C.Structure):
    _fields_ = [("total_ms", C.c_double), ("profile_ms", C.c_double), ("paths_ms", C.c_double), ("intersect_ms", C.c_double),
                ("march_ms", C.c_double), ("finalize_ms", C.c_double), ("pack_ms", C.c_double), ("ray_steps", C.c_uint64),
                ("n_hits", C.c_uint64), ("ceiling_ms", C.c_double)]


class FrameStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("unlisted_rays", "unlisted_columns", "retraced_pixels", "big_steps", "big_blend_pixels", "terrain_lookups", "object_rays", "object_steps")]


def result_to_numpy(res):
    """Copy an atmrt_result_t (library-owned) into a dict of numpy arrays."""
    import numpy as np

    n_px, n_hits = int(res.n_pixels), int(res.n_hits)

    def arr(ptr, n, dtype):
        if n == 0:
            return np.zeros(0, dtype=dtype)
        return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dtype, copy=True)

    h, w = int(res.height), int(res.width)
    out = {
        "width": w, "height": h, "n_hits": n_hits, "ray_steps": int(res.ray_steps), "device_ms": float(res.device_ms),
        "azimuth": arr(res.azimuth, n_px, np.float64).reshape(h, w),
        "elevation_angle": arr(res.elevation_angle, n_px, np.float64).reshape(h, w),
        "hit_count": arr(res.hit_count, n_px, np.uint32).reshape(h, w),
        "hit_offset": arr(res.hit_offset, n_px, np.uint64).reshape(h, w),
        "lat": arr(res.lat, n_hits, np.float64), "lon": arr(res.lon, n_hits, np.float64),
        "distance": arr(res.distance, n_hits, np.float64), "elevation": arr(res.elevation, n_hits, np.float64),
        "path_length": arr(res.path_length, n_hits, np.float64),
        "normal": arr(res.normal, 3 * n_hits, np.float64).reshape(n_hits, 3),
        "color_tag": arr(res.color_tag, n_hits, np.uint32),
        "rgba": arr(res.rgba, 4 * n_hits, np.float64).reshape(n_hits, 4),
    }
    return out
