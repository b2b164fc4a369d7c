"""The rule of include/atmrt.h, "sky rays", restated over the oracle's ray stepper (driven through ctypes, as tests/shadow_model.py
drives it) and the host build of detmath.h's atan2 / sincos (tests/cbuild.dm_export).  Test infrastructure only: what
atmrt_sky_ray_host, atmrt_sky_rays, atmrt_sky_directions* and atmrt_sky_bodies* must return, byte for byte.  The arithmetic is Python's
float: IEEE doubles, every operation rounded on its own."""
import ctypes as C
import math

import numpy as np

from atm_raytracer_amd import _abi
from shadow_lights_model import DEG_PER_RAD, RAD_PER_DEG, dm_atan2, dm_sincos
from shadow_model import _RayState, _Stepper

NONE, EXIT, GROUND, INSIDE, LOST = 0, 1, 2, 3, 4
M_MAX, BODIES_MAX = 1048575, 32
NAN = float("nan")


class Setting:
    """What the rule reads of a context's setting, on the oracle's side: the shape of the earth model, straight_rays and the
    compiled atmosphere.  earth: an _abi.EarthModel; atm: an _abi.Atmosphere (None: US-76)."""

    def __init__(self, oracle, earth, straight=False, atm=None, wavelength=530e-9):
        self.o = oracle
        self.env = oracle.env(atm, wavelength)
        self.straight = bool(straight)
        L = oracle.lib
        L.oracle_to_shape.argtypes = [C.POINTER(_abi.EarthModel), C.POINTER(C.c_double)]
        L.oracle_stepper_init.argtypes = [C.POINTER(_Stepper), C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_double]
        L.oracle_stepper_init.restype = None
        L.oracle_stepper_next.argtypes = [C.POINTER(_Stepper)]
        L.oracle_stepper_next.restype = _RayState
        radius = C.c_double()
        self.spherical = bool(L.oracle_to_shape(C.byref(earth), C.byref(radius)))
        self.radius = radius.value

    @classmethod
    def of_config(cls, oracle, cfg):
        return cls(oracle, cfg.params.earth, cfg.params.straight_rays, cfg.atmosphere, cfg.params.wavelength)


def spec_valid(step, top, floor, m):
    return (math.isfinite(step) and step > 0.0 and math.isfinite(top) and math.isfinite(floor) and floor < top and 1 <= m <= M_MAX)


def ray(setting, h0, elevation_deg, step, top=100000.0, floor=0.0, m=M_MAX):
    """One ray -> (status, steps, true_elevation)."""
    s, L = setting, setting.o.lib
    e = float(elevation_deg)
    assert spec_valid(float(step), float(top), float(floor), int(m))
    if not (-90.0 < e < 90.0):  # a NaN too
        return LOST, 0, NAN
    st = _Stepper()
    L.oracle_stepper_init(C.byref(st), C.addressof(s.env), int(s.spherical), s.radius, float(h0), e * RAD_PER_DEG, int(s.straight), float(step))
    for i in range(1, int(m) + 1):
        h = L.oracle_stepper_next(C.byref(st)).h
        if h != h:
            return LOST, i, NAN
        if h < floor:
            return GROUND, i, NAN
        if h >= top:
            if s.straight:
                return EXIT, i, e
            if s.spherical:
                return EXIT, i, (dm_atan2(st.b, st.a) - st.x / s.radius) * DEG_PER_RAD
            return EXIT, i, dm_atan2(st.b, 1.0) * DEG_PER_RAD
    return INSIDE, int(m), NAN


class Result:
    """true_elevation f64, status u8, steps u32 in the shape of the input, and the counts of atmrt_sky_stats_t (stats)."""


def rays(setting, h0, elevations_deg, step, top=100000.0, floor=0.0, m=M_MAX, sky=None):
    """The rule over an array of launch elevations; sky: a boolean array of the same shape (None: every entry is a ray) — an entry
    that is not sky is NONE.  Equal elevations are marched once."""
    el = np.asarray(elevations_deg, dtype=np.float64)
    flat = el.ravel()
    is_sky = np.ones(flat.size, dtype=bool) if sky is None else np.asarray(sky, dtype=bool).ravel()
    true = np.full(flat.size, np.nan)
    status = np.zeros(flat.size, dtype=np.uint8)
    steps = np.zeros(flat.size, dtype=np.uint32)
    seen = {}
    for i in np.flatnonzero(is_sky):
        key = flat[i].tobytes()
        if key not in seen:
            seen[key] = ray(setting, h0, flat[i], step, top, floor, m)
        status[i], steps[i], true[i] = seen[key]
    out = Result()
    out.true_elevation, out.status, out.steps = true.reshape(el.shape), status.reshape(el.shape), steps.reshape(el.shape)
    out.stats = dict(none=int((~is_sky).sum()), exit=int((status == EXIT).sum()), ground=int((status == GROUND).sum()),
                     inside=int((status == INSIDE).sum()), lost=int(((status == LOST) & is_sky).sum()),
                     integrated_steps=int(steps.astype(np.int64).sum()))
    return out


def frame(setting, res, h0, step, top=100000.0, floor=0.0, m=M_MAX):
    """The rule over a frame (a result dict of the oracle or of the library): the pixels with hit_count == 0 are the rays."""
    return rays(setting, h0, res["elevation_angle"], step, top, floor, m, sky=np.asarray(res["hit_count"]) == 0)


def unit_vector(azimuth_deg, elevation_deg):
    se, ce = dm_sincos(float(elevation_deg) * RAD_PER_DEG)
    sa, ca = dm_sincos(float(azimuth_deg) * RAD_PER_DEG)
    return ce * ca, ce * sa, se


def body_valid(b):
    az, el, radius = float(b[0]), float(b[1]), float(b[2])
    return math.isfinite(az) and math.isfinite(el) and 0.0 < radius < 90.0


def body_of(bodies, azimuth_deg, true_elevation_deg):
    """bodies: rows of (azimuth_deg, elevation_deg, radius_deg[, rgb]) -> k + 1 for the first body k that holds the direction, 0."""
    assert len(bodies) <= BODIES_MAX and all(body_valid(b) for b in bodies)
    d = unit_vector(azimuth_deg, true_elevation_deg)
    for k, b in enumerate(bodies):
        u = unit_vector(b[0], b[1])
        if d[0] * u[0] + d[1] * u[1] + d[2] * u[2] >= dm_sincos(float(b[2]) * RAD_PER_DEG)[1]:
            return k + 1
    return 0


def body_plane(bodies, azimuth, true_elevation, status):
    """The body plane u8 in the shape of `status`."""
    az, te, st = (np.asarray(a) for a in (azimuth, true_elevation, status))
    out = np.zeros(st.size, dtype=np.uint8)
    for i in np.flatnonzero(st.ravel() == EXIT):
        out[i] = body_of(bodies, az.ravel()[i], te.ravel()[i])
    return out.reshape(st.shape)


def draw(rgb, body, bodies):
    """A copy of the image with every body's rgb over exactly the pixels whose body is not 0."""
    out = np.array(rgb, dtype=np.uint8, copy=True)
    for k, b in enumerate(bodies):
        out[np.asarray(body) == k + 1] = np.array(b[3], dtype=np.uint8)
    return out


def bennett(elevation_deg):
    """Bennett's formula for the refraction [deg] at 10 degrees C and 1010 hPa scaled to 15 degrees C and 1013.25 hPa."""
    h = float(elevation_deg)
    r_arcmin = 1.0 / math.tan(math.radians(h + 7.31 / (h + 4.4)))
    return r_arcmin / 60.0 * (1013.25 / 1010.0) * (283.0 / (273.0 + 15.0))
