"""The rule of include/atmrt.h, "sky light", restated over the oracle's ray stepper and oracle_n (driven through ctypes, as
tests/sky_model.py drives the stepper) and the host build of detmath.h's exp / sincos (tests/csrc/sky_light_export.c, built here).
Test infrastructure only: what atmrt_sky_light_ray_host, atmrt_sky_zenith_column_host, atmrt_sky_shade_host, atmrt_sky_light* and
atmrt_sky_shade* must return, byte for byte.  The arithmetic is Python's float: IEEE doubles, every operation rounded on its own."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

import sky_model as sm
from shadow_model import _Stepper
from sky_model import EXIT, GROUND, INSIDE, LOST, NONE, NAN, RAD_PER_DEG, Setting  # noqa: F401  (re-exported for the tests)

HERE = os.path.dirname(os.path.abspath(__file__))
NODES_MAX = 1048575
# the Python and CLI defaults (atm_raytracer_amd.generators): this project's choice
TAU, LIMB, EXPOSURE, AIRLIGHT = (0.06, 0.11, 0.24), (0.5, 0.6, 0.75), 4.0, (255, 255, 255)
_DM = []


def _dm():
    """detmath.h's exp and sincos, compiled for the host with the flags of tests/cbuild.dm_export into tests/_build."""
    if not _DM:
        src = os.path.join(HERE, "csrc", "sky_light_export.c")
        out = os.path.join(HERE, "_build", "libsky_light_export.so")
        hdr = [os.path.join(HERE, "..", "atm-raytracer_amd", "csrc", h) for h in ("detmath.h", "detmath_tables.h")]
        os.makedirs(os.path.dirname(out), exist_ok=True)
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in [src] + hdr):
            subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-o", out, src, "-lm"], check=True)
        L = C.CDLL(out)
        L.sl_exp.argtypes, L.sl_exp.restype = [C.c_double], C.c_double
        L.sl_sincos.argtypes, L.sl_sincos.restype = [C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)], None
        _DM.append(L)
    return _DM[0]


def dm_exp(x):
    return _dm().sl_exp(float(x))


def dm_sincos(x):
    s, c = C.c_double(), C.c_double()
    _dm().sl_sincos(float(x), C.byref(s), C.byref(c))
    return s.value, c.value


def q_of(setting, h):
    """q(h) = n(h) - 1 with n the oracle's."""
    return setting.o.n(setting.env, float(h)) - 1.0


def ray(setting, h0, elevation_deg, step, top=100000.0, floor=0.0, m=sm.M_MAX):
    """One ray -> (status, steps, true_elevation, column)."""
    s, L = setting, setting.o.lib
    e, step, top, floor = float(elevation_deg), float(step), float(top), float(floor)
    assert sm.spec_valid(step, top, floor, int(m))
    if not (-90.0 < e < 90.0):  # a NaN too
        return LOST, 0, NAN, NAN
    st = _Stepper()
    L.oracle_stepper_init(C.byref(st), C.addressof(s.env), int(s.spherical), s.radius, float(h0), e * RAD_PER_DEG, int(s.straight), step)
    h_prev, q_prev, column = float(h0), q_of(s, h0), 0.0
    for i in range(1, int(m) + 1):
        h = L.oracle_stepper_next(C.byref(st)).h
        if h != h:
            return LOST, i, NAN, NAN
        if h < floor:
            return GROUND, i, NAN, NAN
        q = q_of(s, h)
        w = (step / s.radius) * (0.5 * (h_prev + h) + s.radius) if s.spherical else step
        dh = h - h_prev
        column = column + 0.5 * (q_prev + q) * math.sqrt(w * w + dh * dh)
        h_prev, q_prev = h, q
        if h >= top:
            if s.straight:
                return EXIT, i, e, column
            if s.spherical:
                return EXIT, i, (sm.dm_atan2(st.b, st.a) - st.x / s.radius) * sm.DEG_PER_RAD, column
            return EXIT, i, sm.dm_atan2(st.b, 1.0) * sm.DEG_PER_RAD, column
    return INSIDE, int(m), NAN, NAN


def rays(setting, h0, elevations_deg, step, top=100000.0, floor=0.0, m=sm.M_MAX, sky=None):
    """sky_model.rays with the column plane: a sky_model.Result with `column` in the shape of the input."""
    el = np.asarray(elevations_deg, dtype=np.float64)
    flat = el.ravel()
    is_sky = np.ones(flat.size, dtype=bool) if sky is None else np.asarray(sky, dtype=bool).ravel()
    true, column = np.full(flat.size, np.nan), np.full(flat.size, np.nan)
    status = np.zeros(flat.size, dtype=np.uint8)
    steps = np.zeros(flat.size, dtype=np.uint32)
    seen = {}
    for i in np.flatnonzero(is_sky):
        key = flat[i].tobytes()
        if key not in seen:
            seen[key] = ray(setting, h0, flat[i], step, top, floor, m)
        status[i], steps[i], true[i], column[i] = seen[key]
    out = sm.Result()
    out.true_elevation, out.status, out.steps, out.column = (a.reshape(el.shape) for a in (true, status, steps, column))
    out.stats = dict(none=int((~is_sky).sum()), exit=int((status == EXIT).sum()), ground=int((status == GROUND).sum()),
                     inside=int((status == INSIDE).sum()), lost=int(((status == LOST) & is_sky).sum()),
                     integrated_steps=int(steps.astype(np.int64).sum()))
    return out


def frame(setting, res, h0, step, top=100000.0, floor=0.0, m=sm.M_MAX):
    """The rule over a frame: the pixels with hit_count == 0 are the rays."""
    return rays(setting, h0, res["elevation_angle"], step, top, floor, m, sky=np.asarray(res["hit_count"]) == 0)


def zenith_valid(ref_alt, top, dz):
    ref_alt, top, dz = float(ref_alt), float(top), float(dz)
    if not (math.isfinite(dz) and dz > 0.0 and math.isfinite(ref_alt) and math.isfinite(top) and ref_alt < top):
        return False
    return math.ceil((top - ref_alt) / dz) <= NODES_MAX


def zenith_column(setting, ref_alt, top, dz):
    """Z0(ref_alt, top, dz)."""
    ref_alt, top, dz = float(ref_alt), float(top), float(dz)
    assert zenith_valid(ref_alt, top, dz)
    K = max(1, math.ceil((top - ref_alt) / dz))
    h_prev, q_prev, z = ref_alt, q_of(setting, ref_alt), 0.0
    for k in range(1, K + 1):
        h = ref_alt + float(k) * dz if k < K else top
        q = q_of(setting, h)
        z = z + 0.5 * (q_prev + q) * (h - h_prev)
        h_prev, q_prev = h, q
    return z


def shade_valid(z0, tau, limb, exposure):
    return (math.isfinite(z0) and z0 > 0.0 and math.isfinite(exposure) and exposure >= 0.0
            and all(math.isfinite(t) and t >= 0.0 for t in tau) and all(0.0 <= u <= 1.0 for u in limb))


def byte(v):
    return 255 if v >= 255.0 else (int(v) if v > 0.0 else 0)


def unit_vector(azimuth_deg, elevation_deg):
    se, ce = dm_sincos(float(elevation_deg) * RAD_PER_DEG)
    sa, ca = dm_sincos(float(azimuth_deg) * RAD_PER_DEG)
    return ce * ca, ce * sa, se


def shade_pixel(z0, bodies, azimuth_deg, true_elevation_deg, column, tau=TAU, limb=LIMB, exposure=EXPOSURE, airlight=AIRLIGHT):
    """One EXIT pixel -> (body, (r, g, b)).  bodies: rows of (azimuth_deg, elevation_deg, radius_deg, rgb)."""
    assert shade_valid(float(z0), tau, limb, float(exposure))
    body = sm.body_of(bodies, azimuth_deg, true_elevation_deg)
    x = float(column) / float(z0)
    mu = 0.0
    if body:
        b = bodies[body - 1]
        d, u = unit_vector(azimuth_deg, true_elevation_deg), unit_vector(b[0], b[1])
        ex, ey, ez = d[0] - u[0], d[1] - u[1], d[2] - u[2]
        chord2 = ex * ex + ey * ey + ez * ez
        s = dm_sincos(0.5 * (float(b[2]) * RAD_PER_DEG))[0]
        m = 1.0 - chord2 / (4.0 * s * s)
        mu = math.sqrt(m) if m > 0.0 else 0.0
    out = []
    for c in range(3):
        t = dm_exp(-(float(tau[c]) * x))
        if body:
            v = float(bodies[body - 1][3][c]) * t * (1.0 - float(limb[c]) * (1.0 - mu))
        else:
            v = float(airlight[c]) * float(exposure) * (1.0 - t)
        out.append(byte(v))
    return body, tuple(out)


def shade(rgb, z0, bodies, azimuth, true_elevation, status, column, **params):
    """(the body plane u8, a copy of the image with its EXIT pixels shaded)."""
    az, te, st, col = (np.asarray(a) for a in (azimuth, true_elevation, status, column))
    image = np.array(rgb, dtype=np.uint8, copy=True)
    flat = image.reshape(-1, 3)
    body = np.zeros(st.size, dtype=np.uint8)
    for i in np.flatnonzero(st.ravel() == EXIT):
        body[i], flat[i] = shade_pixel(z0, bodies, az.ravel()[i], te.ravel()[i], col.ravel()[i], **params)
    return body.reshape(st.shape), image


def kasten_young(elevation_deg):
    """Kasten and Young 1989: the relative optical air mass at an apparent elevation [deg]."""
    e = float(elevation_deg)
    return 1.0 / (math.sin(math.radians(e)) + 0.50572 * (e + 6.07995) ** -1.6364)
