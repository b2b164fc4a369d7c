"""The rule of include/atmrt.h, "shadow lights", restated in numpy over the oracle's primitives: the light's local direction at a
point from oracle_world_directions and the host build of detmath.h's asin / atan2 (tests/cbuild.dm_export), then the cast-shadow
march of tests/shadow_model.py with the point's own angles.  Test infrastructure only: what atmrt_shadow_lights* and the two host
functions must return, byte for byte.  The arithmetic is Python's float: IEEE doubles, every operation rounded on its own."""
import ctypes as C
import math

import numpy as np

import cbuild
import shadow_model as sm
from shadow_model import LIT, NONE, SHADOWED, Setting, first_points, lattice  # noqa: F401  (re-exported for the tests)

DEG_PER_RAD = 180.0 / 3.141592653589793  # detmath.h's DM_DEG_PER_RAD
RAD_PER_DEG = 3.141592653589793 / 180.0
_DM = []


def _dm():
    if not _DM:
        _DM.append(C.CDLL(cbuild.dm_export()))
    return _DM[0]


def _call(name, *xs):
    ins = [(C.c_double * 1)(float(x)) for x in xs]
    out = (C.c_double * 1)()
    getattr(_dm(), "t_" + name)(*ins, out, C.c_size_t(1))
    return out[0]


def dm_asin(x):
    return _call("asin", x)


def dm_atan2(y, x):
    return _call("atan2", y, x)


def dm_sincos(x):
    s, c = (C.c_double * 1)(), (C.c_double * 1)()
    _dm().t_sincos((C.c_double * 1)(float(x)), s, c, C.c_size_t(1))
    return s[0], c[0]


def normalise(light):
    """The rule's light: (x, y, z) -> L, or None where the rule refuses it."""
    x, y, z = (float(v) for v in light)
    if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(z)):
        return None
    n2 = x * x + y * y + z * z
    if not (math.isfinite(n2) and n2 > 0.0):
        return None
    s = math.sqrt(n2)
    return (x / s, y / s, z / s)


def dot(p, q):
    return float(p[0]) * float(q[0]) + float(p[1]) * float(q[1]) + float(p[2]) * float(q[2])


def local_direction(oracle, earth, L, lat, lon):
    """(azimuth_deg, elevation_deg) of the NORMALISED light L in the local frame of (lat, lon)."""
    n, e, u = oracle.world_directions(earth, float(lat), float(lon))
    a, b, c = dot(L, n), dot(L, e), dot(L, u)
    cc = 1.0 if c > 1.0 else (-1.0 if c < -1.0 else c)  # a NaN passes through
    return dm_atan2(b, a) * DEG_PER_RAD, dm_asin(cc) * DEG_PER_RAD


def light_direction(oracle, earth, lat, lon, azimuth_deg, elevation_deg):
    """The world-frame vector of a light seen from (lat, lon) under the two angles, in the header's order of operations."""
    n, e, u = oracle.world_directions(earth, float(lat), float(lon))
    sa, ca = dm_sincos(float(azimuth_deg) * RAD_PER_DEG)
    se, ce = dm_sincos(float(elevation_deg) * RAD_PER_DEG)
    return np.array([(float(n[k]) * (ce * ca) + float(e[k]) * (ce * sa)) + float(u[k]) * se for k in range(3)])


def lights_from_angles(oracle, params, rows):
    pos = params.position
    return np.array([light_direction(oracle, params.earth, pos.latitude, pos.longitude, az, el) for az, el in rows]).reshape(-1, 3)


class Result:
    """lit_mask [H][W] u64, status / block / esc [n_lights][H][W] as the library writes them (esc: shadow_model.march's), the local
    angles azimuth / elevation [n_lights][H][W] (NaN without a trace point), marched [n_lights][H][W], and the counts of
    atmrt_shadow_stats_t with the shortcut on (stats_on) and off (stats_off)."""


def solve(setting, res, dirs, reach, lift=0.0, lib=None):
    """res: the frame (a result dict of the oracle or of the library); dirs: [n_lights][3] as the caller hands them over."""
    dirs = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    lights = [normalise(v) for v in dirs]
    assert 1 <= len(lights) <= 64 and all(v is not None for v in lights)
    d, m = lattice(setting.step, float(reach))
    floor, ang_max = setting.escape(float(reach), lib)
    H, W = np.asarray(res["hit_count"]).shape
    n = len(lights)
    mask = np.zeros(H * W, dtype=np.uint64)
    status = np.zeros((n, H * W), dtype=np.uint8)
    block = np.zeros((n, H * W), dtype=np.uint16)
    esc = np.zeros((n, H * W), dtype=np.int32)
    marched = np.zeros((n, H * W), dtype=bool)
    azimuth, elevation = np.full((n, H * W), np.nan), np.full((n, H * W), np.nan)
    px, lat, lon, elev = first_points(res)
    for p, la, lo, el in zip(px, lat, lon, elev):
        bits = 0
        for l, L in enumerate(lights):
            az_p, el_p = local_direction(setting.o, setting.params.earth, L, la, lo)
            azimuth[l, p], elevation[l, p] = az_p, el_p
            if el_p >= 90.0:
                out = (LIT, 0, 0)
            elif el_p <= -90.0:
                out = (SHADOWED, 1, 0)
            elif not (-90.0 < el_p < 90.0):  # NaN
                out = (LIT, 0, 0)
            else:
                marched[l, p] = True
                out = sm.march(setting, la, lo, el, (az_p, el_p, float(reach), float(lift)), d, m, floor, ang_max)
            status[l, p], block[l, p], esc[l, p] = out
            if out[0] == LIT:
                bits |= 1 << l
        mask[p] = bits
    r = Result()
    r.m, r.floor, r.n_lights = m, floor, n
    r.lit_mask = mask.reshape(H, W)
    r.status, r.block, r.esc = status.reshape(n, H, W), block.reshape(n, H, W), esc.reshape(n, H, W)
    r.marched, r.azimuth, r.elevation = marched.reshape(n, H, W), azimuth.reshape(n, H, W), elevation.reshape(n, H, W)
    lit, sh = status == LIT, status == SHADOWED
    none = int((np.asarray(res["hit_count"]).ravel() == 0).sum())
    base = dict(none=none, lit=int(lit.sum()), shadowed=int(sh.sum()))
    blocked = int(block[sh & marched].astype(np.int64).sum())
    escaped = lit & marched & (esc > 0)
    r.stats_off = dict(base, integrated_steps=blocked + m * int((lit & marched).sum()), escaped_rays=0)
    r.stats_on = dict(base, integrated_steps=blocked + int(esc[escaped].astype(np.int64).sum()) + m * int((lit & marched & ~escaped).sum()),
                      escaped_rays=int((escaped & (esc < m)).sum()))
    return r
