"""The cast-shadow rule of include/atmrt.h ("cast shadows") restated in numpy over the oracle's primitives of the deterministic
flavour: coords_at_dist, get_elev and the ray stepper (the one oracle_ray_paths drives: H_i are the doubles ray_paths(params, h0 = H_0,
[elevation], step, m) returns; the stepper itself is driven here because the escape test also reads its slope).  Test
infrastructure only: what atmrt_shadow_mask* must return, byte for byte.  Every formula below is written as the header states it,
one IEEE operation at a time."""
import ctypes as C
import math

import numpy as np

import oracle_binding
from atm_raytracer_amd import _abi

NONE, LIT, SHADOWED = 0, 1, 2
M_MAX = 65535


class _Stepper(C.Structure):  # oracle_stepper, oracle/oracle.h
    _fields_ = [("atm", C.c_void_p), ("spherical", C.c_int), ("straight", C.c_int), ("radius", C.c_double), ("step", C.c_double),
                ("x", C.c_double), ("a", C.c_double), ("b", C.c_double), ("h0", C.c_double), ("ang", C.c_double)]


class _RayState(C.Structure):  # oracle_ray_state
    _fields_ = [("x", C.c_double), ("h", C.c_double), ("dh", C.c_double)]


def lattice(step, reach):
    """d_0 = 0, d_i = d_{i-1} + step as far as the first d_m >= reach -> (d [m + 1], m)."""
    d, x = [0.0], 0.0
    while not x >= reach:
        x = x + step
        d.append(x)
        if len(d) - 1 > M_MAX:
            raise ValueError("more than 65535 samples")
    return np.array(d, dtype=np.float64), len(d) - 1


class Setting:
    """The context's setting on the oracle's side: parameters, atmosphere and terrain tiles."""

    def __init__(self, oracle, cfg, tiles):
        self.o, self.params, self.atm = oracle, cfg.params, cfg.atmosphere
        self.terrain = oracle.terrain_new(tiles)
        self.top = float(max([int(t.max()) for t in tiles.values()] + [0])) + 1.0  # the mosaic's skip_above: every post is below it
        self.step = float(self.params.simulation_step)
        self.straight = bool(self.params.straight_rays)
        self.env = oracle.env(self.atm, self.params.wavelength)
        L = oracle.lib
        L.oracle_to_shape.argtypes = [C.POINTER(_abi.EarthModel), C.POINTER(C.c_double)]
        L.oracle_stepper_init.argtypes = [C.POINTER(_Stepper), C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_double]
        L.oracle_stepper_init.restype = None
        L.oracle_stepper_next.argtypes = [C.POINTER(_Stepper)]
        L.oracle_stepper_next.restype = _RayState
        radius = C.c_double()
        self.spherical = bool(L.oracle_to_shape(C.byref(self.params.earth), C.byref(radius)))
        self.radius = radius.value

    def close(self):
        self.o.terrain_free(self.terrain)

    def escape(self, reach, lib=None):
        """(floor, esc_ang_max) of the escape shortcut for a call of `reach`: the floor is the library's host-side certificate
        (atmrt_escape_certificate, no device) for this atmosphere and the mosaic's top; +inf: no certificate."""
        if lib is None:
            from atm_raytracer_amd import _lib
            lib = _lib.load()
        out = (C.c_double * 3)()
        rc = lib.atmrt_escape_certificate(C.byref(self.atm), self.params.wavelength, int(self.spherical), self.radius, int(self.straight),
                                          self.step, self.top, out)
        assert rc == 0
        ang_max = math.inf
        if self.straight and self.spherical:
            ang_max = 1.5207963267948966 - (np.float64(reach) + self.step) * (1.0 / self.radius)
        return out[0], float(ang_max)


def first_points(res):
    """(pixels [n] flat indices, lat, lon, elev) of the first trace point of every pixel with hit_count >= 1."""
    cnt = np.asarray(res["hit_count"]).ravel()
    off = np.asarray(res["hit_offset"]).ravel().astype(np.int64)
    px = np.flatnonzero(cnt >= 1)
    k = off[px]
    return px, res["lat"][k], res["lon"][k], res["elevation"][k]


def march(setting, lat_p, lon_p, elev_p, spec, d, m, floor, ang_max):
    """One pixel -> (status, block, esc): esc = the first index 1 <= i <= m at which a ray that is not yet shadowed passes the
    escape test after its step's test (0: never).  The rule itself never looks at esc."""
    o, L, s = setting.o, setting.o.lib, setting
    azimuth, elevation, _, lift = spec
    calc = oracle_binding.DirCalc()
    L.oracle_dircalc_new(C.byref(s.params.earth), float(lat_p), float(lon_p), float(azimuth), C.byref(calc))
    h0 = np.float64(elev_p) + np.float64(lift)
    st = _Stepper()
    ang = float(np.float64(elevation) * (math.pi / 180.0))  # om_to_radians
    L.oracle_stepper_init(C.byref(st), C.addressof(s.env), int(s.spherical), s.radius, float(h0), ang, int(s.straight), s.step)
    lat, lon, e = C.c_double(), C.c_double(), C.c_double()
    h_prev, esc = float(h0), 0
    for i in range(1, m + 1):
        h = L.oracle_stepper_next(C.byref(st)).h
        L.oracle_coords_at_dist(C.byref(calc), float(d[i]), C.byref(lat), C.byref(lon))
        t = e.value if L.oracle_terrain_get_elev(s.terrain, lat.value, lon.value, C.byref(e)) else 0.0
        if h < t or h_prev < -1000.0:  # a NaN compares false
            return SHADOWED, i, esc
        if not esc and h > floor and ((h > h_prev and st.ang < ang_max) if s.straight else st.b > 0.0):
            esc = i
        h_prev = h
    return LIT, 0, esc


class Result:
    """status / block [height][width] as the library writes them, esc [height][width] (see march), and the counts of
    atmrt_shadow_stats_t with the shortcut on (stats_on) and off (stats_off)."""


def solve(setting, res, spec, lib=None):
    """res: the frame (a result dict of the oracle or of the library); spec: (azimuth_deg, elevation_deg, reach, lift)."""
    spec = tuple(float(v) for v in spec)
    d, m = lattice(setting.step, spec[2])
    floor, ang_max = setting.escape(spec[2], lib)
    H, W = np.asarray(res["hit_count"]).shape
    status = np.zeros(H * W, dtype=np.uint8)
    block = np.zeros(H * W, dtype=np.uint16)
    esc = np.zeros(H * W, dtype=np.int32)
    px, lat, lon, elev = first_points(res)
    for p, la, lo, el in zip(px, lat, lon, elev):
        status[p], block[p], esc[p] = march(setting, la, lo, el, spec, d, m, floor, ang_max)
    out = Result()
    out.m, out.floor = m, floor
    out.status, out.block, out.esc = status.reshape(H, W), block.reshape(H, W), esc.reshape(H, W)
    lit, sh = status == LIT, status == SHADOWED
    base = dict(none=int((status == NONE).sum()), lit=int(lit.sum()), shadowed=int(sh.sum()))
    steps_off = int(block[sh].astype(np.int64).sum()) + m * int(lit.sum())
    escaped = lit & (esc > 0)  # a shadowed ray's esc would contradict the certificate: test_shadow_model.py asserts there is none
    steps_on = int(block[sh].astype(np.int64).sum()) + int(esc[escaped].astype(np.int64).sum()) + m * int((lit & ~escaped).sum())
    out.stats_off = dict(base, integrated_steps=steps_off, escaped_rays=0)
    out.stats_on = dict(base, integrated_steps=steps_on, escaped_rays=int((escaped & (esc < m)).sum()))
    return out


def shadowed_result(res, status):
    """A copy of the frame in which the first trace point's normal of every SHADOWED pixel is (0, 0, 0): oracle.draw_image over it
    is the expected shadowed image — light_dot = 0, brightness = ambient_light exactly, whatever the sign of the zero."""
    out = dict(res)
    normal = np.array(res["normal"], dtype=np.float64, copy=True)
    off = np.asarray(res["hit_offset"]).ravel().astype(np.int64)
    px = np.flatnonzero(np.asarray(status).ravel() == SHADOWED)
    normal.reshape(-1, 3)[off[px]] = 0.0
    out["normal"] = normal
    return out
