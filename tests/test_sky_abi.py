"""The host half of the sky rays (include/atmrt.h, "sky rays"): names and struct sizes, the two host functions — atmrt_sky_ray_host
(the function the kernel's lanes run) and atmrt_sky_body_host — against tests/sky_model.py bit for bit, and every refusal that needs
no device.  The library loads without a GPU; nothing here touches a device.  The refusals that need a context are in
tests/test_gpu_sky.py."""
import ctypes as C
import math
import os
import re
import struct

import numpy as np
import pytest

import shadow_cases
import sky_model as sm
from atm_raytracer_amd import _abi, _lib, config, generators

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("atmrt_sky_ray_host", "atmrt_sky_body_host", "atmrt_sky_rays", "atmrt_sky_directions_device", "atmrt_sky_directions",
         "atmrt_sky_directions_planes_device", "atmrt_sky_bodies_device", "atmrt_sky_bodies", "atmrt_sky_bodies_planes_device",
         "atmrt_last_sky_timings")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def cfg_of(earth, atmosphere=None):
    d = {"view": {"position": {"latitude": 0.0, "longitude": 0.0, "altitude": {"Absolute": 100.0}},
                  "frame": {"direction": 0.0, "fov": 30.0, "tilt": 0.0, "max_distance": 10_000.0}},
         "earth_shape": earth, "output": {"width": 8, "height": 8, "generator": "Fast"}}
    if atmosphere is not None:
        d["atmosphere"] = atmosphere
    return config.Config.from_dict(d)


def same(a, b):
    return struct.pack("d", a) == struct.pack("d", b) or (math.isnan(a) and math.isnan(b))


def test_names_and_struct_sizes(lib):
    header = open(os.path.join(ROOT, "include", "atmrt.h")).read()
    declared = set(re.findall(r"\b(atmrt_[a-z0-9_]+)\s*\(", header))
    for name in NAMES:
        assert name in declared and name in _lib.EXPORTED and hasattr(lib, name), name
    assert lib.atmrt_abi_sizeof(42) == C.sizeof(_abi.SkySpec) == 32
    assert lib.atmrt_abi_sizeof(43) == C.sizeof(_abi.SkyRay) == generators.SKY_RAY_DTYPE.itemsize == 16
    assert lib.atmrt_abi_sizeof(44) == C.sizeof(_abi.SkyStats) == 48
    assert lib.atmrt_abi_sizeof(45) == C.sizeof(_abi.SkyBody) == 32
    assert lib.atmrt_abi_sizeof(41) == 0 and lib.atmrt_abi_sizeof(46) == 0
    assert (_abi.SkySpec.step.offset, _abi.SkySpec.top.offset, _abi.SkySpec.floor.offset, _abi.SkySpec.m.offset) == (0, 8, 16, 24)
    assert (_abi.SkyBody.radius_deg.offset, _abi.SkyBody.rgb.offset) == (16, 24)
    assert lib.atmrt_abi_version() == 5  # the additions are additive
    assert "sky rays" in header and "What bends above `top` is neglected" in header


# some forty elevations: the statuses of tests/test_sky_model.py (GROUND at -1.0, EXIT at -0.5, LOST at 89.9 and outside (-90, 90))
ELEVATIONS = [-89.0, -10.0, -2.0, -1.2, -1.0, -0.9, -0.8, -0.7, -0.5, -0.3, -0.1, 0.0, 0.05, 0.1, 0.2, 0.3, 0.5, 0.7, 1.0, 1.5, 2.0, 3.0, 4.0,
              5.0, 7.5, 10.0, 15.0, 20.0, 30.0, 45.0, 60.0, 75.0, 85.0, 89.0, 89.9, 89.999, 90.0, -90.0, 123.0, math.nan, math.inf, -math.inf]
SETTINGS = [(earth, straight, atm) for earth in ("SimpleSphere", "FlatDistorted") for straight in (False, True) for atm in ("us76", "spline")]


@pytest.mark.parametrize("earth,straight,atm", SETTINGS, ids=[f"{e}-{'straight' if s else 'refracted'}-{a}" for e, s, a in SETTINGS])
def test_ray_host_equals_the_model_bit_for_bit(lib, oracle_det, earth, straight, atm):
    cfg = cfg_of(earth, shadow_cases.spline_atmosphere() if atm == "spline" else None)
    setting = sm.Setting(oracle_det, cfg.params.earth, straight, cfg.atmosphere, cfg.params.wavelength)
    seen = set()
    for m in (1500, 100):
        spec = generators.sky_spec(1000.0, 100000.0, 0.0, m)
        for e in ELEVATIONS:
            got = generators.sky_ray_host(cfg.atmosphere, cfg.params.wavelength, cfg.params.earth, straight, spec, 1000.0, e, lib)
            want = sm.ray(setting, 1000.0, e, 1000.0, 100000.0, 0.0, m)
            assert got[:2] == want[:2] and same(got[2], want[2]), (earth, straight, atm, m, e, got, want)
            seen.add(got[0])
    print(f"sky host {earth} straight={straight} {atm}: statuses {sorted(seen)}")
    assert sm.LOST in seen and sm.GROUND in seen
    if atm == "us76":
        assert {sm.EXIT, sm.INSIDE} <= seen


def test_body_host_equals_the_model(lib):
    sun = (100.0, 3.0, 0.2666, (255, 240, 200))
    moon = (100.3, 3.1, 0.25, (200, 200, 220))
    wide = (250.0, -40.0, 30.0, (1, 2, 3))
    lists = ([sun], [sun, moon], [moon, sun], [wide, sun], [])
    dirs = [(100.0, 3.0), (100.3, 3.1), (100.15, 3.05), (101.0, 3.0), (250.0, -40.0), (250.0, -10.0 + 1e-9), (250.0, -10.0 - 1e-9)]
    for az, el, r, _ in (sun, moon):  # the radius +- 1e-9 degrees, above, below and beside the centre
        for d in (1e-9, -1e-9):
            dirs += [(az, el + r + d), (az, el - r - d), (az + (r + d) / math.cos(math.radians(el)), el)]
    rng = np.random.default_rng(11)
    dirs += [(float(100.0 + rng.uniform(-0.6, 0.9)), float(3.0 + rng.uniform(-0.5, 0.6))) for _ in range(300)]
    counts = {}
    for bodies in lists:
        for az, el in dirs:
            got, want = generators.sky_body_host(bodies, az, el, lib), sm.body_of(bodies, az, el)
            assert got == want, (bodies, az, el, got, want)
            counts[got] = counts.get(got, 0) + 1
    print(f"sky body host: {counts}")
    assert counts[0] > 0 and counts[1] > 0 and counts[2] > 0
    # the centre, the edge, the overlap: the first body wins
    assert generators.sky_body_host([sun], 100.0, 3.0, lib) == 1
    assert generators.sky_body_host([sun], 100.0, 3.0 + 0.2666 - 1e-9, lib) == 1 and generators.sky_body_host([sun], 100.0, 3.0 + 0.2666 + 1e-9, lib) == 0
    assert generators.sky_body_host([sun, moon], 100.15, 3.05, lib) == 1 and generators.sky_body_host([moon, sun], 100.15, 3.05, lib) == 1


def test_refusals(lib):
    cfg = cfg_of("SimpleSphere")
    atm, earth, wl = cfg.atmosphere, cfg.params.earth, cfg.params.wavelength
    bad, nan, inf = _abi.ERR_INVALID_ARGUMENT, math.nan, math.inf
    out = _abi.SkyRay(77, 77, 77.0)
    good = generators.sky_spec(1000.0, 100000.0, 0.0, 1500)

    def call(spec=good, h0=1000.0, e=1.0, atm_p=C.byref(atm), earth_p=C.byref(earth), out_p=C.byref(out)):
        return lib.atmrt_sky_ray_host(atm_p, wl, earth_p, 0, None if spec is None else C.byref(spec), h0, e, out_p)

    assert call() == 0 and out.status == sm.EXIT
    out.status, out.steps, out.true_elevation = 77, 77, 77.0
    assert call(atm_p=None) == bad and call(earth_p=None) == bad and call(spec=None) == bad and call(out_p=None) == bad
    for step, top, floor, m in ((0.0, 1e5, 0.0, 1500),  # no context to take the step from
                                (-1.0, 1e5, 0.0, 1500), (nan, 1e5, 0.0, 1500), (inf, 1e5, 0.0, 1500), (1000.0, nan, 0.0, 1500),
                                (1000.0, inf, 0.0, 1500), (1000.0, 1e5, nan, 1500), (1000.0, 1e5, -inf, 1500), (1000.0, 1e5, 1e5, 1500),
                                (1000.0, 1e5, 2e5, 1500), (1000.0, 1e5, 0.0, 0), (1000.0, 1e5, 0.0, -3), (1000.0, 1e5, 0.0, 1048576)):
        assert not sm.spec_valid(step, top, floor, m)
        assert call(spec=generators.sky_spec(step, top, floor, m)) == bad, (step, top, floor, m)
    assert call(h0=nan) == bad and call(h0=inf) == bad
    unknown = _abi.EarthModel()
    C.memmove(C.byref(unknown), C.byref(earth), C.sizeof(earth))
    unknown.kind = 99
    assert call(earth_p=C.byref(unknown)) == bad
    assert (out.status, out.steps, out.true_elevation) == (77, 77, 77.0)
    assert call(spec=generators.sky_spec(1000.0, 1e5, 0.0, 1048575), e=45.0) == 0 and call(spec=generators.sky_spec(1000.0, 1e5, 0.0, 1)) == 0
    assert call(e=nan) == 0 and (out.status, out.steps) == (sm.LOST, 0)  # no error: LOST at step 0

    body = C.c_uint32(77)
    sun = generators.sky_body(100.0, 3.0)
    one = (_abi.SkyBody * 1)(sun)
    assert lib.atmrt_sky_body_host(one, 1, 100.0, 3.0, C.byref(body)) == 0 and body.value == 1
    body.value = 77
    assert lib.atmrt_sky_body_host(None, 1, 100.0, 3.0, C.byref(body)) == bad
    assert lib.atmrt_sky_body_host(one, 1, 100.0, 3.0, None) == bad
    many = (_abi.SkyBody * 33)(*[sun] * 33)
    assert lib.atmrt_sky_body_host(many, 33, 100.0, 3.0, C.byref(body)) == bad
    for az, el, r in ((nan, 3.0, 0.3), (inf, 3.0, 0.3), (100.0, nan, 0.3), (100.0, -inf, 0.3), (100.0, 3.0, 0.0), (100.0, 3.0, -1.0),
                      (100.0, 3.0, 90.0), (100.0, 3.0, nan), (100.0, 3.0, inf)):
        assert not sm.body_valid((az, el, r))
        assert lib.atmrt_sky_body_host((_abi.SkyBody * 1)(generators.sky_body(az, el, r)), 1, 100.0, 3.0, C.byref(body)) == bad, (az, el, r)
    assert body.value == 77
    assert lib.atmrt_sky_body_host(many, 32, 100.0, 3.0, C.byref(body)) == 0 and body.value == 1
    assert lib.atmrt_sky_body_host(None, 0, 100.0, 3.0, C.byref(body)) == 0 and body.value == 0
    # the entry points refuse a NULL context before they look at anything else
    buf = np.zeros(64, dtype=np.uint64)
    p = buf.ctypes.data
    assert lib.atmrt_sky_rays(None, C.byref(good), 1000.0, 4, p, p, None) == bad
    assert lib.atmrt_sky_directions(None, C.byref(good), p, p, p, None) == bad
    assert lib.atmrt_sky_directions_device(None, C.byref(good), p, p, p, None) == bad
    assert lib.atmrt_sky_directions_planes_device(None, C.byref(good), 1000.0, 8, p, p, p, p, p, None) == bad
    assert lib.atmrt_sky_bodies(None, one, 1, p, p, p, None) == bad
    assert lib.atmrt_sky_bodies_device(None, one, 1, p, p, p, None) == bad
    assert lib.atmrt_sky_bodies_planes_device(None, one, 1, 8, p, p, p, p, None) == bad
    assert lib.atmrt_last_sky_timings(None, (C.c_double * 3)()) == bad
    assert not buf.any()
