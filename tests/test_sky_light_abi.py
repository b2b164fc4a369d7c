"""The host half of the sky light (include/atmrt.h, "sky light"): names and struct sizes, the three host functions —
atmrt_sky_light_ray_host (the function the kernel's lanes run), atmrt_sky_zenith_column_host and atmrt_sky_shade_host — against
tests/sky_light_model.py bit for bit over the lists and the shade grid of tests/sky_light_cases.py, and every refusal that needs no
device.  The library loads without a GPU; nothing here touches a device.  The refusals that need a context are in
tests/test_gpu_sky_light.py."""
import ctypes as C
import math
import os
import re
import struct

import numpy as np
import pytest

import shadow_cases
import sky_light_cases as lc
import sky_light_model as slm
from atm_raytracer_amd import _abi, _lib, config, generators

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("atmrt_sky_zenith_column_host", "atmrt_sky_light_ray_host", "atmrt_sky_shade_host", "atmrt_sky_light_rays", "atmrt_sky_light_device",
         "atmrt_sky_light", "atmrt_sky_light_planes_device", "atmrt_sky_shade_device", "atmrt_sky_shade", "atmrt_sky_shade_planes_device",
         "atmrt_last_sky_shade_timing")


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
    assert lib.atmrt_abi_sizeof(49) == C.sizeof(_abi.SkyLightSpec) == 48
    assert lib.atmrt_abi_sizeof(50) == C.sizeof(_abi.SkyShade) == 72
    assert lib.atmrt_abi_sizeof(48) == 0 and lib.atmrt_abi_sizeof(51) == 0
    assert (_abi.SkyLightSpec.ref_alt.offset, _abi.SkyLightSpec.column_dz.offset) == (32, 40)
    assert (_abi.SkyShade.tau.offset, _abi.SkyShade.limb.offset, _abi.SkyShade.exposure.offset, _abi.SkyShade.airlight.offset) == (8, 32, 56, 64)
    assert lib.atmrt_abi_version() == 5  # the additions are additive
    assert "sky light" in header and "The airlight does not know where the sun is" in header
    assert (generators.SKY_TAU, generators.SUN_LIMB, generators.SKY_EXPOSURE, generators.SKY_AIRLIGHT) == (slm.TAU, slm.LIMB, slm.EXPOSURE, slm.AIRLIGHT)


SETTINGS = [(earth, straight, atm) for earth in ("SimpleSphere", "FlatDistorted") for straight in (False, True) for atm in ("us76", "spline")]


@pytest.mark.parametrize("earth,straight,atm", SETTINGS, ids=[f"{e}-{'straight' if s else 'refracted'}-{a}" for e, s, a in SETTINGS])
def test_ray_host_equals_the_model_bit_for_bit(lib, oracle_det, earth, straight, atm):
    """The lists of the GPU cases (the long one at m = 1500, the short one at m = 100, 65 entries: every distinct elevation of the
    longer lists is among them) and a few elevations beside them, in every setting."""
    cfg = cfg_of(earth, shadow_cases.spline_atmosphere() if atm == "spline" else None)
    setting = slm.Setting(oracle_det, cfg.params.earth, straight, cfg.atmosphere, cfg.params.wavelength)
    extra = [-89.0, -10.0, 5.0, 30.0, 60.0, 85.0, 89.9, 90.0, -90.0, 123.0, math.nan, math.inf]
    seen, columns = set(), 0
    for m, elevations in ((lc.M, list(lc.list_elevations(65)) + extra), (lc.SHORT_M, list(lc.list_elevations_short(65)) + extra)):
        spec = generators.sky_spec(lc.STEP, lc.TOP, lc.FLOOR, m)
        for e in elevations:
            got = generators.sky_light_ray_host(cfg.atmosphere, cfg.params.wavelength, cfg.params.earth, straight, spec, lc.LIST_H0, e, lib)
            want = slm.ray(setting, lc.LIST_H0, e, lc.STEP, lc.TOP, lc.FLOOR, m)
            assert got[:2] == want[:2] and same(got[2], want[2]) and same(got[3], want[3]), (earth, straight, atm, m, e, got, want)
            plain = generators.sky_ray_host(cfg.atmosphere, cfg.params.wavelength, cfg.params.earth, straight, spec, lc.LIST_H0, e, lib)
            assert got[:2] == plain[:2] and same(got[2], plain[2])  # the sky-ray rule's record, the same bits
            # (an EXIT ray's column may be NaN too: a steep ray leaps far above the atmosphere's last layer in one step, where n(h) is NaN)
            assert math.isnan(got[3]) or got[0] == slm.EXIT
            seen.add(got[0])
            columns += got[0] == slm.EXIT and got[3] > 0.0
    print(f"sky light host {earth} straight={straight} {atm}: statuses {sorted(seen)}, {columns} columns")
    assert slm.LOST in seen and slm.GROUND in seen
    if atm == "us76":
        assert {slm.EXIT, slm.INSIDE} <= seen and columns >= (20 if earth == "SimpleSphere" else 5)  # (a flat earth turns the low rays back)


def test_zenith_column_host_equals_the_model(lib, oracle_det):
    for atm in (None, shadow_cases.spline_atmosphere()):
        cfg = cfg_of("SimpleSphere", atm)
        setting = slm.Setting(oracle_det, cfg.params.earth, False, cfg.atmosphere, cfg.params.wavelength)
        top = 100000.0 if atm is None else 20000.0
        for ref_alt, dz in ((0.0, 100.0), (0.0, 1000.0), (0.0, 10.0), (2500.0, 1000.0), (-300.0, 777.7), (0.0, 30000.0), (0.0, top), (0.0, 2.0 * top),
                            (1.0, 176.32698070846498)):
            got = generators.sky_zenith_column(cfg.atmosphere, cfg.params.wavelength, ref_alt, top, dz, lib)
            want = slm.zenith_column(setting, ref_alt, top, dz)
            assert same(got, want), (ref_alt, top, dz, got, want)
    cfg = cfg_of("SimpleSphere")
    assert round(generators.sky_zenith_column(cfg.atmosphere, cfg.params.wavelength, 0.0, 100000.0, 100.0, lib), 8) == 2.34687220


def test_shade_host_equals_the_model(lib):
    """The grid: body centre, mu = 0.5, the limb from inside and outside, just outside, the second body, no body; X from 0.7 to 40;
    the default parameters, a saturating airlight, no and full limb darkening, no extinction."""
    z0 = 2.3468722043030965
    counts, saturated = {}, 0
    for bodies in lc.SHADE_BODIES:
        for params in lc.SHADE_PARAMS:
            sh = generators.sky_shade_params(z0, **params)
            for az, el in lc.SHADE_DIRECTIONS:
                for x in lc.AIR_MASSES:
                    got = generators.sky_shade_host(sh, bodies, az, el, x * z0, lib)
                    want = slm.shade_pixel(z0, bodies, az, el, x * z0, **params)
                    assert got == want, (bodies, params, az, el, x, got, want)
                    assert got[0] == generators.sky_body_host(bodies, az, el, lib)  # the body rule, unchanged
                    counts[got[0]] = counts.get(got[0], 0) + 1
                    saturated += got[0] == 0 and 255 in got[1]
    print(f"sky light shade host: bodies {counts}, {saturated} saturated airlight pixels")
    assert counts[0] > 0 and counts[1] > 0 and counts[2] > 0 and saturated > 0
    sh = generators.sky_shade_params(z0)
    for column in (math.nan, -z0, 0.0, math.inf):
        assert generators.sky_shade_host(sh, [lc.SUN], 100.0, 3.0, column, lib) == slm.shade_pixel(z0, [lc.SUN], 100.0, 3.0, column)
        assert generators.sky_shade_host(sh, [], 100.0, 3.0, column, lib) == slm.shade_pixel(z0, [], 100.0, 3.0, column)
    assert generators.sky_shade_host(sh, [], 10.0, 80.0, z0, lib)[1] == (59, 106, 217)


def test_refusals(lib):
    cfg = cfg_of("SimpleSphere")
    atm, earth, wl = cfg.atmosphere, cfg.params.earth, cfg.params.wavelength
    bad, nan, inf = _abi.ERR_INVALID_ARGUMENT, math.nan, math.inf
    out, column = _abi.SkyRay(77, 77, 77.0), C.c_double(77.0)
    good = generators.sky_spec(1000.0, 100000.0, 0.0, 1500)

    def ray(spec=good, h0=1000.0, e=1.0, atm_p=C.byref(atm), earth_p=C.byref(earth), out_p=C.byref(out), col_p=C.byref(column)):
        return lib.atmrt_sky_light_ray_host(atm_p, wl, earth_p, 0, None if spec is None else C.byref(spec), h0, e, out_p, col_p)

    assert ray() == 0 and out.status == slm.EXIT and column.value > 0.0
    out.status, out.steps, out.true_elevation, column.value = 77, 77, 77.0, 77.0
    assert ray(atm_p=None) == bad and ray(earth_p=None) == bad and ray(spec=None) == bad and ray(out_p=None) == bad and ray(col_p=None) == bad
    for step, top, floor, m in ((0.0, 1e5, 0.0, 1500), (-1.0, 1e5, 0.0, 1500), (nan, 1e5, 0.0, 1500), (1000.0, inf, 0.0, 1500), (1000.0, 1e5, 1e5, 1500),
                                (1000.0, 1e5, 0.0, 0), (1000.0, 1e5, 0.0, 1048576)):
        assert ray(spec=generators.sky_spec(step, top, floor, m)) == bad, (step, top, floor, m)
    assert ray(h0=nan) == bad and ray(h0=inf) == bad
    assert (out.status, out.steps, out.true_elevation, column.value) == (77, 77, 77.0, 77.0)
    assert ray(e=nan) == 0 and (out.status, out.steps) == (slm.LOST, 0) and math.isnan(column.value)  # no error: LOST at step 0

    z = C.c_double(77.0)
    assert lib.atmrt_sky_zenith_column_host(C.byref(atm), wl, 0.0, 1e5, 100.0, C.byref(z)) == 0 and z.value > 2.0
    z.value = 77.0
    assert lib.atmrt_sky_zenith_column_host(None, wl, 0.0, 1e5, 100.0, C.byref(z)) == bad
    assert lib.atmrt_sky_zenith_column_host(C.byref(atm), wl, 0.0, 1e5, 100.0, None) == bad
    for ref_alt, top, dz in ((0.0, 1e5, 0.0), (0.0, 1e5, -1.0), (0.0, 1e5, nan), (0.0, 1e5, inf), (1e5, 1e5, 100.0), (2e5, 1e5, 100.0), (nan, 1e5, 100.0),
                             (-inf, 1e5, 100.0), (0.0, inf, 100.0), (0.0, nan, 100.0), (0.0, 1e5, 0.09)):
        assert not slm.zenith_valid(ref_alt, top, dz)
        assert lib.atmrt_sky_zenith_column_host(C.byref(atm), wl, ref_alt, top, dz, C.byref(z)) == bad, (ref_alt, top, dz)
    assert z.value == 77.0
    assert lib.atmrt_sky_zenith_column_host(C.byref(atm), wl, 0.0, 1048575.0, 1.0, C.byref(z)) == 0  # K = 1 048 575: the last one accepted
    assert lib.atmrt_sky_zenith_column_host(C.byref(atm), wl, 0.0, 1048575.5, 1.0, C.byref(z)) == bad

    body, rgb = C.c_uint32(77), (C.c_uint8 * 3)(7, 7, 7)
    one = (_abi.SkyBody * 1)(generators.sky_body(100.0, 3.0))
    sh = generators.sky_shade_params(2.3468722)

    def shade(shade_p=C.byref(sh), bodies=one, n=1, body_p=C.byref(body), rgb_p=rgb):
        return lib.atmrt_sky_shade_host(shade_p, bodies, n, 100.0, 3.0, 2.3468722, body_p, rgb_p)

    assert shade() == 0 and body.value == 1 and tuple(rgb) != (7, 7, 7)
    body.value, rgb[0], rgb[1], rgb[2] = 77, 7, 7, 7
    assert shade(shade_p=None) == bad and shade(bodies=None) == bad and shade(body_p=None) == bad and shade(rgb_p=None) == bad
    many = (_abi.SkyBody * 33)(*[generators.sky_body(100.0, 3.0)] * 33)
    assert shade(bodies=many, n=33) == bad
    assert shade(bodies=(_abi.SkyBody * 1)(generators.sky_body(100.0, 3.0, 90.0))) == bad
    for kw in (dict(zenith_column=0.0), dict(zenith_column=-1.0), dict(zenith_column=nan), dict(zenith_column=inf), dict(tau=(0.1, -0.1, 0.1)),
               dict(tau=(nan, 0.1, 0.1)), dict(tau=(0.1, 0.1, inf)), dict(limb=(0.5, 1.5, 0.5)), dict(limb=(-0.1, 0.5, 0.5)), dict(limb=(0.5, 0.5, nan)),
               dict(exposure=-1.0), dict(exposure=nan), dict(exposure=inf)):
        args = dict(zenith_column=2.3468722)
        args.update(kw)
        assert not slm.shade_valid(args["zenith_column"], args.get("tau", slm.TAU), args.get("limb", slm.LIMB), args.get("exposure", slm.EXPOSURE))
        assert shade(shade_p=C.byref(generators.sky_shade_params(**args))) == bad, kw
    assert body.value == 77 and tuple(rgb) == (7, 7, 7)
    assert shade(bodies=None, n=0) == 0 and body.value == 0
    # the entry points refuse a NULL context before they look at anything else
    buf = np.zeros(64, dtype=np.uint64)
    p = buf.ctypes.data
    light = generators.sky_light_spec(sky=good)
    assert lib.atmrt_sky_light_rays(None, C.byref(good), 1000.0, 4, p, p, p, None) == bad
    assert lib.atmrt_sky_light(None, C.byref(light), p, p, p, p, None, None) == bad
    assert lib.atmrt_sky_light_device(None, C.byref(light), p, p, p, p, None, None) == bad
    assert lib.atmrt_sky_light_planes_device(None, C.byref(light), 1000.0, 8, p, p, p, p, p, p, None, None) == bad
    assert lib.atmrt_sky_shade(None, C.byref(sh), one, 1, p, p, p, p, p) == bad
    assert lib.atmrt_sky_shade_device(None, C.byref(sh), one, 1, p, p, p, p, p) == bad
    assert lib.atmrt_sky_shade_planes_device(None, C.byref(sh), one, 1, 8, p, p, p, p, p, p) == bad
    assert lib.atmrt_last_sky_shade_timing(None, C.byref(C.c_double())) == bad
    assert not buf.any()
