"""The host half of the shadow lights (include/atmrt.h, "shadow lights"): names and struct sizes, and the two host functions —
atmrt_shadow_local_direction (the function the kernel runs) and atmrt_shadow_light_direction — against tests/shadow_lights_model.py
bit for bit.  The library loads without a GPU; nothing here touches a device.  The refusals that need a context are in
tests/test_gpu_shadow_lights.py."""
import ctypes as C
import math
import os
import re
import struct

import numpy as np
import pytest

import shadow_lights_model as slm
from atm_raytracer_amd import _abi, _lib, config, generators

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("atmrt_shadow_light_direction", "atmrt_shadow_local_direction", "atmrt_shadow_lights_device", "atmrt_shadow_lights",
         "atmrt_shadow_lights_planes_device")
EARTHS = ["SimpleSphere", {"Spherical": {"radius": 3.0e6}}, "Wgs84", {"Ellipsoid": {"a": 6378137.0, "b": 6300000.0}},
          "AzimuthalEquidistant", "FlatDistorted", {"ObserverAe": {"proj_radius": 6371000.0}}, "SimpleObserverAe"]  # all 8 models
IDS = [e if isinstance(e, str) else next(iter(e)) for e in EARTHS]
SPHERICAL_FAMILY = EARTHS[:4]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def earth_pod(earth):
    return config.Config.from_dict({
        "view": {"position": {"latitude": 0.0, "longitude": 0.0, "altitude": {"Absolute": 100.0}},
                 "frame": {"direction": 0.0, "fov": 30.0, "tilt": 0.0, "max_distance": 10_000.0}},
        "earth_shape": earth, "output": {"width": 8, "height": 8, "generator": "Fast"}}).params.earth


def bits(*xs):
    return struct.pack(f"{len(xs)}d", *[float(x) for x in xs])


def test_names_and_struct_sizes(lib):
    header = open(os.path.join(ROOT, "include", "atmrt.h")).read()
    declared = set(re.findall(r"\b(atmrt_[a-z0-9_]+)\s*\(", header))
    for name in NAMES:
        assert name in declared and name in _lib.EXPORTED and hasattr(lib, name), name
    assert lib.atmrt_abi_sizeof(38) == C.sizeof(_abi.ShadowLightsSpec) == 32
    assert lib.atmrt_abi_sizeof(37) == 0 and lib.atmrt_abi_sizeof(39) == 0
    assert [n for n, _ in _abi.ShadowLightsSpec._fields_] == ["dir", "n_lights", "_pad", "reach", "lift"]
    assert (_abi.ShadowLightsSpec.dir.offset, _abi.ShadowLightsSpec.n_lights.offset, _abi.ShadowLightsSpec.reach.offset,
            _abi.ShadowLightsSpec.lift.offset) == (0, 8, 16, 24)
    assert lib.atmrt_abi_version() == 5  # the additions are additive
    # the header states the rule in a section of its own and no longer promises it
    assert "shadow lights" in header and "A direction per point is a later change" not in header


def triples(rng, n):
    """(lat, lon, light): seeded, then the poles, the date line, the axes and the scaled lights."""
    out = [(float(rng.uniform(-90, 90)), float(rng.uniform(-180, 180)), rng.normal(size=3) * float(10.0 ** rng.uniform(-3, 3))) for _ in range(n)]
    axes = [np.array(v, dtype=np.float64) for v in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
    for lat in (90.0, -90.0, 0.0, 46.5):
        for lon in (180.0, -180.0, 0.0, 8.5):
            for v in axes:
                out.append((lat, lon, v))
            w = rng.normal(size=3)
            out += [(lat, lon, w), (lat, lon, w * 1e-150), (lat, lon, w * 1e150)]
    return out


@pytest.mark.parametrize("earth", EARTHS, ids=IDS)
def test_local_direction_equals_the_model_bit_for_bit(lib, oracle_det, earth):
    pod = earth_pod(earth)
    cases = triples(np.random.default_rng(77), 400)  # 8 models x 496 triples
    for lat, lon, v in cases:
        L = slm.normalise(v)
        assert L is not None
        want = slm.local_direction(oracle_det, pod, L, lat, lon)
        got = generators.shadow_local_direction(pod, v, lat, lon, lib)
        assert bits(*got) == bits(*want), (earth, lat, lon, v, got, want)
        assert math.isnan(got[1]) or -90.0 <= got[1] <= 90.0


@pytest.mark.parametrize("earth", EARTHS, ids=IDS)
def test_light_direction_equals_the_model_bit_for_bit(lib, oracle_det, earth):
    pod = earth_pod(earth)
    rng = np.random.default_rng(78)
    places = [(float(rng.uniform(-90, 90)), float(rng.uniform(-180, 180))) for _ in range(300)] + \
        [(lat, lon) for lat in (90.0, -90.0, 0.0) for lon in (180.0, -180.0, 0.0)]
    for lat, lon in places:
        az, el = float(rng.uniform(-400, 800)), float(rng.choice([rng.uniform(-90, 90), 90.0, -90.0, 0.0]))
        want = slm.light_direction(oracle_det, pod, lat, lon, az, el)
        got = generators.shadow_light_direction(pod, lat, lon, az, el, lib)
        assert got.tobytes() == want.tobytes(), (earth, lat, lon, az, el, got, want)


def test_the_exact_zenith_and_nadir(lib, oracle_det):
    pod = earth_pod("SimpleSphere")
    assert generators.shadow_local_direction(pod, (1.0, 0.0, 0.0), 0.0, 0.0, lib)[1] == 90.0
    assert generators.shadow_local_direction(pod, (-1.0, 0.0, 0.0), 0.0, 0.0, lib)[1] == -90.0
    assert generators.shadow_local_direction(pod, (3.0e150, 0.0, 0.0), 0.0, 0.0, lib)[1] == 90.0
    assert slm.local_direction(oracle_det, pod, (1.0, 0.0, 0.0), 0.0, 0.0)[1] == 90.0
    assert slm.local_direction(oracle_det, pod, (-1.0, 0.0, 0.0), 0.0, 0.0)[1] == -90.0


@pytest.mark.parametrize("earth", SPHERICAL_FAMILY, ids=IDS[:4])
def test_round_trip_on_the_spherical_family(lib, earth):
    """light_direction at a place from (az, el), then local_direction at the same place: az (mod 360) and el within 1e-9 degrees
    for |el| <= 89.  Not bitwise: the chain is a few dozen rounded operations at 2^-53 relative on angles of at most 360 degrees
    (1e-13 degrees each at the worst, amplified by 1 / cos(el) <= 57 in the azimuth): it cannot reach 1e-12, and 1e-9 leaves three
    decades.  Closer to the zenith the azimuth is ill-conditioned and not compared."""
    pod = earth_pod(earth)
    rng = np.random.default_rng(79)
    worst = [0.0, 0.0]
    for _ in range(500):
        lat, lon = float(rng.uniform(-89.9, 89.9)), float(rng.uniform(-180, 180))
        az, el = float(rng.uniform(0, 360)), float(rng.uniform(-89, 89))
        v = generators.shadow_light_direction(pod, lat, lon, az, el, lib)
        az2, el2 = generators.shadow_local_direction(pod, v * float(rng.uniform(0.5, 20.0)), lat, lon, lib)
        d_az = abs((az2 - az + 180.0) % 360.0 - 180.0)
        worst = [max(worst[0], d_az), max(worst[1], abs(el2 - el))]
        assert d_az < 1e-9 and abs(el2 - el) < 1e-9, (earth, lat, lon, az, el, az2, el2)
    print(f"shadow lights round trip {earth}: worst azimuth {worst[0]:.3g}, elevation {worst[1]:.3g} degrees")


def test_refusals(lib):
    pod = earth_pod("SimpleSphere")
    out, az, el = (C.c_double * 3)(7.0, 7.0, 7.0), C.c_double(7.0), C.c_double(7.0)
    good = (C.c_double * 3)(1.0, 2.0, 3.0)
    inf, nan, bad = math.inf, math.nan, _abi.ERR_INVALID_ARGUMENT
    assert lib.atmrt_shadow_light_direction(C.byref(pod), 46.0, 8.0, 100.0, 2.0, out) == 0 and out[0] != 7.0
    out[:] = [7.0] * 3
    assert lib.atmrt_shadow_light_direction(None, 46.0, 8.0, 100.0, 2.0, out) == bad
    assert lib.atmrt_shadow_light_direction(C.byref(pod), 46.0, 8.0, 100.0, 2.0, None) == bad
    for args in ((nan, 8.0, 100.0, 2.0), (46.0, inf, 100.0, 2.0), (46.0, 8.0, nan, 2.0), (46.0, 8.0, -inf, 2.0), (46.0, 8.0, 100.0, nan),
                 (46.0, 8.0, 100.0, 90.000001), (46.0, 8.0, 100.0, -91.0), (46.0, 8.0, 100.0, inf)):
        assert lib.atmrt_shadow_light_direction(C.byref(pod), *args, out) == bad, args
    assert list(out) == [7.0] * 3
    assert lib.atmrt_shadow_light_direction(C.byref(pod), 46.0, 8.0, 100.0, 90.0, out) == 0
    assert lib.atmrt_shadow_light_direction(C.byref(pod), 46.0, 8.0, 100.0, -90.0, out) == 0
    unknown = _abi.EarthModel()
    C.memmove(C.byref(unknown), C.byref(pod), C.sizeof(pod))
    unknown.kind = 99
    assert lib.atmrt_shadow_light_direction(C.byref(unknown), 46.0, 8.0, 100.0, 2.0, out) == bad
    assert lib.atmrt_shadow_local_direction(C.byref(unknown), good, 46.0, 8.0, C.byref(az), C.byref(el)) == bad

    assert lib.atmrt_shadow_local_direction(C.byref(pod), good, 46.0, 8.0, C.byref(az), C.byref(el)) == 0 and az.value != 7.0
    az.value = el.value = 7.0
    assert lib.atmrt_shadow_local_direction(None, good, 46.0, 8.0, C.byref(az), C.byref(el)) == bad
    assert lib.atmrt_shadow_local_direction(C.byref(pod), None, 46.0, 8.0, C.byref(az), C.byref(el)) == bad
    assert lib.atmrt_shadow_local_direction(C.byref(pod), good, 46.0, 8.0, None, C.byref(el)) == bad
    assert lib.atmrt_shadow_local_direction(C.byref(pod), good, 46.0, 8.0, C.byref(az), None) == bad
    for v in ((0.0, 0.0, 0.0), (nan, 0.0, 1.0), (1.0, inf, 0.0), (0.0, 1.0, -inf), (1e200, 0.0, 0.0), (1e-170, 1e-170, 0.0), (-0.0, 0.0, -0.0)):
        assert slm.normalise(v) is None
        assert lib.atmrt_shadow_local_direction(C.byref(pod), (C.c_double * 3)(*v), 46.0, 8.0, C.byref(az), C.byref(el)) == bad, v
    assert az.value == 7.0 and el.value == 7.0
    # the entry points refuse a NULL context before they look at anything else
    spec, _ = generators.shadow_lights_spec([[1.0, 0.0, 0.0]], 5_000.0)
    buf = np.zeros(64, dtype=np.uint64)
    p = buf.ctypes.data
    assert lib.atmrt_shadow_lights(None, C.byref(spec), p, None, None, None) == bad
    assert lib.atmrt_shadow_lights_device(None, C.byref(spec), p, None, None, None) == bad
    assert lib.atmrt_shadow_lights_planes_device(None, C.byref(spec), 8, p, p, p, p, p, None, None, None) == bad
    assert not buf.any()
