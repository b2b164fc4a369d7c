"""The host half of the cast shadows (include/atmrt.h): names and struct sizes, what the entry points refuse without a context, and
generators.light_from_coloring against the light vector of atmrt_coloring_from_conf.  The library loads without a GPU; nothing here
touches a device.  The refusals that need a context (and atmrt_shadow_steps against the model's lattice) are in
tests/test_gpu_shadows.py: without a device atmrt_ctx_create fails with ATMRT_ERR_NO_DEVICE (tests/test_abi.py)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import shadow_model as sm
from atm_raytracer_amd import _abi, _lib, config, generators

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("atmrt_shadow_steps", "atmrt_shadow_mask_device", "atmrt_shadow_mask", "atmrt_shadow_mask_planes_device", "atmrt_draw_image_shadowed",
         "atmrt_draw_image_shadowed_device", "atmrt_last_shadow_timings")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_names_and_struct_sizes(lib):
    header = open(os.path.join(ROOT, "include", "atmrt.h")).read()
    declared = set(re.findall(r"\b(atmrt_[a-z0-9_]+)\s*\(", header))
    for name in NAMES:
        assert name in declared and name in _lib.EXPORTED and hasattr(lib, name), name
    assert lib.atmrt_abi_sizeof(35) == C.sizeof(_abi.ShadowSpec) == 32
    assert lib.atmrt_abi_sizeof(36) == C.sizeof(_abi.ShadowStats) == 40
    assert lib.atmrt_abi_sizeof(34) == 0 and lib.atmrt_abi_sizeof(37) == 0
    spec_body = re.search(r"typedef struct atmrt_shadow_spec \{(.*?)\} atmrt_shadow_spec_t;", header, re.S).group(1)
    assert [n for n, _ in _abi.ShadowSpec._fields_] == re.findall(r"double (\w+);", spec_body) == ["azimuth_deg", "elevation_deg", "reach", "lift"]
    assert [n for n, _ in _abi.ShadowStats._fields_] == ["none", "lit", "shadowed", "integrated_steps", "escaped_rays"]
    for text in ("ATMRT_SHADOW_NONE = 0", "ATMRT_SHADOW_LIT = 1", "ATMRT_SHADOW_SHADOWED = 2", "uint64_t none, lit, shadowed, integrated_steps, escaped_rays;"):
        assert text in header, text
    assert (_abi.SHADOW_NONE, _abi.SHADOW_LIT, _abi.SHADOW_SHADOWED) == (sm.NONE, sm.LIT, sm.SHADOWED) == (0, 1, 2)
    assert lib.atmrt_abi_version() == 5
    # the header states the simplification and its size
    assert "cast shadows" in header and "same in the local frame of every surface point" in header and "1.8 degrees" in header


def test_entry_points_refuse_a_null_context(lib):
    spec = generators.shadow_spec(100.0, 2.0, 20_000.0)
    buf = np.zeros(64, dtype=np.uint8)
    col = _abi.Coloring()
    p = buf.ctypes.data
    assert lib.atmrt_shadow_steps(None, 100.0, C.byref(C.c_int32())) == _abi.ERR_INVALID_ARGUMENT
    assert lib.atmrt_shadow_mask(None, C.byref(spec), p, None, None) == _abi.ERR_INVALID_ARGUMENT
    assert lib.atmrt_shadow_mask_device(None, C.byref(spec), p, None, None) == _abi.ERR_INVALID_ARGUMENT
    assert lib.atmrt_shadow_mask_planes_device(None, C.byref(spec), 8, p, p, p, p, p, None, None) == _abi.ERR_INVALID_ARGUMENT
    assert lib.atmrt_draw_image_shadowed(None, C.byref(col), p, p) == _abi.ERR_INVALID_ARGUMENT
    assert lib.atmrt_draw_image_shadowed_device(None, C.byref(col), p, p) == _abi.ERR_INVALID_ARGUMENT
    assert lib.atmrt_last_shadow_timings(None, (C.c_double * 3)()) == _abi.ERR_INVALID_ARGUMENT
    assert not buf.any()


EARTHS = ["SimpleSphere", {"Spherical": {"radius": 6371000.0}}, "Wgs84", "AzimuthalEquidistant", "FlatDistorted"]


@pytest.mark.parametrize("earth", EARTHS, ids=[e if isinstance(e, str) else next(iter(e)) for e in EARTHS])
def test_light_from_coloring_is_the_vector_of_coloring_from_conf(lib, oracle_det, earth):
    """atmrt_coloring_from_conf's light vector, resolved in the OBSERVER's frame with the oracle's world_directions, points along
    (azimuth, elevation) of light_from_coloring: north = cos(el) cos(az), east = cos(el) sin(az), up = sin(el).  The vector is
    normalised and the basis orthonormal, so the components agree to rounding: 1e-12."""
    rng = np.random.default_rng(12)
    for _ in range(25):
        direction, zenith, light_dir = float(rng.uniform(0, 360)), float(rng.uniform(1.0, 89.0)), float(rng.uniform(-180, 360))
        cfg = config.Config.from_dict({
            "view": {"position": {"latitude": float(rng.uniform(-60, 60)), "longitude": float(rng.uniform(-170, 170)), "altitude": {"Absolute": 100.0}},
                     "frame": {"direction": direction, "fov": 30.0, "tilt": 0.0, "max_distance": 10_000.0}},
            "earth_shape": earth, "output": {"width": 8, "height": 8, "generator": "Fast"}})
        p = cfg.params
        conf = dict(kind=1, water_level=0.0, ambient_light=0.3, light_zenith_angle=zenith, light_dir=light_dir, palette=0, has_fog=0, fog_distance=1.0)
        col = generators.into_coloring(lib, p, conf)
        v = np.array(list(col.light_dir))
        n, e, u = oracle_det.world_directions(p.earth, p.position.latitude, p.position.longitude)
        az, el = generators.light_from_coloring(p, zenith, light_dir)
        assert el == 90.0 - zenith and az == direction + 180.0 - light_dir
        a, b = math.radians(az), math.radians(el)
        want = np.array([math.cos(b) * math.cos(a), math.cos(b) * math.sin(a), math.sin(b)])
        got = np.array([v @ n, v @ e, v @ u])
        assert np.abs(got - want).max() < 1e-12, (earth, direction, zenith, light_dir, got, want)
