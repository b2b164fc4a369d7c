"""One wrong call per entry point of the sight lines, the viewshed, the viewshed map, the horizon and the cast shadows: the status and
the whole message.  Every call is wrong in two ways, so that the message also pins which check comes first.  The strings are those of
the commit before these calls shared their host code (one planner, one batch driver, one shadow body), read from its argument checks
and confirmed by running this file against a library built from that commit."""
import ctypes as C

import pytest

from atm_raytracer_amd import _abi, generators, synth

pytestmark = pytest.mark.gpu

INVALID, STATE = -1, -6
NAN = float("nan")


def spec_v(**over):
    v = dict(az_lo_deg=0.0, az_step_deg=10.0, reach=5_000.0, height=0.0, fan_lo_deg=-6.0, fan_hi_deg=6.0, n_az=4, fan_rays=64)
    v.update(over)
    return C.byref(_abi.ViewshedSpec(**v))


def spec_h(**over):
    v = dict(az_lo_deg=0.0, az_step_deg=10.0, reach=5_000.0, fan_lo_deg=-6.0, fan_hi_deg=6.0, n_az=4, fan_rays=64, rounds=2)
    v.update(over)
    return C.byref(_abi.HorizonSpec(**v))


def wrong_calls(lib, h):
    """(entry point, its arguments after the context, status, message); `some`: a pointer that is not NULL and is never followed"""
    buf = (C.c_double * 8)()
    some = C.addressof(buf)
    target = _abi.SightTarget(10.0, -1.0, 0.0)
    bad_grid = C.byref(generators.GeoGrid(46.0, 8.0, 0.0, 0.01, 4, 4))
    shadow = C.byref(_abi.ShadowSpec(10.0, 90.0, 5_000.0, -1.0))
    lights = C.byref(_abi.ShadowLightsSpec(C.cast(buf, C.POINTER(C.c_double)), 0, 0, 5_000.0, -1.0))
    return [
        # a fan that is not finite, and no rounds
        ("atmrt_sight_lines", (some, 1, NAN, 1.0, 0, some), INVALID, "the fan must be finite, increasing and at most 180 degrees wide"),
        # no angles, and a target at a negative distance
        ("atmrt_sight_fan_probe", (C.byref(target), 0, some, some), INVALID, "the number of angles must lie in [1, 4096]"),
        # no spec, and no k_star
        ("atmrt_viewshed", (None, None, some, some, None, None, None, None), INVALID, "atmrt_viewshed: spec is NULL"),
        # no azimuths, and a fan of 65 rays
        ("atmrt_viewshed_device", (spec_v(n_az=0, fan_rays=65), some, some, some, None, None, None, None), INVALID,
         "atmrt_viewshed_device: n_az must lie in [1, 65536]"),
        # nowhere to put m, and a reach that is not a number
        ("atmrt_viewshed_steps", (NAN, None), INVALID, "atmrt_viewshed_steps: m is NULL"),
        # no spec, and a grid whose cells have no height
        ("atmrt_viewshed_map", (None, bad_grid, 0, some, some, None, None), INVALID, "atmrt_viewshed_map: spec is NULL"),
        ("atmrt_viewshed_map_device", (None, bad_grid, 0, some, some, None, None), INVALID, "atmrt_viewshed_map_device: spec is NULL"),
        # no grid, and samples without a status plane
        ("atmrt_viewshed_map_planes_device", (None, 4, None, some, some, some, 0, some, some, None, None), INVALID,
         "atmrt_viewshed_map_planes_device: grid, n_samples or n_seen is NULL"),
        # no rounds, and no azimuths
        ("atmrt_horizon", (spec_h(rounds=0, n_az=0), some), INVALID, "atmrt_horizon: rounds must lie in [1, 4]"),
        ("atmrt_horizon_device", (spec_h(rounds=0, n_az=0), some), INVALID, "atmrt_horizon_device: rounds must lie in [1, 4]"),
        # a light at the zenith, and a negative lift
        ("atmrt_shadow_mask", (shadow, some, None, None), INVALID, "atmrt_shadow_mask: elevation_deg must lie strictly between -90 and 90"),
        ("atmrt_shadow_mask_device", (shadow, some, None, None), INVALID, "atmrt_shadow_mask: elevation_deg must lie strictly between -90 and 90"),
        # no pixels, and no spec
        ("atmrt_shadow_mask_planes_device", (None, 0, some, some, some, some, some, None, None), INVALID,
         "atmrt_shadow_mask_planes_device: n_pixels must lie in [1, 2^32 - 1]"),
        # no lights, and a negative lift
        ("atmrt_shadow_lights", (lights, some, None, None, None), INVALID, "atmrt_shadow_lights: n_lights must lie in [1, 64], not 0"),
        ("atmrt_shadow_lights_device", (lights, some, None, None, None), INVALID, "atmrt_shadow_lights: n_lights must lie in [1, 64], not 0"),
        # no hit_count plane, and no pixels
        ("atmrt_shadow_lights_planes_device", (lights, 0, None, some, some, some, some, None, None, None), INVALID,
         "atmrt_shadow_lights_planes_device: a plane is NULL"),
    ]


def test_a_wrong_call_gets_the_status_and_the_message_it_got(gpu_ctx):
    cfg, tiles = synth.scene("S2", 64, 48, generator="Fast", max_distance=60_000.0)
    gpu_ctx.check(gpu_ctx.lib.atmrt_terrain_clear(gpu_ctx.handle))
    generators.make_generator(generators.Params(cfg), generators.Terrain.from_tiles(tiles, gpu_ctx))._configure()
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    for name, args, status, message in wrong_calls(lib, h):
        rc = getattr(lib, name)(h, *args)
        got = lib.atmrt_last_error(h).decode()
        print(f"wrong call {name}: {rc} {got!r}")
        assert (rc, got) == (status, message), name


def test_the_step_count_refuses_a_reach_before_it_asks_for_parameters():
    """a context nothing was set on: the reach is checked first, the state second"""
    ctx = generators.Context(0)
    try:
        m = C.c_int32(-7)
        assert ctx.lib.atmrt_shadow_steps(ctx.handle, -1.0, C.byref(m)) == INVALID
        assert ctx.lib.atmrt_last_error(ctx.handle).decode() == "atmrt_shadow_steps: reach must be finite and positive"
        assert ctx.lib.atmrt_shadow_steps(ctx.handle, 1_000.0, C.byref(m)) == STATE
        assert ctx.lib.atmrt_last_error(ctx.handle).decode() == "atmrt_shadow_steps: atmrt_set_params has not been called"
        # the viewshed's asks for the parameters first
        assert ctx.lib.atmrt_viewshed_steps(ctx.handle, -1.0, C.byref(m)) == STATE
        assert ctx.lib.atmrt_last_error(ctx.handle).decode() == "atmrt_viewshed_steps: atmrt_set_params has not been called"
        assert m.value == -7  # a refused call leaves m alone
    finally:
        ctx.close()
