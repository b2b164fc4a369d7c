"""tests/sky_light_model.py alone, without a GPU: the rule of include/atmrt.h, "sky light", over the oracle's stepper and oracle_n
reproduces the air masses the feature was specified with (against Kasten and Young 1989 and against the pressure ratio), a flat
straight-ray column is the zenith column over the sine, and the cases of tests/sky_light_cases.py hold what they are about.

Measured with the oracle's deterministic flavour, US-76, a sphere of 6371 km, h0 = 1 m, step 100 m, top 100 km, Z0 with 100 m nodes
(2.3468722043030965 m): X / Kasten-Young = 1.00778 at 0 degrees, 1.00139 at 0.5, 1.00032 at 1, 1.00142 at 2, 1.00157 at 5, 0.99974 at
10, 0.99969 at 30, 1.00017 at 60, 1.00049 at 80; X(2500 m) / X(1 m) at 30 degrees = 0.737184 beside a pressure ratio of 0.737147."""
import math

import numpy as np
import pytest

import sky_light_cases as lc
import sky_light_model as slm
from atm_raytracer_amd import config
from util import run_oracle


def earth_pod(earth):
    return config.Config.from_dict({
        "view": {"position": {"latitude": 0.0, "longitude": 0.0, "altitude": {"Absolute": 100.0}},
                 "frame": {"direction": 0.0, "fov": 30.0, "tilt": 0.0, "max_distance": 10_000.0}},
        "earth_shape": earth, "output": {"width": 8, "height": 8, "generator": "Fast"}}).params.earth


@pytest.fixture(scope="module")
def sphere(oracle_det):
    return slm.Setting(oracle_det, earth_pod("SimpleSphere"))


# elevation -> the air mass the feature was specified with (step 100 m from 1 m)
TABLE = {0.0: 38.215, 0.5: 31.393, 1.0: 26.319, 2.0: 19.461, 5.0: 10.322, 10.0: 5.5846, 30.0: 1.9937, 60.0: 1.1542, 80.0: 1.0156}


def test_zenith_column(sphere):
    z100, z10, z1000 = (slm.zenith_column(sphere, 0.0, 100000.0, dz) for dz in (100.0, 10.0, 1000.0))
    print(f"sky light zenith column: {z100!r} (100 m), {z10!r} (10 m), {z1000!r} (1000 m)")
    assert round(z100, 8) == 2.34687220 and round(z10, 8) == 2.34684803 and round(z1000, 4) == 2.3493
    # a top that is no multiple of dz: the last node is the top itself
    a, b = slm.zenith_column(sphere, 0.0, 100000.0, 30000.0), slm.zenith_column(sphere, 0.0, 100000.0, 100000.0 / 3.0 + 1.0)
    assert a > z100 and b > z100 and a != b
    for ref_alt, top, dz in ((0.0, 1e5, 0.0), (0.0, 1e5, -1.0), (0.0, 1e5, math.nan), (0.0, 1e5, math.inf), (1e5, 1e5, 100.0), (2e5, 1e5, 100.0),
                             (math.nan, 1e5, 100.0), (0.0, math.inf, 100.0), (0.0, 1e5, 0.09)):
        assert not slm.zenith_valid(ref_alt, top, dz), (ref_alt, top, dz)
    assert slm.zenith_valid(0.0, 1e5, 0.1)


def test_air_mass_against_kasten_young(sphere):
    z0 = slm.zenith_column(sphere, 0.0, 100000.0, 100.0)
    for e, printed in TABLE.items():
        status, _, _, column = slm.ray(sphere, 1.0, e, 100.0)
        x = column / z0
        ratio = x / slm.kasten_young(e)
        print(f"sky light air mass {e:g}: X = {x!r}, X / Kasten-Young = {ratio:.5f}")
        assert status == slm.EXIT
        assert abs(x / printed - 1.0) < 1e-4  # the figures of the specification, to the digits it prints
        if e <= 60.0:
            assert abs(ratio - 1.0) <= (0.01 if e == 0.0 else 0.003)


def test_air_mass_follows_pressure(sphere, oracle_det):
    low, high = slm.ray(sphere, 1.0, 30.0, 100.0)[3], slm.ray(sphere, 2500.0, 30.0, 100.0)[3]
    want = oracle_det.pressure(sphere.env, 2500.0) / oracle_det.pressure(sphere.env, 1.0)
    print(f"sky light 2500 m / 1 m at 30 degrees: {high / low!r}, pressure ratio {want!r}")
    assert abs(high / low - want) <= 1e-3


@pytest.mark.parametrize("e", (10.0, 40.0))
def test_flat_straight_column_is_the_zenith_column_over_the_sine(oracle_det, e):
    """Flat earth, straight rays: the ray's nodes are h0 + i step tan(e), the zenith column's nodes at dz = step tan(e), and every
    path element is dz / sin(e) — up to the step that EXITs, which the march takes whole while Z0 stops at the top: an overshoot
    of at most q(top) dz / Z0 relative, below 1e-7."""
    flat = slm.Setting(oracle_det, earth_pod("FlatDistorted"), straight=True)
    assert flat.spherical is False
    h0, step, top = 1000.0, 1000.0, 100000.0
    dz = step * math.tan(math.radians(e))
    status, _, true, column = slm.ray(flat, h0, e, step, top)
    z0 = slm.zenith_column(flat, h0, top, dz)
    overshoot = slm.q_of(flat, top) * dz / z0
    print(f"sky light flat straight {e:g}: C sin(e) / Z0 - 1 = {column * math.sin(math.radians(e)) / z0 - 1.0:.3g}, overshoot bound {overshoot:.3g}")
    assert status == slm.EXIT and true == e
    assert overshoot < 1e-7
    assert abs(column * math.sin(math.radians(e)) / z0 - 1.0) <= 1e-6


def test_column_is_nan_unless_exit(sphere):
    for e, m, want in ((-1.0, lc.M, slm.GROUND), (0.0, lc.SHORT_M, slm.INSIDE), (89.9, lc.M, slm.LOST), (90.0, lc.M, slm.LOST), (math.nan, lc.M, slm.LOST)):
        status, _, true, column = slm.ray(sphere, lc.LIST_H0, e, lc.STEP, lc.TOP, lc.FLOOR, m)
        assert status == want and math.isnan(true) and math.isnan(column)
    status, steps, true, column = slm.ray(sphere, lc.LIST_H0, 50.0, lc.STEP, lc.TOP, lc.FLOOR, lc.SHORT_M)
    assert status == slm.EXIT and column > 0.0 and steps < lc.SHORT_M


def test_the_march_is_the_sky_rule(sphere):
    import sky_model as sm
    for e in (-1.2, -0.9, -0.5, 0.0, 0.3, 5.0, 50.0, 89.9, 90.0):
        for m in (lc.M, lc.SHORT_M):
            a, b = slm.ray(sphere, lc.LIST_H0, e, lc.STEP, lc.TOP, lc.FLOOR, m), sm.ray(sphere, lc.LIST_H0, e, lc.STEP, lc.TOP, lc.FLOOR, m)
            assert a[:2] == b[:2] and (a[2] == b[2] or (math.isnan(a[2]) and math.isnan(b[2])))


def test_the_lists_hold_every_status(sphere):
    for n in lc.LIST_LENGTHS:
        short = slm.rays(sphere, lc.LIST_H0, lc.list_elevations_short(n), lc.STEP, lc.TOP, lc.FLOOR, lc.SHORT_M)
        long = slm.rays(sphere, lc.LIST_H0, lc.list_elevations(n), lc.STEP, lc.TOP, lc.FLOOR, lc.M)
        for r in (short, long):
            assert (np.isnan(r.column) == (r.status != slm.EXIT)).all() and (r.column[r.status == slm.EXIT] > 0.0).all()
        if n >= 63:
            first = short.status.ravel()[:63]
            assert {slm.GROUND, slm.EXIT, slm.INSIDE} <= set(first.tolist())  # inside one wavefront
            assert long.stats["ground"] > 0 and long.stats["exit"] > 0


def test_the_lifted_sun_is_reddened_and_dimmer(sphere, oracle_det):
    """The lifted sun's disc pixels (true elevation -0.3 degrees, seen from 1000 m) come out R >= G >= B with R > B, and dimmer in
    every channel than the same place on the same disc 30 degrees up."""
    cfg, tiles = lc.lifted_frame()
    res = run_oracle(oracle_det, cfg, tiles)
    setting = slm.Setting.of_config(oracle_det, cfg)
    want = slm.frame(setting, res, lc.LIFTED_H0, lc.STEP, lc.TOP, lc.FLOOR, lc.M)
    assert want.stats["exit"] == lc.W * lc.H
    z0 = slm.zenith_column(setting, lc.REF_ALT, lc.TOP, lc.STEP)
    plain = np.zeros((lc.H, lc.W, 3), dtype=np.uint8)
    body, image = slm.shade(plain, z0, [lc.LIFTED_SUN], res["azimuth"], want.true_elevation, want.status, want.column)
    disc = body == 1
    x = want.column / z0
    print(f"sky light lifted sun: {int(disc.sum())} disc pixels, air mass {x[disc].min():.2f} .. {x[disc].max():.2f}, "
          f"colours {image[disc].min(axis=0).tolist()} .. {image[disc].max(axis=0).tolist()}")
    assert 0 < disc.sum() < lc.W * lc.H
    r, g, b = (image[disc][:, c].astype(int) for c in range(3))
    assert (r >= g).all() and (g >= b).all() and (r > b).all()
    # the same place on the disc (the same offset from the centre) at 30 degrees, with that ray's own column
    high = slm.ray(setting, lc.LIFTED_H0, 30.0, lc.STEP, lc.TOP, lc.FLOOR, lc.M)
    assert high[0] == slm.EXIT and high[3] / z0 < 2.0 < x[disc].min()
    centre = slm.shade_pixel(z0, [lc.HIGH_SUN], lc.HIGH_SUN[0], lc.HIGH_SUN[1], high[3])
    assert centre[0] == 1
    compared = 0
    for y, xx in zip(*np.nonzero(disc)):
        d_az, d_el = float(res["azimuth"][y, xx]) - lc.LIFTED_SUN[0], float(want.true_elevation[y, xx]) - lc.LIFTED_SUN[1]
        on_disc, up = slm.shade_pixel(z0, [lc.HIGH_SUN], lc.HIGH_SUN[0] + d_az / math.cos(math.radians(30.0)), lc.HIGH_SUN[1] + d_el, high[3])
        if on_disc:  # (the offset is carried over in the small-angle form: a pixel on the very limb may fall outside up there)
            compared += 1
            assert all(int(image[y, xx, c]) < up[c] for c in range(3)), (y, xx, image[y, xx], up)
    assert compared >= 0.9 * disc.sum()
    # the sky beside the disc: the airlight at air masses above 20 saturates to white with the default exposure
    assert (image[~disc] == 255).all()


def test_the_shade_grid_holds_what_it_is_about():
    z0 = 2.3468722043030965
    seen, colours = set(), set()
    for bodies in lc.SHADE_BODIES:
        for az, el in lc.SHADE_DIRECTIONS:
            for x in lc.AIR_MASSES:
                for params in lc.SHADE_PARAMS:
                    body, rgb = slm.shade_pixel(z0, bodies, az, el, x * z0, **params)
                    seen.add(body)
                    colours.add(rgb)
    assert seen == {0, 1, 2} and (255, 255, 255) in colours and len(colours) >= 100
    sun = [lc.SUN]
    centre, half, limb_in, limb_out = (slm.shade_pixel(z0, sun, *lc.SHADE_DIRECTIONS[i], z0) for i in range(4))
    assert centre[0] == half[0] == limb_in[0] == 1 and limb_out[0] == 0
    assert all(centre[1][c] > half[1][c] > limb_in[1][c] for c in range(3))  # limb darkening
    # at the centre mu = 1 and the limb term is 1: the colour times the transmittance; on the limb mu is about 0: times 1 - u_c
    t = [math.exp(-tau) for tau in slm.TAU]
    assert all(abs(centre[1][c] - lc.SUN[3][c] * t[c]) <= 1.0 for c in range(3))
    assert all(abs(limb_in[1][c] - lc.SUN[3][c] * t[c] * (1.0 - slm.LIMB[c])) <= 1.0 for c in range(3))
    assert all(abs(half[1][c] - lc.SUN[3][c] * t[c] * (1.0 - slm.LIMB[c] * 0.5)) <= 1.0 for c in range(3))
    zenith = slm.shade_pixel(z0, [], 10.0, 80.0, z0)[1]
    print(f"sky light zenith colour {zenith}, sun centre at X = 1 {centre[1]}, at mu = 0.5 {half[1]}, on the limb {limb_in[1]}")
    assert zenith == (59, 106, 217)
    assert slm.shade_pixel(z0, [], 10.0, 0.0, 38.2 * z0)[1] == (255, 255, 255)
    # bytes outside the range: a NaN column gives 0, a negative one (T > 1, 1 - T < 0) 0 for the airlight
    assert slm.shade_pixel(z0, [], 10.0, 0.0, math.nan)[1] == (0, 0, 0) and slm.shade_pixel(z0, [], 10.0, 0.0, -z0)[1] == (0, 0, 0)
