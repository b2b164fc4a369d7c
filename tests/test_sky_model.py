"""tests/sky_model.py alone, without a GPU: the rule of include/atmrt.h, "sky rays", over the oracle's stepper reproduces the figures
the feature was specified with, and the frames and lists of tests/sky_cases.py hold what their GPU cases are about."""
import math
import struct

import numpy as np
import pytest

import sky_cases as sc
import sky_model as sm
from atm_raytracer_amd import config
from util import run_oracle


def earth_pod(earth):
    return config.Config.from_dict({
        "view": {"position": {"latitude": 0.0, "longitude": 0.0, "altitude": {"Absolute": 100.0}},
                 "frame": {"direction": 0.0, "fov": 30.0, "tilt": 0.0, "max_distance": 10_000.0}},
        "earth_shape": earth, "output": {"width": 8, "height": 8, "generator": "Fast"}}).params.earth


@pytest.fixture(scope="module")
def sphere(oracle_det):
    return sm.Setting(oracle_det, earth_pod("SimpleSphere"))


# launch elevation -> (exit step, refraction [deg] as the rule was specified: six decimals, the same figure in full as the oracle's
# deterministic stepper gives it): US-76, a sphere of 6371 km, h0 = 1 m, step 100 m, top 100 km
TABLE = {0.0: (11728, 0.551215, 0.5512149973972923), 1.0: (10495, 0.393148, 0.3931479148354846), 5.0: (7035, 0.161330, 0.16133047706616566),
         10.0: (4660, 0.087170, 0.087169990869155), 30.0: (1670, 0.027477, 0.02747693394135453), 60.0: (568, 0.009191, 0.009190896545305804)}
ANGLES = (0.0, 1.0, 2.0, 5.0, 10.0, 20.0, 30.0, 45.0, 60.0)


def test_the_table_reproduces(sphere):
    for e, (steps, printed, refraction) in TABLE.items():
        status, n, true = sm.ray(sphere, 1.0, e, 100.0)
        print(f"sky table {e:g}: exit step {n}, refraction {e - true!r}")
        assert status == sm.EXIT and n == steps
        assert round(refraction, 6) == printed and abs((e - true) - refraction) <= 1e-9 * refraction


def test_the_libm_flavour_agrees(sphere, oracle_libm):
    libm = sm.Setting(oracle_libm, earth_pod("SimpleSphere"))
    for e in TABLE:
        a, b = sm.ray(sphere, 1.0, e, 100.0), sm.ray(libm, 1.0, e, 100.0)
        assert a[:2] == b[:2] and a[0] == sm.EXIT
        assert abs(a[2] - b[2]) <= 1e-9 * abs(a[2]) and abs((e - a[2]) - (e - b[2])) <= 1e-9 * (e - a[2])
    for e, m in ((-1.0, sm.M_MAX), (-0.5, sm.M_MAX), (0.0, 100), (89.9, sm.M_MAX), (90.0, sm.M_MAX)):
        a, b = sm.ray(sphere, 1000.0, e, 1000.0, m=m), sm.ray(libm, 1000.0, e, 1000.0, m=m)
        assert a[:2] == b[:2]


def test_bennett_and_monotony(sphere):
    last = math.inf
    for e in ANGLES:
        status, _, true = sm.ray(sphere, 1.0, e, 100.0)
        refraction, ratio = e - true, (e - true) / sm.bennett(e)
        print(f"sky bennett {e:g}: {refraction:.6f} deg, ratio {ratio:.3f}")
        assert status == sm.EXIT and 0.96 <= ratio <= 1.01
        assert refraction < last
        last = refraction


def test_straight_rays(oracle_det):
    s = sm.Setting(oracle_det, earth_pod("SimpleSphere"), straight=True)
    R = s.radius
    for e in (0.0, 1.0, 7.3, 45.0, -0.2):
        status, n, true = sm.ray(s, 1000.0, e, 1000.0)
        assert status == sm.EXIT and struct.pack("d", true) == struct.pack("d", e)
        # the closed form: h(x) = (R + h0) cos(a) / cos(a + x / R) - R reaches the top at x = R (acos((R + h0) cos(a) / (R + top)) - a)
        a = math.radians(e)
        x = R * (math.acos((R + 1000.0) * math.cos(a) / (R + 100000.0)) - a)
        assert n == math.ceil(x / 1000.0) or abs(x / 1000.0 - round(x / 1000.0)) < 1e-6, (e, n, x)


def test_ground_exit_inside_lost(sphere, oracle_det):
    assert sm.ray(sphere, 1000.0, -1.0, 1000.0)[:2] == (sm.GROUND, 84)
    assert sm.ray(sphere, 1000.0, -0.5, 1000.0)[0] == sm.EXIT
    flat = sm.Setting(oracle_det, earth_pod("FlatDistorted"))
    assert flat.spherical is False
    assert sm.ray(flat, 1000.0, 1.0, 1000.0)[0] == sm.GROUND
    status, n, true = sm.ray(sphere, 1.0, 0.0, 100.0, m=100)
    assert (status, n) == (sm.INSIDE, 100) and math.isnan(true)
    status, n, true = sm.ray(sphere, 1.0, 89.9, 1000.0)
    assert status == sm.LOST and n >= 1 and math.isnan(true)
    for e in (90.0, -90.0, 135.0, math.nan, math.inf):
        assert sm.ray(sphere, 1.0, e, 1000.0)[:2] == (sm.LOST, 0)


def test_the_body_rule():
    sun = (100.0, 3.0, 0.2666, (255, 240, 200))
    moon = (100.3, 3.0, 0.2666, (200, 200, 220))
    assert sm.body_of([sun], 100.0, 3.0) == 1
    assert sm.body_of([sun], 100.0, 3.0 + 0.2666 - 1e-9) == 1 and sm.body_of([sun], 100.0, 3.0 + 0.2666 + 1e-9) == 0
    assert sm.body_of([sun, moon], 100.15, 3.0) == 1 and sm.body_of([moon, sun], 100.15, 3.0) == 1  # the first body wins
    assert sm.body_of([sun, moon], 100.5, 3.0) == 2 and sm.body_of([], 100.0, 3.0) == 0


@pytest.fixture(scope="module")
def frames(oracle_det):
    made = {}

    def get(name):
        if name not in made:
            cfg, tiles = sc.FRAMES[name]()
            res = run_oracle(oracle_det, cfg, tiles)
            made[name] = (cfg, res, sm.frame(sm.Setting.of_config(oracle_det, cfg), res, sc.H0, sc.STEP, sc.TOP, sc.FLOOR, sc.M))
        return made[name]

    return get


@pytest.mark.parametrize("name", sorted(sc.FRAMES))
def test_the_frames_hold_what_their_cases_are_about(frames, name):
    cfg, res, want = frames(name)
    n, st = sc.W * sc.H, want.stats
    print(f"sky frame {name}: {st}")
    assert cfg.params.position.altitude == sc.H0 and float(np.nanmax(res["elevation_angle"])) <= 60.0
    assert sum(st[k] for k in ("none", "exit", "ground", "inside", "lost")) == n
    if name == "all_sky":
        assert st["none"] == 0 and st["exit"] == n
    elif name == "no_sky":
        assert st["none"] == n and st["integrated_steps"] == 0
    else:
        assert 0.3 * n <= n - st["none"] <= 0.7 * n  # about half of the pixels are sky
    if name in sc.US76_SPHERE:
        assert st["lost"] == 0 and st["inside"] == 0
    if name not in ("no_sky", "flat"):
        # a wavefront of the compacted list (64 consecutive sky pixels) holds more than one exit step
        steps = want.steps.ravel()[np.asarray(res["hit_count"]).ravel() == 0]
        assert len(set(steps[:64].tolist())) > 1
    if name == "straight":
        sky = np.asarray(res["hit_count"]) == 0
        assert want.true_elevation[sky].tobytes() == np.asarray(res["elevation_angle"])[sky].tobytes() or st["ground"] > 0


def test_the_lists_hold_every_status(sphere):
    for n in sc.LIST_LENGTHS:
        want = sm.rays(sphere, sc.LIST_H0, sc.list_elevations(n), sc.STEP, sc.TOP, sc.FLOOR, sc.M)
        short = sm.rays(sphere, sc.LIST_H0, sc.list_elevations_short(n), sc.STEP, sc.TOP, sc.FLOOR, sc.SHORT_M)
        if n >= 63:
            assert want.stats["ground"] > 0 and want.stats["exit"] > 0 and want.stats["none"] == 0
            first = short.status.ravel()[:63]
            assert {sm.GROUND, sm.EXIT, sm.INSIDE} <= set(first.tolist())
