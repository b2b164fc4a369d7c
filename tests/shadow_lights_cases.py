"""The frames and lights of the shadow-lights tests, in one place: tests/test_gpu_shadow_lights.py runs them on the GPU against
tests/shadow_lights_model.py, and tests/test_shadow_lights_model.py asserts without a GPU — over the oracle's frame — that every
light that is not declared all-lit or all-dark holds both kinds of pixel.  Test infrastructure only.

The frames are tests/shadow_cases.FRAMES (scene S2, 60 km of range, reach 20 km at step 100 m: m = 200).  A light is given as the
angles under which the OBSERVER sees it and turned into a world-frame vector there (lights_from_angles): at a trace point 55 km
away its local elevation differs by up to half a degree."""
import numpy as np

import shadow_cases as sc
import shadow_sweep_cases as ssc

REACH = sc.REACH
BOTH, ALL_LIT, ALL_DARK = "both", "all-lit", "all-dark"
# A light 10 degrees under the observer's horizontal: at most 0.5 degrees less steep at any trace point, its ray falls 3.3 km in
# 20 km from points below 2 km: under the terrain (0 m beyond the mosaic) well before the reach.  All dark by construction.
NEGATIVE = (100.0, -10.0, ALL_DARK)
# A light 45 degrees up climbs 100 m per step: steeper than any slope of the tile.  All lit (the model confirms it).
HIGH = (260.0, 45.0, ALL_LIT)


def _low(elevation):
    return (260.0, elevation, BOTH)


# name -> (frame, [(azimuth_deg, elevation_deg at the observer, what the light is meant to show)], the case is about the shortcut).
# The low western light starts from shadow_cases' (2.0 degrees, 1.5 for the two steep frames) and is moved in steps of 0.25 degrees
# inside [1, 3] where the per-point model misses a share of 5 %: chosen by tests/test_shadow_lights_model.py alone.
CASES = {
    "rect_64x32": ("rect_64x32", [_low(2.0), NEGATIVE, HIGH], True),
    "fast_50x20": ("fast_50x20", [_low(2.0), NEGATIVE, HIGH], False),
    "straight": ("straight", [_low(2.0), NEGATIVE, HIGH], True),
    "flat_distorted": ("flat_distorted", [_low(2.0), NEGATIVE, HIGH], False),
    "ellipsoid": ("ellipsoid", [_low(2.0), NEGATIVE, HIGH], False),
    "spline": ("spline", [_low(2.0), NEGATIVE, HIGH], False),
    "alpha": ("alpha", [_low(2.0), NEGATIVE, HIGH], False),
    "objects": ("objects", [_low(1.5), NEGATIVE, HIGH], False),
    "sky": ("sky", [_low(2.0), NEGATIVE, HIGH], False),
    "ground": ("ground", [_low(1.5), NEGATIVE, HIGH], False),
}

# The frame that tells the two rules apart: the 60 km scene on a sphere of 3000 km, where the local frame turns by a degree
# between the observer and the far trace points.
SMALL_SPHERE = ssc.EARTHS[2]
assert SMALL_SPHERE == {"Spherical": {"radius": 3.0e6}}


def small_sphere_frame():
    return sc.scene(50, 20, earth_shape=SMALL_SPHERE)


def angles(name):
    return [(az, el) for az, el, _ in CASES[name][1]]


# ---- planes made by hand (the planes route): reach 5 km at step 100 m, m = 50 ------------------------------------------------
PLANES_REACH = 5_000.0
LIST_SIZES = (1, 63, 64, 65, 257)
LIST_PATTERNS = ("all", "alternate", "last65")
N_LIGHTS = (1, 2, 63, 64)


def fan_of_lights(n):
    """n world-frame lights, un-normalised: azimuths around the compass, z from below the horizontal to steeply up; light l differs
    from every other, so a shifted or dropped bit shows."""
    k = np.arange(n)
    az = np.radians(17.0 + 360.0 * k / max(n, 1))
    up = np.linspace(-0.2, 0.9, n) if n > 1 else np.array([0.05])
    return np.stack([np.cos(az), np.sin(az), up], axis=1) * (1.0 + 0.25 * k[:, None])


TERMINATOR_LIGHT_AT = (46.5, 8.5, 90.0, 0.0)  # (lat, lon, azimuth_deg, elevation_deg): due east on the horizontal of the mosaic's centre


def terminator_points(n=64):
    """n points along the parallel 46.5 N of the 3000 km sphere, 1.5 degrees of longitude (54 km) apart and centred on 8.5 E, 100 m
    up.  For the light on the eastern horizontal of (46.5 N, 8.5 E) the local elevation at longitude x is asin(cos 46.5 sin(x - 8.5)):
    from -30 degrees in the west through 0 to +30 degrees in the east — both signs within one wavefront."""
    lon = 8.5 + 1.5 * (np.arange(n) - (n - 1) / 2.0)
    return np.full(n, 46.5), lon, np.full(n, 100.0)
