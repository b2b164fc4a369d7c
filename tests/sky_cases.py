"""The frames and lists of the sky-ray tests, in one place: tests/test_gpu_sky.py runs them on the GPU against tests/sky_model.py, and
tests/test_sky_model.py asserts without a GPU — over the oracle's frame, which the parity tests pin to the library's bit for bit —
that every one of them holds what its case is about.  Test infrastructure only.

Every case marches at a sky step of 1000 m to a top of 100 km with m = 1500: the horizon ray takes 1173 steps.  The frames are
tests/shadow_cases.py's scene (S2, the observer 2500 m up, absolute, so that h0 is the configured altitude itself) at 48 x 24
pixels: the width is no multiple of 64, so a wavefront of the compacted list spans rows of different elevations and its lanes
exit at different steps."""
import numpy as np

import shadow_cases as sc

STEP, TOP, FLOOR, M = 1000.0, 100000.0, 0.0, 1500
H0 = 2500.0  # shadow_cases.scene's observer altitude, absolute
W, H = 48, 24


def frame(generator="Rectilinear", tilt=-2.0, **over):
    return sc.scene(W, H, generator=generator, tilt=tilt, **over)


# name -> the frame.  tilt -2 over fov 40 (rows from -12 to 8 degrees): about half of the pixels are sky.
FRAMES = {
    "rect": lambda: frame(),
    "fast": lambda: frame("Fast"),
    "interp": lambda: frame("InterpolatingRectilinear"),
    "spline": lambda: frame(atmosphere=sc.spline_atmosphere()),
    "flat": lambda: frame(earth_shape="FlatDistorted"),
    "straight": lambda: frame(straight_rays=True),
    "all_sky": lambda: frame("Fast", tilt=40.0),
    "no_sky": lambda: frame(tilt=-25.0),
}
# The frames in which every ray is decided by m = 1500 without a LOST: US-76 on the sphere.  Not among them: `spline` (that atmosphere
# gives NaN heights above its last point: every ascending ray is LOST) and `flat` — on a flat refracting earth n cos(angle) is
# constant along a ray, so a ray launched below acos(1 / n0), about 1.3 degrees, can never reach n = 1: it turns back (GROUND) or is
# still on its way at m (INSIDE); the rows above that do EXIT.
US76_SPHERE = ("rect", "fast", "interp", "all_sky", "no_sky")

LIST_LENGTHS = (0, 1, 63, 64, 65, 257)
LIST_H0 = 1000.0


def list_elevations(n):
    """n launch elevations from h0 = 1000 m, from -1.2 to 0.6 degrees in an order that mixes them inside every wavefront: GROUND
    (below about -0.9 degrees the ray reaches the floor) and EXIT both occur within any 8 consecutive entries."""
    k = np.arange(n)
    return -1.2 + 1.8 * ((k * 37) % 64) / 63.0


SHORT_M = 100


def list_elevations_short(n):
    """The same list for a call with m = 100, every 8th entry at 50 degrees: there -1.0 degrees is GROUND (step 84), the rays near
    the horizontal are INSIDE and 50 degrees is EXIT (before step 97, where 45 degrees leaves) — all three inside one wavefront."""
    e = list_elevations(n)
    e[3::8] = 50.0
    return e


LIFTED_H0 = 1000.0
LIFTED_SUN = (90.0, -0.3, 0.2666, (255, 236, 170))  # true elevation -0.3 degrees: the whole disc below the astronomical horizon


def lifted_frame():
    """An all-sky frame from 1000 m over an empty terrain (scene S1 without tiles, looking east): 2 degrees wide, rows from about
    -0.2 to 0.8 degrees — every ray clears the sea-level horizon (its dip from 1000 m is about 0.95 degrees) and leaves through the top."""
    from atm_raytracer_amd import _abi, synth
    cfg, tiles = synth.scene("S1", W, H, generator="Rectilinear", fov=2.0, tilt=0.3, max_distance=60_000.0, straight_rays=False)
    cfg.params.position.altitude_kind, cfg.params.position.altitude = _abi.ALT_ABSOLUTE, LIFTED_H0
    return cfg, tiles
