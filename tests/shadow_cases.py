"""The frames and specs of the cast-shadow tests, in one place: tests/test_gpu_shadows.py runs them on the GPU against
tests/shadow_model.py, and tests/test_shadow_model.py asserts without a GPU — over the oracle's frame, which the parity tests pin
to the library's bit for bit — that every one of them holds both kinds of pixel.  Test infrastructure only.

Scene S2 (one synthetic tile 46..47 N, 8..9 E, the observer over its centre, looking north) with 60 km of range: the mosaic ends
55 km north of the observer, terrain beyond it is 0 m.  The tile's horizons stand 1 .. 2.5 degrees high, so the lights stand low.
Reach 20 km at step 100 m: m = 200."""
import numpy as np

from atm_raytracer_amd import _abi, synth
from atmospheres import configuration_atmosphere
from util import nested_cylinders

REACH, STEP = 20_000.0, 100.0
_TILES = {}


def scene(w, h, generator="Rectilinear", longitude=None, **over):
    """The observer 2500 m up (absolute), looking 6 degrees down over 40 degrees: the frame's trace points spread over 5 .. 55 km and
    400 .. 1700 m, so the rays of one call meet many different horizons (from the scene's own 50 m above its valley floor every
    point lies within 4 km and shares one)."""
    over.setdefault("max_distance", 60_000.0)
    over.setdefault("tilt", -6.0)
    over.setdefault("fov", 40.0)
    cfg, tiles = synth.scene("S2", w, h, generator=generator, **over)
    cfg.params.position.altitude_kind, cfg.params.position.altitude = _abi.ALT_ABSOLUTE, 2500.0
    if longitude is not None:
        cfg.params.position.longitude = longitude
    if not _TILES:
        _TILES.update(tiles)
    return cfg, _TILES


def spline_atmosphere():
    rng = np.random.default_rng(5)
    while True:
        a = configuration_atmosphere(rng)
        if "Spline" in a["first_temperature_function"]:
            return a


def with_objects(w, h):
    """Three opaque cylinders of 150 .. 250 m radius and 900 m height 3.3 km north of the observer, in front of the terrain."""
    cfg, tiles = scene(w, h, generator="Fast", tilt=-20.0)
    return nested_cylinders(cfg, 3, r0=150.0, dr=50.0, alpha=1.0), tiles


# name -> the frame
FRAMES = {
    "fast_50x20": lambda: scene(50, 20, generator="Fast"),
    "rect_64x32": lambda: scene(64, 32),
    "straight": lambda: scene(50, 20, straight_rays=True),
    "flat_distorted": lambda: scene(50, 20, earth_shape="FlatDistorted"),
    "ellipsoid": lambda: scene(50, 20, earth_shape={"Ellipsoid": {"a": 6378137.0, "b": 6300000.0}}),
    "spline": lambda: scene(50, 20, atmosphere=spline_atmosphere()),
    "alpha": lambda: scene(50, 20, terrain_alpha=0.5),
    "objects": lambda: with_objects(50, 20),
    "sky": lambda: scene(50, 20, generator="Fast", tilt=40.0),    # no pixel hits
    "ground": lambda: scene(64, 32, tilt=-25.0),                 # every pixel hits
    "from_outside": lambda: scene(64, 32, longitude=9.2, direction=270.0),  # the observer 15 km east of the mosaic, looking back at it
}

WEST = (260.0, 2.0, REACH, 0.0)
WEST_LOW = (260.0, 1.5, REACH, 0.0)  # the two frames that look steeply down see ground within 6 km: one horizon, lower
# name -> (frame, (azimuth_deg, elevation_deg, reach, lift), the case is about the shortcut).  The light elevations are chosen so that
# the model alone gives at least 5 % LIT and 5 % SHADOWED among the hit pixels, and where the case is about the shortcut a LIT ray
# that passes the escape test before m and one that does not (test_shadow_model.py asserts it); `sky` has no hit pixel to take a
# share of.
CASES = {
    "fast": ("fast_50x20", WEST, False),
    "rect": ("rect_64x32", WEST, True),
    "rect_lift2": ("rect_64x32", (260.0, 2.0, REACH, 2.0), False),
    "straight": ("straight", WEST, True),
    "flat_distorted": ("flat_distorted", WEST, False),  # no certificate: escaped_rays == 0
    "ellipsoid": ("ellipsoid", WEST, False),
    "spline": ("spline", WEST, False),
    "alpha": ("alpha", WEST, False),
    "objects": ("objects", WEST_LOW, False),
    "sky": ("sky", WEST, False),
    "ground": ("ground", WEST_LOW, False),
    "negative": ("rect_64x32", (100.0, -1.0, REACH, 2.0), False),
    "leaves_mosaic": ("from_outside", (90.0, 0.3, REACH, 0.0), False),  # toward the observer: T = 0 beyond the mosaic's east edge
}
