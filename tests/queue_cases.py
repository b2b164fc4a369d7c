"""Frames that the whole-frame work queue of the opaque Rectilinear march (k_rect_march_queue) can take, at the
smallest size that still has the property named: opaque terrain, no objects, the whole image, an earth model of the Spherical
calculator (SimpleSphere, Spherical, ObserverAe, SimpleObserverAe: the only one with a ceiling table, so the only one with a queue).
Small frames take the time-sliced march by default; tests/test_gpu_march_queue_scenes.py forces them through the queue in a child
process (ATMRT_MARCH_VARIANT=queue) and compares every bit with the det oracle's frame.  Nothing here needs a device: the child
processes, the oracle and the non-GPU tests that prove the frames are not vacuous (tests/test_queue_cases.py) build them from this
code."""
import functools

import numpy as np

import atmospheres

QUEUE_EARTHS = ("SimpleSphere", "Spherical", "ObserverAe", "SimpleObserverAe")  # earth.calc == 2 (atmrt_core.h, earth_resolve)


def s2(w, h, **kw):
    """The scene of tests/test_gpu_march_queue.py at another size: S2, Rectilinear, 60 km, tilt -1, opaque."""
    from atm_raytracer_amd import synth
    return synth.scene("S2", w, h, generator="Rectilinear", **{**dict(max_distance=60_000.0, tilt=-1.0), **kw})


@functools.lru_cache(maxsize=None)
def s2_observer_altitude():
    """The resolved altitude of S2's observer: the terrain under it (the oracle's lookup) + 50 m."""
    from oracle_binding import Oracle
    return observer_altitude(Oracle("det"), *s2(8, 8))


def _inversion_at():
    """The base of the S2 frames' inversion layer: 100 m above the observer, whole metres, inside the terrain's altitude range (a
    layer at 2500 m is above every ray that meets terrain: the frame is then US-76's in every bit, which proves nothing)."""
    return float(round(s2_observer_altitude() + 100.0))


def _high_observer():
    """the frame of test_gpu_escape.py::test_descending_rays_above_the_terrain_against_the_oracle at 96 x 48"""
    from atm_raytracer_amd import synth
    cfg, tiles = synth.scene("S2", 96, 48, generator="Rectilinear", tilt=-1.0, fov=20.0)
    cfg.params.position.altitude = 6000.0
    return cfg, tiles


def _duct(kind):
    import escape_cases as ec
    c = ec.real_duct_scene(kind)
    return c["cfg"], c["tiles"]


TWO_STEPS_TILT = -10.0  # at tilt -1 no ray of a 250 m march comes down to the ground 50 m under the observer; at -10 a ninth do (57 pixels)

# name -> a function that builds (cfg, tiles).  The figures are the det oracle's (tests/test_queue_cases.py asserts the ones that
# make a frame what it is).
FRAMES = {
    # the CUBIC instantiation k_rect_march_queue<2, true>: an atmosphere with a Spline
    "spline-inversion": lambda: s2(96, 40, atmosphere=atmospheres.inversion(_inversion_at(), 400.0, 0.05, "Natural")),  # 60 groups
    "spline-partial": lambda: s2(50, 13, atmosphere=atmospheres.inversion(_inversion_at(), 400.0, 0.05, "Derivatives")),  # 11 groups, the last of 10 pixels
    "duct-spline": lambda: _duct("SecondDerivatives"),
    "wild-spline": lambda: s2(64, 24, earth_shape="SimpleSphere", atmosphere=atmospheres.WILD_SPLINE),
    "long-atmosphere": lambda: s2(64, 24, atmosphere=atmospheres.long_atmosphere(np.random.default_rng(5))),
    "cubic-interval": lambda: s2(64, 24, atmosphere=atmospheres.cubic_interval(1500.0, 800.0, 2e-4)),
    # the Linear instantiation k_rect_march_queue<2, false>
    "duct-linear": lambda: _duct("Linear"),  # 48 x 32, 250 km, 2,500 steps over a 5 x 5 mosaic: 24 groups
    "straight": lambda: s2(96, 40, straight_rays=True),  # ceil_floor = -inf
    "observer-ae": lambda: s2(96, 40, earth_shape={"ObserverAe": {"proj_radius": 6371000.0}}),  # flat and refracted: no ray escapes
    "simple-observer-ae-straight": lambda: s2(96, 40, earth_shape="SimpleObserverAe", straight_rays=True),
    "small-radius": lambda: s2(96, 40, earth_shape={"Spherical": {"radius": 3.0e6}}),
    "simple-sphere-violet": lambda: s2(96, 40, earth_shape="SimpleSphere", wavelength=4.1e-7),
    "all-sky": lambda: s2(64, 8, tilt=25.0, fov=20.0),  # no hits, 512 escaped rays
    "all-ground": lambda: s2(64, 8, tilt=-35.0, fov=20.0),  # 512 hits, one step each
    "two-steps": lambda: s2(64, 8, max_distance=250.0, tilt=TWO_STEPS_TILT),  # march_steps = 2: a counting sort of three bins
    "high-observer": _high_observer,
}
SPLINE_FRAMES = ("spline-inversion", "spline-partial", "duct-spline", "wild-spline", "long-atmosphere", "cubic-interval")
# the frames whose queue estimates are compared with tests/march_order_model.py
MODEL_FRAMES = ("spline-inversion", "duct-linear", "all-sky", "all-ground", "two-steps", "spline-partial")


SPIKE_FRAMES = ("near", "far", "up", "nadir")  # the opaque spike frames of tests/ceiling_cases.py: neighbouring bins hold different ceilings
MODEL_FRAMES += ("spikes-near", "spikes-nadir")  # (nadir: beyond what every bin shares near the observer, five distinct estimates)


def names():
    """every frame of the family: the named ones, the spike frames and the escape sweep's eligible seeds"""
    return list(FRAMES) + ["spikes-" + n for n in SPIKE_FRAMES] + ["seed%d" % s for s in eligible_seeds()]


@functools.lru_cache(maxsize=None)
def _libm():
    from oracle_binding import Oracle
    return Oracle("libm")


def build(name):
    """(cfg, tiles) of a frame of names()"""
    if name in FRAMES:
        return FRAMES[name]()
    if name.startswith("spikes-"):
        import ceiling_cases
        return ceiling_cases.marched(name[len("spikes-"):])
    if name.startswith("seed"):
        import escape_cases as ec
        c = ec.frame_case(ec.load_lib(), _libm(), int(name[len("seed"):]))
        return c["cfg"], c["tiles"]
    raise KeyError(name)


_WANT = {}


def oracle_frame(oracle_det, name):
    """the det oracle's frame of build(name), computed once per process and left unchanged"""
    from util import run_oracle
    if name not in _WANT:
        _WANT[name] = run_oracle(oracle_det, *build(name))
    return _WANT[name]


def digest(result):
    """[sha256 over the bits of every pixel plane and trace-point field, n_hits, ray_steps], as
    tests/test_gpu_escape.py::test_sweep_frames_under_every_march_variant compares frames across processes"""
    import hashlib
    from util import FIELDS_HIT, FIELDS_PIXEL, bits
    h = hashlib.sha256()
    for k in FIELDS_PIXEL + FIELDS_HIT:
        h.update(np.ascontiguousarray(bits(result[k])).tobytes())
    return [h.hexdigest(), int(result["n_hits"]), int(result["ray_steps"])]


def observer_altitude(oracle, cfg, tiles):
    """the observer's resolved altitude: Absolute as configured, Relative above the oracle's terrain lookup (0 m where there is none)"""
    from atm_raytracer_amd import _abi
    pos = cfg.params.position
    if int(pos.altitude_kind) == _abi.ALT_ABSOLUTE:
        return float(pos.altitude)
    t = oracle.terrain_new(tiles)
    try:
        e = oracle.get_elev(t, float(pos.latitude), float(pos.longitude))
    finally:
        oracle.terrain_free(t)
    return (0.0 if e is None else float(e)) + float(pos.altitude)


def shape_radius(cfg):
    """the radius of the stepper's sphere for the Spherical calculator's earth models, None for its flat ones"""
    from atm_raytracer_amd import _abi
    e = cfg.params.earth
    if int(e.kind) == _abi.EARTH_KINDS["Spherical"]:
        return float(e.radius)
    if int(e.kind) == _abi.EARTH_KINDS["SimpleSphere"]:
        return 6371000.0
    assert int(e.kind) in (_abi.EARTH_KINDS["ObserverAe"], _abi.EARTH_KINDS["SimpleObserverAe"]), int(e.kind)
    return None


def us76_twin():
    """`spline-inversion` under US-76: what that frame must differ from"""
    return s2(96, 40)


def frame(name):
    return FRAMES[name]()


def is_spline(cfg):
    """the atmosphere holds a Spline function: the march takes its CUBIC instantiation (Frame::atm_cubic)"""
    from atm_raytracer_amd import _abi
    atm = cfg.atmosphere
    return atm is not None and any(int(atm.functions[k].kind) == _abi.TEMP_SPLINE for k in range(int(atm.n_functions)))


def groups(cfg):
    p = cfg.params
    return (int(p.width) * int(p.height) + 63) // 64


# ---- the escape sweep's seeds that can take the queue ----
SWEEP_SEEDS = range(60)


def queue_eligible(case):
    """A pure predicate on a case of escape_cases.frame_case: opaque, no objects, the whole image, an earth of the Spherical
    calculator — what march_plan (csrc/atmrt_march_plan.h) asks of a frame before ATMRT_MARCH_VARIANT=queue routes it to the queue."""
    from atm_raytracer_amd import _abi
    cfg = case["cfg"]
    p = cfg.params
    whole = int(p.col_begin) == 0 and int(p.col_end) in (0, int(p.width))
    kinds = [_abi.EARTH_KINDS[k] for k in QUEUE_EARTHS]
    return float(p.terrain_alpha) == 1.0 and not cfg.objects and not case["objects"] and whole and int(p.earth.kind) in kinds


@functools.lru_cache(maxsize=None)
def eligible_seeds():
    """the seeds of the escape sweep that queue_eligible selects (enumerated: 2, 15, 17, 20, 31, 33, 40, 45, 48, 50, 51, 52, 57)"""
    import escape_cases as ec
    from oracle_binding import Oracle
    lib, oracle = ec.load_lib(), Oracle("libm")
    return tuple(seed for seed in SWEEP_SEEDS if queue_eligible(ec.frame_case(lib, oracle, seed)))
