"""The terrain ceiling table on the GPU (csrc/atmrt_ceiling.h): per step and azimuth bin a bound of the terrain
under every ray of the bin.  A sample above its cell skips its lookup, an ascending ray above its bin's suffix leaves the march.
With the table on (the default), off (ATMRT_CEILING=off) and rebuilt in every frame (=rebuild; both read at every frame) every
plane, the trace-point lists, n_hits and ray_steps are the same bits under every march variant (ATMRT_MARCH_VARIANT is read once
per process: one child per variant); views built to tempt a wrong bound match the oracle; the table follows the terrain, the
observer, the step and the view on one context; and the march integrates fewer steps and looks up less terrain with it."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import ctypes as C, hashlib, json, os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import numpy as np
from atm_raytracer_amd import generators, synth
from util import run_gpu, frame_stats, FIELDS_PIXEL, FIELDS_HIT, bits
ctx = generators.Context(0)

def work():
    i, e = C.c_uint64(), C.c_uint64()
    ctx.check(ctx.lib.atmrt_last_march_work(ctx.handle, C.byref(i), C.byref(e)))
    return int(i.value), int(e.value)

frames = []
tiles = None
for name, kw, objects, size in (("headline", dict(), False, (192, 96)), ("translucent", dict(terrain_alpha=0.5), False, (192, 96)),
                                ("objects", dict(terrain_alpha=0.5), True, (192, 96)), ("work", dict(), False, (512, 256))):
    cfg, t = synth.scene("headline", size[0], size[1], generator="Rectilinear", level=1, **kw)
    tiles = tiles or t
    if objects:
        synth.add_objects(cfg, n_cyl=300, n_bill=100, dist=(1_000.0, 100_000.0), spread_deg=60.0)
    frames.append((name, cfg))
out = {{}}
for name, cfg in frames:
    res = {{}}
    for mode in (None, "off", "rebuild"):
        os.environ.pop("ATMRT_CEILING", None)
        if mode:
            os.environ["ATMRT_CEILING"] = mode
        r = run_gpu(ctx, cfg, tiles)
        h = hashlib.sha256()
        for k in FIELDS_PIXEL + FIELDS_HIT:
            h.update(np.ascontiguousarray(bits(r[k])).tobytes())
        integrated, escaped = work()
        res[mode or "on"] = [h.hexdigest(), int(r["n_hits"]), int(r["ray_steps"]), integrated, int(frame_stats(ctx)["terrain_lookups"])]
    out[name] = res
os.environ.pop("ATMRT_CEILING", None)
print("RESULT " + json.dumps(out))
"""

_CHILD_RESULTS = {}


def _child(variant):
    """The child's frames under one march variant (computed once per session)."""
    if variant not in _CHILD_RESULTS:
        env = dict(os.environ)
        for k in ("ATMRT_CEILING", "ATMRT_ESCAPE", "ATMRT_MARCH_VARIANT"):
            env.pop(k, None)
        if variant:
            env["ATMRT_MARCH_VARIANT"] = variant
        p = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], env=env, capture_output=True,
                           text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-2000:]
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
        _CHILD_RESULTS[variant] = json.loads(line[len("RESULT "):])
    return _CHILD_RESULTS[variant]


# queue: the whole-frame work queue, forced on the opaque frames (192 x 96: 288 groups; `work`, 512 x 256: 2,048 groups, whose LDS counter
# sums must give every other route's integrated steps); without a table (ATMRT_CEILING=off) it has no order and falls back to the grid
VARIANTS = [None, "plain", "small", "sliced", "queue"]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
def test_table_on_off_and_rebuilt_give_the_same_frames(variant):
    for name, r in _child(variant).items():
        on, off, rebuild = r["on"], r["off"], r["rebuild"]
        assert on[:3] == off[:3] == rebuild[:3], (name, on, off, rebuild)  # planes and lists, n_hits, ray_steps
        assert on[3:] == rebuild[3:], (name, on, rebuild)  # the same table, the same work
        assert on[3] <= off[3] and on[4] <= off[4], (name, on, off)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
def test_the_march_integrates_and_looks_up_less_with_the_table(variant):
    """The headline's view at 512 x 256: integrated steps and terrain lookups with the table strictly below those without it (the
    escape shortcut on in both), and the integrated steps are one number under every march variant: a ray's bin is its own."""
    r = _child(variant)["work"]
    assert r["on"][3] < r["off"][3] and r["on"][4] < r["off"][4], r
    assert r["on"][3] == _child(None)["work"]["on"][3] and r["off"][3] == _child(None)["work"]["off"][3], (r, _child(None)["work"])


def _work(ctx):
    i, e = C.c_uint64(), C.c_uint64()
    ctx.check(ctx.lib.atmrt_last_march_work(ctx.handle, C.byref(i), C.byref(e)))
    return int(i.value), int(e.value)


@pytest.mark.gpu
def test_three_tiles_integrate_the_steps_of_the_single_context(gpu_ctx):
    from atm_raytracer_amd import generators, synth
    from util import assert_bitexact, run_gpu
    cfg, tiles = synth.scene("headline", 512, 256, generator="Rectilinear", level=1)
    single = run_gpu(gpu_ctx, cfg, tiles)
    w_single = _work(gpu_ctx)
    multi = generators.Context.multi([0, 0, 0])
    try:
        tiled = run_gpu(multi, cfg, tiles)
        w_tiled = _work(multi)
    finally:
        multi.close()
    assert_bitexact(tiled, single)
    assert w_tiled == w_single and w_single[0] == _child(None)["work"]["on"][3], (w_tiled, w_single)


# ---- against the oracle: views that tempt a wrong bound ----
def _check(gpu_ctx, oracle_det, cfg, tiles, escapes=None):
    from util import assert_bitexact, run_gpu, run_oracle
    got = run_gpu(gpu_ctx, cfg, tiles)
    work = _work(gpu_ctx)
    assert_bitexact(got, run_oracle(oracle_det, cfg, tiles))
    if escapes is not None:
        assert (work[1] > 0) == escapes, work
    return got


def _valley_tiles():
    """One level-1 tile: a floor of 200 m, a ridge of 600 m 10 km north of the observer and one of 2500 m 40 km north, both across
    every azimuth of the view: a ray that has cleared the near ridge is above everything close to it, not above its bin's suffix."""
    n = 1201
    lat = 46.0 + np.arange(n) / (n - 1.0)
    north = (lat - 46.1) * 111_195.0
    profile = 200.0 + 400.0 * np.exp(-((north - 10_000.0) / 1_500.0) ** 2) + 2_300.0 * np.exp(-((north - 40_000.0) / 3_000.0) ** 2)
    wiggle = 30.0 * np.sin(np.arange(n) / 7.0)[None, :]
    return {(46, 8): np.rint(profile[:, None] + wiggle).astype(np.int16)}


def _scene(**kw):
    from atm_raytracer_amd import synth
    kw.setdefault("fov", 20.0)
    return synth.scene("S2", 96, 48, generator="Rectilinear", **kw)


@pytest.mark.gpu
def test_a_valley_under_a_farther_and_higher_ridge_against_the_oracle(gpu_ctx, oracle_det):
    cfg, _ = _scene(tilt=2.0, max_distance=80_000.0)
    cfg.params.position.latitude, cfg.params.position.longitude = 46.1, 8.5
    cfg.params.position.altitude = 100.0  # Relative: 330 m, under the near ridge
    got = _check(gpu_ctx, oracle_det, cfg, _valley_tiles(), True)
    far = got["distance"][got["hit_offset"][got["hit_count"] > 0].astype(np.int64)]
    assert (far > 30_000.0).sum() > 100 and (far < 15_000.0).sum() > 100  # both ridges are seen: rays cleared the near one and met the far one


@pytest.mark.gpu
def test_an_observer_outside_the_mosaic_looking_in_against_the_oracle(gpu_ctx, oracle_det):
    cfg, tiles = _scene(direction=90.0, tilt=-1.0)
    cfg.params.position.latitude, cfg.params.position.longitude = 46.5, 7.6
    cfg.params.position.altitude = 1500.0  # over the 0 m outside the tile
    assert _check(gpu_ctx, oracle_det, cfg, tiles, True)["n_hits"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("yaw", [180.0, 45.0])
def test_yaw_against_the_oracle(gpu_ctx, oracle_det, yaw):
    """yaw 180: the rays' directions lie on both sides of atan2's cut at +-pi, the bins must not"""
    got = _check(gpu_ctx, oracle_det, *_scene(direction=yaw, tilt=0.5), True)
    assert got["n_hits"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("tilt", [10.0, -20.0])
def test_tilt_against_the_oracle(gpu_ctx, oracle_det, tilt):
    """a tilted frame's border rows are not lines of constant azimuth: the bins come from all four borders"""
    _check(gpu_ctx, oracle_det, *_scene(tilt=tilt, fov=40.0), tilt > 0)


@pytest.mark.gpu
def test_straight_rays_against_the_oracle(gpu_ctx, oracle_det):
    assert _check(gpu_ctx, oracle_det, *_scene(tilt=0.5, straight_rays=True), True)["n_hits"] > 0


def _inversion_atmosphere(at, thick, gradient):
    return {"pressure": {"altitude": 0.0, "pressure": 101325.0},
            "first_temperature_function": {"Linear": {"gradient": -0.0065}},
            "next_functions": [{"altitude": at, "function": {"Linear": {"gradient": gradient}}},
                               {"altitude": at + thick, "function": {"Linear": {"gradient": -0.0065}}}],
            "temperature_fixed_point": {"altitude": 0.0, "temperature": 288.15}}


@pytest.mark.gpu
@pytest.mark.parametrize("at,thick,gradient", [(2500.0, 400.0, 0.12), (1200.0, 300.0, 0.5)])
def test_a_refused_layer_above_the_local_ceilings_against_the_oracle(gpu_ctx, oracle_det, at, thick, gradient):
    """The certificate refuses the layer (sup (R + h) |n'| / n above 1/2; the second is a duct): no ray may leave below its top,
    however low the ceiling of its bin is there."""
    got = _check(gpu_ctx, oracle_det, *_scene(tilt=1.0, atmosphere=_inversion_atmosphere(at, thick, gradient)))
    assert got["n_hits"] > 0


@pytest.mark.gpu
def test_a_flat_earth_with_refraction_against_the_oracle(gpu_ctx, oracle_det):
    """the Spherical calculator on a flat earth: refracted rays never leave early, but their samples above the cells skip lookups"""
    from util import frame_stats
    cfg, tiles = _scene(tilt=1.0, earth_shape="SimpleObserverAe", max_distance=100_000.0)
    got = _check(gpu_ctx, oracle_det, cfg, tiles, False)
    assert frame_stats(gpu_ctx)["terrain_lookups"] < got["ray_steps"]


# ---- the table's lifetime on one context ----
@pytest.mark.gpu
def test_the_table_follows_terrain_observer_step_and_view(oracle_det):
    """One context, one resident terrain: the second frame of the same view reuses the table (its build time is 0); after the
    observer moved by 0.2 degrees, after other tiles were uploaded, after the step changed and after fov and direction changed the
    table is built again, and every frame matches the oracle."""
    from atm_raytracer_amd import generators, synth
    from util import assert_bitexact, run_oracle
    ctx = generators.Context(0)
    try:
        cfg, tiles = _scene(tilt=0.5)
        terrain = generators.Terrain.from_tiles(tiles, ctx)

        def frame(expect_build, tiles):
            gen = generators.make_generator(generators.Params(cfg), terrain)
            got = gen.generate()
            built = gen.last_timings()["ceiling_ms"]
            assert (built > 0.0) == expect_build, built
            assert_bitexact(got, run_oracle(oracle_det, cfg, tiles))

        frame(True, tiles)
        frame(False, tiles)
        cfg.params.position.altitude += 200.0  # the altitude is not part of the table
        frame(False, tiles)
        cfg.params.position.latitude += 0.2
        frame(True, tiles)
        frame(False, tiles)
        ctx.check(ctx.lib.atmrt_terrain_clear(ctx.handle))
        other = synth.synth_tiles([46], [8], level=1, seed=synth.SEED + 1)
        terrain = generators.Terrain.from_tiles(other, ctx)
        frame(True, other)
        cfg.params.simulation_step = 150.0
        frame(True, other)
        cfg.params.frame.fov, cfg.params.frame.direction = 30.0, 135.0
        frame(True, other)
        frame(False, other)
    finally:
        ctx.close()
