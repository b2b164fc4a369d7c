"""The escape certificate on the GPU: a Rectilinear ray above the mosaic's top (and its wavefront's objects)
that is provably ascending to max_distance leaves the march and is credited the steps it did not integrate.  With the shortcut on
(the default) and off (ATMRT_ESCAPE=off, read at every frame) every plane, n_hits and ray_steps must be the same bits, under every
march variant (ATMRT_MARCH_VARIANT is read once per process: one child per variant); and scenes built to tempt a wrong escape must
still match the oracle."""
import json
import math
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
from util import run_gpu, FIELDS_PIXEL, FIELDS_HIT, bits
full = {full!r}
sweep_seeds = {sweep_seeds!r}
ctx = generators.Context(0)

def work():
    i, e = C.c_uint64(), C.c_uint64()
    ctx.check(ctx.lib.atmrt_last_march_work(ctx.handle, C.byref(i), C.byref(e)))
    return int(i.value), int(e.value)

scenes = [("shard-c3", dict(), False, (4096, 2048), (1536, 2048)), ("shard-c5", dict(), False, (4096, 2048), (2048, 2304)),
          ("translucent", dict(terrain_alpha=0.5), False, (4096, 2048), (1024, 1536)),
          ("objects", dict(terrain_alpha=0.5), True, (4096, 2048), (1792, 2304))]
if full:
    scenes = [("headline", dict(), False, (4096, 2048), None), ("headline-a05", dict(terrain_alpha=0.5), False, (4096, 2048), None)] + scenes
out = {{}}
tiles = None
frames = []
if sweep_seeds:  # frames of the seeded sweep (escape_cases.frame_case) in place of the headline's
    import escape_cases as ec
    from oracle_binding import Oracle
    lib, oracle = ec.load_lib(), Oracle("libm")
    for seed in sweep_seeds:
        c = ec.frame_case(lib, oracle, seed)
        frames.append(("seed%d" % seed, c["cfg"], c["tiles"]))
    scenes = []
for name, kw, objects, size, cols in scenes:
    cfg, t = synth.scene("headline", size[0], size[1], generator="Rectilinear", level=1, **kw)
    tiles = tiles or t
    if cols:
        cfg.params.col_begin, cfg.params.col_end = cols
    if objects:
        synth.add_objects(cfg, n_cyl=300, n_bill=100, dist=(1_000.0, 100_000.0), spread_deg=60.0)
    frames.append((name, cfg, tiles))
for name, cfg, tiles in frames:
    res = {{}}
    for esc in ("on", "off"):
        if esc == "off":
            os.environ["ATMRT_ESCAPE"] = "off"
        else:
            os.environ.pop("ATMRT_ESCAPE", None)
        r = run_gpu(ctx, cfg, tiles)
        h = hashlib.sha256()
        for k in FIELDS_PIXEL + FIELDS_HIT:
            h.update(np.ascontiguousarray(bits(r[k])).tobytes())
        integrated, escaped = work()
        res[esc] = [h.hexdigest(), int(r["n_hits"]), int(r["ray_steps"]), integrated, escaped, ctx.debug_march_route()]
    out[name] = res
os.environ.pop("ATMRT_ESCAPE", None)
print("RESULT " + json.dumps(out))
"""


def _run(variant, full, sweep_seeds=()):
    env = dict(os.environ)
    env.pop("ATMRT_ESCAPE", None)
    if variant:
        env["ATMRT_MARCH_VARIANT"] = variant
    else:
        env.pop("ATMRT_MARCH_VARIANT", None)
    p = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), full=full, sweep_seeds=tuple(sweep_seeds))], env=env,
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [None, "plain", "small", "sliced"])
def test_escape_on_and_off_give_the_same_frames(variant):
    got = _run(variant, full=variant is None)
    for name, r in got.items():
        on, off = r["on"], r["off"]
        assert on[:3] == off[:3], (name, on, off)  # planes, n_hits, ray_steps
        assert off[3] == off[2] and off[4] == 0, (name, off)  # off: every step integrated, no ray escaped
        assert on[4] > 0 and on[3] < on[2], (name, on)  # on: the sky rays leave early


# ---- against the oracle: scenes that tempt a wrong escape ----
def _inversion_atmosphere(at, thick, gradient):
    return {"pressure": {"altitude": 0.0, "pressure": 101325.0},
            "first_temperature_function": {"Linear": {"gradient": -0.0065}},
            "next_functions": [{"altitude": at, "function": {"Linear": {"gradient": gradient}}},
                               {"altitude": at + thick, "function": {"Linear": {"gradient": -0.0065}}}],
            "temperature_fixed_point": {"altitude": 0.0, "temperature": 288.15}}


def _check(gpu_ctx, oracle_det, cfg, tiles, expect_escapes):
    import ctypes as C
    from util import assert_bitexact, run_gpu, run_oracle
    got = run_gpu(gpu_ctx, cfg, tiles)
    i, e = C.c_uint64(), C.c_uint64()
    gpu_ctx.check(gpu_ctx.lib.atmrt_last_march_work(gpu_ctx.handle, C.byref(i), C.byref(e)))
    assert_bitexact(got, run_oracle(oracle_det, cfg, tiles))
    if expect_escapes is not None:
        assert (e.value > 0) == expect_escapes, e.value
    return got


@pytest.mark.gpu
def test_ducting_atmosphere_against_the_oracle(gpu_ctx, oracle_det):
    """An inversion of 0.12 K/m over 400 m above the mosaic's top: sup (R + h) |n'| / n = 0.79 by the libm oracle — above the
    certificate's 1/2, so it is refused and no ray may escape below it, but below 1: not a duct, no ray that rises into it comes
    down again.  The scene that does what a duct does is test_a_real_duct_over_the_terrain_against_the_oracle."""
    from atm_raytracer_amd import synth
    cfg, tiles = synth.scene("S2", 96, 48, generator="Rectilinear", tilt=1.0, fov=20.0,
                             atmosphere=_inversion_atmosphere(2500.0, 400.0, 0.12))
    got = _check(gpu_ctx, oracle_det, cfg, tiles, None)
    assert got["n_hits"] > 0


@pytest.mark.gpu
def test_descending_rays_above_the_terrain_against_the_oracle(gpu_ctx, oracle_det):
    """The observer is far above the mosaic's top and looks slightly down: every ray starts above the floor, descending, and must not
    escape; the upper rows ascend and do."""
    from atm_raytracer_amd import synth
    cfg, tiles = synth.scene("S2", 96, 48, generator="Rectilinear", tilt=-1.0, fov=20.0)
    cfg.params.position.altitude = 6000.0
    got = _check(gpu_ctx, oracle_det, cfg, tiles, True)
    assert got["n_hits"] > 0


@pytest.mark.gpu
def test_objects_taller_than_the_terrain_against_the_oracle(gpu_ctx, oracle_det):
    """Objects reach far above the mosaic's top: rays that pass the top but not the objects' tops must keep marching."""
    from atm_raytracer_amd import synth
    cfg, tiles = synth.scene("S2", 96, 48, generator="Rectilinear", tilt=1.0, fov=30.0, max_distance=60_000.0, terrain_alpha=0.5)
    synth.add_objects(cfg, n_cyl=40, n_bill=10, dist=(2_000.0, 30_000.0), spread_deg=15.0, radius=(100.0, 300.0),
                      height=(2_000.0, 4_000.0), bill_w=(200.0, 500.0), bill_h=(2_000.0, 4_000.0))
    got = _check(gpu_ctx, oracle_det, cfg, tiles, None)
    assert got["n_hits"] > 0


# ---- ducts that overlap the terrain's top, a seeded sweep of tempting frames, tiles ----
N_ESCAPE_SEEDS = int(os.environ.get("ATMRT_ESCAPE_SEEDS", "60"))


def _work(ctx):
    import ctypes as C
    i, e = C.c_uint64(), C.c_uint64()
    ctx.check(ctx.lib.atmrt_last_march_work(ctx.handle, C.byref(i), C.byref(e)))
    return int(i.value), int(e.value)


def _on_and_off(ctx, cfg, tiles):
    """The frame with the shortcut on and off -> (frame on, work on, frame off, work off); the environment is left as it was."""
    from util import run_gpu
    before = os.environ.pop("ATMRT_ESCAPE", None)
    try:
        on = run_gpu(ctx, cfg, tiles)
        w_on = _work(ctx)
        os.environ["ATMRT_ESCAPE"] = "off"
        off = run_gpu(ctx, cfg, tiles)
        w_off = _work(ctx)
    finally:
        os.environ.pop("ATMRT_ESCAPE", None)
        if before is not None:
            os.environ["ATMRT_ESCAPE"] = before
    return on, w_on, off, w_off


def _returning(h, top):
    """A ray that is above `top` and ascending at some sample — where a floor wrongly put at the top would release it — and below
    `top` again later."""
    up = np.flatnonzero((h[1:] > top) & (h[1:] > h[:-1])) + 1
    return bool(up.size and np.any(h[int(up[0]):] < top))


def _hit_after_returning(rows, top, step):
    """How many of the rows' pixels have their first trace point beyond the place where their (returning) ray came below `top`
    again: trace points that an escape at the top would have dropped."""
    n = 0
    for hits, distance, h in rows:
        if hits and _returning(h, top):
            up = int(np.flatnonzero((h[1:] > top) & (h[1:] > h[:-1]))[0]) + 1
            back = up + int(np.flatnonzero(h[up:] < top)[0])
            n += distance > back * step
    return n


def _ends_escaping(h, floor):
    return bool(np.any((h[1:] > floor) & (h[1:] > h[:-1])))



def _real_duct_scene():
    """escape_cases.real_duct_scene (shared with tests/queue_cases.py, which marches it through the work queue): 0.5 K/m over 300 m
    (sup g 2.7) with its base 60 m above the top of a 5 x 5 mosaic and the observer 150 m under the top."""
    import escape_cases as ec
    return ec.real_duct_scene()


_DUCT_FRAME = {}


def _real_duct_frame(oracle_det):
    """(case, the oracle's frame, trace points beyond a return in every fourth column), computed once."""
    import escape_cases as ec
    from util import run_oracle
    if not _DUCT_FRAME:
        c = _real_duct_scene()
        want = run_oracle(oracle_det, c["cfg"], c["tiles"])
        dropped = sum(_hit_after_returning(ec.frame_rays(oracle_det, c, want, col), c["top"], c["step"]) for col in range(0, 48, 4))
        _DUCT_FRAME.update(case=c, want=want, dropped=dropped)
    return _DUCT_FRAME["case"], _DUCT_FRAME["want"], _DUCT_FRAME["dropped"]


def test_the_real_duct_scene_returns_rays_to_the_terrain(oracle_det, oracle_libm):
    """The condition on the scene, from the oracle alone (no device): sup g > 1 in the layer, and pixels whose first trace point lies
    beyond the place where their ray, having risen above the mosaic's top, came below it again."""
    import escape_cases as ec
    c, _, dropped = _real_duct_frame(oracle_det)
    g = ec.G(oracle_libm, c["atm"], c["radius"], c["wavelength"])
    assert max(g(float(h)) for h in np.linspace(c["top"] + 61.0, c["top"] + 359.0, 50)) > 1.5
    assert dropped >= 20, dropped


@pytest.mark.gpu
def test_a_real_duct_over_the_terrain_against_the_oracle(gpu_ctx, oracle_det):
    """A duct (sup g 2.7) whose trapping range overlaps the mosaic's top, 250 km: rays rise above the top, turn in the layer and come
    down onto terrain far out.  An escape at the top would drop those trace points."""
    from util import assert_bitexact
    c, want, dropped = _real_duct_frame(oracle_det)
    assert dropped >= 20
    on, w_on, off, w_off = _on_and_off(gpu_ctx, c["cfg"], c["tiles"])
    assert_bitexact(on, want)
    assert_bitexact(off, want)
    assert w_off == (off["ray_steps"], 0) and w_on[0] <= on["ray_steps"]


_SWEEP = {}


def _sweep_case(seed, oracle_libm, oracle_det):
    """The sweep's case of `seed` with its certificate and the oracle's frame (computed once per session)."""
    import escape_cases as ec
    from util import run_oracle
    if seed not in _SWEEP:
        lib = ec.load_lib()
        c = ec.frame_case(lib, oracle_libm, seed)
        c["floor"], c["from"], c["worst"] = ec.frame_certificate(lib, c)
        c["want"] = run_oracle(oracle_det, c["cfg"], c["tiles"])
        _SWEEP[seed] = c
    return _SWEEP[seed]


def test_the_sweep_of_tempting_frames_is_not_vacuous(oracle_det, oracle_libm):
    """Conditions on the sweep's inputs that the oracle alone must meet (no device): (a) in at least half of the seeds with a refused
    duct some pixel row's ray is a returning one (above the mosaic's top and ascending, then below the top again inside
    max_distance); (b) in at least half of all seeds some row's ray ends above the top and ascending: an escape is possible.
    The mosaic is one tile and the terrain beyond it is 0 m, so most returning rays come down where nothing stands; how many seeds
    have a trace point beyond a return is counted too (the duct seeds use a 5 x 5 mosaic and look towards its ridges for that)."""
    import escape_cases as ec
    ducts = ducts_returning = possible = bite = 0
    for seed in range(N_ESCAPE_SEEDS):
        c = _sweep_case(seed, oracle_libm, oracle_det)
        width = c["want"]["hit_count"].shape[1]
        columns = [ec.frame_rays(oracle_det, c, c["want"], col) for col in range(width)]
        if c["kind"] == "duct" and not c["straight"] and not c["flat"]:
            assert c["from"] > c["top"] - c["step"] or c["at"] + c["thick"] <= c["top"] - c["step"], (seed, "a duct was certified")
            ducts += 1
            ducts_returning += any(_returning(h, c["top"]) for _, _, h in columns[0])
        possible += any(h[-1] > c["top"] and h[-1] > h[-2] for _, _, h in columns[0])
        if not c["straight"]:
            bite += any(_hit_after_returning(rows, c["top"], c["step"]) for rows in columns)
    print(f"\n{N_ESCAPE_SEEDS} seeds: {ducts} refused ducts, {ducts_returning} with a returning ray; an escape is possible in {possible}; "
          f"{bite} seeds have a trace point beyond a return")
    assert ducts_returning >= 0.5 * ducts and possible >= 0.5 * N_ESCAPE_SEEDS
    assert bite >= 3 or N_ESCAPE_SEEDS < 60


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(N_ESCAPE_SEEDS))
def test_tempting_frames_against_the_oracle(gpu_ctx, oracle_det, oracle_libm, seed):
    """A seeded sweep of small Rectilinear frames of 150 .. 400 km (escape_cases.frame_case): layers next to the certificate's
    threshold on either side, real ducts around the mosaic's top with the observer under them, random atmospheres; every spherical
    and ellipsoidal earth model, flat ones in a tenth (the shortcut must stay off when refracted), straight rays in a fifth, column
    shards, translucent terrain and objects taller than the terrain in a third each.  The frame equals the oracle's in every bit
    (ray_steps included), with the shortcut on and off, and the march's work counters are consistent with the certificate: where
    the oracle's path of a pixel without a trace point is, at some step, ascending above the floor, a ray did escape (frames
    without objects: a wavefront whose candidate list holds an object is marched by the general tracer, which has no shortcut; the
    headline-size "objects" scene of test_escape_on_and_off_give_the_same_frames is where escapes next to objects are asserted)."""
    import escape_cases as ec
    from util import assert_bitexact
    c = _sweep_case(seed, oracle_libm, oracle_det)
    want = c["want"]
    on, w_on, off, w_off = _on_and_off(gpu_ctx, c["cfg"], c["tiles"])
    assert_bitexact(on, want)
    assert_bitexact(off, want)
    pixels = on["hit_count"].size
    assert w_on[0] <= on["ray_steps"] and w_on[1] <= pixels, (w_on, on["ray_steps"], pixels)
    assert w_off == (off["ray_steps"], 0), (w_off, off["ray_steps"])
    if math.isinf(c["floor"]):
        assert w_on[1] == 0, w_on
    elif not c["straight"] and not c["objects"]:  # with objects the wavefronts that list one go to the general tracer: no escape there
        floor = c["floor"] + 1.0
        for col in range(want["hit_count"].shape[1]):
            if any(hits == 0 and _ends_escaping(h, floor) for hits, _, h in ec.frame_rays(oracle_det, c, want, col)):
                assert w_on[1] > 0, (w_on, floor, col)
                break


@pytest.fixture(scope="module")
def multi3():
    from atm_raytracer_amd import generators
    ctx = generators.Context.multi([0, 0, 0])
    yield ctx
    ctx.close()


@pytest.mark.gpu
def test_three_tiles_count_the_work_of_the_single_context(gpu_ctx, multi3):
    """The headline's view at 512 x 256 pixels (a multi context cuts its own column tiles and takes no column shard) through a
    3-tile multi context and through the single one: the same bits, and
    atmrt_last_march_work of the multi context (the sum over its tiles) gives the single context's integrated steps and escaped
    rays — no objects, so no wavefront has a floor of its own — with the shortcut on and off."""
    from atm_raytracer_amd import synth
    from util import assert_bitexact
    cfg, tiles = synth.scene("headline", 512, 256, generator="Rectilinear", level=1)
    s_on, sw_on, s_off, sw_off = _on_and_off(gpu_ctx, cfg, tiles)
    m_on, mw_on, m_off, mw_off = _on_and_off(multi3, cfg, tiles)
    assert_bitexact(m_on, s_on)
    assert_bitexact(m_off, s_off)
    assert mw_on == sw_on and mw_off == sw_off, (mw_on, sw_on, mw_off, sw_off)
    assert sw_on[1] > 0 and sw_on[0] < s_on["ray_steps"] and sw_off == (s_off["ray_steps"], 0)


VARIANT_SEEDS = (1, 4, 5, 7, 12)  # a refused duct (1, 7), straight rays (4), objects where the sweep draws them


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["plain", "small", "sliced", "queue"])
def test_sweep_frames_under_every_march_variant(oracle_det, oracle_libm, variant):
    """Five frames of the sweep under each march variant (one child process per variant): on and off give the same bits and the same
    ray_steps as the oracle's frame.  The whole-frame work queue takes opaque whole frames without objects on the Spherical
    calculator only, so `queue` runs over the sweep's seeds of that kind (queue_cases.eligible_seeds: threshold layers, ducts and
    random families, most of them Splines), and every one of them must have been launched as a queue."""
    import hashlib
    from util import bits, FIELDS_PIXEL, FIELDS_HIT
    seeds = VARIANT_SEEDS
    if variant == "queue":
        import queue_cases
        seeds = queue_cases.eligible_seeds()
        assert len(seeds) >= 10
    got = _run(variant, full=False, sweep_seeds=seeds)
    assert len(got) == len(seeds)
    for seed in seeds:
        want = _sweep_case(seed, oracle_libm, oracle_det)["want"]
        h = hashlib.sha256()
        for k in FIELDS_PIXEL + FIELDS_HIT:
            h.update(np.ascontiguousarray(bits(want[k])).tobytes())
        on, off = got["seed%d" % seed]["on"], got["seed%d" % seed]["off"]
        assert on[:3] == off[:3] == [h.hexdigest(), int(want["n_hits"]), int(want["ray_steps"])], (seed, on, off)
        assert off[3] == off[2] and off[4] == 0 and on[3] <= on[2], (seed, on, off)
        if variant == "queue":
            assert on[5] == off[5] == 4, (seed, on, off)
