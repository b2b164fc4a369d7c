"""The Spherical geodesic's sin / cos from a per-step table (Frame::xs_sin / xs_cos): the marching kernels read
sin(xs[i] / R) and cos(xs[i] / R) of the sample after i steps from a table that k_step_trig fills once per distance table, instead
of dividing and reducing the argument in every lane.  The table must hold the bits a lane computes (dm_div or IEEE division, then
dm_sincos), frames must equal the oracle's in every field with the table on and off (ATMRT_STEP_TRIG=off, read at every frame) under
every march variant (ATMRT_MARCH_VARIANT is read once per process: one child per variant), and the table must follow the step,
max_distance, the radius and the earth model."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the table against the per-lane code ----
def _table(ctx, cfg):
    """(n, xs, sin, cos) of atmrt_debug_step_trig for the parameters of cfg."""
    from atm_raytracer_amd import generators
    generators.make_generator(generators.Params(cfg), generators.Terrain(ctx))._configure()
    n = C.c_size_t()
    ctx.check(ctx.lib.atmrt_debug_step_trig(ctx.handle, 0, None, None, None, C.byref(n)))
    xs, s, c = (np.empty(n.value) for _ in range(3))
    if n.value:
        ctx.check(ctx.lib.atmrt_debug_step_trig(ctx.handle, n.value, xs.ctypes.data, s.ctypes.data, c.ctypes.data, C.byref(n)))
    return n.value, xs, s, c


def _probe(ctx, op, a, b=None, two=False):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = None if b is None else np.ascontiguousarray(b, dtype=np.float64)
    o0, o1 = np.empty_like(a), np.empty_like(a)
    ctx.check(ctx.lib.atmrt_math_probe(ctx.handle, op, a.size, a.ctypes.data, None if b is None else b.ctypes.data, o0.ctypes.data,
                                       o1.ctypes.data if two else None))
    return (o0, o1) if two else o0


PROBE_DIV, PROBE_SINCOS, PROBE_IEEE_DIV = 0, 6, 9  # atmrt_math_probe_op, include/atmrt.h


@pytest.mark.gpu
@pytest.mark.parametrize("step,max_distance,radius,fast_div", [(100.0, 200_000.0, 6371000.0, True), (0.0002, 0.5, 6371000.0, True),
                                                               (100.0, 200_000.0, 1.0e31, False)])
def test_table_holds_what_a_lane_computes(gpu_ctx, step, max_distance, radius, fast_div):
    """The headline's step and radius; a 0.2 mm step; a radius outside EARTH_FAST_DIV's 1e-30 .. 1e30 band (IEEE division).  The
    table's distances are the stepper's (0 + step + ...), it ends with the last one inside max_distance, and every entry equals the
    probe's division (the one coords_at_dist takes for that radius) followed by its dm_sincos, bit for bit."""
    from atm_raytracer_amd import synth
    from util import bits
    cfg, _ = synth.scene("S2", 8, 8, generator="Rectilinear", step=step, max_distance=max_distance,
                         earth_shape={"Spherical": {"radius": radius}})
    n, xs, s, c = _table(gpu_ctx, cfg)
    want_xs = [0.0]
    while want_xs[-1] + step <= max_distance:  # the stepper's x: repeated addition
        want_xs.append(want_xs[-1] + step)
    assert n == len(want_xs) and np.array_equal(xs, np.array(want_xs))
    ang = _probe(gpu_ctx, PROBE_DIV if fast_div else PROBE_IEEE_DIV, xs, np.full(n, radius))
    assert np.array_equal(ang, xs / radius)  # both divisions are IEEE's on these operands
    want_s, want_c = _probe(gpu_ctx, PROBE_SINCOS, ang, two=True)
    assert np.array_equal(bits(s), bits(want_s)) and np.array_equal(bits(c), bits(want_c))
    assert s[0] == 0.0 and c[0] == 1.0 and s[-1] > 0.0


@pytest.mark.gpu
def test_no_table_when_switched_off_or_for_another_calculator(gpu_ctx):
    from atm_raytracer_amd import synth
    cfg, _ = synth.scene("S2", 8, 8, generator="Rectilinear", max_distance=5_000.0)
    before = os.environ.pop("ATMRT_STEP_TRIG", None)
    try:
        assert _table(gpu_ctx, cfg)[0] == 51
        os.environ["ATMRT_STEP_TRIG"] = "off"
        assert _table(gpu_ctx, cfg)[0] == 0
        os.environ.pop("ATMRT_STEP_TRIG")
        for earth in ("Wgs84", "AzimuthalEquidistant", "FlatDistorted"):
            cfg, _ = synth.scene("S2", 8, 8, generator="Rectilinear", max_distance=5_000.0, earth_shape=earth)
            assert _table(gpu_ctx, cfg)[0] == 0, earth
    finally:
        os.environ.pop("ATMRT_STEP_TRIG", None)
        if before is not None:
            os.environ["ATMRT_STEP_TRIG"] = before


# ---- small frames against the oracle, table on and off, under every march variant ----
def frames():
    """name -> (cfg, tiles).  64 x 32 and 130 x 17 (tail wavefronts, a row count that does not divide the block); refracted and straight
    rays; 2 samples per ray (max_distance = 1.5 steps: the table's entries 0 and 1, its first and its last) and 2000 (the headline's
    count: entry 2000 is the last); opaque and translucent terrain; objects; a 3-tile column split; the other three calculators."""
    from atm_raytracer_amd import synth
    out = {}

    def add(name, w, h, objects=False, cols=None, **kw):
        cfg, tiles = synth.scene("S2", w, h, generator="Rectilinear", level=301, **kw)
        if objects:
            synth.add_objects(cfg, n_cyl=8, n_bill=4, dist=(300.0, 20_000.0), spread_deg=30.0, radius=(30.0, 120.0), height=(150.0, 600.0),
                              bill_w=(150.0, 500.0), bill_h=(150.0, 500.0))
        if cols:
            cfg.params.col_begin, cfg.params.col_end = cols
        out[name] = (cfg, tiles)

    add("refracted-opaque-2000", 64, 32, tilt=-1.0)
    add("straight-translucent-2000", 130, 17, tilt=-1.0, straight_rays=True, terrain_alpha=0.5)
    add("refracted-translucent-2", 130, 17, tilt=-40.0, max_distance=150.0, terrain_alpha=0.5)
    add("straight-opaque-2", 64, 32, tilt=-40.0, max_distance=150.0, straight_rays=True)
    add("objects-translucent", 64, 32, objects=True, tilt=-1.0, max_distance=60_000.0, terrain_alpha=0.5)
    add("objects-opaque", 130, 17, objects=True, tilt=-1.0, max_distance=60_000.0)
    for k, cols in enumerate(((0, 43), (43, 87), (87, 130))):
        add("tile%d" % k, 130, 17, cols=cols, tilt=-1.0, max_distance=60_000.0)
    for earth in ("AzimuthalEquidistant", "FlatDistorted", "Wgs84"):
        add(earth, 64, 32, tilt=-1.0, max_distance=60_000.0, earth_shape=earth)
    return out


def digest(r):
    from util import FIELDS_HIT, FIELDS_PIXEL, bits
    h = hashlib.sha256()
    for k in FIELDS_PIXEL + FIELDS_HIT:
        h.update(np.ascontiguousarray(bits(r[k])).tobytes())
    return [h.hexdigest(), int(r["n_hits"]), int(r["ray_steps"])]


CHILD = r"""
import json, os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
from atm_raytracer_amd import generators
from util import run_gpu
import test_gpu_step_trig as T
ctx = generators.Context(0)
out = {{}}
for name, (cfg, tiles) in T.frames().items():
    res = {{}}
    for trig in ("on", "off"):
        if trig == "off":
            os.environ["ATMRT_STEP_TRIG"] = "off"
        else:
            os.environ.pop("ATMRT_STEP_TRIG", None)
        res[trig] = T.digest(run_gpu(ctx, cfg, tiles))
    out[name] = res
os.environ.pop("ATMRT_STEP_TRIG", None)
print("RESULT " + json.dumps(out))
"""

_WANT = {}


def _oracle_frames(oracle_det):
    from util import run_oracle
    if not _WANT:
        for name, (cfg, tiles) in frames().items():
            _WANT[name] = digest(run_oracle(oracle_det, cfg, tiles))
    return _WANT


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [None, "plain", "small", "sliced", "queue"])
def test_frames_equal_the_oracle_with_the_table_on_and_off(oracle_det, variant):
    """plain: the whole-frame march and, for the rays it gives up next to objects, k_rect_trace; small: object steps out of line
    (object_step_impl); sliced (what small opaque frames take by default, forced here for the others): k_rect_march_first / _cont,
    whose later slices start at a step index read back from HBM; queue: k_rect_march_queue on the opaque whole frames without objects
    of the Spherical calculator (refracted-opaque-2000 and straight-opaque-2, a frame of two samples), the others by their size."""
    want = _oracle_frames(oracle_det)
    assert want["refracted-translucent-2"][1] > 0 and want["straight-opaque-2"][1] > 0, "the 2-sample frames must have trace points"
    assert want["objects-translucent"][1] > want["refracted-opaque-2000"][1] > 0
    env = dict(os.environ)
    env.pop("ATMRT_STEP_TRIG", None)
    if variant:
        env["ATMRT_MARCH_VARIANT"] = variant
    else:
        env.pop("ATMRT_MARCH_VARIANT", None)
    p = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], env=env, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    got = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])
    assert set(got) == set(want)
    for name, r in got.items():
        assert r["on"] == want[name], (name, "table on", r["on"], want[name])
        assert r["off"] == want[name], (name, "table off", r["off"], want[name])


# ---- the table's lifetime ----
@pytest.mark.gpu
def test_one_context_follows_step_distance_radius_and_earth_model(gpu_ctx):
    """One context through frames that change the step, then max_distance, then the radius, then the earth model, then return to the
    first: each frame equals the frame of a context that has seen nothing else."""
    from atm_raytracer_amd import generators, synth
    from util import assert_bitexact, run_gpu
    base = dict(tilt=-1.0, max_distance=40_000.0, terrain_alpha=0.5)
    sequence = [dict(base), dict(base, step=70.0), dict(base, step=70.0, max_distance=55_000.0),
                dict(base, step=70.0, max_distance=55_000.0, earth_shape={"Spherical": {"radius": 5_000_000.0}}),
                dict(base, step=70.0, max_distance=55_000.0, earth_shape="Wgs84"), dict(base)]
    for kw in sequence:
        cfg, tiles = synth.scene("S2", 64, 32, generator="Rectilinear", level=301, **kw)
        got = run_gpu(gpu_ctx, cfg, tiles)
        fresh = generators.Context(0)
        try:
            want = run_gpu(fresh, cfg, tiles)
        finally:
            fresh.close()
        assert want["n_hits"] > 0
        assert_bitexact(got, want)
