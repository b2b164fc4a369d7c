"""The record of the trace-point epilogue's frame constants (Frame::normal_trig): for the Spherical calculator
find_normal and rect_hit read the sines and cosines of +-15 m / radius and of azimuths 0 and 90, and the observer's three vectors,
from a record that k_normal_trig fills once per earth model and observer, instead of computing them per trace point; fast_hit reads
the per-step table.  The record must hold the bits a lane computes, frames must equal the oracle's in every plane and every list entry
with the record on and off (ATMRT_NORMAL_TRIG=off, read at every frame: one child process per value), and the record must follow the
radius, the earth model and the observer."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_DIV, PROBE_SINCOS, PROBE_IEEE_DIV = 0, 6, 9  # atmrt_math_probe_op, include/atmrt.h
RAD_PER_DEG = np.pi / 180.0  # dm_to_radians multiplies by this double


def _probe(ctx, op, a, b=None, two=False):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = None if b is None else np.ascontiguousarray(b, dtype=np.float64)
    o0, o1 = np.empty_like(a), np.empty_like(a)
    ctx.check(ctx.lib.atmrt_math_probe(ctx.handle, op, a.size, a.ctypes.data, None if b is None else b.ctypes.data, o0.ctypes.data,
                                       o1.ctypes.data if two else None))
    return (o0, o1) if two else o0


def _record(ctx, cfg):
    from atm_raytracer_amd import generators
    generators.make_generator(generators.Params(cfg), generators.Terrain(ctx))._configure()
    return ctx.debug_normal_trig()


def _want_record(ctx, radius, fast_div, lat, lon):
    """The 17 doubles from the probe's division and dm_sincos and the products of spherical_directions (one rounding each)."""
    ang = _probe(ctx, PROBE_DIV if fast_div else PROBE_IEEE_DIV, [15.0, -15.0], [radius, radius])
    assert np.array_equal(ang, np.array([15.0, -15.0]) / radius)  # both divisions are IEEE's on these operands
    s, c = _probe(ctx, PROBE_SINCOS, [ang[0], ang[1], 0.0 * RAD_PER_DEG, 90.0 * RAD_PER_DEG, lon * RAD_PER_DEG, lat * RAD_PER_DEG], two=True)
    sinlon, coslon, sinlat, coslat = s[4], c[4], s[5], c[5]
    north = [-sinlat * coslon, -sinlat * sinlon, coslat]
    east = [-sinlon, coslon, 0.0]
    up = [coslat * coslon, coslat * sinlon, sinlat]
    return np.array([s[0], c[0], s[1], c[1], s[2], c[2], s[3], c[3]] + north + east + up)


# ---- (a) the record against the per-lane code ----
@pytest.mark.gpu
@pytest.mark.parametrize("radius,fast_div", [(6371000.0, True), (6371000.0 * 7.0 / 6.0, True), (1.0e31, False)])
def test_record_holds_what_a_lane_computes(gpu_ctx, radius, fast_div):
    """Two radii under EARTH_FAST_DIV (dm_div) and one outside its 1e-30 .. 1e30 band (IEEE division); the observer of scene S2."""
    from atm_raytracer_amd import synth
    from util import bits
    cfg, _ = synth.scene("S2", 8, 8, generator="Rectilinear", max_distance=5_000.0, earth_shape={"Spherical": {"radius": radius}})
    got = _record(gpu_ctx, cfg)
    want = _want_record(gpu_ctx, radius, fast_div, cfg.params.position.latitude, cfg.params.position.longitude)
    assert got.size == 17
    assert np.array_equal(bits(got), bits(want)), (got, want)
    assert got[4] == 0.0 and got[5] == 1.0 and got[6] == 1.0 and 6.0e-17 < got[7] < 6.2e-17  # cos 90 degrees is not 0
    assert got[0] > 0.0 > got[2]


@pytest.mark.gpu
def test_no_record_when_switched_off_or_for_another_calculator(gpu_ctx):
    from atm_raytracer_amd import synth
    cfg, _ = synth.scene("S2", 8, 8, generator="Rectilinear", max_distance=5_000.0)
    before = os.environ.pop("ATMRT_NORMAL_TRIG", None)
    try:
        assert _record(gpu_ctx, cfg).size == 17
        os.environ["ATMRT_NORMAL_TRIG"] = "off"
        assert _record(gpu_ctx, cfg).size == 0
        os.environ.pop("ATMRT_NORMAL_TRIG")
        for earth in ("Wgs84", "AzimuthalEquidistant", "FlatDistorted"):
            cfg, _ = synth.scene("S2", 8, 8, generator="Rectilinear", max_distance=5_000.0, earth_shape=earth)
            assert _record(gpu_ctx, cfg).size == 0, earth
    finally:
        os.environ.pop("ATMRT_NORMAL_TRIG", None)
        if before is not None:
            os.environ["ATMRT_NORMAL_TRIG"] = before


# ---- (b) small frames against the oracle, record on and off ----
SIZES = ((96, 40), (64, 3))  # a row ends inside a wavefront; three rows in one wavefront
OTHER_EARTHS = ("AzimuthalEquidistant", "FlatDistorted", "Wgs84")


def frames():
    """name -> (cfg, tiles).  Tiles with relief (scene S2), the camera tilted so that the skyline crosses the frame: hit and miss
    lanes share wavefronts.  Spherical calculator: Rectilinear opaque (k_rect_finalize), terrain_alpha 0.5 (k_rect_finalize_list),
    Fast (k_fast_finalize) and InterpolatingRectilinear; the other three calculators: Rectilinear opaque."""
    from atm_raytracer_amd import synth
    out = {}
    for w, h in SIZES:
        tilt = -4.0 if h == 40 else 2.5  # the skyline of the three rows lies above the horizontal
        kw = dict(level=301, tilt=tilt, max_distance=60_000.0)
        tag = "%dx%d" % (w, h)
        out["rect-opaque-" + tag] = synth.scene("S2", w, h, generator="Rectilinear", **kw)
        out["rect-translucent-" + tag] = synth.scene("S2", w, h, generator="Rectilinear", terrain_alpha=0.5, **kw)
        out["fast-" + tag] = synth.scene("S2", w, h, generator="Fast", **kw)
        out["interpolating-" + tag] = synth.scene("S2", w, h, generator="InterpolatingRectilinear", **kw)
        for earth in OTHER_EARTHS:
            out[earth + "-" + tag] = synth.scene("S2", w, h, generator="Rectilinear", earth_shape=earth, **kw)
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
import test_gpu_normal_trig as T
ctx = generators.Context(0)
out = {{}}
for name, (cfg, tiles) in T.frames().items():
    out[name] = T.digest(run_gpu(ctx, cfg, tiles)) + [int(ctx.debug_normal_trig().size)]
print("RESULT " + json.dumps(out))
"""

_WANT = {}


def _oracle_frames(oracle_det):
    from util import run_oracle
    if not _WANT:
        for name, (cfg, tiles) in frames().items():
            r = run_oracle(oracle_det, cfg, tiles)
            hit = float((r["hit_count"] > 0).mean())
            normals = len(np.unique(np.ascontiguousarray(r["normal"]).reshape(-1, 3), axis=0)) if r["n_hits"] else 0
            _WANT[name] = (digest(r), hit, normals)
    return _WANT


@pytest.mark.gpu
@pytest.mark.parametrize("switch", [None, "off"])
def test_frames_equal_the_oracle_with_the_record_on_and_off(oracle_det, switch):
    want = _oracle_frames(oracle_det)
    for name, (_, hit, normals) in want.items():  # the scene condition, from the oracle's output
        assert 0.2 <= hit <= 0.8 and normals >= 100, (name, hit, normals)
    env = dict(os.environ)
    env.pop("ATMRT_NORMAL_TRIG", None)
    if switch:
        env["ATMRT_NORMAL_TRIG"] = switch
    p = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], env=env, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    got = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])
    assert set(got) == set(want)
    for name, r in got.items():
        assert r[:3] == want[name][0], (name, switch, r, want[name][0])
        spherical = not name.startswith(OTHER_EARTHS)
        assert r[3] == (17 if spherical and not switch else 0), (name, switch, r[3])


# ---- (c) the record's lifetime ----
@pytest.mark.gpu
def test_one_context_follows_radius_earth_model_and_observer(gpu_ctx, oracle_det):
    """One context through a frame, the same frame after a change of the earth radius, then of the earth model, then of the observer's
    position, then the first again: each equals the oracle's, and the read-back follows the key."""
    from atm_raytracer_amd import synth
    from util import assert_bitexact, bits, run_gpu, run_oracle
    base = dict(level=301, tilt=-4.0, max_distance=40_000.0, terrain_alpha=0.5)
    radius2 = 5_000_000.0
    sequence = [(dict(base), None), (dict(base, earth_shape={"Spherical": {"radius": radius2}}), None), (dict(base, earth_shape="Wgs84"), None),
                (dict(base), (46.4375, 8.5625)), (dict(base), None)]
    for kw, pos in sequence:
        cfg, tiles = synth.scene("S2", 96, 40, generator="Rectilinear", **kw)
        if pos:
            cfg.params.position.latitude, cfg.params.position.longitude = pos
        got = run_gpu(gpu_ctx, cfg, tiles)
        want = run_oracle(oracle_det, cfg, tiles)
        assert want["n_hits"] > 0
        assert_bitexact(got, want)
        rec = gpu_ctx.debug_normal_trig()
        if kw.get("earth_shape") == "Wgs84":
            assert rec.size == 0
        else:
            radius = radius2 if "earth_shape" in kw else 6371000.0
            exp = _want_record(gpu_ctx, radius, True, cfg.params.position.latitude, cfg.params.position.longitude)
            assert np.array_equal(bits(rec), bits(exp)), (kw, pos)
