"""The escape certificate on the GPU: a Rectilinear ray above the mosaic's top (and its wavefront's objects)
that is provably ascending to max_distance leaves the march and is credited the steps it did not integrate.  With the shortcut on
(the default) and off (ATMRT_ESCAPE=off, read at every frame) every plane, n_hits and ray_steps must be the same bits, under every
march variant (ATMRT_MARCH_VARIANT is read once per process: one child per variant); and scenes built to tempt a wrong escape must
still match the oracle."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import ctypes as C, hashlib, json, os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import numpy as np
from atm_raytracer_amd import generators, synth
from util import run_gpu, FIELDS_PIXEL, FIELDS_HIT, bits
full = {full!r}
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
for name, kw, objects, size, cols in scenes:
    cfg, t = synth.scene("headline", size[0], size[1], generator="Rectilinear", level=1, **kw)
    tiles = tiles or t
    if cols:
        cfg.params.col_begin, cfg.params.col_end = cols
    if objects:
        synth.add_objects(cfg, n_cyl=300, n_bill=100, dist=(1_000.0, 100_000.0), spread_deg=60.0)
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
        res[esc] = [h.hexdigest(), int(r["n_hits"]), int(r["ray_steps"]), integrated, escaped]
    out[name] = res
os.environ.pop("ATMRT_ESCAPE", None)
print("RESULT " + json.dumps(out))
"""


def _run(variant, full):
    env = dict(os.environ)
    env.pop("ATMRT_ESCAPE", None)
    if variant:
        env["ATMRT_MARCH_VARIANT"] = variant
    else:
        env.pop("ATMRT_MARCH_VARIANT", None)
    p = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), full=full)], env=env,
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
    """A strong inversion just above the mosaic's top (dn/dh far below -1/R): rays that rise into it bend back down and hit terrain
    far out.  The certificate refuses the inversion: no ray may escape below it."""
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
