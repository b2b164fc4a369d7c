"""The steppers' own evaluation of n(h) and dn/dh (refr_n_dn_hint: the tight vote, then the certified vote, then the generic path,
each decided per wavefront) at the EDGES of the intervals atm_certify hands it, and frames whose rays cross those edges.

tests/test_gpu_detmath.py runs the shortcut sequences of a tight segment on operands at the certified distance; here the operands
are the ones real atmospheres produce where that distance is reached: a standard troposphere is tight up to 23 km with a dense-sample
max_dt_rel of 0.99 x 2^-21, a lapse rate of -13.6 K/km is tight over the lowest six metres only, -14 K/km nowhere.  Altitudes are
arranged by wavefront (atmrt_atmosphere_sample launches blocks of 256: elements 64 w .. 64 w + 63 vote together) so that each of
the three paths, and each hand-over between them, is taken on purpose; every value is compared bit for bit with the oracle."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cbuild
from atm_raytracer_amd import config, generators
from test_core_host import _certify
from util import FIELDS_HIT, FIELDS_PIXEL, assert_bitexact, bits, run_gpu, run_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAVE = 64


def single_layer(gradient):
    return {"pressure": {"altitude": 0.0, "pressure": 101325.0}, "temperature_fixed_point": {"altitude": 0.0, "temperature": 288.15},
            "first_temperature_function": {"Linear": {"gradient": gradient}}}


TWO_LAYER = {"pressure": {"altitude": 100.0, "pressure": 100000.0}, "first_temperature_function": {"Linear": {"gradient": -0.008}},
             "next_functions": [{"altitude": 2000.0, "function": {"Linear": {"gradient": 0.002}}},
                                {"altitude": 9000.0, "function": {"Linear": {"gradient": 0.0}}}],
             "temperature_fixed_point": {"altitude": 2500.0, "temperature": 270.0}}
ATMOSPHERES = {"-6.5 K/km": single_layer(-0.0065), "-13.6 K/km": single_layer(-0.0136), "-14 K/km": single_layer(-0.014), "US-76": None,
               "isothermal above 9 km": TWO_LAYER}


def cfg_of(name, **doc):
    atm = ATMOSPHERES[name]
    return config.Config.from_dict({**({"atmosphere": atm} if atm else {}), "output": {"width": 8, "height": 8}, "simulation_step": 100.0, **doc})


@pytest.fixture(scope="module")
def certificates():
    core = C.CDLL(cbuild.core_host())
    out = {}
    for name in ATMOSPHERES:
        cfg = cfg_of(name)
        out[name] = _certify(core, cfg.atmosphere, step=cfg.params.simulation_step, wavelength=cfg.params.wavelength)[0]
    return out


def test_the_atmospheres_have_the_tight_intervals_the_cases_rely_on(certificates):
    """What makes the cases below meaningful, from the certificate alone (no GPU)."""
    c = certificates["-6.5 K/km"]
    assert int(c["flags"][0]) & 2 and c["tight_lo"][0] < 1.0 and 23000.0 < c["tight_hi"][0] < 23300.0 and c["tight_hi"][0] < c["safe_hi"][0]
    assert 0.98 * 2.0 ** -21 < c["max_dt_rel"][0] <= 2.0 ** -21, "a standard troposphere runs the vote-free forms at 99 % of the bound"
    c = certificates["-13.6 K/km"]
    assert int(c["flags"][0]) & 2 and 0.0 < c["tight_hi"][0] < 10.0 and c["tight_hi"][0] < c["safe_hi"][0]
    c = certificates["-14 K/km"]
    assert not int(c["flags"][0]) & 2 and c["tight_lo"][0] == np.inf and c["safe_lo"][0] < 0.0 < 1000.0 < c["safe_hi"][0]
    c = certificates["US-76"]
    assert [int(f) & 2 for f in c["flags"]] == [2] * 7
    c = certificates["isothermal above 9 km"]
    assert int(c["flags"][2]) == 3 and c["tight_lo"][2] == 9000.0, "the upper layer is isothermal and tight from its base"


def wavefronts_at_the_edges(c, rng):
    """Altitudes, 64 per wavefront, around every end of every certified and tight interval of the certificate c."""
    eps, waves = 0.01, []

    def below(x, width=1.0):  # the largest altitude whose h + eps is below x, and 63 more within `width` under it
        top = np.nextafter(x - eps, -np.inf)
        while top + eps >= x:
            top = np.nextafter(top, -np.inf)
        return np.concatenate([[top], top - rng.uniform(0.0, width, WAVE - 1)])

    def above(x, width=1.0):  # the smallest altitude whose h - eps is at or above x, and 63 more
        bot = np.nextafter(x + eps, np.inf)
        while bot - eps < x:
            bot = np.nextafter(bot, np.inf)
        return np.concatenate([[bot], bot + rng.uniform(0.0, width, WAVE - 1)])

    n = len(c["from"])
    for k in range(n):
        lo, hi = max(c["safe_lo"][k], -90000.0), min(c["safe_hi"][k], 9.0e6)
        if not lo < hi:
            continue
        ends = [(lo, hi)]
        if int(c["flags"][k]) & 2:
            tl, th = max(c["tight_lo"][k], -90000.0), min(c["tight_hi"][k], 9.0e6)
            ends.append((tl, th))
            inside = below(th)
            for lane, h in ((0, th), (17, th + 0.005), (63, np.nextafter(th, np.inf)), (5, th - 0.005)):  # 63 lanes tight, one not: the certified vote
                w = inside.copy()
                w[lane] = h
                waves.append(w)
        for a, b in ends:
            waves += [below(b), above(a), rng.uniform(b - 1.0, b + 1.0, WAVE), rng.uniform(a - 1.0, a + 1.0, WAVE),
                      rng.uniform(a, b, WAVE)]
            waves.append(np.concatenate([below(b, 0.02)[:32], above(b, 0.02)[:32]]))
    for k in range(1, n):  # the layer boundaries: wavefronts that straddle them, and wavefronts whose lane 0 (the hint's) is in another layer
        f = c["from"][k]
        waves.append(rng.uniform(f - 1.0, f + 1.0, WAVE))
        waves.append(np.concatenate([[f, np.nextafter(f, -np.inf), f - eps, f + eps], rng.uniform(f - 0.03, f + 0.03, WAVE - 4)]))
        for first, rest in ((f - 50.0, above(f, 100.0)[1:]), (f + 50.0, below(f, 100.0)[1:]), (np.nextafter(f, -np.inf), above(f)[1:])):
            waves.append(np.concatenate([[first], rest]))
    return np.concatenate(waves)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ATMOSPHERES))
def test_n_and_dn_at_the_ends_of_the_tight_and_certified_intervals(gpu_ctx, oracle_det, certificates, name):
    cfg = cfg_of(name)
    rng = np.random.default_rng(71)
    alt = wavefronts_at_the_edges(certificates[name], rng)
    assert alt.size % WAVE == 0 and alt.size < 12000
    gpu_ctx.check(gpu_ctx.lib.atmrt_set_params(gpu_ctx.handle, C.byref(cfg.params)))
    gpu_ctx.check(gpu_ctx.lib.atmrt_set_atmosphere(gpu_ctx.handle, C.byref(cfg.atmosphere)))
    try:
        got = generators.atmosphere_sample(gpu_ctx, alt)
    finally:
        us = config.us76()
        gpu_ctx.check(gpu_ctx.lib.atmrt_set_atmosphere(gpu_ctx.handle, C.byref(us)))
    env = oracle_det.env(cfg.atmosphere, cfg.params.wavelength)
    want_n = np.array([oracle_det.n(env, float(h)) for h in alt])
    want_dn = np.array([oracle_det.dn(env, float(h)) for h in alt])
    for key, want in (("n", want_n), ("dn_dh", want_dn)):
        bad = np.flatnonzero(bits(got[key]) != bits(want))
        assert bad.size == 0, (f"{name}: {key} differs at {bad.size} of {alt.size} altitudes, e.g. h = {alt[bad[:3]]!r} (wavefronts {bad[:3] // WAVE}): "
                               f"{got[key][bad[:3]]!r} against {want[bad[:3]]!r}")


FRAMES = {
    # rays start at 3 m and climb through tight_hi = 6.26 m within the first kilometres, neighbouring rows a few steps apart
    "-13.6 K/km": dict(view={"position": {"altitude": {"Absolute": 3.0}}, "frame": {"max_distance": 20000.0, "tilt": 0.0, "fov": 1.0}}),
    # rays climb through tight_hi at 23.1 km (and stay certified above it)
    "-6.5 K/km": dict(view={"position": {"altitude": {"Absolute": 3.0}}, "frame": {"max_distance": 60000.0, "tilt": 30.0, "fov": 30.0}}),
}
SIZES = {"Rectilinear": (64, 24), "Fast": (64, 32)}


def frame_cfg(name, generator):
    w, h = SIZES[generator]
    return cfg_of(name, output={"width": w, "height": h, "generator": generator}, **FRAMES[name])


def digest(r):
    h = hashlib.sha256()
    for k in FIELDS_PIXEL + FIELDS_HIT:
        h.update(np.ascontiguousarray(bits(r[k])).tobytes())
    return [h.hexdigest(), int(r["n_hits"]), int(r["ray_steps"])]


@pytest.fixture(scope="module")
def frames(gpu_ctx):
    try:
        return {(name, gen): run_gpu(gpu_ctx, frame_cfg(name, gen), {}) for name in FRAMES for gen in SIZES}
    finally:  # the session's context goes on with the default atmosphere
        us = config.us76()
        gpu_ctx.check(gpu_ctx.lib.atmrt_set_atmosphere(gpu_ctx.handle, C.byref(us)))


@pytest.mark.gpu
@pytest.mark.parametrize("generator", list(SIZES))
@pytest.mark.parametrize("name", list(FRAMES))
def test_frames_whose_rays_cross_the_end_of_the_tight_interval(frames, oracle_det, name, generator):
    """No terrain tiles: sea level everywhere.  Wavefronts hold lanes on both sides of tight_hi for many steps."""
    got = frames[(name, generator)]
    assert got["ray_steps"] > 1000
    assert_bitexact(got, run_oracle(oracle_det, frame_cfg(name, generator), {}))


CHILD = r"""
import json, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
from atm_raytracer_amd import generators
from util import run_gpu
import test_gpu_tight_segments as t
ctx = generators.Context(0)
print("RESULT " + json.dumps({{name: t.digest(run_gpu(ctx, t.frame_cfg(name, "Rectilinear"), {{}})) for name in t.FRAMES}}))
"""


@pytest.mark.gpu
def test_the_same_frames_without_the_tight_parts(frames):
    """ATMRT_NO_TIGHT=1 (read when the atmosphere is compiled; a fresh process) sends every segment through the voting forms: the
    Rectilinear frames must come out identical to the ones above."""
    env = dict(os.environ, ATMRT_NO_TIGHT="1")
    p = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], env=env, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    assert json.loads(line[len("RESULT "):]) == {name: digest(frames[(name, "Rectilinear")]) for name in FRAMES}
