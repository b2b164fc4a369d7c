"""tests/shadow_lights_model.py (the rule of include/atmrt.h, "shadow lights", in numpy over the oracle) over the oracle's frames, and
the conditions on the inputs of tests/test_gpu_shadow_lights.py: every light that is not declared all-lit or all-dark holds both kinds
of pixel, the declared ones are what they are declared, no SHADOWED ray has passed the escape test, and the per-point rule can be
told from the fixed-direction rule of tests/shadow_model.py.  No GPU."""
import numpy as np
import pytest

import shadow_cases as sc
import shadow_lights_cases as slc
import shadow_lights_model as slm
import shadow_model as sm
from util import run_oracle


@pytest.fixture(scope="module")
def frames(oracle_det):
    made = {}

    def get(name, make=None):
        if name not in made:
            cfg, tiles = (make or sc.FRAMES[name])()
            made[name] = (cfg, run_oracle(oracle_det, cfg, tiles), sm.Setting(oracle_det, cfg, tiles))
        return made[name]

    yield get
    for _, _, s in made.values():
        s.close()


@pytest.mark.parametrize("name", sorted(slc.CASES))
def test_every_light_shows_what_it_is_meant_to(frames, oracle_det, name):
    frame, lights, about_shortcut = slc.CASES[name]
    cfg, res, setting = frames(frame)
    dirs = slm.lights_from_angles(oracle_det, cfg.params, slc.angles(name))
    r = slm.solve(setting, res, dirs, slc.REACH)
    hit = int((np.asarray(res["hit_count"]) > 0).sum())
    assert r.m == 200 and r.stats_on["none"] + hit == r.lit_mask.size
    assert r.stats_on["lit"] + r.stats_on["shadowed"] == hit * len(lights)
    assert not ((r.status == sm.SHADOWED) & (r.esc > 0)).any(), "a ray that passed the escape test was shadowed later: the certificate is broken"
    for l, (az, el, meant) in enumerate(lights):
        lit, dark = int((r.status[l] == sm.LIT).sum()), int((r.status[l] == sm.SHADOWED).sum())
        early = int(((r.status[l] == sm.LIT) & (r.esc[l] > 0) & (r.esc[l] < r.m)).sum())
        spread = (np.nanmin(r.elevation[l]), np.nanmax(r.elevation[l])) if hit else (np.nan, np.nan)
        print(f"shadow lights case {name} light {l} ({az}, {el}, {meant}): hit={hit} lit={lit} shadowed={dark} escaping before m={early} "
              f"local elevation {spread[0]:.4f} .. {spread[1]:.4f}")
        assert lit + dark == hit
        assert (((r.lit_mask >> np.uint64(l)) & np.uint64(1)) == (r.status[l] == sm.LIT)).all()
        if frame == "sky":
            assert hit == 0
            continue
        if meant == slc.BOTH:
            assert lit >= 0.05 * hit and dark >= 0.05 * hit
        elif meant == slc.ALL_LIT:
            assert dark == 0
        else:
            assert meant == slc.ALL_DARK and lit == 0
    if about_shortcut:
        lit0 = r.status[0] == sm.LIT
        assert (lit0 & (r.esc[0] > 0) & (r.esc[0] < r.m)).any() and (lit0 & ((r.esc[0] == 0) | (r.esc[0] == r.m))).any()
        assert r.stats_on["integrated_steps"] < r.stats_off["integrated_steps"] and r.stats_on["escaped_rays"] >= 1


def test_the_two_rules_can_be_told_apart(frames, oracle_det):
    """The 60 km scene on a sphere of 3000 km: the light's angles at the observer, fixed for every point (shadow_model.solve),
    against the same light as a world-frame vector (the per-point rule).  Over 55 km the local frame turns by a degree: some pixel
    changes its status."""
    cfg, res, setting = frames("small_sphere", slc.small_sphere_frame)
    az, el = 260.0, 2.0
    fixed = sm.solve(setting, res, (az, el, slc.REACH, 0.0))
    dirs = slm.lights_from_angles(oracle_det, cfg.params, [(az, el)])
    per_point = slm.solve(setting, res, dirs, slc.REACH)
    hit = fixed.status != sm.NONE
    differ = int((fixed.status != per_point.status[0]).sum())
    spread = per_point.elevation[0][hit]
    print(f"shadow lights rules apart: {differ} of {int(hit.sum())} hit pixels differ; local elevation {spread.min():.4f} .. {spread.max():.4f} "
          f"against {el} fixed; fixed shadowed {int((fixed.status == sm.SHADOWED).sum())}, per point {int((per_point.status[0] == sm.SHADOWED).sum())}")
    assert hit.any() and ((per_point.status[0] != sm.NONE) == hit).all()
    assert differ >= 1
    assert spread.max() - spread.min() > 0.5  # degrees: the turn the simplification ignored


def test_the_observers_own_point_sees_the_observers_angles(oracle_det):
    """At the place the angles were given for, the local direction is those angles again (to rounding), so a single point there
    marches as shadow_model.march does with the fixed direction: the two rules meet at the observer."""
    cfg, tiles = sc.FRAMES["fast_50x20"]()
    pos = cfg.params.position
    dirs = slm.lights_from_angles(oracle_det, cfg.params, [(260.0, 2.0)])
    az, el = slm.local_direction(oracle_det, cfg.params.earth, slm.normalise(dirs[0]), pos.latitude, pos.longitude)
    assert abs(az % 360.0 - 260.0) < 1e-9 and abs(el - 2.0) < 1e-9


def test_decided_without_a_march(oracle_det):
    """The zenith, the nadir and a NaN: LIT / SHADOWED block 1 / LIT, 0 steps, whatever the terrain."""
    import shadow_sweep_cases as ssc
    from atm_raytracer_amd import config
    cfg = config.Config.from_dict({
        "view": {"position": {"latitude": 0.0, "longitude": 0.0, "altitude": {"Absolute": 100.0}},
                 "frame": {"direction": 0.0, "fov": 10.0, "tilt": 0.0, "max_distance": 10_000.0}},
        "earth_shape": "SimpleSphere", "simulation_step": 100.0, "output": {"width": 4, "height": 4, "generator": "Rectilinear"}})
    setting = sm.Setting(oracle_det, cfg, {})
    try:
        res = ssc.planes([0.0, 0.0, np.nan], [0.0, 0.0, 0.0], [100.0, 100.0, 100.0], hit=[True, False, True])
        r = slm.solve(setting, res, [[1.0, 0.0, 0.0], [-2.0, 0.0, 0.0]], 5_000.0)
        assert r.m == 50
        assert r.status.tolist() == [[[sm.LIT, sm.NONE, sm.LIT]], [[sm.SHADOWED, sm.NONE, sm.LIT]]]
        assert r.block.tolist() == [[[0, 0, 0]], [[1, 0, 0]]]
        assert r.lit_mask.tolist() == [[1, 0, 3]]
        assert r.stats_on == r.stats_off == dict(none=1, lit=3, shadowed=1, integrated_steps=0, escaped_rays=0)
    finally:
        setting.close()
