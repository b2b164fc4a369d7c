"""tests/sight_model.py alone, from the oracle's primitives (coords_at_dist, get_elev, ray_paths of the deterministic flavour): on a
bare sphere with straight rays the rule must reproduce the closed-form horizon geometry.  And the inverse geodesic of
generators.sight_targets against the oracle's coords_at_dist.  No device."""
import math

import numpy as np
import pytest

import sight_model as sm
from atm_raytracer_amd import generators, synth
from atm_raytracer_amd.config import Config

R, H0, D, STEP = 6_371_000.0, 100.0, 80_000.0, 100.0
FAN, ROUNDS = (-1.0, 1.0), 3


@pytest.fixture(scope="module")
def setting(oracle_det):
    # scene S1: no terrain, Spherical 6 371 000 m, straight rays, observer Absolute 100 m, step 100 m
    cfg, tiles = synth.scene("S1", 64, 48)
    p = cfg.params
    assert not tiles and p.straight_rays == 1 and p.simulation_step == STEP and p.position.altitude == H0 and p.earth.radius == R
    s = sm.Setting(oracle_det, cfg, tiles)
    yield s
    s.close()


def tangent_height():
    """Height at surface distance D of the ray from H0 that touches the sphere: it touches at the central angle acos(R / (R + H0))
    from the observer, and a straight line tangent there stands R / cos(angle beyond) - R above the sphere."""
    return R / math.cos(D / R - math.acos(R / (R + H0))) - R


def tolerance(resolution_deg):
    """2 * (D * resolution + step^2 / (8 R)).  First term: the first passing ray and the failing ray below it are `resolution`
    apart in angle, so D * resolution apart in height at the target, and the true threshold lies between them.  Second term: the
    rule tests the ray at the samples only; between two samples one step apart the sphere bulges above their chord by at most
    step^2 / (8 R) (the sagitta of a chord of that length), so a ray may pass that much below the tangent ray unnoticed — lower by
    the angle sag / tangent distance, which at the target, D / tangent distance ~ 2.2 times as far, is 2.2 sags.  The factor 2
    covers that lever and the rounding of the lattice."""
    return 2.0 * (D * math.radians(resolution_deg) + STEP * STEP / (8.0 * R))


def test_hidden_height_is_the_tangent_rays(setting):
    rec = sm.solve(setting, [(90.0, D, 0.0)], FAN, ROUNDS)[0]
    want, tol = tangent_height(), tolerance(rec["resolution"])
    print(f"sight model: status {rec['status']} hidden {rec['hidden']:.6f} m, closed form {want:.6f} m, tolerance {tol:.6f} m, "
          f"resolution {rec['resolution']:.3e} deg, block at {rec['block_distance']:.0f} m")
    assert rec["status"] == sm.HIDDEN and rec["rounds_done"] == ROUNDS and rec["m"] == 800 and rec["ground"] == 0.0
    assert rec["resolution"] == (FAN[1] - FAN[0]) / 63.0 ** 3 or abs(rec["resolution"] / ((FAN[1] - FAN[0]) / 63.0 ** 3) - 1) < 1e-9
    assert abs(rec["hidden"] - want) <= tol, (rec["hidden"], want, tol)
    assert rec["hidden"] == rec["arrival"] - 0.0 and 100.0 < want < 200.0


def test_height_above_and_below_the_hidden_height(setting):
    want = tangent_height()
    above, below = sm.solve(setting, [(90.0, D, want + 50.0), (90.0, D, 0.5 * want)], FAN, ROUNDS)
    assert above["status"] == sm.SEEN and above["block_index"] == -1 and np.isnan(above["block_distance"])
    assert 0.0 <= above["hidden"] <= D * math.radians(above["resolution"]) * 2.0  # the first ray at or above the aim: within one spacing
    # the angle of the straight ray from (0, H0) to the aimed point, by plane geometry on the sphere's section
    phi = D / R
    x, y = (R + want + 50.0) * math.sin(phi), (R + want + 50.0) * math.cos(phi) - (R + H0)
    assert abs(above["angle"] - math.degrees(math.atan2(y, x))) <= 2.0 * above["resolution"]
    assert below["status"] == sm.HIDDEN
    # ray k* - 1 lies below the tangent ray by at most the sag's angle plus one spacing, so it is under ground only where the tangent
    # ray, (x - x_t)^2 / (2 R) above it, is lower than x_t * that angle: within sqrt(2 R (sag + x_t * spacing)) of the tangent
    # distance x_t; the rule names the first sample behind the crossing, hence + step; the factor 2 as in tolerance()
    x_t = R * math.acos(R / (R + H0))
    reach = 2.0 * (math.sqrt(2.0 * R * (STEP * STEP / (8.0 * R) + x_t * math.radians(below["resolution"]))) + STEP)
    print(f"sight model: blocked at {below['block_distance']:.0f} m, tangent distance {x_t:.0f} m, allowed +-{reach:.0f} m")
    assert abs(below["block_distance"] - x_t) <= reach and below["block_elevation"] == 0.0
    assert below["block_distance"] == below["block_index"] * STEP
    assert abs(below["hidden"] - 0.5 * want) <= tolerance(below["resolution"])


def test_fans_off_the_target(setting):
    low, high, one = sm.solve(setting, [(90.0, D, 0.0)], (-3.0, -1.0), ROUNDS)[0], sm.solve(setting, [(90.0, D, 0.0)], (1.0, 3.0), ROUNDS)[0], \
        sm.solve(setting, [(90.0, D, 0.0)], FAN, 1)[0]
    assert low["status"] == sm.ABOVE_FAN and low["rounds_done"] == 1 and np.isnan(low["angle"]) and np.isnan(low["hidden"])
    assert high["status"] == sm.BELOW_FAN and high["rounds_done"] == 1 and high["angle"] == 1.0 and high["hidden"] > 0
    assert one["rounds_done"] == 1 and one["resolution"] == 2.0 / 63.0 and one["status"] == sm.HIDDEN


def test_trace_rules_on_made_up_paths():
    """The per-ray rule on hand-made heights: strict sign change, the -1000 m stop, the earlier of the two, m = 1, NaN."""
    d = np.arange(6, dtype=np.float64) * 100.0
    T = np.array([0.0, 10.0, 10.0, 10.0, 10.0, 10.0])
    H = np.array([
        [50.0, 40.0, 30.0, 20.0, 15.0, 12.0],      # clears: arrives
        [50.0, 10.0, 5.0, 20.0, 15.0, 12.0],       # touches (c = 0) at 1, then below at 2: 0 * -5 is not < 0 — no block at 2; -5 * 10 blocks at 3
        [50.0, 40.0, 5.0, 20.0, 15.0, 12.0],       # blocked at 2
        [50.0, -2000.0, -3000.0, 20.0, 15.0, 12.0],  # sign change at 1 (before the -1000 rule could stop it at 2)
        [50.0, 40.0, 30.0, 20.0, 5.0, 12.0],       # c_4 < 0: i = 4 = m - 1 still counts
        [50.0, 40.0, 30.0, 20.0, 15.0, 2.0],       # below the terrain only at m: arrives (low)
        [50.0, np.nan, 30.0, 20.0, 15.0, 12.0],    # a NaN never blocks; the arrival is fine
    ])
    r = sm.trace(H, T, d, 5, 450.0)
    assert r["block_index"].tolist() == [-1, 3, 2, 1, 4, -1, -1]
    assert r["arrival"][0] == 15.0 + 0.5 * (12.0 - 15.0) and r["arrival"][5] == 15.0 + 0.5 * (2.0 - 15.0) and np.isnan(r["arrival"][[1, 2, 3, 4]]).all()
    assert r["min_index"].tolist() == [4, 2, 2, 1, 4, 4, 4] and r["min_clearance"].tolist()[:3] == [5.0, -5.0, -5.0]
    below = np.array([[-1500.0, -1400.0, -1300.0, -1200.0, -1100.0, -900.0]])  # under -1000 m and under the terrain throughout: stops at 1
    assert sm.trace(below, T, d, 5, 450.0)["block_index"][0] == 1
    one = sm.trace(H[:1, :2], T[:2], d[:2], 1, 30.0)  # m = 1: nothing to test, c_0 is the minimum
    assert one["block_index"][0] == -1 and one["arrival"][0] == 50.0 + 0.3 * (40.0 - 50.0) and one["min_index"][0] == 0 and one["min_clearance"][0] == 50.0
    assert sm.lattice(100.0, 300.0)[1] == 3 and sm.lattice(100.0, 300.5)[1] == 4 and sm.lattice(100.0, 1e-9)[1] == 1


EARTHS = {"Spherical": {"Spherical": {"radius": 6371000.0}}, "Ellipsoid": "Wgs84", "FlatDistorted": "FlatDistorted"}


@pytest.mark.parametrize("earth", sorted(EARTHS))
def test_inverse_geodesic_lands_on_the_point(oracle_det, earth):
    cfg = Config.from_dict({"view": {"position": {"latitude": 46.5, "longitude": 8.5, "altitude": {"Absolute": 100.0}}},
                            "earth_shape": EARTHS[earth]})
    e = cfg.params.earth
    lat0, lon0 = 46.5, 8.5
    az = np.repeat([10.0, 100.0, 190.0, 280.0], 3)
    dist = np.tile([5_000.0, 50_000.0, 150_000.0], 4)
    pts = np.array([oracle_det.coords_at_dist(e, lat0, lon0, a, [d])[0] for a, d in zip(az, dist)])

    def forward(a, d):
        return tuple(oracle_det.coords_at_dist(e, lat0, lon0, a, [d])[0])

    got_az, got_d = generators.inverse_geodesic(forward, lat0, lon0, pts[:, 0].copy(), pts[:, 1].copy(), 6371000.0, exact=earth == "Spherical")
    for a, d, (la, lo) in zip(got_az, got_d, pts):
        fl, fo = forward(float(a), float(d))
        assert abs(fl - la) <= 1e-9 and abs(fo - lo) <= 1e-9, (earth, a, d, fl - la, fo - lo)
    assert np.allclose((got_az - az + 180.0) % 360.0 - 180.0, 0.0, atol=1e-6) and np.allclose(got_d, dist, atol=1e-3)
