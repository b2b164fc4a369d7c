"""tests/horizon_model.py alone, from the oracle's primitives: the sea horizon on a sphere with straight rays against its closed form,
every bracket of a ridge scene against the sight-line model's probe of the same two angles, and the per-ray rule on made-up paths.
No device."""
import math

import numpy as np

import horizon_model as hm
import sight_model as sm
from atm_raytracer_amd import synth

R = 6_371_000.0


def test_sea_horizon_on_a_sphere_with_straight_rays(oracle_det):
    """No terrain, a sphere of 6371 km, straight rays, the observer 100 m up: the skyline is the geometric dip -acos(R / (R + 100)), at
    sqrt(2 * 100 * R) = 35.7 km.  The bound of 1e-6 degrees: a grazing ray can pass at most step^2 / (8 R) = 2e-4 m under the sea
    between two samples unseen, 3.2e-7 degrees at 35.7 km."""
    cfg, tiles = synth.scene("S1", 64, 48)
    assert not tiles and cfg.params.straight_rays == 1 and cfg.params.position.altitude == 100.0 and cfg.params.simulation_step == 100.0
    assert cfg.params.earth.radius == R
    dip = -math.degrees(math.acos(R / (R + 100.0)))
    setting = sm.Setting(oracle_det, cfg, tiles)
    try:
        for rounds in (1, 2, 3, 4):
            rec = hm.solve(setting, 10.0, 0.0, 1, 80_000.0, (-3.0, 3.0), 256, rounds)[0][0]
            print(f"horizon model sea rounds={rounds}: status {rec['status']} bracket {rec['angle_blocked'] - dip:+.3e} .. {rec['angle_clear'] - dip:+.3e} deg "
                  f"around the dip {dip:.8f}, resolution {rec['resolution']:.3e}, block_index {rec['block_index']} at {rec['block_distance']:.0f} m")
            assert rec["status"] == hm.FOUND and rec["rounds_done"] == rounds
            assert rec["angle_blocked"] <= dip + 1e-6 and rec["angle_clear"] >= dip - 1e-6
            assert rec["angle_blocked"] < rec["angle_clear"]
            if rounds >= 2:
                assert abs(rec["block_distance"] - math.sqrt(2.0 * 100.0 * R)) < 2_000.0
                assert rec["block_elevation"] == 0.0
    finally:
        setting.close()


def test_brackets_equal_the_sight_models_probe(oracle_det):
    """Scene S2: the two angles of every record, probed by the sight-line model against the target one sample beyond the reach — whose m
    is m + 1, so that its block test runs through i = m — give [block_index, -1]."""
    cfg, tiles = synth.scene("S2", 64, 48, generator="Fast", max_distance=60_000.0)
    setting = sm.Setting(oracle_det, cfg, tiles)
    try:
        reach = 30_000.0
        d, m = sm.lattice(setting.step, reach)
        for az in (0.0, 86.0, 133.0, 200.0, 270.0):
            rec = hm.solve(setting, az, 0.0, 1, reach, (-6.0, 6.0), 128, 3)[0][0]
            rays = sm.fan_probe(setting, (az, d[m] + setting.step, 0.0), [rec["angle_blocked"], rec["angle_clear"]])
            print(f"horizon model az={az:g}: k*={rec['k_star']} bracket [{rec['angle_blocked']:.6f}, {rec['angle_clear']:.6f}] ridge at "
                  f"{rec['block_distance']:.0f} m, {rec['block_elevation']:.1f} m; probe {rays['block_index'].tolist()}")
            assert rec["status"] == hm.FOUND and rec["rounds_done"] == 3
            assert rays["block_index"].tolist() == [rec["block_index"], -1]
            assert 1 <= rec["block_index"] <= m and rec["block_distance"] == d[rec["block_index"]]
    finally:
        setting.close()


def test_rules_on_made_up_paths():
    """m = 3.  A ray blocked exactly at i' = m; a ray that is NaN at m and not blocked (fails, block -1); a clear ray below a failing
    one (k* is still one above the highest failing ray); no ray failing; all failing."""
    T = np.array([0.0, 10.0, 10.0, 10.0])
    angles = np.array([-1.0, 0.0, 1.0, 2.0])
    H = np.array([[50.0, 40.0, 30.0, 5.0],      # crosses the ground between 2 and 3: blocked at i' = m
                  [50.0, 40.0, 30.0, 30.0],     # clear, below a failing ray
                  [50.0, 40.0, 30.0, np.nan],   # NaN at m, never blocked: fails, block -1
                  [50.0, 60.0, 70.0, 80.0]])    # clear
    fails, block = hm.trace(H, T)
    assert fails.tolist() == [True, False, True, False] and block.tolist() == [3, -1, -1, -1]
    assert hm.first_round(H, T, angles) == (hm.FOUND, 3, -1, 2.0, 1.0)
    assert hm.first_round(H[:2], T, angles[:2]) == (hm.FOUND, 1, 3, 0.0, -1.0)
    # a NaN on the way neither blocks nor fails; under -1000 at i' - 1 blocks at i'
    fails, block = hm.trace(np.array([[50.0, np.nan, 30.0, 30.0], [50.0, -2000.0, -2000.0, -2000.0], [50.0, 40.0, -1500.0, 20.0]]), np.full(4, -5000.0))
    assert fails.tolist() == [False, True, True] and block.tolist() == [-1, 2, 3]
    status, k, blk, clear, blocked = hm.first_round(H[[1, 3]], T, angles[:2])  # no ray fails
    assert (status, k, blk, clear) == (hm.BELOW_FAN, 0, -1, -1.0) and np.isnan(blocked)
    status, k, blk, clear, blocked = hm.first_round(H[[2, 0]], T, angles[:2])  # every ray fails: the record is ray K - 1's
    assert (status, k, blk, blocked) == (hm.ABOVE_FAN, 2, 3, 0.0) and np.isnan(clear)
    status, k, blk, clear, blocked = hm.first_round(H[[0, 2]], T, angles[:2])  # ray K - 1 failed by NaN
    assert (status, k, blk, blocked) == (hm.ABOVE_FAN, 2, -1, 0.0) and np.isnan(clear)
    # the records: NaN where there is no block index; a discarded round keeps the bracket and counts
    d, lat, lon = np.arange(4) * 100.0, np.arange(4) + 0.5, np.arange(4) + 8.5
    rec = hm.record(hm.FOUND, 1, 1, 3, 0.0, -1.0, 1.0, d, lat, lon, T)
    assert (rec["block_distance"], rec["block_lat"], rec["block_lon"], rec["block_elevation"]) == (300.0, 3.5, 11.5, 10.0)
    rec = hm.record(hm.FOUND, 1, 3, -1, 2.0, 1.0, 1.0, d, lat, lon, T)
    assert all(np.isnan(rec[k]) for k in ("block_distance", "block_lat", "block_lon", "block_elevation"))
    all_fail = lambda e, m: np.tile(H[0], (64, 1))  # noqa: E731
    none_fail = lambda e, m: np.tile(H[3], (64, 1))  # noqa: E731
    assert hm.refine(all_fail, T, 3, -1.0, 0.0, 3, 1.0, 4) == (-1.0, 0.0, 3, 1.0, 2)
    assert hm.refine(none_fail, T, 3, -1.0, 0.0, 3, 1.0, 4) == (-1.0, 0.0, -1, 1.0, 2)  # cannot happen on a device: ray 0 is the failing ray of before
    assert hm.refine(all_fail, T, 3, -1.0, 0.0, 3, 1.0, 1) == (-1.0, 0.0, 3, 1.0, 1)
    half = lambda e, m: np.where((e < -0.5)[:, None], H[0][None, :], H[3][None, :])  # noqa: E731
    lo, hi, blk, res, done = hm.refine(half, T, 3, -1.0, 0.0, 3, 1.0, 2)
    e = sm.fan_angles(-1.0, 0.0)
    assert (lo, hi, blk, res, done) == (e[31], e[32], 3, 1.0 / 63.0, 2) and e[31] < -0.5 <= e[32]
