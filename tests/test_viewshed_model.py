"""tests/viewshed_model.py alone, from the oracle's primitives: at K = 64 every cell of the viewshed must be the sight-line model's
first round for the target {az_j, d_i, height}, field for field — on a ridge scene and under a ducting atmosphere where rays cross —
and on a flat earth with straight rays and no terrain k* must be the closed-form count.  No device."""
import math

import numpy as np
import pytest

import sight_model as sm
import viewshed_model as vm
from atm_raytracer_amd import _abi, synth
from atmospheres import inversion

FAN = (-6.0, 6.0)
_TILES = {}


def scene(**over):
    """Scene S2 (one synthetic tile, observer 46.5 N 8.5 E, step 100 m)."""
    cfg, tiles = synth.scene("S2", 64, 48, generator="Fast", max_distance=60_000.0, **over)
    if not _TILES:
        _TILES.update(tiles)
    return cfg, _TILES


def ducting_scene():
    """viewshed_model.DUCT on scene S2: the observer inside a strong temperature inversion."""
    cfg, tiles = scene(atmosphere=inversion(vm.DUCT["at"], vm.DUCT["thick"], vm.DUCT["gradient"]))
    cfg.params.position.altitude_kind, cfg.params.position.altitude = _abi.ALT_ABSOLUTE, vm.DUCT["altitude"]
    return cfg, tiles


def check_against_sight_model(setting, az_lo, az_step, n_az, reach, height, tag, FAN=FAN):
    v = vm.solve(setting, az_lo, az_step, n_az, reach, height, FAN, 64)
    d, m = v["d"], v["d"].size - 1
    assert v["angles"].tobytes() == sm.fan_angles(*FAN).tobytes()
    targets = [(float(az), float(d[i]), height) for az in v["azimuths"] for i in range(1, m + 1)]
    want = sm.solve(setting, targets, FAN, rounds=1).reshape(n_az, m)
    counts = np.bincount(v["status"].ravel(), minlength=4).tolist()
    print(f"viewshed model {tag}: {n_az} x {m} cells, seen/hidden/above/below {counts}")
    assert (want["m"] == np.arange(1, m + 1)[None, :]).all() and (want["rounds_done"] == 1).all()
    assert np.array_equal(v["status"], want["status"]), tag
    assert np.array_equal(v["block_index"], want["block_index"]), tag
    assert v["ground"].tobytes() == want["ground"].tobytes(), tag
    # k* through `angle`: e_{k*}, NaN for k* = 64
    angle = np.where(v["k_star"] == 64, np.nan, v["angles"][np.minimum(v["k_star"], 63)])
    for name, got in (("angle", angle), ("hidden", v["hidden"])):
        g, w = got.view(np.uint64).copy(), np.ascontiguousarray(want[name]).view(np.uint64).copy()
        g[np.isnan(got)] = w[np.isnan(want[name])] = 0
        assert np.array_equal(g, w), (tag, name, np.argwhere(g != w)[:5].tolist())
    return v, counts


def test_ridge_scene_equals_the_sight_model(oracle_det):
    cfg, tiles = scene()
    setting = sm.Setting(oracle_det, cfg, tiles)
    try:
        _, counts = check_against_sight_model(setting, 88.0, 4.0, 2, 12_000.0, 0.0, "ridge")
        check_against_sight_model(setting, 92.0, 0.0, 1, 12_000.0, 150.0, "ridge, 150 m tall")
        assert counts[sm.SEEN] and counts[sm.HIDDEN]
    finally:
        setting.close()


def test_ducting_atmosphere_equals_the_sight_model(oracle_det):
    cfg, tiles = ducting_scene()
    setting = sm.Setting(oracle_det, cfg, tiles)
    try:
        v, _ = check_against_sight_model(setting, 30.0, 0.0, 1, 12_000.0, 20.0, "duct", vm.DUCT["fan"])
        H = setting.heights(v["angles"], v["d"].size - 1)
        crossings = int((np.diff(H, axis=0) < 0.0).sum())
        print(f"viewshed model duct: {crossings} places where a ray lies below the ray under it")
        assert crossings > 0, "the ducting atmosphere must make rays cross"
    finally:
        setting.close()


def test_flat_earth_straight_rays_closed_form(oracle_det):
    """No terrain, FlatDistorted, straight rays: ray k stands alt + d_i tan(e_k) above the plane at sample i, rays never cross, and a
    ray that has gone below the plane is below the aim as well — k* is the number of angles with alt + d_i tan(e_k) < height."""
    cfg, tiles = synth.scene("S1", 64, 48, earth_shape="FlatDistorted")
    assert not tiles and cfg.params.straight_rays == 1 and cfg.params.position.altitude == 100.0
    setting = sm.Setting(oracle_det, cfg, tiles)
    try:
        alt, height, fan, K, reach = 100.0, 30.0, (-3.05, 2.9), 128, 6_000.0
        angles = vm.fan_angles(fan[0], fan[1], K)
        d, m = sm.lattice(setting.step, reach)
        line = alt + d[1:, None] * np.tan(np.radians(angles))[None, :]  # [m][K]
        margin = np.abs(line - height).min()
        print(f"viewshed model flat: {m} x {K}, the nearest ray passes {margin:.4f} m from the aim")
        assert margin > 1e-3, "choose another fan: a ray comes too near the aim for an exact comparison"
        v = vm.solve(setting, 10.0, 35.0, 2, reach, height, fan, K)
        want = (line < height).sum(axis=1)
        assert np.array_equal(v["k_star"][0], want) and np.array_equal(v["k_star"][1], want)
        assert want.min() == 0 and 0 < want.max() < K and (np.diff(want) >= 0).all()
        assert (v["ground"] == 0.0).all() and (v["hidden"] >= 0.0).all()
        # no ray fails: BELOW_FAN.  Otherwise ray k* - 1 is merely low (SEEN) unless it has passed below the plane by sample i - 1 (HIDDEN);
        # here the highest ray below a 30 m aim is still above the plane one sample earlier
        gone = alt + d[:-1, None] * np.tan(np.radians(angles))[None, :] < 0.0  # [m][K]: below the plane at i - 1
        expect = np.where(want == 0, sm.BELOW_FAN, np.where(gone[np.arange(m), np.maximum(want - 1, 0)], sm.HIDDEN, sm.SEEN))
        assert np.array_equal(v["status"][0], expect) and set(np.unique(expect).tolist()) == {sm.SEEN, sm.BELOW_FAN}
    finally:
        setting.close()


def test_scan_rules_on_made_up_paths():
    """The per-cell rule on hand-made heights: a blocked ray fails from the NEXT cell on, NaN fails, k* is one above the highest
    failing ray even where a lower ray passes."""
    T = np.array([0.0, 10.0, 10.0, 10.0])
    H = np.array([[50.0, np.nan, 30.0, 30.0],  # NaN at 1: the arrivals of cells 1 and 2 are NaN and fail; it never blocks; cell 3 passes
                  [50.0, 5.0, 20.0, 20.0],     # under the ground at 1 (blocked at 1): merely low at cell 1, blocked for cells 2 and 3
                  [50.0, 40.0, 30.0, 5.0],     # arrives at 1 and 2, low at 3 (blocked at 3: no cell asks)
                  [50.0, 40.0, 30.0, 30.0]])
    r = vm.scan(H, T, 0.0)
    assert r["k_star"].tolist() == [2, 2, 3] and r["status"].tolist() == [sm.SEEN, sm.HIDDEN, sm.SEEN] and r["block_index"].tolist() == [-1, 1, -1]
    assert r["hidden"].tolist() == [30.0, 20.0, 20.0] and r["ground"].tolist() == [10.0, 10.0, 10.0]
    r = vm.scan(H[:2], T, 100.0)
    assert r["k_star"].tolist() == [2, 2, 2] and (r["status"] == sm.ABOVE_FAN).all() and np.isnan(r["hidden"]).all() and (r["block_index"] == -1).all()
    r = vm.scan(H[3:], T, 0.0)
    assert r["k_star"].tolist() == [0, 0, 0] and (r["status"] == sm.BELOW_FAN).all() and r["hidden"].tolist() == [30.0, 20.0, 20.0]
    assert vm.fan_angles(-5.0, 5.0, 64).tobytes() == sm.fan_angles(-5.0, 5.0).tobytes() and math.isclose(vm.fan_angles(0.0, 1.0, 128)[-1], 1.0)
