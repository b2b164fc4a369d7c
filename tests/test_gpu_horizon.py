"""atmrt_horizon on the GPU against tests/horizon_model.py (the rule of include/atmrt.h over the oracle's coords_at_dist, get_elev and
ray_paths) and against atmrt_sight_fan_probe on the same context: every field, doubles by their bits.  One synthetic level-1 tile,
frames of 64 x 48 at most, step 100 m.  Every case prints its figures before it asserts (`horizon <case>: ...`)."""
import ctypes as C
import csv
import os
import subprocess
import sys

import numpy as np
import pytest
import yaml

import horizon_model as hm
import polar_plan_model as pm
import sight_model as sm
import viewshed_model as vm
from atm_raytracer_amd import _abi, generators, synth
from atmospheres import WILD_SPLINE, configuration_atmosphere, inversion

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP = 100.0
FAN = (-6.0, 6.0)
_TILES = {}


def scene(w=64, h=48, **over):
    """Scene S2 (one tile, observer 46.5 N 8.5 E, 50 m above the ground, refraction on, step 100 m) with 60 km of range."""
    over.setdefault("max_distance", 60_000.0)
    cfg, tiles = synth.scene("S2", w, h, generator="Fast", **over)
    if not _TILES:
        _TILES.update(tiles)
    return cfg, _TILES


def spline_atmosphere():
    rng = np.random.default_rng(5)
    while True:
        a = configuration_atmosphere(rng)
        if "Spline" in a["first_temperature_function"]:
            return a


def duct():
    cfg, tiles = scene(atmosphere=inversion(vm.DUCT["at"], vm.DUCT["thick"], vm.DUCT["gradient"]))
    cfg.params.position.altitude_kind, cfg.params.position.altitude = _abi.ALT_ABSOLUTE, vm.DUCT["altitude"]
    return cfg, tiles


SETTINGS = {
    "us76": (lambda: scene(), FAN),                                                        # Spherical, US-76
    "flat_straight": (lambda: scene(earth_shape="FlatDistorted", straight_rays=True), FAN),
    "spline": (lambda: scene(atmosphere=spline_atmosphere()), FAN),
    "duct": (duct, vm.DUCT["fan"]),
    "wild": (lambda: scene(atmosphere=WILD_SPLINE), FAN),
}


def configure(ctx, cfg, tiles):
    """The scene's terrain, parameters and atmosphere on the context, without a frame."""
    ctx.check(ctx.lib.atmrt_terrain_clear(ctx.handle))
    terrain = generators.Terrain.from_tiles(tiles, ctx)
    gen = generators.make_generator(generators.Params(cfg), terrain)
    gen._configure()
    return gen


@pytest.fixture(scope="module")
def models(oracle_det):
    """One model setting per scene, made on first use and shared: the oracle's profiles are computed once."""
    made = {}

    def get(name):
        if name not in made:
            cfg, tiles = SETTINGS[name][0]()
            made[name] = (cfg, tiles, sm.Setting(oracle_det, cfg, tiles), SETTINGS[name][1])
        return made[name]

    yield get
    for _, _, s, _ in made.values():
        s.close()


def rays_per_lane(K):
    return generators.horizon_kernel_shape(K)["rays_per_lane"]


def shape():
    s = generators.horizon_kernel_shape(64)
    two = next(K for K in range(64, 4097, 64) if rays_per_lane(K) >= 2)
    return s["az_per_load"], s["step_tile"], two


def fans():
    """viewshed_model.gpu_fan_rays over the horizon's scan: 64, 128, the smallest fan of every variant of the scan kernel, and 4096
    (tests/test_horizon_abi.py asserts that this list reaches every variant)."""
    return vm.gpu_fan_rays(rays_per_lane)


def check(ctx, setting, az_lo, az_step, n_az, reach, fan, K, rounds, tag):
    got = generators.horizon(ctx, az_lo, az_step, n_az, reach, fan, K, rounds)
    want, az, angles = hm.solve(setting, az_lo, az_step, n_az, reach, fan, K, rounds)
    counts = np.bincount(got.records["status"], minlength=4)
    print(f"horizon {tag} n_az={n_az} K={K} reach={reach:g} rounds={rounds}: found/-/above/below {counts.tolist()}, k* {got.records['k_star'].tolist()}, "
          f"block {got.records['block_index'].tolist()}, rounds done {got.records['rounds_done'].tolist()}, {generators.horizon_work(ctx)}")
    assert got.azimuths.tobytes() == az.tobytes() and got.angles.tobytes() == angles.tobytes()
    hm.assert_same(got.records, want, tag)
    return got, counts


@pytest.mark.parametrize("name", ["us76", "flat_straight", "spline", "duct"])
def test_records_equal_the_model(gpu_ctx, models, name):
    """n_az in {1, A + 1} x K in {64, 128, the first K with two rays per lane} x m in {1, tile - 1, tile, tile + 1, 10, 120, 300}, the rounds
    cycling through 1, 2 and 4 (seven sizes per K: every K meets every number of rounds at several m); and every larger fan of fans()
    — the first fan of every further variant of the scan kernel, and 4096 rays: the largest block — at n_az = A + 1 and m in
    {tile - 1, tile + 1, 300}."""
    cfg, tiles, setting, fan = models(name)
    configure(gpu_ctx, cfg, tiles)
    A, tile, two = shape()
    assert two > 128 and two in fans()
    reaches = [(50.0, 1), ((tile - 1) * STEP, tile - 1), (tile * STEP, tile), ((tile + 1) * STEP - 30.0, tile + 1), (1_000.0, 10), (30_000.0, 300), (12_000.0, 120)]
    seen = np.zeros(4, dtype=np.int64)
    n = 0
    for n_az in (1, A + 1):
        for K in (64, 128, two):
            for reach, m in reaches:
                rounds = (1, 2, 4)[n % 3]
                n += 1
                got, counts = check(gpu_ctx, setting, 20.0, 17.5, n_az, reach, fan, K, rounds, name)
                assert got.records.shape == (n_az,) and (got.records["block_index"] <= m).all()
                seen += counts
    larger = [K for K in fans() if K > two]
    assert larger and larger[-1] == 4096 and {rays_per_lane(K) for K in fans()} == {rays_per_lane(K) for K in range(64, 4097, 64)}
    for K in larger:
        for reach, m in (reaches[1], reaches[3], reaches[5]):
            rounds = (1, 2, 4)[n % 3]
            n += 1
            _, counts = check(gpu_ctx, setting, 20.0, 17.5, A + 1, reach, fan, K, rounds, f"{name} rays/lane={rays_per_lane(K)}")
            seen += counts
    assert seen[hm.BELOW_FAN] and (seen[hm.ABOVE_FAN] if name == "duct" else seen[hm.FOUND])  # 50 m out no ray of the fan has met the ground
    if name == "duct":
        # reach 12 km: azimuth 30 is above the fan, azimuth 200 is blocked exactly at i' = m = 120
        for rounds in (1, 2, 4):
            got, _ = check(gpu_ctx, setting, 30.0, 170.0, 2, 12_000.0, fan, 64, rounds, "duct at 12 km")
            assert got.records["status"].tolist() == [hm.ABOVE_FAN, hm.FOUND] and got.records["rounds_done"].tolist() == [1, rounds]
            assert got.records["block_index"][1] == 120 and got.records["block_distance"][1] == 12_000.0
            assert np.isnan(got.records["angle_clear"][0]) and got.records["angle_blocked"][0] == got.angles[63]


def test_wild_atmosphere_the_nan_rule(gpu_ctx, models):
    """atmospheres.WILD_SPLINE, azimuth 90, K = 64, reach 30 km: rays 55 and 63 are NaN at m and not blocked, and 44 rays are blocked
    with clear rays between them: the NaN rule and a pattern that is not monotone.  k* is one above the HIGHEST failing ray."""
    cfg, tiles, setting, fan = models("wild")
    configure(gpu_ctx, cfg, tiles)
    d, m, _, _, T = setting.profile(90.0, 30_000.0)
    H = setting.heights(vm.fan_angles(fan[0], fan[1], 64), m)
    fails, block = hm.trace(H, T)
    by_nan = np.flatnonzero(np.isnan(H[:, m]) & (block < 0)).tolist()
    print(f"horizon wild: failing rays {np.flatnonzero(fails).tolist()}, NaN at m and not blocked {by_nan}, blocked {int((block >= 0).sum())}")
    assert by_nan == [55, 63] and (block >= 0).sum() == 44 and not fails[42:55].any()
    for rounds in (1, 2, 4):
        got, _ = check(gpu_ctx, setting, 90.0, 0.0, 1, 30_000.0, fan, 64, rounds, "wild")
        r = got.records[0]
        assert (r["status"], r["k_star"], r["block_index"], r["rounds_done"]) == (hm.ABOVE_FAN, 64, -1, 1) and np.isnan(r["block_distance"])
    # narrower fans on which the record is FOUND although clear rays lie below the highest failing ray, all rounds run; on the first
    # of them that ray fails by NaN, so that a FOUND record has no ridge
    by_nan_found = 0
    for hi, K, n_az in ((float(vm.fan_angles(fan[0], fan[1], 64)[56]), 64, 1), (5.0, 64, 1), (5.0, 128, 5)):
        f, _ = hm.trace(setting.heights(vm.fan_angles(fan[0], hi, K), m), T)
        k = sm.pick(f)
        print(f"horizon wild fan to {hi:g} K={K}: k* {k}, clear rays below it {int((~f[:k]).sum())}")
        assert 0 < k < K and (~f[:k]).sum() > 10
        got, _ = check(gpu_ctx, setting, 90.0, 0.0, n_az, 30_000.0, (fan[0], hi), K, 3, f"wild, fan to {hi:g}")
        assert (got.records["status"] == hm.FOUND).all() and (got.records["k_star"] == k).all() and (got.records["rounds_done"] == 3).all()
        by_nan_found += int((got.records["block_index"] == -1).sum())
    assert by_nan_found


def test_brackets_equal_the_fan_probe(gpu_ctx):
    """No oracle: the two angles of every record, probed by atmrt_sight_fan_probe against the target one sample beyond the reach —
    whose m is m + 1, so that its block test runs through i = m — give [block_index, -1]."""
    cfg, tiles = scene()
    configure(gpu_ctx, cfg, tiles)
    reach = 30_000.0
    az = (0.0, 86.0, 133.0, 200.0, 270.0)
    for a in az:
        h = generators.horizon(gpu_ctx, a, 0.0, 1, reach, FAN, 128, 3)
        r = h.records[0]
        rays = generators.sight_fan_probe(gpu_ctx, (a, reach + STEP, 0.0), [r["angle_blocked"], r["angle_clear"]])
        print(f"horizon vs probe az={a:g}: k*={r['k_star']} bracket [{r['angle_blocked']:.6f}, {r['angle_clear']:.6f}] ridge at {r['block_distance']:.0f} m; "
              f"probe {rays['block_index'].tolist()}")
        assert r["status"] == hm.FOUND and r["rounds_done"] == 3 and 1 <= r["block_index"] <= 300
        assert rays["block_index"].tolist() == [r["block_index"], -1]
        assert r["block_distance"] == r["block_index"] * STEP and abs((r["angle_clear"] - r["angle_blocked"]) - r["resolution"]) < 1e-12


def timings_hold(work, found):
    """every interval of the call's timing array is a finite time; after a call that found its path table the table's entry is exactly 0"""
    ms = [v for k, v in work.items() if k.endswith("_ms")]
    assert all(np.isfinite(v) and v >= 0.0 for v in ms), work
    if found:
        assert work["paths_ms"] == 0.0 and not work["table_rebuilt"], work


def test_batches_and_determinism(gpu_ctx, monkeypatch):
    cfg, tiles = scene()
    configure(gpu_ctx, cfg, tiles)
    A, tile, _ = shape()
    n_az, m = 2 * A + 1, tile + 1
    args = (0.0, 40.0, n_az, m * STEP, FAN, 128, 3)
    whole = generators.horizon(gpu_ctx, *args)
    assert generators.horizon_work(gpu_ctx)["batches"] == 1
    timings_hold(generators.horizon_work(gpu_ctx), False)
    again = generators.horizon(gpu_ctx, *args)
    timings_hold(generators.horizon_work(gpu_ctx), True)
    assert whole.records.tobytes() == again.records.tobytes()
    # what an azimuth adds to a batch: its profile, 3 x 8 x (m + 1) + 1024 bytes, and its record of 72
    per_az = 3 * 8 * (m + 1) + 1024 + 72
    monkeypatch.setenv("ATMRT_SIGHT_SCRATCH_BYTES", str(4 * per_az))
    split = generators.horizon(gpu_ctx, *args)
    work = generators.horizon_work(gpu_ctx)
    print(f"horizon batches: limit {4 * per_az} bytes: {work}")
    want = pm.batches(pm.uniform(n_az, m, 4 * per_az, pm.HORIZON_STAGED))
    assert 1 < want < n_az and work["batches"] == want
    timings_hold(work, True)
    monkeypatch.setenv("ATMRT_SIGHT_SCRATCH_BYTES", "1")  # a batch holds at least one azimuth
    single = generators.horizon(gpu_ctx, *args)
    assert generators.horizon_work(gpu_ctx)["batches"] == n_az
    timings_hold(generators.horizon_work(gpu_ctx), True)
    assert whole.records.tobytes() == split.records.tobytes() == single.records.tobytes()
    assert (whole.records["status"] == hm.FOUND).all()


def test_path_table_lifetime(gpu_ctx, models):
    """The table is the viewshed's product under the viewshed's key: either call finds what the other built."""
    cfg, tiles, setting, fan = models("us76")
    configure(gpu_ctx, cfg, tiles)
    generators.viewshed(gpu_ctx, 10.0, 5.0, 2, 7_000.0, 0.0, (fan[0], fan[1] + 1.0), 128)  # another fan: whatever an earlier test left is gone
    generators.viewshed(gpu_ctx, 10.0, 5.0, 2, 7_000.0, 0.0, fan, 128)
    first = generators.viewshed_work(gpu_ctx)
    check(gpu_ctx, setting, 300.0, -7.0, 3, 7_000.0, fan, 128, 3, "after a viewshed of the same fan")
    second = generators.horizon_work(gpu_ctx)
    print(f"horizon table: viewshed {first}, then horizon {second}")
    assert first["table_rebuilt"] and not second["table_rebuilt"] and second["paths_ms"] == 0.0
    check(gpu_ctx, setting, 10.0, 5.0, 2, 7_000.0, fan, 192, 2, "another K")
    built = generators.horizon_work(gpu_ctx)
    assert built["table_rebuilt"] and built["paths_ms"] > 0.0
    generators.viewshed(gpu_ctx, 10.0, 5.0, 2, 7_000.0, 25.0, fan, 192)
    assert not generators.viewshed_work(gpu_ctx)["table_rebuilt"]  # the reverse
    for other in (dict(reach=7_100.0), dict(fan=(fan[0], fan[1] + 0.5)), dict(K=128)):
        check(gpu_ctx, setting, 10.0, 5.0, 2, other.get("reach", 7_000.0), other.get("fan", fan), other.get("K", 192), 2, f"other {sorted(other)}")
        assert generators.horizon_work(gpu_ctx)["table_rebuilt"], other
    check(gpu_ctx, setting, 10.0, 5.0, 2, 7_000.0, fan, 128, 4, "other rounds and azimuths only")
    assert not generators.horizon_work(gpu_ctx)["table_rebuilt"]
    # another atmosphere: rebuilt, and the records are the model's again
    cfg2, tiles2, setting2, _ = models("spline")
    configure(gpu_ctx, cfg2, tiles2)
    check(gpu_ctx, setting2, 10.0, 5.0, 2, 7_000.0, fan, 128, 4, "after the atmosphere changed")
    assert generators.horizon_work(gpu_ctx)["table_rebuilt"]
    configure(gpu_ctx, cfg, tiles)
    check(gpu_ctx, setting, 10.0, 5.0, 2, 7_000.0, fan, 128, 4, "and back")
    assert generators.horizon_work(gpu_ctx)["table_rebuilt"]


def test_a_generated_frame_is_not_disturbed(gpu_ctx):
    """The frame a context holds — here one with translucent terrain, so that pixels hold lists — is the same after a call: its
    trace-point lists in HBM field for field, what the visibility map reads from it, and the picture drawn from it."""
    cfg, tiles = scene(64, 48, tilt=-2.0, terrain_alpha=0.6)
    gpu_ctx.check(gpu_ctx.lib.atmrt_terrain_clear(gpu_ctx.handle))
    gen = generators.make_generator(generators.Params(cfg), generators.Terrain.from_tiles(tiles, gpu_ctx))
    res = gen.generate()
    col = generators.into_coloring(gpu_ctx.lib, cfg.params, dict(kind=0, water_level=0.0, ambient_light=0.4, light_zenith_angle=45.0, light_dir=0.0,
                                                               palette=0, has_fog=0, fog_distance=0.0))
    grid = generators.snap_grid(generators.frame_bounds(gpu_ctx, "all"), 30.0 / 3600.0)

    def state():
        hits = {k: v.cpu().numpy() for k, v in gen.last_hits_device(48, 64).items()}
        count, mind, stats = generators.visibility_map(gpu_ctx, grid, "all")
        return hits, dict(count=count, min_distance=mind, bounds=np.array(generators.frame_bounds(gpu_ctx, "all")), image=generators.draw_image(gpu_ctx, col, 64, 48))

    hits0, rest0 = state()
    assert res["n_hits"] > res["hit_count"].astype(bool).sum() > 0 and len(hits0["lat"]) == res["n_hits"]  # lists, and the frame's own
    a = generators.horizon(gpu_ctx, 0.0, 30.0, 6, 20_000.0, FAN, 128, 3)
    b = generators.horizon(gpu_ctx, 0.0, 30.0, 6, 20_000.0, FAN, 4096, 2)
    assert (a.records["status"] == hm.FOUND).all() and (b.records["status"] == hm.FOUND).all()
    hits1, rest1 = state()
    assert set(hits1) == set(hits0)
    for k in hits0:
        assert hits1[k].tobytes() == hits0[k].tobytes(), k
    for k in rest0:
        assert rest1[k].tobytes() == rest0[k].tobytes(), k
    assert rest0["image"].any() and rest0["count"].sum() > 0


def test_device_records_equal_the_host_route(gpu_ctx):
    import torch
    cfg, tiles = scene()
    configure(gpu_ctx, cfg, tiles)
    A, tile, two = shape()
    n_az, reach = A + 2, (tile + 5) * STEP
    dev = torch.device("cuda", gpu_ctx.device)
    for K in [64] + [K for K in fans() if K >= two]:
        for rounds in (1, 3):
            host = generators.horizon(gpu_ctx, 45.0, 3.0, n_az, reach, FAN, K, rounds)
            spec = _abi.HorizonSpec(45.0, 3.0, reach, FAN[0], FAN[1], n_az, K, rounds)
            buf = torch.full((n_az + 1, 72), 77, dtype=torch.uint8, device=dev)
            gpu_ctx.check(gpu_ctx.lib.atmrt_horizon_device(gpu_ctx.handle, C.byref(spec), buf.data_ptr()))
            torch.cuda.synchronize(dev)
            raw = buf.cpu().numpy()
            assert raw[:n_az].tobytes() == host.records.tobytes(), (K, rounds)
            assert (raw[n_az] == 77).all()  # nothing beyond the last record


def test_argument_and_state_errors(gpu_ctx):
    cfg, tiles = scene()
    configure(gpu_ctx, cfg, tiles)
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    good = dict(az_lo_deg=0.0, az_step_deg=1.0, reach=1_000.0, fan_lo_deg=-1.0, fan_hi_deg=1.0, n_az=2, fan_rays=64, rounds=3)
    out = np.zeros(2, dtype=generators.HORIZON_DTYPE)

    def call(fn=lib.atmrt_horizon, handle=h, spec=True, records=True, **over):
        s = _abi.HorizonSpec(**dict(good, **over))
        rc = fn(handle, C.byref(s) if spec else None, out.ctypes.data if records else None)
        return rc, lib.atmrt_last_error(handle).decode()

    assert call()[0] == 0 and call(rounds=1)[0] == 0 and call(rounds=4)[0] == 0
    bad = [dict(spec=False), dict(records=False), dict(az_lo_deg=np.nan), dict(az_step_deg=np.inf), dict(az_lo_deg=1e308, az_step_deg=1e308),
           dict(reach=0.0), dict(reach=-1.0), dict(reach=np.nan), dict(reach=np.inf), dict(reach=65_536 * STEP), dict(n_az=0), dict(n_az=-3), dict(n_az=65_537),
           dict(fan_rays=0), dict(fan_rays=63), dict(fan_rays=96), dict(fan_rays=4160), dict(fan_lo_deg=np.nan), dict(fan_hi_deg=np.inf),
           dict(fan_lo_deg=1.0, fan_hi_deg=1.0), dict(fan_lo_deg=2.0, fan_hi_deg=1.0), dict(fan_lo_deg=-91.0, fan_hi_deg=90.0),
           dict(rounds=0), dict(rounds=5), dict(rounds=-1),
           dict(reach=65_535 * STEP, fan_rays=4096, n_az=1)]  # m in range, but a path table of 65536 * 4096 * 8 bytes
    out[:] = 0
    before = out.tobytes()
    for kw in bad:
        for fn in (lib.atmrt_horizon, lib.atmrt_horizon_device):  # refused before any record is touched
            rc, msg = call(fn=fn, **kw)
            assert rc == _abi.ERR_INVALID_ARGUMENT and msg, (kw, rc, msg)
    assert "exceeds the scratch limit" in call(reach=65_535 * STEP, fan_rays=4096, n_az=1)[1]
    assert "rounds" in call(rounds=5)[1]
    assert before == out.tobytes()
    assert call(fan_lo_deg=-90.0, fan_hi_deg=90.0)[0] == 0  # 180 degrees wide is allowed
    fresh = generators.Context(gpu_ctx.device)
    try:
        rc, msg = call(handle=fresh.handle)
        assert rc == _abi.ERR_STATE and "atmrt_set_params" in msg
        assert call(fn=lib.atmrt_horizon_device, handle=fresh.handle)[0] == _abi.ERR_STATE
    finally:
        fresh.close()
    multi = generators.Context.multi([gpu_ctx.device, gpu_ctx.device])
    try:
        pod = _abi.Params.from_buffer_copy(cfg.params)
        multi.check(lib.atmrt_set_params(multi.handle, C.byref(pod)))
        rc, msg = call(handle=multi.handle)
        assert rc == _abi.ERR_STATE and "multi-device" in msg
    finally:
        multi.close()


def test_gen_horizon(gpu_ctx, tmp_path):
    """`gen --horizon OUT.csv` end to end: the rows are generators.horizon's for the same call, with the options and by default."""
    synth.write_terrain_dir(str(tmp_path / "terrain"), synth.synth_tiles([46], [8], level=301))
    doc = {"scene": {"terrain_folder": "./terrain"},
           "view": {"position": {"latitude": 46.5, "longitude": 8.5, "altitude": {"Relative": 50.0}},
                    "frame": {"direction": 90.0, "fov": 30.0, "tilt": 0.0, "max_distance": 9_000.0}},
           "simulation_step": 100.0, "output": {"width": 48, "height": 32, "generator": "Fast"}}
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(doc))
    r = subprocess.run([sys.executable, "-m", "atm_raytracer_amd", "gen", "-c", "cfg.yaml", "--output", "out.png", "--horizon", "hz.csv", "--horizon-az", "60", "120", "7",
                        "--horizon-reach", "6450", "--horizon-fan", "-4", "3", "128", "--horizon-rounds", "2"], cwd=str(tmp_path),
                       env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    from atm_raytracer_amd import config
    cfg = config.parse_config(str(tmp_path / "cfg.yaml"))
    gpu_ctx.check(gpu_ctx.lib.atmrt_terrain_clear(gpu_ctx.handle))
    terrain = generators.Terrain.from_folder(str(tmp_path / "terrain"), gpu_ctx)
    generators.make_generator(generators.Params(cfg), terrain)._configure()
    want = generators.horizon(gpu_ctx, 60.0, 10.0, 7, 6_450.0, (-4.0, 3.0), 128, 2)
    generators.write_horizon_csv(str(tmp_path / "want.csv"), want)
    got = (tmp_path / "hz.csv").read_text()
    assert got == (tmp_path / "want.csv").read_text()
    rows = list(csv.reader(got.splitlines()))
    assert tuple(rows[0]) == generators.HORIZON_COLUMNS and len(rows) == 8 and [float(x[0]) for x in rows[1:]] == want.azimuths.tolist()
    assert [x[1] for x in rows[1:]] == [_abi.HORIZON_STATUS[int(v)] for v in want.records["status"]] and "found" in [x[1] for x in rows[1:]]
    found = want.records["status"] == hm.FOUND
    assert [float(x[2]) for x, ok in zip(rows[1:], found) if ok] == want.records["angle_clear"][found].tolist()  # repr() round-trips
    assert all(float(x[3]) < float(x[2]) for x, ok in zip(rows[1:], found) if ok) and (want.records["rounds_done"][found] == 2).all()
    from atm_raytracer_amd.__main__ import viewshed_defaults
    lo, step, n, reach = viewshed_defaults(cfg, None, None, "--horizon-az")
    assert (n, reach, step) == (48, 9_000.0, 30.0 / 48) and lo == 90.0 - 0.5 * 30.0
