"""atmrt_viewshed on the GPU against tests/viewshed_model.py (the rule of include/atmrt.h over the oracle's coords_at_dist, get_elev and
ray_paths) and against atmrt_sight_lines on the same context: every plane, doubles by their bits.  One synthetic level-1 tile, frames
of 64 x 48 at most, step 100 m.  Every case prints its figures before it asserts (`viewshed <case>: ...`)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import yaml

import polar_plan_model as pm
import sight_model as sm
import viewshed_model as vm
from atm_raytracer_amd import _abi, generators, synth
from atmospheres import configuration_atmosphere, inversion
from util import run_gpu

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
    return generators.viewshed_kernel_shape(K)["rays_per_lane"]


def shape():
    s = generators.viewshed_kernel_shape(64)
    two = next(K for K in range(64, 4097, 64) if rays_per_lane(K) >= 2)
    return s["az_per_load"], s["step_tile"], two


def fans():
    """viewshed_model.gpu_fan_rays: 64, 128, the smallest fan of every variant of the scan kernel, and 4096 (tests/test_viewshed_abi.py
    asserts that this list reaches every variant)."""
    return vm.gpu_fan_rays(rays_per_lane)


def check(ctx, setting, az_lo, az_step, n_az, reach, height, fan, K, tag):
    got = generators.viewshed(ctx, az_lo, az_step, n_az, reach, height, fan, K)
    want = vm.solve(setting, az_lo, az_step, n_az, reach, height, fan, K)
    counts = np.bincount(got.status.ravel(), minlength=4).tolist()
    print(f"viewshed {tag} n_az={n_az} K={K} m={got.d.size - 1} height={height:g}: seen/hidden/above/below {counts}, {generators.viewshed_work(ctx)}")
    assert got.d.tobytes() == want["d"].tobytes() and got.azimuths.tobytes() == want["azimuths"].tobytes() and got.angles.tobytes() == want["angles"].tobytes()
    vm.assert_same(got, want, tag)
    return got, counts


@pytest.mark.parametrize("name", sorted(SETTINGS))
def test_scan_equals_the_model(gpu_ctx, models, name):
    """n_az in {1, A + 1} x K in {64, 128, the first K with two rays per lane} x m in {1, tile - 1, tile, tile + 1} and reaches of 1 and
    30 km; and every larger fan of fans() — the first fan of every further variant of the scan kernel, and 4096 rays: the largest
    block and all of its LDS — at n_az = A + 1 and m in {tile - 1, tile + 1}."""
    cfg, tiles, setting, fan = models(name)
    configure(gpu_ctx, cfg, tiles)
    A, tile, two = shape()
    assert two > 128 and two in fans()
    reaches = [(50.0, 1), ((tile - 1) * STEP, tile - 1), (tile * STEP, tile), ((tile + 1) * STEP - 30.0, tile + 1), (1_000.0, 10), (30_000.0, 300)]
    seen = np.zeros(4, dtype=np.int64)
    n = 0
    for n_az in (1, A + 1):
        for K in (64, 128, two):
            for reach, m in reaches:
                height = (0.0, 25.0)[n % 2]
                n += 1
                got, counts = check(gpu_ctx, setting, 20.0, 17.5, n_az, reach, height, fan, K, name)
                assert got.k_star.shape == (n_az, m)
                seen += counts
    larger = [K for K in fans() if K > two]
    assert larger and larger[-1] == 4096 and {rays_per_lane(K) for K in fans()} == {rays_per_lane(K) for K in range(64, 4097, 64)}
    for K in larger:
        for reach, m in (reaches[1], reaches[3]):
            height = (0.0, 25.0)[n % 2]
            n += 1
            got, counts = check(gpu_ctx, setting, 20.0, 17.5, A + 1, reach, height, fan, K, f"{name} rays/lane={rays_per_lane(K)}")
            assert got.k_star.shape == (A + 1, m)
    assert seen[sm.SEEN] and seen[sm.HIDDEN]
    if name == "duct":
        H = setting.heights(vm.fan_angles(fan[0], fan[1], 64), 300)
        crossings = int((np.diff(H, axis=0) < 0.0).sum())
        print(f"viewshed duct: {crossings} places where a ray lies below the ray under it")
        assert crossings > 0


RIDGE = dict(az_lo=86.0, az_step=2.0, n_az=5, reach=40_000.0, fan=(-5.0, 2.0))


def test_scan_equals_the_sight_lines(gpu_ctx):
    """K = 64 on the ridge scene: every cell is what atmrt_sight_lines(rounds = 1) returns for {az_j, d_i, height}.  No oracle."""
    cfg, tiles = scene()
    configure(gpu_ctx, cfg, tiles)
    total = np.zeros(4, dtype=np.int64)
    for height in (0.0, 150.0):
        v = generators.viewshed(gpu_ctx, RIDGE["az_lo"], RIDGE["az_step"], RIDGE["n_az"], RIDGE["reach"], height, RIDGE["fan"], 64)
        n_az, m = v.k_star.shape
        targets = np.empty((n_az, m), dtype=generators.SIGHT_TARGET_DTYPE)
        targets["azimuth_deg"], targets["distance"], targets["height"] = v.azimuths[:, None], v.d[None, 1:], height
        s = generators.sight_lines(gpu_ctx, targets.ravel(), RIDGE["fan"], 1).reshape(n_az, m)
        counts = np.bincount(v.status.ravel(), minlength=4)
        total += counts
        print(f"viewshed vs sight lines height={height:g}: {n_az} x {m} cells, seen/hidden/above/below {counts.tolist()}")
        assert (s["m"] == np.arange(1, m + 1)[None, :]).all() and (s["rounds_done"] == 1).all()
        assert np.array_equal(v.status, s["status"]) and np.array_equal(v.block_index, s["block_index"])
        angle = np.where(v.k_star == 64, np.nan, v.angles[np.minimum(v.k_star, 63)])
        for name, got in (("angle", angle), ("hidden", v.hidden), ("ground", v.ground)):
            g, w = np.ascontiguousarray(got).view(np.uint64).copy(), np.ascontiguousarray(s[name]).view(np.uint64).copy()
            g[np.isnan(got)] = w[np.isnan(s[name])] = 0
            assert np.array_equal(g, w), (name, np.argwhere(g != w)[:5].tolist())
        hid = v.status == sm.HIDDEN
        assert np.array_equal(v.lat[np.nonzero(hid)[0], v.block_index[hid] - 1], s["block_lat"][hid])  # the blocking sample lies on the same lattice
        assert (v.hidden.view(np.uint64)[v.status == sm.ABOVE_FAN] == 0x7FF8000000000000).all()
    assert (total > 0).all(), "the scene must hold all four statuses"


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
    args = (0.0, 40.0, n_az, m * STEP, 10.0, FAN, 128)
    whole = generators.viewshed(gpu_ctx, *args)
    assert generators.viewshed_work(gpu_ctx)["batches"] == 1
    timings_hold(generators.viewshed_work(gpu_ctx), False)
    again = generators.viewshed(gpu_ctx, *args)
    timings_hold(generators.viewshed_work(gpu_ctx), True)
    for k, a in whole.planes().items():
        assert a.tobytes() == getattr(again, k).tobytes(), k
    # a limit that holds a few azimuths of this call, not all nine (one adds some 5 kB: its profile and its cells of the seven planes)
    monkeypatch.setenv("ATMRT_SIGHT_SCRATCH_BYTES", "20000")
    split = generators.viewshed(gpu_ctx, *args)
    work = generators.viewshed_work(gpu_ctx)
    print(f"viewshed batches: limit 20000 bytes: {work}")
    want = pm.batches(pm.uniform(n_az, m, 20000, pm.viewshed_staged(m)))
    assert 1 < want < n_az and work["batches"] == want
    timings_hold(work, True)
    monkeypatch.setenv("ATMRT_SIGHT_SCRATCH_BYTES", "1")  # a batch holds at least one azimuth
    single = generators.viewshed(gpu_ctx, *args)
    assert generators.viewshed_work(gpu_ctx)["batches"] == n_az == pm.batches(pm.uniform(n_az, m, 1, pm.viewshed_staged(m)))
    timings_hold(generators.viewshed_work(gpu_ctx), True)
    for k, a in whole.planes().items():
        assert a.tobytes() == getattr(split, k).tobytes() == getattr(single, k).tobytes(), k


def test_path_table_lifetime(gpu_ctx, models):
    cfg, tiles, setting, fan = models("us76")
    configure(gpu_ctx, cfg, tiles)
    generators.viewshed(gpu_ctx, 10.0, 5.0, 2, 7_000.0, 0.0, fan, 128)
    generators.viewshed(gpu_ctx, 10.0, 5.0, 2, 7_000.0, 0.0, (fan[0], fan[1] + 1.0), 128)
    assert generators.viewshed_work(gpu_ctx)["table_rebuilt"]  # another fan: whatever an earlier test left is gone
    generators.viewshed(gpu_ctx, 10.0, 5.0, 2, 7_000.0, 0.0, fan, 128)
    first = generators.viewshed_work(gpu_ctx)
    check(gpu_ctx, setting, 300.0, -7.0, 3, 7_000.0, 40.0, fan, 128, "other height and azimuths")
    second = generators.viewshed_work(gpu_ctx)
    print(f"viewshed table: first {first}, second {second}")
    assert first["table_rebuilt"] and first["paths_ms"] > 0.0 and not second["table_rebuilt"] and second["paths_ms"] == 0.0
    for other in (dict(reach=7_100.0), dict(K=192)):
        generators.viewshed(gpu_ctx, 10.0, 5.0, 2, other.get("reach", 7_000.0), 0.0, fan, other.get("K", 128))
        assert generators.viewshed_work(gpu_ctx)["table_rebuilt"], other
    generators.viewshed(gpu_ctx, 10.0, 5.0, 2, 7_000.0, 0.0, fan, 128)
    assert generators.viewshed_work(gpu_ctx)["table_rebuilt"]
    # another atmosphere: rebuilt, and the planes are the model's again
    cfg2, tiles2, setting2, fan2 = models("spline")
    configure(gpu_ctx, cfg2, tiles2)
    check(gpu_ctx, setting2, 10.0, 5.0, 2, 7_000.0, 0.0, fan, 128, "after the atmosphere changed")
    assert generators.viewshed_work(gpu_ctx)["table_rebuilt"]
    configure(gpu_ctx, cfg, tiles)
    check(gpu_ctx, setting, 10.0, 5.0, 2, 7_000.0, 0.0, fan, 128, "and back")
    assert generators.viewshed_work(gpu_ctx)["table_rebuilt"]


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
    assert {"hit_offset", "lat", "lon", "distance", "elevation", "path_length", "normal"} <= set(hits0)
    generators.viewshed(gpu_ctx, 0.0, 30.0, 6, 20_000.0, 0.0, FAN, 128)
    generators.viewshed(gpu_ctx, 0.0, 30.0, 6, 20_000.0, 0.0, FAN, 4096)
    hits1, rest1 = state()
    assert set(hits1) == set(hits0)
    for k in hits0:
        assert hits1[k].tobytes() == hits0[k].tobytes(), k
    for k in rest0:
        assert rest1[k].tobytes() == rest0[k].tobytes(), k
    assert rest0["image"].any() and rest0["count"].sum() > 0


def test_device_planes_equal_the_host_route(gpu_ctx):
    import torch
    cfg, tiles = scene()
    configure(gpu_ctx, cfg, tiles)
    A, tile, two = shape()
    n_az, reach = A + 2, (tile + 5) * STEP
    dev = torch.device("cuda", gpu_ctx.device)
    kinds = {"k_star": torch.int16, "status": torch.uint8, "hidden": torch.float64, "block_index": torch.int32, "ground": torch.float64, "lat": torch.float64,
             "lon": torch.float64}
    for K in [K for K in fans() if K >= two]:  # one fan of every variant with several rays per lane, and the largest
        host = generators.viewshed(gpu_ctx, 45.0, 3.0, n_az, reach, 5.0, FAN, K)
        m = host.d.size - 1
        spec = _abi.ViewshedSpec(45.0, 3.0, reach, 5.0, FAN[0], FAN[1], n_az, K)
        for skip in ((), ("block_index", "ground", "lat", "lon")):
            planes = {k: torch.full((n_az, m), 77, dtype=t, device=dev) for k, t in kinds.items()}
            gpu_ctx.check(gpu_ctx.lib.atmrt_viewshed_device(gpu_ctx.handle, C.byref(spec), *[None if k in skip else planes[k].data_ptr() for k, _ in vm.PLANES]))
            torch.cuda.synchronize(dev)
            for k, t in vm.PLANES:
                got = planes[k].cpu().numpy().view(t)
                if k in skip:
                    assert (got == 77).all(), (K, k)
                else:
                    assert got.tobytes() == getattr(host, k).tobytes(), (K, k)
    lean = generators.viewshed(gpu_ctx, 45.0, 3.0, n_az, reach, 5.0, FAN, K, optional=())
    assert lean.block_index is None and lean.lat is None and lean.hidden.tobytes() == host.hidden.tobytes() and lean.k_star.tobytes() == host.k_star.tobytes()


def test_argument_and_state_errors(gpu_ctx):
    cfg, tiles = scene()
    configure(gpu_ctx, cfg, tiles)
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    good = dict(az_lo_deg=0.0, az_step_deg=1.0, reach=1_000.0, height=0.0, fan_lo_deg=-1.0, fan_hi_deg=1.0, n_az=2, fan_rays=64)
    planes = {k: np.zeros(2 * 10, dtype=t) for k, t in vm.PLANES}

    def call(fn=lib.atmrt_viewshed, handle=h, spec=True, missing=(), **over):
        s = _abi.ViewshedSpec(**dict(good, **over))
        rc = fn(handle, C.byref(s) if spec else None, *[None if k in missing else planes[k].ctypes.data for k, _ in vm.PLANES])
        return rc, lib.atmrt_last_error(handle).decode()

    assert call()[0] == 0 and call(missing=("block_index", "ground", "lat", "lon"))[0] == 0
    bad = [dict(spec=False), dict(missing=("k_star",)), dict(missing=("status",)), dict(missing=("hidden",)),
           dict(az_lo_deg=np.nan), dict(az_step_deg=np.inf), dict(az_lo_deg=1e308, az_step_deg=1e308), dict(reach=0.0), dict(reach=-1.0), dict(reach=np.nan),
           dict(reach=np.inf), dict(reach=65_536 * STEP), dict(height=-1.0), dict(height=np.nan), dict(n_az=0), dict(n_az=-3), dict(n_az=65_537),
           dict(fan_rays=0), dict(fan_rays=63), dict(fan_rays=96), dict(fan_rays=4160), dict(fan_lo_deg=np.nan), dict(fan_hi_deg=np.inf),
           dict(fan_lo_deg=1.0, fan_hi_deg=1.0), dict(fan_lo_deg=2.0, fan_hi_deg=1.0), dict(fan_lo_deg=-91.0, fan_hi_deg=90.0),
           dict(reach=65_535 * STEP, fan_rays=4096, n_az=1)]  # m in range, but a path table of 65536 * 4096 * 8 bytes
    for kw in bad:
        for fn in (lib.atmrt_viewshed, lib.atmrt_viewshed_device):  # refused before any plane is touched
            rc, msg = call(fn=fn, **kw)
            assert rc == _abi.ERR_INVALID_ARGUMENT and msg, (kw, rc, msg)
    assert "exceeds the scratch limit" in call(reach=65_535 * STEP, fan_rays=4096, n_az=1)[1]
    assert call(fan_lo_deg=-90.0, fan_hi_deg=90.0)[0] == 0  # 180 degrees wide is allowed
    m = C.c_int32()
    assert lib.atmrt_viewshed_steps(h, 65_535 * STEP, C.byref(m)) == 0 and m.value == 65_535
    assert lib.atmrt_viewshed_steps(h, 65_536 * STEP, C.byref(m)) == _abi.ERR_INVALID_ARGUMENT and lib.atmrt_viewshed_steps(h, 1_000.0, None) == _abi.ERR_INVALID_ARGUMENT
    fresh = generators.Context(gpu_ctx.device)
    try:
        rc, msg = call(handle=fresh.handle)
        assert rc == _abi.ERR_STATE and "atmrt_set_params" in msg
        assert call(fn=lib.atmrt_viewshed_device, handle=fresh.handle)[0] == _abi.ERR_STATE
        assert lib.atmrt_viewshed_steps(fresh.handle, 1_000.0, C.byref(m)) == _abi.ERR_STATE
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


def test_gen_viewshed(gpu_ctx, tmp_path):
    """`gen --viewshed OUT.npz` end to end: the arrays equal generators.viewshed for the same call, with the options and by default."""
    synth.write_terrain_dir(str(tmp_path / "terrain"), synth.synth_tiles([46], [8], level=301))
    doc = {"scene": {"terrain_folder": "./terrain"},
           "view": {"position": {"latitude": 46.5, "longitude": 8.5, "altitude": {"Relative": 50.0}},
                    "frame": {"direction": 90.0, "fov": 30.0, "tilt": 0.0, "max_distance": 9_000.0}},
           "simulation_step": 100.0, "output": {"width": 48, "height": 32, "generator": "Fast"}}
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(doc))
    r = subprocess.run([sys.executable, "-m", "atm_raytracer_amd", "gen", "-c", "cfg.yaml", "--output", "out.png", "--viewshed", "vs.npz", "--viewshed-az", "60", "120", "7",
                        "--viewshed-reach", "6450", "--viewshed-height", "12.5", "--viewshed-fan", "-4", "3", "128"], cwd=str(tmp_path),
                       env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    from atm_raytracer_amd import config
    cfg = config.parse_config(str(tmp_path / "cfg.yaml"))
    gpu_ctx.check(gpu_ctx.lib.atmrt_terrain_clear(gpu_ctx.handle))
    terrain = generators.Terrain.from_folder(str(tmp_path / "terrain"), gpu_ctx)
    generators.make_generator(generators.Params(cfg), terrain)._configure()
    want = generators.viewshed(gpu_ctx, 60.0, 10.0, 7, 6_450.0, 12.5, (-4.0, 3.0), 128)
    with np.load(tmp_path / "vs.npz") as z:
        assert set(z.files) == {"k_star", "status", "hidden", "block_index", "ground", "lat", "lon", "d", "azimuths", "angles", "height"}
        assert z["k_star"].shape == (7, 65) and float(z["height"]) == 12.5
        for k in ("d", "azimuths", "angles") + tuple(k for k, _ in vm.PLANES):
            assert z[k].dtype == getattr(want, k).dtype and z[k].tobytes() == getattr(want, k).tobytes(), k
    from atm_raytracer_amd.__main__ import viewshed_defaults
    lo, step, n, reach = viewshed_defaults(cfg, None, None)
    assert (n, reach, step) == (48, 9_000.0, 30.0 / 48) and lo == 90.0 - 0.5 * 30.0
