"""atmrt_sky_rays, atmrt_sky_directions* and atmrt_sky_bodies* on the GPU against tests/sky_model.py (the rule of include/atmrt.h,
"sky rays", over the oracle's ray stepper): status, steps, the counts and the bits of the true elevation byte for byte, all NaNs as
one value; the body plane and the drawn image byte for byte.  The frames and lists are tests/sky_cases.py's (sky step 1000 m, top
100 km, m = 1500); tests/test_sky_model.py asserts without a GPU what each of them holds.  Every case prints its figures before it
asserts (`sky <case>: ...`)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import sky_cases as sc
import sky_model as sm
from atm_raytracer_amd import _abi, generators
from util import bits, run_gpu

pytestmark = pytest.mark.gpu

SPEC = dict(step=sc.STEP, top=sc.TOP, floor=sc.FLOOR, m=sc.M)
SIMPLE = dict(kind=0, water_level=300.0, ambient_light=0.3, light_zenith_angle=88.0, light_dir=190.0, palette=1, has_fog=0, fog_distance=30_000.0)
SUN_RGB = (255, 236, 170)


def assert_planes(got, want, tag):
    for k in ("status", "steps", "true_elevation"):
        g, w = bits(getattr(got, k)), bits(getattr(want, k))
        bad = np.flatnonzero(g.ravel() != w.ravel())
        assert g.dtype == w.dtype and bad.size == 0, f"{tag} {k}: {bad.size} of {g.size} differ, first at {bad[:5]}: {getattr(got, k).ravel()[bad[:5]]} vs {getattr(want, k).ravel()[bad[:5]]}"
    assert got.stats == want.stats, (tag, got.stats, want.stats)


@pytest.fixture(scope="module")
def sphere(oracle_det):
    cfg, _ = sc.FRAMES["rect"]()
    return cfg, sm.Setting.of_config(oracle_det, cfg)


@pytest.fixture(scope="module")
def frames(oracle_det):
    """The model's answer per frame, computed once from the frame the GPU generated and shared by the tests below."""
    made = {}

    def get(ctx, name):
        cfg, tiles = sc.FRAMES[name]()
        res = run_gpu(ctx, cfg, tiles)  # leaves the frame and its setting on the context
        if name not in made:
            made[name] = sm.frame(sm.Setting.of_config(oracle_det, cfg), res, sc.H0, sc.STEP, sc.TOP, sc.FLOOR, sc.M)
        return cfg, res, made[name]

    return get


@pytest.mark.parametrize("n", sc.LIST_LENGTHS)
def test_list_call_equals_the_model(gpu_ctx, sphere, n):
    cfg, setting = sphere
    generators.make_generator(generators.Params(cfg), generators.Terrain.from_tiles({}, gpu_ctx))._configure()
    for tag, elev, m in (("long", sc.list_elevations(n), sc.M), ("short", sc.list_elevations_short(n), sc.SHORT_M)):
        want = sm.rays(setting, sc.LIST_H0, elev, sc.STEP, sc.TOP, sc.FLOOR, m)
        rec = np.zeros(n + 2, dtype=generators.SKY_RAY_DTYPE)
        rec.view(np.uint8)[:] = 0x77  # pre-filled, and two records of guard behind the list
        st = _abi.SkyStats(*[77] * 6)
        spec = generators.sky_spec(sc.STEP, sc.TOP, sc.FLOOR, m)
        e = np.ascontiguousarray(elev, dtype=np.float64)
        gpu_ctx.check(gpu_ctx.lib.atmrt_sky_rays(gpu_ctx.handle, C.byref(spec), sc.LIST_H0, n, e.ctypes.data, rec.ctypes.data, C.byref(st)))
        got = sm.Result()
        got.status, got.steps, got.true_elevation = rec["status"][:n].astype(np.uint8), rec["steps"][:n].copy(), rec["true_elevation"][:n].copy()
        got.stats = generators._sky_stats(st)
        print(f"sky list {tag} n={n}: {got.stats} {generators.sky_timings(gpu_ctx)}")
        assert (rec.view(np.uint8)[16 * n:] == 0x77).all()
        assert_planes(got, want, f"list {tag} {n}")
        if n >= 63 and tag == "short":
            assert {sm.GROUND, sm.EXIT, sm.INSIDE} <= set(got.status[:63].tolist())  # inside one wavefront


@pytest.mark.parametrize("name", sorted(sc.FRAMES))
def test_frame_equals_the_model(gpu_ctx, frames, monkeypatch, name):
    cfg, res, want = frames(gpu_ctx, name)
    W, H = res["width"], res["height"]
    coloring = generators.into_coloring(gpu_ctx.lib, cfg.params, SIMPLE)
    before = generators.draw_image(gpu_ctx, coloring, W, H)
    if name in sc.US76_SPHERE:  # on the model first, so that a kernel cannot hide rays there
        assert want.stats["lost"] == 0 and want.stats["inside"] == 0
    got = generators.sky_directions(gpu_ctx, W, H, **SPEC)
    t = generators.sky_timings(gpu_ctx)
    print(f"sky {name}: {W}x{H} stats={got.stats} compact {t['compact_ms']:.3f} march {t['march_ms']:.3f} download {t['download_ms']:.3f} ms")
    assert_planes(got, want, name)
    assert sum(got.stats[k] for k in ("none", "exit", "ground", "inside", "lost")) == W * H
    if name in sc.US76_SPHERE:
        assert got.stats["lost"] == 0 and got.stats["inside"] == 0
    if name == "no_sky":
        assert got.stats == dict(none=W * H, exit=0, ground=0, inside=0, lost=0, integrated_steps=0) and not got.status.any()
    if name == "all_sky":
        assert got.stats["none"] == 0 and (got.status == sm.EXIT).all()
    # two equal calls: the same bytes; without the steps plane: the same planes; the other list order: the same bytes
    again = generators.sky_directions(gpu_ctx, W, H, **SPEC)
    assert_planes(again, got, name + " again")
    alone = generators.sky_directions(gpu_ctx, W, H, steps=False, **SPEC)
    assert alone.steps is None and bits(alone.true_elevation).tobytes() == bits(got.true_elevation).tobytes() and alone.status.tobytes() == got.status.tobytes()
    monkeypatch.setenv("ATMRT_SKY_ORDER", "forward")
    forward = generators.sky_directions(gpu_ctx, W, H, **SPEC)
    monkeypatch.delenv("ATMRT_SKY_ORDER")
    assert_planes(forward, got, name + " forward")
    # the frame is intact
    assert generators.draw_image(gpu_ctx, coloring, W, H).tobytes() == before.tobytes()


def test_device_and_planes_entry_points(gpu_ctx, frames, oracle_det):
    """atmrt_sky_directions_device, and atmrt_sky_directions_planes_device over the frame's own planes uploaded again with its h0:
    the bytes and counts of atmrt_sky_directions.  Then hand-made planes: an empty list, one sky pixel in the last lane of the last
    block, and launch elevations of NaN and 90 (both LOST at step 0)."""
    cfg, res, want = frames(gpu_ctx, "rect")
    W, H = res["width"], res["height"]
    lib, spec = gpu_ctx.lib, generators.sky_spec(**SPEC)

    def planes_call(hit_count, elevation, h0):
        n = hit_count.size
        d_hit = torch.from_numpy(np.ascontiguousarray(hit_count, dtype=np.uint32).view(np.int32).ravel()).cuda()
        d_el = torch.from_numpy(np.ascontiguousarray(elevation, dtype=np.float64).ravel()).cuda()
        d_true = torch.full((n + 8,), 77.0, dtype=torch.float64, device="cuda")
        d_status = torch.full((n + 8,), 77, dtype=torch.uint8, device="cuda")
        d_steps = torch.full((n + 8,), 77, dtype=torch.int32, device="cuda")
        st = _abi.SkyStats()
        torch.cuda.synchronize()  # the fills above run on torch's stream, the library on its own
        gpu_ctx.check(lib.atmrt_sky_directions_planes_device(gpu_ctx.handle, C.byref(spec), h0, n, d_hit.data_ptr(), d_el.data_ptr(),
                                                             d_true.data_ptr(), d_status.data_ptr(), d_steps.data_ptr(), C.byref(st)))
        torch.cuda.synchronize()
        assert (d_true[n:] == 77.0).all() and (d_status[n:] == 77).all() and (d_steps[n:] == 77).all()  # nothing behind the planes
        got = sm.Result()
        got.true_elevation, got.status = d_true[:n].cpu().numpy(), d_status[:n].cpu().numpy()
        got.steps, got.stats = d_steps[:n].cpu().numpy().view(np.uint32), generators._sky_stats(st)
        return got

    d_true = torch.full((H, W), 77.0, dtype=torch.float64, device="cuda")
    d_status = torch.full((H, W), 77, dtype=torch.uint8, device="cuda")
    d_steps = torch.full((H, W), 77, dtype=torch.int32, device="cuda")
    st = _abi.SkyStats()
    torch.cuda.synchronize()
    gpu_ctx.check(lib.atmrt_sky_directions_device(gpu_ctx.handle, C.byref(spec), d_true.data_ptr(), d_status.data_ptr(), d_steps.data_ptr(), C.byref(st)))
    dev = sm.Result()
    dev.true_elevation, dev.status, dev.steps = d_true.cpu().numpy(), d_status.cpu().numpy(), d_steps.cpu().numpy().view(np.uint32)
    dev.stats = generators._sky_stats(st)
    assert_planes(dev, want, "device")
    got = planes_call(res["hit_count"], res["elevation_angle"], sc.H0)
    want_flat = sm.Result()
    want_flat.true_elevation, want_flat.status, want_flat.steps, want_flat.stats = want.true_elevation.ravel(), want.status.ravel(), want.steps.ravel(), want.stats
    assert_planes(got, want_flat, "planes")

    setting = sm.Setting.of_config(oracle_det, cfg)
    n = 512  # two blocks of the compaction, eight wavefronts
    elevation = np.linspace(-1.0, 30.0, n)
    for tag, hit in (("empty list", np.ones(n, dtype=np.uint32)), ("last lane", np.ones(n, dtype=np.uint32)), ("mixed", (np.arange(n) % 3 == 0).astype(np.uint32))):
        el = elevation.copy()
        if tag == "last lane":
            hit[n - 1] = 0
        if tag == "mixed":
            el[1], el[2], el[4], el[n - 1] = math.nan, 90.0, -90.0, 123.0  # sky pixels: LOST at step 0
        got = planes_call(hit, el, sc.LIST_H0)
        want_h = sm.rays(setting, sc.LIST_H0, el, sc.STEP, sc.TOP, sc.FLOOR, sc.M, sky=hit == 0)
        print(f"sky planes {tag}: {got.stats}")
        assert_planes(got, want_h, tag)
        if tag == "empty list":
            assert got.stats == dict(none=n, exit=0, ground=0, inside=0, lost=0, integrated_steps=0)
        if tag == "last lane":
            assert got.stats["none"] == n - 1 and got.status[n - 1] == sm.EXIT
        if tag == "mixed":
            assert got.stats["lost"] == 4 and [int(got.steps[i]) for i in (1, 2, 4, n - 1)] == [0] * 4


def test_bodies_equal_the_model(gpu_ctx, frames):
    cfg, res, want = frames(gpu_ctx, "rect")
    W, H = res["width"], res["height"]
    coloring = generators.into_coloring(gpu_ctx.lib, cfg.params, SIMPLE)
    plain = generators.draw_image(gpu_ctx, coloring, W, H)
    sky = generators.sky_directions(gpu_ctx, W, H, **SPEC)
    # the frame's centre sky pixel: the middle column, the middle one of its sky rows
    x = W // 2
    rows = np.flatnonzero(sky.status[:, x] == sm.EXIT)
    y = int(rows[len(rows) // 2])
    sun = (float(res["azimuth"][y, x]), float(sky.true_elevation[y, x]), 0.2666, SUN_RGB)
    moon = (sun[0] + 0.3, sun[1] + 0.1, 0.2666, (200, 200, 220))  # overlaps the sun: the first body wins
    # the moon's centre lies 0.32 degrees from the sun's: the centre pixel is the sun's alone, whichever comes first
    for tag, bodies, centre in (("sun", [sun], 1), ("sun and moon", [sun, moon], 1), ("moon and sun", [moon, sun], 2)):
        want_body = sm.body_plane(bodies, res["azimuth"], want.true_elevation, want.status)
        image = plain.copy()
        body = generators.sky_bodies(gpu_ctx, sky, bodies, image)
        print(f"sky bodies {tag}: centre pixel ({y}, {x}) az {sun[0]:.4f} true elevation {sun[1]:.4f}, body pixels {np.bincount(body.ravel()).tolist()}")
        assert body.dtype == np.uint8 and body.tobytes() == want_body.tobytes()
        assert body[y, x] == centre
        assert image.tobytes() == sm.draw(plain, want_body, bodies).tobytes()
        changed = (image != plain).any(axis=2)
        assert (changed <= (body != 0)).all()  # nothing outside the body pixels
        assert (image[body != 0] == np.array([bodies[k - 1][3] for k in body[body != 0]], dtype=np.uint8)).all()
        assert (body != 0).sum() >= 1 and ((body != 0) <= (sky.status == sm.EXIT)).all()
        # draw_image(bodies=) is the same image; the plane alone leaves no image behind
        assert generators.draw_image(gpu_ctx, coloring, W, H, bodies=bodies, sky=sky).tobytes() == image.tobytes()
        assert generators.sky_bodies(gpu_ctx, sky, bodies).tobytes() == body.tobytes()
    # the device entry point over device planes
    d_true = torch.from_numpy(sky.true_elevation).cuda()
    d_status = torch.from_numpy(sky.status).cuda()
    d_body = torch.full((H, W), 77, dtype=torch.uint8, device="cuda")
    d_rgb = torch.from_numpy(plain.copy()).cuda()
    arr, n = generators._sky_bodies_array([sun, moon])
    torch.cuda.synchronize()
    gpu_ctx.check(gpu_ctx.lib.atmrt_sky_bodies_device(gpu_ctx.handle, arr, n, d_true.data_ptr(), d_status.data_ptr(), d_body.data_ptr(), d_rgb.data_ptr()))
    want_body = sm.body_plane([sun, moon], res["azimuth"], want.true_elevation, want.status)
    assert d_body.cpu().numpy().tobytes() == want_body.tobytes() and d_rgb.cpu().numpy().tobytes() == sm.draw(plain, want_body, [sun, moon]).tobytes()
    d_az = torch.from_numpy(np.ascontiguousarray(res["azimuth"])).cuda()
    d_body.fill_(77)
    torch.cuda.synchronize()
    gpu_ctx.check(gpu_ctx.lib.atmrt_sky_bodies_planes_device(gpu_ctx.handle, arr, n, W * H, d_az.data_ptr(), d_true.data_ptr(), d_status.data_ptr(),
                                                             d_body.data_ptr(), None))
    assert d_body.cpu().numpy().tobytes() == want_body.tobytes()


def test_the_lifted_sun(gpu_ctx, oracle_det):
    """A sun whose whole disc lies below the astronomical horizon (true elevation -0.3 degrees) over an all-sky frame from 1000 m:
    refraction lifts it — the model shows part of the frame in it, at launch elevations above 0, and so does the device.  Then the
    body planes at a sky step of 100 m and of 1000 m side by side: a record of what the cheap step costs, nothing asserted."""
    cfg, tiles = sc.lifted_frame()
    res = run_gpu(gpu_ctx, cfg, tiles)
    W, H = res["width"], res["height"]
    setting = sm.Setting.of_config(oracle_det, cfg)
    want = sm.frame(setting, res, sc.LIFTED_H0, sc.STEP, sc.TOP, sc.FLOOR, sc.M)
    assert want.stats["exit"] == W * H  # all sky, on the model first
    want_body = sm.body_plane([sc.LIFTED_SUN], res["azimuth"], want.true_elevation, want.status)
    inside = want_body == 1
    assert 0 < inside.sum() < W * H and (res["elevation_angle"][inside] > 0.0).any() and (want.true_elevation[inside] < 0.0).all()
    sky = generators.sky_directions(gpu_ctx, W, H, **SPEC)
    assert_planes(sky, want, "lifted")
    body = generators.sky_bodies(gpu_ctx, sky, [sc.LIFTED_SUN])
    print(f"sky lifted sun: {int(inside.sum())} body pixels, launch elevations {res['elevation_angle'][inside].min():.3f} .. {res['elevation_angle'][inside].max():.3f}, "
          f"true {want.true_elevation[inside].min():.3f} .. {want.true_elevation[inside].max():.3f}")
    assert body.tobytes() == want_body.tobytes()
    fine = generators.sky_directions(gpu_ctx, W, H, step=100.0, top=sc.TOP, floor=sc.FLOOR, m=15 * sc.M)
    body_fine = generators.sky_bodies(gpu_ctx, fine, [sc.LIFTED_SUN])
    print(f"sky step 100 m | 1000 m: {int((body_fine != body).sum())} of {W * H} body pixels differ, "
          f"largest true-elevation difference {np.nanmax(np.abs(fine.true_elevation - sky.true_elevation)):.3g} degrees")
    for a, b in zip(body_fine, body):
        print("".join(".#"[v] for v in a), "|", "".join(".#"[v] for v in b))


def test_refusals_that_need_a_context(gpu_ctx, frames):
    cfg, res, _ = frames(gpu_ctx, "rect")
    W, H = res["width"], res["height"]
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    bad, state = _abi.ERR_INVALID_ARGUMENT, _abi.ERR_STATE
    good = generators.sky_spec(**SPEC)
    true, status, steps, body = np.zeros((H, W)), np.zeros((H, W), dtype=np.uint8), np.zeros((H, W), dtype=np.uint32), np.zeros((H, W), dtype=np.uint8)
    e, rec = np.zeros(4), np.zeros(4, dtype=generators.SKY_RAY_DTYPE)
    one = (_abi.SkyBody * 1)(generators.sky_body(100.0, 3.0))

    def calls(handle, spec):
        return (lib.atmrt_sky_rays(handle, C.byref(spec), 1000.0, 4, e.ctypes.data, rec.ctypes.data, None),
                lib.atmrt_sky_directions(handle, C.byref(spec), true.ctypes.data, status.ctypes.data, steps.ctypes.data, None))

    assert calls(h, good) == (0, 0)
    for step, top, floor, m in ((-1.0, 1e5, 0.0, 1500), (math.nan, 1e5, 0.0, 1500), (1000.0, math.inf, 0.0, 1500), (1000.0, 1e5, 1e5, 1500),
                                (1000.0, 1e5, 0.0, 0), (1000.0, 1e5, 0.0, 1048576)):
        assert calls(h, generators.sky_spec(step, top, floor, m)) == (bad, bad), (step, top, floor, m)
    assert lib.atmrt_sky_rays(h, None, 1000.0, 4, e.ctypes.data, rec.ctypes.data, None) == bad
    assert lib.atmrt_sky_rays(h, C.byref(good), math.nan, 4, e.ctypes.data, rec.ctypes.data, None) == bad
    assert lib.atmrt_sky_rays(h, C.byref(good), 1000.0, 4, None, rec.ctypes.data, None) == bad
    assert lib.atmrt_sky_rays(h, C.byref(good), 1000.0, 4, e.ctypes.data, None, None) == bad
    assert lib.atmrt_sky_directions(h, C.byref(good), None, status.ctypes.data, None, None) == bad
    assert lib.atmrt_sky_directions(h, C.byref(good), true.ctypes.data, None, None, None) == bad
    assert lib.atmrt_sky_bodies(h, one, 1, true.ctypes.data, status.ctypes.data, None, None) == bad
    assert lib.atmrt_sky_bodies(h, None, 1, true.ctypes.data, status.ctypes.data, body.ctypes.data, None) == bad
    many = (_abi.SkyBody * 33)(*[generators.sky_body(100.0, 3.0)] * 33)
    assert lib.atmrt_sky_bodies(h, many, 33, true.ctypes.data, status.ctypes.data, body.ctypes.data, None) == bad
    wide = (_abi.SkyBody * 1)(generators.sky_body(100.0, 3.0, 90.0))
    assert lib.atmrt_sky_bodies(h, wide, 1, true.ctypes.data, status.ctypes.data, body.ctypes.data, None) == bad
    assert lib.atmrt_last_sky_timings(h, None) == bad
    # step 0 takes the context's simulation_step
    rec0, _ = generators.sky_rays(gpu_ctx, 1000.0, [0.0, 5.0], step=0.0, top=sc.TOP, floor=sc.FLOOR, m=20000)
    rec1, _ = generators.sky_rays(gpu_ctx, 1000.0, [0.0, 5.0], step=cfg.params.simulation_step, top=sc.TOP, floor=sc.FLOOR, m=20000)
    assert rec0.tobytes() == rec1.tobytes() and (rec0["status"] == sm.EXIT).all()
    # no parameters, then parameters and no frame
    fresh = generators.Context(gpu_ctx.device)
    try:
        assert calls(fresh.handle, good) == (state, state) and b"atmrt_set_params" in lib.atmrt_last_error(fresh.handle)
        generators.make_generator(generators.Params(cfg), generators.Terrain.from_tiles({}, fresh))._configure()
        rc = calls(fresh.handle, good)
        assert rc == (0, state) and b"needs a frame" in lib.atmrt_last_error(fresh.handle)
        assert lib.atmrt_sky_bodies(fresh.handle, one, 1, true.ctypes.data, status.ctypes.data, body.ctypes.data, None) == state
    finally:
        fresh.close()
    multi = generators.Context.multi([gpu_ctx.device, gpu_ctx.device])
    try:
        generators.make_generator(generators.Params(cfg), generators.Terrain.from_tiles({}, multi))._configure()
        assert lib.atmrt_sky_directions(multi.handle, C.byref(good), true.ctypes.data, status.ctypes.data, None, None) == state
        assert b"atmrt_sky_directions_planes_device" in lib.atmrt_last_error(multi.handle)
        assert lib.atmrt_sky_bodies(multi.handle, one, 1, true.ctypes.data, status.ctypes.data, body.ctypes.data, None) == state
    finally:
        multi.close()
