"""atmrt_shadow_lights_true* on the GPU against tests/sky_apparent_model.py's solve_true (the rule of include/atmrt.h,
"apparent elevation": the shadow lights given by their TRUE direction): the mask, every status plane, every block plane byte for
byte and the call's counts over five frames and four lights; the shortcut off against on; the three routes; 1 and 64 lights; a
wavefront that straddles the terminator; the sunset planes, where the same call without the table gives the opposite status at
every point; and atmrt_shadow_lights itself, which returns before and after a true call the bytes it returned before this rule
existed.  The frames and lights are tests/shadow_cases.py's and tests/shadow_lights_cases.py's, the table tests/sky_apparent_cases.py's.
Every case prints its figures before it asserts."""
import ctypes as C

import numpy as np
import pytest
import torch

import shadow_cases as sc
import shadow_lights_cases as slc
import shadow_lights_model as slm
import shadow_model as sm
import shadow_sweep_cases as ssc
import sky_apparent_cases as sac
import sky_apparent_model as sam
import sky_model as skm
from atm_raytracer_amd import _abi, generators
from test_gpu_shadow_lights import Planes, assert_lights, sphere_world
from test_gpu_shadow_sweep import FILL, configure, on_and_off
from util import run_gpu

pytestmark = pytest.mark.gpu

# name -> (the frame of shadow_cases.FRAMES, the sky top of its table, the case is about the shortcut)
FRAMES = {"rect_64x32": (100000.0, True), "fast_50x20": (100000.0, False), "straight": (100000.0, True), "flat_distorted": (100000.0, False),
          "spline": (30000.0, False)}
LIGHTS = [(260.0, 2.0), (260.0, -0.3), slc.NEGATIVE[:2], slc.HIGH[:2]]


def table_model(oracle, cfg, top=100000.0):
    return sam.build(skm.Setting.of_config(oracle, cfg), sac.table_spec(3, 257, top))


@pytest.fixture(scope="module")
def models(oracle_det):
    """Per frame: the lights, the table's model and spec, and solve_true's answer, computed once from the frame the GPU generated."""
    made, settings = {}, {}

    def get(name, cfg, tiles, res):
        if name not in made:
            settings[name] = sm.Setting(oracle_det, cfg, tiles)
            table = table_model(oracle_det, cfg, FRAMES[name][0])
            dirs = slm.lights_from_angles(oracle_det, cfg.params, LIGHTS)
            made[name] = (dirs, table, sac.abi_spec(table.spec), sam.solve_true(settings[name], table, res, dirs, slc.REACH))
        return made[name]

    yield get
    for s in settings.values():
        s.close()


def full_call(ctx, dirs, res, table=None, reach=slc.REACH, lift=0.0):
    return generators.shadow_lights(ctx, dirs, reach, lift, width=res["width"], height=res["height"], status=True, block=True, true_table=table)


class TruePlanes(Planes):
    def lights_true(self, ctx, dirs, table, reach, lift=0.0):
        """atmrt_shadow_lights_true_planes_device into buffers pre-filled with FILL -> ShadowLights."""
        spec, dirs = generators.shadow_lights_spec(dirs, reach, lift)
        n_l = dirs.shape[0]
        d_mask = torch.full((self.n,), FILL, dtype=torch.int64, device="cuda")
        d_status = torch.full((n_l, self.n), FILL, dtype=torch.uint8, device="cuda")
        d_block = torch.full((n_l, self.n), FILL, dtype=torch.int16, device="cuda")
        st = _abi.ShadowStats()
        ctx.check(ctx.lib.atmrt_shadow_lights_true_planes_device(ctx.handle, C.byref(spec), C.byref(table), self.n, self.count.data_ptr(),
                                                                 self.lat.data_ptr(), self.lon.data_ptr(), self.elev.data_ptr(), d_mask.data_ptr(),
                                                                 d_status.data_ptr(), d_block.data_ptr(), C.byref(st)))
        return generators.ShadowLights(d_mask.cpu().numpy().view(np.uint64).reshape(self.shape), d_status.cpu().numpy().reshape((n_l,) + self.shape),
                                       d_block.cpu().numpy().view(np.uint16).reshape((n_l,) + self.shape), generators._shadow_stats(st), dirs)


def check_planes(ctx, setting, table, res, dirs, tag, reach=slc.PLANES_REACH, lift=0.0):
    """The true planes call, shortcut on and off, against the model: mask, planes, counts; a second call: the same bytes."""
    want = sam.solve_true(setting, table, res, dirs, reach, lift)
    spec = sac.abi_spec(table.spec)
    dev = TruePlanes(res)
    on, off = on_and_off(lambda: dev.lights_true(ctx, dirs, spec, reach, lift))
    print(f"shadow true {tag}: m={want.m} floor={want.floor:g} on {on.stats} off {off.stats}")
    assert_lights(on, want, want.stats_on, tag + " on")
    assert_lights(off, want, want.stats_off, tag + " off")
    assert_lights(dev.lights_true(ctx, dirs, spec, reach, lift), on, on.stats, tag + " again")
    return on, want, dev


# ---- frames against the model ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FRAMES))
def test_frames_equal_the_model(gpu_ctx, models, name):
    cfg, tiles = sc.FRAMES[name]()
    res = run_gpu(gpu_ctx, cfg, tiles)
    W, H = res["width"], res["height"]
    dirs, table, spec, want = models(name, cfg, tiles, res)
    before = full_call(gpu_ctx, dirs, res)  # atmrt_shadow_lights: the geometric rule, as it was
    got = full_call(gpu_ctx, dirs, res, spec)
    rebuilt, ms = generators.sky_table_work(gpu_ctx)
    t = generators.shadow_timings(gpu_ctx)
    moved = [int((got.status[l] != before.status[l]).sum()) for l in range(len(dirs))]
    print(f"shadow true {name}: {W}x{H} m={want.m} stats={got.stats} model={want.stats_on} geometric={before.stats} pixels whose status moved per light {moved} "
          f"table rebuilt {rebuilt} {ms}, march {t['march_ms']:.3f} ms")
    assert want.m == 200 and got.status.shape == (len(LIGHTS), H, W)
    assert_lights(got, want, want.stats_on, name)
    hit = W * H - got.stats["none"]
    assert got.stats["lit"] + got.stats["shadowed"] == hit * len(LIGHTS)
    assert (got.status[2][got.status[2] != sm.NONE] == sm.SHADOWED).all() and (got.status[3][got.status[3] != sm.NONE] == sm.LIT).all()
    if name == "straight":  # straight rays: the apparent elevation is the true one, the two rules agree
        assert_lights(got, before, before.stats, name + " against the geometric rule")
    # the geometric call after the true one: the bytes it gave before; the true call again: its own, from the table it finds
    after = full_call(gpu_ctx, dirs, res)
    assert_lights(after, before, before.stats, name + " geometric after true")
    again = full_call(gpu_ctx, dirs, res, spec)
    assert_lights(again, got, got.stats, name + " again")
    assert generators.sky_table_work(gpu_ctx)[0] == 0
    if FRAMES[name][1]:
        on, off = on_and_off(lambda: full_call(gpu_ctx, dirs, res, spec))
        print(f"shadow true escape {name}: on {on.stats}, off {off.stats}")
        assert_lights(on, want, want.stats_on, name + " on")
        assert_lights(off, want, want.stats_off, name + " off")
        assert off.stats["integrated_steps"] > on.stats["integrated_steps"] and on.stats["escaped_rays"] > 0 and off.stats["escaped_rays"] == 0


def test_routes_agree(gpu_ctx, models):
    """atmrt_shadow_lights_true_device, and atmrt_shadow_lights_true_planes_device over the frame's first trace points: the bytes and
    counts of atmrt_shadow_lights_true."""
    name = "fast_50x20"
    cfg, tiles = sc.FRAMES[name]()
    res = run_gpu(gpu_ctx, cfg, tiles)
    W, H = res["width"], res["height"]
    dirs, table, spec, want = models(name, cfg, tiles, res)
    host = full_call(gpu_ctx, dirs, res, spec)
    assert_lights(host, want, want.stats_on, "host route")
    lights, keep = generators.shadow_lights_spec(dirs, slc.REACH)
    n = len(dirs)
    lib, st = gpu_ctx.lib, _abi.ShadowStats()
    mask = torch.full((H, W), FILL, dtype=torch.int64, device="cuda")
    status = torch.full((n, H, W), FILL, dtype=torch.uint8, device="cuda")
    block = torch.full((n, H, W), FILL, dtype=torch.int16, device="cuda")
    gpu_ctx.check(lib.atmrt_shadow_lights_true_device(gpu_ctx.handle, C.byref(lights), C.byref(spec), mask.data_ptr(), status.data_ptr(), block.data_ptr(),
                                                      C.byref(st)))
    assert mask.cpu().numpy().tobytes() == host.lit_mask.tobytes() and status.cpu().numpy().tobytes() == host.status.tobytes()
    assert block.cpu().numpy().tobytes() == host.block.tobytes() and generators._shadow_stats(st) == host.stats
    hit = res["hit_count"] > 0
    first = res["hit_offset"][hit].astype(np.int64)
    planes = {}
    for k in ("lat", "lon", "elevation"):
        a = np.full((H, W), np.nan)
        a[hit] = res[k][first]
        planes[k] = a.ravel()
    got = TruePlanes(dict(hit_count=res["hit_count"], **planes)).lights_true(gpu_ctx, dirs, spec, slc.REACH)
    print(f"shadow true routes: {got.stats}")
    assert_lights(got, host, host.stats, "planes route")
    # the mask alone, the status alone, no stats
    gpu_ctx.check(lib.atmrt_shadow_lights_true_device(gpu_ctx.handle, C.byref(lights), C.byref(spec), mask.data_ptr(), None, None, None))
    assert mask.cpu().numpy().tobytes() == host.lit_mask.tobytes()
    status.fill_(FILL)
    gpu_ctx.check(lib.atmrt_shadow_lights_true_device(gpu_ctx.handle, C.byref(lights), C.byref(spec), None, status.data_ptr(), None, None))
    assert status.cpu().numpy().tobytes() == host.status.tobytes()


# ---- the planes route over hand-made points -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_sphere(oracle_det):
    """The 3000 km sphere under US-76: the wall world of tests/test_gpu_shadow_lights.py and the table of its setting."""
    cfg = sphere_world()
    st = sm.Setting(oracle_det, cfg, ssc.wall_tile())
    yield cfg, st, table_model(oracle_det, cfg)
    st.close()


@pytest.mark.parametrize("n_lights", (1, 64))
def test_one_and_64_lights(gpu_ctx, small_sphere, n_lights):
    """1 and 64 lights over the 65-point list in front of the wall: bit 63, a list that ends one entry into its second wavefront."""
    cfg, setting, table = small_sphere
    configure(gpu_ctx, cfg, ssc.wall_tile())
    dirs = slc.fan_of_lights(n_lights)
    lat, lon, elev = ssc.list_points(65)
    on, want, _ = check_planes(gpu_ctx, setting, table, ssc.planes(lat, lon, elev), dirs, f"{n_lights} lights")
    assert on.status.shape == (n_lights, 1, 65)
    assert not (on.lit_mask >> np.uint64(n_lights - 1) >> np.uint64(1)).any()
    moved = np.abs(want.elevation - want.true_elevation)[want.marched]
    print(f"shadow true {n_lights} lights: the launch elevation moved by {moved.min():.4f} .. {moved.max():.4f} deg")
    assert (moved > 0.0).all()
    if n_lights == 64:
        assert (on.lit_mask >> np.uint64(63)).any() and len({int(v) for v in on.lit_mask.ravel()}) > 1
        assert (want.status == sm.SHADOWED).any() and (want.status == sm.LIT).any()


def test_a_list_that_straddles_the_terminator(gpu_ctx, oracle_det, small_sphere):
    """shadow_lights_cases.terminator_points: the light's true local elevation runs from -30 to +30 degrees within ONE wavefront, so
    the lanes' bisections end in all three arms side by side."""
    _, _, table = small_sphere
    cfg, tiles, _ = ssc.wide_world(earth=slc.SMALL_SPHERE)
    configure(gpu_ctx, cfg, tiles)
    setting = sm.Setting(oracle_det, cfg, tiles)
    try:
        lat, lon, elev = slc.terminator_points(64)
        dirs = [slm.light_direction(oracle_det, cfg.params.earth, *slc.TERMINATOR_LIGHT_AT)]
        on, want, _ = check_planes(gpu_ctx, setting, table, ssc.planes(lat, lon, elev), dirs, "terminator")
        true, el = want.true_elevation[0].ravel(), want.elevation[0].ravel()
        arms = {sam.row(table.spec, table.T[0], int(table.tail[0]), t)[1] for t in true}
        print(f"shadow true terminator: true {true.min():.2f} .. {true.max():.2f} deg, arms of row 0 {sorted(arms)}")
        assert true.min() < -25.0 and true.max() > 25.0 and (np.diff(true) > 0).all() and arms == {"below", "inside", "above"}
        assert (el > true).all()  # refraction lifts every light
        assert (on.status[0].ravel()[el < -1.0] == sm.SHADOWED).all() and (on.status[0].ravel()[el > 20.0] == sm.LIT).all()
    finally:
        setting.close()


def test_the_sunset_planes(gpu_ctx, oracle_det):
    """tests/test_sky_apparent_model.py's sunset on the device: with the table every point is LIT, the same call without it gives
    the opposite status at every point."""
    cfg = sac.sunset_cfg()
    configure(gpu_ctx, cfg, {})
    setting = sm.Setting(oracle_det, cfg, {})
    try:
        table = table_model(oracle_det, cfg)
        lat, lon, elev = sac.sunset_points()
        res = ssc.planes(lat, lon, elev)
        dirs = [slm.light_direction(oracle_det, cfg.params.earth, *sac.SUNSET_AT, 90.0, sac.SUNSET_TRUE_ELEVATION)]
        on, want, dev = check_planes(gpu_ctx, setting, table, res, dirs, "sunset", sac.SUNSET_REACH, sac.SUNSET_LIFT)
        geometric = dev.lights(gpu_ctx, dirs, sac.SUNSET_REACH, sac.SUNSET_LIFT)
        geometric_want = slm.solve(setting, res, dirs, sac.SUNSET_REACH, sac.SUNSET_LIFT)
        assert_lights(geometric, geometric_want, geometric_want.stats_on, "sunset geometric")
        print(f"shadow true sunset: apparent {want.elevation.min():.4f} .. {want.elevation.max():.4f} deg; true rule {on.stats}, geometric {geometric.stats}")
        assert (on.status == sm.LIT).all() and (on.lit_mask == 1).all()
        assert (geometric.status == sm.SHADOWED).all() and not geometric.lit_mask.any()
        assert (geometric.status != on.status).all()
    finally:
        setting.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(gpu_ctx, models):
    name = "fast_50x20"
    cfg, tiles = sc.FRAMES[name]()
    res = run_gpu(gpu_ctx, cfg, tiles)
    W, H = res["width"], res["height"]
    dirs, table, good, want = models(name, cfg, tiles, res)
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    bad, state = _abi.ERR_INVALID_ARGUMENT, _abi.ERR_STATE
    mask, status = np.full((H, W), 9, np.uint64), np.full((len(dirs), H, W), 9, np.uint8)
    d_mask = torch.zeros((H, W), dtype=torch.int64, device="cuda")
    d_f64 = torch.zeros((H, W), dtype=torch.float64, device="cuda")
    d_cnt = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    lights, keep = generators.shadow_lights_spec(dirs, slc.REACH)

    def calls(handle, lspec, tspec, with_outputs=True):
        lp, tp = (None if s is None else C.byref(s) for s in (lspec, tspec))
        m, dm = (mask.ctypes.data, d_mask.data_ptr()) if with_outputs else (None, None)
        return (lib.atmrt_shadow_lights_true(handle, lp, tp, m, status.ctypes.data if with_outputs else None, None, None),
                lib.atmrt_shadow_lights_true_device(handle, lp, tp, dm, None, None, None),
                lib.atmrt_shadow_lights_true_planes_device(handle, lp, tp, W * H, d_cnt.data_ptr(), d_f64.data_ptr(), d_f64.data_ptr(), d_f64.data_ptr(),
                                                           dm, None, None, None))

    def table_of(alt=(0.0, 3000.0, 3), el=(-3.0, 9.8, 257), **sky):
        return generators.sky_table_spec(alt, el, **dict(dict(step=1000.0, top=100000.0, floor=0.0, m=1500), **sky))

    assert calls(h, lights, good) == (0, 0, 0)
    mask[:], status[:] = 9, 9
    for k, tspec in enumerate([None, table_of(alt=(5.0, 5.0, 3)), table_of(el=(-90.0, 9.8, 257)), table_of(el=(-3.0, 90.0, 257)), table_of(alt=(0.0, 3000.0, 1)),
                               table_of(alt=(0.0, 3000.0, 1025)), table_of(el=(-3.0, 9.8, 1)), table_of(alt=(0.0, 3000.0, 512), el=(-3.0, 9.8, 65536)),
                               table_of(step=-1.0), table_of(top=float("nan")), table_of(m=0)]):
        assert calls(h, lights, tspec) == (bad,) * 3, k
        assert lib.atmrt_last_error(h), k
    # what atmrt_shadow_lights refuses, the true calls refuse
    for lspec, keep2 in (generators.shadow_lights_spec(dirs, 0.0), generators.shadow_lights_spec(dirs, slc.REACH, -1.0), generators.shadow_lights_spec([[0.0, 0.0, 0.0]], slc.REACH),
                         generators.shadow_lights_spec(np.ones((65, 3)), slc.REACH)):
        assert calls(h, lspec, good) == (bad,) * 3
    assert calls(h, None, good) == (bad,) * 3 and calls(h, lights, good, with_outputs=False) == (bad,) * 3
    # a table with an unusable row: its two entries are GROUND
    assert calls(h, lights, table_of(el=(-3.0, -2.95, 2))) == (bad,) * 3 and b"not usable" in lib.atmrt_last_error(h)
    assert (mask == 9).all() and (status == 9).all()
    again = full_call(gpu_ctx, dirs, res, good)
    assert_lights(again, want, want.stats_on, "after the refusals")
    # no parameters, then parameters and no frame
    fresh = generators.Context(gpu_ctx.device)
    try:
        assert calls(fresh.handle, lights, good) == (state,) * 3 and b"atmrt_set_params" in lib.atmrt_last_error(fresh.handle)
        generators.make_generator(generators.Params(cfg), generators.Terrain.from_tiles(tiles, fresh))._configure()
        rc = calls(fresh.handle, lights, good)
        assert rc[:2] == (state,) * 2 and b"needs a frame" in lib.atmrt_last_error(fresh.handle)
        assert rc[2] == _abi.OK and not d_mask.any()  # the planes call needs no frame: all NONE here
    finally:
        fresh.close()
    multi = generators.Context.multi([gpu_ctx.device, gpu_ctx.device])
    try:
        generators.make_generator(generators.Params(cfg), generators.Terrain.from_tiles(tiles, multi))._configure()
        assert lib.atmrt_shadow_lights_true(multi.handle, C.byref(lights), C.byref(good), mask.ctypes.data, None, None, None) == state
        assert b"atmrt_shadow_lights_true_planes_device" in lib.atmrt_last_error(multi.handle)
        assert lib.atmrt_shadow_lights_true_planes_device(multi.handle, C.byref(lights), C.byref(good), W * H, d_cnt.data_ptr(), d_f64.data_ptr(),
                                                          d_f64.data_ptr(), d_f64.data_ptr(), d_mask.data_ptr(), None, None, None) == _abi.OK
    finally:
        multi.close()
