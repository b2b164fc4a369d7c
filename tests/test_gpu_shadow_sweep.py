"""atmrt_shadow_mask* on the GPU against tests/shadow_model.py where the 13 fixed cases of tests/test_gpu_shadows.py do not reach:
a seeded sweep of frames and lights (every earth model's calculator with Linear and Spline steppers, the three generators, column
shards, objects, pathological atmospheres, m = 1 and reaches beyond max_distance), ridge points under a real duct, beside the escape
certificate's threshold and under straight rays on a small sphere, the model's hand-derived answers, the compacted list's edges,
m = 65535, azimuths out of range and the gathered multi-device frame.  Status and block byte for byte; every case runs with the
escape shortcut on and off, and the call's counts equal the model's for either.  The inputs are tests/shadow_sweep_cases.py's;
tests/test_shadow_sweep_model.py asserts without a GPU what they reach."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import shadow_cases as sc
import shadow_model as sm
import shadow_sweep_cases as ssc
from atm_raytracer_amd import _abi, generators
from test_gpu_shadows import assert_mask
from util import run_gpu

pytestmark = pytest.mark.gpu

FILL = 77


def on_and_off(call):
    """call() with the shortcut on and with ATMRT_SHADOW_ESCAPE=off; the environment is left as it was."""
    before = os.environ.pop("ATMRT_SHADOW_ESCAPE", None)
    try:
        on = call()
        os.environ["ATMRT_SHADOW_ESCAPE"] = "off"
        off = call()
    finally:
        os.environ.pop("ATMRT_SHADOW_ESCAPE", None)
        if before is not None:
            os.environ["ATMRT_SHADOW_ESCAPE"] = before
    return on, off


def configure(ctx, cfg, tiles):
    """The context's setting without a frame: what the planes entry point needs."""
    ctx.check(ctx.lib.atmrt_terrain_clear(ctx.handle))
    generators.make_generator(generators.Params(cfg), generators.Terrain.from_tiles(tiles, ctx))._configure()


class Planes:
    """A hand-made frame (shadow_sweep_cases.planes) in device memory."""

    def __init__(self, res):
        self.shape = res["hit_count"].shape
        self.n = res["hit_count"].size
        self.count = torch.from_numpy(res["hit_count"].astype(np.int32).ravel()).cuda()
        self.lat, self.lon, self.elev = (torch.from_numpy(np.ascontiguousarray(res[k], dtype=np.float64)).cuda() for k in ("lat", "lon", "elevation"))
        assert self.lat.numel() == self.lon.numel() == self.elev.numel() == self.n

    def mask(self, ctx, spec):
        """atmrt_shadow_mask_planes_device into buffers pre-filled with FILL -> ShadowMask."""
        status = torch.full((self.n,), FILL, dtype=torch.uint8, device="cuda")
        block = torch.full((self.n,), FILL, dtype=torch.int16, device="cuda")
        st, pod = _abi.ShadowStats(), generators.shadow_spec(*spec)
        ctx.check(ctx.lib.atmrt_shadow_mask_planes_device(ctx.handle,C.byref(pod), self.n, self.count.data_ptr(), self.lat.data_ptr(),
                                                          self.lon.data_ptr(), self.elev.data_ptr(), status.data_ptr(), block.data_ptr(), C.byref(st)))
        return generators.ShadowMask(status.cpu().numpy().reshape(self.shape), block.cpu().numpy().view(np.uint16).reshape(self.shape),
                                     generators._shadow_stats(st))


def check_planes(ctx, res, want, spec, tag):
    """The planes call on and off against the model: status, block, counts; nothing but status values in the pre-filled buffers."""
    dev = Planes(res)
    on, off = on_and_off(lambda: dev.mask(ctx, spec))
    print(f"shadow sweep {tag}: m={want.m} floor={want.floor:g} on {on.stats} off {off.stats}")
    assert_mask(on, want, want.stats_on, tag + " on")
    assert_mask(off, want, want.stats_off, tag + " off")
    return on


# ---- 1. the seeded sweep -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", ssc.SEEDS)
def test_shadow_sweep_seed(gpu_ctx, oracle_det, seed):
    c = ssc.shadow_sweep_case(seed)
    cfg, tiles, spec = c["cfg"], c["tiles"], c["spec"]
    res = run_gpu(gpu_ctx, cfg, tiles)
    W, H = res["width"], res["height"]
    st = sm.Setting(oracle_det, cfg, tiles)
    try:
        want = sm.solve(st, res, spec)
    finally:
        st.close()
    assert want.status.shape == (H, W) and generators.shadow_steps(gpu_ctx, spec[2]) == want.m
    on, off = on_and_off(lambda: generators.shadow_mask(gpu_ctx, spec, W, H))
    print(f"shadow sweep seed {seed}: {c['generator']} {W}x{H} earth {c['earth']} m={want.m} floor={want.floor:g} on {on.stats} off {off.stats}")
    assert_mask(on, want, want.stats_on, f"seed {seed} on")
    assert_mask(off, want, want.stats_off, f"seed {seed} off")
    if not (res["hit_count"] > 0).any():
        assert not on.status.any() and not on.block.any()
        assert on.stats == off.stats == dict(none=W * H, lit=0, shadowed=0, integrated_steps=0, escaped_rays=0)
    if seed % 4 == 0:
        pod, stats = generators.shadow_spec(*spec), _abi.ShadowStats()
        status = torch.full((H, W), FILL, dtype=torch.uint8, device="cuda")
        block = torch.full((H, W), FILL, dtype=torch.int16, device="cuda")
        gpu_ctx.check(gpu_ctx.lib.atmrt_shadow_mask_device(gpu_ctx.handle, C.byref(pod), status.data_ptr(), block.data_ptr(), C.byref(stats)))
        got = generators.ShadowMask(status.cpu().numpy(), block.cpu().numpy().view(np.uint16), generators._shadow_stats(stats))
        assert_mask(got, want, want.stats_on, f"seed {seed} device")


# ---- 2. ducts, threshold layers and a small sphere over ridge points -------------------------------------------------------------------
def model_over(oracle, cfg, tiles, res, spec):
    st = sm.Setting(oracle, cfg, tiles)
    try:
        return sm.solve(st, res, spec)
    finally:
        st.close()


@pytest.mark.parametrize("name", sorted(ssc.DUCT_SPECS))
def test_ridge_points_under_a_duct(gpu_ctx, oracle_det, name):
    """1024 ridge points under the real duct, 150 km: rays rise above the mosaic's top, turn in the layer and are blocked far out
    (tests/test_shadow_sweep_model.py counts them); a floor put too low would call them LIT."""
    cfg, tiles, top = ssc.duct_world()
    res, spec = ssc.ridge_points(1024), ssc.DUCT_SPECS[name]
    configure(gpu_ctx, cfg, tiles)
    want = model_over(oracle_det, cfg, tiles, res, spec)
    on = check_planes(gpu_ctx, res, want, spec, f"duct {name}")
    assert on.stats["shadowed"] >= 100 and on.stats["lit"] >= 100


def test_ridge_points_beside_the_certificates_threshold(gpu_ctx, oracle_det):
    res = ssc.ridge_points(256)
    for name, (cfg, tiles, top, certified) in sorted(ssc.threshold_worlds().items()):
        configure(gpu_ctx, cfg, tiles)
        want = model_over(oracle_det, cfg, tiles, res, ssc.THRESHOLD_SPEC)
        on = check_planes(gpu_ctx, res, want, ssc.THRESHOLD_SPEC, f"threshold {name}")
        assert (want.floor == top) == certified
        if certified:
            assert on.stats["escaped_rays"] > 0


def test_straight_rays_on_a_small_sphere(gpu_ctx, oracle_det):
    """The escape test's angle bound for the call's reach: at 44.2 degrees no ray may leave early, at 44.0 the rays above the top do."""
    cfg, tiles, top = ssc.straight_sphere_world()
    res = ssc.ridge_points(256)
    configure(gpu_ctx, cfg, tiles)
    for name, spec in sorted(ssc.STRAIGHT_SPHERE_SPECS.items()):
        want = model_over(oracle_det, cfg, tiles, res, spec)
        on = check_planes(gpu_ctx, res, want, spec, f"small sphere {name}")
        assert (on.stats["escaped_rays"] == 0) == (name == "bites")


# ---- 3. known answers, list edges, range ends ----------------------------------------------------------------------------------------
def test_known_answers_through_the_planes_entry(gpu_ctx, oracle_det):
    """Every hand-derived answer of tests/test_shadow_model.py — the wall at 5555.6 m, the point's own sample, the -1000 m guard (which
    no frame's trace point can reach: terrain is never below 0 m), the NaN elevation — and a point whose latitude is NaN: every
    geodesic point of its ray is NaN, so T_i is 0 (no tile) or NaN (a cell index saturated to tile 0, 0): H_i < T_i is false
    either way and the model gives LIT."""
    cfg = ssc.flat_world()
    loaded = None
    for name, wall, point, spec, want in ssc.KNOWN:
        if wall != loaded:
            configure(gpu_ctx, cfg, ssc.wall_tile() if wall else {})
            loaded = wall
        res = ssc.planes(*point)
        model = model_over(oracle_det, cfg, ssc.wall_tile() if wall else {}, res, spec)
        on = check_planes(gpu_ctx, res, model, spec, name)
        assert (int(on.status[0, 0]), int(on.block[0, 0])) == want, name


@pytest.fixture(scope="module")
def list_models(oracle_det):
    """The model's answer for the 1000 list points, all hit, per spec: every other case is a part of it."""
    st = sm.Setting(oracle_det, ssc.flat_world(), ssc.wall_tile())
    try:
        return {name: sm.solve(st, ssc.planes(*ssc.list_points(1000)), spec) for name, spec in ssc.LIST_SPECS.items()}
    finally:
        st.close()


@pytest.mark.parametrize("n", ssc.LIST_SIZES)
def test_list_edges(gpu_ctx, list_models, n):
    """Lists of 0, 1, 63, 64, 65, 255 .. 257 entries and the grids around them — a last block or wavefront entirely past the list,
    a list that ends one entry into a wavefront: every hit pixel has the model's answer for ITS point, the others NONE and 0, the
    counts are the model's, and a second call returns the same bytes."""
    configure(gpu_ctx, ssc.flat_world(), ssc.wall_tile())
    lat, lon, elev = ssc.list_points(n)
    for pattern in ssc.LIST_PATTERNS:
        hit = ssc.list_hits(n, pattern)
        dev = Planes(ssc.planes(lat, lon, elev, hit))
        for name, spec in sorted(ssc.LIST_SPECS.items()):
            full = list_models[name]
            status = np.where(hit, full.status.ravel()[:n], sm.NONE).astype(np.uint8).reshape(1, n)
            block = np.where(hit, full.block.ravel()[:n], 0).astype(np.uint16).reshape(1, n)
            lit, sh = int((status == sm.LIT).sum()), int((status == sm.SHADOWED).sum())
            steps = int(block.astype(np.int64).sum()) + full.m * lit
            esc = np.where(hit & (full.status.ravel()[:n] == sm.LIT), full.esc.ravel()[:n], 0)
            steps_on = steps - int((full.m - esc[esc > 0]).sum())
            base = dict(none=n - lit - sh, lit=lit, shadowed=sh)
            on, off = on_and_off(lambda: dev.mask(gpu_ctx, spec))
            tag = f"list {n} {pattern} {name}"
            for got, stats in ((on, dict(base, integrated_steps=steps_on, escaped_rays=int(((esc > 0) & (esc < full.m)).sum()))),
                               (off, dict(base, integrated_steps=steps, escaped_rays=0))):
                assert got.status.tobytes() == status.tobytes() and got.block.tobytes() == block.tobytes(), (tag, np.flatnonzero(got.status != status)[:5])
                assert got.stats == stats, (tag, got.stats, stats)
            again = dev.mask(gpu_ctx, spec)
            assert again.status.tobytes() == on.status.tobytes() and again.block.tobytes() == on.block.tobytes() and again.stats == on.stats


def test_the_last_sample_of_the_longest_ray(gpu_ctx, oracle_det):
    """m = 65535, the largest block index: one ray is below 0 m first at its last sample (block 0xFFFF), its neighbour never."""
    cfg = ssc.flat_world()
    configure(gpu_ctx, cfg, {})
    res = ssc.planes([0.5, 0.5], 0.5, [ssc.FAR_BLOCKED, ssc.FAR_LIT])
    want = model_over(oracle_det, cfg, {}, res, ssc.FAR_SPEC)
    on = check_planes(gpu_ctx, res, want, ssc.FAR_SPEC, "far")
    assert generators.shadow_steps(gpu_ctx, ssc.FAR_SPEC[2]) == 65535
    assert on.status.ravel().tolist() == [sm.SHADOWED, sm.LIT] and on.block.ravel().tolist() == [0xFFFF, 0]
    assert want.stats_off["integrated_steps"] == 2 * 65535


@pytest.mark.parametrize("azimuth", ssc.ODD_AZIMUTHS)
def test_azimuths_outside_the_circle(gpu_ctx, oracle_det, azimuth):
    """-725.5 (354.5 after two turns: toward the wall), 360, 1e6 (280) and -0.0 go straight into dircalc_new's range reduction."""
    cfg, tiles = ssc.flat_world(), ssc.wall_tile()
    configure(gpu_ctx, cfg, tiles)
    res = ssc.planes(*ssc.list_points(257))
    spec = (azimuth, 2.0, 10_000.0, 0.0)
    want = model_over(oracle_det, cfg, tiles, res, spec)
    on = check_planes(gpu_ctx, res, want, spec, f"azimuth {azimuth}")
    if azimuth != 1.0e6:  # toward the wall
        assert on.stats["shadowed"] >= 100


# ---- 4. the gathered multi-device frame ------------------------------------------------------------------------------------------------
def test_gathered_multi_device_frame(gpu_ctx, oracle_det):
    """Case `alpha` of shadow_cases generated on a two-tile multi context of the one device; the gathered first-point planes through
    atmrt_shadow_mask_planes_device on that context: the bytes and counts of atmrt_shadow_mask on the single context, and the
    model's."""
    frame, spec, _ = sc.CASES["alpha"]
    cfg, tiles = sc.FRAMES[frame]()
    res = run_gpu(gpu_ctx, cfg, tiles)
    W, H = res["width"], res["height"]
    single, single_off = on_and_off(lambda: generators.shadow_mask(gpu_ctx, spec, W, H))
    want = model_over(oracle_det, cfg, tiles, res, spec)
    assert_mask(single, want, want.stats_on, "single on")
    assert_mask(single_off, want, want.stats_off, "single off")
    ctx = generators.Context.multi([gpu_ctx.device, gpu_ctx.device])
    try:
        gen = generators.make_generator(generators.Params(cfg), generators.Terrain.from_tiles(tiles, ctx))
        dev = torch.device("cuda", gpu_ctx.device)
        images = [generators.image_planes(H, W, dev) for _ in range(2)]
        gen.generate_image_device([pod for _, pod in images])
        t = images[-1][0]
        pod = generators.shadow_spec(*spec)

        def call():
            status = torch.full((H, W), FILL, dtype=torch.uint8, device=dev)
            block = torch.full((H, W), FILL, dtype=torch.int16, device=dev)
            st = _abi.ShadowStats()
            ctx.check(ctx.lib.atmrt_shadow_mask_planes_device(ctx.handle, C.byref(pod), W * H, t["hit_count"].data_ptr(), t["lat"].data_ptr(),
                                                              t["lon"].data_ptr(), t["elevation"].data_ptr(), status.data_ptr(), block.data_ptr(), C.byref(st)))
            return generators.ShadowMask(status.cpu().numpy(), block.cpu().numpy().view(np.uint16), generators._shadow_stats(st))

        on, off = on_and_off(call)
        print(f"shadow gathered: on {on.stats} off {off.stats} single {single.stats}")
        assert on.status.tobytes() == single.status.tobytes() and on.block.tobytes() == single.block.tobytes() and on.stats == single.stats
        assert_mask(on, want, want.stats_on, "gathered on")
        assert_mask(off, want, want.stats_off, "gathered off")
        assert on.stats["lit"] > 0 and on.stats["shadowed"] > 0
    finally:
        ctx.close()
