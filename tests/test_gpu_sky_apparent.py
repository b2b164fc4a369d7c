"""atmrt_sky_table and atmrt_sky_apparent on the GPU against tests/sky_apparent_model.py (the rule of include/atmrt.h, "apparent
elevation", over the oracle's stepper): the table's planes and tail byte for byte over five settings and the lattice sizes at
which a wavefront or a row ends; the cached product (found, rebuilt by a changed top, by a changed atmosphere); the list call
against atmrt_sky_apparent_host over the downloaded table; the refusals that need a context.  The settings and lattices are
tests/sky_apparent_cases.py's; tests/test_sky_apparent_model.py asserts without a GPU what they hold.  Every case prints its
figures before it asserts."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import shadow_cases as sc
import sky_apparent_cases as sac
import sky_apparent_model as sam
import sky_model as skm
from atm_raytracer_amd import _abi, generators
from test_gpu_shadow_sweep import configure
from util import run_gpu

pytestmark = pytest.mark.gpu


def same_bytes(got, want):
    """Equal bytes, every NaN taken as one value."""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype.kind == "f":
        nan = np.isnan(want)
        return bool((np.isnan(got) == nan).all()) and got[~nan].tobytes() == want[~nan].tobytes()
    return got.tobytes() == want.tobytes()


@pytest.fixture(scope="module")
def models(oracle_det):
    """The model's table per (setting, n_alt, n_el), computed once and shared."""
    made = {}

    def get(name, n_alt=3, n_el=257):
        if (name, n_alt, n_el) not in made:
            cfg, top = sac.setting_of(name)
            made[(name, n_alt, n_el)] = sam.build(skm.Setting.of_config(oracle_det, cfg), sac.table_spec(n_alt, n_el, top))
        return made[(name, n_alt, n_el)]

    return get


def assert_table(got, want, tag):
    for k, w in (("true_elevation", want.T), ("status", want.S), ("tail", want.tail)):
        g = getattr(got, k)
        assert same_bytes(g, w), f"{tag} {k}: {int((g != w).sum())} of {g.size} differ"
    assert got.stats == want.stats, (tag, got.stats, want.stats)


@pytest.mark.parametrize("name", sorted(sac.SETTINGS))
def test_the_table_equals_the_model(gpu_ctx, models, name):
    cfg, top = sac.setting_of(name)
    configure(gpu_ctx, cfg, {})
    for n_alt in sac.N_ALT:
        for n_el in sac.N_EL:
            want = models(name, n_alt, n_el)
            got = generators.sky_table(gpu_ctx, sac.abi_spec(want.spec))
            print(f"sky table {name} {n_alt} x {n_el}: tail {got.tail.tolist()} stats {got.stats} rebuilt {got.rebuilt} "
                  f"march {got.ms['march_ms']:.3f} tail {got.ms['tail_ms']:.3f} download {got.ms['download_ms']:.3f} ms")
            assert_table(got, want, f"{name} {n_alt} x {n_el}")
            assert got.rebuilt == 1
    want = models(name)
    if name == "spline100":  # every ascending ray is LOST: the table is built and shown, the inverse and the shadow call refuse it
        assert (want.tail == want.spec.n_el).all()
        spec = sac.abi_spec(want.spec)
        with pytest.raises(generators.AtmrtError) as err:
            generators.sky_apparent(gpu_ctx, [100.0], [1.0], spec)
        assert err.value.status == _abi.ERR_INVALID_ARGUMENT and "row 0" in err.value.message
        count, plane = np.ones(4, dtype=np.uint32), np.zeros(4)
        d_count, d_plane, d_mask = torch.from_numpy(count.view(np.int32)).cuda(), torch.from_numpy(plane).cuda(), torch.zeros(4, dtype=torch.int64, device="cuda")
        lights, keep = generators.shadow_lights_spec([[1.0, 0.0, 0.2]], 5000.0)
        rc = gpu_ctx.lib.atmrt_shadow_lights_true_planes_device(gpu_ctx.handle, C.byref(lights), C.byref(spec), 4, d_count.data_ptr(), d_plane.data_ptr(),
                                                                d_plane.data_ptr(), d_plane.data_ptr(), d_mask.data_ptr(), None, None, None)
        assert rc == _abi.ERR_INVALID_ARGUMENT and b"row 0" in gpu_ctx.lib.atmrt_last_error(gpu_ctx.handle)
        assert generators.sky_table(gpu_ctx, spec).rebuilt == 0  # and the table is still there
        # the frame routes: a frame generated under this atmosphere, then atmrt_shadow_lights_true[_device] over it
        fcfg, tiles = sc.scene(50, 20, atmosphere=sc.spline_atmosphere(), earth_shape=sac.SPHERE)
        res = run_gpu(gpu_ctx, fcfg, tiles)
        assert (res["hit_count"] > 0).any()
        dirs = generators.lights_from_angles(fcfg.params, [(260.0, 2.0)], gpu_ctx.lib)
        with pytest.raises(generators.AtmrtError) as err:
            generators.shadow_lights(gpu_ctx, dirs, sc.REACH, width=res["width"], height=res["height"], true_table=spec)
        assert err.value.status == _abi.ERR_INVALID_ARGUMENT and "atmrt_shadow_lights_true: row 0" in err.value.message and "not usable" in err.value.message
        d_mask = torch.zeros((res["height"], res["width"]), dtype=torch.int64, device="cuda")
        lights, keep = generators.shadow_lights_spec(dirs, sc.REACH)
        assert gpu_ctx.lib.atmrt_shadow_lights_true_device(gpu_ctx.handle, C.byref(lights), C.byref(spec), d_mask.data_ptr(), None, None, None) == _abi.ERR_INVALID_ARGUMENT
        assert not d_mask.any()
        table = generators.sky_table(gpu_ctx, spec)  # the frame's setting: the same all-LOST table
        assert (table.tail == spec.n_el).all() and _abi.SKY_EXIT not in table.status
        assert generators.shadow_lights(gpu_ctx, dirs, sc.REACH, width=res["width"], height=res["height"]).stats["lit"] > 0  # the geometric call works
    else:
        assert want.usable.all()


# (setting, top, the statuses the CPU model finds in each of the two rows)
TWO_KERNEL_CASES = [("us76_sphere", 100000.0, {skm.EXIT, skm.GROUND, skm.INSIDE}), ("spline100", 100000.0, {skm.GROUND, skm.LOST}),
                    ("spline30", 30000.0, {skm.EXIT, skm.GROUND})]


@pytest.mark.parametrize("name,top,statuses", TWO_KERNEL_CASES, ids=[c[0] for c in TWO_KERNEL_CASES])
def test_the_table_march_equals_the_list_march(gpu_ctx, name, top, statuses):
    """k_sky_table_march against k_sky_march, the device against itself: a 2 x 65 lattice (k runs fastest: the second wavefront
    holds one ray of row 0 and 63 of row 1, two values of h0, and the last wavefront holds two rays), 1000 m steps, m = 1000,
    elevations from -1.2 degrees by 0.05.  T (bits) and S of each row equal atmrt_sky_rays from the row's altitude over the row's
    elevations.  US-76 to 100 km: GROUND, EXIT and INSIDE in both rows; the Spline atmosphere to 100 km (NaN above its last
    point: GROUND and LOST) and to 30 km (GROUND and EXIT through the cubic stepper)."""
    cfg, _ = sac.setting_of(name)
    configure(gpu_ctx, cfg, {})
    mspec = sam.Spec((0.0, 1500.0, 2), (-1.2, 2.0, 65), step=1000.0, top=top, floor=0.0, m=1000)
    table = generators.sky_table(gpu_ctx, sac.abi_spec(mspec))
    counted = dict(exit=0, ground=0, inside=0, lost=0, integrated_steps=0)
    for j in range(mspec.n_alt):
        elevations = np.array([mspec.el(k) for k in range(mspec.n_el)])
        rec, stats = generators.sky_rays(gpu_ctx, mspec.alt(j), elevations, step=mspec.step, top=mspec.top, floor=mspec.floor, m=mspec.m)
        print(f"table march {name} row {j} ({mspec.alt(j)} m): {stats}")
        assert same_bytes(table.true_elevation[j], rec["true_elevation"]), j
        assert table.status[j].tolist() == rec["status"].tolist(), j
        assert statuses <= set(rec["status"].tolist()), (j, set(rec["status"].tolist()))
        assert not np.isnan(rec["true_elevation"][rec["status"] == skm.EXIT]).any()
        for key in counted:
            counted[key] += stats[key]
    assert table.stats == dict(counted, none=0), (table.stats, counted)


def test_the_table_is_kept_with_its_key(gpu_ctx, models):
    cfg, top = sac.setting_of("us76_sphere")
    configure(gpu_ctx, cfg, {})
    want = models("us76_sphere", 3, 65)
    spec = sac.abi_spec(want.spec)
    other = sac.abi_spec(sac.table_spec(3, 64, top))
    generators.sky_table(gpu_ctx, other)  # whatever the context held before
    first = generators.sky_table(gpu_ctx, spec)
    again = generators.sky_table(gpu_ctx, spec)
    print(f"sky table kept: first {first.rebuilt} {first.ms}, again {again.rebuilt} {again.ms}")
    assert (first.rebuilt, again.rebuilt) == (1, 0) and again.ms["march_ms"] == 0.0 and again.ms["tail_ms"] == 0.0
    assert_table(first, want, "first")
    assert_table(again, want, "again")
    tail_only = generators.sky_table(gpu_ctx, spec, planes=False)
    assert tail_only.rebuilt == 0 and tail_only.true_elevation is None and tail_only.tail.tobytes() == want.tail.tobytes() and tail_only.stats == want.stats
    # the list call finds it too
    generators.sky_apparent(gpu_ctx, [100.0], [1.0], spec)
    assert generators.sky_table_work(gpu_ctx)[0] == 0
    # a changed top rebuilds, and changes the bytes; the old top rebuilds again
    lower = sac.abi_spec(sac.table_spec(3, 65, 60000.0))
    low = generators.sky_table(gpu_ctx, lower)
    assert low.rebuilt == 1 and low.true_elevation.tobytes() != first.true_elevation.tobytes()
    assert generators.sky_table(gpu_ctx, lower).rebuilt == 0
    back = generators.sky_table(gpu_ctx, spec)
    assert back.rebuilt == 1
    assert_table(back, want, "back")
    # step 0 is the context's simulation_step: resolved in the key
    s0 = sac.abi_spec(want.spec, step=0.0)
    s100 = sac.abi_spec(want.spec, step=cfg.params.simulation_step)
    a = generators.sky_table(gpu_ctx, s0)
    b = generators.sky_table(gpu_ctx, s100)
    assert (a.rebuilt, b.rebuilt) == (1, 0) and a.true_elevation.tobytes() == b.true_elevation.tobytes()
    # a changed atmosphere rebuilds, under the same spec; so does straight_rays
    generators.sky_table(gpu_ctx, spec)
    cfg_spline, _ = sac.setting_of("spline30")
    configure(gpu_ctx, cfg_spline, {})
    spl = generators.sky_table(gpu_ctx, spec)
    assert spl.rebuilt == 1 and spl.true_elevation.tobytes() != first.true_elevation.tobytes()
    assert generators.sky_table(gpu_ctx, spec).rebuilt == 0
    cfg_straight, _ = sac.setting_of("straight")
    configure(gpu_ctx, cfg_straight, {})
    assert generators.sky_table(gpu_ctx, spec).rebuilt == 1
    configure(gpu_ctx, cfg, {})
    back = generators.sky_table(gpu_ctx, spec)
    assert back.rebuilt == 1
    assert_table(back, want, "back from another atmosphere")


@pytest.mark.parametrize("n", (1, 63, 64, 65, 257))
def test_the_list_call_equals_the_host_function(gpu_ctx, models, n):
    """atmrt_sky_apparent against atmrt_sky_apparent_host (which tests/test_sky_apparent_abi.py pins to the model) over the
    downloaded table, bit for bit; the 257-pair list reaches every arm and both clamps, asserted by the model's census."""
    cfg, top = sac.setting_of("us76_sphere")
    configure(gpu_ctx, cfg, {})
    want = models("us76_sphere")
    spec = sac.abi_spec(want.spec)
    table = generators.sky_table(gpu_ctx, spec)
    assert_table(table, want, "list")
    h, t = sac.census_pairs(want)
    h, t = h[:n], t[:n]
    got = generators.sky_apparent(gpu_ctx, h, t, spec)
    host = np.array([generators.sky_apparent_host(spec, table.true_elevation, table.tail, a, b, gpu_ctx.lib) for a, b in zip(h, t)])
    assert same_bytes(got, host), np.flatnonzero(~((got == host) | (np.isnan(got) & np.isnan(host))))[:5]
    if n == 257:
        parts = [sam.apparent_parts(want, a, b) for a, b in zip(h, t)]
        arms = {p[3] for p in parts} | {p[4] for p in parts}
        assert {"inside", "below", "above", "nan", None} <= arms and (h < want.spec.alt_lo).any() and (h > want.spec.alt_hi).any()
        model = np.array([p[0] for p in parts])
        assert same_bytes(got, model)
        print(f"sky apparent list: {n} pairs, arms {sorted(str(a) for a in arms)}, refraction {np.nanmin(got - t):.4f} .. {np.nanmax(got - t):.4f} deg")


def test_straight_rays_return_the_target(gpu_ctx, models):
    cfg, top = sac.setting_of("straight")
    configure(gpu_ctx, cfg, {})
    want = models("straight")
    h, t = sac.census_pairs(want)
    got = generators.sky_apparent(gpu_ctx, h, t, sac.abi_spec(want.spec))
    assert same_bytes(got, t)


def test_refusals_that_need_a_context(gpu_ctx, models):
    cfg, top = sac.setting_of("us76_sphere")
    configure(gpu_ctx, cfg, {})
    lib, handle = gpu_ctx.lib, gpu_ctx.handle
    bad, state, nan, inf = _abi.ERR_INVALID_ARGUMENT, _abi.ERR_STATE, math.nan, math.inf
    mspec = sac.table_spec(3, 65, top)
    good = sac.abi_spec(mspec)
    T, S, tail = np.full((3, 65), 9.0), np.full((3, 65), 9, dtype=np.uint8), np.full(3, 9, dtype=np.uint32)
    h, t, out = np.full(4, 100.0), np.full(4, 1.0), np.full(4, 9.0)

    def calls(hd, spec):
        p = None if spec is None else C.byref(spec)
        return (lib.atmrt_sky_table(hd, p, T.ctypes.data, S.ctypes.data, tail.ctypes.data, None),
                lib.atmrt_sky_apparent(hd, p, 4, h.ctypes.data, t.ctypes.data, out.ctypes.data))

    def spec_of(alt=(mspec.alt_lo, mspec.alt_hi, 3), el=(mspec.el_lo, mspec.el_hi, 65), **sky):
        return generators.sky_table_spec(alt, el, **dict(dict(step=1000.0, top=top, floor=0.0, m=1500), **sky))

    refused = [None, spec_of(alt=(0.0, 0.0, 3)), spec_of(alt=(10.0, 0.0, 3)), spec_of(alt=(nan, 10.0, 3)), spec_of(alt=(0.0, inf, 3)),
               spec_of(el=(-90.0, 0.2, 65)), spec_of(el=(-3.0, 90.0, 65)), spec_of(el=(1.0, 1.0, 65)), spec_of(el=(nan, 1.0, 65)),
               spec_of(alt=(0.0, 10.0, 1)), spec_of(alt=(0.0, 10.0, 1025)), spec_of(el=(-3.0, 1.0, 1)), spec_of(el=(-3.0, 1.0, 65537)),
               spec_of(alt=(0.0, 10.0, 257), el=(-3.0, 1.0, 65536)), spec_of(step=-1.0), spec_of(step=nan), spec_of(top=inf),
               spec_of(top=0.0, floor=0.0), spec_of(m=0), spec_of(m=1048576)]
    for k, spec in enumerate(refused):
        assert calls(handle, spec) == (bad, bad), k
        assert lib.atmrt_last_error(handle), k
    assert (T == 9.0).all() and (S == 9).all() and (tail == 9).all() and (out == 9.0).all()
    assert lib.atmrt_sky_apparent(handle, C.byref(good), 4, None, t.ctypes.data, out.ctypes.data) == bad
    assert lib.atmrt_sky_apparent(handle, C.byref(good), 4, h.ctypes.data, None, out.ctypes.data) == bad
    assert lib.atmrt_sky_apparent(handle, C.byref(good), 4, h.ctypes.data, t.ctypes.data, None) == bad
    assert lib.atmrt_last_sky_table_work(handle, None, (C.c_double * 3)()) == bad
    assert lib.atmrt_last_sky_table_work(handle, C.byref(C.c_int32()), None) == bad
    # every output of the table call may be NULL; n = 0 asks for nothing
    assert lib.atmrt_sky_table(handle, C.byref(good), None, None, None, None) == 0
    assert lib.atmrt_sky_apparent(handle, C.byref(good), 0, None, None, None) == 0
    assert calls(handle, good) == (0, 0) and (out != 9.0).all() and (tail != 9).all()
    # a table with an unusable row: two entries from -3 degrees are GROUND from every altitude of it
    short = spec_of(el=(-3.0, -2.95, 2))
    assert calls(handle, short) == (0, bad) and b"not usable" in lib.atmrt_last_error(handle) and tail.tolist() == [2, 2, 2]
    # no parameters
    fresh = generators.Context(gpu_ctx.device)
    try:
        assert calls(fresh.handle, good) == (state, state) and b"atmrt_set_params" in lib.atmrt_last_error(fresh.handle)
        assert calls(fresh.handle, refused[1]) == (bad, bad)  # the arguments first
        generators.make_generator(generators.Params(cfg), generators.Terrain.from_tiles({}, fresh))._configure()
        assert calls(fresh.handle, good) == (0, 0)  # no frame is needed
        rebuilt, ms = generators.sky_table_work(fresh)
        assert rebuilt == 0
    finally:
        fresh.close()
    # a multi-device context: the list calls run on its first device
    multi = generators.Context.multi([gpu_ctx.device, gpu_ctx.device])
    try:
        generators.make_generator(generators.Params(cfg), generators.Terrain.from_tiles({}, multi))._configure()
        got = generators.sky_table(multi, good)
        assert_table(got, models("us76_sphere", 3, 65), "multi")
        assert same_bytes(generators.sky_apparent(multi, h, t, good), generators.sky_apparent(gpu_ctx, h, t, good))
    finally:
        multi.close()
