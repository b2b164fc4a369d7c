"""atmrt_debug_interp_blend — the last stage of an InterpolatingRectilinear frame (k_lattice_keys, k_interp_blend<FILL,4>,
k_interp_blend_big<FILL>, k_lattice_steps and the host sequence count -> scan -> arena -> scan -> fill -> finish, the very function the
frame calls) — on the hand-made lattices of tests/interp_blend_cases.py against tests/interp_blend_model.py, a model written from the
reference's text (interpolating_rectilinear.rs:186-418, generators/mod.rs:33-79) and from nothing of the kernels or the oracle.

The bar is bit equality of every output: hit_count, hit_offset (the order of the points), every f64 field, the tags and rgba, both
angle planes (also where a pixel has no point), n_hits and ray_steps.  tests/test_interp_blend_model.py shows, with the model alone,
that the cases reach all 16 masks accepted and rejected, every comparison with 0.5 from both sides and at equality, the 4 / 5
hand-over, more than 255 groups and several hundred arena pixels."""
import ctypes as C

import numpy as np
import pytest

import interp_blend_cases as cases
import interp_blend_model as model
from atm_raytracer_amd import _abi

pytestmark = pytest.mark.gpu


def probe(ctx, case):
    return ctx.debug_interp_blend(case["elev"], case["dir"], case["min_elev_step"], case["min_dir_step"], case["simulation_step"], case["lattice"])


def check(ctx, case):
    got, want = probe(ctx, case), model.expected(case)[0]
    bad = model.differences(got, want)
    if bad:
        where = ""
        if "hit_count" in bad:
            y, x = np.argwhere(got["hit_count"] != want["hit_count"])[0]
            where = f": first at pixel ({y}, {x}), {got['hit_count'][y, x]} points against {want['hit_count'][y, x]}, keys {want['keys'][y, x]}, remainders {want['rems'][y, x]}"
        else:
            for k in bad:
                if k in ("azimuth", "elevation_angle"):
                    y, x = np.argwhere(got[k] != want[k])[0]
                    where = f": {k} first at pixel ({y}, {x}): {got[k][y, x]!r} against {want[k][y, x]!r}, remainders {want['rems'][y, x]}"
                    break
                if k in model.FIELDS and k != "hit_offset":
                    n = int(np.argwhere(np.asarray(got[k]).reshape(len(got[k]), -1) != np.asarray(want[k]).reshape(len(got[k]), -1))[0][0])
                    p = int(np.searchsorted(want["hit_offset"].ravel(), n, side="right")) - 1
                    y, x = divmod(p, want["width"])
                    where = f": {k} first at point {n} of pixel ({y}, {x}): {got[k][n]!r} against {want[k][n]!r}, remainders {want['rems'][y, x]}"
                    break
        raise AssertionError(f"{case['name']}: {bad} differ from the model{where} (n_hits {got['n_hits']} / {want['n_hits']}, ray_steps {got['ray_steps']} / {want['ray_steps']})")
    return got


def same_bytes(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in model.FIELDS) and (a["n_hits"], a["ray_steps"]) == (b["n_hits"], b["ray_steps"])


def test_a_table_every_mask_at_every_remainder(gpu_ctx):
    """16 masks x {0, 0.25, just below 0.5, 0.5, 0.75, just below 1}^2: one point per corner present, with field values of its own."""
    for case in cases.cases("a"):
        check(gpu_ctx, case)


def test_b_grouping_rules(gpu_ctx):
    """The strict `<` of a step, the ulp below it, the class, the first group in creation order, membership through a later member,
    the later point of a corner, output in creation order."""
    for case in cases.cases("b"):
        check(gpu_ctx, case)


def test_c_handover_between_the_two_kernels(gpu_ctx):
    """Every split of 4 points over the corners (the in-register kernel's last pixel) and the same pixel with a fifth, far point of
    the other class (the arena kernel's first): the groups they share blend to the same bits."""
    case, = cases.cases("c")
    got = check(gpu_ctx, case)
    off, cnt = got["hit_offset"].ravel(), got["hit_count"].ravel()
    record = lambda k: b"".join(np.asarray(got[f][k]).tobytes() for f in model.FIELDS[4:])
    for p4, p5 in case["pairs"]:
        four = [record(k) for k in range(int(off[p4]), int(off[p4] + cnt[p4]))]
        five = [record(k) for k in range(int(off[p5]), int(off[p5] + cnt[p5])) if got["distance"][k] != 9000.0]
        assert four == five and cnt[p5] - cnt[p4] in (0, 1), (p4, p5)
        assert got["azimuth"].ravel()[p4] != got["azimuth"].ravel()[p5]  # cells of their own


def test_d_arena_many_points_many_groups_many_pixels(gpu_ctx):
    """64 points in a few groups, 320 groups (ids above 255), and 257 x 3 pixels of which several hundred take their member range
    from the arena's cursor, in any order; every case twice on the one context: a stale cursor or counter would show in the second."""
    for case in cases.cases("d"):
        first = check(gpu_ctx, case)
        assert same_bytes(first, probe(gpu_ctx, case)), case["name"]


def test_e_keys_negative_integer_and_the_last_lane(gpu_ctx):
    """Keys of both signs (the floor goes down), integer quotients, the bounds' minimum and maximum in the last lane of the last
    block, single-pixel images.  A bound that is missed changes the rectangle, and the probe refuses the lattice."""
    for case in cases.cases("e"):
        check(gpu_ctx, case)


def test_f_steps_count_each_referenced_point_once(gpu_ctx):
    for case in cases.cases("f"):
        check(gpu_ctx, case)


def test_g_seeded_sweep(gpu_ctx):
    for case in cases.cases("g"):
        check(gpu_ctx, case)


def test_refusals_leave_the_context_usable(gpu_ctx):
    """Wrong ne x nd, NULL planes, a zero or NaN step, an n_hits that is not the sum, an unknown tag: ATMRT_ERR_INVALID_ARGUMENT, and
    the next call on the context gives the model's bits."""
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    good = cases.cases("e")[2]  # a single pixel: a lattice of 2 x 2 points, one trace point each
    assert good["elev"].shape == (1, 1) and good["lattice"]["hit_count"].tolist() == [[1, 1], [1, 1]]
    elev, dirs = np.ascontiguousarray(good["elev"]), np.ascontiguousarray(good["dir"])
    steps = (good["min_elev_step"], good["min_dir_step"], good["simulation_step"])

    def call(lattice=good["lattice"], elev_ptr=elev.ctypes.data, dir_ptr=dirs.ctypes.data, steps=steps, edit=None, res=True):
        lat, keep = _abi.interp_lattice(lattice)
        if edit:
            edit(lat)
        out = _abi.Result()
        rc = lib.atmrt_debug_interp_blend(h, 1, 1, elev_ptr, dir_ptr, steps[0], steps[1], steps[2], C.byref(lat), C.byref(out) if res else None)
        assert rc != 0 or out.n_pixels == 1
        lib.atmrt_result_free(C.byref(out))
        del keep
        return rc

    def refused(**kw):
        assert call(**kw) == _abi.ERR_INVALID_ARGUMENT, kw
        check(gpu_ctx, good)

    assert call() == 0
    wide = {k: (np.concatenate([v, v[:1]], axis=0) if k in ("azimuth", "elevation_angle", "px_steps") else v) for k, v in good["lattice"].items()}
    wide["hit_count"] = np.array([[1, 1], [1, 1], [0, 0]], dtype=np.uint32)
    refused(lattice=wide)                                           # 3 x 2 points, the ray references 2 x 2
    narrow = {k: (v[:, :1] if k in ("azimuth", "elevation_angle", "px_steps", "hit_count") else v[:2]) for k, v in good["lattice"].items()}
    refused(lattice=narrow)                                         # 2 x 1
    refused(elev_ptr=None), refused(dir_ptr=None), refused(res=False)
    for plane in ("hit_count", "azimuth", "elevation_angle", "px_steps", "distance", "color_tag", "rgba"):
        refused(edit=lambda lat, plane=plane: setattr(lat, plane, None))
    assert lib.atmrt_debug_interp_blend(h, 1, 1, elev.ctypes.data, dirs.ctypes.data, steps[0], steps[1], steps[2], None, C.byref(_abi.Result())) == _abi.ERR_INVALID_ARGUMENT
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        for k in range(3):
            refused(steps=tuple(bad if j == k else s for j, s in enumerate(steps)))
    refused(edit=lambda lat: setattr(lat, "n_hits", 3))
    tagged = dict(good["lattice"], color_tag=np.array([0, 1, 2, 0], dtype=np.uint32))
    refused(lattice=tagged)
    lat, keep = _abi.interp_lattice(good["lattice"])
    for w, hgt in ((0, 1), (1, 0), (65536, 1)):  # an empty image; a side a frame cannot have
        assert lib.atmrt_debug_interp_blend(h, w, hgt, elev.ctypes.data, dirs.ctypes.data, steps[0], steps[1], steps[2], C.byref(lat),
                                            C.byref(_abi.Result())) == _abi.ERR_INVALID_ARGUMENT
    del keep
    check(gpu_ctx, good)
