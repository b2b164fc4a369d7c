"""The frames of tests/queue_cases.py, from the oracle and the host alone (no device): each has the property it was built for, the
escape sweep still holds enough frames that can take the work queue, and the inputs of the queue-estimate model
(tests/march_order_model.py) leave almost no group undecided — so that tests/test_gpu_march_queue_scenes.py cannot pass vacuously."""
import numpy as np
import pytest

import march_order_model as mom
import queue_cases as qc
import test_ceiling_host as host


def test_the_escape_sweep_holds_frames_for_the_queue(oracle_libm):
    """The predicate selects at least 10 of the sweep's 60 seeds and at least 6 with a Spline: a change to the sweep must not empty
    the queue's share of it silently."""
    import escape_cases as ec
    seeds = qc.eligible_seeds()
    cases = {seed: ec.frame_case(ec.load_lib(), oracle_libm, seed) for seed in seeds}
    splines = [seed for seed in seeds if qc.is_spline(cases[seed]["cfg"])]
    kinds = {cases[seed]["kind"] for seed in seeds}
    print(f"\neligible seeds {seeds}; with a Spline {splines}; kinds {sorted(kinds)}")
    assert len(seeds) >= 10 and len(splines) >= 6, (seeds, splines)
    assert kinds == {"threshold", "duct", "random"}
    for seed in seeds:  # what the predicate promises, stated on the configuration itself
        p = cases[seed]["cfg"].params
        assert p.terrain_alpha == 1.0 and not cases[seed]["cfg"].objects and p.col_begin == 0 and p.col_end in (0, p.width)


def test_every_frame_is_one_the_queue_can_take():
    from atm_raytracer_amd import _abi
    kinds = [_abi.EARTH_KINDS[k] for k in qc.QUEUE_EARTHS]
    for name in list(qc.FRAMES) + ["spikes-" + n for n in qc.SPIKE_FRAMES]:
        cfg, _ = qc.build(name)
        p = cfg.params
        assert p.terrain_alpha == 1.0 and not cfg.objects and p.col_begin == 0 and p.col_end in (0, p.width), name
        assert p.earth.kind in kinds and p.generator == _abi.GENERATORS["Rectilinear"], name
        assert qc.is_spline(cfg) == (name in qc.SPLINE_FRAMES), name


GROUPS = {"spline-inversion": 60, "spline-partial": 11, "duct-linear": 24, "duct-spline": 24, "all-sky": 8, "all-ground": 8, "two-steps": 8,
          "high-observer": 72}
HITS = {"duct-linear": 768, "duct-spline": 816, "straight": 2409, "observer-ae": 2414, "simple-observer-ae-straight": 2413,
        "small-radius": 2875, "simple-sphere-violet": 2409, "all-sky": 0, "all-ground": 512, "wild-spline": 997, "long-atmosphere": 966,
        "cubic-interval": 967}


def test_the_frames_have_the_properties_they_were_built_for(oracle_det):
    from util import run_oracle
    want = {name: qc.oracle_frame(oracle_det, name) for name in qc.FRAMES}
    for name, r in want.items():
        pixels = r["hit_count"].size
        print(f"{name}: {pixels} pixels, {qc.groups(qc.build(name)[0])} groups, {int(r['n_hits'])} hits, {r['ray_steps'] / pixels:.1f} steps per ray")
    for name, n in GROUPS.items():
        assert qc.groups(qc.build(name)[0]) == n, name
    for name, n in HITS.items():
        assert int(want[name]["n_hits"]) == n, (name, int(want[name]["n_hits"]))
    assert want["spline-partial"]["hit_count"].size % 64 == 10 and want["spline-partial"]["n_hits"] > 0
    # the layer lies inside the terrain's altitude range: the frame is not US-76's
    twin = run_oracle(oracle_det, *qc.us76_twin())
    assert qc.digest(want["spline-inversion"]) != qc.digest(twin) and want["spline-inversion"]["n_hits"] > 0
    assert want["spline-inversion"]["ray_steps"] != twin["ray_steps"] or qc.digest(want["spline-inversion"])[0] != qc.digest(twin)[0]
    assert want["all-sky"]["ray_steps"] == 512 * 600 and want["all-ground"]["ray_steps"] == 512
    two = want["two-steps"]
    assert qc.build("two-steps")[0].params.frame.max_distance / qc.build("two-steps")[0].params.simulation_step == 2.5  # march_steps = 2
    assert 0 < int((two["hit_count"] > 0).sum()) < 512 and two["ray_steps"] <= 2 * 512
    assert int(want["duct-linear"]["ray_steps"]) // (48 * 32) == 1537 and int(want["duct-spline"]["ray_steps"]) // (48 * 32) == 1545
    assert int(want["small-radius"]["ray_steps"]) // (96 * 40) == 155
    high = want["high-observer"]
    assert high["n_hits"] > 0 and (high["hit_count"] == 0).sum() > 0


# ---- the inputs of the queue-estimate model: tables from the host builder, planes from the oracle ----
@pytest.fixture(scope="module")
def exe():
    return host._exe("ceiling_host", ["-O2"])


def host_estimates(exe, tmp_path, oracle_det, name):
    """(estimate, undecided, march steps) of the model over the table tests/csrc/ceiling_host.cpp builds for the frame"""
    cfg, tiles = qc.build(name)
    p = cfg.params
    table = host._run(exe, tmp_path, tiles, p.position.latitude, p.position.longitude, p.frame.direction, p.simulation_step, p.frame.max_distance,
                      tilt=p.frame.tilt, per_cell=-4, fov=p.frame.fov, radius=qc.shape_radius(cfg), width=p.width, height=p.height)
    want = qc.oracle_frame(oracle_det, name)
    xs = mom.distance_table(p.simulation_step, p.frame.max_distance)
    assert np.array_equal(xs, table["xs"])
    est, undecided = mom.estimates(table, want["azimuth"], want["elevation_angle"], xs, qc.observer_altitude(oracle_det, cfg, tiles),
                                   mom.inv_2r(qc.shape_radius(cfg)))
    return est, undecided, len(xs) - 1


@pytest.mark.parametrize("name", qc.MODEL_FRAMES)
def test_the_model_decides_nearly_every_group(exe, tmp_path, oracle_det, name):
    """At most 1 % of a frame's groups (one group below 100) may have a decision within the model's margins, before a GPU is
    involved; and the estimates are what the frame was chosen for."""
    est, undecided, steps = host_estimates(exe, tmp_path, oracle_det, name)
    print(f"\n{name}: {est.size} groups, estimates {int(est.min())} .. {int(est.max())} of {steps} steps, {len(np.unique(est))} distinct, "
          f"{int(undecided.sum())} undecided")
    assert est.size == qc.groups(qc.build(name)[0]) and est.min() >= 1 and est.max() <= steps
    assert int(undecided.sum()) <= mom.undecided_cap(est.size), (int(undecided.sum()), est.size)
    if name in ("spline-inversion", "duct-linear", "spikes-nadir"):
        assert len(np.unique(est)) >= 4, np.unique(est)  # a sort with something to sort
    if name == "spikes-near":
        assert est.max() == 1  # a spike 100 m from the observer tops every bin's cell of step 1: every sampled ray is under it
    if name == "all-ground":
        assert est.max() <= 3  # every sampled ray is below its cell at once
    if name == "two-steps":
        assert steps == 2


def test_the_model_sees_a_slip_of_one_bin_or_row(exe, tmp_path, oracle_det):
    """Teeth: an estimate taken from the neighbouring bin, or from the row before or after, differs from the right one in more
    groups than may be undecided — the comparison with the device's estimates fails for a kernel with such a slip."""
    import ceiling_cases as cc
    name = "spline-inversion"
    cfg, tiles = qc.build(name)
    p = cfg.params
    table = host._run(exe, tmp_path, tiles, p.position.latitude, p.position.longitude, p.frame.direction, p.simulation_step, p.frame.max_distance,
                      tilt=p.frame.tilt, per_cell=-4, fov=p.frame.fov, radius=qc.shape_radius(cfg), width=p.width, height=p.height)
    want = qc.oracle_frame(oracle_det, name)
    xs = mom.distance_table(p.simulation_step, p.frame.max_distance)
    args = (want["azimuth"], want["elevation_angle"], xs, qc.observer_altitude(oracle_det, cfg, tiles), mom.inv_2r(qc.shape_radius(cfg)))
    right, undecided = mom.estimates(table, *args)
    for slip, (rows, bins) in cc.SHIFTS.items():
        slipped = dict(table, cell=cc.shifted(table["cell"], rows, bins), suffix=cc.shifted(table["suffix"], rows, bins))
        est, _ = mom.estimates(slipped, *args)
        changed = int(((est != right) & ~undecided).sum())
        print(f"{slip}: {changed} of {right.size} groups change their estimate")
        assert changed >= 5 > mom.undecided_cap(right.size), (slip, changed)
    # a flat earth's closed form (inv_2r = 0) on this curved one: another height at every step
    flat, _ = mom.estimates(table, *args[:4], 0.0)
    assert ((flat != right) & ~undecided).sum() >= 5
