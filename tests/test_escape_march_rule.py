"""From "the bound is <= 1/2 above `from`" to "the discrete RK4 march never comes down again" (DESIGN.md §7 item 6): the step the
certificate's comment argues, checked against the oracle's stepper in the det flavour — the arithmetic the kernels reproduce bit for
bit.  No device needed."""
import math
import os

import numpy as np
import pytest

import atmospheres
import escape_cases as ec
from atm_raytracer_amd import config

N_SEEDS = int(os.environ.get("ATMRT_CERTIFICATE_SEEDS", "300"))
ANGLES = [1e-9, 1e-6, 1e-3, 0.1, 1.0, 10.0, 45.0, 80.0]
REACH = 400_000.0


@pytest.fixture(scope="module")
def lib():
    return ec.load_lib()


def params(earth_shape, wavelength):
    return config.Config.from_dict({"earth_shape": earth_shape, "wavelength": wavelength, "output": {"width": 8, "height": 8}}).params


def paths(oracle, case, h0s, angles, reach, step=None):
    """The oracle's paths of every (h0, angle), cut where a sample stops being a number (T <= 0: the reference's ray ends there)."""
    step = step or case["step"]
    p = params({"Spherical": {"radius": case["radius"]}}, case["wavelength"])
    atm = config._atmosphere(case["atm"]) if case["atm"] is not None else None
    n_steps = min(int(math.ceil(reach / step)), 100_000)
    out = []
    for h0 in h0s:
        _, h = oracle.ray_paths(p, h0, angles, step, n_steps, False, atm)
        for a, row in zip(angles, h):
            bad = np.flatnonzero(~np.isfinite(row))
            out.append((h0, a, row[:bad[0]] if bad.size else row))
    return out


def test_an_ascending_ray_above_the_floor_never_comes_down(lib, oracle_det):
    """Every certified member of the directed family and 60 certified random cases: rays started at the floor and one ulp above it,
    ascending by 1e-9 .. 80 degrees, with the case's own step, out to 400 km — h[k + 1] > h[k] at every step.  No tolerance."""
    directed, random_ones = [], []
    for seed in range(N_SEEDS):
        c = ec.certificate_case(lib, seed)
        c["floor"], c["from"], c["worst"] = ec.certificate(lib, c["atm"], c["radius"], c["wavelength"], c["top"], c["step"])
        if c["family"] == "directed-in":
            directed.append(c)
        elif not c["family"].startswith("directed") and math.isfinite(c["floor"]) and c["floor"] < 1.0e6 and len(random_ones) < 60:
            random_ones.append(c)
    assert len(directed) >= N_SEEDS // 6 - 1 and len(random_ones) >= min(60, N_SEEDS // 4)
    rays = steps = 0
    for c in directed + random_ones:
        for h0, ang, h in paths(oracle_det, c, [c["floor"], math.nextafter(c["floor"], math.inf)], ANGLES, REACH):
            down = np.flatnonzero(~(h[1:] > h[:-1]))
            assert down.size == 0, (c["seed"], c["family"], h0, ang, int(down[0]), h[down[0]:down[0] + 2])
            rays += 1
            steps += len(h) - 1
    print(f"\n{len(directed)} directed and {len(random_ones)} random certified cases, {rays} rays, {steps} steps: all ascending")


def duct_twins(lib, oracle, n_seeds):
    """The directed pairs' layers again, as real ducts: the gradient for which sup g over the layer is 1.5 .. 5 (the libm oracle's)."""
    out = []
    for j in range(n_seeds // 6):
        c = ec.certificate_case(lib, 6 * j + 4)
        rng = np.random.default_rng(33_000_000 + j)
        gradient = ec.duct_gradient(oracle, c["radius"], c["wavelength"], c["at"], c["thick"], float(rng.uniform(1.5, 5.0)), c["kind"])
        c.update(gradient=gradient, atm=atmospheres.inversion(c["at"], c["thick"], gradient, c["kind"]))
        out.append(c)
    return out


def test_the_march_rule_test_can_see_a_duct(lib, oracle_det, oracle_libm):
    """Non-vacuity: the same layers with sup g = 1.5 .. 5 are refused by the certificate, and rays started inside or just under them
    at small angles do come down again in at least 90 % of them — the assertion of the test above would fire there."""
    twins = duct_twins(lib, oracle_libm, N_SEEDS)
    returning = 0
    for c in twins:
        floor, start, _ = ec.certificate(lib, c["atm"], c["radius"], c["wavelength"], c["top"], c["step"])
        if c["at"] + c["thick"] > c["top"] - c["step"] + 1.0:
            assert start > c["top"] - c["step"] and floor >= min(c["at"] + c["thick"], start) + c["step"] - 1.0, (c["seed"], floor, start)
        h0s = [float(h) for h in np.linspace(c["at"] - 100.0, c["at"] + 0.5 * c["thick"], 5)]
        step = min(max(c["step"], 20.0), 200.0)
        if any(np.any(h[1:] < h[:-1]) for _, _, h in paths(oracle_det, c, h0s, [1e-6, 1e-3, 0.01, 0.05, 0.1, 0.3], 300_000.0, step)):
            returning += 1
    print(f"\n{returning} of {len(twins)} duct twins have a ray that comes down again")
    assert returning >= 0.9 * len(twins)


def test_straight_rays_above_the_floor_and_ascending_stay_above(oracle_det):
    """Straight rays: the kernel lets a ray go when its last sample is above the floor (the mosaic's top) and above the sample before
    and — spherical — the ray's elevation angle at the start (Stepper::ang: the closed form r = r0 cos(ang) / cos(ang + x / R) keeps
    it) is below esc_ang_max = 1.5207963267948966 - max_distance / R, i.e. ang + x / R stays 0.05 rad short of 90 degrees to
    max_distance; flat: always.  Restated here from the oracle's path: whenever that holds at step k, every later sample up to
    max_distance is above the floor."""
    held = rays_held = beyond = beyond_fall = 0
    for seed in range(120):
        rng = np.random.default_rng(34_000_000 + seed)
        flat = seed % 4 == 3
        radius = float(rng.choice(ec.RADII))
        max_distance = float(rng.uniform(3_000.0, 300_000.0))
        step = float(rng.choice([rng.uniform(20.0, 100.0), rng.uniform(100.0, 1500.0)]))
        floor = float(rng.choice([1.0, rng.uniform(1.0, 9000.0), 1780.0]))
        h0 = float(rng.choice([floor + rng.uniform(-floor, 3000.0), floor + 1e-3, rng.uniform(0.0, 12_000.0)]))
        angles = np.concatenate([rng.uniform(-89.0, 89.0, 10), rng.uniform(-3.0, 3.0, 10), [0.0]])
        p = params("FlatDistorted" if flat else {"Spherical": {"radius": radius}}, 530e-9)
        n_steps = int(max_distance / step)
        x, h = oracle_det.ray_paths(p, h0, angles, step, n_steps, True)
        esc_ang_max = math.inf if flat else 1.5207963267948966 - max_distance / radius
        for a, row in zip(angles, h):
            ok = np.flatnonzero((row[1:] > floor) & (row[1:] > row[:-1])) + 1
            if not math.radians(float(a)) < esc_ang_max:  # the angle test matters: past 90 degrees the closed form comes down
                beyond += 1
                beyond_fall += bool(ok.size and np.any(~(row[int(ok[0]):] > floor)))
                continue
            if ok.size:
                rays_held += 1
                held += ok.size
                k = int(ok[0])
                low = np.flatnonzero(~(row[k:] > floor))
                assert low.size == 0, (seed, flat, radius, h0, float(a), k, int(low[0]) + k, row[k], row[int(low[0]) + k])
    print(f"\nthe straight rule held at {held} steps of {rays_held} rays; {beyond} rays were beyond esc_ang_max, {beyond_fall} of them "
          f"rose above the floor and fell below it again")
    assert rays_held >= 500 and beyond >= 30 and beyond_fall >= 1
