"""Atmosphere definitions shared by the seeded sweeps: the GPU parity sweeps (tests/test_gpu_parity.py) and the escape
certificate's sweeps (tests/test_escape_certificate.py, tests/test_gpu_escape.py) draw from these generators, so that the certificate
is checked on the same families the kernels are.  Every generator consumes its random stream exactly as the sweep it was factored
out of did: no seed of an existing sweep changes."""
import numpy as np

WGS84_A, WGS84_B = 6378137.0, 6356752.314245


def shape_radius(earth_shape):
    """The radius of the stepper's sphere (Earth::shape_radius, atmrt_core.h earth_resolve), None for the flat models."""
    if earth_shape == "SimpleSphere":
        return 6371000.0
    if earth_shape == "Wgs84":
        return (2.0 * WGS84_A + WGS84_B) / 3.0
    if isinstance(earth_shape, dict) and "Spherical" in earth_shape:
        return float(earth_shape["Spherical"]["radius"])
    if isinstance(earth_shape, dict) and "Ellipsoid" in earth_shape:
        return (2.0 * float(earth_shape["Ellipsoid"]["a"]) + float(earth_shape["Ellipsoid"]["b"])) / 3.0
    return None


def configuration_atmosphere(ra):
    """test_randomised_configurations: 1-4 Linear layers with lapse, isothermal and inversion gradients, or a Natural Spline."""
    if ra.uniform() < 0.3:
        knots = np.sort(ra.uniform(-500.0, 30_000.0, int(ra.integers(3, 7))))
        knots[0] = -500.0
        temps = 288.0 - 0.0055 * knots + ra.uniform(-6.0, 6.0, knots.size)
        first = {"Spline": {"boundary_condition": "Natural", "points": [[float(a), float(t)] for a, t in zip(knots, temps)]}}
        return {"pressure": {"altitude": 0.0, "pressure": float(ra.uniform(950.0, 1040.0)) * 100.0},
                "first_temperature_function": first}
    grads = [float(ra.choice([-0.0065, -0.0098, 0.0, 0.003, -0.002, float(ra.uniform(-0.009, 0.004))])) for _ in range(int(ra.integers(1, 5)))]
    alts = np.sort(ra.uniform(300.0, 25_000.0, len(grads) - 1))
    return {"pressure": {"altitude": float(ra.uniform(0.0, 500.0)), "pressure": float(ra.uniform(950.0, 1040.0)) * 100.0},
            "temperature_fixed_point": {"altitude": float(ra.uniform(0.0, 2000.0)), "temperature": float(ra.uniform(255.0, 305.0))},
            "first_temperature_function": {"Linear": {"gradient": grads[0]}},
            "next_functions": [{"altitude": float(a), "function": {"Linear": {"gradient": g}}} for a, g in zip(alts, grads[1:])]}


def extreme_atmosphere(rng):
    """test_randomised_extremes: Splines with every boundary condition, Linear stacks with lapse rates up to +-50 K/km, or None
    (US-76)."""
    u = rng.uniform()
    if u < 0.35:
        n_knots = int(rng.integers(2, 9))
        knots = np.sort(rng.uniform(-1000.0, 40_000.0, n_knots))
        temps = 288.0 - 0.006 * knots + rng.uniform(-15.0, 15.0, n_knots)
        bc = rng.choice(["Natural", "Derivatives", "SecondDerivatives"])
        bcv = "Natural" if bc == "Natural" else {str(bc): [float(rng.uniform(-0.01, 0.01)) if bc == "Derivatives" else float(rng.uniform(-1e-6, 1e-6)),
                                                           float(rng.uniform(-0.01, 0.01)) if bc == "Derivatives" else float(rng.uniform(-1e-6, 1e-6))]}
        return {"pressure": {"altitude": float(rng.uniform(-200.0, 3000.0)), "pressure": float(rng.uniform(300.0, 1100.0)) * 100.0},
                "first_temperature_function": {"Spline": {"boundary_condition": bcv, "points": [[float(a), float(t)] for a, t in zip(knots, temps)]}}}
    if u < 0.7:
        grads = [float(rng.choice([-0.0065, 0.0, 0.05, -0.05, -0.0342, float(rng.uniform(-0.02, 0.02)), 1e-9])) for _ in range(int(rng.integers(1, 7)))]
        alts = np.sort(rng.uniform(-500.0, 50_000.0, len(grads) - 1))
        return {"pressure": {"altitude": float(rng.uniform(-300.0, 5000.0)), "pressure": float(rng.uniform(200.0, 1100.0)) * 100.0},
                "temperature_fixed_point": {"altitude": float(rng.uniform(-300.0, 12000.0)), "temperature": float(rng.uniform(180.0, 330.0))},
                "first_temperature_function": {"Linear": {"gradient": grads[0]}},
                "next_functions": [{"altitude": float(a), "function": {"Linear": {"gradient": g}}} for a, g in zip(alts, grads[1:])]}
    return None


def long_atmosphere(rng):
    """test_randomised_long_atmospheres: 9 .. 70 temperature functions (or 1 .. 3 long ones), Linear ones and Splines of 2 .. 120
    knots mixed, thin and thick layers, lapse rates of either sign."""
    n_fn = int(rng.integers(9, 71)) if rng.uniform() < 0.7 else int(rng.integers(1, 4))
    tops = np.sort(rng.uniform(0.0, 45_000.0, n_fn - 1)) + np.arange(n_fn - 1) * 0.5
    functions, t_here = [], float(rng.uniform(270.0, 310.0))
    for j in range(n_fn):
        lo = -2000.0 if j == 0 else float(tops[j - 1])
        hi = float(tops[j]) if j < n_fn - 1 else lo + float(rng.uniform(2000.0, 30_000.0))
        if rng.uniform() < (0.25 if n_fn > 3 else 0.9):  # a Spline over (and a little beyond) this function's range
            n_k = int(rng.integers(2, 121 if n_fn <= 3 else 25))
            ks = np.sort(rng.uniform(lo - 50.0, hi + 50.0, n_k)) + np.arange(n_k) * 1e-2
            ts = np.clip(t_here - 0.005 * (ks - lo) + rng.normal(0.0, 1.0, n_k), 150.0, 340.0)
            functions.append({"Spline": {"boundary_condition": "Natural", "points": [[float(a), float(t)] for a, t in zip(ks, ts)]}})
            t_here = float(ts[-1])
        else:
            g = float(rng.choice([-0.0065, 0.0, 0.003, -0.0098, float(rng.uniform(-0.012, 0.012))]))
            functions.append({"Linear": {"gradient": g}})
            t_here = float(np.clip(t_here + g * (hi - max(lo, 0.0)), 160.0, 330.0))
    return {"pressure": {"altitude": float(rng.uniform(0.0, 1500.0)), "pressure": float(rng.uniform(700.0, 1050.0)) * 100.0},
            "temperature_fixed_point": {"altitude": float(rng.uniform(0.0, 3000.0)), "temperature": float(rng.uniform(250.0, 300.0))},
            "first_temperature_function": functions[0],
            "next_functions": [{"altitude": float(a), "function": f} for a, f in zip(tops, functions[1:])]}


# seed 4899 of test_randomised_configurations' sweep: a Natural spline through two knots 16 m apart swings below 0 K
WILD_SPLINE = {"pressure": {"altitude": 0.0, "pressure": 102390.63927278577},
               "first_temperature_function": {"Spline": {"boundary_condition": "Natural", "points": [
                   [-500.0, 295.22010975963303], [16672.2152178729, 192.93808594359285], [16688.49864235047, 195.36762037322703],
                   [21728.827855811145, 170.01112581350702], [28892.825051123004, 125.19791348512327]]}}}


# seed 31148 of the sweep: the same kind of spline, steeper — the pressure at the base of its upper knot intervals is inf / NaN.
# The reference has no check for a non-positive temperature or pressure, so neither has atmrt_set_atmosphere.
OVERFLOWING_SPLINE = {"pressure": {"altitude": 0.0, "pressure": 99730.24971796537},
                      "first_temperature_function": {"Spline": {"boundary_condition": "Natural", "points": [
                          [-500.0, 295.9785296912339], [13886.76872258016, 216.67442822116288], [13916.894125578941, 207.95894584371578],
                          [22713.29131575354, 163.34485706767265], [27617.68202733401, 130.8150959041496]]}}}


# ---- the directed family: one inversion layer in a US-76 troposphere -------------------------------------------------------------
INVERSION_KINDS = ("Linear", "Natural", "Derivatives", "SecondDerivatives")
US76_LAPSE = -0.0065


def inversion(at, thick, gradient, kind="Linear"):
    """A temperature ramp of `gradient` K/m over [at, at + thick], 288.15 K at 0 m and US-76's tropospheric lapse outside the layer:
    as three Linear functions, or as a Spline through the ramp's corners (and enough points around them to keep the rest of the
    profile close to the lapse) with the boundary condition `kind`."""
    if kind == "Linear":
        return {"pressure": {"altitude": 0.0, "pressure": 101325.0},
                "first_temperature_function": {"Linear": {"gradient": US76_LAPSE}},
                "next_functions": [{"altitude": float(at), "function": {"Linear": {"gradient": float(gradient)}}},
                                   {"altitude": float(at + thick), "function": {"Linear": {"gradient": US76_LAPSE}}}],
                "temperature_fixed_point": {"altitude": 0.0, "temperature": 288.15}}
    t_at = 288.15 + US76_LAPSE * at
    t_top = t_at + gradient * thick

    def below(h):
        return [float(h), 288.15 + US76_LAPSE * h]

    def above(h):
        return [float(h), t_top + US76_LAPSE * (h - at - thick)]

    pts = [below(-1000.0)] + [below(at - d) for d in (2000.0, 600.0, 150.0) if at - d > -900.0]
    pts += [[float(at), t_at], [float(at + thick), t_top]]
    pts += [above(at + thick + d) for d in (150.0, 600.0, 2000.0, 6000.0, 14000.0, 30000.0)]
    bc = "Natural" if kind == "Natural" else {kind: [US76_LAPSE, US76_LAPSE] if kind == "Derivatives" else [0.0, 0.0]}
    return {"pressure": {"altitude": 0.0, "pressure": 101325.0},
            "first_temperature_function": {"Spline": {"boundary_condition": bc, "points": pts}}}


def cubic_interval(at, length, d2_top):
    """US-76's tropospheric lapse below `at` and above `at + length`, and between them ONE Spline knot interval whose temperature
    is a pure cubic: boundary condition SecondDerivatives [0, d2_top] and knot temperatures chosen so that T' = 0 at `at`
    (T = T(at) + d2_top dh^3 / (6 length), T' = d2_top dh^2 / (2 length), at most d2_top length / 2 at the top).  The interval's
    linear and quadratic coefficients vanish: a bound through the coefficients rests on the cubic one alone."""
    t_at = 288.15 + US76_LAPSE * at
    return {"pressure": {"altitude": 0.0, "pressure": 101325.0},
            "temperature_fixed_point": {"altitude": 0.0, "temperature": 288.15},
            "first_temperature_function": {"Linear": {"gradient": US76_LAPSE}},
            "next_functions": [
                {"altitude": float(at), "function": {"Spline": {"boundary_condition": {"SecondDerivatives": [0.0, float(d2_top)]},
                                                                "points": [[float(at), t_at], [float(at + length), t_at + d2_top * length * length / 6.0]]}}},
                {"altitude": float(at + length), "function": {"Linear": {"gradient": US76_LAPSE}}}]}
