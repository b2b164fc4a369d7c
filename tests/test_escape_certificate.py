"""The escape certificate (atmrt_api.hip escape_floor) through its host entry point
atmrt_escape_certificate: no device needed.  out[0] = the floor above which an ascending ray may leave the march, out[1] = the
lowest altitude from which (R + h) |n'| / n <= 1/2 holds everywhere above, out[2] = the largest bound above it."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import atmospheres
import escape_cases as ec
from atm_raytracer_amd import _lib, config

R = 6_371_000.0
TOP = 1780.0  # the headline mosaic's top + 1 m
STEP = 100.0


@pytest.fixture(scope="module")
def lib():
    if not __import__("os").path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def cert(lib, atm, spherical=1, straight=0, top=TOP, step=STEP):
    out = (C.c_double * 3)()
    assert lib.atmrt_escape_certificate(C.byref(atm), 530e-9, spherical, R, straight, step, top, out) == 0
    return tuple(out)


def linear_with_inversion(at, thick, gradient):
    return config._atmosphere({"pressure": {"altitude": 0.0, "pressure": 101325.0},
                               "first_temperature_function": {"Linear": {"gradient": -0.0065}},
                               "next_functions": [{"altitude": at, "function": {"Linear": {"gradient": gradient}}},
                                                  {"altitude": at + thick, "function": {"Linear": {"gradient": -0.0065}}}],
                               "temperature_fixed_point": {"altitude": 0.0, "temperature": 288.15}})


def spline(points):
    return config._atmosphere({"pressure": {"altitude": 0.0, "pressure": 101325.0},
                               "first_temperature_function": {"Spline": {"points": points}}})


def test_us76_is_certified_for_the_headline(lib):
    floor, start, worst = cert(lib, config.us76())
    assert floor == TOP and start == TOP - STEP
    assert 0.1 < worst <= 0.5  # US-76 near the ground: (R + h) |n'| / n ~ 0.15-0.2


def test_a_strong_low_inversion_above_the_mosaic_is_refused(lib):
    # 0.12 K/m over 400 m at 2.5 km: dn/dh well below -1/R (a duct)
    floor, start, _ = cert(lib, linear_with_inversion(2500.0, 400.0, 0.12))
    assert start >= 2900.0 - 1.0 and floor >= start + STEP  # not certified from the mosaic's top: the floor moves above the duct
    assert floor > TOP
    # a mild one passes
    assert cert(lib, linear_with_inversion(2500.0, 400.0, 0.01))[0] == TOP


def test_flat_earth_refraction_is_refused_and_straight_rays_are_accepted(lib):
    assert math.isinf(cert(lib, config.us76(), spherical=0)[0])
    assert cert(lib, config.us76(), spherical=0, straight=1)[0] == TOP
    assert cert(lib, config.us76(), spherical=1, straight=1)[0] == TOP
    assert cert(lib, linear_with_inversion(2500.0, 400.0, 0.12), straight=1)[0] == TOP  # the atmosphere does not bend them


def _spline_with_bump(slope):
    # a Spline through a temperature ramp of `slope` K/m between 3 and 3.2 km, US-76-like elsewhere
    pts = [[0.0, 288.15], [2000.0, 275.15], [3000.0, 268.65], [3200.0, 268.65 + 200.0 * slope], [5000.0, 268.65 + 200.0 * slope - 11.7],
           [11000.0, 216.65], [20000.0, 216.65], [30000.0, 226.65], [80000.0, 196.65]]
    return spline(pts)


def test_spline_atmospheres_fall_on_the_right_side_of_the_bound(lib):
    # the bound grows with the ramp's slope (the spline's overshoot around the ramp too): a gentle one stays inside 1/2 from the
    # mosaic's top up, a steeper one does not and moves the floor above the ramp
    f_in, s_in, w_in = cert(lib, _spline_with_bump(0.005))
    f_out, s_out, _ = cert(lib, _spline_with_bump(0.02))
    assert f_in == TOP and s_in == TOP - STEP and 0.3 < w_in <= 0.5
    assert s_out > 3200.0 and f_out > TOP


# ---- the certificate against an independent n(h): the libm oracle and mpmath ------------------------------------------------------
N_SEEDS = int(os.environ.get("ATMRT_CERTIFICATE_SEEDS", "300"))
# worst / sup g of the parent commit's certificate times 1.5: see test_refusals_are_for_a_reason
SLACK = {False: 1.0578 * 1.5, True: 113.5 * 1.5}
THIN_AIR = 2.0e-6  # n - 1 of US-76 at about 35 km


@pytest.fixture(scope="module")
def sweep(lib, oracle_libm):
    """Every case of the sweep with its certificate and the oracle's g."""
    out = []
    for seed in range(N_SEEDS):
        c = ec.certificate_case(lib, seed)
        c["floor"], c["from"], c["worst"] = ec.certificate(lib, c["atm"], c["radius"], c["wavelength"], c["top"], c["step"])
        c["g"] = ec.G(oracle_libm, c["atm"], c["radius"], c["wavelength"])
        out.append(c)
    return out


def test_the_directed_family_lands_on_both_sides_of_the_bound(sweep):
    """The generator's own condition: the certified member of every pair has its bound in [0.40, 0.50] and is certified from
    top - step up; its twin, 2^-40 of the bracket steeper, is refused."""
    pairs = [c for c in sweep if c["family"] == "directed-in"]
    assert len(pairs) >= N_SEEDS // 6 - 1
    for c in sweep:
        if c["family"] == "directed-in":
            assert c["from"] == c["top"] - c["step"] and 0.40 <= c["worst"] <= 0.50, (c["seed"], c["from"], c["worst"])
        elif c["family"] == "directed-out":
            assert c["from"] > c["top"] - c["step"], c["seed"]


def test_soundness_against_the_libm_oracle(sweep):
    """Where the certificate gives a finite `from`, the oracle's g(h) = (R + h) |dn| / n stays below `worst` <= 1/2 at every sample
    above it (escape_cases.sup_g: boundaries and knots with their +-1 cm surroundings, 200 points per segment, a golden-section search
    on every Spline knot interval, 50 points of the tail).  No tolerance on worst <= 1/2; on g <= worst the rounding of the sample.

    Found by this sweep and fixed in the certificate: seed 133 (a Linear gradient of 1e-9 K/m: the rounding of T / tb, raised to the
    power 3.4e7, moves the computed n by 1e-12 and the central difference by 4e-4 of its value: the bound now carries that term) and
    seed 206 (a stencil centred within 1 cm above a refused piece still reaches into it: `from` is now 2 cm above the piece)."""
    ratios = {False: (0.0, None), True: (0.0, None)}
    finite = top = 0
    for c in sweep:
        if not math.isfinite(c["from"]):
            continue
        finite += 1
        top += c["from"] == c["top"] - c["step"]
        g = c["g"]
        assert c["worst"] <= 0.5, (c["seed"], c["worst"])
        sup, where, _ = ec.sup_g(g, c["from"])
        assert where is None or sup <= c["worst"] + g.tol(where), (c["seed"], c["family"], where, sup, c["worst"])
        spline = any(g.cubic[k] for k in range(g.segment_of(c["from"]), len(g.cubic)))
        if sup > 0.0 and c["worst"] / sup > ratios[spline][0]:
            ratios[spline] = (c["worst"] / sup, c["seed"])
    # the slack may not grow past what the refusal test grants it
    assert ratios[False][0] <= SLACK[False] and ratios[True][0] <= SLACK[True], ratios
    print(f"\nseeds {len(sweep)}: finite from {finite}, certified from the top {top}, refused {len(sweep) - top}; largest worst / sup g: "
          f"Linear {ratios[False][0]:.4f} (seed {ratios[False][1]}), Spline {ratios[True][0]:.1f} (seed {ratios[True][1]})")
    assert top >= len(sweep) // 4  # the sweep is not all refusals


@pytest.mark.parametrize("name,seed", [("near-isothermal-gradient", 133), ("stencil-above-a-refused-piece", 206)])
def test_regressions_of_the_soundness_sweep(lib, oracle_libm, name, seed):
    c = ec.certificate_case(lib, seed)
    _, start, worst = ec.certificate(lib, c["atm"], c["radius"], c["wavelength"], c["top"], c["step"])
    g = ec.G(oracle_libm, c["atm"], c["radius"], c["wavelength"])
    sup, where, _ = ec.sup_g(g, start)
    assert math.isfinite(start) and worst <= 0.5 and sup <= worst + g.tol(where), (name, where, sup, worst)


def _analytic_g(env, k, radius, h):
    """(R + h) |n'(h)| / n(h) of the Linear or isothermal segment k in 50-digit arithmetic, n' differentiated analytically:
    pt = (pb / tb) x^(expo - 1), x = 1 + lapse (h - hb) / tb (isothermal: (pb / tb) exp(expo (h - hb))), Z = 1 - pt A(t) + pt^2 d."""
    import mpmath
    mp = mpmath.mpf
    a0, a1, a2, d = (mp(v) for v in ("1.58123e-6", "-2.9331e-8", "1.1043e-10", "1.83e-11"))
    hb, tb, pb, lapse, expo = (mp(float(v[k])) for v in (env.hb, env.tb, env.pb, env.lapse, env.expo))
    dh = mp(h) - hb
    if lapse != 0:
        x = 1 + lapse / tb * dh
        if x <= 0:
            return None
        pt = pb / tb * x ** (expo - 1)
        dpt = pt * (expo - 1) * (lapse / tb) / x
    else:
        x = mp(1)
        pt = pb / tb * mpmath.exp(expo * dh)
        dpt = pt * expo
    t = tb * x - mp("273.15")
    a, da = a0 + a1 * t + a2 * t * t, (a1 + 2 * a2 * t) * lapse
    z = 1 - pt * a + pt * pt * d
    dz = -dpt * a - pt * da + 2 * pt * dpt * d
    k_refr = mp(env.k_refr)
    n, dn = 1 + k_refr * pt / z, k_refr * (dpt / z - pt * dz / (z * z))
    return float((mp(radius) + mp(h)) * abs(dn) / n)


def test_soundness_against_mpmath_on_the_directed_linear_family(sweep):
    """The analytic (R + h) |n'| / n of every Linear segment above `from`, in 50 digits, stays below `worst` as well: the oracle's
    central difference hides nothing the bound is meant to cover."""
    import mpmath
    mpmath.mp.dps = 50
    checked = 0
    for c in sweep:
        if c["kind"] != "Linear" or not math.isfinite(c["from"]):
            continue
        g = c["g"]
        for k, pts in ec.samples_above(g, c["from"]):
            assert not g.cubic[k]
            for h in pts[::4] + pts[-1:]:
                v = _analytic_g(g.env, k, c["radius"], h)
                assert v is None or v <= c["worst"], (c["seed"], k, h, v, c["worst"])
                checked += 1
    assert checked > 1000


def test_refusals_are_for_a_reason(sweep):
    """Where the certificate moves `from` above top - step, the piece it refused last ([from - L, from], L = 50 m + 2 % of the height
    above the segment's lower boundary, above 0 m in the first segment: the certificate's lattice) shows why in the oracle: g above
    0.5 / S of the piece's segment kind, or, inside the piece, an n that is not a finite number above 1 (a temperature <= 0, Ciddor's
    compressibility outside its range).  `from` = +inf: a non-finite n somewhere above top - step.

    S, the certificate's slack: the largest worst / sup g (sup g from the libm oracle) over the sweep's cases with a finite `from`,
    measured with the certificate of the parent commit, times 1.5 for seeds beyond the default range: 1.0578 (seed 5, the linear
    continuation of WILD_SPLINE) where no Spline knot interval lies above `from`, 113.5 (seed 14, a knot interval bounded through
    its coefficients in air that hardly refracts) where one does.  The certificate as it is now gives 1.0551 (seed 5) and 19.5
    (seed 164); test_soundness_against_the_libm_oracle fails if either passes S.

    Excluded by stated rules, together at most 5 % of the seeds, since the oracle shows nothing there and the
    refusal only costs speed: (1) a refused piece inside a Spline knot interval where n - 1 < 2e-6 over the whole piece (thinner
    than US-76 at 35 km): the temperature bound comes from the coefficients over the whole interval and can reach 0 K where the
    spline does not; (2) a Linear segment whose gradient is so small that one rounding of T / tb (2^-53) raised to the segment's
    exponent could move n by 0.5 / S of n - 1 across the stencil (gradients below about 1e-12 K/m): the certificate charges the
    worst case of that rounding although the computed n may be constant; (3) `from` = +inf without a non-finite n, where the last
    segment is outside the tail rule's stated domain (a Spline, a Linear one cooling without reaching 0 K below 1e7 m, a warming
    one with exponent >= -1)."""
    excluded = {"thin-air": [], "rounding": [], "tail-domain": []}
    refused, reasons = 0, {"g": 0, "nan": 0}
    for c in sweep:
        g, lo, start = c["g"], c["top"] - c["step"], c["from"]
        if start == lo:
            continue
        refused += 1
        if not math.isfinite(start):
            k = len(g.edges)
            if any(not math.isfinite(g(float(h))) for h in np.geomspace(max(lo, 1.0), 1.0e9, 3000)):
                reasons["nan"] += 1
                continue
            lapse, expo = float(g.env.lapse[k]), float(g.env.expo[k])
            reaches_zero = lapse < 0.0 and float(g.env.hb[k]) - float(g.env.tb[k]) / lapse < ec.H_END
            assert g.cubic[k] or (lapse < 0.0 and not reaches_zero) or (lapse > 0.0 and expo - 1.0 >= -1.0), (c["seed"], "from = +inf without a reason")
            excluded["tail-domain"].append(c["seed"])
            continue
        end = start - 0.02  # `from` is 2 cm above the refused piece
        k = g.segment_of(math.nextafter(end, -math.inf))
        length = 50.0 + 0.02 * max(end - (g.bounds(k)[0] if k > 0 else 0.0), 0.0)
        a = max(end - length, g.bounds(k)[0])
        hs = [float(h) for h in np.linspace(a, end, 400)] + [h for h in ec.around(end) + ec.around(a) if a - 0.02 <= h <= end + 0.02]
        vals = [g(h) for h in hs]
        ns = [g._n(g._ref, h) for h in hs]
        if any(not math.isfinite(v) for v in vals) or any(not n >= 1.0 for n in ns):
            reasons["nan"] += 1
        elif max(vals) > 0.5 / SLACK[g.cubic[k]]:
            reasons["g"] += 1
        elif not g.cubic[k] and (c["radius"] + end) * 100.0 * (max(ns) - 1.0) * abs(float(g.env.expo[k]) - 1.0) * 2.0 ** -53 > 0.5 / SLACK[False]:
            excluded["rounding"].append(c["seed"])
        elif g.cubic[k] and max(ns) - 1.0 < THIN_AIR:
            excluded["thin-air"].append(c["seed"])
        else:
            raise AssertionError((c["seed"], c["family"], "refused at", start, "largest g in the piece", max(vals), "Spline" if g.cubic[k] else "Linear"))
    print(f"\nrefused {refused} of {len(sweep)}: {reasons}, excluded {excluded}")
    assert sum(len(v) for v in excluded.values()) <= 0.05 * len(sweep), excluded
    assert reasons["g"] >= len(sweep) // 6  # the twins at least
    assert reasons["g"] + reasons["nan"] >= 0.9 * refused


@pytest.mark.parametrize("length", [8.0, 16.0, 40.0])
@pytest.mark.parametrize("radius", ec.DIRECTED_RADII)
def test_a_spline_interval_that_rests_on_its_cubic_coefficient(lib, oracle_libm, radius, length):
    """The Spline branch of the bound where its third-order term decides: one knot interval 8 .. 40 m long, 50 m above the top,
    whose temperature is a pure cubic (atmospheres.cubic_interval: no linear, no quadratic coefficient), US-76's lapse around it.
    Its curvature is bisected against the ORACLE until sup g over the interval is 0.40, and for the twin 0.55.  The first must be
    certified from top - step with g <= worst <= 1.10 sup g; the twin must be refused up to the interval's top.  A coefficient
    bound without the cubic term leaves worst at the troposphere's 0.09 .. 0.18 and fails both.

    1.10: with all three coefficients of one sign the coefficient bound of T' is exact at the interval's top, where the
    hydrostatic term is largest too; what is left is the piece's temperature bound T(u) - max|T'| (v - u) and the pressure at u
    in place of the values at the top (under 1 % each over 40 m), the centimetre added at both ends and (R + h): a few per cent.
    And 0.40 x 1.25 = 1/2: a bound slacker than 1.25 would refuse the first case outright."""
    at = TOP + 50.0

    def case(target):
        def sup(d2):
            g = ec.G(oracle_libm, atmospheres.cubic_interval(at, length, d2), radius, 530e-9)
            return max(g(float(h)) for h in np.linspace(at, at + length, 81))
        lo, hi = 0.0, 1.0
        for _ in range(40):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if sup(mid) < target else (lo, mid)
        return atmospheres.cubic_interval(at, length, hi)

    atm = case(0.40)
    g = ec.G(oracle_libm, atm, radius, 530e-9)
    k = g.segment_of(at + 0.5 * length)
    assert g.cubic[k] and abs(float(g.env.lapse[k])) < 1e-12 and float(g.env.c2[k]) == 0.0 and float(g.env.c3[k]) > 0.0
    floor, start, worst = ec.certificate(lib, atm, radius, 530e-9, TOP, STEP)
    sup, where, _ = ec.sup_g(g, TOP - STEP)
    assert at <= where <= at + length + 0.02 and 0.40 <= sup < 0.42, (where, sup)
    assert start == TOP - STEP and floor == TOP, (start, floor, worst, sup)
    assert sup <= worst + g.tol(where) and worst <= 1.10 * sup, (worst, sup, worst / sup)
    twin = case(0.55)
    _, start, _ = ec.certificate(lib, twin, radius, 530e-9, TOP, STEP)
    assert at + length <= start <= at + length + 0.03, start


def test_the_floor_is_monotone_where_it_must_be(sweep, lib):
    for c in sweep:
        args = (lib, c["atm"], c["radius"], c["wavelength"])
        floor, start = c["floor"], c["from"]
        assert floor >= c["top"] and floor >= start + c["step"], c["seed"]
        prev = floor
        for raised in sorted((c["top"] + 0.37, c["top"] + c["step"], c["top"] * 2.0 + 300.0, c["top"] + 25_000.0)):
            f = ec.certificate(*args, raised, c["step"])[0]
            assert f >= prev and f >= raised, (c["seed"], raised, f, prev)
            prev = f
        assert ec.certificate(*args, c["top"], c["step"], spherical=1, straight=1)[0] == c["top"]
        assert ec.certificate(*args, c["top"], c["step"], spherical=0, straight=1)[0] == c["top"]
        assert ec.certificate(*args, c["top"], c["step"], spherical=0, straight=0)[0] == math.inf
