"""The escape certificate (atmrt_api.hip escape_floor) through its host entry point
atmrt_escape_certificate: no device needed.  out[0] = the floor above which an ascending ray may leave the march, out[1] = the
lowest altitude from which (R + h) |n'| / n <= 1/2 holds everywhere above, out[2] = the largest bound above it."""
import ctypes as C
import math

import pytest

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
