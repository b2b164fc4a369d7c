"""The operand populations of the GPU tests of the tight-segment shortcuts (tests/tight_populations.py), checked WITHOUT the device:
the neighbours stand at the distance the tests say they do — in exact arithmetic —, the host mirrors of atmrt_math_probe3 are the
plain operations, and the populations built to straddle a wave vote do straddle it according to the host's prediction."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import cbuild
import tight_populations as tp

N = 1 << 14  # >= 10 000 triples of every population


@pytest.fixture(scope="module")
def host():
    return C.CDLL(cbuild.dm_export())


@pytest.fixture(scope="module")
def thr_of():
    core = C.CDLL(cbuild.core_host())
    core.ch_exp_thr.restype = None

    def f(expo1, isothermal=False):
        expo1 = np.ascontiguousarray(expo1, dtype=np.float64)
        thr = np.empty_like(expo1)
        core.ch_exp_thr(C.c_void_p(expo1.ctypes.data), C.c_int(int(isothermal)), C.c_void_p(thr.ctypes.data), C.c_size_t(expo1.size))
        return thr
    return f


def assert_in_band(b0, b, num, what, slack=Fraction(1, 1 << 29)):
    """|1 - b / b0| in (num / 2^56 (1 - slack), num / 2^56], exactly."""
    for x0, x, k in zip(b0.tolist(), b.tolist(), np.broadcast_to(num, b0.shape).tolist()):
        dist, want = abs(1 - Fraction(x) / Fraction(x0)), Fraction(int(k), 1 << 56)
        assert want * (1 - slack) < dist <= want, f"{what}: {x0!r} -> {x!r} is {float(dist / want)} of the stated distance"


ALL_SETS = (("admitted", tp.ADMITTED), ("at bound", (tp.BOUND,)), ("beyond", (tp.BEYOND,)), ("2^-20", (tp.D20,)),
            ("under the vote", (tp.D20_IN,)), ("over the vote", (tp.D20_OUT,)))


def test_neighbours_stand_at_the_stated_distance_exactly():
    rng = np.random.default_rng(61)
    assert Fraction(tp.BOUND, 1 << 56) == Fraction(1, 1 << 21) * (1 + Fraction(1, 1 << 35)) and Fraction(tp.D20, 1 << 56) == Fraction(1, 1 << 20)
    assert Fraction(tp.D20_OUT, 1 << 56) == Fraction(1, 1 << 20) * (1 + Fraction(1, 1 << 10)) and Fraction(tp.D22, 1 << 56) == Fraction(1, 1 << 22)
    for site, (a, b0) in tp.division_sites(rng, N).items():
        for label, nums in ALL_SETS:
            b1, b2, n1, n2 = tp.triple(rng, b0, nums)
            # the band of the issue for the certified bound: <= 2^-21 (1 + 2^-35) and > 2^-21 (1 - 2^-30)
            slack = Fraction(1, 1 << 30) if label == "at bound" else Fraction(1, 1 << 29)
            assert_in_band(b0, b1, n1, f"{site}, {label}", slack)
            assert_in_band(b0, b2, n2, f"{site}, {label}", slack)
            if label == "at bound":
                for x0, x in zip(b0[:2000].tolist(), b1[:2000].tolist()):
                    assert abs(1 - Fraction(x) / Fraction(x0)) > Fraction(1, 1 << 21) * (1 - Fraction(1, 1 << 30))
            assert np.any((b1 > b0) != (b2 > b0)), "the two sides are chosen independently"


def test_pow_and_exp_populations_are_what_they_claim(host, thr_of):
    rng = np.random.default_rng(62)
    for label, nums in ALL_SETS[:4]:
        y, x0, x1, x2, n1, n2, special = tp.pow_population(rng, N, [5000.0, -5000.0, 6000.0], thr_of, nums=nums)
        assert x0.size % tp.WAVE == 0 and x0.size >= 10_000 and np.all((x0 > 0.25) & (x0 < 2.0))
        assert np.all(np.abs(y * np.log(x0)) < 640.0), "inside what atm_interval_certified admits for exp's main branch"
        assert_in_band(x0, x1, n1, f"pow, {label}")
        assert_in_band(x0, x2, n2, f"pow, {label}")
    # the last high words that pass the shared log's vote, with the neighbour across the interval's edge
    x0, up = tp.log_edge_bases(rng, N, tp.LOG_EDGE_PASS)
    hi0 = (x0.view(np.uint64) >> np.uint64(32)).astype(np.int64)
    assert set(((hi0 + 0x1000) & 0x1fff).tolist()) == set(tp.LOG_EDGE_PASS)
    hi1 = (tp.neighbour(x0, up, tp.BOUND).view(np.uint64) >> np.uint64(32)).astype(np.int64)
    assert np.all(np.abs(hi1 - hi0) <= 1), "2^-21 (1 + 2^-35) moves the high word by at most one unit"
    centre = lambda hi: (hi + 0x1000) & ~0x1fff  # noqa: E731
    assert np.all(centre(hi1) == centre(hi0)), "... so a centre that passes the vote shares its table row with its neighbours"
    far = (tp.neighbour(x0, up, tp.D20).view(np.uint64) >> np.uint64(32)).astype(np.int64)
    assert np.any(centre(far) != centre(hi0)), "at 2^-20 it does not: what the certificate is for"
    # the isothermal population: |d_i - d_0| is 1 cm up to the roundings of h -+ eps and of the subtraction of hb (half a unit of a
    # value below 2^17 m and twice half a unit of one below 2^15 m: 1.1e-11 m) — inside the 1.01 x 0.01 (1 + 1e-9) m of exp_thr's margin
    a, d0, d1, d2, special = tp.exp_population(rng, N, [-0.25], lambda v: thr_of(v, True))
    lo_lim, hi_lim = Fraction(0.01) - Fraction(11, 10 ** 12), Fraction(0.01) + Fraction(11, 10 ** 12)
    assert hi_lim < Fraction(0.01) * Fraction(101, 100)
    for c, lo, hi in zip(d0.tolist(), d1.tolist(), d2.tolist()):
        assert lo_lim <= Fraction(c) - Fraction(lo) <= hi_lim and lo_lim <= Fraction(hi) - Fraction(c) <= hi_lim
    assert np.all(np.abs(a * d0) < 640.0) and a.size >= 10_000


def test_host_mirrors_are_the_plain_operations_and_the_populations_straddle_the_votes(host, thr_of):
    rng = np.random.default_rng(63)

    def call(name, *arrs):
        arrs = [np.ascontiguousarray(x, dtype=np.float64) for x in arrs]
        res = [np.empty_like(arrs[0]) for _ in range(3)]
        fn = getattr(host, name)
        fn.restype = None
        fn(*[C.c_void_p(x.ctypes.data) for x in arrs + res], C.c_size_t(arrs[0].size))
        return res

    def votes(a, b0, thr, isothermal):
        log_ok, exp_ok = np.empty(a.size, dtype=np.int32), np.empty(a.size, dtype=np.int32)
        host.t_vote3.restype = None
        host.t_vote3(*[C.c_void_p(np.ascontiguousarray(x).ctypes.data) for x in (a, b0, thr)], C.c_int(int(isothermal)),
                     C.c_void_p(log_ok.ctypes.data), C.c_void_p(exp_ok.ctypes.data), C.c_size_t(a.size))
        return (log_ok != 0).reshape(-1, tp.WAVE).all(axis=1), (exp_ok != 0).reshape(-1, tp.WAVE).all(axis=1)

    for site, (a, b0) in tp.division_sites(rng, N).items():
        b1, b2, _, _ = tp.triple(rng, b0, tp.ADMITTED + (tp.D20,))
        with np.errstate(all="ignore"):
            for got, b in zip(call("t_div3x", a, b0, b1, b2), (b0, b1, b2)):
                assert np.array_equal(got.view(np.uint64), (a / b).view(np.uint64)), site
    y, x0, x1, x2, _, _, special = tp.pow_population(rng, 1 << 16, [5000.0, -5000.0, 6000.0], thr_of)
    log_w, exp_w = votes(y, x0, thr_of(y), False)
    own = special.reshape(-1, tp.WAVE).all(axis=1)
    for w in (log_w, exp_w):
        for sel in (own, ~own):
            assert 0 < int(w[sel].sum()) < int(sel.sum()), "both paths in the edge wavefronts and in the mixed ones"
    got = call("t_pow3x", y, x0, x1, x2)
    with np.errstate(all="ignore"):
        assert np.allclose(got[1], x1 ** y, rtol=1e-13) and np.allclose(got[2], x2 ** y, rtol=1e-13)
    a, d0, d1, d2, special = tp.exp_population(rng, 1 << 16, [-0.25, -0.3], lambda v: thr_of(v, True))
    _, exp_w = votes(a, d0, thr_of(a, True), True)
    own = special.reshape(-1, tp.WAVE).all(axis=1)
    for sel in (own, ~own):
        assert 0 < int(exp_w[sel].sum()) < int(sel.sum())
    got = call("t_exp3x", a, d0, d1, d2)
    assert np.allclose(got[0], np.exp(a * d0), rtol=1e-14) and np.allclose(got[2], np.exp(a * d2), rtol=1e-14)
