"""Operand triples for the three-point math forms of a TIGHT atmosphere segment (atmrt_math_probe3, tests/test_gpu_detmath.py):
a centre operand and two neighbours whose relative distance from it is EXACT — built in integer arithmetic on the significands, the
largest distance not above the stated one — so that a test of the certified bound 2^-21 (1 + 2^-35) runs at that bound and not at
a decimal literal near it.  tests/test_tight_populations.py checks the distances with fractions.Fraction, without a GPU."""
import numpy as np

U = np.uint64
# distances as num / 2^56
D22 = 1 << 34                     # 2^-22: where the fixed-neighbour probes (atmrt_math_probe) stand
D21_99 = round(0.99 * (1 << 35))  # 0.99 2^-21: what a dense sample of a standard atmosphere reaches (max_dt_rel)
D21 = 1 << 35                     # 2^-21
BOUND = (1 << 35) + 1             # 2^-21 (1 + 2^-35): what atm_interval_tight admits
BEYOND = (1 << 35) + (1 << 5)     # 2^-21 (1 + 2^-30)
D20 = 1 << 36                     # 2^-20: the seed tolerance the comments claim, and dm_div3's vote threshold
D20_IN = (1 << 36) - (1 << 26)    # 2^-20 (1 - 2^-10)
D20_OUT = (1 << 36) + (1 << 26)   # 2^-20 (1 + 2^-10)
ADMITTED = (D22, D21_99, D21, BOUND)
WAVE = 64


def neighbour(b0, up, num):
    """The double on the `up` side of b0 (away from zero where up, towards it elsewhere) farthest from it with
    |1 - b / b0| <= num / 2^56; num < 2^37 (an integer or an array of them), b0 finite, normal and non-zero."""
    b0 = np.asarray(b0, dtype=np.float64)
    num = np.broadcast_to(np.asarray(num, dtype=U), b0.shape)
    fr, e = np.frexp(np.abs(b0))
    m0 = np.ldexp(fr, 53).astype(U)  # 2^52 <= m0 < 2^53, exact
    e = e - 53
    # k = floor(m0 num / 2^56) without leaving 64 bits: m0 = mh 2^27 + ml
    k = (((m0 >> U(27)) * num) + (((m0 & U((1 << 27) - 1)) * num) >> U(27))) >> U(29)
    m1 = np.where(up, m0 + k, m0 - k)
    over, under = m1 >= U(1 << 53), m1 < U(1 << 52)
    m1 = np.where(over, m1 >> U(1), np.where(under, m1 << U(1), m1))  # the next binade: half as fine (floor: still inside) / twice as fine
    return np.copysign(np.ldexp(m1.astype(np.float64), e + over.astype(np.int64) - under.astype(np.int64)), b0)


def triple(rng, b0, nums, up1=None, up2=None):
    """(b1, b2, num1, num2): each outer point gets its distance (one of nums) and its side independently of the other."""
    nums = np.asarray(nums, dtype=U)
    n1, n2 = rng.choice(nums, b0.size), rng.choice(nums, b0.size)
    up1 = rng.uniform(size=b0.size) < 0.5 if up1 is None else up1
    up2 = rng.uniform(size=b0.size) < 0.5 if up2 is None else up2
    return neighbour(b0, up1, n1), neighbour(b0, up2, n2), n1, n2


def mantissa(rng, n):
    return rng.uniform(1.0, 2.0, n) * rng.choice([-1.0, 1.0], n)


def in_range_pairs(rng, n, lim=480):
    """(a, b) with the binary exponents of a, b, a/b and 1/b all within +-lim, a quarter of them AT the limits."""
    eb = rng.integers(-lim + 1, lim, n)
    eq = rng.integers(-lim + 1, lim, n)
    edge = rng.uniform(size=n) < 0.25
    eb = np.where(edge, rng.choice([-lim + 1, lim - 1], n), eb)
    eq = np.where(edge & (rng.uniform(size=n) < 0.5), rng.choice([-lim + 2, lim - 2], n), eq)
    ea = np.clip(eb + eq, -lim + 1, lim - 1)
    b = np.ldexp(mantissa(rng, n), eb)
    a = np.ldexp(mantissa(rng, n), ea)
    q = np.abs(a / b)
    ok = (q > 2.0 ** -lim) & (q < 2.0 ** lim)
    a = np.where(ok, a, b * 1.5)
    a[:64] = 0.0  # a may be +0
    return a, b


SEED_Z = 6.9053396600248786e-04  # 2^-10.5: the certified bound of |1 - Z|


def division_sites(rng, n):
    """{name: (a, b0)}: the call sites' own operands and the whole exponent range."""
    z = 1.0 - rng.uniform(-SEED_Z, SEED_Z, n)
    z[: n // 8] = 1.0 - rng.choice([SEED_Z, -SEED_Z, 0.0, 2.0 ** -30, -(2.0 ** -30), 2.0 ** -52, -(2.0 ** -53), 4.0e-4], n // 8)
    return {"p / T": (rng.uniform(100.0, 115000.0, n), rng.uniform(150.0, 330.0, n)),
            "K pt / Z": (rng.uniform(1e-7, 3e-4, n), z),
            "exponent range": in_range_pairs(rng, n)}


def mix_into_wavefronts(rng, special, ordinary):
    """The mask of the special elements of a population that begins with `special` of them in wavefronts of their own and goes on
    with `ordinary` others, ONE special lane in each of their wavefronts."""
    n = ordinary - ordinary % WAVE
    own = special - special % WAVE
    is_special = np.zeros(own + n, dtype=bool)
    is_special[:own] = True
    lanes = own + np.arange(0, n, WAVE) + rng.integers(0, WAVE, n // WAVE)
    is_special[lanes] = True
    return is_special


# ---- pow: x = T / T_b of a Linear segment, y = expo1 --------------------------------------------------------------------------
PHYSICAL_EXPO = (5.2558761132785179, -17.08, 34.163, -3.4e-4 * 288.0, 1.0, -11.388)
LOG_EDGE_PASS = (1, 2, 0x1ffd, 0x1ffe)  # (hi + 0x1000) & 0x1fff: the last values on which dm_log3_core_pow_shared's vote passes
LOG_EDGE_FAIL = (0, 0x1fff)             # ... and the two on which it fails


def log_edge_bases(rng, n, vals):
    """Bases whose high word sits at the given places of a log table interval, in the binades of 0.25 .. 2; low words 0, 1,
    2^32 - 1 and random.  Returns (x0, up1): up1 is the side on which a neighbour crosses into the next table interval."""
    val = rng.choice(np.asarray(vals, dtype=np.int64), n)
    hi = (0x3fd00000 + rng.integers(1, 0x300000 // 0x2000, n) * 0x2000 - 0x1000 + val).astype(U)
    lo = rng.integers(0, 2 ** 32, n).astype(U)
    lo[::2] = rng.choice(np.array([0, 1, 2 ** 32 - 1], dtype=U), lo[::2].size)
    return ((hi << U(32)) | lo).view(np.float64), val >= 0x1000


def binade_edge_bases(rng, n):
    """Bases a few units above 1.0 and 0.5 and below 2.0 and 1.0: a neighbour at the admitted distance lies in the other binade,
    where a unit of the high word is twice or half as large."""
    base = rng.choice(np.array([0x3ff0000000000000, 0x3fe0000000000000], dtype=U), n)
    above = base + rng.choice(np.array([0, 1, 2, 2 ** 31, 2 ** 32, 2 ** 33 + 5], dtype=U), n)
    below = rng.choice(np.array([0x4000000000000000, 0x3ff0000000000000], dtype=U), n) - rng.choice(np.array([1, 2, 2 ** 31, 2 ** 32, 2 ** 32 + 1], dtype=U), n)
    up = rng.uniform(size=n) < 0.5
    return np.where(up, below, above).view(np.float64), up


def hair(rng, thr, inside):
    """Offsets from a half-integer t = k + 1/2 that put k + 1/2 + offset a hair from one of the two places where
    dm_exp3_main_shared's vote |t - rint(t)| <= thr flips: where `inside`, 1e-8 .. 1e-6 on the passing side (beyond the rounding of
    the operand that will carry it); elsewhere 1e-13 .. 1e-6 on the failing side (the smallest ones: whichever side rounding gives)."""
    s = rng.choice([-1.0, 1.0], thr.size)
    mag = 10.0 ** np.where(inside, rng.uniform(-8, -6, thr.size), rng.uniform(-13, -6, thr.size))
    return s * (0.5 - np.maximum(thr, 0.0)) + np.where(inside, s, -s) * mag


def per_wavefront(rng, n, draw):
    """draw(number of wavefronts) repeated over the lanes of each wavefront"""
    return np.repeat(draw(n // WAVE), WAVE)


def half_integer_bases(rng, y, thr, inside, max_e):
    """Bases x with y log x a hair() from the places where the shared exp's vote flips, (k + 1/2 -+ margin) ln2 / 128."""
    invln2n = 184.6649652337873
    n = y.size
    kmax = np.maximum(1, np.minimum(60000, np.floor(max_e * invln2n) - 2)).astype(np.int64)
    k = rng.integers(-kmax, kmax + 1, n)
    e = (k + 0.5 + hair(rng, thr, inside)) / invln2n
    with np.errstate(all="ignore"):
        x = np.exp(e / y)
    bad = ~((x > 0.26) & (x < 1.95))  # outside T / T_b of any segment: the barometric population instead
    x[bad] = rng.uniform(0.72, 1.39, int(bad.sum()))
    return x


def pow_population(rng, n, y_special, thr_of, nums=ADMITTED):
    """(y, x0, x1, x2, num1, num2, is_special): barometric bases, and — in wavefronts of their own and one per ordinary wavefront —
    bases at the edges of the log table, at the binade edges and at the half-integers of exp's reduction.  thr_of(y) -> exp_thr."""
    is_special = mix_into_wavefronts(rng, n // 2, n - n // 2)
    n = is_special.size
    y = rng.choice(np.asarray(PHYSICAL_EXPO), n)
    x0 = rng.uniform(0.72, 1.39, n)
    up1 = rng.uniform(size=n) < 0.5
    # One kind, one special exponent and one side of the exp threshold per wavefront (in the mixed part: of its special lane), so
    # that a lane that fails a vote does not hide the lanes beside it that pass.  0: the last high words that pass the log vote;
    # 1: those that fail it; 2: binade edges; 3: half-integers of exp's reduction with physical exponents; 4: with y_special
    kind = per_wavefront(rng, n, lambda w: rng.integers(0, 5, w))
    y_sp = per_wavefront(rng, n, lambda w: rng.choice(np.asarray(y_special, dtype=np.float64), w))
    inside = per_wavefront(rng, n, lambda w: rng.uniform(size=w) < 0.5)
    for kd, vals in ((0, LOG_EDGE_PASS), (1, LOG_EDGE_FAIL)):
        idx = np.flatnonzero(is_special & (kind == kd))
        x0[idx], up1[idx] = log_edge_bases(rng, idx.size, vals)
    idx = np.flatnonzero(is_special & (kind == 2))
    x0[idx], up1[idx] = binade_edge_bases(rng, idx.size)
    idx = np.flatnonzero(is_special & (kind == 4))
    y[idx] = y_sp[idx]
    idx = np.flatnonzero(is_special & (kind >= 3))
    # |y log x| <= 600 and |log x| <= 0.6
    x0[idx] = half_integer_bases(rng, y[idx], thr_of(y[idx]), inside[idx], np.minimum(600.0, np.abs(y[idx]) * 0.6))
    x1, x2, n1, n2 = triple(rng, x0, nums, up1=up1)
    # the crossing side at the FULL distance of the set
    full = is_special & (rng.uniform(size=n) < 0.75)
    x1[full] = neighbour(x0[full], up1[full], max(nums))
    n1[full] = max(nums)
    return y, x0, x1, x2, n1, n2, is_special


# ---- exp: an isothermal segment, e_i = expo1 (h_i - hb) -------------------------------------------------------------------------
GMR = 9.80665 * 0.0289644 / 8.31432


def exp_population(rng, n, a_special, thr_of, eps=0.01):
    """(a, d0, d1, d2, is_special): a = expo1 = -g M / (R T) for T in 150 .. 330 K (or a_special), d_i = h_i - hb with h_1 = h - eps,
    h_2 = h + eps rounded as the stepper rounds them; special: centres at both sides of the places where the vote flips."""
    is_special = mix_into_wavefronts(rng, n // 2, n - n // 2)
    n = is_special.size
    invln2n = 184.6649652337873
    a = -GMR / rng.uniform(150.0, 330.0, n)
    # per wavefront (in the mixed part: for its special lane): physical exponents or one of a_special, and one side of the threshold
    pick = per_wavefront(rng, n, lambda w: rng.integers(-1, len(a_special), w))
    big = is_special & (pick >= 0)
    a[big] = np.asarray(a_special, dtype=np.float64)[pick[big]]
    inside = per_wavefront(rng, n, lambda w: rng.uniform(size=w) < 0.5)
    hb = rng.choice([0.0, 9000.0, 11000.0, 20000.0, 47000.0, -123.456], n)
    dmax = np.minimum(30000.0, 600.0 / np.abs(a))
    d = rng.uniform(0.0, 1.0, n) * dmax
    sp = np.flatnonzero(is_special)
    k = np.floor(rng.uniform(0.0, 1.0, sp.size) * dmax[sp] * np.abs(a[sp]) * invln2n)
    d[sp] = (k + 0.5 + hair(rng, thr_of(a[sp]), inside[sp])) / (np.abs(a[sp]) * invln2n)
    h = hb + d
    return a, h - hb, (h - eps) - hb, (h + eps) - hb, is_special
