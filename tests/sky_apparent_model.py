"""The rule of include/atmrt.h, "apparent elevation", restated in Python floats (IEEE doubles, every operation rounded on its own, no
fma): the refraction table over tests/sky_model.py's exact route, its tail, the row inverse and apparent(h, t), and the
true-direction shadow lights over tests/shadow_lights_model.py's pieces.  Test infrastructure only: what atmrt_sky_table,
atmrt_sky_tail_host, atmrt_sky_apparent*, and atmrt_shadow_lights_true* must return, byte for byte."""
import math

import numpy as np

import shadow_lights_model as slm
import shadow_model as sm
import sky_model as skm
from shadow_model import LIT, NONE, SHADOWED  # noqa: F401  (re-exported for the tests)

EXIT = skm.EXIT
NAN = float("nan")
ALT_MAX, EL_MAX, ENTRIES_MAX = 1024, 65536, 1 << 24


class Spec:
    """atmrt_sky_table_spec_t with its step resolved: sky = (step, top, floor, m), alt = (lo, hi, n), el = (lo, hi, n)."""

    def __init__(self, alt, el, step=1000.0, top=100000.0, floor=0.0, m=skm.M_MAX):
        self.step, self.top, self.floor, self.m = float(step), float(top), float(floor), int(m)
        self.alt_lo, self.alt_hi, self.n_alt = float(alt[0]), float(alt[1]), int(alt[2])
        self.el_lo, self.el_hi, self.n_el = float(el[0]), float(el[1]), int(el[2])

    def valid(self):
        nums = (self.alt_lo, self.alt_hi, self.el_lo, self.el_hi)
        return (skm.spec_valid(self.step, self.top, self.floor, self.m) and all(math.isfinite(v) for v in nums)
                and self.alt_lo < self.alt_hi and -90.0 < self.el_lo < self.el_hi < 90.0 and 2 <= self.n_alt <= ALT_MAX
                and 2 <= self.n_el <= EL_MAX and self.n_alt * self.n_el <= ENTRIES_MAX)

    @property
    def dh(self):
        return (self.alt_hi - self.alt_lo) / float(self.n_alt - 1)

    @property
    def de(self):
        return (self.el_hi - self.el_lo) / float(self.n_el - 1)

    def alt(self, j):
        return self.alt_lo + float(j) * self.dh

    def el(self, k):
        return self.el_lo + float(k) * self.de


def tail_of(T_row, S_row):
    """tail[j] of one row: the smallest k0 with entries k0 .. n_el - 1 all EXIT and strictly increasing; n_el without an EXIT end."""
    n_el = len(S_row)
    if S_row[n_el - 1] != EXIT:
        return n_el
    k0 = n_el - 1
    while k0 > 0 and S_row[k0 - 1] == EXIT and float(T_row[k0 - 1]) < float(T_row[k0]):
        k0 -= 1
    return k0


def tails(T, S):
    return np.array([tail_of(T[j], S[j]) for j in range(len(S))], dtype=np.uint32)


def usable(tail, n_el):
    return np.asarray(tail).astype(np.int64) <= n_el - 2


class Table:
    """T [n_alt][n_el] f64 (NaN unless EXIT), S [n_alt][n_el] u8, tail [n_alt] u32 of a spec, and the counts of atmrt_sky_stats_t."""

    def __init__(self, spec, T, S, stats=None):
        self.spec = spec
        self.T, self.S = np.asarray(T, dtype=np.float64).reshape(spec.n_alt, spec.n_el), np.asarray(S, dtype=np.uint8).reshape(spec.n_alt, spec.n_el)
        self.tail = tails(self.T, self.S)
        self.stats = stats

    @property
    def usable(self):
        return usable(self.tail, self.spec.n_el)


def build(setting, spec):
    """The table of a sky_model.Setting by the exact route: one sky_model.ray per entry."""
    assert spec.valid()
    T = np.full((spec.n_alt, spec.n_el), np.nan)
    S = np.zeros((spec.n_alt, spec.n_el), dtype=np.uint8)
    steps = 0
    for j in range(spec.n_alt):
        for k in range(spec.n_el):
            S[j, k], n, T[j, k] = skm.ray(setting, spec.alt(j), spec.el(k), spec.step, spec.top, spec.floor, spec.m)
            steps += n
    stats = dict(none=0, exit=int((S == skm.EXIT).sum()), ground=int((S == skm.GROUND).sum()), inside=int((S == skm.INSIDE).sum()),
                 lost=int((S == skm.LOST).sum()), integrated_steps=steps)
    return Table(spec, T, S, stats)


def row(spec, T_row, k0, t):
    """row(j, t) over a usable row: (value, arm) with arm one of 'nan', 'below', 'above', 'inside'."""
    t = float(t)
    if t != t:
        return NAN, "nan"
    L = spec.n_el - 1
    assert k0 <= L - 1
    if t < float(T_row[k0]):
        return t + (spec.el(k0) - float(T_row[k0])), "below"
    if t > float(T_row[L]):
        return t + (spec.el(L) - float(T_row[L])), "above"
    k = k0 + 1
    while not float(T_row[k]) >= t:  # the smallest index in (k0, L]: the tail is strictly increasing, a bisection finds the same
        k += 1
    w = (t - float(T_row[k - 1])) / (float(T_row[k]) - float(T_row[k - 1]))
    return spec.el(k - 1) + w * (spec.el(k) - spec.el(k - 1)), "inside"


def apparent_parts(table, h, t):
    """apparent(h, t) -> (value, j, f, arm of row j, arm of row j + 1); (NaN, None, ...) for a NaN h."""
    s = table.spec
    assert table.usable.all()
    u = (float(h) - s.alt_lo) / s.dh
    if u != u:
        return NAN, None, None, None, None
    last = float(s.n_alt - 1)
    u = 0.0 if u < 0.0 else (last if u > last else u)
    j = min(int(math.floor(u)), s.n_alt - 2)
    f = u - float(j)
    a, arm_a = row(s, table.T[j], int(table.tail[j]), t)
    b, arm_b = row(s, table.T[j + 1], int(table.tail[j + 1]), t)
    return a + f * (b - a), j, f, arm_a, arm_b


def apparent(table, h, t, straight=False):
    """apparent(h, t); with straight rays t itself, no table consulted."""
    if straight:
        return float(t)
    return apparent_parts(table, h, t)[0]


def solve_true(setting, table, res, dirs, reach, lift=0.0, lib=None):
    """shadow_lights_model.solve under the true-direction rule: the local elevation strictly inside (-90, 90) becomes
    apparent(H_0, elevation) before the three no-march tests.  table: a Table (not read with straight rays).  The Result also holds
    true_elevation [n_lights][H][W], the local elevation before the insertion."""
    dirs = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    lights = [slm.normalise(v) for v in dirs]
    assert 1 <= len(lights) <= 64 and all(v is not None for v in lights)
    d, m = sm.lattice(setting.step, float(reach))
    floor, ang_max = setting.escape(float(reach), lib)
    H, W = np.asarray(res["hit_count"]).shape
    n = len(lights)
    mask = np.zeros(H * W, dtype=np.uint64)
    status = np.zeros((n, H * W), dtype=np.uint8)
    block = np.zeros((n, H * W), dtype=np.uint16)
    esc = np.zeros((n, H * W), dtype=np.int32)
    marched = np.zeros((n, H * W), dtype=bool)
    azimuth, elevation, true = np.full((n, H * W), np.nan), np.full((n, H * W), np.nan), np.full((n, H * W), np.nan)
    px, lat, lon, elev = sm.first_points(res)
    for p, la, lo, el in zip(px, lat, lon, elev):
        bits = 0
        h0 = float(el) + float(lift)
        for l, L in enumerate(lights):
            az_p, el_p = slm.local_direction(setting.o, setting.params.earth, L, la, lo)
            true[l, p] = el_p
            if -90.0 < el_p < 90.0:
                el_p = apparent(table, h0, el_p, setting.straight)
            azimuth[l, p], elevation[l, p] = az_p, el_p
            if el_p >= 90.0:
                out = (LIT, 0, 0)
            elif el_p <= -90.0:
                out = (SHADOWED, 1, 0)
            elif not (-90.0 < el_p < 90.0):  # NaN
                out = (LIT, 0, 0)
            else:
                marched[l, p] = True
                out = sm.march(setting, la, lo, el, (az_p, el_p, float(reach), float(lift)), d, m, floor, ang_max)
            status[l, p], block[l, p], esc[l, p] = out
            if out[0] == LIT:
                bits |= 1 << l
        mask[p] = bits
    r = slm.Result()
    r.m, r.floor, r.n_lights = m, floor, n
    r.lit_mask = mask.reshape(H, W)
    r.status, r.block, r.esc = status.reshape(n, H, W), block.reshape(n, H, W), esc.reshape(n, H, W)
    r.marched, r.azimuth, r.elevation = marched.reshape(n, H, W), azimuth.reshape(n, H, W), elevation.reshape(n, H, W)
    r.true_elevation = true.reshape(n, H, W)
    lit, sh = status == LIT, status == SHADOWED
    none = int((np.asarray(res["hit_count"]).ravel() == 0).sum())
    base = dict(none=none, lit=int(lit.sum()), shadowed=int(sh.sum()))
    blocked = int(block[sh & marched].astype(np.int64).sum())
    escaped = lit & marched & (esc > 0)
    r.stats_off = dict(base, integrated_steps=blocked + m * int((lit & marched).sum()), escaped_rays=0)
    r.stats_on = dict(base, integrated_steps=blocked + int(esc[escaped].astype(np.int64).sum()) + m * int((lit & marched & ~escaped).sum()),
                      escaped_rays=int((escaped & (esc < m)).sum()))
    return r
