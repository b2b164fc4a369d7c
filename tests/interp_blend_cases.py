"""Hand-made lattices for atmrt_debug_interp_blend: the inputs of tests/test_gpu_interp_blend.py (probe against model, bit for bit) and
of the census in tests/test_interp_blend_model.py (the cases reach what they claim).  Nothing here computes an expectation.

Every case is a dict {name, group, elev, dir [h][w], min_elev_step, min_dir_step, simulation_step, lattice}; `lattice` is the dict
_abi.interp_lattice takes.  The steps are powers of two and every ray is (key + remainder) * step with key + remainder an exact double,
so the remainder the blend sees is the one the case names.  That limits where the two extreme remainders can stand: the double just
below 0.5 is the remainder of a quotient only under key 0, the double just below 1 only under key 0 or -1 (under any other key the
sum is not a double).  A pixel whose remainders are both of that kind can therefore only own the cell at (0, 0), and a call holds one
such pixel: the table (a) is 64 small calls, four per mask.

Every pixel owns the 2 x 2 lattice points of its cell (Builder.pixel refuses an overlap), so no pixel's corners show up in another's
answer; the steps cases share cells on purpose.  Lattice points of the bounding rectangle that no pixel references carry a filler
point of their own: a blend that reads a neighbour's corner does not read zeros."""
import itertools
import math
from fractions import Fraction

import numpy as np

TERRAIN, RGBA = 0, 1
PRED_HALF, PRED_ONE = math.nextafter(0.5, 0.0), math.nextafter(1.0, 0.0)
REMS6 = (0.0, 0.25, PRED_HALF, 0.5, 0.75, PRED_ONE)   # the grid of (a)
STEP = 50.0                                            # simulation_step of every case
WIDTHS = (1, 63, 64, 65, 257)


def trace_point(rng, distance, tag):
    """A trace point with full-mantissa field values of its own: (lat, lon, distance, elevation, path_length, normal, tag, rgba)."""
    rgba = (0.0, 0.0, 0.0, float(rng.uniform(0.2, 1.0))) if tag == TERRAIN else tuple(float(v) for v in rng.uniform(0.0, 1.0, 4))
    return (float(rng.uniform(40.0, 50.0)), float(rng.uniform(5.0, 15.0)), float(distance), float(rng.uniform(-100.0, 3000.0)),
            float(distance) * float(rng.uniform(1.0, 1.001)), tuple(float(v) for v in rng.uniform(-1.0, 1.0, 3)), tag, rgba)


class Builder:
    def __init__(self, name, group, seed, min_elev_step=2.0 ** -10, min_dir_step=2.0 ** -9, shared_cells=False):
        self.name, self.group, self.rng = name, group, np.random.default_rng(seed)
        self.min_elev_step, self.min_dir_step, self.shared_cells = min_elev_step, min_dir_step, shared_cells
        self.rays, self.points, self.meta = [], {}, {}
        self.n_e_strip = self.n_d_strip = self.n_grid = 0

    def pixel(self, key_e, rem_e, key_d, rem_d, corners=None):
        """The next pixel (row-major): its ray, and the trace points of its four corners in SEQUENCE order (None: leave the lattice
        as it is — shared cells only)."""
        for key, rem in ((key_e, rem_e), (key_d, rem_d)):
            assert 0.0 <= rem < 1.0 and Fraction(float(key) + rem) == Fraction(key) + Fraction(rem), (key, rem)
        self.rays.append((float(key_e) + rem_e, float(key_d) + rem_d))
        if corners is not None:
            for (i, j), tps in zip(((0, 0), (0, 1), (1, 0), (1, 1)), corners):
                assert self.shared_cells or (key_e + i, key_d + j) not in self.points, "every pixel owns its cell"
                self.points[(key_e + i, key_d + j)] = list(tps)

    def place(self, rem_e, rem_d, corners, cw=16):
        """pixel() at a cell of its own that the remainders allow: key 0 for an extreme remainder (a strip along the other axis),
        the grid from (2, 2) on for the others."""
        special_e, special_d = rem_e in (PRED_HALF, PRED_ONE), rem_d in (PRED_HALF, PRED_ONE)
        if special_e and special_d:
            key_e = key_d = 0
        elif special_e:
            self.n_e_strip += 1
            key_e, key_d = 0, 2 * self.n_e_strip
        elif special_d:
            self.n_d_strip += 1
            key_e, key_d = 2 * self.n_d_strip, 0
        else:
            key_e, key_d = 2 * (1 + self.n_grid // cw), 2 * (1 + self.n_grid % cw)
            self.n_grid += 1
        self.pixel(key_e, rem_e, key_d, rem_d, corners)

    def build(self, w, h=1):
        assert len(self.rays) == w * h and w in WIDTHS and h <= 3, (self.name, len(self.rays), w, h)
        rng = self.rng
        q = np.array(self.rays).reshape(h, w, 2)
        ke, kd = np.floor(q[..., 0]).astype(int), np.floor(q[..., 1]).astype(int)
        ei0, di0, ne, nd = ke.min(), kd.min(), ke.max() + 2 - ke.min(), kd.max() + 2 - kd.min()
        assert ne * nd <= 6000, (self.name, ne, nd)
        lat = {"hit_count": np.zeros((ne, nd), dtype=np.uint32), "azimuth": rng.uniform(0.0, 360.0, (ne, nd)),
               "elevation_angle": rng.uniform(-90.0, 90.0, (ne, nd)), "px_steps": rng.integers(1, 5000, (ne, nd)).astype(np.uint32)}
        if "px_steps" in self.meta:
            lat["px_steps"] = self.meta.pop("px_steps")(rng, ne, nd)
        tps = []
        for i in range(ne):
            for j in range(nd):
                here = self.points.get((ei0 + i, di0 + j))
                if here is None:  # no pixel's corner: a filler point
                    here = [trace_point(rng, 777.0, int(rng.integers(0, 2)))]
                lat["hit_count"][i, j] = len(here)
                tps.extend(here)
        n = len(tps)
        for k, name in enumerate(("lat", "lon", "distance", "elevation", "path_length")):
            lat[name] = np.array([t[k] for t in tps], dtype=np.float64)
        lat["normal"] = np.array([t[5] for t in tps], dtype=np.float64).reshape(n, 3)
        lat["color_tag"] = np.array([t[6] for t in tps], dtype=np.uint32)
        lat["rgba"] = np.array([t[7] for t in tps], dtype=np.float64).reshape(n, 4)
        return dict(name=self.name, group=self.group, elev=q[..., 0] * self.min_elev_step, dir=q[..., 1] * self.min_dir_step,
                    min_elev_step=self.min_elev_step, min_dir_step=self.min_dir_step, simulation_step=STEP, lattice=lat, **self.meta)


def mask_corners(rng, mask, tag, base=1000.0):
    """One point in every corner of `mask`, all of one class and within a step of each other: one group with that presence mask."""
    return [[trace_point(rng, base + float(rng.uniform(0.0, 20.0)), tag)] if mask >> c & 1 else [] for c in range(4)]


# ---- (a) the table: 16 masks x REMS6 x REMS6 ----------------------------------------------------------------------------------------
def table_cases():
    combos = list(itertools.product(REMS6, REMS6))
    both = [c for c in combos if c[0] in (PRED_HALF, PRED_ONE) and c[1] in (PRED_HALF, PRED_ONE)]
    rest = [c for c in combos if c not in both]
    cases = []
    for mask in range(16):
        for k, ss in enumerate(both):  # a call holds one pixel with two extreme remainders (module docstring)
            w = (63, 64, 65)[(4 * mask + k) % 3]
            b = Builder(f"table-mask{mask}-{k}", "a", 1000 + 4 * mask + k)
            b.meta["mask"] = mask
            for p in range(w):
                rem_e, rem_d = ss if p == 0 else rest[(p - 1 + 8 * k) % len(rest)]
                b.place(rem_e, rem_d, mask_corners(b.rng, mask, (mask + p) % 2), cw=8)
            cases.append(b.build(w))
    return cases


# ---- (b) grouping ---------------------------------------------------------------------------------------------------------------------
def grouping_scenarios(rng):
    """[(name, corners)]: each one rule of collect_trace_points / match_sequence."""
    T, R = TERRAIN, RGBA
    tp = lambda d, tag=T: trace_point(rng, d, tag)
    return [
        ("exactly-a-step-apart", [[tp(1000.0), tp(1000.0 + STEP)], [], [], []]),                           # `<` is strict: two groups
        ("an-ulp-closer", [[tp(1000.0), tp(math.nextafter(1000.0 + STEP, 0.0))], [], [], []]),             # one group, the later point stays
        ("equal-distance-other-class", [[tp(1000.0, T), tp(1000.0, R)], [], [], []]),                      # two groups
        ("joins-the-first-of-two", [[tp(1000.0), tp(1060.0)], [tp(1030.0)], [], []]),                      # 1030 is near both
        ("through-the-second-member", [[tp(1000.0)], [tp(1040.0)], [tp(1080.0)], []]),                     # 1080 is near 1040 only
        ("creation-order", [[tp(3000.0), tp(1000.0), tp(2000.0)], [tp(2010.0), tp(3010.0)], [], []]),      # out: 3000, 1000, 2000
        ("other-class-between", [[tp(1000.0, R)], [tp(1010.0, T)], [tp(1020.0, R)], [tp(1030.0, T)]]),     # two groups, diagonal masks
    ]


def grouping_cases():
    b = Builder("grouping", "b", 2000)
    rems = [(0.25, 0.25), (0.75, 0.25), (0.25, 0.75), (0.75, 0.75), (0.5, 0.5), (0.0, 0.0), (PRED_HALF, 0.25), (0.25, PRED_HALF), (0.375, 0.625)]
    names = []
    for p in range(63):
        name, corners = grouping_scenarios(b.rng)[p % 7]
        rem_e, rem_d = rems[p // 7]
        names.append(name)
        b.place(rem_e, rem_d, corners)
    b.meta["scenario"] = names
    return [b.build(63)]


# ---- (c) the 4 / 5 hand-over ----------------------------------------------------------------------------------------------------------
def handover_cases():
    """Every split of 4 points over the corners (35), each beside the same pixel with one far point of the other class added (5 points:
    the arena kernel's pixel), and the totals 0 .. 3.  meta pairs: (pixel of 4, pixel of 5), same rays and same first points."""
    b = Builder("handover", "c", 3000)
    rng = b.rng
    splits = [s for s in itertools.product(range(5), repeat=4) if sum(s) == 4]
    assert len(splits) == 35
    small = [(0, 0, 0, 0), (1, 0, 0, 0), (0, 0, 1, 0), (1, 1, 0, 0), (0, 1, 0, 1), (1, 1, 1, 0), (0, 1, 1, 1), (2, 0, 0, 1), (0, 3, 0, 0)]
    rems = [(0.25, 0.25), (0.25, 0.75), (0.75, 0.25), (0.75, 0.75), (0.5, 0.25), (0.375, 0.5)]
    pairs, pixels = [], []
    for n, split in enumerate(splits):
        tag = n % 2
        # the j-th points of the corners lie within a step of each other, consecutive ones more than a step apart
        corners = [[trace_point(rng, 1000.0 + 100.0 * j + float(rng.uniform(0.0, 20.0)), tag) for j in range(c)] for c in split]
        extra = [list(c) for c in corners]
        extra[n % 4] = extra[n % 4] + [trace_point(rng, 9000.0, 1 - tag)]
        pairs.append((len(pixels), len(pixels) + 1))
        pixels += [(rems[n % 6], corners), (rems[n % 6], extra)]
    for n, split in enumerate(small):
        pixels.append((rems[n % 6], [[trace_point(rng, 1000.0 + 100.0 * j + float(rng.uniform(0.0, 20.0)), n % 2) for j in range(c)] for c in split]))
    while len(pixels) < 195:  # the rest of the image: the splits again, other values and remainders
        n = len(pixels)
        split = splits[n % 35]
        pixels.append((rems[(n // 35 + n) % 6], [[trace_point(rng, 1000.0 + 100.0 * j + float(rng.uniform(0.0, 20.0)), n % 2) for j in range(c)] for c in split]))
    for (rem_e, rem_d), corners in pixels:
        b.place(rem_e, rem_d, corners)
    b.meta["pairs"] = pairs
    return [b.build(65, 3)]


# ---- (d) the arena --------------------------------------------------------------------------------------------------------------------
def arena_cases():
    cases = []
    # one pixel, 64 points, four groups: 16 points per corner, four around each of four distances
    b = Builder("arena-64-points", "d", 4000)
    corners = [[trace_point(b.rng, 1000.0 * (1 + j % 4) + float(b.rng.uniform(0.0, 20.0)), TERRAIN) for j in range(16)] for _ in range(4)]
    b.place(0.25, 0.625, corners)
    cases.append(b.build(1))
    # one pixel, 4 x 80 points, all more than a step apart: 320 groups of one corner each; the groups of the last corner have the
    # ids 240 .. 319 and are the ones these remainders accept (one lane walks some ten million member slots: one such pixel is enough)
    b = Builder("arena-320-groups", "d", 4002)
    corners = [[trace_point(b.rng, 1000.0 + 100.0 * (80 * c + j), (c + j) % 2) for j in range(80)] for c in range(4)]
    b.place(0.75, 0.75, corners)
    cases.append(b.build(1))
    # 257 x 3: arena pixels (5 .. 12 corner points) among in-register ones, in both blocks of every row
    b = Builder("arena-mixed-image", "d", 4003)
    rng = b.rng
    rems = [(0.25, 0.25), (0.25, 0.75), (0.75, 0.25), (0.75, 0.75), (0.5, 0.5), (0.125, 0.875)]
    for p in range(257 * 3):
        big = rng.random() < 0.5
        if p % 257 == 256:  # the second block's only lane: an arena pixel in the rows 0 and 2, an in-register one in row 1
            big = p // 257 != 1
        counts = rng.integers(1, 4, 4) if big else rng.integers(0, 2, 4)
        if big and counts.sum() < 5:
            counts[int(rng.integers(0, 4))] += 5 - counts.sum()
        corners = [[trace_point(rng, 1000.0 + 40.0 * int(rng.integers(0, 8)), int(rng.integers(0, 2))) for _ in range(c)] for c in counts]
        rem_e, rem_d = rems[int(rng.integers(0, 6))]
        b.place(rem_e, rem_d, corners, cw=32)
    cases.append(b.build(257, 3))
    return cases


# ---- (e) keys -------------------------------------------------------------------------------------------------------------------------
def key_cases():
    cases = []
    # 257 x 3, keys of both signs: cells from (-15, -19) on, two apart; remainders that make the quotients exact, 0 among them
    # (an integer quotient), and the last pixel — the last lane of the last block of k_lattice_keys — holding two of the four bounds
    for k in range(2):
        b = Builder(f"keys-both-signs-{k}", "e", 5000 + k)
        rems = (0.0, 0.25, 0.5, 0.75)
        for p in range(257 * 3 - 1):
            key_e, key_d = -15 + 2 * (p // 32), -19 + 2 * (p % 32)
            b.pixel(key_e, rems[(p + p // 32) % 4], key_d, rems[(p // 3) % 4], mask_corners(b.rng, 1 + p % 15, p % 2))
        # the keys of the pixels above span [-15, 33] x [-19, 43]
        key_e, key_d = ((-18, 46), (36, -22))[k]
        b.pixel(key_e, 0.75, key_d, 0.0, mask_corners(b.rng, 15, TERRAIN))
        cases.append(b.build(257, 3))
    # -0.25 steps: key -1, remainder 0.75 — and a quotient of exactly -1 — in a single-pixel image each
    for k, (key_e, rem_e, key_d, rem_d) in enumerate(((-1, 0.75, -1, 0.75), (-1, 0.0, -2, 0.0), (0, PRED_HALF, 0, PRED_ONE), (-1, PRED_ONE, 0, 0.5))):
        b = Builder(f"keys-single-pixel-{k}", "e", 5010 + k)
        b.pixel(key_e, rem_e, key_d, rem_d, mask_corners(b.rng, 15, k % 2))
        cases.append(b.build(1))
    return cases


# ---- (f) steps ------------------------------------------------------------------------------------------------------------------------
def step_cases():
    """Pixels that share lattice points: some points are referenced by several pixels, some by none; px_steps up to 2^32 - 1, so that
    the sum needs 64 bits."""
    cases = []
    for k, w in enumerate((63, 257)):
        b = Builder(f"steps-{k}", "f", 6000 + k, shared_cells=True)
        rng = b.rng
        for i in range(-2, 8):
            for j in range(-3, 12):
                b.points[(i, j)] = [trace_point(rng, 1000.0 + 30.0 * int(rng.integers(0, 4)), TERRAIN) for _ in range(int(rng.integers(0, 3)))]
        for p in range(w):
            corner = p in (0, w - 1)  # the rectangle's two far cells, so that its size does not depend on the draw
            key_e = (-2, 6)[p > 0] if corner else int(rng.integers(-2, 7) // 2 * 2)
            key_d = (-3, 10)[p > 0] if corner else int(rng.integers(-3, 11) // 3 * 3)
            b.pixel(key_e, float(rng.integers(0, 8)) / 8.0, key_d, float(rng.integers(0, 8)) / 8.0)
        b.meta["px_steps"] = lambda rng, ne, nd: rng.integers(2 ** 31, 2 ** 32, (ne, nd)).astype(np.uint32)
        cases.append(b.build(w))
    return cases


# ---- (g) the seeded sweep -------------------------------------------------------------------------------------------------------------
SWEEP_SEEDS = tuple(range(20))
SWEEP_COUNTS = (0, 0, 1, 1, 2, 3, 12)
SWEEP_OFFSETS = (0.0, 0.015625, 25.0, 49.984375)  # around the multiples of the step: differences of exactly a step, a little less, a little more


def sweep_case(seed):
    b = Builder(f"sweep-{seed}", "g", 7000 + seed)
    rng = b.rng
    w, h = 65, 3
    exact = (0.0, 0.25, 0.5, 0.75)
    kinds = rng.permutation(np.array([3] + [1] * 12 + [2] * 12 + [0] * (w * h - 25)))  # 3: both remainders extreme, 1 / 2: one of them

    def rem(extreme):
        if extreme:
            return (PRED_HALF, PRED_ONE)[int(rng.integers(0, 2))]
        return exact[int(rng.integers(0, 4))] if rng.random() < 0.5 else float(rng.integers(0, 2 ** 20)) / 2.0 ** 20

    for p in range(w * h):
        corners = [[trace_point(rng, 1000.0 + STEP * int(rng.integers(0, 4)) + SWEEP_OFFSETS[int(rng.integers(0, 4))], int(rng.integers(0, 2)))
                    for _ in range(SWEEP_COUNTS[int(rng.integers(0, 7))])] for _ in range(4)]
        b.place(rem(kinds[p] & 1), rem(kinds[p] & 2), corners)
    return b.build(w, h)


def sweep_cases():
    return [sweep_case(seed) for seed in SWEEP_SEEDS]


GROUPS = {"a": table_cases, "b": grouping_cases, "c": handover_cases, "d": arena_cases, "e": key_cases, "f": step_cases, "g": sweep_cases}
_built = {}


def cases(group):
    """The cases of a group, built once per process and handed out as they are: do not change them."""
    if group not in _built:
        _built[group] = GROUPS[group]()
    return _built[group]
