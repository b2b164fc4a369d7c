"""The tables, targets and planes of the apparent-elevation tests, in one place: tests/test_sky_apparent_model.py asserts the
hand-computed answers and the closure without a GPU, tests/test_sky_apparent_abi.py runs the library's host functions over them and
tests/test_gpu_sky_apparent.py / tests/test_gpu_shadow_true.py the device.  Test infrastructure only."""
import math

import numpy as np

import shadow_cases as sc
import sky_apparent_model as sam
from atm_raytracer_amd import config

E, G, I = sam.EXIT, sam.skm.GROUND, sam.skm.INSIDE
NAN = math.nan

# ---- tables made by hand: de = 1 degree from 0 (e_k = k), dh = 500 m from 0; every number a dyadic rational, so that every
# ---- answer below is exact and was computed by hand --------------------------------------------------------------------------
HAND_ALT, HAND_EL = (0.0, 1000.0, 3), (0.0, 4.0, 5)

# rows for the tail rule: (T, S, tail)
TAIL_ROWS = [
    ([-0.5, 0.75, 1.75, 2.875, 3.9375], [E, E, E, E, E], 0),   # the whole row
    ([NAN, 0.5, 1.5, 2.5, 3.5], [G, E, E, E, E], 1),           # a non-EXIT first entry
    ([0.25, 1.0, 1.0, 2.0, 3.75], [E, E, E, E, E], 2),         # an equal pair: T[1] < T[2] is false
    ([0.0, 1.0, 5.0, 3.0, 3.5], [E, E, E, E, E], 3),           # n_el - 2: the last usable tail
    ([0.0, 1.0, NAN, 3.0, 3.5], [E, E, I, E, E], 3),           # a non-EXIT entry inside the row
    ([0.0, 1.0, 2.0, 3.5, 3.5], [E, E, E, E, E], 4),           # an equal last pair: not usable
    ([0.0, 1.0, 2.0, 4.0, 3.5], [E, E, E, E, E], 4),           # a falling last pair: not usable
    ([0.0, 1.0, 2.0, 3.0, NAN], [E, E, E, E, G], 5),           # the last entry is not EXIT: n_el
    ([NAN] * 5, [G] * 5, 5),
]

# the table of the inverse's answers: rows 0, 1, 2 of TAIL_ROWS (tails 0, 1, 2: all usable)
HAND_T = [TAIL_ROWS[0][0], TAIL_ROWS[1][0], TAIL_ROWS[2][0]]
HAND_S = [TAIL_ROWS[0][1], TAIL_ROWS[1][1], TAIL_ROWS[2][1]]
HAND_TAIL = [0, 1, 2]

# (row j, t, row(j, t), arm)
ROW_ANSWERS = [
    (0, 0.75, 1.0, "inside"),      # on the entry k = 1: the >= side takes k = 1, w = (0.75 + 0.5) / 1.25 = 1 -> e_0 + 1 = e_1
    (0, 1.25, 1.5, "inside"),      # k = 2, w = 0.5 / 1.0
    (0, -0.5, 0.0, "inside"),      # at T[k0]: k = 1, w = 0 -> e_0
    (0, -0.75, -0.25, "below"),    # t + (e_0 - T[0]) = -0.75 + 0.5
    (0, 3.9375, 4.0, "inside"),    # at T[L]: k = 4, w = 1
    (0, 5.0, 5.0625, "above"),     # t + (e_4 - T[4]) = 5 + 0.0625
    (0, NAN, NAN, "nan"),
    (1, 1.25, 1.75, "inside"),     # k = 2, w = 0.75 / 1
    (1, 0.5, 1.0, "inside"),       # at T[k0 = 1]: w = 0 -> e_1
    (1, 0.25, 0.75, "below"),      # t + (e_1 - 0.5)
    (1, -0.75, -0.25, "below"),
    (1, 5.0, 5.5, "above"),
    (2, 1.25, 2.25, "inside"),     # k0 = 2: k = 3, w = 0.25 / 1
    (2, 1.0, 2.0, "inside"),       # at T[k0 = 2] (the equal pair's upper entry): w = 0 -> e_2
    (2, 0.25, 1.25, "below"),      # t + (e_2 - 1.0): entries 0 and 1 are not consulted
    (2, -0.75, 0.25, "below"),
    (2, 5.0, 5.25, "above"),
]

# the same over TAIL_ROWS[3] alone, whose tail is n_el - 2 = 3: (t, row(t), arm)
LAST_TAIL_ANSWERS = [(3.25, 3.5, "inside"), (3.0, 3.0, "inside"), (2.0, 2.0, "below"), (3.5, 4.0, "inside"), (4.0, 4.5, "above")]

# (h, t, apparent(h, t))
APPARENT_ANSWERS = [
    (0.0, 1.25, 1.5),        # on level 0: j = 0, f = 0
    (500.0, 1.25, 1.75),     # on level 1: j = 1, f = 0
    (1000.0, 1.25, 2.25),    # on the last level: j = n_alt - 2 = 1, f = 1
    (250.0, 1.25, 1.625),    # between: j = 0, f = 0.5: 1.5 + 0.5 * 0.25
    (750.0, 1.25, 2.0),      # j = 1, f = 0.5: 1.75 + 0.5 * 0.5
    (-300.0, 1.25, 1.5),     # below alt_lo: u clamped to 0
    (5000.0, 1.25, 2.25),    # above alt_hi: u clamped to 2
    (-math.inf, 1.25, 1.5), (math.inf, 1.25, 2.25),
    (750.0, -0.75, 0.0),     # both rows' first arm: -0.25 + 0.5 * 0.5
    (250.0, 5.0, 5.28125),   # both rows' second arm: 5.0625 + 0.5 * 0.4375
    (250.0, 0.125, 0.5625),  # row 0 inside (k = 1, w = 0.625 / 1.25 = 0.5 -> 0.5), row 1 below (0.625): 0.5 + 0.5 * 0.125
    (NAN, 1.25, NAN), (250.0, NAN, NAN),
]


def hand_spec():
    return sam.Spec(HAND_ALT, HAND_EL)


def hand_table():
    return sam.Table(hand_spec(), HAND_T, HAND_S)


# ---- the closure against the exact route ------------------------------------------------------------------------------------------
SPHERE = {"Spherical": {"radius": 6371000.0}}
CLOSURE_EL = (-4.0, 12.0, 801)  # de = 0.02 degrees
CLOSURE_ROWS = (0.0, 4000.0, 8000.0)
CLOSURE_DH = 281.25
CLOSURE_TOP_TARGET = 11.0
CLOSURE_BOUND = 2.0e-4  # degrees


def closure_spec(alt_lo):
    return sam.Spec((alt_lo, alt_lo + CLOSURE_DH, 2), CLOSURE_EL, step=1000.0, top=100000.0, floor=0.0)


def closure_targets(table, n=102):
    """n true elevations from the higher of the pair's two tail starts to 11 degrees: half of them within 1 degree of the start
    (the first ON it), the rest spread over what is left; none on a lattice value by construction (odd fractions)."""
    start = max(float(table.T[j][int(table.tail[j])]) for j in range(2))
    near = start + 1.0 * (np.arange(n // 2) / (n // 2)) ** 2  # dense next to the start
    far = start + 1.0 + (CLOSURE_TOP_TARGET - start - 1.0) * (np.arange(n - n // 2) + 0.37) / (n - n // 2)
    return start, np.concatenate([near, far])


def setting_cfg(earth=None, atmosphere=None, straight=False, step=100.0):
    """A configuration that holds a setting only (the view is not used): the earth model, straight_rays, the atmosphere."""
    doc = {"view": {"position": {"latitude": 0.5, "longitude": 0.5, "altitude": {"Absolute": 100.0}},
                    "frame": {"direction": 0.0, "fov": 10.0, "tilt": 0.0, "max_distance": 10_000.0}},
           "earth_shape": earth or SPHERE, "straight_rays": straight, "simulation_step": step,
           "output": {"width": 4, "height": 4, "generator": "Rectilinear"}}
    if atmosphere is not None:
        doc["atmosphere"] = atmosphere
    return config.Config.from_dict(doc)


# ---- the tables of the library's tests: 0.05 degrees from -3 degrees, rows 1500 m apart from 0, sky step 1000 m, m = 1500 ----------
TABLE_EL_LO, TABLE_DE, TABLE_DH = -3.0, 0.05, 1500.0
N_ALT, N_EL = (2, 3), (2, 63, 64, 65, 257)
# name -> (earth, straight, the atmosphere's maker or None, top).  From 0 m every setting has GROUND rays below its horizon;
# spline30: every ray that clears the ground EXITs, through the cubic stepper; spline100: that atmosphere gives NaN heights above
# its last point, every ascending ray is LOST: tail == n_el in every row.
SETTINGS = {
    "us76_sphere": (SPHERE, False, None, 100000.0),
    "flat": ("FlatDistorted", False, None, 100000.0),
    "straight": (SPHERE, True, None, 100000.0),
    "spline30": (SPHERE, False, sc.spline_atmosphere, 30000.0),
    "spline100": (SPHERE, False, sc.spline_atmosphere, 100000.0),
}


def table_spec(n_alt=3, n_el=257, top=100000.0):
    return sam.Spec((0.0, TABLE_DH * (n_alt - 1), n_alt), (TABLE_EL_LO, TABLE_EL_LO + TABLE_DE * (n_el - 1), n_el), step=1000.0, top=top, floor=0.0, m=1500)


def setting_of(name):
    earth, straight, atm, top = SETTINGS[name]
    return setting_cfg(earth, atm() if atm else None, straight), top


def abi_spec(spec, step=None):
    """A sky_apparent_model.Spec as the library's atmrt_sky_table_spec_t."""
    from atm_raytracer_amd import generators
    return generators.sky_table_spec((spec.alt_lo, spec.alt_hi, spec.n_alt), (spec.el_lo, spec.el_hi, spec.n_el), step=spec.step if step is None else step,
                                     top=spec.top, floor=spec.floor, m=spec.m)


def census_pairs(table, n=257, seed=3):
    """n (h, t) pairs over a usable table that reach every arm of the row inverse, both clamps, a level, and NaN in either place."""
    s = table.spec
    rng = np.random.default_rng(seed)
    lo = float(min(table.T[j][int(table.tail[j])] for j in range(s.n_alt)))
    hi = float(max(table.T[j][s.n_el - 1] for j in range(s.n_alt)))
    h = rng.uniform(s.alt_lo - 500.0, s.alt_hi + 500.0, n)
    t = rng.uniform(lo - 1.0, hi + 1.0, n)
    h[0], h[1], h[2], h[3], t[4] = s.alt_lo, s.alt(1), s.alt_hi, NAN, NAN
    t[5], t[6] = float(table.T[0][int(table.tail[0])]), float(table.T[0][s.n_el - 1])  # on the tail's two ends
    t[7], h[7] = float(table.T[1][int(table.tail[1]) + 3]), s.alt(1)                   # on an entry
    t[8], t[9], t[10], t[11] = lo - 50.0, hi + 30.0, -89.99, 89.99
    return h, t


# ---- the sunset: the case that tells the two rules apart -------------------------------------------------------------------------
SUNSET_TRUE_ELEVATION, SUNSET_REACH, SUNSET_LIFT = -0.3, 5_000.0, 2.0
SUNSET_AT = (0.5, 0.5)


def sunset_cfg():
    """The 6371 km sphere with US-76 and no terrain at all (every post reads 0 m), step 100 m."""
    return setting_cfg()


def sunset_points(n=65):
    """n points at elevation 0 within 70 m of (0.5 N, 0.5 E): the light's local elevation differs by less than 1e-3 degrees among them."""
    k = np.arange(n)
    return SUNSET_AT[0] + 1.0e-5 * (k % 8), SUNSET_AT[1] + 1.0e-5 * (k // 8), np.zeros(n)
