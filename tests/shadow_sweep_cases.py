"""The inputs of the cast-shadow sweep, in one place: tests/test_gpu_shadow_sweep.py runs them on the GPU against
tests/shadow_model.py, and tests/test_shadow_sweep_model.py asserts without a GPU, by the model alone, that they reach what they
are built to reach.  Test infrastructure only.

  1. shadow_sweep_case(seed): a seeded sweep of small frames over shadow_cases.scene and of lights;
  2. ridge points under a duct, beside the certificate's threshold and under straight rays on a small sphere, as hand-made planes;
  3. the model's known answers (tests/test_shadow_model.py) as planes, the compacted list's edges, m = 65535, azimuths out of range."""
import ctypes as C
import math
import os

import numpy as np

import atmospheres
import escape_cases as ec
import shadow_cases as sc
import shadow_model as sm
from atm_raytracer_amd import config
from util import nested_cylinders

EARTHS = ["SimpleSphere", {"Spherical": {"radius": 6371000.0}}, {"Spherical": {"radius": 3.0e6}}, "Wgs84",
          {"Ellipsoid": {"a": 6378137.0, "b": 6300000.0}}, "AzimuthalEquidistant", "FlatDistorted",
          {"ObserverAe": {"proj_radius": 6371000.0}}, "SimpleObserverAe"]  # the nine of tests/test_gpu_parity.py
# ATMRT_SHADOW_SEEDS widens the sweep and ATMRT_SHADOW_SEED_FIRST moves it, as the parity sweeps' variables do
N_SEEDS = int(os.environ.get("ATMRT_SHADOW_SEEDS", "40"))
SEED_FIRST = int(os.environ.get("ATMRT_SHADOW_SEED_FIRST", "0"))
SEEDS = range(SEED_FIRST, SEED_FIRST + N_SEEDS)
MAX_STEPS = 600  # the reach is capped here: the model stays at a few seconds per seed


# ---- 1. the seeded sweep -------------------------------------------------------------------------------------------------------------
def shadow_sweep_case(seed):
    """Seed -> dict(cfg, tiles, spec = (azimuth_deg, elevation_deg, reach, lift), ...): a frame of 3 .. 40 x 2 .. 24 pixels over
    shadow_cases.scene — generator, earth model, straight rays and the atmosphere's family by the seed's residues, the rest drawn —
    and a light: low (half of the seeds), below the horizontal, high, or just above the tile's horizons; any azimuth, also outside
    [0, 360); a reach inside the first step (m = 1), of 2 .. 30 km, or of 80 km (beyond the mosaic and the frame's max_distance).
    A fifth of the seeds compute a column shard, a fifth stand three opaque cylinders 3.3 km ahead of the observer."""
    rng = np.random.default_rng(41_000_000 + seed)
    generator = ["Fast", "Rectilinear", "InterpolatingRectilinear"][seed % 3]
    w, h = int(rng.integers(3, 41)), int(rng.integers(2, 25))
    earth = EARTHS[seed % 9]
    straight = seed % 4 == 3
    step = float(rng.choice([rng.uniform(37.0, 400.0), 50.0, 100.0]))
    alpha = float(rng.choice([1.0, 1.0, 0.5]))
    direction, tilt, fov = float(rng.uniform(0.0, 360.0)), float(rng.uniform(-25.0, -3.0)), float(rng.uniform(10.0, 60.0))
    family = seed % 5
    if family == 0:
        atm = None
    elif family == 1:
        atm = atmospheres.configuration_atmosphere(rng)
    elif family == 2:
        atm = atmospheres.extreme_atmosphere(rng)
    elif family == 3:
        atm = atmospheres.long_atmosphere(rng)
    else:
        atm = [atmospheres.WILD_SPLINE, atmospheres.OVERFLOWING_SPLINE][(seed // 5) % 2]
    over = dict(earth_shape=earth, straight_rays=straight, simulation_step=step, terrain_alpha=alpha, direction=direction, tilt=tilt, fov=fov)
    if atm is not None:
        over["atmosphere"] = atm
    cfg, tiles = sc.scene(w, h, generator=generator, **over)
    kind = seed % 6
    if kind <= 2:
        elevation = float(rng.uniform(0.3, 4.0))
    elif kind == 3:
        elevation = float(rng.uniform(-3.0, 0.3))
    elif kind == 4:
        elevation = float(rng.uniform(20.0, 89.9))
    else:
        elevation = float(rng.uniform(1.0, 2.5))
    azimuth = float(rng.uniform(-400.0, 800.0))
    # the set {inside the first step, 2 .. 30 km, 80 km}, tilted toward the longer reaches (1 : 5 : 2): at m = 1 no ray can escape early
    far = [float(rng.uniform(2_000.0, 30_000.0)) for _ in range(2)]
    reach = float(rng.choice([0.4 * step, far[0], 80_000.0, far[1], far[0], 80_000.0, far[1], far[0]]))
    reach = min(reach, (MAX_STEPS - 0.5) * step)  # half a step short: the lattice's repeated additions round
    lift = float(rng.choice([0.0, 2.0, 50.0]))
    shard = None
    if rng.uniform() < 0.2:
        c0 = int(rng.integers(0, w))
        shard = (c0, int(rng.integers(c0 + 1, w + 1)))
        cfg.params.col_begin, cfg.params.col_end = shard
    objects = bool(rng.uniform() < 0.2)
    if objects:  # as shadow_cases.with_objects, on the frame's own axis: 0.03 degrees of latitude are 3.3 km
        lat = 46.5 + 0.03 * math.cos(math.radians(direction))
        lon = 8.5 + 0.03 * math.sin(math.radians(direction)) / math.cos(math.radians(46.5))
        nested_cylinders(cfg, 3, lat=lat, lon=lon, r0=150.0, dr=50.0, alpha=1.0)
    return dict(seed=seed, cfg=cfg, tiles=tiles, spec=(azimuth, elevation, reach, lift), generator=generator, earth=seed % 9,
                straight=straight, step=step, family=family, shard=shard, objects=objects)


def is_cubic(setting):
    """The stepper kind the library picks for the setting's atmosphere: Spline (a cubic segment somewhere) or Linear."""
    return any(bool(setting.env.cubic[k]) for k in range(setting.env.n))


# ---- what the rule's model does not return: the ray itself ---------------------------------------------------------------------------
def ray_heights(setting, h0, elevation_deg, m):
    """(H [m + 1], ascending [m + 1]) of the shadow ray from H_0 = h0: the stepper alone, as shadow_model.march drives it;
    ascending[i] is the escape test's second half after step i without its angle bound: b > 0, or for straight rays H_i > H_{i-1}."""
    s, L = setting, setting.o.lib
    st = sm._Stepper()
    ang = float(np.float64(elevation_deg) * (math.pi / 180.0))
    L.oracle_stepper_init(C.byref(st), C.addressof(s.env), int(s.spherical), s.radius, float(h0), ang, int(s.straight), s.step)
    H, up = np.empty(m + 1), np.zeros(m + 1, dtype=bool)
    H[0] = h0
    for i in range(1, m + 1):
        H[i] = L.oracle_stepper_next(C.byref(st)).h
        up[i] = H[i] > H[i - 1] if s.straight else st.b > 0.0
    return H, up


def rose_above(setting, res, spec, result, level):
    """How many SHADOWED rays of `result` were above `level` and ascending at some sample before their block index: the rays a floor
    put at `level` would have released."""
    px, _, _, elev = sm.first_points(res)
    status, block = result.status.ravel(), result.block.ravel()
    n = 0
    for p, el in zip(px, elev):
        if status[p] == sm.SHADOWED and block[p] > 1:
            k = int(block[p])
            H, up = ray_heights(setting, float(np.float64(el) + np.float64(spec[3])), spec[1], k - 1)
            n += bool(np.any((H[1:] > level) & up[1:]))
    return n


# ---- planes made by hand ---------------------------------------------------------------------------------------------------------------
def planes(lat, lon, elev, hit=None):
    """A frame of one row whose pixel p has the first trace point (lat[p], lon[p], elev[p]), or none where hit[p] is false: what
    shadow_model.solve reads, and what atmrt_shadow_mask_planes_device is handed."""
    lat, lon, elev = (np.array(a, dtype=np.float64).ravel() for a in np.broadcast_arrays(lat, lon, elev))
    n = lat.size
    count = np.ones(n, np.uint32) if hit is None else np.asarray(hit).astype(np.uint32)
    return dict(hit_count=count.reshape(1, n), hit_offset=np.arange(n, dtype=np.uint64).reshape(1, n), lat=lat, lon=lon, elevation=elev)


def wide_world(earth=None, atmosphere=None, straight=False, step=100.0):
    """The 5 x 5 mosaic of escape_cases.frame_tiles(wide=True) under a setting: -> (cfg, tiles, top).  The view is not used: the
    planes entry point needs parameters, an atmosphere and terrain, no frame."""
    tiles, top = ec.frame_tiles(wide=True)
    doc = {"view": {"position": {"latitude": 46.5, "longitude": 8.5, "altitude": {"Absolute": top - 150.0}},
                    "frame": {"direction": 270.0, "tilt": 0.0, "fov": 2.0, "max_distance": 20_000.0}},
           "earth_shape": earth or {"Spherical": {"radius": 6371000.0}}, "straight_rays": straight, "simulation_step": step,
           "output": {"width": 4, "height": 4, "generator": "Rectilinear"}}
    if atmosphere is not None:
        doc["atmosphere"] = atmosphere
    return config.Config.from_dict(doc), tiles, top


_RIDGE = {}


def ridge_posts():
    """Every post of the wide mosaic within 150 m of its top, tiles in the order of their keys, row-major: (lat, lon, elev) arrays.
    A post lies at lat0 + row / (n - 1), lon0 + col / (n - 1); get_elev returns its value there."""
    if not _RIDGE:
        tiles, top = ec.frame_tiles(wide=True)
        lat, lon, elev = [], [], []
        for (la, lo) in sorted(tiles):
            posts = tiles[(la, lo)]
            n = posts.shape[0]
            rows, cols = np.nonzero(posts > top - 1.0 - 150.0)
            lat.append(la + rows / (n - 1))
            lon.append(lo + cols / (n - 1))
            elev.append(posts[rows, cols].astype(np.float64))
        _RIDGE.update(lat=np.concatenate(lat), lon=np.concatenate(lon), elev=np.concatenate(elev))
    return _RIDGE["lat"], _RIDGE["lon"], _RIDGE["elev"]


def ridge_points(count):
    """`count` of the ridge posts drawn without replacement by default_rng(0), as planes."""
    lat, lon, elev = ridge_posts()
    pick = np.random.default_rng(0).choice(lat.size, count, replace=False)
    return planes(lat[pick], lon[pick], elev[pick])


# name -> (azimuth_deg, elevation_deg, reach, lift): the real duct of tests/test_gpu_escape.py's _real_duct_scene (0.5 K/m over 300 m
# from 60 m above the top, sup g 2.7) over 1024 ridge points, 150 km: m = 1500
DUCT_SPECS = {"east": (90.0, 0.3, 150_000.0, 2.0), "west": (270.0, 0.15, 150_000.0, 2.0)}


def duct_world():
    _, top = ec.frame_tiles(wide=True)
    return wide_world(atmosphere=atmospheres.inversion(top + 60.0, 300.0, 0.5))


THRESHOLD_SPEC = (90.0, 0.3, 100_000.0, 2.0)
THRESHOLD_LAYERS = (("Linear", 6_371_000.0), ("Natural", 3.0e6), ("Derivatives", 6_371_000.0))
_THRESHOLD = {}


def threshold_worlds():
    """name -> (cfg, tiles, top, certified): both members of three escape_cases.directed_pair layers, bisected against the
    certificate for the setting's own radius, wavelength, step and top."""
    if not _THRESHOLD:
        lib = ec.load_lib()
        for j, (kind, radius) in enumerate(THRESHOLD_LAYERS):
            probe, _, top = wide_world(earth={"Spherical": {"radius": radius}})
            at, thick, g_in, g_out = ec.directed_pair(lib, np.random.default_rng(42_000_000 + j), radius, probe.params.wavelength, top,
                                                      100.0, kind)
            for member, gradient in (("in", g_in), ("out", g_out)):
                world = wide_world(earth={"Spherical": {"radius": radius}}, atmosphere=atmospheres.inversion(at, thick, gradient, kind))
                _THRESHOLD[f"{kind}-{radius:g}-{member}"] = world + (member == "in",)
    return _THRESHOLD


# straight rays on a sphere of 200 km: (reach + step) / R = 0.7505 rad, esc_ang_max = 1.5207963 - 0.7505 = 0.7702963 rad = 44.135
# degrees.  The straight stepper's angle is the launch angle: at 44.2 degrees no ray passes the escape test, at 44.0 every ray that
# is above the floor does.
STRAIGHT_SPHERE_SPECS = {"bites": (90.0, 44.2, 150_000.0, 2.0), "passes": (90.0, 44.0, 150_000.0, 2.0)}


def straight_sphere_world():
    return wide_world(earth={"Spherical": {"radius": 2.0e5}}, straight=True)


# ---- 3. known answers, list edges, range ends ----------------------------------------------------------------------------------------
def flat_world(straight=True, step=100.0):
    """tests/test_shadow_model.py's: no terrain but what a test adds, AzimuthalEquidistant, straight rays."""
    return config.Config.from_dict({
        "view": {"position": {"latitude": 0.5, "longitude": 0.5, "altitude": {"Absolute": 100.0}},
                 "frame": {"direction": 0.0, "fov": 10.0, "tilt": 0.0, "max_distance": 10_000.0}},
        "earth_shape": "AzimuthalEquidistant", "straight_rays": straight, "simulation_step": step,
        "output": {"width": 4, "height": 4, "generator": "Rectilinear"}})


def wall_tile(height=1000, row=660):
    """tests/test_shadow_model.py's: one tile (0..1 N, 0..1 E) that is 0 m but for the posts of latitude row 660 (0.55 N)."""
    posts = np.zeros((1201, 1201), dtype=np.int16)
    posts[row, :] = height
    return {(0, 0): posts}


NAN = math.nan
# (name, the wall tile is loaded, (lat, lon, elev), spec, (status, block)): the literal answers of tests/test_shadow_model.py,
# derived by hand there
KNOWN = [
    ("wall 9 deg", True, (0.5, 0.5, 100.0), (0.0, 9.0, 10_000.0, 0.0), (sm.LIT, 0)),
    ("wall 3.2 deg", True, (0.5, 0.5, 100.0), (0.0, 3.2, 10_000.0, 0.0), (sm.SHADOWED, 56)),
    ("wall 2 deg", True, (0.5, 0.5, 100.0), (0.0, 2.0, 10_000.0, 0.0), (sm.SHADOWED, 55)),
    ("wall reach 5500", True, (0.5, 0.5, 100.0), (0.0, 2.0, 5_500.0, 0.0), (sm.SHADOWED, 55)),
    ("wall reach 5400", True, (0.5, 0.5, 100.0), (0.0, 2.0, 5_400.0, 0.0), (sm.LIT, 0)),
    ("wall behind", True, (0.5, 0.5, 100.0), (180.0, 2.0, 10_000.0, 0.0), (sm.LIT, 0)),
    ("wall along", True, (0.5, 0.5, 100.0), (90.0, 2.0, 10_000.0, 0.0), (sm.LIT, 0)),
    ("wall lift 109", True, (0.5, 0.5, 100.0), (0.0, 2.0, 10_000.0, 109.0), (sm.SHADOWED, 56)),
    ("own sample", True, (0.55, 0.5, 999.0), (180.0, 1.0, 1_000.0, 0.0), (sm.LIT, 0)),
    ("steep down", False, (0.5, 0.5, 100.0), (0.0, -60.0, 1_000.0, 0.0), (sm.SHADOWED, 1)),
    ("guard from -1500", False, (0.5, 0.5, -1500.0), (0.0, 89.0, 1_000.0, 0.0), (sm.SHADOWED, 1)),
    ("guard from -999", False, (0.5, 0.5, -999.0), (0.0, 89.0, 1_000.0, 0.0), (sm.LIT, 0)),
    ("NaN elevation", False, (0.5, 0.5, NAN), (0.0, 10.0, 1_000.0, 0.0), (sm.LIT, 0)),
    # A NaN latitude: every (lat_i, lon_i) is NaN, T_i is 0 or NaN and H_i < T_i false either way (the ray climbs from 100 m): LIT
    ("NaN latitude", True, (NAN, 0.5, 100.0), (0.0, 2.0, 10_000.0, 0.0), (sm.LIT, 0)),
]

LIST_SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)
LIST_PATTERNS = ("all", "none", "alternate", "first", "last", "last65")
LIST_SPECS = {"2deg": (0.0, 2.0, 10_000.0, 0.0), "9deg": (0.0, 9.0, 10_000.0, 0.0)}


def list_hits(n, pattern):
    hit = np.zeros(n, dtype=bool)
    if pattern == "all":
        hit[:] = True
    elif pattern == "alternate":
        hit[::2] = True
    elif pattern == "first":
        hit[0] = True
    elif pattern == "last":
        hit[-1] = True
    elif pattern == "last65":
        hit[-65:] = True
    return hit


def list_points(n):
    """Pixel p stands 1e-4 degrees of latitude (11 m) north of pixel p - 1, from 0.5 N at 100 m: 0.05 degrees from the wall's crest
    (sample 55) down to nothing, so the block index falls from 55 to 1 along the row and a permuted list shows."""
    return 0.5 + 1.0e-4 * np.arange(n), np.full(n, 0.5), np.full(n, 100.0)


# m = 65535: straight rays over the flat world without tiles (T = 0), step 100 m, reach 6,553,500 m, 0.01 degrees down.  H_i = h0 -
# x_i tan 0.01 deg falls 0.01745 m per step; from FAR_BLOCKED the first negative height is H_65535, from FAR_LIT there is none.
FAR_SPEC = (0.0, -0.01, 6_553_500.0, 0.0)
FAR_BLOCKED, FAR_LIT = 1143.79, 1144.0
ODD_AZIMUTHS = (-725.5, 360.0, 1.0e6, -0.0)
