"""Ground on which a slip of one row or one bin of the terrain ceiling table (csrc/atmrt_ceiling.h) shows: isolated spikes on a
plain of 0 m, at a post spacing (31 m at 3601 posts per degree) below the march's step and the width of a bin, so that the table's
neighbouring entries differ and its own slack (the arc's sagitta, two posts, 1 m) does not cover the difference.  Shared by the
CPU tests that prove this (tests/test_ceiling_teeth.py) and the GPU tests that rely on it (tests/test_gpu_ceiling_table.py)."""
import functools

import numpy as np

N_POSTS = 3601          # level-2 spacing
CELL = (46, 8)          # the one tile
OBSERVER = (46.5, 8.5)  # its centre
W, H, FOV, YAW = 64, 32, 12.0, 45.0
STEP, REACH = 100.0, 30_000.0  # 300 steps: the sliced march's three slices of 128
RADIUS = 6_371_000.0
DENSE = (11, 0.02)    # seed, share of posts that are spikes: for the cells
SPARSE = (11, 0.001)  # for the suffix: the last spike of a bin lies well inside the reach (15 % of the suffix entries are 1 m)


def spikes(seed, n, p):
    """n x n posts of 0 m, a share p of them drawn from 300 .. 3000 m"""
    rng = np.random.default_rng(seed)
    posts = np.zeros((n, n), dtype=np.int16)
    mask = rng.random((n, n)) < p
    posts[mask] = rng.integers(300, 3000, size=int(mask.sum())).astype(np.int16)
    return posts


@functools.lru_cache(maxsize=None)
def tile(which, n=N_POSTS):
    """{cell: posts} of the dense or the sparse spike tile (built once per process; do not write to it)"""
    seed, p = DENSE if which == "dense" else SPARSE
    posts = spikes(seed, n, p)
    posts.setflags(write=False)
    return {CELL: posts}


def shifted(plane, rows=0, bins=0):
    """The plane as a march would see it whose row index were `rows` and whose bin index `bins` too high: entry [i][j] is
    plane[i + rows][j + bins] (clamped at the table's border; the last column, the one of the rays outside the bins, stays)."""
    n_rows, stride = plane.shape
    i = np.clip(np.arange(n_rows) + rows, 0, n_rows - 1)
    j = np.clip(np.arange(stride - 1) + bins, 0, stride - 2)
    out = plane.copy()
    out[:, :-1] = plane[i][:, j]
    return out


SHIFTS = {"row + 1": (1, 0), "row - 1": (-1, 0), "bin + 1": (0, 1), "bin - 1": (0, -1)}


# The views of the marched frames (all from OBSERVER along YAW, 64 x 32, fov 12, 300 steps), chosen by tests/test_ceiling_teeth.py:
#   near  the view of the table tests: rays pass low between dense spikes 7 - 27 km away — a slip of one ROW changes hundreds of pixels
#   far   300 steps of 200 m: a bin is 80 - 160 m wide beyond 30 km, more than the cover's two posts — a slip of one BIN shows
#   up    from 50 m upwards over the sparse tile: half the rays leave above their bin's suffix — the suffix plane is used
VIEWS = {
    "near": dict(tile="dense", altitude=800.0, tilt=0.0, step=STEP, reach=REACH),
    "far": dict(tile="dense", altitude=1500.0, tilt=-1.0, step=200.0, reach=60_000.0),
    "up": dict(tile="sparse", altitude=50.0, tilt=2.5, step=STEP, reach=REACH),
}


def config(view, yaw=YAW, fov=FOV, observer=OBSERVER, tilt=None, terrain_alpha=None):
    """The Config of a view: Rectilinear, a Spherical earth of RADIUS, US-76, refracted rays, the observer at an absolute altitude"""
    from atm_raytracer_amd.config import Config
    v = VIEWS[view]
    d = {
        "view": {"position": {"latitude": observer[0], "longitude": observer[1], "altitude": {"Absolute": v["altitude"]}},
                 "frame": {"direction": yaw, "fov": fov, "tilt": v["tilt"] if tilt is None else tilt, "max_distance": v["reach"]}},
        "earth_shape": {"Spherical": {"radius": RADIUS}},
        "straight_rays": False,
        "simulation_step": v["step"],
        "output": {"width": W, "height": H, "generator": "Rectilinear"},
    }
    if terrain_alpha is not None:
        d["scene"] = {"terrain_alpha": terrain_alpha}
    return Config.from_dict(d)


# ---- the marched frames of tests/test_gpu_ceiling_table.py, by name (the variant children build them from the same code) ----
EDGE_OBSERVER = (46.5, 8.97)  # 2.3 km west of the edge between the 3601-post tile and a 301-post one


def two_resolutions():
    """the dense tile and, east of it, spikes at 301 posts: the rays cross from 31 m posts to 370 m posts"""
    coarse = spikes(12, 301, 0.05)
    coarse.setflags(write=False)
    return {CELL: tile("dense")[CELL], (CELL[0], CELL[1] + 1): coarse}


def marched(name):
    """(Config, tiles) of a marched frame: a view of VIEWS, '<view>_translucent' (terrain alpha 0.5), 'yaw_180' (atan2's cut inside
    the bins), 'nadir' (tilt -80, fov 60: the bins reach CEIL_MAX_BINS and some rays lie past the last one), 'two_resolutions',
    'objects' (80 cylinders, cones, frusta and billboards 1 - 25 km away over translucent spikes)."""
    if name in VIEWS:
        return config(name), tile(VIEWS[name]["tile"])
    if name.endswith("_translucent"):
        view = name[:-len("_translucent")]
        return config(view, terrain_alpha=0.5), tile(VIEWS[view]["tile"])
    if name == "yaw_180":
        return config("near", yaw=180.0, tilt=-1.0), tile("dense")
    if name == "nadir":
        return config("near", tilt=-80.0, fov=60.0), tile("dense")
    if name == "two_resolutions":
        return config("near", yaw=90.0, observer=EDGE_OBSERVER), two_resolutions()
    if name == "objects":
        from atm_raytracer_amd import synth
        cfg = config("near", terrain_alpha=0.5)
        synth.add_objects(cfg, n_cyl=60, n_bill=20, dist=(1_000.0, 25_000.0), spread_deg=6.0, height=(200.0, 1500.0))
        return cfg, tile("dense")
    raise KeyError(name)


def frame_hash(result):
    """sha256 over the bits of every pixel plane and trace-point field, n_hits and ray_steps of a frame"""
    import hashlib
    from util import FIELDS_HIT, FIELDS_PIXEL, bits
    h = hashlib.sha256()
    for k in FIELDS_PIXEL + FIELDS_HIT:
        h.update(np.ascontiguousarray(bits(result[k])).tobytes())
    h.update(repr((int(result["n_hits"]), int(result["ray_steps"]))).encode())
    return h.hexdigest()
