"""What the escape certificate's tests share (tests/test_escape_certificate.py, tests/test_escape_march_rule.py,
tests/test_gpu_escape.py and its child processes): the certificate's entry point, g(h) = (R + h) |dn(h)| / n(h) from the libm oracle,
and the seeded cases.  Nothing here needs a device: atmrt_escape_certificate is host code."""
import ctypes as C
import math
import os

import numpy as np

import atmospheres
from atm_raytracer_amd import _lib, config

INF = float("inf")
H_END = 1.0e7  # the certificate sweeps pieces up to here and applies a rule to the tail above
RADII = [6_371_000.0, 3.0e6, 2.0e5, 6.0e8, atmospheres.shape_radius("Wgs84")]
# the directed family needs a radius at which US-76's troposphere itself is certified and a layer of at most a few K/m decides;
# at 6.0e8 m the bound is 14 at the ground (nothing below 25 km is certified), at 2.0e5 m it is 0.005 (no layer below 2 K/m matters)
DIRECTED_RADII = [6_371_000.0, 3.0e6, atmospheres.shape_radius("Wgs84")]


def load_lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def certificate(lib, atm, radius, wavelength, top, step, spherical=1, straight=0):
    """atmrt_escape_certificate -> (floor, from, worst); `atm` is a definition (dict), None (US-76) or a compiled POD."""
    if atm is None:
        atm = config.us76()
    elif isinstance(atm, dict):
        atm = config._atmosphere(atm)
    out = (C.c_double * 3)()
    assert lib.atmrt_escape_certificate(C.byref(atm), wavelength, spherical, radius, straight, step, top, out) == 0
    return tuple(out)


class G:
    """g(h) = (R + h) |dn(h)| / n(h) of one atmosphere from an oracle: `dn` is the stepper's own central difference over +-1 cm."""

    def __init__(self, oracle, atm, radius, wavelength):
        if atm is None:
            pod = None
        elif isinstance(atm, dict):
            pod = config._atmosphere(atm)
        else:
            pod = atm
        self.env = oracle.env(pod, wavelength)
        self.radius = radius
        self._n, self._dn, self._ref = oracle.lib.oracle_n, oracle.lib.oracle_dn, C.byref(self.env)
        self.edges = [float(self.env.from_[k]) for k in range(1, self.env.n)]  # lower boundaries of segments 1 .. n - 1
        self.cubic = [bool(self.env.cubic[k]) for k in range(self.env.n)]

    def __call__(self, h):
        """NaN where n is NaN (a temperature <= 0: no ray gets past there)."""
        n = self._n(self._ref, h)
        return (self.radius + h) * abs(self._dn(self._ref, h)) / n

    def tol(self, h):
        """The rounding of one sample: two roundings of n ~ 1 (2^-53 each) in a difference over 2 cm."""
        return (self.radius + abs(h)) * 2.0 * 2.0 ** -53 / 0.02

    def segment_of(self, h):
        k = 0
        for e in self.edges:
            if h >= e:
                k += 1
        return k

    def bounds(self, k):
        """[lo, hi) of segment k."""
        return (self.edges[k - 1] if k > 0 else -INF), (self.edges[k] if k < len(self.edges) else INF)


def around(b):
    """The samples of a boundary (a segment's edge, a Spline's knot): where a +-1 cm stencil straddles it or just does not."""
    out = [b, math.nextafter(b, INF), math.nextafter(b, -INF)]
    for d in (0.005, 0.01, 0.02):
        out += [b - d, b + d]
    return out


def golden_max(f, a, b, iterations=60):
    """Golden-section search for the maximum of f on [a, b] -> (x, f(x))."""
    r = (math.sqrt(5.0) - 1.0) / 2.0
    c, d = b - r * (b - a), a + r * (b - a)
    fc, fd = f(c), f(d)
    for _ in range(iterations):
        if fc > fd:
            b, d, fd = d, c, fc
            c = b - r * (b - a)
            fc = f(c)
        else:
            a, c, fc = c, d, fd
            d = a + r * (b - a)
            fd = f(d)
    return (c, fc) if fc > fd else (d, fd)


def samples_above(g, start):
    """Per segment that reaches above `start`: (k, sorted sample altitudes in [start, H_END]), as the soundness check wants them:
    200 points spaced geometrically from the segment's lower end, and the surroundings of every boundary above `start`."""
    out = []
    for k in range(len(g.edges) + 1):
        lo, hi = g.bounds(k)
        a, b = max(lo, start), min(hi, H_END)
        if not a < b:
            continue
        pts = [a, b if hi > H_END else math.nextafter(b, -INF)]
        pts += list(a + np.geomspace(1.0e-3, b - a, 200)) if b - a > 1.0e-3 else []
        for e in (lo, hi):
            if math.isfinite(e):
                pts += around(e)
        out.append((k, sorted(float(h) for h in set(pts) if a <= h < hi and h <= H_END and h >= lo)))
    return out


def sup_g(g, start, tail=True):
    """(sup, argmax, kind of the argmax's segment) of the sampled g over [start, 1e9 m): the grid of samples_above, refined by a
    golden-section search around each Spline interval's best grid point, and 50 points of the tail.  Also checks that NaNs (T <= 0)
    only ever end a segment: once a sample is NaN, every higher one of that segment is."""
    best, where, kind = 0.0, None, None
    for k, pts in samples_above(g, start):
        vals = [g(h) for h in pts]
        seen_nan = False
        for h, v in zip(pts, vals):
            if v != v:
                seen_nan = True
                continue
            assert not seen_nan, f"segment {k}: n is a number at {h} m above a NaN"
            if v > best:
                best, where, kind = v, h, g.cubic[k]
        if g.cubic[k] and len(pts) > 2:
            fin = [(v, i) for i, v in enumerate(vals) if v == v]
            if fin:
                i = max(fin)[1]
                a, b = pts[max(i - 1, 0)], pts[min(i + 1, len(pts) - 1)]
                x, v = golden_max(lambda h: g(h) if g(h) == g(h) else -1.0, a, b)
                if v > best:
                    best, where, kind = v, x, True
    if tail:
        k = len(g.edges)
        seen_nan = False
        for h in np.geomspace(H_END, 1.0e9, 50):
            v = g(float(h))
            if v != v:
                seen_nan = True
                continue
            assert not seen_nan, f"tail: n is a number at {h} m above a NaN"
            if v > best:
                best, where, kind = v, float(h), g.cubic[k]
    return best, where, kind


# ---- the directed family -----------------------------------------------------------------------------------------------------------
def directed_pair(lib, rng, radius, wavelength, top, step, kind):
    """One inversion layer (atmospheres.inversion) near `top` whose gradient is bisected against the certificate: returns
    (at, thick, g_in, g_out) with g_in the steepest gradient found that is still certified from top - step up and g_out the gentlest
    found that is refused; they differ by 2^-40 of the bracket."""
    thick = float(rng.uniform(100.0, 500.0))
    at = max(50.0, top - step + float(rng.uniform(-0.5 * thick, 1500.0)))

    def certified(gradient):
        _, start, _ = certificate(lib, atmospheres.inversion(at, thick, gradient, kind), radius, wavelength, top, step)
        return start == top - step

    lo, hi = atmospheres.US76_LAPSE, 1.0
    assert certified(lo) and not certified(hi), (at, thick, kind, radius)
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        if certified(mid):
            lo = mid
        else:
            hi = mid
    return at, thick, lo, hi


def duct_gradient(oracle, radius, wavelength, at, thick, target, kind="Linear"):
    """The gradient of the layer for which sup g over the layer is `target` (bisected against the oracle; g grows with the gradient)."""
    def sup(gradient):
        g = G(oracle, atmospheres.inversion(at, thick, gradient, kind), radius, wavelength)
        return max(g(float(h)) for h in np.linspace(at + 0.02, at + thick - 0.02, 41))

    lo, hi = 0.0, 3.0
    for _ in range(30):
        mid = 0.5 * (lo + hi)
        if sup(mid) < target:
            lo = mid
        else:
            hi = mid
    return hi


# ---- the certificate's sweep -------------------------------------------------------------------------------------------------------
FAMILIES = ("configurations", "extremes", "long", "directed-in", "directed-out", "named")


def certificate_case(lib, seed):
    """Seed -> dict(family, atm (definition or None for US-76), radius, wavelength, top, step).  A sixth of the seeds each: the three
    random families of the GPU sweeps, the directed family just inside and just outside the bound, and the named atmospheres."""
    rng = np.random.default_rng(31_000_000 + seed)
    family = FAMILIES[seed % 6]
    radius = float(rng.choice(DIRECTED_RADII if family.startswith("directed") else RADII))
    wavelength = float(rng.uniform(300e-9, 1100e-9))
    top = float(rng.choice([rng.uniform(1.0, 100.0), rng.uniform(100.0, 3000.0), rng.uniform(3000.0, 9000.0), 1780.0]))
    step = float(rng.choice([rng.uniform(5.0, 40.0), rng.uniform(40.0, 1500.0), 100.0]))
    case = dict(seed=seed, family=family, radius=radius, wavelength=wavelength, top=top, step=step, kind=None)
    if family == "configurations":
        case["atm"] = atmospheres.configuration_atmosphere(rng)
    elif family == "extremes":
        case["atm"] = atmospheres.extreme_atmosphere(rng)
    elif family == "long":
        case["atm"] = atmospheres.long_atmosphere(rng)
    elif family == "named":
        case["atm"] = [atmospheres.WILD_SPLINE, atmospheres.OVERFLOWING_SPLINE, None][(seed // 6) % 3]
    else:
        # the pair shares its stream: seed 6 j + 3 is the certified member, 6 j + 4 its refused twin
        rng = np.random.default_rng(32_000_000 + seed // 6)
        radius = float(rng.choice(DIRECTED_RADII))
        wavelength = float(rng.uniform(300e-9, 1100e-9))
        top = float(rng.choice([rng.uniform(1.0, 100.0), rng.uniform(100.0, 3000.0), rng.uniform(3000.0, 9000.0), 1780.0]))
        step = float(rng.choice([rng.uniform(5.0, 40.0), rng.uniform(40.0, 1500.0), 100.0]))
        kind = atmospheres.INVERSION_KINDS[(seed // 6) % 4]
        at, thick, g_in, g_out = directed_pair(lib, rng, radius, wavelength, top, step, kind)
        case.update(radius=radius, wavelength=wavelength, top=top, step=step, kind=kind, at=at, thick=thick,
                    gradient=g_in if family == "directed-in" else g_out)
        case["atm"] = atmospheres.inversion(at, thick, case["gradient"], kind)
    return case


# ---- frames that tempt a wrong escape (tests/test_gpu_escape.py) -------------------------------------------------------------------
SPHERICAL_EARTHS = ["SimpleSphere", {"Spherical": {"radius": 6371000.0}}, {"Spherical": {"radius": 3.0e6}}, "Wgs84",
                    {"Ellipsoid": {"a": 6378137.0, "b": 6300000.0}}]
FLAT_EARTHS = ["AzimuthalEquidistant", "FlatDistorted", {"ObserverAe": {"proj_radius": 6371000.0}}, "SimpleObserverAe"]
_TILES = {}


def frame_tiles(wide=False):
    """The one-tile mosaic of the parity sweeps — `wide`: 5 x 5 tiles, 250 km of terrain for a trapped ray to come down on — and
    its skip_above (every post is below it)."""
    from atm_raytracer_amd import synth
    if wide not in _TILES:
        _TILES[wide] = synth.synth_tiles([44, 45, 46, 47, 48], [6, 7, 8, 9, 10], level=301) if wide else synth.synth_tiles([46], [8], level=301)
    return _TILES[wide], float(max(int(t.max()) for t in _TILES[wide].values())) + 1.0


def frame_case(lib, oracle, seed):
    """Seed -> dict(cfg, tiles, top, kind of atmosphere, atm definition, radius or None (flat), ...): a small Rectilinear frame of
    150 .. 400 km whose atmosphere is, in a third of the seeds each, a layer next to the certificate's threshold (either side), a real
    duct (sup g 1.5 .. 5 by the oracle) around the mosaic's top with the observer just under it, or one of the random families."""
    from atm_raytracer_amd import synth
    kind = ("threshold", "duct", "random")[seed % 3]
    tiles, top = frame_tiles(wide=kind == "duct")
    rng = np.random.default_rng(35_000_000 + seed)
    flat = seed % 10 == 9
    earth = (FLAT_EARTHS if flat else SPHERICAL_EARTHS)[int(rng.integers(4 if flat else 5))]
    radius = atmospheres.shape_radius(earth)
    step = float(rng.choice([rng.uniform(100.0, 500.0), 100.0, 250.0]))
    wavelength = float(rng.uniform(400e-9, 700e-9))
    altitude = top + float(rng.uniform(-300.0, 3000.0))
    gen_radius = radius or 6_371_000.0  # the layer is built for the frame's own radius (a flat earth refracts over none)
    if kind == "threshold":
        layer = atmospheres.INVERSION_KINDS[(seed // 3) % 4]
        at, thick, g_in, g_out = directed_pair(lib, rng, gen_radius, wavelength, top, step, layer)
        atm = atmospheres.inversion(at, thick, g_in if (seed // 3) % 2 == 0 else g_out, layer)
        if rng.uniform() < 0.5:
            altitude = at - float(rng.uniform(0.0, 200.0))
    elif kind == "duct":
        layer = atmospheres.INVERSION_KINDS[(seed // 3) % 4]
        # the layer's base within reach of the top: a ray is turned back only if it enters the layer at less than
        # sqrt(2 (sup g - 1) thick / R) (0.4 .. 1.1 degrees here), and it gains sqrt(2 D 0.83 / R) on the D metres up to the base
        at, thick = top + float(rng.uniform(-100.0, 80.0)), float(rng.uniform(200.0, 400.0))
        atm = atmospheres.inversion(at, thick, duct_gradient(oracle, gen_radius, wavelength, at, thick, float(rng.uniform(1.5, 5.0)), layer), layer)
        altitude = min(at, top - 100.0) - float(rng.uniform(20.0, 80.0))  # under the layer and the peaks: rays rise into it, turn, and
        # come down onto the mosaic's ridges, which lie west of the observer
    else:
        layer, at, thick = None, None, None
        atm = [atmospheres.configuration_atmosphere, atmospheres.extreme_atmosphere, atmospheres.long_atmosphere][(seed // 3) % 3](rng)
    w, h = int(rng.integers(4, 33)), int(rng.integers(4, 21))
    direction, tilt, fov = float(rng.uniform(0.0, 360.0)), float(rng.uniform(-2.0, 3.0)), float(rng.uniform(2.0, 30.0))
    if kind == "duct":  # rows a fraction of a degree apart around the horizontal: only rays within ~0.5 degrees of it are trapped
        direction, tilt, fov = float(rng.uniform(250.0, 290.0)), float(rng.uniform(-0.2, 0.4)), float(rng.uniform(2.0, 5.0))
    doc = {"view": {"position": {"latitude": 46.5, "longitude": 8.5, "altitude": {"Absolute": altitude}},
                    "frame": {"direction": direction, "tilt": tilt, "fov": fov,
                              "max_distance": float(rng.uniform(150_000.0, 400_000.0))}},
           "earth_shape": earth, "straight_rays": bool(seed % 5 == 4), "simulation_step": step, "wavelength": wavelength,
           "scene": {"terrain_alpha": float(rng.choice([1.0, 0.5]))},
           "output": {"width": w, "height": h, "generator": "Rectilinear"}}
    if atm is not None:
        doc["atmosphere"] = atm
    cfg = config.Config.from_dict(doc)
    if rng.uniform() < 1.0 / 3.0:
        c0 = int(rng.integers(0, w))
        cfg.params.col_begin, cfg.params.col_end = c0, int(rng.integers(c0 + 1, w + 1))
    objects = bool(rng.uniform() < 1.0 / 3.0)
    if objects:
        synth.add_objects(cfg, n_cyl=20, n_bill=6, dist=(2_000.0, 30_000.0), spread_deg=15.0, radius=(100.0, 300.0),
                          height=(2_000.0, 4_000.0), bill_w=(200.0, 500.0), bill_h=(2_000.0, 4_000.0), seed=int(rng.integers(1 << 30)))
    return dict(seed=seed, cfg=cfg, tiles=tiles, top=top, kind=kind, atm=atm, radius=radius, flat=flat, step=step, wavelength=wavelength,
                altitude=altitude, objects=objects, at=at, thick=thick, straight=bool(seed % 5 == 4))



def real_duct_scene(kind="Linear"):
    """0.5 K/m over 300 m (sup g 2.7) with its base 60 m above the top of a 5 x 5 mosaic and the observer 150 m under the top, looking west over its ridges, rows 0.04
    degrees apart around the horizontal: rays that leave at 0 .. 0.3 degrees rise into the layer and are turned back.  `kind`: the
    layer as three Linear functions or as a Spline with that boundary condition (atmospheres.inversion)."""
    tiles, top = frame_tiles(wide=True)  # 250 km of terrain to come down on
    atm = atmospheres.inversion(top + 60.0, 300.0, 0.5, kind)
    cfg = config.Config.from_dict({
        "view": {"position": {"latitude": 46.5, "longitude": 8.5, "altitude": {"Absolute": top - 150.0}},
                 "frame": {"direction": 270.0, "tilt": 0.15, "fov": 2.0, "max_distance": 250_000.0}},
        "earth_shape": {"Spherical": {"radius": 6371000.0}}, "simulation_step": 100.0, "atmosphere": atm,
        "output": {"width": 48, "height": 32, "generator": "Rectilinear"}})
    return dict(cfg=cfg, tiles=tiles, top=top, atm=atm, radius=6371000.0, flat=False, straight=False, step=100.0,
                wavelength=cfg.params.wavelength, altitude=top - 150.0)


def frame_certificate(lib, case):
    """The certificate the frame's context computes: its atmosphere, shape radius, step and the mosaic's skip_above."""
    return certificate(lib, case["atm"], case["radius"] or 0.0, case["wavelength"], case["top"], case["step"],
                       spherical=0 if case["flat"] else 1, straight=1 if case["straight"] else 0)


def frame_rays(oracle, case, frame, col=0):
    """The oracle's paths (ray_paths: no terrain) of column `col` of the computed columns of the frame, one per row, to max_distance:
    (hit_count of the pixel, distance of its first trace point or None, h[0 .. n]) per row."""
    p = case["cfg"].params
    angles = np.ascontiguousarray(frame["elevation_angle"][:, col])
    n_steps = int(p.frame.max_distance / case["step"])
    _, h = oracle.ray_paths(p, case["altitude"], angles, case["step"], n_steps, case["straight"], case["cfg"].atmosphere)
    hits, offs = frame["hit_count"][:, col], frame["hit_offset"][:, col]
    return [(int(c), float(frame["distance"][int(o)]) if c else None, row) for c, o, row in zip(hits, offs, h)]
