"""Command line mirroring the reference's subcommands (src/main.rs:17-39) over the C ABI:

    python -m atm_raytracer_amd gen -c CONFIG.yaml [--output OUT.png] [--metadata OUT.npz|OUT.dat]
                                    [--visibility-map OUT.npz [--map-cell ARCSEC] [--map-all]]
                                    [--landmarks FILE.csv [--landmark-radius ARCSEC] [--landmarks-all] [--landmarks-out OUT.csv]]
                                    [--sight-lines FILE.csv [--sight-out OUT.csv] [--sight-fan LO HI] [--sight-rounds N]]
                                    [--viewshed OUT.npz [--viewshed-az LO HI N] [--viewshed-reach M] [--viewshed-height M]
                                     [--viewshed-fan LO HI K]]
                                    [--viewshed-map OUT.npz [--map-cell ARCSEC] [--viewshed-observers FILE.csv]]
                                    [--horizon OUT.csv [--horizon-az LO HI N] [--horizon-reach M] [--horizon-fan LO HI K]
                                     [--horizon-rounds N]]
                                    [--shadows [--shadow-reach M] [--shadow-lift M] [--shadow-light AZ EL] [--shadow-per-point]]
                                    [--shadow-lights FILE.csv [--shadow-lights-out OUT.npz] [--shadow-reach M] [--shadow-lift M]]
                                    [--shadow-true [--sky-table-alt LO HI N] [--sky-table-el LO HI N]]
                                    [--sun AZ EL [--sun-radius DEG]] [--moon AZ EL] [--sky-top M] [--sky-step M] [--sky-floor M]
                                    [--sky-out OUT.npz] [--refraction-table OUT.csv [--sky-fan LO HI K]]
                                    [--sky-colour [--sky-tau R G B] [--sky-exposure G] [--sun-limb R G B] [--air-mass-ref M]]
    python -m atm_raytracer_amd output-atm CONFIG.yaml [-a MIN] [-b MAX] [-s STEP] [-c]
    python -m atm_raytracer_amd output-ray-paths CONFIG.yaml [-h H] [-a MIN] [-b MAX] [-s DEG] [-r STEP] [-c CUTOFF] [-o OUTSTEP]
    python -m atm_raytracer_amd output-elev-profile CONFIG.yaml [-a AZIM] [-s STEP] [-c CUTOFF]

Column formats follow src/atm_printer.rs:37-46, src/ray_path.rs:65-103 and src/elev_profile.rs:43-64.  `gen` writes the
image of renderer::output_image: draw_image, then — on the device image, before its one download — the azimuth / elevation
ticks, the flat-horizon line and the eye-level line of `output` (renderer/mod.rs:416-431); the tick labels are drawn on the
host with Pillow in DejaVu Sans where the machine has that font (a warning and no labels where not).  On request it also
writes the per-pixel metadata as a compressed .npz (the reference's bincode+gzip layout depends on crates that are absent).
`--visibility-map` (no reference counterpart) bins the frame's trace points over a latitude / longitude grid on the device — the
frame's bounds snapped outward to multiples of the cell, 3 arcseconds unless --map-cell says otherwise; the first trace point of
every pixel, or all of them with --map-all — and writes count, min_distance, lat0, lon0, cell_lat, cell_lon, n_points, n_binned,
n_outside, n_skipped and n_updates to an .npz.
`--landmarks` (no reference counterpart) reads name,lat,lon rows and finds, on the device, the trace point nearest to each within
--landmark-radius (3 arcseconds unless said otherwise; lon_scale = cos(lat); the first trace point of every pixel, or all of them
with --landmarks-all), writes name,lat,lon,found,x,y,point,offset_arcsec,distance_m,elevation_m,n_within to --landmarks-out or to
stdout, and marks the found ones in the image with a short line and their name.  Not found means no trace point that near: outside
the field of view and hidden behind terrain look the same.
`--sight-lines` (no reference counterpart) tells them apart: it reads name,lat,lon[,height] rows, turns each into an azimuth and a
distance from the observer under the configured earth model, and solves on the device at which elevation angle the point `height`
metres above the ground there appears (first fan --sight-fan, -5 5 unless said otherwise, narrowed --sight-rounds times, 3) or how
many metres of it the terrain hides and where that terrain is.  The table — name, azimuth_deg, distance_m, status (seen, hidden,
above_fan, below_fan), angle_deg, hidden_m, ground_m, resolution_deg, the blocking point's block_distance_m, block_lat, block_lon,
block_elevation_m, and the Fast generator's pixel x, y that (azimuth, angle) falls in for the configured frame, empty outside it —
goes to --sight-out or to stdout.
`--viewshed` (no reference counterpart) answers the same question for a whole area: for N azimuths from LO to HI (--viewshed-az; the
frame's field of view at one azimuth per pixel column unless said otherwise) and every sample of the lattice as far as
--viewshed-reach (max_distance), whether a point --viewshed-height metres above the ground (0) is seen over a fan of K rays between
LO and HI degrees (--viewshed-fan, -5 5 64), and how many metres of it are hidden.  OUT.npz holds the planes k_star, status (0 seen,
1 hidden, 2 above_fan, 3 below_fan), hidden, block_index, ground, lat and lon as [N][m] arrays, the lattice d, the azimuths, the
fan's angles and the height.
`--viewshed-map` (no reference counterpart) bins that viewshed (the same --viewshed-az, -reach, -height and -fan) over a latitude /
longitude grid on the device, --map-cell arcseconds a cell (3), laid around the observer as far as the lattice reaches: OUT.npz holds
n_samples, n_seen and min_hidden as [n_lat][n_lon] arrays, rows south to north, the grid's lat0, lon0, cell_lat, cell_lon, n_lat, n_lon
and the call's stats_n_samples, stats_n_binned, stats_n_outside, stats_n_skipped, stats_n_seen.  With --viewshed-observers FILE.csv
(columns lat, lon, altitude — of the configured altitude kind) it is the cumulative form over a grid that holds every observer's
reach: observers_seeing (from how many observers a cell is seen) and min_hidden (the smallest over them), and the grid.
`--horizon` (no reference counterpart) asks where the skyline is: for N azimuths from LO to HI (--horizon-az; one per pixel column of
the frame unless said otherwise) and the terrain within --horizon-reach (max_distance), the refracted elevation angle at which
terrain ends and sky begins, bracketed between the highest blocked ray and the ray above it — first fan --horizon-fan (-5 5 64),
narrowed --horizon-rounds times (3) — and the ridge that forms it.  OUT.csv has one row per azimuth: azimuth_deg, status (found,
above_fan, below_fan), angle_clear_deg, angle_blocked_deg, resolution_deg, ridge_distance_m, ridge_lat, ridge_lon, ridge_elevation_m.
`--shadows` (no reference counterpart) casts shadows into the image: from the first trace point of every pixel a ray is marched toward
the light through the same atmosphere, --shadow-reach metres far (max_distance, at most 65535 steps) from --shadow-lift metres above
the point (0), and a point whose ray meets terrain is drawn at the Shading method's ambient light.  The light is the Shading
configuration's (azimuth = frame direction + 180 - light_dir, elevation = 90 - light_zenith_angle) unless --shadow-light AZ EL names
the azimuth toward it and its elevation in degrees; both are taken as the same at every point of the frame.  With
--shadow-per-point the light is a direction in the world instead — the Shading configuration's own light_dir vector, so that slopes
and shadows share one light, or --shadow-light AZ EL as seen from the observer — and every point marches in its own local direction
toward it (include/atmrt.h, "shadow lights").
`--shadow-lights FILE.csv` (no reference counterpart) asks the same for up to 64 lights in one call, a day's sun path for instance:
rows of azimuth_deg,elevation_deg as seen from the observer, each turned into a world-frame vector there; --shadow-reach and
--shadow-lift as above.  OUT.npz (--shadow-lights-out, shadow_lights.npz) holds lit_mask [height][width] u64 (bit l: light l reaches
the pixel's first trace point), lit_count (its popcount, taken on the host), dirs [n][3], azimuth_deg, elevation_deg and the call's
stats_none, stats_lit, stats_shadowed, stats_integrated_steps, stats_escaped_rays.
`--shadow-true` (with --shadows --shadow-per-point, and with --shadow-lights) takes the given angles as the light's TRUE direction,
as --sun takes the sun's: every shadow ray is launched where its light APPEARS from the point, up to 0.55 degrees higher at the
horizon (include/atmrt.h, "apparent elevation"), so the terrain is lit from where the sun is drawn.  With --sun AZ EL and no
--shadow-light the light is the sun.  The refraction table behind it spans --sky-table-alt LO HI N metres (0 9000 33) and
--sky-table-el LO HI N degrees (-4 88 4601: above 89.5 degrees a 1000 m sky step loses the ray); --sky-top, --sky-step and
--sky-floor apply to its rays as they do for --sun.  Without --sky-step the table is marched at the simulation step, ten times the
work at the usual 100 m; `--sky-step 1000` is the recommended setting —
the closure of 1.1e-4 degrees and the 12 ms of the default table's build were measured with it.
`--sun AZ EL` and `--moon AZ EL` (no reference counterpart) draw a disc where the frame's sky pixels look at it once their rays
have left the atmosphere (include/atmrt.h, "sky rays"): AZ and EL are the body's TRUE direction in degrees, as seen from the observer
with no atmosphere, --sun-radius its angular radius (0.2666; the moon's is the same).  Every pixel without a trace point is marched
through the atmosphere to --sky-top metres (100000) in steps of --sky-step metres (the simulation step) and given up below
--sky-floor metres (0); near the horizon the disc comes out lifted and flattened, and terrain cuts it.  The discs are drawn on the
device image before the overlay: ticks and lines stay on top.  `--sky-out OUT.npz` holds true_elevation, status (0 none, 1 exit,
2 ground, 3 inside, 4 lost), steps and body as [height][width] arrays and the call's stats_none, stats_exit, stats_ground,
stats_inside, stats_lost, stats_integrated_steps.
`--sky-colour` (no reference counterpart; with or without --sun / --moon) shades the sky by air mass (include/atmrt.h, "sky light"):
the sky march also integrates the refractivity along every ray, and its quotient by the same integral taken vertically from
--air-mass-ref metres (0) is the pixel's relative air mass X.  A sky pixel becomes white * --sky-exposure (4) * (1 - exp(-tau X)) per
channel with the zenith optical depths --sky-tau R G B (0.06 0.11 0.24: a blue zenith, a horizon that saturates to white); a disc pixel
its body's colour times exp(-tau X) — the low sun reddens and dims — times the limb darkening 1 - u (1 - mu) with --sun-limb R G B (0.5
0.6 0.75).  These numbers are this project's choice.  --sky-out then also holds column, air_mass and zenith_column.
`--refraction-table OUT.csv` marches K rays from the observer's altitude at launch elevations from LO to
HI degrees (--sky-fan, 0 60 61) with the same --sky-top, --sky-step and --sky-floor: rows of
elevation_deg,status,steps,true_elevation_deg,refraction_deg (the last two empty unless the ray exits).
Floats are printed with Python's repr, the shortest round-trip form like Rust's `{}`.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

from . import _abi, config, generators


def _ctx_with_terrain(cfg, cfg_path):
    ctx = generators.Context()
    folder = os.path.join(os.getcwd(), cfg.terrain_folder)  # env::current_dir().push(terrain_folder), generator/mod.rs:57-58
    terrain = generators.Terrain.from_folder(folder, ctx)
    return ctx, terrain


def _configure(ctx, cfg):
    ctx.check(ctx.lib.atmrt_set_params(ctx.handle, C.byref(cfg.params)))
    ctx.check(ctx.lib.atmrt_set_atmosphere(ctx.handle, C.byref(cfg.atmosphere)))


def find_label_font():
    """DejaVuSans.ttf (the reference embeds its own copy, renderer/mod.rs:20) from the system fonts or matplotlib's data; None if absent."""
    import glob
    dirs = ["/usr/share/fonts", "/usr/local/share/fonts", os.path.expanduser("~/.fonts"), os.path.expanduser("~/.local/share/fonts")]
    try:
        import matplotlib
        dirs.append(os.path.join(matplotlib.get_data_path(), "fonts", "ttf"))
    except ImportError:
        pass
    for d in dirs:
        hits = sorted(glob.glob(os.path.join(d, "**", "DejaVuSans.ttf"), recursive=True))
        if hits:
            return hits[0]
    return None


def draw_labels(img, ticks):
    """draw_text_mut of draw_ticks (renderer/mod.rs:292-321): white, 15 px high, a horizontal tick's label at (x - 8, size + 5), a
    vertical tick's at (size + 5, y - 7); strings and positions come from the library.  Glyph pixels are Pillow's, not rusttype's."""
    labelled = [t for t in ticks if t["labelled"]]
    if not labelled:
        return
    path = find_label_font()
    if path is None:
        print("WARNING: DejaVuSans.ttf not found on this machine: tick labels are left off", file=sys.stderr)
        return
    from PIL import ImageDraw, ImageFont
    # rusttype's Scale is ascent - descent in pixels: 15 px over DejaVu Sans's (1901 + 483) / 2048 em is an em of 12.9 px
    font = ImageFont.truetype(path, 13)
    draw = ImageDraw.Draw(img)
    for t in labelled:
        xy = (t["size"] + 5, t["pos"] - 7) if t["vertical"] else (t["pos"] - 8, t["size"] + 5)
        draw.text(xy, t["label"], fill=(255, 255, 255), font=font, anchor="la")


def write_visibility_map(ctx, path, cell_arcsec, mode):
    """The visibility map of the context's last frame over its own bounds, as an .npz (an empty 1 x 1 map for a frame of sky)."""
    if not (cell_arcsec > 0 and np.isfinite(cell_arcsec)):
        raise config.ConfigError("--map-cell must be a positive number of arcseconds")
    cell = cell_arcsec / 3600.0
    grid = generators.snap_grid(generators.frame_bounds(ctx, mode), cell) or generators.GeoGrid(0.0, 0.0, cell, cell, 1, 1)
    count, mind, stats = generators.visibility_map_device(ctx, grid, mode)
    count = count.cpu().numpy().view(np.uint32)
    with open(path, "wb") as f:  # a file object: numpy appends no extension to the name the user gave
        np.savez_compressed(f, count=count, min_distance=mind.cpu().numpy(), lat0=grid.lat0, lon0=grid.lon0, cell_lat=grid.cell_lat,
                            cell_lon=grid.cell_lon, **{k: np.uint64(v) for k, v in stats.items()})


def locate_landmarks(ctx, path, radius_arcsec, mode, out_path):
    """The landmarks of the CSV file located in the context's last frame; the table to out_path or stdout.  -> (names, records)."""
    if not (radius_arcsec > 0 and radius_arcsec <= 3600.0):
        raise config.ConfigError("--landmark-radius must be a positive number of arcseconds, at most 3600")
    names, lat, lon = generators.read_landmarks_csv(path)
    if not names:
        raise config.ConfigError(f"{path} holds no landmark")
    hits, _ = generators.locate_landmarks(ctx, generators.landmarks(lat, lon), radius_arcsec / 3600.0, mode)
    if out_path:
        with open(out_path, "w", newline="") as f:
            generators.write_landmarks_csv(f, names, lat, lon, hits)
    else:
        generators.write_landmarks_csv(sys.stdout, names, lat, lon, hits)
    return names, hits


def solve_sight_lines(ctx, cfg, path, fan, rounds, out_path):
    """The targets of the CSV file solved against the context's parameters, atmosphere and terrain; the table to out_path or stdout."""
    names, lat, lon, height = generators.read_sight_csv(path)
    if not names:
        raise config.ConfigError(f"{path} holds no target")
    try:
        targets = generators.sight_targets(ctx, lat, lon, height)
    except ValueError as exc:
        raise config.ConfigError(f"{path}: {exc}")
    sights = generators.sight_lines(ctx, targets, fan, rounds)
    if out_path:
        with open(out_path, "w", newline="") as f:
            generators.write_sight_csv(f, names, targets, sights, cfg.params)
    else:
        generators.write_sight_csv(sys.stdout, names, targets, sights, cfg.params)
    return targets, sights


def viewshed_defaults(cfg, az, reach, flag="--viewshed-az"):
    """(az_lo, az_step, n_az, reach) of gen --viewshed (and gen --horizon): what --viewshed-az LO HI N and --viewshed-reach say, else one
    azimuth per pixel column of the frame (the Fast generator's column directions) as far as max_distance."""
    p = cfg.params
    if az is None:
        lo, step, n = p.frame.direction - float(p.width // 2) / p.width * p.frame.fov, p.frame.fov / p.width, int(p.width)
    else:
        lo, hi, n = float(az[0]), float(az[1]), int(az[2])
        if n < 1 or float(az[2]) != n:
            raise config.ConfigError(f"{flag} LO HI N: N must be a positive whole number")
        step = (hi - lo) / (n - 1) if n > 1 else 0.0
    return lo, step, n, p.frame.max_distance if reach is None else float(reach)


def write_viewshed(ctx, cfg, path, az, reach, height, fan):
    """The viewshed of the context's parameters, atmosphere and terrain to an .npz; returns the Viewshed."""
    lo, step, n, reach = viewshed_defaults(cfg, az, reach)
    if float(fan[2]) != int(fan[2]):
        raise config.ConfigError("--viewshed-fan LO HI K: K must be a whole number")
    v = generators.viewshed(ctx, lo, step, n, reach, height, (float(fan[0]), float(fan[1])), int(fan[2]))
    generators.write_viewshed_npz(path, v)
    return v


def read_observers_csv(path):
    """FILE.csv of --viewshed-observers: a header naming lat, lon and altitude, one observer per row -> [{lat, lon, altitude}]."""
    import csv
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    try:
        return [dict(lat=float(r["lat"]), lon=float(r["lon"]), altitude=float(r["altitude"])) for r in rows]
    except (KeyError, TypeError, ValueError) as exc:
        raise config.ConfigError(f"{path}: every row needs the numbers lat, lon and altitude ({exc})")


def write_viewshed_map(ctx, cfg, gen, path, cell_arcsec, az, reach, height, fan, observers_path=None):
    """The viewshed map of the context's parameters, atmosphere and terrain to an .npz over the grid viewshed_map_grid lays around the
    observer (as far as the lattice's last sample); with observers_path the cumulative form over a grid that holds every observer's
    reach.  Returns what it wrote: a ViewshedMap, or (observers_seeing, min_hidden) as numpy arrays."""
    if not (cell_arcsec > 0 and np.isfinite(cell_arcsec)):
        raise config.ConfigError("--map-cell must be a positive number of arcseconds")
    lo, step, n, reach = viewshed_defaults(cfg, az, reach)
    if float(fan[2]) != int(fan[2]):
        raise config.ConfigError("--viewshed-fan LO HI K: K must be a whole number")
    fan, K, cell = (float(fan[0]), float(fan[1])), int(fan[2]), cell_arcsec / 3600.0
    far = float(generators.viewshed_lattice(cfg.params.simulation_step, reach)[-1])
    with open(path, "wb") as f:  # a file object: numpy appends no extension to the name the user gave
        if observers_path is None:
            pos = cfg.params.position
            grid = generators.viewshed_map_grid(pos.latitude, pos.longitude, far, cell)
            v = generators.viewshed_map(ctx, grid, lo, step, n, reach, height, fan, K)
            generators.write_viewshed_map_npz(f, grid, dict(n_samples=v.n_samples, n_seen=v.n_seen, min_hidden=v.min_hidden), v.stats)
            return v
        observers = read_observers_csv(observers_path)
        if not observers:
            raise config.ConfigError(f"{observers_path} holds no observer")
        grids = [generators.viewshed_map_grid(o["lat"], o["lon"], far, cell) for o in observers]
        bounds = (min(g.lat0 for g in grids), max(g.lat0 + g.n_lat * g.cell_lat for g in grids) - 0.5 * cell,
                  min(g.lon0 for g in grids), max(g.lon0 + g.n_lon * g.cell_lon for g in grids) - 0.5 * cell)
        grid = generators.snap_grid(bounds, cell)
        seeing, minh = generators.cumulative_viewshed(gen, observers, grid, lo, step, n, reach, height, fan, K)
        seeing, minh = seeing.cpu().numpy().view(np.uint32), minh.cpu().numpy()
        generators.write_viewshed_map_npz(f, grid, dict(observers_seeing=seeing, min_hidden=minh))
        return seeing, minh


def write_horizon(ctx, cfg, path, az, reach, fan, rounds):
    """The horizon of the context's parameters, atmosphere and terrain to a .csv; returns the Horizon."""
    lo, step, n, reach = viewshed_defaults(cfg, az, reach, "--horizon-az")
    if float(fan[2]) != int(fan[2]):
        raise config.ConfigError("--horizon-fan LO HI K: K must be a whole number")
    h = generators.horizon(ctx, lo, step, n, reach, (float(fan[0]), float(fan[1])), int(fan[2]), rounds)
    generators.write_horizon_csv(path, h)
    return h


def draw_landmarks(img, names, hits):
    """A short vertical marker above every found landmark's pixel and its name, drawn on the host like the tick labels."""
    from PIL import ImageDraw, ImageFont
    draw = ImageDraw.Draw(img)
    path = find_label_font()
    font = ImageFont.truetype(path, 13) if path else None
    for name, h in zip(names, hits):
        if not h["n_within"]:
            continue
        x, y = int(h["x"]), int(h["y"])
        draw.line([(x, y - 14), (x, y - 3)], fill=(255, 255, 255), width=1)
        if font is not None:
            draw.text((x + 3, y - 16), name, fill=(255, 255, 255), font=font, anchor="ls")


def shadow_spec_of(cfg, reach, lift, light):
    """The atmrt_shadow_spec_t of gen --shadows: --shadow-light AZ EL or the Shading configuration's light, --shadow-reach or
    max_distance capped at 65535 steps, --shadow-lift."""
    if light is not None:
        az, el = float(light[0]), float(light[1])
    elif cfg.coloring["kind"] == 1:
        az, el = generators.light_from_coloring(cfg.params, cfg.coloring["light_zenith_angle"], cfg.coloring["light_dir"])
    else:
        raise config.ConfigError("--shadows needs a light: the Shading colouring method's, or --shadow-light AZ EL")
    if not -90.0 < el < 90.0:
        raise config.ConfigError(f"--shadows: the light's elevation {el!r} must lie strictly between -90 and 90 degrees")
    step = cfg.params.simulation_step
    reach = min(float(reach) if reach is not None else cfg.params.frame.max_distance, 65535 * step)
    if not reach > 0.0 or lift < 0.0:
        raise config.ConfigError("--shadow-reach must be positive and --shadow-lift not negative")
    return generators.shadow_spec(az, el, reach, lift)


def shadow_reach_of(cfg, reach, lift):
    step = cfg.params.simulation_step
    reach = min(float(reach) if reach is not None else cfg.params.frame.max_distance, 65535 * step)
    if not reach > 0.0 or lift < 0.0:
        raise config.ConfigError("--shadow-reach must be positive and --shadow-lift not negative")
    return reach


def shadow_world_light(cfg, col, light):
    """The one light of gen --shadows --shadow-per-point as a world-frame vector [1][3]: --shadow-light AZ EL as seen from the
    observer, or the Shading configuration's own light_dir."""
    if light is not None:
        if not -90.0 <= float(light[1]) <= 90.0:
            raise config.ConfigError(f"--shadows: the light's elevation {light[1]!r} must lie between -90 and 90 degrees")
        return generators.lights_from_angles(cfg.params, [(float(light[0]), float(light[1]))])
    if cfg.coloring["kind"] != 1:
        raise config.ConfigError("--shadows needs a light: the Shading colouring method's, or --shadow-light AZ EL")
    return np.array([list(col.light_dir)], dtype=np.float64)


def read_lights_csv(path):
    """Rows of azimuth_deg,elevation_deg; blank lines, lines that start with # and one header line are skipped."""
    rows = []
    with open(path) as f:
        for n, line in enumerate(f, 1):
            text = line.strip()
            if not text or text.startswith("#"):
                continue
            cells = [c.strip() for c in text.split(",")]
            try:
                az, el = float(cells[0]), float(cells[1])
            except (ValueError, IndexError):
                if not rows and any(c.isalpha() for c in text):
                    continue  # the header
                raise config.ConfigError(f"{path}:{n}: expected azimuth_deg,elevation_deg, found {text!r}")
            rows.append((az, el))
    if not 1 <= len(rows) <= 64:
        raise config.ConfigError(f"{path}: {len(rows)} lights; a call takes 1 to 64")
    return rows


def write_shadow_lights(ctx, cfg, path, out, reach, lift, w, h, true_table=None):
    """gen --shadow-lights: the lit mask of the lights of `path` over the frame on the device, its popcount and the call's counts
    to an .npz; returns what was written.  true_table: the table spec of --shadow-true (the rows are TRUE directions), or None."""
    import torch
    rows = read_lights_csv(path)
    spec, dirs = generators.shadow_lights_spec(generators.lights_from_angles(cfg.params, rows, ctx.lib), shadow_reach_of(cfg, reach, lift), lift)
    mask_dev = torch.empty((h, w), dtype=torch.int64, device=torch.device("cuda", ctx.device))
    st = _abi.ShadowStats()
    if true_table is None:
        ctx.check(ctx.lib.atmrt_shadow_lights_device(ctx.handle, C.byref(spec), mask_dev.data_ptr(), None, None, C.byref(st)))
    else:
        ctx.check(ctx.lib.atmrt_shadow_lights_true_device(ctx.handle, C.byref(spec), C.byref(true_table), mask_dev.data_ptr(), None, None, C.byref(st)))
    mask = mask_dev.cpu().numpy().view(np.uint64)
    count = np.unpackbits(mask.view(np.uint8).reshape(h, w, 8), axis=2).sum(axis=2).astype(np.uint8)
    data = dict(lit_mask=mask, lit_count=count, dirs=dirs, azimuth_deg=np.array([r[0] for r in rows]), elevation_deg=np.array([r[1] for r in rows]))
    data.update({"stats_" + k: np.uint64(v) for k, v in generators._shadow_stats(st).items()})
    np.savez_compressed(out, **data)
    print(f"{len(rows)} lights: {st.lit} point-light pairs lit, {st.shadowed} in shadow, {st.none} pixels without a trace point")
    return data


def sky_spec_of(a):
    """The atmrt_sky_spec_t of gen's sky options: --sky-step (0: the simulation step), --sky-top, --sky-floor."""
    step = 0.0 if a.sky_step is None else a.sky_step
    if not (np.isfinite(step) and step >= 0.0 and np.isfinite(a.sky_top) and np.isfinite(a.sky_floor) and a.sky_floor < a.sky_top):
        raise config.ConfigError("--sky-step must not be negative and --sky-floor must lie below --sky-top")
    return generators.sky_spec(step, a.sky_top, a.sky_floor)


def sky_table_spec_of(a):
    """The atmrt_sky_table_spec_t of gen --shadow-true: --sky-table-alt LO HI N, --sky-table-el LO HI N and the sky options."""
    alt, el = a.sky_table_alt, a.sky_table_el
    for name, (lo, hi, n) in (("--sky-table-alt", alt), ("--sky-table-el", el)):
        if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi and float(n) == int(n) and int(n) >= 2):
            raise config.ConfigError(f"{name} needs finite LO < HI and at least two entries")
    if not (-90.0 < el[0] and el[1] < 90.0):
        raise config.ConfigError("--sky-table-el must lie strictly between -90 and 90 degrees")
    if int(alt[2]) > _abi.SKY_TABLE_ALT_MAX or int(el[2]) > _abi.SKY_TABLE_EL_MAX or int(alt[2]) * int(el[2]) > _abi.SKY_TABLE_ENTRIES_MAX:
        raise config.ConfigError("the sky table takes at most 1024 altitudes, 65536 elevations and 2^24 entries")
    return generators.sky_table_spec((alt[0], alt[1], int(alt[2])), (el[0], el[1], int(el[2])), sky=sky_spec_of(a))


def shadow_true_table_of(a):
    """None, or the table spec of --shadow-true, which needs a light given per point: --shadows --shadow-per-point or --shadow-lights."""
    if not a.shadow_true:
        return None
    if not ((a.shadows and a.shadow_per_point) or a.shadow_lights):
        raise config.ConfigError("--shadow-true needs a light per point: --shadows --shadow-per-point, or --shadow-lights FILE.csv")
    return sky_table_spec_of(a)


def sky_bodies_of(a):
    """The bodies of gen --sun / --moon, the sun first."""
    bodies = []
    if a.sun:
        bodies.append(generators.sky_body(a.sun[0], a.sun[1], a.sun_radius, (255, 244, 214)))
    if a.moon:
        bodies.append(generators.sky_body(a.moon[0], a.moon[1], generators.SUN_RADIUS_DEG, (226, 228, 235)))
    return bodies


def draw_sky(ctx, a, rgb_dev, w, h):
    """gen --sun / --moon / --sky-out: the sky march and the discs over the device image; the planes go to --sky-out."""
    import torch
    dev = rgb_dev.device
    true_dev = torch.empty((h, w), dtype=torch.float64, device=dev)
    status_dev = torch.empty((h, w), dtype=torch.uint8, device=dev)
    steps_dev = torch.empty((h, w), dtype=torch.int32, device=dev)
    body_dev = torch.empty((h, w), dtype=torch.uint8, device=dev)
    column_dev = torch.empty((h, w), dtype=torch.float64, device=dev) if a.sky_colour else None
    torch.cuda.synchronize(dev)
    spec, st = sky_spec_of(a), _abi.SkyStats()
    arr, n = generators._sky_bodies_array(sky_bodies_of(a))
    if a.sky_colour:  # "sky light": the march with the column, then the shade instead of the flat discs
        light, z0 = generators.sky_light_spec(a.air_mass_ref, sky=spec), C.c_double()
        ctx.check(ctx.lib.atmrt_sky_light_device(ctx.handle, C.byref(light), true_dev.data_ptr(), status_dev.data_ptr(), steps_dev.data_ptr(),
                                                 column_dev.data_ptr(), C.byref(st), C.byref(z0)))
        shade = generators.sky_shade_params(z0.value, a.sky_tau, a.sun_limb, a.sky_exposure)
        ctx.check(ctx.lib.atmrt_sky_shade_device(ctx.handle, C.byref(shade), arr, n, true_dev.data_ptr(), status_dev.data_ptr(), column_dev.data_ptr(),
                                                 body_dev.data_ptr(), rgb_dev.data_ptr()))
    else:
        ctx.check(ctx.lib.atmrt_sky_directions_device(ctx.handle, C.byref(spec), true_dev.data_ptr(), status_dev.data_ptr(), steps_dev.data_ptr(), C.byref(st)))
        ctx.check(ctx.lib.atmrt_sky_bodies_device(ctx.handle, arr, n, true_dev.data_ptr(), status_dev.data_ptr(), body_dev.data_ptr(), rgb_dev.data_ptr()))
    stats = generators._sky_stats(st)
    print(f"Sky: {stats['exit']} pixels leave the atmosphere, {stats['ground']} reach the floor, {stats['inside']} stay inside, {stats['lost']} lost; "
          f"{int((body_dev != 0).sum())} pixels of {n} bodies")
    if a.sky_colour:
        x = (column_dev / z0.value)[status_dev == _abi.SKY_EXIT]
        span = f"{float(x.min()):.3f} .. {float(x.max()):.3f}" if x.numel() else "of no pixel"
        print(f"Sky colour: zenith column {z0.value!r} m from {a.air_mass_ref!r} m, air mass {span}")
    if a.sky_out:
        data = dict(true_elevation=true_dev.cpu().numpy(), status=status_dev.cpu().numpy(), steps=steps_dev.cpu().numpy().view(np.uint32),
                    body=body_dev.cpu().numpy())
        if a.sky_colour:
            column = column_dev.cpu().numpy()
            data.update(column=column, air_mass=column / z0.value, zenith_column=np.float64(z0.value))
        data.update({"stats_" + k: np.uint64(v) for k, v in stats.items()})
        np.savez_compressed(a.sky_out, **data)


def write_refraction_table(ctx, cfg, a, terrain):
    """gen --refraction-table: the list call over the fan of --sky-fan from the observer's altitude."""
    lo, hi, k = a.sky_fan
    k = int(k)
    if not (k >= 1 and np.isfinite(lo) and np.isfinite(hi)):
        raise config.ConfigError("--sky-fan needs finite LO and HI and at least one ray")
    elev = np.array([lo]) if k == 1 else lo + (hi - lo) * np.arange(k) / (k - 1)
    pos = cfg.params.position
    h0 = pos.altitude
    if pos.altitude_kind == _abi.ALT_RELATIVE:  # Altitude::abs: above the terrain, 0 m where it has none
        ground, valid = terrain.get_elev(pos.latitude, pos.longitude)
        h0 = (float(ground[0]) if valid[0] else 0.0) + pos.altitude
    rec, _ = generators.sky_rays(ctx, h0, elev, spec=sky_spec_of(a))
    with open(a.refraction_table, "w") as f:
        f.write("elevation_deg,status,steps,true_elevation_deg,refraction_deg\n")
        for e, r in zip(elev, rec):
            leaves = int(r["status"]) == _abi.SKY_EXIT
            true = float(r["true_elevation"])
            f.write(f"{float(e)!r},{_abi.SKY_STATUS[int(r['status'])]},{int(r['steps'])},{repr(true) if leaves else ''},{repr(float(e) - true) if leaves else ''}\n")


def cmd_gen(a):
    start = time.time()
    cfg = config.parse_config(a.config)
    true_table = shadow_true_table_of(a)
    stamp = lambda msg: print(f"{time.time() - start:.3f}: {msg}", flush=True)
    stamp(f"Using terrain data directory: {os.path.join(os.getcwd(), cfg.terrain_folder)!r}")
    ctx, terrain = _ctx_with_terrain(cfg, a.config)
    print(f"Detected {terrain.n_files} terrain files")
    gen = generators.make_generator(generators.Params(cfg), terrain)
    stamp("Calculating pixels...")
    res = gen.generate()
    stamp("Done calculating")
    stamp("Outputting image...")
    col = generators.into_coloring(ctx.lib, cfg.params, cfg.coloring)
    import torch
    from PIL import Image
    w, h = res["width"], res["height"]
    rgb_dev = torch.empty((h, w, 3), dtype=torch.uint8, device=torch.device("cuda", ctx.device))
    if a.shadows:  # the second march, then the image through the status plane: both stay on the device
        stamp("Casting shadows...")
        status_dev = torch.empty((h, w), dtype=torch.uint8, device=rgb_dev.device)
        st = _abi.ShadowStats()
        if a.shadow_per_point:  # one light of the world: every point marches in its own local direction
            # --shadow-true: the angles are the light's TRUE direction; without --shadow-light the light is the sun of --sun
            light = shadow_world_light(cfg, col, a.shadow_light if a.shadow_light is not None or true_table is None else a.sun)
            lights, keep = generators.shadow_lights_spec(light, shadow_reach_of(cfg, a.shadow_reach, a.shadow_lift), a.shadow_lift)
            if true_table is None:
                ctx.check(ctx.lib.atmrt_shadow_lights_device(ctx.handle, C.byref(lights), None, status_dev.data_ptr(), None, C.byref(st)))
            else:
                ctx.check(ctx.lib.atmrt_shadow_lights_true_device(ctx.handle, C.byref(lights), C.byref(true_table), None, status_dev.data_ptr(), None,
                                                                  C.byref(st)))
            print(f"Light along {[float(v) for v in keep[0]]!r} of the world{' (true direction)' if true_table is not None else ''}: "
                  f"{st.lit} points lit, {st.shadowed} in shadow")
        else:
            spec = shadow_spec_of(cfg, a.shadow_reach, a.shadow_lift, a.shadow_light)
            ctx.check(ctx.lib.atmrt_shadow_mask_device(ctx.handle, C.byref(spec), status_dev.data_ptr(), None, C.byref(st)))
            print(f"Light at azimuth {spec.azimuth_deg!r}, elevation {spec.elevation_deg!r}: {st.lit} points lit, {st.shadowed} in shadow")
        ctx.check(ctx.lib.atmrt_draw_image_shadowed_device(ctx.handle, C.byref(col), status_dev.data_ptr(), rgb_dev.data_ptr()))
    else:
        ctx.check(ctx.lib.atmrt_draw_image_device(ctx.handle, C.byref(col), rgb_dev.data_ptr()))
    if a.sun or a.moon or a.sky_out or a.sky_colour:  # on the device image, before the overlay: ticks and lines stay on top
        stamp("Marching the sky...")
        draw_sky(ctx, a, rgb_dev, w, h)
    ticks, _ = generators.draw_overlay_device(ctx, generators.into_overlay(cfg.output), rgb_dev.data_ptr(), w, h)
    if a.refraction_table:  # needs no frame: the context's parameters and atmosphere
        stamp("Writing the refraction table...")
        write_refraction_table(ctx, cfg, a, terrain)
    if a.shadow_lights:  # on the device, while the frame is still in HBM
        stamp("Casting the shadows of the light list...")
        write_shadow_lights(ctx, cfg, a.shadow_lights, a.shadow_lights_out, a.shadow_reach, a.shadow_lift, w, h, true_table)
    if a.visibility_map:  # likewise
        stamp("Binning the visibility map...")
        write_visibility_map(ctx, a.visibility_map, a.map_cell, "all" if a.map_all else "first")
    located = None
    if a.landmarks:  # likewise
        stamp("Locating landmarks...")
        located = locate_landmarks(ctx, a.landmarks, a.landmark_radius, "all" if a.landmarks_all else "first", a.landmarks_out)
    if a.sight_lines:  # needs no frame: the context's parameters, atmosphere and terrain
        stamp("Solving sight lines...")
        solve_sight_lines(ctx, cfg, a.sight_lines, tuple(a.sight_fan), a.sight_rounds, a.sight_out)
    if a.viewshed:  # likewise
        stamp("Scanning the viewshed...")
        write_viewshed(ctx, cfg, a.viewshed, a.viewshed_az, a.viewshed_reach, a.viewshed_height, a.viewshed_fan)
    if a.horizon:  # likewise
        stamp("Solving the horizon...")
        write_horizon(ctx, cfg, a.horizon, a.horizon_az, a.horizon_reach, a.horizon_fan, a.horizon_rounds)
    if a.viewshed_map:  # likewise
        stamp("Binning the viewshed map...")
        write_viewshed_map(ctx, cfg, gen, a.viewshed_map, a.map_cell, a.viewshed_az, a.viewshed_reach, a.viewshed_height, a.viewshed_fan, a.viewshed_observers)
    img = Image.fromarray(rgb_dev.cpu().numpy(), "RGB")
    draw_labels(img, ticks)
    if located:
        draw_landmarks(img, *located)
    img.save(a.output)
    meta_path = a.metadata or cfg.output["file_metadata"]  # `if let Some(ref filename) = params.output.file_metadata`, generator/mod.rs:88-94
    if meta_path:
        stamp("Outputting metadata...")
        if meta_path.endswith(".npz"):  # this package's own array dump
            np.savez_compressed(meta_path, **{k: v for k, v in res.items() if isinstance(v, np.ndarray)})
        else:  # gzip(bincode(AllData)) in the reference's field order — but with a stand-in `env` segment (metadata.py): this package's
            # reader only; write_metadata warns on stderr every time
            from . import metadata
            metadata.write_metadata(meta_path, cfg, res, col, metadata.object_elevations(cfg, terrain))
    stamp("Done.")
    return 0


def cmd_output_atm(a):
    cfg = config.parse_config(a.config)
    ctx = generators.Context()
    _configure(ctx, cfg)
    assert a.step > 0
    alts, alt = [], a.min_alt
    while alt <= a.max_alt:  # atm_printer.rs:37-46
        alts.append(alt)
        alt += a.step
    s = generators.atmosphere_sample(ctx, alts)
    for h, t, p in zip(alts, s["temperature"], s["pressure"]):
        print(f"{h!r} {float(t - (273.15 if a.celsius else 0.0))!r} {float(p)!r} 0.0")  # dry air: humidity 0
    return 0


def cmd_output_ray_paths(a):
    cfg = config.parse_config(a.config)
    ctx = generators.Context()
    _configure(ctx, cfg)
    assert a.angle_step > 0, "step must be positive"  # ray_path.rs:53
    angs, ang = [], a.min_ang
    while ang <= a.max_ang:
        angs.append(ang)
        ang += a.angle_step
    n_steps = int(np.ceil(a.cutoff / a.ray_step)) + 1
    x, h = generators.ray_paths(ctx, a.height, angs, a.ray_step, n_steps, straight=False)
    # ray_path.rs:76-91: keep a sample whenever the step straddles a multiple of output_step; stop after x >= cutoff
    xs, keep = [0.0], [0]
    for k in range(1, n_steps + 1):
        xv = x[0, k]
        if np.floor((xv - a.ray_step / 2.0) / a.output_step) != np.floor((xv + a.ray_step / 2.0) / a.output_step):
            xs.append(float(xv))
            keep.append(k)
        if xv >= a.cutoff:
            break
    for xv, k in zip(xs, keep):
        print("\t".join([repr(xv)] + [repr(float(h[i, k])) for i in range(len(angs))]) + "\t")
    return 0


def cmd_output_elev_profile(a):
    cfg = config.parse_config(a.config)
    ctx, terrain = _ctx_with_terrain(cfg, a.config)
    _configure(ctx, cfg)
    assert a.step > 0, "step must be positive"  # elev_profile.rs:32
    xs, x = [], 0.0
    while x <= a.cutoff:  # elev_profile.rs:54-60
        xs.append(x)
        x += a.step
    lat, lon = generators.coords_at_dist(ctx, cfg.params.position.latitude, cfg.params.position.longitude, a.azim, xs)
    elev, valid = terrain.get_elev(lat, lon)
    for xv, e, ok in zip(xs, elev, valid):
        print(f"{xv!r}\t{float(e) if ok else 0.0!r}")
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(prog="atm_raytracer_amd", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    g = sub.add_parser("gen")
    g.add_argument("-c", "--config", required=True)
    g.add_argument("--output", default="./output.png")
    g.add_argument("--metadata", default=None)
    g.add_argument("--visibility-map", default=None, metavar="OUT.npz")
    g.add_argument("--map-cell", type=float, default=3.0, metavar="ARCSEC")
    g.add_argument("--map-all", action="store_true")
    g.add_argument("--landmarks", default=None, metavar="FILE.csv")
    g.add_argument("--landmark-radius", type=float, default=3.0, metavar="ARCSEC")
    g.add_argument("--landmarks-all", action="store_true")
    g.add_argument("--landmarks-out", default=None, metavar="OUT.csv")
    g.add_argument("--sight-lines", default=None, metavar="FILE.csv")
    g.add_argument("--sight-out", default=None, metavar="OUT.csv")
    g.add_argument("--sight-fan", type=float, nargs=2, default=(-5.0, 5.0), metavar=("LO", "HI"))
    g.add_argument("--sight-rounds", type=int, default=3, metavar="N")
    g.add_argument("--viewshed", default=None, metavar="OUT.npz")
    g.add_argument("--viewshed-az", type=float, nargs=3, default=None, metavar=("LO", "HI", "N"))
    g.add_argument("--viewshed-reach", type=float, default=None, metavar="M")
    g.add_argument("--viewshed-height", type=float, default=0.0, metavar="M")
    g.add_argument("--viewshed-fan", type=float, nargs=3, default=(-5.0, 5.0, 64), metavar=("LO", "HI", "K"))
    g.add_argument("--viewshed-map", default=None, metavar="OUT.npz")
    g.add_argument("--viewshed-observers", default=None, metavar="FILE.csv")
    g.add_argument("--shadows", action="store_true")
    g.add_argument("--shadow-reach", type=float, default=None, metavar="M")
    g.add_argument("--shadow-lift", type=float, default=0.0, metavar="M")
    g.add_argument("--shadow-light", type=float, nargs=2, default=None, metavar=("AZ", "EL"))
    g.add_argument("--shadow-per-point", action="store_true")
    g.add_argument("--shadow-lights", default=None, metavar="FILE.csv")
    g.add_argument("--shadow-lights-out", default="shadow_lights.npz", metavar="OUT.npz")
    g.add_argument("--shadow-true", action="store_true")
    g.add_argument("--sky-table-alt", type=float, nargs=3, default=generators.SKY_TABLE_ALT, metavar=("LO", "HI", "N"))
    g.add_argument("--sky-table-el", type=float, nargs=3, default=generators.SKY_TABLE_EL, metavar=("LO", "HI", "N"))
    g.add_argument("--sun", type=float, nargs=2, default=None, metavar=("AZ", "EL"))
    g.add_argument("--sun-radius", type=float, default=generators.SUN_RADIUS_DEG, metavar="DEG")
    g.add_argument("--moon", type=float, nargs=2, default=None, metavar=("AZ", "EL"))
    g.add_argument("--sky-top", type=float, default=generators.SKY_TOP, metavar="M")
    g.add_argument("--sky-step", type=float, default=None, metavar="M")
    g.add_argument("--sky-floor", type=float, default=0.0, metavar="M")
    g.add_argument("--sky-out", default=None, metavar="OUT.npz")
    g.add_argument("--sky-colour", action="store_true")
    g.add_argument("--sky-tau", type=float, nargs=3, default=generators.SKY_TAU, metavar=("R", "G", "B"))
    g.add_argument("--sky-exposure", type=float, default=generators.SKY_EXPOSURE, metavar="G")
    g.add_argument("--sun-limb", type=float, nargs=3, default=generators.SUN_LIMB, metavar=("R", "G", "B"))
    g.add_argument("--air-mass-ref", type=float, default=0.0, metavar="M")
    g.add_argument("--refraction-table", default=None, metavar="OUT.csv")
    g.add_argument("--sky-fan", type=float, nargs=3, default=(0.0, 60.0, 61), metavar=("LO", "HI", "K"))
    g.add_argument("--horizon", default=None, metavar="OUT.csv")
    g.add_argument("--horizon-az", type=float, nargs=3, default=None, metavar=("LO", "HI", "N"))
    g.add_argument("--horizon-reach", type=float, default=None, metavar="M")
    g.add_argument("--horizon-fan", type=float, nargs=3, default=(-5.0, 5.0, 64), metavar=("LO", "HI", "K"))
    g.add_argument("--horizon-rounds", type=int, default=3, metavar="N")
    g.set_defaults(fn=cmd_gen)
    p = sub.add_parser("output-atm")
    p.add_argument("config")
    p.add_argument("-a", "--min-alt", type=float, default=0.0)
    p.add_argument("-b", "--max-alt", type=float, default=1000.0)
    p.add_argument("-s", "--step", type=float, default=0.2)
    p.add_argument("-c", "--celsius", action="store_true")
    p.set_defaults(fn=cmd_output_atm)
    r = sub.add_parser("output-ray-paths", add_help=False)
    r.add_argument("config")
    r.add_argument("-h", "--height", type=float, default=2.0)
    r.add_argument("-a", "--min-ang", type=float, default=-1.0)
    r.add_argument("-b", "--max-ang", type=float, default=1.0)
    r.add_argument("-s", "--angle-step", type=float, default=0.1)
    r.add_argument("-r", "--ray-step", type=float, default=50.0)
    r.add_argument("-c", "--cutoff", "--cutoff-dist", type=float, default=10000.0)
    r.add_argument("-o", "--output-step", type=float, default=50.0)
    r.set_defaults(fn=cmd_output_ray_paths)
    e = sub.add_parser("output-elev-profile")
    e.add_argument("config")
    e.add_argument("-a", "--azim", type=float, default=0.0)
    e.add_argument("-s", "--step", type=float, default=50.0)
    e.add_argument("-c", "--cutoff", "--cutoff-dist", type=float, default=10000.0)
    e.set_defaults(fn=cmd_output_elev_profile)
    a = ap.parse_args(argv)
    try:
        return a.fn(a)
    except (generators.AtmrtError, config.ConfigError, OSError) as exc:
        print(f"ERROR: {exc}", file=sys.stderr)  # main.rs:36-38
        return 1


if __name__ == "__main__":
    sys.exit(main())
