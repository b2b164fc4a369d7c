#!/usr/bin/env python3
"""Render a panorama PNG on the GPU: generator (C ABI) -> renderer::draw_image on the device -> PNG via Pillow.
Usage: python examples/render_png.py OUT.png [--scene S3] [--width 1024] [--height 512] [--generator Fast] [--objects N]
       [--shadows [--sun-elevation DEG] [--shadow-reach M] [--shadow-per-point]] [--sun AZ EL [--shadows --shadow-true]] [--sky-colour]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from atm_raytracer_amd import config, generators, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--scene", default="S3")
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--generator", default="Fast")
    ap.add_argument("--objects", type=int, default=0)
    ap.add_argument("--terrain-alpha", type=float, default=1.0)
    ap.add_argument("--coloring", default="Shading", choices=["Shading", "Simple"])
    ap.add_argument("--fog", type=float, default=None)
    ap.add_argument("--shadows", action="store_true", help="cast shadows from the Shading light (include/atmrt.h, cast shadows)")
    ap.add_argument("--sun-elevation", type=float, default=35.0, help="degrees above the horizon: light_zenith_angle = 90 - this")
    ap.add_argument("--shadow-reach", type=float, default=50_000.0)
    ap.add_argument("--shadow-per-point", action="store_true",
                    help="the light is the Shading method's own world-frame vector: every point marches in its own local direction (shadow lights)")
    ap.add_argument("--sun", type=float, nargs=2, default=None, metavar=("AZ", "EL"),
                    help="draw the sun's disc at this TRUE direction [deg] where the refracted sky rays meet it (include/atmrt.h, sky rays)")
    ap.add_argument("--shadow-true", action="store_true",
                    help="with --sun AZ EL --shadows: the shadows' light is the sun at its TRUE direction, launched where it appears from "
                         "every point (include/atmrt.h, apparent elevation)")
    ap.add_argument("--sky-colour", action="store_true",
                    help="shade the sky by air mass and redden and limb-darken the sun of --sun AZ EL (include/atmrt.h, sky light)")
    a = ap.parse_args()
    if a.shadow_true and not (a.sun and a.shadows):
        ap.error("--shadow-true lights the terrain from the sun of --sun AZ EL: use --sun AZ EL --shadows --shadow-true")
    from PIL import Image
    cfg, tiles = synth.scene(a.scene, a.width, a.height, generator=a.generator, step=100.0, terrain_alpha=a.terrain_alpha)
    view = {"coloring": {a.coloring: {"water_level": 300.0} if a.coloring == "Simple" else {"water_level": 300.0, "light_dir": 40.0, "light_zenith_angle": 90.0 - a.sun_elevation}}}
    if a.fog:
        view["fog_distance"] = a.fog
    cfg.coloring = config._coloring(view)
    if a.objects:
        synth.add_objects(cfg, n_cyl=a.objects * 7 // 10, n_bill=a.objects - a.objects * 7 // 10, dist=(2_000.0, 60_000.0),
                          radius=(40.0, 200.0), height=(200.0, 900.0), bill_w=(200.0, 800.0), bill_h=(200.0, 800.0))
    ctx = generators.Context(0)
    terrain = generators.Terrain.from_tiles(tiles, ctx)
    gen = generators.make_generator(generators.Params(cfg), terrain)
    res = gen.generate()
    shadows = None
    if a.shadows:
        if a.coloring != "Shading":
            ap.error("--shadows darkens the Shading method's image: use --coloring Shading")
        az, el = generators.light_from_coloring(cfg.params, cfg.coloring["light_zenith_angle"], cfg.coloring["light_dir"])
        if a.shadow_true:  # the drawn sun lights the terrain: its true direction, a sky step of 1000 m as for the disc below
            az, el = a.sun
            table = generators.sky_table_spec(step=1000.0)
            mask = generators.shadow_lights(ctx, generators.lights_from_angles(cfg.params, [(az, el)], ctx.lib), a.shadow_reach, status=True,
                                            width=a.width, height=a.height, mask=False, true_table=table)
            mask.status = mask.status[0]
            print(f"refraction table: {generators.sky_table_work(ctx)}")
        elif a.shadow_per_point:  # slopes and shadows share one light: the coloring's light_dir vector
            light = list(generators.into_coloring(ctx.lib, cfg.params, cfg.coloring).light_dir)
            mask = generators.shadow_lights(ctx, [light], a.shadow_reach, status=True, width=a.width, height=a.height, mask=False)
            mask.status = mask.status[0]
        else:
            mask = generators.shadow_mask(ctx, (az, el, a.shadow_reach, 0.0), a.width, a.height, block=False)
        shadows = mask.status
        print(f"light at azimuth {az:g}, elevation {el:g}: {mask.stats['lit']} points lit, {mask.stats['shadowed']} in shadow, "
              f"{generators.shadow_timings(ctx)['march_ms']:.2f} ms of shadow march")
    bodies = None
    if a.sun:  # the sky march at 1000 m a step: within 5e-5 degrees of the frame's own step at a tenth of the work
        bodies = [generators.sky_body(a.sun[0], a.sun[1])]
    if a.sky_colour:  # the same march with the refractivity column carried along, then the shade instead of the flat disc
        sky = generators.sky_light(ctx, a.width, a.height, steps=False, step=1000.0)
        print(f"zenith column {sky.zenith_column:.6f} m, air mass {sky.air_mass[sky.status == 1].min():.2f} .. {sky.air_mass[sky.status == 1].max():.2f}"
              if (sky.status == 1).any() else "no sky pixel leaves the atmosphere")
    else:
        sky = generators.sky_directions(ctx, a.width, a.height, steps=False, step=1000.0) if bodies else None
    rgb = generators.draw_image(ctx, generators.into_coloring(ctx.lib, cfg.params, cfg.coloring), a.width, a.height, shadows=shadows, bodies=bodies,
                                sky=sky, sky_light=sky if a.sky_colour else None)
    if bodies:
        print(f"sun at true azimuth {a.sun[0]:g}, elevation {a.sun[1]:g}: {generators.sky_timings(ctx)['march_ms']:.2f} ms of sky march")
    Image.fromarray(rgb, "RGB").save(a.out)
    print(f"{a.out}: {a.width}x{a.height}, {res['n_hits']} trace points, {res['ray_steps']} ray-steps, {res['device_ms']:.2f} ms on device")


if __name__ == "__main__":
    main()
