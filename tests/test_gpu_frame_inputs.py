"""What a context keeps across frames (csrc/atmrt_ctx.h: the distance table, the step trig table, the compiled atmosphere and its
certificates, the ceiling bins and table, the textures) follows the frame's inputs: one long-lived context renders a sequence of
frames that changes one input at a time and returns to earlier values, and every frame is the same bits as that frame from a
context created for it alone: every pixel plane, the packed hits, n_hits, ray_steps, and the march's work counters (integrated
steps, escaped rays, terrain lookups), which show that the same tables and floors were in force and not merely the same image.
The ceiling table's build time is positive exactly in the frames that must build it."""
import ctypes as C

import pytest

W, H, FOV, STEP, MAX_DISTANCE = 96, 48, 12.0, 100.0, 30_000.0  # 80 ceiling bins of 0.15 degrees, 300 steps


def _inversion():
    """US-76's troposphere with a layer of +0.12 K/m at 2500 .. 2900 m, above the mosaic: the certificate refuses it"""
    return {"pressure": {"altitude": 0.0, "pressure": 101325.0},
            "first_temperature_function": {"Linear": {"gradient": -0.0065}},
            "next_functions": [{"altitude": 2500.0, "function": {"Linear": {"gradient": 0.12}}},
                               {"altitude": 2900.0, "function": {"Linear": {"gradient": -0.0065}}}],
            "temperature_fixed_point": {"altitude": 0.0, "temperature": 288.15}}


def _measure(ctx, gen):
    from util import frame_stats
    got = gen.generate()
    integrated, escaped = C.c_uint64(), C.c_uint64()
    ctx.check(ctx.lib.atmrt_last_march_work(ctx.handle, C.byref(integrated), C.byref(escaped)))
    work = (int(integrated.value), int(escaped.value), int(frame_stats(ctx)["terrain_lookups"]))
    return got, work, gen.last_timings()["ceiling_ms"]


@pytest.mark.gpu
def test_one_context_follows_every_input_of_the_frame():
    from atm_raytracer_amd import _abi, config, generators, synth
    from escape_cases import certificate
    from util import assert_bitexact, nested_cylinders
    cfg, tiles = synth.scene("S2", W, H, generator="Rectilinear", fov=FOV, tilt=1.0, max_distance=MAX_DISTANCE)
    assert cfg.params.simulation_step == STEP
    p = cfg.params
    base_atm, inversion = cfg.atmosphere, config._atmosphere(_inversion())
    rect, fast = _abi.GENERATORS["Rectilinear"], _abi.GENERATORS["Fast"]
    fresh = {}  # the reference is computed once per distinct frame: keyed by the bytes of everything the frame is made from

    def reference():
        atm = cfg.atmosphere
        functions = b"".join(bytes(atm.functions[j]) for j in range(atm.n_functions))  # no Spline here: no borrowed points
        label = (bytes(p), bytes(atm), functions, tuple(bytes(o) for o in cfg.objects))
        if label not in fresh:
            ctx = generators.Context(0)
            try:
                fresh[label] = _measure(ctx, generators.make_generator(generators.Params(cfg), generators.Terrain.from_tiles(tiles, ctx)))[:2]
            finally:
                ctx.close()
        return fresh[label]

    ctx = generators.Context(0)
    try:
        terrain = generators.Terrain.from_tiles(tiles, ctx)

        def frame(label, builds_ceiling):
            got, work, ceiling_ms = _measure(ctx, generators.make_generator(generators.Params(cfg), terrain))
            want, want_work = reference()
            assert_bitexact(got, want)
            assert work == want_work, (label, work, want_work)
            assert (ceiling_ms > 0.0) == builds_ceiling, (label, ceiling_ms)
            return got, work

        # 1, 2: the base frame, twice; the scene is worth the test only if both work counts are non-zero, rays hit and rays escape
        got, work = frame("base", True)
        assert work[0] > 0 and work[2] > 0 and work[1] > 0 and got["n_hits"] > 0, (work, got["n_hits"])
        assert (got["hit_count"] == 0).any() and (got["hit_count"] > 0).any()
        frame("base", False)
        # 3: the step
        p.simulation_step = 150.0
        frame("step 150", True)
        p.simulation_step = STEP
        frame("base", True)
        # 4: the distance
        p.frame.max_distance = 20_000.0
        frame("20 km", True)
        p.frame.max_distance = MAX_DISTANCE
        frame("base", True)
        # 5: the wavelength: a new atmosphere table, the same ceiling table
        wavelength = p.wavelength
        p.wavelength = 1.2 * wavelength
        frame("wavelength", False)
        p.wavelength = wavelength
        frame("base", False)
        # 6: an atmosphere whose escape certificate begins elsewhere
        top = float(max(int(t.max()) for t in tiles.values())) + 1.0
        lib = ctx.lib
        from_base = certificate(lib, base_atm, p.earth.radius, p.wavelength, top, STEP)[1]
        from_inversion = certificate(lib, inversion, p.earth.radius, p.wavelength, top, STEP)[1]
        assert from_inversion != from_base and from_inversion >= 2900.0 > from_base, (from_base, from_inversion)
        cfg.atmosphere = inversion
        frame("inversion", False)
        cfg.atmosphere = base_atm
        frame("base", False)
        # 7: the earth's radius: the trig table and the ceiling table
        radius = p.earth.radius
        p.earth.radius = 6_000_000.0
        frame("radius", True)
        p.earth.radius = radius
        frame("base", True)
        # 8: the observer
        latitude = p.position.latitude
        p.position.latitude = latitude + 0.2
        frame("latitude", True)
        p.position.latitude = latitude
        frame("base", True)
        # 9: the view
        p.frame.fov, p.frame.direction = 30.0, 135.0
        frame("view", True)
        p.frame.fov, p.frame.direction = FOV, 0.0
        frame("base", True)
        # 10: a Fast frame has no ceiling table and leaves the Rectilinear frame's alone
        p.generator = fast
        frame("fast", False)
        p.generator = rect
        frame("base", False)
        # 11: translucent terrain and a handful of objects
        p.terrain_alpha = 0.5
        nested_cylinders(cfg, 4)
        got, _ = frame("objects", False)
        assert got["hit_count"].max() > 1
        p.terrain_alpha = 1.0
        cfg.objects = []
        frame("base", False)
        # 12: sight lines prepare a frame of their own on the same context
        sights = generators.sight_lines(ctx, [(0.0, 5_000.0, 10.0), (2.0, 12_000.0, 50.0)])
        assert len(sights) == 2
        frame("base", False)
        # 13: so does the terrain lookup
        elev, valid = terrain.get_elev([46.5, 46.6], [8.5, 8.4])
        assert valid.all() and (elev > 0.0).all()
        frame("base", False)
    finally:
        ctx.close()
