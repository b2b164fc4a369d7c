"""Host-side mirror of the reference's generator interface above the C ABI.

Reference                                   here
------------------------------------------  -----------------------------------------------
Terrain::from_folder / get_elev             Terrain.from_folder / Terrain.get_elev
  (src/terrain/mod.rs:66-83,120-126)
Config::into_params(&terrain) -> Params     Params(config)
trait Generator { fn generate(&self) }      Generator.generate() -> ResultPixels
  FastGenerator::new(&params,&terrain,..)     FastGenerator(params, terrain)
  RectilinearGenerator::new(..)               RectilinearGenerator(params, terrain)
  InterpolatingRectilinearGenerator::new(..)  InterpolatingRectilinearGenerator(params, terrain)
generator::generate's match on GeneratorDef  make_generator(params, terrain)
  (src/generator/mod.rs:72-78)
"""
import ctypes as C
import os

import numpy as np

from . import _abi, _lib
from ._lib import AtmrtError
from .config import Config


class Context:
    """Owns one atmrt_ctx: one HIP device, or — Context.multi([...]) — several devices of this process behind one handle
    (the library cuts every frame into pixel-column tiles, one per device; include/atmrt.h "several GPUs of one node")."""

    def __init__(self, device=None, devices=None):
        self.lib = _lib.load()
        h = C.c_void_p()
        if devices is not None:
            devices = [int(d) for d in devices]
            arr = (C.c_int32 * len(devices))(*devices)
            rc = self.lib.atmrt_ctx_create_multi(C.byref(h), arr, len(devices))
            device = devices[0] if devices else 0
        else:
            if device is None:
                device = int(os.environ.get("LOCAL_RANK", "0"))
            rc = self.lib.atmrt_ctx_create(C.byref(h), device)
        if rc != 0:
            raise AtmrtError(rc, self.lib.atmrt_last_error(None).decode())
        self.handle = h
        self.device = device
        self.devices = devices or [device]
        self._transport = None

    @classmethod
    def multi(cls, devices):
        return cls(devices=devices)

    # ---- one process per GPU: this context becomes rank `rank` of `world` ranks that share every frame -------------------
    def comm_unique_id(self):
        """ncclGetUniqueId through the library: 128 bytes for the other ranks' comm_init_rank."""
        buf = (C.c_uint8 * _abi.COMM_ID_BYTES)()
        rc = self.lib.atmrt_comm_unique_id(buf)
        if rc != 0:
            raise AtmrtError(rc, self.lib.atmrt_last_error(None).decode())
        return bytes(buf)

    def comm_init_rank(self, unique_id, rank, world):
        buf = (C.c_uint8 * _abi.COMM_ID_BYTES).from_buffer_copy(unique_id)
        self.check(self.lib.atmrt_ctx_comm_init_rank(self.handle, buf, rank, world))

    def comm_init_external(self, rank, world, all_gather):
        """all_gather(send: memoryview, recv: memoryview) moves host bytes between the ranks (MPI, gloo, a test double)."""
        def thunk(_user, send, recv, nbytes):
            try:
                all_gather((C.c_uint8 * nbytes).from_address(send), (C.c_uint8 * (nbytes * world)).from_address(recv))
                return 0
            except Exception as exc:  # an exception must not unwind through the C frames
                import traceback
                traceback.print_exc()
                self._transport_error = exc
                return 1
        self._transport = _abi.ALL_GATHER_FN(thunk)  # keep the trampoline alive as long as the context
        self.check(self.lib.atmrt_ctx_comm_init_external(self.handle, rank, world, self._transport, None))

    def comm_init_external_device(self, rank, world, all_gather):
        """all_gather(send_ptr, recv_ptr, nbytes) moves DEVICE memory (e.g. through the torch.distributed communicator the host
        already owns: torch_device_all_gather below) and returns when the gathered bytes are in place."""
        def thunk(_user, send, recv, nbytes):
            try:
                all_gather(send, recv, nbytes)
                return 0
            except Exception as exc:
                import traceback
                traceback.print_exc()
                self._transport_error = exc
                return 1
        self._transport = _abi.ALL_GATHER_FN(thunk)
        self.check(self.lib.atmrt_ctx_comm_init_external_device(self.handle, rank, world, self._transport, None))

    def comm_timings(self):
        t = _abi.CommTimings()
        self.check(self.lib.atmrt_last_comm_timings(self.handle, C.byref(t)))
        out = {k: getattr(t, k) for k, _ in _abi.CommTimings._fields_ if k != "_pad"}
        out["route"] = _abi.ROUTES.get(out["route"], out["route"])
        return out

    def tile_columns(self, index=-1):
        """[c0, c1) of a tile (atmrt_ctx_tile_columns): of the last exchanged frame, else of the next one."""
        c0, c1 = C.c_int32(), C.c_int32()
        self.check(self.lib.atmrt_ctx_tile_columns(self.handle, index, C.byref(c0), C.byref(c1)))
        return c0.value, c1.value

    def set_tiling(self, cols):
        """Test hook (atmrt_debug_set_tiling): the next frames use exactly these world + 1 column boundaries; None: the library's own."""
        if cols is None:
            self.check(self.lib.atmrt_debug_set_tiling(self.handle, None, 0))
        else:
            arr = (C.c_int32 * len(cols))(*[int(v) for v in cols])
            self.check(self.lib.atmrt_debug_set_tiling(self.handle, arr, len(cols)))

    def debug_ceiling_table(self):
        """Diagnostic (atmrt_debug_ceiling_table): the terrain ceiling table the last generated frame marched with, as
        {'rows', 'n_bins', 'layout': (dir0, rel_lo, w), 'cell', 'suffix'}, the planes float32 [rows][n_bins + 1]; rows == 0 and
        empty planes when that frame had no table."""
        rows, bins, lay = C.c_int32(), C.c_int32(), (C.c_double * 3)()
        self.check(self.lib.atmrt_debug_ceiling_table(self.handle, 0, None, None, C.byref(rows), C.byref(bins), lay))
        n = rows.value * (bins.value + 1) if rows.value else 0
        cell, suffix = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
        if n:
            self.check(self.lib.atmrt_debug_ceiling_table(self.handle, n, cell.ctypes.data, suffix.ctypes.data, C.byref(rows), C.byref(bins), lay))
            assert rows.value * (bins.value + 1) == n
        shape = (rows.value, bins.value + 1) if n else (0, 0)
        return dict(rows=rows.value, n_bins=bins.value, layout=tuple(lay), cell=cell.reshape(shape), suffix=suffix.reshape(shape))

    def debug_march_order(self):
        """Diagnostic (atmrt_debug_march_order): the work queue the last generated frame's whole-frame march took its 64-pixel
        groups from, uint32 [n_groups], longest estimated march first; empty when that frame marched without one."""
        n = C.c_uint32()
        self.check(self.lib.atmrt_debug_march_order(self.handle, 0, None, C.byref(n)))
        order = np.zeros(n.value, dtype=np.uint32)
        if n.value:
            self.check(self.lib.atmrt_debug_march_order(self.handle, n.value, order.ctypes.data, C.byref(n)))
            assert n.value == order.size
        return order

    def debug_march_order_steps(self):
        """Diagnostic (atmrt_debug_march_order_steps): the estimated steps of every entry of debug_march_order(), uint32 [n_groups],
        non-increasing; empty when the last generated frame marched without a queue."""
        n = C.c_uint32()
        self.check(self.lib.atmrt_debug_march_order_steps(self.handle, 0, None, C.byref(n)))
        steps = np.zeros(n.value, dtype=np.uint32)
        if n.value:
            self.check(self.lib.atmrt_debug_march_order_steps(self.handle, n.value, steps.ctypes.data, C.byref(n)))
            assert n.value == steps.size
        return steps

    def debug_march_route(self, index=-1):
        """Diagnostic (atmrt_debug_last_march_route): 1 plain grid, 2 small-launch grid, 3 time-sliced, 4 work queue; 0 not Rectilinear."""
        route = C.c_int32()
        self.check(self.lib.atmrt_debug_last_march_route(self.handle, index, C.byref(route)))
        return route.value

    def debug_normal_trig(self):
        """Diagnostic (atmrt_debug_normal_trig): the record of the trace-point epilogue's frame constants for the parameters now
        set, float64 [17]: sin, cos of +15 m / radius, of -15 m / radius, of 0 and of 90 degrees, then the observer's north, east
        and up vectors; empty when there is none (another calculator than the Spherical one, ATMRT_NORMAL_TRIG=off)."""
        n = C.c_size_t()
        self.check(self.lib.atmrt_debug_normal_trig(self.handle, 0, None, C.byref(n)))
        out = np.zeros(n.value)
        if n.value:
            self.check(self.lib.atmrt_debug_normal_trig(self.handle, n.value, out.ctypes.data, C.byref(n)))
            assert n.value == out.size
        return out

    def debug_interp_blend(self, elev, dir, min_elev_step, min_dir_step, simulation_step, lattice):
        """Diagnostic (atmrt_debug_interp_blend): the last stage of an InterpolatingRectilinear frame — lattice keys, the 4-corner
        blend, the step count — on the caller's rays (elev, dir: float64 [h][w], radians) and lattice (the dict _abi.interp_lattice
        takes), run by the code the frame runs.  Returns what generate() returns: a ResultPixels."""
        elev, dir = np.ascontiguousarray(elev, dtype=np.float64), np.ascontiguousarray(dir, dtype=np.float64)
        assert elev.ndim == 2 and elev.shape == dir.shape
        lat, keep = _abi.interp_lattice(lattice)
        res = _abi.Result()
        self.check(self.lib.atmrt_debug_interp_blend(self.handle, elev.shape[1], elev.shape[0], elev.ctypes.data, dir.ctypes.data, min_elev_step,
                                                     min_dir_step, simulation_step, C.byref(lat), C.byref(res)))
        del keep
        try:
            return ResultPixels(_abi.result_to_numpy(res))
        finally:
            self.lib.atmrt_result_free(C.byref(res))

    def fail_next_collective(self, index=0, nth=1):
        """Test hook (atmrt_debug_fail_next_collective)."""
        self.check(self.lib.atmrt_debug_fail_next_collective(self.handle, index, nth))

    def sky_rays(self, h0, elevation_deg, **spec):
        """generators.sky_rays on this context."""
        return sky_rays(self, h0, elevation_deg, **spec)

    def sky_directions(self, **spec):
        """generators.sky_directions over this context's last frame."""
        return sky_directions(self, **spec)

    def sky_bodies(self, sky, bodies, rgb=None):
        """generators.sky_bodies over this context's last frame."""
        return sky_bodies(self, sky, bodies, rgb)

    def sky_timings(self):
        return sky_timings(self)

    def sky_light(self, **spec):
        """generators.sky_light over this context's last frame."""
        return sky_light(self, **spec)

    def sky_light_rays(self, h0, elevation_deg, **spec):
        """generators.sky_light_rays on this context."""
        return sky_light_rays(self, h0, elevation_deg, **spec)

    def sky_shade(self, light, bodies, rgb, **shade):
        """generators.sky_shade over this context's last frame."""
        return sky_shade(self, light, bodies, rgb, **shade)

    def sky_table(self, spec=None, **kw):
        """generators.sky_table on this context."""
        return sky_table(self, spec, **kw)

    def sky_apparent(self, h, t, spec=None):
        """generators.sky_apparent on this context."""
        return sky_apparent(self, h, t, spec)

    def sky_table_work(self):
        """generators.sky_table_work of this context's last call that needed the table."""
        return sky_table_work(self)

    def sky_table_spec(self, *args, **kw):
        """generators.sky_table_spec (needs no context: here for the calls above)."""
        return sky_table_spec(*args, **kw)

    def sky_tail_host(self, spec, true_elevation, status):
        """generators.sky_tail_host through this context's library (host code, no device)."""
        return sky_tail_host(spec, true_elevation, status, self.lib)

    def sky_apparent_host(self, spec, true_elevation, tail, h, t):
        """generators.sky_apparent_host through this context's library (host code, no device)."""
        return sky_apparent_host(spec, true_elevation, tail, h, t, self.lib)

    def shadow_lights(self, dirs, reach, lift=0.0, **kw):
        """generators.shadow_lights over this context's last frame (true_table=spec: the lights are true directions)."""
        return shadow_lights(self, dirs, reach, lift, **kw)

    def check(self, rc):
        if rc != 0:
            raise AtmrtError(rc, self.lib.atmrt_last_error(self.handle).decode())

    def close(self):
        if getattr(self, "handle", None):
            self.lib.atmrt_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _DeviceBytes:
    """A raw device pointer as a __cuda_array_interface__ object, so that torch can wrap it without a copy."""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (int(ptr), False), "version": 2}


def torch_device_all_gather(dist, device):
    """An all_gather for Context.comm_init_external_device over torch.distributed's own communicator (RCCL on device tensors)."""
    import torch

    def all_gather(send, recv, nbytes):
        world = dist.get_world_size()
        s = torch.as_tensor(_DeviceBytes(send, nbytes), device=device)
        r = torch.as_tensor(_DeviceBytes(recv, nbytes * world), device=device)
        dist.all_gather_into_tensor(r, s)
        torch.cuda.synchronize(device)
    return all_gather


class Terrain:
    """Terrain (src/terrain/mod.rs:55-57): tiles keyed by integer (lat, lon), resident in HBM."""

    def __init__(self, ctx=None):
        self.ctx = ctx or Context()
        self.n_files = 0

    @classmethod
    def from_folder(cls, path, ctx=None):
        t = cls(ctx)
        n = C.c_int32()
        t.ctx.check(t.ctx.lib.atmrt_terrain_load_dir(t.ctx.handle, os.fsencode(path), C.byref(n)))
        t.n_files = n.value
        return t

    @classmethod
    def from_tiles(cls, tiles, ctx=None):
        """tiles: {(lat0, lon0): int16 array [n_lat][n_lon], south->north, west->east}."""
        t = cls(ctx)
        for (lat0, lon0), posts in tiles.items():
            t.add_tile(lat0, lon0, posts)
        return t

    def add_tile(self, lat0, lon0, posts):
        posts = np.ascontiguousarray(posts, dtype=np.int16)
        self.ctx.check(self.ctx.lib.atmrt_terrain_add_tile(self.ctx.handle, lat0, lon0, posts.shape[0], posts.shape[1],
                                                          posts.ctypes.data))
        self.n_files += 1

    def get_elev(self, lat, lon):
        """Batched Terrain::get_elev; returns (elev, valid) arrays; valid=False where the reference returns None."""
        lat = np.ascontiguousarray(np.atleast_1d(lat), dtype=np.float64)
        lon = np.ascontiguousarray(np.atleast_1d(lon), dtype=np.float64)
        elev = np.zeros_like(lat)
        valid = np.zeros(lat.shape, dtype=np.uint8)
        self.ctx.check(self.ctx.lib.atmrt_terrain_get_elev(self.ctx.handle, lat.size, lat.ctypes.data, lon.ctypes.data,
                                                          elev.ctypes.data, valid.ctypes.data))
        return elev, valid.astype(bool)


class Params:
    """`Params` (params.rs:496-505): Config resolved against a Terrain."""

    def __init__(self, config: Config):
        self.config = config
        self.pod = config.params
        self.atmosphere = config.atmosphere
        self.objects = config.objects


class ResultPixels(dict):
    """Vec<Vec<ResultPixel>> as structure-of-arrays (see _abi.result_to_numpy).  `pixel(y, x)` rebuilds one
    ResultPixel {elevation_angle, azimuth, trace_points[]} (generators/mod.rs:13-30)."""

    def pixel(self, y, x):
        off, cnt = int(self["hit_offset"][y, x]), int(self["hit_count"][y, x])
        tps = []
        for k in range(off, off + cnt):
            tps.append({"lat": self["lat"][k], "lon": self["lon"][k], "distance": self["distance"][k],
                        "elevation": self["elevation"][k], "path_length": self["path_length"][k],
                        "normal": self["normal"][k], "color_tag": int(self["color_tag"][k]), "rgba": self["rgba"][k]})
        return {"elevation_angle": self["elevation_angle"][y, x], "azimuth": self["azimuth"][y, x], "trace_points": tps}


class Generator:
    """trait Generator (generators/mod.rs:82-84)."""

    KIND = None

    def __init__(self, params: Params, terrain: Terrain):
        self.params = params
        self.terrain = terrain
        self.ctx = terrain.ctx

    def _configure(self):
        pod = _abi.Params.from_buffer_copy(self.params.pod)
        if self.KIND is not None:
            pod.generator = self.KIND
        self.ctx.check(self.ctx.lib.atmrt_set_params(self.ctx.handle, C.byref(pod)))
        self.ctx.last_params = pod  # what sight_targets reads the observer and the earth model from
        self.ctx.check(self.ctx.lib.atmrt_set_atmosphere(self.ctx.handle, C.byref(self.params.atmosphere)))
        objs = self.params.objects
        arr = (_abi.Object * max(1, len(objs)))(*objs)
        self.ctx.check(self.ctx.lib.atmrt_objects_set(self.ctx.handle, arr, len(objs)))
        return pod

    def generate(self) -> ResultPixels:
        self._configure()
        res = _abi.Result()
        self.ctx.check(self.ctx.lib.atmrt_generate(self.ctx.handle, C.byref(res)))
        try:
            return ResultPixels(_abi.result_to_numpy(res))
        finally:
            self.ctx.lib.atmrt_result_free(C.byref(res))

    def generate_device(self, planes: "_abi.DevicePlanes"):
        """Leave the first-hit planes in HBM (caller-owned device memory).  Returns (ray_steps, device_ms)."""
        self._configure()
        steps, ms = C.c_uint64(), C.c_double()
        self.ctx.check(self.ctx.lib.atmrt_generate_device(self.ctx.handle, C.byref(planes), C.byref(steps), C.byref(ms)))
        return steps.value, ms.value


    def generate_image_device(self, images):
        """The WHOLE [H][W] frame left in HBM on every device of the context (atmrt_generate_image_device): `images` is one
        _abi.DevicePlanes per device (a single one for a plain or rank context).  Returns (ray_steps, device_ms)."""
        self._configure()
        if isinstance(images, _abi.DevicePlanes):
            images = [images]
        arr = (_abi.DevicePlanes * len(images))(*images)
        steps, ms = C.c_uint64(), C.c_double()
        self.ctx.check(self.ctx.lib.atmrt_generate_image_device(self.ctx.handle, arr, C.byref(steps), C.byref(ms)))
        return steps.value, ms.value

    def image_hits_device(self, height, width, skip=()):
        """The trace-point lists of the frame generate_image_device just produced, in the image's pixel order, as torch tensors on
        every device of the context (one dict for a plain or rank context, a list for a multi-device one; the devices whose index
        is in `skip` take part in the exchange but get nothing: None): atmrt_image_hits_device.  The total is known to every rank
        since the frame's own collective (no communication); the fill is ONE collective over the ranks."""
        import torch
        n = C.c_uint64()
        self.ctx.check(self.ctx.lib.atmrt_image_hits_device(self.ctx.handle, None, C.byref(n)))
        devs = self.ctx.devices
        ts = [None if i in skip else _hit_tensors(n.value, height, width, torch.device("cuda", d)) for i, d in enumerate(devs)]
        pods = (_abi.DeviceHits * len(ts))(*[_abi.DeviceHits() if t is None else
                                             _abi.DeviceHits(capacity=n.value, **{k: v.data_ptr() for k, v in t.items()}) for t in ts])
        self.ctx.check(self.ctx.lib.atmrt_image_hits_device(self.ctx.handle, pods, None))
        return ts[0] if len(ts) == 1 else ts

    def last_hits_device(self, height, width):
        """Complete trace-point lists of the frame generate_device just produced, as torch tensors on the context's device:
        {hit_offset [H][W], lat, lon, distance, elevation, path_length, normal [n][3], color_tag, rgba [n][4]}."""
        import torch
        n = C.c_uint64()
        self.ctx.check(self.ctx.lib.atmrt_last_hits_device(self.ctx.handle, None, C.byref(n)))
        n = n.value
        t = _hit_tensors(n, height, width, torch.device("cuda", self.ctx.device))
        pod = _abi.DeviceHits(capacity=n, **{k: v.data_ptr() for k, v in t.items()})
        self.ctx.check(self.ctx.lib.atmrt_last_hits_device(self.ctx.handle, C.byref(pod), None))
        return t

    def last_stats(self):
        """atmrt_frame_stats_t of the last frame: how often it left the fast routes of the device path."""
        t = _abi.FrameStats()
        self.ctx.check(self.ctx.lib.atmrt_last_stats(self.ctx.handle, C.byref(t)))
        return {k: getattr(t, k) for k, _ in _abi.FrameStats._fields_}

    def last_timings(self):
        t = _abi.Timings()
        self.ctx.check(self.ctx.lib.atmrt_last_timings(self.ctx.handle, C.byref(t)))
        return {k: getattr(t, k) for k, _ in _abi.Timings._fields_}


def _hit_tensors(n, height, width, dev):
    """Device arrays laid out like the hit arrays of atmrt_result_t (atmrt_device_hits_t)."""
    import torch
    f64 = dict(dtype=torch.float64, device=dev)
    t = {k: torch.empty(n, **f64) for k in ("lat", "lon", "distance", "elevation", "path_length")}
    t["normal"] = torch.empty((n, 3), **f64)
    t["rgba"] = torch.empty((n, 4), **f64)
    t["color_tag"] = torch.empty(n, dtype=torch.int32, device=dev)
    t["hit_offset"] = torch.empty((height, width), dtype=torch.int64, device=dev)
    return t


def image_planes(height, width, dev):
    """[H][W] planes of a whole frame in HBM + the atmrt_device_planes_t that points at them."""
    import torch
    f64 = dict(dtype=torch.float64, device=dev)
    t = {k: torch.empty((height, width), **f64) for k in ("azimuth", "elevation_angle", "lat", "lon", "distance", "elevation", "path_length")}
    t["normal"] = torch.empty((3, height, width), **f64)
    t["hit_count"] = torch.empty((height, width), dtype=torch.int32, device=dev)
    return t, _abi.DevicePlanes(**{k: v.data_ptr() for k, v in t.items()})


class FastGenerator(Generator):
    KIND = _abi.GENERATORS["Fast"]


class RectilinearGenerator(Generator):
    KIND = _abi.GENERATORS["Rectilinear"]


class InterpolatingRectilinearGenerator(Generator):
    KIND = _abi.GENERATORS["InterpolatingRectilinear"]


def make_generator(params: Params, terrain: Terrain) -> Generator:
    """The `match params.output.generator` of generator::generate (src/generator/mod.rs:72-78)."""
    return {0: FastGenerator, 1: InterpolatingRectilinearGenerator, 2: RectilinearGenerator}[params.pod.generator](params, terrain)


# ---- renderer::draw_image (src/renderer/mod.rs:385-414) on the device -----------------------------
def into_coloring(lib, params_pod, conf):
    """ConfColoring::into_coloring (params.rs:231-277) -> atmrt_coloring_t."""
    col = _abi.Coloring()
    rc = lib.atmrt_coloring_from_conf(C.byref(params_pod), conf["kind"], conf["water_level"], conf["ambient_light"],
                                      conf["light_zenith_angle"], conf["light_dir"], conf["palette"], conf["has_fog"],
                                      conf["fog_distance"], C.byref(col))
    if rc != 0:
        raise AtmrtError(rc, "invalid colouring configuration")
    return col


def draw_image(ctx, coloring, width, height, shadows=None, bodies=None, sky=None, sky_light=None):
    """Composite the frame of the last generate() on `ctx` into an RGB8 image [height][width][3].  shadows: the status plane of
    shadow_mask() for that frame — under Shading the first trace point of a SHADOWED pixel is drawn at ambient_light.  bodies: sky
    bodies (sky_body() or (azimuth_deg, elevation_deg, radius_deg, rgb) each) drawn over the sky pixels their refracted rays meet;
    sky: the SkyDirections of that frame (default: sky_directions(ctx) with the spec's defaults).  sky_light: True, a dict of
    sky_shade's parameters (tau, limb, exposure, airlight) or a SkyLight of that frame — the sky pixels are shaded by air mass and
    the bodies (none if `bodies` is None) reddened and limb-darkened instead of drawn flat (include/atmrt.h, "sky light")."""
    rgb = np.zeros((height, width, 3), dtype=np.uint8)
    if shadows is None:
        ctx.check(ctx.lib.atmrt_draw_image(ctx.handle, C.byref(coloring), rgb.ctypes.data))
    else:
        status = np.ascontiguousarray(shadows, dtype=np.uint8)
        if status.size != width * height:
            raise AtmrtError(_abi.ERR_INVALID_ARGUMENT, f"the shadow status plane has {status.size} entries, the image {width * height} pixels")
        ctx.check(ctx.lib.atmrt_draw_image_shadowed(ctx.handle, C.byref(coloring), status.ctypes.data, rgb.ctypes.data))
    if sky_light is not None and sky_light is not False:
        light = sky_light if isinstance(sky_light, SkyLight) else sky
        if not isinstance(light, SkyLight):
            light = _sky_light_of_frame(ctx, width=width, height=height, steps=False)  # (the argument hides the function's name here)
        sky_shade(ctx, light, bodies or [], rgb, **(sky_light if isinstance(sky_light, dict) else {}))
    elif bodies is not None:
        if sky is None:
            sky = sky_directions(ctx, width=width, height=height, steps=False)
        sky_bodies(ctx, sky, bodies, rgb)
    return rgb


# ---- sky rays: the true direction of every sky pixel, sun and moon discs (include/atmrt.h, "sky rays") ----------------------
SKY_TOP, SKY_M, SUN_RADIUS_DEG = 100000.0, _abi.SKY_M_MAX, 0.2666
SKY_RAY_DTYPE = np.dtype([("status", "<i4"), ("steps", "<u4"), ("true_elevation", "<f8")])


class SkyDirections:
    """One sky call over a frame: true_elevation [height][width] f64 (NaN unless EXIT), status [height][width] u8 (_abi.SKY_*),
    steps [height][width] u32 (None if not asked for), stats (dict)."""

    def __init__(self, true_elevation, status, steps, stats):
        self.true_elevation, self.status, self.steps, self.stats = true_elevation, status, steps, stats


def sky_spec(step=0.0, top=SKY_TOP, floor=0.0, m=SKY_M):
    """atmrt_sky_spec_t.  step 0: the context's simulation_step."""
    return _abi.SkySpec(float(step), float(top), float(floor), int(m), 0)


def sky_body(azimuth_deg, elevation_deg, radius_deg=SUN_RADIUS_DEG, rgb=(255, 255, 224)):
    """atmrt_sky_body_t: the body's TRUE direction [deg], its angular radius [deg] and its colour."""
    r, g, b = (int(v) for v in rgb)
    return _abi.SkyBody(float(azimuth_deg), float(elevation_deg), float(radius_deg), (C.c_uint8 * 3)(r, g, b))


def _sky_bodies_array(bodies):
    bodies = [b if isinstance(b, _abi.SkyBody) else sky_body(*b) for b in bodies]
    return (_abi.SkyBody * max(1, len(bodies)))(*bodies), len(bodies)


def _sky_stats(st):
    return {k: int(getattr(st, k)) for k, _ in _abi.SkyStats._fields_}


def sky_ray_host(atmosphere, wavelength, earth, straight_rays, spec, h0, elevation_deg, lib=None):
    """atmrt_sky_ray_host (host code, no device): (status, steps, true_elevation) of one ray by the function the kernel's lanes run."""
    lib = lib or _lib.load()
    out = _abi.SkyRay()
    rc = lib.atmrt_sky_ray_host(C.byref(atmosphere), float(wavelength), C.byref(earth), int(bool(straight_rays)), C.byref(spec), float(h0),
                                float(elevation_deg), C.byref(out))
    if rc != 0:
        raise AtmrtError(rc, "atmrt_sky_ray_host refused its arguments")
    return out.status, out.steps, out.true_elevation


def sky_body_host(bodies, azimuth_deg, true_elevation_deg, lib=None):
    """atmrt_sky_body_host (host code, no device): k + 1 for the first body k that holds the direction, 0 for none."""
    lib = lib or _lib.load()
    arr, n = _sky_bodies_array(bodies)
    out = C.c_uint32()
    rc = lib.atmrt_sky_body_host(arr, n, float(azimuth_deg), float(true_elevation_deg), C.byref(out))
    if rc != 0:
        raise AtmrtError(rc, "atmrt_sky_body_host refused its arguments")
    return out.value


def sky_rays(ctx, h0, elevation_deg, **spec):
    """atmrt_sky_rays: the list call (and the refraction table), in the setting now on `ctx`.  spec: the arguments of sky_spec, or
    spec=an _abi.SkySpec.  Returns (records [n] of SKY_RAY_DTYPE, stats)."""
    sp = spec["spec"] if "spec" in spec else sky_spec(**spec)
    elev = np.ascontiguousarray(elevation_deg, dtype=np.float64).ravel()
    rec = np.zeros(elev.size, dtype=SKY_RAY_DTYPE)
    st = _abi.SkyStats()
    ctx.check(ctx.lib.atmrt_sky_rays(ctx.handle, C.byref(sp), float(h0), elev.size, elev.ctypes.data, rec.ctypes.data, C.byref(st)))
    return rec, _sky_stats(st)


def sky_directions(ctx, width=None, height=None, steps=True, **spec):
    """atmrt_sky_directions over the frame of the last generate() on `ctx`, in the setting now on the context.  Returns a SkyDirections."""
    sp = spec["spec"] if "spec" in spec else sky_spec(**spec)
    if width is None or height is None:
        p = ctx_params(ctx)
        width, height = int(p.width), int(p.height)
    true = np.zeros((height, width), dtype=np.float64)
    status = np.zeros((height, width), dtype=np.uint8)
    stp = np.zeros((height, width), dtype=np.uint32) if steps else None
    st = _abi.SkyStats()
    ctx.check(ctx.lib.atmrt_sky_directions(ctx.handle, C.byref(sp), true.ctypes.data, status.ctypes.data, None if stp is None else stp.ctypes.data,
                                           C.byref(st)))
    return SkyDirections(true, status, stp, _sky_stats(st))


def sky_bodies(ctx, sky, bodies, rgb=None):
    """atmrt_sky_bodies over the frame of the last generate() on `ctx`: the body plane [height][width] u8 (k + 1 for body k, 0 for
    none) from a SkyDirections of that frame; rgb: an RGB8 image [height][width][3] the discs are drawn into in place."""
    arr, n = _sky_bodies_array(bodies)
    true = np.ascontiguousarray(sky.true_elevation, dtype=np.float64)
    status = np.ascontiguousarray(sky.status, dtype=np.uint8)
    body = np.zeros(status.shape, dtype=np.uint8)
    if rgb is not None and not (rgb.dtype == np.uint8 and rgb.flags["C_CONTIGUOUS"] and rgb.size == 3 * status.size):
        raise AtmrtError(_abi.ERR_INVALID_ARGUMENT, "rgb must be a contiguous uint8 image [height][width][3] of the frame")
    ctx.check(ctx.lib.atmrt_sky_bodies(ctx.handle, arr, n, true.ctypes.data, status.ctypes.data, body.ctypes.data,
                                       None if rgb is None else rgb.ctypes.data))
    return body


def sky_timings(ctx):
    """atmrt_last_sky_timings of the last sky_rays / sky_directions call on `ctx`."""
    out = (C.c_double * 3)()
    ctx.check(ctx.lib.atmrt_last_sky_timings(ctx.handle, out))
    return dict(zip(("compact_ms", "march_ms", "download_ms"), out))


# ---- sky light: air mass per sky ray, a reddened sun, a shaded sky (include/atmrt.h, "sky light") ---------------------------
# This project's choice, with no reference counterpart: zenith optical depths per channel that give a blue zenith of about
# (59, 106, 217) and a horizon that saturates to white, and a limb darkening that is stronger toward the blue.
SKY_TAU, SUN_LIMB, SKY_EXPOSURE, SKY_AIRLIGHT = (0.06, 0.11, 0.24), (0.5, 0.6, 0.75), 4.0, (255, 255, 255)


class SkyLight(SkyDirections):
    """One sky-light call over a frame: a SkyDirections with column [height][width] f64 (NaN unless EXIT) and zenith_column (Z0);
    air_mass is their quotient."""

    def __init__(self, true_elevation, status, steps, stats, column, zenith_column):
        super().__init__(true_elevation, status, steps, stats)
        self.column, self.zenith_column = column, zenith_column

    @property
    def air_mass(self):
        return self.column / self.zenith_column


def sky_light_spec(ref_alt=0.0, column_dz=0.0, **sky):
    """atmrt_sky_light_spec_t.  ref_alt: the altitude whose zenith is air mass 1; column_dz 0: the step of the march; the rest: the
    arguments of sky_spec, or sky=an _abi.SkySpec."""
    sp = sky["sky"] if "sky" in sky else sky_spec(**sky)
    return _abi.SkyLightSpec(sp, float(ref_alt), float(column_dz))


def sky_shade_params(zenith_column, tau=SKY_TAU, limb=SUN_LIMB, exposure=SKY_EXPOSURE, airlight=SKY_AIRLIGHT):
    """atmrt_sky_shade_t."""
    return _abi.SkyShade(float(zenith_column), (C.c_double * 3)(*[float(v) for v in tau]), (C.c_double * 3)(*[float(v) for v in limb]),
                         float(exposure), (C.c_uint8 * 3)(*[int(v) for v in airlight]))


def sky_zenith_column(atmosphere, wavelength, ref_alt=0.0, top=100000.0, dz=100.0, lib=None):
    """atmrt_sky_zenith_column_host (host code, no device): Z0(ref_alt, top, dz) [m] of the atmosphere."""
    lib = lib or _lib.load()
    out = C.c_double()
    rc = lib.atmrt_sky_zenith_column_host(C.byref(atmosphere), float(wavelength), float(ref_alt), float(top), float(dz), C.byref(out))
    if rc != 0:
        raise AtmrtError(rc, "atmrt_sky_zenith_column_host refused its arguments")
    return out.value


def sky_light_ray_host(atmosphere, wavelength, earth, straight_rays, spec, h0, elevation_deg, lib=None):
    """atmrt_sky_light_ray_host (host code, no device): (status, steps, true_elevation, column) of one ray by the function the
    kernel's lanes run."""
    lib = lib or _lib.load()
    out, column = _abi.SkyRay(), C.c_double()
    rc = lib.atmrt_sky_light_ray_host(C.byref(atmosphere), float(wavelength), C.byref(earth), int(bool(straight_rays)), C.byref(spec), float(h0),
                                      float(elevation_deg), C.byref(out), C.byref(column))
    if rc != 0:
        raise AtmrtError(rc, "atmrt_sky_light_ray_host refused its arguments")
    return out.status, out.steps, out.true_elevation, column.value


def sky_shade_host(shade, bodies, azimuth_deg, true_elevation_deg, column, lib=None):
    """atmrt_sky_shade_host (host code, no device): (body, (r, g, b)) of one EXIT pixel."""
    lib = lib or _lib.load()
    arr, n = _sky_bodies_array(bodies)
    body, rgb = C.c_uint32(), (C.c_uint8 * 3)()
    rc = lib.atmrt_sky_shade_host(C.byref(shade), arr, n, float(azimuth_deg), float(true_elevation_deg), float(column), C.byref(body), rgb)
    if rc != 0:
        raise AtmrtError(rc, "atmrt_sky_shade_host refused its arguments")
    return body.value, tuple(rgb)


def sky_light_rays(ctx, h0, elevation_deg, **spec):
    """atmrt_sky_light_rays: sky_rays with the column of every ray.  Returns (records [n] of SKY_RAY_DTYPE, column [n] f64, stats)."""
    sp = spec["spec"] if "spec" in spec else sky_spec(**spec)
    elev = np.ascontiguousarray(elevation_deg, dtype=np.float64).ravel()
    rec = np.zeros(elev.size, dtype=SKY_RAY_DTYPE)
    column = np.zeros(elev.size, dtype=np.float64)
    st = _abi.SkyStats()
    ctx.check(ctx.lib.atmrt_sky_light_rays(ctx.handle, C.byref(sp), float(h0), elev.size, elev.ctypes.data, rec.ctypes.data, column.ctypes.data,
                                           C.byref(st)))
    return rec, column, _sky_stats(st)


def sky_light(ctx, width=None, height=None, steps=True, ref_alt=0.0, column_dz=0.0, **spec):
    """atmrt_sky_light over the frame of the last generate() on `ctx`: sky_directions with the column plane and the zenith column.
    spec: the arguments of sky_spec, or spec=an _abi.SkyLightSpec.  Returns a SkyLight."""
    sp = spec["spec"] if "spec" in spec else sky_light_spec(ref_alt, column_dz, **spec)
    if width is None or height is None:
        p = ctx_params(ctx)
        width, height = int(p.width), int(p.height)
    true = np.zeros((height, width), dtype=np.float64)
    column = np.zeros((height, width), dtype=np.float64)
    status = np.zeros((height, width), dtype=np.uint8)
    stp = np.zeros((height, width), dtype=np.uint32) if steps else None
    st, z0 = _abi.SkyStats(), C.c_double()
    ctx.check(ctx.lib.atmrt_sky_light(ctx.handle, C.byref(sp), true.ctypes.data, status.ctypes.data, None if stp is None else stp.ctypes.data,
                                      column.ctypes.data, C.byref(st), C.byref(z0)))
    return SkyLight(true, status, stp, _sky_stats(st), column, z0.value)


_sky_light_of_frame = sky_light  # draw_image(sky_light=) calls it


def sky_shade(ctx, light, bodies, rgb, **shade):
    """atmrt_sky_shade over the frame of the last generate() on `ctx`: the EXIT pixels of the RGB8 image `rgb` [height][width][3]
    shaded in place from a SkyLight of that frame — the airlight by air mass, the bodies' discs reddened and limb-darkened.  shade:
    tau, limb, exposure, airlight (sky_shade_params), or shade=an _abi.SkyShade.  Returns the body plane [height][width] u8."""
    sh = shade["shade"] if "shade" in shade else sky_shade_params(light.zenith_column, **shade)
    arr, n = _sky_bodies_array(bodies)
    true = np.ascontiguousarray(light.true_elevation, dtype=np.float64)
    column = np.ascontiguousarray(light.column, dtype=np.float64)
    status = np.ascontiguousarray(light.status, dtype=np.uint8)
    body = np.zeros(status.shape, dtype=np.uint8)
    if not (isinstance(rgb, np.ndarray) and rgb.dtype == np.uint8 and rgb.flags["C_CONTIGUOUS"] and rgb.size == 3 * status.size):
        raise AtmrtError(_abi.ERR_INVALID_ARGUMENT, "rgb must be a contiguous uint8 image [height][width][3] of the frame")
    ctx.check(ctx.lib.atmrt_sky_shade(ctx.handle, C.byref(sh), arr, n, true.ctypes.data, status.ctypes.data, column.ctypes.data, body.ctypes.data,
                                      rgb.ctypes.data))
    return body


def sky_shade_timing(ctx):
    """atmrt_last_sky_shade_timing: the milliseconds of the last sky_shade call's kernel on `ctx`."""
    out = C.c_double()
    ctx.check(ctx.lib.atmrt_last_sky_shade_timing(ctx.handle, C.byref(out)))
    return out.value


# ---- apparent elevation: the refraction table and its inverse (include/atmrt.h, "apparent elevation") ----------------------
SKY_TABLE_ALT, SKY_TABLE_EL = (0.0, 9000.0, 33), (-4.0, 88.0, 4601)


class SkyTable:
    """One atmrt_sky_table call: true_elevation [n_alt][n_el] f64 (NaN unless EXIT), status [n_alt][n_el] u8, tail [n_alt] u32, stats
    (of the march that built the table), rebuilt (this call built it) and ms (march, tail, download), the spec."""

    def __init__(self, spec, true_elevation, status, tail, stats, rebuilt, ms):
        self.spec, self.true_elevation, self.status, self.tail, self.stats, self.rebuilt, self.ms = spec, true_elevation, status, tail, stats, rebuilt, ms

    @property
    def usable(self):
        return self.tail.astype(np.int64) <= self.spec.n_el - 2


def sky_table_spec(alt=SKY_TABLE_ALT, el=SKY_TABLE_EL, **sky):
    """atmrt_sky_table_spec_t.  alt: (lo, hi, n) [m]; el: (lo, hi, n) [deg]; the rest: the arguments of sky_spec, or sky=an _abi.SkySpec."""
    sp = sky["sky"] if "sky" in sky else sky_spec(**sky)
    return _abi.SkyTableSpec(sp, float(alt[0]), float(alt[1]), float(el[0]), float(el[1]), int(alt[2]), int(el[2]))


def sky_table_work(ctx):
    """atmrt_last_sky_table_work: (rebuilt, {march_ms, tail_ms, download_ms}) of the last call on `ctx` that needed the table."""
    rebuilt, ms = C.c_int32(), (C.c_double * 3)()
    ctx.check(ctx.lib.atmrt_last_sky_table_work(ctx.handle, C.byref(rebuilt), ms))
    return rebuilt.value, dict(zip(("march_ms", "tail_ms", "download_ms"), ms))


def sky_table(ctx, spec=None, planes=True):
    """atmrt_sky_table: the refraction table of the setting now on `ctx`, built or found.  planes=False: the tail alone."""
    spec = spec or sky_table_spec()
    shape = (spec.n_alt, spec.n_el)
    true = np.zeros(shape, dtype=np.float64) if planes else None
    status = np.zeros(shape, dtype=np.uint8) if planes else None
    tail = np.zeros(spec.n_alt, dtype=np.uint32)
    st = _abi.SkyStats()
    ctx.check(ctx.lib.atmrt_sky_table(ctx.handle, C.byref(spec), *[None if a is None else a.ctypes.data for a in (true, status)], tail.ctypes.data,
                                      C.byref(st)))
    rebuilt, ms = sky_table_work(ctx)
    return SkyTable(spec, true, status, tail, _sky_stats(st), rebuilt, ms)


def sky_tail_host(spec, true_elevation, status, lib=None):
    """atmrt_sky_tail_host (host code, no device): tail [n_alt] of the caller's planes."""
    lib = lib or _lib.load()
    true = np.ascontiguousarray(true_elevation, dtype=np.float64)
    status = np.ascontiguousarray(status, dtype=np.uint8)
    assert true.size == status.size == spec.n_alt * spec.n_el
    tail = np.zeros(spec.n_alt, dtype=np.uint32)
    rc = lib.atmrt_sky_tail_host(C.byref(spec), true.ctypes.data, status.ctypes.data, tail.ctypes.data)
    if rc != 0:
        raise AtmrtError(rc, "atmrt_sky_tail_host refused its arguments")
    return tail


def sky_apparent_host(spec, true_elevation, tail, h, t, lib=None):
    """atmrt_sky_apparent_host (host code, no device): apparent(h, t) over the caller's table by the function the kernels run."""
    lib = lib or _lib.load()
    true = np.ascontiguousarray(true_elevation, dtype=np.float64)
    tail = np.ascontiguousarray(tail, dtype=np.uint32)
    assert true.size == spec.n_alt * spec.n_el and tail.size == spec.n_alt
    out = C.c_double()
    rc = lib.atmrt_sky_apparent_host(C.byref(spec), true.ctypes.data, tail.ctypes.data, float(h), float(t), C.byref(out))
    if rc != 0:
        raise AtmrtError(rc, "atmrt_sky_apparent_host refused its arguments")
    return out.value


def sky_apparent(ctx, h, t, spec=None):
    """atmrt_sky_apparent: where a body of true elevation t[i] [deg] appears from altitude h[i] [m], in the setting now on `ctx`."""
    spec = spec or sky_table_spec()
    h, t = np.ascontiguousarray(h, dtype=np.float64).ravel(), np.ascontiguousarray(t, dtype=np.float64).ravel()
    if h.size != t.size:
        raise AtmrtError(_abi.ERR_INVALID_ARGUMENT, f"{h.size} altitudes for {t.size} true elevations")
    out = np.zeros(h.size, dtype=np.float64)
    ctx.check(ctx.lib.atmrt_sky_apparent(ctx.handle, C.byref(spec), h.size, h.ctypes.data, t.ctypes.data, out.ctypes.data))
    return out


# ---- cast shadows: which of the frame's first trace points the light reaches (include/atmrt.h) ------------------------------
class ShadowMask:
    """One shadow call: status [height][width] u8 (_abi.SHADOW_*), block [height][width] u16 (None if not asked for), stats (dict)."""

    def __init__(self, status, block, stats):
        self.status, self.block, self.stats = status, block, stats


def shadow_spec(azimuth_deg, elevation_deg, reach, lift=0.0):
    return _abi.ShadowSpec(float(azimuth_deg), float(elevation_deg), float(reach), float(lift))


def light_from_coloring(params_pod, light_zenith_angle, light_dir):
    """(azimuth_deg, elevation_deg) of the Shading configuration's light for a shadow spec.  ConfColoring::into_coloring
    (params.rs:250-258) builds the light's horizontal part as -front cos(d) + right sin(d), d = light_dir: front points along
    frame.direction and right 90 degrees clockwise of it, so the direction toward the light is frame.direction + 180 - light_dir;
    light_zenith_angle counts from the vertical, so the elevation is 90 - light_zenith_angle."""
    return params_pod.frame.direction + 180.0 - float(light_dir), 90.0 - float(light_zenith_angle)


def shadow_steps(ctx, reach):
    """atmrt_shadow_steps: m for `reach` under the parameters now set on `ctx`."""
    m = C.c_int32()
    ctx.check(ctx.lib.atmrt_shadow_steps(ctx.handle, float(reach), C.byref(m)))
    return m.value


def _shadow_stats(st):
    return {k: int(getattr(st, k)) for k, _ in _abi.ShadowStats._fields_}


def shadow_mask(ctx, spec, width=None, height=None, block=True):
    """atmrt_shadow_mask over the frame of the last generate() on `ctx`, in the setting now on the context.  spec: an
    _abi.ShadowSpec, or (azimuth_deg, elevation_deg, reach[, lift]).  Returns a ShadowMask."""
    if not isinstance(spec, _abi.ShadowSpec):
        spec = shadow_spec(*spec)
    if width is None or height is None:
        p = ctx_params(ctx)
        width, height = int(p.width), int(p.height)
    status = np.zeros((height, width), dtype=np.uint8)
    blk = np.zeros((height, width), dtype=np.uint16) if block else None
    st = _abi.ShadowStats()
    ctx.check(ctx.lib.atmrt_shadow_mask(ctx.handle, C.byref(spec), status.ctypes.data, None if blk is None else blk.ctypes.data, C.byref(st)))
    return ShadowMask(status, blk, _shadow_stats(st))


# ---- shadow lights: a direction per point and a list of lights per call (include/atmrt.h, "shadow lights") ------------------
class ShadowLights:
    """One shadow-lights call: lit_mask [height][width] u64 (bit l: light l reaches the pixel's first trace point), status
    [n_lights][height][width] u8 and block [n_lights][height][width] u16 (None if not asked for), stats (dict), dirs [n_lights][3]."""

    def __init__(self, lit_mask, status, block, stats, dirs):
        self.lit_mask, self.status, self.block, self.stats, self.dirs = lit_mask, status, block, stats, dirs


def shadow_light_direction(earth, lat, lon, azimuth_deg, elevation_deg, lib=None):
    """atmrt_shadow_light_direction (host code, no device): the world-frame vector of a light seen from (lat, lon) under
    (azimuth_deg, elevation_deg).  earth: an _abi.EarthModel (params.earth)."""
    lib = lib or _lib.load()
    out = (C.c_double * 3)()
    rc = lib.atmrt_shadow_light_direction(C.byref(earth), float(lat), float(lon), float(azimuth_deg), float(elevation_deg), out)
    if rc != 0:
        raise AtmrtError(rc, "atmrt_shadow_light_direction refused its arguments")
    return np.array(out[:], dtype=np.float64)


def shadow_local_direction(earth, direction, lat, lon, lib=None):
    """atmrt_shadow_local_direction (host code, no device): (azimuth_deg, elevation_deg) of the world-frame light `direction` in
    the local frame of (lat, lon) — the function the kernel runs."""
    lib = lib or _lib.load()
    d = (C.c_double * 3)(*[float(v) for v in direction])
    az, el = C.c_double(), C.c_double()
    rc = lib.atmrt_shadow_local_direction(C.byref(earth), d, float(lat), float(lon), C.byref(az), C.byref(el))
    if rc != 0:
        raise AtmrtError(rc, "atmrt_shadow_local_direction refused its arguments")
    return az.value, el.value


def lights_from_angles(params_pod, rows, lib=None):
    """rows of (azimuth_deg, elevation_deg) as seen from the observer of `params_pod` -> dirs [n][3], world frame."""
    pos = params_pod.position
    return np.array([shadow_light_direction(params_pod.earth, pos.latitude, pos.longitude, az, el, lib) for az, el in rows],
                    dtype=np.float64).reshape(-1, 3)


def shadow_lights_spec(dirs, reach, lift=0.0):
    """-> (_abi.ShadowLightsSpec, dirs [n][3] f64 contiguous): the array must outlive the spec, which borrows it."""
    dirs = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
    spec = _abi.ShadowLightsSpec(dirs.ctypes.data_as(C.POINTER(C.c_double)), dirs.shape[0], 0, float(reach), float(lift))
    return spec, dirs


def shadow_lights(ctx, dirs, reach, lift=0.0, status=False, block=False, width=None, height=None, mask=True, true_table=None):
    """atmrt_shadow_lights over the frame of the last generate() on `ctx`, in the setting now on the context.  dirs: [n_lights][3]
    world-frame vectors toward the lights (lights_from_angles, or a coloring's light_dir).  true_table: None, or the
    _abi.SkyTableSpec (sky_table_spec) of the refraction table: the vectors are then the lights' TRUE directions and every shadow
    ray is launched where its light appears (atmrt_shadow_lights_true).  Returns a ShadowLights."""
    spec, dirs = shadow_lights_spec(dirs, reach, lift)
    if width is None or height is None:
        p = ctx_params(ctx)
        width, height = int(p.width), int(p.height)
    n = dirs.shape[0]
    lit = np.zeros((height, width), dtype=np.uint64) if mask else None
    sta = np.zeros((n, height, width), dtype=np.uint8) if status else None
    blk = np.zeros((n, height, width), dtype=np.uint16) if block else None
    st = _abi.ShadowStats()
    out = [None if a is None else a.ctypes.data for a in (lit, sta, blk)]
    if true_table is None:
        ctx.check(ctx.lib.atmrt_shadow_lights(ctx.handle, C.byref(spec), *out, C.byref(st)))
    else:
        ctx.check(ctx.lib.atmrt_shadow_lights_true(ctx.handle, C.byref(spec), C.byref(true_table), *out, C.byref(st)))
    return ShadowLights(lit, sta, blk, _shadow_stats(st), dirs)


def shadow_timings(ctx):
    """atmrt_last_shadow_timings of the last shadow call on `ctx`."""
    out = (C.c_double * 3)()
    ctx.check(ctx.lib.atmrt_last_shadow_timings(ctx.handle, out))
    return dict(zip(("compact_ms", "march_ms", "download_ms"), out))


# ---- the annotations of renderer::output_image (src/renderer/mod.rs:28-365, 416-431) on the device -----------------------
def into_overlay(output):
    """output.ticks / vertical_ticks / show_eye_level / show_flat_horizon as config.Config.output holds them -> atmrt_overlay_t."""
    def tick(t):
        if t[0] == "Single":
            _, angle, size, labelled = t
            return _abi.Tick(kind=_abi.TICK_SINGLE, size=size, angle=angle, labelled=int(labelled))
        _, bias, step, size, labelled = t
        return _abi.Tick(kind=_abi.TICK_MULTIPLE, size=size, bias=bias, step=step, labelled=int(labelled))
    return _abi.Overlay.new([tick(t) for t in output.get("ticks", [])], [tick(t) for t in output.get("vertical_ticks", [])],
                            output.get("show_eye_level", False), output.get("show_flat_horizon", False))


def _drawn_ticks(arr, n):
    return [{"pos": t.pos, "size": t.size, "labelled": bool(t.labelled), "vertical": bool(t.vertical), "label": t.label.decode()}
            for t in arr[:n]]


def resolve_ticks(params_pod, overlay, azimuth_row0, elevation_col0, lib=None):
    """atmrt_overlay_resolve_ticks (host code, no device): the ticks gen_ticks would draw, sorted by (vertical, pos)."""
    lib = lib or _lib.load()
    az = np.ascontiguousarray(azimuth_row0, dtype=np.float64)
    el = np.ascontiguousarray(elevation_col0, dtype=np.float64)
    n = C.c_size_t()
    rc = lib.atmrt_overlay_resolve_ticks(C.byref(params_pod), C.byref(overlay), az.ctypes.data, el.ctypes.data, None, 0, C.byref(n))
    if rc != 0:
        raise AtmrtError(rc, "atmrt_overlay_resolve_ticks refused its arguments")
    arr = (_abi.DrawnTick * max(1, n.value))()
    rc = lib.atmrt_overlay_resolve_ticks(C.byref(params_pod), C.byref(overlay), az.ctypes.data, el.ctypes.data, arr, n.value, C.byref(n))
    if rc != 0:
        raise AtmrtError(rc, "atmrt_overlay_resolve_ticks refused its arguments")
    return _drawn_ticks(arr, n.value)


def _max_ticks(overlay, width, height):
    # one tick per pixel position at most: two definitions on one pixel leave one tick
    return (width if overlay.n_ticks else 0) + (height if overlay.n_vertical_ticks else 0)


def draw_overlay(ctx, overlay, rgb):
    """Ticks, flat-horizon and eye-level lines of the last generate() on `ctx` drawn over `rgb` ([height][width][3] uint8, e.g. of
    draw_image).  Returns (image, ticks, flat_horizon_deg): the resolved ticks carry the label strings for the host to
    rasterise; flat_horizon_deg is NaN when that line is not drawn."""
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8).copy()
    cap = _max_ticks(overlay, rgb.shape[1], rgb.shape[0])
    arr, n, deg = (_abi.DrawnTick * max(1, cap))(), C.c_size_t(), C.c_double()
    ctx.check(ctx.lib.atmrt_draw_overlay(ctx.handle, C.byref(overlay), rgb.ctypes.data, arr, cap, C.byref(n), C.byref(deg)))
    return rgb, _drawn_ticks(arr, n.value), deg.value


def draw_overlay_device(ctx, overlay, rgb_ptr, width, height, planes=None):
    """The same on a device image (a raw pointer, e.g. tensor.data_ptr()); planes = (azimuth_ptr, elevation_angle_ptr) draws on
    explicit [height][width] device planes (a gathered multi-device frame) instead of the context's last frame.
    Returns (ticks, flat_horizon_deg)."""
    cap = _max_ticks(overlay, width, height)
    arr, n, deg = (_abi.DrawnTick * max(1, cap))(), C.c_size_t(), C.c_double()
    if planes is None:
        ctx.check(ctx.lib.atmrt_draw_overlay_device(ctx.handle, C.byref(overlay), rgb_ptr, arr, cap, C.byref(n), C.byref(deg)))
    else:
        ctx.check(ctx.lib.atmrt_draw_overlay_planes_device(ctx.handle, C.byref(overlay), planes[0], planes[1], width, height, rgb_ptr,
                                                           arr, cap, C.byref(n), C.byref(deg)))
    return _drawn_ticks(arr, n.value), deg.value


# ---- the visibility map: the frame's trace points binned over a latitude / longitude grid (no reference counterpart) ------
GeoGrid = _abi.GeoGrid


def geo_grid_cell(grid, lat, lon, lib=None):
    """atmrt_geo_grid_cell (host code, no device) for scalars or arrays: the cell index i * n_lon + j of every point, -1 outside."""
    lib = lib or _lib.load()
    lat, lon = np.broadcast_arrays(np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64))
    out = np.empty(lat.shape, dtype=np.int64)
    cell = C.c_int64()
    flat = out.reshape(-1)
    for i, (a, b) in enumerate(zip(lat.ravel().tolist(), lon.ravel().tolist())):
        rc = lib.atmrt_geo_grid_cell(C.byref(grid), a, b, C.byref(cell))
        if rc != 0:
            raise AtmrtError(rc, "atmrt_geo_grid_cell refused the grid")
        flat[i] = cell.value
    return out if out.ndim else int(out)


def snap_grid(bounds, cell_lat, cell_lon=None):
    """The grid that covers bounds = (lat_min, lat_max, lon_min, lon_max), snapped outward to multiples of the cell size; a point
    exactly on the snapped top or right edge gets a row / column of its own.  None when the bounds are NaN (no trace point)."""
    cell_lon = cell_lat if cell_lon is None else cell_lon
    if any(np.isnan(b) for b in bounds):
        return None

    def axis(lo, hi, cell):  # first cell index and cell count; the binning rule itself has the last word on both ends
        i0 = int(np.floor(lo / cell))
        while np.floor((lo - i0 * cell) / cell) < 0:
            i0 -= 1
        n = int(np.floor(hi / cell)) - i0 + 1
        while np.floor((hi - i0 * cell) / cell) >= n:
            n += 1
        return i0 * cell, n

    (lat0, n_lat), (lon0, n_lon) = axis(bounds[0], bounds[1], cell_lat), axis(bounds[2], bounds[3], cell_lon)
    return GeoGrid(lat0, lon0, cell_lat, cell_lon, n_lat, n_lon)


def _vis_stats(st):
    return {k: getattr(st, k) for k, _ in _abi.VisibilityStats._fields_}


def frame_bounds(ctx, mode="first"):
    """(lat_min, lat_max, lon_min, lon_max) over the trace points of the last generate() on `ctx` that `mode` ("first" / "all")
    would bin; all NaN for a frame without one."""
    out = (C.c_double * 4)()
    ctx.check(ctx.lib.atmrt_frame_bounds(ctx.handle, _abi.VIS_MODES[mode], out))
    return tuple(out)


def visibility_map(ctx, grid, mode="first"):
    """The visibility map of the last generate() on `ctx`: (count [n_lat][n_lon] uint32, min_distance [n_lat][n_lon] float64 with
    +inf in empty cells, stats dict)."""
    count = np.empty((grid.n_lat, grid.n_lon), dtype=np.uint32)
    mind = np.empty((grid.n_lat, grid.n_lon), dtype=np.float64)
    st = _abi.VisibilityStats()
    ctx.check(ctx.lib.atmrt_visibility_map(ctx.handle, C.byref(grid), _abi.VIS_MODES[mode], count.ctypes.data, mind.ctypes.data, C.byref(st)))
    return count, mind, _vis_stats(st)


def visibility_map_device(ctx, grid, mode="first", planes=None, device=None):
    """The same left in HBM as torch tensors (count int32 — the bits of the u32 counts — and min_distance float64).  planes = a dict
    of [H][W] torch tensors lat, lon, distance, hit_count bins explicit planes (a gathered multi-device frame; "first" only)
    instead of the context's last frame.  Returns (count, min_distance, stats)."""
    import torch
    if planes is not None:
        dev = planes["lat"].device
    else:
        dev = torch.device("cuda", ctx.device if device is None else device)
    count = torch.empty((grid.n_lat, grid.n_lon), dtype=torch.int32, device=dev)
    mind = torch.empty((grid.n_lat, grid.n_lon), dtype=torch.float64, device=dev)
    st = _abi.VisibilityStats()
    if planes is None:
        ctx.check(ctx.lib.atmrt_visibility_map_device(ctx.handle, C.byref(grid), _abi.VIS_MODES[mode], count.data_ptr(), mind.data_ptr(), C.byref(st)))
    else:
        if mode != "first":
            raise ValueError("explicit planes hold the first trace point of every pixel: mode must be 'first'")
        h, w = planes["lat"].shape
        ctx.check(ctx.lib.atmrt_visibility_map_planes_device(ctx.handle, C.byref(grid), planes["lat"].data_ptr(), planes["lon"].data_ptr(),
                                                             planes["distance"].data_ptr(), planes["hit_count"].data_ptr(), w, h,
                                                             count.data_ptr(), mind.data_ptr(), C.byref(st)))
    return count, mind, _vis_stats(st)


# ---- landmarks: the nearest trace point of each latitude / longitude (no reference counterpart) ---------------------------
LANDMARK_HIT_DTYPE = np.dtype([("n_within", np.uint32), ("x", np.uint32), ("y", np.uint32), ("point", np.uint32), ("d2", np.float64),
                               ("distance", np.float64), ("elevation", np.float64)])
assert LANDMARK_HIT_DTYPE.itemsize == C.sizeof(_abi.LandmarkHit)


def landmark_scale(lat):
    """What a degree of longitude is worth against a degree of latitude at `lat`: cos(radians(lat)), the lon_scale the mirrors fill in."""
    return np.cos(np.radians(lat))


def landmarks(lat, lon, lon_scale=None):
    """The ctypes array of atmrt_landmark_t for equally long sequences lat, lon [deg]; lon_scale defaults to landmark_scale(lat)."""
    lat, lon = np.atleast_1d(np.asarray(lat, dtype=np.float64)), np.atleast_1d(np.asarray(lon, dtype=np.float64))
    scale = landmark_scale(lat) if lon_scale is None else np.broadcast_to(np.asarray(lon_scale, dtype=np.float64), lat.shape)
    if lat.shape != lon.shape or lat.ndim != 1:
        raise ValueError("lat and lon must be sequences of one length")
    packed = np.ascontiguousarray(np.stack([lat, lon, scale], axis=1))
    arr = (_abi.Landmark * lat.size)()
    C.memmove(arr, packed.ctypes.data, packed.nbytes)
    return arr


def landmark_d2(landmark, lat, lon, lib=None):
    """atmrt_landmark_d2 (host code, no device) for scalars or arrays of trace-point coordinates."""
    lib = lib or _lib.load()
    lat, lon = np.broadcast_arrays(np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64))
    out = np.empty(lat.shape, dtype=np.float64)
    d2 = C.c_double()
    flat = out.reshape(-1)
    for i, (a, b) in enumerate(zip(lat.ravel().tolist(), lon.ravel().tolist())):
        rc = lib.atmrt_landmark_d2(C.byref(landmark), a, b, C.byref(d2))
        if rc != 0:
            raise AtmrtError(rc, "atmrt_landmark_d2 refused its arguments")
        flat[i] = d2.value
    return out if out.ndim else float(out)


def locate_landmarks(ctx, landmarks, radius_deg, mode="first", planes=None):
    """Locates the landmarks (the array landmarks() makes) in the last generate() on `ctx`: per landmark the number of trace points
    within radius_deg and the nearest of them.  planes = a dict of [H][W] torch tensors lat, lon, distance, elevation, hit_count
    searches explicit planes (a gathered multi-device frame; "first" only).  "Not found" (n_within == 0) does not say whether the
    landmark is outside the field of view or hidden behind terrain.  Returns (records, a structured array of LANDMARK_HIT_DTYPE; stats dict)."""
    n = len(landmarks)
    hits = np.empty(n, dtype=LANDMARK_HIT_DTYPE)
    st = _abi.LandmarkStats()
    if planes is None:
        ctx.check(ctx.lib.atmrt_locate_landmarks(ctx.handle, landmarks, n, radius_deg, _abi.VIS_MODES[mode], hits.ctypes.data, C.byref(st)))
    else:
        if mode != "first":
            raise ValueError("explicit planes hold the first trace point of every pixel: mode must be 'first'")
        h, w = planes["lat"].shape
        ctx.check(ctx.lib.atmrt_locate_landmarks_planes_device(ctx.handle, landmarks, n, radius_deg, planes["lat"].data_ptr(), planes["lon"].data_ptr(),
                                                               planes["distance"].data_ptr(), planes["elevation"].data_ptr(),
                                                               planes["hit_count"].data_ptr(), w, h, hits.ctypes.data, C.byref(st)))
    return hits, {k: getattr(st, k) for k, _ in _abi.LandmarkStats._fields_}


def landmark_timings(ctx):
    """atmrt_last_landmark_timings: milliseconds of the last locate_landmarks on `ctx`."""
    out = (C.c_double * 5)()
    ctx.check(ctx.lib.atmrt_last_landmark_timings(ctx.handle, out))
    return dict(zip(("index_build_ms", "upload_reset_ms", "pass_a_ms", "pass_b_ms", "pass_c_ms"), out))


def landmark_index_probe(landmarks, radius_deg, bounds, lat, lon, lib=None):
    """atmrt_landmark_index_probe (host code, a diagnostic): the candidate landmarks the library's filter yields for every point, for
    a frame with bounds (lat_min, lat_max, lon_min, lon_max).  Returns (offsets [n_points + 1] uint64, items uint32)."""
    lib = lib or _lib.load()
    lat, lon = np.ascontiguousarray(lat, dtype=np.float64), np.ascontiguousarray(lon, dtype=np.float64)
    b = (C.c_double * 4)(*bounds)
    offsets = np.zeros(lat.size + 1, dtype=np.uint64)
    need = C.c_size_t()
    items = np.empty(max(4 * lat.size, 1), dtype=np.uint32)
    for _ in range(2):
        rc = lib.atmrt_landmark_index_probe(landmarks, len(landmarks), radius_deg, b, lat.ctypes.data, lon.ctypes.data, lat.size, offsets.ctypes.data,
                                            items.ctypes.data, items.size, C.byref(need))
        if rc == 0:
            return offsets, items[:need.value].copy()
        if need.value <= items.size:
            raise AtmrtError(rc, "atmrt_landmark_index_probe refused its arguments")
        items = np.empty(need.value, dtype=np.uint32)
    raise AtmrtError(rc, "atmrt_landmark_index_probe refused its arguments")


# ---- the landmark tables of the command line (gen --landmarks FILE.csv) -----------------------------------------------------
LANDMARK_COLUMNS = ("name", "lat", "lon", "found", "x", "y", "point", "offset_arcsec", "distance_m", "elevation_m", "n_within")


def read_landmarks_csv(path):
    """name,lat,lon rows (a header line is optional: a first row whose lat and lon are no numbers) -> (names, lat, lon)."""
    import csv
    names, lat, lon = [], [], []
    with open(path, newline="") as f:
        for i, row in enumerate(csv.reader(f)):
            if not row or not "".join(row).strip():
                continue
            if len(row) < 3:
                raise ValueError(f"{path}: line {i + 1}: expected name,lat,lon")
            try:
                a, b = float(row[1]), float(row[2])
            except ValueError:
                if not names and i == 0:
                    continue
                raise ValueError(f"{path}: line {i + 1}: lat and lon must be numbers")
            names.append(row[0].strip()), lat.append(a), lon.append(b)
    return names, np.array(lat, dtype=np.float64), np.array(lon, dtype=np.float64)


def write_landmarks_csv(f, names, lat, lon, hits):
    """The located table, LANDMARK_COLUMNS, to the open text file f; floats in Python's repr.  offset_arcsec = 3600 sqrt(d2)."""
    import csv
    w = csv.writer(f, lineterminator="\n")
    w.writerow(LANDMARK_COLUMNS)
    for name, a, b, h in zip(names, lat.tolist(), lon.tolist(), hits):
        if h["n_within"]:
            w.writerow([name, repr(a), repr(b), 1, int(h["x"]), int(h["y"]), int(h["point"]), repr(float(np.sqrt(h["d2"]) * 3600.0)),
                        repr(float(h["distance"])), repr(float(h["elevation"])), int(h["n_within"])])
        else:
            w.writerow([name, repr(a), repr(b), 0, "", "", "", "", "", "", 0])


# ---- sight lines: where a target appears and what terrain hides it (include/atmrt.h, no reference counterpart) -------------
SIGHT_DTYPE = np.dtype([("status", np.int32), ("rounds_done", np.int32), ("m", np.int32), ("block_index", np.int32)] +
                       [(k, np.float64) for k in ("angle", "arrival", "ground", "hidden", "resolution", "block_distance", "block_lat",
                                                  "block_lon", "block_elevation")])
SIGHT_RAY_DTYPE = np.dtype([("block_index", np.int32), ("min_index", np.int32), ("arrival", np.float64), ("min_clearance", np.float64)])
SIGHT_TARGET_DTYPE = np.dtype([("azimuth_deg", np.float64), ("distance", np.float64), ("height", np.float64)])
assert SIGHT_DTYPE.itemsize == C.sizeof(_abi.Sight) and SIGHT_RAY_DTYPE.itemsize == C.sizeof(_abi.SightRay)
assert SIGHT_TARGET_DTYPE.itemsize == C.sizeof(_abi.SightTarget)


def _sight_target_array(targets):
    """Targets as a contiguous array of SIGHT_TARGET_DTYPE: such an array, or a sequence of (azimuth_deg, distance, height)."""
    if isinstance(targets, np.ndarray) and targets.dtype == SIGHT_TARGET_DTYPE:
        return np.ascontiguousarray(targets.reshape(-1))
    rows = np.asarray(targets, dtype=np.float64).reshape(-1, 3)
    out = np.empty(len(rows), dtype=SIGHT_TARGET_DTYPE)
    out["azimuth_deg"], out["distance"], out["height"] = rows[:, 0], rows[:, 1], rows[:, 2]
    return out


def sight_fan_angles(lo, hi, lib=None):
    """atmrt_sight_fan_angles (host code, no device): the 64 angles of the fan over [lo, hi]."""
    lib = lib or _lib.load()
    out = (C.c_double * 64)()
    rc = lib.atmrt_sight_fan_angles(lo, hi, out)
    if rc != 0:
        raise AtmrtError(rc, "atmrt_sight_fan_angles refused its arguments")
    return np.array(out, dtype=np.float64)


def sight_pick(fails, lib=None):
    """atmrt_sight_pick (host code, no device): k* of a fan whose ray k fails where fails[k] is true."""
    lib = lib or _lib.load()
    f = np.ascontiguousarray(np.asarray(fails).astype(bool), dtype=np.uint8)
    if f.shape != (64,):
        raise ValueError("a fan has 64 rays")
    k = C.c_int32()
    rc = lib.atmrt_sight_pick(f.ctypes.data, C.byref(k))
    if rc != 0:
        raise AtmrtError(rc, "atmrt_sight_pick refused its arguments")
    return k.value


def sight_lines(ctx, targets, fan=(-5.0, 5.0), rounds=3):
    """Solves the targets (sight_targets() makes them; or rows of (azimuth_deg, distance, height)) against the parameters,
    atmosphere and terrain now set on `ctx`: at which elevation angle each appears, or which ridge hides it.  No frame is needed.
    Returns a structured array of SIGHT_DTYPE."""
    t = _sight_target_array(targets)
    out = np.empty(len(t), dtype=SIGHT_DTYPE)
    ctx.check(ctx.lib.atmrt_sight_lines(ctx.handle, t.ctypes.data, len(t), float(fan[0]), float(fan[1]), int(rounds), out.ctypes.data))
    return out


def sight_fan_probe(ctx, target, angles_deg):
    """atmrt_sight_fan_probe: one ray per elevation angle against one target (azimuth_deg, distance, height), by the device functions
    of the solve.  Returns a structured array of SIGHT_RAY_DTYPE."""
    t = _sight_target_array([tuple(target)] if not isinstance(target, np.ndarray) else target)
    pod = _abi.SightTarget(float(t["azimuth_deg"][0]), float(t["distance"][0]), float(t["height"][0]))
    ang = np.ascontiguousarray(angles_deg, dtype=np.float64).reshape(-1)
    rays = np.empty(ang.size, dtype=SIGHT_RAY_DTYPE)
    ctx.check(ctx.lib.atmrt_sight_fan_probe(ctx.handle, C.byref(pod), ang.size, ang.ctypes.data, rays.ctypes.data))
    return rays


def sight_timings(ctx):
    """atmrt_last_sight_timings / atmrt_last_sight_batches of the last sight_lines on `ctx`."""
    out, n = (C.c_double * 3)(), C.c_int32()
    ctx.check(ctx.lib.atmrt_last_sight_timings(ctx.handle, out))
    ctx.check(ctx.lib.atmrt_last_sight_batches(ctx.handle, C.byref(n)))
    return dict(zip(("profile_ms", "solve_ms", "download_ms"), out), batches=n.value)


def _inverse_spherical(lat0, lon0, lat, lon, radius):
    """Azimuth [deg] and great-circle distance [m] from (lat0, lon0) to (lat, lon) on a sphere, closed form."""
    p0, p1, dl = np.radians(lat0), np.radians(lat), np.radians(lon - lon0)
    az = np.degrees(np.arctan2(np.sin(dl) * np.cos(p1), np.cos(p0) * np.sin(p1) - np.sin(p0) * np.cos(p1) * np.cos(dl)))
    a = np.sin((p1 - p0) / 2) ** 2 + np.cos(p0) * np.cos(p1) * np.sin(dl / 2) ** 2
    return az, 2.0 * radius * np.arcsin(np.sqrt(a))


def inverse_geodesic(forward, lat0, lon0, lat, lon, radius=6371000.0, exact=False, tolerance_deg=1e-9, max_corrections=20):
    """(azimuth_deg, distance) arrays that lead from (lat0, lon0) to the points (lat, lon) under the earth model behind
    forward(azimuth_deg, distance) -> (lat, lon).  The closed form of the sphere of `radius` is the answer when `exact`; otherwise it
    seeds a correction: the miss of the forward point in metres north / east, resolved along and across the track where it arrives,
    changes the distance and the azimuth — until the forward point lies within tolerance_deg of the asked one in latitude and in
    longitude, for at most max_corrections corrections, else ValueError."""
    az, dist = _inverse_spherical(lat0, lon0, lat, lon, radius)
    if exact:
        return az, dist
    metres_per_deg = np.pi * radius / 180.0
    for i in range(lat.size):
        back = _inverse_spherical(lat[i], lon[i], lat0, lon0, radius)[0]
        heading = np.radians(back + 180.0)  # of the track where it arrives
        reach = max(radius * np.sin(dist[i] / radius), 1.0)  # metres across the track per radian of azimuth
        for k in range(max_corrections + 1):
            fl, fo = forward(float(az[i]), float(dist[i]))
            dlat, dlon = lat[i] - fl, lon[i] - fo
            if abs(dlat) <= tolerance_deg and abs(dlon) <= tolerance_deg:
                break
            if k == max_corrections:
                raise ValueError(f"({lat[i]}, {lon[i]}) not reached within {tolerance_deg} degrees after {max_corrections} corrections")
            north, east = dlat * metres_per_deg, dlon * metres_per_deg * np.cos(np.radians(lat[i]))
            dist[i] += north * np.cos(heading) + east * np.sin(heading)
            az[i] += np.degrees((east * np.cos(heading) - north * np.sin(heading)) / reach)
    return az, dist


def sight_targets(ctx, lat, lon, height=0.0):
    """The inverse geodesic: targets (SIGHT_TARGET_DTYPE) whose azimuth and distance lead from the observer now set on `ctx` to the
    points (lat, lon) [deg] under the context's earth model.  Closed form on the Spherical models; on every other model the closed
    form is corrected through coords_at_dist on the context (inverse_geodesic)."""
    lat, lon = np.atleast_1d(np.asarray(lat, dtype=np.float64)), np.atleast_1d(np.asarray(lon, dtype=np.float64))
    if lat.shape != lon.shape or lat.ndim != 1:
        raise ValueError("lat and lon must be sequences of one length")
    p = ctx_params(ctx)
    lat0, lon0 = p.position.latitude, p.position.longitude
    spherical = p.earth.kind in (_abi.EARTH_KINDS["SimpleSphere"], _abi.EARTH_KINDS["Spherical"])
    radius = p.earth.radius if p.earth.kind == _abi.EARTH_KINDS["Spherical"] else 6371000.0

    def forward(az, dist):
        fl, fo = coords_at_dist(ctx, lat0, lon0, az, [dist])
        return fl[0], fo[0]

    out = np.empty(lat.size, dtype=SIGHT_TARGET_DTYPE)
    out["azimuth_deg"], out["distance"] = inverse_geodesic(forward, lat0, lon0, lat, lon, radius, exact=spherical)
    out["height"] = np.broadcast_to(np.asarray(height, dtype=np.float64), lat.shape)
    return out


def ctx_params(ctx):
    """The parameters last handed to atmrt_set_params through a Generator on `ctx` (Generator._configure records them)."""
    p = getattr(ctx, "last_params", None)
    if p is None:
        raise AtmrtError(_abi.ERR_STATE, "no parameters have been set on this context")
    return p


# ---- viewshed: the first round of the sight-line rule at every cell of a polar lattice (include/atmrt.h) ---------------------
VIEWSHED_PLANES = (("k_star", np.uint16), ("status", np.uint8), ("hidden", np.float64), ("block_index", np.int32), ("ground", np.float64),
                   ("lat", np.float64), ("lon", np.float64))


class Viewshed:
    """The planes of one viewshed call as numpy arrays [n_az][m] (cell (j, i) at [j, i - 1]; an optional plane that was not asked
    for is None), with d [m + 1] (the lattice), azimuths [n_az], angles [K] (the fan) and height."""

    def __init__(self, **fields):
        self.__dict__.update(fields)

    def planes(self):
        return {k: getattr(self, k) for k, _ in VIEWSHED_PLANES if getattr(self, k) is not None}


def viewshed_fan_angles(lo, hi, fan_rays=64, lib=None):
    """atmrt_viewshed_fan_angles (host code, no device): the fan_rays angles of the fan over [lo, hi]."""
    lib = lib or _lib.load()
    out = np.empty(max(int(fan_rays), 1), dtype=np.float64)
    rc = lib.atmrt_viewshed_fan_angles(lo, hi, int(fan_rays), out.ctypes.data)
    if rc != 0:
        raise AtmrtError(rc, "atmrt_viewshed_fan_angles refused its arguments")
    return out


def viewshed_kernel_shape(fan_rays=64, lib=None):
    """atmrt_debug_viewshed_shape: {'az_per_load', 'step_tile', 'rays_per_lane'} of the scan kernel at fan_rays."""
    lib = lib or _lib.load()
    a, t, r = C.c_int32(), C.c_int32(), C.c_int32()
    lib.atmrt_debug_viewshed_shape(int(fan_rays), C.byref(a), C.byref(t), C.byref(r))
    return dict(az_per_load=a.value, step_tile=t.value, rays_per_lane=r.value)


def viewshed_lattice(step, reach):
    """d_0 = 0, d_i = d_{i-1} + step as far as the first d_m >= reach (the sight lines' lattice) -> d [m + 1]."""
    d, x = [0.0], 0.0
    while not x >= reach:
        x = x + step
        d.append(x)
        if len(d) - 1 > 65535:
            raise ValueError("the reach lies more than 65535 samples away")
    return np.array(d, dtype=np.float64)


def viewshed_azimuths(az_lo_deg, az_step_deg, n_az):
    """az_j = az_lo + (double)j * az_step."""
    return np.float64(az_lo_deg) + np.arange(int(n_az), dtype=np.float64) * np.float64(az_step_deg)


def viewshed(ctx, az_lo_deg, az_step_deg, n_az, reach, height=0.0, fan=(-5.0, 5.0), fan_rays=64, optional=("block_index", "ground", "lat", "lon")):
    """atmrt_viewshed against the parameters, atmosphere and terrain now set on `ctx`: for the n_az azimuths az_lo + j az_step and
    every lattice sample as far as `reach`, whether a point `height` metres above the ground is seen over the fan of fan_rays rays,
    and how many metres are hidden.  No frame is needed.  `optional` names the optional planes to fill.  Returns a Viewshed."""
    spec = _abi.ViewshedSpec(float(az_lo_deg), float(az_step_deg), float(reach), float(height), float(fan[0]), float(fan[1]), int(n_az), int(fan_rays))
    m = C.c_int32()
    ctx.check(ctx.lib.atmrt_viewshed_steps(ctx.handle, float(reach), C.byref(m)))
    m = m.value
    d = viewshed_lattice(ctx_params(ctx).simulation_step, float(reach))
    if d.size != m + 1:
        raise AtmrtError(_abi.ERR_STATE, f"the library's lattice has {m} steps, this module's {d.size - 1}: the parameters on the context are not the ones recorded")
    arrays = {k: np.empty((max(int(n_az), 1), m), dtype=t) if k in ("k_star", "status", "hidden") or k in optional else None for k, t in VIEWSHED_PLANES}
    ctx.check(ctx.lib.atmrt_viewshed(ctx.handle, C.byref(spec), *[None if arrays[k] is None else arrays[k].ctypes.data for k, _ in VIEWSHED_PLANES]))
    return Viewshed(d=d, azimuths=viewshed_azimuths(az_lo_deg, az_step_deg, n_az), angles=viewshed_fan_angles(fan[0], fan[1], fan_rays, ctx.lib),
                    height=float(height), **arrays)


def viewshed_work(ctx):
    """atmrt_last_viewshed_timings / atmrt_last_viewshed_work of the last viewshed on `ctx`."""
    out, n, rebuilt = (C.c_double * 4)(), C.c_int32(), C.c_int32()
    ctx.check(ctx.lib.atmrt_last_viewshed_timings(ctx.handle, out))
    ctx.check(ctx.lib.atmrt_last_viewshed_work(ctx.handle, C.byref(n), C.byref(rebuilt)))
    return dict(zip(("paths_ms", "profiles_ms", "scan_ms", "download_ms"), out), batches=n.value, table_rebuilt=bool(rebuilt.value))


def write_viewshed_npz(path, v):
    """OUT.npz of gen --viewshed: the planes, d, the azimuths, the fan's angles and the height."""
    np.savez_compressed(path, d=v.d, azimuths=v.azimuths, angles=v.angles, height=np.float64(v.height), **v.planes())


# ---- viewshed map: the polar viewshed binned over a latitude / longitude grid on the device (include/atmrt.h) -----------------
VIEWSHED_MAP_PLANES = (("n_samples", np.uint32), ("n_seen", np.uint32), ("min_hidden", np.float64))
VIEWSHED_MAP_RADIUS = 6_371_000.0  # the sphere viewshed_map_grid lays its bounds on


class ViewshedMap:
    """One viewshed map: n_samples, n_seen (uint32) and min_hidden (float64, +inf where no sample takes part), each [n_lat][n_lon] —
    numpy arrays on the host route, the caller's torch tensors on the device route (the counts as int32, the bits of the u32) —
    with the grid and stats (the atmrt_viewshed_map_stats_t of the call, a dict)."""

    def __init__(self, grid, n_samples, n_seen, min_hidden, stats):
        self.grid, self.n_samples, self.n_seen, self.min_hidden, self.stats = grid, n_samples, n_seen, min_hidden, stats


def _vsmap_stats(st):
    return {k: getattr(st, k) for k, _ in _abi.ViewshedMapStats._fields_}


def viewshed_map_tensors(grid, device):
    """The three planes of a map on `grid` as torch tensors on `device` (uninitialised: a call without accumulate overwrites them)."""
    import torch
    shape = (grid.n_lat, grid.n_lon)
    return dict(n_samples=torch.empty(shape, dtype=torch.int32, device=device), n_seen=torch.empty(shape, dtype=torch.int32, device=device),
                min_hidden=torch.empty(shape, dtype=torch.float64, device=device))


def _vsmap_into(grid, into):
    for k, _ in VIEWSHED_MAP_PLANES:
        t = into[k]
        if tuple(t.shape) != (grid.n_lat, grid.n_lon) or not t.is_contiguous() or t.element_size() != (8 if k == "min_hidden" else 4):
            raise ValueError(f"into[{k!r}] must be a contiguous [n_lat][n_lon] tensor of {'float64' if k == 'min_hidden' else 'int32'}")
    return [into[k].data_ptr() for k, _ in VIEWSHED_MAP_PLANES]


def viewshed_map(ctx, grid, az_lo_deg, az_step_deg, n_az, reach, height=0.0, fan=(-5.0, 5.0), fan_rays=64, accumulate=False, into=None):
    """atmrt_viewshed_map against the parameters, atmosphere and terrain now set on `ctx`: the viewshed of the call's lattice (see
    viewshed) binned over `grid` on the device, without its planes ever leaving it.  accumulate adds to a map that is already there:
    `into`, a dict of torch device tensors n_samples, n_seen (int32) and min_hidden (float64) as viewshed_map_tensors makes them —
    the device route, nothing is downloaded — or, on the host route, the arrays of a ViewshedMap passed as `into`.  Returns a ViewshedMap."""
    spec = _abi.ViewshedSpec(float(az_lo_deg), float(az_step_deg), float(reach), float(height), float(fan[0]), float(fan[1]), int(n_az), int(fan_rays))
    st = _abi.ViewshedMapStats()
    if isinstance(into, dict):
        ctx.check(ctx.lib.atmrt_viewshed_map_device(ctx.handle, C.byref(spec), C.byref(grid), int(bool(accumulate)), *_vsmap_into(grid, into), C.byref(st)))
        return ViewshedMap(grid, into["n_samples"], into["n_seen"], into["min_hidden"], _vsmap_stats(st))
    if into is not None:
        arrays = {k: np.ascontiguousarray(getattr(into, k), dtype=t) for k, t in VIEWSHED_MAP_PLANES}
    elif accumulate:
        raise ValueError("accumulate needs the map to add to: pass it as `into`")
    else:
        arrays = {k: np.empty((grid.n_lat, grid.n_lon), dtype=t) for k, t in VIEWSHED_MAP_PLANES}
    ctx.check(ctx.lib.atmrt_viewshed_map(ctx.handle, C.byref(spec), C.byref(grid), int(bool(accumulate)), *[arrays[k].ctypes.data for k, _ in VIEWSHED_MAP_PLANES],
                                         C.byref(st)))
    return ViewshedMap(grid, stats=_vsmap_stats(st), **arrays)


def viewshed_map_planes(ctx, grid, status, hidden, lat, lon, accumulate=False, into=None):
    """atmrt_viewshed_map_planes_device: any samples — torch device tensors status (uint8), hidden, lat, lon (float64) of one size,
    e.g. the planes of atmrt_viewshed_device — binned over `grid` into torch device tensors (`into`, else new ones).  Returns a ViewshedMap."""
    n = status.numel()
    if not (hidden.numel() == lat.numel() == lon.numel() == n) or status.element_size() != 1 or any(t.element_size() != 8 for t in (hidden, lat, lon)):
        raise ValueError("status (uint8), hidden, lat and lon (float64) must hold the same number of samples")
    if not all(t.is_contiguous() for t in (status, hidden, lat, lon)):
        raise ValueError("the sample planes must be contiguous")
    if into is None:
        if accumulate:
            raise ValueError("accumulate needs the map to add to: pass it as `into`")
        into = viewshed_map_tensors(grid, status.device)
    st = _abi.ViewshedMapStats()
    ctx.check(ctx.lib.atmrt_viewshed_map_planes_device(ctx.handle, C.byref(grid), n, status.data_ptr(), hidden.data_ptr(), lat.data_ptr(), lon.data_ptr(),
                                                       int(bool(accumulate)), *_vsmap_into(grid, into), C.byref(st)))
    return ViewshedMap(grid, into["n_samples"], into["n_seen"], into["min_hidden"], _vsmap_stats(st))


def viewshed_map_grid(lat, lon, reach, cell_deg):
    """The grid of cell_deg cells, snapped by snap_grid's rule, that holds every point within `reach` metres of (lat, lon) on the
    sphere of 6,371 km — the cap's extreme latitudes lat +- reach / R, its extreme longitudes lon +- asin(sin(reach / R) / cos(lat)),
    every longitude once the cap holds a pole — with one cell of margin on every side.  There is no antimeridian handling (GeoGrid):
    the longitudes are plain numbers around `lon`.  On other earth models, and for the lattice's last sample where it lies beyond
    `reach`, samples may leave the grid: the map counts them n_outside."""
    delta = float(reach) / VIEWSHED_MAP_RADIUS
    ddeg = np.degrees(delta)
    lat_lo, lat_hi = max(lat - ddeg, -90.0), min(lat + ddeg, 90.0)
    if delta >= np.pi / 2 or abs(lat) + ddeg >= 90.0:
        half = 180.0
    else:
        half = float(np.degrees(np.arcsin(min(1.0, np.sin(delta) / np.cos(np.radians(lat))))))
    return snap_grid((lat_lo - cell_deg, lat_hi + cell_deg, lon - half - cell_deg, lon + half + cell_deg), cell_deg)


def cumulative_viewshed(gen, observers, grid, az_lo_deg, az_step_deg, n_az, reach, height=0.0, fan=(-5.0, 5.0), fan_rays=64):
    """From how many observers each cell of `grid` is seen: for every observer {lat, lon, altitude} (altitude of the kind the
    generator's parameters give) the position is set on gen's context, one fresh map is made on device tensors, and (n_seen > 0) is
    added into observers_seeing with torch — the plumbing; the map is the kernels'.  Returns (observers_seeing int32 — the bits of
    the u32 counts — and the cell-wise minimum min_hidden over the observers, float64), torch tensors [n_lat][n_lon] on the device.
    The generator's own position is set on the context again afterwards."""
    import torch
    ctx = gen.ctx
    dev = torch.device("cuda", ctx.device)
    fresh = viewshed_map_tensors(grid, dev)
    seeing = torch.zeros((grid.n_lat, grid.n_lon), dtype=torch.int32, device=dev)
    min_hidden = torch.full((grid.n_lat, grid.n_lon), float("inf"), dtype=torch.float64, device=dev)
    pos = gen.params.pod.position
    before = (pos.latitude, pos.longitude, pos.altitude)
    try:
        for o in observers:
            pos.latitude, pos.longitude, pos.altitude = float(o["lat"]), float(o["lon"]), float(o["altitude"])
            gen._configure()
            viewshed_map(ctx, grid, az_lo_deg, az_step_deg, n_az, reach, height, fan, fan_rays, into=fresh)
            seeing += (fresh["n_seen"] != 0).to(torch.int32)
            min_hidden = torch.minimum(min_hidden, fresh["min_hidden"])
    finally:
        pos.latitude, pos.longitude, pos.altitude = before
        gen._configure()
    return seeing, min_hidden


def write_viewshed_map_npz(path, grid, planes, stats=None):
    """OUT.npz of gen --viewshed-map: the planes by name (n_samples, n_seen, min_hidden; observers_seeing, min_hidden in the cumulative
    form), the grid's six numbers and, for a single map, the call's stats as stats_<name>."""
    extra = {} if stats is None else {"stats_" + k: np.uint64(v) for k, v in stats.items()}
    np.savez_compressed(path, lat0=np.float64(grid.lat0), lon0=np.float64(grid.lon0), cell_lat=np.float64(grid.cell_lat), cell_lon=np.float64(grid.cell_lon),
                        n_lat=np.uint32(grid.n_lat), n_lon=np.uint32(grid.n_lon), **planes, **extra)


# ---- horizon: per azimuth the bracket of elevation angles between terrain and sky, and the ridge that forms it (include/atmrt.h) ----
HORIZON_DTYPE = np.dtype([("status", np.int32), ("rounds_done", np.int32), ("k_star", np.int32), ("block_index", np.int32)] +
                         [(k, np.float64) for k in ("angle_clear", "angle_blocked", "resolution", "block_distance", "block_lat", "block_lon",
                                                    "block_elevation")])
HORIZON_COLUMNS = ("azimuth_deg", "status", "angle_clear_deg", "angle_blocked_deg", "resolution_deg", "ridge_distance_m", "ridge_lat", "ridge_lon",
                   "ridge_elevation_m")


class Horizon:
    """The records of one horizon call (HORIZON_DTYPE [n_az]) with azimuths [n_az] and angles [K] (the first fan)."""

    def __init__(self, records, azimuths, angles):
        self.records, self.azimuths, self.angles = records, azimuths, angles


def horizon_kernel_shape(fan_rays=64, lib=None):
    """atmrt_debug_horizon_shape: {'az_per_load', 'step_tile', 'rays_per_lane'} of the round-one scan at fan_rays."""
    lib = lib or _lib.load()
    a, t, r = C.c_int32(), C.c_int32(), C.c_int32()
    lib.atmrt_debug_horizon_shape(int(fan_rays), C.byref(a), C.byref(t), C.byref(r))
    return dict(az_per_load=a.value, step_tile=t.value, rays_per_lane=r.value)


def horizon(ctx, az_lo_deg, az_step_deg, n_az, reach, fan=(-5.0, 5.0), fan_rays=64, rounds=3):
    """atmrt_horizon against the parameters, atmosphere and terrain now set on `ctx`: for the n_az azimuths az_lo + j az_step, the
    bracket [angle_blocked, angle_clear] between the highest ray that terrain within `reach` stops and the ray above it — the
    refracted skyline to within `resolution` — and the ridge that stops it.  The first fan has fan_rays rays; every later round
    narrows the bracket 63-fold.  No frame is needed.  Returns a Horizon."""
    spec = _abi.HorizonSpec(float(az_lo_deg), float(az_step_deg), float(reach), float(fan[0]), float(fan[1]), int(n_az), int(fan_rays), int(rounds))
    records = np.empty(max(int(n_az), 1), dtype=HORIZON_DTYPE)
    ctx.check(ctx.lib.atmrt_horizon(ctx.handle, C.byref(spec), records.ctypes.data))
    return Horizon(records, viewshed_azimuths(az_lo_deg, az_step_deg, n_az), viewshed_fan_angles(fan[0], fan[1], fan_rays, ctx.lib))


def horizon_work(ctx):
    """atmrt_last_horizon_timings / atmrt_last_horizon_work of the last horizon on `ctx`."""
    out, n, rebuilt = (C.c_double * 5)(), C.c_int32(), C.c_int32()
    ctx.check(ctx.lib.atmrt_last_horizon_timings(ctx.handle, out))
    ctx.check(ctx.lib.atmrt_last_horizon_work(ctx.handle, C.byref(n), C.byref(rebuilt)))
    return dict(zip(("paths_ms", "profiles_ms", "scan_ms", "refine_ms", "download_ms"), out), batches=n.value, table_rebuilt=bool(rebuilt.value))


def write_horizon_csv(path, h):
    """OUT.csv of gen --horizon: one row per azimuth (HORIZON_COLUMNS); numbers as repr() writes them, NaN as an empty field."""
    import csv

    def num(v):
        return "" if np.isnan(v) else repr(float(v))

    with open(path, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(HORIZON_COLUMNS)
        for az, r in zip(h.azimuths, h.records):
            w.writerow([repr(float(az)), _abi.HORIZON_STATUS[int(r["status"])], num(r["angle_clear"]), num(r["angle_blocked"]), num(r["resolution"]),
                        num(r["block_distance"]), num(r["block_lat"]), num(r["block_lon"]), num(r["block_elevation"])])


# ---- the sight-line tables of the command line (gen --sight-lines FILE.csv) --------------------------------------------------
SIGHT_COLUMNS = ("name", "azimuth_deg", "distance_m", "status", "angle_deg", "hidden_m", "ground_m", "resolution_deg", "block_distance_m",
                 "block_lat", "block_lon", "block_elevation_m", "x", "y")


def read_sight_csv(path):
    """name,lat,lon[,height] rows (header optional, as read_landmarks_csv reads it) -> (names, lat, lon, height)."""
    import csv
    names, lat, lon = read_landmarks_csv(path)
    height = []
    with open(path, newline="") as f:
        rows = [r for r in csv.reader(f) if r and "".join(r).strip()]
    rows = rows[len(rows) - len(names):]  # the header, if any, is the first row
    for i, row in enumerate(rows):
        try:
            height.append(float(row[3]) if len(row) > 3 and row[3].strip() else 0.0)
        except ValueError:
            raise ValueError(f"{path}: target {i + 1}: height must be a number")
    return names, lat, lon, np.array(height, dtype=np.float64)


def fast_pixel_of(params_pod, azimuth_deg, angle_deg):
    """The Fast generator's pixel (x, y) that a ray of this azimuth and elevation angle falls in for the configured frame: the
    inverse of get_ray_dir / get_ray_elev (fast.rs:111-125), the pixel whose own direction and angle are nearest; None outside."""
    w, h = params_pod.width, params_pod.height
    fov, direction, tilt = params_pod.frame.fov, params_pod.frame.direction, params_pod.frame.tilt
    if not (np.isfinite(azimuth_deg) and np.isfinite(angle_deg)):
        return None
    rel = (azimuth_deg - direction + 180.0) % 360.0 - 180.0
    # dir(x) = direction + (x - w // 2) * fov / w; elev(y) = tilt - (y - h // 2) * fov / w: the nearest pixel centre
    x = int(np.floor(rel * w / fov + w // 2 + 0.5))
    y = int(np.floor(h // 2 - (angle_deg - tilt) * w / fov + 0.5))
    return (x, y) if 0 <= x < w and 0 <= y < h else None


def write_sight_csv(f, names, targets, sights, params_pod):
    """The solved table, SIGHT_COLUMNS, to the open text file f; floats in Python's repr, fields that do not apply left empty."""
    import csv
    w = csv.writer(f, lineterminator="\n")
    w.writerow(SIGHT_COLUMNS)

    def num(v):
        return "" if np.isnan(v) else repr(float(v))

    for name, t, s in zip(names, targets, sights):
        px = fast_pixel_of(params_pod, float(t["azimuth_deg"]), float(s["angle"]))
        w.writerow([name, repr(float(t["azimuth_deg"])), repr(float(t["distance"])), _abi.SIGHT_STATUS[int(s["status"])], num(s["angle"]),
                    num(s["hidden"]), num(s["ground"]), num(s["resolution"]), num(s["block_distance"]), num(s["block_lat"]),
                    num(s["block_lon"]), num(s["block_elevation"]), "" if px is None else px[0], "" if px is None else px[1]])


# ---- integrator / sampler harnesses (ray_path.rs, atm_printer.rs, elev_profile.rs) -------------
def ray_paths(ctx, h0, angles_deg, step, n_steps, straight=False):
    ang = np.ascontiguousarray(angles_deg, dtype=np.float64)
    x = np.zeros((ang.size, n_steps + 1))
    h = np.zeros((ang.size, n_steps + 1))
    ctx.check(ctx.lib.atmrt_ray_paths(ctx.handle, h0, ang.size, ang.ctypes.data, int(straight), step, n_steps,
                                      x.ctypes.data, h.ctypes.data))
    return x, h


def atmosphere_sample(ctx, altitudes):
    alt = np.ascontiguousarray(altitudes, dtype=np.float64)
    outs = [np.zeros_like(alt) for _ in range(4)]
    ctx.check(ctx.lib.atmrt_atmosphere_sample(ctx.handle, alt.size, alt.ctypes.data, *[o.ctypes.data for o in outs]))
    return dict(zip(("temperature", "pressure", "n", "dn_dh"), outs))


def coords_at_dist(ctx, lat0, lon0, dir_deg, dists):
    d = np.ascontiguousarray(dists, dtype=np.float64)
    lat, lon = np.zeros_like(d), np.zeros_like(d)
    ctx.check(ctx.lib.atmrt_coords_at_dist(ctx.handle, lat0, lon0, dir_deg, d.size, d.ctypes.data, lat.ctypes.data,
                                           lon.ctypes.data))
    return lat, lon
