"""Python host mirror of the integrator/renderer surface on top of the C ABI (include/prgpu.h).

`RenderContext` follows the call sequence of the reference host (src/client/main.cpp:172-257:
create -> start -> wait -> save) and the `direct` integrator contract (IIntegrator.h:24-37):
``start()`` queues every iteration of every owned tile on the GPU, ``waitForFinish()`` synchronises,
``statistics()`` returns the RenderStatistics counters and ``output()`` the XYZ / sample-count planes.
All compute goes through ``libprgpu.so``; there is no CPU path here.
"""
import collections
import ctypes as C
import os

import numpy as np

from . import _cabi as abi


def _f32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _u32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def check_ray_tensors(org, direction, tmin, tmax, device, last="tmax"):
    """The argument checks of RenderContext.traceRaysDevice / traceShadowRaysDevice (last="distance"); needs no device.  `org` and
    `direction`: float32 CUDA tensors of shape (n, 3); `tmin` and the last argument: float32 CUDA tensors of shape (n,), or Python
    floats (the wrapper expands those on the device).  Every tensor contiguous and on device index `device`.  Returns n; anything
    else raises ValueError naming the argument."""
    import torch

    def tensor(name, a, n, tail):
        """float32, shape (n,) + tail (n None: any length), contiguous"""
        want = "(n%s)" % "".join(", %d" % k for k in tail) if tail else "(n,)"
        if not isinstance(a, torch.Tensor):
            raise ValueError("%s: a torch tensor is expected, not %s" % (name, type(a).__name__))
        if a.dtype != torch.float32:
            raise ValueError("%s: float32 is expected, not %s" % (name, a.dtype))
        if a.dim() != 1 + len(tail) or tuple(a.shape[1:]) != tail:
            raise ValueError("%s: shape %s is expected, not %s" % (name, want, tuple(a.shape)))
        if n is not None and a.shape[0] != n:
            raise ValueError("%s: %d rays are expected as in org, not %d" % (name, n, a.shape[0]))
        if not a.is_contiguous():
            raise ValueError("%s: the tensor is not contiguous" % name)

    tensor("org", org, None, (3,))
    n = int(org.shape[0])
    if n >= 1 << 32:
        raise ValueError("org: more than 2^32 - 1 rays")
    tensor("direction", direction, n, (3,))
    given = [("org", org), ("direction", direction)]
    for name, a in (("tmin", tmin), (last, tmax)):
        if isinstance(a, (int, float)) and not isinstance(a, bool):
            continue
        tensor(name, a, n, ())
        given.append((name, a))
    for name, a in given:   # where the tensors live comes last, so that a test without a device reaches every check above
        if not a.is_cuda:
            raise ValueError("%s: the tensor is on %s, not on the GPU (traceRays / traceShadowRays take host arrays)" % (name, a.device))
        if a.device.index != int(device):
            raise ValueError("%s: the tensor is on %s, the scene on device %d" % (name, a.device, int(device)))
    return n


RayHits = collections.namedtuple("RayHits", "entity prim u v t")
RayHitsCounted = collections.namedtuple("RayHitsCounted", RayHits._fields + ("invalid",))
_GEOMETRY = ("position", "normal", "tangent", "bitangent", "uv", "material", "emission")
RayGeometry = collections.namedtuple("RayGeometry", RayHits._fields + _GEOMETRY)
RayGeometryCounted = collections.namedtuple("RayGeometryCounted", RayGeometry._fields + ("invalid",))
ShadowRaysCounted = collections.namedtuple("ShadowRaysCounted", "occluded invalid")


class RenderContext:
    """One scene resident on one GPU (mirrors renderer/RenderContext.h + Scene + `direct` integrator)."""

    def __init__(self, scene, device=0):
        self.lib = abi.load()
        self.scene = scene
        self._h = C.c_void_p()
        abi.check(self.lib.prgpu_scene_create(C.byref(scene.desc), int(device), C.byref(self._h)))
        self.width, self.height = scene.width, scene.height
        self.device = int(device)
        self._stream = None      # the stream handle setStream was given last (None: the scene's own)
        self._lent_to = None     # the torch stream the scene runs on since a device ray batch (None: it is on its own)
        self.iterations_done = 0
        self.ao_sample_count = 0
        if getattr(scene, "integrator", abi.INTEGRATOR_DIRECT) == abi.INTEGRATOR_AO:   # (integrator :type 'ao') / SceneBuilder.ambient_occlusion
            self.enableAmbientOcclusion(scene.ao_sample_count)
        self.vf_mode = None
        if getattr(scene, "integrator", abi.INTEGRATOR_DIRECT) == abi.INTEGRATOR_VF:   # (integrator :type 'vf') / SceneBuilder.visual_feedback
            self.enableVisualFeedback(scene.vf_mode, scene.vf_weighting)

    def close(self):
        if self._h:
            self.lib.prgpu_scene_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- configuration ---------------------------------------------------------------------------------
    def setTiles(self, tiles):
        """tiles: iterable of (x0, y0, x1, y1); empty -> whole film (RenderTileMap / --itx --ity)."""
        tiles = list(tiles)
        arr = (abi.Tile * max(1, len(tiles)))(*[abi.Tile(*t) for t in tiles])
        abi.check(self.lib.prgpu_set_tiles(self._h, arr, len(tiles)))

    def setStream(self, stream_handle):
        abi.check(self.lib.prgpu_set_stream(self._h, C.c_void_p(stream_handle)))
        self._stream, self._lent_to = stream_handle, None

    def _stream_home(self):
        """After traceRaysDevice / traceShadowRaysDevice the scene is still on torch's stream: put it back on the one it had."""
        if self._lent_to is not None:
            abi.check(self.lib.prgpu_set_stream(self._h, C.c_void_p(self._stream)))
            self._lent_to = None

    def bindFramebuffer(self, xyz_ptr, samples_ptr, feedback_ptr=None):
        abi.check(self.lib.prgpu_bind_framebuffer(self._h, C.c_void_p(xyz_ptr), C.c_void_p(samples_ptr),
                                                  C.c_void_p(feedback_ptr) if feedback_ptr else None))

    def reduce(self, comm, root=0):
        """Sum every rank's frame into planes the library keeps on `root` (RCCL over xGMI); asynchronous on the scene's stream.  The
        rank's own planes -- and a framebuffer bound with bindFramebuffer -- keep the rank's OWN pixels: on the root output() /
        outputAOV() / ... read the sums until the next render call, and reducedPlanes() hands out their device pointers."""
        self._stream_home()
        abi.check(self.lib.prgpu_reduce(self._h, comm._h, int(root)))

    def reducedPlanes(self):
        """Device pointers (xyz, samples, feedback) of the root-side sums of the last reduce, or None when the rank's own planes are the frame."""
        x, s, f = C.c_void_p(), C.c_void_p(), C.c_void_p()
        rc = self.lib.prgpu_reduced_planes(self._h, C.byref(x), C.byref(s), C.byref(f))
        if rc < 0:
            abi.check(rc)
        return (x.value, s.value, f.value) if rc == 1 else None

    def pipelineInfo(self):
        """How the persistent pipeline runs this scene (prgpu_pipeline_info): scheduling facts only."""
        info = abi.PipelineInfo()
        abi.check(self.lib.prgpu_pipeline_info_get(self._h, C.byref(info)))
        out = {f: getattr(info, f) for f, _ in info._fields_}
        out["kernel"] = {0: "none", 1: "throughput", 2: "latency"}.get(out["kernel"], str(out["kernel"]))
        return out

    def setInstrumentation(self, on):
        abi.check(self.lib.prgpu_set_instrumentation(self._h, 1 if on else 0))

    def setTiming(self, on):
        abi.check(self.lib.prgpu_set_timing(self._h, 1 if on else 0))

    # -- rendering ----------------------------------------------------------------------------------------
    def render(self, iterations):
        """Render the next `iterations` iterations (one camera sample per owned pixel each)."""
        self._stream_home()
        b = self.iterations_done
        abi.check(self.lib.prgpu_render(self._h, b, b + int(iterations)))
        self.iterations_done = b + int(iterations)

    def start(self):
        """RenderContext::start: queue all spp iterations."""
        self.render(self.scene.spp - self.iterations_done)

    def waitForFinish(self):
        self._stream_home()
        abi.check(self.lib.prgpu_sync(self._h))

    def statistics(self):
        out = (C.c_uint64 * abi.STAT_COUNT)()
        abi.check(self.lib.prgpu_stats(self._h, out))
        return {n: int(out[i]) for i, n in enumerate(abi.STAT_NAMES)}

    def traceCounters(self):
        tc = abi.TraceCounters()
        abi.check(self.lib.prgpu_trace_counters_get(self._h, C.byref(tc)))
        return {f: int(getattr(tc, f)) for f, _ in tc._fields_}

    def kernelTime(self, family):
        ms, n = C.c_double(), C.c_uint64()
        abi.check(self.lib.prgpu_kernel_time_ms(self._h, family.encode(), C.byref(ms), C.byref(n)))
        return ms.value, int(n.value)

    def output(self):
        """(xyz[H,W,3] float32, samples[H,W] uint32, feedback[H,W] uint32) copied to the host."""
        n = self.width * self.height
        xyz = np.empty(n * 3, dtype=np.float32)
        smp = np.empty(n, dtype=np.uint32)
        fb = np.empty(n, dtype=np.uint32)
        abi.check(self.lib.prgpu_download(self._h, _f32p(xyz), _u32p(smp), _u32p(fb)))
        return xyz.reshape(self.height, self.width, 3), smp.reshape(self.height, self.width), fb.reshape(self.height, self.width)

    def enableAOVs(self, names):
        """Shading-point AOVs (LocalFrameOutputDevice::commitShadingPoints): enable before the first iteration."""
        mask = 0
        for n in names:
            mask |= 1 << abi.AOV_NAMES.index(n)
        abi.check(self.lib.prgpu_enable_aovs(self._h, mask))

    def enableVariance(self):
        """AOV_OnlineMean / AOV_OnlineVariance (Welford per pixel and iteration); enable before the first iteration."""
        abi.check(self.lib.prgpu_enable_variance(self._h))

    def variance(self):
        n = self.width * self.height * 3
        mean, var = np.empty(n, np.float32), np.empty(n, np.float32)
        abi.check(self.lib.prgpu_download_variance(self._h, _f32p(mean), _f32p(var)))
        return mean.reshape(self.height, self.width, 3), var.reshape(self.height, self.width, 3)

    def enableLPE(self, expressions):
        """Light path expressions (LightPathExpression.h): one extra spectral plane per expression; enable before the first iteration."""
        arr = (C.c_char_p * max(1, len(expressions)))(*[e.encode() for e in expressions])
        abi.check(self.lib.prgpu_enable_lpe(self._h, len(expressions), arr))

    def lpe(self, index):
        out = np.empty(self.width * self.height * 3, dtype=np.float32)
        abi.check(self.lib.prgpu_download_lpe(self._h, int(index), _f32p(out)))
        return out.reshape(self.height, self.width, 3)

    def enableAmbientOcclusion(self, sample_count):
        """Render with the ambient occlusion integrator (ambientocclusion.cpp:29-74) instead of `direct`: `sample_count` occlusion rays
        per camera sample that hits a surface; enable before the first iteration."""
        abi.check(self.lib.prgpu_enable_ambient_occlusion(self._h, int(sample_count)))
        self.ao_sample_count = int(sample_count)

    def enableVisualFeedback(self, mode, weighting=True):
        """Render with the visual feedback integrator (visualfeedback.cpp:108-250) instead of `direct`: `mode` is a PRGPU_VF_* number or
        its name (abi.VF_MODE_NAMES), `weighting` multiplies every mode but `ndotv` by |N.V|; enable before the first iteration."""
        if isinstance(mode, str):
            mode = abi.VF_MODES[mode.lower()]
        abi.check(self.lib.prgpu_enable_visual_feedback(self._h, int(mode), 1 if weighting else 0))
        self.vf_mode, self.vf_weighting = int(mode), bool(weighting)

    def aoCounts(self):
        """Occluded rays per pixel over all iterations so far, uint32 [H, W]."""
        out = np.empty(self.width * self.height, dtype=np.uint32)
        abi.check(self.lib.prgpu_download_ao_counts(self._h, _u32p(out)))
        return out.reshape(self.height, self.width)

    def aoSamples(self):
        """The occlusion rays of the LAST iteration (instrumentation must be on): (state uint64 [H, W] -- the pixel's generator before
        its first occlusion draw, 0 where the camera ray missed --, origin float32 [H, W, N, 3], direction float32 [H, W, N, 3],
        occluded bool [H, W, N])."""
        n, k = self.width * self.height, self.ao_sample_count
        state = np.empty(n, dtype=np.uint64)
        org, direction = np.empty(n * k * 3, dtype=np.float32), np.empty(n * k * 3, dtype=np.float32)
        occ = np.empty(n * k, dtype=np.uint8)
        abi.check(self.lib.prgpu_download_ao_samples(self._h, state.ctypes.data_as(C.POINTER(C.c_uint64)), _f32p(org), _f32p(direction),
                                                     occ.ctypes.data_as(C.POINTER(C.c_uint8))))
        shape = (self.height, self.width, k)
        return state.reshape(self.height, self.width), org.reshape(shape + (3,)), direction.reshape(shape + (3,)), occ.reshape(shape).astype(bool)

    def pathCost(self):
        """Path vertices traced per pixel so far (persistent pipeline; scheduling statistic)."""
        out = np.empty(self.width * self.height, dtype=np.uint32)
        abi.check(self.lib.prgpu_path_cost(self._h, _u32p(out)))
        return out.reshape(self.height, self.width)

    def enableOutputs(self, prc_scene):
        """Allocate the planes the scene's (output ...) blocks ask for (OutputSpecification::setup)."""
        ch, n = prc_scene.outputs()
        if n:
            abi.check(self.lib.prgpu_outputs_enable(self._h, ch, n))

    def saveOutputs(self, prc_scene, directory, suffix=""):
        """OutputSpecification::save: one EXR per (output :name ...) block, named <name><suffix>.exr; returns the paths."""
        ch, n = prc_scene.outputs()
        paths = []
        k = 0
        while True:
            name = self.lib.prgpu_prc_output_name(prc_scene._h, k)
            if name is None:
                break
            path = os.path.join(directory, name.decode() + suffix + ".exr")
            abi.check(self.lib.prgpu_outputs_save(self._h, ch, n, k, os.fsencode(path)))
            paths.append(path)
            k += 1
        return paths

    def aov(self, name):
        k = abi.AOV_NAMES.index(name)
        ch = self.lib.prgpu_aov_channels(k)
        out = np.empty(self.width * self.height * ch, dtype=np.float32)
        abi.check(self.lib.prgpu_download_aov(self._h, k, _f32p(out)))
        return out.reshape(self.height, self.width, ch) if ch > 1 else out.reshape(self.height, self.width)

    def primaryHits(self):
        n = self.width * self.height
        e = np.empty(n, dtype=np.uint32)
        p = np.empty(n, dtype=np.uint32)
        abi.check(self.lib.prgpu_download_primary_hits(self._h, _u32p(e), _u32p(p)))
        return e.reshape(self.height, self.width), p.reshape(self.height, self.width)

    # -- IArchive surface ------------------------------------------------------------------------------------
    def traceRays(self, org, direction, tmin, tmax):
        org = np.ascontiguousarray(org, dtype=np.float32).reshape(-1, 3)
        direction = np.ascontiguousarray(direction, dtype=np.float32).reshape(-1, 3)
        n = len(org)
        tmin = np.ascontiguousarray(np.broadcast_to(np.asarray(tmin, dtype=np.float32), (n,)))
        tmax = np.ascontiguousarray(np.broadcast_to(np.asarray(tmax, dtype=np.float32), (n,)))
        ent, prim = np.empty(n, np.uint32), np.empty(n, np.uint32)
        u, v, t = np.empty(n, np.float32), np.empty(n, np.float32), np.empty(n, np.float32)
        self._stream_home()
        abi.check(self.lib.prgpu_trace_closest(self._h, n, _f32p(org), _f32p(direction), _f32p(tmin), _f32p(tmax),
                                               _u32p(ent), _u32p(prim), _f32p(u), _f32p(v), _f32p(t)))
        return ent, prim, u, v, t

    def traceShadowRays(self, org, direction, tmin, distance):
        org = np.ascontiguousarray(org, dtype=np.float32).reshape(-1, 3)
        direction = np.ascontiguousarray(direction, dtype=np.float32).reshape(-1, 3)
        n = len(org)
        tmin = np.ascontiguousarray(np.broadcast_to(np.asarray(tmin, dtype=np.float32), (n,)))
        distance = np.ascontiguousarray(np.broadcast_to(np.asarray(distance, dtype=np.float32), (n,)))
        occ = np.empty(n, np.uint8)
        self._stream_home()
        abi.check(self.lib.prgpu_trace_any(self._h, n, _f32p(org), _f32p(direction), _f32p(tmin), _f32p(distance),
                                           occ.ctypes.data_as(C.POINTER(C.c_uint8))))
        return occ.astype(bool)

    # -- the same service on tensors that live on the GPU --------------------------------------------------------
    def reserveRays(self, n):
        """Size the ray service's scratch for device batches of up to `n` rays, so that none of them allocates."""
        abi.check(self.lib.prgpu_ray_service_reserve(self._h, int(n)))

    def _on_torch_stream(self):
        """Order the scene with torch: it runs on torch's current stream from here on, behind the work that made the rays and ahead of
        the work that reads the answers.  prgpu_sync first: a render in flight on the scene's stream has finished (and a device-side
        error of it is reported here).  The scene STAYS on that stream until the next call that is not a device ray batch puts it back
        (_stream_home): prgpu_set_stream waits for the stream it leaves, so putting it back at once would wait for the launch.  Batch
        after batch on one torch stream neither waits nor switches."""
        import torch
        handle = torch.cuda.current_stream(self.device).cuda_stream or 1   # 1: hipStreamLegacy, the null stream's own handle (0 would mean "the scene's own stream")
        if self._lent_to != handle:
            abi.check(self.lib.prgpu_sync(self._h))
            abi.check(self.lib.prgpu_set_stream(self._h, C.c_void_p(handle)))
            self._lent_to = handle

    @staticmethod
    def _per_ray(a, n, like):
        import torch
        return a if isinstance(a, torch.Tensor) else torch.full((n,), float(a), dtype=torch.float32, device=like.device)

    def traceRaysDevice(self, org, direction, tmin, tmax, geometry=False, count_invalid=False):
        """traceRays on CUDA tensors, where they are (check_ray_tensors states what is accepted): enqueued on torch's current stream, no
        copy and no synchronisation -- the answers are tensors this call allocates, to be read by later work on that stream.
        Returns a named tuple (entity, prim, u, v, t), with geometry=True followed by (position [n, 3], normal, tangent, bitangent,
        uv [n, 2], material, emission) -- the hit's GeometryPoint, bit for bit what a render adds to its AOV planes for the same ray --
        and with count_invalid=True by `invalid`, a one-element int32 tensor: the rays with a negative or NaN tmin, which are answered
        as misses (traceRays refuses such a batch).  Ids are int32 tensors that hold the uint32 bits: a miss (PRGPU_INVALID_ID) reads -1.
        On a miss u = v = 0, t = tmax, the geometry is 0 and its ids are -1."""
        import torch
        n = check_ray_tensors(org, direction, tmin, tmax, self.device)
        with torch.cuda.device(self.device):
            tmin, tmax = self._per_ray(tmin, n, org), self._per_ray(tmax, n, org)
            f32, i32 = dict(dtype=torch.float32, device=org.device), dict(dtype=torch.int32, device=org.device)
            out = [torch.empty(n, **i32), torch.empty(n, **i32), torch.empty(n, **f32), torch.empty(n, **f32), torch.empty(n, **f32)]
            if geometry:
                out += [torch.empty((n, 3), **f32) for _ in range(4)] + [torch.empty((n, 2), **f32), torch.empty(n, **i32), torch.empty(n, **i32)]
            invalid = torch.zeros(1, **i32) if count_invalid else None
            rays = abi.Rays(n, org.data_ptr(), direction.data_ptr(), tmin.data_ptr(), tmax.data_ptr())
            hits = abi.Hits(*[a.data_ptr() for a in out])   # (the fields of prgpu_hits in order; without geometry the rest stay NULL)
            hits.invalid = invalid.data_ptr() if count_invalid else None
            if n:
                self._on_torch_stream()
                abi.check(self.lib.prgpu_trace_closest_device(self._h, C.byref(rays), C.byref(hits)))
        kind = (RayGeometryCounted if count_invalid else RayGeometry) if geometry else (RayHitsCounted if count_invalid else RayHits)
        return kind(*(out + ([invalid] if count_invalid else [])))

    def traceShadowRaysDevice(self, org, direction, tmin, distance, count_invalid=False):
        """traceShadowRays on CUDA tensors, enqueued on torch's current stream as traceRaysDevice is: a bool tensor `occluded` -- anything
        in [tmin, distance - 0.001] --, or with count_invalid=True the named tuple (occluded, invalid): rays with a negative or NaN tmin
        are not occluded and counted."""
        import torch
        n = check_ray_tensors(org, direction, tmin, distance, self.device, last="distance")
        with torch.cuda.device(self.device):
            tmin, distance = self._per_ray(tmin, n, org), self._per_ray(distance, n, org)
            occluded = torch.empty(n, dtype=torch.bool, device=org.device)   # one byte each: the kernel writes 0 or 1
            invalid = torch.zeros(1, dtype=torch.int32, device=org.device) if count_invalid else None
            rays = abi.Rays(n, org.data_ptr(), direction.data_ptr(), tmin.data_ptr(), distance.data_ptr())
            if n:
                self._on_torch_stream()
                abi.check(self.lib.prgpu_trace_any_device(self._h, C.byref(rays), C.c_void_p(occluded.data_ptr()),
                                                          C.c_void_p(invalid.data_ptr()) if count_invalid else None))
        return ShadowRaysCounted(occluded, invalid) if count_invalid else occluded


class Communicator:
    """prgpu_comm: the ranks of a tile-parallel render (one per GPU).  `exchange(bytes or None) -> bytes` ships rank 0's unique id
    to every rank -- the host's transport (bench.py: a torch.distributed broadcast; a C++ host: MPI, a socket, a file)."""

    def __init__(self, n_ranks, rank, device=0, exchange=None):
        self.lib = abi.load()
        self._h = C.c_void_p()
        ident = None
        if n_ranks > 1 or os.environ.get("PRGPU_COMM_FORCE_RCCL", "0") not in ("", "0"):
            if n_ranks > 1 and exchange is None:
                raise ValueError("Communicator: n_ranks > 1 needs an `exchange` callable that ships rank 0's %d-byte id to every rank" % abi.COMM_ID_BYTES)
            raw, err = None, None
            if rank == 0:
                buf = (C.c_uint8 * abi.COMM_ID_BYTES)()
                try:
                    abi.check(self.lib.prgpu_comm_unique_id(buf))
                    raw = bytes(buf)
                except Exception as e:  # noqa: BLE001 -- the other ranks are waiting in the exchange: send them a sentinel first
                    err = e
            raw = exchange(raw) if exchange is not None else raw
            if err is not None:
                raise err
            if not isinstance(raw, (bytes, bytearray)) or len(raw) != abi.COMM_ID_BYTES:
                raise ValueError("Communicator: the exchange delivered %r instead of rank 0's %d-byte id (rank 0 could not create one?)"
                                 % (type(raw).__name__ if raw is not None else None, abi.COMM_ID_BYTES))
            ident = (C.c_uint8 * abi.COMM_ID_BYTES).from_buffer_copy(raw)
        abi.check(self.lib.prgpu_comm_create(ident, int(n_ranks), int(rank), int(device), C.byref(self._h)))

    @property
    def size(self):
        return self.lib.prgpu_comm_size(self._h)

    def query(self):
        """(ranks, rank) as the RCCL communicator itself reports them (ncclCommCount / ncclCommUserRank); (0, -1) without RCCL."""
        n, r = C.c_int(), C.c_int()
        abi.check(self.lib.prgpu_comm_query(self._h, C.byref(n), C.byref(r)))
        return int(n.value), int(r.value)

    def close(self):
        if self._h:
            self.lib.prgpu_comm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def rccl_available():
    """True if this process can reach RCCL through the library (dlopen + ncclGetUniqueId): a rank-symmetric probe to run -- and agree
    on across the ranks -- BEFORE the first call in which one rank could fail while its peers block (id broadcast, ncclCommInitRank)."""
    buf = (C.c_uint8 * abi.COMM_ID_BYTES)()
    return abi.load().prgpu_comm_unique_id(buf) == 0


def mix_leaves(desc, material):
    """The tree below `material` as the device reads it (prgpu_mix_leaves; needs no device): {"leaves": [(material, weight coefficient,
    pdf coefficient), ...] in evaluation order, "delta_only": bool, "symbol_leaf": index into leaves or None, "flag_leaf": likewise}.
    `desc`: a scene description, or a scene object that holds one (`.desc`).  A plain material gives one leaf with (1, 1)."""
    d = getattr(desc, "desc", desc)
    out = (abi.MixLeaf * abi.MIX_MAX_LEAVES)()
    n, delta, sym, flag = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    abi.check(abi.load().prgpu_mix_leaves(C.byref(d), int(material), out, C.byref(n), C.byref(delta), C.byref(sym), C.byref(flag)))

    def index(v):
        return None if v.value == abi.INVALID_ID else int(v.value)
    return {"leaves": [(int(l.material), np.float32(l.weight), np.float32(l.pdf)) for l in out[:n.value]], "delta_only": bool(delta.value),
            "symbol_leaf": index(sym), "flag_leaf": index(flag)}


def write_exr(path, channels):
    """channels: dict name -> float32 array [H, W]; written by the library's EXR writer (uncompressed scanline, float)."""
    lib = abi.load()
    names = sorted(channels)
    arrs = [np.ascontiguousarray(channels[n], dtype=np.float32) for n in names]
    h, w = arrs[0].shape
    c_names = (C.c_char_p * len(names))(*[n.encode() for n in names])
    c_planes = (C.POINTER(C.c_float) * len(names))(*[_f32p(a) for a in arrs])
    strides = (C.c_uint32 * len(names))(*([1] * len(names)))
    abi.check(lib.prgpu_write_exr(os.fsencode(path), w, h, len(names), c_names, c_planes, strides))


def tonemap(xyz, mode=abi.TONE_SRGB, scale=1.0, weight=None):
    """ToneMapper::map through the library (prgpu_tonemap): xyz [..., 3] float32 -> rgb of the same shape."""
    lib = abi.load()
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    rgb = np.zeros_like(xyz)
    w = None if weight is None else np.ascontiguousarray(weight, dtype=np.float32)
    abi.check(lib.prgpu_tonemap(int(mode), float(scale), _f32p(xyz), None if w is None else _f32p(w), _f32p(rgb), 3, xyz.size // 3))
    return rgb


def xyz_to_srgb_linear(xyz):
    """RGBConverter::fromXYZ (spectral/RGBConverter.cpp:15-24): XYZ -> linear sRGB, clamped at 0."""
    return tonemap(xyz, abi.TONE_SRGB)


def image_compare(image, reference, crop=None):
    """prcmp statistics (src/tools/imgcmp/main.cpp) of one channel: `image`, `reference` float32 [H, W] (any stride-1 view of a plane).
    Returns the dict of the reference's PerChannelStats fields."""
    lib = abi.load()
    a = np.ascontiguousarray(image, dtype=np.float32)
    b = np.ascontiguousarray(reference, dtype=np.float32)
    assert a.shape == b.shape and a.ndim == 2, "two planes of the same shape"
    st = abi.ImageStats()
    c = None if crop is None else (C.c_uint32 * 4)(*[int(v) for v in crop])
    abi.check(lib.prgpu_image_compare(_f32p(a), 1, _f32p(b), 1, a.shape[1], a.shape[0], c, C.byref(st)))
    return st


def image_stats_merge(stats):
    """mergeStats over several channels (the "Global" block of prcmp)."""
    lib = abi.load()
    g = abi.ImageStats()
    for st in stats:
        lib.prgpu_image_stats_merge(C.byref(g), C.byref(st))
    return g


def image_stats_report(st):
    """The lines prcmp prints for one PerChannelStats (printStat, main.cpp:198-237), as (label, value) pairs."""
    f = np.float32
    with np.errstate(all="ignore"):
        var = f(st.mean_sqr) - f(st.mean) * f(st.mean)
        var_ref = f(st.mean_sqr_ref) - f(st.mean_ref) * f(st.mean_ref)
        var_diff = f(st.mse) - f(st.mean_diff) * f(st.mean_diff)
        psnr = f(st.max_ref) * f(st.max_ref) / f(st.mse)
        snr, snr_ref, snr_diff = f(st.mean) / np.sqrt(var), f(st.mean_ref) / np.sqrt(var_ref), f(st.mean_diff) / np.sqrt(var_diff)
        snt = (f(st.mean) - f(st.mean_ref)) / (np.sqrt(var) - np.sqrt(var_ref))
        db = lambda v: 10 * np.log10(v)  # noqa: E731
        return [("Min", st.min), ("Max", st.max), ("Mean", st.mean), ("MeanSqr", st.mean_sqr), ("MinRef", st.min_ref), ("MaxRef", st.max_ref),
                ("MeanRef", st.mean_ref), ("MeanSqrRef", st.mean_sqr_ref), ("MinDiff", st.min_diff), ("MaxDiff", st.max_diff),
                ("MeanDiff", st.mean_diff), ("MSE", st.mse), ("RMSE", float(np.sqrt(f(st.mse)))), ("MAE", st.mean_diff),
                ("MAPE", "%g %%" % (st.mape * 100)), ("PSNR", "%g [%g dB]" % (psnr, db(psnr))), ("SNR", "%g [%g dB]" % (snr, db(snr))),
                ("SNRRef", "%g [%g dB]" % (snr_ref, db(snr_ref))), ("SNRDiff", "%g [%g dB]" % (snr_diff, db(snr_diff))), ("SNT", float(snt)),
                ("Variance", float(var)), ("VarianceRef", float(var_ref)), ("VarianceDiff", float(var_diff)), ("StdDev", float(np.sqrt(var))),
                ("StdDevRef", float(np.sqrt(var_ref))), ("StdDevDiff", float(np.sqrt(var_diff)))]


def lpe_match(expression, symbols):
    """LightPathExpression::match on explicit tokens (symbol = scattering type * 3 + event); raises on an invalid expression."""
    lib = abi.load()
    arr = (C.c_uint8 * max(1, len(symbols)))(*symbols)
    rc = lib.prgpu_lpe_match(expression.encode(), arr, len(symbols))
    if rc < 0:
        abi.check(rc)
    return rc == 1
