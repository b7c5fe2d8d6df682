"""dustraytracer_amd -- MI355X-native path-tracing core behind DustRayTracer's Renderer/Scene API.

Python host-side mirror of the reference's classes over the C ABI of include/drt.h
(dustraytracer_amd/libdrt_hip.so, hand-written HIP for gfx950).  Names follow the reference:

    Scene.loadGLTFmodel            Core/Scene/Scene.cuh:41-57
    BVHBuilder.buildIterative      Core/BVH/BVHBuilder.cuh:12-23
    Camera                         Core/Scene/Camera.cuh:14-48
    RendererSettings               Core/Scene/RendererSettings.h:4-35
    Renderer.ResizeBuffer/Render/resetAccumulationBuffer/getSampleCount   Core/Renderer.hpp:14-47

There is no CPU fallback: importing works anywhere the shared library loads, but creating a Renderer
without a GPU raises DrtError.  A missing shared library raises ImportError (build it with
`python -c "import __graft_entry__ as g; g.build()"` or `make -C dustraytracer_amd/csrc`).
"""
import collections
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DRT_LIB_OVERRIDE") or os.path.join(_HERE, "libdrt_hip.so")      # override: A/B of builds (tools/ab_libs.py)

if not os.path.exists(LIB_PATH):
    raise ImportError("dustraytracer_amd: %s is missing -- the HIP extension must be built "
                      "(make -C dustraytracer_amd/csrc); there is no fallback path" % LIB_PATH)


def _preload_hip_runtime():
    """One HIP runtime per process.  libdrt_hip.so needs libamdhip64.so.7; PyTorch-ROCm wheels bundle
    their own copy under the same soname.  Whichever copy is loaded first serves both, and torch
    finds no GPU when the system copy was loaded before its own.  So when a torch wheel is installed
    (and DRT_HIP_RUNTIME != "system") its copy is loaded first, without importing torch."""
    import importlib.util
    import sys
    if os.environ.get("DRT_HIP_RUNTIME", "torch") == "system" or "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


_preload_hip_runtime()
_lib = C.CDLL(LIB_PATH)


class DrtError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("drt error %d: %s" % (code, message))
        self.code = code


OK, ERR_INVALID, ERR_IO, ERR_PARSE, ERR_UNSUPPORTED, ERR_DEVICE, ERR_BVH = 0, -1, -2, -3, -4, -5, -6


class RendererSettings(C.Structure):
    """Core/Scene/RendererSettings.h:4-35"""
    NORMALMODE, DEBUGMODE = 0, 1
    ALBEDO_DEBUG, NORMAL_DEBUG, BARYCENTRIC_DEBUG, UVS_DEBUG, MESHBVH_DEBUG, WORLDBVH_DEBUG = range(6)
    _fields_ = [("gamma_correction", C.c_int32), ("tone_mapping", C.c_int32), ("enableSunlight", C.c_int32),
                ("max_samples", C.c_int32), ("ray_bounce_limit", C.c_int32), ("RenderMode", C.c_int32),
                ("DebugMode", C.c_int32), ("sunlight_dir", C.c_float * 2), ("sunlight_color", C.c_float * 3),
                ("sunlight_intensity", C.c_float), ("sky_color", C.c_float * 3), ("sky_intensity", C.c_float)]

    def __init__(self, **kw):
        super().__init__()
        _lib.drt_default_settings(C.byref(self))
        for k, v in kw.items():
            _assign(self, k, v)


class MaterialModel(C.Structure):
    """include/drt.h drt_material_model: opt-in emissive term / metallic lobe (NOT reference behaviour; all zero = reference image)."""
    _fields_ = [("emissive", C.c_int32), ("specular", C.c_int32), ("emissive_scale", C.c_float), ("transmission", C.c_int32)]

    def __init__(self, emissive=0, specular=0, emissive_scale=1.0, transmission=0):
        super().__init__(int(emissive), int(specular), float(emissive_scale), int(transmission))


class _CameraPOD(C.Structure):
    _fields_ = [("exposure", C.c_float), ("vfov_rad", C.c_float), ("defocus_angle", C.c_float),
                ("focus_dist", C.c_float), ("position", C.c_float * 3), ("forward", C.c_float * 3)]


class Camera:
    """Core/Scene/Camera.cuh:14-48 (public fields + OnUpdate/Rotate/GetPosition)."""

    def __init__(self, pos=(0.0, 2.0, 5.0)):
        pod = _CameraPOD()
        _lib.drt_default_camera(C.byref(pod))
        self.exposure, self.vfov_rad = pod.exposure, pod.vfov_rad
        self.defocus_angle, self.focus_dist = pod.defocus_angle, pod.focus_dist
        self.m_movement_speed = 10.0
        self.m_Position = np.array(pos, np.float32)
        self.m_Forward_dir = np.array([0, 0, -1], np.float32)
        self.m_Up_dir = np.array([0, 1, 0], np.float32)
        self.m_Right_dir = np.cross(self.m_Forward_dir, self.m_Up_dir).astype(np.float32)

    def GetPosition(self):
        return self.m_Position.copy()

    def OnUpdate(self, velocity, delta):
        """Camera.cu:44-58: move along the camera basis (the C ABI's implementation: fp32, the reference's order)."""
        v = np.ascontiguousarray(velocity, np.float32)
        self.m_Position = np.ascontiguousarray(self.m_Position, np.float32)
        r, u, f = (np.ascontiguousarray(a, np.float32) for a in (self.m_Right_dir, self.m_Up_dir, self.m_Forward_dir))
        _lib.drt_camera_move(self.m_Position.ctypes.data, r.ctypes.data, u.ctypes.data, f.ctypes.data, v.ctypes.data,
                             C.c_float(self.m_movement_speed), C.c_float(delta))

    def Rotate(self, delta):
        """Camera.cu:61-80: delta = (sin_x, cos_x, sin_y, cos_y)."""
        d = np.ascontiguousarray(delta, np.float32)
        self.m_Forward_dir = np.ascontiguousarray(self.m_Forward_dir, np.float32)
        self.m_Right_dir = np.ascontiguousarray(self.m_Right_dir, np.float32)
        u = np.ascontiguousarray(self.m_Up_dir, np.float32)
        _lib.drt_camera_rotate(self.m_Forward_dir.ctypes.data, self.m_Right_dir.ctypes.data, u.ctypes.data, d.ctypes.data)

    def _pod(self):
        pod = _CameraPOD()
        pod.exposure, pod.vfov_rad = self.exposure, self.vfov_rad
        pod.defocus_angle, pod.focus_dist = self.defocus_angle, self.focus_dist
        for i in range(3):
            pod.position[i] = float(self.m_Position[i])
            pod.forward[i] = float(self.m_Forward_dir[i])
        return pod


TRIANGLE_DTYPE = np.dtype({"names": ["centroid", "vertex", "face_normal", "material"],
                           "formats": [("<f4", 3), (np.dtype([("position", "<f4", 3), ("normal", "<f4", 3), ("uv", "<f4", 2)]), 3),
                                       ("<f4", 3), "<i4"],
                           "offsets": [0, 16, 112, 124], "itemsize": 128})
NODE_DTYPE = np.dtype({"names": ["is_leaf", "bmin", "bmax", "child1", "child2", "prim_count", "prim_start"],
                       "formats": ["u1", ("<f4", 3), ("<f4", 3), "<i4", "<i4", "<i4", "<i4"],
                       "offsets": [0, 4, 16, 28, 32, 36, 40], "itemsize": 44})
MATERIAL_DTYPE = np.dtype({"names": ["albedo", "emissive", "albedo_tex", "roughness", "transmission", "refractive_index", "metallic"],
                           "formats": [("<f4", 3), ("<f4", 3), "<i4", "<f4", "u1", "<f4", "u1"],
                           "offsets": [0, 12, 24, 28, 32, 36, 40], "itemsize": 44})
MESH_DTYPE = np.dtype([("primitives_offset", "<i4"), ("tris_count", "<i4")])


class _TexInfo(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("components", C.c_int32)]


class DenoiseParams(C.Structure):
    """include/drt.h drt_denoise_params: a-trous passes and the three edge-stopping sigmas (defaults 5, 0.5, 0.1, 0.1)."""
    _fields_ = [("iterations", C.c_int32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_albedo", C.c_float)]

    def __init__(self, **kw):
        super().__init__()
        _lib.drt_default_denoise_params(C.byref(self))
        for k, v in kw.items():
            setattr(self, k, v)


class TemporalParams(C.Structure):
    """include/drt.h drt_temporal_params: a-trous passes, history cap, blend floor, the reprojection's normal test and the
    three edge-stopping sigmas (defaults 5, 32, 0, 0.9, 4, 0.1, 0.1)."""
    _fields_ = [("iterations", C.c_int32), ("max_history", C.c_int32), ("alpha_min", C.c_float), ("normal_cos_min", C.c_float),
                ("sigma_luma", C.c_float), ("sigma_normal", C.c_float), ("sigma_albedo", C.c_float)]

    def __init__(self, **kw):
        super().__init__()
        _lib.drt_default_temporal_params(C.byref(self))
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise TypeError("TemporalParams has no field %r" % k)
            setattr(self, k, v)


class UpscaleParams(C.Structure):
    """include/drt.h drt_upscale_params: the source (0 framebuffer, 1 denoised target), albedo demodulation, the three
    edge-stopping sigmas and the albedo floor (defaults 0, 0, 0.1, 0.05, 0.1, 0.01)."""
    _fields_ = [("source", C.c_int32), ("demodulate", C.c_int32), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float),
                ("sigma_albedo", C.c_float), ("albedo_floor", C.c_float)]

    def __init__(self, **kw):
        super().__init__()
        _lib.drt_default_upscale_params(C.byref(self))
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise TypeError("UpscaleParams has no field %r" % k)
            setattr(self, k, v)


class AdaptiveParams(C.Structure):
    """include/drt.h drt_adaptive_params: the samples of one call (0 = 4 per pixel), the per-call bounds of a pixel's count, the
    relative standard error below which a pixel is converged (0 = off) and the luminance floor (defaults 0, 1, 64, 0, 0.01)."""
    _fields_ = [("budget", C.c_uint32), ("min_spp", C.c_uint32), ("max_spp", C.c_uint32), ("target_error", C.c_float),
                ("luma_floor", C.c_float)]

    def __init__(self, **kw):
        super().__init__()
        _lib.drt_default_adaptive_params(C.byref(self))
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise TypeError("AdaptiveParams has no field %r" % k)
            setattr(self, k, v)


class AdaptiveInfo(C.Structure):
    """include/drt.h drt_adaptive_info: what one RenderAdaptive call did."""
    _fields_ = [("samples", C.c_uint32), ("active_pixels", C.c_uint32), ("max_count", C.c_uint32), ("ms", C.c_float)]

    def __repr__(self):
        return "AdaptiveInfo(samples=%d, active_pixels=%d, max_count=%d, ms=%.3f)" % (self.samples, self.active_pixels, self.max_count, self.ms)


class _Grid(C.Structure):
    """include/drt.h drt_grid: the lattice of an isosurface's field (host memory)."""
    _fields_ = [("lo", C.c_float * 3), ("cell", C.c_float * 3), ("dims", C.c_uint32 * 3)]


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("samples", "rays", "node_visits", "inner_visits", "tri_tests",
                                           "hits_textured", "hits_flat", "shadow_rays", "inner_visits_shadow",
                                           "tri_tests_shadow")] + [("phase_execs", C.c_uint64 * 4), ("phase_lanes", C.c_uint64 * 4), ("phase_ticks", C.c_uint64 * 4), ("wave_ticks", C.c_uint64), ("sampler_tries", C.c_uint64)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, t in self._fields_ if t is C.c_uint64 and n != "wave_ticks"}

    def phase_stats(self):
        """wave_queue kernel: (executions, mean active lanes) of the T, N, S, R phases."""
        return {k: (int(self.phase_execs[i]), self.phase_lanes[i] / max(int(self.phase_execs[i]), 1))
                for i, k in enumerate("TNSR")}

    def algorithmic_bytes(self):
        """40 B/sample + 56 B/interior visit + 36 B/triangle test + 60|32 B/shaded hit (+ shadow terms)."""
        return (40 * self.samples + 56 * self.inner_visits + 36 * self.tri_tests + 60 * self.hits_textured
                + 32 * self.hits_flat + 56 * self.inner_visits_shadow + 36 * self.tri_tests_shadow)


def _sig(name, restype, *argtypes):
    if name.startswith("drt_debug_") and not hasattr(_lib, name):
        return None                   # older A/B builds (DRT_LIB_OVERRIDE) may lack a debug entry point
    fn = getattr(_lib, name)          # AttributeError here = the library does not export what drt.h declares
    fn.restype = restype
    fn.argtypes = list(argtypes)
    return fn


_P = C.c_void_p
_sig("drt_abi_version", C.c_int)
_sig("drt_last_error", C.c_char_p)
_sig("drt_device_count", C.c_int)
_sig("drt_default_settings", None, C.POINTER(RendererSettings))
_sig("drt_default_camera", None, C.POINTER(_CameraPOD))
_sig("drt_camera_rotate", None, _P, _P, _P, _P)
_sig("drt_camera_move", None, _P, _P, _P, _P, _P, C.c_float, C.c_float)
_sig("drt_scene_create", _P)
_sig("drt_scene_destroy", None, _P)
_sig("drt_scene_load_gltf", C.c_int, _P, C.c_char_p)
_sig("drt_scene_load_gltf_ex", C.c_int, _P, C.c_char_p, C.c_uint32)
_sig("drt_scene_set_geometry", C.c_int, _P, _P, _P, _P, _P, C.c_int32)
_sig("drt_scene_add_material", C.c_int, _P, C.POINTER(C.c_float), C.c_int32)
_sig("drt_scene_add_texture", C.c_int, _P, _P, C.c_int32, C.c_int32, C.c_int32)
_sig("drt_scene_build_bvh", C.c_int, _P, C.c_int32, C.c_int32)
_sig("drt_scene_validate", C.c_int, _P)
_sig("drt_scene_add_material_ex", C.c_int, _P, _P)
_sig("drt_pcg_hash", C.c_uint32, C.c_uint32)
_sig("drt_random_float", C.c_float, C.POINTER(C.c_uint32))
_sig("drt_scene_build_bvh_recursive", C.c_int, _P, C.c_int32, C.c_int32)
_sig("drt_scene_build_bvh_device", C.c_int, _P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float))
for _n in ("triangle", "node", "material", "texture", "mesh"):
    _sig("drt_scene_%s_count" % _n, C.c_int32, _P)
_sig("drt_scene_bvh_depth", C.c_int32, _P)
for _n in ("triangles", "nodes", "materials", "meshes"):
    _sig("drt_scene_get_%s" % _n, C.c_int, _P, _P, C.c_int32)
_sig("drt_scene_get_texture_info", C.c_int, _P, C.c_int32, C.POINTER(_TexInfo))
_sig("drt_scene_get_texture_texels", C.c_int, _P, C.c_int32, _P, C.c_size_t)
_sig("drt_renderer_create", _P, C.c_int32)
_sig("drt_renderer_destroy", None, _P)
_sig("drt_renderer_resize", C.c_int, _P, C.c_uint32, C.c_uint32)
_sig("drt_renderer_set_settings", C.c_int, _P, C.POINTER(RendererSettings))
_sig("drt_renderer_get_settings", C.c_int, _P, C.POINTER(RendererSettings))
_sig("drt_renderer_render", C.c_int, _P, C.POINTER(_CameraPOD), _P, C.POINTER(C.c_float))
_sig("drt_renderer_render_batch", C.c_int, _P, C.POINTER(_CameraPOD), _P, C.c_uint32, C.POINTER(C.c_float))
_sig("drt_renderer_render_batch_async", C.c_int, _P, C.POINTER(_CameraPOD), _P, C.c_uint32)
_sig("drt_renderer_wait", C.c_int, _P, C.POINTER(C.c_float))
_sig("drt_renderer_reset", C.c_int, _P)
for _n in ("width", "height", "sample_count", "local_rows"):
    _sig("drt_renderer_%s" % _n, C.c_uint32, _P)
_sig("drt_renderer_read_rgba32f", C.c_int, _P, _P, C.c_size_t)
_sig("drt_renderer_read_accum", C.c_int, _P, _P, C.c_size_t)
_sig("drt_renderer_device_rgba", _P, _P)
_sig("drt_renderer_device_accum", _P, _P)
_sig("drt_renderer_set_shard", C.c_int, _P, C.c_uint32, C.c_uint32, C.c_uint32)
_sig("drt_renderer_bind_buffers", C.c_int, _P, _P, _P)
_sig("drt_renderer_set_stream", C.c_int, _P, _P)
_sig("drt_renderer_set_counting", C.c_int, _P, C.c_int32)
_sig("drt_renderer_get_counters", C.c_int, _P, C.POINTER(Counters))
_sig("drt_renderer_set_material_model", C.c_int, _P, _P)
_sig("drt_renderer_get_material_model", C.c_int, _P, _P)
_sig("drt_renderer_kernel_info", C.c_int, _P, C.c_char_p, C.c_size_t)
_sig("drt_renderer_kernel_span", C.c_int, _P, C.POINTER(C.c_float))
_sig("drt_renderer_launch_count", C.c_int32, _P)
_sig("drt_renderer_set_frames_in_flight", C.c_int, _P, C.c_int32)
_sig("drt_assemble_shards", C.c_int, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _P)
_sig("drt_shard_rows", C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32)
_sig("drt_debug_decode_image", C.c_int, _P, C.c_size_t, _P, _P, C.c_size_t)
_sig("drt_debug_kat", C.c_int, C.c_int32, C.c_int32, _P, C.c_size_t, _P, C.c_size_t, C.c_uint32, C.POINTER(_CameraPOD), C.c_uint32, C.c_uint32)
_sig("drt_debug_hash_cycles", C.c_int, C.c_int32, C.c_uint32, _P, C.c_uint32, C.POINTER(C.c_uint32))
_sig("drt_group_create", _P, C.POINTER(C.c_int32), C.c_int32)
_sig("drt_group_destroy", None, _P)
_sig("drt_group_size", C.c_int32, _P)
_sig("drt_group_renderer", _P, _P, C.c_int32)
_sig("drt_group_resize", C.c_int, _P, C.c_uint32, C.c_uint32)
_sig("drt_group_set_settings", C.c_int, _P, _P)
_sig("drt_group_reset", C.c_int, _P)
_sig("drt_group_render_batch", C.c_int, _P, _P, _P, C.c_uint32, C.POINTER(C.c_float))
_sig("drt_group_render_batch_async", C.c_int, _P, _P, _P, C.c_uint32)
_sig("drt_group_wait", C.c_int, _P, C.POINTER(C.c_float))
_sig("drt_group_sample_count", C.c_uint32, _P)
_sig("drt_group_device_rgba", _P, _P)
_sig("drt_group_read_rgba32f", C.c_int, _P, _P, C.c_size_t)
_sig("drt_shard_stripe", C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64))
_sig("drt_debug_wave_queue_plans", C.c_int, _P, C.c_char_p, C.c_size_t)
_sig("drt_debug_pool_stats", C.c_int, _P, _P, C.c_int32)
_sig("drt_debug_check_rcp", C.c_int, C.c_int32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64))
_sig("drt_debug_check_sqrt", C.c_int, C.c_int32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64))
_sig("drt_renderer_trace_rays", C.c_int, _P, _P, _P, _P, C.c_uint32, _P)
_sig("drt_renderer_occluded", C.c_int, _P, _P, _P, _P, C.c_uint32, _P)
_sig("drt_renderer_nearest", C.c_int, _P, _P, _P, _P, C.c_uint32, _P)
_sig("drt_renderer_crossings", C.c_int, _P, _P, _P, _P, C.c_uint32, _P)
_sig("drt_renderer_sphere_cast", C.c_int, _P, _P, _P, _P, _P, C.c_uint32, _P)
_sig("drt_renderer_list_hits", C.c_int, _P, _P, _P, _P, _P, C.c_uint32, _P, C.c_uint32, _P)
_sig("drt_renderer_nearest_list", C.c_int, _P, _P, _P, _P, _P, _P, C.c_uint32, _P, C.c_uint32, C.c_int32, _P)
_sig("drt_renderer_overlap_boxes", C.c_int, _P, _P, _P, _P, _P, C.c_uint32, _P, C.c_uint32, C.c_int32, _P)
_sig("drt_renderer_overlap_triangles", C.c_int, _P, _P, _P, _P, _P, C.c_uint32, _P, C.c_uint32, C.c_int32, _P)
_sig("drt_renderer_plane_sections", C.c_int, _P, _P, _P, _P, _P, C.c_uint32, _P, C.c_uint32, C.c_int32, _P)
_sig("drt_renderer_intersect_triangles", C.c_int, _P, _P, _P, _P, _P, C.c_uint32, _P, C.c_uint32, _P)
_sig("drt_renderer_triangle_distance", C.c_int, _P, _P, _P, _P, _P, C.c_uint32, C.c_int32, _P)
_sig("drt_renderer_triangle_cast", C.c_int, _P, _P, _P, _P, _P, C.c_uint32, C.c_int32, _P)
_sig("drt_renderer_surface_lookup", C.c_int, _P, _P, _P, _P, _P, C.c_uint32, _P)
_sig("drt_renderer_surface_weights", C.c_int, _P, _P, _P, _P)
_sig("drt_renderer_sample_surface", C.c_int, _P, _P, C.c_uint32, C.c_uint32, _P, C.c_uint32, _P)
_sig("drt_renderer_ambient_occlusion", C.c_int, _P, _P, _P, C.c_uint32, _P, _P, _P)
_sig("drt_debug_ambient_stats", C.c_int, _P, C.c_int32, _P)
_sig("drt_renderer_winding_numbers", C.c_int, _P, _P, _P, C.c_uint32, C.c_float, _P, _P)
_sig("drt_renderer_winding_inside", C.c_int, _P, _P, _P, C.c_uint32, C.c_float, C.c_float, _P, _P)
_sig("drt_renderer_winding_signed_distance", C.c_int, _P, _P, _P, C.c_uint32, C.c_float, C.c_float, _P, _P)
_sig("drt_debug_winding_moments", C.c_int, _P, _P, _P, C.c_size_t, _P)
_sig("drt_renderer_isosurface", C.c_int, _P, _P, _P, C.c_float, C.c_float, C.c_int32, _P, _P, C.c_uint32, _P, _P)
_sig("drt_renderer_weld", C.c_int, _P, _P, C.c_uint32, C.c_uint32, _P, _P, _P, C.c_uint32, _P, _P)
_sig("drt_renderer_vertex_normals", C.c_int, _P, _P, C.c_uint32, _P, C.c_uint32, C.c_int32, _P, _P)
_sig("drt_renderer_smooth_vertices", C.c_int, _P, _P, C.c_uint32, _P, C.c_uint32, _P, C.c_uint32, _P, _P, _P)
_sig("drt_renderer_simplify", C.c_int, _P, _P, C.c_uint32, _P, C.c_uint32, _P, C.c_int32, _P, _P, _P, C.c_uint32, _P, _P, C.c_uint32, _P, _P)
_sig("drt_renderer_tri_adjacency", C.c_int, _P, _P, C.c_uint32, C.c_uint32, _P, _P, _P, C.c_uint32, _P, _P)
_sig("drt_renderer_face_adjacency", C.c_int, _P, _P, C.c_uint32, _P, _P, _P, C.c_uint32, _P, _P)
_sig("drt_renderer_boundary_vertices", C.c_int, _P, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P)
_sig("drt_renderer_adjacency_route", C.c_int, _P)
_sig("drt_renderer_subdivide", C.c_int, _P, _P, C.c_uint32, _P, C.c_uint32, C.c_int32, _P, _P, C.c_uint32, _P, _P, _P)
_sig("drt_scene_edge_adjacency", C.c_int, _P, _P, C.c_uint32)
_sig("drt_renderer_chain_sections", C.c_int, _P, _P, _P, _P, _P, _P, C.c_uint32, C.c_uint32, _P)
_sig("drt_tri_edge_adjacency", C.c_int, _P, C.c_uint32, _P, C.c_uint32)
_sig("drt_renderer_chain_intersections", C.c_int, _P, _P, _P, _P, _P, _P, _P, C.c_uint32, C.c_uint32, _P)
_sig("drt_renderer_shell_labels", C.c_int, _P, _P, _P, _P, _P)
_sig("drt_renderer_boundary_loops", C.c_int, _P, _P, _P, C.c_uint32, _P, _P)
_sig("drt_renderer_shell_terms", C.c_int, _P, _P, _P, _P)
_sig("drt_renderer_edge_adjacency", C.c_int, _P, _P, _P, _P)
_sig("drt_renderer_topology_steps", C.c_int, _P, _P)
_sig("drt_renderer_inside", C.c_int, _P, _P, _P, _P, C.c_uint32, C.c_int32, _P)
_sig("drt_renderer_signed_distance", C.c_int, _P, _P, _P, _P, C.c_uint32, C.c_int32, _P)
_sig("drt_renderer_render_guides", C.c_int, _P, C.POINTER(_CameraPOD), _P, C.c_uint32, _P, _P)
_sig("drt_default_denoise_params", None, C.POINTER(DenoiseParams))
_sig("drt_renderer_denoise", C.c_int, _P, C.POINTER(_CameraPOD), _P, C.POINTER(DenoiseParams), C.POINTER(C.c_float))
_sig("drt_renderer_read_denoised_rgba32f", C.c_int, _P, _P, C.c_size_t)
_sig("drt_renderer_device_denoised", _P, _P)
_sig("drt_default_temporal_params", None, C.POINTER(TemporalParams))
_sig("drt_renderer_temporal_denoise", C.c_int, _P, C.POINTER(_CameraPOD), _P, C.POINTER(TemporalParams), C.POINTER(C.c_float))
_sig("drt_renderer_temporal_reset", C.c_int, _P)
_sig("drt_renderer_read_temporal", C.c_int, _P, C.c_int32, _P, C.c_size_t)
_sig("drt_renderer_device_temporal", _P, _P, C.c_int32)
_sig("drt_renderer_track_motion", C.c_int, _P, C.c_int32)
_sig("drt_renderer_motion_advance", C.c_int, _P)
_sig("drt_renderer_motion_vectors", C.c_int, _P, C.POINTER(_CameraPOD), C.POINTER(_CameraPOD), _P, _P, _P)
_sig("drt_default_upscale_params", None, C.POINTER(UpscaleParams))
_sig("drt_renderer_upscale", C.c_int, _P, C.POINTER(_CameraPOD), _P, C.c_uint32, C.c_uint32, C.POINTER(UpscaleParams), C.POINTER(C.c_float))
_sig("drt_renderer_read_upscaled_rgba32f", C.c_int, _P, _P, C.c_size_t)
_sig("drt_renderer_device_upscaled", _P, _P)
_sig("drt_debug_upscale", C.c_int, C.c_int32, _P, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(UpscaleParams), _P)
_sig("drt_default_adaptive_params", None, C.POINTER(AdaptiveParams))
_sig("drt_renderer_render_adaptive", C.c_int, _P, C.POINTER(_CameraPOD), _P, C.POINTER(AdaptiveParams), C.POINTER(AdaptiveInfo))
_sig("drt_renderer_adaptive_reset", C.c_int, _P)
_sig("drt_renderer_read_adaptive", C.c_int, _P, C.c_int32, _P, C.c_size_t)
_sig("drt_renderer_device_adaptive", _P, _P, C.c_int32)
_sig("drt_debug_adaptive_plan", C.c_int, C.c_int32, _P, C.c_uint32, C.POINTER(AdaptiveParams), C.c_int32, _P, _P, C.POINTER(C.c_uint64))
_sig("drt_debug_adaptive_weights", C.c_int, C.c_int32, _P, _P, C.c_uint32, C.POINTER(AdaptiveParams), _P, C.POINTER(C.c_uint64),
     C.POINTER(C.c_uint32))
_sig("drt_scene_get_triangle_order", C.c_int, _P, _P, C.c_int32)
_sig("drt_scene_refit", C.c_int, _P, _P, _P)
_sig("drt_renderer_refit", C.c_int, _P, _P, _P, _P, C.POINTER(C.c_float), _P)
_sig("drt_renderer_camera_rays", C.c_int, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P)
_sig("drt_renderer_radiance", C.c_int, _P, _P, _P, _P, C.c_uint32, C.c_int32, _P)
_sig("drt_debug_pack_scene", C.c_int, _P, _P, C.c_size_t, _P, C.c_size_t, _P)
_sig("drt_debug_read_device_scene", C.c_int, _P, _P, C.c_size_t, _P, C.c_size_t, _P)

EXPORTED_SYMBOLS = [n for n in dir(_lib) if n.startswith("drt_")]


def _check(rc):
    if rc < 0:
        raise DrtError(rc, (_lib.drt_last_error() or b"").decode("utf-8", "replace"))
    return rc


def _assign(struct, key, value):
    cur = getattr(struct, key)
    if hasattr(cur, "__len__"):
        for i, v in enumerate(value):
            cur[i] = v
    else:
        setattr(struct, key, value)


def device_count():
    return _lib.drt_device_count()


def shard_rows(height, stripe_rows, rank, world):
    return int(_lib.drt_shard_rows(height, stripe_rows, rank, world))


class Scene:
    """Core/Scene/Scene.cuh:41-57: loadGLTFmodel + the public buffers (as numpy copies)."""

    def __init__(self):
        self._h = _lib.drt_scene_create()
        if not self._h:
            raise DrtError(ERR_INVALID, "cannot create scene")

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:              # (at interpreter shutdown the module's globals may be gone already)
            _lib.drt_scene_destroy(h)

    def loadGLTFmodel(self, filepath, strict=False):
        """strict=False: the reference's reading of the file (Scene.cu, quirks included); True: the glTF 2.0 specification's
        (node transforms and hierarchy, accessor offsets / strides / component types, u8/u16/u32 or no indices, ...)."""
        _check(_lib.drt_scene_load_gltf_ex(self._h, os.fsencode(filepath), 1 if strict else 0))
        return True

    def setGeometry(self, positions, normals, uvs, material_ids):
        pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 9)
        nrm = np.ascontiguousarray(normals, np.float32).reshape(-1, 9)
        uv = np.ascontiguousarray(uvs, np.float32).reshape(-1, 6)
        mat = np.ascontiguousarray(material_ids, np.int32).reshape(-1)
        if not (len(pos) == len(nrm) == len(uv) == len(mat)):
            raise ValueError("setGeometry: %d position, %d normal, %d uv triangles for %d material ids" % (len(pos), len(nrm), len(uv), len(mat)))
        _check(_lib.drt_scene_set_geometry(self._h, pos.ctypes.data, nrm.ctypes.data, uv.ctypes.data, mat.ctypes.data, len(mat)))

    def validate(self):
        """Raises DrtError(ERR_INVALID) if a triangle names a material, or a material a texture, that does not exist."""
        _check(_lib.drt_scene_validate(self._h))

    def addMaterial(self, albedo, albedo_tex=-1):
        a = (C.c_float * 3)(*albedo)
        return _check(_lib.drt_scene_add_material(self._h, a, albedo_tex))

    def addMaterialEx(self, albedo, albedo_tex=-1, emissive=(0, 0, 0), roughness=0.0, metallic=False, transmission=False, refractive_index=1.45):
        """A material with the fields only the opt-in material model reads (Renderer.setMaterialModel)."""
        m = np.zeros(1, MATERIAL_DTYPE)
        m["albedo"], m["emissive"], m["albedo_tex"], m["roughness"], m["metallic"] = albedo, emissive, albedo_tex, roughness, int(bool(metallic))
        m["transmission"], m["refractive_index"] = int(bool(transmission)), refractive_index
        return _check(_lib.drt_scene_add_material_ex(self._h, m.ctypes.data))

    def addTexture(self, texels):
        t = np.ascontiguousarray(texels, np.uint8)
        h, w, c = t.shape
        return _check(_lib.drt_scene_add_texture(self._h, t.ctypes.data, w, h, c))

    def _copy(self, getter, count, dtype):
        out = np.zeros(count, dtype)
        if count:
            _check(getter(self._h, out.ctypes.data, count))
        return out

    @property
    def m_PrimitivesBuffer(self):
        return self._copy(_lib.drt_scene_get_triangles, _lib.drt_scene_triangle_count(self._h), TRIANGLE_DTYPE)

    @property
    def m_BVHNodes(self):
        return self._copy(_lib.drt_scene_get_nodes, _lib.drt_scene_node_count(self._h), NODE_DTYPE)

    @property
    def m_Material(self):
        return self._copy(_lib.drt_scene_get_materials, _lib.drt_scene_material_count(self._h), MATERIAL_DTYPE)

    @property
    def m_Meshes(self):
        return self._copy(_lib.drt_scene_get_meshes, _lib.drt_scene_mesh_count(self._h), MESH_DTYPE)

    @property
    def m_Textures(self):
        out = []
        for i in range(_lib.drt_scene_texture_count(self._h)):
            info = _TexInfo()
            _check(_lib.drt_scene_get_texture_info(self._h, i, C.byref(info)))
            tex = np.zeros((info.height, info.width, info.components), np.uint8)
            _check(_lib.drt_scene_get_texture_texels(self._h, i, tex.ctypes.data, tex.size))
            out.append(tex)
        return out

    @property
    def bvh_depth(self):
        return _lib.drt_scene_bvh_depth(self._h)

    def triangleOrder(self):
        """int32 [n]: the load index (setGeometry / file order) of each triangle of m_PrimitivesBuffer (drt_scene_get_triangle_order)."""
        return self._copy(_lib.drt_scene_get_triangle_order, _lib.drt_scene_triangle_count(self._h), np.int32)

    def edgeAdjacency(self):
        """int32 [n, 3]: the twin half-edge 3 * t' + e' of edge e (vertex e to vertex (e + 1) % 3) of each triangle of
        m_PrimitivesBuffer, by bit-equal positions; -1 on a boundary edge, -2 where the edge is non-manifold, flipped or of zero
        length (drt_scene_edge_adjacency).  Needs a BVH: the table is in tree order."""
        n = _lib.drt_scene_triangle_count(self._h)
        out = np.zeros((n, 3), np.int32)
        _check(_lib.drt_scene_edge_adjacency(self._h, out.ctypes.data, 3 * n))
        return out

    def _refit_arrays(self, positions, normals):
        n = _lib.drt_scene_triangle_count(self._h)
        out = []
        for what, a in (("positions", positions), ("normals", normals)):
            if a is None:
                out.append(None)
                continue
            a = np.ascontiguousarray(a, np.float32)
            if a.size != 9 * n:
                raise DrtError(ERR_INVALID, "%s: %d values, [%d, 3, 3] expected" % (what, a.size, n))
            out.append(a)
        return out

    def refit(self, positions, normals=None):
        """Refit the BVH to new vertex positions [n, 3, 3] in load order (and normals, None = keep them): drt_scene_refit.
        Tree topology and triangle order stay; renderers upload the scene again."""
        pos, nrm = self._refit_arrays(positions, normals)
        _check(_lib.drt_scene_refit(self._h, pos.ctypes.data, nrm.ctypes.data if nrm is not None else None))

    def debugPack(self):
        """(InnerNode records uint8 [n_inner, 64], TriHot records uint8 [n, 48], root box float32 [6]) of the host pack (drt_debug_pack_scene)."""
        nodes = self.m_BVHNodes
        inner = np.zeros((int((nodes["is_leaf"] == 0).sum()), 64), np.uint8)
        hot = np.zeros((_lib.drt_scene_triangle_count(self._h), 48), np.uint8)
        root = np.zeros(6, np.float32)
        _check(_lib.drt_debug_pack_scene(self._h, inner.ctypes.data, inner.size, hot.ctypes.data, hot.size, root.ctypes.data))
        return inner, hot, root


class BVHBuilder:
    """Core/BVH/BVHBuilder.cuh:12-23 (defaults of the class; the editor sets 20 / 8, EditorLayer.cpp:52-55)."""

    def __init__(self):
        self.m_BinCount = 8
        self.m_TargetLeafPrimitivesCount = 6
        self.m_BuildDevice = -1          # new: >= 0 builds the same tree on that GPU (drt_scene_build_bvh_device)
        self.m_LastBuildDeviceMs = 0.0

    def buildIterative(self, scene):
        if self.m_BuildDevice >= 0:
            ms = C.c_float(0)
            _check(_lib.drt_scene_build_bvh_device(scene._h, self.m_TargetLeafPrimitivesCount, self.m_BinCount, self.m_BuildDevice, C.byref(ms)))
            self.m_LastBuildDeviceMs = ms.value
        else:
            _check(_lib.drt_scene_build_bvh(scene._h, self.m_TargetLeafPrimitivesCount, self.m_BinCount))
        return scene

    def build(self, scene):
        """BVHBuilder::build (BVHBuilder.cu:100-173): the same tree and triangle order through recursion; the node array comes in
        the recursion's order (children after both of their subtrees, root last), as drt_scene_get_nodes then returns it."""
        _check(_lib.drt_scene_build_bvh_recursive(scene._h, self.m_TargetLeafPrimitivesCount, self.m_BinCount))
        return scene


def shard_stripe(width, height, stripe_rows, rank, world, k):
    """(offset in the rank's compact shard, offset in the full image, length) of the rank's k-th stripe, in floats of an
    RGBA32F frame; None when the rank has no k-th stripe."""
    so, do, cnt = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    if not _lib.drt_shard_stripe(width, height, stripe_rows, rank, world, k, C.byref(so), C.byref(do), C.byref(cnt)):
        return None
    return int(so.value), int(do.value), int(cnt.value)


class RendererGroup:
    """Several GPUs of one node behind the Renderer interface (drt_group_*): one process, a renderer per device, stripes
    gathered into the first device's image over RCCL.  Same calls as Renderer."""

    def __init__(self, devices=(0,)):
        arr = (C.c_int32 * len(devices))(*devices)
        self._h = _lib.drt_group_create(arr, len(devices))
        if not self._h:
            raise DrtError(ERR_DEVICE, (_lib.drt_last_error() or b"").decode())
        self.m_RendererSettings = RendererSettings()
        self._w = self._h_px = 0

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:              # (at interpreter shutdown the module's globals may be gone already)
            _lib.drt_group_destroy(h)

    def size(self):
        return int(_lib.drt_group_size(self._h))

    def ResizeBuffer(self, width, height):
        _check(_lib.drt_group_resize(self._h, width, height))
        self._w, self._h_px = width, height

    def resetAccumulationBuffer(self):
        _check(_lib.drt_group_reset(self._h))

    def getSampleCount(self):
        return int(_lib.drt_group_sample_count(self._h))

    def RenderBatch(self, cam, scene, n_frames):
        _check(_lib.drt_group_set_settings(self._h, C.byref(self.m_RendererSettings)))
        ms = C.c_float(0)
        pod = cam._pod()
        _check(_lib.drt_group_render_batch(self._h, C.byref(pod), scene._h, int(n_frames), C.byref(ms)))
        return ms.value

    def Render(self, cam, scene):
        return self.RenderBatch(cam, scene, 1)

    def RenderBatchAsync(self, cam, scene, n_frames):
        _check(_lib.drt_group_set_settings(self._h, C.byref(self.m_RendererSettings)))
        pod = cam._pod()
        _check(_lib.drt_group_render_batch_async(self._h, C.byref(pod), scene._h, int(n_frames)))

    def Wait(self):
        ms = C.c_float(0)
        _check(_lib.drt_group_wait(self._h, C.byref(ms)))
        return ms.value

    def GetRenderTargetImage(self):
        out = np.zeros((self._h_px, self._w, 4), np.float32)
        _check(_lib.drt_group_read_rgba32f(self._h, out.ctypes.data, out.size))
        return out

    def kernelInfo(self, index=0):
        buf = C.create_string_buffer(128)
        _check(_lib.drt_renderer_kernel_info(_lib.drt_group_renderer(self._h, index), buf, 128))
        return buf.value.decode()


FLT_MAX = float(np.finfo(np.float32).max)
RayHits = collections.namedtuple("RayHits", "t prim u v")     # closest-hit query results (Renderer.traceRays)
Nearest = collections.namedtuple("Nearest", "point d2 prim u v side")   # nearest-surface query results (Renderer.nearest)
Crossings = collections.namedtuple("Crossings", "count winding")       # crossing counts of rays (Renderer.crossings)
SphereHits = collections.namedtuple("SphereHits", "t prim u v point feature")   # first contacts of moving spheres (Renderer.sphereCast)
FirstHits = collections.namedtuple("FirstHits", "t prim u v count")     # the first k hits of rays, in order (Renderer.firstHits)
HitList = collections.namedtuple("HitList", "splits t prim u v")        # every hit of rays, in order, CSR (Renderer.listHits)
KNearest = collections.namedtuple("KNearest", "d2 prim u v point side count")   # the k nearest triangles of points (Renderer.kNearest)
NearList = collections.namedtuple("NearList", "splits d2 prim u v point side")  # every triangle within a radius, CSR (Renderer.withinRadius)
NEAR_GATHER, NEAR_K = 0, 1                                              # drt.h DRT_NEAR_*
BoxList = collections.namedtuple("BoxList", "splits prim")               # every triangle that touches boxes, CSR (Renderer.overlapBoxes)
BoxTable = collections.namedtuple("BoxTable", "prim count")             # the first k triangles that touch boxes (Renderer.overlapBoxes, k=)
TriList = collections.namedtuple("TriList", "splits prim")               # every triangle that query triangles touch, CSR (Renderer.overlapTriangles)
TriTable = collections.namedtuple("TriTable", "prim count")             # the first k triangles that query triangles touch (Renderer.overlapTriangles, k=)
OVERLAP_LIST, OVERLAP_ANY = 0, 1                                        # drt.h DRT_OVERLAP_*
TRIDIST_NEAREST, TRIDIST_ANY = 0, 1                                      # drt.h DRT_TRIDIST_*
TriNearest = collections.namedtuple("TriNearest", "d2 prim point_q point_t u v feature")   # the mesh triangle nearest query triangles (Renderer.triangleDistance)
MeshDistance = collections.namedtuple("MeshDistance", "d2 query prim point_q point_t feature")   # the nearest pair of a batch (Renderer.meshDistance)
TRICAST_FIRST, TRICAST_ANY = 0, 1                                        # drt.h DRT_TRICAST_*
TriHits = collections.namedtuple("TriHits", "t prim point normal u v feature")   # first contacts of translating triangles (Renderer.triangleCast)
MeshHit = collections.namedtuple("MeshHit", "t query prim point normal feature")   # the earliest contact of a batch (Renderer.meshCast)
# what lies on the surface at references (Renderer.surface): material -1 = no such triangle
Surface = collections.namedtuple("Surface", "position normal shading uv albedo emissive alpha roughness refractive_index material load_index texture "
                                            "metallic transmission")
SurfaceSamples = collections.namedtuple("SurfaceSamples", "prim u v")   # references drawn on the mesh by area (Renderer.sampleSurface)
SURFACE_SCAN_BLOCK = 256                                                 # drt.h DRT_SURFACE_SCAN_BLOCK
# cosine-weighted visibility at surface points (Renderer.ambientOcclusion): open -1 = a skipped point; sums = the exact integer record
AmbientOcclusion = collections.namedtuple("AmbientOcclusion", "open visibility bent sums")
AO_MAX_SAMPLES = 4096
SectionList = collections.namedtuple("SectionList", "splits p q prim code")   # every segment where planes cut the mesh, CSR (Renderer.planeSections)
SECTION_LIST, SECTION_ANY = 0, 1                                        # drt.h DRT_SECTION_*
CutList = collections.namedtuple("CutList", "splits p q prim code")     # every segment where query triangles cut the mesh, CSR (Renderer.intersectTriangles)
SelfCuts = collections.namedtuple("SelfCuts", "pairs p q code")         # the segments where the mesh cuts itself (Renderer.selfIntersectionSegments)
CHAIN_LINKED, CHAIN_BOUNDARY, CHAIN_NON_MANIFOLD, CHAIN_NOT_LISTED, CHAIN_OTHER_EDGES, CHAIN_MISS = range(6)   # drt.h: a record's exit status


def _segment_sums(torch, term, at):
    """The sums of the float64 `term` over the ranges at[i]:at[i + 1], on the device, deterministic, no atomics: a running sum over ALL
    terms and its differences at the ends of the ranges.  The running sum rounds relative to what the ranges before have summed to,
    which would leave a small sum behind large ones with few digits.  So the error of every step, (run[i] + term[i]) - run[i + 1],
    is computed with Knuth's two-sum and summed the same way: in exact arithmetic the two differences add up to the range's own sum
    whatever values the scan left in `run` (a device scan does not add left to right), and in float64 the error terms are of the
    size of run's rounding, so theirs is second order."""
    run = torch.zeros(term.shape[0] + 1, dtype=torch.float64, device=term.device)
    run[1:] = torch.cumsum(term, dim=0)
    before, after = run[:-1], run[1:]
    took = after - before
    lost = torch.zeros_like(run)
    lost[1:] = torch.cumsum((before - (after - took)) + (term - took), dim=0)
    return (run[at[1:]] - run[at[:-1]]) + (lost[at[1:]] - lost[at[:-1]])


class ContourList(collections.namedtuple("ContourList", "splits chain_splits closed p q prim code end")):
    """The contours where planes cut the mesh (Renderer.chainSections / contours): the chains of plane i are splits[i]:splits[i + 1];
    chain c is the records chain_splits[c]:chain_splits[c + 1] of p, q, prim, code and end, in chained order: its vertices are the p
    of its records, plus the last q when it is open.  closed [C] bool; end [M] is each record's exit status (0 = linked to the next
    record of its chain, or, for the last record of a closed chain, to the first; CHAIN_*).  normals: the planes' normals [N, 3]
    where the list came from Renderer.contours, else None."""
    normals = None

    def areas(self, normals=None):
        """float64 [C]: 0.5 * sum dot(n / |n|, cross(p, q)) over each closed chain with the normal n of its plane, NaN for an open
        one.  On a mesh with outward faces a positive area is an outer contour and a negative one a hole.  normals [N, 3] (or
        packed planes [N, 4]): the planes the list was made with; Renderer.contours remembers them.  Summed on the device in
        float64 as Renderer.sectionAreas sums.  Device tensors in the list: a device tensor comes back; else a numpy array."""
        import torch
        nrm = self.normals if normals is None else normals
        if nrm is None:
            raise DrtError(ERR_INVALID, "areas: the list does not know its planes; give their normals [N, 3]")
        as_numpy = isinstance(self.p, np.ndarray)
        dev = torch.device("cuda", torch.cuda.current_device()) if as_numpy else self.p.device
        dev_of = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev) if isinstance(a, np.ndarray) else a.to(dev)
        nrm = dev_of(nrm)[:, 0:3].to(torch.float64)
        splits, chain_splits = dev_of(self.splits).to(torch.int64), dev_of(self.chain_splits).to(torch.int64)
        if nrm.shape[0] != splits.shape[0] - 1:
            raise DrtError(ERR_INVALID, "areas: %d normals for %d planes" % (nrm.shape[0], splits.shape[0] - 1))
        length = torch.sqrt((nrm * nrm).sum(dim=1, keepdim=True))
        unit = torch.where(length > 0, nrm / torch.where(length > 0, length, torch.ones_like(length)), torch.zeros_like(nrm))
        n_chains = chain_splits.shape[0] - 1
        plane_of_chain = torch.repeat_interleave(torch.arange(nrm.shape[0], dtype=torch.int64, device=dev), splits[1:] - splits[:-1])
        owner = torch.repeat_interleave(plane_of_chain, chain_splits[1:] - chain_splits[:-1])
        term = (unit[owner] * torch.linalg.cross(dev_of(self.p).to(torch.float64), dev_of(self.q).to(torch.float64), dim=1)).sum(dim=1)
        areas = 0.5 * _segment_sums(torch, term, chain_splits)
        areas = torch.where(dev_of(self.closed).to(torch.bool), areas, torch.full((n_chains,), float("nan"), dtype=torch.float64, device=dev))
        return areas.cpu().numpy() if as_numpy else areas


class CurveList(collections.namedtuple("CurveList", "chain_splits closed p q query prim code end")):
    """The curves along which a query mesh cuts the scene (Renderer.chainIntersections / intersectionCurves): chain c is the records
    chain_splits[c]:chain_splits[c + 1] of p, q, query, prim, code and end, in chained order over the whole batch -- a curve crosses
    queries: its vertices are the p of its records, plus the last q when it is open.  closed [C] bool; query [M] is the query
    triangle a record belongs to, prim its scene triangle; end [M] is each record's exit status (CHAIN_*; 0 = linked to the next
    record of its chain, or, for the last record of a closed chain, to the first)."""

    def lengths(self):
        """float64 [C]: the sum of |q - p| over each chain, in float64.  Device tensors in the list: a device tensor comes back
        (summed as Renderer.sectionAreas sums); else a numpy array."""
        if isinstance(self.p, np.ndarray):
            d = self.q.astype(np.float64) - self.p.astype(np.float64)
            at = self.chain_splits.astype(np.int64)[:-1]                     # (no chain is empty)
            return np.add.reduceat(np.sqrt((d * d).sum(axis=1)), at) if len(at) else np.zeros(0, np.float64)
        import torch
        d = self.q.to(torch.float64) - self.p.to(torch.float64)
        return _segment_sums(torch, torch.sqrt((d * d).sum(dim=1)), self.chain_splits.to(torch.int64))


class Isosurface(collections.namedtuple("Isosurface", "splits tris cube code")):
    """The triangles of an isosurface (Renderer.isosurface / remesh): row r -- the cubes along x of one (y, z) -- owns the triangles
    splits[r]:splits[r + 1] of tris [M, 3, 3] float32, cube [M] (the linear cube index) and code [M] (tetrahedron | case << 4), both
    int32, in ascending cube, tetrahedron and table order.  Triangle soup: no vertex index buffer; shared vertices are bit-equal, so
    triEdgeAdjacency(tris) recovers the connectivity.  Device tensors (tris a strided view of the 48-byte records) or numpy arrays."""

    def records(self):
        """The packed 48-byte records [M, 12] float32 (drt_iso_tri, laid out as drt_tri), as overlapTriangles, intersectTriangles,
        triangleDistance and triangleCast take them: for device tensors the fill's own output, not a copy."""
        if isinstance(self.tris, np.ndarray):
            rec = np.zeros((len(self.tris), 12), np.float32)
            rec[:, 0:9] = self.tris.reshape(-1, 9)
            rec.view(np.int32)[:, 9], rec.view(np.int32)[:, 10] = self.cube, self.code
            return rec
        import torch
        m = self.tris.shape[0]
        if m and self.tris.stride() == (12, 3, 1):
            return torch.as_strided(self.tris, (m, 12), (12, 1), self.tris.storage_offset())
        rec = torch.zeros((m, 12), dtype=torch.float32, device=self.tris.device)
        rec[:, 0:9] = self.tris.reshape(m, 9)
        rec.view(torch.int32)[:, 9], rec.view(torch.int32)[:, 10] = self.cube, self.code
        return rec

    def faceNormals(self):
        """float32 [M, 3]: cross(v1 - v0, v2 - v0) normalised, zeros for a zero-area triangle.  They point to the side where
        f >= level (away from it with flip).  Face normals only: there are no gradient normals."""
        if isinstance(self.tris, np.ndarray):
            n = np.cross(self.tris[:, 1] - self.tris[:, 0], self.tris[:, 2] - self.tris[:, 0]).astype(np.float32)
            length = np.sqrt((n * n).sum(axis=1, keepdims=True))
            return np.where(length > 0, n / np.where(length > 0, length, 1), 0).astype(np.float32)
        import torch
        n = torch.linalg.cross(self.tris[:, 1] - self.tris[:, 0], self.tris[:, 2] - self.tris[:, 0], dim=1)
        length = torch.sqrt((n * n).sum(dim=1, keepdim=True))
        return torch.where(length > 0, n / torch.where(length > 0, length, torch.ones_like(length)), torch.zeros_like(n))

    def toScene(self, albedo=(0.8, 0.8, 0.8)):
        """A Scene of the triangles (Scene.setGeometry) with face normals at the vertices, zero uvs and one material of `albedo`.
        The caller builds the BVH."""
        host = (lambda a: a) if isinstance(self.tris, np.ndarray) else (lambda a: a.detach().cpu().numpy())
        tris = np.ascontiguousarray(host(self.tris), np.float32)
        nrm = np.repeat(host(self.faceNormals())[:, None, :], 3, axis=1)
        sc = Scene()
        sc.addMaterial(tuple(float(c) for c in albedo))
        sc.setGeometry(tris, nrm, np.zeros((len(tris), 3, 2), np.float32), np.zeros(len(tris), np.int32))
        return sc


NORMAL_WEIGHTS = {"angle": 0, "area": 1}                                # Renderer.vertexNormals: drt.h DRT_NORMALS_*


class IndexedMesh(collections.namedtuple("IndexedMesh", "vertices faces first")):
    """A welded mesh (Renderer.weld / smooth): vertices [V, 3] float32, faces [N, 3] int32 -- the vertex id of every corner -- and first
    [V] int32, the corner 3 t + k at which each vertex first appears.  Vertices are numbered by first appearance.  Device tensors or
    numpy arrays."""

    def triangles(self):
        """float32 [N, 3, 3]: the positions gathered through faces -- triangle soup with bit-equal shared positions again, as every
        other query takes it."""
        if isinstance(self.vertices, np.ndarray):
            return self.vertices[self.faces.astype(np.int64)]
        import torch
        return self.vertices[self.faces.to(torch.int64)]

    def toScene(self, normals=None, albedo=(0.8, 0.8, 0.8)):
        """A Scene of the triangles (Scene.setGeometry), zero uvs and one material of `albedo`.  normals: [V, 3] vertex normals, for
        instance Renderer.vertexNormals(mesh), gathered per corner so that the renderer shades the mesh smooth; None: face normals
        at the vertices, as Isosurface.toScene.  The caller builds the BVH."""
        host = (lambda a: a) if isinstance(self.vertices, np.ndarray) else (lambda a: a.detach().cpu().numpy())
        faces = host(self.faces).astype(np.int64)
        tris = np.ascontiguousarray(host(self.vertices)[faces], np.float32)
        if normals is None:
            nrm = np.repeat(Isosurface(None, tris, None, None).faceNormals()[:, None, :], 3, axis=1)
        else:
            normals = normals if isinstance(normals, np.ndarray) else normals.detach().cpu().numpy()
            if normals.dtype != np.float32 or normals.shape != host(self.vertices).shape:
                raise DrtError(ERR_INVALID, "normals: float32 %s expected" % (tuple(host(self.vertices).shape),))
            nrm = np.ascontiguousarray(normals[faces], np.float32)
        sc = Scene()
        sc.addMaterial(tuple(float(c) for c in albedo))
        sc.setGeometry(tris, nrm, np.zeros((len(tris), 3, 2), np.float32), np.zeros(len(tris), np.int32))
        return sc


class MeshEdges(collections.namedtuple("MeshEdges", "adj edge half_edge count")):
    """Renderer.edgeAdjacency(mesh, edges=True): adj [N, 3] int32, the twin of every half-edge (-1 boundary, -2 every other case);
    edge [N, 3] int32, the undirected edge of every half-edge, numbered by first appearance, -1 for a zero-length one; half_edge [E]
    int32, the smallest half-edge of every edge; count = E.  Device tensors or numpy arrays."""

    def euler(self, n_vertices):
        """V - E + F: 2 per closed surface of genus 0."""
        return int(n_vertices) - int(self.count) + int(self.adj.shape[0])


SIMPLIFY_PLACEMENTS = {"mean": 0, "quadric": 1}                         # Renderer.simplify: drt.h DRT_SIMPLIFY_*


class SimplifiedMesh(collections.namedtuple("SimplifiedMesh", "vertices faces first cluster source")):
    """A simplified mesh (Renderer.simplify): vertices [C, 3] float32, one per cluster; faces [M, 3] int32, the cluster ids of the
    surviving triangles in input order; first [C] int32, the smallest input vertex of each cluster; cluster [V] int32, the cluster id
    of every input vertex; source [M] int32, the input triangle of every output triangle.  The first three fields are an
    IndexedMesh's, so vertexNormals, smooth and toScene(normals=) take it unchanged.  Device tensors or numpy arrays."""

    triangles = IndexedMesh.triangles
    toScene = IndexedMesh.toScene


SUBDIVIDE_SCHEMES = {"midpoint": 0, "loop": 1}                           # Renderer.subdivide: drt.h DRT_SUBDIVIDE_*


class SubdividedMesh(collections.namedtuple("SubdividedMesh", "vertices faces parents")):
    """A subdivided mesh (Renderer.subdivide): vertices [V', 3] float32 -- the input's V vertices under their old ids, then one per
    undirected edge, numbered by first appearance; faces [4 N, 3] int32, the four children of input triangle t at 4 t ... 4 t + 3
    (child k < 3 starts at corner k, the last is the middle one); parents [V', 2] int32 of the last level: (v, v) for a vertex that
    was there before, the two ends of its edge for a new one, so per-vertex attributes can follow (None with levels=0).  The first
    two fields are an IndexedMesh's, so vertexNormals, smooth, simplify, edgeAdjacency, subdivide and toScene(normals=) take it
    unchanged.  Device tensors or numpy arrays."""

    triangles = IndexedMesh.triangles
    toScene = IndexedMesh.toScene


def triEdgeAdjacency(tris):
    """int32 [N, 3]: the edge adjacency of a query mesh (drt_tri_edge_adjacency), Scene.edgeAdjacency's rule on the vertices of
    tris -- [N, 3, 3] float32 or a packed [N, 12] (drt_tri) -- in the caller's order: the twin half-edge 3 * i' + e' of edge e (vertex e
    to vertex (e + 1) % 3) of triangle i by bit-equal positions, -1 on a boundary edge, -2 where the edge is non-manifold, flipped or
    of zero length.  What Renderer.chainIntersections takes as query_adj.  The table is made on the host: numpy in, numpy out; a
    device tensor is copied to the host for it, and a device tensor comes back.  Renderer.edgeAdjacency makes the same bytes on
    the device, in milliseconds where this sorts for a second, and takes index buffers as well."""
    as_numpy = isinstance(tris, np.ndarray)
    if as_numpy:
        host = tris
    else:
        import torch                             # (only here: importing the package does not import torch)
        if not torch.is_tensor(tris):
            raise DrtError(ERR_INVALID, "tris: a numpy array or a torch tensor expected")
        host = tris.detach().cpu().numpy()
    if host.dtype != np.float32:
        raise DrtError(ERR_INVALID, "tris: dtype %s, float32 expected" % host.dtype)
    if host.ndim == 3 and host.shape[1:] == (3, 3):
        packed = np.zeros((host.shape[0], 12), np.float32)
        packed[:, 0:9] = host.reshape(-1, 9)
    elif host.ndim == 2 and host.shape[1] == 12:
        packed = np.ascontiguousarray(host)
    else:
        raise DrtError(ERR_INVALID, "tris: shape %s, [N, 3, 3] or a packed [N, 12] expected" % (tuple(host.shape),))
    n = packed.shape[0]
    if n >= 2 ** 31:
        raise DrtError(ERR_INVALID, "%d triangles: fewer than 2^31 expected" % n)
    out = np.zeros((n, 3), np.int32)
    _check(_lib.drt_tri_edge_adjacency(packed.ctypes.data if n else None, n, out.ctypes.data if n else None, 3 * n))
    return out if as_numpy else torch.from_numpy(out).to(tris.device)
# Mesh topology (drt.h "mesh topology"), everything in tree order (Scene.triangleOrder() maps it to load order)
Shells = collections.namedtuple("Shells", "label index count triangles open_edges bad_edges watertight")   # Renderer.shells
LoopList = collections.namedtuple("LoopList", "splits closed half_edge prim edge shell end")              # Renderer.boundaryLoops
ShellMeasures = collections.namedtuple("ShellMeasures", "area volume area_vector")                        # Renderer.shellMeasures
INSIDE_RULES = {"parity": 0, "winding": 1}                             # Renderer.inside / signedDistance: drt.h DRT_INSIDE_*
TemporalHistory = collections.namedtuple("TemporalHistory", "color length moments variance weight")  # Renderer.GetTemporalHistory
Guides = collections.namedtuple("Guides", "albedo normal t prim")  # first-hit guide buffers (Renderer.renderGuides)
AdaptiveState = collections.namedtuple("AdaptiveState", "sum count m1 m2 last_q last_count")  # Renderer.GetAdaptiveState


def _ray_batch(torch, dev, origins, directions, tmin, tmax):
    """(rays [N, 8] float32 on `dev`, came_from_numpy).  Raises DrtError(ERR_INVALID) on a wrong dtype, shape or device."""
    def bad(msg):
        return DrtError(ERR_INVALID, msg)

    def as_tensor(a, what, shape_tail):
        if isinstance(a, np.ndarray):
            if a.dtype != np.float32:
                raise bad("%s: dtype %s, float32 expected" % (what, a.dtype))
            t = torch.from_numpy(np.ascontiguousarray(a))
        elif torch.is_tensor(a):
            if a.dtype != torch.float32:
                raise bad("%s: dtype %s, torch.float32 expected" % (what, a.dtype))
            if a.device != dev:
                raise bad("%s: on %s, the renderer is on %s" % (what, a.device, dev))
            t = a
        else:
            raise bad("%s: a numpy array or a torch tensor expected" % what)
        if t.dim() != 1 + len(shape_tail) or tuple(t.shape[1:]) != shape_tail:
            raise bad("%s: shape %s, [N%s] expected" % (what, tuple(t.shape), "".join(", %d" % d for d in shape_tail)))
        return t

    first = origins
    from_numpy = isinstance(first, np.ndarray)
    if directions is None:
        rays = as_tensor(origins, "rays", (8,))
        parts = [rays]
    else:
        org, dirs = as_tensor(origins, "origins", (3,)), as_tensor(directions, "directions", (3,))
        if org.shape[0] != dirs.shape[0]:
            raise bad("origins and directions hold %d and %d rays" % (org.shape[0], dirs.shape[0]))
        parts = [org, dirs]
    n = parts[0].shape[0]
    interval = []
    for name, v in (("tmin", tmin), ("tmax", tmax)):
        if v is None or isinstance(v, (int, float, np.floating, np.integer)):
            interval.append(v)
        else:
            t = as_tensor(v, name, ())
            if t.shape[0] != n:
                raise bad("%s holds %d values for %d rays" % (name, t.shape[0], n))
            interval.append(t)
            parts.append(t)
    if len({isinstance(p, np.ndarray) for p in (origins, directions, tmin, tmax) if isinstance(p, np.ndarray) or torch.is_tensor(p)}) > 1:
        raise bad("mix of numpy arrays and device tensors")
    if from_numpy:
        parts = [p.to(dev) for p in parts]
    if directions is None:
        rays = parts[0]
        if interval[0] is not None or interval[1] is not None:
            raise bad("packed rays carry their own tmin / tmax")
        if not rays.is_contiguous() or rays.data_ptr() % 16:
            rays = rays.contiguous().clone()
        return rays, from_numpy
    org, dirs = parts[0], parts[1]
    rest = iter(parts[2:])
    rays = torch.empty((n, 8), dtype=torch.float32, device=dev)       # packed on the device, on the current stream
    rays[:, 0:3] = org
    rays[:, 4:7] = dirs
    for col, v in ((3, interval[0]), (7, interval[1])):
        rays[:, col] = next(rest) if torch.is_tensor(v) or isinstance(v, np.ndarray) else float(v)
    return rays, from_numpy


def _point_batch(torch, dev, points, max_dist):
    """(points [N, 4] float32 (p, max_dist) on `dev`, 16-byte aligned, came_from_numpy).  Raises DrtError(ERR_INVALID) on a wrong
    dtype, shape or device."""
    def bad(msg):
        return DrtError(ERR_INVALID, msg)

    def as_tensor(a, what):
        if isinstance(a, np.ndarray):
            if a.dtype != np.float32:
                raise bad("%s: dtype %s, float32 expected" % (what, a.dtype))
            return torch.from_numpy(np.ascontiguousarray(a))
        if torch.is_tensor(a):
            if a.dtype != torch.float32:
                raise bad("%s: dtype %s, torch.float32 expected" % (what, a.dtype))
            if a.device != dev:
                raise bad("%s: on %s, the renderer is on %s" % (what, a.device, dev))
            return a
        raise bad("%s: a numpy array or a torch tensor expected" % what)

    from_numpy = isinstance(points, np.ndarray)
    pts = as_tensor(points, "points")
    if pts.dim() != 2 or pts.shape[1] not in (3, 4):
        raise bad("points: shape %s, [N, 3] or [N, 4] expected" % (tuple(pts.shape),))
    n = pts.shape[0]
    per_point = not isinstance(max_dist, (int, float, np.floating, np.integer))
    if pts.shape[1] == 4:
        if per_point or float(max_dist) != float("inf"):
            raise bad("packed points carry their own max_dist")
        packed = pts.to(dev) if from_numpy else pts
        if not packed.is_contiguous() or packed.data_ptr() % 16:
            packed = packed.contiguous().clone()
    else:
        if per_point:
            if isinstance(max_dist, np.ndarray) != from_numpy:
                raise bad("mix of numpy arrays and device tensors")
            md = as_tensor(max_dist, "max_dist")
            if md.dim() != 1 or md.shape[0] != n:
                raise bad("max_dist: shape %s for %d points" % (tuple(md.shape), n))
        packed = torch.empty((n, 4), dtype=torch.float32, device=dev)     # packed on the device, on the current stream
        packed[:, 0:3] = pts.to(dev) if from_numpy else pts
        packed[:, 3] = (md.to(dev) if from_numpy else md) if per_point else float(max_dist)
    return packed, from_numpy


def _tri_batch(torch, dev, tris):
    """(triangles [N, 12] float32 (drt_tri: v[3][3], three pad words) on `dev`, 16-byte aligned, came_from_numpy) from vertices
    [N, 3, 3] or a packed [N, 12].  Raises DrtError(ERR_INVALID) on a wrong dtype, shape or device, as _box_batch does."""
    def bad(msg):
        return DrtError(ERR_INVALID, msg)

    if isinstance(tris, np.ndarray):
        if tris.dtype != np.float32:
            raise bad("tris: dtype %s, float32 expected" % tris.dtype)
        t, from_numpy = torch.from_numpy(np.ascontiguousarray(tris)), True
    elif torch.is_tensor(tris):
        if tris.dtype != torch.float32:
            raise bad("tris: dtype %s, torch.float32 expected" % tris.dtype)
        if tris.device != dev:
            raise bad("tris: on %s, the renderer is on %s" % (tris.device, dev))
        t, from_numpy = tris, False
    else:
        raise bad("tris: a numpy array or a torch tensor expected")
    shape = tuple(t.shape)
    if len(shape) == 2 and shape[1] == 12:
        packed = t.to(dev) if from_numpy else t
        if not packed.is_contiguous() or packed.data_ptr() % 16:
            packed = packed.contiguous().clone()
        return packed, from_numpy
    if len(shape) != 3 or shape[1:] != (3, 3):
        raise bad("tris: shape %s, [N, 3, 3] or a packed [N, 12] expected" % (shape,))
    packed = torch.zeros((shape[0], 12), dtype=torch.float32, device=dev)     # packed on the device, on the current stream
    packed[:, 0:9] = (t.to(dev) if from_numpy else t).reshape(shape[0], 9)
    return packed, from_numpy


def _plane_batch(torch, dev, normals, d):
    """(planes [N, 4] float32 (drt_plane: n, d) on `dev`, 16-byte aligned, came_from_numpy) from normals [N, 3] + d [N] or a packed
    [N, 4].  Raises DrtError(ERR_INVALID) on a wrong dtype, shape or device, as _box_batch does."""
    def bad(msg):
        return DrtError(ERR_INVALID, msg)

    def as_tensor(a, what):
        if isinstance(a, np.ndarray):
            if a.dtype != np.float32:
                raise bad("%s: dtype %s, float32 expected" % (what, a.dtype))
            return torch.from_numpy(np.ascontiguousarray(a))
        if torch.is_tensor(a):
            if a.dtype != torch.float32:
                raise bad("%s: dtype %s, torch.float32 expected" % (what, a.dtype))
            if a.device != dev:
                raise bad("%s: on %s, the renderer is on %s" % (what, a.device, dev))
            return a
        raise bad("%s: a numpy array or a torch tensor expected" % what)

    from_numpy = isinstance(normals, np.ndarray)
    nrm = as_tensor(normals, "normals")
    if nrm.dim() != 2 or nrm.shape[1] not in (3, 4):
        raise bad("normals: shape %s, [N, 3] or a packed [N, 4] expected" % (tuple(nrm.shape),))
    if nrm.shape[1] == 4:
        if d is not None:
            raise bad("packed planes carry their own d")
        packed = nrm.to(dev) if from_numpy else nrm
        if not packed.is_contiguous() or packed.data_ptr() % 16:
            packed = packed.contiguous().clone()
        return packed, from_numpy
    if d is None:
        raise bad("planes: normals [N, 3] and d [N], or a packed [N, 4] expected")
    if isinstance(d, np.ndarray) != from_numpy:
        raise bad("mix of numpy arrays and device tensors")
    dd = as_tensor(d, "d")
    if dd.dim() != 1 or dd.shape[0] != nrm.shape[0]:
        raise bad("d: shape %s for %d planes" % (tuple(dd.shape), nrm.shape[0]))
    packed = torch.empty((nrm.shape[0], 4), dtype=torch.float32, device=dev)      # packed on the device, on the current stream
    packed[:, 0:3] = nrm.to(dev) if from_numpy else nrm
    packed[:, 3] = dd.to(dev) if from_numpy else dd
    return packed, from_numpy


def _box_batch(torch, dev, center, half, axes, lo, hi):
    """(boxes [N, 16] float32 (drt_box: center, half, axis[3][3], pad) on `dev`, 16-byte aligned, came_from_numpy) from center [N, 3]
    + half [N, 3] (+ axes [N, 3, 3], default the identity), from a packed [N, 16], or from lo [N, 3] + hi [N, 3]
    (center = (lo + hi) / 2, half = (hi - lo) / 2 in float32).  Raises DrtError(ERR_INVALID) on a wrong dtype, shape or device."""
    def bad(msg):
        return DrtError(ERR_INVALID, msg)

    def as_tensor(a, what, tail):
        if isinstance(a, np.ndarray):
            if a.dtype != np.float32:
                raise bad("%s: dtype %s, float32 expected" % (what, a.dtype))
            t = torch.from_numpy(np.ascontiguousarray(a))
        elif torch.is_tensor(a):
            if a.dtype != torch.float32:
                raise bad("%s: dtype %s, torch.float32 expected" % (what, a.dtype))
            if a.device != dev:
                raise bad("%s: on %s, the renderer is on %s" % (what, a.device, dev))
            t = a
        else:
            raise bad("%s: a numpy array or a torch tensor expected" % what)
        if t.dim() != 1 + len(tail) or tuple(t.shape[1:]) != tail:
            raise bad("%s: shape %s, [N%s] expected" % (what, tuple(t.shape), "".join(", %d" % d for d in tail)))
        return t

    corners = lo is not None or hi is not None
    if corners and (lo is None or hi is None or center is not None or half is not None):
        raise bad("boxes: lo= and hi= come together and without center / half")
    if not corners and center is None:
        raise bad("boxes: center and half, a packed [N, 16] or lo= and hi= expected")
    given = [a for a in (center, half, axes, lo, hi) if a is not None]
    if len({isinstance(a, np.ndarray) for a in given}) > 1:
        raise bad("mix of numpy arrays and device tensors")
    from_numpy = isinstance(given[0], np.ndarray)
    up = (lambda t: t.to(dev)) if from_numpy else (lambda t: t)
    if not corners and half is None:
        packed = up(as_tensor(center, "boxes", (16,)))
        if axes is not None:
            raise bad("packed boxes carry their own axes")
        if not packed.is_contiguous() or packed.data_ptr() % 16:
            packed = packed.contiguous().clone()
        return packed, from_numpy
    if corners:
        a, b = up(as_tensor(lo, "lo", (3,))), up(as_tensor(hi, "hi", (3,)))
        if a.shape[0] != b.shape[0]:
            raise bad("lo and hi hold %d and %d boxes" % (a.shape[0], b.shape[0]))
        c, h = (a + b) / 2, (b - a) / 2
    else:
        c, h = up(as_tensor(center, "center", (3,))), up(as_tensor(half, "half", (3,)))
        if c.shape[0] != h.shape[0]:
            raise bad("center and half hold %d and %d boxes" % (c.shape[0], h.shape[0]))
    n = c.shape[0]
    packed = torch.zeros((n, 16), dtype=torch.float32, device=dev)        # packed on the device, on the current stream
    packed[:, 0:3], packed[:, 3:6] = c, h
    if axes is None:
        packed[:, 6], packed[:, 10], packed[:, 14] = 1.0, 1.0, 1.0
    else:
        ax = up(as_tensor(axes, "axes", (3, 3)))
        if ax.shape[0] != n:
            raise bad("axes hold %d boxes, center %d" % (ax.shape[0], n))
        packed[:, 6:15] = ax.reshape(n, 9)
    return packed, from_numpy


class Renderer:
    """Core/Renderer.hpp:14-47."""

    def __init__(self, device=0):
        self._h = _lib.drt_renderer_create(device)
        if not self._h:
            raise DrtError(ERR_DEVICE, (_lib.drt_last_error() or b"").decode())
        self._device = device
        self.m_RendererSettings = RendererSettings()
        self.m_LastDenoiseMs = 0.0               # device time of the last Denoise (guides + filter)
        self.m_LastTemporalMs = 0.0              # device time of the last TemporalDenoise (guides + reprojection + filter)
        self.m_LastUpscaleMs = 0.0               # device time of the last Upscale (both guide passes + the kernel)
        self._upscaled_size = (0, 0)             # (width, height) of the last Upscale
        self.m_LastAdaptiveMs = 0.0              # device time of the last RenderAdaptive (plan + ray lists + tracing + fold)

    def _ray_query(self, scene, origins, directions, tmin, tmax, occluded):
        import torch                             # (only here: importing the package does not import torch)
        dev = torch.device("cuda", self._device)
        rays, from_numpy = _ray_batch(torch, dev, origins, directions, tmin, tmax)
        n = rays.shape[0]
        if occluded:
            out = torch.empty(n, dtype=torch.uint8, device=dev)
            fn = _lib.drt_renderer_occluded
        else:
            out = torch.empty((n, 4), dtype=torch.float32, device=dev)
            fn = _lib.drt_renderer_trace_rays
        if n:
            stream = torch.cuda.current_stream(dev).cuda_stream
            _check(fn(self._h, scene._h, rays.data_ptr(), out.data_ptr(), n, stream))
        if occluded:
            res = out.view(torch.bool)
            return res.cpu().numpy() if from_numpy else res
        if from_numpy:
            h = out.cpu().numpy()
            return RayHits(h[:, 0].copy(), h.view(np.int32)[:, 1].copy(), h[:, 2].copy(), h[:, 3].copy())
        return RayHits(out[:, 0], out.view(torch.int32)[:, 1], out[:, 2], out[:, 3])

    def traceRays(self, scene, origins, directions=None, tmin=0.0, tmax=FLT_MAX):
        """Closest hit of every ray (drt_renderer_trace_rays): RayHits(t, prim, u, v), prim -1 = miss (then t = tmax).
        origins / directions [N, 3] float32, or origins = packed rays [N, 8] (org, tmin, dir, tmax) and directions None;
        tmin / tmax scalars or [N] arrays.  Device tensors in, device tensors out (enqueued on the current torch stream);
        numpy in, numpy out."""
        if directions is None and (tmin, tmax) == (0.0, FLT_MAX):
            tmin = tmax = None
        return self._ray_query(scene, origins, directions, tmin, tmax, False)

    def occluded(self, scene, origins, directions=None, tmin=0.0, tmax=float("inf")):
        """Whether anything lies on each ray within (tmin, tmax) (drt_renderer_occluded): bool [N].  Arguments as traceRays."""
        if directions is None and tmin == 0.0 and tmax == float("inf"):
            tmin = tmax = None
        return self._ray_query(scene, origins, directions, tmin, tmax, True)

    def nearest(self, scene, points, max_dist=float("inf")):
        """The closest point of the mesh for every point (drt_renderer_nearest): Nearest(point [N, 3], d2, prim, u, v, side), prim -1 =
        nothing within max_dist (then point = 0, d2 = max_dist^2).  points [N, 3] float32 with max_dist a scalar or [N], or packed
        [N, 4] (p, max_dist).  Device tensors in, device tensors out (enqueued on the current torch stream); numpy in, numpy out.
        After refit(scene, positions) the moved geometry is the one queried."""
        import torch                             # (only here: importing the package does not import torch)
        dev = torch.device("cuda", self._device)
        packed, from_numpy = _point_batch(torch, dev, points, max_dist)
        n = packed.shape[0]
        out = torch.empty((n, 8), dtype=torch.float32, device=dev)
        if n:
            stream = torch.cuda.current_stream(dev).cuda_stream
            _check(_lib.drt_renderer_nearest(self._h, scene._h, packed.data_ptr(), out.data_ptr(), n, stream))
        if from_numpy:
            h = out.cpu().numpy()
            return Nearest(h[:, 0:3].copy(), h[:, 3].copy(), h.view(np.int32)[:, 4].copy(), h[:, 5].copy(), h[:, 6].copy(), h[:, 7].copy())
        return Nearest(out[:, 0:3], out[:, 3], out.view(torch.int32)[:, 4], out[:, 5], out[:, 6], out[:, 7])

    def sphereCast(self, scene, origins, directions=None, radius=0.0, tmin=0.0, tmax=float("inf")):
        """The first contact of a sphere moving along each ray with the mesh (drt_renderer_sphere_cast): SphereHits(t, prim, u, v,
        point [N, 3], feature), prim -1 = no contact in [tmin, tmax) (then t = tmax, feature = -1).  The centre at t is origin +
        direction t; feature 0 = face, 1..3 = edges, 4..6 = vertices, + 8 when the sphere already overlapped at tmin.  radius is a
        scalar or [N].  Other arguments as crossings.  After refit(scene, positions) the moved geometry is the one queried."""
        import torch                             # (only here: importing the package does not import torch)
        dev = torch.device("cuda", self._device)
        if directions is None and tmin == 0.0 and tmax == float("inf"):
            tmin = tmax = None
        rays, from_numpy = _ray_batch(torch, dev, origins, directions, tmin, tmax)
        n = rays.shape[0]
        if isinstance(radius, (int, float, np.floating, np.integer)):
            radii = torch.full((n,), float(radius), dtype=torch.float32, device=dev)
        else:
            if not (isinstance(radius, np.ndarray) or torch.is_tensor(radius)):
                raise DrtError(ERR_INVALID, "radius: a number, a numpy array or a torch tensor expected")
            if isinstance(radius, np.ndarray) != from_numpy:
                raise DrtError(ERR_INVALID, "mix of numpy arrays and device tensors")
            if radius.dtype != (np.float32 if from_numpy else torch.float32):
                raise DrtError(ERR_INVALID, "radius: dtype %s, float32 expected" % (radius.dtype,))
            if not from_numpy and radius.device != dev:
                raise DrtError(ERR_INVALID, "radius: on %s, the renderer is on %s" % (radius.device, dev))
            if len(radius.shape) != 1 or radius.shape[0] != n:
                raise DrtError(ERR_INVALID, "radius: shape %s for %d rays" % (tuple(radius.shape), n))
            radii = torch.from_numpy(np.ascontiguousarray(radius)).to(dev) if from_numpy else radius.contiguous()
        out = torch.empty((n, 8), dtype=torch.float32, device=dev)
        if n:
            stream = torch.cuda.current_stream(dev).cuda_stream
            _check(_lib.drt_renderer_sphere_cast(self._h, scene._h, rays.data_ptr(), radii.data_ptr(), out.data_ptr(), n, stream))
        if from_numpy:
            h = out.cpu().numpy()
            i = h.view(np.int32)
            return SphereHits(h[:, 0].copy(), i[:, 1].copy(), h[:, 2].copy(), h[:, 3].copy(), h[:, 4:7].copy(), i[:, 7].copy())
        i = out.view(torch.int32)
        return SphereHits(out[:, 0], i[:, 1], out[:, 2], out[:, 3], out[:, 4:7], i[:, 7])

    def crossings(self, scene, origins, directions=None, tmin=0.0, tmax=float("inf")):
        """Every triangle each ray passes through within (tmin, tmax) (drt_renderer_crossings): Crossings(count uint32 [N], winding
        int32 [N]), winding = exits minus entries by the triangles' own winding.  Alpha cut-outs are ignored.  Arguments as traceRays."""
        import torch                             # (only here: importing the package does not import torch)
        dev = torch.device("cuda", self._device)
        if directions is None and tmin == 0.0 and tmax == float("inf"):
            tmin = tmax = None
        rays, from_numpy = _ray_batch(torch, dev, origins, directions, tmin, tmax)
        n = rays.shape[0]
        out = torch.empty((n, 2), dtype=torch.int32, device=dev)
        if n:
            stream = torch.cuda.current_stream(dev).cuda_stream
            _check(_lib.drt_renderer_crossings(self._h, scene._h, rays.data_ptr(), out.data_ptr(), n, stream))
        if from_numpy:
            h = out.cpu().numpy()
            return Crossings(h[:, 0].copy().view(np.uint32), h[:, 1].copy())
        return Crossings(out[:, 0], out[:, 1])       # (torch has no uint32 arithmetic: count is an int32 tensor, < 2^31 triangles)

    def firstHits(self, scene, origins, directions=None, tmin=0.0, tmax=float("inf"), k=4):
        """The first k triangles each ray passes through within (tmin, tmax), in order of (t, prim) (drt_renderer_list_hits with
        k slots per ray): FirstHits(t [N, k], prim [N, k] int32, u [N, k], v [N, k], count [N] int32).  Slots beyond a ray's hits hold
        the miss record (t = tmax, prim = -1, u = v = 0); count is ALL the triangles the ray passes through, crossings' count, so
        count > k tells a truncated row.  Alpha cut-outs are ignored.  Arguments as crossings."""
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
            raise DrtError(ERR_INVALID, "k = %r: a positive integer expected" % (k,))
        k = int(k)
        shape = getattr(origins, "shape", None)
        if shape is not None and len(shape) >= 1 and int(shape[0]) * k >= 2 ** 31:
            raise DrtError(ERR_INVALID, "%d rays x %d slots: fewer than 2^31 records expected" % (int(shape[0]), k))
        import torch                             # (only here: importing the package does not import torch)
        dev = torch.device("cuda", self._device)
        if directions is None and tmin == 0.0 and tmax == float("inf"):
            tmin = tmax = None
        rays, from_numpy = _ray_batch(torch, dev, origins, directions, tmin, tmax)
        n = rays.shape[0]
        hits = torch.empty((n, k, 4), dtype=torch.float32, device=dev)
        count = torch.empty(n, dtype=torch.int32, device=dev)
        if n:
            offsets = (torch.arange(n + 1, dtype=torch.int64, device=dev) * k).to(torch.int32)
            stream = torch.cuda.current_stream(dev).cuda_stream
            _check(_lib.drt_renderer_list_hits(self._h, scene._h, rays.data_ptr(), offsets.data_ptr(), hits.data_ptr(), n * k,
                                               count.data_ptr(), n, stream))
        if from_numpy:
            h = hits.cpu().numpy()
            return FirstHits(h[..., 0].copy(), h.view(np.int32)[..., 1].copy(), h[..., 2].copy(), h[..., 3].copy(), count.cpu().numpy())
        return FirstHits(hits[..., 0], hits.view(torch.int32)[..., 1], hits[..., 2], hits[..., 3], count)

    def listHits(self, scene, origins, directions=None, tmin=0.0, tmax=float("inf")):
        """Every triangle each ray passes through within (tmin, tmax), in order of (t, prim): HitList(splits [N + 1] int32, t, prim
        int32, u, v), ray i's hits at [splits[i], splits[i + 1]).  Two passes: drt_renderer_crossings counts, a cumulative sum on the
        device gives splits, and drt_renderer_list_hits fills.  The total is read back between them to size the result: that read is
        this call's one synchronisation with the device.  Alpha cut-outs are ignored.  Arguments as crossings."""
        import torch                             # (only here: importing the package does not import torch)
        dev = torch.device("cuda", self._device)
        if directions is None and tmin == 0.0 and tmax == float("inf"):
            tmin = tmax = None
        rays, from_numpy = _ray_batch(torch, dev, origins, directions, tmin, tmax)
        n = rays.shape[0]
        splits = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        total = 0
        if n:
            stream = torch.cuda.current_stream(dev).cuda_stream
            crossed = torch.empty((n, 2), dtype=torch.int32, device=dev)
            _check(_lib.drt_renderer_crossings(self._h, scene._h, rays.data_ptr(), crossed.data_ptr(), n, stream))
            splits[1:] = torch.cumsum(crossed[:, 0].to(torch.int64), dim=0)
            total = int(splits[-1].item())       # the one synchronisation: the result's size
            if total >= 2 ** 31:
                raise DrtError(ERR_INVALID, "%d hits in all: fewer than 2^31 expected (split the rays)" % total)
        splits = splits.to(torch.int32)
        hits = torch.empty((total, 4), dtype=torch.float32, device=dev)
        if total:
            _check(_lib.drt_renderer_list_hits(self._h, scene._h, rays.data_ptr(), splits.data_ptr(), hits.data_ptr(), total, None, n, stream))
        if from_numpy:
            h = hits.cpu().numpy()
            return HitList(splits.cpu().numpy(), h[:, 0].copy(), h.view(np.int32)[:, 1].copy(), h[:, 2].copy(), h[:, 3].copy())
        return HitList(splits, hits[:, 0], hits.view(torch.int32)[:, 1], hits[:, 2], hits[:, 3])

    def kNearest(self, scene, points, k=4, max_dist=float("inf")):
        """The k nearest triangles of every point within max_dist, in order of (d2, prim) (drt_renderer_nearest_list in mode
        DRT_NEAR_K with k slots per point): KNearest(d2 [N, k], prim [N, k] int32, u [N, k], v [N, k], point [N, k, 3], side [N, k],
        count [N] int32).  Slots beyond a point's list hold the miss record (d2 = max_dist^2, prim = -1, u = v = 0, point = 0,
        side = 0); count is the number stored.  Alpha cut-outs are ignored.  Arguments as nearest."""
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
            raise DrtError(ERR_INVALID, "k = %r: a positive integer expected" % (k,))
        k = int(k)
        shape = getattr(points, "shape", None)
        if shape is not None and len(shape) >= 1 and int(shape[0]) * k >= 2 ** 31:
            raise DrtError(ERR_INVALID, "%d points x %d slots: fewer than 2^31 records expected" % (int(shape[0]), k))
        import torch                             # (only here: importing the package does not import torch)
        dev = torch.device("cuda", self._device)
        packed, from_numpy = _point_batch(torch, dev, points, max_dist)
        n = packed.shape[0]
        near = torch.empty((n, k, 4), dtype=torch.float32, device=dev)
        surf = torch.empty((n, k, 4), dtype=torch.float32, device=dev)
        count = torch.empty(n, dtype=torch.int32, device=dev)
        if n:
            offsets = (torch.arange(n + 1, dtype=torch.int64, device=dev) * k).to(torch.int32)
            stream = torch.cuda.current_stream(dev).cuda_stream
            _check(_lib.drt_renderer_nearest_list(self._h, scene._h, packed.data_ptr(), offsets.data_ptr(), near.data_ptr(), surf.data_ptr(),
                                                  n * k, count.data_ptr(), n, NEAR_K, stream))
        if from_numpy:
            h, s = near.cpu().numpy(), surf.cpu().numpy()
            return KNearest(h[..., 0].copy(), h.view(np.int32)[..., 1].copy(), h[..., 2].copy(), h[..., 3].copy(), s[..., 0:3].copy(),
                            s[..., 3].copy(), count.cpu().numpy())
        return KNearest(near[..., 0], near.view(torch.int32)[..., 1], near[..., 2], near[..., 3], surf[..., 0:3], surf[..., 3], count)

    def withinRadius(self, scene, points, radius):
        """Every triangle within `radius` of each point, in order of (d2, prim): NearList(splits [N + 1] int32, d2, prim int32, u, v,
        point [M, 3], side), point i's triangles at [splits[i], splits[i + 1]).  Two passes of drt_renderer_nearest_list in mode
        DRT_NEAR_GATHER: a count with capacity 0, a cumulative sum on the device gives splits, and a fill.  The total is read back
        between them to size the result: that read is this call's one synchronisation with the device.  Alpha cut-outs are ignored.
        points and radius as nearest's points and max_dist."""
        import torch                             # (only here: importing the package does not import torch)
        dev = torch.device("cuda", self._device)
        packed, from_numpy = _point_batch(torch, dev, points, radius)
        n = packed.shape[0]
        splits = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        total = 0
        if n:
            stream = torch.cuda.current_stream(dev).cuda_stream
            counts = torch.empty(n, dtype=torch.int32, device=dev)
            no_room = torch.zeros(n + 1, dtype=torch.int32, device=dev)       # capacity 0: every segment is empty
            _check(_lib.drt_renderer_nearest_list(self._h, scene._h, packed.data_ptr(), no_room.data_ptr(), None, None, 0, counts.data_ptr(),
                                                  n, NEAR_GATHER, stream))
            splits[1:] = torch.cumsum(counts.to(torch.int64), dim=0)
            total = int(splits[-1].item())       # the one synchronisation: the result's size
            if total >= 2 ** 31:
                raise DrtError(ERR_INVALID, "%d triangles in all: fewer than 2^31 expected (split the points)" % total)
        splits = splits.to(torch.int32)
        near = torch.empty((total, 4), dtype=torch.float32, device=dev)
        surf = torch.empty((total, 4), dtype=torch.float32, device=dev)
        if total:
            _check(_lib.drt_renderer_nearest_list(self._h, scene._h, packed.data_ptr(), splits.data_ptr(), near.data_ptr(), surf.data_ptr(),
                                                  total, None, n, NEAR_GATHER, stream))
        if from_numpy:
            h, s = near.cpu().numpy(), surf.cpu().numpy()
            return NearList(splits.cpu().numpy(), h[:, 0].copy(), h.view(np.int32)[:, 1].copy(), h[:, 2].copy(), h[:, 3].copy(),
                            s[:, 0:3].copy(), s[:, 3].copy())
        return NearList(splits, near[:, 0], near.view(torch.int32)[:, 1], near[:, 2], near[:, 3], surf[:, 0:3], surf[:, 3])

    def overlapBoxes(self, scene, center=None, half=None, axes=None, k=None, lo=None, hi=None):
        """The triangles that touch each query box, in ascending triangle index (drt_renderer_overlap_boxes in mode
        DRT_OVERLAP_LIST).  Boxes: center [N, 3] + half [N, 3] (+ axes [N, 3, 3], axes[i, j] the world direction of box i's axis j,
        used as given; default axis-aligned), or a packed [N, 16] (drt_box), or lo= / hi= [N, 3] corners
        (center = (lo + hi) / 2, half = (hi - lo) / 2 in float32).  Touching counts; alpha cut-outs are ignored.
        k=None: BoxList(splits [N + 1] int32, prim [M] int32), box i's triangles at [splits[i], splits[i + 1]) -- a count with
        capacity 0, a cumulative sum on the device, and a fill; the total is read back between them to size the result: that read
        is this call's one synchronisation with the device.  k=K: BoxTable(prim [N, K] int32, count [N] int32) in one pass: the
        first K of each list, -1 behind a shorter one; count is the number listed, stored or not.  Device tensors in, device
        tensors out (enqueued on the current torch stream); numpy in, numpy out."""
        if k is not None and (isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1):
            raise DrtError(ERR_INVALID, "k = %r: a positive integer or None expected" % (k,))
        import torch                             # (only here: importing the package does not import torch)
        dev = torch.device("cuda", self._device)
        boxes, from_numpy = _box_batch(torch, dev, center, half, axes, lo, hi)
        n = boxes.shape[0]
        host = (lambda t: t.cpu().numpy()) if from_numpy else (lambda t: t)
        if k is not None:
            k = int(k)
            if n * k >= 2 ** 31:
                raise DrtError(ERR_INVALID, "%d boxes x %d slots: fewer than 2^31 records expected" % (n, k))
            prim = torch.empty((n, k), dtype=torch.int32, device=dev)
            count = torch.empty(n, dtype=torch.int32, device=dev)
            if n:
                offsets = (torch.arange(n + 1, dtype=torch.int64, device=dev) * k).to(torch.int32)
                stream = torch.cuda.current_stream(dev).cuda_stream
                _check(_lib.drt_renderer_overlap_boxes(self._h, scene._h, boxes.data_ptr(), offsets.data_ptr(), prim.data_ptr(), n * k,
                                                       count.data_ptr(), n, OVERLAP_LIST, stream))
            return BoxTable(host(prim), host(count))
        splits = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        total = 0
        if n:
            stream = torch.cuda.current_stream(dev).cuda_stream
            counts = torch.empty(n, dtype=torch.int32, device=dev)
            no_room = torch.zeros(n + 1, dtype=torch.int32, device=dev)       # capacity 0: every segment is empty
            _check(_lib.drt_renderer_overlap_boxes(self._h, scene._h, boxes.data_ptr(), no_room.data_ptr(), None, 0, counts.data_ptr(), n,
                                                   OVERLAP_LIST, stream))
            splits[1:] = torch.cumsum(counts.to(torch.int64), dim=0)
            total = int(splits[-1].item())       # the one synchronisation: the result's size
            if total >= 2 ** 31:
                raise DrtError(ERR_INVALID, "%d triangles in all: fewer than 2^31 expected (split the boxes)" % total)
        splits = splits.to(torch.int32)
        prim = torch.empty(total, dtype=torch.int32, device=dev)
        if total:
            _check(_lib.drt_renderer_overlap_boxes(self._h, scene._h, boxes.data_ptr(), splits.data_ptr(), prim.data_ptr(), total, None, n,
                                                   OVERLAP_LIST, stream))
        return BoxList(host(splits), host(prim))

    def overlapsAny(self, scene, center=None, half=None, axes=None, lo=None, hi=None):
        """Whether any triangle touches each query box: bool [N] (drt_renderer_overlap_boxes in mode DRT_OVERLAP_ANY, whose
        traversal ends at the first triangle found).  Boxes and conventions as overlapBoxes."""
        import torch                             # (only here: importing the package does not import torch)
        dev = torch.device("cuda", self._device)
        boxes, from_numpy = _box_batch(torch, dev, center, half, axes, lo, hi)
        n = boxes.shape[0]
        counts = torch.empty(n, dtype=torch.int32, device=dev)
        if n:
            stream = torch.cuda.current_stream(dev).cuda_stream
            _check(_lib.drt_renderer_overlap_boxes(self._h, scene._h, boxes.data_ptr(), None, None, 0, counts.data_ptr(), n, OVERLAP_ANY, stream))
        res = counts > 0
        return res.cpu().numpy() if from_numpy else res

    def overlapTriangles(self, scene, tris, k=None):
        """The mesh triangles that each query triangle touches, in ascending triangle index (drt_renderer_overlap_triangles in mode
        DRT_OVERLAP_LIST).  tris: vertices [N, 3, 3] float32, or a packed [N, 12] (drt_tri).  Touching counts: a shared vertex or
        edge is a touch, and a triangle of the scene given as a query lists itself and its neighbours.  A query with a NaN or an
        infinity lists nothing.  Alpha cut-outs are ignored.
        k=None: TriList(splits [N + 1] int32, prim [M] int32), query i's triangles at [splits[i], splits[i + 1]) -- a count with
        capacity 0, a cumulative sum on the device, and a fill; the total is read back between them to size the result: that read
        is this call's one synchronisation with the device.  k=K: TriTable(prim [N, K] int32, count [N] int32) in one pass: the
        first K of each list, -1 behind a shorter one; count is the number listed, stored or not.  Device tensors in, device
        tensors out (enqueued on the current torch stream); numpy in, numpy out."""
        if k is not None and (isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1):
            raise DrtError(ERR_INVALID, "k = %r: a positive integer or None expected" % (k,))
        import torch                             # (only here: importing the package does not import torch)
        dev = torch.device("cuda", self._device)
        packed, from_numpy = _tri_batch(torch, dev, tris)
        n = packed.shape[0]
        host = (lambda t: t.cpu().numpy()) if from_numpy else (lambda t: t)
        if k is not None:
            k = int(k)
            if n * k >= 2 ** 31:
                raise DrtError(ERR_INVALID, "%d triangles x %d slots: fewer than 2^31 records expected" % (n, k))
            prim = torch.empty((n, k), dtype=torch.int32, device=dev)
            count = torch.empty(n, dtype=torch.int32, device=dev)
            if n:
                offsets = (torch.arange(n + 1, dtype=torch.int64, device=dev) * k).to(torch.int32)
                stream = torch.cuda.current_stream(dev).cuda_stream
                _check(_lib.drt_renderer_overlap_triangles(self._h, scene._h, packed.data_ptr(), offsets.data_ptr(), prim.data_ptr(), n * k,
                                                           count.data_ptr(), n, OVERLAP_LIST, stream))
            return TriTable(host(prim), host(count))
        splits = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        total = 0
        if n:
            stream = torch.cuda.current_stream(dev).cuda_stream
            counts = torch.empty(n, dtype=torch.int32, device=dev)
            no_room = torch.zeros(n + 1, dtype=torch.int32, device=dev)       # capacity 0: every segment is empty
            _check(_lib.drt_renderer_overlap_triangles(self._h, scene._h, packed.data_ptr(), no_room.data_ptr(), None, 0, counts.data_ptr(), n,
                                                       OVERLAP_LIST, stream))
            splits[1:] = torch.cumsum(counts.to(torch.int64), dim=0)
            total = int(splits[-1].item())       # the one synchronisation: the result's size
            if total >= 2 ** 31:
                raise DrtError(ERR_INVALID, "%d triangles in all: fewer than 2^31 expected (split the queries)" % total)
        splits = splits.to(torch.int32)
        prim = torch.empty(total, dtype=torch.int32, device=dev)
        if total:
            _check(_lib.drt_renderer_overlap_triangles(self._h, scene._h, packed.data_ptr(), splits.data_ptr(), prim.data_ptr(), total, None, n,
                                                       OVERLAP_LIST, stream))
        return TriList(host(splits), host(prim))

    def intersectsAny(self, scene, tris):
        """Whether each query triangle touches any triangle of the mesh: bool [N] (drt_renderer_overlap_triangles in mode
        DRT_OVERLAP_ANY, whose traversal ends at the first triangle found).  Triangles and conventions as overlapTriangles."""
        import torch                             # (only here: importing the package does not import torch)
        dev = torch.device("cuda", self._device)
        packed, from_numpy = _tri_batch(torch, dev, tris)
        n = packed.shape[0]
        counts = torch.empty(n, dtype=torch.int32, device=dev)
        if n:
            stream = torch.cuda.current_stream(dev).cuda_stream
            _check(_lib.drt_renderer_overlap_triangles(self._h, scene._h, packed.data_ptr(), None, None, 0, counts.data_ptr(), n, OVERLAP_ANY, stream))
        res = counts > 0
        return res.cpu().numpy() if from_numpy else res

    def _tri_distance(self, scene, tris, max_dist, mode):
        """(records [N, 12] float32 on the device (drt_tri_near), came_from_numpy) of drt_renderer_triangle_distance.  max_dist: a
        scalar (inf: the entry point's NULL) or [N] float32 of the triangles' kind."""
        import torch                             # (only here: importing the package does not import torch)
        dev = torch.device("cuda", self._device)
        packed, from_numpy = _tri_batch(torch, dev, tris)
        n = packed.shape[0]
        md = None
        if isinstance(max_dist, (int, float, np.floating, np.integer)) and not isinstance(max_dist, bool):
            if float(max_dist) != float("inf"):
                md = torch.full((n,), float(max_dist), dtype=torch.float32, device=dev)
        elif isinstance(max_dist, np.ndarray) or torch.is_tensor(max_dist):
            if isinstance(max_dist, np.ndarray) != from_numpy:
                raise DrtError(ERR_INVALID, "mix of numpy arrays and device tensors")
            if max_dist.dtype != (np.float32 if from_numpy else torch.float32):
                raise DrtError(ERR_INVALID, "max_dist: dtype %s, float32 expected" % max_dist.dtype)
            if not from_numpy and max_dist.device != dev:
                raise DrtError(ERR_INVALID, "max_dist: on %s, the renderer is on %s" % (max_dist.device, dev))
            if tuple(max_dist.shape) != (n,):
                raise DrtError(ERR_INVALID, "max_dist: shape %s for %d triangles" % (tuple(max_dist.shape), n))
            md = torch.from_numpy(np.ascontiguousarray(max_dist)).to(dev) if from_numpy else max_dist.contiguous()
        else:
            raise DrtError(ERR_INVALID, "max_dist: a number, a numpy array or a torch tensor expected")
        out = torch.empty((n, 12), dtype=torch.float32, device=dev)
        if n:
            stream = torch.cuda.current_stream(dev).cuda_stream
            _check(_lib.drt_renderer_triangle_distance(self._h, scene._h, packed.data_ptr(), None if md is None else md.data_ptr(),
                                                       out.data_ptr(), n, mode, stream))
        return out, from_numpy

    def triangleDistance(self, scene, tris, max_dist=float("inf")):
        """The mesh triangle nearest each query triangle (drt_renderer_triangle_distance in mode DRT_TRIDIST_NEAREST): TriNearest(d2 [N],
        prim [N] int32, point_q [N, 3], point_t [N, 3], u, v, feature [N] int32).  point_q lies on the query triangle, point_t on
        triangle prim at barycentrics (u, v), and d2 is their squared distance; feature & 15 names the deciding candidate (0..2 a
        query vertex, 3..5 a vertex of the scene triangle, 6 + 3 i + j an edge pair).  Where the pair touches -- the overlap predicate
        of overlapTriangles does not separate it -- d2 = 0, feature has bit 16 set and the points are not a contact point.  prim -1 =
        nothing within max_dist, a query with a NaN or an infinity, or an empty scene (then d2 = max_dist^2 and the rest is 0).
        tris: vertices [N, 3, 3] float32, or a packed [N, 12] (drt_tri); max_dist: a scalar or [N].  No penetration depth, no
        self-clearance (a triangle of the scene touches itself), alpha cut-outs are ignored.  Device tensors in, device tensors out
        (enqueued on the current torch stream); numpy in, numpy out.  After refit(scene, positions) the moved geometry is queried."""
        import torch
        out, from_numpy = self._tri_distance(scene, tris, max_dist, TRIDIST_NEAREST)
        if from_numpy:
            h = out.cpu().numpy()
            i = h.view(np.int32)
            return TriNearest(h[:, 3].copy(), i[:, 7].copy(), h[:, 0:3].copy(), h[:, 4:7].copy(), h[:, 8].copy(), h[:, 9].copy(), i[:, 10].copy())
        i = out.view(torch.int32)
        return TriNearest(out[:, 3], i[:, 7], out[:, 0:3], out[:, 4:7], out[:, 8], out[:, 9], i[:, 10])

    def withinDistance(self, scene, tris, dist):
        """Whether any triangle of the mesh lies within `dist` (a scalar or [N]) of each query triangle, strictly: bool [N]
        (drt_renderer_triangle_distance in mode DRT_TRIDIST_ANY, whose search ends at the first pair found).  dist = 0 finds nothing:
        touching is intersectsAny.  Triangles and conventions as triangleDistance."""
        import torch
        out, from_numpy = self._tri_distance(scene, tris, dist, TRIDIST_ANY)
        res = out.view(torch.int32)[:, 7] >= 0
        return res.cpu().numpy() if from_numpy else res

    def meshDistance(self, scene, tris, max_dist=float("inf")):
        """The clearance between a query mesh and the scene: the smallest d2 of triangleDistance over the batch, reduced on the device:
        MeshDistance(d2, query, prim, point_q [3], point_t [3], feature) -- query is the index of the query triangle, and of equal d2
        the smallest index wins.  An empty batch or no pair within max_dist: query = prim = -1, d2 = inf, the rest 0.  d2 = 0 means
        that the meshes touch by the overlap predicate; there is no penetration depth.  Device tensors in, 0-dimensional device
        tensors out (nothing is read back); numpy in, numpy scalars out."""
        import torch
        out, from_numpy = self._tri_distance(scene, tris, max_dist, TRIDIST_NEAREST)
        n = out.shape[0]
        dev = out.device
        miss = torch.zeros(12, dtype=torch.float32, device=dev)
        miss[3] = float("inf")
        miss.view(torch.int32)[7] = -1
        query = torch.full((), -1, dtype=torch.int64, device=dev)
        row = miss
        if n:
            hit = out.view(torch.int32)[:, 7] >= 0
            key = torch.where(hit, out[:, 3], torch.full_like(out[:, 3], float("inf")))
            least = hit & (key == key.min())                                       # (a hit's d2 is finite: below max_dist^2)
            index = torch.arange(n, dtype=torch.int64, device=dev)
            first = torch.where(least, index, torch.full_like(index, n)).min()     # the smallest query index of equal minima
            found = first < n
            row = torch.where(found, out.index_select(0, first.clamp(max=n - 1).reshape(1))[0], miss)
            query = torch.where(found, first, query)
        i = row.view(torch.int32)
        res = MeshDistance(row[3], query.to(torch.int32), i[7], row[0:3], row[4:7], i[10])
        if from_numpy:
            return MeshDistance(*(x.cpu().numpy().copy() if x.dim() else x.cpu().numpy()[()] for x in res))
        return res

    def _tri_cast(self, scene, tris, dirs, tmax, mode):
        """(records [N, 12] float32 on the device (drt_tri_hit), came_from_numpy) of drt_renderer_triangle_cast.  dirs: [3] or [N, 3]
        float32 of the triangles' kind; tmax: a scalar or [N] float32 of the triangles' kind."""
        import torch                             # (only here: importing the package does not import torch)
        dev = torch.device("cuda", self._device)
        packed, from_numpy = _tri_batch(torch, dev, tris)
        n = packed.shape[0]

        def per_cast(x, name, tail):
            if isinstance(x, (list, tuple)):
                x = np.asarray(x, np.float32) if from_numpy else torch.tensor(x, dtype=torch.float32, device=dev)
            if not (isinstance(x, np.ndarray) or torch.is_tensor(x)):
                raise DrtError(ERR_INVALID, "%s: a number, a numpy array or a torch tensor expected" % name)
            if isinstance(x, np.ndarray) != from_numpy:
                raise DrtError(ERR_INVALID, "mix of numpy arrays and device tensors")
            if x.dtype != (np.float32 if from_numpy else torch.float32):
                raise DrtError(ERR_INVALID, "%s: dtype %s, float32 expected" % (name, x.dtype))
            if not from_numpy and x.device != dev:
                raise DrtError(ERR_INVALID, "%s: on %s, the renderer is on %s" % (name, x.device, dev))
            if tuple(x.shape) not in (tail, (n,) + tail):
                raise DrtError(ERR_INVALID, "%s: shape %s for %d triangles" % (name, tuple(x.shape), n))
            return torch.from_numpy(np.ascontiguousarray(x)).to(dev) if from_numpy else x

        motions = torch.empty((n, 4), dtype=torch.float32, device=dev)             # drt_motion {d[3], tmax}
        motions[:, 0:3] = per_cast(dirs, "dirs", (3,))
        if isinstance(tmax, (int, float, np.floating, np.integer)) and not isinstance(tmax, bool):
            motions[:, 3] = float(tmax)
        else:
            motions[:, 3] = per_cast(tmax, "tmax", ())
        out = torch.empty((n, 12), dtype=torch.float32, device=dev)
        if n:
            stream = torch.cuda.current_stream(dev).cuda_stream
            _check(_lib.drt_renderer_triangle_cast(self._h, scene._h, packed.data_ptr(), motions.data_ptr(), out.data_ptr(), n, mode, stream))
        return out, from_numpy

    def triangleCast(self, scene, tris, dirs, tmax=1.0):
        """The first contact of each query triangle translating along its direction with the mesh (drt_renderer_triangle_cast in mode
        DRT_TRICAST_FIRST): TriHits(t [N], prim [N] int32, point [N, 3], normal [N, 3], u, v, feature [N] int32).  The triangle is at
        tris + dirs * t, and t is the smallest in [0, tmax) at which it touches triangle prim, at `point` on that triangle with
        barycentrics (u, v); normal is unnormalised and turned against the motion; feature & 15 names the deciding candidate (0..2 a
        query vertex onto the face, 3..5 a vertex of the scene triangle onto the query's face, 6 + 3 i + j an edge pair).  Where the pair
        already touches at the start -- the overlap predicate of overlapTriangles does not separate it -- t = 0, feature has bit 16 set
        and point, normal, u, v are zeros.  prim -1 = nothing touched before tmax, a query with a NaN or an infinity, a NaN in dirs or
        tmax, or an empty scene (then t = tmax, feature = -1 and the rest is 0).  tris: vertices [N, 3, 3] float32, or a packed
        [N, 12] (drt_tri); dirs: [3] or [N, 3]; tmax: a scalar or [N].  No rotation, no thickness or tolerance, no penetration depth; a
        coplanar pair sliding in its plane is seen only if it overlaps at the start; alpha cut-outs are ignored.  Device tensors in,
        device tensors out (enqueued on the current torch stream); numpy in, numpy out.  After refit(scene, positions) the moved
        geometry is queried."""
        import torch
        out, from_numpy = self._tri_cast(scene, tris, dirs, tmax, TRICAST_FIRST)
        if from_numpy:
            h = out.cpu().numpy()
            i = h.view(np.int32)
            return TriHits(h[:, 3].copy(), i[:, 7].copy(), h[:, 0:3].copy(), h[:, 4:7].copy(), h[:, 8].copy(), h[:, 9].copy(), i[:, 10].copy())
        i = out.view(torch.int32)
        return TriHits(out[:, 3], i[:, 7], out[:, 0:3], out[:, 4:7], out[:, 8], out[:, 9], i[:, 10])

    def castsAny(self, scene, tris, dirs, tmax=1.0):
        """Whether each query triangle touches the mesh anywhere along its motion in [0, tmax): bool [N] (drt_renderer_triangle_cast
        in mode DRT_TRICAST_ANY, whose search ends at the first pair found).  Triangles and conventions as triangleCast."""
        import torch
        out, from_numpy = self._tri_cast(scene, tris, dirs, tmax, TRICAST_ANY)
        res = out.view(torch.int32)[:, 7] >= 0
        return res.cpu().numpy() if from_numpy else res

    def meshCast(self, scene, tris, d, tmax=1.0):
        """The time of impact of a query mesh translating along d with the scene: the smallest t of triangleCast over the batch, reduced
        on the device: MeshHit(t, query, prim, point [3], normal [3], feature) -- query is the index of the query triangle, and of
        equal t the smallest index wins.  An empty batch or no contact before tmax: query = prim = -1, t = inf, feature = -1, the rest
        0.  t = 0 with feature bit 16 means that the meshes touch at the start by the overlap predicate; there is no penetration depth
        and no rotation.  Device tensors in, 0-dimensional device tensors out (nothing is read back); numpy in, numpy scalars out."""
        import torch
        out, from_numpy = self._tri_cast(scene, tris, d, tmax, TRICAST_FIRST)
        n = out.shape[0]
        dev = out.device
        miss = torch.zeros(12, dtype=torch.float32, device=dev)
        miss[3] = float("inf")
        miss.view(torch.int32)[7] = -1
        miss.view(torch.int32)[10] = -1
        query = torch.full((), -1, dtype=torch.int64, device=dev)
        row = miss
        if n:
            hit = out.view(torch.int32)[:, 7] >= 0
            key = torch.where(hit, out[:, 3], torch.full_like(out[:, 3], float("inf")))
            least = hit & (key == key.min())                                       # (a hit's t is finite: below tmax)
            index = torch.arange(n, dtype=torch.int64, device=dev)
            first = torch.where(least, index, torch.full_like(index, n)).min()     # the smallest query index of equal minima
            found = first < n
            row = torch.where(found, out.index_select(0, first.clamp(max=n - 1).reshape(1))[0], miss)
            query = torch.where(found, first, query)
        i = row.view(torch.int32)
        res = MeshHit(row[3], query.to(torch.int32), i[7], row[0:3], row[4:7], i[10])
        if from_numpy:
            return MeshHit(*(x.cpu().numpy().copy() if x.dim() else x.cpu().numpy()[()] for x in res))
        return res

    def surface(self, scene, refs, u=None, v=None, normals=None):
        """What lies on the surface at references (prim, u, v) (drt_renderer_surface_lookup): Surface(position, normal, shading [.., 3],
        uv [.., 2], albedo, emissive [.., 3], alpha, roughness, refractive_index, material, load_index, texture int32, metallic,
        transmission bool), of the references' shape.  refs: anything with .prim, .u and .v of one shape -- the results of traceRays,
        nearest, sphereCast, triangleCast, kNearest, sampleSurface ... -- or prim with u and v as three arrays.  prim outside the
        mesh (a miss, -1): zeros with material = load_index = texture = -1.  u and v are used as given and extrapolate outside the
        triangle.  position and normal (the stored face normal, not turned) are the device copy's: after refit(scene, positions) the
        moved mesh's.  albedo and alpha are what the ALBEDO view shows: the flat albedo, or the nearest texel of the texture, as the
        reference has -- no filtering, no normal maps, no tangents.  shading is the interpolated vertex normals and is not
        normalised; normals: [n_tris, 3, 3] float32 in load order (a device tensor or numpy, the array refit takes) to use instead of
        the host scene's, which None means also after a refit.  Device tensors in, device tensors out (enqueued on the current torch
        stream); numpy in, numpy out."""
        import torch                             # (only here: importing the package does not import torch)
        dev = torch.device("cuda", self._device)
        if u is None and v is None:
            if not all(hasattr(refs, f) for f in ("prim", "u", "v")):
                raise DrtError(ERR_INVALID, "refs: something with .prim, .u and .v expected, or prim, u and v")
            prim, u, v = refs.prim, refs.u, refs.v
        elif u is None or v is None:
            raise DrtError(ERR_INVALID, "refs: prim, u and v expected")
        else:
            prim = refs
        parts = []
        from_numpy = isinstance(prim, np.ndarray)
        for name, x, kind in (("prim", prim, "i"), ("u", u, "f"), ("v", v, "f")):
            if not (isinstance(x, np.ndarray) or torch.is_tensor(x)):
                raise DrtError(ERR_INVALID, "refs: %s: a numpy array or a torch tensor expected" % name)
            if isinstance(x, np.ndarray) != from_numpy:
                raise DrtError(ERR_INVALID, "refs: mix of numpy arrays and device tensors")
            want = (np.int32 if from_numpy else torch.int32) if kind == "i" else (np.float32 if from_numpy else torch.float32)
            if x.dtype != want:
                raise DrtError(ERR_INVALID, "refs: %s: dtype %s, %s expected" % (name, x.dtype, "int32" if kind == "i" else "float32"))
            if not from_numpy and x.device != dev:
                raise DrtError(ERR_INVALID, "refs: %s: on %s, the renderer is on %s" % (name, x.device, dev))
            if tuple(x.shape) != tuple(prim.shape):
                raise DrtError(ERR_INVALID, "refs: %s: shape %s, prim has %s" % (name, tuple(x.shape), tuple(prim.shape)))
            parts.append(x)
        if from_numpy:                           # (after every check: nothing touches the device for a bad argument)
            parts = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in parts]
        shape = tuple(prim.shape)
        n_tris = _lib.drt_scene_triangle_count(scene._h)
        if normals is not None:
            if isinstance(normals, np.ndarray):
                normals = torch.from_numpy(np.ascontiguousarray(normals, np.float32)).to(dev)
            elif not torch.is_tensor(normals):
                raise DrtError(ERR_INVALID, "normals: a numpy array or a torch tensor expected")
            if normals.dtype != torch.float32 or normals.device != dev or normals.numel() != 9 * n_tris:
                raise DrtError(ERR_INVALID, "normals: %s %s with %d values, float32 [%d, 3, 3] on %s expected"
                               % (normals.dtype, normals.device, normals.numel(), n_tris, dev))
            normals = normals.contiguous()
        packed = torch.zeros((parts[0].numel(), 4), dtype=torch.float32, device=dev)        # drt_hit {t, prim, u, v}
        packed.view(torch.int32)[:, 1] = parts[0].reshape(-1)
        packed[:, 2], packed[:, 3] = parts[1].reshape(-1), parts[2].reshape(-1)
        n = packed.shape[0]
        out = torch.empty((n, 24), dtype=torch.float32, device=dev)                         # drt_surface
        if n:
            stream = torch.cuda.current_stream(dev).cuda_stream
            _check(_lib.drt_renderer_surface_lookup(self._h, scene._h, packed.data_ptr(), normals.data_ptr() if normals is not None and n_tris else None,
                                                    out.data_ptr(), n, stream))
        if from_numpy:
            h = out.cpu().numpy()
            i = h.view(np.int32)
            f = lambda a: a.copy().reshape(shape + a.shape[1:])
            return Surface(f(h[:, 0:3]), f(h[:, 4:7]), f(h[:, 8:11]), f(h[:, 16:18]), f(h[:, 12:15]), f(h[:, 20:23]), f(h[:, 7]), f(h[:, 18]), f(h[:, 23]),
                           f(i[:, 3]), f(i[:, 11]), f(i[:, 15]), f((i[:, 19] & 1) != 0), f((i[:, 19] & 2) != 0))
        i = out.view(torch.int32)
        f = lambda a: a.reshape(shape + tuple(a.shape[1:]))
        return Surface(f(out[:, 0:3]), f(out[:, 4:7]), f(out[:, 8:11]), f(out[:, 16:18]), f(out[:, 12:15]), f(out[:, 20:23]), f(out[:, 7]), f(out[:, 18]),
                       f(out[:, 23]), f(i[:, 3]), f(i[:, 11]), f(i[:, 15]), f((i[:, 19] & 1) != 0), f((i[:, 19] & 2) != 0))

    def sampleSurface(self, scene, n, seed=0, first=0, as_torch=False):
        """n references drawn on the mesh with probability proportional to area (drt_renderer_sample_surface): SurfaceSamples(prim [n]
        int32, u, v [n] float32) with u, v >= 0 and u + v <= 1; they feed surface() as they are -- surface(scene, smp).position is a
        point cloud of the mesh as it stands on the device, after a refit the moved one.  Sample k has index first + k of the stream
        `seed` and depends on (seed, index) and the scene only, so first= continues a stream; first + n <= 2^32.  A triangle smaller
        than 2^-36 of the largest is never drawn; a mesh without area gives prim -1 everywhere.  Independent hashes: not stratified,
        no blue noise.  as_torch=True: device tensors, the work enqueued on the current torch stream; else numpy arrays."""
        import torch                             # (only here: importing the package does not import torch)
        dev = torch.device("cuda", self._device)
        n, seed, first = int(n), int(seed), int(first)
        if n < 0 or not 0 <= seed < 1 << 32 or not 0 <= first < 1 << 32 or first + n > 1 << 32:
            raise DrtError(ERR_INVALID, "sampleSurface: n >= 0, seed and first in [0, 2^32) and first + n <= 2^32 expected")
        out = torch.empty((n, 4), dtype=torch.float32, device=dev)
        if n:
            stream = torch.cuda.current_stream(dev).cuda_stream
            _check(_lib.drt_renderer_sample_surface(self._h, scene._h, seed, first, out.data_ptr(), n, stream))
        if not as_torch:
            h = out.cpu().numpy()
            return SurfaceSamples(h.view(np.int32)[:, 1].copy(), h[:, 2].copy(), h[:, 3].copy())
        return SurfaceSamples(out.view(torch.int32)[:, 1], out[:, 2], out[:, 3])

    def surfaceWeights(self, scene, as_torch=False):
        """The table sampleSurface draws from (drt_renderer_surface_weights): [n_tris] inclusive sums of the triangles' integer weights,
        |cross(e1, e2)| of the device copy scaled so that the largest lies in [2^34, 2^35) and truncated; the last entry is the total.
        numpy uint64, or with as_torch=True a device int64 tensor (the values are below 2^63), enqueued on the current torch stream."""
        import torch                             # (only here: importing the package does not import torch)
        dev = torch.device("cuda", self._device)
        out = torch.empty(_lib.drt_scene_triangle_count(scene._h), dtype=torch.int64, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        _check(_lib.drt_renderer_surface_weights(self._h, scene._h, out.data_ptr() if out.numel() else None, stream))
        return out if as_torch else out.cpu().numpy().view(np.uint64)

    def ambientOcclusion(self, scene, refs=None, points=None, normals=None, samples=64, max_dist=float("inf"), bias=0.001, seed=0, first=0,
                         side=1.0, facing=None):
        """How much of the hemisphere above surface points is open (drt_renderer_ambient_occlusion): ambient occlusion, sky-view
        factor, accessibility.  Per point `samples` (1 .. 4096) occlusion rays from point + normal * bias in the renderer's bounce
        directions normalize(normal + unit-sphere draw), none longer than max_dist (inf = sky visibility); alpha cut-outs are seen
        through as in occluded.  Returns AmbientOcclusion(open int32 [..] -- the number of open samples, -1 = a skipped point --,
        visibility float32 [..] = open / samples (NaN where skipped), bent float32 [.., 3] = sums / (65536 max(open, 1)): the mean open
        direction, not normalised, sums int32 [.., 3]: the exact integer record), of the points' shape.  The record is integer sums:
        the same bytes on every run.
        refs: anything with .prim, .u and .v -- the results of traceRays, nearest, sampleSurface ... -- whose position and face normal
        surface() looks up; a reference outside the mesh (a miss) is skipped.  Or points= and normals= [.., 3] float32, packed as
        given: pass unit normals for a cosine-weighted answer.  side (a scalar or [..]) multiplies the normals: -1 looks below the
        surface.  facing= directions [.., 3]: every normal is turned against its direction by the renderer's rule, negated where
        dot(normal, direction) > 0 -- pass the rays that found the points.  max_dist and bias: scalars or [..]; a point whose max_dist
        is negative or a NaN is skipped.  Sample streams are (seed, first + index): first= continues a batch, first + N <= 2^32.
        No distance falloff, no weighting beyond the cosine of the draw, independent hashes -- not stratified --, no indirect light
        (radiance does that), no filtering across points; the absolute bias and the triangle test's 1e-6 apply as in traceRays.
        Device tensors in, device tensors out (enqueued on the current torch stream); numpy in, numpy out."""
        import torch                             # (only here: importing the package does not import torch)
        dev = torch.device("cuda", self._device)

        def bad(msg):
            return DrtError(ERR_INVALID, "ambientOcclusion: " + msg)

        samples, seed, first = int(samples), int(seed), int(first)
        if not 1 <= samples <= AO_MAX_SAMPLES:
            raise bad("samples %d: 1 .. 4096 expected" % samples)
        if not 0 <= seed < 1 << 32 or not 0 <= first < 1 << 32:
            raise bad("seed and first in [0, 2^32) expected")
        if (refs is None) == (points is None):
            raise bad("refs, or points= and normals=, expected")
        if refs is not None:
            if normals is not None:
                raise bad("normals= come with points=; the normals of refs are the mesh's")
            if not all(hasattr(refs, f) for f in ("prim", "u", "v")):
                raise bad("refs: something with .prim, .u and .v expected")
            lead = refs.prim
        else:
            if normals is None:
                raise bad("points= come with normals=")
            lead = points
        if not (isinstance(lead, np.ndarray) or torch.is_tensor(lead)):
            raise bad("a numpy array or a torch tensor expected")
        from_numpy = isinstance(lead, np.ndarray)
        shape = tuple(lead.shape) if refs is not None else tuple(lead.shape[:-1])

        def vectors(x, name):                    # [.., 3] float32 of the points' shape, still where it was given
            if isinstance(x, np.ndarray) != from_numpy or not (isinstance(x, np.ndarray) or torch.is_tensor(x)):
                raise bad("%s: a %s expected, as the points are" % (name, "numpy array" if from_numpy else "torch tensor"))
            if x.dtype != (np.float32 if from_numpy else torch.float32):
                raise bad("%s: dtype %s, float32 expected" % (name, x.dtype))
            if tuple(x.shape) != shape + (3,):
                raise bad("%s: shape %s, %s expected" % (name, tuple(x.shape), shape + (3,)))
            if not from_numpy and x.device != dev:
                raise bad("%s: on %s, the renderer is on %s" % (name, x.device, dev))
            return x

        def per_point(x, name):                  # a scalar, or [..] float32 of the points' shape
            if isinstance(x, (int, float, np.floating, np.integer)):
                return float(x)
            if isinstance(x, np.ndarray) or torch.is_tensor(x):
                if tuple(x.shape) != shape:
                    raise bad("%s: shape %s, a scalar or %s expected" % (name, tuple(x.shape), shape))
                if not isinstance(x, np.ndarray) and x.device != dev:
                    raise bad("%s: on %s, the renderer is on %s" % (name, x.device, dev))
                return x
            raise bad("%s: a scalar, a numpy array or a torch tensor expected" % name)

        if refs is None:
            points, normals = vectors(points, "points"), vectors(normals, "normals")
        if facing is not None:
            facing = vectors(facing, "facing")
        max_dist, bias, side = per_point(max_dist, "max_dist"), per_point(bias, "bias"), per_point(side, "side")
        n = 1
        for extent in shape:
            n *= int(extent)
        if first + n > 1 << 32:
            raise bad("first + N must not exceed 2^32")

        def on_device(x, tail=()):               # (after every check: nothing touches the device for a bad argument)
            if isinstance(x, float):
                return x
            if isinstance(x, np.ndarray):
                x = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
            return x.to(torch.float32).reshape((n,) + tail)

        if refs is not None:
            ref3 = SurfaceSamples(*(torch.from_numpy(np.ascontiguousarray(x)).to(dev) if isinstance(x, np.ndarray) else x
                                    for x in (refs.prim, refs.u, refs.v)))
            found = self.surface(scene, ref3)
            pos, nrm = found.position.reshape(n, 3), found.normal.reshape(n, 3)
            missed = found.material.reshape(n) < 0
        else:
            pos, nrm, missed = on_device(points, (3,)), on_device(normals, (3,)), None
        side = on_device(side)
        nrm = nrm * (side if isinstance(side, float) else side[:, None])
        if facing is not None:
            f = on_device(facing, (3,))
            against = ((nrm[:, 0] * f[:, 0] + nrm[:, 1] * f[:, 1]) + nrm[:, 2] * f[:, 2]) > 0
            nrm = torch.where(against[:, None], -nrm, nrm)
        packed = torch.empty((n, 8), dtype=torch.float32, device=dev)                       # drt_ao_point {p, max_dist, n, bias}
        packed[:, 0:3], packed[:, 4:7] = pos, nrm
        packed[:, 3], packed[:, 7] = on_device(max_dist), on_device(bias)
        if missed is not None:
            packed[:, 3] = torch.where(missed, torch.full_like(packed[:, 3], -1.0), packed[:, 3])
        out = torch.empty((n, 4), dtype=torch.int32, device=dev)                            # drt_ao_result {open, bent[3]}
        if n:
            params = (C.c_uint32 * 4)(samples, seed, first, 0)
            stream = torch.cuda.current_stream(dev).cuda_stream
            _check(_lib.drt_renderer_ambient_occlusion(self._h, scene._h, packed.data_ptr(), n, C.addressof(params), out.data_ptr(), stream))
        n_open, sums = out[:, 0], out[:, 1:4]
        visibility = torch.where(n_open < 0, torch.full((n,), float("nan"), dtype=torch.float32, device=dev), n_open.to(torch.float32) / samples)
        bent = sums.to(torch.float32) / (65536.0 * n_open.clamp(min=1).to(torch.float32))[:, None]
        res = AmbientOcclusion(n_open.reshape(shape), visibility.reshape(shape), bent.reshape(shape + (3,)), sums.reshape(shape + (3,)))
        if from_numpy:
            return AmbientOcclusion(*(x.cpu().numpy().copy() for x in res))
        return res

    def selfIntersections(self, scene, positions=None):
        """Where the scene's mesh cuts itself: int32 [P, 2], the pairs i < j of triangle indices (tree order, as every query reports
        them) that touch and share no vertex position, sorted by (i, j).  The queries are the scene's own triangles in tree order:
        by default the positions of the host scene's m_PrimitivesBuffer; with positions= [n, 3, 3] float32 in load order, as refit
        takes them (for a refitted device copy), mapped through triangleOrder().  It runs overlapTriangles, then on the device drops
        j <= i and every pair in which any vertex of one triangle is bit-equal to a vertex of the other: neighbours always touch.
        Two neighbours that also cut each other are therefore not reported.  Degenerate triangles are queried like any other.
        positions as a device tensor: a device tensor comes back; else a numpy array."""
        import torch                             # (only here: importing the package does not import torch)
        verts, as_tensor = self._own_triangles(torch, scene, positions)
        n, dev = verts.shape[0], verts.device
        found = self.overlapTriangles(scene, verts)
        counts = (found.splits[1:] - found.splits[:-1]).to(torch.int64)
        i = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=dev), counts)
        j = found.prim.to(torch.int64)
        later = j > i
        i, j = i[later], j[later]
        shared = self._share_a_vertex(torch, verts, i, j)
        pairs = torch.stack([i[~shared], j[~shared]], dim=1).to(torch.int32)
        return pairs if as_tensor else pairs.cpu().numpy()

    def _own_triangles(self, torch, scene, positions):
        """(the scene's own triangles in tree order as contiguous device vertices [n, 3, 3], positions was a tensor): the host scene's
        m_PrimitivesBuffer, or positions= [n, 3, 3] float32 in load order mapped through triangleOrder()."""
        dev = torch.device("cuda", self._device)
        n = _lib.drt_scene_triangle_count(scene._h)
        as_tensor = torch.is_tensor(positions)
        if positions is None:
            verts = torch.from_numpy(np.ascontiguousarray(scene.m_PrimitivesBuffer["vertex"]["position"], np.float32).reshape(n, 3, 3)).to(dev)
        else:
            if isinstance(positions, np.ndarray):
                if positions.dtype != np.float32:
                    raise DrtError(ERR_INVALID, "positions: dtype %s, float32 expected" % positions.dtype)
                positions = torch.from_numpy(np.ascontiguousarray(positions)).to(dev)
            elif not as_tensor:
                raise DrtError(ERR_INVALID, "positions: a numpy array or a torch tensor expected")
            if positions.dtype != torch.float32 or positions.device != dev or positions.numel() != 9 * n:
                raise DrtError(ERR_INVALID, "positions: %s %s with %d values, float32 [%d, 3, 3] on %s expected"
                               % (positions.dtype, positions.device, positions.numel(), n, dev))
            order = torch.from_numpy(scene.triangleOrder().astype(np.int64)).to(dev)
            verts = positions.reshape(n, 3, 3)[order]
        return verts.contiguous(), as_tensor

    @staticmethod
    def _share_a_vertex(torch, verts, i, j):
        """bool per pair (i, j) of triangles of verts [n, 3, 3]: some vertex of one is bit-equal to a vertex of the other."""
        bits = verts.view(torch.int32)
        return (bits[i][:, :, None, :] == bits[j][:, None, :, :]).all(dim=-1).any(dim=2).any(dim=1)

    def _cuts(self, scene, packed):
        """CutList of device tensors for packed device triangles [N, 12]: a count with capacity 0, a cumulative sum on the device, a
        fill; the total is read back between them to size the result."""
        import torch
        dev = packed.device
        n = packed.shape[0]
        splits = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        total = 0
        if n:
            stream = torch.cuda.current_stream(dev).cuda_stream
            counts = torch.empty(n, dtype=torch.int32, device=dev)
            no_room = torch.zeros(n + 1, dtype=torch.int32, device=dev)       # capacity 0: every segment is empty
            _check(_lib.drt_renderer_intersect_triangles(self._h, scene._h, packed.data_ptr(), no_room.data_ptr(), None, 0, counts.data_ptr(), n,
                                                         stream))
            splits[1:] = torch.cumsum(counts.to(torch.int64), dim=0)
            total = int(splits[-1].item())       # the one synchronisation: the result's size
            if total >= 2 ** 31:
                raise DrtError(ERR_INVALID, "%d segments in all: fewer than 2^31 expected (split the queries)" % total)
        splits = splits.to(torch.int32)
        rec = torch.empty((total, 8), dtype=torch.float32, device=dev)        # drt_isect: p, prim, q, code
        if total:
            _check(_lib.drt_renderer_intersect_triangles(self._h, scene._h, packed.data_ptr(), splits.data_ptr(), rec.data_ptr(), total, None, n,
                                                         stream))
        words = rec.view(torch.int32)
        return CutList(splits, rec[:, 0:3], rec[:, 4:7], words[:, 3], words[:, 7])

    def intersectTriangles(self, scene, tris):
        """Where each query triangle cuts the mesh (drt_renderer_intersect_triangles): one oriented segment per pair (query, mesh
        triangle) that cut each other.  tris: vertices [N, 3, 3] float32, or a packed [N, 12] (drt_tri); a mesh is a batch of queries,
        and its records are the curve along which it cuts the scene's surface, in pieces.  CutList(splits [N + 1] int32, p [M, 3],
        q [M, 3] float32, prim [M], code [M] int32): query i's segments p -> q at [splits[i], splits[i + 1]), in ascending mesh
        triangle prim, running along cross(query normal, triangle normal).  Each endpoint is one of the pair's four edge cut points,
        never interpolated along the line: code = cp + 16 * cq, where an endpoint's code is the mesh triangle's edge 0..2 or 4 + the
        query's edge it lies on, and an endpoint on an edge that two triangles share is the same bits from both.  Touching counts, and
        a zero-length segment is listed.  Coplanar pairs and zero-area triangles on either side give nothing -- stricter than
        overlapTriangles -- and so does a query with a NaN or an infinity.  Not chained into curves; alpha cut-outs are ignored.  A
        count with capacity 0, a cumulative sum on the device, and a fill; the total is read back between them to size the result:
        that read is this call's one synchronisation with the device.  Device tensors in, device tensors out (enqueued on the
        current torch stream); numpy in, numpy out."""
        import torch                             # (only here: importing the package does not import torch)
        dev = torch.device("cuda", self._device)
        packed, from_numpy = _tri_batch(torch, dev, tris)
        res = self._cuts(scene, packed)
        if from_numpy:
            return CutList(*(x.cpu().numpy().copy() for x in res))
        return res

    def selfIntersectionSegments(self, scene, positions=None):
        """The segments along which the scene's mesh cuts itself: SelfCuts(pairs int32 [P, 2], p [P, 3], q [P, 3] float32, code
        int32 [P]).  pairs[k] = (i, j), i < j, triangle indices in tree order, sorted by (i, j); p[k] -> q[k] is the segment of query
        i against mesh triangle j, as intersectTriangles gives it (code's low digit is an edge of j, or 4 + an edge of i).  The
        queries and positions= are selfIntersections': the scene's own triangles, and its filter is applied: j <= i is dropped, and
        so is every pair in which any vertex of one triangle is bit-equal to a vertex of the other.  A pair that only touches in a
        common plane is in selfIntersections but not here: coplanar pairs and zero-area triangles give no segment.  positions as a
        device tensor: device tensors come back; else numpy arrays."""
        import torch                             # (only here: importing the package does not import torch)
        verts, as_tensor = self._own_triangles(torch, scene, positions)
        n, dev = verts.shape[0], verts.device
        found = self.intersectTriangles(scene, verts)
        counts = (found.splits[1:] - found.splits[:-1]).to(torch.int64)
        i = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=dev), counts)
        j = found.prim.to(torch.int64)
        keep = j > i
        keep[keep.clone()] = ~self._share_a_vertex(torch, verts, i[keep], j[keep])
        res = SelfCuts(torch.stack([i[keep], j[keep]], dim=1).to(torch.int32), found.p[keep], found.q[keep], found.code[keep])
        return res if as_tensor else SelfCuts(*(x.cpu().numpy().copy() for x in res))

    def _sections(self, scene, planes):
        """SectionList of device tensors for packed device planes [N, 4]: a count with capacity 0, a cumulative sum on the device, a
        fill; the total is read back between them to size the result."""
        import torch
        dev = planes.device
        n = planes.shape[0]
        splits = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        total = 0
        if n:
            stream = torch.cuda.current_stream(dev).cuda_stream
            counts = torch.empty(n, dtype=torch.int32, device=dev)
            no_room = torch.zeros(n + 1, dtype=torch.int32, device=dev)       # capacity 0: every segment is empty
            _check(_lib.drt_renderer_plane_sections(self._h, scene._h, planes.data_ptr(), no_room.data_ptr(), None, 0, counts.data_ptr(), n,
                                                    SECTION_LIST, stream))
            splits[1:] = torch.cumsum(counts.to(torch.int64), dim=0)
            total = int(splits[-1].item())       # the one synchronisation: the result's size
            if total >= 2 ** 31:
                raise DrtError(ERR_INVALID, "%d segments in all: fewer than 2^31 expected (split the planes)" % total)
        splits = splits.to(torch.int32)
        rec = torch.empty((total, 8), dtype=torch.float32, device=dev)        # drt_section: p, prim, q, code
        if total:
            _check(_lib.drt_renderer_plane_sections(self._h, scene._h, planes.data_ptr(), splits.data_ptr(), rec.data_ptr(), total, None, n,
                                                    SECTION_LIST, stream))
        words = rec.view(torch.int32)
        return SectionList(splits, rec[:, 0:3], rec[:, 4:7], words[:, 3], words[:, 7])

    def planeSections(self, scene, normals, d=None):
        """The segments where each plane dot(n, x) = d cuts the mesh (drt_renderer_plane_sections in mode DRT_SECTION_LIST).  Planes:
        normals [N, 3] + d [N], or a packed [N, 4] (drt_plane: n, d); n is used as given, not normalised.  A plane with a NaN or an
        infinity lists nothing, and neither does n = 0.  SectionList(splits [N + 1] int32, p [M, 3], q [M, 3] float32, prim [M],
        code [M] int32): plane i's segments p -> q at [splits[i], splits[i + 1]), one per cut triangle in ascending triangle index;
        on a closed mesh with outward faces they run counter-clockwise seen from the side n points to.  code = the apex vertex
        (the one alone on its side) + 4 if it is above.  A vertex exactly on the plane counts as above; a triangle lying in the
        plane is not cut.  Not chained into loops, and the endpoints of neighbouring triangles agree only as far as their stored
        vertices do: weld with a tolerance.  No caps or filled polygons; alpha cut-outs are ignored.  A count with capacity 0, a
        cumulative sum on the device, and a fill; the total is read back between them to size the result: that read is this
        call's one synchronisation with the device.  Device tensors in, device tensors out (enqueued on the current torch
        stream); numpy in, numpy out."""
        import torch                             # (only here: importing the package does not import torch)
        dev = torch.device("cuda", self._device)
        planes, from_numpy = _plane_batch(torch, dev, normals, d)
        res = self._sections(scene, planes)
        if from_numpy:
            return SectionList(*(x.cpu().numpy().copy() for x in res))
        return res

    def cutsAny(self, scene, normals, d=None):
        """Whether each plane cuts any triangle: bool [N] (drt_renderer_plane_sections in mode DRT_SECTION_ANY, whose work ends at
        the first cut triangle found).  Planes and conventions as planeSections."""
        import torch                             # (only here: importing the package does not import torch)
        dev = torch.device("cuda", self._device)
        planes, from_numpy = _plane_batch(torch, dev, normals, d)
        n = planes.shape[0]
        counts = torch.empty(n, dtype=torch.int32, device=dev)
        if n:
            stream = torch.cuda.current_stream(dev).cuda_stream
            _check(_lib.drt_renderer_plane_sections(self._h, scene._h, planes.data_ptr(), None, None, 0, counts.data_ptr(), n, SECTION_ANY, stream))
        res = counts > 0
        return res.cpu().numpy() if from_numpy else res

    def slices(self, scene, count, axis=2, lo=None, hi=None):
        """`count` parallel sections along `axis` (0, 1 or 2): (heights [count] float32, SectionList), device tensors.  The planes
        have the unit normal of the axis and sit at the cell centres of the range (lo, hi) along it, by default the scene's bounds,
        laid out as sdfGrid lays out its cells: height i = lo + (i + 0.5) * ((hi - lo) / count).  The planes are made on the device."""
        if isinstance(count, bool) or not isinstance(count, (int, np.integer)) or count < 1:
            raise DrtError(ERR_INVALID, "count = %r: a positive integer expected" % (count,))
        if axis not in (0, 1, 2):
            raise DrtError(ERR_INVALID, "axis = %r: 0, 1 or 2 expected" % (axis,))
        import torch                             # (only here: importing the package does not import torch)
        dev = torch.device("cuda", self._device)
        if lo is None or hi is None:
            nodes = scene.m_BVHNodes
            if len(nodes) == 0:
                raise DrtError(ERR_INVALID, "slices: an empty scene has no bounds; give lo and hi")
            lo = nodes[-1]["bmin"][axis] if lo is None else lo                # the root is the last node
            hi = nodes[-1]["bmax"][axis] if hi is None else hi
        lo, hi = np.float32(lo), np.float32(hi)
        heights = float(lo) + (torch.arange(int(count), dtype=torch.float32, device=dev) + 0.5) * (float(hi - lo) / int(count))
        planes = torch.zeros((int(count), 4), dtype=torch.float32, device=dev)
        planes[:, axis] = 1.0
        planes[:, 3] = heights
        return heights, self._sections(scene, planes)

    def sectionAreas(self, scene, normals, d=None):
        """The signed area enclosed by each plane's contours: float64 [N], 0.5 * sum dot(n / |n|, cross(p, q)) over the plane's
        segments -- positive on a closed mesh with outward faces, where it is the area of the cross-section (n = 0 gives 0).  It
        is computed from planeSections' list on the device in float64 with a deterministic reduction: a cumulative sum over all
        segments (with its rounding errors carried along) and differences at the splits, no atomics.  Planes and conventions as planeSections."""
        import torch                             # (only here: importing the package does not import torch)
        dev = torch.device("cuda", self._device)
        planes, from_numpy = _plane_batch(torch, dev, normals, d)
        n = planes.shape[0]
        sec = self._sections(scene, planes)
        nrm = planes[:, 0:3].to(torch.float64)
        length = torch.sqrt((nrm * nrm).sum(dim=1, keepdim=True))
        unit = torch.where(length > 0, nrm / torch.where(length > 0, length, torch.ones_like(length)), torch.zeros_like(nrm))
        counts = (sec.splits[1:] - sec.splits[:-1]).to(torch.int64)
        owner = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=dev), counts)
        term = (unit[owner] * torch.linalg.cross(sec.p.to(torch.float64), sec.q.to(torch.float64), dim=1)).sum(dim=1)
        areas = 0.5 * _segment_sums(torch, term, sec.splits.to(torch.int64))      # (a compensated running sum: see there)
        return areas.cpu().numpy() if from_numpy else areas

    def _chain(self, scene, sec):
        """(ContourList of device tensors, slots [M, 4] int32, chains [N, 2] int32) for a SectionList of device tensors: the records
        packed again as drt_section, drt_renderer_chain_sections, and the lists read off the slots."""
        import torch
        dev = torch.device("cuda", self._device)
        splits = sec.splits.to(torch.int32).contiguous()
        n, total = splits.shape[0] - 1, sec.prim.shape[0]
        if n < 0 or sec.p.shape != (total, 3) or sec.q.shape != (total, 3) or sec.code.shape != (total,):
            raise DrtError(ERR_INVALID, "a SectionList expected: splits [N + 1], p and q [M, 3], prim and code [M]")
        if total >= 2 ** 31:
            raise DrtError(ERR_INVALID, "%d segments in all: fewer than 2^31 expected (split the planes)" % total)
        rec = torch.empty((total, 8), dtype=torch.float32, device=dev)         # drt_section: p, prim, q, code
        words = rec.view(torch.int32)
        rec[:, 0:3], rec[:, 4:7] = sec.p, sec.q
        words[:, 3], words[:, 7] = sec.prim, sec.code
        slots = torch.empty((total, 4), dtype=torch.int32, device=dev)
        chains = torch.zeros((max(n, 0), 2), dtype=torch.int32, device=dev)
        if n > 0 and total:
            stream = torch.cuda.current_stream(dev).cuda_stream
            _check(_lib.drt_renderer_chain_sections(self._h, scene._h, rec.data_ptr(), splits.data_ptr(), slots.data_ptr(), chains.data_ptr(),
                                                    n, total, stream))
        # what the slots say: a chain starts where first == position; miss records (a list with spare capacity) are in no chain
        status = slots[:, 3] >> 1
        kept = status != CHAIN_MISS
        starts = (slots[:, 1] == torch.arange(total, dtype=torch.int32, device=dev)) & kept
        seg = slots[:, 0][kept].to(torch.int64)
        kept_before = torch.cumsum(kept.to(torch.int64), dim=0) - kept.to(torch.int64)
        m = seg.shape[0]
        chain_splits = torch.cat([kept_before[starts], torch.full((1,), m, dtype=torch.int64, device=dev)]).to(torch.int32)
        plane_splits = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        plane_splits[1:] = torch.cumsum(chains[:, 0].to(torch.int64), dim=0)
        chained = rec[seg]                                                     # the records in chained order
        chained_words = chained.view(torch.int32)
        out = ContourList(plane_splits.to(torch.int32), chain_splits, (slots[:, 3][starts] & 1).to(torch.bool), chained[:, 0:3], chained[:, 4:7],
                          chained_words[:, 3], chained_words[:, 7], status[kept])
        return out, slots, chains

    def chainSections(self, scene, sections):
        """The segments of a SectionList (planeSections, slices) chained into contours: open polylines and closed loops per plane
        (drt_renderer_chain_sections).  The successor of a segment is the segment of the triangle across the edge it leaves
        through, looked up in the scene's edge adjacency (Scene.edgeAdjacency): integers only, no welding, no tolerance, and the
        result is the same bit for bit on every run.  A path starts at its record without a predecessor, a cycle at its record of
        smallest index; a plane's chains are ordered by their first record.  ContourList(splits [N + 1], chain_splits [C + 1],
        closed [C], p [M, 3], q [M, 3], prim [M], code [M], end [M]): the chains of plane i are splits[i]:splits[i + 1], chain c
        is the records chain_splits[c]:chain_splits[c + 1], gathered into chained order; end is each record's exit status (0 =
        linked, 1 = boundary edge, 2 = non-manifold or flipped edge, 3 = the neighbour is not in the list, 4 = the neighbour is cut
        through other edges).  A contour is closed exactly where neighbouring triangles agree on which of their shared vertices
        are above the plane.  No caps or filled polygons.  Device tensors in, device tensors out (enqueued on the current torch
        stream); numpy in, numpy out."""
        import torch                             # (only here: importing the package does not import torch)
        dev = torch.device("cuda", self._device)
        if not isinstance(sections, tuple) or len(sections) != 5:
            raise DrtError(ERR_INVALID, "a SectionList expected")
        from_numpy = isinstance(sections[0], np.ndarray)
        want = (("splits", np.int32, torch.int32), ("p", np.float32, torch.float32), ("q", np.float32, torch.float32),
                ("prim", np.int32, torch.int32), ("code", np.int32, torch.int32))
        parts = []
        for a, (what, np_type, torch_type) in zip(sections, want):
            if isinstance(a, np.ndarray) != from_numpy or not (from_numpy or torch.is_tensor(a)):
                raise DrtError(ERR_INVALID, "%s: numpy arrays or device tensors expected, not a mix" % what)
            if from_numpy:
                if a.dtype != np_type:
                    raise DrtError(ERR_INVALID, "%s: dtype %s, %s expected" % (what, a.dtype, np.dtype(np_type)))
                a = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            elif a.dtype != torch_type or a.device != dev:
                raise DrtError(ERR_INVALID, "%s: %s on %s, %s on %s expected" % (what, a.dtype, a.device, torch_type, dev))
            parts.append(a)
        res = self._chain(scene, SectionList(*parts))[0]
        if from_numpy:
            return ContourList(*(x.cpu().numpy().copy() for x in res))
        return res

    def contours(self, scene, normals, d=None):
        """planeSections followed by chainSections: the ContourList of the planes dot(n, x) = d, which remembers their normals for
        ContourList.areas().  Planes and conventions as planeSections."""
        import torch                             # (only here: importing the package does not import torch)
        dev = torch.device("cuda", self._device)
        planes, from_numpy = _plane_batch(torch, dev, normals, d)
        res = self._chain(scene, self._sections(scene, planes))[0]
        if from_numpy:
            res = ContourList(*(x.cpu().numpy().copy() for x in res))
        res.normals = planes[:, 0:3].cpu().numpy().copy() if from_numpy else planes[:, 0:3].clone()
        return res

    def _query_adjacency(self, torch, dev, n, tris, query_adj):
        """int32 [n, 3] on `dev`: query_adj as given (numpy or a tensor on `dev`), or the table of tris (triEdgeAdjacency)."""
        if query_adj is None:
            if tris is None:
                raise DrtError(ERR_INVALID, "one of tris and query_adj expected: the curve crosses queries through the query mesh's edge adjacency")
            if torch.is_tensor(tris) and tris.device == dev and tris.dtype == torch.float32:
                query_adj = self.edgeAdjacency(tris)      # made on the device: the same bytes
            else:
                query_adj = triEdgeAdjacency(tris)
        if isinstance(query_adj, np.ndarray):
            if query_adj.dtype != np.int32:
                raise DrtError(ERR_INVALID, "query_adj: dtype %s, int32 expected" % query_adj.dtype)
            query_adj = torch.from_numpy(np.ascontiguousarray(query_adj)).to(dev)
        elif not torch.is_tensor(query_adj) or query_adj.dtype != torch.int32 or query_adj.device != dev:
            raise DrtError(ERR_INVALID, "query_adj: a numpy array or a tensor on %s, int32, expected" % (dev,))
        if query_adj.numel() != 3 * n:
            raise DrtError(ERR_INVALID, "query_adj: %d values for %d queries, 3 per query expected" % (query_adj.numel(), n))
        return query_adj.contiguous()

    def _chain_cuts(self, cuts, scene, query_adj):
        """(CurveList of device tensors, slots [M, 4] int32, counts [3] int32) for a CutList of device tensors and the query mesh's
        table on the device: the records packed again as drt_isect, drt_renderer_chain_intersections, and the lists read off the
        slots."""
        import torch
        dev = torch.device("cuda", self._device)
        splits = cuts.splits.to(torch.int32).contiguous()
        n, total = splits.shape[0] - 1, cuts.prim.shape[0]
        if n < 0 or cuts.p.shape != (total, 3) or cuts.q.shape != (total, 3) or cuts.code.shape != (total,):
            raise DrtError(ERR_INVALID, "a CutList expected: splits [N + 1], p and q [M, 3], prim and code [M]")
        if total >= 2 ** 31:
            raise DrtError(ERR_INVALID, "%d segments in all: fewer than 2^31 expected (split the queries)" % total)
        rec = torch.empty((total, 8), dtype=torch.float32, device=dev)         # drt_isect: p, prim, q, code
        words = rec.view(torch.int32)
        rec[:, 0:3], rec[:, 4:7] = cuts.p, cuts.q
        words[:, 3], words[:, 7] = cuts.prim, cuts.code
        slots = torch.empty((total, 4), dtype=torch.int32, device=dev)
        counts = torch.zeros(3, dtype=torch.int32, device=dev)
        if n > 0 and total:
            stream = torch.cuda.current_stream(dev).cuda_stream
            _check(_lib.drt_renderer_chain_intersections(self._h, scene._h, rec.data_ptr(), splits.data_ptr(), query_adj.data_ptr(), slots.data_ptr(),
                                                         counts.data_ptr(), n, total, stream))
        else:
            slots[:, 0] = slots[:, 1] = torch.arange(total, dtype=torch.int32, device=dev)      # (no query: nothing is live)
            slots[:, 2], slots[:, 3] = 1, CHAIN_MISS << 1
        # what the slots say: a chain starts where first == position; records that are not live are dropped
        status = slots[:, 3] >> 1
        kept = status != CHAIN_MISS
        starts = (slots[:, 1] == torch.arange(total, dtype=torch.int32, device=dev)) & kept
        seg = slots[:, 0][kept].to(torch.int64)
        kept_before = torch.cumsum(kept.to(torch.int64), dim=0) - kept.to(torch.int64)
        chain_splits = torch.cat([kept_before[starts], torch.full((1,), seg.shape[0], dtype=torch.int64, device=dev)]).to(torch.int32)
        # the owning query: a CutList's ranges ascend and tile the list, so it is the number of range ends at or before the record
        query = torch.searchsorted(splits[1:].to(torch.int64).contiguous(), torch.arange(total, dtype=torch.int64, device=dev), right=True).to(torch.int32)
        chained = rec[seg]                                                     # the records in chained order
        chained_words = chained.view(torch.int32)
        out = CurveList(chain_splits, (slots[:, 3][starts] & 1).to(torch.bool), chained[:, 0:3], chained[:, 4:7], query[seg],
                        chained_words[:, 3], chained_words[:, 7], status[kept])
        return out, slots, counts

    def chainIntersections(self, scene, cuts, tris=None, query_adj=None):
        """The segments of a CutList (intersectTriangles) chained into curves: closed loops and open polylines over the whole batch
        (drt_renderer_chain_intersections).  A segment that leaves through an edge of the scene triangle continues in the triangle
        across that edge (Scene.edgeAdjacency) with the same query; one that leaves through an edge of the query continues in the
        same scene triangle with the query across that edge, looked up in the query mesh's own table: give the mesh the list was
        made with as tris, or its triEdgeAdjacency(tris) as query_adj (a table stays valid while the mesh moves rigidly or
        deforms without tearing).  Integers only, no welding, no tolerance, the same bytes on every run.  A path starts at its
        record without a predecessor, a cycle at its record of smallest index; the chains are ordered by their first record.
        CurveList(chain_splits [C + 1], closed [C], p [M, 3], q [M, 3], query [M], prim [M], code [M], end [M]) in chained order; end
        is each record's exit status as chainSections has it, here for either mesh (1 = a boundary edge, 2 = a non-manifold or
        flipped edge, 3 = the neighbour is not in the list, 4 = the neighbour is cut through other edges).  A curve is closed
        exactly where neighbouring triangles agree; one that runs through vertices or along edges falls into open chains.
        Self-intersection curves are not chained.  Device tensors in, device tensors out (enqueued on the current torch stream);
        numpy in, numpy out."""
        import torch                             # (only here: importing the package does not import torch)
        dev = torch.device("cuda", self._device)
        if not isinstance(cuts, tuple) or len(cuts) != 5:
            raise DrtError(ERR_INVALID, "a CutList expected")
        from_numpy = isinstance(cuts[0], np.ndarray)
        want = (("splits", np.int32, torch.int32), ("p", np.float32, torch.float32), ("q", np.float32, torch.float32),
                ("prim", np.int32, torch.int32), ("code", np.int32, torch.int32))
        parts = []
        for a, (what, np_type, torch_type) in zip(cuts, want):
            if isinstance(a, np.ndarray) != from_numpy or not (from_numpy or torch.is_tensor(a)):
                raise DrtError(ERR_INVALID, "%s: numpy arrays or device tensors expected, not a mix" % what)
            if from_numpy:
                if a.dtype != np_type:
                    raise DrtError(ERR_INVALID, "%s: dtype %s, %s expected" % (what, a.dtype, np.dtype(np_type)))
                a = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            elif a.dtype != torch_type or a.device != dev:
                raise DrtError(ERR_INVALID, "%s: %s on %s, %s on %s expected" % (what, a.dtype, a.device, torch_type, dev))
            parts.append(a)
        table = self._query_adjacency(torch, dev, parts[0].shape[0] - 1, tris, query_adj)
        res = self._chain_cuts(CutList(*parts), scene, table)[0]
        if from_numpy:
            return CurveList(*(x.cpu().numpy().copy() for x in res))
        return res

    def intersectionCurves(self, scene, tris, query_adj=None):
        """intersectTriangles followed by chainIntersections: the CurveList along which the mesh tris ([N, 3, 3] float32 or a packed
        [N, 12]) cuts the scene.  query_adj: the mesh's triEdgeAdjacency, to reuse the table for a moving tool; made from tris when
        not given.  The one synchronisation with the device is intersectTriangles' read of the total."""
        import torch                             # (only here: importing the package does not import torch)
        dev = torch.device("cuda", self._device)
        packed, from_numpy = _tri_batch(torch, dev, tris)
        table = self._query_adjacency(torch, dev, packed.shape[0], tris, query_adj)
        res = self._chain_cuts(self._cuts(scene, packed), scene, table)[0]
        if from_numpy:
            return CurveList(*(x.cpu().numpy().copy() for x in res))
        return res

    def _shells(self, scene):
        """Shells of device tensors (count a Python int): drt_renderer_shell_labels, and the per-shell arrays made with torch."""
        import torch
        dev = torch.device("cuda", self._device)
        n = _lib.drt_scene_triangle_count(scene._h)
        label = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        adj = torch.empty((max(n, 1), 3), dtype=torch.int32, device=dev)
        counts = torch.zeros(3, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        _check(_lib.drt_renderer_shell_labels(self._h, scene._h, label.data_ptr(), counts.data_ptr(), stream))
        _check(_lib.drt_renderer_edge_adjacency(self._h, scene._h, adj.data_ptr(), stream))
        label, adj = label[:n], adj[:n]
        count = int(counts[0])
        root = label == torch.arange(n, dtype=torch.int32, device=dev)
        dense = torch.cumsum(root.to(torch.int64), dim=0) - 1                  # a root's shell number: roots ascend with their labels
        index = dense[label.to(torch.int64)]
        per_shell = lambda per_tri: torch.zeros(count, dtype=torch.int64, device=dev).index_add_(0, index, per_tri.to(torch.int64)).to(torch.int32)
        triangles = per_shell(torch.ones(n, dtype=torch.int64, device=dev))
        open_edges, bad_edges = per_shell((adj == -1).sum(dim=1)), per_shell((adj == -2).sum(dim=1))
        return Shells(label, index.to(torch.int32), count, triangles, open_edges, bad_edges, (open_edges == 0) & (bad_edges == 0))

    def shells(self, scene, as_torch=False):
        """The shells of the mesh (drt_renderer_shell_labels): triangles joined through twin half-edges of Scene.edgeAdjacency();
        boundary edges and non-manifold, flipped or zero-length edges join nothing, nor does a shared vertex.  Shells(label [n],
        index [n], count, triangles [S], open_edges [S], bad_edges [S], watertight [S]) in tree order (Scene.triangleOrder() maps
        it to load order): label = the smallest triangle index of the triangle's shell, index = its dense shell number in ascending
        order of label, and per shell the number of triangles, of half-edges on the boundary (adjacency -1) and of bad ones (-2); a
        shell is watertight iff it has neither.  Integers only, the same bit for bit on every run.  The labels depend on the
        adjacency alone: the first call after a scene upload computes them (and waits for the device), later ones copy; a device
        refit keeps them.  as_torch=True: device tensors; else numpy arrays."""
        res = self._shells(scene)
        if as_torch:
            return res
        return Shells(*(x if isinstance(x, int) else x.cpu().numpy().copy() for x in res))

    def boundaryLoops(self, scene, as_torch=False):
        """The boundary of the mesh as loops (drt_renderer_boundary_loops): the half-edges without a twin, each followed by the one
        that leaves its end vertex on the boundary, found by rotating about that vertex through the adjacency -- integers only.
        LoopList(splits [L + 1], closed [L], half_edge [M], prim [M], edge [M], shell [L], end [M]): loop i is the records
        splits[i]:splits[i + 1] in walking order; half_edge = 3 * prim + edge runs from vertex `edge` to vertex (edge + 1) % 3 of
        triangle prim (tree order); shell = the dense shell number (Shells.index) of the loop's triangles; end = a record's exit
        status (CHAIN_LINKED, or CHAIN_NON_MANIFOLD where the rotation meets a bad edge: that loop stays open).  A path starts at
        its record without a predecessor, a cycle at its smallest half-edge; the loops are ordered by their first record."""
        import torch
        dev = torch.device("cuda", self._device)
        stream = torch.cuda.current_stream(dev).cuda_stream
        sh = self._shells(scene)
        counts = torch.zeros(3, dtype=torch.int32, device=dev)
        _check(_lib.drt_renderer_boundary_loops(self._h, scene._h, None, 0, counts.data_ptr(), stream))
        m = int(counts[0])
        slots = torch.empty((m, 4), dtype=torch.int32, device=dev)
        if m:
            _check(_lib.drt_renderer_boundary_loops(self._h, scene._h, slots.data_ptr(), m, counts.data_ptr(), stream))
        # what the slots say: a loop starts where first == position
        starts = slots[:, 1] == torch.arange(m, dtype=torch.int32, device=dev)
        first = torch.nonzero(starts).reshape(-1)
        splits = torch.cat([first, torch.full((1,), m, dtype=torch.int64, device=dev)]).to(torch.int32)
        half_edge = slots[:, 0]
        prim = torch.div(half_edge, 3, rounding_mode="floor")
        res = LoopList(splits, (slots[:, 3][first] & 1).to(torch.bool), half_edge, prim, half_edge - 3 * prim,
                       sh.index[prim[first].to(torch.int64)], slots[:, 3] >> 1)
        if as_torch:
            return res
        return LoopList(*(x.cpu().numpy().copy() for x in res))

    def shellTerms(self, scene):
        """float64 [n, 4] on the device: per triangle {c.x, c.y, c.z, w} with c = cross(e1, e2) and w = dot(v0, c) of the device's
        positions -- the refitted ones after Renderer.refit (drt_renderer_shell_terms; drt.h states the rounding)."""
        import torch
        dev = torch.device("cuda", self._device)
        n = _lib.drt_scene_triangle_count(scene._h)
        terms = torch.empty((max(n, 1), 4), dtype=torch.float64, device=dev)
        _check(_lib.drt_renderer_shell_terms(self._h, scene._h, terms.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
        return terms[:n]

    def shellMeasures(self, scene, as_torch=False):
        """Area, enclosed volume and area vector of every shell, float64: ShellMeasures(area [S], volume [S], area_vector [S, 3])
        in the order of Shells.index.  From shellTerms, sorted by shell (a stable sort) and summed on the device as sectionAreas
        sums: area = 0.5 * sum sqrt(dot(c, c)), volume = sum w / 6, area_vector = 0.5 * sum c.  The volume is signed (positive
        for outward faces) and means something for a watertight shell, whose area vector is near zero.  After Renderer.refit
        these are the measures of the refitted mesh."""
        import torch
        sh = self._shells(scene)
        terms = self.shellTerms(scene)
        index = sh.index.to(torch.int64)
        terms = terms[torch.sort(index, stable=True).indices]
        at = torch.zeros(sh.count + 1, dtype=torch.int64, device=terms.device)
        at[1:] = torch.cumsum(sh.triangles.to(torch.int64), dim=0)
        c = terms[:, 0:3]
        area = 0.5 * _segment_sums(torch, torch.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]), at)
        volume = _segment_sums(torch, terms[:, 3].contiguous(), at) / 6.0
        vector = 0.5 * torch.stack([_segment_sums(torch, c[:, k].contiguous(), at) for k in range(3)], dim=1)
        res = ShellMeasures(area, volume, vector)
        return res if as_torch else ShellMeasures(*(x.cpu().numpy().copy() for x in res))

    def topologySteps(self):
        """(enqueued, busy, hooks): the labelling steps of this renderer's last shell labelling (drt_renderer_topology_steps)."""
        out = (C.c_uint32 * 3)()
        _check(_lib.drt_renderer_topology_steps(self._h, out))
        return tuple(int(v) for v in out)

    def voxelize(self, scene, resolution, lo=None, hi=None):
        """Conservative surface voxelisation: a bool [Z, Y, X] device tensor, true where a triangle touches the (closed) cell, over
        the box (lo, hi), by default the scene's bounds.  resolution: an int or (X, Y, Z).  The cells are laid out as sdfGrid lays
        out its centres -- cell i of axis k has the centre lo[k] + (i + 0.5) * step and the half extent step / 2, step =
        (hi[k] - lo[k]) / resolution[k] -- and the boxes are made on the device and asked in mode DRT_OVERLAP_ANY."""
        import torch                             # (only here: importing the package does not import torch)
        dev = torch.device("cuda", self._device)
        res = (int(resolution),) * 3 if isinstance(resolution, (int, np.integer)) else tuple(int(v) for v in resolution)
        if len(res) != 3 or min(res) < 1:
            raise DrtError(ERR_INVALID, "resolution: a positive int or three of them expected")
        if lo is None or hi is None:
            nodes = scene.m_BVHNodes
            if len(nodes) == 0:
                raise DrtError(ERR_INVALID, "voxelize: an empty scene has no bounds; give lo and hi")
            lo = nodes[-1]["bmin"] if lo is None else lo                      # the root is the last node
            hi = nodes[-1]["bmax"] if hi is None else hi
        lo, hi = np.asarray(lo, np.float32).reshape(3), np.asarray(hi, np.float32).reshape(3)
        step = [float(hi[k] - lo[k]) / res[k] for k in range(3)]
        axes = [float(lo[k]) + (torch.arange(res[k], dtype=torch.float32, device=dev) + 0.5) * step[k] for k in range(3)]
        z, y, x = torch.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
        center = torch.stack([x, y, z], dim=-1).reshape(-1, 3)
        half = torch.tensor([0.5 * v for v in step], dtype=torch.float32, device=dev).expand(center.shape[0], 3)
        return self.overlapsAny(scene, center, half).reshape(res[2], res[1], res[0])

    @staticmethod
    def _inside_rule(rule):
        if rule not in INSIDE_RULES:
            raise DrtError(ERR_INVALID, "rule %r: 'parity' or 'winding' expected" % (rule,))
        return INSIDE_RULES[rule]

    def inside(self, scene, points, rule="parity", votes=False):
        """Whether each point lies inside the closed mesh (drt_renderer_inside): three fixed rays per point vote by the parity of
        their crossing count (rule="parity") or by their winding sum (rule="winding", which needs consistent orientation as well);
        bool [N], inside = two votes or more, or with votes=True the uint8 number of votes, 0..3.  points [N, 3] float32 (or packed
        [N, 4]; max_dist is ignored).  Device tensors in, device tensors out (enqueued on the current torch stream); numpy in, numpy
        out.  After refit(scene, positions) the moved geometry is the one queried.  A point on the surface has no defined answer."""
        import torch                             # (only here: importing the package does not import torch)
        dev = torch.device("cuda", self._device)
        rule = self._inside_rule(rule)
        packed, from_numpy = _point_batch(torch, dev, points, float("inf"))
        n = packed.shape[0]
        out = torch.empty(n, dtype=torch.uint8, device=dev)
        if n:
            stream = torch.cuda.current_stream(dev).cuda_stream
            _check(_lib.drt_renderer_inside(self._h, scene._h, packed.data_ptr(), out.data_ptr(), n, rule, stream))
        res = out if votes else out >= 2
        return res.cpu().numpy() if from_numpy else res

    def signedDistance(self, scene, points, max_dist=float("inf"), rule="parity"):
        """nearest(scene, points, max_dist) with side = -1 inside the closed mesh, +1 outside, by inside()'s vote
        (drt_renderer_signed_distance); miss records carry the sign too.  The signed distance is side * sqrt(d2)."""
        import torch                             # (only here: importing the package does not import torch)
        dev = torch.device("cuda", self._device)
        rule = self._inside_rule(rule)
        packed, from_numpy = _point_batch(torch, dev, points, max_dist)
        n = packed.shape[0]
        out = torch.empty((n, 8), dtype=torch.float32, device=dev)
        if n:
            stream = torch.cuda.current_stream(dev).cuda_stream
            _check(_lib.drt_renderer_signed_distance(self._h, scene._h, packed.data_ptr(), out.data_ptr(), n, rule, stream))
        if from_numpy:
            h = out.cpu().numpy()
            return Nearest(h[:, 0:3].copy(), h[:, 3].copy(), h.view(np.int32)[:, 4].copy(), h[:, 5].copy(), h[:, 6].copy(), h[:, 7].copy())
        return Nearest(out[:, 0:3], out[:, 3], out.view(torch.int32)[:, 4], out[:, 5], out[:, 6], out[:, 7])

    def sdfGrid(self, scene, resolution, lo=None, hi=None, rule="parity"):
        """A signed distance field: float32 [Z, Y, X] device tensor of side * sqrt(d2) at the cell centres of a grid over the box
        (lo, hi), by default the scene's bounds.  resolution: an int or (X, Y, Z).  The points are made on the device."""
        import torch                             # (only here: importing the package does not import torch)
        dev = torch.device("cuda", self._device)
        self._inside_rule(rule)
        res = (int(resolution),) * 3 if isinstance(resolution, (int, np.integer)) else tuple(int(v) for v in resolution)
        if len(res) != 3 or min(res) < 1:
            raise DrtError(ERR_INVALID, "resolution: a positive int or three of them expected")
        if lo is None or hi is None:
            nodes = scene.m_BVHNodes
            if len(nodes) == 0:
                raise DrtError(ERR_INVALID, "sdfGrid: an empty scene has no bounds; give lo and hi")
            lo = nodes[-1]["bmin"] if lo is None else lo                      # the root is the last node
            hi = nodes[-1]["bmax"] if hi is None else hi
        lo, hi = np.asarray(lo, np.float32).reshape(3), np.asarray(hi, np.float32).reshape(3)
        axes = [float(lo[k]) + (torch.arange(res[k], dtype=torch.float32, device=dev) + 0.5) * (float(hi[k] - lo[k]) / res[k]) for k in range(3)]
        z, y, x = torch.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
        near = self.signedDistance(scene, torch.stack([x, y, z], dim=-1).reshape(-1, 3), rule=rule)
        return (near.side * torch.sqrt(near.d2)).reshape(res[2], res[1], res[0])

    @staticmethod
    def _winding_beta(beta):
        try:
            beta = float(beta)
        except (TypeError, ValueError):
            beta = float("nan")
        if not beta >= 0.0:
            raise DrtError(ERR_INVALID, "beta %r: a number >= 0 (or inf) expected" % (beta,))
        return beta

    def windingNumbers(self, scene, points, beta=2.0):
        """The generalised winding number of each point (drt_renderer_winding_numbers): float32 [N], the triangles' signed solid
        angles at the point over 4 pi -- 1 inside and 0 outside a closed outward mesh, and a value that degrades smoothly, instead of
        flipping, where the mesh has holes.  Evaluated on the tree: a node farther than beta of its radii is replaced by one dipole
        term (first order); beta=inf is the exact sum over all triangles, beta=0 the root's dipole alone.  points [N, 3] float32 (or
        packed [N, 4]; max_dist is ignored).  Device tensors in, device tensors out (enqueued on the current torch stream); numpy in,
        numpy out.  After refit(scene, positions) the moved geometry is the one queried.  A point with a NaN or an infinity answers
        NaN.  What it is not: first order only; a point on the surface has no defined answer; orientation is still assumed per
        connected patch; no RendererGroup and no command line."""
        import torch                             # (only here: importing the package does not import torch)
        dev = torch.device("cuda", self._device)
        beta = self._winding_beta(beta)
        packed, from_numpy = _point_batch(torch, dev, points, float("inf"))
        n = packed.shape[0]
        out = torch.empty(n, dtype=torch.float32, device=dev)
        if n:
            stream = torch.cuda.current_stream(dev).cuda_stream
            _check(_lib.drt_renderer_winding_numbers(self._h, scene._h, packed.data_ptr(), n, beta, out.data_ptr(), stream))
        return out.cpu().numpy() if from_numpy else out

    def windingInside(self, scene, points, beta=2.0, threshold=0.5):
        """windingNumbers(scene, points, beta) >= threshold as bool [N] (drt_renderer_winding_inside): the inside test that a missing
        triangle or a hole does not break.  A point with a NaN or an infinity is outside."""
        import torch                             # (only here: importing the package does not import torch)
        dev = torch.device("cuda", self._device)
        beta = self._winding_beta(beta)
        packed, from_numpy = _point_batch(torch, dev, points, float("inf"))
        n = packed.shape[0]
        out = torch.empty(n, dtype=torch.uint8, device=dev)
        if n:
            stream = torch.cuda.current_stream(dev).cuda_stream
            _check(_lib.drt_renderer_winding_inside(self._h, scene._h, packed.data_ptr(), n, beta, float(threshold), out.data_ptr(), stream))
        res = out != 0
        return res.cpu().numpy() if from_numpy else res

    def windingSignedDistance(self, scene, points, max_dist=float("inf"), beta=2.0, threshold=0.5):
        """nearest(scene, points, max_dist) with side = -1 where windingNumbers(scene, points, beta) >= threshold, +1 elsewhere
        (drt_renderer_winding_signed_distance); miss records carry the sign too.  The signed distance is side * sqrt(d2)."""
        import torch                             # (only here: importing the package does not import torch)
        dev = torch.device("cuda", self._device)
        beta = self._winding_beta(beta)
        packed, from_numpy = _point_batch(torch, dev, points, max_dist)
        n = packed.shape[0]
        out = torch.empty((n, 8), dtype=torch.float32, device=dev)
        if n:
            stream = torch.cuda.current_stream(dev).cuda_stream
            _check(_lib.drt_renderer_winding_signed_distance(self._h, scene._h, packed.data_ptr(), n, beta, float(threshold), out.data_ptr(), stream))
        if from_numpy:
            h = out.cpu().numpy()
            return Nearest(h[:, 0:3].copy(), h[:, 3].copy(), h.view(np.int32)[:, 4].copy(), h[:, 5].copy(), h[:, 6].copy(), h[:, 7].copy())
        return Nearest(out[:, 0:3], out[:, 3], out.view(torch.int32)[:, 4], out[:, 5], out[:, 6], out[:, 7])

    def windingGrid(self, scene, resolution, lo=None, hi=None, beta=2.0):
        """A winding-number field: float32 [Z, Y, X] device tensor of windingNumbers at the cell centres of a grid over the box (lo, hi),
        by default the scene's bounds, laid out as sdfGrid's.  resolution: an int or (X, Y, Z).  The points are made on the device."""
        import torch                             # (only here: importing the package does not import torch)
        dev = torch.device("cuda", self._device)
        beta = self._winding_beta(beta)
        res = (int(resolution),) * 3 if isinstance(resolution, (int, np.integer)) else tuple(int(v) for v in resolution)
        if len(res) != 3 or min(res) < 1:
            raise DrtError(ERR_INVALID, "resolution: a positive int or three of them expected")
        if lo is None or hi is None:
            nodes = scene.m_BVHNodes
            if len(nodes) == 0:
                raise DrtError(ERR_INVALID, "windingGrid: an empty scene has no bounds; give lo and hi")
            lo = nodes[-1]["bmin"] if lo is None else lo                      # the root is the last node
            hi = nodes[-1]["bmax"] if hi is None else hi
        lo, hi = np.asarray(lo, np.float32).reshape(3), np.asarray(hi, np.float32).reshape(3)
        axes = [float(lo[k]) + (torch.arange(res[k], dtype=torch.float32, device=dev) + 0.5) * (float(hi[k] - lo[k]) / res[k]) for k in range(3)]
        z, y, x = torch.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
        return self.windingNumbers(scene, torch.stack([x, y, z], dim=-1).reshape(-1, 3), beta=beta).reshape(res[2], res[1], res[0])

    @staticmethod
    def _iso_arguments(level, lo, hi, border):
        """(level, lo [3], hi [3], border or NaN) of isosurface, checked: finite numbers."""
        def number(v, what):
            try:
                v = float(v)
            except (TypeError, ValueError):
                v = float("nan")
            if not np.isfinite(v):
                raise DrtError(ERR_INVALID, "%s: a finite number expected" % what)
            return v

        level = number(level, "level %r" % (level,))
        border = float("nan") if border is None else number(border, "border %r" % (border,))
        try:
            lo, hi = np.asarray(lo, np.float32).reshape(-1), np.asarray(hi, np.float32).reshape(-1)
        except (TypeError, ValueError):
            raise DrtError(ERR_INVALID, "lo and hi: three finite numbers each expected")
        if lo.shape != (3,) or hi.shape != (3,) or not (np.isfinite(lo).all() and np.isfinite(hi).all()):
            raise DrtError(ERR_INVALID, "lo and hi: three finite numbers each expected")
        return level, lo, hi, border

    def _iso_passes(self, field, grid, level, border, flip):
        """(splits [R + 1] int32, records [M, 12] float32) on the field's device: drt_renderer_isosurface's count, a cumulative sum on
        the device, the one read-back of the total, the fill."""
        import torch
        dev = field.device
        pad = 0 if np.isnan(border) else 2
        rows = (grid.dims[1] - 1 + pad) * (grid.dims[2] - 1 + pad)
        stream = torch.cuda.current_stream(dev).cuda_stream
        counts = torch.empty(rows, dtype=torch.int32, device=dev)
        _check(_lib.drt_renderer_isosurface(self._h, field.data_ptr(), C.byref(grid), level, border, 1 if flip else 0, None, None, 0,
                                            counts.data_ptr(), stream))
        splits = torch.zeros(rows + 1, dtype=torch.int64, device=dev)
        splits[1:] = torch.cumsum(counts.to(torch.int64), dim=0)
        total = int(splits[-1].item())           # the one synchronisation: the result's size
        if total >= 2 ** 31:
            raise DrtError(ERR_INVALID, "%d triangles in all: fewer than 2^31 expected (extract the field in parts)" % total)
        splits = splits.to(torch.int32)
        rec = torch.empty((total, 12), dtype=torch.float32, device=dev)       # drt_iso_tri: v[3][3], cube, code, 0
        if total:
            _check(_lib.drt_renderer_isosurface(self._h, field.data_ptr(), C.byref(grid), level, border, 1 if flip else 0, splits.data_ptr(),
                                                rec.data_ptr(), total, None, stream))
        return splits, rec

    def isosurface(self, field, level, lo, hi, flip=False, border=None):
        """A watertight triangle mesh of the surface f = level of a field (drt_renderer_isosurface): marching tetrahedra on the
        six-tetrahedron split of every cube of neighbouring samples.  field: float32 [Z, Y, X] whose sample (i, j, k) lies at
        lo + (idx + 0.5) * cell per component, cell = (hi - lo) / (X, Y, Z) in float32 -- what sdfGrid and windingGrid return for
        the same lo, hi.  A sample is above iff f >= level; a vertex on a lattice edge is always interpolated from the end with the
        smaller index, so every cube that shares the edge computes the same bits, and the mesh is a closed, consistently oriented
        2-manifold wherever it does not leave the grid.  Face normals point to the above side -- outward for a signed distance that
        is negative inside; flip=True reverses every triangle, for fields that are large inside, such as winding numbers.
        border=b (a finite number): one virtual layer of samples with that value surrounds the grid, so with b on the outside class
        every surface closes, whatever the field; None: a surface that reaches the grid's edge is open there.  A tetrahedron with a
        NaN or an infinity at a corner emits nothing.
        Isosurface(splits [R + 1] int32, tris [M, 3, 3] float32, cube [M], code [M] int32): row r (the cubes along x of one (y, z))
        owns [splits[r], splits[r + 1]); ascending cube, tetrahedron and table order, the same bytes on every run.  A count, a
        cumulative sum on the device, and a fill; the total is read back between them to size the result: that read is this call's
        one synchronisation with the device.  A device tensor in, device tensors out (enqueued on the current torch stream; tris is
        a strided view of the 48-byte records); numpy in, numpy out.  Needs no scene.
        What it is not: no vertex index buffer -- triangle soup with bit-equal shared positions, triEdgeAdjacency recovers the
        connectivity; a sample exactly equal to level is above, and zero-area triangles with zero-length edges appear there, which
        edgeAdjacency marks -2 -- shift level by an ulp or accept them; no gradient normals -- Isosurface.faceNormals gives face
        normals; roughly twice the triangles of marching cubes; the surface of the piecewise-linear interpolant and no better; no
        simplification, no smoothing and no dual or sharp-feature methods; no RendererGroup and no command line."""
        level, lo, hi, border = self._iso_arguments(level, lo, hi, border)
        import torch                             # (only here: importing the package does not import torch)
        dev = torch.device("cuda", self._device)
        if isinstance(field, np.ndarray):
            if field.dtype != np.float32:
                raise DrtError(ERR_INVALID, "field: dtype %s, float32 expected" % field.dtype)
            from_numpy = True
        elif torch.is_tensor(field):
            if field.dtype != torch.float32:
                raise DrtError(ERR_INVALID, "field: dtype %s, torch.float32 expected" % field.dtype)
            if field.device != dev:
                raise DrtError(ERR_INVALID, "field: on %s, the renderer is on %s" % (field.device, dev))
            from_numpy = False
        else:
            raise DrtError(ERR_INVALID, "field: a numpy array or a torch tensor expected")
        if field.ndim != 3:
            raise DrtError(ERR_INVALID, "field: shape %s, [Z, Y, X] expected" % (tuple(field.shape),))
        least = 2 if np.isnan(border) else 1
        if min(field.shape) < least:
            raise DrtError(ERR_INVALID, "field: shape %s, at least %d samples per axis expected" % (tuple(field.shape), least))
        f = torch.from_numpy(np.ascontiguousarray(field)).to(dev) if from_numpy else field.contiguous()
        grid = _Grid()
        res = (int(f.shape[2]), int(f.shape[1]), int(f.shape[0]))
        cell = ((hi - lo) / np.asarray(res, np.float32)).astype(np.float32)
        grid.lo[:], grid.cell[:], grid.dims[:] = [float(v) for v in lo], [float(v) for v in cell], res
        splits, rec = self._iso_passes(f, grid, level, border, bool(flip))
        words = rec.view(torch.int32)
        res = Isosurface(splits, rec[:, 0:9].unflatten(1, (3, 3)), words[:, 9], words[:, 10])
        if from_numpy:
            return Isosurface(*(x.cpu().numpy().copy() for x in res))
        return res

    def remesh(self, scene, resolution, field="winding", level=None, margin=1, **kw):
        """A closed, uniformly tessellated mesh of `scene`'s surface, also where the scene has holes: the Isosurface of a field of the
        scene sampled on a grid.  resolution: an int or (X, Y, Z), the cells across the scene's bounds; the grid is padded by
        `margin` (>= 0) cells of that size on every side, so that the field is sampled outside the mesh.  field="winding":
        windingGrid, level 0.5 by default and flip=True -- a scan with missing triangles comes out closed; field="sdf": sdfGrid,
        level 0 by default (level = +-d is an offset surface).  The grid gets a border on the outside class, so the result is closed
        whatever the field.  Further keywords go to windingGrid (beta) or sdfGrid (rule).  Device tensors come back; the scene needs
        its BVH."""
        if field not in ("winding", "sdf"):
            raise DrtError(ERR_INVALID, "field = %r: 'winding' or 'sdf' expected" % (field,))
        res = (resolution,) * 3 if isinstance(resolution, (int, np.integer)) and not isinstance(resolution, bool) else resolution
        try:
            ok = len(res) == 3 and all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) and v >= 1 for v in res)
        except TypeError:
            ok = False
        if not ok:
            raise DrtError(ERR_INVALID, "resolution = %r: a positive int or three of them expected" % (resolution,))
        if isinstance(margin, bool) or not isinstance(margin, (int, np.integer)) or margin < 0:
            raise DrtError(ERR_INVALID, "margin = %r: a non-negative integer expected" % (margin,))
        if level is None:
            level = 0.5 if field == "winding" else 0.0
        try:
            level = float(level)
        except (TypeError, ValueError):
            level = float("nan")
        if not np.isfinite(level):
            raise DrtError(ERR_INVALID, "level: a finite number expected")
        nodes = scene.m_BVHNodes
        if len(nodes) == 0:
            raise DrtError(ERR_INVALID, "remesh: an empty scene has no bounds")
        lo, hi = np.asarray(nodes[-1]["bmin"], np.float32), np.asarray(nodes[-1]["bmax"], np.float32)      # the root is the last node
        res = np.asarray([int(v) for v in res], np.int64)
        cell = ((hi - lo) / res.astype(np.float32)).astype(np.float32)
        lo, hi = (lo - np.float32(margin) * cell).astype(np.float32), (hi + np.float32(margin) * cell).astype(np.float32)
        res = tuple(int(v) for v in res + 2 * int(margin))
        if field == "winding":
            grid = self.windingGrid(scene, res, lo, hi, **kw)
            return self.isosurface(grid, level, lo, hi, flip=True, border=min(0.0, level - 1.0))      # outside: w = 0, below
        grid = self.sdfGrid(scene, res, lo, hi, **kw)
        return self.isosurface(grid, level, lo, hi, border=level + float(cell.max()))                 # outside: farther out, above

    def _indexed(self, torch, mesh):
        """(vertices [V, 3] float32, faces [N, 3] int32 on the renderer's device, contiguous, came_from_numpy) of an IndexedMesh or a
        (vertices, faces, ...) tuple, checked."""
        dev = torch.device("cuda", self._device)
        try:
            vertices, faces = mesh[0], mesh[1]
        except (TypeError, IndexError, KeyError):
            raise DrtError(ERR_INVALID, "mesh: an IndexedMesh or (vertices, faces) expected")
        out = []
        for a, what, np_dtype, dtype in ((vertices, "vertices", np.float32, torch.float32), (faces, "faces", np.int32, torch.int32)):
            if isinstance(a, np.ndarray):
                if a.dtype != np_dtype:
                    raise DrtError(ERR_INVALID, "%s: dtype %s, %s expected" % (what, a.dtype, np.dtype(np_dtype).name))
            elif torch.is_tensor(a):
                if a.dtype != dtype:
                    raise DrtError(ERR_INVALID, "%s: dtype %s, %s expected" % (what, a.dtype, dtype))
                if a.device != dev:
                    raise DrtError(ERR_INVALID, "%s: on %s, the renderer is on %s" % (what, a.device, dev))
            else:
                raise DrtError(ERR_INVALID, "%s: a numpy array or a torch tensor expected" % what)
            if a.ndim != 2 or a.shape[1] != 3:
                raise DrtError(ERR_INVALID, "%s: shape %s, [%s, 3] expected" % (what, tuple(a.shape), what[0].upper()))
            out.append(a)
        from_numpy = isinstance(vertices, np.ndarray)
        if from_numpy != isinstance(faces, np.ndarray):
            raise DrtError(ERR_INVALID, "vertices and faces: both numpy arrays or both torch tensors expected")
        if 3 * out[1].shape[0] >= 2 ** 31 or out[0].shape[0] >= 2 ** 31:
            raise DrtError(ERR_INVALID, "%d triangles, %d vertices: 3 N < 2^31 and V < 2^31 expected" % (out[1].shape[0], out[0].shape[0]))
        if from_numpy:
            return torch.from_numpy(np.ascontiguousarray(out[0])).to(dev), torch.from_numpy(np.ascontiguousarray(out[1])).to(dev), True
        return out[0].contiguous(), out[1].contiguous(), False

    def _soup(self, torch, tris):
        """(tensor on the renderer's device, stride 36 or 48, N, came_from_numpy) of a triangle soup -- an Isosurface, [N, 3, 3] float32
        or a packed [N, 12] (drt_tri) -- checked; a view of 48-byte records is read in place."""
        dev = torch.device("cuda", self._device)
        if isinstance(tris, Isosurface):
            tris = tris.tris
        if isinstance(tris, np.ndarray):
            if tris.dtype != np.float32:
                raise DrtError(ERR_INVALID, "tris: dtype %s, float32 expected" % tris.dtype)
            t, from_numpy = tris, True
        elif torch.is_tensor(tris):
            if tris.dtype != torch.float32:
                raise DrtError(ERR_INVALID, "tris: dtype %s, torch.float32 expected" % tris.dtype)
            if tris.device != dev:
                raise DrtError(ERR_INVALID, "tris: on %s, the renderer is on %s" % (tris.device, dev))
            t, from_numpy = tris, False
        else:
            raise DrtError(ERR_INVALID, "tris: an Isosurface, a numpy array or a torch tensor expected")
        shape = tuple(t.shape)
        if not ((len(shape) == 2 and shape[1] == 12) or (len(shape) == 3 and shape[1:] == (3, 3))):
            raise DrtError(ERR_INVALID, "tris: shape %s, [N, 3, 3] or a packed [N, 12] expected" % (shape,))
        if 3 * shape[0] >= 2 ** 31:
            raise DrtError(ERR_INVALID, "%d triangles: 3 N < 2^31 expected" % shape[0])
        if from_numpy:
            t = torch.from_numpy(np.ascontiguousarray(t)).to(dev)
        if len(shape) == 2:
            t, stride = t.contiguous(), 48
        elif shape[0] and t.stride() == (12, 3, 1):        # a view of 48-byte records, as Isosurface.tris is: read in place
            stride = 48
        else:
            t, stride = t.contiguous(), 36
        return t, stride, shape[0], from_numpy

    def weld(self, tris):
        """The index buffer of a triangle soup (drt_renderer_weld).  tris: an Isosurface, [N, 3, 3] float32 or a packed [N, 12]
        (drt_tri).  Two corners are the same vertex iff their three 32-bit words are equal as integers -- triEdgeAdjacency's notion
        of the same position: -0.0 and +0.0 differ, NaNs are compared by their bits, there is no tolerance and nothing is moved.
        Vertices are numbered by first appearance.  IndexedMesh(vertices [V, 3] float32, faces [N, 3] int32, first [V] int32); the
        result depends on the input bytes alone.  Made on the device in integers: a hash table of corner indices, a flag scan, a
        scatter; V is read back to size the result, which is this call's one synchronisation.  A device tensor in, device tensors out
        (enqueued on the current torch stream); numpy in, numpy out.  Needs no scene.
        What it is not: no tolerance -- positions that differ in one bit stay apart; no cotangent weights, no feature preservation,
        no simplification, no vertex-to-triangle lists; no boundary detection and no device edge adjacency from faces in this call
        -- boundaryVertices and edgeAdjacency are those; no RendererGroup and no command line."""
        import torch                             # (only here: importing the package does not import torch)
        dev = torch.device("cuda", self._device)
        t, stride, n, from_numpy = self._soup(torch, tris)
        stream = torch.cuda.current_stream(dev).cuda_stream
        faces = torch.empty((n, 3), dtype=torch.int32, device=dev)
        first = torch.empty(3 * n, dtype=torch.int32, device=dev)
        vertices = torch.empty((3 * n, 3), dtype=torch.float32, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        _check(_lib.drt_renderer_weld(self._h, t.data_ptr() if n else None, n, stride, faces.data_ptr() if n else None,
                                      first.data_ptr() if n else None, vertices.data_ptr() if n else None, 3 * n, count.data_ptr(), stream))
        v = int(count.item())                    # the one synchronisation: the result's size
        res = IndexedMesh(vertices[:v], faces, first[:v])
        if from_numpy:
            return IndexedMesh(*(x.cpu().numpy().copy() for x in res))
        return res

    def vertexNormals(self, mesh, weight="angle"):
        """float32 [V, 3]: unit vertex normals of an IndexedMesh (drt_renderer_vertex_normals).  weight="angle": every triangle's
        unit normal weighted by its interior angle at the vertex, which does not depend on how a surface is cut into triangles;
        "area": the triangles' area vectors.  The sums are 64-bit fixed point added with integer atomics, so the bytes do not depend
        on the order.  A triangle with an index outside [0, V), a coordinate that is not finite or no area adds nothing; a vertex
        that nothing is added to gets zeros.  Device tensors in, a device tensor out (enqueued on the current torch stream); numpy
        in, numpy out."""
        if weight not in NORMAL_WEIGHTS:
            raise DrtError(ERR_INVALID, "weight = %r: 'angle' or 'area' expected" % (weight,))
        import torch                             # (only here: importing the package does not import torch)
        vertices, faces, from_numpy = self._indexed(torch, mesh)
        dev = vertices.device
        out = torch.zeros_like(vertices)
        _check(_lib.drt_renderer_vertex_normals(self._h, vertices.data_ptr(), vertices.shape[0], faces.data_ptr() if len(faces) else None,
                                                faces.shape[0], NORMAL_WEIGHTS[weight], out.data_ptr(),
                                                torch.cuda.current_stream(dev).cuda_stream))
        return out.cpu().numpy() if from_numpy else out

    def smooth(self, mesh, iterations=10, lam=0.5, mu=-0.53, fixed=None, factors=None):
        """Laplacian / Taubin smoothing of an IndexedMesh (drt_renderer_smooth_vertices): an IndexedMesh with the same faces and
        first.  Every step moves a vertex by a factor f towards the mean of its triangles' other vertices (the umbrella operator,
        every edge of a closed manifold counted twice); `iterations` times the pair (lam, mu) -- Taubin's lambda | mu, which does
        not shrink as plain Laplacian smoothing does -- or, with mu=None, `iterations` steps of lam; factors=[...] gives the steps'
        factors outright, |f| <= 1 each.  fixed: bool or uint8 [V], vertices that stay, or "boundary" for boundaryVertices(mesh), the
        ends of the open edges.  The sums are 64-bit fixed point, so the bytes do not depend on the order; shared vertices stay
        shared, so a watertight mesh stays watertight.
        What it is not: no cotangent weights, no feature preservation, no boundary detection of its own (fixed="boundary" calls
        boundaryVertices), no simplification."""
        if factors is None:
            try:
                ok = not isinstance(iterations, bool) and int(iterations) == iterations and iterations >= 0
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise DrtError(ERR_INVALID, "iterations = %r: a non-negative integer expected" % (iterations,))
            factors = ([lam] if mu is None else [lam, mu]) * int(iterations)
        try:
            fac = np.asarray([float(f) for f in factors], np.float32)
        except (TypeError, ValueError):
            raise DrtError(ERR_INVALID, "factors: numbers expected")
        if not (np.abs(fac) <= 1).all():
            raise DrtError(ERR_INVALID, "factors %r: |f| <= 1 expected" % (fac.tolist(),))
        if isinstance(fixed, str) and fixed != "boundary":
            raise DrtError(ERR_INVALID, "fixed = %r: an array, None or 'boundary' expected" % (fixed,))
        import torch                             # (only here: importing the package does not import torch)
        vertices, faces, from_numpy = self._indexed(torch, mesh)
        dev = vertices.device
        fx = None
        if isinstance(fixed, str):
            fx = self._boundary_vertices(torch, vertices.shape[0], faces, None, False)
        elif fixed is not None:
            if isinstance(fixed, np.ndarray):
                fx = torch.from_numpy(np.ascontiguousarray(fixed != 0).view(np.uint8)).to(dev)
            elif torch.is_tensor(fixed):
                if fixed.device != dev:
                    raise DrtError(ERR_INVALID, "fixed: on %s, the renderer is on %s" % (fixed.device, dev))
                fx = (fixed != 0).to(torch.uint8).contiguous()
            else:
                raise DrtError(ERR_INVALID, "fixed: a numpy array or a torch tensor expected")
            if tuple(fx.shape) != (vertices.shape[0],):
                raise DrtError(ERR_INVALID, "fixed: shape %s, [%d] expected" % (tuple(fx.shape), vertices.shape[0]))
        out = torch.empty_like(vertices)
        _check(_lib.drt_renderer_smooth_vertices(self._h, vertices.data_ptr(), vertices.shape[0], faces.data_ptr() if len(faces) else None,
                                                 faces.shape[0], fac.ctypes.data if len(fac) else None, len(fac),
                                                 fx.data_ptr() if fx is not None else None, out.data_ptr(),
                                                 torch.cuda.current_stream(dev).cuda_stream))
        first = mesh[2] if len(mesh) > 2 and not isinstance(mesh, SubdividedMesh) else None      # (its third field is parents)
        return IndexedMesh(out.cpu().numpy() if from_numpy else out, mesh[1], first)

    def _adjacency(self, torch, key, t, stride, n, edges):
        """(adj [n, 3], edge [n, 3] or None, half_edge [E] or None, E) as device tensors: drt_renderer_tri_adjacency of the soup t
        (key "position") or drt_renderer_face_adjacency of the faces t (key "index"), on the current torch stream."""
        dev = torch.device("cuda", self._device)
        stream = torch.cuda.current_stream(dev).cuda_stream
        adj = torch.empty((n, 3), dtype=torch.int32, device=dev)
        edge = half_edge = count = None
        if edges:
            edge = torch.empty((n, 3), dtype=torch.int32, device=dev)
            half_edge = torch.empty(3 * n, dtype=torch.int32, device=dev)
            count = torch.zeros(1, dtype=torch.int32, device=dev)
        tail = (adj.data_ptr() if n else None, edge.data_ptr() if edges and n else None, half_edge.data_ptr() if edges and n else None,
                3 * n if edges else 0, count.data_ptr() if edges else None, stream)
        if key == "position":
            _check(_lib.drt_renderer_tri_adjacency(self._h, t.data_ptr() if n else None, n, stride, *tail))
        else:
            _check(_lib.drt_renderer_face_adjacency(self._h, t.data_ptr() if n else None, n, *tail))
        if not edges:
            return adj, None, None, 0
        e = int(count.item())                    # the one synchronisation: the result's size
        return adj, edge, half_edge[:e], e

    def edgeAdjacency(self, mesh, edges=False):
        """int32 [N, 3]: the edge adjacency of a mesh, made on the device (drt_renderer_face_adjacency / drt_renderer_tri_adjacency).
        mesh: an IndexedMesh, a SimplifiedMesh or a (vertices, faces) pair -- half-edges are matched by vertex index, no vertex is
        read -- or a triangle soup, [N, 3, 3] float32, a packed [N, 12] or an Isosurface -- matched by bit-equal positions, the bytes
        of triEdgeAdjacency(tris).  adj[t, e] is the twin half-edge 3 t' + e' of edge e (corner e to corner (e + 1) % 3) of triangle
        t, -1 on a boundary edge, -2 where three or more triangles meet, two run the same way, or the edge has zero length.  By
        index on weld(tris).faces and by position on tris the tables are equal.  edges=True: MeshEdges(adj, edge, half_edge, count)
        with the undirected edges numbered by first appearance; its euler(n_vertices) is V - E + F.  Integers only: a hash table of
        half-edge indices, two integer minima, a flag scan; the same bytes on every run.  Device tensors in, device tensors out
        (enqueued on the current torch stream; edges=True reads E back); numpy in, numpy out.  Needs no scene.
        What it is not: no vertex-to-triangle lists; no tolerance; no orientation repair -- triangles that disagree about an edge's
        direction get -2; no RendererGroup."""
        import torch                             # (only here: importing the package does not import torch)
        soup = isinstance(mesh, Isosurface) or isinstance(mesh, np.ndarray) or torch.is_tensor(mesh)
        if soup:
            t, stride, n, from_numpy = self._soup(torch, mesh)
            res = self._adjacency(torch, "position", t, stride, n, edges)
        else:
            _, faces, from_numpy = self._indexed(torch, mesh)
            res = self._adjacency(torch, "index", faces, 12, faces.shape[0], edges)
        if not edges:
            return res[0].cpu().numpy() if from_numpy else res[0]
        if from_numpy:
            return MeshEdges(*(x.cpu().numpy().copy() for x in res[:3]), res[3])
        return MeshEdges(*res)

    def _boundary_vertices(self, torch, n_vertices, faces, adj, bad):
        """uint8 [V] on the device: drt_renderer_boundary_vertices of faces (a device tensor) and adj (a device tensor or None: the
        faces' own table)."""
        dev = torch.device("cuda", self._device)
        n = faces.shape[0]
        if adj is None:
            adj = self._adjacency(torch, "index", faces, 12, n, False)[0]
        out = torch.empty(n_vertices, dtype=torch.uint8, device=dev)
        _check(_lib.drt_renderer_boundary_vertices(self._h, faces.data_ptr() if n else None, adj.data_ptr() if n else None, n, n_vertices,
                                                   1 if bad else 0, out.data_ptr() if n_vertices else None,
                                                   torch.cuda.current_stream(dev).cuda_stream))
        return out

    def boundaryVertices(self, mesh, adj=None, bad=False):
        """bool [V]: the vertices of an indexed mesh on its boundary (drt_renderer_boundary_vertices): True iff a half-edge with
        adj == -1 starts or ends at the vertex; bad=True counts adj == -2 as well.  adj: int32 [N, 3], edgeAdjacency(mesh) if None.  A
        triangle with an index outside [0, V) is skipped.  What smooth(fixed="boundary") keeps in place.  Device tensors in, a device
        tensor out; numpy in, numpy out."""
        import torch                             # (only here: importing the package does not import torch)
        vertices, faces, from_numpy = self._indexed(torch, mesh)
        dev = vertices.device
        if adj is not None:
            if isinstance(adj, np.ndarray):
                if adj.dtype != np.int32:
                    raise DrtError(ERR_INVALID, "adj: dtype %s, int32 expected" % adj.dtype)
                adj = torch.from_numpy(np.ascontiguousarray(adj)).to(dev)
            elif not torch.is_tensor(adj) or adj.dtype != torch.int32 or adj.device != dev:
                raise DrtError(ERR_INVALID, "adj: a numpy array or a tensor on %s, int32, expected" % (dev,))
            if adj.numel() != 3 * faces.shape[0]:
                raise DrtError(ERR_INVALID, "adj: %d values for %d triangles, 3 per triangle expected" % (adj.numel(), faces.shape[0]))
            adj = adj.contiguous()
        out = self._boundary_vertices(torch, vertices.shape[0], faces, adj, bool(bad)).to(torch.bool)
        return out.cpu().numpy() if from_numpy else out

    def adjacencyRoute(self):
        """How the uploaded scene's edge adjacency was made (drt_renderer_adjacency_route): 0 = there is no table yet, 1 = on the
        host (DRT_ADJACENCY=host when the renderer was created), 2 = on the device."""
        return int(_lib.drt_renderer_adjacency_route(self._h))

    @staticmethod
    def _simplify_grid(vertices, resolution, cell, lo, hi):
        """The drt_grid of Renderer.simplify's keywords; vertices: a float32 [V, 3] numpy array or None (an explicit box)."""
        def bad(what):
            return DrtError(ERR_INVALID, what)
        if (resolution is None) == (cell is None):
            raise bad("simplify: exactly one of resolution and cell expected")
        if (lo is None) != (hi is None):
            raise bad("lo and hi: both or neither expected")
        if resolution is not None:
            res = (resolution,) * 3 if isinstance(resolution, (int, np.integer)) and not isinstance(resolution, bool) else resolution
            try:
                ok = len(res) == 3 and all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) and v >= 1 for v in res)
            except TypeError:
                ok = False
            if not ok:
                raise bad("resolution = %r: a positive int or three of them expected" % (resolution,))
            res = np.asarray([int(v) for v in res], np.int64)
        else:
            try:
                cell = float(cell)
            except (TypeError, ValueError):
                cell = float("nan")
            if not (np.isfinite(np.float32(cell)) and np.float32(cell) > 0):
                raise bad("cell = %r: one finite edge length greater than 0 expected" % (cell,))
        if lo is not None:
            try:
                lo, hi = np.asarray(lo, np.float32).reshape(3), np.asarray(hi, np.float32).reshape(3)
            except (TypeError, ValueError):
                raise bad("lo and hi: three numbers each expected")
            if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi > lo).all()):
                raise bad("lo and hi: finite values with lo < hi expected")
            if resolution is not None:
                size = ((hi - lo) / res.astype(np.float32)).astype(np.float32)      # the isosurface's rule: nothing is padded
            else:
                size = np.full(3, cell, np.float32)
                res = np.maximum(1, np.ceil((hi.astype(np.float64) - lo.astype(np.float64)) / np.float64(size[0]))).astype(np.int64)
        else:
            # the default box: lo = the smallest finite coordinate per axis, e = the largest - lo in float64, widened by 2^-16 of itself
            # at the upper end so that (p - lo) / cell < dims also after the three fp32 roundings of the rule (2^-24 each)
            finite = vertices[np.isfinite(vertices).all(axis=1)] if vertices is not None and len(vertices) else np.zeros((0, 3), np.float32)
            if len(finite):
                low = finite.min(axis=0).astype(np.float64)
                e = finite.max(axis=0).astype(np.float64) - low
            else:
                low, e = np.zeros(3), np.zeros(3)
            lo, pad = low.astype(np.float32), e * (1.0 + 2.0 ** -16)
            if resolution is not None:
                size = np.where(e > 0, pad / res, 1.0).astype(np.float32)             # a flat axis: one cell of size 1 holds it
            else:
                size = np.full(3, cell, np.float32)
                res = np.maximum(1, np.ceil(pad / np.float64(size[0]))).astype(np.int64)
        if not (np.isfinite(size).all() and (size > 0).all()):
            raise bad("cell size %r: finite and greater than 0 expected (is the box too small or too large for float32?)" % (size.tolist(),))
        if int(res[0]) * int(res[1]) * int(res[2]) >= 2 ** 31:
            raise bad("a grid of %d x %d x %d cells: fewer than 2^31 expected" % tuple(int(v) for v in res))
        grid = _Grid()
        grid.lo[:], grid.cell[:], grid.dims[:] = [float(v) for v in lo], [float(v) for v in size], [int(v) for v in res]
        return grid

    def simplify(self, mesh, resolution=None, cell=None, lo=None, hi=None, placement="quadric"):
        """A smaller mesh by vertex clustering (drt_renderer_simplify): the vertices in one cell of a grid become one vertex, and the
        triangles that still have three different vertices survive, in input order.  mesh: an IndexedMesh or (vertices, faces), as
        vertexNormals takes it.  resolution: an int or (X, Y, Z), the cells across [lo, hi]; or cell: one edge length, with the cell
        counts derived from it.  lo, hi: the box; vertices outside it, and vertices that are not finite, stay as they are, so a box
        over part of a mesh simplifies that part.  With an explicit box cell = (hi - lo) / resolution in float32, as for isosurface,
        and a vertex on hi is outside.  The default box holds every finite vertex: lo is the smallest finite coordinate per axis
        and the extent e = largest - lo is widened by e 2^-16 at the upper end (cell = e (1 + 2^-16) / resolution, or
        ceil(e (1 + 2^-16) / cell) cells), more than the rule's three float32 roundings can take back; an axis without extent gets
        one cell layer of size 1.
        placement="quadric": the point of the cell that minimises the summed squared distances to the planes of the cluster's
        triangles, area-weighted and drawn to the mean where the planes leave it free (Lindstrom), so corners and edges come back;
        an optimum outside its cell falls back to the mean.  "mean": the mean of the members.  The sums are 64-bit fixed point
        added with integer atomics and the finish is float64, so the result depends on the input bytes alone.
        SimplifiedMesh(vertices [C, 3], faces [M, 3], first [C], cluster [V], source [M]); a closed oriented mesh in gives a mesh in
        which every directed edge (a, b) appears as often as (b, a).  The call allocates V and N as capacities and reads the two
        counts back once -- its one synchronisation -- then slices.  (The default box of device tensors is made on the device and
        its six numbers are read back first, because the grid is host memory: pass lo and hi to avoid that second wait.)  Device
        tensors in, device tensors out (enqueued on the current torch stream); numpy in, numpy out.  Needs no scene.
        What it is not: no edge collapse, no error bound and no target count; duplicate and opposite triangle pairs stay;
        non-manifold edges that clustering creates are not repaired; no attribute quadrics, no interpolated normals or uvs; no
        adaptive cells; no RendererGroup and no command line."""
        if placement not in SIMPLIFY_PLACEMENTS:
            raise DrtError(ERR_INVALID, "placement = %r: 'mean' or 'quadric' expected" % (placement,))
        if lo is not None and hi is not None:
            grid = self._simplify_grid(None, resolution, cell, lo, hi)
        else:
            grid = None
            self._simplify_grid(np.zeros((0, 3), np.float32), resolution, cell, lo, hi)      # the keywords' own errors first
        import torch                             # (only here: importing the package does not import torch)
        vertices, faces, from_numpy = self._indexed(torch, mesh)
        dev = vertices.device
        if grid is None:
            if from_numpy:
                host = np.ascontiguousarray(mesh[0])
            elif len(vertices):                  # the box of the finite vertices, made on the device: six numbers come back
                fin = torch.isfinite(vertices).all(dim=1, keepdim=True)
                inf = torch.tensor(float("inf"), device=dev)
                host = torch.stack([torch.where(fin, vertices, inf).amin(dim=0), torch.where(fin, vertices, -inf).amax(dim=0)]).cpu().numpy()
            else:
                host = np.zeros((0, 3), np.float32)
            grid = self._simplify_grid(host, resolution, cell, None, None)
        nv, nt = int(vertices.shape[0]), int(faces.shape[0])
        stream = torch.cuda.current_stream(dev).cuda_stream
        cluster = torch.empty(nv, dtype=torch.int32, device=dev)
        out_v = torch.empty((nv, 3), dtype=torch.float32, device=dev)
        first = torch.empty(nv, dtype=torch.int32, device=dev)
        out_f = torch.empty((nt, 3), dtype=torch.int32, device=dev)
        source = torch.empty(nt, dtype=torch.int32, device=dev)
        counts = torch.zeros(2, dtype=torch.int32, device=dev)
        _check(_lib.drt_renderer_simplify(self._h, vertices.data_ptr() if nv else None, nv, faces.data_ptr() if nt else None, nt, C.byref(grid),
                                          SIMPLIFY_PLACEMENTS[placement], cluster.data_ptr() if nv else None,
                                          out_v.data_ptr() if nv else None, first.data_ptr() if nv else None, nv,
                                          out_f.data_ptr() if nt else None, source.data_ptr() if nt else None, nt, counts.data_ptr(), stream))
        c, m = (int(x) for x in counts.tolist())  # the one synchronisation: the result's sizes
        res = SimplifiedMesh(out_v[:c], out_f[:m], first[:c], cluster, source[:m])
        if from_numpy:
            return SimplifiedMesh(*(x.cpu().numpy().copy() for x in res))
        return res

    def subdivide(self, mesh, levels=1, scheme="loop"):
        """A finer mesh (drt_renderer_subdivide): every triangle becomes four, `levels` times.  mesh: an IndexedMesh, a SimplifiedMesh,
        a SubdividedMesh or a (vertices, faces) pair, as simplify and smooth take it.  scheme="loop": Loop subdivision with Warren's
        weights -- a new vertex on an interior edge at 3/8 3/8 1/8 1/8 of the edge's ends and the two opposite corners, an old vertex
        drawn towards its neighbours, so the surface converges to a smooth one; the open edges, and the edges where three or more
        triangles meet or two run the same way, are creases: their new vertices are midpoints and their old vertices follow the curve
        rule 1/8 6/8 1/8, or stay where they are if they have other than two such edges.  scheme="midpoint": the same topology with
        the old vertices left alone and the new ones at the midpoints -- what one wants before displacement, or before smooth or
        simplify on a finer grid.  The connectivity is edgeAdjacency's by index: the vertex of edge e is V + e, V' = V + E and
        V' - E' + F' = V - E + F; a closed oriented manifold stays one.  The sums are 64-bit fixed point added with integer atomics
        and the weights are applied in float64, so the result depends on the input bytes alone.  A vertex or an edge with an index
        out of range or a coordinate that is not finite is passed through or becomes NaNs; nothing faults.
        SubdividedMesh(vertices [V', 3], faces [4 N, 3], parents [V', 2]); parents is the last level's, and levels=0 returns the
        input's arrays with parents None.  Each level allocates V + 3 N vertices as the capacity and costs one read-back of
        vertex_count to size the result -- its one synchronisation.  Device tensors in, device tensors out (enqueued on the current
        torch stream); numpy in, numpy out.  Needs no scene.
        What it is not: no Catmull-Clark, Butterfly or sqrt(3); no user crease tags or sharpness; no limit-surface projection or
        limit normals; no adaptive refinement; no attribute interpolation beyond parents and the child order; no RendererGroup and
        no command line."""
        try:
            ok = not isinstance(levels, bool) and int(levels) == levels and levels >= 0
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise DrtError(ERR_INVALID, "levels = %r: a non-negative integer expected" % (levels,))
        if not isinstance(scheme, str) or scheme not in SUBDIVIDE_SCHEMES:
            raise DrtError(ERR_INVALID, "scheme = %r: 'loop' or 'midpoint' expected" % (scheme,))
        import torch                             # (only here: importing the package does not import torch)
        vertices, faces, from_numpy = self._indexed(torch, mesh)
        if int(levels) == 0:
            return SubdividedMesh(mesh[0], mesh[1], None)
        dev = vertices.device
        stream = torch.cuda.current_stream(dev).cuda_stream
        parents = None
        for _ in range(int(levels)):
            nv, nt = int(vertices.shape[0]), int(faces.shape[0])
            cap = nv + 3 * nt
            out_v = torch.empty((cap, 3), dtype=torch.float32, device=dev)
            parents = torch.empty((cap, 2), dtype=torch.int32, device=dev)
            out_f = torch.empty((4 * nt, 3), dtype=torch.int32, device=dev)
            count = torch.zeros(1, dtype=torch.int32, device=dev)
            _check(_lib.drt_renderer_subdivide(self._h, vertices.data_ptr() if nv else None, nv, faces.data_ptr() if nt else None, nt,
                                               SUBDIVIDE_SCHEMES[scheme], out_v.data_ptr() if cap else None,
                                               parents.data_ptr() if cap else None, cap, out_f.data_ptr() if nt else None,
                                               count.data_ptr(), stream))
            total = int(count.item())            # the level's one synchronisation: the result's size
            vertices, faces, parents = out_v[:total], out_f, parents[:total]
        res = SubdividedMesh(vertices, faces, parents)
        if from_numpy:
            return SubdividedMesh(*(x.cpu().numpy().copy() for x in res))
        return res

    def debugWindingMoments(self, scene):
        """The node moments the winding calls use for this renderer's copy of `scene` (drt_debug_winding_moments): float32 [nodes, 8]
        = {N[3], r2, p[3], pad}, the interior nodes in the host scene's node order, then the leaves in node order."""
        count = C.c_uint32(0)
        _check(_lib.drt_debug_winding_moments(self._h, scene._h, None, 0, C.byref(count)))
        out = np.zeros((count.value, 8), np.float32)
        _check(_lib.drt_debug_winding_moments(self._h, scene._h, out.ctypes.data, out.size, C.byref(count)))
        return out

    def renderGuides(self, cam, scene, frame_index=1, as_torch=False):
        """First-hit guide buffers of frame `frame_index` (drt_renderer_render_guides): Guides(albedo [H, W, 3], normal [H, W, 3],
        t [H, W], prim [H, W] int32), row 0 = bottom.  as_torch=True: device tensors, the work enqueued on the current torch stream;
        else numpy arrays."""
        import torch                             # (only here: importing the package does not import torch)
        dev = torch.device("cuda", self._device)
        self._push_settings()                    # (the sky colour and intensity of a miss come from the settings)
        g = torch.empty((self.getBufferHeight(), self.getBufferWidth(), 8), dtype=torch.float32, device=dev)
        pod = cam._pod()
        stream = torch.cuda.current_stream(dev).cuda_stream
        _check(_lib.drt_renderer_render_guides(self._h, C.byref(pod), scene._h, int(frame_index), g.data_ptr(), stream))
        if not as_torch:
            h = g.cpu().numpy()
            return Guides(h[..., 0:3].copy(), h[..., 4:7].copy(), h[..., 3].copy(), h.view(np.int32)[..., 7].copy())
        return Guides(g[..., 0:3], g[..., 4:7], g[..., 3], g.view(torch.int32)[..., 7])

    def refit(self, scene, positions, normals=None):
        """Refit this renderer's device copy of `scene` to new vertex positions [n, 3, 3] float32 in load order (normals the same,
        None = the last ones given, else the scene's): drt_renderer_refit.  Device tensors stay on the device and order with the
        current torch stream; numpy arrays are uploaded.  Blocking; returns the device ms.  The host scene is not changed."""
        import torch                             # (only here: importing the package does not import torch)
        dev = torch.device("cuda", self._device)
        n = _lib.drt_scene_triangle_count(scene._h)
        args = []
        for what, a in (("positions", positions), ("normals", normals)):
            if a is None:
                args.append(None)
                continue
            if isinstance(a, np.ndarray):
                a = torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
            elif not torch.is_tensor(a):
                raise DrtError(ERR_INVALID, "%s: a numpy array or a torch tensor expected" % what)
            if a.dtype != torch.float32 or a.device != dev or a.numel() != 9 * n:
                raise DrtError(ERR_INVALID, "%s: %s %s with %d values, float32 [%d, 3, 3] on %s expected" % (what, a.dtype, a.device, a.numel(), n, dev))
            args.append(a.contiguous())
        ms = C.c_float(0)
        stream = torch.cuda.current_stream(dev).cuda_stream
        _check(_lib.drt_renderer_refit(self._h, scene._h, args[0].data_ptr(), args[1].data_ptr() if args[1] is not None else None,
                                       C.byref(ms), stream))
        return ms.value

    def cameraRays(self, cams, width, height, frame_index=1, as_torch=False):
        """RayGen's primary rays of every camera and pixel in frame `frame_index` (drt_renderer_camera_rays): float32 [K, H, W, 8]
        = org, seed (uint32 bits), dir, exposure; row 0 = bottom.  `cams`: a Camera or a list of K.  as_torch=True: a device tensor,
        the work enqueued on the current torch stream; else a numpy array."""
        import torch                             # (only here: importing the package does not import torch)
        dev = torch.device("cuda", self._device)
        cams = [cams] if isinstance(cams, Camera) else list(cams)
        pods = (_CameraPOD * max(len(cams), 1))(*[c._pod() for c in cams])
        rays = torch.empty((len(cams), int(height), int(width), 8), dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        _check(_lib.drt_renderer_camera_rays(self._h, pods, len(cams), int(width), int(height), int(frame_index),
                                             rays.data_ptr() if rays.numel() else None, stream))
        return rays if as_torch else rays.cpu().numpy()

    def radiance(self, scene, rays, out=None, accumulate=False):
        """One path-traced sample of every ray with the current settings and material model (drt_renderer_radiance).  rays:
        float32 [..., 8] (org, seed bits, dir, exposure), a numpy array or a device tensor; returns float32 [..., 4] = (c, 1).
        out: an array / tensor of that shape (same kind as rays) to write into instead; accumulate=True adds c to its rgb and
        keeps its alpha.  Device tensors order with the current torch stream; numpy in, numpy out."""
        import torch                             # (only here: importing the package does not import torch)
        dev = torch.device("cuda", self._device)
        from_numpy = isinstance(rays, np.ndarray)
        if from_numpy:
            if rays.dtype != np.float32:
                raise DrtError(ERR_INVALID, "rays: dtype %s, float32 expected" % rays.dtype)
            r = torch.from_numpy(np.ascontiguousarray(rays)).to(dev)
        elif torch.is_tensor(rays):
            if rays.dtype != torch.float32 or rays.device != dev:
                raise DrtError(ERR_INVALID, "rays: %s on %s, torch.float32 on %s expected" % (rays.dtype, rays.device, dev))
            r = rays.contiguous()
        else:
            raise DrtError(ERR_INVALID, "rays: a numpy array or a torch tensor expected")
        if r.dim() < 1 or r.shape[-1] != 8:
            raise DrtError(ERR_INVALID, "rays: shape %s, [..., 8] expected" % (tuple(r.shape),))
        shape = tuple(r.shape[:-1]) + (4,)
        if accumulate and out is None:
            raise DrtError(ERR_INVALID, "accumulate needs `out`")
        if out is None:
            o = torch.empty(shape, dtype=torch.float32, device=dev)
        elif isinstance(out, np.ndarray) != from_numpy or (not from_numpy and not torch.is_tensor(out)):
            raise DrtError(ERR_INVALID, "out: the same kind as rays (numpy array or device tensor) expected")
        elif tuple(out.shape) != shape:
            raise DrtError(ERR_INVALID, "out: shape %s, %s expected" % (tuple(out.shape), shape))
        elif from_numpy:
            if out.dtype != np.float32:
                raise DrtError(ERR_INVALID, "out: dtype %s, float32 expected" % out.dtype)
            o = torch.from_numpy(np.ascontiguousarray(out)).to(dev)
        else:
            if out.dtype != torch.float32 or out.device != dev or not out.is_contiguous() or out.data_ptr() % 16:
                raise DrtError(ERR_INVALID, "out: a contiguous, 16-byte aligned torch.float32 tensor on %s expected" % dev)
            o = out
        n = r.numel() // 8
        if r.data_ptr() % 16:
            r = r.clone()
        self._push_settings()
        stream = torch.cuda.current_stream(dev).cuda_stream
        if n:
            _check(_lib.drt_renderer_radiance(self._h, scene._h, r.data_ptr(), o.data_ptr(), n, 1 if accumulate else 0, stream))
        if not from_numpy:
            return o
        h = o.cpu().numpy()
        if out is None:
            return h
        out[...] = h
        return out

    def renderViews(self, cams, scene, width, height, spp, as_torch=False):
        """`spp` frames of K cameras at width x height (frames 1..spp): per frame one camera_rays launch for all cameras and one
        accumulating radiance launch over K*H*W rays; returns accum / spp with alpha 1, float32 [K, H, W, 4], row 0 = bottom.
        Each view equals what a renderer that rendered that camera alone (ResizeBuffer, reset, spp frames) shows."""
        import torch                             # (only here: importing the package does not import torch)
        if int(spp) < 1:
            raise DrtError(ERR_INVALID, "spp >= 1 expected")
        dev = torch.device("cuda", self._device)
        cams = [cams] if isinstance(cams, Camera) else list(cams)
        acc = torch.zeros((len(cams), int(height), int(width), 4), dtype=torch.float32, device=dev)
        for f in range(1, int(spp) + 1):
            rays = self.cameraRays(cams, width, height, f, as_torch=True)
            self.radiance(scene, rays, out=acc, accumulate=True)
        if as_torch:
            # RenderKernel.cu:30, one correctly rounded fp32 division: torch's fp32 division on the device is not, the fp64 quotient
            # of two floats rounded once to fp32 is (53 >= 2 * 24 + 2 bits)
            img = (acc.double() / float(spp)).float()
            img[..., 3] = 1.0
            return img
        img = acc.cpu().numpy()
        img[..., :3] = img[..., :3] / np.float32(spp)
        img[..., 3] = 1.0
        return img

    def debugReadDeviceScene(self, scene):
        """The renderer's current device records, shaped as Scene.debugPack() (drt_debug_read_device_scene)."""
        nodes = scene.m_BVHNodes
        inner = np.zeros((int((nodes["is_leaf"] == 0).sum()), 64), np.uint8)
        hot = np.zeros((_lib.drt_scene_triangle_count(scene._h), 48), np.uint8)
        root = np.zeros(6, np.float32)
        _check(_lib.drt_debug_read_device_scene(self._h, inner.ctypes.data, inner.size, hot.ctypes.data, hot.size, root.ctypes.data))
        return inner, hot, root

    def Denoise(self, cam, scene, iterations=5, sigma_color=0.5, sigma_normal=0.1, sigma_albedo=0.1):
        """Edge-avoiding a-trous filter of the current framebuffer, guided by frame 1's albedo and normal (drt_renderer_denoise):
        float32 [H, W, 4], row 0 = bottom.  The framebuffer and the accumulation are left as they are."""
        self._push_settings()
        p = DenoiseParams(iterations=int(iterations), sigma_color=float(sigma_color), sigma_normal=float(sigma_normal),
                          sigma_albedo=float(sigma_albedo))
        ms = C.c_float(0)
        pod = cam._pod()
        _check(_lib.drt_renderer_denoise(self._h, C.byref(pod), scene._h, C.byref(p), C.byref(ms)))
        self.m_LastDenoiseMs = ms.value
        return self.GetDenoisedImage()

    def GetDenoisedImage(self):
        """The last Denoise result as numpy float32 [H, W, 4] (drt_renderer_read_denoised_rgba32f)."""
        out = np.zeros((self.getBufferHeight(), self.getBufferWidth(), 4), np.float32)
        _check(_lib.drt_renderer_read_denoised_rgba32f(self._h, out.ctypes.data, out.size))
        return out

    def DeviceDenoisedTarget(self):
        """Device address of the last Denoise result (float4 [H * W]), None before the first Denoise."""
        return _lib.drt_renderer_device_denoised(self._h)

    def TemporalDenoise(self, cam, scene, **params):
        """Temporal reprojection, moment accumulation and the variance-guided a-trous filter of the current framebuffer
        (drt_renderer_temporal_denoise; `params` = TemporalParams fields): float32 [H, W, 4], row 0 = bottom.  Call once per
        rendered pose; the per-pixel history travels from call to call through the first-hit geometry."""
        self._push_settings()
        p = TemporalParams(**params)
        ms = C.c_float(0)
        pod = cam._pod()
        _check(_lib.drt_renderer_temporal_denoise(self._h, C.byref(pod), scene._h, C.byref(p), C.byref(ms)))
        self.m_LastTemporalMs = ms.value
        return self.GetDenoisedImage()

    def resetTemporalHistory(self):
        """Drop the temporal history (drt_renderer_temporal_reset): the next TemporalDenoise starts at N = 1."""
        _check(_lib.drt_renderer_temporal_reset(self._h))

    def GetTemporalHistory(self):
        """The history the last TemporalDenoise stored: TemporalHistory(color [H, W, 3], length [H, W], moments [H, W, 2],
        variance [H, W], weight [H, W]) -- the unfiltered integrated colour, N, (m1, m2), the variance and the sum of the
        valid taps' weights (drt_renderer_read_temporal)."""
        H, W = self.getBufferHeight(), self.getBufferWidth()
        c, m = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32)
        _check(_lib.drt_renderer_read_temporal(self._h, 0, c.ctypes.data, c.size))
        _check(_lib.drt_renderer_read_temporal(self._h, 1, m.ctypes.data, m.size))
        return TemporalHistory(c[..., :3].copy(), c[..., 3].copy(), m[..., :2].copy(), m[..., 2].copy(), m[..., 3].copy())

    def DeviceTemporalHistory(self, which=0):
        """Device address of the history's colour (which 0) or moments (1) records, None before the first TemporalDenoise."""
        return _lib.drt_renderer_device_temporal(self._h, int(which))

    def Upscale(self, cam, scene, width, height, **params):
        """Joint-bilateral upsampling of the frame to width x height, steered by the first-hit guides of both sizes
        (drt_renderer_upscale; `params` = UpscaleParams fields: source 0 = the framebuffer, 1 = the last Denoise / TemporalDenoise
        result): float32 [height, width, 4], row 0 = bottom.  The renderer's own buffers are left as they are."""
        self._push_settings()
        p = UpscaleParams(**params)
        ms = C.c_float(0)
        pod = cam._pod()
        _check(_lib.drt_renderer_upscale(self._h, C.byref(pod), scene._h, int(width), int(height), C.byref(p), C.byref(ms)))
        self.m_LastUpscaleMs = ms.value
        self._upscaled_size = (int(width), int(height))
        return self.GetUpscaledImage()

    def GetUpscaledImage(self):
        """The last Upscale result as numpy float32 [Ho, Wo, 4] (drt_renderer_read_upscaled_rgba32f)."""
        w, h = self._upscaled_size
        out = np.zeros((h, w, 4), np.float32)
        _check(_lib.drt_renderer_read_upscaled_rgba32f(self._h, out.ctypes.data, out.size))
        return out

    def DeviceUpscaledTarget(self):
        """Device address of the last Upscale result (float4 [Ho * Wo]), None before the first Upscale."""
        return _lib.drt_renderer_device_upscaled(self._h)

    def RenderAdaptive(self, cam, scene, spp=4.0, **params):
        """One adaptive call (drt_renderer_render_adaptive; `params` = AdaptiveParams fields): int(spp * W * H) samples -- or
        `budget` if given -- go where the per-pixel state says the noise is; the framebuffer then shows sum / n of every pixel.
        The first call after a reset or resize is uniform.  Returns the AdaptiveInfo (samples, active_pixels, max_count, ms)."""
        self._push_settings()
        if "budget" not in params:
            params["budget"] = int(spp * self.getBufferWidth() * self.getBufferHeight())
        p = AdaptiveParams(**params)
        info = AdaptiveInfo()
        pod = cam._pod()
        _check(_lib.drt_renderer_render_adaptive(self._h, C.byref(pod), scene._h, C.byref(p), C.byref(info)))
        self.m_LastAdaptiveMs = info.ms
        return info

    def GetAdaptiveState(self):
        """The per-pixel state of adaptive sampling (drt_renderer_read_adaptive): AdaptiveState(sum [H, W, 3] float32, count [H, W]
        uint32, m1 [H, W], m2 [H, W] float32, last_q [H, W], last_count [H, W] uint32 -- the last call's weights and counts)."""
        H, W = self.getBufferHeight(), self.getBufferWidth()
        a, b = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32)
        _check(_lib.drt_renderer_read_adaptive(self._h, 0, a.ctypes.data, a.nbytes))
        _check(_lib.drt_renderer_read_adaptive(self._h, 1, b.ctypes.data, b.nbytes))
        au, bu = a.view(np.uint32), b.view(np.uint32)
        return AdaptiveState(a[..., :3].copy(), au[..., 3].copy(), b[..., 0].copy(), b[..., 1].copy(), bu[..., 2].copy(), bu[..., 3].copy())

    def DeviceAdaptiveState(self, which=0):
        """Device address of the state's (sum, n) records (which 0) or (m1, m2, last q, last count) records (1), None before the
        first RenderAdaptive."""
        return _lib.drt_renderer_device_adaptive(self._h, int(which))

    def resetAdaptive(self):
        """Drop the adaptive state (drt_renderer_adaptive_reset): the next RenderAdaptive is uniform again."""
        _check(_lib.drt_renderer_adaptive_reset(self._h))

    def trackMotion(self, enable=True):
        """Follow geometry that Renderer.refit moves (drt_renderer_track_motion): the first refit after a TemporalDenoise keeps
        the triangles as they were, and the next TemporalDenoise reprojects every moved triangle's pixels through that state.
        False frees the snapshot."""
        _check(_lib.drt_renderer_track_motion(self._h, 1 if enable else 0))

    def advanceMotion(self):
        """The geometry as it is now is the previous geometry from here on (drt_renderer_motion_advance): what TemporalDenoise
        does by itself, for callers that use motionVectors with a filter of their own."""
        _check(_lib.drt_renderer_motion_advance(self._h))

    def motionVectors(self, cam, scene, prev_cam=None, as_torch=False):
        """Screen-space motion of every pixel's first hit (drt_renderer_motion_vectors): float32 [H, W, 4] = (fx - x, fy - y, z,
        flag), where (fx, fy) is the pixel position and z the depth in `prev_cam` (None = the camera of the last TemporalDenoise)
        of the point the pixel shows, carried back onto the geometry of the previous call; flag 0 = none (miss, or behind
        prev_cam), 1 = static, 2 = moved.  Row 0 = bottom.  as_torch=True: a device tensor, the work enqueued on the current
        torch stream; else a numpy array."""
        import torch                             # (only here: importing the package does not import torch)
        dev = torch.device("cuda", self._device)
        self._push_settings()
        out = torch.empty((self.getBufferHeight(), self.getBufferWidth(), 4), dtype=torch.float32, device=dev)
        pod = cam._pod()
        prev = prev_cam._pod() if prev_cam is not None else None
        stream = torch.cuda.current_stream(dev).cuda_stream
        _check(_lib.drt_renderer_motion_vectors(self._h, C.byref(pod), C.byref(prev) if prev is not None else None, scene._h,
                                                out.data_ptr() if out.numel() else None, stream))
        return out if as_torch else out.cpu().numpy()

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:              # (at interpreter shutdown the module's globals may be gone already)
            _lib.drt_renderer_destroy(h)

    def ResizeBuffer(self, width, height):
        _check(_lib.drt_renderer_resize(self._h, width, height))

    def _push_settings(self):
        _check(_lib.drt_renderer_set_settings(self._h, C.byref(self.m_RendererSettings)))

    def setMaterialModel(self, emissive=0, specular=0, emissive_scale=1.0, transmission=0):
        """Opt-in extension (drt_material_model): emissive term, metallic lobe, dielectric lobe.  Off (the default) = the reference's image."""
        m = MaterialModel(emissive, specular, emissive_scale, transmission)
        _check(_lib.drt_renderer_set_material_model(self._h, C.byref(m)))

    def Render(self, cam, scene):
        """One frame index; returns the kernel time in ms (the reference's `float* delta`)."""
        self._push_settings()
        ms = C.c_float(0)
        pod = cam._pod()
        _check(_lib.drt_renderer_render(self._h, C.byref(pod), scene._h, C.byref(ms)))
        return ms.value

    def RenderBatch(self, cam, scene, n_frames):
        self._push_settings()
        ms = C.c_float(0)
        pod = cam._pod()
        _check(_lib.drt_renderer_render_batch(self._h, C.byref(pod), scene._h, n_frames, C.byref(ms)))
        return ms.value

    def RenderBatchAsync(self, cam, scene, n_frames):
        """Enqueue only; Wait() blocks and returns the device time in ms."""
        self._push_settings()
        pod = cam._pod()
        _check(_lib.drt_renderer_render_batch_async(self._h, C.byref(pod), scene._h, n_frames))

    def Wait(self):
        ms = C.c_float(0)
        _check(_lib.drt_renderer_wait(self._h, C.byref(ms)))
        return ms.value

    def resetAccumulationBuffer(self):
        _check(_lib.drt_renderer_reset(self._h))

    def getBufferWidth(self):
        return _lib.drt_renderer_width(self._h)

    def getBufferHeight(self):
        return _lib.drt_renderer_height(self._h)

    def getSampleCount(self):
        return _lib.drt_renderer_sample_count(self._h)

    def getLocalRows(self):
        return _lib.drt_renderer_local_rows(self._h)

    def GetRenderTargetImage(self):
        """RGBA32F framebuffer as numpy [local_rows, width, 4]; row 0 = bottom (replaces the GL texture name)."""
        out = np.zeros((self.getLocalRows(), self.getBufferWidth(), 4), np.float32)
        _check(_lib.drt_renderer_read_rgba32f(self._h, out.ctypes.data, out.size))
        return out

    def GetAccumulationBuffer(self):
        out = np.zeros((self.getLocalRows(), self.getBufferWidth(), 3), np.float32)
        _check(_lib.drt_renderer_read_accum(self._h, out.ctypes.data, out.size))
        return out

    def setShard(self, stripe_rows, rank, world):
        _check(_lib.drt_renderer_set_shard(self._h, stripe_rows, rank, world))

    def bindBuffers(self, accum_ptr, rgba_ptr):
        _check(_lib.drt_renderer_bind_buffers(self._h, accum_ptr, rgba_ptr))

    def setStream(self, stream_ptr):
        _check(_lib.drt_renderer_set_stream(self._h, stream_ptr))

    def setCounting(self, enable):
        _check(_lib.drt_renderer_set_counting(self._h, 1 if enable else 0))

    def getCounters(self):
        c = Counters()
        _check(_lib.drt_renderer_get_counters(self._h, C.byref(c)))
        return c

    def setFramesInFlight(self, n):
        """Hint that n launches are kept in flight on this device (other renderers on other streams): small launches get
        smaller grids so that they overlap -- a share of 1/n while n is below the runtime's hardware queue count, else of one over half
        that count (drt.h).  Does not change results."""
        _check(_lib.drt_renderer_set_frames_in_flight(self._h, int(n)))

    def waveQueuePlans(self):
        """The launch packagings of wave_queue timed so far (list of plans; see drt_debug_wave_queue_plans)."""
        import json
        buf = C.create_string_buffer(1 << 16)
        _check(_lib.drt_debug_wave_queue_plans(self._h, buf, len(buf)))
        return json.loads(buf.value.decode())

    def poolStats(self, reset=True):
        """path_pool statistics (renderer created with DRT_POOL_STATS=1): dict queue -> (batches, mean paths per batch, ticks)."""
        a = np.zeros(40, np.uint64)
        _check(_lib.drt_debug_pool_stats(self._h, a.ctypes.data, 1 if reset else 0))
        out = {}
        for k, name in enumerate(("N", "T0", "T1", "T2", "T3", "B", "E", "R", "S")):
            b, l, t = int(a[3 * k]), int(a[3 * k + 1]), int(a[3 * k + 2])
            out[name] = (b, l / max(b, 1), t)
        out["claim_ticks"], out["idle_polls"], out["lost_claims"], out["wave_ticks"] = int(a[27]), int(a[28]), int(a[29]), int(a[30])
        out["failed_claims"], out["failed_claim_ticks"], out["idle_ticks"] = int(a[31]), int(a[32]), int(a[33])
        out["work"] = dict(n_iterations=int(a[34]), n_lane_pops=int(a[35]), t_steps=int(a[36]), t_lane_tests=int(a[37]), dir_iterations=int(a[38]), dir_lane_tries=int(a[39]))
        return out

    def launchesOfLastBatch(self):
        """Tracing-kernel launches the last RenderBatch was split into (per-launch sample buffer budget)."""
        return int(_lib.drt_renderer_launch_count(self._h))

    def kernelSpanMs(self):
        """Device-measured execution time of the tracing kernel(s) of the last completed batch (no queueing time)."""
        ms = C.c_float(0)
        _check(_lib.drt_renderer_kernel_span(self._h, C.byref(ms)))
        return float(ms.value)

    def kernelInfo(self):
        buf = C.create_string_buffer(128)
        _check(_lib.drt_renderer_kernel_info(self._h, buf, 128))
        return buf.value.decode()


_KAT_WORDS = {0: (1, 5), 1: (1, 5), 2: (12, 1), 3: (15, 5), 4: (3, 7), 5: (1, 3), 6: (10, 7), 7: (3, 6), 8: (1, 2)}


def debug_kat(which, inputs, cam=None, width=0, height=0, device=0):
    """Runs device leaf function `which` (see drt.h drt_debug_kat) on uint32-viewed inputs [n, words]; returns uint32 [n, words]."""
    win, wout = _KAT_WORDS[which]
    a = np.ascontiguousarray(inputs).view(np.uint32).reshape(-1, win)
    out = np.zeros((len(a), wout), np.uint32)
    pod = cam._pod() if cam is not None else None
    _check(_lib.drt_debug_kat(device, which, a.ctypes.data, a.nbytes, out.ctypes.data, out.nbytes, len(a),
                              C.byref(pod) if pod is not None else None, width, height))
    return out


def debug_upscale(colour, guides_lo, guides_hi, device=0, **params):
    """The upscale kernel alone on host arrays (drt.h drt_debug_upscale): colour float32 [H, W, 4], guides_lo [H, W, 8] and
    guides_hi [Ho, Wo, 8] as drt_guide lays them out (albedo rgb, t, normal xyz, prim as int32 bits); `params` = UpscaleParams
    fields.  Returns float32 [Ho, Wo, 4]."""
    c = np.ascontiguousarray(colour, np.float32)
    lo, hi = np.ascontiguousarray(guides_lo, np.float32), np.ascontiguousarray(guides_hi, np.float32)
    H, W = c.shape[:2]
    Ho, Wo = hi.shape[:2]
    if c.shape != (H, W, 4) or lo.shape != (H, W, 8) or hi.shape != (Ho, Wo, 8):
        raise ValueError("colour [H, W, 4], guides_lo [H, W, 8], guides_hi [Ho, Wo, 8]")
    p = UpscaleParams(**params)
    out = np.zeros((Ho, Wo, 4), np.float32)
    _check(_lib.drt_debug_upscale(device, c.ctypes.data, lo.ctypes.data, hi.ctypes.data, W, H, Wo, Ho, C.byref(p), out.ctypes.data))
    return out


def debug_adaptive_plan(q, thresholded=False, device=0, **params):
    """Counts and their exclusive prefix sum on the device from made-up weights (drt.h drt_debug_adaptive_plan): q uint32 [n];
    `params` = AdaptiveParams fields.  Returns (counts uint32 [n], offsets uint32 [n], Q)."""
    q = np.ascontiguousarray(q, np.uint32).reshape(-1)
    p = AdaptiveParams(**params)
    counts, offsets = np.zeros(len(q), np.uint32), np.zeros(len(q), np.uint32)
    Q = C.c_uint64(0)
    _check(_lib.drt_debug_adaptive_plan(device, q.ctypes.data, len(q), C.byref(p), 1 if thresholded else 0, counts.ctypes.data,
                                        offsets.ctypes.data, C.byref(Q)))
    return counts, offsets, int(Q.value)


def debug_adaptive_weights(state, device=0, **params):
    """The weights stage on made-up state records, inside the whole plan as a call runs it (drt.h drt_debug_adaptive_weights):
    `state` has n (or count) uint32 [P], m1 and m2 float32 [P], as tests/adaptive_ref.py's State or AdaptiveState; `params` =
    AdaptiveParams fields.  Returns (q uint32 [P], Q, active)."""
    n = np.ascontiguousarray(state.n if hasattr(state, "n") else state.count, np.uint32).reshape(-1)
    s0, s1 = np.zeros((len(n), 4), np.float32), np.zeros((len(n), 4), np.float32)
    s0.view(np.uint32)[:, 3] = n
    s1[:, 0] = np.asarray(state.m1, np.float32).reshape(-1)
    s1[:, 1] = np.asarray(state.m2, np.float32).reshape(-1)
    p = AdaptiveParams(**params)
    q = np.zeros(len(n), np.uint32)
    Q, active = C.c_uint64(0), C.c_uint32(0)
    _check(_lib.drt_debug_adaptive_weights(device, s0.ctypes.data, s1.ctypes.data, len(n), C.byref(p), q.ctypes.data, C.byref(Q),
                                           C.byref(active)))
    return q, int(Q.value), int(active.value)


def debug_decode_image(file_bytes):
    """The loader's image decoder (PNG / baseline JPEG) on a file held in memory -> uint8 [H, W, C]."""
    buf = (C.c_uint8 * len(file_bytes)).from_buffer_copy(bytes(file_bytes))
    info = _TexInfo()
    _check(_lib.drt_debug_decode_image(buf, len(file_bytes), C.byref(info), None, 0))
    out = np.zeros((info.height, info.width, info.components), np.uint8)
    _check(_lib.drt_debug_decode_image(buf, len(file_bytes), C.byref(info), out.ctypes.data, out.size))
    return out


def debug_hash_cycles(max_len=64, cap=4096, device=0):
    """[(value, cycle length)] for every 32-bit value on a pcg_hash cycle of length <= max_len."""
    pairs = np.zeros((cap, 2), np.uint32)
    found = C.c_uint32(0)
    _check(_lib.drt_debug_hash_cycles(device, max_len, pairs.ctypes.data, cap, C.byref(found)))
    return [(int(v), int(n)) for v, n in pairs[: min(found.value, cap)]]


def debug_check_rcp(device=0):
    """(mismatches, fast-path count) of the kernels' exact_rcp vs IEEE 1.0f/x over all 2^32 floats."""
    bad, fast = C.c_uint64(0), C.c_uint64(0)
    _check(_lib.drt_debug_check_rcp(device, C.byref(bad), C.byref(fast)))
    return int(bad.value), int(fast.value)


def debug_check_sqrt(device=0):
    """(mismatches, fast-path count) of the kernels' exact_sqrt vs sqrtf over all 2^32 floats."""
    bad, fast = C.c_uint64(0), C.c_uint64(0)
    _check(_lib.drt_debug_check_sqrt(device, C.byref(bad), C.byref(fast)))
    return int(bad.value), int(fast.value)


def assemble_shards(gathered_ptr, image_ptr, width, height, stripe_rows, world, padded_rows, stream_ptr=None):
    _check(_lib.drt_assemble_shards(gathered_ptr, image_ptr, width, height, stripe_rows, world, padded_rows, stream_ptr))
