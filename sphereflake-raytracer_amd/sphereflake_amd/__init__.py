"""Python host mirror of the reference ``SphereflakeRaytracer::Sphereflake`` class
(/root/reference/sphereflake/Sphereflake.h:13-58) over the gfx950 C ABI
(include/sphereflake/sf.h, built as build/libsphereflake_hip.so).

There is no CPU fallback: if the HIP library is missing or the device is not a gfx950,
constructing a :class:`Sphereflake` raises. The CPU restatement under ``oracle/`` is test
infrastructure and is never imported from here.

Names follow the reference: ``SetView``, ``GetGBuffer``, ``GetMaxDepthReached``,
``ResetMaxDepthReached``, ``GetRaysPerSecond``, ``ResetRaysPerSecond``,
``GetClosestSphereDistance``, ``ResetClosestSphereDistance``, ``Initialize`` (frame-less
progressive mode), plus ``Render`` (one deterministic full frame). ``Camera`` mirrors
reference camera.h.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
import threading
from dataclasses import dataclass

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT_DIR = os.path.dirname(PKG_DIR)                 # sphereflake-raytracer_amd/
# SF_LIB selects another build of the same library (e.g. the stamp diagnostics build_phases/)
LIB_PATH = os.environ.get("SF_LIB") or os.path.join(ROOT_DIR, "build", "libsphereflake_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(ROOT_DIR), "include", "sphereflake", "sf.h")

SF_OK, SF_EINVAL, SF_ENOMEM, SF_EHIP, SF_ENODEV, SF_ENOVIEW, SF_EDEPTH, SF_ESTATE = 0, -1, -2, -3, -4, -5, -6, -7
SF_KERNEL_WAVE, SF_KERNEL_PER_RAY = 0, 1
SF_MAX_DEPTH_LIMIT = 31
FLT_MAX = float(np.finfo(np.float32).max)

# Camera of reference main.cpp:92-96; BASELINE configs scale the position by K.
DEFAULT_CAMERA_POSITION = (-5.4098, -7.2139, 1.19006)
DEFAULT_PITCH = -1.371
DEFAULT_YAW = 0.921999
SF_DIAG_WAVES = 65536            # per-wave diagnostic records (sf_internal.h)


class SphereflakeError(RuntimeError):
    def __init__(self, code: int, what: str = ""):
        self.code = code
        msg = _strerror(code)
        super().__init__(f"{what}: {msg} ({code})" if what else f"{msg} ({code})")


class sf_render_params(ctypes.Structure):
    _fields_ = [("band_rows", ctypes.c_uint32), ("band_count", ctypes.c_uint32),
                ("band_index", ctypes.c_uint32), ("compact", ctypes.c_uint32),
                ("kernel", ctypes.c_uint32), ("emit_aux", ctypes.c_uint32),
                ("max_depth", ctypes.c_uint32), ("packed", ctypes.c_uint32),
                ("stream", ctypes.c_void_p)]


class sf_dirs_params(ctypes.Structure):
    _fields_ = [("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("stride", ctypes.c_uint32),
                ("max_depth", ctypes.c_uint32), ("stream", ctypes.c_void_p)]


class sf_rays_params(ctypes.Structure):
    _fields_ = [("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("dir_stride", ctypes.c_uint32),
                ("origin_stride", ctypes.c_uint32), ("rays_per_origin", ctypes.c_uint32),
                ("max_depth", ctypes.c_uint32), ("stream", ctypes.c_void_p)]


class sf_shadow_params(ctypes.Structure):
    _fields_ = [("light", ctypes.c_float * 3), ("bias", ctypes.c_float), ("origin", ctypes.c_float * 3),
                ("use_origin", ctypes.c_uint32), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32),
                ("max_depth", ctypes.c_uint32), ("stream", ctypes.c_void_p)]


SF_SHADOW_LIGHTS_MAX = 64


class sf_shadows_params(ctypes.Structure):
    _fields_ = [("lights", ctypes.POINTER(ctypes.c_float)), ("weights", ctypes.POINTER(ctypes.c_float)),
                ("n", ctypes.c_uint32), ("bias", ctypes.c_float), ("origin", ctypes.c_float * 3),
                ("use_origin", ctypes.c_uint32), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32),
                ("max_depth", ctypes.c_uint32), ("stream", ctypes.c_void_p)]


class sf_sun_params(ctypes.Structure):
    _fields_ = [("dir", ctypes.c_float * 3), ("distance", ctypes.c_float), ("bias", ctypes.c_float),
                ("origin", ctypes.c_float * 3), ("use_origin", ctypes.c_uint32), ("width", ctypes.c_uint32),
                ("height", ctypes.c_uint32), ("max_depth", ctypes.c_uint32), ("stream", ctypes.c_void_p)]


SF_SUN_DIRS_MAX = 64


class sf_suns_params(ctypes.Structure):
    _fields_ = [("dirs", ctypes.POINTER(ctypes.c_float)), ("weights", ctypes.POINTER(ctypes.c_float)),
                ("n", ctypes.c_uint32), ("distance", ctypes.c_float), ("bias", ctypes.c_float),
                ("origin", ctypes.c_float * 3), ("use_origin", ctypes.c_uint32), ("width", ctypes.c_uint32),
                ("height", ctypes.c_uint32), ("max_depth", ctypes.c_uint32), ("stream", ctypes.c_void_p)]


SF_SHAFT_SAMPLES_MAX = 64


class sf_shafts_params(ctypes.Structure):
    _fields_ = [("dir", ctypes.c_float * 3), ("distance", ctypes.c_float), ("bias", ctypes.c_float),
                ("fractions", ctypes.POINTER(ctypes.c_float)), ("weights", ctypes.POINTER(ctypes.c_float)),
                ("n", ctypes.c_uint32), ("dirs", ctypes.POINTER(ctypes.c_float)), ("dirs_stride", ctypes.c_uint32),
                ("far", ctypes.c_float), ("origin", ctypes.c_float * 3), ("use_origin", ctypes.c_uint32),
                ("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("max_depth", ctypes.c_uint32),
                ("stream", ctypes.c_void_p)]


SF_LIGHT_SUM_MAX = 65536


class sf_light_sum_params(ctypes.Structure):
    _fields_ = [("points", ctypes.POINTER(ctypes.c_float)), ("colours", ctypes.POINTER(ctypes.c_float)),
                ("n", ctypes.c_uint32), ("accumulate", ctypes.c_uint32), ("distance", ctypes.c_float),
                ("bias", ctypes.c_float), ("origin", ctypes.c_float * 3), ("use_origin", ctypes.c_uint32),
                ("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("max_depth", ctypes.c_uint32),
                ("stream", ctypes.c_void_p)]


SF_AO_SAMPLES_MAX = 64


class sf_ao_params(ctypes.Structure):
    _fields_ = [("samples", ctypes.POINTER(ctypes.c_float)), ("colours", ctypes.POINTER(ctypes.c_float)),
                ("n", ctypes.c_uint32), ("accumulate", ctypes.c_uint32), ("distance", ctypes.c_float),
                ("bias", ctypes.c_float), ("origin", ctypes.c_float * 3), ("use_origin", ctypes.c_uint32),
                ("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("max_depth", ctypes.c_uint32),
                ("stream", ctypes.c_void_p)]


SF_AO_SPIN_MAX = 8


class sf_ao_spin(ctypes.Structure):
    _fields_ = [("cs", ctypes.POINTER(ctypes.c_float)), ("size", ctypes.c_uint32)]


class sf_mirror_params(ctypes.Structure):
    _fields_ = sf_ao_params._fields_ + [("eye", ctypes.c_float * 3), ("use_eye", ctypes.c_uint32),
                                        ("zenith", ctypes.c_float * 3), ("horizon", ctypes.c_float * 3),
                                        ("up", ctypes.c_float * 3)]


class sf_light_filter_params(ctypes.Structure):
    _fields_ = [("size", ctypes.c_uint32), ("normal_min", ctypes.c_float), ("plane_max", ctypes.c_float),
                ("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("stream", ctypes.c_void_p)]


class sf_light_accumulate_params(ctypes.Structure):
    _fields_ = [("max_history", ctypes.c_uint32), ("normal_min", ctypes.c_float), ("plane_max", ctypes.c_float),
                ("origin", ctypes.c_float * 3), ("use_origin", ctypes.c_uint32), ("hist_origin", ctypes.c_float * 3),
                ("hist_m", ctypes.c_float * 9), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32),
                ("stream", ctypes.c_void_p)]


class sf_stats(ctypes.Structure):
    _fields_ = [("max_depth", ctypes.c_int32), ("closest", ctypes.c_float),
                ("rays", ctypes.c_int64), ("overflow_tiles", ctypes.c_int64)]


class sf_post_params(ctypes.Structure):
    _fields_ = [("sample_radius", ctypes.c_float), ("intensity", ctypes.c_float), ("scale", ctypes.c_float),
                ("bias", ctypes.c_float), ("normal_threshold", ctypes.c_float), ("depth_threshold", ctypes.c_float),
                ("camera_position", ctypes.c_float * 3), ("downscale", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("stream", ctypes.c_void_p)]


SF_VARIANT_AVX = 0
SF_VARIANT_SSE = 1
SF_POST_GENERAL = 1
SF_POST_UNIT_NORMALS = 2
SF_DUMP_IMAGE, SF_DUMP_NORMALS, SF_DUMP_POSITIONS_PFM, SF_DUMP_NORMALS_PFM = 0, 1, 2, 3

# exported symbol -> (restype, argtypes); checked against include/sphereflake/sf.h by the tests
_F = ctypes.POINTER(ctypes.c_float)
_U = ctypes.POINTER(ctypes.c_uint32)
_CTX = ctypes.c_void_p
SIGNATURES = {
    "sf_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p)]),
    "sf_destroy": (None, [_CTX]),
    "sf_set_view": (ctypes.c_int, [_CTX, _F, _F, _F, _F]),
    "sf_set_setup": (ctypes.c_int, [_CTX, _F, _F]),
    "sf_get_setup": (ctypes.c_int, [_CTX, _F, _F]),
    "sf_render": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_render_params)]),
    "sf_render_to": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_render_params), ctypes.c_void_p, ctypes.c_void_p,
                                    ctypes.c_void_p, ctypes.c_void_p]),
    "sf_trace_dirs_to": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_dirs_params), ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "sf_trace_dirs": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_dirs_params), ctypes.c_void_p]),
    "sf_probe_dirs": (ctypes.c_int, [_CTX, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_void_p, ctypes.c_void_p]),
    "sf_trace_rays_to": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_rays_params), ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "sf_probe_rays": (ctypes.c_int, [_CTX, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32,
                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "sf_shadow_defaults": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_shadow_params)]),
    "sf_trace_shadow_to": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_shadow_params), ctypes.c_void_p, ctypes.c_void_p]),
    "sf_trace_shadow": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_shadow_params)]),
    "sf_download_shadow": (ctypes.c_int, [_CTX, ctypes.c_void_p]),
    "sf_shadow_buffer": (ctypes.c_int, [_CTX, ctypes.POINTER(ctypes.c_void_p)]),
    "sf_light_image": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_shadow_params), ctypes.c_float, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "sf_shadows_defaults": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_shadows_params)]),
    "sf_trace_shadows_to": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_shadows_params), ctypes.c_void_p, ctypes.c_void_p]),
    "sf_trace_shadows": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_shadows_params)]),
    "sf_download_shadow_masks": (ctypes.c_int, [_CTX, ctypes.c_void_p]),
    "sf_shadow_mask_buffer": (ctypes.c_int, [_CTX, ctypes.POINTER(ctypes.c_void_p)]),
    "sf_light_image_many": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_shadows_params), ctypes.c_float, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "sf_set_shadow_lod": (ctypes.c_int, [_CTX, ctypes.c_float]),
    "sf_get_shadow_lod": (ctypes.c_float, [_CTX]),
    "sf_sun_defaults": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_sun_params)]),
    "sf_trace_sun_to": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_sun_params), ctypes.c_void_p, ctypes.c_void_p]),
    "sf_trace_sun": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_sun_params)]),
    "sf_light_image_sun": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_sun_params), ctypes.c_float, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "sf_suns_defaults": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_suns_params)]),
    "sf_trace_suns_to": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_suns_params), ctypes.c_void_p, ctypes.c_void_p]),
    "sf_trace_suns": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_suns_params)]),
    "sf_light_image_suns": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_suns_params), ctypes.c_float, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "sf_shafts_defaults": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_shafts_params)]),
    "sf_trace_shafts_to": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_shafts_params), ctypes.c_void_p, ctypes.c_void_p]),
    "sf_trace_shafts": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_shafts_params)]),
    "sf_light_image_shafts": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_shafts_params), ctypes.c_float,
                                             ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p]),
    "sf_light_sum_defaults": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_light_sum_params)]),
    "sf_trace_suns_sum_to": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_light_sum_params), ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_void_p]),
    "sf_trace_suns_sum": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_light_sum_params)]),
    "sf_trace_shadows_sum_to": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_light_sum_params), ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.c_void_p]),
    "sf_trace_shadows_sum": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_light_sum_params)]),
    "sf_ao_defaults": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_ao_params)]),
    "sf_trace_ao_to": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_ao_params), ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_void_p]),
    "sf_trace_ao": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_ao_params)]),
    "sf_trace_ao_sum_to": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_ao_params), ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p]),
    "sf_trace_ao_sum": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_ao_params)]),
    "sf_trace_ao_spin_to": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_ao_params), ctypes.POINTER(sf_ao_spin),
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "sf_trace_ao_spin": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_ao_params), ctypes.POINTER(sf_ao_spin)]),
    "sf_trace_ao_spin_sum_to": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_ao_params), ctypes.POINTER(sf_ao_spin),
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "sf_trace_ao_spin_sum": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_ao_params), ctypes.POINTER(sf_ao_spin)]),
    "sf_mirror_defaults": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_mirror_params)]),
    "sf_trace_mirror_to": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_mirror_params), ctypes.POINTER(sf_ao_spin),
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "sf_trace_mirror": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_mirror_params), ctypes.POINTER(sf_ao_spin)]),
    "sf_trace_mirror_sum_to": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_mirror_params), ctypes.POINTER(sf_ao_spin),
                                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "sf_trace_mirror_sum": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_mirror_params), ctypes.POINTER(sf_ao_spin)]),
    "sf_light_filter_defaults": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_light_filter_params)]),
    "sf_light_filter_to": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_light_filter_params), ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "sf_light_filter": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_light_filter_params)]),
    "sf_reproject_matrix": (ctypes.c_int, [_F, _F]),
    "sf_light_accumulate_defaults": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_light_accumulate_params)]),
    "sf_light_accumulate_to": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_light_accumulate_params)] + [ctypes.c_void_p] * 7),
    "sf_light_accumulate": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_light_accumulate_params)]),
    "sf_light_history_reset": (ctypes.c_int, [_CTX]),
    "sf_light_fill": (ctypes.c_int, [_CTX, ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]),
    "sf_light_buffer": (ctypes.c_int, [_CTX, ctypes.POINTER(ctypes.c_void_p)]),
    "sf_download_light": (ctypes.c_int, [_CTX, ctypes.c_void_p]),
    "sf_light_image_buffer": (ctypes.c_int, [_CTX, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p]),
    "sf_render_frames": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32,
                                        ctypes.POINTER(sf_render_params)]),
    "sf_slab_rows": (ctypes.c_uint32, [ctypes.c_uint32] * 4),
    "sf_unpack_bands": (ctypes.c_int, [_CTX, ctypes.c_void_p] + [ctypes.c_uint32] * 5 + [ctypes.c_void_p]),
    "sf_unpack_slabs": (ctypes.c_int, [_CTX, ctypes.c_void_p] + [ctypes.c_uint32] * 6 + [ctypes.c_void_p]),
    "sf_slab_bytes": (ctypes.c_uint32, [_CTX]),
    "sf_download": (ctypes.c_int, [_CTX, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "sf_download_async": (ctypes.c_int, [_CTX, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p]),
    "sf_set_variant": (ctypes.c_int, [_CTX, ctypes.c_int]),
    "sf_get_variant": (ctypes.c_int, [_CTX]),
    "sf_lod_threshold": (ctypes.c_int, [ctypes.c_float, ctypes.c_float, _F]),
    "sf_division_by_reciprocal_exact": (ctypes.c_int, [ctypes.c_uint32]),
    "sf_post_defaults": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_post_params)]),
    "sf_post_process": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_post_params), ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_void_p]),
    "sf_download_image": (ctypes.c_int, [_CTX, ctypes.c_void_p]),
    "sf_ssao_noise": (ctypes.c_int, [_F]),
    "sf_save_image": (ctypes.c_int, [_CTX, ctypes.c_char_p, ctypes.c_int]),
    "sf_write_ppm": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]),
    "sf_write_pfm": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]),
    "sf_get_size": (ctypes.c_int, [_CTX, _U, _U]),
    "sf_host_register": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t]),
    "sf_host_unregister": (ctypes.c_int, [ctypes.c_void_p]),
    "sf_device_buffers": (ctypes.c_int, [_CTX] + [ctypes.POINTER(ctypes.c_void_p)] * 4),
    "sf_synchronize": (ctypes.c_int, [_CTX]),
    "sf_get_stats": (ctypes.c_int, [_CTX, ctypes.POINTER(sf_stats)]),
    "sf_reset_max_depth": (ctypes.c_int, [_CTX]),
    "sf_reset_rays": (ctypes.c_int, [_CTX]),
    "sf_reset_closest": (ctypes.c_int, [_CTX]),
    "sf_progressive": (ctypes.c_int, [_CTX, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p]),
    "sf_camera_corners": (ctypes.c_int, [ctypes.c_uint32, ctypes.c_uint32, _F, ctypes.c_float, ctypes.c_float,
                                         ctypes.c_float, ctypes.c_float, _F, _F, _F, _F]),
    "sf_child_transforms": (ctypes.c_int, [_F]),
    "sf_root_transform": (ctypes.c_int, [_F, _F]),
    "sf_depth_constants": (ctypes.c_int, [ctypes.c_uint32, _F, _F]),
    "sf_rsqrtps": (ctypes.c_float, [ctypes.c_float]),
    "sf_mt19937_jump": (ctypes.c_int, [_U, ctypes.c_uint64, _U]),
    "sf_set_tile_trace": (ctypes.c_int, [_CTX, ctypes.c_int]),
    "sf_get_tile_trace": (ctypes.c_int, [_CTX, ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t]),
    "sf_get_tile_order": (ctypes.c_int, [_CTX, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32),
                                         ctypes.c_size_t]),
    "sf_set_kernel_timing": (ctypes.c_int, [_CTX, ctypes.c_int]),
    "sf_kernel_times": (ctypes.c_int, [_CTX, _F, ctypes.c_uint32]),
    "sf_kernel_clocks": (ctypes.c_int, [_CTX, _F, ctypes.c_uint32]),
    "sf_strerror": (ctypes.c_char_p, [ctypes.c_int]),
    "sf_last_hip_error": (ctypes.c_int, [_CTX]),
    "sf_abi_version": (ctypes.c_int, []),
    "sf_build_id": (ctypes.c_char_p, []),
    "sf_device_count": (ctypes.c_int, []),
    "sf_context_stream": (ctypes.c_void_p, [_CTX]),
    "sf_lean_launches": (ctypes.c_uint32, [_CTX]),
    "sf_pair_launches": (ctypes.c_uint32, [_CTX]),
    "sf_order_units": (ctypes.c_uint32, [_CTX]),
    "sf_group_create": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32,
                                       ctypes.POINTER(ctypes.c_void_p)]),
    "sf_group_destroy": (None, [ctypes.c_void_p]),
    "sf_group_size": (ctypes.c_int, [ctypes.c_void_p]),
    "sf_group_member": (ctypes.c_void_p, [ctypes.c_void_p, ctypes.c_int]),
    "sf_group_set_view": (ctypes.c_int, [ctypes.c_void_p, _F, _F, _F, _F]),
    "sf_group_set_variant": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "sf_group_render": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32]),
    "sf_group_synchronize": (ctypes.c_int, [ctypes.c_void_p]),
    "sf_group_download": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "sf_group_get_stats": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(sf_stats)]),
    "sf_group_last_hip_error": (ctypes.c_int, [ctypes.c_void_p]),
    "sf_group_reset_stats": (ctypes.c_int, [ctypes.c_void_p]),
    "sf_group_slab_bytes": (ctypes.c_int, [ctypes.c_void_p]),
    "sf_dist_unique_id": (ctypes.c_int, [ctypes.c_void_p]),
    "sf_dist_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int,
                                      ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]),
    "sf_dist_destroy": (None, [ctypes.c_void_p]),
    "sf_dist_slots": (ctypes.c_int, [ctypes.c_void_p]),
    "sf_dist_context": (ctypes.c_void_p, [ctypes.c_void_p, ctypes.c_int]),
    "sf_dist_last_slot": (ctypes.c_int, [ctypes.c_void_p]),
    "sf_dist_set_view": (ctypes.c_int, [ctypes.c_void_p, _F, _F, _F, _F]),
    "sf_dist_render": (ctypes.c_int, [ctypes.c_void_p]),
    "sf_dist_render_bands": (ctypes.c_int, [ctypes.c_void_p]),
    "sf_dist_render_bands_frames": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, _F]),
    "sf_dist_synchronize": (ctypes.c_int, [ctypes.c_void_p]),
    "sf_dist_download": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "sf_dist_get_stats": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(sf_stats)]),
    "sf_dist_reset_stats": (ctypes.c_int, [ctypes.c_void_p]),
    "sf_dist_last_error": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "sf_dist_comm_info": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int] + [ctypes.POINTER(ctypes.c_int)] * 3),
    "sf_dist_slab_bytes": (ctypes.c_int, [ctypes.c_void_p]),
}
SF_ECOMM = -8
SF_DIST_ID_BYTES = 128

# the sf_*_defaults of the light traces' parameter blocks (Sphereflake._defaults)
_DEFAULTS = {sf_shadow_params: "sf_shadow_defaults", sf_shadows_params: "sf_shadows_defaults",
             sf_sun_params: "sf_sun_defaults", sf_suns_params: "sf_suns_defaults",
             sf_shafts_params: "sf_shafts_defaults", sf_light_sum_params: "sf_light_sum_defaults",
             sf_ao_params: "sf_ao_defaults", sf_mirror_params: "sf_mirror_defaults"}

_lib = None
_lock = threading.Lock()


def build(force: bool = False) -> str:
    """Compile the gfx950 library in-tree (hipcc cross-compiles without a GPU)."""
    if force or not os.path.exists(LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", ROOT_DIR, "all"])
    return LIB_PATH


def lib() -> ctypes.CDLL:
    """Load build/libsphereflake_hip.so; raises if it is missing (no fallback path exists)."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise ImportError(f"HIP renderer library not built: {LIB_PATH} (run make -C {ROOT_DIR})")
            # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64 (SONAME
            # libamdhip64.so.7). Loading it first makes our NEEDED libamdhip64.so.7 resolve to the
            # same runtime, so torch tensors / streams and our contexts can be mixed freely.
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
            L = ctypes.CDLL(LIB_PATH)
            # (SF_LIB_PARTIAL=1: an older build under A/B -- entry points it predates are left unbound)
            partial = os.environ.get("SF_LIB_PARTIAL") == "1"
            for name, (res, args) in SIGNATURES.items():
                if partial and not hasattr(L, name):
                    continue
                fn = getattr(L, name)
                fn.restype = res
                fn.argtypes = args
            _lib = L
    return _lib


def build_info() -> dict:
    """Which build is loaded: the source hash the library embeds (sf_build_id), the hash of the sources in
    this tree (scripts/source_hash.py), whether they agree, and the SHA-256 of the library file itself."""
    import hashlib
    import importlib.util
    with open(LIB_PATH, "rb") as f:
        lib_sha = hashlib.sha256(f.read()).hexdigest()[:16]
    embedded = lib().sf_build_id().decode()
    tree = None
    sh = os.path.join(os.path.dirname(ROOT_DIR), "scripts", "source_hash.py")
    if os.path.exists(sh):
        spec = importlib.util.spec_from_file_location("_sf_source_hash", sh)
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        tree = m.source_hash()
    return {"source_sha256": embedded, "tree_source_sha256": tree, "lib_matches_tree": embedded == tree,
            "lib_sha256": lib_sha}


def _strerror(code: int) -> str:
    try:
        return lib().sf_strerror(code).decode()
    except Exception:  # library not loadable: still give a message
        return f"sphereflake error {code}"


def _check(rc: int, what: str = "", ctx=None) -> None:
    if rc != SF_OK:
        err = SphereflakeError(rc, what)
        if ctx is not None and rc == SF_EHIP:
            err.hip_error = lib().sf_last_hip_error(ctx)
        raise err


def _f32(a, n=None) -> np.ndarray:
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float32))
    if n is not None and a.size != n:
        raise ValueError(f"expected {n} floats, got {a.size}")
    return a


def _fp(a: np.ndarray):
    return a.ctypes.data_as(_F)


_F3 = ctypes.c_float * 3


# What the parameter builders of the light traces share (Sphereflake.shadow_params ... mirror_params).
def _entries(a, per, limit, what) -> np.ndarray:
    """The list of a parameter block: [n, per] float32 ([n] where per is 1), n in 1..limit."""
    a = np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1 if per == 1 else (-1, per)))
    if not 1 <= a.shape[0] <= limit:
        raise ValueError(f"1..{limit} {what} per call, not {a.shape[0]}")
    return a


def _entry_values(values, n, per, message):
    """The weights [n] or colours [n, 3] beside a list of n entries, or None."""
    if values is None:
        return None
    v = np.ascontiguousarray(np.asarray(values, np.float32).reshape(-1 if per == 1 else (-1, per)))
    if v.shape[0] != n:
        raise ValueError(message)
    return v


def _params_tail(p, distance, bias, origin, width, height, max_depth, stream):
    """The fields every block ends with; distance and bias None keep what sf_*_defaults set, origin None the view's."""
    if distance is not None:
        p.distance = float(distance)
    if bias is not None:
        p.bias = float(bias)
    if origin is not None:
        p.origin[:] = [float(x) for x in _f32(origin, 3)]
        p.use_origin = 1
    p.width, p.height, p.max_depth, p.stream = int(width), int(height), int(max_depth), stream
    return p


def _vec3(v):
    """A view vector as a ctypes float[3] (the per-frame SetView path: a tuple or list of 3 numbers is converted
    without numpy, ~6 us less host time per frame; float32 rounding as np.float32)."""
    if isinstance(v, (tuple, list)) and len(v) == 3:
        return _F3(*v)
    if isinstance(v, np.ndarray) and v.dtype == np.float32 and v.shape == (3,):
        return _F3(*v.tolist())
    return _F3(*_f32(v, 3).ravel().tolist())


# ----------------------------------------------------------------------------- host setup helpers

def child_transforms() -> np.ndarray:
    """9 unit child frames (reference Sphereflake.cpp:216-249), [9, 16] glm column-major."""
    out = np.zeros((9, 16), np.float32)
    _check(lib().sf_child_transforms(_fp(out)), "sf_child_transforms")
    return out


def root_transform(origin) -> np.ndarray:
    """Root transform of SetView (Sphereflake.cpp:83) for a ray origin, [16]."""
    o = _f32(origin, 3)
    out = np.zeros(16, np.float32)
    _check(lib().sf_root_transform(_fp(o), _fp(out)), "sf_root_transform")
    return out


def reproject_matrix(view) -> np.ndarray:
    """sf_reproject_matrix: the inverse [9] (row-major 3 x 3) of the ray generation of the view (origin, top-left,
    top-right, bottom-left), 12 floats. sphereflake_amd.lights.reproject_matrix states the same arithmetic in numpy."""
    v = _f32(np.concatenate([np.asarray(x, np.float32).reshape(-1) for x in view])
             if isinstance(view, (tuple, list)) else view, 12)
    out = np.zeros(9, np.float32)
    _check(lib().sf_reproject_matrix(_fp(v), _fp(out)), "sf_reproject_matrix")
    return out


def depth_constants(depth: int):
    """(radius r_d, exact LOD threshold T_d) used by the kernels at a depth."""
    r, t = ctypes.c_float(), ctypes.c_float()
    _check(lib().sf_depth_constants(depth, ctypes.byref(r), ctypes.byref(t)), "sf_depth_constants")
    return r.value, t.value


def lod_threshold(r: float, lod_constant: float = 70.0) -> float:
    """Exact T with sqrtf(t / r) < lod_constant || t < 0  <=>  t < T (Sphereflake.h:129,146)."""
    t = ctypes.c_float()
    _check(lib().sf_lod_threshold(ctypes.c_float(r), ctypes.c_float(lod_constant), ctypes.byref(t)),
           "sf_lod_threshold")
    return t.value


def rsqrtps(x: float) -> float:
    """x86 rsqrtps as reproduced by the renderer (host copy of the kernels' table)."""
    return lib().sf_rsqrtps(float(x))


def device_count() -> int:
    return lib().sf_device_count()


class Camera:
    """Mirror of reference camera.h (SphereflakeRaytracer::Camera): FOV 60, angles in radians."""

    def __init__(self, width: int, height: int):
        self.width, self.height = int(width), int(height)
        self.position = np.zeros(3, np.float32)
        self.fov, self.roll, self.pitch, self.yaw = 60.0, 0.0, 0.0, 0.0

    def SetPosition(self, p):
        self.position = _f32(p, 3).copy()

    def GetPosition(self):
        return self.position.copy()

    def SetPitch(self, v): self.pitch = float(v)
    def SetYaw(self, v): self.yaw = float(v)
    def SetRoll(self, v): self.roll = float(v)
    def SetFOV(self, v): self.fov = float(v)

    def corners(self):
        o, tl, tr, bl = (np.zeros(3, np.float32) for _ in range(4))
        pos = _f32(self.position, 3)
        _check(lib().sf_camera_corners(self.width, self.height, _fp(pos), self.pitch, self.yaw, self.roll,
                                       self.fov, _fp(o), _fp(tl), _fp(tr), _fp(bl)), "sf_camera_corners")
        return o, tl, tr, bl

    def GetTopLeft(self): return self.corners()[1]
    def GetTopRight(self): return self.corners()[2]
    def GetBottomLeft(self): return self.corners()[3]


def config_camera(width: int, height: int, K: float) -> Camera:
    """The fixed camera of the BASELINE configs: main.cpp:92-96 with position scaled by K."""
    cam = Camera(width, height)
    cam.SetPosition(np.asarray(DEFAULT_CAMERA_POSITION, np.float32) * np.float32(K))
    cam.SetPitch(np.float32(DEFAULT_PITCH))
    cam.SetYaw(np.float32(DEFAULT_YAW))
    cam.SetRoll(0.0)
    return cam


# ----------------------------------------------------------------------------- the renderer

@dataclass
class GBuffer:
    """Reference GBuffer (Sphereflake.h:7-11): positions / normals as [H, W, 4] float32 (x, y, z, 1)."""
    positions: np.ndarray
    normals: np.ndarray


SF_PACKED_NORMAL = 1   # band slab: float4 (nx, ny, nz, minT) per pixel, 16 B
SF_PACKED_INDEX = 2    # band slab: uint32 hit index per pixel, 4 B (where slab_bytes() == 4)


def render_params(band_rows=0, band_count=1, band_index=0, compact=False, kernel=SF_KERNEL_WAVE,
                  emit_aux=False, max_depth=0, stream=None, packed=0) -> sf_render_params:
    """packed: 0 / False (G-buffer layout), 1 / True (16 B slab), 2 (4 B hit-index slab)."""
    return sf_render_params(band_rows, band_count, band_index, int(bool(compact)), kernel, int(bool(emit_aux)),
                            max_depth, int(packed), stream)


class _FifoLock:
    """Ticket lock: waiters are served in arrival order (the C++ class's FairMutex, Sphereflake.hpp). The
    frame-less loop re-locks right after each batch; with a plain Lock a caller's SetView / GetGBuffer
    could lose to it for many batches in a row."""

    def __init__(self):
        self._c = threading.Condition(threading.Lock())
        self._next = 0
        self._serving = 0

    def __enter__(self):
        with self._c:
            t = self._next
            self._next += 1
            while self._serving != t:
                self._c.wait()
        return self

    def __exit__(self, *exc):
        with self._c:
            self._serving += 1
            self._c.notify_all()


def _views12(views) -> np.ndarray:
    """[(origin, top-left, top-right, bottom-left), ...] (or an n x 12 float32 array) -> a contiguous float32 n x 12
    array."""
    if isinstance(views, np.ndarray) and views.dtype == np.float32 and views.ndim == 2 and views.shape[1] == 12 \
            and views.flags.c_contiguous:
        return views
    return np.ascontiguousarray(np.array([[c for v in view for c in v] for view in views], np.float32).reshape(-1, 12))


def render_frames(flakes, **kw):
    """Each flake's current view into its own G-buffer, in ONE multi-frame persistent launch (sf_render_frames):
    bit for bit what flake.Render(**kw) does for each (whole frames or bands at frame positions)."""
    import contextlib
    p = render_params(**kw)
    arr = (ctypes.c_void_p * len(flakes))(*[f.ctx for f in flakes])
    with contextlib.ExitStack() as held:   # (every context's lock once, as each Render would take its own; a
        seen = set()                        # context given twice is the C ABI's SF_EINVAL, not a deadlock here)
        for f in flakes:
            if id(f) not in seen:
                seen.add(id(f))
                held.enter_context(f._mutex)
        _check(lib().sf_render_frames(arr, len(flakes), ctypes.byref(p)), "sf_render_frames", flakes[0].ctx)


_hip = None


def _hip_runtime() -> ctypes.CDLL:
    """The HIP runtime the renderer library itself is linked against (already loaded with it: opened by its
    SONAME, the same instance). Only trace_dirs' numpy path uses it, for its device scratch."""
    global _hip
    if _hip is None:
        lib()
        H = ctypes.CDLL("libamdhip64.so.7")
        H.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        H.hipFree.argtypes = [ctypes.c_void_p]
        H.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        H.hipSetDevice.argtypes = [ctypes.c_int]
        H.hipGetDevice.argtypes = [ctypes.POINTER(ctypes.c_int)]
        _hip = H
    return _hip


class _DeviceScratch:
    """`nbytes` of device memory on `device` for the length of a with-block; synchronous copies."""

    def __init__(self, device: int, nbytes: int):
        self.device, self.nbytes, self.ptr = device, nbytes, None

    def _hipcall(self, what, rc):
        if rc != 0:
            raise SphereflakeError(SF_EHIP, f"{what} (HIP error {rc})")

    def __enter__(self):
        H = _hip_runtime()
        prev = ctypes.c_int(-1)
        H.hipGetDevice(ctypes.byref(prev))
        self._hipcall("hipSetDevice", H.hipSetDevice(self.device))
        p = ctypes.c_void_p()
        try:
            self._hipcall("hipMalloc", H.hipMalloc(ctypes.byref(p), self.nbytes))
        finally:
            if prev.value >= 0:
                H.hipSetDevice(prev.value)
        self.ptr = p.value
        return self

    def upload(self, offset: int, a: np.ndarray):
        self._hipcall("hipMemcpy", _hip_runtime().hipMemcpy(self.ptr + offset, a.ctypes.data, a.nbytes, 1))

    def download(self, offset: int, a: np.ndarray):
        self._hipcall("hipMemcpy", _hip_runtime().hipMemcpy(a.ctypes.data, self.ptr + offset, a.nbytes, 2))

    def __exit__(self, *exc):
        if self.ptr:
            _hip_runtime().hipFree(self.ptr)
            self.ptr = None


class Sphereflake:
    """Drop-in for the reference class. Owns a device context (G-buffer in HBM)."""

    def __init__(self, width: int, height: int, device: int = 0):
        self.width, self.height, self.device = int(width), int(height), int(device)
        L = lib()
        h = ctypes.c_void_p()
        _check(L.sf_create(self.device, self.width, self.height, ctypes.byref(h)), "sf_create")
        self._ctx = h
        self._worker = None
        self._stop = threading.Event()
        self._mutex = _FifoLock()
        self._seed = 0
        self._counter = 0
        self._view_change = 0
        self._worker_error = None

    # lifetime --------------------------------------------------------------
    def close(self):
        self.release_pinned()
        self._stop.set()
        if self._worker is not None:
            self._worker.join()
            self._worker = None
        if getattr(self, "_ctx", None):
            lib().sf_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def ctx(self):
        return self._ctx

    # view ------------------------------------------------------------------
    def SetView(self, origin, topLeft, topRight, bottomLeft):
        o, tl, tr, bl = (_vec3(v) for v in (origin, topLeft, topRight, bottomLeft))
        with self._mutex:   # (the frame-less loop's batches read the view)
            _check(lib().sf_set_view(self._ctx, o, tl, tr, bl), "SetView", self._ctx)
            self._view_change = self._counter

    def GetViewChangePacket(self) -> int:
        """The frame-less loop's packet counter when the last SetView took effect (batches from it on trace
        the new view)."""
        with self._mutex:
            return self._view_change

    def SetCamera(self, cam: Camera):
        o, tl, tr, bl = cam.corners()
        self.SetView(o, tl, tr, bl)

    def SetSetup(self, child, root):
        c, r = _f32(child, 144), _f32(root, 16)
        _check(lib().sf_set_setup(self._ctx, _fp(c), _fp(r)), "sf_set_setup", self._ctx)

    def GetSetup(self):
        c, r = np.zeros((9, 16), np.float32), np.zeros(16, np.float32)
        _check(lib().sf_get_setup(self._ctx, _fp(c), _fp(r)), "sf_get_setup", self._ctx)
        return c, r

    # rendering -------------------------------------------------------------
    def Render(self, **kw):
        """One deterministic frame into the device G-buffer (asynchronous)."""
        p = render_params(**kw)
        with self._mutex:
            _check(lib().sf_render(self._ctx, ctypes.byref(p)), "Render", self._ctx)

    def render_to(self, pos_ptr: int, nrm_ptr: int, min_t_ptr: int = 0, index_ptr: int = 0, **kw):
        """Render into caller-owned device buffers (e.g. torch tensor data_ptr())."""
        p = render_params(**kw)
        _check(lib().sf_render_to(self._ctx, ctypes.byref(p), ctypes.c_void_p(pos_ptr), ctypes.c_void_p(nrm_ptr),
                                  ctypes.c_void_p(min_t_ptr or None), ctypes.c_void_p(index_ptr or None)),
               "sf_render_to", self._ctx)

    # caller-supplied directions (sf_trace_dirs_to / sf_trace_dirs / sf_probe_dirs) ------------
    @staticmethod
    def _out_ptrs(out):
        """`out` of trace_dirs() / trace_rays(), four tensors or device addresses, as pointers (None for None / 0)."""
        addr = [0 if o is None else o.data_ptr() if hasattr(o, "data_ptr") else int(o) for o in out]
        return [ctypes.c_void_p(a) if a else None for a in addr]

    def _trace_host(self, lead, n, inputs, trace, outputs=True):
        """The numpy forms of trace_dirs() and trace_rays(): `inputs` uploaded to a scratch (16-byte aligned, in order),
        trace(input pointers, the four output pointers) under the mutex, a wait, and (pos4, nrm4, min_t, hit_index)
        shaped `lead` downloaded -- without `outputs` the trace writes elsewhere, and None is returned."""
        pos = np.empty(lead + (4,), np.float32)
        nrm = np.empty(lead + (4,), np.float32)
        mint = np.empty(lead, np.float32)
        idx = np.empty(lead, np.uint32)
        if n == 0:
            return pos, nrm, mint, idx
        offs, o0 = [], 0
        for a in inputs:
            offs.append(o0)
            o0 += (a.nbytes + 15) // 16 * 16
        res = ((pos, 0), (nrm, 16 * n), (mint, 32 * n), (idx, 36 * n)) if outputs else ()
        with _DeviceScratch(self.device, o0 + (n * 40 if outputs else 16)) as d:
            for a, off in zip(inputs, offs):
                d.upload(off, a)
            with self._mutex:
                trace([ctypes.c_void_p(d.ptr + off) for off in offs],
                      [ctypes.c_void_p(d.ptr + o0 + off) for _, off in res])
                # (the scratch is freed on leaving: the trace that reads and writes it must be done)
                _check(lib().sf_synchronize(self._ctx), "sf_synchronize", self._ctx)
            for a, off in res:
                d.download(o0 + off, a)
        return (pos, nrm, mint, idx) if outputs else None

    def trace_dirs(self, dirs, width=None, height=None, out=None, stride=None, max_depth=0, stream=None):
        """Trace caller-supplied directions from the current view's origin (sphereflake_amd.dirs has generators).

        dirs: a float32 array of directions, [H, W, 3 | 4] (an image, traced as 8x8 tiles) or [N, 3 | 4] (a list):
          - a numpy array: uploaded, traced, and the results returned as numpy arrays
            (pos4 [.., 4], nrm4 [.., 4], min_t [..], hit_index [..]) -- synchronous;
          - a torch CUDA tensor (contiguous float32), or a device address (int) with width, height (1: a list) and
            stride given: zero copy, asynchronous; results go to `out`.
        out: (pos4, nrm4, min_t, hit_index) torch CUDA tensors or device addresses, any of them None / 0 -- or None:
          an image of the context's frame size is then traced into the context's own G-buffer and aux channels
          (download(), PostProcess(), save_image() see it), and any other numpy input returns numpy arrays.
          out="host" returns numpy arrays for a frame-sized numpy image too."""
        host = isinstance(dirs, np.ndarray)
        if host:
            dirs = np.ascontiguousarray(dirs, np.float32)
        shape = tuple(getattr(dirs, "shape", ()))
        if shape:
            if len(shape) not in (2, 3) or shape[-1] not in (3, 4):
                raise ValueError("dirs must be [H, W, 3 | 4] or [N, 3 | 4]")
            stride = shape[-1] if stride is None else stride
            if width is None and height is None:
                height, width = (shape[0], shape[1]) if len(shape) == 3 else (1, shape[0])
            elif int(width) * int(height) != int(np.prod(shape[:-1])):
                raise ValueError("width x height does not match dirs")
            if not host:
                if not (dirs.is_cuda and dirs.is_contiguous() and dirs.element_size() == 4
                        and dirs.dtype.is_floating_point):
                    raise ValueError("dirs must be a contiguous float32 CUDA tensor")
        elif width is None or height is None or stride is None:
            raise ValueError("a device address needs width, height and stride")
        width, height = int(width), int(height)
        n = width * height
        p = sf_dirs_params(width, height, int(stride), int(max_depth), stream)
        to_ctx = out is None and (width, height) == (self.width, self.height) and height > 1
        if not host:
            dptr = dirs.data_ptr() if shape else int(dirs)
            if to_ctx:
                with self._mutex:
                    _check(lib().sf_trace_dirs(self._ctx, ctypes.byref(p), ctypes.c_void_p(dptr)), "sf_trace_dirs",
                           self._ctx)
                return None
            if out is None or isinstance(out, str):
                raise ValueError("device directions need `out` buffers (or the context's frame size)")
            if len(out) != 4:
                raise ValueError("out must be (pos4, nrm4, min_t, hit_index)")
            with self._mutex:
                _check(lib().sf_trace_dirs_to(self._ctx, ctypes.byref(p), ctypes.c_void_p(dptr), *self._out_ptrs(out)),
                       "sf_trace_dirs_to", self._ctx)
            return None
        if out is not None and not isinstance(out, str):
            raise ValueError("host directions return host arrays: out must be None or 'host'")
        lead = shape[:-1] if len(shape) == 3 else (n,)

        def trace(ins, outs):
            if to_ctx:
                _check(lib().sf_trace_dirs(self._ctx, ctypes.byref(p), ins[0]), "sf_trace_dirs", self._ctx)
            else:
                _check(lib().sf_trace_dirs_to(self._ctx, ctypes.byref(p), ins[0], *outs), "sf_trace_dirs_to", self._ctx)
        return self._trace_host(lead, n, (dirs,), trace, outputs=not to_ctx)

    def probe(self, dirs):
        """A few rays from the current view's origin, host arrays in and out (sf_probe_dirs; synchronous): picking,
        ranging, collision probes. dirs: [N, 3]. Returns (min_t [N], hit_index [N], pos4 [N, 4], nrm4 [N, 4]);
        a miss has min_t = FLT_MAX and hit_index = 0xffffffff."""
        d = np.ascontiguousarray(np.asarray(dirs, np.float32).reshape(-1, 3))
        n = d.shape[0]
        mint, idx = np.empty(n, np.float32), np.empty(n, np.uint32)
        pos, nrm = np.empty((n, 4), np.float32), np.empty((n, 4), np.float32)
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        with self._mutex:
            _check(lib().sf_probe_dirs(self._ctx, vp(d), n, vp(mint), vp(idx), vp(pos), vp(nrm)), "sf_probe_dirs",
                   self._ctx)
        return mint, idx, pos, nrm

    # caller-supplied origins and directions (sf_trace_rays_to / sf_probe_rays) ------------------
    def trace_rays(self, origins, dirs, rays_per_origin=1, out=None, dir_stride=None, origin_stride=None,
                   max_depth=0, stream=None, width=None, height=None):
        """Trace ray i from origins[i // rays_per_origin] along dirs[i] (sphereflake_amd.rays has generators): what
        the reference returns for that direction after SetView at that origin. Positions are relative to the ray's
        own origin; a sphere whose centre is behind the ray is not seen, even from inside it (sf.h).

        dirs as for trace_dirs: [H, W, 3 | 4] (an image, traced as 8x8 tiles) or [N, 3 | 4] (a list); origins
        [M, 3 | 4] with M >= ceil(rays / rays_per_origin). Both numpy arrays: uploaded, traced, and the results
        returned as numpy arrays (pos4, nrm4, min_t, hit_index) -- synchronous (`out` None or "host"). Both torch
        CUDA tensors (contiguous float32) or device addresses (ints, with width, height and the strides given): zero
        copy, asynchronous, results go to `out` = (pos4, nrm4, min_t, hit_index) tensors or addresses, any of them
        None / 0."""
        host = isinstance(dirs, np.ndarray)
        if host != isinstance(origins, np.ndarray):
            raise ValueError("origins and dirs must both be host arrays or both be on the device")
        if host:
            dirs = np.ascontiguousarray(dirs, np.float32)
            origins = np.ascontiguousarray(origins, np.float32)
        shape = tuple(getattr(dirs, "shape", ()))
        oshape = tuple(getattr(origins, "shape", ()))
        if shape:
            if len(shape) not in (2, 3) or shape[-1] not in (3, 4):
                raise ValueError("dirs must be [H, W, 3 | 4] or [N, 3 | 4]")
            dir_stride = shape[-1] if dir_stride is None else dir_stride
            if width is None and height is None:
                height, width = (shape[0], shape[1]) if len(shape) == 3 else (1, shape[0])
            elif int(width) * int(height) != int(np.prod(shape[:-1])):
                raise ValueError("width x height does not match dirs")
        elif width is None or height is None or dir_stride is None:
            raise ValueError("a device address needs width, height and dir_stride")
        width, height = int(width), int(height)
        n = width * height
        rpo = max(int(rays_per_origin), 1)
        if oshape:
            if len(oshape) != 2 or oshape[-1] not in (3, 4):
                raise ValueError("origins must be [M, 3 | 4]")
            origin_stride = oshape[-1] if origin_stride is None else origin_stride
            if oshape[0] * rpo < n:
                raise ValueError("too few origins for the rays")
        elif origin_stride is None:
            raise ValueError("a device address needs origin_stride")
        if not host:
            for t in (dirs, origins):
                if hasattr(t, "data_ptr") and not (t.is_cuda and t.is_contiguous() and t.element_size() == 4
                                                   and t.dtype.is_floating_point):
                    raise ValueError("origins and dirs must be contiguous float32 CUDA tensors")
        p = sf_rays_params(width, height, int(dir_stride), int(origin_stride), rpo, int(max_depth), stream)
        if not host:
            if out is None or isinstance(out, str) or len(out) != 4:
                raise ValueError("device rays need out = (pos4, nrm4, min_t, hit_index)")
            dptr = dirs.data_ptr() if shape else int(dirs)
            optr = origins.data_ptr() if oshape else int(origins)
            with self._mutex:
                _check(lib().sf_trace_rays_to(self._ctx, ctypes.byref(p), ctypes.c_void_p(optr or None),
                                              ctypes.c_void_p(dptr or None), *self._out_ptrs(out)), "sf_trace_rays_to",
                       self._ctx)
            return None
        if out is not None and not isinstance(out, str):
            raise ValueError("host rays return host arrays: out must be None or 'host'")
        lead = shape[:-1] if len(shape) == 3 else (n,)
        return self._trace_host(lead, n, (dirs, origins), lambda ins, outs: _check(
            lib().sf_trace_rays_to(self._ctx, ctypes.byref(p), ins[1], ins[0], *outs), "sf_trace_rays_to", self._ctx))

    def probe_rays(self, origins, dirs, rays_per_origin=1):
        """A few rays from caller-supplied origins, host arrays in and out (sf_probe_rays; synchronous): the
        look-ahead brake (rays.look_ahead), picking from points that are not the camera. origins [M, 3], dirs [N, 3],
        ray i from origins[i // rays_per_origin]. Returns (min_t [N], hit_index [N], pos4 [N, 4], nrm4 [N, 4])."""
        d = np.ascontiguousarray(np.asarray(dirs, np.float32).reshape(-1, 3))
        o = np.ascontiguousarray(np.asarray(origins, np.float32).reshape(-1, 3))
        n = d.shape[0]
        rpo = max(int(rays_per_origin), 1)
        if o.shape[0] * rpo < n:
            raise ValueError("too few origins for the rays")
        mint, idx = np.empty(n, np.float32), np.empty(n, np.uint32)
        pos, nrm = np.empty((n, 4), np.float32), np.empty((n, 4), np.float32)
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        with self._mutex:
            _check(lib().sf_probe_rays(self._ctx, vp(o), vp(d), n, rpo, vp(mint), vp(idx), vp(pos), vp(nrm)),
                   "sf_probe_rays", self._ctx)
        return mint, idx, pos, nrm

    # what the light traces' builders, image passes and own buffers share ----------
    def _defaults(self, block):
        """A parameter block after its sf_*_defaults (_DEFAULTS names it)."""
        p = block()
        _check(getattr(lib(), _DEFAULTS[block])(self._ctx, ctypes.byref(p)), _DEFAULTS[block])
        return p

    def _list_params(self, block, field, entries, per, limit, what, vfield, values, vper, message):
        """(block, keepalive) of a trace of a list: `block` after its defaults with p.n and p.`field` set from `entries`
        (_entries) and, where `values` are given, p.`vfield` from them (_entry_values)."""
        e = _entries(entries, per, limit, what)
        p = self._defaults(block)
        setattr(p, field, _fp(e))
        v = _entry_values(values, e.shape[0], vper, message)
        if v is not None:
            setattr(p, vfield, _fp(v))
        p.n = e.shape[0]
        return p, (e, v)

    def _light_image(self, entry, p, lead, ptrs, keep=None):
        """The light_image* calls: entry(ctx, p, *lead, *ptrs), device addresses with 0 as null. `keep`: the host
        arrays p points into, held by this frame until the call has returned."""
        with self._mutex:
            _check(getattr(lib(), entry)(self._ctx, ctypes.byref(p), *lead,
                                         *(ctypes.c_void_p(x) if x else None for x in ptrs)), entry, self._ctx)

    def _own_pointer(self, entry) -> int:
        """The device address of one of the context's own result buffers (0 where there is none yet)."""
        ptr = ctypes.c_void_p()
        rc = getattr(lib(), entry)(self._ctx, ctypes.byref(ptr))
        if rc == SF_ESTATE:
            return 0
        _check(rc, entry)
        return ptr.value or 0

    def _own_download(self, entry, dtype, tail=()) -> np.ndarray:
        """[H, W] + tail elements of one of the context's own result buffers (synchronous)."""
        a = np.empty((self.height, self.width) + tail, dtype)
        with self._mutex:
            _check(getattr(lib(), entry)(self._ctx, a.ctypes.data_as(ctypes.c_void_p)), entry, self._ctx)
        return a

    # shadows from a point light (sf_trace_shadow_to / sf_trace_shadow / sf_light_image) ----------
    def shadow_params(self, light, bias=None, origin=None, width=0, height=0, max_depth=0, stream=None):
        """sf_shadow_defaults, overridden: bias None keeps the library's default."""
        p = self._defaults(sf_shadow_params)
        p.light[:] = [float(x) for x in _f32(light, 3)]
        return _params_tail(p, None, bias, origin, width, height, max_depth, stream)

    def trace_shadow(self, light, bias=None, pos=None, out=None, origin=None, max_depth=0, stream=None):
        """Which pixels of a position image does a point light at `light` (world) reach? 255 = lit or a miss of the
        frame, 0 = shadowed; the exact definition is in sf.h and sphereflake_amd.lights.shadow_model.

        pos: the view-space position image, relative to `origin` (None: the context's view origin):
          - None: the context's own G-buffer (after Render()), into the context's visibility buffer
            (download_shadow() and light_image() see it) or, with `out`, into that buffer -- asynchronous;
          - a numpy array [H, W, 4]: uploaded, traced, and a numpy [H, W] uint8 returned -- synchronous;
          - a torch CUDA tensor [H, W, 4] (contiguous float32), or a (device address, width, height) tuple: zero
            copy, asynchronous; the result goes to `out`.
        out: a torch CUDA uint8 tensor of H x W elements, or a device address."""
        return self._trace_images(lambda W, H: self.shadow_params(light, bias, origin, W, H, max_depth, stream),
                                  "sf_trace_shadow", pos, out, np.uint8)

    @staticmethod
    def _image4(a, what):
        """(device address, width, height) of a contiguous float32 CUDA tensor [H, W, 4] or such a tuple."""
        if hasattr(a, "data_ptr"):
            shape = tuple(a.shape)
            if len(shape) != 3 or shape[-1] != 4 or not (a.is_cuda and a.is_contiguous() and a.element_size() == 4
                                                         and a.dtype.is_floating_point):
                raise ValueError(f"{what} must be a contiguous float32 CUDA tensor [H, W, 4]")
            return a.data_ptr(), shape[1], shape[0]
        ptr, W, H = (int(x) for x in a)
        return ptr, W, H

    def _trace_images(self, params, entry, pos, out, dtype, tail=(), normals=False, nrm=None, accumulate=False,
                      lead=(), buf=None, has_buf=False):
        """The `pos` / `nrm` / `out` forms of the light traces and of the light filter. params(width, height) makes the
        call's parameter block, or (block, the host arrays it points into, kept alive until the call has returned); `entry` names the
        call into the context's own buffers, `entry`_to the one into a caller's. The result is `dtype` x `tail` per
        pixel; `normals`: a normal image `nrm` travels with the position image; `accumulate`: the host form takes its
        base as `out` and uploads it. `lead`: what the call takes between its parameter block and its images (the spin);
        `has_buf`: a float4 input image `buf` travels after the normals (the filter's light buffer; a device `buf` may
        go with the context's own G-buffer, pos None)."""
        to, own = getattr(lib(), entry + "_to"), getattr(lib(), entry)
        vp = lambda x: ctypes.c_void_p(x) if x else None

        def make(W, H):
            p = params(W, H)
            return p if isinstance(p, tuple) else (p, None)
        if isinstance(pos, np.ndarray):
            pos = np.ascontiguousarray(pos, np.float32)
            if pos.ndim != 3 or pos.shape[-1] != 4:
                raise ValueError("pos must be [H, W, 4]")
            images = [pos]
            if normals:
                if not isinstance(nrm, np.ndarray):
                    raise ValueError("a host position image needs a host normal image")
                nrm = np.ascontiguousarray(nrm, np.float32)
                if nrm.shape != pos.shape:
                    raise ValueError("nrm and pos must have the same shape")
                images.append(nrm)
            if has_buf:
                if not isinstance(buf, np.ndarray):
                    raise ValueError("a host position image needs a host light buffer")
                buf = np.ascontiguousarray(buf, np.float32)
                if buf.shape != pos.shape:
                    raise ValueError("buf and pos must have the same shape")
                images.append(buf)
            H, W = pos.shape[:2]
            if accumulate:
                if not isinstance(out, np.ndarray) or out.shape != (H, W) + tail:
                    raise ValueError("an accumulating call on host images needs the base as `out` [H, W, 4]")
                res = np.array(out, dtype, copy=True, order="C")
            elif out is not None:
                raise ValueError("a host position image returns a host array: out must be None")
            else:
                res = np.empty((H, W) + tail, dtype)
            p, keep = make(W, H)
            if H * W == 0:
                return res
            offs = [k * pos.nbytes for k in range(len(images) + 1)]   # the images, then the result
            with _DeviceScratch(self.device, offs[-1] + res.nbytes) as d:
                for a, off in zip(images, offs):
                    d.upload(off, a)
                if accumulate:
                    d.upload(offs[-1], res)
                with self._mutex:
                    _check(to(self._ctx, ctypes.byref(p), *lead, *[vp(d.ptr + off) for off in offs]), entry + "_to",
                           self._ctx)
                    # (the scratch is freed on leaving: the trace that reads and writes it must be done)
                    _check(lib().sf_synchronize(self._ctx), "sf_synchronize", self._ctx)
                d.download(offs[-1], res)
            del keep
            return res
        optr = 0 if out is None else out.data_ptr() if hasattr(out, "data_ptr") else int(out)
        if pos is None:
            if nrm is not None:
                raise ValueError("nrm goes with pos: None selects the context's G-buffer for both")
            ptrs = [0] * (2 if normals else 1)
            if has_buf:
                if isinstance(buf, np.ndarray):
                    raise ValueError("a host light buffer goes with host images")
                ptrs.append(0 if buf is None else buf.data_ptr() if hasattr(buf, "data_ptr") else int(buf))
                if ptrs[-1] and not optr:
                    raise ValueError("a caller's light buffer needs an `out` buffer")
        else:
            pptr, W, H = self._image4(pos, "pos")
            ptrs = [pptr]
            if normals:
                if nrm is None or isinstance(nrm, np.ndarray):
                    raise ValueError("a device position image needs a device normal image")
                ptrs.append(self._image4(nrm, "nrm")[0] if hasattr(nrm, "data_ptr") or isinstance(nrm, (tuple, list))
                            else int(nrm))
            if has_buf:
                if buf is None or isinstance(buf, np.ndarray):
                    raise ValueError("a device position image needs a device light buffer")
                ptrs.append(self._image4(buf, "buf")[0] if hasattr(buf, "data_ptr") or isinstance(buf, (tuple, list))
                            else int(buf))
            if not optr:
                raise ValueError("a device position image needs an `out` buffer")
        p, keep = make(0, 0) if pos is None else make(W, H)
        with self._mutex:
            if pos is None and not optr:
                _check(own(self._ctx, ctypes.byref(p), *lead), entry, self._ctx)
            else:
                _check(to(self._ctx, ctypes.byref(p), *lead, *[vp(x) for x in ptrs], vp(optr)), entry + "_to",
                       self._ctx)
        del keep
        return None

    def download_shadow(self) -> np.ndarray:
        """[H, W] uint8 of the last trace_shadow() into the context's visibility buffer (synchronous)."""
        return self._own_download("sf_download_shadow", np.uint8)

    def shadow_buffer(self) -> int:
        """Device address of the context's visibility buffer (0 before any trace_shadow() into it)."""
        return self._own_pointer("sf_shadow_buffer")

    def light_image(self, light, ambient=0.25, origin=None, pos_ptr=0, nrm_ptr=0, vis_ptr=0, rgba_ptr=0, stream=None):
        """Scale the image of PostProcess() in place by ambient + (1 - ambient) x (lit ? Lambert term : 0)
        (sf_light_image; sphereflake_amd.lights.light_model). Pointers are device addresses, 0 = the context's
        G-buffer, visibility buffer (trace_shadow()) and image. Asynchronous."""
        p = self.shadow_params(light, None, origin, 0, 0, 0, stream)
        self._light_image("sf_light_image", p, (float(ambient),), (pos_ptr, nrm_ptr, vis_ptr, rgba_ptr))

    # many lights per pixel in one launch (sf_trace_shadows_to / sf_trace_shadows / sf_light_image_many) ----------
    def shadows_params(self, lights, weights=None, bias=None, origin=None, width=0, height=0, max_depth=0, stream=None):
        """sf_shadows_defaults, overridden: (params, keepalive). lights [n, 3], weights [n] or None; the host arrays
        the params point into are in `keepalive` and must outlive the call they are passed to."""
        p, keep = self._list_params(sf_shadows_params, "lights", lights, 3, SF_SHADOW_LIGHTS_MAX, "lights",
                                    "weights", weights, 1, "one weight per light")
        return _params_tail(p, None, bias, origin, width, height, max_depth, stream), keep

    def trace_shadows(self, lights, bias=None, pos=None, out=None, max_depth=0, origin=None, stream=None):
        """Which of up to 64 point lights `lights` [n, 3] (world) reach each pixel of a position image, in one launch:
        a uint64 per pixel, bit i = 1 where trace_shadow(lights[i]) gives 255 (lit, or a miss of the frame), 0 where
        it gives 0; bits n..63 are 0 (sf.h). `pos` and `out` as trace_shadow's:
          - None: the context's own G-buffer (after Render()), into the context's mask buffer
            (download_shadow_masks() and light_image_many() see it) or, with `out`, into that buffer -- asynchronous;
          - a numpy array [H, W, 4]: uploaded, traced, and a numpy [H, W] uint64 returned -- synchronous;
          - a torch CUDA tensor [H, W, 4] (contiguous float32), or a (device address, width, height) tuple: zero
            copy, asynchronous; the result goes to `out`.
        out: a torch CUDA tensor of H x W 8-byte elements, or a device address (8-byte aligned)."""
        return self._trace_images(
            lambda W, H: self.shadows_params(lights, None, bias, origin, W, H, max_depth, stream),
            "sf_trace_shadows", pos, out, np.uint64)

    def download_shadow_masks(self) -> np.ndarray:
        """[H, W] uint64 of the last trace_shadows() into the context's mask buffer (synchronous)."""
        return self._own_download("sf_download_shadow_masks", np.uint64)

    def shadow_mask_buffer(self) -> int:
        """Device address of the context's mask buffer (0 before any trace_shadows() into it)."""
        return self._own_pointer("sf_shadow_mask_buffer")

    def light_image_many(self, lights, weights=None, ambient=0.25, origin=None, pos_ptr=0, nrm_ptr=0, mask_ptr=0,
                         rgba_ptr=0, stream=None):
        """Scale the image of PostProcess() in place by ambient + (1 - ambient) x sum_i w_i (lit_i ? Lambert_i : 0)
        over the lights (sf_light_image_many; sphereflake_amd.lights.light_model_many). weights None: 1 / n each.
        Pointers are device addresses, 0 = the context's G-buffer, mask buffer (trace_shadows()) and image.
        Asynchronous."""
        p, keep = self.shadows_params(lights, weights, None, origin, 0, 0, 0, stream)
        self._light_image("sf_light_image_many", p, (float(ambient),), (pos_ptr, nrm_ptr, mask_ptr, rgba_ptr), keep)

    # the shadow traces' level of detail, shadows from a directional light (sf_set_shadow_lod, sf_trace_sun_to) -------
    def set_shadow_lod(self, lod_constant):
        """trace_shadow(), trace_shadows(), trace_sun(), trace_suns(), trace_shafts(), trace_ao() and their summing
        forms refine a node while
        sqrtf(t / r) < lod_constant instead of the variant's 70 / 60; 0 restores the variant's own (the default).
        Nothing else is affected: Render(), trace_dirs() and trace_rays() keep the variant's constant.
        sphereflake_amd.lights.matched_lod picks a value. Synchronous."""
        with self._mutex:
            _check(lib().sf_set_shadow_lod(self._ctx, float(lod_constant)), "sf_set_shadow_lod", self._ctx)

    def get_shadow_lod(self) -> float:
        return float(lib().sf_get_shadow_lod(self._ctx))

    def sun_params(self, direction, distance=None, bias=None, origin=None, width=0, height=0, max_depth=0, stream=None):
        """sf_sun_defaults, overridden: distance and bias None keep the library's defaults (4, 2^-10)."""
        p = self._defaults(sf_sun_params)
        p.dir[:] = [float(x) for x in _f32(direction, 3)]
        return _params_tail(p, distance, bias, origin, width, height, max_depth, stream)

    def trace_sun(self, direction, distance=None, bias=None, pos=None, out=None, origin=None, max_depth=0, stream=None):
        """Which pixels of a position image does a directional light reach? `direction` points TOWARDS the sun (world,
        used as given: sphereflake_amd.lights.sun_direction normalises); every pixel's ray starts `distance` up that
        direction from its own surface point. 255 = lit or a miss of the frame, 0 = shadowed; the exact definition is
        in sf.h and sphereflake_amd.lights.sun_model. `pos`, `out` and `origin` as trace_shadow's; the context's
        visibility buffer is the one trace_shadow() writes (download_shadow(), light_image_sun() see it)."""
        return self._trace_images(
            lambda W, H: self.sun_params(direction, distance, bias, origin, W, H, max_depth, stream),
            "sf_trace_sun", pos, out, np.uint8)

    def light_image_sun(self, direction, ambient=0.25, pos_ptr=0, nrm_ptr=0, vis_ptr=0, rgba_ptr=0, stream=None):
        """Scale the image of PostProcess() in place by ambient + (1 - ambient) x (lit ? max(0, n . direction) : 0)
        (sf_light_image_sun; sphereflake_amd.lights.light_model_sun). Pointers as light_image's. Asynchronous."""
        p = self.sun_params(direction, None, None, None, 0, 0, 0, stream)
        self._light_image("sf_light_image_sun", p, (float(ambient),), (pos_ptr, nrm_ptr, vis_ptr, rgba_ptr))

    # many sun directions per pixel in one launch (sf_trace_suns_to / sf_trace_suns / sf_light_image_suns) ----------
    def suns_params(self, dirs, weights=None, distance=None, bias=None, origin=None, width=0, height=0, max_depth=0,
                    stream=None):
        """sf_suns_defaults, overridden: (params, keepalive). dirs [n, 3], weights [n] or None; distance and bias None
        keep the library's defaults (4, 2^-10). The host arrays the params point into are in `keepalive` and must
        outlive the call they are passed to."""
        p, keep = self._list_params(sf_suns_params, "dirs", dirs, 3, SF_SUN_DIRS_MAX, "directions",
                                    "weights", weights, 1, "one weight per direction")
        return _params_tail(p, distance, bias, origin, width, height, max_depth, stream), keep

    def trace_suns(self, dirs, distance=None, bias=None, pos=None, out=None, origin=None, max_depth=0, stream=None):
        """Which of up to 64 sun directions `dirs` [n, 3] (each TOWARDS the sun, world, used as given) reach each pixel
        of a position image, in one launch: a uint64 per pixel, bit i = 1 where trace_sun(dirs[i]) with the same
        distance and bias gives 255 (lit, or a miss of the frame), 0 where it gives 0; bits n..63 are 0 (sf.h).
        sphereflake_amd.lights.sun_cone samples a sun with an angular size, sky_dirs a sky dome. `pos`, `out` and
        `origin` as trace_shadows'; the context's mask buffer is the one trace_shadows() writes
        (download_shadow_masks(), light_image_suns() see it)."""
        return self._trace_images(
            lambda W, H: self.suns_params(dirs, None, distance, bias, origin, W, H, max_depth, stream),
            "sf_trace_suns", pos, out, np.uint64)

    def light_image_suns(self, dirs, weights=None, ambient=0.25, pos_ptr=0, nrm_ptr=0, mask_ptr=0, rgba_ptr=0,
                         stream=None):
        """Scale the image of PostProcess() in place by ambient + (1 - ambient) x sum_i w_i (lit_i ? max(0, n . dirs[i])
        : 0) over the directions (sf_light_image_suns; sphereflake_amd.lights.light_model_suns). weights None: 1 / n
        each. Pointers are device addresses, 0 = the context's G-buffer, mask buffer (trace_suns()) and image.
        Asynchronous."""
        p, keep = self.suns_params(dirs, weights, None, None, None, 0, 0, 0, stream)
        self._light_image("sf_light_image_suns", p, (float(ambient),), (pos_ptr, nrm_ptr, mask_ptr, rgba_ptr), keep)

    # light shafts: sun visibility along each pixel's view ray (sf_trace_shafts_to / sf_trace_shafts /
    # sf_light_image_shafts) -------------------------------------------------------------------------------------------
    def shafts_params(self, direction, fractions, weights=None, distance=None, bias=None, dirs_ptr=0, dirs_stride=0,
                      far=0.0, origin=None, width=0, height=0, max_depth=0, stream=None):
        """sf_shafts_defaults, overridden: (params, keepalive). fractions [n], weights [n] or None; distance and bias
        None keep the library's defaults (4, 2^-10); dirs_ptr is a device address (0 = none) of dirs_stride floats per
        pixel. The host arrays the params point into are in `keepalive` and must outlive the call they are passed to."""
        F = _entries(fractions, 1, SF_SHAFT_SAMPLES_MAX, "samples")
        p = self._defaults(sf_shafts_params)
        p.dir[:] = [float(x) for x in _f32(direction, 3)]   # (before the weights, so _list_params does not fit)
        p.fractions, p.n = _fp(F), F.shape[0]
        wts = _entry_values(weights, F.shape[0], 1, "one weight per sample")
        if wts is not None:
            p.weights = _fp(wts)
        p.dirs = ctypes.cast(ctypes.c_void_p(int(dirs_ptr) or None), ctypes.POINTER(ctypes.c_float))
        p.dirs_stride, p.far = int(dirs_stride), float(far)
        return _params_tail(p, distance, bias, origin, width, height, max_depth, stream), (F, wts)

    @staticmethod
    def _dirs_image(dirs):
        """(device address, floats per pixel) of a direction image given as a torch CUDA tensor [H, W, 3 or 4], a
        device address (3 floats per pixel) or (address, stride); (0, 0) for None."""
        if dirs is None:
            return 0, 0
        if hasattr(dirs, "data_ptr"):
            shape = tuple(dirs.shape)
            if len(shape) != 3 or shape[-1] not in (3, 4) or not (dirs.is_cuda and dirs.is_contiguous()
                                                                   and dirs.element_size() == 4
                                                                   and dirs.dtype.is_floating_point):
                raise ValueError("dirs must be a contiguous float32 CUDA tensor [H, W, 3] or [H, W, 4]")
            return dirs.data_ptr(), shape[-1]
        if isinstance(dirs, (tuple, list)):
            return int(dirs[0]), int(dirs[1])
        return int(dirs), 3

    def trace_shafts(self, direction, fractions, distance=None, bias=None, pos=None, dirs=None, far=0.0, out=None,
                     origin=None, max_depth=0, stream=None):
        """Which of up to 64 points along each pixel's view ray does the sun reach, in one launch: a uint64 per pixel,
        bit i = 1 where trace_sun(direction) with the same distance and bias gives 255 at the point fractions[i] of
        the way from the image's origin to the pixel's march end, 0 where it gives 0; bits n..63 are 0 (sf.h). The
        march end is the pixel's surface point, or for a miss of the frame `far` along its direction in `dirs`
        ([H, W, 3 or 4], used as given; None or far = 0: a miss is not marched and has its low n bits set).
        sphereflake_amd.lights.shaft_fractions makes fractions, shaft_distance a safe `distance`. `pos`, `out` and
        `origin` as trace_suns'; `dirs` a numpy array (uploaded beside `pos`), a torch CUDA tensor, a device address
        (3 floats per pixel) or (address, stride). The context's mask buffer is the one trace_shadows() and
        trace_suns() write (download_shadow_masks(), light_image_shafts() see it)."""
        def run(dptr, dstride):
            return self._trace_images(
                lambda W, H: self.shafts_params(direction, fractions, None, distance, bias, dptr, dstride, far, origin,
                                                W, H, max_depth, stream),
                "sf_trace_shafts", pos, out, np.uint64)
        if pos is None:
            size = (self.height, self.width)
        elif hasattr(pos, "shape"):
            size = tuple(pos.shape[:2])
        else:
            size = (int(pos[2]), int(pos[1]))
        if hasattr(dirs, "shape") and tuple(dirs.shape[:2]) != size:
            raise ValueError("dirs and pos must have the same height and width")
        if not isinstance(dirs, np.ndarray):
            return run(*self._dirs_image(dirs))
        D = np.ascontiguousarray(dirs, np.float32)
        if D.ndim != 3 or D.shape[-1] not in (3, 4):
            raise ValueError("dirs must be [H, W, 3] or [H, W, 4]")
        if D.size == 0:
            return run(0, 0)
        with _DeviceScratch(self.device, D.nbytes) as d:
            d.upload(0, D)
            res = run(d.ptr, D.shape[-1])
            # (the scratch is freed on leaving: the trace that reads it must be done)
            _check(lib().sf_synchronize(self._ctx), "sf_synchronize", self._ctx)
        return res

    def light_image_shafts(self, fractions, weights=None, gain=1.0, colour=(255.0, 255.0, 255.0), dirs=None, far=0.0,
                           pos_ptr=0, mask_ptr=0, rgba_ptr=0, stream=None):
        """Blend the image of PostProcess() in place towards `colour` (r, g, b in [0, 255]) by
        min(gain x |march end| x sum_i (bit i ? w_i : 0), 1) (sf_light_image_shafts;
        sphereflake_amd.lights.light_model_shafts): the in-scatter of the samples of trace_shafts(). weights None:
        1 / n each. `dirs` (a torch CUDA tensor, a device address or (address, stride); not a numpy array) and `far`
        as given to trace_shafts(). Pointers are device addresses, 0 = the context's G-buffer, mask buffer and image.
        Asynchronous."""
        if isinstance(dirs, np.ndarray):
            raise ValueError("light_image_shafts is asynchronous: dirs must be on the device")
        dptr, dstride = self._dirs_image(dirs)
        p, keep = self.shafts_params((0.0, 0.0, 1.0), fractions, weights, None, None, dptr, dstride, far, None, 0, 0, 0,
                                     stream)
        col = (ctypes.c_float * 3)(*[float(x) for x in _f32(colour, 3)])
        self._light_image("sf_light_image_shafts", p, (float(gain), col), (pos_ptr, mask_ptr, rgba_ptr), keep)

    # the colour light buffer: sum any number of suns and lights while tracing (sf_trace_suns_sum_to /
    # sf_trace_shadows_sum_to / sf_light_fill / sf_light_image_buffer) ------------------------------------------------
    def light_sum_params(self, points, colours=None, accumulate=False, distance=None, bias=None, origin=None, width=0,
                         height=0, max_depth=0, stream=None):
        """sf_light_sum_defaults, overridden: (params, keepalive). points [n, 3] (sun directions or light positions),
        colours [n, 3] or None (1 / n per component); distance and bias None keep the library's defaults (4, 2^-10).
        The host arrays the params point into are in `keepalive` and must outlive the call they are passed to."""
        p, keep = self._list_params(sf_light_sum_params, "points", points, 3, SF_LIGHT_SUM_MAX, "entries",
                                    "colours", colours, 3, "one colour per entry")
        p.accumulate = 1 if accumulate else 0
        return _params_tail(p, distance, bias, origin, width, height, max_depth, stream), keep

    def trace_suns_sum(self, dirs, colours=None, accumulate=False, distance=None, bias=None, pos=None, nrm=None,
                       out=None, origin=None, max_depth=0, stream=None):
        """Add the light of any number (1..65536) of sun directions `dirs` [n, 3] (each TOWARDS the sun, used as given),
        each with an RGB colour `colours` [n, 3] (None: 1 / n per component), into a float4 light buffer while tracing
        them: per surface pixel and channel, in index order, S += colour_i x (lit_i ? max(0, n . dirs[i]) : 0) with
        lit_i trace_suns()' bit (sf.h; sphereflake_amd.lights.sum_model). accumulate False starts from 0 and zeroes
        the frame's misses, True adds to what the buffer holds and leaves the misses alone.
          - pos None: the context's own G-buffer (after Render()) into the context's light buffer (download_light(),
            light_image_buffer() see it) or, with `out`, into that buffer -- asynchronous;
          - pos, nrm numpy arrays [H, W, 4]: uploaded, traced, and a numpy [H, W, 4] float32 returned (an accumulating
            call takes its base as `out`, a numpy array it does not change) -- synchronous;
          - pos, nrm torch CUDA tensors [H, W, 4] (contiguous float32) or (device address, width, height) tuples: zero
            copy, asynchronous; `out` a torch CUDA tensor [H, W, 4] or a device address."""
        return self._trace_images(
            lambda W, H: self.light_sum_params(dirs, colours, accumulate, distance, bias, origin, W, H, max_depth, stream),
            "sf_trace_suns_sum", pos, out, np.float32, (4,), normals=True, nrm=nrm, accumulate=accumulate)

    def trace_shadows_sum(self, lights, colours=None, accumulate=False, bias=None, pos=None, nrm=None, out=None,
                          origin=None, max_depth=0, stream=None):
        """trace_suns_sum() for point lights `lights` [n, 3] (world): lit_i is trace_shadows()' bit and the Lambert term
        light_image_many()'s."""
        return self._trace_images(
            lambda W, H: self.light_sum_params(lights, colours, accumulate, None, bias, origin, W, H, max_depth, stream),
            "sf_trace_shadows_sum", pos, out, np.float32, (4,), normals=True, nrm=nrm, accumulate=accumulate)

    def light_fill(self, rgb, buf_ptr=0, stream=None):
        """Every pixel of the light buffer becomes (r, g, b, 0): the ambient term (sf_light_fill). buf_ptr 0 = the
        context's buffer, allocated on first use. Asynchronous."""
        col = (ctypes.c_float * 3)(*[float(x) for x in _f32(rgb, 3)])
        with self._mutex:
            _check(lib().sf_light_fill(self._ctx, col, ctypes.c_void_p(buf_ptr) if buf_ptr else None, stream),
                   "sf_light_fill", self._ctx)

    def light_buffer(self) -> int:
        """Device address of the context's light buffer (0 before anything has written it)."""
        return self._own_pointer("sf_light_buffer")

    def download_light(self) -> np.ndarray:
        """[H, W, 4] float32 of the context's light buffer (synchronous)."""
        return self._own_download("sf_download_light", np.float32, (4,))

    def light_image_buffer(self, pos_ptr=0, buf_ptr=0, rgba_ptr=0, stream=None):
        """Scale the image of PostProcess() in place, per channel, by the light buffer (sf_light_image_buffer;
        sphereflake_amd.lights.light_model_buffer). Pointers are device addresses, 0 = the context's G-buffer, light
        buffer and image. Asynchronous."""
        vp = lambda x: ctypes.c_void_p(x) if x else None
        with self._mutex:
            _check(lib().sf_light_image_buffer(self._ctx, stream, vp(pos_ptr), vp(buf_ptr), vp(rgba_ptr)),
                   "sf_light_image_buffer", self._ctx)

    # ambient occlusion about each pixel's normal (sf_trace_ao_to / sf_trace_ao / sf_trace_ao_sum_to / sf_trace_ao_sum) --
    def ao_params(self, samples, colours=None, accumulate=False, distance=None, bias=None, origin=None, width=0,
                  height=0, max_depth=0, stream=None):
        """sf_ao_defaults, overridden: (params, keepalive). samples [n, 3] in the frame about the normal, colours
        [n, 3] or None (1 / n per component; the summing call only); distance and bias None keep the library's
        defaults (4, 2^-10). The host arrays the params point into are in `keepalive` and must outlive the call they are
        passed to."""
        p, keep = self._list_params(sf_ao_params, "samples", samples, 3, SF_AO_SAMPLES_MAX, "samples",
                                    "colours", colours, 3, "one colour per sample")
        p.accumulate = 1 if accumulate else 0
        return _params_tail(p, distance, bias, origin, width, height, max_depth, stream), keep

    @staticmethod
    def _spin(spin):
        """(entry suffix, lead arguments, keepalive) of a trace_ao call: spin None takes the unspun entry points; a
        table [size, size, 2] (sphereflake_amd.lights.ao_spins) or one (c, s) pair the spun ones (sf_ao_spin)."""
        if spin is None:
            return "", (), None
        t = np.ascontiguousarray(np.asarray(spin, np.float32))
        if t.shape == (2,):
            t = t.reshape(1, 1, 2)
        if t.ndim != 3 or t.shape[0] != t.shape[1] or t.shape[2] != 2 or not 1 <= t.shape[0] <= SF_AO_SPIN_MAX:
            raise ValueError(f"spin is one (c, s) pair or a table [size, size, 2], size 1..{SF_AO_SPIN_MAX}")
        sp = sf_ao_spin()
        sp.cs = t.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        sp.size = t.shape[0]
        return "_spin", (ctypes.byref(sp),), (sp, t)

    def trace_ao(self, samples, distance=4.0, bias=2.0 ** -10, pos=None, nrm=None, out=None, max_depth=0, stream=None,
                 origin=None, spin=None):
        """Ray-traced ambient occlusion: which of up to 64 directions over the hemisphere about EACH PIXEL'S OWN normal
        are open, in one launch. `samples` [n, 3] are directions in the local frame whose z axis is the normal
        (sphereflake_amd.lights.ao_samples), used as given; each pixel turns them about its normal (the frame of Duff
        et al.) and traces them as trace_suns() traces its directions: a uint64 per pixel, bit i = 1 where sample i's
        ray from `distance` up its direction reaches the pixel (or the pixel is a miss of the frame), 0 where it is
        stopped; bits n..63 are 0 (sf.h; sphereflake_amd.lights.ao_model).
          - pos None: the context's own G-buffer (after Render()) into the context's mask buffer, the one
            trace_suns() writes (download_shadow_masks() sees it), or, with `out`, into that buffer -- asynchronous;
          - pos, nrm numpy arrays [H, W, 4]: uploaded, traced, and a numpy [H, W] uint64 returned -- synchronous;
          - pos, nrm torch CUDA tensors [H, W, 4] (contiguous float32) or (device address, width, height) tuples: zero
            copy, asynchronous; `out` a torch CUDA tensor of H x W 8-byte elements or a device address.
        `origin` is what pos is relative to (None: the context's view origin).
        spin: None, or a table [size, size, 2] of (cos, sin) pairs (sphereflake_amd.lights.ao_spins), size 1..8:
        pixel (x, y) of the image turns its frame about its normal by entry (y % size, x % size) before the samples
        are laid out, so a size x size block sees n size^2 directions (sf_trace_ao_spin_to, sf.h); light_filter()
        gathers the block back."""
        suffix, lead, keep = self._spin(spin)
        res = self._trace_images(
            lambda W, H: self.ao_params(samples, None, False, distance, bias, origin, W, H, max_depth, stream),
            "sf_trace_ao" + suffix, pos, out, np.uint64, normals=True, nrm=nrm, lead=lead)
        del keep
        return res

    def trace_ao_sum(self, samples, colours=None, accumulate=False, distance=4.0, bias=2.0 ** -10, pos=None, nrm=None,
                     out=None, max_depth=0, stream=None, origin=None, spin=None):
        """trace_ao() with trace_suns_sum()'s ending: per surface pixel and channel, in index order,
        S += colour_i x (open_i ? 1 : 0) into a float4 light buffer -- no Lambert term: the cosine weighting lives in the
        sample set and the colours (sphereflake_amd.lights.ao_samples, ao_colours, ao_sum_model). colours [n, 3] (None:
        1 / n per component); accumulate, pos, nrm and out as trace_suns_sum()'s. At most 64 samples per call: more are
        further accumulating calls. spin: as trace_ao()'s."""
        suffix, lead, keep = self._spin(spin)
        res = self._trace_images(
            lambda W, H: self.ao_params(samples, colours, accumulate, distance, bias, origin, W, H, max_depth, stream),
            "sf_trace_ao" + suffix + "_sum", pos, out, np.float32, (4,), normals=True, nrm=nrm, accumulate=accumulate,
            lead=lead)
        del keep
        return res

    # sky reflections about each pixel's mirror direction (sf_trace_mirror_to / sf_trace_mirror_sum_to and their
    # context forms)
    def mirror_params(self, samples, colours=None, accumulate=False, distance=None, bias=None, origin=None, eye=None,
                      zenith=None, horizon=None, up=None, width=0, height=0, max_depth=0, stream=None):
        """sf_mirror_defaults, overridden: (params, keepalive). samples, colours, accumulate, distance, bias and origin
        as ao_params'; eye None: the view vector is the position itself (positions relative to the viewer), else the
        world point less `eye`; zenith, horizon, up None keep the library's defaults ((1, 1, 1), (1, 1, 1), (0, 0, 1))."""
        q, keep = self.ao_params(samples, colours, accumulate, distance, bias, origin, width, height, max_depth, stream)
        p = self._defaults(sf_mirror_params)
        for name, _ in sf_ao_params._fields_:   # (sf_ao_defaults' distance and bias are sf_mirror_defaults')
            setattr(p, name, getattr(q, name))
        if eye is not None:
            p.eye[:] = [float(x) for x in _f32(eye, 3)]
            p.use_eye = 1
        for field, v in (("zenith", zenith), ("horizon", horizon), ("up", up)):
            if v is not None:
                getattr(p, field)[:] = [float(x) for x in _f32(v, 3)]
        return p, keep

    def trace_mirror(self, samples, distance=4.0, bias=2.0 ** -10, pos=None, nrm=None, out=None, max_depth=0,
                     stream=None, origin=None, spin=None, eye=None):
        """trace_ao() about each pixel's MIRROR DIRECTION instead of its normal: the view vector V (the position itself,
        or with `eye` the world point less the eye) is mirrored about the normal on the device, A = normalise(V - 2 (N . V)
        N), and the `samples` [n, 3] -- a lobe about +z, sphereflake_amd.lights.lobe_samples -- are turned about A and
        traced as trace_ao() traces them: a uint64 per pixel, bit i = 1 where sample i's direction is open to the sky
        (sf_trace_mirror_to, sf.h; sphereflake_amd.lights.mirror_axes, mirror_model). pos, nrm, out, origin and spin as
        trace_ao()'s. The flake does not reflect itself: a closed direction is just closed."""
        lead, keep = self._mirror_spin(spin)
        res = self._trace_images(
            lambda W, H: self.mirror_params(samples, None, False, distance, bias, origin, eye, None, None, None, W, H,
                                            max_depth, stream),
            "sf_trace_mirror", pos, out, np.uint64, normals=True, nrm=nrm, lead=lead)
        del keep
        return res

    def trace_mirror_sum(self, samples, colours=None, zenith=(1.0, 1.0, 1.0), horizon=(1.0, 1.0, 1.0),
                         up=(0.0, 0.0, 1.0), accumulate=False, distance=4.0, bias=2.0 ** -10, pos=None, nrm=None,
                         out=None, max_depth=0, stream=None, origin=None, spin=None, eye=None):
        """trace_mirror() summed into a float4 light buffer: per surface pixel and channel, in index order,
        S += colour_i x (open_i ? E_i : 0) with E_i the sky's colour in the world direction s_i of THAT PIXEL'S ray:
        E_i = horizon + (zenith - horizon) clamp(s_i . up, 0, 1) (sf_trace_mirror_sum_to, sf.h;
        sphereflake_amd.lights.sky_gradient, mirror_sum_model). colours [n, 3] (None: 1 / n per component); accumulate,
        pos, nrm and out as trace_ao_sum()'s. Add it AFTER light_filter(): the mirror direction turns with the normal
        far faster than occlusion does. There is no Fresnel term, and light_image_buffer() still multiplies the image
        by the buffer."""
        lead, keep = self._mirror_spin(spin)
        res = self._trace_images(
            lambda W, H: self.mirror_params(samples, colours, accumulate, distance, bias, origin, eye, zenith, horizon,
                                            up, W, H, max_depth, stream),
            "sf_trace_mirror_sum", pos, out, np.float32, (4,), normals=True, nrm=nrm, accumulate=accumulate, lead=lead)
        del keep
        return res

    @classmethod
    def _mirror_spin(cls, spin):
        """(lead arguments, keepalive) of a trace_mirror call: the spin is always passed, None as a null pointer."""
        _, lead, keep = cls._spin(spin)
        return (lead if lead else (None,)), keep

    def light_filter_params(self, size=4, normal_min=None, plane_max=None, width=0, height=0, stream=None):
        """sf_light_filter_defaults, overridden; normal_min and plane_max None keep the library's defaults (0.9, 0.02)."""
        p = sf_light_filter_params()
        _check(lib().sf_light_filter_defaults(self._ctx, ctypes.byref(p)), "sf_light_filter_defaults")
        p.size = int(size)
        if normal_min is not None:
            p.normal_min = float(normal_min)
        if plane_max is not None:
            p.plane_max = float(plane_max)
        p.width, p.height, p.stream = int(width), int(height), stream
        return p

    def light_filter(self, size=4, normal_min=0.9, plane_max=0.02, pos=None, nrm=None, buf=None, out=None, stream=None):
        """The edge-aware size x size box filter of a light buffer (sf_light_filter_to; sf.h,
        sphereflake_amd.lights.light_filter_model): each surface pixel becomes the mean of the pixels of its window that
        lie on its own surface -- normals within normal_min of its own, positions within plane_max |P| of its tangent
        plane -- so the size x size block of a spun trace_ao_sum(spin=lights.ao_spins(size)) is gathered back without
        bleeding over edges. Misses are copied; .w is carried.
          - pos None: the context's own G-buffer and light buffer, filtered in place (the address light_buffer()
            returns does not change) or, with `out` (and optionally a device `buf`), into that buffer -- asynchronous;
          - pos, nrm, buf numpy arrays [H, W, 4]: uploaded, filtered, and a numpy [H, W, 4] float32 returned --
            synchronous;
          - pos, nrm, buf torch CUDA tensors [H, W, 4] (contiguous float32) or (device address, width, height) tuples:
            zero copy, asynchronous; `out` a torch CUDA tensor [H, W, 4] or a device address, not `buf`."""
        return self._trace_images(lambda W, H: self.light_filter_params(size, normal_min, plane_max, W, H, stream),
                                  "sf_light_filter", pos, out, np.float32, (4,), normals=True, nrm=nrm, buf=buf,
                                  has_buf=True)

    # the light buffer over several frames (sf_light_accumulate_to / sf_light_accumulate / sf_light_history_reset) ------
    def light_accumulate_params(self, max_history=16, normal_min=None, plane_max=None, origin=None, hist_view=None,
                                width=0, height=0, stream=None):
        """sf_light_accumulate_defaults, overridden; normal_min and plane_max None keep the library's defaults
        (0.9, 0.02). hist_view: the history's view (origin, top-left, top-right, bottom-left), 12 floats -- its origin
        becomes hist_origin and its reproject_matrix() hist_m; None leaves both zero (the context form ignores them)."""
        p = sf_light_accumulate_params()
        _check(lib().sf_light_accumulate_defaults(self._ctx, ctypes.byref(p)), "sf_light_accumulate_defaults")
        p.max_history = int(max_history)
        if normal_min is not None:
            p.normal_min = float(normal_min)
        if plane_max is not None:
            p.plane_max = float(plane_max)
        if origin is not None:
            p.origin[:] = [float(x) for x in _f32(origin, 3)]
            p.use_origin = 1
        if hist_view is not None:
            v = _f32(np.concatenate([np.asarray(x, np.float32).reshape(-1) for x in hist_view]), 12)
            p.hist_origin[:] = [float(x) for x in v[:3]]
            p.hist_m[:] = [float(x) for x in reproject_matrix(v)]
        p.width, p.height, p.stream = int(width), int(height), stream
        return p

    def light_accumulate(self, max_history=16, normal_min=0.9, plane_max=0.02, pos=None, nrm=None, buf=None,
                         hist_pos=None, hist_nrm=None, hist=None, hist_view=None, out=None, origin=None, stream=None):
        """Blend a light buffer into the last frame's, reprojected (sf_light_accumulate_to; sf.h,
        sphereflake_amd.lights.light_accumulate_model): each surface pixel's world point is taken back through
        `hist_view` to the pixel of the history it falls in; where that pixel lies on the same surface -- normals within
        normal_min, positions within plane_max |P| of the tangent plane, a history count .w >= 1 -- the result is
        h + (new - h) / min(h.w + 1, max_history) with that as its .w, else the new value with .w = 1. A miss of the
        frame keeps the new value with .w = 0.
          - no images: the context form (sf_light_accumulate). The context's G-buffer, light buffer and current view
            against the history the context keeps, in place (the address light_buffer() returns does not change); the
            frame then becomes the history of the next call -- asynchronous;
          - pos, nrm, buf, hist_pos, hist_nrm, hist numpy arrays [H, W, 4]: uploaded, accumulated, and a numpy
            [H, W, 4] float32 returned -- synchronous;
          - the six torch CUDA tensors [H, W, 4] (contiguous float32), (device address, width, height) tuples or, after
            `pos`, plain device addresses: zero copy, asynchronous; `out` a torch CUDA tensor [H, W, 4] or a device
            address, none of the inputs.
        hist_view is the history's (origin, top-left, top-right, bottom-left); `origin` is what pos is relative to (None:
        the context's view origin)."""
        images = (pos, nrm, buf, hist_pos, hist_nrm, hist)
        names = ("pos", "nrm", "buf", "hist_pos", "hist_nrm", "hist")
        if all(a is None for a in images):
            if out is not None or hist_view is not None:
                raise ValueError("the context form takes no images, no hist_view and no out")
            p = self.light_accumulate_params(max_history, normal_min, plane_max, None, None, 0, 0, stream)
            with self._mutex:
                _check(lib().sf_light_accumulate(self._ctx, ctypes.byref(p)), "sf_light_accumulate", self._ctx)
            return None
        if any(a is None for a in images) or hist_view is None:
            raise ValueError("pos, nrm, buf, hist_pos, hist_nrm, hist and hist_view go together")
        vp = lambda x: ctypes.c_void_p(x) if x else None
        if isinstance(pos, np.ndarray):
            if not all(isinstance(a, np.ndarray) for a in images):
                raise ValueError("a host position image needs host images throughout")
            if out is not None:
                raise ValueError("host images return a host array: out must be None")
            host = [np.ascontiguousarray(a, np.float32) for a in images]
            if host[0].ndim != 3 or host[0].shape[-1] != 4 or any(a.shape != host[0].shape for a in host):
                raise ValueError("the six images must be [H, W, 4] of one size")
            H, W = host[0].shape[:2]
            p = self.light_accumulate_params(max_history, normal_min, plane_max, origin, hist_view, W, H, stream)
            res = np.empty((H, W, 4), np.float32)
            if H * W == 0:
                return res
            offs = [k * res.nbytes for k in range(7)]   # the images, then the result
            with _DeviceScratch(self.device, 7 * res.nbytes) as d:
                for a, off in zip(host, offs):
                    d.upload(off, a)
                with self._mutex:
                    _check(lib().sf_light_accumulate_to(self._ctx, ctypes.byref(p), *[vp(d.ptr + off) for off in offs]),
                           "sf_light_accumulate_to", self._ctx)
                    # (the scratch is freed on leaving: the pass that reads and writes it must be done)
                    _check(lib().sf_synchronize(self._ctx), "sf_synchronize", self._ctx)
                d.download(offs[-1], res)
            return res
        if any(isinstance(a, np.ndarray) for a in images):
            raise ValueError("a device position image needs device images throughout")
        pptr, W, H = self._image4(pos, "pos")
        ptrs = [pptr]
        for a, what in zip(images[1:], names[1:]):
            if hasattr(a, "data_ptr") or isinstance(a, (tuple, list)):
                ptr, w, h = self._image4(a, what)
                if (w, h) != (W, H):
                    raise ValueError(f"{what} and pos must have the same size")
                ptrs.append(ptr)
            else:
                ptrs.append(int(a))
        optr = 0 if out is None else out.data_ptr() if hasattr(out, "data_ptr") else int(out)
        if not optr:
            raise ValueError("device images need an `out` buffer")
        p = self.light_accumulate_params(max_history, normal_min, plane_max, origin, hist_view, W, H, stream)
        with self._mutex:
            _check(lib().sf_light_accumulate_to(self._ctx, ctypes.byref(p), *[vp(x) for x in ptrs], vp(optr)),
                   "sf_light_accumulate_to", self._ctx)
        return None

    def light_history_reset(self):
        """Forget the context form's history: the next light_accumulate() is a first call (sf_light_history_reset)."""
        with self._mutex:
            _check(lib().sf_light_history_reset(self._ctx), "sf_light_history_reset", self._ctx)

    def Synchronize(self):
        _check(lib().sf_synchronize(self._ctx), "sf_synchronize", self._ctx)

    def unpack_bands(self, stage_ptr: int, stage_rows: int, band_rows: int, band_count: int, first_member: int,
                     members: int, stream=None):
        """Packed band slabs on the device (render_to(..., packed=True, compact=True) of members first_member..)
        -> this context's G-buffer at frame positions (sf_unpack_bands), with the current view."""
        _check(lib().sf_unpack_bands(self._ctx, ctypes.c_void_p(stage_ptr), stage_rows, band_rows, band_count,
                                     first_member, members, stream), "sf_unpack_bands", self._ctx)

    def unpack_slabs(self, stage_ptr: int, bytes_per_pixel: int, stage_rows: int, band_rows: int, band_count: int,
                     first_member: int, members: int, stream=None):
        """Band slabs of either format (bytes_per_pixel 16: packed=1, 4: packed=2) -> this context's G-buffer
        (sf_unpack_slabs), with the current view."""
        _check(lib().sf_unpack_slabs(self._ctx, ctypes.c_void_p(stage_ptr), bytes_per_pixel, stage_rows, band_rows,
                                     band_count, first_member, members, stream), "sf_unpack_slabs", self._ctx)

    def slab_bytes(self) -> int:
        """Bytes per pixel of the smallest lossless band slab for the current view (sf_slab_bytes: 4 or 16)."""
        return int(lib().sf_slab_bytes(self._ctx))

    def device_buffers(self):
        ptrs = [ctypes.c_void_p() for _ in range(4)]
        _check(lib().sf_device_buffers(self._ctx, *[ctypes.byref(p) for p in ptrs]), "sf_device_buffers")
        return [p.value for p in ptrs]

    def download(self, aux: bool = False):
        """Synchronous D2H of the device G-buffer (+ minT and hit index channels if aux)."""
        H, W = self.height, self.width
        pos = np.empty((H, W, 4), np.float32)
        nrm = np.empty((H, W, 4), np.float32)
        mint = np.empty((H, W), np.float32) if aux else None
        idx = np.empty((H, W), np.uint32) if aux else None
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None
        self._raise_worker_error()
        with self._mutex:
            _check(lib().sf_download(self._ctx, vp(pos), vp(nrm), vp(mint), vp(idx)), "download", self._ctx)
        return pos, nrm, mint, idx

    def GetGBuffer(self) -> GBuffer:
        pos, nrm, _, _ = self.download()
        return GBuffer(pos, nrm)

    # reference variant ---------------------------------
    def SetVariant(self, variant):
        """'avx' / SF_VARIANT_AVX (default: LOD 70, 8-lane packets) or 'sse' / SF_VARIANT_SSE (LOD 60,
        4-lane packets, 2x2 frame-less footprint): the reference built without / with __ARCH_NO_AVX."""
        v = {"avx": SF_VARIANT_AVX, "sse": SF_VARIANT_SSE}.get(variant, variant)
        with self._mutex:
            _check(lib().sf_set_variant(self._ctx, int(v)), "SetVariant", self._ctx)

    def GetVariant(self) -> int:
        return lib().sf_get_variant(self._ctx)

    # transfer/interop ------------------------------------
    def pinned_gbuffer(self) -> GBuffer:
        """Host G-buffer arrays in the reference layout, page-locked for DMA (sf_host_register).
        Pass them to download_async; release with release_pinned()."""
        H, W = self.height, self.width
        g = GBuffer(np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32))
        for a in (g.positions, g.normals):
            _check(lib().sf_host_register(a.ctypes.data_as(ctypes.c_void_p), a.nbytes), "sf_host_register")
        self._pinned = getattr(self, "_pinned", []) + [g.positions, g.normals]
        return g

    def release_pinned(self):
        for a in getattr(self, "_pinned", []):
            lib().sf_host_unregister(a.ctypes.data_as(ctypes.c_void_p))
        self._pinned = []

    def download_async(self, g: GBuffer, stream: int | None = None):
        """Stream-ordered D2H of the G-buffer into `g` (pinned arrays from pinned_gbuffer());
        complete after Synchronize() (or the given stream's synchronisation)."""
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        with self._mutex:
            _check(lib().sf_download_async(self._ctx, vp(g.positions), vp(g.normals), None, None,
                                           ctypes.c_void_p(stream) if stream else None), "download_async", self._ctx)

    # SSAO post-process -----------------------------------
    def post_params(self, **kw) -> sf_post_params:
        """Reference defaults (SSAO.cpp:50-55, radius from the closest-hit stat, camera = view origin),
        overridden by keyword (sample_radius, intensity, scale, bias, normal_threshold, depth_threshold,
        camera_position, downscale, flags, stream)."""
        p = sf_post_params()
        _check(lib().sf_post_defaults(self._ctx, ctypes.byref(p)), "sf_post_defaults")
        for k, v in kw.items():
            if k == "camera_position":
                p.camera_position[:] = [float(x) for x in _f32(v, 3)]
            elif k == "stream":
                p.stream = v
            else:
                setattr(p, k, v)
        return p

    def PostProcess(self, pos_ptr: int = 0, nrm_ptr: int = 0, rgba_ptr: int = 0, ao_ptr: int = 0, **kw):
        """SSAO + blur x + blur y + final composite on the device (asynchronous). Pointers are device
        addresses (0 = the context's G-buffer / image buffer); ao_ptr receives the SSAO target."""
        p = self.post_params(**kw)
        vp = lambda x: ctypes.c_void_p(x) if x else None
        with self._mutex:
            _check(lib().sf_post_process(self._ctx, ctypes.byref(p), vp(pos_ptr), vp(nrm_ptr), vp(rgba_ptr),
                                         vp(ao_ptr)), "sf_post_process", self._ctx)

    def download_image(self) -> np.ndarray:
        """[H, W, 4] uint8 RGBA of the last PostProcess into the context image buffer."""
        img = np.empty((self.height, self.width, 4), np.uint8)
        with self._mutex:
            _check(lib().sf_download_image(self._ctx, img.ctypes.data_as(ctypes.c_void_p)), "sf_download_image",
                   self._ctx)
        return img

    @staticmethod
    def ssao_noise() -> np.ndarray:
        out = np.empty((64 * 64, 4), np.float32)
        _check(lib().sf_ssao_noise(_fp(out)), "sf_ssao_noise")
        return out

    def save_image(self, path: str, what: int = SF_DUMP_NORMALS) -> None:
        """Download this context's frame and write it as SF_DUMP_* (PPM of the post-processed image or
        of the normals, PFM of positions / normals) through the C ABI's sf_save_image."""
        with self._mutex:
            _check(lib().sf_save_image(self._ctx, os.fsencode(path), int(what)), "sf_save_image", self._ctx)

    @staticmethod
    def save_ppm(path: str, rgb) -> None:
        """Write an [H, W, 3] float image (0..1, clamped) as a binary PPM (8-bit), y = 0 on top."""
        a = np.clip(np.asarray(rgb, np.float32), 0.0, 1.0)
        b = (a * 255.0 + 0.5).astype(np.uint8)
        with open(path, "wb") as f:
            f.write(f"P6 {b.shape[1]} {b.shape[0]} 255\n".encode())
            f.write(np.ascontiguousarray(b[:, :, :3]).tobytes())

    def tile_trace(self, enable: bool | None = None):
        """Diagnostics: enable per-tile timing, or (enable=None) fetch [tiles, 3] uint64
        (start, end in 100 MHz ticks, (xcc << 32) | HW_ID) of the last render."""
        if enable is not None:
            _check(lib().sf_set_tile_trace(self._ctx, int(bool(enable))), "sf_set_tile_trace", self._ctx)
            return None
        n = ((self.width + 7) // 8) * ((self.height + 7) // 8)
        # tiles, SF_DIAG_SLOTS, units and waves (SF_FLAG_DIAG_UNITS): SF_TRACE_WORDS (sf_internal.h)
        out = np.zeros(15 * n + 16 + 2 * SF_DIAG_WAVES, np.uint64)
        _check(lib().sf_get_tile_trace(self._ctx, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), out.size),
               "sf_get_tile_trace", self._ctx)
        self.phase_sums = out[3 * n:3 * n + 16]   # segment cycle sums / event counts of diagnostic builds
        self.unit_trace = out[3 * n + 16:15 * n + 16].reshape(4 * n, 3)   # per order position (SF_FLAG_DIAG_UNITS)
        self.wave_trace = out[15 * n + 16:].reshape(SF_DIAG_WAVES, 2)   # per wave {start, end} (SF_FLAG_DIAG_UNITS)
        return out[:3 * n].reshape(n, 3)

    def tile_order(self):
        """Heavy-first schedule: (units, cost) uint32 arrays -- the work units (tile | part << 29; where the renders
        take pair units, pair_launches(), the pair index and no parts) the next persistent render takes in order, and
        the last render's per-unit shader cycles they were computed from -- or None before any ordered render."""
        n = ((self.width + 7) // 8) * ((self.height + 7) // 8)
        order = np.zeros(4 * n, np.uint32)
        cost = np.zeros(n, np.uint32)
        P = ctypes.POINTER(ctypes.c_uint32)
        k = lib().sf_get_tile_order(self._ctx, order.ctypes.data_as(P), cost.ctypes.data_as(P), 4 * n)
        if k < 0:
            _check(k, "sf_get_tile_order", self._ctx)
        return (order[:k], cost[:int(lib().sf_order_units(self._ctx))]) if k else None

    def kernel_timing(self, enable: bool | None = None, n: int = 64, period: int = 1):
        """Measurement: enable HIP events around the main trace kernel of every `period`-th render, or
        (enable=None) return the durations (ms) of the last n timed renders, oldest first."""
        if enable is not None:
            k = max(1, int(period)) if enable else 0
            _check(lib().sf_set_kernel_timing(self._ctx, k), "sf_set_kernel_timing", self._ctx)
            return None
        out = np.zeros(n, np.float32)
        k = lib().sf_kernel_times(self._ctx, out.ctypes.data_as(_F), n)
        if k < 0:
            _check(k, "sf_kernel_times", self._ctx)
        return out[:k]

    def kernel_clocks(self, n: int = 64):
        """Live shader clock (MHz) of the last n timed renders' trace kernels, oldest first (sf_kernel_clocks)."""
        out = np.zeros(n, np.float32)
        k = lib().sf_kernel_clocks(self._ctx, out.ctypes.data_as(_F), n)
        if k < 0:
            _check(k, "sf_kernel_clocks", self._ctx)
        return out[:k]

    # stats (Sphereflake.h:30-58) --------------------------------------------
    def stats(self) -> sf_stats:
        self._raise_worker_error()
        s = sf_stats()
        with self._mutex:
            _check(lib().sf_get_stats(self._ctx, ctypes.byref(s)), "sf_get_stats", self._ctx)
        return s

    def lean_launches(self) -> int:
        """Trace launches of this context that took the lean tile loop (sf_lean_launches)."""
        return int(lib().sf_lean_launches(self._ctx))

    def pair_launches(self) -> int:
        """Those of them that took the pair-unit loop, two adjacent tiles per wave (sf_pair_launches)."""
        return int(lib().sf_pair_launches(self._ctx))

    def GetMaxDepthReached(self) -> int:
        return int(self.stats().max_depth)

    def ResetMaxDepthReached(self):
        _check(lib().sf_reset_max_depth(self._ctx), "ResetMaxDepthReached")

    def GetRaysPerSecond(self) -> int:
        """Rays traced since the last reset (the reference counter's meaning, main.cpp:285-291)."""
        return int(self.stats().rays)

    def ResetRaysPerSecond(self):
        _check(lib().sf_reset_rays(self._ctx), "ResetRaysPerSecond")

    def GetClosestSphereDistance(self) -> float:
        return float(self.stats().closest)

    def ResetClosestSphereDistance(self):
        _check(lib().sf_reset_closest(self._ctx), "ResetClosestSphereDistance")

    def reset_stats(self):
        """All three reference counters at once (ResetMaxDepthReached, ResetClosestSphereDistance,
        ResetRaysPerSecond)."""
        self.ResetMaxDepthReached()
        self.ResetClosestSphereDistance()
        self.ResetRaysPerSecond()

    # frame-less progressive mode (Sphereflake.cpp:67-74, 86-214) -------------
    def Progressive(self, seed: int, packets: int, counter0: int | None = None, stream=None):
        """Trace `packets` random 8-ray packets of one reference worker stream (seed, Sobol counter)."""
        c0 = self._counter if counter0 is None else int(counter0)
        with self._mutex:
            _check(lib().sf_progressive(self._ctx, seed & 0xffffffff, c0, packets, stream), "sf_progressive",
                   self._ctx)
        self._counter = c0 + packets

    def Initialize(self, seed: int | None = None, batch: int = 1 << 18):
        """Start the frame-less progressive loop on a host thread (reference Initialize(),
        Sphereflake.cpp:67-74; seeded from time() like Sphereflake.cpp:88-89 unless `seed` is given).
        The loop's first error stops it and is re-raised by the next GetGBuffer / stats call /
        Deinitialize."""
        import time
        if self._worker is not None:
            return
        self._raise_worker_error()
        self._seed = int(time.time()) if seed is None else int(seed)
        self._counter = 0
        self._stop.clear()

        def loop():
            try:
                while not self._stop.is_set():
                    with self._mutex:
                        _check(lib().sf_progressive(self._ctx, self._seed & 0xffffffff, self._counter, batch, None),
                               "sf_progressive", self._ctx)
                        _check(lib().sf_synchronize(self._ctx), "sf_synchronize", self._ctx)
                        self._counter += batch
            except Exception as e:   # kept for the caller's thread
                self._worker_error = e

        self._worker = threading.Thread(target=loop, daemon=True)
        self._worker.start()

    def Deinitialize(self):
        """Stop the frame-less loop and join it (the reference does this in its destructor)."""
        self._stop.set()
        if self._worker is not None:
            self._worker.join()
            self._worker = None
        self._raise_worker_error()

    def GetPacketsTraced(self) -> int:
        with self._mutex:
            return self._counter

    def _raise_worker_error(self):
        e, self._worker_error = getattr(self, "_worker_error", None), None
        if e is not None:
            raise RuntimeError(f"frame-less loop failed: {e}") from e


class SphereflakeGroup:
    """Single-process multi-GPU renderer (sf_group_*): interleaved 8-row bands traced on
    the member devices, gathered by strided peer copies into member 0's G-buffer. `devices` may repeat a
    device (n contexts on one GPU)."""

    def __init__(self, devices, width: int, height: int):
        self.width, self.height = int(width), int(height)
        devs = (ctypes.c_int * len(devices))(*[int(d) for d in devices])
        h = ctypes.c_void_p()
        _check(lib().sf_group_create(devs, len(devices), self.width, self.height, ctypes.byref(h)), "sf_group_create")
        self._g = h

    def close(self):
        if getattr(self, "_g", None):
            lib().sf_group_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc, what):
        if rc != SF_OK:
            err = SphereflakeError(rc, what)
            if rc == SF_EHIP:
                err.hip_error = lib().sf_group_last_hip_error(self._g)
            raise err

    def size(self) -> int:
        return lib().sf_group_size(self._g)

    def member(self, k: int):
        """Member k's context handle (k = 0 holds the final G-buffer)."""
        return lib().sf_group_member(self._g, k)

    def SetView(self, origin, topLeft, topRight, bottomLeft):
        o, tl, tr, bl = (_vec3(v) for v in (origin, topLeft, topRight, bottomLeft))
        self._check(lib().sf_group_set_view(self._g, o, tl, tr, bl), "sf_group_set_view")

    def SetCamera(self, cam: Camera):
        self.SetView(*cam.corners())

    def SetVariant(self, variant):
        v = {"avx": SF_VARIANT_AVX, "sse": SF_VARIANT_SSE}.get(variant, variant)
        self._check(lib().sf_group_set_variant(self._g, int(v)), "sf_group_set_variant")

    def Render(self, band_rows: int = 8):
        self._check(lib().sf_group_render(self._g, int(band_rows)), "sf_group_render")

    def Synchronize(self):
        self._check(lib().sf_group_synchronize(self._g), "sf_group_synchronize")

    def download(self):
        H, W = self.height, self.width
        pos = np.empty((H, W, 4), np.float32)
        nrm = np.empty((H, W, 4), np.float32)
        self._check(lib().sf_group_download(self._g, pos.ctypes.data_as(ctypes.c_void_p),
                                            nrm.ctypes.data_as(ctypes.c_void_p)), "sf_group_download")
        return pos, nrm

    def member_kernel_timing(self, k: int, enable: bool | None = None, n: int = 64, period: int = 1):
        """Sphereflake.kernel_timing on member k's context (its main trace kernel)."""
        ctx = self.member(k)
        if enable is not None:
            _check(lib().sf_set_kernel_timing(ctx, max(1, int(period)) if enable else 0), "sf_set_kernel_timing", ctx)
            return None
        out = np.zeros(n, np.float32)
        got = lib().sf_kernel_times(ctx, out.ctypes.data_as(_F), n)
        if got < 0:
            _check(got, "sf_kernel_times", ctx)
        return out[:got]

    def reset_stats(self):
        self._check(lib().sf_group_reset_stats(self._g), "sf_group_reset_stats")

    def stats(self) -> sf_stats:
        """Over the members: max depth, closest distance, rays summed (accumulating across renders
        like the reference's counters until reset_stats)."""
        s = sf_stats()
        self._check(lib().sf_group_get_stats(self._g, ctypes.byref(s)), "sf_group_get_stats")
        return s

    def slab_bytes(self) -> int:
        """Bytes per pixel a member ships for the current view (4: hit index, 16: normal + minT)."""
        return int(lib().sf_group_slab_bytes(self._g))


def dist_unique_id() -> bytes:
    """A fresh RCCL unique id (sf_dist_unique_id): rank 0 makes one per slot and hands them to every rank."""
    buf = (ctypes.c_uint8 * SF_DIST_ID_BYTES)()
    _check(lib().sf_dist_unique_id(buf), "sf_dist_unique_id")
    return bytes(buf)


class SphereflakeDist:
    """One process per GPU (sf_dist_*): this rank's share of every frame (interleaved
    `band_rows`-row bands), gathered to rank 0 over RCCL as packed slabs; `slots` frames in flight. `ids`:
    slots x 128 bytes of dist_unique_id() from rank 0, or None: no communicator (nranks = 1, or this rank's bands
    of a distributed G-buffer via RenderBands only -- Render then raises SF_ESTATE)."""

    def __init__(self, device: int, width: int, height: int, rank: int = 0, nranks: int = 1, slots: int = 2,
                 ids: bytes | None = None, band_rows: int = 8):
        self.width, self.height, self.rank, self.nranks = int(width), int(height), int(rank), int(nranks)
        h = ctypes.c_void_p()
        idb = None
        if ids is not None:
            if len(ids) != slots * SF_DIST_ID_BYTES:
                raise ValueError("ids must hold slots x 128 bytes")
            idb = ctypes.create_string_buffer(bytes(ids), len(ids))
        _check(lib().sf_dist_create(int(device), self.width, self.height, int(band_rows), self.rank, self.nranks,
                                    int(slots), idb, ctypes.byref(h)), "sf_dist_create")
        self._d = h

    def close(self):
        if getattr(self, "_d", None):
            lib().sf_dist_destroy(self._d)
            self._d = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc, what):
        if rc != SF_OK:
            err = SphereflakeError(rc, what)
            hip, nccl = ctypes.c_int(), ctypes.c_int()
            lib().sf_dist_last_error(self._d, ctypes.byref(hip), ctypes.byref(nccl))
            err.hip_error, err.rccl_error = hip.value, nccl.value
            raise err

    @property
    def slots(self) -> int:
        return lib().sf_dist_slots(self._d)

    def context(self, slot: int):
        return lib().sf_dist_context(self._d, int(slot))

    def last_slot(self) -> int:
        return lib().sf_dist_last_slot(self._d)

    def SetView(self, origin, topLeft, topRight, bottomLeft):
        o, tl, tr, bl = (_vec3(v) for v in (origin, topLeft, topRight, bottomLeft))
        self._check(lib().sf_dist_set_view(self._d, o, tl, tr, bl), "sf_dist_set_view")

    def SetCamera(self, cam: Camera):
        self.SetView(*cam.corners())

    def Render(self):
        """One frame: this rank's bands, gathered with the other ranks' into rank 0's G-buffer (RCCL)."""
        self._check(lib().sf_dist_render(self._d), "sf_dist_render")

    def RenderBands(self):
        """One frame as a distributed G-buffer: this rank's bands into its own slot G-buffer, no gather."""
        self._check(lib().sf_dist_render_bands(self._d), "sf_dist_render_bands")

    def RenderBandsFrames(self, views):
        """The next len(views) frames (each (origin, top-left, top-right, bottom-left)) as RenderBands would render
        them one by one, in ONE multi-frame persistent launch (sf_dist_render_bands_frames; len(views) <= slots)."""
        v = _views12(views)
        self._check(lib().sf_dist_render_bands_frames(self._d, len(views), _fp(v)), "sf_dist_render_bands_frames")

    def download_slot(self, slot: int):
        """The G-buffer of one slot's context on this rank (synchronises)."""
        H, W = self.height, self.width
        pos = np.empty((H, W, 4), np.float32)
        nrm = np.empty((H, W, 4), np.float32)
        ctx = self.context(slot)
        _check(lib().sf_download(ctx, pos.ctypes.data_as(ctypes.c_void_p), nrm.ctypes.data_as(ctypes.c_void_p),
                                 None, None), "sf_download", ctx)
        return pos, nrm

    def Synchronize(self):
        self._check(lib().sf_dist_synchronize(self._d), "sf_dist_synchronize")

    def download(self):
        """Rank 0: the last frame's G-buffer (synchronises)."""
        H, W = self.height, self.width
        pos = np.empty((H, W, 4), np.float32)
        nrm = np.empty((H, W, 4), np.float32)
        self._check(lib().sf_dist_download(self._d, pos.ctypes.data_as(ctypes.c_void_p),
                                           nrm.ctypes.data_as(ctypes.c_void_p)), "sf_dist_download")
        return pos, nrm

    def stats(self) -> sf_stats:
        """Over this rank's slots, and over the ranks when made with ids (then collective: every rank calls it);
        without ids the caller combines the ranks' stats."""
        s = sf_stats()
        self._check(lib().sf_dist_get_stats(self._d, ctypes.byref(s)), "sf_dist_get_stats")
        return s

    def reset_stats(self):
        self._check(lib().sf_dist_reset_stats(self._d), "sf_dist_reset_stats")

    def kernel_timing(self, slot: int, enable: bool | None = None, n: int = 64, period: int = 1):
        """Trace-kernel events of one slot's context (Sphereflake.kernel_timing)."""
        ctx = self.context(slot)
        if enable is not None:
            _check(lib().sf_set_kernel_timing(ctx, max(1, int(period)) if enable else 0), "sf_set_kernel_timing", ctx)
            return None
        out = np.zeros(n, np.float32)
        got = lib().sf_kernel_times(ctx, out.ctypes.data_as(_F), n)
        if got < 0:
            _check(got, "sf_kernel_times", ctx)
        return out[:got]

    def comm_info(self, slot: int = 0):
        """(ncclCommCount, ncclCommUserRank, ncclCommCuDevice) of a slot's RCCL communicator (sf_dist_comm_info)."""
        v = [ctypes.c_int() for _ in range(3)]
        self._check(lib().sf_dist_comm_info(self._d, int(slot), *[ctypes.byref(x) for x in v]), "sf_dist_comm_info")
        return tuple(x.value for x in v)

    def slab_bytes(self) -> int:
        """Bytes per pixel the gather ships for the current view (4: hit index, 16: normal + minT)."""
        return int(lib().sf_dist_slab_bytes(self._d))

    def kernel_clocks(self, slot: int, n: int = 64):
        ctx = self.context(slot)
        out = np.zeros(n, np.float32)
        got = lib().sf_kernel_clocks(ctx, out.ctypes.data_as(_F), n)
        if got < 0:
            _check(got, "sf_kernel_clocks", ctx)
        return out[:got]
