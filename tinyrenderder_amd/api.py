"""Python host mirror of the C ABI in include/trgl.h (ctypes over tinyrenderder_amd/libtrgl.so).

This is the product path: it never falls back to a CPU implementation.  If the HIP library is
missing or a call fails, it raises.
"""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libtrgl.so")

FLAT, GOURAUD, PHONG, EYE, CHECKER = 0, 1, 2, 3, 4
VARY = {FLAT: 0, GOURAUD: 3, PHONG: 24, EYE: 24, CHECKER: 0}
SHADER_USER_FIRST, MAX_USER_SHADERS, MAX_USER_VARY = 64, 32, 64      # user shaders: kinds handed out by Context.register_shader
SHADER_MAY_DISCARD = 1        # TRGL_SHADER_MAY_DISCARD: the user shader's trgl_fragment returns trgl_frag_out (it can discard)
SHADER_READS_DEST = 4         # TRGL_SHADER_READS_DEST: in.dst is the pixel the fragment is drawn over (with MAY_DISCARD only)
SHADER_NO_DEPTH_WRITE = 8     # TRGL_SHADER_NO_DEPTH_WRITE: a drawn fragment leaves the depth alone (with MAY_DISCARD only)


def shader_flags(may_discard=False, reads_dest=False, depth_write=True) -> int:
    """The flag word of trgl_shader_compile_ex / trgl_register_shader_ex; which words are valid is the library's decision."""
    return ((SHADER_MAY_DISCARD if may_discard else 0) | (SHADER_READS_DEST if reads_dest else 0)
            | (0 if depth_write else SHADER_NO_DEPTH_WRITE))
MAX_USER_VERTEX_SHADERS = 32  # TRGL_MAX_USER_VERTEX_SHADERS: vertex shaders handed out by Context.register_vertex_shader, from 0
MEM_HOST, MEM_DEVICE = 0, 1
PHASE_SETUP, PHASE_BIN, PHASE_RASTER, PHASE_TOTAL, PHASE_RASTER_KERNEL = 0, 1, 2, 3, 4
NUM_PHASES = 5        # TRGL_NUM_PHASES
MAX_TEXTURES = 16
MAX_Z_SNAPSHOTS = 4           # TRGL_MAX_Z_SNAPSHOTS
MAX_BLUR_RADIUS = 46340       # TRGL_MAX_BLUR_RADIUS
MAX_PCF_RADIUS = 4            # TRGL_MAX_PCF_RADIUS
MAX_CLIP_ATTRS = 24           # TRGL_MAX_CLIP_ATTRS
OCCL_HIDDEN, OCCL_VISIBLE, OCCL_OUTSIDE, OCCL_UNDECIDED = range(4)     # TRGL_OCCL_*: bit 0 set = draw it
# the sizes of the instanced stages (csrc/launch.h): instances per block of the compaction, block counts per block of its scan's lower
# level, output faces per block of the instanced vertex kernels
INST_BLOCK, INST_SCAN_CHUNK, INST_VS_FACES = 256, 256, 64
ORDER_BACK_TO_FRONT, ORDER_FRONT_TO_BACK = 0, 1     # TRGL_ORDER_*
TRI_DEPTH_CENTROID, TRI_DEPTH_NEAREST, TRI_DEPTH_FARTHEST = 0, 1, 2     # TRGL_TRI_DEPTH_*
CENTROID, NEAREST, FARTHEST = TRI_DEPTH_CENTROID, TRI_DEPTH_NEAREST, TRI_DEPTH_FARTHEST
SKIN_NORMAL, SKIN_TANGENT, SKIN_BITANGENT = 1, 2, 4     # TRGL_SKIN_*: the directions of a vertex record that trgl_skin_stage transforms
EDGE_ANY, EDGE_BOUNDARY, EDGE_SILHOUETTE, EDGE_CREASE = 1, 2, 4, 8     # TRGL_EDGE_*: the class bits of an edge's code byte
EDGE_NONE = 0xFFFFFFFF        # every word of a "no edge" record, f1 of a boundary edge, both words of a "no edge" segment
SUBDIV_LINEAR, SUBDIV_LOOP = 0, 1   # TRGL_SUBDIV_*: the modes of subdiv_vertices
SUBDIV_BLOCK, SUBDIV_ITEMS = 256, 4   # lanes per block of the subdivision kernels and doubles per lane of the vertex kernel (csrc/launch.h)
EDGE_BLOCK = 256              # records per block of the edge kernels (csrc/launch.h); their scan has the levels of INST_SCAN_CHUNK
SPRITE_VIEW, SPRITE_SCREEN = 0, 1     # TRGL_SPRITE_*: a sprite's size in eye-space units, or in units of the caller's scale[]
FRUSTUM_SET, FRUSTUM_MERGE = 0, 1     # TRGL_FRUSTUM_*: the mode of trgl_frustum_boxes
NEAR_PLANE = (0.0, 0.0, 1.0, 1.0)     # the near plane of the reference's projection in clip space: z + w >= 0
FRUSTUM_LEFT, FRUSTUM_RIGHT, FRUSTUM_BOTTOM, FRUSTUM_TOP, FRUSTUM_NEAR, FRUSTUM_FAR = range(6)   # Frustum::PlaneIndex (our_gl.h:71-78)

# every symbol include/trgl.h declares (tests check the library exports all of them)
SYMBOLS = [
    "trgl_create", "trgl_destroy", "trgl_last_error", "trgl_set_viewport", "trgl_init_viewport", "trgl_clear",
    "trgl_upload_texture", "trgl_set_strip", "trgl_set_interleave", "trgl_draw", "trgl_flush", "trgl_flush_begin", "trgl_flush_end", "trgl_sync", "trgl_read_framebuffer",
    "trgl_write_framebuffer", "trgl_read_zbuffer", "trgl_write_zbuffer", "trgl_get_stats", "trgl_reset_stats",
    "trgl_format_stats", "trgl_framebuffer_device_ptr", "trgl_zbuffer_device_ptr", "trgl_stream", "trgl_set_stream",
    "trgl_set_profiling", "trgl_get_phase_ms", "trgl_reset_phase_ms", "trgl_get_last_flush_info",
    "trgl_selftest_division", "trgl_selftest_sampler", "trgl_tga_max_size", "trgl_tga_encode", "trgl_tga_info", "trgl_tga_decode", "trgl_draw_indexed", "trgl_ssao_defaults",
    "trgl_postprocess", "trgl_obj_load", "trgl_obj_free",
    "trgl_gather", "trgl_rccl_unique_id", "trgl_rccl_comm_create", "trgl_rccl_comm_destroy",
    "trgl_shader_compile", "trgl_register_shader", "trgl_shader_compile_ex", "trgl_register_shader_ex",
    "trgl_vertex_shader_compile", "trgl_register_vertex_shader", "trgl_draw_indexed_vs", "trgl_vertex_stage",
    "trgl_mesh_bounds", "trgl_aabb_transform", "trgl_frustum_from_matrix", "trgl_frustum_intersects",
    "trgl_zbuffer_snapshot", "trgl_zbuffer_restore", "trgl_zbuffer_snapshot_free",
    "trgl_mesh_normals", "trgl_mesh_tangents",
    "trgl_gaussian_kernel", "trgl_image_blur", "trgl_image_scale", "trgl_framebuffer_blur",
    "trgl_image_downsample", "trgl_framebuffer_resolve", "trgl_texture_from_image", "trgl_texture_from_framebuffer",
    "trgl_shadow_matrix", "trgl_shadow_mask_image", "trgl_shadow_mask", "trgl_image_modulate", "trgl_framebuffer_modulate",
    "trgl_clip_layout", "trgl_clip_stage", "trgl_draw_clipped", "trgl_draw_indexed_vs_clipped",
    "trgl_occlusion_boxes_image", "trgl_occlusion_boxes",
    "trgl_draw_instanced", "trgl_instance_stage",
    "trgl_instance_depths", "trgl_depth_order", "trgl_draw_instanced_ordered", "trgl_instance_stage_ordered",
    "trgl_instance_boxes", "trgl_frustum_boxes",
    "trgl_triangle_depths", "trgl_order_stage", "trgl_draw_ordered",
    "trgl_sprite_stage", "trgl_draw_sprites", "trgl_line_stage", "trgl_draw_lines",
    "trgl_skin_stage", "trgl_pose_palette", "trgl_draw_skinned",
    "trgl_mesh_edges", "trgl_edge_select", "trgl_draw_outline",
    "trgl_subdiv_stencil_words", "trgl_subdiv_topology", "trgl_subdiv_vertices", "trgl_draw_subdivided",
    "trgl_mesh_weld", "trgl_mesh_clean", "trgl_mesh_simplify",
    "trgl_mip_layout", "trgl_image_mipmaps", "trgl_texture_mipmaps", "trgl_selftest_sampler_lod", "trgl_image_sample", "trgl_lod_stage", "trgl_selftest_mip_lod",
]
MAX_MIP_LEVELS = 16
SAMPLE_LEVEL, SAMPLE_LINEAR, SAMPLE_TRILINEAR = 0, 1, 2      # the modes of image_sample / selftest_sampler_lod


class Uniforms(C.Structure):
    """trgl_uniforms"""
    _fields_ = [("model_view", C.c_double * 16), ("key_light_dir_eye", C.c_double * 3),
                ("fill_light_dir_eye", C.c_double * 3), ("rim_light_dir_eye", C.c_double * 3),
                ("normal_map_strength", C.c_double), ("tex_diffuse", C.c_int32), ("tex_normal", C.c_int32),
                ("tex_specular", C.c_int32), ("reserved", C.c_int32)]


class Stats(C.Structure):
    """trgl_stats"""
    _fields_ = [("triangles_rasterized", C.c_uint64), ("fragments_drawn", C.c_uint64),
                ("min_x", C.c_int32), ("min_y", C.c_int32), ("max_x", C.c_int32), ("max_y", C.c_int32),
                ("min_z", C.c_double), ("max_z", C.c_double)]

    def astuple(self):
        # z range as (value, sign bit) so that -0.0 and +0.0 compare unequal, as their printed forms do
        import math
        return (self.triangles_rasterized, self.fragments_drawn, self.min_x, self.min_y, self.max_x, self.max_y,
                self.min_z, self.max_z, math.copysign(1.0, self.min_z), math.copysign(1.0, self.max_z))


class SsaoParams(C.Structure):
    """trgl_ssao_params"""
    _fields_ = [("num_directions", C.c_int32), ("steps_per_direction", C.c_int32), ("sample_radius", C.c_double),
                ("occlusion_threshold", C.c_double), ("intensity", C.c_double)]


class ShadowParams(C.Structure):
    """trgl_shadow_params"""
    _fields_ = [("screen_to_light", C.c_double * 16), ("bias", C.c_double), ("darkness", C.c_double),
                ("pcf_radius", C.c_int32), ("reserved", C.c_int32)]


class ClipAttr(C.Structure):
    """trgl_clip_attr"""
    _fields_ = [("offset", C.c_int32), ("components", C.c_int32)]


def make_shadow_params(screen_to_light, bias=1e-3, darkness=0.5, pcf_radius=0) -> ShadowParams:
    """trgl_shadow_params from a row-major 4x4 (shadow_matrix), the depth bias, how much a shadowed pixel loses and the PCF radius."""
    p = ShadowParams()
    p.screen_to_light[:] = np.asarray(screen_to_light, np.float64).reshape(16).tolist()
    p.bias, p.darkness, p.pcf_radius, p.reserved = float(bias), float(darkness), int(pcf_radius), 0
    return p


def make_uniforms(model_view=None, key=(0, 0, 1), fill=(0, 0, 1), rim=(0, 0, 1), normal_map_strength=1.0,
                  tex_diffuse=-1, tex_normal=-1, tex_specular=-1, cells=0) -> Uniforms:
    u = Uniforms()
    mv = np.eye(4) if model_view is None else np.asarray(model_view, np.float64)
    u.model_view[:] = mv.reshape(16).tolist()
    u.key_light_dir_eye[:] = list(map(float, key))
    u.fill_light_dir_eye[:] = list(map(float, fill))
    u.rim_light_dir_eye[:] = list(map(float, rim))
    u.normal_map_strength = float(normal_map_strength)
    u.tex_diffuse, u.tex_normal, u.tex_specular, u.reserved = tex_diffuse, tex_normal, tex_specular, int(cells)      # cells: CHECKER only
    return u


class TrglError(RuntimeError):
    pass


# ---- diagnostic read-back of a flush's intermediate buffers (trgl_debug_read; not part of include/trgl.h) ----
# struct TriRec of csrc/trgl_device.h, one 128-byte line per triangle
TRI_REC = np.dtype([(n, "<f8") for n in ("ax", "ay", "s0x", "s0y", "s1x", "s1y", "c0", "uz", "g1", "g2", "ruz", "z0", "z1", "z2")]
                   + [(n, "<u2") for n in ("bx0", "by0", "bx1", "by1")] + [("color", "<u4"), ("dl", "<u4")])
assert TRI_REC.itemsize == 128, "TRI_REC must mirror sizeof(TriRec) == 128"
DBG_RECS, DBG_CNT, DBG_TILEBOX, DBG_VALS, DBG_BMASK, DBG_TILE_START, DBG_TILE_END, DBG_INFO = range(8)
DBG_INFO_FIELDS = ("N", "P", "capacity", "wide", "literal_tris", "large_tris", "zq_cull", "pending", "W", "H", "tiles_x", "tiles_y",
                   "strip_y0", "strip_y1", "strip_ty0", "strip_ty1", "il_tiles", "il_world", "il_rank", "side", "direct", "fell_back",
                   "seg_S", "seg_G")
BIN_AUTO, BIN_EXPAND, BIN_DIRECT = 0, 1, 2      # trgl_debug_binning: how the next flushes bin
DL_LITERAL = 0x80000000       # TRGL_DL_LITERAL


_lib = None


def load_library(path: str = None):
    """Load libtrgl.so and declare every prototype.  Raises if the library is absent.
    TRGL_LIB in the environment names another build of the same library (profiles/: diagnostic and A/B builds)."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get("TRGL_LIB") or LIB_PATH
    # One HIP runtime per process: torch wheels bundle their own libamdhip64.  If libtrgl.so pulled in
    # /opt/rocm's copy first, a later `import torch` in the same process finds no GPUs; loaded after torch,
    # libtrgl.so binds to the runtime that is already there.  (A C/C++ host without torch is unaffected.)
    if "torch" not in sys.modules and not os.environ.get("TRGL_NO_TORCH_PRELOAD"):
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    if not os.path.exists(path):
        raise TrglError(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                        "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    L = C.CDLL(path)
    vp, u64p, dp = C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    L.trgl_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.trgl_destroy.argtypes = [vp]
    L.trgl_last_error.argtypes = [vp]; L.trgl_last_error.restype = C.c_char_p
    L.trgl_set_viewport.argtypes = [vp, dp]
    L.trgl_init_viewport.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int]
    L.trgl_clear.argtypes = [vp, C.c_void_p, C.c_double]
    L.trgl_upload_texture.argtypes = [vp, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.trgl_set_strip.argtypes = [vp, C.c_int, C.c_int]
    L.trgl_set_interleave.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    L.trgl_draw.argtypes = [vp, C.c_int, C.POINTER(Uniforms), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int]
    L.trgl_flush.argtypes = [vp]
    L.trgl_flush_begin.argtypes = [vp]
    L.trgl_flush_end.argtypes = [vp]
    L.trgl_sync.argtypes = [vp]
    L.trgl_read_framebuffer.argtypes = [vp, C.c_void_p]
    L.trgl_write_framebuffer.argtypes = [vp, C.c_void_p]
    L.trgl_read_zbuffer.argtypes = [vp, C.c_void_p]
    L.trgl_write_zbuffer.argtypes = [vp, C.c_void_p]
    L.trgl_get_stats.argtypes = [vp, C.POINTER(Stats)]
    L.trgl_reset_stats.argtypes = [vp]
    L.trgl_format_stats.argtypes = [C.POINTER(Stats), C.c_char_p, C.c_size_t]
    for name in ("trgl_framebuffer_device_ptr", "trgl_zbuffer_device_ptr", "trgl_stream"):
        getattr(L, name).argtypes = [vp]; getattr(L, name).restype = C.c_void_p
    L.trgl_set_stream.argtypes = [vp, C.c_void_p, C.c_int]
    L.trgl_set_profiling.argtypes = [vp, C.c_int]
    L.trgl_get_phase_ms.argtypes = [vp, dp, u64p]
    L.trgl_reset_phase_ms.argtypes = [vp]
    L.trgl_get_last_flush_info.argtypes = [vp, u64p, u64p, u64p]
    if hasattr(L, "trgl_debug_read"):      # (diagnostic, not part of include/trgl.h: an older build named by TRGL_LIB may lack it)
        L.trgl_debug_read.argtypes = [vp, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    if hasattr(L, "trgl_debug_binning"):
        L.trgl_debug_binning.argtypes = [vp, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    if hasattr(L, "trgl_debug_radix_blocks"):
        L.trgl_debug_radix_blocks.argtypes = [vp, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    if hasattr(L, "trgl_debug_edge_sort"):
        L.trgl_debug_edge_sort.argtypes = [vp, C.c_uint64, C.c_uint64]
    if hasattr(L, "trgl_debug_subdiv_sort"):
        L.trgl_debug_subdiv_sort.argtypes = [vp, C.c_uint64, C.c_uint64]
    if hasattr(L, "trgl_debug_weld_hash_bits"):
        L.trgl_debug_weld_hash_bits.argtypes = [vp, C.c_int]
        L.trgl_debug_weld_sort.argtypes = [vp, C.c_uint64]
        L.trgl_debug_weld_hash.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    if hasattr(L, "trgl_debug_lod_hash_bits"):
        L.trgl_debug_lod_hash_bits.argtypes = [vp, C.c_int]
        L.trgl_debug_lod_sort.argtypes = [vp, C.c_uint64, C.c_uint64]
        L.trgl_debug_lod_face_hash.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
    L.trgl_selftest_division.argtypes = [vp, C.c_uint64, C.c_uint64, u64p]
    L.trgl_selftest_sampler.argtypes = [vp, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p]
    L.trgl_draw_indexed.argtypes = [vp, C.c_int, C.POINTER(Uniforms), dp, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int]
    L.trgl_ssao_defaults.argtypes = [C.POINTER(SsaoParams)]
    L.trgl_ssao_defaults.restype = None
    L.trgl_postprocess.argtypes = [vp, C.POINTER(SsaoParams), C.c_void_p, C.c_void_p, C.c_void_p]
    L.trgl_obj_load.argtypes = [C.c_char_p, C.POINTER(C.POINTER(C.c_double)), u64p, C.POINTER(C.POINTER(C.c_uint32)), u64p]
    L.trgl_obj_free.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_uint32)]
    L.trgl_obj_free.restype = None
    L.trgl_tga_max_size.argtypes = [C.c_int, C.c_int, C.c_int]
    L.trgl_tga_max_size.restype = C.c_size_t
    L.trgl_tga_encode.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_size_t)]
    L.trgl_tga_info.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.trgl_tga_decode.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    L.trgl_gather.argtypes = [vp, C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.trgl_rccl_unique_id.argtypes = [C.c_void_p]
    L.trgl_rccl_comm_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.trgl_rccl_comm_destroy.argtypes = [C.c_void_p]
    L.trgl_shader_compile.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_size_t]
    L.trgl_register_shader.argtypes = [vp, C.c_char_p, C.c_int, C.POINTER(C.c_int)]
    L.trgl_shader_compile_ex.argtypes = [C.c_char_p, C.c_int, C.c_uint32, C.c_char_p, C.c_size_t]
    L.trgl_register_shader_ex.argtypes = [vp, C.c_char_p, C.c_int, C.c_uint32, C.POINTER(C.c_int)]
    L.trgl_vertex_shader_compile.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_size_t]
    L.trgl_register_vertex_shader.argtypes = [vp, C.c_char_p, C.c_int, C.POINTER(C.c_int)]
    L.trgl_draw_indexed_vs.argtypes = [vp, C.c_int, C.c_int, C.POINTER(Uniforms), dp, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_uint64,
                                       C.c_void_p, C.c_int]
    L.trgl_vertex_stage.argtypes = [vp, C.c_int, C.POINTER(Uniforms), dp, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_uint64,
                                    C.c_void_p, C.c_void_p, C.c_int]
    L.trgl_mesh_bounds.argtypes = [vp, C.c_void_p, C.c_int, C.c_uint64, C.c_int, dp, dp]
    for name in ("trgl_mesh_normals", "trgl_mesh_tangents"):
        getattr(L, name).argtypes = [vp, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.POINTER(C.c_int)]
    L.trgl_aabb_transform.argtypes = [dp, dp, dp, dp, dp]
    L.trgl_frustum_from_matrix.argtypes = [dp, dp]
    L.trgl_frustum_intersects.argtypes = [dp, dp, dp]
    for name in ("trgl_zbuffer_snapshot", "trgl_zbuffer_restore", "trgl_zbuffer_snapshot_free"):
        getattr(L, name).argtypes = [vp, C.c_int]
    L.trgl_gaussian_kernel.argtypes = [C.c_int, C.c_void_p]
    L.trgl_image_blur.argtypes = [vp, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.trgl_image_scale.argtypes = [vp, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.trgl_framebuffer_blur.argtypes = [vp, C.c_int]
    L.trgl_image_downsample.argtypes = [vp, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    L.trgl_framebuffer_resolve.argtypes = [vp, C.c_int, C.c_void_p, C.c_int]
    L.trgl_texture_from_image.argtypes = [vp, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.trgl_texture_from_framebuffer.argtypes = [vp, C.c_int, C.c_int]
    L.trgl_shadow_matrix.argtypes = [dp, dp, dp, dp, dp, dp, dp]
    L.trgl_shadow_mask_image.argtypes = [vp, C.POINTER(ShadowParams), C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    L.trgl_shadow_mask.argtypes = [vp, C.POINTER(ShadowParams), C.c_int, C.c_void_p, C.c_int]
    L.trgl_image_modulate.argtypes = [vp, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    L.trgl_framebuffer_modulate.argtypes = [vp, C.c_void_p, C.c_int]
    cap = C.POINTER(ClipAttr)
    L.trgl_clip_layout.argtypes = [C.c_int, cap, C.POINTER(C.c_int)]
    L.trgl_clip_stage.argtypes = [vp, dp, cap, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                  C.c_void_p, C.c_void_p, C.c_void_p, u64p, C.c_int]
    L.trgl_draw_clipped.argtypes = [vp, C.c_int, C.POINTER(Uniforms), dp, cap, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int]
    L.trgl_draw_indexed_vs_clipped.argtypes = [vp, C.c_int, C.c_int, C.POINTER(Uniforms), dp, dp, cap, C.c_int, C.c_void_p, C.c_int, C.c_uint64,
                                               C.c_void_p, C.c_uint64, C.c_void_p, C.c_int]
    L.trgl_occlusion_boxes_image.argtypes = [vp, C.c_void_p, C.c_int, C.c_int, dp, dp, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int]
    L.trgl_occlusion_boxes.argtypes = [vp, dp, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_void_p, C.c_int]
    inst = [C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int,      # the mesh
            C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int]                   # the instances
    L.trgl_draw_instanced.argtypes = [vp, C.c_int, C.c_int, C.POINTER(Uniforms), dp] + inst
    L.trgl_instance_stage.argtypes = [vp, C.c_int, C.POINTER(Uniforms), dp] + inst + [C.c_void_p, C.c_void_p, C.c_void_p, u64p]
    order = [C.c_void_p, C.c_uint64, C.c_int]
    L.trgl_draw_instanced_ordered.argtypes = [vp, C.c_int, C.c_int, C.POINTER(Uniforms), dp] + inst + order
    L.trgl_instance_stage_ordered.argtypes = [vp, C.c_int, C.POINTER(Uniforms), dp] + inst + order + [C.c_void_p, C.c_void_p, C.c_void_p, u64p]
    L.trgl_instance_depths.argtypes = [vp, dp, dp, C.c_void_p, C.c_int, C.c_uint64, C.c_int, C.c_void_p]
    L.trgl_depth_order.argtypes = [vp, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_void_p]
    L.trgl_instance_boxes.argtypes = [vp, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_uint64, C.c_int, C.c_void_p]
    L.trgl_frustum_boxes.argtypes = [vp, dp, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_void_p]
    L.trgl_triangle_depths.argtypes = [vp, C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_int, C.c_void_p]
    L.trgl_order_stage.argtypes = [vp, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_int,
                                   C.c_void_p, C.c_void_p, C.c_void_p]
    L.trgl_draw_ordered.argtypes = [vp, C.c_int, C.POINTER(Uniforms), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int,
                                    C.c_void_p, C.c_uint64, C.c_uint32, C.c_int]
    ip = C.POINTER(C.c_int)
    L.trgl_mip_layout.argtypes = [C.c_int, C.c_int, C.c_int, ip, ip, ip, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.trgl_image_mipmaps.argtypes = [vp, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    L.trgl_texture_mipmaps.argtypes = [vp, C.c_int]
    L.trgl_selftest_sampler_lod.argtypes = [vp, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p]
    L.trgl_image_sample.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p]
    L.trgl_selftest_mip_lod.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_void_p]
    L.trgl_lod_stage.argtypes = [vp, dp, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int]
    L.trgl_sprite_stage.argtypes = [vp, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.trgl_draw_sprites.argtypes = [vp, C.c_int, C.POINTER(Uniforms), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_int]
    L.trgl_line_stage.argtypes = [vp, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int,
                                  C.c_void_p, C.c_void_p, C.c_void_p]
    L.trgl_draw_lines.argtypes = [vp, C.c_int, C.POINTER(Uniforms), C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p,
                                  C.c_uint64, C.c_int]
    L.trgl_skin_stage.argtypes = [vp, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.trgl_pose_palette.argtypes = [vp, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64]
    L.trgl_draw_skinned.argtypes = [vp, C.c_int, C.c_int, C.POINTER(Uniforms), dp, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int]
    L.trgl_mesh_edges.argtypes = [vp, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p, u64p]
    L.trgl_edge_select.argtypes = [vp, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int,
                                   C.c_void_p, C.c_void_p, C.c_void_p, u64p]
    L.trgl_draw_outline.argtypes = [vp, C.c_int, C.POINTER(Uniforms), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p,
                                    C.c_uint64, C.c_void_p, C.c_uint64, C.c_int]
    L.trgl_mesh_weld.argtypes = [vp, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, u64p]
    L.trgl_mesh_clean.argtypes = [vp, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, u64p]
    L.trgl_mesh_simplify.argtypes = [vp, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, u64p]
    L.trgl_subdiv_stencil_words.argtypes = [C.c_uint64, C.c_uint64]
    L.trgl_subdiv_stencil_words.restype = C.c_uint64
    L.trgl_subdiv_topology.argtypes = [vp, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]
    L.trgl_subdiv_vertices.argtypes = [vp, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]
    L.trgl_draw_subdivided.argtypes = [vp, C.c_int, C.c_int, C.POINTER(Uniforms), dp, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                       C.c_void_p, C.c_uint64, C.c_void_p, C.c_int]
    for name in SYMBOLS:
        f = getattr(L, name)
        if f.restype is C.c_int and name not in ("trgl_last_error",):
            f.restype = C.c_int
    _lib = L
    return L


def rccl_unique_id() -> bytes:
    """ncclGetUniqueId through the C ABI: 128 bytes that rank 0 hands to the other ranks."""
    L = load_library()
    buf = (C.c_uint8 * 128)()
    rc = L.trgl_rccl_unique_id(buf)
    if rc != 0:
        raise TrglError(f"trgl_rccl_unique_id failed ({rc}): {L.trgl_last_error(None).decode()}")
    return bytes(buf)


def rccl_comm_create(unique_id: bytes, rank: int, world: int, device: int = 0):
    """ncclCommInitRank through the C ABI; returns the communicator handle for Context.gather()."""
    L = load_library()
    comm = C.c_void_p()
    buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
    rc = L.trgl_rccl_comm_create(buf, rank, world, device, C.byref(comm))
    if rc != 0:
        raise TrglError(f"trgl_rccl_comm_create failed ({rc}): {L.trgl_last_error(None).decode()}")
    return comm


def rccl_comm_destroy(comm):
    load_library().trgl_rccl_comm_destroy(comm)


def shader_compile(source: str, n_varyings: int, may_discard: bool = False, *, reads_dest: bool = False, depth_write: bool = True):
    """trgl_shader_compile_ex: compile a user shader (include/trgl.h, "User shaders") without a GPU or a context; may_discard: one
    whose trgl_fragment returns trgl_frag_out (TRGL_SHADER_MAY_DISCARD).  reads_dest: in.dst is the pixel under the fragment
    (TRGL_SHADER_READS_DEST); depth_write=False: TRGL_SHADER_NO_DEPTH_WRITE.  Both need may_discard.
    Returns (ok, compiler log); raises when user shaders are unavailable (no hiprtc)."""
    L = load_library()
    log = C.create_string_buffer(16384)
    rc = L.trgl_shader_compile_ex(source.encode(), int(n_varyings), shader_flags(may_discard, reads_dest, depth_write), log, len(log))
    if rc not in (0, -1):
        raise TrglError(f"trgl_shader_compile failed ({rc}): {log.value.decode(errors='replace')}")
    return rc == 0, log.value.decode(errors="replace")


def vertex_shader_compile(source: str, n_varyings: int):
    """trgl_vertex_shader_compile: compile a user vertex shader (include/trgl.h, "User vertex shaders") without a GPU or a context.
    Returns (ok, compiler log); raises when user shaders are unavailable (no hiprtc)."""
    L = load_library()
    log = C.create_string_buffer(16384)
    rc = L.trgl_vertex_shader_compile(source.encode(), int(n_varyings), log, len(log))
    if rc not in (0, -1):
        raise TrglError(f"trgl_vertex_shader_compile failed ({rc}): {log.value.decode(errors='replace')}")
    return rc == 0, log.value.decode(errors="replace")


def _ptr(a):
    """host numpy array, or an object with a device pointer (torch tensor / int)."""
    if a is None:
        return None
    if isinstance(a, int):
        return a
    if hasattr(a, "data_ptr"):
        return a.data_ptr()
    return a.ctypes.data


def _device_ptr(a, what="array"):
    """The address of an array handed over with device=True: an int (a raw device pointer), or an object with data_ptr() whose
    is_cuda is true (a torch CUDA tensor); None stays None.  Anything else - a numpy array, a CPU tensor - raises TypeError
    before the library is called: its address would reach a kernel as it is."""
    if a is None:
        return None
    if isinstance(a, int) and not isinstance(a, bool):
        return a
    if hasattr(a, "data_ptr") and getattr(a, "is_cuda", False) is True:
        return a.data_ptr()
    raise TypeError(f"device=True: {what} must be a device tensor or an int device pointer, not {type(a).__name__}"
                    + (" in host memory" if hasattr(a, "data_ptr") else ""))


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _f64(a, n, what):
    a = np.ascontiguousarray(a, np.float64).reshape(-1)
    if a.size != n:
        raise ValueError(f"{what}: {n} doubles expected, got {a.size}")
    return a


def _mesh_bounds(L, handle, vertices, device):
    lo, hi = np.empty(3, np.float64), np.empty(3, np.float64)
    if device:
        ptr = _device_ptr(vertices, "vertices")
    else:
        vertices = np.ascontiguousarray(vertices, np.float64)
        ptr = vertices.ctypes.data
    if len(vertices.shape) != 2:
        raise ValueError("mesh_bounds: vertices must be [n, stride]")
    nv, stride = vertices.shape
    rc = L.trgl_mesh_bounds(handle, ptr, int(stride), int(nv), MEM_DEVICE if device else MEM_HOST, _dp(lo), _dp(hi))
    if rc != 0:
        raise TrglError(f"trgl_mesh_bounds failed ({rc}): {L.trgl_last_error(handle).decode()}")
    return lo, hi


def mesh_bounds(vertices):
    """trgl_mesh_bounds for a host array without a context: Model::computeAABB (model.cpp:15-40) of vertices [n, stride >= 3] with the
    position at +0; returns (min[3], max[3]) with the reference's 1 % margin.  Needs no GPU."""
    return _mesh_bounds(load_library(), None, vertices, False)


def _mesh_attr(L, handle, name, ptrs, vertices, indices, device, wait):
    if len(vertices.shape) != 2 or len(indices.shape) != 2 or indices.shape[1] != 3:
        raise ValueError(f"{name}: vertices must be [n, stride] and indices [n_faces, 3]")
    nv, stride = vertices.shape
    generated = C.c_int(0)
    rc = getattr(L, "trgl_" + name)(handle, ptrs[0], int(stride), int(nv), ptrs[1], int(indices.shape[0]), MEM_DEVICE if device else MEM_HOST,
                                    C.byref(generated) if wait else None)
    if rc != 0:
        raise TrglError(f"trgl_{name} failed ({rc}): {L.trgl_last_error(handle).decode()}")
    return bool(generated.value) if wait else None


def _host_mesh(vertices, indices):
    """A private, writable, contiguous copy of the vertices, and the indices as [n_faces, 3] uint32."""
    return np.array(vertices, np.float64, order="C"), np.ascontiguousarray(indices, np.uint32).reshape(-1, 3)


def mesh_normals(vertices, indices):
    """trgl_mesh_normals for host arrays without a context: Model::generateNormalsIfNeeded (model.cpp:269-316) on a copy of vertices
    [n, stride >= 6] (normal at +3) with indices [n_faces, 3]; returns (vertices, generated).  Needs no GPU."""
    v, i = _host_mesh(vertices, indices)
    return v, _mesh_attr(load_library(), None, "mesh_normals", (v.ctypes.data, i.ctypes.data), v, i, False, True)


def mesh_tangents(vertices, indices):
    """trgl_mesh_tangents likewise: Model::computeTangentsIfNeeded (model.cpp:318-388) on a copy of vertices [n, stride >= 14]
    (texcoord +6, tangent +8, bitangent +11); returns (vertices, generated).  Needs no GPU."""
    v, i = _host_mesh(vertices, indices)
    return v, _mesh_attr(load_library(), None, "mesh_tangents", (v.ctypes.data, i.ctypes.data), v, i, False, True)


def gaussian_kernel(radius: int) -> np.ndarray:
    """trgl_gaussian_kernel: the 2 * radius + 1 float32 weights of TGAImage::gaussian_blur (tgaimage.cpp:275-284), computed on the host as
    the reference computes them.  Needs no GPU."""
    L = load_library()
    out = np.empty(2 * max(int(radius), 0) + 1, np.float32)
    rc = L.trgl_gaussian_kernel(int(radius), out.ctypes.data)
    if rc != 0:
        raise TrglError(f"trgl_gaussian_kernel failed ({rc}): {L.trgl_last_error(None).decode()}")
    return out


def _image_dims(img, what):
    if len(img.shape) != 3 or img.shape[2] not in (1, 3, 4):
        raise ValueError(f"{what}: the image must be [h, w, bpp] with bpp in (1, 3, 4)")
    return int(img.shape[0]), int(img.shape[1]), int(img.shape[2])


def _image_blur(L, handle, ptr, img, radius, device):
    h, w, bpp = _image_dims(img, "image_blur")
    rc = L.trgl_image_blur(handle, ptr, w, h, bpp, int(radius), MEM_DEVICE if device else MEM_HOST)
    if rc != 0:
        raise TrglError(f"trgl_image_blur failed ({rc}): {L.trgl_last_error(handle).decode()}")


def _image_scale(L, handle, sptr, img, dptr, w2, h2, device):
    h, w, bpp = _image_dims(img, "image_scale")
    rc = L.trgl_image_scale(handle, sptr, w, h, bpp, dptr, int(w2), int(h2), MEM_DEVICE if device else MEM_HOST)
    if rc != 0:
        raise TrglError(f"trgl_image_scale failed ({rc}): {L.trgl_last_error(handle).decode()}")


def _image_downsample(L, handle, sptr, img, factor, dptr, device):
    h, w, bpp = _image_dims(img, "image_downsample")
    rc = L.trgl_image_downsample(handle, sptr, w, h, bpp, int(factor), dptr, MEM_DEVICE if device else MEM_HOST)
    if rc != 0:
        raise TrglError(f"trgl_image_downsample failed ({rc}): {L.trgl_last_error(handle).decode()}")


def _box_shape(img, factor):
    """[h2, w2, bpp] of the box filter's result; zeros where the library will refuse the factor."""
    f = int(factor)
    ok = len(img.shape) == 3 and f >= 1
    return (int(img.shape[0]) // f if ok else 0, int(img.shape[1]) // f if ok else 0, int(img.shape[2]) if len(img.shape) == 3 else 0)


def _host_image_downsample(L, handle, img, factor, out=None):
    src = np.ascontiguousarray(img, np.uint8)
    shape = _box_shape(src, factor)
    if out is None:
        out = np.empty(shape, np.uint8)
    elif out.dtype != np.uint8 or not out.flags.c_contiguous or out.shape != shape:
        raise ValueError("image_downsample: out must be a contiguous uint8 array [h // factor, w // factor, bpp]")
    _image_downsample(L, handle, src.ctypes.data, src, factor, out.ctypes.data, False)
    return out


def _device_image(img, what):
    """The address of a device image: a contiguous uint8 CUDA tensor (its shape says w, h and bpp, so a bare pointer will not do)."""
    if not hasattr(img, "data_ptr"):
        raise TypeError(f"device=True: {what} must be a device tensor, not {type(img).__name__}")
    if str(img.dtype) != "torch.uint8" or not img.is_contiguous():
        raise ValueError(f"device=True: {what} must be a contiguous uint8 tensor")
    return _device_ptr(img, what)


def image_blur(img, radius: int) -> np.ndarray:
    """trgl_image_blur for a host array without a context: TGAImage::gaussian_blur (tgaimage.cpp:271-324) on a copy of img [h, w, bpp] uint8;
    returns the copy.  radius <= 0 returns it unchanged, as the reference does.  Needs no GPU."""
    out = np.array(img, np.uint8, order="C")
    _image_blur(load_library(), None, out.ctypes.data, out, radius, False)
    return out


def image_scale(img, w2: int, h2: int) -> np.ndarray:
    """trgl_image_scale for a host array without a context: TGAImage::scale (tgaimage.cpp:246-267) of img [h, w, bpp] uint8 into a new
    [h2, w2, bpp] array.  Raises where the reference returns false (a size <= 0, an empty image).  Needs no GPU."""
    src = np.ascontiguousarray(img, np.uint8)
    out = np.empty((max(int(h2), 0), max(int(w2), 0), src.shape[2] if len(src.shape) == 3 else 0), np.uint8)
    _image_scale(load_library(), None, src.ctypes.data, src, out.ctypes.data, w2, h2, False)
    return out


def image_downsample(img, factor: int) -> np.ndarray:
    """trgl_image_downsample for a host array without a context: the exact box filter (new work, include/trgl.h) of img [h, w, bpp] uint8
    into a new [h // factor, w // factor, bpp] array: (sum of factor x factor bytes + factor * factor // 2) // (factor * factor) per
    channel.  Raises for a factor outside 1..16 or above w or h.  Needs no GPU."""
    return _host_image_downsample(load_library(), None, img, factor)


def mip_layout(w: int, h: int, bpp: int):
    """trgl_mip_layout: (widths, heights, offsets, total) of the mip chain of a w x h image - the sizes of all L levels, the byte offsets of
    levels 1 .. L-1 in the packed buffer (offsets[0] is 0 and names nothing) and that buffer's bytes.  Needs no GPU."""
    L = load_library()
    n, total = C.c_int(), C.c_size_t()
    ws, hs, offs = (C.c_int * MAX_MIP_LEVELS)(), (C.c_int * MAX_MIP_LEVELS)(), (C.c_size_t * MAX_MIP_LEVELS)()
    rc = L.trgl_mip_layout(int(w), int(h), int(bpp), C.byref(n), ws, hs, offs, C.byref(total))
    if rc != 0:
        raise TrglError(f"trgl_mip_layout failed ({rc}): {L.trgl_last_error(None).decode()}")
    return list(ws[:n.value]), list(hs[:n.value]), list(offs[:n.value]), int(total.value)


def _image_mipmaps(L, handle, sptr, img, dptr, device):
    h, w, bpp = _image_dims(img, "image_mipmaps")
    rc = L.trgl_image_mipmaps(handle, sptr, w, h, bpp, dptr, MEM_DEVICE if device else MEM_HOST)
    if rc != 0:
        raise TrglError(f"trgl_image_mipmaps failed ({rc}): {L.trgl_last_error(handle).decode()}")


def _host_image_mipmaps(L, handle, img, out=None):
    src = np.ascontiguousarray(img, np.uint8)
    h, w, bpp = _image_dims(src, "image_mipmaps")
    total = mip_layout(w, h, bpp)[3]
    if out is None:
        out = np.zeros(total, np.uint8)
    elif out.dtype != np.uint8 or not out.flags.c_contiguous or out.shape != (total,):
        raise ValueError("image_mipmaps: out must be a contiguous uint8 array of mip_layout(w, h, bpp)[3] bytes")
    _image_mipmaps(L, handle, src.ctypes.data, src, out.ctypes.data, False)
    return out


def image_mipmaps(img) -> np.ndarray:
    """trgl_image_mipmaps for a host array without a context: levels 1 .. L-1 of img [h, w, bpp] uint8 as one packed uint8 array in the
    layout of mip_layout (the padding between levels is zero here: the array is new).  Needs no GPU."""
    return _host_image_mipmaps(load_library(), None, img)


def image_sample(img, chain, uv, lod, mode=SAMPLE_TRILINEAR, levels=None) -> np.ndarray:
    """trgl_image_sample: the filtered samplers of the user shaders on the host, over img [h, w, bpp] uint8 and its packed chain (None:
    one level) at uv [n, 2] and lod [n]; mode SAMPLE_LEVEL / SAMPLE_LINEAR (lod converted to int) / SAMPLE_TRILINEAR.  Returns [n, 5]
    uint8 = bgra[4], bytespp, as selftest_sampler does.  Needs no GPU."""
    L = load_library()
    src = np.ascontiguousarray(img, np.uint8)
    h, w, bpp = _image_dims(src, "image_sample")
    chain = None if chain is None else np.ascontiguousarray(chain, np.uint8)
    if levels is None:
        levels = 1 if chain is None else MAX_MIP_LEVELS
    if chain is not None and int(levels) > 1 and chain.size < mip_layout(w, h, bpp)[3]:
        raise ValueError("image_sample: chain is shorter than mip_layout(w, h, bpp)[3] bytes")
    uv = np.ascontiguousarray(uv, np.float64).reshape(-1, 2)
    lod = np.ascontiguousarray(np.broadcast_to(np.asarray(lod, np.float64), (uv.shape[0],)))
    out = np.zeros((uv.shape[0], 5), np.uint8)
    rc = L.trgl_image_sample(src.ctypes.data, None if chain is None else chain.ctypes.data, w, h, bpp, int(levels),
                             uv.ctypes.data, lod.ctypes.data, int(mode), uv.shape[0], out.ctypes.data)
    if rc != 0:
        raise TrglError(f"trgl_image_sample failed ({rc}): {L.trgl_last_error(None).decode()}")
    return out


def mip_lod(bar, k, tex_w: int, tex_h: int) -> np.ndarray:
    """trgl_selftest_mip_lod: the host's compile of the user shaders' trgl_mip_lod over bar [n, 3] and k [n, 4]; returns [n] float64 levels
    of detail for a tex_w x tex_h texture.  Needs no GPU."""
    L = load_library()
    bar = np.ascontiguousarray(bar, np.float64).reshape(-1, 3)
    k = np.ascontiguousarray(np.broadcast_to(np.asarray(k, np.float64), (bar.shape[0], 4)))
    out = np.zeros(bar.shape[0], np.float64)
    rc = L.trgl_selftest_mip_lod(bar.ctypes.data, k.ctypes.data, int(tex_w), int(tex_h), bar.shape[0], out.ctypes.data)
    if rc != 0:
        raise TrglError(f"trgl_selftest_mip_lod failed ({rc}): {L.trgl_last_error(None).decode()}")
    return out


def _lod_stage(L, handle, viewport, clip, varyings, uv_offset, out_offset, device):
    """In place on `varyings`; returns the arrays to keep alive."""
    vp_m = np.ascontiguousarray(viewport, np.float64).reshape(16)
    if device:
        for a, what in ((clip, "clip"), (varyings, "varyings")):
            if not _is_device_tensor(a) or str(a.dtype) != "torch.float64" or not a.is_contiguous() or a.dim() != 2:
                raise ValueError(f"device=True: {what} must be a contiguous float64 device tensor with 2 dimensions")
        n, K = int(clip.shape[0]), int(varyings.shape[1])
        if int(clip.shape[1]) != 12 or int(varyings.shape[0]) != n:
            raise ValueError("lod_stage: clip must be [n, 12] and varyings [n, K]")
        ptrs = (clip.data_ptr() if n else None, varyings.data_ptr() if n else None)
    else:
        if not isinstance(varyings, np.ndarray) or varyings.dtype != np.float64 or not varyings.flags.c_contiguous or varyings.ndim != 2:
            raise ValueError("lod_stage: varyings must be a contiguous float64 array [n, K] (it is rewritten in place)")
        clip = np.ascontiguousarray(clip, np.float64).reshape(-1, 12)
        n, K = clip.shape[0], varyings.shape[1]
        if varyings.shape[0] != n:
            raise ValueError("lod_stage: clip must be [n, 12] and varyings [n, K]")
        ptrs = (clip.ctypes.data if n else None, varyings.ctypes.data if n else None)
    rc = L.trgl_lod_stage(handle, _dp(vp_m), ptrs[0], ptrs[1], n, K, int(uv_offset), int(out_offset), MEM_DEVICE if device else MEM_HOST)
    if rc != 0:
        raise TrglError(f"trgl_lod_stage failed ({rc}): {L.trgl_last_error(handle).decode()}")
    return clip, varyings


def lod_stage(viewport, clip, varyings, uv_offset=0, out_offset=6):
    """trgl_lod_stage for host arrays without a context: for every triangle of clip [n, 12] the four level-of-detail doubles
    (c, W0, W1, W2) from its clip row, the Viewport [4, 4] and its six uv doubles at varyings[:, uv_offset:uv_offset + 6], written in place
    at varyings[:, out_offset:out_offset + 4] (a contiguous float64 array [n, K]); returns varyings.  Needs no GPU."""
    return _lod_stage(load_library(), None, viewport, clip, varyings, uv_offset, out_offset, False)[1]


def shadow_matrix(light_mv, light_proj, light_vp, cam_mv, cam_proj, cam_vp) -> np.ndarray:
    """trgl_shadow_matrix: (Lvp * Lproj * Lmv) * inverse(Cvp * Cproj * Cmv) as a row-major [4, 4] - ShadowParams.screen_to_light.
    Raises where the camera's matrix is singular.  Needs no GPU."""
    L = load_library()
    ms = [_f64(m, 16, "shadow_matrix") for m in (light_mv, light_proj, light_vp, cam_mv, cam_proj, cam_vp)]
    out = np.empty(16, np.float64)
    rc = L.trgl_shadow_matrix(*[_dp(m) for m in ms], _dp(out))
    if rc != 0:
        raise TrglError(f"trgl_shadow_matrix failed ({rc}): {L.trgl_last_error(None).decode()}")
    return out.reshape(4, 4)


def _depth_dims(a, what):
    if len(a.shape) != 2:
        raise ValueError(f"{what} must be [h, w]")
    return int(a.shape[0]), int(a.shape[1])


def _shadow_mask_image(L, handle, params, dptr, depth, mptr, zmap, optr, device):
    h, w = _depth_dims(depth, "shadow_mask_image: depth")
    mh, mw = _depth_dims(zmap, "shadow_mask_image: map")
    rc = L.trgl_shadow_mask_image(handle, C.byref(params), dptr, w, h, mptr, mw, mh, optr, MEM_DEVICE if device else MEM_HOST)
    if rc != 0:
        raise TrglError(f"trgl_shadow_mask_image failed ({rc}): {L.trgl_last_error(handle).decode()}")


def _image_modulate(L, handle, ptr, img, mptr, mask, device):
    h, w, bpp = _image_dims(img, "image_modulate")
    if tuple(mask.shape[:2]) != (h, w) or int(np.prod(tuple(mask.shape))) != h * w:
        raise ValueError("image_modulate: the mask must be [h, w] (or [h, w, 1]) like the image")
    rc = L.trgl_image_modulate(handle, ptr, w, h, bpp, mptr, MEM_DEVICE if device else MEM_HOST)
    if rc != 0:
        raise TrglError(f"trgl_image_modulate failed ({rc}): {L.trgl_last_error(handle).decode()}")


def _host_shadow_mask_image(L, handle, params, depth, zmap):
    depth, zmap = np.ascontiguousarray(depth, np.float64), np.ascontiguousarray(zmap, np.float64)
    out = np.empty(depth.shape, np.uint8)
    _shadow_mask_image(L, handle, params, depth.ctypes.data, depth, zmap.ctypes.data, zmap, out.ctypes.data, False)
    return out


def _host_image_modulate(L, handle, img, mask):
    out, mask = np.array(img, np.uint8, order="C"), np.ascontiguousarray(mask, np.uint8)
    _image_modulate(L, handle, out.ctypes.data, out, mask.ctypes.data, mask, False)
    return out


def shadow_mask_image(params: ShadowParams, depth, zmap) -> np.ndarray:
    """trgl_shadow_mask_image for host arrays without a context: the [h, w] uint8 mask of the depths [h, w] against the light's depth map
    [map_h, map_w] (the steps are written down in include/trgl.h).  Needs no GPU."""
    return _host_shadow_mask_image(load_library(), None, params, depth, zmap)


def image_modulate(img, mask) -> np.ndarray:
    """trgl_image_modulate for host arrays without a context: a copy of img [h, w, bpp] uint8 with its colour channels multiplied by
    mask [h, w] / 255 (main.cpp:775-781); alpha stays.  Needs no GPU."""
    return _host_image_modulate(load_library(), None, img, mask)


def _boxes_count(boxes):
    if len(boxes.shape) != 2 or boxes.shape[1] != 6:
        raise ValueError("occlusion: boxes must be [n, 6] (min.xyz, max.xyz)")
    return int(boxes.shape[0])


def _occlusion_boxes_image(L, handle, dptr, depth, viewport, view_proj, bptr, n, optr, device):
    h, w = _depth_dims(depth, "occlusion_boxes_image: depth")
    rc = L.trgl_occlusion_boxes_image(handle, dptr, w, h, _dp(_f64(viewport, 16, "viewport")), _dp(_f64(view_proj, 16, "view_proj")),
                                      bptr, n, optr, MEM_DEVICE if device else MEM_HOST)
    if rc != 0:
        raise TrglError(f"trgl_occlusion_boxes_image failed ({rc}): {L.trgl_last_error(handle).decode()}")


def _host_occlusion_boxes_image(L, handle, depth, viewport, view_proj, boxes):
    depth, boxes = np.ascontiguousarray(depth, np.float64), np.ascontiguousarray(boxes, np.float64)
    out = np.empty(_boxes_count(boxes), np.uint8)
    _occlusion_boxes_image(L, handle, depth.ctypes.data, depth, viewport, view_proj, boxes.ctypes.data, out.size, out.ctypes.data, False)
    return out


def occlusion_boxes_image(depth, viewport, view_proj, boxes) -> np.ndarray:
    """trgl_occlusion_boxes_image for host arrays without a context: one OCCL_* code (uint8) per box [n, 6] = (min.xyz, max.xyz) against
    the depths [h, w] under the row-major viewport and view_proj = Perspective * ModelView (the steps are written down in include/trgl.h).
    Bit 0 of a code set: draw the model.  Needs no GPU."""
    return _host_occlusion_boxes_image(load_library(), None, depth, viewport, view_proj, boxes)


def _instance_depths(L, handle, model_view, point, instances, device):
    mv, pt = _f64(model_view, 16, "model_view"), _f64(point, 3, "point")
    if device:
        if not hasattr(instances, "data_ptr") or str(instances.dtype) != "torch.float64" or not instances.is_contiguous() or instances.dim() != 2:
            raise ValueError("device=True: instances must be a contiguous float64 device tensor [n, stride]")
        import torch
        out = torch.empty(int(instances.shape[0]), dtype=torch.float64, device=instances.device)
        ptrs = (_device_ptr(instances, "instances") if out.numel() else None, out.data_ptr() if out.numel() else None)
    else:
        instances = np.ascontiguousarray(instances, np.float64)
        if instances.ndim != 2:
            raise ValueError("instances: [n, stride] expected")
        out = np.empty(instances.shape[0], np.float64)
        ptrs = (instances.ctypes.data, out.ctypes.data)
    rc = L.trgl_instance_depths(handle, _dp(mv), _dp(pt), ptrs[0], int(instances.shape[1]), int(instances.shape[0]),
                                MEM_DEVICE if device else MEM_HOST, ptrs[1])
    if rc != 0:
        raise TrglError(f"trgl_instance_depths failed ({rc}): {L.trgl_last_error(handle).decode()}")
    return instances, out


def _depth_order(L, handle, depths, front_to_back, device):
    if device:
        if not hasattr(depths, "data_ptr") or str(depths.dtype) != "torch.float64" or not depths.is_contiguous() or depths.dim() != 1:
            raise ValueError("device=True: depths must be a contiguous float64 device tensor [n]")
        import torch
        out = torch.empty(int(depths.shape[0]), dtype=torch.int32, device=depths.device)       # (torch has no uint32 arithmetic: the bits are uint32)
        ptrs = (_device_ptr(depths, "depths") if out.numel() else None, out.data_ptr() if out.numel() else None)
    else:
        depths = np.ascontiguousarray(depths, np.float64).reshape(-1)
        out = np.empty(depths.shape[0], np.uint32)
        ptrs = (depths.ctypes.data, out.ctypes.data)
    rc = L.trgl_depth_order(handle, ptrs[0], int(depths.shape[0]), ORDER_FRONT_TO_BACK if front_to_back else ORDER_BACK_TO_FRONT,
                            MEM_DEVICE if device else MEM_HOST, ptrs[1])
    if rc != 0:
        raise TrglError(f"trgl_depth_order failed ({rc}): {L.trgl_last_error(handle).decode()}")
    return depths, out


def instance_depths(model_view, point, instances) -> np.ndarray:
    """trgl_instance_depths for host arrays without a context: the view-space z of `point` (model space) under every instance [n, stride
    >= 16] - element 2 of (model_view * M_i) * (point, 1), summed as the reference's geometry.h sums it.  Needs no GPU."""
    return _instance_depths(load_library(), None, model_view, point, instances, False)[1]


def depth_order(depths, front_to_back=False) -> np.ndarray:
    """trgl_depth_order for a host array without a context: the uint32 permutation that draws the depths farthest first (under a view
    matrix that looks down -z: ascending), or nearest first; ties in ascending number either way.  The order is that of the doubles' bit
    patterns as include/trgl.h defines it (-0.0 before +0.0, NaNs at the ends by their sign).  Needs no GPU."""
    return _depth_order(load_library(), None, depths, front_to_back, False)[1]


def _is_device_tensor(a):
    return hasattr(a, "data_ptr") and getattr(a, "is_cuda", False) is True


def _triangle_depths(L, handle, clip, group, mode, device):
    """Returns (the clip array to keep alive, depths [n / group])."""
    group = int(group)
    if device:
        if not _is_device_tensor(clip) or str(clip.dtype) != "torch.float64" or not clip.is_contiguous() or clip.numel() % 12:
            raise ValueError("device=True: clip must be a contiguous float64 device tensor [n, 12]")
        import torch
        n = clip.numel() // 12
        out = torch.empty(n // max(group, 1), dtype=torch.float64, device=clip.device)
        ptrs = (clip.data_ptr() if n else None, out.data_ptr() if out.numel() else None)
    else:
        clip = np.ascontiguousarray(clip, np.float64).reshape(-1, 12)
        n = clip.shape[0]
        out = np.empty(n // max(group, 1), np.float64)
        ptrs = (clip.ctypes.data, out.ctypes.data)
    rc = L.trgl_triangle_depths(handle, ptrs[0], n, group, int(mode), MEM_DEVICE if device else MEM_HOST, ptrs[1])
    if rc != 0:
        raise TrglError(f"trgl_triangle_depths failed ({rc}): {L.trgl_last_error(handle).decode()}")
    return clip, out


def _order_stage(L, handle, clip, varyings, colors, order, group, device, out):
    """Returns (arrays to keep alive, (clip_out, varyings_out, colors_out)) - n_order * group rows each."""
    group = int(group)
    if device:
        import torch
        for a, what in ((clip, "clip"), (varyings, "varyings")):
            if a is not None and (not _is_device_tensor(a) or str(a.dtype) != "torch.float64" or not a.is_contiguous() or a.dim() != 2):
                raise ValueError(f"device=True: {what} must be a contiguous float64 device tensor with 2 dimensions")
        for a, what in ((colors, "colors"), (order, "order")):
            if a is not None and (not _is_device_tensor(a) or a.element_size() != 4 or not a.is_contiguous() or a.dim() != 1):
                raise ValueError(f"device=True: {what} must be a contiguous 32-bit device tensor with 1 dimension")
        n, n_order = int(clip.shape[0]), int(order.shape[0])
        K = 0 if varyings is None else int(varyings.shape[1])
        rows = n_order * group
        if out is None:
            out = (torch.empty((rows, 12), dtype=torch.float64, device=clip.device),
                   None if K == 0 else torch.empty((rows, K), dtype=torch.float64, device=clip.device),
                   None if colors is None else torch.empty(rows, dtype=colors.dtype, device=clip.device))
        ptrs = (_device_ptr(clip, "clip"), _device_ptr(varyings, "varyings") if K else None, _device_ptr(colors, "colors"), _device_ptr(order, "order"))
        optrs = (_device_ptr(out[0], "clip_out"), _device_ptr(out[1], "varyings_out") if K else None, _device_ptr(out[2], "colors_out"))
    else:
        clip = np.ascontiguousarray(clip, np.float64).reshape(-1, 12)
        n = clip.shape[0]
        varyings = None if varyings is None else np.ascontiguousarray(varyings, np.float64).reshape(n, -1)
        K = 0 if varyings is None else varyings.shape[1]
        colors = None if colors is None else np.ascontiguousarray(colors, np.uint32).reshape(n)
        order = np.ascontiguousarray(order, np.uint32).reshape(-1)
        n_order = order.shape[0]
        rows = n_order * group
        if out is None:
            out = (np.empty((rows, 12), np.float64), None if K == 0 else np.empty((rows, K), np.float64),
                   None if colors is None else np.empty(rows, np.uint32))
        ptrs = (_ptr(clip), _ptr(varyings) if K else None, _ptr(colors), _ptr(order))
        optrs = (_ptr(out[0]), _ptr(out[1]) if K else None, _ptr(out[2]))
    rc = L.trgl_order_stage(handle, K, ptrs[0], ptrs[1], ptrs[2], n, ptrs[3], n_order, group, MEM_DEVICE if device else MEM_HOST,
                            optrs[0], optrs[1], optrs[2])
    if rc != 0:
        raise TrglError(f"trgl_order_stage failed ({rc}): {L.trgl_last_error(handle).decode()}")
    return (clip, varyings, colors, order), out


def triangle_depths(clip, group=1, mode=TRI_DEPTH_CENTROID) -> np.ndarray:
    """trgl_triangle_depths for a host array without a context: one depth per group of `group` consecutive triangles of clip [n, 12],
    from the clip w of the group's vertices - their sum (CENTROID), their smallest (NEAREST) or their largest (FARTHEST), negated, so
    that depth_order's default direction draws the farthest group first.  Needs no GPU."""
    return _triangle_depths(load_library(), None, clip, group, mode, False)[1]


def order_stage(clip, varyings=None, colors=None, order=(), group=1):
    """trgl_order_stage for host arrays without a context: the rows of the groups that `order` names, in that order - output group p is
    input group order[p].  Returns (clip, varyings, colors) with len(order) * group rows (None where the input is None).  Needs no GPU."""
    return _order_stage(load_library(), None, clip, varyings, colors, order, group, False, None)[1]


class SpriteParams(C.Structure):
    """trgl_sprite_params"""
    _fields_ = [("model_view", C.c_double * 16), ("projection", C.c_double * 16), ("size", C.c_double), ("scale", C.c_double * 2),
                ("mode", C.c_int32), ("size_offset", C.c_int32), ("attr_offset", C.c_int32), ("n_attr", C.c_int32)]


class LineParams(C.Structure):
    """trgl_line_params"""
    _fields_ = [("model_view", C.c_double * 16), ("projection", C.c_double * 16), ("width", C.c_double), ("half_extent", C.c_double * 2),
                ("w_min", C.c_double)]


def make_sprite_params(model_view, projection, size=1.0, scale=(0.0, 0.0), mode=SPRITE_VIEW, size_offset=-1, attr_offset=0, n_attr=0):
    """trgl_sprite_params: row-major 4x4 matrices; size is used when size_offset < 0, else the point's size is column size_offset of its
    row; scale = (2 / w, 2 / h) gives SPRITE_SCREEN sizes in pixels of a w x h viewport; n_attr columns from attr_offset on follow the
    uv pairs in the varyings of both triangles."""
    return SpriteParams((C.c_double * 16)(*_f64(model_view, 16, "model_view")), (C.c_double * 16)(*_f64(projection, 16, "projection")),
                        float(size), (C.c_double * 2)(*_f64(scale, 2, "scale")), int(mode), int(size_offset), int(attr_offset), int(n_attr))


def make_line_params(model_view, projection, width, half_extent, w_min):
    """trgl_line_params: width in the units of half_extent (pixels with half_extent = (w / 2, h / 2) of the viewport); the segment is cut
    where its clip w falls below w_min > 0."""
    return LineParams((C.c_double * 16)(*_f64(model_view, 16, "model_view")), (C.c_double * 16)(*_f64(projection, 16, "projection")),
                      float(width), (C.c_double * 2)(*_f64(half_extent, 2, "half_extent")), float(w_min))


def _quad_inputs(points, indices, colors, device):
    """(points, indices, colors) as the sprite and line calls take them, checked: device tensors with device=True, else numpy arrays."""
    if device:
        _device_f64(points, 2, "points")
        for a, what in ((indices, "indices"), (colors, "colors")):
            if a is not None and (not _is_device_tensor(a) or a.element_size() != 4 or not a.is_contiguous()):
                raise ValueError(f"device=True: {what} must be a contiguous 32-bit device tensor")
        return points, indices, colors
    points = np.ascontiguousarray(points, np.float64)
    if points.ndim != 2:
        raise ValueError("points must have 2 dimensions [n, stride]")
    return (points, None if indices is None else np.ascontiguousarray(indices, np.uint32).reshape(-1),
            None if colors is None else np.ascontiguousarray(colors, np.uint32).reshape(-1))


def _quad_outputs(points, colors, n, K, device, out):
    """(clip_out [2 n, 12], varyings_out [2 n, K], colors_out [2 n] or None) for n quads"""
    if out is not None:
        return out
    if device:
        import torch
        return (torch.empty((2 * n, 12), dtype=torch.float64, device=points.device), torch.empty((2 * n, K), dtype=torch.float64, device=points.device),
                None if colors is None else torch.empty(2 * n, dtype=colors.dtype, device=points.device))
    return np.empty((2 * n, 12), np.float64), np.empty((2 * n, K), np.float64), None if colors is None else np.empty(2 * n, np.uint32)


def _sprite_stage(L, handle, params, points, colors, device, out):
    """Returns (arrays to keep alive, (clip_out, varyings_out, colors_out)) - two rows per point."""
    points, _, colors = _quad_inputs(points, None, colors, device)
    n, stride = int(points.shape[0]), int(points.shape[1])
    if colors is not None and int(colors.shape[0]) != n:
        raise ValueError("colors: one per point")
    out = _quad_outputs(points, colors, n, 6 + max(int(params.n_attr), 0), device, out)
    p = _device_ptr if device else _ptr
    rc = L.trgl_sprite_stage(handle, C.byref(params), p(points), stride, p(colors), n, MEM_DEVICE if device else MEM_HOST,
                             p(out[0]), p(out[1]), p(out[2]))
    if rc != 0:
        raise TrglError(f"trgl_sprite_stage failed ({rc}): {L.trgl_last_error(handle).decode()}")
    return (points, colors), out


def _line_segments(points, indices, n_segments):
    if n_segments is not None:
        return int(n_segments)
    return int(points.shape[0]) // 2 if indices is None else int(indices.numel() if hasattr(indices, "numel") else indices.size) // 2


def _line_stage(L, handle, params, points, indices, colors, n_segments, device, out):
    """Returns (arrays to keep alive, (clip_out, varyings_out, colors_out)) - two rows per segment."""
    points, indices, colors = _quad_inputs(points, indices, colors, device)
    n_points, stride = int(points.shape[0]), int(points.shape[1])
    n = _line_segments(points, indices, n_segments)
    if colors is not None and int(colors.shape[0]) != n:
        raise ValueError("colors: one per segment")
    out = _quad_outputs(points, colors, n, 6, device, out)
    p = _device_ptr if device else _ptr
    rc = L.trgl_line_stage(handle, C.byref(params), p(points), stride, n_points, p(indices), p(colors), n, MEM_DEVICE if device else MEM_HOST,
                           p(out[0]), p(out[1]), p(out[2]))
    if rc != 0:
        raise TrglError(f"trgl_line_stage failed ({rc}): {L.trgl_last_error(handle).decode()}")
    return (points, indices, colors), out


def sprite_stage(params, points, colors=None):
    """trgl_sprite_stage for host arrays without a context: every point [n, stride >= 3] becomes a quad of two triangles that faces the
    camera (params: make_sprite_params).  Returns (clip [2 n, 12], varyings [2 n, 6 + n_attr], colors [2 n] or None).  Needs no GPU."""
    return _sprite_stage(load_library(), None, params, points, colors, False, None)[1]


def line_stage(params, points, indices=None, colors=None, n_segments=None):
    """trgl_line_stage for host arrays without a context: every segment - a pair of `indices` into points [n_points, stride >= 3], or
    points 2 j and 2 j + 1 - becomes a quad of params.width (params: make_line_params), cut at clip w = w_min.  Returns (clip [2 n, 12],
    varyings [2 n, 6], colors [2 n] or None).  Needs no GPU."""
    return _line_stage(load_library(), None, params, points, indices, colors, n_segments, False, None)[1]


class EdgeParams(C.Structure):
    """trgl_edge_params"""
    _fields_ = [("eye", C.c_double * 4), ("crease_cos", C.c_double), ("class_color", C.c_uint32 * 4), ("select", C.c_uint32),
                ("compact", C.c_uint32), ("reserved", C.c_uint64)]


def make_edge_params(eye, crease_cos=-2.0, select=EDGE_ANY, class_color=(0, 0, 0, 0), compact=False):
    """trgl_edge_params: eye (x, y, z, w) in model space - w = 1 a camera position, w = 0 a direction toward the viewer; an edge is a
    crease when the dot product of its faces' unit normals is below crease_cos (-2: never); select: a mask of EDGE_ANY, EDGE_BOUNDARY,
    EDGE_SILHOUETTE, EDGE_CREASE; class_color: the colour of each of the four in that order; compact: selected segments to the front."""
    return EdgeParams((C.c_double * 4)(*_f64(eye, 4, "eye")), float(crease_cos), (C.c_uint32 * 4)(*[int(x) & 0xFFFFFFFF for x in class_color]),
                      int(select), 1 if compact else 0, 0)


def _words32(a, device, what, cols=None):
    """A 32-bit array as the edge calls take it: a contiguous device tensor with device=True, else a numpy uint32 array."""
    if device:
        if not _is_device_tensor(a) or a.element_size() != 4 or not a.is_contiguous():
            raise ValueError(f"device=True: {what} must be a contiguous 32-bit device tensor")
        return a
    a = np.ascontiguousarray(a, np.uint32)
    return a if cols is None else a.reshape(-1, cols)


def _mesh_edges(L, handle, indices, n_vertices, device, out, count):
    """Returns (arrays to keep alive, edges [3 n_faces, 4], n_edges or None)."""
    indices = _words32(indices, device, "indices", 3)
    nf = int(indices.numel() if device else indices.size) // 3
    if out is None:
        if device:
            import torch
            out = torch.empty((3 * nf, 4), dtype=torch.int32, device=indices.device)
        else:
            out = np.empty((3 * nf, 4), np.uint32)
    n = C.c_uint64(0)
    p = _device_ptr if device else _ptr
    rc = L.trgl_mesh_edges(handle, p(indices) if nf else None, nf, int(n_vertices), MEM_DEVICE if device else MEM_HOST, p(out) if nf else None,
                           C.byref(n) if count else None)
    if rc != 0:
        raise TrglError(f"trgl_mesh_edges failed ({rc}): {L.trgl_last_error(handle).decode()}")
    return (indices,), out, (int(n.value) if count else None)


def _edge_select(L, handle, params, vertices, indices, edges, n_edges, device, out, count):
    """Returns (arrays to keep alive, (codes [n], segments [n, 2], colors [n]), n_selected or None); out: three arrays, each may be None
    (not written) - all three are allocated when out is None."""
    if device:
        _device_f64(vertices, 2, "vertices")
    else:
        vertices = np.ascontiguousarray(vertices, np.float64)
        if vertices.ndim != 2:
            raise ValueError("vertices must have 2 dimensions [n, stride]")
    indices = _words32(indices, device, "indices", 3)
    edges = _words32(edges, device, "edges", 4)
    nf = int(indices.numel() if device else indices.size) // 3
    n = int(edges.numel() if device else edges.size) // 4 if n_edges is None else int(n_edges)
    if out is None:
        if device:
            import torch
            out = (torch.empty(n, dtype=torch.uint8, device=vertices.device), torch.empty((n, 2), dtype=torch.int32, device=vertices.device),
                   torch.empty(n, dtype=torch.int32, device=vertices.device))
        else:
            out = (np.empty(n, np.uint8), np.empty((n, 2), np.uint32), np.empty(n, np.uint32))
    nsel = C.c_uint64(0)
    p = _device_ptr if device else _ptr
    rc = L.trgl_edge_select(handle, C.byref(params), p(vertices), int(vertices.shape[1]), int(vertices.shape[0]), p(indices), nf, p(edges), n,
                            MEM_DEVICE if device else MEM_HOST, p(out[0]), p(out[1]), p(out[2]), C.byref(nsel) if count else None)
    if rc != 0:
        raise TrglError(f"trgl_edge_select failed ({rc}): {L.trgl_last_error(handle).decode()}")
    return (vertices, indices, edges), out, (int(nsel.value) if count else None)


def mesh_edges(indices, n_vertices):
    """trgl_mesh_edges for host arrays without a context: the distinct edges of the faces indices [n_faces, 3] in ascending (lo, hi).
    Returns (edges [3 n_faces, 4] uint32 - records {lo, hi, f0, f1}, f1 = EDGE_NONE on a boundary, every word EDGE_NONE behind the last
    edge - and the number of edges).  Needs no GPU."""
    _, out, n = _mesh_edges(load_library(), None, indices, n_vertices, False, None, True)
    return out, n


def edge_select(params, vertices, indices, edges, n_edges=None):
    """trgl_edge_select for host arrays without a context: the code byte of every edge record under params (make_edge_params), the
    index pair of every selected one - what line_stage takes as indices - and its colour.  Returns (codes [n], segments [n, 2],
    colors [n], n_selected); with params.compact the selected pairs and colours come first.  Needs no GPU."""
    _, out, n = _edge_select(load_library(), None, params, vertices, indices, edges, n_edges, False, None, True)
    return out[0], out[1], out[2], n


class SubdivParams(C.Structure):
    """trgl_subdiv_params"""
    _fields_ = [("vertex_stride", C.c_int32), ("smooth", C.c_int32), ("mode", C.c_uint32), ("reserved32", C.c_uint32), ("reserved", C.c_uint64)]


def make_subdiv_params(vertex_stride, mode=SUBDIV_LOOP, smooth=3):
    """trgl_subdiv_params: records of vertex_stride doubles; mode SUBDIV_LOOP - the first `smooth` doubles of a record get the Loop
    weights, the rest midpoints and copies - or SUBDIV_LINEAR (midpoints and copies throughout; smooth is ignored)."""
    return SubdivParams(int(vertex_stride), int(smooth), int(mode), 0, 0)


def subdiv_stencil_words(n_vertices, n_edges):
    """trgl_subdiv_stencil_words: 6 * n_edges + 4 * n_vertices, the uint32 words of a stencil array"""
    return 6 * int(n_edges) + 4 * int(n_vertices)


def _subdiv_topology(L, handle, indices, n_vertices, edges, n_edges, device, out):
    """Returns (arrays to keep alive, refined indices [4 n_faces, 3], stencils [subdiv_stencil_words]); out: the two, or None."""
    indices = _words32(indices, device, "indices", 3)
    edges = _words32(edges, device, "edges", 4)
    nf = int(indices.numel() if device else indices.size) // 3
    n = int(edges.numel() if device else edges.size) // 4 if n_edges is None else int(n_edges)
    words = subdiv_stencil_words(n_vertices, n)
    if out is None:
        if device:
            import torch
            out = (torch.empty((4 * nf, 3), dtype=torch.int32, device=indices.device), torch.empty(words, dtype=torch.int32, device=indices.device))
        else:
            out = (np.empty((4 * nf, 3), np.uint32), np.empty(words, np.uint32))
    p = _device_ptr if device else _ptr
    rc = L.trgl_subdiv_topology(handle, p(indices) if nf else None, nf, int(n_vertices), p(edges) if n else None, n,
                                MEM_DEVICE if device else MEM_HOST, p(out[0]) if nf else None, p(out[1]) if words else None)
    if rc != 0:
        raise TrglError(f"trgl_subdiv_topology failed ({rc}): {L.trgl_last_error(handle).decode()}")
    return (indices, edges), out[0], out[1]


def _subdiv_inputs(vertices, stencils, n_edges, device):
    """(vertices [n, stride], stencils, n_edges): n_edges from the stencil array's size when not given"""
    if device:
        _device_f64(vertices, 2, "vertices")
    else:
        vertices = np.ascontiguousarray(vertices, np.float64)
        if vertices.ndim != 2:
            raise ValueError("vertices must have 2 dimensions [n, stride]")
    stencils = _words32(stencils, device, "stencils")
    if n_edges is None:
        words = int(stencils.numel() if device else stencils.size) - 4 * int(vertices.shape[0])
        if words < 0 or words % 6:
            raise ValueError("stencils must hold 6 * n_edges + 4 * n_vertices words")
        n_edges = words // 6
    return vertices, stencils, int(n_edges)


def _subdiv_vertices(L, handle, params, vertices, stencils, n_edges, device, out):
    """Returns (arrays to keep alive, refined vertices [n_vertices + n_edges, stride])."""
    vertices, stencils, n_edges = _subdiv_inputs(vertices, stencils, n_edges, device)
    nv, stride = int(vertices.shape[0]), int(vertices.shape[1])
    if out is None:
        if device:
            import torch
            out = torch.empty((nv + n_edges, stride), dtype=torch.float64, device=vertices.device)
        else:
            out = np.empty((nv + n_edges, stride), np.float64)
    p = _device_ptr if device else _ptr
    rc = L.trgl_subdiv_vertices(handle, C.byref(params), p(vertices), nv, p(stencils), n_edges, MEM_DEVICE if device else MEM_HOST, p(out))
    if rc != 0:
        raise TrglError(f"trgl_subdiv_vertices failed ({rc}): {L.trgl_last_error(handle).decode()}")
    return (vertices, stencils), out


def subdiv_topology(indices, n_vertices, edges, n_edges=None):
    """trgl_subdiv_topology for host arrays without a context: from the faces indices [n_faces, 3] and the records mesh_edges made for
    them - n_edges the count, or None for the whole capacity - the refined faces [4 n_faces, 3] over the vertices 0 .. n_vertices - 1
    (even) and n_vertices + e (odd, one per record), and the stencil array subdiv_vertices takes.  Needs no GPU."""
    _, refined, stencils = _subdiv_topology(load_library(), None, indices, n_vertices, edges, n_edges, False, None)
    return refined, stencils


def subdiv_vertices(params, vertices, stencils, n_edges=None):
    """trgl_subdiv_vertices for host arrays without a context: the refined vertices [n_vertices + n_edges, stride] of vertices
    [n_vertices, stride] under params (make_subdiv_params) and the stencils of subdiv_topology.  Normals are not part of the rule:
    smooth = 3 and mesh_normals on the result.  Needs no GPU."""
    return _subdiv_vertices(load_library(), None, params, vertices, stencils, n_edges, False, None)[1]


class WeldParams(C.Structure):
    """trgl_weld_params"""
    _fields_ = [("vertex_stride", C.c_int32), ("key_offset", C.c_int32), ("key_count", C.c_int32), ("reserved32", C.c_int32), ("cell", C.c_double),
                ("reserved", C.c_uint64)]


def make_weld_params(vertex_stride, key_offset=0, key_count=3, cell=0.0):
    """trgl_weld_params: records of vertex_stride doubles, compared by the key_count doubles from key_offset on - the values themselves
    (cell = 0.0: IEEE ==, so -0.0 joins +0.0 and a NaN joins nothing), or their grid cells floor(x / cell + 0.5) (a grid weld: two values
    on either side of a cell border do not join)."""
    return WeldParams(int(vertex_stride), int(key_offset), int(key_count), 0, float(cell), 0)


WELD_OUTPUTS = ("remap", "firsts", "vertices", "indices")


def _mesh_weld(L, handle, params, vertices, indices, device, out, count):
    """Returns (arrays to keep alive, dict(remap [n], firsts [n], vertices [n, stride], indices [n_faces, 3] or None), n_unique or
    None).  out: None - every output is allocated (indices only with `indices`) - or a dict naming the outputs to write, each an array
    or None to allocate it; an output that is not named is not written (NULL)."""
    if device:
        _device_f64(vertices, 2, "vertices")
    else:
        vertices = np.ascontiguousarray(vertices, np.float64)
        if vertices.ndim != 2:
            raise ValueError("vertices must have 2 dimensions [n, stride]")
    nv, stride = int(vertices.shape[0]), int(vertices.shape[1])
    nf = 0
    if indices is not None:
        indices = _words32(indices, device, "indices", 3)
        nf = int(indices.numel() if device else indices.size) // 3
    if out is None:
        out = {k: None for k in WELD_OUTPUTS if k != "indices" or indices is not None}
    unknown = set(out) - set(WELD_OUTPUTS)
    if unknown:
        raise ValueError(f"mesh_weld: unknown outputs {sorted(unknown)}")
    shapes = dict(remap=(nv,), firsts=(nv,), vertices=(nv, stride), indices=(nf, 3))
    res = {}
    for k in WELD_OUTPUTS:
        if k not in out:
            res[k] = None
        elif out[k] is not None:
            res[k] = out[k]
        elif device:
            import torch
            res[k] = torch.empty(shapes[k], dtype=torch.float64 if k == "vertices" else torch.int32, device=vertices.device)
        else:
            res[k] = np.empty(shapes[k], np.float64 if k == "vertices" else np.uint32)
    n = C.c_uint64(0)
    p = _device_ptr if device else _ptr
    rc = L.trgl_mesh_weld(handle, C.byref(params), p(vertices) if nv else None, nv, p(indices) if nf else None, nf,
                          MEM_DEVICE if device else MEM_HOST, p(res["remap"]), p(res["firsts"]), p(res["vertices"]),
                          p(res["indices"]) if nf or indices is None else None, C.byref(n) if count else None)
    if rc != 0:
        raise TrglError(f"trgl_mesh_weld failed ({rc}): {L.trgl_last_error(handle).decode()}")
    return (vertices, indices), res, (int(n.value) if count else None)


def mesh_weld(params, vertices, indices=None):
    """trgl_mesh_weld for host arrays without a context: the vertices [n, stride] whose keys (params: make_weld_params) are identical
    joined.  Returns (dict(remap [n] - the new number of every old vertex -, firsts [n] - the old number of every new vertex, EDGE_NONE
    behind the last -, vertices [n, stride] - the kept records, zeros behind the last -, indices [n_faces, 3] - `indices` renumbered, or
    None without them), n_unique).  For a triangle soup remap.reshape(-1, 3) is the index array.  Needs no GPU."""
    _, out, n = _mesh_weld(load_library(), None, params, vertices, indices, False, None, True)
    return out, n


def weld_hashes(params, vertices):
    """Test hook (trgl_debug_weld_hash): the 64-bit hash the device path of mesh_weld sorts by, per vertex of a host array."""
    L = load_library()
    vertices = np.ascontiguousarray(vertices, np.float64)
    out = np.empty(vertices.shape[0], np.uint64)
    rc = L.trgl_debug_weld_hash(C.addressof(params), _ptr(vertices), int(vertices.shape[0]), _ptr(out))
    if rc != 0:
        raise TrglError(f"trgl_debug_weld_hash failed ({rc}): {L.trgl_last_error(None).decode()}")
    return out


class CleanParams(C.Structure):
    """trgl_clean_params"""
    _fields_ = [("vertex_stride", C.c_int32), ("flags", C.c_uint32), ("fill", C.c_uint32), ("reserved32", C.c_uint32), ("reserved", C.c_uint64)]


class SimplifyParams(C.Structure):
    """trgl_simplify_params"""
    _fields_ = [("vertex_stride", C.c_int32), ("mean_count", C.c_int32), ("fill", C.c_uint32), ("reserved32", C.c_uint32), ("cell", C.c_double),
                ("reserved", C.c_uint64)]


CLEAN_DUPLICATES, CLEAN_VERTICES = 1, 2
CLEAN_FILL_NONE, CLEAN_FILL_ZERO = 0, 1


def make_clean_params(vertex_stride=0, flags=CLEAN_DUPLICATES | CLEAN_VERTICES, fill=CLEAN_FILL_NONE):
    """trgl_clean_params: flags - CLEAN_DUPLICATES drops a face whose canonical triple an earlier face has, CLEAN_VERTICES renumbers the
    vertices that kept faces name -; fill - what stands behind the kept faces in indices: CLEAN_FILL_NONE (no vertex) or CLEAN_FILL_ZERO
    (faces (0, 0, 0), which a draw drops); vertex_stride is read only when records are written."""
    return CleanParams(int(vertex_stride), int(flags), int(fill), 0, 0)


def make_simplify_params(vertex_stride, cell, mean_count=3, fill=CLEAN_FILL_NONE):
    """trgl_simplify_params: one level of vertex clustering over records of vertex_stride >= 3 doubles whose first three are the position;
    cell - the width of the grid (0: the positions themselves); the first mean_count doubles of a kept record become the mean of the
    cell's referenced members; fill as make_clean_params."""
    return SimplifyParams(int(vertex_stride), int(mean_count), int(fill), 0, float(cell), 0)


CLEAN_OUTPUTS = ("indices", "face_firsts", "vremap", "vfirsts", "vertices")
SIMPLIFY_OUTPUTS = ("remap", "firsts", "vertices", "indices", "face_firsts")


def _lod_outputs(names, out, shapes, device, like, what):
    """The outputs of a clean or simplify call: out - None for all of `names`, or a dict naming those to write, each an array or None to
    allocate it; one that is not named is not written (NULL)."""
    if out is None:
        out = {k: None for k in names}
    unknown = set(out) - set(names)
    if unknown:
        raise ValueError(f"{what}: unknown outputs {sorted(unknown)}")
    res = {}
    for k in names:
        if k not in out:
            res[k] = None
        elif out[k] is not None:
            res[k] = out[k]
        elif device:
            import torch
            res[k] = torch.empty(shapes[k], dtype=torch.float64 if k == "vertices" else torch.int32, device=like.device)
        else:
            res[k] = np.empty(shapes[k], np.float64 if k == "vertices" else np.uint32)
    return res


def _lod_vertices(vertices, device, what):
    if device:
        return _device_f64(vertices, 2, what)
    vertices = np.ascontiguousarray(vertices, np.float64)
    if vertices.ndim != 2:
        raise ValueError(f"{what} must have 2 dimensions [n, stride]")
    return vertices


def _mesh_clean(L, handle, params, indices, vertices, n_vertices, device, out, count):
    """Returns (arrays to keep alive, dict(indices [n_faces, 3], face_firsts [n_faces], vremap [n], vfirsts [n], vertices [n, stride] - the
    last three None without CLEAN_VERTICES, the last without `vertices`), (kept faces, kept vertices) or None)."""
    indices = _words32(indices, device, "indices", 3)
    nf = int(indices.numel() if device else indices.size) // 3
    stride = 0
    if vertices is not None:
        vertices = _lod_vertices(vertices, device, "mesh_clean: vertices")
        nv, stride = int(vertices.shape[0]), int(vertices.shape[1])
        if n_vertices is not None and int(n_vertices) != nv:
            raise ValueError("mesh_clean: n_vertices differs from the vertex array")
        if params.vertex_stride != stride and (params.flags & CLEAN_VERTICES):
            raise ValueError("mesh_clean: params.vertex_stride differs from the vertex array")
    elif n_vertices is None:
        raise ValueError("mesh_clean: n_vertices is needed without a vertex array")
    else:
        nv = int(n_vertices)
    names = CLEAN_OUTPUTS if params.flags & CLEAN_VERTICES else CLEAN_OUTPUTS[:2]
    if vertices is None:
        names = tuple(k for k in names if k != "vertices")
    res = _lod_outputs(names, out, dict(indices=(nf, 3), face_firsts=(nf,), vremap=(nv,), vfirsts=(nv,), vertices=(nv, stride)), device, indices, "mesh_clean")
    res.update({k: None for k in CLEAN_OUTPUTS if k not in res})
    n = (C.c_uint64 * 2)(0, 0)
    p = _device_ptr if device else _ptr
    rc = L.trgl_mesh_clean(handle, C.byref(params), p(indices) if nf else None, nf, p(vertices) if vertices is not None and nv else None, nv,
                           MEM_DEVICE if device else MEM_HOST, p(res["indices"]) if nf else None, p(res["face_firsts"]) if nf else None,
                           p(res["vremap"]), p(res["vfirsts"]), p(res["vertices"]), n if count else None)
    if rc != 0:
        raise TrglError(f"trgl_mesh_clean failed ({rc}): {L.trgl_last_error(handle).decode()}")
    return (indices, vertices), res, ((int(n[0]), int(n[1])) if count else None)


def mesh_clean(params, indices, vertices=None, n_vertices=None):
    """trgl_mesh_clean for host arrays without a context: the faces [n_faces, 3] that draw nothing - two equal indices; with
    CLEAN_DUPLICATES the canonical triple of an earlier face - dropped, the kept ones in their order; with CLEAN_VERTICES the vertices they
    name renumbered in ascending old number.  Returns (dict(indices [n_faces, 3] - the fill behind the kept faces -, face_firsts [n_faces]
    - the old number of every kept face, EDGE_NONE behind -, vremap [n], vfirsts [n], vertices [n, stride] as mesh_weld's remap, firsts and
    vertices), (kept faces, kept vertices)).  Without `vertices` pass n_vertices.  Needs no GPU."""
    _, out, n = _mesh_clean(load_library(), None, params, indices, vertices, n_vertices, False, None, True)
    return out, n


def _mesh_simplify(L, handle, params, vertices, indices, device, out, count):
    """Returns (arrays to keep alive, dict(remap [n], firsts [n], vertices [n, stride], indices [n_faces, 3], face_firsts [n_faces]),
    (kept faces, kept vertices) or None)."""
    vertices = _lod_vertices(vertices, device, "mesh_simplify: vertices")
    nv, stride = int(vertices.shape[0]), int(vertices.shape[1])
    indices = _words32(indices, device, "indices", 3)
    nf = int(indices.numel() if device else indices.size) // 3
    res = _lod_outputs(SIMPLIFY_OUTPUTS, out, dict(remap=(nv,), firsts=(nv,), vertices=(nv, stride), indices=(nf, 3), face_firsts=(nf,)), device, vertices,
                       "mesh_simplify")
    n = (C.c_uint64 * 2)(0, 0)
    p = _device_ptr if device else _ptr
    rc = L.trgl_mesh_simplify(handle, C.byref(params), p(vertices) if nv else None, nv, p(indices) if nf else None, nf, MEM_DEVICE if device else MEM_HOST,
                              p(res["remap"]), p(res["firsts"]), p(res["vertices"]), p(res["indices"]) if nf else None,
                              p(res["face_firsts"]) if nf else None, n if count else None)
    if rc != 0:
        raise TrglError(f"trgl_mesh_simplify failed ({rc}): {L.trgl_last_error(handle).decode()}")
    return (vertices, indices), res, ((int(n[0]), int(n[1])) if count else None)


def mesh_simplify(params, vertices, indices):
    """trgl_mesh_simplify for host arrays without a context: one level of vertex clustering - a grid weld by position (params:
    make_simplify_params), the mean of every cell's referenced members, then mesh_clean with both flags.  Returns (dict(remap [n] - the new
    number of every old vertex, EDGE_NONE when its cluster left -, firsts [n] - the lowest old vertex of every new one -, vertices
    [n, stride], indices [n_faces, 3], face_firsts [n_faces]), (kept faces, kept vertices)).  Needs no GPU."""
    _, out, n = _mesh_simplify(load_library(), None, params, vertices, indices, False, None, True)
    return out, n


def lod_face_hashes(indices, n_vertices):
    """Test hook (trgl_debug_lod_face_hash): the 64-bit value the device path of mesh_clean sorts every face of a host array by."""
    L = load_library()
    indices = np.ascontiguousarray(indices, np.uint32).reshape(-1, 3)
    out = np.empty(indices.shape[0], np.uint64)
    rc = L.trgl_debug_lod_face_hash(_ptr(indices), int(indices.shape[0]), int(n_vertices), _ptr(out))
    if rc != 0:
        raise TrglError(f"trgl_debug_lod_face_hash failed ({rc}): {L.trgl_last_error(None).decode()}")
    return out


class SkinParams(C.Structure):
    """trgl_skin_params"""
    _fields_ = [("vertex_stride", C.c_int32), ("n_influences", C.c_int32), ("n_joints", C.c_uint32), ("flags", C.c_uint32),
                ("n_poses", C.c_uint64), ("palette_stride", C.c_uint64), ("reserved", C.c_uint64)]


def _skin_inputs(vertices, joints, weights, palette, device):
    """(vertices [n, stride], joints [n, k] uint16, weights [n, k], palette [n_poses, n_joints, 16] or [n_joints, 16]) as the skinning
    calls take them, checked: device tensors with device=True, else numpy arrays."""
    if device:
        _device_f64(vertices, 2, "vertices"); _device_f64(weights, 2, "weights")
        if not _is_device_tensor(palette) or str(palette.dtype) != "torch.float64" or palette.dim() not in (2, 3) or palette.stride(-1) != 1 or \
                palette.stride(-2) != 16 or int(palette.shape[-1]) != 16:
            raise ValueError("device=True: palette must be a float64 device tensor [n_poses, n_joints, 16] or [n_joints, 16] with packed matrices")
        if not _is_device_tensor(joints) or joints.element_size() != 2 or not joints.is_contiguous() or joints.dim() != 2:
            raise ValueError("device=True: joints must be a contiguous 16-bit device tensor [n, n_influences]")
    else:
        vertices = np.ascontiguousarray(vertices, np.float64)
        joints = np.ascontiguousarray(joints, np.uint16)
        weights = np.ascontiguousarray(weights, np.float64)
        palette = np.asarray(palette, np.float64)
        # (poses may lie further apart than a palette is long - palette_stride -, the matrices of one pose are packed)
        if palette.ndim != 3 or palette.strides[1:] != (128, 8) or palette.strides[0] % 8 or palette.strides[0] < 128 * palette.shape[1]:
            palette = np.ascontiguousarray(palette)
        if vertices.ndim != 2 or joints.ndim != 2 or weights.ndim != 2 or palette.ndim not in (2, 3) or palette.shape[-1] != 16:
            raise ValueError("vertices [n, stride], joints and weights [n, n_influences], palette [n_poses, n_joints, 16] or [n_joints, 16]")
    if tuple(joints.shape) != tuple(weights.shape) or int(joints.shape[0]) != int(vertices.shape[0]):
        raise ValueError("joints and weights: one row of n_influences per vertex")
    return vertices, joints, weights, palette


def _skin_params(vertices, joints, palette, flags):
    """trgl_skin_params of checked arrays; a 3-dimensional palette's first stride is the palette_stride."""
    poses = int(palette.shape[0]) if len(palette.shape) == 3 else 1
    if len(palette.shape) == 3 and poses > 1:
        pstride = int(palette.stride(0)) if hasattr(palette, "data_ptr") else int(palette.strides[0]) // 8
    else:
        pstride = 0
    return SkinParams(int(vertices.shape[1]), int(joints.shape[1]), int(palette.shape[-2]), int(flags), poses, pstride, 0)


def _skin_stage(L, handle, vertices, joints, weights, palette, flags, device, out):
    """Returns (arrays to keep alive, out [n_poses, n, stride])."""
    vertices, joints, weights, palette = _skin_inputs(vertices, joints, weights, palette, device)
    P = _skin_params(vertices, joints, palette, flags)
    n, stride = int(vertices.shape[0]), int(vertices.shape[1])
    if out is None:
        if device:
            import torch
            out = torch.empty((int(P.n_poses), n, stride), dtype=torch.float64, device=vertices.device)
        else:
            out = np.empty((int(P.n_poses), n, stride), np.float64)
    p = _device_ptr if device else _ptr
    rc = L.trgl_skin_stage(handle, C.byref(P), p(vertices), n, p(joints), p(weights), p(palette), MEM_DEVICE if device else MEM_HOST, p(out))
    if rc != 0:
        raise TrglError(f"trgl_skin_stage failed ({rc}): {L.trgl_last_error(handle).decode()}")
    return (vertices, joints, weights, palette), out


def _pose_palette(L, handle, parents, local, inverse_bind, device, out):
    """Returns (arrays to keep alive, palette [n_poses, n_joints, 16]); local: [n_poses, n_joints, 16]."""
    if device:
        _device_f64(local, 3, "local")
        if inverse_bind is not None:
            _device_f64(inverse_bind, 2, "inverse_bind")
        if not _is_device_tensor(parents) or parents.element_size() != 4 or not parents.is_contiguous():
            raise ValueError("device=True: parents must be a contiguous 32-bit device tensor")
    else:
        local = np.ascontiguousarray(local, np.float64)
        parents = np.ascontiguousarray(parents, np.int32).reshape(-1)
        inverse_bind = None if inverse_bind is None else np.ascontiguousarray(inverse_bind, np.float64)
        if local.ndim != 3:
            raise ValueError("local must be [n_poses, n_joints, 16]")
    poses, nj = int(local.shape[0]), int(local.shape[1])
    if int(local.shape[2]) != 16 or int(parents.shape[0]) != nj or (inverse_bind is not None and tuple(inverse_bind.shape) != (nj, 16)):
        raise ValueError("local [n_poses, n_joints, 16], parents [n_joints], inverse_bind [n_joints, 16] or None")
    if out is None:
        if device:
            import torch
            out = torch.empty((poses, nj, 16), dtype=torch.float64, device=local.device)
        else:
            out = np.empty((poses, nj, 16), np.float64)
    if device:
        pstride = int(out.stride(0)) if poses > 1 else 16 * nj
    else:
        pstride = int(out.strides[0]) // 8 if poses > 1 else 16 * nj
    p = _device_ptr if device else _ptr
    rc = L.trgl_pose_palette(handle, p(parents), p(inverse_bind), nj, p(local), 16 * nj, poses, MEM_DEVICE if device else MEM_HOST, p(out), pstride)
    if rc != 0:
        raise TrglError(f"trgl_pose_palette failed ({rc}): {L.trgl_last_error(handle).decode()}")
    return (parents, local, inverse_bind), out


def skin_stage(vertices, joints, weights, palette, flags=0):
    """trgl_skin_stage for host arrays without a context: linear blend skinning of vertices [n, stride >= 3] (the reference's Vertex
    layout) by joints [n, k] (uint16) and weights [n, k], k = 1 .. 8, under palette [n_poses, n_joints, 16] (or [n_joints, 16]: one pose)
    of row-major matrices; flags: SKIN_NORMAL | SKIN_TANGENT | SKIN_BITANGENT.  Returns [n_poses, n, stride].  Needs no GPU."""
    return _skin_stage(load_library(), None, vertices, joints, weights, palette, flags, False, None)[1]


def pose_palette(parents, local, inverse_bind=None):
    """trgl_pose_palette for host arrays without a context: local [n_poses, n_joints, 16] joint matrices composed along parents
    [n_joints] (-1: a root; else a joint below) and multiplied by inverse_bind [n_joints, 16] when given.  Returns the palettes
    [n_poses, n_joints, 16].  Needs no GPU."""
    return _pose_palette(load_library(), None, parents, local, inverse_bind, False, None)[1]


def _device_f64(t, ndim, what):
    if not _is_device_tensor(t) or str(t.dtype) != "torch.float64" or not t.is_contiguous() or t.dim() != ndim:
        raise ValueError(f"{what} must be a contiguous float64 device tensor with {ndim} dimensions (the other arrays are in device memory)")
    return t


def _instance_boxes(L, handle, local, instances, out):
    """Returns (arrays to keep alive, boxes [n, 6]).  Device memory when `instances` is a device tensor."""
    device = _is_device_tensor(instances)
    one = not _is_device_tensor(local) and np.ndim(local) == 1          # one local box for every instance: always host memory
    if device:
        _device_f64(instances, 2, "instance_boxes: instances")
        if not one:
            _device_f64(local, 2, "instance_boxes: local")
    else:
        instances = np.ascontiguousarray(instances, np.float64)
        if instances.ndim != 2:
            raise ValueError("instance_boxes: instances must be [n, stride]")
        if not one:
            local = np.ascontiguousarray(local, np.float64)
    n = int(instances.shape[0])
    if one:
        local, local_stride = _f64(local, 6, "instance_boxes: local"), 0
        lptr = local.ctypes.data
    else:
        if len(local.shape) != 2 or int(local.shape[0]) != n:
            raise ValueError("instance_boxes: local must be [6] (one box for every instance) or [n, stride >= 6]")
        local_stride = int(local.shape[1])
        if local_stride == 0:
            raise ValueError("instance_boxes: a strided local array needs stride >= 6")
        lptr = _device_ptr(local, "local") if device else local.ctypes.data
    if out is None:
        if device:
            import torch
            out = torch.empty((n, 6), dtype=torch.float64, device=instances.device)
        else:
            out = np.empty((n, 6), np.float64)
    else:
        if device:
            _device_f64(out, 2, "instance_boxes: out")
        elif not (isinstance(out, np.ndarray) and out.dtype == np.float64 and out.flags.c_contiguous):
            raise ValueError("instance_boxes: out must be a contiguous float64 numpy array (the other arrays are in host memory)")
        if tuple(out.shape) != (n, 6):
            raise ValueError("instance_boxes: out must be [n, 6]")
    iptr, optr = (_device_ptr(instances, "instances"), _device_ptr(out, "out")) if device else (instances.ctypes.data, out.ctypes.data)
    if n == 0:
        iptr = optr = None
        lptr = lptr if one else None
    rc = L.trgl_instance_boxes(handle, lptr, local_stride, iptr, int(instances.shape[1]), n, MEM_DEVICE if device else MEM_HOST, optr)
    if rc != 0:
        raise TrglError(f"trgl_instance_boxes failed ({rc}): {L.trgl_last_error(handle).decode()}")
    return (local, instances, out), out


def _frustum_boxes(L, handle, planes, boxes, codes, merge):
    """Returns (arrays to keep alive, codes [n] uint8).  Device memory when `boxes` is a device tensor."""
    planes = _f64(planes, 24, "frustum_boxes: planes")
    device = _is_device_tensor(boxes)
    if device:
        _device_f64(boxes, 2, "frustum_boxes: boxes")
    else:
        boxes = np.ascontiguousarray(boxes, np.float64)
    n = _boxes_count(boxes)
    if codes is None:
        if merge:
            raise ValueError("frustum_boxes: merge=True needs the codes to merge into")
        if device:
            import torch
            codes = torch.empty(n, dtype=torch.uint8, device=boxes.device)
        else:
            codes = np.empty(n, np.uint8)
    else:
        if device:
            if not _is_device_tensor(codes) or str(codes.dtype) != "torch.uint8" or not codes.is_contiguous():
                raise ValueError("frustum_boxes: codes must be a contiguous uint8 device tensor (the boxes are in device memory)")
        elif not (isinstance(codes, np.ndarray) and codes.dtype == np.uint8 and codes.flags.c_contiguous and codes.flags.writeable):
            raise ValueError("frustum_boxes: codes must be a contiguous writable uint8 numpy array (the boxes are in host memory)")
        if tuple(codes.shape) != (n,):
            raise ValueError("frustum_boxes: codes must be [n]")
    bptr, cptr = (_device_ptr(boxes, "boxes"), _device_ptr(codes, "codes")) if device else (boxes.ctypes.data, codes.ctypes.data)
    if n == 0:
        bptr = cptr = None
    rc = L.trgl_frustum_boxes(handle, _dp(planes), bptr, n, FRUSTUM_MERGE if merge else FRUSTUM_SET, MEM_DEVICE if device else MEM_HOST, cptr)
    if rc != 0:
        raise TrglError(f"trgl_frustum_boxes failed ({rc}): {L.trgl_last_error(handle).decode()}")
    return (boxes, codes), codes


def instance_boxes(local, instances, out=None) -> np.ndarray:
    """trgl_instance_boxes for host arrays without a context: the world box [n, 6] = (min.xyz, max.xyz) of every instance [n, stride >= 16]
    - AABB::transform (geometry.h:297-327) of `local` under the instance's row-major matrix, bit for bit trgl_aabb_transform.  local: [6],
    one box for every instance (mesh_bounds' two halves concatenated), or [n, stride >= 6], one per instance.  Needs no GPU."""
    if _is_device_tensor(instances):
        raise TypeError("instance_boxes: device tensors need a context (Context.instance_boxes)")
    return _instance_boxes(load_library(), None, local, instances, out)[1]


def frustum_boxes(planes, boxes, codes=None, merge=False) -> np.ndarray:
    """trgl_frustum_boxes for host arrays without a context: one code byte per box [n, 6] from Frustum::intersects (our_gl.cpp:264-280)
    against planes [6, 4] (frustum_from_matrix).  merge=False: OCCL_VISIBLE or OCCL_OUTSIDE, into `codes` or a new array.  merge=True:
    `codes` (uint8 [n], occlusion codes for instance) is changed in place - OCCL_OUTSIDE where the frustum culls, untouched elsewhere.
    Needs no GPU."""
    if _is_device_tensor(boxes):
        raise TypeError("frustum_boxes: device tensors need a context (Context.frustum_boxes)")
    return _frustum_boxes(load_library(), None, planes, boxes, codes, merge)[1]


def clip_layout(kind: int):
    """trgl_clip_layout: the built-in clip attribute layout of a built-in kind as a list of (offset, components).  Needs no GPU."""
    L = load_library()
    attrs, n = (ClipAttr * MAX_CLIP_ATTRS)(), C.c_int(0)
    rc = L.trgl_clip_layout(int(kind), attrs, C.byref(n))
    if rc != 0:
        raise TrglError(f"trgl_clip_layout failed ({rc}): {L.trgl_last_error(None).decode()}")
    return [(attrs[i].offset, attrs[i].components) for i in range(n.value)]


def _clip_attrs(attrs):
    """(ctypes array or None, count) of a list of (offset, components); None stands for the kind's built-in layout (-1)."""
    if attrs is None:
        return None, -1
    attrs = [(int(o), int(k)) for o, k in attrs]
    arr = (ClipAttr * max(len(attrs), 1))()
    for i, (o, k) in enumerate(attrs):
        arr[i].offset, arr[i].components = o, k
    return arr, len(attrs)


def _clip_stage(L, handle, plane, attrs, K, ptrs, n, optrs, device):
    arr, na = _clip_attrs([] if attrs is None else attrs)
    n_out = C.c_uint64(0)
    rc = L.trgl_clip_stage(handle, _dp(_f64(plane, 4, "plane")), arr, na, int(K), ptrs[0], ptrs[1], ptrs[2], int(n),
                           optrs[0], optrs[1], optrs[2], C.byref(n_out), MEM_DEVICE if device else MEM_HOST)
    if rc != 0:
        raise TrglError(f"trgl_clip_stage failed ({rc}): {L.trgl_last_error(handle).decode()}")
    return int(n_out.value)


def _host_clip_stage(L, handle, plane, attrs, clip, varyings, colors):
    clip = np.ascontiguousarray(clip, np.float64).reshape(-1, 12)
    n = clip.shape[0]
    vary = None if varyings is None else np.ascontiguousarray(varyings, np.float64).reshape(n, np.shape(varyings)[-1] if np.ndim(varyings) == 2 else -1)
    K = 0 if vary is None else vary.shape[1]
    col = None if colors is None else np.ascontiguousarray(colors, np.uint32).reshape(n)
    oclip, ovary = np.empty((2 * n, 12), np.float64), np.empty((2 * n, K), np.float64)
    ocol = None if col is None else np.empty(2 * n, np.uint32)
    m = _clip_stage(L, handle, plane, attrs, K, (_ptr(clip), _ptr(vary) if K else None, _ptr(col)), n,
                    (_ptr(oclip), _ptr(ovary) if K else None, _ptr(ocol)), False)
    return oclip[:m].copy(), (ovary[:m].copy() if K else None), (None if ocol is None else ocol[:m].copy())


def clip_stage(plane, clip, varyings=None, colors=None, attrs=None):
    """trgl_clip_stage for host arrays without a context (include/trgl.h writes the operation down): clip [n, 12], varyings [n, K] or
    None, colors [n] or None, attrs a list of (offset, components) (None: no attributes, every varying is a per-triangle constant).
    Returns (clip, varyings, colors) of the output triangles.  Needs no GPU."""
    return _host_clip_stage(load_library(), None, plane, attrs, clip, varyings, colors)


def aabb_transform(bmin, bmax, m):
    """trgl_aabb_transform: AABB::transform (geometry.h:297-327) of the box by the row-major 4x4 m; returns (min[3], max[3])."""
    lo, hi = np.empty(3, np.float64), np.empty(3, np.float64)
    rc = load_library().trgl_aabb_transform(_dp(_f64(bmin, 3, "bmin")), _dp(_f64(bmax, 3, "bmax")), _dp(_f64(m, 16, "m")), _dp(lo), _dp(hi))
    if rc != 0:
        raise TrglError(f"trgl_aabb_transform failed ({rc})")
    return lo, hi


def frustum_from_matrix(m):
    """trgl_frustum_from_matrix: Frustum::createFromMatrix (our_gl.cpp:212-262); returns planes [6, 4] = nx, ny, nz, d in the order
    FRUSTUM_LEFT .. FRUSTUM_FAR."""
    planes = np.empty((6, 4), np.float64)
    rc = load_library().trgl_frustum_from_matrix(_dp(_f64(m, 16, "m")), _dp(planes))
    if rc != 0:
        raise TrglError(f"trgl_frustum_from_matrix failed ({rc})")
    return planes


def frustum_intersects(planes, bmin, bmax) -> bool:
    """trgl_frustum_intersects: Frustum::intersects (our_gl.cpp:264-280)."""
    rc = load_library().trgl_frustum_intersects(_dp(_f64(planes, 24, "planes")), _dp(_f64(bmin, 3, "bmin")), _dp(_f64(bmax, 3, "bmax")))
    if rc < 0:
        raise TrglError(f"trgl_frustum_intersects failed ({rc})")
    return rc == 1


def tga_encode(img, vflip: bool = True, rle: bool = True) -> bytes:
    """The bytes the reference's TGAImage::write_tga_file would write for an [h,w,bpp] uint8 image (host only)."""
    L = load_library()
    img = np.ascontiguousarray(img, np.uint8)
    if img.ndim == 2:
        img = img[..., None]
    h, w, bpp = img.shape
    out = np.empty(L.trgl_tga_max_size(w, h, bpp), np.uint8)
    n = C.c_size_t()
    rc = L.trgl_tga_encode(img.ctypes.data, w, h, bpp, int(vflip), int(rle), out.ctypes.data, C.byref(n))
    if rc != 0:
        raise TrglError(f"trgl_tga_encode failed ({rc})")
    return out[:n.value].tobytes()


def tga_decode(file_bytes: bytes):
    """TGAImage::read_tga_file on a .tga file image: [h,w,bpp] uint8 in TGAImage::buffer() order (host only).
    Raises TrglError where the reference returns false."""
    L = load_library()
    buf = np.frombuffer(file_bytes, np.uint8)
    w, h, bpp = C.c_int(), C.c_int(), C.c_int()
    rc = L.trgl_tga_info(buf.ctypes.data if len(buf) else None, len(buf), C.byref(w), C.byref(h), C.byref(bpp))
    if rc != 0:
        raise TrglError(f"trgl_tga_info: not a TGA file the reference reads ({rc})")
    out = np.empty((h.value, w.value, bpp.value), np.uint8)
    rc = L.trgl_tga_decode(buf.ctypes.data, len(buf), out.ctypes.data)
    if rc != 0:
        raise TrglError(f"trgl_tga_decode failed ({rc})")
    return out


def load_obj(path: str):
    """Wavefront OBJ -> (vertices [nv,14] f64 in the reference's Vertex layout, indices [nf,3] u32).  Host only."""
    L = load_library()
    v, i = C.POINTER(C.c_double)(), C.POINTER(C.c_uint32)()
    nv, nf = C.c_uint64(), C.c_uint64()
    rc = L.trgl_obj_load(path.encode(), C.byref(v), C.byref(nv), C.byref(i), C.byref(nf))
    if rc != 0:
        raise TrglError(f"trgl_obj_load failed ({rc}): {L.trgl_last_error(None).decode()}")
    try:
        verts = np.ctypeslib.as_array(v, shape=(nv.value, 14)).copy() if nv.value else np.zeros((0, 14))
        idx = np.ctypeslib.as_array(i, shape=(nf.value, 3)).copy() if nf.value else np.zeros((0, 3), np.uint32)
    finally:
        L.trgl_obj_free(v, i)
    return verts, idx


class Context:
    """One rasterizer context on one GPU — the reference's globals (Viewport, zbuffer, counters,
    our_gl.cpp:12-22) plus the framebuffer TGAImage, as an object."""

    def __init__(self, width: int, height: int, bpp: int = 3, device: int = 0):
        self.L = load_library()
        self.h = C.c_void_p()
        rc = self.L.trgl_create(device, width, height, bpp, C.byref(self.h))
        if rc != 0:
            raise TrglError(f"trgl_create failed ({rc}): {self.L.trgl_last_error(None).decode()}")
        self.width, self.height, self.bpp, self.device = width, height, bpp, device
        self._keep = []
        self._user_vary = {}        # kind -> K of the user shaders registered here
        self._vertex_vary = {}      # vertex shader -> K of the user vertex shaders registered here

    def _chk(self, rc):
        if rc != 0:
            raise TrglError(f"trgl call failed ({rc}): {self.L.trgl_last_error(self.h).decode()}")

    def close(self):
        if self.h:
            self.L.trgl_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- state ----
    def set_viewport(self, m):
        m = np.ascontiguousarray(m, np.float64).reshape(16)
        self._chk(self.L.trgl_set_viewport(self.h, m.ctypes.data_as(C.POINTER(C.c_double))))

    def init_viewport(self, x, y, w, h):
        self._chk(self.L.trgl_init_viewport(self.h, x, y, w, h))

    def clear(self, bgra=None, z=np.inf):
        b = None if bgra is None else np.asarray(bgra, np.uint8)
        self._chk(self.L.trgl_clear(self.h, None if b is None else b.ctypes.data, float(z)))

    def upload_texture(self, slot, texels):
        t = np.ascontiguousarray(texels, np.uint8)
        if t.ndim == 2:
            t = t[..., None]
        self._chk(self.L.trgl_upload_texture(self.h, slot, t.ctypes.data, t.shape[1], t.shape[0], t.shape[2]))

    def set_strip(self, y0, y1):
        self._chk(self.L.trgl_set_strip(self.h, y0, y1))

    def set_interleave(self, band_rows, rank, world):
        """Own the bands of `band_rows` rows whose number is `rank` modulo `world` (instead of one strip)."""
        self._chk(self.L.trgl_set_interleave(self.h, band_rows, rank, world))

    def gather(self, comm, rank, world, with_z=False):
        """trgl_gather: join the rows of the `world` contexts of a render into this context's framebuffer (and z-buffer) with
        in-place RCCL all-gathers queued on the context's stream; `comm` is an ncclComm_t (rccl_comm_create)."""
        self._chk(self.L.trgl_gather(self.h, comm, rank, world, int(bool(with_z))))

    # ---- submission ----
    def register_shader(self, source: str, n_varyings: int, may_discard: bool = False, *, reads_dest: bool = False,
                        depth_write: bool = True) -> int:
        """trgl_register_shader_ex: compile (or take from the process cache) a user shader and load it on this context; returns its
        kind, for draw() with n x n_varyings varyings.  may_discard: its trgl_fragment returns trgl_frag_out and runs for every
        z-pass in order (TRGL_SHADER_MAY_DISCARD).  With it, reads_dest: in.dst is the pixel the fragment is drawn over
        (TRGL_SHADER_READS_DEST); depth_write=False: a drawn fragment leaves the depth alone (TRGL_SHADER_NO_DEPTH_WRITE)."""
        kind = C.c_int(-1)
        self._chk(self.L.trgl_register_shader_ex(self.h, source.encode(), int(n_varyings),
                                                  shader_flags(may_discard, reads_dest, depth_write), C.byref(kind)))
        self._user_vary[kind.value] = int(n_varyings)
        return kind.value

    def draw(self, kind, clip, varyings=None, colors=None, uniforms=None, n=None, device=False, clip_plane=None, clip_attrs=None,
             order=None, order_device=False, group=1):
        """order: a list of groups of `group` consecutive triangles - the groups it names are drawn, in its order (trgl_draw_ordered; no
        wait).  A numpy array, or with order_device=True a 32-bit integer device tensor such as Context.depth_order(device=True) returns;
        device arrays of such a draw are read when the call's gather runs on the stream, not at the flush.  Not with clip_plane.
        clip_plane: four doubles - the list is cut against that plane first (trgl_draw_clipped; the call waits for the stream once, for
        the count of output triangles), with clip_attrs a list of (offset, components) or None for the kind's built-in layout.
        Host arrays (numpy) are copied before return; with device=True pass torch CUDA tensors (or raw
        pointers with n) that stay alive until the flush has completed: every array of such a draw, a host array
        among them is a TypeError (_device_ptr).  include/trgl.h, TRGL_MEM_DEVICE: alignment and stream ordering."""
        # (a kind in the user range that was not registered here goes to the library, which refuses it)
        K = self._user_vary.get(kind, 0) if kind >= SHADER_USER_FIRST else VARY[kind]
        if not device:
            clip = np.ascontiguousarray(clip, np.float64)
            n = clip.shape[0] if n is None else n
            if K:
                varyings = np.ascontiguousarray(varyings, np.float64)
                assert varyings.shape == (n, K), varyings.shape
            if colors is not None:
                colors = np.ascontiguousarray(colors, np.uint32)
                assert colors.shape == (n,)
            ptrs = (_ptr(clip), _ptr(varyings) if K else None, _ptr(colors))
        else:
            ptrs = (_device_ptr(clip, "clip"), _device_ptr(varyings, "varyings"), _device_ptr(colors, "colors"))
            if not K:
                ptrs = (ptrs[0], None, ptrs[2])
            assert n is not None or hasattr(clip, "shape")
            n = clip.shape[0] if n is None else n
            self._keep.append((clip, varyings, colors))
        if order is not None:
            assert clip_plane is None and clip_attrs is None, "order=: not with clip_plane="
            oargs, _, keep = self._order_args(order, order_device)
            if order_device:
                self._keep.append(keep)
            self._chk(self.L.trgl_draw_ordered(self.h, kind, None if uniforms is None else C.byref(uniforms), ptrs[0], ptrs[1], ptrs[2], int(n),
                                               MEM_DEVICE if device else MEM_HOST, oargs[0], oargs[1], int(group), oargs[2]))
            return
        if clip_plane is not None:
            arr, na = _clip_attrs(clip_attrs)
            self._chk(self.L.trgl_draw_clipped(self.h, kind, None if uniforms is None else C.byref(uniforms), _dp(_f64(clip_plane, 4, "clip_plane")),
                                               arr, na, ptrs[0], ptrs[1], ptrs[2], int(n), MEM_DEVICE if device else MEM_HOST))
            return
        assert clip_attrs is None, "clip_attrs: only with clip_plane="
        self._chk(self.L.trgl_draw(self.h, kind, None if uniforms is None else C.byref(uniforms), ptrs[0], ptrs[1], ptrs[2], int(n),
                                   MEM_DEVICE if device else MEM_HOST))

    def clip_stage(self, plane, clip, varyings=None, colors=None, attrs=None, device=False, out=None):
        """trgl_clip_stage.  Host arrays: as the module's clip_stage.  device=True: clip [n, 12] f64, varyings [n, K] f64 or None and
        colors [n] (32-bit) or None are device tensors, out = (clip_out, varyings_out, colors_out) device tensors with room for 2 n
        triangles (allocated with torch when not given); the stage runs on the context's stream and the call waits for the count.
        Returns (clip_out, varyings_out, colors_out, n_out) - only the first n_out triangles of the outputs were written."""
        if not device:
            return _host_clip_stage(self.L, self.h, plane, attrs, clip, varyings, colors)
        n = int(clip.shape[0])
        K = 0 if varyings is None else int(varyings.shape[1])
        if out is None:
            import torch
            out = (torch.empty((2 * n, 12), dtype=torch.float64, device=clip.device),
                   None if varyings is None else torch.empty((2 * n, K), dtype=torch.float64, device=clip.device),
                   None if colors is None else torch.empty(2 * n, dtype=colors.dtype, device=clip.device))
        ptrs = (_device_ptr(clip, "clip"), _device_ptr(varyings, "varyings"), _device_ptr(colors, "colors"))
        optrs = (_device_ptr(out[0], "clip_out"), _device_ptr(out[1], "varyings_out"), _device_ptr(out[2], "colors_out"))
        m = _clip_stage(self.L, self.h, plane, attrs, K, ptrs, n, optrs, True)
        return out[0], out[1], out[2], m

    def register_vertex_shader(self, source: str, n_varyings: int) -> int:
        """trgl_register_vertex_shader: compile (or take from the process cache) a user vertex shader and load it on this context;
        returns its number (from 0, apart from the fragment kinds), for draw_indexed(vertex_shader=) and vertex_stage()."""
        vs = C.c_int(-1)
        self._chk(self.L.trgl_register_vertex_shader(self.h, source.encode(), int(n_varyings), C.byref(vs)))
        self._vertex_vary[vs.value] = int(n_varyings)
        return vs.value

    def _mesh_ptrs(self, vertices, indices, colors, device):
        """The arrays of an indexed mesh as (vertices, indices, colors, their three addresses): host arrays made contiguous, device
        arrays checked by _device_ptr before anything reaches the library."""
        if not device:
            vertices = np.ascontiguousarray(vertices, np.float64)
            indices = np.ascontiguousarray(indices, np.uint32).reshape(-1, 3)
            if colors is not None:
                colors = np.ascontiguousarray(colors, np.uint32)
                assert colors.shape == (indices.shape[0],), colors.shape
            return vertices, indices, colors, (_ptr(vertices), _ptr(indices), _ptr(colors))
        return vertices, indices, colors, (_device_ptr(vertices, "vertices"), _device_ptr(indices, "indices"), _device_ptr(colors, "colors"))

    def draw_indexed(self, kind, uniforms, projection, vertices, indices, device=False, vertex_shader=None, colors=None,
                     clip_plane=None, clip_attrs=None):
        """clip_plane / clip_attrs: as for draw() - the faces are cut between the vertex stage and the draw (trgl_draw_indexed_vs_clipped).
        Vertex stage on the device (main.cpp:71-90) + draw.  vertices [nv, stride>=8] f64, indices [nf,3] u32.
        vertex_shader: a number from register_vertex_shader - its trgl_vertex runs in place of the built-in stage
        (trgl_draw_indexed_vs): any `kind` with the vertex shader's K, vertices [nv, stride>=1] in the layout the shader reads,
        uniforms None where draw() allows it, colors [nf] u32 per face or None."""
        pj = np.ascontiguousarray(projection, np.float64).reshape(16)
        if clip_plane is not None:
            assert vertex_shader is not None or colors is None, "colors: only with vertex_shader="
            vertices, indices, colors, ptrs = self._mesh_ptrs(vertices, indices, colors, device)
            if device:
                self._keep.append((vertices, indices, colors))
            arr, na = _clip_attrs(clip_attrs)
            self._chk(self.L.trgl_draw_indexed_vs_clipped(
                self.h, -1 if vertex_shader is None else int(vertex_shader), kind, None if uniforms is None else C.byref(uniforms), _dp(pj),
                _dp(_f64(clip_plane, 4, "clip_plane")), arr, na, ptrs[0], vertices.shape[1], vertices.shape[0], ptrs[1], indices.shape[0], ptrs[2],
                MEM_DEVICE if device else MEM_HOST))
            return
        assert clip_attrs is None, "clip_attrs: only with clip_plane="
        if vertex_shader is not None:
            vertices, indices, colors, ptrs = self._mesh_ptrs(vertices, indices, colors, device)
            if device:
                self._keep.append((vertices, indices, colors))
            nv, stride = vertices.shape
            nf = indices.shape[0]
            self._chk(self.L.trgl_draw_indexed_vs(self.h, int(vertex_shader), kind, None if uniforms is None else C.byref(uniforms),
                                                  pj.ctypes.data_as(C.POINTER(C.c_double)), ptrs[0], stride, nv, ptrs[1], nf, ptrs[2],
                                                  MEM_DEVICE if device else MEM_HOST))
            return
        assert colors is None, "colors: only with vertex_shader="
        if not device:
            vertices = np.ascontiguousarray(vertices, np.float64)
            indices = np.ascontiguousarray(indices, np.uint32).reshape(-1, 3)
            ptrs = (_ptr(vertices), _ptr(indices))
        else:
            ptrs = (_device_ptr(vertices, "vertices"), _device_ptr(indices, "indices"))
            self._keep.append((vertices, indices))
        nv, stride = vertices.shape
        nf = indices.shape[0]
        self._chk(self.L.trgl_draw_indexed(self.h, kind, C.byref(uniforms), pj.ctypes.data_as(C.POINTER(C.c_double)), ptrs[0],
                                           stride, nv, ptrs[1], nf, MEM_DEVICE if device else MEM_HOST))

    def vertex_stage(self, vertex_shader, uniforms, projection, vertices, indices, device=False, out=None):
        """trgl_vertex_stage: the vertex stage alone.  vertex_shader: a number from register_vertex_shader, or -1 for the built-in
        stage of draw_indexed (K = 24).  Host arrays: returns (clip [nf, 12], varyings [nf, K]) as numpy arrays.  device=True:
        vertices, indices and out = (clip, varyings) are device tensors (varyings may be None when K = 0), 16-byte aligned outputs
        that the stage fills on the context's stream; returns out."""
        vs = int(vertex_shader)
        K = VARY[PHONG] if vs < 0 else getattr(self, "_vertex_vary", {}).get(vs, 0)   # (an unknown number goes to the library, which refuses it)
        pj = np.ascontiguousarray(projection, np.float64).reshape(16)
        vertices, indices, _, ptrs = self._mesh_ptrs(vertices, indices, None, device)
        nv, stride = vertices.shape
        nf = indices.shape[0]
        if device:
            clip, vary = out
            optrs = (_device_ptr(clip, "clip"), _device_ptr(vary, "varyings"))
            self._keep.append((vertices, indices, clip, vary))
        else:
            assert out is None, "out: only with device=True"
            clip, vary = np.zeros((nf, 12), np.float64), np.zeros((nf, K), np.float64)
            optrs = (clip.ctypes.data, vary.ctypes.data if K else None)
        self._chk(self.L.trgl_vertex_stage(self.h, vs, None if uniforms is None else C.byref(uniforms), pj.ctypes.data_as(C.POINTER(C.c_double)),
                                           ptrs[0], stride, nv, ptrs[1], nf, optrs[0], optrs[1], MEM_DEVICE if device else MEM_HOST))
        return clip, vary

    def _instance_args(self, vertices, indices, instances, face_colors, instance_colors, visible, device, instances_device):
        """The mesh and instance arguments of trgl_draw_instanced / trgl_instance_stage as (ctypes arguments, n_faces, n_instances,
        has_colors, arrays to keep alive).  Host arrays are made contiguous; device arrays are checked by _device_ptr."""
        vertices, indices, face_colors, mp = self._mesh_ptrs(vertices, indices, face_colors, device)
        nv, stride = vertices.shape
        nf = indices.shape[0]
        if instances is None:
            inst_stride = 0
            n_inst = None
        else:
            if not instances_device:
                instances = np.ascontiguousarray(instances, np.float64)
                if instances.ndim != 2:
                    instances = instances.reshape(instances.shape[0], -1)
            n_inst, inst_stride = int(instances.shape[0]), int(instances.shape[1])
        for a, what in ((instance_colors, "instance_colors"), (visible, "visible")):
            if a is not None:
                if n_inst is None:
                    n_inst = int(a.shape[0])
                elif int(a.shape[0]) != n_inst:
                    raise ValueError(f"{what}: one entry per instance expected")
        if n_inst is None:
            raise ValueError("the number of instances comes from instances, instance_colors or visible: all three are None")
        if instances_device:
            ip = (_device_ptr(instances, "instances"), _device_ptr(instance_colors, "instance_colors"), _device_ptr(visible, "visible"))
        else:
            if instance_colors is not None:
                instance_colors = np.ascontiguousarray(instance_colors, np.uint32)
            if visible is not None:
                visible = np.ascontiguousarray(visible, np.uint8)
            ip = (_ptr(instances), _ptr(instance_colors), _ptr(visible))
        args = [mp[0], stride, nv, mp[1], nf, mp[2], MEM_DEVICE if device else MEM_HOST,
                ip[0], inst_stride, n_inst, ip[1], ip[2], MEM_DEVICE if instances_device else MEM_HOST]
        return args, nf, n_inst, face_colors is not None or instance_colors is not None, (vertices, indices, face_colors, instances, instance_colors, visible)

    def _order_args(self, order, order_device):
        """The three order arguments of the ordered calls as (ctypes arguments, n_order, what to keep alive)."""
        if order_device:
            if str(getattr(order, "dtype", "")) not in ("torch.int32", "torch.uint32") or not order.is_contiguous() or order.dim() != 1:
                raise ValueError("order_device=True: order must be a contiguous 32-bit integer device tensor [n_order]")
            n = int(order.shape[0])
            return [_device_ptr(order, "order") if n else None, n, MEM_DEVICE], n, order
        order = np.ascontiguousarray(order, np.uint32).reshape(-1)
        return [order.ctypes.data if order.size else None, int(order.size), MEM_HOST], int(order.size), order

    def instance_depths(self, model_view, point, instances, device=False):
        """trgl_instance_depths: the view-space z of `point` (a point of the mesh in model space) under every instance [n, stride >= 16].
        Host arrays: a numpy array, no GPU work.  device=True: instances is a contiguous float64 device tensor; the depths come back
        as a device tensor, queued on the context's stream without waiting."""
        instances, out = _instance_depths(self.L, self.h, model_view, point, instances, device)
        if device:
            self._keep.append((instances, out))
        return out

    def depth_order(self, depths, front_to_back=False, device=False):
        """trgl_depth_order: the order in which to draw instances of these depths - farthest first, or with front_to_back nearest first;
        ties ascend either way.  Host array: a uint32 numpy array.  device=True: depths is a contiguous float64 device tensor; the
        order comes back as an int32 device tensor (its bits are the uint32 numbers), sorted on the context's stream without waiting.
        Pass it to draw_instanced / instance_stage as order=..., order_device=True."""
        depths, out = _depth_order(self.L, self.h, depths, front_to_back, device)
        if device:
            self._keep.append((depths, out))
        return out

    def triangle_depths(self, clip, group=1, mode=TRI_DEPTH_CENTROID, device=False):
        """trgl_triangle_depths: one depth per group of `group` consecutive triangles of clip [n, 12] (see the module's triangle_depths).
        Host array: a numpy array, no GPU work.  device=True: clip is a contiguous float64 device tensor; the depths come back as a
        device tensor, queued on the context's stream without waiting - pass them to depth_order(device=True)."""
        clip, out = _triangle_depths(self.L, self.h, clip, group, mode, device)
        if device:
            self._keep.append((clip, out))
        return out

    def order_stage(self, clip, varyings=None, colors=None, order=(), group=1, device=False, out=None):
        """trgl_order_stage: the rows of the groups that `order` names, in that order.  Host arrays: as the module's order_stage.
        device=True: clip [n, 12] f64, varyings [n, K] f64 or None, colors [n] (32-bit) or None and order [n_order] (32-bit) are device
        tensors, out = (clip_out, varyings_out, colors_out) device tensors with len(order) * group rows (allocated with torch when not
        given); the gather is queued on the context's stream without waiting, and an entry of the list that names no group gives
        all-zero rows.  Returns (clip_out, varyings_out, colors_out)."""
        keep, out = _order_stage(self.L, self.h, clip, varyings, colors, order, group, device, out)
        if device:
            self._keep.append((keep, out))
        return out

    def sprite_stage(self, params, points, colors=None, device=False, out=None):
        """trgl_sprite_stage: two triangles per point (see the module's sprite_stage).  Host arrays: numpy, no GPU work.  device=True:
        points [n, stride] f64 and colors [n] (32-bit) or None are device tensors, out = (clip_out, varyings_out, colors_out) device
        tensors with 2 n rows (allocated with torch when not given); the stage is queued on the context's stream without waiting.
        Returns (clip_out, varyings_out, colors_out) - what triangle_depths(group=2), order_stage and draw(device=True) take."""
        keep, out = _sprite_stage(self.L, self.h, params, points, colors, device, out)
        if device:
            self._keep.append((keep, out))
        return out

    def line_stage(self, params, points, indices=None, colors=None, n_segments=None, device=False, out=None):
        """trgl_line_stage: two triangles per segment (see the module's line_stage).  device=True: points [n_points, stride] f64, indices
        [2 n] and colors [n] (32-bit) or None are device tensors; an index that names no point gives all-zero rows; queued on the
        context's stream without waiting.  Returns (clip_out, varyings_out, colors_out)."""
        keep, out = _line_stage(self.L, self.h, params, points, indices, colors, n_segments, device, out)
        if device:
            self._keep.append((keep, out))
        return out

    def draw_sprites(self, kind, params, points, colors=None, uniforms=None, device=False):
        """trgl_draw_sprites: draw() of the rows sprite_stage makes; the kind takes 6 + n_attr varyings, or none.  device=True: the
        points are expanded on the context's stream into buffers of the context's (no wait); they are read then, not at the flush."""
        points, _, colors = _quad_inputs(points, None, colors, device)
        p = _device_ptr if device else _ptr
        if device:
            self._keep.append((points, colors))
        self._chk(self.L.trgl_draw_sprites(self.h, kind, None if uniforms is None else C.byref(uniforms), C.byref(params), p(points),
                                           int(points.shape[1]), p(colors), int(points.shape[0]), MEM_DEVICE if device else MEM_HOST))

    def draw_lines(self, kind, params, points, indices=None, colors=None, n_segments=None, uniforms=None, device=False):
        """trgl_draw_lines: draw() of the rows line_stage makes; the kind takes 6 varyings - (t, side) per vertex - or none."""
        points, indices, colors = _quad_inputs(points, indices, colors, device)
        p = _device_ptr if device else _ptr
        if device:
            self._keep.append((points, indices, colors))
        self._chk(self.L.trgl_draw_lines(self.h, kind, None if uniforms is None else C.byref(uniforms), C.byref(params), p(points),
                                         int(points.shape[1]), int(points.shape[0]), p(indices), p(colors),
                                         _line_segments(points, indices, n_segments), MEM_DEVICE if device else MEM_HOST))

    def mesh_edges(self, indices, n_vertices, device=False, out=None, count=True):
        """trgl_mesh_edges (see the module's mesh_edges).  device=True: indices [n_faces, 3] is a 32-bit device tensor and the records
        come back as a device tensor [3 n_faces, 4] (`out` when given); an index >= n_vertices makes no edge.  count=True waits once for
        the 8-byte count; count=False queues the kernels without waiting and returns None for it.  Returns (edges, n_edges)."""
        keep, out, n = _mesh_edges(self.L, self.h, indices, n_vertices, device, out, count)
        if device:
            self._keep.append((keep, out))
        return out, n

    def edge_select(self, params, vertices, indices, edges, n_edges=None, device=False, out=None, count=None):
        """trgl_edge_select (see the module's edge_select).  device=True: vertices [n, stride] f64, indices and edges (32-bit) are device
        tensors - vertices may be one pose of skin_stage's output -, out = (codes uint8, segments, colors) device tensors, each may be
        None (allocated with torch when out is None); queued on the context's stream.  count (default: params.compact): wait once for
        the 8-byte count of selected records.  Returns (codes, segments, colors, n_selected or None): segments and colors are what
        draw_lines takes as indices and colors."""
        if count is None:
            count = bool(params.compact) or not device
        keep, out, n = _edge_select(self.L, self.h, params, vertices, indices, edges, n_edges, device, out, count)
        if device:
            self._keep.append((keep, out))
        return out[0], out[1], out[2], n

    def draw_outline(self, kind, line_params, edge_params, vertices, indices, edges, n_edges=None, uniforms=None, device=False):
        """trgl_draw_outline: edge_select with compaction into buffers of the context's, then draw_lines of the selected segments in
        their class colours with the mesh's vertices as points; the kind takes 6 varyings or none.  device=True: every array is a
        device tensor, and the call waits once for the count.  A line lies in the surface: bias the depth in line_params.projection."""
        if device:
            _device_f64(vertices, 2, "vertices")
        else:
            vertices = np.ascontiguousarray(vertices, np.float64)
        indices = _words32(indices, device, "indices", 3)
        edges = _words32(edges, device, "edges", 4)
        nf = int(indices.numel() if device else indices.size) // 3
        n = int(edges.numel() if device else edges.size) // 4 if n_edges is None else int(n_edges)
        p = _device_ptr if device else _ptr
        if device:
            self._keep.append((vertices, indices, edges))
        self._chk(self.L.trgl_draw_outline(self.h, kind, None if uniforms is None else C.byref(uniforms), C.byref(line_params),
                                           C.byref(edge_params), p(vertices), int(vertices.shape[1]), int(vertices.shape[0]), p(indices), nf,
                                           p(edges), n, MEM_DEVICE if device else MEM_HOST))

    def mesh_weld(self, params, vertices, indices=None, device=False, out=None, count=True):
        """trgl_mesh_weld (see the module's mesh_weld).  device=True: vertices [n, stride] f64 and indices [n_faces, 3] (32-bit, or None)
        are device tensors and so are the outputs; out: None for all of them, or a dict naming those to write - "remap", "firsts",
        "vertices", "indices", each a device tensor or None to allocate it.  count=True waits once for the 8-byte count; count=False
        queues the kernels without waiting and returns None for it: later calls take the capacity n.  Returns (dict, n_unique)."""
        keep, out, n = _mesh_weld(self.L, self.h, params, vertices, indices, device, out, count)
        if device:
            self._keep.append((keep, out))
        return out, n

    def mesh_clean(self, params, indices, vertices=None, n_vertices=None, device=False, out=None, count=True):
        """trgl_mesh_clean (see the module's mesh_clean).  device=True: indices [n_faces, 3] (32-bit) and vertices [n, stride] f64 (or None
        with n_vertices) are device tensors and so are the outputs; out: None for all of them, or a dict naming those to write -
        "indices", "face_firsts", "vremap", "vfirsts", "vertices", each a device tensor or None to allocate it.  count=True waits once for
        the 16 bytes of the counts; count=False queues the kernels without waiting and returns None for them: later calls take the
        capacities.  Returns (dict, (kept faces, kept vertices))."""
        keep, out, n = _mesh_clean(self.L, self.h, params, indices, vertices, n_vertices, device, out, count)
        if device:
            self._keep.append((keep, out))
        return out, n

    def mesh_simplify(self, params, vertices, indices, device=False, out=None, count=True):
        """trgl_mesh_simplify (see the module's mesh_simplify).  device=True: device tensors in and out; out: None for all outputs, or a
        dict naming those to write - "remap", "firsts", "vertices", "indices", "face_firsts".  count=False queues without waiting: with
        fill CLEAN_FILL_NONE a second level takes the outputs at their capacities.  Returns (dict, (kept faces, kept vertices))."""
        keep, out, n = _mesh_simplify(self.L, self.h, params, vertices, indices, device, out, count)
        if device:
            self._keep.append((keep, out))
        return out, n

    def debug_lod_hash_bits(self, bits=64):
        """Test hook (trgl_debug_lod_hash_bits): later device cleans and simplifies keep the low `bits` bits of the face hash (0 .. 64) and
        sort over them.  Small values force the walk through colliding triples; 0 is one run.  The outputs do not change with it."""
        self._chk(self.L.trgl_debug_lod_hash_bits(self.h, int(bits)))

    def debug_lod_sort(self, n_faces, n_vertices):
        """Diagnostic (trgl_debug_lod_sort): the sort of the last device clean of these counts again, over the pairs it left; no wait."""
        self._chk(self.L.trgl_debug_lod_sort(self.h, int(n_faces), int(n_vertices)))

    def debug_weld_hash_bits(self, bits=64):
        """Test hook (trgl_debug_weld_hash_bits): later device welds keep the low `bits` bits of the hash (0 .. 64) and sort over them.
        Small values force the walk through colliding keys; 0 is one run.  The outputs do not change with it."""
        self._chk(self.L.trgl_debug_weld_hash_bits(self.h, int(bits)))

    def debug_weld_sort(self, n_vertices):
        """Diagnostic (trgl_debug_weld_sort): the sort of the last device weld of n_vertices again, over the pairs it left; no wait."""
        self._chk(self.L.trgl_debug_weld_sort(self.h, int(n_vertices)))

    def subdiv_topology(self, indices, n_vertices, edges, n_edges=None, device=False, out=None):
        """trgl_subdiv_topology (see the module's subdiv_topology).  device=True: indices and edges are 32-bit device tensors - edges as
        mesh_edges(device=True) left them; n_edges=None passes the capacity, so no count has to visit the host -, out = (refined indices
        [4 n_faces, 3], stencils [subdiv_stencil_words]) device tensors (allocated with torch when None); queued on the context's
        stream without waiting.  Returns (refined indices, stencils)."""
        keep, refined, stencils = _subdiv_topology(self.L, self.h, indices, n_vertices, edges, n_edges, device, out)
        if device:
            self._keep.append((keep, refined, stencils))
        return refined, stencils

    def subdiv_vertices(self, params, vertices, stencils, n_edges=None, device=False, out=None):
        """trgl_subdiv_vertices (see the module's subdiv_vertices).  device=True: vertices [n, stride] f64 - one pose of skin_stage's
        output, say - and stencils are device tensors, out [n + n_edges, stride] a device tensor (allocated with torch when None); one
        kernel queued on the context's stream without waiting.  n_edges: the E the stencils were made with (None: from their size)."""
        keep, out = _subdiv_vertices(self.L, self.h, params, vertices, stencils, n_edges, device, out)
        if device:
            self._keep.append((keep, out))
        return out

    def draw_subdivided(self, kind, uniforms, projection, params, vertices, stencils, refined_indices, n_edges=None, device=False,
                        vertex_shader=None, colors=None):
        """trgl_draw_subdivided: subdiv_vertices into a buffer of the context's, then draw_indexed of it with the refined indices
        (vertex_shader= and colors= - one per refined face - as there).  device=True: every array is a device tensor; no wait."""
        pj = np.ascontiguousarray(projection, np.float64).reshape(16)
        vertices, stencils, n_edges = _subdiv_inputs(vertices, stencils, n_edges, device)
        _, refined_indices, colors, ptrs = self._mesh_ptrs(vertices, refined_indices, colors, device)
        p = _device_ptr if device else _ptr
        if device:
            self._keep.append((vertices, stencils, refined_indices, colors))
        self._chk(self.L.trgl_draw_subdivided(self.h, -1 if vertex_shader is None else int(vertex_shader), kind,
                                              None if uniforms is None else C.byref(uniforms), _dp(pj), C.byref(params), p(vertices),
                                              int(vertices.shape[0]), p(stencils), n_edges, ptrs[1], int(refined_indices.shape[0]), ptrs[2],
                                              MEM_DEVICE if device else MEM_HOST))

    def skin_stage(self, vertices, joints, weights, palette, flags=0, device=False, out=None):
        """trgl_skin_stage (see the module's skin_stage).  Host arrays: numpy, no GPU work.  device=True: vertices [n, stride] f64,
        joints [n, k] (16-bit), weights [n, k] f64 and palette [n_poses, n_joints, 16] f64 are device tensors, out [n_poses, n, stride]
        a device tensor (allocated with torch when not given); the stage is queued on the context's stream without waiting.  Returns
        out: out[q] is what draw_indexed, mesh_bounds, mesh_normals and mesh_tangents take with device=True."""
        keep, out = _skin_stage(self.L, self.h, vertices, joints, weights, palette, flags, device, out)
        if device:
            self._keep.append((keep, out))
        return out

    def pose_palette(self, parents, local, inverse_bind=None, device=False, out=None):
        """trgl_pose_palette (see the module's pose_palette).  device=True: parents [n_joints] (32-bit), local [n_poses, n_joints, 16] f64
        and inverse_bind [n_joints, 16] f64 or None are device tensors; queued on the context's stream without waiting.  Returns the
        palettes [n_poses, n_joints, 16] - what skin_stage takes."""
        keep, out = _pose_palette(self.L, self.h, parents, local, inverse_bind, device, out)
        if device:
            self._keep.append((keep, out))
        return out

    def draw_skinned(self, kind, uniforms, projection, vertices, joints, weights, palette, indices, flags=0, device=False,
                     vertex_shader=None, colors=None):
        """trgl_draw_skinned: skin_stage with one pose into a buffer of the context's, then draw_indexed of it (vertex_shader= and
        colors= as there).  device=True: every array is a device tensor; no wait."""
        pj = np.ascontiguousarray(projection, np.float64).reshape(16)
        vertices, joints, weights, palette = _skin_inputs(vertices, joints, weights, palette, device)
        P = _skin_params(vertices, joints, palette, flags)
        _, indices, colors, ptrs = self._mesh_ptrs(vertices, indices, colors, device)
        p = _device_ptr if device else _ptr
        if device:
            self._keep.append((vertices, joints, weights, palette, indices, colors))
        self._chk(self.L.trgl_draw_skinned(self.h, -1 if vertex_shader is None else int(vertex_shader), kind,
                                           None if uniforms is None else C.byref(uniforms), _dp(pj), C.byref(P), p(vertices),
                                           int(vertices.shape[0]), p(joints), p(weights), p(palette), ptrs[1], int(indices.shape[0]), ptrs[2],
                                           MEM_DEVICE if device else MEM_HOST))

    def instance_boxes(self, local, instances, out=None):
        """trgl_instance_boxes: the world box [n, 6] = (min.xyz, max.xyz) of every instance [n, stride >= 16], AABB::transform of `local`
        under the instance's matrix.  local: [6] in host memory (one box for every instance: mesh_bounds' halves concatenated) or
        [n, stride >= 6] where the instances are.  numpy instances: a numpy array, no GPU work.  A contiguous float64 device tensor: the
        boxes come back as a device tensor (`out` when given), queued on the context's stream without waiting - the input of
        occlusion_boxes(device=True) and frustum_boxes."""
        keep, out = _instance_boxes(self.L, self.h, local, instances, out)
        if _is_device_tensor(out):
            self._keep.append(keep)
        return out

    def frustum_boxes(self, planes, boxes, codes=None, merge=False):
        """trgl_frustum_boxes: one code byte per box [n, 6] from Frustum::intersects against planes [6, 4] (host memory).  merge=False
        writes OCCL_VISIBLE / OCCL_OUTSIDE into `codes` (allocated when None); merge=True writes OCCL_OUTSIDE into the given codes where
        the frustum culls and leaves every other byte as it is - over the codes of occlusion_boxes that makes the `visible` array of
        draw_instanced.  numpy boxes: no GPU work.  Device tensors (boxes float64, codes uint8 at any address): queued on the context's
        stream without waiting."""
        keep, codes = _frustum_boxes(self.L, self.h, planes, boxes, codes, merge)
        if _is_device_tensor(codes):
            self._keep.append(keep)
        return codes

    def draw_instanced(self, kind, uniforms, projection, vertices, indices, instances=None, vertex_shader=None, face_colors=None,
                       instance_colors=None, visible=None, device=False, instances_device=False, order=None, order_device=False):
        """trgl_draw_instanced: the mesh (vertices [nv, stride], indices [nf, 3]) once per instance whose `visible` byte has bit 0 set
        (visible None: every instance), in ascending instance order.  instances [n, stride]: with the built-in stage (vertex_shader None)
        the first 16 doubles are a row-major model matrix M and the stage runs under uniforms.model_view * M; a user vertex shader
        reads them as in.inst.  Colours: instance_colors [n] or face_colors [nf], not both.  device: the mesh arrays are device
        tensors; instances_device: instances, instance_colors and visible are (the codes of occlusion_boxes(device=True) are a valid
        `visible`; the call then waits once for the count of drawn instances).  order (trgl_draw_instanced_ordered): the instances
        are visited in the order this list of numbers names them - the result of depth_order, or any list; an instance named twice
        is drawn twice, one that is not named is not drawn, an empty list draws nothing; order_device: the list is a device tensor (entries out of range are
        skipped, and the call waits once for the count)."""
        pj = np.ascontiguousarray(projection, np.float64).reshape(16)
        args, _, _, _, keep = self._instance_args(vertices, indices, instances, face_colors, instance_colors, visible, device, instances_device)
        vs = -1 if vertex_shader is None else int(vertex_shader)
        if order is None:
            if device or instances_device:
                self._keep.append(keep)
            self._chk(self.L.trgl_draw_instanced(self.h, vs, kind, None if uniforms is None else C.byref(uniforms), _dp(pj), *args))
            return
        oargs, n_order, okeep = self._order_args(order, order_device)
        if n_order == 0:                     # no position to visit: nothing is drawn (the C call takes a null list for "no list")
            return
        if device or instances_device or order_device:
            self._keep.append(keep + (okeep,))
        self._chk(self.L.trgl_draw_instanced_ordered(self.h, vs, kind, None if uniforms is None else C.byref(uniforms), _dp(pj), *args, *oargs))

    def instance_stage(self, vertex_shader, uniforms, projection, vertices, indices, instances=None, face_colors=None, instance_colors=None,
                       visible=None, device=False, instances_device=False, out=None, order=None, order_device=False):
        """trgl_instance_stage: the stages of draw_instanced alone; returns (clip, varyings, colors, n_out) with n_out = drawn instances
        * nf rows written.  vertex_shader: a number from register_vertex_shader, or -1 / None for the built-in stage (K = 24).
        Host instances: numpy arrays cut to n_out rows (varyings [n_out, K]; colors None when the call has none).  instances_device=True:
        out = (clip, varyings, colors) are 16-byte aligned device tensors with room for n * nf rows (varyings may be None when K = 0,
        colors when the call has none); they come back as they are.  order / order_device: as for draw_instanced
        (trgl_instance_stage_ordered); the outputs then need room for len(order) * nf rows."""
        vs = -1 if vertex_shader is None else int(vertex_shader)
        K = VARY[PHONG] if vs < 0 else getattr(self, "_vertex_vary", {}).get(vs, 0)
        pj = np.ascontiguousarray(projection, np.float64).reshape(16)
        args, nf, n_inst, has_colors, keep = self._instance_args(vertices, indices, instances, face_colors, instance_colors, visible, device, instances_device)
        n_out = C.c_uint64(0)
        oargs, n_order, okeep = (None, n_inst, None) if order is None else self._order_args(order, order_device)
        if order_device:
            self._keep.append((okeep,))
        if instances_device:
            clip, vary, col = out
            optrs = (_device_ptr(clip, "clip"), _device_ptr(vary, "varyings"), _device_ptr(col, "colors"))
            self._keep.append(keep + (clip, vary, col))
        else:
            assert out is None, "out: only with instances_device=True"
            rows = n_order * nf
            clip, vary = np.zeros((rows, 12), np.float64), np.zeros((rows, K), np.float64)
            col = np.zeros(rows, np.uint32) if has_colors else None
            optrs = (clip.ctypes.data, vary.ctypes.data if K else None, col.ctypes.data if has_colors else None)
            if device:
                self._keep.append(keep)
        if order is not None and n_order == 0:
            pass                             # no position to visit: no rows (the C call takes a null list for "no list")
        elif order is None:
            self._chk(self.L.trgl_instance_stage(self.h, vs, None if uniforms is None else C.byref(uniforms), _dp(pj), *args,
                                                 optrs[0], optrs[1], optrs[2], C.byref(n_out)))
        else:
            self._chk(self.L.trgl_instance_stage_ordered(self.h, vs, None if uniforms is None else C.byref(uniforms), _dp(pj), *args, *oargs,
                                                         optrs[0], optrs[1], optrs[2], C.byref(n_out)))
        n = int(n_out.value)
        if instances_device:
            return clip, vary, col, n
        return clip[:n], vary[:n], None if col is None else col[:n], n

    def mesh_bounds(self, vertices, device=False):
        """trgl_mesh_bounds: Model::computeAABB (model.cpp:15-40) of vertices [n, stride >= 3]; returns (min[3], max[3]).  device=True:
        a device tensor, reduced on the context's stream in order with the draws (nothing is flushed); the call waits for the result."""
        return _mesh_bounds(self.L, self.h, vertices, device)

    def _mesh_attr(self, name, vertices, indices, device, wait):
        if not device:
            vertices, indices = _host_mesh(vertices, indices)
        vertices, indices, _, ptrs = self._mesh_ptrs(vertices, indices, None, device)
        if device and not wait:
            self._keep.append((vertices, indices))
        return vertices, _mesh_attr(self.L, self.h, name, ptrs, vertices, indices, device, wait or not device)

    def mesh_normals(self, vertices, indices, device=False, wait=True):
        """trgl_mesh_normals: Model::generateNormalsIfNeeded (model.cpp:269-316); returns (vertices, generated).  Host arrays: computed
        on a copy.  device=True: device tensors [n, stride >= 6] f64 and [n_faces, 3] u32, rewritten in place on the context's stream in
        order with the draws (nothing is flushed); wait=False queues without waiting and returns generated = None."""
        return self._mesh_attr("mesh_normals", vertices, indices, device, wait)

    def mesh_tangents(self, vertices, indices, device=False, wait=True):
        """trgl_mesh_tangents: Model::computeTangentsIfNeeded (model.cpp:318-388) likewise, vertices [n, stride >= 14]."""
        return self._mesh_attr("mesh_tangents", vertices, indices, device, wait)

    def image_blur(self, img, radius, device=False):
        """trgl_image_blur: TGAImage::gaussian_blur (tgaimage.cpp:271-324); returns the blurred image.  Host array: computed on a copy, no
        GPU work.  device=True: a contiguous uint8 device tensor [h, w, bpp], blurred in place on the context's stream in order with
        everything else (nothing is flushed, the call does not wait); the tensor is kept alive until the next sync."""
        if not device:
            out = np.array(img, np.uint8, order="C")
            _image_blur(self.L, self.h, out.ctypes.data, out, radius, False)
            return out
        ptr = _device_image(img, "img")
        self._keep.append((img,))
        _image_blur(self.L, self.h, ptr, img, radius, True)
        return img

    def image_scale(self, img, w2, h2, device=False, out=None):
        """trgl_image_scale: TGAImage::scale (tgaimage.cpp:246-267) of img [h, w, bpp] into [h2, w2, bpp]; returns the result.  device=True:
        contiguous uint8 device tensors, gathered on the context's stream (nothing is flushed, the call does not wait); `out` (must not
        overlap img) is allocated with torch when not given.  Raises where the reference returns false."""
        if not device:
            src = np.ascontiguousarray(img, np.uint8)
            if out is None:
                out = np.empty((max(int(h2), 0), max(int(w2), 0), src.shape[2] if len(src.shape) == 3 else 0), np.uint8)
            if out.dtype != np.uint8 or not out.flags.c_contiguous or out.shape != (int(h2), int(w2), src.shape[2]):
                raise ValueError("image_scale: out must be a contiguous uint8 array [h2, w2, bpp]")
            _image_scale(self.L, self.h, src.ctypes.data, src, out.ctypes.data, w2, h2, False)
            return out
        sptr = _device_image(img, "img")
        if out is None:
            import torch
            out = torch.empty((max(int(h2), 0), max(int(w2), 0), int(img.shape[2])), dtype=torch.uint8, device=img.device)
        elif tuple(out.shape) != (int(h2), int(w2), int(img.shape[2])):
            raise ValueError("image_scale: out must be [h2, w2, bpp]")
        self._keep.append((img, out))
        _image_scale(self.L, self.h, sptr, img, _device_image(out, "out"), w2, h2, True)
        return out

    def image_downsample(self, img, factor, device=False, out=None):
        """trgl_image_downsample: the exact box filter of img [h, w, bpp] into [h // factor, w // factor, bpp]; returns the result.
        Host array: no GPU work.  device=True: contiguous uint8 device tensors at any address, filtered on the context's stream (nothing is
        flushed, the call does not wait); `out` (must not overlap img) is allocated with torch when not given; both are kept alive until
        the next sync."""
        if not device:
            return _host_image_downsample(self.L, self.h, img, factor, out)
        sptr = _device_image(img, "img")
        shape = _box_shape(img, factor)
        if out is None:
            import torch
            out = torch.empty(shape, dtype=torch.uint8, device=img.device)
        elif tuple(out.shape) != shape:
            raise ValueError("image_downsample: out must be [h // factor, w // factor, bpp]")
        self._keep.append((img, out))
        _image_downsample(self.L, self.h, sptr, img, factor, _device_image(out, "out"), True)
        return out

    def framebuffer_resolve(self, factor, device=False, out=None):
        """trgl_framebuffer_resolve: the SSAA resolve - flushes what is queued (a pending clear included), then box-filters the resident
        frame into [H // factor, W // factor, bpp]; the frame, the z-buffer and the stats stay as they are.  device=False: a numpy array,
        the call waits for the small image.  device=True: a uint8 tensor on the context's device (allocated with torch when `out` is
        not given), queued without waiting and kept alive until the next sync.  Not on a strip / band context."""
        f = int(factor)
        shape = (self.height // f if f >= 1 else 0, self.width // f if f >= 1 else 0, self.bpp)
        if not device:
            if out is None:
                out = np.empty(shape, np.uint8)
            elif out.dtype != np.uint8 or not out.flags.c_contiguous or out.shape != shape:
                raise ValueError("framebuffer_resolve: out must be a contiguous uint8 array [H // factor, W // factor, bpp]")
            self._chk(self.L.trgl_framebuffer_resolve(self.h, f, out.ctypes.data, MEM_HOST))
            return out
        if out is None:
            import torch
            out = torch.empty(shape, dtype=torch.uint8, device=f"cuda:{self.device}")
        elif tuple(out.shape) != shape:
            raise ValueError("framebuffer_resolve: out must be [H // factor, W // factor, bpp]")
        ptr = _device_image(out, "out")
        self._keep.append((out,))
        self._chk(self.L.trgl_framebuffer_resolve(self.h, f, ptr, MEM_DEVICE))
        return out

    def texture_from_image(self, slot, img, factor=1, device=False):
        """trgl_texture_from_image: the box filter of img [h, w, bpp] (a [h, w] image counts as bpp 1) becomes the texture of `slot`, ordered
        like upload_texture: draws submitted earlier sample the old texture.  device=True: a contiguous uint8 device tensor, filtered in
        HBM without a host wait when the slot is empty or holds a texture of the same size; kept alive until the next sync."""
        if not device:
            t = np.ascontiguousarray(img, np.uint8)
            if t.ndim == 2:
                t = t[..., None]
            h, w, bpp = _image_dims(t, "texture_from_image")
            self._chk(self.L.trgl_texture_from_image(self.h, int(slot), t.ctypes.data, w, h, bpp, int(factor), MEM_HOST))
            return
        ptr = _device_image(img, "img")
        h, w, bpp = _image_dims(img, "texture_from_image")
        self._keep.append((img,))
        self._chk(self.L.trgl_texture_from_image(self.h, int(slot), ptr, w, h, bpp, int(factor), MEM_DEVICE))

    def texture_from_framebuffer(self, slot, factor=1):
        """trgl_texture_from_framebuffer: render-to-texture - flushes what is queued, then the box filter of the resident frame becomes the
        texture of `slot` [H // factor, W // factor, bpp], a snapshot that later clears and draws do not change.  No host wait when the
        slot is empty or holds a texture of that size.  Not on a strip / band context."""
        self._chk(self.L.trgl_texture_from_framebuffer(self.h, int(slot), int(factor)))

    def texture_mipmaps(self, slot):
        """trgl_texture_mipmaps: builds the mip chain of the texture in `slot`, ordered like the other texture calls (draws submitted earlier
        sample one level).  Every call that replaces the slot's texels drops the chain; a rebuild on a slot that has held one of this size
        is kernels on the stream without a host wait."""
        self._chk(self.L.trgl_texture_mipmaps(self.h, int(slot)))

    def image_mipmaps(self, img, device=False, out=None):
        """trgl_image_mipmaps: levels 1 .. L-1 of img [h, w, bpp] as one packed uint8 array (see mip_layout); returns it.  Host array: no
        GPU work.  device=True: contiguous uint8 device tensors at any address, built on the context's stream (nothing is flushed, the call
        does not wait); `out` (1-D, mip_layout(w, h, bpp)[3] bytes, not overlapping img; only the levels' bytes are written) is allocated
        zeroed with torch when not given; both are kept alive until the next sync."""
        if not device:
            return _host_image_mipmaps(self.L, self.h, img, out)
        sptr = _device_image(img, "img")
        h, w, bpp = _image_dims(img, "image_mipmaps")
        total = mip_layout(w, h, bpp)[3]
        if out is None:
            import torch
            out = torch.zeros(total, dtype=torch.uint8, device=img.device)
        elif tuple(out.shape) != (total,):
            raise ValueError("image_mipmaps: out must be 1-D with mip_layout(w, h, bpp)[3] bytes")
        self._keep.append((img, out))
        _image_mipmaps(self.L, self.h, sptr, img, _device_image(out, "out") if total else None, True)
        return out

    def lod_stage(self, viewport, clip, varyings, uv_offset=0, out_offset=6, device=False):
        """trgl_lod_stage (see the module's lod_stage): in place on varyings [n, K]; returns it.  device=True: contiguous float64 device
        tensors, queued on the context's stream in order with the draws (no wait, no flush), kept alive until the next sync."""
        clip, varyings = _lod_stage(self.L, self.h, viewport, clip, varyings, uv_offset, out_offset, device)
        if device:
            self._keep.append((clip, varyings))
        return varyings

    def framebuffer_blur(self, radius):
        """trgl_framebuffer_blur: framebuffer.gaussian_blur(radius) on the resident frame (flushes what is queued, does not wait); the
        z-buffer and the stats stay as they are.  Not on a strip / band context."""
        self._chk(self.L.trgl_framebuffer_blur(self.h, int(radius)))

    def shadow_mask_image(self, params, depth, zmap, device=False, out=None):
        """trgl_shadow_mask_image; returns the [h, w] uint8 mask.  Host arrays: no GPU work.  device=True: contiguous float64 device tensors
        [h, w] and [map_h, map_w], masked on the context's stream in order with everything else (nothing is flushed, the call does not
        wait); `out` is allocated with torch when not given."""
        if not device:
            return _host_shadow_mask_image(self.L, self.h, params, depth, zmap)
        for t, what in ((depth, "depth"), (zmap, "zmap")):
            if not hasattr(t, "data_ptr") or str(t.dtype) != "torch.float64" or not t.is_contiguous():
                raise ValueError(f"device=True: {what} must be a contiguous float64 device tensor")
        if out is None:
            import torch
            out = torch.empty(tuple(depth.shape), dtype=torch.uint8, device=depth.device)
        elif tuple(out.shape) != tuple(depth.shape):
            raise ValueError("shadow_mask_image: out must be [h, w]")
        self._keep.append((depth, zmap, out))
        _shadow_mask_image(self.L, self.h, params, _device_ptr(depth, "depth"), depth, _device_ptr(zmap, "zmap"), zmap, _device_image(out, "out"), True)
        return out

    def image_modulate(self, img, mask, device=False):
        """trgl_image_modulate; returns the multiplied image.  Host arrays: computed on a copy.  device=True: contiguous uint8 device tensors
        [h, w, bpp] and [h, w], img multiplied in place on the context's stream (nothing is flushed, the call does not wait)."""
        if not device:
            return _host_image_modulate(self.L, self.h, img, mask)
        ptr, mptr = _device_image(img, "img"), _device_image(mask, "mask")
        self._keep.append((img, mask))
        _image_modulate(self.L, self.h, ptr, img, mptr, mask, True)
        return img

    def shadow_mask(self, params, slot=0, out=None, device=False):
        """trgl_shadow_mask: the mask of the resident z-buffer against the depths of snapshot `slot` (flushes what is queued).  Returns a
        [H, W] uint8 numpy array (the call waits for it), or with device=True a device tensor (allocated with torch when `out` is not
        given; the call does not wait).  Not on a strip / band context."""
        if device:
            if out is None:
                import torch
                out = torch.empty((self.height, self.width), dtype=torch.uint8, device=f"cuda:{self.device}")
            ptr = _device_image(out, "out")
            self._keep.append((out,))
        else:
            if out is None:
                out = np.empty((self.height, self.width), np.uint8)
            if out.dtype != np.uint8 or not out.flags.c_contiguous:
                raise ValueError("shadow_mask: out must be a contiguous uint8 array")
            ptr = out.ctypes.data
        if int(np.prod(tuple(out.shape))) != self.width * self.height:
            raise ValueError("shadow_mask: out must hold W * H bytes")
        self._chk(self.L.trgl_shadow_mask(self.h, C.byref(params), int(slot), ptr, MEM_DEVICE if device else MEM_HOST))
        return out

    def framebuffer_modulate(self, mask, device=False):
        """trgl_framebuffer_modulate: the resident frame multiplied by mask [H, W] / 255 in place (flushes what is queued, does not wait);
        the z-buffer and the stats stay as they are.  mask: a host array, or with device=True a contiguous uint8 device tensor."""
        if device:
            ptr = _device_image(mask, "mask")
            self._keep.append((mask,))
        else:
            mask = np.ascontiguousarray(mask, np.uint8)
            ptr = mask.ctypes.data
        if int(np.prod(tuple(mask.shape))) != self.width * self.height:
            raise ValueError("framebuffer_modulate: the mask must hold W * H bytes")
        self._chk(self.L.trgl_framebuffer_modulate(self.h, ptr, MEM_DEVICE if device else MEM_HOST))

    def occlusion_boxes_image(self, depth, viewport, view_proj, boxes, device=False, out=None):
        """trgl_occlusion_boxes_image; returns the [n] uint8 codes.  Host arrays: no GPU work.  device=True: depth [h, w] and boxes [n, 6] are
        contiguous float64 device tensors, queried on the context's stream in order with everything else (nothing is flushed, the call
        does not wait); `out` (uint8 [n], any alignment) is allocated with torch when not given."""
        if not device:
            return _host_occlusion_boxes_image(self.L, self.h, depth, viewport, view_proj, boxes)
        for t, what in ((depth, "depth"), (boxes, "boxes")):
            if not hasattr(t, "data_ptr") or str(t.dtype) != "torch.float64" or not t.is_contiguous():
                raise ValueError(f"device=True: {what} must be a contiguous float64 device tensor")
        n = _boxes_count(boxes)
        if out is None:
            import torch
            out = torch.empty(n, dtype=torch.uint8, device=boxes.device)
        elif tuple(out.shape) != (n,):
            raise ValueError("occlusion_boxes_image: out must be [n]")
        self._keep.append((depth, boxes, out))
        _occlusion_boxes_image(self.L, self.h, _device_ptr(depth, "depth"), depth, viewport, view_proj, _device_ptr(boxes, "boxes"), n,
                               _device_image(out, "out"), True)
        return out

    def occlusion_boxes(self, view_proj, boxes, snapshot=None, device=False):
        """trgl_occlusion_boxes: one OCCL_* code per box [n, 6] against the resident z-buffer (snapshot=None) or the depths of a snapshot
        slot, under the context's viewport (flushes what is queued).  Host boxes give a uint8 numpy array (the call waits for it);
        device=True takes a contiguous float64 device tensor and returns a device tensor without waiting.  Not on a strip / band context."""
        if not device:
            boxes = np.ascontiguousarray(boxes, np.float64)
        n = _boxes_count(boxes)
        m = _dp(_f64(view_proj, 16, "view_proj"))
        slot = -1 if snapshot is None else int(snapshot)
        if device:
            if str(boxes.dtype) != "torch.float64" or not boxes.is_contiguous():
                raise ValueError("device=True: boxes must be a contiguous float64 device tensor")
            import torch
            out = torch.empty(n, dtype=torch.uint8, device=boxes.device)
            self._keep.append((boxes, out))
            self._chk(self.L.trgl_occlusion_boxes(self.h, m, _device_ptr(boxes, "boxes"), n, MEM_DEVICE, slot, _device_ptr(out, "out"), MEM_DEVICE))
            return out
        out = np.empty(n, np.uint8)
        self._chk(self.L.trgl_occlusion_boxes(self.h, m, boxes.ctypes.data, n, MEM_HOST, slot, out.ctypes.data, MEM_HOST))
        return out

    def zbuffer_snapshot(self, slot=0):
        """trgl_zbuffer_snapshot: main.cpp:700 as one device-to-device copy (flushes what is queued, does not wait)."""
        self._chk(self.L.trgl_zbuffer_snapshot(self.h, int(slot)))

    def zbuffer_restore(self, slot=0):
        """trgl_zbuffer_restore: main.cpp:730 likewise; the framebuffer and the stats stay as they are."""
        self._chk(self.L.trgl_zbuffer_restore(self.h, int(slot)))

    def zbuffer_snapshot_free(self, slot=0):
        self._chk(self.L.trgl_zbuffer_snapshot_free(self.h, int(slot)))

    def postprocess(self, zbuffer_image=True, ao=True, final=True, params=None):
        """main.cpp:269-311,317-362,757-783 on the device; returns dict of [h,w,3] uint8 images."""
        out = {}
        shape = (self.height, self.width, 3)
        zi = np.empty(shape, np.uint8) if zbuffer_image else None
        a = np.empty(shape, np.uint8) if ao else None
        f = np.empty(shape, np.uint8) if final else None
        self._chk(self.L.trgl_postprocess(self.h, None if params is None else C.byref(params),
                                          None if zi is None else zi.ctypes.data, None if a is None else a.ctypes.data,
                                          None if f is None else f.ctypes.data))
        return dict(zbuffer_image=zi, ao=a, final=f)

    def flush(self):
        self._chk(self.L.trgl_flush(self.h))

    def flush_begin(self):
        """Setup + binning of what was submitted (does not touch the framebuffer / z-buffer); flush_end() runs the raster."""
        self._chk(self.L.trgl_flush_begin(self.h))

    def flush_end(self):
        self._chk(self.L.trgl_flush_end(self.h))

    def sync(self):
        self._chk(self.L.trgl_sync(self.h))
        self._keep.clear()

    # ---- results ----
    def read_framebuffer(self) -> np.ndarray:
        out = np.empty((self.height, self.width, self.bpp), np.uint8)
        self._chk(self.L.trgl_read_framebuffer(self.h, out.ctypes.data))
        self._keep.clear()
        return out

    def read_zbuffer(self) -> np.ndarray:
        out = np.empty((self.height, self.width), np.float64)
        self._chk(self.L.trgl_read_zbuffer(self.h, out.ctypes.data))
        self._keep.clear()
        return out

    def write_framebuffer(self, fb):
        fb = np.ascontiguousarray(fb, np.uint8)
        assert fb.size == self.width * self.height * self.bpp
        self._chk(self.L.trgl_write_framebuffer(self.h, fb.ctypes.data))

    def write_zbuffer(self, z):
        z = np.ascontiguousarray(z, np.float64)
        assert z.size == self.width * self.height
        self._chk(self.L.trgl_write_zbuffer(self.h, z.ctypes.data))

    def stats(self):
        s = Stats()
        self._chk(self.L.trgl_get_stats(self.h, C.byref(s)))
        return s.astuple()

    def stats_line(self) -> str:
        s = Stats()
        self._chk(self.L.trgl_get_stats(self.h, C.byref(s)))
        buf = C.create_string_buffer(1024)
        self._chk(self.L.trgl_format_stats(C.byref(s), buf, 1024))
        return buf.value.decode().strip()

    def reset_stats(self):
        self._chk(self.L.trgl_reset_stats(self.h))

    @property
    def framebuffer_ptr(self) -> int:
        return self.L.trgl_framebuffer_device_ptr(self.h)

    @property
    def zbuffer_ptr(self) -> int:
        return self.L.trgl_zbuffer_device_ptr(self.h)

    @property
    def stream(self) -> int:
        return self.L.trgl_stream(self.h)

    def set_stream(self, hip_stream, use_own: bool = False):
        """Enqueue on the caller's hipStream_t (int handle, e.g. torch.cuda.current_stream().cuda_stream; 0 is the
        legacy default stream).  use_own=True returns to the context's own stream."""
        self._chk(self.L.trgl_set_stream(self.h, hip_stream or None, 1 if use_own else 0))

    # ---- measurement ----
    def set_profiling(self, on: bool):
        self._chk(self.L.trgl_set_profiling(self.h, 1 if on else 0))

    def phase_ms(self):
        ms = (C.c_double * NUM_PHASES)()
        n = C.c_uint64()
        self._chk(self.L.trgl_get_phase_ms(self.h, ms, C.byref(n)))
        return list(ms), n.value

    def reset_phase_ms(self):
        self._chk(self.L.trgl_reset_phase_ms(self.h))

    def selftest_division(self, samples: int, seed: int = 1) -> int:
        bad = C.c_uint64()
        self._chk(self.L.trgl_selftest_division(self.h, samples, seed, C.byref(bad)))
        return bad.value

    def selftest_sampler(self, slot: int, uv) -> np.ndarray:
        """The device samplers' texel fetch of texture `slot` at uv [n,2]: [n,5] uint8 = bgra[4], bytespp."""
        uv = np.ascontiguousarray(uv, np.float64).reshape(-1, 2)
        out = np.zeros((uv.shape[0], 5), np.uint8)
        self._chk(self.L.trgl_selftest_sampler(self.h, slot, uv.ctypes.data, uv.shape[0], out.ctypes.data))
        return out

    def selftest_sampler_lod(self, slot: int, uv, lod, mode=SAMPLE_TRILINEAR) -> np.ndarray:
        """The filtered device samplers of the user shaders on texture `slot` at uv [n,2] and lod [n] (mode SAMPLE_LEVEL, SAMPLE_LINEAR:
        lod converted to int; SAMPLE_TRILINEAR): [n,5] uint8 = bgra[4], bytespp."""
        uv = np.ascontiguousarray(uv, np.float64).reshape(-1, 2)
        lod = np.ascontiguousarray(np.broadcast_to(np.asarray(lod, np.float64), (uv.shape[0],)))
        out = np.zeros((uv.shape[0], 5), np.uint8)
        self._chk(self.L.trgl_selftest_sampler_lod(self.h, int(slot), uv.ctypes.data, lod.ctypes.data, int(mode), uv.shape[0], out.ctypes.data))
        return out

    def last_flush_info(self):
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._chk(self.L.trgl_get_last_flush_info(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return dict(triangles=a.value, pairs=b.value, tiles=c.value)

    def debug_binning(self, mode=None, S=0, G=0):
        """Test hook (trgl_debug_binning).  mode BIN_AUTO / BIN_EXPAND / BIN_DIRECT (with segments of S pair slots and groups of G
        setup blocks) sets how the next flushes bin; None changes nothing.  Returns what the last complete flush did:
        dict(direct=..., fell_back=...)."""
        d, f = C.c_int(), C.c_int()
        self._chk(self.L.trgl_debug_binning(self.h, -1 if mode is None else mode, S, G, C.byref(d), C.byref(f)))
        return dict(direct=bool(d.value), fell_back=bool(f.value))

    def debug_radix_blocks(self, n=None):
        """Test hook (trgl_debug_radix_blocks).  n caps the grids of the radix scatters of the next flushes (0: automatic, as many
        blocks as the device holds at once; every block walks its chunks with a stride of the grid); None changes nothing.  Returns
        the grids of the last binning queued: dict(first=..., last=...)."""
        if n is not None:
            self._radix_blocks = int(n)
        a, b = C.c_uint32(), C.c_uint32()
        self._chk(self.L.trgl_debug_radix_blocks(self.h, getattr(self, "_radix_blocks", 0), C.byref(a), C.byref(b)))
        return dict(first=a.value, last=b.value)

    def _debug_read(self, what, dtype):
        need = C.c_size_t()
        self._chk(self.L.trgl_debug_read(self.h, what, None, 0, C.byref(need)))
        out = np.zeros(need.value // np.dtype(dtype).itemsize, dtype)
        if need.value:
            self._chk(self.L.trgl_debug_read(self.h, what, out.ctypes.data, out.nbytes, None))
        return out

    def debug_snapshot(self):
        """The intermediate buffers of the flush begun with flush_begin() (which stays pending: this call does not complete
        it) or of the last complete flush (until the next draw or clear): what k_setup and the binning left for k_raster.
        recs [N + 1] TRI_REC (rows of triangles without pairs are not written; row N exists after the complete flush), cnt [N],
        tilebox [N, 2], vals / bmask [P] (the side k_raster reads), tile_start / tile_end [tiles], info: dict of DBG_INFO_FIELDS.
        Raises TrglError where no flush can be read."""
        info = dict(zip(DBG_INFO_FIELDS, (int(v) for v in self._debug_read(DBG_INFO, np.int64))))
        return dict(info=info, recs=self._debug_read(DBG_RECS, TRI_REC), cnt=self._debug_read(DBG_CNT, np.uint32),
                    tilebox=self._debug_read(DBG_TILEBOX, np.uint32).reshape(-1, 2), vals=self._debug_read(DBG_VALS, np.uint32),
                    bmask=self._debug_read(DBG_BMASK, np.uint16), tile_start=self._debug_read(DBG_TILE_START, np.uint32),
                    tile_end=self._debug_read(DBG_TILE_END, np.uint32))
