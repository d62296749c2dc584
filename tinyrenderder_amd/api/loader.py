"""What every family of the binding shares: the constants of include/trgl.h, the structures that its prototypes name, TrglError, and
load_library() - the one place that opens libtrgl.so and declares every prototype."""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))      # tinyrenderder_amd/: the Makefile writes the library there
LIB_PATH = os.path.join(HERE, "libtrgl.so")

FLAT, GOURAUD, PHONG, EYE, CHECKER = 0, 1, 2, 3, 4
VARY = {FLAT: 0, GOURAUD: 3, PHONG: 24, EYE: 24, CHECKER: 0}
SHADER_USER_FIRST, MAX_USER_SHADERS, MAX_USER_VARY = 64, 32, 64      # user shaders: kinds handed out by Context.register_shader
SHADER_MAY_DISCARD = 1        # TRGL_SHADER_MAY_DISCARD: the user shader's trgl_fragment returns trgl_frag_out (it can discard)
SHADER_READS_DEST = 4         # TRGL_SHADER_READS_DEST: in.dst is the pixel the fragment is drawn over (with MAY_DISCARD only)
SHADER_NO_DEPTH_WRITE = 8     # TRGL_SHADER_NO_DEPTH_WRITE: a drawn fragment leaves the depth alone (with MAY_DISCARD only)

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
    _lib = L
    return L
