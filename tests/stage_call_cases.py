"""One table of calls to the entry points that run a stage in front of a draw (csrc/trgl_stage_*.cpp), for tests/test_stage_call_errors.py
and tests/golden/make_stage_call_errors.py: per entry point a valid baseline at the smallest shape - 1 triangle, 1 sprite, 1 segment over
2 points, 1 vertex with 1 joint and 1 influence, 1 instance of a 1-face mesh - and named faults, each the baseline with one argument
edited (two where the case pins which of two faults wins).  What the library answers (return code, trgl_last_error text) is recorded in
tests/golden/stage_call_errors.json.

An argument is a number, None, a numpy array or a ctypes object in host memory, Off(array, bytes) - an address inside a host array -
or Dev(bytes, off) - a real device allocation of that size, `off` bytes in to misalign it.  Every call with a Dev argument is one that
a check refuses before anything is allocated or launched: no case hands over a device array whose contents the library would trust."""
import ctypes as C

import numpy as np

import vertex_shader_sources as V
from tinyrenderder_amd import api

H, D, BAD = api.MEM_HOST, api.MEM_DEVICE, 7
W = 16                       # the frame of the cases that need a context: W x W, 3 bytes per pixel
EYE4 = np.eye(4).reshape(16)
RED = 0xFFFF0000


class Off:
    def __init__(self, array, by):
        self.array, self.by = array, by


class Dev:
    def __init__(self, nbytes, off=0):
        self.nbytes, self.off = nbytes, off


def tri():
    """one triangle in clip space, inside the frame"""
    return np.array([[-0.5, -0.5, 0.0, 1.0, 0.5, -0.5, 0.0, 1.0, 0.0, 0.5, 0.0, 1.0]])


def mesh():
    """a 1-face mesh of the reference's vertex records (pos3, normal3, uv2) and its index triple"""
    v = np.array([[-0.5, -0.5, 0.0, 0, 0, 1, 0, 0], [0.5, -0.5, 0.0, 0, 0, 1, 1, 0], [0.0, 0.5, 0.0, 0, 0, 1, 0.5, 1]], np.float64)
    return v, np.array([0, 1, 2], np.uint32)


def u32(*v):
    return np.array(v, np.uint32)


def sprite_params(**kw):
    d = dict(size=0.5)
    d.update(kw)
    return api.make_sprite_params(EYE4, EYE4, **d)


def line_params(w_min=0.1):
    return api.make_line_params(EYE4, EYE4, 2.0, (W / 2, W / 2), w_min)


def skin_params(stride=3, k=1, nj=1, flags=0, poses=1, pstride=16, reserved=0):
    return api.SkinParams(stride, k, nj, flags, poses, pstride, reserved)


def uniforms():
    return api.make_uniforms(EYE4)


def move(dz=-2.0):
    m = np.eye(4)
    m[2, 3] = dz
    return m.reshape(1, 16)


# ---- the entry points: name -> (needs a context even with host memory, baseline arguments in the order of include/trgl.h) ------------
def _sprite_in():
    return dict(P=sprite_params(), points=np.array([[0.0, 0.0, 0.0]]), stride=3, colors=u32(RED), n=1, mem=H)


def _line_in():
    return dict(P=line_params(), points=np.array([[-0.5, 0.0, 0.0], [0.5, 0.0, 0.0]]), stride=3, n_points=2, indices=u32(0, 1), colors=u32(RED),
                n=1, mem=H)


def _quad_out():
    return dict(clip_out=np.zeros((2, 12)), vary_out=np.zeros((2, 6)), colors_out=np.zeros(2, np.uint32))


def _skin_in():
    pal = np.eye(4)
    pal[:3, 3] = (0.25, 0.5, 0.0)
    return dict(P=skin_params(), vertices=np.array([[-0.5, -0.5, 0.0]]), n=1, joints=np.zeros((1, 1), np.uint16), weights=np.ones((1, 1)),
                palette=pal.reshape(1, 16))


def _mesh_in():
    v, i = mesh()
    return dict(vertices=v, stride=8, n_vertices=3, indices=i, n_faces=1)


def _inst_in():
    d = _mesh_in()
    d.update(face_colors=None, mesh_mem=H, instances=move(0.0), inst_stride=16, n_inst=1, inst_colors=None, visible=None, inst_mem=H)
    return d


def _inst_out():
    return dict(clip_out=np.zeros((1, 12)), vary_out=np.zeros((1, 24)), colors_out=None, n_out=C.c_uint64(77))


BASELINES = {
    "trgl_sprite_stage": (False, lambda: {**_sprite_in(), **_quad_out()}),
    "trgl_draw_sprites": (True, lambda: dict(kind=api.FLAT, u=None, **_sprite_in())),
    "trgl_line_stage": (False, lambda: {**_line_in(), **_quad_out()}),
    "trgl_draw_lines": (True, lambda: dict(kind=api.FLAT, u=None, **_line_in())),
    "trgl_skin_stage": (False, lambda: dict(**_skin_in(), mem=H, out=np.zeros((1, 3)))),
    "trgl_pose_palette": (False, lambda: dict(parents=np.array([-1], np.int32), inverse_bind=EYE4.copy(), n_joints=1, local=move(3.0), local_stride=16,
                                              n_poses=1, mem=H, palette=np.zeros(16), palette_stride=16)),
    "trgl_draw_skinned": (True, lambda: dict(vs=-1, kind=api.PHONG, u=uniforms(), projection=EYE4.copy(), P=skin_params(stride=8),
                                             vertices=mesh()[0], n=3, joints=np.zeros((3, 1), np.uint16), weights=np.ones((3, 1)),
                                             palette=EYE4.copy(), indices=mesh()[1], n_faces=1, colors=None, mem=H)),
    "trgl_triangle_depths": (False, lambda: dict(clip=tri(), n=1, group=1, mode=api.CENTROID, mem=H, depths_out=np.zeros(1))),
    "trgl_order_stage": (False, lambda: dict(K=6, clip=tri(), vary=np.arange(6.0).reshape(1, 6), colors=u32(RED), n=1, order=u32(0), n_order=1,
                                             group=1, mem=H, clip_out=np.zeros((1, 12)), vary_out=np.zeros((1, 6)), colors_out=np.zeros(1, np.uint32))),
    "trgl_draw_ordered": (True, lambda: dict(kind=api.FLAT, u=None, clip=tri(), vary=None, colors=u32(RED), n=1, mem=H, order=u32(0), n_order=1,
                                             group=1, order_mem=H)),
    "trgl_draw_indexed": (True, lambda: dict(kind=api.PHONG, u=uniforms(), projection=EYE4.copy(), **_mesh_in(), mem=H)),
    "trgl_draw_indexed_vs": (True, lambda: dict(vs=0, kind=api.FLAT, u=uniforms(), projection=EYE4.copy(), **_mesh_in(), colors=u32(RED), mem=H)),
    "trgl_draw_indexed_vs_clipped": (True, lambda: dict(vs=-1, kind=api.PHONG, u=uniforms(), projection=EYE4.copy(), plane=np.array([1.0, 0, 0, 0.25]),
                                                        attrs=None, n_attrs=-1, **_mesh_in(), colors=None, mem=H)),
    "trgl_vertex_stage": (True, lambda: dict(vs=-1, u=uniforms(), projection=EYE4.copy(), **_mesh_in(), clip_out=np.zeros((1, 12)),
                                             vary_out=np.zeros((1, 24)), mem=H)),
    "trgl_clip_stage": (False, lambda: dict(plane=np.array([1.0, 0, 0, 0.25]), attrs=None, n_attrs=0, K=0, clip=tri(), vary=None, colors=u32(RED), n=1,
                                            clip_out=np.zeros((2, 12)), vary_out=None, colors_out=np.zeros(2, np.uint32), n_out=C.c_uint64(77), mem=H)),
    "trgl_draw_clipped": (True, lambda: dict(kind=api.FLAT, u=None, plane=np.array([1.0, 0, 0, 0.25]), attrs=None, n_attrs=0, clip=tri(), vary=None,
                                             colors=u32(RED), n=1, mem=H)),
    "trgl_draw_instanced": (True, lambda: dict(vs=-1, kind=api.PHONG, u=uniforms(), projection=EYE4.copy(), **_inst_in())),
    "trgl_instance_stage": (True, lambda: dict(vs=-1, u=uniforms(), projection=EYE4.copy(), **_inst_in(), **_inst_out())),
    "trgl_draw_instanced_ordered": (True, lambda: dict(vs=-1, kind=api.PHONG, u=uniforms(), projection=EYE4.copy(), **_inst_in(), order=u32(0), n_order=1,
                                                       order_mem=H)),
    "trgl_instance_stage_ordered": (True, lambda: dict(vs=-1, u=uniforms(), projection=EYE4.copy(), **_inst_in(), order=u32(0), n_order=1, order_mem=H,
                                                       **_inst_out())),
    "trgl_instance_depths": (False, lambda: dict(model_view=EYE4.copy(), point=np.zeros(3), instances=move(), stride=16, n=1, mem=H, depths_out=np.zeros(1))),
    "trgl_depth_order": (False, lambda: dict(depths=np.array([-2.0]), n=1, direction=api.ORDER_BACK_TO_FRONT, mem=H, order_out=np.zeros(1, np.uint32))),
}

# ---- the faults: entry point -> {name: the arguments that differ from the baseline} ------------------------------------------------
_MEM = dict(bad_mem=dict(mem=BAD), device_without_context=dict(mem=D))       # (with a context the second one is left out: it would run)
_D8 = Dev(256, 4)            # a device address that is a multiple of 4 and not of 8

FAULTS = {
    "trgl_sprite_stage": dict(
        _MEM, null_params=dict(P=None), bad_mode=dict(P=sprite_params(mode=5)), n0_and_bad_mode=dict(n=0, P=sprite_params(mode=5)), n0=dict(n=0),
        stride_2=dict(stride=2), size_offset_outside=dict(P=sprite_params(size_offset=3)), attr_range_outside=dict(P=sprite_params(attr_offset=3, n_attr=1)),
        n_too_large=dict(n=1 << 30), vary_null_with_attrs=dict(P=sprite_params(attr_offset=2, n_attr=1), vary_out=None), null_points=dict(points=None),
        null_clip_out=dict(clip_out=None), colors_without_colors_out=dict(colors_out=None), output_over_input=dict(clip_out="points"),
        two_outputs_overlap=dict(vary_out="clip_out"), misaligned_points=dict(points=("off", "points", 4)), misaligned_colors=dict(colors=("off", "colors", 2)),
        device_misaligned=dict(mem=D, points=_D8, colors=None, clip_out=Dev(256), vary_out=Dev(256), colors_out=None)),
    "trgl_draw_sprites": dict(
        bad_mem=dict(mem=BAD), null_params=dict(P=None), bad_mode=dict(P=sprite_params(mode=5)), unknown_kind=dict(kind=63),
        kind_does_not_fit=dict(kind=api.PHONG, u=uniforms()), checker_without_uniforms=dict(kind=api.CHECKER), n0=dict(n=0), null_points=dict(points=None),
        device_null_points=dict(mem=D, points=None, colors=None)),
    "trgl_line_stage": dict(
        _MEM, null_params=dict(P=None), stride_2=dict(stride=2), w_min_zero=dict(P=line_params(0.0)), w_min_infinite=dict(P=line_params(float("inf"))),
        n_too_large=dict(n=1 << 30), too_few_points_without_indices=dict(indices=None, n_points=1), index_out_of_range=dict(indices=u32(0, 2)),
        n0=dict(n=0), null_points=dict(points=None), misaligned_indices=dict(indices=("off", "indices", 2)),
        device_misaligned=dict(mem=D, points=Dev(256), indices=Dev(64, 2), colors=None, clip_out=Dev(256), vary_out=Dev(256), colors_out=None)),
    "trgl_draw_lines": dict(
        bad_mem=dict(mem=BAD), null_params=dict(P=None), unknown_kind=dict(kind=63), kind_does_not_fit=dict(kind=api.GOURAUD), n0=dict(n=0),
        index_out_of_range=dict(indices=u32(0, 2))),
    "trgl_skin_stage": dict(
        _MEM, null_params=dict(P=None), stride_2=dict(P=skin_params(stride=2)), no_influences=dict(P=skin_params(k=0)), nine_influences=dict(P=skin_params(k=9)),
        no_joints=dict(P=skin_params(nj=0)), no_poses=dict(P=skin_params(poses=0)), palette_stride_small=dict(P=skin_params(pstride=15)),
        reserved_set=dict(P=skin_params(reserved=1)), unknown_flag=dict(P=skin_params(flags=8)), normal_outside=dict(P=skin_params(flags=1)),
        arrays_too_large=dict(n=1 << 62), n0=dict(n=0), null_vertices=dict(vertices=None), null_out=dict(out=None),
        misaligned_joints=dict(joints=("off", "joints", 1)), misaligned_out=dict(out=("off", "out", 4)), output_over_input=dict(out="vertices"),
        joint_out_of_range=dict(joints=np.ones((1, 1), np.uint16)),
        device_misaligned=dict(mem=D, vertices=_D8, joints=Dev(64), weights=Dev(64), palette=Dev(256), out=Dev(256)),
        device_stride_above_5120=dict(mem=D, P=skin_params(stride=5121), vertices=Dev(5121 * 8), joints=Dev(64), weights=Dev(64), palette=Dev(256),
                                      out=Dev(5121 * 8))),
    "trgl_pose_palette": dict(
        _MEM, no_joints=dict(n_joints=0), local_stride_small=dict(local_stride=15), palette_stride_small=dict(palette_stride=15),
        arrays_too_large=dict(n_poses=1 << 58), no_poses=dict(n_poses=0), null_parents=dict(parents=None), null_local=dict(local=None),
        null_palette=dict(palette=None), misaligned_parents=dict(parents=("off", "parents", 2)), misaligned_local=dict(local=("off", "local", 4)),
        output_over_input=dict(palette="local"), parent_is_itself=dict(parents=np.array([0], np.int32)),
        device_misaligned=dict(mem=D, parents=Dev(64), inverse_bind=None, local=_D8, palette=Dev(256))),
    "trgl_draw_skinned": dict(
        bad_mem=dict(mem=BAD), null_params=dict(P=None), two_poses=dict(P=skin_params(stride=8, poses=2, pstride=16)),
        two_poses_and_colors_without_shader=dict(P=skin_params(stride=8, poses=2, pstride=16), colors=u32(RED)), colors_without_shader=dict(colors=u32(RED)),
        unknown_vertex_shader=dict(vs=9, kind=api.FLAT), kind_not_phong=dict(kind=api.FLAT), null_uniforms=dict(u=None), index_out_of_range=dict(indices=u32(0, 1, 3)),
        no_faces=dict(n_faces=0), faces_without_vertices=dict(n=0, mem=D, vertices=Dev(256), indices=Dev(64)), null_joints=dict(joints=None),
        joint_out_of_range=dict(joints=np.ones((3, 1), np.uint16))),
    "trgl_triangle_depths": dict(
        _MEM, bad_mode=dict(mode=7), group_0=dict(group=0), n_not_a_multiple=dict(group=2), n_too_large=dict(n=1 << 31), n0=dict(n=0), null_clip=dict(clip=None),
        null_out=dict(depths_out=None), device_misaligned=dict(mem=D, clip=_D8, depths_out=Dev(64))),
    "trgl_order_stage": dict(
        _MEM, bad_mem_and_negative_K=dict(mem=BAD, K=-1), negative_K=dict(K=-1), K_above_max=dict(K=1000), group_0=dict(group=0), n_not_a_multiple=dict(group=2),
        null_order=dict(order=None), list_too_long=dict(n_order=1 << 31), empty_list=dict(n_order=0), null_clip_out=dict(clip_out=None),
        null_vary_out=dict(vary_out=None), colors_without_colors_out=dict(colors_out=None), null_clip=dict(clip=None), null_vary=dict(vary=None),
        entry_is_no_group=dict(order=u32(1)),
        device_misaligned=dict(mem=D, clip=Dev(256), vary=Dev(64), colors=None, order=Dev(64, 2), clip_out=Dev(256), vary_out=Dev(64), colors_out=None)),
    "trgl_draw_ordered": dict(
        bad_order_mem=dict(order_mem=BAD), list_without_count=dict(n_order=0), null_list_group_0=dict(order=None, n_order=0, group=0), unknown_kind=dict(kind=63),
        bad_mem=dict(mem=BAD), group_0=dict(group=0), null_clip=dict(clip=None), kind_needs_varyings=dict(kind=api.GOURAUD), checker_without_uniforms=dict(kind=api.CHECKER),
        entry_is_no_group=dict(order=u32(1)), device_rows_misaligned=dict(mem=D, clip=_D8, colors=None), device_list_misaligned=dict(order_mem=D, order=Dev(64, 2))),
    "trgl_draw_indexed": dict(
        bad_mem=dict(mem=BAD), kind_not_phong=dict(kind=api.FLAT), null_uniforms=dict(u=None), null_indices=dict(indices=None), stride_7=dict(stride=7),
        no_faces=dict(n_faces=0), no_faces_and_index_out_of_range=dict(n_faces=0, indices=u32(0, 1, 3)), too_many_faces=dict(n_faces=1 << 31),
        index_out_of_range=dict(indices=u32(0, 1, 3))),
    "trgl_draw_indexed_vs": dict(
        bad_mem=dict(mem=BAD), builtin_stage=dict(vs=-1), unknown_vertex_shader=dict(vs=9), null_projection=dict(projection=None), stride_0=dict(stride=0),
        too_many_faces=dict(n_faces=1 << 31), index_out_of_range=dict(indices=u32(0, 1, 3)), unknown_kind=dict(kind=63), kind_differs_in_varyings=dict(kind=api.GOURAUD),
        no_faces=dict(n_faces=0)),
    "trgl_draw_indexed_vs_clipped": dict(
        bad_mem=dict(mem=BAD), null_plane=dict(plane=None), no_faces_and_null_plane=dict(n_faces=0, plane=None), kind_not_phong=dict(kind=api.FLAT),
        bad_attribute_list=dict(attrs=(api.ClipAttr * 1)(api.ClipAttr(23, 3)), n_attrs=1), index_out_of_range=dict(indices=u32(0, 1, 3)), no_faces=dict(n_faces=0)),
    "trgl_vertex_stage": dict(
        bad_mem=dict(mem=BAD), unknown_vertex_shader=dict(vs=9), null_vertices=dict(vertices=None), null_uniforms=dict(u=None), stride_7=dict(stride=7),
        too_many_faces=dict(n_faces=1 << 31), index_out_of_range=dict(indices=u32(0, 1, 3)), null_clip_out=dict(clip_out=None), null_vary_out=dict(vary_out=None),
        no_faces=dict(n_faces=0), device_outputs_misaligned=dict(mem=D, vertices=Dev(256), indices=Dev(64), clip_out=Dev(256, 8), vary_out=Dev(256))),
    "trgl_clip_stage": dict(
        _MEM, device_without_context_and_null_plane=dict(mem=D, plane=None), null_plane=dict(plane=None), null_n_out=dict(n_out=None), negative_K=dict(K=-1),
        bad_attribute_list=dict(attrs=(api.ClipAttr * 1)(api.ClipAttr(0, 3)), n_attrs=1), n0=dict(n=0), null_clip=dict(clip=None), null_clip_out=dict(clip_out=None),
        colors_without_colors_out=dict(colors_out=None), device_misaligned=dict(mem=D, clip=_D8, colors=None, clip_out=Dev(256), colors_out=None)),
    "trgl_draw_clipped": dict(
        unknown_kind=dict(kind=63), null_plane=dict(plane=None), n0=dict(n=0), n0_and_bad_mem=dict(n=0, mem=BAD), bad_mem=dict(mem=BAD), null_clip=dict(clip=None),
        kind_needs_varyings=dict(kind=api.GOURAUD), checker_without_uniforms=dict(kind=api.CHECKER)),
    "trgl_draw_instanced": dict(
        bad_mesh_mem=dict(mesh_mem=BAD), bad_instance_mem=dict(inst_mem=BAD), unknown_vertex_shader=dict(vs=9), null_uniforms=dict(u=None),
        instance_stride_15=dict(inst_stride=15), null_instances=dict(instances=None), both_colors=dict(face_colors=u32(RED), inst_colors=u32(RED)),
        too_many_instances=dict(n_inst=1 << 31, n_faces=0), index_out_of_range=dict(indices=u32(0, 1, 3)), unknown_kind=dict(kind=63), kind_differs_in_varyings=dict(kind=api.FLAT),
        no_instances=dict(n_inst=0), no_instances_and_index_out_of_range=dict(n_inst=0, indices=u32(0, 1, 3)), device_instances_misaligned=dict(inst_mem=D, instances=_D8)),
    "trgl_instance_stage": dict(
        bad_instance_mem=dict(inst_mem=BAD), null_n_out=dict(n_out=None), nothing_to_run_and_null_n_out=dict(n_inst=0, n_out=None), no_instances=dict(n_inst=0),
        null_clip_out=dict(clip_out=None), null_vary_out=dict(vary_out=None), colors_without_colors_out=dict(face_colors=u32(RED)),
        device_outputs_misaligned=dict(inst_mem=D, instances=Dev(256), clip_out=Dev(256, 8), vary_out=Dev(256))),
    "trgl_draw_instanced_ordered": dict(
        bad_order_mem=dict(order_mem=BAD), list_without_count=dict(n_order=0), list_too_long=dict(n_order=1 << 31, n_faces=0), entry_is_no_instance=dict(order=u32(1)),
        no_faces_and_entry_is_no_instance=dict(n_faces=0, order=u32(1)), device_list_misaligned=dict(order_mem=D, order=Dev(64, 2)),
        bad_instance_mem_and_bad_order_mem=dict(inst_mem=BAD, order_mem=BAD)),
    "trgl_instance_stage_ordered": dict(
        bad_order_mem=dict(order_mem=BAD), bad_order_mem_and_null_n_out=dict(order_mem=BAD, n_out=None), entry_is_no_instance=dict(order=u32(1)),
        null_n_out=dict(n_out=None), null_clip_out=dict(clip_out=None)),
    "trgl_instance_depths": dict(
        _MEM, null_model_view=dict(model_view=None), null_point=dict(point=None), stride_15=dict(stride=15), n_too_large=dict(n=1 << 31), n0=dict(n=0),
        null_instances=dict(instances=None), null_out=dict(depths_out=None), device_misaligned=dict(mem=D, instances=_D8, depths_out=Dev(64))),
    "trgl_depth_order": dict(
        _MEM, bad_direction=dict(direction=2), n_too_large=dict(n=1 << 31), n0=dict(n=0), null_depths=dict(depths=None), null_out=dict(order_out=None),
        device_misaligned=dict(mem=D, depths=Dev(64), order_out=Dev(64, 2))),
}

# a vertex shader for trgl_draw_indexed_vs (number 0 of the context; K = 0 goes with FLAT)
VERTEX_SHADER = (V.TRANSFORM, 0)


def arguments(entry, fault=None):
    """The baseline arguments of `entry` with the edits of `fault` (None: the baseline).  An edit "name" stands for the baseline's own
    argument of that name (an output laid over an input), ("off", name, bytes) for an address inside it."""
    args = BASELINES[entry][1]()
    for k, v in (FAULTS[entry][fault] if fault else {}).items():
        assert k in args, (entry, fault, k)
        if isinstance(v, str):
            v = args[v]
        elif isinstance(v, tuple) and v and v[0] == "off":
            v = Off(args[v[1]], v[2])
        args[k] = v
    return args


def uses_device(args):
    return any(isinstance(v, Dev) for v in args.values())


def cases(with_context):
    """[(entry, fault or None)] of one part: the calls that run with c = NULL (host memory, plus what every entry point that needs a
    context answers without one), or the calls that need a context."""
    out = []
    for entry, (needs_ctx, _) in BASELINES.items():
        for fault in [None] + list(FAULTS[entry]):
            dev = uses_device(arguments(entry, fault))
            if with_context and (needs_ctx or dev):
                out.append((entry, fault))
            elif not with_context and not dev and (not needs_ctx or fault is None):
                out.append((entry, fault))      # (needs_ctx: the baseline's arguments with c = NULL - the code alone is recorded)
    return out


def case_id(entry, fault):
    return f"{entry}:{fault or 'baseline'}"


def call(L, handle, entry, args, device_ptr=None):
    """Call `entry` of library L on context `handle` (None: c = NULL).  device_ptr(Dev) gives the address of a device allocation.
    Returns (return code, trgl_last_error text) - the text None where the call was made without the context it needs."""
    f = getattr(L, entry)
    conv = []
    for v, t in zip(args.values(), f.argtypes[1:]):
        if isinstance(v, np.ndarray):
            v = v.ctypes.data
        elif isinstance(v, Off):
            v = v.array.ctypes.data + v.by
        elif isinstance(v, Dev):
            v = device_ptr(v)
        elif isinstance(v, (C.Structure, C._SimpleCData)):
            v = C.byref(v)
        if isinstance(v, int) and hasattr(t, "contents"):       # an address for a typed pointer
            v = C.cast(C.c_void_p(v), t)
        conv.append(v)
    assert len(conv) == len(f.argtypes) - 1, entry
    rc = f(handle, *conv)
    if handle is None and BASELINES[entry][0]:
        return rc, None
    return rc, L.trgl_last_error(handle).decode() if rc else ""


def run_host_part(L):
    """Every case of cases(False) with c = NULL: ({case id: [rc, text]}, {entry: the baseline's arguments as the call left them})."""
    results, baselines = {}, {}
    for entry, fault in cases(False):
        args = arguments(entry, fault)
        results[case_id(entry, fault)] = list(call(L, None, entry, args))
        if fault is None:
            baselines[entry] = args
    return results, baselines


def run_context_part(L):
    """Every case of cases(True) on one W x W context of GPU 0: ({case id: [rc, text]}, {entry: the baseline's arguments as the call
    left them}, {entry: the depths of the frame behind the baseline of a draw})."""
    import torch
    h = C.c_void_p()
    assert L.trgl_create(0, W, W, 3, C.byref(h)) == 0, L.trgl_last_error(None)
    held = {}

    def device_ptr(d):
        if id(d) not in held:
            held[id(d)] = torch.zeros(d.nbytes + 16, dtype=torch.uint8, device="cuda:0")
        assert held[id(d)].data_ptr() % 256 == 0
        return held[id(d)].data_ptr() + d.off

    results, baselines, frames = {}, {}, {}
    try:
        vs = C.c_int(-1)
        assert L.trgl_register_vertex_shader(h, VERTEX_SHADER[0].encode(), VERTEX_SHADER[1], C.byref(vs)) == 0 and vs.value == 0, L.trgl_last_error(h)
        for entry, fault in cases(True):
            args = arguments(entry, fault)
            if fault is None:
                assert L.trgl_clear(h, None, float("inf")) == 0
            results[case_id(entry, fault)] = list(call(L, h, entry, args, device_ptr))
            if fault is None:
                baselines[entry] = args
                if "_draw_" in entry:
                    frames[entry] = np.zeros((W, W))
                    assert L.trgl_read_zbuffer(h, frames[entry].ctypes.data) == 0, L.trgl_last_error(h)
        assert L.trgl_sync(h) == 0, L.trgl_last_error(h)
    finally:
        L.trgl_destroy(h)
    return results, baselines, frames
