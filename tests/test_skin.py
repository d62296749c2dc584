"""Skeletal animation in host memory (include/trgl.h: trgl_skin_stage, trgl_pose_palette; no GPU).

tests/skin_model.py is pinned to the reference's geometry.h: its 4x4 product reproduces tests/golden/instance_matmul_golden.npz and
its blend, transforms, normalisation and hierarchy reproduce tests/golden/skin_golden.npz (make_skin_golden.py) on all bits.  The host
twins equal the model bit for bit - stored NaNs and copied NaN payloads included - write nothing behind their output, refuse a joint
or parent out of range without writing, and return every error of the header.  Meaning: one influence of weight 1 is the model's
mat * vec, identities return the positions (up to -0.0), and a bent arm drawn through the CPU oracle covers where the bent arm is."""
import ctypes as C
import os

import numpy as np
import pytest

import skin_cases as SC
import skin_model as M
from oracle import orc
from tinyrenderder_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
E_INVALID, E_UNSUPPORTED = -1, -5
H, D = api.MEM_HOST, api.MEM_DEVICE


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(got, want, what):
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    bad = np.argwhere(_bits(got) != _bits(want))
    assert bad.size == 0, f"{what}: differ at {bad[:4].tolist()}: {_bits(got)[tuple(bad[0])]:#x} != {_bits(want)[tuple(bad[0])]:#x}"


# ---- the model against the reference ------------------------------------------------------------------------------------------------
def test_the_models_product_reproduces_the_reference():
    g = np.load(os.path.join(HERE, "golden", "instance_matmul_golden.npz"))
    ab = g["ab"].view(np.float64).reshape(-1, 2, 4, 4)
    got = M.mat_product(ab[:, 0], ab[:, 1]).reshape(-1, 16)
    want = g["c"].view(np.float64)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


def test_the_model_reproduces_the_references_skinning_and_hierarchy():
    g = np.load(os.path.join(HERE, "golden", "skin_golden.npz"))
    f = lambda k: g[k].view(np.float64)
    want = M.canon(f("skinned"))
    assert np.isnan(want).any() and np.isinf(want).any() and (want == 0).any() and np.isfinite(want).mean() > 0.5
    _same(M.skin(f("vertices"), g["joints"], f("weights"), f("palette"), M.NORMAL | M.TANGENT | M.BITANGENT)[0], want, "skinned")
    want = M.canon(f("palettes"))
    assert np.isnan(want).any() and np.isfinite(want).mean() > 0.4
    _same(M.pose_palette(g["parents"], f("local"), f("inverse_bind")), want, "palettes")
    # ... and the host twins on the same fixture
    _same(api.skin_stage(f("vertices"), g["joints"], f("weights"), f("palette"), 7)[0], M.canon(f("skinned")), "host skinned")
    _same(api.pose_palette(g["parents"], f("local"), f("inverse_bind")), want, "host palettes")


# ---- the host twins against the model ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_infl", SC.INFLUENCES)
@pytest.mark.parametrize("stride", SC.STRIDES)
def test_host_skinning_equals_the_model(stride, n_infl):
    seen_nan = False
    for n in SC.COUNTS:
        for flags in SC.flag_sets(stride):
            for n_poses, pad in ((1, 0), (3, 5)):
                n_joints = 7
                v, j, w = SC.mesh(n, stride, n_infl, n_joints, seed=1000 * stride + 10 * n_infl + n)
                pal = SC.palette(n_poses, n_joints, seed=n + flags, pad=pad)
                want = M.skin(v, j, w, pal, flags)
                v0 = v.copy()
                got = api.skin_stage(v, j, w, pal, flags)
                _same(got, want, f"n={n} flags={flags} poses={n_poses}")
                assert np.array_equal(_bits(v), _bits(v0))
                seen_nan |= bool(np.isnan(want[..., :3]).any()) and not np.isnan(want[..., :3]).all()
    assert seen_nan, "the planted rows left no trace in the model's output"


def test_copied_doubles_keep_their_nan_payloads():
    v, j, w = SC.mesh(65, 8, 2, 5, seed=3)
    out = api.skin_stage(v, j, w, SC.palette(2, 5, 4, pad=3), M.NORMAL)
    for q in range(2):
        assert np.array_equal(_bits(out[q][15:17, 7]), _bits(SC.NAN_PAYLOAD)) and _bits(out[q][17, 6]) == _bits(SC.NAN_PAYLOAD)[1]
        assert np.array_equal(_bits(out[q][:, 6:]), _bits(v[:, 6:]))


def _raw_skin(L, P, v, j, w, pal, out, n=None, mem=H, params=True):
    return L.trgl_skin_stage(None, C.byref(P) if params else None, None if v is None else v.ctypes.data, v.shape[0] if n is None else n,
                             None if j is None else j.ctypes.data, None if w is None else w.ctypes.data,
                             None if pal is None else pal.ctypes.data, mem, out if out is None or isinstance(out, int) else out.ctypes.data)


def test_nothing_is_written_behind_the_output():
    L = api.load_library()
    n, stride, k, nj, poses = 65, 9, 3, 6, 3
    v, j, w = SC.mesh(n, stride, k, nj, seed=8)
    pal = SC.palette(poses, nj, 9, pad=4)
    out = np.full(poses * n * stride + 3 * stride, SC.SENTINEL_F64)
    P = api.SkinParams(stride, k, nj, M.NORMAL, poses, 16 * nj + 4, 0)
    assert _raw_skin(L, P, v, j, w, pal.base if pal.base is not None else pal, out) == 0
    _same(out[:poses * n * stride].reshape(poses, n, stride), M.skin(v, j, w, pal, M.NORMAL), "rows")
    assert (_bits(out[poses * n * stride:]) == _bits(SC.SENTINEL_F64)).all()


def test_a_host_joint_out_of_range_is_refused_and_nothing_is_written():
    L = api.load_library()
    v, j, w = SC.mesh(40, 6, 2, 5, seed=12)
    pal = SC.palette(1, 5, 13)
    j[39, 1] = 5
    out = np.full((40, 6), SC.SENTINEL_F64)
    assert _raw_skin(L, api.SkinParams(6, 2, 5, 0, 1, 0, 0), v, j, w, pal, out) == E_INVALID
    assert b"joint" in L.trgl_last_error(None) and (_bits(out) == _bits(SC.SENTINEL_F64)).all()
    with pytest.raises(ValueError):
        M.skin(v, j, w, pal)


def test_skin_stage_error_codes():
    L = api.load_library()
    n, stride, k, nj = 30, 14, 4, 6
    v, j, w = SC.mesh(n, stride, k, nj, seed=21)
    pal = SC.palette(2, nj, 22, pad=2)
    buf = pal.base if pal.base is not None else pal
    out = np.zeros((2, n, stride))

    def call(stride=stride, k=k, nj=nj, flags=7, poses=2, pstride=16 * nj + 2, reserved=0, v=v, j=j, w=w, pal=buf, out=out, n=None, mem=H, params=True):
        return _raw_skin(L, api.SkinParams(stride, k, nj, flags, poses, pstride, reserved), v, j, w, pal, out, n=n, mem=mem, params=params)

    assert call() == 0
    class Off:      # an address 4 (or 1) bytes into an array
        def __init__(self, a, by): self.ctypes = type("c", (), {"data": a.ctypes.data + by}); self.shape = a.shape
    for name, kw in dict(null_params=dict(params=False), bad_mem=dict(mem=7), device_without_context=dict(mem=D), stride_below_3=dict(stride=2, flags=0),
                         no_influences=dict(k=0), nine_influences=dict(k=9), no_joints=dict(nj=0, pstride=0, poses=1), too_many_joints=dict(nj=65537),
                         no_poses=dict(poses=0), palette_stride_below_a_palette=dict(pstride=16 * nj - 1), palette_stride_0_with_two_poses=dict(pstride=0),
                         reserved_set=dict(reserved=1), unknown_flag=dict(flags=8), normal_outside=dict(stride=5, flags=1),
                         tangent_outside=dict(stride=10, flags=2), bitangent_outside=dict(stride=13, flags=4),
                         null_vertices=dict(v=None, n=n), null_joints=dict(j=None), null_weights=dict(w=None), null_palette=dict(pal=None),
                         null_out=dict(out=None), misaligned_vertices=dict(v=Off(v, 4)), misaligned_weights=dict(w=Off(w, 4)),
                         misaligned_joints=dict(j=Off(j, 1)), misaligned_palette=dict(pal=Off(buf, 4)), misaligned_out=dict(out=out.ctypes.data + 4),
                         out_over_vertices=dict(out=v.ctypes.data), out_over_weights=dict(out=w.ctypes.data),
                         out_over_palette=dict(out=buf.ctypes.data + 8 * (16 * nj + 2)), out_over_joints=dict(out=j.ctypes.data)).items():
        before = out.copy()
        assert call(**kw) == E_INVALID, name
        assert L.trgl_last_error(None), name
        assert np.array_equal(_bits(before), _bits(out)), f"{name}: a refused call wrote"
    assert call(n=0, v=None, j=None, w=None, pal=None, out=None) == 0
    assert call(n=0, k=0) == E_INVALID, "the scalars are checked before n_vertices == 0 returns"
    assert call(poses=1, pstride=0) == 0, "one pose needs no palette_stride"
    assert call(n=1 << 62) == E_UNSUPPORTED
    assert C.sizeof(api.SkinParams) == 40


def test_pose_palette_equals_the_model_and_refuses_bad_parents():
    L = api.load_library()
    for kind in ("chain", "star", "forest"):
        for nj in (1, 2, 17, 64):
            for poses in (1, 3):
                parents = SC.hierarchy(kind, nj, seed=nj)
                loc, ib = SC.locals_(poses, nj, seed=100 + nj + poses)
                _same(api.pose_palette(parents, loc, ib), M.pose_palette(parents, loc, ib), f"{kind} {nj} {poses} with inverse_bind")
                _same(api.pose_palette(parents, loc), M.pose_palette(parents, loc), f"{kind} {nj} {poses}")
    parents = SC.hierarchy("forest", 17, 3)
    assert (parents == -1).sum() > 1 and (parents > 0).any()
    loc, ib = SC.locals_(2, 17, 5)
    want = M.pose_palette(parents, loc, ib)
    assert np.isnan(want[0]).any() and np.isfinite(want[1]).all()
    out = np.full((2, 17 * 16 + 3), SC.SENTINEL_F64)

    def call(parents=parents, ib=ib.ctypes.data, nj=17, loc=loc.ctypes.data, ls=16 * 17, poses=2, mem=H, out=out.ctypes.data, ps=16 * 17 + 3):
        return L.trgl_pose_palette(None, None if parents is None else parents.ctypes.data, ib, nj, loc, ls, poses, mem, out, ps)

    assert call() == 0
    _same(out[:, :16 * 17].reshape(2, 17, 16), want, "a padded palette")
    assert (_bits(out[:, 16 * 17:]) == _bits(SC.SENTINEL_F64)).all()
    for bad_at, bad in ((0, 0), (5, 5), (5, 9), (3, -2), (16, 17)):
        p = parents.copy(); p[bad_at] = bad
        before = out.copy()
        assert call(parents=p) == E_INVALID, (bad_at, bad)
        assert b"parent" in L.trgl_last_error(None) and np.array_equal(_bits(before), _bits(out))
        with pytest.raises(ValueError):
            M.pose_palette(p, loc, ib)
    for name, kw in dict(bad_mem=dict(mem=3), device_without_context=dict(mem=D), no_joints=dict(nj=0), local_stride_small=dict(ls=16 * 17 - 1),
                         palette_stride_small=dict(ps=16 * 17 - 1), stride_0_with_two_poses=dict(ps=0), null_parents=dict(parents=None),
                         null_local=dict(loc=None), null_out=dict(out=None), misaligned_local=dict(loc=loc.ctypes.data + 4),
                         misaligned_inverse_bind=dict(ib=ib.ctypes.data + 4), misaligned_out=dict(out=out.ctypes.data + 4),
                         out_over_local=dict(out=loc.ctypes.data + 64), out_over_inverse_bind=dict(out=ib.ctypes.data)).items():
        assert call(**kw) == E_INVALID, name
    assert call(poses=0, parents=None, loc=None, out=None) == 0 and call(poses=0, nj=0) == E_INVALID
    assert call(poses=1, ls=0, ps=0) == 0 and call(ib=None) == 0


# ---- meaning ------------------------------------------------------------------------------------------------------------------------
def test_one_influence_of_weight_one_is_mat_times_vec():
    rng = SC.scenes.SplitMix64(31)
    n = 200
    v, j, w = SC.mesh(n, 8, 1, 9, seed=32, planted=False)
    w[:] = 1.0
    pal = SC.rigid(rng, 9)
    out = api.skin_stage(v, j, w, pal, M.NORMAL)[0]
    m = pal[j[:, 0].astype(np.int64)].reshape(n, 4, 4)
    for r in range(3):
        assert np.array_equal(_bits(out[:, r]), _bits(M.dot4(m[:, r], (v[:, 0], v[:, 1], v[:, 2], 1.0))))
    # the directions come out with unit length and turn with the bone: a rotation with uniform scale keeps the angle to the position's image
    assert np.allclose(np.linalg.norm(out[:, 3:6], axis=1), 1.0, atol=1e-15)
    lin = np.einsum("nij,nj->ni", m[:, :3, :3], v[:, 3:6])
    assert np.allclose(out[:, 3:6], lin / np.linalg.norm(lin, axis=1, keepdims=True), atol=1e-14)


def test_identities_return_the_positions_up_to_minus_zero():
    v, j, w = SC.mesh(300, 6, 4, 5, seed=41, planted=False)
    w[:] = 0.0; w[:, 2] = 1.0
    v[::7, 0] = -0.0
    v[3::7, 2] = 0.0
    pal = np.tile(np.eye(4).reshape(16), (5, 1))
    out = api.skin_stage(v, j, w, pal)[0]
    differ = _bits(out[:, :3]) != _bits(v[:, :3])
    assert np.array_equal(differ, _bits(v[:, :3]) == _bits(np.float64(-0.0))) and differ.any()      # 0.0 + -0.0 is +0.0
    assert (out[:, :3][differ] == 0).all() and np.array_equal(_bits(out[:, 3:]), _bits(v[:, 3:]))


def _coverage(vertices, indices):
    o = orc.Oracle(64, 64, 3)
    o.draw(orc.FLAT, SC.clip_rows(vertices, indices), colors=np.full(len(indices), 0xFFFF0000, np.uint32))
    return (o.fb != 0).any(axis=-1)


def test_a_bent_arm_covers_where_the_bent_arm_is():
    v, idx, j, w, parents, ib = SC.arm()
    straight = api.skin_stage(v, j, w, api.pose_palette(parents, SC.arm_locals(0.0), ib))[0]
    assert np.allclose(straight[:, :3], v[:, :3], atol=1e-15), "bind pose: palette = identities"
    bent = api.skin_stage(v, j, w, api.pose_palette(parents, SC.arm_locals(90.0), ib))[0]
    rest, now = _coverage(v, idx), _coverage(bent, idx)
    # screen: x = 32 + 32 ndc, rows counted from the frame's first row as the oracle stores them; the first bone stays, the rest of
    # the arm now points along +y from the elbow at ndc x = -0.25 (column 24)
    cols = np.arange(64)
    assert rest.sum() > 300 and now.sum() > 300
    assert np.array_equal(rest[:, cols < 20], now[:, cols < 20]) and rest[:, cols < 20].any(), "the first bone did not move"
    assert not now[:, cols >= 30].any(), "the bent arm left pixels where the straight forearm was"
    assert rest[:, cols >= 30].any()
    up = now & ~rest
    assert up.sum() > 150 and up[:, (cols >= 18) & (cols < 30)].sum() == up.sum(), "the forearm should stand over the elbow"
    rows_with = np.flatnonzero(up.any(axis=1))
    assert rows_with.max() - rows_with.min() >= 24, "the forearm and hand are a unit long: 32 rows"
