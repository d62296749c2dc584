"""Times of trgl_mesh_normals / trgl_mesh_tangents on one MI355X (DESIGN.md §6 records the results).

  python profiles/mesh_attr_probe.py [--reps 50] [--big-faces 10000000]

Two meshes in device memory at stride 14: the 327 k-face head stand-in with shared vertices, and a random mesh of --big-faces faces over
half as many vertices.  Before every timed call the vertex buffer is restored from a device copy (outside the clock), so every call
has work to do; the call is made with a `generated` pointer, so a host clock around it covers the need test, the face vectors, the
sort, the ordered accumulate, the 4-byte copy and the stream sync.  "needs_nothing" times the call on a mesh that is already
prepared (the need test and the library's sort still run).  Next to it, what a caller does today for a device mesh: copy to the host,
the host loop (trgl_mesh_normals with TRGL_MEM_HOST: the loop that shim/trgl_obj.h keeps a copy of), copy back.  The device result is
compared with the host's, bit for bit, before anything is timed.
Warm-up first, then medians over --reps repetitions (fewer for the host path); the spread is printed as min / max.  Under
`rocprofv3 --kernel-trace --stats` the same script lists k_mesh_need, k_face_vectors, the sort's kernels and k_vertex_finish: take
the split between sort and accumulate from that run and the call times from a run without the profiler."""
import argparse
import json
import statistics
import sys
import time

sys.path.insert(0, ".")
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tinyrenderder_amd import api, scenes  # noqa: E402
from tinyrenderder_amd.api import Context  # noqa: E402


def timed(fn, reps, warm=3, before=None):
    ts = []
    for k in range(warm + reps):
        if before:
            before()
        t0 = time.perf_counter(); fn(); dt = time.perf_counter() - t0
        if k >= warm:
            ts.append(dt)
    return dict(median_us=statistics.median(ts) * 1e6, min_us=min(ts) * 1e6, max_us=max(ts) * 1e6, reps=reps)


def head_mesh():
    hd = scenes.head_standin(7, 64, 64)                                     # 327 680 faces
    pos = hd["positions"].reshape(-1, 3)
    uniq, first, inv = np.unique(pos, axis=0, return_index=True, return_inverse=True)
    v = np.zeros((uniq.shape[0], 14)); v[:, 0:3] = uniq; v[:, 6:8] = hd["uvs"].reshape(-1, 2)[first]
    return v, inv.reshape(-1, 3).astype(np.uint32)


def random_mesh(nf):
    rng = np.random.default_rng(7)
    nv = max(3, nf // 2)
    v = np.zeros((nv, 14)); v[:, 0:3] = rng.standard_normal((nv, 3)); v[:, 6:8] = rng.uniform(0, 1, (nv, 2))
    return v, rng.integers(0, nv, (nf, 3)).astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--big-faces", type=int, default=10_000_000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_attr_probe: no GPU; there is nothing to measure without one")
    res = {}
    with Context(64, 64, 3) as ctx:
        for name, (v, i) in (("head_standin", head_mesh()), ("random_%d" % a.big_faces, random_mesh(a.big_faces))):
            di = torch.from_numpy(i.view(np.int32)).cuda()
            for kind, host_fn, dev_fn in (("normals", api.mesh_normals, ctx.mesh_normals), ("tangents", api.mesh_tangents, ctx.mesh_tangents)):
                if kind == "tangents":
                    v = api.mesh_normals(v, i)[0]                          # tangents need normals
                fresh = torch.from_numpy(v).cuda()
                dv = fresh.clone(); torch.cuda.synchronize()
                t0 = time.perf_counter(); want, gen = host_fn(v, i); host_once = time.perf_counter() - t0
                assert gen and dev_fn(dv, di, device=True)[1] is True
                assert np.array_equal(dv.cpu().numpy().view(np.uint64), want.view(np.uint64)), (name, kind)

                def restore():
                    dv.copy_(fresh); torch.cuda.synchronize()

                def through_host():
                    h = dv.cpu().numpy()
                    out, _ = host_fn(h, i)
                    dv.copy_(torch.from_numpy(out)); torch.cuda.synchronize()

                key = "%s_%s" % (kind, name)
                res[key] = dict(n_vertices=int(v.shape[0]), n_faces=int(i.shape[0]), host_loop_once_us=host_once * 1e6,
                                device=timed(lambda: dev_fn(dv, di, device=True), a.reps, before=restore),
                                needs_nothing=timed(lambda: dev_fn(dv, di, device=True), a.reps),
                                copy_host_loop_copy=timed(through_host, max(3, a.reps // 10), warm=1, before=restore))
                del fresh, dv
            del di
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
