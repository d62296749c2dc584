"""k_vertex_stage on the head stand-in (327680 faces, indexed): run under rocprofv3 --kernel-trace.

Also times the vertex kernel of a user vertex shader that restates the built-in stage (tests/vertex_shader_sources.RESTATED, K = 24;
csrc/vertex_user.h) against k_vertex_stage: both through trgl_vertex_stage on device arrays, so each timed interval holds exactly one
kernel; alternating runs in one process, HIP events on the context's stream, medians.  A probe, not a test: it prints one JSON line."""
import json
import sys
sys.path.insert(0, '.'); sys.path.insert(0, 'tests')
import numpy as np, torch
from tinyrenderder_amd import scenes
from tinyrenderder_amd.api import Context, PHONG, make_uniforms
import test_next_rows as T
import vertex_shader_sources as V
W = H = 4096
ROUNDS = 50
hd, verts, idx = T._indexed_head(7, W, H)
d, n, s = scenes.procedural_textures(1024)
u = make_uniforms(hd["model_view"], hd["key"], hd["fill"], hd["rim"], 1.0, 0, 1, 2)
dv = torch.from_numpy(verts).cuda(); di = torch.from_numpy(idx.view(np.int32)).cuda()
with Context(W, H, 3) as ctx:
    for slot, t in ((0, d), (1, n), (2, s)): ctx.upload_texture(slot, t)
    for it in range(5):
        ctx.clear(); ctx.draw_indexed(PHONG, u, hd["projection"], dv, di, device=True); ctx.flush(); ctx.sync()
    print("faces", idx.shape[0], "vertices", verts.shape, ctx.stats_line())

    # the user restatement against the built-in kernel
    nf = idx.shape[0]
    vs = ctx.register_vertex_shader(V.RESTATED, 24)
    outs = {k: (torch.empty((nf, 12), dtype=torch.float64, device="cuda"), torch.empty((nf, 24), dtype=torch.float64, device="cuda")) for k in (-1, vs)}
    stream = torch.cuda.ExternalStream(ctx.stream)
    torch.cuda.synchronize()
    ms = {-1: [], vs: []}
    for it in range(ROUNDS + 5):
        for which in (-1, vs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            ctx.vertex_stage(which, u, hd["projection"], dv, di, device=True, out=outs[which])
            e1.record(stream)
            ctx.sync()
            if it >= 5:
                ms[which].append(e0.elapsed_time(e1))
    assert torch.equal(outs[-1][0], outs[vs][0]) and torch.equal(outs[-1][1], outs[vs][1]), "the restatement differs from k_vertex_stage"
    builtin, user = float(np.median(ms[-1])), float(np.median(ms[vs]))
    print(json.dumps(dict(probe="vertex_stage", faces=nf, rounds=ROUNDS, k_vertex_stage_us=round(builtin * 1e3, 2),
                          trgl_vertex_user_us=round(user * 1e3, 2), ratio=round(user / builtin, 3),
                          min_us=[round(min(ms[-1]) * 1e3, 2), round(min(ms[vs]) * 1e3, 2)])))
