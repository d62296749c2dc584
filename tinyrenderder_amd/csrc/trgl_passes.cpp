// trgl_passes.cpp — the optional passes of include/trgl.h over finished frames and over caller-owned images and meshes: SSAO post-process,
// z-buffer snapshots, blur and scale, the box-filter resolve and textures from frames, mip chains and the LOD stage, the shadow mask and modulate, occlusion culling of boxes, world boxes and frustum codes of instances, mesh bounds and attributes in device memory, the two self-tests.
// None of them knows the flush pipeline of trgl_api.cpp: each finishes what is pending (end_pending_raster, trgl_flush, flush_sync), then
// launches on the context's stream.  With TRGL_MEM_HOST the work is done by the host loops (trgl_host.cpp, shim/trgl_image.h).
#include <climits>
#include <cmath>
#include <cstring>
#include <new>

#include "trgl_stage.h"
#include "mip_core.h"
#include "../shim/trgl_image.h"

static int zsnap_slot(trgl_ctx* c, int slot, const char* who) {
    if (slot >= 0 && slot < TRGL_MAX_Z_SNAPSHOTS) return TRGL_OK;
    return fail(c, TRGL_E_INVALID, std::string(who) + ": slot must be 0.." + std::to_string(TRGL_MAX_Z_SNAPSHOTS - 1));
}

// ---- TGAImage::gaussian_blur and TGAImage::scale (tgaimage.cpp:246-324) ------------------------------------------------------------
// The weights of `radius` in c->blur_weights, uploaded on the stream unless the previous blur left the same ones there.
static int upload_blur_weights(trgl_ctx* c, int radius) {
    if (c->blur_radius == radius) return TRGL_OK;
    const size_t n = 2 * (size_t)radius + 1;
    if (!c->ev_blur_w) HIPCHK(c, hipEventCreateWithFlags(&c->ev_blur_w, hipEventDisableTiming));
    HIPCHK(c, hipEventSynchronize(c->ev_blur_w));            // the previous upload has read the pinned weights (no wait when none was queued)
    c->blur_radius = 0;
    if (n > c->blur_w_pinned_cap) {
        if (c->blur_w_pinned) { HIPCHK(c, hipHostFree(c->blur_w_pinned)); c->blur_w_pinned = nullptr; c->blur_w_pinned_cap = 0; }
        HIPCHK(c, hipHostMalloc((void**)&c->blur_w_pinned, headroom(n) * sizeof(float)));
        c->blur_w_pinned_cap = headroom(n);
    }
    if (int r = c->blur_weights.grow(c, n)) return r;
    trgl_image::gaussian_weights(radius, c->blur_w_pinned);
    HIPCHK(c, hipMemcpyAsync(c->blur_weights.p, c->blur_w_pinned, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipEventRecord(c->ev_blur_w, c->stream));
    c->blur_radius = radius;
    return TRGL_OK;
}

// both passes of the blur over device memory, queued on the stream; nbytes = w * h * bpp
static int queue_blur(trgl_ctx* c, uint8_t* pixels, int w, int h, int bpp, int radius, size_t nbytes) {
    int r = upload_blur_weights(c, radius); if (r) return r;
    if ((r = c->blur_tmp.grow(c, nbytes))) return r;
    launch_image_blur(c->stream, pixels, w, h, bpp, radius, c->blur_weights.p, c->blur_tmp.p);
    HIPCHK(c, hipGetLastError());
    return TRGL_OK;
}

// ---- box-filter resolve and frames as textures (include/trgl.h; host loop in trgl_host.cpp, kernel in kernels_resolve.hip) ------------
// what trgl_image_downsample checks of an image and a factor, for every call that filters (mem_kind, the pointers and overlap: the caller)
static int check_box(trgl_ctx* c, const std::string& who, int w, int h, int bpp, int factor) {
    if (!(bpp == 1 || bpp == 3 || bpp == 4)) return fail(c, TRGL_E_INVALID, who + ": bpp must be 1, 3 or 4");
    if (factor < 1 || factor > TRGL_MAX_BOX_FACTOR) return fail(c, TRGL_E_INVALID, who + ": factor must be 1.." + std::to_string(TRGL_MAX_BOX_FACTOR));
    if (w < factor || h < factor) return fail(c, TRGL_E_INVALID, who + ": w / factor or h / factor is 0");
    if ((int64_t)w * h * bpp > INT_MAX) return fail(c, TRGL_E_UNSUPPORTED, who + ": w * h * bpp above INT_MAX");
    return TRGL_OK;
}
static bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    return (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na;
}
static int texture_slot(trgl_ctx* c, int slot, const char* who) {
    if (slot >= 0 && slot < TRGL_MAX_TEXTURES) return TRGL_OK;
    return fail(c, TRGL_E_INVALID, std::string(who) + ": slot must be 0.." + std::to_string(TRGL_MAX_TEXTURES - 1));
}

// The box filter of a device image (the resident frame or a caller's) into texture `slot`, all of it in stream order.  A slot that holds
// a texture of the result's size keeps its memory and its entry in tex_dev; an empty slot gets memory by the sampler's rule (bytes + 8,
// the tail zeroed: the samplers read each texel as one 4-byte load) and enters the table through a kernel on the stream - never a host
// write that races a running flush; a slot of another size is released first, behind a wait for the stream.
static int texture_from_device(trgl_ctx* c, const std::string& who, int slot, const uint8_t* src, int w, int h, int bpp, int factor) {
    const int w2 = w / factor, h2 = h / factor;
    const size_t bytes = (size_t)w2 * h2 * bpp;
    DevTexture& t = c->tex_host[slot];
    const bool reuse = t.data && t.w == w2 && t.h == h2 && t.bpp == bpp;
    if (reuse && ranges_overlap(src, (size_t)w * h * bpp, t.data, bytes)) return fail(c, TRGL_E_INVALID, who + ": the source is the slot's own texture");
    int r = end_pending_raster(c); if (r) return r;
    if ((r = trgl_flush(c))) return r;                // draws submitted earlier sample what the slot held; a pending clear reaches the frame
    if (!reuse) {
        if (t.data) {
            HIPCHK(c, hipStreamSynchronize(c->stream));
            HIPCHK(c, hipFree((void*)t.data));
            t = DevTexture{ nullptr, 0, 0, 0, 0 };
            c->tex_cap[slot] = 0;
        }
        uint8_t* d = nullptr;
        if (hipMalloc((void**)&d, bytes + 8) != hipSuccess) {
            (void)hipGetLastError();
            HIPCHK(c, launch_set_texture(c->stream, c->tex_dev.p, slot, t));
            return fail(c, TRGL_E_NOMEM, who + ": out of device memory");
        }
        t = DevTexture{ d, w2, h2, bpp, 0 };
        c->tex_cap[slot] = bytes + 8;
        HIPCHK(c, hipMemsetAsync(d + bytes, 0, 8, c->stream));
        HIPCHK(c, launch_set_texture(c->stream, c->tex_dev.p, slot, t));
    } else if (t.pad) {      // new texels: one level until trgl_texture_mipmaps is called again (the levels' memory stays with the slot)
        t.pad = 0;
        HIPCHK(c, launch_set_texture(c->stream, c->tex_dev.p, slot, t));
    }
    HIPCHK(c, launch_box_filter(c->stream, src, w, h, bpp, factor, const_cast<uint8_t*>(t.data)));
    return TRGL_OK;
}

// ---- the shadow post-pass (include/trgl.h; host loops in shim/trgl_image.h, kernels in kernels_shadow.hip) ----------------------------
static int check_shadow_params(trgl_ctx* c, const char* who, const trgl_shadow_params* p) {
    const std::string w(who);
    if (!p) return fail(c, TRGL_E_INVALID, w + ": params is null");
    if (p->pcf_radius < 0 || p->pcf_radius > TRGL_MAX_PCF_RADIUS || p->reserved != 0)
        return fail(c, TRGL_E_INVALID, w + ": need pcf_radius in 0.." + std::to_string(TRGL_MAX_PCF_RADIUS) + " and reserved == 0");
    if (!(p->darkness >= 0.0 && p->darkness <= 1.0) || !std::isfinite(p->bias))
        return fail(c, TRGL_E_INVALID, w + ": need darkness in [0, 1] and a finite bias");
    return TRGL_OK;
}

static ShadowArgs shadow_args(const trgl_shadow_params* p, const double* depth, int w, int h, const double* map, int map_w, int map_h, uint8_t* mask) {
    ShadowArgs a;
    std::memcpy(a.M, p->screen_to_light, sizeof(a.M));
    a.bias = p->bias; a.darkness = p->darkness;
    a.depth = depth; a.map = map; a.mask = mask;
    a.w = w; a.h = h; a.map_w = map_w; a.map_h = map_h; a.radius = p->pcf_radius;
    return a;
}

// ---- occlusion culling of boxes (include/trgl.h; host loop in trgl_host.cpp, kernels in kernels_occlusion.hip) ------------------------
// Both kernels over device arrays, queued on the stream: the levels of the depths, then one wavefront per box.  n > 0, w * h <= INT_MAX.
static int queue_occlusion(trgl_ctx* c, const double* depth, int w, int h, const double* viewport, const double* view_proj,
                           const double* boxes, uint64_t n, uint8_t* codes) {
    OcclArgs a;
    std::memcpy(a.M, view_proj, sizeof(a.M));
    std::memcpy(a.V, viewport, sizeof(a.V));
    a.depth = depth; a.levels = nullptr; a.boxes = boxes; a.codes = codes; a.n = n; a.w = w; a.h = h;
    if (w > 0 && h > 0) {
        if (int r = c->occl_levels.grow(c, occl_level_doubles(w, h))) return r;
        launch_occl_build(c->stream, depth, w, h, c->occl_levels.p);
        a.levels = c->occl_levels.p;
    }
    launch_occl_query(c->stream, a);
    HIPCHK(c, hipGetLastError());
    return TRGL_OK;
}

// ---- Model::generateNormalsIfNeeded (model.cpp:269-316) and Model::computeTangentsIfNeeded (model.cpp:318-388) ----------------------
static int mesh_attr(trgl_ctx* c, bool tangents, double* vertices, int stride, uint64_t n, const uint32_t* indices, uint64_t nfaces,
                     int mem_kind, int* generated) {
    const std::string who = tangents ? "trgl_mesh_tangents: " : "trgl_mesh_normals: ";
    if (!valid_mem_kind(mem_kind)) return fail(c, TRGL_E_INVALID, who + "bad mem_kind");
    if (stride < (tangents ? 14 : 6)) return fail(c, TRGL_E_INVALID, who + (tangents ? "vertex stride must be >= 14 doubles (pos3, normal3, uv2, tangent3, bitangent3)"
                                                                                      : "vertex stride must be >= 6 doubles (pos3, normal3)"));
    if (nfaces > 0xffffffffull / 3) return fail(c, TRGL_E_INVALID, who + "3 * n_faces must fit in 32 bits");
    if (mem_kind == TRGL_MEM_DEVICE && !c) return fail(c, TRGL_E_INVALID, who + "TRGL_MEM_DEVICE needs a context");
    if (generated) *generated = 0;
    if (n == 0) return TRGL_OK;
    if (!vertices) return fail(c, TRGL_E_INVALID, who + "vertices is null");
    if (nfaces && !indices) return fail(c, TRGL_E_INVALID, who + "indices is null");
    if (mem_kind == TRGL_MEM_HOST) {
        const int g = host_mesh_attr(tangents, vertices, stride, n, indices, nfaces);
        if (g < 0) return fail(c, TRGL_E_INVALID, who + "index out of range");
        if (generated) *generated = g;
        return TRGL_OK;
    }
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    size_t bytes = 0;
    HIPCHK(c, mesh_attr_scratch_bytes(n, (uint32_t)nfaces, &bytes));
    if ((r = c->mesh_scratch.grow(c, bytes))) return r;
    const uint32_t* flag = nullptr;
    HIPCHK(c, launch_mesh_attr(c->stream, tangents, vertices, stride, n, indices, (uint32_t)nfaces, c->mesh_scratch.p, c->mesh_scratch.cap, &flag));
    if (generated) {
        uint32_t word = 0;
        HIPCHK(c, hipMemcpyAsync(&word, flag, sizeof(word), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        *generated = word ? 1 : 0;
    }
    return TRGL_OK;
}

extern "C" {

int trgl_postprocess(trgl_ctx* c, const trgl_ssao_params* params, uint8_t* zimg, uint8_t* ao, uint8_t* fin) {
    CHKCTX(c);
    trgl_ssao_params sp; trgl_ssao_defaults(&sp);
    if (params) sp = *params;
    if (sp.num_directions < 1 || sp.num_directions > 16 || sp.steps_per_direction < 1)
        return fail(c, TRGL_E_INVALID, "trgl_postprocess: 1..16 directions, >= 1 step");
    int r = flush_sync(c); if (r) return r;
    const size_t npx = (size_t)c->W * c->H;
    // three [H][W][3] images, each at a 16-byte boundary (the kernels store dwords: W * H need not be a multiple of 4), then the keys
    const size_t img = (npx * 3 + 15) & ~size_t(15);
    if ((r = c->pp_out.grow(c, img * 3 + 64))) return r;      // allocated once per context, not per call
    uint8_t* d_out = c->pp_out.p;
    unsigned long long* d_keys = reinterpret_cast<unsigned long long*>(d_out + img * 3);
    uint8_t* d_z = d_out; uint8_t* d_ao = d_out + img; uint8_t* d_fin = d_out + img * 2;
    hipStream_t s = c->stream;
    if (zimg) launch_zimage(s, c->zb.p, c->W, c->H, d_keys, d_z);
    if (ao || fin) {
        double dx[16], dy[16];
        for (int d = 0; d < sp.num_directions; ++d) {         // main.cpp:333-334, host libm as in the reference
            double angle = 2.0 * 3.14159265358979323846 * d / sp.num_directions;
            dx[d] = std::cos(angle); dy[d] = std::sin(angle);
        }
        launch_ssao(s, c->zb.p, c->W, c->H, dx, dy, sp.num_directions, sp.steps_per_direction, sp.sample_radius,
                    sp.occlusion_threshold, sp.intensity, d_ao);
    }
    if (fin) {
        if (c->bpp < 3) return fail(c, TRGL_E_UNSUPPORTED, "trgl_postprocess: composite needs an RGB(A) framebuffer");
        launch_composite(s, c->fb.p, c->bpp, d_ao, c->W, c->H, d_fin);
    }
    HIPCHK(c, hipGetLastError());
    if (zimg) HIPCHK(c, hipMemcpyAsync(zimg, d_z, npx * 3, hipMemcpyDeviceToHost, s));
    if (ao) HIPCHK(c, hipMemcpyAsync(ao, d_ao, npx * 3, hipMemcpyDeviceToHost, s));
    if (fin) HIPCHK(c, hipMemcpyAsync(fin, d_fin, npx * 3, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return TRGL_OK;
}

// ---- scene logic around the draws (model.cpp:15-40) -----------------------------------------------------------------------------------
int trgl_mesh_bounds(trgl_ctx* c, const double* vertices, int stride, uint64_t n, int mem_kind, double out_min[3], double out_max[3]) {
    if (!out_min || !out_max) return fail(c, TRGL_E_INVALID, "trgl_mesh_bounds: null output");
    if (!valid_mem_kind(mem_kind)) return fail(c, TRGL_E_INVALID, "trgl_mesh_bounds: bad mem_kind");
    if (stride < 3) return fail(c, TRGL_E_INVALID, "trgl_mesh_bounds: vertex stride must be >= 3 doubles (the position)");
    if (n && !vertices) return fail(c, TRGL_E_INVALID, "trgl_mesh_bounds: vertices is null");
    if (mem_kind == TRGL_MEM_DEVICE && !c) return fail(c, TRGL_E_INVALID, "trgl_mesh_bounds: TRGL_MEM_DEVICE needs a context");
    if (n == 0) {                                                               // model.cpp:16-19
        for (int a = 0; a < 3; ++a) out_min[a] = out_max[a] = 0.0;
        return TRGL_OK;
    }
    if (mem_kind == TRGL_MEM_HOST) { host_mesh_bounds(vertices, stride, n, out_min, out_max); return TRGL_OK; }
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    if (!c->bounds_scratch.p && (r = c->bounds_scratch.alloc(c, 1 + MESH_BOUNDS_MAX_BLOCKS))) return r;
    launch_mesh_bounds(c->stream, vertices, stride, n, c->bounds_scratch.p);
    HIPCHK(c, hipGetLastError());
    double res[6];
    HIPCHK(c, hipMemcpyAsync(res, c->bounds_scratch.p->v, sizeof(res), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int a = 0; a < 3; ++a) { out_min[a] = res[a]; out_max[a] = res[3 + a]; }
    return TRGL_OK;
}

int trgl_mesh_normals(trgl_ctx* c, double* vertices, int stride, uint64_t n, const uint32_t* indices, uint64_t nfaces, int mem_kind, int* generated) {
    return mesh_attr(c, false, vertices, stride, n, indices, nfaces, mem_kind, generated);
}
int trgl_mesh_tangents(trgl_ctx* c, double* vertices, int stride, uint64_t n, const uint32_t* indices, uint64_t nfaces, int mem_kind, int* generated) {
    return mesh_attr(c, true, vertices, stride, n, indices, nfaces, mem_kind, generated);
}

int trgl_zbuffer_snapshot(trgl_ctx* c, int slot) {
    CHKCTX(c);
    int r = zsnap_slot(c, slot, "trgl_zbuffer_snapshot"); if (r) return r;
    if ((r = trgl_flush(c))) return r;                // completes a begun flush, draws what is queued, runs a pending clear
    const size_t npx = (size_t)c->W * c->H;
    if (!c->zsnap[slot].p && c->zsnap[slot].alloc(c, npx)) return fail(c, TRGL_E_NOMEM, "trgl_zbuffer_snapshot: out of device memory");
    HIPCHK(c, hipMemcpyAsync(c->zsnap[slot].p, c->zb.p, npx * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    return TRGL_OK;
}

int trgl_zbuffer_restore(trgl_ctx* c, int slot) {
    CHKCTX(c);
    int r = zsnap_slot(c, slot, "trgl_zbuffer_restore"); if (r) return r;
    if (!c->zsnap[slot].p) return fail(c, TRGL_E_STATE, "trgl_zbuffer_restore: the slot holds no snapshot");
    if ((r = trgl_flush(c))) return r;                // what is queued was submitted against the depths as they are now
    HIPCHK(c, hipMemcpyAsync(c->zb.p, c->zsnap[slot].p, (size_t)c->W * c->H * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    return TRGL_OK;
}

int trgl_zbuffer_snapshot_free(trgl_ctx* c, int slot) {
    CHKCTX(c);
    int r = zsnap_slot(c, slot, "trgl_zbuffer_snapshot_free"); if (r) return r;
    if ((r = end_pending_raster(c))) return r;
    return c->zsnap[slot].release(c);
}

int trgl_image_blur(trgl_ctx* c, uint8_t* pixels, int w, int h, int bpp, int radius, int mem_kind) {
    if (!valid_mem_kind(mem_kind)) return fail(c, TRGL_E_INVALID, "trgl_image_blur: bad mem_kind");
    if (!(bpp == 1 || bpp == 3 || bpp == 4) || w < 0 || h < 0) return fail(c, TRGL_E_INVALID, "trgl_image_blur: need w, h >= 0 and bpp in {1, 3, 4}");
    if (mem_kind == TRGL_MEM_DEVICE && !c) return fail(c, TRGL_E_INVALID, "trgl_image_blur: TRGL_MEM_DEVICE needs a context");
    if (radius <= 0 || w == 0 || h == 0) return TRGL_OK;                         // tgaimage.cpp:272
    if (!pixels) return fail(c, TRGL_E_INVALID, "trgl_image_blur: pixels is null");
    if (radius > TRGL_MAX_BLUR_RADIUS) return fail(c, TRGL_E_UNSUPPORTED, "trgl_image_blur: radius above 46340 (i * i overflows the reference's int)");
    if ((int64_t)w * h * bpp > INT_MAX) return fail(c, TRGL_E_UNSUPPORTED, "trgl_image_blur: w * h * bpp above INT_MAX (the reference's int byte index overflows)");
    const size_t nbytes = (size_t)w * h * bpp;
    if (mem_kind == TRGL_MEM_HOST) {
        try {
            std::vector<float> weights(2 * (size_t)radius + 1);
            std::vector<uint8_t> tmp(nbytes);
            trgl_image::gaussian_weights(radius, weights.data());
            trgl_image::blur_bytes(pixels, w, h, bpp, radius, weights.data(), tmp.data());
        } catch (const std::bad_alloc&) { return fail(c, TRGL_E_NOMEM, "trgl_image_blur: out of memory"); }
        return TRGL_OK;
    }
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    return queue_blur(c, pixels, w, h, bpp, radius, nbytes);
}

int trgl_image_scale(trgl_ctx* c, const uint8_t* src, int w, int h, int bpp, uint8_t* dst, int w2, int h2, int mem_kind) {
    if (!valid_mem_kind(mem_kind)) return fail(c, TRGL_E_INVALID, "trgl_image_scale: bad mem_kind");
    if (!(bpp == 1 || bpp == 3 || bpp == 4)) return fail(c, TRGL_E_INVALID, "trgl_image_scale: bpp must be 1, 3 or 4");
    if (mem_kind == TRGL_MEM_DEVICE && !c) return fail(c, TRGL_E_INVALID, "trgl_image_scale: TRGL_MEM_DEVICE needs a context");
    if (w2 <= 0 || h2 <= 0 || w <= 0 || h <= 0) return fail(c, TRGL_E_INVALID, "trgl_image_scale: a size <= 0 or an empty source (the reference returns false)");   // tgaimage.cpp:247
    if (!src || !dst) return fail(c, TRGL_E_INVALID, "trgl_image_scale: null image");
    if ((int64_t)(w2 - 1) * w > INT_MAX || (int64_t)(h2 - 1) * h > INT_MAX || (int64_t)w2 * h2 * bpp > INT_MAX || (int64_t)w * h * bpp > INT_MAX)
        return fail(c, TRGL_E_UNSUPPORTED, "trgl_image_scale: (w2 - 1) * w, (h2 - 1) * h or a byte count above INT_MAX (the reference's int arithmetic overflows)");
    const size_t nsrc = (size_t)w * h * bpp, ndst = (size_t)w2 * h2 * bpp;
    if ((uintptr_t)src < (uintptr_t)dst + ndst && (uintptr_t)dst < (uintptr_t)src + nsrc) return fail(c, TRGL_E_INVALID, "trgl_image_scale: src and dst overlap");
    if (mem_kind == TRGL_MEM_HOST) { trgl_image::scale_bytes(src, w, h, bpp, dst, w2, h2); return TRGL_OK; }
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    launch_image_scale(c->stream, src, w, h, bpp, dst, w2, h2);
    HIPCHK(c, hipGetLastError());
    return TRGL_OK;
}

int trgl_framebuffer_blur(trgl_ctx* c, int radius) {
    CHKCTX(c);
    if (!owns_whole_frame(c))
        return fail(c, TRGL_E_STATE, "trgl_framebuffer_blur: the context owns a strip or interleaved bands; the vertical pass would read rows of another rank");
    if (radius <= 0) return TRGL_OK;                                             // tgaimage.cpp:272
    if (radius > TRGL_MAX_BLUR_RADIUS) return fail(c, TRGL_E_UNSUPPORTED, "trgl_framebuffer_blur: radius above 46340 (i * i overflows the reference's int)");
    if ((int64_t)c->W * c->H * c->bpp > INT_MAX) return fail(c, TRGL_E_UNSUPPORTED, "trgl_framebuffer_blur: W * H * bpp above INT_MAX (the reference's int byte index overflows)");
    int r = trgl_flush(c); if (r) return r;          // completes a begun flush, draws what is queued, runs a pending clear
    return queue_blur(c, c->fb.p, c->W, c->H, c->bpp, radius, (size_t)c->W * c->H * c->bpp);
}

int trgl_image_downsample(trgl_ctx* c, const uint8_t* src, int w, int h, int bpp, int factor, uint8_t* dst, int mem_kind) {
    if (int r = check_mem(c, "trgl_image_downsample: ", mem_kind)) return r;
    if (int r = check_box(c, "trgl_image_downsample", w, h, bpp, factor)) return r;
    if (!src || !dst) return fail(c, TRGL_E_INVALID, "trgl_image_downsample: null image");
    if (ranges_overlap(src, (size_t)w * h * bpp, dst, (size_t)(w / factor) * (h / factor) * bpp))
        return fail(c, TRGL_E_INVALID, "trgl_image_downsample: src and dst overlap");
    if (mem_kind == TRGL_MEM_HOST) { host_box_filter(src, w, h, bpp, factor, dst); return TRGL_OK; }
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    HIPCHK(c, launch_box_filter(c->stream, src, w, h, bpp, factor, dst));
    return TRGL_OK;
}

int trgl_framebuffer_resolve(trgl_ctx* c, int factor, uint8_t* dst, int mem_kind) {
    CHKCTX(c);
    if (!valid_mem_kind(mem_kind)) return fail(c, TRGL_E_INVALID, "trgl_framebuffer_resolve: bad mem_kind");
    if (!owns_whole_frame(c))
        return fail(c, TRGL_E_STATE, "trgl_framebuffer_resolve: the context owns a strip or interleaved bands; its frame holds only this rank's rows (gather the frame and resolve it on one context)");
    int r = check_box(c, "trgl_framebuffer_resolve", c->W, c->H, c->bpp, factor); if (r) return r;
    if (!dst) return fail(c, TRGL_E_INVALID, "trgl_framebuffer_resolve: dst is null");
    const size_t nsrc = (size_t)c->W * c->H * c->bpp, ndst = (size_t)(c->W / factor) * (c->H / factor) * c->bpp;
    if (mem_kind == TRGL_MEM_DEVICE && ranges_overlap(c->fb.p, nsrc, dst, ndst)) return fail(c, TRGL_E_INVALID, "trgl_framebuffer_resolve: dst lies inside the frame");
    if ((r = trgl_flush(c))) return r;                // completes a begun flush, draws what is queued, runs a pending clear
    if (mem_kind == TRGL_MEM_HOST && factor == 1) {   // the bytes of trgl_read_framebuffer
        HIPCHK(c, hipMemcpyAsync(dst, c->fb.p, nsrc, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return TRGL_OK;
    }
    uint8_t* d_dst = dst;
    if (mem_kind == TRGL_MEM_HOST) { if ((r = c->resolve_tmp.grow(c, ndst))) return r; d_dst = c->resolve_tmp.p; }
    HIPCHK(c, launch_box_filter(c->stream, c->fb.p, c->W, c->H, c->bpp, factor, d_dst));
    if (mem_kind == TRGL_MEM_HOST) {
        HIPCHK(c, hipMemcpyAsync(dst, d_dst, ndst, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return TRGL_OK;
}

int trgl_texture_from_image(trgl_ctx* c, int slot, const uint8_t* src, int w, int h, int bpp, int factor, int mem_kind) {
    CHKCTX(c);
    if (!valid_mem_kind(mem_kind)) return fail(c, TRGL_E_INVALID, "trgl_texture_from_image: bad mem_kind");
    int r = texture_slot(c, slot, "trgl_texture_from_image"); if (r) return r;
    if ((r = check_box(c, "trgl_texture_from_image", w, h, bpp, factor))) return r;
    if (!src) return fail(c, TRGL_E_INVALID, "trgl_texture_from_image: src is null");
    if (mem_kind == TRGL_MEM_DEVICE) return texture_from_device(c, "trgl_texture_from_image", slot, src, w, h, bpp, factor);
    if (factor == 1) return trgl_upload_texture(c, slot, src, w, h, bpp);
    try {
        std::vector<uint8_t> tmp((size_t)(w / factor) * (h / factor) * bpp);
        host_box_filter(src, w, h, bpp, factor, tmp.data());
        return trgl_upload_texture(c, slot, tmp.data(), w / factor, h / factor, bpp);
    } catch (const std::bad_alloc&) { return fail(c, TRGL_E_NOMEM, "trgl_texture_from_image: out of memory"); }
}

int trgl_texture_from_framebuffer(trgl_ctx* c, int slot, int factor) {
    CHKCTX(c);
    int r = texture_slot(c, slot, "trgl_texture_from_framebuffer"); if (r) return r;
    if (!owns_whole_frame(c))
        return fail(c, TRGL_E_STATE, "trgl_texture_from_framebuffer: the context owns a strip or interleaved bands; its frame holds only this rank's rows (gather the frame and capture it on one context)");
    if ((r = check_box(c, "trgl_texture_from_framebuffer", c->W, c->H, c->bpp, factor))) return r;
    return texture_from_device(c, "trgl_texture_from_framebuffer", slot, c->fb.p, c->W, c->H, c->bpp, factor);
}

// ---- mipmapped textures (include/trgl.h; host loops in trgl_host.cpp, kernels in kernels_mip.hip, the arithmetic in mip_core.h) ----------
int trgl_image_mipmaps(trgl_ctx* c, const uint8_t* src, int w, int h, int bpp, uint8_t* dst, int mem_kind) {
    if (int r = check_mem(c, "trgl_image_mipmaps: ", mem_kind)) return r;
    int L = 0; size_t total = 0;
    if (int r = trgl_mip_layout(w, h, bpp, &L, nullptr, nullptr, nullptr, &total)) return c ? fail(c, r, std::string("trgl_image_mipmaps: ") + trgl_last_error(nullptr)) : r;
    if (!src) return fail(c, TRGL_E_INVALID, "trgl_image_mipmaps: src is null");
    if (L == 1) return TRGL_OK;
    if (!dst) return fail(c, TRGL_E_INVALID, "trgl_image_mipmaps: dst is null");
    if (ranges_overlap(src, (size_t)w * h * bpp, dst, total)) return fail(c, TRGL_E_INVALID, "trgl_image_mipmaps: src and dst overlap");
    if (mem_kind == TRGL_MEM_HOST) { host_mipmaps(src, w, h, bpp, dst); return TRGL_OK; }
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    HIPCHK(c, launch_mip_chain(c->stream, src, w, h, bpp, dst, false));
    return TRGL_OK;
}

int trgl_texture_mipmaps(trgl_ctx* c, int slot) {
    CHKCTX(c);
    int r = texture_slot(c, slot, "trgl_texture_mipmaps"); if (r) return r;
    DevTexture& t = c->tex_host[slot];
    if (!t.data || t.w <= 0 || t.h <= 0) return fail(c, TRGL_E_STATE, "trgl_texture_mipmaps: the slot holds no texture");
    if (t.w > 65535 || t.h > 65535) return fail(c, TRGL_E_UNSUPPORTED, "trgl_texture_mipmaps: a side above 65535");
    if ((r = end_pending_raster(c))) return r;
    if ((r = trgl_flush(c))) return r;                // draws submitted earlier sample one level
    const int L = mip_levels(t.w, t.h);
    if (L == 1) return TRGL_OK;
    const size_t bytes0 = (size_t)t.w * t.h * t.bpp, need = mip_slot_offset(t.w, t.h, t.bpp, L);
    if (c->tex_cap[slot] < need) {
        // the first build on this slot: room for the levels behind level 0, every byte between and behind them zero (the samplers'
        // 4-byte loads), level 0 copied over on the stream; the old memory goes behind a wait
        uint8_t* d = nullptr;
        if (hipMalloc((void**)&d, need) != hipSuccess) { (void)hipGetLastError(); return fail(c, TRGL_E_NOMEM, "trgl_texture_mipmaps: out of device memory"); }
        const DevTexture nt{ d, t.w, t.h, t.bpp, 0 };
        hipError_t e = hipMemsetAsync(d + bytes0, 0, need - bytes0, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d, t.data, bytes0, hipMemcpyDeviceToDevice, c->stream);
        if (e == hipSuccess) e = launch_set_texture(c->stream, c->tex_dev.p, slot, nt);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) { (void)hipFree(d); HIPCHK(c, e); }
        HIPCHK(c, hipFree((void*)t.data));
        t = nt;
        c->tex_cap[slot] = need;
    }
    HIPCHK(c, launch_mip_chain(c->stream, t.data, t.w, t.h, t.bpp, const_cast<uint8_t*>(t.data), true));
    t.pad = L - 1;
    HIPCHK(c, launch_set_texture(c->stream, c->tex_dev.p, slot, t));
    return TRGL_OK;
}

int trgl_lod_stage(trgl_ctx* c, const double viewport[16], const double* clip, double* vary, uint64_t n, int K,
                   int uv_offset, int out_offset, int mem_kind) {
    const std::string w = "trgl_lod_stage: ";
    if (int r = check_mem(c, w, mem_kind)) return r;
    if (!viewport) return fail(c, TRGL_E_INVALID, w + "viewport is null");
    if (K < 0 || K > TRGL_MAX_USER_VARY) return fail(c, TRGL_E_INVALID, w + "K outside 0..TRGL_MAX_USER_VARY");
    if (uv_offset < 0 || out_offset < 0 || uv_offset > K - 6 || out_offset > K - 4 || (uv_offset < out_offset + 4 && out_offset < uv_offset + 6))
        return fail(c, TRGL_E_INVALID, w + "need uv_offset + 6 <= K, out_offset + 4 <= K and ranges that do not overlap");
    if (n > 0x7fffffffull) return fail(c, TRGL_E_UNSUPPORTED, w + "2^31 or more triangles in one call");
    if (n == 0) return TRGL_OK;
    if (!clip || !vary) return fail(c, TRGL_E_INVALID, w + "null array");
    if (((uintptr_t)clip | (uintptr_t)vary) & 7) return fail(c, TRGL_E_INVALID, w + "arrays must be 8-byte aligned");
    if (mem_kind == TRGL_MEM_HOST) { host_lod_stage(viewport, clip, vary, n, K, uv_offset, out_offset); return TRGL_OK; }
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    HIPCHK(c, launch_lod_stage(c->stream, viewport, clip, vary, (uint32_t)n, K, uv_offset, out_offset));
    return TRGL_OK;
}

int trgl_shadow_mask_image(trgl_ctx* c, const trgl_shadow_params* params, const double* depth, int w, int h,
                           const double* map, int map_w, int map_h, uint8_t* mask, int mem_kind) {
    if (!valid_mem_kind(mem_kind)) return fail(c, TRGL_E_INVALID, "trgl_shadow_mask_image: bad mem_kind");
    if (int r = check_shadow_params(c, "trgl_shadow_mask_image", params)) return r;
    if (w < 0 || h < 0 || map_w < 0 || map_h < 0) return fail(c, TRGL_E_INVALID, "trgl_shadow_mask_image: a negative dimension");
    if (mem_kind == TRGL_MEM_DEVICE && !c) return fail(c, TRGL_E_INVALID, "trgl_shadow_mask_image: TRGL_MEM_DEVICE needs a context");
    if (w == 0 || h == 0) return TRGL_OK;
    if (map_w == 0 || map_h == 0) return fail(c, TRGL_E_INVALID, "trgl_shadow_mask_image: an empty depth map");
    if (!depth || !map || !mask) return fail(c, TRGL_E_INVALID, "trgl_shadow_mask_image: null array");
    if ((int64_t)w * h > INT_MAX || (int64_t)map_w * map_h > INT_MAX) return fail(c, TRGL_E_UNSUPPORTED, "trgl_shadow_mask_image: w * h or map_w * map_h above INT_MAX");
    if (mem_kind == TRGL_MEM_HOST) {
        trgl_image::shadow_mask_bytes(depth, w, h, params->screen_to_light, map, map_w, map_h, params->bias, params->darkness, params->pcf_radius, mask);
        return TRGL_OK;
    }
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    launch_shadow_mask(c->stream, shadow_args(params, depth, w, h, map, map_w, map_h, mask));
    HIPCHK(c, hipGetLastError());
    return TRGL_OK;
}

int trgl_shadow_mask(trgl_ctx* c, const trgl_shadow_params* params, int slot, uint8_t* mask, int mask_mem_kind) {
    CHKCTX(c);
    if (!valid_mem_kind(mask_mem_kind)) return fail(c, TRGL_E_INVALID, "trgl_shadow_mask: bad mask_mem_kind");
    int r = check_shadow_params(c, "trgl_shadow_mask", params); if (r) return r;
    if ((r = zsnap_slot(c, slot, "trgl_shadow_mask"))) return r;
    if (!mask) return fail(c, TRGL_E_INVALID, "trgl_shadow_mask: mask is null");
    if (!owns_whole_frame(c))
        return fail(c, TRGL_E_STATE, "trgl_shadow_mask: the context owns a strip or interleaved bands; its snapshot holds only this rank's rows (gather with with_z and mask on one context)");
    if (!c->zsnap[slot].p) return fail(c, TRGL_E_STATE, "trgl_shadow_mask: the slot holds no snapshot");
    const size_t npx = (size_t)c->W * c->H;
    if (npx > (size_t)INT_MAX) return fail(c, TRGL_E_UNSUPPORTED, "trgl_shadow_mask: W * H above INT_MAX");
    if ((r = trgl_flush(c))) return r;                // completes a begun flush, draws what is queued, runs a pending clear
    uint8_t* d_mask = mask;
    if (mask_mem_kind == TRGL_MEM_HOST) { if ((r = c->shadow_tmp.grow(c, npx))) return r; d_mask = c->shadow_tmp.p; }
    launch_shadow_mask(c->stream, shadow_args(params, c->zb.p, c->W, c->H, c->zsnap[slot].p, c->W, c->H, d_mask));
    HIPCHK(c, hipGetLastError());
    if (mask_mem_kind == TRGL_MEM_HOST) {
        HIPCHK(c, hipMemcpyAsync(mask, d_mask, npx, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return TRGL_OK;
}

int trgl_image_modulate(trgl_ctx* c, uint8_t* pixels, int w, int h, int bpp, const uint8_t* mask, int mem_kind) {
    if (!valid_mem_kind(mem_kind)) return fail(c, TRGL_E_INVALID, "trgl_image_modulate: bad mem_kind");
    if (!(bpp == 1 || bpp == 3 || bpp == 4) || w < 0 || h < 0) return fail(c, TRGL_E_INVALID, "trgl_image_modulate: need w, h >= 0 and bpp in {1, 3, 4}");
    if (mem_kind == TRGL_MEM_DEVICE && !c) return fail(c, TRGL_E_INVALID, "trgl_image_modulate: TRGL_MEM_DEVICE needs a context");
    if (w == 0 || h == 0) return TRGL_OK;
    if (!pixels || !mask) return fail(c, TRGL_E_INVALID, "trgl_image_modulate: null image");
    if ((int64_t)w * h * bpp > INT_MAX) return fail(c, TRGL_E_UNSUPPORTED, "trgl_image_modulate: w * h * bpp above INT_MAX");
    if (mem_kind == TRGL_MEM_HOST) { trgl_image::modulate_bytes(pixels, (size_t)w * h, bpp, mask); return TRGL_OK; }
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    launch_modulate(c->stream, pixels, (uint64_t)w * h, bpp, mask);
    HIPCHK(c, hipGetLastError());
    return TRGL_OK;
}

int trgl_framebuffer_modulate(trgl_ctx* c, const uint8_t* mask, int mask_mem_kind) {
    CHKCTX(c);
    if (!valid_mem_kind(mask_mem_kind)) return fail(c, TRGL_E_INVALID, "trgl_framebuffer_modulate: bad mask_mem_kind");
    if (!mask) return fail(c, TRGL_E_INVALID, "trgl_framebuffer_modulate: mask is null");
    const size_t npx = (size_t)c->W * c->H;
    if (npx * c->bpp > (size_t)INT_MAX) return fail(c, TRGL_E_UNSUPPORTED, "trgl_framebuffer_modulate: W * H * bpp above INT_MAX");
    int r = trgl_flush(c); if (r) return r;          // completes a begun flush, draws what is queued, runs a pending clear
    if (mask_mem_kind == TRGL_MEM_HOST) {
        if ((r = c->shadow_tmp.grow(c, npx))) return r;
        // in stream order behind an earlier modulate that may still read shadow_tmp; a pinned mask is read when the stream gets here (include/trgl.h)
        HIPCHK(c, hipMemcpyAsync(c->shadow_tmp.p, mask, npx, hipMemcpyHostToDevice, c->stream));
        mask = c->shadow_tmp.p;
    }
    launch_modulate(c->stream, c->fb.p, npx, c->bpp, mask);
    HIPCHK(c, hipGetLastError());
    return TRGL_OK;
}

int trgl_occlusion_boxes_image(trgl_ctx* c, const double* depth, int w, int h, const double viewport[16], const double view_proj[16],
                               const double* boxes, uint64_t n, uint8_t* codes, int mem_kind) {
    if (!valid_mem_kind(mem_kind)) return fail(c, TRGL_E_INVALID, "trgl_occlusion_boxes_image: bad mem_kind");
    if (w < 0 || h < 0) return fail(c, TRGL_E_INVALID, "trgl_occlusion_boxes_image: a negative dimension");
    if (!viewport || !view_proj) return fail(c, TRGL_E_INVALID, "trgl_occlusion_boxes_image: null matrix");
    if (mem_kind == TRGL_MEM_DEVICE && !c) return fail(c, TRGL_E_INVALID, "trgl_occlusion_boxes_image: TRGL_MEM_DEVICE needs a context");
    if (n == 0) return TRGL_OK;
    const bool empty = w == 0 || h == 0;
    if (!boxes || !codes || (!depth && !empty)) return fail(c, TRGL_E_INVALID, "trgl_occlusion_boxes_image: null array");
    if ((int64_t)w * h > INT_MAX || n > (uint64_t)INT_MAX) return fail(c, TRGL_E_UNSUPPORTED, "trgl_occlusion_boxes_image: w * h or n above INT_MAX");
    if (mem_kind == TRGL_MEM_HOST) { host_occlusion_boxes(depth, w, h, viewport, view_proj, boxes, n, codes); return TRGL_OK; }
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    return queue_occlusion(c, depth, w, h, viewport, view_proj, boxes, n, codes);
}

int trgl_occlusion_boxes(trgl_ctx* c, const double view_proj[16], const double* boxes, uint64_t n, int boxes_mem_kind, int slot,
                         uint8_t* codes, int codes_mem_kind) {
    CHKCTX(c);
    if (!valid_mem_kind(boxes_mem_kind) || !valid_mem_kind(codes_mem_kind)) return fail(c, TRGL_E_INVALID, "trgl_occlusion_boxes: bad mem_kind");
    if (slot != -1) { if (int r = zsnap_slot(c, slot, "trgl_occlusion_boxes")) return r; }
    if (!view_proj) return fail(c, TRGL_E_INVALID, "trgl_occlusion_boxes: view_proj is null");
    if (n && (!boxes || !codes)) return fail(c, TRGL_E_INVALID, "trgl_occlusion_boxes: null array");
    if (!owns_whole_frame(c))
        return fail(c, TRGL_E_STATE, "trgl_occlusion_boxes: the context owns a strip or interleaved bands; its depths hold only this rank's rows (gather with with_z and query on one context)");
    if (slot >= 0 && !c->zsnap[slot].p) return fail(c, TRGL_E_STATE, "trgl_occlusion_boxes: the slot holds no snapshot");
    if ((int64_t)c->W * c->H > INT_MAX || n > (uint64_t)INT_MAX) return fail(c, TRGL_E_UNSUPPORTED, "trgl_occlusion_boxes: W * H or n above INT_MAX");
    if (n == 0) return TRGL_OK;
    int r = trgl_flush(c); if (r) return r;            // completes a begun flush, draws what is queued, runs a pending clear
    const double* d_boxes = boxes;
    if (boxes_mem_kind == TRGL_MEM_HOST) {
        if ((r = c->occl_boxes.grow(c, 6 * (size_t)n))) return r;
        // in stream order behind an earlier query that may still read occl_boxes; pinned boxes are read when the stream gets here (include/trgl.h)
        HIPCHK(c, hipMemcpyAsync(c->occl_boxes.p, boxes, 6 * (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
        d_boxes = c->occl_boxes.p;
    }
    uint8_t* d_codes = codes;
    if (codes_mem_kind == TRGL_MEM_HOST) { if ((r = c->occl_codes.grow(c, (size_t)n))) return r; d_codes = c->occl_codes.p; }
    if ((r = queue_occlusion(c, slot < 0 ? c->zb.p : c->zsnap[slot].p, c->W, c->H, c->vp, view_proj, d_boxes, n, d_codes))) return r;
    if (codes_mem_kind == TRGL_MEM_HOST) {
        HIPCHK(c, hipMemcpyAsync(codes, d_codes, (size_t)n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return TRGL_OK;
}

// ---- world boxes of instances and frustum codes of boxes (include/trgl.h; host loops in trgl_host.cpp, kernels in kernels_scene.hip) ----
int trgl_instance_boxes(trgl_ctx* c, const double* local_boxes, int local_stride, const double* instances, int instance_stride,
                        uint64_t n_instances, int mem_kind, double* boxes_out) {
    if (int r = check_mem(c, "trgl_instance_boxes: ", mem_kind)) return r;
    if (local_stride != 0 && local_stride < 6) return fail(c, TRGL_E_INVALID, "trgl_instance_boxes: local_stride must be 0 (one box for all) or >= 6 doubles");
    if (instance_stride < 16) return fail(c, TRGL_E_INVALID, "trgl_instance_boxes: instance stride must be >= 16 doubles (a row-major 4x4 matrix)");
    if (n_instances > 0x7fffffffull) return fail(c, TRGL_E_UNSUPPORTED, "trgl_instance_boxes: 2^31 or more instances in one call");
    if (n_instances == 0) return TRGL_OK;
    if (!local_boxes || !instances || !boxes_out) return fail(c, TRGL_E_INVALID, "trgl_instance_boxes: null array");
    if (mem_kind == TRGL_MEM_HOST) { host_instance_boxes(local_boxes, local_stride, instances, instance_stride, n_instances, boxes_out); return TRGL_OK; }
    CHKCTX(c);
    if ((((uintptr_t)instances | (uintptr_t)boxes_out) & 7) || (local_stride && ((uintptr_t)local_boxes & 7)))
        return fail(c, TRGL_E_INVALID, "trgl_instance_boxes: device arrays must be 8-byte aligned");
    launch_instance_boxes(c->stream, local_boxes, local_stride, instances, instance_stride, (uint32_t)n_instances, boxes_out);
    HIPCHK(c, hipGetLastError());
    return TRGL_OK;
}

int trgl_frustum_boxes(trgl_ctx* c, const double planes[24], const double* boxes, uint64_t n, int mode, int mem_kind, uint8_t* codes) {
    if (int r = check_mem(c, "trgl_frustum_boxes: ", mem_kind)) return r;
    if (mode != TRGL_FRUSTUM_SET && mode != TRGL_FRUSTUM_MERGE) return fail(c, TRGL_E_INVALID, "trgl_frustum_boxes: bad mode");
    if (!planes) return fail(c, TRGL_E_INVALID, "trgl_frustum_boxes: planes is null");
    if (n > 0x7fffffffull) return fail(c, TRGL_E_UNSUPPORTED, "trgl_frustum_boxes: 2^31 or more boxes in one call");
    if (n == 0) return TRGL_OK;
    if (!boxes || !codes) return fail(c, TRGL_E_INVALID, "trgl_frustum_boxes: null array");
    const bool merge = mode == TRGL_FRUSTUM_MERGE;
    if (mem_kind == TRGL_MEM_HOST) { host_frustum_boxes(planes, boxes, n, merge, codes); return TRGL_OK; }
    CHKCTX(c);
    if ((uintptr_t)boxes & 7) return fail(c, TRGL_E_INVALID, "trgl_frustum_boxes: device boxes must be 8-byte aligned");
    launch_frustum_boxes(c->stream, planes, boxes, (uint32_t)n, merge, codes);
    HIPCHK(c, hipGetLastError());
    return TRGL_OK;
}

int trgl_selftest_division(trgl_ctx* c, uint64_t samples, uint64_t seed, uint64_t* mismatches) {
    CHKCTX(c);
    if (!mismatches) return fail(c, TRGL_E_INVALID, "null mismatches");
    int r = trgl_flush(c); if (r) return r;
    DevBuf<unsigned long long> d;
    if ((r = d.alloc(c, 1))) return r;
    HIPCHK(c, hipMemsetAsync(d.p, 0, 8, c->stream));
    unsigned long long per_thread = (samples + 1024ull * 256 - 1) / (1024ull * 256);
    launch_selftest_division(c->stream, per_thread, seed, d.p);
    unsigned long long h = 0;
    HIPCHK(c, hipMemcpyAsync(&h, d.p, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *mismatches = h;
    return TRGL_OK;
}

int trgl_selftest_sampler(trgl_ctx* c, int slot, const double* uv, uint64_t n, uint8_t* out) {
    CHKCTX(c);
    if (!uv || !out) return fail(c, TRGL_E_INVALID, "trgl_selftest_sampler: null argument");
    if (slot < 0 || slot >= TRGL_MAX_TEXTURES) return fail(c, TRGL_E_INVALID, "trgl_selftest_sampler: bad slot");
    int r = trgl_flush(c); if (r) return r;
    if (!n) return TRGL_OK;
    DevBuf<double> d_uv; DevBuf<uint8_t> d_out;
    if ((r = d_uv.alloc(c, n * 2)) || (r = d_out.alloc(c, n * 5))) return r;
    HIPCHK(c, hipMemcpyAsync(d_uv.p, uv, n * 16, hipMemcpyHostToDevice, c->stream));
    launch_selftest_sampler(c->stream, c->tex_dev.p, slot, d_uv.p, n, d_out.p);
    HIPCHK(c, hipMemcpyAsync(out, d_out.p, n * 5, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return TRGL_OK;
}

int trgl_selftest_sampler_lod(trgl_ctx* c, int slot, const double* uv, const double* lod, int mode, uint64_t n, uint8_t* out) {
    CHKCTX(c);
    if (!uv || !lod || !out) return fail(c, TRGL_E_INVALID, "trgl_selftest_sampler_lod: null argument");
    if (slot < 0 || slot >= TRGL_MAX_TEXTURES) return fail(c, TRGL_E_INVALID, "trgl_selftest_sampler_lod: bad slot");
    if (mode < 0 || mode > 2) return fail(c, TRGL_E_INVALID, "trgl_selftest_sampler_lod: mode must be 0, 1 or 2");
    int r = trgl_flush(c); if (r) return r;
    if (!n) return TRGL_OK;
    DevBuf<double> d_uv, d_lod; DevBuf<uint8_t> d_out;
    if ((r = d_uv.alloc(c, n * 2)) || (r = d_lod.alloc(c, n)) || (r = d_out.alloc(c, n * 5))) return r;
    HIPCHK(c, hipMemcpyAsync(d_uv.p, uv, n * 16, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_lod.p, lod, n * 8, hipMemcpyHostToDevice, c->stream));
    launch_selftest_sampler_lod(c->stream, c->tex_dev.p, slot, d_uv.p, d_lod.p, mode, n, d_out.p);
    HIPCHK(c, hipMemcpyAsync(out, d_out.p, n * 5, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return TRGL_OK;
}

}  // extern "C"
