// trgl_rccl.cpp — RCCL, loaded on demand (the library has no link-time dependency on it): the communicator calls of include/trgl.h and
// trgl_gather, which completes the rows of every rank's framebuffer (and z-buffer) on each rank.
#include <dlfcn.h>

#include <cstring>

#include "trgl_ctx.h"

namespace {
struct Rccl {
    struct Id { char b[128]; };          // ncclUniqueId, passed by value (rccl.h)
    void* lib = nullptr;
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, Id, int) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    bool ok = false;
};
Rccl& rccl() {
    static Rccl r;
    if (!r.lib) {
        r.lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!r.lib) r.lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (r.lib) {
            r.GetUniqueId = reinterpret_cast<decltype(r.GetUniqueId)>(dlsym(r.lib, "ncclGetUniqueId"));
            r.CommInitRank = reinterpret_cast<decltype(r.CommInitRank)>(dlsym(r.lib, "ncclCommInitRank"));
            r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(dlsym(r.lib, "ncclCommDestroy"));
            r.AllGather = reinterpret_cast<decltype(r.AllGather)>(dlsym(r.lib, "ncclAllGather"));
            r.GroupStart = reinterpret_cast<decltype(r.GroupStart)>(dlsym(r.lib, "ncclGroupStart"));
            r.GroupEnd = reinterpret_cast<decltype(r.GroupEnd)>(dlsym(r.lib, "ncclGroupEnd"));
            r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(dlsym(r.lib, "ncclGetErrorString"));
            r.ok = r.GetUniqueId && r.CommInitRank && r.CommDestroy && r.AllGather && r.GroupStart && r.GroupEnd;
        }
    }
    return r;
}
std::string rccl_err(const char* what, int code) {
    Rccl& r = rccl();
    return std::string(what) + ": " + (r.GetErrorString ? r.GetErrorString(code) : "RCCL error") + " (" + std::to_string(code) + ")";
}
constexpr int NCCL_UINT8 = 1;       // ncclUint8 (rccl.h, ncclDataType_t)
}  // namespace

extern "C" {

int trgl_rccl_unique_id(uint8_t id[TRGL_RCCL_ID_BYTES]) {
    if (!id) return TRGL_E_INVALID;
    Rccl& r = rccl();
    if (!r.ok) return fail(nullptr, TRGL_E_UNSUPPORTED, "librccl.so.1 could not be loaded");
    const int rc = r.GetUniqueId(id);
    return rc ? fail(nullptr, TRGL_E_HIP, rccl_err("ncclGetUniqueId", rc)) : TRGL_OK;
}
int trgl_rccl_comm_create(const uint8_t id[TRGL_RCCL_ID_BYTES], int rank, int world, int device, void** comm) {
    if (!id || !comm || world < 1 || rank < 0 || rank >= world) return TRGL_E_INVALID;
    Rccl& r = rccl();
    if (!r.ok) return fail(nullptr, TRGL_E_UNSUPPORTED, "librccl.so.1 could not be loaded");
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, TRGL_E_HIP, "hipSetDevice failed");
    Rccl::Id uid; std::memcpy(uid.b, id, 128);
    const int rc = r.CommInitRank(comm, world, uid, rank);
    return rc ? fail(nullptr, TRGL_E_HIP, rccl_err("ncclCommInitRank", rc)) : TRGL_OK;
}
int trgl_rccl_comm_destroy(void* comm) {
    if (!comm) return TRGL_E_INVALID;
    Rccl& r = rccl();
    if (!r.ok) return TRGL_E_UNSUPPORTED;
    return r.CommDestroy(comm) ? TRGL_E_HIP : TRGL_OK;
}

int trgl_gather(trgl_ctx* c, void* comm, int rank, int world, int with_z) {
    CHKCTX(c);
    if (!comm || world < 1 || rank < 0 || rank >= world) return fail(c, TRGL_E_INVALID, "trgl_gather: bad communicator / rank / world");
    Rccl& r = rccl();
    if (!r.ok) return fail(c, TRGL_E_UNSUPPORTED, "trgl_gather: librccl.so.1 could not be loaded");
    int fr = trgl_flush(c); if (fr) return fr;               // the rows this context owns are complete behind this point of the stream
    // Inside each period of world * band rows the bands lie in rank order.  One strip per rank (equal, contiguous chunks of the row-major
    // buffers) is the case of one period: band = H / world.
    int band;
    if (c->il_tiles == 0) {
        if (c->H % world) return fail(c, TRGL_E_INVALID, "trgl_gather: the height is not divisible by the number of ranks (equal strips are required)");
        band = c->H / world;
        if (c->strip_y0 != rank * band || c->strip_y1 != (rank + 1) * band)
            return fail(c, TRGL_E_STATE, "trgl_gather: this context's strip is not rows [rank * H / world, (rank + 1) * H / world)");
    } else {
        if (c->il_world != world || c->il_rank != rank) return fail(c, TRGL_E_STATE, "trgl_gather: rank / world differ from trgl_set_interleave");
        band = c->il_tiles * TRGL_TILE;
        if (c->H % (band * world)) return fail(c, TRGL_E_INVALID, "trgl_gather: the height is not a multiple of world * band_rows");
    }
    const int period = band * world;
    const size_t row_fb = (size_t)c->W * c->bpp, row_z = (size_t)c->W * sizeof(double);
    uint8_t* const zb = reinterpret_cast<uint8_t*>(c->zb.p);
    int rc = r.GroupStart();
    if (rc) return fail(c, TRGL_E_HIP, rccl_err("ncclGroupStart", rc));
    for (int p0 = 0; p0 < c->H && !rc; p0 += period) {
        const int y0 = p0 + rank * band;
        rc = r.AllGather(c->fb.p + (size_t)y0 * row_fb, c->fb.p + (size_t)p0 * row_fb, (size_t)band * row_fb, NCCL_UINT8, comm, c->stream);
        if (!rc && with_z) rc = r.AllGather(zb + (size_t)y0 * row_z, zb + (size_t)p0 * row_z, (size_t)band * row_z, NCCL_UINT8, comm, c->stream);
    }
    const int rc2 = r.GroupEnd();
    if (!rc) rc = rc2;
    return rc ? fail(c, TRGL_E_HIP, rccl_err("ncclAllGather", rc)) : TRGL_OK;
}

}  // extern "C"
