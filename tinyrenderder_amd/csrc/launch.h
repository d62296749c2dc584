// launch.h — host-callable launchers of the gfx950 kernels (kernels_bin.hip, kernels_items.hip, kernels_raster.hip, kernels_post.hip,
// kernels_mesh.hip, kernels_image.hip, kernels_resolve.hip, kernels_mip.hip, kernels_shadow.hip, kernels_clip.hip,
// kernels_occlusion.hip, kernels_instance.hip, kernels_order.hip, kernels_triorder.hip, kernels_sprite.hip, kernels_skin.hip,
// kernels_edge.hip, kernels_subdiv.hip, kernels_weld.hip, kernels_lod.hip, kernels_scene.hip, kernels_selftest.hip), called by trgl_api.cpp (the flush), trgl_stage_mesh.cpp, trgl_stage_instance.cpp and
// trgl_stage_rows.cpp (the stages in front of a draw) and trgl_passes.cpp (the rest).
#pragma once
#include <hip/hip_runtime.h>
#include "trgl_device.h"
#include "clip_core.h"
#include "work_items.h"

namespace trgl {

// The direct path: every setup block writes its pairs into a segment of S slots of its own (keys / vals at
// block * S; S a multiple of 4, at most 4096), and a block of the first radix pass sorts the segments of G <= 16 consecutive setup
// blocks.  flag: device word k_chunk_spine sets to 1 when a block has more than S pairs or a group more than the radix chunk -
// the kernels of the direct path then do nothing.  nsetup: setup blocks of the flush.
struct SegLayout { uint32_t* keys; uint32_t* vals; const uint32_t* blk_sums; const uint32_t* flag; uint32_t nsetup, S, G; };
bool seg_layout_ok(const SegLayout& seg);
uint32_t seg_num_groups(const SegLayout& seg);      // blocks of the direct path's first radix pass

uint32_t setup_num_blocks(uint32_t n);      // blocks of 256 triangles of one draw (k_setup and k_expand use the same)
// (`draw` travels as a kernel argument; the kernel leaves it at draws_dev[draw_idx] for the kernels behind it)
void launch_setup(hipStream_t s, const FrameParams& fp, const DrawDesc& draw, DrawDesc* draws_dev, int draw_idx, uint32_t n,
                  TriRec* recs, TriW* recs_w, uint32_t* cnt, uint2* tilebox, DevStats* stats, uint32_t* blk_sums, uint32_t blk_base,
                  const SegLayout* seg);      // seg: the flush takes the direct path - the pairs go to seg->keys / seg->vals as well
// chunk_off[c] = pairs before setup block 16c; *total64 = all pairs of the flush
// (host_copy: pinned host memory that receives the pair count and the two counts behind it in DevStats)
// tile_bounds: tile_start followed by tile_end, `half_words` (a multiple of 4) each, 16-byte aligned; set to the empty bounds
// the last radix pass starts from (tile_start ~0, tile_end 0)
void launch_chunk_spine(hipStream_t s, const uint32_t* blk_sums, uint32_t nblk, uint32_t* chunk_off, unsigned long long* total64, unsigned long long* host_copy,
                        uint32_t* tile_bounds, size_t half_words, uint32_t seg_S, uint32_t seg_G, uint32_t seg_chunk, uint32_t* seg_flag,
                        uint32_t* seg_flag_host);
// (seg_S, seg_G, seg_chunk: the segment and group sizes the flush is checked against, and the pairs a block of the first radix pass
// holds; *seg_flag and its pinned copy *seg_flag_host receive 1 when the flush does not fit them - or seg_S is 0 - else 0)


// expand / radix read the flush's pair count from device memory and cover `cap` (the capacity of the pair buffers)
// with their grids; they do nothing when the count exceeds it (the host then grows the buffers and queues them again)
// wide: the frame has more than 65536 tiles.  Else a pair's sort word holds the 16-bit tile id in its low half and the 4x4 block
// mask in its high half, and `bmask` is only written by the last radix pass; wide frames sort 32-bit tile ids and carry the mask
// in `bmask` from k_expand on.
void launch_expand(hipStream_t s, const FrameParams& fp, uint32_t first, uint32_t n, int tiles_x, const uint32_t* cnt, const uint32_t* blk_sums,
                   const uint32_t* chunk_off, uint32_t blk_base, const uint2* tilebox, uint32_t* keys, bool wide, uint32_t* vals, uint16_t* bmask,
                   const unsigned long long* pairs_total, uint32_t cap);

uint32_t radix_num_workers(uint32_t cap);      // blocks of a radix pass over pair buffers of capacity `cap` (4 or 8 waves each)
uint32_t radix_chunk(uint32_t cap);            // pairs per block of such a pass: 4096 or 8192
// one stable pass on `bits` bits of the tile id at `shift`.  The last pass writes vals_out and msk_out (what the raster reads, no sort
// words) and the per-tile slices [tile_start, tile_end) of the sorted list; the others write keys_out, vals_out (and msk_out when wide).
struct RadixPass {
    const uint32_t* keys_in; const uint32_t* vals_in; const uint16_t* msk_in;
    uint32_t* keys_out; uint32_t* vals_out; uint16_t* msk_out;
    uint32_t* tile_start; uint32_t* tile_end;
    int shift, bits;
};
// seg: the pass reads k_setup's segments in place of keys_in / vals_in (the first pass of the direct path; not wide)
// skip: a later pass of the direct path - it does nothing when *skip (the flag of SegLayout) is set, as the first pass did
// The scatter of a pass runs as many blocks as the device holds at once (at most one per chunk, and at most max_blocks when that is
// not 0), each walking its chunks with a stride of the grid; returns that grid (0: nothing was queued).
uint32_t launch_radix_pass(hipStream_t s, const RadixPass& ps, bool wide, bool last, const unsigned long long* pairs_total, uint32_t cap,
                           uint32_t* hist, uint32_t* scan_tmp, const SegLayout* seg = nullptr, const uint32_t* skip = nullptr,
                           uint32_t max_blocks = 0);

uint32_t owned_tiles(const FrameParams& fp);       // tiles of the rows this context owns (strip or interleaved bands)
uint32_t raster_max_items(const FrameParams& fp);   // work items (workgroups of k_raster) of a flush, at most
// The bookkeeping either side of the raster kernel (kernels_items.hip; launch_raster calls both).  launch_make_items: the work items
// of the flush from the per-tile slices of the sorted pair list, over the `tiles` tiles of the context's strip; it also writes the
// record behind the flush's last one (recs[fp.n_tris]).  launch_fold_stats: the items' partials into *stats; resets the per-flush counts.
void launch_make_items(hipStream_t s, const FrameParams& fp, int tiles, const uint32_t* tile_start, const uint32_t* tile_end, uint4* items,
                       uint32_t* n_items, TriRec* recs);
void launch_fold_stats(hipStream_t s, DevStats* stats, uint32_t* n_items, const unsigned long long* item_stats);
// the shade kernel of one user kind of a flush (shade_user.h, loaded by trgl_register_shader)
struct UserShade { hipFunction_t fn; int kind; };
// item_stats: TRGL_ITEM_STATS_WORDS x uint64 per work item (work_items.h: one partial of the counters per workgroup)
// builtin_shade: the flush has PHONG / EYE draws (k_shade runs); user[0..n_user): the user kinds it has, shaded behind it
// user_raster: the raster kernel of a user kind that may discard (raster_user.h), which runs in place of k_raster when the flush
// holds only draws of that kind; null: k_raster
void launch_raster(hipStream_t s, const FrameParams& fp, int kind, bool all_well_scaled, const TriRec* recs, const TriW* recs_w,
                   const uint32_t* vals, const uint16_t* bmask,
                   const uint32_t* tile_start, const uint32_t* tile_end, const DrawDesc* draws,
                   const DevTexture* tex, DevStats* stats, uint32_t max_items, uint4* items,
                   uint32_t* n_items, unsigned long long* item_stats, bool builtin_shade, const UserShade* user, int n_user,
                   hipFunction_t user_raster,
                   hipEvent_t ev_before = nullptr, hipEvent_t ev_after = nullptr);     // optional events recorded right around the raster kernel's launch

void launch_vertex_stage(hipStream_t s, const double mv[16], const double proj[16], const double* vertices, int stride,
                         const uint32_t* indices, uint32_t nfaces, double* clip, double* vary);
void launch_zimage(hipStream_t s, const double* zb, int W, int H, unsigned long long* keys2, uint8_t* out);
void launch_ssao(hipStream_t s, const double* zb, int W, int H, const double* dir_x, const double* dir_y, int ndir, int steps,
                 double radius, double threshold, double intensity, uint8_t* out);
void launch_composite(hipStream_t s, const uint8_t* fb, int bpp, const uint8_t* ao, int W, int H, uint8_t* out);

// Model::computeAABB (model.cpp:15-40) over `n` vertex records of `stride` doubles in device memory (8-byte aligned).
// scratch: 1 + MESH_BOUNDS_MAX_BLOCKS entries; entry 0 receives the result - v[0..2] = AABB min, v[3..5] = AABB max, margin applied -
// and the others the per-block partials of the first launch, which the second (one block) folds.  n > 0.
struct BoundsPartial { double v[6]; unsigned long long i[6]; };      // running min x, y, z, max x, y, z and the vertex each came from
constexpr uint32_t MESH_BOUNDS_MAX_BLOCKS = 1024;
void launch_mesh_bounds(hipStream_t s, const double* vertices, int stride, uint64_t n, BoundsPartial* scratch);

// Model::generateNormalsIfNeeded (model.cpp:269-316) or, with `tangents`, Model::computeTangentsIfNeeded (model.cpp:318-388) over an
// indexed mesh in device memory, in place (kernels_mesh.hip).  scratch: at least mesh_attr_scratch_bytes() bytes, 256-byte aligned;
// *flag then points at the word in it that holds 1 once the arrays were rewritten and 0 when they were left alone.  nverts > 0.
hipError_t mesh_attr_scratch_bytes(uint64_t nverts, uint32_t nfaces, size_t* bytes);
hipError_t launch_mesh_attr(hipStream_t s, bool tangents, double* vertices, int stride, uint64_t nverts, const uint32_t* indices, uint32_t nfaces,
                            void* scratch, size_t scratch_bytes, const uint32_t** flag);

// TGAImage::gaussian_blur (tgaimage.cpp:271-324) on w * h * bpp bytes in device memory, in place (kernels_image.hip): the horizontal pass
// into `tmp` (as many bytes, not overlapping), the vertical pass back.  weights: the 2 * radius + 1 floats of trgl_gaussian_kernel in
// device memory.  Pointers need no alignment.  radius >= 1, w * h * bpp in 1..INT_MAX, bpp in {1, 3, 4}.
// Up to BLUR_LDS_RADIUS both passes work from LDS tiles with a clamped halo; above it the halo would outgrow the tile and each thread
// reads its clamped taps from global memory.  Both paths add the same products in the same order: the bytes do not depend on the path.
constexpr int BLUR_LDS_RADIUS = 32;                          // the switch radius
constexpr int BLUR_H_BYTES = 256, BLUR_H_ROWS = 4;           // horizontal tile: bytes of a row (one per thread) x rows
constexpr int BLUR_V_BYTES = 64, BLUR_V_ROWS = 64;           // vertical tile: bytes of a row (one per lane) x rows
void launch_image_blur(hipStream_t s, uint8_t* pixels, int w, int h, int bpp, int radius, const float* weights, uint8_t* tmp);
// TGAImage::scale (tgaimage.cpp:246-267): dst(x, y) = src(x * w / w2, y * h / h2), bpp bytes each; src and dst do not overlap.
// (w2 - 1) * w, (h2 - 1) * h and both byte counts fit an int.
constexpr int SCALE_BYTES = 256, SCALE_ROWS = 8;             // tile: bytes of an output row (one per thread) x output rows
void launch_image_scale(hipStream_t s, const uint8_t* src, int w, int h, int bpp, uint8_t* dst, int w2, int h2);
// The box filter of box_core.h (kernels_resolve.hip): dst (w / f) x (h / f) from src w x h, both bpp bytes a pixel, at any address, not
// overlapping.  f in 1..TRGL_MAX_BOX_FACTOR with w / f, h / f >= 1, w * h * bpp <= INT_MAX.  f = 1 is queued as a device-to-device copy.
hipError_t launch_box_filter(hipStream_t s, const uint8_t* src, int w, int h, int bpp, int f, uint8_t* dst);
// table[slot] = t by a one-thread kernel: an update of the context's texture table that keeps its place in the stream
hipError_t launch_set_texture(hipStream_t s, DevTexture* table, int slot, const DevTexture& t);
// Mip chains, the level-of-detail constants and the self-test of the filtered samplers (kernels_mip.hip; written down under "Mipmapped
// textures" in include/trgl.h, the arithmetic is mip_core.h's).
// launch_mip_chain: levels 1 .. L-1 of the w x h image at level0 into `chain`: with slot_layout at mip_slot_offset() from chain (the
// caller passes level0 itself: a texture slot's allocation), else at mip_packed_offset().  Any byte alignment, level0 and the written
// levels disjoint, w and h in 1..65535, w * h * bpp <= INT_MAX.  Only the levels' bytes are written.  One launch per MIP_STEP levels.
// launch_lod_stage: one thread per triangle, 0 < n < 2^31, doubles 8-byte aligned; the offsets lie inside K and do not overlap.
hipError_t launch_mip_chain(hipStream_t s, const uint8_t* level0, int w, int h, int bpp, uint8_t* chain, bool slot_layout);
hipError_t launch_lod_stage(hipStream_t s, const double viewport[16], const double* clip, double* vary, uint32_t n, int K, int uv_offset, int out_offset);
void launch_selftest_sampler_lod(hipStream_t s, const DevTexture* tex, int slot, const double* uv, const double* lod, int mode, unsigned long long n, uint8_t* out);

// The shadow post-pass (kernels_shadow.hip; the arithmetic is written down at trgl_shadow_mask_image in include/trgl.h).
// depth: w * h depths, map: map_w * map_h depths of the light's view, both 8-byte aligned (16-byte aligned arrays are read as 16-byte
// loads); mask: w * h bytes at any address.  w * h and map_w * map_h in 1..INT_MAX, radius in 0..TRGL_MAX_PCF_RADIUS.  The struct
// travels as the kernel's argument.
struct ShadowArgs {
    double M[16]; double bias, darkness;
    const double* depth; const double* map; uint8_t* mask;
    int32_t w, h, map_w, map_h, radius;
};
constexpr int SHADOW_TILE_W = 32, SHADOW_TILE_H = 32;        // pixels of a block: four waves of 32 x 8 below one another
void launch_shadow_mask(hipStream_t s, const ShadowArgs& a);
// px[c] = (unsigned char)std::min(255.0, px[c] * (mask / 255.0)) for the colour channels c < min(bpp, 3) of npixels pixels, in place
// (main.cpp:775-781); pixels and mask at any address, not overlapping.  npixels * bpp in 1..INT_MAX, bpp in {1, 3, 4}.
void launch_modulate(hipStream_t s, uint8_t* pixels, uint64_t npixels, int bpp, const uint8_t* mask);

// The clip stage (kernels_clip.hip; the operation is written down at trgl_clip_stage in include/trgl.h, its arithmetic is clip_core.h's).
// clip / vary / colors: n triangles (vary unused when K = 0, colors may be null - colors_out is then not written); the outputs have room
// for 2 n triangles; doubles 8-byte aligned, colours 4.  n < 2^31, K <= TRGL_MAX_USER_VARY.  The struct travels as the kernels' argument.
struct ClipArgs {
    double plane[4];
    const double* clip; const double* vary; const uint32_t* colors;
    double* clip_out; double* vary_out; uint32_t* colors_out;
    uint64_t n; int32_t K;
    ClipTable tab;
};
constexpr int CLIP_BLOCK_TRIS = 256;         // triangles of a block of k_clip_count / k_clip_scatter, one per lane
constexpr int CLIP_SCAN_CHUNK = 256;         // block sums a block of the scan's lower level takes; more of them need its upper level
uint32_t clip_num_blocks(uint64_t n);
size_t clip_scratch_words(uint64_t n);       // the block sums and, behind them, the sums of the scan's chunks
// scratch: clip_scratch_words(n) words; *total receives the number of output triangles.  Four launches, in order on `s`.
void launch_clip_stage(hipStream_t s, const ClipArgs& a, uint32_t* scratch, unsigned long long* total);

// Occlusion culling of boxes (kernels_occlusion.hip; the test is written down at trgl_occlusion_boxes_image in include/trgl.h, steps 1-6
// are occlusion_core.h's).  levels: occl_level_doubles(w, h) doubles of scratch - level 1, ceil(w / 8) x ceil(h / 8) maxima of the 8 x 8
// pixel blocks, then level 2, ceil(w / 64) x ceil(h / 64) maxima of the 64 x 64 blocks; a NaN depth counts as -inf, an edge block covers
// the pixels that exist.  depth and boxes 8-byte aligned, codes at any address; w * h and n in 0..INT_MAX.
constexpr int OCCL_L1 = 8, OCCL_L2 = 64;     // pixels along a block's side at the two levels; a workgroup of the build owns one level-2 block
constexpr int OCCL_QUERY_BOXES = 4;          // boxes of a workgroup of the query, one wavefront each
size_t occl_level_doubles(int w, int h);
// one pass over the w * h depths (w * h > 0) that leaves both levels
void launch_occl_build(hipStream_t s, const double* depth, int w, int h, double* levels);
// The struct travels as the query kernel's argument.  With w * h == 0 neither depth nor levels is read.
struct OcclArgs {
    double M[16]; double V[8];               // view_proj, rows 0 and 1 of the viewport matrix
    const double* depth; const double* levels; const double* boxes; uint8_t* codes;
    uint64_t n; int32_t w, h;
};
void launch_occl_query(hipStream_t s, const OcclArgs& a);

// The stages in front of an instanced draw (kernels_instance.hip; the operation is written down at trgl_draw_instanced in include/trgl.h).
// Compaction of the visibility bytes: INST_BLOCK instances per block, one per lane; the scan over the block counts has two levels,
// INST_SCAN_CHUNK block counts per block of the lower one.  The instance list may have any length below 2^31.
constexpr int INST_BLOCK = 256;
constexpr int INST_SCAN_CHUNK = 256;
constexpr int INST_VS_FACES = 64;            // output faces of a block of the instanced vertex stage (three threads each)
uint32_t inst_num_blocks(uint64_t n);
size_t inst_scratch_words(uint64_t n);       // 2 words for the 8-byte count, the block counts, the chunk sums
// The scan of that compaction alone, for any kernel pair that counts per block of INST_BLOCK lanes (kernels_edge.hip): blk[0 .. nblk)
// become their exclusive prefix sums within chunks of INST_SCAN_CHUNK, chunk[c] the sum of the chunks before c, *total the sum of all.
// An entry's position is chunk[b / INST_SCAN_CHUNK] + blk[b] + its rank within block b.  Two launches; nblk > 0, the sum below 2^32.
void launch_block_count_scan(hipStream_t s, uint32_t* blk, uint32_t nblk, uint32_t* chunk, unsigned long long* total);
// list[j] = i_j, the instances with (visible[i] & 1) in ascending order, and *total = n_vis; with mv_out, slot j also receives
// MV = model_view * M_{i_j} (geometry.h:196-205; M: the first 16 doubles of the instance's record).  scratch: inst_scratch_words(n)
// words, *total its first two.  Four launches, in order on `s`.  0 < n < 2^31.
void launch_inst_compact(hipStream_t s, const uint8_t* visible, uint32_t n, uint32_t* scratch, uint32_t* list,
                         const double model_view[16], const double* instances, int inst_stride, double* mv_out);
// The same over the positions of an order list (trgl_draw_instanced_ordered): position p names instance i = order[p] and is drawn when
// i < n and (visible null or visible[i] & 1); list[j] = i_j in ascending p, *total = n_vis, mv_out as above.  An entry >= n is skipped
// and never used as an index.  scratch: inst_scratch_words(n_order) words; list (and mv_out) with room for n_order entries.
// 0 < n_order < 2^31, 0 < n < 2^31.
void launch_inst_compact_ordered(hipStream_t s, const uint32_t* order, uint32_t n_order, const uint8_t* visible, uint32_t n, uint32_t* scratch,
                                 uint32_t* list, const double model_view[16], const double* instances, int inst_stride, double* mv_out);
// mv_out[j] = model_view * M_{list[j]} for j < n_vis (list null: M_j) - for a list that was not made by launch_inst_compact
void launch_inst_mv(hipStream_t s, const uint32_t* list, uint32_t n_vis, const double model_view[16], const double* instances,
                    int inst_stride, double* mv_out);
// k_vertex_stage over the flattened faces ip.total = n_vis * nfaces, the model-view matrix of output face g being ip.mv + 16 * (g / nfaces)
void launch_instance_vertex_stage(hipStream_t s, const InstanceParams& ip, const double proj[16], const double* vertices, int stride,
                                  const uint32_t* indices, uint32_t nfaces, double* clip, double* vary);

// Depths and a depth order for the instances (kernels_order.hip; both are written down at trgl_instance_depths / trgl_depth_order in
// include/trgl.h).  launch_instance_depths: one thread per instance, 0 < n < 2^31.  launch_depth_order: a key kernel (key or ~key as
// uint64, and 0 .. n-1), then hipcub's stable radix sort of the pairs over all 64 bits; scratch: depth_order_scratch_bytes(n) bytes,
// 256-byte aligned.  0 < n < 2^31.
void launch_instance_depths(hipStream_t s, const double model_view[16], const double point[3], const double* instances, int inst_stride,
                            uint32_t n, double* depths);
hipError_t depth_order_scratch_bytes(uint32_t n, size_t* bytes);
hipError_t launch_depth_order(hipStream_t s, const double* depths, uint32_t n, bool front_to_back, void* scratch, size_t scratch_bytes,
                              uint32_t* order);

// A depth per group of triangles and the gather of rows under an order list (kernels_triorder.hip; both are written down at
// trgl_triangle_depths / trgl_order_stage in include/trgl.h, the depth expressions are triorder_core.h's).
// launch_triangle_depths: one thread per group; clip holds G * g triangles, depths G doubles, both 8-byte aligned; mode one of
// TRGL_TRI_DEPTH_*; 0 < G, g >= 1, G * g < 2^31.
// launch_gather_rows: for p < n_order, the g rows of out group p are those of in group order[p], or zeros when order[p] >= G (the entry
// is then no index).  Rows of row_bytes bytes (a multiple of 4); in and out aligned to 4 bytes at least, and moved 16 or 8 bytes at a
// time where they and row_bytes allow it.  0 < n_order, n_order * g < 2^31, G * g < 2^31.
void launch_triangle_depths(hipStream_t s, const double* clip, uint32_t G, uint32_t g, int mode, double* depths);
void launch_gather_rows(hipStream_t s, const void* in, void* out, uint32_t row_bytes, const uint32_t* order, uint32_t n_order, uint32_t G, uint32_t g);

// Point sprites and wide lines (kernels_sprite.hip; both are written down at trgl_sprite_stage / trgl_line_stage in include/trgl.h, the
// arithmetic is sprite_core.h's).  One launch per call: a block computes SPRITE_BLOCK quads, one per lane, and its lanes then store the
// block's rows as contiguous memory.  points 8-byte aligned, colours and indices 4; clip_out / vary_out 8-byte aligned (moved 16 bytes
// at a time where 16-byte aligned); vary_out null: no varyings; colors null: colors_out is not written.  0 < n, 2 n < 2^31.  The
// structs travel as the kernels' arguments.
constexpr int SPRITE_BLOCK = 256;
struct SpriteArgs {
    trgl_sprite_params P;
    const double* points; const uint32_t* colors;
    double* clip_out; double* vary_out; uint32_t* colors_out;
    uint64_t n; int32_t stride;
};
struct LineArgs {
    trgl_line_params P;
    const double* points; const uint32_t* indices; const uint32_t* colors;      // indices null: segment j = points 2 j, 2 j + 1
    double* clip_out; double* vary_out; uint32_t* colors_out;
    uint64_t n_points, n; int32_t stride;
};
void launch_sprite_stage(hipStream_t s, const SpriteArgs& a);
void launch_line_stage(hipStream_t s, const LineArgs& a);

// Skeletal animation (kernels_skin.hip; both are written down at trgl_skin_stage / trgl_pose_palette in include/trgl.h, the
// arithmetic is skin_core.h's).  launch_skin_stage: one launch per call; a block of SKIN_BLOCK lanes owns `vb` consecutive vertices -
// vb * stride <= SKIN_TILE_DOUBLES, the LDS tile its records pass through on the way in and out - and SKIN_POSE_GROUP consecutive
// poses, n_vblocks = ceil(n / vb) blocks per group of poses.  A palette of up to SKIN_LDS_JOINTS joints is staged in LDS, three rows
// per joint; a larger one is read through the cache.  vertices, weights, palette, out 8-byte aligned, joints 2.  n, n_poses > 0; the
// number of blocks below 2^31.  LDS is sized per launch: skin_tile_doubles(vb, stride) doubles of tile and 12 per staged joint.
// launch_pose_palette: POSE_GROUP poses per block of POSE_BLOCK lanes (one wave), 16 lanes per pose; the matrices of up to
// POSE_LDS_JOINTS joints stay in LDS from load to store, those of more go through the palette in memory.  The structs travel as the
// kernels' arguments.
constexpr int SKIN_BLOCK = 256;
constexpr int SKIN_TILE_DOUBLES = SKIN_BLOCK * 20;      // 40 KiB: 256 records of up to 20 doubles, fewer of wider ones
constexpr int SKIN_MAX_DEVICE_STRIDE = SKIN_TILE_DOUBLES;
__host__ __device__ inline uint32_t skin_tile_doubles(uint32_t vb, uint32_t stride) { return (vb * stride + 1u) & ~1u; }      // (16-byte units)
constexpr int SKIN_LDS_JOINTS = 128;                    // 12 KiB of palette rows
constexpr int SKIN_POSE_GROUP = 8;
struct SkinArgs {
    const double* vertices; const uint16_t* joints; const double* weights; const double* palette; double* out;
    uint64_t n, n_poses, palette_stride, n_vblocks;
    uint32_t stride, n_joints, flags, vb;
};
void launch_skin_stage(hipStream_t s, const SkinArgs& a, int n_influences);
constexpr int POSE_GROUP = 4, POSE_BLOCK = 16 * POSE_GROUP;
constexpr int POSE_LDS_JOINTS = 96;                     // 4 poses x 96 joints x 128 bytes = 48 KiB
struct PoseArgs {
    const int32_t* parents; const double* inverse_bind; const double* local; double* palette;      // inverse_bind null: palette = world
    uint64_t local_stride, n_poses, palette_stride;
    uint32_t n_joints;
};
void launch_pose_palette(hipStream_t s, const PoseArgs& a);

// Mesh edges (kernels_edge.hip; written down under "mesh edges" in include/trgl.h, the key and the arithmetic are edge_core.h's).
// Every kernel runs EDGE_BLOCK lanes a block, one half-edge or one record per lane; the counts of the blocks go through
// launch_block_count_scan, so its two levels (INST_SCAN_CHUNK block counts per block of the lower one) are this stage's too.
// launch_mesh_edges: nh = 3 * n_faces half-edges, 0 < nh < 2^31; indices and edges_out (room for nh records) 4-byte aligned, written 16
// bytes per record where 16-byte aligned.  scratch: mesh_edges_scratch_bytes() bytes, 256-byte aligned; *total then points at the 8-byte
// count of edges in it.  A key kernel, the sort, a count, the scan's two launches and a write kernel, in order on `s`.
// launch_edge_select: 0 < n_edges < 2^31; vertices 8-byte aligned, indices / edges / segments / colors 4, codes any; a null output is not
// written.  P.compact: scratch of edge_select_scratch_bytes(n_edges) bytes, *total the 8-byte count of selected records in it (four
// launches); else scratch is unused and *total null (one launch).  The struct travels as the kernels' argument.
constexpr int EDGE_BLOCK = 256;
hipError_t mesh_edges_scratch_bytes(uint32_t nh, uint64_t n_vertices, size_t* bytes);
hipError_t launch_mesh_edges(hipStream_t s, const uint32_t* indices, uint32_t nh, uint64_t n_vertices, void* scratch, size_t scratch_bytes,
                             uint32_t* edges_out, const unsigned long long** total);
// the sort of launch_mesh_edges alone, over the keys that call left in the same scratch (a measurement's floor: profiles/outline_probe.py)
hipError_t launch_mesh_edges_sort(hipStream_t s, uint32_t nh, uint64_t n_vertices, void* scratch, size_t scratch_bytes);
struct EdgeSelectArgs {
    trgl_edge_params P;
    const double* vertices; const uint32_t* indices; const uint32_t* edges;
    uint8_t* codes; uint32_t* segments; uint32_t* colors;
    uint64_t n_vertices; uint32_t n_faces, n_edges; int32_t stride;
};
size_t edge_select_scratch_bytes(uint32_t n_edges);
hipError_t launch_edge_select(hipStream_t s, const EdgeSelectArgs& a, void* scratch, const unsigned long long** total);

// Mesh subdivision (kernels_subdiv.hip; written down under "mesh subdivision" in include/trgl.h, the rules are subdiv_core.h's).
// launch_subdiv_topology: 0 < n_faces, 3 * n_faces < 2^31, 0 < n_vertices, n_edges <= 3 * n_faces (0: no record), n_vertices + n_edges
// < 2^32; every array 4-byte aligned, written 16 bytes at a time where 16-byte aligned.  scratch: subdiv_topology_scratch_bytes() bytes,
// 256-byte aligned.  A stencil kernel, the sort, a ring, an even-record and an index kernel, in order on `s`.
// launch_subdiv_vertices: one launch of SUBDIV_BLOCK lanes a block, SUBDIV_ITEMS doubles of the output per lane; vertices and out 8-byte
// aligned, stencils 4; (n_vertices + n_edges) * stride below 2^31 * SUBDIV_BLOCK * SUBDIV_ITEMS.  smooth: 0 for the linear mode.  The
// struct travels as the kernel's argument (step_q and step_r are filled in by the launch).
constexpr int SUBDIV_BLOCK = 256;
constexpr int SUBDIV_ITEMS = 4;
hipError_t subdiv_topology_scratch_bytes(uint64_t n_edges, uint64_t n_vertices, size_t* bytes);
hipError_t launch_subdiv_topology(hipStream_t s, const uint32_t* indices, uint64_t n_faces, uint64_t n_vertices, const uint32_t* edges,
                                  uint64_t n_edges, void* scratch, size_t scratch_bytes, uint32_t* indices_out, uint32_t* stencils_out);
// the sort of launch_subdiv_topology alone, over the entries that call left in the same scratch (a measurement's floor: profiles/subdiv_probe.py)
hipError_t launch_subdiv_topology_sort(hipStream_t s, uint64_t n_edges, uint64_t n_vertices, void* scratch, size_t scratch_bytes);
struct SubdivVertexArgs {
    const double* vertices; const uint32_t* stencils; double* out;
    uint64_t n_vertices, n_edges;
    uint32_t stride, smooth, step_q, step_r;
};
hipError_t launch_subdiv_vertices(hipStream_t s, SubdivVertexArgs a);

// Mesh welding (kernels_weld.hip; written down under "mesh welding" in include/trgl.h, the key, the comparison and the hash are
// weld_core.h's).  Every kernel runs WELD_BLOCK lanes a block, one vertex, sorted entry or index per lane; the counts of the blocks go
// through launch_block_count_scan.  0 < n < 2^31 vertices, n_idx < 2^31 indices (0: none); vertices and vertices_out 8-byte aligned, the
// uint32 arrays 4; a null output is not written (indices_out needs indices).  hash_bits 0 .. 64: the low bits of the hash the sort runs
// over (0: no sort, one run).  scratch: mesh_weld_scratch_bytes() bytes, 256-byte aligned; *total then points at the 8-byte count of
// distinct vertices in it.  The struct travels as the kernels' argument.
constexpr int WELD_BLOCK = 256;
// the pieces of a scratch buffer start on 256-byte boundaries (kernels_weld.hip, kernels_lod.hip, trgl_stage_mesh.cpp)
inline size_t scratch_align256(size_t n) { return (n + 255) & ~size_t(255); }
struct WeldArgs {
    trgl_weld_params P;
    const double* vertices; const uint32_t* indices;
    uint32_t* remap_out; uint32_t* firsts_out; double* vertices_out; uint32_t* indices_out;
    uint32_t n, n_idx; int32_t hash_bits;
};
hipError_t mesh_weld_scratch_bytes(uint32_t n, int hash_bits, size_t* bytes);
hipError_t launch_mesh_weld(hipStream_t s, const WeldArgs& a, void* scratch, size_t scratch_bytes, const unsigned long long** total);
// the sort of launch_mesh_weld alone, over the pairs that call left in the same scratch (a measurement's floor: profiles/weld_probe.py)
hipError_t launch_mesh_weld_sort(hipStream_t s, uint32_t n, int hash_bits, void* scratch, size_t scratch_bytes);

// What launch_mesh_weld leaves in its scratch for a kernel queued behind it (kernels_lod.hip, the mean of a cell): the (hash, vertex)
// pairs as sorted - a run of equal hashes ascends in vertex number; hash_bits == 0: one run -, rep[v] the representative of vertex v and
// newnum[v] the new number of a representative v (other entries are not written).  n and hash_bits as passed to launch_mesh_weld.
struct WeldPairs { const unsigned long long* hashes; const uint32_t* numbers; const uint32_t* rep; const uint32_t* newnum; };
WeldPairs mesh_weld_pairs(const void* scratch, uint32_t n, int hash_bits);

// Mesh levels of detail (kernels_lod.hip; written down under "mesh levels of detail" in include/trgl.h, the class of a face, the
// canonical triple, its hash and the mean's arithmetic are lod_core.h's).  Every kernel runs LOD_BLOCK lanes a block, one face, sorted
// entry or vertex per lane; the counts of the blocks go through launch_block_count_scan.
// launch_mesh_clean: n_faces < 2^31 / 3, 0 < n_vertices < 2^31 (n_faces == 0 needs CLEAN_VERTICES); indices 4-byte aligned, vertices
// and vertices_out 8; a null output is not written; the vertex outputs need TRGL_CLEAN_VERTICES in P.flags.  hash_bits 0 .. 64: the low
// bits of the face hash the sort runs over (0: no sort, one run).  scratch: mesh_clean_scratch_bytes() bytes, 256-byte aligned; *totals
// then points at the two 8-byte counts { kept faces, kept vertices } in it (the second is only written with TRGL_CLEAN_VERTICES).
constexpr int LOD_BLOCK = 256;
struct CleanArgs {
    trgl_clean_params P;
    const uint32_t* indices; const double* vertices;
    uint32_t* indices_out; uint32_t* face_firsts_out; uint32_t* vremap_out; uint32_t* vfirsts_out; double* vertices_out;
    uint32_t n_faces, n_vertices; int32_t hash_bits;
};
hipError_t mesh_clean_scratch_bytes(uint32_t n_faces, uint32_t n_vertices, int hash_bits, size_t* bytes);
hipError_t launch_mesh_clean(hipStream_t s, const CleanArgs& a, void* scratch, size_t scratch_bytes, const unsigned long long** totals);
// the sort of launch_mesh_clean alone, over the pairs that call left in the same scratch (a measurement's floor: profiles/lod_probe.py)
hipError_t launch_mesh_clean_sort(hipStream_t s, uint32_t n_faces, uint32_t n_vertices, int hash_bits, void* scratch, size_t scratch_bytes);
// The pieces of trgl_mesh_simplify between its weld and its clean, and behind the clean.
// launch_lod_mean: queued behind launch_mesh_weld(n vertices, hash_bits) whose scratch is weld_scratch and whose vertices_out is
// `records`: the first mean_count doubles of every kept record become the mean of the cluster's members that some word of
// indices[0 .. n_idx) names.  referenced: n words of scratch.
hipError_t launch_lod_mean(hipStream_t s, const double* vertices, int stride, int mean_count, uint32_t n, const uint32_t* indices, uint32_t n_idx,
                           const void* weld_scratch, int hash_bits, uint32_t* referenced, double* records);
// launch_lod_compose: remap_out[v] = vremap[weld_remap[v]] and firsts_out[j] = weld_firsts[vfirsts[j]], NONE where vfirsts[j] is (either
// output may be null)
hipError_t launch_lod_compose(hipStream_t s, uint32_t n, const uint32_t* weld_remap, const uint32_t* vremap, uint32_t* remap_out,
                              const uint32_t* weld_firsts, const uint32_t* vfirsts, uint32_t* firsts_out);

// World boxes of instances and frustum codes of boxes (kernels_scene.hip; both are written down at trgl_instance_boxes /
// trgl_frustum_boxes in include/trgl.h, the arithmetic is scene_core.h's).  One thread per instance or box, 0 < n < 2^31; doubles 8-byte
// aligned, codes at any address.  local_stride == 0: local_boxes is HOST memory, 6 doubles that travel as the kernel's argument; else
// device memory, instance i's box at local_boxes + i * local_stride.  planes: host memory, the kernel's argument.  merge: only the
// bytes of culled boxes are written (TRGL_FRUSTUM_MERGE); else every byte (TRGL_FRUSTUM_SET).
void launch_instance_boxes(hipStream_t s, const double* local_boxes, int local_stride, const double* instances, int inst_stride,
                           uint32_t n, double* boxes_out);
void launch_frustum_boxes(hipStream_t s, const double planes[24], const double* boxes, uint32_t n, bool merge, uint8_t* codes);

void launch_selftest_sampler(hipStream_t s, const DevTexture* tex, int slot, const double* uv, unsigned long long n, uint8_t* out);
void launch_selftest_division(hipStream_t s, unsigned long long n_per_thread, unsigned long long seed,
                              unsigned long long* mismatches);

}  // namespace trgl
