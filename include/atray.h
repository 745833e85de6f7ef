/*
 * atray.h -- C-ABI of the MI355X (gfx950) intersection engine for ATRay's per-pixel render
 * loop. Drop-in boundary under the reference's render API (Source/engine/renderer/renderer.h):
 *
 *   prep_scene(Scene&, uint32&)                        renderer.h:35 / renderer.cpp:264-291
 *       -> atr_mesh_load_obj + atr_octree_build (host prerequisites, or the caller's own
 *          build_KD_tree output flattened by atr_octree_from_nodes) + atr_scene_upload
 *   start_render_from_camera(RenderInfo&, ThreadPool&) renderer.h:32 / renderer.cpp:403-455
 *       -> atr_make_tiles + atr_render_start (async on a HIP stream)
 *   wait_for_render_from_camera_to_finish(...)         renderer.h:33 / renderer.cpp:457-471
 *       -> atr_render_wait (TRUE/1 = still running, FALSE/0 = done, <0 = error)
 *
 * Plain C types and pointers only; every entry point returns an int status (0 = ok,
 * negative = ATR_E_* or -(1000 + hipError_t)). No exceptions cross the ABI. One context per
 * GPU; a context is used by one host thread at a time.
 */
#ifndef ATRAY_H
#define ATRAY_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI 2 (round 6): atr_tuning gained reserved[4] (zero; room for later knobs without a size
   change); ABI 1's last two words became path_sort_bits and path_split in round 5.
   atr_trace_rays and atr_ray_hits were added since without a version change: no existing struct
   or entry point changed. atr_occluded_rays likewise; atr_gather_occlusion, atr_gather_out and
   atr_gather_directions likewise; atr_radiance_rays and atr_radiance_out likewise;
   atr_gather_radiance and atr_gather_radiance_out likewise; atr_mesh_texels, atr_texels_out and
   atr_texels_to_image likewise; atr_denoise, atr_denoise_params, atr_denoise_guides and
   atr_default_denoise_params likewise; atr_accumulate, atr_accumulate_check, atr_history,
   atr_accumulate_params and atr_default_accumulate_params likewise; atr_denoise_variance,
   atr_denoise_variance_check, atr_denoise_variance_params and atr_default_denoise_variance_params
   likewise; atr_camera_guides, atr_guides_out, atr_camera_rays and atr_camera_rays_host likewise;
   atr_probe_sh, atr_probe_sh_out, atr_probe_directions and atr_sh_basis likewise. */
#define ATR_ABI_VERSION 2

enum {
    ATR_OK = 0,
    ATR_E_INVALID = -1,     /* bad argument */
    ATR_E_IO = -2,          /* file could not be read */
    ATR_E_NOMEM = -3,       /* memory could not be had, or a tree build passed its reference budget
                               (atr_octree_build). No exception leaves an entry point that returns a
                               status or a count: std::bad_alloc comes back as this, anything else as
                               ATR_E_INVALID -- from the count-returning ones (atr_make_tiles,
                               atr_make_shard_tiles, atr_balance_shard_tiles, atr_render_packed_size,
                               atr_packed_pixel_map, atr_camera_pads_row, atr_camera_leaf_boxes_row), whose results are never
                               negative, as that negative value */
    ATR_E_NOSCENE = -4,     /* render before atr_scene_upload */
    ATR_E_TREE_DEPTH = -5,  /* octree deeper than the traversal's mask stack (16 levels) */
    ATR_E_TREE_LAYOUT = -6, /* children boxes are not the parent's split-point octants
                               (build_oct_kd_tree makes them so, kd_tree.cpp:116-148) */
    ATR_E_HIP = -1000       /* -(1000 + hipError_t) */
};

typedef struct { float x, y, z; } atr_vec3;

/* Material (material.h:4-8). materials[0] is the sky (renderer.cpp:154). */
typedef struct { atr_vec3 emission, reflection; float scatter; } atr_material;

/* Host mesh = ModelData (model.h:15-23) with 0-based indices (OBJ_loader.cpp:229-267). */
typedef struct atr_mesh atr_mesh;
/* Host octree = KD_Tree (kd_tree.h:38-47) flattened in reference node order. */
typedef struct atr_octree atr_octree;

/* load_model_data (OBJ_loader.h:6): custom parse_f64 (parser.h:113-191), faces keep the first
   triangle of each polygon, negative indices relative to the end. atr_mesh_load_obj parses on
   the host's threads (threads = min(hardware threads, 16)); atr_mesh_parse_obj on one. */
int atr_mesh_load_obj(const char* path, atr_mesh** out);
int atr_mesh_parse_obj(const char* text, size_t len, atr_mesh** out);
/* The reference's parallel load (OBJ_loader.cpp:298-340): the text split into `threads`
   newline-aligned chunks parsed concurrently and joined in order (join_chunks, :190-227), then
   the relative indices resolved (prep_model_data, :229-267). threads = 0 picks the default.
   The mesh is bit-identical for every thread count. */
int atr_mesh_load_obj_threaded(const char* path, int32_t threads, atr_mesh** out);
int atr_mesh_parse_obj_threaded(const char* text, size_t len, int32_t threads, atr_mesh** out);
/* ModelData from caller arrays (copied). normals may be NULL (flat shading). */
int atr_mesh_from_arrays(const float* vertices, uint32_t nvertices, const int32_t* face_vertices,
                         uint32_t nfaces, const float* normals, uint32_t nnormals,
                         const int32_t* face_normals, atr_mesh** out);
void atr_mesh_free(atr_mesh* m);
int atr_mesh_info(const atr_mesh* m, uint32_t* nvertices, uint32_t* nnormals, uint32_t* nfaces);
/* Copy ModelData out (any pointer may be NULL): 3 floats per vertex / normal / texcoord, 3 ints
   per face for each index array (0-based, -1 = absent). ntexcoords (may be NULL) receives the
   texcoord count. */
int atr_mesh_export(const atr_mesh* m, float* vertices, float* normals, float* texcoords, uint32_t* ntexcoords,
                    int32_t* face_v, int32_t* face_t, int32_t* face_n);
/* get_AABB (model.h:41-61): min xyz, max xyz padded by 1e-4. */
int atr_mesh_aabb(const atr_mesh* m, float aabb_out[6]);
/* translate_to (model.h:136-152): moves the vertices and the caller's AABB (in/out). */
int atr_mesh_translate_to(atr_mesh* m, float aabb_inout[6], atr_vec3 new_center);

/* build_KD_tree (kd_tree.cpp:20-64) -> build_oct_kd_tree (:67-288), SAH-named split, leaf
   size max_faces (app.cpp:77 uses 300). Result is bit-identical to the reference's tree.
   The reference hands a triangle to every child box that holds one of its vertices (closed boxes), so
   coincident triangles whose split point lies on a shared child-box face are copied into several
   children at every level down to depth 64, and its build of such a mesh never ends (two equal
   triangles in an axis-aligned plane at max_faces 1; a mesh moved 2^22 from the origin, whose vertices
   collapse onto the float lattice). The build therefore bounds the tree's live primitive references
   -- those of every node that is a leaf so far or still to be split -- by
   min(2^31 - 1, 256 * nfaces + 2^20) and returns ATR_E_NOMEM, with *out untouched, as soon as they
   pass it. A split never lowers that sum, so a mesh is refused whatever the order of the build; every
   tree the reference does finish within the budget is unchanged (the largest ratio of references to
   faces among the meshes the tests build is 3.0: DESIGN.md section 3, "Tree build"). */
int atr_octree_build(const atr_mesh* m, uint32_t max_faces, atr_octree** out);
/* A tree the caller already built (e.g. the reference's own KD_Tree walked into arrays):
   per node 6 floats (min, max) and children_start_position (0 = leaf); per leaf node its
   primitive range into prim_vertices (9 floats each) / prim_face. */
int atr_octree_from_nodes(int32_t nnodes, const float* node_bounds, const int32_t* node_children,
                          const uint32_t* leaf_first, const uint32_t* leaf_count, uint32_t nprims,
                          const float* prim_vertices, const uint32_t* prim_face, atr_octree** out);
/* f3: the same build on GPU `device` (atray_amd/csrc/build.hip): level-synchronous
   split sums and ordered vertex-in-box partitions as HIP kernels, nodes numbered in the
   reference's LIFO order on the host. Result bit-identical to atr_octree_build, its reference budget
   and ATR_E_NOMEM included: the budget is checked on the host from each level's counts before the next
   level's primitive list is allocated or filled. ms_out (may be NULL): [0] wall time of the call incl.
   transfers, [1] device time of the build kernels. */
int atr_octree_build_device(const atr_mesh* m, uint32_t max_faces, int32_t device, atr_octree** out,
                            float ms_out[2]);
void atr_octree_free(atr_octree* t);
/* Copy the flattened tree out (any pointer may be NULL): 6 floats and children_start_position
   per node, leaf primitive range per node, 9 floats + face index per leaf primitive. */
int atr_octree_export(const atr_octree* t, float* node_bounds, int32_t* node_children,
                      uint32_t* leaf_first, uint32_t* leaf_count, float* prim_vertices,
                      uint32_t* prim_face);
/* nodes, inner, leaves, empty leaves, leaf primitive refs, max leaf, depth */
int atr_octree_stats(const atr_octree* t, int64_t stats_out[7]);

/* Model (model.h:66-71). tree == NULL selects the brute-force branch (renderer.cpp:58-82). */
typedef struct {
    const atr_mesh* mesh;
    const atr_octree* tree;
    float surrounding_aabb[6];
    int32_t material;
} atr_model;
typedef struct { atr_vec3 center; float radius; int32_t material; } atr_sphere; /* sphere.h:5-10 */
typedef struct { atr_vec3 normal; float distance; int32_t material; } atr_plane; /* plane.h:5-10 */

/* Camera (camera.h:9-21) + RenderSettings (settings.h:4-10). atr_camera_set = set_camera. */
typedef struct {
    int32_t width, height;
    int32_t anti_aliasing;
    uint32_t samples_per_pixel;
    int32_t bounce_limit;
    float aspect_ratio;
    atr_vec3 camera_z, camera_x, camera_y, eye, frame_center;
    float h_fov, half_pixel_width, half_pixel_height;
} atr_camera;
int atr_camera_set(atr_camera* cm, atr_vec3 eye, atr_vec3 facing, int32_t width, int32_t height,
                   int32_t anti_aliasing, uint32_t spp, int32_t bounce_limit, float h_fov);

/* Tile (PL_math.h:147-149,185): inclusive pixel rect, row 0 = bottom. */
typedef struct { int32_t min_x, min_y, max_x, max_y; } atr_tile;
/* Reference tile grid (renderer.cpp:406-445): side W/threads (or H/threads), rects overlap by
   one pixel. Returns the tile count; writes at most cap tiles. */
int32_t atr_make_tiles(int32_t width, int32_t height, int32_t threads, atr_tile* out, int32_t cap);
/* Engine tiling for sharding: non-overlapping side x side tiles, tile k owned by rank
   k % world (interleaved for load balance). Returns the count written for `rank`. */
int32_t atr_make_shard_tiles(int32_t width, int32_t height, int32_t side, int32_t rank,
                             int32_t world, atr_tile* out, int32_t cap);
/* Cost-balanced alternative: the same side x side grid (row-major, costs[i] per grid tile, e.g.
   from atr_render_tile_costs) dealt longest-first to the least loaded rank; rank 0 starts with
   rank0_extra (its frame assembly). Writes owner_out[i] per grid tile; returns the tile count. */
int32_t atr_balance_shard_tiles(int32_t width, int32_t height, int32_t side, int32_t world,
                                const int64_t* costs, int64_t rank0_extra, int32_t* owner_out);

/* Live-view output (texture.cpp:66-115, Write_To_File): the BGRX u32 image (row 0 = bottom) as a
   32-bit BI_BITFIELDS BMP, 14-byte file header + 56-byte header, written to the first of
   "<name>_0.bmp", "<name>_1.bmp", ... that does not exist yet (created exclusively). The path
   taken goes to out_path (out_cap bytes, may be NULL). Like the reference's name buffer of
   strlen(name) + 8 bytes, ids stop at 99: ATR_E_IO once <name>_0 .. <name>_99 all exist, or the
   file cannot be created. Host memory only; no device needed. */
int atr_write_bmp(const uint32_t* pixels, int32_t width, int32_t height, const char* name, char* out_path,
                  int32_t out_cap);

/* ---------------------------------------------------------------- device engine */
typedef struct atr_ctx atr_ctx;
/* atr_create reads one environment variable, for A/B runs: ATR_CAMERA_PADS=0 makes this context's
   primary-only kernels compute each cluster's box growths per ray instead of reading them from the
   per-camera table; unset or any other value: the table. Same output bits either way.
   And a second one: ATR_WAVE_CULL=0 makes them test every cluster of a leaf per ray instead of
   first culling the leaf's clusters against the wave's direction hull; same bits.
   And a third: ATR_FACING_FOLD=0 leaves the table's loose growths unfolded, sized for the smallest
   det the culled test accepts instead of the camera's det floor per cluster; same bits.
   And a fourth: ATR_LEAF_BOX=0 builds no per-camera table of leaf boxes, so the primary passes insert
   every leaf the reference scans instead of leaving out those whose grown content the ray misses
   (DESIGN.md 4b); same bits.
   And a fifth: ATR_SKY_PATH=0 makes every wavefront of the primary-only kernels walk the scene, also
   those none of whose rays passes any model's first box test; same bits. */
int atr_create(int device, atr_ctx** out);
int atr_destroy(atr_ctx* ctx);
const char* atr_version(void);

/* Scheduling knobs of a context. They change launch order and work distribution only, never an
   output bit (every value is covered by the GPU parity tests). atr_default_tuning fills the
   measured defaults; atr_set_tuning validates and copies (ATR_E_INVALID on an out
   of range field); cluster_size takes effect at the next
   atr_scene_upload, the others at the next launch. */
typedef struct {
    int32_t xcd_chunk;      /* cell schedules: consecutive workgroups per XCD chunk (0 = one
                               contiguous range per XCD), 0..4096; default 16 */
    int32_t frame_rotate;   /* multi-frame launches: frame f's cell list starts f/F x this/1024 of
                               the way in, 0..1024; default 0 */
    int32_t hybrid_a, hybrid_b; /* HYBRID: a leaf step is dealt over the lanes when the largest
                               cluster count exceeds a x rounds + b, -4096..4096; default 2, 0 */
    int32_t path_batch_log2; /* PATHS: paths per batch = 2^this (the path queues hold one batch,
                               144 B per path, 156 with the queue sort), 12..28; default 28
                               (1920x1080 at 64 spp: a frame in one batch). A workspace holds the
                               launch's paths rounded up to 2^24, at most one batch: 20.9 GB for a
                               1920x1080 64-spp frame, 42 GB at most (4 per context: 167 GB);
                               a workspace too small for a later launch grows to a whole batch.
                               2^29 measured 5-7x slower */
    int32_t cluster_size;   /* primitives per leaf cluster, 1..16; default 16 */
    int32_t frame_plan;     /* 1: a single-frame launch on the stream of the previous ones
                               dispatches its tiles' cells by the measured cost of the launch two
                               before it, heaviest first, the heaviest 1 % over two waves (built on
                               the GPU on the context's plan stream after each such launch, beside
                               the next one); 0: list order; default 1. With an
                               atr_set_cell_plan plan for the image size it re-orders that plan's
                               block list */
    int32_t path_camera_occ; /* PATHS: waves/SIMD of the camera-ray and bounce launches, 5..7, */
    int32_t path_bounce_occ; /* or 0 = the measured default */
    int32_t primary_occ;    /* HYBRID primary cell launches: waves/SIMD 6, 7 or 8, or 0 = the
                               measured default (8 for one frame, 7 for frames in flight;
                               DESIGN.md §4e) */
    int32_t path_sort_bits; /* PATHS: 2..7 = each level's queue is put in the order of (the ray's
                               direction cell, 16 x 16 octahedral; its origin's cell, this many
                               bits per axis of the scene box) before the next bounce launch, so a
                               wavefront takes rays that walk the same tree nodes (6 at most is
                               used); 0 = queue order; default 5 */
    int32_t path_split;     /* PATHS: 1 = a launch that is one batch (a single frame) runs as two
                               half batches on two internal streams, forked from and joined back
                               into the render's stream; 0 = one stream */
    int32_t reserved[4];    /* must be 0 (ATR_E_INVALID otherwise) */
} atr_tuning;
void atr_default_tuning(atr_tuning* out);
int atr_set_tuning(atr_ctx* ctx, const atr_tuning* tuning);
int atr_get_tuning(atr_ctx* ctx, atr_tuning* out);

/* Flatten + upload the scene (copies; the caller keeps its buffers). prep_scene's tree build
   happens before this call (atr_octree_build); upload is not part of the render timing.
   An upload rejected for its input (ATR_E_INVALID, ATR_E_TREE_DEPTH, ATR_E_TREE_LAYOUT) is
   rejected as a whole and leaves the scene uploaded before in place. */
int atr_scene_upload(atr_ctx* ctx, const atr_material* materials, int32_t nmaterials,
                     const atr_model* models, int32_t nmodels, const atr_sphere* spheres,
                     int32_t nspheres, const atr_plane* planes, int32_t nplanes);
/* device bytes of the uploaded scene, per-model node count and max tree depth */
int atr_scene_info(atr_ctx* ctx, int64_t* device_bytes, int32_t* max_nodes, int32_t* max_depth);
/* Path-engine workspaces held by the context (PATHS: two path queues + per-path results, 144 B per
   path of a batch): how many (at most 4, whatever the number of streams rendering: a stream without
   one takes an idle or the least recently used one) and their device bytes. When the device cannot
   hold a batch's workspace the engine halves the batch (down to 2^16 paths), then renders on FLAT,
   which needs none; outputs are identical either way. */
int atr_workspace_info(atr_ctx* ctx, int32_t* workspaces, int64_t* device_bytes);

/* Output layout of a render. IMAGE: pixel (x,y) at y*width + x. PACKED: the pixels of the
   render's work blocks back to back (atr_render_packed_size); atr_unpack scatters them. */
enum { ATR_LAYOUT_IMAGE = 0, ATR_LAYOUT_PACKED = 1 };

/* Per-pixel outputs; DEVICE pointers (hipMalloc / torch cuda tensors). Optional ones may be
   NULL. framebuffer: BGRX u32 (texture.h:27-38). hit_face/hit_t: primary-ray closest hit of
   sample 0 (face index, 0xFFFFFFFF = miss; t = 3.402823466e38 on miss). rgb: 3 floats per pixel,
   the spp average before clamp (renderer.cpp:358). ray_casts: the reference's per-pixel
   non-sky bounce count (renderer.cpp:260). traced_rays: one u64 accumulator (+= every
   get_intersection_data-equivalent call). */
typedef struct {
    int32_t layout;
    uint32_t* framebuffer;
    uint32_t* hit_face;
    float* hit_t;
    float* rgb;
    uint32_t* ray_casts;
    unsigned long long* traced_rays;
} atr_frame;

/* Kernel variant: AUTO picks the fastest exact variant (HYBRID for primary-only renders -- one
   sample, bounce_limit 1, no AA -- else PATHS, or FLAT beyond 64 bounces). All variants are
   bit-identical; any other value is ATR_E_INVALID. (Codes 2-7 were round-1..3 schedules measured
   slower and removed) */
enum { ATR_KERNEL_AUTO = 0,
       ATR_KERNEL_LANE = 1 /* the reference's exact work: every triangle of every scanned leaf */,
       ATR_KERNEL_FLAT = 8 /* cell megakernel: clustered scan, the wavefront's (ray, cluster) work
                              dealt over its lanes in rounds, a pixel's samples in sequence */,
       ATR_KERNEL_HYBRID = 9 /* cell kernel, per leaf step: lane-private scans when the rays' cluster
                                counts are alike, FLAT rounds when one ray's leaf dominates */,
       ATR_KERNEL_PATHS = 10 /* sample-parallel path engine: one lane per (pixel, sample) path, one
                                launch per bounce over a queue of the live paths (<= 64 bounces) */ };

/* start_render_from_camera: renders the pixels of `tiles` (inclusive rects; overlapping pixels
   are traced once) into `frame`, enqueued on `stream` (hipStream_t; NULL = the null stream, HIP's
   convention). RNG: one deterministic PCG stream per (pixel, sample) from `seed`.
   Returns immediately. */
int atr_render_start(atr_ctx* ctx, const atr_camera* cam, const atr_tile* tiles, int32_t ntiles,
                     const atr_frame* frame, uint64_t seed, void* stream);
/* Progressive start for a live view (app.cpp:162-186): the tiles are rendered in list order,
   tiles_per_launch per launch, so atr_render_wait's tiles_done grows while the render runs and
   the finished tiles of the IMAGE framebuffer can be shown. Each pixel is still traced once (a
   pixel of overlapping tiles belongs to the first), and every output equals atr_render_start's. */
int atr_render_start_progressive(atr_ctx* ctx, const atr_camera* cam, const atr_tile* tiles, int32_t ntiles,
                                 const atr_frame* frame, uint64_t seed, void* stream, int32_t variant,
                                 int32_t tiles_per_launch);
/* Like atr_render_start with an explicit kernel variant. */
int atr_render_start_ex(atr_ctx* ctx, const atr_camera* cam, const atr_tile* tiles, int32_t ntiles,
                        const atr_frame* frame, uint64_t seed, void* stream, int32_t variant);
/* Sample-progressive rendering: one PASS of a single frame. Renders samples first_sample ..
   first_sample + cam->samples_per_pixel - 1 of every pixel of `tiles` (cam->samples_per_pixel is
   the pass's size, not the frame's). sample_sum: a DEVICE buffer of 3 floats per output slot, laid
   out and indexed as frame->rgb (IMAGE or PACKED; not the same memory as rgb), holding the f32 sum
   of the pixel's sample colours in sample order. first_sample == 0: sample_sum is written, never
   read. first_sample > 0: it is read as the accumulator's starting value and the new sum is written
   back. After the pass, with total = first_sample + samples_per_pixel:
     framebuffer, rgb  sum / float(total), then the usual clamp and quantisation;
     ray_casts         cumulative (first_sample > 0: read, added to, written back);
     hit_face, hit_t   written only by the pass with first_sample == 0 (the frame's sample 0, or
                       the miss record); later passes leave them untouched;
     traced_rays       accumulates as always.
   Contract: passes with the same camera (but for samples_per_pixel), tiles, seed, layout and
   buffers, issued in order on ONE stream and covering [0, N) without gap or overlap, leave every
   output equal to atr_render_start_ex with samples_per_pixel = N, bit for bit; after each pass
   every output equals that render with samples_per_pixel = total. (Every (pixel, sample) has its
   own PCG stream, independent of samples_per_pixel, and a pass performs exactly the one-shot
   render's f32 additions, continued from the stored sum.) first_sample == 0 with the full sample
   count equals atr_render_start_ex.
   Ordering between passes is stream order: they may be enqueued back to back without waiting, and
   atr_render_wait covers the last one enqueued. Passes of one frame on different streams are the
   caller's synchronisation problem. The path-engine workspace is sized by the pass, so a frame of
   many samples can be split into passes that fit a small workspace.
   ATR_E_INVALID: sample_sum == NULL; samples_per_pixel == 0; first_sample + samples_per_pixel >
   2^24 (the stream hash and float(total)); a variant other than AUTO, PATHS or FLAT (AUTO: PATHS up
   to 64 bounces, else FLAT; LANE and HYBRID do not take passes); and atr_render_start_ex's checks. */
int atr_render_start_samples(atr_ctx* ctx, const atr_camera* cam, const atr_tile* tiles, int32_t ntiles,
                             const atr_frame* frame, uint64_t seed, void* stream, int32_t variant,
                             uint32_t first_sample, float* sample_sum);
/* Adaptive sampling: a sample pass (atr_render_start_samples) that skips the pixels that have
   stopped. sample_count: a DEVICE buffer of one u32 per output slot, indexed as frame->rgb and
   sample_sum: the samples the pixel has received, and bit 31 (ATR_SAMPLES_CONVERGED) once it has
   stopped for good. A pixel is LIVE in a pass iff first_sample == 0, or sample_count[o] ==
   first_sample exactly with the flag clear. first_sample == 0: sample_count and sample_sum are
   written, never read.
   A live pixel does exactly what it does in atr_render_start_samples, then sample_count[o] =
   first_sample + n (n = cam->samples_per_pixel), and if first_sample > 0 it is tested, in separately
   rounded f32 operations (sum_before, sum_after: its sample_sum before and after the pass):
     a = sum_before / float(first_sample)         m = sum_after / float(first_sample + n)   (= rgb)
     d = (|m.x - a.x| + |m.y - a.y|) + |m.z - a.z|        l = ((m.x + m.y) + m.z) + 0.01f
     converged iff d < tolerance * l      (strict: tolerance 0 never stops a pixel; nor does a NaN)
   and a converged pixel gets ATR_SAMPLES_CONVERGED OR-ed into its count. The first pass tests
   nothing: its size is the caller's minimum sample count.
   A pixel that is not live: nothing of it but its count is read, none of its outputs (framebuffer,
   rgb, ray_casts, sample_sum, sample_count, hit_*) is written and it traces no ray, so traced_rays
   grows by the live pixels' rays only. Hence after any number of passes every pixel's outputs equal
   the one-shot render with samples_per_pixel = that pixel's own count, bit for bit.
   The path engine only (variant AUTO or PATHS, at most 64 bounces); there is no fallback to a cell
   kernel: if no path workspace can be had the call returns -(1000 + hipErrorOutOfMemory) before
   anything is enqueued, every buffer untouched. Nothing is read back to the host: passes may be
   enqueued back to back like sample passes.
   ATR_E_INVALID: atr_render_start_samples' checks; sample_count == NULL; tolerance negative, NaN or
   infinite; a variant other than AUTO or PATHS; bounce_limit > 64. */
#define ATR_SAMPLES_CONVERGED 0x80000000u
int atr_render_start_adaptive(atr_ctx* ctx, const atr_camera* cam, const atr_tile* tiles, int32_t ntiles,
                              const atr_frame* frame, uint64_t seed, void* stream, int32_t variant,
                              uint32_t first_sample, float* sample_sum, uint32_t* sample_count,
                              float tolerance);
/* The counts of the last adaptive pass enqueued on the context; valid once atr_render_wait
   returned 0. info_out[0] pixels live at the start of the pass, [1] blocks with at least one live
   pixel (the launch's 8x8 cells, or their row bands under a cell plan), [2] camera path groups
   traced (64 consecutive paths of one block's live pixels), [3] pixels still live after the pass
   ([0] minus the newly converged; 0 = further passes would do nothing). ATR_E_INVALID if the
   context has enqueued no adaptive pass. */
int atr_render_adaptive_info(atr_ctx* ctx, int64_t info_out[4]);
/* Frames in flight in one launch (throughput, e.g. a live view rendering ahead): nframes renders
   of the same camera and tiles; frame f's outputs start frame_stride elements after frame f-1's
   (rgb: 3 x frame_stride floats; frame_stride >= the layout's pixels per frame). The cell
   schedules run all frames as one grid, so one frame's slow cells overlap the next frame's; the
   path engine runs the frames' cells as one list. Every frame equals atr_render_start_ex's
   output. */
int atr_render_start_frames(atr_ctx* ctx, const atr_camera* cam, const atr_tile* tiles, int32_t ntiles,
                            const atr_frame* frame, int32_t nframes, int64_t frame_stride, uint64_t seed,
                            void* stream, int32_t variant);
/* The same with one camera per frame (an animation, a camera path): frame f renders cams[f]
   (1 <= nframes <= 24). All cameras must share width, height, samples_per_pixel, bounce_limit
   and anti_aliasing (ATR_E_INVALID otherwise); eye, facing and field of view may differ. Every
   frame equals atr_render_start_ex's output for its camera. */
int atr_render_start_cameras(atr_ctx* ctx, const atr_camera* cams, int32_t nframes, const atr_tile* tiles,
                             int32_t ntiles, const atr_frame* frame, int64_t frame_stride, uint64_t seed,
                             void* stream, int32_t variant);
/* Load-balance calibration, synchronous: renders `tiles` once (default kernel) and returns the
   GPU shader clocks spent per tile (sum over the 8x8 blocks whose area first falls in the tile,
   list order). Used to deal shard tiles to GPUs by measured cost (atray_amd/shard.py). */
int atr_render_tile_costs(atr_ctx* ctx, const atr_camera* cam, const atr_tile* tiles, int32_t ntiles,
                          uint64_t seed, int64_t* cost_out);
/* Diagnostic, synchronous: an instrumented render of the same work that returns
   [0] traced rays, [1] box tests, [2] triangle tests, [3] leaves scanned -- the reference's own
   per-ray work on this input (kd_tree.cpp:337-465) for every variant but the clustered ones,
   whose [2] counts the full triangle tests they still run -- and the engine's [4] wave-level
   triangle iterations, [5] DFS passes, [6] all octree box tests, [7] wavefronts, [8] cluster
   boxes tested and [9] primitives screened by the clustered scan. */
int atr_render_counters(atr_ctx* ctx, const atr_camera* cam, const atr_tile* tiles, int32_t ntiles,
                        uint64_t seed, int32_t variant, int64_t counters_out[10]);
/* Diagnostic, synchronous: the same instrumented render's counters of the primary kernels' wave
   cull: [0] (wavefront, cluster) pairs culled against the wave's direction hull
   before the per-ray tests (0 with ATR_WAVE_CULL=0 and for every kernel without the cull),
   [1] wave-level iterations of the lane-private cluster loop, [2] dealt rounds, [3] dealt items,
   [4] the per-ray cluster tests run ([8] of atr_render_counters less the culled ones). */
int atr_render_cull_counters(atr_ctx* ctx, const atr_camera* cam, const atr_tile* tiles, int32_t ntiles,
                             uint64_t seed, int32_t variant, int64_t counters_out[5]);
/* Diagnostic, synchronous: the same instrumented render's counters of the facing fold (DESIGN.md
   §4b), the work that the folded table takes from the primary kernels: [0] (ray, cluster) pairs that
   pass the unfolded loose box and fail the folded one, [1] the primitives that were screened for
   them. Both 0 with ATR_FACING_FOLD=0 or ATR_CAMERA_PADS=0 and for every kernel without the table. */
int atr_render_fold_counters(atr_ctx* ctx, const atr_camera* cam, const atr_tile* tiles, int32_t ntiles,
                             uint64_t seed, int32_t variant, int64_t counters_out[2]);
/* Diagnostic, synchronous: the row of the table of box growths that a one-camera launch of this
   context at `eye` reads, built as the launch builds it: the same table kernel with the same
   arguments (with ATR_FACING_FOLD=0 the kernel that fills the unfolded table). Returns the scene's
   cluster count n (or an error < 0); with row == NULL or cap < n nothing else is done. Every index in
   [0, n) is a cluster of one of the scene's tree models. row: 4 f32 per cluster = the table's entry
   {loose growth (folded), tight growth}, then {det floor delta, bits(mask of the primitive slots
   treated as rejected for every ray)}, side outputs of the folding kernel (with ATR_FACING_FOLD=0 of
   a second launch of it with the fold switched off: kTol and 0). From the same launch as the second
   pair: boxes (may be NULL), 12 f32 per cluster = {lo.xyz, P}{hi.xyz, q}{unfolded loose growth, 0,
   0, 0}; edges (may be NULL), 96 f32 per cluster = ab.xyz, ac.xyz of its 16 primitive slots, 0 past
   its count. */
int64_t atr_camera_pads_row(atr_ctx* ctx, const float eye[3], float* row, float* boxes, float* edges, int64_t cap);
/* Diagnostic, synchronous: the same instrumented render's counters of the primary kernels' leaf boxes
   (DESIGN.md §4b). The instrumented render scans every leaf; it runs the leaf test only to count
   [0] the (ray, leaf) visits whose leaf the product kernels' passes leave out, and [1] those of them in
   which a cluster passed the table's loose box all the same -- always 0. Both 0 with ATR_LEAF_BOX=0 or
   ATR_CAMERA_PADS=0 and for every kernel without the table. */
int atr_render_leaf_box_counters(atr_ctx* ctx, const atr_camera* cam, const atr_tile* tiles, int32_t ntiles,
                                 uint64_t seed, int32_t variant, int64_t counters_out[2]);
/* Diagnostic, synchronous: the same instrumented render's count of the primary kernels' sky cells
   (DESIGN.md §4a): the wavefronts (8x8 cells, or parts of split cells) none of whose pixels' rays passes
   the first box test of any model, which the product kernels finish from their arguments without
   reading the scene. The instrumented render walks the scene for them as for every other wavefront and
   only counts them. 0 with ATR_SKY_PATH=0, in a scene with a sphere, a plane or more than 4 models,
   and for every kernel without the path (LANE, every launch that is not primary-only). */
int atr_render_sky_cells(atr_ctx* ctx, const atr_camera* cam, const atr_tile* tiles, int32_t ntiles,
                         uint64_t seed, int32_t variant, int64_t* cells_out);
/* Diagnostic, host-only: what the sky path's kernels get of the uploaded scene, as they load it.
   info = {path usable (0 with ATR_SKY_PATH=0, a sphere, a plane or more than 4 models), models
   recorded, bit i set: model i is brute force and its box is tested as its surrounding_aabb is (else
   the root node's bounds of its tree), the hit_face of a sky pixel}; values = {the hit_t of a sky
   pixel, the sky's emission (3), then 6 floats per model slot (4 slots): lo.xyz, hi.xyz of the box
   its query starts with, 0 past the models recorded}. atr_sky_record_host computes the same record
   from an upload's arguments without a context or a device (and so without ATR_SKY_PATH). */
int atr_scene_sky_record(atr_ctx* ctx, int32_t info[4], float values[28]);
int atr_sky_record_host(const atr_material* mats, int32_t nmats, const atr_model* models, int32_t nmodels,
                        int32_t nspheres, int32_t nplanes, int32_t info[4], float values[28]);
/* Diagnostic, synchronous: the row of the table of leaf boxes that a one-camera launch of this context
   at `eye` reads, built as the launch builds it (the row of box growths of atr_camera_pads_row, then
   the boxes from it), whether or not ATR_LEAF_BOX switched the table off. Returns the scene's leaf
   count n -- the leaves of its tree models in model order, each model's by discovery rank -- or an
   error < 0; with row == NULL or cap < n nothing else is done. row: 8 f32 per leaf = {LO.xyz,
   bits(flag)}{HI.xyz, 0}; flag 0: a ray from the eye that misses [LO, HI] passes no cluster of the leaf,
   1: a leaf without clusters, 2: never left out (a non-finite operand). ranges (may be NULL): 2 int32
   per leaf = its first cluster in atr_camera_pads_row's numbering and its cluster count. */
int64_t atr_camera_leaf_boxes_row(atr_ctx* ctx, const float eye[3], float* row, int32_t* ranges, int64_t cap);
/* Number of pixels a PACKED render of these tiles writes. */
int64_t atr_render_packed_size(const atr_tile* tiles, int32_t ntiles);
/* Host-only: pixel index (y * width + x) of every slot of a PACKED render of these tiles, in
   slot order (lets a host consumer read packed buffers). Returns the slot count. */
int64_t atr_packed_pixel_map(const atr_tile* tiles, int32_t ntiles, int32_t width, int32_t height,
                             int64_t* out, int64_t cap);
/* Scatter a PACKED buffer (u32 per pixel) of these tiles into an IMAGE buffer (device). */
int atr_unpack(atr_ctx* ctx, const atr_tile* tiles, int32_t ntiles, int32_t width,
               const uint32_t* packed, uint32_t* image, void* stream);
/* Per-tile sum of an IMAGE ray_casts buffer over inclusive (possibly overlapping) tile rects
   -> the reference's RenderTile::ray_casts (renderer.h:11-15); out is a device int64 array. */
int atr_tile_ray_casts(atr_ctx* ctx, const atr_tile* tiles, int32_t ntiles, int32_t width,
                       const uint32_t* ray_casts_image, int64_t* out, void* stream);
/* Per-tile sums of a PACKED ray_casts buffer holding `nframes` frames (frame f at f *
   frame_stride elements) rendered with these tiles at width x height -- the reference's
   RenderTile::ray_casts (renderer.h:11-15, summed at renderer.cpp:465-468) for a shard's tiles
   without an IMAGE copy: out[f * ntiles + i] = sum over the pixels of tile i (a pixel of
   overlapping tiles counts in the first tile holding it: the packed layout traces it once).
   Asynchronous on `stream`; out is a device int64 array, zeroed here. */
int atr_packed_tile_ray_casts(atr_ctx* ctx, const atr_tile* tiles, int32_t ntiles, int32_t width,
                              int32_t height, const uint32_t* packed_ray_casts, int32_t nframes,
                              int64_t frame_stride, int64_t* out, void* stream);
/* Multi-GPU frame exchange in 3 bytes per pixel (the framebuffer's X byte is always 0,
   texture.h:27-38). atr_pack_bgr: npixels BGRX u32 -> 3 * npixels bytes (B, G, R per pixel).
   atr_scatter_bgr: the inverse with a scatter, image[dst_index[i]] = B | G << 8 | R << 16 for
   pixel i of `packed` (e.g. rank 0's gathered shard frames and their assembly index). Device
   pointers; asynchronous on `stream`. */
int atr_pack_bgr(atr_ctx* ctx, const uint32_t* framebuffer, int64_t npixels, uint8_t* out, void* stream);
int atr_scatter_bgr(atr_ctx* ctx, const uint8_t* packed, int64_t npixels, const int64_t* dst_index, uint32_t* image,
                    void* stream);
/* Lossless masked exchange (round 6): frames that are mostly one background value (a c3 frame is
   86% sky) travel as a bit per pixel plus 3 bytes for each pixel that differs from `background`
   (any value is correct; the common one compresses best): ~0.54 B per c3 pixel instead of 3.
   Stream: a 16-byte header {magic "ATRN", background, chunks, payload pixels}, one u32 payload
   offset per 8192-pixel chunk, 1 KB of mask bits per chunk, 512 B of group offsets per chunk (the
   payload offset of every 64 pixels, so decoders need no scan), then B, G, R of every
   non-background pixel in order. atr_pack_bgr_masked_bound(n) = the largest stream for n pixels (host, no device;
   size `out` by it); atr_pack_bgr_masked writes the stream and its exact byte count to the DEVICE
   int64 *nbytes (the sender ships that many bytes); atr_scatter_bgr_masked decodes a stream of
   npixels into image[dst_index[i]] (as atr_scatter_bgr). Device pointers; async on `stream`;
   npixels < 2^32. */
int64_t atr_pack_bgr_masked_bound(int64_t npixels);
int atr_pack_bgr_masked(atr_ctx* ctx, const uint32_t* framebuffer, int64_t npixels, uint32_t background, uint8_t* out,
                        int64_t* nbytes, void* stream);
int atr_scatter_bgr_masked(atr_ctx* ctx, const uint8_t* packed, int64_t npixels, const int64_t* dst_index,
                           uint32_t* image, void* stream);
/* The masked stream of a PACKED render of these tiles (nframes frames, as atr_pack_bgr_masked wrote
   it from that render's framebuffer) straight into IMAGE frames: frame f's pixel (x, y) at
   image[f * image_stride + y * width + x]. Positions come from the tile list's 8x8 blocks (as
   atr_unpack) instead of an index per pixel: ~5 B of traffic per pixel instead of ~13. The encoded
   frames must be contiguous (the render's frame_stride == its packed pixels, atr_render_packed_size):
   with `own` packed pixels per frame, stream pixel f * own + slot is frame f's packed slot. */
int atr_unpack_masked(atr_ctx* ctx, const atr_tile* tiles, int32_t ntiles, int32_t width, int32_t height,
                      const uint8_t* packed, int32_t nframes, uint32_t* image, int64_t image_stride, void* stream);
/* Several masked streams into the same IMAGE frames in one call (rank 0's received shards, one
   source per rank): source i is the PACKED render of tiles[i] (ntiles[i] tiles, the list it was
   rendered with), its stream at packed[i] (device), nframes frames each, image_stride apart; with
   raw[i] nonzero (raw may be NULL) packed[i] is that render's u32 PACKED framebuffer itself (rank
   0's own frames), copied in by the same launch. Either way a source's frames are contiguous
   (frame_stride == its packed pixels: frame f's slot k is pixel, or u32, f * own + k of
   packed[i]). The same pixels as atr_unpack_masked (or
   atr_unpack) per source, from one decode launch per 16 sources instead of a launch and an event
   per source. Asynchronous on `stream`. */
int atr_unpack_masked_ranks(atr_ctx* ctx, int32_t nsrc, const atr_tile* const* tiles, const int32_t* ntiles,
                            int32_t width, int32_t height, const uint8_t* const* packed, const int32_t* raw,
                            int32_t nframes, uint32_t* image, int64_t image_stride, void* stream);
/* Per-cell launch plan for renders of width x height (NULL clears): one byte per 8x8 cell (row
   major, ceil(W/8) x ceil(H/8)). Low nibble: the number of waves the cell is split into (0/1 =
   one, 2, 4 or 8 row bands: a heavy cell's rays then share their dealt leaf scans with 2-8x as
   many lanes and its dependent chain shortens). Bits 4-6: the cell's dispatch class c (0-7):
   cells of class 7 are dispatched first, then 6, ..., then 0 (list order within a class), e.g.
   the heaviest cells of the previous frame first (ATR_PLAN_CLASS(c) = c << 4). ATR_PLAN_PRIO:
   its waves issue at raised priority on their SIMD. Only scheduling changes: outputs and the
   PACKED slot order are identical with any plan. */
#define ATR_PLAN_CLASS(c) ((uint8_t)(((c) & 7) << 4))
enum { ATR_PLAN_PRIO = 0x80 };
int atr_set_cell_plan(atr_ctx* ctx, int32_t width, int32_t height, const uint8_t* plan);
/* Diagnostic, synchronous: the single-frame plan of a tile list (tuning frame_plan) built last,
   from the last planned launch's costs (the list the launch after next dispatches by): *nplanned =
   the planned block list's length (0 = no plan yet; a size query when cap is too small); per
   planned block its base block index (base_out) and lane mask (2 u32, lo then hi); cost_out = the
   clocks per base block of the last measured launch (the base list's length). */
int atr_render_plan_info(atr_ctx* ctx, const atr_tile* tiles, int32_t ntiles, int32_t width, int32_t height,
                         int32_t* base_out, uint32_t* mask_hi_lo_out, int64_t cap, uint64_t* cost_out,
                         int64_t* nplanned);
/* Measured cost (shader clocks) of every 8x8 cell of a full-frame render of `cam` with `variant`
   (cell kernels only): out has ceil(W/8) x ceil(H/8) entries, row major. Synchronous. */
int atr_render_cell_costs(atr_ctx* ctx, const atr_camera* cam, uint64_t seed, int32_t variant,
                          int64_t* out);
/* Ray queries: get_intersection_data (renderer.cpp:34-160) for a batch of the caller's own rays
   (picking, visibility between points, a light sampler or a baker of the caller's, collision
   probes). origins and directions: DEVICE pointers, 3 floats per ray. Models are visited in upload
   order with strict <, so the lowest model index wins a tie; then the spheres, then the planes;
   kind has the reference's precedence: a plane that improved t, else a sphere, else the triangle.
   Every output is written at the ray's input index.
   Directions must be normalised: the clustered scan's exclusion proofs assume |d| = 1 up to f32
   normalisation error. Every ray is tested before it is traced: all six inputs
   finite and fabsf(len2(d) - 1.0f) <= 0x1p-20f, len2(d) = (d.x*d.x + d.y*d.y) + d.z*d.z in separately
   rounded f32 operations (v * (1 / sqrtf(len2(v))) in f32 leaves at most 6 x 2^-24). A ray that
   fails is not traced: it gets kind ATR_RAY_INVALID and the miss record, and does not count in
   traced_rays. No NaN or zero direction reaches the traversal.
   variant: ATR_KERNEL_AUTO and ATR_KERNEL_FLAT = the clustered scan in its bounce flavour,
   ATR_KERNEL_LANE = the per-lane reference scan; the same bits; any other value is ATR_E_INVALID.
   sort_bits: 0 = the batch is traced in input order; 2..7 = in (direction cell, origin cell) order
   at that many bits per axis of the scene box (the path engine's queue order, tuning
   path_sort_bits; 6 at most is used; an origin outside the box counts in the edge cell); -1 = the
   context's tuning path_sort_bits; any other value is ATR_E_INVALID. No output bit depends on it.
   The order pays for incoherent batches; pass 0 for a batch that is coherent as it comes (camera
   rays in pixel order), which the sort pass only slows down.
   Asynchronous on `stream`, like a render: atr_render_wait covers it (tiles_done 0; a tree-depth
   flag surfaces as ATR_E_TREE_DEPTH), atr_last_kernel_ms times it. nrays == 0: ATR_OK, nothing is
   enqueued or written. The context keeps one grow-only query workspace (12 B per ray of the largest
   sorted batch, 8 B per sort bin), apart from the path workspaces of atr_workspace_info.
   ATR_E_INVALID: ctx NULL; hits, origins or directions NULL with nrays > 0; nrays < 0 or >= 2^31;
   a bad variant or sort_bits. ATR_E_NOSCENE before an upload. */
enum { ATR_RAY_SKY = 0, ATR_RAY_TRI = 1, ATR_RAY_SPHERE = 2, ATR_RAY_PLANE = 3, ATR_RAY_INVALID = 4 };
typedef struct {           /* DEVICE pointers, one element per ray, input order; any may be NULL */
    float* t;              /* closest t (> 1e-4, the reference's tolerance); 3.402823466e38 = none */
    uint32_t* face;        /* face index within its model; 0xFFFFFFFF unless kind == TRI */
    int32_t* model;        /* model index; -1 unless kind == TRI */
    float* uv;             /* 2 per ray: barycentrics of the closest MODEL hit found -- left in place
                              when a sphere or plane is nearer; 0, 0 when no model was hit */
    int32_t* kind;         /* ATR_RAY_* */
    int32_t* material;     /* the hit's material index; 0 (sky) for SKY and INVALID */
    float* normal;         /* 3 per ray: the hit's unit normal (not flipped); 0,0,0 for SKY/INVALID */
    unsigned long long* traced_rays; /* one accumulator, += rays actually traced */
} atr_ray_hits;
int atr_trace_rays(atr_ctx* ctx, const float* origins, const float* directions, int64_t nrays,
                   const atr_ray_hits* hits, int32_t variant, int32_t sort_bits, void* stream);

/* Occlusion queries (shadow rays, visibility between points): is there ANY hit with
   1e-4 < t < t_max along the ray (strict on both sides)? One byte per ray, no hit record.
   It is the reference's own traversal with its closest distance started at the ray's t_max instead
   of MAX_FLOAT -- how a user of the reference would cast a shadow ray. With T the ray's t_max:
     tree models   the walk of get_ray_kd_tree_intersection (root box; the root leaf, or the DFS with
                   its nodes_hit <= 4 loop and the leaves scanned in ascending distance) with closest
                   = T; the model occludes iff some leaf's scan improves on T, i.e. iff some triangle
                   of some leaf that walk reaches has 1e-4 < t < T. A leaf whose hits are all >= T does
                   not end the walk (closest-hit's stop at the first leaf that holds any hit does not
                   apply to hits that do not count).
     brute-force   the surrounding box test, then any face.
     spheres, planes  the reference's tests with the same window.
   The answer does not depend on the order of models or leaves. Triangles are tested with the
   reference's CULLED test: a back-facing triangle does not occlude, so the rays p->q and q->p can
   differ. Consequences (both tested):
     - with t_max NULL or 3.402823466e38, occluded == (atr_trace_rays' t < 3.402823466e38);
     - for any t_max, atr_trace_rays' t < t_max implies occluded. The converse fails only where
       closest-hit's first-hit-leaf rule kept a farther hit and hid a nearer one in a later leaf; there
       this query is the geometrically right one.
   origins, directions: as for atr_trace_rays (DEVICE, 3 floats per ray, the same validity test).
   t_max: DEVICE, one float per ray, or NULL = every ray unbounded (3.402823466e38). +inf counts as
   3.402823466e38; NaN, zero or negative makes the ray invalid; 0 < t_max <= 1e-4 is valid and
   VISIBLE (nothing can be accepted below the tolerance). An invalid ray (direction, origin or t_max)
   gets ATR_OCCL_INVALID, is not traced and does not count in traced_rays; no NaN reaches the traversal.
   occluded: DEVICE, one byte per ray (ATR_OCCL_*), written at the ray's input index; required when
   nrays > 0. traced_rays: optional DEVICE accumulator, += the valid rays.
   variant: ATR_KERNEL_AUTO and ATR_KERNEL_FLAT = the clustered scan with its exclusion bound started
   at t_max, ATR_KERNEL_LANE = the per-lane reference scan; the same bytes; else ATR_E_INVALID.
   sort_bits, stream, atr_render_wait, atr_last_kernel_ms, the query workspace, nrays == 0, the
   argument errors and ATR_E_NOSCENE: exactly as for atr_trace_rays. No output byte depends on
   sort_bits. No struct and no ABI version change. */
enum { ATR_OCCL_VISIBLE = 0, ATR_OCCL_OCCLUDED = 1, ATR_OCCL_INVALID = 2 };
int atr_occluded_rays(atr_ctx* ctx, const float* origins, const float* directions, const float* t_max,
                      int64_t nrays, uint8_t* occluded, unsigned long long* traced_rays,
                      int32_t variant, int32_t sort_bits, void* stream);

/* Hemisphere gathers (ambient occlusion, sky visibility, the visibility term of a lightmap or vertex
   baker): for npoints surface points with unit normals, nsamples directions per point are drawn on
   the device and each one is answered as atr_occluded_rays answers it; per point the counts and a
   bit per sample come back. No ray array exists anywhere.
   Samples. Sample s of point i is the renderer's own diffuse direction (cast_ray's random direction
   for a surface with scatter 0) on the renderer's per-(pixel, sample) PCG stream, in separately
   rounded f32 operations in this order:
     state, stream = the path stream of (seed, pixel = point_base + i, sample = first_sample + s):
                     state = splitmix64(seed ^ pixel ^ sample << 40), increment 2 pixel + 1;
     r0, r1, r2    = three rand_bi draws (-1 + 2 * (float(pcg32) * 2.328306437e-10f)), in that order;
     d             = v * (1 / sqrtf(len2(v))) with v = (r0, r1, r2) + n.
   Which samples are traced. A sample is traced iff (p, d) passes atr_trace_rays' validity test (this
   covers the NaN of a zero sum) and dot(d, n) = (d.x*n.x + d.y*n.y) + d.z*n.z > 0. The sampler reaches
   below the tangent plane for oblique normals (0 % of the draws for an axis normal, 3 to 4 % for
   others), where the culled triangle test would call an inward ray visible. A sample that is not
   traced counts in neither visible nor occluded, has mask bit 0 and does not count in traced_rays.
   What a traced sample answers: exactly atr_occluded_rays for (p, d, t_max[i]) -- the same window,
   the same culled test, the same walk.
   points, normals: DEVICE, 3 floats per point. t_max: DEVICE, one float per point, or NULL = unbounded;
   atr_occluded_rays' rules (+inf counts as 3.402823466e38; NaN, zero or negative is invalid;
   0 < t_max <= 1e-4 is valid and visible).
   Invalid points. A point is invalid when p is not finite, n fails the direction test
   (fabsf(len2(n) - 1.0f) <= 0x1p-20f) or its t_max is bad. Both its counts are 0, its mask words 0,
   its dirs 0,0,0; nothing is traced and its neighbours are untouched.
   Ranges, ATR_E_INVALID otherwise: nsamples 1..65,536; first_sample + nsamples <= 2^24;
   point_base >= 0 and point_base + npoints <= 2^39; npoints >= 0 and npoints * nsamples < 2^31.
   Split invariance (from the streams; part of the contract): a batch cut in two calls at any point,
   the second with point_base advanced by the cut, gives the per-point outputs of one call; a sample
   range cut in two calls, the second with first_sample advanced by the cut, gives counts that add up
   and masks that concatenate.
   Each call WRITES its outputs: visible, occluded and mask are zeroed on the stream by the call and
   then accumulated; nothing is added to what was there (traced_rays alone is an accumulator).
   variant: ATR_KERNEL_AUTO and ATR_KERNEL_FLAT = the clustered scan, ATR_KERNEL_LANE = the per-lane
   reference scan; the same outputs; any other value is ATR_E_INVALID. There is no sort_bits: the
   batch is coherent by origin as it comes. Asynchronous on `stream`; atr_render_wait covers it
   (tiles_done 0; a tree-depth flag surfaces as ATR_E_TREE_DEPTH), atr_last_kernel_ms times it.
   npoints == 0: ATR_OK, nothing is enqueued or written. ATR_E_INVALID also for ctx NULL and for out,
   points or normals NULL with npoints > 0. ATR_E_NOSCENE before an upload. No struct and no ABI version
   change. */
typedef struct {            /* DEVICE pointers; any may be NULL */
    uint32_t* visible;      /* per point: traced samples with no hit in (1e-4, t_max) */
    uint32_t* occluded;     /* per point: traced samples with one */
    uint32_t* mask;         /* per point ceil(nsamples/32) words; bit s%32 of word s/32 set iff sample s is visible */
    float*    dirs;         /* 3 floats per (point, sample), point-major: the generated direction */
    unsigned long long* traced_rays;   /* one accumulator, += traced samples */
} atr_gather_out;
int atr_gather_occlusion(atr_ctx* ctx, const float* points, const float* normals, const float* t_max,
                         int64_t npoints, int32_t nsamples, uint32_t first_sample, int64_t point_base,
                         uint64_t seed, const atr_gather_out* out, int32_t variant, void* stream);
/* Host only, no device: the same sampler, for a caller that weights the mask bits by direction.
   normals: HOST, 3 floats per point. dirs_out (3 floats per (point, sample), point-major) and
   traced_out (one byte per (point, sample): 1 iff the direction passes the validity test and lies
   above the tangent plane) are HOST and optional. A normal that fails the direction test gives
   0,0,0 and 0 for its samples. The same range checks; ATR_E_INVALID for normals NULL with
   npoints > 0. */
int atr_gather_directions(const float* normals, int64_t npoints, int32_t nsamples, uint32_t first_sample,
                          int64_t point_base, uint64_t seed, float* dirs_out, uint8_t* traced_out);

/* Radiance along the caller's rays (a light-probe or lightmap baker, the reflection or GI pass of a
   rasteriser, a region-of-interest or foveated re-render, a camera that is not a pinhole): what colour
   arrives along this ray, by the renderer's own shading loop (cast_ray, renderer.cpp:213-262) on the
   renderer's own streams.
   Sample. Sample s of ray i is cast_ray(o_i, d_i, bounce_limit) on the path stream of (seed,
   pixel = ray_base + i, sample = first_sample + s) (state = splitmix64(seed ^ pixel ^ sample << 40),
   increment 2 pixel + 1). No draw is made before the first intersection: the caller's ray is the
   path's first segment, as in the renderer's branch without anti-aliasing (renderer.cpp:348-357).
   Every f32 operation is separately rounded, in cast_ray's order.
   Outputs. sum is the ray's sample colours added in sample order, starting from 0 when
   first_sample == 0. When first_sample > 0, sum is required: it is read as the starting value and
   written back, and ray_casts (if given) is read, added to and written back -- the semantics of
   atr_render_start_samples. rgb = sum / float(first_sample + nsamples), not clamped.
   Consequences (each is tested):
     1. With origins/directions the primary rays of a camera without anti-aliasing in pixel order,
        ray_base = 0, the same seed, nsamples = samples_per_pixel and the same bounce_limit, rgb and
        ray_casts equal atr_render_start_ex's IMAGE rgb and ray_casts, bit for bit.
     2. A batch cut at any ray, the second call's ray_base advanced by the cut, gives the per-ray
        outputs of one call; a sample range cut in two calls that continue through sum gives the
        bits of one call.
     3. No output bit depends on sort_bits, on the tuning's path_batch_log2, or on the stream.
   Invalid rays. The validity test is atr_trace_rays' (six finite inputs, fabsf(len2(d) - 1.0f) <=
   0x1p-20f). An invalid ray is not traced. With first_sample == 0 its rgb and sum are written 0,0,0 and
   its ray_casts 0; with first_sample > 0 its sum and ray_casts are left as they are (and its rgb is
   not written). Its invalid byte is 1. Its neighbours are untouched; no NaN reaches the traversal.
   traced_rays accumulates the rays actually traced: one per valid ray for the first segment, which is
   traced once per ray and not once per sample (every sample of a ray shares it), plus one per bounce
   ray. This differs from the renderer's count, which traces the camera ray once per sample.
   sort_bits: -1 = the tuning's path_sort_bits, 0 = queue order, 2..7 as for the path engine. It orders
   each bounce level's queue; the first segment is traced in input order. With bounce_limit < 2 it has
   no effect.
   Ranges, ATR_E_INVALID otherwise: nrays 0 .. 2^31 - 1; nsamples 1..65,536; first_sample + nsamples
   <= 2^24; ray_base >= 0 and ray_base + nrays <= 2^32 (the queues carry the stream index in 32
   bits); bounce_limit 1..64; sort_bits as above. ATR_E_INVALID also for ctx NULL; for out, origins or
   directions NULL with nrays > 0; for sum NULL with first_sample > 0; for all five pointers of out
   NULL with nrays > 0. ATR_E_NOSCENE before an upload. nrays == 0: ATR_OK, nothing is enqueued or
   written.
   origins, directions: DEVICE, 3 floats per ray. Asynchronous on `stream`; atr_render_wait covers it
   (tiles_done 0; a tree-depth flag surfaces as ATR_E_TREE_DEPTH), atr_last_kernel_ms times it. It
   runs on a path workspace (atr_workspace_info counts it), in batches of the tuning's
   2^path_batch_log2 paths over groups of 64 rays. There is no cell-kernel fallback: as with an
   adaptive pass the tuned batch size is tried even below 2^16 paths, and if no workspace can be had
   the call returns -(1000 + hipErrorOutOfMemory) before anything is enqueued, every buffer untouched.
   No struct and no ABI version change. */
typedef struct {            /* DEVICE pointers; any may be NULL (sum: see above) */
    float*    rgb;          /* 3 per ray: sum / float(first_sample + nsamples), not clamped */
    float*    sum;          /* 3 per ray: the running f32 sum of the ray's sample colours, in sample order */
    uint32_t* ray_casts;    /* per ray: cast_ray's bounce count (renderer.cpp:260) summed over its samples */
    uint8_t*  invalid;      /* per ray: 1 iff the ray failed the validity test, else 0 */
    unsigned long long* traced_rays;   /* one accumulator */
} atr_radiance_out;
int atr_radiance_rays(atr_ctx* ctx, const float* origins, const float* directions, int64_t nrays,
                      int32_t nsamples, uint32_t first_sample, int64_t ray_base, int32_t bounce_limit,
                      uint64_t seed, const atr_radiance_out* out, int32_t sort_bits, void* stream);

/* Hemisphere radiance gathers (a lightmap or vertex baker, an irradiance probe, a final-gather pass):
   what light arrives at a surface point over its hemisphere. For npoints surface points with unit
   normals, nsamples paths per point are started on the device, each one the renderer's own path after
   a diffuse hit at that point; per point their colours are summed in sample order. No ray array
   exists anywhere.
   Sample. Sample s of point i, in separately rounded f32 operations in this order:
     state, stream = the path stream of (seed, pixel = point_base + i, sample = first_sample + s)
                     (state = splitmix64(seed ^ pixel ^ sample << 40), increment 2 pixel + 1);
     r0, r1, r2    = three rand_bi draws, in that order;
     d             = v * (1 / sqrtf(len2(v))) with v = (r0, r1, r2) + n
   -- exactly atr_gather_occlusion's and atr_gather_directions' direction, bit for bit. The sample is
   traced iff the point is valid, (p, d) passes atr_trace_rays' validity test and dot(d, n) > 0:
   atr_gather_occlusion's rule, so atr_gather_directions' traced_out flags describe this call too. A
   traced sample's colour is cast_ray(p, d, bounce_limit) (renderer.cpp:213-262) continued on the same
   stream after those three draws, every f32 operation separately rounded, in cast_ray's order. A
   sample that is not traced adds to nothing.
   Point outputs. sum is the traced samples' colours added in sample order; samples counts them;
   ray_casts adds up cast_ray's bounce counts over them. All three start from 0 when first_sample == 0.
   When first_sample > 0, sum and samples are required: they are read as the starting values and
   written back, and ray_casts (if given) is read, added to and written back. rgb = sum /
   float(samples), or 0,0,0 while samples == 0; not clamped. sample_rgb and dirs are per-call outputs,
   3 floats per (point, sample) of this call, point-major: written whole, never read; an untraced
   sample's sample_rgb is 0,0,0, and dirs is the generated direction whether traced or not (as
   atr_gather_out.dirs).
   Invalid points. A point is invalid when p is not finite or n fails the direction test
   (fabsf(len2(n) - 1.0f) <= 0x1p-20f). It traces nothing: its invalid byte is 1, its sample_rgb and
   dirs rows are zeros; with first_sample == 0 its rgb, sum, samples and ray_casts are written 0, with
   first_sample > 0 they are left as they are. Its neighbours are untouched; no NaN reaches the
   traversal.
   traced_rays accumulates every segment traced: one first segment per traced sample plus the bounce
   rays. Nothing is shared between samples here, so this is the renderer's count over the same
   cast_ray calls.
   Consequences (each is tested):
     1. samples[i] equals visible[i] + occluded[i] of atr_gather_occlusion with the same points,
        normals, nsamples, first_sample, point_base and seed and t_max NULL; with bounce_limit == 1,
        ray_casts[i] equals that call's occluded[i] (an unbounded occlusion query equals closest-hit
        t < 3.402823466e38, above).
     2. A batch cut at any point, the second call's point_base advanced by the cut, gives the
        per-point outputs of one call; a sample range cut in two calls that continue through sum,
        samples and ray_casts gives the bits of one call, and the sample_rgb and dirs rows concatenate.
     3. No output bit depends on sort_bits, on the tuning's path_batch_log2, or on the stream.
   There is deliberately no bit-for-bit tie to a render's pixels: after a diffuse hit the renderer
   normalises the bounce direction a second time after its lerp, traces directions below the tangent
   plane too, and carries the surface's weight into the tail's products. The tie is to cast_ray.
   sort_bits: -1 = the tuning's path_sort_bits, 0 = queue order, 2..7 as for atr_radiance_rays. It
   orders the bounce levels' queues only; the first segments are traced in (point, sample) order.
   Ranges, ATR_E_INVALID otherwise: npoints >= 0 and npoints * nsamples < 2^31; nsamples 1..65,536;
   first_sample + nsamples <= 2^24; point_base >= 0 and point_base + npoints <= 2^32 (the queues carry
   the stream index in 32 bits); bounce_limit 1..64; sort_bits as above. ATR_E_INVALID also for ctx
   NULL; for out, points or normals NULL with npoints > 0; for sum or samples NULL with first_sample >
   0; for all eight pointers of out NULL with npoints > 0. ATR_E_NOSCENE before an upload.
   npoints == 0: ATR_OK, nothing is enqueued or written.
   points, normals: DEVICE, 3 floats per point. Asynchronous on `stream`; atr_render_wait covers it
   (tiles_done 0; a tree-depth flag surfaces as ATR_E_TREE_DEPTH), atr_last_kernel_ms times it. It
   runs on a path workspace, in batches of whole points of about the tuning's 2^path_batch_log2 paths
   (at least one point; the tuned size is tried even below 2^16 paths). There is no cell-kernel
   fallback: if no workspace can be had the call returns -(1000 + hipErrorOutOfMemory) before anything
   is enqueued, every buffer untouched. No struct and no ABI version change. */
typedef struct {            /* DEVICE pointers; any may be NULL (sum, samples: see above) */
    float*    rgb;          /* 3 per point: sum / float(samples), or 0,0,0 while samples == 0; not clamped */
    float*    sum;          /* 3 per point: running f32 sum of the traced samples' colours, in sample order */
    uint32_t* samples;      /* per point: traced samples so far (the divisor) */
    uint32_t* ray_casts;    /* per point: cast_ray's bounce count summed over the traced samples */
    uint8_t*  invalid;      /* per point: 1 iff the point failed the validity test */
    float*    sample_rgb;   /* 3 per (point, sample) of THIS call, point-major: the sample's colour; 0,0,0 if untraced */
    float*    dirs;         /* 3 per (point, sample) of this call: the generated direction (as atr_gather_out.dirs) */
    unsigned long long* traced_rays;   /* one accumulator */
} atr_gather_radiance_out;
int atr_gather_radiance(atr_ctx* ctx, const float* points, const float* normals, int64_t npoints,
                        int32_t nsamples, uint32_t first_sample, int64_t point_base, int32_t bounce_limit,
                        uint64_t seed, const atr_gather_radiance_out* out, int32_t sort_bits, void* stream);

/* Light probes (lighting for moving objects, or for any normal at all, from points in free space): the
   radiance arriving at a point over the WHOLE sphere, projected on the nine real spherical harmonics
   of bands 0..2 per colour channel. A probe has no normal and no surface. For npoints probes, nsamples
   paths per probe are started on the device, each one cast_ray from the probe along a direction drawn
   uniformly over the sphere; per probe 27 sums are kept in sample order. No ray array exists anywhere.
   Every f32 operation below is separately rounded, in the order written.
   Sample. Sample s of probe i:
     state, stream = the path stream of (seed, pixel = point_base + i, sample = first_sample + s)
                     (state = splitmix64(seed ^ pixel ^ sample << 40), increment 2 pixel + 1);
     up to 32 tries, each: r0, r1, r2 = three rand_bi draws, in that order;
                           l2 = (r0*r0 + r1*r1) + r2*r2;
     the first try with 0x1p-10f <= l2 && l2 <= 1.0f is accepted: d = (r0, r1, r2) * (1 / sqrtf(l2));
     if all 32 tries fail, d = (0, 0, 1).
   Rejection inside a radial shell is uniform in direction and needs no sine or cosine, so the device
   and plain C agree bit for bit (atr_probe_directions below is the same function on the host). A try
   is accepted with probability about 0.5236; the fallback has a probability of about 1e-10 per sample
   and exists so that the loop ends on every lane. The sample's colour is cast_ray(p, d, bounce_limit)
   (renderer.cpp:213-262) continued on the same stream after those draws, exactly as in
   atr_gather_radiance. Every sample of a valid probe is traced: there is no tangent plane and no
   untraced state. The culled triangle test applies as everywhere: a probe inside a closed mesh sees
   out through its back faces.
   Basis, on d = (x, y, z), as f32 literals:
     Y0 = 0.282094792f                 Y1 = 0.488602512f*y               Y2 = 0.488602512f*z
     Y3 = 0.488602512f*x               Y4 = 1.092548431f*(x*y)           Y5 = 1.092548431f*(y*z)
     Y6 = 0.315391565f*((3.0f*(z*z)) - 1.0f)                             Y7 = 1.092548431f*(x*z)
     Y8 = 0.546274215f*((x*x) - (y*y))
   (atr_sh_basis below evaluates them on the host.)
   Probe outputs. For each sample in sample order, sum[3k+c] = sum[3k+c] + (colour.c * Yk(d)); ray_casts
   adds up cast_ray's bounce counts. Both start from 0 when first_sample == 0. When first_sample > 0,
   sum is required: it is read as the starting value and written back, and ray_casts (if given) is read,
   added to and written back. sh[3k+c] = (sum[3k+c] * 12.566370614f) / float(first_sample + nsamples):
   the Monte-Carlo estimate of the radiance's projection on Yk, not clamped. sample_rgb and dirs are
   per-call outputs, 3 floats per (probe, sample) of this call, probe-major: written whole, never read.
   Invalid probes. A probe is invalid when p is not finite. It traces nothing: its invalid byte is 1,
   its sample_rgb and dirs rows are zeros; with first_sample == 0 its sh, sum and ray_casts are written
   0, with first_sample > 0 they are left as they are. Its neighbours are untouched; no NaN reaches the
   traversal.
   traced_rays accumulates every segment traced: one first segment per sample of a valid probe plus the
   bounce rays.
   Consequences (each is tested):
     1. With bounce_limit == 1, ray_casts[i] equals the count of atr_trace_rays(p_i, dirs[i, s]) with
        t < 3.402823466e38, and the sample_rgb of the misses is the sky's emission.
     2. A batch cut at any probe, the second call's point_base advanced by the cut, gives the per-probe
        outputs of one call; a sample range cut in two calls that continue through sum and ray_casts
        gives the bits of one call, and the sample_rgb and dirs rows concatenate.
     3. No output bit depends on sort_bits, on the tuning's path_batch_log2, or on the stream.
   sort_bits: -1 = the tuning's path_sort_bits, 0 = queue order, 2..7 as for atr_radiance_rays. It
   orders the bounce levels' queues only; the first segments are traced in (probe, sample) order.
   Ranges, ATR_E_INVALID otherwise: npoints >= 0 and npoints * nsamples < 2^31; nsamples 1..65,536;
   first_sample + nsamples <= 2^24; point_base >= 0 and point_base + npoints <= 2^32 (the queues carry
   the stream index in 32 bits); bounce_limit 1..64; sort_bits as above. ATR_E_INVALID also for ctx
   NULL; for out or points NULL with npoints > 0; for sum NULL with first_sample > 0; for all seven
   pointers of out NULL with npoints > 0. ATR_E_NOSCENE before an upload. npoints == 0: ATR_OK, nothing
   is enqueued or written.
   points: DEVICE, 3 floats per probe. Asynchronous on `stream`; atr_render_wait covers it (tiles_done
   0; a tree-depth flag surfaces as ATR_E_TREE_DEPTH), atr_last_kernel_ms times it. It runs on a path
   workspace, in batches of whole probes of about the tuning's 2^path_batch_log2 paths (at least one
   probe). There is no cell-kernel fallback: if no workspace can be had the call returns
   -(1000 + hipErrorOutOfMemory) before anything is enqueued, every buffer untouched. No struct and no
   ABI version change. */
typedef struct {            /* DEVICE pointers; any may be NULL (sum: see above) */
    float*    sh;           /* 27 per probe, index 3*k + c (coefficient k = 0..8, channel c): (sum * 12.566370614f) / float(first_sample + nsamples) */
    float*    sum;          /* 27 per probe: running f32 sums, in sample order */
    uint32_t* ray_casts;    /* per probe: cast_ray's bounce count summed over its samples */
    uint8_t*  invalid;      /* per probe: 1 iff the point is not finite */
    float*    sample_rgb;   /* 3 per (probe, sample) of THIS call, probe-major */
    float*    dirs;         /* 3 per (probe, sample) of this call: the generated direction */
    unsigned long long* traced_rays;   /* one accumulator */
} atr_probe_sh_out;
int atr_probe_sh(atr_ctx* ctx, const float* points, int64_t npoints, int32_t nsamples, uint32_t first_sample,
                 int64_t point_base, int32_t bounce_limit, uint64_t seed, const atr_probe_sh_out* out,
                 int32_t sort_bits, void* stream);
/* The probes' sampler and basis on the host: no device, no context. atr_probe_directions writes the
   direction of every (probe, sample) (3 floats, probe-major; the bits atr_probe_sh's dirs holds for a
   valid probe) and the try that was accepted (1..32, or 33 for the fallback); either output may be
   NULL. Its ranges are atr_probe_sh's. atr_sh_basis writes Y0..Y8 of n directions, 9 floats each. */
int atr_probe_directions(int64_t npoints, int32_t nsamples, uint32_t first_sample, int64_t point_base,
                         uint64_t seed, float* dirs_out, uint8_t* tries_out);
int atr_sh_basis(const float* dirs, int64_t n, float* basis_out /* 9 per direction */);

/* Lightmap texels: the surface points a lightmap baker feeds to the gathers above, one per texel of
   the mesh's UV layout, made on the device; atr_texels_to_image turns per-texel results back into an
   image. Texels, gather, image: a mesh with texture coordinates goes in and a lightmap comes out.
   Every f32 operation below is separately rounded (tests/c/texel_ref.c restates them in plain C).
   Texels. A width x height map; texel (i, j) has index j*width + i and the centre
     p = ((float(i) + 0.5f) / float(width), (float(j) + 0.5f) / float(height)),
   row 0 at v near 0 (the images' bottom-row-first convention). A texcoord's u, v are the first two of
   its three floats. Texels exist only inside the map: UVs outside [0, 1) cover nothing.
   Usable faces. With a, b, c the face's three UVs, a face is usable iff its three texcoord indices are
   present (>= 0; an index past the array counts as absent), the six floats are finite and
     area2 = (b.x-a.x)*(c.y-a.y) - (b.y-a.y)*(c.x-a.x)  is neither 0 nor NaN.
   Coverage. E(p0, p1, p): if (p1.x, p1.y) is lexicographically below (p0.x, p0.y), swap the two and
   s = -1, else s = 1; E = s * ((p1.x-p0.x)*(p.y-p0.y) - (p1.y-p0.y)*(p.x-p0.x)). Two faces that share
   an edge compute the same magnitude with opposite signs, so no centre is lost between them. With
   g = 1 if area2 > 0 else -1:  e0 = g*E(b,c,p), e1 = g*E(c,a,p), e2 = g*E(a,b,p), den = (e0 + e1) + e2;
   the face covers p iff e0 >= 0 && e1 >= 0 && e2 >= 0 && den > 0. A texel's face is the LOWEST usable
   face index that covers its centre; a texel no face covers is not covered.
   Sample of a covered texel: u = e1/den, v = e2/den (the weights of the face's 2nd and 3rd vertex);
   point = (A + AB*u) + AC*v with AB = B - A, AC = C - A on the face's vertices (a vertex index outside
   the array reads as the origin, as in atr_scene_upload); normal = the renderer's own for a hit of this
   face at (u, v): with vertex normals (the mesh has any: atr_scene_upload's rule) unit(na*(1 - u - v) +
   nb*u + nc*v), else unit(cross(v0 - v1, v0 - v2)); ATR_TEXELS_FLIP negates it (a mesh wound the other
   way round). A degenerate normal (NaN) is passed through: the gathers call such a point invalid and
   leave its neighbours alone.
   Outputs. slot is per texel; the others are per covered texel k, k ascending with the texel index
   (so texel[] is ascending and slot[texel[k]] == k). *ncovered always receives the count. If cap <
   count the per-k arrays are left untouched and slot is still written: a size query (the pattern of
   atr_render_plan_info); call again with arrays of `count` elements.
   A set-up call, synchronous like atr_scene_upload and atr_octree_build_device: it runs on a stream
   of the context's own and every output is complete on return; the caller's earlier work on the
   output buffers must have finished. `mesh` is the host mesh; what the kernels read of it is copied
   into a grow-only texel workspace of the context (apart from the query and path workspaces; with the
   face map 4 B per texel), after waiting for everything the context has in flight. To bake an
   uploaded scene, pass the mesh that was uploaded, at the position it was uploaded with. No scene is
   needed. ms_out (may be NULL): [0] wall time of the call, [1] device time of its kernels.
   ATR_E_INVALID: ctx, mesh, out or ncovered NULL; a mesh without texcoords; width or height outside
   1..16,384; cap < 0; unknown flag bits. No struct and no ABI version change. */
enum { ATR_TEXELS_FLIP = 1 };       /* negate every normal */
typedef struct {                    /* DEVICE pointers; any may be NULL */
    int32_t*  slot;    /* width*height: rank k of the texel among the covered ones, or -1 */
    int32_t*  texel;   /* per covered k (ascending texel index): j*width + i */
    uint32_t* face;    /* per k: the covering face */
    float*    bary;    /* 2 per k: u, v */
    float*    point;   /* 3 per k */
    float*    normal;  /* 3 per k, unit */
} atr_texels_out;
int atr_mesh_texels(atr_ctx* ctx, const atr_mesh* mesh, int32_t width, int32_t height, int32_t flags,
                    int64_t cap, const atr_texels_out* out, int64_t* ncovered, float ms_out[2]);
/* Per-texel results into a finished lightmap: image[texel[k]] = values[k] (3 floats each), every other
   texel empty; then `passes` (0..64) dilation passes, each reading only the state at its start: an
   empty texel with n >= 1 non-empty texels among its 8 neighbours inside the map gets, per channel,
   ((0 + v_1) + ... + v_n) / float(n), the neighbours taken in the order dy = -1..1, dx = -1..1, and is
   non-empty from the next pass on; after the last pass the texels still empty get `fill` (HOST, 3
   floats). `image` (3 floats per texel, row 0 at the bottom) is written whole and must not overlap
   `values`. values, texel, image: DEVICE. texel must be ascending and unique, as atr_mesh_texels wrote
   it; that is the caller's to keep and is not checked (an index outside the map is skipped).
   Asynchronous on `stream`; atr_render_wait covers it (tiles_done 0), atr_last_kernel_ms times it.
   The passes ping-pong between `image` and a grow-only image workspace of the context (14 B per
   texel), which a call on another stream than the last first waits for on the GPU.
   ATR_E_INVALID: ctx, image or fill NULL; values or texel NULL with ncovered > 0; ncovered < 0 or >
   width*height; width or height outside 1..16,384; passes outside 0..64. */
int atr_texels_to_image(atr_ctx* ctx, const float* values, const int32_t* texel, int64_t ncovered,
                        int32_t width, int32_t height, int32_t passes, const float fill[3], float* image,
                        void* stream);

/* Guided denoising of a frame or a lightmap: the edge-avoiding a-trous wavelet filter of Dammertz et al.
   2010 (a 5x5 B3-spline tap pattern whose spacing doubles per pass; stopping weights from normal,
   position, object id and colour), with rational weights 1 / (1 + x) where the paper has Gaussians, so
   that no transcendental is involved: every f32 operation below is separately rounded
   (tests/c/denoise_ref.c restates them in plain C), dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z and
   len2(a) = dot(a, a).
   Buffers. color and out: DEVICE, 3 f32 per pixel, IMAGE layout (pixel (x, y) at y*width + x); color is
   required. guides == NULL means all three guide pointers are NULL. out == color (the same pointer) is
   allowed: color and the guides are read in full before anything is written; any other overlap is the
   caller's error and is not checked. framebuffer (optional): BGRX u32 per pixel, made from the result
   by the renderer's own clamp and quantisation per channel, k = pl_max(0, pl_min(c, 1)) with pl_max(a,
   b) = a > b ? a : b and pl_min(a, b) = a > b ? b : a, uint32_t(k * 255.0f) & 0xFF (0 for a NaN), then
   b | g << 8 | r << 16; written for every pixel. At least one of out and framebuffer is non-NULL.
   Inert pixels. Decided once, from the caller's inputs: a pixel is inert if ident is given and equals
   ATR_DENOISE_EMPTY, or any of its three colour floats is not finite, or normal is given and any of its
   three floats is not finite, or position is given and any of its three floats is not finite. An inert
   pixel keeps its input colour bit for bit through every pass and is never used as a tap (sky pixels,
   uncovered texels, NaNs from elsewhere).
   Per-pass constants, computed on the host in f32: s = 1 << p; sc = sigma_color / float(s), kc = 1.0f /
   (sc * sc) (the colour tolerance halves per pass, as in the paper); sp = sigma_position * float(s), kp
   = 1.0f / (sp * sp). The colour term is on iff sigma_color > 0, the position term iff position is
   given and sigma_position > 0.
   Pass p (0 .. passes-1) for a pixel P at (x, y) that is not inert, c_* the colours at the start of the
   pass: sum = 0,0,0, wsum = 0; for dy = -2..2 (outer), dx = -2..2 (inner): Q = (x + dx*s, y + dy*s);
   skip Q if it lies outside the image, is inert, or (ident given) ident_Q != ident_P; else
     w = h[dy+2] * h[dx+2], h = {1/16, 1/4, 3/8, 1/4, 1/16} (exact);
     normal given: c = dot(n_P, n_Q); c = c > 0 ? c : 0 (a NaN gives 0); c = c*c, normal_power_log2
       times; w = w * c;
     position term on: dv = p_Q - p_P; with normal given e = dot(n_P, dv), e2 = e*e (the distance of Q
       from P's tangent plane, so that a surface seen at a grazing angle is not cut apart), else e2 =
       len2(dv); w = w * (1.0f / (1.0f + e2 * kp));
     colour term on: d2 = len2(c_Q - c_P); w = w * (1.0f / (1.0f + d2 * kc));
     skip Q unless w > 0 (drops zero, NaN and negative weights);
     per channel sum = sum + c_Q * w; then wsum = wsum + w.
   The pixel's new colour is sum / wsum (three divisions) if wsum > 0, else c_P. The centre tap is an
   ordinary tap. Each pass reads only the state at its start; the last pass's state is `out`.
   Asynchronous on `stream`; atr_render_wait covers it (tiles_done 0), atr_last_kernel_ms times it. No
   scene is needed. The passes run in a grow-only denoise workspace of the context, apart from the
   query, path, texel and image workspaces: two colour images of 16 B per pixel (r, g, b and the id),
   and 16 B per pixel more for each of normal and position that is given (32 to 64 B per pixel); a call
   on another stream than the last first waits for it on the GPU.
   ATR_E_INVALID, with nothing enqueued or written: ctx, params or color NULL; out and framebuffer both
   NULL; width or height outside 1..16,384; passes outside 1..8; normal_power_log2 outside 0..7; a sigma
   that is negative, NaN or infinite; non-zero reserved; a term that is on whose kc or kp is, in any of
   the `passes` passes, not finite and > 0. No struct and no ABI version change. */
#define ATR_DENOISE_EMPTY 0xFFFFFFFFu
typedef struct {
    int32_t passes;            /* 1..8; pass p (from 0) has tap spacing s = 2^p */
    float   sigma_color;       /* > 0: colour term on; 0: off */
    float   sigma_position;    /* > 0: position term on; 0: off; ignored when position == NULL */
    int32_t normal_power_log2; /* 0..7: the normal term is max(dot, 0)^(2^this); ignored when normal == NULL */
    int32_t reserved[4];       /* must be 0 */
} atr_denoise_params;
typedef struct {               /* DEVICE pointers, IMAGE layout (pixel (x, y) at y*width + x); any may be NULL */
    const float*    normal;    /* 3 per pixel; need not be unit */
    const float*    position;  /* 3 per pixel */
    const uint32_t* ident;     /* per pixel: taps with another id weigh 0; ATR_DENOISE_EMPTY = inert pixel */
} atr_denoise_guides;
void atr_default_denoise_params(atr_denoise_params* out);   /* 5, 0.01f, 0.0f, 5, zeros */
int atr_denoise(atr_ctx* ctx, const float* color, const atr_denoise_guides* guides, int32_t width,
                int32_t height, const atr_denoise_params* params, float* out, uint32_t* framebuffer,
                void* stream);

/* Temporal accumulation of a frame into a history that is reprojected from the previous camera: a
   static scene and a world-space position per pixel need no motion vectors, the previous camera alone
   says where a surface point was on the previous film. The caller keeps two atr_history sets and
   ping-pongs them, and keeps the previous frame's guides (atr_denoise_guides, as atr_denoise takes
   them; Engine.render_guides makes them). Every f32 operation below is separately rounded, in the
   order written (tests/c/accumulate_ref.c restates them in plain C); dot and len2 are atr_denoise's.
   Buffers. All DEVICE, IMAGE layout. color: 3 f32 per pixel, this frame. guides: this frame's;
   prev_cam, prev_guides, prev: the previous frame's camera, guides and history (the `out` of the call
   before). prev == NULL starts a history: prev_cam and prev_guides are ignored and every live pixel
   takes the "no history" branch; guides may then be NULL (three NULL pointers). out: the new history.
   variance (optional): one f32 per pixel. framebuffer (optional): BGRX u32 per pixel, made from
   out.color by atr_denoise's clamp and quantisation, for every pixel.
   Inert pixels: atr_denoise's rule on this frame's inputs (ident given and ATR_DENOISE_EMPTY; a colour
   float that is not finite; normal given and one of its floats not finite; position given and one of
   its floats not finite). An inert pixel's out.color is the input colour's bits, its out.moments 0, 0,
   its out.length 0, its variance 0.
   Host constants: k = prev_cam->h_fov * prev_cam->aspect_ratio; hw = 0.5f * float(width), hh = 0.5f *
   float(height).
   Reprojection of a live pixel P (position p, normal n, colour c) inverts the kernels' film mapping
   film = frame_center + camera_x*fx + camera_y*fy, the film at distance 1 along -camera_z, fx = ((-1 +
   2*(x/W))*h_fov)*aspect, fy = -1 + 2*(y/H); eye and the axes are prev_cam's:
     v = p - eye; depth = -dot(v, camera_z); no history unless depth > 0;
     a = dot(v, camera_x) / depth; b = dot(v, camera_y) / depth;
     sx = (a / k + 1.0f) * hw; sy = (b + 1.0f) * hh;
     no history unless sx >= -1.0f && sx < float(width) && sy >= -1.0f && sy < float(height)
     (every comparison is written so that a NaN fails it);
     fx0 = floorf(sx), x0 = int(fx0), tx = sx - fx0; fy0 = floorf(sy), y0 = int(fy0), ty = sy - fy0.
   Taps: four, in the order (dy, dx) = (0,0), (0,1), (1,0), (1,1); Q = (x0+dx, y0+dy) in the previous
   frame, w = (dx ? tx : 1.0f - tx) * (dy ? ty : 1.0f - ty). Q is skipped if
     1. it lies outside the image;
     2. prev.length[Q] == 0;
     3. idents are given and prev_ident_Q != ident_P, or prev_ident_Q == ATR_DENOISE_EMPTY;
     4. normals are given and !(dot(n, n_Q) >= min_normal_dot);
     5. with dv = p_Q - p, e2 = e*e where e = dot(n, dv) when normals are given, else e2 = len2(dv), and
        tol = plane_tolerance * depth: !(e2 <= tol*tol);
     6. one of Q's three history colour floats is not finite or, moments given, one of its two moments;
     7. !(w > 0).
   A kept tap adds: per channel sum = sum + hc_Q * w; the two moments msum = msum + m_Q * w; wsum =
   wsum + w; nmin = min(nmin, length_Q).
   Blend. l = (0.2126f*c.x + 0.7152f*c.y) + 0.0722f*c.z. If wsum > 0: h = sum / wsum (three divisions),
   hm = msum / wsum, len = min(nmin, max_length - 1) + 1, aw = 1.0f / float(len), ac = alpha > aw ?
   alpha : aw, am = alpha_moments > aw ? alpha_moments : aw; out.color = h + (c - h) * ac; m1 = hm.x +
   (l - hm.x) * am; m2 = hm.y + (l*l - hm.y) * am; out.length = len. Else out.color = c (its bits), m1 =
   l, m2 = l*l, out.length = 1. out.moments = m1, m2; variance = m2 - m1*m1, then variance > 0 ?
   variance : 0.
   Pointers. color, out->color and out->length are required. With prev: prev_cam, prev_guides,
   guides->position, prev_guides->position, prev->color and prev->length are required; normal is in
   both guides or in neither, ident likewise, moments in both histories or in neither. variance needs
   out->moments. out->color == color is allowed (a lane reads only its own pixel of color). No out
   pointer may equal the corresponding prev pointer; only pointer equality is checked, other overlap
   is the caller's error.
   Asynchronous on `stream`; atr_render_wait covers it (tiles_done 0), atr_last_kernel_ms times it. No
   scene and no workspace are needed.
   ATR_E_INVALID, with nothing enqueued or written: a NULL among the required arguments (ctx, params,
   out included); width or height outside 1..16,384; with prev, prev_cam->width/height other than
   width/height, or a k that is not finite and > 0; alpha or alpha_moments outside [0, 1] or NaN;
   max_length outside 1..2^24; plane_tolerance not finite or not > 0; min_normal_dot outside [-1, 1] or
   NaN; non-zero reserved; any pointer rule above. atr_accumulate_check is that validation alone, on
   the host, with no context and no device (no pointer into DEVICE memory is followed): ATR_OK or
   ATR_E_INVALID. No struct and no ABI version change. */
typedef struct {            /* DEVICE, IMAGE layout, caller-owned; one frame's history */
    float*    color;        /* 3 per pixel: the accumulated colour */
    float*    moments;      /* 2 per pixel: accumulated luminance and luminance^2; may be NULL */
    uint32_t* length;       /* per pixel: frames accumulated (0 = inert pixel, 1 = no history found) */
} atr_history;
typedef struct {
    float   alpha;           /* 0..1: lower bound of the new frame's weight for colour */
    float   alpha_moments;   /* 0..1: the same for the moments */
    int32_t max_length;      /* 1..2^24: the history length saturates here */
    float   plane_tolerance; /* > 0, finite: a tap's distance from P's tangent plane, per unit of depth */
    float   min_normal_dot;  /* -1..1: a tap's normal must reach this dot with P's; ignored without normals */
    int32_t reserved[3];     /* must be 0 */
} atr_accumulate_params;
void atr_default_accumulate_params(atr_accumulate_params* out);   /* 0, 0, 64, 0.02f, 0.9f, zeros */
int atr_accumulate_check(const float* color, const atr_denoise_guides* guides, const atr_camera* prev_cam,
                         const atr_denoise_guides* prev_guides, const atr_history* prev, int32_t width,
                         int32_t height, const atr_accumulate_params* params, const atr_history* out,
                         const float* variance);
int atr_accumulate(atr_ctx* ctx, const float* color, const atr_denoise_guides* guides,
                   const atr_camera* prev_cam, const atr_denoise_guides* prev_guides,
                   const atr_history* prev, int32_t width, int32_t height,
                   const atr_accumulate_params* params, const atr_history* out,
                   float* variance, uint32_t* framebuffer, void* stream);

/* Variance-guided denoising: the spatial stage of SVGF (Schied et al. 2017) on atr_denoise's a-trous
   pattern, for frames whose noise differs from pixel to pixel, such as atr_accumulate's output (its
   `variance`, and its history's moments and length, are this call's inputs). The luminance stopping
   weight is scaled per pixel by the local standard deviation, the variance is filtered along with the
   colour, and a pixel whose history is too short to have a variance takes one from its neighbours'
   moments. Every f32 operation below is separately rounded, in the order written
   (tests/c/denoise_variance_ref.c restates them in plain C); divisions and sqrtf are IEEE; dot and len2
   are atr_denoise's; lum(c) = (0.2126f*c.x + 0.7152f*c.y) + 0.0722f*c.z is atr_accumulate's.
   Buffers. All DEVICE, IMAGE layout. color: 3 f32 per pixel; variance: 1 f32 per pixel, the variance of
   the pixel's luminance; both required. guides: atr_denoise's, each optional, NULL = three NULLs.
   moments (2 f32 per pixel) and length (u32 per pixel): an atr_history's, both given or both NULL. out
   (3 f32 per pixel), variance_out (1 f32 per pixel) and framebuffer (BGRX u32 per pixel, atr_denoise's
   clamp and quantisation of the result) are each optional; at least one of out and framebuffer is
   non-NULL. out == color and variance_out == variance are allowed: every input is read in full before
   any output is written; any other overlap is the caller's error and is not checked.
   Inert pixels: atr_denoise's rule (ident given and ATR_DENOISE_EMPTY; a colour, normal or position
   float that is not finite); the variance makes no pixel inert. An inert pixel keeps its colour bits,
   has variance_out 0 and is never a tap.
   Variance at the start, per live pixel: v = (variance > 0 && variance < inf) ? variance : 0 (a NaN, a
   negative value and an infinity give 0).
   Spatial estimate, only with moments and length given and spatial_below > 0, for a live P with
   length_P < spatial_below; it reads the caller's inputs alone, never another pixel's estimate: a = b =
   ws = 0; for dy = -3..3 (outer), dx = -3..3 (inner): Q = (x + dx, y + dy); skip Q if it lies outside
   the image, is inert, (ident given) ident_Q != ident_P, or one of its two moments is not finite; else
     w = 1.0f; normal given: atr_denoise's normal term, w = w * c; position term on: atr_denoise's
     position term with pass 0's kp; skip Q unless w > 0; a = a + m_Q.x * w; b = b + m_Q.y * w; ws = ws
     + w.
   If ws > 0: m1 = a / ws, m2 = b / ws, e = m2 - m1*m1, e = e > 0 ? e : 0; lp = length_P > 0 ? length_P :
   1; v = e * (float(spatial_below) / float(lp)) (SVGF's boost of short histories); else v stays.
   Per-pass constant, on the host in f32: s = 1 << p; sp = sigma_position * float(s), kp = 1.0f / (sp *
   sp). The position term is on iff position is given and sigma_position > 0, the luminance term iff
   sigma_luminance > 0. There is no colour constant: the tolerance shrinks as the variance does.
   Pass p (0 .. passes-1) for a live P, c_* and v_* the state at the start of the pass:
     1. the variance under a 3 x 3 Gaussian at spacing 1 (not s): gs = ks = 0; for dy = -1..1 (outer),
        dx = -1..1 (inner), over the Q inside the image, not inert and of P's ident: k = g[dy+1] *
        g[dx+1], g = {0.25f, 0.5f, 0.25f}; gs = gs + v_Q * k; ks = ks + k. gv = gs / ks.
     2. luminance term on: rl = 1.0f / (sigma_luminance * sqrtf(gv) + luminance_floor).
     3. sum = 0,0,0, vs = 0, wsum = 0; the 25 taps in atr_denoise's order and under its skips (outside,
        inert, another ident): w = h[dy+2] * h[dx+2]; atr_denoise's normal term; atr_denoise's position
        term; luminance term on: x = fabsf(lum(c_Q) - lum(c_P)) * rl, w = w * (1.0f / (1.0f + x)); skip
        Q unless w > 0; per channel sum = sum + c_Q * w; vs = vs + v_Q * (w * w); wsum = wsum + w.
     4. if wsum > 0 the new colour is sum / wsum (three divisions) and the new variance vs / (wsum *
        wsum), else both are kept.
   The last pass's state is `out` and `variance_out`.
   Asynchronous on `stream`; atr_render_wait covers it (tiles_done 0), atr_last_kernel_ms times it. No
   scene is needed. The passes run in a grow-only workspace of their own, apart from atr_denoise's (the
   two calls on two streams share nothing): 48 B per pixel, and 16 B more for each of normal and
   position that is given; a call on another stream than the last first waits for it on the GPU.
   ATR_E_INVALID, with nothing enqueued or written: ctx, params, color or variance NULL; out and
   framebuffer both NULL; exactly one of moments and length given; width or height outside 1..16,384;
   passes outside 1..8; normal_power_log2 outside 0..7; spatial_below outside 0..2^24; sigma_luminance
   or sigma_position negative, NaN or infinite; luminance_floor not finite or not > 0; non-zero
   reserved; a position term that is on whose kp is, in any of the passes, not finite and > 0.
   atr_denoise_variance_check is that validation alone (without ctx), on the host, with no context and
   no device: ATR_OK or ATR_E_INVALID. No struct and no ABI version change. */
typedef struct {
    int32_t passes;             /* 1..8; pass p (from 0) has tap spacing s = 2^p */
    float   sigma_luminance;    /* >= 0, finite; 0: luminance term off */
    float   luminance_floor;    /* > 0, finite: added to sigma_luminance * sd */
    float   sigma_position;     /* as atr_denoise; ignored when position == NULL */
    int32_t normal_power_log2;  /* 0..7, as atr_denoise */
    int32_t spatial_below;      /* 0..2^24: histories shorter than this take the spatial estimate; 0: none do */
    int32_t reserved[2];        /* must be 0 */
} atr_denoise_variance_params;
void atr_default_denoise_variance_params(atr_denoise_variance_params* out);   /* 3, 8.0f, 1e-4f, 0.0f, 5, 4, zeros */
int atr_denoise_variance_check(const float* color, const float* variance, const atr_denoise_guides* guides,
                               const float* moments, const uint32_t* length, int32_t width, int32_t height,
                               const atr_denoise_variance_params* params, const float* out,
                               const float* variance_out, const uint32_t* framebuffer);
int atr_denoise_variance(atr_ctx* ctx, const float* color, const float* variance,
                         const atr_denoise_guides* guides, const float* moments, const uint32_t* length,
                         int32_t width, int32_t height, const atr_denoise_variance_params* params,
                         float* out, float* variance_out, uint32_t* framebuffer, void* stream);

/* ---------------------------------------------------------------- a camera's rays and guides
   The primary ray of pixel (x, y) of a camera, as atr_render_start_ex casts it without anti-aliasing
   (every step a separately rounded f32 operation):
     film_y = -1 + 2 * (y / height);  film_x = ((-1 + 2 * (x / width)) * h_fov) * aspect_ratio;
     origin = eye;  direction = unit((frame_center + camera_x * film_x) + camera_y * film_y - eye).
   It goes through the pixel's centre whatever cam->anti_aliasing says; samples_per_pixel and
   bounce_limit are not read. A camera is accepted when width and height are 1..65,536 and every float
   field is finite (ATR_E_INVALID otherwise, checked on the host before anything is enqueued).

   atr_camera_rays_host: the rays of pixels first_pixel .. first_pixel + npixels - 1 in pixel order
   (pixel p = (p % width, p / width)), 3 floats each, into HOST arrays; no context. atr_camera_rays: the
   same bits into DEVICE arrays, asynchronous on `stream`; ready-made input for atr_trace_rays and
   atr_radiance_rays (ray_base = first_pixel re-renders that range of pixels). ATR_E_INVALID for a
   range outside [0, width * height] or NULL outputs with npixels > 0; npixels == 0 is ATR_OK. */
int atr_camera_rays_host(const atr_camera* cam, int64_t first_pixel, int64_t npixels, float* origins,
                         float* directions);
int atr_camera_rays(atr_ctx* ctx, const atr_camera* cam, int64_t first_pixel, int64_t npixels,
                    float* origins, float* directions, void* stream);

/* atr_camera_guides: the guides atr_denoise, atr_accumulate and atr_denoise_variance read, for the
   pixels of `tiles` (inclusive rects inside the image; a pixel in overlapping tiles is done once;
   pixels outside them are not written), in one kernel: the pixel's ray above is tested as
   atr_trace_rays tests a caller's ray (a failing ray is not traced: kind ATR_RAY_INVALID), traced to
   atr_trace_rays' closest hit, and
     depth    = that hit's t (3.402823466e38: none);   material = its material (0: sky, invalid);
     position = eye + direction * t (a multiply, then an add, each rounded; with the t above on sky
                and invalid pixels);
     normal   = the hit's unit normal n, negated where (-d.x * n.x + -d.y * n.y) + -d.z * n.z < 0 (the
                bounce's convention); +0, 0, 0 on sky and invalid pixels;
     ident    = ATR_DENOISE_EMPTY on sky and invalid pixels, else (kind << 28) | (model + 1) with
                atr_trace_rays' kind and model (model + 1 = 0 for a sphere or a plane).
   Every value equals, bit for bit, what atr_trace_rays on atr_camera_rays' rays followed by that
   arithmetic gives. Asynchronous on `stream`; atr_render_wait covers it (tiles_done 0,
   ATR_E_TREE_DEPTH as for a render) and atr_last_kernel_ms times it; no workspace. ATR_E_INVALID: ctx,
   cam or out NULL, all five outputs NULL, ntiles <= 0 or tiles NULL, a tile outside the image or
   empty, a camera that is not accepted (above). ATR_E_NOSCENE before atr_scene_upload. */
typedef struct {            /* DEVICE pointers, IMAGE layout (pixel (x,y) at y*width + x); any may be NULL */
    float*    normal;       /* 3 per pixel */
    float*    position;     /* 3 per pixel */
    uint32_t* ident;
    float*    depth;
    int32_t*  material;
} atr_guides_out;
int atr_camera_guides(atr_ctx* ctx, const atr_camera* cam, const atr_tile* tiles, int32_t ntiles,
                      const atr_guides_out* out, void* stream);

/* wait_for_render_from_camera_to_finish: 1 = still running after timeout_ms, 0 = done,
   <0 = error. tiles_done (optional) = tiles of the last render known complete (progress). */
int atr_render_wait(atr_ctx* ctx, uint32_t timeout_ms, int32_t* tiles_done);

/* Device-time of the last render's trace kernel(s) in milliseconds (HIP events recorded on the
   launch stream around the kernel). Valid after atr_render_wait returned 0. */
int atr_last_kernel_ms(atr_ctx* ctx, float* ms);

/* device memory helpers for C callers without a framework */
int atr_device_alloc(atr_ctx* ctx, size_t bytes, void** dptr);
int atr_device_free(atr_ctx* ctx, void* dptr);
int atr_memcpy_d2h(atr_ctx* ctx, void* dst, const void* src, size_t bytes);
int atr_memcpy_h2d(atr_ctx* ctx, void* dptr, const void* src, size_t bytes);
int atr_memset_d(atr_ctx* ctx, void* dptr, int value, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif
