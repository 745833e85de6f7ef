// engine.h -- internal types shared by the host side (scene prep, C-ABI) and the HIP kernels.
// Everything here is plain data; f32 helpers are __host__ __device__ so host-side
// precomputation and the kernels evaluate the same expressions in the same order
// (reference op order: PL/PL_math.h:106-123,416-422). Built with -ffp-contract=off.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/atray.h"

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define ATR_HD __host__ __device__ __forceinline__
#else
#define ATR_HD inline
#endif

namespace atr {

struct alignas(16) float4_t { float x, y, z, w; };
struct alignas(16) uint4_t { uint32_t x, y, z, w; };
struct alignas(8) float2_t { float x, y; };
struct alignas(8) uint2_t { uint32_t x, y; };

constexpr float kMaxFloat = 3.402823466e+38F;     // PL_base_defs.h:72
constexpr float kInvU32Max = 2.328306437e-10F;    // PL_base_defs.h:75
constexpr float kTol = 0.0001f;                   // ray.h:5
constexpr int kMaskLevels = 16;                   // traversal mask-stack depth (8 bits/level)
constexpr int kMaxMaterials = 32;
#ifndef ATR_MAX_FRAME_CAMS  // experiment builds: more cameras per launch (kernel argument size)
#define ATR_MAX_FRAME_CAMS 24
#endif
constexpr int kMaxFrameCams = ATR_MAX_FRAME_CAMS;  // distinct cameras per multi-frame launch (kernel argument)
constexpr int kMaxModels = 8;
// Primitive slots per leaf cluster (atr_tuning.cluster_size <= this) and 16-B words per cluster
// block (one 128-B line: record (2), screen normals (6)). 32 slots in 256-B blocks measured slower
// (DESIGN.md §4b); the layout code is written for either.
constexpr int kMaxClusterSize = 16;
constexpr int kClusterBlock = 8;
constexpr int kNormWords = kMaxClusterSize + kMaxClusterSize / 2;  // u32 screen-normal words per cluster

struct V3 { float x, y, z; };
ATR_HD V3 mk(float x, float y, float z) { V3 r; r.x = x; r.y = y; r.z = z; return r; }
ATR_HD V3 add(V3 a, V3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
ATR_HD V3 sub(V3 a, V3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
ATR_HD V3 neg(V3 a) { return mk(-a.x, -a.y, -a.z); }
ATR_HD V3 scale(V3 a, float s) { return mk(a.x * s, a.y * s, a.z * s); }
ATR_HD V3 divs(V3 a, float s) { return mk(a.x / s, a.y / s, a.z / s); }
ATR_HD V3 had(V3 a, V3 b) { return mk(a.x * b.x, a.y * b.y, a.z * b.z); }
ATR_HD float dot(V3 a, V3 b) { return (a.x * b.x) + (a.y * b.y) + (a.z * b.z); }
ATR_HD V3 cross(V3 a, V3 b) { return mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
ATR_HD float len2(V3 v) { return (v.x * v.x) + (v.y * v.y) + (v.z * v.z); }
// normalize (PL_math.h:387-392). SVML _mm_invsqrt_ps is declared as 1/sqrtf.
ATR_HD V3 unit(V3 v) { float inv = 1.0f / sqrtf(len2(v)); return scale(v, inv); }
ATR_HD V3 lerp3(V3 s, V3 t, float k) { return add(scale(sub(t, s), k), s); }
ATR_HD float pl_max(float a, float b) { return a > b ? a : b; }
ATR_HD float pl_min(float a, float b) { return a > b ? b : a; }
ATR_HD V3 from(atr_vec3 v) { return mk(v.x, v.y, v.z); }

// PCG-XSH-RR (PL_math.h:506-516)
ATR_HD uint32_t pcg_next(uint64_t& state, uint64_t stream) {
    uint64_t old = state;
    state = old * 6364136223846793005ULL + (stream | 1ULL);
    uint32_t xs = (uint32_t)(((old >> 18u) ^ old) >> 27u);
    uint32_t rot = (uint32_t)(old >> 59u);
    return (xs >> rot) | (xs << ((0u - rot) & 31u));
}
ATR_HD float rand_bi(uint64_t& state, uint64_t stream) {  // PL_math.h:525-541
    float rd = (float)pcg_next(state, stream) * kInvU32Max;
    return -1.0f + 2.0f * rd;
}
// One PCG stream per (pixel, sample) (deviation from renderer.cpp:376-378's rdtsc*thread seeding,
// DESIGN.md §2): state = splitmix64(seed ^ pixel ^ sample << 40), increment 2 pixel + 1. A pixel's
// samples are independent paths, so they can run in parallel (paths.hip); sample 0's stream is the
// round-1..3 per-pixel stream.
ATR_HD void path_stream(uint64_t seed, int64_t pixel, uint32_t sample, uint64_t& state, uint64_t& stream) {
    uint64_t x = seed ^ (uint64_t)pixel ^ ((uint64_t)sample << 40);
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    state = x ^ (x >> 31);
    stream = ((uint64_t)pixel << 1) | 1ULL;
}

// ---------------------------------------------------------------- device scene layout
// Octree node, 32 B: two float4 loads. children = children_start_position (0 = leaf),
// parent = index of the parent node (-1 for the root), used by the stackless DFS.
struct alignas(16) DNode {
    float lo_x, lo_y, lo_z, hi_x;
    float hi_y, hi_z;
    int32_t children;
    int32_t parent;
};
static_assert(sizeof(DNode) == 32, "DNode layout");

// Leaf primitive / brute-force triangle, 48 B: a, ab = b - a, ac = c - a (the first two
// subtractions of model.h:77-78, done once on the host: same IEEE f32 results), face index.
struct alignas(16) DTri {
    float ax, ay, az, abx;
    float aby, abz, acx, acy;
    float acz;
    uint32_t face;
    float pad0, pad1;
};
static_assert(sizeof(DTri) == 48, "DTri layout");

// Per-model device view. has_tree == 0 selects the brute-force branch (renderer.cpp:58-82).
struct DModel {
    const DNode* nodes;          // octree nodes in reference order (root = 0)
    // inner nodes only: 3 float4 = {lo.xyz, v.x}{v.yz, hi.xy}{hi.z, bits(first
    // child node), bits(parent inner id), bits((inner id of first inner child << 8) | leaf mask)};
    // the children boxes are derived from lo, v, hi (kd_tree.cpp:116-148)
    const float4_t* inner;
    int32_t ninner;
    const uint32_t* leaf_range;  // 2 u32 per node: first DTri, count (leaves only)
    const DTri* tris;            // leaf-ordered primitives (tree) or face-ordered (brute force)
    // the same primitives as SoA streams for per-lane loads: t0 = {a.xyz, ab.x},
    // t1 = {ab.yz, ac.xy}, t2 = ac.z (36 B per test); tface read only for the final hit
    const float4_t* t0;
    const float4_t* t1;
    const float* t2;
    const uint32_t* tface;
    // leaf clusters, 2 float4 per cluster: {lo.xyz, bound of |ab||ac| with
    // (n - 1) in its low 5 mantissa bits}, {hi.xyz, q}; cl_range = first cluster, count per
    // node. Cluster c owns the primitive slots [16 c, 16 c + n) and the 128-B block clus[8 c ..]:
    // its record (2 words), then (cnrm = clus + 2) 6 words of its screen normals
    // n = ab x ac as f16 integer multiples of q (the screen, cluster.h); prim = 48 B per slot:
    // {a.xyz, ab.x}{ab.yz, ac.xy}{ac.z, bits(leaf rank), bits(face index), 0}
    const float4_t* clus;
    const uint32_t* cl_range;
    const uint4_t* cnrm;
    const float4_t* prim;
    const float* shade;          // 9 f32 per face: smooth -> na, nb, nc; flat -> v0, v1, v2
    uint32_t nfaces;
    int32_t has_tree;
    int32_t root_leaf;           // root never split (kd_tree.cpp:344-361)
    int32_t near_ok;             // depth <= 8 and < 2^16 inner nodes: near-first passes (trace.h)
    int32_t smooth;              // normals.size > 0 (renderer.cpp:129)
    int32_t material;
    float aabb[6];               // Model::surrounding_aabb
    // the model's clusters in the scene-wide cluster numbering (the tree models' clusters in model
    // order): the index of the per-camera table of box growths (RenderParams::pads)
    uint32_t cl_base, cl_count;
    // and its leaves (discovery ranks, what cl_range is indexed by) in the scene-wide leaf numbering:
    // the index of the per-camera table of leaf boxes (RenderParams::lbox)
    uint32_t lf_base, lf_count;
};

struct DMaterial { float ex, ey, ez, rx, ry, rz, scatter, pad; };
struct DSphere { float cx, cy, cz, r; int32_t material, pad0, pad1, pad2; };
struct DPlane { float nx, ny, nz, d; int32_t material, pad0, pad1, pad2; };

// Scene-wide device data, uploaded once by atr_scene_upload (read via scalar loads).
struct DScene {
    DMaterial mats[kMaxMaterials];
    DModel models[kMaxModels];
    int32_t nmats, nmodels, nspheres, nplanes;
    const DSphere* spheres;
    const DPlane* planes;
};

// A work block: one wavefront, an 8x8 pixel cell at (x0, y0); lane l -> (x0 + (l & 7),
// y0 + (l >> 3)); only lanes whose bit is set in `mask` own a pixel of the render.
struct alignas(16) DBlock {
    int32_t x0, y0;
    uint32_t mask_lo, mask_hi;
    int32_t out_base;  // PACKED layout: output slot of the block's first owned pixel
    int32_t flags;     // kBlockPrio: the wave raises its issue priority (cell plan, atr_set_cell_plan)
    int32_t base;      // index of the block in its tile list's base block list (per-block cost slot)
    int32_t pad;
};
static_assert(sizeof(DBlock) == 32, "DBlock layout");
constexpr int32_t kBlockPrio = 1;
// cell plan byte (atr_set_cell_plan): low nibble = waves per cell (0/1, 2, 4, 8); bits 4-6 = the
// cell's dispatch class (blocks of class 7 lead the block list, then 6, ..., 0; Morton order within
// a class; their packed slots do not move); kPlanPrio = its waves issue at raised priority
constexpr int kPlanClassShift = 4;
constexpr uint8_t kPlanClassMask = 0x70, kPlanPrio = 0x80;

// What a ray that passes no model's first test gets, and those tests' operands, as the kernels load
// them (capi.cpp atr_scene_upload): box i = the six floats model i's query starts with -- a tree
// model's nodes[0] bounds for box_check (scan.h flat_begin), a brute-force model's aabb for box_entry
// (scan.h intersect_models; bit i of `brute`), lo.xyz then hi.xyz -- and the record scene_finish
// (shade.h) leaves for no model hit in a scene without spheres and planes: the emission of material
// 0, face, t. on: the path is usable (n <= kSkyBoxes models, no sphere, no plane, not switched off).
constexpr int kSkyBoxes = 4;
constexpr uint32_t kSkyFace = 0xFFFFFFFFu;  // shade.h scene_finish: id.face of a hit that is no triangle
struct SkyRecord {
    int32_t on;
    int32_t n;
    uint32_t brute;
    uint32_t face;
    float t;
    float em[3];
    float box[kSkyBoxes][6];
};

// Per-render kernel argument (by value, no dynamic indexing into it).
struct RenderParams {
    atr_camera cam;
    const DScene* scene;
    uint64_t seed;
    const DBlock* blocks;
    int32_t nblocks;
    int32_t layout;
    uint32_t* framebuffer;
    uint32_t* hit_face;
    float* hit_t;
    float* rgb;
    uint32_t* ray_casts;
    // 64 traced-ray counters 128 B apart (a zeroed 8-KB slot of the context's ring, capi.cpp
    // launch_render); the kernel adds each wave's count to slot (block & 63). Never a caller's
    // single accumulator: atr_launch_render rejects it together with `counters`.
    unsigned long long* traced_rays;
    int32_t* error_flag;  // set to 1 if a ray hit a traversal limit (never for depth <= 16)
    unsigned long long* counters;  // non-null -> instrumented kernel (10 u64, see render.hip)
    unsigned long long* block_cost;  // non-null -> shader clocks added per base block (blocks[b].base)
    unsigned long long* wave_trace;  // non-null -> per block: start, end (100 MHz clock), HW_ID | XCC_ID << 32
    int32_t xcd_chunk;  // 0: contiguous block range per XCD; k > 0: k-workgroup chunks dealt round-robin
    int32_t frame_blocks;  // > 0: nblocks = frames x frame_blocks, one launch renders every frame
    int64_t frame_stride;  // output elements between consecutive frames (rgb: 3 x this)
    int32_t frame_rotate;  // frame f's blocks start f / frames x frame_rotate / 1024 into its list
    int32_t hyb_a, hyb_b;  // HYBRID: a step's leaves are dealt in rounds when max clusters > a x rounds + b
    int32_t nfcam;         // > 0: frame f renders with fcam[f] instead of cam (same size/spp/bounces)
    atr_camera fcam[kMaxFrameCams];
    // A sample pass (atr_render_start_samples): the launch renders samples first_sample ..
    // first_sample + cam.samples_per_pixel - 1 and continues the f32 sums kept in sample_sum (3 per
    // output slot, indexed as rgb). Last in the struct and read by the ACCUM kernels only, so every
    // other kernel's code is what it was without them.
    uint32_t first_sample;
    float* sample_sum;     // non-null -> an accumulating pass
    // The primary kernels' table of box growths (cluster.h cluster_grow): row f --
    // frame f's camera (row 0 alone without per-frame cameras) -- holds one {loose, tight} pair per
    // cluster of the scene, pads_stride pairs per row. Non-null selects the primary kernels that
    // read it; after the fields above, and read by those kernels only.
    const float2_t* pads;
    int32_t pads_stride;
    // The primary kernels' wave cull (scan.h flat_leaf_step WCULL): non-zero, a leaf's
    // clusters are tested against the wave's direction hull before the per-ray tests. Read by
    // HYBRID's primary kernels only; same output bits either way.
    int32_t wave_cull;
    // The primary table kernels' leaf boxes (cluster.h leaf_box): row f holds one
    // 32-byte entry {LO.xyz, bits(flag)}{HI.xyz, 0} per leaf of the scene (lbox_stride entries per
    // row), the bounds of the leaf's clusters grown by the row's own loose growths. Non-null (only
    // with pads), a lane's pass leaves out the leaves whose box its ray misses. Last in the struct and
    // read by the kernels that read pads only; same output bits either way.
    const float4_t* lbox;
    int32_t lbox_stride;
    // HYBRID's primary kernels' sky path (render.hip): the scene's record of every
    // model's first test (SkyRecord below, filled at upload), by value. sky.on != 0: a wave none of
    // whose active lanes passes any of the sky.n tests writes the sky's outputs from this record and
    // reads nothing of the scene. Last in the struct and read by those kernels only; same output bits
    // either way.
    SkyRecord sky;
};

// The eyes of a launch's cameras, by value, for the kernel that fills the table.
struct PadEyes {
    float e[kMaxFrameCams][3];
};

// Sample-parallel path engine (paths.hip): one lane per (pixel, sample) path. A batch
// is a contiguous range [cell0, cell0 + ncells) of the launch's cell list (frames interleaved as in
// RenderParams: cell c renders block c / nf of frame c % nf). The camera launch's wavefront w of
// the batch takes paths r = 64 w .. 64 w + 63 of cell w / spp (r -> pixel lane r / spp, sample
// r % spp: a pixel's samples side by side), so a wavefront lies in one cell. Path records between
// bounces are four float4 planes of `cap` entries each:
//   p0 = {o.xyz, d.x}, p1 = {d.y, d.z, bits(pixel), bits(g)}, p2 = {ret.xyz, w.x},
//   p3 = {w.y, w.z, bits(rng lo), bits(rng hi)};
// a finished path leaves {colour.xyz, bits(ray_casts)} in its result slot
// out[g], g = (c - cell0) x 64 spp + sample x 64 + pixel lane.
constexpr int kPathPlanes = 4;
// Per bounce level k of a batch (zeroed before the batch): the launch of level k (0 = the camera
// rays) appends its surviving paths to queue k & 1 (tail); the bounce launch k + 1 reads them,
// its persistent waves claiming 64 at a time (head of level k + 1).
struct PathCtl {
    uint32_t tail;
    uint32_t head;
};
// Queue sort (tuning path_sort_bits = b > 0): the queues are entry-major (an entry's
// four records together, q[4 e + i], 64 B) and every queued path also records {key, rank} in `kr`:
// key = the ray's coarse direction cell (4 x 4 of the 16 x 16 octahedral cells), a Morton code of
// its origin quantised to b bits per axis over the scene box (lo, sc = 2^b / extent), then its fine
// direction cell within the coarse one (paths.hip path_sort_key), rank = its arrival
// in the key's bin (atomicAdd on hist). The sort launches turn hist into bin starts and write the
// level's key order perm[start[key] + rank] = entry; the next bounce launch's waves claim positions
// of that order, so a wavefront takes rays of one direction cell and one region together (a
// counting sort of 4-B indices; the entries never move; the order within a bin is arrival order,
// and no output depends on queue order).
#ifndef ATR_SORT_DIRS
#define ATR_SORT_DIRS 16
#endif
constexpr int kSortDirs = ATR_SORT_DIRS;  // direction cells per side of the octahedral map
constexpr int kMaxSortBits = 7;
constexpr int64_t kSortBinsMax = int64_t(1) << 26;  // 256 direction cells x 6 bits per axis
constexpr int32_t kSortChunk = 4096;  // bins per block of the bin scan
static_assert((kSortDirs * kSortDirs << 6) % kSortChunk == 0, "the fewest bins (2 bits per axis) fill whole scan blocks");
static_assert((kSortBinsMax / kSortChunk) <= 32768, "path_sort_part_scan: one workgroup, 32 sums per lane");
struct PathSort {
    int32_t bits;      // 0: off
    int32_t nbins;     // kSortDirs^2 << 3 bits
    float lo[3], sc[3];
    uint2_t* kr;       // {key, rank} per entry of the level being written
    uint32_t* perm;    // the previous level's key order (entry per position)
    uint32_t* hist;    // nbins arrival counters (zero between levels)
    uint32_t* start;   // nbins bin starts
    uint32_t* part;    // nbins / kSortChunk block sums
};

// An adaptive sample pass (atr_render_start_adaptive): only the pixels still live --
// count[o] == first_sample with ATR_SAMPLES_CONVERGED clear, or every pixel when first_sample == 0 --
// are traced and resolved. Per batch the live-list kernels (paths.hip path_live_*) leave, for cell
// c of the batch, its live-pixel mask and the first of its camera path groups (a group = 64
// consecutive paths of one cell's live pixels, pixel-major: ceil(popcount(mask) x spp / 64) per
// cell, numbered in cell order), and for every group its cell. kLiveChunk cells form one block of
// the three-phase scan; part holds 3 u32 per chunk (groups, live pixels, live cells).
constexpr int32_t kLiveChunk = 64;
struct PathLiveCtl {
    uint32_t groups;  // camera path groups of the batch
    uint32_t claim;   // next group to hand out (persistent camera waves)
};
struct PathLive {
    uint32_t* count;    // the caller's sample_count (null: not an adaptive pass)
    float tolerance;
    uint2_t* mask;      // per cell of the batch: its live pixels
    uint32_t* first;    // per cell: its first group (path_live_build leaves the group count here)
    uint32_t* group;    // per group: its cell
    uint32_t* part;     // per chunk: groups (scanned in place), live pixels, live cells
    PathLiveCtl* ctl;
    // the pass's counts (atr_render_adaptive_info): pixels live at the start, live blocks, camera
    // path groups, pixels that converged in this pass
    unsigned long long* info;
};

struct PathParams {
    atr_camera cam;
    const DScene* scene;
    uint64_t seed;
    const DBlock* blocks;
    int32_t frame_blocks;  // blocks per frame (the launch's frames: nf = nblocks / frame_blocks)
    int32_t nblocks;       // cells of the launch (all frames)
    int32_t cell0, ncells; // this batch
    int32_t layout;
    int64_t frame_stride;
    uint32_t* framebuffer;
    uint32_t* hit_face;
    float* hit_t;
    float* rgb;
    uint32_t* ray_casts;
    unsigned long long* traced_rays;  // 64 spread counters (a ring slot), or null
    int32_t* error_flag;
    unsigned long long* block_cost;   // non-null -> shader clocks per base block (calibration)
    float4_t* q[2];   // path queues, kPathPlanes planes of cap entries each
    int64_t cap;      // entries per plane (>= the batch's paths)
    float4_t* out;    // per path: colour and ray_casts of the finished path
    PathCtl* ctl;     // one per bounce level
    unsigned long long* counters;  // non-null -> instrumented kernels (counters [0..9] of render.hip)
    int32_t bounce;   // bounce launch: this bounce (1 .. bounce_limit - 1)
    int32_t xcd_chunk;
    int32_t hyb_a, hyb_b;
    int32_t nfcam;
    PathSort sort;
    atr_camera fcam[kMaxFrameCams];
    uint32_t first_sample;  // a sample pass (RenderParams): read by the ACCUM camera kernel and
    float* sample_sum;      // path_resolve_accum_kernel only
    PathLive live;          // an adaptive pass: read by the path_live_* and *_adaptive kernels only
};

// A ray query (atr_trace_rays, query.hip): n caller rays, 3 floats each, traced by
// persistent waves that claim 64 positions at a time on `head`; with sort.bits > 0 position i of
// the batch is ray sort.perm[i] (the batch in PathSort key order), else ray i. Every output is
// written at the ray's input index; a null output is not written.
struct QueryParams {
    const DScene* scene;
    const float* o;
    const float* d;
    uint32_t n;
    int32_t hyb_a, hyb_b;
    float* t;
    uint32_t* face;
    int32_t* model;
    float* uv;
    int32_t* kind;
    int32_t* material;
    float* normal;
    unsigned long long* traced_rays;  // 64 spread counters (a ring slot), or null
    int32_t* error_flag;
    uint32_t* head;  // zeroed before the launch
    PathSort sort;
};

// An occlusion query (atr_occluded_rays, occlusion.hip): the batch, its claim counter
// and its key order as in QueryParams (the order is made by the ray query's own sort kernels, in the
// same workspace); tmax one float per ray or null (every ray unbounded); out one byte per ray at its
// input index (ATR_OCCL_*).
struct OcclParams {
    const DScene* scene;
    const float* o;
    const float* d;
    const float* tmax;
    uint32_t n;
    uint8_t* out;
    unsigned long long* traced_rays;  // 64 spread counters (a ring slot), or null
    int32_t* error_flag;
    uint32_t* head;        // zeroed before the launch
    const uint32_t* perm;  // sorted launches: position -> ray
};

// A hemisphere gather (atr_gather_occlusion, gather.hip): npoints surface points with
// unit normals, nsamples directions each, drawn in the kernel (gather_dir below); item i * nsamples + s
// of the flattened batch is sample first_sample + s of point point_base + i. Persistent waves claim
// 64 items at a time on `head`. visible, occluded and mask (words per point) are zeroed before the
// launch and added / ORed to; a null output is not written.
struct GatherParams {
    const DScene* scene;
    const float* p;        // 3 per point
    const float* nrm;      // 3 per point
    const float* tmax;     // one per point, or null
    uint32_t n;            // npoints x nsamples (< 2^31)
    uint32_t nsamples;
    uint32_t first_sample;
    uint32_t words;        // mask words per point: ceil(nsamples / 32)
    int64_t point_base;
    uint64_t seed;
    uint32_t* visible;
    uint32_t* occluded;
    uint32_t* mask;
    float* dirs;           // 3 per item
    unsigned long long* traced_rays;  // 64 spread counters (a ring slot), or null
    int32_t* error_flag;
    uint32_t* head;        // zeroed before the launch
};

// A radiance query (atr_radiance_rays, radiance.hip): one batch of the call's rays,
// [ray0, ray0 + n) of the arrays o and d, ray0 a multiple of 64. A group is 64 consecutive rays (the
// path engine's "cell"); the entry kernel's persistent waves claim groups on ctl[0].head (zeroed with
// the batch's control words; the bounce launches use the heads of levels >= 1 only), trace each
// first segment once and seed queue 0 with the samples that go on; sample s of the batch's ray i has
// the result slot (i / 64) x 64 nsamples + s x 64 + i % 64 and the stream of (seed, ray_base + ray0
// + i, first_sample + s). The bounce levels are the path engine's own launches on a PathParams; the
// resolve reads the slots and writes the outputs at the rays' input indices (a null one is not written).
constexpr uint32_t kRayInvalid = 0xFFFFFFFEu;  // sample 0's slot of a ray that failed the validity test
struct RadianceParams {
    const DScene* scene;
    const float* o;
    const float* d;
    uint32_t ray0, n;
    uint32_t nsamples, first_sample;
    int32_t bounce_limit;
    int32_t hyb_a, hyb_b;
    int64_t ray_base;
    uint64_t seed;
    float4_t* q0;     // queue 0 of the workspace (PathParams::q[0])
    int64_t cap;
    float4_t* out;    // the result slots (PathParams::out)
    PathCtl* ctl;
    PathSort sort;
    unsigned long long* traced_rays;  // 64 spread counters (a ring slot), or null
    int32_t* error_flag;
    float* rgb;
    float* sum;
    uint32_t* ray_casts;
    uint8_t* invalid;
};

// A hemisphere radiance gather (atr_gather_radiance, gather_radiance.hip): one batch of
// the call's points, [point0, point0 + npoints) of the arrays p and nrm, nsamples samples each. Item
// i * nsamples + s of the flattened batch is sample first_sample + s of point point_base + point0 + i
// and owns result slot i * nsamples + s: a point's samples are contiguous, so the resolve reads 64 of
// them as one 1-KB row. The entry kernel's persistent waves claim 64 items at a time on ctl[0].head,
// draw the direction on the item's stream (gather_dir_state below), trace it and either finish the
// path in its slot or append it to queue 0 with the stream as the draws left it; the bounce levels
// are the path engine's own launches on a PathParams. Every item's slot is written exactly once: a
// finished path's {colour, casts}, kSampleUntraced for a sample of a valid point that is not traced,
// kRayInvalid for every item of an invalid point. The resolve (a wave per point) adds the traced
// samples' colours in sample order and writes the outputs at the points' input indices (a null one
// is not written).
constexpr uint32_t kSampleUntraced = 0xFFFFFFFDu;  // beside kAllSky and kRayInvalid, above any real count
struct GatherRadianceParams {
    const DScene* scene;
    const float* p;        // 3 per point of the call
    const float* nrm;      // 3 per point of the call
    uint32_t point0, npoints;
    uint32_t n;            // npoints x nsamples (< 2^31)
    uint32_t nsamples, first_sample;
    int32_t bounce_limit;
    int32_t hyb_a, hyb_b;
    int64_t point_base;
    uint64_t seed;
    float4_t* q0;     // queue 0 of the workspace (PathParams::q[0])
    int64_t cap;
    float4_t* out;    // the result slots (PathParams::out)
    PathCtl* ctl;
    PathSort sort;
    unsigned long long* traced_rays;  // 64 spread counters (a ring slot), or null
    int32_t* error_flag;
    float* rgb;
    float* sum;
    uint32_t* samples;
    uint32_t* ray_casts;
    uint8_t* invalid;
    float* sample_rgb;     // 3 per item of the call
    float* dirs;           // 3 per item of the call
};

// Sample `sample` of point `point` around the unit normal n: bounce_shade's diffuse direction (scan.h)
// on the (pixel, sample) stream of path_stream. A zero sum gives NaN, which ray_ok rejects.
ATR_HD V3 gather_dir(uint64_t seed, int64_t point, uint32_t sample, V3 n) {
    uint64_t st, stream;
    path_stream(seed, point, sample, st, stream);
    const float r0 = rand_bi(st, stream);
    const float r1 = rand_bi(st, stream);
    const float r2 = rand_bi(st, stream);
    return unit(add(mk(r0, r1, r2), n));
}

// gather_dir that also hands back the stream after its three draws, for a path that continues on it
// (atr_gather_radiance): the same draws and the same f32 operations, so the same direction bits.
ATR_HD V3 gather_dir_state(uint64_t seed, int64_t point, uint32_t sample, V3 n, uint64_t& st, uint64_t& stream) {
    path_stream(seed, point, sample, st, stream);
    const float r0 = rand_bi(st, stream);
    const float r1 = rand_bi(st, stream);
    const float r2 = rand_bi(st, stream);
    return unit(add(mk(r0, r1, r2), n));
}

// A light-probe batch (atr_probe_sh, probe_sh.hip): GatherRadianceParams without the
// normals and with 27 sums per probe. [point0, point0 + npoints) of the array p, nsamples samples each;
// item i * nsamples + s is sample first_sample + s of probe point_base + point0 + i and owns result
// slot i * nsamples + s. The entry kernel draws the direction over the whole sphere on the item's
// stream (probe_dir_state below), traces it and finishes the path in its slot or appends it to queue
// 0; every sample of a valid probe is traced, so a slot holds a finished path's {colour, casts} or,
// for every item of an invalid probe, kRayInvalid. The resolve (a wave per probe) draws each slot's
// direction again, evaluates the nine basis functions on it (sh_basis) and adds colour x basis in
// sample order into the 27 sums (index 3 k + c); a null output is not written.
struct ProbeShParams {
    const DScene* scene;
    const float* p;        // 3 per probe of the call
    uint32_t point0, npoints;
    uint32_t n;            // npoints x nsamples (< 2^31)
    uint32_t nsamples, first_sample;
    int32_t bounce_limit;
    int32_t hyb_a, hyb_b;
    int64_t point_base;
    uint64_t seed;
    float4_t* q0;     // queue 0 of the workspace (PathParams::q[0])
    int64_t cap;
    float4_t* out;    // the result slots (PathParams::out)
    PathCtl* ctl;
    PathSort sort;
    unsigned long long* traced_rays;  // 64 spread counters (a ring slot), or null
    int32_t* error_flag;
    float* sh;             // 27 per probe
    float* sum;            // 27 per probe
    uint32_t* ray_casts;
    uint8_t* invalid;
    float* sample_rgb;     // 3 per item of the call
    float* dirs;           // 3 per item of the call
};

// Sample `sample` of probe `point`: a direction uniform over the sphere, on the (pixel, sample) stream
// of path_stream, by rejection inside the radial shell 2^-10 <= |v|^2 <= 1 of the cube's draws -- no
// sine or cosine, so the host and the device make the same bits. At most kProbeTries tries of three
// rand_bi draws each; the first one inside the shell is normalised as unit() does. If none is (about
// 1e-10 per sample), the direction is +z: the loop has a fixed end on every lane. The stream comes
// back as the draws left it. `tries` = the accepted try, 1-based, or kProbeTries + 1. No operation in
// the loop crosses lanes, so lanes of a wave may leave it at different trips.
constexpr int kProbeTries = 32;
constexpr float kProbeLen2Min = 0.0009765625f;  // 0x1p-10f
ATR_HD V3 probe_dir_state(uint64_t seed, int64_t point, uint32_t sample, uint64_t& st, uint64_t& stream,
                          uint32_t& tries) {
    path_stream(seed, point, sample, st, stream);
    for (int t = 1; t <= kProbeTries; ++t) {
        const float r0 = rand_bi(st, stream);
        const float r1 = rand_bi(st, stream);
        const float r2 = rand_bi(st, stream);
        const float l2 = (r0 * r0 + r1 * r1) + r2 * r2;
        if (kProbeLen2Min <= l2 && l2 <= 1.0f) {
            tries = uint32_t(t);
            return scale(mk(r0, r1, r2), 1.0f / sqrtf(l2));
        }
    }
    tries = uint32_t(kProbeTries) + 1u;
    return mk(0.f, 0.f, 1.f);
}

// The nine real spherical harmonics of bands 0..2 on a unit direction (atray.h atr_probe_sh), each
// product separately rounded in this order.
ATR_HD void sh_basis(V3 d, float y[9]) {
    y[0] = 0.282094792f;
    y[1] = 0.488602512f * d.y;
    y[2] = 0.488602512f * d.z;
    y[3] = 0.488602512f * d.x;
    y[4] = 1.092548431f * (d.x * d.y);
    y[5] = 1.092548431f * (d.y * d.z);
    y[6] = 0.315391565f * ((3.0f * (d.z * d.z)) - 1.0f);
    y[7] = 1.092548431f * (d.x * d.z);
    y[8] = 0.546274215f * ((d.x * d.x) - (d.y * d.y));
}

// The validity test of a caller's ray (atray.h atr_trace_rays): six finite inputs and a direction
// normalised to within 2^-20 in len2 (what unit() leaves is within 6 x 2^-24). The comparisons are
// false for a NaN, and an infinite component fails the first one.
constexpr float kRayLen2Tol = 9.5367431640625e-07f;  // 0x1p-20f
ATR_HD bool ray_ok(V3 o, V3 d) {
    const bool fin = fabsf(o.x) <= kMaxFloat && fabsf(o.y) <= kMaxFloat && fabsf(o.z) <= kMaxFloat &&
                     fabsf(d.x) <= kMaxFloat && fabsf(d.y) <= kMaxFloat && fabsf(d.z) <= kMaxFloat;
    return fin && fabsf(len2(d) - 1.0f) <= kRayLen2Tol;
}

// The validity test of a gather's point (atray.h atr_gather_occlusion): a finite point and a unit
// normal (the ray test), and a t_max that is positive or +inf, tested on its bits (NaN, zero and
// negative values fail, whatever the denormal mode).
ATR_HD bool gather_point_ok(V3 p, V3 n, float tm) {
    int32_t tb;
    __builtin_memcpy(&tb, &tm, sizeof(tb));
    return ray_ok(p, n) && tb > 0 && tb <= 0x7F800000;
}

}  // namespace atr
