// capi.cpp -- the extern "C" boundary of include/atray.h: scene flattening + upload, render
// launches on a HIP stream, progress/wait, and the host prerequisites behind opaque handles.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <fcntl.h>
#include <unistd.h>
#include <cerrno>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "engine.h"
#include "host_scene.h"
#include "launch.h"
#ifdef ATR_DIAG
#include "../../include/atray_diag.h"
#endif

using namespace atr;

#define HIPCHK(x)                                      \
    do {                                               \
        hipError_t e_ = (x);                           \
        if (e_ != hipSuccess) return -(1000 + int(e_)); \
    } while (0)

namespace {

struct DevBuf {
    void* p = nullptr;
    size_t n = 0;
};

// Blocks for one tile list: the 8x8 cells covering the union of the (inclusive) tile rects,
// each pixel owned exactly once (the reference traces the 1-px overlaps twice, renderer.cpp:429-442).
struct BlockSet {
    std::vector<atr_tile> tiles;
    int32_t width = 0, height = 0;
    std::vector<DBlock> host;
    DevBuf dev;
    DevBuf dev_tiles;
    uint32_t cplan_gen = 0;  // the ctx's cell plan this set was built with
    DevBuf dev_tile;  // owning tile per packed slot (atr_packed_tile_ray_casts; built on first use)
    bool tile_ready = false;
    int64_t packed_pixels = 0;
    // single-frame plan (plan.hip), double-buffered: launch n (parity n & 1) renders from the list
    // planned on the costs of launch n - 2 and writes its per-base-block clocks into its parity's
    // cost half; the plan kernels then run on the context's plan stream, after the render and
    // beside launch n + 1, and rebuild that parity's list from them (plan_ev[parity] after them)
    DevBuf cost, cost_last, plan_work, plan_blocks;
    int32_t max_split = 0;
    bool plan_ready = false;   // a plan was issued on this set (the buffers hold plan state)
    bool plan_valid[2] = {};   // a list is built (or being built) in that parity's half
    hipEvent_t plan_ev[2] = {};
    int plan_par = 0;          // the parity of the next planned launch
    hipStream_t plan_stream = nullptr;
};

// Device scratch freed on every exit path.
struct DevTmp {
    void* p = nullptr;
    ~DevTmp() { if (p) (void)hipFree(p); }
};

uint64_t morton2(uint32_t x, uint32_t y) {
    uint64_t r = 0;
    for (int i = 0; i < 16; ++i) r |= (uint64_t((x >> i) & 1u) << (2 * i)) | (uint64_t((y >> i) & 1u) << (2 * i + 1));
    return r;
}

// first_emit > 0: the pixels of tiles[0, first_emit) are left out (they belong to an earlier
// launch of a progressive render) and only tiles[first_emit, ntiles) emit blocks.
void build_blocks(const atr_tile* tiles, int32_t ntiles, int32_t W, int32_t H, std::vector<DBlock>& out,
                  int64_t& npix, int32_t first_emit = 0, const uint8_t* cplan = nullptr) {
    const int32_t cw = (W + 7) / 8, ch = (H + 7) / 8;
    std::vector<uint64_t> cell(size_t(cw) * size_t(ch), 0), done(first_emit > 0 ? cell.size() : 0, 0);
    // tile order decides the block order: cells are emitted tile by tile (first owner wins)
    std::vector<int32_t> order;
    order.reserve(cell.size());
    std::vector<uint8_t> seen(cell.size(), 0);
    std::vector<int32_t> fresh;
    for (int32_t k = 0; k < ntiles; ++k) {
        atr_tile t = tiles[k];
        fresh.clear();
        if (t.min_x < 0) t.min_x = 0;
        if (t.min_y < 0) t.min_y = 0;
        if (t.max_x > W - 1) t.max_x = W - 1;
        if (t.max_y > H - 1) t.max_y = H - 1;
        if (t.max_x < t.min_x || t.max_y < t.min_y) continue;
        for (int32_t cy = t.min_y / 8; cy <= t.max_y / 8; ++cy)
            for (int32_t cx = t.min_x / 8; cx <= t.max_x / 8; ++cx) {
                const size_t ci = size_t(cy) * size_t(cw) + size_t(cx);
                uint64_t m = 0;
                for (int32_t ly = 0; ly < 8; ++ly) {
                    const int32_t y = cy * 8 + ly;
                    if (y < t.min_y || y > t.max_y) continue;
                    for (int32_t lx = 0; lx < 8; ++lx) {
                        const int32_t x = cx * 8 + lx;
                        if (x >= t.min_x && x <= t.max_x) m |= uint64_t(1) << (ly * 8 + lx);
                    }
                }
                if (k < first_emit) { done[ci] |= m; continue; }
                if (first_emit > 0) m &= ~done[ci];
                if (!m) continue;
                if (!seen[ci]) { seen[ci] = 1; fresh.push_back(int32_t(ci)); }
                cell[ci] |= m;
            }
        // the tile's cells along a Z curve (Morton order): consecutive waves trace a 2D patch and
        // share its leaves in their XCD's L2
        std::stable_sort(fresh.begin(), fresh.end(), [cw](int32_t a, int32_t b) {
                return morton2(uint32_t(a % cw), uint32_t(a / cw)) < morton2(uint32_t(b % cw), uint32_t(b / cw));
            });
        order.insert(order.end(), fresh.begin(), fresh.end());
    }
    out.clear();
    out.reserve(order.size());
    npix = 0;
    bool classes = false;  // some cell has a dispatch class: blocks are reordered after the loop
    for (int32_t ci : order) {
        // cell plan (atr_set_cell_plan): a heavy cell is split into `parts` row bands, one wave
        // each, emitted back to back in lane order (the packed slot order does not change)
        const uint8_t pl = cplan ? cplan[ci] : 0;
        const int parts = (pl & 0xF) >= 2 ? (pl & 0xF) : 1;
        const uint64_t cm = cell[size_t(ci)];
        for (int k = 0; k < parts; ++k) {
            const int rows = 8 / parts;
            const uint64_t band = parts == 1 ? ~uint64_t(0) : ((uint64_t(1) << (8 * rows)) - 1) << (8 * rows * k);
            const uint64_t m = cm & band;
            if (!m) continue;
            DBlock b;
            std::memset(&b, 0, sizeof(b));
            b.x0 = (ci % cw) * 8;
            b.y0 = (ci / cw) * 8;
            b.mask_lo = uint32_t(m);
            b.mask_hi = uint32_t(m >> 32);
            b.out_base = int32_t(npix);
            b.flags = (pl & kPlanPrio) ? kBlockPrio : 0;
            npix += __builtin_popcountll(m);
            out.push_back(b);
            if (pl & kPlanClassMask) classes = true;
        }
    }
    if (classes) {  // dispatch order only: out_base keeps every block's packed slots
        std::stable_sort(out.begin(), out.end(), [&](const DBlock& a, const DBlock& b) {
            return (cplan[size_t(a.y0 / 8) * size_t(cw) + size_t(a.x0 / 8)] & kPlanClassMask) >
                   (cplan[size_t(b.y0 / 8) * size_t(cw) + size_t(b.x0 / 8)] & kPlanClassMask);
        });
    }
    for (size_t i = 0; i < out.size(); ++i) out[i].base = int32_t(i);
}

// load_model_data's pool size (OBJ_loader.cpp:298: one chunk per pool thread): the host's
// hardware threads, at most 16.
int32_t default_parse_threads() {
    const unsigned hw = std::thread::hardware_concurrency();
    return int32_t(std::max(1u, std::min(16u, hw)));
}
#ifndef ATR_MAX_BATCH_LOG2  // experiment builds: 29 to study the 2^29-path cliff
#define ATR_MAX_BATCH_LOG2 28
#endif
#ifndef ATR_PATH_SPLIT_DEFAULT
#define ATR_PATH_SPLIT_DEFAULT 0
#endif
atr_tuning default_tuning() {
    atr_tuning t;
    std::memset(&t, 0, sizeof(t));
    t.xcd_chunk = 16;      // chunks of 16 cells per XCD, interleaved
    t.frame_rotate = 0;    // §4b: rotation measured slower
    t.hybrid_a = 2;        // §4e: sweep optimum
    t.hybrid_b = 0;
    t.path_batch_log2 = 28;  // §4h: 2^28 paths per batch (c4: a frame in one batch, two per batch in flight)
    t.cluster_size = kMaxClusterSize;  // §4b: 8-16 is the flat optimum
    t.frame_plan = 1;      // §4g: single-frame launches dispatch by the previous frame's costs
    t.path_sort_bits = 5;  // §4h: each level's queue in (direction, origin) order, 5 bits per axis
    t.path_split = ATR_PATH_SPLIT_DEFAULT;  // §4h: a one-batch launch as two half batches
    return t;
}
constexpr int kSchedPaths = 10;             // the sample-parallel path engine (paths.hip)
constexpr int kMaxPathBounces = 64;         // bounce launches per batch (AUTO: deeper paths run FLAT)
constexpr int kQueueSlots = 32;             // traced-ray counter sets in flight (ring)
constexpr size_t kTraceBytes = 64 * 128;    // 64 traced-ray counters, 128 B apart (render.hip)

}  // namespace

struct atr_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t last_stream = nullptr;
    // ev_start before every render; its completion event ev_last: the traced-ray set's event of
    // launch_render (one record per launch), or ev_stop for a launch without traced rays
    hipEvent_t ev_start = nullptr, ev_stop = nullptr, ev_last = nullptr;
    bool have_render = false;
    int32_t last_ntiles = 0;
    std::vector<DevBuf> scene_bufs;
    DScene* d_scene = nullptr;
    int64_t scene_bytes = 0;
    int32_t max_nodes = 0, max_depth = 0, nmodels = 0, max_inner = 0;
    float scene_box[6] = {0.f, 0.f, 0.f, 1.f, 1.f, 1.f};  // the models' vertex bounds (lo, hi): queue-sort cells
    atr_tuning tune = default_tuning();  // atr_set_tuning
    int64_t nclusters = 0;
    // the tree models' leaves (discovery ranks) in model order, DModel::lf_base / lf_count, and per
    // scene leaf its {first scene cluster, cluster count} (atr_camera_leaf_boxes_row)
    int64_t nleaves = 0;
    std::vector<uint32_t> leaf_clusters;
    // per-cell plan (atr_set_cell_plan) for images of cplan_w x cplan_h; cplan_gen invalidates
    // the block cache
    std::vector<uint8_t> cplan;
    int32_t cplan_w = 0, cplan_h = 0;
    uint32_t cplan_gen = 0;
    static constexpr int kBlockSlots = 24;  // tile-list cache: own render + one unpack per rank
    BlockSet blocks[kBlockSlots];
    uint64_t block_use[kBlockSlots] = {};
    uint64_t use_clock = 0;
    int32_t* d_error = nullptr;
    int ncu = 256;
    // path engine workspace per stream (paths.hip: two path queues, the per-path results and the
    // per-level counters), grown on demand
    struct PathWS {
        hipStream_t stream = nullptr;
        DevBuf mem;
        int64_t cap = 0;
        int32_t levels = 0;
        int64_t sort_bins = 0;    // queue-sort buffers for this many bins (PathSort), or none
        bool live = false;        // has the live-list area of adaptive passes (PathLive)
        hipEvent_t ev = nullptr;  // recorded after the latest launch that used `mem`
        uint64_t last_use = 0;
    };
    static constexpr size_t kMaxPathWS = 4;  // workspaces at most (streams beyond share them)
    // a one-batch PATHS launch runs as two half batches on these streams (fork / join events)
    hipStream_t split_stream[2] = {};
    hipEvent_t split_fork = nullptr, split_join[2] = {};
    uint64_t ws_clock = 0;
    std::vector<PathWS> path_ws;
    // launches' traced-ray counter sets: a ring, each set reused only after the launch that last
    // used it (event) has finished; zeroed by its finish kernel
    void* tring = nullptr;
    hipEvent_t tev[kQueueSlots] = {};
    bool tused[kQueueSlots] = {};
    int tnext = 0;
    // progressive render (atr_render_start_progressive): one launch per tile group, an event
    // after each; prog_end[g] = tiles complete once group g is
    bool prog_active = false;
    std::vector<DevBuf> prog_blocks;
    std::vector<hipEvent_t> prog_ev;
    std::vector<int32_t> prog_end;
    // last launch per stream: everything this context has in flight (scene frees, workspace
    // regrowth and progressive group buffers wait for all of them)
    std::vector<std::pair<hipStream_t, hipEvent_t>> stream_ev;
    int32_t wave_slots = 0;  // CUs x 4 SIMDs x 6 waves (single-frame plan policy), 0 until first use
    hipStream_t plan_side = nullptr;  // the single-frame plan kernels' stream (created on first use)
    // adaptive passes' counts (atr_render_adaptive_info): a ring of 4 u64 per pass, zeroed on the
    // pass's stream before its kernels add to it; adapt_last = the last pass enqueued (-1: none)
    static constexpr int kAdaptSlots = 8;
    unsigned long long* adapt_info = nullptr;
    int adapt_next = 0, adapt_last = -1;
    // Tables of box growths for the primary kernels (RenderParams::pads): one row of
    // {loose, tight} pairs per camera of a launch. A launch whose scene upload (scene_gen), row
    // count and eyes (bit-equal) match a slot reads it as it is -- any number of launches in flight
    // may share a table -- else it rebuilds the least recently used slot on its own stream, after a
    // GPU-side wait for that slot's build and for the last launch on every stream that read it
    // (`readers`: the slot's own events, never the traced-ray ring's). camera_pads: ATR_CAMERA_PADS
    // at atr_create (0 = the kernels that compute the pairs inline).
    struct PadSlot {
        DevBuf mem;
        uint64_t gen = 0;  // scene_gen of the table's scene; 0: empty
        int32_t rows = 0;
        bool wide = false;  // a COUNT launch's table: two pairs per cluster (cluster.h pads_entry)
        // The rows' leaf boxes (RenderParams::lbox; cluster.h leaf_box_add) follow the pairs in the same
        // buffer, built right after them on the same stream: one key, one build event, one set of
        // readers, one cap. 0: the table has none (ATR_LEAF_BOX=0).
        size_t lbox_off = 0;
        float eye[kMaxFrameCams][3];
        hipEvent_t built = nullptr;
        hipStream_t built_on = nullptr;
        std::vector<std::pair<hipStream_t, hipEvent_t>> readers;
        uint64_t last_use = 0;
    };
    static constexpr int kPadSlots = 4;
    static constexpr size_t kPadMaxBytes = size_t(256) << 20;  // larger tables: the inline kernels
    PadSlot pad_slot[kPadSlots];
    uint64_t pad_clock = 0, scene_gen = 0;
    bool camera_pads = true;
    // ATR_FACING_FOLD at atr_create (0 = the table holds the unfolded loose growths; cluster.h fold_box)
    bool facing_fold = true;
    // ATR_WAVE_CULL at atr_create (0 = the primary kernels test every cluster of a leaf per ray)
    bool wave_cull = true;
    // ATR_LEAF_BOX at atr_create (0 = no table of leaf boxes: the primary passes insert every leaf)
    bool leaf_box = true;
    // ATR_SKY_PATH at atr_create (0 = every wave of the primary kernels walks the scene), and the
    // scene's record for that path (engine.h SkyRecord; atr_scene_upload fills it, `on` included)
    bool sky_path = true;
    SkyRecord sky = {};
    // Ray queries' workspace (atr_trace_rays, query.hip), apart from the path workspaces and grow-only:
    // `rays` = {key, rank} and the key order for `cap` rays (12 B each; sorted batches only) and, in
    // its first 256 B, the head counter; `bins` = `nbins` arrival counters (zero between calls: the
    // bin scan leaves them so), their starts and block sums. One per context: a call on another
    // stream than the last first waits (on the GPU) for `ev`, recorded after every call.
    struct QueryWS {
        DevBuf rays, bins;
        int64_t cap = 0, nbins = 0;
        hipEvent_t ev = nullptr;
        hipStream_t stream = nullptr;
        bool used = false;
    } query_ws;
    // Lightmap texels' workspaces (texels.hip), grow-only and apart from the two above. tex_ws
    // (atr_mesh_texels): `mesh` = the mesh's arrays as the kernels read them, `map` = the face per texel,
    // `aux` = the scan's block sums and the larger faces' list. The call is synchronous, so nothing of
    // it is in flight between calls; it still starts with wait_all and records its launches
    // (note_launch). img_ws (atr_texels_to_image): the dilation's second image and the two flag
    // arrays; one per context, ordered between streams by `ev` as query_ws is.
    struct TexelWS {
        DevBuf mesh, map, aux;
    } tex_ws;
    struct ImageWS {
        DevBuf image, flags;
        hipEvent_t ev = nullptr;
        hipStream_t stream = nullptr;
        bool used = false;
    } img_ws;
    // Denoise workspace (atr_denoise, denoise.hip), grow-only and apart from all of the above: `color` =
    // the two ping-pong images of 16-B colour records, `guides` = the 16-B normal and position records
    // of the guides the call has; one per context, ordered between streams by `ev` as img_ws is.
    struct DenoiseWS {
        DevBuf color, guides;
        hipEvent_t ev = nullptr;
        hipStream_t stream = nullptr;
        bool used = false;
    } dn_ws;
    // Variance-guided denoise workspace (atr_denoise_variance, denoise_variance.hip), grow-only and apart
    // from dn_ws, so that an atr_denoise and an atr_denoise_variance on two streams share nothing:
    // `color` = the two ping-pong images of 16-B colour records, `var` = the two images of 8-B
    // {variance, luminance} records, `guides` as in dn_ws; ordered between streams by `ev` as dn_ws is.
    struct DenoiseVarWS {
        DevBuf color, var, guides;
        hipEvent_t ev = nullptr;
        hipStream_t stream = nullptr;
        bool used = false;
    } dnv_ws;
};

namespace {

// Scheduling knobs of a context (atr_set_tuning); each launch copies them into RenderParams.
void apply_tuning(const atr_ctx* c, RenderParams& P) {
    P.xcd_chunk = c->tune.xcd_chunk;
    P.frame_rotate = 0;
    P.hyb_a = c->tune.hybrid_a;
    P.hyb_b = c->tune.hybrid_b;
    P.wave_cull = c->wave_cull ? 1 : 0;
    P.sky = c->sky;
}

int dev_upload(atr_ctx* c, const void* src, size_t bytes, void** out) {
    DevBuf b;
    b.n = bytes ? bytes : 16;
    HIPCHK(hipMalloc(&b.p, b.n));
    if (bytes) {
        const hipError_t e = hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(b.p);
            return -(1000 + int(e));
        }
    }
    c->scene_bufs.push_back(b);
    c->scene_bytes += int64_t(b.n);
    *out = b.p;
    return ATR_OK;
}

// The sky path's record of a scene (engine.h SkyRecord; render.hip) from an upload's inputs and its
// packed trees (packed[i] of a tree model, as pack_tree left it): per model the six floats its query
// starts with as the device tables hold them -- nodes[0]'s bounds of a tree model (scan.h flat_begin:
// box_check), the surrounding_aabb copied into DModel::aabb of a brute-force one (scan.h
// intersect_models: box_entry) -- and what shade.h scene_finish leaves for a ray that hits no model
// when there is no sphere and no plane: type T_SKY, so material 0's emission, face kSkyFace, and t =
// the kMaxFloat that intersect_models' SceneHit starts from. on = 0, and no box recorded, with more
// models than the record holds or with any sphere or plane.
void sky_record(const atr_material* mats, const atr_model* models, int32_t nmodels, int32_t nspheres,
                int32_t nplanes, const std::vector<PackedTree>& packed, SkyRecord& sky) {
    sky = SkyRecord{};
    sky.on = nmodels <= kSkyBoxes && nspheres == 0 && nplanes == 0 ? 1 : 0;
    sky.face = kSkyFace;
    sky.t = kMaxFloat;
    sky.em[0] = mats[0].emission.x, sky.em[1] = mats[0].emission.y, sky.em[2] = mats[0].emission.z;
    if (!sky.on) return;
    sky.n = nmodels;
    for (int32_t i = 0; i < nmodels; ++i) {
        if (models[i].tree) {
            if (packed[size_t(i)].nodes.empty()) {  // no root to test: every wave walks the scene
                sky.on = sky.n = 0;
                return;
            }
            const DNode& r = packed[size_t(i)].nodes[0];
            const float b[6] = {r.lo_x, r.lo_y, r.lo_z, r.hi_x, r.hi_y, r.hi_z};
            std::memcpy(sky.box[i], b, sizeof(b));
        } else {
            std::memcpy(sky.box[i], models[i].surrounding_aabb, sizeof(sky.box[i]));
            sky.brute |= 1u << i;
        }
    }
}

// A mesh's per-face shading record (renderer.cpp:124-149; DModel::shade, read by shade.h's
// scene_finish): 9 floats per face, the three vertex normals of a smooth mesh (one that has any
// normals, renderer.cpp:129) or the three vertices of a flat one. Returns DModel::smooth. The scene
// upload and atr_mesh_texels both build theirs here, so the texels' normals are the renderer's.
int32_t shade_records(const HostMesh& M, std::vector<float>& shade) {
    const int32_t smooth = M.normals.empty() ? 0 : 1;
    const size_t nf = M.nfaces();
    shade.assign(9 * (nf ? nf : 1), 0.f);
    for (size_t f = 0; f < nf; ++f) {
        for (int k = 0; k < 3; ++k) {
            V3 v = mk(0.f, 0.f, 0.f);
            if (smooth) {
                const int32_t ni = M.face_n[3 * f + size_t(k)];
                if (ni >= 0 && size_t(ni) < M.normals.size()) v = M.normals[size_t(ni)];
            } else {
                const int32_t vi = M.face_v[3 * f + size_t(k)];
                if (vi >= 0 && size_t(vi) < M.vertices.size()) v = M.vertices[size_t(vi)];
            }
            shade[9 * f + 3 * size_t(k)] = v.x;
            shade[9 * f + 3 * size_t(k) + 1] = v.y;
            shade[9 * f + 3 * size_t(k) + 2] = v.z;
        }
    }
    return smooth;
}

// Record on stream s, in a (stream, event) list, that work on s is in flight. Entries whose work
// has completed are reused, so a caller that creates a stream per job does not grow the list.
hipError_t note_stream(std::vector<std::pair<hipStream_t, hipEvent_t>>& list, hipStream_t s) {
    for (auto& se : list)
        if (se.first == s) return hipEventRecord(se.second, s);
    for (auto& se : list)
        if (hipEventQuery(se.second) == hipSuccess) {  // finished: take over its event
            se.first = s;
            return hipEventRecord(se.second, s);
        }
    hipEvent_t ev = nullptr;
    hipError_t e;
    if ((e = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) != hipSuccess) return e;
    list.emplace_back(s, ev);
    return hipEventRecord(ev, s);
}

// Wait for every entry of a list (all streams).
hipError_t wait_list(const std::vector<std::pair<hipStream_t, hipEvent_t>>& list) {
    for (const auto& se : list) {
        const hipError_t e = hipEventSynchronize(se.second);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// Record that a launch on stream s is in flight. (A block set's buffers are rewritten or freed
// only after every stream's latest launch, wait_all: a cache miss or a first per-tile query, rare,
// so launches record no event per block set.) A render whose completion event is one of the
// traced-ray ring's (ring = true) records nothing here: wait_all also waits for every ring event in
// use, and a ring event is re-recorded only on a stream that first waited for its previous record
// (launch_render), so it still covers every launch that recorded it.
hipError_t note_launch(atr_ctx* c, hipStream_t s, bool ring = false) {
    return ring ? hipSuccess : note_stream(c->stream_ev, s);
}

// Wait for every launch of this context still in flight, on any stream.
hipError_t wait_all(atr_ctx* c) {
    hipError_t e = wait_list(c->stream_ev);
    for (int k = 0; e == hipSuccess && k < kQueueSlots; ++k)
        if (c->tused[k]) e = hipEventSynchronize(c->tev[k]);
    return e;
}

// A launch's set of 64 spread traced-ray counters from the ring: ring_take hands out the next set
// (zeroed by the finish kernel of the launch that last used it, which s first waits for) and
// ring_done, after the launch's own finish kernel (atr_launch_traced_finish), records the set's
// event -- the launch's completion event.
hipError_t ring_take(atr_ctx* c, hipStream_t s, int& k, unsigned long long*& slots) {
    k = c->tnext;
    c->tnext = (k + 1) % kQueueSlots;
    if (c->tused[k]) {
        const hipError_t e = hipStreamWaitEvent(s, c->tev[k], 0);
        if (e != hipSuccess) return e;
    }
    slots = reinterpret_cast<unsigned long long*>(static_cast<char*>(c->tring) + size_t(k) * kTraceBytes);
    return hipSuccess;
}
hipError_t ring_done(atr_ctx* c, hipStream_t s, int k) {
    const hipError_t e = hipEventRecord(c->tev[k], s);
    if (e == hipSuccess) c->tused[k] = true;
    return e;
}

void free_scene(atr_ctx* c) {
    for (DevBuf& b : c->scene_bufs) (void)hipFree(b.p);
    c->scene_bufs.clear();
    c->d_scene = nullptr;
    c->scene_bytes = 0;
}

BlockSet* get_blocks(atr_ctx* c, const atr_tile* tiles, int32_t ntiles, int32_t W, int32_t H, int& rc) {
    rc = ATR_OK;
    int lru = 0;
    for (int i = 0; i < atr_ctx::kBlockSlots; ++i) {
        BlockSet& b = c->blocks[i];
        if (b.width == W && b.height == H && int32_t(b.tiles.size()) == ntiles && b.dev.p &&
            b.cplan_gen == c->cplan_gen && (ntiles == 0 || std::memcmp(b.tiles.data(), tiles, sizeof(atr_tile) * size_t(ntiles)) == 0)) {
            c->block_use[i] = ++c->use_clock;
            return &b;
        }
        if (c->block_use[i] < c->block_use[lru]) lru = i;
    }
    BlockSet& b = c->blocks[lru];
    c->block_use[lru] = ++c->use_clock;
    // the slot may still be read by in-flight kernels of earlier renders, on several streams
    {
        const hipError_t e = wait_all(c);
        if (e != hipSuccess) { rc = -(1000 + int(e)); return nullptr; }
    }
    b.tiles.assign(tiles, tiles + ntiles);
    b.tile_ready = false;
    b.plan_ready = false;
    b.width = W;
    b.height = H;
    b.cplan_gen = c->cplan_gen;
    const bool planned = !c->cplan.empty() && c->cplan_w == W && c->cplan_h == H;
    build_blocks(tiles, ntiles, W, H, b.host, b.packed_pixels, 0, planned ? c->cplan.data() : nullptr);
    const size_t need = std::max<size_t>(b.host.size() * sizeof(DBlock), 32);
    if (b.dev.n < need) {
        if (b.dev.p) (void)hipFree(b.dev.p);
        b.dev = DevBuf();
        if (hipMalloc(&b.dev.p, need) != hipSuccess) { rc = ATR_E_NOMEM; return nullptr; }
        b.dev.n = need;
    }
    const size_t tneed = std::max<size_t>(sizeof(atr_tile) * size_t(ntiles), 16);
    if (b.dev_tiles.n < tneed) {
        if (b.dev_tiles.p) (void)hipFree(b.dev_tiles.p);
        b.dev_tiles = DevBuf();
        if (hipMalloc(&b.dev_tiles.p, tneed) != hipSuccess) { rc = ATR_E_NOMEM; return nullptr; }
        b.dev_tiles.n = tneed;
    }
    hipError_t e = hipMemcpy(b.dev.p, b.host.data(), b.host.size() * sizeof(DBlock), hipMemcpyHostToDevice);
    if (e == hipSuccess && ntiles)
        e = hipMemcpy(b.dev_tiles.p, tiles, sizeof(atr_tile) * size_t(ntiles), hipMemcpyHostToDevice);
    if (e != hipSuccess) { rc = -(1000 + int(e)); b.width = -1; return nullptr; }
    return &b;
}

// Grow a device buffer to `bytes` (contents undefined when it grows; zeroed if `zero`).
int ensure_buf(DevBuf& d, size_t bytes, bool zero) {
    if (d.n >= bytes && d.p) return ATR_OK;
    if (d.p) (void)hipFree(d.p);
    d = DevBuf();
    if (hipMalloc(&d.p, bytes) != hipSuccess) return ATR_E_NOMEM;
    d.n = bytes;
    if (zero && hipMemset(d.p, 0, bytes) != hipSuccess) return ATR_E_NOMEM;
    return ATR_OK;
}

// variant (atray.h) -> kernel schedule (render.hip). AUTO = the measured fastest.
// variant (atray.h) -> schedule (render.hip / paths.hip); -1 = not a variant of this build.
int sched_of(int32_t variant) {
    switch (variant) {
        case ATR_KERNEL_LANE: return 0;
        case ATR_KERNEL_FLAT: return 6;
        case ATR_KERNEL_HYBRID: return 7;
        case ATR_KERNEL_PATHS: return kSchedPaths;
        default: return -1;
    }
}

// AUTO: the fastest exact schedule for the camera (measured): primary-only renders
// (one sample, bounce_limit 1, no AA) on HYBRID cells (lane-private leaf scans for coherent rays,
// dealt rounds for the stragglers); everything else on the sample-parallel path engine (a pixel's
// samples side by side, one launch per bounce), or the FLAT cell megakernel for paths deeper than
// its bounce launches.
// -1: not a variant of this build, or a request it cannot run (PATHS beyond its bounce launches):
// every entry point answers ATR_E_INVALID before it changes any state.
int auto_sched(int32_t variant, const atr_camera& cam) {
    if (variant == ATR_KERNEL_PATHS && cam.bounce_limit > kMaxPathBounces) return -1;
    if (variant != ATR_KERNEL_AUTO) return sched_of(variant);
    if (cam.bounce_limit == 1 && !cam.anti_aliasing && cam.samples_per_pixel == 1) return sched_of(ATR_KERNEL_HYBRID);
    return cam.bounce_limit <= kMaxPathBounces ? kSchedPaths : sched_of(ATR_KERNEL_FLAT);
}

// A single-frame launch of a cell schedule with the single-frame plan (tuning frame_plan, plan.hip):
// the render dispatches the block list planned after the previous such launch of this tile list on
// this stream (the base list the first time), adds each cell's clocks into the set's cost buffer,
// and the plan kernels then build the next list from them. Another stream, a user cell plan for the
// size or frame_plan 0 -> the plain base-list launch.
// The render's completion event (ev_last) is recorded right after the render; the plan kernels
// run on the plan stream, so atr_render_wait, atr_last_kernel_ms and the next launch on s do not
// wait for them.
hipError_t launch_render(atr_ctx* c, RenderParams& P, int sched, hipStream_t s, hipEvent_t* done = nullptr,
                         const PathLive* live = nullptr);

// One completion record per launch: `done` (the traced-ray set's event launch_render recorded after
// the render) when there is one, else ev_stop.
hipError_t record_stop(atr_ctx* c, hipStream_t s, hipEvent_t done) {
    if (done) {
        c->ev_last = done;
        return hipSuccess;
    }
    c->ev_last = c->ev_stop;
    return hipEventRecord(c->ev_stop, s);
}

// The opening and the closing of a device call on stream s: the start of its timed range, and its
// completion record -- `done`, the traced-ray ring event that covers the call, or null for ev_stop,
// which the stream's list then notes (note_launch) -- with what atr_render_wait reads of it.
hipError_t call_begin(atr_ctx* c, hipStream_t s) {
    c->prog_active = false;
    return hipEventRecord(c->ev_start, s);
}
hipError_t call_end(atr_ctx* c, hipStream_t s, hipEvent_t done, int32_t ntiles = 0) {
    hipError_t e = record_stop(c, s, done);
    if (e == hipSuccess) e = note_launch(c, s, c->ev_last != c->ev_stop);  // a ring event covers it
    if (e != hipSuccess) return e;
    c->have_render = true;
    c->last_stream = s;
    c->last_ntiles = ntiles;
    return hipSuccess;
}

int launch_planned(atr_ctx* c, BlockSet* bs, RenderParams& P, int sched, hipStream_t s) {
    const int32_t nb = int32_t(bs->host.size());
    // on top of a user cell plan too: its classes order the base list (and the multi-frame
    // launches), the frame plan re-orders that list for single frames by their measured cost
    const bool use = c->tune.frame_plan && nb > 0 && sched != kSchedPaths &&
                     (!bs->plan_ready || bs->plan_stream == s);
    hipEvent_t done = nullptr;
    if (!use) {
        HIPCHK(launch_render(c, P, sched, s, &done));
        HIPCHK(record_stop(c, s, done));
        return ATR_OK;
    }
    // A launch whose cells fit the chip's wave slots at once (a shard's frame: 4,050 cells of an
    // 8-way c3 plan vs 6,144 slots at 6 waves/SIMD) leaves slots idle while its heaviest cells
    // finish: there the heaviest 3 % take four waves and the next 7 % two, which shortens the
    // frame's critical path at no throughput cost. Larger launches split the heaviest 1 % in two.
    if (!c->wave_slots) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess || cus <= 0)
            cus = 256;
        c->wave_slots = cus * 4 * 6;
    }
    const bool small = nb <= c->wave_slots;
    const float split2 = small ? 0.10f : -1.f, split4 = small ? 0.03f : -1.f;
    const int32_t max_split = std::max<int32_t>(1, small ? nb / 5 : nb / 25);  // spare blocks for splits
    const size_t cap = size_t(nb + max_split);
    int rc;
    const bool fresh = !bs->cost.p;  // the buffers start zeroed; each plan leaves them zeroed
    if ((rc = ensure_buf(bs->cost, 2 * size_t(nb) * sizeof(unsigned long long), true))) return rc;
    if ((rc = ensure_buf(bs->cost_last, size_t(nb) * sizeof(unsigned long long), false))) return rc;
    if ((rc = ensure_buf(bs->plan_work, atr_plan_work_bytes(nb), true))) return rc;
    if ((rc = ensure_buf(bs->plan_blocks, 2 * cap * sizeof(DBlock), false))) return rc;
    if (!c->plan_side) HIPCHK(hipStreamCreateWithFlags(&c->plan_side, hipStreamNonBlocking));
    for (hipEvent_t& e : bs->plan_ev)
        if (!e) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    if (!bs->plan_ready && !fresh) {  // a rebuilt set reuses buffers a plan may not have cleared
        HIPCHK(hipMemsetAsync(bs->cost.p, 0, 2 * size_t(nb) * sizeof(unsigned long long), s));
        // and the work area's thresholds (learned on the old list, whose nb and max_split differ):
        // back to the documented zeroed state (class 0, no split) for the first plan on this list
        HIPCHK(hipMemsetAsync(bs->plan_work.p, 0, atr_plan_work_bytes(nb), s));
    }
    if (!bs->plan_ready) {
        bs->plan_valid[0] = bs->plan_valid[1] = false;
        bs->plan_par = 0;
    }
    bs->max_split = max_split;
    const int par = bs->plan_par;
    DBlock* list = static_cast<DBlock*>(bs->plan_blocks.p) + size_t(par) * cap;
    unsigned long long* cost = static_cast<unsigned long long*>(bs->cost.p) + size_t(par) * size_t(nb);
    if (bs->plan_valid[par]) {  // this parity's list, built beside the previous launch, and its cost
        HIPCHK(hipStreamWaitEvent(s, bs->plan_ev[par], 0));  // half cleared by the same kernels
        P.blocks = list;
        P.nblocks = int32_t(cap);
    }
    P.block_cost = cost;
    HIPCHK(launch_render(c, P, sched, s, &done));
    HIPCHK(record_stop(c, s, done));
    HIPCHK(hipStreamWaitEvent(c->plan_side, c->ev_last, 0));
    HIPCHK(atr_launch_plan(static_cast<const DBlock*>(bs->dev.p), nb, cost,
                           static_cast<unsigned long long*>(bs->cost_last.p), bs->plan_work.p, list, max_split,
                           split2, split4, c->plan_side));
    HIPCHK(hipEventRecord(bs->plan_ev[par], c->plan_side));
    HIPCHK(note_stream(c->stream_ev, c->plan_side));
    bs->plan_valid[par] = true;
    bs->plan_par = par ^ 1;
    bs->plan_ready = true;
    bs->plan_stream = s;
    return ATR_OK;
}

// The path engine's workspace for stream s, at least `cap` paths per batch and `levels` bounce
// levels. Each workspace belongs to the stream that used it last; a stream without one takes over
// an idle workspace (its last launch finished), else opens a new one while there are fewer than
// kMaxPathWS, else takes the least recently used one after a GPU-side wait on that workspace's last
// launch. So the total stays bounded however many streams render. Growing a workspace waits for
// its own last launch only. When the device has no memory for it, idle workspaces of other streams
// are released and the allocation retried once; hipErrorOutOfMemory then goes back to the caller
// (launch_paths halves its batch, then drops the queue sort, and launch_kernels falls back to FLAT).
// Queue-sort buffers after the queues and counters (256-B aligned): {key, rank} and the key order
// per entry, then `bins` bins, their starts and block sums.
size_t sort_offset(int64_t cap, int32_t levels) {
    return (size_t(cap) * 16 * (2 * kPathPlanes + 1) + size_t(levels) * sizeof(PathCtl) + 255) & ~size_t(255);
}
size_t sort_bytes(int64_t cap, int64_t bins) {
    return size_t(cap) * 12 + size_t(bins) * 8 + size_t(bins / kSortChunk) * 4;
}

// The live list of an adaptive pass (PathLive) after everything else (256-B aligned; only in a
// workspace that an adaptive pass has used): per cell a mask and a first group, per group its
// cell, per scan chunk three sums, and the control words. A batch of `cap` paths has at most
// cap / 64 cells and as many groups.
size_t live_bytes(int64_t cap) {
    const size_t cells = size_t(cap) / 64 + 1;
    return cells * 16 + (cells / kLiveChunk + 1) * 12 + 256;
}
size_t live_offset(int64_t cap, int32_t levels, int64_t bins) {
    const size_t b = bins ? sort_offset(cap, levels) + sort_bytes(cap, bins)
                          : size_t(cap) * 16 * (2 * kPathPlanes + 1) + size_t(levels) * sizeof(PathCtl);
    return (b + 255) & ~size_t(255);
}

hipError_t path_workspace(atr_ctx* c, hipStream_t s, int64_t cap, int64_t grow_to, int32_t levels, int64_t sort_bins,
                          bool live, atr_ctx::PathWS*& out) {
    atr_ctx::PathWS* ws = nullptr;
    hipError_t e;
    for (auto& w : c->path_ws)
        if (w.stream == s) ws = &w;
    if (!ws)
        for (auto& w : c->path_ws)
            if (!ws && w.ev && hipEventQuery(w.ev) == hipSuccess) ws = &w;
    if (!ws && c->path_ws.size() < atr_ctx::kMaxPathWS) {
        c->path_ws.emplace_back();
        ws = &c->path_ws.back();
        if ((e = hipEventCreateWithFlags(&ws->ev, hipEventDisableTiming)) != hipSuccess) return e;
    }
    if (!ws) {
        ws = &c->path_ws[0];
        for (auto& w : c->path_ws)
            if (w.last_use < ws->last_use) ws = &w;
    }
    if (ws->stream != s && ws->mem.p && (e = hipStreamWaitEvent(s, ws->ev, 0)) != hipSuccess) return e;
    ws->stream = s;
    ws->last_use = ++c->ws_clock;
    if (ws->cap < cap || ws->levels < levels || ws->sort_bins < sort_bins || (live && !ws->live)) {
        if ((e = hipEventSynchronize(ws->ev)) != hipSuccess) return e;
        if (ws->mem.p && (e = hipFree(ws->mem.p)) != hipSuccess) return e;
        ws->mem = DevBuf();
        // a workspace that already held paths and is too small grows to grow_to (a full batch)
        int64_t ncap = std::max(ws->cap, ws->cap > 0 && ws->cap < cap ? std::max(cap, grow_to) : cap);
        const int32_t nlev = std::max(ws->levels, levels);
        const int64_t nbins = std::max(ws->sort_bins, sort_bins);
        const bool nlive = ws->live || live;
        ws->live = false;
        ws->cap = 0;
        ws->levels = 0;
        ws->sort_bins = 0;
        // 2 queues x kPathPlanes planes + the per-path results, 16 B per entry; the level counters;
        // the queue-sort buffers; once an adaptive pass used the workspace, the live list (0.25 B
        // per entry)
        auto bytes_for = [&](int64_t n) {
            return nlive ? live_offset(n, nlev, nbins) + live_bytes(n)
                   : nbins ? sort_offset(n, nlev) + sort_bytes(n, nbins)
                           : size_t(n) * 16 * (2 * kPathPlanes + 1) + size_t(nlev) * sizeof(PathCtl);
        };
        size_t bytes = bytes_for(ncap);
        e = hipMalloc(&ws->mem.p, bytes);
        if (e == hipErrorOutOfMemory && ncap > cap) {  // the full batch does not fit: this launch's size
            (void)hipGetLastError();
            ncap = cap;
            bytes = bytes_for(ncap);
            e = hipMalloc(&ws->mem.p, bytes);
        }
        if (e == hipErrorOutOfMemory) {
            (void)hipGetLastError();
            for (auto& w : c->path_ws)
                if (&w != ws && w.mem.p && hipEventQuery(w.ev) == hipSuccess) {
                    (void)hipFree(w.mem.p);
                    w.mem = DevBuf();
                    w.cap = 0;
                    w.levels = 0;
                    w.sort_bins = 0;
                    w.live = false;
                }
            e = hipMalloc(&ws->mem.p, bytes);
        }
        if (e != hipSuccess) {
            (void)hipGetLastError();
            ws->mem = DevBuf();
            return e;
        }
        ws->mem.n = bytes;
        ws->cap = ncap;
        ws->levels = nlev;
        ws->sort_bins = nbins;
        ws->live = nlive;
    }
    out = ws;
    return hipSuccess;
}

// The queue sort's cells over the scene box (PathSort: bits, bins, lo, sc), for the path engine's
// queues and the ray queries' batch order alike.
int32_t clamp_sort_bits(int32_t bits) {
    while (bits > 0 && (int64_t(kSortDirs) * kSortDirs << (3 * bits)) > kSortBinsMax) --bits;
    return bits;
}
void sort_cells(const atr_ctx* c, int32_t bits, PathSort& so) {
    so.bits = bits;
    so.nbins = int32_t(kSortDirs * kSortDirs) << (3 * bits);
    const float* box = c->scene_box;
    for (int a = 0; a < 3; ++a) {
        so.lo[a] = box[a];
        const float ext = box[3 + a] - box[a];
        so.sc[a] = ext > 0.0f ? float(1 << bits) / ext : 0.0f;
    }
}

// The workspace of a path launch over `ncells` cells of per_cell paths each (a render's 8x8 cells, a
// radiance query's groups of 64 rays) and the cells per batch it allows: a batch of
// 2^path_batch_log2 paths, halved while the device cannot hold its workspace (down to 2^lg_min
// paths; the outputs do not depend on the batch size); then the same without the queue sort
// (sort_bits comes back 0).
hipError_t path_batches(atr_ctx* c, hipStream_t s, int64_t per_cell, int64_t ncells, int32_t levels, int32_t lg_min,
                        bool live, int32_t& sort_bits, atr_ctx::PathWS*& ws, int64_t& cells) {
    hipError_t e = hipErrorOutOfMemory;
    for (;;) {
        const int64_t bins = sort_bits > 0 ? int64_t(kSortDirs) * kSortDirs << (3 * sort_bits) : 0;
        for (int32_t lg = c->tune.path_batch_log2; lg >= lg_min && e == hipErrorOutOfMemory; --lg) {
            const int64_t batch = std::max<int64_t>(1, (int64_t(1) << lg) / per_cell);
            cells = std::min<int64_t>(batch, ncells);
            // capacity: this launch's paths rounded up to 2^24 (at most a full batch): a one-frame c4
            // launch holds its 132.7 M paths (21 GB), not a whole 2^28 batch; a workspace that has to
            // grow grows to a full batch at once, so a stream regrows at most once (a regrow inside a
            // timed multi-frame run once measured a 4x slower c4 line, round 6)
            const int64_t need = cells * per_cell, gran = int64_t(1) << 24;
            const int64_t cap = std::max(need, std::min((need + gran - 1) / gran * gran, batch * per_cell));
            e = path_workspace(c, s, cap, std::max(batch * per_cell, cap), std::max(levels, 8), bins, live, ws);
            if (e == hipSuccess && ws->cap < cap) e = hipErrorOutOfMemory;
        }
        if (e != hipErrorOutOfMemory || sort_bits == 0) break;
        sort_bits = 0;
    }
    return e;
}

// A workspace's queues, result slots and control words and, with sort_bits > 0, its queue-sort
// buffers, bound to a launch.
void bind_path_workspace(const atr_ctx* c, const atr_ctx::PathWS* ws, int32_t sort_bits, PathParams& Q) {
    float4_t* base = static_cast<float4_t*>(ws->mem.p);
    Q.cap = ws->cap;
    Q.q[0] = base;
    Q.q[1] = base + kPathPlanes * ws->cap;
    Q.out = base + 2 * kPathPlanes * ws->cap;
    Q.ctl = reinterpret_cast<PathCtl*>(base + (2 * kPathPlanes + 1) * ws->cap);
    if (sort_bits > 0) {
        PathSort& so = Q.sort;
        sort_cells(c, sort_bits, so);
        char* sb = static_cast<char*>(ws->mem.p) + sort_offset(ws->cap, ws->levels);
        so.kr = reinterpret_cast<uint2_t*>(sb);
        sb += size_t(ws->cap) * 8;
        so.perm = reinterpret_cast<uint32_t*>(sb);
        sb += size_t(ws->cap) * 4;
        so.hist = reinterpret_cast<uint32_t*>(sb);
        so.start = so.hist + ws->sort_bins;
        so.part = so.start + ws->sort_bins;
    }
}

// A batch's control words and sort bins zeroed, ahead of its entry launch.
hipError_t reset_path_batch(const PathParams& Q, int32_t levels, int32_t sort_bits, hipStream_t s) {
    const hipError_t e = hipMemsetAsync(Q.ctl, 0, sizeof(PathCtl) * size_t(levels), s);
    if (e != hipSuccess || sort_bits <= 0) return e;
    return hipMemsetAsync(Q.sort.hist, 0, sizeof(uint32_t) * size_t(Q.sort.nbins), s);
}

// Bounce levels 1 .. bl - 1 of a batch whose entry launch filled queue 0.
hipError_t launch_bounce_levels(atr_ctx* c, PathParams& Q, int32_t bl, int32_t sort_bits, hipStream_t s) {
    hipError_t e;
    for (int32_t k = 1; k < bl; ++k) {
        if (sort_bits > 0) {  // level k - 1's queue in key order (the launches zero the bins)
            Q.bounce = k - 1;
            if ((e = atr_launch_path_sort(Q, c->ncu, s)) != hipSuccess) return e;
        }
        Q.bounce = k;
        if ((e = atr_launch_path_bounce(Q, c->ncu, c->tune.path_bounce_occ, s)) != hipSuccess) return e;
    }
    return hipSuccess;
}

// The sample-parallel path engine (paths.hip) over a cell launch's blocks: the cell list in
// batches of 2^tuning.path_batch_log2 paths, per batch the camera launch, one launch per further
// bounce (persistent waves over the previous level's queue) and the per-pixel resolve, all on s.
// With `live` (an adaptive pass: its count buffer, tolerance and info slot) every batch first builds
// its live list, the camera launch traces the list's path groups and the resolve is the adaptive one.
hipError_t launch_paths_range(atr_ctx* c, const RenderParams& P, hipStream_t s, int64_t cbeg, int64_t cend,
                              const PathLive* live = nullptr) {
    const int64_t spp = P.cam.samples_per_pixel;
    const int32_t bl = P.cam.bounce_limit;
    if (cend <= cbeg) return hipSuccess;
    if (bl > kMaxPathBounces) return hipErrorInvalidValue;
    const int64_t per_cell = 64 * std::max<int64_t>(spp, 1);
    const int32_t levels = std::max(bl, 1);
    // the queue sort pays off only when a level's queue feeds another bounce launch
    int32_t sort_bits = clamp_sort_bits(bl >= 2 ? c->tune.path_sort_bits : 0);
    atr_ctx::PathWS* ws = nullptr;
    int64_t cells = 0;
    // An adaptive pass has no cell-kernel fallback, so it tries the tuned batch size itself even
    // below 2^16 paths (other launches with such a tuning get no workspace here and render FLAT).
    const int32_t lg_min = live ? std::min(16, c->tune.path_batch_log2) : 16;
    hipError_t e = path_batches(c, s, per_cell, cend - cbeg, levels, lg_min, live != nullptr, sort_bits, ws, cells);
    if (e != hipSuccess) return e;
    PathParams Q;
    std::memset(&Q, 0, sizeof(Q));
    Q.cam = P.cam;
    Q.scene = P.scene;
    Q.seed = P.seed;
    Q.blocks = P.blocks;
    Q.frame_blocks = P.frame_blocks;
    Q.nblocks = P.nblocks;
    Q.layout = P.layout;
    Q.frame_stride = P.frame_stride;
    Q.framebuffer = P.framebuffer;
    Q.hit_face = P.hit_face;
    Q.hit_t = P.hit_t;
    Q.rgb = P.rgb;
    Q.ray_casts = P.ray_casts;
    Q.traced_rays = P.traced_rays;
    Q.error_flag = P.error_flag;
    Q.block_cost = P.block_cost;
    Q.counters = P.counters;
    bind_path_workspace(c, ws, sort_bits, Q);
    Q.xcd_chunk = P.xcd_chunk;
    Q.hyb_a = P.hyb_a;
    Q.hyb_b = P.hyb_b;
    Q.nfcam = P.nfcam;
    for (int32_t f = 0; f < P.nfcam; ++f) Q.fcam[f] = P.fcam[f];
    Q.first_sample = P.first_sample;
    Q.sample_sum = P.sample_sum;
    if (live) {
        Q.live = *live;
        char* lb = static_cast<char*>(ws->mem.p) + live_offset(ws->cap, ws->levels, ws->sort_bins);
        const size_t cells = size_t(ws->cap) / 64 + 1;
        Q.live.mask = reinterpret_cast<uint2_t*>(lb);
        Q.live.first = reinterpret_cast<uint32_t*>(lb + cells * 8);
        Q.live.group = Q.live.first + cells;
        Q.live.part = Q.live.group + cells;
        Q.live.ctl = reinterpret_cast<PathLiveCtl*>(lb + live_bytes(ws->cap) - 256);
    }
    const int occ_cam = c->tune.path_camera_occ;
    for (int64_t c0 = cbeg; c0 < cend; c0 += cells) {
        Q.cell0 = int32_t(c0);
        Q.ncells = int32_t(std::min<int64_t>(cells, cend - c0));
        if (live && (e = atr_launch_path_live(Q, s)) != hipSuccess) return e;
        if (bl > 0 && spp > 0) {
            if ((e = reset_path_batch(Q, levels, sort_bits, s)) != hipSuccess) return e;
            if ((e = live ? atr_launch_path_camera_adaptive(Q, c->ncu, s) : atr_launch_path_camera(Q, occ_cam, s)) !=
                hipSuccess)
                return e;
            if ((e = launch_bounce_levels(c, Q, bl, sort_bits, s)) != hipSuccess) return e;
        }
        if ((e = live ? atr_launch_path_resolve_adaptive(Q, s) : atr_launch_path_resolve(Q, s)) != hipSuccess) return e;
    }
    return hipEventRecord(ws->ev, s);
}

// The path engine over a launch's cell list. With tuning path_split = 1 a launch that is one batch
// (a single frame: c4's 2 M-pixel frame at 64 spp) runs as two half batches on the context's two
// split streams, forked from and joined back into s, so one half's level tails and queue sorts
// could overlap the other half's tracing; off by default (one c4 frame measured 61.1 vs 60.3 ms,
// DESIGN.md §4h). Outputs do not depend on the batching.
// A sample pass (P.sample_sum) is never split, whatever the tuning says: it runs as one range, whose
// workspace is obtained before any of its kernels is enqueued, so an out-of-memory return leaves
// the running sums untouched and launch_kernels' FLAT fallback continues from them exactly. A split
// launch's first half could have added its samples to the sums before the second half failed.
constexpr int64_t kSplitMinCells = 1024;
hipError_t launch_paths(atr_ctx* c, const RenderParams& P, hipStream_t s) {
    if (P.nblocks <= 0) return hipSuccess;
    const int64_t per_cell = 64 * std::max<int64_t>(P.cam.samples_per_pixel, 1);
    const int64_t batch = std::max<int64_t>(1, (int64_t(1) << c->tune.path_batch_log2) / per_cell);
    if (!c->tune.path_split || P.nblocks > batch || P.nblocks < kSplitMinCells || P.counters || P.block_cost ||
        P.sample_sum)
        return launch_paths_range(c, P, s, 0, P.nblocks);
    hipError_t e;
    if (!c->split_fork) {
        for (int i = 0; i < 2; ++i) {
            if ((e = hipStreamCreateWithFlags(&c->split_stream[i], hipStreamNonBlocking)) != hipSuccess) return e;
            if ((e = hipEventCreateWithFlags(&c->split_join[i], hipEventDisableTiming)) != hipSuccess) return e;
        }
        if ((e = hipEventCreateWithFlags(&c->split_fork, hipEventDisableTiming)) != hipSuccess) return e;
    }
    if ((e = hipEventRecord(c->split_fork, s)) != hipSuccess) return e;
    const int64_t half = (P.nblocks + 1) / 2;
    hipError_t r = hipSuccess;
    for (int i = 0; i < 2; ++i) {
        hipStream_t a = c->split_stream[i];
        if ((e = hipStreamWaitEvent(a, c->split_fork, 0)) != hipSuccess) return e;
        if (r == hipSuccess) r = launch_paths_range(c, P, a, i ? half : 0, i ? P.nblocks : half);
        // joined whatever happened, so a fallback render on s runs after anything queued here
        if ((e = hipEventRecord(c->split_join[i], a)) != hipSuccess) return e;
        if ((e = hipStreamWaitEvent(s, c->split_join[i], 0)) != hipSuccess) return e;
    }
    return r;
}

// An adaptive pass (`live`) is the path engine as one range, like a sample pass, and has no
// fallback: hipErrorOutOfMemory goes back to the caller, returned by launch_paths_range before it
// enqueues anything.
// Bind a table of box growths to a launch that runs HYBRID's primary kernels (atr_ctx::PadSlot):
// a cached table of the same scene and eyes, or the least recently used slot rebuilt on s ahead of
// the render. *used = the slot the launch reads (launch_kernels records the launch in its readers),
// or null with P.pads null: the kernels that compute the pairs inline (the switch is off, no
// clusters, a table beyond kPadMaxBytes, or no memory for it -- the same output bits either way).
hipError_t bind_pads(atr_ctx* c, RenderParams& P, int sched, hipStream_t s, atr_ctx::PadSlot** used) {
    *used = nullptr;
    P.pads = nullptr;
    P.pads_stride = 0;
    P.lbox = nullptr;
    P.lbox_stride = 0;
    if (!c->camera_pads || c->nclusters <= 0 || c->nclusters > int64_t(1) << 30 || !atr_render_reads_pads(P, sched))
        return hipSuccess;
    const int32_t rows = P.nfcam > 0 ? P.nfcam : 1;
    if (rows > kMaxFrameCams) return hipSuccess;
    const int32_t stride = int32_t(c->nclusters);
    // an instrumented launch reads the unfolded pair and the folded growth: a table of its own kind
    const bool wide = P.counters != nullptr;
    const size_t pbytes = size_t(rows) * size_t(stride) * sizeof(float2_t) * (wide ? 2 : 1);
    // the rows' leaf boxes behind the pairs (32-byte entries, 32-byte aligned), under the same cap
    const bool boxes = c->leaf_box && c->nleaves > 0 && c->nleaves <= int64_t(1) << 30;
    const size_t lbox_off = boxes ? (pbytes + 31) / 32 * 32 : 0;
    const size_t bytes = boxes ? lbox_off + size_t(rows) * size_t(c->nleaves) * 2 * sizeof(float4_t) : pbytes;
    if (bytes > atr_ctx::kPadMaxBytes) return hipSuccess;
    PadEyes eyes;
    std::memset(&eyes, 0, sizeof(eyes));
    for (int32_t f = 0; f < rows; ++f) {
        const atr_vec3& e = P.nfcam > 0 ? P.fcam[f].eye : P.cam.eye;
        eyes.e[f][0] = e.x, eyes.e[f][1] = e.y, eyes.e[f][2] = e.z;
    }
    hipError_t e;
    atr_ctx::PadSlot* sl = nullptr;
    atr_ctx::PadSlot* lru = &c->pad_slot[0];
    for (atr_ctx::PadSlot& q : c->pad_slot) {
        if (q.gen == c->scene_gen && q.rows == rows && q.wide == wide && std::memcmp(q.eye, eyes.e, sizeof(float) * 3 * size_t(rows)) == 0) {
            sl = &q;
            break;
        }
        if (q.last_use < lru->last_use) lru = &q;
    }
    if (sl) {  // cached: read it as it is, after its build when that ran on another stream
        if (sl->built_on != s && (e = hipStreamWaitEvent(s, sl->built, 0)) != hipSuccess) return e;
    } else {
        sl = lru;
        if (!sl->built && (e = hipEventCreateWithFlags(&sl->built, hipEventDisableTiming)) != hipSuccess) return e;
        if (sl->mem.n < bytes || !sl->mem.p) {  // grow: nothing in flight may still touch the old buffer
            if (sl->mem.p) {
                if ((e = wait_list(sl->readers)) != hipSuccess) return e;
                if ((e = hipEventSynchronize(sl->built)) != hipSuccess) return e;
                (void)hipFree(sl->mem.p);
            }
            sl->mem = DevBuf();
            sl->gen = 0;
            if (hipMalloc(&sl->mem.p, bytes) != hipSuccess) {
                (void)hipGetLastError();  // no memory for a table: the inline kernels
                sl->mem = DevBuf();
                return hipSuccess;
            }
            sl->mem.n = bytes;
        } else {  // rewrite in place: after the slot's last build and its last reader on every stream
            if (sl->gen && sl->built_on != s && (e = hipStreamWaitEvent(s, sl->built, 0)) != hipSuccess) return e;
            for (const auto& se : sl->readers)
                if (se.first != s && (e = hipStreamWaitEvent(s, se.second, 0)) != hipSuccess) return e;
        }
        sl->gen = 0;  // stays empty if the build cannot be enqueued
        if ((e = atr_launch_camera_pads(c->d_scene, eyes, rows, stride, c->facing_fold, wide, static_cast<float2_t*>(sl->mem.p),
                                        nullptr, nullptr, nullptr, s)) != hipSuccess)
            return e;
        if (boxes && (e = atr_launch_camera_leaf_boxes(c->d_scene, eyes, rows, stride, wide, static_cast<const float2_t*>(sl->mem.p),
                                                       int32_t(c->nleaves),
                                                       reinterpret_cast<float4_t*>(static_cast<char*>(sl->mem.p) + lbox_off),
                                                       s)) != hipSuccess)
            return e;
        if ((e = hipEventRecord(sl->built, s)) != hipSuccess) return e;
        sl->built_on = s;
        sl->gen = c->scene_gen;
        sl->rows = rows;
        sl->wide = wide;
        sl->lbox_off = lbox_off;
        std::memcpy(sl->eye, eyes.e, sizeof(eyes.e));
    }
    sl->last_use = ++c->pad_clock;
    P.pads = static_cast<const float2_t*>(sl->mem.p);
    P.pads_stride = stride;
    if (sl->lbox_off) {
        P.lbox = reinterpret_cast<const float4_t*>(static_cast<const char*>(sl->mem.p) + sl->lbox_off);
        P.lbox_stride = int32_t(c->nleaves);
    }
    *used = sl;
    return hipSuccess;
}

hipError_t launch_kernels(atr_ctx* c, RenderParams& P, int sched, hipStream_t s, const PathLive* live = nullptr) {
    if (live) return launch_paths_range(c, P, s, 0, P.nblocks, live);
    if (sched == kSchedPaths) {
        hipError_t e = launch_paths(c, P, s);
        if (e != hipErrorOutOfMemory) return e;
        // no memory for a path workspace: the cell megakernel, which needs none (same outputs,
        // DESIGN.md §4). A split launch may have rendered its first half already: every output is
        // rewritten, and the traced-ray counters (always a launch's zeroed ring set of 64 spread
        // counters, launch_render) start again from zero so no ray is counted twice.
        if (P.traced_rays && (e = hipMemsetAsync(P.traced_rays, 0, kTraceBytes, s)) != hipSuccess) return e;
        sched = sched_of(ATR_KERNEL_FLAT);
    }
    atr_ctx::PadSlot* pads = nullptr;  // HYBRID's primaries read the cameras' table of box growths
    hipError_t e = bind_pads(c, P, sched, s, &pads);
    if (e != hipSuccess) return e;
    e = atr_launch_render(P, sched, c->tune.primary_occ, s);
    if (e == hipSuccess && pads) e = note_stream(pads->readers, s);
    return e;
}

// Launch a render schedule; the traced rays go into a zeroed set of 64 spread counters from the
// ring, then one add to the caller's accumulator.
hipError_t launch_render(atr_ctx* c, RenderParams& P, int sched, hipStream_t s, hipEvent_t* done,
                         const PathLive* live) {
    if (done) *done = nullptr;
    if (!P.traced_rays) return launch_kernels(c, P, sched, s, live);
    int k = -1;
    unsigned long long* caller = P.traced_rays;
    hipError_t e = ring_take(c, s, k, P.traced_rays);
    if (e != hipSuccess) return e;
    e = launch_kernels(c, P, sched, s, live);
    if (e == hipSuccess) e = atr_launch_traced_finish(P.traced_rays, caller, s);
    P.traced_rays = caller;
    if (e != hipSuccess) return e;
    if ((e = ring_done(c, s, k)) != hipSuccess) return e;
    if (done) *done = c->tev[k];
    return hipSuccess;
}

}  // namespace

// No exception crosses the ABI (atray.h): every entry point that returns a status is a function
// try block, std::bad_alloc comes back as ATR_E_NOMEM and anything else as ATR_E_INVALID.
#define ATR_ABI_CATCH                                    \
    catch (const std::bad_alloc&) { return ATR_E_NOMEM; } \
    catch (...) { return ATR_E_INVALID; }

extern "C" {

const char* atr_version(void) { return "atray-mi355x 0.2 (gfx950)"; }

// ------------------------------------------------------------------ host prerequisites
int atr_mesh_parse_obj_threaded(const char* text, size_t len, int32_t threads, atr_mesh** out) try {
    if (!text || !out || threads < 0) return ATR_E_INVALID;
    if (threads == 0) threads = default_parse_threads();
    std::unique_ptr<atr_mesh> own(new (std::nothrow) atr_mesh());
    atr_mesh* m = own.get();
    if (!m) return ATR_E_NOMEM;
    const int rc = parse_obj_text(text, len, m->m, threads);
    if (rc != ATR_OK) return rc;
    *out = own.release();
    return ATR_OK;
} ATR_ABI_CATCH

int atr_mesh_parse_obj(const char* text, size_t len, atr_mesh** out) try {
    return atr_mesh_parse_obj_threaded(text, len, 1, out);
} ATR_ABI_CATCH

int atr_mesh_load_obj_threaded(const char* path, int32_t threads, atr_mesh** out) try {
    if (!path || !out || threads < 0) return ATR_E_INVALID;
    FILE* f = std::fopen(path, "rb");
    if (!f) return ATR_E_IO;
    std::string buf;
    if (std::fseek(f, 0, SEEK_END) == 0) {
        const long sz = std::ftell(f);
        if (sz > 0) buf.reserve(size_t(sz));
        std::rewind(f);
    }
    char tmp[1 << 16];
    size_t n;
    while ((n = std::fread(tmp, 1, sizeof(tmp), f)) > 0) buf.append(tmp, n);
    const bool bad = std::ferror(f) != 0;
    std::fclose(f);
    if (bad) return ATR_E_IO;
    return atr_mesh_parse_obj_threaded(buf.data(), buf.size(), threads, out);
} ATR_ABI_CATCH

int atr_mesh_load_obj(const char* path, atr_mesh** out) { return atr_mesh_load_obj_threaded(path, 0, out); }

int atr_mesh_from_arrays(const float* vertices, uint32_t nvertices, const int32_t* face_vertices,
                         uint32_t nfaces, const float* normals, uint32_t nnormals,
                         const int32_t* face_normals, atr_mesh** out) try {
    if (!out || (nvertices && !vertices) || (nfaces && !face_vertices)) return ATR_E_INVALID;
    if (nnormals && (!normals || !face_normals)) return ATR_E_INVALID;
    std::unique_ptr<atr_mesh> own(new (std::nothrow) atr_mesh());
    atr_mesh* m = own.get();
    if (!m) return ATR_E_NOMEM;
    for (uint32_t i = 0; i < nvertices; ++i) m->m.vertices.push_back(mk(vertices[3 * i], vertices[3 * i + 1], vertices[3 * i + 2]));
    for (uint32_t i = 0; i < nnormals; ++i) m->m.normals.push_back(mk(normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]));
    m->m.face_v.assign(face_vertices, face_vertices + 3 * size_t(nfaces));
    m->m.face_t.assign(3 * size_t(nfaces), -1);
    if (nnormals) m->m.face_n.assign(face_normals, face_normals + 3 * size_t(nfaces));
    else m->m.face_n.assign(3 * size_t(nfaces), -1);
    *out = own.release();
    return ATR_OK;
} ATR_ABI_CATCH

void atr_mesh_free(atr_mesh* m) { delete m; }

int atr_mesh_info(const atr_mesh* m, uint32_t* nv, uint32_t* nn, uint32_t* nf) try {
    if (!m) return ATR_E_INVALID;
    if (nv) *nv = uint32_t(m->m.vertices.size());
    if (nn) *nn = uint32_t(m->m.normals.size());
    if (nf) *nf = uint32_t(m->m.nfaces());
    return ATR_OK;
} ATR_ABI_CATCH

int atr_mesh_export(const atr_mesh* m, float* vertices, float* normals, float* texcoords, uint32_t* ntexcoords,
                    int32_t* face_v, int32_t* face_t, int32_t* face_n) try {
    if (!m) return ATR_E_INVALID;
    auto put = [](float* dst, const std::vector<V3>& src) {
        if (!dst) return;
        for (size_t i = 0; i < src.size(); ++i) { dst[3 * i] = src[i].x; dst[3 * i + 1] = src[i].y; dst[3 * i + 2] = src[i].z; }
    };
    put(vertices, m->m.vertices);
    put(normals, m->m.normals);
    put(texcoords, m->m.texcoords);
    if (ntexcoords) *ntexcoords = uint32_t(m->m.texcoords.size());
    if (face_v) std::memcpy(face_v, m->m.face_v.data(), m->m.face_v.size() * sizeof(int32_t));
    if (face_t) std::memcpy(face_t, m->m.face_t.data(), m->m.face_t.size() * sizeof(int32_t));
    if (face_n) std::memcpy(face_n, m->m.face_n.data(), m->m.face_n.size() * sizeof(int32_t));
    return ATR_OK;
} ATR_ABI_CATCH

int atr_mesh_aabb(const atr_mesh* m, float aabb_out[6]) try {
    if (!m || !aabb_out) return ATR_E_INVALID;
    mesh_aabb(m->m, aabb_out);
    return ATR_OK;
} ATR_ABI_CATCH

int atr_mesh_translate_to(atr_mesh* m, float aabb[6], atr_vec3 c) try {
    if (!m || !aabb) return ATR_E_INVALID;
    mesh_translate(m->m, aabb, mk(c.x, c.y, c.z));
    return ATR_OK;
} ATR_ABI_CATCH

int atr_octree_build(const atr_mesh* m, uint32_t max_faces, atr_octree** out) try {
    if (!m || !out) return ATR_E_INVALID;
    std::unique_ptr<atr_octree> own(new (std::nothrow) atr_octree());
    atr_octree* t = own.get();
    if (!t) return ATR_E_NOMEM;
    const int rc = octree_build(m->m, max_faces, t->t);
    if (rc != ATR_OK) return rc;
    *out = own.release();
    return ATR_OK;
} ATR_ABI_CATCH

int atr_octree_build_device(const atr_mesh* m, uint32_t max_faces, int32_t device, atr_octree** out,
                            float ms_out[2]) try {
    if (!m || !out || device < 0) return ATR_E_INVALID;
    std::unique_ptr<atr_octree> own(new (std::nothrow) atr_octree());
    atr_octree* t = own.get();
    if (!t) return ATR_E_NOMEM;
    const int rc = octree_build_device(m->m, max_faces, device, t->t, ms_out);
    if (rc != ATR_OK) return rc;
    *out = own.release();
    return ATR_OK;
} ATR_ABI_CATCH

int atr_octree_from_nodes(int32_t nnodes, const float* bounds, const int32_t* children,
                          const uint32_t* leaf_first, const uint32_t* leaf_count, uint32_t nprims,
                          const float* prim_vertices, const uint32_t* prim_face, atr_octree** out) try {
    if (nnodes <= 0 || !bounds || !children || !leaf_first || !leaf_count || !out) return ATR_E_INVALID;
    if (nprims && (!prim_vertices || !prim_face)) return ATR_E_INVALID;
    std::unique_ptr<atr_octree> own(new (std::nothrow) atr_octree());
    atr_octree* t = own.get();
    if (!t) return ATR_E_NOMEM;
    HostTree& T = t->t;
    T.nnodes = nnodes;
    T.bounds.assign(bounds, bounds + 6 * size_t(nnodes));
    T.children.assign(children, children + nnodes);
    T.leaf_first.assign(leaf_first, leaf_first + nnodes);
    T.leaf_count.assign(leaf_count, leaf_count + nnodes);
    T.prim_vertices.assign(prim_vertices, prim_vertices + 9 * size_t(nprims));
    T.prim_face.assign(prim_face, prim_face + nprims);
    for (int32_t i = 0; i < nnodes; ++i)
        if (children[i] == 0 && uint64_t(leaf_first[i]) + leaf_count[i] > nprims) return ATR_E_INVALID;
    const int rc = octree_finish(T);
    if (rc != ATR_OK) return rc;
    *out = own.release();
    return ATR_OK;
} ATR_ABI_CATCH

void atr_octree_free(atr_octree* t) { delete t; }

int atr_octree_export(const atr_octree* t, float* bounds, int32_t* children, uint32_t* leaf_first,
                      uint32_t* leaf_count, float* prim_vertices, uint32_t* prim_face) try {
    if (!t) return ATR_E_INVALID;
    const HostTree& T = t->t;
    if (bounds) std::memcpy(bounds, T.bounds.data(), T.bounds.size() * sizeof(float));
    if (children) std::memcpy(children, T.children.data(), T.children.size() * sizeof(int32_t));
    if (leaf_first) std::memcpy(leaf_first, T.leaf_first.data(), T.leaf_first.size() * sizeof(uint32_t));
    if (leaf_count) std::memcpy(leaf_count, T.leaf_count.data(), T.leaf_count.size() * sizeof(uint32_t));
    if (prim_vertices) std::memcpy(prim_vertices, T.prim_vertices.data(), T.prim_vertices.size() * sizeof(float));
    if (prim_face) std::memcpy(prim_face, T.prim_face.data(), T.prim_face.size() * sizeof(uint32_t));
    return ATR_OK;
} ATR_ABI_CATCH

int atr_octree_stats(const atr_octree* t, int64_t s[7]) try {
    if (!t || !s) return ATR_E_INVALID;
    octree_stats(t->t, s);
    return ATR_OK;
} ATR_ABI_CATCH

int atr_camera_set(atr_camera* cm, atr_vec3 eye, atr_vec3 facing, int32_t w, int32_t h, int32_t aa,
                   uint32_t spp, int32_t bounces, float h_fov) try {
    if (!cm || w <= 0 || h <= 0) return ATR_E_INVALID;
    camera_set(*cm, mk(eye.x, eye.y, eye.z), mk(facing.x, facing.y, facing.z), w, h, aa, spp, bounces, h_fov);
    return ATR_OK;
} ATR_ABI_CATCH

namespace {
void put_le(uint8_t* p, uint32_t v, int n) {
    for (int i = 0; i < n; ++i) p[i] = uint8_t(v >> (8 * i));
}
}  // namespace

int atr_write_bmp(const uint32_t* pixels, int32_t width, int32_t height, const char* name, char* out_path,
                  int32_t out_cap) try {
    if (!pixels || !name || width <= 0 || height <= 0) return ATR_E_INVALID;
    const size_t len = std::strlen(name);
    if (len + 8 > 1024) return ATR_E_INVALID;  // the reference's new_name[1024]
    const uint64_t bytes = uint64_t(width) * uint64_t(height) * 4;
    if (bytes + 70 > 0x7FFFFFFFull) return ATR_E_INVALID;  // int32 total_file_size
    uint8_t hdr[70] = {};
    hdr[0] = 'B';
    hdr[1] = 'M';
    put_le(hdr + 2, uint32_t(70 + bytes), 4);  // total size; reserved1/2 = 0
    put_le(hdr + 10, 70, 4);                   // pixel offset = 14 + 56
    uint8_t* d = hdr + 14;
    put_le(d + 0, 56, 4);
    put_le(d + 4, uint32_t(width), 4);
    put_le(d + 8, uint32_t(height), 4);  // positive: bottom-up rows, matching row 0 = bottom
    put_le(d + 12, 1, 2);                // planes
    put_le(d + 14, 32, 2);               // bits per pixel
    put_le(d + 16, 3, 4);                // BI_BITFIELDS
    put_le(d + 20, uint32_t(bytes), 4);
    put_le(d + 24, 197, 4);  // ppm x, y as the reference sets them
    put_le(d + 28, 39, 4);
    put_le(d + 40, 0x00FF0000u, 4);  // clr_used/clr_important (32, 36) = 0; R, G, B, A masks
    put_le(d + 44, 0x0000FF00u, 4);
    put_le(d + 48, 0x000000FFu, 4);
    put_le(d + 52, 0, 4);
    std::string path;
    int fd = -1;
    for (uint32_t id = 0; id < 100 && fd < 0; ++id) {  // "%s_%u.bmp" fits len + 8 bytes for ids < 100
        path = std::string(name) + "_" + std::to_string(id) + ".bmp";
        fd = ::open(path.c_str(), O_WRONLY | O_CREAT | O_EXCL, 0644);
        if (fd < 0 && errno != EEXIST) return ATR_E_IO;
    }
    if (fd < 0) return ATR_E_IO;
    bool ok = ::write(fd, hdr, sizeof(hdr)) == ssize_t(sizeof(hdr));
    const uint8_t* src = reinterpret_cast<const uint8_t*>(pixels);
    for (uint64_t off = 0; ok && off < bytes;) {
        const ssize_t w = ::write(fd, src + off, size_t(std::min<uint64_t>(bytes - off, 1ull << 30)));
        ok = w > 0;
        off += ok ? uint64_t(w) : 0;
    }
    ok = (::close(fd) == 0) && ok;
    if (!ok) return ATR_E_IO;
    if (out_path && out_cap > 0) {
        std::strncpy(out_path, path.c_str(), size_t(out_cap) - 1);
        out_path[out_cap - 1] = 0;
    }
    return ATR_OK;
} ATR_ABI_CATCH

// The count-returning entry points are guarded too: their results are never negative, so an
// exception comes back as the negative ATR_E_* code.
int32_t atr_make_tiles(int32_t w, int32_t h, int32_t threads, atr_tile* out, int32_t cap) try {
    return reference_tiles(w, h, threads, out, out ? cap : 0);
} ATR_ABI_CATCH

int32_t atr_make_shard_tiles(int32_t w, int32_t h, int32_t side, int32_t rank, int32_t world, atr_tile* out,
                             int32_t cap) try {
    return shard_tiles(w, h, side, rank, world, out, out ? cap : 0);
} ATR_ABI_CATCH

int32_t atr_balance_shard_tiles(int32_t w, int32_t h, int32_t side, int32_t world, const int64_t* costs,
                                int64_t rank0_extra, int32_t* owner_out) try {
    return balance_shard_tiles(w, h, side, world, costs, rank0_extra, owner_out);
} ATR_ABI_CATCH

// ------------------------------------------------------------------ device engine
int atr_create(int device, atr_ctx** out) try {
    if (!out) return ATR_E_INVALID;
    int n = 0;
    HIPCHK(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return ATR_E_INVALID;
    HIPCHK(hipSetDevice(device));
    atr_ctx* c = new (std::nothrow) atr_ctx();
    if (!c) return ATR_E_NOMEM;
    // released (atr_destroy: whatever was created so far) on every way out but the last, a throw included
    struct Owner { atr_ctx* c; ~Owner() { if (c) atr_destroy(c); } } own{c};
    c->device = device;
    // ATR_CAMERA_PADS=0: this context's primary kernels compute the box growths inline (A/B runs and
    // the tests that compare the two); unset or anything else: they read the per-camera table
    if (const char* v = std::getenv("ATR_CAMERA_PADS")) c->camera_pads = !(v[0] == '0' && v[1] == '\0');
    // ATR_WAVE_CULL=0: this context's primary kernels skip the wave cull of a leaf's clusters (A/B runs
    // and the tests that compare the two); unset or anything else: they cull
    if (const char* v = std::getenv("ATR_WAVE_CULL")) c->wave_cull = !(v[0] == '0' && v[1] == '\0');
    // ATR_FACING_FOLD=0: this context's table holds the unfolded loose growths (A/B runs and tests; same
    // output bits either way)
    if (const char* v = std::getenv("ATR_FACING_FOLD")) c->facing_fold = !(v[0] == '0' && v[1] == '\0');
    // ATR_LEAF_BOX=0: this context builds no table of leaf boxes and its primary passes insert every
    // leaf (A/B runs and tests; same output bits either way)
    if (const char* v = std::getenv("ATR_LEAF_BOX")) c->leaf_box = !(v[0] == '0' && v[1] == '\0');
    // ATR_SKY_PATH=0: no wave of this context's primary kernels takes the sky path (render.hip); the
    // same kernels, and the same output bits either way.
    if (const char* v = std::getenv("ATR_SKY_PATH")) c->sky_path = !(v[0] == '0' && v[1] == '\0');
    const int rc = [&]() -> int {  // any failure below releases what was created (atr_destroy)
        HIPCHK(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
        HIPCHK(hipEventCreate(&c->ev_start));
        HIPCHK(hipEventCreate(&c->ev_stop));
        HIPCHK(hipMalloc(&c->d_error, 16));
        HIPCHK(hipMemset(c->d_error, 0, 16));
        HIPCHK(hipDeviceGetAttribute(&c->ncu, hipDeviceAttributeMultiprocessorCount, device));
        HIPCHK(hipMalloc(&c->tring, kQueueSlots * kTraceBytes));
        HIPCHK(hipMemset(c->tring, 0, kQueueSlots * kTraceBytes));
        for (hipEvent_t& e : c->tev) HIPCHK(hipEventCreate(&e));  // timed: a launch's ev_last
        return ATR_OK;
    }();
    if (rc != ATR_OK) return rc;
    own.c = nullptr;
    *out = c;
    return ATR_OK;
} ATR_ABI_CATCH

void atr_default_tuning(atr_tuning* out) {
    if (out) *out = default_tuning();
}

int atr_set_tuning(atr_ctx* c, const atr_tuning* t) try {
    if (!c || !t) return ATR_E_INVALID;
    if (t->xcd_chunk < 0 || t->xcd_chunk > 4096 || t->frame_rotate < 0 || t->frame_rotate > 1024 ||
        t->hybrid_a < -4096 || t->hybrid_a > 4096 || t->hybrid_b < -4096 || t->hybrid_b > 4096 ||
        t->path_batch_log2 < 12 || t->path_batch_log2 > ATR_MAX_BATCH_LOG2 || t->cluster_size < 1 || t->cluster_size > kMaxClusterSize ||
        t->frame_plan < 0 || t->frame_plan > 1 || (t->path_camera_occ != 0 && (t->path_camera_occ < 5 || t->path_camera_occ > 7)) ||
        (t->path_bounce_occ != 0 && (t->path_bounce_occ < 5 || t->path_bounce_occ > 7)) ||
        (t->primary_occ != 0 && (t->primary_occ < 6 || t->primary_occ > 8)) ||
        (t->path_sort_bits != 0 && (t->path_sort_bits < 2 || t->path_sort_bits > kMaxSortBits)) ||
        t->path_split < 0 || t->path_split > 1)
        return ATR_E_INVALID;
    for (int32_t r : t->reserved)  // room for later knobs: must be zero
        if (r != 0) return ATR_E_INVALID;
    c->tune = *t;
    return ATR_OK;
} ATR_ABI_CATCH

int atr_get_tuning(atr_ctx* c, atr_tuning* out) try {
    if (!c || !out) return ATR_E_INVALID;
    *out = c->tune;
    return ATR_OK;
} ATR_ABI_CATCH

int atr_destroy(atr_ctx* c) try {
    if (!c) return ATR_E_INVALID;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    free_scene(c);
    for (BlockSet& b : c->blocks) {
        if (b.dev.p) (void)hipFree(b.dev.p);
        if (b.dev_tiles.p) (void)hipFree(b.dev_tiles.p);
        if (b.dev_tile.p) (void)hipFree(b.dev_tile.p);
        for (DevBuf* d : {&b.cost, &b.cost_last, &b.plan_work, &b.plan_blocks})
            if (d->p) (void)hipFree(d->p);
        for (hipEvent_t e : b.plan_ev)
            if (e) (void)hipEventDestroy(e);
    }
    for (auto& se : c->stream_ev) (void)hipEventDestroy(se.second);
    for (auto& w : c->path_ws) {
        if (w.mem.p) (void)hipFree(w.mem.p);
        if (w.ev) (void)hipEventDestroy(w.ev);
    }
    if (c->d_error) (void)hipFree(c->d_error);
    for (DevBuf& b : c->prog_blocks)
        if (b.p) (void)hipFree(b.p);
    for (hipEvent_t e : c->prog_ev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->tev)
        if (e) (void)hipEventDestroy(e);
    if (c->tring) (void)hipFree(c->tring);
    if (c->adapt_info) (void)hipFree(c->adapt_info);
    if (c->query_ws.rays.p) (void)hipFree(c->query_ws.rays.p);
    if (c->query_ws.bins.p) (void)hipFree(c->query_ws.bins.p);
    if (c->query_ws.ev) (void)hipEventDestroy(c->query_ws.ev);
    for (DevBuf* d : {&c->tex_ws.mesh, &c->tex_ws.map, &c->tex_ws.aux, &c->img_ws.image, &c->img_ws.flags})
        if (d->p) (void)hipFree(d->p);
    if (c->img_ws.ev) (void)hipEventDestroy(c->img_ws.ev);
    for (DevBuf* d : {&c->dn_ws.color, &c->dn_ws.guides})
        if (d->p) (void)hipFree(d->p);
    if (c->dn_ws.ev) (void)hipEventDestroy(c->dn_ws.ev);
    for (DevBuf* d : {&c->dnv_ws.color, &c->dnv_ws.var, &c->dnv_ws.guides})
        if (d->p) (void)hipFree(d->p);
    if (c->dnv_ws.ev) (void)hipEventDestroy(c->dnv_ws.ev);
    for (atr_ctx::PadSlot& q : c->pad_slot) {
        if (q.mem.p) (void)hipFree(q.mem.p);
        if (q.built) (void)hipEventDestroy(q.built);
        for (auto& se : q.readers) (void)hipEventDestroy(se.second);
    }
    if (c->ev_start) (void)hipEventDestroy(c->ev_start);
    if (c->ev_stop) (void)hipEventDestroy(c->ev_stop);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    if (c->plan_side) (void)hipStreamDestroy(c->plan_side);
    for (int i = 0; i < 2; ++i) {
        if (c->split_stream[i]) (void)hipStreamDestroy(c->split_stream[i]);
        if (c->split_join[i]) (void)hipEventDestroy(c->split_join[i]);
    }
    if (c->split_fork) (void)hipEventDestroy(c->split_fork);
    delete c;
    return ATR_OK;
} ATR_ABI_CATCH

int atr_scene_upload(atr_ctx* c, const atr_material* mats, int32_t nmats, const atr_model* models,
                     int32_t nmodels, const atr_sphere* spheres, int32_t nspheres, const atr_plane* planes,
                     int32_t nplanes) try {
    if (!c || !mats || nmats <= 0 || nmats > kMaxMaterials || nmodels < 0 || nmodels > kMaxModels ||
        (nmodels && !models) || nspheres < 0 || nplanes < 0 || (nspheres && !spheres) || (nplanes && !planes))
        return ATR_E_INVALID;
    for (int32_t i = 0; i < nspheres; ++i)  // shading indexes mats[material] on the device
        if (spheres[i].material < 0 || spheres[i].material >= nmats) return ATR_E_INVALID;
    for (int32_t i = 0; i < nplanes; ++i)
        if (planes[i].material < 0 || planes[i].material >= nmats) return ATR_E_INVALID;
    for (int32_t i = 0; i < nmodels; ++i) {
        const atr_model& md = models[i];
        if (!md.mesh || md.material < 0 || md.material >= nmats) return ATR_E_INVALID;
        if (md.tree) {
            for (int32_t d : md.tree->t.depth)
                if (d >= kMaskLevels) return ATR_E_TREE_DEPTH;
        }
    }
    // Every check of the input that can fail runs before the old scene is freed: a rejected upload
    // leaves the context as it was. The trees are packed here (pack_tree reports ATR_E_TREE_LAYOUT
    // and the index errors of a caller-made tree), the brute-force models' face indices checked.
    std::vector<PackedTree> packed(size_t(nmodels), PackedTree{});
    int64_t total_clusters = 0;
    for (int32_t i = 0; i < nmodels; ++i) {
        const atr_model& md = models[i];
        if (md.tree) {
            if (const int rc = pack_tree(md.tree->t, c->tune.cluster_size, packed[size_t(i)])) return rc;
            total_clusters += int64_t(packed[size_t(i)].nclusters);
            if (total_clusters > int64_t(UINT32_MAX)) return ATR_E_INVALID;
        } else {
            const HostMesh& M = md.mesh->m;
            for (int32_t vi : M.face_v)
                if (vi < 0 || size_t(vi) >= M.vertices.size()) return ATR_E_INVALID;
        }
    }
    SkyRecord sky;  // from the packed trees, before the loop below takes them apart
    sky_record(mats, models, nmodels, nspheres, nplanes, packed, sky);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(wait_all(c));  // kernels on any stream may still read the old scene
    free_scene(c);
    ++c->scene_gen;  // every table of box growths belongs to the old scene now
    c->sky = SkyRecord{};  // the new scene's at the end of a successful upload alone
    DScene S;
    std::memset(&S, 0, sizeof(S));
    for (int32_t i = 0; i < nmats; ++i) {
        const atr_material& m = mats[i];
        S.mats[i] = DMaterial{m.emission.x, m.emission.y, m.emission.z, m.reflection.x, m.reflection.y,
                              m.reflection.z, m.scatter, 0.f};
    }
    S.nmats = nmats;
    S.nmodels = nmodels;
    c->max_nodes = 0;
    c->max_depth = 0;
    c->max_inner = 0;
    c->nclusters = 0;
    c->nleaves = 0;
    c->leaf_clusters.clear();
    float box[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int32_t i = 0; i < nmodels; ++i)
        for (const V3& v : models[i].mesh->m.vertices) {
            box[0] = std::min(box[0], v.x), box[1] = std::min(box[1], v.y), box[2] = std::min(box[2], v.z);
            box[3] = std::max(box[3], v.x), box[4] = std::max(box[4], v.y), box[5] = std::max(box[5], v.z);
        }
    for (int32_t i = 0; i < nspheres; ++i) {  // a sphere's bounds (planes are unbounded: left out)
        const atr_sphere& sp = spheres[i];
        const float r = std::fabs(sp.radius);
        box[0] = std::min(box[0], sp.center.x - r), box[1] = std::min(box[1], sp.center.y - r);
        box[2] = std::min(box[2], sp.center.z - r), box[3] = std::max(box[3], sp.center.x + r);
        box[4] = std::max(box[4], sp.center.y + r), box[5] = std::max(box[5], sp.center.z + r);
    }
    // the queue sort's origin cells span this box; a scene with nothing bounded gets the unit box
    // (not the previous upload's)
    const float unit[6] = {0.f, 0.f, 0.f, 1.f, 1.f, 1.f};
    const bool finite = std::isfinite(box[0]) && std::isfinite(box[1]) && std::isfinite(box[2]) &&
                        std::isfinite(box[3]) && std::isfinite(box[4]) && std::isfinite(box[5]);
    std::memcpy(c->scene_box, finite && box[0] <= box[3] && box[1] <= box[4] && box[2] <= box[5] ? box : unit,
                sizeof(box));
    for (int32_t i = 0; i < nmodels; ++i) {
        const atr_model& md = models[i];
        const HostMesh& M = md.mesh->m;
        DModel& dm = S.models[i];
        std::memset(&dm, 0, sizeof(dm));
        const size_t nf = M.nfaces();
        dm.nfaces = uint32_t(nf);
        dm.material = md.material;
        std::memcpy(dm.aabb, md.surrounding_aabb, sizeof(dm.aabb));
        std::vector<float> shade;
        dm.smooth = shade_records(M, shade);
        void* p = nullptr;
        int rc = dev_upload(c, shade.data(), shade.size() * sizeof(float), &p);
        if (rc) return rc;
        dm.shade = static_cast<const float*>(p);
        if (md.tree) {
            const HostTree& T = md.tree->t;
            // every device table of the model (host_scene.cpp pack_tree), packed above; dropped after this model
            PackedTree PT = std::move(packed[size_t(i)]);
            c->max_depth = std::max(c->max_depth, PT.max_depth);
            auto up = [&](const auto& v, auto*& dst) {
                void* q = nullptr;
                const int r = dev_upload(c, v.data(), v.size() * sizeof(v[0]), &q);
                dst = static_cast<std::remove_reference_t<decltype(dst)>>(q);
                return r;
            };
            dm.ninner = PT.ninner;
            if (dm.ninner > c->max_inner) c->max_inner = dm.ninner;
            if ((rc = up(PT.inner, dm.inner)) || (rc = up(PT.t0, dm.t0)) || (rc = up(PT.t1, dm.t1)) ||
                (rc = up(PT.t2, dm.t2)) || (rc = up(PT.tface, dm.tface)))
                return rc;
            const float4_t* clus = nullptr;
            if ((rc = up(PT.clus, clus))) return rc;
            dm.clus = clus;
            dm.cnrm = reinterpret_cast<const uint4_t*>(dm.clus + 2);
            if ((rc = up(PT.cl_range, dm.cl_range)) || (rc = up(PT.prim, dm.prim))) return rc;
            if (c->nclusters + int64_t(PT.nclusters) > int64_t(UINT32_MAX)) return ATR_E_INVALID;
            dm.cl_base = uint32_t(c->nclusters);  // the model's place in the scene-wide cluster numbering
            dm.cl_count = uint32_t(PT.nclusters);
            if (c->nleaves + int64_t(PT.nleaves) > int64_t(UINT32_MAX)) return ATR_E_INVALID;
            dm.lf_base = uint32_t(c->nleaves);  // and in the scene-wide leaf numbering
            dm.lf_count = uint32_t(PT.nleaves);
            for (size_t k = 0; k < PT.nleaves; ++k) {
                c->leaf_clusters.push_back(dm.cl_base + PT.cl_range[2 * k]);
                c->leaf_clusters.push_back(PT.cl_range[2 * k + 1]);
            }
            c->nleaves += int64_t(PT.nleaves);
            c->nclusters += int64_t(PT.nclusters);
            if ((rc = up(PT.nodes, dm.nodes)) || (rc = up(PT.leaf_range, dm.leaf_range))) return rc;
            if (PT.tris.empty()) PT.tris.resize(1);
            if ((rc = up(PT.tris, dm.tris))) return rc;
            dm.has_tree = 1;
            dm.root_leaf = T.children[0] == 0;
            dm.near_ok = PT.near_ok;
            if (T.nnodes > c->max_nodes) c->max_nodes = T.nnodes;
        } else {  // brute force: face-ordered triangles straight from the mesh (renderer.cpp:61-66)
            std::vector<DTri> tris(nf);
            for (size_t f = 0; f < nf; ++f) {
                float v[9];
                for (int k = 0; k < 3; ++k) {
                    const int32_t vi = M.face_v[3 * f + size_t(k)];
                    if (vi < 0 || size_t(vi) >= M.vertices.size()) return ATR_E_INVALID;
                    const V3 q = M.vertices[size_t(vi)];
                    v[3 * k] = q.x; v[3 * k + 1] = q.y; v[3 * k + 2] = q.z;
                }
                tris[f] = make_tri(v, uint32_t(f));
            }
            if ((rc = dev_upload(c, tris.data(), tris.size() * sizeof(DTri), &p))) return rc;
            dm.tris = static_cast<const DTri*>(p);
            dm.has_tree = 0;
        }
    }
    {
        std::vector<DSphere> sp(size_t(nspheres) + 1);
        for (int32_t i = 0; i < nspheres; ++i)
            sp[size_t(i)] = DSphere{spheres[i].center.x, spheres[i].center.y, spheres[i].center.z,
                                    spheres[i].radius, spheres[i].material, 0, 0, 0};
        std::vector<DPlane> pl(size_t(nplanes) + 1);
        for (int32_t i = 0; i < nplanes; ++i)
            pl[size_t(i)] = DPlane{planes[i].normal.x, planes[i].normal.y, planes[i].normal.z,
                                   planes[i].distance, planes[i].material, 0, 0, 0};
        void* p = nullptr;
        int rc;
        if ((rc = dev_upload(c, sp.data(), sp.size() * sizeof(DSphere), &p))) return rc;
        S.spheres = static_cast<const DSphere*>(p);
        if ((rc = dev_upload(c, pl.data(), pl.size() * sizeof(DPlane), &p))) return rc;
        S.planes = static_cast<const DPlane*>(p);
        S.nspheres = nspheres;
        S.nplanes = nplanes;
        if ((rc = dev_upload(c, &S, sizeof(S), &p))) return rc;
        c->d_scene = static_cast<DScene*>(p);
    }
    c->nmodels = nmodels;
    if (!c->sky_path) sky.on = 0;
    c->sky = sky;
    return ATR_OK;
} ATR_ABI_CATCH

int atr_scene_info(atr_ctx* c, int64_t* bytes, int32_t* max_nodes, int32_t* max_depth) try {
    if (!c) return ATR_E_INVALID;
    if (bytes) *bytes = c->scene_bytes;
    if (max_nodes) *max_nodes = c->max_nodes;
    if (max_depth) *max_depth = c->max_depth;
    return ATR_OK;
} ATR_ABI_CATCH

int atr_workspace_info(atr_ctx* c, int32_t* workspaces, int64_t* bytes) try {
    if (!c) return ATR_E_INVALID;
    int32_t n = 0;
    int64_t b = 0;
    for (const auto& w : c->path_ws)
        if (w.mem.p) { ++n; b += int64_t(w.mem.n); }
    if (workspaces) *workspaces = n;
    if (bytes) *bytes = b;
    return ATR_OK;
} ATR_ABI_CATCH

int64_t atr_render_packed_size(const atr_tile* tiles, int32_t ntiles) try {
    if (!tiles || ntiles <= 0) return 0;
    int32_t W = 0, H = 0;
    for (int32_t i = 0; i < ntiles; ++i) {
        if (tiles[i].max_x + 1 > W) W = tiles[i].max_x + 1;
        if (tiles[i].max_y + 1 > H) H = tiles[i].max_y + 1;
    }
    std::vector<DBlock> b;
    int64_t n = 0;
    build_blocks(tiles, ntiles, W, H, b, n);
    return n;
} ATR_ABI_CATCH

int64_t atr_packed_pixel_map(const atr_tile* tiles, int32_t ntiles, int32_t W, int32_t H, int64_t* out,
                             int64_t cap) try {
    if (ntiles < 0 || (ntiles && !tiles) || W <= 0 || H <= 0) return ATR_E_INVALID;
    std::vector<DBlock> b;
    int64_t n = 0;
    build_blocks(tiles, ntiles, W, H, b, n);
    if (out) {
        int64_t k = 0;
        for (const DBlock& blk : b) {
            const uint64_t m = uint64_t(blk.mask_lo) | (uint64_t(blk.mask_hi) << 32);
            for (int lane = 0; lane < 64; ++lane)
                if ((m >> lane) & 1) {
                    if (k < cap) out[k] = int64_t(blk.y0 + (lane >> 3)) * W + (blk.x0 + (lane & 7));
                    ++k;
                }
        }
    }
    return n;
} ATR_ABI_CATCH

int atr_render_start_ex(atr_ctx* c, const atr_camera* cam, const atr_tile* tiles, int32_t ntiles,
                        const atr_frame* fr, uint64_t seed, void* stream, int32_t variant) try {
    if (!c || !cam || !fr || !fr->framebuffer || ntiles < 0 || (ntiles && !tiles)) return ATR_E_INVALID;
    if (cam->width <= 0 || cam->height <= 0 || cam->width > (1 << 16) || cam->height > (1 << 16)) return ATR_E_INVALID;
    if (fr->layout != ATR_LAYOUT_IMAGE && fr->layout != ATR_LAYOUT_PACKED) return ATR_E_INVALID;
    if (!c->d_scene) return ATR_E_NOSCENE;
    HIPCHK(hipSetDevice(c->device));
    const int wave = auto_sched(variant, *cam);
    if (wave < 0) return ATR_E_INVALID;
    hipStream_t s = static_cast<hipStream_t>(stream);  // NULL = the null stream (HIP convention)
    int rc = ATR_OK;
    BlockSet* bs = get_blocks(c, tiles, ntiles, cam->width, cam->height, rc);
    if (!bs) return rc;
    RenderParams P;
    std::memset(&P, 0, sizeof(P));
    P.cam = *cam;
    P.scene = c->d_scene;
    P.seed = seed;
    P.blocks = static_cast<const DBlock*>(bs->dev.p);
    P.nblocks = int32_t(bs->host.size());
    P.layout = fr->layout;
    P.framebuffer = fr->framebuffer;
    P.hit_face = fr->hit_face;
    P.hit_t = fr->hit_t;
    P.rgb = fr->rgb;
    P.ray_casts = fr->ray_casts;
    P.traced_rays = fr->traced_rays;
    P.error_flag = c->d_error;
    P.counters = nullptr;
    apply_tuning(c, P);
    HIPCHK(call_begin(c, s));
    if ((rc = launch_planned(c, bs, P, wave, s))) return rc;
    // not call_end: launch_planned records the completion itself, ahead of its plan kernels
    HIPCHK(note_launch(c, s, c->ev_last != c->ev_stop));  // a ring event covers it
    c->have_render = true;
    c->last_stream = s;
    c->last_ntiles = ntiles;
    return ATR_OK;
} ATR_ABI_CATCH

// One sample pass of a frame (atray.h): samples [first_sample, first_sample + spp) of every pixel,
// continuing the running sums in sample_sum. PATHS (the camera kernel's ACCUM flavour and
// path_resolve_accum_kernel) or the FLAT cell kernel's ACCUM flavour; never HYBRID's primary
// kernels, also for a one-sample one-bounce pass. The single-frame plan is not applied: a pass is
// a fraction of a frame, and its cost would train the plan of the tile list's full frames.
int atr_render_start_samples(atr_ctx* c, const atr_camera* cam, const atr_tile* tiles, int32_t ntiles,
                             const atr_frame* fr, uint64_t seed, void* stream, int32_t variant,
                             uint32_t first_sample, float* sample_sum) try {
    if (!c || !cam || !fr || !fr->framebuffer || ntiles < 0 || (ntiles && !tiles)) return ATR_E_INVALID;
    if (cam->width <= 0 || cam->height <= 0 || cam->width > (1 << 16) || cam->height > (1 << 16)) return ATR_E_INVALID;
    if (fr->layout != ATR_LAYOUT_IMAGE && fr->layout != ATR_LAYOUT_PACKED) return ATR_E_INVALID;
    // the stream hash shifts the sample index by 40 bits, and float(total) is exact up to 2^24
    if (!sample_sum || cam->samples_per_pixel == 0 ||
        uint64_t(first_sample) + uint64_t(cam->samples_per_pixel) > (uint64_t(1) << 24))
        return ATR_E_INVALID;
    if (variant != ATR_KERNEL_AUTO && variant != ATR_KERNEL_PATHS && variant != ATR_KERNEL_FLAT) return ATR_E_INVALID;
    if (variant == ATR_KERNEL_PATHS && cam->bounce_limit > kMaxPathBounces) return ATR_E_INVALID;
    if (!c->d_scene) return ATR_E_NOSCENE;
    HIPCHK(hipSetDevice(c->device));
    const int sched = variant == ATR_KERNEL_FLAT || cam->bounce_limit > kMaxPathBounces ? sched_of(ATR_KERNEL_FLAT)
                                                                                         : kSchedPaths;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = ATR_OK;
    BlockSet* bs = get_blocks(c, tiles, ntiles, cam->width, cam->height, rc);
    if (!bs) return rc;
    RenderParams P;
    std::memset(&P, 0, sizeof(P));
    P.cam = *cam;
    P.scene = c->d_scene;
    P.seed = seed;
    P.blocks = static_cast<const DBlock*>(bs->dev.p);
    P.nblocks = int32_t(bs->host.size());
    P.layout = fr->layout;
    P.framebuffer = fr->framebuffer;
    P.hit_face = fr->hit_face;
    P.hit_t = fr->hit_t;
    P.rgb = fr->rgb;
    P.ray_casts = fr->ray_casts;
    P.traced_rays = fr->traced_rays;
    P.error_flag = c->d_error;
    P.first_sample = first_sample;
    P.sample_sum = sample_sum;
    apply_tuning(c, P);
    HIPCHK(call_begin(c, s));
    hipEvent_t done = nullptr;
    HIPCHK(launch_render(c, P, sched, s, &done));
    HIPCHK(call_end(c, s, done, ntiles));
    return ATR_OK;
} ATR_ABI_CATCH

// One adaptive sample pass (atray.h): atr_render_start_samples' PATHS route with a
// device-side live list, so only the pixels whose count equals first_sample are traced and
// resolved. The pass's counts go to a slot of the context's info ring, zeroed on the stream first.
int atr_render_start_adaptive(atr_ctx* c, const atr_camera* cam, const atr_tile* tiles, int32_t ntiles,
                              const atr_frame* fr, uint64_t seed, void* stream, int32_t variant,
                              uint32_t first_sample, float* sample_sum, uint32_t* sample_count, float tolerance) try {
    if (!c || !cam || !fr || !fr->framebuffer || ntiles < 0 || (ntiles && !tiles)) return ATR_E_INVALID;
    if (cam->width <= 0 || cam->height <= 0 || cam->width > (1 << 16) || cam->height > (1 << 16)) return ATR_E_INVALID;
    if (fr->layout != ATR_LAYOUT_IMAGE && fr->layout != ATR_LAYOUT_PACKED) return ATR_E_INVALID;
    if (!sample_sum || !sample_count || cam->samples_per_pixel == 0 ||
        uint64_t(first_sample) + uint64_t(cam->samples_per_pixel) > (uint64_t(1) << 24))
        return ATR_E_INVALID;
    if (!(tolerance >= 0.0f) || !std::isfinite(tolerance)) return ATR_E_INVALID;  // also a NaN
    if (variant != ATR_KERNEL_AUTO && variant != ATR_KERNEL_PATHS) return ATR_E_INVALID;
    if (cam->bounce_limit > kMaxPathBounces) return ATR_E_INVALID;
    if (!c->d_scene) return ATR_E_NOSCENE;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = ATR_OK;
    BlockSet* bs = get_blocks(c, tiles, ntiles, cam->width, cam->height, rc);
    if (!bs) return rc;
    if (!c->adapt_info) HIPCHK(hipMalloc(&c->adapt_info, atr_ctx::kAdaptSlots * 4 * sizeof(unsigned long long)));
    RenderParams P;
    std::memset(&P, 0, sizeof(P));
    P.cam = *cam;
    P.scene = c->d_scene;
    P.seed = seed;
    P.blocks = static_cast<const DBlock*>(bs->dev.p);
    P.nblocks = int32_t(bs->host.size());
    P.layout = fr->layout;
    P.framebuffer = fr->framebuffer;
    P.hit_face = fr->hit_face;
    P.hit_t = fr->hit_t;
    P.rgb = fr->rgb;
    P.ray_casts = fr->ray_casts;
    P.traced_rays = fr->traced_rays;
    P.error_flag = c->d_error;
    P.first_sample = first_sample;
    P.sample_sum = sample_sum;
    apply_tuning(c, P);
    PathLive live;
    std::memset(&live, 0, sizeof(live));
    live.count = sample_count;
    live.tolerance = tolerance;
    const int slot = c->adapt_next;
    live.info = c->adapt_info + 4 * slot;
    HIPCHK(call_begin(c, s));
    // the next slot of the ring, never the one atr_render_adaptive_info reads now: a call that
    // fails below (no workspace) has touched nothing the caller can see
    HIPCHK(hipMemsetAsync(live.info, 0, 4 * sizeof(unsigned long long), s));
    hipEvent_t done = nullptr;
    HIPCHK(launch_render(c, P, kSchedPaths, s, &done, &live));
    c->adapt_next = (slot + 1) % atr_ctx::kAdaptSlots;
    c->adapt_last = slot;
    HIPCHK(call_end(c, s, done, ntiles));
    return ATR_OK;
} ATR_ABI_CATCH

// A batch of the caller's rays (atray.h): with an order, the batch's keys, the bin
// scan and the key order (query.hip, paths.hip); then the persistent query launch. The traced rays
// go through a set of the ring, as a render's do (launch_render). Shared by atr_trace_rays and
// atr_occluded_rays (occlusion.hip): `launch` gets the batch, its order, the claim
// counter and the ring's counters in a QueryParams and enqueues the query's own kernel.
extern "C++" {  // a template
namespace {
// Argument domains the query calls share (atray.h). The stream hash shifts the sample index by 40
// bits, and float(first_sample + nsamples) is exact up to 2^24; the path queues carry the stream
// index, base + item, in 32 bits.
bool sample_range_ok(int32_t nsamples, uint32_t first_sample) {
    return nsamples >= 1 && nsamples <= 65536 && uint64_t(first_sample) + uint64_t(nsamples) <= (uint64_t(1) << 24);
}
bool stream_base_ok(int64_t base, int64_t n) { return base >= 0 && base <= (int64_t(1) << 32) - n; }
bool sort_bits_ok(int32_t bits) { return bits == -1 || bits == 0 || (bits >= 2 && bits <= kMaxSortBits); }
bool bounce_limit_ok(int32_t bl) { return bl >= 1 && bl <= kMaxPathBounces; }

// The argument checks both queries share (atray.h); `out` is the required output.
int query_args(atr_ctx* c, const float* origins, const float* directions, int64_t nrays, const void* out,
               int32_t variant, int32_t sort_bits) {
    if (!c) return ATR_E_INVALID;
    if (nrays < 0 || nrays >= (int64_t(1) << 31)) return ATR_E_INVALID;
    if (nrays > 0 && (!out || !origins || !directions)) return ATR_E_INVALID;
    if (variant != ATR_KERNEL_AUTO && variant != ATR_KERNEL_FLAT && variant != ATR_KERNEL_LANE) return ATR_E_INVALID;
    if (!sort_bits_ok(sort_bits)) return ATR_E_INVALID;
    if (!c->d_scene) return ATR_E_NOSCENE;
    return ATR_OK;
}

template <class Launch>
int query_call(atr_ctx* c, const float* origins, const float* directions, int64_t nrays, int32_t sort_bits,
               void* stream, unsigned long long* traced_out, Launch launch) {
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int32_t bits = clamp_sort_bits(sort_bits < 0 ? c->tune.path_sort_bits : sort_bits);
    const int64_t nbins = bits > 0 ? int64_t(kSortDirs) * kSortDirs << (3 * bits) : 0;
    atr_ctx::QueryWS& ws = c->query_ws;
    if (!ws.ev) HIPCHK(hipEventCreateWithFlags(&ws.ev, hipEventDisableTiming));
    const int64_t need = bits > 0 ? nrays : 0;
    if (!ws.rays.p || ws.cap < need || ws.nbins < nbins) {  // grow: after the last call that used it
        if (ws.used) HIPCHK(hipEventSynchronize(ws.ev));
        int rc;
        if (!ws.rays.p || ws.cap < need) {
            if ((rc = ensure_buf(ws.rays, 256 + size_t(std::max(need, ws.cap)) * 12, false))) return rc;
            ws.cap = std::max(need, ws.cap);
        }
        if (ws.nbins < nbins) {
            const size_t bytes = size_t(nbins) * 8 + size_t(nbins / kSortChunk) * 4;
            ws.nbins = 0;
            if ((rc = ensure_buf(ws.bins, bytes, false))) return rc;
            HIPCHK(hipMemset(ws.bins.p, 0, bytes));
            ws.nbins = nbins;
        }
    }
    if (ws.used && ws.stream != s) HIPCHK(hipStreamWaitEvent(s, ws.ev, 0));
    QueryParams Q;
    std::memset(&Q, 0, sizeof(Q));
    Q.scene = c->d_scene;
    Q.o = origins;
    Q.d = directions;
    Q.n = uint32_t(nrays);
    Q.hyb_a = c->tune.hybrid_a;
    Q.hyb_b = c->tune.hybrid_b;
    Q.error_flag = c->d_error;
    Q.head = static_cast<uint32_t*>(ws.rays.p);
    if (bits > 0) {
        PathSort& so = Q.sort;
        sort_cells(c, bits, so);  // the path engine's cells
        char* rb = static_cast<char*>(ws.rays.p) + 256;
        so.kr = reinterpret_cast<uint2_t*>(rb);
        so.perm = reinterpret_cast<uint32_t*>(rb + size_t(ws.cap) * 8);
        so.hist = static_cast<uint32_t*>(ws.bins.p);
        so.start = so.hist + ws.nbins;
        so.part = so.start + ws.nbins;
    }
    HIPCHK(call_begin(c, s));
    ws.used = true;  // from here on kernels of this call may be in flight on s
    ws.stream = s;
    hipEvent_t done = nullptr;
    int k = -1;
    if (traced_out) HIPCHK(ring_take(c, s, k, Q.traced_rays));  // a zeroed set of 64 spread counters
    HIPCHK(hipMemsetAsync(Q.head, 0, sizeof(uint32_t), s));
    if (bits > 0) HIPCHK(atr_launch_query_sort(Q, c->ncu, s));
    HIPCHK(launch(Q, s));
    if (k >= 0) {
        HIPCHK(atr_launch_traced_finish(Q.traced_rays, traced_out, s));
        HIPCHK(ring_done(c, s, k));
        done = c->tev[k];
    }
    HIPCHK(hipEventRecord(ws.ev, s));
    HIPCHK(call_end(c, s, done));
    return ATR_OK;
}

// The fields a path query's params share with the engine's launch (RadianceParams,
// GatherRadianceParams and ProbeShParams name them alike), from a bound PathParams.
template <class Params>
void bind_path_query(const PathParams& Q, uint32_t first_sample, Params& R) {
    R.scene = Q.scene;
    R.nsamples = Q.cam.samples_per_pixel;
    R.first_sample = first_sample;
    R.bounce_limit = Q.cam.bounce_limit;
    R.hyb_a = Q.hyb_a;
    R.hyb_b = Q.hyb_b;
    R.seed = Q.seed;
    R.q0 = Q.q[0];
    R.cap = Q.cap;
    R.out = Q.out;
    R.ctl = Q.ctl;
    R.sort = Q.sort;
    R.error_flag = Q.error_flag;
}

// The path engine on a caller's items (atray.h): atr_radiance_rays, atr_gather_radiance
// and atr_probe_sh. The call is `units` units of per_unit paths each (groups of 64 rays, points,
// probes), batched the way launch_paths_range batches over cells: a batch is a whole number of units,
// at least one even when per_unit exceeds the tuned batch size, so a unit's paths never straddle two
// batches. Per batch, `set_batch(first unit, units)` sets the range in the call's params R, then the
// batch's reset, `entry`, the engine's own bounce levels and `resolve`. The workspace is obtained
// before anything is enqueued and there is no cell-kernel fallback: the tuned batch size is tried even
// below 2^16 paths, as for an adaptive pass. The traced rays go through a set of the ring, as a
// render's and a query's do.
template <class Params, class SetBatch>
int path_query_call(atr_ctx* c, void* stream, int32_t sort_bits, int32_t bounce_limit, int32_t nsamples,
                    uint32_t first_sample, uint64_t seed, unsigned long long* traced_out, int64_t units,
                    int64_t per_unit, Params& R, SetBatch set_batch,
                    hipError_t (*entry)(const Params&, int, hipStream_t),
                    hipError_t (*resolve)(const Params&, hipStream_t)) {
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    // the order is of the bounce levels' queues: without a second level there is nothing to order
    int32_t bits = clamp_sort_bits(bounce_limit >= 2 ? (sort_bits < 0 ? c->tune.path_sort_bits : sort_bits) : 0);
    atr_ctx::PathWS* ws = nullptr;
    int64_t per_batch = 0;  // units
    HIPCHK(path_batches(c, s, per_unit, units, bounce_limit, std::min(16, c->tune.path_batch_log2), false, bits, ws,
                        per_batch));
    PathParams Q;
    std::memset(&Q, 0, sizeof(Q));
    Q.cam.bounce_limit = bounce_limit;
    Q.cam.samples_per_pixel = uint32_t(nsamples);
    Q.scene = c->d_scene;
    Q.seed = seed;
    Q.error_flag = c->d_error;
    Q.hyb_a = c->tune.hybrid_a;
    Q.hyb_b = c->tune.hybrid_b;
    bind_path_workspace(c, ws, bits, Q);
    bind_path_query(Q, first_sample, R);
    HIPCHK(call_begin(c, s));
    hipEvent_t done = nullptr;
    int k = -1;
    if (traced_out) {
        HIPCHK(ring_take(c, s, k, Q.traced_rays));
        R.traced_rays = Q.traced_rays;
    }
    for (int64_t u0 = 0; u0 < units; u0 += per_batch) {
        const int64_t nu = std::min<int64_t>(per_batch, units - u0);
        Q.ncells = int32_t(nu);
        set_batch(u0, nu);
        HIPCHK(reset_path_batch(Q, bounce_limit, bits, s));
        HIPCHK(entry(R, c->ncu, s));
        HIPCHK(launch_bounce_levels(c, Q, bounce_limit, bits, s));
        HIPCHK(resolve(R, s));
    }
    if (k >= 0) {
        HIPCHK(atr_launch_traced_finish(Q.traced_rays, traced_out, s));
        HIPCHK(ring_done(c, s, k));
        done = c->tev[k];
    }
    HIPCHK(hipEventRecord(ws->ev, s));
    HIPCHK(call_end(c, s, done));
    return ATR_OK;
}
}  // namespace
}  // extern "C++"

int atr_trace_rays(atr_ctx* c, const float* origins, const float* directions, int64_t nrays, const atr_ray_hits* hits,
                   int32_t variant, int32_t sort_bits, void* stream) try {
    const int rc = query_args(c, origins, directions, nrays, hits, variant, sort_bits);
    if (rc != ATR_OK || nrays == 0) return rc;
    return query_call(c, origins, directions, nrays, sort_bits, stream, hits->traced_rays,
                      [&](QueryParams& Q, hipStream_t s) {
                          Q.t = hits->t;
                          Q.face = hits->face;
                          Q.model = hits->model;
                          Q.uv = hits->uv;
                          Q.kind = hits->kind;
                          Q.material = hits->material;
                          Q.normal = hits->normal;
                          return atr_launch_query(Q, variant == ATR_KERNEL_LANE ? 1 : 0, c->ncu, s);
                      });
} ATR_ABI_CATCH

// An occlusion query (atray.h): the ray query's order and workspace, its own kernel.
int atr_occluded_rays(atr_ctx* c, const float* origins, const float* directions, const float* t_max, int64_t nrays,
                      uint8_t* occluded, unsigned long long* traced_rays, int32_t variant, int32_t sort_bits,
                      void* stream) try {
    const int rc = query_args(c, origins, directions, nrays, occluded, variant, sort_bits);
    if (rc != ATR_OK || nrays == 0) return rc;
    return query_call(c, origins, directions, nrays, sort_bits, stream, traced_rays,
                      [&](QueryParams& Q, hipStream_t s) {
                          OcclParams P;
                          std::memset(&P, 0, sizeof(P));
                          P.scene = Q.scene;
                          P.o = Q.o;
                          P.d = Q.d;
                          P.tmax = t_max;
                          P.n = Q.n;
                          P.out = occluded;
                          P.traced_rays = Q.traced_rays;
                          P.error_flag = Q.error_flag;
                          P.head = Q.head;
                          P.perm = Q.sort.bits > 0 ? Q.sort.perm : nullptr;
                          return atr_launch_occlusion(P, variant == ATR_KERNEL_LANE ? 1 : 0, c->ncu, s);
                      });
} ATR_ABI_CATCH

// A hemisphere gather (atray.h): the queries' claim counter, ring set and hand-over
// between streams (query_call without an order), its own kernel; the per-point outputs are zeroed on
// the stream first, inside the timed range.
int atr_gather_occlusion(atr_ctx* c, const float* points, const float* normals, const float* t_max, int64_t npoints,
                         int32_t nsamples, uint32_t first_sample, int64_t point_base, uint64_t seed,
                         const atr_gather_out* out, int32_t variant, void* stream) try {
    if (!c) return ATR_E_INVALID;
    if (npoints < 0 || !sample_range_ok(nsamples, first_sample)) return ATR_E_INVALID;
    if (point_base < 0 || npoints > (int64_t(1) << 39) || point_base > (int64_t(1) << 39) - npoints) return ATR_E_INVALID;
    if (npoints >= (int64_t(1) << 31) || npoints * int64_t(nsamples) >= (int64_t(1) << 31)) return ATR_E_INVALID;
    if (npoints > 0 && (!out || !points || !normals)) return ATR_E_INVALID;
    if (variant != ATR_KERNEL_AUTO && variant != ATR_KERNEL_FLAT && variant != ATR_KERNEL_LANE) return ATR_E_INVALID;
    if (!c->d_scene) return ATR_E_NOSCENE;
    if (npoints == 0) return ATR_OK;
    const uint32_t words = (uint32_t(nsamples) + 31u) / 32u;
    return query_call(c, nullptr, nullptr, npoints * int64_t(nsamples), 0, stream, out->traced_rays,
                      [&](QueryParams& Q, hipStream_t s) -> hipError_t {
                          GatherParams P;
                          std::memset(&P, 0, sizeof(P));
                          P.scene = Q.scene;
                          P.p = points;
                          P.nrm = normals;
                          P.tmax = t_max;
                          P.n = Q.n;
                          P.nsamples = uint32_t(nsamples);
                          P.first_sample = first_sample;
                          P.words = words;
                          P.point_base = point_base;
                          P.seed = seed;
                          P.visible = out->visible;
                          P.occluded = out->occluded;
                          P.mask = out->mask;
                          P.dirs = out->dirs;
                          P.traced_rays = Q.traced_rays;
                          P.error_flag = Q.error_flag;
                          P.head = Q.head;
                          hipError_t e = hipSuccess;
                          const size_t per = size_t(npoints) * sizeof(uint32_t);
                          if (P.visible && (e = hipMemsetAsync(P.visible, 0, per, s)) != hipSuccess) return e;
                          if (P.occluded && (e = hipMemsetAsync(P.occluded, 0, per, s)) != hipSuccess) return e;
                          if (P.mask && (e = hipMemsetAsync(P.mask, 0, per * words, s)) != hipSuccess) return e;
                          return atr_launch_gather(P, variant == ATR_KERNEL_LANE ? 1 : 0, c->ncu, s);
                      });
} ATR_ABI_CATCH

// The gather's sampler on the host (atray.h): the kernel's own functions (engine.h), compiled with the
// library's -ffp-contract=off. No device, no context.
int atr_gather_directions(const float* normals, int64_t npoints, int32_t nsamples, uint32_t first_sample,
                          int64_t point_base, uint64_t seed, float* dirs_out, uint8_t* traced_out) try {
    if (npoints < 0 || !sample_range_ok(nsamples, first_sample)) return ATR_E_INVALID;
    if (point_base < 0 || npoints > (int64_t(1) << 39) || point_base > (int64_t(1) << 39) - npoints) return ATR_E_INVALID;
    if (npoints >= (int64_t(1) << 31) || npoints * int64_t(nsamples) >= (int64_t(1) << 31)) return ATR_E_INVALID;
    if (npoints > 0 && !normals) return ATR_E_INVALID;
    const V3 zero = mk(0.f, 0.f, 0.f);
    for (int64_t i = 0; i < npoints; ++i) {
        const V3 n = mk(normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]);
        const bool nok = ray_ok(zero, n);  // the direction test on the normal
        for (int32_t s = 0; s < nsamples; ++s) {
            const int64_t k = i * nsamples + s;
            V3 d = zero;
            bool traced = false;
            if (nok) {
                d = gather_dir(seed, point_base + i, first_sample + uint32_t(s), n);
                traced = ray_ok(zero, d) && dot(d, n) > 0.0f;
            }
            if (dirs_out) {
                dirs_out[3 * k] = d.x;
                dirs_out[3 * k + 1] = d.y;
                dirs_out[3 * k + 2] = d.z;
            }
            if (traced_out) traced_out[k] = traced ? 1 : 0;
        }
    }
    return ATR_OK;
} ATR_ABI_CATCH

// Path-traced radiance along the caller's rays (atray.h): path_query_call over groups of
// 64 rays, the last of which may be short, with the entry kernel and the per-ray resolve of
// radiance.hip.
int atr_radiance_rays(atr_ctx* c, const float* origins, const float* directions, int64_t nrays, int32_t nsamples,
                      uint32_t first_sample, int64_t ray_base, int32_t bounce_limit, uint64_t seed,
                      const atr_radiance_out* out, int32_t sort_bits, void* stream) try {
    if (!c) return ATR_E_INVALID;
    if (nrays < 0 || nrays >= (int64_t(1) << 31) || !sample_range_ok(nsamples, first_sample)) return ATR_E_INVALID;
    if (!stream_base_ok(ray_base, nrays) || !bounce_limit_ok(bounce_limit) || !sort_bits_ok(sort_bits))
        return ATR_E_INVALID;
    if (nrays > 0 && (!out || !origins || !directions)) return ATR_E_INVALID;
    if (out && first_sample > 0 && !out->sum) return ATR_E_INVALID;
    if (nrays > 0 && !out->rgb && !out->sum && !out->ray_casts && !out->invalid && !out->traced_rays)
        return ATR_E_INVALID;
    if (!c->d_scene) return ATR_E_NOSCENE;
    if (nrays == 0) return ATR_OK;
    RadianceParams R;
    std::memset(&R, 0, sizeof(R));
    R.o = origins;
    R.d = directions;
    R.ray_base = ray_base;
    R.rgb = out->rgb;
    R.sum = out->sum;
    R.ray_casts = out->ray_casts;
    R.invalid = out->invalid;
    return path_query_call(c, stream, sort_bits, bounce_limit, nsamples, first_sample, seed, out->traced_rays,
                           (nrays + 63) / 64, 64 * int64_t(nsamples), R,
                           [&](int64_t g0, int64_t ng) {  // no batch crosses a group
                               R.ray0 = uint32_t(g0 * 64);
                               R.n = uint32_t(std::min<int64_t>(ng * 64, nrays - g0 * 64));
                           },
                           atr_launch_radiance_entry, atr_launch_radiance_resolve);
} ATR_ABI_CATCH

// Hemisphere radiance gathered on the device (atray.h): path_query_call over points, so
// a point's samples never straddle two batches and the resolve sums them in sample order in one
// launch, with the entry kernel and the per-point resolve of gather_radiance.hip.
int atr_gather_radiance(atr_ctx* c, const float* points, const float* normals, int64_t npoints, int32_t nsamples,
                        uint32_t first_sample, int64_t point_base, int32_t bounce_limit, uint64_t seed,
                        const atr_gather_radiance_out* out, int32_t sort_bits, void* stream) try {
    if (!c) return ATR_E_INVALID;
    if (npoints < 0 || npoints >= (int64_t(1) << 31) || !sample_range_ok(nsamples, first_sample)) return ATR_E_INVALID;
    if (npoints * int64_t(nsamples) >= (int64_t(1) << 31)) return ATR_E_INVALID;
    if (!stream_base_ok(point_base, npoints) || !bounce_limit_ok(bounce_limit) || !sort_bits_ok(sort_bits))
        return ATR_E_INVALID;
    if (npoints > 0 && (!out || !points || !normals)) return ATR_E_INVALID;
    if (out && first_sample > 0 && (!out->sum || !out->samples)) return ATR_E_INVALID;
    if (npoints > 0 && !out->rgb && !out->sum && !out->samples && !out->ray_casts && !out->invalid &&
        !out->sample_rgb && !out->dirs && !out->traced_rays)
        return ATR_E_INVALID;
    if (!c->d_scene) return ATR_E_NOSCENE;
    if (npoints == 0) return ATR_OK;
    GatherRadianceParams R;
    std::memset(&R, 0, sizeof(R));
    R.p = points;
    R.nrm = normals;
    R.point_base = point_base;
    R.rgb = out->rgb;
    R.sum = out->sum;
    R.samples = out->samples;
    R.ray_casts = out->ray_casts;
    R.invalid = out->invalid;
    R.sample_rgb = out->sample_rgb;
    R.dirs = out->dirs;
    return path_query_call(c, stream, sort_bits, bounce_limit, nsamples, first_sample, seed, out->traced_rays,
                           npoints, nsamples, R,
                           [&](int64_t p0, int64_t np) {  // whole points
                               R.point0 = uint32_t(p0);
                               R.npoints = uint32_t(np);
                               R.n = uint32_t(np * int64_t(nsamples));
                           },
                           atr_launch_gather_radiance_entry, atr_launch_gather_radiance_resolve);
} ATR_ABI_CATCH

// Light probes as L2 spherical harmonics (atray.h): path_query_call over probes, points
// without normals, with the entry kernel and the per-probe resolve of probe_sh.hip.
int atr_probe_sh(atr_ctx* c, const float* points, int64_t npoints, int32_t nsamples, uint32_t first_sample,
                 int64_t point_base, int32_t bounce_limit, uint64_t seed, const atr_probe_sh_out* out,
                 int32_t sort_bits, void* stream) try {
    if (!c) return ATR_E_INVALID;
    if (npoints < 0 || npoints >= (int64_t(1) << 31) || !sample_range_ok(nsamples, first_sample)) return ATR_E_INVALID;
    if (npoints * int64_t(nsamples) >= (int64_t(1) << 31)) return ATR_E_INVALID;
    if (!stream_base_ok(point_base, npoints) || !bounce_limit_ok(bounce_limit) || !sort_bits_ok(sort_bits))
        return ATR_E_INVALID;
    if (npoints > 0 && (!out || !points)) return ATR_E_INVALID;
    if (out && first_sample > 0 && !out->sum) return ATR_E_INVALID;
    if (npoints > 0 && !out->sh && !out->sum && !out->ray_casts && !out->invalid && !out->sample_rgb && !out->dirs &&
        !out->traced_rays)
        return ATR_E_INVALID;
    if (!c->d_scene) return ATR_E_NOSCENE;
    if (npoints == 0) return ATR_OK;
    ProbeShParams R;
    std::memset(&R, 0, sizeof(R));
    R.p = points;
    R.point_base = point_base;
    R.sh = out->sh;
    R.sum = out->sum;
    R.ray_casts = out->ray_casts;
    R.invalid = out->invalid;
    R.sample_rgb = out->sample_rgb;
    R.dirs = out->dirs;
    return path_query_call(c, stream, sort_bits, bounce_limit, nsamples, first_sample, seed, out->traced_rays,
                           npoints, nsamples, R,
                           [&](int64_t p0, int64_t np) {  // whole probes
                               R.point0 = uint32_t(p0);
                               R.npoints = uint32_t(np);
                               R.n = uint32_t(np * int64_t(nsamples));
                           },
                           atr_launch_probe_sh_entry, atr_launch_probe_sh_resolve);
} ATR_ABI_CATCH

// The probes' sampler and basis on the host (atray.h): the kernels' own functions (engine.h), compiled
// with the library's -ffp-contract=off. No device, no context.
int atr_probe_directions(int64_t npoints, int32_t nsamples, uint32_t first_sample, int64_t point_base, uint64_t seed,
                         float* dirs_out, uint8_t* tries_out) try {
    if (npoints < 0 || npoints >= (int64_t(1) << 31) || !sample_range_ok(nsamples, first_sample)) return ATR_E_INVALID;
    if (npoints * int64_t(nsamples) >= (int64_t(1) << 31)) return ATR_E_INVALID;
    if (!stream_base_ok(point_base, npoints)) return ATR_E_INVALID;
    for (int64_t i = 0; i < npoints; ++i) {
        for (int32_t s = 0; s < nsamples; ++s) {
            const int64_t k = i * nsamples + s;
            uint64_t st, stream;
            uint32_t tries;
            const V3 d = probe_dir_state(seed, point_base + i, first_sample + uint32_t(s), st, stream, tries);
            if (dirs_out) {
                dirs_out[3 * k] = d.x;
                dirs_out[3 * k + 1] = d.y;
                dirs_out[3 * k + 2] = d.z;
            }
            if (tries_out) tries_out[k] = uint8_t(tries);
        }
    }
    return ATR_OK;
} ATR_ABI_CATCH

int atr_sh_basis(const float* dirs, int64_t n, float* basis_out) try {
    if (n < 0 || (n > 0 && (!dirs || !basis_out))) return ATR_E_INVALID;
    for (int64_t i = 0; i < n; ++i) sh_basis(mk(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]), basis_out + 9 * i);
    return ATR_OK;
} ATR_ABI_CATCH

int atr_render_adaptive_info(atr_ctx* c, int64_t info_out[4]) try {
    if (!c || !info_out || c->adapt_last < 0) return ATR_E_INVALID;
    HIPCHK(hipSetDevice(c->device));
    unsigned long long v[4];
    HIPCHK(hipMemcpy(v, c->adapt_info + 4 * c->adapt_last, sizeof(v), hipMemcpyDeviceToHost));
    info_out[0] = int64_t(v[0]);
    info_out[1] = int64_t(v[1]);
    info_out[2] = int64_t(v[2]);
    info_out[3] = int64_t(v[0]) - int64_t(v[3]);  // live at the start minus the newly converged
    return ATR_OK;
} ATR_ABI_CATCH

namespace {
// Frames in flight in one launch (atr_render_start_frames / _cameras): ncams == 1 -> every frame
// renders cams[0]; ncams == nframes -> frame f renders cams[f].
int start_frames(atr_ctx* c, const atr_camera* cams, int32_t ncams, const atr_tile* tiles, int32_t ntiles,
                 const atr_frame* fr, int32_t nframes, int64_t frame_stride, uint64_t seed, void* stream,
                 int32_t variant) {
    if (!c || !cams || !fr || !fr->framebuffer || ntiles < 0 || (ntiles && !tiles) || nframes < 1 || nframes > 64)
        return ATR_E_INVALID;
    if (ncams != 1 && (ncams != nframes || nframes > kMaxFrameCams)) return ATR_E_INVALID;
    const atr_camera* cam = cams;
    if (cam->width <= 0 || cam->height <= 0 || cam->width > (1 << 16) || cam->height > (1 << 16)) return ATR_E_INVALID;
    for (int32_t f = 1; f < ncams; ++f) {  // one block list and one kernel specialization per launch
        const atr_camera& q = cams[f];
        if (q.width != cam->width || q.height != cam->height || q.samples_per_pixel != cam->samples_per_pixel ||
            q.bounce_limit != cam->bounce_limit || q.anti_aliasing != cam->anti_aliasing)
            return ATR_E_INVALID;
    }
    if (fr->layout != ATR_LAYOUT_IMAGE && fr->layout != ATR_LAYOUT_PACKED) return ATR_E_INVALID;
    const int sched = auto_sched(variant, *cam);
    if (sched < 0) return ATR_E_INVALID;
    if (!c->d_scene) return ATR_E_NOSCENE;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = ATR_OK;
    BlockSet* bs = get_blocks(c, tiles, ntiles, cam->width, cam->height, rc);
    if (!bs) return rc;
    const int64_t per_frame = fr->layout == ATR_LAYOUT_IMAGE ? int64_t(cam->width) * cam->height : bs->packed_pixels;
    if (nframes > 1 && frame_stride < per_frame) return ATR_E_INVALID;
    const int32_t nb = int32_t(bs->host.size());
    if (int64_t(nb) * nframes > (int64_t(1) << 30)) return ATR_E_INVALID;
    RenderParams P;
    std::memset(&P, 0, sizeof(P));
    P.cam = *cam;
    P.scene = c->d_scene;
    P.seed = seed;
    P.blocks = static_cast<const DBlock*>(bs->dev.p);
    P.layout = fr->layout;
    P.framebuffer = fr->framebuffer;
    P.hit_face = fr->hit_face;
    P.hit_t = fr->hit_t;
    P.rgb = fr->rgb;
    P.ray_casts = fr->ray_casts;
    P.traced_rays = fr->traced_rays;
    P.error_flag = c->d_error;
    apply_tuning(c, P);
    HIPCHK(call_begin(c, s));
    if (nframes == 1) {  // one frame: the single-frame plan applies
        P.nblocks = nb;
        P.frame_stride = frame_stride;
        if ((rc = launch_planned(c, bs, P, sched, s))) return rc;
    } else {  // one launch over frames x blocks (render_kernel / paths: fidx)
        P.nblocks = nb * nframes;
        P.frame_blocks = nb;
        P.frame_stride = frame_stride;
        P.frame_rotate = c->tune.frame_rotate;
        if (ncams > 1) {
            P.nfcam = ncams;
            for (int32_t f = 0; f < ncams; ++f) P.fcam[f] = cams[f];
        }
        hipEvent_t done = nullptr;
        HIPCHK(launch_render(c, P, sched, s, &done));
        HIPCHK(record_stop(c, s, done));
    }
    // not call_end: launch_planned records the completion itself, ahead of its plan kernels
    HIPCHK(note_launch(c, s, c->ev_last != c->ev_stop));  // a ring event covers it
    c->have_render = true;
    c->last_stream = s;
    c->last_ntiles = ntiles;
    return ATR_OK;
}
}  // namespace

int atr_render_start_frames(atr_ctx* c, const atr_camera* cam, const atr_tile* tiles, int32_t ntiles,
                            const atr_frame* fr, int32_t nframes, int64_t frame_stride, uint64_t seed, void* stream,
                            int32_t variant) try {
    return start_frames(c, cam, 1, tiles, ntiles, fr, nframes, frame_stride, seed, stream, variant);
} ATR_ABI_CATCH

int atr_render_start_cameras(atr_ctx* c, const atr_camera* cams, int32_t nframes, const atr_tile* tiles,
                             int32_t ntiles, const atr_frame* fr, int64_t frame_stride, uint64_t seed, void* stream,
                             int32_t variant) try {
    return start_frames(c, cams, nframes, tiles, ntiles, fr, nframes, frame_stride, seed, stream, variant);
} ATR_ABI_CATCH

#ifdef ATR_DIAG
int atr_render_wave_trace(atr_ctx* c, const atr_camera* cam, const atr_tile* tiles, int32_t ntiles,
                          uint64_t seed, int32_t variant, uint64_t* out, int64_t cap, int64_t* nblocks) try {
    if (!c || !cam || !nblocks || ntiles < 0 || (ntiles && !tiles)) return ATR_E_INVALID;
    if (!c->d_scene) return ATR_E_NOSCENE;
    HIPCHK(hipSetDevice(c->device));
    int rc = ATR_OK;
    BlockSet* bs = get_blocks(c, tiles, ntiles, cam->width, cam->height, rc);
    if (!bs) return rc;
    const size_t nb = bs->host.size();
    *nblocks = int64_t(nb);
    if (!out || cap < int64_t(3 * nb)) return ATR_OK;  // size query
    DevTmp fb;
    DevTmp tr;
    HIPCHK(hipMalloc(&fb.p, std::max<size_t>(1, size_t(bs->packed_pixels)) * 4));
    HIPCHK(hipMalloc(&tr.p, std::max<size_t>(1, 3 * nb) * sizeof(unsigned long long)));
    RenderParams P;
    std::memset(&P, 0, sizeof(P));
    P.cam = *cam;
    P.scene = c->d_scene;
    P.seed = seed;
    P.blocks = static_cast<const DBlock*>(bs->dev.p);
    P.nblocks = int32_t(nb);
    P.layout = ATR_LAYOUT_PACKED;
    P.framebuffer = static_cast<uint32_t*>(fb.p);
    P.error_flag = c->d_error;
    P.wave_trace = static_cast<unsigned long long*>(tr.p);
    apply_tuning(c, P);
    const int ts = sched_of(variant);  // per-cell trace: 8x8-cell schedules only
    // through launch_kernels, as a product launch goes: HYBRID's primaries read the camera's table
    HIPCHK(launch_kernels(c, P, ts < 0 || ts == kSchedPaths ? 7 : ts, nullptr));
    HIPCHK(hipDeviceSynchronize());
    if (nb) HIPCHK(hipMemcpy(out, tr.p, 3 * nb * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return ATR_OK;
} ATR_ABI_CATCH

#endif  // ATR_DIAG

// One instrumented (COUNT) render; h = the 16 device counters (render.hip: [0..9] work counters,
// [10..15] phase clocks, zero unless built with -DATR_PHASE_CLOCKS).
constexpr int kCounterSlots = 35;
static int count_launch(atr_ctx* c, const atr_camera* cam, const atr_tile* tiles, int32_t ntiles, uint64_t seed,
                        int32_t variant, unsigned long long h[kCounterSlots]) {
    if (!c || !cam || ntiles < 0 || (ntiles && !tiles)) return ATR_E_INVALID;
    if (!c->d_scene) return ATR_E_NOSCENE;
    HIPCHK(hipSetDevice(c->device));
    int rc = ATR_OK;
    BlockSet* bs = get_blocks(c, tiles, ntiles, cam->width, cam->height, rc);
    if (!bs) return rc;
    DevTmp fb;
    DevTmp ctr;
    HIPCHK(hipMalloc(&fb.p, size_t(cam->width) * size_t(cam->height) * 4));
    HIPCHK(hipMalloc(&ctr.p, kCounterSlots * sizeof(unsigned long long)));
    HIPCHK(hipMemset(ctr.p, 0, kCounterSlots * sizeof(unsigned long long)));
    RenderParams P;
    std::memset(&P, 0, sizeof(P));
    P.cam = *cam;
    P.scene = c->d_scene;
    P.seed = seed;
    P.blocks = static_cast<const DBlock*>(bs->dev.p);
    P.nblocks = int32_t(bs->host.size());
    P.layout = ATR_LAYOUT_IMAGE;
    P.framebuffer = static_cast<uint32_t*>(fb.p);
    P.error_flag = c->d_error;
    P.counters = static_cast<unsigned long long*>(ctr.p);
    apply_tuning(c, P);  // the product's HYBRID thresholds (the counts do not depend on them, the clocks do)
    const int sc = auto_sched(variant, *cam);
    if (sc < 0) return ATR_E_INVALID;
    HIPCHK(launch_render(c, P, sc, nullptr));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(h, ctr.p, kCounterSlots * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return ATR_OK;
}

int atr_render_counters(atr_ctx* c, const atr_camera* cam, const atr_tile* tiles, int32_t ntiles,
                        uint64_t seed, int32_t variant, int64_t out[10]) try {
    if (!out) return ATR_E_INVALID;
    unsigned long long h[kCounterSlots];
    const int rc = count_launch(c, cam, tiles, ntiles, seed, variant, h);
    if (rc != ATR_OK) return rc;
    for (int k = 0; k < 10; ++k) out[k] = int64_t(h[k]);
    return ATR_OK;
} ATR_ABI_CATCH

int atr_render_cull_counters(atr_ctx* c, const atr_camera* cam, const atr_tile* tiles, int32_t ntiles,
                             uint64_t seed, int32_t variant, int64_t out[5]) try {
    if (!out) return ATR_E_INVALID;
    unsigned long long h[kCounterSlots];
    const int rc = count_launch(c, cam, tiles, ntiles, seed, variant, h);
    if (rc != ATR_OK) return rc;
    out[4] = int64_t(h[29]);  // cluster tests run per ray (lane level)
    out[0] = int64_t(h[27]);  // (wave, cluster) pairs culled against the direction hull
    out[1] = int64_t(h[28]);  // wave-level iterations of the lane-private cluster loop
    out[2] = int64_t(h[25]);  // dealt rounds
    out[3] = int64_t(h[26]);  // dealt items
    return ATR_OK;
} ATR_ABI_CATCH

int atr_render_fold_counters(atr_ctx* c, const atr_camera* cam, const atr_tile* tiles, int32_t ntiles,
                             uint64_t seed, int32_t variant, int64_t out[2]) try {
    if (!out) return ATR_E_INVALID;
    unsigned long long h[kCounterSlots];
    const int rc = count_launch(c, cam, tiles, ntiles, seed, variant, h);
    if (rc != ATR_OK) return rc;
    out[0] = int64_t(h[30]);  // (ray, cluster) pairs past the unfolded loose box that fail the folded one
    out[1] = int64_t(h[31]);  // the primitives screened for them
    return ATR_OK;
} ATR_ABI_CATCH

int atr_render_leaf_box_counters(atr_ctx* c, const atr_camera* cam, const atr_tile* tiles, int32_t ntiles,
                                 uint64_t seed, int32_t variant, int64_t out[2]) try {
    if (!out) return ATR_E_INVALID;
    unsigned long long h[kCounterSlots];
    const int rc = count_launch(c, cam, tiles, ntiles, seed, variant, h);
    if (rc != ATR_OK) return rc;
    out[0] = int64_t(h[32]);  // (lane, leaf) visits whose leaf the product passes leave out
    out[1] = int64_t(h[33]);  // those of them in which a cluster passed the table's loose box
    return ATR_OK;
} ATR_ABI_CATCH

int atr_render_sky_cells(atr_ctx* c, const atr_camera* cam, const atr_tile* tiles, int32_t ntiles, uint64_t seed,
                         int32_t variant, int64_t* out) try {
    if (!out) return ATR_E_INVALID;
    unsigned long long h[kCounterSlots];
    const int rc = count_launch(c, cam, tiles, ntiles, seed, variant, h);
    if (rc != ATR_OK) return rc;
    *out = int64_t(h[34]);  // waves whose active lanes all fail every model's first test
    return ATR_OK;
} ATR_ABI_CATCH

static void sky_record_out(const SkyRecord& sky, int32_t info[4], float values[28]) {
    info[0] = sky.on, info[1] = sky.n, info[2] = int32_t(sky.brute), info[3] = int32_t(sky.face);
    values[0] = sky.t;
    std::memcpy(values + 1, sky.em, sizeof(sky.em));
    std::memcpy(values + 4, sky.box, sizeof(sky.box));
}

int atr_scene_sky_record(atr_ctx* c, int32_t info[4], float values[28]) try {
    if (!c || !info || !values) return ATR_E_INVALID;
    if (!c->d_scene) return ATR_E_NOSCENE;
    sky_record_out(c->sky, info, values);
    return ATR_OK;
} ATR_ABI_CATCH

int atr_sky_record_host(const atr_material* mats, int32_t nmats, const atr_model* models, int32_t nmodels,
                        int32_t nspheres, int32_t nplanes, int32_t info[4], float values[28]) try {
    if (!mats || nmats <= 0 || nmats > kMaxMaterials || nmodels < 0 || nmodels > kMaxModels || (nmodels && !models) ||
        nspheres < 0 || nplanes < 0 || !info || !values)
        return ATR_E_INVALID;
    std::vector<PackedTree> packed(size_t(nmodels), PackedTree{});
    for (int32_t i = 0; i < nmodels; ++i) {
        if (!models[i].mesh) return ATR_E_INVALID;
        if (!models[i].tree) continue;
        if (const int rc = pack_tree(models[i].tree->t, default_tuning().cluster_size, packed[size_t(i)])) return rc;
    }
    SkyRecord sky;
    sky_record(mats, models, nmodels, nspheres, nplanes, packed, sky);
    sky_record_out(sky, info, values);
    return ATR_OK;
} ATR_ABI_CATCH

int64_t atr_camera_leaf_boxes_row(atr_ctx* c, const float eye[3], float* row, int32_t* ranges, int64_t cap) try {
    if (!c || !eye || cap < 0) return ATR_E_INVALID;
    if (!c->d_scene) return ATR_E_NOSCENE;
    const int64_t n = c->nleaves, ncl = c->nclusters;
    if (n <= 0 || ncl <= 0) return 0;
    if (n > int64_t(1) << 30 || ncl > int64_t(1) << 30) return ATR_E_INVALID;
    if (!row || cap < n) return n;  // the count alone
    HIPCHK(hipSetDevice(c->device));
    PadEyes eyes;
    std::memset(&eyes, 0, sizeof(eyes));
    eyes.e[0][0] = eye[0], eyes.e[0][1] = eye[1], eyes.e[0][2] = eye[2];
    // as bind_pads builds a one-camera launch's table: the row of growths, then the boxes from it
    DevTmp d_tab, d_box;
    HIPCHK(hipMalloc(&d_tab.p, size_t(ncl) * sizeof(float2_t)));
    HIPCHK(hipMalloc(&d_box.p, size_t(n) * 2 * sizeof(float4_t)));
    HIPCHK(hipMemset(d_tab.p, 0, size_t(ncl) * sizeof(float2_t)));
    HIPCHK(hipMemset(d_box.p, 0, size_t(n) * 2 * sizeof(float4_t)));
    HIPCHK(atr_launch_camera_pads(c->d_scene, eyes, 1, int32_t(ncl), c->facing_fold, 0, static_cast<float2_t*>(d_tab.p),
                                  nullptr, nullptr, nullptr, nullptr));
    HIPCHK(atr_launch_camera_leaf_boxes(c->d_scene, eyes, 1, int32_t(ncl), 0, static_cast<const float2_t*>(d_tab.p),
                                        int32_t(n), static_cast<float4_t*>(d_box.p), nullptr));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(row, d_box.p, size_t(n) * 2 * sizeof(float4_t), hipMemcpyDeviceToHost));
    if (ranges) std::memcpy(ranges, c->leaf_clusters.data(), size_t(n) * 2 * sizeof(uint32_t));
    return n;
} ATR_ABI_CATCH

int64_t atr_camera_pads_row(atr_ctx* c, const float eye[3], float* row, float* boxes, float* edges, int64_t cap) try {
    if (!c || !eye || cap < 0) return ATR_E_INVALID;
    if (!c->d_scene) return ATR_E_NOSCENE;
    const int64_t n = c->nclusters;
    if (n <= 0 || n > int64_t(1) << 30) return n <= 0 ? 0 : ATR_E_INVALID;
    if (!row || cap < n) return n;  // the count alone
    HIPCHK(hipSetDevice(c->device));
    PadEyes eyes;
    std::memset(&eyes, 0, sizeof(eyes));
    eyes.e[0][0] = eye[0], eyes.e[0][1] = eye[1], eyes.e[0][2] = eye[2];
    // the table row as bind_pads builds it for a one-camera launch of this context (the same kernel,
    // the same arguments), with the fold kernel's side outputs; without the fold the row comes from
    // camera_pads_kernel and the side outputs from a second launch into a table of their own
    const size_t nn = size_t(n);
    DevTmp d_tab, d_info, d_box, d_edge, d_tab2;
    HIPCHK(hipMalloc(&d_tab.p, nn * sizeof(float2_t)));
    HIPCHK(hipMalloc(&d_info.p, nn * sizeof(float2_t)));
    HIPCHK(hipMalloc(&d_box.p, nn * 3 * sizeof(float4_t)));
    HIPCHK(hipMalloc(&d_edge.p, nn * 96 * sizeof(float)));
    HIPCHK(hipMemset(d_tab.p, 0, nn * sizeof(float2_t)));  // (an entry no tree model covers reads back as 0)
    HIPCHK(hipMemset(d_info.p, 0, nn * sizeof(float2_t)));
    HIPCHK(hipMemset(d_box.p, 0, nn * 3 * sizeof(float4_t)));
    HIPCHK(hipMemset(d_edge.p, 0, nn * 96 * sizeof(float)));
    float2_t* const tab = static_cast<float2_t*>(d_tab.p);
    float2_t* const info = static_cast<float2_t*>(d_info.p);
    float4_t* const box = static_cast<float4_t*>(d_box.p);
    float* const edge = static_cast<float*>(d_edge.p);
    if (c->facing_fold) {
        HIPCHK(atr_launch_camera_pads(c->d_scene, eyes, 1, int32_t(n), 1, 0, tab, info, box, edge, nullptr));
    } else {
        HIPCHK(atr_launch_camera_pads(c->d_scene, eyes, 1, int32_t(n), 0, 0, tab, nullptr, nullptr, nullptr, nullptr));
        HIPCHK(hipMalloc(&d_tab2.p, nn * sizeof(float2_t)));
        HIPCHK(atr_launch_camera_pads(c->d_scene, eyes, 1, int32_t(n), 0, 0, static_cast<float2_t*>(d_tab2.p), info, box,
                                      edge, nullptr));
    }
    HIPCHK(hipDeviceSynchronize());
    std::vector<float2_t> h_tab(nn), h_info(nn);
    HIPCHK(hipMemcpy(h_tab.data(), d_tab.p, nn * sizeof(float2_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(h_info.data(), d_info.p, nn * sizeof(float2_t), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < nn; ++i) {
        row[4 * i] = h_tab[i].x, row[4 * i + 1] = h_tab[i].y;
        row[4 * i + 2] = h_info[i].x, row[4 * i + 3] = h_info[i].y;
    }
    if (boxes) HIPCHK(hipMemcpy(boxes, d_box.p, nn * 3 * sizeof(float4_t), hipMemcpyDeviceToHost));
    if (edges) HIPCHK(hipMemcpy(edges, d_edge.p, nn * 96 * sizeof(float), hipMemcpyDeviceToHost));
    return n;
} ATR_ABI_CATCH

#ifdef ATR_DIAG
int atr_render_phase_clocks(atr_ctx* c, const atr_camera* cam, const atr_tile* tiles, int32_t ntiles,
                            uint64_t seed, int32_t variant, int64_t out[6]) try {
    if (!out) return ATR_E_INVALID;
    unsigned long long h[kCounterSlots];
    const int rc = count_launch(c, cam, tiles, ntiles, seed, variant, h);
    if (rc != ATR_OK) return rc;
    for (int k = 0; k < 6; ++k) out[k] = int64_t(h[10 + k]);
    return ATR_OK;
} ATR_ABI_CATCH

int atr_render_path_counters(atr_ctx* c, const atr_camera* cam, const atr_tile* tiles, int32_t ntiles,
                             uint64_t seed, int32_t variant, int64_t out[6]) try {
    if (!out) return ATR_E_INVALID;
    unsigned long long h[kCounterSlots];
    const int rc = count_launch(c, cam, tiles, ntiles, seed, variant, h);
    if (rc != ATR_OK) return rc;
    for (int k = 0; k < 6; ++k) out[k] = int64_t(h[16 + k]);
    return ATR_OK;
} ATR_ABI_CATCH

int atr_render_simd_counters(atr_ctx* c, const atr_camera* cam, const atr_tile* tiles, int32_t ntiles,
                             uint64_t seed, int32_t variant, int64_t out[7]) try {
    if (!out) return ATR_E_INVALID;
    unsigned long long h[kCounterSlots];
    const int rc = count_launch(c, cam, tiles, ntiles, seed, variant, h);
    if (rc != ATR_OK) return rc;
    out[0] = int64_t(h[22]);  // candidate-loop wave iterations
    out[1] = int64_t(h[2]);   // full triangle tests (lane level)
    for (int k = 0; k < 4; ++k) out[2 + k] = int64_t(h[23 + k]);
    out[6] = int64_t(h[0]);   // traced rays
    return ATR_OK;
} ATR_ABI_CATCH

#endif  // ATR_DIAG

int atr_render_tile_costs(atr_ctx* c, const atr_camera* cam, const atr_tile* tiles, int32_t ntiles,
                          uint64_t seed, int64_t* cost_out) try {
    if (!c || !cam || (ntiles && (!tiles || !cost_out)) || ntiles < 0) return ATR_E_INVALID;
    if (!c->d_scene) return ATR_E_NOSCENE;
    HIPCHK(hipSetDevice(c->device));
    int rc = ATR_OK;
    BlockSet* bs = get_blocks(c, tiles, ntiles, cam->width, cam->height, rc);
    if (!bs) return rc;
    const size_t nb = bs->host.size();
    DevTmp fb;
    DevTmp cost;
    HIPCHK(hipMalloc(&fb.p, std::max<size_t>(1, size_t(bs->packed_pixels)) * 4));
    HIPCHK(hipMalloc(&cost.p, std::max<size_t>(1, nb) * sizeof(unsigned long long)));
    HIPCHK(hipMemset(cost.p, 0, std::max<size_t>(1, nb) * sizeof(unsigned long long)));  // atomically added
    RenderParams P;
    std::memset(&P, 0, sizeof(P));
    P.cam = *cam;
    P.scene = c->d_scene;
    P.seed = seed;
    P.blocks = static_cast<const DBlock*>(bs->dev.p);
    P.nblocks = int32_t(nb);
    P.layout = ATR_LAYOUT_PACKED;
    P.framebuffer = static_cast<uint32_t*>(fb.p);
    P.error_flag = c->d_error;
    P.block_cost = static_cast<unsigned long long*>(cost.p);
    apply_tuning(c, P);
    HIPCHK(launch_render(c, P, auto_sched(ATR_KERNEL_AUTO, *cam), nullptr));  // per-cell clocks, AUTO's kernels
    HIPCHK(hipDeviceSynchronize());
    std::vector<unsigned long long> h(nb);
    if (nb) HIPCHK(hipMemcpy(h.data(), cost.p, nb * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    // a block (one 8x8 cell of the image grid) belongs to the first tile (list order) that
    // overlaps it: paint cell owners in list order, first writer wins
    const int32_t cw = (cam->width + 7) / 8, chh = (cam->height + 7) / 8;
    std::vector<int32_t> owner(size_t(cw) * size_t(chh), -1);
    for (int32_t t = 0; t < ntiles; ++t) {
        const atr_tile& T = tiles[t];
        const int32_t x0 = std::max(0, T.min_x) / 8, x1 = std::min(cam->width - 1, T.max_x) / 8;
        const int32_t y0 = std::max(0, T.min_y) / 8, y1 = std::min(cam->height - 1, T.max_y) / 8;
        for (int32_t cy = y0; cy <= y1; ++cy)
            for (int32_t cx = x0; cx <= x1; ++cx) {
                int32_t& o = owner[size_t(cy) * size_t(cw) + size_t(cx)];
                if (o < 0) o = t;
            }
    }
    for (int32_t t = 0; t < ntiles; ++t) cost_out[t] = 0;
    for (size_t k = 0; k < nb; ++k) {
        const DBlock& b = bs->host[k];
        const int32_t o = owner[size_t(b.y0 / 8) * size_t(cw) + size_t(b.x0 / 8)];
        if (o >= 0) cost_out[o] += int64_t(h[k]);
    }
    return ATR_OK;
} ATR_ABI_CATCH

int atr_render_start_progressive(atr_ctx* c, const atr_camera* cam, const atr_tile* tiles, int32_t ntiles,
                                 const atr_frame* fr, uint64_t seed, void* stream, int32_t variant,
                                 int32_t tiles_per_launch) try {
    if (!c || !cam || !fr || !fr->framebuffer || ntiles < 0 || (ntiles && !tiles) || tiles_per_launch < 1)
        return ATR_E_INVALID;
    if (cam->width <= 0 || cam->height <= 0 || cam->width > (1 << 16) || cam->height > (1 << 16)) return ATR_E_INVALID;
    if (fr->layout != ATR_LAYOUT_IMAGE) return ATR_E_INVALID;
    const int sched = auto_sched(variant, *cam);
    if (sched < 0) return ATR_E_INVALID;
    if (!c->d_scene) return ATR_E_NOSCENE;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIPCHK(wait_all(c));  // group buffers are reused
    const int32_t ngroups = (ntiles + tiles_per_launch - 1) / tiles_per_launch;
    while (int32_t(c->prog_ev.size()) < ngroups) {
        hipEvent_t e;
        HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        c->prog_ev.push_back(e);
    }
    c->prog_blocks.resize(std::max<size_t>(c->prog_blocks.size(), size_t(ngroups)));
    c->prog_end.assign(size_t(ngroups), 0);
    RenderParams P;
    std::memset(&P, 0, sizeof(P));
    P.cam = *cam;
    P.scene = c->d_scene;
    P.seed = seed;
    P.layout = ATR_LAYOUT_IMAGE;
    P.framebuffer = fr->framebuffer;
    P.hit_face = fr->hit_face;
    P.hit_t = fr->hit_t;
    P.rgb = fr->rgb;
    P.ray_casts = fr->ray_casts;
    P.traced_rays = fr->traced_rays;
    P.error_flag = c->d_error;
    apply_tuning(c, P);
    HIPCHK(hipEventRecord(c->ev_start, s));
    for (int32_t g = 0; g < ngroups; ++g) {
        const int32_t a = g * tiles_per_launch, e = std::min(ntiles, a + tiles_per_launch);
        std::vector<DBlock> blocks;
        int64_t npix = 0;
        build_blocks(tiles, e, cam->width, cam->height, blocks, npix, a);  // tiles[a, e), new pixels
        DevBuf& d = c->prog_blocks[size_t(g)];
        const size_t need = std::max<size_t>(blocks.size() * sizeof(DBlock), 32);
        if (d.n < need) {
            if (d.p) HIPCHK(hipFree(d.p));
            d = DevBuf();
            HIPCHK(hipMalloc(&d.p, need));
            d.n = need;
        }
        if (!blocks.empty()) HIPCHK(hipMemcpy(d.p, blocks.data(), blocks.size() * sizeof(DBlock), hipMemcpyHostToDevice));
        P.blocks = static_cast<const DBlock*>(d.p);
        P.nblocks = int32_t(blocks.size());
        HIPCHK(launch_render(c, P, sched, s));
        HIPCHK(hipEventRecord(c->prog_ev[size_t(g)], s));
        c->prog_end[size_t(g)] = e;
    }
    // not call_begin / call_end: a progressive render leaves prog_active set
    HIPCHK(record_stop(c, s, nullptr));
    HIPCHK(note_launch(c, s));
    c->have_render = true;
    c->prog_active = true;
    c->last_stream = s;
    c->last_ntiles = ntiles;
    return ATR_OK;
} ATR_ABI_CATCH

int atr_render_start(atr_ctx* c, const atr_camera* cam, const atr_tile* tiles, int32_t ntiles,
                     const atr_frame* fr, uint64_t seed, void* stream) try {
    return atr_render_start_ex(c, cam, tiles, ntiles, fr, seed, stream, ATR_KERNEL_AUTO);
} ATR_ABI_CATCH

// ------------------------------------------------------------------ lightmap texels (texels.hip)
namespace {
// Timing events of one synchronous call, destroyed on every exit path.
struct EventSet {
    hipEvent_t e[6] = {};
    ~EventSet() {
        for (hipEvent_t x : e)
            if (x) (void)hipEventDestroy(x);
    }
};
size_t round_up(size_t n, size_t a) { return (n + a - 1) / a * a; }
}  // namespace

int atr_mesh_texels(atr_ctx* c, const atr_mesh* mesh, int32_t width, int32_t height, int32_t flags, int64_t cap,
                    const atr_texels_out* out, int64_t* ncovered, float ms_out[2]) try {
    if (!c || !mesh || !out || !ncovered) return ATR_E_INVALID;
    const HostMesh& M = mesh->m;
    const size_t nf = M.nfaces();
    if (M.texcoords.empty() || M.face_t.size() != 3 * nf || nf >= size_t(kTexelNone)) return ATR_E_INVALID;
    if (width < 1 || width > kTexelMaxSide || height < 1 || height > kTexelMaxSide || cap < 0 ||
        (flags & ~int32_t(ATR_TEXELS_FLIP)))
        return ATR_E_INVALID;
    const auto t0 = std::chrono::steady_clock::now();
    HIPCHK(hipSetDevice(c->device));
    // the workspaces are rewritten below: nothing of this context may still be in flight on them
    HIPCHK(wait_all(c));
    atr_ctx::TexelWS& ws = c->tex_ws;
    // the mesh as the kernels read it, in one buffer: the one-model scene of scene_finish, its per-face
    // 9 floats (the upload's own, shade_records), vertices, texcoords, the two index arrays
    DScene S;
    std::memset(&S, 0, sizeof(S));
    std::vector<float> shade;
    S.nmodels = 1;
    S.models[0].smooth = shade_records(M, shade);
    S.models[0].nfaces = uint32_t(nf);
    const size_t at_shade = round_up(sizeof(DScene), 256), at_v = at_shade + round_up(shade.size() * 4, 256);
    const size_t at_t = at_v + round_up(M.vertices.size() * sizeof(V3) + 16, 256);
    const size_t at_fv = at_t + round_up(M.texcoords.size() * sizeof(V3), 256);
    const size_t at_ft = at_fv + round_up(3 * nf * 4 + 16, 256), total = at_ft + round_up(3 * nf * 4 + 16, 256);
    int rc;
    if ((rc = ensure_buf(ws.mesh, total, false))) return rc;
    char* const base = static_cast<char*>(ws.mesh.p);
    S.models[0].shade = reinterpret_cast<const float*>(base + at_shade);
    std::vector<char> host(total, 0);
    std::memcpy(host.data(), &S, sizeof(S));
    std::memcpy(host.data() + at_shade, shade.data(), shade.size() * 4);
    if (!M.vertices.empty()) std::memcpy(host.data() + at_v, M.vertices.data(), M.vertices.size() * sizeof(V3));
    std::memcpy(host.data() + at_t, M.texcoords.data(), M.texcoords.size() * sizeof(V3));
    if (nf) {
        std::memcpy(host.data() + at_fv, M.face_v.data(), 3 * nf * 4);
        std::memcpy(host.data() + at_ft, M.face_t.data(), 3 * nf * 4);
    }
    HIPCHK(hipMemcpy(base, host.data(), total, hipMemcpyHostToDevice));
    const size_t ntexels = size_t(width) * size_t(height);
    const size_t nblocks = (ntexels + kTexelScanBlock - 1) / kTexelScanBlock;
    const size_t map_bytes = nblocks * kTexelScanBlock * sizeof(uint32_t);
    if ((rc = ensure_buf(ws.map, map_bytes, false))) return rc;
    // aux: [0] the list's length; [4 ..] nblocks + 1 sums; then the list, one u32 per face at most
    if ((rc = ensure_buf(ws.aux, (4 + nblocks + 4 + nf + 4) * sizeof(uint32_t), false))) return rc;
    TexelParams P;
    std::memset(&P, 0, sizeof(P));
    P.mesh.shade = reinterpret_cast<const DScene*>(base);
    P.mesh.vertices = reinterpret_cast<const float*>(base + at_v);
    P.mesh.texcoords = reinterpret_cast<const float*>(base + at_t);
    P.mesh.face_v = reinterpret_cast<const int32_t*>(base + at_fv);
    P.mesh.face_t = reinterpret_cast<const int32_t*>(base + at_ft);
    P.mesh.nvertices = uint32_t(M.vertices.size());
    P.mesh.ntexcoords = uint32_t(M.texcoords.size());
    P.mesh.nfaces = uint32_t(nf);
    P.width = width;
    P.height = height;
    P.flip = (flags & ATR_TEXELS_FLIP) ? 1 : 0;
    P.map = static_cast<uint32_t*>(ws.map.p);
    P.nbig = static_cast<uint32_t*>(ws.aux.p);
    P.sums = P.nbig + 4;
    P.nblocks = uint32_t(nblocks);
    P.big = P.sums + nblocks + 4;
    P.out = *out;
    hipStream_t s = c->own_stream;
    EventSet ev;
    for (hipEvent_t& e : ev.e) HIPCHK(hipEventCreate(&e));
    // coverage: the faces with small boxes, and the list of the others
    HIPCHK(hipEventRecord(ev.e[0], s));
    HIPCHK(hipMemsetAsync(P.map, 0xFF, map_bytes, s));
    HIPCHK(hipMemsetAsync(P.nbig, 0, 4 * sizeof(uint32_t), s));
    HIPCHK(atr_launch_texel_classify(P, s));
    HIPCHK(hipEventRecord(ev.e[1], s));
    HIPCHK(note_launch(c, s));
    uint32_t nbig = 0, count = 0;
    HIPCHK(hipMemcpyAsync(&nbig, P.nbig, sizeof(nbig), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (nbig > nf) return -(1000 + int(hipErrorUnknown));
    // the listed faces, then the slot scan
    HIPCHK(hipEventRecord(ev.e[2], s));
    HIPCHK(atr_launch_texel_big(P, nbig, s));
    HIPCHK(atr_launch_texel_scan(P, s));
    HIPCHK(hipEventRecord(ev.e[3], s));
    HIPCHK(note_launch(c, s));
    HIPCHK(hipMemcpyAsync(&count, P.sums + nblocks, sizeof(count), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *ncovered = int64_t(count);
    // slots, and the samples when the caller's arrays hold them
    P.fill = cap >= int64_t(count) ? 1 : 0;
    const bool write = out->slot || (P.fill && count > 0 && (out->texel || out->face || out->bary || out->point || out->normal));
    HIPCHK(hipEventRecord(ev.e[4], s));
    if (write) HIPCHK(atr_launch_texel_write(P, s));
    HIPCHK(hipEventRecord(ev.e[5], s));
    HIPCHK(note_launch(c, s));
    HIPCHK(hipStreamSynchronize(s));
    if (ms_out) {
        float dev = 0.f;
        for (int k = 0; k < 6; k += 2) {
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, ev.e[k], ev.e[k + 1]));
            dev += ms;
        }
        ms_out[0] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        ms_out[1] = dev;
    }
    return ATR_OK;
} ATR_ABI_CATCH

int atr_texels_to_image(atr_ctx* c, const float* values, const int32_t* texel, int64_t ncovered, int32_t width,
                        int32_t height, int32_t passes, const float fill[3], float* image, void* stream) try {
    if (!c || !image || !fill) return ATR_E_INVALID;
    if (width < 1 || width > kTexelMaxSide || height < 1 || height > kTexelMaxSide || passes < 0 ||
        passes > kTexelMaxPasses)
        return ATR_E_INVALID;
    const int64_t ntexels = int64_t(width) * int64_t(height);
    if (ncovered < 0 || ncovered > ntexels || (ncovered > 0 && (!values || !texel))) return ATR_E_INVALID;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);  // NULL = the null stream (HIP convention)
    atr_ctx::ImageWS& ws = c->img_ws;
    if (!ws.ev) HIPCHK(hipEventCreateWithFlags(&ws.ev, hipEventDisableTiming));
    const size_t flag_stride = round_up(size_t(ntexels), 256);
    const size_t need_image = passes > 0 ? size_t(ntexels) * 3 * sizeof(float) : 0;
    if (!ws.flags.p || ws.flags.n < 2 * flag_stride || ws.image.n < need_image) {  // grow: after the last call that used it
        if (ws.used) HIPCHK(hipEventSynchronize(ws.ev));
        int rc;
        if ((rc = ensure_buf(ws.flags, 2 * flag_stride, false))) return rc;
        if (need_image && (rc = ensure_buf(ws.image, need_image, false))) return rc;
    }
    if (ws.used && ws.stream != s) HIPCHK(hipStreamWaitEvent(s, ws.ev, 0));
    HIPCHK(call_begin(c, s));
    ws.used = true;  // from here on kernels of this call may be in flight on s
    ws.stream = s;
    // the passes alternate between the caller's image and the workspace's; the last one writes the caller's
    float* img[2] = {image, static_cast<float*>(ws.image.p)};
    uint8_t* flg[2] = {static_cast<uint8_t*>(ws.flags.p), static_cast<uint8_t*>(ws.flags.p) + flag_stride};
    int cur = passes & 1;
    HIPCHK(hipMemsetAsync(flg[0], 0, size_t(ntexels), s));
    HIPCHK(atr_launch_texel_scatter(values, texel, ncovered, ntexels, img[cur], flg[0], s));
    TexelImageParams P;
    std::memset(&P, 0, sizeof(P));
    P.width = width;
    P.height = height;
    std::memcpy(P.fill, fill, sizeof(P.fill));
    for (int p = 0; p < passes; ++p) {
        P.last = p == passes - 1 ? 1 : 0;
        P.src = img[cur];
        P.src_flag = flg[p & 1];
        P.dst = img[cur ^ 1];
        P.dst_flag = flg[(p & 1) ^ 1];
        HIPCHK(atr_launch_texel_dilate(P, s));
        cur ^= 1;
    }
    if (passes == 0) {
        P.last = 1;
        P.src_flag = flg[0];
        P.dst = image;
        HIPCHK(atr_launch_texel_fill(P, s));
    }
    HIPCHK(hipEventRecord(ws.ev, s));
    HIPCHK(call_end(c, s, nullptr));
    return ATR_OK;
} ATR_ABI_CATCH

void atr_default_denoise_params(atr_denoise_params* out) {
    if (!out) return;
    std::memset(out, 0, sizeof(*out));
    out->passes = 5;
    out->sigma_color = 0.01f;  // the scale of the renderer's noise at 1-4 spp, not of its signal
    out->sigma_position = 0.0f;
    out->normal_power_log2 = 5;
}

int atr_denoise(atr_ctx* c, const float* color, const atr_denoise_guides* guides, int32_t width, int32_t height,
                const atr_denoise_params* params, float* out, uint32_t* framebuffer, void* stream) try {
    if (!c || !params || !color || (!out && !framebuffer)) return ATR_E_INVALID;
    if (width < 1 || width > kDenoiseMaxSide || height < 1 || height > kDenoiseMaxSide) return ATR_E_INVALID;
    const atr_denoise_params& dp = *params;
    if (dp.passes < 1 || dp.passes > kDenoiseMaxPasses || dp.normal_power_log2 < 0 ||
        dp.normal_power_log2 > kDenoiseMaxNormalPower)
        return ATR_E_INVALID;
    if (!(dp.sigma_color >= 0.0f) || !std::isfinite(dp.sigma_color) || !(dp.sigma_position >= 0.0f) ||
        !std::isfinite(dp.sigma_position))
        return ATR_E_INVALID;
    for (int32_t r : dp.reserved)
        if (r) return ATR_E_INVALID;
    const atr_denoise_guides none = {nullptr, nullptr, nullptr};
    const atr_denoise_guides& g = guides ? *guides : none;
    const bool colour_on = dp.sigma_color > 0.0f, position_on = g.position && dp.sigma_position > 0.0f;
    // the per-pass constants, in f32 (atray.h); a term that is on needs every one of them finite and > 0
    float kc[kDenoiseMaxPasses], kp[kDenoiseMaxPasses];
    for (int p = 0; p < dp.passes; ++p) {
        const float sf = float(1 << p);
        const float sc = dp.sigma_color / sf, sp = dp.sigma_position * sf;
        kc[p] = colour_on ? 1.0f / (sc * sc) : 0.0f;
        kp[p] = position_on ? 1.0f / (sp * sp) : 0.0f;
        if (colour_on && !(std::isfinite(kc[p]) && kc[p] > 0.0f)) return ATR_E_INVALID;
        if (position_on && !(std::isfinite(kp[p]) && kp[p] > 0.0f)) return ATR_E_INVALID;
    }
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);  // NULL = the null stream (HIP convention)
    atr_ctx::DenoiseWS& ws = c->dn_ws;
    if (!ws.ev) HIPCHK(hipEventCreateWithFlags(&ws.ev, hipEventDisableTiming));
    const size_t npix = size_t(width) * size_t(height), image = npix * sizeof(float4_t);
    const size_t need_guides = image * ((g.normal ? 1 : 0) + (g.position ? 1 : 0));
    if (!ws.color.p || ws.color.n < 2 * image || ws.guides.n < need_guides) {  // grow: after the last call that used it
        if (ws.used) HIPCHK(hipEventSynchronize(ws.ev));
        int rc;
        if ((rc = ensure_buf(ws.color, 2 * image, false))) return rc;
        if (need_guides && (rc = ensure_buf(ws.guides, need_guides, false))) return rc;
    }
    if (ws.used && ws.stream != s) HIPCHK(hipStreamWaitEvent(s, ws.ev, 0));
    HIPCHK(call_begin(c, s));
    ws.used = true;  // from here on kernels of this call may be in flight on s
    ws.stream = s;
    float4_t* img[2] = {static_cast<float4_t*>(ws.color.p), static_cast<float4_t*>(ws.color.p) + npix};
    float4_t* rec = static_cast<float4_t*>(ws.guides.p);
    DenoisePack K;
    std::memset(&K, 0, sizeof(K));
    K.color = color;
    K.normal = g.normal;
    K.position = g.position;
    K.ident = g.ident;
    K.npixels = int64_t(npix);
    K.color4 = img[0];
    K.normal4 = g.normal ? rec : nullptr;
    K.position4 = g.position ? rec + (g.normal ? npix : 0) : nullptr;
    HIPCHK(atr_launch_denoise_pack(K, s));
    DenoisePass P;
    std::memset(&P, 0, sizeof(P));
    P.width = width;
    P.height = height;
    P.normal_power = dp.normal_power_log2;
    P.normal4 = K.normal4;
    P.position4 = K.position4;
    for (int p = 0; p < dp.passes; ++p) {
        const bool last = p == dp.passes - 1;
        P.step = 1 << p;
        P.kc = kc[p];
        P.kp = kp[p];
        P.src = img[p & 1];
        P.dst = last ? nullptr : img[(p & 1) ^ 1];
        P.out = last ? out : nullptr;
        P.framebuffer = last ? framebuffer : nullptr;
        HIPCHK(atr_launch_denoise_pass(P, g.normal != nullptr, position_on, colour_on, s));
    }
    HIPCHK(hipEventRecord(ws.ev, s));
    HIPCHK(call_end(c, s, nullptr));
    return ATR_OK;
} ATR_ABI_CATCH

void atr_default_denoise_variance_params(atr_denoise_variance_params* out) {
    if (!out) return;
    std::memset(out, 0, sizeof(*out));
    out->passes = 3;  // the grid point with the lowest worst-seed error under its conditions
    out->sigma_luminance = 8.0f;
    out->luminance_floor = 1e-4f;
    out->sigma_position = 0.0f;
    out->normal_power_log2 = 5;
    out->spatial_below = 4;
}

// atr_denoise_variance's argument rules (atray.h), host only: the structs are read, no DEVICE pointer is followed.
int atr_denoise_variance_check(const float* color, const float* variance, const atr_denoise_guides* guides,
                               const float* moments, const uint32_t* length, int32_t width, int32_t height,
                               const atr_denoise_variance_params* params, const float* out, const float* variance_out,
                               const uint32_t* framebuffer) try {
    (void)variance_out;  // optional, and it may be `variance` itself
    if (!params || !color || !variance || (!out && !framebuffer)) return ATR_E_INVALID;
    if (!moments != !length) return ATR_E_INVALID;
    if (width < 1 || width > kDenoiseMaxSide || height < 1 || height > kDenoiseMaxSide) return ATR_E_INVALID;
    const atr_denoise_variance_params& dp = *params;
    if (dp.passes < 1 || dp.passes > kDenoiseMaxPasses || dp.normal_power_log2 < 0 ||
        dp.normal_power_log2 > kDenoiseMaxNormalPower || dp.spatial_below < 0 ||
        dp.spatial_below > kDenoiseVarMaxSpatialBelow)
        return ATR_E_INVALID;
    if (!(dp.sigma_luminance >= 0.0f) || !std::isfinite(dp.sigma_luminance) || !(dp.luminance_floor > 0.0f) ||
        !std::isfinite(dp.luminance_floor) || !(dp.sigma_position >= 0.0f) || !std::isfinite(dp.sigma_position))
        return ATR_E_INVALID;
    for (int32_t r : dp.reserved)
        if (r) return ATR_E_INVALID;
    if (guides && guides->position && dp.sigma_position > 0.0f)  // the position term is on
        for (int p = 0; p < dp.passes; ++p) {
            const float sp = dp.sigma_position * float(1 << p);
            const float kp = 1.0f / (sp * sp);
            if (!(std::isfinite(kp) && kp > 0.0f)) return ATR_E_INVALID;
        }
    return ATR_OK;
} ATR_ABI_CATCH

int atr_denoise_variance(atr_ctx* c, const float* color, const float* variance, const atr_denoise_guides* guides,
                         const float* moments, const uint32_t* length, int32_t width, int32_t height,
                         const atr_denoise_variance_params* params, float* out, float* variance_out,
                         uint32_t* framebuffer, void* stream) try {
    if (!c) return ATR_E_INVALID;
    const int vrc = atr_denoise_variance_check(color, variance, guides, moments, length, width, height, params, out,
                                               variance_out, framebuffer);
    if (vrc) return vrc;
    const atr_denoise_variance_params& dp = *params;
    const atr_denoise_guides none = {nullptr, nullptr, nullptr};
    const atr_denoise_guides& g = guides ? *guides : none;
    const bool luminance_on = dp.sigma_luminance > 0.0f, position_on = g.position && dp.sigma_position > 0.0f;
    const bool estimate_on = moments && dp.spatial_below > 0;
    float kp[kDenoiseMaxPasses];
    for (int p = 0; p < dp.passes; ++p) {
        const float sp = dp.sigma_position * float(1 << p);
        kp[p] = position_on ? 1.0f / (sp * sp) : 0.0f;
    }
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);  // NULL = the null stream (HIP convention)
    atr_ctx::DenoiseVarWS& ws = c->dnv_ws;
    if (!ws.ev) HIPCHK(hipEventCreateWithFlags(&ws.ev, hipEventDisableTiming));
    const size_t npix = size_t(width) * size_t(height), image = npix * sizeof(float4_t), vimage = npix * sizeof(float2_t);
    const size_t need_guides = image * ((g.normal ? 1 : 0) + (g.position ? 1 : 0));
    if (!ws.color.p || ws.color.n < 2 * image || !ws.var.p || ws.var.n < 2 * vimage ||
        ws.guides.n < need_guides) {  // grow: after the last call that used it
        if (ws.used) HIPCHK(hipEventSynchronize(ws.ev));
        int rc;
        if ((rc = ensure_buf(ws.color, 2 * image, false))) return rc;
        if ((rc = ensure_buf(ws.var, 2 * vimage, false))) return rc;
        if (need_guides && (rc = ensure_buf(ws.guides, need_guides, false))) return rc;
    }
    if (ws.used && ws.stream != s) HIPCHK(hipStreamWaitEvent(s, ws.ev, 0));
    HIPCHK(call_begin(c, s));
    ws.used = true;  // from here on kernels of this call may be in flight on s
    ws.stream = s;
    float4_t* img[2] = {static_cast<float4_t*>(ws.color.p), static_cast<float4_t*>(ws.color.p) + npix};
    float2_t* vl[2] = {static_cast<float2_t*>(ws.var.p), static_cast<float2_t*>(ws.var.p) + npix};
    float4_t* rec = static_cast<float4_t*>(ws.guides.p);
    DenoiseVarPack K;
    std::memset(&K, 0, sizeof(K));
    K.color = color;
    K.variance = variance;
    K.normal = g.normal;
    K.position = g.position;
    K.ident = g.ident;
    K.npixels = int64_t(npix);
    K.color4 = img[0];
    K.vl = vl[0];
    K.normal4 = g.normal ? rec : nullptr;
    K.position4 = g.position ? rec + (g.normal ? npix : 0) : nullptr;
    HIPCHK(atr_launch_denoise_variance_pack(K, s));
    if (estimate_on) {
        DenoiseVarEstimate Q;
        std::memset(&Q, 0, sizeof(Q));
        Q.width = width;
        Q.height = height;
        Q.normal_power = dp.normal_power_log2;
        Q.below = uint32_t(dp.spatial_below);
        Q.kp = kp[0];
        Q.fbelow = float(dp.spatial_below);
        Q.color4 = img[0];
        Q.normal4 = K.normal4;
        Q.position4 = K.position4;
        Q.moments = reinterpret_cast<const float2_t*>(moments);
        Q.length = length;
        Q.vl = vl[0];
        HIPCHK(atr_launch_denoise_variance_estimate(Q, g.normal != nullptr, position_on, s));
    }
    DenoiseVarPass P;
    std::memset(&P, 0, sizeof(P));
    P.width = width;
    P.height = height;
    P.normal_power = dp.normal_power_log2;
    P.sigma_luminance = dp.sigma_luminance;
    P.luminance_floor = dp.luminance_floor;
    P.normal4 = K.normal4;
    P.position4 = K.position4;
    for (int p = 0; p < dp.passes; ++p) {
        const bool last = p == dp.passes - 1;
        P.step = 1 << p;
        P.kp = kp[p];
        P.src = img[p & 1];
        P.src_vl = vl[p & 1];
        P.dst = last ? nullptr : img[(p & 1) ^ 1];
        P.dst_vl = last ? nullptr : vl[(p & 1) ^ 1];
        P.out = last ? out : nullptr;
        P.variance_out = last ? variance_out : nullptr;
        P.framebuffer = last ? framebuffer : nullptr;
        HIPCHK(atr_launch_denoise_variance_pass(P, g.normal != nullptr, position_on, luminance_on, s));
    }
    HIPCHK(hipEventRecord(ws.ev, s));
    HIPCHK(call_end(c, s, nullptr));
    return ATR_OK;
} ATR_ABI_CATCH

void atr_default_accumulate_params(atr_accumulate_params* out) {
    if (!out) return;
    std::memset(out, 0, sizeof(*out));
    out->alpha = 0.0f;           // the plain running mean up to max_length frames
    out->alpha_moments = 0.0f;
    out->max_length = 64;
    out->plane_tolerance = 0.02f;
    out->min_normal_dot = 0.9f;
}

// atr_accumulate's argument rules (atray.h), host only: the structs are read, no DEVICE pointer is followed.
int atr_accumulate_check(const float* color, const atr_denoise_guides* guides, const atr_camera* prev_cam,
                         const atr_denoise_guides* prev_guides, const atr_history* prev, int32_t width, int32_t height,
                         const atr_accumulate_params* params, const atr_history* out, const float* variance) try {
    if (!color || !params || !out || !out->color || !out->length) return ATR_E_INVALID;
    if (width < 1 || width > kDenoiseMaxSide || height < 1 || height > kDenoiseMaxSide) return ATR_E_INVALID;
    const atr_accumulate_params& ap = *params;
    if (!(ap.alpha >= 0.0f && ap.alpha <= 1.0f) || !(ap.alpha_moments >= 0.0f && ap.alpha_moments <= 1.0f))
        return ATR_E_INVALID;
    if (ap.max_length < 1 || ap.max_length > kAccumulateMaxLength) return ATR_E_INVALID;
    if (!std::isfinite(ap.plane_tolerance) || !(ap.plane_tolerance > 0.0f)) return ATR_E_INVALID;
    if (!(ap.min_normal_dot >= -1.0f && ap.min_normal_dot <= 1.0f)) return ATR_E_INVALID;
    for (int32_t r : ap.reserved)
        if (r) return ATR_E_INVALID;
    if (variance && !out->moments) return ATR_E_INVALID;
    if (prev) {
        if (!prev_cam || !prev_guides || !guides || !prev->color || !prev->length) return ATR_E_INVALID;
        if (!guides->position || !prev_guides->position) return ATR_E_INVALID;
        if (!guides->normal != !prev_guides->normal || !guides->ident != !prev_guides->ident) return ATR_E_INVALID;
        if (!out->moments != !prev->moments) return ATR_E_INVALID;
        if (out->color == prev->color || out->length == prev->length || (out->moments && out->moments == prev->moments))
            return ATR_E_INVALID;
        if (prev_cam->width != width || prev_cam->height != height) return ATR_E_INVALID;
        const float k = prev_cam->h_fov * prev_cam->aspect_ratio;
        if (!(std::isfinite(k) && k > 0.0f)) return ATR_E_INVALID;
    }
    return ATR_OK;
} ATR_ABI_CATCH

int atr_accumulate(atr_ctx* c, const float* color, const atr_denoise_guides* guides, const atr_camera* prev_cam,
                   const atr_denoise_guides* prev_guides, const atr_history* prev, int32_t width, int32_t height,
                   const atr_accumulate_params* params, const atr_history* out, float* variance, uint32_t* framebuffer,
                   void* stream) try {
    if (!c) return ATR_E_INVALID;
    const int rc = atr_accumulate_check(color, guides, prev_cam, prev_guides, prev, width, height, params, out, variance);
    if (rc) return rc;
    const atr_denoise_guides none = {nullptr, nullptr, nullptr};
    const atr_denoise_guides& g = guides ? *guides : none;
    AccumulateParams P;
    std::memset(&P, 0, sizeof(P));
    P.width = width;
    P.height = height;
    P.max_length = uint32_t(params->max_length);
    P.alpha = params->alpha;
    P.alpha_moments = params->alpha_moments;
    P.plane_tolerance = params->plane_tolerance;
    P.min_normal_dot = params->min_normal_dot;
    P.hw = 0.5f * float(width);
    P.hh = 0.5f * float(height);
    P.fw = float(width);
    P.fh = float(height);
    P.color = color;
    P.normal = g.normal;
    P.position = g.position;
    P.ident = g.ident;
    if (prev) {
        const atr_camera& pc = *prev_cam;
        P.has_prev = 1;
        P.k = pc.h_fov * pc.aspect_ratio;
        const atr_vec3* src[4] = {&pc.eye, &pc.camera_x, &pc.camera_y, &pc.camera_z};
        float* dst[4] = {P.eye, P.cx, P.cy, P.cz};
        for (int i = 0; i < 4; ++i) dst[i][0] = src[i]->x, dst[i][1] = src[i]->y, dst[i][2] = src[i]->z;
        P.prev_normal = prev_guides->normal;
        P.prev_position = prev_guides->position;
        P.prev_ident = prev_guides->ident;
        P.prev_color = prev->color;
        P.prev_moments = prev->moments;
        P.prev_length = prev->length;
    }
    P.out_color = out->color;
    P.out_moments = out->moments;
    P.out_length = out->length;
    P.variance = variance;
    P.framebuffer = framebuffer;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);  // NULL = the null stream (HIP convention)
    HIPCHK(call_begin(c, s));
    HIPCHK(atr_launch_accumulate(P, s));
    HIPCHK(call_end(c, s, nullptr));
    return ATR_OK;
} ATR_ABI_CATCH

namespace {
// A camera whose rays the camera calls can make (atray.h atr_camera_guides): a size, and every float
// field finite. Host only.
bool camera_rays_ok(const atr_camera& cm) {
    if (cm.width < 1 || cm.height < 1 || cm.width > (1 << 16) || cm.height > (1 << 16)) return false;
    const atr_vec3* v[5] = {&cm.camera_z, &cm.camera_x, &cm.camera_y, &cm.eye, &cm.frame_center};
    for (const atr_vec3* a : v)
        if (!std::isfinite(a->x) || !std::isfinite(a->y) || !std::isfinite(a->z)) return false;
    return std::isfinite(cm.aspect_ratio) && std::isfinite(cm.h_fov) && std::isfinite(cm.half_pixel_width) &&
           std::isfinite(cm.half_pixel_height);
}

int camera_rays_args(const atr_camera* cam, int64_t first_pixel, int64_t npixels, const float* origins,
                     const float* directions) {
    if (!cam || !camera_rays_ok(*cam)) return ATR_E_INVALID;
    const int64_t total = int64_t(cam->width) * cam->height;
    if (first_pixel < 0 || npixels < 0 || first_pixel > total || npixels > total - first_pixel) return ATR_E_INVALID;
    if (npixels > 0 && (!origins || !directions)) return ATR_E_INVALID;
    return ATR_OK;
}
}  // namespace

// The primary rays of a range of pixels on the host (atray.h): guides.h's function, the one the
// device kernels call.
int atr_camera_rays_host(const atr_camera* cam, int64_t first_pixel, int64_t npixels, float* origins,
                         float* directions) try {
    const int rc = camera_rays_args(cam, first_pixel, npixels, origins, directions);
    if (rc) return rc;
    for (int64_t i = 0; i < npixels; ++i) {
        const int64_t pix = first_pixel + i;
        const V3 d = camera_ray_dir(*cam, int32_t(pix % cam->width), int32_t(pix / cam->width));
        origins[3 * i] = cam->eye.x; origins[3 * i + 1] = cam->eye.y; origins[3 * i + 2] = cam->eye.z;
        directions[3 * i] = d.x; directions[3 * i + 1] = d.y; directions[3 * i + 2] = d.z;
    }
    return ATR_OK;
} ATR_ABI_CATCH

// The same rays into device arrays (guides.hip camera_rays_kernel).
int atr_camera_rays(atr_ctx* c, const atr_camera* cam, int64_t first_pixel, int64_t npixels, float* origins,
                    float* directions, void* stream) try {
    if (!c) return ATR_E_INVALID;
    const int rc = camera_rays_args(cam, first_pixel, npixels, origins, directions);
    if (rc || npixels == 0) return rc;
    CameraRaysParams P;
    std::memset(&P, 0, sizeof(P));
    P.cam = *cam;
    P.first = first_pixel;
    P.n = npixels;
    P.o = origins;
    P.d = directions;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);  // NULL = the null stream (HIP convention)
    HIPCHK(call_begin(c, s));
    HIPCHK(atr_launch_camera_rays(P, s));
    HIPCHK(call_end(c, s, nullptr));
    return ATR_OK;
} ATR_ABI_CATCH

// A camera's guides (atray.h): the render's block list for the tiles, one kernel
// (guides.hip), no workspace.
int atr_camera_guides(atr_ctx* c, const atr_camera* cam, const atr_tile* tiles, int32_t ntiles,
                      const atr_guides_out* out, void* stream) try {
    if (!c || !cam || !out || ntiles <= 0 || !tiles) return ATR_E_INVALID;
    if (!out->normal && !out->position && !out->ident && !out->depth && !out->material) return ATR_E_INVALID;
    if (!camera_rays_ok(*cam)) return ATR_E_INVALID;
    for (int32_t i = 0; i < ntiles; ++i) {
        const atr_tile& t = tiles[i];
        if (t.min_x < 0 || t.min_y < 0 || t.max_x < t.min_x || t.max_y < t.min_y || t.max_x >= cam->width ||
            t.max_y >= cam->height)
            return ATR_E_INVALID;
    }
    if (!c->d_scene) return ATR_E_NOSCENE;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);  // NULL = the null stream (HIP convention)
    int rc = ATR_OK;
    BlockSet* bs = get_blocks(c, tiles, ntiles, cam->width, cam->height, rc);
    if (!bs) return rc;
    GuidesParams P;
    std::memset(&P, 0, sizeof(P));
    P.cam = *cam;
    P.scene = c->d_scene;
    P.blocks = static_cast<const DBlock*>(bs->dev.p);  // the base list: no plan, its cost would train the render's
    P.nblocks = int32_t(bs->host.size());
    P.xcd_chunk = c->tune.xcd_chunk;
    P.hyb_a = c->tune.hybrid_a;
    P.hyb_b = c->tune.hybrid_b;
    P.normal = out->normal;
    P.position = out->position;
    P.ident = out->ident;
    P.depth = out->depth;
    P.material = out->material;
    P.error_flag = c->d_error;
    HIPCHK(call_begin(c, s));
    HIPCHK(atr_launch_camera_guides(P, s));
    HIPCHK(call_end(c, s, nullptr));
    return ATR_OK;
} ATR_ABI_CATCH

int atr_render_wait(atr_ctx* c, uint32_t timeout_ms, int32_t* tiles_done) try {
    if (!c) return ATR_E_INVALID;
    if (tiles_done) *tiles_done = 0;
    if (!c->have_render) { return ATR_OK; }
    HIPCHK(hipSetDevice(c->device));
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t q = hipEventQuery(c->ev_last);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady) return -(1000 + int(q));
        const auto el = std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0);
        if (uint32_t(el.count()) >= timeout_ms) {
            if (tiles_done && c->prog_active) {  // tiles of the leading groups already complete
                size_t g = 0;
                for (; g < c->prog_end.size(); ++g) {
                    const hipError_t qg = hipEventQuery(c->prog_ev[g]);
                    if (qg != hipSuccess) break;
                    *tiles_done = c->prog_end[g];
                }
                // every group finished since ev_last was queried: the render is done (ev_last
                // follows the last group on the same stream), report it as done, not running
                if (g == c->prog_end.size() && !c->prog_end.empty()) {
                    HIPCHK(hipEventSynchronize(c->ev_last));
                    break;
                }
            }
            return 1;
        }
        std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
    int32_t err = 0;
    HIPCHK(hipMemcpy(&err, c->d_error, sizeof(err), hipMemcpyDeviceToHost));
    if (err) {
        HIPCHK(hipMemset(c->d_error, 0, sizeof(int32_t)));
        // bit 1: a queue-sort slot outside its level (paths.hip path_sort_rank; never expected)
        return (err & 2) ? -(1000 + int(hipErrorUnknown)) : ATR_E_TREE_DEPTH;
    }
    if (tiles_done) *tiles_done = c->last_ntiles;
    return ATR_OK;
} ATR_ABI_CATCH

int atr_last_kernel_ms(atr_ctx* c, float* ms) try {
    if (!c || !ms || !c->have_render) return ATR_E_INVALID;
    HIPCHK(hipEventSynchronize(c->ev_last));
    HIPCHK(hipEventElapsedTime(ms, c->ev_start, c->ev_last));
    return ATR_OK;
} ATR_ABI_CATCH

int atr_unpack(atr_ctx* c, const atr_tile* tiles, int32_t ntiles, int32_t width, const uint32_t* packed,
               uint32_t* image, void* stream) try {
    if (!c || !packed || !image || width <= 0 || ntiles < 0 || (ntiles && !tiles)) return ATR_E_INVALID;
    HIPCHK(hipSetDevice(c->device));
    int32_t H = 0;
    for (int32_t i = 0; i < ntiles; ++i) if (tiles[i].max_y + 1 > H) H = tiles[i].max_y + 1;
    int rc = ATR_OK;
    BlockSet* bs = get_blocks(c, tiles, ntiles, width, H, rc);
    if (!bs) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);  // NULL = the null stream (HIP convention)
    HIPCHK(atr_launch_unpack(static_cast<const DBlock*>(bs->dev.p), int32_t(bs->host.size()), width, packed, image, s));
    HIPCHK(note_launch(c, s));
    return ATR_OK;
} ATR_ABI_CATCH

int atr_tile_ray_casts(atr_ctx* c, const atr_tile* tiles, int32_t ntiles, int32_t width,
                       const uint32_t* casts, int64_t* out, void* stream) try {
    if (!c || !casts || !out || width <= 0 || ntiles < 0 || (ntiles && !tiles)) return ATR_E_INVALID;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);  // NULL = the null stream (HIP convention)
    void* dt = nullptr;
    HIPCHK(hipMallocAsync(&dt, sizeof(atr_tile) * size_t(ntiles ? ntiles : 1), s));
    HIPCHK(hipMemcpyAsync(dt, tiles, sizeof(atr_tile) * size_t(ntiles), hipMemcpyHostToDevice, s));
    HIPCHK(atr_launch_tile_casts(static_cast<const atr_tile*>(dt), ntiles, width, casts, out, s));
    HIPCHK(hipFreeAsync(dt, s));
    HIPCHK(hipStreamSynchronize(s));
    return ATR_OK;
} ATR_ABI_CATCH

int atr_packed_tile_ray_casts(atr_ctx* c, const atr_tile* tiles, int32_t ntiles, int32_t width, int32_t height,
                              const uint32_t* casts, int32_t nframes, int64_t frame_stride, int64_t* out,
                              void* stream) try {
    if (!c || !casts || !out || width <= 0 || height <= 0 || ntiles < 0 || (ntiles && !tiles) || nframes < 0 ||
        nframes > 65535)
        return ATR_E_INVALID;
    HIPCHK(hipSetDevice(c->device));
    int rc = ATR_OK;
    BlockSet* bs = get_blocks(c, tiles, ntiles, width, height, rc);  // the render's cached set
    if (!bs) return rc;
    if (nframes > 1 && frame_stride < bs->packed_pixels) return ATR_E_INVALID;
    hipStream_t s = static_cast<hipStream_t>(stream);  // NULL = the null stream (HIP convention)
    const int64_t n = bs->packed_pixels;
    if (!bs->tile_ready) {  // owner of every pixel = the first tile holding it (packed: traced once)
        std::vector<int32_t> owner(size_t(width) * size_t(height), -1);
        for (int32_t k = 0; k < ntiles; ++k) {
            const int32_t x0 = std::max(tiles[k].min_x, 0), x1 = std::min(tiles[k].max_x, width - 1);
            const int32_t y0 = std::max(tiles[k].min_y, 0), y1 = std::min(tiles[k].max_y, height - 1);
            for (int32_t y = y0; y <= y1; ++y)
                for (int32_t x = x0; x <= x1; ++x) {
                    int32_t& o = owner[size_t(y) * size_t(width) + size_t(x)];
                    if (o < 0) o = k;
                }
        }
        std::vector<int32_t> st(size_t(n > 0 ? n : 1), -1);
        for (const DBlock& blk : bs->host) {  // slots out_base.. in lane order (not list order)
            const uint64_t m = uint64_t(blk.mask_lo) | (uint64_t(blk.mask_hi) << 32);
            size_t k = size_t(blk.out_base);
            for (int lane = 0; lane < 64; ++lane)
                if ((m >> lane) & 1)
                    st[k++] = owner[size_t(blk.y0 + (lane >> 3)) * size_t(width) + size_t(blk.x0 + (lane & 7))];
        }
        // a hipMemcpy below may overwrite a buffer a kernel on another stream still reads
        HIPCHK(wait_all(c));
        const size_t need = st.size() * sizeof(int32_t);
        if (bs->dev_tile.n < need) {
            if (bs->dev_tile.p) (void)hipFree(bs->dev_tile.p);
            bs->dev_tile = DevBuf();
            if (hipMalloc(&bs->dev_tile.p, need) != hipSuccess) return ATR_E_NOMEM;
            bs->dev_tile.n = need;
        }
        HIPCHK(hipMemcpy(bs->dev_tile.p, st.data(), need, hipMemcpyHostToDevice));
        bs->tile_ready = true;
    }
    HIPCHK(hipMemsetAsync(out, 0, sizeof(int64_t) * size_t(nframes) * size_t(ntiles), s));
    HIPCHK(atr_launch_packed_tile_casts(static_cast<const int32_t*>(bs->dev_tile.p), n, casts, frame_stride, nframes,
                                        ntiles, reinterpret_cast<unsigned long long*>(out), s));
    HIPCHK(note_launch(c, s));
    return ATR_OK;
} ATR_ABI_CATCH

int atr_pack_bgr(atr_ctx* c, const uint32_t* framebuffer, int64_t npixels, uint8_t* out, void* stream) try {
    if (!c || npixels < 0 || (npixels && (!framebuffer || !out))) return ATR_E_INVALID;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(atr_launch_pack_bgr(framebuffer, npixels, out, static_cast<hipStream_t>(stream)));
    return ATR_OK;
} ATR_ABI_CATCH

int atr_scatter_bgr(atr_ctx* c, const uint8_t* packed, int64_t npixels, const int64_t* dst_index, uint32_t* image,
                    void* stream) try {
    if (!c || npixels < 0 || (npixels && (!packed || !dst_index || !image))) return ATR_E_INVALID;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(atr_launch_scatter_bgr(packed, npixels, dst_index, image, static_cast<hipStream_t>(stream)));
    return ATR_OK;
} ATR_ABI_CATCH

int64_t atr_pack_bgr_masked_bound(int64_t npixels) {
    if (npixels < 0) return ATR_E_INVALID;
    const int64_t nc = atr_masked_chunks(npixels);
    return 16 + 4 * nc + 1024 * nc + 512 * nc + 3 * npixels;  // header, chunk offsets, masks, group offsets
}

int atr_pack_bgr_masked(atr_ctx* c, const uint32_t* framebuffer, int64_t npixels, uint32_t background, uint8_t* out,
                        int64_t* nbytes, void* stream) try {
    if (!c || npixels < 0 || npixels >= (int64_t(1) << 32) || !out || !nbytes || (npixels && !framebuffer))
        return ATR_E_INVALID;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(atr_launch_pack_bgr_masked(framebuffer, npixels, background, out, nbytes, static_cast<hipStream_t>(stream)));
    return ATR_OK;
} ATR_ABI_CATCH

int atr_scatter_bgr_masked(atr_ctx* c, const uint8_t* packed, int64_t npixels, const int64_t* dst_index,
                           uint32_t* image, void* stream) try {
    if (!c || npixels < 0 || npixels >= (int64_t(1) << 32) || (npixels && (!packed || !dst_index || !image)))
        return ATR_E_INVALID;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(atr_launch_scatter_bgr_masked(packed, npixels, dst_index, image, static_cast<hipStream_t>(stream)));
    return ATR_OK;
} ATR_ABI_CATCH

int atr_unpack_masked(atr_ctx* c, const atr_tile* tiles, int32_t ntiles, int32_t width, int32_t height,
                      const uint8_t* packed, int32_t nframes, uint32_t* image, int64_t image_stride, void* stream) try {
    if (!c || !packed || !image || width <= 0 || height <= 0 || ntiles < 0 || (ntiles && !tiles) || nframes < 0 ||
        image_stride < int64_t(width) * height)
        return ATR_E_INVALID;
    HIPCHK(hipSetDevice(c->device));
    int rc = ATR_OK;
    BlockSet* bs = get_blocks(c, tiles, ntiles, width, height, rc);  // the render's cached set
    if (!bs) return rc;
    const int64_t own = bs->packed_pixels;
    if (nframes == 0 || own == 0) return ATR_OK;
    if (int64_t(nframes) * own >= (int64_t(1) << 32)) return ATR_E_INVALID;
    hipStream_t s = static_cast<hipStream_t>(stream);  // NULL = the null stream (HIP convention)
    HIPCHK(atr_launch_unpack_masked(static_cast<const DBlock*>(bs->dev.p), int32_t(bs->host.size()), width, packed,
                                    nframes, own, image, image_stride, s));
    HIPCHK(note_launch(c, s));
    return ATR_OK;
} ATR_ABI_CATCH

int atr_unpack_masked_ranks(atr_ctx* c, int32_t nsrc, const atr_tile* const* tiles, const int32_t* ntiles,
                            int32_t width, int32_t height, const uint8_t* const* packed, const int32_t* raw,
                            int32_t nframes, uint32_t* image, int64_t image_stride, void* stream) try {
    if (!c || nsrc < 0 || (nsrc && (!tiles || !ntiles || !packed)) || !image || width <= 0 || height <= 0 ||
        nframes < 0 || image_stride < int64_t(width) * height)
        return ATR_E_INVALID;
    for (int32_t i = 0; i < nsrc; ++i)
        if (ntiles[i] < 0 || (ntiles[i] && !tiles[i]) || !packed[i]) return ATR_E_INVALID;
    HIPCHK(hipSetDevice(c->device));
    if (nsrc == 0 || nframes == 0) return ATR_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);  // NULL = the null stream (HIP convention)
    const int32_t kMax = atr_unpack_max_sources();
    for (int32_t i0 = 0; i0 < nsrc; i0 += kMax) {  // one launch pair per kMax sources
        const int32_t n = std::min(kMax, nsrc - i0);
        std::vector<const DBlock*> blocks(size_t(n), nullptr);
        std::vector<int32_t> nb(size_t(n), 0);
        std::vector<int64_t> own(size_t(n), 0);
        for (int32_t k = 0; k < n; ++k) {
            int rc = ATR_OK;
            // the renders' cached sets (the most recently used slots: a later lookup here does not
            // evict an earlier one of this batch)
            BlockSet* bs = get_blocks(c, tiles[i0 + k], ntiles[i0 + k], width, height, rc);
            if (!bs) return rc;
            blocks[size_t(k)] = static_cast<const DBlock*>(bs->dev.p);
            nb[size_t(k)] = int32_t(bs->host.size());
            own[size_t(k)] = bs->packed_pixels;
            if (int64_t(nframes) * own[size_t(k)] >= (int64_t(1) << 32)) return ATR_E_INVALID;
        }
        HIPCHK(atr_launch_unpack_masked_multi(n, blocks.data(), nb.data(), own.data(), packed + i0,
                                              raw ? raw + i0 : nullptr, width, nframes, image, image_stride, s));
        // recorded per batch: a cache miss of the next batch may evict one of this batch's sets,
        // and its wait_all has to cover this decode before the copy rewrites the blocks
        HIPCHK(note_launch(c, s));
    }
    return ATR_OK;
} ATR_ABI_CATCH

int atr_render_plan_info(atr_ctx* c, const atr_tile* tiles, int32_t ntiles, int32_t width, int32_t height,
                         int32_t* base_out, uint32_t* mask_hi_lo_out, int64_t cap, uint64_t* cost_out,
                         int64_t* nplanned) try {
    if (!c || !nplanned || width <= 0 || height <= 0 || ntiles < 0 || (ntiles && !tiles)) return ATR_E_INVALID;
    HIPCHK(hipSetDevice(c->device));
    int rc = ATR_OK;
    BlockSet* bs = get_blocks(c, tiles, ntiles, width, height, rc);
    if (!bs) return rc;
    *nplanned = 0;
    if (!bs->plan_ready) return ATR_OK;
    HIPCHK(wait_all(c));  // the plan stream's kernels too
    const int64_t nb = int64_t(bs->host.size()), np = nb + bs->max_split;
    *nplanned = np;
    if (cap < np) return ATR_OK;  // size query
    std::vector<DBlock> h(static_cast<size_t>(np));
    // the list built last (from the last planned launch's costs, in that launch's parity half)
    const DBlock* last = static_cast<const DBlock*>(bs->plan_blocks.p) + size_t(bs->plan_par ^ 1) * size_t(np);
    HIPCHK(hipMemcpy(h.data(), last, size_t(np) * sizeof(DBlock), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < np; ++i) {
        if (base_out) base_out[i] = h[size_t(i)].base;
        if (mask_hi_lo_out) {
            mask_hi_lo_out[2 * i] = h[size_t(i)].mask_lo;
            mask_hi_lo_out[2 * i + 1] = h[size_t(i)].mask_hi;
        }
    }
    if (cost_out) HIPCHK(hipMemcpy(cost_out, bs->cost_last.p, size_t(nb) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return ATR_OK;
} ATR_ABI_CATCH

int atr_set_cell_plan(atr_ctx* c, int32_t width, int32_t height, const uint8_t* plan) try {
    if (!c || (plan && (width <= 0 || height <= 0))) return ATR_E_INVALID;
    const int32_t cw = (width + 7) / 8, ch = (height + 7) / 8;
    if (plan) {
        for (size_t i = 0; i < size_t(cw) * size_t(ch); ++i) {
            const int p = plan[i] & 0xF;
            if (!(p == 0 || p == 1 || p == 2 || p == 4 || p == 8)) return ATR_E_INVALID;
        }
        c->cplan.assign(plan, plan + size_t(cw) * size_t(ch));
        c->cplan_w = width;
        c->cplan_h = height;
    } else {
        c->cplan.clear();
        c->cplan_w = c->cplan_h = 0;
    }
    ++c->cplan_gen;  // cached block lists are rebuilt on their next use
    return ATR_OK;
} ATR_ABI_CATCH

int atr_render_cell_costs(atr_ctx* c, const atr_camera* cam, uint64_t seed, int32_t variant, int64_t* out) try {
    if (!c || !cam || !out || cam->width <= 0 || cam->height <= 0) return ATR_E_INVALID;
    if (!c->d_scene) return ATR_E_NOSCENE;
    HIPCHK(hipSetDevice(c->device));
    const int32_t cw = (cam->width + 7) / 8, ch = (cam->height + 7) / 8;
    const atr_tile full = {0, 0, cam->width - 1, cam->height - 1};
    int rc = ATR_OK;
    BlockSet* bs = get_blocks(c, &full, 1, cam->width, cam->height, rc);
    if (!bs) return rc;
    const size_t nb = bs->host.size();
    DevTmp fb;
    DevTmp cost;
    HIPCHK(hipMalloc(&fb.p, std::max<size_t>(1, size_t(bs->packed_pixels)) * 4));
    HIPCHK(hipMalloc(&cost.p, std::max<size_t>(1, nb) * sizeof(unsigned long long)));
    HIPCHK(hipMemset(cost.p, 0, std::max<size_t>(1, nb) * sizeof(unsigned long long)));  // atomically added
    RenderParams P;
    std::memset(&P, 0, sizeof(P));
    P.cam = *cam;
    P.scene = c->d_scene;
    P.seed = seed;
    P.blocks = static_cast<const DBlock*>(bs->dev.p);
    P.nblocks = int32_t(nb);
    P.layout = ATR_LAYOUT_PACKED;
    P.framebuffer = static_cast<uint32_t*>(fb.p);
    P.error_flag = c->d_error;
    P.block_cost = static_cast<unsigned long long*>(cost.p);
    apply_tuning(c, P);
    const int sched = auto_sched(variant, *cam);
    if (sched < 0) return ATR_E_INVALID;
    HIPCHK(launch_render(c, P, sched, nullptr));
    HIPCHK(hipDeviceSynchronize());
    std::vector<unsigned long long> h(nb);
    if (nb) HIPCHK(hipMemcpy(h.data(), cost.p, nb * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < size_t(cw) * size_t(ch); ++i) out[i] = 0;
    for (size_t k = 0; k < nb; ++k)  // a split cell's waves add up
        out[size_t(bs->host[k].y0 / 8) * size_t(cw) + size_t(bs->host[k].x0 / 8)] += int64_t(h[k]);
    return ATR_OK;
} ATR_ABI_CATCH

int atr_device_alloc(atr_ctx* c, size_t bytes, void** p) try {
    if (!c || !p) return ATR_E_INVALID;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMalloc(p, bytes ? bytes : 16));
    return ATR_OK;
} ATR_ABI_CATCH
int atr_device_free(atr_ctx* c, void* p) try {
    if (!c) return ATR_E_INVALID;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipFree(p));
    return ATR_OK;
} ATR_ABI_CATCH
int atr_memcpy_d2h(atr_ctx* c, void* dst, const void* src, size_t bytes) try {
    if (!c || !dst || !src) return ATR_E_INVALID;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return ATR_OK;
} ATR_ABI_CATCH
int atr_memcpy_h2d(atr_ctx* c, void* dst, const void* src, size_t bytes) try {
    if (!c || !dst || !src) return ATR_E_INVALID;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipDeviceSynchronize());  // a render may still read the destination
    HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return ATR_OK;
} ATR_ABI_CATCH
int atr_memset_d(atr_ctx* c, void* p, int v, size_t bytes) try {
    if (!c || !p) return ATR_E_INVALID;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemset(p, v, bytes));
    return ATR_OK;
} ATR_ABI_CATCH

}  // extern "C"
