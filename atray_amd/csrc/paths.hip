// paths.hip -- the sample-parallel path engine for multi-bounce renders.
//
// render_tile_from_camera (renderer.cpp:336-358) runs a pixel's spp samples one after another,
// each a cast_ray bounce loop (:213-262). With one PCG stream per (pixel, sample) (engine.h
// path_stream) the samples are independent paths, so here every lane owns one PATH and a pixel's
// samples run side by side:
//   path_camera_kernel  one wavefront = 64 consecutive paths of one 8x8 cell (a pixel's samples
//                       together): the camera rays (one origin per wave: HYBRID's coherent flavour,
//                       scan.h), then the first shading step; a path that goes on is appended to a
//                       queue (a ballot, one atomic per wave);
//   path_bounce_kernel  bounce k of every queued path: persistent waves claim 64 queue entries at a
//                       time, trace them (FLAT's dealt rounds for incoherent rays), shade, and
//                       append the survivors to the other queue -- one launch per bounce level, so
//                       the trace holds no path state (loaded after the query) and each kernel has
//                       its own register budget;
//   path_resolve_kernel per pixel, the sample colours summed in sample order with the reference's
//                       f32 adds (col += cast_ray(...), :353-356), then average, clamp, BGRX byte
//                       conversion (:358-365) -- every output bit-identical to the cell kernels';
//   path_resolve_accum_kernel  the resolve of a sample pass (atr_render_start_samples, DESIGN.md
//                       §4k): the sums continue from the frame's stored running sums.
// A batch is a range of the launch's cell list (PathParams, engine.h); the host runs camera,
// bounces and resolve per batch on one stream (capi.cpp launch_paths).
#include <hip/hip_runtime.h>

#include "launch.h"
#include "paths.h"
#include "scan.h"
#include "sort_key.h"

namespace atr {

// (The helpers take plain values: a reference to the kernel argument passed to a function made the
// compiler copy the whole 1.8-KB argument into scratch.)
// cell c of the launch's list -> its frame and block (frames interleaved, RenderParams)
__device__ __forceinline__ void cell_of(int32_t frame_blocks, int32_t nblocks, int32_t c, int32_t& fidx, int32_t& bi) {
    const int32_t nf = frame_blocks > 0 ? nblocks / frame_blocks : 1;
    fidx = c % nf;
    bi = c / nf;
}

__device__ __forceinline__ size_t out_index(int32_t layout, int32_t width, int64_t frame_stride, const DBlock& blk,
                                            uint64_t mask, int pl, int32_t fidx) {
    size_t o;
    if (layout == ATR_LAYOUT_PACKED) o = size_t(blk.out_base) + __popcll(mask & ((uint64_t(1) << pl) - 1));
    else o = size_t(blk.y0 + (pl >> 3)) * size_t(width) + size_t(blk.x0 + (pl & 7));
    return o + size_t(fidx) * size_t(frame_stride);
}

// path_finish, kAllSky and path_enqueue: paths.h (the radiance query's entry kernel feeds the same
// queues and result slots).
#ifndef ATR_SKY_ELIDE  // experiment builds: 0 = every sample writes its result slot (round 5)
#define ATR_SKY_ELIDE 1
#endif

template <bool COUNT>
__device__ __forceinline__ void path_counters(unsigned long long* C, const Ctr& ct, uint32_t traced) {
    const int lane = threadIdx.x & 63;
    uint32_t v[10] = {traced, ct.box, ct.tri, ct.leaf, ct.wave_tri, ct.pass, ct.box_all, 0u, ct.cbox, ct.screen};
#pragma unroll
    for (int k = 0; k < 10; ++k) {
        uint32_t t = v[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off);
        if (lane == 0 && t) atomicAdd(C + k, (unsigned long long)t);
    }
    if (lane == 0) atomicAdd(C + 7, 1ull);
    // [10..15] wave clocks of the scan phases (DIAG build only; zero otherwise), [22..26] SIMD use
    if (lane == 0) {
        atomicAdd(C + 10, (unsigned long long)ct.t_pass);
        atomicAdd(C + 11, (unsigned long long)ct.t_lp);
        atomicAdd(C + 12, (unsigned long long)ct.t_deal);
        atomicAdd(C + 14, (unsigned long long)ct.t_prep);
        atomicAdd(C + 15, (unsigned long long)ct.t_scan);
    }
    uint32_t e[5] = {ct.cand_wave, ct.node_wave, ct.node_lane, ct.round_wave, ct.round_items};
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        uint32_t x = e[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
        if (lane == 0 && x) atomicAdd(C + 22 + k, (unsigned long long)x);
    }
}

// ------------------------------------------------------------------ camera rays + first shading
// ACCUM (a sample pass, atr_render_start_samples): the pass's sample s is the frame's sample
// P.first_sample + s -- its stream, and the primary hit outputs are the frame's sample 0's. The
// all-sky shortcut stays keyed on the pass's own sample 0: without AA every sample of the pixel,
// in this pass or another, casts the same camera ray.
template <bool COUNT, int OCC, bool SORT, bool ACCUM = false>
__global__ __launch_bounds__(256, OCC) void path_camera_kernel(PathParams P) {
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const uint32_t spp = uint32_t(__builtin_amdgcn_readfirstlane(int(P.cam.samples_per_pixel)));
    const int64_t wv = int64_t(remap_xcd(blockIdx.x, gridDim.x, P.xcd_chunk)) * 4 + wave;  // wave of the batch
    if (wv >= int64_t(P.ncells) * spp) return;  // whole wavefront
    // a cell's 64 x spp paths are spp consecutive waves: the cell is wave-uniform
    const int32_t cellrel = int32_t(wv / spp);
    const uint32_t r = uint32_t(wv - int64_t(cellrel) * spp) * 64u + uint32_t(lane);  // path within the cell
    const int pl = int(r / spp);  // the pixel's lane in the 8x8 cell
    const uint32_t s = r - uint32_t(pl) * spp;  // its sample
    const uint32_t g = uint32_t(cellrel) * 64u * spp + s * 64u + uint32_t(pl);  // result slot
    int32_t fidx, bi;
    cell_of(P.frame_blocks, P.nblocks, P.cell0 + cellrel, fidx, bi);
    const DBlock blk = P.blocks[bi];
    const uint64_t mask = uint64_t(blk.mask_lo) | (uint64_t(blk.mask_hi) << 32);
    const atr_camera& cm = P.nfcam > 0 ? P.fcam[__builtin_amdgcn_readfirstlane(fidx)] : P.cam;
    const int32_t bl = cm.bounce_limit;
    const bool active = ((mask >> pl) & 1) && bl > 0;
    const uint64_t clk0 = P.block_cost ? clock64() : 0;
    const DScene* S = uniform_global(P.scene);
    const int32_t x = blk.x0 + (pl & 7), y = blk.y0 + (pl >> 3);
    const int64_t pix = int64_t(y) * cm.width + x;
    uint64_t st, stream;
    uint32_t fs = s;  // the sample's index in the frame
    if constexpr (ACCUM) fs += P.first_sample;
    path_stream(P.seed, pix, fs, st, stream);
    const float film_y = -1.0f + 2.0f * (float(y) / float(cm.height));                                  // :317
    const float film_x = ((-1.0f + 2.0f * (float(x) / float(cm.width))) * cm.h_fov) * cm.aspect_ratio;  // :329
    const V3 eye = from(cm.eye), fc = from(cm.frame_center), cx = from(cm.camera_x), cy = from(cm.camera_y);
    V3 d;
    if (cm.anti_aliasing) {  // :338-347, the sample's two jitter draws
        const float xo = rand_bi(st, stream) * cm.half_pixel_width + film_x;
        const float yo = rand_bi(st, stream) * cm.half_pixel_height + film_y;
        d = unit(sub(add(add(fc, scale(cx, xo)), scale(cy, yo)), eye));
    } else {
        d = unit(sub(add(add(fc, scale(cx, film_x)), scale(cy, film_y)), eye));  // :350-351
    }
    int err = 0;
    Ctr ct;
    Isect id;
    id.type = T_NONE;
    intersect_scene<SCHED_HYBRID, FlavCamera, COUNT>(S, eye, d, active, id, err, ct, P.hyb_a, P.hyb_b);
    bool go = false;
    V3 o = eye, ret = mk(0.f, 0.f, 0.f), w = mk(1.f, 1.f, 1.f);
    if (active) {
        if (fs == 0) {  // sample 0's camera ray: the primary hit outputs
            const size_t oi = out_index(P.layout, cm.width, P.frame_stride, blk, mask, pl, fidx);
            if (P.hit_face) P.hit_face[oi] = id.face;
            if (P.hit_t) P.hit_t[oi] = id.t;
        }
        const DMaterial& mat = S->mats[id.material];
        if (id.type == T_SKY) {  // :225-229 at i = 0
            ret = add(ret, had(w, mk(mat.ex, mat.ey, mat.ez)));
            if (cm.anti_aliasing || !ATR_SKY_ELIDE) path_finish(P.out, g, ret, 0u);
            else if (s == 0) path_finish(P.out, g, ret, kAllSky);  // the pixel's every sample (kAllSky)
        } else {
            bounce_shade(mat, id, o, d, ret, w, st, stream);  // :231-258
            if (bl <= 1) path_finish(P.out, g, ret, uint32_t(bl));  // ran to the limit (:260)
            else go = true;
        }
    }
    path_enqueue<SORT>(P.q[0], P.cap, &P.ctl[0], go, o, d, uint32_t(pix), g, ret, w, st, P.sort);
    const uint32_t traced = active ? 1u : 0u;
    if (P.traced_rays) add_traced(P.traced_rays, traced, int(wv));
    if (err && P.error_flag) atomicOr(P.error_flag, 1);
    if (P.block_cost && lane == 0) atomicAdd(P.block_cost + blk.base, (unsigned long long)(clock64() - clk0));
    if constexpr (COUNT) path_counters<COUNT>(P.counters, ct, traced);
}

// ------------------------------------------------------------------ bounce k of the queued paths
// Leaf buffer entries of the bounce rays' queries (the scan is templated on it). 6 entries cut the
// LDS to 18 KB per workgroup, enough for 8 waves/SIMD, but cost re-walks: c4 71.0 ms per frame at 7
// waves and 72.1 at 8 (64 VGPRs, scratch in the hot loop) vs 69.5 with 8 entries.
#ifndef ATR_BOUNCE_LEAFBUF
#define ATR_BOUNCE_LEAFBUF kLeafBuf
#endif
constexpr int kBounceLeafBuf = ATR_BOUNCE_LEAFBUF;  // experiment builds: -DATR_BOUNCE_LEAFBUF=6
template <bool COUNT, int OCC, bool SORT>
__global__ __launch_bounds__(256, OCC) void path_bounce_kernel(PathParams P) {
    const int lane = threadIdx.x & 63;
    const int32_t k = P.bounce;  // 1 .. bounce_limit - 1
    const int32_t bl = P.cam.bounce_limit;
    const float4_t* __restrict__ qin = P.q[(k - 1) & 1];
    const uint32_t n = uint32_t(__builtin_amdgcn_readfirstlane(int(P.ctl[k - 1].tail)));
    const DScene* S = uniform_global(P.scene);
    const uint32_t spp = P.cam.samples_per_pixel;
    int err = 0;
    Ctr ct;
    uint32_t traced = 0;
    for (;;) {  // every wave leaves once the queue is claimed: the exit every wave reaches
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(&P.ctl[k].head, 64u);
        base = uint32_t(__builtin_amdgcn_readfirstlane(int(__shfl(int(base), 0))));
        if (base >= n) break;
        const uint64_t clk0 = P.block_cost ? clock64() : 0;
        const uint32_t i = base + uint32_t(lane);
        const bool valid = i < n;
        // sorted queues: claimed position i of the level's key order -> its entry (PathSort)
        uint32_t e = i;
        if (SORT && valid) e = P.sort.perm[i];
        V3 o = mk(0.f, 0.f, 0.f), d = mk(0.f, 0.f, 1.f);
        if (valid) {
            const float4_t a = qin[SORT ? 4 * int64_t(e) : e], b = qin[SORT ? 4 * int64_t(e) + 1 : P.cap + e];
            o = mk(a.x, a.y, a.z);
            d = mk(a.w, b.x, b.y);
        }
        const SceneHit sh = intersect_models<SCHED_FLAT, FlavBounce, COUNT, kBounceLeafBuf>(S, o, d, valid, err, ct, P.hyb_a, P.hyb_b);
        // the path -- its ray too -- is read again after the query instead of being held through
        // it: the memory clobber keeps the loads here, the opaque copy of the entry index keeps
        // their addresses from being formed before the query
        uint32_t ea = e;
        __asm__ volatile("" : "+v"(ea) :: "memory");
        bool go = false;
        uint32_t pix = 0, g = 0;
        V3 ret = mk(0.f, 0.f, 0.f), w = mk(1.f, 1.f, 1.f);
        uint64_t st = 0;
        if (valid) {
            traced += 1;
            const int64_t e0 = SORT ? 4 * int64_t(ea) : ea, es = SORT ? 1 : P.cap;
            const float4_t a = qin[e0], b = qin[es + e0], c = qin[2 * es + e0], q3 = qin[3 * es + e0];
            o = mk(a.x, a.y, a.z);
            d = mk(a.w, b.x, b.y);
            Isect id;
            scene_finish(S, o, d, sh.best, sh.face, sh.fu, sh.fv, sh.nm, id);  // renderer.cpp:86-160
            pix = __float_as_uint(b.z);
            g = __float_as_uint(b.w);
            ret = mk(c.x, c.y, c.z);
            w = mk(c.w, q3.x, q3.y);
            st = uint64_t(__float_as_uint(q3.z)) | (uint64_t(__float_as_uint(q3.w)) << 32);
            const uint64_t stream = (uint64_t(pix) << 1) | 1ULL;
            const DMaterial& mat = S->mats[id.material];
            if (id.type == T_SKY) {  // :225-229 at i = k
                ret = add(ret, had(w, mk(mat.ex, mat.ey, mat.ez)));
                path_finish(P.out, g, ret, uint32_t(k));
            } else {
                bounce_shade(mat, id, o, d, ret, w, st, stream);  // :231-258
                if (k + 1 >= bl) path_finish(P.out, g, ret, uint32_t(bl));  // ran to the limit (:260)
                else go = true;
            }
            if (P.block_cost) {  // calibration: the chunk's clocks split over its paths' cells
                const int32_t c = P.cell0 + int32_t(g / (64u * spp));
                int32_t fidx, bi;
                cell_of(P.frame_blocks, P.nblocks, c, fidx, bi);
                const uint32_t nv = n - base < 64u ? n - base : 64u;
                atomicAdd(P.block_cost + P.blocks[bi].base, (unsigned long long)((clock64() - clk0) / nv));
            }
        }
        path_enqueue<SORT>(P.q[k & 1], P.cap, &P.ctl[k], go, o, d, pix, g, ret, w, st, P.sort);
    }
    if (P.traced_rays) add_traced(P.traced_rays, traced, int(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (err && P.error_flag) atomicOr(P.error_flag, 1);
    if constexpr (COUNT) path_counters<COUNT>(P.counters, ct, traced);
}

// ------------------------------------------------------------------ per-pixel resolve
__global__ __launch_bounds__(256) void path_resolve_kernel(PathParams P) {
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int32_t cellrel = int32_t(blockIdx.x) * 4 + wave;
    if (cellrel >= P.ncells) return;
    int32_t fidx, bi;
    cell_of(P.frame_blocks, P.nblocks, P.cell0 + cellrel, fidx, bi);
    const DBlock blk = P.blocks[bi];
    const uint64_t mask = uint64_t(blk.mask_lo) | (uint64_t(blk.mask_hi) << 32);
    if (!((mask >> lane) & 1)) return;
    const atr_camera& cm = P.nfcam > 0 ? P.fcam[__builtin_amdgcn_readfirstlane(fidx)] : P.cam;
    const uint32_t spp = cm.samples_per_pixel;
    const bool traced = cm.bounce_limit > 0;
    const float4_t* src = P.out + int64_t(cellrel) * 64 * int64_t(spp) + lane;
    V3 col = mk(0.f, 0.f, 0.f);
    uint32_t casts = 0;
    // sample 0 first: kAllSky = every sample of the pixel met the sky with this colour
    const float4_t v0 = traced && spp > 0 ? src[0] : float4_t{0.f, 0.f, 0.f, 0.f};
    const bool all_sky = traced && spp > 0 && !cm.anti_aliasing && __float_as_uint(v0.w) == kAllSky;
    for (uint32_t s = 0; s < spp; ++s) {  // col += cast_ray(...) in sample order (:353-356)
        V3 c = mk(0.f, 0.f, 0.f);
        if (all_sky) {
            c = mk(v0.x, v0.y, v0.z);
        } else if (traced) {
            const float4_t v = s == 0 ? v0 : src[64 * int64_t(s)];
            c = mk(v.x, v.y, v.z);
            casts += __float_as_uint(v.w);
        }
        col = add(col, c);
    }
    col = divs(col, float(spp));  // :358
    const float cr = pl_max(0.0f, pl_min(col.x, 1.0f));
    const float cg = pl_max(0.0f, pl_min(col.y, 1.0f));
    const float cb = pl_max(0.0f, pl_min(col.z, 1.0f));
    const uint32_t r8 = uint32_t(cr * 255.0f) & 0xFFu, g8 = uint32_t(cg * 255.0f) & 0xFFu,
                   b8 = uint32_t(cb * 255.0f) & 0xFFu;
    const size_t o = out_index(P.layout, cm.width, P.frame_stride, blk, mask, lane, fidx);
    P.framebuffer[o] = b8 | (g8 << 8) | (r8 << 16);  // Set_Pixel (texture.h:27-38)
    if (!traced || spp == 0) {  // no camera ray ran: the miss record
        if (P.hit_face) P.hit_face[o] = 0xFFFFFFFFu;
        if (P.hit_t) P.hit_t[o] = kMaxFloat;
    }
    if (P.rgb) { P.rgb[3 * o] = col.x; P.rgb[3 * o + 1] = col.y; P.rgb[3 * o + 2] = col.z; }
    if (P.ray_casts) P.ray_casts[o] = casts;
}

// The resolve of a sample pass (atr_render_start_samples): the same cell and lane mapping and row
// reads, but the sums continue from the pixel's stored running sum (P.sample_sum, the f32 sum of
// samples [0, first_sample) in sample order; ray_casts likewise) instead of zero, go back there,
// and the mean is over first_sample + spp samples. The adds are those of a one-shot render of that
// many samples, in its order, so every output is bit-identical to it. A slot is read and written
// by the one lane that owns it: no atomics. The primary hit outputs belong to the frame's sample 0,
// so only the pass with first_sample == 0 writes the miss record.
__global__ __launch_bounds__(256) void path_resolve_accum_kernel(PathParams P) {
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int32_t cellrel = int32_t(blockIdx.x) * 4 + wave;
    if (cellrel >= P.ncells) return;
    int32_t fidx, bi;
    cell_of(P.frame_blocks, P.nblocks, P.cell0 + cellrel, fidx, bi);
    const DBlock blk = P.blocks[bi];
    const uint64_t mask = uint64_t(blk.mask_lo) | (uint64_t(blk.mask_hi) << 32);
    if (!((mask >> lane) & 1)) return;
    const atr_camera& cm = P.nfcam > 0 ? P.fcam[__builtin_amdgcn_readfirstlane(fidx)] : P.cam;
    const uint32_t spp = cm.samples_per_pixel, first = P.first_sample;
    const bool traced = cm.bounce_limit > 0;
    const float4_t* src = P.out + int64_t(cellrel) * 64 * int64_t(spp) + lane;
    const size_t o = out_index(P.layout, cm.width, P.frame_stride, blk, mask, lane, fidx);
    V3 col = mk(0.f, 0.f, 0.f);
    uint32_t casts = 0;
    if (first > 0) {
        col = mk(P.sample_sum[3 * o], P.sample_sum[3 * o + 1], P.sample_sum[3 * o + 2]);
        if (P.ray_casts) casts = P.ray_casts[o];
    }
    const float4_t v0 = traced && spp > 0 ? src[0] : float4_t{0.f, 0.f, 0.f, 0.f};
    const bool all_sky = traced && spp > 0 && !cm.anti_aliasing && __float_as_uint(v0.w) == kAllSky;
    for (uint32_t s = 0; s < spp; ++s) {  // col += cast_ray(...) in sample order (:353-356)
        V3 c = mk(0.f, 0.f, 0.f);
        if (all_sky) {
            c = mk(v0.x, v0.y, v0.z);
        } else if (traced) {
            const float4_t v = s == 0 ? v0 : src[64 * int64_t(s)];
            c = mk(v.x, v.y, v.z);
            casts += __float_as_uint(v.w);
        }
        col = add(col, c);
    }
    P.sample_sum[3 * o] = col.x; P.sample_sum[3 * o + 1] = col.y; P.sample_sum[3 * o + 2] = col.z;
    col = divs(col, float(first + spp));  // :358 over the samples so far
    const float cr = pl_max(0.0f, pl_min(col.x, 1.0f));
    const float cg = pl_max(0.0f, pl_min(col.y, 1.0f));
    const float cb = pl_max(0.0f, pl_min(col.z, 1.0f));
    const uint32_t r8 = uint32_t(cr * 255.0f) & 0xFFu, g8 = uint32_t(cg * 255.0f) & 0xFFu,
                   b8 = uint32_t(cb * 255.0f) & 0xFFu;
    P.framebuffer[o] = b8 | (g8 << 8) | (r8 << 16);  // Set_Pixel (texture.h:27-38)
    if (first == 0 && (!traced || spp == 0)) {  // no camera ray ran: the miss record
        if (P.hit_face) P.hit_face[o] = 0xFFFFFFFFu;
        if (P.hit_t) P.hit_t[o] = kMaxFloat;
    }
    if (P.rgb) { P.rgb[3 * o] = col.x; P.rgb[3 * o + 1] = col.y; P.rgb[3 * o + 2] = col.z; }
    if (P.ray_casts) P.ray_casts[o] = casts;
}

// ------------------------------------------------------------------ adaptive passes (PathLive)
// The live list of a batch, three phases like the queue sort's bin scan below. Phase 1: one
// wavefront per cell (a workgroup's four waves take a chunk's kLiveChunk cells, 16 each): lane pl
// reads its slot's sample count, the ballot is the cell's live mask, and the cell's group count
// goes where the scan will leave its first group; the chunk's sums go to part.
__global__ __launch_bounds__(256) void path_live_build(PathParams P) {
    __shared__ uint32_t ws[4][3];
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const uint32_t spp = P.cam.samples_per_pixel, first = P.first_sample;
    uint32_t tg = 0, tp = 0, tb = 0;
    for (int j = 0; j < kLiveChunk / 4; ++j) {
        const int32_t c = int32_t(blockIdx.x) * kLiveChunk + wave * (kLiveChunk / 4) + j;
        if (c >= P.ncells) break;  // whole wavefront
        int32_t fidx, bi;
        cell_of(P.frame_blocks, P.nblocks, P.cell0 + c, fidx, bi);
        const DBlock blk = P.blocks[bi];
        const uint64_t mask = uint64_t(blk.mask_lo) | (uint64_t(blk.mask_hi) << 32);
        bool live = (mask >> lane) & 1;
        if (live && first > 0) {  // a first pass reads no count; a converged count never equals first (bit 31)
            const size_t o = out_index(P.layout, P.cam.width, P.frame_stride, blk, mask, lane, fidx);
            live = P.live.count[o] == first;
        }
        const uint64_t lm = __ballot(live);
        const uint32_t np = uint32_t(__popcll(lm)), ng = (np * spp + 63u) / 64u;
        if (lane == 0) {
            P.live.mask[c] = uint2_t{uint32_t(lm), uint32_t(lm >> 32)};
            P.live.first[c] = ng;
        }
        tg += ng;
        tp += np;
        tb += np ? 1u : 0u;
    }
    if (lane == 0) { ws[wave][0] = tg; ws[wave][1] = tp; ws[wave][2] = tb; }
    __syncthreads();
    if (threadIdx.x < 3)
        P.live.part[3 * blockIdx.x + threadIdx.x] =
            ws[0][threadIdx.x] + ws[1][threadIdx.x] + ws[2][threadIdx.x] + ws[3][threadIdx.x];
}

// Phase 2 (one workgroup): the chunks' group sums scanned in place (exclusive), the batch's group
// total for the camera launch, and the pass's info counts (one thread adds the batch's: batches run
// one after another on the stream).
__global__ __launch_bounds__(1024) void path_live_part_scan(PathParams P) {
    __shared__ uint32_t ws[16], wp[16], wb[16];
    const int n = (P.ncells + kLiveChunk - 1) / kLiveChunk, per = (n + 1023) / 1024;
    const int i0 = int(threadIdx.x) * per, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t t = 0, p = 0, b = 0;
    for (int i = i0; i < i0 + per && i < n; ++i) {
        t += P.live.part[3 * i];
        p += P.live.part[3 * i + 1];
        b += P.live.part[3 * i + 2];
    }
    uint32_t inc = t;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t y = __shfl_up(inc, off);
        if (lane >= off) inc += y;
    }
    for (int off = 32; off > 0; off >>= 1) {
        p += __shfl_xor(p, off);
        b += __shfl_xor(b, off);
    }
    if (lane == 63) ws[wave] = inc;
    if (lane == 0) { wp[wave] = p; wb[wave] = b; }
    __syncthreads();
    uint32_t run = inc - t;
    for (int w = 0; w < wave; ++w) run += ws[w];
    for (int i = i0; i < i0 + per && i < n; ++i) {
        const uint32_t v = P.live.part[3 * i];
        P.live.part[3 * i] = run;
        run += v;
    }
    if (threadIdx.x == 0) {
        uint32_t groups = 0, pixels = 0, blocks = 0;
        for (int w = 0; w < 16; ++w) { groups += ws[w]; pixels += wp[w]; blocks += wb[w]; }
        P.live.ctl->groups = groups;
        P.live.ctl->claim = 0;
        P.live.info[0] += pixels;
        P.live.info[1] += blocks;
        P.live.info[2] += groups;
    }
}

// Phase 3: chunk b's cells, one per lane: each cell's first group (its chunk's start, then a scan
// over the wave, in cell order: the block list is in dispatch order and neighbouring cells share
// tree nodes), and the cell of every one of its groups.
__global__ __launch_bounds__(64) void path_live_scan(PathParams P) {
    const int lane = threadIdx.x & 63;
    const int32_t c = int32_t(blockIdx.x) * kLiveChunk + lane;
    const uint32_t ng = c < P.ncells ? P.live.first[c] : 0u;
    uint32_t inc = ng;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t y = __shfl_up(inc, off);
        if (lane >= off) inc += y;
    }
    if (c >= P.ncells) return;
    const uint32_t start = P.live.part[3 * blockIdx.x] + inc - ng;
    P.live.first[c] = start;
    for (uint32_t j = 0; j < ng; ++j) P.live.group[start + j] = uint32_t(c);
}

// The camera kernel of an adaptive pass: path_camera_kernel's ACCUM flavour (a sibling, so that
// kernel's instantiations stay what they were), but a wavefront takes one path group of the live
// list instead of 64 paths of every cell: path r of a cell is sample first_sample + r % spp of the
// pixel at the (r / spp)-th set bit of the cell's live mask. Result slots keep their layout, so
// the bounce kernels, the queue sort and the all-sky shortcut serve the pass as they are. The host
// does not know the group count: either the worst-case grid (every cell live) whose waves beyond
// the device-side total leave at once, or (ATR_ADAPT_PERSIST) persistent waves that claim groups
// the way the bounce kernel claims queue entries (DESIGN.md §4l has the measurement).
#ifndef ATR_ADAPT_PERSIST
#define ATR_ADAPT_PERSIST 0
#endif
constexpr bool kAdaptPersist = ATR_ADAPT_PERSIST != 0;
constexpr int kAdaptXcdChunk = 16;  // worst-case grid: the live groups dealt over the XCDs in chunks
template <bool SORT>
__global__ __launch_bounds__(256, 6) void path_camera_adaptive_kernel(PathParams P) {
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const uint32_t spp = uint32_t(__builtin_amdgcn_readfirstlane(int(P.cam.samples_per_pixel)));
    const uint32_t total = uint32_t(__builtin_amdgcn_readfirstlane(int(P.live.ctl->groups)));
    const DScene* S = uniform_global(P.scene);
    const atr_camera& cm = P.cam;
    const int32_t bl = cm.bounce_limit;
    uint32_t traced = 0;
    int err = 0;
    for (;;) {
        uint32_t gi;
        if constexpr (kAdaptPersist) {
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(&P.live.ctl->claim, 1u);
            gi = uint32_t(__builtin_amdgcn_readfirstlane(int(__shfl(int(base), 0))));
            if (gi >= total) break;
        } else {
            const int64_t wv =
                int64_t(remap_xcd(blockIdx.x, gridDim.x, P.xcd_chunk > 0 ? P.xcd_chunk : kAdaptXcdChunk)) * 4 + wave;
            if (wv >= int64_t(total)) break;  // whole wavefront
            gi = uint32_t(wv);
        }
        const int32_t cellrel = __builtin_amdgcn_readfirstlane(int(P.live.group[gi]));
        const uint32_t g0 = uint32_t(__builtin_amdgcn_readfirstlane(int(P.live.first[cellrel])));
        const uint2_t lv = P.live.mask[cellrel];
        const uint64_t live = uint64_t(uint32_t(__builtin_amdgcn_readfirstlane(int(lv.x)))) |
                              (uint64_t(uint32_t(__builtin_amdgcn_readfirstlane(int(lv.y)))) << 32);
        const uint32_t r = (gi - g0) * 64u + uint32_t(lane);  // path within the cell's live pixels
        const bool valid = r < uint32_t(__popcll(live)) * spp;
        const uint32_t k = valid ? r / spp : 0u;        // the pixel's rank among the live ones
        const uint32_t s = valid ? r - k * spp : 0u;    // its sample in the pass
        int pl = 0;  // the k-th set bit of the live mask
        {
            uint32_t rem = k;
#pragma unroll
            for (int w = 32; w > 0; w >>= 1) {
                const uint32_t cnt = uint32_t(__popcll((live >> pl) & ((uint64_t(1) << w) - 1)));
                if (rem >= cnt) { rem -= cnt; pl += w; }
            }
            pl &= 63;
        }
        const uint32_t g = uint32_t(cellrel) * 64u * spp + s * 64u + uint32_t(pl);  // result slot
        int32_t fidx, bi;
        cell_of(P.frame_blocks, P.nblocks, P.cell0 + cellrel, fidx, bi);
        const DBlock blk = P.blocks[bi];
        const uint64_t mask = uint64_t(blk.mask_lo) | (uint64_t(blk.mask_hi) << 32);
        const bool active = valid && ((live >> pl) & 1) && bl > 0;
        const int32_t x = blk.x0 + (pl & 7), y = blk.y0 + (pl >> 3);
        const int64_t pix = int64_t(y) * cm.width + x;
        uint64_t st, stream;
        const uint32_t fs = s + P.first_sample;  // the sample's index in the frame
        path_stream(P.seed, pix, fs, st, stream);
        const float film_y = -1.0f + 2.0f * (float(y) / float(cm.height));                                  // :317
        const float film_x = ((-1.0f + 2.0f * (float(x) / float(cm.width))) * cm.h_fov) * cm.aspect_ratio;  // :329
        const V3 eye = from(cm.eye), fc = from(cm.frame_center), cx = from(cm.camera_x), cy = from(cm.camera_y);
        V3 d;
        if (cm.anti_aliasing) {  // :338-347, the sample's two jitter draws
            const float xo = rand_bi(st, stream) * cm.half_pixel_width + film_x;
            const float yo = rand_bi(st, stream) * cm.half_pixel_height + film_y;
            d = unit(sub(add(add(fc, scale(cx, xo)), scale(cy, yo)), eye));
        } else {
            d = unit(sub(add(add(fc, scale(cx, film_x)), scale(cy, film_y)), eye));  // :350-351
        }
        Ctr ct;
        Isect id;
        id.type = T_NONE;
        intersect_scene<SCHED_HYBRID, FlavCamera, false>(S, eye, d, active, id, err, ct, P.hyb_a, P.hyb_b);
        bool go = false;
        V3 o = eye, ret = mk(0.f, 0.f, 0.f), w = mk(1.f, 1.f, 1.f);
        if (active) {
            if (fs == 0) {  // sample 0's camera ray: the primary hit outputs
                const size_t oi = out_index(P.layout, cm.width, P.frame_stride, blk, mask, pl, fidx);
                if (P.hit_face) P.hit_face[oi] = id.face;
                if (P.hit_t) P.hit_t[oi] = id.t;
            }
            const DMaterial& mat = S->mats[id.material];
            if (id.type == T_SKY) {  // :225-229 at i = 0
                ret = add(ret, had(w, mk(mat.ex, mat.ey, mat.ez)));
                if (cm.anti_aliasing || !ATR_SKY_ELIDE) path_finish(P.out, g, ret, 0u);
                else if (s == 0) path_finish(P.out, g, ret, kAllSky);  // the pixel's every sample (kAllSky)
            } else {
                bounce_shade(mat, id, o, d, ret, w, st, stream);  // :231-258
                if (bl <= 1) path_finish(P.out, g, ret, uint32_t(bl));  // ran to the limit (:260)
                else go = true;
            }
            traced += 1;
        }
        path_enqueue<SORT>(P.q[0], P.cap, &P.ctl[0], go, o, d, uint32_t(pix), g, ret, w, st, P.sort);
        if constexpr (!kAdaptPersist) break;
    }
    if (P.traced_rays) add_traced(P.traced_rays, traced, int(blockIdx.x * 4 + wave));
    if (err && P.error_flag) atomicOr(P.error_flag, 1);
}

// The resolve of an adaptive pass: path_resolve_accum_kernel's arithmetic for the live lanes of a
// live cell, then the slot's sample count and the stopping rule (atray.h: separately rounded f32
// operations, -ffp-contract=off). A lane that is not live reads and writes nothing. A slot is owned
// by one lane; the only atomic is the wave's count of newly converged pixels.
__global__ __launch_bounds__(256) void path_resolve_adaptive_kernel(PathParams P) {
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int32_t cellrel = int32_t(blockIdx.x) * 4 + wave;
    if (cellrel >= P.ncells) return;
    const uint2_t lv = P.live.mask[cellrel];
    const uint64_t live = uint64_t(lv.x) | (uint64_t(lv.y) << 32);
    if (live == 0) return;  // whole wavefront
    int32_t fidx, bi;
    cell_of(P.frame_blocks, P.nblocks, P.cell0 + cellrel, fidx, bi);
    const DBlock blk = P.blocks[bi];
    const uint64_t mask = uint64_t(blk.mask_lo) | (uint64_t(blk.mask_hi) << 32);
    const atr_camera& cm = P.cam;
    const uint32_t spp = cm.samples_per_pixel, first = P.first_sample;
    const bool traced = cm.bounce_limit > 0;
    bool conv = false;
    if ((live >> lane) & 1) {
        const float4_t* src = P.out + int64_t(cellrel) * 64 * int64_t(spp) + lane;
        const size_t o = out_index(P.layout, cm.width, P.frame_stride, blk, mask, lane, fidx);
        V3 col = mk(0.f, 0.f, 0.f), before = col;
        uint32_t casts = 0;
        if (first > 0) {
            col = mk(P.sample_sum[3 * o], P.sample_sum[3 * o + 1], P.sample_sum[3 * o + 2]);
            before = col;
            if (P.ray_casts) casts = P.ray_casts[o];
        }
        const float4_t v0 = traced ? src[0] : float4_t{0.f, 0.f, 0.f, 0.f};
        const bool all_sky = traced && !cm.anti_aliasing && __float_as_uint(v0.w) == kAllSky;
        for (uint32_t s = 0; s < spp; ++s) {  // col += cast_ray(...) in sample order (:353-356)
            V3 c = mk(0.f, 0.f, 0.f);
            if (all_sky) {
                c = mk(v0.x, v0.y, v0.z);
            } else if (traced) {
                const float4_t v = s == 0 ? v0 : src[64 * int64_t(s)];
                c = mk(v.x, v.y, v.z);
                casts += __float_as_uint(v.w);
            }
            col = add(col, c);
        }
        P.sample_sum[3 * o] = col.x; P.sample_sum[3 * o + 1] = col.y; P.sample_sum[3 * o + 2] = col.z;
        col = divs(col, float(first + spp));  // :358 over the samples so far
        const float cr = pl_max(0.0f, pl_min(col.x, 1.0f));
        const float cg = pl_max(0.0f, pl_min(col.y, 1.0f));
        const float cb = pl_max(0.0f, pl_min(col.z, 1.0f));
        const uint32_t r8 = uint32_t(cr * 255.0f) & 0xFFu, g8 = uint32_t(cg * 255.0f) & 0xFFu,
                       b8 = uint32_t(cb * 255.0f) & 0xFFu;
        P.framebuffer[o] = b8 | (g8 << 8) | (r8 << 16);  // Set_Pixel (texture.h:27-38)
        if (first == 0 && !traced) {  // no camera ray ran: the miss record
            if (P.hit_face) P.hit_face[o] = 0xFFFFFFFFu;
            if (P.hit_t) P.hit_t[o] = kMaxFloat;
        }
        if (P.rgb) { P.rgb[3 * o] = col.x; P.rgb[3 * o + 1] = col.y; P.rgb[3 * o + 2] = col.z; }
        if (P.ray_casts) P.ray_casts[o] = casts;
        if (first > 0) {  // the mean moved by less than tolerance x its brightness (false for a NaN)
            const V3 a = divs(before, float(first));
            const float dd = (fabsf(col.x - a.x) + fabsf(col.y - a.y)) + fabsf(col.z - a.z);
            const float l = ((col.x + col.y) + col.z) + 0.01f;
            conv = dd < P.live.tolerance * l;
        }
        P.live.count[o] = (first + spp) | (conv ? ATR_SAMPLES_CONVERGED : 0u);
    }
    const uint64_t cvm = __ballot(conv);
    if (lane == 0 && cvm) atomicAdd(P.live.info + 3, (unsigned long long)__popcll(cvm));
}

// ------------------------------------------------------------------ queue sort (PathSort)
// Level k's bins: block b sums hist[b x kSortChunk ..) into part[b].
__global__ __launch_bounds__(256) void path_sort_sums(PathSort so) {
    const uint4_t* h = reinterpret_cast<const uint4_t*>(so.hist + int64_t(blockIdx.x) * kSortChunk);
    uint32_t t = 0;
#pragma unroll
    for (int i = 0; i < kSortChunk / 1024; ++i) {
        const uint4_t v = h[i * 256 + threadIdx.x];
        t += v.x + v.y + v.z + v.w;
    }
    for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off);
    __shared__ uint32_t ws[4];
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) so.part[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}

// The block sums' exclusive scan, in place (one workgroup; nbins / kSortChunk <= 2^15 sums).
__global__ __launch_bounds__(1024) void path_sort_part_scan(PathSort so) {
    __shared__ uint32_t ws[16];
    const int n = so.nbins / kSortChunk, per = (n + 1023) / 1024;
    const int i0 = int(threadIdx.x) * per, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t t = 0;
    for (int i = i0; i < i0 + per && i < n; ++i) t += so.part[i];
    uint32_t inc = t;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t y = __shfl_up(inc, off);
        if (lane >= off) inc += y;
    }
    if (lane == 63) ws[wave] = inc;
    __syncthreads();
    uint32_t run = inc - t;
    for (int w = 0; w < wave; ++w) run += ws[w];
    for (int i = i0; i < i0 + per && i < n; ++i) {
        const uint32_t v = so.part[i];
        so.part[i] = run;
        run += v;
    }
}

// Block b: its bins' exclusive starts (its block's start, then a scan of its own kSortChunk bins,
// 16 per thread), and the bins zeroed for the next level.
__global__ __launch_bounds__(256) void path_sort_scan(PathSort so) {
    __shared__ uint32_t ws[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t pre = so.part[blockIdx.x];
    uint4_t* h = reinterpret_cast<uint4_t*>(so.hist + int64_t(blockIdx.x) * kSortChunk) + 4 * threadIdx.x;
    uint4_t* st = reinterpret_cast<uint4_t*>(so.start + int64_t(blockIdx.x) * kSortChunk) + 4 * threadIdx.x;
    uint4_t v[4];
    uint32_t t = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[i] = h[i];
        t += v[i].x + v[i].y + v[i].z + v[i].w;
    }
    uint32_t inc = t;  // inclusive scan over the wave, then over the four waves
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t y = __shfl_up(inc, off);
        if (lane >= off) inc += y;
    }
    if (lane == 63) ws[wave] = inc;
    __syncthreads();
    uint32_t run = pre + inc - t;
    for (int w = 0; w < wave; ++w) run += ws[w];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint4_t o;
        o.x = run; run += v[i].x;
        o.y = run; run += v[i].y;
        o.z = run; run += v[i].z;
        o.w = run; run += v[i].w;
        st[i] = o;
        h[i] = uint4_t{0u, 0u, 0u, 0u};
    }
}

// Level k's key order: perm[start[key] + rank] = entry, for every entry of the level (grid-stride
// over its tail). A slot outside the tail, impossible for consistent keys and ranks, is flagged.
__global__ __launch_bounds__(256) void path_sort_rank(PathParams P) {
    const int32_t k = P.bounce;
    const uint32_t n = uint32_t(__builtin_amdgcn_readfirstlane(int(P.ctl[k].tail)));
    const PathSort so = P.sort;
    // four entries per lane per step: their loads in flight together (c4 +0.2% over one)
    constexpr int U = 4;
    const uint32_t stride = gridDim.x * 256u;
    for (uint32_t e0 = blockIdx.x * 256u + threadIdx.x; e0 < n; e0 += U * stride) {
        uint2_t kr[U];
        uint32_t st[U];
#pragma unroll
        for (int j = 0; j < U; ++j) {
            const uint32_t e = e0 + uint32_t(j) * stride;
            kr[j] = e < n ? so.kr[e] : uint2_t{0u, 0u};
        }
#pragma unroll
        for (int j = 0; j < U; ++j) st[j] = so.start[kr[j].x];
#pragma unroll
        for (int j = 0; j < U; ++j) {
            const uint32_t e = e0 + uint32_t(j) * stride;
            const uint32_t dst = st[j] + kr[j].y;
            if (e >= n) continue;
            if (dst < n) so.perm[dst] = e;
            else if (P.error_flag) atomicOr(P.error_flag, 2);
        }
    }
}

// Occupancy (waves/SIMD) of the two trace kernels, 5..7 (the LDS limit is 7: 22.5 KB per
// workgroup); tuning path_camera_occ / path_bounce_occ pick another (0 = these defaults). The
// camera kernel at 7 spills 21 dwords whose write-backs reach HBM (14.9 GB per c4 frame against
// 4.6 GB at 6) and is no faster.
constexpr int kCameraOcc = 6;
#ifndef ATR_BOUNCE_OCC
#define ATR_BOUNCE_OCC 7
#endif
constexpr int kBounceOcc = ATR_BOUNCE_OCC;
#if ATR_BOUNCE_OCC == 8  // experiment: the bounce kernel at 8 waves/SIMD (needs a 6-leaf buffer's LDS)
#define ATR_PATH_BOUNCE8(SORT) template __global__ void path_bounce_kernel<false, 8, SORT>(PathParams);
#else
#define ATR_PATH_BOUNCE8(SORT)
#endif
#define ATR_PATH_KERNELS(SORT)                                                  \
    template __global__ void path_camera_kernel<false, 5, SORT>(PathParams);    \
    template __global__ void path_camera_kernel<false, 6, SORT>(PathParams);    \
    template __global__ void path_camera_kernel<false, 7, SORT>(PathParams);    \
    template __global__ void path_camera_kernel<true, 4, SORT>(PathParams);     \
    template __global__ void path_bounce_kernel<false, 5, SORT>(PathParams);    \
    template __global__ void path_bounce_kernel<false, 6, SORT>(PathParams);    \
    template __global__ void path_bounce_kernel<false, 7, SORT>(PathParams);    \
    ATR_PATH_BOUNCE8(SORT)                                                      \
    template __global__ void path_bounce_kernel<true, 4, SORT>(PathParams);
ATR_PATH_KERNELS(false)
ATR_PATH_KERNELS(true)
#undef ATR_PATH_KERNELS
// the sample passes' camera kernel, at the default occupancy (the bounce kernels serve them as they are)
template __global__ void path_camera_kernel<false, kCameraOcc, false, true>(PathParams);
template __global__ void path_camera_kernel<false, kCameraOcc, true, true>(PathParams);
// the adaptive passes' camera kernel (its launch bounds name the same occupancy)
static_assert(kCameraOcc == 6, "path_camera_adaptive_kernel's launch bounds");
template __global__ void path_camera_adaptive_kernel<false>(PathParams);
template __global__ void path_camera_adaptive_kernel<true>(PathParams);

}  // namespace atr

// ------------------------------------------------------------------ launchers used by capi.cpp
namespace {
template <bool SORT>
void launch_camera(const atr::PathParams& P, int occ, dim3 g, hipStream_t s) {
    const dim3 b(256);
    if (P.sample_sum) hipLaunchKernelGGL((atr::path_camera_kernel<false, atr::kCameraOcc, SORT, true>), g, b, 0, s, P);
    else if (P.counters) hipLaunchKernelGGL((atr::path_camera_kernel<true, 4, SORT>), g, b, 0, s, P);
    else if (occ == 5) hipLaunchKernelGGL((atr::path_camera_kernel<false, 5, SORT>), g, b, 0, s, P);
    else if (occ == 6) hipLaunchKernelGGL((atr::path_camera_kernel<false, 6, SORT>), g, b, 0, s, P);
    else hipLaunchKernelGGL((atr::path_camera_kernel<false, 7, SORT>), g, b, 0, s, P);
}
template <bool SORT>
void launch_bounce(const atr::PathParams& P, int occ, dim3 g, hipStream_t s) {
    const dim3 b(256);
    if (P.counters) hipLaunchKernelGGL((atr::path_bounce_kernel<true, 4, SORT>), g, b, 0, s, P);
    else if (occ == 5) hipLaunchKernelGGL((atr::path_bounce_kernel<false, 5, SORT>), g, b, 0, s, P);
    else if (occ == 6) hipLaunchKernelGGL((atr::path_bounce_kernel<false, 6, SORT>), g, b, 0, s, P);
#if ATR_BOUNCE_OCC == 8
    else if (occ == 8) hipLaunchKernelGGL((atr::path_bounce_kernel<false, 8, SORT>), g, b, 0, s, P);
#endif
    else hipLaunchKernelGGL((atr::path_bounce_kernel<false, 7, SORT>), g, b, 0, s, P);
}
}  // namespace

// With P.sort.bits > 0 the launch reads and writes entry-major queues and its survivors record
// their sort keys and ranks (the queue sort, PathSort).
extern "C" hipError_t atr_launch_path_camera(const atr::PathParams& P, int occ, hipStream_t s) {
    const int64_t waves = int64_t(P.ncells) * P.cam.samples_per_pixel;
    if (waves <= 0) return hipSuccess;
    const dim3 g(unsigned((waves + 3) / 4));
    if (!occ) occ = atr::kCameraOcc;
    if (P.sort.bits) launch_camera<true>(P, occ, g, s);
    else launch_camera<false>(P, occ, g, s);
    return hipGetLastError();
}

// Persistent: `ncu` x occupancy workgroups (4 waves each, one per SIMD) claim the queue 64 entries
// at a time.
extern "C" hipError_t atr_launch_path_bounce(const atr::PathParams& P, int ncu, int occ, hipStream_t s) {
    if (!occ) occ = atr::kBounceOcc;
    const dim3 g(unsigned(ncu) * unsigned(P.counters ? 4 : occ));
    if (P.sort.bits) launch_bounce<true>(P, occ, g, s);
    else launch_bounce<false>(P, occ, g, s);
    return hipGetLastError();
}

// The bin scan (hist -> start, hist zeroed): its three kernels take a PathSort and nothing else, so
// the ray queries' batch order (query.hip) runs them too.
extern "C" hipError_t atr_launch_sort_bins(const atr::PathSort& so, hipStream_t s) {
    const unsigned blocks = unsigned(so.nbins / atr::kSortChunk);
    hipLaunchKernelGGL(atr::path_sort_sums, dim3(blocks), dim3(256), 0, s, so);
    hipLaunchKernelGGL(atr::path_sort_part_scan, dim3(1), dim3(1024), 0, s, so);
    hipLaunchKernelGGL(atr::path_sort_scan, dim3(blocks), dim3(256), 0, s, so);
    return hipGetLastError();
}

extern "C" hipError_t atr_launch_path_sort(const atr::PathParams& P, int ncu, hipStream_t s) {
    const hipError_t e = atr_launch_sort_bins(P.sort, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(atr::path_sort_rank, dim3(unsigned(ncu) * 16u), dim3(256), 0, s, P);
    return hipGetLastError();
}

// An adaptive pass (P.live): the batch's live list, its camera launch (the worst-case grid, or `ncu`
// x occupancy persistent workgroups) and its resolve.
extern "C" hipError_t atr_launch_path_live(const atr::PathParams& P, hipStream_t s) {
    if (P.ncells <= 0) return hipSuccess;
    const unsigned chunks = unsigned((P.ncells + atr::kLiveChunk - 1) / atr::kLiveChunk);
    hipLaunchKernelGGL(atr::path_live_build, dim3(chunks), dim3(256), 0, s, P);
    hipLaunchKernelGGL(atr::path_live_part_scan, dim3(1), dim3(1024), 0, s, P);
    hipLaunchKernelGGL(atr::path_live_scan, dim3(chunks), dim3(64), 0, s, P);
    return hipGetLastError();
}

extern "C" hipError_t atr_launch_path_camera_adaptive(const atr::PathParams& P, int ncu, hipStream_t s) {
    const int64_t waves = int64_t(P.ncells) * P.cam.samples_per_pixel;
    if (waves <= 0) return hipSuccess;
    const dim3 g(atr::kAdaptPersist ? unsigned(ncu) * unsigned(atr::kCameraOcc) : unsigned((waves + 3) / 4));
    if (P.sort.bits) hipLaunchKernelGGL(atr::path_camera_adaptive_kernel<true>, g, dim3(256), 0, s, P);
    else hipLaunchKernelGGL(atr::path_camera_adaptive_kernel<false>, g, dim3(256), 0, s, P);
    return hipGetLastError();
}

extern "C" hipError_t atr_launch_path_resolve_adaptive(const atr::PathParams& P, hipStream_t s) {
    if (P.ncells <= 0) return hipSuccess;
    hipLaunchKernelGGL(atr::path_resolve_adaptive_kernel, dim3(unsigned((P.ncells + 3) / 4)), dim3(256), 0, s, P);
    return hipGetLastError();
}

extern "C" hipError_t atr_launch_path_resolve(const atr::PathParams& P, hipStream_t s) {
    if (P.ncells <= 0) return hipSuccess;
    const dim3 g(unsigned((P.ncells + 3) / 4));
    if (P.sample_sum) hipLaunchKernelGGL(atr::path_resolve_accum_kernel, g, dim3(256), 0, s, P);
    else hipLaunchKernelGGL(atr::path_resolve_kernel, g, dim3(256), 0, s, P);
    return hipGetLastError();
}
