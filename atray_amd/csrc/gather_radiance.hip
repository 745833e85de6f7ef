// gather_radiance.hip -- hemisphere radiance gathered on the device (atr_gather_radiance, DESIGN.md
// §4q): for a batch of surface points with unit normals, every sample is the renderer's own path
// after a diffuse hit at the point -- the direction drawn in registers on the (point, sample) stream
// (engine.h gather_dir_state), then cast_ray from the point along it, continued on that stream. The
// path engine (paths.hip) entered from a point array; no ray array exists anywhere.
//   gather_radiance_entry_kernel    persistent waves claim 64 items of the flattened (point, sample)
//                                   index at a time, one lane per item: the lane tests its point,
//                                   draws its direction, traces it (FLAT's dealt rounds in the bounce
//                                   flavour), applies the first shading step and either finishes the
//                                   path in the item's result slot or appends it to queue 0. A sample
//                                   that is not traced writes the untraced marker there, an item of
//                                   an invalid point the invalid marker;
//   (the bounce levels)             path_bounce_kernel and the queue sort, as they are, on a PathParams;
//   gather_radiance_resolve_kernel  one wave per point: rows of 64 consecutive samples' slots (1 KB,
//                                   coalesced), the traced ones packed in sample order into the
//                                   wave's LDS and added from there by lane 0; the sum, the sample
//                                   and cast counts, the mean, the invalid byte and the row's
//                                   colours (sample_rgb) come out.
//                                   Every slot has one owner: no atomics.
// A file of its own: the other kernels' code objects are what they were.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "launch.h"
#include "paths.h"
#include "scan.h"

namespace atr {

// Waves/SIMD: the radiance query's 7 (radiance.hip kRadianceOcc), whose scan and LDS the entry kernel has.
#ifndef ATR_GATHER_RADIANCE_OCC  // experiment builds
#define ATR_GATHER_RADIANCE_OCC 7
#endif
constexpr int kGatherRadianceOcc = ATR_GATHER_RADIANCE_OCC;

template <bool SORT>
__global__ __launch_bounds__(256, kGatherRadianceOcc) void gather_radiance_entry_kernel(GatherRadianceParams P) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t n = uint32_t(__builtin_amdgcn_readfirstlane(int(P.n)));
    const uint32_t ns = uint32_t(__builtin_amdgcn_readfirstlane(int(P.nsamples)));
    const int32_t bl = P.bounce_limit;
    const DScene* S = uniform_global(P.scene);
    int err = 0;
    Ctr ct;
    uint32_t traced = 0;
    for (;;) {  // every wave leaves once the batch is claimed: the exit every wave reaches
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(&P.ctl[0].head, 64u);
        base = uint32_t(__builtin_amdgcn_readfirstlane(int(__shfl(int(base), 0))));
        if (base >= n) break;
        const uint32_t idx = base + lane;  // the item, and its result slot
        const bool in = idx < n;
        // (point, sample) of the item; a lane past the batch's end reads the wave's first point (in
        // bounds) and writes nothing
        const uint32_t c = in ? idx : base;
        const uint32_t i = c / ns, s = c - i * ns;
        const size_t e = size_t(P.point0) + i;  // the point's index in the call's arrays
        const V3 p = mk(P.p[3 * e], P.p[3 * e + 1], P.p[3 * e + 2]);
        const V3 nn = mk(P.nrm[3 * e], P.nrm[3 * e + 1], P.nrm[3 * e + 2]);
        const bool pok = in && ray_ok(p, nn);  // a finite point, a unit normal
        // the placeholder of an inactive lane
        V3 o = mk(0.f, 0.f, 0.f), d = mk(0.f, 0.f, 1.f), g = mk(0.f, 0.f, 0.f);
        uint64_t st = 0, stream = 1;
        bool ok = false;  // traced: a valid point, a direction that passes the ray test, above the plane
        if (pok) {
            g = gather_dir_state(P.seed, P.point_base + int64_t(e), P.first_sample + s, nn, st, stream);
            ok = ray_ok(p, g) && dot(g, nn) > 0.0f;
            if (ok) { o = p; d = g; }
        }
        // every generated direction of a valid point, traced or not (zeros for an invalid point): stored
        // before the scan
        if (in && P.dirs) {
            float* q = P.dirs + 3 * (size_t(P.point0) * ns + idx);
            q[0] = g.x;
            q[1] = g.y;
            q[2] = g.z;
        }
        const SceneHit sh = intersect_models<SCHED_FLAT, FlavBounce, false>(S, o, d, ok, err, ct, P.hyb_a, P.hyb_b);
        // the point is read again after the query instead of being held through it (as radiance.hip
        // reads its ray): the memory clobber keeps the loads here, the opaque copy of the index keeps
        // their addresses from being formed before the query
        uint32_t ia = i;
        __asm__ volatile("" : "+v"(ia) :: "memory");
        const uint32_t pix = uint32_t(uint64_t(P.point_base) + P.point0 + ia);  // the stream index, 32 bits
        bool go = false;
        V3 ret = mk(0.f, 0.f, 0.f), w = mk(1.f, 1.f, 1.f);
        if (ok) {
            traced += 1;
            const size_t ea = size_t(P.point0) + ia;
            o = mk(P.p[3 * ea], P.p[3 * ea + 1], P.p[3 * ea + 2]);
            Isect id;
            scene_finish(S, o, d, sh.best, sh.face, sh.fu, sh.fv, sh.nm, id);  // renderer.cpp:86-160
            const DMaterial& mat = S->mats[id.material];
            if (id.type == T_SKY) {  // :225-229 at i = 0
                ret = add(ret, had(w, mk(mat.ex, mat.ey, mat.ez)));
                path_finish(P.out, idx, ret, 0u);
            } else {
                bounce_shade(mat, id, o, d, ret, w, st, stream);  // :231-258, on the stream after the draws
                if (bl <= 1) path_finish(P.out, idx, ret, 1u);  // ran to the limit (:260)
                else go = true;
            }
        } else if (in) {
            path_finish(P.out, idx, mk(0.f, 0.f, 0.f), pok ? kSampleUntraced : kRayInvalid);
        }
        path_enqueue<SORT>(P.q0, P.cap, &P.ctl[0], go, o, d, pix, idx, ret, w, st, P.sort);
    }
    if (P.traced_rays) add_traced(P.traced_rays, traced, int(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (err && P.error_flag) atomicOr(P.error_flag, 1);
}

template __global__ void gather_radiance_entry_kernel<false>(GatherRadianceParams);
template __global__ void gather_radiance_entry_kernel<true>(GatherRadianceParams);

// The wave's own LDS traffic in program order for the compiler too: a row's writes by many lanes before
// lane 0's reads, and those before the next row's writes (the hardware runs a wave's LDS operations
// in order).
__device__ __forceinline__ void wave_lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One wave per point of the batch. The adds are cast_ray's colours in sample order, from zero or from
// the caller's running sum. A row of 64 slots is loaded by the lanes (1 KB, coalesced); its traced
// lanes write their slots to the wave's 1 KB of LDS, each at its rank among them (the ballot's bits
// below it), so the row's traced samples lie there in sample order without gaps; lane 0 then adds
// them one after the other, eight LDS reads in flight at a time, while the next row's loads are on
// their way. An untraced sample is never written there: it adds nothing and counts nowhere. The
// sample and cast counts are integer sums and need no order: a popcount per row, a wave sum at the
// end. (The first version broadcast each traced lane's colour with v_readlane to a sum that every
// lane held: 13 instructions per sample against 3 here)
__global__ __launch_bounds__(256) void gather_radiance_resolve_kernel(GatherRadianceParams P) {
    __shared__ float4_t rows[4][64];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t i = uint32_t(__builtin_amdgcn_readfirstlane(int(blockIdx.x * 4u + (threadIdx.x >> 6))));
    if (i >= P.npoints) return;  // whole wavefront
    const uint32_t ns = uint32_t(__builtin_amdgcn_readfirstlane(int(P.nsamples))), first = P.first_sample;
    const float4_t* src = P.out + size_t(i) * ns;
    const size_t r = size_t(P.point0) + i;
    float* srgb = P.sample_rgb ? P.sample_rgb + 3 * (r * ns) : nullptr;
    if (__float_as_uint(src[0].w) == kRayInvalid) {  // not traced: zeros from a first call, else what was there
        for (uint32_t s = lane; srgb && s < ns; s += 64u) {
            srgb[3 * size_t(s)] = 0.f;
            srgb[3 * size_t(s) + 1] = 0.f;
            srgb[3 * size_t(s) + 2] = 0.f;
        }
        if (lane != 0) return;
        if (first == 0) {
            if (P.rgb) { P.rgb[3 * r] = 0.f; P.rgb[3 * r + 1] = 0.f; P.rgb[3 * r + 2] = 0.f; }
            if (P.sum) { P.sum[3 * r] = 0.f; P.sum[3 * r + 1] = 0.f; P.sum[3 * r + 2] = 0.f; }
            if (P.samples) P.samples[r] = 0u;
            if (P.ray_casts) P.ray_casts[r] = 0u;
        }
        if (P.invalid) P.invalid[r] = 1;
        return;
    }
    float4_t* buf = rows[threadIdx.x >> 6];
    V3 col = mk(0.f, 0.f, 0.f);  // lane 0's
    uint32_t cnt = 0, casts = 0;  // cnt: every lane's; casts: a partial sum per lane
    if (first > 0) {  // the host requires sum and samples then
        col = mk(P.sum[3 * r], P.sum[3 * r + 1], P.sum[3 * r + 2]);
        cnt = P.samples[r];
        if (P.ray_casts && lane == 0) casts = P.ray_casts[r];
    }
    const float4_t none = float4_t{0.f, 0.f, 0.f, __uint_as_float(kSampleUntraced)};
    float4_t v = none;
    if (lane < ns) v = src[lane];
    for (uint32_t row = 0; row < ns; row += 64u) {  // wave-uniform
        const uint32_t s = row + lane;
        const bool have = s < ns;
        const bool tr = have && __float_as_uint(v.w) != kSampleUntraced;
        if (have && srgb) {
            srgb[3 * size_t(s)] = tr ? v.x : 0.f;
            srgb[3 * size_t(s) + 1] = tr ? v.y : 0.f;
            srgb[3 * size_t(s) + 2] = tr ? v.z : 0.f;
        }
        const unsigned long long m = __ballot(tr);
        const uint32_t k = uint32_t(__popcll(m));  // the row's traced samples
        if (tr) {
            buf[__builtin_amdgcn_mbcnt_hi(uint32_t(m >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(m), 0u))] = v;
            casts += __float_as_uint(v.w);
        }
        cnt += k;
        float4_t vn = none;  // the next row's slots
        if (s + 64u < ns) vn = src[s + 64u];
        wave_lds_order();
        if (lane == 0) {
            uint32_t j = 0;
            for (; j + 8u <= k; j += 8u) {  // whole eights: no test between the adds
                float4_t c[8];
#pragma unroll
                for (uint32_t u = 0; u < 8u; ++u) c[u] = buf[j + u];
#pragma unroll
                for (uint32_t u = 0; u < 8u; ++u) col = add(col, mk(c[u].x, c[u].y, c[u].z));
            }
            if (j < k) {  // the last one to seven: read as an eight (inside the row's 64 entries), added under a test
                float4_t c[8];
#pragma unroll
                for (uint32_t u = 0; u < 8u; ++u) c[u] = buf[j + u];
#pragma unroll
                for (uint32_t u = 0; u < 8u; ++u)
                    if (j + u < k) col = add(col, mk(c[u].x, c[u].y, c[u].z));
            }
        }
        wave_lds_order();
        v = vn;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) casts += __shfl_xor(casts, off);
    if (lane != 0) return;
    if (P.sum) { P.sum[3 * r] = col.x; P.sum[3 * r + 1] = col.y; P.sum[3 * r + 2] = col.z; }
    if (P.samples) P.samples[r] = cnt;
    if (P.ray_casts) P.ray_casts[r] = casts;
    if (P.rgb) {
        const V3 mean = cnt ? divs(col, float(cnt)) : mk(0.f, 0.f, 0.f);
        P.rgb[3 * r] = mean.x;
        P.rgb[3 * r + 1] = mean.y;
        P.rgb[3 * r + 2] = mean.z;
    }
    if (P.invalid) P.invalid[r] = 0;
}

}  // namespace atr

// Persistent, sized like the radiance query's launch: `ncu` x occupancy workgroups (4 waves each), at
// most one wave per 64 items.
extern "C" hipError_t atr_launch_gather_radiance_entry(const atr::GatherRadianceParams& P, int ncu, hipStream_t s) {
    const uint64_t need = (uint64_t(P.n) + 255u) / 256u;
    const dim3 g(unsigned(std::min<uint64_t>(uint64_t(ncu) * atr::kGatherRadianceOcc, need))), b(256);
    if (P.sort.bits > 0) hipLaunchKernelGGL(atr::gather_radiance_entry_kernel<true>, g, b, 0, s, P);
    else hipLaunchKernelGGL(atr::gather_radiance_entry_kernel<false>, g, b, 0, s, P);
    return hipGetLastError();
}

extern "C" hipError_t atr_launch_gather_radiance_resolve(const atr::GatherRadianceParams& P, hipStream_t s) {
    if (P.npoints == 0) return hipSuccess;
    hipLaunchKernelGGL(atr::gather_radiance_resolve_kernel, dim3((P.npoints + 3u) / 4u), dim3(256), 0, s, P);
    return hipGetLastError();
}
