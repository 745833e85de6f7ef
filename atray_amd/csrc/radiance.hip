// radiance.hip -- path-traced radiance along the caller's rays (atr_radiance_rays):
// the path engine (paths.hip) entered from a ray array instead of a camera and a tile list.
//   radiance_entry_kernel    persistent waves claim 64 consecutive rays (a group, the engine's "cell"),
//                            one lane per ray: the lane tests its ray, traces it ONCE (FLAT's dealt rounds
//                            in the bounce flavour: the batch is incoherent by assumption), and then,
//                            sample by sample, seeds the (ray, sample) stream, applies the first shading
//                            step to a copy of the hit and either finishes the path or appends it to
//                            queue 0. A first segment that meets the sky writes sample 0's slot alone,
//                            with the all-sky marker (paths.h); a ray that fails the test writes the
//                            invalid marker there and nothing else;
//   (the bounce levels)      path_bounce_kernel and the queue sort, as they are, on a PathParams;
//   radiance_resolve_kernel  one lane per ray: the ray's slots summed in sample order from zero or from
//                            the caller's running sum, the mean, ray_casts and the invalid byte, written
//                            at the ray's input index. Every slot has one owner: no atomics.
// A file of its own: the other kernels' code objects are what they were.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "launch.h"
#include "paths.h"
#include "scan.h"

namespace atr {

// Waves/SIMD: the ray query's 7 (query.hip kQueryOcc), whose scan and LDS the entry kernel has. The
// 72 registers of that occupancy are the scan's; the sample loop after it holds the hit record, the
// material and the ray, and the allocator leaves a few 8-byte reloads in it (DESIGN.md §4p has the
// figures).
#ifndef ATR_RADIANCE_OCC  // experiment builds
#define ATR_RADIANCE_OCC 7
#endif
constexpr int kRadianceOcc = ATR_RADIANCE_OCC;

template <bool SORT>
__global__ __launch_bounds__(256, kRadianceOcc) void radiance_entry_kernel(RadianceParams P) {
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
        const uint32_t i = base + lane;
        const bool in = i < n;
        const uint32_t e = P.ray0 + i;  // the ray's index in the call's arrays
        V3 o = mk(0.f, 0.f, 0.f), d = mk(0.f, 0.f, 1.f);
        bool ok = false;
        if (in) {
            V3 ro, rd;
            load_ray(P.o, P.d, e, ro, rd);
            ok = ray_ok(ro, rd);
            if (ok) { o = ro; d = rd; }  // a ray that fails keeps the placeholder: an inactive lane
        }
        const SceneHit sh = intersect_models<SCHED_FLAT, FlavBounce, false>(S, o, d, ok, err, ct, P.hyb_a, P.hyb_b);
        // the ray is read again after the query instead of being held through it (as the bounce
        // kernel does): the memory clobber keeps the loads here, the opaque copy of the index keeps
        // their addresses from being formed before the query
        uint32_t ea = e;
        __asm__ volatile("" : "+v"(ea) :: "memory");
        // sample 0's slot of the ray: group x 64 nsamples + lane (base is a multiple of 64)
        const uint32_t g0 = base * ns + lane;
        bool hit = false;
        Isect id;
        id.type = T_NONE;
        if (ok) {
            traced += 1;
            load_ray(P.o, P.d, ea, o, d);
            scene_finish(S, o, d, sh.best, sh.face, sh.fu, sh.fv, sh.nm, id);  // renderer.cpp:86-160
            if (id.type == T_SKY) {  // :225-229 at i = 0: every sample's colour (kAllSky)
                const DMaterial& sky = S->mats[id.material];
                const V3 ret = add(mk(0.f, 0.f, 0.f), had(mk(1.f, 1.f, 1.f), mk(sky.ex, sky.ey, sky.ez)));
                path_finish(P.out, g0, ret, kAllSky);
            } else {
                hit = true;
            }
        } else if (in) {
            path_finish(P.out, g0, mk(0.f, 0.f, 0.f), kRayInvalid);
        }
        if (__ballot(hit) == 0) continue;  // whole wavefront: no path starts here
        const int64_t pix = P.ray_base + int64_t(ea);
        // a copy: not re-read after the queue's stores. (Reading the ray and the material again for
        // every sample, the bounce kernel's reload, left the loop's scratch traffic where it was:
        // DESIGN.md §4p.)
        const DMaterial mat = S->mats[hit ? id.material : 0];
        for (uint32_t s = 0; s < ns; ++s) {  // wave-uniform: the lanes without a hit append nothing
            V3 po = o, pd = d, ret = mk(0.f, 0.f, 0.f), w = mk(1.f, 1.f, 1.f);
            uint64_t st = 0, stream = 1;
            bool go = false;
            const uint32_t g = g0 + s * 64u;
            if (hit) {
                path_stream(P.seed, pix, P.first_sample + s, st, stream);
                bounce_shade(mat, id, po, pd, ret, w, st, stream);  // :231-258
                if (bl <= 1) path_finish(P.out, g, ret, uint32_t(bl));  // ran to the limit (:260)
                else go = true;
            }
            path_enqueue<SORT>(P.q0, P.cap, &P.ctl[0], go, po, pd, uint32_t(pix), g, ret, w, st, P.sort);
        }
    }
    if (P.traced_rays) add_traced(P.traced_rays, traced, int(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (err && P.error_flag) atomicOr(P.error_flag, 1);
}

template __global__ void radiance_entry_kernel<false>(RadianceParams);
template __global__ void radiance_entry_kernel<true>(RadianceParams);

// One lane per ray of the batch. The adds are path_resolve_accum_kernel's: col += cast_ray(...) in
// sample order (renderer.cpp:353-356), from the stored running sum when first_sample > 0, the mean
// over first_sample + nsamples samples (:358), not clamped.
__global__ __launch_bounds__(256) void radiance_resolve_kernel(RadianceParams P) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= P.n) return;
    const uint32_t ns = P.nsamples, first = P.first_sample;
    const float4_t* src = P.out + int64_t(i >> 6) * 64 * int64_t(ns) + (i & 63u);
    const size_t r = size_t(P.ray0) + i;
    const float4_t v0 = src[0];
    const uint32_t mark = __float_as_uint(v0.w);
    if (mark == kRayInvalid) {  // not traced: zeros from a first call, else what was there
        if (first == 0) {
            if (P.rgb) { P.rgb[3 * r] = 0.f; P.rgb[3 * r + 1] = 0.f; P.rgb[3 * r + 2] = 0.f; }
            if (P.sum) { P.sum[3 * r] = 0.f; P.sum[3 * r + 1] = 0.f; P.sum[3 * r + 2] = 0.f; }
            if (P.ray_casts) P.ray_casts[r] = 0u;
        }
        if (P.invalid) P.invalid[r] = 1;
        return;
    }
    V3 col = mk(0.f, 0.f, 0.f);
    uint32_t casts = 0;
    if (first > 0) {  // the host requires sum then
        col = mk(P.sum[3 * r], P.sum[3 * r + 1], P.sum[3 * r + 2]);
        if (P.ray_casts) casts = P.ray_casts[r];
    }
    const bool all_sky = mark == kAllSky;
    for (uint32_t s = 0; s < ns; ++s) {
        V3 c;
        if (all_sky) {
            c = mk(v0.x, v0.y, v0.z);
        } else {
            const float4_t v = s == 0 ? v0 : src[64 * int64_t(s)];
            c = mk(v.x, v.y, v.z);
            casts += __float_as_uint(v.w);
        }
        col = add(col, c);
    }
    if (P.sum) { P.sum[3 * r] = col.x; P.sum[3 * r + 1] = col.y; P.sum[3 * r + 2] = col.z; }
    col = divs(col, float(first + ns));
    if (P.rgb) { P.rgb[3 * r] = col.x; P.rgb[3 * r + 1] = col.y; P.rgb[3 * r + 2] = col.z; }
    if (P.ray_casts) P.ray_casts[r] = casts;
    if (P.invalid) P.invalid[r] = 0;
}

}  // namespace atr

// Persistent, sized like the ray query's launch: `ncu` x occupancy workgroups (4 waves each), at most
// one wave per group of 64 rays.
extern "C" hipError_t atr_launch_radiance_entry(const atr::RadianceParams& P, int ncu, hipStream_t s) {
    const uint64_t need = (uint64_t(P.n) + 255u) / 256u;
    const dim3 g(unsigned(std::min<uint64_t>(uint64_t(ncu) * atr::kRadianceOcc, need))), b(256);
    if (P.sort.bits > 0) hipLaunchKernelGGL(atr::radiance_entry_kernel<true>, g, b, 0, s, P);
    else hipLaunchKernelGGL(atr::radiance_entry_kernel<false>, g, b, 0, s, P);
    return hipGetLastError();
}

extern "C" hipError_t atr_launch_radiance_resolve(const atr::RadianceParams& P, hipStream_t s) {
    if (P.n == 0) return hipSuccess;
    hipLaunchKernelGGL(atr::radiance_resolve_kernel, dim3((P.n + 255u) / 256u), dim3(256), 0, s, P);
    return hipGetLastError();
}
