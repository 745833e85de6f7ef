// occlusion.hip -- occlusion queries (atr_occluded_rays): for a batch of the caller's
// rays, is there any hit with kTol < t < t_max -- the reference's own traversal with *td.closest
// started at the ray's t_max instead of MAX_FLOAT, one byte per ray.
//   ray_occlusion_kernel  persistent waves claim 64 positions of the batch at a time (the batch's
//                         key order comes from query.hip's ray_query_keys / ray_query_rank), test
//                         the spheres and planes, then the models in upload order with the scan's
//                         bound seeded at t_max (scan.h flat_query in FlavOcclusion; LANE: the
//                         per-lane reference scan started at t_max); a lane retires at its first
//                         hit, the model loop ends when no lane of the wave is left (occlusion.h,
//                         shared with gather.hip).
// A file of its own: the render, path and ray-query kernels' code objects are what they were.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "launch.h"
#include "occlusion.h"
#include "scan.h"
#include "sort_key.h"

namespace atr {

// Waves/SIMD: the ray query's 7 (query.hip kQueryOcc). Without the u/v rows the LDS is 20 KB per
// workgroup, so 8 would fit a CU; built for 8 (64 VGPRs, 31 spilled dwords instead of 6) the query
// measured 3-14 % slower on the clustered scan and 7-45 % on LANE (one box).
#ifndef ATR_OCCL_OCC  // experiment builds
#define ATR_OCCL_OCC 7
#endif
constexpr int kOcclOcc = ATR_OCCL_OCC;

template <bool LANE, bool SORT>
__global__ __launch_bounds__(256, kOcclOcc) void ray_occlusion_kernel(OcclParams P) {
    const int lane = threadIdx.x & 63;
    const uint32_t n = uint32_t(__builtin_amdgcn_readfirstlane(int(P.n)));
    const DScene* S = uniform_global(P.scene);
    int err = 0;
    Ctr ct;
    uint32_t traced = 0;
    for (;;) {  // every wave leaves once the batch is claimed: the exit every wave reaches
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(P.head, 64u);
        base = uint32_t(__builtin_amdgcn_readfirstlane(int(__shfl(int(base), 0))));
        if (base >= n) break;
        const uint32_t i = base + uint32_t(lane);
        bool in = i < n;
        uint32_t e = i;
        if (SORT && in) {
            e = P.perm[i];
            // an index outside the batch, impossible for a complete order, is neither read nor written
            if (e >= n) {
                in = false;
                if (P.error_flag) atomicOr(P.error_flag, 2);
            }
        }
        V3 o = mk(0.f, 0.f, 0.f), d = mk(0.f, 0.f, 1.f);
        float T = kMaxFloat;
        bool ok = false;
        if (in) {
            V3 ro, rd;
            load_ray(P.o, P.d, e, ro, rd);
            float tm = kMaxFloat;
            if (P.tmax) tm = P.tmax[e];
            // t_max: positive or +inf, tested on its bits (NaN, zero and negative values fail, whatever
            // the denormal mode); +inf is clamped to kMaxFloat
            const int32_t tb = __float_as_int(tm);
            ok = ray_ok(ro, rd) && tb > 0 && tb <= 0x7F800000;
            if (ok) { o = ro; d = rd; T = fminf(tm, kMaxFloat); }  // else the placeholder: an inactive lane
        }
        // nothing can be accepted in (kTol, T) when T <= kTol: valid, visible, not walked
        bool active = ok && T > kTol;
        bool occ = active && occluded_analytic(S, o, d, T);
        active = active && !occ;
        if (occluded_models<LANE>(S, o, d, T, active, err, ct)) occ = true;
        if (in) {
            if (ok) traced += 1;
            P.out[e] = uint8_t(!ok ? ATR_OCCL_INVALID : occ ? ATR_OCCL_OCCLUDED : ATR_OCCL_VISIBLE);
        }
    }
    if (P.traced_rays) add_traced(P.traced_rays, traced, int(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (err && P.error_flag) atomicOr(P.error_flag, 1);
}

template __global__ void ray_occlusion_kernel<false, false>(OcclParams);
template __global__ void ray_occlusion_kernel<false, true>(OcclParams);
template __global__ void ray_occlusion_kernel<true, false>(OcclParams);
template __global__ void ray_occlusion_kernel<true, true>(OcclParams);

}  // namespace atr

// Persistent, sized like the ray query's launch: `ncu` x occupancy workgroups (4 waves each), at
// most one wave per 64 rays.
extern "C" hipError_t atr_launch_occlusion(const atr::OcclParams& P, int lane, int ncu, hipStream_t s) {
    const uint64_t need = (uint64_t(P.n) + 255u) / 256u;
    const dim3 g(unsigned(std::min<uint64_t>(uint64_t(ncu) * atr::kOcclOcc, need))), b(256);
    const bool sort = P.perm != nullptr;
    if (lane) {
        if (sort) hipLaunchKernelGGL((atr::ray_occlusion_kernel<true, true>), g, b, 0, s, P);
        else hipLaunchKernelGGL((atr::ray_occlusion_kernel<true, false>), g, b, 0, s, P);
    } else {
        if (sort) hipLaunchKernelGGL((atr::ray_occlusion_kernel<false, true>), g, b, 0, s, P);
        else hipLaunchKernelGGL((atr::ray_occlusion_kernel<false, false>), g, b, 0, s, P);
    }
    return hipGetLastError();
}
