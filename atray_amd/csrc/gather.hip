// gather.hip -- hemisphere visibility gathered on the device (atr_gather_occlusion):
// for a batch of surface points with unit normals, nsamples directions per point are drawn in
// registers (engine.h gather_dir: bounce_shade's diffuse direction on the (point, sample) PCG
// streams) and each one above the tangent plane is answered as atr_occluded_rays answers it
// (occlusion.h); per point the counts of visible and occluded samples and a bit per sample come out.
//   gather_occlusion_kernel  persistent waves claim 64 items of the flattened (point, sample) index at
//                            a time; a point's lanes are contiguous in the wave, so the first of them
//                            adds the popcounts of the wave's two ballots, masked to the point's
//                            lanes, to the point's counters, and the first lane of every mask word
//                            ORs its slice of the visible ballot in. The scan runs in FlavOcclusion
//                            for every nsamples: a one-origin flavour for whole waves of one point
//                            measured slower.
// A file of its own: the other kernels' code objects are what they were.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "launch.h"
#include "occlusion.h"
#include "scan.h"

namespace atr {

// Waves/SIMD: the occlusion query's 7 (occlusion.hip kOcclOcc), whose scan and LDS this kernel has.
#ifndef ATR_GATHER_OCC  // experiment builds
#define ATR_GATHER_OCC 7
#endif
constexpr int kGatherOcc = ATR_GATHER_OCC;

template <bool LANE>
__global__ __launch_bounds__(256, kGatherOcc) void gather_occlusion_kernel(GatherParams P) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t n = uint32_t(__builtin_amdgcn_readfirstlane(int(P.n)));
    const uint32_t ns = uint32_t(__builtin_amdgcn_readfirstlane(int(P.nsamples)));
    const DScene* S = uniform_global(P.scene);
    int err = 0;
    Ctr ct;
    uint32_t traced = 0;
    for (;;) {  // every wave leaves once the batch is claimed: the exit every wave reaches
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(P.head, 64u);
        base = uint32_t(__builtin_amdgcn_readfirstlane(int(__shfl(int(base), 0))));
        if (base >= n) break;
        const uint32_t idx = base + lane;
        const bool in = idx < n;
        // (point, sample) of the item; a lane past the batch's end reads the wave's first point (in
        // bounds) and writes nothing
        const uint32_t c = in ? idx : base;
        const uint32_t i = c / ns, s = c - i * ns;
        const V3 p = mk(P.p[3 * size_t(i)], P.p[3 * size_t(i) + 1], P.p[3 * size_t(i) + 2]);
        const V3 nn = mk(P.nrm[3 * size_t(i)], P.nrm[3 * size_t(i) + 1], P.nrm[3 * size_t(i) + 2]);
        float tm = kMaxFloat;
        if (P.tmax) tm = P.tmax[i];
        const bool pok = in && gather_point_ok(p, nn, tm);
        // the placeholder of an inactive lane
        V3 o = mk(0.f, 0.f, 0.f), d = mk(0.f, 0.f, 1.f), g = mk(0.f, 0.f, 0.f);
        float T = kMaxFloat;
        bool ok = false;  // traced: a valid point, a direction that passes the ray test, above the plane
        if (pok) {
            g = gather_dir(P.seed, P.point_base + int64_t(i), P.first_sample + s, nn);
            ok = ray_ok(p, g) && dot(g, nn) > 0.0f;
            if (ok) { o = p; d = g; T = fminf(tm, kMaxFloat); }
        }
        // every generated direction of a valid point, traced or not (zeros for an invalid point): stored
        // before the scan, which then need not hold it
        if (in && P.dirs) {
            float* q = P.dirs + 3 * size_t(idx);
            q[0] = g.x;
            q[1] = g.y;
            q[2] = g.z;
        }
        // nothing can be accepted in (kTol, T) when T <= kTol: valid, visible, not walked
        bool active = ok && T > kTol;
        bool occ = active && occluded_analytic(S, o, d, T);
        active = active && !occ;
        if (occluded_models<LANE>(S, o, d, T, active, err, ct)) occ = true;
        const unsigned long long bv = __ballot(ok && !occ), bo = __ballot(ok && occ);
        if (in) {
            if (ok) traced += 1;
            // the point's lanes in this wave: first .. last
            const uint32_t first = s > lane ? 0u : lane - s;
            const uint32_t end = lane + (ns - 1u - s), last = end < 63u ? end : 63u;
            if (lane == first) {
                const uint32_t cnt = last - first + 1u;
                const unsigned long long pm = (cnt == 64u ? ~0ull : (1ull << cnt) - 1ull) << first;
                const uint32_t cv = uint32_t(__popcll(bv & pm)), co = uint32_t(__popcll(bo & pm));
                if (P.visible && cv) atomicAdd(P.visible + i, cv);
                if (P.occluded && co) atomicAdd(P.occluded + i, co);
            }
            if (P.mask && (lane == first || (s & 31u) == 0u)) {  // the first lane of a mask word's samples
                const uint32_t room = 32u - (s & 31u), left = last - lane + 1u, cnt = room < left ? room : left;
                const uint32_t bits = uint32_t(bv >> lane) & (cnt == 32u ? ~0u : (1u << cnt) - 1u);
                if (bits) atomicOr(P.mask + size_t(i) * P.words + (s >> 5), bits << (s & 31u));
            }
        }
    }
    if (P.traced_rays) add_traced(P.traced_rays, traced, int(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (err && P.error_flag) atomicOr(P.error_flag, 1);
}

template __global__ void gather_occlusion_kernel<false>(GatherParams);
template __global__ void gather_occlusion_kernel<true>(GatherParams);

}  // namespace atr

// Persistent, sized like the occlusion query's launch: `ncu` x occupancy workgroups (4 waves each),
// at most one wave per 64 items.
extern "C" hipError_t atr_launch_gather(const atr::GatherParams& P, int lane, int ncu, hipStream_t s) {
    const uint64_t need = (uint64_t(P.n) + 255u) / 256u;
    const dim3 g(unsigned(std::min<uint64_t>(uint64_t(ncu) * atr::kGatherOcc, need))), b(256);
    if (lane) hipLaunchKernelGGL((atr::gather_occlusion_kernel<true>), g, b, 0, s, P);
    else hipLaunchKernelGGL((atr::gather_occlusion_kernel<false>), g, b, 0, s, P);
    return hipGetLastError();
}
