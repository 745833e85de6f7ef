// query.hip -- ray queries (atr_trace_rays): get_intersection_data for a batch of
// the caller's rays instead of the camera's or a path queue's.
//   ray_query_keys    with an order: every ray's sort key (sort_key.h, the path engine's) and its
//                     arrival rank in the key's bin; a ray that fails the validity test goes to bin 0;
//   (the bin scan)    paths.hip's three kernels turn the bins into bin starts (atr_launch_sort_bins);
//   ray_query_rank    perm[start[key] + rank] = ray: the batch in key order;
//   ray_query_kernel  persistent waves claim 64 positions of the batch at a time, test and trace
//                     their rays (FLAT's dealt rounds in the bounce flavour, or the per-lane reference
//                     scan), finish the hit record (shade.h) and write the outputs that were asked
//                     for at each ray's input index.
// A file of its own: the render and path kernels' code objects are what they were without it.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "launch.h"
#include "scan.h"
#include "sort_key.h"

namespace atr {

// Key and arrival rank per ray (grid-stride, a wavefront takes 64 consecutive rays). kr and hist as
// in the path engine's queue sort, but the lanes of a wave that share a key arrive together: the
// first of them adds their number to the bin and each takes base + its place among them. A caller's
// batch can put most of its rays into a few bins -- camera rays have one origin cell and a handful
// of direction cells -- and one atomic per ray then queues up on those few addresses: 7.2 ms for 2 M
// primary rays in pixel order against 0.09 ms for rays spread over the bins. The
// grouping is ballots only, one iteration per distinct key of the wave; the atomics go out together.
__global__ __launch_bounds__(256) void ray_query_keys(QueryParams P) {
    const PathSort so = P.sort;
    const int lane = threadIdx.x & 63;
    const uint32_t n = uint32_t(__builtin_amdgcn_readfirstlane(int(P.n)));
    const uint32_t stride = gridDim.x * 256u;
    for (uint32_t e0 = blockIdx.x * 256u + (threadIdx.x & ~63u); e0 < n; e0 += stride) {  // wave-uniform
        const uint32_t e = e0 + uint32_t(lane);
        const bool has = e < n;
        uint32_t key = 0u;
        if (has) {
            V3 o, d;
            load_ray(P.o, P.d, e, o, d);
            // path_sort_key clamps an origin outside the scene box to the edge cell (fmaxf, then fminf)
            if (ray_ok(o, d)) key = path_sort_key(o, d, so);
        }
        uint64_t pending = __ballot(has);
        int leader = lane;
        uint32_t place = 0u, count = 1u;
        while (pending) {  // wave-uniform: the lanes of the first pending lane's key
            const int l = __builtin_ctzll(pending);
            const uint32_t k = uint32_t(__builtin_amdgcn_readlane(int(key), l));
            const bool same = has && key == k;
            const uint64_t m = __ballot(same);
            if (same) {
                leader = l;
                place = uint32_t(__popcll(m & ((uint64_t(1) << lane) - 1)));
                count = uint32_t(__popcll(m));
            }
            pending &= ~m;
        }
        uint32_t base = 0u;
        if (has && lane == leader) base = atomicAdd(so.hist + key, count);
        base = uint32_t(__shfl(int(base), leader));
        if (has) so.kr[e] = uint2_t{key, base + place};
    }
}

// The batch's key order. A slot outside the batch, impossible for consistent keys and ranks, is
// flagged (bit 1 of the error word, as path_sort_rank does).
__global__ __launch_bounds__(256) void ray_query_rank(QueryParams P) {
    const PathSort so = P.sort;
    const uint32_t stride = gridDim.x * 256u;
    for (uint32_t e = blockIdx.x * 256u + threadIdx.x; e < P.n; e += stride) {
        const uint2_t kr = so.kr[e];
        const uint32_t dst = so.start[kr.x] + kr.y;
        if (dst < P.n) so.perm[dst] = e;
        else if (P.error_flag) atomicOr(P.error_flag, 2);
    }
}

// Waves/SIMD: the bounce kernel's measured default (paths.hip kBounceOcc; the same scan, the same
// LDS leaf buffer).
constexpr int kQueryOcc = 7;

template <bool LANE, bool SORT>
__global__ __launch_bounds__(256, kQueryOcc) void ray_query_kernel(QueryParams P) {
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
            e = P.sort.perm[i];
            // an index outside the batch, impossible for a complete order, is neither read nor written
            if (e >= n) {
                in = false;
                if (P.error_flag) atomicOr(P.error_flag, 2);
            }
        }
        V3 o = mk(0.f, 0.f, 0.f), d = mk(0.f, 0.f, 1.f);
        bool ok = false;
        if (in) {
            V3 ro, rd;
            load_ray(P.o, P.d, e, ro, rd);
            ok = ray_ok(ro, rd);
            if (ok) { o = ro; d = rd; }  // a ray that fails keeps the placeholder: an inactive lane
        }
        SceneHit sh;
        if constexpr (LANE) sh = intersect_models<SCHED_LANE, FlavBounce, false>(S, o, d, ok, err, ct, P.hyb_a, P.hyb_b);
        else sh = intersect_models<SCHED_FLAT, FlavBounce, false>(S, o, d, ok, err, ct, P.hyb_a, P.hyb_b);
        // the ray is read again after the query instead of being held through it (as the bounce
        // kernel does): the memory clobber keeps the loads here, the opaque copy of the index keeps
        // their addresses from being formed before the query
        uint32_t ea = e;
        __asm__ volatile("" : "+v"(ea) :: "memory");
        if (in) {
            float t = kMaxFloat, fu = 0.f, fv = 0.f;
            uint32_t face = 0xFFFFFFFFu;
            int32_t model = -1, kind = ATR_RAY_INVALID, material = 0;
            V3 nrm = mk(0.f, 0.f, 0.f);
            if (ok) {
                traced += 1;
                load_ray(P.o, P.d, ea, o, d);
                Isect id;
                scene_finish(S, o, d, sh.best, sh.face, sh.fu, sh.fv, sh.nm, id);  // renderer.cpp:86-160
                t = id.t;
                face = id.face;
                fu = sh.fu;
                fv = sh.fv;
                material = id.material;
                if (id.type == T_SKY) {
                    kind = ATR_RAY_SKY;
                } else {
                    kind = id.type == T_TRI ? ATR_RAY_TRI : id.type == T_SPHERE ? ATR_RAY_SPHERE : ATR_RAY_PLANE;
                    nrm = id.normal;
                    if (id.type == T_TRI) model = sh.nm;
                }
            }
            const size_t r = size_t(ea);
            if (P.t) P.t[r] = t;
            if (P.face) P.face[r] = face;
            if (P.model) P.model[r] = model;
            if (P.uv) { P.uv[2 * r] = fu; P.uv[2 * r + 1] = fv; }
            if (P.kind) P.kind[r] = kind;
            if (P.material) P.material[r] = material;
            if (P.normal) { P.normal[3 * r] = nrm.x; P.normal[3 * r + 1] = nrm.y; P.normal[3 * r + 2] = nrm.z; }
        }
    }
    if (P.traced_rays) add_traced(P.traced_rays, traced, int(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (err && P.error_flag) atomicOr(P.error_flag, 1);
}

template __global__ void ray_query_kernel<false, false>(QueryParams);
template __global__ void ray_query_kernel<false, true>(QueryParams);
template __global__ void ray_query_kernel<true, false>(QueryParams);
template __global__ void ray_query_kernel<true, true>(QueryParams);

}  // namespace atr

// The batch's key order into P.sort.perm (the bins zero before and after).
extern "C" hipError_t atr_launch_query_sort(const atr::QueryParams& P, int ncu, hipStream_t s) {
    const unsigned grid = unsigned(std::min<uint64_t>(uint64_t(ncu) * 16u, (uint64_t(P.n) + 255u) / 256u));
    hipLaunchKernelGGL(atr::ray_query_keys, dim3(grid), dim3(256), 0, s, P);
    const hipError_t e = atr_launch_sort_bins(P.sort, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(atr::ray_query_rank, dim3(grid), dim3(256), 0, s, P);
    return hipGetLastError();
}

// Persistent, sized like the bounce launch: `ncu` x occupancy workgroups (4 waves each), at most
// one wave per 64 rays.
extern "C" hipError_t atr_launch_query(const atr::QueryParams& P, int lane, int ncu, hipStream_t s) {
    const uint64_t need = (uint64_t(P.n) + 255u) / 256u;
    const dim3 g(unsigned(std::min<uint64_t>(uint64_t(ncu) * atr::kQueryOcc, need))), b(256);
    const bool sort = P.sort.bits > 0;
    if (lane) {
        if (sort) hipLaunchKernelGGL((atr::ray_query_kernel<true, true>), g, b, 0, s, P);
        else hipLaunchKernelGGL((atr::ray_query_kernel<true, false>), g, b, 0, s, P);
    } else {
        if (sort) hipLaunchKernelGGL((atr::ray_query_kernel<false, true>), g, b, 0, s, P);
        else hipLaunchKernelGGL((atr::ray_query_kernel<false, false>), g, b, 0, s, P);
    }
    return hipGetLastError();
}
