// occlusion.h -- the wave-wide "any hit with kTol < t < T" tests shared by the occlusion query
// (occlusion.hip) and the hemisphere gather (gather.hip): the spheres
// and planes, then the models in upload order with the scan's bound seeded at T.
#pragma once
#include <hip/hip_runtime.h>

#include "scan.h"

namespace atr {

// Any sphere or plane with kTol < t < T (every lane of the wave; the counts are wave-uniform).
__device__ __forceinline__ bool occluded_analytic(const DScene* __restrict__ S, V3 o, V3 d, float T) {
    const int32_t nspheres = __builtin_amdgcn_readfirstlane(S->nspheres), nplanes = __builtin_amdgcn_readfirstlane(S->nplanes);
    bool occ = false;
    for (int32_t i = 0; i < nspheres; ++i) {
        const float t = sphere_t(o, d, uniform_global(S->spheres)[i]);
        occ = occ || (t > kTol && t < T);
    }
    for (int32_t i = 0; i < nplanes; ++i) {
        const float t = plane_t(o, d, uniform_global(S->planes)[i]);
        occ = occ || (t > kTol && t < T);
    }
    return occ;
}

// Any triangle of any model with kTol < t < T, for every lane of the wave (converged call; inactive
// lanes take part in the wave-wide scans). Models in upload order; the lanes a model occludes are
// inactive for the models after it, and the loop ends once no lane is left. Tree models: the
// reference's walk (root box, root leaf or the DFS's leaves in ascending distance) with its closest
// started at T, which ends at the first leaf that improves on it. LANE: the per-lane reference scan;
// otherwise the clustered scan's query loop (scan.h flat_query) in FlavOcclusion -- the bounce flavour
// without barycentrics (near-first passes into the LDS leaf buffer, every step dealt, no u/v rows in
// LDS), the key seeded with T -- and "the key moved" in place of the closest hit's read-out.
template <bool LANE>
__device__ __forceinline__ bool occluded_models(const DScene* __restrict__ S, V3 o, V3 d, float T, bool active, int& err,
                                                Ctr& ct) {
    const Ray r = make_ray(o, d);
    bool occ = false;
    const int32_t nmodels = __builtin_amdgcn_readfirstlane(S->nmodels);
    for (int32_t i = 0; i < nmodels; ++i) {
        if (__ballot(active) == 0) break;  // wave-uniform
        const DModel m = uniform_model(S->models[i]);
        bool hit = false;
        if (m.has_tree) {
            if constexpr (LANE) {
                if (active) {
                    Hit h;
                    tree_closest_lane<false>(r, m, h, err, ct, T);
                    hit = h.t < T;
                }
            } else {
                const int w = threadIdx.x >> 6, ln = threadIdx.x & 63;
                const unsigned long long start = static_cast<unsigned long long>(__float_as_uint(T)) << 32;
                flat_query<FlavOcclusion, false>(r, m, active, w, ln, err, ct, 0, 0, nullptr, 0, start);
                hit = active && flat_lds<kLeafBuf, FlavOcclusion::UV>().key[w][ln] != start;
            }
        } else if (active) {  // brute force: the surrounding box, then the faces up to the first hit
            if (box_entry(r, m.aabb[0], m.aabb[1], m.aabb[2], m.aabb[3], m.aabb[4], m.aabb[5]) != 0) {
                for (uint32_t j = 0; j < m.nfaces && !hit; ++j) {
                    const DTri* t = m.tris + j;
                    float u = 0.f, v = 0.f;
                    const float tt = tri_hit(r, mk(t->ax, t->ay, t->az), mk(t->abx, t->aby, t->abz),
                                             mk(t->acx, t->acy, t->acz), u, v);
                    hit = tt > kTol && tt < T;
                }
            }
        }
        if (hit) {
            occ = true;
            active = false;
        }
    }
    return occ;
}

}  // namespace atr
