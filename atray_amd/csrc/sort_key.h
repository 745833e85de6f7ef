// sort_key.h -- the (direction cell, origin cell) key of a ray (PathSort, engine.h), shared by the
// path engine's queue sort (paths.hip) and the ray queries' batch order (query.hip); load_ray, how
// the ray and occlusion queries (query.hip, occlusion.hip) read a ray of the caller's batch.
#pragma once
#include "engine.h"

#ifndef ATR_SORT_ILEAVE  // fine direction bits per side below the origin cell (0: direction, then origin)
#define ATR_SORT_ILEAVE 2
#endif

namespace atr {

__device__ __forceinline__ void load_ray(const float* __restrict__ po, const float* __restrict__ pd, uint32_t e, V3& o,
                                         V3& d) {
    const size_t b = 3 * size_t(e);
    o = mk(po[b], po[b + 1], po[b + 2]);
    d = mk(pd[b], pd[b + 1], pd[b + 2]);
}

// Sort key of a queued ray (PathSort, engine.h): the octahedral cell of its direction (kSortDirs x
// kSortDirs over the unfolded octahedron) and the Morton code of its origin's cell, b bits per axis
// over the scene box, interleaved as below.
__device__ __forceinline__ uint32_t spread3(uint32_t x) {  // bits 0..9 -> every third bit
    x = (x | (x << 16)) & 0x030000FFu;
    x = (x | (x << 8)) & 0x0300F00Fu;
    x = (x | (x << 4)) & 0x030C30C3u;
    return (x | (x << 2)) & 0x09249249u;
}
__device__ __forceinline__ uint32_t path_sort_key(V3 o, V3 d, PathSort so) {
    const float qmax = float((1 << so.bits) - 1);
    // fmaxf first: a NaN coordinate lands in cell 0; an origin outside the box clamps to the edge cell
    const uint32_t qx = uint32_t(fminf(fmaxf((o.x - so.lo[0]) * so.sc[0], 0.0f), qmax));
    const uint32_t qy = uint32_t(fminf(fmaxf((o.y - so.lo[1]) * so.sc[1], 0.0f), qmax));
    const uint32_t qz = uint32_t(fminf(fmaxf((o.z - so.lo[2]) * so.sc[2], 0.0f), qmax));
    const uint32_t morton = (spread3(qx) << 2) | (spread3(qy) << 1) | spread3(qz);
    // octahedral direction: (x, y) / (|x| + |y| + |z|), the lower hemisphere folded out
    const float sum = fabsf(d.x) + fabsf(d.y) + fabsf(d.z);
    float u = d.x / sum, v = d.y / sum;
    if (d.z < 0.0f) {
        const float uu = (1.0f - fabsf(v)) * (u >= 0.0f ? 1.0f : -1.0f);
        v = (1.0f - fabsf(u)) * (v >= 0.0f ? 1.0f : -1.0f);
        u = uu;
    }
    constexpr float D = float(kSortDirs);
    const uint32_t iu = uint32_t(fminf(fmaxf((u * 0.5f + 0.5f) * D, 0.0f), D - 1.0f));
    const uint32_t iv = uint32_t(fminf(fmaxf((v * 0.5f + 0.5f) * D, 0.0f), D - 1.0f));
    // coarse direction cell (the low F bits of iu, iv dropped), origin cell, then the fine bits:
    // a run of the order is one coarse direction and one region, fine directions side by side
    // (F = 2 of the 16 x 16 map: c4 +1.2%, c5 +1.5% over direction cell, then origin)
    constexpr int F = ATR_SORT_ILEAVE;
    const uint32_t coarse = (iv >> F) * uint32_t(kSortDirs >> F) + (iu >> F);
    const uint32_t fine = ((iv & ((1u << F) - 1u)) << F) | (iu & ((1u << F) - 1u));
    return (((coarse << (3 * so.bits)) | morton) << (2 * F)) | fine;
}

}  // namespace atr
