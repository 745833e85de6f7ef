// paths.h -- what a kernel needs to feed the path engine's queues and result slots (paths.hip,
// DESIGN.md §4h): the finished path's record, the all-sky marker and the queue append. Shared by the
// path kernels and the radiance query's entry kernel (radiance.hip).
#pragma once
#include "sort_key.h"

namespace atr {

// A finished path: its colour (cast_ray's ret) and the reference's ray_casts (renderer.cpp:260),
// at its result slot o (cell x 64 spp + sample x 64 + pixel lane: the resolve's lanes read a
// sample's 64 results as one coalesced 1-KB row).
__device__ __forceinline__ void path_finish(float4_t* out, uint32_t o, V3 ret, uint32_t casts) {
    out[o] = float4_t{ret.x, ret.y, ret.z, __uint_as_float(casts)};
}

// Without AA every sample of a pixel casts the same camera ray (renderer.cpp:348-357), so when it
// meets the sky every sample's path ends there with the same colour and no ray_casts. Then only
// sample 0 writes its result slot, with this marker in place of the count (a real count is at most
// the bounce limit), and the resolve takes that colour for every sample: c4 skips ~86% of the
// camera kernel's result writes and of the resolve's reads; the sum is the same f32 adds.
constexpr uint32_t kAllSky = 0xFFFFFFFFu;

// Append this lane's path (if `go`) to queue q (planes `cap` entries apart): one atomic per wave for
// the wave's survivors, each at base + its rank among them. With the queue sort on, the entry also
// records its key and its rank in the key's bin (PathSort).
template <bool SORT>
__device__ __forceinline__ void path_enqueue(float4_t* q, int64_t cap, PathCtl* ctl, bool go, V3 o, V3 d,
                                             uint32_t pix, uint32_t g, V3 ret, V3 w, uint64_t st, PathSort so) {
    const uint64_t m = __ballot(go);
    if (m == 0) return;
    const int lane = threadIdx.x & 63;
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(&ctl->tail, uint32_t(__popcll(m)));
    base = uint32_t(__builtin_amdgcn_readfirstlane(int(__shfl(int(base), 0))));
    if (!go) return;
    const int64_t e = int64_t(base) + __popcll(m & ((uint64_t(1) << lane) - 1));
    // sorted queues hold each entry's four records together (64 B, entry-major: q[4 e + i]) so the
    // sort moves whole 64-B blocks; unsorted queues keep the four planes (q[i cap + e])
    const int64_t e0 = SORT ? 4 * e : e, es = SORT ? 1 : cap;
    if constexpr (SORT) {
        const uint32_t key = path_sort_key(o, d, so);
        so.kr[e] = uint2_t{key, atomicAdd(so.hist + key, 1u)};
    }
    q[e0] = float4_t{o.x, o.y, o.z, d.x};
    q[es + e0] = float4_t{d.y, d.z, __uint_as_float(pix), __uint_as_float(g)};
    q[2 * es + e0] = float4_t{ret.x, ret.y, ret.z, w.x};
    q[3 * es + e0] = float4_t{w.y, w.z, __uint_as_float(uint32_t(st)), __uint_as_float(uint32_t(st >> 32))};
}

}  // namespace atr
