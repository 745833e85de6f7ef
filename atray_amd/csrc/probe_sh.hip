// probe_sh.hip -- light probes as L2 spherical harmonics on the device (atr_probe_sh):
// for a batch of points in free space, every sample is the renderer's own path from the point along a
// direction drawn uniformly over the whole sphere on the (probe, sample) stream (engine.h
// probe_dir_state: rejection inside a radial shell, no transcendentals), continued on that stream; per
// probe the samples' colours are projected on the nine real SH of bands 0..2, 27 ordered f32 sums.
//   probe_sh_entry_kernel    gather_radiance_entry_kernel (gather_radiance.hip) without a normal: the
//                            persistent claim of 64 items, one lane per item, the same slot layout
//                            (item = probe x nsamples + sample), the first segment traced in FLAT's
//                            bounce flavour, the path finished in its slot or appended to queue 0.
//                            Every sample of a valid probe is traced; an item of an invalid probe
//                            writes the invalid marker;
//   (the bounce levels)      path_bounce_kernel and the queue sort, as they are, on a PathParams;
//   probe_sh_resolve_kernel  one wave per probe: rows of 64 consecutive samples' slots (1 KB,
//                            coalesced); the lane that loaded a slot draws its direction again (the
//                            same function, so the same bits), evaluates the nine basis values and
//                            puts {colour, Y0..Y8} into the wave's LDS; lanes 0..26 each own one
//                            (coefficient, channel) and walk the row in sample order, the 27 sums side
//                            by side. Every output has one owner: no atomics.
// A file of its own: the other kernels' code objects are what they were.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "launch.h"
#include "paths.h"
#include "scan.h"

namespace atr {

// Waves/SIMD: the radiance gather's 7 (gather_radiance.hip), whose scan and LDS the entry kernel has.
#ifndef ATR_PROBE_SH_OCC  // experiment builds
#define ATR_PROBE_SH_OCC 7
#endif
constexpr int kProbeShOcc = ATR_PROBE_SH_OCC;

template <bool SORT>
__global__ __launch_bounds__(256, kProbeShOcc) void probe_sh_entry_kernel(ProbeShParams P) {
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
        // (probe, sample) of the item; a lane past the batch's end reads the wave's first point (in
        // bounds) and writes nothing
        const uint32_t c = in ? idx : base;
        const uint32_t i = c / ns, s = c - i * ns;
        const size_t e = size_t(P.point0) + i;  // the probe's index in the call's arrays
        const V3 p = mk(P.p[3 * e], P.p[3 * e + 1], P.p[3 * e + 2]);
        const bool ok = in && ray_ok(p, mk(0.f, 0.f, 1.f));  // a finite point: every sample of it is traced
        // the placeholder of an inactive lane
        V3 o = mk(0.f, 0.f, 0.f), d = mk(0.f, 0.f, 1.f);
        uint64_t st = 0, stream = 1;
        if (ok) {  // per lane, at most kProbeTries trips, nothing in it crosses lanes
            uint32_t tries;
            d = probe_dir_state(P.seed, P.point_base + int64_t(e), P.first_sample + s, st, stream, tries);
            o = p;
        }
        // the generated direction (zeros for an invalid probe): stored before the scan
        if (in && P.dirs) {
            float* q = P.dirs + 3 * (size_t(P.point0) * ns + idx);
            q[0] = ok ? d.x : 0.f;
            q[1] = ok ? d.y : 0.f;
            q[2] = ok ? d.z : 0.f;
        }
        const SceneHit sh = intersect_models<SCHED_FLAT, FlavBounce, false>(S, o, d, ok, err, ct, P.hyb_a, P.hyb_b);
        // the point is read again after the query instead of being held through it (as
        // gather_radiance.hip does): the memory clobber keeps the loads here, the opaque copy of the
        // index keeps their addresses from being formed before the query
        uint32_t ia = i;
        __asm__ volatile("" : "+v"(ia) :: "memory");
        const uint32_t pix = uint32_t(uint64_t(P.point_base) + P.point0 + ia);  // the stream index, 32 bits
        bool go = false;
        V3 ret = mk(0.f, 0.f, 0.f), w = mk(1.f, 1.f, 1.f);
        if (ok) {
            traced += 1;
            const size_t ea = size_t(P.point0) + ia;
            o = mk(P.p[3 * ea], P.p[3 * ea + 1], P.p[3 * ea + 2]);
            stream = (uint64_t(P.point_base + int64_t(ea)) << 1) | 1ULL;
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
            path_finish(P.out, idx, mk(0.f, 0.f, 0.f), kRayInvalid);
        }
        path_enqueue<SORT>(P.q0, P.cap, &P.ctl[0], go, o, d, pix, idx, ret, w, st, P.sort);
    }
    if (P.traced_rays) add_traced(P.traced_rays, traced, int(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (err && P.error_flag) atomicOr(P.error_flag, 1);
}

template __global__ void probe_sh_entry_kernel<false>(ProbeShParams);
template __global__ void probe_sh_entry_kernel<true>(ProbeShParams);

// The wave's own LDS traffic in program order for the compiler too: a row's writes by many lanes before
// the summing lanes' reads, and those before the next row's writes (the hardware runs a wave's LDS
// operations in order).
__device__ __forceinline__ void wave_lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// A sample's record in the wave's LDS: colour (3), Y0..Y8 (9), one word of padding. The odd stride
// puts the 64 lanes' writes of one word on distinct banks (12 would fold them four to a bank); a
// sample's twelve words are consecutive, so the 27 summing lanes' reads of them are twelve distinct
// banks, each address a broadcast.
constexpr uint32_t kProbeRec = 13;

// One wave per probe of the batch. sum[3 k + c] = sum[3 k + c] + (colour.c * Yk(d)) for the samples in
// sample order, from zero or from the caller's running sums. A row of 64 slots is loaded by the lanes
// (1 KB, coalesced); lane l draws the direction of sample row + l again on the sample's stream,
// evaluates the basis and writes its record; lanes 0..26 then each add the row's products of their
// own (k, c) one after the other -- two LDS reads, one multiply and one add per sample, eight samples'
// reads in flight at a time -- while the next row's loads are on their way. Every slot of a valid probe
// holds a traced sample, so nothing is packed. ray_casts is an integer sum and needs no order.
__global__ __launch_bounds__(256) void probe_sh_resolve_kernel(ProbeShParams P) {
    __shared__ float recs[4][64 * kProbeRec];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t i = uint32_t(__builtin_amdgcn_readfirstlane(int(blockIdx.x * 4u + (threadIdx.x >> 6))));
    if (i >= P.npoints) return;  // whole wavefront
    const uint32_t ns = uint32_t(__builtin_amdgcn_readfirstlane(int(P.nsamples))), first = P.first_sample;
    const float4_t* src = P.out + size_t(i) * ns;
    const size_t r = size_t(P.point0) + i;
    float* srgb = P.sample_rgb ? P.sample_rgb + 3 * (r * ns) : nullptr;
    const bool mine = lane < 27u;  // the owner of sum 3 k + c = lane
    if (__float_as_uint(src[0].w) == kRayInvalid) {  // not traced: zeros from a first call, else what was there
        for (uint32_t s = lane; srgb && s < ns; s += 64u) {
            srgb[3 * size_t(s)] = 0.f;
            srgb[3 * size_t(s) + 1] = 0.f;
            srgb[3 * size_t(s) + 2] = 0.f;
        }
        if (first == 0) {
            if (mine && P.sh) P.sh[27 * r + lane] = 0.f;
            if (mine && P.sum) P.sum[27 * r + lane] = 0.f;
            if (lane == 0 && P.ray_casts) P.ray_casts[r] = 0u;
        }
        if (lane == 0 && P.invalid) P.invalid[r] = 1;
        return;
    }
    float* buf = recs[threadIdx.x >> 6];
    const uint32_t kc = mine ? lane / 3u + 3u : 3u, cc = mine ? lane % 3u : 0u;  // the record's words this lane reads
    float acc = 0.f;      // lanes 0..26
    uint32_t casts = 0;   // a partial sum per lane
    if (first > 0) {  // the host requires sum then
        if (mine) acc = P.sum[27 * r + lane];
        if (P.ray_casts && lane == 0) casts = P.ray_casts[r];
    }
    const int64_t pixel = P.point_base + int64_t(r);
    float4_t v = float4_t{0.f, 0.f, 0.f, 0.f};
    if (lane < ns) v = src[lane];
    for (uint32_t row = 0; row < ns; row += 64u) {  // wave-uniform
        const uint32_t s = row + lane;
        const uint32_t k = std::min(64u, ns - row);  // the row's samples
        if (s < ns) {
            if (srgb) {
                srgb[3 * size_t(s)] = v.x;
                srgb[3 * size_t(s) + 1] = v.y;
                srgb[3 * size_t(s) + 2] = v.z;
            }
            uint64_t st, stream;
            uint32_t tries;
            const V3 d = probe_dir_state(P.seed, pixel, first + s, st, stream, tries);
            float y[9];
            sh_basis(d, y);
            float* q = buf + lane * kProbeRec;
            q[0] = v.x;
            q[1] = v.y;
            q[2] = v.z;
#pragma unroll
            for (int u = 0; u < 9; ++u) q[3 + u] = y[u];
            casts += __float_as_uint(v.w);
        }
        float4_t vn = float4_t{0.f, 0.f, 0.f, 0.f};  // the next row's slots
        if (s + 64u < ns) vn = src[s + 64u];
        wave_lds_order();
        if (mine) {
            const float* a = buf + cc;
            const float* b = buf + kc;
            uint32_t j = 0;
            for (; j + 8u <= k; j += 8u) {  // whole eights: no test between the adds
                float ca[8], ya[8];
#pragma unroll
                for (uint32_t u = 0; u < 8u; ++u) {
                    ca[u] = a[(j + u) * kProbeRec];
                    ya[u] = b[(j + u) * kProbeRec];
                }
#pragma unroll
                for (uint32_t u = 0; u < 8u; ++u) acc = acc + (ca[u] * ya[u]);
            }
            for (; j < k; ++j) acc = acc + (a[j * kProbeRec] * b[j * kProbeRec]);  // the last one to seven
        }
        wave_lds_order();
        v = vn;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) casts += __shfl_xor(casts, off);
    if (mine) {
        if (P.sum) P.sum[27 * r + lane] = acc;
        if (P.sh) P.sh[27 * r + lane] = (acc * 12.566370614f) / float(first + ns);
    }
    if (lane != 0) return;
    if (P.ray_casts) P.ray_casts[r] = casts;
    if (P.invalid) P.invalid[r] = 0;
}

}  // namespace atr

// Persistent, sized like the radiance gather's launch: `ncu` x occupancy workgroups (4 waves each), at
// most one wave per 64 items.
extern "C" hipError_t atr_launch_probe_sh_entry(const atr::ProbeShParams& P, int ncu, hipStream_t s) {
    const uint64_t need = (uint64_t(P.n) + 255u) / 256u;
    const dim3 g(unsigned(std::min<uint64_t>(uint64_t(ncu) * atr::kProbeShOcc, need))), b(256);
    if (P.sort.bits > 0) hipLaunchKernelGGL(atr::probe_sh_entry_kernel<true>, g, b, 0, s, P);
    else hipLaunchKernelGGL(atr::probe_sh_entry_kernel<false>, g, b, 0, s, P);
    return hipGetLastError();
}

extern "C" hipError_t atr_launch_probe_sh_resolve(const atr::ProbeShParams& P, hipStream_t s) {
    if (P.npoints == 0) return hipSuccess;
    hipLaunchKernelGGL(atr::probe_sh_resolve_kernel, dim3((P.npoints + 3u) / 4u), dim3(256), 0, s, P);
    return hipGetLastError();
}
