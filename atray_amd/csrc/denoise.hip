// denoise.hip -- atr_denoise: the edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) with rational
// stopping weights; DESIGN.md §4s. A pack kernel reads the caller's buffers once (so out == color is
// safe), decides which pixels are inert and writes 16-byte records; every pass is then one lane per
// pixel, the lanes of a wave along x, so that a tap at x + dx*s is a contiguous run of records across
// the wave at every spacing. Every f32 operation is separately rounded (-ffp-contract=off) and the
// divisions are IEEE, so tests/c/denoise_ref.c equals the result bit for bit.
#include <hip/hip_runtime.h>

#include "denoise.h"
#include "launch.h"

namespace atr {

namespace {

__device__ __forceinline__ bool finite3(float x, float y, float z) {
    // |v| < inf is false for an infinity and for a NaN
    return __builtin_fabsf(x) < __builtin_inff() && __builtin_fabsf(y) < __builtin_inff() &&
           __builtin_fabsf(z) < __builtin_inff();
}

}  // namespace

// One lane per pixel: inertness, decided once from the caller's inputs, and the records.
__global__ __launch_bounds__(256) void denoise_pack_kernel(DenoisePack P) {
    const int64_t t = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (t >= P.npixels) return;
    float4_t c;
    c.x = P.color[3 * t], c.y = P.color[3 * t + 1], c.z = P.color[3 * t + 2];
    bool inert = !finite3(c.x, c.y, c.z);
    uint32_t id = 0u;
    if (P.ident) {
        id = P.ident[t];
        inert = inert || id == kDenoiseEmpty;
    }
    if (P.normal) {
        float4_t n;
        n.x = P.normal[3 * t], n.y = P.normal[3 * t + 1], n.z = P.normal[3 * t + 2], n.w = 0.0f;
        inert = inert || !finite3(n.x, n.y, n.z);
        P.normal4[t] = n;
    }
    if (P.position) {
        float4_t p;
        p.x = P.position[3 * t], p.y = P.position[3 * t + 1], p.z = P.position[3 * t + 2], p.w = 0.0f;
        inert = inert || !finite3(p.x, p.y, p.z);
        P.position4[t] = p;
    }
    c.w = __uint_as_float(inert ? kDenoiseEmpty : id);
    P.color4[t] = c;
}

// One pass. NORMAL: the normal guide is given; POSITION: the position term is on (the guide is given
// and sigma_position > 0); COLOUR: the colour term is on. A term that is off loads nothing.
template <bool NORMAL, bool POSITION, bool COLOUR>
__global__ __launch_bounds__(kDenoiseBlockX * kDenoiseBlockY) void denoise_pass_kernel(DenoisePass P) {
    const int32_t x = int32_t(blockIdx.x) * kDenoiseBlockX + int32_t(threadIdx.x);
    const int32_t y = int32_t(blockIdx.y) * kDenoiseBlockY + int32_t(threadIdx.y);
    if (x >= P.width || y >= P.height) return;
    const int64_t t = int64_t(y) * P.width + x;
    const float4_t cp = P.src[t];
    const uint32_t idp = __float_as_uint(cp.w);
    float r0 = cp.x, r1 = cp.y, r2 = cp.z;
    if (idp != kDenoiseEmpty) {
        float4_t np = {0.0f, 0.0f, 0.0f, 0.0f}, pp = np;
        if (NORMAL) np = P.normal4[t];
        if (POSITION) pp = P.position4[t];
        const int32_t s = P.step;
        float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, wsum = 0.0f;
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy) {
            const int32_t qy = y + dy * s;
            if (qy < 0 || qy >= P.height) continue;
            const int64_t row = int64_t(qy) * P.width;
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                const int32_t qx = x + dx * s;
                if (qx < 0 || qx >= P.width) continue;
                const int64_t q = row + qx;
                const float4_t cq = P.src[q];
                if (__float_as_uint(cq.w) != idp) continue;  // inert, or another id
                // h = {1/16, 1/4, 3/8, 1/4, 1/16}: every product is exact
                const float hy = dy == 0 ? 0.375f : (dy == 1 || dy == -1) ? 0.25f : 0.0625f;
                const float hx = dx == 0 ? 0.375f : (dx == 1 || dx == -1) ? 0.25f : 0.0625f;
                float w = hy * hx;
                float4_t nq;
                if (NORMAL) {
                    nq = P.normal4[q];
                    float c = (np.x * nq.x + np.y * nq.y) + np.z * nq.z;
                    c = c > 0.0f ? c : 0.0f;
                    for (int32_t k = 0; k < P.normal_power; ++k) c = c * c;
                    w = w * c;
                }
                if (POSITION) {
                    const float4_t pq = P.position4[q];
                    const float vx = pq.x - pp.x, vy = pq.y - pp.y, vz = pq.z - pp.z;
                    float e2;
                    if (NORMAL) {
                        const float e = (np.x * vx + np.y * vy) + np.z * vz;
                        e2 = e * e;
                    } else {
                        e2 = (vx * vx + vy * vy) + vz * vz;
                    }
                    w = w * (1.0f / (1.0f + e2 * P.kp));
                }
                if (COLOUR) {
                    const float ux = cq.x - cp.x, uy = cq.y - cp.y, uz = cq.z - cp.z;
                    const float d2 = (ux * ux + uy * uy) + uz * uz;
                    w = w * (1.0f / (1.0f + d2 * P.kc));
                }
                if (!(w > 0.0f)) continue;  // zero, NaN, negative
                s0 = s0 + cq.x * w;
                s1 = s1 + cq.y * w;
                s2 = s2 + cq.z * w;
                wsum = wsum + w;
            }
        }
        if (wsum > 0.0f) {
            r0 = s0 / wsum;
            r1 = s1 / wsum;
            r2 = s2 / wsum;
        }
    }
    if (P.dst) {
        float4_t o;
        o.x = r0, o.y = r1, o.z = r2, o.w = cp.w;
        P.dst[t] = o;
    } else {
        if (P.out) {
            P.out[3 * t] = r0;
            P.out[3 * t + 1] = r1;
            P.out[3 * t + 2] = r2;
        }
        if (P.framebuffer) P.framebuffer[t] = denoise_bgrx(r0, r1, r2);
    }
}

}  // namespace atr

using namespace atr;

extern "C" {

hipError_t atr_launch_denoise_pack(const DenoisePack& P, hipStream_t s) {
    denoise_pack_kernel<<<dim3(uint32_t((P.npixels + 255) / 256)), dim3(256), 0, s>>>(P);
    return hipGetLastError();
}

hipError_t atr_launch_denoise_pass(const DenoisePass& P, int normal, int position, int colour, hipStream_t s) {
    const dim3 grid(uint32_t((P.width + kDenoiseBlockX - 1) / kDenoiseBlockX),
                    uint32_t((P.height + kDenoiseBlockY - 1) / kDenoiseBlockY));
    const dim3 block(kDenoiseBlockX, kDenoiseBlockY);
    switch ((normal ? 4 : 0) | (position ? 2 : 0) | (colour ? 1 : 0)) {
        case 0: denoise_pass_kernel<false, false, false><<<grid, block, 0, s>>>(P); break;
        case 1: denoise_pass_kernel<false, false, true><<<grid, block, 0, s>>>(P); break;
        case 2: denoise_pass_kernel<false, true, false><<<grid, block, 0, s>>>(P); break;
        case 3: denoise_pass_kernel<false, true, true><<<grid, block, 0, s>>>(P); break;
        case 4: denoise_pass_kernel<true, false, false><<<grid, block, 0, s>>>(P); break;
        case 5: denoise_pass_kernel<true, false, true><<<grid, block, 0, s>>>(P); break;
        case 6: denoise_pass_kernel<true, true, false><<<grid, block, 0, s>>>(P); break;
        default: denoise_pass_kernel<true, true, true><<<grid, block, 0, s>>>(P); break;
    }
    return hipGetLastError();
}

}  // extern "C"
