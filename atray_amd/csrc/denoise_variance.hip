// denoise_variance.hip -- atr_denoise_variance: the spatial stage of SVGF (Schied et al. 2017) on
// atr_denoise's a-trous pattern; DESIGN.md §4u. The luminance stopping weight is scaled per pixel by the
// local standard deviation (a 3 x 3 Gaussian of the variance image), the variance is filtered along with
// the colour, and a pixel whose history is too short takes its variance from a 7 x 7 window of the
// moments. A pack kernel reads the caller's colour, variance and guides once (so out == color and
// variance_out == variance are safe) and writes records; the estimate reads the caller's moments and
// lengths and nothing another lane writes; every pass is one lane per pixel, the lanes of a wave along
// x. Every f32 operation is separately rounded (-ffp-contract=off), the divisions and the square root
// are IEEE, so tests/c/denoise_variance_ref.c equals the result bit for bit.
#include <hip/hip_runtime.h>

#include "denoise_variance.h"
#include "launch.h"

namespace atr {

namespace {

__device__ __forceinline__ bool dv_finite(float x) { return __builtin_fabsf(x) < __builtin_inff(); }

__device__ __forceinline__ bool dv_finite3(float x, float y, float z) {
    return dv_finite(x) && dv_finite(y) && dv_finite(z);
}

__device__ __forceinline__ float dv_lum(float r, float g, float b) {
    return (0.2126f * r + 0.7152f * g) + 0.0722f * b;
}

// atr_denoise's normal term: max(dot, 0)^(2^power)
__device__ __forceinline__ float dv_normal_term(const float4_t& np, const float4_t& nq, int32_t power) {
    float c = (np.x * nq.x + np.y * nq.y) + np.z * nq.z;
    c = c > 0.0f ? c : 0.0f;
    for (int32_t k = 0; k < power; ++k) c = c * c;
    return c;
}

// atr_denoise's position term: the distance from P's tangent plane with a normal, else the distance
template <bool NORMAL>
__device__ __forceinline__ float dv_position_term(const float4_t& np, const float4_t& pp, const float4_t& pq, float kp) {
    const float vx = pq.x - pp.x, vy = pq.y - pp.y, vz = pq.z - pp.z;
    float e2;
    if (NORMAL) {
        const float e = (np.x * vx + np.y * vy) + np.z * vz;
        e2 = e * e;
    } else {
        e2 = (vx * vx + vy * vy) + vz * vz;
    }
    return 1.0f / (1.0f + e2 * kp);
}

}  // namespace

// One lane per pixel: inertness, the sanitised variance, the luminance and the records.
__global__ __launch_bounds__(256) void denoise_variance_pack_kernel(DenoiseVarPack P) {
    const int64_t t = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (t >= P.npixels) return;
    float4_t c;
    c.x = P.color[3 * t], c.y = P.color[3 * t + 1], c.z = P.color[3 * t + 2];
    bool inert = !dv_finite3(c.x, c.y, c.z);
    uint32_t id = 0u;
    if (P.ident) {
        id = P.ident[t];
        inert = inert || id == kDenoiseEmpty;
    }
    if (P.normal) {
        float4_t n;
        n.x = P.normal[3 * t], n.y = P.normal[3 * t + 1], n.z = P.normal[3 * t + 2], n.w = 0.0f;
        inert = inert || !dv_finite3(n.x, n.y, n.z);
        P.normal4[t] = n;
    }
    if (P.position) {
        float4_t p;
        p.x = P.position[3 * t], p.y = P.position[3 * t + 1], p.z = P.position[3 * t + 2], p.w = 0.0f;
        inert = inert || !dv_finite3(p.x, p.y, p.z);
        P.position4[t] = p;
    }
    const float v = P.variance[t];
    float2_t vl;
    vl.x = (!inert && v > 0.0f && v < __builtin_inff()) ? v : 0.0f;  // a NaN fails both comparisons
    vl.y = dv_lum(c.x, c.y, c.z);
    c.w = __uint_as_float(inert ? kDenoiseEmpty : id);
    P.color4[t] = c;
    P.vl[t] = vl;
}

// The spatial estimate of a live pixel whose history is shorter than `below`: the moments of its 7 x 7
// window under the normal and position weights, boosted by below / length.
template <bool NORMAL, bool POSITION>
__global__ __launch_bounds__(kDenoiseBlockX * kDenoiseBlockY) void denoise_variance_estimate_kernel(DenoiseVarEstimate P) {
    const int32_t x = int32_t(blockIdx.x) * kDenoiseBlockX + int32_t(threadIdx.x);
    const int32_t y = int32_t(blockIdx.y) * kDenoiseBlockY + int32_t(threadIdx.y);
    if (x >= P.width || y >= P.height) return;
    const int64_t t = int64_t(y) * P.width + x;
    const uint32_t idp = __float_as_uint(P.color4[t].w);
    if (idp == kDenoiseEmpty) return;
    const uint32_t lp = P.length[t];
    if (!(lp < P.below)) return;
    float4_t np = {0.0f, 0.0f, 0.0f, 0.0f}, pp = np;
    if (NORMAL) np = P.normal4[t];
    if (POSITION) pp = P.position4[t];
    float a = 0.0f, b = 0.0f, ws = 0.0f;
    for (int dy = -3; dy <= 3; ++dy) {
        const int32_t qy = y + dy;
        if (qy < 0 || qy >= P.height) continue;
        const int64_t row = int64_t(qy) * P.width;
#pragma unroll
        for (int dx = -3; dx <= 3; ++dx) {
            const int32_t qx = x + dx;
            if (qx < 0 || qx >= P.width) continue;
            const int64_t q = row + qx;
            if (__float_as_uint(P.color4[q].w) != idp) continue;  // inert, or another id
            const float2_t m = P.moments[q];
            if (!(dv_finite(m.x) && dv_finite(m.y))) continue;
            float w = 1.0f;
            if (NORMAL) w = w * dv_normal_term(np, P.normal4[q], P.normal_power);
            if (POSITION) w = w * dv_position_term<NORMAL>(np, pp, P.position4[q], P.kp);
            if (!(w > 0.0f)) continue;
            a = a + m.x * w;
            b = b + m.y * w;
            ws = ws + w;
        }
    }
    if (ws > 0.0f) {
        const float m1 = a / ws, m2 = b / ws;
        float e = m2 - m1 * m1;
        e = e > 0.0f ? e : 0.0f;
        const uint32_t l1 = lp > 0u ? lp : 1u;
        P.vl[t].x = e * (P.fbelow / float(l1));
    }
}

// One pass. NORMAL: the normal guide is given; POSITION: the position term is on (the guide is given and
// sigma_position > 0); LUMINANCE: the luminance term is on. A term that is off loads nothing more.
template <bool NORMAL, bool POSITION, bool LUMINANCE>
__global__ __launch_bounds__(kDenoiseBlockX * kDenoiseBlockY) void denoise_variance_pass_kernel(DenoiseVarPass P) {
    const int32_t x = int32_t(blockIdx.x) * kDenoiseBlockX + int32_t(threadIdx.x);
    const int32_t y = int32_t(blockIdx.y) * kDenoiseBlockY + int32_t(threadIdx.y);
    if (x >= P.width || y >= P.height) return;
    const int64_t t = int64_t(y) * P.width + x;
    const float4_t cp = P.src[t];
    const float2_t vp = P.src_vl[t];
    const uint32_t idp = __float_as_uint(cp.w);
    float r0 = cp.x, r1 = cp.y, r2 = cp.z, rv = vp.x, rl = vp.y;
    if (idp != kDenoiseEmpty) {
        float rlum = 0.0f;
        if (LUMINANCE) {
            // the variance under a 3 x 3 Gaussian at spacing 1, over the taps of P's kind
            float gs = 0.0f, ks = 0.0f;
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy) {
                const int32_t qy = y + dy;
                if (qy < 0 || qy >= P.height) continue;
                const int64_t row = int64_t(qy) * P.width;
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    const int32_t qx = x + dx;
                    if (qx < 0 || qx >= P.width) continue;
                    const int64_t q = row + qx;
                    if (__float_as_uint(P.src[q].w) != idp) continue;
                    const float k = (dy == 0 ? 0.5f : 0.25f) * (dx == 0 ? 0.5f : 0.25f);
                    gs = gs + P.src_vl[q].x * k;
                    ks = ks + k;
                }
            }
            const float gv = gs / ks;
            rlum = 1.0f / (P.sigma_luminance * sqrtf(gv) + P.luminance_floor);
        }
        float4_t np = {0.0f, 0.0f, 0.0f, 0.0f}, pp = np;
        if (NORMAL) np = P.normal4[t];
        if (POSITION) pp = P.position4[t];
        const int32_t s = P.step;
        float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, vs = 0.0f, wsum = 0.0f;
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
                const float2_t vq = P.src_vl[q];
                // h = {1/16, 1/4, 3/8, 1/4, 1/16}: every product is exact
                const float hy = dy == 0 ? 0.375f : (dy == 1 || dy == -1) ? 0.25f : 0.0625f;
                const float hx = dx == 0 ? 0.375f : (dx == 1 || dx == -1) ? 0.25f : 0.0625f;
                float w = hy * hx;
                if (NORMAL) w = w * dv_normal_term(np, P.normal4[q], P.normal_power);
                if (POSITION) w = w * dv_position_term<NORMAL>(np, pp, P.position4[q], P.kp);
                if (LUMINANCE) {
                    const float xl = __builtin_fabsf(vq.y - vp.y) * rlum;
                    w = w * (1.0f / (1.0f + xl));
                }
                if (!(w > 0.0f)) continue;  // zero, NaN, negative
                s0 = s0 + cq.x * w;
                s1 = s1 + cq.y * w;
                s2 = s2 + cq.z * w;
                vs = vs + vq.x * (w * w);
                wsum = wsum + w;
            }
        }
        if (wsum > 0.0f) {
            r0 = s0 / wsum;
            r1 = s1 / wsum;
            r2 = s2 / wsum;
            rv = vs / (wsum * wsum);
            rl = dv_lum(r0, r1, r2);
        }
    }
    if (P.dst) {
        float4_t o;
        o.x = r0, o.y = r1, o.z = r2, o.w = cp.w;
        float2_t ov;
        ov.x = rv, ov.y = rl;
        P.dst[t] = o;
        P.dst_vl[t] = ov;
    } else {
        if (P.out) {
            P.out[3 * t] = r0;
            P.out[3 * t + 1] = r1;
            P.out[3 * t + 2] = r2;
        }
        if (P.variance_out) P.variance_out[t] = rv;
        if (P.framebuffer) P.framebuffer[t] = denoise_bgrx(r0, r1, r2);
    }
}

}  // namespace atr

using namespace atr;

extern "C" {

hipError_t atr_launch_denoise_variance_pack(const DenoiseVarPack& P, hipStream_t s) {
    denoise_variance_pack_kernel<<<dim3(uint32_t((P.npixels + 255) / 256)), dim3(256), 0, s>>>(P);
    return hipGetLastError();
}

hipError_t atr_launch_denoise_variance_estimate(const DenoiseVarEstimate& P, int normal, int position, hipStream_t s) {
    const dim3 grid(uint32_t((P.width + kDenoiseBlockX - 1) / kDenoiseBlockX),
                    uint32_t((P.height + kDenoiseBlockY - 1) / kDenoiseBlockY));
    const dim3 block(kDenoiseBlockX, kDenoiseBlockY);
    switch ((normal ? 2 : 0) | (position ? 1 : 0)) {
        case 0: denoise_variance_estimate_kernel<false, false><<<grid, block, 0, s>>>(P); break;
        case 1: denoise_variance_estimate_kernel<false, true><<<grid, block, 0, s>>>(P); break;
        case 2: denoise_variance_estimate_kernel<true, false><<<grid, block, 0, s>>>(P); break;
        default: denoise_variance_estimate_kernel<true, true><<<grid, block, 0, s>>>(P); break;
    }
    return hipGetLastError();
}

hipError_t atr_launch_denoise_variance_pass(const DenoiseVarPass& P, int normal, int position, int luminance,
                                            hipStream_t s) {
    const dim3 grid(uint32_t((P.width + kDenoiseBlockX - 1) / kDenoiseBlockX),
                    uint32_t((P.height + kDenoiseBlockY - 1) / kDenoiseBlockY));
    const dim3 block(kDenoiseBlockX, kDenoiseBlockY);
    switch ((normal ? 4 : 0) | (position ? 2 : 0) | (luminance ? 1 : 0)) {
        case 0: denoise_variance_pass_kernel<false, false, false><<<grid, block, 0, s>>>(P); break;
        case 1: denoise_variance_pass_kernel<false, false, true><<<grid, block, 0, s>>>(P); break;
        case 2: denoise_variance_pass_kernel<false, true, false><<<grid, block, 0, s>>>(P); break;
        case 3: denoise_variance_pass_kernel<false, true, true><<<grid, block, 0, s>>>(P); break;
        case 4: denoise_variance_pass_kernel<true, false, false><<<grid, block, 0, s>>>(P); break;
        case 5: denoise_variance_pass_kernel<true, false, true><<<grid, block, 0, s>>>(P); break;
        case 6: denoise_variance_pass_kernel<true, true, false><<<grid, block, 0, s>>>(P); break;
        default: denoise_variance_pass_kernel<true, true, true><<<grid, block, 0, s>>>(P); break;
    }
    return hipGetLastError();
}

}  // extern "C"
