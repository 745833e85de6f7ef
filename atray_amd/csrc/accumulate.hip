// accumulate.hip -- atr_accumulate: temporal accumulation of a frame into a history reprojected from
// the previous camera; DESIGN.md §4t. One lane per pixel, the lanes of a wave along x: a lane reads its
// own pixel of this frame, inverts the previous camera's film mapping for its surface point and gathers
// the four previous pixels around it. Neighbouring lanes reproject to neighbouring taps, so the gathers
// of a wave are runs of the previous frame's rows (the very same run for a camera at rest). A guide
// that is absent is compiled out together with its loads. No LDS, no workspace, no atomics. Every f32
// operation is separately rounded (-ffp-contract=off), the divisions and floorf are IEEE, so
// tests/c/accumulate_ref.c equals the result bit for bit.
#include <hip/hip_runtime.h>

#include "accumulate.h"
#include "launch.h"

namespace atr {

namespace {

__device__ __forceinline__ bool acc_finite(float x) {
    return __builtin_fabsf(x) < __builtin_inff();  // false for an infinity and for a NaN
}
__device__ __forceinline__ float acc_dot(const float* a, float bx, float by, float bz) {
    return (a[0] * bx + a[1] * by) + a[2] * bz;
}

}  // namespace

// NORMAL, IDENT: the guide is given (in this frame and, with a previous frame, in that one too);
// MOMENTS: the histories carry moments.
template <bool NORMAL, bool IDENT, bool MOMENTS>
__global__ __launch_bounds__(kAccumulateBlockX * kAccumulateBlockY) void accumulate_kernel(AccumulateParams P) {
    const int32_t x = int32_t(blockIdx.x) * kAccumulateBlockX + int32_t(threadIdx.x);
    const int32_t y = int32_t(blockIdx.y) * kAccumulateBlockY + int32_t(threadIdx.y);
    if (x >= P.width || y >= P.height) return;
    const int64_t t = int64_t(y) * P.width + x;
    const float c0 = P.color[3 * t], c1 = P.color[3 * t + 1], c2 = P.color[3 * t + 2];
    bool inert = !(acc_finite(c0) && acc_finite(c1) && acc_finite(c2));
    uint32_t idp = 0u;
    if (IDENT) {
        idp = P.ident[t];
        inert = inert || idp == kDenoiseEmpty;
    }
    float n[3] = {0.0f, 0.0f, 0.0f}, p[3] = {0.0f, 0.0f, 0.0f};
    if (NORMAL) {
        n[0] = P.normal[3 * t], n[1] = P.normal[3 * t + 1], n[2] = P.normal[3 * t + 2];
        inert = inert || !(acc_finite(n[0]) && acc_finite(n[1]) && acc_finite(n[2]));
    }
    if (P.position) {
        p[0] = P.position[3 * t], p[1] = P.position[3 * t + 1], p[2] = P.position[3 * t + 2];
        inert = inert || !(acc_finite(p[0]) && acc_finite(p[1]) && acc_finite(p[2]));
    }
    float o0 = c0, o1 = c1, o2 = c2, m1 = 0.0f, m2 = 0.0f, var = 0.0f;
    uint32_t len = 0u;
    if (!inert) {
        float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, ms0 = 0.0f, ms1 = 0.0f, wsum = 0.0f;
        uint32_t nmin = 0xFFFFFFFFu;
        if (P.has_prev) {
            const float vx = p[0] - P.eye[0], vy = p[1] - P.eye[1], vz = p[2] - P.eye[2];
            const float depth = -acc_dot(P.cz, vx, vy, vz);
            if (depth > 0.0f) {
                const float a = acc_dot(P.cx, vx, vy, vz) / depth;
                const float b = acc_dot(P.cy, vx, vy, vz) / depth;
                const float sx = (a / P.k + 1.0f) * P.hw;
                const float sy = (b + 1.0f) * P.hh;
                if (sx >= -1.0f && sx < P.fw && sy >= -1.0f && sy < P.fh) {
                    const float fx0 = floorf(sx), fy0 = floorf(sy);
                    const int32_t x0 = int32_t(fx0), y0 = int32_t(fy0);
                    const float tx = sx - fx0, ty = sy - fy0;
                    const float tol = P.plane_tolerance * depth;
                    const float tol2 = tol * tol;
#pragma unroll
                    for (int dy = 0; dy < 2; ++dy) {
                        const int32_t qy = y0 + dy;
                        if (qy < 0 || qy >= P.height) continue;
#pragma unroll
                        for (int dx = 0; dx < 2; ++dx) {
                            const int32_t qx = x0 + dx;
                            if (qx < 0 || qx >= P.width) continue;
                            const int64_t q = int64_t(qy) * P.width + qx;
                            const uint32_t lq = P.prev_length[q];
                            if (lq == 0u) continue;
                            if (IDENT) {
                                const uint32_t idq = P.prev_ident[q];
                                if (idq != idp || idq == kDenoiseEmpty) continue;
                            }
                            if (NORMAL) {
                                const float d = acc_dot(n, P.prev_normal[3 * q], P.prev_normal[3 * q + 1],
                                                        P.prev_normal[3 * q + 2]);
                                if (!(d >= P.min_normal_dot)) continue;
                            }
                            const float ux = P.prev_position[3 * q] - p[0], uy = P.prev_position[3 * q + 1] - p[1],
                                        uz = P.prev_position[3 * q + 2] - p[2];
                            float e2;
                            if (NORMAL) {
                                const float e = acc_dot(n, ux, uy, uz);
                                e2 = e * e;
                            } else {
                                e2 = (ux * ux + uy * uy) + uz * uz;
                            }
                            if (!(e2 <= tol2)) continue;
                            const float h0 = P.prev_color[3 * q], h1 = P.prev_color[3 * q + 1],
                                        h2 = P.prev_color[3 * q + 2];
                            if (!(acc_finite(h0) && acc_finite(h1) && acc_finite(h2))) continue;
                            float q0 = 0.0f, q1 = 0.0f;
                            if (MOMENTS) {
                                q0 = P.prev_moments[2 * q], q1 = P.prev_moments[2 * q + 1];
                                if (!(acc_finite(q0) && acc_finite(q1))) continue;
                            }
                            const float w = (dx ? tx : 1.0f - tx) * (dy ? ty : 1.0f - ty);
                            if (!(w > 0.0f)) continue;
                            s0 = s0 + h0 * w;
                            s1 = s1 + h1 * w;
                            s2 = s2 + h2 * w;
                            if (MOMENTS) {
                                ms0 = ms0 + q0 * w;
                                ms1 = ms1 + q1 * w;
                            }
                            wsum = wsum + w;
                            nmin = lq < nmin ? lq : nmin;
                        }
                    }
                }
            }
        }
        const float l = (0.2126f * c0 + 0.7152f * c1) + 0.0722f * c2;
        if (wsum > 0.0f) {
            const float h0 = s0 / wsum, h1 = s1 / wsum, h2 = s2 / wsum;
            const uint32_t cap = P.max_length - 1u;
            len = (nmin < cap ? nmin : cap) + 1u;
            const float aw = 1.0f / float(len);
            const float ac = P.alpha > aw ? P.alpha : aw;
            o0 = h0 + (c0 - h0) * ac;
            o1 = h1 + (c1 - h1) * ac;
            o2 = h2 + (c2 - h2) * ac;
            if (MOMENTS) {
                const float hm0 = ms0 / wsum, hm1 = ms1 / wsum;
                const float am = P.alpha_moments > aw ? P.alpha_moments : aw;
                m1 = hm0 + (l - hm0) * am;
                m2 = hm1 + (l * l - hm1) * am;
            }
        } else {
            len = 1u;
            m1 = l;
            m2 = l * l;
        }
        if (MOMENTS) {
            var = m2 - m1 * m1;
            var = var > 0.0f ? var : 0.0f;
        }
    }
    P.out_color[3 * t] = o0;
    P.out_color[3 * t + 1] = o1;
    P.out_color[3 * t + 2] = o2;
    P.out_length[t] = len;
    if (MOMENTS) {
        P.out_moments[2 * t] = m1;
        P.out_moments[2 * t + 1] = m2;
        if (P.variance) P.variance[t] = var;
    }
    if (P.framebuffer) P.framebuffer[t] = denoise_bgrx(o0, o1, o2);
}

}  // namespace atr

using namespace atr;

extern "C" {

hipError_t atr_launch_accumulate(const AccumulateParams& P, hipStream_t s) {
    const dim3 grid(uint32_t((P.width + kAccumulateBlockX - 1) / kAccumulateBlockX),
                    uint32_t((P.height + kAccumulateBlockY - 1) / kAccumulateBlockY));
    const dim3 block(kAccumulateBlockX, kAccumulateBlockY);
    switch ((P.normal ? 4 : 0) | (P.ident ? 2 : 0) | (P.out_moments ? 1 : 0)) {
        case 0: accumulate_kernel<false, false, false><<<grid, block, 0, s>>>(P); break;
        case 1: accumulate_kernel<false, false, true><<<grid, block, 0, s>>>(P); break;
        case 2: accumulate_kernel<false, true, false><<<grid, block, 0, s>>>(P); break;
        case 3: accumulate_kernel<false, true, true><<<grid, block, 0, s>>>(P); break;
        case 4: accumulate_kernel<true, false, false><<<grid, block, 0, s>>>(P); break;
        case 5: accumulate_kernel<true, false, true><<<grid, block, 0, s>>>(P); break;
        case 6: accumulate_kernel<true, true, false><<<grid, block, 0, s>>>(P); break;
        default: accumulate_kernel<true, true, true><<<grid, block, 0, s>>>(P); break;
    }
    return hipGetLastError();
}

}  // extern "C"
