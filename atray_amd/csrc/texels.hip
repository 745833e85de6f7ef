// texels.hip -- a mesh's lightmap texels on the device (atr_mesh_texels) and per-texel results back
// into an image (atr_texels_to_image); DESIGN.md §4r. Coverage: one atomicMin per covering (face,
// texel) on a u32 face map, so the lowest covering face wins in any arrival order; slots: a two-level
// exclusive scan of the covered flags in texel order (no float atomics anywhere: every output is
// deterministic); samples: the lane of a covered texel recomputes the edge values with the function
// the coverage pass used (texels.h) and takes its normal from shade.h's scene_finish.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "launch.h"
#include "shade.h"
#include "texels.h"

namespace atr {

struct TexelFace {
    UV a, b, c;
    float area2, g;
    bool usable;
};

__device__ __forceinline__ bool texel_finite(float x) { return fabsf(x) <= kMaxFloat; }  // false for NaN and inf

// A face's UV triangle. Usable iff its three texcoord indices are present (and inside the array), the
// six floats are finite and area2 is neither 0 nor NaN.
__device__ __forceinline__ TexelFace texel_face(const TexelMesh& M, uint32_t f) {
    TexelFace F;
    F.a = F.b = F.c = UV{0.f, 0.f};
    F.area2 = 0.f;
    F.g = 1.f;
    const int32_t* ft = M.face_t + 3 * size_t(f);
    const int32_t t0 = ft[0], t1 = ft[1], t2 = ft[2];
    F.usable = t0 >= 0 && t1 >= 0 && t2 >= 0 && uint32_t(t0) < M.ntexcoords && uint32_t(t1) < M.ntexcoords &&
               uint32_t(t2) < M.ntexcoords;
    if (!F.usable) return F;
    const float* tc = M.texcoords;
    F.a = UV{tc[3 * size_t(t0)], tc[3 * size_t(t0) + 1]};
    F.b = UV{tc[3 * size_t(t1)], tc[3 * size_t(t1) + 1]};
    F.c = UV{tc[3 * size_t(t2)], tc[3 * size_t(t2) + 1]};
    F.usable = texel_finite(F.a.x) && texel_finite(F.a.y) && texel_finite(F.b.x) && texel_finite(F.b.y) &&
               texel_finite(F.c.x) && texel_finite(F.c.y);
    if (!F.usable) return F;
    F.area2 = texel_area2(F.a, F.b, F.c);
    F.usable = F.area2 != 0.0f && F.area2 == F.area2;
    F.g = F.area2 > 0.0f ? 1.0f : -1.0f;
    return F;
}

// The texels a face's lanes test: i0 .. i0 + nx - 1, j0 .. j0 + ny - 1 (nx or ny 0: none). The result is
// the rule's alone, so the box only has to hold every centre the rule can accept. A face with
// coordinates within +-64, an extent L = max(dx, dy) within 2^-40 .. 2^40 and |area2| >= 2^-16 L^2 (no
// sliver) gets its UV bounds grown by a whole texel. The argument: each difference and
// product of an edge value is off by 2^-24 of itself, which for such a face is what moving the centre
// by less than 2^-17 (|p - p0| <= 65) and turning the edge by about 2^-23 rad would do; a centre a whole
// texel (>= 2^-14) outside the bounds stays outside a triangle none of whose angles is that small.
// Any other face -- a sliver, far or huge coordinates -- gets the whole map. Every float is clamped
// into the map before it becomes an integer.
struct TexelBox { int32_t i0, j0, nx, ny; };
__device__ __forceinline__ void texel_span(float lo, float hi, float nf, int32_t& first, int32_t& count) {
    const float a = fminf(fmaxf(floorf(lo * nf - 1.5f), 0.0f), nf);         // 0 .. n
    const float b = fmaxf(fminf(ceilf(hi * nf + 0.5f), nf - 1.0f), -1.0f);  // -1 .. n - 1
    first = int32_t(a);
    count = int32_t(b) >= first ? int32_t(b) - first + 1 : 0;
}
__device__ __forceinline__ TexelBox texel_box(const TexelFace& F, int32_t W, int32_t H) {
    const float minx = fminf(fminf(F.a.x, F.b.x), F.c.x), maxx = fmaxf(fmaxf(F.a.x, F.b.x), F.c.x);
    const float miny = fminf(fminf(F.a.y, F.b.y), F.c.y), maxy = fmaxf(fmaxf(F.a.y, F.b.y), F.c.y);
    const float L = fmaxf(maxx - minx, maxy - miny);
    const float far = fmaxf(fmaxf(fabsf(minx), fabsf(maxx)), fmaxf(fabsf(miny), fabsf(maxy)));
    const bool fat = far <= 64.0f && L >= 0x1p-40f && L <= 0x1p40f && fabsf(F.area2) >= 0x1p-16f * (L * L);
    TexelBox B{0, 0, W, H};
    if (fat) {
        texel_span(minx, maxx, float(W), B.i0, B.nx);
        texel_span(miny, maxy, float(H), B.j0, B.ny);
    }
    return B;
}

__device__ __forceinline__ void texel_test(const TexelParams& P, const TexelFace& F, uint32_t f, int32_t i, int32_t j) {
    float e1, e2, den;
    if (texel_cover(F.a, F.b, F.c, F.g, texel_centre(i, j, float(P.width), float(P.height)), e1, e2, den))
        atomicMin(P.map + (size_t(j) * size_t(P.width) + size_t(i)), f);
}

// One lane per face: a box of at most kTexelSmallBox texels is finished here; a larger one goes to the
// list, appended with one ballot and one atomic per wave.
__global__ __launch_bounds__(256) void texel_classify_kernel(TexelParams P) {
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    bool big = false;
    if (f < P.mesh.nfaces) {
        const TexelFace F = texel_face(P.mesh, f);
        if (F.usable) {
            const TexelBox B = texel_box(F, P.width, P.height);
            const int64_t n = int64_t(B.nx) * int64_t(B.ny);
            if (n > kTexelSmallBox) big = true;
            else
                for (int32_t k = 0; k < int32_t(n); ++k) texel_test(P, F, f, B.i0 + k % B.nx, B.j0 + k / B.nx);
        }
    }
    const unsigned long long m = __ballot(big);
    if (m) {  // wave-uniform
        const int lane = threadIdx.x & 63, lead = __ffsll(m) - 1;
        uint32_t base = 0;
        if (lane == lead) base = atomicAdd(P.nbig, uint32_t(__popcll(m)));
        base = __shfl(base, lead);
        if (big) P.big[base + uint32_t(__popcll(m & ((1ull << lane) - 1ull)))] = f;  // < nfaces entries in all
    }
}

// kTexelFaceWaves waves (4 blocks) per listed face: wave q takes the 8x8 tiles q, q + 16, ... of its box.
__global__ __launch_bounds__(256) void texel_big_kernel(TexelParams P) {
    constexpr uint32_t kBlocksPerFace = kTexelFaceWaves / 4;
    const uint32_t entry = blockIdx.x / kBlocksPerFace;
    if (entry >= *P.nbig) return;
    const uint32_t f = P.big[entry];
    if (f >= P.mesh.nfaces) return;
    const TexelFace F = texel_face(P.mesh, f);
    if (!F.usable) return;
    const TexelBox B = texel_box(F, P.width, P.height);
    const int32_t tnx = (B.nx + 7) / 8, tny = (B.ny + 7) / 8, ntiles = tnx * tny;  // <= 2048 x 2048
    const int32_t lane = threadIdx.x & 63;
    for (int32_t t = int32_t(blockIdx.x % kBlocksPerFace) * 4 + int32_t(threadIdx.x >> 6); t < ntiles; t += kTexelFaceWaves) {
        const int32_t di = (t % tnx) * 8 + (lane & 7), dj = (t / tnx) * 8 + (lane >> 3);
        if (di < B.nx && dj < B.ny) texel_test(P, F, f, B.i0 + di, B.j0 + dj);
    }
}

// Slot scan, level 1: the covered count of each block of kTexelScanBlock texels. The map is padded to
// whole blocks with kTexelNone. Thread t of a block reads the texels base + 256 q + t, q = 0..3.
__global__ __launch_bounds__(256) void texel_count_kernel(TexelParams P) {
    __shared__ uint32_t part[4];
    const size_t base = size_t(blockIdx.x) * kTexelScanBlock;
    uint32_t cnt = 0;
    for (int q = 0; q < 4; ++q) cnt += uint32_t(__popcll(__ballot(P.map[base + size_t(q) * 256 + threadIdx.x] != kTexelNone)));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) P.sums[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}

// Level 2, one workgroup of 1,024 threads: the block counts (at most 2^28 / 1,024 = 262,144, so at most
// 256 consecutive ones per thread) become exclusive offsets in place; sums[nblocks] = the total.
__global__ __launch_bounds__(1024) void texel_scan_kernel(TexelParams P) {
    __shared__ uint32_t sh[1024];
    const uint32_t nb = P.nblocks, per = (nb + 1023u) / 1024u;
    const uint32_t first = min(threadIdx.x * per, nb), end = min(first + per, nb);
    uint32_t own = 0;
    for (uint32_t i = first; i < end; ++i) own += P.sums[i];
    sh[threadIdx.x] = own;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {
        const uint32_t v = threadIdx.x >= d ? sh[threadIdx.x - d] : 0u;
        __syncthreads();
        sh[threadIdx.x] += v;
        __syncthreads();
    }
    uint32_t run = sh[threadIdx.x] - own;
    for (uint32_t i = first; i < end; ++i) {
        const uint32_t v = P.sums[i];
        P.sums[i] = run;
        run += v;
    }
    if (threadIdx.x == 1023u) P.sums[nb] = sh[1023];
}

// The surface sample of covered texel t (rank k, face f).
__device__ __forceinline__ void texel_sample(const TexelParams& P, uint32_t t, uint32_t f, uint32_t k) {
    const atr_texels_out& O = P.out;
    if (O.texel) O.texel[k] = int32_t(t);
    if (O.face) O.face[k] = f;
    if (!O.bary && !O.point && !O.normal) return;
    const TexelFace F = texel_face(P.mesh, f);
    float e1, e2, den;
    const int32_t i = int32_t(t % uint32_t(P.width)), j = int32_t(t / uint32_t(P.width));
    (void)texel_cover(F.a, F.b, F.c, F.g, texel_centre(i, j, float(P.width), float(P.height)), e1, e2, den);
    const float u = e1 / den, v = e2 / den;
    if (O.bary) {
        O.bary[2 * size_t(k)] = u;
        O.bary[2 * size_t(k) + 1] = v;
    }
    if (O.point) {
        V3 vt[3];
        for (int q = 0; q < 3; ++q) {  // a vertex index outside the array reads as the origin, as the upload does
            const int32_t vi = P.mesh.face_v[3 * size_t(f) + q];
            vt[q] = mk(0.f, 0.f, 0.f);
            if (vi >= 0 && uint32_t(vi) < P.mesh.nvertices)
                vt[q] = mk(P.mesh.vertices[3 * size_t(vi)], P.mesh.vertices[3 * size_t(vi) + 1], P.mesh.vertices[3 * size_t(vi) + 2]);
        }
        const V3 p = add(add(vt[0], scale(sub(vt[1], vt[0]), u)), scale(sub(vt[2], vt[0]), v));
        O.point[3 * size_t(k)] = p.x;
        O.point[3 * size_t(k) + 1] = p.y;
        O.point[3 * size_t(k) + 2] = p.z;
    }
    if (O.normal) {  // the renderer's own normal for a hit of model 0 at (f, u, v); no sphere, no plane
        Isect id;
        scene_finish(P.mesh.shade, mk(0.f, 0.f, 0.f), mk(0.f, 0.f, 1.f), kMaxFloat, f, u, v, 0, id);
        const V3 n = P.flip ? neg(id.normal) : id.normal;
        O.normal[3 * size_t(k)] = n.x;
        O.normal[3 * size_t(k) + 1] = n.y;
        O.normal[3 * size_t(k) + 2] = n.z;
    }
}

// Level 1 again, now with each block's offset: a covered texel's rank is the offset, plus the counts
// of the (q, wave) groups before its own in the block, plus the covered lanes below it in its ballot.
__global__ __launch_bounds__(256) void texel_write_kernel(TexelParams P) {
    __shared__ uint32_t part[16];
    const size_t base = size_t(blockIdx.x) * kTexelScanBlock;
    const size_t ntexels = size_t(P.width) * size_t(P.height);
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t face[4];
    unsigned long long bal[4];
    for (int q = 0; q < 4; ++q) {
        face[q] = P.map[base + size_t(q) * 256 + threadIdx.x];
        bal[q] = __ballot(face[q] != kTexelNone);
        if (lane == 0) part[q * 4 + w] = uint32_t(__popcll(bal[q]));
    }
    __syncthreads();
    uint32_t run = P.sums[blockIdx.x], pre[4] = {0, 0, 0, 0};
    for (int g = 0; g < 16; ++g) {
        if ((g & 3) == w) pre[g >> 2] = run;
        run += part[g];
    }
    for (int q = 0; q < 4; ++q) {
        const size_t t = base + size_t(q) * 256 + threadIdx.x;
        if (t >= ntexels) continue;
        const bool covered = face[q] != kTexelNone;
        const uint32_t k = pre[q] + uint32_t(__popcll(bal[q] & ((1ull << lane) - 1ull)));
        if (P.out.slot) P.out.slot[t] = covered ? int32_t(k) : -1;
        if (covered && P.fill) texel_sample(P, uint32_t(t), face[q], k);
    }
}

// ---------------------------------------------------------------- atr_texels_to_image
// image[texel[k]] = values[k]; a texel index outside the map is skipped.
__global__ __launch_bounds__(256) void texel_scatter_kernel(const float* __restrict__ values, const int32_t* __restrict__ texel,
                                                            int64_t n, int64_t ntexels, float* __restrict__ image,
                                                            uint8_t* __restrict__ flag) {
    const int64_t k = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (k >= n) return;
    const int64_t t = texel[k];
    if (t < 0 || t >= ntexels) return;
    image[3 * t] = values[3 * k];
    image[3 * t + 1] = values[3 * k + 1];
    image[3 * t + 2] = values[3 * k + 2];
    flag[t] = 1;
}

// One dilation pass, one lane per texel: reads only the state at the pass's start (src), writes dst.
__global__ __launch_bounds__(256) void texel_dilate_kernel(TexelImageParams P) {
    const int64_t t = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (t >= int64_t(P.width) * int64_t(P.height)) return;
    const int32_t i = int32_t(t % P.width), j = int32_t(t / P.width);
    float r[3];
    uint8_t full = P.src_flag[t];
    if (full) {
        for (int ch = 0; ch < 3; ++ch) r[ch] = P.src[3 * t + ch];
    } else {
        float s[3] = {0.f, 0.f, 0.f};
        int32_t n = 0;
        for (int32_t dy = -1; dy <= 1; ++dy)
            for (int32_t dx = -1; dx <= 1; ++dx) {
                const int32_t x = i + dx, y = j + dy;
                if (x < 0 || y < 0 || x >= P.width || y >= P.height) continue;
                const int64_t q = int64_t(y) * P.width + x;
                if (!P.src_flag[q]) continue;  // the texel itself is empty
                for (int ch = 0; ch < 3; ++ch) s[ch] = s[ch] + P.src[3 * q + ch];
                ++n;
            }
        if (n) {
            for (int ch = 0; ch < 3; ++ch) r[ch] = s[ch] / float(n);
            full = 1;
        } else {
            for (int ch = 0; ch < 3; ++ch) r[ch] = P.last ? P.fill[ch] : 0.f;
        }
    }
    for (int ch = 0; ch < 3; ++ch) P.dst[3 * t + ch] = r[ch];
    P.dst_flag[t] = full;
}

// Without a dilation pass: the empty texels get `fill`.
__global__ __launch_bounds__(256) void texel_fill_kernel(TexelImageParams P) {
    const int64_t t = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (t >= int64_t(P.width) * int64_t(P.height) || P.src_flag[t]) return;
    for (int ch = 0; ch < 3; ++ch) P.dst[3 * t + ch] = P.fill[ch];
}

}  // namespace atr

using namespace atr;

extern "C" {

hipError_t atr_launch_texel_classify(const TexelParams& P, hipStream_t s) {
    if (!P.mesh.nfaces) return hipSuccess;
    texel_classify_kernel<<<dim3((P.mesh.nfaces + 255u) / 256u), dim3(256), 0, s>>>(P);
    return hipGetLastError();
}

hipError_t atr_launch_texel_big(const TexelParams& P, uint32_t nbig, hipStream_t s) {
    if (!nbig) return hipSuccess;
    texel_big_kernel<<<dim3(nbig * uint32_t(kTexelFaceWaves / 4)), dim3(256), 0, s>>>(P);
    return hipGetLastError();
}

hipError_t atr_launch_texel_scan(const TexelParams& P, hipStream_t s) {
    texel_count_kernel<<<dim3(P.nblocks), dim3(256), 0, s>>>(P);
    texel_scan_kernel<<<dim3(1), dim3(1024), 0, s>>>(P);
    return hipGetLastError();
}

hipError_t atr_launch_texel_write(const TexelParams& P, hipStream_t s) {
    texel_write_kernel<<<dim3(P.nblocks), dim3(256), 0, s>>>(P);
    return hipGetLastError();
}

hipError_t atr_launch_texel_scatter(const float* values, const int32_t* texel, int64_t n, int64_t ntexels, float* image,
                                    uint8_t* flag, hipStream_t s) {
    if (!n) return hipSuccess;
    texel_scatter_kernel<<<dim3(uint32_t((n + 255) / 256)), dim3(256), 0, s>>>(values, texel, n, ntexels, image, flag);
    return hipGetLastError();
}

hipError_t atr_launch_texel_dilate(const TexelImageParams& P, hipStream_t s) {
    const int64_t n = int64_t(P.width) * int64_t(P.height);
    texel_dilate_kernel<<<dim3(uint32_t((n + 255) / 256)), dim3(256), 0, s>>>(P);
    return hipGetLastError();
}

hipError_t atr_launch_texel_fill(const TexelImageParams& P, hipStream_t s) {
    const int64_t n = int64_t(P.width) * int64_t(P.height);
    texel_fill_kernel<<<dim3(uint32_t((n + 255) / 256)), dim3(256), 0, s>>>(P);
    return hipGetLastError();
}

}  // extern "C"
