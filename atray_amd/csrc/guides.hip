// guides.hip -- a camera's denoiser guides in one device call (atr_camera_guides), and
// its primary rays as arrays (atr_camera_rays).
//   camera_guides_kernel  a wavefront per 8x8 cell of the tile list's block list, as render_kernel: the
//                         pixel's ray is made in registers (guides.h camera_ray_dir), tested (ray_ok),
//                         traced with the camera flavour of the clustered scan (u and v kept: a smooth
//                         mesh's normal needs them), finished (shade.h scene_finish) and turned into the
//                         guide record -- the faced normal, the hit point, the ident, t, the material --
//                         which is written once, in IMAGE layout;
//   camera_rays_kernel    elementwise: the same rays for a range of pixels, in pixel order.
// A file of its own: the render and path kernels' code objects are what they were without it.
#include <hip/hip_runtime.h>

#include "guides.h"
#include "launch.h"
#include "scan.h"

namespace atr {

// Waves/SIMD: the path engine's camera kernel's measured default (paths.hip kCameraOcc): the same
// scan instantiation with the same LDS, and less state held through it.
#ifndef ATR_GUIDES_OCC
#define ATR_GUIDES_OCC 6
#endif
constexpr int kGuidesOcc = ATR_GUIDES_OCC;  // experiment builds: -DATR_GUIDES_OCC=5

__global__ __launch_bounds__(256, kGuidesOcc) void camera_guides_kernel(GuidesParams P) {
    // the wave index is uniform: in an SGPR, so is the cell index derived from it
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int b = remap_xcd(blockIdx.x, gridDim.x, P.xcd_chunk) * 4 + wave;
    if (b >= P.nblocks) return;  // whole wavefront
    const DScene* S = uniform_global(P.scene);
    const V3 eye = from(P.cam.eye);
    int err = 0;
    SceneHit sh{kMaxFloat, 0.f, 0.f, 0u, -1};
    {
        const DBlock blk = P.blocks[b];
        const uint64_t mask = uint64_t(blk.mask_lo) | (uint64_t(blk.mask_hi) << 32);
        V3 d = camera_ray_dir(P.cam, blk.x0 + (lane & 7), blk.y0 + (lane >> 3));
        // a ray that fails the test is an inactive lane with a placeholder direction (as the ray
        // query's); the origin stays the eye, the one origin of the wave
        const bool ok = ray_ok(eye, d);
        if (!ok) d = mk(0.f, 0.f, 1.f);
        const bool active = ((mask >> lane) & 1) && ok;
        // a wave without a ray to trace (a degenerate camera) reads nothing of the scene
        if (__ballot(active) != 0) {
            Ctr ct;
            sh = intersect_models<SCHED_HYBRID, FlavCamera, false>(S, eye, d, active, err, ct, P.hyb_a, P.hyb_b);
        }
    }
    // the pixel and its ray from the cell record read again, instead of being held through the query
    // (render.hip's idiom: the asm clobber keeps the compiler from reusing the first read)
    __asm__ volatile("" ::: "memory");
    const DBlock ob = P.blocks[b];
    int olane = int(threadIdx.x);
    __asm__ volatile("" : "+v"(olane));  // recomputed here, not kept from the start
    olane &= 63;
    const uint64_t omask = uint64_t(ob.mask_lo) | (uint64_t(ob.mask_hi) << 32);
    if ((omask >> olane) & 1) {
        const int32_t x = ob.x0 + (olane & 7), y = ob.y0 + (olane >> 3);
        const V3 d = camera_ray_dir(P.cam, x, y);
        float t = kMaxFloat;
        int32_t material = 0;
        uint32_t ident = kDenoiseEmpty;
        V3 n = mk(0.f, 0.f, 0.f);
        if (ray_ok(eye, d)) {
            Isect id;
            scene_finish(S, eye, d, sh.best, sh.face, sh.fu, sh.fv, sh.nm, id);  // renderer.cpp:86-160
            t = id.t;
            material = id.material;
            if (id.type != T_SKY) {
                // (kind << 28) | (model + 1): ATR_RAY_TRI, _SPHERE, _PLANE are T_TRI, T_SPHERE, T_PLANE
                ident = (uint32_t(id.type) << 28) | (id.type == T_TRI ? uint32_t(sh.nm + 1) : 0u);
                n = id.normal;
            }
        }
        const V3 p = add(eye, scale(d, t));
        if (dot(neg(d), n) < 0) n = neg(n);  // bounce_shade's convention (scan.h)
        const size_t o = size_t(y) * size_t(P.cam.width) + size_t(x);
        if (P.normal) { P.normal[3 * o] = n.x; P.normal[3 * o + 1] = n.y; P.normal[3 * o + 2] = n.z; }
        if (P.position) { P.position[3 * o] = p.x; P.position[3 * o + 1] = p.y; P.position[3 * o + 2] = p.z; }
        if (P.ident) P.ident[o] = ident;
        if (P.depth) P.depth[o] = t;
        if (P.material) P.material[o] = material;
    }
    if (err && P.error_flag) atomicOr(P.error_flag, 1);
}

__global__ __launch_bounds__(256) void camera_rays_kernel(CameraRaysParams P) {
    const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= P.n) return;
    const int64_t pix = P.first + i;
    const V3 d = camera_ray_dir(P.cam, int32_t(pix % P.cam.width), int32_t(pix / P.cam.width));
    P.o[3 * i] = P.cam.eye.x; P.o[3 * i + 1] = P.cam.eye.y; P.o[3 * i + 2] = P.cam.eye.z;
    P.d[3 * i] = d.x; P.d[3 * i + 1] = d.y; P.d[3 * i + 2] = d.z;
}

}  // namespace atr

// One wavefront per block, four per workgroup.
extern "C" hipError_t atr_launch_camera_guides(const atr::GuidesParams& P, hipStream_t s) {
    if (P.nblocks <= 0) return hipSuccess;
    hipLaunchKernelGGL(atr::camera_guides_kernel, dim3(unsigned((P.nblocks + 3) / 4)), dim3(256), 0, s, P);
    return hipGetLastError();
}

extern "C" hipError_t atr_launch_camera_rays(const atr::CameraRaysParams& P, hipStream_t s) {
    if (P.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(atr::camera_rays_kernel, dim3(unsigned((P.n + 255) / 256)), dim3(256), 0, s, P);
    return hipGetLastError();
}
