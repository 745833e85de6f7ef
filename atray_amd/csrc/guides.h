// guides.h -- a camera's primary rays and the denoiser's guides made from them (atr_camera_rays,
// atr_camera_rays_host, atr_camera_guides; guides.hip): the one function every one of
// them builds a pixel's ray with, and the kernels' arguments.
#pragma once
#include "engine.h"

namespace atr {

// The ray render_kernel casts through pixel (x, y) without anti-aliasing (render.hip; renderer.cpp
// :317, :329, :350-351): its direction, from the pixel's centre. Host and device evaluate the same
// separately rounded f32 operations in the same order.
ATR_HD V3 camera_ray_dir(const atr_camera& cm, int32_t x, int32_t y) {
    const float film_y = -1.0f + 2.0f * (float(y) / float(cm.height));
    const float film_x = ((-1.0f + 2.0f * (float(x) / float(cm.width))) * cm.h_fov) * cm.aspect_ratio;
    const V3 eye = from(cm.eye), fc = from(cm.frame_center), cx = from(cm.camera_x), cy = from(cm.camera_y);
    return unit(sub(add(add(fc, scale(cx, film_x)), scale(cy, film_y)), eye));
}

// atr_camera_rays: pixels [first, first + n) in pixel order, 3 floats each.
struct CameraRaysParams {
    atr_camera cam;
    int64_t first, n;
    float* o;
    float* d;
};

// atr_camera_guides: one wavefront per cell of the tile list's block list, as a render. Every output
// is in IMAGE layout and may be null.
struct GuidesParams {
    atr_camera cam;
    const DScene* scene;
    const DBlock* blocks;
    int32_t nblocks;
    int32_t xcd_chunk;
    int32_t hyb_a, hyb_b;
    float* normal;      // 3 per pixel
    float* position;    // 3 per pixel
    uint32_t* ident;
    float* depth;
    int32_t* material;
    int32_t* error_flag;
};

}  // namespace atr
