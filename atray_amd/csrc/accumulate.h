// accumulate.h -- temporal accumulation (atr_accumulate; accumulate.hip): the kernel's
// arguments. tests/c/accumulate_ref.c restates the kernel in plain C.
#pragma once
#include "denoise.h"

namespace atr {

constexpr int32_t kAccumulateMaxLength = 1 << 24;  // max_length: 1..2^24, so float(length) is exact
constexpr int kAccumulateBlockX = 64;              // one wave per row segment of 64 pixels,
constexpr int kAccumulateBlockY = 4;               // four rows per block

struct AccumulateParams {
    int32_t width, height;
    int32_t has_prev;             // 0: start a history (the prev_* pointers are not read)
    uint32_t max_length;
    float alpha, alpha_moments;
    float plane_tolerance, min_normal_dot;
    float eye[3], cx[3], cy[3], cz[3];  // the previous camera's eye, camera_x, camera_y, camera_z
    float k, hw, hh, fw, fh;      // h_fov * aspect_ratio, 0.5f * float(width), 0.5f * float(height), float(width), float(height)
    const float* color;           // this frame
    const float* normal;          // NULL iff the kernel's NORMAL is false
    const float* position;        // may be NULL without a previous frame
    const uint32_t* ident;        // NULL iff IDENT is false
    const float* prev_normal;     // the previous frame's guides and history
    const float* prev_position;
    const uint32_t* prev_ident;
    const float* prev_color;
    const float* prev_moments;
    const uint32_t* prev_length;
    float* out_color;
    float* out_moments;           // NULL iff MOMENTS is false
    uint32_t* out_length;
    float* variance;              // may be NULL
    uint32_t* framebuffer;        // may be NULL
};

}  // namespace atr
