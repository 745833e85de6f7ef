// denoise_variance.h -- the variance-guided a-trous filter (atr_denoise_variance; denoise_variance.hip,
// DESIGN.md §4u): the kernels' arguments. tests/c/denoise_variance_ref.c restates the filter in plain C.
// The limits, the inert id, the block shape and the framebuffer's quantisation are denoise.h's.
#pragma once
#include "denoise.h"

namespace atr {

constexpr int32_t kDenoiseVarMaxSpatialBelow = 1 << 24;  // spatial_below: 0..2^24, exact as an f32

// The workspace's records per pixel. colour (16 B): {r, g, b, id bits} as in denoise.h, id = kDenoiseEmpty
// for an inert pixel. vl (8 B): {the variance of the luminance, lum(r, g, b)}; the luminance is stored
// because it has the same bits as recomputing it from the record would give. normal, position (16 B
// each): {x, y, z, 0}, present only when the caller gave the guide.
struct DenoiseVarPack {
    const float* color;
    const float* variance;
    const float* normal;      // may be NULL
    const float* position;    // may be NULL
    const uint32_t* ident;    // may be NULL
    int64_t npixels;
    float4_t* color4;
    float2_t* vl;
    float4_t* normal4;        // NULL iff normal is
    float4_t* position4;      // NULL iff position is
};

// The spatial estimate: the 7 x 7 window over the caller's moments, for live pixels of length < below.
struct DenoiseVarEstimate {
    int32_t width, height;
    int32_t normal_power;     // normal_power_log2
    uint32_t below;           // spatial_below, > 0
    float kp;                 // pass 0's position constant
    float fbelow;             // float(spatial_below)
    const float4_t* color4;   // for the ids only
    const float4_t* normal4;
    const float4_t* position4;
    const float2_t* moments;  // the caller's
    const uint32_t* length;   // the caller's
    float2_t* vl;             // .x of the pixel's own record is replaced
};

struct DenoiseVarPass {
    int32_t width, height;
    int32_t step;             // s = 2^p
    int32_t normal_power;     // normal_power_log2
    float kp;                 // 1 / (sigma_position * s)^2 (host, f32)
    float sigma_luminance, luminance_floor;
    const float4_t* src;      // colour records at the start of the pass
    const float2_t* src_vl;   // variance and luminance at the start of the pass
    const float4_t* normal4;
    const float4_t* position4;
    float4_t* dst;            // the next pass's records, or both NULL: the last pass, which writes the
    float2_t* dst_vl;         //   caller's
    float* out;               //   image (may be NULL),
    float* variance_out;      //   variance (may be NULL) and
    uint32_t* framebuffer;    //   framebuffer (may be NULL)
};

}  // namespace atr
