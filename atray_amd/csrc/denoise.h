// denoise.h -- the edge-avoiding a-trous filter (atr_denoise; denoise.hip): the kernels'
// arguments and the renderer's quantisation of a colour into a BGRX pixel. tests/c/denoise_ref.c
// restates the filter in plain C.
#pragma once
#include "engine.h"

namespace atr {

constexpr int32_t kDenoiseMaxSide = 16384;  // width, height: 1..16,384
constexpr int32_t kDenoiseMaxPasses = 8;    // tap spacing 2^p: at most 128 pixels
constexpr int32_t kDenoiseMaxNormalPower = 7;
constexpr uint32_t kDenoiseEmpty = 0xFFFFFFFFu;  // ATR_DENOISE_EMPTY
constexpr int kDenoiseBlockX = 64;          // pass kernel: one wave per row segment of 64 pixels,
constexpr int kDenoiseBlockY = 4;           // four rows per block

// The workspace's records, 16 B each per pixel. colour: {r, g, b, id bits}, where id is the pixel's
// ident (0 without one) and kDenoiseEmpty for an inert pixel: a pixel that is not inert never has that
// id, so "Q is inert or of another id" is the one comparison id_Q != id_P. normal, position: {x, y, z, 0},
// present only when the caller gave the guide.
struct DenoisePack {
    const float* color;
    const float* normal;      // may be NULL
    const float* position;    // may be NULL
    const uint32_t* ident;    // may be NULL
    int64_t npixels;
    float4_t* color4;
    float4_t* normal4;        // NULL iff normal is
    float4_t* position4;      // NULL iff position is
};

struct DenoisePass {
    int32_t width, height;
    int32_t step;             // s = 2^p
    int32_t normal_power;     // normal_power_log2
    float kc, kp;             // 1 / (sigma_color / s)^2, 1 / (sigma_position * s)^2 (host, f32)
    const float4_t* src;      // colour records at the start of the pass
    const float4_t* normal4;
    const float4_t* position4;
    float4_t* dst;            // colour records of the next pass, or NULL: the last pass, which writes
    float* out;               //   the caller's image (may be NULL) and
    uint32_t* framebuffer;    //   framebuffer (may be NULL)
};

// The resolve's clamp and quantisation (paths.hip path_resolve), one channel; a NaN gives 0.
ATR_HD uint32_t denoise_quant(float c) {
    const float k = pl_max(0.0f, pl_min(c, 1.0f));
    return k == k ? (uint32_t(k * 255.0f) & 0xFFu) : 0u;
}
ATR_HD uint32_t denoise_bgrx(float r, float g, float b) {
    return denoise_quant(b) | (denoise_quant(g) << 8) | (denoise_quant(r) << 16);
}

}  // namespace atr
