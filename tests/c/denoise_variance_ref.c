/* denoise_variance_ref.c -- atr_denoise_variance's contract (include/atray.h) as a plain loop, for the
   tests: gcc, -O2 -ffp-contract=off -fno-fast-math, OpenMP over rows. Every f32 operation is separately
   rounded. With -DDENOISE_VARIANCE_REF_MAIN a small main runs the edge sizes, every guide subset, the
   estimate on and off and in-place calls (built with the address and undefined sanitizers by
   tests/test_denoise_variance_sanitize.py). */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define EMPTY 0xFFFFFFFFu

static float dot3(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
static int finite3(const float* a) { return isfinite(a[0]) && isfinite(a[1]) && isfinite(a[2]); }
static float lum(const float* c) { return (0.2126f * c[0] + 0.7152f * c[1]) + 0.0722f * c[2]; }
static float pl_max(float a, float b) { return a > b ? a : b; }
static float pl_min(float a, float b) { return a > b ? b : a; }
static uint32_t quant(float c) {
    const float k = pl_max(0.0f, pl_min(c, 1.0f));
    return k == k ? ((uint32_t)(k * 255.0f) & 0xFFu) : 0u;
}

/* atr_denoise's normal and position terms of the tap q seen from the pixel t */
static float normal_term(const float* normal, size_t t, size_t q, int32_t power) {
    float c = dot3(normal + 3 * t, normal + 3 * q);
    c = c > 0.0f ? c : 0.0f;
    for (int32_t k = 0; k < power; ++k) c = c * c;
    return c;
}
static float position_term(const float* normal, const float* position, size_t t, size_t q, float kp) {
    float dv[3], e2;
    for (int ch = 0; ch < 3; ++ch) dv[ch] = position[3 * q + ch] - position[3 * t + ch];
    if (normal) {
        const float e = dot3(normal + 3 * t, dv);
        e2 = e * e;
    } else {
        e2 = dot3(dv, dv);
    }
    return 1.0f / (1.0f + e2 * kp);
}

/* The per-pass position constants; 0 = ok, -1 = the call is ATR_E_INVALID by the kp rule. */
int ref_denoise_variance_constants(int32_t passes, float sigma_position, int position_given, float* kp) {
    const int pon = position_given && sigma_position > 0.0f;
    for (int32_t p = 0; p < passes; ++p) {
        const float sp = sigma_position * (float)(1 << p);
        kp[p] = pon ? 1.0f / (sp * sp) : 0.0f;
        if (pon && !(isfinite(kp[p]) && kp[p] > 0.0f)) return -1;
    }
    return 0;
}

/* color, normal, position: 3 floats per pixel; variance: one; ident, length: one u32; moments: two
   floats. normal, position, ident, moments and length (both or neither), out, variance_out and
   framebuffer may be NULL; out may be color and variance_out may be variance. Returns 0, or -1 for the
   kp rule or a pass count outside 1..8 (nothing written). */
int ref_denoise_variance(const float* color, const float* variance, const float* normal, const float* position,
                         const uint32_t* ident, const float* moments, const uint32_t* length, int32_t width,
                         int32_t height, int32_t passes, float sigma_luminance, float luminance_floor,
                         float sigma_position, int32_t normal_power_log2, int32_t spatial_below, float* out,
                         float* variance_out, uint32_t* framebuffer) {
    static const float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    static const float g[3] = {0.25f, 0.5f, 0.25f};
    float kps[8];
    if (passes < 1 || passes > 8) return -1;
    if (ref_denoise_variance_constants(passes, sigma_position, position != NULL, kps)) return -1;
    const size_t n = (size_t)width * (size_t)height;
    const int luminance_on = sigma_luminance > 0.0f, position_on = position && sigma_position > 0.0f;
    uint8_t* inert = (uint8_t*)malloc(n);
    float* cur = (float*)malloc(3 * n * sizeof(float));
    float* nxt = (float*)malloc(3 * n * sizeof(float));
    float* vcur = (float*)malloc(n * sizeof(float));
    float* vnxt = (float*)malloc(n * sizeof(float));
    memcpy(cur, color, 3 * n * sizeof(float));
    for (size_t t = 0; t < n; ++t) {
        inert[t] = (ident && ident[t] == EMPTY) || !finite3(color + 3 * t) || (normal && !finite3(normal + 3 * t)) ||
                   (position && !finite3(position + 3 * t));
        const float v = variance[t];
        vcur[t] = (!inert[t] && v > 0.0f && v < INFINITY) ? v : 0.0f;
    }
    if (moments && length && spatial_below > 0) {
        const float kp = kps[0];
#pragma omp parallel for schedule(static)
        for (int32_t y = 0; y < height; ++y)
            for (int32_t x = 0; x < width; ++x) {
                const size_t t = (size_t)y * (size_t)width + (size_t)x;
                if (inert[t] || !(length[t] < (uint32_t)spatial_below)) continue;
                float a = 0.0f, b = 0.0f, ws = 0.0f;
                for (int dy = -3; dy <= 3; ++dy)
                    for (int dx = -3; dx <= 3; ++dx) {
                        const int32_t qx = x + dx, qy = y + dy;
                        if (qx < 0 || qy < 0 || qx >= width || qy >= height) continue;
                        const size_t q = (size_t)qy * (size_t)width + (size_t)qx;
                        if (inert[q] || (ident && ident[q] != ident[t])) continue;
                        const float* m = moments + 2 * q;
                        if (!(isfinite(m[0]) && isfinite(m[1]))) continue;
                        float w = 1.0f;
                        if (normal) w = w * normal_term(normal, t, q, normal_power_log2);
                        if (position_on) w = w * position_term(normal, position, t, q, kp);
                        if (!(w > 0.0f)) continue;
                        a = a + m[0] * w;
                        b = b + m[1] * w;
                        ws = ws + w;
                    }
                if (ws > 0.0f) {
                    const float m1 = a / ws, m2 = b / ws;
                    float e = m2 - m1 * m1;
                    e = e > 0.0f ? e : 0.0f;
                    const uint32_t lp = length[t] > 0u ? length[t] : 1u;
                    vcur[t] = e * ((float)spatial_below / (float)lp);
                }
            }
    }
    for (int32_t p = 0; p < passes; ++p) {
        const int32_t s = 1 << p;
        const float kp = kps[p];
#pragma omp parallel for schedule(static)
        for (int32_t y = 0; y < height; ++y)
            for (int32_t x = 0; x < width; ++x) {
                const size_t t = (size_t)y * (size_t)width + (size_t)x;
                const float* cp = cur + 3 * t;
                float* r = nxt + 3 * t;
                memcpy(r, cp, 3 * sizeof(float));
                vnxt[t] = vcur[t];
                if (inert[t]) continue;
                float rl = 0.0f;
                if (luminance_on) {
                    float gs = 0.0f, ks = 0.0f;
                    for (int dy = -1; dy <= 1; ++dy)
                        for (int dx = -1; dx <= 1; ++dx) {
                            const int32_t qx = x + dx, qy = y + dy;
                            if (qx < 0 || qy < 0 || qx >= width || qy >= height) continue;
                            const size_t q = (size_t)qy * (size_t)width + (size_t)qx;
                            if (inert[q] || (ident && ident[q] != ident[t])) continue;
                            const float k = g[dy + 1] * g[dx + 1];
                            gs = gs + vcur[q] * k;
                            ks = ks + k;
                        }
                    const float gv = gs / ks;
                    rl = 1.0f / (sigma_luminance * sqrtf(gv) + luminance_floor);
                }
                const float lp = lum(cp);
                float sum[3] = {0.0f, 0.0f, 0.0f}, vs = 0.0f, wsum = 0.0f;
                for (int dy = -2; dy <= 2; ++dy)
                    for (int dx = -2; dx <= 2; ++dx) {
                        const int32_t qx = x + dx * s, qy = y + dy * s;
                        if (qx < 0 || qy < 0 || qx >= width || qy >= height) continue;
                        const size_t q = (size_t)qy * (size_t)width + (size_t)qx;
                        if (inert[q] || (ident && ident[q] != ident[t])) continue;
                        const float* cq = cur + 3 * q;
                        float w = h[dy + 2] * h[dx + 2];
                        if (normal) w = w * normal_term(normal, t, q, normal_power_log2);
                        if (position_on) w = w * position_term(normal, position, t, q, kp);
                        if (luminance_on) {
                            const float xl = fabsf(lum(cq) - lp) * rl;
                            w = w * (1.0f / (1.0f + xl));
                        }
                        if (!(w > 0.0f)) continue;
                        for (int ch = 0; ch < 3; ++ch) sum[ch] = sum[ch] + cq[ch] * w;
                        vs = vs + vcur[q] * (w * w);
                        wsum = wsum + w;
                    }
                if (wsum > 0.0f) {
                    for (int ch = 0; ch < 3; ++ch) r[ch] = sum[ch] / wsum;
                    vnxt[t] = vs / (wsum * wsum);
                }
            }
        float* tf = cur; cur = nxt; nxt = tf;
        tf = vcur; vcur = vnxt; vnxt = tf;
    }
    if (out) memcpy(out, cur, 3 * n * sizeof(float));
    if (variance_out) memcpy(variance_out, vcur, n * sizeof(float));
    if (framebuffer)
        for (size_t t = 0; t < n; ++t)
            framebuffer[t] = quant(cur[3 * t + 2]) | (quant(cur[3 * t + 1]) << 8) | (quant(cur[3 * t]) << 16);
    free(inert), free(cur), free(nxt), free(vcur), free(vnxt);
    return 0;
}

#ifdef DENOISE_VARIANCE_REF_MAIN
#include <stdio.h>

/* The edge sizes, every guide subset, both terms and the estimate on and off, 8 passes, separate and in
   place; NaN, inf and EMPTY planted in the inputs, NaN, inf and negative values in the variance and the
   moments, lengths on both sides of spatial_below. */
int main(void) {
    static const int32_t sizes[][2] = {{1, 1}, {1, 7}, {7, 1}, {5, 5}, {63, 3}, {64, 4}, {65, 5}, {130, 67}, {3, 3}};
    uint32_t state = 12345u, check = 0u;
    for (size_t k = 0; k < sizeof(sizes) / sizeof(sizes[0]); ++k) {
        const int32_t w = sizes[k][0], hgt = sizes[k][1];
        const size_t n = (size_t)w * (size_t)hgt;
        float* buf = (float*)malloc(16 * n * sizeof(float)); /* colour, normal, position, variance, moments, out, vout */
        uint32_t* id = (uint32_t*)malloc(n * sizeof(uint32_t));
        uint32_t* len = (uint32_t*)malloc(n * sizeof(uint32_t));
        uint32_t* fb = (uint32_t*)malloc(n * sizeof(uint32_t));
        float* var = buf + 9 * n;
        float* mom = buf + 10 * n;
        float* o = buf + 12 * n;
        float* vo = buf + 15 * n;
        for (int g = 0; g < 8; ++g)
            for (int sg = 0; sg < 8; ++sg) {
                for (size_t i = 0; i < 12 * n; ++i) {
                    state = state * 1664525u + 1013904223u;
                    buf[i] = (float)(state >> 8) * (1.0f / 16777216.0f);
                }
                for (size_t i = 0; i < n; ++i) id[i] = (uint32_t)(i % 3 == 0 ? 1 : 2), len[i] = (uint32_t)(i % 7);
                if (n > 4) {
                    buf[3] = NAN, buf[3 * n + 7] = INFINITY, buf[6 * n + 11] = -INFINITY;
                    id[n - 1] = EMPTY;
                    var[0] = NAN, var[2] = -1.0f, var[3] = INFINITY, mom[4] = NAN, mom[7] = INFINITY;
                }
                const int in_place = sg & 4;
                if (ref_denoise_variance(buf, var, g & 1 ? buf + 3 * n : NULL, g & 2 ? buf + 6 * n : NULL, g & 4 ? id : NULL,
                                         sg & 2 ? mom : NULL, sg & 2 ? len : NULL, w, hgt, (g + sg) % 8 + 1,
                                         sg & 1 ? 2.0f : 0.0f, 0.001f, g & 1 ? 0.5f : 0.0f, 3, 4, in_place ? buf : o,
                                         in_place ? var : (g & 1 ? vo : NULL), fb))
                    return 1;
                for (size_t i = 0; i < n; ++i) check = check * 31u + fb[i];
            }
        free(buf), free(id), free(len), free(fb);
    }
    printf("denoise_variance_ref ok %08x\n", (unsigned)check);
    return 0;
}
#endif
