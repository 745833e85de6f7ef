/* denoise_ref.c -- atr_denoise's contract (include/atray.h) as a plain loop, for the tests: gcc, -O2
   -ffp-contract=off -fno-fast-math, OpenMP over rows. Every f32 operation is separately rounded.
   With -DDENOISE_REF_MAIN a small main runs the edge sizes (built with the address and undefined
   sanitizers by tests/test_denoise_cpu.py). */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define EMPTY 0xFFFFFFFFu

static float dot3(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
static int finite3(const float* a) { return isfinite(a[0]) && isfinite(a[1]) && isfinite(a[2]); }
static float pl_max(float a, float b) { return a > b ? a : b; }
static float pl_min(float a, float b) { return a > b ? b : a; }
static uint32_t quant(float c) {
    const float k = pl_max(0.0f, pl_min(c, 1.0f));
    return k == k ? ((uint32_t)(k * 255.0f) & 0xFFu) : 0u;
}

/* The per-pass constants; 0 = ok, -1 = the call is ATR_E_INVALID by the kc/kp rule. */
int ref_denoise_constants(int32_t passes, float sigma_color, float sigma_position, int position_given, float* kc,
                          float* kp) {
    for (int32_t p = 0; p < passes; ++p) {
        const float s = (float)(1 << p);
        const float sc = sigma_color / s, sp = sigma_position * s;
        const int con = sigma_color > 0.0f, pon = position_given && sigma_position > 0.0f;
        kc[p] = con ? 1.0f / (sc * sc) : 0.0f;
        kp[p] = pon ? 1.0f / (sp * sp) : 0.0f;
        if (con && !(isfinite(kc[p]) && kc[p] > 0.0f)) return -1;
        if (pon && !(isfinite(kp[p]) && kp[p] > 0.0f)) return -1;
    }
    return 0;
}

/* color, normal, position: 3 floats per pixel; ident: one u32; normal, position, ident, out and
   framebuffer may be NULL. Returns 0, or -1 for the kc/kp rule (nothing written). */
int ref_denoise(const float* color, const float* normal, const float* position, const uint32_t* ident, int32_t width,
                int32_t height, int32_t passes, float sigma_color, float sigma_position, int32_t normal_power_log2,
                float* out, uint32_t* framebuffer) {
    static const float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    float kcs[32], kps[32];
    if (passes < 1 || passes > 8) return -1;
    if (ref_denoise_constants(passes, sigma_color, sigma_position, position != NULL, kcs, kps)) return -1;
    const size_t n = (size_t)width * (size_t)height;
    const int colour_on = sigma_color > 0.0f, position_on = position && sigma_position > 0.0f;
    uint8_t* inert = (uint8_t*)malloc(n);
    float* cur = (float*)malloc(3 * n * sizeof(float));
    float* nxt = (float*)malloc(3 * n * sizeof(float));
    memcpy(cur, color, 3 * n * sizeof(float));
    for (size_t t = 0; t < n; ++t)
        inert[t] = (ident && ident[t] == EMPTY) || !finite3(color + 3 * t) || (normal && !finite3(normal + 3 * t)) ||
                   (position && !finite3(position + 3 * t));
    for (int32_t p = 0; p < passes; ++p) {
        const int32_t s = 1 << p;
        const float kc = kcs[p], kp = kps[p];
#pragma omp parallel for schedule(static)
        for (int32_t y = 0; y < height; ++y)
            for (int32_t x = 0; x < width; ++x) {
                const size_t t = (size_t)y * (size_t)width + (size_t)x;
                const float* cp = cur + 3 * t;
                float* r = nxt + 3 * t;
                memcpy(r, cp, 3 * sizeof(float));
                if (inert[t]) continue;
                float sum[3] = {0.0f, 0.0f, 0.0f}, wsum = 0.0f;
                for (int dy = -2; dy <= 2; ++dy)
                    for (int dx = -2; dx <= 2; ++dx) {
                        const int32_t qx = x + dx * s, qy = y + dy * s;
                        if (qx < 0 || qy < 0 || qx >= width || qy >= height) continue;
                        const size_t q = (size_t)qy * (size_t)width + (size_t)qx;
                        if (inert[q] || (ident && ident[q] != ident[t])) continue;
                        const float* cq = cur + 3 * q;
                        float w = h[dy + 2] * h[dx + 2];
                        if (normal) {
                            float c = dot3(normal + 3 * t, normal + 3 * q);
                            c = c > 0.0f ? c : 0.0f;
                            for (int32_t k = 0; k < normal_power_log2; ++k) c = c * c;
                            w = w * c;
                        }
                        if (position_on) {
                            float dv[3], e2;
                            for (int ch = 0; ch < 3; ++ch) dv[ch] = position[3 * q + ch] - position[3 * t + ch];
                            if (normal) {
                                const float e = dot3(normal + 3 * t, dv);
                                e2 = e * e;
                            } else {
                                e2 = dot3(dv, dv);
                            }
                            w = w * (1.0f / (1.0f + e2 * kp));
                        }
                        if (colour_on) {
                            float dc[3];
                            for (int ch = 0; ch < 3; ++ch) dc[ch] = cq[ch] - cp[ch];
                            const float d2 = dot3(dc, dc);
                            w = w * (1.0f / (1.0f + d2 * kc));
                        }
                        if (!(w > 0.0f)) continue;
                        for (int ch = 0; ch < 3; ++ch) sum[ch] = sum[ch] + cq[ch] * w;
                        wsum = wsum + w;
                    }
                if (wsum > 0.0f)
                    for (int ch = 0; ch < 3; ++ch) r[ch] = sum[ch] / wsum;
            }
        float* tf = cur; cur = nxt; nxt = tf;
    }
    if (out) memcpy(out, cur, 3 * n * sizeof(float));
    if (framebuffer)
        for (size_t t = 0; t < n; ++t)
            framebuffer[t] = quant(cur[3 * t + 2]) | (quant(cur[3 * t + 1]) << 8) | (quant(cur[3 * t]) << 16);
    free(inert), free(cur), free(nxt);
    return 0;
}

#ifdef DENOISE_REF_MAIN
#include <stdio.h>

/* The edge sizes, every guide subset, both terms on and off, 8 passes; NaN, inf and EMPTY planted. */
int main(void) {
    static const int32_t sizes[][2] = {{1, 1}, {1, 7}, {7, 1}, {5, 5}, {63, 3}, {64, 4}, {65, 5}, {130, 67}, {3, 3}};
    uint32_t state = 12345u, check = 0u;
    for (size_t k = 0; k < sizeof(sizes) / sizeof(sizes[0]); ++k) {
        const int32_t w = sizes[k][0], hgt = sizes[k][1];
        const size_t n = (size_t)w * (size_t)hgt;
        float* buf = (float*)malloc(12 * n * sizeof(float));
        uint32_t* id = (uint32_t*)malloc(n * sizeof(uint32_t));
        uint32_t* fb = (uint32_t*)malloc(n * sizeof(uint32_t));
        for (size_t i = 0; i < 9 * n; ++i) {
            state = state * 1664525u + 1013904223u;
            buf[i] = (float)(state >> 8) * (1.0f / 16777216.0f);
        }
        for (size_t i = 0; i < n; ++i) id[i] = (uint32_t)(i % 3 == 0 ? 1 : 2);
        if (n > 4) {
            buf[3] = NAN, buf[3 * n + 7] = INFINITY, buf[6 * n + 11] = -INFINITY;
            id[n - 1] = EMPTY;
        }
        for (int g = 0; g < 8; ++g)
            for (int sg = 0; sg < 4; ++sg) {
                if (ref_denoise(buf, g & 1 ? buf + 3 * n : NULL, g & 2 ? buf + 6 * n : NULL, g & 4 ? id : NULL, w, hgt,
                                8, sg & 1 ? 1.0f : 0.0f, sg & 2 ? 0.5f : 0.0f, 3, buf + 9 * n, fb))
                    return 1;
                for (size_t i = 0; i < n; ++i) check = check * 31u + fb[i];
            }
        free(buf), free(id), free(fb);
    }
    printf("denoise_ref ok %08x\n", (unsigned)check);
    return 0;
}
#endif
