/* accumulate_ref.c -- atr_accumulate's contract (include/atray.h) as a plain loop, for the tests: gcc, -O2
   -ffp-contract=off -fno-fast-math, OpenMP over rows. Every f32 operation is separately rounded.
   With -DACCUMULATE_REF_MAIN a small main runs the edge sizes and every guide subset (built with the
   address and undefined sanitizers by tests/test_accumulate_sanitize.py). */
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

/* cam: the previous camera as 13 floats, eye, camera_x, camera_y, camera_z (3 each) and k = h_fov *
   aspect_ratio. has_prev 0 starts a history (cam and the prev_* pointers are not read). normal, ident
   (and prev_normal, prev_ident), the moments, variance and framebuffer may be NULL; position may be
   NULL without a previous frame. The caller has validated the arguments (atray.h). */
void ref_accumulate(const float* color, const float* normal, const float* position, const uint32_t* ident, int has_prev,
                    const float* cam, const float* prev_normal, const float* prev_position, const uint32_t* prev_ident,
                    const float* prev_color, const float* prev_moments, const uint32_t* prev_length, int32_t width,
                    int32_t height, float alpha, float alpha_moments, int32_t max_length, float plane_tolerance,
                    float min_normal_dot, float* out_color, float* out_moments, uint32_t* out_length, float* variance,
                    uint32_t* framebuffer) {
    const float hw = 0.5f * (float)width, hh = 0.5f * (float)height;
#pragma omp parallel for schedule(static)
    for (int32_t y = 0; y < height; ++y)
        for (int32_t x = 0; x < width; ++x) {
            const size_t t = (size_t)y * (size_t)width + (size_t)x;
            const float* c = color + 3 * t;
            const int inert = (ident && ident[t] == EMPTY) || !finite3(c) || (normal && !finite3(normal + 3 * t)) ||
                              (position && !finite3(position + 3 * t));
            float o[3] = {c[0], c[1], c[2]}, m1 = 0.0f, m2 = 0.0f, var = 0.0f;
            uint32_t len = 0u;
            if (!inert) {
                float sum[3] = {0.0f, 0.0f, 0.0f}, msum[2] = {0.0f, 0.0f}, wsum = 0.0f;
                uint32_t nmin = 0xFFFFFFFFu;
                while (has_prev) {  /* one round: `break` is "no history" */
                    const float* p = position + 3 * t;
                    const float* n = normal ? normal + 3 * t : NULL;
                    float v[3];
                    for (int ch = 0; ch < 3; ++ch) v[ch] = p[ch] - cam[ch];
                    const float depth = -dot3(v, cam + 9);
                    if (!(depth > 0.0f)) break;
                    const float a = dot3(v, cam + 3) / depth;
                    const float b = dot3(v, cam + 6) / depth;
                    const float sx = (a / cam[12] + 1.0f) * hw;
                    const float sy = (b + 1.0f) * hh;
                    if (!(sx >= -1.0f && sx < (float)width && sy >= -1.0f && sy < (float)height)) break;
                    const float fx0 = floorf(sx), fy0 = floorf(sy);
                    const int32_t x0 = (int32_t)fx0, y0 = (int32_t)fy0;
                    const float tx = sx - fx0, ty = sy - fy0;
                    const float tol = plane_tolerance * depth;
                    for (int dy = 0; dy < 2; ++dy)
                        for (int dx = 0; dx < 2; ++dx) {
                            const int32_t qx = x0 + dx, qy = y0 + dy;
                            if (qx < 0 || qy < 0 || qx >= width || qy >= height) continue;
                            const size_t q = (size_t)qy * (size_t)width + (size_t)qx;
                            if (prev_length[q] == 0u) continue;
                            if (ident && (prev_ident[q] != ident[t] || prev_ident[q] == EMPTY)) continue;
                            if (n && !(dot3(n, prev_normal + 3 * q) >= min_normal_dot)) continue;
                            float dv[3], e2;
                            for (int ch = 0; ch < 3; ++ch) dv[ch] = prev_position[3 * q + ch] - p[ch];
                            if (n) {
                                const float e = dot3(n, dv);
                                e2 = e * e;
                            } else {
                                e2 = dot3(dv, dv);
                            }
                            if (!(e2 <= tol * tol)) continue;
                            const float* hc = prev_color + 3 * q;
                            if (!finite3(hc)) continue;
                            if (out_moments && !(isfinite(prev_moments[2 * q]) && isfinite(prev_moments[2 * q + 1]))) continue;
                            const float w = (dx ? tx : 1.0f - tx) * (dy ? ty : 1.0f - ty);
                            if (!(w > 0.0f)) continue;
                            for (int ch = 0; ch < 3; ++ch) sum[ch] = sum[ch] + hc[ch] * w;
                            if (out_moments)
                                for (int ch = 0; ch < 2; ++ch) msum[ch] = msum[ch] + prev_moments[2 * q + ch] * w;
                            wsum = wsum + w;
                            nmin = prev_length[q] < nmin ? prev_length[q] : nmin;
                        }
                    break;
                }
                const float l = (0.2126f * c[0] + 0.7152f * c[1]) + 0.0722f * c[2];
                if (wsum > 0.0f) {
                    const uint32_t cap = (uint32_t)max_length - 1u;
                    len = (nmin < cap ? nmin : cap) + 1u;
                    const float aw = 1.0f / (float)len;
                    const float ac = alpha > aw ? alpha : aw, am = alpha_moments > aw ? alpha_moments : aw;
                    for (int ch = 0; ch < 3; ++ch) {
                        const float h = sum[ch] / wsum;
                        o[ch] = h + (c[ch] - h) * ac;
                    }
                    const float hm0 = msum[0] / wsum, hm1 = msum[1] / wsum;
                    m1 = hm0 + (l - hm0) * am;
                    m2 = hm1 + (l * l - hm1) * am;
                } else {
                    len = 1u;
                    m1 = l;
                    m2 = l * l;
                }
                var = m2 - m1 * m1;
                var = var > 0.0f ? var : 0.0f;
            }
            memcpy(out_color + 3 * t, o, sizeof(o));
            out_length[t] = len;
            if (out_moments) out_moments[2 * t] = m1, out_moments[2 * t + 1] = m2;
            if (variance) variance[t] = var;
            if (framebuffer) framebuffer[t] = quant(o[2]) | (quant(o[1]) << 8) | (quant(o[0]) << 16);
        }
}

#ifdef ACCUMULATE_REF_MAIN
#include <stdio.h>

/* The edge sizes, every subset of {normal, ident, moments}, a chain of three frames through two
   ping-ponged histories, seen from a camera at the origin facing -z that steps sideways; NaN, inf and
   EMPTY planted. */
int main(void) {
    static const int32_t sizes[][2] = {{1, 1}, {1, 7}, {7, 1}, {5, 5}, {63, 3}, {64, 4}, {65, 5}, {130, 67}, {3, 3}};
    uint32_t state = 12345u, check = 0u;
    for (size_t k = 0; k < sizeof(sizes) / sizeof(sizes[0]); ++k) {
        const int32_t w = sizes[k][0], hgt = sizes[k][1];
        const size_t n = (size_t)w * (size_t)hgt;
        float* col = (float*)malloc(3 * n * sizeof(float));
        float* nrm = (float*)malloc(3 * n * sizeof(float));
        float* pos = (float*)malloc(3 * n * sizeof(float));
        uint32_t* id = (uint32_t*)malloc(n * sizeof(uint32_t));
        float* hc[2] = {(float*)malloc(3 * n * sizeof(float)), (float*)malloc(3 * n * sizeof(float))};
        float* hm[2] = {(float*)malloc(2 * n * sizeof(float)), (float*)malloc(2 * n * sizeof(float))};
        uint32_t* hl[2] = {(uint32_t*)malloc(n * sizeof(uint32_t)), (uint32_t*)malloc(n * sizeof(uint32_t))};
        float* var = (float*)malloc(n * sizeof(float));
        uint32_t* fb = (uint32_t*)malloc(n * sizeof(uint32_t));
        /* the plane z = -2 seen through a film of k = 1: pixel (x, y) shows (2*fx, 2*fy, -2) */
        for (int32_t y = 0; y < hgt; ++y)
            for (int32_t x = 0; x < w; ++x) {
                const size_t t = (size_t)y * (size_t)w + (size_t)x;
                pos[3 * t] = 2.0f * (-1.0f + 2.0f * ((float)x / (float)w));
                pos[3 * t + 1] = 2.0f * (-1.0f + 2.0f * ((float)y / (float)hgt));
                pos[3 * t + 2] = -2.0f;
                nrm[3 * t] = 0.0f, nrm[3 * t + 1] = 0.0f, nrm[3 * t + 2] = 1.0f;
                id[t] = (uint32_t)(x % 5 == 4 ? 2 : 1);
            }
        for (int g = 0; g < 8; ++g) {
            float cam[13] = {0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 1.0f};
            for (int f = 0; f < 3; ++f) {
                for (size_t i = 0; i < 3 * n; ++i) {
                    state = state * 1664525u + 1013904223u;
                    col[i] = (float)(state >> 8) * (1.0f / 16777216.0f);
                }
                if (n > 4) col[3] = NAN, col[3 * n - 1] = INFINITY;
                const int cur = f & 1, old = cur ^ 1;
                if (f == 1 && n > 4) hc[old][7] = NAN, hm[old][5] = -INFINITY, hl[old][n - 2] = 0u;
                ref_accumulate(col, g & 1 ? nrm : NULL, pos, g & 2 ? id : NULL, f > 0, cam, g & 1 ? nrm : NULL, pos,
                               g & 2 ? id : NULL, hc[old], g & 4 ? hm[old] : NULL, hl[old], w, hgt, 0.0f, 0.0f, 2, 0.02f,
                               0.9f, hc[cur], g & 4 ? hm[cur] : NULL, hl[cur], g & 4 ? var : NULL, fb);
                for (size_t i = 0; i < n; ++i) check = check * 31u + fb[i] + hl[cur][i];
                cam[0] = cam[0] + 0.37f;  /* the next frame reprojects between pixels, and off the film */
                cam[1] = cam[1] - 0.11f;
            }
        }
        free(col), free(nrm), free(pos), free(id), free(var), free(fb);
        for (int i = 0; i < 2; ++i) free(hc[i]), free(hm[i]), free(hl[i]);
    }
    printf("accumulate_ref ok %08x\n", (unsigned)check);
    return 0;
}
#endif
