/* texel_ref.c -- the plain C reference of atr_mesh_texels and atr_texels_to_image (include/atray.h):
   a loop over the faces in ascending order and over all texels, every f32 operation separately
   rounded (built with -ffp-contract=off -fno-fast-math). No box, no list, no scan: the rule alone.
   Rows of texels are independent, so the loop over rows may run on several threads (OpenMP); the
   result does not depend on it. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct { float x, y; } uv_t;
typedef struct { float x, y, z; } v3_t;

static v3_t mk(float x, float y, float z) { v3_t r = {x, y, z}; return r; }
static v3_t add(v3_t a, v3_t b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
static v3_t sub(v3_t a, v3_t b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
static v3_t scale(v3_t a, float s) { return mk(a.x * s, a.y * s, a.z * s); }
static v3_t cross(v3_t a, v3_t b) { return mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
static v3_t unit(v3_t v) {
    const float l2 = (v.x * v.x) + (v.y * v.y) + (v.z * v.z);
    const float inv = 1.0f / sqrtf(l2);
    return scale(v, inv);
}
static v3_t fetch(const float* a, uint32_t n, int32_t i) {
    return (i >= 0 && (uint32_t)i < n) ? mk(a[3 * (size_t)i], a[3 * (size_t)i + 1], a[3 * (size_t)i + 2]) : mk(0.f, 0.f, 0.f);
}

static float edge(uv_t p0, uv_t p1, uv_t p) {
    float s = 1.0f;
    if (p1.x < p0.x || (p1.x == p0.x && p1.y < p0.y)) {
        const uv_t t = p0;
        p0 = p1;
        p1 = t;
        s = -1.0f;
    }
    return s * ((p1.x - p0.x) * (p.y - p0.y) - (p1.y - p0.y) * (p.x - p0.x));
}

typedef struct { uv_t a, b, c; float g; int usable; } face_t;

static int finite6(const face_t* F) {
    return isfinite(F->a.x) && isfinite(F->a.y) && isfinite(F->b.x) && isfinite(F->b.y) && isfinite(F->c.x) && isfinite(F->c.y);
}

static int covers(const face_t* F, uv_t p, float* e1, float* e2, float* den) {
    const float e0 = F->g * edge(F->b, F->c, p);
    *e1 = F->g * edge(F->c, F->a, p);
    *e2 = F->g * edge(F->a, F->b, p);
    *den = (e0 + *e1) + *e2;
    return e0 >= 0.0f && *e1 >= 0.0f && *e2 >= 0.0f && *den > 0.0f;
}

/* Outputs sized for width*height texels (the per-k ones too). Returns the covered count. */
int64_t ref_mesh_texels(const float* vertices, uint32_t nv, const float* normals, uint32_t nn, const float* texcoords,
                        uint32_t nt, const int32_t* face_v, const int32_t* face_t_, const int32_t* face_n, uint32_t nf,
                        int32_t width, int32_t height, int32_t flags, int32_t* slot, int32_t* texel, uint32_t* face,
                        float* bary, float* point, float* normal) {
    const size_t ntexels = (size_t)width * (size_t)height;
    face_t* F = (face_t*)calloc(nf ? nf : 1, sizeof(face_t));
    uint32_t* map = (uint32_t*)malloc(ntexels * sizeof(uint32_t));
    const float wf = (float)width, hf = (float)height;
    for (uint32_t f = 0; f < nf; ++f) {
        const int32_t* t = face_t_ + 3 * (size_t)f;
        face_t* X = &F[f];
        X->usable = t[0] >= 0 && t[1] >= 0 && t[2] >= 0 && (uint32_t)t[0] < nt && (uint32_t)t[1] < nt && (uint32_t)t[2] < nt;
        if (!X->usable) continue;
        X->a.x = texcoords[3 * (size_t)t[0]], X->a.y = texcoords[3 * (size_t)t[0] + 1];
        X->b.x = texcoords[3 * (size_t)t[1]], X->b.y = texcoords[3 * (size_t)t[1] + 1];
        X->c.x = texcoords[3 * (size_t)t[2]], X->c.y = texcoords[3 * (size_t)t[2] + 1];
        if (!(X->usable = finite6(X))) continue;
        const float area2 = (X->b.x - X->a.x) * (X->c.y - X->a.y) - (X->b.y - X->a.y) * (X->c.x - X->a.x);
        X->usable = area2 != 0.0f && !isnan(area2);
        X->g = area2 > 0.0f ? 1.0f : -1.0f;
    }
#pragma omp parallel for schedule(dynamic, 4)
    for (int32_t j = 0; j < height; ++j) {
        uint32_t* row = map + (size_t)j * (size_t)width;
        for (int32_t i = 0; i < width; ++i) row[i] = 0xFFFFFFFFu;
        for (uint32_t f = 0; f < nf; ++f) {
            if (!F[f].usable) continue;
            for (int32_t i = 0; i < width; ++i) {
                if (row[i] != 0xFFFFFFFFu) continue; /* a lower face has it */
                uv_t p;
                float e1, e2, den;
                p.x = ((float)i + 0.5f) / wf;
                p.y = ((float)j + 0.5f) / hf;
                if (covers(&F[f], p, &e1, &e2, &den)) row[i] = f;
            }
        }
    }
    const int smooth = nn > 0;
    int64_t k = 0;
    for (size_t t = 0; t < ntexels; ++t) {
        const uint32_t f = map[t];
        if (f == 0xFFFFFFFFu) {
            slot[t] = -1;
            continue;
        }
        slot[t] = (int32_t)k;
        texel[k] = (int32_t)t;
        face[k] = f;
        uv_t p;
        float e1, e2, den;
        p.x = ((float)(int32_t)(t % (size_t)width) + 0.5f) / wf;
        p.y = ((float)(int32_t)(t / (size_t)width) + 0.5f) / hf;
        (void)covers(&F[f], p, &e1, &e2, &den);
        const float u = e1 / den, v = e2 / den;
        bary[2 * k] = u, bary[2 * k + 1] = v;
        const int32_t* iv = face_v + 3 * (size_t)f;
        const v3_t A = fetch(vertices, nv, iv[0]), B = fetch(vertices, nv, iv[1]), Cc = fetch(vertices, nv, iv[2]);
        const v3_t pt = add(add(A, scale(sub(B, A), u)), scale(sub(Cc, A), v));
        point[3 * k] = pt.x, point[3 * k + 1] = pt.y, point[3 * k + 2] = pt.z;
        v3_t n;
        if (smooth) { /* the three vertex normals, interpolated */
            const int32_t* in = face_n + 3 * (size_t)f;
            const v3_t na = fetch(normals, nn, in[0]), nb = fetch(normals, nn, in[1]), nc = fetch(normals, nn, in[2]);
            n = add(add(scale(na, (1 - u - v)), scale(nb, u)), scale(nc, v));
        } else { /* flat */
            n = cross(sub(A, B), sub(A, Cc));
        }
        n = unit(n);
        if (flags & 1) n = mk(-n.x, -n.y, -n.z);
        normal[3 * k] = n.x, normal[3 * k + 1] = n.y, normal[3 * k + 2] = n.z;
        ++k;
    }
    free(map);
    free(F);
    return k;
}

/* image: 3 floats per texel, written whole. */
void ref_texels_to_image(const float* values, const int32_t* texel, int64_t n, int32_t width, int32_t height,
                         int32_t passes, const float* fill, float* image) {
    const size_t ntexels = (size_t)width * (size_t)height;
    float* cur = (float*)calloc(3 * ntexels, sizeof(float));
    float* nxt = (float*)calloc(3 * ntexels, sizeof(float));
    uint8_t* fc = (uint8_t*)calloc(ntexels, 1);
    uint8_t* fn = (uint8_t*)calloc(ntexels, 1);
    for (int64_t k = 0; k < n; ++k) {
        memcpy(cur + 3 * (size_t)texel[k], values + 3 * k, 3 * sizeof(float));
        fc[texel[k]] = 1;
    }
    for (int32_t pass = 0; pass < passes; ++pass) {
        for (int32_t j = 0; j < height; ++j)
            for (int32_t i = 0; i < width; ++i) {
                const size_t t = (size_t)j * (size_t)width + (size_t)i;
                if (fc[t]) {
                    memcpy(nxt + 3 * t, cur + 3 * t, 3 * sizeof(float));
                    fn[t] = 1;
                    continue;
                }
                float s[3] = {0.f, 0.f, 0.f};
                int cnt = 0;
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int32_t x = i + dx, y = j + dy;
                        if (x < 0 || y < 0 || x >= width || y >= height) continue;
                        const size_t q = (size_t)y * (size_t)width + (size_t)x;
                        if (!fc[q]) continue;
                        for (int ch = 0; ch < 3; ++ch) s[ch] = s[ch] + cur[3 * q + ch];
                        ++cnt;
                    }
                fn[t] = cnt > 0;
                for (int ch = 0; ch < 3; ++ch) nxt[3 * t + ch] = cnt ? s[ch] / (float)cnt : 0.f;
            }
        float* tf = cur; cur = nxt; nxt = tf;
        uint8_t* tb = fc; fc = fn; fn = tb;
    }
    for (size_t t = 0; t < ntexels; ++t)
        for (int ch = 0; ch < 3; ++ch) image[3 * t + ch] = fc[t] ? cur[3 * t + ch] : fill[ch];
    free(cur), free(nxt), free(fc), free(fn);
}
