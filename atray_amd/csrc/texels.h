// texels.h -- lightmap texels (atr_mesh_texels, atr_texels_to_image; texels.hip): the
// coverage rule in separately rounded f32 operations, shared by every kernel that evaluates it, and the
// kernels' arguments. tests/c/texel_ref.c restates the rule in plain C.
#pragma once
#include "engine.h"

namespace atr {

constexpr int32_t kTexelMaxSide = 16384;     // width, height: 1..16,384 (a map of at most 2^28 texels)
constexpr uint32_t kTexelNone = 0xFFFFFFFFu; // face map: no face covers the texel
constexpr int kTexelScanBlock = 1024;        // texels per block of the slot scan's first level
constexpr int kTexelSmallBox = 16;           // a face whose box holds at most this many texels is finished in its lane
constexpr int kTexelFaceWaves = 16;          // waves that share the box of one larger face, 8x8 texels at a time
constexpr int kTexelMaxPasses = 64;

struct UV { float x, y; };

// Centre of texel (i, j) of a w x h map; row 0 is v near 0.
ATR_HD UV texel_centre(int32_t i, int32_t j, float wf, float hf) {
    UV p;
    p.x = (float(i) + 0.5f) / wf;
    p.y = (float(j) + 0.5f) / hf;
    return p;
}
ATR_HD float texel_area2(UV a, UV b, UV c) { return (b.x - a.x) * (c.y - a.y) - (b.y - a.y) * (c.x - a.x); }
// Edge function of p0 -> p1 at p, evaluated from the lexicographically lower end: two faces that share
// the edge compute the same magnitude with opposite signs, so a centre is never lost between them.
ATR_HD float texel_edge(UV p0, UV p1, UV p) {
    float s = 1.0f;
    if (p1.x < p0.x || (p1.x == p0.x && p1.y < p0.y)) {
        const UV t = p0;
        p0 = p1;
        p1 = t;
        s = -1.0f;
    }
    return s * ((p1.x - p0.x) * (p.y - p0.y) - (p1.y - p0.y) * (p.x - p0.x));
}
// Does the face (a, b, c; g = the sign of its area2) cover p? e1, e2, den: the sample's weights.
ATR_HD bool texel_cover(UV a, UV b, UV c, float g, UV p, float& e1, float& e2, float& den) {
    const float e0 = g * texel_edge(b, c, p);
    e1 = g * texel_edge(c, a, p);
    e2 = g * texel_edge(a, b, p);
    den = (e0 + e1) + e2;
    return e0 >= 0.0f && e1 >= 0.0f && e2 >= 0.0f && den > 0.0f;
}

// The mesh as atr_mesh_texels copied it into the context's texel workspace. shade: a scene of one
// model that holds the per-face 9 floats and the smooth flag, so that the normal is shade.h's own
// scene_finish.
struct TexelMesh {
    const float* vertices;    // 3 per vertex
    const float* texcoords;   // 3 per texcoord (u, v, w)
    const int32_t* face_v;    // 3 per face
    const int32_t* face_t;    // 3 per face, -1 = absent
    const DScene* shade;
    uint32_t nvertices, ntexcoords, nfaces;
};

struct TexelParams {
    TexelMesh mesh;
    int32_t width, height;
    int32_t flip;             // ATR_TEXELS_FLIP
    int32_t fill;             // write the per-k arrays (cap >= the count)
    uint32_t* map;            // covering face per texel, padded to whole scan blocks
    uint32_t* sums;           // per scan block: its count, then (scan) its exclusive offset; [nblocks] = the total
    uint32_t nblocks;
    uint32_t* big;            // faces with larger boxes; nbig = the list's length
    uint32_t* nbig;
    atr_texels_out out;
};

struct TexelImageParams {
    int32_t width, height;
    int32_t last;             // the last pass: a texel still empty gets `fill`
    float fill[3];
    const float* src;         // state at the start of the pass
    const uint8_t* src_flag;  // 1 = not empty
    float* dst;
    uint8_t* dst_flag;
};

}  // namespace atr
