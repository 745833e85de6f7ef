// cluster.h -- the clustered leaf scan: one leaf's result from a fraction of
// the reference's triangle tests, bit-identical.
//
// Each leaf's primitives are regrouped into spatial clusters of <= 16 with a bounding box, and a
// primitive is skipped only when it provably cannot be accepted with t <= the best so far:
//   * rounding (first order): an accepted hit of the culled test (computed
//     det >= kTol; u, v in range) has its true line within D_lat of the triangle and its
//     computed t within D_t of the true t, D_lat + D_t <= W (29 eps |ab||ac| / det + 6 eps),
//     W >= |o - a| + |edge|: the u, v, t numerators carry ~7.5 eps |tvec| |ac| (resp. |ab|,
//     |ab||ac|) of cancellation, det ~6.5 eps |ab||ac|. A box grown by that much (36 and
//     12 eps here, with the slab's own rounding) is entered no later than the computed t of any
//     acceptable primitive inside and left no earlier.
//   * D depends on det, which is not known per cluster: the box is grown twice, for det >= kTol
//     (loose) and det >= kTau (tight). Missing the loose box skips the cluster. Inside the
//     tight box every front-facing primitive is a candidate. In between, only primitives whose
//     det could lie in [kTol, kTau) are: the det estimate -(d . n) (n = ab x ac, stored per
//     cluster as f16 integer multiples of one step) is within a bounded margin of the computed det
//     (cluster_step), which widens the screen's band.
//     Back-facing primitives (det < kTol) are screened out the same way in both cases.
//   * one level up, per (camera, leaf): the primary table kernels' passes leave out a leaf whose box
//     -- the bounds of its clusters' loose boxes for that camera -- the ray misses (leaf_box_add below;
//     trace.h leaf_box_miss).
//   * inside the leaf the reference keeps the FIRST primitive (leaf order) with the smallest t
//     below the incoming best (strict <, kd_tree.cpp:440-456); clusters change the visiting
//     order, so equal t is resolved by the leaf rank, and a best carried in from an earlier
//     leaf never loses a tie.
#pragma once
#include "trace.h"

namespace atr {

constexpr float kTau = 3e-3f;
constexpr float kEps = 5.9604645e-8f;  // 2^-24
constexpr float kPadRel = 36.0f * kEps, kPadAbs = 12.0f * kEps;

// The full-test operands of slot k, one 48-B record {a.xyz, ab.x}{ab.yz, ac.xy}{ac.z, bits(leaf
// rank), bits(face), 0}: one cache line (at most two) per test. (Round 3's three SoA streams
// touched three lines per test; incoherent bounce rays miss in L2 on most of them)
__device__ __forceinline__ void load_prim(const DModel& m, uint32_t k, float4_t& a0, float4_t& a1, float4_t& a2) {
    a0 = m.prim[3 * size_t(k)];
    a1 = m.prim[3 * size_t(k) + 1];
    a2 = m.prim[3 * size_t(k) + 2];
}

typedef _Float16 h2_t __attribute__((ext_vector_type(2)));

// Which scan flavours load the first screen normals with the box test (cluster_cands EARLY): bit 0
// primary-only rays, bit 1 camera rays of the path engine, bit 2 bounce rays, bit 3 primary-only
// rays that read the per-camera table of box growths (experiment builds set others; 0 = every
// flavour loads them after the box test passes). Not the camera rays: their 6-wave kernel then
// spills 20 dwords instead of 5 and writes 4 GB more per c4 frame, for no time measured (c4
// 3,824-3,826 Mrays/s without, 3,828-3,834 with). The table flavour keeps them although its 7-wave
// kernel would have no scratch without: c3 8,851-8,952 Mrays/s with, 8,603-8,799 without
// 
#ifndef ATR_EARLY_NRM
#define ATR_EARLY_NRM 13
#endif

// Ray-side constants of the cluster screen, once per ray (f16 direction, its L1 norm).
struct ScreenRay {
    float ax, ay, az, sd;
    h2_t dxy, dz_lo, dz_hi;
};
__device__ __forceinline__ ScreenRay screen_ray(const Ray& r) {
    ScreenRay s;
    s.ax = fabsf(r.inv.x); s.ay = fabsf(r.inv.y); s.az = fabsf(r.inv.z);
    s.sd = fabsf(r.d.x) + fabsf(r.d.y) + fabsf(r.d.z);
    s.dxy = h2_t{(_Float16)r.d.x, (_Float16)r.d.y};
    const _Float16 hz = (_Float16)r.d.z;
    s.dz_lo = h2_t{hz, (_Float16)0.0f};
    s.dz_hi = h2_t{(_Float16)0.0f, hz};
    return s;
}

// The part of the padded box test that depends only on the ray origin and the cluster record
// lo = {lo.xyz, P | (n - 1)}, hi = {hi.xyz, q}: the growths of the loose (x) and the tight (y) box.
// Camera rays share one origin, so the primary kernels read this pair per (camera, cluster) from a
// table (render.hip camera_pads_kernel) that calls this same function: the same operations in the
// same order (-ffp-contract=off), the same bits as the inline evaluation.
__device__ __forceinline__ float2_t cluster_grow(V3 o, float4_t lo, float4_t hi) {
    const float ex = hi.x - lo.x, ey = hi.y - lo.y, ez = hi.z - lo.z;
    const float fx = fmaxf(fabsf(lo.x - o.x), fabsf(hi.x - o.x));
    const float fy = fmaxf(fabsf(lo.y - o.y), fabsf(hi.y - o.y));
    const float fz = fmaxf(fabsf(lo.z - o.z), fabsf(hi.z - o.z));
    // W >= |o - a| + |edge| for every primitive inside (far corner; L1 extent >= diagonal). The
    // hardware square root (v_sqrt_f32, within 1 ulp) instead of the correctly rounded expansion
    // (~15 VALU: denormal scaling, two FMA corrections): W only has to bound the distance from
    // above, the 1 + 2^-21 factor covers 8 ulp, and the 2^-63 term the flushed denormal case
    const float W = (__builtin_amdgcn_sqrtf(fx * fx + fy * fy + fz * fz) + 1.0842022e-19f) * 1.0000005f + (ex + ey + ez);
    const float P = lo.w;  // >= |ab||ac| of every primitive inside
    float2_t g;
    g.x = W * (P * (kPadRel / (0.9f * kTol)) + kPadAbs);
    g.y = W * (P * (kPadRel / (0.9f * kTau)) + kPadAbs);
    return g;
}

// The det floor of a (camera, cluster) pair (the facing fold): a delta in
// [kTol, kTau] such that, for every ray from `eye` that accepts a primitive of the cluster, that
// primitive's computed det is >= delta. The loose growth may then be sized for det >= delta instead
// of det >= kTol (cluster_grow_fold): camera_pads_kernel stores that growth where the primary
// kernels read the loose one. Evaluated in f64 (the table kernel is no hot path), so that the
// rounding of the bound itself is far below its margin.
//
//   * The rays. A ray (eye, d) that accepts a primitive has computed det >= kTol, so by the rounding
//     bound above its true line passes within W (29 eps P / kTol + 6 eps) <= gl of the triangle, at
//     a parameter within that distance of the computed t. B = the cluster box grown per axis by
//     gl (1 + 2^-10) + 2^-20 F_axis (F = the far face's distance from the eye: the f32 slab test's
//     own rounding, with room). With the eye outside B -- required here as r_min > r_max / 1024,
//     r_min and r_max the distances from the eye to B and to its far corner -- that point p of the
//     line lies in B at a positive parameter: d = |d| (p - eye) / |p - eye|.
//   * The bound. With N = ab x ac, s(p) = -(p - eye) . N is affine in p: over B its extremes are
//     per axis at one of the two faces. The true det -(d . N) = |d| s(p) / |p - eye| then lies in
//     [L, U] |d| with L = s_min / (s_min >= 0 ? r_max : r_min), U = s_max / (s_max >= 0 ? r_min : r_max).
//   * The margin m = 32 eps P, P >= |ab||ac| >= |N| the cluster's bound: 16 eps P between -(d . N)
//     and the computed det (what the screen uses, cluster_pads); 8 eps P for |d| = 1 +- 4.5 eps
//     (unit(): three products and two adds, a square root, a division, a product); 8 eps P for the
//     evaluation here: f32 products are exact in f64 and N's differences round by 2^-53 |ab||ac|,
//     the sums of s by a few 2^-53 r_max P, the square roots and quotients by 2^-52 relative, and
//     r_max / r_min <= 1024, so the whole is below 2^-38 P.
//   * A primitive with U < kTol - m is rejected by the culled test for every such ray and takes no
//     part. Otherwise computed det >= L - m; delta = clamp(min L - m, kTol, kTau), rounded down to
//     f32. NaN or infinite operands give comparisons that are false: not rejected, delta = kTol.
struct FoldBox {
    double x0[3], x1[3];  // B's faces relative to the eye
    double rmin, rmax;
    bool ok;  // finite operands, the eye clearly outside B, a usable screen step
};
__device__ __forceinline__ FoldBox fold_box(V3 eye, float4_t lo, float4_t hi, float gl) {
    FoldBox b;
    const double l[3] = {lo.x, lo.y, lo.z}, h[3] = {hi.x, hi.y, hi.z}, e[3] = {eye.x, eye.y, eye.z};
    const double g = double(gl) * (1.0 + 0x1p-10);
    double n2 = 0.0, f2 = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double F = fmax(fabs(l[a] - e[a]), fabs(h[a] - e[a]));
        const double slack = g + 0x1p-20 * F;
        b.x0[a] = l[a] - e[a] - slack;
        b.x1[a] = h[a] - e[a] + slack;
        const double nr = fmax(fmax(b.x0[a], -b.x1[a]), 0.0), fr = fmax(fabs(b.x0[a]), fabs(b.x1[a]));
        n2 += nr * nr;
        f2 += fr * fr;
    }
    b.rmin = sqrt(n2);
    b.rmax = sqrt(f2);
    // f2 finite: every operand was; hi.w: a zero or subnormal screen step means no screen
    b.ok = f2 < double(__builtin_inff()) && b.rmin > b.rmax * 0x1p-10 && hi.w >= 1.1754944e-38f;
    return b;
}

// One primitive's part: rejected for every ray of the cone (true), or its lower bound less the margin.
__device__ __forceinline__ bool fold_prim(const FoldBox& b, float P, float4_t a0, float4_t a1, float4_t a2,
                                          double& lower) {
    const double abx = a0.w, aby = a1.x, abz = a1.y, acx = a1.z, acy = a1.w, acz = a2.x;
    const double N[3] = {aby * acz - abz * acy, abz * acx - abx * acz, abx * acy - aby * acx};
    double smin = 0.0, smax = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double u = -b.x0[a] * N[a], v = -b.x1[a] * N[a];
        smin += fmin(u, v);
        smax += fmax(u, v);
    }
    const double m = 32.0 * double(kEps) * double(P);
    const double L = smin / (smin >= 0.0 ? b.rmax : b.rmin), U = smax / (smax >= 0.0 ? b.rmin : b.rmax);
    lower = L - m;
    if (!(lower == lower)) lower = -double(__builtin_inff());
    return U < double(kTol) - m;
}

// delta from the smallest lower bound of the primitives that take part (+inf: none does).
__device__ __forceinline__ float fold_delta(double lower) {
    if (!(lower > double(kTol))) return kTol;
    if (lower >= double(kTau)) return kTau;
    float d = float(lower);
    if (double(d) > lower) d = __uint_as_float(__float_as_uint(d) - 1u);  // positive: the float below
    return fmaxf(d, kTol);
}

// cluster_grow's loose growth for det >= delta (kTol <= delta <= kTau): the same W and P and the
// same order of operations, delta in kTol's place; g = cluster_grow's pair. delta = kTol returns
// g.x itself, and the result never falls below the tight growth.
__device__ __forceinline__ float cluster_grow_fold(V3 o, float4_t lo, float4_t hi, float delta, float2_t g) {
    if (!(delta > kTol)) return g.x;
    const float ex = hi.x - lo.x, ey = hi.y - lo.y, ez = hi.z - lo.z;
    const float fx = fmaxf(fabsf(lo.x - o.x), fabsf(hi.x - o.x));
    const float fy = fmaxf(fabsf(lo.y - o.y), fabsf(hi.y - o.y));
    const float fz = fmaxf(fabsf(lo.z - o.z), fabsf(hi.z - o.z));
    const float W = (__builtin_amdgcn_sqrtf(fx * fx + fy * fy + fz * fz) + 1.0842022e-19f) * 1.0000005f + (ex + ey + ez);
    const float P = lo.w;
    const float gf = W * (P * (kPadRel / (0.9f * delta)) + kPadAbs);  // IEEE division
    return fminf(fmaxf(gf, g.y), g.x);
}

// Cluster record lo, hi and its growths g (cluster_grow): the two rounding-padded box
// tests. False: no primitive inside can be accepted with t <= best. Else the det band
// [dlo, dhi) of the primitives that still need the full test.
__device__ __forceinline__ bool cluster_pads(const Ray& r, const ScreenRay& sr, float4_t lo, float4_t hi, float2_t g,
                                             float best, float& dlo, float& dhi) {
    const float gl = g.x, gt = g.y;
    const float P = lo.w;
    // slab entry/exit of the unpadded box per axis, then widened by g |inv| per axis
    const float x0 = (lo.x - r.o.x) * r.inv.x, x1 = (hi.x - r.o.x) * r.inv.x;
    const float y0 = (lo.y - r.o.y) * r.inv.y, y1 = (hi.y - r.o.y) * r.inv.y;
    const float z0 = (lo.z - r.o.z) * r.inv.z, z1 = (hi.z - r.o.z) * r.inv.z;
    const float nx = fminf(x0, x1), fx1 = fmaxf(x0, x1), ny = fminf(y0, y1), fy1 = fmaxf(y0, y1),
                nz = fminf(z0, z1), fz1 = fmaxf(z0, z1);
    float tn = fmaxf(fmaxf(nx - gl * sr.ax, ny - gl * sr.ay), nz - gl * sr.az);
    float tf = fminf(fminf(fx1 + gl * sr.ax, fy1 + gl * sr.ay), fz1 + gl * sr.az);
    if (tn > tf || tf < 0.f || tn > best) return false;
    tn = fmaxf(fmaxf(nx - gt * sr.ax, ny - gt * sr.ay), nz - gt * sr.az);
    tf = fminf(fminf(fx1 + gt * sr.ax, fy1 + gt * sr.ay), fz1 + gt * sr.az);
    const bool tight = !(tn > tf || tf < 0.f || tn > best);
    // screen: det estimate -q (d . p) with the cluster's quantized normals n ~ q p (p integers
    // of at most 511, f16, 96 B per cluster) and d rounded to f16, two f16 dot products per
    // primitive. |n - q p| <= q/2 per component, d's f16 rounding <= 2^-11 |d_a| + 2^-25, the
    // f32 accumulation a few eps: the estimate is within
    //   (|d.x| + |d.y| + |d.z|) q (0.51 + 511 (2^-11 + 8 eps)) + 16 eps 511 q + 2^-20 q
    // of -(d . n), which is within 16 eps |ab||ac| of the computed det; the band is widened by it.
    const float q = hi.w;
    const float mq = sr.sd * (q * (0.51f + 511.0f * (4.8828125e-4f + 8.0f * kEps))) +
                     q * (16.0f * kEps * 511.0f + 9.5367432e-7f) + 16.0f * kEps * P;
    dlo = kTol - mq;
    dhi = tight ? __builtin_inff() : kTau + mq;
    return true;
}

// The direction hull of a wave of one-origin rays: per axis the smallest and the largest r.inv of
// its lanes (wave-uniform: SGPRs). ok: all six are finite and an axis' two ends have one sign.
struct WaveHull {
    float lx, hx, ly, hy, lz, hz;
    bool ok;
};

// The loose test of cluster_pads on the hull instead of one ray (the wave cull):
// false only when cluster_pads returns false in every lane of the wave, whatever its best. The same
// f32 operations on the interval's ends: lo - o and hi - o are the lanes' own bits (one origin),
// fl(a s) is monotone in s, so is fl(g |s|) for g >= 0, fl(x - y) and fl(x + y) in each argument,
// min and max; so every lane's tn is at least the lower tn here and its tf at most the upper tf.
// Any NaN keeps the cluster (the comparisons are false), and so does a growth that overflows.
__device__ __forceinline__ bool cluster_hull_keep(V3 o, const WaveHull& hl, float4_t lo, float4_t hi, float gl) {
    const float ax = lo.x - o.x, bx = hi.x - o.x, ay = lo.y - o.y, by = hi.y - o.y, az = lo.z - o.z, bz = hi.z - o.z;
    const float x0 = ax * hl.lx, x1 = ax * hl.hx, x2 = bx * hl.lx, x3 = bx * hl.hx;
    const float y0 = ay * hl.ly, y1 = ay * hl.hy, y2 = by * hl.ly, y3 = by * hl.hy;
    const float z0 = az * hl.lz, z1 = az * hl.hz, z2 = bz * hl.lz, z3 = bz * hl.hz;
    const float nx = fminf(fminf(x0, x1), fminf(x2, x3)), fx = fmaxf(fmaxf(x0, x1), fmaxf(x2, x3));
    const float ny = fminf(fminf(y0, y1), fminf(y2, y3)), fy = fmaxf(fmaxf(y0, y1), fmaxf(y2, y3));
    const float nz = fminf(fminf(z0, z1), fminf(z2, z3)), fz = fmaxf(fmaxf(z0, z1), fmaxf(z2, z3));
    const float gx = gl * fmaxf(fabsf(hl.lx), fabsf(hl.hx)), gy = gl * fmaxf(fabsf(hl.ly), fabsf(hl.hy)),
                gz = gl * fmaxf(fabsf(hl.lz), fabsf(hl.hz));
    const float tn = fmaxf(fmaxf(nx - gx, ny - gy), nz - gz);
    const float tf = fminf(fminf(fx + gx, fy + gy), fz + gz);
    const bool cull = tn > tf || tf < 0.f;
    return !cull || !(fmaxf(fmaxf(gx, gy), gz) < __builtin_inff());
}

// The leaf box of a (camera, leaf) pair: per axis, bounds of every cluster box of the
// leaf grown by the row's own loose growth of that cluster -- the folded g.x the product kernels read
// -- and by a slack for the slab arithmetic, in fold_box's form: g (1 + 2^-10) + 2^-20 F_axis, F the
// far face's distance from the eye. A ray from the eye whose plain slab test misses [LO, HI]
// (trace.h leaf_box_miss) fails cluster_pads' loose test on every cluster of the leaf. All in f32, one
// operation at a time (-ffp-contract=off), so that a test can restate it; every bound is moved one
// float outward after its last rounding, so the rounding of the construction itself only widens it.
// An entry is {LO.xyz, bits(flag)}{HI.xyz, 0}: kLeafBoxTest (0) the slab test decides, kLeafBoxEmpty
// a leaf without clusters (always left out: LO = +inf, HI = -inf would not fail a slab test),
// kLeafBoxKeep a leaf that is never left out -- a NaN, an infinite operand or growth, or a bound
// whose difference from the eye overflows, so that the test's own operands are always finite.

// The float below / above x (finite x; a zero steps to the smallest subnormal of that sign).
__device__ __forceinline__ float f32_below(float x) {
    const uint32_t u = __float_as_uint(x);
    if (x > 0.f) return __uint_as_float(u - 1u);
    if (x < 0.f) return __uint_as_float(u + 1u);
    return x == 0.f ? __uint_as_float(0x80000001u) : x;
}
__device__ __forceinline__ float f32_above(float x) { return -f32_below(-x); }

struct LeafBox {
    float lo[3], hi[3];
    bool bad;
};
__device__ __forceinline__ void leaf_box_init(LeafBox& b) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { b.lo[a] = __builtin_inff(); b.hi[a] = -__builtin_inff(); }
    b.bad = false;
}
// One cluster's part: record words lo, hi and the row's loose growth gl of that cluster.
__device__ __forceinline__ void leaf_box_add(LeafBox& b, V3 eye, float4_t lo, float4_t hi, float gl) {
    constexpr float inf = __builtin_inff();
    const float l[3] = {lo.x, lo.y, lo.z}, h[3] = {hi.x, hi.y, hi.z}, e[3] = {eye.x, eye.y, eye.z};
    const float g = gl * 1.0009765625f;  // 1 + 2^-10
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float F = fmaxf(fabsf(l[a] - e[a]), fabsf(h[a] - e[a]));
        const float slack = g + 9.5367432e-7f * F;  // 2^-20 F
        const float x0 = f32_below(l[a] - slack), x1 = f32_above(h[a] + slack);
        // (the comparisons are false for a NaN, which fminf and fmaxf would drop)
        if (!(slack < inf) || !(fabsf(x0) < inf) || !(fabsf(x1) < inf)) b.bad = true;
        b.lo[a] = fminf(b.lo[a], x0);
        b.hi[a] = fmaxf(b.hi[a], x1);
    }
}
// The entry of a leaf of n clusters, all added.
__device__ __forceinline__ void leaf_box_entry(const LeafBox& b, uint32_t n, V3 eye, float4_t& e0, float4_t& e1) {
    constexpr float inf = __builtin_inff();
    const float e[3] = {eye.x, eye.y, eye.z};
    bool bad = b.bad;
#pragma unroll
    for (int a = 0; a < 3; ++a)  // the slab test's first operation, on its own operands
        if (!(fabsf(b.lo[a] - e[a]) < inf) || !(fabsf(b.hi[a] - e[a]) < inf)) bad = true;
    const uint32_t flag = n == 0 ? kLeafBoxEmpty : bad ? kLeafBoxKeep : kLeafBoxTest;
    const bool box = flag == kLeafBoxTest;
    e0 = float4_t{box ? b.lo[0] : 0.f, box ? b.lo[1] : 0.f, box ? b.lo[2] : 0.f, __uint_as_float(flag)};
    e1 = float4_t{box ? b.hi[0] : 0.f, box ? b.hi[1] : 0.f, box ? b.hi[2] : 0.f, 0.f};
}

// Screen of 8 primitives g .. g + 7 of n: words a0, a1 hold (nx, ny) of slots g .. g + 7 as f16,
// z the nz of slots g .. g + 7 (two per word). Bit j: slot g + j needs the full test.
// Bit j set iff the f16 dot D_j of slot g + j lies in (blo, ahi]: the det band mapped back through
// the cluster's step by the caller (cluster_cands). (The slots past n are masked off once per
// cluster by the caller, not per primitive.)
#ifndef ATR_SCREEN_TWO_CMP
// The band as one comparison: |D - mid| <= half. mid enters as the z dot's accumulator, so each
// primitive costs two dots and one compare (|.| is an operand modifier). Every dot D lies within
// +-3 x 511 x 1.0005 < 1600 (f16 direction, integer normals of at most 511), so the band is first
// clipped to [-1600, 1600] -- the tight band (blo = -inf) and bands beyond every D keep exactly
// the D they kept -- which also bounds mid and half. half covers the closed band plus the
// rounding of mid and of the accumulation with mid in it (<= 2^-22 (1600 + |mid|)): the screen
// only grows. An empty band stays empty (half < 0); NaN ends open the band.
__device__ __forceinline__ void screen_band(float blo, float ahi, float& mid, float& half) {
    const float lo = fmaxf(blo, -1600.0f), hi = fminf(ahi, 1600.0f);
    mid = 0.5f * (lo + hi);
    half = 0.5f * (hi - lo) * 1.000001f + (fabsf(mid) + 2048.0f) * 4.7683716e-7f;  // 2^-21
}
__device__ __forceinline__ uint32_t screen8(const ScreenRay& sr, float nmid, float half, uint4_t a0, uint4_t a1,
                                            uint4_t z) {
    const uint32_t xy[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
    const uint32_t zz[4] = {z.x, z.y, z.z, z.w};
    uint32_t gc = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const h2_t pxy = __builtin_bit_cast(h2_t, xy[j]), pz = __builtin_bit_cast(h2_t, zz[j / 2]);
        float dz;
        asm("v_dot2_f32_f16 %0, %1, %2, %3" : "=v"(dz) : "v"((j & 1) ? sr.dz_hi : sr.dz_lo), "v"(pz), "v"(nmid));
        const float e = __builtin_amdgcn_fdot2(sr.dxy, pxy, dz, false);
        if (fabsf(e) <= half) gc |= 1u << j;
    }
    return gc;
}
#else
__device__ __forceinline__ uint32_t screen8(const ScreenRay& sr, float blo, float ahi, uint4_t a0, uint4_t a1,
                                            uint4_t z) {
    const uint32_t xy[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
    const uint32_t zz[4] = {z.x, z.y, z.z, z.w};
    uint32_t gc = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const h2_t pxy = __builtin_bit_cast(h2_t, xy[j]), pz = __builtin_bit_cast(h2_t, zz[j / 2]);
        // the z term with a zero accumulator operand (VOP3P v_dot2_f32_f16 ..., 0): the builtin
        // selects v_dot2c_f32_f16, whose accumulator is its destination, plus a v_mov of the zero
        float dz;
        asm("v_dot2_f32_f16 %0, %1, %2, 0" : "=v"(dz) : "v"((j & 1) ? sr.dz_hi : sr.dz_lo), "v"(pz));
        const float e = __builtin_amdgcn_fdot2(sr.dxy, pxy, dz, false);
        if (e > blo && e <= ahi) gc |= 1u << j;
    }
    return gc;
}
#endif

// The table's entry of cluster c (RenderParams::pads): one pair per cluster, {folded loose, tight}, in
// the tables the product kernels read; two in the COUNT launches' tables, {unfolded loose, tight}
// {folded loose, det floor}, so the COUNT build's tests read what the table kernel wrote for them.
template <bool COUNT>
__device__ __forceinline__ size_t pads_entry(size_t c) { return COUNT ? 2 * c : c; }

// Cluster c of a leaf: the padded box tests and the screen against the bound `best`. Returns the
// mask of the primitives (slot 16 c + bit) that still need the full test.
// PADS: the growths of the box come from the camera's table row `pads` (indexed by the model's
// cluster), loaded with the cluster record, instead of being computed from the origin.
// wskip (COUNT with PADS): the leaf box says the ray misses this leaf; counted if the cluster passes.
template <bool COUNT, bool EARLY = true, bool PADS = false>
__device__ __forceinline__ uint32_t cluster_cands(const Ray& r, const DModel& m, uint32_t c, float4_t lo, float4_t hi,
                                                  float best, Ctr& ct, const float2_t* pads = nullptr,
                                                  [[maybe_unused]] bool wskip = false) {
    // (the COUNT build's table is wide, pads_entry below: the unfolded pair, then the folded growth)
    float2_t g;
    if constexpr (PADS) g = pads[pads_entry<COUNT>(c)];
    // the screen constants (7 values) are recomputed for every cluster from an opaque copy of the
    // ray instead of being hoisted out of the scan loops and held through the passes and rounds:
    // ~10 VALU per cluster for 7 VGPRs, what lets HYBRID run 6 waves/SIMD
    Ray rr = r;
    asm volatile("" : "+v"(rr.d.x), "+v"(rr.d.y), "+v"(rr.d.z), "+v"(rr.inv.x), "+v"(rr.inv.y), "+v"(rr.inv.z));
    const ScreenRay sr = screen_ray(rr);
    const uint4_t* nb = m.cnrm + kClusterBlock * size_t(c);
    // EARLY: the first 8 slots' screen normals are loaded together with the box test instead of
    // after it passes -- one dependent memory round trip less per cluster on the dealt rounds' chain,
    // at 12 VGPRs held through the pads (c3 +1.2%, c4 +0.7%, round 6)
    uint4_t e0, e1, ez;
    if constexpr (EARLY) {
        e0 = nb[0], e1 = nb[1], ez = nb[kMaxClusterSize / 4];
    }
    // The COUNT build goes on counting the unfolded loose box's work (its counters are compared with
    // the inline kernels'): its table holds the unfolded pair too, written by the table kernel next to
    // the folded growth, which it tests only to count what the product kernels no longer do.
    [[maybe_unused]] float2_t gfold;
    if constexpr (PADS && COUNT) gfold = float2_t{pads[pads_entry<COUNT>(c) + 1].x, g.y};
    if constexpr (!PADS) g = cluster_grow(r.o, lo, hi);
    float dlo, dhi;
    if (!cluster_pads(r, sr, lo, hi, g, best, dlo, dhi)) return 0;
    const uint32_t n = (__float_as_uint(lo.w) & 31u) + 1u;
    if constexpr (COUNT) ct.screen += n;
    if constexpr (PADS && COUNT) {
        float fl, fh;
        if (!cluster_pads(r, sr, lo, hi, gfold, best, fl, fh)) { ct.fold_box += 1; ct.fold_screen += n; }
        else if (wskip) ct.lb_unsound += 1;  // wskip: the product pass leaves this visit's leaf out
    }
    const uint32_t slots = (2u << (n - 1)) - 1u;  // [0, n), 1 <= n <= 16
    const float q = hi.w;
    if (!(q >= 1.1754944e-38f)) return slots;  // zero or subnormal step (degenerate normals): no screen
    // The band dlo <= -q D < dhi of the estimate, as a band of the dot D itself: D in
    // (-dhi / q, -dlo / q] (one reciprocal per cluster instead of a product per primitive). The
    // ends are widened by 2^-20 relative -- the hardware reciprocal (1 ulp) and the products'
    // rounding are below 2^-22 -- and by 2^-126 absolute (flushed subnormals), so every primitive
    // whose rounded product fell in the band still passes: the screen only grows.
    const float rq = __builtin_amdgcn_rcpf(q);
    const float a = -dlo * rq, b = -dhi * rq;  // b = -inf for the tight case (dhi = inf)
    const float ahi = a + fabsf(a) * 9.5367432e-7f + 1.1754944e-38f;
    const float blo = b - fabsf(b) * 9.5367432e-7f - 1.1754944e-38f;
    uint32_t cand = 0;
#ifndef ATR_SCREEN_TWO_CMP
    float mid, half;
    screen_band(blo, ahi, mid, half);
    if constexpr (EARLY) {
        cand = screen8(sr, -mid, half, e0, e1, ez);
        if (n > 8) cand |= screen8(sr, -mid, half, nb[2], nb[3], nb[kMaxClusterSize / 4 + 1]) << 8;
    } else {
        for (uint32_t g = 0; g < n; g += 8)  // eight primitives per step: (nx, ny) x 8, nz x 8
            cand |= screen8(sr, -mid, half, nb[g / 4], nb[g / 4 + 1], nb[kMaxClusterSize / 4 + g / 8]) << g;
    }
#else
    for (uint32_t g = 0; g < n; g += 8)
        cand |= screen8(sr, blo, ahi, nb[g / 4], nb[g / 4 + 1], nb[kMaxClusterSize / 4 + g / 8]) << g;
#endif
    return cand & slots;
}

}  // namespace atr
