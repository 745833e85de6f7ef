/* The hemisphere gather's reference (atr_gather_occlusion): the sampler restated with the
   oracle's own om_path_rng / om_pcg_u32 (through its rand_bi) and vector helpers in C f32, then
   ref_occluded's walk (occlusion_ref.c) for every traced sample, reduced per point. The oracle and
   occlusion_ref.c stay as they are; they are reached by including their source.
   Built by tests/gather_ref.py with the oracle Makefile's flags. */
#include "occlusion_ref.c"

/* atr_trace_rays' validity test on a direction: three finite components, |len2 - 1| <= 2^-20 */
static int dir_ok(ov3 d) {
    if (!(fabsf(d.x) <= OM_MAX_FLOAT && fabsf(d.y) <= OM_MAX_FLOAT && fabsf(d.z) <= OM_MAX_FLOAT)) return 0;
    return fabsf(vmag2(d) - 1.0f) <= 9.5367431640625e-07f;
}

/* Sample s of point i around the normal n: cast_ray's rnd (atr_oracle.c, the scatter-0 direction) on
   the (point_base + i, first_sample + s) stream. */
static ov3 gather_dir(uint64_t seed, int64_t point, uint32_t sample, ov3 n) {
    uint64_t st, stream;
    om_path_rng(seed, point, sample, &st, &stream);
    float r0 = rand_bi(&st, stream);
    float r1 = rand_bi(&st, stream);
    float r2 = rand_bi(&st, stream);
    return vnormalize(vadd(v3(r0, r1, r2), n));
}

/* The sampler alone: dirs (3 per (point, sample)) and traced flags for unit normals; a normal that
   fails the direction test gives zeros. */
void ref_gather_directions(const float* nrm, int64_t npoints, int32_t nsamples, uint32_t first_sample,
                           int64_t point_base, uint64_t seed, float* dirs, uint8_t* traced) {
    for (int64_t i = 0; i < npoints; i++) {
        ov3 n = v3(nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]);
        int nok = dir_ok(n);
        for (int32_t s = 0; s < nsamples; s++) {
            int64_t k = i * nsamples + s;
            ov3 d = v3(0, 0, 0);
            int tr = 0;
            if (nok) {
                d = gather_dir(seed, point_base + i, first_sample + (uint32_t)s, n);
                tr = dir_ok(d) && vdot(d, n) > 0.0f;
            }
            dirs[3 * k] = d.x; dirs[3 * k + 1] = d.y; dirs[3 * k + 2] = d.z;
            traced[k] = (uint8_t)tr;
        }
    }
}

/* The whole gather. visible, occluded: one u32 per point; mask: ceil(nsamples / 32) words per point;
   dirs, traced as above (an invalid point -- p not finite, n not unit, t_max NaN, zero or negative --
   gives zeros everywhere). Returns the number of traced samples. */
int64_t ref_gather(const om_scene* sc, const float* p, const float* nrm, const float* t_max, int64_t npoints,
                   int32_t nsamples, uint32_t first_sample, int64_t point_base, uint64_t seed, float* dirs,
                   uint8_t* traced, uint32_t* visible, uint32_t* occluded, uint32_t* mask) {
    int64_t total = npoints * nsamples, words = (nsamples + 31) / 32, nt = 0;
    ref_gather_directions(nrm, npoints, nsamples, first_sample, point_base, seed, dirs, traced);
    float* ro = (float*)malloc(sizeof(float) * 3 * (size_t)(total ? total : 1));
    float* rd = (float*)malloc(sizeof(float) * 3 * (size_t)(total ? total : 1));
    float* rt = (float*)malloc(sizeof(float) * (size_t)(total ? total : 1));
    int64_t* item = (int64_t*)malloc(sizeof(int64_t) * (size_t)(total ? total : 1));
    uint8_t* out = (uint8_t*)malloc((size_t)(total ? total : 1));
    for (int64_t i = 0; i < npoints; i++) {
        float T = t_max ? t_max[i] : OM_MAX_FLOAT;
        int pok = fabsf(p[3 * i]) <= OM_MAX_FLOAT && fabsf(p[3 * i + 1]) <= OM_MAX_FLOAT &&
                  fabsf(p[3 * i + 2]) <= OM_MAX_FLOAT && T > 0.0f;
        visible[i] = occluded[i] = 0;
        for (int64_t w = 0; w < words; w++) mask[i * words + w] = 0;
        for (int32_t s = 0; s < nsamples; s++) {
            int64_t k = i * nsamples + s;
            if (!pok) {
                dirs[3 * k] = dirs[3 * k + 1] = dirs[3 * k + 2] = 0.0f;
                traced[k] = 0;
            }
            if (!traced[k]) continue;
            for (int a = 0; a < 3; a++) { ro[3 * nt + a] = p[3 * i + a]; rd[3 * nt + a] = dirs[3 * k + a]; }
            rt[nt] = T;
            item[nt++] = k;
        }
    }
    ref_occluded(sc, ro, rd, rt, nt, out, NULL);
    for (int64_t j = 0; j < nt; j++) {
        int64_t i = item[j] / nsamples, s = item[j] % nsamples;
        if (out[j] == 1) occluded[i]++;
        else if (out[j] == 0) { visible[i]++; mask[i * words + s / 32] |= 1u << (s % 32); }
    }
    free(ro); free(rd); free(rt); free(item); free(out);
    return nt;
}
