/* The radiance query's reference (atr_radiance_rays): for every valid (ray, sample) the
   oracle's own cast_ray on the oracle's own om_path_rng stream, summed in sample order with optional
   continuation. Nothing of the shading loop is restated; the oracle, occlusion_ref.c and gather_ref.c
   stay as they are and are reached by including their source (gather_ref.c for dir_ok).
   Built by tests/radiance_ref.py with the oracle Makefile's flags. */
#include "gather_ref.c"

static int ray_valid(ov3 ro, ov3 rd) {
    return fabsf(ro.x) <= OM_MAX_FLOAT && fabsf(ro.y) <= OM_MAX_FLOAT && fabsf(ro.z) <= OM_MAX_FLOAT && dir_ok(rd);
}

/* A batch of n rays chosen from a pool so that every bounce level is exercised (the tests' coverage
   condition; tests/test_radiance_cpu.py asserts it on the finished batch with ref_radiance). Walking
   the batch's positions i with a count of the paths chosen so far per final bounce count: while some
   count of 1 .. bounce_limit is below `quota`, position i takes -- for the deepest such count that
   the pool can serve -- the first pool ray (scanning on from the last find, wrapping; a ray may be
   taken again at another position) one of whose nsamples samples on the streams of (seed, ray_base + i,
   first_sample + s) ends with that count; otherwise it takes the next pool ray in pool order, whatever
   it does. pick[i] = the pool index at position i. */
void ref_pick_rays(const om_scene* sc, const float* po, const float* pd, int64_t npool, int64_t n,
                   int32_t nsamples, uint32_t first_sample, int64_t ray_base, int32_t bounce_limit, uint64_t seed,
                   int32_t quota, int64_t* pick) {
    int32_t maxn = 1;
    for (int32_t i = 0; i < sc->nmodels; i++)
        if (sc->models[i].tree && sc->models[i].tree->nnodes > maxn) maxn = sc->models[i].tree->nnodes;
    trav_ws w;
    ws_init(&w, maxn);
    int32_t* count = (int32_t*)calloc((size_t)bounce_limit + 1, sizeof(int32_t));
    int64_t cursor = 0, fill = 0;
    for (int64_t i = 0; i < n; i++) {
        int64_t got = -1;
        for (int32_t want = bounce_limit; want >= 1 && got < 0; want--) {
            if (count[want] >= quota) continue;
            for (int64_t t = 0; t < npool && got < 0; t++) {
                int64_t j = (cursor + t) % npool;
                ov3 ro = v3(po[3 * j], po[3 * j + 1], po[3 * j + 2]), rd = v3(pd[3 * j], pd[3 * j + 1], pd[3 * j + 2]);
                if (!ray_valid(ro, rd)) continue;
                for (int32_t s = 0; s < nsamples && got < 0; s++) {
                    uint64_t st, stream;
                    uint32_t c = 0;
                    om_path_rng(seed, ray_base + i, first_sample + (uint32_t)s, &st, &stream);
                    (void)cast_ray(sc, ro, rd, bounce_limit, &st, stream, &c, &w, NULL);
                    if ((int32_t)c == want) got = j;
                }
            }
            if (got >= 0) cursor = (got + 1) % npool;
        }
        if (got < 0) got = fill++ % npool;
        pick[i] = got;
        ov3 ro = v3(po[3 * got], po[3 * got + 1], po[3 * got + 2]), rd = v3(pd[3 * got], pd[3 * got + 1], pd[3 * got + 2]);
        if (!ray_valid(ro, rd)) continue;
        for (int32_t s = 0; s < nsamples; s++) {
            uint64_t st, stream;
            uint32_t c = 0;
            om_path_rng(seed, ray_base + i, first_sample + (uint32_t)s, &st, &stream);
            (void)cast_ray(sc, ro, rd, bounce_limit, &st, stream, &c, &w, NULL);
            count[c]++;
        }
    }
    free(count);
    ws_free(&w);
}

/* sum (3 per ray), ray_casts: in and out -- read as the starting values when first_sample > 0.
   rgb (3 per ray), invalid (a byte per ray): out. sample_casts (optional, nsamples per ray): cast_ray's
   bounce count of every sample, 0xFFFFFFFF for the samples of an invalid ray. An invalid ray (origin
   not finite, or the direction fails dir_ok) is not traced: with first_sample == 0 its rgb and sum
   become 0,0,0 and its ray_casts 0, else all three stay as they came. *nvalid = the valid rays.
   Returns the oracle's n_rays (every intersect_scene call: nsamples first segments per valid ray). */
int64_t ref_radiance(const om_scene* sc, const float* o, const float* d, int64_t nrays, int32_t nsamples,
                     uint32_t first_sample, int64_t ray_base, int32_t bounce_limit, uint64_t seed, float* sum,
                     float* rgb, uint32_t* ray_casts, uint8_t* invalid, uint32_t* sample_casts, int64_t* nvalid) {
    int32_t maxn = 1;
    for (int32_t i = 0; i < sc->nmodels; i++)
        if (sc->models[i].tree && sc->models[i].tree->nnodes > maxn) maxn = sc->models[i].tree->nnodes;
    trav_ws w;
    ws_init(&w, maxn);
    om_counters ctr;
    memset(&ctr, 0, sizeof(ctr));
    int64_t nv = 0;
    for (int64_t i = 0; i < nrays; i++) {
        ov3 ro = v3(o[3 * i], o[3 * i + 1], o[3 * i + 2]), rd = v3(d[3 * i], d[3 * i + 1], d[3 * i + 2]);
        int ok = ray_valid(ro, rd);
        invalid[i] = (uint8_t)!ok;
        if (!ok) {
            if (first_sample == 0) {
                sum[3 * i] = sum[3 * i + 1] = sum[3 * i + 2] = 0.0f;
                rgb[3 * i] = rgb[3 * i + 1] = rgb[3 * i + 2] = 0.0f;
                ray_casts[i] = 0;
            }
            if (sample_casts)
                for (int32_t s = 0; s < nsamples; s++) sample_casts[i * nsamples + s] = 0xFFFFFFFFu;
            continue;
        }
        nv++;
        ov3 col = v3(0, 0, 0);
        uint32_t casts = 0;
        if (first_sample > 0) {
            col = v3(sum[3 * i], sum[3 * i + 1], sum[3 * i + 2]);
            casts = ray_casts[i];
        }
        for (int32_t s = 0; s < nsamples; s++) {
            uint64_t st, stream;
            uint32_t c = 0;
            om_path_rng(seed, ray_base + i, first_sample + (uint32_t)s, &st, &stream);
            col = vadd(col, cast_ray(sc, ro, rd, bounce_limit, &st, stream, &c, &w, &ctr));
            casts += c;
            if (sample_casts) sample_casts[i * nsamples + s] = c;
        }
        sum[3 * i] = col.x; sum[3 * i + 1] = col.y; sum[3 * i + 2] = col.z;
        col = vdiv(col, (float)(first_sample + (uint32_t)nsamples));
        rgb[3 * i] = col.x; rgb[3 * i + 1] = col.y; rgb[3 * i + 2] = col.z;
        ray_casts[i] = casts;
    }
    ws_free(&w);
    if (nvalid) *nvalid = nv;
    return (int64_t)ctr.n_rays;
}
