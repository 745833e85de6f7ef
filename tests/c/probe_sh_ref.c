/* The light probes' reference (atr_probe_sh): for every sample of a valid probe the sphere
   sampler restated on the oracle's own om_path_rng stream and rand_bi (rejection inside a radial
   shell, keeping the state), then the oracle's own cast_ray from the probe along it on that same
   state; the colour times the nine basis values added per probe in sample order, with optional
   continuation. Nothing of the shading loop is restated; the oracle and the other references stay as
   they are and are reached by including their source (radiance_ref.c for OM_MAX_FLOAT's test).
   max_tries is a parameter (the library's is 32), so that the fallback can be reached here.
   Built by tests/probe_sh_ref.py with the oracle Makefile's flags. */
#include "radiance_ref.c"

/* Sample `sample` of probe `point`: up to max_tries tries of three draws; the first with
   2^-10 <= l2 <= 1 is normalised, else +z. *tries = the accepted try (1-based) or max_tries + 1. */
static ov3 probe_dir(uint64_t seed, int64_t point, uint32_t sample, int32_t max_tries, uint64_t* st,
                     uint64_t* stream, int32_t* tries) {
    om_path_rng(seed, point, sample, st, stream);
    for (int32_t t = 1; t <= max_tries; t++) {
        float r0 = rand_bi(st, *stream);
        float r1 = rand_bi(st, *stream);
        float r2 = rand_bi(st, *stream);
        float l2 = (r0 * r0 + r1 * r1) + r2 * r2;
        if (0x1p-10f <= l2 && l2 <= 1.0f) {
            float inv = 1.0f / sqrtf(l2);
            *tries = t;
            return v3(r0 * inv, r1 * inv, r2 * inv);
        }
    }
    *tries = max_tries + 1;
    return v3(0.0f, 0.0f, 1.0f);
}

static void probe_basis(ov3 d, float y[9]) {
    float x = d.x, yy = d.y, z = d.z;
    y[0] = 0.282094792f;
    y[1] = 0.488602512f * yy;
    y[2] = 0.488602512f * z;
    y[3] = 0.488602512f * x;
    y[4] = 1.092548431f * (x * yy);
    y[5] = 1.092548431f * (yy * z);
    y[6] = 0.315391565f * ((3.0f * (z * z)) - 1.0f);
    y[7] = 1.092548431f * (x * z);
    y[8] = 0.546274215f * ((x * x) - (yy * yy));
}

/* The sampler alone: dirs (3 per (probe, sample)) and tries (a byte each). */
void ref_probe_directions(int64_t npoints, int32_t nsamples, uint32_t first_sample, int64_t point_base, uint64_t seed,
                          int32_t max_tries, float* dirs, uint8_t* tries) {
    for (int64_t i = 0; i < npoints; i++)
        for (int32_t s = 0; s < nsamples; s++) {
            int64_t k = i * nsamples + s;
            uint64_t st, stream;
            int32_t t;
            ov3 d = probe_dir(seed, point_base + i, first_sample + (uint32_t)s, max_tries, &st, &stream, &t);
            dirs[3 * k] = d.x; dirs[3 * k + 1] = d.y; dirs[3 * k + 2] = d.z;
            tries[k] = (uint8_t)t;
        }
}

/* sum (27 per probe, index 3 k + c), ray_casts (per probe): in and out -- read as the starting values
   when first_sample > 0. sh (27 per probe), invalid (a byte per probe), sample_rgb, dirs (3 per (probe,
   sample), probe-major), tries (a byte per (probe, sample)): out. sample_casts (one per (probe,
   sample)): cast_ray's bounce count, 0xFFFFFFFF for a sample of an invalid probe. first_kind (a byte
   per (probe, sample)): what the first segment hits, the oracle's OT_* (1 triangle, 2 sphere, 3 plane,
   4 sky), 0 for an invalid probe -- one more intersect_scene call, outside the counters. An invalid
   probe (p not finite) traces nothing: its sample_rgb and dirs rows are zeros, and with first_sample
   == 0 its sh, sum and ray_casts become 0, else all three stay as they came. Returns the oracle's
   n_rays (every intersect_scene call of the samples' cast_ray). */
int64_t ref_probe_sh(const om_scene* sc, const float* p, int64_t npoints, int32_t nsamples, uint32_t first_sample,
                     int64_t point_base, int32_t bounce_limit, uint64_t seed, int32_t max_tries, float* sum,
                     uint32_t* ray_casts, float* sh, uint8_t* invalid, float* sample_rgb, float* dirs, uint8_t* tries,
                     uint32_t* sample_casts, uint8_t* first_kind) {
    int32_t maxn = 1;
    for (int32_t i = 0; i < sc->nmodels; i++)
        if (sc->models[i].tree && sc->models[i].tree->nnodes > maxn) maxn = sc->models[i].tree->nnodes;
    trav_ws w;
    ws_init(&w, maxn);
    om_counters ctr;
    memset(&ctr, 0, sizeof(ctr));
    for (int64_t i = 0; i < npoints; i++) {
        ov3 po = v3(p[3 * i], p[3 * i + 1], p[3 * i + 2]);
        int ok = fabsf(po.x) <= OM_MAX_FLOAT && fabsf(po.y) <= OM_MAX_FLOAT && fabsf(po.z) <= OM_MAX_FLOAT;
        invalid[i] = (uint8_t)!ok;
        if (!ok) {
            if (first_sample == 0) {
                for (int j = 0; j < 27; j++) sum[27 * i + j] = sh[27 * i + j] = 0.0f;
                ray_casts[i] = 0;
            }
            for (int32_t s = 0; s < nsamples; s++) {
                int64_t k = i * nsamples + s;
                sample_rgb[3 * k] = sample_rgb[3 * k + 1] = sample_rgb[3 * k + 2] = 0.0f;
                dirs[3 * k] = dirs[3 * k + 1] = dirs[3 * k + 2] = 0.0f;
                tries[k] = 0;
                sample_casts[k] = 0xFFFFFFFFu;
                first_kind[k] = 0;
            }
            continue;
        }
        float acc[27];
        uint32_t casts = 0;
        for (int j = 0; j < 27; j++) acc[j] = first_sample > 0 ? sum[27 * i + j] : 0.0f;
        if (first_sample > 0) casts = ray_casts[i];
        for (int32_t s = 0; s < nsamples; s++) {
            int64_t k = i * nsamples + s;
            uint64_t st, stream;
            int32_t t;
            ov3 d = probe_dir(seed, point_base + i, first_sample + (uint32_t)s, max_tries, &st, &stream, &t);
            dirs[3 * k] = d.x; dirs[3 * k + 1] = d.y; dirs[3 * k + 2] = d.z;
            tries[k] = (uint8_t)t;
            isect id;
            memset(&id, 0, sizeof(id));
            intersect_scene(sc, po, d, &id, &w, NULL);
            first_kind[k] = (uint8_t)id.type;
            uint32_t cc = 0;
            ov3 c = cast_ray(sc, po, d, bounce_limit, &st, stream, &cc, &w, &ctr);
            casts += cc;
            sample_rgb[3 * k] = c.x; sample_rgb[3 * k + 1] = c.y; sample_rgb[3 * k + 2] = c.z;
            sample_casts[k] = cc;
            float y[9];
            probe_basis(d, y);
            float col[3] = {c.x, c.y, c.z};
            for (int q = 0; q < 9; q++)
                for (int ch = 0; ch < 3; ch++) acc[3 * q + ch] = acc[3 * q + ch] + (col[ch] * y[q]);
        }
        for (int j = 0; j < 27; j++) {
            sum[27 * i + j] = acc[j];
            sh[27 * i + j] = (acc[j] * 12.566370614f) / (float)(first_sample + (uint32_t)nsamples);
        }
        ray_casts[i] = casts;
    }
    ws_free(&w);
    return (int64_t)ctr.n_rays;
}
