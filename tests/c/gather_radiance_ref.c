/* The hemisphere radiance gather's reference (atr_gather_radiance): for every sample of a
   valid point the gather's direction on the oracle's own om_path_rng stream (three rand_bi draws, as
   gather_ref.c's gather_dir, keeping the state), then the oracle's own cast_ray from the point along it
   on that same state; summed per point in sample order with optional continuation. Nothing of the
   shading loop is restated; the oracle and the other references stay as they are and are reached by
   including their source (radiance_ref.c for ray_valid's parts, gather_ref.c for dir_ok).
   Built by tests/gather_radiance_ref.py with the oracle Makefile's flags. */
#include "radiance_ref.c"

/* sum (3 per point), samples, ray_casts (per point): in and out -- read as the starting values when
   first_sample > 0. rgb (3 per point), invalid (a byte per point), sample_rgb, dirs (3 per (point,
   sample), point-major), traced (a byte per (point, sample)): out. sample_casts (optional, one per
   (point, sample)): cast_ray's bounce count, 0xFFFFFFFF for a sample that is not traced. An invalid
   point (p not finite, or n fails dir_ok) traces nothing: its sample_rgb and dirs rows are zeros, and
   with first_sample == 0 its rgb, sum, samples and ray_casts become 0, else all four stay as they
   came. Returns the oracle's n_rays (every intersect_scene call of the traced samples' cast_ray). */
int64_t ref_gather_radiance(const om_scene* sc, const float* p, const float* nrm, int64_t npoints, int32_t nsamples,
                            uint32_t first_sample, int64_t point_base, int32_t bounce_limit, uint64_t seed,
                            float* sum, uint32_t* samples, uint32_t* ray_casts, float* rgb, uint8_t* invalid,
                            float* sample_rgb, float* dirs, uint8_t* traced, uint32_t* sample_casts) {
    int32_t maxn = 1;
    for (int32_t i = 0; i < sc->nmodels; i++)
        if (sc->models[i].tree && sc->models[i].tree->nnodes > maxn) maxn = sc->models[i].tree->nnodes;
    trav_ws w;
    ws_init(&w, maxn);
    om_counters ctr;
    memset(&ctr, 0, sizeof(ctr));
    for (int64_t i = 0; i < npoints; i++) {
        ov3 po = v3(p[3 * i], p[3 * i + 1], p[3 * i + 2]), n = v3(nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]);
        int ok = ray_valid(po, n);
        invalid[i] = (uint8_t)!ok;
        if (!ok) {
            if (first_sample == 0) {
                sum[3 * i] = sum[3 * i + 1] = sum[3 * i + 2] = 0.0f;
                rgb[3 * i] = rgb[3 * i + 1] = rgb[3 * i + 2] = 0.0f;
                samples[i] = 0;
                ray_casts[i] = 0;
            }
            for (int32_t s = 0; s < nsamples; s++) {
                int64_t k = i * nsamples + s;
                sample_rgb[3 * k] = sample_rgb[3 * k + 1] = sample_rgb[3 * k + 2] = 0.0f;
                dirs[3 * k] = dirs[3 * k + 1] = dirs[3 * k + 2] = 0.0f;
                traced[k] = 0;
                if (sample_casts) sample_casts[k] = 0xFFFFFFFFu;
            }
            continue;
        }
        ov3 col = v3(0, 0, 0);
        uint32_t cnt = 0, casts = 0;
        if (first_sample > 0) {
            col = v3(sum[3 * i], sum[3 * i + 1], sum[3 * i + 2]);
            cnt = samples[i];
            casts = ray_casts[i];
        }
        for (int32_t s = 0; s < nsamples; s++) {
            int64_t k = i * nsamples + s;
            uint64_t st, stream;
            om_path_rng(seed, point_base + i, first_sample + (uint32_t)s, &st, &stream);
            float r0 = rand_bi(&st, stream);
            float r1 = rand_bi(&st, stream);
            float r2 = rand_bi(&st, stream);
            ov3 d = vnormalize(vadd(v3(r0, r1, r2), n));
            int tr = dir_ok(d) && vdot(d, n) > 0.0f;
            dirs[3 * k] = d.x; dirs[3 * k + 1] = d.y; dirs[3 * k + 2] = d.z;
            traced[k] = (uint8_t)tr;
            ov3 c = v3(0, 0, 0);
            uint32_t cc = 0xFFFFFFFFu;
            if (tr) {
                cc = 0;
                c = cast_ray(sc, po, d, bounce_limit, &st, stream, &cc, &w, &ctr);
                col = vadd(col, c);
                casts += cc;
                cnt++;
            }
            sample_rgb[3 * k] = c.x; sample_rgb[3 * k + 1] = c.y; sample_rgb[3 * k + 2] = c.z;
            if (sample_casts) sample_casts[k] = cc;
        }
        sum[3 * i] = col.x; sum[3 * i + 1] = col.y; sum[3 * i + 2] = col.z;
        samples[i] = cnt;
        ray_casts[i] = casts;
        if (cnt) col = vdiv(col, (float)cnt);
        else col = v3(0, 0, 0);
        rgb[3 * i] = col.x; rgb[3 * i + 1] = col.y; rgb[3 * i + 2] = col.z;
    }
    ws_free(&w);
    return (int64_t)ctr.n_rays;
}
