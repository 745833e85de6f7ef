/* The occlusion query's reference (atr_occluded_rays): the oracle's own traversal with
   `closest` started at the ray's t_max instead of MAX_FLOAT -- how a user of the reference casts a
   shadow ray. The oracle stays as it is; its static helpers (check_aabb, get_aabb, scan_leaf,
   mt_culled, sphere_hit, plane_hit, ws_init) are reached by including its source.
   Built by tests/occlusion_ref.py with the oracle Makefile's flags. */
#include "../../oracle/atr_oracle.c"

/* tree_intersect (atr_oracle.c:452-497) with closest = tmax. Returns 1 iff scan_leaf ever returns 1:
   some triangle of a leaf the reference's DFS reaches has 1e-4 < t < tmax. A leaf whose hits are
   all >= tmax does not end the walk; the first leaf that improves does (the answer is known).
   *found: the t that leaf left in closest (a witness below tmax, not the nearest hit). */
static int tree_occluded(const om_tree* t, const oray* r, trav_ws* w, float tmax, float* found) {
    float closest = tmax;
    uint32_t face = 0;
    float u = 0, v = 0;
    int occ = 0;
    const om_node* N = t->nodes;
    if (!check_aabb(r, N[0].bmin, N[0].bmax)) return 0;
    if (N[0].children == 0) {
        occ = scan_leaf(t, &N[0], r, &closest, &face, &u, &v, NULL);
        if (occ) *found = closest;
        return occ;
    }
    leafpair* lf = w->leaf + 1;
    w->leaf[0].node = -1; w->leaf[0].dist = -OM_MAX_FLOAT;
    int32_t nleaf = 0, nhit = 1;
    w->hit[0] = 0;
    while (nhit > 0) {
        int32_t cur = w->hit[--nhit];
        int32_t ch = N[cur].children;
        int nodes_hit = 0;
        for (int i = 0; i < 8 && nodes_hit <= 4; i++, ch++) {
            const om_node* c = &N[ch];
            if (c->children) {
                if (check_aabb(r, c->bmin, c->bmax)) { nodes_hit++; w->hit[nhit++] = ch; }
            } else {
                float dis = get_aabb(r, c->bmin, c->bmax);
                if (dis > 0.0f) {
                    nodes_hit++;
                    if (nleaf == 0) { lf[0].node = ch; lf[0].dist = dis; nleaf++; }
                    else {
                        int32_t e = nleaf - 1;
                        while (dis < lf[e].dist) { lf[e + 1] = lf[e]; e--; }
                        lf[e + 1].node = ch; lf[e + 1].dist = dis;
                        nleaf++;
                    }
                }
            }
        }
    }
    for (int32_t j = 0; j < nleaf; j++) {
        if (scan_leaf(t, &N[lf[j].node], r, &closest, &face, &u, &v, NULL)) { occ = 1; break; }
    }
    if (occ) *found = closest;
    return occ;
}

/* out: 0 visible, 1 occluded, 2 invalid t_max (NaN, zero or negative; +inf counts as MAX_FLOAT).
   The rays themselves are the caller's to validate (atr_trace_rays' test). t_max NULL: unbounded.
   t_found (optional): a t with 1e-4 < t < t_max for an occluded ray, else MAX_FLOAT. */
void ref_occluded(const om_scene* s, const float* o, const float* d, const float* t_max, int64_t n,
                  uint8_t* out, float* t_found) {
    int32_t mx = 0;
    for (int32_t i = 0; i < s->nmodels; i++)
        if (s->models[i].tree && s->models[i].tree->nnodes > mx) mx = s->models[i].tree->nnodes;
    trav_ws w;
    ws_init(&w, mx);
    for (int64_t k = 0; k < n; k++) {
        float T = t_max ? t_max[k] : OM_MAX_FLOAT;
        if (t_found) t_found[k] = OM_MAX_FLOAT;
        if (!(T > 0.0f)) { out[k] = 2; continue; }
        if (T > OM_MAX_FLOAT) T = OM_MAX_FLOAT;
        ov3 ro = v3(o[3 * k], o[3 * k + 1], o[3 * k + 2]), rd = v3(d[3 * k], d[3 * k + 1], d[3 * k + 2]);
        oray r; r.o = ro; r.d = rd;
        r.inv = v3(1 / rd.x, 1 / rd.y, 1 / rd.z);
        r.s[0] = r.inv.x < 0; r.s[1] = r.inv.y < 0; r.s[2] = r.inv.z < 0;
        int occ = 0;
        float found = OM_MAX_FLOAT;
        for (int32_t i = 0; i < s->nspheres && !occ; i++) {
            float t = sphere_hit(ro, rd, &s->spheres[i]);
            if (t > OM_TOL && t < T) { occ = 1; found = t; }
        }
        for (int32_t i = 0; i < s->nplanes && !occ; i++) {
            float t = plane_hit(ro, rd, &s->planes[i]);
            if (t > OM_TOL && t < T) { occ = 1; found = t; }
        }
        for (int32_t i = 0; i < s->nmodels && !occ; i++) {
            const om_model* md = &s->models[i];
            if (md->tree) {
                occ = tree_occluded(md->tree, &r, &w, T, &found);
            } else if (get_aabb(&r, md->surrounding_aabb, md->surrounding_aabb + 3) != 0) {
                const om_mesh* m = md->mesh;
                for (uint32_t j = 0; j < m->nf && !occ; j++) {
                    float u = 0, v = 0;
                    float t = mt_culled(ro, rd, m->vertices[m->face_v[3 * j]], m->vertices[m->face_v[3 * j + 1]],
                                        m->vertices[m->face_v[3 * j + 2]], &u, &v);
                    if (t > OM_TOL && t < T) { occ = 1; found = t; }
                }
            }
        }
        out[k] = (uint8_t)occ;
        if (t_found && occ) t_found[k] = found;
    }
    ws_free(&w);
}
