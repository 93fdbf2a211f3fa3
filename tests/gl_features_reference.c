/*
 * gl_features_reference.c -- TEST INFRASTRUCTURE ONLY: the first-hit features of a GL-shaded frame (pt_set_shading_features,
 * DESIGN 3.8b), restated on glshade_reference.c's own camera constants (ctx_open) and its own hitWorld (hit_world), with no
 * product header.
 *
 * For pixel (x, y), pass p < k and stratum j = 0 .. 15, in (p, j) order from zero: the camera ray of path 16 p + j as the shader's
 * main makes it (stream (seed ^ "GL_SHADE", pixel, 16 p + j), two jitter draws, at most 16 tries of randomInUnitSphere when the lens
 * is open, the normalised direction); its first hit hitWorld(o, d, 0.001, 1e20) with nothing skipped.  A hit adds the record's
 * face-forward normal to fn, the hit material's albedo (after the host packing, emissive materials included) to fa, t to fd[0] and 1
 * to fd[1]; every path adds 1 to fd[2].  ids = the object of (p = 0, j = 0), -1 on a miss.  Only passes below `passes` exist.
 *
 *   glf_features  the planes and ids of a frame
 *   glf_classes   what the first hits of that frame were: {paths, sphere hits, plane hits, box hits, back-face hits, misses}
 */
#include "glshade_reference.c"

/* the camera ray of path (pass, j) of pixel (x, y): main's, gpu.go:1685-1718 with buildCamera :1110-1124 */
static void glf_ray(gr_ctx *c, int x, int y, uint32_t pass, int j, double o[3], double d[3]) {
    const int sy = j / 4, sx = j % 4;
    const uint64_t pix = (uint64_t)y * (uint64_t)c->w + (uint64_t)x;
    uint64_t st = ora_stream_init(c->seed ^ GR_SALT, pix, (uint64_t)pass * 16u + (uint64_t)j);
    const double jx = ora_stream_next(&st), jy = ora_stream_next(&st);
    const double su = ((double)sx + jx) / 4.0, sv = ((double)sy + jy) / 4.0;
    const double u = ((double)x + su) / (double)(c->w - 1);
    const double v = ((double)(c->h - 1 - y) + sv) / (double)(c->h - 1);
    double off[3] = {0, 0, 0};
    if (c->lens > 0.0) {
        double p[3] = {0, 0, 1};
        for (int t = 0; t < 16; t++) {
            const double a = ora_stream_next(&st), b = ora_stream_next(&st), e = ora_stream_next(&st);
            const double q[3] = {2.0 * a - 1.0, 2.0 * b - 1.0, 2.0 * e - 1.0};
            if (dot(q, q) >= 1.0) continue;
            memcpy(p, q, sizeof p);
            break;
        }
        const double rx = c->lens * p[0], ry = c->lens * p[1];
        for (int i = 0; i < 3; i++) off[i] = c->cam_u[i] * rx + c->cam_vv[i] * ry;
        for (int i = 0; i < 3; i++) {
            d[i] = c->cam_llc[i] + u * c->cam_h[i] + v * c->cam_v[i] - c->cam_origin[i] - off[i];
            o[i] = c->cam_origin[i] + off[i];
        }
    } else {
        for (int i = 0; i < 3; i++) {
            d[i] = c->cam_llc[i] + u * c->cam_h[i] + v * c->cam_v[i] - c->cam_origin[i];
            o[i] = c->cam_origin[i];
        }
    }
    vnorm(d);
}

static void glf_frame(const ora_scene *sc, const gr_extra *ex, int32_t w, int32_t h, int32_t passes, int32_t k, uint64_t seed, double *fn,
                      double *fa, double *fd, int32_t *ids, uint64_t cls[6]) {
    gr_ctx c;
    ctx_open(&c, sc, ex, w, h, 1, seed, NULL);
    const int take = k < passes ? k : passes;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const size_t i = (size_t)y * (size_t)w + (size_t)x;
            double n[3] = {0, 0, 0}, a[3] = {0, 0, 0}, z[3] = {0, 0, 0};
            int id = -1;
            for (int p = 0; p < take; p++)
                for (int j = 0; j < 16; j++) {
                    double o[3], d[3];
                    gr_hit hit;
                    glf_ray(&c, x, y, (uint32_t)p, j, o, d);
                    const int any = hit_world(&c, o, d, 0.001, 1e20, -1, &hit);
                    if (p == 0 && j == 0) id = any ? hit.obj : -1;
                    if (cls) cls[0]++;
                    if (any) {
                        const gr_mat *m = &c.mats[hit.mat];
                        for (int q = 0; q < 3; q++) {
                            n[q] += hit.normal[q];
                            a[q] += m->albedo[q];
                        }
                        z[0] += hit.t;
                        z[1] += 1.0;
                        if (cls) {
                            cls[1 + c.objs[hit.obj].typ]++;
                            if (!hit.front) cls[4]++;
                        }
                    } else if (cls) {
                        cls[5]++;
                    }
                    z[2] += 1.0;
                }
            if (fn) memcpy(fn + 3 * i, n, sizeof n);
            if (fa) memcpy(fa + 3 * i, a, sizeof a);
            if (fd) memcpy(fd + 3 * i, z, sizeof z);
            if (ids) ids[i] = take > 0 ? id : -1;
        }
    ctx_close(&c);
}

void glf_features(const ora_scene *sc, const gr_extra *ex, int32_t w, int32_t h, int32_t passes, int32_t k, uint64_t seed, double *fn,
                  double *fa, double *fd, int32_t *ids) {
    glf_frame(sc, ex, w, h, passes, k, seed, fn, fa, fd, ids, NULL);
}

/* (gr_obj.typ: 0 sphere, 1 plane, 2 box -- so cls[1] spheres, cls[2] planes, cls[3] boxes) */
void glf_classes(const ora_scene *sc, const gr_extra *ex, int32_t w, int32_t h, int32_t passes, int32_t k, uint64_t seed, uint64_t cls[6]) {
    memset(cls, 0, 6 * sizeof(uint64_t));
    glf_frame(sc, ex, w, h, passes, k, seed, NULL, NULL, NULL, NULL, cls);
}
