/* object_ids_reference.c -- independent CPU restatement of the object index plane (pt_set_object_ids, include/ptcore.h), on the
 * oracle: ora_primary_ray makes sample 0's ray of every pixel, ora_hit tests it against the scene's objects in file order with the
 * first-segment loop's own rule (renderer.go:297-302: tmin 0.001, tmax = the closest t so far, a hit replaces the winner).  The
 * index is the one into the scene's object list: an object of unknown type keeps its place in the count and is never tested.  Built
 * at test time (tests/temporal_motion_support.py) with the oracle's flags.  Nothing here is shared with the product's headers or
 * with atrous_reference.c. */
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "pt_oracle.h"

/* ora_hit's view of scene object o: 0 when the type is unknown */
static int oid_shape(const ora_object *o, int32_t *kind, double a[3], double b[3], double *radius) {
    *radius = 0;
    for (int k = 0; k < 3; k++) a[k] = b[k] = 0;
    if (o->type == 0 || o->type == 3) {
        *kind = 0;
        for (int k = 0; k < 3; k++) a[k] = o->position[k];
        *radius = o->size[0];
        return 1;
    }
    if (o->type == 1) {
        *kind = 1;
        for (int k = 0; k < 3; k++) a[k] = o->position[k];
        b[1] = 1;
        return 1;
    }
    if (o->type == 2) {
        *kind = 2;
        for (int k = 0; k < 3; k++) {
            a[k] = o->position[k] - o->size[k] * 0.5;
            b[k] = o->position[k] + o->size[k] * 0.5;
        }
        return 1;
    }
    return 0;
}

/* The winner of one ray, or -1; *tie = 1 when another object's own nearest hit lies within 1e-9 (relative) of the winner's, so that
 * the order of the list, not the geometry, chose. */
static int32_t oid_one(const ora_scene *sc, const double o[3], const double d[3], uint8_t *tie) {
    double closest = DBL_MAX;
    int32_t best = -1;
    for (int32_t i = 0; i < sc->nobjects; i++) {
        int32_t kind;
        double a[3], b[3], radius, rec[8];
        if (!oid_shape(&sc->objects[i], &kind, a, b, &radius)) continue;
        if (ora_hit(kind, a, b, radius, o, d, 0.001, closest, rec)) {
            closest = rec[0];
            best = i;
        }
    }
    *tie = 0;
    if (best < 0) return best;
    for (int32_t i = 0; i < sc->nobjects; i++) {
        int32_t kind;
        double a[3], b[3], radius, rec[8];
        if (i == best || !oid_shape(&sc->objects[i], &kind, a, b, &radius)) continue;
        if (ora_hit(kind, a, b, radius, o, d, 0.001, DBL_MAX, rec) && fabs(rec[0] - closest) <= 1e-9 * (closest > 1 ? closest : 1)) *tie = 1;
    }
    return best;
}

/* ids, tie: [H][W], of sample 0 of every pixel of the frame */
void oid_frame(const ora_scene *sc, const ora_config *cfg, int32_t *ids, uint8_t *tie) {
    for (int32_t y = 0; y < cfg->height; y++)
        for (int32_t x = 0; x < cfg->width; x++) {
            const size_t i = (size_t)y * (size_t)cfg->width + (size_t)x;
            double o[3], d[3];
            ora_primary_ray(sc, cfg, x, y, 0, o, d);
            ids[i] = oid_one(sc, o, d, &tie[i]);
        }
}

/* the same of n chosen rays [n][6] (origin, direction) */
void oid_rays(const ora_scene *sc, int64_t n, const double *rays, int32_t *ids, uint8_t *tie) {
    for (int64_t i = 0; i < n; i++) ids[i] = oid_one(sc, rays + 6 * i, rays + 6 * i + 3, &tie[i]);
}
