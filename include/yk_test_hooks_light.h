/* yk_test_hooks_light.h -- test-only probe of the lights' device functions.
 * Like yk_test_hooks.h it is NOT part of the product ABI (include/yk_api.h),
 * and the hook refuses to run (YK_ERR_UNSUPPORTED) unless the process
 * environment has YK_DEBUG_HOOKS=1. */
#ifndef YK_TEST_HOOKS_LIGHT_H
#define YK_TEST_HOOKS_LIGHT_H
#include "yk_api.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Runs, in a kernel on `d`, the device functions the shading kernels call
 * for light `light_index` of the resident scene, over n host-supplied inputs
 * (`in`: floats per input as listed). `out` gets YK_LIGHT_PROBE_STRIDE floats
 * per input, laid out as listed and zero where the function wrote nothing
 * (ok = 0 or 1 as a float; a refused sample leaves its record at zero):
 *   ILLUMINATE    in: P[3]             -> ok, dir[3], tmax, col[3]
 *                 light_t::illuminate: point, directional and spot lights
 *                 (a spot light answers whether or not it has soft shadows);
 *                 ok = 0 for the others, as their illuminate() returns false
 *   ILLUM_SAMPLE  in: P[3], s1, s2     -> ok, dir[3], tmax, col[3], pdf
 *                 light_t::illumSample: area, spot, sphere, mesh, sun and
 *                 background lights
 *   INTERSECT     in: from[3], dir[3]  -> ok, t, t_set, col[3], ipdf
 *                 light_t::intersect: area, spot, sphere, mesh and sun lights;
 *                 t_set = 0 for a sphere light, whose intersect() never writes
 *                 t (spherelight.cc:134-149), and for a background light,
 *                 whose intersect() does not either (bglight.cc:191-206: t
 *                 reads 0 here); a sun writes t = -1
 *   EMIT_PHOTON   in: s1, s2, s3, s4   -> from[3], dir[3], ipdf, col[3]
 *                 light_t::emitPhoton as k_photon_emit runs it: area, point,
 *                 directional and sun lights (the kinds yk_photon_build
 *                 accepts); a zero record for the others. There is no ok
 *                 field: emitPhoton always answers.
 * col is ls.col / lcol as doLightEstimation receives it. A mesh light also
 * writes out[YK_LIGHT_PROBE_TRI]: the index, in the light's own triangle
 * order, of the triangle ILLUM_SAMPLE sampled or INTERSECT hit, as a float
 * (0 for the other kinds). Its ILLUMINATE answers ok = 0.
 * A background light also writes out[YK_LIGHT_PROBE_U] and
 * out[YK_LIGHT_PROBE_V]: the (u, v) CalcFromSample drew (ILLUM_SAMPLE) or
 * spheremap gave the direction (INTERSECT), both in [0, 1]; the fields are
 * zero for every other kind. Its col is the background evaluated at
 * invSpheremap(u, v); its ILLUMINATE and EMIT_PHOTON records are zero. */
enum { YK_LIGHT_PROBE_ILLUMINATE = 0, YK_LIGHT_PROBE_ILLUM_SAMPLE = 1, YK_LIGHT_PROBE_INTERSECT = 2,
       YK_LIGHT_PROBE_EMIT_PHOTON = 3 };
enum { YK_LIGHT_PROBE_STRIDE = 12, YK_LIGHT_PROBE_TRI = 11, YK_LIGHT_PROBE_U = 9, YK_LIGHT_PROBE_V = 10 };
int yk_debug_light_probe(yk_device* d, int32_t light_index, int32_t fn, const float* in, int64_t n, float* out);

#ifdef __cplusplus
}
#endif
#endif /* YK_TEST_HOOKS_LIGHT_H */
