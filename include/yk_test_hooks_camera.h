/* yk_test_hooks_camera.h -- test-only probe of the cameras' device ray
 * generators. Like yk_test_hooks.h it is NOT part of the product ABI
 * (include/yk_api.h), and the hook refuses to run (YK_ERR_UNSUPPORTED) unless
 * the process environment has YK_DEBUG_HOOKS=1. */
#ifndef YK_TEST_HOOKS_CAMERA_H
#define YK_TEST_HOOKS_CAMERA_H
#include "yk_api.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Runs, in a kernel on `d`, the device shootRay of the resident scene's
 * camera -- the function k_camera calls for that camera kind -- on n
 * host-supplied inputs of four floats each: the film position px, py and the
 * lens sample lu, lv (read by a perspective or architect camera with an
 * aperture only). rays_out gets n rays, wt_out n weights: 1, or 0 for an
 * angular camera's sample outside its circle, whose ray is then the one
 * k_camera stores for such a sample (from = position, dir = 0, tmin = 0,
 * tmax = -1) and is never traced. */
int yk_debug_camera_rays(yk_device* d, const float* pxy_lens, int64_t n, yk_ray* rays_out, float* wt_out);

#ifdef __cplusplus
}
#endif
#endif /* YK_TEST_HOOKS_CAMERA_H */
