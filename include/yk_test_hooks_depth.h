/* yk_test_hooks_depth.h -- test-only entry point into the depth gather, the
 * ordered walk that runs imageFilm_t::addDepthSample (imagefilm.cc:513-564).
 * Like yk_test_hooks_film.h it is NOT part of the product ABI
 * (include/yk_api.h), and the hook refuses to run (YK_ERR_UNSUPPORTED) unless
 * the process environment has YK_DEBUG_HOOKS=1. It needs no uploaded scene. */
#ifndef YK_TEST_HOOKS_DEPTH_H
#define YK_TEST_HOOKS_DEPTH_H
#include "yk_api.h"
#ifdef __cplusplus
extern "C" {
#endif

/* yk_debug_film_splat's inputs (yk_test_hooks_film.h) with one float per
 * sample in place of a colour -- a NaN means the sample has no depth value
 * (an angular camera's sample without a ray) and adds neither value nor
 * weight -- and a film of width*height*{val, weight} floats, copied in, added
 * to and copied back. The same refusals, before anything is launched. */
int yk_debug_depth_splat(yk_device* d, const yk_render_params* p, int32_t shard, int32_t nshards, int32_t spp,
                         int32_t tiles_per_batch, const uint8_t* flags, const float* depths, const float* offsets,
                         int64_t n, float* film);

#ifdef __cplusplus
}
#endif
#endif /* YK_TEST_HOOKS_DEPTH_H */
