/* yk_test_hooks_film.h -- test-only entry points into the film stage: the
 * ordered gather that runs imageFilm_t::addSample, and imageFilm_t::nextPass.
 * Like yk_test_hooks.h it is NOT part of the product ABI (include/yk_api.h),
 * and the hooks refuse to run (YK_ERR_UNSUPPORTED) unless the process
 * environment has YK_DEBUG_HOOKS=1. Neither needs an uploaded scene. */
#ifndef YK_TEST_HOOKS_FILM_H
#define YK_TEST_HOOKS_FILM_H
#include "yk_api.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Splats n host-supplied samples into a host film with the renderer's own
 * tile lists and its extent + gather launches (one stream, batch after batch).
 *
 * Read from p: the render area (xstart, ystart, width, height), tile_size,
 * filter, aa_pixelwidth / filter_width, tile_order, and premult_alpha /
 * clamp_rgb (the gather's compile-time variants). The pass is that of
 * shard `shard` of `nshards` with spp samples per pixel in batches of
 * tiles_per_batch owned tiles (<= 0: all of them in one batch). flags is NULL,
 * or width*height bytes (film-local, row-major) of an adaptive pass: only
 * pixels with a non-zero byte have samples.
 *
 * colours (n x 4 floats, RGBA) and offsets (n x 2 floats, the sample's dx, dy
 * inside its pixel) come in the film's own order: the shard's tiles in the
 * order the film hands them out, the (flagged) pixels of a tile row-major,
 * spp samples per pixel. film (width*height*5 floats: the RGBA sums and the
 * weight of every pixel) is copied in, added to and copied back.
 *
 * YK_ERR_ARG, before anything is launched, when n is not the sample count
 * those lists imply, when a dx or dy lies outside [0, 1) (the gather's source
 * windows assume that range), or when the filter or its width is not one the
 * film accepts. All device memory used is the call's own: the handle's batch
 * buffers and its record of the last render's plan stay as they were. */
int yk_debug_film_splat(yk_device* d, const yk_render_params* p, int32_t shard, int32_t nshards, int32_t spp,
                        int32_t tiles_per_batch, const uint8_t* flags, const float* colours, const float* offsets,
                        int64_t n, float* film);

/* imageFilm_t::nextPass's flags for a host film of w*h*5 floats, through the
 * path the adaptive passes use, into flags_out (w*h bytes, 0 or 1). With
 * threshold <= 0 every byte is 1: doMoreSamples is then always true and the
 * renderer computes no flags at all. */
int yk_debug_aa_flags(yk_device* d, const float* film, int32_t w, int32_t h, float threshold, uint8_t* flags_out);

#ifdef __cplusplus
}
#endif
#endif /* YK_TEST_HOOKS_FILM_H */
