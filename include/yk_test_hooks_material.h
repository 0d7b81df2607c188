/* yk_test_hooks_material.h -- test-only probe of the materials' device
 * functions. Like yk_test_hooks.h it is NOT part of the product ABI
 * (include/yk_api.h), and the hook refuses to run (YK_ERR_UNSUPPORTED) unless
 * the process environment has YK_DEBUG_HOOKS=1. */
#ifndef YK_TEST_HOOKS_MATERIAL_H
#define YK_TEST_HOOKS_MATERIAL_H
#include "yk_api.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Runs, in a kernel on `d`, the device functions the shading kernels call for
 * material `mat_index` of the resident scene (shinydiffuse, light_mat or
 * glossy, coated glossy or glass) at a flat surface point, over n host-supplied inputs. Every input
 * is YK_MATERIAL_PROBE_IN floats, every output YK_MATERIAL_PROBE_OUT floats,
 * zero where nothing is listed. The surface point is sp.Ng = sp.N = N; its
 * tangents are createCS(N) when in[19] is 0, and NU = in[13..15],
 * NV = in[16..18] otherwise. Flags travel as floats holding the integer.
 *   EVAL    in: N[0..2], wo[3..5], wl[6..8], bsdfs[9]    -> col[0..2]
 *           (bsdfs reaches glossy's eval; shinydiffuse's takes none)
 *   SAMPLE  in: N[0..2], wo[3..5], s1[6], s2[7], flags[9]
 *           -> ok[0], wi[1..3], col[4..6], pdf[7], W[8], sampledFlags[9];
 *           wi and W start at zero, so an early return shows them untouched
 *   PDF     in: N[0..2], wo[3..5], wi[6..8], flags[9]    -> pdf[0]
 *           (flags reaches glossy's pdf; shinydiffuse's takes none)
 *   FPOW    in: a[0], b[1]  -> fPow(a, b)[0], fLog2(a)[1], fExp2(b)[2]
 *   ATAN_TAN in: x[0]       -> atanf(x)[0], tanf(x)[1] of the device library,
 *           which sample_quadrant_aniso calls
 *   SPECULAR in: N[0..2], wo[3..5], raylevel[9] (state.raylevel after
 *           recursiveRaytrace's increment: 1 at a camera hit)
 *           -> refl[0], dir[1..3], col[4..6] of the material's getSpecular
 *           reflection (zero where it reflects nothing); for a coated glossy
 *           material also fresnel()'s Kr[7], Kt[8] at FACE_FORWARD(Ng, N, wo)
 *           For a glass material in[8] chooses the child: 0 the reflection as
 *           above, 1 the refraction, refr[0], dir[1..3], col[4..6]; [7] is then
 *           the other child's flag (refr beside the reflection, refl beside
 *           the refraction)
 *   TRANSPARENCY in: N[0..2], wo[3..5] -> getTransparency(sp, wo)[0..2] of a
 *           shinydiffuse or glass material (the transparent-shadow leaf body);
 *           zero for every other kind
 *   ALPHA   in: N[0..2], wo[3..5] -> a glass material's getAlpha[0]; 0 for
 *           every other kind
 * For a glass material EVAL gives black and PDF 0, and SAMPLE reads s1 only.
 * FPOW and ATAN_TAN read no material; mat_index must still be valid.
 * With in[19] == 2 the tangents are given as above and the geometric normal
 * is sp.Ng = in[10..12], so that N and Ng can disagree about wo's side. */
enum { YK_MATERIAL_PROBE_EVAL = 0, YK_MATERIAL_PROBE_SAMPLE = 1, YK_MATERIAL_PROBE_PDF = 2,
       YK_MATERIAL_PROBE_FPOW = 3, YK_MATERIAL_PROBE_ATAN_TAN = 4, YK_MATERIAL_PROBE_SPECULAR = 5,
       YK_MATERIAL_PROBE_TRANSPARENCY = 6, YK_MATERIAL_PROBE_ALPHA = 7 };
enum { YK_MATERIAL_PROBE_IN = 20, YK_MATERIAL_PROBE_OUT = 10 };
int yk_debug_material_probe(yk_device* d, int32_t mat_index, int32_t fn, const float* in, int64_t n, float* out);

#ifdef __cplusplus
}
#endif
#endif /* YK_TEST_HOOKS_MATERIAL_H */
