// Host side of the film (included by yk_device.hip after
// yk_upload_host.inc): the filter functions in the reference's compiled
// forms (host_fexp2, filter_gauss, filter_lanczos), make_film, which fills
// the FilmConst of yk_film.inc from the render parameters, and
// yk_film_filter_from_table. Depends on FilmConst, on yk_math.h (host_fsin,
// YK_PI_D) and on set_error only.

extern "C" {

// Filter functions of imageFilm_t (imagefilm.cc:81-123), in the survey
// build's compiled forms: Gauss folds -6*log2(e) into one constant and drops
// fExp2's upper clamp (the argument is never positive); Lanczos2 uses the
// FAST_TRIG fSin (yk::host_fsin) on (float)(x*pi) and (float)(x*pi/2).
// fExp2, mathOptimizations.h:100-114 (POLYEXP :85); pinned bit for bit to
// the reference's own fExp2 compiled in the build container
// (oracle/ref_check.cc, tests/test_ref_pinning.py through yk_debug_qmc_probe)
static float host_fexp2(float x) {
  x = (x < 129.00000f) ? x : 129.00000f;    // f_HI
  x = (x > -126.99999f) ? x : -126.99999f;  // f_LOW
  const int ip = (int)(x - 0.5f);
  const float fp = x - (float)ip;
  const uint32_t eb = (uint32_t)(ip + 127) << 23;
  float e;
  std::memcpy(&e, &eb, 4);
  const float poly = ((((1.8775767e-3f * fp + 8.9893397e-3f) * fp + 5.5826318e-2f) * fp + 2.4015361e-1f) * fp +
                      6.9315308e-1f) * fp + 9.9999994e-1f;
  return e * poly;
}
static float filter_gauss(float dx, float dy) {
  const float r2 = dx * dx + dy * dy;
  float k;
  const uint32_t kbits = 0xc10a7facu;  // (float)(-6 * (float)M_LOG2E)
  std::memcpy(&k, &kbits, 4);
  // r2 * k <= 0: the upper clamp the compiled form drops is a no-op
  const float v = (float)((double)host_fexp2(r2 * k) - 0.00247875);
  return (v > 0.f) ? v : 0.f;
}
static float filter_lanczos(float dx, float dy) {
  const float x = std::sqrt(dx * dx + dy * dy);
  if (x == 0.f) return 1.f;
  if (!(x > -2.f) || !(x < 2.f)) return 0.f;
  const float a = (float)((double)x * YK_PI_D);
  const float b = (float)((double)x * (YK_PI_D * 0.5));
  return (host_fsin(b) * host_fsin(a)) / (a * b);
}

static FilmConst make_film(const yk_render_params* p) {
  FilmConst F{};
  F.cx0 = p->xstart;
  F.cy0 = p->ystart;
  F.w = p->width;
  F.h = p->height;
  F.cx1 = p->xstart + p->width;
  F.cy1 = p->ystart + p->height;
  F.tile = p->tile_size > 0 ? p->tile_size : 32;
  F.ntx = (p->width + F.tile - 1) / F.tile;
  float fw = (float)((double)p->aa_pixelwidth * 0.5);
  if (p->filter == YK_FILTER_MITCHELL) fw *= 2.6f;
  else if (p->filter == YK_FILTER_GAUSS) fw *= 2.f;
  if (fw < 0.501f) fw = 0.501f;
  if (fw > 4.f) fw = 4.f;
  if (p->filter_width > 0.f) fw = p->filter_width;  // the live film's filterw (yk_film_filter_from_table)
  F.filterw = fw;
  F.tableScale = 0.9999 * 16 / F.filterw;
  auto r2i = [](double v) { return (int)(v + (0.5 - 1.4e-11)); };
  // target - source offsets reachable by Round2Int extents for dx in [0,1)
  F.olo_x = F.olo_y = r2i(0.0 - fw);
  F.ohi_x = F.ohi_y = r2i(1.0 + fw - 1.0);
  const float scale = 1.f / 16.f;
  for (int y = 0; y < 16; ++y)
    for (int x = 0; x < 16; ++x) {
      const float fx = (x + .5f) * scale, fy = (y + .5f) * scale;
      float v = 1.f;
      if (p->filter == YK_FILTER_MITCHELL) {
        const float xx = 2.f * std::sqrt(fx * fx + fy * fy);
        if (xx >= 2.f) v = 0.f;
        else if (xx >= 1.f) v = (float)(xx * (xx * (xx * -0.38888889f + 2.0f) - 3.33333333f) + 1.77777778f);
        else v = (float)(xx * xx * (1.16666666f * xx - 2.0f) + 0.88888889f);
      } else if (p->filter == YK_FILTER_GAUSS) {
        v = filter_gauss(fx, fy);
      } else if (p->filter == YK_FILTER_LANCZOS) {
        v = filter_lanczos(fx, fy);
      }
      F.table[y * 16 + x] = v;
    }
  F.spp = p->aa_samples > 0 ? p->aa_samples : 1;
  F.d1 = (float)(1.0 / (double)(float)F.spp);
  return F;
}

int yk_film_filter_from_table(const float* table, float filterw, yk_render_params* p) {
  if (!table || !p) return set_error(YK_ERR_ARG, "yk_film_filter_from_table: NULL argument");
  if (!(filterw >= 0.501f && filterw <= 4.f))
    return set_error(YK_ERR_UNSUPPORTED, "film filterw outside [0.501, 4] (imagefilm.cc:150)");
  for (int f : {YK_FILTER_BOX, YK_FILTER_MITCHELL, YK_FILTER_GAUSS, YK_FILTER_LANCZOS}) {
    yk_render_params q = *p;
    q.filter = f;
    const FilmConst F = make_film(&q);
    if (std::memcmp(F.table, table, sizeof F.table) == 0) {
      p->filter = f;
      p->filter_width = filterw;
      return YK_OK;
    }
  }
  return set_error(YK_ERR_UNSUPPORTED, "film filter table is none of box / Mitchell / Gauss / Lanczos2");
}

}  // extern "C"
