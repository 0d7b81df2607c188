// The scene's background as a function of direction, and bgLight_t, the light
// that samples it (included by yk_device.hip after the other lights' sample
// and intersect functions). Depends on yk_math.h (fsin_ref / fcos_ref), v3 /
// c3 and the DLight / DMeshLight records.

// RenderConst::has_bg / DLight::bg.kind (scene.h's YK_BG_*)
constexpr int kBgNone = 0, kBgConstant = 1, kBgGradient = 2;

// gradientBackground_t::eval (gradientback.cc:60-79) in source order; g =
// szenith, shoriz, gzenith, ghoriz (each times power). A colour whose
// smallest channel is below 1e-6f becomes color_t(1e-5f).
__device__ __forceinline__ c3 bg_gradient(const float* g, v3 dir) {
  float blend = dir.z;
  if (!(blend >= 0.f)) {
    blend = -blend;
    g += 6;
  }
  c3 c = C3(blend * g[0] + (1.f - blend) * g[3], blend * g[1] + (1.f - blend) * g[4],
            blend * g[2] + (1.f - blend) * g[5]);
  if (fminf(c.r, fminf(c.g, c.b)) < 1e-6f) c = C3(1e-5f, 1e-5f, 1e-5f);
  return c;
}

// background_t::eval: constBackground_t answers its colour whatever the ray
__device__ __forceinline__ c3 bg_eval(int kind, const float* constant, const float* grad, v3 dir) {
  if (kind == kBgGradient) return bg_gradient(grad, dir);
  return C3(constant[0], constant[1], constant[2]);
}

// A background light's tables (bgLight_t::init), packed by make_bg_light into
// one run of 32-bit words behind DMeshLight::cdf, nv = DMeshLight::n rows:
// count[nv] and offset[nv] (ints: uDist[y]->count, the row's first element in
// func_u), invIntegral[nv], vDist's func[nv] and cdf[nv + 1], then the rows'
// func back to back and their cdfs (count + 1 entries each) back to back.
struct BgTables {
  const int* count;
  const int* offset;
  const float* inv_integral;
  const float* func_v;
  const float* cdf_v;
  const float* func_u;
  const float* cdf_u;
  int nv;
};
__device__ __forceinline__ BgTables bg_tables(const DMeshLight& R, const DLight& L) {
  BgTables T;
  const int nv = R.n;
  T.nv = nv;
  T.count = reinterpret_cast<const int*>(R.cdf);
  T.offset = T.count + nv;
  T.inv_integral = R.cdf + 2 * nv;
  T.func_v = R.cdf + 3 * nv;
  T.cdf_v = R.cdf + 4 * nv;
  T.func_u = R.cdf + 5 * nv + 1;
  T.cdf_u = T.func_u + L.bg.total_u;
  return T;
}

// pdf1D_t::Sample (sample_utils.h:123-138): std::lower_bound over
// cdf[0..count] (the first entry >= u), minus 1, clamped at 0; index + delta.
// cdf[count] is exactly 1 (integral / integral), so a u below 1 -- every
// sample the integrators draw -- ends inside the table; a u above it would
// make the reference read past the arrays, which this does not follow: the
// index stops at the last segment.
__device__ __forceinline__ float pdf1d_sample(const float* func, const float* cdf, int count, float inv_integral,
                                              float u, float& pdf) {
  int lo = 0, len = count + 1;
  while (len > 0) {  // std::lower_bound
    const int half = len >> 1;
    if (cdf[lo + half] < u) {
      lo += half + 1;
      len -= half + 1;
    } else {
      len = half;
    }
  }
  int index = lo - 1;
  if (index < 0) index = 0;
  if (index > count - 1) index = count - 1;
  const float delta = (u - cdf[index]) / (cdf[index + 1] - cdf[index]);
  pdf = func[index] * inv_integral;
  return (float)index + delta;
}

// bglight.cc:37-53: clampSample, sinSample, clampZero, calcPdf / calcInvPdf
// with sigma = 0.000001f. std::max(sigma, x) answers sigma unless sigma < x.
__device__ __forceinline__ int bg_clamp_sample(float s, int m) { return max(0, min((int)s, m - 1)); }
__device__ __forceinline__ float bg_sin_sample(float s) { return fsin_ref((float)((double)s * YK_PI_D)); }
__device__ __forceinline__ float bg_clamp_zero(float v) { return v > 0.f ? 1.f / v : 0.f; }
__device__ __forceinline__ float bg_calc_pdf(float p0, float p1, float s) {
  const float x = ((p0 * p1) * (float)0.15915494309189533577) * bg_clamp_zero(bg_sin_sample(s));
  return 0.000001f < x ? x : 0.000001f;
}
__device__ __forceinline__ float bg_calc_inv_pdf(float p0, float p1, float s) {
  const float x = ((float)YK_2PI_D * bg_sin_sample(s)) * bg_clamp_zero(p0 * p1);
  return 0.000001f < x ? x : 0.000001f;
}

// invSpheremap (texture.h:93-102): theta = v * M_PI and phi = -(u * M_2PI)
// are double products stored to float
__device__ __forceinline__ v3 inv_spheremap(float u, float v) {
  const float theta = (float)((double)v * YK_PI_D);
  const float phi = (float)-((double)u * YK_2PI_D);
  const float costheta = fcos_ref(theta), sintheta = fsin_ref(theta);
  const float cosphi = fcos_ref(phi), sinphi = fsin_ref(phi);
  return V3(sintheta * cosphi, sintheta * sinphi, -costheta);
}

// fAcos (mathOptimizations.h:282-288): the two range guards, then the double
// acos of the float argument narrowed to float (which overload the
// reference's build picked is not pinned: DESIGN.md)
__device__ __forceinline__ float facos_ref(float x) {
  if ((double)x <= -1.0) return (float)YK_PI_D;
  if ((double)x >= 1.0) return 0.f;
  return (float)acos((double)x);
}

// spheremap (texture.h:73-90): the products with M_1_2PI / M_1_PI and the
// difference from M_2PI are double; phiRatio is stored to float before
// u = 1.f - phiRatio, v is the double 1.f - (...) stored to float
__device__ __forceinline__ void spheremap(v3 p, float& u, float& v) {
  const float sqrtRPhi = p.x * p.x + p.y * p.y;
  const float sqrtRTheta = sqrtRPhi + p.z * p.z;
  u = 0.f;
  v = 0.f;
  if (sqrtRPhi > 0.f) {
    float phiRatio;
    const double a = (double)facos_ref(p.x / sqrtf(sqrtRPhi));
    if (p.y < 0.f) phiRatio = (float)((YK_2PI_D - a) * 0.15915494309189533577);
    else phiRatio = (float)(a * 0.15915494309189533577);
    u = 1.f - phiRatio;
  }
  v = (float)((double)1.f - (double)facos_ref(p.z / sqrtf(sqrtRTheta)) * YK_1_PI_D);
}

// bgLight_t::illumSample (bglight.cc:175-189) through CalcFromSample
// (:120-137): v from vDist, the row clampSample(v + 0.4999f, count) -- it
// rounds, it does not floor --, u from that row, both scaled by invCount
// (1.f / count), the pdf from calcPdf at the scaled v. tmax = -1: unbounded.
// col = eval of the sampled direction. Always true. (u, v) go to the light
// probe.
__device__ __forceinline__ bool bg_illum(const DLight& L, const DMeshLight& R, float s1, float s2, v3& ldir,
                                         float& tmax, float& pdf, c3& col, float& u, float& v) {
  const BgTables T = bg_tables(R, L);
  float pdf1 = 0.f, pdf2 = 0.f;
  v = pdf1d_sample(T.func_v, T.cdf_v, T.nv, L.bg.v_inv_integral, s2, pdf2);
  const int iv = bg_clamp_sample(v + 0.4999f, T.nv);
  const int cnt = T.count[iv], off = T.offset[iv];
  u = pdf1d_sample(T.func_u + off, T.cdf_u + off + iv, cnt, T.inv_integral[iv], s1, pdf1);
  u *= 1.f / (float)cnt;
  v *= 1.f / (float)T.nv;
  pdf = bg_calc_pdf(pdf1, pdf2, v);
  tmax = -1.f;
  ldir = inv_spheremap(u, v);
  col = bg_eval(L.bg.kind, L.color, L.bg.grad, ldir);
  return true;
}

// bgLight_t::intersect (bglight.cc:191-206) through CalcFromDir (:139-156):
// the direction negated first under abs_intersect, mapped to (u, v), the
// rounded row and column, ipdf from calcInvPdf; the colour is evaluated at
// invSpheremap(u, v), not at the ray's own direction. t is never written: the
// caller's ray stays unbounded. Always true.
__device__ __forceinline__ bool bg_hit(const DLight& L, const DMeshLight& R, v3 dir, float& ipdf, c3& col, float& u,
                                       float& v) {
  const BgTables T = bg_tables(R, L);
  if (L.bg.abs_inter) dir = vneg(dir);
  spheremap(dir, u, v);
  const int iv = bg_clamp_sample(v * (float)T.nv + 0.4999f, T.nv);
  const int cnt = T.count[iv], off = T.offset[iv];
  const int iu = bg_clamp_sample(u * (float)cnt + 0.4999f, cnt);
  const float pdf1 = T.func_u[off + iu] * T.inv_integral[iv];
  const float pdf2 = T.func_v[iv] * L.bg.v_inv_integral;
  ipdf = bg_calc_inv_pdf(pdf1, pdf2, v);
  col = bg_eval(L.bg.kind, L.color, L.bg.grad, inv_spheremap(u, v));
  return true;
}
