// Test-only entry points (declared in include/yk_test_hooks.h, not in the
// product header; each refuses to run unless YK_DEBUG_HOOKS=1).
//
// yk_debug_qmc_probe runs the device's QMC / FAST_TRIG / rounding functions
// (yk_math.h, the film's round2int / floor2int) and the host-side fExp2 /
// fSin the film's filter tables use, over caller inputs, so that tests can
// compare them with the reference's own functions compiled in the build
// container (tests/golden/ref_qmc.npz, oracle/ref_check.cc).

namespace {

bool debug_hooks_on() {
  const char* e = std::getenv("YK_DEBUG_HOOKS");
  return e && e[0] == '1';
}
// the refusal every entry point opens with, under the entry point's own name
#define YK_HOOK_ONLY \
  if (!debug_hooks_on()) \
  return set_error(YK_ERR_UNSUPPORTED, std::string(__func__) + ": test hook disabled (YK_DEBUG_HOOKS=1)")

__global__ void k_qmc_probe(int fn, const void* in, const uint32_t* in2, long long n, void* out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t* u = (const uint32_t*)in;
  const float* f = (const float*)in;
  const double* dv = (const double*)in;
  float* fo = (float*)out;
  uint32_t* uo = (uint32_t*)out;
  int32_t* io = (int32_t*)out;
  switch (fn) {
    case YK_PROBE_RI_VDC: fo[i] = ri_vdc(u[i], in2[i]); break;
    case YK_PROBE_RI_S: fo[i] = ri_s(u[i], in2[i]); break;
    case YK_PROBE_RI_LP: fo[i] = ri_lp(u[i], in2[i]); break;
    case YK_PROBE_FNV: uo[i] = fnv32a(u[i]); break;
    case YK_PROBE_FSIN: fo[i] = fsin_ref(f[i]); break;
    case YK_PROBE_FCOS: fo[i] = fcos_ref(f[i]); break;
    case YK_PROBE_HALTON2:
    case YK_PROBE_HALTON3:
    case YK_PROBE_HALTON5: {
      const unsigned base = fn == YK_PROBE_HALTON2 ? 2u : (fn == YK_PROBE_HALTON3 ? 3u : 5u);
      Halton h;
      hal_start(h, base, u[i]);
      for (int k = 0; k < 8; ++k) fo[8 * i + k] = hal_next(h);
      break;
    }
    case YK_PROBE_ROUND2INT: io[i] = round2int(dv[i]); break;
    case YK_PROBE_FLOOR2INT: io[i] = floor2int(dv[i]); break;
    default: break;
  }
}

// yk_debug_light_probe: the shading kernels' own light functions (dirac_illum,
// light_illum / spot_illum / sphere_illum / mesh_illum / sun_illum / bg_illum,
// light_hit / spot_hit / sphere_hit / mesh_hit / sun_hit / bg_hit) on light li
// of the bound constants (ml: the handle's mesh-light records, which reach a
// background light's tables too); col as gen_light / gen_sampled form it.
// EMIT_PHOTON: k_photon_emit's emit_photon.
__global__ void k_light_probe(int li, int fn, const float* in, long long n, float* out, const DMeshLight* ml) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const DLight& L = c_lights[li];
  float* o = out + YK_LIGHT_PROBE_STRIDE * i;
  for (int k = 0; k < YK_LIGHT_PROBE_STRIDE; ++k) o[k] = 0.f;
  const c3 lcol = C3(L.color[0], L.color[1], L.color[2]);
  v3 dir = V3(0.f, 0.f, 0.f);
  float tmax = 0.f, pdf = 0.f, cv = 1.f;
  int tri = 0;
  c3 col = C3(0.f, 0.f, 0.f);
  if (L.type == YK_LIGHT_BACKGROUND) {  // per-sample colour, and the sampled or mapped (u, v) beside it
    float u = 0.f, v = 0.f;
    if (fn == YK_LIGHT_PROBE_ILLUM_SAMPLE) {
      const float* x = in + 5 * i;
      bg_illum(L, ml[L.mesh], x[3], x[4], dir, tmax, pdf, col, u, v);
      o[0] = 1.f;
      o[1] = dir.x;
      o[2] = dir.y;
      o[3] = dir.z;
      o[4] = tmax;
      o[5] = col.r;
      o[6] = col.g;
      o[7] = col.b;
      o[8] = pdf;
    } else if (fn == YK_LIGHT_PROBE_INTERSECT) {
      bg_hit(L, ml[L.mesh], ld3(in + 6 * i + 3), pdf, col, u, v);
      o[0] = 1.f;  // t and t_set stay 0: intersect() never writes t
      o[3] = col.r;
      o[4] = col.g;
      o[5] = col.b;
      o[6] = pdf;
    } else {
      return;  // illuminate() is false; emitPhoton is not on the path
    }
    o[YK_LIGHT_PROBE_U] = u;
    o[YK_LIGHT_PROBE_V] = v;
    return;
  }
  if (fn == YK_LIGHT_PROBE_EMIT_PHOTON) {
    const float* x = in + 4 * i;
    if (L.type != YK_LIGHT_AREA && L.type != YK_LIGHT_POINT && L.type != YK_LIGHT_DIRECTIONAL && L.type != YK_LIGHT_SUN)
      return;  // yk_photon_build refuses the others
    v3 from = V3(0.f, 0.f, 0.f);
    col = emit_photon<kXLSun>(L, x[0], x[1], x[2], x[3], from, dir, pdf);
    o[0] = from.x;
    o[1] = from.y;
    o[2] = from.z;
    o[3] = dir.x;
    o[4] = dir.y;
    o[5] = dir.z;
    o[6] = pdf;
    o[7] = col.r;
    o[8] = col.g;
    o[9] = col.b;
    return;
  }
  if (fn == YK_LIGHT_PROBE_ILLUMINATE) {
    const bool dirac = L.type == YK_LIGHT_POINT || L.type == YK_LIGHT_DIRECTIONAL || L.type == YK_LIGHT_SPOT;
    if (!(dirac && dirac_illum(L, ld3(in + 3 * i), dir, tmax, col))) return;
  } else if (fn == YK_LIGHT_PROBE_ILLUM_SAMPLE) {
    const float* x = in + 5 * i;
    bool ok = false;
    if (L.type == YK_LIGHT_AREA) ok = light_illum(L, ld3(x), x[3], x[4], dir, tmax, pdf);
    else if (L.type == YK_LIGHT_SPOT) ok = spot_illum(L, ld3(x), x[3], x[4], dir, tmax, pdf, cv);
    else if (L.type == YK_LIGHT_SPHERE) ok = sphere_illum(L, ld3(x), x[3], x[4], dir, tmax, pdf);
    else if (L.type == YK_LIGHT_MESH) ok = mesh_illum(L, ml[L.mesh], ld3(x), x[3], x[4], dir, tmax, pdf, tri);
    else if (L.type == YK_LIGHT_SUN) ok = sun_illum(L, x[3], x[4], dir, tmax, pdf);
    if (!ok) return;
    col = L.type == YK_LIGHT_SPOT ? cscale(cv, lcol) : lcol;
  } else {
    const float* x = in + 6 * i;
    bool ok = false;
    float t = 0.f;
    if (L.type == YK_LIGHT_AREA) ok = light_hit(L, ld3(x), ld3(x + 3), t, pdf);
    else if (L.type == YK_LIGHT_SPOT) ok = spot_hit(L, ld3(x), ld3(x + 3), t, pdf, cv);
    else if (L.type == YK_LIGHT_SPHERE) ok = sphere_hit(L, ld3(x), ld3(x + 3), pdf);
    else if (L.type == YK_LIGHT_MESH) ok = mesh_hit(L, ml[L.mesh], ld3(x), ld3(x + 3), t, pdf, tri);
    else if (L.type == YK_LIGHT_SUN) ok = sun_hit(L, ld3(x + 3), t, pdf);
    if (!ok) return;
    col = L.type == YK_LIGHT_SPOT ? cscale(cv, lcol) : lcol;
    o[0] = 1.f;
    o[1] = t;
    o[2] = L.type == YK_LIGHT_SPHERE ? 0.f : 1.f;
    o[3] = col.r;
    o[4] = col.g;
    o[5] = col.b;
    o[6] = pdf;
    o[YK_LIGHT_PROBE_TRI] = (float)tri;
    return;
  }
  o[0] = 1.f;
  o[1] = dir.x;
  o[2] = dir.y;
  o[3] = dir.z;
  o[4] = tmax;
  o[5] = col.r;
  o[6] = col.g;
  o[7] = col.b;
  o[8] = pdf;
  o[YK_LIGHT_PROBE_TRI] = (float)tri;
}

// yk_debug_material_probe: mat_eval / mat_sample / mat_pdf with glossy's code
// compiled in (GL), on material mi of the bound constants at a flat surface
// point; fpow_ref and the device library's atanf / tanf on their own
__global__ void k_material_probe(int mi, int fn, const float* in, long long n, float* out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* x = in + YK_MATERIAL_PROBE_IN * i;
  float* o = out + YK_MATERIAL_PROBE_OUT * i;
  for (int k = 0; k < YK_MATERIAL_PROBE_OUT; ++k) o[k] = 0.f;
  if (fn == YK_MATERIAL_PROBE_FPOW) {
    o[0] = fpow_ref(x[0], x[1]);
    o[1] = flog2_ref(x[0]);
    o[2] = fexp2_ref(x[1]);
    return;
  }
  if (fn == YK_MATERIAL_PROBE_ATAN_TAN) {
    o[0] = atanf(x[0]);
    o[1] = tanf(x[0]);
    return;
  }
  const DMat& M = c_mats[mi];
  SurfPt sp{};
  sp.N = sp.Ng = ld3(x);
  sp.mat = mi;
  if (x[19] != 0.f) {
    sp.NU = ld3(x + 13);
    sp.NV = ld3(x + 16);
    if (x[19] == 2.f) sp.Ng = ld3(x + 10);  // a geometric normal of its own
  } else {
    create_cs(sp.N, sp.NU, sp.NV);
  }
  const v3 wo = ld3(x + 3);
  const unsigned flags = (unsigned)x[9];
  if (fn == YK_MATERIAL_PROBE_EVAL) {
    const c3 col = M.type == YK_MAT_GLOSSY          ? glossy_eval(M, sp, wo, ld3(x + 6), flags)
                   : M.type == YK_MAT_COATED_GLOSSY ? coated_eval(M, sp, wo, ld3(x + 6), flags)
                   : M.type == YK_MAT_GLASS         ? mat_eval<true, kGLGlass>(M, sp, wo, ld3(x + 6))
                                                    : mat_eval(M, sp, wo, ld3(x + 6));
    o[0] = col.r;
    o[1] = col.g;
    o[2] = col.b;
  } else if (fn == YK_MATERIAL_PROBE_SAMPLE) {
    v3 wi = V3(0.f, 0.f, 0.f);
    float pdf = 0.f, W = 0.f;
    bool ok;
    unsigned sfl;
    const c3 col = mat_sample<false, kGLGlass>(M, sp, wo, wi, x[6], x[7], flags, pdf, W, ok, sfl);
    o[0] = ok ? 1.f : 0.f;
    o[1] = wi.x;
    o[2] = wi.y;
    o[3] = wi.z;
    o[4] = col.r;
    o[5] = col.g;
    o[6] = col.b;
    o[7] = pdf;
    o[8] = W;
    o[9] = (float)sfl;
  } else if (fn == YK_MATERIAL_PROBE_SPECULAR) {
    bool refl, refr;
    v3 dir[2] = {V3(0.f, 0.f, 0.f), V3(0.f, 0.f, 0.f)};
    c3 col[2] = {C3(0.f, 0.f, 0.f), C3(0.f, 0.f, 0.f)};
    mat_specular<kGLGlass>(M, sp, wo, refl, refr, dir, col, (int)x[9]);
    // a glass with in[8] == 1: the refraction child in the reflection's slots, and the reflection's flag behind it
    const int k = (M.type == YK_MAT_GLASS && x[8] == 1.f) ? 1 : 0;
    o[0] = (k ? refr : refl) ? 1.f : 0.f;
    o[1] = k ? dir[1].x : dir[0].x;
    o[2] = k ? dir[1].y : dir[0].y;
    o[3] = k ? dir[1].z : dir[0].z;
    o[4] = k ? col[1].r : col[0].r;
    o[5] = k ? col[1].g : col[0].g;
    o[6] = k ? col[1].b : col[0].b;
    if (M.type == YK_MAT_GLASS) o[7] = (k ? refl : refr) ? 1.f : 0.f;
    if (M.type == YK_MAT_COATED_GLOSSY) {  // fresnel() on its own, at the face-forwarded normal
      float Kr, Kt;
      fresnel_ref(wo, face_forward(sp.Ng, sp.N, wo), M.gl.ior, Kr, Kt);
      o[7] = Kr;
      o[8] = Kt;
    }
  } else if (fn == YK_MATERIAL_PROBE_TRANSPARENCY) {
    // glossy and coated records have no getTransparency and lie over the shinydiffuse members: zeros
    if (M.type == YK_MAT_SHINYDIFFUSE || M.type == YK_MAT_GLASS) {
      const c3 col = mat_transparency<true>(M, sp, wo);
      o[0] = col.r;
      o[1] = col.g;
      o[2] = col.b;
    }
  } else if (fn == YK_MATERIAL_PROBE_ALPHA) {
    if (M.type == YK_MAT_GLASS) o[0] = glass_alpha(M, sp, wo);
  } else {
    o[0] = M.type == YK_MAT_GLOSSY          ? glossy_pdf(M, sp, wo, ld3(x + 6), flags)
           : M.type == YK_MAT_COATED_GLOSSY ? coated_pdf(M, sp, wo, ld3(x + 6), flags)
           : M.type == YK_MAT_GLASS         ? mat_pdf<kGLGlass>(M, sp, wo, ld3(x + 6))
                                            : mat_pdf(M, sp, wo, ld3(x + 6));
  }
}

// yk_debug_camera_rays: cam_shoot of the bound camera's kind, the function
// k_camera calls, on host-supplied film positions and lens samples
template <int KIND>
__global__ void k_camera_probe(const float* in, long long n, yk_ray* rays, float* wt) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  yk_ray r;
  wt[i] = cam_shoot<KIND>(in[4 * i], in[4 * i + 1], in[4 * i + 2], in[4 * i + 3], r);
  rays[i] = r;
}

}  // namespace

extern "C" int yk_debug_camera_rays(yk_device* d, const float* pxy_lens, int64_t n, yk_ray* rays_out, float* wt_out) {
  YK_HOOK_ONLY;
  if (!d || !pxy_lens || !rays_out || !wt_out || n < 0 || n > (1ll << 24))
    return set_error(YK_ERR_ARG, "yk_debug_camera_rays: bad arguments");
  if (!d->uploaded) return set_error(YK_ERR_STATE, "yk_debug_camera_rays: no scene uploaded");
  if (n == 0) return YK_OK;
  YK_GUARD_BEGIN
  HIPCHK(hipSetDevice(d->ordinal));
  bind_constants(d);
  DBuf<float> din, dwt;
  DBuf<yk_ray> drays;
  din.ensure((size_t)n * 4);
  dwt.ensure((size_t)n);
  drays.ensure((size_t)n);
  HIPCHK(hipMemcpy(din.p, pxy_lens, (size_t)n * 4 * sizeof(float), hipMemcpyHostToDevice));
  auto* kernel = d->cam_host.kind == YK_CAMERA_ORTHOGRAPHIC ? k_camera_probe<YK_CAMERA_ORTHOGRAPHIC>
                 : d->cam_host.kind == YK_CAMERA_ANGULAR    ? k_camera_probe<YK_CAMERA_ANGULAR>
                                                            : k_camera_probe<YK_CAMERA_PERSPECTIVE>;
  hipLaunchKernelGGL(kernel, dim3(grid_for(n)), dim3(256), 0, d->stream, (const float*)din.p, (long long)n, drays.p,
                     dwt.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(d->stream));
  HIPCHK(hipMemcpy(rays_out, drays.p, (size_t)n * sizeof(yk_ray), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(wt_out, dwt.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
  return YK_OK;
  YK_GUARD_END
}

extern "C" int yk_debug_material_probe(yk_device* d, int32_t mat_index, int32_t fn, const float* in, int64_t n,
                                       float* out) {
  YK_HOOK_ONLY;
  if (!d || !in || !out || n < 0 || n > (1ll << 24))
    return set_error(YK_ERR_ARG, "yk_debug_material_probe: bad arguments");
  if (!d->uploaded) return set_error(YK_ERR_STATE, "yk_debug_material_probe: no scene uploaded");
  if (mat_index < 0 || mat_index >= (int32_t)d->mats_host.size())
    return set_error(YK_ERR_ARG, "yk_debug_material_probe: no such material");
  if (fn < YK_MATERIAL_PROBE_EVAL || fn > YK_MATERIAL_PROBE_ALPHA)
    return set_error(YK_ERR_ARG, "yk_debug_material_probe: unknown function");
  if (n == 0) return YK_OK;
  YK_GUARD_BEGIN
  HIPCHK(hipSetDevice(d->ordinal));
  bind_constants(d);
  DBuf<float> din, dout;
  din.ensure((size_t)n * YK_MATERIAL_PROBE_IN);
  dout.ensure((size_t)n * YK_MATERIAL_PROBE_OUT);
  HIPCHK(hipMemcpy(din.p, in, (size_t)n * YK_MATERIAL_PROBE_IN * sizeof(float), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_material_probe, dim3(grid_for(n)), dim3(256), 0, d->stream, (int)mat_index, (int)fn,
                     (const float*)din.p, (long long)n, dout.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(d->stream));
  HIPCHK(hipMemcpy(out, dout.p, (size_t)n * YK_MATERIAL_PROBE_OUT * sizeof(float), hipMemcpyDeviceToHost));
  return YK_OK;
  YK_GUARD_END
}

extern "C" int yk_debug_light_probe(yk_device* d, int32_t light_index, int32_t fn, const float* in, int64_t n,
                                    float* out) {
  YK_HOOK_ONLY;
  if (!d || !in || !out || n < 0 || n > (1ll << 24)) return set_error(YK_ERR_ARG, "yk_debug_light_probe: bad arguments");
  if (!d->uploaded) return set_error(YK_ERR_STATE, "yk_debug_light_probe: no scene uploaded");
  if (light_index < 0 || light_index >= d->nlights)
    return set_error(YK_ERR_ARG, "yk_debug_light_probe: no such light");
  size_t in_f;
  switch (fn) {
    case YK_LIGHT_PROBE_ILLUMINATE: in_f = 3; break;
    case YK_LIGHT_PROBE_ILLUM_SAMPLE: in_f = 5; break;
    case YK_LIGHT_PROBE_INTERSECT: in_f = 6; break;
    case YK_LIGHT_PROBE_EMIT_PHOTON: in_f = 4; break;
    default: return set_error(YK_ERR_ARG, "yk_debug_light_probe: unknown function");
  }
  if (n == 0) return YK_OK;
  YK_GUARD_BEGIN
  HIPCHK(hipSetDevice(d->ordinal));
  bind_constants(d);
  DBuf<float> din, dout;
  din.ensure((size_t)n * in_f);
  dout.ensure((size_t)n * YK_LIGHT_PROBE_STRIDE);
  HIPCHK(hipMemcpy(din.p, in, (size_t)n * in_f * sizeof(float), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_light_probe, dim3(grid_for(n)), dim3(256), 0, d->stream, (int)light_index, (int)fn,
                     (const float*)din.p, (long long)n, dout.p, d->S.ml);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(d->stream));
  HIPCHK(hipMemcpy(out, dout.p, (size_t)n * YK_LIGHT_PROBE_STRIDE * sizeof(float), hipMemcpyDeviceToHost));
  return YK_OK;
  YK_GUARD_END
}

extern "C" int yk_debug_qmc_probe(yk_device* d, int32_t fn, const void* in, const uint32_t* in2, int64_t n,
                                  void* out) {
  YK_HOOK_ONLY;
  if (!in || !out || n < 0 || n > (1ll << 28)) return set_error(YK_ERR_ARG, "yk_debug_qmc_probe: bad arguments");
  const bool ri = fn == YK_PROBE_RI_VDC || fn == YK_PROBE_RI_S || fn == YK_PROBE_RI_LP;
  if (ri && !in2) return set_error(YK_ERR_ARG, "yk_debug_qmc_probe: RI_* need the scramble words");
  size_t in_b = 4, out_b = 4;
  switch (fn) {
    case YK_PROBE_HOST_FEXP2:  // host-side (filter tables), no device needed
      for (int64_t i = 0; i < n; ++i) ((float*)out)[i] = host_fexp2(((const float*)in)[i]);
      return YK_OK;
    case YK_PROBE_HOST_FSIN:
      for (int64_t i = 0; i < n; ++i) ((float*)out)[i] = host_fsin(((const float*)in)[i]);
      return YK_OK;
    case YK_PROBE_RI_VDC: case YK_PROBE_RI_S: case YK_PROBE_RI_LP: case YK_PROBE_FNV:
    case YK_PROBE_FSIN: case YK_PROBE_FCOS: break;
    case YK_PROBE_HALTON2: case YK_PROBE_HALTON3: case YK_PROBE_HALTON5: out_b = 32; break;
    case YK_PROBE_ROUND2INT: case YK_PROBE_FLOOR2INT: in_b = 8; break;
    default: return set_error(YK_ERR_ARG, "yk_debug_qmc_probe: unknown function");
  }
  if (!d) return set_error(YK_ERR_ARG, "yk_debug_qmc_probe: NULL device");
  if (n == 0) return YK_OK;
  YK_GUARD_BEGIN
  HIPCHK(hipSetDevice(d->ordinal));
  DBuf<uint8_t> din, dout;
  DBuf<uint32_t> dr;
  din.ensure((size_t)n * in_b);
  dout.ensure((size_t)n * out_b);
  HIPCHK(hipMemcpy(din.p, in, (size_t)n * in_b, hipMemcpyHostToDevice));
  if (ri) {
    dr.ensure((size_t)n);
    HIPCHK(hipMemcpy(dr.p, in2, (size_t)n * 4, hipMemcpyHostToDevice));
  }
  hipLaunchKernelGGL(k_qmc_probe, dim3(grid_for(n)), dim3(256), 0, d->stream, (int)fn, (const void*)din.p,
                     (const uint32_t*)(ri ? dr.p : nullptr), (long long)n, (void*)dout.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(d->stream));
  HIPCHK(hipMemcpy(out, dout.p, (size_t)n * out_b, hipMemcpyDeviceToHost));
  return YK_OK;
  YK_GUARD_END
}

extern "C" int yk_debug_small_scene(yk_device* d, int64_t* bytes) {
  YK_HOOK_ONLY;
  if (!d || !bytes) return set_error(YK_ERR_ARG, "yk_debug_small_scene: bad arguments");
  if (!d->uploaded) return set_error(YK_ERR_STATE, "yk_debug_small_scene: no scene uploaded");
  *bytes = (d->small && !d->big_leaves) ? (int64_t)d->small_bytes : 0;
  return YK_OK;
}

extern "C" int yk_debug_shading_kind(yk_device* d, int32_t* diff_only) {
  YK_HOOK_ONLY;
  if (!d || !diff_only) return set_error(YK_ERR_ARG, "yk_debug_shading_kind: bad arguments");
  if (!d->uploaded) return set_error(YK_ERR_STATE, "yk_debug_shading_kind: no scene uploaded");
  *diff_only = d->shade.mat == kMatDiffuse ? 1 : 0;
  return YK_OK;
}

extern "C" int yk_debug_shadow_form(yk_device* d, const yk_render_params* p, int32_t* split) {
  YK_HOOK_ONLY;
  if (!d || !p || !split) return set_error(YK_ERR_ARG, "yk_debug_shadow_form: bad arguments");
  if (!d->uploaded) return set_error(YK_ERR_STATE, "yk_debug_shadow_form: no scene uploaded");
  *split = shadow_split(d, p) ? 1 : 0;
  return YK_OK;
}

extern "C" int yk_debug_batch_plan(const yk_batch_plan_in* in, yk_batch_plan* out) {
  YK_HOOK_ONLY;
  if (!in || !out) return set_error(YK_ERR_ARG, "yk_debug_batch_plan: bad arguments");
  if (const char* why = plan_batches(*in, *out)) return set_error(YK_ERR_UNSUPPORTED, why);
  return YK_OK;
}

extern "C" int yk_debug_last_plan(yk_device* d, yk_last_plan* out) {
  YK_HOOK_ONLY;
  if (!d || !out) return set_error(YK_ERR_ARG, "yk_debug_last_plan: bad arguments");
  if (!d->last_plan_valid) return set_error(YK_ERR_STATE, "yk_debug_last_plan: no render yet");
  *out = yk_last_plan{};
  out->plan = d->last_plan;
  out->max_batches_on_pipe = d->last_max_batches;
  // batches go round-robin from pipe 0, so pipe 0 ran the most
  out->pipe_bytes = d->pipe[0].all_bytes();
  out->batch_bytes = d->pipe[0].batch_bytes();
  return YK_OK;
}

// yk_debug_film_splat / yk_debug_depth_splat: host samples through the
// renderer's tile lists (owned_tiles, build_tile_lists) and its gather launch
// (launch_film_gather), in buffers of the call's own. depth: `colours` holds
// one float per sample and the film is {val, weight}.
static int debug_splat(yk_device* d, const yk_render_params* p, int32_t shard, int32_t nshards, int32_t spp,
                       int32_t tiles_per_batch, const uint8_t* flags, const float* colours, const float* offsets,
                       int64_t n, float* film, bool depth) {
  if (!d || !p || !film || n < 0 || n > (1ll << 24) || (n > 0 && (!colours || !offsets)) || nshards < 1 || shard < 0 ||
      shard >= nshards || spp < 1)
    return set_error(YK_ERR_ARG, "yk_debug_film_splat: bad arguments");
  if (p->width <= 0 || p->height <= 0 || (long long)p->width * p->height > (1ll << 24))
    return set_error(YK_ERR_ARG, "yk_debug_film_splat: empty or too large render area");
  if (p->filter < YK_FILTER_BOX || p->filter > YK_FILTER_LANCZOS) return set_error(YK_ERR_ARG, "unknown filter");
  if (!std::isfinite(p->aa_pixelwidth) ||
      (p->filter_width != 0.f && !(p->filter_width >= 0.501f && p->filter_width <= 4.f)))
    return set_error(YK_ERR_ARG, "aa_pixelwidth must be finite, filter_width 0 or in [0.501, 4]");
  if (const int rc = check_tiles(p)) return rc;
  if (flags && (p->xstart + p->width > 65535 || p->ystart + p->height > 65535))
    return set_error(YK_ERR_UNSUPPORTED, "adaptive passes need coordinates < 65536");
  for (int64_t i = 0; i < 2 * n; ++i)
    if (!(offsets[i] >= 0.f && offsets[i] < 1.f))
      return set_error(YK_ERR_ARG, "yk_debug_film_splat: a sample offset outside [0, 1)");
  YK_GUARD_BEGIN
  FilmConst F = make_film(p);
  F.shard = shard;
  F.nshards = nshards;
  F.spp = spp;
  F.d1 = (float)(1.0 / (double)(float)spp);
  F.rank_of = nullptr;
  TileLists L;
  owned_tiles(F, p->tile_order, p->tile_order_len, L);
  const int tpb = tiles_per_batch > 0 ? tiles_per_batch : std::max(1, (int)L.owned.size());
  const int nbatch = (int)((L.owned.size() + (size_t)tpb - 1) / (size_t)tpb);
  build_tile_lists(F, nbatch, tpb, spp, flags, L);
  long long total = 0, maxnc = 1;
  for (const long long nc : L.nc_of) {
    total += nc;
    maxnc = std::max(maxnc, nc);
  }
  if (total != n) return set_error(YK_ERR_ARG, "yk_debug_film_splat: n is not the sample count of the tile lists");
  HIPCHK(hipSetDevice(d->ordinal));
  const size_t nfl = (size_t)F.w * F.h * (depth ? 2 : 5);
  const size_t per = depth ? 1 : 4;  // floats per sample
  DBuf<float> dfilm;
  DBuf<float> dcol;
  DBuf<float2> dxy;
  DBuf<char4> dext;
  DBuf<int> dbase, dpmap, drank;
  dfilm.ensure(nfl);
  dcol.ensure((size_t)maxnc * per);
  dxy.ensure((size_t)maxnc);
  dext.ensure((size_t)maxnc);  // one per pixel slot; maxnc bounds the slots of any spp
  dbase.ensure(std::max<size_t>(1, L.base.size()));
  HIPCHK(hipMemcpy(dfilm.p, film, nfl * sizeof(float), hipMemcpyHostToDevice));
  if (!L.base.empty()) HIPCHK(hipMemcpy(dbase.p, L.base.data(), L.base.size() * sizeof(int), hipMemcpyHostToDevice));
  if (!L.pmap.empty()) {
    dpmap.ensure(L.pmap.size());
    HIPCHK(hipMemcpy(dpmap.p, L.pmap.data(), L.pmap.size() * sizeof(int), hipMemcpyHostToDevice));
  }
  if (!L.rank_of.empty()) {
    drank.ensure(L.rank_of.size());
    HIPCHK(hipMemcpy(drank.p, L.rank_of.data(), L.rank_of.size() * sizeof(int), hipMemcpyHostToDevice));
    F.rank_of = drank.p;
  }
  long long at = 0;
  for (int bi = 0; bi < nbatch; ++bi) {
    const long long nc = L.nc_of[bi];
    const int tb0 = bi * tpb, tb1 = (int)std::min<size_t>(L.owned.size(), (size_t)(bi + 1) * tpb);
    if (nc > 0) {
      // the batch's buffers are reused: the copies wait for the previous gather
      HIPCHK(hipStreamSynchronize(d->stream));
      HIPCHK(hipMemcpy(dcol.p, colours + per * at, (size_t)nc * per * sizeof(float), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(dxy.p, offsets + 2 * at, (size_t)nc * sizeof(float2), hipMemcpyHostToDevice));
    }
    launch_film_gather(d->stream, F, flags ? dpmap.p : nullptr, tb0, tb1, L.rect_of[bi], nc,
                       depth ? nullptr : reinterpret_cast<const float4*>(dcol.p), dxy.p,
                       dbase.p + (size_t)bi * (tpb + 1), dext.p, dfilm.p, film_options(p), depth ? dcol.p : nullptr,
                       depth ? dfilm.p : nullptr);
    at += nc;
  }
  HIPCHK(hipStreamSynchronize(d->stream));
  HIPCHK(hipMemcpy(film, dfilm.p, nfl * sizeof(float), hipMemcpyDeviceToHost));
  return YK_OK;
  YK_GUARD_END
}

extern "C" int yk_debug_film_splat(yk_device* d, const yk_render_params* p, int32_t shard, int32_t nshards, int32_t spp,
                                   int32_t tiles_per_batch, const uint8_t* flags, const float* colours,
                                   const float* offsets, int64_t n, float* film) {
  YK_HOOK_ONLY;
  return debug_splat(d, p, shard, nshards, spp, tiles_per_batch, flags, colours, offsets, n, film, false);
}

extern "C" int yk_debug_depth_splat(yk_device* d, const yk_render_params* p, int32_t shard, int32_t nshards,
                                    int32_t spp, int32_t tiles_per_batch, const uint8_t* flags, const float* depths,
                                    const float* offsets, int64_t n, float* film) {
  YK_HOOK_ONLY;
  return debug_splat(d, p, shard, nshards, spp, tiles_per_batch, flags, depths, offsets, n, film, true);
}

// yk_debug_aa_flags: next_pass_flags, the adaptive passes' own path, on an
// uploaded film. threshold <= 0: no flags exist (doMoreSamples is always
// true), reported as all ones.
extern "C" int yk_debug_aa_flags(yk_device* d, const float* film, int32_t w, int32_t h, float threshold,
                                 uint8_t* flags_out) {
  YK_HOOK_ONLY;
  if (!d || !film || !flags_out || w <= 0 || h <= 0 || (long long)w * h > (1ll << 24))
    return set_error(YK_ERR_ARG, "yk_debug_aa_flags: bad arguments");
  YK_GUARD_BEGIN
  HIPCHK(hipSetDevice(d->ordinal));
  const size_t npx = (size_t)w * h;
  DBuf<float> dfilm;
  dfilm.ensure(npx * 5);
  HIPCHK(hipMemcpy(dfilm.p, film, npx * 5 * sizeof(float), hipMemcpyHostToDevice));
  yk_render_params q{};
  q.width = w;
  q.height = h;
  q.aa_threshold = threshold;
  std::vector<uint8_t> host_flags;
  const uint8_t* fl = next_pass_flags(d, dfilm.p, &q, host_flags);
  if (fl) std::memcpy(flags_out, fl, npx);
  else std::memset(flags_out, 1, npx);
  return YK_OK;
  YK_GUARD_END
}

// ---------------------------------------------------------------------------
// include/yk_test_hooks_photon.h: the photon-map lookups on a synthetic map.
// yk_debug_photon_load takes yk_photon_build's steps from the kd-tree build
// on; the probe kernels call pm_gather / pm_nearest, the functions k_pregather,
// k_pm_post and caustic_estimate call; yk_debug_photon_lookup_queue launches
// the production k_pm_lookup the way enqueue_photon_mapping does.

namespace {

__global__ void __launch_bounds__(64) k_photon_gather_probe(PMapDev M, const float* __restrict__ pos,
                                                            const float* __restrict__ r2, long long nq, int K,
                                                            int* __restrict__ count, int* __restrict__ idx,
                                                            float* __restrict__ d2, float* __restrict__ r2_out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nq) return;
  PFound f[kMaxSearch];
  const v3 p = V3(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]);
  float radius = r2[i];
  const int ng = M.n > 0 ? pm_gather(M, p, f, K, radius) : 0;  // the guard of k_pm_post / k_pm_finish
  count[i] = ng;
  r2_out[i] = radius;
  for (int k = 0; k < ng; ++k) {
    idx[i * K + k] = f[k].idx;
    d2[i * K + k] = f[k].d2;
  }
}

__global__ void __launch_bounds__(64) k_photon_nearest_probe(PMapDev M, const float* __restrict__ pos,
                                                             const float* __restrict__ nrm,
                                                             const float* __restrict__ r2, long long nq,
                                                             int* __restrict__ nearest) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nq) return;
  const v3 p = V3(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]);
  const v3 n = V3(nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]);
  nearest[i] = M.n > 0 ? pm_nearest(M, p, n, r2[i]) : -1;
}

bool photon_slot_ok(int32_t which) {
  return which == YK_PHOTON_MAP_DIFFUSE || which == YK_PHOTON_MAP_CAUSTIC || which == YK_PHOTON_MAP_RADIANCE;
}

// the PMapDev pm_const hands the render kernels for this slot
PMapDev debug_map(const yk_device* d, int32_t which) {
  if (which == YK_PHOTON_MAP_RADIANCE)
    return PMapDev{d->rm_nodes.p, d->rm_pos.p, d->rm_dir.p, d->rm_col.p, (int)(d->rm_host.size() / 9), d->rm_pk.p};
  if (which == YK_PHOTON_MAP_CAUSTIC)
    return PMapDev{d->cm_nodes.p, d->cm_pos.p, d->cm_dir.p, d->cm_col.p, (int)(d->cm_host.size() / 9)};
  return PMapDev{d->dm_nodes.p, d->dm_pos.p, d->dm_dir.p, d->dm_col.p, (int)(d->dm_host.size() / 9)};
}

constexpr int64_t kProbeMaxQueries = 1ll << 24;
constexpr int64_t kProbeMaxRecords = 1ll << 26;  // nq * K of one gather call
constexpr int64_t kProbeMaxQueue = 1ll << 25;

// photonGather_t::operator() (photon.cc:53-73) over libstdc++'s own heap functions
struct HostFound {
  int idx;
  float d2;
  bool operator<(const HostFound& o) const { return d2 < o.d2; }
};
struct HostGather {
  HostFound* f;
  int k, n;
  void operator()(int d, float dist2, float& maxd2) {
    if (n < k) {
      f[n++] = HostFound{d, dist2};
      if (n == k) {
        std::make_heap(f, f + k);
        maxd2 = f[0].d2;
      }
    } else {
      std::pop_heap(f, f + k);
      f[k - 1] = HostFound{d, dist2};
      std::push_heap(f, f + k);
      maxd2 = f[0].d2;
    }
  }
};
// nearestPhoton_t::operator(), photon.h:167-176
struct HostNearest {
  const float* photons;
  const float* n;
  int nearest;
  void operator()(int d, float dist2, float& maxd2) {
    const float* w = photons + 9 * (size_t)d + 3;
    if (w[0] * n[0] + w[1] * n[1] + w[2] * n[2] > 0.f) {
      nearest = d;
      maxd2 = dist2;
    }
  }
};

}  // namespace

extern "C" int yk_debug_photon_load(yk_device* d, int32_t which, const float* photons, int32_t n, int32_t depth_limit,
                                    yk_photon_map_info* info) {
  YK_HOOK_ONLY;
  if (!d || !photon_slot_ok(which) || n < 0 || n > (1 << 24) || (n > 0 && !photons))
    return set_error(YK_ERR_ARG, "yk_debug_photon_load: bad arguments");
  YK_GUARD_BEGIN
  HIPCHK(hipSetDevice(d->ordinal));
  std::vector<float> ph(photons, photons + 9 * (size_t)n);
  PointTree t;
  point_tree_build(ph.data(), 9, n, t);
  const int limit = (depth_limit > 0 && depth_limit < kMaxPointTreeDepth) ? depth_limit : kMaxPointTreeDepth;
  if (t.depth > limit) return set_error(YK_ERR_UNSUPPORTED, "yk_debug_photon_load: photon tree too deep");
  HIPCHK(hipStreamSynchronize(d->stream));
  d->pm_ready = false;  // the slots no longer hold what pm_params describes
  const bool radiance = which == YK_PHOTON_MAP_RADIANCE;
  std::vector<float>& host = radiance ? d->rm_host : (which == YK_PHOTON_MAP_CAUSTIC ? d->cm_host : d->dm_host);
  host.swap(ph);
  if (radiance) {
    d->rm_depth = t.depth;
    d->rm_nnodes = t.nodes.size() / 2;
  }
  upload_map(d, which, host, t);
  if (radiance && lookup_lds(d)) {
    int blocks = 0;
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, k_pm_lookup<true>, 64, lookup_lds_bytes(d->rm_depth)));
    d->per_cu_lookup[1] = std::max(1, blocks);
  }
  if (info) {
    *info = yk_photon_map_info{};
    info->photons = n;
    info->nodes = (int32_t)(t.nodes.size() / 2);
    info->depth = t.depth;
    if (radiance) {
      const bool lds = lookup_lds(d);
      info->lookup_lds = lds ? 1 : 0;
      info->lookup_grid = (int32_t)((long long)d->cus * d->per_cu_lookup[lds]);
    }
  }
  return YK_OK;
  YK_GUARD_END
}

extern "C" int yk_debug_photon_gather(yk_device* d, int32_t which, const float* pos, const float* r2, int64_t nq,
                                      int32_t K, int32_t* count, int32_t* idx, float* d2, float* r2_out) {
  YK_HOOK_ONLY;
  if (!d || !photon_slot_ok(which) || nq < 0 || nq > kProbeMaxQueries ||
      (nq > 0 && (!pos || !r2 || !count || !idx || !d2 || !r2_out)))
    return set_error(YK_ERR_ARG, "yk_debug_photon_gather: bad arguments");
  if (K < 1 || K > kMaxSearch) return set_error(YK_ERR_UNSUPPORTED, "search must be in [1, 256]");
  if (nq * K > kProbeMaxRecords) return set_error(YK_ERR_ARG, "yk_debug_photon_gather: too many records");
  if (nq == 0) return YK_OK;
  YK_GUARD_BEGIN
  HIPCHK(hipSetDevice(d->ordinal));
  const size_t n = (size_t)nq, nk = n * (size_t)K;
  DBuf<float> dpos, dr2, dd2, dr2o;
  DBuf<int> dcnt, didx;
  dpos.ensure(3 * n);
  dr2.ensure(n);
  dr2o.ensure(n);
  dcnt.ensure(n);
  didx.ensure(nk);
  dd2.ensure(nk);
  HIPCHK(hipMemcpy(dpos.p, pos, 3 * n * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dr2.p, r2, n * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(hipMemsetAsync(didx.p, 0xFF, nk * sizeof(int), d->stream));
  HIPCHK(hipMemsetAsync(dd2.p, 0xFF, nk * sizeof(float), d->stream));
  launch(k_photon_gather_probe, grid_for(nq, 64), 64, 0, d->stream, debug_map(d, which), (const float*)dpos.p,
         (const float*)dr2.p, (long long)nq, (int)K, dcnt.p, didx.p, dd2.p, dr2o.p);
  HIPCHK(hipStreamSynchronize(d->stream));
  HIPCHK(hipMemcpy(count, dcnt.p, n * sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(idx, didx.p, nk * sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(d2, dd2.p, nk * sizeof(float), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(r2_out, dr2o.p, n * sizeof(float), hipMemcpyDeviceToHost));
  return YK_OK;
  YK_GUARD_END
}

extern "C" int yk_debug_photon_nearest(yk_device* d, int32_t which, const float* pos, const float* nrm,
                                       const float* r2, int64_t nq, int32_t* nearest) {
  YK_HOOK_ONLY;
  if (!d || !photon_slot_ok(which) || nq < 0 || nq > kProbeMaxQueries || (nq > 0 && (!pos || !nrm || !r2 || !nearest)))
    return set_error(YK_ERR_ARG, "yk_debug_photon_nearest: bad arguments");
  if (nq == 0) return YK_OK;
  YK_GUARD_BEGIN
  HIPCHK(hipSetDevice(d->ordinal));
  const size_t n = (size_t)nq;
  DBuf<float> dpos, dnrm, dr2;
  DBuf<int> dout;
  dpos.ensure(3 * n);
  dnrm.ensure(3 * n);
  dr2.ensure(n);
  dout.ensure(n);
  HIPCHK(hipMemcpy(dpos.p, pos, 3 * n * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dnrm.p, nrm, 3 * n * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dr2.p, r2, n * sizeof(float), hipMemcpyHostToDevice));
  launch(k_photon_nearest_probe, grid_for(nq, 64), 64, 0, d->stream, debug_map(d, which), (const float*)dpos.p,
         (const float*)dnrm.p, (const float*)dr2.p, (long long)nq, dout.p);
  HIPCHK(hipStreamSynchronize(d->stream));
  HIPCHK(hipMemcpy(nearest, dout.p, n * sizeof(int), hipMemcpyDeviceToHost));
  return YK_OK;
  YK_GUARD_END
}

extern "C" int yk_debug_photon_lookup_queue(yk_device* d, const float* lq, int64_t nq, float rad2,
                                            int32_t force_scratch, float* lcol, int64_t ncol, int32_t* lds_out,
                                            int32_t* grid_out) {
  YK_HOOK_ONLY;
  if (!d || nq < 0 || nq > kProbeMaxQueue || ncol < 0 || ncol > 3 * kProbeMaxQueue || (nq > 0 && !lq) ||
      (ncol > 0 && !lcol))
    return set_error(YK_ERR_ARG, "yk_debug_photon_lookup_queue: bad arguments");
  if (d->rm_host.empty() || d->rm_nnodes == 0)
    return set_error(YK_ERR_STATE, "yk_debug_photon_lookup_queue: the radiance slot is empty");
  for (int64_t q = 0; q < nq; ++q) {  // k_pm_lookup writes lcol[3 * owner .. + 2] unchecked
    int32_t owner;
    std::memcpy(&owner, &lq[8 * q + 3], sizeof owner);
    if (owner < 0 || 3 * (int64_t)owner + 2 >= ncol)
      return set_error(YK_ERR_ARG, "yk_debug_photon_lookup_queue: an owner outside the colour array");
  }
  YK_GUARD_BEGIN
  HIPCHK(hipSetDevice(d->ordinal));
  DBuf<float4> dlq;
  DBuf<float> dcol;
  DBuf<unsigned long long> words;  // [0] the queue's count word, [1] the hand-out's work word
  dlq.ensure(std::max<size_t>(1, 2 * (size_t)nq));
  dcol.ensure(std::max<size_t>(1, (size_t)ncol));
  words.ensure(2);
  const unsigned long long w[2] = {(unsigned long long)nq, 0ull};
  if (nq > 0) HIPCHK(hipMemcpy(dlq.p, lq, (size_t)nq * 8 * sizeof(float), hipMemcpyHostToDevice));
  if (ncol > 0) HIPCHK(hipMemcpy(dcol.p, lcol, (size_t)ncol * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(words.p, w, sizeof w, hipMemcpyHostToDevice));
  const PMapDev rmap = debug_map(d, YK_PHOTON_MAP_RADIANCE);
  const bool lds = !force_scratch && lookup_lds(d);
  const unsigned grid = (unsigned)((long long)d->cus * d->per_cu_lookup[lds]);
  launch(lds ? k_pm_lookup<true> : k_pm_lookup<false>, grid, 64, lds ? lookup_lds_bytes(d->rm_depth) : 0, d->stream,
         rmap, rad2, d->rm_depth, (const float4*)dlq.p, (const unsigned long long*)words.p, dcol.p, words.p + 1);
  HIPCHK(hipStreamSynchronize(d->stream));
  if (ncol > 0) HIPCHK(hipMemcpy(lcol, dcol.p, (size_t)ncol * sizeof(float), hipMemcpyDeviceToHost));
  if (lds_out) *lds_out = lds ? 1 : 0;
  if (grid_out) *grid_out = (int32_t)grid;
  return YK_OK;
  YK_GUARD_END
}

extern "C" int yk_debug_photon_host_tree(const float* photons, int32_t n, uint32_t* nodes, int64_t cap_nodes,
                                         int32_t* nnodes, int32_t* depth) {
  YK_HOOK_ONLY;
  if (n < 0 || n > (1 << 24) || (n > 0 && !photons) || cap_nodes < 0 || (cap_nodes > 0 && !nodes) || !nnodes || !depth)
    return set_error(YK_ERR_ARG, "yk_debug_photon_host_tree: bad arguments");
  YK_GUARD_BEGIN
  PointTree t;
  point_tree_build(photons, 9, n, t);
  const size_t nn = t.nodes.size() / 2;
  *nnodes = (int32_t)nn;
  *depth = t.depth;
  const size_t take = std::min<size_t>(nn, (size_t)cap_nodes);
  if (take) std::memcpy(nodes, t.nodes.data(), take * 2 * sizeof(uint32_t));
  return YK_OK;
  YK_GUARD_END
}

extern "C" int yk_debug_photon_host_gather(const float* photons, int32_t n, const float* pos, const float* r2,
                                           int64_t nq, int32_t K, int32_t* count, int32_t* idx, float* d2,
                                           float* r2_out) {
  YK_HOOK_ONLY;
  if (n < 0 || n > (1 << 24) || (n > 0 && !photons) || nq < 0 || nq > kProbeMaxQueries ||
      (nq > 0 && (!pos || !r2 || !count || !idx || !d2 || !r2_out)))
    return set_error(YK_ERR_ARG, "yk_debug_photon_host_gather: bad arguments");
  if (K < 1 || K > kMaxSearch) return set_error(YK_ERR_UNSUPPORTED, "search must be in [1, 256]");
  YK_GUARD_BEGIN
  PointTree t;
  point_tree_build(photons, 9, n, t);
  if (t.depth > kMaxPointTreeDepth) return set_error(YK_ERR_UNSUPPORTED, "photon tree too deep");
  std::vector<HostFound> f((size_t)K);
  for (int64_t q = 0; q < nq; ++q) {
    HostGather g{f.data(), K, 0};
    float radius = r2[q];
    if (n > 0) point_tree_lookup(t, photons, 9, pos + 3 * q, g, radius);
    count[q] = g.n;
    r2_out[q] = radius;
    for (int k = 0; k < K; ++k) {
      idx[q * K + k] = k < g.n ? f[k].idx : -1;
      if (k < g.n) d2[q * K + k] = f[k].d2;
      else std::memset(&d2[q * K + k], 0xFF, sizeof(float));
    }
  }
  return YK_OK;
  YK_GUARD_END
}

extern "C" int yk_debug_photon_host_nearest(const float* photons, int32_t n, const float* pos, const float* nrm,
                                            const float* r2, int64_t nq, int32_t* nearest) {
  YK_HOOK_ONLY;
  if (n < 0 || n > (1 << 24) || (n > 0 && !photons) || nq < 0 || nq > kProbeMaxQueries ||
      (nq > 0 && (!pos || !nrm || !r2 || !nearest)))
    return set_error(YK_ERR_ARG, "yk_debug_photon_host_nearest: bad arguments");
  YK_GUARD_BEGIN
  PointTree t;
  point_tree_build(photons, 9, n, t);
  if (t.depth > kMaxPointTreeDepth) return set_error(YK_ERR_UNSUPPORTED, "photon tree too deep");
  for (int64_t q = 0; q < nq; ++q) {
    HostNearest pr{photons, nrm + 3 * q, -1};
    float radius = r2[q];
    if (n > 0) point_tree_lookup(t, photons, 9, pos + 3 * q, pr, radius);
    nearest[q] = pr.nearest;
  }
  return YK_OK;
  YK_GUARD_END
}
