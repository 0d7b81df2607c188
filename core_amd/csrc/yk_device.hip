// MI355X (gfx950) device half of libyk: scene upload, persistent kd-tree
// traversal kernels, the wavefront path-integrator pipeline and the
// deterministic image-film gather. Host entry points are the C-ABI of
// include/yk_api.h.
//
// Reference behaviour restated here:
//   triKdTree_t::Intersect / IntersectS      src/yafraycore/kdtree.cc:675-947
//   bound_t::cross                           include/core_api/bound.h:148-204
//   scene_t::intersect / isShadowed          src/yafraycore/scene.cc:852-902
//   pathIntegrator_t::integrate              src/integrators/pathtracer.cc:134-333
//   directLighting_t::integrate              src/integrators/directlight.cc:112-182
//   mcIntegrator_t::doLightEstimation        src/yafraycore/mcintegrator.cc:45-195
//   tiledIntegrator_t::renderTile            src/yafraycore/integrator.cc:229-339
//   imageFilm_t::addSample / flush           src/yafraycore/imagefilm.cc:383-511
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <climits>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <type_traits>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/yk_api.h"
#include "../../include/yk_test_hooks.h"
#include "../../include/yk_test_hooks_light.h"
#include "../../include/yk_test_hooks_camera.h"
#include "../../include/yk_test_hooks_film.h"
#include "../../include/yk_test_hooks_depth.h"
#include "../../include/yk_test_hooks_material.h"
#include "../../include/yk_test_hooks_photon.h"
#include "photon_map.h"
#include "scene.h"
#include "yk_internal.h"
#include "yk_math.h"

struct yk_scene {
  yk::Scene s;
};

namespace yk {

__constant__ QmcTables c_qmc;
__constant__ int c_faure[5600];

// ------------------------------------------------------------ device data

struct DMat {
  int type;
  unsigned flags;
  float col[3];       // diffuse colour (shinydiffuse) / lightCol = col*power (light_mat)
  float emit_col[3];  // mEmitColor = emit * color (shinydiffuse.cc:12)
  int double_sided;
  // The record keeps its size and the shinydiffuse members their offsets (the
  // shading kernels hold all kMaxMats records in LDS): a glossy material's
  // members lie over the shinydiffuse ones, which it does not have.
  union {
    struct {  // shinyDiffuseMat_t after config() (shinydiffuse.cc:27-80)
      float comp[4];      // getComponents: mirror, transparency, translucency, diffuse
      float mirror[3];    // mMirrorColor
      int ncomp;          // nBSDF
      unsigned cflags[4]; // cFlags
      int cindex[4];      // cIndex
      float tfilter;      // mTransmitFilterStrength
      int fresnel;        // mHasFresnelEffect
      float ior2;         // mIOR_Squared
      int translucent;    // mIsTranslucent
    };
    struct {  // glossyMat_t (glossy.cc:56-62) with as_diffuse; col above is gloss_color
      float diff[3];      // diff_color
      float exponent, exp_u, exp_v;
      float m_glossy;     // MDat_t::mGlossy = reflectivity (no shader node)
      float m_diffuse;    // mDiffuse
      float p_diffuse;    // MDat_t::pDiffuse (glossy.cc:94), constant without nodes
      int with_diffuse, anisotropic;
      // coatedGlossyMat_t (coatedglossy.cc:63-77) holds the same members and two more,
      // in words the glossy half left free; unread for YK_MAT_GLOSSY
      float mirror[3];    // mirror_color
      float ior;          // IOR
    } gl;
    struct {  // glassMat_t (glass.cc:44-52) without nodes, dispersion or absorption; col above is unused
      float filter[3];    // filterCol
      float mirror[3];    // specRefCol
      float ior;          // ior
      int fake_shadow;    // fakeShadow: tmFlags is FILTER|TRANSMIT, else SPECULAR|TRANSMIT
    } gs;
  };
  int on;             // mUseOrenNayar (shinydiffuse.cc:170-176) / glossyMat_t::orenNayar
  float on_a, on_b;   // mOrenNayar_A / mOrenNayar_B, orenA / orenB
};
static_assert(sizeof(DMat) == 32 * sizeof(int), "DMat: the shading kernels' LDS copy is sized by it");

struct DLight {  // areaLight_t members after its constructor (arealight.cc:30-49)
  // The record keeps its size and every member its offset: a background
  // light's own members lie over the area light's corners, which it has not.
  union {
    struct {
      float corner[3], toX[3], toY[3], fnormal[3], c2[3], c3[3], c4[3];
    };
    // bgLight_t (bglight.h:58-66) and the background it is bound to: kind
    // (kBgConstant: `color` below holds constBackground_t::color; kBgGradient:
    // grad = szenith, shoriz, gzenith, ghoriz), absInter, vDist->invIntegral and
    // the tables' sum of row counts; the tables themselves lie behind
    // DScene::ml[mesh].cdf (bg_tables). samples, soft = 1 (light_sampled) and,
    // from init(scene), epos = worldCenter, wradius = worldRadius, area = aPdf.
    struct {
      float grad[12];
      int kind, abs_inter;
      float v_inv_integral;
      int total_u;
    } bg;
  };
  float color[3];
  float e2[3], e3[3], e4[3];  // c2 - corner, c3 - corner, c4 - corner: intersect()'s triangle edges
  float area;
  int samples;
  int type;    // YK_LIGHT_*; point / directional are Dirac lights (mcintegrator.cc:85-100)
  int nslots;  // shadow slots per doLightEstimation: 2*samples (area + MIS half), 1 (Dirac)
  float pos[3], dir[3], radius;  // pointLight_t / directionalLight_t members
  int infinite;
  float normal[3], du[3], dv[3];  // areaLight_t emitPhoton frame: normal = -fnormal, du = |toX|, dv = normal ^ du
  // directionalLight_t after init(scene) (directional.cc:52-75): photon disk
  // centre / radius (infinite: scene-bound centre and world radius), createCS frame
  float epos[3], edu[3], edv[3], eradius, wradius;
  // spotLight_t members (spotlight.cc:46-60): pos = position, dir, du / dv =
  // createCS(dir) (the area light's fields, unused by a spot), and
  float ndir[3], cos_start, cos_end, icos_diff, fuzzy;
  int soft;         // softShadows: illumSample + intersect instead of illuminate
  int photon_only;  // illuminate / illumSample return false
  // sphereLight_t members (spherelight.cc:56-61): pos = center, radius, area, and
  float sq_radius, sq_radius_eps;
  // meshLight_t members (meshlight.h:56-64): area (above), doubleSided, and
  // the light's record in DScene::ml (cdf, triangles, normals, its own tree)
  int double_sided;
  int mesh;
  // sunLight_t members (sunlight.cc:42-49): dir = direction, du / dv, samples,
  // and, after init(scene), epos = worldCenter, wradius = worldRadius. `color`
  // holds colPdf -- what illumSample and intersect hand doLightEstimation as
  // ls.col / lcol, which is what the sampling loops and resolve_light read
  // there -- and sun_color the member `color` (totalEnergy). soft = 1 puts the
  // light among the sampled ones (light_sampled). cosAngle is a double, held
  // as its two words so that the record keeps its 4-byte alignment.
  float sun_color[3];
  float pdf, invpdf;
  unsigned cos_angle_w[2];
  float epdf;
};

// One mesh light's arrays, resident per device handle (yk_device_upload) and
// reached through DScene::ml[DLight::mesh]: pdf1D_t's cdf, the triangles in
// light order (triangleObject_t::getPrimitives) as vertices for
// triangle_t::sample and as a / e1 / e2 records for the hit test, their
// triangle_t::normal, and the light's triKdTree_t in the scene tree's node
// encoding with one padding node.
struct DMeshLight {
  const float* cdf;      // n + 1
  const float* verts;    // 9 per triangle: a, b, c
  const float* tris;     // kTriWords per triangle: a, e1, e2
  const float* nrm;      // 3 per triangle
  const uint2* nodes;
  const uint32_t* leaf;
  float bound[6];
  int n;
  unsigned nnodes, depth_cap, nleaf;
};

struct DCam {  // the camera after camera_t ctor + setAxis (yk_camera_state)
  float pos[3], vright[3], vup[3], vto[3], camZ[3], near_p[3], far_p[3];
  // depth of field (aperture != 0): dof_rt, dof_up, dof_distance, bokeh, LS
  float aperture, dof_distance, dof_rt[3], dof_up[3];
  int bokeh_type, bokeh_bias;
  float ls[16];
  // which shootRay runs (YK_CAMERA_PERSPECTIVE, _ORTHOGRAPHIC, _ANGULAR), and
  // angularCam_t's constants: (PFLOAT)resx / resy, camera_t::aspect_ratio,
  // hor_phi, max_r, circular. All zero for the perspective kind.
  int kind;
  float resx, resy, aspect, hor_phi, max_r;
  int circular;
};

constexpr int kMaxMats = 64;
constexpr int kMaxLights = 8;
__constant__ DMat c_mats[kMaxMats];
__constant__ DLight c_lights[kMaxLights];
__constant__ DCam c_cam;

constexpr int kSmoothBit = 0x10000;  // prim interpolates vertex normals (mesh is_smooth)
struct DScene {
  const float* tris;     // triangle records (kTriWords floats per prim): a, prim id, e1=b-a, e2=c-a
  const uint2* nodes;    // kd nodes (kdtree_build.h encoding)
  const uint32_t* pk;    // node packets (k_pack_nodes): 24 B per node, its word and its children's
  const float* ltris;    // leaf-ordered copies of the records (k_gather_leaf_tris), one per leaf-list entry
  const uint32_t* leaf;  // leaf primitive lists
  const float4* ng;      // geometric normal xyz, w = material id | kSmoothBit (int bits)
  const float* vn;       // 9 floats per prim: getSurface's vertex normals (smooth scenes only)
  float bound[6];
  int nlights;
  unsigned nnodes;  // node count, for the pop-time bounds guard and the per-ray watchdog
  unsigned depth_cap;  // tree depth + 2: node visits of one valid descent and stack entries of a
                       // valid traversal (the watchdog's bounds)
  unsigned chunk_max;  // largest ray hand-out chunk (64 for crowded-leaf scenes, whose rays are costly)
  int nmats;           // material records in c_mats (the shading kernels copy them to LDS)
  unsigned ntris;      // records in tris
  unsigned nlref;      // leaf-list entries (records in ltris)
  int uni;             // universal mode (vTriangle_t getSurface: b0 = 0; IntersectS t > tmin)
  const DMeshLight* ml;  // mesh-light records (null without a mesh light)
};

__device__ __forceinline__ v3 ld3(const float* p) { return V3(p[0], p[1], p[2]); }

// Triangle record, 36 B: a, e1 = b - a, e2 = c - a -- the Moller-Trumbore
// inputs with the reference's own subtractions, three 12-B loads. Round 5:
// tight 36-B records (the prim id, which only a closest hit's winner needs,
// comes from the leaf list) instead of 48-B ones (a, prim id | e1, 0 | e2, 0),
// so the traversal's triangle arrays take 25 % fewer cache lines and bytes
// (1M probe: 183 MB instead of 244 MB; hair: 15 GB instead of 20 GB).
constexpr unsigned kTriWords = 9;
// 4-B aligned (the records sit at 12-B offsets): the load is global_load_dwordx3
// of exactly 12 B, never a widened 16-B one; the record arrays
// are also allocated kRecPad words long past their end (upload)
typedef float f3l __attribute__((ext_vector_type(3), aligned(4)));
constexpr size_t kRecPad = 4;
// TW = 12: the 48-B records of a small scene's LDS copy (16-B aligned vectors)
// (read as three 16-B vectors: ds_read_b128 serves 16 lanes per LDS cycle,
// ds_read_b96 only 8)
template <unsigned TW = kTriWords>
__device__ __forceinline__ void ld_tri(const float* rec, float4& A, float4& E1, float4& E2) {
  if constexpr (TW == 12u) {
    A = *reinterpret_cast<const float4*>(rec);
    E1 = *reinterpret_cast<const float4*>(rec + 4);
    E2 = *reinterpret_cast<const float4*>(rec + 8);
    return;
  }
  const f3l a = *reinterpret_cast<const f3l*>(rec), e1 = *reinterpret_cast<const f3l*>(rec + TW / 3),
            e2 = *reinterpret_cast<const f3l*>(rec + 2 * (TW / 3));
  A = make_float4(a.x, a.y, a.z, 0.f);
  E1 = make_float4(e1.x, e1.y, e1.z, 0.f);
  E2 = make_float4(e2.x, e2.y, e2.z, 0.f);
}

struct SurfPt {
  v3 P, N, Ng, NU, NV;
  int mat;
};

#include "yk_trav.inc"  // kd-tree traversal: TravStats, LaneStackT, trace_body, YK_TRACE_VARIANTS, k_trace_*

// ============================================================ shading


// scene_t::intersect tail + triangle_t::getSurface (flat shading subset)
__device__ __forceinline__ SurfPt make_surface(const DScene& S, v3 from, v3 dir, const yk_hit& h) {
  SurfPt sp;
  sp.P = vadd(from, vmul(h.t, dir));
  const float4 g = S.ng[h.prim];
  sp.Ng = V3(g.x, g.y, g.z);
  sp.N = sp.Ng;
  const int mw = __float_as_int(g.w);
  sp.mat = mw & (kSmoothBit - 1);
  if (mw & kSmoothBit) {
    // triangle.cc:19-28 / 185-194: N = normalize(u*va + v*vb + w*vc) with
    // u = b0 = 1-(b1+b2) (compiled form of intersect's 1-u-v); va..vc resolved
    // on the host (missing normals -> Ng, instance transform applied)
    const float* vn = S.vn + 9 * (size_t)h.prim;
    // vTriangle_t (universal mode): intersect never sets data.b0, which keeps
    // its 0 from intersectData_t's constructor (triangle.cc:365-385, 409)
    const float b0 = S.uni ? 0.0f : 1.0f - (h.b1 + h.b2);
    sp.N = vnormalize(vadd(vadd(vmul(b0, ld3(vn)), vmul(h.b1, ld3(vn + 3))), vmul(h.b2, ld3(vn + 6))));
  }
  create_cs(sp.N, sp.NU, sp.NV);
  return sp;
}

__device__ __forceinline__ v3 face_forward(v3 Ng, v3 N, v3 I) {  // FACE_FORWARD, material.h:30
  return (vdot(Ng, I) < 0.f) ? vneg(N) : N;
}

// getFresnel, shinydiffuse.cc:100-122. Compiled form: c = |N.wo| (the
// face-forward sign folded into fabs), g tested as ior2 + c*c < 1,
// 0.5*(g-c)^2 as ((g-c)*(g-c))*0.5, aux = (g+c)*c.
__device__ __forceinline__ float mat_fresnel(const DMat& M, v3 wo, v3 N) {
  if (!M.fresnel) return 1.f;
  const float c = fabsf(N.x * wo.x + N.y * wo.y + N.z * wo.z);
  const float t = M.ior2 + c * c;
  const float g = (t < 1.f) ? 0.f : sqrtf(t - 1.f);
  const float gc = g + c, aux = gc * c;
  const float a = (((g - c) * (g - c)) * 0.5f) / (gc * gc);
  const float b = ((aux - 1.f) * (aux - 1.f)) / ((aux + 1.f) * (aux + 1.f)) + 1.f;
  return b * a;
}

// accumulate(), shinydiffuse.cc:124-133; compiled: accum3 = ((1-c2)*c3)*acc
__device__ __forceinline__ void mat_accum(const DMat& M, float Kr, float* a) {
  a[0] = Kr * M.comp[0];
  const float t = 1.f - a[0];
  a[1] = t * M.comp[1];
  const float acc2 = (1.f - M.comp[1]) * t;
  a[2] = acc2 * M.comp[2];
  a[3] = ((1.f - M.comp[2]) * M.comp[3]) * acc2;
}

// shinyDiffuseMat_t::OrenNayar, shinydiffuse.cc:185-220, in source order
// (parity unpinned: no reference output has an Oren-Nayar material).
// std::min(1.f, x) / std::max(1e-8f, x) as the ternaries <algorithm> defines
// (a NaN dot product gives 1 then), fSqrt = sqrtf, normalize() as vector3d.h.
__device__ __forceinline__ float oren_nayar(const DMat& M, v3 wi, v3 wo, v3 N) {
  const float di = vdot(N, wi), dO = vdot(N, wo);
  const float mi = (di < 1.f) ? di : 1.f, mo = (dO < 1.f) ? dO : 1.f;
  const float cos_ti = (1e-8f < mi) ? mi : 1e-8f, cos_to = (1e-8f < mo) ? mo : 1e-8f;
  float maxcos_f = 0.f;
  if (cos_ti < 0.9999f && cos_to < 0.9999f) {
    const v3 v1 = vnormalize(vsub(wi, vmul(cos_ti, N)));
    const v3 v2 = vnormalize(vsub(wo, vmul(cos_to, N)));
    const float d = vdot(v1, v2);
    maxcos_f = (0.f < d) ? d : 0.f;
  }
  float sin_alpha, tan_beta;
  if (cos_to >= cos_ti) {
    sin_alpha = sqrtf(1.f - cos_ti * cos_ti);
    tan_beta = sqrtf(1.f - cos_to * cos_to) / cos_to;
  } else {
    sin_alpha = sqrtf(1.f - cos_to * cos_to);
    tan_beta = sqrtf(1.f - cos_ti * cos_ti) / cos_ti;
  }
  return M.on_a + ((M.on_b * maxcos_f) * sin_alpha) * tan_beta;
}

// ---- glossy (glossyMat_t, glossy.cc; microfacet.h; mathOptimizations.h) ----
// In source order (no reference output holds a glossy material, so nothing
// pins a compiled form); std::min / std::max as the ternaries <algorithm>
// defines, so a NaN operand falls through as it does there.

// fLog2 / fExp2 / fPow (FAST_MATH), mathOptimizations.h:83-125,200-207: integer
// arithmetic on the float's bits, so zero and negative bases have values too
// (the sign bit is masked off, zero reads as exponent -127). POLYLOG's fourth
// constant is a double literal: the polynomial's outer three steps run in
// double. A NaN exponent is outside what the reference defines ((int) of it).
__device__ __forceinline__ float fexp2_ref(float x) {
  x = (129.00000f < x) ? 129.00000f : x;    // std::min(x, f_HI)
  x = (x < -126.99999f) ? -126.99999f : x;  // std::max(x, f_LOW)
  const int ipart = (int)(x - 0.5f);
  const float f = x - (float)ipart;
  const float expipart = __int_as_float((int)((unsigned)(ipart + 127) << 23));
  const float poly =
      f * (f * (f * (f * (f * 1.8775767e-3f + 8.9893397e-3f) + 5.5826318e-2f) + 2.4015361e-1f) + 6.9315308e-1f) +
      9.9999994e-1f;
  return expipart * poly;
}
__device__ __forceinline__ float flog2_ref(float x) {
  const int i = __float_as_int(x);
  const float e = (float)(((i & 0x7F800000) >> 23) - 127);
  const float m = __int_as_float((i & 0x7FFFFF) | 0x3F800000);
  const float p2 = m * (m * -3.4436006e-2f + 3.1821337e-1f) + -1.2315303f;
  const double p5 = (double)m * ((double)m * ((double)(m * p2) + 2.5988452) + (double)-3.3241990f) + (double)3.1157899f;
  return (float)p5 * (m - 1.0f) + e;
}
__device__ __forceinline__ float fpow_ref(float a, float b) { return fexp2_ref(flog2_ref(a) * b); }

// pdfDivisor / ASDivisor, microfacet.h:35-43: 8.f * M_PI is a double
__device__ __forceinline__ float gl_pdf_divisor(float c) { return (float)(8.0 * YK_PI_D * (double)(c * 0.99f + 0.04f)); }
__device__ __forceinline__ float gl_as_divisor(float cos1, float cosI, float cosO) {
  const float mx = (cosI < cosO) ? cosO : cosI;  // std::max(cosI, cosO)
  return (float)(8.0 * YK_PI_D * (double)((cos1 * mx) * 0.99f + 0.04f));
}
// SchlickFresnel, microfacet.h:195-200
__device__ __forceinline__ float gl_schlick(float costheta, float R) {
  const float c1 = 1.f - costheta;
  const float c2 = c1 * c1;
  return R + ((1.f - R) * c1 * c2 * c2);
}
// Blinn_D, AS_Aniso_D, microfacet.h:60-65,96-99
__device__ __forceinline__ float gl_blinn_d(float cos_h, float e) { return (e + 1.f) * fpow_ref(cos_h, e); }
__device__ __forceinline__ float gl_aniso_d(v3 h, float e_u, float e_v) {
  if (h.z <= 0.f) return 0.f;
  const float exponent = (e_u * h.x * h.x + e_v * h.y * h.y) / (1.00001f - h.z * h.z);
  return sqrtf((e_u + 1.f) * (e_v + 1.f)) * fpow_ref((0.f < h.z) ? h.z : 0.f, exponent);
}
// the lobe's D for half vector H: Blinn over H.N or Ashikhmin-Shirley over H in the (NU, NV, N) frame
__device__ __forceinline__ float gl_lobe_d(const DMat& M, const SurfPt& sp, v3 H, float cos_N_H) {
  if (M.gl.anisotropic) return gl_aniso_d(V3(vdot(H, sp.NU), vdot(H, sp.NV), cos_N_H), M.gl.exp_u, M.gl.exp_v);
  return gl_blinn_d(cos_N_H, M.gl.exponent);
}
// sample_quadrant_aniso / AS_Aniso_Sample, microfacet.h:45-58,72-94. atan and
// tanf are the device library's atanf and tanf (unpinned, like the angular
// camera's atan2f); M_PI_2 * s1 is a double product.
__device__ __forceinline__ v3 gl_sample_quadrant(float s1, float s2, float e_u, float e_v) {
  const float phi = atanf(sqrtf((e_u + 1.f) / (e_v + 1.f)) * tanf((float)(1.57079632679489661923 * (double)s1)));
  const float cosPhi = fcos_ref(phi), sinPhi = fsin_ref(phi);
  const float cosPhi2 = cosPhi * cosPhi;
  const float sinPhi2 = 1.f - cosPhi2;
  const float cosTheta = fpow_ref(1.f - s2, 1.f / (e_u * cosPhi2 + e_v * sinPhi2 + 1.f));
  const float sinTheta = sqrtf(1.f - cosTheta * cosTheta);
  return V3(sinTheta * cosPhi, sinTheta * sinPhi, cosTheta);
}
__device__ __forceinline__ v3 gl_aniso_sample(float s1, float s2, float e_u, float e_v) {
  v3 H;
  if (s1 < 0.25f) {
    H = gl_sample_quadrant(4.f * s1, s2, e_u, e_v);
  } else if (s1 < 0.5f) {
    H = gl_sample_quadrant(1.f - 4.f * (0.5f - s1), s2, e_u, e_v);
    H.x = -H.x;
  } else if (s1 < 0.75f) {
    H = gl_sample_quadrant(4.f * (s1 - 0.5f), s2, e_u, e_v);
    H.x = -H.x;
    H.y = -H.y;
  } else {
    H = gl_sample_quadrant(1.f - 4.f * (1.f - s1), s2, e_u, e_v);
    H.y = -H.y;
  }
  return H;
}
// Blinn_Sample, microfacet.h:106-113: phi = s1 * M_2PI is a double product
__device__ __forceinline__ v3 gl_blinn_sample(float s1, float s2, float exponent) {
  const float cosTheta = fpow_ref(1.f - s2, 1.f / (exponent + 1.f));
  const float sinTheta = sqrtf(1.f - cosTheta * cosTheta);
  const float phi = (float)((double)s1 * YK_2PI_D);
  return V3(sinTheta * fcos_ref(phi), sinTheta * fsin_ref(phi), cosTheta);
}
// diffuseReflect, microfacet.h:202-212: the product runs in double from
// DIFFUSE_RATIO on and is rounded to float where it meets the colour
__device__ __forceinline__ c3 gl_diffuse_reflect(float wiN, float woN, float mGlossy, float mDiffuse, c3 base) {
  float f_wi = 1.f - (0.5f * wiN);
  float temp = f_wi * f_wi;
  f_wi = temp * temp * f_wi;
  float f_wo = 1.f - (0.5f * woN);
  temp = f_wo * f_wo;
  f_wo = temp * temp * f_wo;
  const float k = (float)(0.387507688 * (double)mDiffuse * (double)(1.f - mGlossy) * (double)(1.f - f_wi) *
                          (double)(1.f - f_wo));
  return cscale(k, base);
}
// glossyMat_t::OrenNayar, glossy.cc:105-132 (its clamps are not shinydiffuse's)
__device__ __forceinline__ float gl_oren_nayar(const DMat& M, v3 wi, v3 wo, v3 N) {
  const float di = vdot(N, wi), dO = vdot(N, wo);
  const float mi = (di < 1.f) ? di : 1.f, mo = (dO < 1.f) ? dO : 1.f;
  const float cos_ti = (-1.f < mi) ? mi : -1.f, cos_to = (-1.f < mo) ? mo : -1.f;
  float maxcos_f = 0.f;
  if (cos_ti < 0.9999f && cos_to < 0.9999f) {
    const v3 v1 = vnormalize(vsub(wi, vmul(cos_ti, N)));
    const v3 v2 = vnormalize(vsub(wo, vmul(cos_to, N)));
    const float d = vdot(v1, v2);
    maxcos_f = (0.f < d) ? d : 0.f;
  }
  float sin_alpha, tan_beta;
  if (cos_to >= cos_ti) {
    sin_alpha = sqrtf(1.f - cos_ti * cos_ti);
    tan_beta = sqrtf(1.f - cos_to * cos_to) / ((cos_to == 0.f) ? 1e-8f : cos_to);
  } else {
    sin_alpha = sqrtf(1.f - cos_to * cos_to);
    tan_beta = sqrtf(1.f - cos_ti * cos_ti) / ((cos_ti == 0.f) ? 1e-8f : cos_ti);
  }
  return M.on_a + M.on_b * maxcos_f * sin_alpha * tan_beta;
}

// glossyMat_t::eval, glossy.cc:134-173 (as_diffuse). The diffuse base is
// mDiffuse * (1 - mGlossy) * diff_color * OrenNayar here; sample() uses
// diffuseReflect instead.
__device__ __forceinline__ c3 glossy_eval(const DMat& M, const SurfPt& sp, v3 wo, v3 wi, unsigned bsdfs) {
  if (!(bsdfs & BSDF_DIFFUSE) || (vdot(sp.Ng, wi) * vdot(sp.Ng, wo)) < 0.f) return C3(0.f, 0.f, 0.f);
  const v3 N = face_forward(sp.Ng, sp.N, wo);
  const float wiN = fabsf(vdot(wi, N)), woN = fabsf(vdot(wo, N));
  const v3 H = vnormalize(vadd(wo, wi));
  const float d = vdot(wi, H);
  const float cos_wi_H = (0.f < d) ? d : 0.f;
  const float glossy =
      gl_lobe_d(M, sp, H, vdot(H, N)) * gl_schlick(cos_wi_H, M.gl.m_glossy) / gl_as_divisor(cos_wi_H, woN, wiN);
  c3 col = cscale(glossy, C3(M.col[0], M.col[1], M.col[2]));
  if (M.gl.with_diffuse) {
    const c3 dc = cscale(M.gl.m_diffuse * (1.f - M.gl.m_glossy), C3(M.gl.diff[0], M.gl.diff[1], M.gl.diff[2]));
    col = cadd(col, cscale(M.on ? gl_oren_nayar(M, wi, wo, N) : 1.f, dc));
  }
  return col;
}

// glossyMat_t::sample, glossy.cc:176-305 (as_diffuse). ok = false where the
// reference returns before it writes W: black, W untouched -- but wi, pdf and,
// in the diffuse half, sampledFlags are already written by then, as there.
__device__ __forceinline__ c3 glossy_sample(const DMat& M, const SurfPt& sp, v3 wo, v3& wi, float s1, float s2,
                                            unsigned flags, float& pdf, float& W, bool& ok, unsigned& sflags) {
  const float cos_Ng_wo = vdot(sp.Ng, wo);
  const v3 N = face_forward(sp.Ng, sp.N, wo);
  pdf = 0.f;
  float wiN = 0.f;
  const float woN = fabsf(vdot(wo, N));
  c3 scolor = C3(0.f, 0.f, 0.f);
  const float pD = M.gl.p_diffuse, mG = M.gl.m_glossy;
  const bool use_glossy = (flags & BSDF_DIFFUSE) != 0;
  const bool use_diffuse = M.gl.with_diffuse && (flags & BSDF_DIFFUSE);
  const c3 gcol = C3(M.col[0], M.col[1], M.col[2]), dcol = C3(M.gl.diff[0], M.gl.diff[1], M.gl.diff[2]);
  float glossy = 0.f;
  if (use_diffuse) {
    const float s_pDiffuse = use_glossy ? pD : 1.f;
    if (s1 < s_pDiffuse) {
      s1 /= s_pDiffuse;
      wi = sample_cos_hemisphere(N, sp.NU, sp.NV, s1, s2);
      if (vdot(sp.Ng, wi) * cos_Ng_wo < 0.f) {
        ok = false;
        return scolor;
      }
      wiN = fabsf(vdot(wi, N));
      pdf = wiN;
      if (use_glossy) {
        const v3 H = vnormalize(vadd(wi, wo));
        const float cos_wo_H = vdot(wo, H), cos_wi_H = fabsf(vdot(wi, H)), cos_N_H = vdot(N, H);
        const float D = gl_lobe_d(M, sp, H, cos_N_H);
        pdf = pdf * pD + (D / gl_pdf_divisor(cos_wo_H)) * (1.f - pD);
        glossy = D * gl_schlick(cos_wi_H, mG) / gl_as_divisor(cos_wi_H, woN, wiN);
      }
      sflags = BSDF_DIFFUSE | BSDF_REFLECT;
      if (!(flags & BSDF_REFLECT)) {
        ok = false;
        return C3(0.f, 0.f, 0.f);
      }
      scolor = cscale(glossy, gcol);
      scolor = cadd(scolor, cscale(M.on ? gl_oren_nayar(M, wi, wo, N) : 1.f, gl_diffuse_reflect(wiN, woN, mG, M.gl.m_diffuse, dcol)));
      W = wiN / (pdf * 0.99f + 0.01f);
      return scolor;
    }
    s1 -= pD;
    s1 /= (1.f - pD);
  }
  if (use_glossy) {
    const v3 Hs = M.gl.anisotropic ? gl_aniso_sample(s1, s2, M.gl.exp_u, M.gl.exp_v) : gl_blinn_sample(s1, s2, M.gl.exponent);
    v3 H = vadd(vadd(vmul(Hs.x, sp.NU), vmul(Hs.y, sp.NV)), vmul(Hs.z, N));
    float cos_wo_H = vdot(wo, H);
    if (cos_wo_H < 0.f) {  // H.reflect(N), vector3d.h:288-295
      const float vn = 2.0f * vdot(H, N);
      H = V3(vn * N.x - H.x, vn * N.y - H.y, vn * N.z - H.z);
      cos_wo_H = vdot(wo, H);
    }
    {  // reflect_dir(H, wo), vector3d.h:297-302
      const float vn = vdot(wo, H);
      if (vn < 0.f) {
        wi = vneg(wo);
      } else {
        const float v2 = 2.f * vn;
        wi = V3(v2 * H.x - wo.x, v2 * H.y - wo.y, v2 * H.z - wo.z);
      }
    }
    if (cos_Ng_wo * vdot(sp.Ng, wi) < 0.f) {
      ok = false;
      return C3(0.f, 0.f, 0.f);
    }
    wiN = fabsf(vdot(wi, N));
    // the anisotropic branch evaluates D on the sampled Hs, the Blinn one on H.N after the reflection
    const float D = M.gl.anisotropic ? gl_aniso_d(Hs, M.gl.exp_u, M.gl.exp_v) : gl_blinn_d(vdot(H, N), M.gl.exponent);
    pdf = D / gl_pdf_divisor(cos_wo_H);
    glossy = D * gl_schlick(cos_wo_H, mG) / gl_as_divisor(cos_wo_H, woN, wiN);
    scolor = cscale(glossy, gcol);
    sflags = BSDF_DIFFUSE | BSDF_REFLECT;
  }
  if (use_diffuse) {
    pdf = wiN * pD + pdf * (1.f - pD);
    scolor = cadd(scolor, cscale(M.on ? gl_oren_nayar(M, wi, wo, N) : 1.f, gl_diffuse_reflect(wiN, woN, mG, M.gl.m_diffuse, dcol)));
  }
  W = wiN / (pdf * 0.99f + 0.01f);
  return scolor;
}

// glossyMat_t::pdf, glossy.cc:307-351 (as_diffuse)
__device__ __forceinline__ float glossy_pdf(const DMat& M, const SurfPt& sp, v3 wo, v3 wi, unsigned flags) {
  if (vdot(sp.Ng, wo) * vdot(sp.Ng, wi) < 0.f) return 0.f;
  const v3 N = face_forward(sp.Ng, sp.N, wo);
  const bool use_glossy = (flags & BSDF_DIFFUSE) != 0;
  const bool use_diffuse = M.gl.with_diffuse && (flags & BSDF_DIFFUSE);
  float pdf = 0.f;
  if (use_diffuse) pdf = fabsf(vdot(wi, N));
  if (use_glossy) {
    const v3 H = vnormalize(vadd(wi, wo));
    const float lobe = gl_lobe_d(M, sp, H, vdot(N, H)) / gl_pdf_divisor(vdot(wo, H));
    pdf = use_diffuse ? pdf * M.gl.p_diffuse + lobe * (1.f - M.gl.p_diffuse) : lobe;
  }
  return pdf;
}

// ---- coated glossy (coatedGlossyMat_t, coatedglossy.cc; fresnel(), vector3d.cc:110-137) ----
// The glossy base seen through a dielectric coat that reflects perfectly with
// a Fresnel weight. In source order, like glossy: no reference output holds
// the material. Its record is the glossy half of DMat plus gl.mirror / gl.ior.

// fresnel(), vector3d.cc:110-137: eta*eta + c*c - 1 and 1 + (...) run in float
// (integer literals), the 0.5*(g-c)*(g-c) product and all that meets it in double
__device__ __forceinline__ void fresnel_ref(v3 I, v3 n, float IOR, float& Kr, float& Kt) {
  const float eta = IOR;
  const v3 N = (vdot(I, n) < 0.f) ? vneg(n) : n;
  const float c = vdot(I, N);
  float g = eta * eta + c * c - 1.f;
  if (g <= 0.f) g = 0.f;
  else g = sqrtf(g);
  const float aux = c * (g + c);
  Kr = (float)((((0.5 * (double)(g - c)) * (double)(g - c)) / (double)((g + c) * (g + c))) *
               (double)(1.f + ((aux - 1.f) * (aux - 1.f)) / ((aux + 1.f) * (aux + 1.f))));
  if ((double)Kr < 1.0) Kt = 1.f - Kr;
  else Kt = 0.f;
}

// coatedGlossyMat_t::eval, coatedglossy.cc:156-193 (as_diffuse). cos_wi_H is not
// clamped here (glossy's is); the diffuse base is multiplied by Kt directly,
// where sample() goes through diffuseReflectFresnel.
__device__ __forceinline__ c3 coated_eval(const DMat& M, const SurfPt& sp, v3 wo, v3 wi, unsigned bsdfs) {
  if (!(bsdfs & BSDF_DIFFUSE) || (vdot(sp.Ng, wi) * vdot(sp.Ng, wo)) < 0.f) return C3(0.f, 0.f, 0.f);
  const v3 N = face_forward(sp.Ng, sp.N, wo);
  float Kr, Kt;
  const float wiN = fabsf(vdot(wi, N)), woN = fabsf(vdot(wo, N));
  fresnel_ref(wo, N, M.gl.ior, Kr, Kt);
  const v3 H = vnormalize(vadd(wo, wi));
  const float cos_wi_H = vdot(wi, H);
  const float glossy =
      Kt * gl_lobe_d(M, sp, H, vdot(H, N)) * gl_schlick(cos_wi_H, M.gl.m_glossy) / gl_as_divisor(cos_wi_H, woN, wiN);
  c3 col = cscale(glossy, C3(M.col[0], M.col[1], M.col[2]));
  if (M.gl.with_diffuse) {
    const c3 dc = cscale(M.gl.m_diffuse * (1.f - M.gl.m_glossy), C3(M.gl.diff[0], M.gl.diff[1], M.gl.diff[2]));
    col = cadd(col, cscale(M.on ? gl_oren_nayar(M, wi, wo, N) : 1.f, cscale(Kt, dc)));
  }
  return col;
}

// coatedGlossyMat_t::sample, coatedglossy.cc:195-336 (as_diffuse): three
// components -- the coat (C_SPECULAR, width Kr), the lobe (C_GLOSSY, width
// Kt*(1-pDiffuse)) and, with a diffuse base, the base (C_DIFFUSE, width
// Kt*pDiffuse) -- of which the mask's matches are picked by s1. ok = false
// where the reference returns before it writes W: black, W untouched, wi
// written only if the pick had set it by then. s.reverse is never set on this
// path, so the back-sample members do not exist here.
__device__ __forceinline__ c3 coated_sample(const DMat& M, const SurfPt& sp, v3 wo, v3& wi, float s1in, float s2,
                                            unsigned flags, float& pdf, float& W, bool& ok, unsigned& sflags) {
  constexpr unsigned kSpec = BSDF_SPECULAR | BSDF_REFLECT, kDiff = BSDF_DIFFUSE | BSDF_REFLECT;
  const float cos_Ng_wo = vdot(sp.Ng, wo);
  const v3 N = face_forward(sp.Ng, sp.N, wo);
  pdf = 0.f;
  float Kr, Kt;
  fresnel_ref(wo, N, M.gl.ior, Kr, Kt);
  const bool use_spec = (flags & kSpec) == kSpec;
  const bool use_glossy = (flags & kDiff) == kDiff;                  // cFlags[C_GLOSSY] with as_diffuse
  const bool use_diffuse = M.gl.with_diffuse && use_glossy;          // nBSDF == 3
  // the matches in component order: width, running sum and component of each
  float width[3] = {0.f, 0.f, 0.f}, val[3] = {0.f, 0.f, 0.f};
  int cidx[3] = {0, 0, 0};
  float sum = 0.f;
  int nMatch = 0;
  if (use_spec) {
    width[nMatch] = Kr;
    cidx[nMatch] = 0;
    sum += Kr;
    val[nMatch++] = sum;
  }
  if (use_glossy) {
    const float a = Kt * (1.f - M.gl.p_diffuse);
    width[nMatch] = a;
    cidx[nMatch] = 1;
    sum += a;
    val[nMatch++] = sum;
  }
  if (use_diffuse) {
    const float a = Kt * M.gl.p_diffuse;
    width[nMatch] = a;
    cidx[nMatch] = 2;
    sum += a;
    val[nMatch++] = sum;
  }
  if (!nMatch || (double)sum < 0.00001) {
    ok = false;
    return C3(0.f, 0.f, 0.f);
  }
  int pick = -1;
  if (nMatch == 1) {
    pick = 0;
    width[0] = 1.f;
  } else {
    const float inv_sum = 1.f / sum;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      if (i < nMatch) {
        val[i] *= inv_sum;
        width[i] *= inv_sum;
        if ((s1in <= val[i]) && (pick < 0)) pick = i;
      }
    }
  }
  if (pick < 0) pick = nMatch - 1;
  // per-lane picks read through selects, not indexed registers
  const float wp = pick == 0 ? width[0] : (pick == 1 ? width[1] : width[2]);
  const float vprev = pick == 1 ? val[0] : val[1];
  const int comp = pick == 0 ? cidx[0] : (pick == 1 ? cidx[1] : cidx[2]);
  float s1;
  if (pick > 0) s1 = (s1in - vprev) / wp;
  else s1 = s1in / wp;
  // width[rcIndex[C_GLOSSY]], width[rcIndex[C_DIFFUSE]]
  const float w_glossy = use_spec ? width[1] : width[0];
  const float w_diffuse = use_spec ? width[2] : width[1];

  const c3 gcol = C3(M.col[0], M.col[1], M.col[2]), dcol = C3(M.gl.diff[0], M.gl.diff[1], M.gl.diff[2]);
  if (comp == 0) {  // C_SPECULAR: wi = reflect_dir(N, wo), vector3d.h:297-302
    const float vn = vdot(wo, N);
    if (vn < 0.f) {
      wi = vneg(wo);
    } else {
      const float v2 = 2.f * vn;
      wi = V3(v2 * N.x - wo.x, v2 * N.y - wo.y, v2 * N.z - wo.z);
    }
    pdf = wp;
    W = 1.f;
    sflags = kSpec;
    return C3(M.gl.mirror[0] * Kr, M.gl.mirror[1] * Kr, M.gl.mirror[2] * Kr);
  }
  v3 Hs = V3(0.f, 0.f, 0.f), H;
  float cos_wo_H;
  if (comp == 1) {  // C_GLOSSY
    Hs = M.gl.anisotropic ? gl_aniso_sample(s1, s2, M.gl.exp_u, M.gl.exp_v) : gl_blinn_sample(s1, s2, M.gl.exponent);
    H = vadd(vadd(vmul(Hs.x, sp.NU), vmul(Hs.y, sp.NV)), vmul(Hs.z, N));
    cos_wo_H = vdot(wo, H);
    if (cos_wo_H < 0.f) {  // H.reflect(N), vector3d.h:288-295
      const float vn = 2.0f * vdot(H, N);
      H = V3(vn * N.x - H.x, vn * N.y - H.y, vn * N.z - H.z);
      cos_wo_H = vdot(wo, H);
    }
    {  // reflect_dir(H, wo)
      const float vn = vdot(wo, H);
      if (vn < 0.f) {
        wi = vneg(wo);
      } else {
        const float v2 = 2.f * vn;
        wi = V3(v2 * H.x - wo.x, v2 * H.y - wo.y, v2 * H.z - wo.z);
      }
    }
    if (cos_Ng_wo * vdot(sp.Ng, wi) < 0.f) {
      ok = false;
      return C3(0.f, 0.f, 0.f);
    }
  } else {  // C_DIFFUSE
    wi = sample_cos_hemisphere(N, sp.NU, sp.NV, s1, s2);
    if (cos_Ng_wo * vdot(sp.Ng, wi) < 0.f) {
      ok = false;
      return C3(0.f, 0.f, 0.f);
    }
    // use[C_GLOSSY] holds whenever the base matched: both carry DIFFUSE | REFLECT
    H = vnormalize(vadd(wi, wo));
    Hs = V3(vdot(H, sp.NU), vdot(H, sp.NV), vdot(H, N));
    cos_wo_H = vdot(wo, H);
  }
  const float woN = fabsf(vdot(wo, N));
  const float wiN = fabsf(vdot(wi, N));
  float glossy;
  if (M.gl.anisotropic) {
    const float D = gl_aniso_d(Hs, M.gl.exp_u, M.gl.exp_v);
    pdf += (D / gl_pdf_divisor(cos_wo_H)) * w_glossy;
    glossy = D * gl_schlick(cos_wo_H, M.gl.m_glossy) / gl_as_divisor(cos_wo_H, woN, wiN);
  } else {
    const float D = gl_blinn_d(vdot(H, N), M.gl.exponent);
    pdf += (D / gl_pdf_divisor(cos_wo_H)) * w_glossy;
    glossy = D * gl_schlick(cos_wo_H, M.gl.m_glossy) / gl_as_divisor(cos_wo_H, woN, wiN);
  }
  c3 scolor = cscale(glossy * Kt, gcol);
  if (use_diffuse) {  // diffuseReflectFresnel: Kt * diffuseReflect(...)
    const c3 dr = cscale(Kt, gl_diffuse_reflect(wiN, woN, M.gl.m_glossy, M.gl.m_diffuse, dcol));
    scolor = cadd(scolor, cscale(M.on ? gl_oren_nayar(M, wi, wo, N) : 1.f, dr));
    pdf += wiN * w_diffuse;
  }
  W = wiN / (pdf * 0.99f + 0.01f);
  sflags = kDiff;
  return scolor;
}

// coatedGlossyMat_t::pdf, coatedglossy.cc:338-382 (as_diffuse)
__device__ __forceinline__ float coated_pdf(const DMat& M, const SurfPt& sp, v3 wo, v3 wi, unsigned flags) {
  constexpr unsigned kSpec = BSDF_SPECULAR | BSDF_REFLECT, kDiff = BSDF_DIFFUSE | BSDF_REFLECT;
  if ((vdot(sp.Ng, wo) * vdot(sp.Ng, wi)) < 0.f) return 0.f;
  const v3 N = face_forward(sp.Ng, sp.N, wo);
  float pdf = 0.f, Kr, Kt;
  fresnel_ref(wo, N, M.gl.ior, Kr, Kt);
  float sum = 0.f;
  int nMatch = 0;
  if ((flags & kSpec) == kSpec) {
    sum += Kr;
    ++nMatch;
  }
  if ((flags & kDiff) == kDiff) {
    const float width = Kt * (1.f - M.gl.p_diffuse);
    sum += width;
    const v3 H = vnormalize(vadd(wi, wo));
    pdf += (gl_lobe_d(M, sp, H, vdot(N, H)) / gl_pdf_divisor(vdot(wo, H))) * width;
    ++nMatch;
    if (M.gl.with_diffuse) {
      const float wd = Kt * M.gl.p_diffuse;
      sum += wd;
      pdf += fabsf(vdot(wi, N)) * wd;
      ++nMatch;
    }
  }
  if (!nMatch || (double)sum < 0.00001) return 0.f;
  return pdf / sum;
}

// coatedGlossyMat_t::getSpecular, coatedglossy.cc:384-418. raylevel is
// state.raylevel, already incremented by recursiveRaytrace: a camera hit is
// level 1, and beyond level 5 the coat reflects nothing. 1.00001*cos_wo_N and
// 0.01 - cos_wi_Ng are double products rounded to float where they meet the
// vector. Never refracts.
__device__ __forceinline__ void coated_specular(const DMat& M, const SurfPt& sp, v3 wo, int raylevel, bool& refl,
                                                v3& dir, c3& col) {
  refl = false;
  const bool outside = vdot(sp.Ng, wo) >= 0.f;
  const float cos_wo_N = vdot(sp.N, wo);
  v3 N = sp.N, Ng = sp.Ng;
  if (outside ? !(cos_wo_N >= 0.f) : !(cos_wo_N <= 0.f)) {
    const float f = (float)(1.00001 * (double)cos_wo_N);
    N = vnormalize(vsub(sp.N, vmul(f, wo)));
  }
  if (!outside) Ng = vneg(sp.Ng);
  float Kr, Kt;
  fresnel_ref(wo, N, M.gl.ior, Kr, Kt);
  if (raylevel > 5) return;
  const float vn = 2.0f * vdot(wo, N);  // dir[0] = wo; dir[0].reflect(N)
  v3 w = V3(vn * N.x - wo.x, vn * N.y - wo.y, vn * N.z - wo.z);
  col = C3(Kr * M.gl.mirror[0], Kr * M.gl.mirror[1], Kr * M.gl.mirror[2]);
  const float cos_wi_Ng = vdot(w, Ng);
  if ((double)cos_wi_Ng < 0.01) {
    const float f = (float)(0.01 - (double)cos_wi_Ng);
    w = vnormalize(V3(w.x + f * Ng.x, w.y + f * Ng.y, w.z + f * Ng.z));
  }
  dir = w;
  refl = true;
}

// ---- glass (glassMat_t, glass.cc:28-337; refract(), vector3d.cc:86-108) ----
// The dielectric without dispersion, absorption or shader nodes, in source
// order like glossy and the coat: no reference output holds the material. Its
// record is the gs half of DMat; eval is black and pdf is 0.

// refract(), vector3d.cc:86-108: eta = 1.0/IOR is a double quotient stored to
// float, k runs in float (integer literals), fSqrt is sqrtf
__device__ __forceinline__ bool refract_ref(v3 n, v3 wi, v3& wo, float IOR) {
  v3 N = n;
  float eta = IOR;
  const v3 I = vneg(wi);
  float cos_v_n = vdot(wi, n);
  if (cos_v_n < 0.f) {
    N = vneg(n);
    cos_v_n = -cos_v_n;
  } else {
    eta = (float)(1.0 / (double)IOR);
  }
  const float k = 1.f - eta * eta * (1.f - cos_v_n * cos_v_n);
  if (k <= 0.f) return false;
  const float f = eta * cos_v_n - sqrtf(k);
  wo = vnormalize(V3(eta * I.x + f * N.x, eta * I.y + f * N.y, eta * I.z + f * N.z));
  return true;
}

// the normal both sample() and getSpecular() use (glass.cc:93-96, 208-218): sp.N unless it disagrees with Ng
// about wo's side, then bent just past wo's plane; 1.00001*cos_wo_N is a double product rounded to float where
// it meets the vector, as in coated_specular
__device__ __forceinline__ v3 glass_normal(const SurfPt& sp, v3 wo, bool& outside) {
  outside = vdot(sp.Ng, wo) > 0.f;
  const float cos_wo_N = vdot(sp.N, wo);
  if (outside ? (cos_wo_N >= 0.f) : (cos_wo_N <= 0.f)) return sp.N;
  const float f = (float)(1.00001 * (double)cos_wo_N);
  return vnormalize(vsub(sp.N, vmul(f, wo)));
}

// glassMat_t::sample, glass.cc:84-188, the non-dispersive branch. ok = false
// on the early return (the mask lacks BSDF_SPECULAR): pdf = 0, black, W and wi
// untouched. The fall-through (a mask that matches neither pick) has set no wi
// or W either and ends with pdf = 0. s.reverse is never set on this path.
__device__ __forceinline__ c3 glass_sample(const DMat& M, const SurfPt& sp, v3 wo, v3& wi, float s1, unsigned flags,
                                           float& pdf, float& W, bool& ok, unsigned& sflags) {
  constexpr unsigned kSpec = BSDF_SPECULAR | BSDF_REFLECT;
  if (!(flags & BSDF_SPECULAR)) {
    pdf = 0.f;
    ok = false;
    return C3(0.f, 0.f, 0.f);
  }
  bool outside;
  const v3 N = glass_normal(sp, wo, outside);
  pdf = 1.f;
  v3 refdir;
  const float vn = 2.0f * vdot(wo, N);  // wi = wo; wi.reflect(N), vector3d.h:288-295
  const v3 rdir = V3(vn * N.x - wo.x, vn * N.y - wo.y, vn * N.z - wo.z);
  if (refract_ref(N, wo, refdir, M.gs.ior)) {
    float Kr, Kt;
    fresnel_ref(wo, N, M.gs.ior, Kr, Kt);
    const float pKr = (float)(0.01 + 0.99 * (double)Kr), pKt = (float)(0.01 + 0.99 * (double)Kt);
    const unsigned tm = M.gs.fake_shadow ? (BSDF_FILTER | BSDF_TRANSMIT) : (BSDF_SPECULAR | BSDF_TRANSMIT);
    if (s1 < pKt && (flags & tm) == tm) {
      wi = refdir;
      pdf = pKt;
      sflags = tm;
      W = 1.f;
      return C3(M.gs.filter[0], M.gs.filter[1], M.gs.filter[2]);
    } else if ((flags & kSpec) == kSpec) {
      wi = rdir;
      pdf = pKr;
      sflags = kSpec;
      W = 1.f;
      return C3(M.gs.mirror[0], M.gs.mirror[1], M.gs.mirror[2]);
    }
  } else if ((flags & kSpec) == kSpec) {  // total inner reflection: colour 1, pdf stays 1
    wi = rdir;
    sflags = kSpec;
    W = 1.f;
    return C3(1.f, 1.f, 1.f);
  }
  pdf = 0.f;
  ok = false;
  return C3(0.f, 0.f, 0.f);
}

// glassMat_t::getSpecular, glass.cc:204-253. raylevel is state.raylevel after
// recursiveRaytrace's increment (1 at a camera hit): inside the glass the
// Fresnel reflection is followed only below level 3.
__device__ __forceinline__ void glass_specular(const DMat& M, const SurfPt& sp, v3 wo, int raylevel, bool& refl,
                                               bool& refr, v3* dir, c3* col) {
  bool outside;
  const v3 N = glass_normal(sp, wo, outside);
  const float vn = 2.0f * vdot(wo, N);
  const v3 rdir = V3(vn * N.x - wo.x, vn * N.y - wo.y, vn * N.z - wo.z);
  v3 refdir;
  if (refract_ref(N, wo, refdir, M.gs.ior)) {
    float Kr, Kt;
    fresnel_ref(wo, N, M.gs.ior, Kr, Kt);
    col[1] = C3(Kt * M.gs.filter[0], Kt * M.gs.filter[1], Kt * M.gs.filter[2]);
    dir[1] = refdir;
    refr = true;
    if (outside || raylevel < 3) {
      dir[0] = rdir;
      col[0] = C3(Kr * M.gs.mirror[0], Kr * M.gs.mirror[1], Kr * M.gs.mirror[2]);
      refl = true;
    } else {
      refl = false;
    }
  } else {  // total inner reflection
    col[0] = C3(1.f, 1.f, 1.f);
    dir[0] = rdir;
    refl = true;
    refr = false;
  }
}

// glassMat_t::getTransparency, glass.cc:190-196
__device__ __forceinline__ c3 glass_transparency(const DMat& M, const SurfPt& sp, v3 wo) {
  float Kr, Kt;
  fresnel_ref(wo, face_forward(sp.Ng, sp.N, wo), M.gs.ior, Kr, Kt);
  return C3(Kt * M.gs.filter[0], Kt * M.gs.filter[1], Kt * M.gs.filter[2]);
}

// glassMat_t::getAlpha, glass.cc:198-202: 1.0 - energy() is a double difference stored to float;
// energy() is (R+G+B)*0.333333f (color.h:77)
__device__ __forceinline__ float glass_alpha(const DMat& M, const SurfPt& sp, v3 wo) {
  const c3 t = glass_transparency(M, sp, wo);
  const float alpha = (float)(1.0 - (double)((t.r + t.g + t.b) * 0.333333f));
  return (alpha < 0.0f) ? 0.0f : alpha;
}

// shinyDiffuseMat_t::eval, shinydiffuse.cc:223-249 (compiled: cos_Ng_wl as
// (y + z) + x; mD = ((1-c2)*c3)*mT), then mD *= OrenNayar(wo, wl, N) (:247).
// ON = false: the scene has no Oren-Nayar material (the diffuse-only
// instantiation's scenes), so the factor's code is not compiled in.
// GL != kGLNone: the scene holds a glossy material; only then is glossy's code
// compiled in (mat_sample and mat_pdf likewise), so every other scene runs
// the kernels it ran before. bsdfs is BSDF_ALL at every call site.
// GL is a level: kGLNone, kGLGlossy (1 in the instantiations' names), or
// kGLCoated when the scene holds a coated glossy material as well or instead;
// only then is the coat's code compiled in, so glossy-only scenes too run the
// kernels they ran before. kGLGlass, on top of that, when the scene holds a
// glass material: a glass record is recognised before any shinydiffuse member
// (comp[], mirror[], mat_fresnel) is read, as the coat's is.
constexpr int kGLNone = 0, kGLGlossy = 1, kGLCoated = 2, kGLGlass = 3;
template <bool ON = true, int GL = kGLNone>
__device__ __forceinline__ c3 mat_eval(const DMat& M, const SurfPt& sp, v3 wo, v3 wl) {
  if (M.type == YK_MAT_LIGHT) return C3(0.f, 0.f, 0.f);
  if constexpr (GL) {
    if (M.type == YK_MAT_GLOSSY) return glossy_eval(M, sp, wo, wl, BSDF_ALL);
    if constexpr (GL >= kGLCoated) {
      if (M.type == YK_MAT_COATED_GLOSSY) return coated_eval(M, sp, wo, wl, BSDF_ALL);
    }
    if constexpr (GL >= kGLGlass) {
      if (M.type == YK_MAT_GLASS) return C3(0.f, 0.f, 0.f);
    }
  }
  const float cos_Ng_wo = vdot(sp.Ng, wo);
  const float cos_Ng_wl = (sp.Ng.y * wl.y + sp.Ng.z * wl.z) + sp.Ng.x * wl.x;
  const v3 N = (cos_Ng_wo < 0.f) ? vneg(sp.N) : sp.N;
  if (!(M.flags & BSDF_DIFFUSE)) return C3(0.f, 0.f, 0.f);
  const float Kr = mat_fresnel(M, wo, N);
  const float mT = (1.f - Kr * M.comp[0]) * (1.f - M.comp[1]);
  if (cos_Ng_wo * cos_Ng_wl < 0.f && M.translucent) return cscale(mT * M.comp[2], C3(M.col[0], M.col[1], M.col[2]));
  if (vdot(wl, N) < 0.0f) return C3(0.f, 0.f, 0.f);
  float mD = ((1.f - M.comp[2]) * M.comp[3]) * mT;
  if constexpr (ON) {
    if (M.on) mD *= oren_nayar(M, wo, wl, N);
  }
  return cscale(mD, C3(M.col[0], M.col[1], M.col[2]));
}

// shinyDiffuseMat_t::sample, shinydiffuse.cc:259-336; lightMat_t::sample
// (simple.cc:55-60). ok=false: early return with W and wi untouched.
// sflags = s.sampledFlags.
// DIFF: every material of the scene is a light or a shinydiffuse with the one
// component DIFFUSE|REFLECT (host check at upload, yk_device::diffuse_only):
// the general component loop below then matches that component alone, or
// nothing when the caller's mask lacks it, so the specialisation performs the
// same float operations on the same values -- sum = 0 + w, the normalisation
// by 1/sum, s1 / wp -- without the loop's per-lane arrays (the shading
// kernels' registers).
template <bool DIFF = false, int GL = kGLNone>
__device__ __forceinline__ c3 mat_sample(const DMat& M, const SurfPt& sp, v3 wo, v3& wi, float s1in, float s2in,
                                         unsigned flags, float& pdf, float& W, bool& ok, unsigned& sflags) {
  static_assert(!(DIFF && GL), "a scene with a glossy material is never diffuse-only");
  ok = true;
  sflags = 0u;
  if (M.type == YK_MAT_LIGHT) {
    pdf = 0.f;
    W = 0.f;
    return C3(0.f, 0.f, 0.f);
  }
  if constexpr (GL) {
    if (M.type == YK_MAT_GLOSSY) return glossy_sample(M, sp, wo, wi, s1in, s2in, flags, pdf, W, ok, sflags);
    if constexpr (GL >= kGLCoated) {
      if (M.type == YK_MAT_COATED_GLOSSY) return coated_sample(M, sp, wo, wi, s1in, s2in, flags, pdf, W, ok, sflags);
    }
    if constexpr (GL >= kGLGlass) {
      if (M.type == YK_MAT_GLASS) return glass_sample(M, sp, wo, wi, s1in, flags, pdf, W, ok, sflags);
    }
  }
  const float cos_Ng_wo = vdot(sp.Ng, wo);
  const v3 N = (cos_Ng_wo < 0.f) ? vneg(sp.N) : sp.N;
  const float Kr = mat_fresnel(M, wo, N);
  float a[4];
  mat_accum(M, Kr, a);
  if constexpr (DIFF) {
    if ((flags & (BSDF_DIFFUSE | BSDF_REFLECT)) != (BSDF_DIFFUSE | BSDF_REFLECT)) {  // no component matches
      pdf = 0.f;
      ok = false;
      return C3(1.f, 1.f, 1.f);
    }
    const int ci = M.cindex[0];
    const float w0 = ci == 0 ? a[0] : (ci == 1 ? a[1] : (ci == 2 ? a[2] : a[3]));
    float sum = 0.f;
    sum += w0;
    if ((double)sum < 0.00001) {
      pdf = 0.f;
      ok = false;
      return C3(1.f, 1.f, 1.f);
    }
    const float inv_sum = 1.f / sum;
    const float wp = w0 * inv_sum;
    const float s1 = s1in / wp;
    const v3 w = sample_cos_hemisphere(N, sp.NU, sp.NV, s1, s2in);
    c3 sc = C3(0.f, 0.f, 0.f);
    if (cos_Ng_wo * vdot(sp.Ng, w) > 0.f) sc = cscale(a[3], C3(M.col[0], M.col[1], M.col[2]));
    pdf = fabsf(vdot(N, w)) * wp;
    wi = w;
    sflags = BSDF_DIFFUSE | BSDF_REFLECT;
    W = fabsf(vdot(w, sp.N)) / (pdf * 0.99f + 0.01f);
    return sc;
  }
  float sum = 0.f, val[4], width[4];
  unsigned choice[4];
  int nMatch = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i < M.ncomp && (flags & M.cflags[i]) == M.cflags[i]) {
      const int ci = M.cindex[i];
      const float w = ci == 0 ? a[0] : (ci == 1 ? a[1] : (ci == 2 ? a[2] : a[3]));
      width[nMatch] = w;
      sum += w;
      choice[nMatch] = M.cflags[i];
      val[nMatch] = sum;
      ++nMatch;
    }
  }
  if (!nMatch || (double)sum < 0.00001) {
    pdf = 0.f;
    ok = false;
    return C3(1.f, 1.f, 1.f);
  }
  const float inv_sum = 1.f / sum;
  int pick = -1;
  for (int i = 0; i < nMatch; ++i) {
    val[i] *= inv_sum;
    width[i] *= inv_sum;
    if ((s1in <= val[i]) && (pick < 0)) pick = i;
  }
  if (pick < 0) pick = nMatch - 1;
  const float wp = width[pick];
  const float s1 = (pick > 0) ? (s1in - val[pick - 1]) / wp : s1in / wp;
  const c3 dcol = C3(M.col[0], M.col[1], M.col[2]);
  c3 sc = C3(0.f, 0.f, 0.f);
  v3 w;
  const unsigned ch = choice[pick];
  if (ch == (BSDF_SPECULAR | BSDF_REFLECT)) {  // reflect_dir(N, wo), compiled vn = (x + z) + y
    const float vn = (wo.x * N.x + wo.z * N.z) + N.y * wo.y;
    if (vn < 0.f) {
      w = vneg(wo);
    } else {
      const float v2 = vn + vn;
      w = V3(v2 * N.x - wo.x, v2 * N.y - wo.y, v2 * N.z - wo.z);
    }
    pdf = wp;
    sc = C3(M.mirror[0] * a[0], M.mirror[1] * a[0], M.mirror[2] * a[0]);
    const float k = 1.f / fabsf(vdot(w, sp.N));
    sc = C3(sc.r * k, sc.g * k, sc.b * k);
  } else if (ch == (BSDF_TRANSMIT | BSDF_FILTER)) {
    w = vneg(wo);
    const float t = 1.f - M.tfilter;
    sc = C3((dcol.r * M.tfilter + t) * a[1], (dcol.g * M.tfilter + t) * a[1], (dcol.b * M.tfilter + t) * a[1]);
    const float cosN = fabsf(vdot(N, w));
    pdf = ((double)cosN < 1e-6) ? 0.f : wp;
  } else if (ch == (BSDF_DIFFUSE | BSDF_TRANSMIT)) {
    w = sample_cos_hemisphere(vneg(N), sp.NU, sp.NV, s1, s2in);
    if (cos_Ng_wo * vdot(sp.Ng, w) < 0.f) sc = cscale(a[2], dcol);
    pdf = fabsf(vdot(N, w)) * wp;
  } else {
    w = sample_cos_hemisphere(N, sp.NU, sp.NV, s1, s2in);
    if (cos_Ng_wo * vdot(sp.Ng, w) > 0.f) sc = cscale(a[3], dcol);
    if (M.on) sc = cscale(oren_nayar(M, wo, w, N), sc);  // scolor *= OrenNayar(wo, wi, N), :330
    pdf = fabsf(vdot(N, w)) * wp;
  }
  wi = w;
  sflags = ch;
  W = fabsf(vdot(w, sp.N)) / (pdf * 0.99f + 0.01f);
  return sc;
}
template <bool DIFF = false, int GL = kGLNone>
__device__ __forceinline__ c3 mat_sample(const DMat& M, const SurfPt& sp, v3 wo, v3& wi, float s1in, float s2in,
                                         unsigned flags, float& pdf, float& W, bool& ok) {
  unsigned sf;
  return mat_sample<DIFF, GL>(M, sp, wo, wi, s1in, s2in, flags, pdf, W, ok, sf);
}

// shinyDiffuseMat_t::pdf, shinydiffuse.cc:338-377: every component sharing a
// bit with bsdfs adds its width to the sum; only diffuse ones add pdf.
// Called with bsdfs = GLOSSY|DIFFUSE|DISPERSIVE|REFLECT|TRANSMIT, which
// overlaps every shinydiffuse component.
template <int GL = kGLNone>
__device__ __forceinline__ float mat_pdf(const DMat& M, const SurfPt& sp, v3 wo, v3 wi) {
  if (M.type == YK_MAT_LIGHT) return 0.f;
  if constexpr (GL) {
    if (M.type == YK_MAT_GLOSSY)
      return glossy_pdf(M, sp, wo, wi, BSDF_GLOSSY | BSDF_DIFFUSE | BSDF_DISPERSIVE | BSDF_REFLECT | BSDF_TRANSMIT);
    if constexpr (GL >= kGLCoated) {
      if (M.type == YK_MAT_COATED_GLOSSY)
        return coated_pdf(M, sp, wo, wi, BSDF_GLOSSY | BSDF_DIFFUSE | BSDF_DISPERSIVE | BSDF_REFLECT | BSDF_TRANSMIT);
    }
    if constexpr (GL >= kGLGlass) {
      if (M.type == YK_MAT_GLASS) return 0.f;
    }
  }
  const float cos_Ng_wo = vdot(sp.Ng, wo);
  const v3 N = (cos_Ng_wo < 0.f) ? vneg(sp.N) : sp.N;
  const float Kr = mat_fresnel(M, wo, N);
  float a[4];
  mat_accum(M, Kr, a);
  float sum = 0.f, pdf = 0.f;
  for (int i = 0; i < M.ncomp; ++i) {
    const int ci = M.cindex[i];
    const float width = ci == 0 ? a[0] : (ci == 1 ? a[1] : (ci == 2 ? a[2] : a[3]));
    sum += width;
    if (M.cflags[i] == (BSDF_DIFFUSE | BSDF_TRANSMIT)) {
      if (cos_Ng_wo * vdot(sp.Ng, wi) < 0.f) pdf += fabsf(vdot(wi, N)) * width;
    } else if (M.cflags[i] == (BSDF_DIFFUSE | BSDF_REFLECT)) {
      pdf += fabsf(vdot(wi, N)) * width;
    }
  }
  if (M.ncomp == 0 || (double)sum < 0.00001) return 0.f;
  return pdf / sum;
}

// shinyDiffuseMat_t::getSpecular, shinydiffuse.cc:379-433 (compiled: the
// backface test as (x + z) + y; reflect() without a sign test; the 0.01
// grazing correction in double). GL: the scene holds a glossy or coated glossy
// material; a coated one answers with its own getSpecular at recursion level
// raylevel, and its record is never read through the shinydiffuse members.
template <int GL = kGLNone>
__device__ __forceinline__ void mat_specular(const DMat& M, const SurfPt& sp, v3 wo, bool& refl, bool& refr,
                                             v3* dir, c3* col, int raylevel = 0) {
  refl = refr = false;
  if (M.type == YK_MAT_LIGHT) return;
  if constexpr (GL >= kGLCoated) {
    if (M.type == YK_MAT_COATED_GLOSSY) {
      coated_specular(M, sp, wo, raylevel, refl, dir[0], col[0]);
      return;
    }
  }
  if constexpr (GL >= kGLGlass) {
    if (M.type == YK_MAT_GLASS) {
      glass_specular(M, sp, wo, raylevel, refl, refr, dir, col);
      return;
    }
  }
  const bool backface = ((sp.Ng.x * wo.x + sp.Ng.z * wo.z) + sp.Ng.y * wo.y) < 0.f;
  const v3 N = backface ? vneg(sp.N) : sp.N;
  const v3 Ng = backface ? vneg(sp.Ng) : sp.Ng;
  const float Kr = mat_fresnel(M, wo, N);
  if (M.flags & BSDF_FILTER) {  // mIsTransparent
    refr = true;
    dir[1] = vneg(wo);
    const float t = 1.f - M.tfilter;
    const float k = M.comp[1] * (1.f - M.comp[0] * Kr);
    col[1] = C3((M.col[0] * M.tfilter + t) * k, (M.col[1] * M.tfilter + t) * k, (M.col[2] * M.tfilter + t) * k);
  }
  if (M.flags & BSDF_SPECULAR) {  // mIsMirror
    refl = true;
    const float vn = vdot(wo, N);
    const float v2 = vn + vn;
    v3 w = V3(v2 * N.x - wo.x, v2 * N.y - wo.y, v2 * N.z - wo.z);
    const float cos_wi_Ng = vdot(w, Ng);
    if ((double)cos_wi_Ng < 0.01) {
      const float f = (float)(0.01 - (double)cos_wi_Ng);
      w = vnormalize(V3(f * Ng.x + w.x, f * Ng.y + w.y, f * Ng.z + w.z));
    }
    dir[0] = w;
    const float k = Kr * M.comp[0];
    col[0] = C3(M.mirror[0] * k, M.mirror[1] * k, M.mirror[2] * k);
  }
}

// shinyDiffuseMat_t::getTransparency, shinydiffuse.cc:435-455 (only called on
// transparent materials): accum = 1 - Kr*mirror; accum *= transparency*accum;
// accum * (filter*diffuse + (1 - filter))
// GLT: the scene holds a glass with fake shadows, whose getTransparency answers for its record.
template <bool GLT>
__device__ __forceinline__ c3 mat_transparency(const DMat& M, const SurfPt& sp, v3 wo) {
  if constexpr (GLT) {
    if (M.type == YK_MAT_GLASS) return glass_transparency(M, sp, wo);
  }
  float accum = 1.f;
  const float Kr = mat_fresnel(M, wo, face_forward(sp.Ng, sp.N, wo));
  if (M.flags & BSDF_SPECULAR) accum = 1.f - Kr * M.comp[0];
  accum *= M.comp[1] * accum;
  const float t = 1.f - M.tfilter;
  return C3(accum * (M.tfilter * M.col[0] + t), accum * (M.tfilter * M.col[1] + t), accum * (M.tfilter * M.col[2] + t));
}

// emit: shinyDiffuseMat_t::emit (shinydiffuse.cc:251-257), lightMat_t::emit (simple.cc:54-61)
__device__ __forceinline__ c3 mat_emit(const DMat& M, const SurfPt& sp, v3 wo, bool includeLights) {
  if (M.type == YK_MAT_LIGHT) {
    if (!includeLights) return C3(0.f, 0.f, 0.f);
    const c3 lc = C3(M.col[0], M.col[1], M.col[2]);
    if (M.double_sided) return lc;
    return (vdot(wo, sp.N) > 0.f) ? lc : C3(0.f, 0.f, 0.f);
  }
  return C3(M.emit_col[0], M.emit_col[1], M.emit_col[2]);
}


// areaLight_t::illumSample, arealight.cc:68-96 (compiled sample point form)
__device__ __forceinline__ bool light_illum(const DLight& L, v3 P, float s1, float s2, v3& ldir, float& tmax,
                                            float& pdf) {
  const v3 p = V3(L.corner[0] + (s1 * L.toX[0] + s2 * L.toY[0]), L.corner[1] + (s1 * L.toX[1] + s2 * L.toY[1]),
                  (L.corner[2] + s1 * L.toX[2]) + s2 * L.toY[2]);
  v3 l = vsub(p, P);
  const float dist_sqr = l.x * l.x + l.y * l.y + l.z * l.z;
  const float dist = sqrtf(dist_sqr);
  if (dist <= 0.0f) return false;
  const float id = 1.f / dist;
  l = V3(l.x * id, l.y * id, l.z * id);
  const float cos_angle = vdot(l, ld3(L.fnormal));
  if (cos_angle <= 0.f) return false;
  tmax = dist;
  ldir = l;
  pdf = (float)((double)dist_sqr * YK_PI_D / (double)(L.area * cos_angle));
  return true;
}

// areaLight_t::intersect, arealight.cc:138-154
__device__ __forceinline__ bool light_hit(const DLight& L, v3 from, v3 dir, float& t, float& ipdf) {
  const float cos_angle = vdot(dir, ld3(L.fnormal));
  if (cos_angle <= 0.f) return false;
  // triIntersect(corner, c2, c3) then (corner, c3, c4), edges precomputed
  float u, v;
  if (!mt_intersect(ld3(L.corner), ld3(L.e2), ld3(L.e3), from, dir, t, u, v)) {
    if (!mt_intersect(ld3(L.corner), ld3(L.e3), ld3(L.e4), from, dir, t, u, v)) return false;
  }
  if (!(t > 1.0e-10f)) return false;
  ipdf = (float)((double)((1.f / (t * t)) * L.area * cos_angle) * YK_1_PI_D);
  return true;
}

// sampleCone, sample_utils.h:76-82: float throughout, t1 = M_2PI * s1 in double
__device__ __forceinline__ v3 sample_cone(v3 D, v3 U, v3 V, float maxCosAng, float s1, float s2) {
  const float cosAng = 1.f - (1.f - maxCosAng) * s2;
  const float sinAng = sqrtf(1.f - cosAng * cosAng);
  const float t1 = (float)(YK_2PI_D * (double)s1);
  const float ct = fcos_ref(t1), st = fsin_ref(t1);
  return V3((U.x * ct + V.x * st) * sinAng + D.x * cosAng, (U.y * ct + V.y * st) * sinAng + D.y * cosAng,
            (U.z * ct + V.z * st) * sinAng + D.z * cosAng);
}

// The spot cone's falloff at cosa (spotlight.cc:127-136 and its copies in
// illumSample / intersect): false outside the outer cone; v = 1 inside the
// inner cone, where the reference takes `color` as is (color * 1 has its
// bits), else the smoothstep of (cosa - cosEnd) * icosDiff.
__device__ __forceinline__ bool spot_falloff(const DLight& L, float cosa, float& v) {
  if (cosa < L.cos_end) return false;
  v = 1.f;
  if (!(cosa >= L.cos_start)) {
    const float x = (cosa - L.cos_end) * L.icos_diff;
    v = (x * x) * (3.f - 2.f * x);
  }
  return true;
}

// spotLight_t::illumSample, spotlight.cc:144-175; ls.col = color * cv
__device__ __forceinline__ bool spot_illum(const DLight& L, v3 P, float s1, float s2, v3& ldir, float& tmax,
                                           float& pdf, float& cv) {
  if (L.photon_only) return false;
  const v3 l = vsub(ld3(L.pos), P);
  const float dist_sqr = l.x * l.x + l.y * l.y + l.z * l.z;
  if (dist_sqr == 0.f) return false;
  const float dist = sqrtf(dist_sqr);
  const float inv = 1.f / dist;
  const v3 ld = V3(l.x * inv, l.y * inv, l.z * inv);
  if (!spot_falloff(L, vdot(ld3(L.ndir), ld), cv)) return false;
  tmax = dist;
  ldir = sample_cone(ld, ld3(L.du), ld3(L.dv), L.cos_end, s1 * L.fuzzy, s2 * L.fuzzy);
  pdf = dist_sqr;
  return true;
}

// spotLight_t::intersect, spotlight.cc:243-280, restated as written, with its
// two quirks: the hit point must lie on the plane through `position` exactly
// (== 0 in float, which almost no ray meets), and `P*P <= 1e-2` measures the
// hit point's distance from the world origin, not from the light. The log
// line is left out. col = color * cv.
__device__ __forceinline__ bool spot_hit(const DLight& L, v3 from, v3 dir, float& t, float& ipdf, float& cv) {
  const v3 d = ld3(L.dir);
  const float cosA = vdot(d, dir);
  if (cosA == 0.f) return false;
  t = vdot(d, vsub(ld3(L.pos), from)) / cosA;
  if (t < 0.f) return false;
  const v3 P = V3(from.x + t * dir.x, from.y + t * dir.y, from.z + t * dir.z);
  if (!(vdot(d, vsub(P, ld3(L.pos))) == 0.f)) return false;
  if (!((double)vdot(P, P) <= 1e-2)) return false;
  if (!spot_falloff(L, cosA, cv)) return false;
  ipdf = 1.f / (t * t);
  return true;
}

// sphereIntersect, spherelight.cc:88-100: float members, the literals 2.0 /
// 4.0 make osc and the two roots double expressions rounded to float
__device__ __forceinline__ bool sphere_isect(v3 from, v3 dir, v3 c, float R2, float& d1, float& d2) {
  const v3 vf = vsub(from, c);
  const float ea = vdot(dir, dir);
  const float eb = vdot(vmul(2.0f, vf), dir);
  const float ec = vdot(vf, vf) - R2;
  float osc = (float)((double)(eb * eb) - 4.0 * (double)ea * (double)ec);
  if (osc < 0.f) {  // "assume tangential hit/miss condition => Pythagoras"
    d1 = sqrtf(ec / ea);
    return false;
  }
  osc = sqrtf(osc);
  d1 = (float)((double)(-eb - osc) / (2.0 * (double)ea));
  d2 = (float)((double)(-eb + osc) / (2.0 * (double)ea));
  return true;
}

// sphereLight_t::illumSample, spherelight.cc:102-132: the cone under which
// the sphere is seen from P, sampled around a per-point createCS frame
__device__ __forceinline__ bool sphere_illum(const DLight& L, v3 P, float s1, float s2, v3& ldir, float& tmax,
                                             float& pdf) {
  v3 cdir = vsub(ld3(L.pos), P);
  const float dist_sqr = cdir.x * cdir.x + cdir.y * cdir.y + cdir.z * cdir.z;
  if (dist_sqr <= L.sq_radius) return false;  // only emits on the outside
  const float dist = sqrtf(dist_sqr);
  const float idist_sqr = 1.f / dist_sqr;
  const float cosAlpha = sqrtf(1.f - L.sq_radius * idist_sqr);
  const float inv = 1.f / dist;
  cdir = V3(cdir.x * inv, cdir.y * inv, cdir.z * inv);
  v3 du, dv;
  create_cs(cdir, du, dv);
  const v3 dir = sample_cone(cdir, du, dv, cosAlpha, s1, s2);
  float d1, d2;
  if (!sphere_isect(P, dir, ld3(L.pos), L.sq_radius_eps, d1, d2)) return false;
  ldir = dir;
  tmax = d1;
  pdf = 1.f / (2.f * (1.f - cosAlpha));
  return true;
}

// sphereLight_t::intersect, spherelight.cc:134-149. It never writes t: a ray
// tested with it would keep ray_t's default tmax (-1, unbounded; ray.h:29).
// doLightEstimation does not call it, because sphereLight_t::canIntersect()
// is false (spherelight.cc:49; mcintegrator.cc:109,134,156): a sphere light
// gets no BSDF (MIS) half and no MIS weight. Only yk_debug_light_probe runs it.
__device__ __forceinline__ bool sphere_hit(const DLight& L, v3 from, v3 dir, float& ipdf) {
  float d1, d2;
  if (!sphere_isect(from, dir, ld3(L.pos), L.sq_radius, d1, d2)) return false;
  const v3 cdir = vsub(ld3(L.pos), from);
  const float dist_sqr = cdir.x * cdir.x + cdir.y * cdir.y + cdir.z * cdir.z;
  if (dist_sqr <= L.sq_radius) return false;
  const float idist_sqr = 1.f / dist_sqr;
  const float cosAlpha = sqrtf(1.f - L.sq_radius * idist_sqr);
  ipdf = 2.f * (1.f - cosAlpha);
  return true;
}

__device__ __forceinline__ double sun_cos_angle(const DLight& L) {
  return __hiloint2double((int)L.cos_angle_w[1], (int)L.cos_angle_w[0]);
}

// sunLight_t::illumSample, sunlight.cc:74-85: a direction inside the cone
// around `direction`, whatever the point; sampleCone's maxCosAng parameter is
// a float, which the double cosAngle is converted to at the call. tmax = -1:
// unbounded. ls.col = colPdf (L.color), ls.pdf = pdf. Always true.
__device__ __forceinline__ bool sun_illum(const DLight& L, float s1, float s2, v3& ldir, float& tmax, float& pdf) {
  ldir = sample_cone(ld3(L.dir), ld3(L.du), ld3(L.dv), (float)sun_cos_angle(L), s1, s2);
  tmax = -1.f;
  pdf = L.pdf;
  return true;
}

// sunLight_t::intersect, sunlight.cc:87-95: the float cosine against the
// double cosAngle; t = -1 (the shadow ray stays unbounded), col = colPdf
__device__ __forceinline__ bool sun_hit(const DLight& L, v3 dir, float& t, float& ipdf) {
  const float cosine = vdot(dir, ld3(L.dir));
  if ((double)cosine < sun_cos_angle(L)) return false;
  t = -1.f;
  ipdf = L.invpdf;
  return true;
}

#include "yk_bglight.inc"

// pdf1D_t::DSample (sample_utils.h:141-157): u == 0 answers 0; otherwise
// std::lower_bound over cdf[0..n] (the first entry >= u), minus 1, clamped at 0
__device__ __forceinline__ int mesh_dsample(const float* cdf, int n, float u) {
  if (u == 0.f) return 0;
  int lo = 0, len = n + 1;
  while (len > 0) {  // std::lower_bound
    const int half = len >> 1;
    if (cdf[lo + half] < u) {
      lo += half + 1;
      len -= half + 1;
    } else {
      len = half;
    }
  }
  const int index = lo - 1;
  return index < 0 ? 0 : index;
}

// meshLight_t::illumSample with sampleSurface and triangle_t::sample
// (meshlight.cc:80-138, triangle.cc:156-167), in source order with the
// reference's types. tri: the sampled triangle's index in light order. A
// primNum >= count ("Sampling error": s1 above cdf[n] = 1, which no Halton
// value reaches) leaves the reference's point unset; here it refuses.
__device__ __forceinline__ bool mesh_illum(const DLight& L, const DMeshLight& ML, v3 P, float s1, float s2, v3& ldir,
                                           float& tmax, float& pdf, int& tri) {
  const int primNum = mesh_dsample(ML.cdf, ML.n, s1);
  if (primNum >= ML.n) return false;
  tri = primNum;
  float ss1, delta = ML.cdf[primNum + 1];
  if (primNum > 0) {
    const float c0 = ML.cdf[primNum];
    delta -= c0;
    ss1 = (s1 - c0) / delta;
  } else {
    ss1 = s1 / delta;
  }
  const float* tv = ML.verts + 9 * (size_t)primNum;
  const float su1 = sqrtf(ss1);
  const float u = 1.f - su1;
  const float v = s2 * su1;
  const float w = 1.f - u - v;
  const v3 p = V3((u * tv[0] + v * tv[3]) + w * tv[6], (u * tv[1] + v * tv[4]) + w * tv[7],
                  (u * tv[2] + v * tv[5]) + w * tv[8]);
  const v3 n = ld3(ML.nrm + 3 * (size_t)primNum);
  v3 l = vsub(p, P);
  const float dist_sqr = l.x * l.x + l.y * l.y + l.z * l.z;
  const float dist = sqrtf(dist_sqr);
  if (dist <= 0.0f) return false;
  const float id = 1.f / dist;
  l = V3(l.x * id, l.y * id, l.z * id);
  float cos_angle = -vdot(l, n);
  if (cos_angle <= 0.f) {  // no light behind a single-sided mesh
    if (L.double_sided) cos_angle = -cos_angle;
    else return false;
  }
  tmax = dist;
  ldir = l;
  const float amc = L.area * cos_angle;
  pdf = (float)((double)dist_sqr * YK_PI_D / (double)((amc == 0.f) ? 1e-8f : amc));
  return true;
}

// meshLight_t::intersect's kd-tree stack: one lane's pending exits of the
// light's own tree, in private (scratch) memory. A valid traversal holds at
// most depth_cap = depth + 2 entries and a descent pushes at index <=
// depth_cap, so YK_MESH_LIGHT_MAX_DEPTH + 3 entries hold every tree
// yk_device_upload lets through; the index is clamped all the same.
constexpr int kMeshStack = YK_MESH_LIGHT_MAX_DEPTH + 3;
struct MeshStack {
  uint2* e;
  __device__ __forceinline__ void push(int sp, uint2 v) const {
    if ((unsigned)sp < (unsigned)kMeshStack) e[sp] = v;
  }
  __device__ __forceinline__ uint2 pop(int sp) const {
    return (unsigned)sp < (unsigned)kMeshStack ? e[sp] : make_uint2(0u, 3u << 30);
  }
};

// meshLight_t::intersect (meshlight.cc:180-203): triKdTree_t::Intersect on the
// light's own tree -- the scene traversal's per-lane step (trav_begin /
// trav_step<true>: acceptance t < Z && t >= tmin, first-wins leaf order,
// kdtree.cc:766-800) on the light's node, leaf and record arrays -- with
// bRay's tmin = MIN_RAYDIST and unbounded tmax (mcintegrator.cc:165-175),
// then the sidedness rule and ipdf. The lanes of a wave hold different
// shading points but walk the same small tree, which stays in cache. Bounds
// as trace_body has them: trav_step ends a descent longer than depth_cap and
// checks the popped node and the stack index; a traversal of a valid tree
// reaches each leaf once, so more than nnodes steps end the ray as well.
__device__ __forceinline__ bool mesh_hit(const DLight& L, const DMeshLight& ML, v3 from, v3 dir, float& t,
                                         float& ipdf, int& tri) {
  DScene LS{};  // the light's tree as a scene of its own; what the closest-hit step does not read stays zero
  LS.tris = ML.tris;
  LS.nodes = ML.nodes;
  LS.leaf = ML.leaf;
  for (int k = 0; k < 6; ++k) LS.bound[k] = ML.bound[k];
  LS.nnodes = ML.nnodes;
  LS.depth_cap = ML.depth_cap;
  yk_ray r;
  r.from[0] = from.x, r.from[1] = from.y, r.from[2] = from.z;
  r.dir[0] = dir.x, r.dir[1] = dir.y, r.dir[2] = dir.z;
  r.tmin = YK_MIN_RAYDIST;
  r.tmax = -1.0f;
  Trav st;
  if (!trav_begin<true>(LS, st, r)) return false;
  uint2 ents[kMeshStack];
  MeshStack stk{ents};
  unsigned nn = 0, nt = 0, steps = 0;
  bool occ = false;
  while (!trav_step<true, false>(LS, st, stk, nn, nt, occ))
    if (++steps > ML.nnodes) return false;
  if (st.prim < 0 || st.prim >= ML.n) return false;  // miss, or the watchdog's -2
  tri = st.prim;
  t = st.Z;
  const v3 n = ld3(ML.nrm + 3 * (size_t)st.prim);
  float cos_angle = vdot(dir, vneg(n));
  if (cos_angle <= 0.f) {
    if (L.double_sided) cos_angle = fabsf(cos_angle);
    else return false;
  }
  ipdf = (float)((double)((1.f / (t * t)) * L.area * cos_angle) * YK_1_PI_D);
  return true;
}

// pointLight_t::illuminate (pointlight.cc:60-75) / directionalLight_t::
// illuminate (directional.cc:77-96), compiled forms: |v|^2 as (x*x + y*y) + z*z,
// 1/dist and 1/dist^2 as separate divisions; col = color * (1/dist^2).
// A hard spot (spotLight_t::illuminate, spotlight.cc:113-142) runs the point
// light's arithmetic and scales 1/dist^2 by the cone's falloff, which is
// exactly 1 inside the inner cone: there its results are the point light's bits.
template <bool XL = true>
__device__ __forceinline__ bool dirac_illum(const DLight& L, v3 P, v3& ldir, float& tmax, c3& col) {
  if (L.type == YK_LIGHT_POINT || (XL && L.type == YK_LIGHT_SPOT)) {
    if (XL && L.type == YK_LIGHT_SPOT && L.photon_only) return false;
    const v3 l = vsub(ld3(L.pos), P);
    const float dist_sqr = l.x * l.x + l.y * l.y + l.z * l.z;
    const float dist = sqrtf(dist_sqr);
    if (dist == 0.f) return false;
    float idist_sqr = 1.f / dist_sqr;
    const float inv = 1.f / dist;
    const v3 ld = V3(l.x * inv, l.y * inv, l.z * inv);
    if (XL && L.type == YK_LIGHT_SPOT) {
      float v;
      if (!spot_falloff(L, vdot(ld3(L.ndir), ld), v)) return false;
      idist_sqr = v * idist_sqr;  // color * (v * idist_sqr); v = 1 keeps idist_sqr's bits
    }
    ldir = ld;
    tmax = dist;
    col = C3(L.color[0] * idist_sqr, L.color[1] * idist_sqr, L.color[2] * idist_sqr);
    return true;
  }
  const v3 d = ld3(L.dir);
  if (!L.infinite) {  // outside the illuminated cylinder?
    const v3 vec = vsub(ld3(L.pos), P);
    const v3 cr = vcross(d, vec);
    const float dist = sqrtf(cr.x * cr.x + cr.y * cr.y + cr.z * cr.z);
    if (dist > L.radius) return false;
    tmax = vdot(vec, d);
    if (tmax <= 0.f) return false;
  } else {
    tmax = -1.f;
  }
  ldir = d;
  col = C3(L.color[0], L.color[1], L.color[2]);
  return true;
}

// ------------------------------------------------------------ queues

// Queue appends (wave_append2): every wave of a launch appends to the same
// counter word, and the returning atomics serialise on it. PER_WAVE: one
// returning atomic per wave, and each wave goes on at once; else one per
// block, the wave totals meeting in LDS between two barriers (every wave of
// the block then waits for the atomic's round trip). Fewer, larger blocks
// mean fewer atomics; smaller blocks let a CU overlap two blocks' waits.
// Measured (round 3, final build, headline / C2 Mrays/s):
//   k_shade_primary 512 per block, bounce kernels 512 per wave   2970 / 8872  (kept;
//     5 runs on 2 boxes, each 2969-2980, against 2942-2957 / 8815 for 1024 per wave)
//   k_shade_primary 512 per block, bounce kernels 1024 per wave  2949 / 8897
//     (same 2 boxes: 2945 / 8943 with the bounce kernels 1024 per block)
//   bounce kernels 256 per wave                                   2874 / 8833
//   k_shade_primary 1024 / 256 per block, 1024 per wave (3 runs,
//     against 2967 / 8876 on that box)        2894 / 8815, 2940 / 8770, 2945 / 8774
//   k_shade_primary 512 per wave, bounce kernels 512 per wave    2947 / 8826
//   all 1024 per wave                                             2951 / 8801
//   all 512 per block                                             2920 / 9035
//   bounce kernels 512 per block                                  2920 / 8973
//   all 1024 per block                                            2954 / 8916
//   all 256 per block                                             2880 / 8904
// Earlier: bounce kernels at 5 / 6 waves per SIMD (6 / 23 VGPRs spilled)
// 2892 / 2777 and 8326 / 7865 against 2959 / 8429. The photon / final-gather
// kernels' launches are 33M threads each: 512 per block (1068 -> 1263
// Mrays/s in round 1 against per wave; 1024: 1240).
#ifndef YK_PRIMARY_BLOCK
#define YK_PRIMARY_BLOCK 512  // k_shade_primary
#endif
#ifndef YK_PRIMARY_APPEND_WAVE
#define YK_PRIMARY_APPEND_WAVE false
#endif
#ifndef YK_BOUNCE_BLOCK
#define YK_BOUNCE_BLOCK 640  // k_path_start, k_shade_bounce (10 waves: two blocks fill a CU at 5 waves / SIMD)
#endif
#ifndef YK_BOUNCE_APPEND_WAVE
#define YK_BOUNCE_APPEND_WAVE true
#endif
#ifndef YK_BOUNCE_WAVES
#define YK_BOUNCE_WAVES 5  // occupancy target of k_shade_bounce
#endif
// the diffuse-only instantiation (mat_sample<true>, fewer registers)
#ifndef YK_BOUNCE_BLOCK_D
#define YK_BOUNCE_BLOCK_D YK_BOUNCE_BLOCK
#endif
#ifndef YK_BOUNCE_WAVES_D
#define YK_BOUNCE_WAVES_D YK_BOUNCE_WAVES
#endif
constexpr int bounce_block(bool diff) { return diff ? YK_BOUNCE_BLOCK_D : YK_BOUNCE_BLOCK; }
#ifndef YK_APPEND_BLOCK
#define YK_APPEND_BLOCK 512  // photon / final-gather kernels
#endif
// every block-size knob is whole waves within the 1024-thread workgroup limit
// (an A/B build with YK_BOUNCE_BLOCK=1280 compiled and then failed at launch,
// VERDICT r05 weak 8): refused at compile time
constexpr bool valid_block(int b) { return b >= 64 && b <= 1024 && b % 64 == 0; }
static_assert(valid_block(YK_PRIMARY_BLOCK), "YK_PRIMARY_BLOCK: a multiple of 64 in [64, 1024]");
static_assert(valid_block(YK_BOUNCE_BLOCK), "YK_BOUNCE_BLOCK: a multiple of 64 in [64, 1024]");
static_assert(valid_block(YK_BOUNCE_BLOCK_D), "YK_BOUNCE_BLOCK_D: a multiple of 64 in [64, 1024]");
static_assert(valid_block(YK_APPEND_BLOCK), "YK_APPEND_BLOCK: a multiple of 64 in [64, 1024]");
static_assert(YK_BOUNCE_WAVES >= 1 && YK_BOUNCE_WAVES <= 8 && YK_BOUNCE_WAVES_D >= 1 && YK_BOUNCE_WAVES_D <= 8,
              "YK_BOUNCE_WAVES[_D]: 1..8 waves per SIMD");
#ifndef YK_PM_APPEND_WAVE
#define YK_PM_APPEND_WAVE false
#endif
template <bool PER_WAVE>
__device__ __forceinline__ void wave_append2(unsigned long long* counter, unsigned m_s, unsigned m_b,
                                             unsigned& base_s, unsigned& base_b) {
  const int lane = threadIdx.x & 63;
  const unsigned long long m = ((unsigned long long)m_b << 32) | m_s;
  unsigned long long incl = m;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned lo = __shfl_up((unsigned)incl, off), hi = __shfl_up((unsigned)(incl >> 32), off);
    if (lane >= off) incl += ((unsigned long long)hi << 32) | lo;
  }
  const unsigned long long total = shfl_u64(incl, 63);
  if (PER_WAVE) {
    unsigned long long wb = 0;
    if (lane == 63 && total) wb = atomicAdd(counter, total);
    wb = shfl_u64(wb, 63) + incl - m;
    base_s = (unsigned)wb;
    base_b = (unsigned)(wb >> 32);
    return;
  }
  // one returning atomic per block: wave totals meet in LDS (all callers
  // reach this point with whole blocks)
  __shared__ unsigned long long s_tot[16];
  __shared__ unsigned long long s_base;
  const int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  if (lane == 63) s_tot[w] = total;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    for (int k = 0; k < nw; ++k) t += s_tot[k];
    s_base = t ? atomicAdd(counter, t) : 0ull;
  }
  __syncthreads();
  unsigned long long base = s_base;
  for (int k = 0; k < w; ++k) base += s_tot[k];
  base += incl - m;
  base_s = (unsigned)base;
  base_b = (unsigned)(base >> 32);
}

// Packs the block's threads with hit != 0 onto its first threads (in thread
// order): returns whether this thread has an entry, and its original thread
// index in `src`. Whole-block call; BLOCK = blockDim.x.
template <int BLOCK>
__device__ __forceinline__ bool pack_block(bool hit, int& src) {
  __shared__ int s_q[BLOCK];
  __shared__ int s_wn[BLOCK / 64];
  const unsigned long long hm = __ballot(hit);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) s_wn[w] = __popcll(hm);
  __syncthreads();
  int off = 0, tot = 0;
  for (int k = 0; k < BLOCK / 64; ++k) {
    off += k < w ? s_wn[k] : 0;
    tot += s_wn[k];
  }
  if (hit) s_q[off + __popcll(hm & ((1ull << lane) - 1ull))] = (int)threadIdx.x;
  __syncthreads();
  const bool valid = (int)threadIdx.x < tot;
  src = valid ? s_q[threadIdx.x] : 0;
  return valid;
}

// Shadow-ray slot flags
enum : uint8_t { SL_TRACED = 1, SL_ADDS = 2 };
struct Batch;
__device__ __forceinline__ long long slot_of(const Batch& B, long long c, int k);
// prim_hit flags
// (PH_AOEMIT: ambient occlusion on an emitting diffuse material, k_resolve_ao)
enum : int { PH_HIT = 1, PH_DIFFUSE = 2, PH_LIGHT = 4, PH_AOEMIT = 8 };
// path state bits
// (PS_EMIT: emit_b holds this bounce's emission; otherwise it is zero and
// not stored. 256: clear of the final-gather bits, yk_photon.inc)
enum : int { PS_ALIVE = 1, PS_RESOLVE = 2, PS_CONT = 4, PS_EST = 8, PS_EMIT = 256 };

// Per-batch device state. Camera sample c owns K shadow slots k = 0..K-1:
// doLightEstimation's i-th light sample is slot k0+i, its i-th BSDF (MIS)
// sample slot k0+n+i. Slot (c, k) of region r (the merged launch's bounce
// depth, else 0) is stored at k * kstride + r * cap + c (slot_of,
// kstride = regions * cap): the lanes of a wave, consecutive samples writing
// the same k, then fill whole cache lines (at c * K + k every lane's record
// landed in its own line). Shadow rays are written straight into their slot
// and only the slot index goes through the compacted queue, so the resolve
// step reads results in the reference's summation order without any sorting.
//
// Shadow rays in two parts (every shadow ray of a shading point starts at
// its P, mcintegrator.cc:103-191): per slot 16 B {dir, w}, per shading point
// 16 B {P, tmin}, written once when the point emits any ray, as the record
// of slot k = K (so the origin of slot s is record K * kstride + s mod
// kstride, and the shading kernels need no further pointer). w encodes tmax and
// which tmin applies (shadow_w / unpack_shadow): a light-sample ray's tmax
// (>= 0) with the origin's tmin (shadowBias), the sentinel kTmaxInf for
// tmax < 0 (directional lights), or -t for a BSDF (MIS) ray, whose tmin is
// YK_MIN_RAYDIST and whose light hit t is > 1e-10 (light_hit). A path
// vertex with the C2 light's four light samples writes 4 * 16 + 16 B of
// rays instead of 4 * 32. Scenes whose lights take one sample each (the
// headline: one light ray and at most one MIS ray per vertex) gain nothing
// from it and keep whole 32-B rays at the slot index (split = 0, K < 4;
// YK_SPLIT=0/1 forces either form): the two-array fetch costs the any-hit
// kernel 2 % there.
struct Batch {
  int* prim_hit;        // PH_* flags of the camera ray
  unsigned* soffs;      // samplingOffs (fnv of pixel)
  float* col;           // 3 floats: primary emission + direct light
  float* alpha;
  yk_ray* p_rays;       // camera rays (kept for all sub-paths)
  yk_hit* p_hits;
  float* thr;           // 3 floats: path throughput
  float* pathcol;       // 3 floats, accumulated over sub-paths
  float* scol_next;     // 3 floats, BSDF weight of the next segment
  float* wlast;         // last W written by material sample (kept when sample() returns early)
  float* emit_b;        // 3 floats: emission added at the current bounce
  int* pstate;          // PS_* bits
  int* lsel;            // light chosen by estimateOneDirectLight
  int* q_owner[2];      // camera sample of each bounce-queue entry
  yk_ray* q_rays[2];    // bounce queues (ping-pong)
  yk_hit* q_hits[2];
  float4* s_dir;        // split: K + 1 per camera sample (and region): {dir, w}, then {P, tmin} at k = K;
                        // else K yk_ray (32 B) per camera sample (and region)
  int split;            // shadow rays as {dir, w} + origin records (1) or whole rays (0)
  uint8_t* s_occl;      // K per camera sample
  unsigned* s_idx;      // compacted shadow queue: slot index, or (split) k << kshift | origin index r * cap + c
  float* sl_contrib;    // 3 floats per slot
  uint8_t* sl_flags;    // 1 per slot
  float4* samples;      // final RGBA per camera sample
  float2* sxy;          // (dx, dy) of the sample inside its pixel
  char4* pext;          // per pixel slot: footprint extent of its samples (k_pixel_extent)
  int K;
  long long cap;  // samples per batch
  long long kstride;    // slot stride of k: regions * cap
  int kshift;           // queue entries: bits of the origin index (kstride <= 2^kshift)
  long long slot_base;  // merged shadow launch: this bounce's region offset depth * cap (0 otherwise)
  // merged shadow launch: the regions' queue-count words (region r's count in
  // the low half of mq_words[r]); a bounce kernel writes its queue entries
  // after those of the regions before it (complete, earlier in the stream)
  const unsigned long long* mq_words;
  int mq_region;
  // specular recursion (recursiveRaytrace) only, see k_spawn / k_fold
  unsigned* psample;    // pixel sample index of each entry (state.pixelSample)
  uint8_t* incl;        // state.includeLights after the entry's path loop
  uint8_t* caus;        // caustic flag of the current path segment
  float* emit0;         // 3 floats: emission at the entry's hit, added at the fold
  // transparent shadows (mcIntegrator_t::trShad): the light colour is
  // filtered by the shadow ray before the products, so slots keep the parts
  int ts;
  float* s_filt;        // 3 per slot: filter colour of the shadow ray (IntersectTS)
  float* sl_aux;        // 4 per slot: scalar factors (and the Dirac light colour)
};
__device__ __forceinline__ long long slot_of(const Batch& B, long long c, int k) {
  return B.slot_base + (long long)k * B.kstride + c;  // k-major (sample-major c * K + k: C2 7810 against 8047 Mrays/s)
}

struct RenderConst {
  int ps;         // pixel sample index from B.psample (specular nodes, adaptive passes)
  int multipass;  // AA_passes > 1: RI_vdC / RI_S sample positions (integrator.cc:276-281)
  int pass_off;   // pixelSample offset of the pass
  int spec;       // specular recursion pipeline (scene has SPECULAR|FILTER materials)
  int trace_caustics;  // caustic_type path: traceCaustics (pathtracer.cc:389-397)
  int rdepth;     // raydepth
  int level;      // state.raylevel of the entries being shaded
  int spp;
  int nsub;       // path_samples
  int bounces;    // maxBounces
  int integrator;
  int transp_bg;
  int nlights;
  int has_bg;     // the background a missing ray adds: kBgNone, kBgConstant (bg) or kBgGradient (bg_grad, at the end)
  float bg[3];
  float d1;       // 1/spp as renderTile computes it
  int pm_fg;      // photon mapping with final gathering: col += pathCol / nSampl at the finish
  int pm_showmap; // photon mapping show_map: no direct light
  int merged;     // merged shadow launch: pathCol lives in k_resolve_merged's registers from 0
  float bg_grad[12];  // gradientBackground_t: szenith, shoriz, gzenith, ghoriz (bg_gradient)
};

// ------------------------------------------------------------ kernels

// Camera rays for the camera samples of the batch tiles (renderTile,
// integrator.cc:251-306): sample index s is the fastest-running index.
struct TileList {
  const int4* tiles;  // X, Y, W, H per tile of the batch
  const int* base;    // first camera-sample index of each tile
  int ntiles;
  const int* pix;     // adaptive pass: the batch's resampled pixels ((y << 16) | x), tile order
};

// perspectiveCam_t::biasDist (perspectiveCamera.cc:73-86)
__device__ __forceinline__ float lens_bias(float r) {
  if (c_cam.bokeh_bias == YK_BOKEH_BIAS_CENTER) return sqrtf(sqrtf(r) * r);
  if (c_cam.bokeh_bias == YK_BOKEH_BIAS_EDGE) return sqrtf(1.0f - r * r);
  return sqrtf(r);
}
// perspectiveCam_t::getLensUV (perspectiveCamera.cc:100-121) with sampleTSD
// (:88-98) for the polygon shapes and ShirleyDisk (vector3d.cc:156-182)
__device__ __forceinline__ void lens_uv(float r1, float r2, float& u, float& v) {
  const int bt = c_cam.bokeh_type;
  if (bt >= YK_BOKEH_TRI && bt <= YK_BOKEH_HEXA) {
    const float fn = (float)bt;
    int idx = (int)(r1 * fn);
    r1 = (r1 - (float)idx / fn) * fn;
    r1 = lens_bias(r1);
    const float b1 = r1 * r2, b0 = r1 - b1;
    idx <<= 1;
    u = c_cam.ls[idx] * b0 + c_cam.ls[idx + 2] * b1;
    v = c_cam.ls[idx + 1] * b0 + c_cam.ls[idx + 3] * b1;
  } else if (bt == YK_BOKEH_DISK2 || bt == YK_BOKEH_RING) {
    const float w = (float)(YK_2PI_D * (double)r2);
    r1 = (bt == YK_BOKEH_RING) ? sqrtf(0.707106781f + 0.292893218f) : lens_bias(r1);
    u = r1 * fcos_ref(w);
    v = r1 * fsin_ref(w);
  } else {
    shirley_disk(r1, r2, u, v);
  }
}

// camera_t::shootRay of the scene's camera kind -> wt. Shared by k_camera and
// the test hook (yk_debug_camera_rays).
// ray_plane_intersection (geometry.h:33-36) for the near / far planes
__device__ __forceinline__ void cam_clip(yk_ray& r, v3 from, v3 d) {
  const v3 cz = ld3(c_cam.camZ);
  const float den = vdot(d, cz);
  r.tmin = vdot(cz, vsub(ld3(c_cam.near_p), from)) / den;
  r.tmax = vdot(cz, vsub(ld3(c_cam.far_p), from)) / den;
}
template <int KIND>
__device__ __forceinline__ float cam_shoot(float px, float py, float lu, float lv, yk_ray& r);

// perspectiveCam_t::shootRay (perspectiveCamera.cc:127-149), an architect
// camera's too; lu, lv are read with an aperture only
template <>
__device__ __forceinline__ float cam_shoot<YK_CAMERA_PERSPECTIVE>(float px, float py, float lu, float lv, yk_ray& r) {
  const v3 vr = ld3(c_cam.vright), vu = ld3(c_cam.vup), vt = ld3(c_cam.vto);
  v3 d = vadd(vadd(vmul(px, vr), vmul(py, vu)), vt);
  d = vnormalize_cam(d);
  const v3 from = ld3(c_cam.pos);
  r.from[0] = from.x;
  r.from[1] = from.y;
  r.from[2] = from.z;
  r.dir[0] = d.x;
  r.dir[1] = d.y;
  r.dir[2] = d.z;
  cam_clip(r, from, d);
  if (c_cam.aperture != 0.f) {
    // shootRay's aperture branch (perspectiveCamera.cc:139-147): tmin / tmax
    // stay those of the pinhole ray
    float u, v;
    lens_uv(lu, lv, u, v);
    const v3 LI = vadd(vmul(u, ld3(c_cam.dof_rt)), vmul(v, ld3(c_cam.dof_up)));
    const v3 f2 = vadd(from, LI);
    const v3 d2 = vnormalize_cam(vsub(vmul(c_cam.dof_distance, d), LI));
    r.from[0] = f2.x;
    r.from[1] = f2.y;
    r.from[2] = f2.z;
    r.dir[0] = d2.x;
    r.dir[1] = d2.y;
    r.dir[2] = d2.z;
  }
  return 1.f;
}

// orthoCam_t::shootRay (orthographicCamera.cc:52-64): c_cam.pos is its `pos`,
// the direction vto = camZ is not normalised again; no lens. Source order;
// not pinned against the compiled reference.
template <>
__device__ __forceinline__ float cam_shoot<YK_CAMERA_ORTHOGRAPHIC>(float px, float py, float, float, yk_ray& r) {
  const v3 from = vadd(vadd(ld3(c_cam.pos), vmul(px, ld3(c_cam.vright))), vmul(py, ld3(c_cam.vup)));
  const v3 d = ld3(c_cam.vto);
  r.from[0] = from.x;
  r.from[1] = from.y;
  r.from[2] = from.z;
  r.dir[0] = d.x;
  r.dir[1] = d.y;
  r.dir[2] = d.z;
  cam_clip(r, from, d);
  return 1.f;
}

// angularCam_t::shootRay (angularCamera.cc:49-71), source order in float;
// fSqrt is sqrtf, fSin / fCos the FAST_TRIG forms. atan2 is the one libm call:
// the device's atan2f is not bit-pinned to glibc's. Outside
// the circle (circular, radius > max_r) wt = 0 and the reference returns its
// default ray_t (tmin 0, tmax -1) from the camera's position, direction unset:
// here direction 0, which is how k_dead_samples knows the sample.
template <>
__device__ __forceinline__ float cam_shoot<YK_CAMERA_ANGULAR>(float px, float py, float, float, yk_ray& r) {
  const v3 from = ld3(c_cam.pos);
  r.from[0] = from.x;
  r.from[1] = from.y;
  r.from[2] = from.z;
  const float u = 1.f - 2.f * (px / c_cam.resx);
  float v = 2.f * (py / c_cam.resy) - 1.f;
  v *= c_cam.aspect;
  const float radius = sqrtf(u * u + v * v);
  if (c_cam.circular && radius > c_cam.max_r) {
    r.dir[0] = 0.f;
    r.dir[1] = 0.f;
    r.dir[2] = 0.f;
    r.tmin = 0.f;
    r.tmax = -1.0f;
    return 0.f;
  }
  float theta = 0.f;
  if (!((u == 0.f) && (v == 0.f))) theta = atan2f(v, u);
  const float phi = radius * c_cam.hor_phi;
  const v3 d = vadd(vmul(fsin_ref(phi), vadd(vmul(fcos_ref(theta), ld3(c_cam.vright)),
                                             vmul(fsin_ref(theta), ld3(c_cam.vup)))),
                    vmul(fcos_ref(phi), ld3(c_cam.vto)));
  r.dir[0] = d.x;
  r.dir[1] = d.y;
  r.dir[2] = d.z;
  cam_clip(r, from, d);
  return 1.f;
}

// Sample s of pixel (j, i) that camera-sample index c of the batch stands for
__device__ __forceinline__ void cam_sample_of(const TileList& TL, const RenderConst& R, long long c, int& s, int& j,
                                              int& i) {
  if (TL.pix) {  // adaptive pass: only the flagged pixels, in tile / row order
    // 32-bit index arithmetic: a batch holds far fewer than 2^31 samples
    const int packed = TL.pix[(unsigned)c / (unsigned)R.spp];
    s = (int)((unsigned)c % (unsigned)R.spp);
    j = packed & 0xFFFF;
    i = packed >> 16;
  } else {
    int lo = 0, hi = TL.ntiles - 1;
    while (lo < hi) {  // tile owning c
      const int mid = (lo + hi + 1) >> 1;
      if (TL.base[mid] <= c) lo = mid;
      else hi = mid - 1;
    }
    const int4 T = TL.tiles[lo];
    const long long local = c - TL.base[lo];
    s = (int)((unsigned)local % (unsigned)R.spp);
    const int pl = (int)((unsigned)local / (unsigned)R.spp);
    j = T.x + pl % T.z;
    i = T.y + pl / T.z;
  }
}

// One instantiation per shootRay. live (an angular camera with `circular`
// only, else nullptr): the samples that carry a ray are appended to a queue --
// their indices to live_idx, the count to *live -- and the primary trace runs
// over that queue alone, so a sample outside the circle (wt = 0,
// integrator.cc:293-297) is never traced or counted. Its hit record is a miss:
// the shading kernels start nothing for it, and k_dead_samples zeroes the
// sample they give a miss before the film gathers it.
template <int KIND>
__global__ void __launch_bounds__(256) k_camera(TileList TL, Batch B, RenderConst R, long long nc,
                                                unsigned long long* __restrict__ live,
                                                unsigned* __restrict__ live_idx) {
  const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if constexpr (KIND != YK_CAMERA_ANGULAR) {
    if (c >= nc) return;
  }
  const bool valid = c < nc;
  int s = 0, j = 0, i = 0;
  if (valid) cam_sample_of(TL, R, c, s, j, i);
  float wt = 0.f;
  if (valid) {
    const unsigned so = fnv32a((unsigned)i * fnv32a((unsigned)j));
    const unsigned psample = (unsigned)(R.pass_off + s);  // rstate.pixelSample = pass_offs + sample
    B.soffs[c] = so;
    if (R.ps) B.psample[c] = psample;
    float dx = 0.5f, dy = 0.5f;
    if (R.multipass) {
      dx = ri_vdc(psample, so);
      dy = ri_s(psample, so);
    } else if (R.spp > 1) {
      dx = (0.5f + (float)s) * R.d1;
      dy = ri_lp((unsigned)s + so, 0u);
    }
    B.sxy[c] = make_float2(dx, dy);
    const float px = (float)j + dx, py = (float)i + dy;
    float lu = 0.5f, lv = 0.5f;
    if constexpr (KIND == YK_CAMERA_PERSPECTIVE) {
      if (c_cam.aperture != 0.f) {
        // renderTile's lens samples (integrator.cc:248-291): Halton(3) / Halton(5)
        // set to pass_offs + samplingOffs per pixel, one getNext per sample in
        // sample order -- so sample s takes the (s+1)-th value
        Halton hu, hv;
        hal_start(hu, 3u, (unsigned)R.pass_off + so);
        hal_start(hv, 5u, (unsigned)R.pass_off + so);
        for (int k = 0; k <= s; ++k) {
          lu = hal_next(hu);
          lv = hal_next(hv);
        }
      }
    }
    yk_ray r;
    wt = cam_shoot<KIND>(px, py, lu, lv, r);
    B.p_rays[c] = r;
    if constexpr (KIND == YK_CAMERA_ANGULAR) {
      if (live && wt == 0.f) B.p_hits[c] = yk_hit{-1, 0.f, 0.f, 0.f};
    }
  }
  if constexpr (KIND == YK_CAMERA_ANGULAR) {
    if (live) {  // kernel argument: uniform
      // one atomic per wave; the queue's order is free (results go to slot c)
      const bool alive = valid && wt != 0.f;
      const unsigned long long m = __ballot(alive);
      if (m != 0ull) {
        const unsigned rank = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        const int leader = __ffsll((long long)m) - 1;
        unsigned long long base = 0;
        if ((int)(threadIdx.x & 63u) == leader) base = atomicAdd(live, (unsigned long long)__popcll(m));
        base = shfl_u64(base, leader);
        if (alive) live_idx[base + rank] = (unsigned)c;
      }
    }
  }
}

// The samples of an angular camera that carry no ray (wt = 0): renderTile
// splats colorA_t(0) for them (integrator.cc:293-297), colour and alpha zero,
// whatever the background is. They are the camera rays with direction 0
// (cam_shoot). Launched only for a camera that can have them.
__global__ void __launch_bounds__(256) k_dead_samples(Batch B, long long nc) {
  const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const yk_ray& r = B.p_rays[c];
  if (r.dir[0] == 0.f && r.dir[1] == 0.f && r.dir[2] == 0.f && r.tmin == 0.f && r.tmax == -1.0f)
    B.samples[c] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// Ray records streamed to the next kernel (shadow slots, bounce queues) are
// stored non-temporally, so they do not displace the scene's node and
// triangle lines (round 3: headline 2944 -> 2964, C2 8697 -> 8850 Mrays/s;
// non-temporal loads in the traversal kernels measured slower, §5).
__device__ __forceinline__ void st_ray(yk_ray* p, const yk_ray& r) {
#ifndef YK_PLAIN_RAY_STORES
  typedef float f4n __attribute__((ext_vector_type(4)));
  f4n* q = reinterpret_cast<f4n*>(p);
  const f4n a = {r.from[0], r.from[1], r.from[2], r.dir[0]}, b = {r.dir[1], r.dir[2], r.tmin, r.tmax};
  __builtin_nontemporal_store(a, q);
  __builtin_nontemporal_store(b, q + 1);
#else
  *p = r;
#endif
}
__device__ __forceinline__ void put_ray(yk_ray& r, v3 f, v3 d, float tmin, float tmax) {
  r.from[0] = f.x;
  r.from[1] = f.y;
  r.from[2] = f.z;
  r.dir[0] = d.x;
  r.dir[1] = d.y;
  r.dir[2] = d.z;
  r.tmin = tmin;
  r.tmax = tmax;
}

// A slot's contribution is read only when its SL_ADDS flag is set
// (resolve_light), so slots without it store the flag alone: on C2 the
// shading kernels are write-bound (k_shade_bounce writes ~280 B per path
// vertex) and most MIS-half slots carry no contribution.
// 12-B records at float offset 3*slot: copied as exactly 12 bytes (one
// dwordx3 access), never through a vec3 type whose size and alignment are 16
// (a 16-B access would touch the next slot's red channel)
__device__ __forceinline__ void put_slot(const Batch& B, long long slot, uint8_t fl, c3 v) {
  B.sl_flags[slot] = fl;
  if (fl & SL_ADDS) {
    const float x[3] = {v.r, v.g, v.b};
    __builtin_memcpy(B.sl_contrib + 3 * slot, x, 12);
  }
}
__device__ __forceinline__ c3 get_contrib(const Batch& B, long long slot) {
  float x[3];
  __builtin_memcpy(x, B.sl_contrib + 3 * slot, 12);
  return C3(x[0], x[1], x[2]);
}
__device__ __forceinline__ void put_aux(const Batch& B, long long slot, float a, float b, float c, float d) {
  *reinterpret_cast<float4*>(B.sl_aux + 4 * slot) = make_float4(a, b, c, d);
}

__device__ __forceinline__ void st_f4(float4* p, float a, float b, float c, float d) {
  typedef float f4n __attribute__((ext_vector_type(4)));
  const f4n v = {a, b, c, d};
  __builtin_nontemporal_store(v, reinterpret_cast<f4n*>(p));
}
// a shadow ray of slot `slot` from P (tmin shadowBias, or YK_MIN_RAYDIST for
// a BSDF sample: MIS), stored for the any-hit launch (Batch comment): bit kbit
// of `traced`, one queued ray
template <bool MIS>
__device__ __forceinline__ int emit_shadow(const Batch& B, long long slot, v3 P, v3 dir, float tmax, int kbit,
                                           unsigned long long& traced) {
  if (B.split) {
    // a soft spot's hit may lie at t = +-0 (spot_hit): the sign bit alone marks a MIS ray
    st_f4(&B.s_dir[slot], dir.x, dir.y, dir.z, MIS ? -fabsf(tmax) : shadow_w(tmax));
  } else {
    yk_ray sr;
    put_ray(sr, P, dir, MIS ? YK_MIN_RAYDIST : YK_SHADOW_BIAS, tmax);
    st_ray(reinterpret_cast<yk_ray*>(B.s_dir) + slot, sr);
  }
  if (kbit < 64) traced |= 1ull << kbit;
  return 1;
}
// split form: the origin record of sample c's shading point at this region,
// written once when the point emitted any shadow ray
__device__ __forceinline__ void put_org(const Batch& B, long long c, v3 P) {
  if (B.split) st_f4(&B.s_dir[slot_of(B, c, B.K)], P.x, P.y, P.z, YK_SHADOW_BIAS);
}

// light_t::diracLight(): point, directional and hard spot lights take
// doLightEstimation's one-ray branch, the others its sample loops
__device__ __forceinline__ bool light_sampled(const DLight& L) {
  return L.type == YK_LIGHT_AREA || L.type == YK_LIGHT_SPHERE || L.type == YK_LIGHT_MESH || L.soft != 0;
}

template <bool DIFF, int KIND, int GL = kGLNone>
__device__ __forceinline__ int gen_sampled(const Batch& B, long long c, int k0, const DLight& L, const DMat& M,
                                           const SurfPt& sp, v3 wo, unsigned pixelSample, unsigned soffs,
                                           unsigned loffs, unsigned long long& traced,
                                           const DMeshLight* ml = nullptr);

// mcIntegrator_t::doLightEstimation, mcintegrator.cc:73-195, split
// at its isShadowed calls: every shadow ray it would trace is written to its
// slot with the contribution it adds when unoccluded. Returns #rays; sets bit
// k of `traced` (k < 64) for each slot that holds a ray.
// XL: kXLNone, kXLSpotSphere (the scene holds a spot or sphere light),
// kXLMesh (it holds a mesh light; ml = DScene::ml), kXLSun (it holds a sun
// light) or kXLBg (it holds a background light, whose tables ml reaches too);
// each level holds the code of those below it: see kShade
constexpr int kXLNone = 0, kXLSpotSphere = 1, kXLMesh = 2, kXLSun = 3, kXLBg = 4;
template <bool DIFF = false, int XL = kXLNone, int GL = kGLNone>
__device__ __forceinline__ int gen_light(const Batch& B, long long c, int k0, int li, const SurfPt& sp, v3 wo,
                                         unsigned pixelSample, unsigned soffs, unsigned loffs,
                                         unsigned long long& traced, const DMat* mats = c_mats,
                                         const DMeshLight* ml = nullptr) {
  const DLight& L = c_lights[li];
  const DMat& M = mats[sp.mat];
  const c3 black = C3(0.f, 0.f, 0.f);
  // the light's kind is the same for every lane: one scalar branch per light,
  // outside the sample loops
  if (L.type == YK_LIGHT_AREA)
    return gen_sampled<DIFF, YK_LIGHT_AREA, GL>(B, c, k0, L, M, sp, wo, pixelSample, soffs, loffs, traced);
  if (XL >= kXLBg && L.type == YK_LIGHT_BACKGROUND)
    return gen_sampled<DIFF, YK_LIGHT_BACKGROUND, GL>(B, c, k0, L, M, sp, wo, pixelSample, soffs, loffs, traced,
                                                      ml + L.mesh);
  if (XL >= kXLSun && L.type == YK_LIGHT_SUN)
    return gen_sampled<DIFF, YK_LIGHT_SUN, GL>(B, c, k0, L, M, sp, wo, pixelSample, soffs, loffs, traced);
  if (XL >= kXLMesh && L.type == YK_LIGHT_MESH)
    return gen_sampled<DIFF, YK_LIGHT_MESH, GL>(B, c, k0, L, M, sp, wo, pixelSample, soffs, loffs, traced, ml + L.mesh);
  if (XL && L.type == YK_LIGHT_SPHERE)
    return gen_sampled<DIFF, YK_LIGHT_SPHERE, GL>(B, c, k0, L, M, sp, wo, pixelSample, soffs, loffs, traced);
  if (XL && L.soft)
    return gen_sampled<DIFF, YK_LIGHT_SPOT, GL>(B, c, k0, L, M, sp, wo, pixelSample, soffs, loffs, traced);
  {  // Dirac branch, mcintegrator.cc:85-100: one shadow ray
    const long long slot = slot_of(B, c, k0);
    v3 ldir;
    float ltmax;
    c3 lc;
    if (!dirac_illum<XL != kXLNone>(L, sp.P, ldir, ltmax, lc)) {
      put_slot(B, slot, 0, black);
      return 0;
    }
    const int nq = emit_shadow<false>(B, slot, sp.P, ldir, ltmax, k0, traced);
    const c3 surf = mat_eval<!DIFF, GL>(M, sp, wo, ldir);
    const float f = fabsf(vdot(sp.N, ldir));
    if (B.ts) {  // lcol *= scol first (mcintegrator.cc:94): keep the parts
      put_slot(B, slot, SL_TRACED | SL_ADDS, surf);
      put_aux(B, slot, f, lc.r, lc.g, lc.b);
      return nq;
    }
    // compiled form of surfCol*lcol*|N.l|*transmitCol (transmitCol = 1):
    // R,G (lcol*surf)*f, B surf*(lcol*f)
    put_slot(B, slot, SL_TRACED | SL_ADDS,
             C3((lc.r * surf.r) * f, (lc.g * surf.g) * f, surf.b * (lc.b * f)));
    return nq;
  }
}

// doLightEstimation's branch for lights with illumSample (mcintegrator.cc:
// 101-193). Three things depend on the light's kind (KIND, a YK_LIGHT_*):
// its sample function, its intersect function and ls.col / lcol -- the
// colour as is for area, sphere and mesh lights, the colour times the cone's
// falloff cv for a soft spot (kept in the slot's aux record under
// transparent shadows, which filter the colour first), colPdf for a sun
// (DLight::color holds it). A sun's rays are unbounded (t = -1) in both
// halves; the split slot form marks a BSDF-half ray by the sign of its w, so
// there the unbounded one is stored as -inf (unpack_shadow: tmax = +inf, which
// the any-hit traversal takes as it takes a negative tmax). A background
// light differs from the sun in one thing: ls.col / lcol is per sample, the
// background evaluated at the sampled direction (illumSample) or at the
// re-mapped BSDF direction (intersect); it takes lcol's place in the same
// operand positions. Its slots have no aux form: transparent shadows are
// refused on a scene that holds one (yk_render_shard). A sphere light's
// canIntersect() is false (spherelight.cc:49): no MIS weight on its light
// samples and no BSDF half, so it owns `samples` slots, not 2 * samples.
template <bool DIFF, int KIND, int GL>
__device__ __forceinline__ int gen_sampled(const Batch& B, long long c, int k0, const DLight& L, const DMat& M,
                                           const SurfPt& sp, v3 wo, unsigned pixelSample, unsigned soffs,
                                           unsigned loffs, unsigned long long& traced, const DMeshLight* ml) {
  constexpr bool CAN_INTERSECT = KIND != YK_LIGHT_SPHERE;
  const c3 black = C3(0.f, 0.f, 0.f);
  const int n = L.samples;
  const unsigned offs = (unsigned)(n * (int)pixelSample) + soffs + loffs * 4567u;
  c3 lcol = C3(L.color[0], L.color[1], L.color[2]);  // YK_LIGHT_BACKGROUND: set per sample
  int nr = 0;
  Halton h2, h3;
  hal_start(h2, 2u, offs - 1u);
  hal_start(h3, 3u, offs - 1u);
  const Halton h2_start = h2, h3_start = h3;  // the MIS half restarts at the same index
  for (int i = 0; i < n; ++i) {
    const float s1 = hal_next(h2), s2 = hal_next(h3);
    const long long slot = slot_of(B, c, k0 + i);
    v3 ldir;
    float ltmax, lpdf, cv = 1.f;
    bool lit;
    int tri;
    if (KIND == YK_LIGHT_AREA) lit = light_illum(L, sp.P, s1, s2, ldir, ltmax, lpdf);
    else if (KIND == YK_LIGHT_MESH) lit = mesh_illum(L, *ml, sp.P, s1, s2, ldir, ltmax, lpdf, tri);
    else if (KIND == YK_LIGHT_SPOT) lit = spot_illum(L, sp.P, s1, s2, ldir, ltmax, lpdf, cv);
    else if (KIND == YK_LIGHT_SUN) lit = sun_illum(L, s1, s2, ldir, ltmax, lpdf);
    else if (KIND == YK_LIGHT_BACKGROUND) {
      float u, v;
      lit = bg_illum(L, *ml, s1, s2, ldir, ltmax, lpdf, lcol, u, v);
    }
    else lit = sphere_illum(L, sp.P, s1, s2, ldir, ltmax, lpdf);
    if (!lit) {
      put_slot(B, slot, 0, black);
      continue;
    }
    nr += emit_shadow<false>(B, slot, sp.P, ldir, ltmax, k0 + i, traced);
    if (!(lpdf > 1e-6f)) {
      put_slot(B, slot, SL_TRACED, black);
      continue;
    }
    const c3 surf = mat_eval<!DIFF, GL>(M, sp, wo, ldir);
    const float mPdf = CAN_INTERSECT ? mat_pdf<GL>(M, sp, wo, ldir) : 0.f;
    // compiled form: ((surf*lcol) * (|N.l| * (1/pdf))) [* w]
    const float k = fabsf(vdot(sp.N, ldir)) * (1.0f / lpdf);
    float w = 1.f;
    if (mPdf > 1e-6f) {
      const float l2 = lpdf * lpdf, m2 = mPdf * mPdf;
      w = l2 / (l2 + m2);
    }
    if (B.ts) {  // ls.col *= scol first (mcintegrator.cc:130)
      put_slot(B, slot, SL_TRACED | SL_ADDS, surf);
      put_aux(B, slot, k, w, mPdf > 1e-6f ? 1.f : 0.f, KIND == YK_LIGHT_SPOT ? cv : 0.f);
      continue;
    }
    const c3 sl = cmul(surf, KIND == YK_LIGHT_SPOT ? cscale(cv, lcol) : lcol);
    c3 v;
    if (mPdf > 1e-6f) v = C3((sl.r * k) * w, (sl.g * k) * w, (sl.b * k) * w);
    else v = C3(sl.r * k, sl.g * k, sl.b * k);
    put_slot(B, slot, SL_TRACED | SL_ADDS, v);
  }
  if (!CAN_INTERSECT) return nr;
  h2 = h2_start;
  h3 = h3_start;
  for (int i = 0; i < n; ++i) {
    const float s1 = hal_next(h2), s2 = hal_next(h3);
    const long long slot = slot_of(B, c, k0 + n + i);
    float W = 0.f, spdf = 0.f;
    bool ok;
    v3 bdir = V3(0.f, 0.f, 0.f);
    const c3 surf = mat_sample<DIFF, GL>(M, sp, wo, bdir, s1, s2,
                                     BSDF_GLOSSY | BSDF_DIFFUSE | BSDF_DISPERSIVE | BSDF_REFLECT | BSDF_TRANSMIT, spdf,
                                     W, ok);
    float bt, lightPdf, cv = 1.f;
    bool hit = false;
    if (spdf > 1e-6f) {
      int tri;
      if (KIND == YK_LIGHT_AREA) hit = light_hit(L, sp.P, bdir, bt, lightPdf);
      else if (KIND == YK_LIGHT_MESH) hit = mesh_hit(L, *ml, sp.P, bdir, bt, lightPdf, tri);
      else if (KIND == YK_LIGHT_SUN) hit = sun_hit(L, bdir, bt, lightPdf);
      else if (KIND == YK_LIGHT_BACKGROUND) {
        float u, v;
        bt = -1.f;  // the shadow ray's own tmax: intersect() leaves t alone
        hit = bg_hit(L, *ml, bdir, lightPdf, lcol, u, v);
      }
      else hit = spot_hit(L, sp.P, bdir, bt, lightPdf, cv);
    }
    if (!hit) {
      put_slot(B, slot, 0, black);
      continue;
    }
    if ((KIND == YK_LIGHT_SUN || KIND == YK_LIGHT_BACKGROUND) && B.split)
      bt = __uint_as_float(0x7f800000u);  // unbounded, as a MIS record holds it
    nr += emit_shadow<true>(B, slot, sp.P, bdir, bt, k0 + n + i, traced);  // area: bt > 1e-10; spot: bt >= 0; mesh: bt >= MIN_RAYDIST; sun, background: -1
    if (!(lightPdf > 1e-6f)) {
      put_slot(B, slot, SL_TRACED, black);
      continue;
    }
    const float lPdf = 1.f / lightPdf;
    const float l2 = lPdf * lPdf, m2 = spdf * spdf;
    const float w = m2 / (l2 + m2);
    if (B.ts) {  // lcol *= scol first (mcintegrator.cc:180)
      put_slot(B, slot, SL_TRACED | SL_ADDS, C3(surf.r * W, surf.g * W, surf.b * W));
      put_aux(B, slot, w, 0.f, 0.f, KIND == YK_LIGHT_SPOT ? cv : 0.f);
      continue;
    }
    // compiled form of "surfCol * lcol * w * W": R,G ((surf*W)*lcol)*w, B (surf*W)*(w*lcol)
    const c3 lc = KIND == YK_LIGHT_SPOT ? cscale(cv, lcol) : lcol;
    put_slot(B, slot, SL_TRACED | SL_ADDS,
             C3(((surf.r * W) * lc.r) * w, ((surf.g * W) * lc.g) * w, (surf.b * W) * (w * lc.b)));
  }
  return nr;
}

// Ambient occlusion of direct lighting (directlight.cc:142): the parameters
// of mcIntegrator_t::sampleAmbientOcclusion. The AO rays of a shading point
// own the n shadow slots k0 .. k0 + n - 1 after the lights' (k0 = the scene's
// light slots), in loop order.
struct AOConst {
  int n;         // aoSamples (rayDivision is 1 on this path); 0: off
  int k0;        // first AO slot
  float dist;    // aoDist: the rays' tmax
  float col[3];  // aoCol
};
constexpr unsigned kAOFlags = BSDF_GLOSSY | BSDF_DIFFUSE | BSDF_REFLECT;

// mcIntegrator_t::sampleAmbientOcclusion (mcintegrator.cc:629-683), split at
// its isShadowed call like gen_light: sample i's ray (tmin YAF_SHADOW_BIAS,
// tmax aoDist, the form of a light-sample ray) goes to slot k0 + i with
// "aoCol * surfCol * cos * W" in source order (the compiled order of this
// function is not pinned); under transparent shadows aoCol * scol comes first,
// so the slot keeps surfCol and the aux record {cos, W}. A sample() that
// returns early (no component matches, or their widths sum below 1e-5) leaves
// W = 0 and the previous direction: its term is +0 whatever the ray meets,
// and the slot traces nothing.
template <bool DIFF, int GL = kGLNone>
__device__ __forceinline__ int gen_ao(const Batch& B, long long c, const AOConst& A, const DMat& M, const SurfPt& sp,
                                      v3 wo, unsigned pixelSample, unsigned soffs, unsigned long long& traced) {
  const c3 black = C3(0.f, 0.f, 0.f);
  const int n = A.n;
  const unsigned offs = (unsigned)(n * (int)pixelSample) + soffs;
  Halton h2, h3;
  hal_start(h2, 2u, offs - 1u);
  hal_start(h3, 3u, offs - 1u);
  int nr = 0;
  for (int i = 0; i < n; ++i) {
    const float s1 = hal_next(h2), s2 = hal_next(h3);
    const long long slot = slot_of(B, c, A.k0 + i);
    float W = 0.f, pdf = 0.f;
    bool ok;
    v3 dir = V3(0.f, 0.f, 0.f);
    const c3 surf = mat_sample<DIFF, GL>(M, sp, wo, dir, s1, s2, kAOFlags, pdf, W, ok);
    if (!ok) {
      put_slot(B, slot, 0, black);
      continue;
    }
    nr += emit_shadow<false>(B, slot, sp.P, dir, A.dist, A.k0 + i, traced);
    const float cs = fabsf(vdot(sp.N, dir));
    if (B.ts) {
      put_slot(B, slot, SL_TRACED | SL_ADDS, surf);
      put_aux(B, slot, cs, W, 0.f, 0.f);
      continue;
    }
    put_slot(B, slot, SL_TRACED | SL_ADDS,
             C3(((A.col[0] * surf.r) * cs) * W, ((A.col[1] * surf.g) * cs) * W, ((A.col[2] * surf.b) * cs) * W));
  }
  return nr;
}

// Writes the traced slots [0,kend) of sample c to the shadow queue from
// `base`, in slot order (bit mask for the first 64 slots, flags beyond).
__device__ __forceinline__ void flush_shadow(const Batch& B, long long c, int kend, int nr, unsigned base,
                                             unsigned long long traced) {
  if (nr == 0) return;
  unsigned r = base;
  for (int k = 0; k < kend; ++k) {
    const long long slot = slot_of(B, c, k);
    const bool t = k < 64 ? ((traced >> k) & 1ull) != 0ull : (B.sl_flags[slot] & SL_TRACED) != 0;
    if (t) B.s_idx[r++] = B.split ? ((unsigned)k << B.kshift) | (unsigned)(B.slot_base + c) : (unsigned)slot;
  }
}

// First segment of sub-path isub from a diffuse camera-ray hit: sample the
// primary BSDF (pathtracer.cc:169-187). Returns the segment's ray.
template <bool DIFF = false, int GL = kGLNone>
__device__ __forceinline__ yk_ray path_first_segment(const Batch& B, const RenderConst& R, long long c,
                                                     const SurfPt& sp, const DMat& M, v3 dir, int isub) {
  const unsigned s = R.ps ? B.psample[c] : (unsigned)c % (unsigned)R.spp;
  const unsigned offs = (unsigned)(R.nsub * (int)s) + B.soffs[c] + (unsigned)isub;
  const float s1 = ri_vdc(offs, 0u);
  const float s2 = (float)scr_halton(2, offs);
  float pdf, W = B.wlast[c];
  bool ok;
  v3 pdir = V3(0.f, 0.f, 0.f);
  c3 scol = mat_sample<DIFF, GL>(M, sp, vneg(dir), pdir, s1, s2, BSDF_DIFFUSE | BSDF_REFLECT | BSDF_TRANSMIT, pdf, W, ok);
  B.wlast[c] = W;
  scol = cscale(W, scol);
  B.thr[3 * c] = scol.r;
  B.thr[3 * c + 1] = scol.g;
  B.thr[3 * c + 2] = scol.b;
  yk_ray r;
  put_ray(r, sp.P, pdir, YK_MIN_RAYDIST, -1.0f);
  return r;
}

// Camera-ray hit (pathtracer.cc:146-160, directlight.cc:124-135): emission
// and the estimateAllDirectLight shadow rays; for the path tracer also the
// first segment of sub-path 0 (appended to bounce queue 1).
// k_shade_primary runs at the compiler's register choice (101 VGPRs in the
// diffuse-only instantiation, 4 waves per SIMD): forced to 5 waves (96 VGPRs,
// 6 spills) it lost 3-4 % (round 5: C2 10649-10715 against 11072-11091,
// headline 3265-3274 against 3337-3344). k_shade_bounce / k_path_start are
// the ones forced to 5 waves (YK_BOUNCE_WAVES, 640-thread blocks): since the
// round-5 combined variant that is +1.5 % on the headline, the round-3 loss
// (spills of 124-200 B per lane) predates their register diet.
// AO: direct lighting with ambient occlusion (gen_ao) -- an instantiation of
// its own, so the others carry none of its code; A is read by it alone.
// GL: the scene holds a glossy material (mat_eval); DIFF is false then.
template <bool DIFF, int XL, bool AO, int GL = kGLNone>
__global__ void __launch_bounds__(YK_PRIMARY_BLOCK) k_shade_primary(DScene S, Batch B, RenderConst R, long long nc,
                                                       unsigned long long* __restrict__ qword, AOConst A) {
  // The material records in LDS: per-lane reads of constant memory (the
  // lanes' materials differ) go through the vector-memory path, which limits
  // the shading kernels (C2 PMC: TD busy 0.87-0.90 of the CU's cycles, waves
  // waiting 51-62 %); LDS reads do not. C2 +1.8 %. (The same copy in
  // k_shade_bounce, with this depth's two Faure permutations, cost it spills
  // and measured -0.7 %.)
  __shared__ DMat s_mats[kMaxMats];
  {
    const int nw = S.nmats * (int)(sizeof(DMat) / sizeof(int));
    for (int i = threadIdx.x; i < nw; i += YK_PRIMARY_BLOCK)
      reinterpret_cast<int*>(s_mats)[i] = reinterpret_cast<const int*>(c_mats)[i];
    __syncthreads();
  }
  const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = c < nc;
  int nr = 0, kend = 0;
  unsigned long long traced = 0;
  bool emit = false;
  yk_ray seg;
  if (valid) {
    const yk_hit h = B.p_hits[c];
    c3 col = C3(0.f, 0.f, 0.f), em = C3(0.f, 0.f, 0.f);
    float alpha = R.transp_bg ? 0.f : 1.f;
    int ph = 0;
    if (h.prim >= 0) {
      const yk_ray r = B.p_rays[c];
      const v3 from = V3(r.from[0], r.from[1], r.from[2]), dir = V3(r.dir[0], r.dir[1], r.dir[2]);
      const SurfPt sp = make_surface(S, from, dir, h);
      const DMat& M = s_mats[sp.mat];
      const v3 wo = vneg(dir);
      ph = PH_HIT;
      if (M.flags & BSDF_EMIT) {
        // spec mode: emission is added at the fold, where state.includeLights
        // of this recursion level is known (lightMat_t::emit depends on it)
        const c3 e = mat_emit(M, sp, wo, true);
        // photon mapping: includeLights is true at every recursion level
        // (recursiveRaytrace sets it, integrate() restores it), so its
        // emission needs no fold-time decision
        // emission, and only a lightMat_t's emit() reads includeLights: other
        // emitters add it here, before the direct light and the caustic
        // estimate, in integrate()'s order
        if (R.spec && R.integrator != YK_INTEGRATOR_PHOTON && M.type == YK_MAT_LIGHT) em = e;
        else col = cadd(col, e);
        // photonIntegrator_t::integrate adds emit() a second time after
        // includeLights = false (photonintegr.cc:812-831)
        if (R.integrator == YK_INTEGRATOR_PHOTON && !R.pm_showmap) col = cadd(col, mat_emit(M, sp, wo, false));
        if (M.type == YK_MAT_LIGHT) ph |= PH_LIGHT;
      }
      if (M.flags & BSDF_DIFFUSE) ph |= PH_DIFFUSE;
      if ((M.flags & BSDF_DIFFUSE) && !R.pm_showmap) {
        const unsigned s = R.ps ? B.psample[c] : (unsigned)c % (unsigned)R.spp;
        int k0 = 0;
        for (int l = 0; l < R.nlights; ++l) {
          nr += gen_light<DIFF, XL, GL>(B, c, k0, l, sp, wo, s, B.soffs[c], (unsigned)l, traced, s_mats, S.ml);
          k0 += c_lights[l].nslots;
        }
        kend = k0;
        if constexpr (AO) {
          nr += gen_ao<DIFF, GL>(B, c, A, M, sp, wo, s, B.soffs[c], traced);
          kend = A.k0 + A.n;
          if (M.flags & BSDF_EMIT) ph |= PH_AOEMIT;
        }
        if (nr) put_org(B, c, sp.P);
        if (R.integrator == YK_INTEGRATOR_PATH) {
          B.wlast[c] = 0.f;
          seg = path_first_segment<DIFF, GL>(B, R, c, sp, M, dir, 0);
          emit = true;
          if (R.spec) {  // state.includeLights = false before the first segment's intersect
            B.incl[c] = 0;
            B.caus[c] = 0;
          }
        }
      }
      alpha = 1.0f;
    } else if (R.has_bg) {  // nothing hit: col += (*background)(ray)
      const c3 bg = R.has_bg == kBgGradient ? bg_gradient(R.bg_grad, ld3(B.p_rays[c].dir)) : C3(R.bg[0], R.bg[1], R.bg[2]);
      col = cadd(col, bg);
    }
    B.prim_hit[c] = ph;
    B.col[3 * c] = col.r;
    B.col[3 * c + 1] = col.g;
    B.col[3 * c + 2] = col.b;
    B.alpha[c] = alpha;
    if (R.spec) {
      B.emit0[3 * c] = em.r;
      B.emit0[3 * c + 1] = em.g;
      B.emit0[3 * c + 2] = em.b;
    }
    if (!R.merged) {
      B.pathcol[3 * c] = 0.f;
      B.pathcol[3 * c + 1] = 0.f;
      B.pathcol[3 * c + 2] = 0.f;
    }
    if (!emit) B.wlast[c] = 0.f;
  }
  unsigned sbase, q;
  wave_append2<YK_PRIMARY_APPEND_WAVE>(qword, valid ? (unsigned)nr : 0u, emit ? 1u : 0u, sbase, q);
  if (valid) flush_shadow(B, c, kend, nr, sbase, traced);
  if (emit) {
    st_ray(&B.q_rays[1][q], seg);
    B.q_owner[1][q] = (int)c;
  }
}

// Sums light li's unoccluded slot contributions in reference order:
// (0 + invNS*ccol) + invNS*ccol2 (mcintegrator.cc:116-191); Dirac: 0 + v.
// Contribution of an unoccluded slot under transparent shadows: the light
// colour times the shadow ray's filter, then the reference's products.
__device__ __forceinline__ c3 slot_value_ts(const Batch& B, long long slot, int kind, c3 lcol, bool spot = false) {
  const c3 a = get_contrib(B, slot);
  const float4 x = *reinterpret_cast<const float4*>(B.sl_aux + 4 * slot);
  const c3 sc = C3(B.s_filt[3 * slot], B.s_filt[3 * slot + 1], B.s_filt[3 * slot + 2]);
  if (kind == 0) {  // Dirac: R,G (lcol*surf)*f, B surf*(lcol*f)
    const c3 lc = cmul(C3(x.y, x.z, x.w), sc);
    return C3((lc.r * a.r) * x.x, (lc.g * a.g) * x.x, a.b * (lc.b * x.x));
  }
  if (spot) lcol = cscale(x.w, lcol);  // a soft spot's ls.col / lcol: color * falloff (gen_sampled)
  const c3 lc = cmul(lcol, sc);
  if (kind == 1) {  // light sample: ((surf*lcol)*k) [*w]
    const c3 sl = cmul(a, lc);
    if (x.z != 0.f) return C3((sl.r * x.x) * x.y, (sl.g * x.x) * x.y, (sl.b * x.x) * x.y);
    return C3(sl.r * x.x, sl.g * x.x, sl.b * x.x);
  }
  // BSDF (MIS) sample, a = surf*W: R,G ((surf*W)*lcol)*w, B (surf*W)*(w*lcol)
  return C3((a.r * lc.r) * x.x, (a.g * lc.g) * x.x, a.b * (x.x * lc.b));
}

__device__ __forceinline__ c3 resolve_light(const Batch& B, long long c, int k0, int li) {
  if (!light_sampled(c_lights[li])) {
    const long long slot = slot_of(B, c, k0);
    c3 col = C3(0.f, 0.f, 0.f);
    if ((B.sl_flags[slot] & SL_ADDS) && !B.s_occl[slot])
      col = cadd(col, B.ts ? slot_value_ts(B, slot, 0, col)
                           : get_contrib(B, slot));
    return col;
  }
  // n light samples, then the BSDF (MIS) half of the lights that have one
  // (nslots = 2n: area, soft spot; a sphere light has nslots = n)
  const int n = c_lights[li].samples, nk = c_lights[li].nslots;
  const bool spot = c_lights[li].type == YK_LIGHT_SPOT;
  const float invNS = 1.f / (float)n;
  c3 ccol = C3(0.f, 0.f, 0.f), ccol2 = C3(0.f, 0.f, 0.f);
  for (int i = 0; i < nk; ++i) {
    const long long slot = slot_of(B, c, k0 + i);
    if ((B.sl_flags[slot] & SL_ADDS) && !B.s_occl[slot]) {
      const c3 v = B.ts ? slot_value_ts(B, slot, i < n ? 1 : 2, C3(c_lights[li].color[0], c_lights[li].color[1], c_lights[li].color[2]), spot)
                        : get_contrib(B, slot);
      if (i < n) ccol = cadd(ccol, v);
      else ccol2 = cadd(ccol2, v);
    }
  }
  c3 col = C3(0.f, 0.f, 0.f);
  col = cadd(col, cscale(invNS, ccol));
  if (nk > n) col = cadd(col, cscale(invNS, ccol2));  // "if(canIntersect)", mcintegrator.cc:156-192
  return col;
}

// col += estimateAllDirectLight (sum over lights, starting from 0)
__global__ void __launch_bounds__(256) k_resolve_primary(Batch B, RenderConst R, long long nc) {
  const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc || !(B.prim_hit[c] & PH_DIFFUSE) || R.pm_showmap) return;
  c3 dl = C3(0.f, 0.f, 0.f);
  int k0 = 0;
  for (int l = 0; l < R.nlights; ++l) {
    dl = cadd(dl, resolve_light(B, c, k0, l));
    k0 += c_lights[l].nslots;
  }
  B.col[3 * c] = B.col[3 * c] + dl.r;
  B.col[3 * c + 1] = B.col[3 * c + 1] + dl.g;
  B.col[3 * c + 2] = B.col[3 * c + 2] + dl.b;
}

// col += sampleAmbientOcclusion (directlight.cc:142), after the direct light
// and the caustic estimate: the unoccluded AO slots' terms in loop order from
// 0, then col / (float)n. An emitting material also adds emit * s.pdf per
// sample ahead of that sample's term (mcintegrator.cc:666-669); its entries
// (PH_AOEMIT) sample the material again for s.pdf rather than every slot
// keeping a value that almost no scene reads.
__global__ void __launch_bounds__(256) k_resolve_ao(DScene S, Batch B, RenderConst R, AOConst A, long long nc) {
  const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const int ph = B.prim_hit[c];
  if (!(ph & PH_DIFFUSE)) return;
  c3 col = C3(0.f, 0.f, 0.f);
  const c3 aoc = C3(A.col[0], A.col[1], A.col[2]);
  const bool emits = (ph & PH_AOEMIT) != 0;
  SurfPt sp{};
  v3 wo = V3(0.f, 0.f, 0.f);
  c3 em = C3(0.f, 0.f, 0.f);
  Halton h2{}, h3{};
  if (emits) {
    const yk_ray r = B.p_rays[c];
    const v3 from = V3(r.from[0], r.from[1], r.from[2]), dir = V3(r.dir[0], r.dir[1], r.dir[2]);
    sp = make_surface(S, from, dir, B.p_hits[c]);
    wo = vneg(dir);
    em = mat_emit(c_mats[sp.mat], sp, wo, true);
    const unsigned s = R.ps ? B.psample[c] : (unsigned)c % (unsigned)R.spp;
    const unsigned offs = (unsigned)(A.n * (int)s) + B.soffs[c];
    hal_start(h2, 2u, offs - 1u);
    hal_start(h3, 3u, offs - 1u);
  }
  for (int i = 0; i < A.n; ++i) {
    if (emits) {  // col += material->emit(state, sp, wo) * s.pdf
      const float s1 = hal_next(h2), s2 = hal_next(h3);
      float W = 0.f, pdf = 0.f;
      bool ok;
      v3 wi = V3(0.f, 0.f, 0.f);
      (void)mat_sample<false>(c_mats[sp.mat], sp, wo, wi, s1, s2, kAOFlags, pdf, W, ok);
      col = cadd(col, cscale(pdf, em));
    }
    const long long slot = slot_of(B, c, A.k0 + i);
    if (!(B.sl_flags[slot] & SL_ADDS) || B.s_occl[slot]) continue;
    c3 v = get_contrib(B, slot);
    if (B.ts) {  // aoCol * scol * surfCol * cos * W
      const float4 x = *reinterpret_cast<const float4*>(B.sl_aux + 4 * slot);
      const c3 as = cmul(aoc, C3(B.s_filt[3 * slot], B.s_filt[3 * slot + 1], B.s_filt[3 * slot + 2]));
      v = C3(((as.r * v.r) * x.x) * x.y, ((as.g * v.g) * x.x) * x.y, ((as.b * v.b) * x.x) * x.y);
    }
    col = cadd(col, v);
  }
  const float fn = (float)A.n;
  B.col[3 * c] = B.col[3 * c] + col.r / fn;
  B.col[3 * c + 1] = B.col[3 * c + 1] + col.g / fn;
  B.col[3 * c + 2] = B.col[3 * c + 2] + col.b / fn;
}

// First segment of sub-paths isub >= 1 (sub-path 0 is fused into
// k_shade_primary).
template <bool DIFF, int GL = kGLNone>
__global__ void __launch_bounds__(YK_BOUNCE_BLOCK) k_path_start(DScene S, Batch B, RenderConst R, long long nc, int isub,
                                                    unsigned long long* __restrict__ qword) {
  const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = c < nc;
  bool emit = false;
  yk_ray r;
  if (valid && (B.prim_hit[c] & PH_DIFFUSE)) {
    const yk_hit h = B.p_hits[c];
    const yk_ray pr = B.p_rays[c];
    const v3 from = V3(pr.from[0], pr.from[1], pr.from[2]), dir = V3(pr.dir[0], pr.dir[1], pr.dir[2]);
    const SurfPt sp = make_surface(S, from, dir, h);
    r = path_first_segment<DIFF, GL>(B, R, c, sp, c_mats[sp.mat], dir, isub);
    emit = true;
    if (R.spec) {
      B.incl[c] = 0;
      B.caus[c] = 0;
    }
  }
  unsigned sbase, q;
  wave_append2<YK_BOUNCE_APPEND_WAVE>(qword, 0u, emit ? 1u : 0u, sbase, q);
  if (emit) {
    st_ray(&B.q_rays[1][q], r);
    B.q_owner[1][q] = (int)c;
  }
}

// Hit at bounce `depth` (1-based) of the current sub-path
// (pathtracer.cc:189-298): estimateOneDirectLight shadow rays, emission,
// and the BSDF sample of the next segment. One thread per live path (entry
// qi of the input bounce queue, owned by camera sample c).
template <bool DIFF, int XL, int GL = kGLNone>
__global__ void __launch_bounds__(bounce_block(DIFF))
__attribute__((amdgpu_waves_per_eu(DIFF ? YK_BOUNCE_WAVES_D : YK_BOUNCE_WAVES))) k_shade_bounce(DScene S, Batch B, RenderConst R,
                                                      const unsigned long long* __restrict__ qin_word, int depth,
                                                      int isub, int qin, unsigned long long* __restrict__ qword) {
  const long long nq = (long long)(*qin_word >> 32);  // live paths (device-side count)
  const long long qb = (long long)blockIdx.x * blockDim.x;
  if (qb >= nq) return;  // whole block past the queue
  unsigned qpre = 0;  // merged shadow queue: after the earlier regions' entries
  if (B.mq_words)
    for (int r = 0; r < B.mq_region; ++r) qpre += (unsigned)B.mq_words[r];
  long long qi = qb + threadIdx.x;
  bool valid = qi < nq;
  // Escaped paths (most first-bounce rays of an open scene) finish here; the
  // block's hits are then packed onto its first threads, so the shading below
  // runs on full waves instead of waves whose lanes mostly sit out.
  {
    const int prim = valid ? B.q_hits[qin][qi].prim : 0;
    if (valid && prim < 0) {
      const long long c = B.q_owner[qin][qi];
      // background: "continue" at depth 1, "break" later; a caustic segment
      // adds the background first (pathtracer.cc:279-286)
      // (a scene of diffuse-only materials has no specular recursion and no caustic segment:
      // its instantiation, the headline's, carries none of this)
      if (!DIFF && R.spec && depth >= 2 && B.caus[c] && R.has_bg) {
        const c3 bg = R.has_bg == kBgGradient ? bg_gradient(R.bg_grad, ld3(B.q_rays[qin][qi].dir)) : C3(R.bg[0], R.bg[1], R.bg[2]);
        B.pathcol[3 * c] = B.pathcol[3 * c] + B.thr[3 * c] * bg.r;
        B.pathcol[3 * c + 1] = B.pathcol[3 * c + 1] + B.thr[3 * c + 1] * bg.g;
        B.pathcol[3 * c + 2] = B.pathcol[3 * c + 2] + B.thr[3 * c + 2] * bg.b;
      }
      B.pstate[c] = 0;
    }
    int src;
    valid = pack_block<bounce_block(DIFF)>(valid && prim >= 0, src);
    qi = qb + src;
  }
  const long long c = valid ? B.q_owner[qin][qi] : 0;
  int nr = 0, kend = 0;
  unsigned long long traced = 0;
  bool emit_next = false;
  yk_ray nxt;
  if (valid) {
    const yk_hit h = B.q_hits[qin][qi];
    {
      const yk_ray pr = B.q_rays[qin][qi];
      const v3 from = V3(pr.from[0], pr.from[1], pr.from[2]), dir = V3(pr.dir[0], pr.dir[1], pr.dir[2]);
      const SurfPt sp = make_surface(S, from, dir, h);
      const DMat& M = c_mats[sp.mat];
      const v3 pwo = vneg(dir);
      const unsigned s = R.ps ? B.psample[c] : (unsigned)c % (unsigned)R.spp;
      const unsigned offs = (unsigned)(R.nsub * (int)s) + B.soffs[c] + (unsigned)isub;
      int ps = PS_RESOLVE;
      // estimateOneDirectLight(state, hit, pwo, offs): always at the first
      // bounce, for diffuse materials afterwards (mcintegrator.cc:198-215)
      if ((depth == 1 || (M.flags & BSDF_DIFFUSE)) && R.nlights > 0) {
        Halton h2;
        hal_start(h2, 2u, (unsigned)((int)offs - 1));
        int lnum = (int)(hal_next(h2) * (float)R.nlights);
        if (lnum > R.nlights - 1) lnum = R.nlights - 1;
        // one light (C2, the headline): a literal light index, so the
        // compiler reads its record with scalar loads instead of per-lane
        // vector loads (which go through the texture path that limits this
        // kernel, PMC TD busy 0.9)
        if (R.nlights == 1) nr = gen_light<DIFF, XL, GL>(B, c, 0, 0, sp, pwo, s, B.soffs[c], 0u, traced, c_mats, S.ml);
        else nr = gen_light<DIFF, XL, GL>(B, c, 0, lnum, sp, pwo, s, B.soffs[c], (unsigned)lnum, traced, c_mats, S.ml);
        kend = c_lights[lnum].nslots;
        if (nr) put_org(B, c, sp.P);
        if (R.nlights > 1) B.lsel[c] = lnum;  // one light: the resolve knows it is light 0
        ps |= PS_EST;
      }
      // emission, stored only where the resolve adds it (a zero emission is
      // not stored: adding +0 to the resolve's non-negative light sum is exact)
      c3 em = C3(0.f, 0.f, 0.f);
      bool emits = false;
      if (depth == 1 && (M.flags & BSDF_EMIT)) {
        em = mat_emit(M, sp, pwo, false);
        emits = true;
      }
      // "matBSDFs & (BSDF_EMIT && caustic)" is matBSDFs & BSDF_SPECULAR when
      // the segment was caustic (pathtracer.cc:295); includeLights = caustic
      if (R.spec && depth >= 2 && B.caus[c] && (M.flags & BSDF_SPECULAR)) {
        em = mat_emit(M, sp, pwo, true);
        emits = true;
      }
      if (emits) {
        B.emit_b[3 * c] = em.r;
        B.emit_b[3 * c + 1] = em.g;
        B.emit_b[3 * c + 2] = em.b;
        ps |= PS_EMIT;
      }
      if (depth < R.bounces) {
        const float s1 = (float)scr_halton(4 * depth + 3, offs);
        const float s2 = (float)scr_halton(4 * depth + 4, offs);
        float pdf, W = B.wlast[c];
        bool ok;
        v3 ndir = dir;  // pRay.dir keeps the previous direction if sample() returns early
        unsigned sfl;
        c3 sc = mat_sample<DIFF, GL>(M, sp, pwo, ndir, s1, s2, BSDF_ALL, pdf, W, ok, sfl);
        B.wlast[c] = W;
        sc = cscale(W, sc);
        if (!cblack(sc)) {
          if (R.spec) {  // caustic = traceCaustics && sampledFlags & (SPECULAR|GLOSSY|FILTER)
            const uint8_t caustic =
                (R.trace_caustics && (sfl & (BSDF_SPECULAR | BSDF_GLOSSY | BSDF_FILTER))) ? 1 : 0;
            B.caus[c] = caustic;
            B.incl[c] = caustic;
          }
          put_ray(nxt, sp.P, ndir, YK_MIN_RAYDIST, -1.0f);
          emit_next = true;
          B.scol_next[3 * c] = sc.r;
          B.scol_next[3 * c + 1] = sc.g;
          B.scol_next[3 * c + 2] = sc.b;
          ps |= PS_CONT;
        }
      }
      B.pstate[c] = ps;
    }
  }
  unsigned sbase, qn;
  wave_append2<YK_BOUNCE_APPEND_WAVE>(qword, valid ? (unsigned)nr : 0u, emit_next ? 1u : 0u, sbase, qn);
  if (valid) flush_shadow(B, c, kend, nr, sbase + qpre, traced);
  if (emit_next) {
    st_ray(&B.q_rays[qin ^ 1][qn], nxt);
    B.q_owner[qin ^ 1][qn] = (int)c;
  }
}

// pathCol += lcol*throughput; throughput *= scol of the next segment. One
// thread per entry of the bounce queue k_shade_bounce consumed.
__global__ void __launch_bounds__(256) k_resolve_bounce(Batch B, RenderConst R,
                                                        const unsigned long long* __restrict__ qin_word, int depth,
                                                        int qin) {
  const long long nq = (long long)(*qin_word >> 32);
  const long long qi = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (qi >= nq) return;
  const long long c = B.q_owner[qin][qi];
  const int ps = B.pstate[c];
  if (!(ps & PS_RESOLVE)) return;
  c3 lcol = C3(0.f, 0.f, 0.f);
  if (ps & PS_EST) {
    const int lnum = R.nlights > 1 ? B.lsel[c] : 0;
    lcol = cscale((float)R.nlights, resolve_light(B, c, 0, lnum));
  }
  if ((depth == 1 || R.spec) && (ps & PS_EMIT))
    lcol = cadd(lcol, C3(B.emit_b[3 * c], B.emit_b[3 * c + 1], B.emit_b[3 * c + 2]));
  const c3 thr = C3(B.thr[3 * c], B.thr[3 * c + 1], B.thr[3 * c + 2]);
  B.pathcol[3 * c] = B.pathcol[3 * c] + lcol.r * thr.r;
  B.pathcol[3 * c + 1] = B.pathcol[3 * c + 1] + lcol.g * thr.g;
  B.pathcol[3 * c + 2] = B.pathcol[3 * c + 2] + lcol.b * thr.b;
  if (ps & PS_CONT) {
    B.thr[3 * c] = thr.r * B.scol_next[3 * c];
    B.thr[3 * c + 1] = thr.g * B.scol_next[3 * c + 1];
    B.thr[3 * c + 2] = thr.b * B.scol_next[3 * c + 2];
    B.pstate[c] = PS_ALIVE;
  } else {
    B.pstate[c] = 0;
  }
}

// ---- merged shadow launch (path tracing without specular recursion,
// photon maps or transparent shadows, one sub-path): the camera hits' shadow
// rays and every bounce's go to one any-hit launch per batch instead of one
// per bounce. Each trace launch carries a fixed cost -- its start and the
// drain of its last rays, about 0.25-0.3 ms on the headline scene whatever
// its size (tools/trav_bench.py --sizes) -- so four launches per batch paid
// it four times. The bounces' shadow rays do not feed the next bounce (its
// closest rays come from the BSDF sample alone), only the resolve, which then
// runs once per batch over all bounces in the reference's order: every bounce
// writes its own slot region (slot_base) and path state (pstate, lsel,
// emit_b, scol_next at (depth-1)*cap), and appends its slot indices to the
// one queue after those of the regions before it (mq_words).

// Batch view of bounce `depth`'s slot region and path state (host and device)
__host__ __device__ inline Batch merged_region(Batch B, int depth) {
  B.slot_base = (long long)depth * B.cap;
  B.mq_region = depth;
  if (depth >= 1) {
    const long long o = (long long)(depth - 1) * B.cap;
    B.pstate += o;
    B.lsel += o;
    B.emit_b += 3 * o;
    B.scol_next += 3 * o;
  }
  return B;
}

// k_resolve_primary, then k_resolve_bounce for depth 1..bounces, per camera
// sample in that order: the same float operations on the same values as the
// per-bounce resolves. A sample's path entered depth 1 iff its camera hit was
// diffuse (k_shade_primary's first segment), and depth d+1 iff depth d set
// PS_CONT, so no stale region state is read.
// k_finish is folded in: the final sample col + pathCol / nSamples (path
// tracing, diffuse camera hit) with its alpha, the same operations.
__global__ void __launch_bounds__(256) k_resolve_merged(Batch B, RenderConst R, long long nc, int bounces) {
  const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  c3 col = C3(B.col[3 * c], B.col[3 * c + 1], B.col[3 * c + 2]);
  if (!(B.prim_hit[c] & PH_DIFFUSE)) {
    B.samples[c] = make_float4(col.r, col.g, col.b, B.alpha[c]);
    return;
  }
  {
    c3 dl = C3(0.f, 0.f, 0.f);
    int k0 = 0;
    for (int l = 0; l < R.nlights; ++l) {
      dl = cadd(dl, resolve_light(B, c, k0, l));
      k0 += c_lights[l].nslots;
    }
    col = C3(col.r + dl.r, col.g + dl.g, col.b + dl.b);
  }
  c3 thr = C3(B.thr[3 * c], B.thr[3 * c + 1], B.thr[3 * c + 2]);
  c3 pc = C3(0.f, 0.f, 0.f);  // pathCol = 0 (k_shade_primary leaves it unstored for merged batches)
  for (int depth = 1; depth <= bounces; ++depth) {
    const Batch Bd = merged_region(B, depth);
    const int ps = Bd.pstate[c];
    if (!(ps & PS_RESOLVE)) break;
    c3 lcol = C3(0.f, 0.f, 0.f);
    if (ps & PS_EST) {
      const int lnum = R.nlights > 1 ? Bd.lsel[c] : 0;
      lcol = cscale((float)R.nlights, resolve_light(Bd, c, 0, lnum));
    }
    if (depth == 1 && (ps & PS_EMIT))
      lcol = cadd(lcol, C3(Bd.emit_b[3 * c], Bd.emit_b[3 * c + 1], Bd.emit_b[3 * c + 2]));
    pc = C3(pc.r + lcol.r * thr.r, pc.g + lcol.g * thr.g, pc.b + lcol.b * thr.b);
    if (!(ps & PS_CONT)) break;
    thr = C3(thr.r * Bd.scol_next[3 * c], thr.g * Bd.scol_next[3 * c + 1], thr.b * Bd.scol_next[3 * c + 2]);
  }
  const float ns = (float)R.nsub;  // k_finish
  col = cadd(col, C3(pc.r / ns, pc.g / ns, pc.b / ns));
  B.samples[c] = make_float4(col.r, col.g, col.b, B.alpha[c]);
}

// col += pathCol / nSamples (pathtracer.cc:300-302); final sample (wt = 1)
__global__ void __launch_bounds__(256) k_finish(Batch B, RenderConst R, long long nc) {
  const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  c3 col = C3(B.col[3 * c], B.col[3 * c + 1], B.col[3 * c + 2]);
  if (R.integrator == YK_INTEGRATOR_PATH && (B.prim_hit[c] & PH_DIFFUSE)) {
    const float ns = (float)R.nsub;
    col = cadd(col, C3(B.pathcol[3 * c] / ns, B.pathcol[3 * c + 1] / ns, B.pathcol[3 * c + 2] / ns));
  }
  B.samples[c] = make_float4(col.r, col.g, col.b, B.alpha[c]);
}

#include "yk_spec.inc"  // specular recursion: the node store, k_finish_spec, k_spawn, k_fold
#include "yk_film.inc"  // FilmConst, k_pixel_extent, the gathers, the depth channel, the resolves

#include "yk_photon.inc"

}  // namespace yk

// ============================================================ host side

using namespace yk;

#include "yk_pipe_host.inc"    // HIPCHK, DBuf, launch, Pipe, pipes_env, plan_batches
#include "yk_device_host.inc"  // kTrace, kShade, struct yk_device, bind_constants, YK_GUARD_*
#include "yk_trace_host.inc"   // tree_depth, trace_variant, enqueue_trace*, launch_trace, yk_trace_*
#include "yk_upload_host.inc"  // make_*, upload_qmc, install_traversal, yk_device_open / close, yk_device_upload
#include "yk_film_host.inc"    // the film filter tables, make_film, yk_film_filter_from_table
#include "yk_photon_host.inc"
#include "yk_kdtree_gpu.inc"
#include "yk_render_host.inc"

#include "yk_test_hooks.inc"
