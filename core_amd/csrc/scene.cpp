// Host scene assembly, kd-tree build trigger and the procedural probe scenes.
#include "scene.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>

namespace yk {

// ---- reference constructor arithmetic --------------------------------------
namespace {
struct hv3 {
  float x, y, z;
};
hv3 H(const float* p) { return {p[0], p[1], p[2]}; }
hv3 hsub(hv3 a, hv3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
hv3 hadd(hv3 a, hv3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
hv3 hmul(float f, hv3 b) { return {f * b.x, f * b.y, f * b.z}; }
hv3 hcross(hv3 a, hv3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
hv3 hnorm(hv3 a) {  // vector3d_t::normalize, vector3d.h:249-260
  float len = a.x * a.x + a.y * a.y + a.z * a.z;
  if (len != 0.f) {
    len = 1.0f / std::sqrt(len);
    a.x *= len;
    a.y *= len;
    a.z *= len;
  }
  return a;
}
void put(float* d, hv3 v) {
  d[0] = v.x;
  d[1] = v.y;
  d[2] = v.z;
}
constexpr unsigned kSpecular = 0x1u, kGlossy = 0x2u, kDiffuse = 0x4u, kReflect = 0x10u, kTransmit = 0x20u, kFilter = 0x40u,
                   kEmit = 0x80u;  // material.h:49-66
}  // namespace

yk_material_state material_state(const yk_material& m) {
  yk_material_state o{};
  o.type = m.type;
  if (m.type == YK_MAT_LIGHT) {  // lightMat_t(color * power, double_sided), simple.cc:80-90
    o.bsdf_flags = kEmit;
    for (int k = 0; k < 3; ++k) o.color[k] = m.color[k] * m.power;
    o.double_sided = m.double_sided;
  } else if (m.type == YK_MAT_COATED_GLOSSY) {  // coatedGlossyMat_t ctor + factory, coatedglossy.cc:80-102,420-463
    for (int k = 0; k < 3; ++k) {
      o.gloss_color[k] = m.color[k];
      o.diff_color[k] = m.diffuse_color[k];
      o.mirror_color[k] = m.mirror_color[k];
    }
    double ior = m.ior;
    if (ior == 1.f) ior = 1.0000001f;  // coatedglossy.cc:441, as written
    o.ior = (float)ior;                // PFLOAT IOR
    o.exponent = m.exponent;
    o.reflectivity = m.glossy_reflect;
    o.m_diffuse = m.diffuse_reflect;
    o.as_diffuse = m.as_diffuse ? 1 : 0;
    o.comp_flags[0] = kSpecular | kReflect;
    o.comp_flags[1] = o.as_diffuse ? (kDiffuse | kReflect) : (kGlossy | kReflect);
    if (m.diffuse_reflect > 0.f) {
      o.comp_flags[2] = kDiffuse | kReflect;
      o.with_diffuse = 1;
      o.ncomp = 3;
    } else {
      o.comp_flags[2] = 0u;  // BSDF_NONE
      o.ncomp = 2;
    }
    o.bsdf_flags = o.comp_flags[0] | o.comp_flags[1] | o.comp_flags[2];
    o.anisotropic = m.anisotropic ? 1 : 0;
    o.exp_u = m.exp_u;
    o.exp_v = m.exp_v;
    if (m.diffuse_brdf == YK_BRDF_OREN_NAYAR) {  // coatedGlossyMat_t::initOrenNayar(sigma), coatedglossy.cc:119-125
      const double sigma2 = m.sigma * m.sigma;
      o.oren_nayar = 1;
      o.oren_nayar_a = (float)(1.0 - 0.5 * (sigma2 / (sigma2 + 0.33)));
      o.oren_nayar_b = (float)(0.45 * sigma2 / (sigma2 + 0.09));
    }
  } else if (m.type == YK_MAT_GLOSSY) {  // glossyMat_t ctor + factory, glossy.cc:65-80,353-389 (no shader nodes)
    for (int k = 0; k < 3; ++k) {
      o.gloss_color[k] = m.color[k];
      o.diff_color[k] = m.diffuse_color[k];
    }
    o.exponent = m.exponent;
    o.reflectivity = m.glossy_reflect;
    o.m_diffuse = m.diffuse_reflect;
    o.as_diffuse = m.as_diffuse ? 1 : 0;
    if (m.diffuse_reflect > 0.f) {
      o.bsdf_flags = kDiffuse | kReflect;
      o.with_diffuse = 1;
    }
    o.bsdf_flags |= o.as_diffuse ? (kDiffuse | kReflect) : (kGlossy | kReflect);
    o.anisotropic = m.anisotropic ? 1 : 0;
    o.exp_u = m.exp_u;
    o.exp_v = m.exp_v;
    if (m.diffuse_brdf == YK_BRDF_OREN_NAYAR) {  // glossyMat_t::initOrenNayar(sigma), glossy.cc:97-103
      const double sigma2 = m.sigma * m.sigma;
      o.oren_nayar = 1;
      o.oren_nayar_a = (float)(1.0 - 0.5 * (sigma2 / (sigma2 + 0.33)));
      o.oren_nayar_b = (float)(0.45 * sigma2 / (sigma2 + 0.09));
    }
  } else {  // shinyDiffuseMat_t ctor + factory + config(), shinydiffuse.cc:9-80,474-562
    if (m.emit > 0.f) o.bsdf_flags |= kEmit;
    for (int k = 0; k < 3; ++k) {
      o.color[k] = m.color[k];
      o.emit_color[k] = m.emit * m.color[k];
      o.mirror_color[k] = m.mirror_color[k];
    }
    o.diffuse_strength = m.diffuse_reflect;
    o.transmit_filter = m.transmit_filter;
    if (m.fresnel_effect) {
      o.has_fresnel = 1;
      o.ior_squared = (float)(m.ior * m.ior);
    }
    float acc = 1.f;
    int n = 0;
    auto add = [&](unsigned flags, int index, float strength) {
      o.bsdf_flags |= flags;
      o.comp_flags[n] = flags;
      o.comp_index[n] = index;
      o.component[index] = strength;
      ++n;
    };
    if (m.specular_reflect > 0.00001f) {
      if (!o.has_fresnel) acc = 1.f - m.specular_reflect;
      add(kSpecular | kReflect, 0, m.specular_reflect);
    }
    if (m.transparency * acc > 0.00001f) {
      acc *= 1.f - m.transparency;
      add(kTransmit | kFilter, 1, m.transparency);
    }
    if (m.translucency * acc > 0.00001f) {
      acc *= 1.f - m.transparency;  // sic, shinydiffuse.cc:59
      add(kDiffuse | kTransmit, 2, m.translucency);
    }
    if (m.diffuse_reflect * acc > 0.00001f) add(kDiffuse | kReflect, 3, m.diffuse_reflect);
    o.ncomp = n;
    if (m.diffuse_brdf == YK_BRDF_OREN_NAYAR) {  // factory -> initOrenNayar(sigma), shinydiffuse.cc:170-176,505-514
      const double s2 = m.sigma * m.sigma;
      o.oren_nayar = 1;
      o.oren_nayar_a = (float)(1.0 - 0.5 * (s2 / (s2 + 0.33)));
      o.oren_nayar_b = (float)(0.45 * s2 / (s2 + 0.09));
    }
  }
  return o;
}

// glassMat_t::factory + ctor, glass.cc:55-69, 262-274 (no shader nodes, no dispersion, no absorption).
// filt is the factory's double: filt*filtCol goes through color_t's operator*(CFLOAT, color_t), which
// takes filt as a float, and color_t(1.f-filt) rounds the double difference to a float (color.h:41,64).
yk_material_state glass_material_state(const yk_material& m, const yk_glass_params& g, yk_glass_state& gs) {
  yk_material_state o{};
  o.type = YK_MAT_GLASS;
  const double filt = m.transmit_filter;
  const float ff = (float)filt, rest = (float)(1.f - filt);
  for (int k = 0; k < 3; ++k) {
    gs.filter_col[k] = ff * g.filter_color[k] + rest;
    o.mirror_color[k] = m.mirror_color[k];  // specRefCol
  }
  gs.fake_shadow = g.fake_shadows ? 1 : 0;
  o.ior = (float)m.ior;  // glassMat_t(float IOR, ...)
  o.bsdf_flags = kSpecular | kReflect | kTransmit;  // BSDF_ALL_SPECULAR
  if (gs.fake_shadow) o.bsdf_flags |= kFilter;
  return o;
}

yk_area_light_state light_state(const yk_light& l) {  // areaLight_t::factory + ctor, arealight.cc:30-49,171-192
  yk_area_light_state o{};
  const hv3 c = H(l.corner);
  put(o.corner, c);
  put(o.to_x, hsub(H(l.point1), c));
  put(o.to_y, hsub(H(l.point2), c));
  const float pi = (float)3.14159265358979323846;
  for (int k = 0; k < 3; ++k) o.color[k] = pi * (l.color[k] * l.power);
  o.samples = l.samples;
  return o;
}

// pointLight_t::pointLight_t (pointlight.cc:53-58) / directionalLight_t::
// directionalLight_t (directional.cc:50-58): color*power, direction.normalize()
yk_dirac_light_state dirac_state(const yk_light& l) {
  yk_dirac_light_state o{};
  o.type = l.type;
  for (int k = 0; k < 3; ++k) {
    o.position[k] = l.from[k];
    o.color[k] = l.color[k] * l.power;
  }
  if (l.type == YK_LIGHT_DIRECTIONAL) {
    float d[3] = {l.direction[0], l.direction[1], l.direction[2]};
    const float len = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    if (len != 0.f) {
      const float inv = 1.0f / std::sqrt(len);
      for (float& x : d) x *= inv;
    }
    for (int k = 0; k < 3; ++k) o.direction[k] = d[k];
    o.radius = l.radius;
    o.infinite = l.infinite;
  }
  return o;
}

// createCS (vector3d.h:316-334): d = 1.0 / fSqrt(..) is a double division of
// float values rounded to float, which equals the float division
static void create_cs(const float* N, float* u, float* v) {
  if (N[0] == 0.f && N[1] == 0.f) {
    u[0] = N[2] < 0.f ? -1.f : 1.f;
    u[1] = 0.f;
    u[2] = 0.f;
    v[0] = 0.f;
    v[1] = 1.f;
    v[2] = 0.f;
    return;
  }
  const float d = (float)(1.0 / (double)std::sqrt(N[1] * N[1] + N[0] * N[0]));
  u[0] = N[1] * d;
  u[1] = -N[0] * d;
  u[2] = 0.f;
  v[0] = N[1] * u[2] - N[2] * u[1];
  v[1] = N[2] * u[0] - N[0] * u[2];
  v[2] = N[0] * u[1] - N[1] * u[0];
}

// spotLight_t::spotLight_t, spotlight.cc:63-75: ndir = (from - to).normalize(),
// the angles in double (degToRad), fCos on their float values, icosDiff in double
yk_spot_light_state spot_state(const yk_light& l) {
  yk_spot_light_state o{};
  float nd[3] = {l.from[0] - l.to[0], l.from[1] - l.to[1], l.from[2] - l.to[2]};
  float len = nd[0] * nd[0] + nd[1] * nd[1] + nd[2] * nd[2];  // vector3d_t::normalize, vector3d.h:249-260
  if (len != 0.f) {
    len = 1.0f / std::sqrt(len);
    for (float& x : nd) x *= len;
  }
  for (int k = 0; k < 3; ++k) {
    o.position[k] = l.from[k];
    o.ndir[k] = nd[k];
    o.dir[k] = -nd[k];
    o.color[k] = l.color[k] * l.power;
  }
  create_cs(o.dir, o.du, o.dv);
  const double rad_angle = (double)l.cone_angle * 0.01745329251994329576922;  // degToRad
  const double rad_inner_angle = rad_angle * (double)(1.f - l.blend);
  o.cos_start = host_fcos((float)rad_inner_angle);
  o.cos_end = host_fcos((float)rad_angle);
  o.icos_diff = (float)(1.0 / (double)(o.cos_start - o.cos_end));
  o.soft_shadows = l.soft_shadows ? 1 : 0;
  o.shadow_fuzzyness = l.shadow_fuzzyness;
  o.samples = l.samples;
  o.photon_only = l.photon_only ? 1 : 0;
  return o;
}

// sphereLight_t::sphereLight_t, spherelight.cc:64-72
yk_sphere_light_state sphere_state(const yk_light& l) {
  yk_sphere_light_state o{};
  for (int k = 0; k < 3; ++k) {
    o.center[k] = l.from[k];
    o.color[k] = l.color[k] * l.power;
  }
  o.radius = l.radius;
  o.square_radius = l.radius * l.radius;
  o.square_radius_epsilon = (float)((double)o.square_radius * 1.000003815);
  o.area = (float)((double)o.square_radius * 4.0 * 3.14159265358979323846);
  o.samples = l.samples;
  return o;
}

// sunLight_t::sunLight_t, sunlight.cc:52-63, with the source's types:
// direction.normalize() normalizes the member while createCS takes the
// constructor's argument `dir` as given (un-normalized: du is its xy part
// normalized, dv = dir ^ du is as long as dir); angle is clamped to 80;
// cosAngle is a double holding the float fCos of degToRad(angle) (a double
// product) rounded to fCos's float parameter; invpdf = M_2PI * (1.f - cosAngle)
// and pdf = 1.0 / invpdf are double expressions stored to float.
yk_sun_light_state sun_state(const yk_light& l) {
  yk_sun_light_state o{};
  float d[3] = {l.direction[0], l.direction[1], l.direction[2]};
  create_cs(d, o.du, o.dv);
  float len = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];  // vector3d_t::normalize, vector3d.h:249-260
  if (len != 0.f) {
    len = 1.0f / std::sqrt(len);
    for (float& x : d) x *= len;
  }
  float angle = l.cone_angle;
  if (angle > 80.f) angle = 80.f;
  o.cos_angle = (double)host_fcos((float)((double)angle * 0.01745329251994329576922));
  o.invpdf = (float)(6.28318530717958647692 * ((double)1.f - o.cos_angle));
  o.pdf = (float)(1.0 / (double)o.invpdf);
  for (int k = 0; k < 3; ++k) {
    o.direction[k] = d[k];
    o.color[k] = l.color[k] * l.power;
    o.col_pdf[k] = o.color[k] * o.pdf;
  }
  o.samples = l.samples;
  return o;
}

int light_slots(const Scene& s, size_t i) {
  switch (s.light_kind[i]) {
    case YK_LIGHT_AREA: return 2 * s.light_states[i].samples;  // light samples + BSDF (MIS) samples
    case YK_LIGHT_SPOT: return s.spot_states[i].soft_shadows ? 2 * s.spot_states[i].samples : 1;
    case YK_LIGHT_SPHERE: return s.sphere_states[i].samples;  // canIntersect() is false: no MIS half
    case YK_LIGHT_MESH: return 2 * s.mesh_lights[i].params.samples;  // canIntersect(): light + BSDF halves
    case YK_LIGHT_SUN: return 2 * s.sun_states[i].samples;           // canIntersect(): light + BSDF halves
    case YK_LIGHT_BACKGROUND: return 2 * s.bg_lights[i].params.samples;  // canIntersect() (bglight.h:47)
    default: return 1;
  }
}

yk_camera_state camera_state(const yk_camera& c) {  // camera_t ctor + setAxis
  yk_camera_state o{};
  const hv3 pos = H(c.from), look = H(c.to), up = H(c.up);
  const float aspect = c.aspect_ratio * (float)c.resy / (float)c.resx;  // camera.h:44
  hv3 camY = hsub(up, pos), camZ = hsub(look, pos);
  hv3 camX = hcross(camZ, camY);
  camY = hcross(camZ, camX);
  camX = hnorm(camX);
  camY = hnorm(camY);
  camZ = hnorm(camZ);
  put(o.position, pos);
  put(o.cam_z, camZ);
  put(o.near_p, hadd(pos, hmul(c.near_clip, camZ)));
  put(o.far_p, hadd(pos, hmul(c.far_clip, camZ)));
  o.resx = c.resx;
  o.resy = c.resy;
  // The cameras below are restated in source order with the types the
  // reference's operators give each expression; how its -ffast-math build
  // orders them is not known (unpinned).
  if (c.type == YK_CAMERA_ORTHOGRAPHIC) {
    // orthoCam_t::setAxis (orthographicCamera.cc:37-49); the factory's double
    // scale reaches the ctor as PFLOAT. 0.5 * scale is a double product handed
    // to operator*(PFLOAT, vector3d_t); scale / (PFLOAT)res a float division.
    const float scale = (float)c.scale;
    hv3 vright = camX, vup = hmul(aspect, camY);
    put(o.vto, camZ);
    put(o.position, hsub(pos, hmul((float)(0.5 * (double)scale), hadd(vup, vright))));
    const float sy = scale / (float)c.resy, sx = scale / (float)c.resx;
    put(o.vup, {vup.x * sy, vup.y * sy, vup.z * sy});
    put(o.vright, {vright.x * sx, vright.y * sx, vright.z * sx});
    o.kind = YK_CAMERA_ORTHOGRAPHIC;
    return o;
  }
  if (c.type == YK_CAMERA_ANGULAR) {
    // angularCam_t ctor + setAxis + the factory's tail (angularCamera.cc:27-47,
    // 96-98): hor_phi(angle * M_PI / 180.f) with the PFLOAT ctor argument,
    // vright *= -1.0 when mirrored, max_r = max_angle / angle in double
    const float angle = (float)c.angle;
    o.hor_phi = (float)((double)angle * 3.14159265358979323846 / (double)180.f);
    put(o.vright, c.mirrored ? hmul(-1.0f, camX) : camX);
    put(o.vup, camY);
    put(o.vto, camZ);
    o.max_r = (float)(c.max_angle / c.angle);
    o.circular = c.circular ? 1 : 0;
    o.aspect_ratio = aspect;
    o.kind = YK_CAMERA_ANGULAR;
    return o;
  }
  // depth of field: setAxis's dof_rt / dof_up, the ctor's polygon table
  // (perspectiveCamera.cc:29-50, 57-62)
  o.aperture = c.aperture;
  o.dof_distance = c.dof_distance;
  put(o.dof_rt, hmul(c.aperture, camX));
  put(o.dof_up, hmul(c.aperture, camY));
  o.bokeh_type = c.bokeh_type;
  o.bokeh_bias = c.bokeh_bias;
  if (c.bokeh_type >= YK_BOKEH_TRI && c.bokeh_type <= YK_BOKEH_HEXA) {
    const int ns = c.bokeh_type;
    float w = (float)((double)c.bokeh_rotation * 0.01745329251994329576922);  // degToRad
    const float wi = (float)(6.28318530717958647692 / (double)(float)ns);    // M_2PI / ns
    for (int i = 0; i < (ns + 2) * 2; i += 2) {
      o.lens_ls[i] = host_fcos(w);
      o.lens_ls[i + 1] = host_fsin(w);
      w += wi;
    }
  }
  // architectCam_t::setAxis (architectCamera.cc:54-68) differs in vup alone:
  // aspect_ratio * vector3d_t(0, 0, -1); its ctor repeats the lens table above
  const hv3 vright = camX, vup = hmul(aspect, c.type == YK_CAMERA_ARCHITECT ? hv3{0.f, 0.f, -1.f} : camY);
  put(o.vto, hsub(hmul(c.focal, camZ), hmul(0.5f, hadd(vup, vright))));
  const float ry = 1.0f / (float)c.resy, rx = 1.0f / (float)c.resx;  // compiled form of "/= res"
  put(o.vup, {vup.x * ry, vup.y * ry, vup.z * ry});
  put(o.vright, {vright.x * rx, vright.y * rx, vright.z * rx});
  return o;
}

int Scene::add_material(const yk_material& m, const yk_glass_params* g) {
  materials.push_back(m);
  material_has_params.push_back(true);
  yk_glass_state gs{};
  if (m.type == YK_MAT_GLASS) {
    const yk_glass_params def{{1.f, 1.f, 1.f}, 0, 0.0};  // the factory's defaults
    material_states.push_back(glass_material_state(m, g ? *g : def, gs));
  } else {
    material_states.push_back(material_state(m));
  }
  glass_states.push_back(gs);
  built = false;
  return (int)material_states.size() - 1;
}
int Scene::add_material_state(const yk_material_state& m, const yk_glass_state* g) {
  materials.push_back(yk_material{});
  material_has_params.push_back(false);
  material_states.push_back(m);
  yk_glass_state gs{};
  if (m.type == YK_MAT_GLASS) gs = g ? *g : yk_glass_state{{1.f, 1.f, 1.f}, 0};
  glass_states.push_back(gs);
  built = false;
  return (int)material_states.size() - 1;
}
void Scene::add_light(const yk_light& l) {
  lights.push_back(l);
  light_has_params.push_back(true);
  light_kind.push_back(l.type);
  yk_area_light_state a{};
  a.samples = 1;
  light_states.push_back(l.type == YK_LIGHT_AREA ? light_state(l) : a);
  dirac_states.push_back(l.type == YK_LIGHT_POINT || l.type == YK_LIGHT_DIRECTIONAL ? dirac_state(l)
                                                                                  : yk_dirac_light_state{});
  spot_states.push_back(l.type == YK_LIGHT_SPOT ? spot_state(l) : yk_spot_light_state{});
  sphere_states.push_back(l.type == YK_LIGHT_SPHERE ? sphere_state(l) : yk_sphere_light_state{});
  mesh_lights.emplace_back();
  sun_states.push_back(l.type == YK_LIGHT_SUN ? sun_state(l) : yk_sun_light_state{});
  bg_lights.emplace_back();
}
void Scene::add_dirac_light_state(const yk_dirac_light_state& l) {
  lights.push_back(yk_light{});
  light_has_params.push_back(false);
  light_kind.push_back(l.type);
  yk_area_light_state a{};
  a.samples = 1;
  light_states.push_back(a);
  dirac_states.push_back(l);
  spot_states.push_back(yk_spot_light_state{});
  sphere_states.push_back(yk_sphere_light_state{});
  mesh_lights.emplace_back();
  sun_states.push_back(yk_sun_light_state{});
  bg_lights.emplace_back();
}
void Scene::add_light_state(const yk_area_light_state& l) {
  lights.push_back(yk_light{});
  light_has_params.push_back(false);
  light_kind.push_back(YK_LIGHT_AREA);
  light_states.push_back(l);
  dirac_states.push_back(yk_dirac_light_state{});
  spot_states.push_back(yk_spot_light_state{});
  sphere_states.push_back(yk_sphere_light_state{});
  mesh_lights.emplace_back();
  sun_states.push_back(yk_sun_light_state{});
  bg_lights.emplace_back();
}
void Scene::add_spot_light_state(const yk_spot_light_state& l) {
  lights.push_back(yk_light{});
  light_has_params.push_back(false);
  light_kind.push_back(YK_LIGHT_SPOT);
  yk_area_light_state a{};
  a.samples = 1;
  light_states.push_back(a);
  dirac_states.push_back(yk_dirac_light_state{});
  spot_states.push_back(l);
  sphere_states.push_back(yk_sphere_light_state{});
  mesh_lights.emplace_back();
  sun_states.push_back(yk_sun_light_state{});
  bg_lights.emplace_back();
}
void Scene::add_sphere_light_state(const yk_sphere_light_state& l) {
  lights.push_back(yk_light{});
  light_has_params.push_back(false);
  light_kind.push_back(YK_LIGHT_SPHERE);
  yk_area_light_state a{};
  a.samples = 1;
  light_states.push_back(a);
  dirac_states.push_back(yk_dirac_light_state{});
  spot_states.push_back(yk_spot_light_state{});
  sphere_states.push_back(l);
  mesh_lights.emplace_back();
  sun_states.push_back(yk_sun_light_state{});
  bg_lights.emplace_back();
}
void Scene::add_sun_light_state(const yk_sun_light_state& l) {
  lights.push_back(yk_light{});
  light_has_params.push_back(false);
  light_kind.push_back(YK_LIGHT_SUN);
  yk_area_light_state a{};
  a.samples = 1;
  light_states.push_back(a);
  dirac_states.push_back(yk_dirac_light_state{});
  spot_states.push_back(yk_spot_light_state{});
  sphere_states.push_back(yk_sphere_light_state{});
  mesh_lights.emplace_back();
  sun_states.push_back(l);
  bg_lights.emplace_back();
}
// meshLight_t::factory (meshlight.cc:221-236): color * (CFLOAT)power * M_PI,
// both through color_t's operator*(color_t, CFLOAT): float products
void Scene::add_mesh_light(const yk_mesh_light& l, const int32_t* obj_ids, int nobj) {
  MeshLight m;
  m.params = l;
  m.params.double_sided = l.double_sided ? 1 : 0;
  for (int k = 0; k < 3; ++k) m.color[k] = (l.color[k] * l.power) * (float)3.14159265358979323846;
  m.obj_ids.assign(obj_ids, obj_ids + nobj);
  yk_light p{};
  p.type = YK_LIGHT_MESH;
  for (int k = 0; k < 3; ++k) p.color[k] = l.color[k];
  p.power = l.power;
  p.samples = l.samples;
  lights.push_back(p);
  light_has_params.push_back(true);
  light_kind.push_back(YK_LIGHT_MESH);
  yk_area_light_state a{};
  a.samples = 1;
  light_states.push_back(a);
  dirac_states.push_back(yk_dirac_light_state{});
  spot_states.push_back(yk_spot_light_state{});
  sphere_states.push_back(yk_sphere_light_state{});
  mesh_lights.push_back(std::move(m));
  sun_states.push_back(yk_sun_light_state{});
  bg_lights.emplace_back();
  built = false;
}
void Scene::add_background_light(const yk_background_light& l) {
  BgLight b;
  b.params = l;
  b.params.shoot_caustics = l.shoot_caustics ? 1 : 0;
  b.params.shoot_diffuse = l.shoot_diffuse ? 1 : 0;
  b.params.abs_intersect = l.abs_intersect ? 1 : 0;
  b.present = true;
  yk_light p{};
  p.type = YK_LIGHT_BACKGROUND;
  p.samples = l.samples;
  lights.push_back(p);
  light_has_params.push_back(false);
  light_kind.push_back(YK_LIGHT_BACKGROUND);
  yk_area_light_state a{};
  a.samples = 1;
  light_states.push_back(a);
  dirac_states.push_back(yk_dirac_light_state{});
  spot_states.push_back(yk_spot_light_state{});
  sphere_states.push_back(yk_sphere_light_state{});
  mesh_lights.emplace_back();
  sun_states.push_back(yk_sun_light_state{});
  bg_lights.push_back(std::move(b));
  built = false;
}
// gradientBackground_t::factory (gradientback.cc:83-97): each colour times power
void Scene::set_gradient_background(const yk_gradient_background* g) {
  has_gradient = g != nullptr;
  gradient_params = g ? *g : yk_gradient_background{};
  for (int k = 0; k < 3; ++k) {
    gradient[k] = g ? g->zenith_color[k] * g->power : 0.f;
    gradient[3 + k] = g ? g->horizon_color[k] * g->power : 0.f;
    gradient[6 + k] = g ? g->zenith_ground_color[k] * g->power : 0.f;
    gradient[9 + k] = g ? g->horizon_ground_color[k] * g->power : 0.f;
  }
  if (g) {
    has_background = false;
    for (float& x : background) x = 0.f;
  }
}
void Scene::set_camera(const yk_camera& c) {
  camera = c;
  camera_has_params = true;
  camera_state = yk::camera_state(c);
  has_camera = true;
}
void Scene::set_camera_state(const yk_camera_state& c) {
  camera = yk_camera{};
  camera_has_params = false;
  camera_state = c;
  has_camera = true;
}

void rec_normal(const float* t, float* n) {
  // triangle_t::recNormal, triangle_inline.h:100-107
  float e1x = t[3] - t[0], e1y = t[4] - t[1], e1z = t[5] - t[2];
  float e2x = t[6] - t[0], e2y = t[7] - t[1], e2z = t[8] - t[2];
  float x = e1y * e2z - e1z * e2y;
  float y = e1z * e2x - e1x * e2z;
  float z = e1x * e2y - e1y * e2x;
  float len = x * x + y * y + z * z;  // vector3d_t::normalize, vector3d.h:249-260
  if (len != 0) {
    len = 1.0f / std::sqrt(len);
    x *= len;
    y *= len;
    z *= len;
  }
  n[0] = x;
  n[1] = y;
  n[2] = z;
}

// matrix4x4_t * point3d_t, compiled form of the instance's getVertex
// (meshtypes.h:140-143): each row as (m0*x + m1*y) + (m2*z + m3)
float host_fsin(float x) {
  const double pi = 3.14159265358979323846, two_pi = 6.28318530717958647692;
  if ((double)x > two_pi || (double)x < -two_pi)
    x -= (float)((int)(x * (float)0.15915494309189533577)) * (float)two_pi;
  if ((double)x < -pi) x += (float)two_pi;
  else if ((double)x > pi) x -= (float)two_pi;
  x = ((float)1.27323954473516268615 * x) - (((float)0.40528473456935108578 * x) * std::fabs(x));
  float r = x + (std::fabs(x) - 1.0f) * (0.225f * x);
  if (r > 1.0f) r = 1.0f;
  if (r < -1.0f) r = -1.0f;
  return r;
}

static void xform_point(const float* m, const float* p, float* o) {
  for (int r = 0; r < 3; ++r) {
    const float* a = m + 4 * r;
    o[r] = (a[0] * p[0] + a[1] * p[1]) + (a[2] * p[2] + a[3]);
  }
}
// matrix4x4_t * vector3d_t, compiled form of getVertexNormal / getNormal of
// instances: each row as (m0*x + m2*z) + m1*y
static void xform_vector(const float* m, const float* v, float* o) {
  for (int r = 0; r < 3; ++r) {
    const float* a = m + 4 * r;
    o[r] = (a[0] * v[0] + a[2] * v[2]) + a[1] * v[1];
  }
}
// vector3d_t::normalize, vector3d.h:249-260
static void normalize3(float* v) {
  float len = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
  if (len != 0.f) {
    len = 1.0f / std::sqrt(len);
    v[0] *= len;
    v[1] *= len;
    v[2] *= len;
  }
}

// meshLight_t::initIS (meshlight.cc:47-65), source order: the triangles of
// the light's meshes in getPrimitives order, triangle_t::surfaceArea
// (triangle.cc:144-154: float cross product and length, the 0.5 * in double),
// the double running total, pdf1D_t's cdf (CumulateStep1dDF, sample_utils.h:
// 85-98) and the light's own triKdTree_t(tris, nTris, -1, 1, 0.8, 0.33)
static void init_mesh_light(const Scene& S, MeshLight& L) {
  L.verts.clear();
  L.normals.clear();
  L.areas.clear();
  for (const int32_t id : L.obj_ids) {
    const Mesh& m = S.meshes[(size_t)id - 1];
    const size_t nf = m.faces.size() / 3;
    const int np = (int)(m.points.size() / 3);
    for (size_t f = 0; f < nf; ++f) {
      float tv[9];
      for (int k = 0; k < 3; ++k) {
        const int vi = m.faces[3 * f + k];
        if (vi < 0 || vi >= np) throw std::invalid_argument("mesh face references a missing vertex");
        for (int c = 0; c < 3; ++c) tv[3 * k + c] = m.points[3 * vi + c];
      }
      L.verts.insert(L.verts.end(), tv, tv + 9);
      float nrm[3];
      rec_normal(tv, nrm);
      L.normals.insert(L.normals.end(), nrm, nrm + 3);
      const float e1x = tv[3] - tv[0], e1y = tv[4] - tv[1], e1z = tv[5] - tv[2];
      const float e2x = tv[6] - tv[0], e2y = tv[7] - tv[1], e2z = tv[8] - tv[2];
      const float x = e1y * e2z - e1z * e2y, y = e1z * e2x - e1x * e2z, z = e1x * e2y - e1y * e2x;
      L.areas.push_back((float)(0.5 * (double)std::sqrt(x * x + y * y + z * z)));
    }
  }
  const int n = (int)L.areas.size();
  if (n == 0) throw std::invalid_argument("mesh light has no triangles");
  double total = 0.0;
  for (int i = 0; i < n; ++i) total += (double)L.areas[i];
  L.area = (float)total;
  L.inv_area = (float)(1.0 / total);
  L.cdf.assign((size_t)n + 1, 0.f);
  double c = 0.0;
  const double delta = 1.0 / (double)n;
  for (int i = 1; i < n + 1; ++i) {
    c += (double)L.areas[i - 1] * delta;
    L.cdf[i] = (float)c;
  }
  const float integral = (float)c;
  if (!(total > 0.0) || !(integral > 0.f)) throw std::invalid_argument("mesh light has zero total area");
  for (int i = 1; i < n + 1; ++i) L.cdf[i] /= integral;
  build_kdtree(L.verts.data(), n, L.tree, -1, 1, 0.8f, 0.33f);
}

void background_eval(int kind, const float* constant, const float* grad, const float* dir, float* rgb) {
  if (kind != YK_BG_GRADIENT) {
    for (int k = 0; k < 3; ++k) rgb[k] = constant[k];
    return;
  }
  float blend = dir[2];
  const float* z = grad;
  if (!(blend >= 0.f)) {
    blend = -blend;
    z = grad + 6;
  }
  for (int k = 0; k < 3; ++k) rgb[k] = blend * z[k] + (1.f - blend) * z[3 + k];
  if (std::min(rgb[0], std::min(rgb[1], rgb[2])) < 1e-6f) rgb[0] = rgb[1] = rgb[2] = 1e-5f;
}

// pdf1D_t's constructor (sample_utils.h:109-118) with CumulateStep1dDF (:85-98):
// the double running total, cdf[i] = float(c), integral = (float)c, then each
// cdf entry divided by the float integral
static void pdf1d(const float* f, int n, float* cdf, float& integral, float& inv_integral) {
  double c = 0.0;
  const double delta = 1.0 / (double)n;
  cdf[0] = 0.f;
  for (int i = 1; i < n + 1; ++i) {
    c += (double)f[i - 1] * delta;
    cdf[i] = (float)c;
  }
  integral = (float)c;
  for (int i = 1; i < n + 1; ++i) cdf[i] /= integral;
  inv_integral = 1.f / integral;
}

// bgLight_t::init (bglight.cc:68-118) up to the tables, source order:
// MAX_VSAMPLES rows; per row fy = (y + 0.5f) * inv, sintheta = fSin of the
// double fy * M_PI narrowed at the call, nu = MIN_SAMPLES + (int)(sintheta *
// (MAX_USAMPLES - MIN_SAMPLES)) columns of eval(invSpheremap(fx, fy)).energy()
// * sintheta; invSpheremap is texture.h:93-102 (theta = v * M_PI and phi =
// -(u * M_2PI) are double products stored to float). The members taken from
// the scene bound come at upload (make_bg_light).
static void init_bg_light(const Scene& S, BgLight& L) {
  constexpr int kMaxV = 360, kMaxU = 720, kMin = 16;
  const int kind = S.background_kind();
  const int nv = kMaxV;
  const float inv = 1.f / (float)nv;
  L.row_count.assign(nv, 0);
  L.row_offset.assign(nv, 0);
  L.row_integral.assign(nv, 0.f);
  L.row_inv_integral.assign(nv, 0.f);
  L.func_u.clear();
  L.cdf_u.clear();
  L.func_v.assign(nv, 0.f);
  L.cdf_v.assign((size_t)nv + 1, 0.f);
  float fu[kMaxU];
  for (int y = 0; y < nv; ++y) {
    const float fy = ((float)y + 0.5f) * inv;
    const float sintheta = host_fsin((float)((double)fy * 3.14159265358979323846));
    const int nu = kMin + (int)(sintheta * (float)(kMaxU - kMin));
    const float inu = 1.f / (float)nu;
    for (int x = 0; x < nu; ++x) {
      const float fx = ((float)x + 0.5f) * inu;
      const float theta = (float)((double)fy * 3.14159265358979323846);
      const float phi = (float)-((double)fx * 6.28318530717958647692);
      const float ct = host_fcos(theta), st = host_fsin(theta);
      const float cp = host_fcos(phi), sp = host_fsin(phi);
      const float dir[3] = {st * cp, st * sp, -ct};
      float c[3];
      background_eval(kind, S.background, S.gradient, dir, c);
      fu[x] = (((c[0] + c[1]) + c[2]) * 0.333333f) * sintheta;  // color_t::energy(), color.h
    }
    L.row_count[y] = nu;
    L.row_offset[y] = (int32_t)L.func_u.size();
    L.func_u.insert(L.func_u.end(), fu, fu + nu);
    const size_t at = L.cdf_u.size();
    L.cdf_u.resize(at + (size_t)nu + 1);
    pdf1d(fu, nu, &L.cdf_u[at], L.row_integral[y], L.row_inv_integral[y]);
    L.func_v[y] = L.row_integral[y];
  }
  pdf1d(L.func_v.data(), nv, L.cdf_v.data(), L.v_integral, L.v_inv_integral);
}

void Scene::finalize() {
  // scene_t::update, scene.cc:755-782: visible non-base TRIM meshes and
  // instances in object id order, triangles in insertion order. Universal
  // mode (scene.cc:791-819): the VTRIM meshes in object id order, visible or
  // not; vTriangle_t::getSurface smooths with is_smooth and takes normal
  // index 0 as "none" (na > 0, triangle.cc:410-415).
  auto t0 = std::chrono::steady_clock::now();
  const bool uni = mode == YK_MODE_UNIVERSAL;
  tri_verts.clear();
  tri_material.clear();
  tri_normal.clear();
  tri_smooth.clear();
  tri_vnormal.clear();
  any_smooth = false;
  for (const Mesh& inst : meshes) {
    if (uni ? inst.type != YK_MESH_VTRIM : (!inst.visible || inst.is_base || inst.type != YK_MESH_TRIM)) continue;
    const bool is_inst = inst.instance_of >= 0;
    const Mesh& m = is_inst ? meshes[inst.instance_of] : inst;
    const size_t nf = m.faces.size() / 3;
    const int np = (int)(m.points.size() / 3);
    const int nn = (int)(m.normals.size() / 3);
    // triangle_t::getSurface smooths with is_smooth; triangleInstance_t with
    // is_smooth || normals_exported and treats normal index 0 as missing
    // (triangle.cc:19-26 vs 185-192)
    const bool smooth = is_inst ? (m.is_smooth || m.normals_exported) : m.is_smooth;
    const bool idx0_none = is_inst || uni;  // normal index 0 treated as missing
    for (size_t f = 0; f < nf; ++f) {
      float tv[9], base_tv[9];
      for (int k = 0; k < 3; ++k) {
        int vi = m.faces[3 * f + k];
        if (vi < 0 || vi >= np) throw std::invalid_argument("mesh face references a missing vertex");
        for (int c = 0; c < 3; ++c) base_tv[3 * k + c] = m.points[3 * vi + c];
        if (is_inst) xform_point(inst.m, base_tv + 3 * k, tv + 3 * k);
        else for (int c = 0; c < 3; ++c) tv[3 * k + c] = base_tv[3 * k + c];
      }
      tri_verts.insert(tri_verts.end(), tv, tv + 9);
      tri_material.push_back(m.material);
      float nrm[3];
      rec_normal(base_tv, nrm);  // the (base) triangle's recNormal
      if (is_inst) {  // triangleInstance_t::getNormal: normalize(objToWorld * base normal)
        float t[3];
        xform_vector(inst.m, nrm, t);
        normalize3(t);
        nrm[0] = t[0];
        nrm[1] = t[1];
        nrm[2] = t[2];
      }
      tri_normal.insert(tri_normal.end(), nrm, nrm + 3);
      float vn[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      if (smooth) {
        for (int k = 0; k < 3; ++k) {
          const int ni = m.face_normals.empty() ? -1 : m.face_normals[3 * f + k];
          const bool has = idx0_none ? (ni > 0) : (ni >= 0);
          if (has && ni >= nn) throw std::invalid_argument("face references a missing vertex normal");
          if (has) {
            if (is_inst) xform_vector(inst.m, &m.normals[3 * ni], vn + 3 * k);
            else for (int c = 0; c < 3; ++c) vn[3 * k + c] = m.normals[3 * ni + c];
          } else {
            for (int c = 0; c < 3; ++c) vn[3 * k + c] = nrm[c];  // sp.Ng
          }
        }
        any_smooth = true;
      }
      tri_smooth.push_back(smooth ? 1 : 0);
      tri_vnormal.insert(tri_vnormal.end(), vn, vn + 9);
    }
  }
  const int ntris = (int)tri_material.size();
  if (ntris == 0) throw std::invalid_argument("scene is empty");
  build_kdtree(tri_verts.data(), ntris, tree);
  for (MeshLight& L : mesh_lights)
    if (!L.obj_ids.empty()) init_mesh_light(*this, L);
  for (BgLight& L : bg_lights)
    if (L.present) init_bg_light(*this, L);
  static std::atomic<uint64_t> next_generation{1};
  generation = next_generation.fetch_add(1);
  built = true;
  build_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// scene_t::endCurveMesh (scene.cc:138-264): a strand polyline extruded to a
// triangular prism, in the compiled operation order of the survey build
// (-O3 -ffast-math, read from its disassembly):
//   (float)i/(n-1)       -> i * (1.0f/(n-1))
//   r                    -> start + pow(t, 1+shape)*(end-start)         (shape < 0)
//                           start + (1 - pow(t', 1-shape))*(end-start)  (else)
//   1.5*r/sqrt(3.f)      -> (float)((double)r * (1.5/(double)sqrtf(3)))
//   a, b                 -> (o - (0.5r)*v) -/+ c*u per component; u.z == 0
// Points: the n centre points, then a_i, b_i per point; faces: bottom cap,
// 6 per segment, top cap (2 + 6(n-1) triangles).
Mesh curve_mesh(const float* pts, int n, int material, float strand_start, float strand_end, float strand_shape) {
  if (n < 2) throw std::invalid_argument("a curve needs at least 2 points");
  Mesh m;
  m.material = material;
  m.points.assign(pts, pts + 3 * (size_t)n);
  m.points.reserve(9 * (size_t)n);
  const float inv_nm1 = 1.0f / (float)(n - 1);
  const float span = strand_end - strand_start;
  const double k_half_w = 1.5 / (double)std::sqrt(3.0f);
  float ux = 0, uy = 0, vx = 0, vy = 0, vz = 0;
  for (int i = 0; i < n; ++i) {
    const float* o = pts + 3 * i;
    float r;
    if (strand_shape < 0)
      r = std::pow((float)i * inv_nm1, 1.0f + strand_shape) * span + strand_start;
    else
      r = (1.0f - std::pow((float)(n - i - 1) * inv_nm1, 1.0f - strand_shape)) * span + strand_start;
    if (i < n - 1) {  // the last point keeps the previous tangent frame
      float N[3] = {o[3] - o[0], o[4] - o[1], o[5] - o[2]};
      const float len = (N[0] * N[0] + N[1] * N[1]) + N[2] * N[2];
      if (len != 0.f) {
        const float inv = 1.0f / std::sqrt(len);
        N[0] *= inv;
        N[1] *= inv;
        N[2] *= inv;
      }
      if (N[0] == 0.f && N[1] == 0.f) {  // createCS, vector3d.h:316-334
        ux = N[2] < 0.f ? -1.f : 1.f;
        uy = 0.f;
        vx = 0.f;
        vy = 1.f;
        vz = 0.f;
      } else {
        const float d = 1.0f / std::sqrt(N[1] * N[1] + N[0] * N[0]);
        ux = N[1] * d;
        uy = -(N[0] * d);
        vx = -(N[2] * uy);
        vy = N[2] * ux;
        vz = N[0] * uy - N[1] * ux;
      }
    }
    const float h = r * 0.5f;
    const float c = (float)((double)r * k_half_w);
    const float px = o[0] - h * vx, py = o[1] - h * vy, pz = o[2] - h * vz;
    const float a[3] = {px - c * ux, py - c * uy, pz}, b[3] = {px + c * ux, py + c * uy, pz};
    m.points.insert(m.points.end(), a, a + 3);
    m.points.insert(m.points.end(), b, b + 3);
  }
  m.faces.reserve(3 * (size_t)(6 * (n - 1) + 2));
  int i = 0;
  for (; i < n - 1; ++i) {
    const int a1 = i, a2 = 2 * i + n, a3 = a2 + 1, b1 = i + 1, b2 = a2 + 2, b3 = b2 + 1;
    if (i == 0) m.faces.insert(m.faces.end(), {a1, a3, a2});
    m.faces.insert(m.faces.end(), {a1, b2, b1, a1, a2, b2, a2, b3, b2, a2, a3, b3, b3, a3, a1, b3, a1, b1});
  }
  m.faces.insert(m.faces.end(), {i, 2 * i + n, 2 * i + n + 1});
  return m;
}

namespace {

inline float atof_f(double v) { return (float)v; }  // xmlparser.cc:237-239: atof -> float

void add_quad(Scene& s, const double p[4][3], int mat) {
  Mesh m;
  for (int i = 0; i < 4; ++i)
    for (int k = 0; k < 3; ++k) m.points.push_back(atof_f(p[i][k]));
  m.faces = {0, 1, 2, 0, 2, 3};
  m.material = mat;
  s.meshes.push_back(m);
}

void add_box(Scene& s, double cx, double cz, double sx, double sz, double h, int mat) {
  const double x0 = cx - sx, x1 = cx + sx, z0 = cz - sz, z1 = cz + sz;
  const double v[8][3] = {{x0, 0, z0}, {x1, 0, z0}, {x1, 0, z1}, {x0, 0, z1},
                          {x0, h, z0}, {x1, h, z0}, {x1, h, z1}, {x0, h, z1}};
  static const int f[12][3] = {{4, 5, 6}, {4, 6, 7}, {0, 1, 5}, {0, 5, 4}, {1, 2, 6}, {1, 6, 5},
                               {2, 3, 7}, {2, 7, 6}, {3, 0, 4}, {3, 4, 7}, {0, 2, 1}, {0, 3, 2}};
  Mesh m;
  for (int i = 0; i < 8; ++i)
    for (int k = 0; k < 3; ++k) m.points.push_back(atof_f(v[i][k]));
  for (int i = 0; i < 12; ++i)
    for (int k = 0; k < 3; ++k) m.faces.push_back(f[i][k]);
  m.material = mat;
  s.meshes.push_back(m);
}

int add_mat(Scene& s, int type, float r, float g, float b, float power) {
  yk_material m{};
  m.type = type;
  m.color[0] = r;
  m.color[1] = g;
  m.color[2] = b;
  m.diffuse_reflect = 1.f;
  m.emit = 0.f;
  m.power = power;
  m.double_sided = 0;
  m.mirror_color[0] = m.mirror_color[1] = m.mirror_color[2] = 1.f;  // factory defaults
  m.transmit_filter = 1.f;
  m.ior = 1.33;
  return s.add_material(m);
}

// value as the XML loader sees a "%.6f" formatted coordinate: strtod of the
// text, then (float) (xmlparser.cc:237-239)
inline float fmt6(double v) {
  char buf[64];
  std::snprintf(buf, sizeof buf, "%.6f", v);
  return (float)std::strtod(buf, nullptr);
}

}  // namespace

// Cornell probe of BASELINE.md "Probe scenes": 5 walls (10 tris), two boxes
// (24 tris), light quad (2 tris) = 36 tris; area light with 4 samples.
void gen_cornell(Scene& s, int resx, int resy) {
  s = Scene();
  const int white = add_mat(s, YK_MAT_SHINYDIFFUSE, 0.8f, 0.8f, 0.8f, 1.f);
  const int red = add_mat(s, YK_MAT_SHINYDIFFUSE, 0.8f, 0.1f, 0.1f, 1.f);
  const int green = add_mat(s, YK_MAT_SHINYDIFFUSE, 0.1f, 0.8f, 0.1f, 1.f);
  const int lightm = add_mat(s, YK_MAT_LIGHT, 1.f, 1.f, 1.f, 10.f);
  const double floor_[4][3] = {{-1, 0, -1}, {1, 0, -1}, {1, 0, 1}, {-1, 0, 1}};
  const double ceil_[4][3] = {{-1, 2, -1}, {-1, 2, 1}, {1, 2, 1}, {1, 2, -1}};
  const double back_[4][3] = {{-1, 0, 1}, {1, 0, 1}, {1, 2, 1}, {-1, 2, 1}};
  const double left_[4][3] = {{-1, 0, -1}, {-1, 0, 1}, {-1, 2, 1}, {-1, 2, -1}};
  const double right_[4][3] = {{1, 0, -1}, {1, 2, -1}, {1, 2, 1}, {1, 0, 1}};
  const double lq[4][3] = {{-0.25, 1.98, -0.25}, {-0.25, 1.98, 0.25}, {0.25, 1.98, 0.25}, {0.25, 1.98, -0.25}};
  add_quad(s, floor_, white);
  add_quad(s, ceil_, white);
  add_quad(s, back_, white);
  add_quad(s, left_, red);
  add_quad(s, right_, green);
  add_box(s, -0.35, 0.3, 0.3, 0.3, 1.2, white);
  add_box(s, 0.4, -0.3, 0.3, 0.3, 0.6, white);
  add_quad(s, lq, lightm);
  yk_light l{};
  l.type = YK_LIGHT_AREA;
  const float c[3] = {-0.25f, 1.979f, -0.25f}, p1[3] = {0.25f, 1.979f, -0.25f}, p2[3] = {-0.25f, 1.979f, 0.25f};
  for (int k = 0; k < 3; ++k) {
    l.corner[k] = c[k];
    l.point1[k] = p1[k];
    l.point2[k] = p2[k];
    l.color[k] = 1.f;
  }
  l.power = 10.f;
  l.samples = 4;
  s.add_light(l);
  yk_camera cam{};
  const float from[3] = {0, 1, -3.6f}, to[3] = {0, 1, 0}, up[3] = {0, 2, -3.6f};
  for (int k = 0; k < 3; ++k) {
    cam.from[k] = from[k];
    cam.to[k] = to[k];
    cam.up[k] = up[k];
  }
  cam.resx = resx;
  cam.resy = resy;
  cam.focal = 1.3f;
  cam.aspect_ratio = 1.f;
  cam.near_clip = 0.f;
  cam.far_clip = -1.f;
  s.set_camera(cam);
}

// 1M-triangle probe of BASELINE.md: displaced UV sphere (NU x NV grid,
// 2*NU*(NV-1) tris) centred at (0,1.2,0) over a 2-tri 6x6 floor, 1x1 area light
// at y=3 with 1 sample. Coordinates go through "%.6f" text like the XML.
void gen_bumpy(Scene& s, int nu, int nv, int resx, int resy) {
  s = Scene();
  const int white = add_mat(s, YK_MAT_SHINYDIFFUSE, 0.8f, 0.8f, 0.8f, 1.f);
  const int red = add_mat(s, YK_MAT_SHINYDIFFUSE, 0.8f, 0.1f, 0.1f, 1.f);
  {
    Mesh m;
    const double fl[4][3] = {{-3, 0, -3}, {3, 0, -3}, {3, 0, 3}, {-3, 0, 3}};
    for (int i = 0; i < 4; ++i)
      for (int k = 0; k < 3; ++k) m.points.push_back(fmt6(fl[i][k]));
    m.faces = {0, 2, 1, 0, 3, 2};
    m.material = white;
    s.meshes.push_back(m);
  }
  {
    Mesh m;
    m.points.reserve((size_t)nu * nv * 3);
    const double pi = 3.141592653589793;
    for (int j = 0; j < nv; ++j) {
      const double th = pi * (double)j / (double)(nv - 1);
      for (int i = 0; i < nu; ++i) {
        const double ph = 2.0 * pi * (double)i / (double)nu;
        const double r = 1.0 + 0.08 * std::sin(7.0 * th) * std::cos(9.0 * ph) +
                         0.03 * std::sin(23.0 * th + 5.0 * ph);
        const double sth = std::sin(th), cth = std::cos(th);
        m.points.push_back(fmt6(r * sth * std::cos(ph)));
        m.points.push_back(fmt6(1.2 + r * cth));
        m.points.push_back(fmt6(r * sth * std::sin(ph)));
      }
    }
    m.faces.reserve((size_t)nu * (nv - 1) * 6);
    for (int j = 0; j < nv - 1; ++j)
      for (int i = 0; i < nu; ++i) {
        const int a = j * nu + i, b = j * nu + (i + 1) % nu, c = a + nu, d = b + nu;
        m.faces.insert(m.faces.end(), {a, c, b, b, c, d});
      }
    m.material = red;
    s.meshes.push_back(m);
  }
  yk_light l{};
  l.type = YK_LIGHT_AREA;
  const float c[3] = {-0.5f, 3.f, -0.5f}, p1[3] = {0.5f, 3.f, -0.5f}, p2[3] = {-0.5f, 3.f, 0.5f};
  for (int k = 0; k < 3; ++k) {
    l.corner[k] = c[k];
    l.point1[k] = p1[k];
    l.point2[k] = p2[k];
    l.color[k] = 1.f;
  }
  l.power = 8.f;
  l.samples = 1;
  s.add_light(l);
  yk_camera cam{};
  const float from[3] = {0, 1.5f, -4.f}, to[3] = {0, 1.2f, 0}, up[3] = {0, 2.5f, -4.f};
  for (int k = 0; k < 3; ++k) {
    cam.from[k] = from[k];
    cam.to[k] = to[k];
    cam.up[k] = up[k];
  }
  cam.resx = resx;
  cam.resy = resy;
  cam.focal = 1.4f;
  cam.aspect_ratio = 1.f;
  cam.near_clip = 0.f;
  cam.far_clip = -1.f;
  s.set_camera(cam);
}

// C5 probe: hair. A flat-shaded head sphere (200x101
// grid) at (0,1.2,0) over the 6x6 floor, with `nstrands` <curve> strands of
// `npoints` points (6(n-1)+2 triangles each, scene.cc:138-264) rooted on a
// Fibonacci spiral over the upper 80 % of the sphere and drooping under a
// fixed bend; strand thickness 0.012 -> 0.004, shape alternating -0.3 / 0.3
// (both branches of the radius law). 200,000 strands x 9 points = 10.0M
// strand triangles. Coordinates go through "%.6f" text like the XML.
void gen_hair(Scene& s, int nstrands, int npoints, int resx, int resy) {
  gen_bumpy(s, 200, 101, resx, resy);
  s.meshes[1].material = 0;
  const int hair_a = add_mat(s, YK_MAT_SHINYDIFFUSE, 0.45f, 0.3f, 0.15f, 1.f);
  const int hair_b = add_mat(s, YK_MAT_SHINYDIFFUSE, 0.3f, 0.2f, 0.1f, 1.f);
  const double pi = 3.141592653589793, golden = pi * (3.0 - std::sqrt(5.0));
  {  // key light in front of the head (the top light is mostly blocked by the hair)
    yk_light l = s.lights[0];
    const float c[3] = {-1.f, 1.5f, -3.f}, p1[3] = {1.f, 1.5f, -3.f}, p2[3] = {-1.f, 2.5f, -3.f};
    for (int k = 0; k < 3; ++k) {
      l.corner[k] = c[k];
      l.point1[k] = p1[k];
      l.point2[k] = p2[k];
    }
    l.power = 3.f;
    s.add_light(l);
  }
  const double len = 0.7;
  std::vector<float> pts(3 * (size_t)npoints);
  s.meshes.reserve(s.meshes.size() + nstrands);
  for (int k = 0; k < nstrands; ++k) {
    const double y = 1.0 - 1.8 * (k + 0.5) / nstrands;  // root height on the unit sphere
    const double rr = std::sqrt(std::max(0.0, 1.0 - y * y)), ph = golden * k;
    const double n[3] = {rr * std::cos(ph), y, rr * std::sin(ph)};
    double p[3] = {n[0], 1.2 + n[1], n[2]};
    const double seg = len / (npoints - 1);
    for (int j = 0; j < npoints; ++j) {
      for (int c = 0; c < 3; ++c) pts[3 * j + c] = fmt6(p[c]);
      const double t = (double)(j + 1) / (npoints - 1);
      const double curl = 0.15 * std::sin(3.0 * t + 0.7 * k);
      double d[3] = {n[0] * (1.0 - t) + curl * n[2], n[1] * (1.0 - t) - 0.9 * t, n[2] * (1.0 - t) - curl * n[0]};
      const double dl = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
      for (int c = 0; c < 3; ++c) p[c] += seg * d[c] / (dl > 0 ? dl : 1.0);
    }
    s.meshes.push_back(curve_mesh(pts.data(), npoints, (k & 1) ? hair_b : hair_a, 0.012f, 0.004f,
                                  (k & 1) ? 0.3f : -0.3f));
  }
}

}  // namespace yk
