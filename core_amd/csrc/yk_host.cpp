// Host half of the C-ABI (include/yk_api.h): scene assembly, kd-tree build,
// fixture generation, error reporting. No GPU needed; exercised by the CPU
// tests and by the oracle harness.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <new>
#include <stdexcept>
#include <string>

#include "../../include/yk_api.h"
#include "scene.h"
#include "yk_internal.h"

struct yk_scene {
  yk::Scene s;
};

namespace yk {
thread_local std::string g_last_error;
int set_error(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}
}  // namespace yk

using yk::set_error;

#define YK_GUARD_BEGIN try {
#define YK_GUARD_END                                                   \
  }                                                                    \
  catch (const std::bad_alloc&) { return set_error(YK_ERR_ALLOC, "out of host memory"); } \
  catch (const std::invalid_argument& e) { return set_error(YK_ERR_ARG, e.what()); }      \
  catch (const std::exception& e) { return set_error(YK_ERR_INTERNAL, e.what()); }        \
  catch (...) { return set_error(YK_ERR_INTERNAL, "unknown C++ exception"); }

extern "C" {

const char* yk_last_error(void) { return yk::g_last_error.c_str(); }
const char* yk_version(void) { return "yk 0.1 (gfx950)"; }

int yk_scene_create(yk_scene** out) {
  if (!out) return set_error(YK_ERR_ARG, "yk_scene_create: out is NULL");
  YK_GUARD_BEGIN
  *out = new yk_scene();
  return YK_OK;
  YK_GUARD_END
}

void yk_scene_destroy(yk_scene* s) { delete s; }

namespace {
bool finite3(const float* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }
}  // namespace

int yk_scene_add_glass(yk_scene* s, const yk_material* m, const yk_glass_params* g, int32_t* id_out) {
  if (!s || !m) return set_error(YK_ERR_ARG, "yk_scene_add_glass: NULL argument");
  if (m->type != YK_MAT_GLASS) return set_error(YK_ERR_ARG, "yk_scene_add_glass: the material's type must be YK_MAT_GLASS");
  if (!finite3(m->mirror_color) || !std::isfinite(m->ior) || !std::isfinite(m->transmit_filter) ||
      (g && (!finite3(g->filter_color) || std::isnan(g->dispersion_power))))
    return set_error(YK_ERR_ARG, "yk_scene_add_glass: glass colours, transmit_filter, IOR and dispersion_power must be finite");
  if (g && g->dispersion_power > 0.0)
    return set_error(YK_ERR_UNSUPPORTED, "glass with dispersion_power > 0 (BSDF_DISPERSIVE) is not on the GPU path");
  YK_GUARD_BEGIN
  const int id = s->s.add_material(*m, g);
  if (id_out) *id_out = id;
  return YK_OK;
  YK_GUARD_END
}

int yk_scene_add_material(yk_scene* s, const yk_material* m, int32_t* id_out) {
  if (!s || !m) return set_error(YK_ERR_ARG, "yk_scene_add_material: NULL argument");
  if (m->type == YK_MAT_GLASS) return yk_scene_add_glass(s, m, nullptr, id_out);
  if (m->type != YK_MAT_SHINYDIFFUSE && m->type != YK_MAT_LIGHT && m->type != YK_MAT_GLOSSY &&
      m->type != YK_MAT_COATED_GLOSSY)
    return set_error(YK_ERR_UNSUPPORTED, "material type not supported by the GPU path");
  if (m->type == YK_MAT_COATED_GLOSSY) {
    if (!finite3(m->color) || !finite3(m->diffuse_color) || !finite3(m->mirror_color) ||
        !std::isfinite(m->glossy_reflect) || !std::isfinite(m->diffuse_reflect) || !std::isfinite(m->exponent) ||
        !std::isfinite(m->ior) || (m->anisotropic && !(std::isfinite(m->exp_u) && std::isfinite(m->exp_v))))
      return set_error(YK_ERR_ARG,
                       "yk_scene_add_material: coated glossy colours, reflect strengths, exponents and IOR must be finite");
    if (!m->as_diffuse)
      return set_error(YK_ERR_UNSUPPORTED, "coated glossy with as_diffuse = false (BSDF_GLOSSY) is not on the GPU path");
  }
  if (m->type == YK_MAT_GLOSSY) {
    if (!finite3(m->color) || !finite3(m->diffuse_color) || !std::isfinite(m->glossy_reflect) ||
        !std::isfinite(m->diffuse_reflect) || !std::isfinite(m->exponent) ||
        (m->anisotropic && !(std::isfinite(m->exp_u) && std::isfinite(m->exp_v))))
      return set_error(YK_ERR_ARG, "yk_scene_add_material: glossy colours, reflect strengths and exponents must be finite");
    if (!m->as_diffuse)
      return set_error(YK_ERR_UNSUPPORTED, "glossy with as_diffuse = false (BSDF_GLOSSY) is not on the GPU path");
  }
  if (m->diffuse_brdf != YK_BRDF_LAMBERT && m->diffuse_brdf != YK_BRDF_OREN_NAYAR)
    return set_error(YK_ERR_ARG, "yk_scene_add_material: diffuse_brdf must be YK_BRDF_LAMBERT or YK_BRDF_OREN_NAYAR");
  YK_GUARD_BEGIN
  const int id = s->s.add_material(*m);
  if (id_out) *id_out = id;
  return YK_OK;
  YK_GUARD_END
}

int yk_scene_add_glass_state(yk_scene* s, const yk_material_state* m, const yk_glass_state* g, int32_t* id_out) {
  if (!s || !m) return set_error(YK_ERR_ARG, "yk_scene_add_glass_state: NULL argument");
  if (m->type != YK_MAT_GLASS)
    return set_error(YK_ERR_ARG, "yk_scene_add_glass_state: the state's type must be YK_MAT_GLASS");
  if (!finite3(m->mirror_color) || !std::isfinite(m->ior) || (g && !finite3(g->filter_col)))
    return set_error(YK_ERR_ARG, "yk_scene_add_glass_state: glass colours and IOR must be finite");
  // BSDF_DISPERSIVE (dispersion_power > 0) and BSDF_VOLUMETRIC ("absorption": the beer volume handler)
  if (m->bsdf_flags & (0x8u | 0x100u))
    return set_error(YK_ERR_UNSUPPORTED, "glass with dispersion or absorption (BSDF_DISPERSIVE, BSDF_VOLUMETRIC) is not on the GPU path");
  // glass.cc:60-61. The device record keeps glass's members over shinydiffuse's, so no other flag may steer a kernel there.
  const bool fake = g && g->fake_shadow;
  if ((g && g->fake_shadow != 0 && g->fake_shadow != 1) || m->bsdf_flags != ((0x1u | 0x10u | 0x20u) | (fake ? 0x40u : 0u)))
    return set_error(YK_ERR_ARG,
                     "yk_scene_add_glass_state: a glass state's bsdf_flags must be BSDF_SPECULAR | BSDF_REFLECT | "
                     "BSDF_TRANSMIT, with BSDF_FILTER if and only if fake_shadow is 1");
  YK_GUARD_BEGIN
  const int id = s->s.add_material_state(*m, g);
  if (id_out) *id_out = id;
  return YK_OK;
  YK_GUARD_END
}

int yk_scene_get_glass_state(const yk_scene* s, int32_t i, yk_glass_state* out) {
  if (!s || !out || i < 0 || i >= (int32_t)s->s.material_states.size())
    return set_error(YK_ERR_ARG, "yk_scene_get_glass_state: bad arguments");
  if (s->s.material_states[i].type != YK_MAT_GLASS)
    return set_error(YK_ERR_STATE, "yk_scene_get_glass_state: material is not a glass");
  *out = s->s.glass_states[i];
  return YK_OK;
}

int yk_scene_add_material_state(yk_scene* s, const yk_material_state* m, int32_t* id_out) {
  if (!s || !m) return set_error(YK_ERR_ARG, "yk_scene_add_material_state: NULL argument");
  if (m->type == YK_MAT_GLASS) return yk_scene_add_glass_state(s, m, nullptr, id_out);
  if (m->type != YK_MAT_SHINYDIFFUSE && m->type != YK_MAT_LIGHT && m->type != YK_MAT_GLOSSY &&
      m->type != YK_MAT_COATED_GLOSSY)
    return set_error(YK_ERR_UNSUPPORTED, "material type not supported by the GPU path");
  if (m->type == YK_MAT_COATED_GLOSSY) {
    if (!finite3(m->gloss_color) || !finite3(m->diff_color) || !finite3(m->mirror_color) ||
        !std::isfinite(m->reflectivity) || !std::isfinite(m->m_diffuse) || !std::isfinite(m->exponent) ||
        !std::isfinite(m->ior) || (m->anisotropic && !(std::isfinite(m->exp_u) && std::isfinite(m->exp_v))))
      return set_error(
          YK_ERR_ARG,
          "yk_scene_add_material_state: coated glossy colours, reflect strengths, exponents and IOR must be finite");
    if (!m->as_diffuse)
      return set_error(YK_ERR_UNSUPPORTED, "coated glossy with as_diffuse = false (BSDF_GLOSSY) is not on the GPU path");
    // coatedglossy.cc:84-101 with as_diffuse. The device record keeps the material's members over
    // shinydiffuse's, so no other flag (BSDF_FILTER, BSDF_EMIT) may steer a kernel there.
    const uint32_t spec = 0x1u | 0x10u, diff = 0x4u | 0x10u;
    const bool wd = m->with_diffuse != 0;
    if (m->bsdf_flags != (spec | diff) || m->ncomp != (wd ? 3 : 2) || m->comp_flags[0] != spec ||
        m->comp_flags[1] != diff || m->comp_flags[2] != (wd ? diff : 0u))
      return set_error(YK_ERR_ARG,
                       "yk_scene_add_material_state: a coated glossy state's bsdf_flags must be BSDF_SPECULAR | "
                       "BSDF_REFLECT | BSDF_DIFFUSE, with nBSDF and cFlags as its constructor sets them");
  }
  if (m->type == YK_MAT_GLOSSY) {
    if (!finite3(m->gloss_color) || !finite3(m->diff_color) || !std::isfinite(m->reflectivity) ||
        !std::isfinite(m->m_diffuse) || !std::isfinite(m->exponent) ||
        (m->anisotropic && !(std::isfinite(m->exp_u) && std::isfinite(m->exp_v))))
      return set_error(YK_ERR_ARG,
                       "yk_scene_add_material_state: glossy colours, reflect strengths and exponents must be finite");
    if (!m->as_diffuse)
      return set_error(YK_ERR_UNSUPPORTED, "glossy with as_diffuse = false (BSDF_GLOSSY) is not on the GPU path");
    // glossy.cc:69-79 with as_diffuse: BSDF_DIFFUSE | BSDF_REFLECT and nothing else. The device
    // record keeps glossy's members over shinydiffuse's, so no other flag may steer a kernel there.
    if (m->bsdf_flags != (0x4u | 0x10u))
      return set_error(YK_ERR_ARG,
                       "yk_scene_add_material_state: a glossy state's bsdf_flags must be BSDF_DIFFUSE | BSDF_REFLECT");
  }
  if (m->oren_nayar != 0 && m->oren_nayar != 1)
    return set_error(YK_ERR_ARG, "yk_scene_add_material_state: oren_nayar must be 0 or 1");
  YK_GUARD_BEGIN
  const int id = s->s.add_material_state(*m);
  if (id_out) *id_out = id;
  return YK_OK;
  YK_GUARD_END
}

int yk_scene_add_mesh(yk_scene* s, const float* points, int32_t npoints, const int32_t* faces,
                      int32_t nfaces, int32_t material, int32_t* obj_id_out) {
  if (!s || (npoints > 0 && !points) || (nfaces > 0 && !faces) || npoints < 0 || nfaces < 0)
    return set_error(YK_ERR_ARG, "yk_scene_add_mesh: bad arguments");
  if (material < 0 || material >= (int32_t)s->s.material_states.size())
    return set_error(YK_ERR_ARG, "yk_scene_add_mesh: unknown material id");
  for (int64_t i = 0; i < 3 * (int64_t)nfaces; ++i)
    if (faces[i] < 0 || faces[i] >= npoints)
      return set_error(YK_ERR_ARG, "yk_scene_add_mesh: face index out of range");
  YK_GUARD_BEGIN
  yk::Mesh m;
  m.points.assign(points, points + 3 * (size_t)npoints);
  m.faces.assign(faces, faces + 3 * (size_t)nfaces);
  m.material = material;
  s->s.meshes.push_back(std::move(m));
  s->s.built = false;
  if (obj_id_out) *obj_id_out = (int32_t)s->s.meshes.size();
  return YK_OK;
  YK_GUARD_END
}

int yk_scene_set_mesh_normals(yk_scene* s, int32_t obj_id, const float* normals, int32_t nnormals,
                              const int32_t* face_normals, int32_t flags) {
  if (!s || obj_id < 1 || obj_id > (int32_t)s->s.meshes.size() || nnormals < 0 || (nnormals > 0 && !normals))
    return set_error(YK_ERR_ARG, "yk_scene_set_mesh_normals: bad arguments");
  if (flags & ~(YK_MESH_SMOOTH | YK_MESH_NORMALS_EXPORTED))
    return set_error(YK_ERR_ARG, "yk_scene_set_mesh_normals: unknown flags");
  yk::Mesh& m = s->s.meshes[obj_id - 1];
  if (m.instance_of >= 0) return set_error(YK_ERR_ARG, "yk_scene_set_mesh_normals: object is an instance");
  const size_t nf = m.faces.size() / 3;
  if (face_normals)
    for (size_t i = 0; i < 3 * nf; ++i)
      if (face_normals[i] < -1 || face_normals[i] >= nnormals)
        return set_error(YK_ERR_ARG, "yk_scene_set_mesh_normals: normal index out of range");
  YK_GUARD_BEGIN
  m.normals.assign(normals, normals + 3 * (size_t)nnormals);
  if (face_normals) m.face_normals.assign(face_normals, face_normals + 3 * nf);
  else m.face_normals.clear();
  m.is_smooth = (flags & YK_MESH_SMOOTH) != 0;
  m.normals_exported = (flags & YK_MESH_NORMALS_EXPORTED) != 0;
  s->s.built = false;
  return YK_OK;
  YK_GUARD_END
}

int yk_scene_set_mode(yk_scene* s, int32_t mode) {
  if (!s || (mode != YK_MODE_TRIANGLE && mode != YK_MODE_UNIVERSAL))
    return set_error(YK_ERR_ARG, "yk_scene_set_mode: bad arguments");
  s->s.mode = mode;
  s->s.built = false;
  return YK_OK;
}

int yk_scene_set_mesh_type(yk_scene* s, int32_t obj_id, int32_t type) {
  if (!s || obj_id < 1 || obj_id > (int32_t)s->s.meshes.size())
    return set_error(YK_ERR_ARG, "yk_scene_set_mesh_type: bad object id");
  if (type != YK_MESH_TRIM && type != YK_MESH_VTRIM)
    return set_error(YK_ERR_UNSUPPORTED, "yk_scene_set_mesh_type: only TRIM and VTRIM meshes (MTRIM bezier is not on the path)");
  yk::Mesh& m = s->s.meshes[obj_id - 1];
  if (m.instance_of >= 0) return set_error(YK_ERR_ARG, "yk_scene_set_mesh_type: object is an instance");
  m.type = type;
  s->s.built = false;
  return YK_OK;
}

int yk_scene_set_mesh_base(yk_scene* s, int32_t obj_id) {
  if (!s || obj_id < 1 || obj_id > (int32_t)s->s.meshes.size())
    return set_error(YK_ERR_ARG, "yk_scene_set_mesh_base: bad object id");
  yk::Mesh& m = s->s.meshes[obj_id - 1];
  if (m.instance_of >= 0) return set_error(YK_ERR_ARG, "yk_scene_set_mesh_base: object is an instance");
  m.is_base = true;
  s->s.built = false;
  return YK_OK;
}

int yk_scene_add_instance(yk_scene* s, int32_t base_obj_id, const float* obj_to_world, int32_t* obj_id_out) {
  if (!s || !obj_to_world || base_obj_id < 1 || base_obj_id > (int32_t)s->s.meshes.size())
    return set_error(YK_ERR_ARG, "yk_scene_add_instance: bad arguments");
  if (s->s.meshes[base_obj_id - 1].instance_of >= 0)
    return set_error(YK_ERR_ARG, "yk_scene_add_instance: base object is itself an instance");
  YK_GUARD_BEGIN
  yk::Mesh m;
  m.instance_of = base_obj_id - 1;
  std::memcpy(m.m, obj_to_world, sizeof m.m);
  s->s.meshes.push_back(std::move(m));
  s->s.built = false;
  if (obj_id_out) *obj_id_out = (int32_t)s->s.meshes.size();
  return YK_OK;
  YK_GUARD_END
}

int yk_scene_add_curve(yk_scene* s, const float* points, int32_t npoints, int32_t material, float strand_start,
                       float strand_end, float strand_shape, int32_t* obj_id_out) {
  if (!s || !points || npoints < 2) return set_error(YK_ERR_ARG, "yk_scene_add_curve: need >= 2 points");
  if (material < 0 || material >= (int32_t)s->s.material_states.size())
    return set_error(YK_ERR_ARG, "yk_scene_add_curve: unknown material id");
  YK_GUARD_BEGIN
  s->s.meshes.push_back(yk::curve_mesh(points, npoints, material, strand_start, strand_end, strand_shape));
  s->s.built = false;
  if (obj_id_out) *obj_id_out = (int32_t)s->s.meshes.size();
  return YK_OK;
  YK_GUARD_END
}

int yk_scene_add_light(yk_scene* s, const yk_light* l) {
  if (!s || !l) return set_error(YK_ERR_ARG, "yk_scene_add_light: NULL argument");
  if (l->type != YK_LIGHT_AREA && l->type != YK_LIGHT_POINT && l->type != YK_LIGHT_DIRECTIONAL &&
      l->type != YK_LIGHT_SPOT && l->type != YK_LIGHT_SPHERE && l->type != YK_LIGHT_SUN)
    return set_error(YK_ERR_UNSUPPORTED, "light type not supported");
  if (l->type == YK_LIGHT_SUN) {
    const float* d = l->direction;
    if (!std::isfinite(d[0]) || !std::isfinite(d[1]) || !std::isfinite(d[2]) ||
        (d[0] == 0.f && d[1] == 0.f && d[2] == 0.f))
      return set_error(YK_ERR_ARG, "sun light needs a finite, non-zero direction");
    if (!std::isfinite(l->color[0]) || !std::isfinite(l->color[1]) || !std::isfinite(l->color[2]) ||
        !std::isfinite(l->power))
      return set_error(YK_ERR_ARG, "sun light needs a finite colour and power");
    // angle 0: cosAngle == 1, invpdf == 0 and an infinite pdf (sunlight.cc:59-61)
    if (!std::isfinite(l->cone_angle) || !(l->cone_angle > 0.f))
      return set_error(YK_ERR_ARG, "sun light needs a finite angle > 0 (cone_angle carries it)");
    if (l->samples < 1) return set_error(YK_ERR_ARG, "sun light needs samples >= 1");
  }
  if (l->type == YK_LIGHT_AREA && l->samples < 1) return set_error(YK_ERR_ARG, "area light needs samples >= 1");
  if (l->type == YK_LIGHT_SPOT) {
    if (l->soft_shadows && l->samples < 1) return set_error(YK_ERR_ARG, "soft-shadow spot light needs samples >= 1");
    if (l->from[0] == l->to[0] && l->from[1] == l->to[1] && l->from[2] == l->to[2])
      return set_error(YK_ERR_ARG, "spot light needs from != to");
    if (!(l->cone_angle > 0.f && l->cone_angle <= 180.f))
      return set_error(YK_ERR_ARG, "spot light needs cone_angle in (0, 180]");
  }
  if (l->type == YK_LIGHT_SPHERE) {
    if (l->samples < 1) return set_error(YK_ERR_ARG, "sphere light needs samples >= 1");
    if (!(l->radius > 0.f)) return set_error(YK_ERR_ARG, "sphere light needs radius > 0");
  }
  YK_GUARD_BEGIN
  s->s.add_light(*l);
  return YK_OK;
  YK_GUARD_END
}

// what scene_t::getMesh hands meshLight_t::init as a triangleObject_t
// (scene.cc:709-713): a TRIM mesh, not an instance
static int mesh_light_target(const yk::Scene& S, int32_t id, const char* who) {
  if (id < 1 || id > (int32_t)S.meshes.size())
    return set_error(YK_ERR_ARG, std::string(who) + ": unknown object id " + std::to_string(id));
  const yk::Mesh& m = S.meshes[(size_t)id - 1];
  if (m.instance_of >= 0)
    return set_error(YK_ERR_UNSUPPORTED, std::string(who) + ": object " + std::to_string(id) + " is an instance");
  if (m.type != YK_MESH_TRIM)
    return set_error(YK_ERR_UNSUPPORTED, std::string(who) + ": object " + std::to_string(id) + " is a VTRIM mesh");
  return YK_OK;
}

int yk_scene_add_mesh_light(yk_scene* s, const yk_mesh_light* l, const int32_t* obj_ids, int32_t nobj) {
  if (!s || !l) return set_error(YK_ERR_ARG, "yk_scene_add_mesh_light: NULL argument");
  if (nobj < 1 || !obj_ids) return set_error(YK_ERR_ARG, "yk_scene_add_mesh_light: empty object list");
  if (l->samples < 1) return set_error(YK_ERR_ARG, "mesh light needs samples >= 1");
  if (!std::isfinite(l->color[0]) || !std::isfinite(l->color[1]) || !std::isfinite(l->color[2]) ||
      !std::isfinite(l->power))
    return set_error(YK_ERR_ARG, "mesh light needs a finite colour and power");
  int64_t ntris = 0;
  for (int32_t i = 0; i < nobj; ++i) {
    if (const int rc = mesh_light_target(s->s, obj_ids[i], "yk_scene_add_mesh_light")) return rc;
    for (int32_t j = 0; j < i; ++j)
      if (obj_ids[j] == obj_ids[i])
        return set_error(YK_ERR_ARG, "yk_scene_add_mesh_light: object id " + std::to_string(obj_ids[i]) + " repeated");
    ntris += (int64_t)(s->s.meshes[(size_t)obj_ids[i] - 1].faces.size() / 3);
  }
  if (ntris > YK_MESH_LIGHT_MAX_TRIS)
    return set_error(YK_ERR_UNSUPPORTED, "mesh light has more than YK_MESH_LIGHT_MAX_TRIS triangles");
  YK_GUARD_BEGIN
  s->s.add_mesh_light(*l, obj_ids, nobj);
  return YK_OK;
  YK_GUARD_END
}

int yk_scene_get_mesh_light(const yk_scene* s, int32_t i, yk_mesh_light* out, int32_t* obj_ids, int32_t cap,
                            int32_t* nobj_out) {
  if (!s || i < 0 || i >= (int32_t)s->s.mesh_lights.size() || cap < 0 || (cap > 0 && !obj_ids))
    return set_error(YK_ERR_ARG, "yk_scene_get_mesh_light: bad arguments");
  if (s->s.light_kind[i] != YK_LIGHT_MESH) return set_error(YK_ERR_STATE, "light is not a mesh light");
  const yk::MeshLight& L = s->s.mesh_lights[i];
  if (out) *out = L.params;
  for (int32_t k = 0; k < cap && k < (int32_t)L.obj_ids.size(); ++k) obj_ids[k] = L.obj_ids[k];
  if (nobj_out) *nobj_out = (int32_t)L.obj_ids.size();
  return YK_OK;
}

int yk_scene_get_mesh_light_state(const yk_scene* s, int32_t i, yk_mesh_light_state* out, float* cdf,
                                  float* tri_areas, int32_t cap_tris) {
  if (!s || !out || i < 0 || i >= (int32_t)s->s.mesh_lights.size() || cap_tris < 0)
    return set_error(YK_ERR_ARG, "yk_scene_get_mesh_light_state: bad arguments");
  if (s->s.light_kind[i] != YK_LIGHT_MESH) return set_error(YK_ERR_STATE, "light is not a mesh light");
  if (!s->s.built) return set_error(YK_ERR_STATE, "yk_scene_get_mesh_light_state: scene not built");
  const yk::MeshLight& L = s->s.mesh_lights[i];
  std::memset(out, 0, sizeof *out);
  for (int k = 0; k < 3; ++k) out->color[k] = L.color[k];
  out->samples = L.params.samples;
  out->double_sided = L.params.double_sided;
  out->area = L.area;
  out->inv_area = L.inv_area;
  out->ntris = (int32_t)L.areas.size();
  out->tree_depth = L.tree.max_depth;
  out->tree_nodes = (int32_t)(L.tree.nodes.size() / 2);
  const int32_t n = std::min(cap_tris, out->ntris);
  if (cdf && n > 0) std::memcpy(cdf, L.cdf.data(), ((size_t)n + 1) * sizeof(float));
  if (tri_areas && n > 0) std::memcpy(tri_areas, L.areas.data(), (size_t)n * sizeof(float));
  return YK_OK;
}

int yk_scene_set_mesh_light_color(yk_scene* s, int32_t i, const float* rgb) {
  if (!s || !rgb || i < 0 || i >= (int32_t)s->s.mesh_lights.size())
    return set_error(YK_ERR_ARG, "yk_scene_set_mesh_light_color: bad arguments");
  if (s->s.light_kind[i] != YK_LIGHT_MESH) return set_error(YK_ERR_STATE, "light is not a mesh light");
  if (!std::isfinite(rgb[0]) || !std::isfinite(rgb[1]) || !std::isfinite(rgb[2]))
    return set_error(YK_ERR_ARG, "mesh light needs a finite colour");
  for (int k = 0; k < 3; ++k) s->s.mesh_lights[i].color[k] = rgb[k];
  return YK_OK;
}

int yk_scene_add_area_light_state(yk_scene* s, const yk_area_light_state* l) {
  if (!s || !l) return set_error(YK_ERR_ARG, "yk_scene_add_area_light_state: NULL argument");
  if (l->samples < 1) return set_error(YK_ERR_ARG, "area light needs samples >= 1");
  YK_GUARD_BEGIN
  s->s.add_light_state(*l);
  return YK_OK;
  YK_GUARD_END
}

int yk_scene_add_dirac_light_state(yk_scene* s, const yk_dirac_light_state* l) {
  if (!s || !l) return set_error(YK_ERR_ARG, "yk_scene_add_dirac_light_state: NULL argument");
  if (l->type != YK_LIGHT_POINT && l->type != YK_LIGHT_DIRECTIONAL)
    return set_error(YK_ERR_ARG, "yk_scene_add_dirac_light_state: type must be point or directional");
  YK_GUARD_BEGIN
  s->s.add_dirac_light_state(*l);
  return YK_OK;
  YK_GUARD_END
}

int yk_scene_get_dirac_light_state(const yk_scene* s, int32_t i, yk_dirac_light_state* out) {
  if (!s || !out || i < 0 || i >= (int32_t)s->s.dirac_states.size())
    return set_error(YK_ERR_ARG, "yk_scene_get_dirac_light_state: bad arguments");
  if (s->s.light_kind[i] != YK_LIGHT_POINT && s->s.light_kind[i] != YK_LIGHT_DIRECTIONAL)
    return set_error(YK_ERR_STATE, "light is not a point or directional light");
  *out = s->s.dirac_states[i];
  return YK_OK;
}

int yk_scene_add_spot_light_state(yk_scene* s, const yk_spot_light_state* l) {
  if (!s || !l) return set_error(YK_ERR_ARG, "yk_scene_add_spot_light_state: NULL argument");
  if (l->soft_shadows && l->samples < 1) return set_error(YK_ERR_ARG, "soft-shadow spot light needs samples >= 1");
  YK_GUARD_BEGIN
  yk_spot_light_state c = *l;
  c.soft_shadows = c.soft_shadows ? 1 : 0;
  c.photon_only = c.photon_only ? 1 : 0;
  s->s.add_spot_light_state(c);
  return YK_OK;
  YK_GUARD_END
}

int yk_scene_get_spot_light_state(const yk_scene* s, int32_t i, yk_spot_light_state* out) {
  if (!s || !out || i < 0 || i >= (int32_t)s->s.spot_states.size())
    return set_error(YK_ERR_ARG, "yk_scene_get_spot_light_state: bad arguments");
  if (s->s.light_kind[i] != YK_LIGHT_SPOT) return set_error(YK_ERR_STATE, "light is not a spot light");
  *out = s->s.spot_states[i];
  return YK_OK;
}

int yk_scene_add_sphere_light_state(yk_scene* s, const yk_sphere_light_state* l) {
  if (!s || !l) return set_error(YK_ERR_ARG, "yk_scene_add_sphere_light_state: NULL argument");
  if (l->samples < 1) return set_error(YK_ERR_ARG, "sphere light needs samples >= 1");
  if (!(l->radius > 0.f)) return set_error(YK_ERR_ARG, "sphere light needs radius > 0");
  YK_GUARD_BEGIN
  s->s.add_sphere_light_state(*l);
  return YK_OK;
  YK_GUARD_END
}

int yk_scene_get_sphere_light_state(const yk_scene* s, int32_t i, yk_sphere_light_state* out) {
  if (!s || !out || i < 0 || i >= (int32_t)s->s.sphere_states.size())
    return set_error(YK_ERR_ARG, "yk_scene_get_sphere_light_state: bad arguments");
  if (s->s.light_kind[i] != YK_LIGHT_SPHERE) return set_error(YK_ERR_STATE, "light is not a sphere light");
  *out = s->s.sphere_states[i];
  return YK_OK;
}

int yk_scene_add_sun_light_state(yk_scene* s, const yk_sun_light_state* l) {
  if (!s || !l) return set_error(YK_ERR_ARG, "yk_scene_add_sun_light_state: NULL argument");
  if (l->samples < 1) return set_error(YK_ERR_ARG, "sun light needs samples >= 1");
  YK_GUARD_BEGIN
  s->s.add_sun_light_state(*l);
  return YK_OK;
  YK_GUARD_END
}

int yk_scene_get_sun_light_state(const yk_scene* s, int32_t i, yk_sun_light_state* out) {
  if (!s || !out || i < 0 || i >= (int32_t)s->s.sun_states.size())
    return set_error(YK_ERR_ARG, "yk_scene_get_sun_light_state: bad arguments");
  if (s->s.light_kind[i] != YK_LIGHT_SUN) return set_error(YK_ERR_STATE, "light is not a sun light");
  *out = s->s.sun_states[i];
  return YK_OK;
}

int yk_scene_set_background(yk_scene* s, const float* rgb, float power) {
  if (!s) return set_error(YK_ERR_ARG, "yk_scene_set_background: NULL scene");
  s->s.has_background = rgb != nullptr;
  for (int k = 0; k < 3; ++k) s->s.background[k] = rgb ? rgb[k] * power : 0.f;  // col*power, textureback.cc:218
  if (rgb) s->s.set_gradient_background(nullptr);  // one background per scene
  if (s->s.has_bg_light()) s->s.built = false;     // the light's tables come from the background
  return YK_OK;
}

int yk_scene_get_background(const yk_scene* s, float* rgb_out, int32_t* has_out) {
  if (!s) return set_error(YK_ERR_ARG, "yk_scene_get_background: NULL scene");
  if (s->s.has_gradient) return set_error(YK_ERR_STATE, "the scene's background is a gradient");
  if (rgb_out)
    for (int k = 0; k < 3; ++k) rgb_out[k] = s->s.background[k];
  if (has_out) *has_out = s->s.has_background ? 1 : 0;
  return YK_OK;
}

int yk_scene_set_gradient_background(yk_scene* s, const yk_gradient_background* g) {
  if (!s) return set_error(YK_ERR_ARG, "yk_scene_set_gradient_background: NULL scene");
  if (g) {
    bool finite = std::isfinite(g->power);
    for (int k = 0; k < 3; ++k)
      finite = finite && std::isfinite(g->horizon_color[k]) && std::isfinite(g->zenith_color[k]) &&
               std::isfinite(g->horizon_ground_color[k]) && std::isfinite(g->zenith_ground_color[k]);
    if (!finite) return set_error(YK_ERR_ARG, "gradient background needs finite colours and power");
  }
  s->s.set_gradient_background(g);
  if (s->s.has_bg_light()) s->s.built = false;
  return YK_OK;
}

int yk_scene_get_gradient_background(const yk_scene* s, yk_gradient_background* out, int32_t* has_out) {
  if (!s) return set_error(YK_ERR_ARG, "yk_scene_get_gradient_background: NULL scene");
  if (out && s->s.has_gradient) *out = s->s.gradient_params;
  if (has_out) *has_out = s->s.has_gradient ? 1 : 0;
  return YK_OK;
}

int yk_scene_add_background_light(yk_scene* s, const yk_background_light* l) {
  if (!s || !l) return set_error(YK_ERR_ARG, "yk_scene_add_background_light: NULL argument");
  if (l->samples < 1) return set_error(YK_ERR_ARG, "background light needs samples >= 1");
  YK_GUARD_BEGIN
  s->s.add_background_light(*l);
  return YK_OK;
  YK_GUARD_END
}

int yk_scene_get_background_light(const yk_scene* s, int32_t i, yk_background_light* out) {
  if (!s || !out || i < 0 || i >= (int32_t)s->s.bg_lights.size())
    return set_error(YK_ERR_ARG, "yk_scene_get_background_light: bad arguments");
  if (s->s.light_kind[i] != YK_LIGHT_BACKGROUND) return set_error(YK_ERR_STATE, "light is not a background light");
  *out = s->s.bg_lights[i].params;
  return YK_OK;
}

int yk_scene_export_background_light(const yk_scene* s, int32_t i, int32_t* nrows_out, int32_t* total_u_out,
                                     int32_t* row_count, int32_t* row_offset, float* row_integral,
                                     float* row_inv_integral, float* func_u, float* cdf_u, float* func_v,
                                     float* cdf_v, float* v_integrals) {
  if (!s || i < 0 || i >= (int32_t)s->s.bg_lights.size())
    return set_error(YK_ERR_ARG, "yk_scene_export_background_light: bad arguments");
  if (s->s.light_kind[i] != YK_LIGHT_BACKGROUND) return set_error(YK_ERR_STATE, "light is not a background light");
  if (!s->s.built) return set_error(YK_ERR_STATE, "yk_scene_export_background_light: scene not built");
  const yk::BgLight& L = s->s.bg_lights[i];
  auto copy = [](auto* dst, const auto& v) {
    if (dst) std::memcpy(dst, v.data(), v.size() * sizeof v[0]);
  };
  if (nrows_out) *nrows_out = (int32_t)L.row_count.size();
  if (total_u_out) *total_u_out = (int32_t)L.func_u.size();
  copy(row_count, L.row_count);
  copy(row_offset, L.row_offset);
  copy(row_integral, L.row_integral);
  copy(row_inv_integral, L.row_inv_integral);
  copy(func_u, L.func_u);
  copy(cdf_u, L.cdf_u);
  copy(func_v, L.func_v);
  copy(cdf_v, L.cdf_v);
  if (v_integrals) {
    v_integrals[0] = L.v_integral;
    v_integrals[1] = L.v_inv_integral;
  }
  return YK_OK;
}

int yk_scene_set_camera(yk_scene* s, const yk_camera* c) {
  if (!s || !c) return set_error(YK_ERR_ARG, "yk_scene_set_camera: NULL argument");
  if (c->resx <= 0 || c->resy <= 0) return set_error(YK_ERR_ARG, "camera resolution must be > 0");
  if (c->type < YK_CAMERA_PERSPECTIVE || c->type > YK_CAMERA_ANGULAR)
    return set_error(YK_ERR_UNSUPPORTED, "unknown camera type");
  const bool lensless = c->type == YK_CAMERA_ORTHOGRAPHIC || c->type == YK_CAMERA_ANGULAR;
  if (c->type == YK_CAMERA_ORTHOGRAPHIC && !(std::isfinite(c->scale) && c->scale > 0.0))
    return set_error(YK_ERR_ARG, "orthographic camera: scale must be finite and > 0");
  if (c->type == YK_CAMERA_ANGULAR && !(std::isfinite(c->angle) && c->angle > 0.0))
    return set_error(YK_ERR_ARG, "angular camera: angle must be finite and > 0");
  if (c->type == YK_CAMERA_ANGULAR && !(std::isfinite(c->max_angle) && c->max_angle >= 0.0))
    return set_error(YK_ERR_ARG, "angular camera: max_angle must be finite and >= 0");
  // camera_t::sampleLense() is false for them: an aperture would be dropped
  if (lensless && c->aperture != 0.f)
    return set_error(YK_ERR_ARG, "orthographic and angular cameras have no lens: aperture must be 0");
  YK_GUARD_BEGIN
  s->s.set_camera(*c);
  return YK_OK;
  YK_GUARD_END
}

int yk_scene_set_camera_state(yk_scene* s, const yk_camera_state* c) {
  if (!s || !c) return set_error(YK_ERR_ARG, "yk_scene_set_camera_state: NULL argument");
  if (c->resx <= 0 || c->resy <= 0) return set_error(YK_ERR_ARG, "camera resolution must be > 0");
  if (c->kind < YK_CAMERA_PERSPECTIVE || c->kind > YK_CAMERA_ANGULAR)
    return set_error(YK_ERR_UNSUPPORTED, "unknown camera kind");
  if ((c->kind == YK_CAMERA_ORTHOGRAPHIC || c->kind == YK_CAMERA_ANGULAR) && c->aperture != 0.f)
    return set_error(YK_ERR_ARG, "orthographic and angular cameras have no lens: aperture must be 0");
  yk_camera_state k = *c;
  // an architect camera's shootRay is perspectiveCam_t's: one kind
  if (k.kind == YK_CAMERA_ARCHITECT) k.kind = YK_CAMERA_PERSPECTIVE;
  k.circular = k.circular ? 1 : 0;
  s->s.set_camera_state(k);
  return YK_OK;
}

int yk_scene_get_material_state(const yk_scene* s, int32_t i, yk_material_state* out) {
  if (!s || !out || i < 0 || i >= (int32_t)s->s.material_states.size())
    return set_error(YK_ERR_ARG, "yk_scene_get_material_state: bad arguments");
  *out = s->s.material_states[i];
  return YK_OK;
}

int yk_scene_get_area_light_state(const yk_scene* s, int32_t i, yk_area_light_state* out) {
  if (!s || !out || i < 0 || i >= (int32_t)s->s.light_states.size())
    return set_error(YK_ERR_ARG, "yk_scene_get_area_light_state: bad arguments");
  if (s->s.light_kind[i] != YK_LIGHT_AREA) return set_error(YK_ERR_STATE, "light is not an area light");
  *out = s->s.light_states[i];
  return YK_OK;
}

int yk_scene_get_camera_state(const yk_scene* s, yk_camera_state* out) {
  if (!s || !out) return set_error(YK_ERR_ARG, "yk_scene_get_camera_state: NULL argument");
  if (!s->s.has_camera) return set_error(YK_ERR_STATE, "scene has no camera");
  *out = s->s.camera_state;
  return YK_OK;
}

int yk_scene_build(yk_scene* s) {
  if (!s) return set_error(YK_ERR_ARG, "yk_scene_build: NULL scene");
  if (s->s.mode == YK_MODE_UNIVERSAL)
    for (const yk::Mesh& m : s->s.meshes)
      if (m.instance_of >= 0)  // scene_t::addInstance refuses outside triangle mode (scene.cc:985)
        return set_error(YK_ERR_UNSUPPORTED, "yk_scene_build: universal mode has no instances");
  for (const yk::MeshLight& L : s->s.mesh_lights) {  // a target retyped after yk_scene_add_mesh_light
    int64_t ntris = 0;
    for (const int32_t id : L.obj_ids) {
      if (const int rc = mesh_light_target(s->s, id, "yk_scene_build: mesh light")) return rc;
      ntris += (int64_t)(s->s.meshes[(size_t)id - 1].faces.size() / 3);
    }
    if (ntris > YK_MESH_LIGHT_MAX_TRIS)
      return set_error(YK_ERR_UNSUPPORTED, "mesh light has more than YK_MESH_LIGHT_MAX_TRIS triangles");
  }
  if (s->s.has_bg_light() && s->s.background_kind() == yk::YK_BG_NONE)
    return set_error(YK_ERR_STATE, "yk_scene_build: a background light needs a background");
  YK_GUARD_BEGIN
  s->s.finalize();
  return YK_OK;
  YK_GUARD_END
}

int yk_scene_info_get(const yk_scene* s, yk_scene_info* o) {
  if (!s || !o) return set_error(YK_ERR_ARG, "yk_scene_info_get: NULL argument");
  std::memset(o, 0, sizeof *o);
  const yk::Scene& S = s->s;
  o->ntris = (int32_t)S.tri_material.size();
  o->nmeshes = (int32_t)S.meshes.size();
  o->nmaterials = (int32_t)S.materials.size();
  o->nlights = (int32_t)S.lights.size();
  if (S.built) {
    o->nnodes = (int32_t)(S.tree.nodes.size() / 2);
    o->nleaf_prims = (int32_t)S.tree.leaf_prims.size();
    o->max_depth = S.tree.max_depth;
    o->inodes = S.tree.stats.inodes;
    o->leaves = S.tree.stats.leaves;
    o->empty_leaves = S.tree.stats.empty_leaves;
    o->leaf_refs = S.tree.stats.leaf_prims;
    o->depth_limit_leaves = S.tree.stats.depth_limit_reached;
    o->bad_split_leaves = S.tree.stats.bad_splits;
    std::memcpy(o->bound, S.tree.bound, sizeof o->bound);
    o->build_seconds = S.build_seconds;
  }
  o->mode = S.mode;
  return YK_OK;
}

int yk_scene_export(const yk_scene* s, float* tri_verts, int32_t* tri_material, float* tri_normal,
                    uint32_t* nodes, uint32_t* leaf_prims) {
  if (!s) return set_error(YK_ERR_ARG, "yk_scene_export: NULL scene");
  const yk::Scene& S = s->s;
  if (!S.built) return set_error(YK_ERR_STATE, "yk_scene_export: scene not built");
  if (tri_verts) std::memcpy(tri_verts, S.tri_verts.data(), S.tri_verts.size() * sizeof(float));
  if (tri_material) std::memcpy(tri_material, S.tri_material.data(), S.tri_material.size() * sizeof(int32_t));
  if (tri_normal) std::memcpy(tri_normal, S.tri_normal.data(), S.tri_normal.size() * sizeof(float));
  if (nodes) std::memcpy(nodes, S.tree.nodes.data(), S.tree.nodes.size() * sizeof(uint32_t));
  if (leaf_prims) std::memcpy(leaf_prims, S.tree.leaf_prims.data(), S.tree.leaf_prims.size() * sizeof(uint32_t));
  return YK_OK;
}

int yk_scene_export_shading(const yk_scene* s, uint8_t* smooth, float* vertex_normals) {
  if (!s) return set_error(YK_ERR_ARG, "yk_scene_export_shading: NULL scene");
  const yk::Scene& S = s->s;
  if (!S.built) return set_error(YK_ERR_STATE, "yk_scene_export_shading: scene not built");
  if (smooth) std::memcpy(smooth, S.tri_smooth.data(), S.tri_smooth.size());
  if (vertex_normals) std::memcpy(vertex_normals, S.tri_vnormal.data(), S.tri_vnormal.size() * sizeof(float));
  return YK_OK;
}

int yk_scene_get_material(const yk_scene* s, int32_t i, yk_material* out) {
  if (!s || !out || i < 0 || i >= (int32_t)s->s.materials.size())
    return set_error(YK_ERR_ARG, "yk_scene_get_material: bad index");
  if (!s->s.material_has_params[i]) return set_error(YK_ERR_STATE, "material was given as object state only");
  *out = s->s.materials[i];
  return YK_OK;
}

int yk_scene_get_light(const yk_scene* s, int32_t i, yk_light* out) {
  if (!s || !out || i < 0 || i >= (int32_t)s->s.lights.size())
    return set_error(YK_ERR_ARG, "yk_scene_get_light: bad index");
  if (!s->s.light_has_params[i]) return set_error(YK_ERR_STATE, "light was given as object state only");
  *out = s->s.lights[i];
  return YK_OK;
}

int yk_scene_get_camera(const yk_scene* s, yk_camera* out) {
  if (!s || !out) return set_error(YK_ERR_ARG, "yk_scene_get_camera: NULL argument");
  if (!s->s.has_camera || !s->s.camera_has_params)
    return set_error(YK_ERR_STATE, "scene has no parameter-level camera");
  *out = s->s.camera;
  return YK_OK;
}

int yk_tile_order_random(int32_t ntiles, uint32_t seed, int32_t* order_out) {
  if (ntiles < 0 || (ntiles > 0 && !order_out)) return set_error(YK_ERR_ARG, "yk_tile_order_random: bad arguments");
  // glibc's rand() is random() on the default TYPE_3 generator (a 128-byte
  // state); the reentrant random_r on a private state of that size, seeded
  // like srand(seed), gives the same sequence
  char state[128];
  random_data rd{};
  if (initstate_r(seed, state, sizeof state, &rd) != 0) return set_error(YK_ERR_INTERNAL, "initstate_r failed");
  for (int32_t i = 0; i < ntiles; ++i) order_out[i] = i;
  // libstdc++ std::random_shuffle(first, last): for i in [first + 1, last):
  // j = first + rand() % ((i - first) + 1); swap(*i, *j) when i != j
  for (int32_t i = 1; i < ntiles; ++i) {
    int32_t r = 0;
    random_r(&rd, &r);
    const int32_t j = r % (i + 1);
    if (j != i) std::swap(order_out[i], order_out[j]);
  }
  return YK_OK;
}

void yk_render_params_default(yk_render_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  // defaults of pathIntegrator_t::factory (pathtracer.cc:337-343) and
  // renderEnvironment_t::createImageFilm/setupScene (environment.cc:484-490,598-654)
  p->integrator = YK_INTEGRATOR_PATH;
  p->raydepth = 5;
  p->path_samples = 32;
  p->bounces = 3;
  p->caustic_type = YK_CAUSTIC_PATH;
  p->width = 320;
  p->height = 240;
  p->aa_samples = 1;
  p->aa_passes = 1;
  p->filter = YK_FILTER_BOX;
  p->aa_pixelwidth = 1.5f;
  p->tile_size = 32;
  p->transp_background = 1;
  p->aa_inc_samples = 0;  // = aa_samples
  p->aa_threshold = 0.05f;
  p->transp_shadows = 0;  // "transpShad"
  p->shadow_depth = 5;    // "shadowDepth" (pathtracer.cc:338, photonintegr.cc:889)
  // photonIntegrator_t::factory (photonintegr.cc:884-960)
  yk_photon_params& q = p->photon;
  q.photons = 100000;
  q.caustic_photons = 500000;
  q.diffuse_radius = 0.1f;
  q.caustic_radius = 0.01f;
  q.search = 50;
  q.caustic_mix = 50;
  q.bounces = 5;
  q.final_gather = 1;
  q.fg_samples = 32;
  q.fg_bounces = 2;
  q.fg_min_pathlen = 0.1f;  // = diffuseRadius
  q.show_map = 0;
  q.seed = 123212;          // myseed, vector3d.cc:185
  // directLighting_t::factory (directlight.cc:184-252)
  p->do_ao = 0;
  p->ao_samples = 32;
  p->ao_distance = 1.0f;
  p->ao_color[0] = p->ao_color[1] = p->ao_color[2] = 1.f;
  p->dl_caustics = 0;
}

int yk_scene_generate(yk_scene* s, const char* name, int32_t p0, int32_t p1, int32_t resx,
                      int32_t resy, yk_render_params* params_out) {
  if (!s || !name) return set_error(YK_ERR_ARG, "yk_scene_generate: NULL argument");
  if (resx <= 0 || resy <= 0) return set_error(YK_ERR_ARG, "yk_scene_generate: bad resolution");
  YK_GUARD_BEGIN
  yk_render_params p;
  yk_render_params_default(&p);
  p.width = resx;
  p.height = resy;
  p.aa_pixelwidth = 1.0f;
  p.filter = YK_FILTER_BOX;
  p.tile_size = 32;
  p.aa_passes = 1;
  p.raydepth = 2;
  p.caustic_type = YK_CAUSTIC_NONE;
  p.path_samples = 1;
  std::string n(name);
  if (n == "cornell_dl" || n == "cornell_pt") {
    yk::gen_cornell(s->s, resx, resy);
    if (n == "cornell_dl") {
      p.integrator = YK_INTEGRATOR_DIRECT;
      p.aa_samples = 4;
    } else {
      p.integrator = YK_INTEGRATOR_PATH;
      p.bounces = 4;
      p.aa_samples = 16;
    }
  } else if (n == "bumpy") {
    const int nu = p0 > 0 ? p0 : 1000, nv = p1 > 0 ? p1 : 501;
    if (nu < 3 || nv < 3) return set_error(YK_ERR_ARG, "bumpy: nu, nv must be >= 3");
    yk::gen_bumpy(s->s, nu, nv, resx, resy);
    p.integrator = YK_INTEGRATOR_PATH;
    p.bounces = 3;
    p.aa_samples = 4;
  } else if (n == "hair") {
    const int ns = p0 > 0 ? p0 : 200000, np = p1 > 0 ? p1 : 9;
    if (np < 2) return set_error(YK_ERR_ARG, "hair: strands need >= 2 points");
    yk::gen_hair(s->s, ns, np, resx, resy);
    p.integrator = YK_INTEGRATOR_PATH;
    p.bounces = 8;
    p.aa_samples = 4;
  } else {
    return set_error(YK_ERR_ARG, "unknown procedural scene '" + n + "'");
  }
  if (params_out) *params_out = p;
  return YK_OK;
  YK_GUARD_END
}

}  // extern "C"
