// Host-side scene container: the subset of scene_t state the hot path reads
// (include/core_api/scene.h:158-250, src/yafraycore/scene.cc). Geometry is kept
// as a triangle soup in scene_t::update prim order (scene.cc:760-781): meshes
// in ascending object id, triangles in insertion order.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/yk_api.h"
#include "kdtree_build.h"

namespace yk {

// FAST_TRIG fSin / fCos (mathOptimizations.h:249-280) in the compiled form of
// yk_math.h's fsin_ref, host IEEE arithmetic (camera polygon table, film
// filter tables)
float host_fsin(float x);
inline float host_fcos(float x) { return host_fsin(x + (float)1.57079632679489661923); }

struct Mesh {
  std::vector<float> points;  // xyz per vertex (point3d_t, float)
  std::vector<int> faces;     // a,b,c per triangle
  int material = -1;
  bool visible = true;
  bool is_base = false;       // instancing base: not traced itself
  int type = YK_MESH_TRIM;    // startTriMesh type: TRIM (triangle_t) or VTRIM (vTriangle_t)
  // vertex normals (triangleObject_t::normals) and per-face indices (na,nb,nc)
  std::vector<float> normals;
  std::vector<int> face_normals;  // 3 per face, -1 = none (empty: all -1)
  bool is_smooth = false, normals_exported = false;
  // triangleObjectInstance_t: base mesh index and objToWorld (row-major)
  int instance_of = -1;
  float m[16] = {};
};

// meshLight_t: parameters, the yk meshes whose triangles it holds, and after
// finalize() the members initIS computes (meshlight.cc:47-65)
struct MeshLight {
  yk_mesh_light params{};
  float color[3] = {0.f, 0.f, 0.f};  // color * (float)power * M_PI
  std::vector<int32_t> obj_ids;      // 1-based, light order
  std::vector<float> verts;          // 9 floats per triangle, getPrimitives order
  std::vector<float> normals;        // triangle_t::normal, 3 per triangle
  std::vector<float> areas;          // triangle_t::surfaceArea
  std::vector<float> cdf;            // pdf1D_t::cdf, n + 1
  float area = 0.f, inv_area = 0.f;
  KdTree tree;
};

// bgLight_t: parameters, and after finalize() the tables init() computes
// (bglight.cc:68-118): one pdf1D_t per row (uDist[y]) and one over the rows'
// integrals (vDist); a cdf holds count + 1 entries
struct BgLight {
  yk_background_light params{};
  bool present = false;              // the entry is a background light (the others' entries stay empty)
  std::vector<int32_t> row_count, row_offset;  // per row: count, first element in func_u
  std::vector<float> row_integral, row_inv_integral;
  std::vector<float> func_u, cdf_u;  // rows back to back: sum(count), sum(count) + nrows
  std::vector<float> func_v, cdf_v;  // nrows, nrows + 1
  float v_integral = 0.f, v_inv_integral = 0.f;
};

enum { YK_BG_NONE = 0, YK_BG_CONSTANT = 1, YK_BG_GRADIENT = 2 };  // Scene::background_kind()
// background_t::eval of a scene's background (constBackground_t: the colour;
// gradientBackground_t::eval, gradientback.cc:60-79); grad = szenith, shoriz, gzenith, ghoriz
void background_eval(int kind, const float* constant, const float* grad, const float* dir, float* rgb);

struct Scene {
  std::vector<Mesh> meshes;          // object-id order
  int mode = YK_MODE_TRIANGLE;       // scene_t::mode: which meshes the tree holds
  // parameter-level descriptions (when the caller gave them) ...
  std::vector<yk_material> materials;
  std::vector<bool> material_has_params;
  std::vector<yk_light> lights;
  std::vector<bool> light_has_params;
  yk_camera camera{};
  bool camera_has_params = false;
  // ... and the reference object state the kernels consume
  std::vector<yk_material_state> material_states;
  std::vector<yk_glass_state> glass_states;         // glass materials (zero entry for every other kind)
  std::vector<int> light_kind;                      // YK_LIGHT_*, scene light order
  std::vector<yk_area_light_state> light_states;    // area lights (zero entry for Dirac lights)
  std::vector<yk_dirac_light_state> dirac_states;   // point / directional (zero entry for area lights)
  std::vector<yk_spot_light_state> spot_states;     // spot lights (zero entry for every other kind)
  std::vector<yk_sphere_light_state> sphere_states; // sphere lights (zero entry for every other kind)
  std::vector<MeshLight> mesh_lights;               // mesh lights (empty entry for every other kind)
  std::vector<yk_sun_light_state> sun_states;       // sun lights (zero entry for every other kind)
  std::vector<BgLight> bg_lights;                   // background lights (empty entry for every other kind)
  bool has_background = false;
  float background[3] = {0.f, 0.f, 0.f};            // constBackground_t::color (color*power)
  // gradientBackground_t: excludes the constant one. gradient_params as set;
  // gradient = szenith, shoriz, gzenith, ghoriz, each times power (gradientback.cc:97)
  bool has_gradient = false;
  yk_gradient_background gradient_params{};
  float gradient[12] = {};
  int background_kind() const { return has_gradient ? YK_BG_GRADIENT : has_background ? YK_BG_CONSTANT : YK_BG_NONE; }
  bool has_bg_light() const {
    for (const int k : light_kind)
      if (k == YK_LIGHT_BACKGROUND) return true;
    return false;
  }
  yk_camera_state camera_state{};
  bool has_camera = false;

  int add_material(const yk_material& m, const yk_glass_params* g = nullptr);
  int add_material_state(const yk_material_state& m, const yk_glass_state* g = nullptr);
  void add_light(const yk_light& l);
  void add_light_state(const yk_area_light_state& l);
  void add_dirac_light_state(const yk_dirac_light_state& l);
  void add_spot_light_state(const yk_spot_light_state& l);
  void add_sphere_light_state(const yk_sphere_light_state& l);
  void add_sun_light_state(const yk_sun_light_state& l);
  void add_mesh_light(const yk_mesh_light& l, const int32_t* obj_ids, int nobj);
  void add_background_light(const yk_background_light& l);
  void set_gradient_background(const yk_gradient_background* g);
  void set_camera(const yk_camera& c);
  void set_camera_state(const yk_camera_state& c);

  // built by finalize(): flattened prim arrays + kd-tree
  std::vector<float> tri_verts;      // 9 floats per prim
  std::vector<int32_t> tri_material; // material id per prim
  std::vector<float> tri_normal;     // geometric normal per prim (triangle_t::recNormal / instance getNormal)
  std::vector<uint8_t> tri_smooth;   // getSurface interpolates vertex normals
  std::vector<float> tri_vnormal;    // 9 floats per prim: va, vb, vc (zero where not smooth)
  bool any_smooth = false;
  KdTree tree;
  bool built = false;
  uint64_t generation = 0;           // unique per finalize() (process-wide), so a device can tell scenes apart
  double build_seconds = 0.0;

  void finalize();                   // scene_t::update: gather prims, build tree
};

// Procedural fixtures (deterministic, no RNG): the probe scenes of BASELINE.md.
Mesh curve_mesh(const float* pts, int n, int material, float strand_start, float strand_end, float strand_shape);
void gen_cornell(Scene& s, int resx, int resy);
void gen_hair(Scene& s, int nstrands, int npoints, int resx, int resy);
void gen_bumpy(Scene& s, int nu, int nv, int resx, int resy);

// Reference constructor arithmetic (IEEE, no contraction):
// shinyDiffuseMat_t / lightMat_t factories, areaLight_t ctor (arealight.cc:30-49),
// camera_t ctor + perspectiveCam_t::setAxis (camera.h:41-60, perspectiveCamera.cc:28-71).
yk_material_state material_state(const yk_material& m);
// glassMat_t factory + ctor (glass.cc:55-69, 262-274): the state and filterCol / fakeShadow beside it
yk_material_state glass_material_state(const yk_material& m, const yk_glass_params& g, yk_glass_state& gs);
yk_area_light_state light_state(const yk_light& l);
yk_dirac_light_state dirac_state(const yk_light& l);
// spotLight_t ctor (spotlight.cc:63-75), sphereLight_t ctor (spherelight.cc:64-72)
yk_spot_light_state spot_state(const yk_light& l);
yk_sphere_light_state sphere_state(const yk_light& l);
// sunLight_t ctor (sunlight.cc:52-63)
yk_sun_light_state sun_state(const yk_light& l);
// shadow slots of one doLightEstimation of scene light i (DLight.nslots)
int light_slots(const Scene& s, size_t i);
yk_camera_state camera_state(const yk_camera& c);

// recNormal: ((b-a)^(c-a)).normalize() with the reference's float op order
// (triangle_inline.h:100-107, vector3d.h:176-260).
void rec_normal(const float* tri, float* n);

}  // namespace yk
