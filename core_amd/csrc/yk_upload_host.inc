// Scene upload (included by yk_device.hip): the record builders make_cam /
// make_*_light / make_mat, upload_qmc, the traversal copies of the resident
// tree (install_traversal), yk_device_open / close / sync and
// yk_device_upload with its steps. Depends on yk_pipe_host.inc, on
// yk_device_host.inc (struct yk_device, bind_constants, the YK_GUARD_*
// macros) and on yk_trace_host.inc (tree_depth, set_tree_bounds,
// fill_trace_occupancy).

namespace {

// Device records from the reference object state (yk_material_state etc.;
// the parameter-level conversion is host arithmetic in scene.cpp).
DCam make_cam(const yk_camera_state& c) {
  DCam C{};
  std::memcpy(C.pos, c.position, sizeof C.pos);
  std::memcpy(C.vright, c.vright, sizeof C.vright);
  std::memcpy(C.vup, c.vup, sizeof C.vup);
  std::memcpy(C.vto, c.vto, sizeof C.vto);
  std::memcpy(C.camZ, c.cam_z, sizeof C.camZ);
  std::memcpy(C.near_p, c.near_p, sizeof C.near_p);
  std::memcpy(C.far_p, c.far_p, sizeof C.far_p);
  C.aperture = c.aperture;
  C.dof_distance = c.dof_distance;
  std::memcpy(C.dof_rt, c.dof_rt, sizeof C.dof_rt);
  std::memcpy(C.dof_up, c.dof_up, sizeof C.dof_up);
  C.bokeh_type = c.bokeh_type;
  C.bokeh_bias = c.bokeh_bias;
  std::memcpy(C.ls, c.lens_ls, sizeof C.ls);
  C.kind = c.kind == YK_CAMERA_ARCHITECT ? YK_CAMERA_PERSPECTIVE : c.kind;
  if (C.kind == YK_CAMERA_ANGULAR) {
    C.resx = (float)c.resx;
    C.resy = (float)c.resy;
    C.aspect = c.aspect_ratio;
    C.hor_phi = c.hor_phi;
    C.max_r = c.max_r;
    C.circular = c.circular ? 1 : 0;
  }
  return C;
}

// areaLight_t ctor tail (arealight.cc:36-49): fnormal = toY ^ toX, normLen,
// corners c2..c4 -- IEEE host arithmetic, -ffp-contract=off
DLight make_light(const yk_area_light_state& L) {
  DLight D{};
  const float* c = L.corner;
  const float* x = L.to_x;
  const float* y = L.to_y;
  float f[3] = {y[1] * x[2] - y[2] * x[1], y[2] * x[0] - y[0] * x[2], y[0] * x[1] - y[1] * x[0]};
  float vl = f[0] * f[0] + f[1] * f[1] + f[2] * f[2];  // normLen, vector3d.h:61-70
  if (vl != 0.f) {
    vl = std::sqrt(vl);
    const float d = 1.0f / vl;
    f[0] *= d;
    f[1] *= d;
    f[2] *= d;
  }
  for (int k = 0; k < 3; ++k) {
    D.corner[k] = c[k];
    D.toX[k] = x[k];
    D.toY[k] = y[k];
    D.fnormal[k] = f[k];
    D.c2[k] = c[k] + x[k];
    D.c3[k] = c[k] + (x[k] + y[k]);
    D.c4[k] = c[k] + y[k];
    D.color[k] = L.color[k];
  }
  for (int k = 0; k < 3; ++k) {  // the device's b - a of triIntersect (arealight.cc:98-115)
    D.e2[k] = D.c2[k] - D.corner[k];
    D.e3[k] = D.c3[k] - D.corner[k];
    D.e4[k] = D.c4[k] - D.corner[k];
  }
  D.area = vl;
  D.samples = L.samples;
  D.type = YK_LIGHT_AREA;
  D.nslots = 2 * L.samples;
  // emitPhoton frame (arealight.cc:40-43): normal = -fnormal; du = toX.normalize(); dv = normal ^ du
  float du[3] = {x[0], x[1], x[2]};
  float len = du[0] * du[0] + du[1] * du[1] + du[2] * du[2];
  if (len != 0.f) {
    len = 1.0f / std::sqrt(len);
    du[0] *= len;
    du[1] *= len;
    du[2] *= len;
  }
  const float n[3] = {-f[0], -f[1], -f[2]};
  for (int k = 0; k < 3; ++k) {
    D.normal[k] = n[k];
    D.du[k] = du[k];
  }
  D.dv[0] = n[1] * du[2] - n[2] * du[1];
  D.dv[1] = n[2] * du[0] - n[0] * du[2];
  D.dv[2] = n[0] * du[1] - n[1] * du[0];
  return D;
}

DLight make_dirac_light(const yk_dirac_light_state& L) {
  DLight D{};
  D.type = L.type;
  D.nslots = 1;
  D.samples = 1;
  for (int k = 0; k < 3; ++k) {
    D.pos[k] = L.position[k];
    D.dir[k] = L.direction[k];
    D.color[k] = L.color[k];
  }
  D.radius = L.radius;
  D.infinite = L.infinite;
  return D;
}

// spotLight_t members as yk_spot_light_state holds them (spotlight.cc:46-60)
DLight make_spot_light(const yk_spot_light_state& L) {
  DLight D{};
  D.type = YK_LIGHT_SPOT;
  D.soft = L.soft_shadows ? 1 : 0;
  D.samples = D.soft ? L.samples : 1;
  D.nslots = D.soft ? 2 * L.samples : 1;  // soft: cone samples + BSDF (MIS) samples
  for (int k = 0; k < 3; ++k) {
    D.pos[k] = L.position[k];
    D.dir[k] = L.dir[k];
    D.ndir[k] = L.ndir[k];
    D.du[k] = L.du[k];
    D.dv[k] = L.dv[k];
    D.color[k] = L.color[k];
  }
  D.cos_start = L.cos_start;
  D.cos_end = L.cos_end;
  D.icos_diff = L.icos_diff;
  D.fuzzy = L.shadow_fuzzyness;
  D.photon_only = L.photon_only ? 1 : 0;
  return D;
}

// sphereLight_t members (spherelight.cc:56-61); canIntersect() is false, so
// an estimate takes `samples` shadow slots and no BSDF (MIS) half
DLight make_sphere_light(const yk_sphere_light_state& L) {
  DLight D{};
  D.type = YK_LIGHT_SPHERE;
  D.samples = L.samples;
  D.nslots = L.samples;
  for (int k = 0; k < 3; ++k) {
    D.pos[k] = L.center[k];
    D.color[k] = L.color[k];
  }
  D.radius = L.radius;
  D.sq_radius = L.square_radius;
  D.sq_radius_eps = L.square_radius_epsilon;
  D.area = L.area;
  return D;
}

// sunLight_t members as yk_sun_light_state holds them (sunlight.cc:42-49), and
// init(scene) (sunlight.cc:65-72) on the scene bound {a, g}: worldRadius =
// 0.5 * (g - a).length() is a double product of the float length, stored to
// float; worldCenter = 0.5 * (a + g) goes through operator*(PFLOAT, point3d_t),
// float products; ePdf = M_PI * worldRadius * worldRadius in double, to float
DLight make_sun_light(const yk_sun_light_state& L, const float* bound) {
  DLight D{};
  D.type = YK_LIGHT_SUN;
  D.soft = 1;  // light_sampled(): doLightEstimation's sample loops
  D.samples = L.samples;
  D.nslots = 2 * L.samples;  // cone samples + BSDF (MIS) samples
  for (int k = 0; k < 3; ++k) {
    D.dir[k] = L.direction[k];
    D.du[k] = L.du[k];
    D.dv[k] = L.dv[k];
    D.color[k] = L.col_pdf[k];
    D.sun_color[k] = L.color[k];
    D.epos[k] = 0.5f * (bound[k] + bound[3 + k]);
  }
  D.pdf = L.pdf;
  D.invpdf = L.invpdf;
  uint64_t w;
  std::memcpy(&w, &L.cos_angle, sizeof w);
  D.cos_angle_w[0] = (unsigned)(w & 0xffffffffu);
  D.cos_angle_w[1] = (unsigned)(w >> 32);
  const float dx = bound[3] - bound[0], dy = bound[4] - bound[1], dz = bound[5] - bound[2];
  D.wradius = (float)(0.5 * (double)std::sqrt(dx * dx + dy * dy + dz * dz));
  D.epdf = (float)(3.14159265358979323846 * (double)D.wradius * (double)D.wradius);
  return D;
}

// directionalLight_t ctor createCS(direction, du, dv) + init(scene)
// (directional.cc:52-75) -- host IEEE arithmetic, -ffp-contract=off
void directional_photon_frame(DLight& D, const float* bound) {
  const float* N = D.dir;
  if (N[0] == 0.f && N[1] == 0.f) {  // createCS, vector3d.h:316-334
    D.edu[0] = N[2] < 0.f ? -1.f : 1.f;
    D.edu[1] = 0.f;
    D.edu[2] = 0.f;
    D.edv[0] = 0.f;
    D.edv[1] = 1.f;
    D.edv[2] = 0.f;
  } else {
    const float d = 1.0f / std::sqrt(N[1] * N[1] + N[0] * N[0]);
    D.edu[0] = N[1] * d;
    D.edu[1] = -N[0] * d;
    D.edu[2] = 0.f;
    D.edv[0] = N[1] * D.edu[2] - N[2] * D.edu[1];
    D.edv[1] = N[2] * D.edu[0] - N[0] * D.edu[2];
    D.edv[2] = N[0] * D.edu[1] - N[1] * D.edu[0];
  }
  const float dx = bound[3] - bound[0], dy = bound[4] - bound[1], dz = bound[5] - bound[2];
  D.wradius = (float)(0.5 * (double)std::sqrt(dx * dx + dy * dy + dz * dz));
  for (int k = 0; k < 3; ++k) D.epos[k] = D.pos[k];
  D.eradius = D.radius;
  if (D.infinite) {
    for (int k = 0; k < 3; ++k) D.epos[k] = 0.5f * (bound[k] + bound[3 + k]);
    D.eradius = D.wradius;
  }
}

DMat make_mat(const yk_material_state& m, const yk_glass_state& g) {
  DMat M{};
  M.type = m.type;
  M.flags = m.bsdf_flags;
  for (int k = 0; k < 3; ++k) {
    M.col[k] = m.color[k];
    M.emit_col[k] = m.emit_color[k];
  }
  M.double_sided = m.double_sided;
  M.on = m.oren_nayar ? 1 : 0;
  M.on_a = m.oren_nayar_a;
  M.on_b = m.oren_nayar_b;
  if (m.type == YK_MAT_GLASS) {
    for (int k = 0; k < 3; ++k) {
      M.gs.filter[k] = g.filter_col[k];
      M.gs.mirror[k] = m.mirror_color[k];
    }
    M.gs.ior = m.ior;
    M.gs.fake_shadow = g.fake_shadow ? 1 : 0;
    return M;
  }
  if (m.type == YK_MAT_GLOSSY || m.type == YK_MAT_COATED_GLOSSY) {
    for (int k = 0; k < 3; ++k) {
      M.col[k] = m.gloss_color[k];
      M.gl.diff[k] = m.diff_color[k];
    }
    if (m.type == YK_MAT_COATED_GLOSSY) {
      for (int k = 0; k < 3; ++k) M.gl.mirror[k] = m.mirror_color[k];
      M.gl.ior = m.ior;
    }
    M.gl.exponent = m.exponent;
    M.gl.exp_u = m.exp_u;
    M.gl.exp_v = m.exp_v;
    M.gl.m_glossy = m.reflectivity;
    M.gl.m_diffuse = m.m_diffuse;
    // initBSDF, glossy.cc:94: std::min(0.6f, x) is (x < 0.6f) ? x : 0.6f, so a NaN x gives 0.6
    const float x = 1.f - (m.reflectivity / (m.reflectivity + (1.f - m.reflectivity) * m.m_diffuse));
    M.gl.p_diffuse = (x < 0.6f) ? x : 0.6f;
    M.gl.with_diffuse = m.with_diffuse ? 1 : 0;
    M.gl.anisotropic = m.anisotropic ? 1 : 0;
    return M;
  }
  for (int k = 0; k < 3; ++k) M.mirror[k] = m.mirror_color[k];
  M.ncomp = std::max(0, std::min(4, (int)m.ncomp));
  for (int i = 0; i < 4; ++i) {
    M.comp[i] = m.component[i];
    M.cflags[i] = m.comp_flags[i];
    M.cindex[i] = std::max(0, std::min(3, (int)m.comp_index[i]));
    if (i < M.ncomp && m.comp_flags[i] == (BSDF_DIFFUSE | BSDF_TRANSMIT)) M.translucent = 1;
  }
  M.tfilter = m.transmit_filter;
  M.fresnel = m.has_fresnel;
  M.ior2 = m.ior_squared;
  return M;
}

void upload_qmc() {
  QmcTables T{};
  std::vector<int> fa;
  int prims[50];
  prims[0] = 1;
  int n = 1;
  for (int c = 2; n < 50; ++c) {
    bool isp = true;
    for (int d = 2; d * d <= c; ++d)
      if (c % d == 0) {
        isp = false;
        break;
      }
    if (isp) prims[n++] = c;
  }
  // Faure permutations by the standard construction (faure_tables.cc)
  std::vector<std::vector<int>> perm(232);
  perm[2] = {0, 1};
  for (int b = 3; b <= 231; ++b) {
    perm[b].resize(b);
    if (b % 2 == 0) {
      const int h = b / 2;
      for (int i = 0; i < h; ++i) {
        perm[b][i] = 2 * perm[h][i];
        perm[b][i + h] = 2 * perm[h][i] + 1;
      }
    } else {
      const int c = (b - 1) / 2;
      int k = 0;
      for (int i = 0; i < b - 1; ++i) {
        if (i == c) perm[b][k++] = c;
        const int v = perm[b - 1][i];
        perm[b][k++] = v >= c ? v + 1 : v;
      }
    }
  }
  for (int d = 0; d < 50; ++d) {
    T.prims[d] = prims[d];
    char buf[64];
    std::snprintf(buf, sizeof buf, "%.9f", 1.0 / prims[d]);
    T.invprims[d] = std::strtod(buf, nullptr);
    T.off[d] = (int)fa.size();
    const std::vector<int>& p = perm[d < 2 ? 3 : prims[d]];
    for (int i = 0; i < prims[d]; ++i) fa.push_back(p[i]);
  }
  if (fa.size() > 5600) throw std::runtime_error("faure table overflow");
  HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(c_qmc), &T, sizeof T));
  HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(c_faure), fa.data(), fa.size() * sizeof(int)));
}

inline unsigned grid_for(long long n, int b = 256) { return (unsigned)((n + b - 1) / b); }

// traversal stack entries hold (node + 1) in 30 bits
constexpr size_t kMaxNodes = (1u << 30) - 2u;
// leaves of this many references need the BIG owner keys (coop_leaves)
constexpr uint32_t kBigLeaf = 1u << 17;

// Ray hand-out per scene: crowded-leaf trees (costly, uneven rays) take
// 64-ray chunks. Refill threshold (idle lanes a wave collects before it
// fetches new rays): 24 (closest hit), 16 (any hit), and 48 for the any-hit kernels on trees of at most
// 2^16 nodes, whose cheap shadow rays make the refill's two dependent loads a
// larger share of a wave's time. Round 3, headline (1M tris) at 16 / 24 / 32:
// 2867 / 2915 / 2902 Mrays/s (any-hit kernel alone 2959 / 2971 / 2919); C2
// (36 tris), both kernels at 16 / 24 / 32 / 40 / 48 / 56 / 64: 8442 / 8669 /
// 8710 / 8791 / 8788 / 8716 / 8426; closest : any-hit at 40:40 / 24:40 /
// 24:48 / 32:48 / 24:56 (3 runs each, one box): 8784 / 8851 / 8938 / 8928 /
// 8889. Round 6, with the merged shadow launch (one larger any-hit launch
// per batch), the any-hit kernel on large trees at 12 / 16 / 20 / 24 (two
// reps, one box): headline 3505-3514 / 3499-3507 / 3484-3495 / 3485-3494,
// both kernels at 16: 3436-3442; the any-hit threshold is 16 since.
// YK_REFILL / YK_REFILL_SHADOW override (tuning). (Round 3 also tried 4 chunks per wave instead of 16 for trees
// of at most 2^16 nodes, as a per-scene value: the runtime divisor made the
// closest-hit kernel spill 9 VGPRs instead of 4, headline 2904 against 2950,
// for no C2 gain in the same A/B: 8927 against 8925.)
// crowded-leaf trees (mean references per non-empty leaf above
// YK_CROWDED_LEAF, default 8): the hair scene's; one threshold for the host
// and the device-built tree
bool crowded(long long filled_leaves, long long leaf_refs) {
  static const double crowd = [] {
    const char* e = std::getenv("YK_CROWDED_LEAF");
    return e ? std::atof(e) : 8.0;
  }();
  const double mean = filled_leaves > 0 ? (double)leaf_refs / (double)filled_leaves : 0.0;
  return mean > crowd;
}

void set_handout(yk_device* d, size_t nn) {
  const char* e = std::getenv("YK_REFILL_SHADOW");
  const int rs = e ? std::atoi(e) : 0;
  d->refill = refill_env() ? refill_env() : 24;
  d->refill_shadow = (rs >= 1 && rs <= 64) ? rs : (refill_env() ? refill_env() : (nn <= (1u << 16) ? 48 : 16));
  d->S.chunk_max = d->crowded_leaves ? 64u : (unsigned)YK_POOL_CHUNK_MAX;
}

// Node packets of the resident tree (k_pack_nodes).
void pack_nodes(yk_device* d, size_t nn) {
  launch(k_pack_nodes, grid_for((long long)nn), 256, 0, d->stream, d->nodes.p, d->pk.p, (unsigned)nn);
  d->S.pk = d->pk.p;
}

// Traversal copies of the resident tree, both made on the device from the
// uploaded nodes / leaf lists / records: the leaf-ordered records and the
// node packets.
void install_traversal(yk_device* d, size_t nn, size_t nleaf, uint32_t max_leaf_refs) {
  d->big_leaves = max_leaf_refs >= kBigLeaf;
  HIPCHK(hipDeviceSynchronize());  // every copy into nodes / leaf / tris has landed
  if (nleaf) {
    d->ltris.ensure(kTriWords * nleaf + kRecPad);
    launch(k_gather_leaf_tris, grid_for((long long)nleaf), 256, 0, d->stream, d->tris.p, d->leaf.p, d->ltris.p,
           (unsigned)nleaf);
  }
  d->S.ltris = nleaf ? d->ltris.p : nullptr;
  d->S.nlref = (unsigned)nleaf;
  d->pk.ensure(kPkWords * nn);
  pack_nodes(d, nn);
  HIPCHK(hipStreamSynchronize(d->stream));
  // small scenes trace from an LDS copy of the traversal data. YK_SMALL (read
  // per upload: A/B runs, tests): 0 never, a byte count > 1 overrides the
  // size limit YK_SMALL_MAX (at most 46 KB: with the
  // per-wave blocks a workgroup stays within 64 KB of LDS)
  const char* small_env = std::getenv("YK_SMALL");
  const long long small_v = small_env ? std::atoll(small_env) : 1;
  const size_t small_max = small_v > 1 ? (size_t)std::min(small_v, 47104ll) : (size_t)YK_SMALL_MAX;
  d->small_bytes = small_scene_bytes(nn, d->S.ntris, nleaf);
  d->small = small_v != 0 && d->small_bytes <= small_max;
  if (d->small) fill_trace_occupancy(d, true);
}

// ---- the steps of yk_device_upload, in the order it takes them

// Every refusal that reads host data only: YK_OK, or the error set and nothing of the handle touched. On the way it
// works out what later steps use: the depth of the scene's kd-tree and of every mesh light's (0 for the other lights).
int check_upload(const Scene& S, int& depth, std::vector<int>& mesh_depth) {
  if (!S.built) return set_error(YK_ERR_STATE, "yk_device_upload: scene not built (call yk_scene_build)");
  if (!S.has_camera) return set_error(YK_ERR_STATE, "yk_device_upload: scene has no camera");
  if ((int)S.material_states.size() > kMaxMats) return set_error(YK_ERR_UNSUPPORTED, "too many materials");
  if ((int)S.light_states.size() > kMaxLights) return set_error(YK_ERR_UNSUPPORTED, "too many lights");
  if (S.tree.nodes.size() / 2 > kMaxNodes) return set_error(YK_ERR_UNSUPPORTED, "kd-tree has 2^30 - 1 nodes or more");
  int slots = 0;  // shadow slots per doLightEstimation sweep (DLight.nslots)
  for (size_t i = 0; i < S.light_states.size(); ++i) {
    const int n = light_slots(S, i);  // 1 for a Dirac light, else from the light's samples
    if (n < 1) return set_error(YK_ERR_ARG, "light samples must be >= 1");
    if (n > 8192) return set_error(YK_ERR_UNSUPPORTED, "too many light samples per shading point");
    slots += n;
  }
  if (slots > 8192) return set_error(YK_ERR_UNSUPPORTED, "too many light samples per shading point");
  std::string terr;
  depth = tree_depth(S.tree.nodes.data(), S.tree.nodes.size() / 2, S.tree.leaf_prims.size(), S.tri_material.size(),
                     &terr);
  if (depth < 0) return set_error(YK_ERR_ARG, "yk_device_upload: " + terr);
  // mesh lights: a tree deeper than the shading kernels' per-lane stack is refused, not cut
  mesh_depth.assign(S.light_states.size(), 0);
  for (size_t i = 0; i < S.light_states.size(); ++i) {
    if (S.light_kind[i] != YK_LIGHT_MESH) continue;
    const MeshLight& ML = S.mesh_lights[i];
    if (ML.areas.size() > (size_t)YK_MESH_LIGHT_MAX_TRIS)
      return set_error(YK_ERR_UNSUPPORTED, "mesh light has more than YK_MESH_LIGHT_MAX_TRIS triangles");
    std::string lerr;
    mesh_depth[i] = tree_depth(ML.tree.nodes.data(), ML.tree.nodes.size() / 2, ML.tree.leaf_prims.size(),
                               ML.areas.size(), &lerr);
    if (mesh_depth[i] < 0) return set_error(YK_ERR_ARG, "yk_device_upload: mesh light: " + lerr);
    if (mesh_depth[i] > YK_MESH_LIGHT_MAX_DEPTH)
      return set_error(YK_ERR_UNSUPPORTED, "mesh light kd-tree deeper than YK_MESH_LIGHT_MAX_DEPTH");
  }
  return YK_OK;
}

// The triangle record {v0, e1, e2} (kTriWords floats) of the nine vertex floats: the scene's and the mesh lights'.
void tri_record(const float* t, float* r) {
  for (int k = 0; k < 3; ++k) {
    r[k] = t[k];
    r[3 + k] = t[3 + k] - t[k];
    r[6 + k] = t[6 + k] - t[k];
  }
}

// The scene's geometry into the resident arrays: records, normals, vertex normals, nodes (+ the padding node), leaf lists.
void upload_geometry(yk_device* d, const Scene& S) {
  const size_t nt = S.tri_material.size(), nn = S.tree.nodes.size() / 2;
  std::vector<float> tris(nt * kTriWords, 0.f);
  std::vector<float4> ng(nt);
  for (size_t p = 0; p < nt; ++p) {
    tri_record(&S.tri_verts[9 * p], &tris[p * kTriWords]);
    float nw;
    const int m = S.tri_material[p] | (S.tri_smooth[p] ? kSmoothBit : 0);
    std::memcpy(&nw, &m, 4);
    ng[p] = make_float4(S.tri_normal[3 * p], S.tri_normal[3 * p + 1], S.tri_normal[3 * p + 2], nw);
  }
  d->tris.ensure(tris.size() + kRecPad);
  d->ng.ensure(ng.size());
  d->nodes.ensure(nn + 1);  // + one padding node for the node-pair loads
  HIPCHK(hipMemset(d->nodes.p + nn, 0, sizeof(uint2)));
  d->leaf.ensure(std::max<size_t>(S.tree.leaf_prims.size(), 1));
  HIPCHK(hipMemcpy(d->tris.p, tris.data(), tris.size() * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d->ng.p, ng.data(), ng.size() * sizeof(float4), hipMemcpyHostToDevice));
  if (S.any_smooth) {
    d->vn.ensure(S.tri_vnormal.size());
    HIPCHK(hipMemcpy(d->vn.p, S.tri_vnormal.data(), S.tri_vnormal.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  HIPCHK(hipMemcpy(d->nodes.p, S.tree.nodes.data(), nn * sizeof(uint2), hipMemcpyHostToDevice));
  if (!S.tree.leaf_prims.empty())
    HIPCHK(hipMemcpy(d->leaf.p, S.tree.leaf_prims.data(), S.tree.leaf_prims.size() * sizeof(uint32_t),
                     hipMemcpyHostToDevice));
}

// The material records, and what the handle derives from them: spec, ts_glass, mat_flags, the material level.
std::vector<DMat> build_materials(yk_device* d, const Scene& S) {
  std::vector<DMat> mats;
  d->spec = false;
  d->mat_flags.clear();
  d->ts_glass = false;
  // the scene's material level: the highest any material needs; YK_DIFF=0: never the diffuse-only one
  const char* e = std::getenv("YK_DIFF");
  int level = (e && std::atoi(e) == 0) ? kMatGeneral : kMatDiffuse;
  for (size_t i = 0; i < S.material_states.size(); ++i) {
    const auto& s = S.material_states[i];
    mats.push_back(make_mat(s, S.glass_states[i]));
    d->mat_flags.push_back(s.bsdf_flags);
    if (s.bsdf_flags & (BSDF_SPECULAR | BSDF_FILTER)) d->spec = true;
    if (s.type == YK_MAT_GLASS && S.glass_states[i].fake_shadow) d->ts_glass = true;
    const DMat& m = mats.back();
    const bool diff = m.type == YK_MAT_LIGHT || (m.ncomp == 1 && m.cflags[0] == (BSDF_DIFFUSE | BSDF_REFLECT) && !m.on);
    level = std::max<int>(level, m.type == YK_MAT_GLASS ? kMatGlass : m.type == YK_MAT_COATED_GLOSSY ? kMatCoated
                                 : m.type == YK_MAT_GLOSSY ? kMatGlossy : diff ? kMatDiffuse : kMatGeneral);
  }
  d->shade.mat = level;
  return mats;
}

// The mesh lights of a scene as they go to the device: one record per light, its arrays packed in three buffers.
struct MeshLightPack {
  std::vector<DMeshLight> recs;  // pointers filled in by upload_mesh_lights, once the buffers have their size
  std::vector<float> f;          // per light: cdf (n + 1), verts (9n), records (kTriWords * n, + kRecPad), normals (3n)
  std::vector<uint32_t> nodes, leaf;
  std::vector<size_t> off;  // per record: float, node (in nodes) and leaf offsets
};

// meshLight_t as a DLight, its arrays appended to the pack
DLight make_mesh_light(const MeshLight& ML, int depth, MeshLightPack& P) {
  const size_t n = ML.areas.size(), nn = ML.tree.nodes.size() / 2;
  DLight D{};
  D.type = YK_LIGHT_MESH;
  D.samples = ML.params.samples;
  D.nslots = 2 * ML.params.samples;  // light samples + BSDF (MIS) samples
  D.area = ML.area;
  D.double_sided = ML.params.double_sided ? 1 : 0;
  D.mesh = (int)P.recs.size();
  for (int k = 0; k < 3; ++k) D.color[k] = ML.color[k];
  DMeshLight R{};
  std::memcpy(R.bound, ML.tree.bound, sizeof R.bound);
  R.n = (int)n;
  R.nnodes = (unsigned)nn;
  R.depth_cap = (unsigned)depth + 2u;
  R.nleaf = (unsigned)ML.tree.leaf_prims.size();
  P.recs.push_back(R);
  P.off.push_back(P.f.size());
  P.off.push_back(P.nodes.size() / 2);
  P.off.push_back(P.leaf.size());
  P.f.insert(P.f.end(), ML.cdf.begin(), ML.cdf.end());
  P.f.insert(P.f.end(), ML.verts.begin(), ML.verts.end());
  const size_t at = P.f.size();
  P.f.resize(at + kTriWords * n + kRecPad, 0.f);
  for (size_t p = 0; p < n; ++p) tri_record(&ML.verts[9 * p], &P.f[at + kTriWords * p]);
  P.f.insert(P.f.end(), ML.normals.begin(), ML.normals.end());
  P.nodes.insert(P.nodes.end(), ML.tree.nodes.begin(), ML.tree.nodes.end());
  P.nodes.insert(P.nodes.end(), 2, 0u);  // one padding node for the node-pair loads
  P.leaf.insert(P.leaf.end(), ML.tree.leaf_prims.begin(), ML.tree.leaf_prims.end());
  P.leaf.push_back(0u);
  return D;
}

// bgLight_t as a DLight bound to the scene's background, with what init(scene)
// takes from the scene bound (bglight.cc:112-117, as make_sun_light): aPdf =
// worldRadius * worldRadius. Its tables go to the mesh-light pack as one run
// of words in the order bg_tables reads them.
DLight make_bg_light(const Scene& S, const BgLight& BL, MeshLightPack& P) {
  const float* bound = S.tree.bound;
  DLight D{};
  D.type = YK_LIGHT_BACKGROUND;
  D.soft = 1;  // light_sampled(): doLightEstimation's sample loops
  D.samples = BL.params.samples;
  D.nslots = 2 * BL.params.samples;  // table samples + BSDF (MIS) samples
  D.bg.kind = S.background_kind();
  D.bg.abs_inter = BL.params.abs_intersect ? 1 : 0;
  D.bg.v_inv_integral = BL.v_inv_integral;
  D.bg.total_u = (int)BL.func_u.size();
  for (int k = 0; k < 12; ++k) D.bg.grad[k] = S.gradient[k];
  for (int k = 0; k < 3; ++k) {
    D.color[k] = S.background[k];
    D.epos[k] = 0.5f * (bound[k] + bound[3 + k]);
  }
  const float dx = bound[3] - bound[0], dy = bound[4] - bound[1], dz = bound[5] - bound[2];
  D.wradius = (float)(0.5 * (double)std::sqrt(dx * dx + dy * dy + dz * dz));
  D.area = D.wradius * D.wradius;
  D.mesh = (int)P.recs.size();
  DMeshLight R{};  // nnodes == 0: no mesh behind it (upload_mesh_lights)
  R.n = (int)BL.row_count.size();
  P.recs.push_back(R);
  P.off.push_back(P.f.size());
  P.off.push_back(P.nodes.size() / 2);
  P.off.push_back(P.leaf.size());
  auto words = [&P](const std::vector<int32_t>& v) {
    const size_t at = P.f.size();
    P.f.resize(at + v.size());
    std::memcpy(&P.f[at], v.data(), v.size() * sizeof(int32_t));
  };
  words(BL.row_count);
  words(BL.row_offset);
  P.f.insert(P.f.end(), BL.row_inv_integral.begin(), BL.row_inv_integral.end());
  P.f.insert(P.f.end(), BL.func_v.begin(), BL.func_v.end());
  P.f.insert(P.f.end(), BL.cdf_v.begin(), BL.cdf_v.end());
  P.f.insert(P.f.end(), BL.func_u.begin(), BL.func_u.end());
  P.f.insert(P.f.end(), BL.cdf_u.begin(), BL.cdf_u.end());
  return D;
}

// The light records in scene order, and the mesh lights' arrays packed.
std::vector<DLight> build_lights(const Scene& S, const std::vector<int>& mesh_depth, MeshLightPack& P) {
  std::vector<DLight> lights;
  for (size_t i = 0; i < S.light_states.size(); ++i) {
    switch (S.light_kind[i]) {
      case YK_LIGHT_MESH: lights.push_back(make_mesh_light(S.mesh_lights[i], mesh_depth[i], P)); break;
      case YK_LIGHT_AREA: lights.push_back(make_light(S.light_states[i])); break;
      case YK_LIGHT_SPOT: lights.push_back(make_spot_light(S.spot_states[i])); break;
      case YK_LIGHT_SPHERE: lights.push_back(make_sphere_light(S.sphere_states[i])); break;
      case YK_LIGHT_SUN: lights.push_back(make_sun_light(S.sun_states[i], S.tree.bound)); break;
      case YK_LIGHT_BACKGROUND: lights.push_back(make_bg_light(S, S.bg_lights[i], P)); break;
      default:
        lights.push_back(make_dirac_light(S.dirac_states[i]));
        if (lights.back().type == YK_LIGHT_DIRECTIONAL) directional_photon_frame(lights.back(), S.tree.bound);
    }
  }
  return lights;
}

// The packed mesh lights into the handle's four buffers, the records' pointers set to where their arrays landed.
void upload_mesh_lights(yk_device* d, MeshLightPack& P) {
  d->S.ml = nullptr;
  if (P.recs.empty()) return;
  d->ml_f.ensure(P.f.size());
  d->ml_nodes.ensure(std::max<size_t>(P.nodes.size() / 2, 1));
  d->ml_leaf.ensure(std::max<size_t>(P.leaf.size(), 1));
  d->ml_recs.ensure(P.recs.size());
  for (size_t k = 0; k < P.recs.size(); ++k) {
    DMeshLight& R = P.recs[k];
    const size_t n = (size_t)R.n;
    const float* f = d->ml_f.p + P.off[3 * k];
    R.cdf = f;
    if (R.nnodes == 0) continue;  // a background light's tables (make_bg_light): cdf alone
    R.verts = f + (n + 1);
    R.tris = R.verts + 9 * n;
    R.nrm = R.tris + kTriWords * n + kRecPad;
    R.nodes = d->ml_nodes.p + P.off[3 * k + 1];
    R.leaf = d->ml_leaf.p + P.off[3 * k + 2];
  }
  HIPCHK(hipMemcpy(d->ml_f.p, P.f.data(), P.f.size() * sizeof(float), hipMemcpyHostToDevice));
  if (!P.nodes.empty())
    HIPCHK(hipMemcpy(d->ml_nodes.p, P.nodes.data(), P.nodes.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  if (!P.leaf.empty())
    HIPCHK(hipMemcpy(d->ml_leaf.p, P.leaf.data(), P.leaf.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d->ml_recs.p, P.recs.data(), P.recs.size() * sizeof(DMeshLight), hipMemcpyHostToDevice));
  d->S.ml = d->ml_recs.p;
}

// The scene's light level (ShadeVariant::xl): the highest any light needs.
int light_level(const std::vector<DLight>& lights) {
  int xl = kXLNone;
  for (const DLight& L : lights)
    xl = std::max(xl, L.type == YK_LIGHT_BACKGROUND ? kXLBg
                      : L.type == YK_LIGHT_SUN  ? kXLSun
                      : L.type == YK_LIGHT_MESH ? kXLMesh
                      : (L.type == YK_LIGHT_SPOT || L.type == YK_LIGHT_SPHERE) ? kXLSpotSphere : kXLNone);
  return xl;
}

// DScene of the uploaded geometry, its traversal copies, the ray hand-out and the tree bounds.
void install_scene(yk_device* d, const Scene& S, int depth) {
  const size_t nn = S.tree.nodes.size() / 2;
  d->S.tris = d->tris.p;
  d->S.nodes = d->nodes.p;
  d->S.leaf = d->leaf.p;
  d->S.ng = d->ng.p;
  d->S.vn = S.any_smooth ? d->vn.p : nullptr;
  std::memcpy(d->S.bound, S.tree.bound, sizeof d->S.bound);
  d->S.nlights = (int)S.light_states.size();
  d->S.nmats = (int)S.material_states.size();
  d->S.nnodes = (unsigned)nn;
  d->S.ntris = (unsigned)S.tri_material.size();
  d->S.uni = S.mode == YK_MODE_UNIVERSAL ? 1 : 0;
  uint32_t max_refs = 0;
  for (size_t i = 0; i < nn; ++i)
    if ((S.tree.nodes[2 * i + 1] & 3u) == 3u) max_refs = std::max(max_refs, S.tree.nodes[2 * i + 1] >> 2);
  install_traversal(d, nn, S.tree.leaf_prims.size(), max_refs);
  const long long filled = (long long)S.tree.stats.leaves - S.tree.stats.empty_leaves;
  d->crowded_leaves = crowded(filled, (long long)S.tree.stats.leaf_prims);
  set_handout(d, nn);
  set_tree_bounds(d, depth);
  d->nleaf = S.tree.leaf_prims.size();
}

}  // namespace

extern "C" {

int yk_device_open(int32_t ordinal, yk_device** out) {
  if (!out) return set_error(YK_ERR_ARG, "yk_device_open: out is NULL");
  YK_GUARD_BEGIN
  int n = 0;
  HIPCHK(hipGetDeviceCount(&n));
  if (ordinal < 0 || ordinal >= n) return set_error(YK_ERR_ARG, "yk_device_open: no such device");
  HIPCHK(hipSetDevice(ordinal));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, ordinal));
  if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos)
    return set_error(YK_ERR_UNSUPPORTED, std::string("libyk is built for gfx950, device is ") + prop.gcnArchName);
  yk_device* d = new yk_device();
  d->ordinal = ordinal;
  d->cus = prop.multiProcessorCount;
  for (auto& P : d->pipe) P.create();
  for (auto& e : d->gather_ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  d->stream = d->pipe[0].stream;
  std::fill(d->per_cu, d->per_cu + kTraceVariants, 1);
  fill_trace_occupancy(d, false);
  int blocks = 0;
  HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, k_trace_shadow_ts, 64, 0));
  d->per_cu_ts = std::max(1, blocks);
  HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, k_trace_shadow_ts_glass, 64, 0));
  d->per_cu_ts_glass = std::max(1, blocks);
  HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, k_pm_lookup<false>, 64, 0));
  d->per_cu_lookup[0] = std::max(1, blocks);
  if (const char* v = std::getenv("YK_VERBOSE"); v && std::atoi(v) > 0)
    std::fprintf(stderr, "[libyk] %d CUs; resident workgroups per CU: any-hit %d, closest %d, big %d / %d, "
                 "transparent-shadow %d\n", d->cus, d->per_cu[kShadow], d->per_cu[kClosest], d->per_cu[kShadowBig],
                 d->per_cu[kClosestBig], d->per_cu_ts);
  upload_qmc();
  *out = d;
  return YK_OK;
  YK_GUARD_END
}

void yk_device_close(yk_device* d) {
  if (!d) return;
  (void)hipSetDevice(d->ordinal);
  (void)hipStreamSynchronize(d->stream);
  delete d;
}

void* yk_device_stream(yk_device* d) { return d ? (void*)d->stream : nullptr; }

int yk_device_count(int32_t* n) {
  if (!n) return set_error(YK_ERR_ARG, "yk_device_count: NULL argument");
  YK_GUARD_BEGIN
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
  *n = c;
  return YK_OK;
  YK_GUARD_END
}

int yk_device_set_abort(yk_device* d, yk_abort_fn fn, void* user) {
  if (!d) return set_error(YK_ERR_ARG, "yk_device_set_abort: NULL device");
  d->abort_fn = fn;
  d->abort_user = user;
  return YK_OK;
}

int yk_device_sync(yk_device* d) {
  if (!d) return set_error(YK_ERR_ARG, "yk_device_sync: NULL device");
  YK_GUARD_BEGIN
  HIPCHK(hipStreamSynchronize(d->stream));
  return YK_OK;
  YK_GUARD_END
}

int yk_device_upload(yk_device* d, const yk_scene* s) {
  if (!d || !s) return set_error(YK_ERR_ARG, "yk_device_upload: NULL argument");
  const Scene& S = s->s;
  YK_GUARD_BEGIN
  int depth = 0;
  std::vector<int> mesh_depth;
  if (const int rc = check_upload(S, depth, mesh_depth)) return rc;
  HIPCHK(hipSetDevice(d->ordinal));
  // the resident arrays are replaced below: until that has succeeded the
  // device holds no usable scene
  d->uploaded = false;
  d->uploaded_scene = nullptr;
  upload_geometry(d, S);
  std::vector<DMat> mats = build_materials(d, S);
  MeshLightPack mesh_lights;
  std::vector<DLight> lights = build_lights(S, mesh_depth, mesh_lights);
  upload_mesh_lights(d, mesh_lights);
  d->shade.xl = light_level(lights);
  d->sum_light_slots = 0;
  for (const DLight& L : lights) d->sum_light_slots += L.nslots;
  d->lights_host = std::move(lights);
  d->mats_host = std::move(mats);
  d->pm_ready = false;
  d->bg_kind = S.background_kind();
  for (int k = 0; k < 3; ++k) d->bg[k] = S.background[k];
  for (int k = 0; k < 12; ++k) d->bg_grad[k] = S.gradient[k];
  d->cam_host = make_cam(S.camera_state);
  d->cam_resx = S.camera_state.resx;
  d->cam_resy = S.camera_state.resy;
  d->cam_has_clip = S.camera_has_params;
  d->cam_near_clip = S.camera.near_clip;
  d->cam_far_clip = S.camera.far_clip;
  install_scene(d, S, depth);
  d->nlights = (int)S.light_states.size();
  d->ntris = (int)S.tri_material.size();
  d->uploaded = true;
  d->uploaded_scene = s;
  d->uploaded_gen = S.generation;
  d->const_token = g_upload_token.fetch_add(1);
  bind_constants(d);  // materials, lights and camera into the GPU's constant memory
  return YK_OK;
  YK_GUARD_END
}

}  // extern "C"
