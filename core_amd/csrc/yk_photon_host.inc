// Host half of photonIntegrator_t::preprocess (photonintegr.cc:126-633),
// included at the end of yk_device.hip. The photon paths and the radiance
// pre-gather run on the device; the ordered photon-vector assembly, the
// ourRandom() radiance-point choice, the point kd-trees and the radiance
// point elimination are sequential in the reference and run here.

namespace {

// deepest point kd-tree the device lookups take: a lookup pushes one stack
// entry per interior level, and the stacks hold kPStack
constexpr int kMaxPointTreeDepth = kPStack - 2;

// light_t::totalEnergy().energy(): areaLight_t color * area (arealight.cc:66),
// pointLight_t color * 4.0f * M_PI (pointlight.cc:32), directionalLight_t
// color * radius*radius * M_PI (directional.cc:33), sunLight_t color * ePdf
// (sunlight.cc:32); energy() = (R+G+B)*0.333333f
float light_energy(const DLight& L) {
  float e[3];
  for (int k = 0; k < 3; ++k) {
    if (L.type == YK_LIGHT_POINT) e[k] = (L.color[k] * 4.0f) * (float)YK_PI_D;
    else if (L.type == YK_LIGHT_DIRECTIONAL) e[k] = ((L.color[k] * L.eradius) * L.eradius) * (float)YK_PI_D;
    else if (L.type == YK_LIGHT_SUN) e[k] = L.sun_color[k] * L.epdf;
    else e[k] = L.color[k] * L.area;
  }
  return ((e[0] + e[1]) + e[2]) * 0.333333f;
}

void upload_map(yk_device* d, int which, const std::vector<float>& ph, const PointTree& t) {
  const int n = (int)(ph.size() / 9);
  std::vector<float4> pos(n), dir(n), col(n);
  for (int i = 0; i < n; ++i) {
    const float* p = &ph[9 * (size_t)i];
    pos[i] = make_float4(p[0], p[1], p[2], 0.f);
    dir[i] = make_float4(p[3], p[4], p[5], 0.f);
    col[i] = make_float4(p[6], p[7], p[8], 0.f);
  }
  const bool radiance = which == YK_PHOTON_MAP_RADIANCE, caustic = which == YK_PHOTON_MAP_CAUSTIC;
  DBuf<uint2>& nodes = radiance ? d->rm_nodes : (caustic ? d->cm_nodes : d->dm_nodes);
  DBuf<float4>& P = radiance ? d->rm_pos : (caustic ? d->cm_pos : d->dm_pos);
  DBuf<float4>& D = radiance ? d->rm_dir : (caustic ? d->cm_dir : d->dm_dir);
  DBuf<float4>& C = radiance ? d->rm_col : (caustic ? d->cm_col : d->dm_col);
  nodes.ensure(std::max<size_t>(1, t.nodes.size() / 2));
  P.ensure(std::max(1, n));
  D.ensure(std::max(1, n));
  C.ensure(std::max(1, n));
  if (n > 0) {
    HIPCHK(hipMemcpy(nodes.p, t.nodes.data(), t.nodes.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(P.p, pos.data(), n * sizeof(float4), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(D.p, dir.data(), n * sizeof(float4), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(C.p, col.data(), n * sizeof(float4), hipMemcpyHostToDevice));
  }
  if (radiance) {  // 16-B nodes for k_pm_lookup: a leaf carries its photon's position
    const size_t nn = t.nodes.size() / 2;
    std::vector<uint4> pk(std::max<size_t>(1, nn));
    for (size_t i = 0; i < nn; ++i) {
      const uint32_t w0 = t.nodes[2 * i], w1 = t.nodes[2 * i + 1];
      if ((w1 & 3u) == 3u) {
        uint32_t b[3];
        std::memcpy(b, &pos[w0], sizeof b);
        pk[i] = make_uint4(b[0], b[1], b[2], 3u | (w0 << 2));
      } else {
        pk[i] = make_uint4(w0, 0u, 0u, w1);
      }
    }
    d->rm_pk.ensure(pk.size());
    HIPCHK(hipMemcpy(d->rm_pk.p, pk.data(), pk.size() * sizeof(uint4), hipMemcpyHostToDevice));
  }
}

}  // namespace

PMConst pm_const(const yk_device* d, const yk_photon_params& q) {
  PMConst M{};
  M.dmap = PMapDev{d->dm_nodes.p, d->dm_pos.p, d->dm_dir.p, d->dm_col.p, (int)(d->dm_host.size() / 9)};
  M.rmap = PMapDev{d->rm_nodes.p, d->rm_pos.p, d->rm_dir.p, d->rm_col.p, (int)(d->rm_host.size() / 9), d->rm_pk.p};
  M.final_gather = q.final_gather ? 1 : 0;
  M.show_map = q.show_map ? 1 : 0;
  M.search = q.search;
  M.fg_bounces = q.fg_bounces;
  M.dpaths = d->dm_paths;
  M.gather_dist = q.fg_min_pathlen;
  M.lookup_rad = (4 * q.diffuse_radius) * q.diffuse_radius;  // lookupRad, photonintegr.cc:535
  M.ds_radius = q.diffuse_radius;
  M.cmap = PMapDev{d->cm_nodes.p, d->cm_pos.p, d->cm_dir.p, d->cm_col.p, (int)(d->cm_host.size() / 9)};
  M.caustic_mix = q.caustic_mix;
  M.cpaths = d->cm_paths;
  M.caus_radius = q.caustic_radius;
  return M;
}

extern "C" {

int yk_photon_build(yk_device* d, const yk_render_params* p, yk_photon_info* info) {
  if (!d || !p) return set_error(YK_ERR_ARG, "yk_photon_build: NULL argument");
  if (!d->uploaded) return set_error(YK_ERR_STATE, "yk_photon_build: no scene uploaded");
  const yk_photon_params& q = p->photon;
  // pathtracing with caustic_type photon / both: pathIntegrator_t::preprocess
  // builds only the caustic map (createCausticMap, mcintegrator.cc:197-377)
  // directlighting with "caustics" runs the same pass (directLighting_t::
  // preprocess, directlight.cc:78-83): pt stands for "the caustic map alone"
  const bool pt = p->integrator == YK_INTEGRATOR_PATH ||
                  (p->integrator == YK_INTEGRATOR_DIRECT && p->dl_caustics != 0);
  if (!pt && p->integrator != YK_INTEGRATOR_PHOTON)
    return set_error(YK_ERR_ARG, "yk_photon_build: integrator must be photonmapping, pathtracing or directlighting "
                                 "with caustics");
  if (!pt && d->nlights < 1) return set_error(YK_ERR_STATE, "photon mapping: the scene has no lights");
  for (const DLight& L : d->lights_host)  // emitPhoton of these lights is not on the path
    if (L.type == YK_LIGHT_SPOT || L.type == YK_LIGHT_SPHERE)
      return set_error(YK_ERR_UNSUPPORTED,
                       "yk_photon_build: the scene holds a spot or sphere light, whose photon emission is not "
                       "supported (direct lighting and path tracing without photon caustics are)");
  for (const DLight& L : d->lights_host)  // meshLight_t::emitPhoton / emitSample are not on the path
    if (L.type == YK_LIGHT_MESH)
      return set_error(YK_ERR_UNSUPPORTED,
                       "yk_photon_build: the scene holds a mesh light, whose photon emission is not supported "
                       "(direct lighting and path tracing without photon caustics are)");
  for (const DLight& L : d->lights_host)  // bgLight_t::emitPhoton is not on the path
    if (L.type == YK_LIGHT_BACKGROUND)
      return set_error(YK_ERR_UNSUPPORTED,
                       "yk_photon_build: the scene holds a background light, whose photon emission is not supported "
                       "(direct lighting and path tracing without photon caustics are)");
  if (!pt && q.photons <= 0) return set_error(YK_ERR_ARG, "photons must be > 0");
  if (!pt && (q.search < 1 || q.search > kMaxSearch)) return set_error(YK_ERR_UNSUPPORTED, "search must be in [1, 256]");
  if (q.caustic_mix < 1 || q.caustic_mix > kMaxSearch) return set_error(YK_ERR_UNSUPPORTED, "caustic_mix must be in [1, 256]");
  if (q.caustic_photons < 0) return set_error(YK_ERR_ARG, "cPhotons must be >= 0");
  if (q.bounces < 0 || 3 * q.bounces + 7 > 50) return set_error(YK_ERR_UNSUPPORTED, "photon bounces must be in [0, 14]");
  if (!pt && (q.fg_bounces < 0 || 4 * q.fg_bounces + 4 >= 50)) return set_error(YK_ERR_UNSUPPORTED, "fg_bounces must be in [0, 11]");
  YK_GUARD_BEGIN
  HIPCHK(hipSetDevice(d->ordinal));
  bind_constants(d);
  auto t0 = std::chrono::steady_clock::now();
  d->pm_ready = false;
  const int nL = d->nlights;
  const unsigned N = pt ? (unsigned)q.caustic_photons : (unsigned)q.photons;
  const int MB = q.bounces;
  // pdf1D_t over the light energies (CumulateStep1dDF, sample_utils.h:85-118)
  PhotonConst PC{};
  PC.nphotons = N;
  PC.nlights = nL;
  PC.fnum_lights = (float)nL;
  PC.inv_photons = 1.f / (float)N;
  PC.max_bounces = MB;
  PC.final_gather = q.final_gather ? 1 : 0;
  if (nL > 0) {
    double c = 0.0, delta = 1.0 / (double)nL;
    PC.cdf[0] = 0.0f;
    for (int i = 0; i < nL; ++i) {
      PC.func[i] = light_energy(d->lights_host[i]);
      c += (double)PC.func[i] * delta;
      PC.cdf[i + 1] = (float)c;
    }
    const float integral = (float)c;
    for (int i = 1; i < nL + 1; ++i) PC.cdf[i] /= integral;
    PC.inv_integral = 1.f / integral;
  }
  // ---- photon paths on the device: one pass per map (the same kernels)
  Pipe& P = d->pipe[0];
  unsigned long long photon_rays = 0;
  struct PassOut {
    std::vector<uint8_t> flag;
    std::vector<float4> pos, wi, col, nrm, refl, trn;
  };
  auto run_pass = [&](unsigned N, int caustic_pass, PassOut& o) {
    PhotonConst C = PC;
    C.nphotons = N;
    C.inv_photons = 1.f / (float)N;
    C.caustic_pass = caustic_pass;
    // DSample(curr / N) must stay below nL (photonintegr.cc:231-237, mcintegrator.cc:262-268)
    const float smax = caustic_pass == 2 ? (float)(N - 1) / (float)N : (float)(N - 1) * C.inv_photons;
    if (N > 1 && !(smax <= C.cdf[nL])) throw std::runtime_error("lightPDF sample error");
    const bool rad = q.final_gather && !caustic_pass;
    const size_t nslots = (size_t)N * (MB + 1);
    DBuf<yk_ray> qr0, qr1;
    DBuf<yk_hit> qh0, qh1;
    DBuf<unsigned> qi0, qi1;
    DBuf<float> pcol;
    DBuf<uint8_t> pfl, s_flag;
    DBuf<float4> s_pos, s_wi, s_col, s_nrm, s_refl, s_trn;
    qr0.ensure(N);
    qr1.ensure(N);
    qh0.ensure(N);
    qh1.ensure(N);
    qi0.ensure(N);
    qi1.ensure(N);
    pcol.ensure(3 * (size_t)N);
    pfl.ensure(N);
    s_flag.ensure(nslots);
    s_pos.ensure(nslots);
    s_wi.ensure(nslots);
    s_col.ensure(nslots);
    if (rad) {
      s_nrm.ensure(nslots);
      s_refl.ensure(nslots);
      s_trn.ensure(nslots);
    }
    PhotonBuf PB{{qr0.p, qr1.p}, {qh0.p, qh1.p}, {qi0.p, qi1.p}, pcol.p, pfl.p, s_flag.p,
                 s_pos.p, s_wi.p, s_col.p, s_nrm.p, s_refl.p, s_trn.p};
    // words: [0, kAccWords) trace accumulators, then MB + 2 queue words, then 128 per trace launch
    DBuf<unsigned long long> words;
    const size_t nw = kAccWords + (size_t)(MB + 2) + 128 * (size_t)(MB + 1);
    words.ensure(nw);
    HIPCHK(hipMemsetAsync(words.p, 0, nw * sizeof(unsigned long long), P.stream));
    HIPCHK(hipMemsetAsync(s_flag.p, 0, nslots, P.stream));
    unsigned long long* qwd = words.p + kAccWords;
    launch(shade_kernels(d).photon_emit, grid_for(N, YK_APPEND_BLOCK), YK_APPEND_BLOCK, 0, P.stream, C, PB, qwd);
    int qin = 1;
    for (int b = 0; b <= MB; ++b) {
      unsigned long long* work = words.p + kAccWords + (MB + 2) + 128ll * b;
      enqueue_trace<true>(d, P, ray_src(PB.q_rays[qin]), nullptr, RayCount{qwd + b, 32, 0}, PB.q_hits[qin], nullptr, work,
                          words.p, nullptr, nullptr);
      launch(shade_kernels(d).photon_hit, grid_for(N, YK_APPEND_BLOCK), YK_APPEND_BLOCK, 0, P.stream, d->S, C, PB, b, qwd + b,
             qin, qwd + b + 1);
      qin ^= 1;
    }
    unsigned long long acc[kAccWords];
    HIPCHK(hipMemcpyAsync(acc, words.p, sizeof acc, hipMemcpyDeviceToHost, P.stream));
    o.flag.resize(nslots);
    o.pos.resize(nslots);
    o.wi.resize(nslots);
    o.col.resize(nslots);
    HIPCHK(hipMemcpyAsync(o.flag.data(), s_flag.p, nslots, hipMemcpyDeviceToHost, P.stream));
    HIPCHK(hipMemcpyAsync(o.pos.data(), s_pos.p, nslots * sizeof(float4), hipMemcpyDeviceToHost, P.stream));
    HIPCHK(hipMemcpyAsync(o.wi.data(), s_wi.p, nslots * sizeof(float4), hipMemcpyDeviceToHost, P.stream));
    HIPCHK(hipMemcpyAsync(o.col.data(), s_col.p, nslots * sizeof(float4), hipMemcpyDeviceToHost, P.stream));
    if (rad) {
      o.nrm.resize(nslots);
      o.refl.resize(nslots);
      o.trn.resize(nslots);
      HIPCHK(hipMemcpyAsync(o.nrm.data(), s_nrm.p, nslots * sizeof(float4), hipMemcpyDeviceToHost, P.stream));
      HIPCHK(hipMemcpyAsync(o.refl.data(), s_refl.p, nslots * sizeof(float4), hipMemcpyDeviceToHost, P.stream));
      HIPCHK(hipMemcpyAsync(o.trn.data(), s_trn.p, nslots * sizeof(float4), hipMemcpyDeviceToHost, P.stream));
    }
    HIPCHK(hipStreamSynchronize(P.stream));
    if (acc[2]) throw watchdog_error("kd-tree traversal watchdog fired during photon tracing");
    photon_rays += acc[3];
  };
  PassOut dpass;
  if (!pt) run_pass(N, 0, dpass);
  // caustic pass (photonintegr.cc:316-460): every light shoots caustic photons
  // (light_t::shootsCausticP); a photon turns caustic only after a SPECULAR
  // sample, so without such a component the pass stores nothing and is skipped
  bool any_specular = false;
  for (int m = 0; m < kMaxMats && m < (int)d->mat_flags.size(); ++m)
    any_specular |= (d->mat_flags[m] & (BSDF_SPECULAR | BSDF_GLOSSY)) != 0;
  PassOut cpass;
  if (q.caustic_photons > 0 && any_specular && nL > 0) run_pass((unsigned)q.caustic_photons, pt ? 2 : 1, cpass);
  auto t1 = std::chrono::steady_clock::now();
  const std::vector<uint8_t>& hflag = dpass.flag;
  const std::vector<float4>&hpos = dpass.pos, &hwi = dpass.wi, &hcol = dpass.col, &hnrm = dpass.nrm,
                       &hrefl = dpass.refl, &htrn = dpass.trn;
  const size_t nslots = hflag.size();

  // ---- photon vector in the reference's push order (path, then bounce), and
  // the radiance points: one ourRandom() per diffuse hit (photonintegr.cc:272-291)
  std::vector<float>& dm = d->dm_host;
  dm.clear();
  int dpaths = 0, seed = q.seed;
  std::vector<float> rpos, rnrm, rrefl, rtrn;  // 3 floats each per candidate
  for (size_t s = 0; s < nslots; ++s) {
    const uint8_t f = hflag[s];
    if (!f) continue;
    if (f & 2) {
      const float v[9] = {hpos[s].x, hpos[s].y, hpos[s].z, hwi[s].x, hwi[s].y, hwi[s].z, hcol[s].x, hcol[s].y, hcol[s].z};
      dm.insert(dm.end(), v, v + 9);
      dpaths = (int)(s / (size_t)(MB + 1));
    }
    if (q.final_gather && our_random(seed) < 0.125 && (f & 2)) {
      const float4 a = hpos[s], n = hnrm[s], r = hrefl[s], t = htrn[s];
      rpos.insert(rpos.end(), {a.x, a.y, a.z});
      rnrm.insert(rnrm.end(), {n.x, n.y, n.z});
      rrefl.insert(rrefl.end(), {r.x, r.y, r.z});
      rtrn.insert(rtrn.end(), {t.x, t.y, t.z});
    }
  }
  const int ndm = (int)(dm.size() / 9);
  const int ncand = (int)(rpos.size() / 3);
  if (!pt && ndm < 50) return set_error(YK_ERR_STATE, "photon mapping: too few diffuse photons (< 50)");
  d->dm_paths = dpaths;
  PointTree dtree;
  if (!pt) {
    point_tree_build(dm.data(), 9, ndm, dtree);
    if (dtree.depth > kMaxPointTreeDepth) return set_error(YK_ERR_UNSUPPORTED, "diffuse photon tree too deep");
    upload_map(d, YK_PHOTON_MAP_DIFFUSE, dm, dtree);
  }
  // caustic map, same push order
  std::vector<float>& cm = d->cm_host;
  cm.clear();
  int cpaths = 0;
  for (size_t s = 0; s < cpass.flag.size(); ++s) {
    if (!(cpass.flag[s] & 2)) continue;
    const float4 a = cpass.pos[s], w = cpass.wi[s], c = cpass.col[s];
    const float v[9] = {a.x, a.y, a.z, w.x, w.y, w.z, c.x, c.y, c.z};
    cm.insert(cm.end(), v, v + 9);
    cpaths = (int)(s / (size_t)(MB + 1));
  }
  d->cm_paths = cpaths;
  int cdepth = 0;
  if (!cm.empty()) {
    PointTree ctree;
    point_tree_build(cm.data(), 9, (int)(cm.size() / 9), ctree);
    if (ctree.depth > kMaxPointTreeDepth) return set_error(YK_ERR_UNSUPPORTED, "caustic photon tree too deep");
    cdepth = ctree.depth;
    upload_map(d, YK_PHOTON_MAP_CAUSTIC, cm, ctree);
  }

  // ---- radiance map: eliminate close points, pre-gather on the device
  std::vector<float>& rm = d->rm_host;
  rm.clear();
  int rdepth = 0;
  double ms_pre = 0.0;
  if (q.final_gather && !pt) {
    PointTree rt;
    point_tree_build(rpos.data(), 3, ncand, rt);
    std::vector<uint8_t> use(ncand, 1);
    std::vector<int> cleaned;
    const float maxrad = 0.01f * q.diffuse_radius;
    for (int i = 0; i < ncand; ++i) {
      if (!use[i]) continue;
      cleaned.push_back(i);
      const float* ni = &rnrm[3 * (size_t)i];
      auto elim = [&](int k, float, float&) {  // eliminatePhoton_t, photon.h:179-187
        const float* nk = &rnrm[3 * (size_t)k];
        if (nk[0] * ni[0] + nk[1] * ni[1] + nk[2] * ni[2] > 0.f) use[k] = 0;
      };
      float md = maxrad;
      point_tree_lookup(rt, rpos.data(), 3, &rpos[3 * (size_t)i], elim, md);
    }
    const int nr = (int)cleaned.size();
    if (nr == 0) return set_error(YK_ERR_STATE, "photon mapping: no radiance points");
    std::vector<float4> cp(nr), cn(nr), cr(nr), ct(nr);
    for (int j = 0; j < nr; ++j) {
      const size_t i = 3 * (size_t)cleaned[j];
      cp[j] = make_float4(rpos[i], rpos[i + 1], rpos[i + 2], 0.f);
      cn[j] = make_float4(rnrm[i], rnrm[i + 1], rnrm[i + 2], 0.f);
      cr[j] = make_float4(rrefl[i], rrefl[i + 1], rrefl[i + 2], 0.f);
      ct[j] = make_float4(rtrn[i], rtrn[i + 1], rtrn[i + 2], 0.f);
    }
    DBuf<float4> dp, dn, dr, dt, dc;
    dp.ensure(nr);
    dn.ensure(nr);
    dr.ensure(nr);
    dt.ensure(nr);
    dc.ensure(nr);
    HIPCHK(hipMemcpy(dp.p, cp.data(), nr * sizeof(float4), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dn.p, cn.data(), nr * sizeof(float4), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dr.p, cr.data(), nr * sizeof(float4), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dt.p, ct.data(), nr * sizeof(float4), hipMemcpyHostToDevice));
    const PMapDev dmap{d->dm_nodes.p, d->dm_pos.p, d->dm_dir.p, d->dm_col.p, ndm};
    const float iscale = (float)(1.0 / ((double)(float)dpaths * YK_PI_D));
    auto tp = std::chrono::steady_clock::now();
    launch(k_pregather, grid_for(nr, 64), 64, 0, P.stream, dmap, dp.p, dn.p, dr.p, dt.p, nr,
           q.diffuse_radius * q.diffuse_radius, iscale, q.search, dc.p);
    std::vector<float4> col(nr);
    HIPCHK(hipMemcpyAsync(col.data(), dc.p, nr * sizeof(float4), hipMemcpyDeviceToHost, P.stream));
    HIPCHK(hipStreamSynchronize(P.stream));
    ms_pre = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tp).count();
    rm.resize(9 * (size_t)nr);
    for (int j = 0; j < nr; ++j) {
      const float v[9] = {cp[j].x, cp[j].y, cp[j].z, cn[j].x, cn[j].y, cn[j].z, col[j].x, col[j].y, col[j].z};
      std::memcpy(&rm[9 * (size_t)j], v, sizeof v);
    }
    PointTree rtree;
    point_tree_build(rm.data(), 9, nr, rtree);
    if (rtree.depth > kMaxPointTreeDepth) return set_error(YK_ERR_UNSUPPORTED, "radiance photon tree too deep");
    rdepth = rtree.depth;
    d->rm_depth = rtree.depth;
    d->rm_nnodes = rtree.nodes.size() / 2;
    upload_map(d, YK_PHOTON_MAP_RADIANCE, rm, rtree);
    if (lookup_lds(d)) {  // resident lookup waves with this tree's LDS stack
      int blocks = 0;
      HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, k_pm_lookup<true>, 64, lookup_lds_bytes(d->rm_depth)));
      d->per_cu_lookup[1] = std::max(1, blocks);
    }
  }
  d->pm_params = q;
  d->pm_integrator = p->integrator;
  d->pm_ready = true;
  if (info) {
    *info = yk_photon_info{};
    info->diffuse_photons = ndm;
    info->diffuse_paths = dpaths;
    info->caustic_photons = (int)(cm.size() / 9);
    info->caustic_paths = cpaths;
    info->rad_candidates = ncand;
    info->radiance_photons = (int)(rm.size() / 9);
    info->seed_out = seed;
    info->tree_depth = std::max(std::max(dtree.depth, rdepth), cdepth);
    info->photon_rays = photon_rays;
    info->ms_shoot = std::chrono::duration<double, std::milli>(t1 - t0).count();
    info->ms_pregather = ms_pre;
    info->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    info->ms_tree = info->ms_total - info->ms_shoot - ms_pre;
  }
  return YK_OK;
  YK_GUARD_END
}

int yk_photon_export(yk_device* d, int32_t which, float* out, int32_t cap, int32_t* n_out) {
  if (!d || !n_out) return set_error(YK_ERR_ARG, "yk_photon_export: NULL argument");
  if (which != YK_PHOTON_MAP_DIFFUSE && which != YK_PHOTON_MAP_CAUSTIC && which != YK_PHOTON_MAP_RADIANCE)
    return set_error(YK_ERR_ARG, "yk_photon_export: unknown map");
  const std::vector<float>& v =
      which == YK_PHOTON_MAP_DIFFUSE ? d->dm_host : (which == YK_PHOTON_MAP_RADIANCE ? d->rm_host : d->cm_host);
  const int n = (int)(v.size() / 9);
  *n_out = n;
  if (out && cap > 0) std::memcpy(out, v.data(), (size_t)std::min(n, cap) * 9 * sizeof(float));
  return YK_OK;
}

}  // extern "C"
