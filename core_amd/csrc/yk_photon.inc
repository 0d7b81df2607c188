// Photon mapping on gfx950 (included by yk_device.hip inside namespace yk).
//
//   photonIntegrator_t::preprocess   photonintegr.cc:126-633
//     photon paths                   k_photon_emit / k_photon_hit (the
//                                    closest-hit kernel traces every segment)
//     preGatherWorker_t::body        k_pregather
//   photonIntegrator_t::integrate    photonintegr.cc:792-882: k_pm_post
//     finalGathering                 photonintegr.cc:637-790: k_fg_start,
//                                    k_fg_hit, k_fg_resolve
//   photonMap_t::gather/findNearest  photon.cc:115-129 over
//   kdtree::pointKdTree::lookup      pkdtree.h:180-236: pt_lookup
//
// The photon kd-trees are built on the host (photon_map.cpp) in the
// reference's node layout; the gather heap restates libstdc++'s
// make_heap / pop_heap / push_heap (bits/stl_heap.h) because the heap layout
// is the order gathered photons are summed in.

struct PMapDev {  // one photon map: pointKdTree nodes + photon_t fields
  const uint2* nodes;  // w0 split bits / photon index (leaf), w1 axis | right << 2, 3 = leaf
  const float4* pos;
  const float4* dir;
  const float4* col;
  int n;
  const uint4* pk;  // radiance map only: 16-B nodes, {split, -, -, axis | right << 2} or {pos xyz, 3 | photon << 2}
};

constexpr int kPStack = 48;      // point-tree depth bound (checked on the host)
constexpr int kMaxSearch = 256;  // "search" bound of the device gather heap

// pointKdTree::lookup, NON_REC_LOOKUP form. Stack entries: far child | axis
// << 30, split bits. proc(i, dist2, maxd2) may lower maxd2.
struct ScratchStack {  // per-thread private array (scratch memory)
  uint2 s[kPStack];
  __device__ __forceinline__ void put(int i, uint2 e) { s[i] = e; }
  __device__ __forceinline__ uint2 get(int i) const { return s[i]; }
};
constexpr int kLdsPStack = 16;  // LDS stack entries per lane (k_fg_hit, trees of depth <= 16)
struct LdsStack {  // entry i of this lane at base[i * blockDim + lane]: no bank conflicts
  uint2* base;
  int lane, stride;
  __device__ __forceinline__ void put(int i, uint2 e) { base[i * stride + lane] = e; }
  __device__ __forceinline__ uint2 get(int i) const { return base[i * stride + lane]; }
};

// One iteration of the lookup loop: descend from `cur` to a leaf (pushing
// the far children), process the leaf, pop the first stack entry whose plane
// lies within sqrt(maxd2). Returns false when the stack ran empty (the lookup
// is finished), else leaves the popped far child in `cur`.
template <class Proc, class Stk>
__device__ __forceinline__ bool pt_lookup_step(const PMapDev& M, v3 p, Proc& proc, float& maxd2, Stk& stack,
                                               int& cur, int& sp) {
  uint2 nd = M.nodes[cur];
  while ((nd.y & 3u) != 3u) {
    const uint32_t axis = nd.y & 3u;
    const float split = __uint_as_float(nd.x);
    const int right = (int)(nd.y >> 2);
    int farc;
    if (sel3(p, axis) <= split) {
      farc = right;
      cur = cur + 1;
    } else {
      farc = cur + 1;
      cur = right;
    }
    stack.put(sp++, make_uint2((uint32_t)farc | (axis << 30), nd.x));
    nd = M.nodes[cur];
  }
  const int d = (int)nd.x;
  const float4 q = M.pos[d];
  const float vx = q.x - p.x, vy = q.y - p.y, vz = q.z - p.z;
  float dist2 = vx * vx + vy * vy + vz * vz;
  if (dist2 < maxd2) proc(d, dist2, maxd2);
  if (sp == 0) return false;
  uint2 e = stack.get(sp - 1);
  dist2 = sel3(p, e.x >> 30) - __uint_as_float(e.y);
  dist2 *= dist2;
  while (dist2 > maxd2) {
    --sp;
    if (sp == 0) return false;
    e = stack.get(sp - 1);
    dist2 = sel3(p, e.x >> 30) - __uint_as_float(e.y);
    dist2 *= dist2;
  }
  cur = (int)(e.x & 0x3FFFFFFFu);
  --sp;
  return true;
}
// pt_lookup_step over the 16-B nodes (PMapDev::pk), for k_pm_lookup: the
// same decisions and float operations, with a leaf's photon position read
// from the leaf itself (one dependent load less per leaf visit), and stack
// entries of (far child, squared plane distance): the distance is computed
// at the push with the expression the pop would evaluate on the same inputs,
// so it is the same float, and an entry takes 6 B of LDS (16-bit child
// index) instead of 8.
template <typename I>
struct FarStackLds {  // entry i of lane l at [i * 64 + l]
  I* farc;
  float* dd;
  int lane;
  __device__ __forceinline__ void put(int i, int f, float d) {
    farc[i * 64 + lane] = (I)f;
    dd[i * 64 + lane] = d;
  }
  __device__ __forceinline__ int far_at(int i) const { return (int)farc[i * 64 + lane]; }
  __device__ __forceinline__ float dd_at(int i) const { return dd[i * 64 + lane]; }
};
struct FarStackScratch {
  int farc[kPStack];
  float dd[kPStack];
  __device__ __forceinline__ void put(int i, int f, float d) {
    farc[i] = f;
    dd[i] = d;
  }
  __device__ __forceinline__ int far_at(int i) const { return farc[i]; }
  __device__ __forceinline__ float dd_at(int i) const { return dd[i]; }
};
template <class Proc, class Stk>
__device__ __forceinline__ bool pt_lookup_step_pk(const PMapDev& M, v3 p, Proc& proc, float& maxd2, Stk& stack,
                                                  int& cur, int& sp) {
  uint4 nd = M.pk[cur];
  while ((nd.w & 3u) != 3u) {
    const uint32_t axis = nd.w & 3u;
    const float split = __uint_as_float(nd.x);
    const int right = (int)(nd.w >> 2);
    int farc;
    if (sel3(p, axis) <= split) {
      farc = right;
      cur = cur + 1;
    } else {
      farc = cur + 1;
      cur = right;
    }
    float dd = sel3(p, axis) - split;
    dd *= dd;
    stack.put(sp++, farc, dd);
    nd = M.pk[cur];
  }
  const int d = (int)(nd.w >> 2);
  const float vx = __uint_as_float(nd.x) - p.x, vy = __uint_as_float(nd.y) - p.y, vz = __uint_as_float(nd.z) - p.z;
  const float dist2 = vx * vx + vy * vy + vz * vz;
  if (dist2 < maxd2) proc(d, dist2, maxd2);
  if (sp == 0) return false;
  while (stack.dd_at(sp - 1) > maxd2) {
    --sp;
    if (sp == 0) return false;
  }
  cur = stack.far_at(sp - 1);
  --sp;
  return true;
}
template <class Proc, class Stk>
__device__ __forceinline__ void pt_lookup_s(const PMapDev& M, v3 p, Proc& proc, float& maxd2, Stk& stack) {
  int sp = 0, cur = 0;
  while (pt_lookup_step(M, p, proc, maxd2, stack, cur, sp)) {
  }
}
template <class Proc>
__device__ __forceinline__ void pt_lookup(const PMapDev& M, v3 p, Proc& proc, float& maxd2) {
  ScratchStack stk;
  pt_lookup_s(M, p, proc, maxd2, stk);
}

// nearestPhoton_t, photon.h:167-176
struct NearestProc {
  const float4* dir;
  v3 n;
  int nearest;
  __device__ __forceinline__ void operator()(int d, float dist2, float& maxd2) {
    const float4 w = dir[d];
    if (w.x * n.x + w.y * n.y + w.z * n.z > 0.f) {
      nearest = d;
      maxd2 = dist2;
    }
  }
};

__device__ __forceinline__ int pm_nearest(const PMapDev& M, v3 p, v3 n, float dist) {
  NearestProc pr{M.dir, n, -1};
  pt_lookup(M, p, pr, dist);
  return pr.nearest;
}
struct PFound {  // foundPhoton_t: photon index + distSquare, ordered by distSquare
  int idx;
  float d2;
};

// std::__adjust_heap + std::__push_heap (libstdc++ bits/stl_heap.h), less on d2
__device__ __forceinline__ void heap_push_up(PFound* f, int hole, int top, PFound v) {
  int parent = (hole - 1) / 2;
  while (hole > top && f[parent].d2 < v.d2) {
    f[hole] = f[parent];
    hole = parent;
    parent = (hole - 1) / 2;
  }
  f[hole] = v;
}
__device__ __forceinline__ void heap_adjust(PFound* f, int hole, int len, PFound v) {
  const int top = hole;
  int child = hole;
  while (child < (len - 1) / 2) {
    child = 2 * (child + 1);
    if (f[child].d2 < f[child - 1].d2) child--;
    f[hole] = f[child];
    hole = child;
  }
  if ((len & 1) == 0 && child == (len - 2) / 2) {
    child = 2 * (child + 1);
    f[hole] = f[child - 1];
    hole = child - 1;
  }
  heap_push_up(f, hole, top, v);
}
__device__ __forceinline__ void heap_make(PFound* f, int len) {  // std::make_heap
  if (len < 2) return;
  for (int parent = (len - 2) / 2;; --parent) {
    heap_adjust(f, parent, len, f[parent]);
    if (parent == 0) return;
  }
}

// photonGather_t::operator(), photon.cc:53-73
struct GatherProc {
  PFound* f;
  int k, n;
  __device__ __forceinline__ void operator()(int d, float dist2, float& maxd2) {
    if (n < k) {
      f[n].idx = d;
      f[n].d2 = dist2;
      ++n;
      if (n == k) {
        heap_make(f, k);
        maxd2 = f[0].d2;
      }
    } else {
      if (k > 1) {  // std::pop_heap
        const PFound last = f[k - 1];
        f[k - 1] = f[0];
        heap_adjust(f, 0, k - 1, last);
      }
      const PFound v{d, dist2};  // std::push_heap of the new last element
      heap_push_up(f, k - 1, 0, v);
      maxd2 = f[0].d2;
    }
  }
};

__device__ __forceinline__ int pm_gather(const PMapDev& M, v3 p, PFound* f, int K, float& sqRadius) {
  GatherProc g{f, K, 0};
  pt_lookup(M, p, g, sqRadius);
  return g.n;
}


// ------------------------------------------------------------ photon paths

struct PhotonConst {
  unsigned nphotons;
  int nlights;
  float fnum_lights, inv_photons, inv_integral;
  float func[kMaxLights];
  float cdf[kMaxLights + 1];
  int max_bounces;
  int final_gather;
  int caustic_pass;  // 0: diffuse map (photonintegr.cc:219-314), 1: caustic map (:316-460),
                     // 2: pathIntegrator_t's caustic map (mcIntegrator_t::createCausticMap,
                     // mcintegrator.cc:197-377)
};

struct PhotonBuf {
  yk_ray* q_rays[2];
  yk_hit* q_hits[2];
  unsigned* q_id[2];  // photon index (curr) of each queue entry
  float* pcol;        // 3 per photon: the path colour
  uint8_t* pfl;       // per photon: 1 causticPhoton, 2 directPhoton
  // deposit slot curr * (max_bounces + 1) + bounce
  uint8_t* s_flag;    // 1 diffuse hit (one ourRandom() call), 2 stored in the diffuse map
  float4* s_pos;
  float4* s_wi;
  float4* s_col;
  float4* s_nrm;      // radData_t normal: FACE_FORWARD(Ng, N, wi)
  float4* s_refl;     // getReflectivity(DIFFUSE|GLOSSY|REFLECT)
  float4* s_trn;      // getReflectivity(DIFFUSE|GLOSSY|TRANSMIT)
};

// material_t::getReflectivity, material.cc:48-66
template <int GL = kGLNone>
__device__ __forceinline__ c3 get_reflectivity(const DMat& M, const SurfPt& sp, unsigned flags) {
  if (!(flags & (BSDF_TRANSMIT | BSDF_REFLECT) & M.flags)) return C3(0.f, 0.f, 0.f);
  float W = 0.f;
  c3 total = C3(0.f, 0.f, 0.f);
  for (int i = 0; i < 16; ++i) {
    const float s1 = (float)(0.03125 + 0.0625 * (double)(float)i);
    const float s2 = ri_vdc((unsigned)i, 0u);
    const float s3 = (float)scr_halton(2, (unsigned)i);
    const float s4 = (float)scr_halton(3, (unsigned)i);
    const v3 wo = sample_cos_hemisphere(sp.N, sp.NU, sp.NV, s1, s2);
    v3 wi = V3(0.f, 0.f, 0.f);
    float pdf;
    bool ok;
    const c3 col = mat_sample<false, GL>(M, sp, wo, wi, s3, s4, flags, pdf, W, ok);
    total = cadd(total, C3(col.r * W, col.g * W, col.b * W));
  }
  return C3(total.r * 0.0625f, total.g * 0.0625f, total.b * 0.0625f);
}

__device__ __forceinline__ float cmax3(c3 c) {  // color_t::maximum
  const float gb = (c.g < c.b) ? c.b : c.g;
  return (c.r < gb) ? gb : c.r;
}

__device__ __forceinline__ void store4(float4* p, v3 v) { *p = make_float4(v.x, v.y, v.z, 0.f); }
__device__ __forceinline__ void store4(float4* p, c3 v) { *p = make_float4(v.r, v.g, v.b, 0.f); }


// minRot, sample_utils.h:168-176, as written: U2 = cosAlpha*U + (1.f-cosAlpha) * (v*U) + sinAlpha * (v^U),
// where v*U is the dot product, so the middle term is a float: it becomes
// vector3d_t(PFLOAT) (vector3d.h:57) and is added to all three components.
// sinAlpha = fSqrt(1 - cosAlpha*cosAlpha) is NaN where rounding puts
// cosAlpha a little above 1; it is kept (a NaN frame gives a NaN origin).
__device__ __forceinline__ void min_rot(v3 D, v3 U, v3 D2, v3& U2, v3& V2) {
  const float cosAlpha = vdot(D, D2);
  const float sinAlpha = sqrtf(1.f - cosAlpha * cosAlpha);
  const v3 v = vcross(D, D2);
  const float m = (1.f - cosAlpha) * vdot(v, U);
  const v3 w = vcross(v, U);
  U2 = V3((cosAlpha * U.x + m) + sinAlpha * w.x, (cosAlpha * U.y + m) + sinAlpha * w.y,
          (cosAlpha * U.z + m) + sinAlpha * w.z);
  V2 = vcross(D2, U2);
}

// light_t::emitPhoton of the lights that photon maps take: the ray, ipdf and
// the returned colour. XL == kXLSun adds sunLight_t::emitPhoton (sunlight.cc:
// 97-112) as written: the disk point and the cone direction both come from
// s3, s4 (s1, s2 are unused), the disk is carried by minRot's frame around
// ldir, and the colour is colPdf * ePdf.
template <int XL>
__device__ __forceinline__ c3 emit_photon(const DLight& L, float s1, float s2, float s3, float s4, v3& from, v3& dir,
                                          float& ipdf) {
  if (XL >= kXLSun && L.type == YK_LIGHT_SUN) {
    float u, v;
    shirley_disk(s3, s4, u, v);
    const v3 ldir = sample_cone(ld3(L.dir), ld3(L.du), ld3(L.dv), (float)sun_cos_angle(L), s3, s4);
    v3 du2, dv2;
    min_rot(ld3(L.dir), ld3(L.du), ldir, du2, dv2);
    ipdf = L.invpdf;
    const v3 off = vadd(vadd(vmul(u, du2), vmul(v, dv2)), ldir);
    from = vadd(ld3(L.epos), vmul(L.wradius, off));
    dir = vneg(ldir);
    return C3(L.color[0] * L.epdf, L.color[1] * L.epdf, L.color[2] * L.epdf);
  }
  if (L.type == YK_LIGHT_DIRECTIONAL) {  // directionalLight_t::emitPhoton, directional.cc:106-116
    dir = vneg(ld3(L.dir));
    float u, v;
    shirley_disk(s1, s2, u, v);
    const v3 off = vadd(vmul(u, ld3(L.edu)), vmul(v, ld3(L.edv)));
    from = vadd(ld3(L.epos), vmul(L.eradius, off));
    if (L.infinite) from = vadd(from, vmul(L.wradius, ld3(L.dir)));
    ipdf = (float)(YK_PI_D * (double)L.eradius * (double)L.eradius);
  } else if (L.type == YK_LIGHT_POINT) {  // pointLight_t::emitPhoton + SampleSphere (sample_utils.h:54-72)
    from = ld3(L.pos);
    dir.z = 1.0f - 2.0f * s1;
    float rr = 1.0f - dir.z * dir.z;
    if (rr > 0.0f) {
      rr = sqrtf(rr);
      const float a = (float)(YK_2PI_D * (double)s2);
      dir.x = fcos_ref(a) * rr;
      dir.y = fsin_ref(a) * rr;
    } else {
      dir.x = 0.0f;
      dir.y = 0.0f;
    }
    ipdf = (float)(4.0 * YK_PI_D);
  } else {  // areaLight_t::emitPhoton, arealight.cc:98-104
    ipdf = L.area;
    from = vadd(vadd(ld3(L.corner), vmul(s3, ld3(L.toX))), vmul(s4, ld3(L.toY)));
    dir = sample_cos_hemisphere(ld3(L.normal), ld3(L.du), ld3(L.dv), s1, s2);
  }
  return C3(L.color[0], L.color[1], L.color[2]);
}

// Photon emission for photon `curr` (photonintegr.cc:224-246): QMC numbers,
// pdf1D_t::DSample light choice, light_t::emitPhoton, colour scaling.
// XL: kXLNone, or kXLSun for scenes that hold a sun (emit_photon).
template <int XL = kXLNone>
__global__ void __launch_bounds__(YK_APPEND_BLOCK) k_photon_emit(PhotonConst PC, PhotonBuf PB, unsigned long long* qword) {
  const unsigned curr = blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = curr < PC.nphotons;
  bool emit = false;
  yk_ray r;
  if (valid) {
    const float s1 = ri_vdc(curr, 0u), s2 = (float)scr_halton(2, curr), s3 = (float)scr_halton(3, curr),
                s4 = (float)scr_halton(4, curr);
    // createCausticMap divides (mcintegrator.cc:258), photonintegr.cc multiplies
    const float sL = PC.caustic_pass == 2 ? (float)curr / (float)PC.nphotons : (float)curr * PC.inv_photons;
    int ln = 0;
    if (sL != 0.f) {  // std::lower_bound over cdf[0..n]
      int k = 0;
      while (k < PC.nlights + 1 && PC.cdf[k] < sL) ++k;
      ln = k - 1 < 0 ? 0 : k - 1;
    }
    if (ln >= PC.nlights) ln = PC.nlights - 1;  // host checks that this never happens
    const float lightNumPdf = PC.func[ln] * PC.inv_integral;
    const DLight& L = c_lights[ln];
    v3 from, dir;
    float ipdf;
    const c3 ecol = emit_photon<XL>(L, s1, s2, s3, s4, from, dir, ipdf);
    const float k = (PC.fnum_lights * ipdf) / lightNumPdf;
    const c3 pcol = C3(ecol.r * k, ecol.g * k, ecol.b * k);
    if (!cblack(pcol)) {
      emit = true;
      PB.pcol[3 * (size_t)curr] = pcol.r;
      PB.pcol[3 * (size_t)curr + 1] = pcol.g;
      PB.pcol[3 * (size_t)curr + 2] = pcol.b;
      PB.pfl[curr] = 2;  // directPhoton
      put_ray(r, from, dir, YK_MIN_RAYDIST, -1.0f);
    }
  }
  unsigned sb, q;
  wave_append2<YK_PM_APPEND_WAVE>(qword, 0u, emit ? 1u : 0u, sb, q);
  if (emit) {
    PB.q_rays[1][q] = r;
    PB.q_id[1][q] = curr;
  }
}

// One hit of every live photon path (photonintegr.cc:256-314): deposit on a
// diffuse surface, radiance-point data, and scatterPhoton for the next segment.
// GL (here and below): the scene holds a glossy material, as in the shading kernels.
template <int GL = kGLNone>
__global__ void __launch_bounds__(YK_APPEND_BLOCK) k_photon_hit(DScene S, PhotonConst PC, PhotonBuf PB, int bounce,
                                                    const unsigned long long* __restrict__ in_w, int qin,
                                                    unsigned long long* __restrict__ out_w) {
  const long long nq = (long long)(*in_w >> 32);
  if ((long long)blockIdx.x * blockDim.x >= nq) return;
  const long long qi = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = qi < nq;
  bool emit = false;
  yk_ray nxt;
  unsigned curr = 0;
  if (valid) {
    curr = PB.q_id[qin][qi];
    const yk_hit h = PB.q_hits[qin][qi];
    if (h.prim >= 0) {
      const yk_ray r = PB.q_rays[qin][qi];
      const v3 from = V3(r.from[0], r.from[1], r.from[2]), dir = V3(r.dir[0], r.dir[1], r.dir[2]);
      const SurfPt sp = make_surface(S, from, dir, h);
      const DMat& M = c_mats[sp.mat];
      const v3 wi = vneg(dir);
      const size_t pc3 = 3 * (size_t)curr;
      c3 pcol = C3(PB.pcol[pc3], PB.pcol[pc3 + 1], PB.pcol[pc3 + 2]);
      const uint8_t fl = PB.pfl[curr];
      const bool caustic = (fl & 1) != 0;
      bool direct = (fl & 2) != 0;
      if (PC.caustic_pass == 2) {  // deposit on DIFFUSE | GLOSSY (mcintegrator.cc:309-318)
        if ((M.flags & (BSDF_DIFFUSE | BSDF_GLOSSY)) && caustic) {
          const size_t slot = (size_t)curr * (PC.max_bounces + 1) + bounce;
          PB.s_flag[slot] = 2;
          store4(&PB.s_pos[slot], sp.P);
          store4(&PB.s_wi[slot], wi);
          store4(&PB.s_col[slot], pcol);
        }
      } else if (M.flags & BSDF_DIFFUSE) {
        // diffuse pass: every diffuse hit draws one ourRandom() (bit 0), non-caustic
        // photons are stored (bit 1); caustic pass: caustic photons are stored
        const size_t slot = (size_t)curr * (PC.max_bounces + 1) + bounce;
        PB.s_flag[slot] = PC.caustic_pass ? (caustic ? 2 : 0) : (caustic ? 1 : 3);
        store4(&PB.s_pos[slot], sp.P);
        store4(&PB.s_wi[slot], wi);
        store4(&PB.s_col[slot], pcol);
        if (PC.final_gather && !caustic && !PC.caustic_pass) {
          store4(&PB.s_nrm[slot], face_forward(sp.Ng, sp.N, wi));
          store4(&PB.s_refl[slot], get_reflectivity<GL>(M, sp, BSDF_DIFFUSE | BSDF_GLOSSY | BSDF_REFLECT));
          store4(&PB.s_trn[slot], get_reflectivity<GL>(M, sp, BSDF_DIFFUSE | BSDF_GLOSSY | BSDF_TRANSMIT));
        }
      }
      if (bounce < PC.max_bounces) {
        const int d5 = 3 * bounce + 5;
        const float s5 = (float)scr_halton(d5, curr), s6 = (float)scr_halton(d5 + 1, curr),
                    s7 = (float)scr_halton(d5 + 2, curr);
        // material_t::scatterPhoton, material.cc:29-46 (alpha = transm = 1)
        float W = 0.f, pdf = 0.f;
        bool ok;
        unsigned sfl;
        v3 wo = V3(0.f, 0.f, 0.f);
        // createCausticMap samples only BSDF_ALL_SPECULAR | GLOSSY | FILTER | DISPERSIVE
        const unsigned sflags = PC.caustic_pass == 2 ? (BSDF_SPECULAR | BSDF_REFLECT | BSDF_TRANSMIT | BSDF_GLOSSY |
                                                        BSDF_FILTER | BSDF_DISPERSIVE)
                                                     : BSDF_ALL;
        const c3 scol = mat_sample<false, GL>(M, sp, wi, wo, s5, s6, sflags, pdf, W, ok, sfl);
        if (pdf > 1.0e-6f) {
          c3 cnew = cmul(cmul(pcol, C3(1.f, 1.f, 1.f)), scol);
          cnew = C3(cnew.r * W, cnew.g * W, cnew.b * W);
          const float q = cmax3(cnew) / cmax3(pcol);
          const float prob = (q < 1.f) ? q : 1.f;
          if (s7 <= prob && prob > 1e-4f) {
            pcol = C3(cnew.r / prob, cnew.g / prob, cnew.b / prob);
            const bool nc = ((sfl & (BSDF_GLOSSY | BSDF_SPECULAR | BSDF_DISPERSIVE)) && direct) ||
                            ((sfl & (BSDF_GLOSSY | BSDF_SPECULAR | BSDF_FILTER | BSDF_DISPERSIVE)) && caustic);
            direct = (sfl & BSDF_FILTER) && direct;
            // the caustic-only pass stops once a photon is neither caustic nor direct
            if (PC.caustic_pass != 2 || nc || direct) {
              PB.pcol[pc3] = pcol.r;
              PB.pcol[pc3 + 1] = pcol.g;
              PB.pcol[pc3 + 2] = pcol.b;
              PB.pfl[curr] = (uint8_t)((nc ? 1 : 0) | (direct ? 2 : 0));
              put_ray(nxt, sp.P, wo, YK_MIN_RAYDIST, -1.0f);
              emit = true;
            }
          }
        }
      }
    }
  }
  unsigned sb, qn;
  wave_append2<YK_PM_APPEND_WAVE>(out_w, 0u, emit ? 1u : 0u, sb, qn);
  if (emit) {
    PB.q_rays[qin ^ 1][qn] = nxt;
    PB.q_id[qin ^ 1][qn] = curr;
  }
}

// preGatherWorker_t::body, photonintegr.cc:50-96: radiance of each kept
// radiance point from its nSearch nearest diffuse photons.
__global__ void __launch_bounds__(64) k_pregather(PMapDev dmap, const float4* __restrict__ rp_pos,
                                                  const float4* __restrict__ rp_nrm, const float4* __restrict__ rp_refl,
                                                  const float4* __restrict__ rp_trn, int n, float ds_radius2,
                                                  float iscale, int K, float4* __restrict__ out_col) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  PFound f[kMaxSearch];
  const float4 p4 = rp_pos[i], n4 = rp_nrm[i];
  const v3 p = V3(p4.x, p4.y, p4.z), rn = V3(n4.x, n4.y, n4.z);
  float radius = ds_radius2;
  const int ng = pm_gather(dmap, p, f, K, radius);
  c3 sum = C3(0.f, 0.f, 0.f);
  if (ng > 0) {
    const float scale = iscale / radius;
    const float4 rf = rp_refl[i], tr = rp_trn[i];
    for (int k = 0; k < ng; ++k) {
      const int d = f[k].idx;
      const float4 w = dmap.dir[d], c = dmap.col[d];
      const bool front = rn.x * w.x + rn.y * w.y + rn.z * w.z > 0.f;
      const float4 s = front ? rf : tr;
      sum = cadd(sum, cmul(C3(s.x * scale, s.y * scale, s.z * scale), C3(c.x, c.y, c.z)));
    }
  }
  out_col[i] = make_float4(sum.r, sum.g, sum.b, 0.f);
}

// ------------------------------------------------------------ integrate

struct PMConst {
  PMapDev dmap, rmap, cmap;
  int final_gather, show_map;
  int search;
  int fg_bounces;
  int dpaths;  // diffuseMap.nPaths()
  float gather_dist, lookup_rad, ds_radius;
  int caustic_mix;  // nCausSearch
  int cpaths;       // causticMap.nPaths()
  float caus_radius;
};

// photonIntegrator_t::integrate after estimateAllDirectLight
// (photonintegr.cc:819-866): show_map lookups and the direct diffuse-map
// estimate of the non-final-gather mode.
template <int GL = kGLNone>
__global__ void __launch_bounds__(64) k_pm_post(DScene S, Batch B, PMConst PM, long long nc) {
  const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const int ph = B.prim_hit[c];
  if (!(ph & PH_HIT)) return;
  if (!PM.show_map && !(ph & PH_DIFFUSE)) return;
  const yk_ray r = B.p_rays[c];
  const v3 from = V3(r.from[0], r.from[1], r.from[2]), dir = V3(r.dir[0], r.dir[1], r.dir[2]);
  const SurfPt sp = make_surface(S, from, dir, B.p_hits[c]);
  const v3 wo = vneg(dir);
  c3 col = C3(B.col[3 * c], B.col[3 * c + 1], B.col[3 * c + 2]);
  if (PM.show_map) {
    const v3 N = face_forward(sp.Ng, sp.N, wo);
    const PMapDev& map = PM.final_gather ? PM.rmap : PM.dmap;
    const int nr = pm_nearest(map, sp.P, N, PM.final_gather ? PM.lookup_rad : PM.ds_radius);
    if (nr >= 0) {
      const float4 pc = map.col[nr];
      col = cadd(col, C3(pc.x, pc.y, pc.z));
    }
  } else {
    PFound f[kMaxSearch];
    float radius = PM.ds_radius;  // "actually the square radius"
    const int ng = PM.dmap.n > 0 ? pm_gather(PM.dmap, sp.P, f, PM.search, radius) : 0;
    if (ng > 0) {
      const float scale = (float)(1.0 / ((double)((float)PM.dpaths * radius) * YK_PI_D));
      const DMat& M = c_mats[sp.mat];
      for (int k = 0; k < ng; ++k) {
        const int d = f[k].idx;
        const float4 w = PM.dmap.dir[d], pc = PM.dmap.col[d];
        const c3 surf = mat_eval<true, GL>(M, sp, wo, V3(w.x, w.y, w.z));
        col = cadd(col, cmul(C3(surf.r * scale, surf.g * scale, surf.b * scale), C3(pc.x, pc.y, pc.z)));
      }
    }
  }
  B.col[3 * c] = col.r;
  B.col[3 * c + 1] = col.g;
  B.col[3 * c + 2] = col.b;
}

// final-gather path state bits (pstate), next to PS_*
enum : int { FG_ADD = 16, FG_EMIT = 32, FG_CAUS = 64, FG_SPECF = 128 };

// "Zero'th" FG bounce of gather path isub (photonintegr.cc:660-684): sample
// the camera hit's BSDF; a black weight skips the path.
template <bool DIFF, int GL = kGLNone>
__global__ void __launch_bounds__(YK_APPEND_BLOCK) k_fg_start(DScene S, Batch B, RenderConst R, long long nc, int isub,
                                                  float* __restrict__ fg_lcol, unsigned long long* __restrict__ qword) {
  const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = c < nc;
  bool emit = false;
  yk_ray r;
  if (valid && (B.prim_hit[c] & PH_DIFFUSE)) {
    const yk_hit h = B.p_hits[c];
    const yk_ray pr = B.p_rays[c];
    const v3 from = V3(pr.from[0], pr.from[1], pr.from[2]), dir = V3(pr.dir[0], pr.dir[1], pr.dir[2]);
    const SurfPt sp = make_surface(S, from, dir, h);
    const unsigned s = R.ps ? B.psample[c] : (unsigned)c % (unsigned)R.spp;
    const unsigned offs = (unsigned)(R.nsub * (int)s) + B.soffs[c] + (unsigned)isub;
    const float s1 = ri_vdc(offs, 0u);
    const float s2 = (float)scr_halton(2, offs);
    float pdf, W = B.wlast[c];
    bool ok;
    v3 pdir = V3(0.f, 0.f, 0.f);
    c3 scol = mat_sample<DIFF, GL>(c_mats[sp.mat], sp, vneg(dir), pdir, s1, s2, BSDF_DIFFUSE | BSDF_REFLECT | BSDF_TRANSMIT,
                               pdf, W, ok);
    B.wlast[c] = W;
    scol = C3(scol.r * W, scol.g * W, scol.b * W);
    B.pstate[c] = 0;
    if (!cblack(scol)) {
      B.thr[3 * c] = scol.r;
      B.thr[3 * c + 1] = scol.g;
      B.thr[3 * c + 2] = scol.b;
      fg_lcol[3 * c] = 0.f;
      fg_lcol[3 * c + 1] = 0.f;
      fg_lcol[3 * c + 2] = 0.f;
      put_ray(r, sp.P, pdir, YK_MIN_RAYDIST, -1.0f);
      emit = true;
    }
  }
  unsigned sb, q;
  wave_append2<YK_PM_APPEND_WAVE>(qword, 0u, emit ? 1u : 0u, sb, q);
  if (emit) {
    B.q_rays[1][q] = r;
    B.q_owner[1][q] = (int)c;
  }
}

// Hit `it` of a gather path (photonintegr.cc:686-777). it = 0 is the hit of
// the zero'th segment; loop iteration `depth = it` runs while it < fg_bounces
// and do_bounce, otherwise the path ends here with the radiance-map lookup
// of the did_hit tail. Shadow rays of estimateOneDirectLight and the next
// segment go to the queues, and so do the radiance-map lookups (query point,
// normal, owner: k_pm_lookup runs them); k_fg_resolve adds lcol * throughput.
#ifndef YK_FG_WAVES_D
#define YK_FG_WAVES_D 1  // occupancy target of the diffuse-only k_fg_hit (1: the compiler's choice)
#endif
// XL: kXLNone, or kXLSun for scenes that hold a sun, the one light beyond the
// area, point and directional lights that yk_photon_build accepts (gen_light).
template <bool DIFF, int GL = kGLNone, int XL = kXLNone>
__global__ void __launch_bounds__(YK_APPEND_BLOCK) __attribute__((amdgpu_waves_per_eu(DIFF ? YK_FG_WAVES_D : 1)))
k_fg_hit(DScene S, Batch B, RenderConst R, PMConst PM,
                                                const unsigned long long* __restrict__ qin_word, int it, int isub,
                                                int qin, float* __restrict__ fg_lcol, float* __restrict__ fg_len,
                                                unsigned long long* __restrict__ qword, float4* __restrict__ lq,
                                                unsigned long long* __restrict__ lword) {
  const long long nq = (long long)(*qin_word >> 32);
  const long long qb = (long long)blockIdx.x * blockDim.x;
  if (qb >= nq) return;
  const long long qi = qb + threadIdx.x;
  bool valid = qi < nq;
  {  // escaped gather paths end first (packing the block's hits as in
     // k_shade_bounce measured 1490 against 1560 Mrays/s, and packing the
     // radiance lookups 1478 against 1581: the lookup loop diverges by its
     // own length, not by idle lanes)
    const int prim = valid ? B.q_hits[qin][qi].prim : 0;
    if (valid && prim < 0) {  // background: the path ends (a caustic segment adds the background first)
      const long long c = B.q_owner[qin][qi];
      if (it > 0 && (B.pstate[c] & FG_CAUS) && R.has_bg) {
        const c3 bg = R.has_bg == kBgGradient ? bg_gradient(R.bg_grad, ld3(B.q_rays[qin][qi].dir)) : C3(R.bg[0], R.bg[1], R.bg[2]);
        B.pathcol[3 * c] = B.pathcol[3 * c] + B.thr[3 * c] * bg.r;
        B.pathcol[3 * c + 1] = B.pathcol[3 * c + 1] + B.thr[3 * c + 1] * bg.g;
        B.pathcol[3 * c + 2] = B.pathcol[3 * c + 2] + B.thr[3 * c + 2] * bg.b;
      }
      B.pstate[c] = 0;
    }
    valid = valid && prim >= 0;
  }
  const long long c = valid ? B.q_owner[qin][qi] : 0;
  int nr = 0, kend = 0;
  unsigned long long traced = 0;
  bool emit_next = false;
  yk_ray nxt;
  bool look = false;  // a radiance-map lookup at (lp, ln) for this path
  v3 lp = V3(0.f, 0.f, 0.f), ln = lp;
  if (valid) {
    const yk_hit h = B.q_hits[qin][qi];
    int ps = B.pstate[c];
    bool caustic = (ps & FG_CAUS) != 0;
    {
      const yk_ray pr = B.q_rays[qin][qi];
      const v3 from = V3(pr.from[0], pr.from[1], pr.from[2]), dir = V3(pr.dir[0], pr.dir[1], pr.dir[2]);
      const SurfPt sp = make_surface(S, from, dir, h);
      const DMat& M = c_mats[sp.mat];
      float length;
      bool do_bounce;
      if (it == 0) {
        length = h.t;
        caustic = false;
        do_bounce = (length < PM.gather_dist) || (M.flags & BSDF_SPECULAR);
      } else {
        length = fg_len[c] + h.t;
        caustic = (caustic || it == 1) && (ps & FG_SPECF);
        do_bounce = caustic || (length < PM.gather_dist);
      }
      const bool close = length < PM.gather_dist;
      fg_len[c] = length;
      ps = PS_RESOLVE | (caustic ? FG_CAUS : 0);
      const v3 pwo = vneg(dir);
      if (it < PM.fg_bounces && do_bounce) {
        const unsigned s = R.ps ? B.psample[c] : (unsigned)c % (unsigned)R.spp;
        const unsigned offs = (unsigned)(R.nsub * (int)s) + B.soffs[c] + (unsigned)isub;
        if (M.flags & BSDF_DIFFUSE) {
          if (close) {
            if (R.nlights > 0) {  // estimateOneDirectLight(state, hit, pwo, offs)
              Halton h2;
              hal_start(h2, 2u, (unsigned)((int)offs - 1));
              int lnum = (int)(hal_next(h2) * (float)R.nlights);
              if (lnum > R.nlights - 1) lnum = R.nlights - 1;
              nr = gen_light<DIFF, XL, GL>(B, c, 0, lnum, sp, pwo, s, B.soffs[c], (unsigned)lnum, traced, c_mats, S.ml);
              kend = c_lights[lnum].nslots;
              if (nr) put_org(B, c, sp.P);
              B.lsel[c] = lnum;
              ps |= PS_EST;
            } else {
              fg_lcol[3 * c] = 0.f;
              fg_lcol[3 * c + 1] = 0.f;
              fg_lcol[3 * c + 2] = 0.f;
            }
          } else if (caustic) {
            look = true;
            lp = sp.P;
            ln = face_forward(sp.Ng, sp.N, pwo);
          }
          if (close || caustic) {
            ps |= FG_ADD;
            if (M.flags & BSDF_EMIT) {
              const c3 em = mat_emit(M, sp, pwo, false);
              B.emit_b[3 * c] = em.r;
              B.emit_b[3 * c + 1] = em.g;
              B.emit_b[3 * c + 2] = em.b;
              ps |= FG_EMIT;
            }
          }
        }
        const int d4 = 4 * it;
        const float s1 = (float)scr_halton(d4 + 3, offs);
        const float s2 = (float)scr_halton(d4 + 4, offs);
        float pdf, W = B.wlast[c];
        bool ok;
        v3 ndir = dir;
        unsigned sfl;
        const unsigned fl = close ? BSDF_ALL : (BSDF_SPECULAR | BSDF_REFLECT | BSDF_TRANSMIT | BSDF_FILTER);
        c3 sc = mat_sample<DIFF, GL>(M, sp, pwo, ndir, s1, s2, fl, pdf, W, ok, sfl);
        B.wlast[c] = W;
        if (pdf > 1.0e-6f) {
          sc = C3(sc.r * W, sc.g * W, sc.b * W);
          B.scol_next[3 * c] = sc.r;
          B.scol_next[3 * c + 1] = sc.g;
          B.scol_next[3 * c + 2] = sc.b;
          if (sfl & (BSDF_SPECULAR | BSDF_FILTER)) ps |= FG_SPECF;
          put_ray(nxt, sp.P, ndir, YK_MIN_RAYDIST, -1.0f);
          emit_next = true;
          ps |= PS_CONT;
        }
      } else if (M.flags & (BSDF_DIFFUSE | BSDF_GLOSSY)) {  // did_hit tail: radiance map at the path end
        look = true;
        lp = sp.P;
        ln = face_forward(sp.Ng, sp.N, pwo);
        ps |= FG_ADD;
        if (M.flags & BSDF_EMIT) {
          const c3 em = mat_emit(M, sp, pwo, false);
          B.emit_b[3 * c] = em.r;
          B.emit_b[3 * c + 1] = em.g;
          B.emit_b[3 * c + 2] = em.b;
          ps |= FG_EMIT;
        }
      }
      B.pstate[c] = ps;
    }
  }
  unsigned sbase, qn;
  wave_append2<YK_PM_APPEND_WAVE>(qword, valid ? (unsigned)nr : 0u, emit_next ? 1u : 0u, sbase, qn);
  if (valid) flush_shadow(B, c, kend, nr, sbase, traced);
  if (emit_next) {
    B.q_rays[qin ^ 1][qn] = nxt;
    B.q_owner[qin ^ 1][qn] = (int)c;
  }
  unsigned lb, lb_hi;
  if (!YK_PM_APPEND_WAVE) __syncthreads();  // the block append's LDS words are reused
  wave_append2<YK_PM_APPEND_WAVE>(lword, look ? 1u : 0u, 0u, lb, lb_hi);
  if (look) {
    lq[2 * (size_t)lb] = make_float4(lp.x, lp.y, lp.z, __int_as_float((int)c));
    lq[2 * (size_t)lb + 1] = make_float4(ln.x, ln.y, ln.z, 0.f);
  }
}

// Radiance-map lookups of the final-gather paths (photonMap_t::findNearest,
// photon.cc:115-129, over pointKdTree::lookup, pkdtree.h:180-236) as a
// persistent kernel. Run inside k_fg_hit, a wave's lookups were one
// divergent loop that lasted as long as its longest query: on the headline
// scene's radiance map (4152 photons) a lookup visits 129 nodes on average,
// a wave's longest about 4x that. Here every lane of a resident wave runs
// one query at a time and takes the next from a wave-private pool of the
// queue once a quarter of the wave is idle, so lanes stay busy until the
// queue drains. Each lane makes the reference's serial decisions
// (pt_lookup_step: near-first descent, the same pruning, nearestPhoton_t's
// strict improvement), so the photon found is the per-thread lookup's; only
// the lane a query runs on differs. A found photon's colour becomes the
// owner's lcol; none leaves lcol as it was, as in the reference.
// LDS: the stack lives in dynamic LDS, depth x 64 entries of 16-bit child
// index + float (trees of < 2^16 nodes; sized by the tree's depth at launch).
template <bool LDS>
__global__ void __launch_bounds__(64) k_pm_lookup(PMapDev M, float rad2, int depth, const float4* __restrict__ lq,
                                                  const unsigned long long* __restrict__ lword,
                                                  float* __restrict__ fg_lcol, unsigned long long* __restrict__ work) {
  extern __shared__ float lds_dd[];
  const long long n = (long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)*lword);
  if ((long long)blockIdx.x * 64 >= n + 63) return;  // waves a small queue cannot fill
  const int lane = threadIdx.x;
  // ~8 chunks per wave, at least 64 queries each
  const unsigned chunk = (unsigned)__builtin_amdgcn_readfirstlane(
      (int)max(64u, (unsigned)(n / ((long long)gridDim.x * 8)) & ~63u));
  std::conditional_t<LDS, FarStackLds<unsigned short>, FarStackScratch> stk;
  if constexpr (LDS) stk = FarStackLds<unsigned short>{reinterpret_cast<unsigned short*>(lds_dd + depth * 64), lds_dd, lane};
  unsigned pool_next = 0, pool_end = 0;
  bool drained = false;  // wave-uniform: the queue has no chunks left
  bool exhausted = false;
  int c = -1;  // owner of this lane's query; -1 idle
  v3 p = V3(0.f, 0.f, 0.f);
  NearestProc pr{M.dir, p, -1};
  float maxd2 = 0.f;
  int cur = 0, sp = 0;
  for (;;) {
    const unsigned long long want = __ballot(c < 0 && !exhausted);
    const unsigned long long act = __ballot(c >= 0);
    if (want != 0ull && (act == 0ull || __popcll(want) >= 16)) {
      const unsigned cnt = (unsigned)__popcll(want);
      const unsigned avail = pool_end - pool_next;
      unsigned cb = 0, ce = 0;
      if (avail < cnt && !drained) {
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(work, (unsigned long long)chunk);
        base = shfl_u64(base, 0);
        if (base < (unsigned long long)n) {
          cb = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)base);
          ce = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)min(base + chunk, (unsigned long long)n));
        } else {
          drained = true;
        }
      }
      if (c < 0 && !exhausted) {
        const unsigned rank = __builtin_amdgcn_mbcnt_hi((unsigned)(want >> 32),
                                                         __builtin_amdgcn_mbcnt_lo((unsigned)want, 0u));
        long long q = -1;
        if (rank < avail) q = pool_next + rank;
        else if (rank - avail < ce - cb) q = cb + (rank - avail);
        if (q < 0) {
          exhausted = drained;
        } else {
          const float4 a = lq[2 * q], b = lq[2 * q + 1];
          p = V3(a.x, a.y, a.z);
          c = __float_as_int(a.w);
          pr.n = V3(b.x, b.y, b.z);
          pr.nearest = -1;
          maxd2 = rad2;
          cur = 0;
          sp = 0;
        }
      }
      if (avail < cnt) {
        pool_next = cb + min(cnt - avail, ce - cb);
        pool_end = ce;
      } else {
        pool_next += cnt;
      }
      pool_next = (unsigned)__builtin_amdgcn_readfirstlane((int)pool_next);
      pool_end = (unsigned)__builtin_amdgcn_readfirstlane((int)pool_end);
    }
    if (__ballot(c >= 0) == 0ull) {
      if (__ballot(!exhausted) == 0ull) break;
      continue;
    }
    if (c >= 0 && !pt_lookup_step_pk(M, p, pr, maxd2, stk, cur, sp)) {
      if (pr.nearest >= 0) {
        const float4 pc = M.col[pr.nearest];
        fg_lcol[3 * (size_t)c] = pc.x;
        fg_lcol[3 * (size_t)c + 1] = pc.y;
        fg_lcol[3 * (size_t)c + 2] = pc.z;
      }
      c = -1;
    }
  }
}

// pathCol += lcol * throughput; throughput *= scol (photonintegr.cc:705-745)
__global__ void __launch_bounds__(256) k_fg_resolve(Batch B, RenderConst R,
                                                    const unsigned long long* __restrict__ qin_word, int qin,
                                                    float* __restrict__ fg_lcol) {
  const long long nq = (long long)(*qin_word >> 32);
  const long long qi = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (qi >= nq) return;
  const long long c = B.q_owner[qin][qi];
  const int ps = B.pstate[c];
  if (!(ps & PS_RESOLVE)) return;
  c3 lcol = C3(fg_lcol[3 * c], fg_lcol[3 * c + 1], fg_lcol[3 * c + 2]);
  if (ps & PS_EST) lcol = cscale((float)R.nlights, resolve_light(B, c, 0, B.lsel[c]));
  if (ps & FG_ADD) {
    if (ps & FG_EMIT) lcol = cadd(lcol, C3(B.emit_b[3 * c], B.emit_b[3 * c + 1], B.emit_b[3 * c + 2]));
    const c3 thr = C3(B.thr[3 * c], B.thr[3 * c + 1], B.thr[3 * c + 2]);
    B.pathcol[3 * c] = B.pathcol[3 * c] + lcol.r * thr.r;
    B.pathcol[3 * c + 1] = B.pathcol[3 * c + 1] + lcol.g * thr.g;
    B.pathcol[3 * c + 2] = B.pathcol[3 * c + 2] + lcol.b * thr.b;
  }
  fg_lcol[3 * c] = lcol.r;
  fg_lcol[3 * c + 1] = lcol.g;
  fg_lcol[3 * c + 2] = lcol.b;
  if (ps & PS_CONT) {
    B.thr[3 * c] = B.thr[3 * c] * B.scol_next[3 * c];
    B.thr[3 * c + 1] = B.thr[3 * c + 1] * B.scol_next[3 * c + 1];
    B.thr[3 * c + 2] = B.thr[3 * c + 2] * B.scol_next[3 * c + 2];
    B.pstate[c] = ps & (FG_CAUS | FG_SPECF);
  } else {
    B.pstate[c] = 0;
  }
}

// mcIntegrator_t::estimateCausticPhotons (mcintegrator.cc:384-419, kernel()
// sample_utils.h:27-31) at the hit of entry c; the caller checks
// causticMap.ready() (cmap.n > 0).
template <int GL = kGLNone>
__device__ __forceinline__ c3 caustic_estimate(const DScene& S, const Batch& B, const PMConst& PM, long long c) {
  const yk_ray r = B.p_rays[c];
  const v3 from = V3(r.from[0], r.from[1], r.from[2]), dir = V3(r.dir[0], r.dir[1], r.dir[2]);
  const SurfPt sp = make_surface(S, from, dir, B.p_hits[c]);
  const v3 wo = vneg(dir);
  PFound f[kMaxSearch];
  float g = PM.caus_radius * PM.caus_radius;
  const int ng = pm_gather(PM.cmap, sp.P, f, PM.caustic_mix, g);
  g = 1.f / g;
  c3 sum = C3(0.f, 0.f, 0.f);
  if (ng > 0) {
    const DMat& M = c_mats[sp.mat];
    for (int k = 0; k < ng; ++k) {
      const int d = f[k].idx;
      const float4 w = PM.cmap.dir[d], pc = PM.cmap.col[d];
      const c3 surf = mat_eval<true, GL>(M, sp, wo, V3(w.x, w.y, w.z));
      const float s = 1.f - f[k].d2 * g;
      const float kk = (float)((((double)(3.f * g) * YK_1_PI_D) * (double)s) * (double)s);
      sum = cadd(sum, cmul(C3(surf.r * kk, surf.g * kk, surf.b * kk), C3(pc.x, pc.y, pc.z)));
    }
    const float inv = 1.f / (float)PM.cpaths;
    sum = C3(sum.r * inv, sum.g * inv, sum.b * inv);
  }
  return sum;
}

// col += finalGathering (pathCol / nSampl) and col += estimateCausticPhotons
// in the order photonIntegrator_t::integrate adds them (photonintegr.cc:827-852).
template <int GL = kGLNone>
__global__ void __launch_bounds__(64) k_pm_finish(DScene S, Batch B, RenderConst R, PMConst PM, long long nc) {
  const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc || !(B.prim_hit[c] & PH_DIFFUSE)) return;
  c3 col = C3(B.col[3 * c], B.col[3 * c + 1], B.col[3 * c + 2]);
  if (R.pm_fg) {
    const float ns = (float)R.nsub;
    col = cadd(col, C3(B.pathcol[3 * c] / ns, B.pathcol[3 * c + 1] / ns, B.pathcol[3 * c + 2] / ns));
  }
  if (PM.cmap.n > 0) col = cadd(col, caustic_estimate<GL>(S, B, PM, c));  // causticMap.ready()
  B.col[3 * c] = col.r;
  B.col[3 * c + 1] = col.g;
  B.col[3 * c + 2] = col.b;
}

// pathIntegrator_t::integrate with caustic_type photon / both: col +=
// estimateCausticPhotons right after estimateAllDirectLight on a diffuse hit
// (pathtracer.cc:168-172), before the path samples are added.
template <int GL = kGLNone>
__global__ void __launch_bounds__(64) k_pt_caustic(DScene S, Batch B, PMConst PM, long long nc) {
  const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc || !(B.prim_hit[c] & PH_DIFFUSE)) return;
  const c3 sum = caustic_estimate<GL>(S, B, PM, c);
  B.col[3 * c] = B.col[3 * c] + sum.r;
  B.col[3 * c + 1] = B.col[3 * c + 1] + sum.g;
  B.col[3 * c + 2] = B.col[3 * c + 2] + sum.b;
}
