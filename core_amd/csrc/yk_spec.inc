// Specular recursion on gfx950 (included by yk_device.hip inside namespace
// yk, after the shading kernels): the node store of the recursion's
// generations and the kernels k_finish_spec, k_spawn and k_fold. Depends on
// yk_device.hip's records and constant memory (c_mats), its materials
// (make_surface, face_forward, mat_fresnel, glass_alpha, mat_specular), its batch records
// (Batch, RenderConst, the PH_* flags) and put_ray.

// ------------------------------------------------------------ specular recursion
//
// mcIntegrator_t::recursiveRaytrace (mcintegrator.cc:421-627) calls the
// integrator again for the mirror and refraction rays of a specular hit, up
// to raydepth levels. Here every such call is an entry ("node") of a later
// generation: generation g holds the rays of recursion level g, shaded by the
// same kernels as camera rays. Each node keeps its own terms (emission,
// direct light, path estimate) and its children; k_fold then sums every
// camera sample's tree in the reference's order. state.includeLights is
// shared by the recursive calls, and lightMat_t::emit reads it, so a node's
// emission is only added at the fold, where the value left by the previous
// sibling's subtree is known (pathtracer.cc:149-152,220,264; directlight.cc
// restores it on return).

enum : int { NF_HIT = 1, NF_LIGHT = 2, NF_LOOP = 4, NF_LOOPT = 8, NF_SPEC = 16 };

struct NodeStore {
  float* E;      // 3 per node: emission at the node's hit (includeLights = true)
  float* D;      // 3 per node: direct light (or background on a miss)
  float* P;      // 3 per node: pathCol / nSamples (path tracer)
  int* flags;    // NF_*
  int* child;    // 2 per node: reflect, refract (-1 none)
  float* rcol;   // 6 per node: getSpecular colours of the two children
  float* alpha;  // camera nodes
  yk_ray* ray;   // rays of nodes of generation >= 1 (by node id)
  unsigned* soffs;
  unsigned* psample;
  unsigned long long* count;  // allocated node ids
  long long cap;
  int* overflow;
  float* malpha;  // photon mapping: material_t::getAlpha at the node's hit (1 unless transparent)
};

// Terms of the n entries of one chunk (node ids base..base+n-1).
__global__ void __launch_bounds__(256) k_finish_spec(Batch B, RenderConst R, NodeStore NS, long long base,
                                                     long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long long node = base + i;
  const int ph = B.prim_hit[i];
  const bool loop = R.integrator == YK_INTEGRATOR_PATH && (ph & PH_DIFFUSE);
  c3 P = C3(0.f, 0.f, 0.f);
  if (loop) {
    const float ns = (float)R.nsub;
    P = C3(B.pathcol[3 * i] / ns, B.pathcol[3 * i + 1] / ns, B.pathcol[3 * i + 2] / ns);
  }
  int f = 0;
  if (ph & PH_HIT) f |= NF_HIT;
  if (ph & PH_LIGHT) f |= NF_LIGHT;
  if (loop) f |= NF_LOOP | (B.incl[i] ? NF_LOOPT : 0);
  NS.flags[node] = f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    NS.E[3 * node + k] = (ph & PH_HIT) ? B.emit0[3 * i + k] : 0.f;
    NS.D[3 * node + k] = B.col[3 * i + k];
  }
  NS.P[3 * node] = P.r;
  NS.P[3 * node + 1] = P.g;
  NS.P[3 * node + 2] = P.b;
  NS.child[2 * node] = -1;
  NS.child[2 * node + 1] = -1;
  NS.malpha[node] = 1.f;
  if (R.level == 0) NS.alpha[node] = B.alpha[i];
}

// recursiveRaytrace's specular block for the hits of one chunk: allocate the
// reflect / refract children (rays from sp.P, tmin MIN_RAYDIST, unbounded).
// GL: as in the shading kernels (a coated glossy material's getSpecular).
template <int GL = kGLNone>
__global__ void __launch_bounds__(256) k_spawn(DScene S, Batch B, RenderConst R, NodeStore NS, long long base,
                                               long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !(B.prim_hit[i] & PH_HIT)) return;
  const int lv = R.level + 1;  // state.raylevel++
  if (lv > R.rdepth || lv >= 20) return;
  const yk_hit h = B.p_hits[i];
  const yk_ray r = B.p_rays[i];
  const v3 from = V3(r.from[0], r.from[1], r.from[2]), dir = V3(r.dir[0], r.dir[1], r.dir[2]);
  const SurfPt sp = make_surface(S, from, dir, h);
  const DMat& M = c_mats[sp.mat];
  if (!(M.flags & (BSDF_SPECULAR | BSDF_FILTER))) return;
  const long long node = base + i;
  NS.flags[node] |= NF_SPEC;
  bool glass = false;
  if constexpr (GL >= kGLGlass) glass = M.type == YK_MAT_GLASS;
  if (glass) {  // glassMat_t::getAlpha, whether or not it fakes shadows
    if (R.integrator == YK_INTEGRATOR_PHOTON) NS.malpha[node] = glass_alpha(M, sp, vneg(dir));
  } else if (R.integrator == YK_INTEGRATOR_PHOTON && (M.flags & BSDF_FILTER)) {
    // shinyDiffuseMat_t::getAlpha (shinydiffuse.cc:457-469) of a transparent material
    const v3 wo = vneg(dir);
    const float Kr = mat_fresnel(M, wo, face_forward(sp.Ng, sp.N, wo));
    const float refl = (1.f - M.comp[0] * Kr) * M.comp[1];
    NS.malpha[node] = 1.f - refl;
  }
  bool refl, refr;
  v3 d[2];
  c3 col[2];
  mat_specular<GL>(M, sp, vneg(dir), refl, refr, d, col, lv);
  const bool want[2] = {refl, refr};
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    if (!want[k]) continue;
    const unsigned long long id = atomicAdd(NS.count, 1ull);
    if ((long long)id >= NS.cap) {
      *NS.overflow = 1;
      continue;
    }
    NS.child[2 * node + k] = (int)id;
    NS.rcol[6 * node + 3 * k] = col[k].r;
    NS.rcol[6 * node + 3 * k + 1] = col[k].g;
    NS.rcol[6 * node + 3 * k + 2] = col[k].b;
    put_ray(NS.ray[id], sp.P, d[k], YK_MIN_RAYDIST, -1.0f);
    NS.soffs[id] = B.soffs[i];
    NS.psample[id] = B.psample[i];
  }
}

// Sums each camera sample's node tree depth first, in the reference's order:
// col = (emit + direct) + path; col += child_r * rcol0; col += child_t * rcol1.
__global__ void __launch_bounds__(256) k_fold(Batch B, RenderConst R, NodeStore NS, long long nc) {
  const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  constexpr int kMaxLevel = 22;
  int nodes[kMaxLevel], stage[kMaxLevel];
  c3 acc[kMaxLevel];
  float alp[kMaxLevel];  // photon mapping: integrate()'s alpha, set by the refract child
  const bool pt = R.integrator == YK_INTEGRATOR_PATH, pm = R.integrator == YK_INTEGRATOR_PHOTON;
  const float a_init = R.transp_bg ? 0.f : 1.f;
  float result_alpha = 0.f;
  bool e = true;  // state.includeLights
  int dd = 0;
  nodes[0] = (int)c;
  stage[0] = 0;
  c3 result = C3(0.f, 0.f, 0.f);
  for (;;) {
    const int n = nodes[dd];
    const int F = NS.flags[n];
    if (stage[dd] == 0) {
      c3 col = C3(NS.D[3 * n], NS.D[3 * n + 1], NS.D[3 * n + 2]);
      if (F & NF_HIT) {
        if (dd == 0) e = true;  // raylevel 0: includeLights = true
        const bool incl = pt ? e : true;
        const c3 E = ((F & NF_LIGHT) && !incl) ? C3(0.f, 0.f, 0.f)
                                               : C3(NS.E[3 * n], NS.E[3 * n + 1], NS.E[3 * n + 2]);
        col = cadd(E, col);
        col = cadd(col, C3(NS.P[3 * n], NS.P[3 * n + 1], NS.P[3 * n + 2]));
        if (pt && (F & NF_LOOP)) e = (F & NF_LOOPT) != 0;
        if (F & NF_SPEC) e = true;
      }
      acc[dd] = col;
      alp[dd] = a_init;
      stage[dd] = 1;
      const int ch = (F & NF_HIT) ? NS.child[2 * n] : -1;
      if (ch >= 0 && dd + 1 < kMaxLevel) {
        ++dd;
        nodes[dd] = ch;
        stage[dd] = 0;
        continue;
      }
    }
    if (stage[dd] == 1) {
      stage[dd] = 2;
      const int ch = (F & NF_HIT) ? NS.child[2 * n + 1] : -1;
      if (ch >= 0 && dd + 1 < kMaxLevel) {
        ++dd;
        nodes[dd] = ch;
        stage[dd] = 0;
        continue;
      }
    }
    const c3 v = acc[dd];
    // photonintegr.cc:862-866: alpha = m_alpha + (1 - m_alpha) * alpha on a hit
    const float m = NS.malpha[n];
    const float va = (F & NF_HIT) ? m + (1.f - m) * alp[dd] : a_init;
    if (dd == 0) {
      result = v;
      result_alpha = va;
      break;
    }
    --dd;
    const int pn = nodes[dd];
    const int k = stage[dd] - 1;
    if (k == 1) alp[dd] = va;  // recursiveRaytrace: alpha = integ.A of the refracted ray
    const float* rc = NS.rcol + 6 * pn + 3 * k;
    acc[dd] = cadd(acc[dd], C3(v.r * rc[0], v.g * rc[1], v.b * rc[2]));
  }
  B.samples[c] = make_float4(result.r, result.g, result.b, pm ? result_alpha : NS.alpha[c]);
}
