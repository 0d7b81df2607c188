// kd-tree traversal on gfx950 (included by yk_device.hip inside namespace yk,
// after its records): the tree-bound test, the per-lane exit stack
// (LaneStackT), the descent and leaf helpers (trav_begin, trav_descend,
// trav_next, coop_leaves, lane_leaves, trav_step), the node packets
// (k_pack_nodes, k_gather_leaf_tris), the small scenes' LDS layout, the ray
// hand-out (RaySrc, RayCount), trace_body, the list
// YK_TRACE_VARIANTS and the k_trace_* kernels. Its host counterpart is
// yk_trace_host.inc. Depends on yk_math.h, yk_api.h (yk_ray, yk_hit) and the
// records ahead of it in yk_device.hip: DScene, DMat (c_mats), SurfPt, ld_tri
// and kTriWords. One forward dependency: trav_step's transparent shadows call
// mat_transparency and make_surface, which the materials of yk_device.hip's
// shading section define; they are declared here ahead of leaf_test.

// ============================================================ traversal

// bound_t::cross (Smits), compiled form: ((a1-a0)-p)*inv evaluates as (a1-from)*inv
// inv: 1/dir per axis, the traversal's own invDir (bound.h computes the same
// float 1.0/dir on every axis it uses), so each ray divides three times, not six
__device__ __forceinline__ bool bound_cross(const float* bb, v3 from, v3 dir, v3 inv, float& enter, float& leave,
                                            float dist) {
  float lmin = -1e38f, lmax = 1e38f;
  const float o[3] = {from.x, from.y, from.z}, d[3] = {dir.x, dir.y, dir.z}, iv[3] = {inv.x, inv.y, inv.z};
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) {
    if (d[ax] != 0.f) {
      const float invr = iv[ax];
      const float t0 = (bb[ax] - o[ax]) * invr, t1 = (bb[3 + ax] - o[ax]) * invr;
      const float ltmin = invr > 0.f ? t0 : t1, ltmax = invr > 0.f ? t1 : t0;
      if (ax == 0) {
        lmin = ltmin;
        lmax = ltmax;
      } else {
        lmin = (ltmin < lmin) ? lmin : ltmin;
        lmax = (lmax < ltmax) ? lmax : ltmax;
      }
      if ((lmax < 0.f) || (lmin > dist)) return false;
    }
  }
  if ((lmin <= lmax) && (lmax >= 0.f) && (lmin <= dist)) {
    enter = lmin;
    leave = lmax;
    return true;
  }
  return false;
}

// Exit-point stack. The reference keeps {node*, t, pb[3], prev} per entry
// (kdtree.h:103-109); exits form a LIFO (prev links). Here the current entry
// and exit live in registers and older exits on a per-lane stack of 8-byte
// entries {split, far node | axis<<30}. On pop, t is recomputed with the
// push-time expression (split - from[axis]) * invDir[axis] and pb as
// pb[axis] = split, other axes from + t*dir -- the same float operations on
// the same inputs, so bit-identical. Axis code 3 is the initial exit, whose
// entry stores t itself. The top kStackLds entries of every lane live in an
// LDS ring; deeper ones spill to a global overflow area (rare: a 1M-tri tree
// has depth ~40 but a ray rarely holds more than a dozen pending exits).
#ifndef YK_STACK_LDS
#define YK_STACK_LDS 8
#endif
constexpr int kStackLds = YK_STACK_LDS;  // LDS ring depth per lane (16 measured slower: 1807 vs 2054, round 1)
#ifndef YK_STACK_LDS_C
#define YK_STACK_LDS_C YK_STACK_LDS
#endif
constexpr int kStackLdsC = YK_STACK_LDS_C;  // the closest-hit kernels' ring (any depth: not a power of two -> mod)
// The diagnostic build's (-DYK_TRAV_STATS) counters, behind this one
// conditional: trace_body and LaneStackT::push call TravStats where they
// count, and in the default build every call is empty. kAccWords: accumulator
// words per traversal kernel kind ({nodes, triangle tests, errors, rays}; the
// diagnostic build adds its own, ctr[4..12], which launch_trace prints).
#ifdef YK_TRAV_STATS
constexpr int kAccWords = 16;
__device__ unsigned long long g_spill_stores[1];
struct TravStats {
  enum Phase { kRefill, kDescend, kLeaf, kPop };
  // wave iterations, active lanes per iteration, wave-level
  // descent / leaf-loop trips (max over lanes), refills
  unsigned long long s_it = 0, s_act = 0, s_dmax = 0, s_lmax = 0, s_refill = 0;
  // cycles per phase (clock64 deltas, wave-uniform): refill, descent, leaf test, pop
  unsigned long long c_ref = 0, c_desc = 0, c_leaf = 0, c_pop = 0, c_t0 = clock64();
  unsigned n_before = 0, t_before = 0;  // the lane's node visits / triangle tests before the iteration
  static __device__ __forceinline__ void spill() { atomicAdd(g_spill_stores, 1ull); }  // overflow-area stores (8 B each)
  __device__ __forceinline__ void refill() { s_refill++; }
  // the phase that ends here; all but the refill wait for their memory operations first
  __device__ __forceinline__ void phase(Phase p) {
    if (p != kRefill) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    const unsigned long long t = clock64();
    (p == kRefill ? c_ref : p == kDescend ? c_desc : p == kLeaf ? c_leaf : c_pop) += t - c_t0;
    c_t0 = t;
  }
  __device__ __forceinline__ void iteration(unsigned long long active, unsigned nnodes, unsigned ntris) {
    n_before = nnodes;
    t_before = ntris;
    s_it++;
    s_act += (unsigned long long)__popcll(active);
  }
  __device__ __forceinline__ void iteration_end(unsigned nnodes, unsigned ntris) {
    unsigned dm = nnodes - n_before, lm = ntris - t_before;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      dm = max(dm, (unsigned)__shfl_xor((int)dm, off));
      lm = max(lm, (unsigned)__shfl_xor((int)lm, off));
    }
    s_dmax += dm;
    s_lmax += lm;
  }
  __device__ __forceinline__ void flush(unsigned long long* ctr, int lane) const {
    if (lane != 0) return;
    atomicAdd(&ctr[4], s_it);
    atomicAdd(&ctr[5], s_act);
    atomicAdd(&ctr[6], s_dmax);
    atomicAdd(&ctr[7], s_lmax);
    atomicAdd(&ctr[8], s_refill);
    atomicAdd(&ctr[9], c_ref);
    atomicAdd(&ctr[10], c_desc);
    atomicAdd(&ctr[11], c_leaf);
    atomicAdd(&ctr[12], c_pop);
  }
};
#else
constexpr int kAccWords = 4;
// static: as members (a `this` to pass) the empty calls gave every trace
// kernel other code, as static ones they leave it byte for byte
struct TravStats {
  enum Phase { kRefill, kDescend, kLeaf, kPop };
  static __device__ __forceinline__ void spill() {}
  static __device__ __forceinline__ void refill() {}
  static __device__ __forceinline__ void phase(Phase) {}
  static __device__ __forceinline__ void iteration(unsigned long long, unsigned, unsigned) {}
  static __device__ __forceinline__ void iteration_end(unsigned, unsigned) {}
  static __device__ __forceinline__ void flush(unsigned long long*, int) {}
};
#endif
// Tree depth limit: the reference caps maxDepth at KD_MAX_STACK = 64
// (kdtree.cc:42), and yk_device_upload refuses deeper trees, so a descent of
// a valid tree never takes more than kDescTrips trips of the descent loop (a
// compile-time bound: the watchdog adds no register to the loop)
constexpr int kMaxTreeDepth = 64;
constexpr unsigned kDescTrips = kMaxTreeDepth + 2;
// The cooperative kernels keep no hit record in registers: a closest hit has
// been found iff Z < dist (every accepted hit lowers Z below its start,
// dist), and its (t, b1, b2, prim) stay in the lane's LDS candidate slot
// (coop_leaves); a corrupt traversal marks the lane with sp = kSpError.
constexpr int kSpError = -16;  // an inline constant: no register holds it

// A constant materialised where it is used (the compiler otherwise keeps
// non-inline constants in VGPRs for the whole traversal loop).
template <unsigned C>
__device__ __forceinline__ unsigned vconst() {
  unsigned v;
  asm volatile("v_mov_b32 %0, %1" : "=v"(v) : "i"(C));
  return v;
}
// x of lane src (ds_bpermute; __shfl adds a lane-dependent term for narrow
// widths that the compiler keeps live)
__device__ __forceinline__ float bperm(float x, int src) {
  return __int_as_float(__builtin_amdgcn_ds_bpermute(src << 2, __float_as_int(x)));
}
__device__ __forceinline__ unsigned bperm(unsigned x, int src) {
  return (unsigned)__builtin_amdgcn_ds_bpermute(src << 2, (int)x);
}
// The lane index, recomputed where it is used (two VALU ops) instead of
// kept live: the compiler hoists a lane index and every lane address derived
// from it (LDS slots, a 64-bit overflow pointer) out of the traversal loop,
// and in the any-hit kernel those invariants held ~8 VGPRs for its whole
// life -- the difference between 6 and 7 waves per SIMD. The volatile asm
// keeps the compiler from hoisting it.
__device__ __forceinline__ int lane_fresh() {
  int l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  return l;
}
// R: LDS ring depth (a power of two)
template <int R>
struct LaneStackT {
  uint2* lds;    // [R][64], this wave's
  uint2* ovf;    // overflow area of the launch: each lane's entries contiguous (one cache line holds 8)
  unsigned depth;  // overflow entries per lane
  unsigned wave;   // the wave's index in the launch (wave-uniform)
  // the lane's overflow entry k, addressed on use (rare)
  __device__ __forceinline__ uint2* ovf_at(int k) const {
    return ovf + ((size_t)(wave * 64u + (unsigned)lane_fresh()) * depth + (unsigned)k);
  }
  // ring slot of entry sp (R a power of two: a mask; else sp mod R)
  static __device__ __forceinline__ int ring(int sp) { return (R & (R - 1)) == 0 ? (sp & (R - 1)) : (int)((unsigned)sp % (unsigned)R); }
  __device__ __forceinline__ void push(int sp, uint2 e) const {
    uint2* slot = lds + ring(sp) * 64 + lane_fresh();
    if (sp >= R) {
      *ovf_at(sp - R) = *slot;
      TravStats::spill();
    }
    *slot = e;
  }
  __device__ __forceinline__ uint2 pop(int sp) const {  // sp = index of the entry to pop
    uint2* slot = lds + ring(sp) * 64 + lane_fresh();
    const uint2 e = *slot;
    if (sp >= R) *slot = *ovf_at(sp - R);
    return e;
  }
};
using LaneStack = LaneStackT<kStackLds>;
// Entry and exit points are kept implicitly (no 3-float points in
// registers): the reference's pb of an entry / exit is from + t*dir on every
// axis but the one of the split plane it lies on, which is the split itself
// (kdtree.cc:740-760 computes it so), so a point is (t, split, code) with
// code 0-2 that axis, 3 none (the tree-bound exit) and, for the entry only,
// 4 = the ray origin (an entry t < 0, kdtree.cc:699). One coordinate is
// rebuilt on use with the same float operations, so it is bit-identical to
// the stored point. (5 registers fewer than two stored points.)
struct Trav {
  v3 o, d, inv;
  float tmin, dist;
  float en_t, en_split, ex_t, ex_split;
  uint32_t en_code;
  uint32_t ex_w;  // (exit far node + 1) | axis code << 30; node -1 = the initial exit
  int node, sp;
  float Z, b1, b2;
  int prim;
  // transparent shadows (IntersectTS): filter colour, transparent surfaces
  // crossed, and the prims already filtered (std::set in the reference)
  c3 filt;
  int tdepth, nfilt, ts_max;
  int filtered[9];
};

struct __attribute__((aligned(8))) NodePair {
  uint32_t a, b, c, d;
};
__device__ __forceinline__ NodePair ld_pair(const uint2* nodes, int i) {
  return *reinterpret_cast<const NodePair*>(nodes + i);
}

// v[axis] for axis in 0..2 via selects (no dynamic register indexing)
__device__ __forceinline__ float sel3(v3 v, uint32_t ax) { return ax == 0u ? v.x : (ax == 1u ? v.y : v.z); }
// the same with the axis masks already computed (v by value: selects of
// registers, never of addresses)
__device__ __forceinline__ float sel3m(v3 v, bool a0, bool a1) { return a0 ? v.x : (a1 ? v.y : v.z); }

// coordinate ax of an implicit point (t, split, code): oa, da = from[ax], dir[ax]
__device__ __forceinline__ float pt_coord(float t, float split, uint32_t code, uint32_t ax, float oa, float da) {
  const float v = oa + t * da;
  return code == ax ? split : (code == 4u ? oa : v);
}

// scene_t::intersect (scene.cc:852-879) / isShadowed (scene.cc:881-902)
// setup + tree bound test; false = miss. UNI: universal mode, whose
// IntersectS accepts t > tmin of the shifted ray (ray_kdtree.cc:936), kept
// as t >= the next float after tmin.
template <bool CLOSEST, bool TS = false, bool UNI = false>
__device__ __forceinline__ bool trav_begin(const DScene& S, Trav& st, const yk_ray& r) {
  st.d = V3(r.dir[0], r.dir[1], r.dir[2]);
  if (CLOSEST) {
    st.o = V3(r.from[0], r.from[1], r.from[2]);
    st.tmin = r.tmin;
    st.dist = (r.tmax < 0.f) ? __uint_as_float(vconst<0x7f800000u>()) : r.tmax;
  } else {
    st.o = V3(r.from[0] + r.tmin * st.d.x, r.from[1] + r.tmin * st.d.y, r.from[2] + r.tmin * st.d.z);
    // IntersectS accepts t >= 0 (universal: t > tmin); IntersectTS keeps the
    // ray's tmin in both modes (kdtree.cc:1061, ray_kdtree.cc identical)
    st.tmin = TS ? r.tmin : (UNI ? nextafterf(r.tmin, INFINITY) : 0.f);
    st.dist = (r.tmax < 0.f) ? __uint_as_float(vconst<0x7f800000u>()) : r.tmax - 2.0f * r.tmin;
  }
  if (TS) {
    st.filt = C3(1.f, 1.f, 1.f);
    st.tdepth = 0;
    st.nfilt = 0;
  }
  st.Z = st.dist;
  st.prim = -1;
  st.b1 = st.b2 = 0.f;
  float a, b;
  st.inv = V3(1.0f / st.d.x, 1.0f / st.d.y, 1.0f / st.d.z);
  if (!bound_cross(S.bound, st.o, st.d, st.inv, a, b, st.dist)) return false;
  st.en_t = a;
  st.en_split = a;
  st.en_code = (a >= 0.0f) ? 3u : 4u;  // from + a*dir, or the origin itself
  st.ex_t = b;
  st.ex_split = b;          // code 3 entries carry t
  st.ex_w = 3u << 30;       // node -1, code 3
  st.node = 0;
  st.sp = 0;
  return true;
}

// One iteration of the reference's outer traversal loop (kdtree.cc:707-812):
// descend to a leaf, test its primitives, then stop or pop. Returns true when
// the ray is finished. The descent's four reference cases reduce to a
// near/far choice plus an optional push: with enter <= split the near child
// is the left one and the far one is pushed unless exit <= split; otherwise
// the near child is the right one and the left is pushed unless split < exit.
// (The reference's "exit == split" branch follows "exit <= split" and is
// never taken, NaN included.)
// Triangle test of one leaf entry; true when an any-hit query is done.
template <bool GLT = false>
__device__ __forceinline__ c3 mat_transparency(const DMat& M, const SurfPt& sp, v3 wo);
__device__ __forceinline__ SurfPt make_surface(const DScene& S, v3 from, v3 dir, const yk_hit& h);

template <bool CLOSEST, bool TS = false, bool GLT = false>
__device__ __forceinline__ bool leaf_test(const DScene& S, Trav& st, uint32_t p, float4 A, float4 E1, float4 E2,
                                          bool& occluded) {
  float th, u, v;
  if (mt_intersect(V3(A.x, A.y, A.z), V3(E1.x, E1.y, E1.z), V3(E2.x, E2.y, E2.z), st.o, st.d, th, u, v)) {
    if (TS) {  // IntersectTS leaf body, kdtree.cc:1054-1100
      if (!(th < st.dist && th >= st.tmin)) return false;
      const int mat = __float_as_int(S.ng[p].w) & (kSmoothBit - 1);
      const DMat& M = c_mats[mat];
      if (!(M.flags & BSDF_FILTER)) {  // !isTransparent(): opaque occluder
        occluded = true;
        return true;
      }
      bool seen = false;
#pragma unroll
      for (int k = 0; k < 9; ++k) seen |= (k < st.nfilt) && st.filtered[k] == (int)p;
      if (seen) return false;  // filtered.insert(mp).second == false
#pragma unroll
      for (int k = 0; k < 9; ++k)
        if (k == st.nfilt) st.filtered[k] = (int)p;
      st.nfilt++;
      if (st.tdepth >= st.ts_max) {
        occluded = true;
        return true;
      }
      const SurfPt sp = make_surface(S, st.o, st.d, yk_hit{(int)p, th, u, v});
      st.filt = cmul(st.filt, mat_transparency<GLT>(M, sp, st.d));
      st.tdepth++;
      return false;
    }
    if (CLOSEST) {
      if (th < st.Z && th >= st.tmin) {
        st.Z = th;
        st.prim = (int)p;
        st.b1 = u;
        st.b2 = v;
      }
    } else if (th < st.dist && th >= 0.f) {
      occluded = true;
      return true;
    }
  }
  return false;
}

// Per-lane step (the transparent-shadow kernel, whose leaf body is
// sequential: IntersectTS filters each transparent prim once, in leaf order).
template <bool CLOSEST, bool TS = false, bool GLT = false, class STK = LaneStack>
__device__ __forceinline__ bool trav_step(const DScene& S, Trav& st, const STK& stk, unsigned& nnodes,
                                          unsigned& ntris, bool& occluded) {
  if (st.dist < st.en_t) return true;
  int node = st.node;
  // node pairs: every load brings nodes[node] and nodes[node + 1] (the left
  // child), so a descent to the left child right after a load needs no
  // memory round trip (the node array carries one padding node)
  NodePair q = ld_pair(S.nodes, node);
  uint2 nd = make_uint2(q.a, q.b), nx = make_uint2(q.c, q.d);
  bool have = true;
  nnodes++;
  const unsigned n0 = nnodes;
  for (;;) {
    const uint32_t ax = nd.y & 3u;
    if (ax == 3u) break;
    if (nnodes - n0 > S.depth_cap || st.sp > (int)S.depth_cap) {  // watchdog: no valid descent is this deep
      st.prim = -2;
      return true;
    }
    const float split = __uint_as_float(nd.x);
    const int right = (int)(nd.y >> 2);
    const float oa = sel3(st.o, ax), da = sel3(st.d, ax);
    const float enp = pt_coord(st.en_t, st.en_split, st.en_code, ax, oa, da);
    const float exq = pt_coord(st.ex_t, st.ex_split, st.ex_w >> 30, ax, oa, da);
    const bool left_first = enp <= split;
    const bool push = left_first ? !(exq <= split) : !(split < exq);
    if (push) {
      const int far_ = left_first ? right : node + 1;
      const float t = (split - oa) * sel3(st.inv, ax);
      stk.push(st.sp, make_uint2(__float_as_uint(st.ex_split), st.ex_w));
      st.sp++;
      st.ex_t = t;
      st.ex_split = split;
      st.ex_w = (uint32_t)(far_ + 1) | (ax << 30);
    }
    if (left_first && have) {
      node = node + 1;
      nd = nx;
      have = false;
    } else {
      node = left_first ? node + 1 : right;
      q = ld_pair(S.nodes, node);
      nd = make_uint2(q.a, q.b);
      nx = make_uint2(q.c, q.d);
      have = true;
    }
    nnodes++;
  }
  const uint32_t n = nd.y >> 2, w0 = nd.x;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t p = (n == 1) ? w0 : S.leaf[w0 + i];
    ntris++;
    float4 A, E1, E2;
    ld_tri(S.tris + (size_t)p * kTriWords, A, E1, E2);
    // keep the three loads together (the compiler would otherwise sink A's
    // load past the det test: a second dependent round trip per triangle)
    asm volatile("" : "+v"(A.x), "+v"(A.y), "+v"(A.z), "+v"(E1.x), "+v"(E1.y), "+v"(E1.z), "+v"(E2.x),
                 "+v"(E2.y), "+v"(E2.z));
    if (leaf_test<CLOSEST, TS, GLT>(S, st, p, A, E1, E2, occluded)) return true;
  }
  if (CLOSEST && st.prim >= 0 && st.Z <= st.ex_t) return true;
  // pop: entry := exit, exit := previous exit
  st.en_t = st.ex_t;
  st.en_split = st.ex_split;
  st.en_code = st.ex_w >> 30;
  st.node = (int)(st.ex_w & 0x3FFFFFFFu) - 1;
  if (st.node < 0) return true;
  // corrupt state (never index out of the tree or the stack area): a node
  // outside the tree, or a stack outside [1, depth_cap] -- a valid traversal
  // holds at most depth_cap entries, and the overflow area has room for one
  // more descent's pushes than that
  if ((unsigned)st.node >= S.nnodes || (unsigned)(st.sp - 1) >= S.depth_cap) {
    st.prim = -2;
    return true;
  }
  st.sp--;
  const uint2 e = stk.pop(st.sp);
  st.ex_split = __uint_as_float(e.x);
  st.ex_w = e.y;
  const uint32_t code = e.y >> 30;
  st.ex_t = (code == 3u) ? st.ex_split : (st.ex_split - sel3(st.o, code)) * sel3(st.inv, code);
  return false;
}

// ---- wave-cooperative leaf testing -------------------------------------
// The traversal kernels are bound by VALU issue, and the per-lane leaf loop
// ran at 17-31 % lane utilisation (a wave loops to the longest leaf among its
// lanes while most lanes hold 0-2 references). Here each iteration is split:
// every lane descends to its next leaf (trav_descend), then the wave tests the
// (ray, reference) pairs of ALL its lanes' leaves together, 64 pairs per
// round (coop_leaves), then every lane applies its leaf's outcome and pops
// (trav_next). The outcome of a leaf is the reference's sequential leaf loop
// (kdtree.cc:760-800 closest, 905-940 any-hit):
//  * closest: the first reference i with the smallest t among the hits with
//    tmin <= t < Z (Z as the leaf is entered) -- the lexicographic minimum of
//    (t, i), found with one LDS atomic min per hit on a (t bits, i) key;
//  * any-hit: occluded when any reference hits with 0 <= t < dist; the
//    reference stops at the first such i and has tested i + 1 triangles,
//    which the triangle-test counter reproduces (LDS atomic min on i).
// Results, node and triangle-test counts are therefore those of the per-lane
// loop, bit for bit.

// Node packets: 24 B per node X holding X's own 8-B word and those of its two
// children (left = X + 1, right), built by k_pack_nodes. One
// load then serves two levels of the descent: the decision at X picks the near
// child, whose word is already in registers, and the decision there picks the
// next packet to load. Every lane of a wave advances two levels per memory
// round trip, which a pair-reuse scheme (round 1: +2 %, round 2: -1 %) cannot
// promise -- a wave waits for its slowest lane's load. 82 MB on the 1M probe
// (a 32-B stride, two aligned 16-B loads, measured 2765 against 2786 Mrays/s
// for the 24-B one: 25 % less footprint in the 256 MB Infinity Cache).
// (Empty-leaf skipping -- parent bits marking empty children, walked through
// or popped through without loads -- measured 2185 / 2072 / 2394 Mrays/s
// against 2497 without: lanes that keep going stretch the wave's iteration.)
constexpr unsigned kPkWords = 6;
// packet of node i: p0 = (word of i, word of its left child), r = right child's word.
// LDSL: the LDS copy of a small scene, split in two arrays -- p0 at base +
// 16 i, r at base2 + 8 i: a ds_read_b128 serves 16 lanes per LDS cycle when
// their 16-B slots lie in distinct bank quads, and a 32-B packet stride
// would leave half of the quads unused (MI355X_MICROARCH.md §LDS)
template <bool LDSL = false>
__device__ __forceinline__ void ld_packet(const char* base, const char* base2, uint32_t i, uint4& p0, uint2& r) {
  if constexpr (LDSL) {
    p0 = reinterpret_cast<const uint4*>(base)[i];
    r = reinterpret_cast<const uint2*>(base2)[i];
  } else {
    const char* a = base + (size_t)i * (4 * kPkWords);
    p0 = *reinterpret_cast<const uint4*>(a);
    r = *reinterpret_cast<const uint2*>(a + 16);
  }
}
__global__ void k_pack_nodes(const uint2* __restrict__ nodes, uint32_t* __restrict__ pk, unsigned n) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint2 w = nodes[i];
  uint2 l = make_uint2(0u, 0u), r = make_uint2(0u, 0u);
  if ((w.y & 3u) != 3u) {
    l = nodes[i + 1];
    r = nodes[w.y >> 2];
  }
  uint32_t* o = pk + (size_t)i * kPkWords;
  *reinterpret_cast<uint4*>(o) = make_uint4(w.x, w.y, l.x, l.y);
  *reinterpret_cast<uint2*>(o + 4) = r;
}

// Leaf-ordered triangles: a copy of every leaf-list entry's
// triangle (a, e1, e2 as in S.tris) in leaf-list order. A multi-primitive
// leaf's k-th test then loads ltris[w0 + k] directly instead of leaf[w0 + k]
// and then tris[p]: one dependent memory round trip less per test, for 36 B
// per leaf reference (147 MB on the 1M probe, 15 GB on the 10M hair scene:
// HBM is 288 GB).
__global__ void k_gather_leaf_tris(const float* __restrict__ tris, const uint32_t* __restrict__ leaf,
                                   float* __restrict__ out, unsigned n) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* src = tris + (size_t)leaf[i] * kTriWords;
  float* dst = out + (size_t)i * kTriWords;
#pragma unroll
  for (unsigned w = 0; w < kTriWords; ++w) dst[w] = src[w];
}

// One descent decision at interior node `node` (word nd, axis ax): the near /
// far choice of kdtree.cc:711-761 plus the push of the far child (exit :=
// split point). Returns the near child.
// (Round 5: empty-leaf elision here -- a near child that is an empty leaf
// entered past in registers, a far one pushed flagged and popped through --
// was parity-green and lost: DESIGN.md §5.)
template <class STK>
__device__ __forceinline__ uint32_t desc_decide(Trav& st, const STK& stk, uint2 nd, uint32_t node, uint32_t ax) {
  const float split = __uint_as_float(nd.x);
  const uint32_t right = nd.y >> 2;
  const bool a0 = ax == 0u, a1 = ax == 1u;
  const float oa = sel3m(st.o, a0, a1), da = sel3m(st.d, a0, a1);
  const float enp = pt_coord(st.en_t, st.en_split, st.en_code, ax, oa, da);
  const float exq = pt_coord(st.ex_t, st.ex_split, st.ex_w >> 30, ax, oa, da);
  const bool left_first = enp <= split;
  // far child pushed unless the exit stays on the near side; evaluated on
  // wave masks (SALU) instead of per-lane 0/1 selects
  const unsigned long long m_lf = __builtin_amdgcn_ballot_w64(left_first);
  const unsigned long long m_c1 = __builtin_amdgcn_ballot_w64(exq <= split);
  const unsigned long long m_c2 = __builtin_amdgcn_ballot_w64(split < exq);
  const bool push = __builtin_amdgcn_inverse_ballot_w64((m_lf & ~m_c1) | (~m_lf & ~m_c2));
  if (push) {
    const uint32_t far_ = left_first ? right : node + 1u;
    const float t = (split - oa) * sel3m(st.inv, a0, a1);
    stk.push(st.sp, make_uint2(__float_as_uint(st.ex_split), st.ex_w));
    st.sp++;
    st.ex_t = t;
    st.ex_split = split;
    st.ex_w = (far_ + 1u) | (ax << 30);
  }
  return left_first ? node + 1u : right;
}

#ifndef YK_DESC_FRAC
#define YK_DESC_FRAC 4  // measured 2 / 3 / 4 / 8: 2477 / 2524 / 2527 / 2450 Mrays/s (off: 2344)
#endif
#ifndef YK_DESC_FRAC_S
#define YK_DESC_FRAC_S 3  // any-hit kernel (round 4: 1/3 vs 1/4, +0.4-0.8 % with the combined defaults)
#endif
// Descends from st.node to a leaf (the descent of trav_step); false when the
// ray is already finished (dist < entry t). Outputs the leaf's w0 and count.
// nbase: the packets (S.pk, or with LDSL their LDS copy, right words at nbase2).
template <bool CLOSEST, bool LDSL = false, class STK>
__device__ __forceinline__ bool trav_descend(const DScene& S, const char* nbase, const char* nbase2, Trav& st,
                                             const STK& stk,
                                             unsigned& nnodes, uint32_t& w0, uint32_t& nref, bool& paused) {
  paused = false;
  if (st.dist < st.en_t) return false;
  // node indices are unsigned 32-bit offsets from the uniform node pointer
  // (one address VALU per load: base in SGPRs, 32-bit lane offset)
  uint32_t node = (uint32_t)st.node;
  uint4 p0;
  uint2 p1, nd;
  ld_packet<LDSL>(nbase, nbase2, node, p0, p1);
  nd = make_uint2(p0.x, p0.y);
  nnodes++;
  uint32_t ax = nd.y & 3u;
  constexpr unsigned kFrac = CLOSEST ? YK_DESC_FRAC : YK_DESC_FRAC_S;
  // descent pause (YK_DESC_FRAC = f > 0): once fewer than 1/f of the lanes
  // that started this descent are still descending, those pause at their
  // current node and resume in the next iteration, so the wave does not loop
  // to its longest descent while the other lanes idle
  const unsigned started = kFrac ? (unsigned)__popcll(__builtin_amdgcn_ballot_w64(true)) : 0u;
  // watchdog: every trip of this loop takes each descending lane at least one
  // level down, so in a valid tree no descent outlasts kDescTrips trips (a
  // wave-uniform count against a constant). A longer one is cut there like a
  // paused descent; a lane caught in a cycle keeps visiting nodes, which the
  // per-ray node-visit bound in trace_body turns into an error.
  unsigned trips = 0;
  // wave-uniform loop: the exit test is a ballot, and lanes whose descent
  // ended sit out the body under the exec mask. (A divergent loop exit makes
  // the compiler copy the descent's live-out registers every step, 13 of ~27
  // VALU ops; removing them measured equal: the loop waits on its loads.)
  bool desc = ax != 3u;
  for (;;) {
    const unsigned long long m = __builtin_amdgcn_ballot_w64(desc);
    if (m == 0ull) break;
    if (kFrac && (unsigned)__popcll(m) * kFrac < started) break;
    if (++trips > kDescTrips) break;
    if (!desc) continue;
    uint32_t nxt = desc_decide(st, stk, nd, node, ax);
    // the near child's word is in the packet: decide there too (unless it is
    // a leaf), then load the packet of the node that decision picks
    const bool left = nxt == node + 1u;
    nd = left ? make_uint2(p0.z, p0.w) : p1;
    node = nxt;
    nnodes++;
    ax = nd.y & 3u;
    if (ax != 3u) {
      nxt = desc_decide(st, stk, nd, node, ax);
      ld_packet<LDSL>(nbase, nbase2, nxt, p0, p1);
      nd = make_uint2(p0.x, p0.y);
      node = nxt;
      nnodes++;
      ax = nd.y & 3u;
    }
    desc = ax != 3u;
  }
  if (desc) {  // paused: resumes at this node in the next iteration
    if ((unsigned)st.sp > S.depth_cap) {  // watchdog: a stack no valid traversal reaches
      st.sp = kSpError;
      return false;
    }
    paused = true;
    st.node = (int)node;
    nnodes--;  // counted again when the next descent reloads it
    return true;
  }
  w0 = nd.x;
  nref = nd.y >> 2;
  return true;
}

// After the leaf: the closest-hit stop test, then pop (kdtree.cc:802-812).
// True when the ray is finished.
template <bool CLOSEST, class STK>
__device__ __forceinline__ bool trav_next(const DScene& S, Trav& st, const STK& stk) {
  if (CLOSEST && st.Z < st.dist && st.Z <= st.ex_t) return true;
  st.en_t = st.ex_t;
  st.en_split = st.ex_split;
  st.en_code = st.ex_w >> 30;
  st.node = (int)(st.ex_w & 0x3FFFFFFFu) - 1;
  if (st.node < 0) return true;
  // corrupt state (never index out of the tree or the stack area): a node
  // outside the tree, or a stack outside [1, depth_cap] -- a valid traversal
  // holds at most depth_cap entries, and the overflow area has room for one
  // more descent's pushes than that
  if ((unsigned)st.node >= S.nnodes || (unsigned)(st.sp - 1) >= S.depth_cap) {
    st.sp = kSpError;
    return true;
  }
  st.sp--;
  const uint2 e = stk.pop(st.sp);
  st.ex_split = __uint_as_float(e.x);
  st.ex_w = e.y;
  const uint32_t code = e.y >> 30;
  st.ex_t = (code == 3u) ? st.ex_split : (st.ex_split - sel3(st.o, code)) * sel3(st.inv, code);
  return false;
}

// total-order key of a float (for t >= 0 the raw bits; -0 is made +0 first so
// that equal t compare equal, as the reference's t < Z does)
__device__ __forceinline__ uint32_t ord_key(float t) {
  const uint32_t b = __float_as_uint(t + 0.0f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// Owner of a pair slot: lanes whose reference range starts in
// the round's 64 slots write ((range start + 1) << 8 | lane) at that slot of an LDS
// table, and an inclusive max-scan over the table (DPP, seeded with the
// previous round's last owner) gives every slot the lane whose range covers it
// -- one LDS write / read and six VALU steps instead of a six-step binary
// search of dependent cross-lane reads (measured equal; kept for the shorter
// dependency chain).
__device__ __forceinline__ unsigned dpp_max_scan(unsigned x) {
  // row_shr 1/2/4/8 within 16-lane rows, then row_bcast 15 / 31; lanes whose
  // source is out of range keep their value (old = x, max is idempotent)
  x = max(x, (unsigned)__builtin_amdgcn_update_dpp((int)x, (int)x, 0x111, 0xf, 0xf, false));
  x = max(x, (unsigned)__builtin_amdgcn_update_dpp((int)x, (int)x, 0x112, 0xf, 0xf, false));
  x = max(x, (unsigned)__builtin_amdgcn_update_dpp((int)x, (int)x, 0x114, 0xf, 0xf, false));
  x = max(x, (unsigned)__builtin_amdgcn_update_dpp((int)x, (int)x, 0x118, 0xf, 0xf, false));
  x = max(x, (unsigned)__builtin_amdgcn_update_dpp((int)x, (int)x, 0x142, 0xa, 0xf, false));
  x = max(x, (unsigned)__builtin_amdgcn_update_dpp((int)x, (int)x, 0x143, 0xc, 0xf, false));
  return x;
}

#ifndef YK_ANYHIT_SKIP
#define YK_ANYHIT_SKIP 1
#endif
#ifndef YK_ANYHIT_DYN
#define YK_ANYHIT_DYN 1  // any-hit leaves of several rounds: rounds scheduled over the lanes not yet occluded
#endif
// Wave-uniform: every lane calls it; nref = 0 for lanes without a leaf to test.
// BIG: trees with a leaf of 2^17 references or more (degenerate or heavily
// overlapping geometry at maxDepth), whose absolute range starts overflow the
// 24-bit owner keys: the keys then hold the start relative to the round and
// the owner's start is read from its lane (one cross-lane read more per
// round; measured 0.7 % slower, so only such trees run it).
// Orders a wave's LDS traffic between the phases of the leaf test. W waves
// per workgroup: with one, a barrier (which is what it was written with);
// with several (the small-scene kernels), fences only -- the waves run
// independent rays and never wait for each other.
template <int W>
__device__ __forceinline__ void wave_lds_sync() {
  if constexpr (W == 1) {
    __syncthreads();
  } else {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }
}

// tb / lb: the triangle records by prim and in leaf order (S.tris / S.ltris,
// or their LDS copies: W > 1, 48-B records)
template <bool CLOSEST, bool BIG = false, bool UNI = false, int W = 1>
__device__ __forceinline__ void coop_leaves(const DScene& S, const float* tb, const float* lb, Trav& st,
                                            uint32_t nref, uint32_t w0,
                                            std::conditional_t<CLOSEST, unsigned long long, unsigned>* keys,
                                            float4* cand, unsigned* otab, const float* s_tmin,
                                            unsigned& ntris, bool& occluded) {
  constexpr unsigned TW = W > 1 ? 12u : kTriWords;  // record stride (words)
  const int lane = lane_fresh();
  unsigned x = nref;  // inclusive prefix sum of the lanes' reference counts
  // DPP scan: row_shr 1/2/4/8 within 16-lane rows, then row_bcast 15 / 31
  // carry the row totals (out-of-row sources read 0)
  x += (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, false);
  x += (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, false);
  x += (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, false);
  x += (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, false);
  x += (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xa, 0xf, false);
  x += (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xc, 0xf, false);
  const unsigned pre = x - nref;
  const unsigned total = (unsigned)__builtin_amdgcn_readlane((int)x, 63);
  if (total == 0u) return;
  {
    const unsigned m1 = vconst<0xFFFFFFFFu>();
    if (CLOSEST) keys[lane] = ((unsigned long long)m1 << 32) | m1;
    else keys[lane] = m1;  // any-hit keys are reference indices: 32 bits
  }
  wave_lds_sync<W>();
  const float zlim = CLOSEST ? st.Z : st.dist;
  if constexpr (!CLOSEST && YK_ANYHIT_DYN) {
    // Any-hit leaves of more than one round (crowded leaves: hair): the
    // rounds are scheduled as they go -- each round hands its 64 slots to the
    // next untested references of the lanes not yet occluded (a prefix scan
    // of what they have left), so an occluded lane's remaining references
    // take no slots at all. A lane's references are still tested in index
    // order, and its key is the lowest hitting index: the reference's first
    // hit and test count.
    if (total > 64u) {
      unsigned cons = 0u;  // references of this lane already tested
      for (;;) {
        const unsigned rem = (keys[lane] == ~0u) ? nref - cons : 0u;
        unsigned y = rem;
        y += (unsigned)__builtin_amdgcn_update_dpp(0, (int)y, 0x111, 0xf, 0xf, false);
        y += (unsigned)__builtin_amdgcn_update_dpp(0, (int)y, 0x112, 0xf, 0xf, false);
        y += (unsigned)__builtin_amdgcn_update_dpp(0, (int)y, 0x114, 0xf, 0xf, false);
        y += (unsigned)__builtin_amdgcn_update_dpp(0, (int)y, 0x118, 0xf, 0xf, false);
        y += (unsigned)__builtin_amdgcn_update_dpp(0, (int)y, 0x142, 0xa, 0xf, false);
        y += (unsigned)__builtin_amdgcn_update_dpp(0, (int)y, 0x143, 0xc, 0xf, false);
        const unsigned rpre = y - rem;
        const unsigned rtot = (unsigned)__builtin_amdgcn_readlane((int)y, 63);
        if (rtot == 0u) break;
        otab[lane] = 0u;
        if (rem > 0u && rpre < 64u) otab[rpre] = (rpre << 8) + (vconst<0x100u>() | (unsigned)lane);
        wave_lds_sync<W>();
        // slot 0 always starts a range (the first lane with references left)
        const unsigned ov = dpp_max_scan(otab[lane]);
        int own;
        asm volatile("v_and_b32 %0, 0xff, %1" : "=v"(own) : "v"(ov));
        const unsigned k = bperm(cons, own) + ((unsigned)lane - ((ov >> 8) - 1u));
        const uint32_t ow0 = bperm(w0, own), on = bperm(nref, own);
        const v3 ro = V3(bperm(st.o.x, own), bperm(st.o.y, own), bperm(st.o.z, own));
        const v3 rd = V3(bperm(st.d.x, own), bperm(st.d.y, own), bperm(st.d.z, own));
        const float rz = bperm(zlim, own);
        const float rtmin = UNI ? s_tmin[own] : 0.f;
        if ((unsigned)lane < rtot) {
          const float* tp = (on == 1u) ? tb + (size_t)ow0 * TW : lb + (size_t)(ow0 + k) * TW;
          float4 A, E1, E2;
          ld_tri<TW>(tp, A, E1, E2);
          asm volatile("" : "+v"(A.x), "+v"(A.y), "+v"(A.z), "+v"(E1.x), "+v"(E1.y), "+v"(E1.z), "+v"(E2.x),
                       "+v"(E2.y), "+v"(E2.z));
          float th, u, v;
          if (mt_intersect(V3(A.x, A.y, A.z), V3(E1.x, E1.y, E1.z), V3(E2.x, E2.y, E2.z), ro, rd, th, u,
                                        v) &&
              th < rz && th >= rtmin)
            atomicMin(&keys[own], k);
        }
        if (rem > 0u && rpre < 64u) cons += min(rem, 64u - rpre);
        wave_lds_sync<W>();
      }
      if (nref > 0u) {
        const unsigned kk = keys[lane];
        if (kk != ~0u) {
          occluded = true;
          ntris += kk + 1u;
        } else {
          ntris += nref;
        }
      }
      return;
    }
  }
  unsigned carry = 0u;  // ((start + 1) << 8 | lane) of the range covering the previous slot
  for (unsigned base = 0; base < total; base += 64u) {
    const unsigned s = base + (unsigned)lane;
    const unsigned sc = min(s, total - 1u);
    // owner of slot s: the last lane whose range starts at or before s
    // keys hold (range start + 1) << 8 in 32 bits: without BIG every leaf has
    // fewer than 2^17 references (64 lanes x 2^17 < 2^24)
    otab[lane] = 0u;
    if (nref > 0u && pre >= base && pre - base < 64u)
      otab[pre - base] = ((BIG ? pre - base : pre) << 8) + (vconst<0x100u>() | (unsigned)lane);
    wave_lds_sync<W>();
    const unsigned ov = dpp_max_scan(otab[lane]);
    // slots before the round's first range start continue the range that
    // covered the previous round's last slot
    const unsigned okey = ov ? ov : carry;
    carry = (unsigned)__builtin_amdgcn_readlane((int)okey, 63);
    // owner lane, extracted once into a plain register (folded into SDWA
    // shifts the compiler would keep 2, 3 and 4 in VGPRs for the whole loop)
    int own;
    asm volatile("v_and_b32 %0, 0xff, %1" : "=v"(own) : "v"(okey));
    const unsigned pown = BIG ? bperm(pre, own) : (okey >> 8) - 1u;
    const unsigned k = sc - pown;
    const uint32_t ow0 = bperm(w0, own), on = bperm(nref, own);
    const v3 ro = V3(bperm(st.o.x, own), bperm(st.o.y, own), bperm(st.o.z, own));
    const v3 rd = V3(bperm(st.d.x, own), bperm(st.d.y, own), bperm(st.d.z, own));
    const float rz = bperm(zlim, own);
    // the owner's tmin (closest hits, universal any-hit) from LDS: one
    // register fewer for the whole traversal than keeping it in Trav
    const float rtmin = (CLOSEST || UNI) ? s_tmin[own] : 0.f;
    bool valid = false;
    unsigned long long key = 0;
    float th = 0.f, u = 0.f, v = 0.f;
    uint32_t p = 0;
    // any-hit, from the second round on: a pair whose owner already has a hit
    // at a lower reference (an earlier round's atomic) is not tested -- the
    // reference's leaf loop stopped there, and the owner's key is final
    // (crowded leaves span many rounds: hair)
    if (s < total && (CLOSEST || !YK_ANYHIT_SKIP || base == 0u || keys[own] > k)) {
      // one record: the leaf's own, in leaf order (a single-reference leaf's
      // from the prim array)
      const float* tp = (on == 1u) ? tb + (size_t)ow0 * TW : lb + (size_t)(ow0 + k) * TW;
      float4 A, E1, E2;
      ld_tri<TW>(tp, A, E1, E2);
      asm volatile("" : "+v"(A.x), "+v"(A.y), "+v"(A.z), "+v"(E1.x), "+v"(E1.y), "+v"(E1.z), "+v"(E2.x),
                   "+v"(E2.y), "+v"(E2.z));
      if (mt_intersect(V3(A.x, A.y, A.z), V3(E1.x, E1.y, E1.z), V3(E2.x, E2.y, E2.z), ro, rd, th, u,
                                    v)) {
        valid = th < rz && th >= rtmin;
        if (valid) {
          if (CLOSEST) {
            key = ((unsigned long long)ord_key(th) << 32) | k;
            atomicMin(&keys[own], key);
          } else {
            atomicMin(&keys[own], k);
          }
        }
      }
    }
    if (CLOSEST) {
      wave_lds_sync<W>();
      // the winner keeps its prim as a code: prim | 1 << 31 for a
      // single-reference leaf, else its leaf-list position, read when the
      // ray finishes (a leaf-list load here put a dependent global load on
      // every round that has a winner)
      if (valid && keys[own] == key) {
        p = (on == 1u) ? (ow0 | 0x80000000u) : ow0 + k;
        cand[own] = make_float4(th, u, v, __uint_as_float(p));
      }
    }
  }
  wave_lds_sync<W>();
  if (nref > 0u) {
    const unsigned long long kk = CLOSEST ? (unsigned long long)keys[lane] : (keys[lane] == ~0u ? ~0ull : keys[lane]);
    if (CLOSEST) {
      ntris += nref;
      if (kk != ~0ull) st.Z = cand[lane].x;  // (t, b1, b2, prim) stay in cand[lane]
    } else if (kk != ~0ull) {
      occluded = true;
      ntris += (unsigned)kk + 1u;
    } else {
      ntris += nref;
    }
  }
}

// Per-lane leaf test of the small-scene kernels (YK_SMALL_LANE_LEAF): each
// lane runs its own leaf's references in the reference's order
// (kdtree.cc:760-800 closest, 905-940 any-hit) from the LDS records. With
// the 1-2 references per leaf of such trees this costs a wave max(nref)
// tests instead of the cooperative round's scans and ray shuffles. Closest
// hits keep (t, b1, b2, code) in cand[lane]: code = prim | 1 << 31 for a
// single-reference leaf, else the leaf-list position (the prim id is read
// from the leaf list once, when the ray finishes).
template <bool CLOSEST, bool UNI>
__device__ __forceinline__ void lane_leaves(const float* tb, const float* lb, Trav& st, uint32_t nref, uint32_t w0,
                                            float4* cand, const float* s_tmin, unsigned& ntris, bool& occluded) {
  if (nref == 0u) return;
  const int lane = lane_fresh();
  const float tmin = (CLOSEST || UNI) ? s_tmin[lane] : 0.f;
  uint32_t i = 0;
  for (; i < nref; ++i) {
    const float* tp = (nref == 1u) ? tb + (size_t)w0 * 12u : lb + (size_t)(w0 + i) * 12u;
    float4 A, E1, E2;
    ld_tri<12u>(tp, A, E1, E2);
    float th, u, v;
    if (mt_intersect(V3(A.x, A.y, A.z), V3(E1.x, E1.y, E1.z), V3(E2.x, E2.y, E2.z), st.o, st.d, th, u,
                                  v)) {
      if (CLOSEST) {
        if (th < st.Z && th >= tmin) {
          st.Z = th;
          cand[lane] = make_float4(th, u, v, __uint_as_float(nref == 1u ? (w0 | 0x80000000u) : w0 + i));
        }
      } else if (th < st.dist && th >= tmin) {
        occluded = true;
        break;
      }
    }
  }
  ntris += (!CLOSEST && occluded) ? i + 1u : nref;
}

__device__ __forceinline__ unsigned long long shfl_u64(unsigned long long v, int src) {
  const unsigned lo = bperm((unsigned)v, src), hi = bperm((unsigned)(v >> 32), src);
  return ((unsigned long long)hi << 32) | lo;
}

// Persistent ray-query kernel. One 64-lane wave per workgroup (W waves for
// the small-scene kernels, which share an LDS copy of the scene); each lane owns
// one ray at a time and advances it one leaf visit per loop iteration. Lanes
// whose ray finished are refilled from a global work counter in bulk
// (__ballot + one atomicAdd per wave + mbcnt-style ranks), so the wave stays
// packed with live rays until the queue drains. Stack: LDS, [depth][lane].
// idx (optional): queue entry r is ray idx[r]; the result goes to the same
// slot (used by the shadow queue, whose rays sit in per-sample slots).
// Number of rays of a launch: a host value, or a 32-bit field of a device
// queue-count word (so launches need no host round trip).
// nsum > 1: the sum of the fields of nsum consecutive words (the merged
// shadow queue: one count word per slot region)
struct RayCount {
  const unsigned long long* word;
  int shift;
  long long host;
  int nsum = 1;
  __device__ __forceinline__ long long get() const {
    if (!word) return host;
    long long t = 0;
    for (int i = 0; i < nsum; ++i) t += (long long)((word[i] >> shift) & 0xFFFFFFFFull);
    return t;
  }
};

// Small-scene kernels (W > 1 waves per workgroup): the workgroup copies the
// whole traversal data -- node packets (32-B stride) and both record arrays
// (48-B records) -- into LDS once, and its waves then trace from there, off
// the vector-memory path that bounds the traversal (DESIGN.md §4). The waves
// share nothing else: each has its own block of the per-wave LDS below.
#ifndef YK_SMALL_W
#define YK_SMALL_W 4  // waves per workgroup of the small-scene kernels
#endif
static_assert(YK_SMALL_W >= 1 && YK_SMALL_W <= 16, "YK_SMALL_W: 1..16 waves per workgroup (<= 1024 threads)");
#ifndef YK_SMALL_RING
#define YK_SMALL_RING 4  // their LDS stack ring depth (entries per lane)
#endif
#ifndef YK_SMALL_LANE_LEAF
#define YK_SMALL_LANE_LEAF 1  // small-scene kernels test leaves per lane (lane_leaves), not cooperatively
#endif
#ifndef YK_SMALL_MAX
#define YK_SMALL_MAX 16384  // largest LDS copy (bytes) that takes the small-scene kernels
#endif
extern __shared__ uint4 yk_dyn_lds[];
template <bool CLOSEST, bool UNI, int R>
struct WaveLds {
  // owner table and keys of the cooperative leaf test (unused by lane_leaves)
  unsigned otab[YK_SMALL_LANE_LEAF ? 1 : 64];
  std::conditional_t<CLOSEST, unsigned long long, unsigned> keys[YK_SMALL_LANE_LEAF ? 1 : 64];
  float s_tmin[(CLOSEST || UNI) ? 64 : 1];
  unsigned ray_n0[64];
  unsigned res_slot[CLOSEST ? 1 : 128];
  float4 cand[CLOSEST ? 64 : 1];
  uint2 stack[R * 64];
};
// LDS copy of the traversal data: the packets' 16-B halves (4 words per
// node), their right words (2 per node), then -- from a 16-B boundary -- the
// records by prim and in leaf order (12 words each: a, e1, e2 padded to 16 B)
__host__ __device__ __forceinline__ unsigned small_rec_word(unsigned nn) { return (nn * 6u + 3u) & ~3u; }
__device__ __forceinline__ void small_scene_copy(const DScene& S, uint32_t* dst, int W) {
  const unsigned nthr = 64u * (unsigned)W;
  const unsigned n4 = S.nnodes * 4u, n6 = S.nnodes * 6u;
  for (unsigned i = threadIdx.x; i < n6; i += nthr) {
    const unsigned node = i < n4 ? i >> 2 : (i - n4) >> 1, w = i < n4 ? i & 3u : 4u + ((i - n4) & 1u);
    dst[i] = S.pk[node * kPkWords + w];
  }
  float* t = reinterpret_cast<float*>(dst + small_rec_word(S.nnodes));
  const unsigned nt = S.ntris * 12u, nl = S.nlref * 12u;
  for (unsigned i = threadIdx.x; i < nt + nl; i += nthr) {
    const bool own = i < nt;
    const unsigned j = own ? i : i - nt, rec = j / 12u, w = j - rec * 12u, c = w & 3u;
    const float* src = own ? S.tris : S.ltris;
    t[i] = c < 3u ? src[rec * kTriWords + (w >> 2) * 3u + c] : 0.f;
  }
}
size_t small_scene_bytes(size_t nn, size_t ntris, size_t nlref) {
  return 4 * (((6 * nn + 3) & ~(size_t)3) + 12 * (ntris + nlref));  // small_rec_word in 64 bits
}

// w of a shadow ray whose tmin is its origin record's (Batch comment): tmax,
// or the sentinel for tmax < 0 (no distance limit); a NaN tmax is stored as
// the positive quiet NaN, never as the sentinel
constexpr unsigned kTmaxInf = 0xFFC00000u;  // negative quiet NaN
__device__ __forceinline__ float shadow_w(float tmax) {
  // fabsf: a tmax of -0 loses its sign bit, which marks a MIS ray (unpack_shadow)
  return tmax < 0.f ? __uint_as_float(kTmaxInf) : (tmax != tmax ? __uint_as_float(0x7FC00000u) : fabsf(tmax));
}
// the shadow ray of slot record dw and origin record o (inverse of the
// encodings above; every value read back is the one the shading computed)
__device__ __forceinline__ yk_ray unpack_shadow(float4 dw, float4 o) {
  yk_ray r;
  r.from[0] = o.x;
  r.from[1] = o.y;
  r.from[2] = o.z;
  r.dir[0] = dw.x;
  r.dir[1] = dw.y;
  r.dir[2] = dw.z;
  const bool inf = __float_as_uint(dw.w) == kTmaxInf, mis = !inf && (__float_as_uint(dw.w) >> 31) != 0u;
  r.tmin = mis ? YK_MIN_RAYDIST : o.w;
  r.tmax = inf ? -1.f : (mis ? -dw.w : dw.w);
  return r;
}

// The rays of a trace launch: whole 32-B rays, or (the SPLIT any-hit kernels,
// batches with split = 1) the shadow-slot records {dir, w} and the origin
// records {P, tmin} (Batch comment). A split queue entry e holds the slot's k
// above its origin index: origin e & omask, slot (e >> kshift) * kstride +
// (e & omask). (A modulo of the slot index instead spilled two more
// registers inside the any-hit kernel's loop, and one kernel serving both
// forms a third: the forms are separate instantiations.)
struct RaySrc {
  const yk_ray* rays;
  const float4* sdir;
  const float4* sorg;
  unsigned omask, kshift, kstride;
};

// trace_body's FLAGS: transparent shadows (filter colours, up to ts_depth
// surfaces), a leaf of 2^17 references or more (coop_leaves BIG), a
// universal-mode scene (t > tmin), split shadow slots (RaySrc), the camera
// rays' group hand-out, glass transparency in the leaf body (mat_transparency<true>)
constexpr unsigned kTrTS = 1, kTrBig = 2, kTrUni = 4, kTrSplit = 8, kTrGroup = 16, kTrGlt = 32;

template <bool CLOSEST, int NSEG, int W = 1, unsigned FLAGS = 0>
__device__ __forceinline__ void trace_body(DScene S, RaySrc src, const unsigned* __restrict__ idx,
                                           RayCount rc, yk_hit* __restrict__ hits, uint8_t* __restrict__ occl,
                                           unsigned long long* __restrict__ work, unsigned long long* __restrict__ ctr,
                                           uint2* __restrict__ ovf, int ovf_depth, int refill_min,
                                           float* __restrict__ tsf = nullptr, int ts_depth = 0) {
  constexpr bool TS = (FLAGS & kTrTS) != 0, BIG = (FLAGS & kTrBig) != 0, UNI = (FLAGS & kTrUni) != 0,
                 SPLIT = (FLAGS & kTrSplit) != 0, GROUP = (FLAGS & kTrGroup) != 0, GLT = (FLAGS & kTrGlt) != 0;
  static_assert(!GROUP || (CLOSEST && !TS && !UNI && !SPLIT), "the group hand-out serves the camera-ray closest-hit kernels");
  using KeyT = std::conditional_t<CLOSEST, unsigned long long, unsigned>;
  constexpr int R = W > 1 ? YK_SMALL_RING : (CLOSEST ? kStackLdsC : kStackLds);
  unsigned* otab;
  uint2* lds;
  float* s_tmin;    // the lanes' tmin, read by the cooperative leaf test
  unsigned* res_slot;  // any-hit results awaiting their store: (ray index << 1) | occluded
  unsigned* ray_n0;
  KeyT* keys;
  float4* cand;
  const char* nbase;  // traversal data: HBM, or the workgroup's LDS copy
  const char* nbase2 = nullptr;
  const float *tb, *lb;
  unsigned wv = 0;  // wave of the workgroup
  int lane;
  if constexpr (W == 1) {
    // LDS of the cooperative leaf test first: its owner table then sits at
    // offset 0, and its addresses need no base register
    __shared__ unsigned a_otab[64];
    __shared__ uint2 a_lds[R * 64];
    __shared__ float a_tmin[(CLOSEST || UNI) ? 64 : 1];
    __shared__ unsigned a_res[(!CLOSEST && !TS) ? 128 : 1];
    __shared__ unsigned a_n0[64];
    __shared__ KeyT a_keys[64];
    __shared__ float4 a_cand[CLOSEST ? 64 : 1];
    otab = a_otab;
    lds = a_lds;
    s_tmin = a_tmin;
    res_slot = a_res;
    ray_n0 = a_n0;
    keys = a_keys;
    cand = a_cand;
    nbase = reinterpret_cast<const char*>(S.pk);
    tb = S.tris;
    lb = S.ltris;
    lane = threadIdx.x;
  } else {
    __shared__ WaveLds<CLOSEST, UNI, R> s_w[W];
    wv = (unsigned)__builtin_amdgcn_readfirstlane((int)threadIdx.x) >> 6;
    WaveLds<CLOSEST, UNI, R>& L = s_w[wv];
    otab = L.otab;
    lds = L.stack;
    s_tmin = L.s_tmin;
    res_slot = L.res_slot;
    ray_n0 = L.ray_n0;
    keys = L.keys;
    cand = L.cand;
    uint32_t* dst = reinterpret_cast<uint32_t*>(yk_dyn_lds);
    small_scene_copy(S, dst, W);
    __syncthreads();  // the only workgroup barrier: the waves run independently from here
    nbase = reinterpret_cast<const char*>(dst);
    nbase2 = reinterpret_cast<const char*>(dst + S.nnodes * 4u);
    tb = reinterpret_cast<const float*>(dst + small_rec_word(S.nnodes));
    lb = tb + S.ntris * 12u;
    lane = threadIdx.x & 63u;
  }
  const unsigned gw = blockIdx.x * (unsigned)W + wv;  // wave of the launch
  unsigned npend = 0;  // wave-uniform
  const long long n = __builtin_amdgcn_readfirstlane((int)rc.get());
  if (gw == 0 && lane == 0 && n > 0) atomicAdd(&ctr[3], (unsigned long long)n);  // rays traced
  // Small launches (the later bounces: 0.1-2.5M rays on a grid of ~6k waves)
  // engage only the waves they can fill with a 64-ray chunk each: the others
  // leave at once instead of contending on the queue and counter atomics
  // (each wave's end-of-launch adds; a tail of ~0.3 ms per small launch)
  if ((long long)gw * 64 >= n + 63) return;
  const LaneStackT<R> stk{lds, ovf, (unsigned)ovf_depth, gw};
  int rid = -1;  // ray of this lane (host guarantees n < 2^31)
  bool exhausted = false;
  Trav st;
  unsigned nnodes = 0, ntris = 0, nerr = 0;
  // Ray hand-out. The queue is cut into NSEG (1 or 8) contiguous segments, one per XCD:
  // consecutive queue entries are spatially coherent (tile / pixel order), so
  // the rays an XCD traces touch a compact part of the tree and its private
  // 4 MB L2 keeps it. A wave takes chunks of its own XCD's segment (one
  // atomic per chunk), then steals from the other segments. Chunks are sized
  // so that every wave takes about YK_POOL_CHUNKS of them, within
  // [64, S.chunk_max] rays: with cheap rays (the 36-tri Cornell box) a fixed
  // 64-ray chunk made the segment counters' atomics the limit (shadow
  // launches at 5.2 Grays/s; 256-ray chunks +52 %), while small launches keep
  // small chunks for the tail. Crowded-leaf scenes (hair: 528 triangle tests
  // per ray) keep 64-ray chunks: their rays are costly and uneven, and larger
  // chunks measured 446 against 518 Mrays/s there. Pool bounds are
  // wave-uniform (scalar registers).
#ifndef YK_POOL_CHUNKS
#define YK_POOL_CHUNKS 16
#endif
#ifndef YK_POOL_CHUNK_MAX
#define YK_POOL_CHUNK_MAX 512
#endif
  const unsigned kPoolChunk = (unsigned)__builtin_amdgcn_readfirstlane((int)max(
      64u, min(min((unsigned)YK_POOL_CHUNK_MAX, S.chunk_max),
               (unsigned)(n / ((long long)gridDim.x * W * YK_POOL_CHUNKS)) & ~63u)));
  unsigned xcc;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(xcc));
  constexpr unsigned kAll = (1u << NSEG) - 1u;
  // (GROUP: whole groups per segment, so every chunk starts at a multiple of 64)
  const unsigned seg_len = GROUP ? ((unsigned)((n + NSEG - 1) / NSEG) + 63u) & ~63u : (unsigned)((n + NSEG - 1) / NSEG);
  unsigned pool_next = 0, pool_end = 0;
  unsigned seg_done = 0;  // bit s: segment s has no chunks left
  // Group hand-out (GROUP: the camera-ray launch, whose queue holds a pixel's
  // samples consecutively). The pool hands out aligned groups of 64
  // consecutive entries, and lane l only ever traces entry gbase + l: the
  // lanes of a wave then walk almost the same nodes in the same iterations,
  // and a wave-load touches few lines. The wave takes its next group once at
  // most YK_CAMERA_T lanes are still active (0: lock-step); those stragglers
  // keep their rays, and their entries of the new group (`pending`) start
  // together when the last of them has finished. Idle lanes stay masked out.
  // Lock-step is the default: headline +2.7 % against the lane-by-lane
  // refill; thresholds of 2 and 4 kept half of that, 8 and more none of it
  // (DESIGN §5).
#ifndef YK_CAMERA_T
#define YK_CAMERA_T 0
#endif
  unsigned gbase = 0;                // wave-uniform
  unsigned long long pending = 0ull;  // entries gbase + l not started yet
  bool drained = false;               // no group left anywhere (wave-uniform)

  // per-ray watchdog: a valid traversal visits every node at most once, so a
  // ray whose node visits exceed the tree's node count is looping through a
  // corrupt tree; checked every 32nd wave iteration against the lane's node
  // count at the ray's start (kept in LDS, off the register budget: ray_n0)
  unsigned iters = 0;
  TravStats ts;  // diagnostic build only (empty otherwise)
  for (;;) {
    if constexpr (GROUP) {
      const unsigned long long act = __ballot(rid >= 0);
      bool fresh = false;
      if (pending == 0ull && !drained && __popcll(act) <= YK_CAMERA_T) {
        if (pool_next >= pool_end && seg_done != kAll) {
          // the chunk search of the refill below, at group granularity. (Its
          // own copy, as the ray start further down: shared through local
          // lambdas, every other trace kernel came out with other code and
          // k_trace_closest with 16 B of scratch instead of 8. One
          // __forceinline__ free function called from both places was tried
          // as well: all sixteen k_trace_* kernels came out with other code.)
#pragma unroll 1
          for (unsigned k = 0; k < (unsigned)NSEG; ++k) {
            const unsigned sgi = (xcc + k) % (unsigned)NSEG;
            if (seg_done & (1u << sgi)) continue;
            const unsigned long long s0 = (unsigned long long)sgi * seg_len;
            const unsigned long long s1 = min(s0 + seg_len, (unsigned long long)n);
            unsigned long long base = 0;
            if (lane == 0) base = atomicAdd(work + 16 * sgi, (unsigned long long)kPoolChunk);
            base = s0 + shfl_u64(base, 0);
            if (base < s1) {
              pool_next = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)base);
              pool_end = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)min(base + kPoolChunk, s1));
              break;
            }
            seg_done |= 1u << sgi;
          }
        }
        if (pool_next < pool_end) {
          const unsigned cnt = min(64u, pool_end - pool_next);  // a ragged last group
          gbase = pool_next;
          pending = ~0ull >> (64u - cnt);
          pool_next += cnt;
          fresh = true;
        } else {
          drained = true;
        }
      }
      // the new group's idle lanes at once; the stragglers' entries together
      const unsigned long long go = pending & ~act;
      if (go != 0ull && (fresh || (pending & act) == 0ull)) {
        ts.refill();
        const unsigned l = (unsigned)lane_fresh();
        if ((go >> l) & 1ull) {
          const int r = idx ? (int)idx[gbase + l] : (int)(gbase + l);
          if (trav_begin<CLOSEST, TS, UNI>(S, st, src.rays[r])) {
            rid = r;
            ray_n0[l] = nnodes;
            s_tmin[l] = st.tmin;
          } else {
            const unsigned m1 = vconst<0xFFFFFFFFu>(), z = vconst<0u>();
            hits[r] = yk_hit{(int)m1, __uint_as_float(z), __uint_as_float(z), __uint_as_float(z)};
          }
        }
        pending &= ~go;
      }
    }
    const unsigned long long want = GROUP ? 0ull : __ballot(rid < 0 && !exhausted);
    const unsigned long long act = __ballot(rid >= 0);
    if (want != 0ull && (act == 0ull || __popcll(want) >= refill_min)) {
      ts.refill();
      const unsigned cnt = (unsigned)__popcll(want);
      const unsigned avail = pool_end - pool_next;
      unsigned cb = 0, ce = 0;  // newly grabbed chunk [cb, ce)
      if (avail < cnt && seg_done != kAll) {
#pragma unroll 1  // rolled: an unrolled search held every segment's bounds in SGPRs (spilled to VGPR lanes)
        for (unsigned k = 0; k < (unsigned)NSEG; ++k) {
          const unsigned sgi = (xcc + k) % (unsigned)NSEG;
          if (seg_done & (1u << sgi)) continue;
          const unsigned long long s0 = (unsigned long long)sgi * seg_len;
          const unsigned long long s1 = min(s0 + seg_len, (unsigned long long)n);
          unsigned long long base = 0;
          if (lane == 0) base = atomicAdd(work + 16 * sgi, (unsigned long long)kPoolChunk);
          base = s0 + shfl_u64(base, 0);
          if (base < s1) {
            cb = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)base);
            ce = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)min(base + kPoolChunk, s1));
            break;
          }
          seg_done |= 1u << sgi;
        }
      }
      if (rid < 0 && !exhausted) {
        // lanes of `want` below this one (mbcnt: no lane mask kept live)
        const unsigned rank = __builtin_amdgcn_mbcnt_hi((unsigned)(want >> 32),
                                                         __builtin_amdgcn_mbcnt_lo((unsigned)want, 0u));
        long long q = -1;
        if (rank < avail) q = pool_next + rank;
        else if (rank - avail < ce - cb) q = cb + (rank - avail);
        if (q < 0) {
          exhausted = (seg_done == kAll);  // nothing left anywhere; else retry at the next refill
        } else {
          int r;
          yk_ray ray;
          if constexpr (!SPLIT) {
            r = idx ? (int)idx[q] : (int)q;
            ray = src.rays[r];
          } else {
            const unsigned e = idx ? idx[q] : (unsigned)q, oi = e & src.omask;
            r = (int)((e >> src.kshift) * src.kstride + oi);
            ray = unpack_shadow(src.sdir[r], src.sorg[oi]);
          }
          if (TS) st.ts_max = ts_depth;
          if (trav_begin<CLOSEST, TS, UNI>(S, st, ray)) {
            rid = r;
            ray_n0[lane_fresh()] = nnodes;
            if (CLOSEST || UNI) s_tmin[lane_fresh()] = st.tmin;
          } else if (CLOSEST) {
            // the miss record from constants materialised here (hoisted out of
            // the loop, the compiler kept the 16-B constant in 4 VGPRs)
            const unsigned m1 = vconst<0xFFFFFFFFu>(), z = vconst<0u>();
            hits[r] = yk_hit{(int)m1, __uint_as_float(z), __uint_as_float(z), __uint_as_float(z)};
          } else {
            occl[r] = 0;
            if (TS) {
              tsf[3 * (size_t)r] = 1.f;
              tsf[3 * (size_t)r + 1] = 1.f;
              tsf[3 * (size_t)r + 2] = 1.f;
            }
          }
        }
      }
      if (avail < cnt) {
        const unsigned take = min(cnt - avail, ce - cb);
        pool_next = cb + take;
        pool_end = ce;
      } else {
        pool_next += cnt;
      }
      pool_next = (unsigned)__builtin_amdgcn_readfirstlane((int)pool_next);
      pool_end = (unsigned)__builtin_amdgcn_readfirstlane((int)pool_end);
    }
    ts.phase(TravStats::kRefill);
    if (__ballot(rid >= 0) == 0ull) {
      if (GROUP ? drained && pending == 0ull : __ballot(!exhausted) == 0ull) break;
      continue;
    }
    // (ahead of the watchdog check: even an empty call after it gave the two
    // transparent-shadow kernels other code)
    ts.iteration(__ballot(rid >= 0), nnodes, ntris);
    bool runaway = false;
    if ((++iters & 31u) == 0u) runaway = rid >= 0 && nnodes - ray_n0[lane_fresh()] > S.nnodes + 2u;
    if constexpr (!TS) {
      const bool act = rid >= 0;
      bool live = false;
      uint32_t w0 = 0, nref = 0;
      bool paused = false;
      if (act) live = trav_descend<CLOSEST, (W > 1)>(S, nbase, nbase2, st, stk, nnodes, w0, nref, paused);
      ts.phase(TravStats::kDescend);
      bool occ = false;
      if constexpr (W > 1 && YK_SMALL_LANE_LEAF)
        lane_leaves<CLOSEST, UNI>(tb, lb, st, (live && !paused) ? nref : 0u, w0, cand, s_tmin, ntris, occ);
      else
        coop_leaves<CLOSEST, BIG, UNI, W>(S, tb, lb, st, (live && !paused) ? nref : 0u, w0, keys, cand, otab, s_tmin,
                                           ntris, occ);
      ts.phase(TravStats::kLeaf);
      bool fin = false;  // any-hit: a result to stage
      int fin_rid = 0;
      if (act) {
        bool done = !live || occ || (!paused && trav_next<CLOSEST>(S, st, stk));
        if (runaway) {
          st.sp = kSpError;
          done = true;
        }
        const bool err = st.sp == kSpError;
        if (err) nerr++;
        if (done) {
          if (CLOSEST) {
            yk_hit h{-1, 0.f, 0.f, 0.f};
            if (st.Z < st.dist && !err) {
              const float4 c = cand[lane_fresh()];
              unsigned p = __float_as_uint(c.w);
              p = (p & 0x80000000u) ? p & 0x7FFFFFFFu : S.leaf[p];  // the prim code of coop_leaves / lane_leaves
              h = yk_hit{(int)p, c.x, c.y, c.z};
            }
            hits[rid] = h;
          } else {
            fin = true;
            fin_rid = rid;
          }
          rid = -1;
        }
      }
      if (!CLOSEST) {
        // Any-hit results are staged in LDS and written 64 at a time: one
        // store instruction then covers the consecutive slots of the rays
        // that just finished (mostly a few cache lines), where a 1-B store
        // per finishing lane left ~33 B of partial-line HBM writes per ray
        // (round 3 PMC: 30x the result bytes)
        const unsigned long long fm = __builtin_amdgcn_ballot_w64(fin);
        if (fm) {
          const unsigned rk = __builtin_amdgcn_mbcnt_hi((unsigned)(fm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)fm, 0u));
          if (fin) {
            res_slot[npend + rk] = ((unsigned)fin_rid << 1) | (occ ? 1u : 0u);
          }
          npend += (unsigned)__popcll(fm);
          if (npend >= 64u) {
            wave_lds_sync<W>();
            const int l = lane_fresh();
            const unsigned e = res_slot[l];
            occl[e >> 1] = (uint8_t)(e & 1u);
            if (l + 64u < npend) res_slot[l] = res_slot[l + 64];
            npend -= 64u;
            wave_lds_sync<W>();
          }
        }
      }
      ts.phase(TravStats::kPop);
    } else if (rid >= 0) {
      bool occ = false;
      bool done = trav_step<CLOSEST, TS, GLT>(S, st, stk, nnodes, ntris, occ);
      if (runaway) {
        st.prim = -2;
        done = true;
      }
      if (st.prim == -2) {
        nerr++;
        st.prim = -1;
      }
      if (done) {
        if (CLOSEST) {
          hits[rid] = (st.prim >= 0) ? yk_hit{st.prim, st.Z, st.b1, st.b2} : yk_hit{-1, 0.f, 0.f, 0.f};
        } else {
          occl[rid] = occ ? 1 : 0;
          if (TS) {
            tsf[3 * (size_t)rid] = st.filt.r;
            tsf[3 * (size_t)rid + 1] = st.filt.g;
            tsf[3 * (size_t)rid + 2] = st.filt.b;
          }
        }
        rid = -1;
      }
    }
    ts.iteration_end(nnodes, ntris);
  }
  ts.flush(ctr, lane);
  if (!CLOSEST && !TS && npend) {  // the staged results left
    wave_lds_sync<W>();
    const int l = lane_fresh();
    if ((unsigned)l < npend) {
      const unsigned e = res_slot[l];
      occl[e >> 1] = (uint8_t)(e & 1u);
    }
  }
  // wave-reduced work counters (nodes visited, triangle tests)
  unsigned long long a = nnodes, b = ntris;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a += shfl_u64(a, lane ^ off);
    b += shfl_u64(b, lane ^ off);
  }
  if (lane == 0 && (a | b)) {  // waves that traced nothing add nothing
    atomicAdd(&ctr[0], a);
    atomicAdd(&ctr[1], b);
  }
  if (nerr) atomicAdd(&ctr[2], (unsigned long long)nerr);
}

// Occupancy targets (measured on MI355X, 1M-tri scene, cooperative leaves).
// Round 4 cut the kernels' registers (implicit entry / exit points: -5; lane
// index and constants recomputed at use instead of held as loop invariants:
// -8 any-hit, -6 closest-hit; hit record in LDS: -3 closest-hit), which let
// the any-hit kernel run at 7 waves per SIMD (72 VGPRs, 2 spilled to scratch
// on rare paths): same-box A/B, traversal microbenchmark camera-hit shadow
// rays 2479 (5 waves, round 3) -> 2614 (6 waves) -> 2661 (7 waves) Mrays/s,
// the centre crop at 64 spp (112 nodes per ray) 2086 -> 2455, headline
// 2976 -> 3076 (6) -> 3114 (7); 8 waves (18 spills) fell to 1715 on the
// microbenchmark. Closest-hit: its diet (80 VGPRs, 6.4 KB LDS per wave) let
// it run 6 (round 3 measured a forced 6 with spills at 2657 against 2835);
// round 5 asks for 7 (72 VGPRs, one cold spill), which the LDS caps at 25
// waves per CU (+1.4 % headline); per-XCD ray segments (+12 % from L2 locality). Any-hit per-XCD segments: 2700 / 2719 (round 2),
// 2806 / 2800 (round 3), +0.3 % at 7 waves (round 4, YK_SHADOW_SEGS=8: under
// the 2 % bar); non-temporal ray / result accesses 2775 against
// 2824; resident grids below the occupancy limit lost 2-4 %. PMC (round 3):
// the any-hit kernel's texture data path is busy 85 % of its cycles, 58 % of
// them stalled on L1 misses (L1 hit 68 %, L2 hit 65 %, 360-cycle L2 latency),
// which more resident waves hide better. Crowded-leaf scenes (hair) run the
// same kernels with 64-ray hand-out chunks (DScene.chunk_max).
// per-XCD ray segments of the any-hit kernel (A/B builds; 1 = one queue)
#ifndef YK_SHADOW_SEGS
#define YK_SHADOW_SEGS 8
#endif
#ifndef YK_CLOSEST_WAVES
#define YK_CLOSEST_WAVES 7  // round 5: 72 VGPRs (1 spilled on a cold path); its 6.4 KB of LDS per wave then allow 25 waves per CU (24 at 76 VGPRs)
#endif
#ifndef YK_SHADOW_WAVES
#define YK_SHADOW_WAVES 7
#endif

// The trace kernels of one signature, written once: X(enumerator, kernel,
// amdgpu_waves_per_eu, waves per workgroup, LDS ring depth per lane, body).
// Expanded here into the kernels and in yk_device_host.inc into TraceVariant
// and kTrace, so a kernel always meets its own workgroup size and ring; a new
// trace kernel is one line. The order is the order of the kernels in the
// code object. First the kernels of large trees (traversal data in HBM):
// plain, over a batch's split shadow slots (kTrSplit), camera rays with the
// group hand-out (kTrGroup; refill_min is unused), trees with a leaf of 2^17
// references or more (kTrBig), universal-mode scenes
// (kdTree_t<primitive_t>::IntersectS: t > tmin, kTrUni). Then the small
// scenes: traversal data in LDS, YK_SMALL_W waves per workgroup, dynamic
// LDS = small_scene_bytes.
#define YK_TRACE_VARIANTS_LARGE(X)                                                                                    \
  X(kClosest, k_trace_closest, YK_CLOSEST_WAVES, 1, kStackLdsC, trace_body<true, 8>)                                  \
  X(kShadow, k_trace_shadow, YK_SHADOW_WAVES, 1, kStackLds, trace_body<false, YK_SHADOW_SEGS>)                        \
  X(kShadowSplit, k_trace_shadow_split, YK_SHADOW_WAVES, 1, kStackLds, trace_body<false, YK_SHADOW_SEGS, 1, kTrSplit>) \
  X(kCamera, k_trace_camera, YK_CLOSEST_WAVES, 1, kStackLdsC, trace_body<true, 8, 1, kTrGroup>)                       \
  X(kCameraBig, k_trace_camera_big, YK_CLOSEST_WAVES, 1, kStackLdsC, trace_body<true, 8, 1, kTrBig | kTrGroup>)       \
  X(kClosestBig, k_trace_closest_big, YK_CLOSEST_WAVES, 1, kStackLdsC, trace_body<true, 8, 1, kTrBig>)                \
  X(kShadowBig, k_trace_shadow_big, YK_SHADOW_WAVES, 1, kStackLds, trace_body<false, 1, 1, kTrBig>)                   \
  X(kShadowUni, k_trace_shadow_uni, YK_SHADOW_WAVES, 1, kStackLds, trace_body<false, 1, 1, kTrUni>)                   \
  X(kShadowBigUni, k_trace_shadow_big_uni, YK_SHADOW_WAVES, 1, kStackLds, trace_body<false, 1, 1, kTrBig | kTrUni>)
#define YK_TRACE_VARIANTS_SMALL(X)                                                                                    \
  X(kClosestSmall, k_trace_closest_small, YK_CLOSEST_WAVES, YK_SMALL_W, YK_SMALL_RING,                                \
    trace_body<true, 8, YK_SMALL_W>)                                                                                  \
  X(kCameraSmall, k_trace_camera_small, YK_CLOSEST_WAVES, YK_SMALL_W, YK_SMALL_RING,                                  \
    trace_body<true, 8, YK_SMALL_W, kTrGroup>)                                                                        \
  X(kShadowSmall, k_trace_shadow_small, YK_SHADOW_WAVES, YK_SMALL_W, YK_SMALL_RING,                                   \
    trace_body<false, YK_SHADOW_SEGS, YK_SMALL_W>)                                                                    \
  X(kShadowSmallSplit, k_trace_shadow_small_split, YK_SHADOW_WAVES, YK_SMALL_W, YK_SMALL_RING,                        \
    trace_body<false, YK_SHADOW_SEGS, YK_SMALL_W, kTrSplit>)                                                          \
  X(kShadowUniSmall, k_trace_shadow_uni_small, YK_SHADOW_WAVES, YK_SMALL_W, YK_SMALL_RING,                            \
    trace_body<false, 1, YK_SMALL_W, kTrUni>)
#define YK_TRACE_VARIANTS(X) YK_TRACE_VARIANTS_LARGE(X) YK_TRACE_VARIANTS_SMALL(X)

#define YK_TRACE_KERNEL(id, name, wpe, W, ring, ...)                                                                  \
  __global__ void __launch_bounds__(64 * (W)) __attribute__((amdgpu_waves_per_eu(wpe)))                               \
  name(DScene S, RaySrc src, const unsigned* __restrict__ idx, RayCount n, yk_hit* __restrict__ hits,                 \
       uint8_t* __restrict__ occl, unsigned long long* __restrict__ work, unsigned long long* __restrict__ ctr,       \
       uint2* __restrict__ ovf, int ovf_depth, int refill_min) {                                                      \
    __VA_ARGS__(S, src, idx, n, hits, occl, work, ctr, ovf, ovf_depth, refill_min);                                   \
  }

YK_TRACE_VARIANTS_LARGE(YK_TRACE_KERNEL)
// The two transparent-shadow kernels take two more arguments and stay out of
// the list (enqueue_trace_ts, per_cu_ts); they keep their place between the
// listed kernels.
// transparent shadows (scene_t::isShadowed(state, ray, maxDepth, filt),
// scene.cc:904-928 -> IntersectTS): occlusion + filter colour per ray
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5)))
k_trace_shadow_ts(DScene S, RaySrc src, const unsigned* __restrict__ idx, RayCount n,
                  uint8_t* __restrict__ occl, float* __restrict__ tsf, int ts_depth, unsigned long long* __restrict__ work,
                  unsigned long long* __restrict__ ctr, uint2* __restrict__ ovf, int ovf_depth, int refill_min) {
  trace_body<false, 1, 1, kTrTS>(S, src, idx, n, nullptr, occl, work, ctr, ovf, ovf_depth, refill_min, tsf, ts_depth);
}
// the same for scenes that hold a glass with fake shadows: glassMat_t::getTransparency in the leaf body
// (mat_transparency<true>); no other scene launches it
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5)))
k_trace_shadow_ts_glass(DScene S, RaySrc src, const unsigned* __restrict__ idx, RayCount n,
                        uint8_t* __restrict__ occl, float* __restrict__ tsf, int ts_depth,
                        unsigned long long* __restrict__ work, unsigned long long* __restrict__ ctr,
                        uint2* __restrict__ ovf, int ovf_depth, int refill_min) {
  trace_body<false, 1, 1, kTrTS | kTrGlt>(S, src, idx, n, nullptr, occl, work, ctr, ovf, ovf_depth, refill_min, tsf,
                                          ts_depth);
}
YK_TRACE_VARIANTS_SMALL(YK_TRACE_KERNEL)
#undef YK_TRACE_KERNEL
