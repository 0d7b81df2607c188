// Trace launches, the host counterpart of yk_trav.inc's kernels (included
// by yk_device.hip after yk_device_host.inc): the
// tree check and traversal bounds (tree_depth, set_tree_bounds, stack_depth),
// the choice and sizing of a trace kernel (trace_variant,
// fill_trace_occupancy), enqueue_trace / enqueue_trace_ts, shadow_split,
// launch_trace, and the ray queries yk_trace_closest, yk_trace_shadow and
// yk_trace_shadow_filtered. Depends on yk_pipe_host.inc and yk_device_host.inc
// (kTrace, struct yk_device, bind_constants, YK_GUARD_*); nothing here needs
// the upload.

namespace {

// Structural check of a kd-tree in the export encoding (2 words per node:
// split bits / single prim / leaf-list offset; axis | right child or count
// << 2), before it becomes resident: every interior node i has its left child
// at i + 1 and its right child r with i + 1 < r < nn, every node but the root
// has exactly one parent, and every leaf references prims (single) or
// leaf-list entries within range. Such a structure is a tree, so a traversal
// visits each node at most once and its stack never holds more than the
// depth. Returns the depth (root = 0), or -1 with *err set.
int tree_depth(const uint32_t* w, size_t nn, size_t nleaf, size_t nprims, std::string* err) {
  if (nn == 0) {
    *err = "empty kd-tree";
    return -1;
  }
  std::vector<uint8_t> parents(nn, 0), depth(nn, 0);
  int maxd = 0;
  for (size_t i = 0; i < nn; ++i) {
    const uint32_t w0 = w[2 * i], w1 = w[2 * i + 1];
    if ((w1 & 3u) == 3u) {  // leaf
      const uint64_t cnt = w1 >> 2;
      if ((cnt == 1 && w0 >= nprims) || (cnt > 1 && (uint64_t)w0 + cnt > nleaf)) {
        *err = "kd-tree leaf " + std::to_string(i) + " references out of range";
        return -1;
      }
      continue;
    }
    const uint64_t r = w1 >> 2;
    if (i + 1 >= nn || r <= i + 1 || r >= nn) {
      *err = "kd-tree node " + std::to_string(i) + " has a child out of order or range";
      return -1;
    }
    for (const uint64_t c : {(uint64_t)i + 1, r}) {
      if (++parents[c] > 1) {
        *err = "kd-tree node " + std::to_string(c) + " has two parents";
        return -1;
      }
      if (depth[i] >= kMaxTreeDepth) {
        *err = "kd-tree deeper than 64 levels (KD_MAX_STACK)";
        return -1;
      }
      depth[c] = (uint8_t)(depth[i] + 1);  // parents precede children: one forward pass
      maxd = std::max(maxd, (int)depth[c]);
    }
  }
  for (size_t i = 1; i < nn; ++i)
    if (parents[i] != 1) {
      *err = "kd-tree node " + std::to_string(i) + " is unreachable";
      return -1;
    }
  return maxd;
}

// Traversal bounds of the resident tree (tree_depth): descents and stacks of
// a valid traversal stay within depth + 2 (depth_cap); the per-lane overflow
// area holds one descent's pushes beyond that, so a corrupt tree never
// writes outside it (stack_depth).
void set_tree_bounds(yk_device* d, int depth) {
  d->max_depth = depth;
  d->S.depth_cap = (unsigned)depth + 2u;
}
// a lane's stack is checked against depth_cap at every pop and every paused
// descent, and one descent pushes at most two entries per trip of its
// kDescTrips trips
int stack_depth(const yk_device* d) { return (int)d->S.depth_cap + 2 * (int)kDescTrips + 2; }

// YK_REFILL (1-64) overrides the per-scene refill threshold (set_handout);
// 0 = none
int refill_env() {
  static const int v = [] {
    const char* e = std::getenv("YK_REFILL");
    const int r = e ? std::atoi(e) : 0;
    return (r >= 1 && r <= 64) ? r : 0;
  }();
  return v;
}

// RaySrc of whole 32-B rays / of a batch's shadow slots
inline RaySrc ray_src(const yk_ray* r) { return RaySrc{r, nullptr, nullptr, 0u, 0u, 0u}; }
inline RaySrc shadow_src(const Batch& B) {
  if (!B.split) return ray_src(reinterpret_cast<const yk_ray*>(B.s_dir));
  return RaySrc{nullptr, B.s_dir, B.s_dir + (long long)B.K * B.kstride, (1u << B.kshift) - 1u, (unsigned)B.kshift,
                (unsigned)B.kstride};
}

// Camera rays take the group hand-out kernels (trace_body GROUP);
// YK_CAMERA_GROUPS=0 (read per render: A/B runs, tests) keeps them on the
// closest-hit kernels of the bounce rays
bool camera_groups() {
  const char* e = std::getenv("YK_CAMERA_GROUPS");
  return !(e && std::atoi(e) == 0);
}

// The kernel a trace runs: small scenes (not with big leaves) the LDS-copy
// kernels, big-leaf trees the BIG ones, universal scenes their own any-hit
// kernels; split: a render batch's shadow slots in the split form (never
// universal or big-leaf: shadow_split); camera: a render batch's camera rays.
TraceVariant trace_variant(const yk_device* d, bool closest, bool split, bool camera = false) {
  const bool small = d->small && !d->big_leaves;
  if (closest && camera) return small ? kCameraSmall : d->big_leaves ? kCameraBig : kCamera;
  if (split) return small ? kShadowSmallSplit : kShadowSplit;
  if (small) return closest ? kClosestSmall : d->S.uni ? kShadowUniSmall : kShadowSmall;
  if (closest) return d->big_leaves ? kClosestBig : kClosest;
  if (d->S.uni) return d->big_leaves ? kShadowBigUni : kShadowUni;
  return d->big_leaves ? kShadowBig : kShadow;
}

// per_cu of the variants with / without dynamic LDS (install_traversal once
// small_bytes is known / yk_device_open)
void fill_trace_occupancy(yk_device* d, bool dyn_lds) {
  for (int v = 0; v < kTraceVariants; ++v) {
    const TraceInfo& t = kTrace[v];
    if (t.dyn_lds != dyn_lds) continue;
    int blocks = 0;
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, t.kernel, 64 * t.waves,
                                                        dyn_lds ? d->small_bytes : 0));
    d->per_cu[v] = std::max(1, blocks);
  }
  if (dyn_lds) return;
  // on large trees the universal any-hit kernels run on the plain ones' grids
  d->per_cu[kShadowUni] = d->per_cu[kShadow];
  d->per_cu[kShadowBigUni] = d->per_cu[kShadowBig];
}

// Enqueues one persistent traversal launch; no host synchronisation.
// work: 128 zeroed words (per-XCD segment counters); acc: this kernel kind's
// accumulators {nodes, triangle tests, errors, rays}. ev: timing pair or null.
template <bool CLOSEST>
void enqueue_trace(yk_device* d, Pipe& P, RaySrc rays, const unsigned* idx, RayCount n, yk_hit* hits,
                   uint8_t* occ, unsigned long long* work, unsigned long long* acc, hipEvent_t ev0, hipEvent_t ev1,
                   bool camera = false) {
  const TraceVariant v = trace_variant(d, CLOSEST, !CLOSEST && rays.rays == nullptr, camera);
  const TraceInfo& t = kTrace[v];
  const long long grid = (long long)d->cus * d->per_cu[v];
  const int ovf_depth = std::max(1, stack_depth(d) - t.ring);
  P.ovf.ensure((size_t)ovf_depth * (size_t)grid * 64 * t.waves);
  if (ev0) HIPCHK(hipEventRecord(ev0, P.stream));
  launch(t.kernel, (unsigned)grid, 64 * t.waves, t.dyn_lds ? d->small_bytes : 0, P.stream, d->S, rays, idx, n, hits,
         occ, work, acc, P.ovf.p, ovf_depth, CLOSEST ? d->refill : d->refill_shadow);
  if (ev1) HIPCHK(hipEventRecord(ev1, P.stream));
}

// Transparent-shadow any-hit launch (k_trace_shadow_ts): occlusion + filter.
void enqueue_trace_ts(yk_device* d, Pipe& P, RaySrc rays, const unsigned* idx, RayCount n, uint8_t* occ,
                      float* filt, int max_depth, unsigned long long* work, unsigned long long* acc, hipEvent_t ev0,
                      hipEvent_t ev1) {
  const long long grid = (long long)d->cus * (d->ts_glass ? d->per_cu_ts_glass : d->per_cu_ts);
  const int ovf_depth = std::max(1, stack_depth(d) - kStackLds);
  P.ovf.ensure((size_t)ovf_depth * (size_t)grid * 64);
  if (ev0) HIPCHK(hipEventRecord(ev0, P.stream));
  launch(d->ts_glass ? k_trace_shadow_ts_glass : k_trace_shadow_ts, (unsigned)grid, 64, 0, P.stream, d->S, rays, idx, n,
         occ, filt, max_depth, work, acc, P.ovf.p, ovf_depth, d->refill_shadow);
  if (ev1) HIPCHK(hipEventRecord(ev1, P.stream));
}

// k_pm_lookup keeps its stack in LDS (6 B per entry, depth entries per lane)
// for radiance trees of < 2^16 nodes and depth <= kLdsPStack; else scratch.
bool lookup_lds(const yk_device* d) { return d->rm_depth <= kLdsPStack && d->rm_nnodes < 65536; }
size_t lookup_lds_bytes(int depth) { return (size_t)std::max(1, depth) * 64 * (sizeof(float) + sizeof(unsigned short)); }

// Direct lighting's ambient occlusion: ao_samples more slots per shading
// point. They take the split form with the lights' slots: every AO ray of a
// point shares its origin and bias, so 32 rays are 32 * 16 + 16 B, not 32 * 32.
inline int ao_slots(const yk_render_params* p) {
  return (p->integrator == YK_INTEGRATOR_DIRECT && p->do_ao) ? std::max(0, p->ao_samples) : 0;
}
// Shadow rays as direction records + one origin per shading point (Batch
// comment) when the lights take several samples (K >= 4) and the scene runs
// the kernels that have the split form (not universal, big-leaf or
// transparent-shadow); YK_SPLIT=0/1 (read per render: A/B runs, tests)
// forces either form where it exists
bool shadow_split(const yk_device* d, const yk_render_params* p) {
  const char* e = std::getenv("YK_SPLIT");
  const long long K = std::max<long long>(1, (long long)d->sum_light_slots + ao_slots(p));
  return (e ? std::atoi(e) != 0 : K >= 4) && !d->S.uni && !d->big_leaves && !p->transp_shadows;
}

// One kernel kind's share of yk_stats.
void add_trace_stats(yk_stats* st, bool closest, uint64_t rays, uint64_t nodes, uint64_t tris, double ms,
                     uint64_t launches = 1) {
  if (closest) {
    st->closest_rays += rays;
    st->closest_nodes += nodes;
    st->closest_tris += tris;
    st->ms_closest += ms;
    st->closest_launches += launches;
  } else {
    st->shadow_rays += rays;
    st->shadow_nodes += nodes;
    st->shadow_tris += tris;
    st->ms_shadow += ms;
    st->shadow_launches += launches;
  }
}

// Ray-query entry points: one launch, synchronised, statistics added to st.
// filt: the transparent-shadow query (k_trace_shadow_ts, up to ts_depth surfaces).
template <bool CLOSEST>
void launch_trace(yk_device* d, Pipe& P, const yk_ray* rays, long long n, yk_hit* hits, uint8_t* occ, yk_stats* st,
                  float* filt = nullptr, int ts_depth = 0) {
  if (n <= 0) return;
  if (n > 0x7FFFFFFFll - (1ll << 24)) throw std::invalid_argument("ray batch too large (max ~2^31 rays per call)");
  unsigned long long* work = P.counters.p;
  unsigned long long* acc = P.counters.p + 128;
  HIPCHK(hipMemsetAsync(work, 0, 144 * sizeof(unsigned long long), P.stream));
#ifdef YK_TRAV_STATS
  {
    const unsigned long long z = 0;
    HIPCHK(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_spill_stores), &z, sizeof z, 0, hipMemcpyHostToDevice, P.stream));
  }
#endif
  const RayCount cnt{nullptr, 0, n};
  if (filt) enqueue_trace_ts(d, P, ray_src(rays), nullptr, cnt, occ, filt, ts_depth, work, acc, P.ev0, P.ev1);
  else enqueue_trace<CLOSEST>(d, P, ray_src(rays), nullptr, cnt, hits, occ, work, acc, P.ev0, P.ev1);
  unsigned long long h[13];
  HIPCHK(hipMemcpyAsync(h, acc, sizeof h, hipMemcpyDeviceToHost, P.stream));
  HIPCHK(hipStreamSynchronize(P.stream));
  if (h[2]) throw watchdog_error("kd-tree traversal watchdog fired on " + std::to_string(h[2]) + " rays");
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, P.ev0, P.ev1));
#ifdef YK_TRAV_STATS
  std::fprintf(stderr,
               "[trav-stats] %s rays %lld: wave iterations %llu, active lanes/iter %.2f, descent trips max %.2f / "
               "mean-active %.2f, leaf trips max %.2f / mean-active %.2f, refills %llu (%.1f rays each)\n",
               CLOSEST ? "closest" : "shadow", n, h[4], (double)h[5] / (double)h[4], (double)h[6] / (double)h[4],
               (double)h[0] / (double)h[5], (double)h[7] / (double)h[4], (double)h[1] / (double)h[5], h[8],
               (double)n / (double)h[8]);
  {
    const double tot = (double)(h[9] + h[10] + h[11] + h[12]);
    std::fprintf(stderr, "[trav-stats] %s cycles: refill %.1f%% descent %.1f%% leaf %.1f%% pop %.1f%%; per wave iteration %.0f\n",
                 CLOSEST ? "closest" : "shadow", 100.0 * h[9] / tot, 100.0 * h[10] / tot, 100.0 * h[11] / tot,
                 100.0 * h[12] / tot, tot / (double)h[4]);
    unsigned long long sp = 0;
    HIPCHK(hipMemcpyFromSymbol(&sp, HIP_SYMBOL(g_spill_stores), sizeof sp));
    std::fprintf(stderr, "[trav-stats] %s overflow-area stores %llu (%.3f per ray, %.1f MB at 8 B each)\n",
                 CLOSEST ? "closest" : "shadow", sp, (double)sp / (double)n, 8e-6 * (double)sp);
  }
#endif
  if (st) add_trace_stats(st, CLOSEST, (uint64_t)n, h[0], h[1], ms);
}

// What the three ray queries share once their arguments have passed: the
// scene must be uploaded (no_scene: the refusal's text), then, under the
// guard, the handle's GPU is made current and run(stats) launches, with a
// yk_stats of its own where the caller gave none. empty_ok: an empty batch
// of an uploaded scene returns YK_OK before any of that (the filtered query).
template <class Run>
int ray_query(yk_device* d, const char* no_scene, bool empty_ok, yk_stats* st, Run run) {
  if (!d->uploaded) return set_error(YK_ERR_STATE, no_scene);
  if (empty_ok) return YK_OK;
  YK_GUARD_BEGIN
  HIPCHK(hipSetDevice(d->ordinal));
  yk_stats local{};
  run(st ? st : &local);
  return YK_OK;
  YK_GUARD_END
}

}  // namespace

extern "C" {

int yk_trace_closest(yk_device* d, const yk_ray* d_rays, int64_t n, yk_hit* d_hits, yk_stats* st) {
  if (!d || (n > 0 && (!d_rays || !d_hits)) || n < 0) return set_error(YK_ERR_ARG, "yk_trace_closest: bad arguments");
  return ray_query(d, "yk_trace_closest: no scene uploaded", false, st,
                   [&](yk_stats* s) { launch_trace<true>(d, d->pipe[0], d_rays, n, d_hits, nullptr, s); });
}

int yk_trace_shadow(yk_device* d, const yk_ray* d_rays, int64_t n, uint8_t* d_occ, yk_stats* st) {
  if (!d || (n > 0 && (!d_rays || !d_occ)) || n < 0) return set_error(YK_ERR_ARG, "yk_trace_shadow: bad arguments");
  return ray_query(d, "yk_trace_shadow: no scene uploaded", false, st,
                   [&](yk_stats* s) { launch_trace<false>(d, d->pipe[0], d_rays, n, nullptr, d_occ, s); });
}

int yk_trace_shadow_filtered(yk_device* d, const yk_ray* d_rays, int64_t n, uint8_t* d_occ, float* d_filter,
                             int32_t max_depth, yk_stats* st) {
  if (!d || (n > 0 && (!d_rays || !d_occ || !d_filter)) || n < 0)
    return set_error(YK_ERR_ARG, "yk_trace_shadow_filtered: bad arguments");
  if (max_depth < 0 || max_depth > 8) return set_error(YK_ERR_UNSUPPORTED, "max_depth must be in [0, 8]");
  return ray_query(d, "yk_trace_shadow_filtered: no scene uploaded", n <= 0, st, [&](yk_stats* s) {
    bind_constants(d);  // the transparent-shadow leaf body reads the materials
    launch_trace<false>(d, d->pipe[0], d_rays, n, nullptr, d_occ, s, d_filter, max_depth);
  });
}

}  // extern "C"
