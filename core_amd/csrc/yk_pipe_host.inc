// Host plumbing (included by yk_device.hip after namespace yk, first on the
// host side): HIPCHK, DBuf, the checked launch, Pipe with its batch buffers,
// pipes_env and the batch planner plan_batches. Depends on Batch
// (yk_device.hip, the queue and batch records) only.

#define HIPCHK(x)                                                                                \
  do {                                                                                           \
    hipError_t e_ = (x);                                                                         \
    if (e_ != hipSuccess)                                                                        \
      throw std::runtime_error(std::string("HIP error ") + hipGetErrorString(e_) + " at " #x); \
  } while (0)

namespace {

template <class T>
struct DBuf {
  T* p = nullptr;
  size_t n = 0;
  void ensure(size_t cnt) {
    if (cnt <= n && p) return;
    if (p) HIPCHK(hipFree(p));
    p = nullptr;
    n = 0;
    if (cnt == 0) return;
    HIPCHK(hipMalloc(&p, cnt * sizeof(T)));
    n = cnt;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  DBuf() = default;
  DBuf(const DBuf&) = delete;
  DBuf& operator=(const DBuf&) = delete;
  ~DBuf() { release(); }
};

// One kernel launch, checked. (dim3 converts from a plain count.)
template <class... KArgs, class... Args>
void launch(void (*kernel)(KArgs...), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, Args&&... args) {
  hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, std::forward<Args>(args)...);
  HIPCHK(hipGetLastError());
}

}  // namespace

// One batch pipeline: a stream with its own queues, counters and scratch.
// Pipes run alternate batches so one batch's kernels fill the other's launch
// tails; film gathers stay in batch order through events. Every launch reads
// its ray / path count from device memory, so a whole render is enqueued
// without a host round trip and synchronised once.
struct Pipe {
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  DBuf<unsigned long long> counters;  // [0,136): per-call ray segments + counters (ray queries)
  DBuf<unsigned long long> words;     // per-render: queue-count words, ray segments, accumulators
  DBuf<uint2> ovf;                    // traversal stack overflow (entries deeper than the LDS ring)
  std::vector<hipEvent_t> evpool;     // per-launch timing events of one render
  DBuf<unsigned> soffs, s_idx;
  DBuf<float> col, alpha, thr, pathcol, scol_next, wlast, emit_b, sl_contrib;
  DBuf<int> prim_hit, pstate, lsel, qo0, qo1, tile_base;
  DBuf<int4> tiles;
  DBuf<yk_ray> p_rays, qr0, qr1;
  DBuf<float4> s_dir;  // shadow slots (and origins) in either form (Batch)
  DBuf<yk_hit> p_hits, qh0, qh1;
  DBuf<uint8_t> sl_flags, s_occl;
  DBuf<float4> samples;
  DBuf<float2> sxy;
  DBuf<char4> pext;
  DBuf<unsigned> psample;
  DBuf<uint8_t> incl, caus;
  DBuf<float> emit0;
  DBuf<float> fgl, fglen;  // final gathering: lcol (3 per sample) and path length
  DBuf<float4> lkq;        // final gathering: radiance-map lookup queue (point | owner, normal)
  DBuf<float> s_filt, sl_aux;  // transparent shadows
  DBuf<float> zs;              // z_channel: one depth sample per camera sample (k_depth_samples)
  void create() {
    HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreate(&ev0));
    HIPCHK(hipEventCreate(&ev1));
    counters.ensure(144);
  }
  hipEvent_t event(size_t i) {
    while (evpool.size() <= i) {
      hipEvent_t e;
      HIPCHK(hipEventCreate(&e));
      evpool.push_back(e);
    }
    return evpool[i];
  }
  ~Pipe() {
    for (auto e : evpool) (void)hipEventDestroy(e);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (stream) (void)hipStreamDestroy(stream);
  }
  template <class T>
  static long long held(const DBuf<T>& b) { return (long long)(b.n * sizeof(T)); }
  // bytes of the buffers a batch plan sizes (bind, and the final-gather
  // buffers of bind_pipes): what plan_batches budgets as maxc * bytes_per_sample
  long long batch_bytes() const {
    return held(soffs) + held(s_idx) + held(col) + held(alpha) + held(thr) + held(pathcol) + held(scol_next) +
           held(wlast) + held(emit_b) + held(sl_contrib) + held(prim_hit) + held(pstate) + held(lsel) + held(qo0) +
           held(qo1) + held(tile_base) + held(tiles) + held(p_rays) + held(qr0) + held(qr1) + held(s_dir) +
           held(p_hits) + held(qh0) + held(qh1) + held(sl_flags) + held(s_occl) + held(samples) + held(sxy) +
           held(pext) + held(psample) + held(incl) + held(caus) + held(emit0) + held(fgl) + held(fglen) + held(lkq) +
           held(s_filt) + held(sl_aux) + held(zs);
  }
  // every device buffer of the pipe
  long long all_bytes() const { return batch_bytes() + held(counters) + held(words) + held(ovf); }
  // regions > 1: the merged shadow launch's slot regions (camera hits + one
  // per bounce) and per-bounce path state (merged_region)
  Batch bind(long long maxc, int K, int tiles_per_batch, bool spec, bool ts, int regions, bool split) {
    const long long nst = std::max(1, regions - 1);  // path-state copies
    soffs.ensure(maxc);
    col.ensure(3 * maxc);
    alpha.ensure(maxc);
    prim_hit.ensure(maxc);
    p_rays.ensure(maxc);
    p_hits.ensure(maxc);
    thr.ensure(3 * maxc);
    pathcol.ensure(3 * maxc);
    scol_next.ensure(3 * maxc * nst);
    wlast.ensure(maxc);
    emit_b.ensure(3 * maxc * nst);
    pstate.ensure(maxc * nst);
    lsel.ensure(maxc * nst);
    qo0.ensure(maxc);
    qo1.ensure(maxc);
    qr0.ensure(maxc);
    qr1.ensure(maxc);
    qh0.ensure(maxc);
    qh1.ensure(maxc);
    s_dir.ensure(maxc * (split ? K + 1 : 2 * K) * regions);  // K {dir, w} + one origin, or K 32-B rays (Batch)
    s_occl.ensure(maxc * K * regions);
    s_idx.ensure(maxc * K * regions);
    sl_contrib.ensure(3 * maxc * K * regions);
    sl_flags.ensure(maxc * K * regions);
    samples.ensure(maxc);
    sxy.ensure(maxc);
    pext.ensure(maxc);  // one per pixel slot; maxc bounds the slots of any spp
    tiles.ensure(tiles_per_batch);
    tile_base.ensure(tiles_per_batch + 1);
    Batch B{};
    B.prim_hit = prim_hit.p;
    B.soffs = soffs.p;
    B.col = col.p;
    B.alpha = alpha.p;
    B.p_rays = p_rays.p;
    B.p_hits = p_hits.p;
    B.thr = thr.p;
    B.pathcol = pathcol.p;
    B.scol_next = scol_next.p;
    B.wlast = wlast.p;
    B.emit_b = emit_b.p;
    B.pstate = pstate.p;
    B.lsel = lsel.p;
    B.q_owner[0] = qo0.p;
    B.q_owner[1] = qo1.p;
    B.q_rays[0] = qr0.p;
    B.q_rays[1] = qr1.p;
    B.q_hits[0] = qh0.p;
    B.q_hits[1] = qh1.p;
    B.s_dir = s_dir.p;
    B.s_occl = s_occl.p;
    B.s_idx = s_idx.p;
    B.sl_contrib = sl_contrib.p;
    B.sl_flags = sl_flags.p;
    B.samples = samples.p;
    B.sxy = sxy.p;
    B.pext = pext.p;
    B.split = split ? 1 : 0;
    B.K = K;
    B.cap = maxc;
    B.kstride = maxc * regions;
    B.kshift = 0;
    while ((1ll << B.kshift) < B.kstride) ++B.kshift;
    if (ts) {
      s_filt.ensure(3 * maxc * K);
      sl_aux.ensure(4 * maxc * K);
      B.ts = 1;
      B.s_filt = s_filt.p;
      B.sl_aux = sl_aux.p;
    }
    if (spec) {
      psample.ensure(maxc);
      incl.ensure(maxc);
      caus.ensure(maxc);
      emit0.ensure(3 * maxc);
      B.psample = psample.p;
      B.incl = incl.p;
      B.caus = caus.p;
      B.emit0 = emit0.p;
    }
    return B;
  }
};

// Batch pipelines (streams) in flight. Measured: 2 -> 1873, 3 -> 1892, 4 ->
// 1923 Mrays/s (round 1); 2 / 6 -> 2794 / 2790 against 2803 with 4 (round 2).
// YK_PIPES=1 serialises the kernels of a frame (each kernel's duration is then
// its own, for the roofline measurement in bench.py), read on every render.
constexpr int kPipes = 4;
inline int pipes_env() {
  const char* e = std::getenv("YK_PIPES");
  const int v = e ? std::atoi(e) : 0;
  return (v >= 1 && v <= kPipes) ? v : kPipes;
}

// The batch planner (host only, no device state: yk_debug_batch_plan runs it
// as it stands). Cuts the shard's tiles into batches of whole tiles, about
// `target_samples` camera samples each (default 32M: each trace launch ends
// in a tail of long rays, which large batches amortise), capped so that the
// batch buffers of all pipes stay within `budget_bytes`; the cap itself is
// floored at 1M samples, an explicit target is not (one-tile batches: tests).
// Returns nullptr, or the reason the frame cannot be planned
// (out.status = YK_ERR_UNSUPPORTED).
constexpr long long kNodeBytes = 116;  // specular node store, per node
const char* plan_batches(const yk_batch_plan_in& in, yk_batch_plan& out) {
  out = yk_batch_plan{};
  out.status = YK_ERR_UNSUPPORTED;
  if (in.slots > (1 << 20) || in.bounces < 0 || in.bounces > 62) return "too many shadow slots or bounces";
  const int K = std::max(1, in.slots);
  const int pipes_cfg = std::min(kPipes, std::max(1, in.pipes));
  const long long owned = std::max<long long>(0, in.owned_tiles);
  const int regions = in.merged ? in.bounces + 1 : 1;
  out.regions = regions;
  // one pipe's batch buffers per camera sample (Pipe::bind): 232 B of sample
  // state, rays, hits and bounce queues, 32 B of path state, 48 B of
  // final-gather state (fgl, fglen, lkq) and 18 B of specular-entry state are
  // the 400 B; 2 B per slot of margin; per region 50 B per slot (32-B ray,
  // contribution, flag, result, queue entry), 34 B + a 16-B origin per sample
  // in the split form; + 32 B of path state per extra region; transparent
  const long long region_bytes = in.split ? 34ll * K + 16 : 50ll * K;
  // shadows add 28 B per slot (s_filt, sl_aux); z_channel (reserved bit 0)
  // adds the 4-B depth sample (Pipe::zs)
  const long long bytes_per_sample = 400 + 2ll * K + region_bytes + (long long)(regions - 1) * (region_bytes + 32) +
                                     (in.transp_shadows ? 28ll * K : 0) + ((in.reserved & 1) ? 4 : 0);
  out.bytes_per_sample = bytes_per_sample;
  const long long target_env = in.target_samples > 0 ? in.target_samples : (32ll << 20);
  const long long target =
      std::min(target_env, std::max(1ll << 20, std::max<long long>(0, in.budget_bytes) / pipes_cfg / bytes_per_sample));
  const long long tile_samples = (long long)in.tile * in.tile * in.spp;
  if (in.tile < 1 || in.spp < 1) return "empty tile";
  // specular recursion: generation g holds recursion level g; every node has
  // at most two children, so a batch of nc camera samples needs at most
  // nc * (2^(L+1) - 1) nodes, L = spec_levels
  const long long spec_worst = (2ll << std::max(0, std::min(in.spec_levels, 19))) - 1;
  if (in.spec && spec_worst * tile_samples * kNodeBytes > (48ll << 30))
    return "raydepth too large for the tile size / spp (node store > 48 GB)";
  const long long target_spec = in.spec ? std::min(target, (12ll << 30) / (kNodeBytes * spec_worst)) : target;
  // at least one batch per pipeline when the frame has the tiles for it -- a
  // frame of 2 full batches (C2: 1024 tiles of 64K samples) leaves two
  // pipelines idle (C2 8388 -> 8700 Mrays/s, headline and hair unchanged);
  // photon mapping too since round 6 (its 16-spp bench frame in 4 batches
  // instead of 1: 2123-2129 against 2086-2090 Mrays/s; 6 or 8 batches lost:
  // 1874-1944; round 2 had measured 1572 -> 1537 before the final-gather
  // pipeline took its present form)
  const long long tiles_fill = in.spec ? LLONG_MAX : (owned + pipes_cfg - 1) / pipes_cfg;
  long long tiles_per_batch =
      std::max<long long>(1, std::min<long long>(INT_MAX, std::min(target_spec / tile_samples, tiles_fill)));
  // the trace kernels hold a ray's index in a signed int (-1: no ray) and
  // read a launch's ray count as one: camera-sample indices, shadow-slot
  // indices (k * kstride + r * maxc + c) and the merged launch's queue count
  // (at most maxc * K * regions) stay below 2^31; a split shadow-queue entry
  // holds k above the origin index r * maxc + c in 32 bits (Batch)
  auto index_fits = [&](long long mc) {
    if (mc >= (1ll << 31)) return false;
    int kshift = 0;
    while ((1ll << kshift) < mc * regions) ++kshift;
    return mc * (long long)K * regions < (1ll << 31) && kshift <= 31 && ((long long)(K - 1) << kshift) < (1ll << 32);
  };
  while (tiles_per_batch > 1 && !index_fits(tiles_per_batch * tile_samples)) tiles_per_batch /= 2;
  const long long maxc = tiles_per_batch * tile_samples;
  if (!index_fits(maxc)) return "one tile holds too many samples (tile^2 * spp * shadow slots * regions >= 2^31)";
  out.tiles_per_batch = (int)tiles_per_batch;
  out.maxc = maxc;
  out.kstride = maxc * regions;
  while ((1ll << out.kshift) < out.kstride) ++out.kshift;
  out.nbatch = (int)((owned + tiles_per_batch - 1) / tiles_per_batch);
  out.npipes = in.spec ? 1 : std::min(pipes_cfg, std::max(1, out.nbatch));
  out.status = YK_OK;
  return nullptr;
}
