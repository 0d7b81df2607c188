// One renderPass (integrator.cc:172-224): n samples per pixel from pixel
// sample `off`; flags (film-local bytes, host) restricts it to the pixels
// imageFilm_t::nextPass flagged.
struct PassSpec {
  int n, off;
  bool multipass;
  const uint8_t* flags;
  float* d_depth = nullptr;  // z_channel: the pass's depth film on the device (p->depth_film may be host memory)
};

namespace {

// the render reads photon maps: photon mapping, and photon caustics under
// path tracing or direct lighting (yk_photon_build for that integrator first)
bool needs_photon_maps(const yk_render_params* p) {
  return p->integrator == YK_INTEGRATOR_PHOTON ||
         (p->integrator == YK_INTEGRATOR_PATH &&
          (p->caustic_type == YK_CAUSTIC_PHOTON || p->caustic_type == YK_CAUSTIC_BOTH)) ||
         (p->integrator == YK_INTEGRATOR_DIRECT && p->dl_caustics != 0);
}

// Tile size, tile count and a custom tile order of the render area (width and
// height checked before); YK_OK or the error set.
int check_tiles(const yk_render_params* p) {
  const int tile = p->tile_size > 0 ? p->tile_size : 32;  // make_film
  if (tile > 4096) return set_error(YK_ERR_UNSUPPORTED, "tile_size > 4096");
  const int ntiles = ((p->width + tile - 1) / tile) * ((p->height + tile - 1) / tile);
  if (ntiles >= (1 << 19)) return set_error(YK_ERR_UNSUPPORTED, "too many tiles");
  if (p->tile_order && p->tile_order_len > 0) {
    if (p->tile_order_len != ntiles)
      return set_error(YK_ERR_ARG, "tile_order must list every tile of the render area once");
    std::vector<char> seen((size_t)ntiles, 0);
    for (int i = 0; i < ntiles; ++i) {
      const int t = p->tile_order[i];
      if (t < 0 || t >= ntiles || seen[(size_t)t])
        return set_error(YK_ERR_ARG, "tile_order is not a permutation of the tiles");
      seen[(size_t)t] = 1;
    }
  }
  return YK_OK;
}

// z_channel's own parameters (the depth film's memory space is the caller's
// matter); YK_OK or the error set. maxDepth may be inf, as in the reference.
int check_depth_params(const yk_render_params* p) {
  if (!p->z_channel) return YK_OK;
  if (!p->depth_film) return set_error(YK_ERR_ARG, "z_channel needs a depth_film");
  if (p->normalize_z_channel && !std::isfinite(p->depth_min))
    return set_error(YK_ERR_ARG, "normalize_z_channel needs a finite depth_min (yk_depth_range)");
  return YK_OK;
}

// Every argument and state check of a render pass; YK_OK or the error set.
int check_render_params(const yk_device* d, const yk_render_params* p, int32_t shard, int32_t nshards,
                        const float* d_film, const PassSpec& ps) {
  if (!d || !p || !d_film || nshards < 1 || shard < 0 || shard >= nshards)
    return set_error(YK_ERR_ARG, "yk_render_shard: bad arguments");
  if (!d->uploaded) return set_error(YK_ERR_STATE, "yk_render_shard: no scene uploaded");
  if (p->filter < YK_FILTER_BOX || p->filter > YK_FILTER_LANCZOS) return set_error(YK_ERR_ARG, "unknown filter");
  if (p->integrator != YK_INTEGRATOR_PATH && p->integrator != YK_INTEGRATOR_DIRECT &&
      p->integrator != YK_INTEGRATOR_PHOTON)
    return set_error(YK_ERR_ARG, "unknown integrator");
  if (p->integrator == YK_INTEGRATOR_PATH &&
      (p->caustic_type < YK_CAUSTIC_NONE || p->caustic_type > YK_CAUSTIC_BOTH))
    return set_error(YK_ERR_ARG, "unknown caustic_type");
  if (needs_photon_maps(p) && (!d->pm_ready || d->pm_integrator != p->integrator))
    return set_error(YK_ERR_STATE, "photon maps: call yk_photon_build for this integrator first (preprocess)");
  if (needs_photon_maps(p) && std::memcmp(&p->photon, &d->pm_params, sizeof(yk_photon_params)) != 0)
    return set_error(YK_ERR_STATE, "photon mapping: the maps were built with different photon parameters");
  const bool ao = p->integrator == YK_INTEGRATOR_DIRECT && p->do_ao != 0;
  if (ao && p->ao_samples < 1) return set_error(YK_ERR_ARG, "AO_samples must be >= 1");
  if (ao && !(std::isfinite(p->ao_distance) && p->ao_distance > 0.f))
    return set_error(YK_ERR_ARG, "AO_distance must be finite and > 0");
  if (ao && (long long)d->sum_light_slots + p->ao_samples > 8192)
    return set_error(YK_ERR_UNSUPPORTED,
                     "too many shadow slots per shading point (light samples + AO_samples > 8192)");
  if (p->integrator == YK_INTEGRATOR_PATH && (p->bounces < 1 || 4 * p->bounces + 4 >= 50))
    return set_error(YK_ERR_UNSUPPORTED, "bounces must be in [1, 11]");
  if (p->width <= 0 || p->height <= 0) return set_error(YK_ERR_ARG, "empty render area");
  if (p->filter_width != 0.f && !(p->filter_width >= 0.501f && p->filter_width <= 4.f))
    return set_error(YK_ERR_ARG, "filter_width must be 0 or in [0.501, 4]");
  if (const int rc = check_tiles(p)) return rc;
  // transparent shadows: the device keeps the filtered-prim set of a shadow
  // ray in 9 registers, so at most 8 transparent surfaces (defaults 4-5)
  if (p->transp_shadows && (p->shadow_depth < 0 || p->shadow_depth > 8))
    return set_error(YK_ERR_UNSUPPORTED, "shadowDepth must be in [0, 8] with transpShad");
  // a slot's aux record applies one light colour at resolve: none per sample
  if (p->transp_shadows && d->shade.xl >= kXLBg)
    return set_error(YK_ERR_UNSUPPORTED, "transparent shadows are not supported on a scene that holds a background light");
  if (ps.flags && (p->xstart + p->width > 65535 || p->ystart + p->height > 65535))
    return set_error(YK_ERR_UNSUPPORTED, "adaptive passes need coordinates < 65536");
  if (const int rc = check_depth_params(p)) return rc;
  return YK_OK;
}

// The film's side of a pass: which tiles the shard owns and, per batch, the
// tiles, sample offsets and flagged pixels (owned_tiles, build_tile_lists).
struct TileLists {
  std::vector<int> owned;   // the shard's tiles in the order the film hands them out
  std::vector<int> rank_of; // custom order: tile -> rank in `owned`, -1 other shards' tiles
  // tile lists of all batches
  std::vector<int4> tiles, rect_of;
  std::vector<int> base;
  std::vector<long long> nc_of;
  // adaptive pass: flagged pixels per batch (tile order, rows, columns) and
  // the film-pixel -> batch-local first sample map the gather reads
  std::vector<int> pix, pmap;
  std::vector<size_t> pix_off;
};

// The tiles of shard F.shard in the order the film hands them out: row-major,
// or the custom order's (a checked permutation of the film's tiles).
void owned_tiles(const FilmConst& F, const int32_t* tile_order, int tile_order_len, TileLists& L) {
  const int ntiles = F.ntx * ((F.h + F.tile - 1) / F.tile);
  if (tile_order && tile_order_len > 0) {
    L.rank_of.assign((size_t)ntiles, -1);
    for (int i = 0; i < ntiles; ++i) {
      const int t = tile_order[i];
      if (t % F.nshards != F.shard) continue;
      L.rank_of[(size_t)t] = (int)L.owned.size();
      L.owned.push_back(t);
    }
  } else {
    for (int t = F.shard; t < ntiles; t += F.nshards) L.owned.push_back(t);
  }
}

// The lists of nbatch batches of tpb owned tiles each, spp samples per pixel;
// flags (film-local bytes) restricts the samples to the flagged pixels.
void build_tile_lists(const FilmConst& F, int nbatch, int tpb, int spp, const uint8_t* flags, TileLists& L) {
  L.base.assign((size_t)nbatch * (tpb + 1), 0);
  L.nc_of.assign(nbatch, 0);
  L.rect_of.resize(nbatch);
  L.pix_off.assign(nbatch, 0);
  if (flags) L.pmap.assign((size_t)F.w * F.h, -1);
  for (int bi = 0; bi < nbatch; ++bi) {
    const size_t tb0 = (size_t)bi * tpb, tb1 = std::min(L.owned.size(), tb0 + (size_t)tpb);
    long long nc = 0;
    int rx0 = 1 << 30, ry0 = 1 << 30, rx1 = -(1 << 30), ry1 = -(1 << 30);
    L.pix_off[bi] = L.pix.size();
    for (size_t k = tb0; k < tb1; ++k) {
      const int t = L.owned[k];
      const int X = F.cx0 + (t % F.ntx) * F.tile, Y = F.cy0 + (t / F.ntx) * F.tile;
      const int W = std::min(F.tile, F.cx1 - X), H = std::min(F.tile, F.cy1 - Y);
      L.tiles.push_back(make_int4(X, Y, W, H));
      L.base[(size_t)bi * (tpb + 1) + (k - tb0)] = (int)nc;
      if (flags) {
        for (int yy = Y; yy < Y + H; ++yy)
          for (int xx = X; xx < X + W; ++xx) {
            const size_t px = (size_t)(yy - F.cy0) * F.w + (xx - F.cx0);
            if (!flags[px]) continue;
            L.pmap[px] = (int)nc;
            L.pix.push_back((yy << 16) | xx);
            nc += spp;
          }
      } else {
        nc += (long long)W * H * spp;
      }
      rx0 = std::min(rx0, X);
      ry0 = std::min(ry0, Y);
      rx1 = std::max(rx1, X + W);
      ry1 = std::max(ry1, Y + H);
    }
    L.base[(size_t)bi * (tpb + 1) + (tb1 - tb0)] = (int)nc;
    L.nc_of[bi] = nc;
    L.rect_of[bi] = make_int4(rx0, ry0, rx1, ry1);
  }
}

// The film gather of one batch on `stream`: owned tile ranks [tb0, tb1) with
// nc samples (colours, in-pixel positions, per-tile sample offsets `base`)
// into d_film; rect is the batch's tile bounds, pmap the adaptive pass's
// film-pixel map or null, pext scratch of one entry per pixel slot.
// opt: the colour gather's variant (clamp_rgb, premult_alpha; both off is the
// kernel every other render runs). depths / d_depth: the batch's depth samples
// and the depth film, or null -- the depth gather reuses the extents.
struct FilmOptions {
  bool clamp, premult;
};
inline FilmOptions film_options(const yk_render_params* p) { return FilmOptions{p->clamp_rgb != 0, p->premult_alpha != 0}; }
void launch_film_gather(hipStream_t stream, const FilmConst& F, const int* pmap, int tb0, int tb1, int4 rect,
                        long long nc, const float4* samples, const float2* sxy, const int* base, char4* pext,
                        float* d_film, FilmOptions opt = FilmOptions{false, false}, const float* depths = nullptr,
                        float* d_depth = nullptr) {
  FilmConst Fb = F;
  Fb.pmap = pmap;
  Fb.tb0 = tb0;
  Fb.tb1 = tb1;
  const int gx0 = std::max(F.cx0, rect.x + F.olo_x), gy0 = std::max(F.cy0, rect.y + F.olo_y);
  const int gx1 = std::min(F.cx1, rect.z + F.ohi_x), gy1 = std::min(F.cy1, rect.w + F.ohi_y);
  const int gw = gx1 - gx0, gh = gy1 - gy0;
  if (nc > 0 && gw > 0 && gh > 0) {
    const long long npix = nc / F.spp;  // the batch's pixel slots (spp samples each)
    launch(k_pixel_extent, grid_for(npix * 64), 256, 0, stream, Fb, sxy, pext, npix);
    auto* gather = opt.clamp ? (opt.premult ? k_film_gather<true, true> : k_film_gather<true, false>)
                             : (opt.premult ? k_film_gather<false, true> : k_film_gather<false, false>);
    if (samples)
      launch(gather, grid_for((long long)gw * gh), 256, 0, stream, Fb, samples, sxy, base, pext, d_film, gx0, gy0, gw,
             gh);
    if (depths)
      launch(k_depth_gather, grid_for((long long)gw * gh), 256, 0, stream, Fb, depths, sxy, base, pext, d_depth, gx0,
             gy0, gw, gh);
  }
}

// Everything one pass decides on the host before it enqueues: constants, the
// batch plan and the tile lists of all batches (build_frame_plan; no device
// state is touched, checked parameters are assumed).
struct FramePlan : TileLists {
  bool pm, cmap, ao, path, merged, split;
  bool cam_groups;  // camera rays take the group hand-out kernels (camera_groups)
  FilmConst F;
  RenderConst R;
  AOConst AOC;
  PMConst PMC;
  int K;                    // shadow slots per shading point: the lights', then the AO rays' (gen_ao)
  int bounces, nsub;        // trace depths and sub-paths (gather paths) of the bounce loop
  int spec_levels;          // specular recursion: the node store holds min(raydepth, 19) levels (plan_batches)
  yk_batch_plan plan;
  // per-pipe device words: [0, 2 kAccWords) accumulators {closest nodes,
  // tris, errors, rays; any-hit ...}; then per batch: queue-count words
  // (isub, depth), the final gather's lookup-queue counts (isub, depth) and
  // one 128-word hand-out block per trace or lookup launch.
  // All zeroed once; no launch needs a reset or a host round trip.
  int qwords_per_batch, launches_per_batch;
  long long words_per_batch;
};

// nullptr, or the reason the frame cannot be planned (plan_batches)
const char* build_frame_plan(const yk_device* d, const yk_render_params* p, int32_t shard, int32_t nshards,
                             const PassSpec& ps, FramePlan& fp) {
  fp.pm = p->integrator == YK_INTEGRATOR_PHOTON;
  fp.path = p->integrator == YK_INTEGRATOR_PATH;
  // pathtracing with photon caustics reads the caustic map its preprocess built;
  // direct lighting's own options (directlight.cc:137-142): photon caustics
  // under pathtracing's rules, ambient occlusion with its own shadow slots
  const bool pt_cmap = fp.path && (p->caustic_type == YK_CAUSTIC_PHOTON || p->caustic_type == YK_CAUSTIC_BOTH);
  fp.cmap = needs_photon_maps(p) && !fp.pm;
  fp.ao = p->integrator == YK_INTEGRATOR_DIRECT && p->do_ao != 0;
  FilmConst& F = fp.F;
  F = make_film(p);
  F.shard = shard;
  F.nshards = nshards;
  F.spp = ps.n;
  F.d1 = (float)(1.0 / (double)(float)ps.n);
  F.rank_of = nullptr;
  const int spp = F.spp;
  owned_tiles(F, p->tile_order, p->tile_order_len, fp);
  RenderConst& R = fp.R;
  R = RenderConst{};
  R.spp = spp;
  R.nsub = fp.path ? std::max(1, p->path_samples) : 1;
  R.pm_fg = (fp.pm && p->photon.final_gather && !p->photon.show_map) ? 1 : 0;
  R.pm_showmap = (fp.pm && p->photon.show_map) ? 1 : 0;
  if (R.pm_fg) R.nsub = std::max(1, p->photon.fg_samples);  // nSampl = max(1, nPaths / rayDivision)
  fp.PMC = needs_photon_maps(p) ? pm_const(d, p->photon) : PMConst{};
  R.bounces = p->bounces;
  R.integrator = p->integrator;
  R.transp_bg = p->transp_background;
  R.nlights = d->nlights;
  R.has_bg = d->bg_kind;
  for (int k = 0; k < 3; ++k) R.bg[k] = d->bg[k];
  for (int k = 0; k < 12; ++k) R.bg_grad[k] = d->bg_grad[k];
  R.d1 = F.d1;
  R.spec = d->spec ? 1 : 0;
  R.trace_caustics =
      (fp.path && (p->caustic_type == YK_CAUSTIC_PATH || p->caustic_type == YK_CAUSTIC_BOTH)) ? 1 : 0;
  R.rdepth = p->raydepth;
  R.level = 0;
  R.multipass = ps.multipass ? 1 : 0;
  R.pass_off = ps.off;
  R.ps = (R.spec || R.multipass) ? 1 : 0;
  fp.K = std::max(1, d->sum_light_slots + ao_slots(p));
  fp.AOC = AOConst{};
  if (fp.ao) {
    fp.AOC.n = p->ao_samples;
    fp.AOC.k0 = d->sum_light_slots;
    fp.AOC.dist = p->ao_distance;
    for (int k = 0; k < 3; ++k) fp.AOC.col[k] = p->ao_color[k];
  }
  fp.spec_levels = d->spec ? std::max(0, std::min(p->raydepth, 19)) : 0;
  // merged shadow launch (k_resolve_merged): path tracing without specular
  // recursion, photon maps or transparent shadows, one sub-path; YK_MERGE=0
  // (read per render: A/B runs, tests) keeps one any-hit launch per bounce
  const char* merge_env = std::getenv("YK_MERGE");
  fp.merged = !(merge_env && std::atoi(merge_env) == 0) && fp.path && !d->spec && !pt_cmap && !p->transp_shadows &&
              p->path_samples <= 1 && p->bounces >= 1;
  R.merged = fp.merged ? 1 : 0;
  // HBM for the batch buffers of all pipes (YK_BATCH_GB, default 64 of the
  // 288 GB, 192 with the merged launch's slot regions: C2's eight slots per
  // sample in five regions at 128 GB cut its batches from 16M to 12.6M
  // samples, six batches on four pipes, -5 %; at 192 GB it keeps four)
  static const long long batch_gb_env = [] {
    const char* e = std::getenv("YK_BATCH_GB");
    const long long v = e ? std::atoll(e) : 0;
    return (v > 0 && v <= 240) ? v : 0ll;
  }();
  fp.split = shadow_split(d, p);
  fp.cam_groups = camera_groups();
  // batches, pipes and every buffer size: plan_batches. YK_BATCH_SAMPLES and
  // YK_PIPES are read on every render (A/B runs, tests)
  yk_batch_plan_in pin{};
  pin.slots = fp.K;
  pin.bounces = fp.merged ? p->bounces : 0;
  pin.merged = fp.merged ? 1 : 0;
  pin.split = fp.split ? 1 : 0;
  pin.transp_shadows = p->transp_shadows ? 1 : 0;
  pin.spec = d->spec ? 1 : 0;
  pin.final_gather = R.pm_fg;
  pin.spec_levels = fp.spec_levels;
  pin.tile = F.tile;
  pin.spp = spp;
  pin.pipes = pipes_env();
  pin.reserved = p->z_channel ? 1 : 0;  // 4 B per sample of depth samples
  pin.owned_tiles = (long long)fp.owned.size();
  const char* target_env = std::getenv("YK_BATCH_SAMPLES");
  pin.target_samples = target_env ? std::atoll(target_env) : 0;
  pin.budget_bytes = (batch_gb_env ? batch_gb_env : (fp.merged ? 192ll : 64ll)) << 30;
  if (const char* why = plan_batches(pin, fp.plan)) return why;
  // final gathering: hits 0..fg_bounces of each gather path, queue words up to fg_bounces + 1
  fp.bounces = fp.path ? R.bounces : (R.pm_fg ? p->photon.fg_bounces + 1 : 0);
  fp.nsub = (fp.path || R.pm_fg) ? R.nsub : 1;
  fp.qwords_per_batch = fp.nsub * (fp.bounces + 1);
  fp.launches_per_batch = 2 + 2 * fp.nsub * fp.bounces + (R.pm_fg ? fp.nsub * fp.bounces : 0);
  fp.words_per_batch = 2ll * fp.qwords_per_batch + 128ll * fp.launches_per_batch;

  build_tile_lists(F, fp.plan.nbatch, fp.plan.tiles_per_batch, spp, ps.flags, fp);
  return nullptr;
}

// The plan's lists into the handle's grow-only buffers (a repeated render
// allocates nothing); F.rank_of then points at the device copy.
void upload_frame_plan(yk_device* d, FramePlan& fp) {
  auto up = [](auto& dev, const auto& host, size_t at_least) {
    dev.ensure(std::max(at_least, host.size()));
    if (!host.empty())
      HIPCHK(hipMemcpy(dev.p, host.data(), host.size() * sizeof(host[0]), hipMemcpyHostToDevice));
  };
  up(d->tiles_dev, fp.tiles, 0);
  up(d->base_dev, fp.base, 0);
  if (!fp.pmap.empty()) {  // adaptive pass
    up(d->pix_dev, fp.pix, 1);
    up(d->pmap_dev, fp.pmap, 0);
  }
  if (!fp.rank_of.empty()) {  // custom tile order: the film gather walks a window's tiles by rank
    up(d->rank_dev, fp.rank_of, 0);
    fp.F.rank_of = d->rank_dev.p;
  }
}

// Word buffers and batch buffers of the pipes the plan uses.
void bind_pipes(yk_device* d, const yk_render_params* p, const FramePlan& fp, Batch* Bp) {
  const yk_batch_plan& pl = fp.plan;
  for (int pi = 0; pi < pl.npipes; ++pi) {
    Pipe& P = d->pipe[pi];
    const int nb_here = (pl.nbatch - pi + pl.npipes - 1) / pl.npipes;
    P.words.ensure((size_t)(2 * kAccWords + (d->spec ? 0 : fp.words_per_batch * nb_here)));
    HIPCHK(hipMemsetAsync(P.words.p, 0, P.words.n * sizeof(unsigned long long), P.stream));
    Bp[pi] = P.bind(pl.maxc, fp.K, pl.tiles_per_batch, fp.R.ps != 0, p->transp_shadows != 0, pl.regions, fp.split);
    if (p->z_channel) P.zs.ensure(pl.maxc);
    if (fp.R.pm_fg) {
      P.fgl.ensure(3 * pl.maxc);
      P.fglen.ensure(pl.maxc);
      P.lkq.ensure(2 * pl.maxc);
    }
  }
}

// Node store of the specular recursion, sized for the plan's batches.
NodeStore bind_node_store(yk_device* d, const FramePlan& fp) {
  if (!d->spec) return NodeStore{};
  const long long cap = fp.plan.maxc * ((2ll << fp.spec_levels) - 1);
  d->nE.ensure(3 * cap);
  d->nD.ensure(3 * cap);
  d->nP.ensure(3 * cap);
  d->nrcol.ensure(6 * cap);
  d->nalpha.ensure(fp.plan.maxc);
  d->nflags.ensure(cap);
  d->nchild.ensure(2 * cap);
  d->nray.ensure(cap);
  d->nsoffs.ensure(cap);
  d->npsample.ensure(cap);
  d->ncount.ensure(1);
  d->noverflow.ensure(1);
  d->nmalpha.ensure(cap);
  d->spec_words.ensure((size_t)fp.words_per_batch);
  HIPCHK(hipMemsetAsync(d->noverflow.p, 0, sizeof(int), d->pipe[0].stream));
  return NodeStore{d->nE.p,   d->nD.p,     d->nP.p,       d->nflags.p, d->nchild.p,    d->nrcol.p,    d->nalpha.p,
                   d->nray.p, d->nsoffs.p, d->npsample.p, d->ncount.p, (long long)cap, d->noverflow.p, d->nmalpha.p};
}

struct Timed {
  int pipe;
  size_t ev;
  bool closest;
};

// An angular camera with `circular` set gives the samples outside its circle
// no ray (wt = 0): only then do renders keep a live-sample queue.
bool cam_can_die(const yk_device* d) { return d->cam_host.kind == YK_CAMERA_ANGULAR && d->cam_host.circular != 0; }

// What enqueueing one batch needs: the batch's pipe and buffers, its word
// block and launch cursor, and the render's list of timed trace launches.
struct BatchCtx {
  yk_device* d;
  const yk_render_params* p;
  const FramePlan* fp;
  const PassSpec* ps;
  float* d_film;
  NodeStore NS;
  std::vector<Timed>* timed;
  size_t* evn;  // timing events used so far, per pipe
  // per batch (enqueue_batch)
  int pi;
  Pipe* P;
  Batch B;
  unsigned long long* bw;  // the batch's words (FramePlan)
  int launch;              // hand-out blocks taken
  // the batch's live camera-sample count (d->cam_live), nullptr unless the
  // camera can have samples without a ray (cam_can_die)
  unsigned long long* live = nullptr;
  // z_channel: the batch's depth samples (the pipe's zs) and what
  // k_depth_samples computes them with; nullptr otherwise
  float* zs = nullptr;
  DepthConst DC{};
};

unsigned long long* qw(const BatchCtx& c, int isub, int depth) { return c.bw + isub * (c.fp->bounces + 1) + depth; }
unsigned long long* next_work(BatchCtx& c) { return c.bw + 2ll * c.fp->qwords_per_batch + 128ll * c.launch++; }

// camera: the closest-hit launch over a batch's camera rays, in sample order
void trace(BatchCtx& c, bool closest, RaySrc rays, const unsigned* idx, RayCount n, yk_hit* hits, uint8_t* occ,
           bool camera = false) {
  Pipe& P = *c.P;
  unsigned long long* work = next_work(c);
  const hipEvent_t e0 = P.event(c.evn[c.pi]), e1 = P.event(c.evn[c.pi] + 1);
  c.timed->push_back(Timed{c.pi, c.evn[c.pi], closest});
  c.evn[c.pi] += 2;
  if (closest) enqueue_trace<true>(c.d, P, rays, idx, n, hits, occ, work, P.words.p, e0, e1, camera && c.fp->cam_groups);
  else if (c.B.ts)  // transparent shadows: IntersectTS, filter colour into the slot
    enqueue_trace_ts(c.d, P, rays, idx, n, occ, c.B.s_filt, c.p->shadow_depth, work, P.words.p + kAccWords, e0, e1);
  else enqueue_trace<false>(c.d, P, rays, idx, n, hits, occ, work, P.words.p + kAccWords, e0, e1);
}
void trace_shadow_slots(BatchCtx& c, const Batch& Bc, RayCount n) {
  trace(c, false, shadow_src(Bc), Bc.s_idx, n, nullptr, Bc.s_occl);
}

// photonIntegrator_t::integrate after the direct light: show_map /
// diffuse-map estimate, final gathering, caustics (photonintegr.cc:819-852)
void enqueue_photon_mapping(BatchCtx& c, const Batch& Bc, const RenderConst& Rc, long long n) {
  yk_device* d = c.d;
  Pipe& P = *c.P;
  const PMConst& PMC = c.fp->PMC;
  const ShadeKernels& K = shade_kernels(d);
  const int fg_bounces = c.p->photon.fg_bounces;
  if (PMC.show_map || !PMC.final_gather) launch(K.pm_post, grid_for(n, 64), 64, 0, P.stream, d->S, Bc, PMC, n);
  // final gathering (photonintegr.cc:637-790): gather path index outermost,
  // pathCol accumulated across paths in the reference's order
  for (int isub = 0; isub < (Rc.pm_fg ? c.fp->nsub : 0); ++isub) {
    launch(K.fg_start, grid_for(n, YK_APPEND_BLOCK), YK_APPEND_BLOCK, 0, P.stream, d->S, Bc, Rc, n, isub, P.fgl.p,
           qw(c, isub, 0));
    int qin = 1;
    for (int it = 0; it <= fg_bounces; ++it) {
      const unsigned long long* in_w = qw(c, isub, it);
      unsigned long long* out_w = qw(c, isub, it + 1);
      trace(c, true, ray_src(Bc.q_rays[qin]), nullptr, RayCount{in_w, 32, 0}, Bc.q_hits[qin], nullptr);
      unsigned long long* lk_w = qw(c, isub, it) + c.fp->qwords_per_batch;  // lookup-queue count
      launch(K.fg_hit, grid_for(n, YK_APPEND_BLOCK), YK_APPEND_BLOCK, 0, P.stream, d->S, Bc, Rc, PMC, in_w, it, isub, qin,
             P.fgl.p, P.fglen.p, out_w, P.lkq.p, lk_w);
      if (it < fg_bounces) trace_shadow_slots(c, Bc, RayCount{out_w, 0, 0});
      const bool lds = lookup_lds(d);
      launch(lds ? k_pm_lookup<true> : k_pm_lookup<false>, (unsigned)((long long)d->cus * d->per_cu_lookup[lds]), 64,
             lds ? lookup_lds_bytes(d->rm_depth) : 0, P.stream, PMC.rmap, PMC.lookup_rad, d->rm_depth, P.lkq.p, lk_w,
             P.fgl.p, next_work(c));
      launch(k_fg_resolve, grid_for(n), 256, 0, P.stream, Bc, Rc, in_w, qin, P.fgl.p);
      qin ^= 1;
    }
  }
  launch(K.pm_finish, grid_for(n, 64), 64, 0, P.stream, d->S, Bc, Rc, PMC, n);
}

// What follows the direct light at the camera hits: photon mapping's
// estimate, photon caustics, ambient occlusion.
void enqueue_post_direct(BatchCtx& c, const Batch& Bc, const RenderConst& Rc, long long n) {
  const FramePlan& fp = *c.fp;
  hipStream_t s = c.P->stream;
  if (fp.pm) enqueue_photon_mapping(c, Bc, Rc, n);
  if (fp.cmap && fp.PMC.cmap.n != 0)  // causticMap.ready()
    launch(shade_kernels(c.d).pt_caustic, grid_for(n, 64), 64, 0, s, c.d->S, Bc, fp.PMC, n);
  if (fp.ao) launch(k_resolve_ao, grid_for(n), 256, 0, s, c.d->S, Bc, Rc, fp.AOC, n);
}

// The shading sequence of n entries (a batch's camera samples; with specular
// recursion one chunk of a generation's nodes, stored from node_base):
// primary trace and shading, direct light, the sub-paths' bounces, the ending.
void enqueue_entries(BatchCtx& c, const Batch& Bc, const RenderConst& Rc, long long n, long long node_base) {
  yk_device* d = c.d;
  const ShadeKernels& K = shade_kernels(d);
  const FramePlan& fp = *c.fp;
  hipStream_t s = c.P->stream;
  const bool merged = fp.merged;  // never with specular recursion
  // the recursion pipeline has always run the post-direct block after the
  // bounce loop; only k_pt_caustic under path tracing could tell
  const bool post_direct_after_bounces = d->spec;
  if (d->spec) {  // one word block, reused by every call
    HIPCHK(hipMemsetAsync(d->spec_words.p, 0, d->spec_words.n * sizeof(unsigned long long), s));
    c.launch = 0;
  }
  // camera rays of a camera with dead samples: the live ones' queue (k_camera;
  // the shadow queue's buffer, which k_shade_primary fills only afterwards)
  // (group hand-out: the batch's camera rays as k_camera wrote them, a pixel's
  // samples consecutive; not the live queue, not the recursion's later nodes)
  if (c.live && node_base == 0) trace(c, true, ray_src(Bc.p_rays), Bc.s_idx, RayCount{c.live, 0, 0}, Bc.p_hits, nullptr);
  else trace(c, true, ray_src(Bc.p_rays), nullptr, RayCount{nullptr, 0, n}, Bc.p_hits, nullptr, node_base == 0 && Rc.level == 0);
  // z_channel: the camera samples' depth, before the specular recursion's
  // later generations reuse the hit records
  if (c.zs && node_base == 0) launch(k_depth_samples, grid_for(n), 256, 0, s, Bc.p_rays, Bc.p_hits, c.zs, c.DC, n);
  launch(K.primary[fp.ao], grid_for(n, YK_PRIMARY_BLOCK), YK_PRIMARY_BLOCK, 0, s, d->S, Bc, Rc, n, qw(c, 0, 0), fp.AOC);
  if (!merged) {
    trace_shadow_slots(c, Bc, RayCount{qw(c, 0, 0), 0, 0});
    launch(k_resolve_primary, grid_for(n), 256, 0, s, Bc, Rc, n);
  }
  if (!post_direct_after_bounces) enqueue_post_direct(c, Bc, Rc, n);
  // sub-path index outermost: pathCol is shared across sub-paths and
  // accumulated in the reference's order (pathtracer.cc:164-298)
  for (int isub = 0; isub < (fp.path ? fp.nsub : 0); ++isub) {
    if (isub > 0)  // sub-path 0's first segment came out of k_shade_primary
      launch(K.path_start, grid_for(n, YK_BOUNCE_BLOCK), YK_BOUNCE_BLOCK, 0, s, d->S, Bc, Rc, n, isub, qw(c, isub, 0));
    int qin = 1;
    for (int depth = 1; depth <= fp.bounces; ++depth) {
      const unsigned long long* in_w = qw(c, isub, depth - 1);
      unsigned long long* out_w = qw(c, isub, depth);
      trace(c, true, ray_src(Bc.q_rays[qin]), nullptr, RayCount{in_w, 32, 0}, Bc.q_hits[qin], nullptr);
      Batch Bd = Bc;
      if (merged) {
        Bd = merged_region(Bc, depth);
        Bd.mq_words = qw(c, 0, 0);
      }
      launch(K.bounce, grid_for(n, K.bounce_block), K.bounce_block, 0, s, d->S, Bd, Rc, in_w, depth, isub, qin, out_w);
      if (!merged) {
        trace_shadow_slots(c, Bc, RayCount{out_w, 0, 0});
        launch(k_resolve_bounce, grid_for(n), 256, 0, s, Bc, Rc, in_w, depth, qin);
      }
      qin ^= 1;
    }
  }
  if (post_direct_after_bounces) enqueue_post_direct(c, Bc, Rc, n);
  if (d->spec) {
    launch(k_finish_spec, grid_for(n), 256, 0, s, Bc, Rc, c.NS, node_base, n);
    launch(K.spawn, grid_for(n), 256, 0, s, d->S, Bc, Rc, c.NS, node_base, n);
  } else if (merged) {  // one any-hit launch for the camera hits and all bounces, then one resolve
    trace_shadow_slots(c, Bc, RayCount{qw(c, 0, 0), 0, 0, fp.plan.regions});
    launch(k_resolve_merged, grid_for(n), 256, 0, s, Bc, Rc, n, fp.bounces);
  } else {
    launch(k_finish, grid_for(n), 256, 0, s, Bc, Rc, n);
  }
}

// Specular recursion: generations of nodes, host-synchronised; each
// generation shaded in chunks of at most the batch's capacity, then folded.
int enqueue_spec_generations(BatchCtx& c, long long nc) {
  const FramePlan& fp = *c.fp;
  const NodeStore& NS = c.NS;
  hipStream_t s = c.P->stream;
  const long long maxc = fp.plan.maxc;
  const unsigned long long start = (unsigned long long)nc;
  HIPCHK(hipMemcpyAsync(NS.count, &start, sizeof start, hipMemcpyHostToDevice, s));
  enqueue_entries(c, c.B, fp.R, nc, 0);
  long long g0 = 0, g1 = nc;
  for (int level = 1; level <= fp.spec_levels; ++level) {
    unsigned long long cnt = 0;
    HIPCHK(hipMemcpyAsync(&cnt, NS.count, sizeof cnt, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if ((long long)cnt > NS.cap) return set_error(YK_ERR_INTERNAL, "specular node store overflow");
    g0 = g1;
    g1 = (long long)cnt;
    if (g1 <= g0) break;
    RenderConst Rl = fp.R;
    Rl.level = level;
    for (long long off = g0; off < g1; off += maxc) {
      Batch Bc = c.B;
      Bc.p_rays = NS.ray + off;
      Bc.soffs = NS.soffs + off;
      Bc.psample = NS.psample + off;
      enqueue_entries(c, Bc, Rl, std::min<long long>(maxc, g1 - off), off);
    }
  }
  launch(k_fold, grid_for(nc), 256, 0, s, c.B, fp.R, NS, nc);
  return YK_OK;
}

// Batch bi on its pipe: camera rays, the shading sequence, the film gather
// (in batch order, whichever pipe ran the batch: gather_ev).
int enqueue_batch(BatchCtx& c, int bi) {
  yk_device* d = c.d;
  const FramePlan& fp = *c.fp;
  const FilmConst& F = fp.F;
  const int tpb = fp.plan.tiles_per_batch, npipes = fp.plan.npipes;
  Pipe& P = *c.P;
  const Batch& B = c.B;
  const long long nc = fp.nc_of[bi];
  c.bw = d->spec ? d->spec_words.p : P.words.p + 2 * kAccWords + fp.words_per_batch * (bi / npipes);
  c.launch = 0;
  const int tb0 = bi * tpb, tb1 = (int)std::min<size_t>(fp.owned.size(), (size_t)(bi + 1) * tpb);
  const TileList TL{d->tiles_dev.p + (size_t)tb0, d->base_dev.p + (size_t)bi * (tpb + 1), tb1 - tb0,
                    c.ps->flags ? d->pix_dev.p + fp.pix_off[bi] : nullptr};
  c.live = cam_can_die(d) ? d->cam_live.p + bi : nullptr;
  c.zs = (c.p->z_channel && c.ps->d_depth) ? P.zs.p : nullptr;
  if (nc > 0) {  // else an adaptive pass with nothing to resample in this batch
    // one instantiation per shootRay; a perspective or architect camera runs
    // the first, whose per-sample code is the only one those scenes launch
    switch (d->cam_host.kind) {
      case YK_CAMERA_ORTHOGRAPHIC:
        launch(k_camera<YK_CAMERA_ORTHOGRAPHIC>, grid_for(nc), 256, 0, P.stream, TL, B, fp.R, nc, nullptr, nullptr);
        break;
      case YK_CAMERA_ANGULAR:
        launch(k_camera<YK_CAMERA_ANGULAR>, grid_for(nc), 256, 0, P.stream, TL, B, fp.R, nc, c.live, B.s_idx);
        break;
      default:
        launch(k_camera<YK_CAMERA_PERSPECTIVE>, grid_for(nc), 256, 0, P.stream, TL, B, fp.R, nc, nullptr, nullptr);
    }
    if (d->spec) {
      if (const int rc = enqueue_spec_generations(c, nc)) return rc;
    } else {
      enqueue_entries(c, B, fp.R, nc, 0);
    }
    if (c.live) launch(k_dead_samples, grid_for(nc), 256, 0, P.stream, B, nc);
  }
  // film: in batch order (tile order), whichever pipe ran the batch; an
  // empty batch keeps the chain of gather events
  if (bi > 0) HIPCHK(hipStreamWaitEvent(P.stream, d->gather_ev[(bi - 1) % kPipes], 0));
  launch_film_gather(P.stream, F, c.ps->flags ? d->pmap_dev.p : nullptr, tb0, tb1, fp.rect_of[bi], nc, B.samples, B.sxy,
                     TL.base, B.pext, c.d_film, film_options(c.p), c.zs, c.ps->d_depth);
  HIPCHK(hipEventRecord(d->gather_ev[bi % kPipes], P.stream));
  return YK_OK;
}

// After the last batch: accumulators back (synchronises every pipe), the
// watchdog's verdict, the YK_LAUNCH_LOG dump, timed launches, yk_stats.
int collect_stats(yk_device* d, const FramePlan& fp, const std::vector<Timed>& timed, long long samples_total,
                  std::chrono::steady_clock::time_point t0, yk_stats* st) {
  const int npipes = fp.plan.npipes;
  unsigned long long acc[kPipes][2 * kAccWords] = {};
  for (int pi = 0; pi < npipes; ++pi) {
    Pipe& P = d->pipe[pi];
    HIPCHK(hipMemcpyAsync(acc[pi], P.words.p, sizeof acc[pi], hipMemcpyDeviceToHost, P.stream));
    HIPCHK(hipStreamSynchronize(P.stream));
  }
  if (std::getenv("YK_LAUNCH_LOG") && !d->spec) {
    // diagnostic: rays of every traversal launch (queue-count words), per batch
    for (int bi = 0; bi < fp.plan.nbatch; ++bi) {
      std::vector<unsigned long long> q((size_t)fp.qwords_per_batch);
      HIPCHK(hipMemcpy(q.data(), d->pipe[bi % npipes].words.p + 2 * kAccWords + fp.words_per_batch * (bi / npipes),
                       q.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
      std::fprintf(stderr, "[launch-log] batch %d samples %lld:", bi, fp.nc_of[bi]);
      for (int w = 0; w < fp.qwords_per_batch; ++w)
        std::fprintf(stderr, " d%d shadow %llu next %llu;", w, q[w] & 0xFFFFFFFFull, q[w] >> 32);
      std::fprintf(stderr, "\n");
    }
  }
  yk_stats local{};
  yk_stats* S = st ? st : &local;
  for (int pi = 0; pi < npipes; ++pi) {
    if (acc[pi][2] || acc[pi][kAccWords + 2])
      return set_error(YK_ERR_INTERNAL, "kd-tree traversal watchdog fired (corrupt tree or stack)");
    add_trace_stats(S, true, acc[pi][3], acc[pi][0], acc[pi][1], 0.0, 0);
    add_trace_stats(S, false, acc[pi][kAccWords + 3], acc[pi][kAccWords], acc[pi][kAccWords + 1], 0.0, 0);
  }
  for (const Timed& t : timed) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, d->pipe[t.pipe].evpool[t.ev], d->pipe[t.pipe].evpool[t.ev + 1]));
    add_trace_stats(S, t.closest, 0, 0, 0, ms);
  }
  // camera samples that carry a ray: all of them, unless the camera can have
  // dead ones (the batches' live counts; the pipes are synchronised by now)
  if (cam_can_die(d)) {
    std::vector<unsigned long long> live((size_t)fp.plan.nbatch);
    HIPCHK(hipMemcpy(live.data(), d->cam_live.p, live.size() * sizeof live[0], hipMemcpyDeviceToHost));
    samples_total = 0;
    for (const unsigned long long n : live) samples_total += (long long)n;
  }
  S->camera_samples += (uint64_t)samples_total;
  S->ms_total += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return YK_OK;
}

int render_pass(yk_device* d, const yk_render_params* p, int32_t shard, int32_t nshards, float* d_film, yk_stats* st,
                const PassSpec& ps) {
  YK_GUARD_BEGIN
  if (const int rc = check_render_params(d, p, shard, nshards, d_film, ps)) return rc;
  HIPCHK(hipSetDevice(d->ordinal));
  bind_constants(d);
  const auto t0 = std::chrono::steady_clock::now();
  FramePlan fp;
  if (const char* why = build_frame_plan(d, p, shard, nshards, ps, fp)) return set_error(YK_ERR_UNSUPPORTED, why);
  const int nbatch = fp.plan.nbatch, npipes = fp.plan.npipes;
  d->last_plan = fp.plan;
  d->last_plan_valid = true;
  d->last_max_batches = (nbatch + npipes - 1) / npipes;
  upload_frame_plan(d, fp);
  if (cam_can_die(d)) {  // one live-sample count per batch, zero for a batch an abort leaves out
    d->cam_live.ensure((size_t)nbatch);
    HIPCHK(hipMemsetAsync(d->cam_live.p, 0, (size_t)nbatch * sizeof(unsigned long long), d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
  }
  Batch Bp[kPipes];
  bind_pipes(d, p, fp, Bp);
  std::vector<Timed> timed;
  size_t evn[kPipes] = {};
  BatchCtx c{d, p, &fp, &ps, d_film, bind_node_store(d, fp), &timed, evn, 0, nullptr, Batch{}, nullptr, 0};
  c.DC = DepthConst{p->normalize_z_channel ? 1 : 0, p->depth_min, p->depth_inv_range};
  long long samples_total = 0;
  bool aborted = false;
  for (int bi = 0; bi < nbatch; ++bi) {
    c.pi = bi % npipes;
    c.P = &d->pipe[c.pi];
    c.B = Bp[c.pi];
    if (d->abort_fn) {
      // abort polling between batches: this pipe's previous batch has
      // finished (the other pipes keep the GPU busy meanwhile)
      if (bi >= npipes) HIPCHK(hipStreamSynchronize(c.P->stream));
      if (d->abort_fn(d->abort_user)) {
        aborted = true;
        break;
      }
    }
    if (const int rc = enqueue_batch(c, bi)) return rc;
    samples_total += fp.nc_of[bi];
  }
  if (const int rc = collect_stats(d, fp, timed, samples_total, t0, st)) return rc;
  if (aborted) return set_error(YK_ERR_ABORTED, "render aborted by the abort callback");
  return YK_OK;
  YK_GUARD_END
}

// imageFilm_t::nextPass (imagefilm.cc:213-289) on the device: the pixels of
// `film` the next adaptive pass resamples, into host_flags (w * h bytes).
// nullptr when AA_threshold <= 0: doMoreSamples is always true.
const uint8_t* next_pass_flags(yk_device* d, const float* film, const yk_render_params* p,
                               std::vector<uint8_t>& host_flags) {
  if (!(p->aa_threshold > 0.f)) return nullptr;
  const int w = p->width, h = p->height;
  host_flags.resize((size_t)w * h);
  d->flags_dev.ensure(host_flags.size());
  HIPCHK(hipSetDevice(d->ordinal));
  HIPCHK(hipMemsetAsync(d->flags_dev.p, 0, host_flags.size(), d->stream));
  if (w > 1 && h > 1)
    launch(k_aa_flags, grid_for((long long)(w - 1) * (h - 1)), 256, 0, d->stream, film, w, h, p->aa_threshold,
           d->flags_dev.p);
  HIPCHK(hipMemcpyAsync(host_flags.data(), d->flags_dev.p, host_flags.size(), hipMemcpyDeviceToHost, d->stream));
  HIPCHK(hipStreamSynchronize(d->stream));
  return host_flags.data();
}

}  // namespace

extern "C" {

int yk_render_shard(yk_device* d, const yk_render_params* p, int32_t shard, int32_t nshards, float* d_film,
                    yk_stats* st) {
  if (!d || !p || !d_film || nshards < 1 || shard < 0 || shard >= nshards)
    return set_error(YK_ERR_ARG, "yk_render_shard: bad arguments");
  if (p->aa_passes < 1) return set_error(YK_ERR_ARG, "AA_passes must be >= 1");
  const int n0 = std::max(1, p->aa_samples);  // scene_t::setAntialiasing, scene.cc:736-742
  float* d_depth = p->z_channel ? p->depth_film : nullptr;  // device memory, as d_film is
  if (p->aa_passes == 1) return render_pass(d, p, shard, nshards, d_film, st, PassSpec{n0, 0, false, nullptr, d_depth});
  // tiledIntegrator_t::render, integrator.cc:132-170: pass 0 everywhere, then
  // AA_inc_samples more in the pixels imageFilm_t::nextPass flags
  if (nshards != 1)
    return set_error(YK_ERR_UNSUPPORTED, "AA_passes > 1 needs the whole film (nshards = 1): nextPass reads it");
  const int inc = p->aa_inc_samples > 0 ? p->aa_inc_samples : n0;
  int rc = render_pass(d, p, 0, 1, d_film, st, PassSpec{n0, 0, true, nullptr, d_depth});
  if (rc != YK_OK) return rc;  // YK_ERR_ABORTED included: no further passes
  YK_GUARD_BEGIN
  std::vector<uint8_t> flags;
  for (int pass = 1; pass < p->aa_passes; ++pass) {
    const uint8_t* fl = next_pass_flags(d, d_film, p, flags);
    // depth samples land in the resampled pixels alone, as the colour samples do
    rc = render_pass(d, p, 0, 1, d_film, st, PassSpec{inc, n0 + (pass - 1) * inc, true, fl, d_depth});
    if (rc != YK_OK) return rc;
  }
  return YK_OK;
  YK_GUARD_END
}

int yk_film_resolve(yk_device* d, const yk_render_params* p, const float* d_film, float* d_rgba) {
  if (!d || !p || !d_film || !d_rgba) return set_error(YK_ERR_ARG, "yk_film_resolve: NULL argument");
  YK_GUARD_BEGIN
  HIPCHK(hipSetDevice(d->ordinal));
  const long long npx = (long long)p->width * p->height;
  launch(k_film_resolve, grid_for(npx), 256, 0, d->stream, d_film, d_rgba, npx, p->premult_alpha ? 1 : 0);
  HIPCHK(hipStreamSynchronize(d->stream));
  return YK_OK;
  YK_GUARD_END
}

int yk_depth_resolve(yk_device* d, const yk_render_params* p, const float* d_depth, float* d_z) {
  if (!d || !p || !d_depth || !d_z) return set_error(YK_ERR_ARG, "yk_depth_resolve: NULL argument");
  if (p->width <= 0 || p->height <= 0) return set_error(YK_ERR_ARG, "empty render area");
  YK_GUARD_BEGIN
  HIPCHK(hipSetDevice(d->ordinal));
  const long long npx = (long long)p->width * p->height;
  launch(k_depth_resolve, grid_for(npx), 256, 0, d->stream, d_depth, d_z, npx);
  HIPCHK(hipStreamSynchronize(d->stream));
  return YK_OK;
  YK_GUARD_END
}

// tiledIntegrator_t::precalcDepths (integrator.cc:99-130) and the maxDepth /
// minDepth it starts from (integrator.cc:150-151).
int yk_depth_range(yk_device* d, const yk_render_params* p, float* min_out, float* inv_range_out) {
  if (!d || !p || !min_out || !inv_range_out) return set_error(YK_ERR_ARG, "yk_depth_range: NULL argument");
  if (!d->uploaded) return set_error(YK_ERR_STATE, "yk_depth_range: no scene uploaded");
  float min_depth = 1e38f, max_depth = 0.f;
  YK_GUARD_BEGIN
  if (d->cam_has_clip && d->cam_far_clip > -1) {
    min_depth = d->cam_near_clip;
    max_depth = d->cam_far_clip;
  } else {
    // a sample outside a circular angular camera's circle is traced with an
    // uninitialised direction there: nothing to restate
    if (cam_can_die(d))
      return set_error(YK_ERR_UNSUPPORTED,
                       "yk_depth_range: a circular angular camera without a far clip (the reference traces its "
                       "samples outside the circle with an uninitialised direction)");
    const long long n = (long long)d->cam_resx * d->cam_resy;
    if (d->cam_resx <= 0 || d->cam_resy <= 0 || n > (1ll << 28))
      return set_error(YK_ERR_ARG, "yk_depth_range: the camera's resolution is empty or too large");
    HIPCHK(hipSetDevice(d->ordinal));
    bind_constants(d);
    DBuf<yk_ray> rays;
    DBuf<yk_hit> hits;
    DBuf<unsigned> mm;
    rays.ensure((size_t)n);
    hits.ensure((size_t)n);
    mm.ensure(2);
    float init[2] = {0.f, 1e38f};
    HIPCHK(hipMemcpy(mm.p, init, sizeof init, hipMemcpyHostToDevice));
    auto* shoot = d->cam_host.kind == YK_CAMERA_ORTHOGRAPHIC ? k_depth_range_rays<YK_CAMERA_ORTHOGRAPHIC>
                  : d->cam_host.kind == YK_CAMERA_ANGULAR    ? k_depth_range_rays<YK_CAMERA_ANGULAR>
                                                             : k_depth_range_rays<YK_CAMERA_PERSPECTIVE>;
    launch(shoot, grid_for(n), 256, 0, d->stream, d->cam_resx, d->cam_resy, rays.p);
    yk_stats local{};
    launch_trace<true>(d, d->pipe[0], rays.p, n, hits.p, nullptr, &local);  // d->stream is pipe 0's
    launch(k_depth_range_reduce, grid_for(n), 256, 0, d->stream, (const yk_ray*)rays.p, (const yk_hit*)hits.p, n, mm.p);
    HIPCHK(hipStreamSynchronize(d->stream));
    float out[2];
    HIPCHK(hipMemcpy(out, mm.p, sizeof out, hipMemcpyDeviceToHost));
    max_depth = out[0];
    min_depth = out[1];
  }
  if (max_depth > 0.f) max_depth = 1.f / (max_depth - min_depth);
  *min_out = min_depth;
  *inv_range_out = max_depth;
  return YK_OK;
  YK_GUARD_END
}

int yk_render_film(yk_device* d, const yk_render_params* p, int32_t shard, int32_t nshards, float* film_host,
                   yk_stats* st) {
  if (!d || !p || !film_host) return set_error(YK_ERR_ARG, "yk_render_film: NULL argument");
  if (p->width <= 0 || p->height <= 0) return set_error(YK_ERR_ARG, "empty render area");
  if (const int rc = check_depth_params(p)) return rc;
  YK_GUARD_BEGIN
  HIPCHK(hipSetDevice(d->ordinal));
  const size_t npx = (size_t)p->width * p->height;
  DBuf<float> film, depth;
  film.ensure(npx * 5);
  HIPCHK(hipMemsetAsync(film.p, 0, npx * 5 * sizeof(float), d->stream));
  yk_render_params q = *p;
  if (p->z_channel) {  // the depth film is host memory here: a device film of the call's own
    depth.ensure(npx * 2);
    HIPCHK(hipMemsetAsync(depth.p, 0, npx * 2 * sizeof(float), d->stream));
    q.depth_film = depth.p;
  }
  const int rc = yk_render_shard(d, &q, shard, nshards, film.p, st);
  if (rc != YK_OK) return rc;
  HIPCHK(hipMemcpy(film_host, film.p, npx * 5 * sizeof(float), hipMemcpyDeviceToHost));
  if (p->z_channel) HIPCHK(hipMemcpy(p->depth_film, depth.p, npx * 2 * sizeof(float), hipMemcpyDeviceToHost));
  return YK_OK;
  YK_GUARD_END
}

// Whole frame on ndev devices (tiledIntegrator_t::render's threads,
// integrator.cc:177-211, one host thread per device): device i renders the
// tiles t % ndev == i into its own film; the films are reduced into device
// 0's by peer copies over xGMI (hipMemcpyPeerAsync) and one add per shard,
// in shard order. Adaptive passes (AA_passes > 1): after every pass the
// reduced film gives imageFilm_t::nextPass's flags (k_aa_flags, imagefilm.cc:
// 213-289), which every device then resamples in its own tiles.
int yk_render_multi(yk_device* const* devs, int32_t ndev, const yk_render_params* p, float* film_host,
                    yk_stats* st) {
  if (!devs || ndev < 1 || !p || !film_host) return set_error(YK_ERR_ARG, "yk_render_multi: bad arguments");
  if (ndev > kMaxMultiDev) return set_error(YK_ERR_UNSUPPORTED, "yk_render_multi: at most 16 devices");
  for (int i = 0; i < ndev; ++i) {
    if (!devs[i]) return set_error(YK_ERR_ARG, "yk_render_multi: NULL device");
    if (!devs[i]->uploaded) return set_error(YK_ERR_STATE, "yk_render_multi: a device has no scene uploaded");
    for (int j = 0; j < i; ++j)
      if (devs[j] == devs[i]) return set_error(YK_ERR_ARG, "yk_render_multi: a device handle is listed twice");
    // one frame = one scene: the same uploaded scene generation everywhere
    // (handles on one GPU share its constant memory, and shards of different
    // scenes would be summed into one film)
    if (devs[i]->uploaded_gen != devs[0]->uploaded_gen || !same_constants(devs[i], devs[0]))
      return set_error(YK_ERR_STATE,
                       "yk_render_multi: the devices hold different scenes (upload the same scene to all)");
    if (needs_photon_maps(p) && (!devs[i]->pm_ready || devs[i]->pm_integrator != p->integrator ||
                 std::memcmp(&devs[i]->pm_params, &p->photon, sizeof(yk_photon_params)) != 0))
      return set_error(YK_ERR_STATE, "yk_render_multi: device " + std::to_string(i) +
                                         " has no photon maps built with these parameters (yk_photon_build)");
  }
  if (p->aa_passes < 1) return set_error(YK_ERR_ARG, "AA_passes must be >= 1");
  if (p->width <= 0 || p->height <= 0) return set_error(YK_ERR_ARG, "empty render area");
  if (const int rc = check_depth_params(p)) return rc;
  YK_GUARD_BEGIN
  const size_t npx = (size_t)p->width * p->height, nfl = npx * 5;
  // z_channel: every device keeps a shard depth film next to its shard film,
  // reduced the same way (k_film_sum, shard order) into p->depth_film (host)
  const bool zch = p->z_channel != 0;
  const size_t ndf = npx * 2;
  yk_device* d0 = devs[0];
  // shard films and reduce buffers live on the handles: sized once, reused
  for (int i = 0; i < ndev; ++i) {
    HIPCHK(hipSetDevice(devs[i]->ordinal));
    devs[i]->mfilm.ensure(nfl);
    HIPCHK(hipMemsetAsync(devs[i]->mfilm.p, 0, nfl * sizeof(float), devs[i]->stream));
    if (zch) {
      devs[i]->mdepth.ensure(ndf);
      HIPCHK(hipMemsetAsync(devs[i]->mdepth.p, 0, ndf * sizeof(float), devs[i]->stream));
    }
    HIPCHK(hipStreamSynchronize(devs[i]->stream));
    if (devs[i]->ordinal != d0->ordinal) {  // direct xGMI access where the pair allows it
      int can = 0;
      HIPCHK(hipDeviceCanAccessPeer(&can, d0->ordinal, devs[i]->ordinal));
      if (can) {
        HIPCHK(hipSetDevice(d0->ordinal));
        const hipError_t e = hipDeviceEnablePeerAccess(devs[i]->ordinal, 0);
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) HIPCHK(e);
        (void)hipGetLastError();
      }
    }
  }
  HIPCHK(hipSetDevice(d0->ordinal));
  d0->macc.ensure(nfl);
  if (zch) d0->mdacc.ensure(ndf);
  FilmShards FS{}, FSD{};
  FS.n = FSD.n = ndev;
  // YK_MULTI_STAGE_ALL=1 (test only): shards on d0's own GPU also take the
  // peer path (staging film, copy stream, event), so one-GPU boxes run it
  const bool stage_all = [] {
    const char* e = std::getenv("YK_MULTI_STAGE_ALL");
    return e && e[0] == '1';
  }();
  auto staged = [&](int i) { return i > 0 && (devs[i]->ordinal != d0->ordinal || stage_all); };
  for (int i = 0; i < ndev; ++i) {
    // a shard on d0's own GPU is read in place; a peer GPU's film is copied
    // into a staging film first, on a copy stream of its own
    if (!staged(i)) {
      FS.f[i] = devs[i]->mfilm.p;
      FSD.f[i] = zch ? devs[i]->mdepth.p : nullptr;
      continue;
    }
    d0->mstage[i].ensure(nfl);
    if (zch) {
      d0->mdstage[i].ensure(ndf);
      FSD.f[i] = d0->mdstage[i].p;
    }
    if (!d0->mstream[i]) HIPCHK(hipStreamCreateWithFlags(&d0->mstream[i], hipStreamNonBlocking));
    if (!d0->mevent[i]) HIPCHK(hipEventCreateWithFlags(&d0->mevent[i], hipEventDisableTiming));
    FS.f[i] = d0->mstage[i].p;
  }
  std::vector<yk_stats> sts(ndev);
  double ms_reduce = 0.0;
  // one pass on every device, each in its own host thread
  auto run = [&](const PassSpec& ps) -> int {
    std::vector<int> rc(ndev, YK_OK);
    std::vector<std::string> msg(ndev);
    std::vector<std::thread> th;
    for (int i = 0; i < ndev; ++i)
      th.emplace_back([&, i] {
        PassSpec psi = ps;
        psi.d_depth = zch ? devs[i]->mdepth.p : nullptr;
        rc[i] = render_pass(devs[i], p, i, ndev, devs[i]->mfilm.p, &sts[i], psi);
        if (rc[i] != YK_OK) msg[i] = yk_last_error();
      });
    for (auto& t : th) t.join();
    int out = YK_OK;
    for (int i = 0; i < ndev; ++i) {
      if (rc[i] == YK_OK) continue;
      if (rc[i] != YK_ERR_ABORTED) return set_error(rc[i], "device " + std::to_string(i) + ": " + msg[i]);
      out = YK_ERR_ABORTED;
    }
    return out;
  };
  // acc = film[0] + film[1] + ... (shard order) on device 0: every peer copy
  // is in flight at once (one stream each), then one summing pass
  auto reduce = [&]() {
    const auto t0 = std::chrono::steady_clock::now();
    HIPCHK(hipSetDevice(d0->ordinal));
    hipStream_t s0 = d0->stream;
    for (int i = 1; i < ndev; ++i) {
      if (!staged(i)) continue;
      HIPCHK(hipMemcpyPeerAsync(d0->mstage[i].p, d0->ordinal, devs[i]->mfilm.p, devs[i]->ordinal, nfl * sizeof(float),
                                d0->mstream[i]));
      if (zch)
        HIPCHK(hipMemcpyPeerAsync(d0->mdstage[i].p, d0->ordinal, devs[i]->mdepth.p, devs[i]->ordinal,
                                  ndf * sizeof(float), d0->mstream[i]));
      HIPCHK(hipEventRecord(d0->mevent[i], d0->mstream[i]));
      HIPCHK(hipStreamWaitEvent(s0, d0->mevent[i], 0));
    }
    launch(k_film_sum, grid_for(((long long)nfl + 3) / 4), 256, 0, s0, d0->macc.p, FS, (long long)nfl);
    if (zch) launch(k_film_sum, grid_for(((long long)ndf + 3) / 4), 256, 0, s0, d0->mdacc.p, FSD, (long long)ndf);
    HIPCHK(hipStreamSynchronize(s0));
    ms_reduce += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  };
  const int n0 = std::max(1, p->aa_samples);  // scene_t::setAntialiasing, scene.cc:736-742
  const bool multipass = p->aa_passes > 1;
  int rc = run(PassSpec{n0, 0, multipass, nullptr});
  if (rc != YK_OK && rc != YK_ERR_ABORTED) return rc;
  reduce();
  if (multipass && rc == YK_OK) {
    const int inc = p->aa_inc_samples > 0 ? p->aa_inc_samples : n0;
    std::vector<uint8_t> flags;
    for (int pass = 1; pass < p->aa_passes; ++pass) {
      const uint8_t* fl = next_pass_flags(d0, d0->macc.p, p, flags);
      rc = run(PassSpec{inc, n0 + (pass - 1) * inc, true, fl});
      if (rc != YK_OK && rc != YK_ERR_ABORTED) return rc;
      reduce();
      if (rc == YK_ERR_ABORTED) break;
    }
  }
  HIPCHK(hipSetDevice(d0->ordinal));
  HIPCHK(hipMemcpy(film_host, d0->macc.p, nfl * sizeof(float), hipMemcpyDeviceToHost));
  if (zch) HIPCHK(hipMemcpy(p->depth_film, d0->mdacc.p, ndf * sizeof(float), hipMemcpyDeviceToHost));
  if (st) {
    for (const yk_stats& x : sts) {
      add_trace_stats(st, true, x.closest_rays, x.closest_nodes, x.closest_tris, x.ms_closest, x.closest_launches);
      add_trace_stats(st, false, x.shadow_rays, x.shadow_nodes, x.shadow_tris, x.ms_shadow, x.shadow_launches);
      st->camera_samples += x.camera_samples;
      st->ms_total = std::max(st->ms_total, x.ms_total);
    }
    st->ms_reduce += ms_reduce;
  }
  if (rc == YK_ERR_ABORTED)
    return set_error(rc, "render aborted by the abort callback (film holds the finished batches)");
  return YK_OK;
  YK_GUARD_END
}

int yk_render(yk_device* d, const yk_render_params* p, float* rgba_host, yk_stats* st) {
  if (!d || !p || !rgba_host) return set_error(YK_ERR_ARG, "yk_render: NULL argument");
  YK_GUARD_BEGIN
  HIPCHK(hipSetDevice(d->ordinal));
  const size_t npx = (size_t)p->width * p->height;
  DBuf<float> film, rgba;
  film.ensure(npx * 5);
  rgba.ensure(npx * 4);
  HIPCHK(hipMemsetAsync(film.p, 0, npx * 5 * sizeof(float), d->stream));
  yk_render_params q = *p;  // RGBA only: no depth film is produced here
  q.z_channel = 0;
  int rc = yk_render_shard(d, &q, 0, 1, film.p, st);
  if (rc == YK_OK) rc = yk_film_resolve(d, &q, film.p, rgba.p);
  if (rc == YK_OK) HIPCHK(hipMemcpy(rgba_host, rgba.p, npx * 4 * sizeof(float), hipMemcpyDeviceToHost));
  return rc;
  YK_GUARD_END
}

}  // extern "C"
