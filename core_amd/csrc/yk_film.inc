// The image film on gfx950 (included by yk_device.hip inside namespace yk,
// after yk_spec.inc): FilmConst, k_pixel_extent, the colour and depth gathers
// (film_gather_walk), the depth channel's sample and range kernels,
// k_film_sum over the shards of several GPUs, k_aa_flags and the two
// resolves. Depends on yk_ray, the cameras' cam_shoot (k_depth_range_rays)
// and yk_math.h; the host fills FilmConst in make_film (yk_film_host.inc).

// ------------------------------------------------------------ film

struct FilmConst {
  int cx0, cy0, cx1, cy1, w, h;  // film area (imagefilm.cc:119-127)
  int tile, ntx;                 // tile size, tiles per row (imagesplitter.cc:29-53)
  float filterw;
  double tableScale;
  int olo_x, ohi_x, olo_y, ohi_y;  // target-source offset window
  int shard, nshards;
  int tb0, tb1;                  // batch = owned tile ranks [tb0, tb1)
  const int* rank_of;            // custom tile order: rank of each tile in the shard's list (-1: not owned); null: row-major
  int spp;
  float d1;
  const int* pmap;  // adaptive pass: batch-local first sample of each film pixel, -1 = not resampled
  float table[256];
};

__device__ __forceinline__ int round2int(double v) { return (int)(v + (0.5 - 1.4e-11)); }
constexpr int kGatherGroup = 8;  // samples loaded per group (16 measured equal)
__device__ __forceinline__ int floor2int(double v) { return (int)floor(v); }

// Footprint extent of every source pixel of a batch: over its samples, the
// smallest dx0 / dy0 and the largest dx1 / dy1 of addSample's target window
// (the same Round2Int expressions as the gather). A target offset outside
// them can take no sample of the pixel, so the gather skips the pixel's
// sample loop: with a box filter a pixel's samples reach its 8 neighbours
// almost never, and those loops were ~8/9 of the gather's work. One wave per
// pixel slot (slot i = samples [i*spp, (i+1)*spp) of the batch).
__global__ void __launch_bounds__(256) k_pixel_extent(FilmConst F, const float2* __restrict__ sxy,
                                                      char4* __restrict__ ext, long long npix) {
  const long long slot = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (slot >= npix) return;
  int x0 = 127, x1 = -128, y0 = 127, y1 = -128;
  for (int s = lane; s < F.spp; s += 64) {
    const float2 d = sxy[slot * F.spp + s];
    const double dx = d.x, dy = d.y;
    x0 = min(x0, round2int(dx - F.filterw));
    x1 = max(x1, round2int(dx + F.filterw - 1.0));
    y0 = min(y0, round2int(dy - F.filterw));
    y1 = max(y1, round2int(dy + F.filterw - 1.0));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    x0 = min(x0, __shfl_xor(x0, off));
    x1 = max(x1, __shfl_xor(x1, off));
    y0 = min(y0, __shfl_xor(y0, off));
    y1 = max(y1, __shfl_xor(y1, off));
  }
  if (lane == 0) ext[slot] = make_char4((signed char)x0, (signed char)x1, (signed char)y0, (signed char)y1);
}

// What a gather adds up, as a policy of the shared walk (film_gather_walk):
// the sample type, the pixel's sums (loaded from and stored to the film) and
// the per-contribution arithmetic. GatherColour<false, false> is the film of
// every render without film options, with the arithmetic the gather has
// always had; the other instantiations are chosen on the host
// (launch_film_gather) and cost those renders nothing.
//
// CLAMP: colorA_t::clampRGB01 once per sample, on load (imagefilm.cc:457,
// color.h:119-124; a NaN passes both comparisons and stays). PREMULT:
// addSample premultiplies its local copy inside the pixel loop (imagefilm.cc:
// 502), so the m-th pixel of the sample's window, row-major after the clamp
// to the film area, takes the colour after m sequential RGB *= A.
template <bool CLAMP, bool PREMULT>
struct GatherColour {
  using Sample = float4;
  static constexpr bool kPremult = PREMULT;
  static constexpr int kStride = 5;
  float aR, aG, aB, aA, aW;
  __device__ __forceinline__ void load(const float* px) {
    aR = px[0];
    aG = px[1];
    aB = px[2];
    aA = px[3];
    aW = px[4];
  }
  __device__ __forceinline__ void store(float* px) const {
    px[0] = aR;
    px[1] = aG;
    px[2] = aB;
    px[3] = aA;
    px[4] = aW;
  }
  static __device__ __forceinline__ Sample none() { return make_float4(0.f, 0.f, 0.f, 0.f); }
  static __device__ __forceinline__ Sample fetch(const Sample* __restrict__ s, long long i) {
    float4 c = s[i];
    if constexpr (CLAMP) {
      c.x = c.x < 0.f ? 0.f : (c.x > 1.f ? 1.f : c.x);
      c.y = c.y < 0.f ? 0.f : (c.y > 1.f ? 1.f : c.y);
      c.z = c.z < 0.f ? 0.f : (c.z > 1.f ? 1.f : c.z);
    }
    return c;
  }
  // -> whether the contribution counts
  __device__ __forceinline__ bool add(float wt, Sample c, int m) {
    if constexpr (PREMULT) {
      for (int i = 0; i < m; ++i) {
        c.x = c.x * c.w;
        c.y = c.y * c.w;
        c.z = c.z * c.w;
      }
    }
    aR = aR + wt * c.x;
    aG = aG + wt * c.y;
    aB = aB + wt * c.z;
    aA = aA + wt * c.w;
    aW = aW + wt;
    return true;
  }
};

// imageFilm_t::addDepthSample (imagefilm.cc:513-564): one colour channel's
// arithmetic plus the weight, on a film of {val, weight}. A NaN is a sample
// without a depth value (k_depth_samples): it adds nothing, weight included.
struct GatherDepth {
  using Sample = float;
  static constexpr bool kPremult = false;
  static constexpr int kStride = 2;
  float aV, aW;
  __device__ __forceinline__ void load(const float* px) {
    aV = px[0];
    aW = px[1];
  }
  __device__ __forceinline__ void store(float* px) const {
    px[0] = aV;
    px[1] = aW;
  }
  static __device__ __forceinline__ Sample none() { return 0.f; }
  static __device__ __forceinline__ Sample fetch(const Sample* __restrict__ s, long long i) { return s[i]; }
  __device__ __forceinline__ bool add(float wt, Sample v, int) {
    if (v != v) return false;
    aV = aV + wt * v;
    aW = aW + wt;
    return true;
  }
};

// imageFilm_t::addSample as a gather (imagefilm.cc:453-511): each thread owns
// one target pixel and adds every covering sample of the batch in the
// reference's single-thread order -- tiles in the order the film hands them
// out (row-major, or the tile_order list), then rows, columns and samples --
// so the float sums match the sequential CPU splat bit for bit.
// Candidate sources are walked in that order directly: the tiles the filter
// window touches in row-major tile order, inside each its window rows and
// columns. The walk is shared by the colour film and the depth film (Acc).
template <class Acc>
__device__ __forceinline__ void film_gather_walk(const FilmConst& F, const typename Acc::Sample* __restrict__ samples,
                                                 const float2* __restrict__ sxy, const int* __restrict__ tile_base,
                                                 const char4* __restrict__ ext, float* __restrict__ film, int rx0,
                                                 int ry0, int rw, int rh) {
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= rw * rh) return;
  const int tx = rx0 + tid % rw, ty = ry0 + tid / rw;
  if (tx < F.cx0 || tx >= F.cx1 || ty < F.cy0 || ty >= F.cy1) return;
  // sources s with target - s in [olo, ohi]
  const int sx0 = max(F.cx0, tx - F.ohi_x), sx1 = min(F.cx1 - 1, tx - F.olo_x);
  const int sy0 = max(F.cy0, ty - F.ohi_y), sy1 = min(F.cy1 - 1, ty - F.olo_y);
  if (sx0 > sx1 || sy0 > sy1) return;
  const int tc0 = (sx0 - F.cx0) / F.tile, tc1 = (sx1 - F.cx0) / F.tile;
  const int tr0 = (sy0 - F.cy0) / F.tile, tr1 = (sy1 - F.cy0) / F.tile;
  float* px = film + Acc::kStride * ((size_t)(ty - F.cy0) * F.w + (tx - F.cx0));
  Acc a;
  a.load(px);
  bool any = false;
  // one tile of the batch: its source pixels in the window, rows, columns, samples
  auto tile = [&](int tr, int tc, int rank) {
      const int X = F.cx0 + tc * F.tile, Y = F.cy0 + tr * F.tile;
      const int W = min(F.tile, F.cx1 - X);
      const int ya = max(sy0, Y), yb = min(sy1, Y + F.tile - 1);
      const int xa = max(sx0, X), xb = min(sx1, X + F.tile - 1);
      const long long tb = tile_base[rank - F.tb0];
      for (int sy = ya; sy <= yb; ++sy)
        for (int sx = xa; sx <= xb; ++sx) {
          long long cbase;
          if (F.pmap) {
            cbase = F.pmap[(size_t)(sy - F.cy0) * F.w + (sx - F.cx0)];
            if (cbase < 0) continue;
          } else {
            cbase = tb + (long long)((sy - Y) * W + (sx - X)) * F.spp;
          }
          const int ox = tx - sx, oy = ty - sy;
          {  // no sample of this source pixel reaches the target (k_pixel_extent)
            const char4 e = ext[cbase / F.spp];
            if (ox < e.x || ox > e.y || oy < e.z || oy > e.w) continue;
          }
          // samples in groups of kGatherGroup: the group's positions, then the
          // colours of the accepted ones, are loaded together (independent
          // loads in flight instead of one dependent round trip per sample);
          // the sums still run sample by sample in order
          for (int s0 = 0; s0 < F.spp; s0 += kGatherGroup) {
            float2 dd[kGatherGroup];
#pragma unroll
            for (int k = 0; k < kGatherGroup; ++k)
              dd[k] = (s0 + k < F.spp) ? sxy[cbase + s0 + k] : make_float2(-8.f, -8.f);
            float wt[kGatherGroup];
            bool acc[kGatherGroup];
            int mm[Acc::kPremult ? kGatherGroup : 1];
#pragma unroll
            for (int k = 0; k < kGatherGroup; ++k) {
              const double dx = dd[k].x, dy = dd[k].y;
              const int dx0 = round2int(dx - F.filterw), dx1 = round2int(dx + F.filterw - 1.0);
              const int dy0 = round2int(dy - F.filterw), dy1 = round2int(dy + F.filterw - 1.0);
              // film-edge clamps (cx0 - x etc.) hold by construction: tx, ty lie inside the film
              acc[k] = s0 + k < F.spp && !(ox < dx0 || ox > dx1 || oy < dy0 || oy > dy1);
              wt[k] = 0.f;
              if (acc[k]) {
                const int xi = floor2int(fabs(((double)ox - (dx - 0.5)) * F.tableScale));
                const int yi = floor2int(fabs(((double)oy - (dy - 0.5)) * F.tableScale));
                wt[k] = F.table[yi * 16 + xi];
                if constexpr (Acc::kPremult) {
                  // the target's place in the sample's window after the clamp
                  // to the film area, row-major from 1 (imagefilm.cc:463-466, 492-502)
                  const int wx0 = max(F.cx0 - sx, dx0), wx1 = min(F.cx1 - sx - 1, dx1);
                  const int wy0 = max(F.cy0 - sy, dy0);
                  mm[k] = (oy - wy0) * (wx1 - wx0 + 1) + (ox - wx0) + 1;
                }
              }
            }
            typename Acc::Sample col[kGatherGroup];
#pragma unroll
            for (int k = 0; k < kGatherGroup; ++k)
              col[k] = acc[k] ? Acc::fetch(samples, cbase + s0 + k) : Acc::none();
#pragma unroll
            for (int k = 0; k < kGatherGroup; ++k) {
              if (!acc[k]) continue;
              if (a.add(wt[k], col[k], Acc::kPremult ? mm[k] : 0)) any = true;
            }
          }
        }
  };
  if (F.rank_of) {
    // custom order (tiles_order "random"): the window's tiles of the batch by
    // rank, the smallest rank above the previous one each time
    int last = -1;
    for (;;) {
      int best = INT_MAX, btr = 0, btc = 0;
      for (int r = tr0; r <= tr1; ++r)
        for (int q = tc0; q <= tc1; ++q) {
          const int k = F.rank_of[r * F.ntx + q];
          if (k > last && k >= F.tb0 && k < F.tb1 && k < best) {
            best = k;
            btr = r;
            btc = q;
          }
        }
      if (best == INT_MAX) break;
      last = best;
      tile(btr, btc, best);
    }
  } else {
    for (int tr = tr0; tr <= tr1; ++tr)  // row-major tiles
      for (int tc = tc0; tc <= tc1; ++tc) {
        const int ti = tr * F.ntx + tc;
        if (ti % F.nshards != F.shard) continue;
        const int rank = ti / F.nshards;
        if (rank < F.tb0 || rank >= F.tb1) continue;
        tile(tr, tc, rank);
      }
  }
  if (!any) return;
  a.store(px);
}

template <bool CLAMP, bool PREMULT>
__global__ void __launch_bounds__(256) k_film_gather(FilmConst F, const float4* __restrict__ samples,
                                                     const float2* __restrict__ sxy, const int* __restrict__ tile_base,
                                                     const char4* __restrict__ ext, float* __restrict__ film,
                                                     int rx0, int ry0, int rw, int rh) {
  film_gather_walk<GatherColour<CLAMP, PREMULT>>(F, samples, sxy, tile_base, ext, film, rx0, ry0, rw, rh);
}

// The depth film's gather: the same walk over the batch's depth samples.
__global__ void __launch_bounds__(256) k_depth_gather(FilmConst F, const float* __restrict__ depths,
                                                      const float2* __restrict__ sxy, const int* __restrict__ tile_base,
                                                      const char4* __restrict__ ext, float* __restrict__ film,
                                                      int rx0, int ry0, int rw, int rh) {
  film_gather_walk<GatherDepth>(F, depths, sxy, tile_base, ext, film, rx0, ry0, rw, rh);
}

// The depth sample of every camera sample of a batch (renderTile,
// integrator.cc:313-334), after the batch's primary closest-hit launch:
// c_ray.tmax is the camera hit's t (scene_t::intersect stores it, scene.cc:
// 877), on a miss what shootRay left, the far plane's distance. Raw: tmax,
// 99999997952.f where it is <= 0. Normalised: 1 - (tmax - minDepth) * maxDepth
// where tmax > 0, else 0 (source order; contraction is off). A sample
// without a ray (wt = 0, an angular camera's; cam_shoot gives it direction 0)
// reaches `continue` before this point: NaN, which the gather skips.
struct DepthConst {
  int normalize;
  float dmin, dinv;
};
__global__ void __launch_bounds__(256) k_depth_samples(const yk_ray* __restrict__ rays,
                                                       const yk_hit* __restrict__ hits, float* __restrict__ out,
                                                       DepthConst D, long long nc) {
  const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const yk_ray r = rays[c];
  const yk_hit h = hits[c];
  float depth;
  if (r.dir[0] == 0.f && r.dir[1] == 0.f && r.dir[2] == 0.f && r.tmin == 0.f && r.tmax == -1.0f) {
    depth = __int_as_float(0x7fc00000);
  } else {
    const float tmax = h.prim >= 0 ? h.t : r.tmax;
    if (D.normalize) {
      depth = 0.f;
      if (tmax > 0.f) depth = 1.f - (tmax - D.dmin) * D.dinv;
    } else {
      depth = tmax;
      if (depth <= 0.f) depth = 99999997952.f;
    }
  }
  out[c] = depth;
}

// precalcDepths' rays (integrator.cc:116-121): shootRay(i, j, 0.5, 0.5) for
// i < resY, j < resX -- the row index goes in as px -- in that order.
template <int KIND>
__global__ void __launch_bounds__(256) k_depth_range_rays(int resx, int resy, yk_ray* __restrict__ rays) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)resx * resy) return;
  const int i = (int)(t / resx), j = (int)(t % resx);
  yk_ray r;
  cam_shoot<KIND>((float)i, (float)j, 0.5f, 0.5f, r);
  rays[t] = r;
}

// precalcDepths' min / max (integrator.cc:122-124) over the traced rays:
// tmax = the hit's t, else the ray's own. Both are order-independent:
// maxDepth starts at 0 and minDepth takes only tmax >= 0, so every value
// that can win is a non-negative float, and those order as their bits do.
// mm[0]: max bits (from 0), mm[1]: min bits (from 1e38f's).
__global__ void __launch_bounds__(256) k_depth_range_reduce(const yk_ray* __restrict__ rays,
                                                            const yk_hit* __restrict__ hits, long long n,
                                                            unsigned* __restrict__ mm) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned hi = 0u, lo = 0xFFFFFFFFu;
  if (t < n) {
    const yk_hit h = hits[t];
    float tmax = h.prim >= 0 ? h.t : rays[t].tmax;
    if (tmax == 0.f) tmax = 0.f;  // -0 compares >= 0: its place is +0's
    if (tmax >= 0.f) hi = lo = (unsigned)__float_as_int(tmax);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    hi = max(hi, (unsigned)__shfl_xor((int)hi, off));
    lo = min(lo, (unsigned)__shfl_xor((int)lo, off));
  }
  if ((threadIdx.x & 63) == 0) {
    if (hi != 0u) atomicMax(mm, hi);
    if (lo != 0xFFFFFFFFu) atomicMin(mm + 1, lo);
  }
}

// yk_render_multi's reduce: acc = ((f[0] + f[1]) + f[2]) + ... in shard
// order, one pass over all shard films (each element summed in the order the
// sequential reduce added them, so the result does not depend on how the
// copies were scheduled). Four floats per thread where the range allows.
constexpr int kMaxMultiDev = 16;
struct FilmShards {
  const float* f[kMaxMultiDev];
  int n;
};
__global__ void __launch_bounds__(256) k_film_sum(float* __restrict__ acc, FilmShards S, long long n) {
  const long long i4 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i4 >= n) return;
  if (i4 + 4 <= n) {
    float4 a = *reinterpret_cast<const float4*>(S.f[0] + i4);
    for (int k = 1; k < S.n; ++k) {
      const float4 b = *reinterpret_cast<const float4*>(S.f[k] + i4);
      a = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
    }
    *reinterpret_cast<float4*>(acc + i4) = a;
    return;
  }
  for (long long i = i4; i < n; ++i) {
    float a = S.f[0][i];
    for (int k = 1; k < S.n; ++k) a = a + S.f[k][i];
    acc[i] = a;
  }
}

// imageFilm_t::nextPass (imagefilm.cc:213-271): flag the pixels whose
// brightness differs from a neighbour's by >= threshold. Compiled form: the
// centre as abscol2bri of col*(1/w); each neighbour folded as
// |(c - (0.0722*B)*inv) - (0.7152*G + 0.2126*R)*inv|, |c| when its weight is 0.
__global__ void k_aa_flags(const float* __restrict__ film, int w, int h, float thr, uint8_t* __restrict__ flags) {
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= (w - 1) * (h - 1)) return;
  const int x = tid % (w - 1), y = tid / (w - 1);
  const float* a = film + 5 * ((size_t)y * w + x);
  float c = 0.f;
  if (a[4] > 0.f) {
    const float inv = 1.0f / a[4];
    c = (0.2126f * fabsf(a[0] * inv) + 0.7152f * fabsf(a[1] * inv)) + 0.0722f * fabsf(a[2] * inv);
  }
  auto differs = [&](int nx, int ny) {
    const float* b = film + 5 * ((size_t)ny * w + nx);
    float d = c;
    if (b[4] > 0.f) {
      const float inv = 1.0f / b[4];
      d = (c - (0.0722f * b[2]) * inv) - (0.2126f * b[0] + 0.7152f * b[1]) * inv;
    }
    return fabsf(d) >= thr;
  };
  bool need = false;
  if (differs(x + 1, y)) { need = true; flags[(size_t)y * w + x + 1] = 1; }
  if (differs(x, y + 1)) { need = true; flags[(size_t)(y + 1) * w + x] = 1; }
  if (differs(x + 1, y + 1)) { need = true; flags[(size_t)(y + 1) * w + x + 1] = 1; }
  if (x > 0 && differs(x - 1, y + 1)) { need = true; flags[(size_t)(y + 1) * w + x - 1] = 1; }
  if (need) flags[(size_t)y * w + x] = 1;
}

// imageFilm_t::flush: pixel_t::normalized (colorA_t / f multiplies by 1.0/f,
// color.h:329-333) + clampRGB0 (imagefilm.cc:400-424); premult: the clamped
// pixel's alphaPremultiply (imagefilm.cc:423)
__global__ void k_film_resolve(const float* __restrict__ film, float* __restrict__ rgba, long long npx, int premult) {
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npx) return;
  const float* a = film + 5 * p;
  float r = 0.f, g = 0.f, b = 0.f, al = 0.f;
  if (a[4] > 0.f) {
    const float f = (float)(1.0 / (double)a[4]);
    r = a[0] * f;
    g = a[1] * f;
    b = a[2] * f;
    al = a[3] * f;
  }
  r = r < 0.f ? 0.f : r;
  g = g < 0.f ? 0.f : g;
  b = b < 0.f ? 0.f : b;
  if (premult) {
    r = r * al;
    g = g * al;
    b = b * al;
  }
  rgba[4 * p] = r;
  rgba[4 * p + 1] = g;
  rgba[4 * p + 2] = b;
  rgba[4 * p + 3] = al;
}

// pixelGray_t::normalized (image_buffers.h:50-54): a float division
__global__ void k_depth_resolve(const float* __restrict__ depth, float* __restrict__ z, long long npx) {
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npx) return;
  const float v = depth[2 * p], w = depth[2 * p + 1];
  z[p] = w > 0.f ? v / w : 0.f;
}
