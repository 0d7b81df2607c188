// The device handle and its kernel tables (included by yk_device.hip after
// yk_pipe_host.inc): TraceVariant and kTrace, expanded from the list
// YK_TRACE_VARIANTS of yk_trav.inc; ShadeVariant,
// ShadeKernels, shade_cell and kShade with its static_asserts; struct
// yk_device and shade_kernels; the constant-memory binding (bind_constants,
// same_constants); watchdog_error and the YK_GUARD_* macros. Depends on the
// kernels and records of the device side and on yk_pipe_host.inc (HIPCHK,
// DBuf, Pipe).

// The trace kernels of one signature, as a table: the enumerators and the
// rows both come from YK_TRACE_VARIANTS (yk_trav.inc),
// in its order. k_trace_shadow_ts takes two more arguments (filter colours,
// depth) and stays on its own (enqueue_trace_ts, per_cu_ts).
enum TraceVariant {
#define YK_TRACE_ENUM(id, ...) id,
  YK_TRACE_VARIANTS(YK_TRACE_ENUM)
#undef YK_TRACE_ENUM
  kTraceVariants
};
using TraceKernel = void (*)(DScene, RaySrc, const unsigned*, RayCount, yk_hit*, uint8_t*, unsigned long long*,
                             unsigned long long*, uint2*, int, int);
struct TraceInfo {
  TraceKernel kernel;
  int waves;     // per workgroup
  bool dyn_lds;  // small_bytes of dynamic LDS (the scene copy)
  int ring;      // LDS stack ring depth per lane; deeper entries go to the overflow area
};
constexpr TraceInfo kTrace[kTraceVariants] = {
#define YK_TRACE_ROW(id, kernel, wpe, W, ring, ...) {kernel, W, (W) > 1, ring},
    YK_TRACE_VARIANTS(YK_TRACE_ROW)
#undef YK_TRACE_ROW
};

// The shading kernels of a scene, as a table. A scene's variant is its
// material level (the kernels' DIFF and GL arguments, which exclude each
// other: mat_sample) and its light level (XL), both fixed at upload.
// kMatDiffuse: every material a light or a one-component DIFFUSE|REFLECT shinydiffuse (mat_sample<true>);
// kMatGlossy: a material is glossy (kGLGlossy); kMatCoated: one is coated glossy (kGLCoated);
// kMatGlass: one is glass (kGLGlass, which holds the glossy and coated code too)
enum ShadeMat { kMatDiffuse, kMatGeneral, kMatGlossy, kMatCoated, kMatGlass, kShadeMats };
constexpr int kXLLevels = kXLBg + 1;
struct ShadeVariant {
  int mat = kMatGeneral;  // ShadeMat
  int xl = kXLNone;       // kXLSpotSphere: the scene holds a spot or sphere light; kXLMesh: a mesh light; kXLSun: a sun;
                          // kXLBg: a background light
};
struct ShadeKernels {
  decltype(&k_shade_primary<false, kXLNone, false>) primary[2];  // [AO]
  decltype(&k_shade_bounce<false, kXLNone>) bounce;
  int bounce_block;
  decltype(&k_path_start<false>) path_start;
  decltype(&k_spawn<>) spawn;
  decltype(&k_fg_start<false>) fg_start;
  decltype(&k_fg_hit<false>) fg_hit;
  decltype(&k_photon_emit<>) photon_emit;
  decltype(&k_pm_post<>) pm_post;
  decltype(&k_pm_finish<>) pm_finish;
  decltype(&k_pt_caustic<>) pt_caustic;
  decltype(&k_photon_hit<>) photon_hit;
};
// Which instantiation a variant runs: DIFF (diffuse-only materials) and XL
// (the scene holds a spot or sphere light). With the spot and sphere code in
// every instantiation k_shade_primary grew from 105 / 123 to 117 / 132 VGPRs
// (the general one from 4 to 3 waves per SIMD) and k_shade_bounce, held at 96,
// spilled 8 / 58 VGPRs instead of 0 / 23; scenes without such a light
// therefore run kernels that leave that code out (kXLNone), as scenes
// with plain diffuse materials leave out the component loop.
// A mesh light (kXLMesh) adds its own instantiations on top of the spot and
// sphere code: meshLight_t::intersect walks the light's kd-tree per BSDF-half
// sample with a per-lane stack in scratch memory (MeshStack), which no other
// scene pays for.
// A glossy material (GL) adds general-material instantiations of its own in
// the same way, one per XL x AO: glossy's lobe code reaches no other scene.
// Only k_shade_primary and k_shade_bounce sample lights, so only they take XL;
// the photon, k_pm_* and k_pt_caustic kernels take GL alone; k_spawn differs
// only for the coat (mat_specular), so glossy scenes run the general one.
// A sun light (kXLSun) is the top level: its cone sampling and cone test, on
// top of everything below. It is also the one sampled light beyond the area
// light that photon maps accept, so at this level alone k_fg_hit (whose
// estimateOneDirectLight may pick the sun) and k_photon_emit (emitPhoton)
// have instantiations of their own; at every other level they are the
// kernels they were before the sun.
// A background light (kXLBg) sits above the sun: its two table searches and
// the double acos of its sphere map reach k_shade_primary and k_shade_bounce
// of such scenes alone. Photon maps refuse the light (yk_photon_build), so
// k_fg_hit and k_photon_emit of this level are the sun level's.
template <int MAT, int XL>
constexpr ShadeKernels shade_cell() {
  constexpr bool DIFF = MAT == kMatDiffuse;
  constexpr int GL = MAT == kMatGlass ? kGLGlass : MAT == kMatCoated ? kGLCoated : (MAT == kMatGlossy ? kGLGlossy : kGLNone);
  return {{k_shade_primary<DIFF, XL, false, GL>, k_shade_primary<DIFF, XL, true, GL>}, k_shade_bounce<DIFF, XL, GL>,
          bounce_block(DIFF), k_path_start<DIFF, GL>, k_spawn<(GL >= kGLCoated ? GL : kGLNone)>,
          k_fg_start<DIFF, GL>, k_fg_hit<DIFF, GL, (XL >= kXLSun ? kXLSun : kXLNone)>,
          k_photon_emit<(XL >= kXLSun ? kXLSun : kXLNone)>, k_pm_post<GL>, k_pm_finish<GL>, k_pt_caustic<GL>,
          k_photon_hit<GL>};
}
constexpr ShadeKernels kShade[kShadeMats][kXLLevels] = {
    {shade_cell<kMatDiffuse, kXLNone>(), shade_cell<kMatDiffuse, kXLSpotSphere>(), shade_cell<kMatDiffuse, kXLMesh>(),
     shade_cell<kMatDiffuse, kXLSun>(), shade_cell<kMatDiffuse, kXLBg>()},
    {shade_cell<kMatGeneral, kXLNone>(), shade_cell<kMatGeneral, kXLSpotSphere>(), shade_cell<kMatGeneral, kXLMesh>(),
     shade_cell<kMatGeneral, kXLSun>(), shade_cell<kMatGeneral, kXLBg>()},
    {shade_cell<kMatGlossy, kXLNone>(), shade_cell<kMatGlossy, kXLSpotSphere>(), shade_cell<kMatGlossy, kXLMesh>(),
     shade_cell<kMatGlossy, kXLSun>(), shade_cell<kMatGlossy, kXLBg>()},
    {shade_cell<kMatCoated, kXLNone>(), shade_cell<kMatCoated, kXLSpotSphere>(), shade_cell<kMatCoated, kXLMesh>(),
     shade_cell<kMatCoated, kXLSun>(), shade_cell<kMatCoated, kXLBg>()},
    {shade_cell<kMatGlass, kXLNone>(), shade_cell<kMatGlass, kXLSpotSphere>(), shade_cell<kMatGlass, kXLMesh>(),
     shade_cell<kMatGlass, kXLSun>(), shade_cell<kMatGlass, kXLBg>()},
};
// below the sun's level the table names no instantiation beyond those it named before: no glossy k_spawn, no
// DIFF or XL where a kernel takes none; the sun's level adds k_fg_hit and k_photon_emit of its own
static_assert(kShade[kMatGlossy][kXLNone].spawn == kShade[kMatGeneral][kXLNone].spawn &&
              kShade[kMatCoated][kXLNone].spawn != kShade[kMatGeneral][kXLNone].spawn &&
              kShade[kMatDiffuse][kXLNone].photon_hit == kShade[kMatGeneral][kXLNone].photon_hit &&
              kShade[kMatDiffuse][kXLNone].pm_post == kShade[kMatGeneral][kXLNone].pm_post &&
              kShade[kMatCoated][kXLMesh].fg_hit == kShade[kMatCoated][kXLNone].fg_hit &&
              kShade[kMatDiffuse][kXLMesh].path_start == kShade[kMatDiffuse][kXLNone].path_start &&
              kShade[kMatGeneral][kXLMesh].photon_emit == kShade[kMatDiffuse][kXLNone].photon_emit &&
              kShade[kMatCoated][kXLSun].fg_hit != kShade[kMatCoated][kXLNone].fg_hit &&
              kShade[kMatDiffuse][kXLSun].photon_emit != kShade[kMatDiffuse][kXLNone].photon_emit &&
              kShade[kMatDiffuse][kXLSun].path_start == kShade[kMatDiffuse][kXLNone].path_start);
static_assert(kBgNone == YK_BG_NONE && kBgConstant == YK_BG_CONSTANT && kBgGradient == YK_BG_GRADIENT,
              "the device's background kinds are the scene's");
// the background light's level adds k_shade_primary and k_shade_bounce alone
static_assert(kShade[kMatGeneral][kXLBg].bounce != kShade[kMatGeneral][kXLSun].bounce &&
              kShade[kMatGeneral][kXLBg].primary[0] != kShade[kMatGeneral][kXLSun].primary[0] &&
              kShade[kMatGlass][kXLBg].fg_hit == kShade[kMatGlass][kXLSun].fg_hit &&
              kShade[kMatDiffuse][kXLBg].photon_emit == kShade[kMatDiffuse][kXLSun].photon_emit &&
              kShade[kMatCoated][kXLBg].spawn == kShade[kMatCoated][kXLNone].spawn);
// the glass row names kernels of its own wherever the coated row does, and the coated row names what it named before
static_assert(kShade[kMatCoated][kXLNone].spawn == &k_spawn<kGLCoated> &&
              kShade[kMatCoated][kXLNone].bounce == &k_shade_bounce<false, kXLNone, kGLCoated> &&
              kShade[kMatCoated][kXLNone].photon_hit == &k_photon_hit<kGLCoated> &&
              kShade[kMatGlass][kXLNone].spawn == &k_spawn<kGLGlass> &&
              kShade[kMatGlass][kXLNone].bounce != kShade[kMatCoated][kXLNone].bounce &&
              kShade[kMatGlass][kXLNone].photon_hit != kShade[kMatCoated][kXLNone].photon_hit &&
              kShade[kMatGlass][kXLMesh].fg_hit == kShade[kMatGlass][kXLNone].fg_hit &&
              kShade[kMatGlass][kXLMesh].photon_emit == kShade[kMatDiffuse][kXLNone].photon_emit);

struct yk_device {
  int ordinal = 0;
  int cus = 0;
  int per_cu[kTraceVariants] = {};  // resident workgroups per CU of each trace kernel (fill_trace_occupancy)
  // small scenes: traversal data copied to LDS per workgroup (install_traversal)
  bool small = false;
  size_t small_bytes = 0;
  hipStream_t stream = nullptr;  // = pipe[0].stream (ray queries, film resolve)
  bool uploaded = false;
  const yk_scene* uploaded_scene = nullptr;  // the scene the resident arrays came from
  uint64_t uploaded_gen = 0;                 // its Scene::generation at upload
  uint64_t const_token = 0;                  // unique per yk_device_upload (bind_constants)
  size_t nleaf = 0;                          // leaf-list entries of the resident tree
  // scene
  DBuf<float> tris;  // triangle records (kTriWords floats per prim)
  DBuf<float4> ng;
  DBuf<float> vn;  // smooth-shading vertex normals (9 per prim), only when the scene has smooth meshes
  DBuf<uint2> nodes;
  DBuf<uint32_t> pk;   // node packets (k_pack_nodes), rebuilt whenever nodes change
  DBuf<float> ltris;  // leaf-ordered record copies, rebuilt whenever the leaf lists change
  DBuf<uint32_t> leaf;
  DScene S{};
  int ntris = 0, max_depth = 0, nlights = 0, sum_light_slots = 0;
  bool spec = false;  // some material has SPECULAR|FILTER components: recursion pipeline
  ShadeVariant shade;  // material and light level of the scene: its shading kernels (shade_kernels)
  // mesh lights: one record per light in DScene::ml, its arrays packed in three buffers
  DBuf<DMeshLight> ml_recs;
  DBuf<float> ml_f;
  DBuf<uint2> ml_nodes;
  DBuf<uint32_t> ml_leaf;
  yk_abort_fn abort_fn = nullptr;  // yk_device_set_abort: polled between batches
  void* abort_user = nullptr;
  bool big_leaves = false;  // the resident tree has a leaf of 2^17 references or more: *_big kernels
  bool crowded_leaves = false;  // mean references per non-empty leaf above YK_CROWDED_LEAF: 64-ray hand-out chunks
  int refill = 24;  // idle lanes before a traversal wave refills (set_handout)
  int refill_shadow = 24;  // the same for the any-hit kernels
  int per_cu_ts = 1;
  int per_cu_ts_glass = 1;  // k_trace_shadow_ts_glass
  bool ts_glass = false;    // the scene holds a glass with fake shadows: transparent shadows run k_trace_shadow_ts_glass
  int per_cu_lookup[2] = {1, 1};  // k_pm_lookup<false / true> resident waves per CU
  // node store of the specular recursion (k_finish_spec / k_spawn / k_fold)
  DBuf<float> nE, nD, nP, nrcol, nalpha, nmalpha;
  DBuf<int> nflags, nchild, noverflow;
  DBuf<yk_ray> nray;
  DBuf<unsigned> nsoffs, npsample;
  DBuf<unsigned long long> ncount, spec_words;
  int bg_kind = kBgNone;  // the scene's background: kBgConstant (bg) or kBgGradient (bg_grad)
  float bg[3] = {0.f, 0.f, 0.f};
  float bg_grad[12] = {};
  std::vector<DLight> lights_host;
  // photon maps of yk_photon_build (photonIntegrator_t::preprocess)
  bool pm_ready = false;
  int pm_integrator = -1;  // integrator whose preprocess built the maps
  yk_photon_params pm_params{};
  DBuf<uint2> dm_nodes, rm_nodes, cm_nodes;
  DBuf<float4> dm_pos, dm_dir, dm_col, rm_pos, rm_dir, rm_col, cm_pos, cm_dir, cm_col;
  DBuf<uint4> rm_pk;  // radiance tree as 16-B nodes (k_pm_lookup): split | axis, right; leaf: position | photon
  std::vector<float> dm_host, rm_host, cm_host;  // 9 floats per photon, photon-vector order
  int dm_paths = 0, cm_paths = 0;
  int rm_depth = 0;  // radiance kd-tree depth (k_fg_hit keeps its lookup stack in LDS up to kLdsPStack)
  size_t rm_nnodes = 0;  // radiance kd-tree nodes
  std::vector<unsigned> mat_flags;  // bsdfFlags per material
  Pipe pipe[kPipes];
  hipEvent_t gather_ev[kPipes] = {};
  // device records of the uploaded scene, kept to re-bind the GPU's constant
  // memory when another handle on the same GPU uploaded a different scene
  std::vector<DMat> mats_host;
  DCam cam_host{};
  // what precalcDepths reads of the camera (yk_depth_range): its resolution,
  // and the clip values when it was set from parameters
  int cam_resx = 0, cam_resy = 0;
  bool cam_has_clip = false;
  float cam_near_clip = 0.f, cam_far_clip = 0.f;
  // yk_render_multi state, kept across calls (no allocation once sized): this
  // device's shard film; as the reducing device, the sum, one staging film per
  // peer GPU and one copy stream + event per peer (each peer's copy drives its
  // own xGMI link)
  DBuf<float> mfilm, macc;
  DBuf<float> mdepth, mdacc;  // z_channel: this device's shard depth film; the reducing device's sum
  DBuf<float> mstage[kMaxMultiDev];
  DBuf<float> mdstage[kMaxMultiDev];  // z_channel: a peer GPU's shard depth film
  // the frame plan's tile lists (upload_frame_plan; grow-only, so repeated renders allocate nothing)
  DBuf<int4> tiles_dev;
  DBuf<int> base_dev, pix_dev, pmap_dev, rank_dev;
  DBuf<uint8_t> flags_dev;
  // per batch of a render: the camera samples that carry a ray (an angular
  // camera with `circular`; unused otherwise)
  DBuf<unsigned long long> cam_live;
  // the last render's batch plan (yk_debug_last_plan)
  yk_batch_plan last_plan{};
  bool last_plan_valid = false;
  int last_max_batches = 0;
  hipStream_t mstream[kMaxMultiDev] = {};
  hipEvent_t mevent[kMaxMultiDev] = {};
  ~yk_device() {
    for (auto& e : gather_ev)
      if (e) (void)hipEventDestroy(e);
    for (int i = 0; i < kMaxMultiDev; ++i) {
      if (mevent[i]) (void)hipEventDestroy(mevent[i]);
      if (mstream[i]) (void)hipStreamDestroy(mstream[i]);
    }
  }
};

namespace {
inline const ShadeKernels& shade_kernels(const yk_device* d) { return kShade[d->shade.mat][d->shade.xl]; }

// Constant memory (c_mats, c_lights, c_cam) is per GPU, not per handle: the
// upload whose records a GPU's constants hold. Every yk_device_upload takes a
// fresh process-wide token (the scene's generation alone is not enough: the
// camera can change on a built scene, yk_scene_set_camera, and a re-upload
// must then reach c_cam). A handle whose token differs re-binds them before
// it launches (bind_constants). If the records the GPU holds are byte-equal
// to the handle's (handles of one scene on one GPU, as yk_render_multi's
// concurrent threads have them), the handle adopts them without a copy, so
// no handle rewrites constant memory while another one's kernels read it
// (ADVICE r05).
std::mutex g_const_mu;
uint64_t g_const_token[64] = {};
struct ConstImage {
  std::vector<unsigned char> mats, lights, cam;
};
ConstImage g_const_img[64];
std::atomic<uint64_t> g_upload_token{1};

template <class T>
void bytes_of(std::vector<unsigned char>& v, const T* p, size_t n) {
  v.assign(reinterpret_cast<const unsigned char*>(p), reinterpret_cast<const unsigned char*>(p) + n * sizeof(T));
}

void bind_constants(yk_device* d) {
  std::lock_guard<std::mutex> lk(g_const_mu);
  const int o = d->ordinal & 63;
  if (g_const_token[o] == d->const_token) return;
  ConstImage img;
  bytes_of(img.mats, d->mats_host.data(), d->mats_host.size());
  bytes_of(img.lights, d->lights_host.data(), d->lights_host.size());
  bytes_of(img.cam, &d->cam_host, 1);
  ConstImage& cur = g_const_img[o];
  if (g_const_token[o] != 0 && img.mats == cur.mats && img.lights == cur.lights && img.cam == cur.cam) {
    g_const_token[o] = d->const_token;  // same records already resident: adopt, no rewrite
    return;
  }
  if (!d->mats_host.empty())
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(c_mats), d->mats_host.data(), d->mats_host.size() * sizeof(DMat)));
  if (!d->lights_host.empty())
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(c_lights), d->lights_host.data(), d->lights_host.size() * sizeof(DLight)));
  HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(c_cam), &d->cam_host, sizeof(DCam)));
  g_const_token[o] = d->const_token;
  cur = std::move(img);
}

// two handles render one frame only if their constant records are the same
// (same scene generation is checked separately; this catches a camera, light
// or material changed between the two uploads)
bool same_constants(const yk_device* a, const yk_device* b) {
  return a->mats_host.size() == b->mats_host.size() && a->lights_host.size() == b->lights_host.size() &&
         std::memcmp(&a->cam_host, &b->cam_host, sizeof(DCam)) == 0 &&
         (a->mats_host.empty() ||
          std::memcmp(a->mats_host.data(), b->mats_host.data(), a->mats_host.size() * sizeof(DMat)) == 0) &&
         (a->lights_host.empty() ||
          std::memcmp(a->lights_host.data(), b->lights_host.data(), a->lights_host.size() * sizeof(DLight)) == 0) &&
         a->bg_kind == b->bg_kind && std::memcmp(a->bg, b->bg, sizeof a->bg) == 0 &&
         std::memcmp(a->bg_grad, b->bg_grad, sizeof a->bg_grad) == 0;
}

// the traversal watchdog fired (corrupt tree or stack): YK_ERR_INTERNAL
struct watchdog_error : std::runtime_error {
  using std::runtime_error::runtime_error;
};

#define YK_GUARD_BEGIN try {
#define YK_GUARD_END                                                                              \
  }                                                                                               \
  catch (const watchdog_error& e) { return set_error(YK_ERR_INTERNAL, e.what()); }               \
  catch (const std::bad_alloc&) { return set_error(YK_ERR_ALLOC, "out of host memory"); }        \
  catch (const std::invalid_argument& e) { return set_error(YK_ERR_ARG, e.what()); }             \
  catch (const std::runtime_error& e) { return set_error(YK_ERR_HIP, e.what()); }                \
  catch (const std::exception& e) { return set_error(YK_ERR_INTERNAL, e.what()); }               \
  catch (...) { return set_error(YK_ERR_INTERNAL, "unknown C++ exception"); }

}  // namespace
