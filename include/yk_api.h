/*
 * yk_api.h -- C-ABI boundary of the MI355X ray-scene intersection and
 * path-integrator hot path (libyk.so).
 *
 * Replaces, behind the reference's own plugin API, these reference entry points
 * (reference = inferrna/Core, TheBounty 0.1.6):
 *   scene_t::startTriMesh/addVertex/addTriangle/endTriMesh  scene.cc:265-320,520-625
 *   scene_t::update (prim gather + triKdTree_t build)        scene.cc:748-850
 *   scene_t::intersect  -> triKdTree_t::Intersect            scene.cc:852-879, kdtree.cc:675-817
 *   scene_t::isShadowed -> triKdTree_t::IntersectS           scene.cc:881-902, kdtree.cc:820-947
 *   tiledIntegrator_t::render/renderPass/renderTile          integrator.cc:132-339
 *   pathIntegrator_t::integrate                              pathtracer.cc:134-333
 *   directLighting_t::integrate                              directlight.cc:112-182
 *   imageFilm_t::addSample / flush                           imagefilm.cc:383-511
 * The C++ plugin (plugin/yk_pathtrace_plugin.cc) binds these from inside a
 * tiledIntegrator_t subclass registered as "pathtracing"/"directlighting".
 *
 * Conventions: every function returns 0 (YK_OK) or a YK_ERR_* code; the text
 * of the last error of the calling thread is yk_last_error(). No C++ exception
 * and no HIP error crosses this boundary. Pointers named d_* are device (HBM)
 * pointers on the device the yk_device was opened on; all others are host.
 */
#ifndef YK_API_H
#define YK_API_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YK_OK 0
#define YK_ERR_ARG 1
#define YK_ERR_STATE 2
#define YK_ERR_HIP 3
#define YK_ERR_UNSUPPORTED 4
#define YK_ERR_ALLOC 5
#define YK_ERR_INTERNAL 6
#define YK_ERR_ABORTED 7 /* the abort callback asked to stop: the film holds the finished batches */

/* ---- scene description (POD mirrors of the reference paraMap_t params) ---- */

/* Value 3 is unassigned and stays refused (YK_ERR_UNSUPPORTED): callers and
 * tests rely on it as "a type the path does not know". */
enum { YK_MAT_SHINYDIFFUSE = 0, YK_MAT_LIGHT = 1, YK_MAT_GLOSSY = 2, YK_MAT_COATED_GLOSSY = 4, YK_MAT_GLASS = 5 };
typedef struct yk_material {
  int32_t type;           /* YK_MAT_*                                               */
  float color[3];         /* "color"  shinydiffuse.cc:474,483 / simple.cc:82        */
  float diffuse_reflect;  /* "diffuse_reflect" (shinydiffusemat, default 1)         */
  float emit;             /* "emit" (shinydiffusemat, default 0)                    */
  float power;            /* "power" (light_mat, default 1)                         */
  int32_t double_sided;   /* "double_sided" (light_mat, default 0)                  */
  /* shinydiffusemat specular / transmissive parameters (shinydiffuse.cc:474-503;
   * reference defaults in brackets -- a zero-initialised struct must set them) */
  float mirror_color[3];  /* "mirror_color" [1,1,1]                                 */
  float specular_reflect; /* "specular_reflect" [0]: mirror strength                */
  float transparency;     /* "transparency" [0]                                     */
  float translucency;     /* "translucency" [0]                                     */
  float transmit_filter;  /* "transmit_filter" [1]                                  */
  int32_t fresnel_effect; /* "fresnel_effect" [0]                                   */
  double ior;             /* "IOR" [1.33] (parsed as double; mIOR_Squared = IOR*IOR) */
  /* "diffuse_brdf" (shinydiffuse.cc:505-514): YK_BRDF_LAMBERT [default] or
   * YK_BRDF_OREN_NAYAR ("oren_nayar"), whose roughness is "sigma" [0.1,
   * parsed as double; a zero-initialised struct must set it]:
   * initOrenNayar(sigma), shinydiffuse.cc:170-176 */
  int32_t diffuse_brdf;
  double sigma;
  /* glossy (glossyMat_t::factory, glossy.cc:353-389). Appended fields only: the
   * offsets above are what earlier callers compiled against, and the other
   * kinds do not read the tail. For YK_MAT_GLOSSY `color` is the gloss colour
   * ("color" [1,1,1]), `diffuse_reflect` is "diffuse_reflect" [0 for glossy; > 0
   * adds the diffuse base], and diffuse_brdf YK_BRDF_OREN_NAYAR ("Oren-Nayar")
   * with sigma [0.1] is glossy's own initOrenNayar (glossy.cc:97-103). A
   * zero-initialised struct must set the bracketed defaults. as_diffuse == 0
   * (BSDF_GLOSSY, the glossy branch of recursiveRaytrace) is not on the path:
   * YK_ERR_UNSUPPORTED. */
  float diffuse_color[3]; /* "diffuse_color" [1,1,1]                                */
  float glossy_reflect;   /* "glossy_reflect" [1]                                   */
  float exponent;         /* "exponent" [50]                                        */
  int32_t as_diffuse;     /* "as_diffuse" [1]                                       */
  int32_t anisotropic;    /* "anisotropic" [0]: exp_u / exp_v instead of exponent   */
  float exp_u, exp_v;     /* "exp_u" [50], "exp_v" [50]                             */
  /* coated_glossy (coatedGlossyMat_t::factory, coatedglossy.cc:420-498) adds no
   * field: YK_MAT_COATED_GLOSSY reads the glossy fields as above plus
   * `mirror_color` ("mirror_color" [1,1,1]) and `ior` ("IOR" [1.4 for this
   * kind]). A zero-initialised struct must set IOR 1.4, mirror_color 1,
   * exponent 50, glossy_reflect 1, diffuse_reflect 0, as_diffuse 1. The
   * factory's `if(ior == 1.f) ior = 1.0000001f` is applied as written (the
   * double compared with and assigned a float literal, then held as a float).
   * as_diffuse == 0 is YK_ERR_UNSUPPORTED here too. */
  /* glass (glassMat_t::factory, glass.cc:260-337) reads `ior` ("IOR" [1.4 for
   * this kind]), `mirror_color` ("mirror_color" [1,1,1]) and `transmit_filter`
   * ("transmit_filter" [0 for this kind]) from this struct, whose size and
   * offsets callers have pinned; its own parameters travel in yk_glass_params. */
} yk_material;
/* glassMat_t's own parameters, beside a yk_material of type YK_MAT_GLASS
 * (yk_scene_add_glass). There is no absorption field: "absorption" makes the
 * reference attach the beer volume handler (BSDF_VOLUMETRIC), which the GPU
 * path does not have, so a host plugin must refuse such a material itself.
 * dispersion_power > 0 (BSDF_DISPERSIVE: state.chromatic, wavelengths) is
 * YK_ERR_UNSUPPORTED. Shader nodes and bump stay out, as for every kind. */
typedef struct yk_glass_params {
  float filter_color[3];   /* "filter_color" [1,1,1]                                 */
  int32_t fake_shadows;    /* "fake_shadows" [0]: isTransparent(), BSDF_FILTER       */
  double dispersion_power; /* "dispersion_power" [0], parsed as double               */
} yk_glass_params;
enum { YK_BRDF_LAMBERT = 0, YK_BRDF_OREN_NAYAR = 1 };

/* YK_LIGHT_MESH is the kind yk_scene_get_light and the device state report for
 * a mesh light; it is added with yk_scene_add_mesh_light, and
 * yk_scene_add_light answers YK_ERR_UNSUPPORTED for it (yk_light has no room
 * for object ids). YK_LIGHT_BACKGROUND (bgLight_t) likewise has an entry point
 * of its own, yk_scene_add_background_light: yk_scene_add_light answers
 * YK_ERR_UNSUPPORTED for it and yk_scene_get_light YK_ERR_STATE. */
enum { YK_LIGHT_AREA = 0, YK_LIGHT_POINT = 1, YK_LIGHT_DIRECTIONAL = 2, YK_LIGHT_SPOT = 3, YK_LIGHT_SPHERE = 4,
       YK_LIGHT_MESH = 5, YK_LIGHT_SUN = 6, YK_LIGHT_BACKGROUND = 7 };
typedef struct yk_light {
  int32_t type;
  /* area: areaLight_t::factory, arealight.cc:171-192 */
  float corner[3], point1[3], point2[3];
  float color[3];
  float power;
  int32_t samples;
  /* point: pointLight_t::factory (pointlight.cc:129-139), position = from;
   * directional: directionalLight_t::factory (directional.cc:139-165):
   * direction, and from/radius when infinite == 0 */
  float from[3];
  float direction[3];
  float radius;
  int32_t infinite;
  /* spot: spotLight_t::factory (spotlight.cc:284-305): from [0,0,0], to
   * [0,0,-1], color [1,1,1], power [1], cone_angle [45, degrees, the half
   * angle of the cone], blend [0.15], photon_only [0], soft_shadows [0],
   * shadow_fuzzyness ("shadowFuzzyness") [1], samples [8]; a zero-initialised
   * struct must set them.
   * sphere: sphereLight_t::factory (spherelight.cc:196-213): from [0,0,0]
   * (the centre), color [1,1,1], power [1], radius [1], samples [4]; its
   * "object" link is not on the path. Appended fields only: the offsets
   * above are what earlier callers compiled against.
   * sun: sunLight_t::factory (sunlight.cc:115-130): direction [0,0,1], color
   * [1,1,1], power [1], angle [0.27, degrees, the half angle of the sun's
   * disc], samples [4]; a zero-initialised struct must set them. The struct
   * does not grow for it: `cone_angle` carries the sun's "angle" (above 80 it
   * is clamped to 80, as the constructor does). YK_ERR_ARG for a zero or
   * non-finite direction, a non-finite colour or power, an angle that is not
   * finite or <= 0 (cosAngle == 1: invpdf 0, pdf infinite) and samples < 1. */
  float to[3];
  float cone_angle;
  float blend;
  int32_t soft_shadows;
  float shadow_fuzzyness;
  int32_t photon_only;
} yk_light;

/* meshlight: meshLight_t::factory (meshlight.cc:221-236): color [1,1,1],
 * power [1], samples [4], double_sided [0]; a zero-initialised struct must set
 * them. Its "object" is the obj_ids list of yk_scene_add_mesh_light. The
 * stored colour is color * (float)power * M_PI in the factory's types. */
typedef struct yk_mesh_light {
  float color[3];
  float power;
  int32_t samples;
  int32_t double_sided;
} yk_mesh_light;
/* Device limits of one mesh light (YK_ERR_UNSUPPORTED from yk_scene_build
 * above the first, from yk_device_upload above the second; never a truncated
 * light): triangles in its list, and depth of its private kd-tree -- the
 * per-lane traversal stack of the shading kernels holds depth + 3 entries.
 * triKdTree_t's own depth limit for 65536 triangles is 25. */
enum { YK_MESH_LIGHT_MAX_TRIS = 65536, YK_MESH_LIGHT_MAX_DEPTH = 29 };

/* perspectiveCam_t bokeh shapes and bias (perspectiveCamera.h:33-34) */
enum { YK_BOKEH_DISK1 = 0, YK_BOKEH_DISK2 = 1, YK_BOKEH_TRI = 3, YK_BOKEH_SQR = 4, YK_BOKEH_PENTA = 5,
       YK_BOKEH_HEXA = 6, YK_BOKEH_RING = 7 };
enum { YK_BOKEH_BIAS_NONE = 0, YK_BOKEH_BIAS_CENTER = 1, YK_BOKEH_BIAS_EDGE = 2 };
/* the reference's four cameras (src/cameras/): architect is perspectiveCam_t
 * with its own setAxis; orthographic and angular derive from camera_t and
 * have no lens (sampleLense() is false) */
enum { YK_CAMERA_PERSPECTIVE = 0, YK_CAMERA_ARCHITECT = 1, YK_CAMERA_ORTHOGRAPHIC = 2, YK_CAMERA_ANGULAR = 3 };
typedef struct yk_camera { /* perspectiveCam_t::factory, perspectiveCamera.cc:191-232 */
  float from[3], to[3], up[3];
  int32_t resx, resy;
  float focal, aspect_ratio, near_clip, far_clip;
  /* depth of field: "aperture" [0 = pinhole], "dof_distance", "bokeh_type",
   * "bokeh_bias", "bokeh_rotation" (degrees) */
  float aperture, dof_distance;
  int32_t bokeh_type, bokeh_bias;
  float bokeh_rotation;
  /* Appended fields only: the offsets above are what earlier callers compiled
   * against, and a zero-initialised tail is the perspective camera.
   * architect: architectCam_t::factory (architectCamera.cc:94-135), the
   * perspective parameters. orthographic: orthoCam_t::factory
   * (orthographicCamera.cc:83-103), "scale" [1]. angular: angularCam_t::factory
   * (angularCamera.cc:73-101), "angle" [90, degrees], "max_angle" [= angle],
   * "circular" [1], "mirrored" [0]; a zero-initialised struct must set them.
   * Those two factories hold aspect, scale, angle and max_angle as double:
   * aspect and scale only pass through a PFLOAT constructor argument
   * (aspect_ratio above is that float), max_r = max_angle / angle is a double
   * division. No aperture on an orthographic or angular camera (YK_ERR_ARG). */
  int32_t type;     /* YK_CAMERA_* */
  int32_t circular; /* angular: samples with radius > max_r carry no ray (wt = 0) */
  int32_t mirrored; /* angular: vright = -camX */
  int32_t reserved0;
  double scale;     /* orthographic: finite, > 0 */
  double angle;     /* angular: finite, > 0 */
  double max_angle; /* angular: finite, >= 0 */
} yk_camera;

enum { YK_INTEGRATOR_DIRECT = 0, YK_INTEGRATOR_PATH = 1, YK_INTEGRATOR_PHOTON = 2 };
enum { YK_FILTER_BOX = 0, YK_FILTER_MITCHELL = 1, YK_FILTER_GAUSS = 2, YK_FILTER_LANCZOS = 3 };
/* pathtracing "caustic_type" (pathtracer.cc:367-385): photon / both build a
 * caustic photon map in preprocess (mcIntegrator_t::createCausticMap,
 * mcintegrator.cc:197-377) from params.photon: caustic_photons ("photons"),
 * caustic_mix ("caustic_mix"), caustic_radius ("caustic_radius") and bounces
 * (= "caustic_depth", default 10 there); yk_photon_build builds it. */
enum { YK_CAUSTIC_NONE = 0, YK_CAUSTIC_PATH = 1, YK_CAUSTIC_PHOTON = 2, YK_CAUSTIC_BOTH = 3 };

/* photonIntegrator_t parameters (photonintegr.cc:884-960 factory; defaults
 * in brackets, set by yk_render_params_default). */
typedef struct yk_photon_params {
  int32_t photons;         /* "photons" [100000]: diffuse photons shot                */
  int32_t caustic_photons; /* "cPhotons" [500000]                                     */
  float diffuse_radius;    /* "diffuseRadius" [0.1]                                   */
  float caustic_radius;    /* "causticRadius" [0.01]                                  */
  int32_t search;          /* "search" [50]: nDiffuseSearch                           */
  int32_t caustic_mix;     /* "caustic_mix" [= search]: nCausSearch                   */
  int32_t bounces;         /* "bounces" [5]: maxBounces of the photon paths           */
  int32_t final_gather;    /* "finalGather" [1]                                       */
  int32_t fg_samples;      /* "fg_samples" [32]: nPaths                               */
  int32_t fg_bounces;      /* "fg_bounces" [2]: gatherBounces                         */
  float fg_min_pathlen;    /* "fg_min_pathlen" [= diffuseRadius]: gatherDist          */
  int32_t show_map;        /* "show_map" [0]                                          */
  int32_t seed;            /* the global ourRandom() state (myseed, vector3d.cc:185)
                              when preprocess() starts [123212]                       */
} yk_photon_params;

typedef struct yk_render_params {
  int32_t integrator;     /* YK_INTEGRATOR_*                                         */
  int32_t raydepth;       /* "raydepth"                                              */
  int32_t path_samples;   /* "path_samples" (pathtracing)                            */
  int32_t bounces;        /* "bounces" (pathtracing)                                 */
  int32_t caustic_type;   /* "caustic_type": YK_CAUSTIC_NONE or YK_CAUSTIC_PATH      */
  int32_t width, height;  /* render area ("width"/"height")                          */
  int32_t xstart, ystart; /* crop offset ("xstart"/"ystart")                         */
  int32_t aa_samples;     /* "AA_minsamples"                                         */
  int32_t aa_passes;      /* "AA_passes" (> 1: adaptive passes, single shard only)   */
  int32_t filter;         /* YK_FILTER_*                                             */
  float aa_pixelwidth;    /* "AA_pixelwidth"                                         */
  int32_t tile_size;      /* "tile_size"                                             */
  int32_t transp_background; /* "bg_transp" (default 1)                             */
  int32_t aa_inc_samples; /* "AA_inc_samples": samples per pass after the first (<= 0:
                             aa_samples, scene_t::setAntialiasing scene.cc:736-742)    */
  float aa_threshold;     /* "AA_threshold" (default 0.05): adaptive resampling     */
  yk_photon_params photon; /* integrator == YK_INTEGRATOR_PHOTON                   */
  int32_t transp_shadows;  /* "transpShad" [0]: shadow rays pass transparent materials,
                              scene_t::isShadowed(.., maxDepth, filt) / IntersectTS    */
  int32_t shadow_depth;    /* "shadowDepth" [5]: transparent surfaces a shadow ray may
                              cross (mcIntegrator_t::sDepth)                           */
  float filter_width;      /* imageFilm_t::filterw as the film holds it (> 0), taking
                              precedence over aa_pixelwidth; 0: derived from
                              aa_pixelwidth as imagefilm.cc:143-150 does [0]            */
  /* The order in which the film hands out its tiles (imageFilm_t::nextArea
   * over its imageSpliter_t, imagefilm.cc:190-195,291-304): tile_order_len
   * tile indices ty * ntx + tx, a permutation of all of the render area's
   * tiles; NULL / 0: row-major ("tiles_order" "linear", imagesplitter.cc:
   * 29-45). For "random" (std::random_shuffle, imagesplitter.cc:48) a plugin
   * reads the live film's splitter; yk_tile_order_random computes it for a
   * given rand() seed. Samples are splatted in this order (single-thread
   * reference order); a shard renders the listed tiles t with
   * t % nshards == shard, in list order. [NULL, 0]                           */
  const int32_t* tile_order;
  int32_t tile_order_len;
  /* directlighting's own options (directLighting_t::factory, directlight.cc:
   * 184-252; used at directlight.cc:137-142). Read only when integrator ==
   * YK_INTEGRATOR_DIRECT; appended, so the offsets above are what earlier
   * callers compiled against, and a zero-initialised struct has both off.
   * Ambient occlusion (mcIntegrator_t::sampleAmbientOcclusion, mcintegrator.cc:
   * 629-683): ao_samples any-hit rays of length ao_distance per diffuse
   * shading point, camera hits and specular-recursion nodes alike. do_ao != 0
   * needs ao_samples >= 1 and a finite ao_distance > 0 (YK_ERR_ARG), and
   * light slots + ao_samples <= 8192 (YK_ERR_UNSUPPORTED). */
  int32_t do_ao;        /* "do_AO" [0]                                              */
  int32_t ao_samples;   /* "AO_samples" [32]                                        */
  float ao_distance;    /* "AO_distance" [1.0] (parsed as double, held as float aoDist) */
  float ao_color[3];    /* "AO_color" [1,1,1]                                       */
  /* "caustics" [0]: col += estimateCausticPhotons on diffuse hits, from the
   * caustic map yk_photon_build makes for YK_INTEGRATOR_DIRECT with this flag
   * set (directLighting_t::preprocess, directlight.cc:78-83), out of
   * photon.caustic_photons ("photons"), caustic_mix, caustic_radius and
   * bounces ("caustic_depth"), as path tracing's photon caustics do. */
  int32_t dl_caustics;
  /* Film options (appended: the offsets above are what earlier callers compiled
   * against, and a zero-initialised tail renders exactly as before).
   * z_channel ("z_channel", scene_t::doDepth()): every camera sample that
   * carries a ray also splats one depth value into depth_film
   * (imageFilm_t::addDepthSample, imagefilm.cc:513-564; integrator.cc:313-334).
   * Raw: the camera hit's t, the camera ray's far-plane tmax on a miss, and
   * 99999997952.f where that is <= 0. normalize_z_channel
   * ("normalize_z_channel"): 1 - (tmax - depth_min) * depth_inv_range where
   * tmax > 0, else 0; depth_min / depth_inv_range are the reference's minDepth
   * and maxDepth after tiledIntegrator_t::precalcDepths (yk_depth_range).
   * depth_film: width*height*{val, weight} floats, caller-zeroed, in the
   * memory space of the call's film argument (device for yk_render_shard, host
   * for yk_render_film and yk_render_multi). YK_ERR_ARG: z_channel without a
   * depth_film; normalize_z_channel with a non-finite depth_min
   * (depth_inv_range may be inf, as in the reference). */
  int32_t z_channel;
  int32_t normalize_z_channel;
  float depth_min;
  float depth_inv_range;
  float* depth_film;
  /* "premult" (imageFilm_t::premultAlpha): addSample premultiplies its local
   * copy of the sample inside the pixel loop (imagefilm.cc:502), so the m-th
   * pixel of the sample's window (row-major, after the clamp to the film area)
   * takes the colour premultiplied m times; yk_film_resolve premultiplies once
   * more after its clamp, as flush does (imagefilm.cc:423).
   * "clamp_rgb" (imageFilm_t::clamp): clampRGB01 once per sample, before the
   * splat and before any premultiply (imagefilm.cc:457). */
  int32_t premult_alpha;
  int32_t clamp_rgb;
} yk_render_params;
enum { YK_TILES_LINEAR = 0, YK_TILES_RANDOM = 1 };

/* one ray, 32 bytes: ray_t (ray.h:26-49) without time */
typedef struct yk_ray {
  float from[3];
  float dir[3];
  float tmin;
  float tmax; /* < 0 means unbounded, as scene_t::intersect (scene.cc:855-856) */
} yk_ray;

/* closest-hit record, 16 bytes: prim id (scene_t::update order) + t + b1,b2
 * (intersectData_t, surface.h:35-56); b0 = 1 - b1 - b2. prim = -1 on miss. */
typedef struct yk_hit {
  int32_t prim;
  float t;
  float b1;
  float b2;
} yk_hit;

typedef struct yk_scene_info {
  int32_t ntris, nmeshes, nmaterials, nlights;
  int32_t nnodes, nleaf_prims, max_depth;
  int32_t inodes, leaves, empty_leaves, leaf_refs, depth_limit_leaves, bad_split_leaves;
  float bound[6];
  double build_seconds;
  int32_t mode; /* YK_MODE_* of the built scene */
} yk_scene_info;

typedef struct yk_stats {
  uint64_t closest_rays;   /* scene_t::intersect calls (camera + bounces)          */
  uint64_t shadow_rays;    /* scene_t::isShadowed calls                            */
  uint64_t closest_nodes;  /* kd nodes visited by closest-hit traversal            */
  uint64_t closest_tris;   /* triangle tests (= leaf refs read) by closest-hit     */
  uint64_t shadow_nodes;
  uint64_t shadow_tris;
  uint64_t camera_samples;
  double ms_total;         /* wall time of the render passes (device-synchronised) */
  double ms_closest;       /* summed kernel time of the closest-hit kernels        */
  double ms_shadow;        /* summed kernel time of the any-hit kernels            */
  uint64_t closest_launches, shadow_launches;
  double ms_reduce;        /* yk_render_multi: wall time of the film reduces (peer
                              copies + sum), included in the call's time          */
} yk_stats;

typedef struct yk_scene yk_scene;   /* host scene + kd-tree (no GPU needed) */
typedef struct yk_device yk_device; /* one GPU with an uploaded scene       */

const char* yk_last_error(void);
const char* yk_version(void);

/* ---- host scene (scene_t geometry state machine + update) ---- */
int yk_scene_create(yk_scene** out);
void yk_scene_destroy(yk_scene* s);
/* YK_ERR_UNSUPPORTED for an unknown type and for a glossy or coated glossy
 * material with as_diffuse == 0; YK_ERR_ARG for a glossy or coated glossy
 * material with a non-finite colour, glossy_reflect, diffuse_reflect or
 * exponent (a coated one: mirror_color and ior too).
 * yk_scene_add_material_state likewise, for the state's members; for a glossy
 * state whose bsdf_flags are not exactly BSDF_DIFFUSE | BSDF_REFLECT; and for
 * a coated state whose bsdf_flags, ncomp and comp_flags are not what
 * coatedglossy.cc:84-101 computes (see yk_material_state). */
int yk_scene_add_material(yk_scene* s, const yk_material* m, int32_t* id_out);
/* A glass material: m->type must be YK_MAT_GLASS, g its own parameters (NULL:
 * the factory defaults, which is also what yk_scene_add_material gives a
 * YK_MAT_GLASS). Runs glassMat_t's factory and constructor as written
 * (glass.cc:55-69, 262-274). YK_ERR_ARG for a non-finite colour, IOR or
 * transmit_filter; YK_ERR_UNSUPPORTED for dispersion_power > 0. */
int yk_scene_add_glass(yk_scene* s, const yk_material* m, const yk_glass_params* g, int32_t* id_out);
/* one TRIM mesh: points xyz (npoints*3), faces abc (nfaces*3); startTriMesh +
 * addVertex* + addTriangle* + endTriMesh (scene.cc:265-320,520-625) */
int yk_scene_add_mesh(yk_scene* s, const float* points, int32_t npoints, const int32_t* faces,
                      int32_t nfaces, int32_t material, int32_t* obj_id_out);
/* Vertex normals of mesh obj_id (triangle_t::na/nb/nc + triangleObject_t::normals):
 * normals xyz (nnormals*3), face_normals 3 indices per face (-1 = none),
 * flags YK_MESH_SMOOTH (triangleObject_t::is_smooth, set by smoothMesh or
 * exported normals, scene.cc:365-381) and YK_MESH_NORMALS_EXPORTED. */
enum { YK_MESH_SMOOTH = 1, YK_MESH_NORMALS_EXPORTED = 2 };
int yk_scene_set_mesh_normals(yk_scene* s, int32_t obj_id, const float* normals, int32_t nnormals,
                              const int32_t* face_normals, int32_t flags);
/* scene_t::startCurveMesh/addVertex/endCurveMesh (scene.cc:110-264): a hair
 * strand through npoints points, extruded to a triangular prism of
 * 6*(npoints-1)+2 triangles with the reference's radius law
 * (strand_start/end/shape) and vertex arithmetic. */
int yk_scene_add_curve(yk_scene* s, const float* points, int32_t npoints, int32_t material, float strand_start,
                       float strand_end, float strand_shape, int32_t* obj_id_out);
/* Scene mode (scene_t::setMode, xmlparser.cc:282-283; scene_t's default is
 * universal). YK_MODE_TRIANGLE: the tree holds the TRIM meshes and instances
 * (triKdTree_t); YK_MODE_UNIVERSAL: it holds the VTRIM meshes
 * (kdTree_t<primitive_t> over vTriangle_t, scene.cc:791-819), every one
 * whatever its visibility, whose any-hit test accepts t > tmin of the shifted
 * shadow ray (ray_kdtree.cc:936) and whose smooth shading weighs the first
 * vertex normal by intersectData_t::b0 = 0 (vTriangle_t::intersect never sets
 * it, triangle.cc:365-410) with normal index 0 meaning "none". */
enum { YK_MODE_TRIANGLE = 0, YK_MODE_UNIVERSAL = 1 };
int yk_scene_set_mode(yk_scene* s, int32_t mode);
/* the mesh type startTriMesh was given (object3d.h: TRIM 0, VTRIM 1) */
enum { YK_MESH_TRIM = 0, YK_MESH_VTRIM = 1 };
int yk_scene_set_mesh_type(yk_scene* s, int32_t obj_id, int32_t type);
/* mark a mesh as an instancing base: not traced itself (objData_t BASEMESH,
 * scene_t::update skips isBaseObject(), scene.cc:764) */
int yk_scene_set_mesh_base(yk_scene* s, int32_t obj_id);
/* scene_t::addInstance (scene.cc:983-1008): a triangleObjectInstance_t of a
 * base mesh with objToWorld as 16 floats, row-major (matrix4x4_t). Its prims
 * are flattened with the reference's vertex / normal transform arithmetic. */
int yk_scene_add_instance(yk_scene* s, int32_t base_obj_id, const float* obj_to_world, int32_t* obj_id_out);
int yk_scene_add_light(yk_scene* s, const yk_light* l);
/* meshLight_t over the triangles of the nobj TRIM meshes obj_ids, concatenated
 * in the order given (one reference object may arrive as several yk meshes,
 * one per run of equal material): triangleObject_t::getPrimitives order. The
 * light samples and intersects those triangles; the meshes themselves stay
 * ordinary scene geometry with their own material (a light_mat, usually).
 * YK_ERR_ARG: an unknown or repeated id, an empty list, samples < 1, a
 * non-finite colour or power; from yk_scene_build, a list whose total area is
 * zero. YK_ERR_UNSUPPORTED: a VTRIM mesh or an instance id (scene_t::getMesh
 * hands meshLight_t::init neither as a triangleObject_t), also when the mesh
 * is retyped after the call (found by yk_scene_build), and a list above
 * YK_MESH_LIGHT_MAX_TRIS. Photon emission of a mesh light is not on the path:
 * yk_photon_build refuses a scene that holds one. */
int yk_scene_add_mesh_light(yk_scene* s, const yk_mesh_light* l, const int32_t* obj_ids, int32_t nobj);
/* parameters and id list of mesh light i (YK_ERR_STATE for another kind);
 * at most cap ids are written, *nobj_out is the list's length; out, obj_ids
 * and nobj_out may be NULL */
int yk_scene_get_mesh_light(const yk_scene* s, int32_t i, yk_mesh_light* out, int32_t* obj_ids, int32_t cap,
                            int32_t* nobj_out);
/* YK_ERR_UNSUPPORTED for an unknown type; YK_ERR_ARG for a non-finite or
 * non-positive scale (orthographic) or angle (angular), a non-finite or
 * negative max_angle (angular), and an aperture on an orthographic or angular
 * camera (they have no lens; the parameter is not silently dropped) */
int yk_scene_set_camera(yk_scene* s, const yk_camera* c);
/* scene_t::update: gather prims and build the kd-tree (scene.cc:748-785) */
int yk_scene_build(yk_scene* s);
int yk_scene_info_get(const yk_scene* s, yk_scene_info* out);
/* copy out flattened prims / tree; any pointer may be NULL */
int yk_scene_export(const yk_scene* s, float* tri_verts, int32_t* tri_material, float* tri_normal,
                    uint32_t* nodes, uint32_t* leaf_prims);
/* per-prim shading data: smooth flag (1 byte per prim) and the three vertex
 * normals getSurface interpolates (9 floats per prim, zero where not smooth) */
int yk_scene_export_shading(const yk_scene* s, uint8_t* smooth, float* vertex_normals);
int yk_scene_get_material(const yk_scene* s, int32_t i, yk_material* out);
int yk_scene_get_light(const yk_scene* s, int32_t i, yk_light* out);
int yk_scene_get_camera(const yk_scene* s, yk_camera* out);
/* procedural probe scenes: "cornell" (36 tris) or "bumpy" (2*nu*(nv-1)+2 tris);
 * fills the scene and the matching render params of BASELINE.md */
int yk_scene_generate(yk_scene* s, const char* name, int32_t p0, int32_t p1, int32_t resx,
                      int32_t resy, yk_render_params* params_out);
void yk_render_params_default(yk_render_params* p);
/* imageSpliter_t's "random" tile order (imagesplitter.cc:48): the row-major
 * list 0..ntiles-1 shuffled by libstdc++'s std::random_shuffle, whose
 * rand() is glibc's after srand(seed) -- seed 1 is a process that has not
 * called srand() or rand() before the film is set up. Uses a private
 * generator state (the caller's rand() is untouched). */
int yk_tile_order_random(int32_t ntiles, uint32_t seed, int32_t* order_out);
/* A live imageFilm_t -> render parameters: identifies the film's filter by
 * comparing its 16x16 filterTable (imagefilm.cc:119-165) with the box /
 * Mitchell / Gauss / Lanczos2 tables libyk builds, bit for bit, and takes its
 * filterw as is (p->filter, p->filter_width). YK_ERR_UNSUPPORTED when the
 * table is none of them or filterw lies outside [0.501, 4]. */
int yk_film_filter_from_table(const float* filter_table, float filterw, yk_render_params* p);

/* ---- reference object state ----
 * What the reference's constructors computed, for a plugin that reads it out
 * of the live objects: re-deriving it from the XML
 * parameters would not round-trip in float. The parameter-level calls above
 * convert to these states with the reference's constructor arithmetic. */
typedef struct yk_material_state {
  int32_t type;             /* YK_MAT_*                                                  */
  uint32_t bsdf_flags;      /* material_t::bsdfFlags (material.h:49-66)                 */
  float color[3];           /* shinyDiffuseMat_t::mDiffuseColor | lightMat_t::lightCol  */
  float diffuse_strength;   /* shinyDiffuseMat_t::mDiffuseStrength                      */
  float emit_color[3];      /* shinyDiffuseMat_t::mEmitColor (= emit strength * color)  */
  int32_t double_sided;     /* lightMat_t::doubleSided                                  */
  /* shinyDiffuseMat_t after config() (shinydiffuse.cc:27-80) */
  float mirror_color[3];    /* mMirrorColor                                              */
  float component[4];       /* getComponents: mirror, transparency, translucency,
                               diffuse strength; 0 where config() left it off           */
  int32_t ncomp;            /* nBSDF                                                     */
  uint32_t comp_flags[4];   /* cFlags                                                    */
  int32_t comp_index[4];    /* cIndex                                                    */
  float transmit_filter;    /* mTransmitFilterStrength                                   */
  int32_t has_fresnel;      /* mHasFresnelEffect                                         */
  float ior_squared;        /* mIOR_Squared                                              */
  int32_t oren_nayar;       /* mUseOrenNayar                                             */
  float oren_nayar_a;       /* mOrenNayar_A = 1 - 0.5 s^2/(s^2 + 0.33), in double        */
  float oren_nayar_b;       /* mOrenNayar_B = 0.45 s^2/(s^2 + 0.09), in double           */
  /* glossyMat_t members after its constructor and factory (glossy.cc:56-62);
   * appended, zero for the other kinds. For YK_MAT_GLOSSY bsdf_flags are what
   * glossy.cc:69-79 sets, oren_nayar / _a / _b are orenNayar / orenA / orenB of
   * glossyMat_t::initOrenNayar, and the shinydiffuse members above are zero.
   * exp_u / exp_v are read only when anisotropic (the constructor leaves them
   * unset otherwise; they are stored as given). */
  float gloss_color[3], diff_color[3];
  float exponent, exp_u, exp_v;
  float reflectivity;       /* "glossy_reflect": MDat_t::mGlossy without shader nodes     */
  float m_diffuse;          /* mDiffuse                                                  */
  int32_t as_diffuse, with_diffuse, anisotropic;
  /* coatedGlossyMat_t (coatedglossy.cc:63-77), appended: the member IOR; zero
   * for the other kinds. A YK_MAT_COATED_GLOSSY state holds glossyMat_t's
   * members above with the same meaning, mirror_color, and the constructor's
   * flags (coatedglossy.cc:84-101): bsdf_flags = BSDF_SPECULAR | BSDF_REFLECT |
   * BSDF_DIFFUSE, ncomp = nBSDF (3 with a diffuse base, else 2), comp_flags =
   * cFlags {SPECULAR|REFLECT, DIFFUSE|REFLECT, DIFFUSE|REFLECT or BSDF_NONE};
   * anything else is YK_ERR_ARG. */
  float ior;
  /* A YK_MAT_GLASS state (glassMat_t, glass.cc:44-52) holds specRefCol in
   * mirror_color and the member ior in `ior`; filterCol and fakeShadow travel in
   * yk_glass_state (yk_scene_add_glass_state), since this struct's size is
   * pinned by its callers. bsdf_flags must be exactly BSDF_SPECULAR |
   * BSDF_REFLECT | BSDF_TRANSMIT, with BSDF_FILTER if and only if fake_shadow is
   * set (YK_ERR_ARG otherwise; BSDF_DISPERSIVE or BSDF_VOLUMETRIC:
   * YK_ERR_UNSUPPORTED); tmFlags follows from fake_shadow. */
} yk_material_state;
typedef struct yk_glass_state {
  float filter_col[3];      /* filterCol = filt*filter_color + color_t(1.f - filt)      */
  int32_t fake_shadow;      /* fakeShadow                                                */
} yk_glass_state;

typedef struct yk_area_light_state { /* areaLight_t members (arealight.h:45-53) */
  float corner[3], to_x[3], to_y[3];
  float color[3];           /* includes pi * power (arealight.cc:38)                    */
  int32_t samples;
} yk_area_light_state;

typedef struct yk_dirac_light_state { /* pointLight_t / directionalLight_t members after their ctors */
  int32_t type;          /* YK_LIGHT_POINT or YK_LIGHT_DIRECTIONAL                                  */
  float position[3];     /* pointLight_t::position / directionalLight_t::position                  */
  float direction[3];    /* directional: normalized (directional.cc:53)                             */
  float color[3];        /* color * power (pointlight.cc:55, directional.cc:51)                     */
  float radius;          /* directional, non-infinite                                              */
  int32_t infinite;
} yk_dirac_light_state;

typedef struct yk_spot_light_state { /* spotLight_t members after its ctor (spotlight.cc:63-75) */
  float position[3];
  float dir[3], ndir[3];    /* ndir = (from - to).normalize(), dir = -ndir              */
  float du[3], dv[3];       /* createCS(dir, du, dv), vector3d.h:316-334                */
  float cos_start, cos_end; /* fCos of the inner / outer angle (cos_start >= cos_end)   */
  float icos_diff;          /* 1.0 / (cosStart - cosEnd)                                */
  float color[3];           /* color * power                                            */
  int32_t soft_shadows;     /* 0: a Dirac light (one shadow ray); 1: illumSample + intersect */
  float shadow_fuzzyness;
  int32_t samples;          /* read when soft_shadows != 0                              */
  int32_t photon_only;      /* illuminate / illumSample return false                    */
} yk_spot_light_state;

typedef struct yk_sphere_light_state { /* sphereLight_t members after its ctor (spherelight.cc:64-72) */
  float center[3];
  float radius, square_radius;
  float square_radius_epsilon; /* square_radius * 1.000003815 (in double)               */
  float area;                  /* square_radius * 4.0 * M_PI (in double)                */
  float color[3];              /* color * power                                         */
  int32_t samples;
} yk_sphere_light_state;

typedef struct yk_sun_light_state { /* sunLight_t members after its ctor (sunlight.cc:52-63) */
  float color[3];           /* color * power                                            */
  float col_pdf[3];         /* colPdf = color * pdf                                     */
  float direction[3];       /* normalized                                               */
  float du[3], dv[3];       /* createCS of the constructor's UN-normalized argument     */
  float pdf, invpdf;        /* invpdf = M_2PI * (1.f - cosAngle), pdf = 1.0 / invpdf: in double, stored to float */
  double cos_angle;         /* cosAngle: a double holding the float fCos((float)degToRad(angle)) */
  int32_t samples;
} yk_sun_light_state;

typedef struct yk_camera_state { /* the camera after its ctor and setAxis (perspectiveCamera.cc:57-71) */
  float position[3], vright[3], vup[3], vto[3], cam_z[3];
  float near_p[3], far_p[3]; /* near_plane.p / far_plane.p (camera.h:54-57)            */
  int32_t resx, resy;
  /* depth of field (perspectiveCam_t ctor + setAxis): aperture (0 = pinhole),
   * dof_distance, dof_rt = aperture * camX, dof_up = aperture * camY, bokeh
   * type / bias and the polygon corner table LS (cos, sin pairs, up to 16) */
  float aperture, dof_distance;
  float dof_rt[3], dof_up[3];
  int32_t bokeh_type, bokeh_bias;
  float lens_ls[16];
  /* Appended; all zero for the perspective kind. kind names the shootRay that
   * runs: YK_CAMERA_PERSPECTIVE also for an architect camera, which differs
   * from perspectiveCam_t in setAxis alone (vup along (0,0,-1),
   * architectCamera.cc:54-68) and so in the vectors above, not in kind;
   * yk_scene_set_camera_state takes YK_CAMERA_ARCHITECT as that kind too.
   * YK_CAMERA_ORTHOGRAPHIC: position is orthoCam_t::pos (the film's corner),
   * vto = camZ, vup / vright the pixel steps (orthographicCamera.cc:37-49).
   * YK_CAMERA_ANGULAR: vright = +-camX, vup = camY, vto = camZ, and
   * angularCam_t's hor_phi, max_r, circular with camera_t's aspect_ratio
   * (aspect * resy / resx), which its shootRay multiplies v by. */
  int32_t kind;
  float hor_phi;      /* angle * M_PI / 180.f, in double, stored to float */
  float max_r;        /* max_angle / angle, in double, stored to float     */
  int32_t circular;
  float aspect_ratio; /* angular only; 0 otherwise                         */
} yk_camera_state;

int yk_scene_add_material_state(yk_scene* s, const yk_material_state* m, int32_t* id_out);
/* A YK_MAT_GLASS state with its filterCol and fakeShadow (g NULL: filterCol 1,
 * no fake shadows, which is also what yk_scene_add_material_state gives a
 * glass state). So a glass with fake shadows, whose bsdf_flags carry
 * BSDF_FILTER, is YK_ERR_ARG through yk_scene_add_material_state and
 * round-trips through this pair only: yk_scene_get_material_state plus
 * yk_scene_get_glass_state, then yk_scene_add_glass_state.
 * yk_scene_get_glass_state: YK_ERR_STATE when material i is of another kind. */
int yk_scene_add_glass_state(yk_scene* s, const yk_material_state* m, const yk_glass_state* g, int32_t* id_out);
int yk_scene_get_glass_state(const yk_scene* s, int32_t i, yk_glass_state* out);
int yk_scene_add_area_light_state(yk_scene* s, const yk_area_light_state* l);
/* point / directional light (light_t::diracLight() == true): one shadow ray
 * per estimate, mcintegrator.cc:85-100 */
int yk_scene_add_dirac_light_state(yk_scene* s, const yk_dirac_light_state* l);
int yk_scene_get_dirac_light_state(const yk_scene* s, int32_t i, yk_dirac_light_state* out);
/* spot light: Dirac (one shadow ray) unless soft_shadows, then `samples`
 * cone samples and as many BSDF (MIS) samples per estimate; sphere light:
 * `samples` cone samples and no MIS half (sphereLight_t::canIntersect() is
 * false, spherelight.cc:49). YK_ERR_STATE from a getter when light i is of
 * another kind. Photon emission of these lights is not on the path:
 * yk_photon_build refuses scenes that hold one. */
int yk_scene_add_spot_light_state(yk_scene* s, const yk_spot_light_state* l);
int yk_scene_get_spot_light_state(const yk_scene* s, int32_t i, yk_spot_light_state* out);
int yk_scene_add_sphere_light_state(yk_scene* s, const yk_sphere_light_state* l);
int yk_scene_get_sphere_light_state(const yk_scene* s, int32_t i, yk_sphere_light_state* out);
/* sun light: `samples` cone samples and as many BSDF (MIS) samples per
 * estimate (sunLight_t::canIntersect() is true), all unbounded rays. Its
 * photon members (worldCenter, worldRadius, ePdf: sunLight_t::init) come from
 * the scene bound at yk_device_upload, and yk_photon_build accepts it.
 * YK_ERR_ARG unless samples >= 1; the other members are taken as the live
 * object holds them. (FAST_TRIG's fCos answers exactly 1 for angles below
 * about 0.02 degrees: such a sun has invpdf 0 and an infinite pdf and colPdf,
 * as in the reference.) */
int yk_scene_add_sun_light_state(yk_scene* s, const yk_sun_light_state* l);
int yk_scene_get_sun_light_state(const yk_scene* s, int32_t i, yk_sun_light_state* out);
/* constBackground_t (textureback.cc:187-218, "constant", ibl off): camera
 * rays that miss add color*power. Setting it replaces a gradient background.
 * rgb NULL removes the constant background and leaves a gradient one alone
 * (yk_scene_set_gradient_background with NULL removes that). */
int yk_scene_set_background(yk_scene* s, const float* rgb, float power);
/* has_out = 0 when the scene has no background. YK_ERR_STATE when the scene's
 * background is a gradient (yk_scene_get_gradient_background reads that). */
int yk_scene_get_background(const yk_scene* s, float* rgb_out, int32_t* has_out);
/* gradientBackground_t (gradientback.cc:60-97, "gradientback"): a ray that
 * misses adds eval(dir): blend = dir.z; blend >= 0: blend * zenith +
 * (1.f - blend) * horizon, else the ground pair with -blend; a colour whose
 * smallest channel is below 1e-6f becomes (1e-5f, 1e-5f, 1e-5f). The four
 * colours are multiplied by power when set, as the factory does. It is a miss
 * colour wherever the constant background is one (camera rays, specular
 * recursion nodes, caustic segments), under all three integrators. Setting
 * either background replaces the other; g NULL removes a gradient (and leaves
 * a constant background alone). YK_ERR_ARG for a non-finite colour or power.
 * On a scene that holds a background light, setting or removing a background
 * returns the scene to the unbuilt state: the light's tables are made from
 * the background by yk_scene_build.
 * "sunsky", "darksky" and "textureback" backgrounds and bgPortalLight are not
 * on the GPU path. */
typedef struct yk_gradient_background {
  float horizon_color[3];        /* "horizon_color" [1,1,1]                */
  float zenith_color[3];         /* "zenith_color" [0.4,0.5,1]             */
  float horizon_ground_color[3]; /* "horizon_ground_color" [= horizon]     */
  float zenith_ground_color[3];  /* "zenith_ground_color" [= zenith]       */
  float power;                   /* "power" [1]                            */
} yk_gradient_background;
int yk_scene_set_gradient_background(yk_scene* s, const yk_gradient_background* g);
/* has_out = 0 (and out untouched) when the scene's background is not a
 * gradient; otherwise out holds the colours and power as they were set */
int yk_scene_get_gradient_background(const yk_scene* s, yk_gradient_background* out, int32_t* has_out);
/* bgLight_t (bglight.cc, "bglight"; what "ibl" of the constant and gradient
 * backgrounds creates): the scene's background as a sampled light with
 * `samples` importance samples over its tables and as many BSDF (MIS) samples
 * per estimate (canIntersect() is true), all unbounded rays; ls.col / lcol is
 * the background evaluated per sample. The light is appended to the light
 * list at the call and binds to whichever background the scene has at
 * yk_scene_build, which builds its tables (bgLight_t::init, bglight.cc:68-118:
 * 360 rows of 16..720 columns, one pdf1D_t per row and one over the rows'
 * integrals) and answers YK_ERR_STATE when the scene has no background.
 * YK_ERR_ARG unless samples >= 1.
 * Not on the GPU path, refused and never approximated:
 *  - emitPhoton: yk_photon_build answers YK_ERR_UNSUPPORTED ("background
 *    light") on a scene that holds one -- photon mapping, caustic_type photon
 *    / both and dl_caustics alike, so YK_INTEGRATOR_PHOTON cannot render it;
 *  - transparent shadows: a render with transp_shadows != 0 is
 *    YK_ERR_UNSUPPORTED (the slot's aux record applies one light colour at
 *    resolve and has no room for a per-sample one). */
typedef struct yk_background_light {
  int32_t samples;        /* "samples" / "ibl_samples" [16]                               */
  int32_t shoot_caustics; /* [1 gradient, 0 constant]; photon-only, held, not used here   */
  int32_t shoot_diffuse;  /* [1]; likewise                                                */
  int32_t abs_intersect;  /* "abs_intersect" [0]: intersect() negates the direction       */
} yk_background_light;
int yk_scene_add_background_light(yk_scene* s, const yk_background_light* l);
/* YK_ERR_STATE when light i is of another kind */
int yk_scene_get_background_light(const yk_scene* s, int32_t i, yk_background_light* out);
/* The tables of background light i of a built scene, bit for bit; any pointer
 * may be NULL. nrows_out: vDist->count (360). Per row y: row_count[y] =
 * uDist[y]->count, row_offset[y] = the row's first element in func_u (its cdf
 * starts at cdf_u[row_offset[y] + y], since a cdf holds count + 1 entries),
 * row_integral[y] / row_inv_integral[y] = uDist[y]->integral / invIntegral.
 * func_u holds sum(row_count) floats, cdf_u sum(row_count) + nrows; func_v
 * nrows (= the rows' integrals), cdf_v nrows + 1; v_integrals[2] =
 * {vDist->integral, vDist->invIntegral}. total_u_out = sum(row_count), so a
 * first call with NULL arrays sizes the second. invCount is 1.f / count. */
int yk_scene_export_background_light(const yk_scene* s, int32_t i, int32_t* nrows_out, int32_t* total_u_out,
                                     int32_t* row_count, int32_t* row_offset, float* row_integral,
                                     float* row_inv_integral, float* func_u, float* cdf_u, float* func_v,
                                     float* cdf_v, float* v_integrals);
int yk_scene_set_camera_state(yk_scene* s, const yk_camera_state* c);
int yk_scene_get_material_state(const yk_scene* s, int32_t i, yk_material_state* out);
int yk_scene_get_area_light_state(const yk_scene* s, int32_t i, yk_area_light_state* out);
/* meshLight_t members after init() (meshlight.cc:47-65), of a built scene:
 * the colour with pi * power, area = (float)total and inv_area =
 * (float)(1.0 / total) of the double running total of the float triangle
 * areas. cdf (ntris + 1 floats, pdf1D_t::cdf as CumulateStep1dDF leaves it)
 * and tri_areas (ntris floats, triangle_t::surfaceArea) may be NULL; at most
 * cap_tris triangles' worth is written. tree_depth (triKdTree_t::maxDepth, the
 * build's depth limit) and tree_nodes describe the light's own kd-tree
 * (triKdTree_t(tris, n, -1, 1, 0.8, 0.33)). */
typedef struct yk_mesh_light_state {
  float color[3];
  int32_t samples;
  int32_t double_sided;
  float area, inv_area;
  int32_t ntris;
  int32_t tree_depth, tree_nodes;
} yk_mesh_light_state;
int yk_scene_get_mesh_light_state(const yk_scene* s, int32_t i, yk_mesh_light_state* out, float* cdf,
                                  float* tri_areas, int32_t cap_tris);
/* meshLight_t::color of mesh light i as a live object holds it (pi * power
 * already in it): replaces the colour yk_scene_add_mesh_light computed, so a
 * plugin hands the member on bit for bit. yk_scene_get_light and
 * yk_scene_get_mesh_light go on reporting the color and power the light was
 * added with, which then no longer give the stored colour;
 * yk_scene_get_mesh_light_state reports the stored one. The colour is read
 * by yk_device_upload: the call does not touch the built scene, and a device
 * that already holds the scene keeps the earlier colour until the next upload.
 * YK_ERR_ARG for a non-finite colour, YK_ERR_STATE when light i is of another
 * kind. */
int yk_scene_set_mesh_light_color(yk_scene* s, int32_t i, const float* rgb);
int yk_scene_get_camera_state(const yk_scene* s, yk_camera_state* out);

/* ---- device ---- */
/* number of GPUs libyk can open (ordinals 0 .. n-1) */
int yk_device_count(int32_t* n);
int yk_device_open(int32_t ordinal, yk_device** out);
void yk_device_close(yk_device* d);
/* Uploads scene s (geometry, kd-tree, materials, lights, camera) and builds
 * the traversal's copies (node packets, leaf-ordered triangle records).
 * YK_ERR_ARG if the kd-tree has a leaf with 2^17 or more references (the
 * cooperative leaf test's limit) or 2^30 - 1 nodes or more (stack entries). */
int yk_device_upload(yk_device* d, const yk_scene* s);
int yk_device_sync(yk_device* d);
/* Abort polling (scene_t::getSignals() & Y_SIG_ABORT, integrator.cc:255):
 * renders on d call fn(user) between batches (tens of ms apart) and stop when
 * it returns non-zero -- the batches already running finish, the film holds
 * them, and the render returns YK_ERR_ABORTED. fn NULL removes the callback. */
typedef int32_t (*yk_abort_fn)(void* user);
int yk_device_set_abort(yk_device* d, yk_abort_fn fn, void* user);
/* hipStream_t the kernels run on, as an opaque pointer (for external timing) */
void* yk_device_stream(yk_device* d);

/* batched ray queries on device memory; bit-exact with the reference
 * triKdTree_t::Intersect (closest) and scene_t::isShadowed (any hit).
 * Closest: hits with tmin <= t < (tmax < 0 ? inf : tmax); prim -1 = miss.
 * Shadow: isShadowed(from, dir, tmin, tmax) semantics -- the query ray
 * starts at from + tmin*dir and reaches tmax - 2*tmin (scene.cc:884-889). */
int yk_trace_closest(yk_device* d, const yk_ray* d_rays, int64_t n, yk_hit* d_hits, yk_stats* st);
int yk_trace_shadow(yk_device* d, const yk_ray* d_rays, int64_t n, uint8_t* d_occluded, yk_stats* st);
/* scene_t::isShadowed(state, ray, maxDepth, filt) (scene.cc:904-928) ->
 * triKdTree_t::IntersectTS (kdtree.cc:953-1108): transparent materials let the
 * ray through and multiply d_filter (3 floats per ray) by getTransparency;
 * an opaque hit, or more than max_depth (<= 8) transparent ones, occludes. */
int yk_trace_shadow_filtered(yk_device* d, const yk_ray* d_rays, int64_t n, uint8_t* d_occluded, float* d_filter,
                             int32_t max_depth, yk_stats* st);

/* Render the tiles t with (t % nshards == shard) and accumulate the film
 * sums (R,G,B,A,weight per pixel, width*height*5 floats, pixel-major) into
 * d_film (device pointer, caller-allocated, caller-zeroed). With
 * p->z_channel the depth sums go to p->depth_film (device) likewise. */
int yk_render_shard(yk_device* d, const yk_render_params* p, int32_t shard, int32_t nshards,
                    float* d_film, yk_stats* st);
/* imageFilm_t::flush normalisation (+clampRGB0): film sums -> RGBA floats;
 * with p->premult_alpha the clamped pixel is premultiplied (RGB *= A) */
int yk_film_resolve(yk_device* d, const yk_render_params* p, const float* d_film, float* d_rgba);
/* tiledIntegrator_t::precalcDepths (integrator.cc:99-130) for the resident
 * scene and camera: *min_out / *inv_range_out are minDepth and maxDepth as
 * render() holds them afterwards (p->depth_min / p->depth_inv_range). A camera
 * set from parameters with far_clip > -1 gives its near and far clip; otherwise
 * one ray per pixel of the camera's resolution is shot at (row, column, 0.5,
 * 0.5) -- the reference passes the row index as px -- and traced, tmax of a
 * hit being its t: max over tmax from 0, min over tmax >= 0 from 1e38f. Then
 * maxDepth > 0 becomes 1 / (maxDepth - minDepth). A camera set as object state
 * (yk_scene_set_camera_state) carries no clip values: the rays are shot, and
 * the caller that holds the live camera takes its getNearClip / getFarClip
 * itself when far_clip > -1. YK_ERR_UNSUPPORTED for a circular angular camera
 * on the ray branch: the reference traces its samples outside the circle with
 * an uninitialised direction (angularCamera.cc:52-59, vector3d.h:56). p gives
 * nothing but its presence today (reserved for options); it must not be NULL. */
int yk_depth_range(yk_device* d, const yk_render_params* p, float* min_out, float* inv_range_out);
/* pixelGray_t::normalized (image_buffers.h:50-54): depth sums (width*height*
 * {val, weight}, device) -> width*height floats (device): weight > 0 ?
 * val / weight : 0, a float division */
int yk_depth_resolve(yk_device* d, const yk_render_params* p, const float* d_depth, float* d_z);
/* convenience for host callers (the reference plugin): render the tiles of
 * `shard` and return the film sums (width*height*5 floats) in host memory */
int yk_render_film(yk_device* d, const yk_render_params* p, int32_t shard, int32_t nshards, float* film_host,
                   yk_stats* st);
/* Whole frame on ndev devices, replacing tiledIntegrator_t::render's worker
 * threads (integrator.cc:177-211): devs[i] renders the tiles t % ndev == i on
 * its own host thread, and the film sums are reduced on devs[0] by peer
 * copies over xGMI, in shard order, into film_host (width*height*5 floats).
 * With AA_passes > 1 the reduced film gives every pass's imageFilm_t::nextPass
 * flags (imagefilm.cc:213-289), so adaptive passes work across devices (per
 * pixel the result equals the 1-device film up to float summation order).
 * Every device must hold the same uploaded scene (YK_ERR_STATE otherwise) and,
 * for photon mapping / photon caustics, maps built with p->photon; a device
 * handle may appear only once, but two handles may be opened on one GPU.
 * The peer copies run concurrently (one stream per source GPU) and one pass
 * sums the films in shard order; the films and staging buffers stay on the
 * handles, so repeated calls allocate nothing. st->ms_reduce gets the reduce
 * time. Handles opened on one GPU share its constant memory (materials,
 * lights, camera): a handle re-binds it from its own upload before it
 * renders, so handles on one GPU that hold different scenes must not render
 * at the same time. "Same uploaded scene" means the same built scene and the
 * same camera, lights and materials at upload time (a camera changed between
 * two handles' uploads is refused). At most 16 handles (YK_ERR_UNSUPPORTED).
 * Memory: devs[0] keeps one staging film per peer-GPU shard and the sum film
 * (width*height*5 floats each) until yk_device_close. */
int yk_render_multi(yk_device* const* devs, int32_t ndev, const yk_render_params* p, float* film_host,
                    yk_stats* st);
/* convenience: whole frame on one device, RGBA float image to host memory */
int yk_render(yk_device* d, const yk_render_params* p, float* rgba_host, yk_stats* st);

/* ---- photon mapping (photonIntegrator_t, photonintegr.cc) ---- */
typedef struct yk_photon_info {
  int32_t diffuse_photons;   /* diffuseMap.nPhotons()                                */
  int32_t diffuse_paths;     /* diffuseMap.nPaths(): last path index that stored one */
  int32_t caustic_photons;   /* causticMap.nPhotons()                                */
  int32_t caustic_paths;
  int32_t rad_candidates;    /* radiance points chosen by ourRandom() < 0.125        */
  int32_t radiance_photons;  /* radiance points left after the 0.01*r elimination    */
  int32_t seed_out;          /* myseed after preprocess                              */
  int32_t tree_depth;        /* deepest diffuse-map kd-tree leaf                     */
  uint64_t photon_rays;      /* scene_t::intersect calls of the photon paths         */
  double ms_shoot, ms_tree, ms_pregather, ms_total;
} yk_photon_info;

/* photonIntegrator_t::preprocess (photonintegr.cc:126-633): shoot the diffuse
 * and caustic photons on the device, build the photon kd-trees
 * (kdtree::pointKdTree, pkdtree.h) on the host, pre-gather the radiance
 * photons of final gathering on the device. The maps stay resident for
 * yk_render_shard with p->integrator == YK_INTEGRATOR_PHOTON.
 * With p->integrator == YK_INTEGRATOR_PATH it is pathIntegrator_t::preprocess
 * for caustic_type photon / both (pathtracer.cc:76-129): only the caustic map
 * of mcIntegrator_t::createCausticMap (mcintegrator.cc:197-377). The same
 * pass runs for p->integrator == YK_INTEGRATOR_DIRECT with p->dl_caustics set
 * (directLighting_t::preprocess, directlight.cc:78-83); without the flag
 * direct lighting has no preprocess and the call returns YK_ERR_ARG. */
int yk_photon_build(yk_device* d, const yk_render_params* p, yk_photon_info* info);
enum { YK_PHOTON_MAP_DIFFUSE = 0, YK_PHOTON_MAP_CAUSTIC = 1, YK_PHOTON_MAP_RADIANCE = 2 };
/* copy a map out in photon-vector order: 9 floats per photon (pos, dir, color);
 * cap = capacity in photons; *n_out = photons in the map */
int yk_photon_export(yk_device* d, int32_t which, float* out, int32_t cap, int32_t* n_out);

/* ---- GPU kd-tree build ----
 * Replaces triKdTree_t's CPU constructor (kdtree.cc:75-666, called from
 * scene_t::update, scene.cc:782) for a device that already holds scene s
 * (yk_device_upload): a binned-SAH kd-tree built level by level on the device,
 * in the same node encoding, replacing the uploaded reference tree until the
 * next upload. Opt-in, with a documented tie-break: hits equal those of the
 * reference tree except for which primitive wins at exactly equal t
 * (DESIGN.md §4 "GPU kd-tree build"). flags must be 0. */
typedef struct yk_tree_info {
  int32_t nodes, interior, leaves, empty_leaves, max_depth;
  int64_t leaf_refs;
  double ms_build; /* host wall time of the call, uploads included */
} yk_tree_info;
int yk_device_build_tree(yk_device* d, const yk_scene* s, int32_t flags, yk_tree_info* info);
/* Copies the device's resident kd-tree (the uploaded reference tree, or the
 * one yk_device_build_tree made) to host memory in the export encoding of
 * yk_scene_export: 2 u32 per node (split bits / prim / leaf offset; axis |
 * right child or count << 2), leaf lists as u32 prim ids. With nodes / leaf
 * NULL only the counts are returned. Test and tooling hook: it lets checks
 * aim rays at the split planes of the tree actually traversed. */
int yk_device_export_tree(yk_device* d, uint32_t* nodes, int64_t node_cap, uint32_t* leaf, int64_t leaf_cap,
                          int64_t* nnodes_out, int64_t* nleaf_out);
/* Test-only hooks (the watchdog's tree damage, the lights' function probe)
 * are declared in yk_test_hooks.h, yk_test_hooks_light.h,
 * yk_test_hooks_camera.h, yk_test_hooks_film.h, yk_test_hooks_depth.h and
 * yk_test_hooks_material.h, not here, and are disabled unless
 * YK_DEBUG_HOOKS=1. */

#ifdef __cplusplus
}
#endif
#endif /* YK_API_H */
