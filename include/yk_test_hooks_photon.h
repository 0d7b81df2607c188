/* yk_test_hooks_photon.h -- test-only entry points into the photon-map
 * lookups (core_amd/csrc/yk_photon.inc, photon_map.h): a synthetic map goes
 * through the steps yk_photon_build takes with a traced one, and host queries
 * run through the production device functions (pm_gather, pm_nearest), the
 * production k_pm_lookup launch and the host's point_tree_lookup.
 * Like yk_test_hooks.h it is NOT part of the product ABI (include/yk_api.h),
 * and every hook refuses to run (YK_ERR_UNSUPPORTED) unless the process
 * environment has YK_DEBUG_HOOKS=1. None needs an uploaded scene. */
#ifndef YK_TEST_HOOKS_PHOTON_H
#define YK_TEST_HOOKS_PHOTON_H
#include "yk_api.h"
#ifdef __cplusplus
extern "C" {
#endif

/* What yk_debug_photon_load made of the photons. lookup_lds / lookup_grid are
 * what enqueue_photon_mapping would launch k_pm_lookup with on this tree
 * (radiance slot; 0 for the other two). */
typedef struct yk_photon_map_info {
  int32_t photons;
  int32_t nodes;       /* 2n - 1 */
  int32_t depth;       /* deepest leaf, root = 1 */
  int32_t lookup_lds;  /* 1: the LDS-stack instantiation, 0: the scratch one */
  int32_t lookup_grid; /* workgroups of 64 */
  int32_t reserved;
} yk_photon_map_info;

/* Loads n photons (9 floats each: position, direction, colour) into map slot
 * `which` (YK_PHOTON_MAP_*) of the device: the host kd-tree build, the depth
 * check, the upload (the radiance slot also gets its 16-byte nodes, its depth
 * and node count, and the resident-wave count of the LDS lookup kernel), as in
 * yk_photon_build. n = 0 empties the slot. The maps of an earlier
 * yk_photon_build are gone afterwards: renders need a new one.
 *
 * depth_limit <= 0 or above the production bound (the lookup stacks' 48
 * entries less two) means that bound; a lower one makes the same check refuse
 * (YK_ERR_UNSUPPORTED) a shallower tree. The build is balanced, so no photon
 * count a test can hold reaches the production bound. */
int yk_debug_photon_load(yk_device* d, int32_t which, const float* photons, int32_t n, int32_t depth_limit,
                         yk_photon_map_info* info);

/* pm_gather (photonMap_t::gather) of nq queries in map `which`, one per
 * thread: pos nq x 3, r2 nq squared radii, K in [1, 256]. Out: count[q], the
 * found records idx / d2 (nq x K, heap order, the first count[q] valid; the
 * rest are all-ones bits: index -1) and r2_out[q], the radius the gather left.
 * An empty map answers 0 for every query, as the callers' own guard does. */
int yk_debug_photon_gather(yk_device* d, int32_t which, const float* pos, const float* r2, int64_t nq, int32_t K,
                           int32_t* count, int32_t* idx, float* d2, float* r2_out);

/* pm_nearest (photonMap_t::findNearest): pos, nrm nq x 3, r2 nq squared
 * radii; nearest[q] is the photon index or -1. */
int yk_debug_photon_nearest(yk_device* d, int32_t which, const float* pos, const float* nrm, const float* r2,
                            int64_t nq, int32_t* nearest);

/* The production k_pm_lookup over a host lookup queue on the radiance slot,
 * launched as enqueue_photon_mapping launches it: grid, LDS bytes, depth, a
 * count word and a zeroed work word on the device.
 *
 * lq: nq x 8 floats in the queue's layout, {position xyz, owner (int bits)},
 * {normal xyz, unused}. lcol: ncol floats, copied in, written by the kernel
 * (3 floats at 3 * owner for every query that finds a photon) and copied
 * back. Every owner must satisfy 0 <= owner and 3 * owner + 2 < ncol
 * (YK_ERR_ARG before any launch otherwise). force_scratch != 0 runs the
 * scratch-stack instantiation even on a tree the LDS one would take.
 * lds_out / grid_out (may be NULL): the instantiation and grid that ran.
 * YK_ERR_STATE when the radiance slot is empty. */
int yk_debug_photon_lookup_queue(yk_device* d, const float* lq, int64_t nq, float rad2, int32_t force_scratch,
                                 float* lcol, int64_t ncol, int32_t* lds_out, int32_t* grid_out);

/* The host side (photon_map.h), no device needed. photons as above.
 * host_tree: the nodes of point_tree_build (2 words each; up to cap_nodes are
 * written, *nnodes is the full count) and its depth.
 * host_gather / host_nearest: point_tree_lookup with photonGather_t over
 * libstdc++'s heap functions, and with nearestPhoton_t; arguments as the
 * device calls. */
int yk_debug_photon_host_tree(const float* photons, int32_t n, uint32_t* nodes, int64_t cap_nodes, int32_t* nnodes,
                              int32_t* depth);
int yk_debug_photon_host_gather(const float* photons, int32_t n, const float* pos, const float* r2, int64_t nq,
                                int32_t K, int32_t* count, int32_t* idx, float* d2, float* r2_out);
int yk_debug_photon_host_nearest(const float* photons, int32_t n, const float* pos, const float* nrm,
                                 const float* r2, int64_t nq, int32_t* nearest);

#ifdef __cplusplus
}
#endif
#endif /* YK_TEST_HOOKS_PHOTON_H */
