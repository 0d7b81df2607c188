"""Float64 brute force of the three ray queries over all triangles of a scene:
no kd-tree, no float32 operation order. A helper for tests/test_ground_truth.py.

Written from the definitions in include/yk_api.h, not from yk_math.h or the
oracle: a hit record (prim, t, b1, b2) names the point
    from + t * dir  =  (1 - b1 - b2) * A + b1 * B + b2 * C
of triangle (A, B, C), so per ray and triangle (u, v, t) solve the 3x3 system
    u * e1 + v * e2 - t * dir = from - A,        e1 = B - A, e2 = C - A,
by Cramer's rule with det = e1 . (dir x e2) = -dir . (e1 x e2):
    t = (from - A) . (e1 x e2) / det
    u = ((from x dir) . e2 - dir . (e2 x A)) / det
    v = -((from x dir) . e1 - dir . (e1 x A)) / det
Every product is bilinear in a per-ray and a per-triangle vector, so a chunk
of rays against all triangles is four float64 matrix products (torch, on the
GPU in the gpu tests, on the CPU otherwise), at most 2^26 ray x triangle pairs
at a time. BruteForce.pairs() evaluates the same system for single (ray,
triangle) pairs with explicit cross products, as a second formulation.

The answers of a float32 traversal are compared with these only where the
float64 decision has a margin:

* loose candidate:  det != 0, u >= -e, v >= -e, u + v <= 1 + e,
                    lo - e_t <= t < hi + e_t
* strict candidate: |det| >= GRAZE |e1| |e2| |dir| (never at grazing incidence),
                    u >= e, v >= e, u + v <= 1 - e, lo + e_t <= t < hi - e_t
  with e = 1e-4 and e_t = 1e-4 max(1, |t|), [lo, hi) the query's t range.
* closest hit: decided-hit when the nearest loose candidate is strict and no
  other loose candidate lies within e_t of it; decided-miss when no loose
  candidate exists; undecided otherwise.
* any hit (yk_trace_shadow): the query ray starts at from + tmin * dir and
  reaches tmax - 2 tmin; with t' = t - tmin the range is [0, tmax - 2 tmin) in
  triangle mode and (tmin, tmax - 2 tmin) in universal mode (yk_scene_set_mode:
  "accepts t > tmin of the shifted shadow ray"). yk_trace_shadow_filtered
  (IntersectTS) keeps tmin on the shifted ray as well: [tmin, tmax - 2 tmin).
  Decided-occluded when a strict candidate exists, decided-free when no loose
  one does.

On decided rays the answer must be the float64 one (check_closest /
check_occlusion); on undecided rays it must still be possible: a hit is a
loose candidate, not beyond the nearest strict candidate by more than e_t, and
a miss needs that no strict candidate exists. One named exclusion: a hit on a
triangle met below the grazing cutoff is not held to the loose margins
(check_closest, DESIGN.md §4 "Ground truth").
"""
import numpy as np
import torch

E_BARY = 1e-4    # margin on the barycentrics
E_T = 1e-4       # margin on t, times max(1, |t|)
GRAZE = 1e-3     # |det| / (|e1| |e2| |dir|) below which a candidate is never strict
MAX_PAIRS = 1 << 26

UNDECIDED, DECIDED_HIT, DECIDED_MISS = 0, 1, 2
INF = float("inf")


def _et(t):
    return E_T * torch.clamp(t.abs(), min=1.0)


def _cross(a, b):
    return torch.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                        a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


class BruteForce:
    """All triangles of one scene (tri_verts (n, 9) float32 as exported) in
    float64 on `device`; pairs: ray x triangle pairs per chunk (<= 2^26)."""

    def __init__(self, tri_verts, device="cpu", pairs=None):
        self.device = torch.device(device)
        V = torch.from_numpy(np.ascontiguousarray(tri_verts, np.float32).reshape(-1, 3, 3)).to(self.device,
                                                                                               torch.float64)
        self.ntris = V.shape[0]
        self.A = V[:, 0].contiguous()
        self.e1 = (V[:, 1] - V[:, 0]).contiguous()
        self.e2 = (V[:, 2] - V[:, 0]).contiguous()
        self.n = _cross(self.e1, self.e2)
        self.e1xA = _cross(self.e1, self.A)
        self.e2xA = _cross(self.e2, self.A)
        self.An = (self.A * self.n).sum(-1)
        self.len12 = self.e1.norm(dim=-1) * self.e2.norm(dim=-1)
        if pairs is None:
            pairs = 1 << 24 if self.device.type == "cuda" else 1 << 22
        self.pairs_per_chunk = min(int(pairs), MAX_PAIRS)
        if self.ntris > self.pairs_per_chunk:
            raise ValueError("more triangles than ray x triangle pairs of one chunk")

    def _rays(self, rays):
        r = torch.from_numpy(np.ascontiguousarray(rays, np.float32).reshape(-1, 8)).to(self.device, torch.float64)
        return r[:, 0:3], r[:, 3:6], r[:, 6], r[:, 7]

    def chunks(self, rays):
        """Yields (rows, u, v, t, det, steep) with (rows, ntris) float64 / bool
        tensors; steep = not at grazing incidence."""
        o, d, _, _ = self._rays(rays)
        step = max(1, self.pairs_per_chunk // max(self.ntris, 1))
        for r0 in range(0, o.shape[0], step):
            rows = slice(r0, min(r0 + step, o.shape[0]))
            oo, dd = o[rows], d[rows]
            m = _cross(oo, dd)
            det = -(dd @ self.n.T)
            t = (oo @ self.n.T - self.An) / det
            u = (m @ self.e2.T - dd @ self.e2xA.T) / det
            v = -(m @ self.e1.T - dd @ self.e1xA.T) / det
            steep = det.abs() >= GRAZE * dd.norm(dim=-1, keepdim=True) * self.len12
            yield rows, u, v, t, det, steep

    def pairs(self, rays, prim):
        """(u, v, t, det, steep) float64 numpy arrays of ray i against triangle
        prim[i], by the explicit cross products."""
        o, d, _, _ = self._rays(rays)
        p = torch.from_numpy(np.asarray(prim, np.int64)).to(self.device)
        e1, e2, tv = self.e1[p], self.e2[p], o - self.A[p]
        pv = _cross(d, e2)
        det = (e1 * pv).sum(-1)
        u = (tv * pv).sum(-1) / det
        qv = _cross(tv, e1)
        v = (d * qv).sum(-1) / det
        t = (e2 * qv).sum(-1) / det
        steep = det.abs() >= GRAZE * d.norm(dim=-1) * self.len12[p]
        return tuple(x.cpu().numpy() for x in (u, v, t, det, steep))

    # ---- closest hit -------------------------------------------------------
    def closest(self, rays):
        """Closest hit with tmin <= t < (tmax < 0 ? inf : tmax). Returns a dict
        of per-ray numpy arrays: state (UNDECIDED / DECIDED_HIT / DECIDED_MISS),
        prim / t / u / v of the nearest loose candidate (prim -1 without one),
        t_strict (t of the nearest strict candidate, inf without one)."""
        _, _, tmin, tmax = self._rays(rays)
        tmax = torch.where(tmax < 0, torch.full_like(tmax, INF), tmax)
        out = {k: [] for k in ("state", "prim", "t", "u", "v", "t_strict")}
        for rows, u, v, t, det, steep in self.chunks(rays):
            et = _et(t)
            lo, hi = tmin[rows, None], tmax[rows, None]
            s = u + v
            loose = (det != 0) & (u >= -E_BARY) & (v >= -E_BARY) & (s <= 1 + E_BARY) & (t >= lo - et) & (t < hi + et)
            strict = steep & (u >= E_BARY) & (v >= E_BARY) & (s <= 1 - E_BARY) & (t >= lo + et) & (t < hi - et)
            tl = torch.where(loose, t, torch.full_like(t, INF))
            tn, idx = tl.min(dim=1)
            some = torch.isfinite(tn)
            near = (tl <= (tn + _et(tn))[:, None]).sum(dim=1)
            g = idx[:, None]
            hit = some & strict.gather(1, g)[:, 0] & (near == 1)
            state = torch.where(hit, DECIDED_HIT, torch.where(some, UNDECIDED, DECIDED_MISS))
            out["state"].append(state.to(torch.int8))
            out["prim"].append(torch.where(some, idx, torch.full_like(idx, -1)))
            out["t"].append(tn)
            out["u"].append(u.gather(1, g)[:, 0])
            out["v"].append(v.gather(1, g)[:, 0])
            out["t_strict"].append(torch.where(strict, t, torch.full_like(t, INF)).min(dim=1).values)
        return {k: torch.cat(x).cpu().numpy() for k, x in out.items()}

    # ---- any hit -----------------------------------------------------------
    def any_hit(self, rays, lower="zero", transparent=None, kmax=9):
        """yk_trace_shadow's query (lower="zero"; "tmin" in universal mode) or,
        with transparent = bool per triangle, yk_trace_shadow_filtered's
        (lower="tmin"). Per ray: strict / loose (a strict / loose candidate
        lies in the segment; with `transparent` these count opaque triangles
        only), and with `transparent` also ambiguous (a loose candidate that is
        not strict, of either kind), ncross / ncross_loose (strict / loose
        transparent candidates) and cross_prim / cross_t (the first kmax of them by t', prim -1 past the
        end; t' is measured from the shifted origin)."""
        _, _, tmin, tmax = self._rays(rays)
        hi_r = torch.where(tmax < 0, torch.full_like(tmax, INF), tmax - 2 * tmin)
        lo_r = tmin if lower == "tmin" else torch.zeros_like(tmin)
        tr = None if transparent is None else torch.from_numpy(np.asarray(transparent, bool)).to(self.device)
        keys = ("strict", "loose") + (() if tr is None else ("ambiguous", "ncross", "ncross_loose", "cross_prim",
                                                             "cross_t"))
        out = {k: [] for k in keys}
        for rows, u, v, t, det, steep in self.chunks(rays):
            t = t - tmin[rows, None]
            et = _et(t)
            lo, hi = lo_r[rows, None], hi_r[rows, None]
            s = u + v
            loose = (det != 0) & (u >= -E_BARY) & (v >= -E_BARY) & (s <= 1 + E_BARY) & (t >= lo - et) & (t < hi + et)
            strict = steep & (u >= E_BARY) & (v >= E_BARY) & (s <= 1 - E_BARY) & (t >= lo + et) & (t < hi - et)
            if tr is None:
                out["strict"].append(strict.any(dim=1))
                out["loose"].append(loose.any(dim=1))
                continue
            out["strict"].append((strict & ~tr).any(dim=1))
            out["loose"].append((loose & ~tr).any(dim=1))
            out["ambiguous"].append((loose & ~strict).any(dim=1))
            cross = strict & tr
            out["ncross"].append(cross.sum(dim=1))
            out["ncross_loose"].append((loose & tr).sum(dim=1))
            k = min(kmax, self.ntris)
            ct, ci = torch.where(cross, t, torch.full_like(t, INF)).topk(k, dim=1, largest=False)
            out["cross_prim"].append(torch.where(torch.isfinite(ct), ci, torch.full_like(ci, -1)))
            out["cross_t"].append(ct)
        return {k: torch.cat(x).cpu().numpy() for k, x in out.items()}


# ---- assertions, the same for the oracle and the device ----------------------

def check_closest(bf, rays, c, prim, t, b1, b2, tol_t=None, tol_b=None, who=""):
    """c = bf.closest(rays); (prim, t, b1, b2) the answer under test. Asserts
    the rules of the module docstring (the tolerances only where given) and
    returns the figures: decided rays, decided hits, max relative t error
    (over max(1, |t64|)) and max barycentric error on the decided hits."""
    prim, t, b1, b2 = (np.asarray(x) for x in (prim, t, b1, b2))
    n = len(prim)
    hit64, miss64 = c["state"] == DECIDED_HIT, c["state"] == DECIDED_MISS
    bad = np.flatnonzero((hit64 & (prim != c["prim"])) | (miss64 & (prim >= 0)))
    assert len(bad) == 0, (f"{who}: {len(bad)} decided rays disagree with float64, first ray {bad[0]}: "
                           f"{rays[bad[0]].tolist()} answer prim {prim[bad[0]]} t {t[bad[0]]}, float64 prim "
                           f"{c['prim'][bad[0]]} t {c['t'][bad[0]]} state {c['state'][bad[0]]}")
    err_t = np.abs(t[hit64].astype(np.float64) - c["t"][hit64]) / np.maximum(1.0, np.abs(c["t"][hit64]))
    err_b = np.maximum(np.abs(b1[hit64].astype(np.float64) - c["u"][hit64]),
                       np.abs(b2[hit64].astype(np.float64) - c["v"][hit64]))
    fig = dict(n=n, decided=int(hit64.sum() + miss64.sum()), decided_hits=int(hit64.sum()),
               max_t=float(err_t.max()) if len(err_t) else 0.0, max_b=float(err_b.max()) if len(err_b) else 0.0)
    if tol_t is not None:
        assert fig["max_t"] <= tol_t, (who, fig)
    if tol_b is not None:
        assert fig["max_b"] <= tol_b, (who, fig)
    # every ray, undecided ones included: the answer must be possible
    h = np.flatnonzero(prim >= 0)
    _, _, tmin, tmax = (rays[:, 0:3], rays[:, 3:6], rays[:, 6].astype(np.float64), rays[:, 7].astype(np.float64))
    tmax = np.where(tmax < 0, np.inf, tmax)
    u, v, tt, det, steep = bf.pairs(rays[h], prim[h])
    with np.errstate(invalid="ignore"):
        et = E_T * np.maximum(1.0, np.abs(tt))
        loose = ((det != 0) & (u >= -E_BARY) & (v >= -E_BARY) & (u + v <= 1 + E_BARY) & (tt >= tmin[h] - et)
                 & (tt < tmax[h] + et))
    # The grazing exclusion (DESIGN.md §4 "Ground truth"): a hit on a triangle
    # the ray meets below the grazing cutoff is not held to the loose margins.
    # There float32 Moller-Trumbore (triangle_inline.h:27-64, one rounding of
    # dir x e2 scaled by 1 / det) has a barycentric error of about
    # 2^-24 / (|det| / |e1||e2||dir|), past e at the cutoff's 1e-3; such a
    # triangle is never strict, so this touches undecided rays only.
    fig["grazing_hits"] = int((~loose & ~steep).sum())
    bad = h[~loose & steep]
    assert len(bad) == 0, (f"{who}: {len(bad)} hits are no loose float64 candidate, first ray {bad[0]}: "
                           f"{rays[bad[0]].tolist()} prim {prim[bad[0]]} t {t[bad[0]]}")
    ts = c["t_strict"][h]
    late = h[t[h].astype(np.float64) > ts + E_T * np.maximum(1.0, np.abs(ts))]
    assert len(late) == 0, (f"{who}: {len(late)} hits lie beyond a strict candidate, first ray {late[0]}: "
                            f"{rays[late[0]].tolist()} prim {prim[late[0]]} t {t[late[0]]}, strict t "
                            f"{c['t_strict'][late[0]]}")
    lost = np.flatnonzero((prim < 0) & np.isfinite(c["t_strict"]))
    assert len(lost) == 0, (f"{who}: {len(lost)} misses although a strict candidate exists, first ray {lost[0]}: "
                            f"{rays[lost[0]].tolist()}, strict t {c['t_strict'][lost[0]]}")
    return fig


def check_occlusion(rays, a, occ, who=""):
    """a = bf.any_hit(rays, ...) without `transparent`; occ the answer under
    test. Occluded when a strict candidate exists, free when no loose one
    does; any answer where only loose ones exist. Returns the figures."""
    occ = np.asarray(occ).astype(bool)
    bad = np.flatnonzero((a["strict"] & ~occ) | (~a["loose"] & occ))
    assert len(bad) == 0, (f"{who}: {len(bad)} occlusion answers disagree with float64, first ray {bad[0]}: "
                           f"{rays[bad[0]].tolist()} answer {occ[bad[0]]} strict {a['strict'][bad[0]]} "
                           f"loose {a['loose'][bad[0]]}")
    return dict(n=len(occ), decided=int((a["strict"] | ~a["loose"]).sum()), occluded=int(a["strict"].sum()))


def check_filtered_occlusion(rays, a, depth, occ, who=""):
    """a = bf.any_hit(rays, "tmin", transparent); occ the answer of
    yk_trace_shadow_filtered at max_depth = depth. A ray is decided when no
    loose candidate of its segment fails to be strict; then it is occluded by
    a strict opaque triangle or by more than `depth` strict transparent ones.
    On the other rays the answer must be possible: occluded needs a loose
    opaque candidate or more than `depth` loose transparent ones, free needs
    that the strict candidates alone do not occlude. Returns the figures and
    the mask of decided free rays."""
    occ = np.asarray(occ).astype(bool)
    must = a["strict"] | (a["ncross"] > depth)
    may = a["loose"] | (a["ncross_loose"] > depth)
    decided = ~a["ambiguous"]
    assert (must == may)[decided].all()
    bad = np.flatnonzero((must & ~occ) | (~may & occ))
    assert len(bad) == 0, (f"{who} depth {depth}: {len(bad)} answers disagree with float64, first ray {bad[0]}: "
                           f"{rays[bad[0]].tolist()} answer {occ[bad[0]]}, opaque strict {a['strict'][bad[0]]} loose "
                           f"{a['loose'][bad[0]]}, crossings strict {a['ncross'][bad[0]]} loose "
                           f"{a['ncross_loose'][bad[0]]}")
    return dict(n=len(occ), decided=int(decided.sum()), occluded=int((decided & must).sum())), decided & ~must
