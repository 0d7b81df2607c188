"""Brute-force float64 reference of the photon-map lookups, and the two input
families of tests/test_photon_lookup.py. No tree: every query is compared
with every photon.

  nearest: the smallest squared distance among photons with dir . n > 0 and
           d2 < r2 (photonMap_t::findNearest)
  gather:  the K smallest squared distances with d2 < r2 (photonMap_t::gather)

Lattice sets: every coordinate of photons and queries is a multiple of 2^-10
in [0, 1). A difference is then a multiple of 2^-10 below 1, its square a
multiple of 2^-20 below 1 and a three-term sum one below 3: all fit in 24
bits, so float32 and float64 agree exactly with or without fused
multiply-add, every comparison is exact and every tie is a real tie
(eps = 0 below). Directions and normals have components in {-1, -1/2, 0, 1/2,
1}, so the facing test is exact as well, dot products of exactly 0 included.

Random float32 sets: the device's d2 = fl(fl(fl(vx^2) + fl(vy^2)) + fl(vz^2))
with v = fl(photon - query) is five roundings away from the exact value, a
relative error below (1 + 2^-24)^5 - 1 < 8 * 2^-24 = EPS. An answer is right
if its float64 d2 lies within the factor 1 + EPS of the brute-force one, and a
photon whose d2 lies within that factor of r2 may be in or out.
"""
import numpy as np

F32, F64 = np.float32, np.float64
EPS = 8.0 * 2.0 ** -24
LAT = 1024  # lattice steps per unit
BOX_LO, BOX_HI = 256, 768  # lattice photons lie in [BOX_LO, BOX_HI)^3 / LAT


def dist2(photons, q):
    """(nq, n) float64 squared distances of the float32 inputs"""
    p = np.asarray(photons, F32)[:, :3].astype(F64)
    q = np.asarray(q, F32).astype(F64).reshape(-1, 3)
    out = np.zeros((len(q), len(p)), F64)
    for k in range(3):
        v = p[None, :, k] - q[:, None, k]
        out += v * v
    return out


def facing(photons, nrm):
    """(nq, n) bool: dir . n > 0 in float64 (exact on the lattice sets; the
    random sets keep |dir . n| > 1e-3)"""
    d = np.asarray(photons, F32)[:, 3:6].astype(F64)
    n = np.asarray(nrm, F32).astype(F64).reshape(-1, 3)
    return n @ d.T > 0.0


def in_range(D, r2, eps):
    """(sure, maybe): photons certainly inside the radius, and those that may be"""
    r2 = np.asarray(r2, F32).astype(F64).reshape(-1, 1)
    return D < r2 * (1.0 - eps), D < r2 * (1.0 + eps)


def boundary_queries(D, r2, eps=EPS):
    """(nq,) bool: some photon's d2 lies within the factor of r2"""
    sure, maybe = in_range(D, r2, eps)
    return (sure != maybe).any(axis=1)


def nearest_sets(photons, q, nrm, r2, eps):
    """-> (ok (nq, n) bool, may_miss (nq,) bool, D). ok[s, i]: photon i is a right
    answer of query s; may_miss[s]: -1 is one."""
    D = dist2(photons, q)
    face = facing(photons, nrm)
    sure, maybe = in_range(D, r2, eps)
    sure &= face
    maybe &= face
    best = np.where(sure, D, np.inf).min(axis=1, initial=np.inf)
    ok = maybe & (D <= best[:, None] * (1.0 + eps))
    return ok, ~sure.any(axis=1), D


def check_nearest(photons, q, nrm, r2, got, eps):
    """Asserts every answer; returns how many queries found a photon."""
    ok, may_miss, D = nearest_sets(photons, q, nrm, r2, eps)
    got = np.asarray(got)
    n = D.shape[1]
    assert ((got >= -1) & (got < max(n, 1))).all() and (n > 0 or (got == -1).all())
    miss = got < 0
    assert may_miss[miss].all(), np.flatnonzero(miss & ~may_miss)[:8]
    s = np.flatnonzero(~miss)
    bad = s[~ok[s, got[s]]]
    assert len(bad) == 0, [(int(b), int(got[b]), D[b, got[b]], D[b][ok[b]][:3]) for b in bad[:4]]
    if eps == 0.0 and len(s):  # stated once more for the exact family: the brute-force minimum itself
        elig = facing(photons, nrm) & (D < np.asarray(r2, F32).astype(F64).reshape(-1, 1))
        assert (D[s, got[s]] == np.where(elig, D, np.inf).min(axis=1)[s]).all()
    return len(s)


def check_gather(photons, q, r2, K, count, idx, d2, r2_out, eps):
    """Asserts every gather (count (nq,), idx / d2 (nq, K) in heap order, r2_out
    (nq,)); returns (queries that found < K, exactly the K in range, K of more)."""
    D = dist2(photons, q)
    r2 = np.asarray(r2, F32)
    sure, maybe = in_range(D, r2, eps)
    classes = [0, 0, 0]
    for s in range(len(D)):
        m = int(count[s])
        ns, nm = int(sure[s].sum()), int(maybe[s].sum())
        assert min(K, ns) <= m <= min(K, nm), (s, m, ns, nm)
        R = np.asarray(idx[s, :m])
        got = np.asarray(d2[s, :m], F32)
        assert (idx[s, m:] == -1).all()
        assert len(set(R.tolist())) == m and ((R >= 0) & (R < D.shape[1])).all(), (s, R)
        assert maybe[s, R].all(), (s, "a photon outside the radius")
        # the d2 returned is the float32 d2 of that photon
        assert (np.abs(got.astype(F64) - D[s, R]) <= eps * D[s, R]).all(), (s, got, D[s, R])
        if m == K:
            # whoever is closer than the farthest photon returned was returned
            T = D[s, R].max()
            closer = np.flatnonzero(maybe[s] & (D[s] * (1.0 + eps) < T))
            assert np.isin(closer, R).all(), (s, "a closer photon was left out")
            assert F32(r2_out[s]) == got[0] == got.max(), (s, r2_out[s], got[0])  # maxDistSquared = heap top
            for i in range(1, m):  # std::make_heap / push_heap invariant
                assert got[(i - 1) // 2] >= got[i], (s, i)
        else:
            assert np.isin(np.flatnonzero(sure[s]), R).all(), (s, "a photon inside the radius was left out")
            assert F32(r2_out[s]).view(np.uint32) == r2[s].view(np.uint32), (s, r2_out[s], r2[s])
        if eps == 0.0:  # the exact family once more, as the multiset of the K smallest
            want = np.sort(D[s][maybe[s]])[:K]
            assert (np.sort(got.astype(F64)) == want).all(), (s, np.sort(got), want)
        classes[0 if m < K else (1 if nm == K else 2)] += 1
    return tuple(classes)


# ------------------------------------------------------------------ inputs

def _colours(n):
    i = np.arange(n, dtype=F64)
    return np.stack([i, i + 0.5, -i], axis=1).astype(F32)  # exact below 2^23


def _lattice_dirs(rng, n):
    d = rng.integers(-2, 3, size=(n, 3)).astype(F32) * F32(0.5)
    d[(d == 0).all(axis=1)] = (0.5, 0.0, -1.0)
    return d


def lattice_photons(n, seed):
    """(n, 9) float32 [pos, dir, colour (i, i + 0.5, -i)]. From 100 photons on:
    coincident clusters of 300 (> the gather heap's cap of 256), 60 and 10 as
    far as n allows, a fifth of the photons on the plane x = 1/2 and a tenth on
    the line x = 1/2, y = 3/8, so that median splits meet equal keys on both
    sides; below that, n = 2 and 3 hold one coincident pair."""
    rng = np.random.default_rng(seed)
    pos = rng.integers(BOX_LO, BOX_HI, size=(n, 3))
    if n >= 100:
        at = 0
        for size in (300, 60, 10, 10):
            if at + size <= n // 2:
                pos[at:at + size] = pos[at]
                at += size
        plane = np.arange(at, at + n // 5)
        pos[plane, 0] = 512
        line = plane[: n // 10]
        pos[line, 1] = 384
        pos = pos[rng.permutation(n)]
    elif n in (2, 3):
        pos[1] = pos[0]
    out = np.zeros((n, 9), F32)
    out[:, :3] = pos.astype(F32) / F32(LAT)
    out[:, 3:6] = _lattice_dirs(rng, n)
    out[:, 6:] = _colours(n)
    return out


def lattice_queries(photons, nodes, nq, seed):
    """(pos (nq, 3), nrm (nq, 3)) on the lattice: a quarter at photon
    positions, a quarter on split planes of the tree `nodes` ((nn, 2) u32; p[axis]
    == split), an eighth far outside the photons' bound, the rest anywhere in
    it."""
    rng = np.random.default_rng(seed)
    n = len(photons)
    q = rng.integers(BOX_LO, BOX_HI, size=(nq, 3)).astype(F32) / F32(LAT)
    a, b, c = nq // 4, nq // 2, nq // 2 + nq // 8
    if n:
        q[:a] = photons[rng.integers(0, n, size=a), :3]
    if nodes is not None and len(nodes):
        inner = np.flatnonzero((nodes[:, 1] & 3) != 3)
        if len(inner):
            pick = inner[rng.integers(0, len(inner), size=b - a)]
            q[np.arange(a, b), nodes[pick, 1] & 3] = nodes[pick, 0].view(F32)
    far = rng.integers(0, 32, size=(c - b, 3)) + (LAT - 32) * rng.integers(0, 2, size=(c - b, 3))
    q[b:c] = far.astype(F32) / F32(LAT)
    return q, _lattice_dirs(rng, nq)


def random_photons(n, seed):
    """(n, 9) float32: positions uniform in the unit cube, directions drawn from
    32 unit vectors (so that a normal can keep clear of every photon's
    direction, however many photons there are), colour (i, i + 0.5, -i)."""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, 9), F32)
    out[:, :3] = rng.random((n, 3), dtype=F32)
    d = rng.normal(size=(32, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    out[:, 3:6] = d[rng.integers(0, 32, size=n)]
    out[:, 6:] = _colours(n)
    return out


def random_queries(photons, nq, seed):
    """(pos, nrm) float32; normals redrawn until |dir . n| > 1e-3 for every
    photon, so the facing test is never in doubt. A tenth of the queries lie
    outside the unit cube."""
    rng = np.random.default_rng(seed)
    q = rng.random((nq, 3), dtype=F32)
    out = nq // 10
    q[:out] = (q[:out] * F32(4.0) - F32(1.5)).astype(F32)
    nrm = np.zeros((nq, 3), F32)
    todo = np.arange(nq)
    d = np.unique(np.asarray(photons, F32)[:, 3:6], axis=0).astype(F64)
    while len(todo):
        v = rng.normal(size=(len(todo), 3))
        nrm[todo] = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)
        if len(d) == 0:
            break
        todo = todo[(np.abs(nrm[todo].astype(F64) @ d.T) <= 1e-3).any(axis=1)]
    return q, nrm


def gather_radii(D, K, exact):
    """Per query, squared radii (float32) that hold fewer than K photons,
    exactly K where the distances allow it, and all of them: (nq, 3). exact
    (lattice): the radii are distances of photons, which the `<` test must then
    exclude; otherwise they lie half way between two neighbouring distances."""
    nq, n = D.shape
    S = np.sort(D, axis=1)
    r = np.full((nq, 3), 64.0, F32)  # all: no query is further than 5 from a photon
    if n == 0:
        return r
    few = min(K, n) // 2  # the radius stops at photon number `few` (0-based): at most few < K inside
    if exact:
        r[:, 0] = S[:, few]
    else:
        r[:, 0] = 0.5 * (S[:, few - 1] + S[:, few]) if few else 0.5 * S[:, 0]
    if n > K:  # K inside when the K-th and (K+1)-th distances differ; n == K: the third column
        r[:, 1] = S[:, K] if exact else 0.5 * (S[:, K - 1] + S[:, K])
    return r
