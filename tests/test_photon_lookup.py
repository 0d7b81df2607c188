"""The photon-map lookups against a float64 brute force over all photons
(tests/photon_lookup_ref.py), through include/yk_test_hooks_photon.h: a
synthetic map takes yk_photon_build's steps from the kd-tree build on, and
host queries run through

* the host's point_tree_build / point_tree_lookup (CPU tests),
* pm_gather and pm_nearest, one query per thread (pt_lookup_step over the
  8-byte nodes with the per-thread ScratchStack; no render kernel instantiates
  the LdsStack form of pt_lookup_s, so there is none to compare),
* the production k_pm_lookup (pt_lookup_step_pk over the 16-byte nodes), in
  its LDS-stack and scratch-stack instantiations, on queues whose lengths walk
  the hand-out's arithmetic.

Lattice sets are checked for equality, ties as sets; random float32 sets
within the derived factor 1 + 8 * 2^-24 (photon_lookup_ref's docstring). The
gather heap is compared index for index with oracle.point_gather, which runs
libstdc++'s make_heap / pop_heap / push_heap.
"""
import ctypes as C
import time

import numpy as np
import pytest

from core_amd import _abi as A
from oracle import oracle as O
from tests import photon_lookup_ref as R

F32, F64 = np.float32, np.float64
DIFFUSE, CAUSTIC, RADIANCE = A.YK_PHOTON_MAP_DIFFUSE, A.YK_PHOTON_MAP_CAUSTIC, A.YK_PHOTON_MAP_RADIANCE
KS = [1, 2, 7, 50, 256]
FAMILIES = ["lattice", "random"]


class yk_photon_map_info(C.Structure):
    _fields_ = [("photons", C.c_int32), ("nodes", C.c_int32), ("depth", C.c_int32), ("lookup_lds", C.c_int32),
                ("lookup_grid", C.c_int32), ("reserved", C.c_int32)]


i32, i64, vp, fp = C.c_int32, C.c_int64, C.c_void_p, A.fp
HOOKS = {  # include/yk_test_hooks_photon.h, bound here: not part of the product ABI table
    "yk_debug_photon_load": [vp, i32, fp, i32, i32, C.POINTER(yk_photon_map_info)],
    "yk_debug_photon_gather": [vp, i32, fp, fp, i64, i32, vp, vp, fp, fp],
    "yk_debug_photon_nearest": [vp, i32, fp, fp, fp, i64, vp],
    "yk_debug_photon_lookup_queue": [vp, fp, i64, C.c_float, i32, fp, i64, A.i32p, A.i32p],
    "yk_debug_photon_host_tree": [fp, i32, vp, i64, A.i32p, A.i32p],
    "yk_debug_photon_host_gather": [fp, i32, fp, fp, i64, i32, vp, vp, fp, fp],
    "yk_debug_photon_host_nearest": [fp, i32, fp, fp, fp, i64, vp],
}


def hook(name):
    fn = getattr(A.lib(), name)
    fn.restype, fn.argtypes = C.c_int, HOOKS[name]
    return fn


def _f(a):
    return a.ctypes.data_as(fp)


@pytest.fixture
def hooks(monkeypatch):
    monkeypatch.setenv("YK_DEBUG_HOOKS", "1")


# ------------------------------------------------------------ call wrappers

def host_tree(photons):
    """point_tree_build -> (nodes (2n - 1, 2) u32, depth)"""
    photons = np.ascontiguousarray(photons, F32)
    n = len(photons)
    nodes = np.zeros((max(2 * n - 1, 1), 2), np.uint32)
    nn, depth = i32(), i32()
    A.check(hook("yk_debug_photon_host_tree")(_f(photons), n, nodes.ctypes.data, len(nodes), C.byref(nn),
                                              C.byref(depth)))
    return nodes[:nn.value], depth.value


def _gather(call, q, r2, K):
    q, r2 = np.ascontiguousarray(q, F32), np.ascontiguousarray(r2, F32)
    nq = len(q)
    count = np.full(nq, -7, np.int32)
    idx = np.zeros((nq, K), np.int32)
    d2 = np.zeros((nq, K), F32)
    r2_out = np.zeros(nq, F32)
    rc = call(_f(q), _f(r2), nq, K, count.ctypes.data, idx.ctypes.data, _f(d2), _f(r2_out))
    return rc, count, idx, d2, r2_out


def host_gather(photons, q, r2, K, check=True):
    photons = np.ascontiguousarray(photons, F32)
    out = _gather(lambda *a: hook("yk_debug_photon_host_gather")(_f(photons), len(photons), *a), q, r2, K)
    if check:
        A.check(out[0])
    return out


def dev_gather(dev, which, q, r2, K, check=True):
    out = _gather(lambda *a: hook("yk_debug_photon_gather")(dev._p, which, *a), q, r2, K)
    if check:
        A.check(out[0])
    return out


def host_nearest(photons, q, nrm, r2):
    photons, q, nrm, r2 = (np.ascontiguousarray(x, F32) for x in (photons, q, nrm, r2))
    out = np.full(len(q), -7, np.int32)
    A.check(hook("yk_debug_photon_host_nearest")(_f(photons), len(photons), _f(q), _f(nrm), _f(r2), len(q),
                                                 out.ctypes.data))
    return out


def dev_nearest(dev, which, q, nrm, r2):
    q, nrm, r2 = (np.ascontiguousarray(x, F32) for x in (q, nrm, r2))
    out = np.full(len(q), -7, np.int32)
    A.check(hook("yk_debug_photon_nearest")(dev._p, which, _f(q), _f(nrm), _f(r2), len(q), out.ctypes.data))
    return out


def dev_load(dev, which, photons, depth_limit=0, check=True):
    photons = np.ascontiguousarray(photons, F32).reshape(-1, 9)
    info = yk_photon_map_info()
    rc = hook("yk_debug_photon_load")(dev._p, which, _f(photons), len(photons), depth_limit, C.byref(info))
    if check:
        A.check(rc)
    return rc, info


def dev_queue(dev, lq, rad2, lcol, force_scratch=False, check=True):
    """k_pm_lookup over lq (nq, 8) on a copy of lcol -> (rc, lcol, lds, grid)"""
    lq = np.ascontiguousarray(lq, F32).reshape(-1, 8)
    col = np.array(lcol, F32)
    lds, grid = i32(-1), i32(-1)
    rc = hook("yk_debug_photon_lookup_queue")(dev._p, _f(lq), len(lq), float(rad2), 1 if force_scratch else 0, _f(col),
                                              col.size, C.byref(lds), C.byref(grid))
    if check:
        A.check(rc)
    return rc, col, lds.value, grid.value


# ------------------------------------------------------------------- inputs

_cache = {}


def photon_set(family, n):
    key = (family, n)
    if key not in _cache:
        _cache[key] = (R.lattice_photons if family == "lattice" else R.random_photons)(n, 1000 + n)
    return _cache[key]


def query_set(family, n, nq):
    """(pos, nrm) for the set (family, n); the lattice queries use the host
    tree's split planes (YK_DEBUG_HOOKS must be set)"""
    key = (family, n, nq)
    if key not in _cache:
        ph = photon_set(family, n)
        if family == "lattice":
            _cache[key] = R.lattice_queries(ph, host_tree(ph)[0] if n else None, nq, 77 + n)
        else:
            _cache[key] = R.random_queries(ph, nq, 77 + n)
    return _cache[key]


def eps_of(family):
    return 0.0 if family == "lattice" else R.EPS


def gather_case(family, n, K, nq=48):
    """nq queries with each of the three radii -> (pos (3 nq, 3), r2 (3 nq,))"""
    key = ("gather", family, n, K, nq)
    if key not in _cache:
        q, _ = query_set(family, n, nq)
        r = R.gather_radii(R.dist2(photon_set(family, n), q), K, family == "lattice")
        _cache[key] = (np.repeat(q, 3, axis=0), r.reshape(-1))
    return _cache[key]


def check_gather_case(family, n, K, out):
    """The brute-force check of one gather_case, the radius classes it must have
    reached, and the random family's boundary budget."""
    _, count, idx, d2, r2_out = out
    q, r2 = gather_case(family, n, K)
    ph = photon_set(family, n)
    few, exactly, more = R.check_gather(ph, q, r2, K, count, idx, d2, r2_out, eps_of(family))
    if n == 0:
        assert (count == 0).all() and (r2_out.view(np.uint32) == r2.view(np.uint32)).all()
    if n >= 1000:  # radii that hold fewer than K photons, exactly K, and more (the tiny sets: what they can)
        assert few > 0 and exactly > 0 and more > 0, (few, exactly, more)
    assert few + exactly + more == len(q)
    if family == "random" and n:
        assert R.boundary_queries(R.dist2(ph, q), r2).mean() < 0.01
    return count, idx, d2, r2_out


def nearest_radii(family, n, nq):
    """squared radii: a third hold a handful of photons; a third equal the
    distance of the nearest facing photon, which `<` must then exclude
    (lattice), or hold nothing (random); the rest hold everything"""
    key = ("nr", family, n, nq)
    if key not in _cache:
        q, nrm = query_set(family, n, nq)
        ph = photon_set(family, n)
        r2 = np.full(nq, 64.0, F32)
        if n:
            D = R.dist2(ph, q)
            S = np.sort(D, axis=1)
            k = min(n - 1, 6)
            a = np.arange(0, nq, 3)
            r2[a] = S[a, k] if family == "lattice" else 0.5 * (S[a, k] + S[a, k - 1] if k else S[a, 0])
            b = np.arange(1, nq, 3)
            if family == "lattice":
                best = np.where(R.facing(ph, nrm), D, np.inf).min(axis=1)
                r2[b] = np.where(np.isfinite(best[b]) & (best[b] > 0), best[b], 64.0)
            else:  # half way to the nearest photon: nothing in range
                r2[b] = 0.5 * S[b, 0]
        _cache[key] = r2
    return _cache[key]


def check_nearest_case(family, n, nq, got):
    q, nrm = query_set(family, n, nq)
    r2 = nearest_radii(family, n, nq)
    ph = photon_set(family, n)
    found = R.check_nearest(ph, q, nrm, r2, got, eps_of(family))
    if n >= 1000:
        assert 0 < found < nq  # some queries have no facing photon in range, some have one
    if family == "random" and n:
        assert R.boundary_queries(R.dist2(ph, q), r2).mean() < 0.01


# -------------------------------------------------------------- CPU: refusals

def test_the_hooks_are_outside_the_product_table_and_off_by_default(monkeypatch):
    monkeypatch.delenv("YK_DEBUG_HOOKS", raising=False)
    z = np.zeros(9, F32)
    for name, args in HOOKS.items():
        assert name not in A.SIGNATURES
        rc = hook(name)(*[0 if t in (i32, i64) else (0.0 if t is C.c_float else None) for t in args])
        assert rc == A.YK_ERR_UNSUPPORTED and b"YK_DEBUG_HOOKS" in A.lib().yk_last_error(), name
    assert host_gather(z.reshape(1, 9), z[:3].reshape(1, 3), [1.0], 1, check=False)[0] == A.YK_ERR_UNSUPPORTED


def test_host_gather_refuses_k_outside_1_to_256(hooks):
    ph = photon_set("lattice", 3)
    q = ph[:1, :3]
    for K in (0, -1, 257):
        # the wrapper's arrays must hold K >= 1 columns whatever K is asked for
        count, idx = np.zeros(1, np.int32), np.zeros((1, 300), np.int32)
        d2, r2o = np.zeros((1, 300), F32), np.zeros(1, F32)
        rc = hook("yk_debug_photon_host_gather")(_f(ph), 3, _f(q), _f(np.ones(1, F32)), 1, K, count.ctypes.data,
                                                 idx.ctypes.data, _f(d2), _f(r2o))
        assert rc == A.YK_ERR_UNSUPPORTED and b"[1, 256]" in A.lib().yk_last_error(), K
    assert host_gather(ph, q, [1.0], 256)[0] == A.YK_OK


# ------------------------------------------------------- CPU: the host tree

@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n", [1, 2, 3, 5, 1000, 32768, 32769])
def test_host_tree_structure(hooks, family, n):
    ph = photon_set(family, n)
    nodes, depth = host_tree(ph)
    assert len(nodes) == 2 * n - 1
    assert depth == int(np.ceil(np.log2(n))) + 1
    leaf = (nodes[:, 1] & 3) == 3
    assert sorted(nodes[leaf, 0].tolist()) == list(range(n))  # every photon in exactly one leaf
    assert (nodes[leaf, 1] == 3).all()
    axis = (nodes[:, 1] & 3).astype(np.int64)
    right = (nodes[:, 1] >> 2).astype(np.int64)
    split = nodes[:, 0].view(F32)
    # children have larger indices than their parent (left = node + 1), so one
    # backward sweep gives every subtree's bound and size, one forward sweep its level
    lo, hi = np.zeros((len(nodes), 3), F32), np.zeros((len(nodes), 3), F32)
    size = np.ones(len(nodes), np.int64)
    for i in range(len(nodes) - 1, -1, -1):
        if leaf[i]:
            lo[i] = hi[i] = ph[nodes[i, 0], :3]
            continue
        l, r, a = i + 1, right[i], axis[i]
        assert i + 1 < r < len(nodes)
        assert l + size[l] == r, i  # the left subtree ends where the right one starts
        assert hi[l, a] <= split[i] <= lo[r, a], (i, hi[l, a], split[i], lo[r, a])
        lo[i], hi[i] = np.minimum(lo[l], lo[r]), np.maximum(hi[l], hi[r])
        size[i] = 1 + size[l] + size[r]
    assert size[0] == len(nodes)
    level = np.zeros(len(nodes), np.int64)
    level[0] = 1
    for i in range(len(nodes)):
        if not leaf[i]:
            level[i + 1] = level[right[i]] = level[i] + 1
    assert level[leaf].max() == depth
    if family == "lattice" and n >= 1000:  # equal keys on both sides of some median split
        inner = np.flatnonzero(~leaf)
        a = axis[inner]
        assert ((hi[inner + 1, a] == split[inner]) & (lo[right[inner], a] == split[inner])).any()


# ---------------------------------------------------- CPU: the host lookups

@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("n", [0, 1, 2, 3, 1000])
def test_host_gather_against_the_brute_force(hooks, family, n, K):
    q, r2 = gather_case(family, n, K)
    ph = photon_set(family, n)
    count, idx, _, r2_out = check_gather_case(family, n, K, host_gather(ph, q, r2, K))
    if n:  # libstdc++ here, libstdc++ in the oracle: the same heap, index for index
        for s in range(0, len(q), 5):
            oi, od, orad = O.point_gather(ph[:, :3], q[s], K, r2[s])
            assert oi.tolist() == idx[s, :count[s]].tolist() and F32(orad) == r2_out[s], s


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n,nq", [(0, 30), (1, 30), (2, 30), (3, 30), (1000, 300), (32768, 120), (32769, 120)])
def test_host_nearest_against_the_brute_force(hooks, family, n, nq):
    q, nrm = query_set(family, n, nq)
    check_nearest_case(family, n, nq, host_nearest(photon_set(family, n), q, nrm, nearest_radii(family, n, nq)))


# --------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def pdev(gpu_device):
    """A device handle of this module's own: loading a synthetic map drops the
    maps of a handle's last yk_photon_build."""
    from core_amd.device import Device
    d = Device(0)
    d.loaded = {}
    yield d
    d.close()


def ensure_map(dev, which, family, n):
    """Loads (family, n) into slot `which` unless it is there already -> info"""
    if dev.loaded.get(which, (None,))[0] != (family, n):
        dev.loaded[which] = ((family, n), dev_load(dev, which, photon_set(family, n))[1])
    return dev.loaded[which][1]


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("n", [0, 1, 2, 3, 1000])
def test_device_gather_against_the_brute_force(pdev, hooks, family, n, K):
    which = DIFFUSE if family == "lattice" else CAUSTIC
    info = ensure_map(pdev, which, family, n)
    assert (info.photons, info.nodes) == (n, max(2 * n - 1, 0))
    q, r2 = gather_case(family, n, K)
    ph = photon_set(family, n)
    count, idx, d2, r2_out = check_gather_case(family, n, K, dev_gather(pdev, which, q, r2, K))
    if n:  # the device's heap restatement against libstdc++, through the oracle and through the host
        for s in range(0, len(q), 5):
            oi, od, orad = O.point_gather(ph[:, :3], q[s], K, r2[s])
            assert oi.tolist() == idx[s, :count[s]].tolist(), s
            assert (od.view(np.uint32) == d2[s, :count[s]].view(np.uint32)).all() and F32(orad) == r2_out[s], s
        _, hc, hi, hd, hr = host_gather(ph, q, r2, K)
        assert (hc == count).all() and (hi == idx).all()
        assert (hd.view(np.uint32) == d2.view(np.uint32)).all() and (hr.view(np.uint32) == r2_out.view(np.uint32)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("which", [DIFFUSE, CAUSTIC, RADIANCE])
@pytest.mark.parametrize("n,nq", [(0, 30), (1, 30), (2, 30), (3, 30), (1000, 300)])
def test_device_nearest_against_the_brute_force(pdev, hooks, family, which, n, nq):
    ensure_map(pdev, which, family, n)
    q, nrm = query_set(family, n, nq)
    got = dev_nearest(pdev, which, q, nrm, nearest_radii(family, n, nq))
    check_nearest_case(family, n, nq, got)
    if family == "lattice":  # ties included, the host's traversal makes the device's choices
        assert (got == host_nearest(photon_set(family, n), q, nrm, nearest_radii(family, n, nq))).all()


# ----------------------------------------------------------- k_pm_lookup

def sentinel(owners):
    """lcol prefill of owner c: no photon's colour (their first component is >= 0)"""
    c = np.asarray(owners, F64)
    return np.stack([-(c + 1.0), np.full(len(c), 0.25), c + 1.0], axis=1).astype(F32)


def queue_case(family, n, nd, rad2_rank=8):
    """nd distinct queries on the radiance set (family, n), one squared radius
    for all of them (lattice: the last query's distance to its photon number
    rad2_rank, which `<` excludes), and the brute-force answer sets."""
    key = ("queue", family, n, nd)
    if key not in _cache:
        q, nrm = query_set(family, n, nd)
        ph = photon_set(family, n)
        d0 = np.sort(R.dist2(ph, q[-1:])[0])  # the last query lies anywhere inside the photons' bound
        rad2 = F32(d0[rad2_rank]) if family == "lattice" else F32(0.5 * (d0[rad2_rank] + d0[rad2_rank + 1]))
        if family == "lattice" and rad2 == 0:
            rad2 = F32(d0[d0 > 0][0])
        ok, may_miss, D = R.nearest_sets(ph, q, nrm, np.full(nd, rad2, F32), eps_of(family))
        must_find = ok.any(axis=1) & ~may_miss
        # a dropped query and a missed one must not look alike: both kinds of query, in numbers
        assert may_miss.mean() > 0.05 and must_find.mean() > 0.05, (may_miss.mean(), must_find.mean())
        if family == "lattice":
            assert (D == F64(rad2)).any()  # a photon exactly on the radius
        else:
            assert R.boundary_queries(D, np.full(nd, rad2, F32)).mean() < 0.01
        _cache[key] = (q, nrm, rad2, ok, may_miss)
    return _cache[key]


def run_queue(dev, family, n, nd, nq, seed, force_scratch=False, tail=7):
    """A queue of nq entries: the nd distinct queries tiled under nq distinct
    owners, shuffled; checks every owner's colour and the entries beyond.
    -> (lcol, lds, grid, seconds of the hook call)"""
    q, nrm, rad2, ok, may_miss = queue_case(family, n, nd)
    rng = np.random.default_rng(seed)
    sel = rng.permutation(nq) % nd if nq else np.zeros(0, np.int64)  # which query each entry is
    owners = rng.permutation(nq).astype(np.int32)
    lq = np.zeros((nq, 8), F32)
    lq[:, 0:3] = q[sel]
    lq[:, 3] = owners.view(F32)
    lq[:, 4:7] = nrm[sel]
    before = sentinel(np.arange(nq + tail))
    t0 = time.perf_counter()
    _, col, lds, grid = dev_queue(dev, lq, rad2, before, force_scratch)
    dt = time.perf_counter() - t0
    assert (col[nq:].view(np.uint32) == before[nq:].view(np.uint32)).all()  # beyond the owners: untouched
    got = col[owners]  # entry order
    kept = (got.view(np.uint32) == before[owners].view(np.uint32)).all(axis=1)
    assert may_miss[sel[kept]].all(), ("owners left as they were although a photon is in range", int(kept.sum()))
    f = np.flatnonzero(~kept)
    i = got[f, 0].astype(np.int64)
    assert ((got[f, 0] >= 0) & (i < n)).all()
    assert (got[f].view(np.uint32) == photon_set(family, n)[i, 6:].view(np.uint32)).all()  # one photon's whole colour
    assert ok[sel[f], i].all(), ("not the brute force's photon", f[~ok[sel[f], i]][:8])
    return col, lds, grid, dt


@pytest.mark.gpu
@pytest.mark.parametrize("n,lds", [(32768, 1), (32769, 0)])
def test_lookup_kernel_on_either_side_of_the_lds_boundary(pdev, hooks, n, lds):
    """32768 photons: 65535 nodes, depth 16, child indices up to 65534 in 16
    bits; one photon more flips both of lookup_lds()'s conditions."""
    info = ensure_map(pdev, RADIANCE, "lattice", n)
    assert (info.nodes, info.depth, info.lookup_lds) == (2 * n - 1, 17 - lds, lds)
    _, ran_lds, grid, _ = run_queue(pdev, "lattice", n, 512, 3000,seed=n)
    assert ran_lds == lds and grid == info.lookup_grid
    _, forced, _, _ = run_queue(pdev, "lattice", n, 512, 3000,seed=n, force_scratch=True)
    assert forced == 0


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_lds_and_scratch_lookup_kernels_answer_alike(pdev, hooks, family):
    info = ensure_map(pdev, RADIANCE, family, 1000)
    assert info.lookup_lds == 1
    a, lds_a, _, _ = run_queue(pdev, family, 1000, 2048, 5000, seed=5)
    b, lds_b, _, _ = run_queue(pdev, family, 1000, 2048, 5000, seed=5, force_scratch=True)
    assert (lds_a, lds_b) == (1, 0)
    assert (a.view(np.uint32) == b.view(np.uint32)).all()


QUEUE_LENGTHS = [0, 1, 15, 16, 63, 64, 65, "64*grid+1", "128*8*grid+77"]


@pytest.mark.gpu
@pytest.mark.parametrize("scratch", [False, True], ids=["lds", "scratch"])
@pytest.mark.parametrize("length", QUEUE_LENGTHS)
def test_lookup_queue_hand_out(pdev, hooks, length, scratch):
    """Queue lengths below one wave, off a multiple of 64, one past a full
    round of 64-query chunks, and one where the chunk max(64, (n / (grid * 8))
    & ~63) is 128. Every owner holds its query's photon or still its sentinel."""
    ensure_map(pdev, RADIANCE, "lattice", 1000)
    grid = dev_queue(pdev, np.zeros((0, 8), F32), 1.0, np.zeros(3, F32), scratch)[3]
    assert grid >= 64
    nq = length if isinstance(length, int) else {"64*grid+1": 64 * grid + 1, "128*8*grid+77": 128 * 8 * grid + 77}[length]
    if length == "128*8*grid+77":
        assert max(64, (nq // (grid * 8)) & ~63) == 128
    elif nq:
        assert max(64, (nq // (grid * 8)) & ~63) == 64
    _, lds, ran_grid, dt = run_queue(pdev, "lattice", 1000, 4096, nq, seed=nq % 1000, force_scratch=scratch)
    assert lds == (0 if scratch else 1) and ran_grid == grid
    print(f"k_pm_lookup queue of {nq} ({'scratch' if scratch else 'lds'}, grid {grid}): hook call {dt * 1e3:.1f} ms")


# ------------------------------------------------------------ GPU: refusals

@pytest.mark.gpu
def test_device_hooks_refuse_without_the_environment(pdev, monkeypatch):
    monkeypatch.delenv("YK_DEBUG_HOOKS", raising=False)
    assert dev_load(pdev, DIFFUSE, photon_set("lattice", 3), check=False)[0] == A.YK_ERR_UNSUPPORTED
    q = np.zeros((1, 3), F32)
    assert dev_gather(pdev, DIFFUSE, q, [1.0], 1, check=False)[0] == A.YK_ERR_UNSUPPORTED
    assert dev_queue(pdev, np.zeros((0, 8), F32), 1.0, np.zeros(3, F32), check=False)[0] == A.YK_ERR_UNSUPPORTED


@pytest.mark.gpu
def test_device_refusals(pdev, hooks):
    ph = photon_set("lattice", 5)  # depth 4
    pdev.loaded.clear()
    assert dev_load(pdev, DIFFUSE, ph)[1].depth == 4
    # the depth check of yk_photon_build, with the bound lowered to where a test's tree reaches it
    rc, _ = dev_load(pdev, DIFFUSE, ph, depth_limit=3, check=False)
    assert rc == A.YK_ERR_UNSUPPORTED and b"too deep" in A.lib().yk_last_error()
    assert dev_load(pdev, DIFFUSE, ph, depth_limit=4)[0] == A.YK_OK
    assert dev_load(pdev, DIFFUSE, ph, depth_limit=1000)[0] == A.YK_OK  # never above the production bound
    # the refused load left the slot as it was
    q = ph[:2, :3]
    assert dev_gather(pdev, DIFFUSE, q, [64.0, 64.0], 5)[1].tolist() == [5, 5]
    for K in (0, -3, 257):
        count, idx = np.zeros(2, np.int32), np.zeros((2, 300), np.int32)
        d2, r2o = np.zeros((2, 300), F32), np.zeros(2, F32)
        rc = hook("yk_debug_photon_gather")(pdev._p, DIFFUSE, _f(q), _f(np.ones(2, F32)), 2, K, count.ctypes.data,
                                            idx.ctypes.data, _f(d2), _f(r2o))
        assert rc == A.YK_ERR_UNSUPPORTED and b"[1, 256]" in A.lib().yk_last_error(), K
    assert dev_load(pdev, 3, ph, check=False)[0] == A.YK_ERR_ARG
    # k_pm_lookup: an empty radiance slot, and owners outside the colour array
    dev_load(pdev, RADIANCE, np.zeros((0, 9), F32))
    assert dev_queue(pdev, np.zeros((0, 8), F32), 1.0, np.zeros(3, F32), check=False)[0] == A.YK_ERR_STATE
    dev_load(pdev, RADIANCE, ph)
    lq = np.zeros((2, 8), F32)
    lq[:, 3] = np.array([0, 1], np.int32).view(F32)
    col = sentinel(np.arange(2))
    assert dev_queue(pdev, lq, 64.0, col)[0] == A.YK_OK
    assert dev_queue(pdev, lq, 64.0, col[:1], check=False)[0] == A.YK_ERR_ARG
    lq[1, 3] = np.array([-1], np.int32).view(F32)[0]
    rc, out, _, _ = dev_queue(pdev, lq, 64.0, col, check=False)
    assert rc == A.YK_ERR_ARG and (out.view(np.uint32) == col.view(np.uint32)).all()
