"""Ray queries against a float64 brute force over all triangles
(tests/bruteforce.py): the check that shares neither the kd-tree, nor the
curve extrusion / instance flattening's leaf contents, nor the float32
Moller-Trumbore operation order with the code under test. The CPU tests put
the oracle (and with it the host kd-tree builder) under it, the gpu tests
every traversal kernel family of yk_trace_closest / yk_trace_shadow /
yk_trace_shadow_filtered.

Rules (bruteforce.py): on rays whose float64 decision has a margin (e = 1e-4
in the barycentrics, e_t = 1e-4 max(1, |t|), no strict candidate below
|det| = 1e-3 |e1||e2||dir|) the answer is the float64 one: same prim, misses
are misses, |t - t64| <= TOL_T max(1, |t64|), |b - b64| <= TOL_B, same
occlusion. On the other rays the answer must be possible.

Caps (conditions on the ray families, so that nothing passes by deciding
nothing; per scene and query): decided >= 80 % of `random` and `bounded`,
>= 40 % of `edge` and `graze`; decided hits >= 30 % of `random` and >= 15 % of
`bounded` (whose tmax is half the bound's diagonal). The camera rays of the
tie-in count as `random`.

Tolerances: the oracle against float64 on the CPU, over every scene, family
and the camera rays below (the CPU tests' rays), measured on decided hits
    max |t - t64| / max(1, |t64|) = 3.65e-6   (MEASURED_T)
    max |b - b64|                 = 1.64e-4   (MEASURED_B)
both on the hair scene, and TOL_T, TOL_B are 4x these maxima (the factor
covers float32 operation-order differences between compilers). Never measured
on the device. Decided rays of the CPU tests per scene (closest hit): cornell
2712 of 3060, bumpy 3009 of 3100, hair 3024, smooth_inst 2969, panes 2848,
universal 2953; on none of them, nor on the occlusion queries, do the oracle
and float64 disagree. Hits exempted by the grazing exclusion (bruteforce.
check_closest): 0 to 5 per scene, all in the `graze` family.

Transparent shadows: IntersectTS (kdtree.cc:953-1108) keeps a set of the
*triangles* it has filtered, not of panes or objects: a pane of the test scene
is one planar quad grid of 72 triangles, a ray crosses its plane once, and
where it does so inside one triangle that triangle is the pane's one
crossing. On a shared edge or diagonal two triangles of the pane can both
pass the float32 test and both count; there both are loose but not strict, so
the ray is undecided and either count is accepted. A decided ray has every
candidate strict, hence one triangle per pane: strict transparent crossings
are panes.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from core_amd import _abi as A
from core_amd.scene import probe_scene
from oracle.oracle import Oracle
from tests import bruteforce as B
from tests.raygen import edge_rays, graze_rays, random_rays
from tests.scenes import smooth_instanced, transparent_panes
from tests.test_universal import universal_scene

MEASURED_T = 3.65e-6  # hair; cornell 1.6e-7, bumpy 1.8e-6, smooth_inst 6.6e-7, panes 2.2e-7, universal 2.4e-6
MEASURED_B = 1.64e-4  # hair (triangles of ~1e-3 seen from ~1 away); the others 4.3e-7 ... 2.8e-5
TOL_T = 4 * MEASURED_T
TOL_B = 4 * MEASURED_B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = ["cornell", "bumpy", "hair", "smooth_inst", "panes", "universal"]
CPU_RAYS, GPU_RAYS = (1500, 500), (8000, 2000)
DEPTHS = (0, 1, 3, 8)

_S = {}


def _scene(name):
    """(scene, export, oracle, universal, transparent-triangle mask)"""
    if name not in _S:
        if name == "cornell":
            s, _ = probe_scene("cornell_pt", 32, 32)
        elif name == "bumpy":
            s, _ = probe_scene("bumpy", 32, 32, 120, 61)
        elif name == "hair":  # curve extrusion, crowded leaves
            s, _ = probe_scene("hair", 32, 32, 300, 9)
        elif name == "smooth_inst":  # instance flattening
            s, _, _ = smooth_instanced(32, 32)
        elif name == "panes":
            s, _ = transparent_panes(32, 32)
        else:
            s, _ = universal_scene(32)
        e = s.export()
        mats = s.materials()
        transp = np.array([m.type == A.YK_MAT_SHINYDIFFUSE and m.transparency > 0 for m in mats], bool)
        _S[name] = (s, e, Oracle(s), s.info().mode == A.YK_MODE_UNIVERSAL, transp[e["tri_material"]])
    return _S[name]


def _families(e, n_random, n_bounded, seed):
    """The ray families of one scene and their [start, end) ranges."""
    b = e["bound"]
    half_diag = 0.5 * float(np.linalg.norm(b[3:].astype(np.float64) - b[:3]))
    fams = [("random", random_rays(b, n_random, seed)),
            ("bounded", random_rays(b, n_bounded, seed + 1, tmax=half_diag)),
            ("edge", edge_rays(b, e["nodes"], seed + 2, 200, 300, 200)),
            ("graze", graze_rays(e["tri_verts"], b, 400, seed + 3))]
    ranges, at = {}, 0
    for name, r in fams:
        ranges[name] = (at, at + len(r))
        at += len(r)
    return np.concatenate([r for _, r in fams]), ranges


def _shadow_rays(rays, tmin):
    """tmin 0.0005: the bias the integrators pass, every other ray bounded (as
    test_trace_shadow_bit_exact); tmin 0: the closest-hit rays' own range."""
    r = rays.copy()
    r[:, 6] = tmin
    if tmin > 0:
        r[::2, 7] = np.abs(r[::2, 7]) + 0.3
    return r


CAPS = {"random": (0.80, 0.30), "bounded": (0.80, 0.15), "edge": (0.40, 0.0), "graze": (0.40, 0.0)}


def _caps(who, ranges, decided, decided_hit=None):
    for fam, (a, b) in ranges.items():
        cap_d, cap_h = CAPS[fam]
        d = float(decided[a:b].mean())
        h = float(decided_hit[a:b].mean()) if decided_hit is not None else 1.0
        print(f"  {who} {fam}: {b - a} rays, decided {d:.3f}" + (f", decided hits {h:.3f}" if decided_hit is not None
                                                                  else ""))
        assert d >= cap_d and h >= cap_h, (who, fam, d, h)


_BF = {}


def _truth(name, device, counts, seed=101):
    """Rays of scene `name` and their float64 answers, computed once per
    (scene, device): closest, shadow at tmin 0.0005 and at tmin 0."""
    key = (name, str(device))
    if key not in _BF:
        s, e, _, uni, _ = _scene(name)
        bf = B.BruteForce(e["tri_verts"], device)
        rays, ranges = _families(e, counts[0], counts[1], seed)
        sh = [_shadow_rays(rays, 0.0005), _shadow_rays(rays, 0.0)]
        _BF[key] = dict(bf=bf, rays=rays, ranges=ranges, closest=bf.closest(rays), shadow_rays=sh,
                        shadow=[bf.any_hit(r, "tmin" if uni else "zero") for r in sh])
    return _BF[key]


def _check_closest(who, T, hits, tol=True):
    prim, t, b1, b2 = hits
    c = T["closest"]
    fig = B.check_closest(T["bf"], T["rays"], c, prim, t, b1, b2, TOL_T if tol else None, TOL_B if tol else None, who)
    print(f"{who} closest: {fig}")
    _caps(who + " closest", T["ranges"], c["state"] != B.UNDECIDED, c["state"] == B.DECIDED_HIT)
    return fig


def _check_shadow(who, T, k, occ):
    a = T["shadow"][k]
    fig = B.check_occlusion(T["shadow_rays"][k], a, occ, f"{who} shadow[{k}]")
    print(f"{who} shadow[{k}]: {fig}")
    _caps(f"{who} shadow[{k}]", T["ranges"], a["strict"] | ~a["loose"])
    assert 0 < fig["occluded"] < fig["decided"]


# ---- CPU: the oracle (and the shared host tree builder) against float64 -----

@pytest.mark.parametrize("name", SCENES)
def test_oracle_closest_vs_float64(name):
    orc = _scene(name)[2]
    T = _truth(name, "cpu", CPU_RAYS)
    _check_closest(f"oracle {name}", T, orc.intersect(T["rays"])[:4])


@pytest.mark.parametrize("name", SCENES)
def test_oracle_shadow_vs_float64(name):
    orc = _scene(name)[2]
    T = _truth(name, "cpu", CPU_RAYS)
    for k in (0, 1):
        _check_shadow(f"oracle {name}", T, k, orc.shadow(T["shadow_rays"][k])[0])


def _camera_truth(device):
    key = ("camera", str(device))
    if key not in _BF:
        s, e, orc, _, _ = _scene("cornell")
        rays = orc.camera_rays(0, 0, 32, 32, 1)
        bf = B.BruteForce(e["tri_verts"], device)
        _BF[key] = dict(bf=bf, rays=rays, ranges={"random": (0, len(rays))}, closest=bf.closest(rays))
    return _BF[key]


def test_oracle_camera_rays_vs_float64():
    """The ray population the renders trace: cornell_pt 32x32, 1 spp."""
    T = _camera_truth("cpu")
    _check_closest("oracle camera", T, _scene("cornell")[2].intersect(T["rays"])[:4])


# ---- transparent shadows ----------------------------------------------------

def _ts_rays(e, n_random, n_bounded, n_vertical, seed):
    b = e["bound"]
    rng = np.random.default_rng(seed + 2)
    v = np.zeros((n_vertical, 8), np.float32)  # floor to light plane, through the panes
    v[:, 0] = rng.uniform(-0.5, 0.5, n_vertical)
    v[:, 1] = 0.01
    v[:, 2] = rng.uniform(-0.5, 0.5, n_vertical)
    v[:, 3:6] = rng.normal(size=(n_vertical, 3)) * 0.15 + np.array([0.0, 1.0, 0.0])
    v[:, 3:6] /= np.linalg.norm(v[:, 3:6], axis=1, keepdims=True)
    v[:, 6] = 0.0005
    v[:, 7] = 1.9
    r = np.concatenate([random_rays(b, n_random, seed), random_rays(b, n_bounded, seed + 1, tmax=1.0)])
    r[:, 6] = np.where(np.arange(len(r)) % 2 == 0, 0.0005, 0.0)
    ranges = {"random": (0, n_random), "bounded": (n_random, len(r)), "vertical": (len(r), len(r) + n_vertical)}
    return np.concatenate([r, v]), ranges


def _sub_rays(rays, a, idx):
    """For the rays idx (each crossing >= 2 panes): one ray per crossing, on
    the same line with the same direction bits, whose segment holds that
    crossing alone. Returns (sub rays, parent index per sub ray, crossed prim)."""
    out, parent, prim = [], [], []
    for i in idx:
        n = int(a["ncross"][i])
        ts = a["cross_t"][i, :n].astype(np.float64)
        for k in range(n):
            g0 = min(0.01, 0.5 * (ts[k] - ts[k - 1])) if k else 0.01
            g1 = min(0.01, 0.5 * (ts[k + 1] - ts[k])) if k + 1 < n else 0.01
            r = rays[i].copy()
            r[0:3] = (rays[i, 0:3].astype(np.float64)
                      + (float(rays[i, 6]) + ts[k] - g0) * rays[i, 3:6].astype(np.float64)).astype(np.float32)
            r[6] = 0.0
            r[7] = g0 + g1
            out.append(r)
            parent.append(i)
            prim.append(a["cross_prim"][i, k])
    return np.asarray(out, np.float32).reshape(-1, 8), np.asarray(parent), np.asarray(prim)


def _check_filtered(who, device, counts, trace):
    """trace(rays, depth) -> (occluded, filter (n, 3))."""
    s, e, _, _, transp = _scene("panes")
    key = ("ts", str(device))
    if key not in _BF:
        bf = B.BruteForce(e["tri_verts"], device)
        rays, ranges = _ts_rays(e, counts[0], counts[1], 600, 131)
        _BF[key] = (bf, rays, ranges, bf.any_hit(rays, "tmin", transp))
    bf, rays, ranges, a = _BF[key]
    for fam, (lo, hi) in ranges.items():
        d = float((~a["ambiguous"][lo:hi]).mean())
        print(f"  {who} {fam}: {hi - lo} rays, decided {d:.3f}")
        assert d >= 0.80, (fam, d)
    answers = {}
    for depth in DEPTHS:
        occ, filt = trace(rays, depth)
        fig, free = B.check_filtered_occlusion(rays, a, depth, occ, who)
        print(f"{who} depth {depth}: {fig}, crossings of the free rays {np.bincount(a['ncross'][free]).tolist()}")
        assert 0 < fig["occluded"] < fig["decided"]
        answers[depth] = (np.asarray(filt, np.float32), free)
    # depth limits bite: fewer free rays at smaller depths
    assert answers[0][1].sum() < answers[1][1].sum() < answers[3][1].sum() == answers[8][1].sum()
    # filter colour: the filter of a decided ray through panes {A, B, ...}
    # equals the product of the filters of decided rays through one pane each
    filt, free = answers[8]
    assert (filt[free & (a["ncross"] == 0)] == 1.0).all()
    multi = np.flatnonzero(free & (a["ncross"] >= 2))
    sub, parent, prim = _sub_rays(rays, a, multi)
    sa = bf.any_hit(sub, "tmin", transp)
    s_occ, s_filt = trace(sub, 8)
    _, s_free = B.check_filtered_occlusion(sub, sa, 8, s_occ, who + " single-pane")
    good = s_free & (sa["ncross"] == 1) & (sa["cross_prim"][:, 0] == prim)
    usable = np.array([good[parent == i].all() for i in multi], bool)
    print(f"{who}: {len(multi)} rays through several panes, {usable.sum()} with decided single-pane rays")
    assert usable.sum() >= 0.25 * 600  # of the vertical family alone
    ulp = 2.0 ** -23
    for i in multi[usable]:
        f = np.asarray(s_filt, np.float32)[parent == i].astype(np.float64)
        prod = f.prod(axis=0)
        assert (np.abs(filt[i].astype(np.float64) - prod) <= 4 * len(f) * ulp * prod).all(), (i, filt[i], prod)


def test_oracle_filtered_shadow_vs_float64():
    orc = _scene("panes")[2]
    _check_filtered("oracle", "cpu", CPU_RAYS, lambda r, d: orc.shadow_ts(r, d)[:2])


# ---- GPU: every traversal kernel family against float64 ---------------------

def _small_bytes(dev):
    nb = C.c_int64(-1)
    A.check(A.lib().yk_debug_small_scene(dev._p, C.byref(nb)))
    return nb.value


def _device_answers(dev, T):
    hits = dev.split_hits(dev.trace_closest(dev.rays_to_device(T["rays"])))
    occ = [dev.trace_shadow(dev.rays_to_device(r)).cpu().numpy() for r in T["shadow_rays"]]
    return hits, occ


# (scene, YK_SMALL, LDS small-scene kernels expected)
GPU_CASES = [("cornell", None, True), ("cornell", "0", False), ("bumpy", None, False), ("bumpy", "0", False),
             ("hair", None, False), ("smooth_inst", None, False), ("universal", None, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,small,lds", GPU_CASES, ids=[f"{c[0]}-small{c[1]}" for c in GPU_CASES])
def test_device_vs_float64(gpu_device, monkeypatch, name, small, lds):
    monkeypatch.setenv("YK_DEBUG_HOOKS", "1")
    if small is None:
        monkeypatch.delenv("YK_SMALL", raising=False)
    else:
        monkeypatch.setenv("YK_SMALL", small)
    s = _scene(name)[0]
    gpu_device.upload(s)
    assert (_small_bytes(gpu_device) > 0) == lds  # the kernel family under test
    if name == "hair":
        # yk_upload_host.inc crowded(): a tree is crowded when its mean references per
        # filled leaf exceed YK_CROWDED_LEAF (default 8). At 300 strands the
        # mean is 2.8: the default takes the ordinary ray hand-out, and
        # test_device_hair_crowded_leaf_path forces the other one.
        i = s.info()
        assert "YK_CROWDED_LEAF" not in os.environ and i.leaf_refs <= 8.0 * (i.leaves - i.empty_leaves)
    T = _truth(name, gpu_device.torch_device, GPU_RAYS)
    hits, occ = _device_answers(gpu_device, T)
    _check_closest(f"device {name}", T, hits)
    for k in (0, 1):
        _check_shadow(f"device {name}", T, k, occ[k])


@pytest.mark.gpu
def test_device_hair_crowded_leaf_path(gpu_device, tmp_path):
    """The crowded-leaf ray hand-out (64-ray chunks) on the hair scene.
    YK_CROWDED_LEAF is read once per process (a function-local static in
    crowded()), so the setting other than the default needs a process of its
    own: tests/ground_truth_worker.py traces the same rays with the threshold
    below the scene's mean references per filled leaf (2.8, uncrowded at the
    default 8: test_device_vs_float64[hair])."""
    s = _scene("hair")[0]
    i = s.info()
    mean = i.leaf_refs / (i.leaves - i.empty_leaves)
    on = 1.0
    assert on < mean <= 8.0
    T = _truth("hair", gpu_device.torch_device, GPU_RAYS)
    src, dst = str(tmp_path / "rays.npz"), str(tmp_path / "answers.npz")
    np.savez(src, rays=T["rays"], shadow0=T["shadow_rays"][0], shadow1=T["shadow_rays"][1])
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), YK_CROWDED_LEAF=str(on))
    subprocess.run([sys.executable, "-m", "tests.ground_truth_worker", src, dst], cwd=ROOT, env=env, check=True,
                   timeout=120)
    r = np.load(dst)
    assert float(r["crowded_leaf"]) == on
    h = r["hits"]
    _check_closest("device hair, crowded", T, (h.view(np.int32)[:, 0].copy(), h[:, 1], h[:, 2], h[:, 3]))
    for k in (0, 1):
        _check_shadow("device hair, crowded", T, k, r[f"occ{k}"])


@pytest.mark.gpu
def test_device_camera_rays_vs_float64(gpu_device):
    T = _camera_truth(gpu_device.torch_device)
    gpu_device.upload(_scene("cornell")[0])
    hits = gpu_device.trace_closest(gpu_device.rays_to_device(T["rays"]))
    _check_closest("device camera", T, gpu_device.split_hits(hits))


@pytest.mark.gpu
def test_device_filtered_shadow_vs_float64(gpu_device):
    gpu_device.upload(_scene("panes")[0])

    def trace(rays, depth):
        occ, filt = gpu_device.trace_shadow_filtered(gpu_device.rays_to_device(rays), depth)
        return occ.cpu().numpy(), filt.cpu().numpy()

    _check_filtered("device", gpu_device.torch_device, GPU_RAYS, trace)
