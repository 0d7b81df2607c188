"""Mesh lights (meshlight.cc) on the GPU path.

CPU: yk_scene_add_mesh_light's accept / refuse table, round trips, and the host
state (triangle areas, cdf, area) against a numpy restatement of
meshLight_t::initIS / CumulateStep1dDF, bit for bit.
GPU: mesh_illum against a float32 restatement and mesh_hit against the oracle's
closest-hit query on the light's triangles as a scene of their own, bit for
bit with the triangle index; the direct-lighting film against a float32
restatement of doLightEstimation's sampled branch on the oracle's camera rays,
hits and isShadowed; a mixed frame against its single-light frames; path
tracing's image mean against the oracle's area light; a light that lights
nothing against the oracle's film of the scene without it; form invariance
under path tracing; the photon refusal, the light limit and two handles.

The oracle knows nothing of mesh lights and is never given a scene that holds
one. Like SURVEY row f1 the restatements are source order, unpinned against
the compiled reference.
"""
import ctypes as C

import numpy as np
import pytest

from core_amd import _abi as A
from core_amd.scene import Scene
from tests import mesh_light_common as M
from tests import raygen

F = np.float32
gpu = pytest.mark.gpu
PROBE_ILLUMINATE, PROBE_ILLUM_SAMPLE, PROBE_INTERSECT, PROBE_STRIDE = 0, 1, 2, 12
NAMES = ["one", "two_1_3", "zero_mid", "box", "sphere40", "sphere200", "two_mesh"]
COLOR, POWER = (1.0, 0.8, 0.6), 1.5


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _add(s, l, ids):
    ids = np.ascontiguousarray(ids, np.int32)
    return A.lib().yk_scene_add_mesh_light(s._p, None if l is None else C.byref(l), ids.ctypes.data_as(A.i32p),
                                           len(ids))


def _base():
    s = Scene()
    m = s.add_material(color=(0.5, 0.5, 0.5))
    a = s.add_mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 1, 2]], m)
    b = s.add_mesh([[0, 0, 1], [2, 0, 1], [0, 3, 1]], [[0, 1, 2]], m)
    s.set_camera((0, 0, 5), (0, 0, 0), (0, 1, 5), 8, 8)
    return s, m, a, b


# ------------------------------------------------------------------ CPU

def test_add_mesh_light_accepts_and_refuses():
    s, m, a, b = _base()
    v = s.add_mesh([[0, 0, 2], [1, 0, 2], [0, 1, 2]], [[0, 1, 2]], m)
    s.set_mesh_type(v, A.YK_MESH_VTRIM)
    inst = s.add_instance(a, np.eye(4))
    ok = A.yk_mesh_light(A.f3(1, 1, 1), 1.0, 4, 0)

    def lit(**kw):
        l = A.yk_mesh_light(A.f3(1, 1, 1), 1.0, 4, 0)
        for k, val in kw.items():
            setattr(l, k, val)
        return l
    inf, nan = float("inf"), float("nan")
    table = [
        (ok, [99], A.YK_ERR_ARG), (ok, [0], A.YK_ERR_ARG), (ok, [-1], A.YK_ERR_ARG),  # unknown ids
        (ok, [], A.YK_ERR_ARG),                                                      # empty list
        (ok, [a, b, a], A.YK_ERR_ARG),                                               # repeated id
        (lit(samples=0), [a], A.YK_ERR_ARG), (lit(samples=-3), [a], A.YK_ERR_ARG),
        (lit(color=A.f3(1, nan, 1)), [a], A.YK_ERR_ARG), (lit(color=A.f3(inf, 1, 1)), [a], A.YK_ERR_ARG),
        (lit(power=nan), [a], A.YK_ERR_ARG), (lit(power=-inf), [a], A.YK_ERR_ARG),
        (ok, [v], A.YK_ERR_UNSUPPORTED), (ok, [a, v], A.YK_ERR_UNSUPPORTED),        # VTRIM
        (ok, [inst], A.YK_ERR_UNSUPPORTED),                                          # instance id
        (None, [a], A.YK_ERR_ARG),
    ]
    for l, ids, want in table:
        assert _add(s, l, ids) == want, (ids, want)
        assert len(A.lib().yk_last_error()) > 0
        assert s.info().nlights == 0
    # yk_light cannot carry object ids: its entry point keeps refusing the kind
    old = A.yk_light(type=A.YK_LIGHT_MESH, color=A.f3(1, 1, 1), power=1.0, samples=4)
    assert A.lib().yk_scene_add_light(s._p, C.byref(old)) == A.YK_ERR_UNSUPPORTED
    assert s.info().nlights == 0
    assert _add(s, ok, [b, a]) == A.YK_OK and _add(s, lit(samples=1, double_sided=1), [a]) == A.YK_OK
    assert s.info().nlights == 2
    s.build()


def test_zero_area_and_retyped_targets_are_found_at_build():
    s, m, a, b = _base()
    z = s.add_mesh([[0, 0, 0], [1, 1, 1], [2, 2, 2]], [[0, 1, 2], [0, 0, 0]], m)  # collinear, degenerate
    s.add_mesh_light([z])
    with pytest.raises(A.YkError) as e:
        s.build()
    assert e.value.code == A.YK_ERR_ARG and "area" in str(e.value)
    t, m, a, b = _base()
    t.add_mesh_light([a])
    t.set_mesh_type(a, A.YK_MESH_VTRIM)
    with pytest.raises(A.YkError) as e:
        t.build()
    assert e.value.code == A.YK_ERR_UNSUPPORTED


def test_too_many_triangles_is_unsupported_not_truncated():
    s, m, a, b = _base()
    n = A.YK_MESH_LIGHT_MAX_TRIS + 1
    big = s.add_mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.tile(np.array([[0, 1, 2]], np.int32), (n, 1)), m)
    ok = A.yk_mesh_light(A.f3(1, 1, 1), 1.0, 4, 0)
    assert _add(s, ok, [big]) == A.YK_ERR_UNSUPPORTED and s.info().nlights == 0


def test_round_trip_and_mixed_scene_lights():
    s, m, a, b = _base()
    s.add_point_light((0, 0, 5), (1, 1, 1), 2.0)
    s.add_mesh_light([b, a], color=(0.25, 0.5, 1.0), power=3.0, samples=3, double_sided=True)
    s.add_area_light((0, 2, 0), (1, 2, 0), (0, 2, 1), samples=2)
    s.add_mesh_light(a)  # the factory's defaults
    assert [l.type for l in s.lights()] == [A.YK_LIGHT_POINT, A.YK_LIGHT_MESH, A.YK_LIGHT_AREA, A.YK_LIGHT_MESH]
    g = s.lights()[1]
    assert (tuple(g.color), g.power, g.samples) == ((0.25, 0.5, 1.0), 3.0, 3)
    l, ids = s.mesh_light(1)
    assert ids == [b, a] and (tuple(l.color), l.power, l.samples, l.double_sided) == ((0.25, 0.5, 1.0), 3.0, 3, 1)
    l, ids = s.mesh_light(3)
    assert ids == [a] and (tuple(l.color), l.power, l.samples, l.double_sided) == ((1.0, 1.0, 1.0), 1.0, 4, 0)
    n = C.c_int32()
    two = np.full(1, -7, np.int32)  # cap below the list's length: the length is still reported
    assert A.lib().yk_scene_get_mesh_light(s._p, 1, None, two.ctypes.data_as(A.i32p), 1, C.byref(n)) == A.YK_OK
    assert n.value == 2 and two[0] == b
    assert A.lib().yk_scene_get_mesh_light(s._p, 0, None, None, 0, C.byref(n)) == A.YK_ERR_STATE
    assert A.lib().yk_scene_get_mesh_light(s._p, 9, None, None, 0, C.byref(n)) == A.YK_ERR_ARG
    s.build()
    st = s.light_states()
    assert [type(x).__name__ for x in st] == ["yk_dirac_light_state", "yk_mesh_light_state", "yk_area_light_state",
                                              "yk_mesh_light_state"]
    assert (_bits(st[1].color[:]) == _bits(M.stored_color((0.25, 0.5, 1.0), 3.0))).all()
    assert st[1].samples == 3 and st[1].double_sided == 1 and st[1].ntris == 2 and st[3].ntris == 1
    # the stored colour as a plugin reads it from a live object
    rgb = np.array([0.1, 7.5, 3.25], F)
    assert A.lib().yk_scene_set_mesh_light_color(s._p, 3, rgb.ctypes.data_as(A.fp)) == A.YK_OK
    assert A.lib().yk_scene_set_mesh_light_color(s._p, 0, rgb.ctypes.data_as(A.fp)) == A.YK_ERR_STATE
    assert (_bits(s.light_states()[3].color[:]) == _bits(rgb)).all()


def test_yk_light_layout_is_unchanged():
    assert C.sizeof(A.yk_light) == 124
    assert [getattr(A.yk_light, f).offset for f in ("type", "corner", "color", "power", "samples", "from_", "to",
                                                    "photon_only")] == [0, 4, 40, 52, 56, 60, 92, 120]


def _scene_of_lists(double_sided):
    """every light list of light_meshes() as one mesh light of a scene, in NAMES order"""
    s = Scene()
    m = s.add_material(type_=1, color=(1, 1, 1), power=1.0)
    f = s.add_material(color=(0.5, 0.5, 0.5))
    s.add_mesh(np.array([(-2, 0, -2), (-2, 0, 2), (2, 0, 2), (2, 0, -2)], F), [[0, 1, 2], [0, 2, 3]], f)
    lists = M.light_meshes()
    for name in NAMES:
        ids = [s.add_mesh(p, fc, m) for p, fc in lists[name]]
        s.add_mesh_light(ids, color=COLOR, power=POWER, samples=2, double_sided=double_sided)
    s.set_camera((0, 1, -5), (0, 1, 0), (0, 2, -5), 8, 8)
    s.build()
    return s, lists


def test_host_state_equals_initis_restatement():
    s, lists = _scene_of_lists(False)
    for li, name in enumerate(NAMES):
        tv = M.tri_list(lists[name])
        areas, cdf, area, inv_area = M.init_is(tv)
        st, gcdf, gareas = s.mesh_light_state(li)
        assert st.ntris == len(tv), name
        assert (_bits(gareas) == _bits(areas)).all(), name
        assert (_bits(gcdf) == _bits(cdf)).all(), name
        assert _bits(st.area) == _bits(area) and _bits(st.inv_area) == _bits(inv_area), name
        assert gcdf[0] == 0 and gcdf[-1] == 1 and (np.diff(gcdf) >= 0).all()
        assert st.tree_nodes >= 1 and st.tree_depth <= A.YK_MESH_LIGHT_MAX_DEPTH
    assert M.init_is(M.tri_list(lists["two_1_3"]))[1].tolist() == [0.0, 0.25, 1.0]
    z = M.init_is(M.tri_list(lists["zero_mid"]))
    assert z[0][1] == 0 and z[1][1] == z[1][2]  # the zero-area triangle's interval is empty


# ------------------------------------------------------------------ GPU

def _light_probe(dev, light, fn, inp):
    f = A.lib().yk_debug_light_probe  # a test hook: bound here, not in the product ABI table
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int32, C.c_int32, A.fp, C.c_int64, A.fp]
    inp = np.ascontiguousarray(inp, F)
    out = np.full((len(inp), PROBE_STRIDE), np.nan, F)
    A.check(f(dev._p, light, fn, inp.ctypes.data_as(A.fp), len(inp), out.ctypes.data_as(A.fp)))
    return out


def _same(got, want, what):
    bad = np.flatnonzero((_bits(got) != _bits(want)).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} of {len(got)} rows differ; first {bad[0]}: got {got[bad[0]]} want {want[bad[0]]}"


def _illum_inputs(tv, cdf, rng):
    """P, s1, s2 rows: random points, the cdf's interior entries and their
    neighbours, s1 = 0 and just below 1, points behind / in the plane of / on
    the sampled point"""
    n = 96
    P = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(0.0, 3.5, n), rng.uniform(-1.5, 1.5, n)], 1).astype(F)
    s = rng.random((n, 2)).astype(F)
    edge = [F(0.0), np.nextafter(F(1.0), F(0.0)), np.nextafter(F(0.0), F(1.0))]
    for c in cdf[1:-1]:
        edge += [c, np.nextafter(c, F(0.0)), np.nextafter(c, F(2.0))]
    edge = np.array(edge, F)
    Pe = np.tile(np.array([[0.2, 0.5, -0.1], [0.1, 3.0, 0.3]], F), (len(edge), 1))
    se = np.stack([np.repeat(edge, 2), np.tile(np.array([0.3, 0.9], F), len(edge))], 1)
    X = np.concatenate([np.concatenate([P, s], 1), np.concatenate([Pe, se], 1)]).astype(F)
    # the sampled point itself (dist == 0), and points in the triangle's plane
    k = 24
    sk = rng.random((k, 2)).astype(F)
    prim, p = M.sample_point(tv, cdf, sk[:, 0], sk[:, 1])
    on = np.concatenate([p, sk], 1)
    a = tv[prim, 0:3]
    inplane = np.concatenate([(a + (a - p)).astype(F), sk], 1)
    return np.concatenate([X, on, inplane]).astype(F)


@gpu
@pytest.mark.parametrize("double_sided", [False, True], ids=["single", "double"])
def test_mesh_illum_equals_float32_restatement(gpu_device, monkeypatch, double_sided):
    monkeypatch.setenv("YK_DEBUG_HOOKS", "1")
    s, lists = _scene_of_lists(double_sided)
    gpu_device.upload(s)
    col = M.stored_color(COLOR, POWER)
    rng = np.random.default_rng(11)
    refused = 0
    for li, name in enumerate(NAMES):
        tv = M.tri_list(lists[name])
        _, cdf, area, _ = M.init_is(tv)
        X = _illum_inputs(tv, cdf, rng)
        want = M.mesh_illum(tv, cdf, area, M.normals(tv), col, double_sided, X)
        got = _light_probe(gpu_device, li, PROBE_ILLUM_SAMPLE, X)
        _same(got, want, f"mesh_illum {name}")
        refused += int((want[:, 0] == 0).sum())
        assert (want[:, 0] == 1).sum() > 20, name
        out = _light_probe(gpu_device, li, PROBE_ILLUMINATE, X[:4, :3])
        assert (out == 0).all()  # meshLight_t::illuminate returns false
    assert refused > 0


def _hit_rays(tv, bound, seed):
    """random rays, rays at triangle edges and vertices (shared ones on the
    closed meshes), grazing rays, and origins on the surface"""
    rng = np.random.default_rng(seed)
    r1 = raygen.random_rays(bound, 600, seed)
    r2 = raygen.graze_rays(tv, bound, 300, seed + 1)
    k = 150
    t = tv[rng.integers(len(tv), size=k)].reshape(k, 3, 3)
    lo, hi = np.asarray(bound[:3], F), np.asarray(bound[3:], F)
    o = (lo + (hi - lo) * rng.random((k, 3))).astype(F)
    vert = t[np.arange(k), rng.integers(3, size=k)]
    r3 = np.zeros((k, 8), F)
    r3[:, 0:3], r3[:, 3:6] = o, vert - o
    b = rng.dirichlet((1, 1, 1), k).astype(F)
    on = (b[:, 0, None] * t[:, 0] + b[:, 1, None] * t[:, 1] + b[:, 2, None] * t[:, 2]).astype(F)
    r4 = np.zeros((k, 8), F)
    r4[:, 0:3] = on
    r4[:, 3:6] = rng.normal(size=(k, 3))
    rays = np.concatenate([r1, r2, r3, r4]).astype(F)
    nd = np.linalg.norm(rays[:, 3:6], axis=1, keepdims=True).astype(F)
    rays[:, 3:6] = np.where(nd > 0, rays[:, 3:6] / np.maximum(nd, F(1e-30)), F([0, 1, 0]))
    rays[:, 6] = M.MIN_RAYDIST  # bRay.tmin (mcintegrator.cc:165)
    rays[:, 7] = -1.0           # ray_t's default tmax: unbounded
    return rays


@gpu
@pytest.mark.parametrize("double_sided", [False, True], ids=["single", "double"])
def test_mesh_hit_equals_oracle_closest_hit(gpu_device, monkeypatch, double_sided):
    from oracle.oracle import Oracle
    monkeypatch.setenv("YK_DEBUG_HOOKS", "1")
    s, lists = _scene_of_lists(double_sided)
    gpu_device.upload(s)
    col = M.stored_color(COLOR, POWER)
    back = 0
    for li, name in enumerate(NAMES):
        tv = M.tri_list(lists[name])
        alone = M.triangles_scene(tv)
        orc = Oracle(alone)
        e = alone.export()
        assert (_bits(e["tri_verts"]) == _bits(tv)).all()
        if name == "sphere200":
            assert alone.info().leaves > 8  # a multi-leaf tree
        rays = _hit_rays(tv, e["bound"], 100 + li)
        prim, t = orc.intersect(rays)[:2]
        _, _, area, _ = M.init_is(tv)
        want = M.mesh_hit_tail(prim, t.astype(F), rays[:, 3:6], e["tri_normal"].astype(F), area, col, double_sided)
        got = _light_probe(gpu_device, li, PROBE_INTERSECT, rays[:, :6])
        _same(got, want, f"mesh_hit {name}")
        assert (prim >= 0).sum() > 50 and (prim < 0).sum() > 50, name
        back += int(((prim >= 0) & (want[:, 0] == 0)).sum())
    assert double_sided or back > 0  # single-sided back hits were among the rays


def _params(integ, res, spp, **over):
    p = A.yk_render_params()
    A.lib().yk_render_params_default(C.byref(p))
    p.integrator = integ
    p.width = p.height = res
    p.aa_samples = spp
    p.tile_size = 16
    p.filter = A.YK_FILTER_BOX
    p.aa_pixelwidth = 1.0
    p.raydepth = 2
    p.caustic_type = A.YK_CAUSTIC_NONE
    p.path_samples = 1
    p.bounces = 3
    for k, v in over.items():
        setattr(p, k, v)
    return p


def _render(dev, s, q, shard=0, nshards=1):
    dev.upload(s)
    film = dev.new_film(q)
    st = dev.render_shard(q, film, shard, nshards)
    return film.cpu().numpy(), st


@gpu
def test_mesh_light_that_lights_nothing_equals_no_light_direct(gpu_device):
    """A single-sided quad facing up, above all geometry: illumSample refuses
    every sample (cos <= 0) and intersect every BSDF ray (no geometry looks at
    its front), so direct lighting adds nothing and traces no shadow ray."""
    from oracle.oracle import Oracle
    up = (np.array([[-0.4, 2, -0.4], [0.4, 2, -0.4], [0.4, 2, 0.4], [-0.4, 2, 0.4]], F), np.array([[0, 2, 1], [0, 3, 2]], np.int32))
    lit = M.lit_scene(32, [up], samples=3)
    plain = M.lit_scene(32, [up], add_light=False)
    q = _params(A.YK_INTEGRATOR_DIRECT, 32, 2)
    _, sums_o, cnt = Oracle(plain).render(q)
    film, st = _render(gpu_device, lit, q)
    assert (st.closest_rays, st.shadow_rays) == (cnt["closest"], cnt["shadow"]) and st.shadow_rays == 0
    assert (film.view(np.uint32) == sums_o.view(np.uint32)).all()


@gpu
def test_mesh_light_that_lights_nothing_equals_dark_light_path(gpu_device):
    """Path tracing picks one light per vertex and scales by their number, so
    the yardstick is the oracle's frame with a light it knows that gives
    nothing either in the mesh light's place (a finite directional light
    whose cylinder misses the scene). The quad hangs under the floor and
    faces down, so no ray reaches it: a bounce hit on the light's own mesh
    would lie in its plane, where illumSample's cosine is rounding noise."""
    from oracle.oracle import Oracle
    up = (np.array([[-0.4, -1, -0.4], [0.4, -1, -0.4], [0.4, -1, 0.4], [-0.4, -1, 0.4]], F), np.array([[0, 1, 2], [0, 2, 3]], np.int32))
    lit = M.lit_scene(32, [up], samples=2)
    s = Scene()
    M.add_floor_and_occluder(s)
    lm = s.add_material(type_=1, color=(1.0, 0.9, 0.8), power=2.0)
    s.add_mesh(up[0], up[1], lm)
    s.add_directional_light((0, 0, -1), (1, 1, 1), 5.0, infinite=False, from_=(50, 50, 50), radius=0.01)
    s.set_camera((0.3, 2.6, -4.5), (0, 0.6, 0), (0.3, 3.6, -4.5), 32, 32, focal=1.4)
    s.build()
    q = _params(A.YK_INTEGRATOR_PATH, 32, 2)
    _, sums_o, cnt = Oracle(s).render(q)
    film, st = _render(gpu_device, lit, q)
    assert (st.closest_rays, st.shadow_rays) == (cnt["closest"], cnt["shadow"]) and st.closest_rays > 32 * 32 * 2
    assert (film.view(np.uint32) == sums_o.view(np.uint32)).all()


# (environment, expected split form or None, expected "traversal data in LDS" or None), checked
# through yk_debug_shadow_form / yk_debug_small_scene: full, split and split_hbm slot forms
FORMS = [(dict(), None, None), (dict(YK_MERGE="0"), None, None), (dict(YK_SPLIT="0"), 0, None),
         (dict(YK_SPLIT="1"), 1, True), (dict(YK_SPLIT="1", YK_SMALL="0"), 1, False),
         (dict(YK_PIPES="1"), None, None), (dict(YK_PIPES="4"), None, None), (dict(YK_DIFF="0"), None, None),
         (dict(YK_SMALL="0"), None, False)]
FORM_KEYS = ("YK_MERGE", "YK_SPLIT", "YK_PIPES", "YK_DIFF", "YK_SMALL")
# transparent shadows have no split form (shadow_split() is false): their YK_SPLIT rows could not differ
FORM_CASES = [(f, 0) for f in range(len(FORMS))] + [(f, 1) for f in range(len(FORMS)) if "YK_SPLIT" not in FORMS[f][0]]


def _form_scene(ts):
    s = M.lit_scene(24, [M.light_meshes()["box"][0]], pane=bool(ts), color=(1.0, 0.9, 0.7), power=3.0, samples=2,
                    double_sided=True)
    return s, _params(A.YK_INTEGRATOR_PATH, 24, 2, transp_shadows=ts, tile_size=8)


@pytest.fixture(scope="module")
def form_reference(gpu_device):
    """Per shadow kind the film and ray counts with the environment unset,
    checked to be lit and to equal two shards summed."""
    import os
    saved = {k: os.environ.pop(k) for k in FORM_KEYS if k in os.environ}
    ref = {}
    try:
        for ts in (0, 1):
            s, q = _form_scene(ts)
            film, st = _render(gpu_device, s, q)
            assert np.isfinite(film).all() and film[..., :3].max() > 0 and st.shadow_rays > 0
            acc = None
            for i in range(2):
                f, _ = _render(gpu_device, s, q, i, 2)
                acc = f.copy() if acc is None else acc + f
            assert (acc.view(np.uint32) == film.view(np.uint32)).all(), "two shards differ from one"
            ref[ts] = (film, (st.closest_rays, st.shadow_rays))
    finally:
        os.environ.update(saved)
    return ref


@gpu
@pytest.mark.parametrize("form,ts", FORM_CASES,
                         ids=[("-".join(f"{k}{v}" for k, v in FORMS[f][0].items()) or "default") + ("-ts" if t else "")
                              for f, t in FORM_CASES])
def test_path_tracing_form_invariance(gpu_device, monkeypatch, form_reference, form, ts):
    """3 bounces, 2 spp under a double-sided box mesh light (and, with
    transparent shadows, a filtering pane between light and floor): the same
    film bits and ray counts whatever the shadow-launch and slot form (full,
    split, split read from HBM: confirmed through the form hooks), the pipe
    count, the material instantiation and the traversal variant."""
    monkeypatch.setenv("YK_DEBUG_HOOKS", "1")
    s, q = _form_scene(ts)
    env, want_split, want_small = FORMS[form]
    for k in FORM_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    film, st = _render(gpu_device, s, q)
    split, small = C.c_int32(-1), C.c_int64(-1)
    A.check(A.lib().yk_debug_shadow_form(gpu_device._p, C.byref(q), C.byref(split)))
    A.check(A.lib().yk_debug_small_scene(gpu_device._p, C.byref(small)))
    if ts:
        assert split.value == 0
    elif want_split is not None:
        assert split.value == want_split
    if want_small is not None:
        assert (small.value > 0) == want_small
    assert (st.closest_rays, st.shadow_rays) == form_reference[ts][1]
    assert (film.view(np.uint32) == form_reference[ts][0].view(np.uint32)).all()


# ---- films ------------------------------------------------------------------

def _dl_cases():
    quad = M.light_meshes()["two_mesh"][:1]
    box = [M.light_meshes()["box"][0]]
    return [("quad", quad, False), ("box", box, True)]


@gpu
@pytest.mark.parametrize("spp", [1, 2])
@pytest.mark.parametrize("samples", [1, 3])
@pytest.mark.parametrize("kind", ["quad", "box"])
def test_direct_lighting_film_equals_restatement(gpu_device, kind, samples, spp):
    """A Lambert floor and occluder under a single-sided quad / a double-sided
    box mesh light whose mesh carries a light_mat: the film against the
    float32 restatement of doLightEstimation's sampled branch on the oracle's
    camera rays, hits and isShadowed (the scene handed to the oracle holds
    the same geometry and materials and no light), bit for bit, ray counts
    included."""
    from oracle.oracle import Oracle
    from tests.dl_common import film_of
    meshes, ds = {k: (m, d) for k, m, d in _dl_cases()}[kind]
    col, power = (1.0, 0.9, 0.8), 3.0
    lit = M.lit_scene(24, meshes, color=col, power=power, samples=samples, double_sided=ds)
    plain = M.lit_scene(24, meshes, add_light=False)
    q = _params(A.YK_INTEGRATOR_DIRECT, 24, spp, tile_size=8)
    r = M.restate_direct_mesh(Oracle(plain), plain, q, M.tri_list(meshes), M.stored_color(col, power), samples, ds)
    film, st = _render(gpu_device, lit, q)
    want = film_of(r["col"], q)
    assert r["diffuse_hits"] > 100 and (want.sum(-1) > 0).sum() > 100
    assert st.shadow_rays == r["shadow_rays"] and st.closest_rays == 24 * 24 * spp
    bad = (film[..., :3].view(np.uint32) != want.view(np.uint32)).any(-1)
    assert not bad.any(), f"{bad.sum()} pixels differ; first {np.argwhere(bad)[0]}: {film[..., :3][bad][0]} vs {want[bad][0]}"


# Path tracing against the oracle's parallelogram area light on the same
# emitting quad, 16 x 16, 3 bounces, 16 spp. The yardstick's own noise: the
# oracle's per-channel image mean at 16 spp against its mean at 64 spp; three
# times that difference is allowed (the mesh light estimates the same
# integrand with other sample positions).
ORACLE_AREA_MEAN_16 = np.array([0.08262815481703001, 0.0695928718905634, 0.05910532987854822])
ORACLE_AREA_MEAN_64 = np.array([0.08250194110041775, 0.0694463714135054, 0.05891874810367881])
PT_MEAN_TOL = 3.0 * np.abs(ORACLE_AREA_MEAN_16 - ORACLE_AREA_MEAN_64)  # 3.79e-4, 4.40e-4, 5.60e-4


@gpu
def test_path_tracing_mean_matches_the_area_light(gpu_device):
    from oracle.oracle import Oracle
    col, power = (1.0, 0.9, 0.8), 3.0
    q = _params(A.YK_INTEGRATOR_PATH, 16, 16)
    area = M.lit_scene(16, None, add_light="area", color=col, power=power, samples=2)
    _, sums_o, _ = Oracle(area).render(q)
    mean_o = sums_o[..., :3].reshape(-1, 3).astype(np.float64).mean(0) / 16
    assert np.allclose(mean_o, ORACLE_AREA_MEAN_16, rtol=0, atol=1e-9)  # the constants are this scene's
    mesh = M.lit_scene(16, None, color=col, power=power, samples=2)
    film, _ = _render(gpu_device, mesh, q)
    mean_g = film[..., :3].reshape(-1, 3).astype(np.float64).mean(0) / 16
    print("mesh light mean", mean_g, "area light mean", mean_o, "difference", mean_g - mean_o, "allowed", PT_MEAN_TOL)
    assert (np.abs(mean_g - mean_o) <= PT_MEAN_TOL).all()


def _mixed(which, res=20):
    """floor + occluder; lights by name, in the order given: an area light (4
    samples, 8 slots), a point light (1), mesh light A (a quad, 16 samples,
    32 slots: slots 9-40) and mesh light B (a box, 14 samples, 28 slots:
    slots 41-68, across the 64-bit traced mask)"""
    s = Scene()
    M.add_floor_and_occluder(s)
    lm = s.add_material(type_=1, color=(1.0, 0.9, 0.8), power=1.0)
    qa = M.light_meshes()["two_mesh"][0]
    ida = s.add_mesh(qa[0] + F([-0.8, 0, 0.3]), qa[1], lm)
    bx = M.light_meshes()["box"][0]
    idb = s.add_mesh(bx[0] + F([0.9, -0.3, -0.4]), bx[1], lm)
    for name in which:  # in the order given: a light's index enters its Halton offset (l_offs)
        if name == "area":
            s.add_area_light((-0.3, 2.4, -0.3), (0.3, 2.4, -0.3), (-0.3, 2.4, 0.3), (0.9, 1.0, 0.8), 2.0, samples=4)
        elif name == "point":
            s.add_point_light((1.2, 1.5, -1.0), (1.0, 0.8, 0.7), 3.0)
        elif name == "a":
            s.add_mesh_light(ida, color=(0.7, 0.9, 1.0), power=2.0, samples=16)
        elif name == "b":
            s.add_mesh_light(idb, color=(1.0, 0.6, 0.5), power=1.5, samples=14, double_sided=True)
        else:  # "dark": a finite directional light whose cylinder misses the scene: one empty slot, no ray, +0
            s.add_directional_light((0, 0, -1), (1, 1, 1), 5.0, infinite=False, from_=(50, 50, 50), radius=0.01)
    s.set_camera((0.3, 2.6, -4.5), (0, 0.6, 0), (0.3, 3.6, -4.5), res, res, focal=1.4)
    s.build()
    return s


@gpu
def test_mixed_lights_own_their_slots_and_add_up(gpu_device):
    """Direct lighting at one sample per pixel sums the lights in order from
    0, ((0 + a) + p) + A) + B, and a pixel's film value is that one sample: at
    pixels whose camera hit is diffuse (no emission term) the mixed film is
    the single-light films added in light order, bit for bit, and the shadow
    rays are the single-light frames' added up. Each single-light scene keeps
    the light at its index (dark lights that give nothing stand before it:
    the index enters the light's Halton offset). The area and point frames
    come from the oracle. 69 slots per shading point: mesh light B's lie on
    both sides of the 64-bit traced mask."""
    from oracle.oracle import Oracle
    names = ["area", "point", "a", "b"]
    q = _params(A.YK_INTEGRATOR_DIRECT, 20, 1, tile_size=10)
    mixed = _mixed(names)
    assert [l.type for l in mixed.lights()] == [A.YK_LIGHT_AREA, A.YK_LIGHT_POINT, A.YK_LIGHT_MESH, A.YK_LIGHT_MESH]
    film, st = _render(gpu_device, mixed, q)
    acc, rays = np.zeros((20, 20, 3), F), 0
    for n in names:
        # the light alone at its index of the mixed scene, dark lights before it
        single = _mixed(["dark"] * names.index(n) + [n])
        if n in ("area", "point"):
            _, f, cnt = Oracle(single).render(q)
            nr = cnt["shadow"]
        else:
            f, s1 = _render(gpu_device, single, q)
            nr = s1.shadow_rays
        assert nr > 0 and f[..., :3].max() > 0, n
        acc = (acc + f[..., :3]).astype(F)
        rays += nr
    plain = Oracle(_mixed([]))
    prim = plain.intersect(plain.camera_rays(0, 0, 20, 20, 1))[0]
    ms = mixed.material_states()
    diffuse = np.array([p >= 0 and ms[plain.arrays["tri_material"][p]].type == 0 for p in prim], bool).reshape(20, 20)
    assert diffuse.sum() > 150
    assert st.shadow_rays == rays and st.shadow_rays <= 69 * diffuse.sum()
    assert (film[..., :3].view(np.uint32) == acc.view(np.uint32))[diffuse].all()


@gpu
def test_upload_refuses_more_than_eight_lights(gpu_device):
    s = Scene()
    M.add_floor_and_occluder(s)
    lm = s.add_material(type_=1, color=(1, 1, 1), power=1.0)
    q = M.light_meshes()["one"][0]
    for k in range(9):
        s.add_mesh_light(s.add_mesh(q[0] + F([0.1 * k, 0, 0]), q[1], lm), samples=1)
    s.set_camera((0.3, 2.6, -4.5), (0, 0.6, 0), (0.3, 3.6, -4.5), 8, 8)
    s.build()
    with pytest.raises(A.YkError) as e:
        gpu_device.upload(s)
    assert e.value.code == A.YK_ERR_UNSUPPORTED and "lights" in str(e.value)


@gpu
def test_direct_lighting_with_ao_and_specular_recursion_run(gpu_device):
    """The AO and specular-recursion instantiations with a mesh light present:
    finite, lit frames, and the mirror sees the lit floor."""
    s = Scene()
    M.add_floor_and_occluder(s)
    lm = s.add_material(type_=1, color=(1.0, 0.9, 0.8), power=2.0)
    mir = s.add_material(color=(1, 1, 1), diffuse_reflect=0.2, specular_reflect=0.8, mirror_color=(0.9, 0.9, 0.8))
    quad = M.light_meshes()["two_mesh"][0]
    lid = s.add_mesh(quad[0], quad[1], lm)
    s.add_mesh(np.array([(-1.5, 0, 1.5), (1.5, 0, 1.5), (1.5, 2, 1.5), (-1.5, 2, 1.5)], F), [[0, 1, 2], [0, 2, 3]], mir)
    s.add_mesh_light(lid, power=4.0, samples=2)
    s.set_camera((0.3, 2.6, -4.5), (0, 0.6, 0), (0.3, 3.6, -4.5), 24, 24, focal=1.4)
    s.build()
    plain = _render(gpu_device, s, _params(A.YK_INTEGRATOR_DIRECT, 24, 1, raydepth=3))[0]
    ao = _render(gpu_device, s, _params(A.YK_INTEGRATOR_DIRECT, 24, 1, raydepth=3, do_ao=1, ao_samples=4))[0]
    for f in (plain, ao):
        assert np.isfinite(f).all() and f[..., :3].max() > 0
    assert (ao[..., :3] >= plain[..., :3]).all() and (ao[..., :3] > plain[..., :3]).any()


@gpu
def test_photon_build_refuses_a_mesh_light_and_two_handles_keep_their_tables(gpu_device, monkeypatch):
    from core_amd.device import Device
    monkeypatch.setenv("YK_DEBUG_HOOKS", "1")
    a = M.lit_scene(16, None, samples=2)
    gpu_device.upload(a)
    for integ, caustic, dlc in ((A.YK_INTEGRATOR_PHOTON, A.YK_CAUSTIC_NONE, 0), (A.YK_INTEGRATOR_PATH, A.YK_CAUSTIC_PHOTON, 0),
                                (A.YK_INTEGRATOR_DIRECT, A.YK_CAUSTIC_NONE, 1)):
        q = _params(integ, 16, 1, caustic_type=caustic, dl_caustics=dlc)
        q.photon.photons = q.photon.caustic_photons = 2000
        with pytest.raises(A.YkError) as e:
            gpu_device.photon_build(q)
        assert e.value.code == A.YK_ERR_UNSUPPORTED and "mesh light" in str(e.value)
    b = M.lit_scene(16, [M.light_meshes()["sphere40"][0]], samples=2, double_sided=True)
    X = np.array([[0.1, 0.2, 0.0, 0.37, 0.61], [0.5, 0.1, -0.4, 0.93, 0.05]], F)
    d2 = Device(0)
    try:
        d2.upload(b)
        ra, rb = _light_probe(gpu_device, 0, PROBE_ILLUM_SAMPLE, X), _light_probe(d2, 0, PROBE_ILLUM_SAMPLE, X)
        ra2 = _light_probe(gpu_device, 0, PROBE_ILLUM_SAMPLE, X)
    finally:
        d2.close()
    col = M.stored_color((1, 1, 1), 1.0)
    for got, meshes, ds in ((ra, M.light_meshes()["two_mesh"][:1], False), (rb, [M.light_meshes()["sphere40"][0]], True),
                            (ra2, M.light_meshes()["two_mesh"][:1], False)):
        tv = M.tri_list(meshes)
        _, cdf, area, _ = M.init_is(tv)
        _same(got, M.mesh_illum(tv, cdf, area, M.normals(tv), col, ds, X), "two handles")
