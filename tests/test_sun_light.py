"""The sun light (sunLight_t, sunlight.cc): ABI and constructor state on the
CPU; on the GPU its illumSample / intersect / emitPhoton against the float32
restatement of tests/sun_common.py, direct-lighting films against the
restatement of doLightEstimation on the oracle's camera hits and isShadowed,
a sun that lights nothing against the oracle, form invariance, photon
emission and maps, and a plain scene after a sun scene on one handle.

The oracle has no sun: parity is source order, unpinned against a compiled
reference build.
"""
import ctypes as C
import os

import numpy as np
import pytest

from core_amd import _abi as A
from core_amd.scene import Scene
from tests import sun_common as S

gpu = pytest.mark.gpu
F = np.float32
RES = 32
PROBE_ILLUMINATE, PROBE_ILLUM_SAMPLE, PROBE_INTERSECT, PROBE_EMIT_PHOTON = 0, 1, 2, 3
PROBE_STRIDE = 12


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _sun(direction=(0.0, 0.0, 1.0), color=(1.0, 1.0, 1.0), power=1.0, angle=0.27, samples=4):
    return A.yk_light(type=A.YK_LIGHT_SUN, color=A.f3(*color), power=power, samples=samples,
                      direction=A.f3(*direction), cone_angle=angle)


# ------------------------------------------------------------------ CPU

def test_constant_and_struct_size():
    assert A.YK_LIGHT_SUN == 6
    assert C.sizeof(A.yk_light) == 124  # the sun reuses cone_angle: the struct does not grow


def test_accepted_and_refused_parameters():
    s = Scene()
    bad = [_sun(direction=(0, 0, 0)), _sun(direction=(np.nan, 0, 1)), _sun(direction=(0, np.inf, 1)),
           _sun(color=(1, np.nan, 1)), _sun(color=(np.inf, 1, 1)), _sun(power=np.inf), _sun(power=np.nan),
           _sun(angle=0.0), _sun(angle=-1.0), _sun(angle=np.nan), _sun(angle=np.inf), _sun(samples=0),
           _sun(samples=-3)]
    for l in bad:
        rc = A.lib().yk_scene_add_light(s._p, C.byref(l))
        assert rc == A.YK_ERR_ARG and "sun light" in A.lib().yk_last_error().decode()
        assert s.info().nlights == 0
    for l in (_sun(), _sun(angle=120.0), _sun(direction=(3, -4, 12), samples=1), _sun(angle=1e-3), _sun(power=0.0)):
        assert A.lib().yk_scene_add_light(s._p, C.byref(l)) == A.YK_OK
    assert s.info().nlights == 5
    b = S.state_struct(S.sun_state((0, 0, 1)))
    b.samples = 0
    assert A.lib().yk_scene_add_sun_light_state(s._p, C.byref(b)) == A.YK_ERR_ARG
    assert s.info().nlights == 5


def test_parameters_and_state_round_trip_and_info_counts():
    s = Scene()
    s.add_sun_light((0.3, 0.5, -1.0), (1.0, 0.9, 0.8), 2.5, angle=3.0, samples=3)
    s.add_point_light((0, 1, 0))
    st0 = S.sun_state((0, 1, 0.2), (0.5, 0.6, 0.7), 4.0, 12.0, 2)
    s.add_sun_light_state(S.state_struct(st0))
    assert s.info().nlights == 3
    l = A.yk_light()
    A.check(A.lib().yk_scene_get_light(s._p, 0, C.byref(l)))
    assert A.lib().yk_scene_get_light(s._p, 2, C.byref(l.__class__())) == A.YK_ERR_STATE  # given as state only
    assert l.type == A.YK_LIGHT_SUN and tuple(l.direction) == tuple(F([0.3, 0.5, -1.0]))
    assert tuple(l.color) == tuple(F([1.0, 0.9, 0.8])) and l.power == F(2.5) and l.cone_angle == 3.0 and l.samples == 3
    states = s.light_states()
    assert [type(x) for x in states] == [A.yk_sun_light_state, A.yk_dirac_light_state, A.yk_sun_light_state]
    assert S.same_state(S.struct_state(states[2]), st0)
    assert S.same_state(S.struct_state(states[0]), S.sun_state((0.3, 0.5, -1.0), (1.0, 0.9, 0.8), 2.5, 3.0, 3))
    out = A.yk_sun_light_state()
    assert A.lib().yk_scene_get_sun_light_state(s._p, 1, C.byref(out)) == A.YK_ERR_STATE
    assert A.lib().yk_scene_get_sun_light_state(s._p, 3, C.byref(out)) == A.YK_ERR_ARG


DIRECTIONS = [(0, 0, 1), (0, 0, -1), (1, 0, 0), (0, -1, 0), (0.3, 0.5, -1.0), (-0.6, 0.2, 0.77), (3, -4, 12),
              (0.01, 0.02, -0.005), (0, 0, 5)]


@pytest.mark.parametrize("angle", [0.01, 0.27, 5.0, 80.0, 120.0])
def test_constructor_state_equals_the_restatement(angle):
    s = Scene()
    for d in DIRECTIONS:
        s.add_sun_light(d, (1.0, 0.9, 0.8), 2.5, angle=angle, samples=2)
    for d, got in zip(DIRECTIONS, s.light_states()):
        want = S.sun_state(d, (1.0, 0.9, 0.8), 2.5, angle, 2)
        assert S.same_state(S.struct_state(got), want), (d, S.struct_state(got), want)
    if angle == 120.0:  # clamped to 80
        assert S.struct_state(s.light_states()[0])["cos_angle"] == S.sun_state((0, 0, 1), angle=80.0)["cos_angle"]
    # createCS takes the un-normalized argument: du and dv are not those of the normalized direction
    a, b = S.sun_state((3, -4, 12), angle=angle), S.sun_state(tuple(F([3, -4, 12]) / F(13)), angle=angle)
    assert np.allclose(a["direction"], b["direction"], atol=1e-6)
    assert abs(np.linalg.norm(a["dv"]) - 13.0) < 1e-4 and abs(np.linalg.norm(b["dv"]) - 1.0) < 1e-5
    st = S.struct_state(s.light_states()[6])
    assert _bits(st["dv"]).tolist() == _bits(a["dv"]).tolist()
    # a direction along z: createCS's axis branch, du = (+-1, 0, 0) and dv = (0, 1, 0) whatever its length
    z = S.struct_state(s.light_states()[8])
    assert z["du"].tolist() == [1, 0, 0] and z["dv"].tolist() == [0, 1, 0] and z["direction"].tolist() == [0, 0, 1]


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


def _no_light_cornell(gen, res=RES):
    """The Cornell probe without its area light (the emitting quad stays a
    mesh), rebuilt from its parameters and triangles: the scene's lights are the test's."""
    src = Scene()
    p = src.generate(gen, res, res)
    src.build()
    e = src.export()
    t = Scene()
    for m in src.materials():  # parameter-level, as the oracle reads them
        A.check(A.lib().yk_scene_add_material(t._p, C.byref(m), None))
    tv, tm = e["tri_verts"], e["tri_material"]
    start = 0
    while start < len(tm):
        end = start
        while end < len(tm) and tm[end] == tm[start]:
            end += 1
        pts = tv[start:end].reshape(-1, 3)
        t.add_mesh(pts, np.arange(len(pts), dtype=np.int32).reshape(-1, 3), int(tm[start]))
        start = end
    cam = src.camera()
    A.check(A.lib().yk_scene_set_camera(t._p, C.byref(cam)))
    return t, p


def _cornell(gen, add=None, res=RES):
    s, p = _no_light_cornell(gen, res)
    if add:
        add(s)
    s.build()
    return s, p


def _params(p, integ, spp, **over):
    q = p.copy()
    q.integrator = integ
    q.width = q.height = RES
    q.aa_samples = spp
    q.tile_size = 16
    q.filter = A.YK_FILTER_BOX
    q.aa_pixelwidth = 1.0
    q.caustic_type = A.YK_CAUSTIC_NONE
    q.path_samples = 1
    q.bounces = 3
    for k, v in over.items():
        setattr(q, k, v)
    return q


def _render(dev, s, q, shard=0, nshards=1):
    dev.upload(s)
    film = dev.new_film(q)
    st = dev.render_shard(q, film, shard, nshards)
    return film.cpu().numpy(), st


SUNS = [dict(direction=(0.35, 0.6, -1.0), color=(1.0, 0.9, 0.8), power=2.0, angle=20.0, samples=2),
        dict(direction=(0.0, 0.0, 1.0), color=(0.5, 0.7, 1.0), power=1.5, angle=0.27, samples=1),
        dict(direction=(-3.0, 4.0, -12.0), color=(1.0, 1.0, 1.0), power=1.0, angle=120.0, samples=3)]


def _quads(rng, n):
    """s values: uniform, 0, next to 0, next to 1, and 1"""
    edge = np.array([0.0, np.nextafter(F(0), F(1)), 0.5, np.nextafter(F(1), F(0)), 1.0], F)
    grid = np.stack(np.meshgrid(edge, edge, edge, edge, indexing="ij"), -1).reshape(-1, 4)
    return np.concatenate([rng.random((n, 4)).astype(F), grid]).astype(F)


def _hit_dirs(st, rng, n):
    """unit directions all over, on the axis, and around the cone's edge on both sides of cosAngle"""
    d, du = st["direction"].astype(np.float64), st["du"].astype(np.float64)
    dv = np.cross(d, du)
    w = rng.normal(size=(n, 3))
    a = np.arccos(min(1.0, st["cos_angle"])) + np.linspace(-3e-4, 3e-4, 4001)
    ph = rng.uniform(0, 2 * np.pi, a.shape)
    edge = d * np.cos(a)[:, None] + (du * np.cos(ph)[:, None] + dv * np.sin(ph)[:, None]) * np.sin(a)[:, None]
    w = np.concatenate([w, edge, d[None], -d[None]])
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    return w.astype(F)


@gpu
def test_probe_equals_float32_restatement(gpu_device, monkeypatch):
    """illumSample, intersect and emitPhoton of three suns, and emitPhoton of
    the area, point and directional lights beside them, bit for bit."""
    monkeypatch.setenv("YK_DEBUG_HOOKS", "1")

    def add(s):
        for k in SUNS:
            s.add_sun_light(**k)
        s.add_point_light((0.2, 1.5, -0.3), (1.0, 0.8, 0.6), 3.0)
        s.add_directional_light((0.2, -1.0, 0.3), (0.9, 1.0, 0.8), 2.0, infinite=True)
        s.add_directional_light((0.0, -1.0, 0.0), (0.9, 1.0, 0.8), 2.0, infinite=False, from_=(0, 1.9, 0), radius=0.4)
        s.add_area_light((-0.25, 1.979, -0.25), (0.25, 1.979, -0.25), (-0.25, 1.979, 0.25), (1, 0.9, 0.8), 10.0, 2)
    s, _ = _cornell("cornell_pt", add)
    bound = s.export()["bound"]
    gpu_device.upload(s)
    states = s.light_states()
    rng = np.random.default_rng(5)
    total = nan_frames = edge_in = edge_out = 0
    for li, k in enumerate(SUNS):
        st = S.struct_state(states[li])
        assert S.same_state(st, S.sun_state(**k))
        Q = _quads(rng, 6000)
        X = np.concatenate([rng.uniform(-1, 1, (len(Q), 3)).astype(F), Q[:, :2]], 1)
        _same(_light_probe(gpu_device, li, PROBE_ILLUM_SAMPLE, X), S.sun_illum(st, X), f"sun_illum {li}")
        dirs = _hit_dirs(st, rng, 4000)
        R = np.concatenate([rng.uniform(-1, 1, (len(dirs), 3)).astype(F), dirs], 1)
        want = S.sun_hit(st, R)
        _same(_light_probe(gpu_device, li, PROBE_INTERSECT, R), want, f"sun_hit {li}")
        edge = want[4000:8001, 0]
        edge_in += int((edge == 1).sum())
        edge_out += int((edge == 0).sum())
        # s4 = 0 makes ldir == direction (cosAng = 1): minRot's sinAlpha is 0, or NaN where the float dot product exceeds 1
        E = np.concatenate([Q, np.stack([rng.random(500), rng.random(500), rng.random(500), np.zeros(500)], 1).astype(F)])
        want = S.sun_emit(st, bound, E)
        _same(_light_probe(gpu_device, li, PROBE_EMIT_PHOTON, E), want, f"sun_emit {li}")
        nan_frames += int(np.isnan(want[:, 0]).sum())
        total += len(X) + len(R) + len(E)
        assert (_light_probe(gpu_device, li, PROBE_ILLUMINATE, X[:4, :3]) == 0).all()  # illuminate() returns false
    assert total > 45000 and edge_in > 100 and edge_out > 100
    print(f"{total} probe inputs; {nan_frames} emitPhoton inputs with a NaN minRot frame; edge: {edge_in} in, {edge_out} out")
    E = _quads(rng, 2000)
    _same(_light_probe(gpu_device, 3, PROBE_EMIT_PHOTON, E), S.point_emit(states[3], E), "point emit")
    _same(_light_probe(gpu_device, 4, PROBE_EMIT_PHOTON, E), S.directional_emit(states[4], bound, E), "directional emit")
    _same(_light_probe(gpu_device, 5, PROBE_EMIT_PHOTON, E), S.directional_emit(states[5], bound, E), "finite directional emit")
    _same(_light_probe(gpu_device, 6, PROBE_EMIT_PHOTON, E), S.area_emit(states[6], E)[0], "area emit")


DL_SUN = dict(direction=(0.35, 0.6, -1.0), color=(1.0, 0.9, 0.8), power=2.0, angle=20.0)


@gpu
@pytest.mark.parametrize("spp", [1, 2])
@pytest.mark.parametrize("samples", [1, 3])
def test_direct_lighting_film_equals_restatement(gpu_device, samples, spp):
    """The Cornell room lit through its open front by a wide sun (un-normalized
    direction): the film against doLightEstimation restated in float32 on the
    oracle's camera hits and isShadowed, light half, BSDF half and MIS
    weights, bit for bit, shadow-ray count included."""
    from oracle.oracle import Oracle
    from tests.dl_common import film_of
    lit, p = _cornell("cornell_dl", lambda s: s.add_sun_light(samples=samples, **DL_SUN))
    plain, _ = _cornell("cornell_dl")
    q = _params(p, A.YK_INTEGRATOR_DIRECT, spp)
    r = S.restate_direct_sun(Oracle(plain), plain, q, S.sun_state(samples=samples, **DL_SUN))
    film, st = _render(gpu_device, lit, q)
    want = film_of(r["col"], q)
    print(f"samples {samples} spp {spp}: {r['diffuse_hits']} diffuse hits, {r['lit_samples']} lit light samples, "
          f"{r['mis_samples']} unoccluded BSDF-half samples, {r['shadow_rays']} shadow rays (GPU {st.shadow_rays})")
    assert r["diffuse_hits"] > 500 and r["lit_samples"] > 100 and r["mis_samples"] > 0
    assert st.shadow_rays == r["shadow_rays"] and st.closest_rays == RES * RES * spp
    full = film[..., 4] == spp  # the pixels that hold exactly their own samples
    assert full.mean() > 0.9
    bad = (_bits(film[..., :3]) != _bits(want)).any(-1) & full
    assert not bad.any(), f"{bad.sum()} pixels differ; first {np.argwhere(bad)[0]}: {film[..., :3][bad][0]} vs {want[bad][0]}"


BEHIND = dict(direction=(0.0, 0.0, 1.0), color=(1.0, 1.0, 1.0), power=5.0, angle=0.27, samples=2)


@gpu
def test_sun_that_lights_nothing_equals_no_light_direct(gpu_device):
    """A sun behind the back wall: every shadow ray towards it from a surface
    that faces it meets a wall. The film equals the oracle's of the scene
    without the sun; the shadow rays are the restatement's (samples per point,
    plus the BSDF-half rays that fall inside the cone), none of them free."""
    from oracle.oracle import Oracle
    lit, p = _cornell("cornell_dl", lambda s: s.add_sun_light(**BEHIND))
    plain, _ = _cornell("cornell_dl")
    q = _params(p, A.YK_INTEGRATOR_DIRECT, 2)
    orc = Oracle(plain)
    _, sums_o, cnt = orc.render(q)
    r = S.restate_direct_sun(orc, plain, q, S.sun_state(**BEHIND))
    film, st = _render(gpu_device, lit, q)
    assert cnt["shadow"] == 0 and r["lit_samples"] == 0 and r["mis_samples"] == 0
    assert st.closest_rays == cnt["closest"] and st.shadow_rays == r["shadow_rays"]
    assert BEHIND["samples"] * r["diffuse_hits"] <= st.shadow_rays <= 2 * BEHIND["samples"] * r["diffuse_hits"]
    assert (_bits(film) == _bits(sums_o)).all()


@gpu
def test_sun_that_lights_nothing_equals_dark_light_path(gpu_device):
    """Path tracing picks one light per vertex and scales by their number: the
    yardstick is the oracle's frame with a directional light that gives
    nothing in the sun's place (a finite one whose cylinder misses the scene),
    beside the room's own area light. A second wall stands behind the back
    wall in both scenes: a path vertex that lands within YAF_SHADOW_BIAS
    (0.0005) of the back wall starts its shadow ray beyond that wall (tmin is
    applied along the ray), and without the second wall the sun would light
    it, here as in the reference (one such vertex in this frame: pixel (6, 8),
    +2.8e-3)."""
    from oracle.oracle import Oracle

    def backstop(s):
        s.add_mesh(np.array([[-3, -2, 1.5], [3, -2, 1.5], [3, 4, 1.5], [-3, 4, 1.5]], F),
                   np.array([[0, 1, 2], [0, 2, 3]], np.int32), 0)

    def area(s):
        s.add_area_light((-0.25, 1.979, -0.25), (0.25, 1.979, -0.25), (-0.25, 1.979, 0.25), (1, 1, 1), 10.0, 2)

    def sun(s):
        backstop(s)
        s.add_sun_light(**BEHIND)
        area(s)

    def dark(s):
        backstop(s)
        s.add_directional_light((0, 0, -1), (1, 1, 1), 5.0, infinite=False, from_=(50, 50, 50), radius=0.01)
        area(s)
    lit, p = _cornell("cornell_pt", sun)
    ref, _ = _cornell("cornell_pt", dark)
    q = _params(p, A.YK_INTEGRATOR_PATH, 2)
    _, sums_o, cnt = Oracle(ref).render(q)
    film, st = _render(gpu_device, lit, q)
    assert st.closest_rays == cnt["closest"] and st.closest_rays > RES * RES * 2
    extra = st.shadow_rays - cnt["shadow"]  # the sun's rays where a vertex picked it, all occluded
    assert 0 < extra <= 2 * BEHIND["samples"] * st.closest_rays
    bad = (_bits(film) != _bits(sums_o)).any(-1)
    d = film.astype(np.float64) - sums_o.astype(np.float64)
    print(f"{bad.sum()} of {bad.size} pixels differ; largest difference {np.abs(d).max():.3e}, sum {d[..., :3].sum():.3e}; "
          f"first {np.argwhere(bad)[:3].tolist()}; sun rays {extra}; finite {np.isfinite(film).all()}")
    assert not bad.any()


FORMS = [dict(), dict(YK_MERGE="0"), dict(YK_SPLIT="0"), dict(YK_SPLIT="1"), dict(YK_SPLIT="1", YK_SMALL="0"),
         dict(YK_SMALL="0"), dict(YK_DIFF="0"), dict(YK_PIPES="1")]
FORM_KEYS = ("YK_MERGE", "YK_SPLIT", "YK_PIPES", "YK_DIFF", "YK_SMALL")
FORM_SUN = dict(direction=(0.35, 0.6, -1.0), color=(1.0, 0.9, 0.8), power=2.0, angle=25.0, samples=2)


def _form_case(integ):
    def add(s):
        s.add_sun_light(**FORM_SUN)
        s.add_area_light((-0.25, 1.979, -0.25), (0.25, 1.979, -0.25), (-0.25, 1.979, 0.25), (1, 1, 1), 4.0, 1)
    s, p = _cornell("cornell_pt" if integ == A.YK_INTEGRATOR_PATH else "cornell_dl", add)
    return s, _params(p, integ, 2, tile_size=8)


@pytest.fixture(scope="module")
def form_reference(gpu_device):
    saved = {k: os.environ.pop(k) for k in FORM_KEYS if k in os.environ}
    ref = {}
    try:
        for integ in (A.YK_INTEGRATOR_PATH, A.YK_INTEGRATOR_DIRECT):
            s, q = _form_case(integ)
            film, st = _render(gpu_device, s, q)
            assert np.isfinite(film).all() and film[..., :3].max() > 0 and st.shadow_rays > 0
            ref[integ] = (film, (st.closest_rays, st.shadow_rays))
    finally:
        os.environ.update(saved)
    return ref


@gpu
@pytest.mark.parametrize("integ", [A.YK_INTEGRATOR_PATH, A.YK_INTEGRATOR_DIRECT], ids=["pt", "dl"])
@pytest.mark.parametrize("form", range(len(FORMS)), ids=[("-".join(f"{k}{v}" for k, v in f.items()) or "default") for f in FORMS])
def test_form_invariance(gpu_device, monkeypatch, form_reference, form, integ):
    """A sun and an area light in the Cornell room: the same film bits and ray
    counts for merged and per-bounce any-hit launches, whole and split slots
    (an unbounded BSDF-half ray has a record of its own in the split form),
    small-scene and general kernels, diffuse-only and general materials."""
    monkeypatch.setenv("YK_DEBUG_HOOKS", "1")
    s, q = _form_case(integ)
    for k in FORM_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    film, st = _render(gpu_device, s, q)
    if "YK_SPLIT" in FORMS[form]:
        split = C.c_int32(-1)
        A.check(A.lib().yk_debug_shadow_form(gpu_device._p, C.byref(q), C.byref(split)))
        assert split.value == int(FORMS[form]["YK_SPLIT"])
    assert (st.closest_rays, st.shadow_rays) == form_reference[integ][1]
    assert (_bits(film) == _bits(form_reference[integ][0])).all()


@gpu
@pytest.mark.parametrize("integ", [A.YK_INTEGRATOR_PATH, A.YK_INTEGRATOR_DIRECT], ids=["pt", "dl"])
def test_shards_repeat_and_two_handles(gpu_device, form_reference, integ):
    from core_amd.device import Device
    s, q = _form_case(integ)
    want, rays = form_reference[integ]
    again, st = _render(gpu_device, s, q)
    assert (_bits(again) == _bits(want)).all() and (st.closest_rays, st.shadow_rays) == rays
    acc = None
    for i in range(2):
        f, _ = _render(gpu_device, s, q, i, 2)
        acc = f.copy() if acc is None else acc + f
    assert (_bits(acc) == _bits(want)).all(), "two shards differ from one"
    d2 = Device(0)
    try:
        gpu_device.upload(s)
        d2.upload(s)
        multi, stn = Device.render_multi([gpu_device, d2], q)
    finally:
        d2.close()
    assert (stn.closest_rays, stn.shadow_rays) == rays
    assert (_bits(multi) == _bits(acc)).all()


# ---- photons ----------------------------------------------------------------

PH_SUN = dict(direction=(0.2, 0.5, -1.0), color=(1.0, 0.9, 0.8), power=1.5, angle=10.0, samples=1)


def _photon_scene(mirror=False, sun_samples=1):
    def add(s):
        if mirror:
            m = s.add_material(color=(1, 1, 1), diffuse_reflect=0.2, specular_reflect=0.8, mirror_color=(0.9, 0.9, 0.8))
            s.add_mesh(np.array([[-0.9, 0.01, -0.6], [-0.9, 0.01, 0.2], [-0.1, 0.01, 0.2], [-0.1, 0.01, -0.6]], F),
                       np.array([[0, 1, 2], [0, 2, 3]], np.int32), m)
        s.add_sun_light(**dict(PH_SUN, samples=sun_samples))
        s.add_area_light((-0.25, 1.979, -0.25), (0.25, 1.979, -0.25), (-0.25, 1.979, 0.25), (1, 1, 1), 10.0, 1)
    return _cornell("cornell_pt", add)


@gpu
def test_photon_emission_and_deposits_equal_the_restatement(gpu_device):
    """bounces = 0, a sun and the room's area light: every photon's light
    choice (pdf1D_t over the restated energies), emission ray and colour, then
    the oracle's closest hit of those rays on the same geometry: the exported
    diffuse map holds their deposits on diffuse surfaces, in photon order, bit
    for bit."""
    from oracle import oracle as O
    from oracle.oracle import Oracle
    N = 6000
    s, p = _photon_scene()
    plain, _ = _cornell("cornell_pt")
    q = _params(p, A.YK_INTEGRATOR_PHOTON, 1)
    q.photon.photons, q.photon.bounces, q.photon.final_gather = N, 0, 0
    gpu_device.upload(s)
    info = gpu_device.photon_build(q)
    got = gpu_device.photon_map(A.YK_PHOTON_MAP_DIFFUSE)[:info.diffuse_photons]
    bound = s.export()["bound"]
    states = s.light_states()
    st = S.struct_state(states[0])
    energies = [S.light_energy(A.YK_LIGHT_SUN, None, bound, st), S.light_energy(A.YK_LIGHT_AREA, states[1], bound)]
    cdf, inv_integral = S.light_pdf(energies)
    L = O.lib()
    curr = np.arange(N, dtype=np.uint32)
    Q = np.array([[L.orc_ri_vdc(int(c), 0), F(L.orc_scrhalton(2, int(c))), F(L.orc_scrhalton(3, int(c))),
                   F(L.orc_scrhalton(4, int(c)))] for c in curr], F)
    sL = (curr.astype(F) * (F(1.0) / F(N))).astype(F)
    ln = np.where(sL == 0, 0, np.maximum(np.searchsorted(cdf, sL, side="left") - 1, 0))
    assert (ln == 0).sum() > 100 and (ln == 1).sum() > 100
    rec = np.where((ln == 0)[:, None], S.sun_emit(st, bound, Q), S.area_emit(states[1], Q)[0]).astype(F)
    num_pdf = (np.array(energies, F)[ln] * inv_integral).astype(F)
    k = ((F(2.0) * rec[:, 6]).astype(F) / num_pdf).astype(F)
    pcol = (rec[:, 7:10] * k[:, None]).astype(F)
    rays = np.zeros((N, 8), F)
    rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7] = rec[:, 0:3], rec[:, 3:6], S.MIN_RAYDIST, -1.0
    live = np.isfinite(rays[:, :6]).all(1) & (pcol != 0).any(1)
    orc = Oracle(plain)
    prim, t = orc.intersect(rays[live])[:2]
    ms = plain.material_states()
    hit = prim >= 0
    diffuse = np.zeros(len(prim), bool)
    diffuse[hit] = [bool(ms[m].bsdf_flags & 0x4) for m in orc.arrays["tri_material"][prim[hit]]]
    r = rays[live][diffuse]
    want = np.concatenate([(r[:, 0:3] + t[diffuse, None] * r[:, 3:6]).astype(F), -r[:, 3:6], pcol[live][diffuse]], 1)
    print(f"{N} photons: {(ln == 0).sum()} from the sun, {int(live.sum())} traced, {len(want)} deposits (GPU {len(got)})")
    assert len(got) == len(want) and (ln[live][diffuse] == 0).sum() > 100
    _same(got, want, "diffuse map")


@gpu
@pytest.mark.parametrize("fg", [0, 1])
def test_photon_mapping_runs_and_repeats(gpu_device, fg):
    """3 bounces, final gathering off and on: maps and films are finite, lit
    and repeat bit for bit; with final gathering the gather paths' one-light
    estimates pick the sun: doubling the sun's samples alone adds more shadow
    rays than the camera hits can account for."""
    def run(samples):
        s, p = _photon_scene(sun_samples=samples)
        q = _params(p, A.YK_INTEGRATOR_PHOTON, 1)
        q.photon.photons, q.photon.bounces, q.photon.final_gather = 20000, 3, fg
        q.photon.fg_samples, q.photon.fg_bounces, q.photon.fg_min_pathlen = 8, 2, 100.0
        gpu_device.upload(s)
        info = gpu_device.photon_build(q)
        maps = [gpu_device.photon_map(w).copy() for w in
                ([A.YK_PHOTON_MAP_DIFFUSE] + ([A.YK_PHOTON_MAP_RADIANCE] if fg else []))]
        film = gpu_device.new_film(q)
        st = gpu_device.render_shard(q, film)
        return info, maps, film.cpu().numpy(), st
    info, maps, film, st = run(1)
    info2, maps2, film2, st2 = run(1)
    assert info.diffuse_photons > 1000 and (not fg or info.radiance_photons > 0)
    for a, b in zip(maps, maps2):
        assert np.isfinite(a).all() and np.abs(a[:, 6:9]).max() > 0 and (_bits(a) == _bits(b)).all()
    assert np.isfinite(film).all() and film[..., :3].max() > 0 and (_bits(film) == _bits(film2)).all()
    assert (st.closest_rays, st.shadow_rays) == (st2.closest_rays, st2.shadow_rays)
    if fg:
        # A camera hit estimates all lights: the sun owns 2 slots with one sample, of which the light sample always
        # traces, and 4 with two, so doubling adds at most 3 rays per camera hit. What it adds beyond that comes
        # from gather vertices whose estimateOneDirectLight picked the sun (8 gather paths per camera hit).
        _, _, _, st_d = run(2)
        extra = st_d.shadow_rays - st.shadow_rays
        print(f"shadow rays {st.shadow_rays} -> {st_d.shadow_rays} with the sun's samples doubled; camera hits <= {RES * RES}")
        assert extra > 3 * RES * RES, (st.shadow_rays, st_d.shadow_rays)


@gpu
def test_caustic_only_builds(gpu_device):
    """A mirror on the floor under a sun and the area light: photon mapping's
    caustic pass, path tracing with photon caustics and direct lighting with
    dl_caustics all build a caustic map. The two caustic-only builds run the
    same pass (createCausticMap) and give the same map bit for bit, which is
    the equality the existing tests state for the area light; photon mapping's
    own pass draws its light choice as curr * (1 / N), not curr / N, and
    samples all components, so its map is another one (its size is printed)."""
    s, p = _photon_scene(mirror=True)
    gpu_device.upload(s)
    q = _params(p, A.YK_INTEGRATOR_PHOTON, 1)
    q.photon.photons = q.photon.caustic_photons = 20000
    q.photon.bounces, q.photon.final_gather = 3, 0
    info = gpu_device.photon_build(q)
    pm = gpu_device.photon_map(A.YK_PHOTON_MAP_CAUSTIC)[:info.caustic_photons].copy()
    assert info.caustic_photons > 50 and np.isfinite(pm).all()
    maps = {}
    for mode in ("pt_caustic", "dl_caustic"):
        if mode == "pt_caustic":
            c = _params(p, A.YK_INTEGRATOR_PATH, 1, caustic_type=A.YK_CAUSTIC_PHOTON)
        else:
            c = _params(p, A.YK_INTEGRATOR_DIRECT, 1, dl_caustics=1)
        c.photon = q.photon
        info_c = gpu_device.photon_build(c)
        maps[mode] = gpu_device.photon_map(A.YK_PHOTON_MAP_CAUSTIC)[:info_c.caustic_photons].copy()
        print(f"{mode}: {info_c.caustic_photons} caustic photons, photon mapping {info.caustic_photons}")
        assert info_c.caustic_photons > 50 and np.isfinite(maps[mode]).all() and np.abs(maps[mode][:, 6:9]).max() > 0
        film = gpu_device.new_film(c)
        gpu_device.render_shard(c, film)
        f = film.cpu().numpy()
        assert np.isfinite(f).all() and f[..., :3].max() > 0
    assert maps["pt_caustic"].shape == maps["dl_caustic"].shape
    assert (_bits(maps["pt_caustic"]) == _bits(maps["dl_caustic"])).all()


@gpu
def test_photon_build_still_refuses_spot_sphere_and_mesh_lights_beside_a_sun(gpu_device):
    s, p = _cornell("cornell_pt", lambda s: (s.add_sun_light(**PH_SUN), s.add_sphere_light((0, 1, 0), 0.2)))
    gpu_device.upload(s)
    q = _params(p, A.YK_INTEGRATOR_PHOTON, 1)
    q.photon.photons = 1000
    with pytest.raises(A.YkError) as e:
        gpu_device.photon_build(q)
    assert e.value.code == A.YK_ERR_UNSUPPORTED and "spot or sphere light" in str(e.value)


@gpu
def test_plain_scene_after_a_sun_scene_equals_the_oracle(gpu_device, monkeypatch):
    from oracle.oracle import Oracle
    monkeypatch.setenv("YK_DEBUG_HOOKS", "1")
    kind = C.c_int32(-1)
    plain = Scene()
    p = plain.generate("cornell_pt", RES, RES)
    plain.build()
    gpu_device.upload(plain)
    A.check(A.lib().yk_debug_shading_kind(gpu_device._p, C.byref(kind)))
    before = kind.value
    s, ps = _photon_scene()
    film, _ = _render(gpu_device, s, _params(ps, A.YK_INTEGRATOR_PATH, 1))
    assert film[..., :3].max() > 0
    q = _params(p, A.YK_INTEGRATOR_PATH, 2)
    film, st = _render(gpu_device, plain, q)
    A.check(A.lib().yk_debug_shading_kind(gpu_device._p, C.byref(kind)))
    assert kind.value == before == 1
    _, sums_o, cnt = Oracle(plain).render(q)
    assert (st.closest_rays, st.shadow_rays) == (cnt["closest"], cnt["shadow"])
    assert (_bits(film) == _bits(sums_o)).all()
