"""Spot and sphere lights (spotlight.cc, spherelight.cc) on the GPU path.

CPU: the C-ABI's argument checks, the parameter -> state conversion against a
float32 / float64 restatement of the two constructors, round trips.
GPU: the lights' device functions against a float32 restatement (no fused
multiply-add, the reference source's operation order and types), a hard spot's
inner cone against the oracle's point light, a spot that lights nothing
against the oracle's scene without it, the blend region's monotonicity, form
invariance of the sampled lights, the photon refusal and two handles.

The oracle knows nothing of these lights and is never given a scene that
holds one. Where the oracle is not the yardstick (light functions, blend,
forms, handles) the checks are restatements or invariants: like SURVEY row f1
they are unpinned against the compiled reference.

A sphere light takes `samples` shadow rays per estimate, not 2 * samples:
sphereLight_t::canIntersect() is false (spherelight.cc:49), so
doLightEstimation (mcintegrator.cc:109,134,156) gives it neither a MIS weight
nor a BSDF half.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

from core_amd import _abi as A
from core_amd.scene import Scene

f32 = np.float32
f64 = np.float64
PI2_D = 6.28318530717958647692
DEG = 0.01745329251994329576922

PROBE_ILLUMINATE, PROBE_ILLUM_SAMPLE, PROBE_INTERSECT, PROBE_STRIDE = 0, 1, 2, 12
YK_PROBE_FSIN, YK_PROBE_FCOS, YK_PROBE_HOST_FSIN = 4, 5, 12


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _light_probe(dev, light, fn, inp):
    """yk_debug_light_probe (include/yk_test_hooks_light.h), bound here: the
    hook is not part of the product ABI table."""
    f = A.lib().yk_debug_light_probe
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int32, C.c_int32, A.fp, C.c_int64, A.fp]
    inp = np.ascontiguousarray(inp, f32)
    out = np.full((len(inp), PROBE_STRIDE), np.nan, f32)
    A.check(f(dev._p, light, fn, inp.ctypes.data_as(A.fp), len(inp), out.ctypes.data_as(A.fp)))
    return out


def _qmc_probe(dev_p, fn, x):
    x = np.ascontiguousarray(x, f32)
    out = np.zeros_like(x)
    A.check(A.lib().yk_debug_qmc_probe(dev_p, fn, x.ctypes.data, None, x.size, out.ctypes.data))
    return out


# ------------------------------------------------------------------ CPU


def _spot(**kw):
    a = dict(type=A.YK_LIGHT_SPOT, color=A.f3(1, 1, 1), power=1.0, samples=8, from_=A.f3(0, 0, 0),
             to=A.f3(0, 0, -1), cone_angle=45.0, blend=0.15, soft_shadows=0, shadow_fuzzyness=1.0, photon_only=0)
    a.update(kw)
    return A.yk_light(**a)


def _sphere(**kw):
    a = dict(type=A.YK_LIGHT_SPHERE, color=A.f3(1, 1, 1), power=1.0, samples=4, from_=A.f3(0, 0, 0), radius=1.0)
    a.update(kw)
    return A.yk_light(**a)


def test_add_light_accepts_and_refuses():
    s = Scene()
    add = lambda l: A.lib().yk_scene_add_light(s.handle, C.byref(l))
    assert A.YK_LIGHT_SPOT == 3 and A.YK_LIGHT_SPHERE == 4
    assert add(_spot()) == A.YK_OK
    assert add(_spot(soft_shadows=1, samples=1)) == A.YK_OK
    assert add(_spot(samples=0)) == A.YK_OK  # a hard spot never reads samples
    assert add(_spot(cone_angle=180.0)) == A.YK_OK
    assert add(_sphere()) == A.YK_OK
    assert s.info().nlights == 5
    bad = [_spot(soft_shadows=1, samples=0), _spot(to=A.f3(0, 0, 0)), _spot(cone_angle=0.0),
           _spot(cone_angle=-10.0), _spot(cone_angle=180.5), _spot(cone_angle=float("nan")),
           _sphere(samples=0), _sphere(radius=0.0), _sphere(radius=-1.0)]
    for l in bad:
        assert add(l) == A.YK_ERR_ARG
        assert len(A.lib().yk_last_error()) > 0
    assert add(A.yk_light(type=5)) == A.YK_ERR_UNSUPPORTED
    assert s.info().nlights == 5
    # the state-level entry points check what they can
    st = A.yk_spot_light_state(soft_shadows=1, samples=0)
    assert A.lib().yk_scene_add_spot_light_state(s.handle, C.byref(st)) == A.YK_ERR_ARG
    sp = A.yk_sphere_light_state(radius=0.0, samples=1)
    assert A.lib().yk_scene_add_sphere_light_state(s.handle, C.byref(sp)) == A.YK_ERR_ARG


def test_appended_fields_keep_the_old_offsets():
    """yk_light grew at its end only (the oracle is compiled against it)."""
    assert A.yk_light.infinite.offset == 88 and A.yk_light.to.offset == 92
    assert C.sizeof(A.yk_light) == 92 + 12 + 5 * 4


def test_round_trip_parameters_and_states():
    s = Scene()
    s.add_spot_light((0.5, 2, -1), (0, 0, 0.25), (1, 0.5, 0.25), 3.0, cone_angle=33.0, blend=0.4,
                     soft_shadows=True, samples=5, shadow_fuzzyness=0.7, photon_only=True)
    s.add_sphere_light((1, 2, 3), 0.25, (0.5, 1, 2), 4.0, samples=3)
    s.add_point_light((0, 1, 0))
    l = s.lights()
    assert l[0].type == A.YK_LIGHT_SPOT and l[0].to[:] == [0, 0, 0.25] and l[0].cone_angle == 33.0
    assert l[0].blend == f32(0.4) and l[0].soft_shadows == 1 and l[0].samples == 5
    assert l[0].shadow_fuzzyness == f32(0.7) and l[0].photon_only == 1
    assert l[1].type == A.YK_LIGHT_SPHERE and l[1].from_[:] == [1, 2, 3] and l[1].radius == 0.25 and l[1].samples == 3
    st = s.light_states()
    assert [type(x) for x in st] == [A.yk_spot_light_state, A.yk_sphere_light_state, A.yk_dirac_light_state]
    # every getter refuses the other kinds
    L = A.lib()
    assert L.yk_scene_get_spot_light_state(s.handle, 1, C.byref(A.yk_spot_light_state())) == A.YK_ERR_STATE
    assert L.yk_scene_get_sphere_light_state(s.handle, 0, C.byref(A.yk_sphere_light_state())) == A.YK_ERR_STATE
    assert L.yk_scene_get_dirac_light_state(s.handle, 0, C.byref(A.yk_dirac_light_state())) == A.YK_ERR_STATE
    assert L.yk_scene_get_area_light_state(s.handle, 1, C.byref(A.yk_area_light_state())) == A.YK_ERR_STATE
    assert L.yk_scene_get_spot_light_state(s.handle, 3, C.byref(A.yk_spot_light_state())) == A.YK_ERR_ARG
    # states -> a second scene -> the same states; no parameter-level light there
    t = Scene()
    t.add_spot_light_state(st[0])
    t.add_sphere_light_state(st[1])
    t.add_dirac_light_state(st[2])
    assert [bytes(x) for x in t.light_states()] == [bytes(x) for x in st]
    with pytest.raises(A.YkError) as e:
        t.lights()
    assert e.value.code == A.YK_ERR_STATE


def _host_fcos(x, monkeypatch):
    """fCos = fSin(x + (float)M_PI_2) (mathOptimizations.h:273-280), fSin from
    the host probe (the copy the film tables use)."""
    monkeypatch.setenv("YK_DEBUG_HOOKS", "1")
    return _qmc_probe(None, YK_PROBE_HOST_FSIN, f32(x) + f32(1.57079632679489661923))


def _create_cs(N):
    """createCS, vector3d.h:316-334, one float32 vector"""
    N = np.asarray(N, f32)
    if N[0] == 0 and N[1] == 0:
        return np.array([-1 if N[2] < 0 else 1, 0, 0], f32), np.array([0, 1, 0], f32)
    d = f32(1.0 / f64(np.sqrt(N[1] * N[1] + N[0] * N[0])))
    u = np.array([N[1] * d, -N[0] * d, 0], f32)
    v = np.array([N[1] * u[2] - N[2] * u[1], N[2] * u[0] - N[0] * u[2], N[0] * u[1] - N[1] * u[0]], f32)
    return u, v


SPOT_CASES = [((0.5, 2.0, -1.0), (0.1, 0.0, 0.25), 33.0, 0.4), ((0, 0, 0), (0, 0, -1), 45.0, 0.15),
              ((0, 0, 0), (0, 0, 2), 80.0, 0.1), ((1, 1, 1), (-2, 0.5, 7), 180.0, 1.0), ((0, 3, 0), (0, 0, 0), 0.5, 0.0)]


@pytest.mark.parametrize("frm,to,angle,blend", SPOT_CASES)
def test_spot_state_equals_constructor_restatement(monkeypatch, frm, to, angle, blend):
    """spotLight_t::spotLight_t, spotlight.cc:63-75, bit for bit."""
    s = Scene()
    s.add_spot_light(frm, to, (0.3, 0.7, 1.1), 2.5, cone_angle=angle, blend=blend, samples=6, soft_shadows=True)
    st = s.light_states()[0]
    nd = np.asarray(frm, f32) - np.asarray(to, f32)
    l = nd[0] * nd[0] + nd[1] * nd[1] + nd[2] * nd[2]
    nd = nd * (f32(1) / np.sqrt(l))
    du, dv = _create_cs(-nd)
    rad = f64(f32(angle)) * DEG
    rad_in = rad * f64(f32(1) - f32(blend))
    cs = _host_fcos(np.array([f32(rad_in)]), monkeypatch)[0]
    ce = _host_fcos(np.array([f32(rad)]), monkeypatch)[0]
    with np.errstate(divide="ignore"):
        icd = f32(1.0 / f64(cs - ce))
    for got, want in ((st.position, frm), (st.ndir, nd), (st.dir, -nd), (st.du, du), (st.dv, dv),
                      (st.color, np.array([0.3, 0.7, 1.1], f32) * f32(2.5)),
                      ([st.cos_start, st.cos_end, st.icos_diff], [cs, ce, icd])):
        assert (_bits(got[:]) == _bits(want)).all(), (got[:], want)
    assert (st.soft_shadows, st.samples, st.photon_only, st.shadow_fuzzyness) == (1, 6, 0, 1.0)
    assert st.cos_start >= st.cos_end


@pytest.mark.parametrize("radius", [1.0, 0.25, 0.1, 3.3, 1e-3, 777.7])
def test_sphere_state_equals_constructor_restatement(radius):
    """sphereLight_t::sphereLight_t, spherelight.cc:64-72, bit for bit."""
    s = Scene()
    s.add_sphere_light((1, 2, 3), radius, (0.5, 1, 2), 4.0, samples=3)
    st = s.light_states()[0]
    r = f32(radius)
    sr = r * r
    want = [r, sr, f32(f64(sr) * 1.000003815), f32(f64(sr) * 4.0 * 3.14159265358979323846)]
    assert (_bits([st.radius, st.square_radius, st.square_radius_epsilon, st.area]) == _bits(want)).all()
    assert st.center[:] == [1, 2, 3] and st.color[:] == [2, 4, 8] and st.samples == 3


# ------------------------------------------------------------------ GPU

gpu = pytest.mark.gpu


def _no_light_cornell(resx, resy, gen):
    """The Cornell probe without its area light (the emitting quad stays a
    mesh): rebuilt from its object state, so that the scene's only lights are
    the ones a test adds."""
    src = Scene()
    p = src.generate(gen, resx, resy)
    src.build()
    e = src.export()
    t = Scene()
    for m in src.material_states():
        t.add_material_state(m)
    tv, tm = e["tri_verts"], e["tri_material"]
    start = 0
    while start < len(tm):
        end = start
        while end < len(tm) and tm[end] == tm[start]:
            end += 1
        pts = tv[start:end].reshape(-1, 3)
        t.add_mesh(pts, np.arange(len(pts), dtype=np.int32).reshape(-1, 3), int(tm[start]))
        start = end
    t.set_camera_state(src.camera_state())
    return t, p


def _params(p, **over):
    q = A.yk_render_params.from_buffer_copy(p)
    q.width = q.height = 64
    q.aa_samples = 4
    q.filter = A.YK_FILTER_BOX
    for k, v in over.items():
        setattr(q, k, v)
    return q


def _render(dev, s, q):
    dev.upload(s)
    film = dev.new_film(q)
    st = dev.render_shard(q, film)
    return film.cpu().numpy(), st


def _angles_to_axis(s, frm, to):
    """Angle (degrees, float64) between the spot's axis and every mesh vertex."""
    v = s.export()["tri_verts"].reshape(-1, 3).astype(f64) - np.asarray(frm, f64)
    ax = np.asarray(to, f64) - np.asarray(frm, f64)
    c = v @ ax / (np.linalg.norm(v, axis=1) * np.linalg.norm(ax))
    return np.degrees(np.arccos(np.clip(c, -1, 1)))


# --- 1. light functions ---------------------------------------------------

def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def _sample_cone(D, U, V, maxcos, s1, s2, trig):
    """sampleCone, sample_utils.h:76-82"""
    cos_a = f32(1) - (f32(1) - maxcos) * s2
    sin_a = np.sqrt(f32(1) - cos_a * cos_a)
    t1 = (PI2_D * s1.astype(f64)).astype(f32)
    ct, st = trig(YK_PROBE_FCOS, t1)[:, None], trig(YK_PROBE_FSIN, t1)[:, None]
    return (U * ct + V * st) * sin_a[:, None] + D * cos_a[:, None]


def _falloff(st, cosa):
    ok = ~(cosa < f32(st.cos_end))
    x = (cosa - f32(st.cos_end)) * f32(st.icos_diff)
    v = np.where(cosa >= f32(st.cos_start), f32(1), (x * x) * (f32(3) - f32(2) * x)).astype(f32)
    return ok, v


def _pack(ok, cols):
    out = np.zeros((len(ok), PROBE_STRIDE), f32)
    out[:, 0] = ok
    for k, c in enumerate(cols):
        out[:, 1 + k] = np.where(ok, c, f32(0))
    return out


def spot_illuminate(st, P):
    """spotLight_t::illuminate, spotlight.cc:113-142"""
    color = np.asarray(st.color[:], f32)
    l = np.asarray(st.position[:], f32) - P
    d2 = _dot(l, l)
    dist = np.sqrt(d2)
    ok = (dist != 0) & (st.photon_only == 0)
    idist = f32(1) / d2
    ld = l * (f32(1) / dist)[:, None]
    cosa = _dot(np.broadcast_to(np.asarray(st.ndir[:], f32), ld.shape), ld)
    inside, v = _falloff(st, cosa)
    k = np.where(cosa >= f32(st.cos_start), idist, v * idist).astype(f32)
    col = color[None, :] * k[:, None]
    return _pack(ok & inside, [ld[:, 0], ld[:, 1], ld[:, 2], dist, col[:, 0], col[:, 1], col[:, 2]])


def spot_illum_sample(st, X, trig):
    """spotLight_t::illumSample, spotlight.cc:144-175"""
    P, s1, s2 = X[:, :3], X[:, 3], X[:, 4]
    color = np.asarray(st.color[:], f32)
    l = np.asarray(st.position[:], f32) - P
    d2 = _dot(l, l)
    ok = (d2 != 0) & (st.photon_only == 0)
    dist = np.sqrt(d2)
    ld = l * (f32(1) / dist)[:, None]
    cosa = _dot(np.broadcast_to(np.asarray(st.ndir[:], f32), ld.shape), ld)
    inside, v = _falloff(st, cosa)
    fz = f32(st.shadow_fuzzyness)
    U = np.broadcast_to(np.asarray(st.du[:], f32), ld.shape)
    V = np.broadcast_to(np.asarray(st.dv[:], f32), ld.shape)
    d = _sample_cone(ld, U, V, f32(st.cos_end), s1 * fz, s2 * fz, trig)
    col = color[None, :] * v[:, None]
    return _pack(ok & inside, [d[:, 0], d[:, 1], d[:, 2], dist, col[:, 0], col[:, 1], col[:, 2], d2])


def spot_intersect(st, X):
    """spotLight_t::intersect, spotlight.cc:243-280 (with its exact plane test
    and its distance from the world origin)"""
    frm, dr = X[:, :3], X[:, 3:6]
    color = np.asarray(st.color[:], f32)
    d = np.broadcast_to(np.asarray(st.dir[:], f32), dr.shape)
    pos = np.asarray(st.position[:], f32)
    cosA = _dot(d, dr)
    ok = cosA != 0
    t = _dot(d, pos - frm) / cosA
    ok &= ~(t < 0)
    P = frm + t[:, None] * dr
    ok &= _dot(d, P - pos) == 0
    ok &= _dot(P, P).astype(f64) <= 1e-2
    inside, v = _falloff(st, cosA)
    col = color[None, :] * v[:, None]
    return _pack(ok & inside, [t, np.ones_like(t), col[:, 0], col[:, 1], col[:, 2], f32(1) / (t * t)])


def _sphere_isect(frm, dr, c, R2):
    """sphereIntersect, spherelight.cc:88-100"""
    vf = frm - c
    ea = _dot(dr, dr)
    eb = _dot(f32(2) * vf, dr)
    ec = _dot(vf, vf) - R2
    osc = ((eb * eb).astype(f64) - 4.0 * ea.astype(f64) * ec.astype(f64)).astype(f32)
    hit = ~(osc < 0)
    d1 = ((-eb - np.sqrt(osc)).astype(f64) / (2.0 * ea.astype(f64))).astype(f32)
    return hit, d1


def _create_cs_rows(N):
    pole = (N[:, 0] == 0) & (N[:, 1] == 0)
    d = f32(1) / np.sqrt(N[:, 1] * N[:, 1] + N[:, 0] * N[:, 0])
    z = np.zeros_like(d)
    u = np.stack([N[:, 1] * d, -N[:, 0] * d, z], 1)
    v = np.stack([N[:, 1] * u[:, 2] - N[:, 2] * u[:, 1], N[:, 2] * u[:, 0] - N[:, 0] * u[:, 2],
                  N[:, 0] * u[:, 1] - N[:, 1] * u[:, 0]], 1)
    u[pole] = np.stack([np.where(N[pole, 2] < 0, f32(-1), f32(1)), z[pole], z[pole]], 1)
    v[pole] = [0, 1, 0]
    return u.astype(f32), v.astype(f32)


def sphere_illum_sample(st, X, trig):
    """sphereLight_t::illumSample, spherelight.cc:102-132"""
    P, s1, s2 = X[:, :3], X[:, 3], X[:, 4]
    c = np.asarray(st.center[:], f32)
    sr = f32(st.square_radius)
    cdir = c - P
    d2 = _dot(cdir, cdir)
    ok = ~(d2 <= sr)
    dist = np.sqrt(d2)
    idist = f32(1) / d2
    cos_alpha = np.sqrt(f32(1) - sr * idist)
    cdir = cdir * (f32(1) / dist)[:, None]
    du, dv = _create_cs_rows(cdir)
    d = _sample_cone(cdir, du, dv, cos_alpha, s1, s2, trig)
    hit, d1 = _sphere_isect(P, d, c, f32(st.square_radius_epsilon))
    pdf = f32(1) / (f32(2) * (f32(1) - cos_alpha))
    col = np.asarray(st.color[:], f32)
    one = np.ones_like(d1)
    return _pack(ok & hit, [d[:, 0], d[:, 1], d[:, 2], d1, col[0] * one, col[1] * one, col[2] * one, pdf])


def sphere_intersect(st, X):
    """sphereLight_t::intersect, spherelight.cc:134-149: t is never written"""
    frm, dr = X[:, :3], X[:, 3:6]
    c = np.asarray(st.center[:], f32)
    sr = f32(st.square_radius)
    hit, _ = _sphere_isect(frm, dr, c, sr)
    cdir = c - frm
    d2 = _dot(cdir, cdir)
    ok = hit & ~(d2 <= sr)
    cos_alpha = np.sqrt(f32(1) - sr * (f32(1) / d2))
    col = np.asarray(st.color[:], f32)
    z = np.zeros_like(d2)
    return _pack(ok, [z, z, col[0] + z, col[1] + z, col[2] + z, f32(2) * (f32(1) - cos_alpha)])


def _unit(v):
    v = np.asarray(v, f64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _probe_scene():
    """Cornell + [1] soft spot (fuzzy 1), [2] soft spot (fuzzy 0, wide blend),
    [3] hard spot, [4] sphere, [5] soft spot at the world origin looking down
    -z (the only place where spotLight_t::intersect can answer yes)."""
    s = Scene()
    s.generate("cornell_dl", 16, 16)
    s.add_spot_light((0.2, 1.8, -0.3), (0.0, 0.0, 0.1), (1, 0.9, 0.8), 3.0, cone_angle=35, blend=0.3,
                     soft_shadows=True, samples=4)
    s.add_spot_light((-0.5, 1.5, 0.2), (0.5, 0.0, 0.0), (0.5, 0.7, 1), 2.0, cone_angle=50, blend=0.8,
                     soft_shadows=True, samples=2, shadow_fuzzyness=0.0)
    s.add_spot_light((0.0, 1.9, 0.0), (0.0, 0.0, 0.0), (1, 1, 1), 1.5, cone_angle=30, blend=0.5)
    s.add_sphere_light((0.3, 1.2, -0.2), 0.25, (1, 0.8, 0.6), 5.0, samples=4)
    s.add_spot_light((0, 0, 0), (0, 0, -1), (0.9, 1, 1.1), 2.0, cone_angle=40, blend=0.25, soft_shadows=True,
                     samples=2)
    s.build()
    return s


def _spot_points(st, rng, n):
    """Random points plus the edges: on the axis, at the light, and around
    both cone angles (cosa straddling cosEnd and cosStart)."""
    pos, dr = np.asarray(st.position[:], f64), np.asarray(st.dir[:], f64)
    du = np.asarray(st.du[:], f64)
    P = [rng.uniform(-1.2, 1.2, (n, 3)) + [0, 1, 0]]
    P.append(pos + dr * rng.uniform(0.01, 3, (64, 1)))  # on the axis
    P.append(np.repeat(pos[None], 4, 0))  # dist == 0
    for c in (st.cos_end, st.cos_start):
        a = np.arccos(np.clip(c, -1, 1)) + np.linspace(-2e-3, 2e-3, 801)
        ph = rng.uniform(0, 2 * np.pi, a.shape)
        dv = np.cross(dr, du)
        w = dr * np.cos(a)[:, None] + (du * np.cos(ph)[:, None] + dv * np.sin(ph)[:, None]) * np.sin(a)[:, None]
        P.append(pos + w * rng.uniform(0.2, 2.5, (len(a), 1)))
    return np.concatenate(P).astype(f32)


def _samples(rng, n):
    edge = np.array([0.0, 1.0 - 2.0 ** -24, 1.0 - 2.0 ** -12, 0.5, 2.0 ** -30], f32)
    s = rng.random((n, 2)).astype(f32)
    k = min(n, 400)
    s[:k] = np.array(list(itertools.product(edge, edge)), f32)[np.arange(k) % 25]
    return s


def _same(got, want, what):
    assert (got[:, 0] == want[:, 0]).all(), f"{what}: ok differs in {(got[:, 0] != want[:, 0]).sum()} of {len(got)}"
    bad = (_bits(got) != _bits(want)).any(axis=1)
    assert not bad.any(), f"{what}: {bad.sum()} of {len(got)} differ, first {got[bad][0]} vs {want[bad][0]}"


@gpu
def test_light_functions_equal_float32_restatement(gpu_device, monkeypatch):
    monkeypatch.setenv("YK_DEBUG_HOOKS", "1")
    s = _probe_scene()
    gpu_device.upload(s)
    st = s.light_states()
    trig = lambda fn, x: _qmc_probe(gpu_device._p, fn, x)
    rng = np.random.default_rng(5)
    n = 3000
    with np.errstate(all="ignore"):
        seen = dict(spot_ok=0, spot_out=0, spot_blend=0, sph_ok=0, sph_in=0, sph_graze=0, hit_ok=0)
        for li in (1, 2, 3, 5):
            P = _spot_points(st[li], rng, n)
            got = _light_probe(gpu_device, li, PROBE_ILLUMINATE, P)
            _same(got, spot_illuminate(st[li], P), f"illuminate[{li}]")
            seen["spot_ok"] += int(got[:, 0].sum())
            seen["spot_out"] += int((got[:, 0] == 0).sum())
            X = np.concatenate([P, _samples(rng, len(P))], 1)
            got = _light_probe(gpu_device, li, PROBE_ILLUM_SAMPLE, X)
            want = spot_illum_sample(st[li], X, trig)
            _same(got, want, f"illumSample[{li}]")
            seen["spot_blend"] += int(((got[:, 0] == 1) & (got[:, 5] < f32(st[li].color[0]))).sum())
            R = np.concatenate([P, _unit(rng.normal(size=P.shape)).astype(f32)], 1)
            _same(_light_probe(gpu_device, li, PROBE_INTERSECT, R), spot_intersect(st[li], R), f"intersect[{li}]")
        # the spot at the origin: rays that meet its plane z = 0 exactly, inside and outside |P|^2 <= 1e-2
        xy = rng.uniform(-0.15, 0.15, (n, 2))
        tilt = rng.uniform(-1.2, 1.2, (n, 2)) * (rng.random((n, 1)) < 0.5)
        R = np.concatenate([xy - tilt, np.ones((n, 1)), tilt, -np.ones((n, 1))], 1).astype(f32)
        got = _light_probe(gpu_device, 5, PROBE_INTERSECT, R)
        _same(got, spot_intersect(st[5], R), "intersect[origin spot]")
        seen["hit_ok"] = int(got[:, 0].sum())
        # sphere: outside, inside, on the surface, far away
        sp = st[4]
        c, r = np.asarray(sp.center[:], f64), sp.radius
        u = _unit(rng.normal(size=(n, 3)))
        P = np.concatenate([rng.uniform(-1.2, 1.2, (n, 3)) + [0, 1, 0], c + u * r * rng.random((n, 1)),
                            c + u[:500] * r, c + u[:600] * 10 ** rng.uniform(1, 5, (600, 1)), c[None]]).astype(f32)
        X = np.concatenate([P, _samples(rng, len(P))], 1)
        got = _light_probe(gpu_device, 4, PROBE_ILLUM_SAMPLE, X)
        _same(got, sphere_illum_sample(sp, X, trig), "sphere illumSample")
        seen["sph_ok"] = int(got[:, 0].sum())
        d2 = ((c - P.astype(f64)) ** 2).sum(1)
        seen["sph_in"] = int((d2 <= sp.square_radius).sum())
        seen["sph_graze"] = int(((got[:, 0] == 0) & (d2 > sp.square_radius * 1.001)).sum())  # osc < 0
        # intersect: rays aimed at, past and tangent to the sphere
        frm = P[:n]
        aim = c + u * r * np.concatenate([rng.uniform(0, 2, (n - 600, 1)), rng.uniform(0.999, 1.001, (600, 1))])
        dr = (aim - frm).astype(f32)
        dr[: n // 2] = _unit(dr[: n // 2]).astype(f32)
        R = np.concatenate([frm, dr], 1)
        got = _light_probe(gpu_device, 4, PROBE_INTERSECT, R)
        _same(got, sphere_intersect(sp, R), "sphere intersect")
        assert 0 < got[:, 0].sum() < n and (got[:, 2] == 0).all()  # t_set: never
        # the kinds that have no such function answer no
        assert (_light_probe(gpu_device, 4, PROBE_ILLUMINATE, P[:64])[:, 0] == 0).all()
        assert (_light_probe(gpu_device, 0, PROBE_ILLUMINATE, P[:64])[:, 0] == 0).all()
    print("light-function cases seen:", seen)
    seen.pop("sph_graze")  # rounding decides whether a cone-edge sample misses the enlarged sphere
    assert all(v > 0 for v in seen.values()), seen


# --- 2. / 3. against the oracle ---------------------------------------------

SPOT_FROM, SPOT_TO = (0.0, 1.0, -4.0), (0.0, 1.0, 0.0)
MODES = [("dl", 0), ("pt", 0), ("dl", 1), ("pt", 1)]


def _mode(p, integ, ts):
    return _params(p, integrator=A.YK_INTEGRATOR_DIRECT if integ == "dl" else A.YK_INTEGRATOR_PATH, bounces=3,
                   transp_shadows=ts)


def _cornell_with(add, gen, pane):
    s = Scene()
    p = s.generate(gen, 64, 64)
    if pane:  # a transparent wall in front of the back wall, so that shadow rays get filtered
        m = s.add_material(color=(0.9, 0.5, 0.2), diffuse_reflect=0.3, transparency=0.7, transmit_filter=0.6)
        s.add_mesh([[-0.9, 0.1, 0.6], [0.9, 0.1, 0.6], [0.9, 1.9, 0.6], [-0.9, 1.9, 0.6]], [[0, 1, 2], [0, 2, 3]], m)
    add(s)
    s.build()
    return s, p


@gpu
@pytest.mark.parametrize("integ,ts", MODES)
def test_hard_spot_inner_cone_equals_point_light(gpu_device, integ, ts):
    from oracle.oracle import Oracle
    gen = "cornell_dl" if integ == "dl" else "cornell_pt"
    col, power = (1.0, 0.9, 0.7), 6.0
    spot, p = _cornell_with(lambda s: s.add_spot_light(SPOT_FROM, SPOT_TO, col, power, cone_angle=80, blend=0.1),
                            gen, ts)
    point, _ = _cornell_with(lambda s: s.add_point_light(SPOT_FROM, col, power), gen, ts)
    assert _angles_to_axis(spot, SPOT_FROM, SPOT_TO).max() <= 80 * (1 - 0.1) - 5  # inside the inner cone (72 degrees)
    q = _mode(p, integ, ts)
    _, sums_o, cnt = Oracle(point).render(q)
    film, st = _render(gpu_device, spot, q)
    assert (st.closest_rays, st.shadow_rays) == (cnt["closest"], cnt["shadow"])
    assert (film.view(np.uint32) == sums_o.view(np.uint32)).all()


@gpu
@pytest.mark.parametrize("integ", ["dl", "pt"])
@pytest.mark.parametrize("kind", ["aimed_away", "photon_only"])
def test_spot_that_lights_nothing_equals_no_light(gpu_device, integ, kind):
    from oracle.oracle import Oracle
    gen = "cornell_dl" if integ == "dl" else "cornell_pt"
    if kind == "aimed_away":
        frm, to = (0.0, 1.0, -3.0), (0.0, 1.0, -10.0)
        add = lambda s: s.add_spot_light(frm, to, (1, 1, 1), 5.0, cone_angle=30, blend=0.2)
    else:
        frm, to = SPOT_FROM, SPOT_TO
        add = lambda s: s.add_spot_light(frm, to, (1, 1, 1), 5.0, cone_angle=80, blend=0.1, photon_only=True)
    spot, p = _cornell_with(add, gen, False)
    # Direct lighting sums every light (estimateAllDirectLight): the scene
    # without the spot is the yardstick. A path vertex chooses ONE of the
    # scene's lights and scales by their number (estimateOneDirectLight,
    # mcintegrator.cc:56-70), so a light that gives nothing still changes a
    # path-traced frame; there the yardstick is the oracle's frame with a
    # light it knows that gives nothing either, in the spot's place: a finite
    # directional light whose cylinder misses the scene (illuminate() false
    # everywhere: an empty slot and no shadow ray, like the spot).
    dark = lambda s: s.add_directional_light((0, 0, -1), (1, 1, 1), 5.0, infinite=False, from_=(50, 50, 50),
                                             radius=0.01)
    plain, _ = _cornell_with((lambda s: None) if integ == "dl" else dark, gen, False)
    ang = _angles_to_axis(spot, frm, to)
    assert ang.min() >= 30 + 5 if kind == "aimed_away" else ang.max() <= 72 - 5
    q = _mode(p, integ, 0)
    _, sums_o, cnt = Oracle(plain).render(q)
    film, st = _render(gpu_device, spot, q)
    assert (st.closest_rays, st.shadow_rays) == (cnt["closest"], cnt["shadow"])
    assert (film.view(np.uint32) == sums_o.view(np.uint32)).all()


# --- 4. blend region --------------------------------------------------------

@gpu
def test_blend_region_lies_between_nothing_and_the_point_light(gpu_device):
    frm, to, col, power = (0.0, 1.5, 0.0), (0.0, 0.0, 0.0), (1.0, 0.8, 0.6), 2.0
    a, p = _no_light_cornell(64, 64, "cornell_dl")
    a.add_spot_light(frm, to, col, power, cone_angle=30, blend=0.5)
    a.build()
    b, _ = _no_light_cornell(64, 64, "cornell_dl")
    b.add_point_light(frm, col, power)
    b.build()
    q = _params(p, integrator=A.YK_INTEGRATOR_DIRECT)
    fs, _ = _render(gpu_device, a, q)
    fp, _ = _render(gpu_device, b, q)
    fs, fp = fs[..., :3], fp[..., :3]
    assert np.isfinite(fs).all() and (fs >= 0).all() and (fs <= fp).all()
    lit = fp.sum(-1) > 0
    equal = lit & (fs == fp).all(-1)
    zero = lit & (fs.sum(-1) == 0)
    less = (fs.sum(-1) > 0) & (fs < fp).any(-1)
    print("blend sets:", equal.sum(), less.sum(), zero.sum())
    assert equal.any() and less.any() and zero.any()


# --- 5. form invariance -------------------------------------------------------

def _mixed_scene():
    """area light + soft spot (4 samples) + sphere light (4 samples)"""
    s = Scene()
    p = s.generate("cornell_pt", 64, 64)
    s.add_spot_light((0.6, 1.7, -0.6), (-0.2, 0.0, 0.3), (1, 0.9, 0.7), 4.0, cone_angle=40, blend=0.4,
                     soft_shadows=True, samples=4)
    s.add_sphere_light((-0.5, 0.6, -0.3), 0.15, (0.6, 0.8, 1.0), 6.0, samples=4)
    s.build()
    return s, _params(p, integrator=A.YK_INTEGRATOR_PATH, bounces=2)


_FORM_REF = {}
FORMS = list(itertools.product("01", repeat=4))


@gpu
@pytest.mark.parametrize("merge,split,small,diff", FORMS, ids=["".join(f) for f in FORMS])
def test_sampled_lights_form_invariance(gpu_device, monkeypatch, merge, split, small, diff):
    """YK_MERGE x YK_SPLIT x YK_SMALL x YK_DIFF: the same film bits and ray
    counts. The settings are read at upload and at render time, so each case
    sets them and uploads afresh (as the existing form tests do)."""
    s, q = _mixed_scene()
    if not _FORM_REF:
        for k in ("YK_MERGE", "YK_SPLIT", "YK_SMALL", "YK_DIFF"):
            monkeypatch.delenv(k, raising=False)
        film, st = _render(gpu_device, s, q)
        assert np.isfinite(film).all() and film[..., :3].max() > 0
        _FORM_REF["film"], _FORM_REF["rays"] = film, (st.closest_rays, st.shadow_rays)
    for k, v in (("YK_MERGE", merge), ("YK_SPLIT", split), ("YK_SMALL", small), ("YK_DIFF", diff)):
        monkeypatch.setenv(k, v)
    film, st = _render(gpu_device, s, q)
    assert (st.closest_rays, st.shadow_rays) == _FORM_REF["rays"]
    assert (film.view(np.uint32) == _FORM_REF["film"].view(np.uint32)).all()


@gpu
def test_sphere_light_shadow_ray_bounds(gpu_device):
    """One sphere light, direct lighting: at most `samples` shadow rays per
    camera sample (no BSDF half, so well inside the 2 * samples a light with
    one could take), at least one somewhere, and a lit, finite frame."""
    samples = 4
    s, p = _no_light_cornell(64, 64, "cornell_dl")
    s.add_sphere_light((0.0, 1.2, -0.2), 0.2, (1, 1, 1), 8.0, samples=samples)
    s.build()
    q = _params(p, integrator=A.YK_INTEGRATOR_DIRECT)
    film, st = _render(gpu_device, s, q)
    assert st.camera_samples == 64 * 64 * 4
    assert 1 <= st.shadow_rays <= samples * st.camera_samples
    assert np.isfinite(film).all() and film[..., :3].max() > 0


# --- slot cap, photon refusal, two handles ---------------------------------------

@gpu
@pytest.mark.parametrize("kind", ["spot", "sphere"])
def test_slot_cap_counts_the_new_lights(gpu_device, kind):
    """8192 shadow slots per shading point: the Cornell light's 8 plus a soft
    spot's 2 * 4093 or a sphere light's 8185 is one too many; the refusal
    leaves the resident scene as it was."""
    good, q = _mixed_scene()
    ref, _ = _render(gpu_device, good, q)
    for n, ok in ((4092, True), (4093, False)) if kind == "spot" else ((8184, True), (8185, False)):
        bad = Scene()
        bad.generate("cornell_pt", 16, 16)
        if kind == "spot":
            bad.add_spot_light((0, 1.9, 0), (0, 0, 0), soft_shadows=True, samples=n)
        else:
            bad.add_sphere_light((0, 1, 0), 0.1, samples=n)
        bad.build()
        if ok:
            gpu_device.upload(bad)
            gpu_device.upload(good)
            continue
        with pytest.raises(A.YkError) as e:
            gpu_device.upload(bad)
        assert e.value.code == A.YK_ERR_UNSUPPORTED
    film = gpu_device.new_film(q)
    gpu_device.render_shard(q, film)
    assert (film.cpu().numpy().view(np.uint32) == ref.view(np.uint32)).all()


@gpu
@pytest.mark.parametrize("kind", ["spot", "soft_spot", "sphere"])
def test_photon_build_refuses_spot_and_sphere_lights(gpu_device, kind):
    s = Scene()
    p = s.generate("cornell_pt", 32, 32)
    if kind == "sphere":
        s.add_sphere_light((0.3, 1.2, -0.2), 0.2, power=5.0)
    else:
        s.add_spot_light((0, 1.9, 0), (0, 0, 0), power=5.0, soft_shadows=kind == "soft_spot", samples=2)
    s.build()
    gpu_device.upload(s)
    for integ, caustic in ((A.YK_INTEGRATOR_PHOTON, A.YK_CAUSTIC_NONE), (A.YK_INTEGRATOR_PATH, A.YK_CAUSTIC_PHOTON)):
        q = _params(p, integrator=integ, caustic_type=caustic, width=32, height=32)
        q.photon.photons = q.photon.caustic_photons = 2000
        with pytest.raises(A.YkError) as e:
            gpu_device.photon_build(q)
        assert e.value.code == A.YK_ERR_UNSUPPORTED and "spot or sphere" in str(e.value)
    q = _params(p, integrator=A.YK_INTEGRATOR_DIRECT, width=32, height=32)
    film = gpu_device.new_film(q)
    gpu_device.render_shard(q, film)
    f = film.cpu().numpy()
    assert np.isfinite(f).all() and f[..., :3].max() > 0


@gpu
def test_render_multi_two_handles(gpu_device):
    """yk_render_multi over two handles on one GPU: the shard-order sum of the
    yk_render_shard films, bit for bit."""
    from core_amd.device import Device
    s, q = _mixed_scene()
    gpu_device.upload(s)
    acc = None
    for i in range(2):
        film = gpu_device.new_film(q)
        gpu_device.render_shard(q, film, i, 2)
        f = film.cpu().numpy()
        acc = f.copy() if acc is None else acc + f
    d2 = Device(0)
    try:
        d2.upload(s)
        out, st = Device.render_multi([gpu_device, d2], q)
    finally:
        d2.close()
    assert (out.view(np.uint32) == acc.view(np.uint32)).all()
    assert st.camera_samples == 64 * 64 * 4
