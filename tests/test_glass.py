"""The glass material (glassMat_t without dispersion, absorption or shader nodes: refraction, Fresnel
reflection, fake shadows) on the GPU path.

The oracle knows no glass and is never given one. The yardstick of the material is the float32 / float64
restatement in tests/glass_common.py, in source order; films are compared form against form. Helpers that are
not about the material (the probe binding, directions, the room, the render forms) are tests/test_glossy.py's
and tests/test_coated_glossy.py's.
"""
import ctypes as C
import os

import numpy as np
import pytest

from core_amd import _abi as A
from core_amd.scene import Scene
from tests import coated_common as K
from tests import glass_common as GS
from tests import glossy_common as G
from tests import test_coated_glossy as TC
from tests import test_glossy as TG

gpu = pytest.mark.gpu
F = np.float32
GLASS = 5
SPECULAR_FN, TRANSPARENCY_FN, ALPHA_FN = 5, 6, 7
_same = TG._same


def _bits(a):
    return TG._bits(a).tolist()

MATERIALS = {
    "plain": dict(),
    "ior1": dict(ior=1.0000001, mirror_color=(0.9, 1.0, 0.8), filter_color=(0.2, 0.9, 0.5), transmit_filter=0.3),
    "dense_fake": dict(ior=2.5, mirror_color=(1.0, 0.7, 0.5), filter_color=(0.9, 0.4, 0.3), transmit_filter=1.0,
                       fake_shadows=True),
    "bright": dict(ior=1.4, filter_color=(4.0, 3.0, 5.0), transmit_filter=1.0, fake_shadows=True),
}


def _want(kw):
    return GS.state_of(**{k: v for k, v in kw.items()})


# ---- CPU: interface ------------------------------------------------------------

def test_type_and_layout():
    """YK_MAT_GLASS = 5, 3 still refused; yk_material and yk_material_state keep every offset and their sizes
    (callers pin both), and glass's own members travel in yk_glass_params / yk_glass_state"""
    assert A.YK_MAT_GLASS == GLASS
    for cls, want in ((A.yk_material, TG.PARENT_MATERIAL), (A.yk_material_state, TG.PARENT_MATERIAL_STATE)):
        for name, off in want.items():
            assert getattr(cls, name).offset == off, (cls.__name__, name)
    assert C.sizeof(A.yk_material) == 128 and C.sizeof(A.yk_material_state) == 188
    assert A.yk_material_state.ior.offset == 184
    assert (A.yk_glass_params.filter_color.offset, A.yk_glass_params.fake_shadows.offset,
            A.yk_glass_params.dispersion_power.offset, C.sizeof(A.yk_glass_params)) == (0, 12, 16, 24)
    assert (A.yk_glass_state.filter_col.offset, A.yk_glass_state.fake_shadow.offset,
            C.sizeof(A.yk_glass_state)) == (0, 12, 16)
    s = Scene()
    assert s.add_material(type_=GLASS) == 0
    with pytest.raises(A.YkError) as e:
        s.add_material(type_=3)
    assert e.value.code == A.YK_ERR_UNSUPPORTED


def test_factory_state_equals_the_restatement():
    s = Scene()
    cases = list(MATERIALS.values()) + [dict(transmit_filter=0.0, filter_color=(0.3, 0.6, 0.9)),
                                        dict(transmit_filter=0.3, filter_color=(0.3, 0.6, 0.9), ior=1.0 / 3.0)]
    for kw in cases:
        s.add_material(type_=GLASS, **kw)
    for i, kw in enumerate(cases):
        st, gs, m, want = s.material_states()[i], s.glass_state(i), s.materials()[i], _want(kw)
        assert st.type == GLASS and m.type == GLASS and m.ior == kw.get("ior", 1.4)
        assert m.transmit_filter == F(kw.get("transmit_filter", 0.0))
        assert _bits(st.ior) == _bits(want["ior"])
        assert _bits(tuple(gs.filter_col)) == _bits(want["filter_col"]), (i, tuple(gs.filter_col), want["filter_col"])
        assert _bits(tuple(st.mirror_color)) == _bits(want["mirror_color"])
        assert gs.fake_shadow == want["fake_shadow"] and st.bsdf_flags == want["bsdf_flags"]
        assert st.ncomp == 0 and tuple(st.component) == (0, 0, 0, 0) and tuple(st.color) == (0, 0, 0)
    assert s.material_states()[0].bsdf_flags == GS.ALL_SPECULAR
    assert s.material_states()[2].bsdf_flags == GS.ALL_SPECULAR | GS.FILTER
    assert tuple(s.glass_state(0).filter_col) == (1, 1, 1) and tuple(s.glass_state(4).filter_col) == (1, 1, 1)
    assert _bits(tuple(s.glass_state(2).filter_col)) == _bits(F([0.9, 0.4, 0.3]))
    # the plain entry point gives a glass the factory's defaults
    m = s.materials()[1]
    mid = C.c_int32()
    A.check(A.lib().yk_scene_add_material(s.handle, C.byref(m), C.byref(mid)))
    assert _bits(tuple(s.glass_state(mid.value).filter_col)) == _bits(GS.state_of(transmit_filter=0.3)["filter_col"])
    assert s.glass_state(mid.value).fake_shadow == 0


def test_refusals():
    s = Scene()

    def code(**kw):
        with pytest.raises(A.YkError) as e:
            s.add_material(type_=GLASS, **kw)
        return e.value.code

    assert code(dispersion_power=0.05) == A.YK_ERR_UNSUPPORTED
    for bad in (float("nan"), float("inf")):
        assert code(ior=bad) == A.YK_ERR_ARG
        assert code(mirror_color=(1, bad, 1)) == A.YK_ERR_ARG
        assert code(filter_color=(bad, 1, 1)) == A.YK_ERR_ARG
        assert code(transmit_filter=bad) == A.YK_ERR_ARG
    assert len(s.materials()) == 0
    s.add_material(type_=GLASS, **MATERIALS["dense_fake"])
    s.add_material(type_=GLASS, **MATERIALS["ior1"])
    st_f, g_f, st_p, g_p = s.material_states()[0], s.glass_state(0), s.material_states()[1], s.glass_state(1)

    def scode(st, g, gkw=None, **kw):
        t = A.yk_material_state.from_buffer_copy(bytes(st))
        u = A.yk_glass_state.from_buffer_copy(bytes(g))
        for k, v in kw.items():
            setattr(t, k, v)
        for k, v in (gkw or {}).items():
            setattr(u, k, v)
        with pytest.raises(A.YkError) as e:
            s.add_material_state(t, u)
        return e.value.code

    assert scode(st_p, g_p, bsdf_flags=GS.ALL_SPECULAR | GS.VOLUMETRIC) == A.YK_ERR_UNSUPPORTED
    assert scode(st_f, g_f, bsdf_flags=GS.ALL_SPECULAR | GS.FILTER | GS.VOLUMETRIC) == A.YK_ERR_UNSUPPORTED
    assert scode(st_p, g_p, bsdf_flags=GS.ALL_SPECULAR | GS.DISPERSIVE) == A.YK_ERR_UNSUPPORTED
    for flags in (GS.ALL_SPECULAR | GS.FILTER, GS.SPECULAR | GS.REFLECT, GS.ALL_SPECULAR | GS.DIFFUSE,
                  GS.ALL_SPECULAR | 0x80, 0):
        assert scode(st_p, g_p, bsdf_flags=flags) == A.YK_ERR_ARG
    assert scode(st_f, g_f, bsdf_flags=GS.ALL_SPECULAR) == A.YK_ERR_ARG  # fake_shadow without BSDF_FILTER
    assert scode(st_f, g_f, gkw=dict(fake_shadow=2)) == A.YK_ERR_ARG
    assert scode(st_p, g_p, ior=float("nan")) == A.YK_ERR_ARG
    assert scode(st_p, g_p, mirror_color=A.f3(1, float("inf"), 1)) == A.YK_ERR_ARG
    assert scode(st_p, g_p, gkw=dict(filter_col=A.f3(float("nan"), 1, 1))) == A.YK_ERR_ARG
    t = A.yk_material_state.from_buffer_copy(bytes(st_p))
    t.type = 3
    with pytest.raises(A.YkError) as e:
        s.add_material_state(t)
    assert e.value.code == A.YK_ERR_UNSUPPORTED
    with pytest.raises(A.YkError) as e:  # the getter of another kind
        s2 = Scene()
        s2.add_material()
        s2.glass_state(0)
    assert e.value.code == A.YK_ERR_STATE


def test_state_round_trip():
    s = Scene()
    for kw in MATERIALS.values():
        s.add_material(type_=GLASS, **kw)
    n = len(MATERIALS)
    for i in range(n):
        st, g = s.material_states()[i], s.glass_state(i)
        j = s.add_material_state(st, g)
        assert j == n + i
        assert bytes(s.material_states()[j]) == bytes(st) and bytes(s.glass_state(j)) == bytes(g)
    j = s.add_material_state(s.material_states()[0])  # no glass state: filterCol 1, no fake shadows
    assert tuple(s.glass_state(j).filter_col) == (1, 1, 1) and s.glass_state(j).fake_shadow == 0


# ---- GPU: material functions -----------------------------------------------------

def _material_scene():
    s = Scene()
    for kw in MATERIALS.values():
        s.add_material(type_=GLASS, **kw)
    sd = s.add_material(color=(0.8, 0.7, 0.6), diffuse_reflect=0.9)
    s.add_mesh(np.array([[-1, 0, -1], [-1, 0, 1], [1, 0, 1], [1, 0, -1]], F), TG.QUAD, sd)
    s.add_point_light((0, 2, 0))
    s.set_camera((0, 2, -3), (0, 0, 0), (0, 3, -3), 16, 16)
    s.build()
    return s


@pytest.fixture(scope="module")
def material_device(gpu_device):
    s = _material_scene()
    gpu_device.upload(s)
    return gpu_device, s


def _glass_frames(rng, n, ior):
    """test_coated_glossy's frames (random, grazing, back-facing, N tilted off Ng so that wo.N < 0 with
    wo.Ng >= 0 and the reverse), with wo flipped inside for every other row, and a block of inside
    directions on and around the critical angle: sin(theta) = 1/ior (k = 0 in exact arithmetic), its float
    neighbours and +-1e-3, so that k comes out exactly 0, tiny negative and tiny positive."""
    N, Ng, NU, NV, wo, _ = TC._frames(rng, n)
    k = n // 8
    inside = np.arange(n) % 2 == 1
    inside[6 * k:7 * k] = False  # the tilted block keeps its construction
    wo[inside] = -wo[inside]
    blk = slice(2 * k, 3 * k)
    m = blk.stop - blk.start
    st = np.float64(1.0) / np.float64(ior) if ior > 1 else np.float64(ior)
    inward = ior > 1  # the dense side is inside for ior > 1
    # candidates within a few float steps of the critical angle, and +-1e-3; those whose k the restatement
    # rounds to exactly 0, to a tiny negative and to a tiny positive value come first
    c = 256 * m
    cn = np.repeat(N[blk], 256, axis=0).astype(np.float64)
    cu, cv = (np.repeat(a[blk], 256, axis=0).astype(np.float64) for a in (NU, NV))
    off = rng.uniform(-3e-7, 3e-7, c)
    off[::8] = np.where(np.arange(len(off[::8])) % 2 == 0, 1e-3, -1e-3)
    sin_t = np.clip(st + off, 0.0, 1.0)
    cos_t = np.sqrt(1.0 - sin_t * sin_t)
    phi = rng.uniform(0, 2 * np.pi, c)
    t = np.cos(phi)[:, None] * cu + np.sin(phi)[:, None] * cv
    w = (sin_t[:, None] * t + (-1.0 if inward else 1.0) * cos_t[:, None] * cn).astype(F)
    _, _, kk = GS.refract(cn.astype(F), w, F(ior))
    order = np.concatenate([np.flatnonzero(kk == 0)[: m // 4], np.flatnonzero((kk < 0) & (kk > -1e-6))[: m // 4],
                            np.flatnonzero((kk > 0) & (kk < 1e-6))[: m // 4], np.arange(0, c, 8)])[:m]
    N[blk] = cn[order].astype(F)
    NU[blk], NV[blk] = cu[order].astype(F), cv[order].astype(F)
    w = w[order]
    Ng[blk] = N[blk]
    wo[blk] = w
    return N, Ng, NU, NV, wo


MASKS = [GS.ALL_SPECULAR, GS.SPECULAR | GS.REFLECT, GS.SPECULAR | GS.TRANSMIT, GS.FILTER | GS.TRANSMIT,
         GS.DIFFUSE | GS.REFLECT, G.BSDF_ALL]


@gpu
@pytest.mark.parametrize("name", list(MATERIALS))
def test_sample_equals_the_restatement(material_device, monkeypatch, name):
    monkeypatch.setenv("YK_DEBUG_HOOKS", "1")
    dev, s = material_device
    mi = list(MATERIALS).index(name)
    M = GS.Glass(s.material_states()[mi], s.glass_state(mi))
    rng = np.random.default_rng(900 + mi)
    n = 12288
    N, Ng, NU, NV, wo = _glass_frames(rng, n, float(M.ior))
    outside, Nn, bent = GS.glass_normal(Ng, N, wo)
    ok, _, kk = GS.refract(Nn, wo, M.ior)
    assert bent.sum() > n // 64 and (bent & outside).any() and (bent & ~outside).any()
    assert (~ok).any() and ok.any() and (outside & ok).any() and (~outside & ok).any()
    # refract()'s k on both sides of the critical angle, within float steps of it. k is exactly 0 only where
    # fl(eta*eta*fl(1 - fl(c*c))) can be 1: a search over the 8000 floats around the critical cosine finds such
    # a c for IOR 1.0000001 and none for 1.4 or 2.5, so that case is asserted for the first alone.
    assert ((kk < 0) & (kk > -1e-5)).any() and ((kk > 0) & (kk < 1e-5)).any()
    if M.ior < 1.01:
        assert (kk == 0).sum() > 16
    # s1: random, then on and next to pKt
    Kr, Kt = K.fresnel(wo, Nn, M.ior)
    _, pKt = GS.p_widths(Kr, Kt)
    s1 = rng.random(n, dtype=F)
    q = n // 4
    s1[:q] = pKt[:q]
    s1[q:2 * q] = np.where(np.arange(q) % 2 == 0, np.nextafter(pKt[q:2 * q], F(-1)), np.nextafter(pKt[q:2 * q], F(2)))
    s1 = np.clip(s1, F(0.0), np.nextafter(F(1.0), F(0.0)))
    rows = TC._rows(N, Ng, NU, NV, wo)
    rows[:, 6], rows[:, 7] = s1, rng.random(n, dtype=F)
    picks = set()
    for flags in MASKS:
        rows[:, 9] = flags
        out = TG._probe(dev, mi, TG.SAMPLE, rows)
        want = GS.glass_sample(M, Ng, N, wo, s1, flags)
        what = f"sample {name} flags {flags:#x}"
        assert (out[:, 0] == want["ok"].astype(F)).all(), what
        _same(out[:, 1:4], want["wi"], what + " wi")
        _same(out[:, 4:7], want["col"], what + " col")
        _same(out[:, 7], want["pdf"], what + " pdf")
        _same(out[:, 8], want["W"], what + " W")
        assert (out[:, 9] == want["sflags"].astype(F)).all(), what
        picks |= set(np.unique(want["sflags"]).tolist())
        if flags == GS.DIFFUSE | GS.REFLECT:  # the early return: wi and W untouched, pdf 0, black
            assert not out.any()
        pdf = TG._probe(dev, mi, TG.PDF, rows)[:, 0]
        col = TG._probe(dev, mi, TG.EVAL, rows)[:, 0:3]
        assert not pdf.any() and not col.any()
    assert {0, GS.SPECULAR | GS.REFLECT, M.tm} <= picks


@gpu
@pytest.mark.parametrize("name", list(MATERIALS))
def test_specular_transparency_and_alpha_equal_the_restatement(material_device, monkeypatch, name):
    monkeypatch.setenv("YK_DEBUG_HOOKS", "1")
    dev, s = material_device
    mi = list(MATERIALS).index(name)
    M = GS.Glass(s.material_states()[mi], s.glass_state(mi))
    rng = np.random.default_rng(950 + mi)
    n = 8192
    N, Ng, NU, NV, wo = _glass_frames(rng, n, float(M.ior))
    rows = TC._rows(N, Ng, NU, NV, wo)
    for level in (1, 2, 3, 4):
        rows[:, 9] = level
        refl, d0, c0, refr, d1, c1 = GS.glass_specular(M, Ng, N, wo, level)
        rows[:, 8] = 0
        out = TG._probe(dev, mi, SPECULAR_FN, rows)
        assert (out[:, 0] == refl.astype(F)).all() and (out[:, 7] == refr.astype(F)).all(), (name, level)
        _same(out[:, 1:4], d0, f"getSpecular reflect dir {name} level {level}")
        _same(out[:, 4:7], c0, f"getSpecular reflect col {name} level {level}")
        rows[:, 8] = 1
        out = TG._probe(dev, mi, SPECULAR_FN, rows)
        assert (out[:, 0] == refr.astype(F)).all() and (out[:, 7] == refl.astype(F)).all(), (name, level)
        _same(out[:, 1:4], d1, f"getSpecular refract dir {name} level {level}")
        _same(out[:, 4:7], c1, f"getSpecular refract col {name} level {level}")
        outside = G.dot(Ng, wo) > 0
        assert (refl | refr).all() and (~refr).any() and (refl[~refr]).all()  # total inner reflection
        assert refl[outside].all() and (level < 3) == bool(refl[~outside & refr].all())
        assert level < 3 or not refl[~outside & refr].any()
    rows[:, 8] = 0
    t = TG._probe(dev, mi, TRANSPARENCY_FN, rows)[:, 0:3]
    _same(t, GS.glass_transparency(M, Ng, N, wo), f"getTransparency {name}")
    a = TG._probe(dev, mi, ALPHA_FN, rows)[:, 0]
    want = GS.glass_alpha(M, Ng, N, wo)
    _same(a, want, f"getAlpha {name}")
    assert (a >= 0).all() and (a <= 1).all()
    if name == "bright":
        assert (a == 0).sum() > n // 4 and (a > 0).any()  # clamped, and not (grazing, total reflection)
    else:
        assert (a > 0).all()


# ---- GPU: films --------------------------------------------------------------

SD = [dict(color=c, diffuse_reflect=d) for c, d in TG.DIFFUSE_PARTS]


def _glass_room(res, lights="dirac", **glass):
    return TG._room(res, SD[:4] + [dict(type_=GLASS, **glass)], lights)


def _sphere(center, radius, nu=12, nv=8):
    """a UV sphere: points, faces and the unit vertex normals that make it smooth"""
    pts = [(0.0, 1.0, 0.0)]
    for j in range(1, nv):
        th = np.pi * j / nv
        pts += [(np.sin(th) * np.cos(2 * np.pi * i / nu), np.cos(th), np.sin(th) * np.sin(2 * np.pi * i / nu))
                for i in range(nu)]
    pts.append((0.0, -1.0, 0.0))
    nrm = np.array(pts, np.float64)
    ring = lambda j, i: 1 + (j - 1) * nu + i % nu
    faces = [(0, ring(1, i + 1), ring(1, i)) for i in range(nu)]
    for j in range(1, nv - 1):
        for i in range(nu):
            faces += [(ring(j, i), ring(j, i + 1), ring(j + 1, i + 1)), (ring(j, i), ring(j + 1, i + 1), ring(j + 1, i))]
    faces += [(len(pts) - 1, ring(nv - 1, i), ring(nv - 1, i + 1)) for i in range(nu)]
    return (np.array(center)[None, :] + radius * nrm).astype(F), np.array(faces, np.int32), nrm.astype(F)


def _white_room(res, sphere=False, **glass):
    """TG._room's geometry under one white area light, so that every channel of an emitted photon is its
    maximum; sphere: a smooth glass sphere stands in the box's place"""
    s = Scene()
    m = [s.add_material(**kw) for kw in SD[:4] + [dict(type_=GLASS, **glass)]]
    s.add_mesh(np.array([[-2, 0, -2], [-2, 0, 2], [2, 0, 2], [2, 0, -2]], F), TG.QUAD, m[0])
    s.add_mesh(np.array([[-2, 0, 2], [-2, 3, 2], [2, 3, 2], [2, 0, 2]], F), TG.QUAD, m[1])
    s.add_mesh(np.array([[-2, 0, -2], [-2, 3, -2], [-2, 3, 2], [-2, 0, 2]], F), TG.QUAD, m[2])
    s.add_mesh(np.array([[2, 0, -2], [2, 0, 2], [2, 3, 2], [2, 3, -2]], F), TG.QUAD, m[3])
    b = np.array([[x, y, z] for x in (-0.7, 0.2) for y in (0.0, 1.0) for z in (-0.3, 0.6)], F)
    if sphere:
        pts, faces, nrm = _sphere((-0.2, 0.75, 0.1), 0.6)
        s.set_mesh_normals(s.add_mesh(pts, faces, m[4]), nrm, faces)
    else:
        s.add_mesh(b, TG.BOX_FACES, m[4])
    s.add_area_light((-0.5, 2.9, -0.5), (0.5, 2.9, -0.5), (-0.5, 2.9, 0.5), (1.0, 1.0, 1.0), 6.0, 2)
    s.set_camera((0.2, 1.6, -5.0), (0, 1.1, 0), (0.2, 2.6, -5.0), res, res, focal=1.6)
    s.build()
    return s


@gpu
def test_direct_lighting_recursion_levels(gpu_device):
    """raydepth 0: the glass box carries no light of its own (eval is black), so its pixels hold nothing that
    the same room without the box's recursion would not; black mirror and filter colours under raydepth 3
    give the film of raydepth 0 (every child is weighted by zero); with colours the recursion adds light and
    traces more rays; all of it repeats bit for bit."""
    s = _glass_room(16, ior=1.5)
    black = _glass_room(16, ior=1.5, mirror_color=(0, 0, 0), filter_color=(0, 0, 0), transmit_filter=1.0)
    q0 = TG._params(A.YK_INTEGRATOR_DIRECT, 16, 1, raydepth=0)
    q3 = TG._params(A.YK_INTEGRATOR_DIRECT, 16, 1, raydepth=3)
    f0, st0 = TG._render(gpu_device, s, q0)
    fb0, _ = TG._render(gpu_device, black, q0)
    fb3, stb3 = TG._render(gpu_device, black, q3)
    f3, st3 = TG._render(gpu_device, s, q3)
    f3b, st3b = TG._render(gpu_device, s, q3)
    assert np.isfinite(f3).all() and (f3.view(np.uint32) == f3b.view(np.uint32)).all()
    assert (st3.closest_rays, st3.shadow_rays) == (st3b.closest_rays, st3b.shadow_rays)
    assert (f0.view(np.uint32) == fb0.view(np.uint32)).all()
    assert (fb3[..., :3].view(np.uint32) == f0[..., :3].view(np.uint32)).all()
    assert st0.closest_rays == 16 * 16 and st3.closest_rays > st0.closest_rays == 256
    assert stb3.closest_rays == st3.closest_rays  # the children are traced, and weigh nothing
    glass_px = (f3[..., :3] != f0[..., :3]).any(axis=-1)
    assert glass_px.sum() > 8 and (f0[glass_px][:, :3] == 0).all(), "a glass pixel carries light without recursion"
    assert (f3[glass_px][:, :3].sum(axis=-1) > 0).all()


SLAB = dict(ior=1.5, mirror_color=(0.9, 1.0, 0.8), filter_color=(0.6, 0.9, 0.7), transmit_filter=0.8)


def _slab_scene(res, glass=True, **over):
    """a glass slab over a Lambert floor, a Lambert wall behind them, a point and a directional light;
    glass = False: the oracle's twin (the same geometry with shinydiffuse materials)"""
    s = Scene()
    floor = s.add_material(color=(0.8, 0.7, 0.6), diffuse_reflect=0.9)
    wall = s.add_material(**TC.WALL)
    g = s.add_material(type_=GLASS, **dict(SLAB, **over)) if glass else s.add_material(color=(0.5, 0.5, 0.5))
    s.add_mesh(np.array([[-3, 0, -3], [-3, 0, 3], [3, 0, 3], [3, 0, -3]], F), TG.QUAD, floor)
    s.add_mesh(np.array([[-3, 0, 3], [-3, 2.5, 3], [3, 2.5, 3], [3, 0, 3]], F), TG.QUAD, wall)
    b = np.array([[x, y, z] for x in (-1.2, 1.0) for y in (0.5, 0.8) for z in (-1.0, 1.1)], F)
    s.add_mesh(b, TG.BOX_FACES, g)
    s.add_point_light((0.4, 2.0, 0.3), (1.0, 0.9, 0.8), 6.0)
    s.add_directional_light((0.3, 1.0, -0.5), (0.9, 0.9, 1.0), 0.7)
    s.set_camera((0.2, 1.6, -4.0), (0, 0.5, 0), (0.2, 2.6, -4.0), res, res, focal=1.3)
    s.build()
    return s


def _restate(scene, twin, q):
    from oracle.oracle import Oracle
    orc = Oracle(twin)
    rays = orc.camera_rays(q.xstart, q.ystart, q.width, q.height, q.aa_samples)
    stats = dict(closest=0, shadow=0)
    col = GS.fold_direct(orc, scene, rays, 0, q.raydepth, stats)
    _, _, _, mat, _ = K.hit_points(orc, rays)
    idx = K.hit_points(orc, rays)[0]
    on_glass = np.zeros(len(rays), bool)
    on_glass[idx] = np.array([scene.material_states()[m].type == GLASS for m in mat], bool)
    return col, stats, on_glass


@gpu
@pytest.mark.parametrize("raydepth", [0, 1, 2])
def test_slab_under_direct_lighting_equals_the_fold_of_the_restated_children(gpu_device, raydepth):
    """Every pixel is the fold, in the fold's order, of the reflect and refract colours of the restated
    getSpecular over the oracle's camera hits, closest hits and isShadowed, bit for bit, ray counts
    included. With raydepth 0 the slab's pixels carry no light."""
    res = 16
    scene, twin = _slab_scene(res), _slab_scene(res, glass=False)
    q = TG._params(A.YK_INTEGRATOR_DIRECT, res, 1, raydepth=raydepth, tile_size=16)
    col, stats, on_glass = _restate(scene, twin, q)
    assert on_glass.sum() > res * res // 8 and (~on_glass).sum() > res * res // 8
    film, st = TG._render(gpu_device, scene, q)
    assert (st.closest_rays, st.shadow_rays) == (stats["closest"], stats["shadow"])
    own = TG.check_film(film, col, q)
    lit = own.reshape(-1, 3)[on_glass].sum(-1) > 0
    if raydepth == 0:
        assert stats["closest"] == res * res and not lit.any()
    else:
        # each slab pixel spawned a reflection and a refraction; at level 2 hits from inside branch again (only
        # the refracted rays can hit glass there, and there are more level-2 rays than those)
        assert stats["levels"][1] == 2 * on_glass.sum() and lit.sum() > on_glass.sum() // 2
        if raydepth == 2:
            assert stats["levels"][2] > on_glass.sum()


def _closed_box(glass=True):
    s = Scene()
    g = s.add_material(type_=GLASS, ior=1.5, filter_color=(0.9, 0.8, 0.7), transmit_filter=1.0) if glass \
        else s.add_material(color=(0.5, 0.5, 0.5))
    floor = s.add_material(color=(0.8, 0.7, 0.6), diffuse_reflect=0.9)
    b = np.array([[x, y, z] for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (-1.0, 1.0)], F)
    s.add_mesh(b, TG.BOX_FACES, g)
    s.add_mesh(np.array([[-9, -2, -9], [-9, -2, 9], [9, -2, 9], [9, -2, -9]], F), TG.QUAD, floor)
    s.add_mesh(np.array([[-9, -2, 4], [-9, 9, 4], [9, 9, 4], [9, -2, 4]], F), TG.QUAD, floor)
    s.add_point_light((3.0, 4.0, -1.0), (1, 1, 1), 30.0)
    s.set_camera((0.1, 0.05, -0.2), (0.3, -0.1, 1.0), (0.1, 1.05, -0.2), 16, 16, focal=0.7)
    s.build()
    return s


@gpu
def test_ray_level_rule_inside_a_closed_box(gpu_device):
    """A camera inside a closed glass box, raydepth 4: every glass hit up to the way out is from inside, so
    the Fresnel reflection is followed only below ray level 3 (total inner reflection aside). The ray count
    equals the restated tree's node count, level by level below the full binary tree's, and the film is the
    restated fold."""
    scene, twin = _closed_box(), _closed_box(glass=False)
    q = TG._params(A.YK_INTEGRATOR_DIRECT, 16, 1, raydepth=4, tile_size=16)
    col, stats, on_glass = _restate(scene, twin, q)
    assert on_glass.all()
    lv = stats["levels"]
    # levels 1 and 2 branch in two unless the reflection is total; from level 3 on a hit has one child at most
    assert lv[0] == 256 and 256 < lv[1] <= 512 and lv[1] // 2 < lv[2] <= 2 * lv[1]
    assert 0 < lv[4] <= lv[3] <= lv[2] and stats["closest"] < 256 * 31
    film, st = TG._render(gpu_device, scene, q)
    assert (st.closest_rays, st.shadow_rays) == (stats["closest"], stats["shadow"])
    own = TG.check_film(film, col, q)
    assert (own.sum(-1) > 0).sum() > 64
    # one level less and one more give other counts: the rule sits at the level after the increment
    q3 = TG._params(A.YK_INTEGRATOR_DIRECT, 16, 1, raydepth=3, tile_size=16)
    _, stats3, _ = _restate(scene, twin, q3)
    _, st3 = TG._render(gpu_device, scene, q3)
    assert st3.closest_rays == stats3["closest"] == stats["closest"] - lv[4]


def _pane_scene(fake):
    s = Scene()
    floor = s.add_material(color=(0.8, 0.8, 0.8), diffuse_reflect=0.9)
    g = s.add_material(type_=GLASS, ior=1.5, filter_color=(0.9, 0.5, 0.3), transmit_filter=0.8, fake_shadows=bool(fake))
    s.add_mesh(np.array([[-2, 0, -2], [-2, 0, 2], [2, 0, 2], [2, 0, -2]], F), TG.QUAD, floor)
    if fake is not None:
        s.add_mesh(np.array([[-0.6, 1, -0.6], [-0.6, 1, 0.6], [0.6, 1, 0.6], [0.6, 1, -0.6]], F), TG.QUAD, g)
    s.add_point_light((0.0, 2.0, 0.0), (1, 1, 1), 4.0)
    s.set_camera((0, 3.0, -3.0), (0, 0, 0), (0, 4.0, -2.0), 16, 16, focal=1.2)
    s.build()
    return s


@gpu
def test_fake_shadows(gpu_device):
    """isShadowed(.., maxDepth 2, filt) through a glass pane: Kt*filterCol of the crossing, bit for bit; the
    same rays are occluded without fake shadows; the lit film lies between the occluded and the open one."""
    rng = np.random.default_rng(77)
    n = 4096
    P = np.stack([rng.uniform(-0.25, 0.25, n), np.full(n, 0.0), rng.uniform(-0.25, 0.25, n)], 1).astype(F)
    P[: n // 2] = np.stack([rng.uniform(-1.9, 1.9, n // 2), np.zeros(n // 2), rng.uniform(-1.9, 1.9, n // 2)], 1)
    L = F([0.0, 2.0, 0.0])
    d = (L[None, :] - P).astype(F)
    dist = np.sqrt(G.dot(d, d)).astype(F)
    d = (d * (F(1.0) / dist)[:, None]).astype(F)
    rays = np.zeros((n, 8), F)
    rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7] = P, d, F(0.0005), dist
    # through the pane: the point where the ray meets y = 1
    t = (1.0 - P[:, 1].astype(np.float64)) / d[:, 1].astype(np.float64)
    X = P.astype(np.float64) + t[:, None] * d.astype(np.float64)
    through = (np.abs(X[:, 0]) < 0.59) & (np.abs(X[:, 2]) < 0.59)
    edge = (np.abs(np.abs(X[:, 0]) - 0.6) < 0.01) | (np.abs(np.abs(X[:, 2]) - 0.6) < 0.01)
    assert through.sum() > n // 4 and (~through & ~edge).sum() > n // 8
    s = _pane_scene(True)
    gpu_device.upload(s)
    occ, filt = gpu_device.trace_shadow_filtered(gpu_device.rays_to_device(rays), 2)
    occ, filt = occ.cpu().numpy().astype(bool), filt.cpu().numpy()
    M = GS.Glass(s.material_states()[1], s.glass_state(1))
    Ng = np.broadcast_to(F([0, 1, 0]), (n, 3)).astype(F)
    # the pane's geometric normal as the scene holds it
    want = GS.glass_transparency(M, Ng, Ng, d)
    wantn = GS.glass_transparency(M, -Ng, -Ng, d)
    assert _bits(want) == _bits(wantn)  # fresnel() face-forwards: the normal's sign is immaterial
    assert not occ[through].any() and not occ[~through & ~edge].any()
    _same(filt[through], want[through], "filter through the pane")
    assert (filt[~through & ~edge] == 1).all()
    assert (want[through] > 0).all() and (want[through] < 1).all()
    plain = _pane_scene(False)
    gpu_device.upload(plain)
    occ2, _ = gpu_device.trace_shadow_filtered(gpu_device.rays_to_device(rays), 2)
    occ2 = occ2.cpu().numpy().astype(bool)
    assert occ2[through].all() and not occ2[~through & ~edge].any()
    # films: floor pixels under the pane
    q = TG._params(A.YK_INTEGRATOR_DIRECT, 16, 1, raydepth=0, transp_shadows=1, shadow_depth=2)
    f_fake, _ = TG._render(gpu_device, s, q)
    f_occ, _ = TG._render(gpu_device, plain, q)
    f_open, _ = TG._render(gpu_device, _pane_scene(None), q)
    assert np.isfinite(f_fake).all()
    # floor pixels in the pane's shadow, from the occluded and the open film and the geometry alone: black with
    # an opaque pane, lit without one, and the camera ray does not meet the pane itself (glass is black at
    # raydepth 0)
    from oracle.oracle import Oracle
    cr = Oracle(_pane_scene(None)).camera_rays(0, 0, 16, 16, 1)
    tp = (1.0 - cr[:, 1].astype(np.float64)) / cr[:, 4].astype(np.float64)
    Xp = cr[:, 0:3].astype(np.float64) + tp[:, None] * cr[:, 3:6].astype(np.float64)
    sees_pane = ((tp > 0) & (np.abs(Xp[:, 0]) < 0.65) & (np.abs(Xp[:, 2]) < 0.65)).reshape(16, 16)
    under = (f_occ[..., :3].sum(-1) == 0) & (f_open[..., :3].sum(-1) > 0) & ~sees_pane
    assert under.sum() >= 4 and sees_pane.sum() >= 4
    for c in range(3):
        assert (f_fake[under][:, c] > f_occ[under][:, c]).all() and (f_fake[under][:, c] < f_open[under][:, c]).all()


def _pt_scene():
    return _glass_room(16, "area", ior=1.5, filter_color=(0.9, 0.95, 1.0), transmit_filter=0.5), \
        TG._params(A.YK_INTEGRATOR_PATH, 16, 2, raydepth=2, caustic_type=A.YK_CAUSTIC_PATH)


@pytest.fixture(scope="module")
def pt_reference(gpu_device):
    saved = {k: os.environ.pop(k) for k in TG.FORM_KEYS if k in os.environ}
    try:
        s, q = _pt_scene()
        film, st = TG._render(gpu_device, s, q)
        assert np.isfinite(film).all() and film[..., :3].max() > 0
        again, st2 = TG._render(gpu_device, s, q)
        assert (again.view(np.uint32) == film.view(np.uint32)).all(), "a repeated call differs"
        assert (st2.closest_rays, st2.shadow_rays) == (st.closest_rays, st.shadow_rays)
        acc = None
        for i in range(2):
            f, _ = TG._render(gpu_device, s, q, i, 2)
            acc = f.copy() if acc is None else acc + f
        assert (acc.view(np.uint32) == film.view(np.uint32)).all(), "two shards differ from one"
        from core_amd.device import Device
        other = Device(0)
        try:
            f2, _ = TG._render(other, s, q)
        finally:
            other.close()
        assert (f2.view(np.uint32) == film.view(np.uint32)).all(), "a second device handle differs"
    finally:
        os.environ.update(saved)
    return film, (st.closest_rays, st.shadow_rays)


@gpu
@pytest.mark.parametrize("form", range(len(TG.FORMS)),
                         ids=["-".join(f"{k}{v}" for k, v in f.items()) or "default" for f in TG.FORMS])
def test_path_tracing_form_invariance(gpu_device, monkeypatch, pt_reference, form):
    s, q = _pt_scene()
    for k in TG.FORM_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in TG.FORMS[form].items():
        monkeypatch.setenv(k, v)
    film, st = TG._render(gpu_device, s, q)
    assert (st.closest_rays, st.shadow_rays) == pt_reference[1]
    assert (film.view(np.uint32) == pt_reference[0].view(np.uint32)).all()


def _photon_params(integ, res, **ph):
    q = TG._params(integ, res, 1)
    q.photon.photons = 20000
    q.photon.caustic_photons = 20000
    q.photon.search = 32
    q.photon.caustic_mix = 32
    for k, v in ph.items():
        setattr(q.photon, k, v)
    return q


@gpu
def test_photon_caustics(gpu_device):
    """A smooth glass sphere (IOR 1.5) in the Lambert room, whose interpolated normals differ from the
    triangles' (the bent-normal branch): photons that glass's specular picks bent or mirrored are
    stored as caustic photons at the next diffuse hit. None with bounces = 0 (an equality); with bounces 3 the
    map is non-empty, finite, repeats bit for bit and is the same map under the three integrators; no photon is
    brighter than the emitted one when filter and mirror colours are <= 1."""
    s = _white_room(16, sphere=True, ior=1.5, filter_color=(0.9, 0.8, 1.0), transmit_filter=1.0, mirror_color=(1.0, 0.9, 0.8))
    gpu_device.upload(s)
    q0 = _photon_params(A.YK_INTEGRATOR_PHOTON, 16, bounces=0, final_gather=0)
    assert gpu_device.photon_build(q0).caustic_photons == 0
    maps, paths = [], []
    for integ, extra in ((A.YK_INTEGRATOR_PHOTON, {}), (A.YK_INTEGRATOR_PHOTON, {}),
                         (A.YK_INTEGRATOR_PATH, dict(caustic_type=A.YK_CAUSTIC_PHOTON)),
                         (A.YK_INTEGRATOR_DIRECT, dict(dl_caustics=1))):
        q = _photon_params(integ, 16, bounces=3, final_gather=0)
        for k, v in extra.items():
            setattr(q, k, v)
        gpu_device.upload(s)
        info = gpu_device.photon_build(q)
        cmap = gpu_device.photon_map(A.YK_PHOTON_MAP_CAUSTIC)
        print("caustic photons stored with bounces 3:", info.caustic_photons)
        assert info.caustic_photons > 0 and len(cmap) == info.caustic_photons and np.isfinite(cmap).all()
        maps.append(cmap)
        paths.append(info.caustic_paths)
    assert (maps[0].view(np.uint32) == maps[1].view(np.uint32)).all(), "a repeated build differs"
    assert maps[2].shape == maps[3].shape and (maps[2].view(np.uint32) == maps[3].view(np.uint32)).all()
    # the emitted photon colour bounds every stored one, channel by channel (colours are the map's last three columns)
    gpu_device.upload(s)
    qd = _photon_params(A.YK_INTEGRATOR_PHOTON, 16, bounces=0, final_gather=0)
    dinfo = gpu_device.photon_build(qd)
    # a scatter multiplies by W and the colour and divides by the survival probability, which keeps the largest
    # channel: three roundings of 2^-24 each per bounce, three bounces, so 1e-6 relative covers the rounding
    emitted = gpu_device.photon_map(A.YK_PHOTON_MAP_DIFFUSE)[:, 6:9].astype(np.float64).max(axis=0)
    assert dinfo.diffuse_photons > 0 and (emitted > 0).all()
    assert (maps[0][:, 6:9].astype(np.float64) <= emitted[None, :] * (1 + 1e-6)).all()
    for fg in (0, 1):
        q = _photon_params(A.YK_INTEGRATOR_PHOTON, 16, bounces=3, final_gather=fg, fg_samples=2, fg_bounces=2)
        gpu_device.upload(s)
        gpu_device.photon_build(q)
        film = gpu_device.new_film(q)
        gpu_device.render_shard(q, film)
        f = film.cpu().numpy()
        assert np.isfinite(f).all() and f[..., :3].max() > 0


def _kind(dev):
    k = C.c_int32(-1)
    A.check(A.lib().yk_debug_shading_kind(dev._p, C.byref(k)))
    return k.value


@gpu
def test_no_cross_talk(gpu_device, monkeypatch):
    """shinydiffuse, glossy-only and coated scenes render the same bits on a handle before and after a glass
    scene, and report the variants they reported before. yk_debug_shading_kind tells the diffuse-only
    variant from the others only; that the glossy and the coated scene run their own table rows again is
    shown by their films and ray counts, which a glass-level kernel would reproduce only by computing
    the same thing."""
    monkeypatch.setenv("YK_DEBUG_HOOKS", "1")
    q = TG._params(A.YK_INTEGRATOR_PATH, 16, 1)
    scenes = [TG._room(16, SD, "area"),
              TG._room(16, SD[:4] + [dict(type_=A.YK_MAT_GLOSSY, **TG.MATERIALS["iso_diff"])], "area"),
              TG._room(16, SD[:4] + [dict(type_=A.YK_MAT_COATED_GLOSSY, **TC.MATERIALS["iso_diff_on"])], "area")]
    before = []
    for sc in scenes:
        f, st = TG._render(gpu_device, sc, q)
        before.append((f, st.closest_rays, st.shadow_rays, _kind(gpu_device)))
    gs, gq = _pt_scene()
    gf, _ = TG._render(gpu_device, gs, gq)
    assert (gf.view(np.uint32) != 0).any() and _kind(gpu_device) == 0
    for sc, (f0, c0, s0, k0) in zip(scenes, before):
        f, st = TG._render(gpu_device, sc, q)
        assert (f.view(np.uint32) == f0.view(np.uint32)).all() and (st.closest_rays, st.shadow_rays) == (c0, s0)
        assert _kind(gpu_device) == k0
    assert [b[3] for b in before] == [1, 0, 0]
