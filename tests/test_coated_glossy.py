"""The coated glossy material (coatedGlossyMat_t with as_diffuse: glossy's Blinn
or Ashikhmin-Shirley base under a perfectly specular dielectric coat with a
Fresnel weight) on the GPU path.

The oracle knows no glossy material and is never given one: it serves camera
rays, closest hits and isShadowed of the same geometry. The yardstick of the
material is the float32 restatement in tests/coated_common.py, in source order.
Helpers that are not about the material (the probe binding, the direction and
film helpers, the room) are tests/test_glossy.py's.
"""
import ctypes as C

import numpy as np
import pytest

from core_amd import _abi as A
from core_amd.scene import Scene
from tests import coated_common as K
from tests import glossy_common as G
from tests import test_glossy as TG

gpu = pytest.mark.gpu
F = np.float32
CG = 4  # YK_MAT_COATED_GLOSSY
SPECULAR_FN = 5  # YK_MATERIAL_PROBE_SPECULAR
_bits, _same = TG._bits, TG._same

# iso and aniso, with and without the diffuse base, one Oren-Nayar, IOR 1.0000001 (from 1) / 1.4 / 2.5
MATERIALS = {
    "iso": dict(color=(0.9, 0.8, 0.7), exponent=50.0, mirror_color=(0.9, 1.0, 0.8)),
    "iso_diff_ior1": dict(color=(0.9, 0.8, 0.7), exponent=200.0, glossy_reflect=0.3, diffuse_reflect=0.8,
                          diffuse_color=(0.2, 0.5, 0.9), ior=1.0),
    "iso_diff_on": dict(color=(0.6, 0.6, 0.9), exponent=20.0, glossy_reflect=0.3, diffuse_reflect=0.6,
                        diffuse_color=(0.8, 0.4, 0.3), diffuse_brdf="Oren-Nayar", sigma=0.4, ior=2.5,
                        mirror_color=(1.0, 0.7, 0.5)),
    "aniso": dict(color=(0.7, 0.9, 0.8), anisotropic=True, exp_u=10.0, exp_v=400.0, ior=2.5),
    "aniso_diff": dict(color=(0.7, 0.9, 0.8), anisotropic=True, exp_u=300.0, exp_v=8.0, glossy_reflect=0.3,
                       diffuse_reflect=0.7, diffuse_color=(0.9, 0.8, 0.2)),
}


def _full(kw):
    full = dict(color=(1, 1, 1), diffuse_color=(1, 1, 1), glossy_reflect=1.0, diffuse_reflect=0.0, exponent=50.0,
                anisotropic=False, exp_u=50.0, exp_v=50.0, diffuse_brdf="lambert", sigma=0.1, mirror_color=(1, 1, 1),
                ior=1.4)
    full.update(kw)
    return full


def _want_state(kw):
    f = _full(kw)
    return K.state_of(mirror_color=f["mirror_color"], ior=f["ior"], color=f["color"], diffuse_color=f["diffuse_color"],
                      glossy_reflect=f["glossy_reflect"], diffuse_reflect=f["diffuse_reflect"], exponent=f["exponent"],
                      anisotropic=f["anisotropic"], exp_u=f["exp_u"], exp_v=f["exp_v"],
                      oren_nayar=f["diffuse_brdf"] == "Oren-Nayar", sigma=f["sigma"])


# ---- CPU: interface ------------------------------------------------------------

def test_type_values():
    assert A.YK_MAT_COATED_GLOSSY == CG
    s = Scene()
    assert s.add_material(type_=CG) == 0
    with pytest.raises(A.YkError) as e:  # 3 stays unassigned
        s.add_material(type_=3)
    assert e.value.code == A.YK_ERR_UNSUPPORTED
    st = s.material_states()[0]
    st.type = 3
    with pytest.raises(A.YkError) as e:
        s.add_material_state(st)
    assert e.value.code == A.YK_ERR_UNSUPPORTED


def test_layout():
    """yk_material gained nothing; yk_material_state gained `ior` at its end, zero for the other kinds"""
    assert C.sizeof(A.yk_material) == 128 and A.yk_material.exp_v.offset == 120
    for cls, want in ((A.yk_material, TG.PARENT_MATERIAL), (A.yk_material_state, TG.PARENT_MATERIAL_STATE)):
        for name, off in want.items():
            assert getattr(cls, name).offset == off, (cls.__name__, name)
    glossy_tail = dict(gloss_color=128, diff_color=140, exponent=152, exp_u=156, exp_v=160, reflectivity=164,
                       m_diffuse=168, as_diffuse=172, with_diffuse=176, anisotropic=180)
    for name, off in glossy_tail.items():
        assert getattr(A.yk_material_state, name).offset == off, name
    assert A.yk_material_state.ior.offset == 184 and C.sizeof(A.yk_material_state) == 188
    s = Scene()
    s.add_material(color=(0.1, 0.2, 0.3), ior=1.7, fresnel_effect=True, specular_reflect=0.5)
    s.add_material(type_=A.YK_MAT_GLOSSY, **TG.MATERIALS["iso_diff"])
    for st in s.material_states():
        assert st.ior == 0.0


def test_add_material_accepts_and_refuses():
    s = Scene()
    for kw in MATERIALS.values():
        s.add_material(type_=CG, **kw)

    def code(**kw):
        with pytest.raises(A.YkError) as e:
            s.add_material(type_=CG, **kw)
        return e.value.code

    assert code(as_diffuse=False) == A.YK_ERR_UNSUPPORTED
    for bad in (float("nan"), float("inf")):
        assert code(color=(1, bad, 1)) == A.YK_ERR_ARG
        assert code(diffuse_color=(bad, 1, 1)) == A.YK_ERR_ARG
        assert code(mirror_color=(1, 1, bad)) == A.YK_ERR_ARG
        assert code(glossy_reflect=bad) == A.YK_ERR_ARG
        assert code(diffuse_reflect=bad) == A.YK_ERR_ARG
        assert code(exponent=bad) == A.YK_ERR_ARG
        assert code(ior=bad) == A.YK_ERR_ARG
        assert code(anisotropic=True, exp_u=bad) == A.YK_ERR_ARG
        assert code(anisotropic=True, exp_v=bad) == A.YK_ERR_ARG
    # the state entry point: the same rules, and the constructor's flags exactly
    n = len(MATERIALS)
    st = s.material_states()[1]
    assert s.add_material_state(st) == n

    def scode(**kw):
        t = A.yk_material_state.from_buffer_copy(bytes(st))
        for k, v in kw.items():
            if k == "comp_flags":
                for i, x in enumerate(v):
                    t.comp_flags[i] = x
            else:
                setattr(t, k, v)
        with pytest.raises(A.YkError) as e:
            s.add_material_state(t)
        return e.value.code

    assert scode(as_diffuse=0) == A.YK_ERR_UNSUPPORTED
    assert scode(reflectivity=float("nan")) == A.YK_ERR_ARG
    assert scode(ior=float("inf")) == A.YK_ERR_ARG
    assert scode(mirror_color=A.f3(1, float("nan"), 1)) == A.YK_ERR_ARG
    for flags in (K.DIFF, K.SPEC, K.SPEC | K.DIFF | 0x40, K.SPEC | K.DIFF | 0x80, K.SPEC | K.DIFF | 0x2):
        assert scode(bsdf_flags=flags) == A.YK_ERR_ARG
    assert scode(ncomp=2) == A.YK_ERR_ARG  # this one has a diffuse base: nBSDF is 3
    assert scode(comp_flags=(K.SPEC, K.DIFF, 0, 0)) == A.YK_ERR_ARG
    assert scode(comp_flags=(K.DIFF, K.SPEC, K.DIFF, 0)) == A.YK_ERR_ARG
    st0 = s.material_states()[0]  # no diffuse base: nBSDF 2, cFlags[C_DIFFUSE] = BSDF_NONE
    t = A.yk_material_state.from_buffer_copy(bytes(st0))
    t.ncomp = 3
    with pytest.raises(A.YkError) as e:
        s.add_material_state(t)
    assert e.value.code == A.YK_ERR_ARG


def test_parameters_and_host_state_equal_the_restatement():
    s = Scene()
    for kw in MATERIALS.values():
        s.add_material(type_=CG, **kw)
    s.add_material(type_=CG, ior=float(np.nextafter(F(1.0), F(2.0))))  # not 1: kept
    s.add_material(type_=CG, ior=1.0 + 1e-12)                           # a double that is not 1.f: kept, rounds to 1
    mats, states = s.materials(), s.material_states()
    for i, (name, kw) in enumerate(MATERIALS.items()):
        m, st, f = mats[i], states[i], _full(kw)
        assert m.type == CG and m.as_diffuse == 1 and m.ior == f["ior"]
        assert tuple(m.mirror_color) == tuple(F(c) for c in f["mirror_color"])
        assert tuple(m.color) == tuple(F(c) for c in f["color"])
        assert (m.glossy_reflect, m.diffuse_reflect, m.exponent) == tuple(
            F(f[k]) for k in ("glossy_reflect", "diffuse_reflect", "exponent"))
        for k, v in _want_state(kw).items():
            got = getattr(st, k)
            got = tuple(got) if hasattr(got, "__len__") else got
            if isinstance(v, (np.floating, float)):
                assert _bits(got) == _bits(v), (name, k, got, v)
            else:
                assert got == v, (name, k, got, v)
        assert tuple(st.component) == (0, 0, 0, 0) and tuple(st.emit_color) == (0, 0, 0)
        j = s.add_material_state(st)
        assert bytes(s.material_states()[j]) == bytes(st)
        # pDiffuse (coatedglossy.cc:116) of the restatement from the state, against the expression in float32
        M = K.Coated(st)
        with np.errstate(all="ignore"):
            x = F(1.0) - (F(f["glossy_reflect"]) / (F(f["glossy_reflect"]) + (F(1.0) - F(f["glossy_reflect"])) * F(f["diffuse_reflect"])))
        assert _bits(M.pD) == _bits(x if x < F(0.6) else F(0.6))
    flags = {n: st.bsdf_flags for n, st in zip(MATERIALS, states)}
    assert set(flags.values()) == {K.BSDF_SPECULAR | K.BSDF_REFLECT | K.BSDF_DIFFUSE}
    assert [st.ncomp for st in states[:5]] == [2, 3, 3, 2, 3]
    assert tuple(states[0].comp_flags) == (K.SPEC, K.DIFF, 0, 0) and tuple(states[1].comp_flags) == (K.SPEC, K.DIFF, K.DIFF, 0)
    # the factory's `if(ior == 1.f) ior = 1.0000001f`
    assert _bits(states[1].ior) == _bits(np.nextafter(F(1.0), F(2.0))) == _bits(F(1.0000001))
    assert _bits(states[5].ior) == _bits(np.nextafter(F(1.0), F(2.0)))
    assert _bits(states[6].ior) == _bits(F(1.0))
    assert _bits(states[0].ior) == _bits(F(1.4))


def test_python_defaults_are_the_factory_defaults():
    s = Scene()
    s.add_material(type_=CG)
    m = s.materials()[0]
    assert (m.ior, m.exponent, m.glossy_reflect, m.diffuse_reflect, m.as_diffuse) == (1.4, 50.0, 1.0, 0.0, 1)
    assert tuple(m.mirror_color) == (1, 1, 1)
    s.add_material()  # shinydiffuse keeps its own IOR default
    assert s.materials()[1].ior == 1.33


# ---- GPU: material functions -----------------------------------------------------

def _material_scene():
    s = Scene()
    for kw in MATERIALS.values():
        s.add_material(type_=CG, **kw)
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


def _frames(rng, n):
    """N, Ng, NU, NV, wo, wl: test_glossy's directions (random, createCS's flat branch, grazing, back-facing,
    mirror), then a block where the shading normal is tilted off the geometric one so that wo.N < 0 with
    wo.Ng >= 0 (and the reverse)"""
    N, wo, wl = TG._directions(rng, n)
    Ng = N.copy()
    k = n // 8
    sl = slice(6 * k, 7 * k)
    NUg, _ = G.create_cs(Ng)
    N[sl] = TG._unit(Ng[sl] + 0.6 * NUg[sl])
    # wo between the two planes: just above Ng's, below N's (half of them), and the reverse
    t = rng.uniform(0.02, 0.3, size=(k, 1)).astype(F)
    a = TG._unit(-NUg[sl] + t * Ng[sl])
    b = TG._unit(NUg[sl] * 0.9 - t * Ng[sl])
    wo[sl] = np.where((np.arange(k) % 2 == 0)[:, None], a, b)
    NU, NV = G.create_cs(N)
    return N, Ng, NU, NV, wo, wl


def _rows(N, Ng, NU, NV, wo):
    rows = np.zeros((len(N), 20), F)
    rows[:, 0:3], rows[:, 3:6], rows[:, 10:13], rows[:, 13:16], rows[:, 16:19], rows[:, 19] = N, wo, Ng, NU, NV, 2
    return rows


FLAG_CASES = [K.BSDF_ALL, K.DIFF, K.SPEC, G.BSDF_GLOSSY | 0x20]  # the last matches nothing


@gpu
@pytest.mark.parametrize("name", list(MATERIALS))
def test_eval_pdf_fresnel_and_specular_equal_the_restatement(material_device, monkeypatch, name):
    monkeypatch.setenv("YK_DEBUG_HOOKS", "1")
    dev, s = material_device
    mi = list(MATERIALS).index(name)
    M = K.Coated(s.material_states()[mi])
    rng = np.random.default_rng(300 + mi)
    n = 2048
    N, Ng, NU, NV, wo, wl = _frames(rng, n)
    sl = slice(6 * (n // 8), 7 * (n // 8))
    assert ((G.dot(wo[sl], N[sl]) < 0) & (G.dot(wo[sl], Ng[sl]) >= 0)).sum() > n // 32
    rows = _rows(N, Ng, NU, NV, wo)
    rows[:, 6:9] = wl
    for flags in FLAG_CASES:
        rows[:, 9] = flags
        col = TG._probe(dev, mi, TG.EVAL, rows)[:, 0:3]
        _same(col, K.coated_eval(M, Ng, N, NU, NV, wo, wl, flags), f"eval {name} flags {flags:#x}")
        pdf = TG._probe(dev, mi, TG.PDF, rows)[:, 0]
        _same(pdf, K.coated_pdf(M, Ng, N, NU, NV, wo, wl, flags), f"pdf {name} flags {flags:#x}")
        if flags == K.BSDF_ALL:
            assert (col > 0).any() and (pdf > 0).any()
    for level in (1, 5, 6):
        rows[:, 9] = level
        out = TG._probe(dev, mi, SPECULAR_FN, rows)
        refl, d, c = K.coated_specular(M, Ng, N, wo, level)
        assert (out[:, 0] == refl.astype(F)).all() and refl.all() == (level <= 5)
        _same(out[:, 1:4], d, f"getSpecular dir {name} level {level}")
        _same(out[:, 4:7], c, f"getSpecular col {name} level {level}")
        Kr, Kt = K.fresnel(wo, G.face_forward(Ng, N, wo), M.ior)
        _same(out[:, 7], Kr, f"fresnel Kr {name}")
        _same(out[:, 8], Kt, f"fresnel Kt {name}")
    assert np.isfinite(Kr).all() and (Kr >= 0).all() and Kr.max() > 0 and (Kt >= 0).all()
    assert M.ior < 1.01 or Kr.max() > 0.5  # grazing directions: the coat takes nearly everything
    # the grazing correction and the bent normal both occur
    refl, d, _ = K.coated_specular(M, Ng, N, wo, 1)
    assert (np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1) < 1e-3).all()


def _sample_numbers(rng, n, M, N, Ng, wo):
    """s1 random, then on and next to every component boundary of BSDF_ALL's pick (per row: the
    boundaries depend on Kr), s2 random with 0 and 1 - ulp"""
    s1 = rng.random(n, dtype=F)
    s2 = rng.random(n, dtype=F)
    below = np.nextafter(F(1.0), F(0.0))
    Kr, Kt = K.fresnel(wo, G.face_forward(Ng, N, wo), M.ior)
    comps, w = K.widths(M, Kr, Kt, K.BSDF_ALL)
    tot = np.zeros(n, F)
    vals = []
    for x in w:
        tot = (tot + x).astype(F)
        vals.append(tot)
    with np.errstate(all="ignore"):
        vals = [(v * (F(1.0) / tot)).astype(F) for v in vals]
    k = n // 8
    for j, v in enumerate(vals[:-1]):
        a = slice((2 * j) * k // 2, (2 * j + 1) * k // 2)
        s1[a] = v[a]
        b = slice((2 * j + 1) * k // 2, (2 * j + 2) * k // 2)
        s1[b] = np.where(np.arange(b.stop - b.start) % 2 == 0, np.nextafter(v[b], F(-1)), np.nextafter(v[b], F(2)))
    s1 = np.clip(np.nan_to_num(s1), F(0.0), below)
    s2[3 * k:4 * k] = F(0.0)
    s2[4 * k:5 * k] = below
    return s1, s2


@gpu
@pytest.mark.parametrize("name", list(MATERIALS))
def test_sample_equals_the_restatement(material_device, monkeypatch, name):
    monkeypatch.setenv("YK_DEBUG_HOOKS", "1")
    dev, s = material_device
    mi = list(MATERIALS).index(name)
    M = K.Coated(s.material_states()[mi])
    trig = TG.DeviceTrig(dev)
    rng = np.random.default_rng(400 + mi)
    n = 2048
    N, Ng, NU, NV, wo, _ = _frames(rng, n)
    s1, s2 = _sample_numbers(rng, n, M, N, Ng, wo)
    rows = _rows(N, Ng, NU, NV, wo)
    rows[:, 6], rows[:, 7] = s1, s2
    for flags in FLAG_CASES:
        rows[:, 9] = flags
        out = TG._probe(dev, mi, TG.SAMPLE, rows)
        want = K.coated_sample(M, Ng, N, NU, NV, wo, s1, s2, flags, trig)
        what = f"sample {name} flags {flags:#x}"
        assert (out[:, 0] == want["ok"].astype(F)).all(), what
        _same(out[:, 1:4], want["wi"], what + " wi")
        _same(out[:, 4:7], want["col"], what + " col")
        _same(out[:, 7], want["pdf"], what + " pdf")
        _same(out[:, 8], want["W"], what + " W")
        assert (out[:, 9] == want["sflags"].astype(F)).all(), what
        if flags == K.BSDF_ALL:  # every component is picked, the coat with W = 1 and pdf = its width
            for c in range(3 if M.with_diffuse else 2):
                assert (want["comp"] == c).sum() > 20, (name, c)
            sp = want["comp"] == 0
            assert (want["W"][sp] == 1).all() and (want["sflags"][sp] == K.SPEC).all() and (want["pdf"][sp] >= 0).all()
        if flags == K.SPEC:  # nMatch == 1: width[0] = 1
            live = want["ok"]
            assert (want["pdf"][live] == 1).all() and (want["W"][live] == 1).all()
            assert live.sum() > (n // 2 if M.ior > 1.01 else 0)  # IOR 1.0000001: Kr < 1e-5 returns early nearly everywhere
        if flags == FLAG_CASES[-1]:  # nothing matches: W and wi untouched
            assert not want["ok"].any() and not out[:, 1:9].any()


# ---- GPU: films --------------------------------------------------------------------

FLOOR = dict(color=(0.9, 0.8, 0.7), exponent=80.0, glossy_reflect=0.4, diffuse_reflect=0.7,
             diffuse_color=(0.3, 0.6, 0.9), ior=1.8, mirror_color=(0.9, 1.0, 0.8))
WALL = dict(color=(0.8, 0.3, 0.2), diffuse_reflect=0.9)


def _floor_scene(res, coated=True, **floor_over):
    """a coated floor under a point and a directional light, and a Lambert wall behind it that the
    floor reflects; coated = False: the oracle's twin (same geometry, shinydiffuse materials)"""
    s = Scene()
    kw = dict(FLOOR, **floor_over)
    mf = s.add_material(type_=CG, **kw) if coated else s.add_material(color=(0.5, 0.5, 0.5))
    mw = s.add_material(**WALL)
    s.add_mesh(np.array([[-3, 0, -3], [-3, 0, 3], [3, 0, 3], [3, 0, -3]], F), TG.QUAD, mf)
    s.add_mesh(np.array([[-3, 0, 3], [-3, 2.5, 3], [3, 2.5, 3], [3, 0, 3]], F), TG.QUAD, mw)
    s.add_point_light((0.4, 2.0, 0.3), (1.0, 0.9, 0.8), 6.0)
    s.add_directional_light((0.3, 1.0, -0.5), (0.9, 0.9, 1.0), 0.7)
    s.set_camera((0.2, 1.2, -4.0), (0, 0.4, 0), (0.2, 2.2, -4.0), res, res, focal=1.3)
    s.build()
    return s


def _dl(res, raydepth):
    return TG._params(A.YK_INTEGRATOR_DIRECT, res, 1, raydepth=raydepth, tile_size=16)


def _restate_floor(scene, twin, q, raydepth):
    """per camera sample: direct light at the hit, plus (raydepth >= 1, one level) rcol * the direct light
    at the hit of getSpecular's ray, added as k_fold does: col = (0 + direct) + 0; col += child * rcol"""
    from oracle.oracle import Oracle
    orc = Oracle(twin)
    rays = orc.camera_rays(q.xstart, q.ystart, q.width, q.height, q.aa_samples)
    idx, P, Ng, mat, wo = K.hit_points(orc, rays)
    direct, nsh = K.direct_dirac(orc, scene, P, Ng, mat, wo)
    col = np.zeros((len(rays), 3), F)
    states = scene.material_states()
    stats = dict(children=0, child_hits=0, shadow=nsh)
    if raydepth >= 1:
        assert raydepth == 1
        acc = ((F(0.0) + direct) + F(0.0)).astype(F)
        coated = np.flatnonzero(np.array([states[m].type == CG for m in mat]))
        M = K.Coated(states[mat[coated[0]]])
        assert len(set(mat[coated])) == 1
        refl, d, rc = K.coated_specular(M, Ng[coated], Ng[coated], wo[coated], 1)
        assert refl.all()
        cr = np.zeros((len(coated), 8), F)
        cr[:, 0:3], cr[:, 3:6], cr[:, 6], cr[:, 7] = P[coated], d, F(0.00005), F(-1.0)
        ci, cP, cNg, cmat, cwo = K.hit_points(orc, cr)
        cdir, nsh2 = K.direct_dirac(orc, scene, cP, cNg, cmat, cwo)
        child = np.zeros((len(coated), 3), F)
        child[ci] = ((F(0.0) + cdir) + F(0.0)).astype(F)
        acc[coated] = (acc[coated] + child * rc).astype(F)
        direct = acc
        stats.update(children=len(coated), child_hits=len(ci), shadow=nsh + nsh2)
    col[idx] = direct
    return col, stats


@gpu
def test_direct_lighting_without_recursion_equals_the_restatement(gpu_device):
    res = 16
    scene, twin, q = _floor_scene(res), _floor_scene(res, coated=False), _dl(res, 0)
    col, stats = _restate_floor(scene, twin, q, 0)
    film, st = TG._render(gpu_device, scene, q)
    assert st.closest_rays == res * res and st.shadow_rays == stats["shadow"]
    own = TG.check_film(film, col, q)
    assert (own.sum(-1) > 0).sum() > res * res // 3


@gpu
def test_one_level_of_recursion_equals_the_restatement(gpu_device):
    res = 16
    scene, twin, q = _floor_scene(res), _floor_scene(res, coated=False), _dl(res, 1)
    col, stats = _restate_floor(scene, twin, q, 1)
    assert stats["child_hits"] > res * res // 8, "the floor reflects the wall in too few pixels"
    film, st = TG._render(gpu_device, scene, q)
    assert st.closest_rays == res * res + stats["children"] and st.shadow_rays == stats["shadow"]
    TG.check_film(film, col, q)
    flat, _ = TG._render(gpu_device, scene, _dl(res, 0))
    assert (film.view(np.uint32) != flat.view(np.uint32)).any()
    # a black coat reflects nothing: three levels of it change no bit
    black = _floor_scene(res, mirror_color=(0, 0, 0))
    f0, _ = TG._render(gpu_device, black, _dl(res, 0))
    f3, st3 = TG._render(gpu_device, black, _dl(res, 3))
    assert st3.closest_rays > res * res and (f0.view(np.uint32) == f3.view(np.uint32)).all()


@gpu
def test_raylevel_cap(gpu_device):
    """getSpecular reflects nothing beyond raylevel 5: two facing coated planes and a light between them
    give the same film for raydepth 5 and 12, and another one for raydepth 4"""
    res = 16
    s = Scene()
    m = s.add_material(type_=CG, color=(0.8, 0.8, 0.8), exponent=30.0, glossy_reflect=0.5, diffuse_reflect=0.8,
                       diffuse_color=(0.7, 0.6, 0.5), ior=2.5)
    s.add_mesh(np.array([[-30, 0, -30], [-30, 0, 30], [30, 0, 30], [30, 0, -30]], F), TG.QUAD, m)
    s.add_mesh(np.array([[-30, 2, -30], [30, 2, -30], [30, 2, 30], [-30, 2, 30]], F), TG.QUAD, m)
    s.add_point_light((0.0, 1.0, 2.0), (1.0, 0.9, 0.8), 8.0)
    s.set_camera((0.0, 1.0, -3.0), (0, 0.2, 1.0), (0.0, 2.0, -3.0), res, res, focal=1.0)
    s.build()
    films, rays = {}, {}
    for rd in (4, 5, 12):
        films[rd], st = TG._render(gpu_device, s, _dl(res, rd))
        rays[rd] = st.closest_rays
        assert np.isfinite(films[rd]).all()
    assert rays[5] == rays[12] > rays[4] > res * res
    assert (films[5].view(np.uint32) == films[12].view(np.uint32)).all()
    assert (films[4].view(np.uint32) != films[5].view(np.uint32)).any()


def _coated_room(res, lights="area", spp=4):
    lobes = [MATERIALS["iso_diff_ior1"], MATERIALS["iso"], MATERIALS["aniso_diff"], MATERIALS["iso_diff_on"],
             MATERIALS["aniso"]]
    mats = [dict(type_=CG, **(dict(kw, ior=1.6) if kw.get("ior") == 1.0 else kw)) for kw in lobes]
    q = TG._params(A.YK_INTEGRATOR_PATH, res, spp, caustic_type=A.YK_CAUSTIC_PATH, bounces=3)
    return TG._room(res, mats, lights), q


@gpu
def test_path_tracing_invariants(gpu_device, monkeypatch):
    """finite, non-black, and the same bits over repeat, two shards against one, merged against
    per-bounce and whole against split slot forms"""
    monkeypatch.setenv("YK_DEBUG_HOOKS", "1")
    for k in TG.FORM_KEYS:
        monkeypatch.delenv(k, raising=False)
    s, q = _coated_room(16)
    film, st = TG._render(gpu_device, s, q)
    assert np.isfinite(film).all() and film[..., :3].max() > 0 and st.shadow_rays > 0
    assert st.closest_rays > 2 * 16 * 16 * 4
    again, st2 = TG._render(gpu_device, s, q)
    assert (again.view(np.uint32) == film.view(np.uint32)).all(), "a repeated call differs"
    acc = None
    for i in range(2):
        f, _ = TG._render(gpu_device, s, q, i, 2)
        acc = f.copy() if acc is None else acc + f
    assert (acc.view(np.uint32) == film.view(np.uint32)).all(), "two shards differ from one"
    for form in TG.FORMS[1:]:
        for k in TG.FORM_KEYS:
            monkeypatch.delenv(k, raising=False)
        for k, v in form.items():
            monkeypatch.setenv(k, v)
        f, stf = TG._render(gpu_device, s, q)
        kind = C.c_int32(-1)
        A.check(A.lib().yk_debug_shading_kind(gpu_device._p, C.byref(kind)))
        assert kind.value == 0, "a scene with a coated glossy material is never diffuse-only"
        assert (stf.closest_rays, stf.shadow_rays) == (st.closest_rays, st.shadow_rays), form
        assert (f.view(np.uint32) == film.view(np.uint32)).all(), form


# ---- GPU: photon mapping -------------------------------------------------------------

@gpu
def test_photon_deposits_do_not_depend_on_the_material(gpu_device):
    """bounces = 0: a photon is stored at its first hit and never scattered, and both materials are
    BSDF_DIFFUSE: the coated room's diffuse map == the shinydiffuse room's == the oracle's"""
    from oracle.oracle import Oracle
    sd = [dict(color=c, diffuse_reflect=d) for c, d in TG.DIFFUSE_PARTS]
    q = TG._photon_params(16, 1, bounces=0, final_gather=0)
    plain = TG._room(16, sd, "points")
    coated, _ = _coated_room(16, "points")
    orc = Oracle(plain)
    info_o = orc.photon_build(q)
    want = orc.photon_map(A.YK_PHOTON_MAP_DIFFUSE)
    for scene in (plain, coated):
        gpu_device.upload(scene)
        info = gpu_device.photon_build(q)
        assert info.diffuse_photons == info_o["diffuse_photons"] > 300
        got = gpu_device.photon_map(A.YK_PHOTON_MAP_DIFFUSE)
        assert got.shape == want.shape and (got.view(np.uint32) == want.view(np.uint32)).all()


def _sphere_room():
    """a closed Lambert box with a coated sphere (IOR 2.5) under a point light"""
    from tests.scenes import uv_sphere
    s = Scene()
    wall = s.add_material(color=(0.8, 0.8, 0.8), diffuse_reflect=0.8)
    ball = s.add_material(type_=CG, color=(0.9, 0.9, 0.9), exponent=100.0, glossy_reflect=0.5, diffuse_reflect=0.5,
                          diffuse_color=(0.8, 0.3, 0.3), ior=2.5)
    b = np.array([[x, y, z] for x in (-2.0, 2.0) for y in (0.0, 3.0) for z in (-2.0, 2.0)], F)
    s.add_mesh(b, TG.BOX_FACES, wall)
    pts, faces = uv_sphere(24, 16, 0.6, (0.0, 0.8, 0.0))[:2]
    s.add_mesh(pts, faces, ball)
    s.add_point_light((0.0, 2.5, 0.0), (1.0, 1.0, 1.0), 10.0)
    s.set_camera((0.0, 1.5, -1.9), (0, 0.8, 0), (0.0, 2.5, -1.9), 16, 16, focal=1.0)
    s.build()
    return s


def _predicted_caustic_photons(n):
    """Photons of a point light leave uniformly over the sphere of directions; one that meets the ball first
    takes the coat (the specular pick of BSDF_ALL) with probability Kr / (Kr + Kt) = Kr, survives
    scatterPhoton's roulette with probability max(colour * Kr) / max(colour) = Kr (white mirror_color, W = 1),
    leaves the convex ball and lands on a wall, all of which are diffuse: one caustic photon. Later bounces
    add none (a photon is `direct` only up to its first scatter). So the count is n * E[hit * Kr(cos)^2]."""
    rng = np.random.default_rng(1)
    d = rng.normal(size=(200000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.array([0.0, 2.5, 0.0]) - np.array([0.0, 0.8, 0.0])
    b = d @ o
    disc = b * b - (o @ o - 0.36)
    hit = (disc > 0) & (b < 0)
    t = -b - np.sqrt(np.where(hit, disc, 0))
    nrm = (o + t[:, None] * d) / 0.6
    Kr, _ = K.fresnel((-d[hit]).astype(F), nrm[hit].astype(F), F(2.5))
    return n * float((Kr.astype(np.float64) ** 2).sum()) / len(d)


@gpu
def test_photon_mapping_with_a_coated_sphere(gpu_device):
    s = _sphere_room()
    films = {}
    for fg in (1, 0):
        q = TG._photon_params(16, 1, bounces=3, final_gather=fg, fg_samples=2, fg_bounces=2, photons=4000,
                              caustic_photons=40000)
        runs = []
        for _ in range(2):
            gpu_device.upload(s)
            info = gpu_device.photon_build(q)
            dmap = gpu_device.photon_map(A.YK_PHOTON_MAP_DIFFUSE)
            cmap = gpu_device.photon_map(A.YK_PHOTON_MAP_CAUSTIC)
            rmap = gpu_device.photon_map(A.YK_PHOTON_MAP_RADIANCE) if fg else np.zeros((1, 9), F)
            want = _predicted_caustic_photons(40000)
            print("caustic photons:", info.caustic_photons, "predicted", round(want, 1))
            assert want > 20 and want / 2 <= info.caustic_photons <= want * 2
            assert len(cmap) == info.caustic_photons
            for m in (dmap, cmap, rmap):
                assert np.isfinite(m).all()
            assert dmap[:, 6:].max() > 0 and cmap[:, 6:].max() > 0
            film = gpu_device.new_film(q)
            gpu_device.render_shard(q, film)
            runs.append((info.diffuse_photons, info.caustic_photons, info.radiance_photons, dmap, cmap, rmap,
                         film.cpu().numpy()))
        a, b = runs
        assert a[:3] == b[:3]
        for x, y in zip(a[3:], b[3:]):
            assert (x.view(np.uint32) == y.view(np.uint32)).all(), "a repeated photon-mapped run differs"
        assert np.isfinite(a[6]).all() and a[6][..., :3].max() > 0
        films[fg] = a[6]


# ---- GPU: no cross-talk ------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("other", ["shinydiffuse", "glossy"])
def test_no_cross_talk_after_a_coated_scene(gpu_device, other):
    if other == "glossy":
        plain, q = TG._mixed_scene()
    else:
        sd = [dict(color=c, diffuse_reflect=d) for c, d in TG.DIFFUSE_PARTS]
        plain, q = TG._room(20, sd, "area"), TG._params(A.YK_INTEGRATOR_PATH, 20, 2)
    fresh, st0 = TG._render(gpu_device, plain, q)
    cs, cq = _coated_room(16, spp=1)
    cfilm, _ = TG._render(gpu_device, cs, cq)
    after, st1 = TG._render(gpu_device, plain, q)
    assert fresh[..., :3].max() > 0 and (cfilm.view(np.uint32) != 0).any()
    assert (st0.closest_rays, st0.shadow_rays) == (st1.closest_rays, st1.shadow_rays)
    assert (fresh.view(np.uint32) == after.view(np.uint32)).all()
