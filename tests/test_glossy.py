"""The glossy material (glossyMat_t with as_diffuse: a Blinn or anisotropic
Ashikhmin-Shirley lobe over a diffuse base) on the GPU path.

The oracle knows no glossy material, so the yardsticks are: the reference's
own fPow / fLog2 / fExp2 bits (tests/golden/ref_fpow.npz), the float32
restatement of the material in tests/glossy_common.py, the oracle's films
where glossy's arithmetic reduces to shinydiffuse's, and invariants.

Photon mapping has no restatement either: its deposits are compared with the
oracle's where they cannot depend on the material, the rest by invariants.
"""
import ctypes as C
import os

import numpy as np
import pytest

from core_amd import _abi as A
from core_amd.scene import Scene
from tests import glossy_common as G
from tests.conftest import GOLDEN

gpu = pytest.mark.gpu
F = np.float32
GL = A.YK_MAT_GLOSSY
TINY = np.finfo(F).tiny

# the materials of the probe and film tests: isotropic / anisotropic, with and
# without the diffuse base, with and without Oren-Nayar, glossy_reflect 0, 0.3, 1
MATERIALS = {
    "iso": dict(color=(0.9, 0.8, 0.7), exponent=50.0),
    "iso_r0": dict(color=(0.9, 0.8, 0.7), exponent=5.0, glossy_reflect=0.0),
    "iso_diff": dict(color=(0.9, 0.8, 0.7), exponent=500.0, glossy_reflect=0.3, diffuse_reflect=0.8,
                     diffuse_color=(0.2, 0.5, 0.9)),
    "iso_diff_on": dict(color=(0.6, 0.6, 0.9), exponent=20.0, glossy_reflect=0.3, diffuse_reflect=0.6,
                        diffuse_color=(0.8, 0.4, 0.3), diffuse_brdf="Oren-Nayar", sigma=0.4),
    "aniso": dict(color=(0.7, 0.9, 0.8), anisotropic=True, exp_u=10.0, exp_v=400.0),
    "aniso_diff": dict(color=(0.7, 0.9, 0.8), anisotropic=True, exp_u=300.0, exp_v=8.0, glossy_reflect=0.3,
                       diffuse_reflect=0.7, diffuse_color=(0.9, 0.8, 0.2)),
    "aniso_diff_on_r1": dict(color=(1.0, 0.9, 0.8), anisotropic=True, exp_u=50.0, exp_v=50.0, glossy_reflect=1.0,
                             diffuse_reflect=0.5, diffuse_color=(0.5, 0.5, 0.5), diffuse_brdf="Oren-Nayar",
                             sigma=0.2),
}


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _state(s, i):
    return s.material_states()[i]


# ---- 1. API and state (CPU) --------------------------------------------------

# offsets of the parent commit's fields (its build's ctypes mirror and C structs): appended fields only
PARENT_MATERIAL = dict(type=0, color=4, diffuse_reflect=16, emit=20, power=24, double_sided=28, mirror_color=32,
                       specular_reflect=44, transparency=48, translucency=52, transmit_filter=56, fresnel_effect=60,
                       ior=64, diffuse_brdf=72, sigma=80)
PARENT_MATERIAL_STATE = dict(type=0, bsdf_flags=4, color=8, diffuse_strength=20, emit_color=24, double_sided=36,
                             mirror_color=40, component=52, ncomp=68, comp_flags=72, comp_index=88,
                             transmit_filter=104, has_fresnel=108, ior_squared=112, oren_nayar=116, oren_nayar_a=120,
                             oren_nayar_b=124)


def test_earlier_fields_keep_their_offsets():
    for cls, want, first_new in ((A.yk_material, PARENT_MATERIAL, "diffuse_color"),
                                 (A.yk_material_state, PARENT_MATERIAL_STATE, "gloss_color")):
        for name, off in want.items():
            assert getattr(cls, name).offset == off, (cls.__name__, name)
        assert getattr(cls, first_new).offset >= max(want.values()) + 4
    # the parent's sizes, where the appended fields start
    assert A.yk_material.diffuse_color.offset == 88 and A.yk_material_state.gloss_color.offset == 128


def test_add_material_accepts_and_refuses():
    s = Scene()
    assert s.add_material(type_=GL) == 0
    for kw in MATERIALS.values():
        s.add_material(type_=GL, **kw)

    def code(**kw):
        with pytest.raises(A.YkError) as e:
            s.add_material(type_=GL, **kw)
        return e.value.code

    assert code(as_diffuse=False) == A.YK_ERR_UNSUPPORTED
    for bad in (float("nan"), float("inf")):
        assert code(color=(1, bad, 1)) == A.YK_ERR_ARG
        assert code(diffuse_color=(bad, 1, 1)) == A.YK_ERR_ARG
        assert code(glossy_reflect=bad) == A.YK_ERR_ARG
        assert code(diffuse_reflect=bad) == A.YK_ERR_ARG
        assert code(exponent=bad) == A.YK_ERR_ARG
        assert code(anisotropic=True, exp_u=bad) == A.YK_ERR_ARG
        assert code(anisotropic=True, exp_v=bad) == A.YK_ERR_ARG
    with pytest.raises(A.YkError) as e:
        s.add_material(type_=3)
    assert e.value.code == A.YK_ERR_UNSUPPORTED
    # the state entry point: the same rules
    st = _state(s, 1)
    assert s.add_material_state(st) == len(MATERIALS) + 1
    st.as_diffuse = 0
    with pytest.raises(A.YkError) as e:
        s.add_material_state(st)
    assert e.value.code == A.YK_ERR_UNSUPPORTED
    st.as_diffuse, st.reflectivity = 1, float("nan")
    with pytest.raises(A.YkError) as e:
        s.add_material_state(st)
    assert e.value.code == A.YK_ERR_ARG
    # the other kinds do not read the tail
    assert s.add_material(color=(0.5, 0.5, 0.5), exponent=float("nan"), as_diffuse=False) == len(MATERIALS) + 2


def test_parameters_and_state_round_trip_and_equal_the_restatement():
    s = Scene()
    for kw in MATERIALS.values():
        s.add_material(type_=GL, **kw)
    s.add_material(color=(0.1, 0.2, 0.3))  # a shinydiffuse: its appended state is zero
    mats, states = s.materials(), s.material_states()
    for i, (name, kw) in enumerate(MATERIALS.items()):
        m, st = mats[i], states[i]
        full = dict(color=(1, 1, 1), diffuse_color=(1, 1, 1), glossy_reflect=1.0, diffuse_reflect=0.0, exponent=50.0,
                    anisotropic=False, exp_u=50.0, exp_v=50.0, diffuse_brdf="lambert", sigma=0.1)
        full.update(kw)
        assert m.type == GL and m.as_diffuse == 1 and m.anisotropic == int(full["anisotropic"])
        assert tuple(m.color) == tuple(F(c) for c in full["color"])
        assert tuple(m.diffuse_color) == tuple(F(c) for c in full["diffuse_color"])
        assert (m.glossy_reflect, m.diffuse_reflect, m.exponent, m.exp_u, m.exp_v) == tuple(
            F(full[k]) for k in ("glossy_reflect", "diffuse_reflect", "exponent", "exp_u", "exp_v"))
        assert m.sigma == full["sigma"] and m.diffuse_brdf == int(full["diffuse_brdf"] == "Oren-Nayar")
        want = G.state_of(color=full["color"], diffuse_color=full["diffuse_color"],
                          glossy_reflect=full["glossy_reflect"], diffuse_reflect=full["diffuse_reflect"],
                          exponent=full["exponent"], anisotropic=full["anisotropic"], exp_u=full["exp_u"],
                          exp_v=full["exp_v"], oren_nayar=full["diffuse_brdf"] == "Oren-Nayar", sigma=full["sigma"])
        for k, v in want.items():
            got = getattr(st, k)
            got = tuple(got) if hasattr(got, "__len__") else got
            assert got == v, (name, k, got, v)
        # nothing of shinydiffuse's in a glossy state
        assert st.ncomp == 0 and tuple(st.component) == (0, 0, 0, 0) and tuple(st.emit_color) == (0, 0, 0)
        # a state handed back in reads out the same
        j = s.add_material_state(st)
        assert bytes(s.material_states()[j]) == bytes(st)
    sd = states[len(MATERIALS)]
    assert sd.type == 0 and bytes(sd)[A.yk_material_state.gloss_color.offset:] == bytes(
        C.sizeof(A.yk_material_state) - A.yk_material_state.gloss_color.offset)
    # flags as glossy.cc:69-79 sets them
    assert states[0].bsdf_flags == states[2].bsdf_flags == (G.BSDF_DIFFUSE | G.BSDF_REFLECT)
    assert states[0].with_diffuse == 0 and states[2].with_diffuse == 1


def test_the_probe_is_exported_and_off_by_default(monkeypatch):
    """a test hook like the lights' probe: outside the product header and its binding table, refused
    unless YK_DEBUG_HOOKS=1"""
    monkeypatch.delenv("YK_DEBUG_HOOKS", raising=False)
    assert "yk_debug_material_probe" not in A.SIGNATURES
    assert _probe_fn()(None, 0, 0, None, 0, None) == A.YK_ERR_UNSUPPORTED


# ---- 2. fPow pinned to the reference (CPU) -----------------------------------

@pytest.fixture(scope="module")
def ref_fpow():
    g = np.load(os.path.join(GOLDEN, "ref_fpow.npz"))
    return {k: g[k] for k in g.files}


def _normal_or_zero(bits):
    v = bits.view(F)
    return (v == 0) | (np.abs(v) >= TINY) | ~np.isfinite(v)


def test_fpow_restatement_equals_the_reference(ref_fpow):
    g = ref_fpow
    assert len(g["a"]) > 10000 and (~_normal_or_zero(g["fpow"])).mean() <= 0.01
    for name, mine in (("fpow", G.fpow(g["a"], g["b"])), ("flog2", G.flog2(g["a"])), ("fexp2", G.fexp2(g["b"]))):
        ok = _normal_or_zero(g[name])
        bad = (_bits(mine) != g[name]) & ok
        assert not bad.any(), f"{name}: {bad.sum()} differ, first a={g['a'][bad][0]!r} b={g['b'][bad][0]!r}"
    # zero and negative bases have values: the sign is masked off, zero reads as 2^-127
    assert (G.flog2(F([0.0, -0.0])) == F(-127.0)).all()
    assert _bits(G.fpow(F([-0.5]), F([5.0])))[0] == _bits(G.fpow(F([0.5]), F([5.0])))[0]


# ---- GPU: probes -------------------------------------------------------------

def _probe_fn():
    fn = A.lib().yk_debug_material_probe  # include/yk_test_hooks_material.h
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int32, C.c_int32, A.fp, C.c_int64, A.fp]
    return fn


def _probe(dev, mat, fn, rows):
    """rows: (n, 20) float32 inputs of yk_debug_material_probe; returns (n, 10)"""
    rows = np.ascontiguousarray(rows, F)
    out = np.zeros((len(rows), 10), F)
    A.check(_probe_fn()(dev._p, mat, fn, rows.ctypes.data_as(A.fp), len(rows),
                                            out.ctypes.data_as(A.fp)))
    return out


EVAL, SAMPLE, PDF, FPOW, ATAN_TAN = range(5)


class DeviceTrig:
    """the device library's atanf / tanf, through the ATAN_TAN probe"""

    def __init__(self, dev):
        self.dev = dev

    def _run(self, x, col):
        rows = np.zeros((len(x), 20), F)
        rows[:, 0] = x
        return _probe(self.dev, 0, ATAN_TAN, rows)[:, col].copy()

    def atanf(self, x):
        return self._run(x, 0)

    def tanf(self, x):
        return self._run(x, 1)


def _material_scene():
    """every MATERIALS entry (ids in dict order), then a shinydiffuse; one quad and a point light"""
    s = Scene()
    for kw in MATERIALS.values():
        s.add_material(type_=GL, **kw)
    sd = s.add_material(color=(0.8, 0.7, 0.6), diffuse_reflect=0.9)
    s.add_mesh(np.array([[-1, 0, -1], [-1, 0, 1], [1, 0, 1], [1, 0, -1]], F), np.array([[0, 1, 2], [0, 2, 3]], np.int32), sd)
    s.add_point_light((0, 2, 0))
    s.set_camera((0, 2, -3), (0, 0, 0), (0, 3, -3), 16, 16)
    s.build()
    return s


@pytest.fixture(scope="module")
def material_device(gpu_device):
    s = _material_scene()
    gpu_device.upload(s)
    return gpu_device, s


@gpu
def test_device_fpow_equals_the_reference(material_device, monkeypatch, ref_fpow):
    monkeypatch.setenv("YK_DEBUG_HOOKS", "1")
    dev, _ = material_device
    g = ref_fpow
    rows = np.zeros((len(g["a"]), 20), F)
    rows[:, 0], rows[:, 1] = g["a"], g["b"]
    out = _probe(dev, 0, FPOW, rows)
    flushed = 0
    for col, name in ((0, "fpow"), (1, "flog2"), (2, "fexp2")):
        got, want = _bits(out[:, col]), g[name]
        sub = ~_normal_or_zero(want)
        # the one exception: a subnormal reference result may read (signed) zero on the device
        ok = (got == want) | (sub & ((got & 0x7FFFFFFF) == 0))
        assert ok.all(), f"{name}: {(~ok).sum()} differ, first a={g['a'][~ok][0]!r} b={g['b'][~ok][0]!r}"
        flushed += int((sub & (got != want)).sum())
    print("flushed subnormal results:", flushed, "of", len(g["a"]))
    assert flushed <= 0.01 * len(g["a"])


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F)


def _directions(rng, n):
    """N, wo, wl: random unit vectors, then grazing ones and wo below Ng"""
    N = _unit(rng.normal(size=(n, 3)))
    wo = _unit(rng.normal(size=(n, 3)))
    wl = _unit(rng.normal(size=(n, 3)))
    k = n // 8
    N[:k] = (0, 0, 1)                      # createCS's flat branch
    N[k:2 * k] = (0, 0, -1)
    # grazing: wo (and wl) nearly in the tangent plane
    NU, _ = G.create_cs(N)
    eps = rng.uniform(-2e-3, 2e-3, size=(n, 1)).astype(F)
    wo[2 * k:3 * k] = _unit(NU[2 * k:3 * k] + eps[2 * k:3 * k] * N[2 * k:3 * k])
    wl[3 * k:4 * k] = _unit(-NU[3 * k:4 * k] + eps[3 * k:4 * k] * N[3 * k:4 * k])
    # wo below Ng, wl on either side
    flip = np.einsum("ij,ij->i", wo[4 * k:5 * k], N[4 * k:5 * k]) > 0
    wo[4 * k:5 * k][flip] *= -1
    # mirror directions: the lobe's peak
    d = np.einsum("ij,ij->i", wo[5 * k:6 * k], N[5 * k:6 * k])[:, None]
    wl[5 * k:6 * k] = _unit(2 * d * N[5 * k:6 * k] - wo[5 * k:6 * k])
    return N, wo, wl


def _same(got, want, what):
    got, want = np.asarray(got, F), np.asarray(want, F)
    # a NaN is a NaN (0 * inf at a degenerate direction): its payload is not compared
    bad = (_bits(got) != _bits(want)) & ~(np.isnan(got) & np.isnan(want))
    if bad.ndim > 1:
        bad = bad.any(-1)
    assert not bad.any(), f"{what}: {bad.sum()} of {len(bad)} differ; first at {np.flatnonzero(bad)[0]}: " \
                          f"{got[bad][0]!r} vs {want[bad][0]!r}"


FLAG_CASES = [G.BSDF_ALL, G.BSDF_DIFFUSE, G.BSDF_ALL & ~G.BSDF_REFLECT]


@gpu
@pytest.mark.parametrize("name", list(MATERIALS))
def test_eval_and_pdf_equal_the_restatement(material_device, monkeypatch, name):
    monkeypatch.setenv("YK_DEBUG_HOOKS", "1")
    dev, s = material_device
    mi = list(MATERIALS).index(name)
    Mt = G.Glossy(_state(s, mi))
    rng = np.random.default_rng(100 + mi)
    n = 2048
    N, wo, wl = _directions(rng, n)
    NU, NV = G.create_cs(N)
    rows = np.zeros((n, 20), F)
    rows[:, 0:3], rows[:, 3:6], rows[:, 6:9] = N, wo, wl
    for flags in FLAG_CASES + [G.BSDF_GLOSSY | G.BSDF_REFLECT]:
        rows[:, 9] = flags
        col = _probe(dev, mi, EVAL, rows)[:, 0:3]
        want = G.glossy_eval(Mt, N, N, NU, NV, wo, wl, flags)
        _same(col, want, f"eval {name} flags {flags:#x}")
        pdf = _probe(dev, mi, PDF, rows)[:, 0]
        _same(pdf, G.glossy_pdf(Mt, N, N, NU, NV, wo, wl, flags), f"pdf {name} flags {flags:#x}")
        if flags == G.BSDF_ALL:
            assert np.isfinite(col).all() and (col > 0).any() and (pdf > 0).any()
    # given tangents (an anisotropic lobe turned about N)
    rows[:, 9] = G.BSDF_ALL
    rows[:, 13:16], rows[:, 16:19], rows[:, 19] = NV, -NU, 1
    _same(_probe(dev, mi, EVAL, rows)[:, 0:3], G.glossy_eval(Mt, N, N, NV, -NU, wo, wl), f"eval {name} turned")


def _sample_numbers(rng, n, pD):
    """s1 on both sides of pDiffuse and at the four quadrant edges of AS_Aniso_Sample (as sample() rescales
    it: (s1 - pD) / (1 - pD) lands on 0.25 / 0.5 / 0.75 and next to them), s2 in {0, 1 - ulp} and random"""
    s1 = rng.random(n, dtype=F)
    s2 = rng.random(n, dtype=F)
    below = np.nextafter(F(1.0), F(0.0))
    k = n // 8
    edges = []
    for q in (0.0, 0.25, 0.5, 0.75):
        v = F(q)
        edges += [np.nextafter(v, F(-1)), v, np.nextafter(v, F(2))]
    edges = np.abs(np.array(edges + [below], F))
    s1[:k] = rng.choice(edges, k)                                  # the edges themselves (no diffuse half)
    s1[k:2 * k] = (F(pD) + rng.choice(edges, k) * (F(1.0) - F(pD))).astype(F)  # ... behind the diffuse half
    s1[2 * k:3 * k] = rng.choice(np.array([np.nextafter(F(pD), F(-1)), F(pD), np.nextafter(F(pD), F(2))], F), k)
    s1 = np.clip(s1, F(0.0), below)
    s2[3 * k:4 * k] = F(0.0)
    s2[4 * k:5 * k] = below
    s2[:k // 2] = F(0.0)
    return s1, s2


@gpu
@pytest.mark.parametrize("name", list(MATERIALS))
def test_sample_equals_the_restatement(material_device, monkeypatch, name):
    monkeypatch.setenv("YK_DEBUG_HOOKS", "1")
    dev, s = material_device
    mi = list(MATERIALS).index(name)
    Mt = G.Glossy(_state(s, mi))
    trig = DeviceTrig(dev)
    rng = np.random.default_rng(200 + mi)
    n = 2048
    N, wo, _ = _directions(rng, n)
    NU, NV = G.create_cs(N)
    s1, s2 = _sample_numbers(rng, n, Mt.pD)
    rows = np.zeros((n, 20), F)
    rows[:, 0:3], rows[:, 3:6], rows[:, 6], rows[:, 7] = N, wo, s1, s2
    for flags in FLAG_CASES:
        rows[:, 9] = flags
        out = _probe(dev, mi, SAMPLE, rows)
        want = G.glossy_sample(Mt, N, N, NU, NV, wo, s1, s2, flags, trig)
        what = f"sample {name} flags {flags:#x}"
        assert (out[:, 0] == want["ok"].astype(F)).all(), what
        _same(out[:, 1:4], want["wi"], what + " wi")
        _same(out[:, 4:7], want["col"], what + " col")
        _same(out[:, 7], want["pdf"], what + " pdf")
        _same(out[:, 8], want["W"], what + " W")
        assert (out[:, 9] == want["sflags"].astype(F)).all(), what
        if flags == G.BSDF_ALL:
            assert want["ok"].sum() > n // 2 and (want["W"] > 0).sum() > n // 2
            if Mt.with_diffuse and Mt.pD > 0:  # glossy_reflect = 1 gives pDiffuse = 0: no diffuse half to take
                assert (s1 < Mt.pD).any() and (s1 >= Mt.pD).any()


@gpu
def test_probe_serves_a_shinydiffuse_material(material_device, monkeypatch):
    """eval of the one-component Lambert material is d * c on the lit side; its sample is a unit
    direction in N's hemisphere flagged DIFFUSE | REFLECT"""
    monkeypatch.setenv("YK_DEBUG_HOOKS", "1")
    dev, s = material_device
    mi = len(MATERIALS)
    rng = np.random.default_rng(7)
    N, wo, wl = _directions(rng, 512)
    rows = np.zeros((512, 20), F)
    rows[:, 0:3], rows[:, 3:6], rows[:, 6:9], rows[:, 9] = N, wo, wl, G.BSDF_ALL
    col = _probe(dev, mi, EVAL, rows)[:, 0:3]
    st = _state(s, mi)
    dc = F(st.component[3]) * F(list(st.color))
    Nf = G.face_forward(N, N, wo)
    lit = G.dot(wl, Nf) >= 0
    assert lit.any() and (~lit).any()
    assert (_bits(col[lit]) == _bits(dc)[None, :]).all() and (col[~lit] == 0).all()
    rows[:, 6], rows[:, 7] = rng.random(512, dtype=F), rng.random(512, dtype=F)
    out = _probe(dev, mi, SAMPLE, rows)
    assert (out[:, 0] == 1).all() and (out[:, 9] == (G.BSDF_DIFFUSE | G.BSDF_REFLECT)).all()
    wi = out[:, 1:4].astype(np.float64)
    # FAST_TRIG's parabola sine is within 1.1e-3 of sin, so cos^2 + sin^2 is within 2.2e-3 of 1
    assert np.allclose(np.linalg.norm(wi, axis=1), 1.0, atol=2.5e-3) and (np.einsum("ij,ij->i", wi, Nf) > -1e-6).all()


# ---- GPU: films --------------------------------------------------------------

def _params(integ, res, spp, **over):
    p = A.yk_render_params()
    A.lib().yk_render_params_default(C.byref(p))
    p.integrator = integ
    p.width = p.height = res
    p.aa_samples = spp
    p.tile_size = 8
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


BOX_FACES = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1],
                      [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.int32)
QUAD = np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def _room(res, mats, lights="dirac"):
    """Cornell-like and flat-shaded: floor, back wall, two side walls and a box, one material each
    (mats: five add_material keyword dicts). lights "dirac": a point and an infinite directional
    light strictly above every surface's lit side; "points": two point lights; "area": one area light."""
    s = Scene()
    m = [s.add_material(**kw) for kw in mats]
    s.add_mesh(np.array([[-2, 0, -2], [-2, 0, 2], [2, 0, 2], [2, 0, -2]], F), QUAD, m[0])
    s.add_mesh(np.array([[-2, 0, 2], [-2, 3, 2], [2, 3, 2], [2, 0, 2]], F), QUAD, m[1])
    s.add_mesh(np.array([[-2, 0, -2], [-2, 3, -2], [-2, 3, 2], [-2, 0, 2]], F), QUAD, m[2])
    s.add_mesh(np.array([[2, 0, -2], [2, 0, 2], [2, 3, 2], [2, 3, -2]], F), QUAD, m[3])
    b = np.array([[x, y, z] for x in (-0.7, 0.2) for y in (0.0, 1.0) for z in (-0.3, 0.6)], F)
    s.add_mesh(b, BOX_FACES, m[4])
    if lights == "area":
        s.add_area_light((-0.5, 2.9, -0.5), (0.5, 2.9, -0.5), (-0.5, 2.9, 0.5), (1.0, 0.95, 0.9), 6.0, 2)
    else:
        s.add_point_light((0.4, 2.5, -0.6), (1.0, 0.9, 0.8), 6.0)
        if lights == "points":
            s.add_point_light((-1.2, 2.0, -1.0), (0.6, 0.8, 1.0), 3.0)
        else:
            s.add_directional_light((0.3, 1.0, -0.5), (0.9, 0.9, 1.0), 0.7)
    s.set_camera((0.2, 1.6, -5.0), (0, 1.1, 0), (0.2, 2.6, -5.0), res, res, focal=1.6)
    s.build()
    return s


DIFFUSE_PARTS = [((0.8, 0.8, 0.7), 0.9), ((0.7, 0.7, 0.8), 0.8), ((0.8, 0.1, 0.1), 1.0), ((0.1, 0.8, 0.1), 0.7),
                 ((0.3, 0.5, 0.9), 0.6)]


@gpu
@pytest.mark.parametrize("spp", [1, 2])
def test_direct_lighting_equals_the_oracle_where_the_arithmetic_coincides(gpu_device, spp):
    """Glossy with a black gloss colour, glossy_reflect 0, diffuse_reflect d and diffuse_color c evaluates to
    0 + 1 * (d * (1 - 0)) * c_k = d * c_k, the product shinydiffuse(color c, diffuse_reflect d) evaluates to:
    the film of the glossy scene equals the oracle's film of the shinydiffuse scene bit for bit."""
    from oracle.oracle import Oracle
    res = 24
    gl = [dict(type_=GL, color=(0, 0, 0), glossy_reflect=0.0, diffuse_reflect=d, diffuse_color=c,
               exponent=e, anisotropic=a, exp_u=30.0, exp_v=90.0)
          for (c, d), e, a in zip(DIFFUSE_PARTS, (50.0, 5.0, 500.0, 50.0, 20.0), (False, True, False, True, False))]
    sd = [dict(color=c, diffuse_reflect=d) for c, d in DIFFUSE_PARTS]
    q = _params(A.YK_INTEGRATOR_DIRECT, res, spp)
    _, sums_o, cnt = Oracle(_room(res, sd, "points")).render(q)
    film, st = _render(gpu_device, _room(res, gl, "points"), q)
    assert (st.closest_rays, st.shadow_rays) == (cnt["closest"], cnt["shadow"]) and st.shadow_rays > res * res
    assert sums_o[..., :3].max() > 0
    bad = (film.view(np.uint32) != sums_o.view(np.uint32)).any(-1)
    assert not bad.any(), f"{bad.sum()} pixels differ; first {np.argwhere(bad)[0]}: {film[bad][0]} vs {sums_o[bad][0]}"


LOBES = {
    "iso": [MATERIALS["iso_diff"], MATERIALS["iso"], MATERIALS["iso_diff_on"], MATERIALS["iso_r0"],
            MATERIALS["iso_diff"]],
    "aniso": [MATERIALS["aniso_diff"], MATERIALS["aniso"], MATERIALS["aniso_diff_on_r1"], MATERIALS["aniso_diff"],
              MATERIALS["aniso"]],
}


def restate_direct_dirac(orc, glossy_scene, p):
    """Per camera sample (pixel-major, sample fastest) the colour direct lighting returns for Dirac lights
    (mcintegrator.cc:85-100) on flat-shaded glossy surfaces: camera rays, hits and isShadowed from the
    oracle (of the same geometry), eval from tests/glossy_common.py, products in the order the device
    keeps (R, G: (lcol * surf) * |N.l|; B: surf * (lcol * |N.l|)), lights summed from 0 in scene order."""
    spp = p.aa_samples
    rays = orc.camera_rays(p.xstart, p.ystart, p.width, p.height, spp)
    prim, t, _, _, _ = orc.intersect(rays)
    e = orc.arrays
    states = glossy_scene.material_states()
    col = np.zeros((len(rays), 3), F)
    idx = np.flatnonzero(prim >= 0)
    mat = e["tri_material"][prim[idx]]
    frm, d = rays[idx, 0:3], rays[idx, 3:6]
    P = (frm + t[idx, None] * d).astype(F)
    Ng = e["tri_normal"][prim[idx]].astype(F)
    NU, NV = G.create_cs(Ng)
    wo = (-d).astype(F)
    acc = np.zeros((len(idx), 3), F)
    nshadow = 0
    for L in glossy_scene.light_states():
        lc = F(list(L.color))
        if L.type == A.YK_LIGHT_POINT:
            l = (F(list(L.position))[None, :] - P).astype(F)
            dist_sqr = l[:, 0] * l[:, 0] + l[:, 1] * l[:, 1] + l[:, 2] * l[:, 2]
            dist = np.sqrt(dist_sqr)
            idist_sqr, inv = F(1.0) / dist_sqr, F(1.0) / dist
            ldir = (l * inv[:, None]).astype(F)
            tmax = dist
            lcol = (lc[None, :] * idist_sqr[:, None]).astype(F)
            assert (dist > 0).all()
        else:
            assert L.infinite
            ldir = np.broadcast_to(F(list(L.direction)), P.shape).astype(F)
            tmax = np.full(len(P), F(-1.0))
            lcol = np.broadcast_to(lc, P.shape).astype(F)
        sr = np.zeros((len(P), 8), F)
        sr[:, 0:3], sr[:, 3:6], sr[:, 6], sr[:, 7] = P, ldir, F(0.0005), tmax
        occ, _ = orc.shadow(sr)
        nshadow += len(sr)
        surf = np.zeros((len(P), 3), F)
        for m in np.unique(mat):
            k = mat == m
            surf[k] = G.glossy_eval(G.Glossy(states[m]), Ng[k], Ng[k], NU[k], NV[k], wo[k], ldir[k])
        f = np.abs(G.dot(Ng, ldir))
        v = np.stack([(lcol[:, 0] * surf[:, 0]) * f, (lcol[:, 1] * surf[:, 1]) * f, surf[:, 2] * (lcol[:, 2] * f)], 1)
        v = np.where(occ.astype(bool)[:, None], F(0.0), v).astype(F)
        acc = (acc + (F(0.0) + v)).astype(F)
    col[idx] = (F(0.0) + acc).astype(F)
    return dict(col=col, hits=len(idx), shadow_rays=nshadow)


def check_film(film, col, p):
    """The film sums against the per-sample colours, bit for bit. The box filter's width is held at
    0.501 pixels at least (imagefilm.cc:143-150), so a sample within 0.001 of its pixel's border also
    lands in the neighbour: a pixel's sum is its own samples' colours in order (weight = spp), or, where
    the weight says one more sample arrived, those plus one sample of a neighbouring pixel, added ahead
    of them or after them as the film's pixel order has it. Every pixel must be one of the two, exactly."""
    spp = p.aa_samples
    c = col.reshape(p.height, p.width, spp, 3)
    own = np.zeros((p.height, p.width, 3), F)
    for s in range(spp):
        own = (own + c[:, :, s]).astype(F)
    wt = film[..., 4]
    plain = wt == spp
    assert plain.mean() > 0.95 and ((wt == spp) | (wt == spp + 1)).all(), np.unique(wt)
    bad = (film[..., :3].view(np.uint32) != own.view(np.uint32)).any(-1) & plain
    assert not bad.any(), f"{bad.sum()} pixels differ; first {np.argwhere(bad)[0]}: {film[..., :3][bad][0]} vs {own[bad][0]}"
    for y, x in np.argwhere(~plain):
        found = False
        got = np.ascontiguousarray(film[y, x, :3]).view(np.uint32)
        for ny in range(max(0, y - 1), min(p.height, y + 2)):
            for nx in range(max(0, x - 1), min(p.width, x + 2)):
                for s in range(spp if (ny, nx) != (y, x) else 0):
                    before = c[ny, nx, s]
                    for k in range(spp):
                        before = (before + c[y, x, k]).astype(F)
                    after = (own[y, x] + c[ny, nx, s]).astype(F)
                    found |= bool((got == before.view(np.uint32)).all() or (got == after.view(np.uint32)).all())
        assert found, f"pixel {(y, x)} with weight {wt[y, x]}: {film[y, x, :3]} is not its samples {own[y, x]} plus a neighbour's"
    return own


@gpu
@pytest.mark.parametrize("spp", [1, 2])
@pytest.mark.parametrize("lobe", list(LOBES))
def test_direct_lighting_with_a_lobe_equals_the_restatement(gpu_device, lobe, spp):
    from oracle.oracle import Oracle
    res = 24
    gl = [dict(type_=GL, **kw) for kw in LOBES[lobe]]
    sd = [dict(color=c, diffuse_reflect=d) for c, d in DIFFUSE_PARTS]  # the oracle's twin: geometry alone matters
    scene = _room(res, gl)
    q = _params(A.YK_INTEGRATOR_DIRECT, res, spp)
    r = restate_direct_dirac(Oracle(_room(res, sd)), scene, q)
    film, st = _render(gpu_device, scene, q)
    assert r["hits"] > res * res * spp // 2
    assert st.shadow_rays == r["shadow_rays"] and st.closest_rays == res * res * spp
    want = check_film(film, r["col"], q)
    assert (want.sum(-1) > 0).sum() > res * res // 3


# path tracing: glossy and shinydiffuse materials under an area light
FORMS = [dict(), dict(YK_MERGE="0"), dict(YK_SPLIT="0"), dict(YK_SPLIT="1"), dict(YK_MERGE="0", YK_SPLIT="1"),
         dict(YK_MERGE="0", YK_SPLIT="0")]
FORM_KEYS = ("YK_MERGE", "YK_SPLIT", "YK_PIPES", "YK_DIFF", "YK_SMALL")


def _mixed_scene(res=20):
    sd = [dict(color=c, diffuse_reflect=d) for c, d in DIFFUSE_PARTS]
    mats = [dict(type_=GL, **MATERIALS["iso_diff"]), sd[1], dict(type_=GL, **MATERIALS["aniso_diff"]), sd[3],
            dict(type_=GL, **MATERIALS["iso_diff_on"])]
    return _room(res, mats, "area"), _params(A.YK_INTEGRATOR_PATH, res, 2)


@pytest.fixture(scope="module")
def form_reference(gpu_device):
    saved = {k: os.environ.pop(k) for k in FORM_KEYS if k in os.environ}
    try:
        s, q = _mixed_scene()
        film, st = _render(gpu_device, s, q)
        assert np.isfinite(film).all() and film[..., :3].max() > 0 and st.shadow_rays > 0
        assert st.closest_rays > 2 * q.width * q.height * q.aa_samples  # the paths went on past the camera hit
        again, st2 = _render(gpu_device, s, q)
        assert (again.view(np.uint32) == film.view(np.uint32)).all(), "a repeated call differs"
        assert (st2.closest_rays, st2.shadow_rays) == (st.closest_rays, st.shadow_rays)
        acc = None
        for i in range(2):  # box filter one pixel wide: no sample crosses a tile border, the shards' sums add up
            f, _ = _render(gpu_device, s, q, i, 2)
            acc = f.copy() if acc is None else acc + f
        assert (acc.view(np.uint32) == film.view(np.uint32)).all(), "two shards differ from one"
    finally:
        os.environ.update(saved)
    return film, (st.closest_rays, st.shadow_rays)


@gpu
@pytest.mark.parametrize("form", range(len(FORMS)),
                         ids=["-".join(f"{k}{v}" for k, v in f.items()) or "default" for f in FORMS])
def test_path_tracing_form_invariance(gpu_device, monkeypatch, form_reference, form):
    monkeypatch.setenv("YK_DEBUG_HOOKS", "1")
    s, q = _mixed_scene()
    for k in FORM_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    film, st = _render(gpu_device, s, q)
    kind = C.c_int32(-1)
    A.check(A.lib().yk_debug_shading_kind(gpu_device._p, C.byref(kind)))
    assert kind.value == 0, "a scene with a glossy material is never diffuse-only"
    if "YK_SPLIT" in FORMS[form]:
        split = C.c_int32(-1)
        A.check(A.lib().yk_debug_shadow_form(gpu_device._p, C.byref(q), C.byref(split)))
        assert split.value == int(FORMS[form]["YK_SPLIT"])
    assert (st.closest_rays, st.shadow_rays) == form_reference[1]
    assert (film.view(np.uint32) == form_reference[0].view(np.uint32)).all()


@gpu
@pytest.mark.parametrize("integ", [A.YK_INTEGRATOR_DIRECT, A.YK_INTEGRATOR_PATH])
def test_no_cross_talk_after_a_glossy_scene(gpu_device, integ):
    """A scene without glossy materials renders the same bits whether or not a glossy scene was uploaded
    and rendered on the handle before it (the constants are bound again, the other kernels are launched)."""
    sd = [dict(color=c, diffuse_reflect=d) for c, d in DIFFUSE_PARTS]
    lights = "dirac" if integ == A.YK_INTEGRATOR_DIRECT else "area"
    plain = _room(20, sd, lights)
    q = _params(integ, 20, 2)
    before, st0 = _render(gpu_device, plain, q)
    gs, gq = _mixed_scene()
    gfilm, _ = _render(gpu_device, gs, gq)
    after, st1 = _render(gpu_device, plain, q)
    assert before[..., :3].max() > 0 and (gfilm.view(np.uint32) != 0).any()
    assert (st0.closest_rays, st0.shadow_rays) == (st1.closest_rays, st1.shadow_rays)
    assert (before.view(np.uint32) == after.view(np.uint32)).all()


@gpu
def test_ambient_occlusion_runs_on_glossy_surfaces(gpu_device):
    """direct lighting's AO samples the material (mat_sample with GLOSSY | DIFFUSE | REFLECT): finite, adds
    light, and repeats bit for bit"""
    s, _ = _mixed_scene()
    q = _params(A.YK_INTEGRATOR_DIRECT, 20, 1)
    base, _ = _render(gpu_device, s, q)
    q.do_ao, q.ao_samples, q.ao_distance, q.ao_color = 1, 4, 1.0, A.f3(1, 1, 1)
    f1, st = _render(gpu_device, s, q)
    f2, _ = _render(gpu_device, s, q)
    assert np.isfinite(f1).all() and (f1.view(np.uint32) == f2.view(np.uint32)).all()
    assert f1[..., :3].sum() > base[..., :3].sum() and st.shadow_rays > 20 * 20 * 4


def _photon_params(res, spp, **ph):
    q = _params(A.YK_INTEGRATOR_PHOTON, res, spp)
    q.photon.photons = 3000
    q.photon.search = 32
    for k, v in ph.items():
        setattr(q.photon, k, v)
    return q


@gpu
@pytest.mark.parametrize("lights", ["points", "area"])
def test_photon_deposits_do_not_depend_on_the_material(gpu_device, lights):
    """With photon.bounces = 0 a photon is stored at its first hit and never scattered (deposits happen
    before scatterPhoton), and both materials are BSDF_DIFFUSE: the diffuse map of the glossy scene equals
    the map of the same scene with shinydiffuse materials, and so the oracle's, bit for bit."""
    from oracle.oracle import Oracle
    sd = [dict(color=c, diffuse_reflect=d) for c, d in DIFFUSE_PARTS]
    gl = [dict(type_=GL, **m) for m in LOBES["iso"][:3] + LOBES["aniso"][:2]]
    q = _photon_params(16, 1, bounces=0, final_gather=0)
    plain = _room(16, sd, lights)
    orc = Oracle(plain)
    info_o = orc.photon_build(q)
    want = orc.photon_map(A.YK_PHOTON_MAP_DIFFUSE)
    maps = []
    for scene in (plain, _room(16, gl, lights)):
        gpu_device.upload(scene)
        info = gpu_device.photon_build(q)
        assert info.diffuse_photons == info_o["diffuse_photons"] > 300 and info.seed_out == info_o["seed_out"]
        maps.append(gpu_device.photon_map(A.YK_PHOTON_MAP_DIFFUSE))
    assert maps[0].shape == want.shape == maps[1].shape
    assert (maps[0].view(np.uint32) == want.view(np.uint32)).all(), "the shinydiffuse map differs from the oracle's"
    assert (maps[1].view(np.uint32) == want.view(np.uint32)).all(), "the glossy map differs"


@gpu
@pytest.mark.parametrize("final_gather", [1, 0])
def test_photon_mapping_runs_on_glossy_surfaces(gpu_device, final_gather):
    """Three photon bounces (scatterPhoton samples glossy), the radiance map (its colours are built from
    getReflectivity, 16 glossy samples each, so finite colours mean finite reflectivities) and the render,
    with final gathering or with the diffuse-map estimate (eval over the gathered photons): the build
    succeeds, everything is finite, the film is not black, and a repeat gives the same bits."""
    s, _ = _mixed_scene(16)
    q = _photon_params(16, 2, bounces=3, final_gather=final_gather, fg_samples=2, fg_bounces=2)
    gpu_device.upload(s)
    first_hits = gpu_device.photon_build(_photon_params(16, 2, bounces=0, final_gather=0)).diffuse_photons
    films, built = [], []
    for _ in range(2):
        gpu_device.upload(s)
        info = gpu_device.photon_build(q)
        assert info.diffuse_photons > first_hits > 0  # photons went on past their first hit
        dmap = gpu_device.photon_map(A.YK_PHOTON_MAP_DIFFUSE)
        assert np.isfinite(dmap).all() and (dmap[:, 6:] >= 0).all() and dmap[:, 6:].max() > 0
        rmap = None
        if final_gather:
            assert info.radiance_photons > 0
            rmap = gpu_device.photon_map(A.YK_PHOTON_MAP_RADIANCE)
            assert np.isfinite(rmap).all() and rmap[:, 6:].max() > 0
        film = gpu_device.new_film(q)
        gpu_device.render_shard(q, film)
        films.append(film.cpu().numpy())
        built.append((info.diffuse_photons, info.radiance_photons, info.seed_out, dmap, rmap))
    assert np.isfinite(films[0]).all() and films[0][..., :3].max() > 0
    assert built[0][:3] == built[1][:3] and (built[0][3].view(np.uint32) == built[1][3].view(np.uint32)).all()
    if final_gather:
        assert (built[0][4].view(np.uint32) == built[1][4].view(np.uint32)).all()
    assert (films[0].view(np.uint32) == films[1].view(np.uint32)).all(), "a repeated photon-mapped render differs"


def test_glossy_state_with_other_flags_is_refused():
    """as_diffuse glossy is BSDF_DIFFUSE | BSDF_REFLECT (glossy.cc:69-79); a state carrying any other flag
    would steer the kernels onto members a glossy record does not have"""
    s = Scene()
    s.add_material(type_=GL, **MATERIALS["iso_diff"])
    st = _state(s, 0)
    assert st.bsdf_flags == (G.BSDF_DIFFUSE | G.BSDF_REFLECT)
    assert s.add_material_state(st) == 1
    for extra in (0x1, 0x40, 0x80):  # BSDF_SPECULAR, BSDF_FILTER, BSDF_EMIT
        st.bsdf_flags = G.BSDF_DIFFUSE | G.BSDF_REFLECT | extra
        with pytest.raises(A.YkError) as e:
            s.add_material_state(st)
        assert e.value.code == A.YK_ERR_ARG
