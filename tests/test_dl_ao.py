"""Direct lighting's ambient occlusion (directlight.cc:142,
mcIntegrator_t::sampleAmbientOcclusion mcintegrator.cc:629-683).

The CPU oracle has no AO, so the GPU film is checked against a float32 numpy
restatement in source order (tests/dl_common.py) built on the oracle's camera
rays, hits and isShadowed, on the pixels of a box-filtered film that hold
only their own samples (weight == spp); and against the oracle's no-AO film
where AO must add exactly +0. Parity with the compiled (-ffast-math)
reference: unpinned.
"""
import ctypes as C

import numpy as np
import pytest

from core_amd import _abi as A
from core_amd.scene import Scene, probe_scene
from oracle import oracle as O
from oracle.oracle import Oracle
from tests import dl_common as D
from tests.scenes import uv_sphere

RES = 48
# offsets of yk_render_params as the parent commit's ctypes struct had them
PARENT_OFFSETS = {'integrator': 0, 'raydepth': 4, 'path_samples': 8, 'bounces': 12, 'caustic_type': 16, 'width': 20,
                  'height': 24, 'xstart': 28, 'ystart': 32, 'aa_samples': 36, 'aa_passes': 40, 'filter': 44,
                  'aa_pixelwidth': 48, 'tile_size': 52, 'transp_background': 56, 'aa_inc_samples': 60,
                  'aa_threshold': 64, 'photon': 68, 'transp_shadows': 120, 'shadow_depth': 124, 'filter_width': 128,
                  'tile_order': 136, 'tile_order_len': 144}

_CACHE = {}


def scene(kind, res=RES):
    key = (kind, res)
    if key not in _CACHE:
        s = {"box": lambda: D.ao_scene(res), "pane": lambda: D.ao_scene(res, pane=True),
             "emit": lambda: D.ao_scene(res, emit=0.4), "closed": lambda: D.closed_box_scene(res)}[kind]()
        _CACHE[key] = (s, Oracle(s))
    return _CACHE[key]


# ---- CPU ------------------------------------------------------------------

def test_struct_layout_and_defaults():
    for name, off in PARENT_OFFSETS.items():
        assert getattr(A.yk_render_params, name).offset == off, name
    assert A.yk_render_params.do_ao.offset >= PARENT_OFFSETS["tile_order_len"] + 4
    p = A.yk_render_params()
    A.lib().yk_render_params_default(C.byref(p))
    assert (p.do_ao, p.ao_samples, p.ao_distance, tuple(p.ao_color), p.dl_caustics) == (0, 32, 1.0, (1.0, 1.0, 1.0), 0)
    z = A.yk_render_params()
    assert z.do_ao == 0 and z.dl_caustics == 0


@pytest.mark.parametrize("K,ao", [(8, 32), (0, 1), (94, 3)])
def test_batch_plan_covers_the_ao_slots(monkeypatch, K, ao):
    """AO slots take the split form with the lights' slots: per sample 34 B
    per slot (16-B direction record, contribution, flag, result, queue entry)
    and one 16-B origin, within what the plan reports."""
    monkeypatch.setenv("YK_DEBUG_HOOKS", "1")
    slots = K + ao
    pin = A.yk_batch_plan_in(slots=slots, split=1, tile=16, spp=3, pipes=4, owned_tiles=9, budget_bytes=64 << 30)
    plan = A.yk_batch_plan()
    A.check(A.lib().yk_debug_batch_plan(C.byref(pin), C.byref(plan)))
    assert plan.status == A.YK_OK and plan.maxc >= 16 * 16 * 3
    assert plan.bytes_per_sample >= 34 * slots + 16
    pin.split, pin.transp_shadows = 0, 1  # whole rays (transparent shadows have no split form): 50 + 28 B per slot
    A.check(A.lib().yk_debug_batch_plan(C.byref(pin), C.byref(plan)))
    assert plan.bytes_per_sample >= 78 * slots
    assert plan.maxc * slots < 2 ** 31


@pytest.mark.parametrize("kind", ["box", "pane"])
def test_box_filter_premise(kind):
    s, orc = scene(kind)
    for spp in (1, 3):
        _, sums, _ = orc.render(D.params(RES, spp))
        share = float((sums[..., 4] == spp).mean())
        print(f"{kind} spp {spp}: {share:.3f} of the pixels have weight == spp")
        assert share >= 0.9


def test_numpy_fsin_is_the_oracles():
    L = O.lib()
    L.orc_fcos.restype = C.c_float
    L.orc_fcos.argtypes = [C.c_float]
    x = np.concatenate([np.linspace(-7, 7, 2001), np.linspace(0, 2 * np.pi, 2001)]).astype(np.float32)
    assert D.bits_equal(D.fsin(x), np.array([L.orc_fsin(float(v)) for v in x], np.float32)).all()
    assert D.bits_equal(D.fcos(x), np.array([L.orc_fcos(float(v)) for v in x], np.float32)).all()


# ---- GPU ------------------------------------------------------------------

def render(dev, p, shard=(0, 1)):
    film = dev.new_film(p)
    st = dev.render_shard(p, film, *shard)
    return film.cpu().numpy(), st


def check_restated(dev, kind, spp, n, dist, color=(0.9, 1.0, 0.8), ts=False):
    s, orc = scene(kind)
    p = D.with_ao(D.params(RES, spp), n, dist, color, transp_shadows=int(ts), shadow_depth=3)
    dev.upload(s)
    film, st = render(dev, p)
    r = D.restate_ao(orc, s, p, n, dist, color, ts_depth=3 if ts else None)
    own = film[..., 4] == spp
    assert own.mean() >= 0.9
    want = D.film_of(r["col"], p)
    bad = ~D.bits_equal(film[..., :3], want).all(axis=2) & own
    err = np.abs(film[..., :3] - want)[own].max()
    print(f"{kind} spp {spp} n {n} dist {dist}: {own.sum()} pixels, {bad.sum()} differ, max abs {err:.3g}, "
          f"occluded {r['occ'].mean():.3f}, film max {want.max():.3g}")
    assert not bad.any()
    assert want.max() > 0
    assert st.shadow_rays == n * r["hits"] == r["nrays"]
    assert (st.shadow_nodes, st.shadow_tris) == (int(r["cnt"][0]), int(r["cnt"][1]))
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("spp,n,dist", [(1, 1, 1.5), (3, 3, 1.5), (1, 32, 1.5), (3, 32, 0.2), (1, 3, 0.2)])
def test_gpu_ao_equals_the_restatement(gpu_device, spp, n, dist):
    r = check_restated(gpu_device, "box", spp, n, dist)
    if n == 32:  # the short rays end inside the 0.3 gap under the box, the long ones reach it
        assert (r["occ"].mean() > 0.02) == (dist > 0.3)


@pytest.mark.gpu
def test_gpu_ao_on_an_emitting_material(gpu_device):
    """emit * s.pdf ahead of every sample's term, on the box's hits"""
    check_restated(gpu_device, "emit", 3, 5, 1.5)


@pytest.mark.gpu
def test_gpu_ao_transparent_shadows(gpu_device):
    s, _ = scene("pane")
    r = check_restated(gpu_device, "pane", 3, 8, 1.5, ts=True)
    # the pane lets every ray through, filtered by getTransparency: T * (f * color + (1 - f))
    m = s.material_states()[1]
    F = np.float32
    acc = F(m.component[1]) * F(1.0)
    T = np.array([acc * (F(m.transmit_filter) * F(c) + (F(1.0) - F(m.transmit_filter))) for c in m.color], F)
    f = r["filt"].reshape(-1, 3)
    through = ~D.bits_equal(f, np.ones(3, F)).all(axis=1)
    assert through.any() and not r["occ"].any()
    assert D.bits_equal(f[through], T).all()


@pytest.mark.gpu
def test_gpu_ao_adds_exactly_zero(gpu_device):
    """ao_color 0, and every AO ray occluded: the oracle's no-AO film."""
    s, p0 = probe_scene("cornell_dl", RES, RES)
    orc = Oracle(s)
    p0.tile_size = 16
    _, sums_o, cnt = orc.render(p0)
    gpu_device.upload(s)
    rays = orc.camera_rays(p0.xstart, p0.ystart, p0.width, p0.height, p0.aa_samples)
    prim = orc.intersect(rays)[0]
    ms = s.material_states()
    hits = sum(bool(ms[m].bsdf_flags & D.BSDF_DIFFUSE) for m in orc.arrays["tri_material"][prim[prim >= 0]])
    film, st = render(gpu_device, D.with_ao(p0, 5, 0.7, (0, 0, 0)))
    assert D.bits_equal(film, sums_o).all()
    assert st.shadow_rays == cnt["shadow"] + 5 * hits and hits > 0
    s, orc = scene("closed")
    p = D.params(RES, 2)
    _, sums_o, cnt = orc.render(p)
    assert sums_o[..., :3].max() > 0
    gpu_device.upload(s)
    film, st = render(gpu_device, D.with_ao(p, 7, 6.0))
    assert D.bits_equal(film, sums_o).all()
    assert st.shadow_rays == cnt["shadow"] + 7 * RES * RES * 2


def mirror_scene(res):
    s = Scene()
    p = s.generate("cornell_dl", res, res)
    m = s.add_material(color=(1, 1, 1), diffuse_reflect=0.0, specular_reflect=1.0, mirror_color=(0.95, 0.9, 0.8))
    pts, faces, nrm = uv_sphere(16, 10, 0.45, (0.0, 0.9, 0.0))
    oid = s.add_mesh(pts, faces, m)
    s.set_mesh_normals(oid, nrm, faces, smooth=True)
    s.build()
    p.raydepth, p.tile_size = 3, 16
    return s, p, m


@pytest.mark.gpu
def test_gpu_ao_at_specular_recursion_nodes(gpu_device):
    s, p, m = mirror_scene(RES)
    orc = Oracle(s)
    _, sums_o, _ = orc.render(p)
    gpu_device.upload(s)
    film, _ = render(gpu_device, D.with_ao(p, 4, 0.8))
    zero, _ = render(gpu_device, D.with_ao(p, 4, 0.8, (0, 0, 0)))
    assert D.bits_equal(zero, sums_o).all()
    rays = orc.camera_rays(p.xstart, p.ystart, p.width, p.height, p.aa_samples)
    prim = orc.intersect(rays)[0].reshape(p.height, p.width, p.aa_samples)
    mat = np.where(prim >= 0, orc.arrays["tri_material"][np.maximum(prim, 0)], -1)
    inside = (mat == m).all(axis=2) & (film[..., 4] == p.aa_samples)
    assert inside.sum() > 20
    # the mirror has no diffuse component: what changes in its image was added
    # at recursion nodes. Reflected rays that leave through the open front or
    # meet the light have no diffuse node, so no share of the image is implied:
    # some pixels gain, none loses.
    more = (film[..., :3] > sums_o[..., :3]).any(axis=2)
    print(f"mirror image: {inside.sum()} pixels, {more[inside].sum()} gain from AO at recursion nodes")
    assert more[inside].any()
    assert (film[..., :3] >= sums_o[..., :3])[inside].all()


@pytest.mark.gpu
def test_gpu_ao_form_invariance(gpu_device, monkeypatch):
    monkeypatch.setenv("YK_DEBUG_HOOKS", "1")
    for k in ("YK_PIPES", "YK_BATCH_SAMPLES", "YK_SPLIT", "YK_SMALL"):
        monkeypatch.delenv(k, raising=False)
    s, p0 = probe_scene("cornell_dl", RES, RES)
    p0.tile_size, p0.filter, p0.aa_pixelwidth, p0.aa_samples = 16, A.YK_FILTER_BOX, 1.0, 2
    p = D.with_ao(p0, 6, 0.6, (0.5, 0.6, 0.7))
    gpu_device.upload(s)
    form = C.c_int32(-1)
    A.check(A.lib().yk_debug_shadow_form(gpu_device._p, C.byref(p), C.byref(form)))
    assert form.value == 1  # 8 light slots + 6: the split form
    base, st0 = render(gpu_device, p)
    noao, _ = render(gpu_device, p0)
    assert not D.bits_equal(base, noao).all()
    for env in ({"YK_BATCH_SAMPLES": str(16 * 16 * 2)}, {"YK_PIPES": "1"}, {"YK_PIPES": "4"}, {"YK_SPLIT": "0"},
                {"YK_SPLIT": "1"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        film, st = render(gpu_device, p)
        for k in env:
            monkeypatch.delenv(k)
        assert D.bits_equal(film, base).all(), env
        assert (st.shadow_rays, st.shadow_nodes, st.shadow_tris) == (st0.shadow_rays, st0.shadow_nodes, st0.shadow_tris)
    for small in ("0", "1"):  # read at upload
        monkeypatch.setenv("YK_SMALL", small)
        gpu_device.upload(s)
        film, _ = render(gpu_device, p)
        assert D.bits_equal(film, base).all(), small
    monkeypatch.delenv("YK_SMALL")
    gpu_device.upload(s)
    # shards: tile interiors hold one shard's samples only
    a, _ = render(gpu_device, p, (0, 2))
    b, _ = render(gpu_device, p, (1, 2))
    yy, xx = np.mgrid[0:RES, 0:RES]
    interior = ((yy % 16 >= 2) & (yy % 16 < 14) & (xx % 16 >= 2) & (xx % 16 < 14))
    assert D.bits_equal(a + b, base)[interior].all()
    # two handles on one GPU
    from core_amd.device import Device
    d2 = Device(0)
    try:
        d2.upload(s)
        multi, _ = Device.render_multi([gpu_device, d2], p)
        assert D.bits_equal(multi, a + b).all()
    finally:
        d2.close()
    # adaptive passes, twice
    q = D.with_ao(p0, 6, 0.6, (0.5, 0.6, 0.7), aa_passes=2, aa_inc_samples=1, aa_threshold=0.01)
    f1, s1 = render(gpu_device, q)
    f2, s2 = render(gpu_device, q)
    assert D.bits_equal(f1, f2).all() and s1.shadow_rays == s2.shadow_rays > st0.shadow_rays


@pytest.mark.gpu
def test_gpu_ao_refusals(gpu_device):
    s, p0 = probe_scene("cornell_dl", 32, 32)
    orc = Oracle(s)
    gpu_device.upload(s)
    _, sums_o, _ = orc.render(p0)

    def refused(q, code):
        with pytest.raises(A.YkError) as e:
            render(gpu_device, q)
        assert e.value.code == code
        film, _ = render(gpu_device, p0)  # a normal render still succeeds
        assert D.bits_equal(film, sums_o).all()

    refused(D.with_ao(p0, 0, 1.0), A.YK_ERR_ARG)
    refused(D.with_ao(p0, 4, 0.0), A.YK_ERR_ARG)
    refused(D.with_ao(p0, 4, float("nan")), A.YK_ERR_ARG)
    refused(D.with_ao(p0, 8192, 1.0), A.YK_ERR_UNSUPPORTED)
    # the fields belong to direct lighting alone
    s, p1 = probe_scene("cornell_pt", 32, 32)
    gpu_device.upload(s)
    a, _ = render(gpu_device, p1)
    b, _ = render(gpu_device, D.with_ao(p1, 4, 1.0))
    assert D.bits_equal(a, b).all()
    p2 = p1.copy()
    p2.integrator = A.YK_INTEGRATOR_PHOTON
    p2.photon.photons, p2.photon.fg_samples = 5000, 2
    gpu_device.photon_build(p2)
    a, _ = render(gpu_device, p2)
    b, _ = render(gpu_device, D.with_ao(p2, 4, 1.0))
    assert D.bits_equal(a, b).all()
