"""Direct lighting's photon caustics (directlight.cc:78-83,137-141): the
caustic map of mcIntegrator_t::createCausticMap, built by yk_photon_build for
YK_INTEGRATOR_DIRECT with dl_caustics, and col += estimateCausticPhotons on
diffuse hits.

The CPU oracle has the estimate under path tracing only. On a scene where the
path term is exactly +0 (the premise test) its path-traced film with
caustic_type photon is what direct lighting with caustics must give.
"""
import numpy as np
import pytest

from core_amd import _abi as A
from oracle.oracle import Oracle
from tests import dl_common as D
from tests.scenes import specular

RES = 48
_CACHE = {}


def pin_scene():
    if "pin" not in _CACHE:
        s = D.caustic_pin_scene(RES)
        _CACHE["pin"] = (s, Oracle(s))
    return _CACHE["pin"]


def photon(p, **kw):
    q = p.copy()
    ph = q.photon
    # the sphere fills about 1 % of the point light's sphere of directions
    ph.caustic_photons, ph.caustic_radius, ph.caustic_mix, ph.bounces = 200000, 0.15, 30, 10
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def dl(p, caustics=1, **kw):
    return photon(p, integrator=A.YK_INTEGRATOR_DIRECT, dl_caustics=caustics, **kw)


def pt(p, ctype, **kw):
    return photon(p, integrator=A.YK_INTEGRATOR_PATH, caustic_type=ctype, bounces=1, path_samples=1, **kw)


def render(dev, p, shard=(0, 1)):
    film = dev.new_film(p)
    st = dev.render_shard(p, film, *shard)
    return film.cpu().numpy(), st


def test_caustic_pin_premise():
    """Bounce rays from the floor escape or meet the mirror sphere: the path
    term is +0, and the oracle's direct-lighting film is its path-traced one."""
    s, orc = pin_scene()
    p = D.params(RES, 2)
    _, a, ca = orc.render(dl(p, 0))
    _, b, _ = orc.render(pt(p, A.YK_CAUSTIC_NONE))
    assert not np.isnan(a).any() and not np.isnan(b).any()
    assert (a == b).all() and a[..., :3].max() > 0
    assert ca["shadow"] > 0


@pytest.mark.gpu
def test_gpu_dl_caustic_map_is_pathtracings(gpu_device):
    s, orc = pin_scene()
    p = D.params(RES, 2)
    gpu_device.upload(s)
    i_pt = gpu_device.photon_build(pt(p, A.YK_CAUSTIC_PHOTON))
    m_pt = gpu_device.photon_map(A.YK_PHOTON_MAP_CAUSTIC)
    i_dl = gpu_device.photon_build(dl(p))
    m_dl = gpu_device.photon_map(A.YK_PHOTON_MAP_CAUSTIC)
    i_o = orc.photon_build(pt(p, A.YK_CAUSTIC_PHOTON))
    m_o = orc.photon_map(A.YK_PHOTON_MAP_CAUSTIC)
    assert m_dl.shape == m_pt.shape == m_o.shape and len(m_dl) > 100
    assert D.bits_equal(m_dl, m_pt).all() and D.bits_equal(m_dl, m_o).all()
    for f in ("caustic_photons", "caustic_paths", "diffuse_photons", "radiance_photons", "seed_out", "photon_rays"):
        assert getattr(i_dl, f) == getattr(i_pt, f) == i_o[f], f


@pytest.mark.gpu
def test_gpu_dl_caustic_film_pin(gpu_device):
    s, orc = pin_scene()
    p = D.params(RES, 2)
    gpu_device.upload(s)
    gpu_device.photon_build(dl(p))
    film, st = render(gpu_device, dl(p))
    orc.photon_build(pt(p, A.YK_CAUSTIC_PHOTON))
    _, want, _ = orc.render(pt(p, A.YK_CAUSTIC_PHOTON))
    _, plain, cnt = orc.render(dl(p, 0))
    assert not np.isnan(film).any()
    assert (film == want).all()
    assert (want != plain).any()  # photons landed
    assert (st.closest_rays, st.shadow_rays) == (cnt["closest"], cnt["shadow"])


@pytest.mark.gpu
def test_gpu_dl_caustics_at_recursion_nodes(gpu_device):
    s, p0 = specular(RES, 40, "cornell_pt", raydepth=3, caustic=True)
    p0.tile_size, p0.filter, p0.aa_pixelwidth, p0.aa_samples = 16, A.YK_FILTER_BOX, 1.0, 2
    q, q0 = dl(p0), dl(p0, 0)
    gpu_device.upload(s)
    plain, st0 = render(gpu_device, q0)
    _, want0, _ = Oracle(s).render(q0)
    assert D.bits_equal(plain, want0).all()
    info = gpu_device.photon_build(q)
    assert info.caustic_photons > 0
    a, st = render(gpu_device, q)
    b, _ = render(gpu_device, q)
    assert D.bits_equal(a, b).all() and not D.bits_equal(a, plain).all()
    assert (st.closest_rays, st.shadow_rays) == (st0.closest_rays, st0.shadow_rays)
    h0, _ = render(gpu_device, q, (0, 2))
    h1, _ = render(gpu_device, q, (1, 2))
    yy, xx = np.mgrid[0:40, 0:RES]
    interior = ((yy % 16 >= 2) & (yy % 16 < 14) & (xx % 16 >= 2) & (xx % 16 < 14))
    assert D.bits_equal(h0 + h1, a)[interior].all()
    from core_amd.device import Device
    d2 = Device(0)
    try:
        d2.upload(s)
        with pytest.raises(A.YkError) as e:  # the second handle has no maps yet
            Device.render_multi([gpu_device, d2], q)
        assert e.value.code == A.YK_ERR_STATE
        d2.photon_build(q)
        multi, _ = Device.render_multi([gpu_device, d2], q)
        assert D.bits_equal(multi, h0 + h1).all()
    finally:
        d2.close()


@pytest.mark.gpu
def test_gpu_dl_caustic_state_errors(gpu_device):
    s, _ = pin_scene()
    p = D.params(RES, 1)
    gpu_device.upload(s)  # a fresh upload drops the maps

    def state_error(q):
        with pytest.raises(A.YkError) as e:
            render(gpu_device, q)
        assert e.value.code == A.YK_ERR_STATE

    state_error(dl(p))
    with pytest.raises(A.YkError) as e:
        gpu_device.photon_build(dl(p, 0))
    assert e.value.code == A.YK_ERR_ARG
    gpu_device.photon_build(pt(p, A.YK_CAUSTIC_PHOTON))
    state_error(dl(p))  # built for path tracing
    gpu_device.photon_build(dl(p))
    render(gpu_device, dl(p))
    state_error(pt(p, A.YK_CAUSTIC_PHOTON))  # built for direct lighting
    q = dl(p)
    q.photon.caustic_mix = 31
    state_error(q)
    render(gpu_device, dl(p, 0))  # without the option no maps are needed


@pytest.mark.gpu
def test_gpu_dl_lights_caustics_and_ao_add_up(gpu_device):
    """film = (DL + caustics) + AO: against the two films rendered apart the
    third term costs two more roundings per sample."""
    s, _ = pin_scene()
    spp = 2
    p = D.params(RES, spp)
    gpu_device.upload(s)
    gpu_device.photon_build(dl(p))
    all3 = D.with_ao(dl(p), 5, 1.2, (0.6, 0.7, 0.8))
    a, _ = render(gpu_device, all3)
    b, _ = render(gpu_device, all3)
    assert D.bits_equal(a, b).all()
    two, _ = render(gpu_device, dl(p))
    gpu_device.upload(D.caustic_pin_scene(RES, light=False))  # the same geometry without its light
    ao, _ = render(gpu_device, D.with_ao(D.params(RES, spp), 5, 1.2, (0.6, 0.7, 0.8)))
    assert ao[..., :3].max() > 0
    err = np.abs(a[..., :3].astype(np.float64) - two[..., :3] - ao[..., :3])
    bound = 4 * spp * 2.0 ** -24 * float(np.abs(a[..., :3]).max())
    print(f"max |film - (DL + caustic) - AO| {err.max():.3g}, bound {bound:.3g}")
    assert err.max() <= bound
