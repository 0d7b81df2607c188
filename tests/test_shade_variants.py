"""Every cell of the shading-kernel table (kShade, yk_device_host.inc):
material level {diffuse-only, general, glossy, coated} x light level {area light only,
+ a spot light, + a mesh light}, under integrator settings that between them
launch every kernel the table holds.

One scene per (light level, setting): the 36-triangle Cornell box at 32 x 32,
one AA sample. Its four material levels must give the same film bits and ray
counts:
  diffuse-only / general   the same scene with YK_DIFF unset / YK_DIFF=0 at
                           upload (the mirror settings are general already);
  glossy / coated          the same scene plus an unreferenced glossy or
                           coated_glossy material, which moves the scene to the
                           GL kernels; these do the same float operations on
                           shinydiffuse surfaces.
With the area light alone the general film also equals the oracle's, except
under direct lighting with AO: the oracle has no ambient occlusion (and knows
neither spot nor mesh lights), so those cells are compared with each other
only. Photon maps are refused for scenes with a spot or a mesh light, so the
photon settings exist at the first light level only; the table's photon
entries do not depend on the light level.
"""
import ctypes as C

import numpy as np
import pytest

from core_amd import _abi as A
from core_amd.scene import Scene

gpu = pytest.mark.gpu
RES = 32
F = np.float32
QUAD = np.array([[0, 1, 2], [0, 2, 3]], np.int32)

LIGHTS = ("area", "spot", "mesh")
# setting -> (mirror surface in the scene, needs photon maps, kernels of the table it launches)
SETTINGS = {
    "pt": (False, False, "primary[0], bounce, path_start"),
    "dl_ao": (False, False, "primary[1]"),
    "pt_mirror": (True, False, "primary[0], bounce, path_start, spawn"),
    "pm_fg": (False, True, "photon_hit, primary[0], fg_start, fg_hit, pm_finish"),
    "pm_direct": (False, True, "photon_hit, primary[0], pm_post, pm_finish"),
    "pt_mirror_cphot": (True, True, "photon_hit, primary[0], bounce, pt_caustic, spawn"),
}
CELLS = [(l, s) for l in LIGHTS for s, (_, photons, _) in SETTINGS.items() if l == "area" or not photons]


def _scene(light, mirror, extra):
    """extra: None, or the type of a material appended after all others that no triangle uses"""
    s = Scene()
    p = s.generate("cornell_pt", RES, RES)
    if mirror:  # in front of the back wall, under the light: seen by the camera, met by photons
        m = s.add_material(color=(1, 1, 1), diffuse_reflect=0.2, specular_reflect=0.8, mirror_color=(0.9, 0.9, 0.8))
        s.add_mesh(np.array([[-0.9, 1.2, 0.99], [0.9, 1.2, 0.99], [0.9, 1.9, 0.99], [-0.9, 1.9, 0.99]], F), QUAD, m)
    if light == "spot":
        s.add_spot_light((0.3, 1.8, -0.4), (0.0, 0.0, 0.2), (1, 0.9, 0.8), 3.0, cone_angle=40, blend=0.3,
                         soft_shadows=True, samples=2)
    elif light == "mesh":
        lm = s.add_material(type_=A.YK_MAT_LIGHT, color=(1.0, 0.9, 0.8), power=2.0)
        lid = s.add_mesh(np.array([[-0.9, 1.0, 0.2], [-0.9, 1.4, 0.2], [-0.9, 1.4, 0.6], [-0.9, 1.0, 0.6]], F), QUAD, lm)
        s.add_mesh_light(lid, color=(1.0, 0.9, 0.8), power=2.0, samples=2, double_sided=True)
    if extra is not None:
        s.add_material(type_=extra, color=(0.9, 0.9, 0.9), diffuse_reflect=0.5, diffuse_color=(0.8, 0.3, 0.3))
    s.build()
    return s, p


def _params(p, setting):
    q = p.copy()
    q.aa_samples, q.tile_size = 1, 16
    if setting == "dl_ao":
        q.integrator = A.YK_INTEGRATOR_DIRECT
        q.do_ao, q.ao_samples, q.ao_distance = 1, 4, 1.0
    elif setting.startswith("pt"):
        q.integrator, q.bounces = A.YK_INTEGRATOR_PATH, 2
        q.path_samples = 2  # the second sub-path starts in k_path_start
        if setting == "pt_mirror_cphot":
            q.caustic_type = A.YK_CAUSTIC_BOTH
            q.photon.caustic_photons = 4000
    else:
        q.integrator = A.YK_INTEGRATOR_PHOTON
        q.photon.photons = 2000
        q.photon.final_gather = 1 if setting == "pm_fg" else 0
        q.photon.fg_samples, q.photon.fg_bounces = 2, 1
    return q


def _shading_kind(dev):
    k = C.c_int32(-1)
    A.check(A.lib().yk_debug_shading_kind(dev._p, C.byref(k)))
    return k.value


def _render(dev, s, q, photons):
    dev.upload(s)
    info = dev.photon_build(q) if photons else None
    film = dev.new_film(q)
    st = dev.render_shard(q, film)
    return film.cpu().numpy(), (st.closest_rays, st.shadow_rays), info


@gpu
@pytest.mark.parametrize("light,setting", CELLS, ids=[f"{l}-{s}" for l, s in CELLS])
def test_material_levels_give_the_same_film(gpu_device, monkeypatch, light, setting):
    mirror, photons, _ = SETTINGS[setting]
    monkeypatch.setenv("YK_DEBUG_HOOKS", "1")
    s, p = _scene(light, mirror, None)
    q = _params(p, setting)
    monkeypatch.setenv("YK_DIFF", "0")
    want, rays, info = _render(gpu_device, s, q, photons)
    assert _shading_kind(gpu_device) == 0
    assert np.isfinite(want).all() and want[..., :3].max() > 0 and rays[0] >= RES * RES and rays[1] > 0
    if setting not in ("dl_ao", "pm_direct"):  # these two trace camera and shadow rays only
        assert rays[0] > RES * RES  # bounce, gather or recursion rays beyond the camera's
    if setting == "pt_mirror_cphot":
        assert info.caustic_photons > 0  # an empty caustic map launches no k_pt_caustic
    if light == "area" and setting != "dl_ao":
        from oracle.oracle import Oracle
        orc = Oracle(s)
        if photons:
            orc.photon_build(q)
        _, sums_o, cnt = orc.render(q)
        assert rays == (cnt["closest"], cnt["shadow"])
        assert (want.view(np.uint32) == sums_o.view(np.uint32)).all(), "the general form differs from the oracle"
    monkeypatch.delenv("YK_DIFF")
    levels = [("glossy", A.YK_MAT_GLOSSY), ("coated", A.YK_MAT_COATED_GLOSSY)]
    if not mirror:
        levels.insert(0, ("diffuse-only", None))
    for name, extra in levels:
        t = s if extra is None else _scene(light, mirror, extra)[0]
        film, r, _ = _render(gpu_device, t, q, photons)
        assert _shading_kind(gpu_device) == (1 if extra is None else 0), name
        bad = (film.view(np.uint32) != want.view(np.uint32)).any(-1)
        print(f"{light} {setting} {name}: {bad.sum()} of {bad.size} pixels differ from the general form; rays {r} / {rays}")
        assert r == rays, name
        assert not bad.any(), f"{name}: {bad.sum()} pixels differ, first {np.argwhere(bad)[0]}"
