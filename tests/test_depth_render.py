"""The depth channel, premultiplied alpha and clamp_rgb on rendered frames
(48 x 32, 16-pixel tiles).

Depth films against the float32 splat (tests/depth_common.py) of the oracle's
per-sample camera-hit t -- its camera rays and intersect, as
tests/dl_common.restate_ao obtains them -- bit for bit; yk_depth_range against
numpy's min and max over the device's own camera rays at the transposed
positions, traced by yk_trace_closest; the colour film and the ray counts
untouched by z_channel; the multi-device reduce, the adaptive passes and the
refusals.
"""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before libyk: one HIP runtime)

from core_amd import _abi as A
from core_amd.device import Device
from core_amd.scene import Scene, probe_scene
from oracle import oracle as O
from tests import depth_common as D
from tests import dl_common as DL

F32 = np.float32
pytestmark = pytest.mark.gpu
W, H, TILE = 48, 32, 16


def params(integrator=A.YK_INTEGRATOR_DIRECT, spp=1, pw=1.5, **kw):
    p = DL.params(W, spp, TILE, integrator=integrator, aa_pixelwidth=pw)
    p.width, p.height = W, H
    p.bounces, p.path_samples, p.caustic_type = 2, 1, A.YK_CAUSTIC_NONE
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def depth_scene(near_clip=0.0, far_clip=-1.0, type=A.YK_CAMERA_PERSPECTIVE):
    """a tilted parallelogram 3.5 .. 5 away and a small box 2 .. 2.4 away,
    both narrower than the view: camera rays miss at every edge"""
    s = Scene()
    m = s.add_material(color=(0.8, 0.7, 0.6))
    DL.quad(s, (-1.2, -0.8, 3.5), (-1.2, 0.9, 4.5), (1.0, 0.9, 5.0), (1.0, -0.8, 4.0), m)
    b = np.array([[x, y, z] for x in (-0.3, 0.3) for y in (-0.2, 0.3) for z in (2.0, 2.4)], F32)
    s.add_mesh(b, DL.BOX_FACES, s.add_material(color=(0.4, 0.6, 0.9)))
    s.add_point_light((0.0, 2.0, 0.0), (1.0, 0.9, 0.8), 20.0)
    s.set_camera((0, 0, 0), (0, 0, 1), (0, 1, 0), W, H, focal=1.0, near_clip=near_clip, far_clip=far_clip, type=type)
    s.build()
    return s


def render(dev, p, depth=True, **kw):
    """-> colour film (h, w, 5), depth film (h, w, 2) or None, yk_stats"""
    q = p.copy()
    for k, v in kw.items():
        setattr(q, k, v)
    film = dev.new_film(q)
    dfilm = dev.new_depth_film(q) if depth else None
    st = dev.render_shard(q, film, depth_film=dfilm)
    return film.cpu().numpy(), None if dfilm is None else dfilm.cpu().numpy(), st


def restated_depth(orc, p, spp, **kw):
    """the float32 splat of the oracle's per-sample depth -> (h, w, 2), and the samples"""
    rays = orc.camera_rays(p.xstart, p.ystart, p.width, p.height, spp)
    prim, t, _, _, _ = orc.intersect(rays)
    v = D.sample_depths(rays, prim, t, **kw)
    P = D.render_film(p, O.film_table)
    pixels, rows = D.tile_major(P, np.column_stack([v, D.sample_offsets(p, spp)]), spp)
    zero = np.zeros((p.height, p.width, 2), F32)
    return D.depth_splat32(P, pixels, spp, rows[:, 0], rows[:, 1:3], zero), v, prim


@pytest.mark.parametrize("spp", [1, 3])
@pytest.mark.parametrize("far_clip", [-1.0, 4.2])
def test_raw_depth_film_equals_the_splat_of_the_oracles_hits(gpu_device, spp, far_clip):
    s = depth_scene(far_clip=far_clip)
    gpu_device.upload(s)
    p = params(spp=spp)
    _, depth, st = render(gpu_device, p)
    want, v, prim = restated_depth(O.Oracle(s), p, spp)
    miss = prim < 0
    assert miss.any() and (~miss).any()
    if far_clip < 0:
        assert (v[miss] == D.FAR).all()
    else:  # the far plane cuts the parallelogram: a miss keeps the ray's far-plane tmax
        assert (v[miss] >= F32(far_clip)).all() and (v[miss] < 6).all() and (v[~miss] < v[miss].max()).all()
    assert st.camera_samples == W * H * spp
    assert (D.bits(depth) == D.bits(want)).all()


def test_raw_depth_with_specular_recursion(gpu_device):
    """the recursion's later generations reuse the hit records: the depth is
    taken after the camera rays' own launch"""
    s = DL.caustic_pin_scene(W)
    gpu_device.upload(s)
    p = params(spp=3, ystart=8)
    _, depth, _ = render(gpu_device, p)
    want, _, prim = restated_depth(O.Oracle(s), p, 3)
    assert (prim < 0).any() and (prim >= 0).any()
    assert (D.bits(depth) == D.bits(want)).all()


def camera_rays(dev, px, py):
    """yk_debug_camera_rays (include/yk_test_hooks_camera.h), bound here: the
    hook is not part of the product ABI table -> (n, 8) rays"""
    f = A.lib().yk_debug_camera_rays
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, A.fp, C.c_int64, C.c_void_p, A.fp]
    n = len(px)
    inp = np.full((n, 4), 0.5, F32)
    inp[:, 0], inp[:, 1] = px, py
    rays, wt = np.zeros((n, 8), F32), np.zeros(n, F32)
    A.check(f(dev._p, D.cptr(inp), n, rays.ctypes.data, D.cptr(wt)))
    return rays


def test_depth_range_of_a_clipped_camera_and_its_film(gpu_device):
    s = depth_scene(near_clip=0.5, far_clip=6.0)
    gpu_device.upload(s)
    p = params(spp=3)
    dmin, dinv = gpu_device.depth_range(p)
    assert dmin == F32(0.5) and D.bits(dinv) == D.bits(F32(1.0) / (F32(6.0) - F32(0.5)))
    _, depth, _ = render(gpu_device, p, normalize_z_channel=1, depth_min=dmin, depth_inv_range=dinv)
    want, v, _ = restated_depth(O.Oracle(s), p, 3, normalize=True, dmin=dmin, dinv=dinv)
    assert (v > 0).any() and (v < 1).all()
    assert (D.bits(depth) == D.bits(want)).all()


def test_depth_range_of_an_unclipped_camera_and_its_film(gpu_device, monkeypatch):
    monkeypatch.setenv("YK_DEBUG_HOOKS", "1")
    s = depth_scene()
    gpu_device.upload(s)
    p = params(spp=1)
    # precalcDepths: shootRay(i, j, 0.5, 0.5) for i < resY, j < resX -- the row index as px
    i, j = np.mgrid[0:H, 0:W]
    rays = camera_rays(gpu_device, i.ravel().astype(F32), j.ravel().astype(F32))
    prim, t, _, _ = gpu_device.split_hits(gpu_device.trace_closest(gpu_device.rays_to_device(rays)))
    tmax = np.where(prim >= 0, t, rays[:, 7]).astype(F32)
    assert (prim >= 0).any() and (prim < 0).any() and (tmax[prim < 0] < 0).all()
    hi = max(F32(0.0), tmax.max())
    lo = min(F32(1e38), tmax[tmax >= 0].min())
    dmin, dinv = gpu_device.depth_range(p)
    assert D.bits(dmin) == D.bits(lo) and D.bits(dinv) == D.bits(F32(1.0) / (hi - lo))
    _, depth, _ = render(gpu_device, p, normalize_z_channel=1, depth_min=dmin, depth_inv_range=dinv)
    want, v, prim = restated_depth(O.Oracle(s), p, 1, normalize=True, dmin=dmin, dinv=dinv)
    assert (v[prim < 0] == 0).all()  # far_clip -1: a miss has tmax < 0
    assert (D.bits(depth) == D.bits(want)).all()
    # an infinite maxDepth is taken as the reference takes it
    _, depth, _ = render(gpu_device, p, normalize_z_channel=1, depth_min=dmin, depth_inv_range=float("inf"))
    want, _, _ = restated_depth(O.Oracle(s), p, 1, normalize=True, dmin=dmin, dinv=F32(np.inf))
    assert ((D.bits(depth) == D.bits(want)) | (np.isnan(depth) & np.isnan(want))).all()


def test_depth_range_of_a_circular_angular_camera_is_refused(gpu_device):
    s = depth_scene(type=A.YK_CAMERA_ANGULAR)
    gpu_device.upload(s)
    with pytest.raises(A.YkError) as e:
        gpu_device.depth_range(params())
    assert e.value.code == A.YK_ERR_UNSUPPORTED
    # its samples outside the circle take no depth sample and no depth weight
    p = params(spp=1, pw=1.0)
    film, depth, st = render(gpu_device, p)
    assert 0 < st.camera_samples < W * H
    assert (depth[..., 1] <= film[..., 4]).all() and (depth[..., 1] < film[..., 4]).any()
    assert depth[..., 1].sum() == st.camera_samples  # box 1.0: every weight is 1, the sums are exact


@pytest.mark.parametrize("integrator", ["path", "direct", "photon"])
def test_z_channel_leaves_the_colour_film_and_the_ray_counts_alone(gpu_device, integrator):
    s, p = probe_scene("cornell_pt", W, H)
    gpu_device.upload(s)
    p.aa_samples, p.tile_size, p.bounces = 2, TILE, 2
    if integrator == "direct":
        p.integrator = A.YK_INTEGRATOR_DIRECT
    elif integrator == "photon":  # a tiny map
        p.integrator = A.YK_INTEGRATOR_PHOTON
        p.photon.photons, p.photon.fg_samples = 3000, 2
        gpu_device.photon_build(p)
    off, _, st0 = render(gpu_device, p, depth=False)
    on, depth, st1 = render(gpu_device, p)
    assert (D.bits(on) == D.bits(off)).all()
    for k in ("closest_rays", "shadow_rays", "camera_samples", "closest_launches", "shadow_launches"):
        assert getattr(st0, k) == getattr(st1, k), k
    assert (D.bits(depth[..., 1]) == D.bits(on[..., 4])).all() and (depth[..., 0] > 0).all()


def test_premultiplied_render_is_rgb_times_alpha(gpu_device):
    """box 1.0 at spp 1: each sample covers its own pixel alone, m = 1"""
    s = depth_scene()
    gpu_device.upload(s)
    p = params(spp=1, pw=1.0)
    film, _, _ = render(gpu_device, p, depth=False)
    pre, _, _ = render(gpu_device, p, depth=False, premult_alpha=1)
    assert (film[..., 4] == 1).all() and (film[..., 3] == 0).any() and (film[..., 3] == 1).any()
    assert (D.bits(pre[..., :3]) == D.bits(film[..., :3] * film[..., 3:4])).all()
    assert (D.bits(pre[..., 3:]) == D.bits(film[..., 3:])).all()
    # yk_film_resolve premultiplies once more, after its clamp
    q = p.copy()
    q.premult_alpha = 1
    d_film = torch.from_numpy(pre).to(gpu_device.torch_device)
    assert (D.bits(gpu_device.film_resolve(q, d_film).cpu().numpy()) == D.bits(D.resolve32(pre, premult=True))).all()
    assert (D.bits(gpu_device.film_resolve(p, d_film).cpu().numpy()) == D.bits(D.resolve32(pre))).all()


def test_clamp_rgb_on_a_visible_light(gpu_device):
    s, p = probe_scene("cornell_pt", W, H)
    gpu_device.upload(s)
    p.aa_samples, p.tile_size, p.bounces, p.aa_pixelwidth = 1, TILE, 2, 1.0
    film, _, _ = render(gpu_device, p, depth=False)
    cl, _, _ = render(gpu_device, p, depth=False, clamp_rgb=1)
    assert (film[..., 4] == 1).all() and (film[..., :3] > 1).any()  # the light itself
    # weight 1, one sample per pixel: the film is the sample, so the clamped film is its clamp
    assert (D.bits(cl) == D.bits(D.clamp01(film.reshape(-1, 5)).reshape(film.shape))).all()
    # and with overlapping footprints no normalised channel exceeds 1
    cl3, _, _ = render(gpu_device, p, depth=False, clamp_rgb=1, aa_samples=3, aa_pixelwidth=1.5)
    raw3, _, _ = render(gpu_device, p, depth=False, aa_samples=3, aa_pixelwidth=1.5)
    assert (D.resolve32(raw3)[..., :3] > 1).any()
    assert (cl3[..., :3] <= cl3[..., 4:5]).all()  # sums of w * c with c <= 1 against the sum of w, w >= 0


def test_resolves_equal_numpy(gpu_device):
    from tests import film_cases as FC
    film = FC.resolve_film(w=W, h=H)
    p = params()
    d_depth = torch.from_numpy(np.ascontiguousarray(film[..., [0, 4]])).to(gpu_device.torch_device)
    z = gpu_device.depth_resolve(p, d_depth).cpu().numpy()
    assert (D.bits(z) == D.bits(D.depth_resolve32(film[..., [0, 4]]))).all()
    q = p.copy()
    q.premult_alpha = 1
    rgba = gpu_device.film_resolve(q, torch.from_numpy(film).to(gpu_device.torch_device)).cpu().numpy()
    assert (D.bits(rgba) == D.bits(D.resolve32(film, premult=True))).all()


def test_multi_device_depth_is_the_shard_order_sum(gpu_device):
    s = depth_scene()
    gpu_device.upload(s)
    second = Device(0)
    try:
        second.upload(s)
        p = params(spp=3, z_channel=1)
        film, st = Device.render_multi([gpu_device, second], p)
        parts = []
        for k in range(2):
            f, dpt = gpu_device.new_film(p), gpu_device.new_depth_film(p)
            gpu_device.render_shard(p, f, shard=k, nshards=2, depth_film=dpt)
            parts.append((f.cpu().numpy(), dpt.cpu().numpy()))
        assert (D.bits(st.depth_film) == D.bits(parts[0][1] + parts[1][1])).all()
        assert (D.bits(film) == D.bits(parts[0][0] + parts[1][0])).all()
        assert (parts[0][1][..., 1] > 0).any() and (parts[1][1][..., 1] > 0).any()
        whole, depth, _ = render(gpu_device, p)
        assert np.allclose(st.depth_film, depth, rtol=1e-5)
    finally:
        second.close()


def test_adaptive_passes_add_depth_samples_in_resampled_pixels_only(gpu_device, monkeypatch):
    monkeypatch.setenv("YK_DEBUG_HOOKS", "1")
    s = depth_scene()
    gpu_device.upload(s)
    thr = 0.02
    p = params(spp=1, pw=1.0, aa_passes=2, aa_inc_samples=2, aa_threshold=thr)
    # a threshold nothing reaches: pass 1 resamples no pixel, the films are pass 0's
    film0, depth0, _ = render(gpu_device, p, aa_threshold=1e30)
    film1, depth1, _ = render(gpu_device, p)
    flags = np.zeros((H, W), np.uint8)
    A.check(A.lib().yk_debug_aa_flags(gpu_device._p, D.cptr(film0), W, H, thr, flags.ctypes.data))
    flags = flags.astype(bool)
    assert flags.any() and not flags.all()
    assert (D.bits(depth0[..., 1]) == D.bits(film0[..., 4])).all()
    assert (D.bits(depth1[..., 1]) == D.bits(film1[..., 4])).all()  # as the colour samples are
    grew = depth1[..., 1] - depth0[..., 1]
    assert (grew[flags] >= 2).all()
    # a sample reaches at most the next pixel (filterw 0.501): away from the flagged pixels not a bit moves
    near = np.zeros_like(flags)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            near[max(0, dy):H + min(0, dy), max(0, dx):W + min(0, dx)] |= \
                flags[max(0, -dy):H + min(0, -dy), max(0, -dx):W + min(0, -dx)]
    assert (~near).any()
    assert (D.bits(depth1[~near]) == D.bits(depth0[~near])).all()
    assert (grew[~flags] < 2).all()


def test_refusals(gpu_device):
    s = depth_scene()
    gpu_device.upload(s)
    p = params(z_channel=1)
    film = gpu_device.new_film(p)
    host = np.zeros((H, W, 5), F32)
    L = A.lib()

    def refused():
        rcs = [L.yk_render_shard(gpu_device._p, C.byref(p), 0, 1, C.c_void_p(film.data_ptr()), None),
               L.yk_render_film(gpu_device._p, C.byref(p), 0, 1, D.cptr(host), None)]
        arr = (C.c_void_p * 1)(gpu_device._p.value)
        rcs.append(L.yk_render_multi(arr, 1, C.byref(p), D.cptr(host), None))
        return rcs == [A.YK_ERR_ARG] * 3 and not host.any() and not film.cpu().numpy().any()

    assert refused()  # z_channel without a depth film
    dfilm = gpu_device.new_depth_film(p)
    hdepth = np.zeros((H, W, 2), F32)
    for bad in (float("nan"), float("inf"), -float("inf")):
        p.normalize_z_channel, p.depth_min, p.depth_inv_range = 1, bad, 1.0
        p.depth_film = dfilm.data_ptr()
        assert L.yk_render_shard(gpu_device._p, C.byref(p), 0, 1, C.c_void_p(film.data_ptr()), None) == A.YK_ERR_ARG
        p.depth_film = hdepth.ctypes.data
        assert L.yk_render_film(gpu_device._p, C.byref(p), 0, 1, D.cptr(host), None) == A.YK_ERR_ARG
        assert not dfilm.cpu().numpy().any() and not hdepth.any() and not host.any()
    # yk_render_film and yk_render stay usable: a host depth film, and RGBA alone
    p.normalize_z_channel, p.depth_min = 0, 0.0
    A.check(L.yk_render_film(gpu_device._p, C.byref(p), 0, 1, D.cptr(host), None))
    _, depth, _ = render(gpu_device, params())
    assert (D.bits(hdepth) == D.bits(depth)).all()
    rgba = gpu_device.render(p)
    assert rgba.shape == (H, W, 4) and (D.bits(hdepth) == D.bits(depth)).all()
    assert L.yk_depth_range(gpu_device._p, C.byref(p), None, None) == A.YK_ERR_ARG
    assert L.yk_depth_resolve(gpu_device._p, C.byref(p), None, None) == A.YK_ERR_ARG
