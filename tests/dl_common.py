"""Scenes and the numpy restatement shared by tests/test_dl_ao.py and
tests/test_dl_caustics.py: direct lighting's ambient occlusion
(mcIntegrator_t::sampleAmbientOcclusion, mcintegrator.cc:629-683) restated in
float32 in source order on top of the oracle's camera rays, hits and
isShadowed, and small scenes built through the public scene API.
"""
import ctypes as C

import numpy as np
import torch  # noqa: F401  (before libyk: one HIP runtime, also when these files run alone)

from core_amd import _abi as A
from core_amd.scene import Scene
from oracle import oracle as O
from tests.scenes import uv_sphere

F = np.float32
BSDF_DIFFUSE, BSDF_EMIT = 0x4, 0x80
SHADOW_BIAS = F(0.0005)
BOX_FACES = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1],
                      [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.int32)


def params(res, spp=1, tile=16, **kw):
    p = A.yk_render_params()
    A.lib().yk_render_params_default(C.byref(p))
    p.integrator = A.YK_INTEGRATOR_DIRECT
    p.width = p.height = res
    p.aa_samples = spp
    p.tile_size = tile
    p.filter = A.YK_FILTER_BOX
    p.aa_pixelwidth = 1.0
    p.raydepth = 3
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def with_ao(p, n, dist, color=(1.0, 1.0, 1.0), **kw):
    q = p.copy()
    q.do_ao = 1
    q.ao_samples = n
    q.ao_distance = dist
    q.ao_color = A.f3(*color)
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def quad(s, a, b, c, d, mat):
    return s.add_mesh(np.array([a, b, c, d], np.float32), np.array([[0, 1, 2], [0, 2, 3]], np.int32), mat)


def floor(s, mat, half=2.0, y=0.0):
    """an upward-facing quad"""
    return quad(s, (-half, y, -half), (-half, y, half), (half, y, half), (half, y, -half), mat)


def ao_scene(res, pane=False, emit=0.0):
    """No lights: a Lambert floor and a Lambert box floating 0.3 above it.
    pane: instead of the box a transparent pane 0.4 above the floor's right
    half, outside the narrow view, so no camera ray meets it."""
    s = Scene()
    m = s.add_material(color=(0.8, 0.7, 0.6))
    floor(s, m)
    if pane:
        t = s.add_material(color=(0.9, 0.5, 0.2), diffuse_reflect=0.2, transparency=0.8, transmit_filter=0.6)
        quad(s, (0.6, 0.4, -2), (0.6, 0.4, 2), (2.6, 0.4, 2), (2.6, 0.4, -2), t)
        s.set_camera((0, 2.0, -3.5), (0, 0, 0), (0, 3.0, -3.5), res, res, focal=4.0)
    else:
        m2 = s.add_material(color=(0.4, 0.6, 0.9), diffuse_reflect=0.9, emit=emit)  # emit > 0: emit * s.pdf terms
        b = np.array([[x, y, z] for x in (-0.4, 0.45) for y in (0.3, 1.1) for z in (-0.35, 0.4)], np.float32)
        s.add_mesh(b, BOX_FACES, m2)
        s.set_camera((0.3, 2.0, -3.5), (0, 0.4, 0), (0.3, 3.0, -3.5), res, res, focal=1.3)
    s.build()
    return s


def closed_box_scene(res):
    """Six overlapping walls around the camera and a point light: every AO
    ray of length >= the diagonal (< 5.2) is occluded."""
    s = Scene()
    m = s.add_material(color=(0.7, 0.8, 0.6))
    h, r = 1.0, 1.5
    for ax in range(3):
        for sg in (-1.0, 1.0):
            c = []
            for u, v in ((-r, -r), (-r, r), (r, r), (r, -r)):
                pt = [0.0, 0.0, 0.0]
                pt[ax] = sg * h
                pt[(ax + 1) % 3] = u
                pt[(ax + 2) % 3] = v
                c.append(tuple(pt))
            quad(s, *c, m)
    s.add_point_light((0.3, 0.5, 0.0), (1.0, 0.9, 0.8), 2.0)
    s.set_camera((0, 0, -0.5), (0, 0, 1), (0, 1, -0.5), res, res, focal=0.8)
    s.build()
    return s


def caustic_pin_scene(res, glass=False, light=True):
    """One upward-facing floor quad, one specular sphere above it, one point
    light, no background: bounce rays from the floor escape or meet the
    sphere, which has no diffuse component."""
    s = Scene()
    fm = s.add_material(color=(0.8, 0.8, 0.7))
    if glass:
        sm = s.add_material(color=(0.9, 0.95, 1.0), diffuse_reflect=0.0, transparency=1.0, transmit_filter=0.5)
    else:
        sm = s.add_material(color=(1, 1, 1), diffuse_reflect=0.0, specular_reflect=1.0, mirror_color=(0.9, 0.9, 0.8))
    floor(s, fm, 3.0)
    pts, faces, nrm = uv_sphere(16, 10, 0.5, (0.0, 0.9, 0.0))
    oid = s.add_mesh(pts, faces, sm)
    s.set_mesh_normals(oid, nrm, faces, smooth=True)
    if light:
        s.add_point_light((1.5, 2.5, -0.5), (1.0, 1.0, 0.9), 30.0)
    s.set_camera((0, 3.0, -5.0), (0, 0.2, 0), (0, 4.0, -5.0), res, res, focal=1.5)
    s.build()
    return s


# ---- float32 restatement -------------------------------------------------

def fsin(x):
    """FAST_TRIG fSin (mathOptimizations.h:249-268) as the project states it"""
    x = np.array(x, F)
    two_pi, k2 = F(6.28318530717958647692), np.uint32(0x40c90fda).view(F)
    kp = np.uint32(0x40490fda).view(F)
    m = (x > k2) | (x < -k2)
    x = np.where(m, x - (x * F(0.15915494309189533577)).astype(np.int32).astype(F) * two_pi, x).astype(F)
    x = np.where(x < -kp, x + two_pi, np.where(x > kp, x - two_pi, x)).astype(F)
    x = (F(1.27323954473516268615) * x) - ((F(0.40528473456935108578) * x) * np.abs(x))
    r = x + (np.abs(x) - F(1.0)) * (F(0.225) * x)
    return np.clip(r, F(-1.0), F(1.0)).astype(F)


def fcos(x):
    return fsin(np.array(x, F) + F(1.57079632679489661923))


def dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def create_cs(N):
    """createCS, vector3d.h:316-334"""
    u = np.zeros_like(N)
    v = np.zeros_like(N)
    flat = (N[:, 0] == 0) & (N[:, 1] == 0)
    u[flat, 0] = np.where(N[flat, 2] < 0, F(-1), F(1))
    v[flat, 1] = F(1)
    g = ~flat
    with np.errstate(divide="ignore", invalid="ignore"):
        d = F(1.0) / np.sqrt(N[:, 1] * N[:, 1] + N[:, 0] * N[:, 0])
        ug = np.stack([N[:, 1] * d, -N[:, 0] * d, np.zeros_like(d)], 1)
        vg = np.stack([N[:, 1] * ug[:, 2] - N[:, 2] * ug[:, 1], N[:, 2] * ug[:, 0] - N[:, 0] * ug[:, 2],
                       N[:, 0] * ug[:, 1] - N[:, 1] * ug[:, 0]], 1)
    u[g], v[g] = ug[g], vg[g]
    return u.astype(F), v.astype(F)


def halton_pairs(offs, n):
    """Halton(2) / Halton(3) with setStart(offs - 1), n getNext() each"""
    L = O.lib()
    s1 = np.zeros((len(offs), n), F)
    s2 = np.zeros((len(offs), n), F)
    for k, o in enumerate(offs):
        start = C.c_uint((int(o) - 1) & 0xFFFFFFFF)
        L.orc_halton_seq(2, start, n, s1[k].ctypes.data)
        L.orc_halton_seq(3, start, n, s2[k].ctypes.data)
    return s1, s2


def restate_ao(orc, scene, p, n, dist, aocol, ts_depth=None):
    """Per camera sample (pixel-major, sample fastest): the colour direct
    lighting returns in a scene without lights -- (0 + 0) + AO -- its AO rays
    (diffuse hits only) and the oracle's isShadowed counters for them.
    Flat-shaded one-component Lambert materials at the shading points."""
    spp = p.aa_samples
    rays = orc.camera_rays(p.xstart, p.ystart, p.width, p.height, spp)
    prim, t, _, _, _ = orc.intersect(rays)
    ms = scene.material_states()
    e = orc.arrays
    nc = len(rays)
    col = np.zeros((nc, 3), F)
    idx = np.flatnonzero(prim >= 0)
    mat = e["tri_material"][prim[idx]]
    diffuse = np.array([bool(ms[m].bsdf_flags & BSDF_DIFFUSE) for m in mat], bool)
    idx, mat = idx[diffuse], mat[diffuse]
    frm, d = rays[idx, 0:3], rays[idx, 3:6]
    P = (frm + t[idx, None] * d).astype(F)
    Ng = e["tri_normal"][prim[idx]].astype(F)
    wo = -d
    cos_ng_wo = dot(Ng, wo)
    N = np.where((cos_ng_wo < 0)[:, None], -Ng, Ng)  # sample()'s N; sp.N stays Ng
    NU, NV = create_cs(Ng)
    # accumulate() of a material with the diffuse component alone, Kr = 1
    comp = np.array([[ms[m].component[k] for k in range(4)] for m in mat], F)
    dcol = np.array([list(ms[m].color) for m in mat], F)
    a0 = F(1.0) * comp[:, 0]
    tt = F(1.0) - a0
    acc2 = (F(1.0) - comp[:, 1]) * tt
    a3 = ((F(1.0) - comp[:, 2]) * comp[:, 3]) * acc2
    ssum = F(0.0) + a3
    wp = a3 * (F(1.0) / ssum)
    # samplingOffs = fnv(i * fnv(j)), pixelSample = s
    pix = idx // spp
    py, px = p.ystart + pix // p.width, p.xstart + pix % p.width
    L = O.lib()
    soffs = np.array([L.orc_fnv((int(i) * L.orc_fnv(int(j))) & 0xFFFFFFFF) for i, j in zip(py, px)], np.uint64)
    offs = ((n * (idx % spp)).astype(np.uint64) + soffs) & 0xFFFFFFFF
    s1a, s2a = halton_pairs(offs, n)
    aoc = np.array(aocol, F)
    acc = np.zeros((len(idx), 3), F)
    all_rays = np.zeros((len(idx), n, 8), F)
    terms = []
    for i in range(n):
        s1 = s1a[:, i] / wp
        z2 = (s2a[:, i].astype(np.float64) * 6.28318530717958647692).astype(F)
        c, sn = fcos(z2), fsin(z2)
        sq1, sqz = np.sqrt(F(1.0) - s1), np.sqrt(s1)
        w = (sq1[:, None] * (c[:, None] * NU + sn[:, None] * NV) + sqz[:, None] * N).astype(F)
        w = np.where((s1 >= 1.0)[:, None], N, w)
        surf = np.where((cos_ng_wo * dot(Ng, w) > 0)[:, None], a3[:, None] * dcol, F(0.0)).astype(F)
        pdf = np.abs(dot(N, w)) * wp
        W = np.abs(dot(w, Ng)) / (pdf * F(0.99) + F(0.01))
        cs = np.abs(dot(Ng, w))
        all_rays[:, i, 0:3], all_rays[:, i, 3:6] = P, w
        all_rays[:, i, 6], all_rays[:, i, 7] = SHADOW_BIAS, F(dist)
        terms.append((surf, cs, W, pdf))
    flat = all_rays.reshape(-1, 8)
    if ts_depth is None:
        occ, cnt = orc.shadow(flat)
        filt = None
    else:
        occ, filt, cnt = orc.shadow_ts(flat, ts_depth)
        filt = filt.reshape(len(idx), n, 3)
    occ = occ.reshape(len(idx), n).astype(bool)
    emits = np.array([bool(ms[m].bsdf_flags & BSDF_EMIT) for m in mat], bool)
    em = np.array([list(ms[m].emit_color) for m in mat], F)
    for i, (surf, cs, W, pdf) in enumerate(terms):
        # col += material->emit(state, sp, wo) * s.pdf, ahead of the sample's own term
        acc = np.where(emits[:, None], acc + pdf[:, None] * em, acc).astype(F)
        a = aoc[None, :] * filt[:, i] if filt is not None else np.broadcast_to(aoc, surf.shape)
        v = (((a * surf).astype(F) * cs[:, None]).astype(F) * W[:, None]).astype(F)
        acc = np.where(occ[:, i, None], acc, acc + v).astype(F)
    ao = (acc / F(n)).astype(F)
    col[idx] = np.where(emits[:, None], (F(0.0) + em) + ao, ao).astype(F)  # col = emit; col += 0; col += AO
    return dict(col=col, nrays=flat.shape[0], cnt=cnt, hits=len(idx), filt=filt, occ=occ)


def film_of(col, p):
    """box filter, weight == spp pixels: the samples' colours summed in order"""
    spp = p.aa_samples
    c = col.reshape(p.height, p.width, spp, 3)
    out = np.zeros((p.height, p.width, 3), F)
    for s in range(spp):
        out = (out + c[:, :, s]).astype(F)
    return out


def bits_equal(a, b):
    return (np.ascontiguousarray(a, F).view(np.uint32) == np.ascontiguousarray(b, F).view(np.uint32))
