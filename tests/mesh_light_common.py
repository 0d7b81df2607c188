"""Light meshes, scenes and the numpy restatement shared by
tests/test_mesh_light.py: meshLight_t::initIS with CumulateStep1dDF
(meshlight.cc:47-65, sample_utils.h:85-98), illumSample with sampleSurface and
triangle_t::sample (meshlight.cc:80-138, triangle.cc:156-167) and the cos /
ipdf tail of intersect (meshlight.cc:192-201), in source order with float32
and float64 where the source has them.
"""
import numpy as np

from core_amd.scene import Scene
from tests.dl_common import BOX_FACES
from tests.scenes import uv_sphere

F = np.float32
PI_D = 3.14159265358979323846
INV_PI_D = 0.31830988618379067154
MIN_RAYDIST = F(0.00005)
PROBE_TRI = 11


def _box(lo, hi):
    pts = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])], F)
    return pts, BOX_FACES


def light_meshes():
    """name -> list of (points, faces): the triangle lists the tests use, all
    around (0, 2, 0). "two_mesh" is one light over two meshes."""
    one = (np.array([[-0.5, 2.0, -0.5], [0.5, 2.0, -0.5], [-0.5, 2.0, 0.5]], F), np.array([[0, 1, 2]], np.int32))
    # areas 1 : 3, both facing down (-y)
    two = (np.array([[-1, 2, 0], [0, 2, 0], [-1, 2, 2], [0, 2, 0], [2, 2, 0], [0, 2, 3]], F) * F(0.5),
           np.array([[0, 1, 2], [3, 4, 5]], np.int32))
    # a zero-area triangle (three collinear points) between two real ones
    zero = (np.array([[-1, 2, -1], [0, 2, -1], [-1, 2, 0], [0, 2, 0], [0.5, 2, 0.5], [1, 2, 1],
                      [0, 2.2, 0], [1, 2.2, 0], [0, 2.2, 1]], F),
            np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]], np.int32))
    box = _box((-0.3, 1.8, -0.25), (0.35, 2.2, 0.3))
    sp40 = uv_sphere(5, 5, 0.4, (0.0, 2.0, 0.0))[:2]
    sp200 = uv_sphere(10, 11, 0.45, (0.1, 2.0, -0.05))[:2]
    quad = (np.array([[-0.4, 2, -0.4], [0.4, 2, -0.4], [0.4, 2, 0.4], [-0.4, 2, 0.4]], F),
            np.array([[0, 1, 2], [0, 2, 3]], np.int32))  # facing down
    return {"one": [one], "two_1_3": [two], "zero_mid": [zero], "box": [box], "sphere40": [sp40],
            "sphere200": [sp200], "two_mesh": [quad, _box((0.6, 1.9, -0.2), (0.9, 2.1, 0.2))]}


def tri_list(meshes):
    """(n, 9) float32: the light's triangles, meshes concatenated in order"""
    out = []
    for pts, faces in meshes:
        pts = np.asarray(pts, F).reshape(-1, 3)
        out.append(pts[np.asarray(faces, np.int32).reshape(-1, 3)].reshape(-1, 9))
    return np.concatenate(out).astype(F)


def init_is(tv):
    """meshLight_t::initIS: (areas float32, cdf float32, area, inv_area)"""
    tv = np.asarray(tv, F).reshape(-1, 9)
    e1, e2 = tv[:, 3:6] - tv[:, 0:3], tv[:, 6:9] - tv[:, 0:3]
    c = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1).astype(F)
    ln = np.sqrt(((c[:, 0] * c[:, 0]).astype(F) + (c[:, 1] * c[:, 1]).astype(F)).astype(F) + (c[:, 2] * c[:, 2]).astype(F))
    areas = (0.5 * ln.astype(np.float64)).astype(F)  # 0.5 * (float)length(): a double product
    n = len(areas)
    total = 0.0
    for a in areas:
        total += float(a)
    cdf = np.zeros(n + 1, F)
    acc, delta = 0.0, 1.0 / float(n)
    for i in range(1, n + 1):
        acc += float(areas[i - 1]) * delta
        cdf[i] = F(acc)
    integral = F(acc)
    cdf[1:] = (cdf[1:] / integral).astype(F)
    return areas, cdf, F(total), F(1.0 / total)


def normals(tv):
    """triangle_t::recNormal: ((b - a) ^ (c - a)).normalize(), float32"""
    tv = np.asarray(tv, F).reshape(-1, 9)
    e1, e2 = tv[:, 3:6] - tv[:, 0:3], tv[:, 6:9] - tv[:, 0:3]
    c = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1).astype(F)
    l2 = ((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]).astype(F) + c[:, 2] * c[:, 2]).astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(l2 != 0, F(1.0) / np.sqrt(l2), F(1.0)).astype(F)
    return (c * inv[:, None]).astype(F)


def _dot(a, b):
    return ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]).astype(F) + a[:, 2] * b[:, 2]).astype(F)


def dsample(cdf, u):
    """pdf1D_t::DSample: std::lower_bound (first entry >= u) minus 1, clamped at 0; u == 0 -> 0"""
    idx = np.searchsorted(np.asarray(cdf, F), np.asarray(u, F), side="left").astype(np.int64) - 1
    idx = np.maximum(idx, 0)
    return np.where(np.asarray(u, F) == 0, 0, idx)


def sample_point(tv, cdf, s1, s2):
    """sampleSurface + triangle_t::sample: (triangle index, point)"""
    s1, s2 = np.asarray(s1, F), np.asarray(s2, F)
    prim = dsample(cdf, s1)
    with np.errstate(divide="ignore", invalid="ignore"):
        c0, c1 = cdf[prim], cdf[prim + 1]
        ss1 = np.where(prim > 0, ((s1 - c0).astype(F) / (c1 - c0).astype(F)).astype(F), (s1 / c1).astype(F))
        su1 = np.sqrt(ss1).astype(F)
    u = (F(1.0) - su1).astype(F)
    v = (s2 * su1).astype(F)
    w = ((F(1.0) - u).astype(F) - v).astype(F)
    t = tv[prim]
    p = ((u[:, None] * t[:, 0:3]).astype(F) + (v[:, None] * t[:, 3:6]).astype(F)).astype(F) + (w[:, None] * t[:, 6:9]).astype(F)
    return prim, p.astype(F)


def mesh_illum(tv, cdf, area, nrm, color, double_sided, X):
    """illumSample over rows X = (P, s1, s2): the probe's records
    (ok, dir[3], tmax, col[3], pdf, .., tri at PROBE_TRI); a refusal is a zero row"""
    X = np.asarray(X, F)
    prim, p = sample_point(tv, cdf, X[:, 3], X[:, 4])
    n = nrm[prim]
    l = (p - X[:, 0:3]).astype(F)
    d2 = ((l[:, 0] * l[:, 0] + l[:, 1] * l[:, 1]).astype(F) + l[:, 2] * l[:, 2]).astype(F)
    dist = np.sqrt(d2).astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = (F(1.0) / dist).astype(F)
        l = (l * inv[:, None]).astype(F)
        cosa = (-_dot(l, n)).astype(F)
        back = cosa <= 0
        ok = ~(dist <= 0) & (~back | bool(double_sided))
        cosa = np.where(back, -cosa, cosa).astype(F)
        amc = (F(area) * cosa).astype(F)
        den = np.where(amc == 0, F(1e-8), amc).astype(F)
        pdf = (d2.astype(np.float64) * PI_D / den.astype(np.float64)).astype(F)
    out = np.zeros((len(X), 12), F)
    out[:, 0] = 1
    out[:, 1:4] = l
    out[:, 4] = dist
    out[:, 5:8] = np.asarray(color, F)
    out[:, 8] = pdf
    out[:, PROBE_TRI] = prim.astype(F)
    out[~ok] = 0
    return out


def mesh_hit_tail(prim, t, dirs, nrm, area, color, double_sided):
    """meshLight_t::intersect after the tree query (prim < 0: a miss): the
    probe's records (ok, t, t_set, col[3], ipdf, .., tri at PROBE_TRI)"""
    hit = prim >= 0
    n = nrm[np.maximum(prim, 0)]
    cosa = _dot(np.asarray(dirs, F), (-n).astype(F))
    back = cosa <= 0
    ok = hit & (~back | bool(double_sided))
    cosa = np.abs(cosa).astype(F)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        idist = (F(1.0) / (t * t).astype(F)).astype(F)
        ipdf = (((idist * F(area)).astype(F) * cosa).astype(F).astype(np.float64) * INV_PI_D).astype(F)
    out = np.zeros((len(prim), 12), F)
    out[:, 0] = 1
    out[:, 1] = t
    out[:, 2] = 1
    out[:, 3:6] = np.asarray(color, F)
    out[:, 6] = ipdf
    out[:, PROBE_TRI] = prim.astype(F)
    out[~ok] = 0
    return out


def stored_color(color, power):
    """meshLight_t::factory: color * (CFLOAT)power * M_PI through color_t's float operators"""
    return ((np.asarray(color, F) * F(power)).astype(F) * F(PI_D)).astype(F)


def triangles_scene(tv, res=8):
    """The light's triangles alone, in light order, as a scene of their own:
    what the oracle is given for the closest-hit yardstick."""
    s = Scene()
    m = s.add_material(color=(0.5, 0.5, 0.5))
    tv = np.asarray(tv, F).reshape(-1, 3)
    s.add_mesh(tv, np.arange(len(tv), dtype=np.int32).reshape(-1, 3), m)
    s.set_camera((0, 0.5, -4), (0, 1, 0), (0, 1.5, -4), res, res)
    s.build()
    return s


def add_floor_and_occluder(s):
    """a Lambert floor at y = 0 and a Lambert box floating above it"""
    fm = s.add_material(color=(0.8, 0.7, 0.6))
    om = s.add_material(color=(0.4, 0.6, 0.9), diffuse_reflect=0.9)
    s.add_mesh(np.array([(-2, 0, -2), (-2, 0, 2), (2, 0, 2), (2, 0, -2)], F), np.array([[0, 1, 2], [0, 2, 3]], np.int32), fm)
    s.add_mesh(*_box((-0.5, 0.4, -0.3), (0.3, 0.9, 0.4)), om)


def lit_scene(res, meshes=None, add_light=True, pane=False, **light):
    """Floor + occluder under a mesh light whose meshes carry a light_mat.
    meshes: list of (points, faces); None: a single-sided quad facing down.
    add_light=False leaves the emitting meshes in as plain geometry."""
    s = Scene()
    add_floor_and_occluder(s)
    lm = s.add_material(type_=1, color=(1.0, 0.9, 0.8), power=2.0)
    if meshes is None:
        meshes = light_meshes()["two_mesh"][:1]
    ids = [s.add_mesh(np.asarray(p, F), np.asarray(f, np.int32), lm) for p, f in meshes]
    if pane:  # a filtering pane between light and floor
        t = s.add_material(color=(0.9, 0.5, 0.2), diffuse_reflect=0.2, transparency=0.8, transmit_filter=0.6)
        s.add_mesh(np.array([(-1.5, 1.4, -1.5), (-1.5, 1.4, 1.5), (1.5, 1.4, 1.5), (1.5, 1.4, -1.5)], F),
                   np.array([[0, 1, 2], [0, 2, 3]], np.int32), t)
    if add_light == "area":  # the parallelogram area light over the quad facing down, for the oracle
        q = np.asarray(meshes[0][0], F)
        s.add_area_light(tuple(q[0]), tuple(q[1]), tuple(q[3]), light.get("color", (1, 1, 1)), light.get("power", 1.0),
                         light.get("samples", 4))
    elif add_light:
        s.add_mesh_light(ids, **light)
    s.set_camera((0.3, 2.6, -4.5), (0, 0.6, 0), (0.3, 3.6, -4.5), res, res, focal=1.4)
    s.build()
    return s


# ---- doLightEstimation's sampled branch (mcintegrator.cc:101-193) ---------

def _cos_hemisphere(N, NU, NV, s1, s2):
    """SampleCosHemisphere as tests/dl_common.py restates it for the AO rays"""
    from tests.dl_common import fcos, fsin
    z2 = (s2.astype(np.float64) * 6.28318530717958647692).astype(F)
    c, sn = fcos(z2), fsin(z2)
    with np.errstate(invalid="ignore"):
        sq1, sqz = np.sqrt(F(1.0) - s1), np.sqrt(s1)
    w = (sq1[:, None] * (c[:, None] * NU + sn[:, None] * NV) + sqz[:, None] * N).astype(F)
    return np.where((s1 >= 1.0)[:, None], N, w).astype(F)


def restate_direct_mesh(orc, scene, p, tv, color, samples, double_sided, light_index=0):
    """Per camera sample (pixel-major, sample fastest) the colour direct
    lighting returns in a scene whose only light is one mesh light over the
    triangles tv: emit + (0 + doLightEstimation). Flat-shaded one-component
    Lambert materials (no Fresnel) and light_mat emitters. The light half is
    mesh_illum above; the BSDF half asks the oracle for the closest hit on the
    light's triangles as a scene of their own and applies mesh_hit_tail; both
    halves' shadow rays go to the oracle's isShadowed on the full scene.
    Operation order of the contributions: the area light's compiled form,
    which gen_sampled shares between its kinds.
    Returns dict(col, shadow_rays)."""
    from oracle.oracle import Oracle
    from tests.dl_common import create_cs, dot, halton_pairs, SHADOW_BIAS
    from oracle import oracle as O
    tv = np.asarray(tv, F).reshape(-1, 9)
    _, cdf, area, _ = init_is(tv)
    nrm = normals(tv)
    alone = Oracle(triangles_scene(tv))
    color = np.asarray(color, F)
    n, spp = samples, p.aa_samples
    rays = orc.camera_rays(p.xstart, p.ystart, p.width, p.height, spp)
    prim, t = orc.intersect(rays)[:2]
    ms = scene.material_states()
    e = orc.arrays
    col = np.zeros((len(rays), 3), F)
    hit = np.flatnonzero(prim >= 0)
    hmat = e["tri_material"][prim[hit]]
    # emitters (lightMat_t::emit: the colour when double sided or seen from the front), no direct light
    for k, m in zip(hit, hmat):
        if ms[m].type == 1:
            front = float(np.dot(-rays[k, 3:6].astype(F), e["tri_normal"][prim[k]].astype(F))) > 0
            col[k] = np.array(ms[m].color[:], F) if (ms[m].double_sided or front) else 0
    diffuse = np.array([ms[m].type == 0 and bool(ms[m].bsdf_flags & 0x4) for m in hmat], bool)
    idx, mat = hit[diffuse], hmat[diffuse]
    frm, d = rays[idx, 0:3], rays[idx, 3:6]
    P = (frm + t[idx, None] * d).astype(F)
    Ng = e["tri_normal"][prim[idx]].astype(F)
    wo = (-d).astype(F)
    cos_ng_wo = dot(Ng, wo)
    N = np.where((cos_ng_wo < 0)[:, None], -Ng, Ng).astype(F)
    NU, NV = create_cs(Ng)
    comp = np.array([[ms[m].component[k] for k in range(4)] for m in mat], F)
    dcol = np.array([list(ms[m].color) for m in mat], F)
    a0 = F(1.0) * comp[:, 0]
    tt = F(1.0) - a0
    a3 = ((F(1.0) - comp[:, 2]) * comp[:, 3]) * ((F(1.0) - comp[:, 1]) * tt)      # accumulate()
    mD = ((F(1.0) - comp[:, 2]) * comp[:, 3]) * ((F(1.0) - a0) * (F(1.0) - comp[:, 1]))  # eval()'s mD
    ssum = F(0.0) + a3
    wp = a3 * (F(1.0) / ssum)
    pix = idx // spp
    py, px = p.ystart + pix // p.width, p.xstart + pix % p.width
    L = O.lib()
    soffs = np.array([L.orc_fnv((int(i) * L.orc_fnv(int(j))) & 0xFFFFFFFF) for i, j in zip(py, px)], np.uint64)
    offs = ((n * (idx % spp)).astype(np.uint64) + soffs + np.uint64(light_index * 4567)) & 0xFFFFFFFF
    s1a, s2a = halton_pairs(offs, n)
    m = len(idx)
    ccol, ccol2 = np.zeros((m, 3), F), np.zeros((m, 3), F)
    nrays = 0
    for i in range(n):
        # light half
        X = np.concatenate([P, s1a[:, i:i + 1], s2a[:, i:i + 1]], 1).astype(F)
        r = mesh_illum(tv, cdf, area, nrm, color, double_sided, X)
        lit = r[:, 0] == 1
        ldir, ltmax, lpdf = r[:, 1:4], r[:, 4], r[:, 8]
        sr = np.zeros((m, 8), F)
        sr[:, 0:3], sr[:, 3:6], sr[:, 6], sr[:, 7] = P, ldir, SHADOW_BIAS, ltmax
        occ = np.ones(m, bool)
        if lit.any():
            occ[lit] = orc.shadow(sr[lit])[0].astype(bool)
            nrays += int(lit.sum())
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            surf = np.where((dot(ldir, N) < 0)[:, None], F(0.0), mD[:, None] * dcol).astype(F)
            mpdf = ((F(0.0) + np.abs(dot(ldir, N)) * a3).astype(F) / ssum).astype(F)
            k = (np.abs(dot(Ng, ldir)) * (F(1.0) / lpdf)).astype(F)
            l2, m2 = lpdf * lpdf, mpdf * mpdf
            w = (l2 / (l2 + m2)).astype(F)
            sl = (surf * color[None, :]).astype(F)
            v = np.where((mpdf > 1e-6)[:, None], ((sl * k[:, None]).astype(F) * w[:, None]).astype(F),
                         (sl * k[:, None]).astype(F))
        add = lit & ~occ & (lpdf > F(1e-6))
        ccol = np.where(add[:, None], ccol + v, ccol).astype(F)
        # BSDF half: the same Halton pair
        s1 = (s1a[:, i] / wp).astype(F)
        bdir = _cos_hemisphere(N, NU, NV, s1, s2a[:, i])
        bsurf = np.where((cos_ng_wo * dot(Ng, bdir) > 0)[:, None], a3[:, None] * dcol, F(0.0)).astype(F)
        spdf = (np.abs(dot(N, bdir)) * wp).astype(F)
        W = (np.abs(dot(bdir, Ng)) / (spdf * F(0.99) + F(0.01))).astype(F)
        br = np.zeros((m, 8), F)
        br[:, 0:3], br[:, 3:6], br[:, 6], br[:, 7] = P, bdir, MIN_RAYDIST, -1.0
        lp, lt = alone.intersect(br)[:2]
        h = mesh_hit_tail(lp, lt.astype(F), bdir, nrm, area, color, double_sided)
        bhit = (h[:, 0] == 1) & (spdf > F(1e-6))
        bt, lightpdf = h[:, 1], h[:, 6]
        br[:, 7] = bt
        occ = np.ones(m, bool)
        if bhit.any():
            occ[bhit] = orc.shadow(br[bhit])[0].astype(bool)
            nrays += int(bhit.sum())
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            lPdf = (F(1.0) / lightpdf).astype(F)
            l2, m2 = lPdf * lPdf, spdf * spdf
            w = (m2 / (l2 + m2)).astype(F)
            sw = (bsurf * W[:, None]).astype(F)
            v = np.stack([((sw[:, 0] * color[0]).astype(F) * w), ((sw[:, 1] * color[1]).astype(F) * w),
                          sw[:, 2] * (w * color[2]).astype(F)], 1).astype(F)
        add = bhit & ~occ & (lightpdf > F(1e-6))
        ccol2 = np.where(add[:, None], ccol2 + v, ccol2).astype(F)
    inv = F(1.0) / F(n)
    est = ((F(0.0) + inv * ccol).astype(F) + (inv * ccol2).astype(F)).astype(F)
    col[idx] = (F(0.0) + (F(0.0) + est)).astype(F)
    return dict(col=col, shadow_rays=nrays, diffuse_hits=m)
