"""The numpy restatement shared by tests/test_sun_light.py: sunLight_t's
constructor, init(scene), illumSample, intersect and emitPhoton
(sunlight.cc:52-112) with sampleCone, minRot (sample_utils.h:76-82, 168-176)
and ShirleyDisk (vector3d.cc:156-182), in source order with float32 and
float64 where the source's types have them; emitPhoton of the point,
directional and area lights as k_photon_emit runs them; and
doLightEstimation's sampled branch (mcintegrator.cc:101-193) for a scene
whose light is a sun, on the oracle's camera hits and isShadowed.

The compiled reference has no sun in the oracle and none was run for these
tests: everything here is source order, unpinned against a compiled build.
"""
import numpy as np

from core_amd import _abi as A
from tests.dl_common import create_cs, dot, fcos, fsin

F = np.float32
D = np.float64
PI_D = 3.14159265358979323846
TWO_PI_D = 6.28318530717958647692
DEG_D = 0.01745329251994329576922
MIN_RAYDIST = F(0.00005)
PROBE_EMIT_PHOTON = 3


def _v(x):
    return np.asarray(x, F)


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1).astype(F)


def sun_state(direction, color=(1, 1, 1), power=1.0, angle=0.27, samples=4):
    """sunLight_t::sunLight_t: the members as yk_sun_light_state names them.
    direction.normalize() normalizes the member; createCS gets the
    un-normalized argument."""
    d = _v(direction)
    du, dv = create_cs(d[None, :])
    ln = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    nd = d * (F(1.0) / np.sqrt(ln)) if ln != 0 else d
    angle = F(angle)
    if angle > F(80.0):
        angle = F(80.0)
    cos_angle = float(fcos(F(D(angle) * DEG_D)))  # double degToRad -> fCos(float) -> double member
    invpdf = F(TWO_PI_D * (1.0 - cos_angle))
    with np.errstate(divide="ignore"):
        pdf = F(1.0 / D(invpdf))  # infinite where fCos answered exactly 1 (angles below about 0.02 degrees)
    col = (_v(color) * F(power)).astype(F)
    return dict(color=col, col_pdf=(col * pdf).astype(F), direction=nd.astype(F), du=du[0], dv=dv[0], pdf=pdf,
                invpdf=invpdf, cos_angle=cos_angle, samples=int(samples))


def state_struct(st):
    return A.yk_sun_light_state(A.f3(*st["color"]), A.f3(*st["col_pdf"]), A.f3(*st["direction"]), A.f3(*st["du"]),
                                A.f3(*st["dv"]), st["pdf"], st["invpdf"], st["cos_angle"], st["samples"])


def struct_state(s):
    return dict(color=_v(s.color[:]), col_pdf=_v(s.col_pdf[:]), direction=_v(s.direction[:]), du=_v(s.du[:]),
                dv=_v(s.dv[:]), pdf=F(s.pdf), invpdf=F(s.invpdf), cos_angle=float(s.cos_angle), samples=int(s.samples))


def same_state(a, b):
    for k in ("color", "col_pdf", "direction", "du", "dv", "pdf", "invpdf"):
        if not (np.atleast_1d(_v(a[k])).view(np.uint32) == np.atleast_1d(_v(b[k])).view(np.uint32)).all():
            return False
    return np.array(a["cos_angle"], D).view(np.uint64) == np.array(b["cos_angle"], D).view(np.uint64) and \
        a["samples"] == b["samples"]


def sun_init(bound):
    """sunLight_t::init on the scene bound (ax, ay, az, gx, gy, gz): worldCenter, worldRadius, ePdf"""
    b = _v(bound)
    dlt = (b[3:] - b[:3]).astype(F)
    ln = np.sqrt((dlt[0] * dlt[0] + dlt[1] * dlt[1]) + dlt[2] * dlt[2])
    radius = F(0.5 * D(ln))
    center = (F(0.5) * (b[:3] + b[3:]).astype(F)).astype(F)
    epdf = F(PI_D * D(radius) * D(radius))
    return center, radius, epdf


def sample_cone(Dv, U, V, max_cos, s1, s2):
    """sampleCone: float throughout, t1 = M_2PI * s1 a double product"""
    s1, s2, mc = _v(s1), _v(s2), F(max_cos)
    cos_a = (F(1.0) - ((F(1.0) - mc) * s2).astype(F)).astype(F)
    with np.errstate(invalid="ignore"):
        sin_a = np.sqrt((F(1.0) - (cos_a * cos_a).astype(F)).astype(F)).astype(F)
    t1 = (TWO_PI_D * s1.astype(D)).astype(F)
    c, s = fcos(t1), fsin(t1)
    uv = ((U[None, :] * c[:, None]).astype(F) + (V[None, :] * s[:, None]).astype(F)).astype(F)
    return ((uv * sin_a[:, None]).astype(F) + (Dv[None, :] * cos_a[:, None]).astype(F)).astype(F)


def sun_illum(st, X):
    """illumSample over rows X = (P, s1, s2): the probe's records (ok, dir[3], tmax, col[3], pdf)"""
    X = _v(X)
    out = np.zeros((len(X), 12), F)
    out[:, 0] = 1
    out[:, 1:4] = sample_cone(st["direction"], st["du"], st["dv"], F(st["cos_angle"]), X[:, 3], X[:, 4])
    out[:, 4] = -1
    out[:, 5:8] = st["col_pdf"]
    out[:, 8] = st["pdf"]
    return out


def sun_hit(st, X):
    """intersect over rows X = (from, dir): the probe's records (ok, t, t_set, col[3], ipdf)"""
    X = _v(X)
    d = st["direction"]
    cosine = ((X[:, 3] * d[0] + X[:, 4] * d[1]).astype(F) + X[:, 5] * d[2]).astype(F)
    ok = ~(cosine.astype(D) < st["cos_angle"])
    out = np.zeros((len(X), 12), F)
    out[:, 0] = 1
    out[:, 1] = -1
    out[:, 2] = 1
    out[:, 3:6] = st["col_pdf"]
    out[:, 6] = st["invpdf"]
    out[~ok] = 0
    return out


def shirley_disk(r1, r2):
    r1, r2 = _v(r1), _v(r2)
    a, b = (F(2) * r1 - F(1)).astype(F), (F(2) * r2 - F(1)).astype(F)
    q = PI_D / 4
    with np.errstate(divide="ignore", invalid="ignore"):
        ba, ab = (b / a).astype(F), (a / b).astype(F)
        c1 = (a > -b) & (a > b)
        c2 = (a > -b) & ~(a > b)
        c3 = ~(a > -b) & (a < b)
        r = np.where(c1, a, np.where(c2, b, np.where(c3, -a, -b))).astype(F)
        phi = np.where(c1, (q * ba.astype(D)).astype(F),
                       np.where(c2, (q * (F(2) - ab).astype(F).astype(D)).astype(F),
                                np.where(c3, (q * (F(4) + ba).astype(F).astype(D)).astype(F),
                                         np.where(b != 0, (q * (F(6) - ab).astype(F).astype(D)).astype(F), F(0))))).astype(F)
    return (r * fcos(phi)).astype(F), (r * fsin(phi)).astype(F)


def min_rot(Dv, U, D2):
    """minRot as written: the middle term of U2 is a float, (1.f - cosAlpha) *
    (v * U) with the dot product v * U, which vector3d_t(PFLOAT) turns into a
    vector of three equal components"""
    Dn, Un = np.broadcast_to(Dv, D2.shape), np.broadcast_to(U, D2.shape)
    cos_a = ((Dn[:, 0] * D2[:, 0] + Dn[:, 1] * D2[:, 1]).astype(F) + Dn[:, 2] * D2[:, 2]).astype(F)
    with np.errstate(invalid="ignore"):
        sin_a = np.sqrt((F(1) - (cos_a * cos_a).astype(F)).astype(F)).astype(F)
    v = cross(Dn, D2)
    vu = ((v[:, 0] * Un[:, 0] + v[:, 1] * Un[:, 1]).astype(F) + v[:, 2] * Un[:, 2]).astype(F)
    m = ((F(1) - cos_a).astype(F) * vu).astype(F)
    w = cross(v, Un)
    U2 = (((cos_a[:, None] * Un).astype(F) + m[:, None]).astype(F) + (sin_a[:, None] * w).astype(F)).astype(F)
    return U2, cross(D2, U2), sin_a


def sun_emit(st, bound, S):
    """emitPhoton over rows S = (s1, s2, s3, s4): the probe's records (from[3], dir[3], ipdf, col[3])"""
    S = _v(S)
    center, radius, epdf = sun_init(bound)
    u, v = shirley_disk(S[:, 2], S[:, 3])
    ldir = sample_cone(st["direction"], st["du"], st["dv"], F(st["cos_angle"]), S[:, 2], S[:, 3])
    du2, dv2, _ = min_rot(st["direction"], st["du"], ldir)
    off = (((u[:, None] * du2).astype(F) + (v[:, None] * dv2).astype(F)).astype(F) + ldir).astype(F)
    out = np.zeros((len(S), 12), F)
    out[:, 0:3] = (center[None, :] + (radius * off).astype(F)).astype(F)
    out[:, 3:6] = -ldir
    out[:, 6] = st["invpdf"]
    out[:, 7:10] = (st["col_pdf"] * epdf).astype(F)
    return out


def cos_hemisphere(N, NU, NV, s1, s2):
    """SampleCosHemisphere, sample_utils.h:41-50"""
    z2 = (s2.astype(D) * TWO_PI_D).astype(F)
    c, sn = fcos(z2), fsin(z2)
    with np.errstate(invalid="ignore"):
        sq1, sqz = np.sqrt(F(1.0) - s1).astype(F), np.sqrt(s1).astype(F)
    w = (sq1[:, None] * (c[:, None] * NU + sn[:, None] * NV).astype(F) + sqz[:, None] * N).astype(F)
    return np.where((s1 >= 1.0)[:, None], N, w).astype(F)


def area_emit(ls, S):
    """areaLight_t::emitPhoton (arealight.cc:98-104) on a yk_area_light_state, with the
    constructor's frame (arealight.cc:30-49): fnormal = toY ^ toX, area = its
    length, normal = -fnormal.normalize(), du = toX.normalize(), dv = normal ^ du"""
    S = _v(S)
    c, x, y = _v(ls.corner[:]), _v(ls.to_x[:]), _v(ls.to_y[:])
    f = cross(y, x)
    area = np.sqrt((f[0] * f[0] + f[1] * f[1]) + f[2] * f[2]).astype(F)
    f = (f * (F(1.0) / area)).astype(F)
    du = (x * (F(1.0) / np.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]))).astype(F)
    n = (-f).astype(F)
    dv = cross(n, du)
    out = np.zeros((len(S), 12), F)
    out[:, 0:3] = ((c[None, :] + (S[:, 2:3] * x).astype(F)).astype(F) + (S[:, 3:4] * y).astype(F)).astype(F)
    out[:, 3:6] = cos_hemisphere(n[None, :], du[None, :], dv[None, :], S[:, 0], S[:, 1])
    out[:, 6] = area
    out[:, 7:10] = _v(ls.color[:])
    return out, area


def point_emit(ls, S):
    """pointLight_t::emitPhoton + SampleSphere (sample_utils.h:54-72)"""
    S = _v(S)
    out = np.zeros((len(S), 12), F)
    out[:, 0:3] = _v(ls.position[:])
    z = (F(1.0) - F(2.0) * S[:, 0]).astype(F)
    rr = (F(1.0) - z * z).astype(F)
    a = (TWO_PI_D * S[:, 1].astype(D)).astype(F)
    with np.errstate(invalid="ignore"):
        r = np.sqrt(rr).astype(F)
    pos = rr > 0
    out[:, 3] = np.where(pos, fcos(a) * r, F(0))
    out[:, 4] = np.where(pos, fsin(a) * r, F(0))
    out[:, 5] = z
    out[:, 6] = F(4.0 * PI_D)
    out[:, 7:10] = _v(ls.color[:])
    return out


def directional_emit(ls, bound, S):
    """directionalLight_t::emitPhoton (directional.cc:106-116) after init(scene)"""
    S = _v(S)
    d = _v(ls.direction[:])
    du, dv = create_cs(d[None, :])
    center, wradius, _ = sun_init(bound)
    pos, radius = (center, wradius) if ls.infinite else (_v(ls.position[:]), F(ls.radius))
    u, v = shirley_disk(S[:, 0], S[:, 1])
    off = ((u[:, None] * du).astype(F) + (v[:, None] * dv).astype(F)).astype(F)
    frm = (pos[None, :] + (radius * off).astype(F)).astype(F)
    if ls.infinite:
        frm = (frm + (wradius * d)[None, :].astype(F)).astype(F)
    out = np.zeros((len(S), 12), F)
    out[:, 0:3] = frm
    out[:, 3:6] = -d
    out[:, 6] = F(PI_D * D(radius) * D(radius))
    out[:, 7:10] = _v(ls.color[:])
    return out


def light_energy(kind, ls, bound, st=None):
    """light_t::totalEnergy().energy() as yk_photon_build computes it"""
    if kind == A.YK_LIGHT_SUN:
        e = (st["color"] * sun_init(bound)[2]).astype(F)
    elif kind == A.YK_LIGHT_POINT:
        e = ((_v(ls.color[:]) * F(4.0)).astype(F) * F(PI_D)).astype(F)
    elif kind == A.YK_LIGHT_DIRECTIONAL:
        r = sun_init(bound)[1] if ls.infinite else F(ls.radius)
        e = (((_v(ls.color[:]) * r).astype(F) * r).astype(F) * F(PI_D)).astype(F)
    else:
        e = (_v(ls.color[:]) * area_emit(ls, np.zeros((1, 4), F))[1]).astype(F)
    return F(((e[0] + e[1]) + e[2]) * F(0.333333))


def light_pdf(energies):
    """pdf1D_t over the light energies (CumulateStep1dDF): cdf, 1 / integral"""
    n = len(energies)
    c, delta = 0.0, 1.0 / n
    cdf = np.zeros(n + 1, F)
    for i, e in enumerate(energies):
        c += float(e) * delta
        cdf[i + 1] = F(c)
    integral = F(c)
    cdf[1:] = (cdf[1:] / integral).astype(F)
    return cdf, F(1.0) / integral


def restate_direct_sun(orc, scene, p, st, light_index=0):
    """Per camera sample (pixel-major, sample fastest) the colour direct
    lighting returns in a scene whose only light is the sun st: emit + (0 +
    doLightEstimation). Flat-shaded one-component Lambert materials. The
    light half is sun_illum, the BSDF half sun_hit on the material's cosine
    sample; both halves' rays are unbounded (tmax -1) and go to the oracle's
    isShadowed. Operation order of the contributions: the area light's
    compiled form, which gen_sampled shares between its kinds (the order
    tests/mesh_light_common.py uses). Returns dict(col, shadow_rays, ...)."""
    from oracle import oracle as O
    from tests.dl_common import SHADOW_BIAS, halton_pairs
    color = st["col_pdf"]
    n, spp = st["samples"], p.aa_samples
    rays = orc.camera_rays(p.xstart, p.ystart, p.width, p.height, spp)
    prim, t = orc.intersect(rays)[:2]
    ms = scene.material_states()
    e = orc.arrays
    col = np.zeros((len(rays), 3), F)
    hit = np.flatnonzero(prim >= 0)
    hmat = e["tri_material"][prim[hit]]
    for k, m in zip(hit, hmat):  # emitters (lightMat_t::emit), no direct light
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
    nrays = lit_samples = mis_samples = 0
    for i in range(n):
        # light half: always lit, always traced
        X = np.concatenate([P, s1a[:, i:i + 1], s2a[:, i:i + 1]], 1).astype(F)
        r = sun_illum(st, X)
        ldir, lpdf = r[:, 1:4], r[:, 8]
        sr = np.zeros((m, 8), F)
        sr[:, 0:3], sr[:, 3:6], sr[:, 6], sr[:, 7] = P, ldir, SHADOW_BIAS, -1.0
        occ = orc.shadow(sr)[0].astype(bool)
        nrays += m
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            surf = np.where((dot(ldir, N) < 0)[:, None], F(0.0), mD[:, None] * dcol).astype(F)
            mpdf = ((F(0.0) + np.abs(dot(ldir, N)) * a3).astype(F) / ssum).astype(F)
            k = (np.abs(dot(Ng, ldir)) * (F(1.0) / lpdf)).astype(F)
            l2, m2 = lpdf * lpdf, mpdf * mpdf
            w = (l2 / (l2 + m2)).astype(F)
            sl = (surf * color[None, :]).astype(F)
            v = np.where((mpdf > 1e-6)[:, None], ((sl * k[:, None]).astype(F) * w[:, None]).astype(F),
                         (sl * k[:, None]).astype(F))
        add = ~occ & (lpdf > F(1e-6))
        lit_samples += int((add & (v.sum(-1) > 0)).sum())
        ccol = np.where(add[:, None], ccol + v, ccol).astype(F)
        # BSDF half: the same Halton pair
        s1 = (s1a[:, i] / wp).astype(F)
        bdir = cos_hemisphere(N, NU, NV, s1, s2a[:, i])
        bsurf = np.where((cos_ng_wo * dot(Ng, bdir) > 0)[:, None], a3[:, None] * dcol, F(0.0)).astype(F)
        spdf = (np.abs(dot(N, bdir)) * wp).astype(F)
        W = (np.abs(dot(bdir, Ng)) / (spdf * F(0.99) + F(0.01))).astype(F)
        h = sun_hit(st, np.concatenate([P, bdir], 1))
        bhit = (h[:, 0] == 1) & (spdf > F(1e-6))
        lightpdf = h[:, 6]
        br = np.zeros((m, 8), F)
        br[:, 0:3], br[:, 3:6], br[:, 6], br[:, 7] = P, bdir, MIN_RAYDIST, -1.0
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
        mis_samples += int(add.sum())
        ccol2 = np.where(add[:, None], ccol2 + v, ccol2).astype(F)
    inv = F(1.0) / F(n)
    est = ((F(0.0) + inv * ccol).astype(F) + (inv * ccol2).astype(F)).astype(F)
    col[idx] = (F(0.0) + (F(0.0) + est)).astype(F)
    return dict(col=col, shadow_rays=nrays, diffuse_hits=m, lit_samples=lit_samples, mis_samples=mis_samples)
