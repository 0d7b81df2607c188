"""float32 / float64 numpy restatement of the glass material (glassMat_t, glass.cc:28-337, without
dispersion, absorption or shader nodes) and of refract() (vector3d.cc:86-108), in source order, row-wise
over arrays of inputs. fresnel() is tests/coated_common.py's."""
import numpy as np

from tests import coated_common as K
from tests import glossy_common as G

F, D = np.float32, np.float64
dot, normalize, f32 = G.dot, G.normalize, G.f32
SPECULAR, REFLECT, TRANSMIT, FILTER, DIFFUSE, DISPERSIVE, VOLUMETRIC = 0x1, 0x10, 0x20, 0x40, 0x4, 0x8, 0x100
ALL_SPECULAR = SPECULAR | REFLECT | TRANSMIT
GLASS = 5  # YK_MAT_GLASS


def state_of(ior=1.4, filter_color=(1, 1, 1), transmit_filter=0.0, mirror_color=(1, 1, 1), fake_shadows=False):
    """factory + constructor, glass.cc:55-69, 262-274: filt is a double (here the float the parameter
    struct holds, widened); filt*filtCol takes it as a float, color_t(1.f-filt) rounds the double difference"""
    filt = D(F(transmit_filter))
    fc = (F(filt) * f32(list(filter_color)) + F(D(1.0) - filt)).astype(F)
    return dict(ior=F(D(ior)), filter_col=fc, mirror_color=f32(list(mirror_color)), fake_shadow=int(bool(fake_shadows)),
                bsdf_flags=ALL_SPECULAR | (FILTER if fake_shadows else 0))


class Glass:
    def __init__(self, st, gs):
        self.ior = F(st.ior)
        self.mirror = f32(list(st.mirror_color))
        self.filter = f32(list(gs.filter_col))
        self.fake = bool(gs.fake_shadow)
        self.tm = (FILTER | TRANSMIT) if self.fake else (SPECULAR | TRANSMIT)


def refract(n, wi, ior):
    """refract(): -> (ok, wo); wo is zero where it returns false"""
    with np.errstate(all="ignore"):
        c = dot(wi, n)
        neg = c < 0
        N = np.where(neg[:, None], -n, n).astype(F)
        c = np.where(neg, -c, c).astype(F)
        eta = np.where(neg, F(ior), F(D(1.0) / D(ior))).astype(F)
        I = (-wi).astype(F)
        k = (F(1.0) - eta * eta * (F(1.0) - c * c)).astype(F)
        ok = ~(k <= 0)
        f = (eta * c - np.sqrt(np.where(ok, k, F(0.0)))).astype(F)
        wo = normalize((eta[:, None] * I + f[:, None] * N).astype(F))
    return ok, np.where(ok[:, None], wo, F(0.0)).astype(F), k


def glass_normal(Ng, N, wo):
    with np.errstate(all="ignore"):
        outside = dot(Ng, wo) > 0
        cw = dot(N, wo)
        f = (1.00001 * cw.astype(D)).astype(F)
        bent = normalize((N - f[:, None] * wo).astype(F))
        keep = np.where(outside, cw >= 0, cw <= 0)
    return outside, np.where(keep[:, None], N, bent).astype(F), ~keep


def _reflect(wo, N):
    vn = F(2.0) * dot(wo, N)
    return (vn[:, None] * N - wo).astype(F)


def p_widths(Kr, Kt):
    return (0.01 + 0.99 * Kr.astype(D)).astype(F), (0.01 + 0.99 * Kt.astype(D)).astype(F)


def glass_sample(M, Ng, N, wo, s1, flags):
    """-> dict ok, wi, col, pdf, W, sflags as the probe reports them (wi and W zero where untouched)"""
    n = len(wo)
    out = dict(ok=np.zeros(n, bool), wi=np.zeros((n, 3), F), col=np.zeros((n, 3), F), pdf=np.zeros(n, F),
               W=np.zeros(n, F), sflags=np.zeros(n, np.int64))
    if not (flags & SPECULAR):
        return out
    _, Nn, _ = glass_normal(Ng, N, wo)
    ok, refdir, _ = refract(Nn, wo, M.ior)
    Kr, Kt = K.fresnel(wo, Nn, M.ior)
    pKr, pKt = p_widths(Kr, Kt)
    rdir = _reflect(wo, Nn)
    tm_ok = (flags & M.tm) == M.tm
    sp_ok = (flags & (SPECULAR | REFLECT)) == (SPECULAR | REFLECT)
    pick_t = ok & (s1 < pKt) & tm_ok
    pick_r = ok & ~pick_t & sp_ok
    tir = ~ok & sp_ok
    for sel, wi, col, pdf, sf in ((pick_t, refdir, M.filter[None, :], pKt, M.tm),
                                  (pick_r, rdir, M.mirror[None, :], pKr, SPECULAR | REFLECT),
                                  (tir, rdir, f32([1, 1, 1])[None, :], np.ones(n, F), SPECULAR | REFLECT)):
        out["ok"] |= sel
        out["wi"] = np.where(sel[:, None], wi, out["wi"]).astype(F)
        out["col"] = np.where(sel[:, None], col, out["col"]).astype(F)
        out["pdf"] = np.where(sel, pdf, out["pdf"]).astype(F)
        out["W"] = np.where(sel, F(1.0), out["W"]).astype(F)
        out["sflags"] = np.where(sel, sf, out["sflags"])
    return out


def glass_specular(M, Ng, N, wo, raylevel):
    """getSpecular -> (refl, dir0, col0, refr, dir1, col1); zero where a child is absent"""
    n = len(wo)
    raylevel = np.broadcast_to(np.asarray(raylevel), (n,))
    outside, Nn, _ = glass_normal(Ng, N, wo)
    ok, refdir, _ = refract(Nn, wo, M.ior)
    Kr, Kt = K.fresnel(wo, Nn, M.ior)
    rdir = _reflect(wo, Nn)
    refr = ok
    refl = ~ok | outside | (raylevel < 3)
    col0 = np.where(ok[:, None], (Kr[:, None] * M.mirror[None, :]).astype(F), F(1.0)).astype(F)
    col1 = (Kt[:, None] * M.filter[None, :]).astype(F)
    z = F(0.0)
    return (refl, np.where(refl[:, None], rdir, z).astype(F), np.where(refl[:, None], col0, z).astype(F),
            refr, np.where(refr[:, None], refdir, z).astype(F), np.where(refr[:, None], col1, z).astype(F))


def glass_transparency(M, Ng, N, wo):
    _, Kt = K.fresnel(wo, G.face_forward(Ng, N, wo), M.ior)
    return (Kt[:, None] * M.filter[None, :]).astype(F)


def glass_alpha(M, Ng, N, wo):
    t = glass_transparency(M, Ng, N, wo)
    e = ((t[:, 0] + t[:, 1] + t[:, 2]) * F(0.333333)).astype(F)
    a = (1.0 - e.astype(D)).astype(F)
    return np.where(a < 0, F(0.0), a).astype(F)


def fold_direct(orc, scene, rays, level, raydepth, stats):
    """directlighting's integrate() of `rays` (n, 8) at recursion level `level` (0: camera rays), restated
    per ray as the device's fold has it: col = (0 + direct) + 0 at a hit (Dirac lights, tests/coated_common.py's
    direct_dirac; nothing on glass, whose eval is black), then, while state.raylevel = level + 1 <= raydepth,
    col += integrate(reflect child) * col[0] and col += integrate(refract child) * col[1] with the children
    of the restated getSpecular, rays from the hit point with tmin MIN_RAYDIST, unbounded. Closest hits and
    isShadowed come from the oracle of the same geometry. stats counts the closest and shadow rays and the
    nodes per level."""
    n = len(rays)
    col = np.zeros((n, 3), F)
    stats["closest"] += n
    stats.setdefault("levels", {}).setdefault(level, 0)
    stats["levels"][level] += n
    idx, P, Ng, mat, wo = K.hit_points(orc, rays)
    if not len(idx):
        return col
    states = scene.material_states()
    glass = np.array([states[m].type == GLASS for m in mat], bool)
    for m in np.unique(mat[~glass]):
        assert not states[m].bsdf_flags & (SPECULAR | FILTER), "only glass recurses in these scenes"
    node = np.zeros((len(idx), 3), F)
    if (~glass).any():
        d = ~glass
        direct, nsh = K.direct_dirac(orc, scene, P[d], Ng[d], mat[d], wo[d])
        node[d] = ((F(0.0) + direct) + F(0.0)).astype(F)
        stats["shadow"] += nsh
    lv = level + 1
    if lv <= raydepth and lv < 20:
        for m in np.unique(mat[glass]):
            k = np.flatnonzero(glass & (mat == m))
            M = Glass(states[m], scene.glass_state(int(m)))
            refl, d0, c0, refr, d1, c1 = glass_specular(M, Ng[k], Ng[k], wo[k], lv)
            for flag, dd, cc in ((refl, d0, c0), (refr, d1, c1)):  # the fold's order: reflection, then refraction
                kk = k[flag]
                if not len(kk):
                    continue
                cr = np.zeros((len(kk), 8), F)
                cr[:, 0:3], cr[:, 3:6], cr[:, 6], cr[:, 7] = P[kk], dd[flag], F(0.00005), F(-1.0)
                v = fold_direct(orc, scene, cr, level + 1, raydepth, stats)
                node[kk] = (node[kk] + v * cc[flag]).astype(F)
    col[idx] = node
    return col
