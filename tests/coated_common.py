"""float32 restatement of the coated glossy material (coatedGlossyMat_t,
coatedglossy.cc, with as_diffuse; fresnel(), vector3d.cc:110-137) in numpy, in
source order, on top of tests/glossy_common.py (the lobes, fPow, Oren-Nayar
and diffuseReflect are glossy's). Shared by tests/test_coated_glossy.py. Every
operation rounds once, in the type the C++ source gives it; where that type is
double the step says so.
"""
import numpy as np

from tests import glossy_common as G

F, D = G.F, G.D
f32, dot, normalize = G.f32, G.dot, G.normalize
BSDF_SPECULAR, BSDF_DIFFUSE, BSDF_REFLECT, BSDF_ALL = 0x1, 0x4, 0x10, 0x7F
SPEC = BSDF_SPECULAR | BSDF_REFLECT   # cFlags[C_SPECULAR]
DIFF = BSDF_DIFFUSE | BSDF_REFLECT    # cFlags[C_GLOSSY] with as_diffuse, cFlags[C_DIFFUSE]
COATED = 4                            # YK_MAT_COATED_GLOSSY


def state_of(mirror_color=(1, 1, 1), ior=1.4, **glossy_kw):
    """the constructor (coatedglossy.cc:80-102) and the factory (:420-463): glossy's members, the
    flags and component table, mirror_color, and IOR after `if(ior == 1.f) ior = 1.0000001f`
    (a double compared with and assigned a float literal, then held as a float)"""
    st = G.state_of(**glossy_kw)
    ior = float(ior)
    if ior == float(F(1.0)):
        ior = float(F(1.0000001))
    wd = st["with_diffuse"]
    st.update(type=COATED, bsdf_flags=SPEC | DIFF | (DIFF if wd else 0), ncomp=3 if wd else 2,
              comp_flags=(SPEC, DIFF, DIFF if wd else 0, 0), mirror_color=tuple(F(c) for c in mirror_color),
              ior=F(ior))
    return st


class Coated(G.Glossy):
    """coatedGlossyMat_t's members as yk_material_state reports them, plus pDiffuse (coatedglossy.cc:116,
    the same expression as glossy's)"""

    def __init__(self, st):
        super().__init__(st)
        self.mirror = f32(list(st.mirror_color))
        self.ior = F(st.ior)


def fresnel(I, n, ior):
    """fresnel(), vector3d.cc:110-137: float up to aux; 0.5*(g-c)*(g-c) and what meets it in double"""
    with np.errstate(all="ignore"):
        N = np.where((dot(I, n) < 0)[:, None], -n, n).astype(F)
        c = dot(I, N)
        g = ior * ior + c * c - F(1.0)
        g = np.where(g <= 0, F(0.0), np.sqrt(np.where(g <= 0, F(0.0), g))).astype(F)
        aux = c * (g + c)
        gm = (g - c).astype(D)
        a = ((0.5 * gm) * gm) / ((g + c) * (g + c)).astype(D)
        b = (F(1.0) + ((aux - F(1.0)) * (aux - F(1.0))) / ((aux + F(1.0)) * (aux + F(1.0)))).astype(D)
        Kr = (a * b).astype(F)
        Kt = np.where(Kr.astype(D) < 1.0, F(1.0) - Kr, F(0.0)).astype(F)
    return Kr, Kt


def coated_eval(M, Ng, N, NU, NV, wo, wi, bsdfs=BSDF_ALL):
    """coatedGlossyMat_t::eval, coatedglossy.cc:156-193: cos_wi_H unclamped, the diffuse base times Kt"""
    n = len(wo)
    if not (bsdfs & BSDF_DIFFUSE):
        return np.zeros((n, 3), F)
    with np.errstate(all="ignore"):
        zero = (dot(Ng, wi) * dot(Ng, wo)) < 0
        Nf = G.face_forward(Ng, N, wo)
        wiN, woN = np.abs(dot(wi, Nf)), np.abs(dot(wo, Nf))
        _, Kt = fresnel(wo, Nf, M.ior)
        H = normalize((wo + wi).astype(F))
        cwh = dot(wi, H)
        glossy = Kt * G.lobe_d(M, H, NU, NV, dot(H, Nf)) * G.schlick(cwh, M.mG) / G.as_divisor(cwh, woN, wiN)
        col = (glossy[:, None] * M.gloss[None, :]).astype(F)
        if M.with_diffuse:
            dc = ((M.mD * (F(1.0) - M.mG)) * M.diff).astype(F)
            col = (col + G.on_factor(M, wi, wo, Nf)[:, None] * (Kt[:, None] * dc[None, :])).astype(F)
    return np.where(zero[:, None], F(0.0), col).astype(F)


def widths(M, Kr, Kt, flags):
    """the component table of sample(): the matched components in order, and their accumC"""
    use_spec = (flags & SPEC) == SPEC
    use_glossy = (flags & DIFF) == DIFF
    use_diffuse = M.with_diffuse and use_glossy
    comps, acc = [], []
    if use_spec:
        comps.append(0)
        acc.append(Kr)
    if use_glossy:
        comps.append(1)
        acc.append((Kt * (F(1.0) - M.pD)).astype(F))
    if use_diffuse:
        comps.append(2)
        acc.append((Kt * M.pD).astype(F))
    return comps, acc


def coated_sample(M, Ng, N, NU, NV, wo, s1, s2, flags, trig=G.HostTrig):
    """coatedGlossyMat_t::sample, coatedglossy.cc:195-336. Returns dict(ok, wi, col, pdf, W, sflags, comp);
    wi and W start at zero, and ok = 0 marks the returns ahead of the W assignment (what they had
    written by then stays); comp is the picked component (-1: none)."""
    n = len(wo)
    Ng, N, NU, NV, wo, s1, s2 = (f32(a) for a in (Ng, N, NU, NV, wo, s1, s2))
    out = dict(ok=np.ones(n, bool), wi=np.zeros((n, 3), F), col=np.zeros((n, 3), F), pdf=np.zeros(n, F),
               W=np.zeros(n, F), sflags=np.zeros(n, np.uint32), comp=np.full(n, -1))
    with np.errstate(all="ignore"):
        cos_Ng_wo = dot(Ng, wo)
        Nf = G.face_forward(Ng, N, wo)
        Kr, Kt = fresnel(wo, Nf, M.ior)
        comps, width = widths(M, Kr, Kt, flags)
        nm = len(comps)
        if nm == 0:
            out["ok"][:] = False
            return out
        total = np.zeros(n, F)
        val = []
        for w in width:
            total = (total + w).astype(F)
            val.append(total)
        early = total.astype(D) < 0.00001
        if nm == 1:
            pick = np.zeros(n, int)
            width = [np.ones(n, F)]
        else:
            inv = F(1.0) / total
            val = [(v * inv).astype(F) for v in val]
            width = [(w * inv).astype(F) for w in width]
            pick = np.full(n, -1)
            for i in range(nm):
                pick = np.where((s1 <= val[i]) & (pick < 0), i, pick)
            pick = np.where(pick < 0, nm - 1, pick)
        W_ = np.stack(width, 1)
        V_ = np.stack(val, 1)
        idx = np.arange(n)
        wp = W_[idx, pick]
        vprev = V_[idx, np.maximum(pick - 1, 0)]
        s1p = np.where(pick > 0, (s1 - vprev) / wp, s1 / wp).astype(F)
        comp = np.array(comps)[pick]
        use_glossy, use_diffuse = 1 in comps, 2 in comps
        w_gl = width[comps.index(1)] if use_glossy else None
        w_df = width[comps.index(2)] if use_diffuse else None
        woN = np.abs(dot(wo, Nf))

        # C_SPECULAR: reflect_dir(N, wo)
        vn = dot(wo, Nf)
        wi_s = np.where((vn < 0)[:, None], -wo, (F(2.0) * vn)[:, None] * Nf - wo).astype(F)
        col_s = (M.mirror[None, :] * Kr[:, None]).astype(F)
        m = (comp == 0) & ~early
        out["wi"][m], out["col"][m], out["pdf"][m], out["W"][m], out["sflags"][m] = wi_s[m], col_s[m], wp[m], F(1.0), SPEC

        def finish(mask, wi, H, Hs, cwoH, wrong):
            wiN = np.abs(dot(wi, Nf))
            Dv = G.aniso_d(Hs[:, 0], Hs[:, 1], Hs[:, 2], M.exp_u, M.exp_v) if M.aniso else G.blinn_d(dot(H, Nf), M.exponent)
            pdf = (F(0.0) + (Dv / G.pdf_divisor(cwoH)) * w_gl).astype(F)
            glossy = Dv * G.schlick(cwoH, M.mG) / G.as_divisor(cwoH, woN, wiN)
            col = ((glossy * Kt)[:, None] * M.gloss[None, :]).astype(F)
            if use_diffuse:
                dr = (Kt[:, None] * G.diffuse_reflect(wiN, woN, M)).astype(F)
                col = (col + G.on_factor(M, wi, wo, Nf)[:, None] * dr).astype(F)
                pdf = (pdf + wiN * w_df).astype(F)
            W = wiN / (pdf * F(0.99) + F(0.01))
            a, full = mask & wrong, mask & ~wrong
            out["wi"][mask] = wi[mask]
            out["ok"][a] = False
            for k, v in (("col", col), ("pdf", pdf), ("W", W)):
                out[k][full] = v[full]
            out["sflags"][full] = DIFF

        if use_glossy:  # C_GLOSSY
            Hs = G.aniso_sample(s1p, s2, M.exp_u, M.exp_v, trig) if M.aniso else G.blinn_sample(s1p, s2, M.exponent)
            H = (Hs[:, 0:1] * NU + Hs[:, 1:2] * NV + Hs[:, 2:3] * Nf).astype(F)
            cwoH = dot(wo, H)
            vn = F(2.0) * dot(H, Nf)
            Hr = (vn[:, None] * Nf - H).astype(F)
            H = np.where((cwoH < 0)[:, None], Hr, H).astype(F)
            cwoH = np.where(cwoH < 0, dot(wo, H), cwoH).astype(F)
            vn = dot(wo, H)
            wi = np.where((vn < 0)[:, None], -wo, ((F(2.0) * vn)[:, None] * H - wo)).astype(F)
            finish((comp == 1) & ~early, wi, H, Hs, cwoH, cos_Ng_wo * dot(Ng, wi) < 0)
        if use_diffuse:  # C_DIFFUSE
            wi = G.sample_cos_hemisphere(Nf, NU, NV, s1p, s2)
            H = normalize((wi + wo).astype(F))
            Hs = np.stack([dot(H, NU), dot(H, NV), dot(H, Nf)], 1).astype(F)
            finish((comp == 2) & ~early, wi, H, Hs, dot(wo, H), cos_Ng_wo * dot(Ng, wi) < 0)
        out["ok"][early] = False
        out["comp"] = np.where(early, -1, comp)
    return out


def coated_pdf(M, Ng, N, NU, NV, wo, wi, flags):
    """coatedGlossyMat_t::pdf, coatedglossy.cc:338-382"""
    n = len(wo)
    with np.errstate(all="ignore"):
        zero = dot(Ng, wo) * dot(Ng, wi) < 0
        Nf = G.face_forward(Ng, N, wo)
        Kr, Kt = fresnel(wo, Nf, M.ior)
        comps, width = widths(M, Kr, Kt, flags)
        if not comps:
            return np.zeros(n, F)
        total, pdf = np.zeros(n, F), np.zeros(n, F)
        for c, w in zip(comps, width):
            total = (total + w).astype(F)
            if c == 1:
                H = normalize((wi + wo).astype(F))
                pdf = (pdf + (G.lobe_d(M, H, NU, NV, dot(Nf, H)) / G.pdf_divisor(dot(wo, H))) * w).astype(F)
            elif c == 2:
                pdf = (pdf + np.abs(dot(wi, Nf)) * w).astype(F)
        r = (pdf / total).astype(F)
    return np.where(zero | (total.astype(D) < 0.00001), F(0.0), r).astype(F)


def coated_specular(M, Ng, N, wo, raylevel):
    """coatedGlossyMat_t::getSpecular, coatedglossy.cc:384-418 -> (refl, dir, col); raylevel is
    state.raylevel after recursiveRaytrace's increment (scalar or per row). dir and col are zero where
    nothing is reflected."""
    n = len(wo)
    raylevel = np.broadcast_to(np.asarray(raylevel), (n,))
    with np.errstate(all="ignore"):
        outside = dot(Ng, wo) >= 0
        cw = dot(N, wo)
        f = (1.00001 * cw.astype(D)).astype(F)
        bent = normalize((N - f[:, None] * wo).astype(F))
        keep = np.where(outside, cw >= 0, cw <= 0)
        Nn = np.where(keep[:, None], N, bent).astype(F)
        Ngg = np.where(outside[:, None], Ng, -Ng).astype(F)
        Kr, _ = fresnel(wo, Nn, M.ior)
        vn = F(2.0) * dot(wo, Nn)
        w = (vn[:, None] * Nn - wo).astype(F)
        col = (Kr[:, None] * M.mirror[None, :]).astype(F)
        c = dot(w, Ngg)
        fix = c.astype(D) < 0.01
        g = (0.01 - c.astype(D)).astype(F)
        w2 = normalize((w + g[:, None] * Ngg).astype(F))
        w = np.where(fix[:, None], w2, w).astype(F)
    refl = raylevel <= 5
    return refl, np.where(refl[:, None], w, F(0.0)).astype(F), np.where(refl[:, None], col, F(0.0)).astype(F)


# ---- direct lighting by Dirac lights, per shading point --------------------------

def lambert_eval(st, Ng, wo, wl):
    """shinyDiffuseMat_t::eval of a one-component DIFFUSE | REFLECT material on a flat surface: its diffuse
    strength times its colour where wl lies on wo's side of N"""
    assert st.type == 0 and st.ncomp == 1 and st.comp_flags[0] == DIFF and not st.oren_nayar
    dc = (F(st.component[3]) * f32(list(st.color))).astype(F)
    Nf = G.face_forward(Ng, Ng, wo)
    return np.where((dot(wl, Nf) < 0)[:, None], F(0.0), dc[None, :]).astype(F)


def surface_eval(st, Ng, NU, NV, wo, wl):
    if st.type == COATED:
        return coated_eval(Coated(st), Ng, Ng, NU, NV, wo, wl)
    if st.type == 2:
        return G.glossy_eval(G.Glossy(st), Ng, Ng, NU, NV, wo, wl)
    return lambert_eval(st, Ng, wo, wl)


def direct_dirac(orc, scene, P, Ng, mat, wo):
    """estimateAllDirectLight for Dirac lights (mcintegrator.cc:85-100) at the flat-shaded points P with
    geometric normal Ng, material ids mat and outgoing directions wo: isShadowed from the oracle (of the
    same geometry), eval from the restatements, products in the order the device keeps (R, G:
    (lcol * surf) * |N.l|; B: surf * (lcol * |N.l|)), lights summed from 0 in scene order. Only
    materials with BSDF_DIFFUSE are lit. Returns (colours, shadow rays traced)."""
    A = orc._A
    states = scene.material_states()
    NU, NV = G.create_cs(Ng)
    acc = np.zeros((len(P), 3), F)
    lit = np.array([bool(states[m].bsdf_flags & BSDF_DIFFUSE) for m in mat], bool)
    nshadow = 0
    for L in scene.light_states():
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
        nshadow += int(lit.sum())
        surf = np.zeros((len(P), 3), F)
        for m in np.unique(mat):
            k = mat == m
            surf[k] = surface_eval(states[m], Ng[k], NU[k], NV[k], wo[k], ldir[k])
        f = np.abs(dot(Ng, ldir))
        v = np.stack([(lcol[:, 0] * surf[:, 0]) * f, (lcol[:, 1] * surf[:, 1]) * f, surf[:, 2] * (lcol[:, 2] * f)], 1)
        v = np.where(occ.astype(bool)[:, None], F(0.0), v).astype(F)
        acc = (acc + (F(0.0) + v)).astype(F)
    acc = (F(0.0) + acc).astype(F)
    return np.where(lit[:, None], acc, F(0.0)).astype(F), nshadow


def hit_points(orc, rays):
    """closest hits of rays (n, 8) through the oracle -> (index of the rays that hit, P, Ng, material, wo)"""
    prim, t, _, _, _ = orc.intersect(rays)
    e = orc.arrays
    idx = np.flatnonzero(prim >= 0)
    frm, d = rays[idx, 0:3], rays[idx, 3:6]
    P = (frm + t[idx, None] * d).astype(F)
    return idx, P, e["tri_normal"][prim[idx]].astype(F), e["tri_material"][prim[idx]], (-d).astype(F)
