"""float32 restatement of the glossy material (glossyMat_t, glossy.cc, with
as_diffuse; microfacet.h; mathOptimizations.h fLog2 / fExp2 / fPow) in numpy,
in source order, and the constructor / initOrenNayar state. Shared by
tests/test_glossy.py. Every operation below rounds once, in the type the C++
source gives it; where that type is double the step says so.

The anisotropic sampler's atan / tanf are library calls the project does not
pin: `trig` supplies them (on the GPU tests, the device's own values through
the ATAN_TAN probe), everything downstream is restated bit for bit.
"""
import numpy as np

F = np.float32
D = np.float64
BSDF_GLOSSY, BSDF_DIFFUSE, BSDF_REFLECT, BSDF_ALL = 0x2, 0x4, 0x10, 0x7F
PI_D, TWO_PI_D, PI_2_D = 3.14159265358979323846, 6.28318530717958647692, 1.57079632679489661923


def f32(x):
    return np.ascontiguousarray(x, F)


# ---- mathOptimizations.h -------------------------------------------------

def fexp2(x):
    x = f32(x)
    with np.errstate(all="ignore"):
        x = np.where(F(129.0) < x, F(129.0), x)        # std::min(x, f_HI)
        x = np.where(x < F(-126.99999), F(-126.99999), x)  # std::max(x, f_LOW)
        ip = (x - F(0.5)).astype(np.int32)
        f = x - ip.astype(F)
        e = ((ip + 127).astype(np.uint32) << np.uint32(23)).view(F)
        poly = f * (f * (f * (f * (f * F(1.8775767e-3) + F(8.9893397e-3)) + F(5.5826318e-2)) + F(2.4015361e-1))
                    + F(6.9315308e-1)) + F(9.9999994e-1)
        return (e * poly).astype(F)


def flog2(x):
    i = f32(x).view(np.int32)
    e = (((i & 0x7F800000) >> 23) - 127).astype(F)
    m = ((i & 0x7FFFFF) | 0x3F800000).astype(np.int32).view(F)
    p2 = m * (m * F(-3.4436006e-2) + F(3.1821337e-1)) + F(-1.2315303)
    md = m.astype(D)  # POLYLOG's 2.5988452 is a double literal: double from here on
    p5 = md * (md * ((m * p2).astype(D) + 2.5988452) + D(F(-3.3241990))) + D(F(3.1157899))
    return (p5.astype(F) * (m - F(1.0)) + e).astype(F)


def fpow(a, b):
    a, b = np.broadcast_arrays(f32(a), f32(b))
    with np.errstate(all="ignore"):
        return fexp2(flog2(a) * b)


def fsin(x):
    """FAST_TRIG fSin as the device states it (yk_math.h fsin_ref)"""
    x = np.array(x, F)
    two_pi, k2 = F(6.28318530717958647692), np.uint32(0x40c90fda).view(F)
    kp = np.uint32(0x40490fda).view(F)
    with np.errstate(all="ignore"):
        m = (x > k2) | (x < -k2)
        x = np.where(m, x - (x * F(0.15915494309189533577)).astype(np.int32).astype(F) * two_pi, x).astype(F)
        x = np.where(x < -kp, x + two_pi, np.where(x > kp, x - two_pi, x)).astype(F)
        x = (F(1.27323954473516268615) * x) - ((F(0.40528473456935108578) * x) * np.abs(x))
        r = x + (np.abs(x) - F(1.0)) * (F(0.225) * x)
        r = np.where(r > F(1.0), F(1.0), r)
        return np.where(r < F(-1.0), F(-1.0), r).astype(F)


def fcos(x):
    return fsin(np.array(x, F) + F(1.57079632679489661923))


# ---- vectors -------------------------------------------------------------

def dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def normalize(v):
    ln = v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]
    with np.errstate(all="ignore"):
        inv = np.where(ln != 0, F(1.0) / np.sqrt(ln), F(1.0)).astype(F)
    return np.where((ln != 0)[:, None], v * inv[:, None], v).astype(F)


def create_cs(N):
    """createCS, vector3d.h:316-334"""
    N = f32(N)
    u, v = np.zeros_like(N), np.zeros_like(N)
    flat = (N[:, 0] == 0) & (N[:, 1] == 0)
    u[flat, 0] = np.where(N[flat, 2] < 0, F(-1), F(1))
    v[flat, 1] = F(1)
    g = ~flat
    with np.errstate(all="ignore"):
        d = F(1.0) / np.sqrt(N[:, 1] * N[:, 1] + N[:, 0] * N[:, 0])
        ug = np.stack([N[:, 1] * d, -N[:, 0] * d, np.zeros_like(d)], 1)
        vg = np.stack([N[:, 1] * ug[:, 2] - N[:, 2] * ug[:, 1], N[:, 2] * ug[:, 0] - N[:, 0] * ug[:, 2],
                       N[:, 0] * ug[:, 1] - N[:, 1] * ug[:, 0]], 1)
    u[g], v[g] = ug[g], vg[g]
    return u.astype(F), v.astype(F)


def sample_cos_hemisphere(N, Ru, Rv, s1, s2):
    z2 = (s2.astype(D) * TWO_PI_D).astype(F)
    c, s = fcos(z2), fsin(z2)
    with np.errstate(all="ignore"):
        sq1, sqz = np.sqrt(F(1.0) - s1), np.sqrt(s1)
    w = sq1[:, None] * (c[:, None] * Ru + s[:, None] * Rv) + sqz[:, None] * N
    return np.where((s1 >= F(1.0))[:, None], N, w).astype(F)


# ---- the material --------------------------------------------------------

class Glossy:
    """glossyMat_t's members as yk_material_state reports them, plus pDiffuse"""

    def __init__(self, st):
        self.gloss = f32(list(st.gloss_color))
        self.diff = f32(list(st.diff_color))
        self.exponent, self.exp_u, self.exp_v = F(st.exponent), F(st.exp_u), F(st.exp_v)
        self.mG, self.mD = F(st.reflectivity), F(st.m_diffuse)
        self.with_diffuse, self.aniso = bool(st.with_diffuse), bool(st.anisotropic)
        self.on, self.on_a, self.on_b = bool(st.oren_nayar), F(st.oren_nayar_a), F(st.oren_nayar_b)
        with np.errstate(all="ignore"):  # initBSDF, glossy.cc:94; std::min(0.6f, x): a NaN x gives 0.6
            x = F(1.0) - (self.mG / (self.mG + (F(1.0) - self.mG) * self.mD))
        self.pD = x if x < F(0.6) else F(0.6)


def state_of(color=(1, 1, 1), diffuse_color=(1, 1, 1), glossy_reflect=1.0, diffuse_reflect=0.0, exponent=50.0,
             as_diffuse=True, anisotropic=False, exp_u=50.0, exp_v=50.0, oren_nayar=False, sigma=0.1):
    """the constructor (glossy.cc:65-80), the factory's anisotropic block and initOrenNayar (glossy.cc:97-103)"""
    flags = 0
    with_diffuse = F(diffuse_reflect) > 0
    if with_diffuse:
        flags = BSDF_DIFFUSE | BSDF_REFLECT
    flags |= (BSDF_DIFFUSE | BSDF_REFLECT) if as_diffuse else (BSDF_GLOSSY | BSDF_REFLECT)
    st = dict(type=2, bsdf_flags=flags, gloss_color=tuple(F(c) for c in color),
              diff_color=tuple(F(c) for c in diffuse_color), exponent=F(exponent), exp_u=F(exp_u), exp_v=F(exp_v),
              reflectivity=F(glossy_reflect), m_diffuse=F(diffuse_reflect), as_diffuse=int(as_diffuse),
              with_diffuse=int(with_diffuse), anisotropic=int(anisotropic), oren_nayar=0, oren_nayar_a=F(0),
              oren_nayar_b=F(0))
    if oren_nayar:
        s2 = float(sigma) * float(sigma)
        st.update(oren_nayar=1, oren_nayar_a=F(1.0 - 0.5 * (s2 / (s2 + 0.33))), oren_nayar_b=F(0.45 * s2 / (s2 + 0.09)))
    return st


def pdf_divisor(c):
    return (8.0 * PI_D * (c * F(0.99) + F(0.04)).astype(D)).astype(F)


def as_divisor(cos1, cosI, cosO):
    mx = np.where(cosI < cosO, cosO, cosI)  # std::max(cosI, cosO)
    return (8.0 * PI_D * ((cos1 * mx) * F(0.99) + F(0.04)).astype(D)).astype(F)


def schlick(c, R):
    c1 = F(1.0) - c
    c2 = c1 * c1
    return R + ((F(1.0) - R) * c1 * c2 * c2)


def blinn_d(cos_h, e):
    return (e + F(1.0)) * fpow(cos_h, e)


def aniso_d(hx, hy, hz, e_u, e_v):
    with np.errstate(all="ignore"):
        ex = (e_u * hx * hx + e_v * hy * hy) / (F(1.00001) - hz * hz)
        d = np.sqrt((e_u + F(1.0)) * (e_v + F(1.0))) * fpow(np.where(F(0.0) < hz, hz, F(0.0)), ex)
    return np.where(hz <= 0, F(0.0), d).astype(F)


def lobe_d(M, H, NU, NV, cos_N_H):
    if M.aniso:
        return aniso_d(dot(H, NU), dot(H, NV), cos_N_H, M.exp_u, M.exp_v)
    return blinn_d(cos_N_H, M.exponent)


def oren_nayar(M, wi, wo, N):
    di, do = dot(N, wi), dot(N, wo)
    mi, mo = np.where(di < F(1.0), di, F(1.0)), np.where(do < F(1.0), do, F(1.0))
    cti, cto = np.where(F(-1.0) < mi, mi, F(-1.0)).astype(F), np.where(F(-1.0) < mo, mo, F(-1.0)).astype(F)
    v1 = normalize((wi - cti[:, None] * N).astype(F))
    v2 = normalize((wo - cto[:, None] * N).astype(F))
    d = dot(v1, v2)
    maxcos = np.where((cti < F(0.9999)) & (cto < F(0.9999)), np.where(F(0.0) < d, d, F(0.0)), F(0.0)).astype(F)
    with np.errstate(all="ignore"):
        si, so = np.sqrt(F(1.0) - cti * cti), np.sqrt(F(1.0) - cto * cto)
        ge = cto >= cti
        sin_alpha = np.where(ge, si, so)
        tan_beta = np.where(ge, so / np.where(cto == 0, F(1e-8), cto), si / np.where(cti == 0, F(1e-8), cti))
        return (M.on_a + M.on_b * maxcos * sin_alpha * tan_beta).astype(F)


def face_forward(Ng, N, I):
    return np.where((dot(Ng, I) < 0)[:, None], -N, N).astype(F)


def diffuse_reflect(wiN, woN, M):
    f_wi = F(1.0) - (F(0.5) * wiN)
    t = f_wi * f_wi
    f_wi = t * t * f_wi
    f_wo = F(1.0) - (F(0.5) * woN)
    t = f_wo * f_wo
    f_wo = t * t * f_wo
    k = (0.387507688 * D(M.mD) * D(F(1.0) - M.mG) * (F(1.0) - f_wi).astype(D) * (F(1.0) - f_wo).astype(D)).astype(F)
    return (k[:, None] * M.diff[None, :]).astype(F)


def on_factor(M, wi, wo, N):
    return oren_nayar(M, wi, wo, N) if M.on else np.ones(len(wi), F)


def glossy_eval(M, Ng, N, NU, NV, wo, wi, bsdfs=BSDF_ALL):
    """glossyMat_t::eval, glossy.cc:134-173"""
    n = len(wo)
    with np.errstate(all="ignore"):
        zero = (dot(Ng, wi) * dot(Ng, wo)) < 0
        if not (bsdfs & BSDF_DIFFUSE):
            return np.zeros((n, 3), F)
        Nf = face_forward(Ng, N, wo)
        wiN, woN = np.abs(dot(wi, Nf)), np.abs(dot(wo, Nf))
        H = normalize((wo + wi).astype(F))
        d = dot(wi, H)
        cwh = np.where(F(0.0) < d, d, F(0.0)).astype(F)
        glossy = lobe_d(M, H, NU, NV, dot(H, Nf)) * schlick(cwh, M.mG) / as_divisor(cwh, woN, wiN)
        col = (glossy[:, None] * M.gloss[None, :]).astype(F)
        if M.with_diffuse:
            dc = ((M.mD * (F(1.0) - M.mG)) * M.diff).astype(F)
            col = (col + on_factor(M, wi, wo, Nf)[:, None] * dc[None, :]).astype(F)
    return np.where(zero[:, None], F(0.0), col).astype(F)


def glossy_pdf(M, Ng, N, NU, NV, wo, wi, flags):
    """glossyMat_t::pdf, glossy.cc:307-351"""
    with np.errstate(all="ignore"):
        zero = dot(Ng, wo) * dot(Ng, wi) < 0
        Nf = face_forward(Ng, N, wo)
        use_glossy = bool(flags & BSDF_DIFFUSE)
        use_diffuse = M.with_diffuse and bool(flags & BSDF_DIFFUSE)
        pdf = np.abs(dot(wi, Nf)) if use_diffuse else np.zeros(len(wo), F)
        if use_glossy:
            H = normalize((wi + wo).astype(F))
            lobe = lobe_d(M, H, NU, NV, dot(Nf, H)) / pdf_divisor(dot(wo, H))
            pdf = pdf * M.pD + lobe * (F(1.0) - M.pD) if use_diffuse else lobe
    return np.where(zero, F(0.0), pdf).astype(F)


class HostTrig:
    """numpy's float32 atan / tan: for CPU-side use only (not the device's values)"""
    atanf = staticmethod(lambda x: np.arctan(f32(x)).astype(F))
    tanf = staticmethod(lambda x: np.tan(f32(x)).astype(F))


def sample_quadrant(s1, s2, e_u, e_v, trig):
    with np.errstate(all="ignore"):
        t = trig.tanf((PI_2_D * s1.astype(D)).astype(F))
        phi = trig.atanf((np.sqrt((e_u + F(1.0)) / (e_v + F(1.0))) * t).astype(F))
        cp, sp = fcos(phi), fsin(phi)
        cp2 = cp * cp
        sp2 = F(1.0) - cp2
        ct = fpow(F(1.0) - s2, F(1.0) / (e_u * cp2 + e_v * sp2 + F(1.0)))
        st = np.sqrt(F(1.0) - ct * ct)
    return np.stack([st * cp, st * sp, ct], 1).astype(F)


def aniso_quadrant_arg(s1):
    """AS_Aniso_Sample's quadrant choice: the s1 handed to sample_quadrant_aniso and the signs of H.x, H.y"""
    s1 = f32(s1)
    q = np.where(s1 < F(0.25), 0, np.where(s1 < F(0.5), 1, np.where(s1 < F(0.75), 2, 3)))
    arg = np.where(q == 0, F(4.0) * s1,
                   np.where(q == 1, F(1.0) - F(4.0) * (F(0.5) - s1),
                            np.where(q == 2, F(4.0) * (s1 - F(0.5)), F(1.0) - F(4.0) * (F(1.0) - s1)))).astype(F)
    sx = np.where((q == 1) | (q == 2), F(-1.0), F(1.0))
    sy = np.where((q == 2) | (q == 3), F(-1.0), F(1.0))
    return arg, sx, sy


def aniso_sample(s1, s2, e_u, e_v, trig):
    arg, sx, sy = aniso_quadrant_arg(s1)
    H = sample_quadrant(arg, s2, e_u, e_v, trig)
    H[:, 0] = np.where(sx < 0, -H[:, 0], H[:, 0])
    H[:, 1] = np.where(sy < 0, -H[:, 1], H[:, 1])
    return H


def blinn_sample(s1, s2, e):
    with np.errstate(all="ignore"):
        ct = fpow(F(1.0) - s2, F(1.0) / (e + F(1.0)))
        st = np.sqrt(F(1.0) - ct * ct)
    phi = (s1.astype(D) * TWO_PI_D).astype(F)
    return np.stack([st * fcos(phi), st * fsin(phi), ct], 1).astype(F)


def glossy_sample(M, Ng, N, NU, NV, wo, s1, s2, flags, trig=HostTrig):
    """glossyMat_t::sample, glossy.cc:176-305. Returns dict(ok, wi, col, pdf, W, sflags); wi and W start at
    zero, and ok = 0 marks the returns ahead of the W assignment (what they had written by then stays)."""
    n = len(wo)
    Ng, N, NU, NV, wo, s1, s2 = (f32(a) for a in (Ng, N, NU, NV, wo, s1, s2))
    out = dict(ok=np.ones(n, bool), wi=np.zeros((n, 3), F), col=np.zeros((n, 3), F), pdf=np.zeros(n, F),
               W=np.zeros(n, F), sflags=np.zeros(n, np.uint32))
    use_glossy = bool(flags & BSDF_DIFFUSE)
    use_diffuse = M.with_diffuse and bool(flags & BSDF_DIFFUSE)
    DR = BSDF_DIFFUSE | BSDF_REFLECT
    with np.errstate(all="ignore"):
        cos_Ng_wo = dot(Ng, wo)
        Nf = face_forward(Ng, N, wo)
        woN = np.abs(dot(wo, Nf))
        in_diff = np.zeros(n, bool)
        if use_diffuse:
            spD = M.pD if use_glossy else F(1.0)
            in_diff = s1 < spD
            s1d = (s1 / spD).astype(F)
            wi = sample_cos_hemisphere(Nf, NU, NV, s1d, s2)
            wrong = dot(Ng, wi) * cos_Ng_wo < 0
            wiN = np.abs(dot(wi, Nf))
            pdf = wiN
            glossy = np.zeros(n, F)
            if use_glossy:
                H = normalize((wi + wo).astype(F))
                cwoH, cwiH, cNH = dot(wo, H), np.abs(dot(wi, H)), dot(Nf, H)
                Dv = lobe_d(M, H, NU, NV, cNH)
                pdf = pdf * M.pD + (Dv / pdf_divisor(cwoH)) * (F(1.0) - M.pD)
                glossy = Dv * schlick(cwiH, M.mG) / as_divisor(cwiH, woN, wiN)
            col = (glossy[:, None] * M.gloss[None, :]).astype(F)
            col = (col + on_factor(M, wi, wo, Nf)[:, None] * diffuse_reflect(wiN, woN, M)).astype(F)
            W = wiN / (pdf * F(0.99) + F(0.01))
            no_refl = not (flags & BSDF_REFLECT)
            a = in_diff & wrong                 # return scolor: wi written, nothing else
            b = in_diff & ~wrong                # pdf and sampledFlags written
            full = b if not no_refl else np.zeros(n, bool)
            out["wi"][in_diff] = wi[in_diff]
            out["pdf"][b] = pdf[b]
            out["sflags"][b] = DR
            out["ok"][a] = False
            if no_refl:
                out["ok"][b] = False
            out["col"][full] = col[full]
            out["W"][full] = W[full]
            s1 = ((s1 - M.pD) / (F(1.0) - M.pD)).astype(F)
        rest = ~in_diff
        if use_glossy:
            Hs = aniso_sample(s1, s2, M.exp_u, M.exp_v, trig) if M.aniso else blinn_sample(s1, s2, M.exponent)
            H = (Hs[:, 0:1] * NU + Hs[:, 1:2] * NV + Hs[:, 2:3] * Nf).astype(F)
            cwoH = dot(wo, H)
            vn = F(2.0) * dot(H, Nf)
            Hr = (vn[:, None] * Nf - H).astype(F)
            H = np.where((cwoH < 0)[:, None], Hr, H).astype(F)
            cwoH = np.where(cwoH < 0, dot(wo, H), cwoH).astype(F)
            vn = dot(wo, H)
            wi = np.where((vn < 0)[:, None], -wo, ((F(2.0) * vn)[:, None] * H - wo)).astype(F)
            wrong = cos_Ng_wo * dot(Ng, wi) < 0
            wiN = np.abs(dot(wi, Nf))
            Dv = aniso_d(Hs[:, 0], Hs[:, 1], Hs[:, 2], M.exp_u, M.exp_v) if M.aniso else blinn_d(dot(H, Nf), M.exponent)
            pdf = Dv / pdf_divisor(cwoH)
            glossy = Dv * schlick(cwoH, M.mG) / as_divisor(cwoH, woN, wiN)
            col = (glossy[:, None] * M.gloss[None, :]).astype(F)
            if use_diffuse:
                pdf = wiN * M.pD + pdf * (F(1.0) - M.pD)
                col = (col + on_factor(M, wi, wo, Nf)[:, None] * diffuse_reflect(wiN, woN, M)).astype(F)
            W = wiN / (pdf * F(0.99) + F(0.01))
            a, full = rest & wrong, rest & ~wrong
            out["wi"][rest] = wi[rest]
            out["ok"][a] = False
            for k, v in (("col", col), ("pdf", pdf), ("W", W)):
                out[k][full] = v[full]
            out["sflags"][full] = DR
        # neither half (the mask lacks BSDF_DIFFUSE): W = 0 / 0.01, nothing else written
    return out
