"""Float32 restatements of the film options, sequential and in source order,
shared by tests/test_film_options_cpu.py, tests/test_film_options_gather.py
and tests/test_depth_render.py:

- imageFilm_t::addDepthSample (imagefilm.cc:513-564): addSample's window and
  table index, then val += val * w; weight += w. A NaN depth is a sample that
  never reaches addDepthSample (integrator.cc:293-297) and adds nothing.
- imageFilm_t::addSample with clamp and premultAlpha (imagefilm.cc:453-511):
  clampRGB01 once on the sample's copy; alphaPremultiply on that copy inside
  the pixel loop, so the m-th pixel of the window (row-major, after the clamp
  to the film area) takes the colour after m sequential RGB *= A.
- the camera samples' in-pixel offsets of renderTile (integrator.cc:270-286)
  and the depth sample of integrator.cc:313-334.

The windows and weights are tests/film_ref.py's (_footprint).
"""
import ctypes as C

import numpy as np

from tests import film_ref as R

F32, F64 = np.float32, np.float64
FAR = F32(99999997952.0)


def _each(P, pixels, spp, n):
    assert n == len(pixels) * spp, (n, len(pixels), spp)
    for i, (x, y) in enumerate(pixels):
        for s in range(i * spp, (i + 1) * spp):
            yield s, x, y


def depth_splat32(P, pixels, spp, depths, offsets, film_in):
    """-> film (h, w, 2) float32: {val, weight}"""
    depths = np.asarray(depths, F32).reshape(-1)
    offsets = np.asarray(offsets, F32).reshape(-1, 2)
    film = np.array(film_in, F32).reshape(P.h, P.w, 2)
    for s, x, y in _each(P, pixels, spp, len(depths)):
        v = depths[s]
        if np.isnan(v):
            continue
        fp = R._footprint(P, x, y, offsets[s, 0], offsets[s, 1])
        if fp is None:
            continue
        sl, wt = fp
        a = film[sl]
        with np.errstate(over="ignore", invalid="ignore"):
            a[:, :, 0] = a[:, :, 0] + wt * v
            a[:, :, 1] = a[:, :, 1] + wt
    return film


def clamp01(c):
    """colorA_t::clampRGB01 (color.h:119-124): a NaN passes both comparisons"""
    c = np.array(c, F32)
    rgb = c[..., :3]
    rgb[rgb < 0] = 0
    rgb[rgb > 1] = 1
    return c


def colour_splat32(P, pixels, spp, colours, offsets, film_in, clamp=False, premult=False):
    """-> film (h, w, 5) float32, pixel by pixel in the reference's loop order"""
    colours = np.asarray(colours, F32).reshape(-1, 4)
    offsets = np.asarray(offsets, F32).reshape(-1, 2)
    film = np.array(film_in, F32).reshape(P.h, P.w, 5)
    with np.errstate(over="ignore", invalid="ignore"):
        for s, x, y in _each(P, pixels, spp, len(colours)):
            fp = R._footprint(P, x, y, offsets[s, 0], offsets[s, 1])
            if fp is None:
                continue
            (ys, xs), wt = fp
            col = clamp01(colours[s]) if clamp else colours[s].copy()
            for j in range(ys.start, ys.stop):
                for i in range(xs.start, xs.stop):
                    if premult:
                        col[:3] = col[:3] * col[3]
                    w = wt[j - ys.start, i - xs.start]
                    film[j, i, :4] = film[j, i, :4] + col * w
                    film[j, i, 4] = film[j, i, 4] + w
    return film


def colour_splat64(P, pixels, spp, colours, offsets, film_in, clamp=False, premult=False):
    """The same scatter with every product and sum in float64 -> film, n
    (contributions per pixel), S (sum of magnitudes), mmax (largest m)"""
    colours = np.asarray(colours, F32).reshape(-1, 4)
    offsets = np.asarray(offsets, F32).reshape(-1, 2)
    film = np.asarray(film_in, F32).reshape(P.h, P.w, 5).astype(F64)
    S = np.abs(film)
    n = np.zeros((P.h, P.w), np.int64)
    mmax = 0
    for s, x, y in _each(P, pixels, spp, len(colours)):
        fp = R._footprint(P, x, y, offsets[s, 0], offsets[s, 1])
        if fp is None:
            continue
        (ys, xs), wt = fp
        col = (clamp01(colours[s]) if clamp else colours[s]).astype(F64)
        m = 0
        for j in range(ys.start, ys.stop):
            for i in range(xs.start, xs.stop):
                m += 1
                c = col.copy()
                if premult:
                    c[:3] = c[:3] * c[3] ** m
                w = F64(wt[j - ys.start, i - xs.start])
                term = np.append(c * w, w)
                film[j, i] += term
                S[j, i] += np.abs(term)
                n[j, i] += 1
        mmax = max(mmax, m)
    return film, n, S, mmax


def resolve32(film, premult=False):
    """imageFilm_t::flush: col * (float)(1.0 / weight), clampRGB0, then the
    premultiply (imagefilm.cc:408-423); weight <= 0 gives 0"""
    film = np.asarray(film, F32)
    w = film[..., 4]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        f = (1.0 / w.astype(F64)).astype(F32)
        out = np.where((w > 0)[..., None], film[..., :4] * f[..., None], F32(0)).astype(F32)
        rgb = out[..., :3]
        rgb[rgb < 0] = 0
        if premult:
            out[..., :3] = rgb * out[..., 3:4]
    return out


def depth_resolve32(depth):
    """pixelGray_t::normalized: weight > 0 ? val / weight : 0"""
    d = np.asarray(depth, F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d[..., 1] > 0, d[..., 0] / d[..., 1], F32(0)).astype(F32)


# ------------------------------------------------------------------ renders

def sample_offsets(p, spp):
    """(dx, dy) of every camera sample of a single-pass render of p's area,
    pixel-major, sample fastest: (0.5, 0.5) at spp 1, else
    ((0.5 + s) * d1, RI_LP(s + fnv(i * fnv(j))))"""
    from oracle import oracle as O
    L = O.lib()
    out = np.full((p.height, p.width, spp, 2), 0.5, F32)
    if spp > 1:
        d1 = F32(1.0 / F64(F32(spp)))
        for yy in range(p.height):
            for xx in range(p.width):
                i, j = p.ystart + yy, p.xstart + xx
                so = L.orc_fnv((i * L.orc_fnv(j)) & 0xFFFFFFFF)
                for s in range(spp):
                    out[yy, xx, s, 0] = (F32(0.5) + F32(s)) * d1
                    out[yy, xx, s, 1] = L.orc_ri_lp((s + so) & 0xFFFFFFFF, 0)
    return out.reshape(-1, 2)


def sample_depths(rays, prim, t, normalize=False, dmin=0.0, dinv=0.0):
    """integrator.cc:313-334 on camera rays (n, 8) and their hits"""
    tmax = np.where(prim >= 0, t, rays[:, 7]).astype(F32)
    if normalize:
        with np.errstate(over="ignore", invalid="ignore"):
            v = (F32(1.0) - (tmax - F32(dmin)) * F32(dinv)).astype(F32)
        return np.where(tmax > 0, v, F32(0)).astype(F32)
    return np.where(tmax <= 0, FAR, tmax).astype(F32)


def tile_major(P, per_pixel, spp):
    """reorder per-sample rows from pixel-major (row-major over the film) to
    the film's hand-out order (row-major tiles, a tile's pixels row-major)
    -> (pixels, rows)"""
    pixels = P.sample_pixels(P.shard_tiles())
    a = np.asarray(per_pixel).reshape(P.h, P.w, spp, -1)
    rows = np.concatenate([a[y - P.cy0, x - P.cx0] for x, y in pixels], axis=0)
    return pixels, rows


def render_film(p, table_of):
    """tests/film_ref.Film of render params p (table_of: oracle.film_table)"""
    table, fw = table_of(p)
    return R.Film(p.xstart, p.ystart, p.width, p.height, p.tile_size, fw, table)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def cptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))
