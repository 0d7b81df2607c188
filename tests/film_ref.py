"""An independent reference of the film stage, in plain numpy.

Written from imageFilm_t (imagefilm.cc:81-165 the filters and the
constructor, 213-271 nextPass, 400-424 flush, 453-511 addSample) and
math_utils.h:60-86 (Round2Int, Floor2Int). It calls neither the oracle nor
libyk: the filters are closed forms in float64, the splat is a literal
scatter in the reference's single-thread order, and nextPass / flush are
float64 restatements.
"""
import numpy as np

F32, F64 = np.float32, np.float64
BOX, MITCHELL, GAUSS, LANCZOS = 0, 1, 2, 3
U = 2.0 ** -24  # unit roundoff of float32
TABLE = 16      # FILTER_TABLE_SIZE
ROUND_EPS = 0.5 - 1.4e-11  # _doublemagicroundeps


# ------------------------------------------------------------------ filters

def mitchell_terms(r):
    """Mitchell-Netravali, B = C = 1/3, on x = 2r: the polynomial's terms
    (their sum is the filter value, the sum of their magnitudes scales its
    float32 rounding)."""
    x = 2.0 * np.asarray(r, F64)
    B = C = 1.0 / 3.0
    inner = np.stack([(12 - 9 * B - 6 * C) * x ** 3, (-18 + 12 * B + 6 * C) * x ** 2, 0 * x, (6 - 2 * B) + 0 * x]) / 6
    outer = np.stack([(-B - 6 * C) * x ** 3, (6 * B + 30 * C) * x ** 2, (-12 * B - 48 * C) * x, (8 * B + 24 * C) + 0 * x]) / 6
    t = np.where(x < 1.0, inner, outer)
    return np.where(x >= 2.0, 0.0, t)


def filter64(filt, r):
    r = np.asarray(r, F64)
    if filt == BOX:
        return np.ones_like(r)
    if filt == MITCHELL:
        return mitchell_terms(r).sum(axis=0)
    if filt == GAUSS:
        return np.maximum(0.0, np.exp(-6.0 * r * r) - np.exp(-6.0))
    if filt == LANCZOS:
        a, b = np.pi * r, np.pi * r / 2
        with np.errstate(invalid="ignore", divide="ignore"):
            v = np.sin(a) * np.sin(b) / (a * b)
        return np.where(r == 0, 1.0, np.where(r < 2.0, v, 0.0))
    raise ValueError(filt)


def table_radii():
    """r of the 16 x 16 table entries, row-major (y, x): ((x+.5)/16, (y+.5)/16)"""
    c = (np.arange(TABLE, dtype=F64) + 0.5) / TABLE
    return np.sqrt(c[None, :] ** 2 + c[:, None] ** 2).ravel()


def table64(filt):
    return filter64(filt, table_radii())


def filterw(filt, pixelwidth, filter_width=0.0):
    """The constructor's filterw: filterSize * 0.5 in double, stored as
    float; * 2.6f (Mitchell) or * 2.f (Gauss) in float; clamped to
    [0.501f, 4] in float. A filter_width > 0 is a live film's filterw as is."""
    if filter_width > 0:
        return F32(filter_width)
    fw = F32(F64(F32(pixelwidth)) * 0.5)
    if filt == MITCHELL:
        fw = F32(fw * F32(2.6))
    elif filt == GAUSS:
        fw = F32(fw * F32(2.0))
    return min(max(F32(0.501), fw), F32(4.0))


def table_scale(fw):
    return 0.9999 * TABLE / F64(F32(fw))


# -------------------------------------------------------------------- splat

def round2int(v):
    """Round2Int: int(val + (0.5 - 1.4e-11)), a C conversion (towards zero)"""
    return np.trunc(np.asarray(v, F64) + ROUND_EPS).astype(np.int64)


def floor2int(v):
    return np.floor(np.asarray(v, F64)).astype(np.int64)


class Film:
    """What the splat reads of a film: its area, tiles, filter width and table."""

    def __init__(self, x0, y0, w, h, tile, fw, table):
        self.cx0, self.cy0, self.w, self.h, self.tile = x0, y0, w, h, tile
        self.cx1, self.cy1 = x0 + w, y0 + h
        self.ntx, self.nty = (w + tile - 1) // tile, (h + tile - 1) // tile
        self.ntiles = self.ntx * self.nty
        self.fw = F64(F32(fw))
        self.scale = table_scale(fw)
        self.table = np.asarray(table, F32).reshape(TABLE * TABLE)

    def shard_tiles(self, shard=0, nshards=1, order=None):
        """The tiles t % nshards == shard in hand-out order (row-major or `order`)"""
        seq = range(self.ntiles) if order is None else [int(t) for t in order]
        return [t for t in seq if t % nshards == shard]

    def tile_pixels(self, t):
        X, Y = self.cx0 + (t % self.ntx) * self.tile, self.cy0 + (t // self.ntx) * self.tile
        W, H = min(self.tile, self.cx1 - X), min(self.tile, self.cy1 - Y)
        return [(x, y) for y in range(Y, Y + H) for x in range(X, X + W)]

    def sample_pixels(self, tiles, flags=None):
        """(x, y) of every pixel that takes samples, in the film's order:
        tiles as given, a tile's pixels row-major, only flagged ones if flags
        ((h, w), film-local) is given"""
        out = []
        for t in tiles:
            for x, y in self.tile_pixels(t):
                if flags is None or flags[y - self.cy0, x - self.cx0]:
                    out.append((x, y))
        return out


def _footprint(P, x, y, dx, dy):
    """addSample's target window and weights of one sample: film-local slices
    and the (rows, columns) float32 weights, or None if the window is empty"""
    dx, dy = F64(dx), F64(dy)
    dx0 = max(P.cx0 - x, int(round2int(dx - P.fw)))
    dx1 = min(P.cx1 - x - 1, int(round2int(dx + P.fw - 1.0)))
    dy0 = max(P.cy0 - y, int(round2int(dy - P.fw)))
    dy1 = min(P.cy1 - y - 1, int(round2int(dy + P.fw - 1.0)))
    if dx0 > dx1 or dy0 > dy1:
        return None
    xi = floor2int(np.abs((np.arange(dx0, dx1 + 1, dtype=F64) - (dx - 0.5)) * P.scale))
    yi = floor2int(np.abs((np.arange(dy0, dy1 + 1, dtype=F64) - (dy - 0.5)) * P.scale))
    wt = P.table[yi[:, None] * TABLE + xi[None, :]]
    return (slice(y + dy0 - P.cy0, y + dy1 - P.cy0 + 1), slice(x + dx0 - P.cx0, x + dx1 - P.cx0 + 1)), wt


def _samples(P, pixels, spp, colours, offsets):
    colours = np.asarray(colours, F32).reshape(-1, 4)
    offsets = np.asarray(offsets, F32).reshape(-1, 2)
    assert len(colours) == len(offsets) == len(pixels) * spp, (len(colours), len(pixels), spp)
    for i, (x, y) in enumerate(pixels):
        for s in range(i * spp, (i + 1) * spp):
            fp = _footprint(P, x, y, offsets[s, 0], offsets[s, 1])
            if fp is not None:
                yield fp[0], fp[1], colours[s]


def splat64(P, pixels, spp, colours, offsets, film_in):
    """-> film (h, w, 5) in float64; n (h, w) contributions per pixel;
    S (h, w, 5) = |film_in| + sum |w c| (weight channel: sum |w|)"""
    film = np.asarray(film_in, F32).reshape(P.h, P.w, 5).astype(F64)
    S = np.abs(film)
    n = np.zeros((P.h, P.w), np.int64)
    for sl, wt, c in _samples(P, pixels, spp, colours, offsets):
        w64 = wt.astype(F64)
        term = w64[:, :, None] * np.append(c.astype(F64), 1.0)[None, None, :]
        film[sl] += term
        S[sl] += np.abs(term)
        n[sl] += 1
    return film, n, S


def splat32(P, pixels, spp, colours, offsets, film_in):
    """The same scatter in float32: per contribution one rounded multiply,
    then one rounded add (the weight: one add), in the reference's order"""
    film = np.array(film_in, F32).reshape(P.h, P.w, 5)
    for sl, wt, c in _samples(P, pixels, spp, colours, offsets):
        v = film[sl]
        for k in range(4):
            v[:, :, k] = v[:, :, k] + wt * c[k]  # float32 * float32, float32 + float32
        v[:, :, 4] = v[:, :, 4] + wt
    return film


def splat_bound(n, S):
    """(n + 1) 2^-24 S: n rounded products summed sequentially onto the film"""
    return (n[:, :, None] + 1) * U * S


# ----------------------------------------------------------------- nextPass

W_R, W_G, W_B = (F64(F32(v)) for v in (0.2126, 0.7152, 0.0722))


def _normalized64(film):
    f = np.asarray(film, F32).astype(F64)
    w = f[..., 4:5]
    with np.errstate(divide="ignore", invalid="ignore"):
        c = f[..., :4] * (1.0 / w)
    return np.where(w > 0, c, 0.0)


def next_pass_flags64(film, thr):
    """-> flags (h, w) uint8 and the tested pairs as a dict of arrays:
    cx, cy, nx, ny, c (centre abscol2bri), b (neighbour col2bri), diff,
    margin = | |c - b| - thr |"""
    film = np.asarray(film, F32)
    h, w = film.shape[:2]
    thr = F64(F32(thr))
    flags = np.zeros((h, w), np.uint8)
    empty = {k: np.zeros(0, np.int64 if k in ("cx", "cy", "nx", "ny") else F64)
             for k in ("cx", "cy", "nx", "ny", "c", "b", "diff", "margin")}
    if not thr > 0:
        flags[:] = 1
        return flags, empty
    if w < 2 or h < 2:
        return flags, empty
    col = _normalized64(film)
    bri = W_R * col[..., 0] + W_G * col[..., 1] + W_B * col[..., 2]
    absbri = W_R * np.abs(col[..., 0]) + W_G * np.abs(col[..., 1]) + W_B * np.abs(col[..., 2])
    ys, xs = np.meshgrid(np.arange(h - 1), np.arange(w - 1), indexing="ij")
    ys, xs = ys.ravel(), xs.ravel()
    parts = []
    for ox, oy in ((1, 0), (0, 1), (1, 1), (-1, 1)):
        m = xs + ox >= 0 if ox >= 0 else xs > 0
        parts.append((xs[m], ys[m], xs[m] + ox, ys[m] + oy))
    cx, cy, nx, ny = (np.concatenate([p[k] for p in parts]) for k in range(4))
    c, b = absbri[cy, cx], bri[ny, nx]
    diff = np.abs(c - b)
    hit = diff >= thr
    flags[cy[hit], cx[hit]] = 1
    flags[ny[hit], nx[hit]] = 1
    return flags, dict(cx=cx, cy=cy, nx=nx, ny=ny, c=c, b=b, diff=diff, margin=np.abs(diff - thr))


def flags_from_pairs(shape, pairs, hit):
    f = np.zeros(shape, np.uint8)
    f[pairs["cy"][hit], pairs["cx"][hit]] = 1
    f[pairs["ny"][hit], pairs["nx"][hit]] = 1
    return f


# -------------------------------------------------------------------- flush

def resolve64(film):
    """col * (1 / weight); RGB clamped at 0, alpha not; weight <= 0 gives 0"""
    out = _normalized64(film)
    out[..., :3] = np.maximum(out[..., :3], 0.0)
    return out
