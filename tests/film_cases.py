"""The synthetic gather cases of the film tests: films of a few hundred
pixels that reach the gather's edges. The CPU tests check that the float32
reference splat lies within the derived bound of the float64 one on every
case; the GPU tests run the same cases through yk_debug_film_splat.

The filter table of a case is the oracle's (oracle.film_table, compared with
the closed forms in test_film_tables.py); everything else comes from
tests/film_ref.py.
"""
import ctypes as C
import functools

import numpy as np
import torch  # noqa: F401  (before libyk: one HIP runtime)

from core_amd import _abi as A
from oracle.oracle import film_table
from tests import film_ref as R

F32 = np.float32
BOX, MIT, GAUSS, LANC = A.YK_FILTER_BOX, A.YK_FILTER_MITCHELL, A.YK_FILTER_GAUSS, A.YK_FILTER_LANCZOS


def render_params(filt, pw, crop, tile, filter_width=0.0):
    p = A.yk_render_params()
    A.lib().yk_render_params_default(C.byref(p))
    p.filter, p.aa_pixelwidth, p.filter_width, p.tile_size = filt, pw, filter_width, tile
    p.xstart, p.ystart, p.width, p.height = crop
    return p


def random_order(ntiles, seed):
    """yk_tile_order_random: the reference's shuffled tile list (test_tile_order.py)"""
    out = (C.c_int32 * max(ntiles, 1))()
    A.check(A.lib().yk_tile_order_random(ntiles, seed, out))
    return np.array(out[:ntiles], np.int32)


def boundary_offsets(fw):
    """The float32 offsets at which an extent of addSample changes: either
    side of every dx in [0, 1) where dx - fw or dx + fw - 1 crosses
    k - (0.5 - 1.4e-11) for an integer k (Round2Int steps there; 2.8e-11, far
    less than a float32 step, from k - 1 + 0.5 - 1.4e-11); and 0, 2^-24, 0.5,
    the last float below 1."""
    fw = np.float64(F32(fw))
    out = [F32(0), F32(2.0 ** -24), F32(0.5), np.nextafter(F32(1), F32(0))]
    for k in range(-6, 7):
        for dx in (k - R.ROUND_EPS + fw, k - R.ROUND_EPS - fw + 1.0):
            if 0.0 <= dx < 1.0:
                f = F32(dx)
                out += [np.nextafter(f, F32(-1)), f, np.nextafter(f, F32(2))]
    out = sorted({float(v) for v in out if 0.0 <= v < 1.0})
    return np.array(out, F32)


def colours(rng, n, exact=False):
    """exact: small integers (every float32 sum of a box splat is exact);
    else negatives, zeros and magnitudes 2^-20 .. 2^4"""
    if exact:
        return rng.integers(-3, 8, size=(n, 4)).astype(F32)
    c = (rng.choice([-1.0, 1.0], size=(n, 4)) * 2.0 ** rng.uniform(-20, 4, size=(n, 4))).astype(F32)
    c[rng.random((n, 4)) < 0.1] = 0
    return c


def pattern_film(w, h):
    """a distinct finite bit pattern in every float of the film (~5e-4)"""
    bits = np.uint32(0x3A000000) + np.arange(w * h * 5, dtype=np.uint32) * np.uint32(977)
    return bits.view(F32).reshape(h, w, 5).copy()


class Case:
    def __init__(self, name, filt, pw, crop, tile, spp, *, filter_width=0.0, tpb=0, order=None, shard=0, nshards=1,
                 flags=None, film_in="pattern", offsets=None, exact=False, seed=1):
        self.name, self.filt, self.pw, self.crop, self.tile, self.spp = name, filt, pw, crop, tile, spp
        self.filter_width, self.tpb, self.order, self.shard, self.nshards = filter_width, tpb, order, shard, nshards
        self.flags, self.exact, self.seed = flags, exact, seed
        self._film_in, self._offsets = film_in, offsets

    def __repr__(self):
        return self.name

    @functools.cached_property
    def params(self):
        p = render_params(self.filt, self.pw, self.crop, self.tile, self.filter_width)
        if self.order is not None:
            self._keep = (C.c_int32 * len(self.order))(*[int(t) for t in self.order])
            p.tile_order = C.cast(self._keep, C.POINTER(C.c_int32))
            p.tile_order_len = len(self.order)
        return p

    @functools.cached_property
    def film(self):
        table, fw = film_table(render_params(self.filt, self.pw, self.crop, self.tile, self.filter_width))
        ref_fw = R.filterw(self.filt, self.pw, self.filter_width)
        assert F32(fw) == ref_fw, (fw, ref_fw)
        return R.Film(*self.crop, self.tile, ref_fw, table)

    @functools.cached_property
    def pixels(self):
        P = self.film
        return P.sample_pixels(P.shard_tiles(self.shard, self.nshards, self.order), self.flags)

    @functools.cached_property
    def inputs(self):
        """colours (n, 4), offsets (n, 2), film_in (h, w, 5)"""
        rng = np.random.default_rng(self.seed)
        n = len(self.pixels) * self.spp
        col = colours(rng, n, self.exact)
        if self._offsets is None:
            off = rng.random((n, 2), dtype=F32)
        else:  # every pair of the given offsets, in turn
            b = np.asarray(self._offsets, F32)
            i = np.arange(n)
            off = np.stack([b[i % len(b)], b[(i // len(b)) % len(b)]], axis=1)
        assert (off >= 0).all() and (off < 1).all()
        _, _, w, h = self.crop
        if isinstance(self._film_in, str):
            film_in = np.zeros((h, w, 5), F32) if self._film_in == "zero" else pattern_film(w, h)
        else:
            film_in = np.asarray(self._film_in, F32).reshape(h, w, 5)
        return col, off, film_in

    @functools.cached_property
    def ref64(self):
        return R.splat64(self.film, self.pixels, self.spp, *self.inputs)

    @functools.cached_property
    def ref32(self):
        return R.splat32(self.film, self.pixels, self.spp, *self.inputs)


def _ntiles(crop, tile):
    return ((crop[2] + tile - 1) // tile) * ((crop[3] + tile - 1) // tile)


@functools.lru_cache(maxsize=None)
def _first_splat(crop, tile):
    """a non-zero film for the adaptive passes: a first splat's float32 output"""
    c = Case("first", GAUSS, 3.0, crop, tile, 1, film_in="zero", seed=77)
    return c.ref32


def _adaptive_cases():
    crop, tile = (5, 3, 20, 14), 4
    ntiles = _ntiles(crop, tile)
    order = random_order(ntiles, 3)
    rng = np.random.default_rng(11)
    h, w = crop[3], crop[2]
    pats = {"random30": (rng.random((h, w)) < 0.3).astype(np.uint8)}
    one = np.zeros((h, w), np.uint8)
    one[9, 13] = 1
    pats["one_pixel"] = one
    # tiles_per_batch 2: the second batch of the hand-out order has no flagged pixel
    gap = (rng.random((h, w)) < 0.5).astype(np.uint8)
    P = R.Film(*crop, tile, 1.0, np.ones(256, F32))
    for t in order[2:4]:
        for x, y in P.tile_pixels(int(t)):
            gap[y - crop[1], x - crop[0]] = 0
    pats["empty_batch"] = gap
    pats["none"] = np.zeros((h, w), np.uint8)
    pats["all"] = np.ones((h, w), np.uint8)
    return [Case(f"adaptive_{k}", GAUSS, 3.0, crop, tile, 3, tpb=2, order=order, flags=f,
                 film_in=_first_splat(crop, tile), seed=40 + i) for i, (k, f) in enumerate(pats.items())]


@functools.lru_cache(maxsize=None)
def gather_cases():
    crop = (5, 3, 23, 13)
    cases = [
        Case("box_pw1", BOX, 1.0, crop, 8, 3),
        Case("box_pw3", BOX, 3.0, crop, 8, 3),
        Case("mitchell_pw1.5", MIT, 1.5, crop, 8, 3),
        Case("mitchell_fw1.7", MIT, 1.0, crop, 8, 3, filter_width=1.7),
        Case("gauss_pw2", GAUSS, 2.0, crop, 8, 3),
        Case("lanczos_pw2", LANC, 2.0, crop, 8, 3),
        Case("lanczos_pw8_tile4", LANC, 8.0, (5, 3, 12, 10), 4, 3),
        # small-integer colours under a box filter: every float32 sum is exact
        Case("exact_box_pw1", BOX, 1.0, crop, 8, 3, exact=True, film_in="zero"),
        Case("exact_box_pw3", BOX, 3.0, crop, 8, 3, exact=True, film_in="zero"),
        Case("exact_box_pw8_tile4", BOX, 8.0, (5, 3, 12, 10), 4, 2, exact=True, film_in="zero"),
    ]
    # Round2Int boundaries: every pair of the boundary offsets as (dx, dy)
    for filt, pw, fwidth in ((BOX, 1.0, 0.0), (BOX, 3.0, 0.0), (MIT, 1.0, 1.7), (LANC, 8.0, 0.0)):
        fw = R.filterw(filt, pw, fwidth)
        b = boundary_offsets(fw)
        c7 = (2, 1, 7, 5)
        spp = -(-len(b) ** 2 // (c7[2] * c7[3]))
        cases.append(Case(f"boundary_fw{float(fw):.3f}", filt, pw, c7, 4, spp, filter_width=fwidth, offsets=b))
        cases.append(Case(f"boundary_exact_fw{float(fw):.3f}", BOX, 2 * float(fw), c7, 4, spp,
                          filter_width=float(fw), offsets=b, exact=True, film_in="zero"))
    for spp in (1, 3, 8, 9, 16, 64, 65, 70):
        cases.append(Case(f"spp{spp}", BOX, 3.0, (0, 0, 10, 6), 4, spp, seed=spp))
    cases += [
        Case("film_1x1", GAUSS, 2.0, (3, 2, 1, 1), 4, 3),
        Case("film_1x9", GAUSS, 2.0, (3, 2, 1, 9), 4, 3),
        Case("film_9x1", GAUSS, 2.0, (3, 2, 9, 1), 4, 3),
        Case("film_3x2_fw4", LANC, 8.0, (0, 0, 3, 2), 4, 3),
        Case("film_narrower_than_tile", MIT, 1.5, (1, 1, 5, 11), 8, 2),
        Case("film_not_tile_multiple", MIT, 1.5, (1, 1, 11, 7), 4, 2),
    ]
    bc = (5, 3, 20, 14)
    for tpb in (1, 2, 5, 0):
        cases.append(Case(f"batches_tpb{tpb or 'all'}", GAUSS, 3.0, bc, 4, 2, tpb=tpb, seed=5))
    nt = _ntiles(bc, 4)
    orders = {"random1": random_order(nt, 1), "random9": random_order(nt, 9),
              "reversed": np.arange(nt - 1, -1, -1, dtype=np.int32)}
    for k, o in orders.items():
        for tpb in (1, 3):
            cases.append(Case(f"order_{k}_tpb{tpb}", GAUSS, 3.0, bc, 4, 2, tpb=tpb, order=o, seed=6))
    for nshards in (2, 3):
        for k, o in (("rowmajor", None), ("random", orders["random1"])):
            for shard in range(nshards):
                cases.append(Case(f"shard{shard}of{nshards}_{k}", GAUSS, 3.0, bc, 4, 2, tpb=3, order=o, shard=shard,
                                  nshards=nshards, film_in="zero", seed=7 + shard))
    return cases + _adaptive_cases()


def case(name):
    return {c.name: c for c in gather_cases()}[name]


def case_names():
    return [c.name for c in gather_cases()]


def check_shard_sum(shard_films, cases):
    """the shard films' float32 sum, in shard order, against the float64
    splat of the whole film: the shards' float64 films, counts and S add up to
    the whole film's (a shard that adds nothing to a pixel adds an exact 0)"""
    acc = shard_films[0].astype(F32)
    for f in shard_films[1:]:
        acc = acc + f.astype(F32)
    f64 = sum(c.ref64[0] for c in cases)
    n = sum(c.ref64[1] for c in cases)
    S = sum(c.ref64[2] for c in cases)
    assert (n > 0).all()
    assert (np.abs(acc.astype(np.float64) - f64) <= R.splat_bound(n, S)).all()


# ---------------------------------------------------------------- flag films

K_G = F32(0.7152)  # col2bri's weight of G; films with R = B = 0 keep every operation exact


def _g_film(g, weight=2.0):
    """film whose normalised colour is (0, g, 0) at weight `weight` (a power
    of two; 0 where g is None)"""
    g = np.array([[np.nan if v is None else v for v in row] for row in g], np.float64)
    film = np.zeros(g.shape + (5,), F32)
    film[..., 1] = np.where(np.isnan(g), 5.0, g * weight)  # a zero-weight pixel's colour is not read
    film[..., 4] = np.where(np.isnan(g), 0.0, weight)
    return film


def planted_flag_films():
    """(film, threshold, expected flags): dyadic values, every operation exact"""
    up = np.nextafter(K_G, F32(2))
    out = [
        # a difference equal to the threshold is flagged; one float below it is not
        (_g_film([[2, 1], [1, 1]]), K_G, [[1, 1], [1, 1]]),
        (_g_film([[2, 1], [1, 1]]), up, [[0, 0], [0, 0]]),
        # weight-0 centre (brightness 0) and weight-0 neighbour (the centre's own brightness)
        (_g_film([[None, 1], [0, 0]]), K_G, [[1, 1], [0, 0]]),
        (_g_film([[1, None], [1, 1]]), K_G, [[1, 1], [0, 0]]),
        # the centre's colour as abs: -1 against 1 is no difference; against 0 it is K_G
        (_g_film([[-1, 1], [1, 1]]), K_G, [[0, 0], [0, 0]]),
        (_g_film([[-1, 0], [1, 1]]), K_G, [[1, 1], [0, 0]]),
        # the neighbour's colour signed: 1 against -1 differs by 2 K_G
        (_g_film([[1, -1], [1, 1]]), F32(2) * K_G, [[1, 1], [0, 0]]),
        (_g_film([[1, -1], [1, 1]]), np.nextafter(F32(2) * K_G, F32(4)), [[0, 0], [0, 0]]),
        # column 0 has no down-left test: (0, 0) is not compared with the end of its own row
        (_g_film([[1, 1, 3], [1, 1, 1]]), K_G, [[0, 1, 1], [0, 0, 0]]),
        # down-left is tested elsewhere: centre (1, 0) against (0, 1)
        (_g_film([[1, 1, 1], [3, 1, 1]]), K_G, [[1, 1, 0], [1, 0, 0]]),
        # last row and last column are never centres, but flagged as neighbours
        (_g_film([[1, 1, 1], [1, 1, 1], [1, 3, 1]]), K_G, [[0, 0, 0], [1, 1, 0], [0, 1, 0]]),
        (_g_film([[1, 1, 1], [1, 1, 3], [1, 1, 1]]), K_G, [[0, 1, 0], [0, 1, 1], [0, 0, 0]]),
        (_g_film([[1, 1, 1], [1, 1, 1], [1, 1, 3]]), K_G, [[0, 0, 0], [0, 1, 0], [0, 0, 1]]),
        # one row or one column: nothing to compare
        (_g_film([[1, 3, 1, 3]]), K_G, [[0, 0, 0, 0]]),
        (_g_film([[1], [3], [1]]), K_G, [[0], [0], [0]]),
        # threshold <= 0: every pixel is resampled
        (_g_film([[1, 1], [1, 1]]), F32(0), [[1, 1], [1, 1]]),
        (_g_film([[1, 1, 1]]), F32(-1), [[1, 1, 1]]),
    ]
    return [(f, F32(t), np.array(w, np.uint8)) for f, t, w in out]


RANDOM_FLAG_FILMS = {"17x11": (17, 11, 21), "64x3": (64, 3, 22), "33x33": (33, 33, 23)}


def random_flag_film(name, thr=0.25):
    """sums of a smooth image plus noise, with negative colours, non-uniform
    weights (0.5 .. 4) and some weight-0 pixels"""
    w, h, seed = RANDOM_FLAG_FILMS[name]
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = 0.5 + 0.4 * np.sin(xx / 3.0)[..., None] * np.cos(yy / 2.0)[..., None]
    col = base + rng.normal(0, 0.15, (h, w, 4))
    col[rng.random((h, w)) < 0.05] *= -1
    weight = rng.uniform(0.5, 4.0, (h, w))
    weight[rng.random((h, w)) < 0.05] = 0
    film = np.zeros((h, w, 5), F32)
    film[..., :4] = col * np.where(weight > 0, weight, 1.0)[..., None]
    film[..., 4] = weight
    return film, F32(thr)


def flag_margin(pairs, thr):
    """8 * 2^-24 * (|c| + |b| + thr): the compiled form's operations (three
    products and two sums for c, a reciprocal, four products, two sums and two
    differences for the comparison) against float64"""
    return 8 * R.U * (np.abs(pairs["c"]) + np.abs(pairs["b"]) + np.float64(thr))


def resolve_film(seed=31, w=19, h=7):
    """film sums with weight 0, negative weights and sums, weights down to 2^-20"""
    rng = np.random.default_rng(seed)
    film = (rng.choice([-1.0, 1.0], (h, w, 5), p=[0.3, 0.7]) * 2.0 ** rng.uniform(-20, 4, (h, w, 5))).astype(F32)
    film[..., 4] = np.abs(film[..., 4])
    film[rng.random((h, w)) < 0.1, 4] = 0
    film[rng.random((h, w)) < 0.05, 4] *= -1
    return film
