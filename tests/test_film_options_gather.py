"""The gather's film options on synthetic samples, through the hooks
(yk_debug_film_splat with premult_alpha / clamp_rgb, yk_debug_depth_splat):
the renderer's own tile lists and launches on a 40 x 24 film at (5, 3) with
16-pixel tiles, so both edges have partial tiles.

The premultiply and clamp films equal the float32 restatement of
tests/depth_common.py bit for bit: the same operations in the same order with
contraction off, so no tolerance. (Where a sum is NaN both are NaN; which NaN
an operation returns is not part of IEEE 754's value semantics and is not
compared.) The depth film equals channel 0 and the weight of the colour film
fed (v, 0, 0, 0), bit for bit, and NaN entries add neither value nor weight.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from core_amd import _abi as A
from tests import depth_common as D
from tests import film_cases as FC
from tests import film_ref as R

F32 = np.float32
pytestmark = pytest.mark.gpu
CROP, TILE = (5, 3, 40, 24), 16
NT = 3 * 2


@pytest.fixture
def hooks(monkeypatch):
    monkeypatch.setenv("YK_DEBUG_HOOKS", "1")


@functools.lru_cache(maxsize=None)
def _mask():
    rng = np.random.default_rng(17)
    m = (rng.random((CROP[3], CROP[2])) < 0.3).astype(np.uint8)
    m[0, 0] = m[-1, -1] = m[15, 15] = m[16, 16] = 1
    return m


# name: filter, pixel width, spp, shards, tiles per batch (0: all), random order, adaptive mask
CONFIGS = {
    "box1.0_spp1": (FC.BOX, 1.0, 1, 1, 0, False, False),
    "box1.0_spp3_2shards_tpb1": (FC.BOX, 1.0, 3, 2, 1, False, False),
    "box1.5_spp9_tpb1_random": (FC.BOX, 1.5, 9, 1, 1, True, False),
    "box1.5_spp3_2shards_random": (FC.BOX, 1.5, 3, 2, 0, True, False),
    "box1.5_spp3_adaptive": (FC.BOX, 1.5, 3, 1, 0, False, True),
    "gauss3.0_spp1_tpb1": (FC.GAUSS, 3.0, 1, 1, 1, False, False),
    "gauss3.0_spp3_2shards_random": (FC.GAUSS, 3.0, 3, 2, 0, True, False),
    "gauss3.0_spp3_adaptive_tpb1_random": (FC.GAUSS, 3.0, 3, 1, 1, True, True),
    "gauss3.0_spp9": (FC.GAUSS, 3.0, 9, 1, 0, False, False),
}
# every variant on the cheap configurations, the combined one everywhere
ALL_MODES = [(False, True), (True, False), (True, True)]


def _modes(name):
    return [(True, True)] if name.startswith("gauss3.0_spp") and "spp1" not in name else ALL_MODES


@functools.lru_cache(maxsize=None)
def _cases(name):
    filt, pw, spp, nshards, tpb, rnd, adaptive = CONFIGS[name]
    order = FC.random_order(NT, 5) if rnd else None
    return [FC.Case(f"{name}_{s}", filt, pw, CROP, TILE, spp, tpb=tpb, order=order, shard=s, nshards=nshards,
                    flags=_mask() if adaptive else None, seed=100 + s) for s in range(nshards)]


@functools.lru_cache(maxsize=None)
def _inputs(name, shard):
    """colours below 0, above 1 and NaN; alphas 0, 0.5, 1, above 1, negative"""
    c = _cases(name)[shard]
    col, off, film_in = c.inputs
    rng = np.random.default_rng(7 + shard)
    col = col.copy()
    n = len(col)
    a = rng.uniform(0.0, 1.25, n).astype(F32)
    a[::11], a[1::11], a[2::11], a[3::11], a[4::11] = 0.0, 0.5, 1.0, 1.5, -0.75
    col[:, 3] = a
    col[5::13, :3] = rng.uniform(0.0, 1.0, (len(col[5::13]), 3)).astype(F32)  # inside [0, 1] too
    for k, ch in ((n // 5, 0), (n // 2, 1), (n - 3, 2)):
        col[k, ch] = np.nan
    assert (col[:, :3] < 0).any() and (col[:, :3] > 1).any()
    return col, off, film_in


def _film_splat(dev, c, col, off, film_in, clamp=False, premult=False):
    p = c.params.copy()
    p.clamp_rgb, p.premult_alpha = int(clamp), int(premult)
    col = np.ascontiguousarray(col, F32)
    off = np.ascontiguousarray(off, F32)
    film = np.array(film_in, F32)
    flags = None if c.flags is None else np.ascontiguousarray(c.flags, np.uint8)
    A.check(A.lib().yk_debug_film_splat(dev._p, C.byref(p), c.shard, c.nshards, c.spp, c.tpb,
                                        None if flags is None else flags.ctypes.data, D.cptr(col), D.cptr(off),
                                        len(col), D.cptr(film)))
    return film


def _depth_splat(dev, c, v, off, film_in, check=True, n=None):
    """yk_debug_depth_splat (include/yk_test_hooks_depth.h), bound here: the
    hook is not part of the product ABI table"""
    f = A.lib().yk_debug_depth_splat
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.POINTER(A.yk_render_params), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                  A.fp, A.fp, C.c_int64, A.fp]
    v = np.ascontiguousarray(v, F32)
    off = np.ascontiguousarray(off, F32)
    film = np.array(film_in, F32)
    flags = None if c.flags is None else np.ascontiguousarray(c.flags, np.uint8)
    rc = f(dev._p, C.byref(c.params), c.shard, c.nshards, c.spp, c.tpb, None if flags is None else flags.ctypes.data,
           D.cptr(v), D.cptr(off), len(v) if n is None else n, D.cptr(film))
    if check:
        A.check(rc)
    return rc, film


def _same(a, b):
    """bit for bit, a NaN matching any NaN"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return (D.bits(a) == D.bits(b)) | (np.isnan(a) & np.isnan(b))


@pytest.mark.parametrize("name", list(CONFIGS))
def test_premultiply_and_clamp_films_equal_the_restatement(gpu_device, hooks, name):
    for c in _cases(name):
        col, off, film_in = _inputs(name, c.shard)
        for clamp, premult in _modes(name):
            film = _film_splat(gpu_device, c, col, off, film_in, clamp, premult)
            want = D.colour_splat32(c.film, c.pixels, c.spp, col, off, film_in, clamp=clamp, premult=premult)
            bad = np.argwhere(~_same(film, want))
            assert len(bad) == 0, (c.name, clamp, premult, len(bad), bad[:6].tolist())
            assert np.isfinite(want).mean() > 0.8  # the NaN samples leave most of the film checked
        # both options off: the film of every other render
        plain = _film_splat(gpu_device, c, col, off, film_in)
        assert _same(plain, D.colour_splat32(c.film, c.pixels, c.spp, col, off, film_in)).all()


def test_the_options_change_the_film(gpu_device, hooks):
    c = _cases("box1.5_spp3_2shards_random")[0]
    col, off, film_in = _inputs("box1.5_spp3_2shards_random", 0)
    films = [_film_splat(gpu_device, c, col, off, film_in, cl, pm) for cl, pm in [(False, False)] + ALL_MODES]
    for i in range(len(films)):
        for j in range(i):
            assert not _same(films[i], films[j]).all(), (i, j)
    # clamp first, once, then the compounding: not the other way round
    pre_then_clamp = D.colour_splat32(c.film, c.pixels, c.spp, col, off, film_in, premult=True)
    assert not _same(films[3], pre_then_clamp).all()


@pytest.mark.parametrize("name", list(CONFIGS))
def test_depth_splat_equals_one_colour_channel_and_skips_nan(gpu_device, hooks, name):
    for c in _cases(name):
        col, off, film_in = c.inputs
        v = col[:, 0].copy()
        depth_in = np.ascontiguousarray(film_in[..., [0, 4]])
        _, depth = _depth_splat(gpu_device, c, v, off, depth_in)
        only_v = np.zeros_like(col)
        only_v[:, 0] = v
        film = _film_splat(gpu_device, c, only_v, off, film_in)
        assert (D.bits(depth) == D.bits(film[..., [0, 4]])).all(), c.name
        # NaN entries: the film of the others alone, val and weight
        holes = v.copy()
        holes[::3] = np.nan
        holes[len(holes) // 2:len(holes) // 2 + 2 * c.spp] = np.nan  # two whole pixels
        _, got = _depth_splat(gpu_device, c, holes, off, depth_in)
        want = D.depth_splat32(c.film, c.pixels, c.spp, holes, off, depth_in)
        assert not np.isnan(got).any()
        assert (D.bits(got) == D.bits(want)).all(), c.name
        # nothing but NaN: not a bit of the film changes
        _, same = _depth_splat(gpu_device, c, np.full_like(v, np.nan), off, depth_in)
        assert (D.bits(same) == D.bits(depth_in)).all()


def test_shard_depth_films_sum_to_the_whole(gpu_device, hooks):
    name = "gauss3.0_spp3_2shards_random"
    cases = _cases(name)
    zero = np.zeros((CROP[3], CROP[2], 2), F32)
    films = [_depth_splat(gpu_device, c, c.inputs[0][:, 0], c.inputs[1], zero)[1] for c in cases]
    # as film_cases.check_shard_sum: the shards' float64 films, counts and S add
    # up to the whole film's; channel 0 and the weight of the cases' own colours
    acc = films[0] + films[1]
    refs = [R.splat64(c.film, c.pixels, c.spp, c.inputs[0], c.inputs[1], np.zeros((CROP[3], CROP[2], 5), F32))
            for c in cases]
    f64, n, S = (sum(r[k] for r in refs) for k in range(3))
    b = R.splat_bound(n, S)
    assert (n > 0).all()
    assert (np.abs(acc[..., 0].astype(np.float64) - f64[..., 0]) <= b[..., 0]).all()
    assert (np.abs(acc[..., 1].astype(np.float64) - f64[..., 4]) <= b[..., 4]).all()


def test_depth_hook_refusals(gpu_device, hooks, monkeypatch):
    c = _cases("box1.0_spp1")[0]
    col, off, film_in = c.inputs
    depth_in = np.ascontiguousarray(film_in[..., [0, 4]])
    v = col[:, 0]
    rc, film = _depth_splat(gpu_device, c, v, off, depth_in, check=False, n=len(v) - 1)
    assert rc == A.YK_ERR_ARG and (D.bits(film) == D.bits(depth_in)).all()
    bad = off.copy()
    bad[3, 1] = 1.0
    rc, film = _depth_splat(gpu_device, c, v, bad, depth_in, check=False)
    assert rc == A.YK_ERR_ARG and (D.bits(film) == D.bits(depth_in)).all()
    monkeypatch.delenv("YK_DEBUG_HOOKS")
    rc, _ = _depth_splat(gpu_device, c, v, off, depth_in, check=False)
    assert rc == A.YK_ERR_UNSUPPORTED
