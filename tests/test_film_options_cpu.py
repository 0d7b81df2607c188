"""The film options (z_channel, premult_alpha, clamp_rgb) without a device:
the appended ABI fields, the batch planner's depth bytes, and the float32
restatements of tests/depth_common.py against tests/film_ref.py's float64
splat within its derived bound."""
import ctypes as C

import numpy as np
import pytest

from core_amd import _abi as A
from tests import depth_common as D
from tests import film_cases as FC
from tests import film_ref as R

F32, F64 = np.float32, np.float64
f3 = A.f3
GB = 1 << 30

# yk_render_params as it was before the film options were appended
OLD_FIELDS = [("integrator", C.c_int32), ("raydepth", C.c_int32), ("path_samples", C.c_int32),
              ("bounces", C.c_int32), ("caustic_type", C.c_int32), ("width", C.c_int32),
              ("height", C.c_int32), ("xstart", C.c_int32), ("ystart", C.c_int32),
              ("aa_samples", C.c_int32), ("aa_passes", C.c_int32), ("filter", C.c_int32),
              ("aa_pixelwidth", C.c_float), ("tile_size", C.c_int32),
              ("transp_background", C.c_int32), ("aa_inc_samples", C.c_int32), ("aa_threshold", C.c_float),
              ("photon", A.yk_photon_params), ("transp_shadows", C.c_int32), ("shadow_depth", C.c_int32),
              ("filter_width", C.c_float), ("tile_order", C.POINTER(C.c_int32)), ("tile_order_len", C.c_int32),
              ("do_ao", C.c_int32), ("ao_samples", C.c_int32), ("ao_distance", C.c_float), ("ao_color", f3),
              ("dl_caustics", C.c_int32)]
NEW_FIELDS = ["z_channel", "normalize_z_channel", "depth_min", "depth_inv_range", "depth_film", "premult_alpha",
              "clamp_rgb"]


class OldParams(C.Structure):
    _fields_ = OLD_FIELDS


def test_old_render_param_offsets_are_unchanged_and_the_new_tail_defaults_to_zero():
    for name, _ in OLD_FIELDS:
        assert getattr(A.yk_render_params, name).offset == getattr(OldParams, name).offset, name
        assert getattr(A.yk_render_params, name).size == getattr(OldParams, name).size, name
    names = [n for n, _ in A.yk_render_params._fields_]
    assert names == [n for n, _ in OLD_FIELDS] + NEW_FIELDS
    assert A.yk_render_params.z_channel.offset >= C.sizeof(OldParams) - 4  # appended, after every old byte in use
    assert A.yk_render_params.z_channel.offset == OldParams.dl_caustics.offset + 4
    p = A.yk_render_params()
    C.memset(C.byref(p), 0xFF, C.sizeof(p))
    A.lib().yk_render_params_default(C.byref(p))
    tail = bytes(p)[A.yk_render_params.z_channel.offset:]
    assert tail == bytes(len(tail))


def _plan(reserved, **kw):
    i = A.yk_batch_plan_in(reserved=reserved, **kw)
    o = A.yk_batch_plan()
    assert A.lib().yk_debug_batch_plan(C.byref(i), C.byref(o)) == o.status == A.YK_OK
    return o


PLAN_FIELDS = [n for n, _ in A.yk_batch_plan._fields_]


@pytest.mark.parametrize("kw", [
    dict(slots=1, bounces=4, merged=1, split=0, tile=32, spp=4, pipes=4, owned_tiles=64, budget_bytes=192 * GB),
    dict(slots=8, bounces=0, merged=0, split=1, tile=16, spp=3, pipes=4, owned_tiles=6, budget_bytes=64 * GB),
    dict(slots=2, bounces=0, merged=0, split=0, transp_shadows=1, tile=32, spp=1, pipes=2, owned_tiles=5,
         target_samples=1024, budget_bytes=64 * GB),
])
def test_depth_samples_add_four_bytes_per_sample_to_the_plan(monkeypatch, kw):
    monkeypatch.setenv("YK_DEBUG_HOOKS", "1")
    a, b = _plan(0, **kw), _plan(1, **kw)
    assert b.bytes_per_sample == a.bytes_per_sample + 4
    for n in PLAN_FIELDS:  # these frames are not bound by the budget: nothing else follows
        if n != "bytes_per_sample":
            assert getattr(a, n) == getattr(b, n), n


def test_depth_bytes_reach_a_budget_bound_plan(monkeypatch):
    """a budget that caps the batch: the cap is budget / pipes / bytes_per_sample
    (floored at 2^20 samples), so 4 B more per sample give whole tiles fewer"""
    monkeypatch.setenv("YK_DEBUG_HOOKS", "1")
    kw = dict(slots=1, bounces=0, merged=0, split=0, tile=32, spp=16, pipes=4, owned_tiles=1 << 14,
              budget_bytes=8 * GB)
    a, b = _plan(0, **kw), _plan(1, **kw)
    assert b.bytes_per_sample == a.bytes_per_sample + 4
    tile_samples = 32 * 32 * 16
    for o in (a, b):
        cap = max(1 << 20, (8 * GB) // 4 // o.bytes_per_sample)
        assert o.tiles_per_batch == cap // tile_samples and o.maxc == o.tiles_per_batch * tile_samples
        assert o.nbatch == -(-(1 << 14) // o.tiles_per_batch)
    assert b.tiles_per_batch < a.tiles_per_batch
    assert (a.regions, a.npipes) == (b.regions, b.npipes)
    # bit 0 only
    assert _plan(2, **kw).bytes_per_sample == a.bytes_per_sample


# ---------------------------------------------------------------- restatements

CASES = ["box_pw1", "box_pw3", "gauss_pw2", "mitchell_pw1.5", "spp9", "shard0of2_random", "adaptive_random30",
         "film_not_tile_multiple"]


def _alphas(rng, n):
    """0, 0.5, 1, above 1 and negative values among random ones in (0, 1.5)"""
    a = rng.uniform(0.0, 1.5, n).astype(F32)
    a[::7], a[1::7], a[2::7], a[3::7], a[4::7] = 0.0, 0.5, 1.0, 1.75, -0.5
    return a


@pytest.mark.parametrize("name", CASES)
def test_depth_restatement_lies_within_the_float64_splat_bound(name):
    c = FC.case(name)
    col, off, film_in = c.inputs
    v = col[:, 0].copy()
    film = D.depth_splat32(c.film, c.pixels, c.spp, v, off, film_in[..., [0, 4]])
    only_v = np.zeros_like(col)
    only_v[:, 0] = v
    f64, n, S = R.splat64(c.film, c.pixels, c.spp, only_v, off, film_in)
    bound = R.splat_bound(n, S)
    assert (np.abs(film[..., 0].astype(F64) - f64[..., 0]) <= bound[..., 0]).all()
    assert (np.abs(film[..., 1].astype(F64) - f64[..., 4]) <= bound[..., 4]).all()
    # the depth splat is the colour splat's channel 0 and weight, bit for bit
    ref = R.splat32(c.film, c.pixels, c.spp, only_v, off, film_in)
    assert (D.bits(film) == D.bits(ref[..., [0, 4]])).all()
    # a NaN sample adds nothing: the film of the others alone
    holes = v.copy()
    holes[::3] = np.nan
    zeroed = only_v.copy()
    zeroed[::3] = 0
    got = D.depth_splat32(c.film, c.pixels, c.spp, holes, off, np.zeros((c.film.h, c.film.w, 2), F32))
    keep = np.ones(len(v), bool)
    keep[::3] = False
    want64, n2, S2 = _splat64_subset(c, zeroed, off, keep)
    assert (np.abs(got[..., 0].astype(F64) - want64[..., 0]) <= R.splat_bound(n2, S2)[..., 0]).all()
    assert (np.abs(got[..., 1].astype(F64) - want64[..., 4]) <= R.splat_bound(n2, S2)[..., 4]).all()


def _splat64_subset(c, col, off, keep):
    """film_ref.splat64's scatter onto a zero film, of the kept samples alone"""
    P = c.film
    film = np.zeros((P.h, P.w, 5), F64)
    n = np.zeros((P.h, P.w), np.int64)
    S = np.zeros((P.h, P.w, 5), F64)
    for k, (x, y) in enumerate(c.pixels):
        for s in range(k * c.spp, (k + 1) * c.spp):
            fp = R._footprint(P, x, y, off[s, 0], off[s, 1])
            if fp is None or not keep[s]:
                continue
            sl, wt = fp
            term = wt.astype(F64)[:, :, None] * np.append(col[s].astype(F64), 1.0)[None, None, :]
            film[sl] += term
            S[sl] += np.abs(term)
            n[sl] += 1
    return film, n, S


@pytest.mark.parametrize("name", ["box_pw1", "spp9"])
def test_single_pixel_windows_premultiply_once(name):
    """offsets well inside the pixel under the narrowest box: every window is
    the sample's own pixel, m = 1, and the film is film_ref.splat64's of the
    once-premultiplied colours within its bound"""
    c = FC.case(name)
    col, off, film_in = c.inputs
    P = R.Film(*c.crop, c.tile, R.filterw(FC.BOX, 1.0), np.ones(256, F32))
    rng = np.random.default_rng(3)
    col = col.copy()
    col[:, 3] = _alphas(rng, len(col))
    off = (0.25 + 0.5 * off).astype(F32)
    film = D.colour_splat32(P, c.pixels, c.spp, col, off, film_in, premult=True)
    once = col.copy()
    once[:, :3] = col[:, :3] * col[:, 3:4]
    f64, n, S = R.splat64(P, c.pixels, c.spp, once, off, film_in)
    assert (n <= c.spp).all()
    assert (np.abs(film.astype(F64) - f64) <= R.splat_bound(n, S)).all()
    assert (D.bits(film) == D.bits(R.splat32(P, c.pixels, c.spp, once, off, film_in))).all()


@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("name", ["box_pw3", "gauss_pw2", "film_not_tile_multiple", "shard0of2_random"])
def test_compounded_premultiply_lies_within_the_float64_bound(name, clamp):
    """windows of several pixels: the m-th takes rgb * a^m. Against the float64
    scatter, with m more roundings per contribution than the plain splat:
    (n + 1 + m_max) 2^-24 S"""
    c = FC.case(name)
    col, off, film_in = c.inputs
    rng = np.random.default_rng(5)
    col = col.copy()
    col[:, 3] = _alphas(rng, len(col))
    film = D.colour_splat32(c.film, c.pixels, c.spp, col, off, film_in, clamp=clamp, premult=True)
    f64, n, S, mmax = D.colour_splat64(c.film, c.pixels, c.spp, col, off, film_in, clamp=clamp, premult=True)
    assert mmax > 1
    assert (np.abs(film.astype(F64) - f64) <= (n[:, :, None] + 1 + mmax) * R.U * S).all()
    # without the option the restatement is film_ref's splat
    plain = D.colour_splat32(c.film, c.pixels, c.spp, col, off, film_in)
    assert (D.bits(plain) == D.bits(R.splat32(c.film, c.pixels, c.spp, col, off, film_in))).all()
    # clamp alone: film_ref's splat of the clamped colours
    cl = D.colour_splat32(c.film, c.pixels, c.spp, col, off, film_in, clamp=True)
    assert (D.bits(cl) == D.bits(R.splat32(c.film, c.pixels, c.spp, D.clamp01(col), off, film_in))).all()


def test_clamp_keeps_nan_and_alpha():
    c = np.array([[-1.0, 0.5, 2.0, 3.0], [np.nan, 1.0, 0.0, -2.0]], F32)
    out = D.clamp01(c)
    assert out[0].tolist() == [0.0, 0.5, 1.0, 3.0]
    assert np.isnan(out[1, 0]) and out[1, 1:].tolist() == [1.0, 0.0, -2.0]


def test_resolve_restatements():
    film = FC.resolve_film()
    plain = D.resolve32(film)
    ref = R.resolve64(film)
    assert (np.abs(plain.astype(F64) - ref) <= 3 * R.U * np.abs(ref)).all()
    pre = D.resolve32(film, premult=True)
    assert (D.bits(pre[..., :3]) == D.bits(plain[..., :3] * plain[..., 3:4])).all()
    assert (D.bits(pre[..., 3]) == D.bits(plain[..., 3])).all()
    d = film[..., [0, 4]]
    z = D.depth_resolve32(d)
    assert (z[d[..., 1] <= 0] == 0).all()
    m = d[..., 1] > 0
    assert (D.bits(z[m]) == D.bits(d[..., 0][m] / d[..., 1][m])).all()
