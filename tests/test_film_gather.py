"""The film gather (k_pixel_extent, k_film_gather and the tile lists that feed
them) on synthetic samples, through yk_debug_film_splat
(include/yk_test_hooks_film.h): the renderer's own lists and launches, host
samples in place of rendered ones.

For every case of tests/film_cases.py the device film
1. equals the float32 reference splat bit for bit (contribution sets, table
   indices; tile, pixel and sample order),
2. lies within (n + 1) 2^-24 S of the float64 splat, per pixel and channel
   (n rounded products summed sequentially: derived, not tuned),
3. keeps the input film's bits where no contribution lands;
with a box filter and small-integer colours it equals the float64 splat
exactly and its weight channel is the contribution count. The references are
tests/film_ref.py's (test_film_tables.py checks them without a device).
"""
import ctypes as C

import numpy as np
import pytest

from core_amd import _abi as A
from tests import film_cases as FC
from tests import film_ref as R

F32, F64 = np.float32, np.float64
pytestmark = pytest.mark.gpu


def device_splat(dev, c, col=None, off=None, n=None, params=None, check=True):
    """yk_debug_film_splat on case c -> (return code, film)"""
    ccol, coff, film_in = c.inputs
    col = np.ascontiguousarray(ccol if col is None else col, F32)
    off = np.ascontiguousarray(coff if off is None else off, F32)
    film = np.array(film_in, F32)
    flags = None if c.flags is None else np.ascontiguousarray(c.flags, np.uint8)
    p = c.params if params is None else params
    rc = A.lib().yk_debug_film_splat(dev._p, C.byref(p), c.shard, c.nshards, c.spp, c.tpb,
                                     None if flags is None else flags.ctypes.data, col.ctypes.data_as(A.fp),
                                     off.ctypes.data_as(A.fp), len(col) if n is None else n, film.ctypes.data_as(A.fp))
    if check:
        A.check(rc)
    return rc, film


@pytest.fixture
def hooks(monkeypatch):
    monkeypatch.setenv("YK_DEBUG_HOOKS", "1")


def _last_plan(dev):
    lp = A.yk_last_plan()
    return A.lib().yk_debug_last_plan(dev._p, C.byref(lp)), bytes(lp)


@pytest.mark.parametrize("name", FC.case_names())
def test_gather_against_the_reference_splats(gpu_device, hooks, name):
    c = FC.case(name)
    before = _last_plan(gpu_device)
    _, film = device_splat(gpu_device, c)
    assert _last_plan(gpu_device) == before  # the hook leaves the handle's plan and batch buffers alone
    f64, n, S = c.ref64
    film_in = c.inputs[2]
    bad = np.argwhere(film.view(np.uint32) != c.ref32.view(np.uint32))
    assert len(bad) == 0, (len(bad), bad[:6].tolist())
    assert (np.abs(film.astype(F64) - f64) <= R.splat_bound(n, S)).all()
    assert (film[n == 0].view(np.uint32) == film_in[n == 0].view(np.uint32)).all()
    if c.exact:
        assert (film.astype(F64) == f64).all() and (film[..., 4] == n).all()
    if c.flags is not None and not c.flags.any():
        assert (film.view(np.uint32) == film_in.view(np.uint32)).all()


def test_batch_cuts_do_not_change_a_bit(gpu_device, hooks):
    cases = [FC.case(f"batches_tpb{t}") for t in (1, 2, 5, "all")]
    films = [device_splat(gpu_device, c)[1] for c in cases]
    for c, f in zip(cases, films):
        assert all((a == b).all() for a, b in zip(c.inputs, cases[0].inputs))  # the same samples
        assert (f.view(np.uint32) == films[0].view(np.uint32)).all(), c.name


@pytest.mark.parametrize("order", ["rowmajor", "random"])
@pytest.mark.parametrize("nshards", [2, 3])
def test_shard_films_sum_to_the_whole_film(gpu_device, hooks, nshards, order):
    cases = [FC.case(f"shard{s}of{nshards}_{order}") for s in range(nshards)]
    FC.check_shard_sum([device_splat(gpu_device, c)[1] for c in cases], cases)


def test_bad_arguments_are_refused_before_any_launch(gpu_device, hooks):
    c = FC.case("gauss_pw2")
    col, off, film_in = c.inputs

    def refused(**kw):
        rc, film = device_splat(gpu_device, c, check=False, **kw)
        return rc == A.YK_ERR_ARG and (film.view(np.uint32) == film_in.view(np.uint32)).all()

    assert refused(col=col[:-c.spp], off=off[:-c.spp])  # one pixel's samples short
    assert refused(n=len(col) - 1)
    for v in (1.0, -2.0 ** -30, float("nan")):
        for k in (0, 1):
            bad = off.copy()
            bad[len(bad) // 2, k] = v
            assert refused(off=bad), (v, k)
    for fwidth, pw in ((4.5, c.pw), (0.3, c.pw), (-1.0, c.pw), (0.0, float("nan"))):
        assert refused(params=FC.render_params(c.filt, pw, c.crop, c.tile, fwidth)), (fwidth, pw)
    assert device_splat(gpu_device, c)[0] == A.YK_OK
