"""imageFilm_t::nextPass (k_aa_flags, through yk_debug_aa_flags) and
imageFilm_t::flush (k_film_resolve) against the float64 restatements of
tests/film_ref.py.

Flags. Planted films of dyadic values, where every float operation is exact,
pin the comparison itself: >= at the threshold, abs of the centre, the signed
neighbour, weight 0 on either side, no down-left test in column 0, the last
row and column as neighbours only. Random films must give the float64 flags
except for pairs closer to the threshold than 8 * 2^-24 * (|c| + |b| + thr),
the rounding of the compiled form's operations; test_film_tables.py shows
those are at most 1 % of the pairs.

Resolve. Within 2^-23 |x| of col * (1 / weight) (two roundings); clamped and
zero-weight outputs exactly 0; alpha not clamped.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from core_amd import _abi as A
from tests import film_cases as FC
from tests import film_ref as R

F32, F64 = np.float32, np.float64
pytestmark = pytest.mark.gpu


def device_flags(dev, film, thr):
    film = np.ascontiguousarray(film, F32)
    h, w = film.shape[:2]
    out = np.full((h, w), 7, np.uint8)
    A.check(A.lib().yk_debug_aa_flags(dev._p, film.ctypes.data_as(A.fp), w, h, float(thr), out.ctypes.data))
    return out


@pytest.fixture
def hooks(monkeypatch):
    monkeypatch.setenv("YK_DEBUG_HOOKS", "1")


def test_planted_films(gpu_device, hooks):
    for film, thr, want in FC.planted_flag_films():
        got = device_flags(gpu_device, film, thr)
        assert (got == want).all(), (film[..., 1].tolist(), float(thr), got.tolist(), want.tolist())
        assert (got == R.next_pass_flags64(film, thr)[0]).all()


@pytest.mark.parametrize("name", FC.RANDOM_FLAG_FILMS)
def test_random_films(gpu_device, hooks, name):
    film, thr = FC.random_flag_film(name)
    got = device_flags(gpu_device, film, thr)
    _, pairs = R.next_pass_flags64(film, thr)
    hit = pairs["diff"] >= F64(thr)
    close = pairs["margin"] < FC.flag_margin(pairs, thr)
    assert close.mean() <= 0.01
    must = R.flags_from_pairs(got.shape, pairs, hit & ~close)
    may = R.flags_from_pairs(got.shape, pairs, hit | close)
    assert set(np.unique(got).tolist()) <= {0, 1}
    assert (got >= must).all() and (got <= may).all(), np.argwhere((got < must) | (got > may))[:8].tolist()


def test_resolve(gpu_device):
    film = FC.resolve_film()
    h, w = film.shape[:2]
    p = FC.render_params(A.YK_FILTER_BOX, 1.0, (0, 0, w, h), 8)
    d_film = torch.from_numpy(film).to(gpu_device.torch_device)
    got = gpu_device.film_resolve(p, d_film).cpu().numpy()
    want = R.resolve64(film)
    assert (np.abs(got.astype(F64) - want) <= 2.0 ** -23 * np.abs(want)).all()
    assert (got[want == 0] == 0).all()
    dead = film[..., 4] <= 0
    assert dead.any() and (got[dead] == 0).all()
    norm = film[..., :4].astype(F64) / np.where(dead, 1.0, film[..., 4].astype(F64))[..., None]
    clamped = (norm[..., :3] < 0) & ~dead[..., None]
    assert clamped.any() and (got[..., :3][clamped] == 0).all()
    neg_alpha = (norm[..., 3] < 0) & ~dead
    assert neg_alpha.any() and (got[..., 3][neg_alpha] < 0).all()
    assert (film[..., 4][~dead] < 2.0 ** -15).any()  # tiny weights are among the cases
