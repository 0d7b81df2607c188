"""The film's filter tables against float64 closed forms, and the film
reference's own self-checks (no GPU).

Tables: oracle.film_table (the bits libyk builds, test_film_state.py) entry by
entry against tests/film_ref.py's closed forms, with a bound derived per entry:
box exact; Mitchell 8 * 2^-24 * (sum of the polynomial's |terms|); Gauss and
Lanczos2 go through the reference's fExp2 and FAST_TRIG fSin, whose errors are
measured from the reference's own recorded outputs (tests/golden/ref_qmc.npz)
over the argument ranges the tables use and propagated per entry, plus the
float32 rounding of the remaining operations, doubled for the evaluation order
of -ffast-math.

Self-checks: on every gather case of tests/film_cases.py the float32 splat
lies within (n + 1) 2^-24 S of the float64 splat (this proves the bound and the
case inputs before any device is involved), the box / small-integer cases are
exact, and the random films of the flag tests skip at most 1 % of their pairs.
"""
import ctypes as C
import os

import numpy as np
import pytest

from core_amd import _abi as A
from oracle.oracle import film_table
from tests import film_cases as FC
from tests import film_ref as R
from tests.conftest import GOLDEN

F32, F64 = np.float32, np.float64
U = R.U
FILTERS = {"box": A.YK_FILTER_BOX, "mitchell": A.YK_FILTER_MITCHELL, "gauss": A.YK_FILTER_GAUSS,
           "lanczos": A.YK_FILTER_LANCZOS}
WIDTHS = [1.0, 1.5, 2.2, 4.0, 8.0]
R_MAX = np.sqrt(2.0) * 15.5 / 16  # the largest r of a table entry
LOG2E6 = 6.0 * np.log2(np.e)


def _params(filt, pw):
    p = A.yk_render_params()
    A.lib().yk_render_params_default(C.byref(p))
    p.filter, p.aa_pixelwidth = filt, pw
    return p


def test_constants_agree_with_the_abi():
    assert (R.BOX, R.MITCHELL, R.GAUSS, R.LANCZOS) == tuple(FILTERS.values())


@pytest.mark.parametrize("pw", WIDTHS + [0.5, 100.0])
@pytest.mark.parametrize("filt", FILTERS.values(), ids=FILTERS.keys())
def test_filterw_is_the_constructors_arithmetic(filt, pw):
    _, fw = film_table(_params(filt, pw))
    assert F32(fw) == R.filterw(filt, pw) and F32(0.501) <= F32(fw) <= F32(4.0)


def _measured(name_in, name_out, lo, hi, truth, relative):
    """Largest error of the reference's recorded function over [lo, hi];
    fails, naming the range, unless the records cover it (a record within
    1/256 of the range of each end, no gap wider than that)."""
    g = np.load(os.path.join(GOLDEN, "ref_qmc.npz"))
    x = g[name_in].astype(F64)
    y = g[name_out].view(F32).astype(F64)
    m = (x >= lo) & (x <= hi)
    xs = np.sort(x[m])
    step = (hi - lo) / 256
    covered = len(xs) >= 256 and xs[0] - lo <= step and hi - xs[-1] <= step and np.diff(xs).max() <= step
    assert covered, f"ref_qmc.npz: {name_out} records do not cover [{lo}, {hi}]"
    err = np.abs(y[m] - truth(x[m]))
    return float((err / np.abs(truth(x[m]))).max() if relative else err.max())


def eps_sin():
    """absolute error of FAST_TRIG fSin over a = pi r and over b = pi r / 2"""
    return max(_measured("f_in", "fsin", 0.0, np.pi * R_MAX, np.sin, False),
               _measured("f_in", "fsin", 0.0, np.pi * R_MAX / 2, np.sin, False))


def eps_exp2():
    """relative error of fExp2 over -6 log2(e) r^2"""
    return _measured("e_in", "fexp2", -LOG2E6 * R_MAX ** 2, 0.0, np.exp2, True)


def table_bound(filt):
    """per-entry bound of |table - closed form| (see the module docstring)"""
    r = R.table_radii()
    v = np.abs(R.table64(filt))
    if filt == R.BOX:
        return np.zeros_like(r)
    if filt == R.MITCHELL:
        return 8 * U * np.abs(R.mitchell_terms(r)).sum(axis=0)
    if filt == R.GAUSS:
        # x = fl(r^2 * fl(-6 log2 e)), r^2 exact: two roundings of the argument, each
        # ln2 |x| 2^-24 relative in 2^x; fExp2's own error; the final rounding to float
        x = -LOG2E6 * r * r
        approx = eps_exp2() * np.exp2(x)
        rounding = U * (2 * np.log(2.0) * np.abs(x) * np.exp2(x) + v)
        return 2 * (approx + rounding)
    # Lanczos2: the arguments a, b carry two roundings (sqrt, the product with
    # pi): |d sin| <= 2 * 2^-24 * arg; product, a * b and the division: 3 more, 4 with margin
    a, b = np.pi * r, np.pi * r / 2
    e = eps_sin()
    approx = (e * (np.abs(np.sin(a)) + np.abs(np.sin(b))) + e * e) / (a * b)
    rounding = U * ((2 * a * np.abs(np.sin(b)) + 2 * b * np.abs(np.sin(a))) / (a * b) + 4 * v)
    return 2 * (approx + rounding)


def test_fixture_errors_are_those_recorded_in_the_design_notes(capsys):
    es, ee = eps_sin(), eps_exp2()
    with capsys.disabled():
        print(f"\n[film tables] eps fSin {es:.4e} (absolute), eps fExp2 {ee:.4e} (relative)")
    # DESIGN.md's test section quotes these
    assert 1.0e-3 < es < 1.2e-3 and 1.5e-4 < ee < 1.9e-4


@pytest.mark.parametrize("pw", WIDTHS)
@pytest.mark.parametrize("filt", FILTERS.values(), ids=FILTERS.keys())
def test_table_against_closed_form(filt, pw, capsys):
    table, _ = film_table(_params(filt, pw))
    want, bound = R.table64(filt), table_bound(filt)
    dev = np.abs(table.astype(F64) - want)
    with capsys.disabled():
        print(f"\n[film tables] filter {filt} pw {pw}: largest deviation {dev.max():.4e}, "
              f"largest deviation / bound {np.max(dev / np.maximum(bound, 1e-300)):.3f}")
    if filt == R.BOX:
        assert (table == 1.0).all()
    bad = np.flatnonzero(dev > bound)
    assert len(bad) == 0, [(int(i), float(table[i]), float(want[i]), float(bound[i])) for i in bad[:8]]


def test_hooks_refuse_without_env(monkeypatch):
    monkeypatch.delenv("YK_DEBUG_HOOKS", raising=False)
    assert A.lib().yk_debug_film_splat(None, None, 0, 1, 1, 0, None, None, None, 0, None) == A.YK_ERR_UNSUPPORTED
    assert b"YK_DEBUG_HOOKS" in A.lib().yk_last_error()
    assert A.lib().yk_debug_aa_flags(None, None, 1, 1, 0.1, None) == A.YK_ERR_UNSUPPORTED
    assert b"YK_DEBUG_HOOKS" in A.lib().yk_last_error()


# ------------------------------------------------- the reference's self-checks

def test_round2int_is_a_c_conversion():
    assert R.round2int([-3.7, -0.5, 0.4999, 0.5, 0.50000000002, 1.5 - 1e-12]).tolist() == [-3, 0, 0, 0, 1, 1]
    assert R.floor2int([-0.1, 0.0, 15.9984]).tolist() == [-1, 0, 15]


def test_boundary_offsets_change_an_extent():
    """either side of a boundary offset gives another Round2Int"""
    for fw in (0.501, 1.5, 1.7, 4.0):
        fw = F64(F32(fw))
        b = FC.boundary_offsets(fw).astype(F64)
        lo, hi = R.round2int(b - fw), R.round2int(b + fw - 1.0)
        # (a conversion towards zero: fw = 0.501 keeps dx - fw + 0.5 inside (-1, 1), one value)
        assert len(set(lo.tolist())) >= (2 if fw > 0.6 else 1) and len(set(hi.tolist())) >= 2, fw
        assert b.min() == 0.0 and b.max() == float(np.nextafter(F32(1), F32(0)))


@pytest.mark.parametrize("name", FC.case_names())
def test_splat32_within_bound_of_splat64(name):
    c = FC.case(name)
    f64, n, S = c.ref64
    f32 = c.ref32
    err = np.abs(f32.astype(F64) - f64)
    assert (err <= R.splat_bound(n, S)).all(), float((err / np.maximum(R.splat_bound(n, S), 1e-300)).max())
    film_in = c.inputs[2]
    assert (f32[n == 0].view(np.uint32) == film_in[n == 0].view(np.uint32)).all()
    if c.exact:
        assert (f32.astype(F64) == f64).all() and (f32[..., 4] == n).all()
    if c.flags is None:
        assert (n > 0).all() or c.nshards > 1  # every pixel takes at least its own samples
    elif not c.flags.any():
        assert (n == 0).all()


def test_cases_reach_what_they_are_for():
    # a footprint of the fw 4 case spans three or four tiles each way
    c = FC.case("lanczos_pw8_tile4")
    assert c.film.fw == 4.0 and c.film.ntx == 3 and c.film.nty == 3
    # the empty-batch pattern: batch 1 of the hand-out order has no flagged pixel, its neighbours have
    c = FC.case("adaptive_empty_batch")
    P = c.film
    tiles = P.shard_tiles(0, 1, c.order)
    per_batch = [len(P.sample_pixels(tiles[i:i + 2], c.flags)) for i in range(0, len(tiles), 2)]
    assert per_batch[1] == 0 and per_batch[0] > 0 and per_batch[2] > 0
    assert FC.case("adaptive_one_pixel").flags.sum() == 1
    # shards: the shard films' float32 sum against the whole film's bound
    for nshards in (2, 3):
        for k in ("rowmajor", "random"):
            cs = [FC.case(f"shard{s}of{nshards}_{k}") for s in range(nshards)]
            FC.check_shard_sum([c.ref32 for c in cs], cs)


def test_flag_reference_on_the_planted_films():
    for film, thr, want in FC.planted_flag_films():
        got, _ = R.next_pass_flags64(film, thr)
        assert (got == want).all(), (film[..., 1].tolist(), thr, got.tolist(), want.tolist())


@pytest.mark.parametrize("name", FC.RANDOM_FLAG_FILMS)
def test_flag_films_skip_at_most_one_percent(name):
    film, thr = FC.random_flag_film(name)
    flags, pairs = R.next_pass_flags64(film, thr)
    skip = pairs["margin"] < FC.flag_margin(pairs, thr)
    assert skip.mean() <= 0.01
    assert 0.1 < flags.mean() < 0.9  # the threshold separates: neither nothing nor everything flagged
    assert (film[..., 4] == 0).any()
