"""The batch planner (plan_batches in core_amd/csrc/yk_pipe_host.inc, through
yk_debug_batch_plan) on the host: no GPU.

The planner sizes every per-batch buffer and with them every 32-bit index
the kernels form. The bounds asserted here are read off the kernels' types,
in Python integers, not off the planner:

* trace_body keeps the ray of a lane in a signed `int` (`r = (int)idx[q]`,
  `r = (int)((e >> kshift) * kstride + oi)`) with -1 as the "no ray"
  sentinel, and reads a launch's ray count through `(int)rc.get()`: every
  shadow-slot index k * kstride + r * maxc + c and every queue count (at most
  maxc * K * regions, the merged launch's sum over its regions) must be
  <= 2^31 - 1.
* camera-sample indices and the tile bases (`base_all`, `int`) are < 2^31.
* a split queue entry packs k above the origin index in 32 bits
  (`k << kshift | r * maxc + c`, RaySrc: `omask = (1u << kshift) - 1`,
  `unsigned kstride`).

Budget: the planner promises npipes * maxc * bytes_per_sample <= budget,
except where one tile is already more than that, or where the 1M-sample
floor of the budget cap binds; the share of such plans in the grid is
bounded (a quarter), so the promise cannot erode unnoticed.
"""
import ctypes as C
import itertools

import pytest

from core_amd import _abi as A

INT_MAX = 2 ** 31 - 1
GB = 1 << 30
FLOOR = 1 << 20

KS = (1, 2, 8, 94, 512)
BOUNCES = (0, 1, 3, 8, 16)
TILES = (16, 32, 64)
SPPS = (1, 16, 256, 4096)
OWNED = (1, 9, 2040)
PIPES = (1, 4)
BUDGETS = (64 * GB, 192 * GB, 240 * GB)
TARGETS = (0, 8192, 3_000_000)  # unset, one-tile batches of the invariance tests' frame, an odd explicit size


@pytest.fixture(autouse=True)
def _hooks(monkeypatch):
    monkeypatch.setenv("YK_DEBUG_HOOKS", "1")


def plan(K, bounces, merged, split, tile, spp, owned, pipes, budget, target=0, ts=0, spec=0, fg=0, levels=0):
    i = A.yk_batch_plan_in(slots=K, bounces=bounces, merged=merged, split=split, transp_shadows=ts, spec=spec,
                           final_gather=fg, spec_levels=levels, tile=tile, spp=spp, pipes=pipes, owned_tiles=owned,
                           target_samples=target, budget_bytes=budget)
    o = A.yk_batch_plan()
    rc = A.lib().yk_debug_batch_plan(C.byref(i), C.byref(o))
    assert rc == o.status
    return o


def check_indices(o, K, bounces, merged, split, tile, spp, owned, pipes):
    """the kernels' index types hold every index the plan implies"""
    regions = o.regions
    assert regions >= (bounces + 1 if merged else 1)  # k_resolve_merged: one region per depth 0..bounces
    assert o.tiles_per_batch >= 1
    assert o.maxc == o.tiles_per_batch * tile * tile * spp  # a batch holds whole tiles
    assert o.kstride == regions * o.maxc
    assert o.maxc < 2 ** 31  # camera-sample index, base_all entries (<= maxc)
    top_slot = (K - 1) * o.kstride + (regions - 1) * o.maxc + (o.maxc - 1)
    assert top_slot <= INT_MAX, f"slot index {top_slot} does not fit the kernel's int"
    assert o.maxc * K * regions <= INT_MAX, "merged queue count does not fit (int)rc.get()"
    if split:
        assert 0 <= o.kshift <= 31
        assert o.kstride <= 2 ** o.kshift
        assert (((K - 1) << o.kshift) | (regions * o.maxc - 1)) < 2 ** 32
    assert o.nbatch * o.tiles_per_batch >= owned
    assert (o.nbatch - 1) * o.tiles_per_batch < owned  # no empty batch
    assert 1 <= o.npipes <= min(pipes, o.nbatch)


def one_tile_fits(K, regions, tile, spp):
    """one tile alone stays inside the kernel's int (the least a plan needs)"""
    return K * regions * tile * tile * spp <= INT_MAX


def grid():
    return itertools.product(KS, BOUNCES, (0, 1), (0, 1), TILES, SPPS, OWNED, PIPES, BUDGETS, TARGETS)


def test_grid_indices_fit_and_budget_holds():
    n = refused = over = over_floor = over_tile = 0
    for K, bounces, merged, split, tile, spp, owned, pipes, budget, target in grid():
        n += 1
        o = plan(K, bounces, merged, split, tile, spp, owned, pipes, budget, target)
        regions = bounces + 1 if merged else 1
        case = (K, bounces, merged, split, tile, spp, owned, pipes, budget // GB, target)
        if o.status != A.YK_OK:
            # refused, never wrapped: and only where one tile really is too much
            assert o.status == A.YK_ERR_UNSUPPORTED, case
            assert not one_tile_fits(K, regions, tile, spp), case
            refused += 1
            continue
        assert one_tile_fits(K, regions, tile, spp), case
        try:
            check_indices(o, K, bounces, merged, split, tile, spp, owned, pipes)
        except AssertionError as e:
            raise AssertionError(f"{case}: {e}") from None
        tile_samples = tile * tile * spp
        # the sample target is honoured down to one tile
        assert o.maxc <= max(target or (32 << 20), tile_samples), case
        if o.npipes * o.maxc * o.bytes_per_sample <= budget:
            continue
        # over budget: allowed only at the one-tile minimum, or where the 1M
        # floor of the budget cap binds (then the floor is the cap)
        over += 1
        if o.tiles_per_batch == 1:
            over_tile += 1
        else:
            assert budget // pipes // o.bytes_per_sample < FLOOR, case
            assert o.maxc <= FLOOR, case
            over_floor += 1
    assert n == 64800 and refused < n // 4
    share = over / (n - refused)
    print(f"planner grid: {n} plans, {refused} refused, {over} over budget ({over_tile} at one tile, "
          f"{over_floor} at the 1M floor): share {share:.4f}")
    assert share <= 0.25, share


def test_advice_case_stays_inside_int():
    """94 slots, 8 bounces merged, one pipe, tile 32, 256 spp,
    2040 tiles at 192 GB. The budget alone allows 18 tiles = 4,718,592 samples
    per batch, whose 94 * 9 * maxc = 3.99e9 slots pass 2^31."""
    for split in (0, 1):
        o = plan(94, 8, 1, split, 32, 256, 2040, 1, 192 * GB)
        assert o.status == A.YK_OK
        print(f"ADVICE case split={split}: tiles_per_batch {o.tiles_per_batch} maxc {o.maxc} "
              f"slots {o.maxc * 94 * o.regions}")
        check_indices(o, 94, 8, 1, split, 32, 256, 2040, 1)
        assert o.tiles_per_batch >= 2  # shrunk, not refused: 9 tiles still fit


def test_unset_target_is_32m_and_explicit_target_is_not_floored():
    for K, pipes in itertools.product(KS, PIPES):
        a = plan(K, 4, 1, 0, 32, 256, 2040, pipes, 192 * GB, 0)
        b = plan(K, 4, 1, 0, 32, 256, 2040, pipes, 192 * GB, 32 << 20)
        assert bytes(a) == bytes(b)
    # 8 spp at tile 32: 8192 samples per tile; explicit targets below the 1M floor are taken as they are
    for target, tiles in ((8192, 1), (16384, 2), (32769, 4), (8191, 1)):
        o = plan(2, 4, 1, 0, 32, 8, 9, 1, 192 * GB, target)
        assert (o.tiles_per_batch, o.nbatch) == (tiles, -(-9 // tiles)), target
    # unset: one batch per pipe when the frame has the tiles for it
    o = plan(2, 4, 1, 0, 32, 8, 9, 4, 192 * GB)
    assert (o.tiles_per_batch, o.nbatch, o.npipes) == (3, 3, 3)
    o = plan(2, 4, 1, 0, 32, 8, 9, 1, 192 * GB)
    assert (o.tiles_per_batch, o.nbatch, o.npipes) == (9, 1, 1)


def test_spec_plans_one_pipe_and_bounds_the_node_store():
    """specular recursion: one pipe, and maxc * (2^(L+1) - 1) nodes of 116 B
    within the 12 GB the node store is given (one tile at the least)"""
    for levels, tile, spp, pipes in itertools.product((0, 1, 3, 8, 19), TILES, (1, 16, 256), PIPES):
        o = plan(2, 4, 0, 0, tile, spp, 2040, pipes, 64 * GB, spec=1, levels=levels)
        nodes_per_sample = 2 ** (levels + 1) - 1
        tile_samples = tile * tile * spp
        if o.status != A.YK_OK:
            assert o.status == A.YK_ERR_UNSUPPORTED
            assert tile_samples * nodes_per_sample * 116 > 12 * GB  # refused only where one tile is too much
            continue
        assert o.npipes == 1
        check_indices(o, 2, 4, 0, 0, tile, spp, 2040, pipes)
        assert o.maxc * nodes_per_sample * 116 <= max(12 * GB, tile_samples * nodes_per_sample * 116)
        assert tile_samples * nodes_per_sample * 116 <= 48 * GB


def test_transparent_shadows_are_budgeted():
    a = plan(8, 4, 0, 0, 32, 16, 2040, 4, 64 * GB)
    b = plan(8, 4, 0, 0, 32, 16, 2040, 4, 64 * GB, ts=1)
    assert b.bytes_per_sample == a.bytes_per_sample + 28 * 8  # s_filt (12 B) + sl_aux (16 B) per slot


def test_hook_needs_the_debug_environment(monkeypatch):
    monkeypatch.delenv("YK_DEBUG_HOOKS", raising=False)
    i, o = A.yk_batch_plan_in(slots=1, tile=32, spp=1, pipes=1, owned_tiles=1, budget_bytes=GB), A.yk_batch_plan()
    assert A.lib().yk_debug_batch_plan(C.byref(i), C.byref(o)) == A.YK_ERR_UNSUPPORTED
    assert b"YK_DEBUG_HOOKS" in A.lib().yk_last_error()
    assert A.lib().yk_debug_last_plan(None, None) == A.YK_ERR_UNSUPPORTED
