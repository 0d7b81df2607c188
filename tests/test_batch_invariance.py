"""DESIGN §2's promise on the GPU: the film and the counters do not depend on
how render_pass cuts a frame into batches, how many pipes run them, or which
shard owns the tiles.

One frame shape with partial right and bottom tiles (crop (5, 3, 90, 75) of
a 96 x 96 scene at tile_size 32: 3 x 3 tiles, the last column 26 wide, the
last row 11 high). Per case: a baseline render with the environment unset,
bit-exact against the CPU oracle (film sums and ray counts); then, on the
same handle and without a re-upload, so that every grow-only buffer of the
pipes is reused by later and shorter batches, one render per (YK_PIPES,
batch size) pair, each bit-equal to the baseline in the film and in every
yk_stats counter. yk_debug_last_plan shows that the environment was obeyed:
the intended number of batches, and more than one batch on a pipe.

Batch sizes are given in tiles of the pass the plan is read from (1, 2 and
"4 and one sample": YK_BATCH_SAMPLES = 8192, 16384, 32769 at 8 spp), so the
cases with other sample counts (adaptive passes, photon mapping at 2 spp)
get the same one-, two- and four-tile batches.

Budget against allocation: what a pipe's batch buffers hold after a render
on a fresh handle is at most maxc * bytes_per_sample of the plan.
"""
import ctypes as C

import numpy as np
import pytest

from core_amd import _abi as A
from core_amd.scene import probe_scene
from oracle.oracle import Oracle
from tests.scenes import many_light_slots, specular, transparent_panes
from tests.test_photon_gpu import CASES as PHOTON_CASES, pm_params
from tests.test_tile_order import _with_order, order_of

pytestmark = pytest.mark.gpu

RES, CROP, TILE = 96, (5, 3, 90, 75), 32
NTILES = 9
# (YK_PIPES, batch size in tiles; None: unset; 4.x: four tiles and one sample)
VARIANTS = [(1, 1), (1, 2), (2, 1), (3, 2), (2, 4.5), (4, 1), (1, None)]
NBATCH_OF_9 = {1: 9, 2: 5, 4.5: 3}  # batches of a 9-tile frame
STAT_FIELDS = ("closest_rays", "shadow_rays", "closest_nodes", "closest_tris", "shadow_nodes", "shadow_tris",
               "camera_samples")
NODE_BYTES, NODE_STORE = 116, 12 << 30  # specular node store: bytes per node, bytes per batch


def _frame(p, **over):
    q = A.yk_render_params.from_buffer_copy(p)
    q.xstart, q.ystart, q.width, q.height = CROP
    q.tile_size = TILE
    q.aa_samples = 8
    for k, v in over.items():
        setattr(q, k, v)
    return q


def _cornell_pt():
    s, p = probe_scene("cornell_pt", RES, RES)
    return s, _frame(p, bounces=4, filter=A.YK_FILTER_BOX), {}


def _cornell_unmerged():
    s, p = probe_scene("cornell_pt", RES, RES)
    return s, _frame(p, bounces=4, filter=A.YK_FILTER_BOX, path_samples=2), {"env": {"YK_MERGE": "0"}}


def _many_slots():
    s, p = many_light_slots(RES, RES, "cornell_pt")
    return s, _frame(p, filter=A.YK_FILTER_GAUSS, aa_pixelwidth=3.0), {"split": 1}


def _cornell_dl():
    s, p = probe_scene("cornell_dl", RES, RES)
    return s, _frame(p, filter=A.YK_FILTER_MITCHELL), {}


def _adaptive():
    s, p = probe_scene("cornell_pt", RES, RES)
    return s, _frame(p, aa_samples=4, aa_passes=3, aa_inc_samples=2, aa_threshold=0.05), {}


def _spec():
    s, p = specular(RES, RES, "cornell_pt", raydepth=3, caustic=True)
    return s, _frame(p), {}


def _photon_fg():
    name, kw = PHOTON_CASES[0]  # cornell, final gathering
    assert name == "cornell" and kw.get("final_gather", 1)
    s, p = probe_scene("cornell_pt", RES, RES)
    q = pm_params(_frame(p), **kw)  # 2 spp, 20000 photons, 4 gather paths
    return s, q, {"photon": True}


def _panes():
    s, p = transparent_panes(RES, RES, "cornell_pt")
    return s, _frame(p, transp_shadows=1, shadow_depth=3), {}


def _bumpy():
    s, p = probe_scene("bumpy", RES, RES, 120, 61)
    return s, _frame(p), {"small": 0}


def _random_shard():
    s, p = probe_scene("cornell_dl", RES, RES)
    q = _frame(p)
    keep = _with_order(q, order_of(NTILES, 5))
    return s, q, {"shard": (1, 2), "keep": keep}


BUILDERS = {"cornell_pt": _cornell_pt, "cornell_pt_unmerged_2sub": _cornell_unmerged, "many_slots_gauss": _many_slots,
            "cornell_dl_mitchell": _cornell_dl, "cornell_pt_adaptive": _adaptive, "spec_rd3_caustic": _spec,
            "photon_final_gather": _photon_fg, "transparent_panes_sd3": _panes, "bumpy_hbm": _bumpy,
            "cornell_dl_random_shard1of2": _random_shard}


def _is_spec(s):
    return any(m.bsdf_flags & 0x41 for m in s.material_states())  # BSDF_SPECULAR | BSDF_FILTER: recursion pipeline


def _last_plan(dev):
    lp = A.yk_last_plan()
    A.check(A.lib().yk_debug_last_plan(dev._p, C.byref(lp)))
    return lp


def _render(dev, q, shard):
    film = dev.new_film(q)
    st = dev.render_shard(q, film, *shard)
    return film.cpu().numpy(), st


def _set_variant(monkeypatch, pipes, tiles, tile_samples):
    monkeypatch.setenv("YK_PIPES", str(pipes))
    if tiles is None:
        monkeypatch.delenv("YK_BATCH_SAMPLES", raising=False)
        return None
    target = int(tiles) * tile_samples + (1 if tiles != int(tiles) else 0)
    monkeypatch.setenv("YK_BATCH_SAMPLES", str(target))
    return target


def _expected_batches(owned, pipes, target, tile_samples, spec_levels):
    """batches, pipes and batches on the busiest pipe that (pipes, target)
    ask for on `owned` tiles; no budget binds at these sizes"""
    cap = target if target else 32 << 20
    if spec_levels is not None:  # one pipe; the node store caps the batch
        cap = min(cap, NODE_STORE // (NODE_BYTES * (2 ** (spec_levels + 1) - 1)))
        tpb = min(owned, max(1, cap // tile_samples))
    else:  # at least one batch per pipe when the frame has the tiles
        tpb = max(1, min(cap // tile_samples, -(-owned // pipes)))
    nbatch = -(-owned // tpb)
    npipes = 1 if spec_levels is not None else min(pipes, nbatch)
    return nbatch, npipes, -(-nbatch // npipes)


def _prepare(dev, monkeypatch, name):
    s, q, x = BUILDERS[name]()
    monkeypatch.setenv("YK_DEBUG_HOOKS", "1")
    for k in ("YK_PIPES", "YK_BATCH_SAMPLES", "YK_MERGE", "YK_SPLIT", "YK_SMALL", "YK_BATCH_GB"):
        monkeypatch.delenv(k, raising=False)
    for k, v in x.get("env", {}).items():
        monkeypatch.setenv(k, v)
    orc = Oracle(s)
    dev.upload(s)
    if x.get("photon"):
        orc.photon_build(q)
        dev.photon_build(q)
    if "split" in x:
        v = C.c_int32(-1)
        A.check(A.lib().yk_debug_shadow_form(dev._p, C.byref(q), C.byref(v)))
        assert v.value == x["split"]
    if "small" in x:
        nb = C.c_int64(-1)
        A.check(A.lib().yk_debug_small_scene(dev._p, C.byref(nb)))
        assert nb.value == x["small"]
    return s, q, x, orc


@pytest.mark.parametrize("name", list(BUILDERS))
def test_film_and_counters_do_not_depend_on_batches_or_pipes(gpu_device, monkeypatch, name):
    s, q, x, orc = _prepare(gpu_device, monkeypatch, name)
    shard = x.get("shard", (0, 1))
    owned = len(range(shard[0], NTILES, shard[1]))
    spec_levels = min(q.raydepth, 19) if _is_spec(s) else None
    # baseline, environment unset: bit-exact against the oracle
    base, st0 = _render(gpu_device, q, shard)
    if shard == (0, 1):
        _, sums_o, cnt = orc.render(q)
    else:
        sums_o, cnt = orc.render_shard(q, *shard)
    assert st0.closest_rays == cnt["closest"] and st0.shadow_rays == cnt["shadow"], (st0.closest_rays, cnt)
    assert (base.view(np.uint32) == sums_o.view(np.uint32)).all(), "baseline film differs from the oracle"
    if "closest_nodes" in cnt:
        assert st0.closest_nodes == cnt["closest_nodes"] and st0.shadow_tris == cnt["shadow_tris"]
    assert st0.camera_samples > 0
    # the pass the last plan belongs to
    spp_last = (q.aa_inc_samples or q.aa_samples) if q.aa_passes > 1 else q.aa_samples
    tile_samples = TILE * TILE * spp_last
    for i, (pipes, tiles) in enumerate(VARIANTS):
        target = _set_variant(monkeypatch, pipes, tiles, tile_samples)
        film, st = _render(gpu_device, q, shard)
        tag = f"{name} YK_PIPES={pipes} YK_BATCH_SAMPLES={target}"
        lp = _last_plan(gpu_device)
        nbatch, npipes, on_pipe = _expected_batches(owned, pipes, target, tile_samples, spec_levels)
        got = (lp.plan.nbatch, lp.plan.npipes, lp.max_batches_on_pipe)
        print(f"{tag}: tiles_per_batch {lp.plan.tiles_per_batch} nbatch/npipes/on one pipe {got}")
        assert got == (nbatch, npipes, on_pipe), tag
        if owned == NTILES and tiles is not None:
            assert lp.plan.nbatch == NBATCH_OF_9[tiles], tag
            if i < 5:
                assert lp.max_batches_on_pipe >= 2, tag
        diff = film.view(np.uint32) != base.view(np.uint32)
        assert not diff.any(), f"{tag}: {diff.any(axis=2).sum()} pixels differ from the baseline"
        for f in STAT_FIELDS:
            assert getattr(st, f) == getattr(st0, f), (tag, f, getattr(st, f), getattr(st0, f))
    if owned != NTILES:  # the shard's 4 tiles still give a pipe a second batch in the first three pairs
        assert [_expected_batches(owned, p, int(t) * tile_samples, tile_samples, None)[2] >= 2
                for p, t in VARIANTS[:3]] == [True] * 3


@pytest.mark.parametrize("name", ["many_slots_gauss", "photon_final_gather", "transparent_panes_sd3"])
def test_pipe_buffers_stay_within_the_plan_budget(monkeypatch, name):
    """Buffers are grow-only, so a fresh handle per case. batch_bytes is what
    the plan sizes (Pipe::bind and the final-gather buffers); the traversal
    stack overflow area, the counters and the per-launch words follow the
    launch grid, not the batch, and are reported apart (pipe_bytes)."""
    import torch  # noqa: F401
    from core_amd.device import Device
    dev = Device(0)
    try:
        s, q, x, _ = _prepare(dev, monkeypatch, name)
        _set_variant(monkeypatch, 4, None, 0)
        _render(dev, q, x.get("shard", (0, 1)))
        lp = _last_plan(dev)
        budget = lp.plan.maxc * lp.plan.bytes_per_sample
        print(f"{name}: maxc {lp.plan.maxc} x {lp.plan.bytes_per_sample} B = {budget}; batch buffers "
              f"{lp.batch_bytes}, all buffers of the pipe {lp.pipe_bytes}")
        assert lp.plan.status == A.YK_OK and lp.plan.maxc > 0
        assert 0 < lp.batch_bytes <= budget
        assert lp.pipe_bytes >= lp.batch_bytes
    finally:
        dev.close()
