"""Group hand-out of the camera-ray launch (trace_body GROUP: k_trace_camera,
its _big and _small forms).

The hand-out decides only which ray sits in which lane, and when; a ray's own
traversal is the closest-hit kernels'. So every frame must come out as before:
film sums bit for bit and all six work counters equal to the oracle's, with
the group kernels (the default) and with YK_CAMERA_GROUPS=0, which keeps the
camera rays on the bounce rays' kernels -- and the two runs equal to each
other in every yk_stats counter.

The bumpy frames are the 96 x 64 scene less its last column and row (95 x 63
pixels): 96 * 64 * spp is a multiple of 64 at any spp, and the case is there
for a ragged last group (41,895 and 418,950 camera rays; the 31-pixel edge
tiles make every batch ragged too) with groups that straddle pixels (7 and 70
samples per pixel against groups of 64).
"""
import ctypes as C

import numpy as np
import pytest

from core_amd import _abi as A
from core_amd.scene import probe_scene
from oracle.oracle import Oracle
from tests.test_big_leaf import big_leaf_scene

pytestmark = pytest.mark.gpu

COUNTERS = ("closest_rays", "shadow_rays", "closest_nodes", "closest_tris", "shadow_nodes", "shadow_tris")
ENV_KEYS = ("YK_CAMERA_GROUPS", "YK_SMALL", "YK_PIPES", "YK_BATCH_SAMPLES", "YK_MERGE", "YK_SPLIT", "YK_BATCH_GB",
            "YK_REFILL")
TILE = 32
BUMPY = ("bumpy", 96, 64, 40, 26)  # 2 * 40 * 25 + 2 = 2002 triangles
BUMPY_CROP = (0, 0, 95, 63)
ADAPTIVE = {"aa_samples": 4, "aa_passes": 2, "aa_inc_samples": 3, "aa_threshold": 0.05}

# name: (scene, crop, parameter overrides, environment, small-scene kernels expected or None)
CASES = {
    "bumpy_7spp": (BUMPY, BUMPY_CROP, {"aa_samples": 7}, {}, None),
    "bumpy_70spp": (BUMPY, BUMPY_CROP, {"aa_samples": 70}, {}, None),
    "cornell_small": (("cornell_pt", 64, 48), (0, 0, 64, 48), {}, {}, True),
    "cornell_hbm": (("cornell_pt", 64, 48), (0, 0, 64, 48), {}, {"YK_SMALL": "0"}, False),
    "under_64_rays": (("cornell_pt", 64, 48), (30, 20, 5, 4), {"aa_samples": 3}, {}, None),  # 60 camera rays
    "under_64_rays_hbm": (("cornell_pt", 64, 48), (30, 20, 5, 4), {"aa_samples": 3}, {"YK_SMALL": "0"}, False),
    "adaptive_pass": (("cornell_pt", 64, 48), (0, 0, 64, 48), ADAPTIVE, {}, None),
    "adaptive_pass_hbm": (("cornell_pt", 64, 48), (0, 0, 64, 48), ADAPTIVE, {"YK_SMALL": "0"}, False),
    "big_leaf": (("big_leaf", 24, 24), (0, 0, 24, 24), {"aa_samples": 1, "bounces": 2}, {}, False),
    "bumpy_one_pipe": (BUMPY, BUMPY_CROP, {"aa_samples": 7}, {"YK_PIPES": "1"}, None),
    "bumpy_batch_of_one_tile": (BUMPY, BUMPY_CROP, {"aa_samples": 7}, {"YK_BATCH_SAMPLES": str(TILE * TILE * 7)},
                                None),
}

_SCENES = {}
_ORACLE = {}


def _scene(key):
    if key not in _SCENES:
        s, p = big_leaf_scene(key[1]) if key[0] == "big_leaf" else probe_scene(*key)
        _SCENES[key] = (s, p, Oracle(s))
    return _SCENES[key]


def _params(p, crop, over):
    q = A.yk_render_params.from_buffer_copy(p)
    q.xstart, q.ystart, q.width, q.height = crop
    q.tile_size = TILE
    for k, v in over.items():
        setattr(q, k, v)
    return q


def _oracle(key, crop, over):
    """One oracle frame per (scene, crop, parameters), shared by the cases that differ only in their environment."""
    k = (key, crop, tuple(sorted(over.items())))
    if k not in _ORACLE:
        s, p, orc = _scene(key)
        _, sums, cnt = orc.render(_params(p, crop, over))
        sums.setflags(write=False)
        _ORACLE[k] = (sums, cnt)
    return _ORACLE[k]


@pytest.mark.parametrize("name", list(CASES))
def test_camera_group_handout(gpu_device, monkeypatch, name):
    key, crop, over, env, small = CASES[name]
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("YK_DEBUG_HOOKS", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s, p, _ = _scene(key)
    q = _params(p, crop, over)
    sums_o, cnt = _oracle(key, crop, over)
    gpu_device.upload(s)
    if small is not None:
        nb = C.c_int64(-1)
        A.check(A.lib().yk_debug_small_scene(gpu_device._p, C.byref(nb)))
        assert (nb.value > 0) == small, nb.value
    runs = {}
    for groups in ("1", "0"):
        monkeypatch.setenv("YK_CAMERA_GROUPS", groups)
        film = gpu_device.new_film(q)
        st = gpu_device.render_shard(q, film)
        runs[groups] = (film.cpu().numpy(), {f: int(getattr(st, f)) for f in COUNTERS + ("camera_samples",)})
    want = {"closest_rays": cnt["closest"], "shadow_rays": cnt["shadow"], "closest_nodes": cnt["closest_nodes"],
            "closest_tris": cnt["closest_tris"], "shadow_nodes": cnt["shadow_nodes"],
            "shadow_tris": cnt["shadow_tris"]}
    for groups, (sums_g, got) in runs.items():
        print(f"{name} YK_CAMERA_GROUPS={groups}: {got}; oracle {want}")
        assert {f: got[f] for f in COUNTERS} == want, f"YK_CAMERA_GROUPS={groups}"
        diff = sums_g.view(np.uint32) != sums_o.view(np.uint32)
        assert not diff.any(), f"YK_CAMERA_GROUPS={groups}: {diff.sum()} film floats differ"
    assert runs["1"][1] == runs["0"][1]
    assert (runs["1"][0].view(np.uint32) == runs["0"][0].view(np.uint32)).all()
    assert want["closest_rays"] > 0 and runs["1"][1]["camera_samples"] > 0
