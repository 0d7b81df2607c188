"""The shape of a batch's launch sequence, through yk_stats.closest_launches
and yk_stats.shadow_launches: how many closest-hit and any-hit traversal
launches one batch enqueues, per integrator form.

Cornell box, 64 x 64 at tile_size 32 and 2 spp, YK_BATCH_SAMPLES set to one
tile's samples: nb = 4 one-tile batches (checked through yk_debug_last_plan).
Per batch:

  path tracing, one sub-path, merged     1 + bounces closest, 1 any-hit
  path tracing, one sub-path, YK_MERGE=0 1 + bounces closest, 1 + bounces any-hit
  path tracing, n sub-paths (unmerged)   1 + n * bounces of each
  direct lighting (AO, transparent
  shadows or neither)                    1 closest, 1 any-hit
  photon mapping, final gathering with
  s paths of b bounces                   1 + s * (b + 1) closest, 1 + s * b any-hit

The merged launch traces the same shadow rays as the per-bounce launches.
Specular scenes are left out: their generation count depends on the data.
"""
import ctypes as C

import pytest

from core_amd import _abi as A
from core_amd.scene import probe_scene
from tests.dl_common import with_ao
from tests.test_photon_gpu import pm_params

pytestmark = pytest.mark.gpu

RES, TILE, SPP, NB = 64, 32, 2, 4


def _frame(name, **over):
    s, p = probe_scene(name, RES, RES)
    q = p.copy()
    q.tile_size = TILE
    q.aa_samples = SPP
    for k, v in over.items():
        setattr(q, k, v)
    return s, q


def _render(dev, monkeypatch, s, q, merge=None, photon=False):
    monkeypatch.setenv("YK_DEBUG_HOOKS", "1")  # yk_debug_last_plan
    monkeypatch.setenv("YK_BATCH_SAMPLES", str(TILE * TILE * SPP))
    if merge is None:
        monkeypatch.delenv("YK_MERGE", raising=False)
    else:
        monkeypatch.setenv("YK_MERGE", str(merge))
    dev.upload(s)
    if photon:
        dev.photon_build(q)
    st = dev.render_shard(q, dev.new_film(q))
    lp = A.yk_last_plan()
    A.check(A.lib().yk_debug_last_plan(dev._p, C.byref(lp)))
    assert lp.plan.nbatch == NB, lp.plan.nbatch
    print(f"closest_launches {st.closest_launches} shadow_launches {st.shadow_launches} "
          f"closest_rays {st.closest_rays} shadow_rays {st.shadow_rays}")
    return st


def test_path_merged_and_unmerged(gpu_device, monkeypatch):
    s, q = _frame("cornell_pt", bounces=3, path_samples=1)
    m = _render(gpu_device, monkeypatch, s, q, merge=1)
    u = _render(gpu_device, monkeypatch, s, q, merge=0)
    assert (m.closest_launches, m.shadow_launches) == (NB * (1 + 3), NB * 1)
    assert (u.closest_launches, u.shadow_launches) == (NB * (1 + 3), NB * (1 + 3))
    assert m.shadow_rays == u.shadow_rays and m.closest_rays == u.closest_rays


def test_path_two_sub_paths(gpu_device, monkeypatch):
    s, q = _frame("cornell_pt", bounces=3, path_samples=2)
    st = _render(gpu_device, monkeypatch, s, q)  # never merged
    assert (st.closest_launches, st.shadow_launches) == (NB * (1 + 2 * 3), NB * (1 + 2 * 3))


@pytest.mark.parametrize("ts", [0, 1])
def test_direct_lighting(gpu_device, monkeypatch, ts):
    s, q = _frame("cornell_dl", transp_shadows=ts, shadow_depth=3)
    st = _render(gpu_device, monkeypatch, s, q)
    assert (st.closest_launches, st.shadow_launches) == (NB, NB)


def test_direct_lighting_ao(gpu_device, monkeypatch):
    s, q = _frame("cornell_dl")
    st = _render(gpu_device, monkeypatch, s, with_ao(q, 3, 1.0))
    assert (st.closest_launches, st.shadow_launches) == (NB, NB)


@pytest.mark.parametrize("fg", [(2, 1), (3, 2)], ids=lambda v: f"s{v[0]}b{v[1]}")
def test_photon_final_gather(gpu_device, monkeypatch, fg):
    fs, fb = fg
    s, q = _frame("cornell_pt")
    q = pm_params(q, spp=SPP, photons=20000, fg_samples=fs, fg_bounces=fb)
    st = _render(gpu_device, monkeypatch, s, q, photon=True)
    assert (st.closest_launches, st.shadow_launches) == (NB * (1 + fs * (fb + 1)), NB * (1 + fs * fb))
