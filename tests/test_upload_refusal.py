"""yk_device_upload refuses before it touches the handle (check_upload,
core_amd/csrc/yk_upload_host.inc): a refused upload leaves the resident scene
as usable as it was, and the next valid upload gives what a fresh handle gives.

The 36-triangle Cornell box at 16 x 16, one sample per pixel, path tracing
with one bounce, on handles opened with YK_PIPES=1. The refusal is the summed
shadow-slot limit: two sphere lights of 4096 and 4097 samples (a sphere light
takes `samples` slots) are each within the 8192 slots a shading point may own
and exceed them together, whatever else the scene holds.
"""
import numpy as np
import pytest

from core_amd import _abi as A
from core_amd.scene import Scene

gpu = pytest.mark.gpu


def _box(more=None):
    s = Scene()
    p = s.generate("cornell_pt", 16, 16)
    if more:
        more(s)
    s.build()
    q = A.yk_render_params.from_buffer_copy(p)
    q.aa_samples = 1
    q.integrator = A.YK_INTEGRATOR_PATH
    q.bounces = 1
    return s, q


def _render(dev, q):
    film = dev.new_film(q)
    st = dev.render_shard(q, film)
    return film.cpu().numpy().view(np.uint32), (st.closest_rays, st.shadow_rays)


@gpu
def test_refused_upload_keeps_the_scene_and_the_next_upload_is_clean(monkeypatch):
    import torch  # noqa: F401  (before libyk: one HIP runtime)
    from core_amd.device import Device
    monkeypatch.setenv("YK_PIPES", "1")
    dev, other, fresh = Device(0), Device(0), None
    try:
        # 1. the box, rendered
        box, q = _box()
        dev.upload(box)
        film0, rays0 = _render(dev, q)
        assert rays0[0] >= 16 * 16 and rays0[1] > 0 and film0.any()

        # 2. two sampled lights, each allowed, together too many
        def two_spheres(s):
            s.add_sphere_light((0.3, 1.0, 0.0), 0.1, samples=4096)
            s.add_sphere_light((-0.3, 1.0, 0.0), 0.1, samples=4097)

        bad, _ = _box(two_spheres)
        with pytest.raises(A.YkError) as e:
            dev.upload(bad)
        assert e.value.code == A.YK_ERR_UNSUPPORTED
        for n in (4096, 4097):  # each of the two alone is accepted (on another handle: dev gets no upload)
            alone, _ = _box(lambda s: s.add_sphere_light((0.3, 1.0, 0.0), 0.1, samples=n))
            other.upload(alone)

        # 3. no upload in between: the same film and the same rays
        film1, rays1 = _render(dev, q)
        assert rays1 == rays0
        assert (film1 == film0).all()

        # 4. the box with one more point light: as on a handle that never held anything else
        third, q3 = _box(lambda s: s.add_point_light((0.2, 1.2, -0.1), (1.0, 0.9, 0.8), 3.0))
        dev.upload(third)
        film2, rays2 = _render(dev, q3)
        fresh = Device(0)
        fresh.upload(third)
        film3, rays3 = _render(fresh, q3)
        assert rays2 == rays3
        assert (film2 == film3).all()
        assert (film2 != film0).any()  # the third scene is another scene
    finally:
        for d in (dev, other, fresh):
            if d is not None:
                d.close()
