"""Throughput of a Cornell-like room with glossy walls, path traced:
  python tools/glossy_bench.py [--res 1024] [--spp 64] [--steps 3] [--warmup 1] [--coated]
The room is closed (floor, ceiling, three walls, the camera looks in through
the open fourth side) with one box and one area light under the ceiling. It is
rendered twice: every surface glossy (isotropic and anisotropic lobes over a
diffuse base, one with Oren-Nayar), then every surface shinydiffuse with the
same diffuse part, so the glossy instantiations' cost stands beside the
diffuse-only kernels' on the same geometry. One JSON line per form: Mrays/s
(closest + shadow rays over wall time, film resolve included, as bench.py
counts them). --coated renders a third form first: the same room with every
glossy surface coated (coated_glossy, IOR 1.4, white mirror_color) and
raydepth 2, so the coat's recursion rays are in the count. Ungated: a record,
not a check."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from core_amd import _abi as A  # noqa: E402
from core_amd.device import Device  # noqa: E402
from core_amd.scene import Scene  # noqa: E402

F = np.float32
QUAD = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
BOX_FACES = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1],
                      [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.int32)
# floor, ceiling, back wall, left wall, right wall, box: (diffuse colour, diffuse_reflect)
DIFFUSE = [((0.8, 0.8, 0.7), 0.9), ((0.8, 0.8, 0.8), 0.8), ((0.7, 0.7, 0.8), 0.8), ((0.8, 0.1, 0.1), 1.0),
           ((0.1, 0.8, 0.1), 0.7), ((0.3, 0.5, 0.9), 0.6)]
LOBES = [dict(exponent=500.0), dict(exponent=50.0), dict(anisotropic=True, exp_u=300.0, exp_v=8.0),
         dict(exponent=20.0, diffuse_brdf="Oren-Nayar", sigma=0.4), dict(anisotropic=True, exp_u=10.0, exp_v=400.0),
         dict(exponent=50.0)]


def room(res, form):
    s = Scene()
    glossy = form == "glossy"
    if form == "coated":
        m = [s.add_material(type_=A.YK_MAT_COATED_GLOSSY, color=(0.9, 0.85, 0.8), glossy_reflect=0.3, diffuse_color=c,
                            diffuse_reflect=d, ior=1.4, mirror_color=(1, 1, 1), **lobe)
             for (c, d), lobe in zip(DIFFUSE, LOBES)]
    elif glossy:
        m = [s.add_material(type_=A.YK_MAT_GLOSSY, color=(0.9, 0.85, 0.8), glossy_reflect=0.3, diffuse_color=c,
                            diffuse_reflect=d, **lobe) for (c, d), lobe in zip(DIFFUSE, LOBES)]
    else:
        m = [s.add_material(color=c, diffuse_reflect=d) for c, d in DIFFUSE]
    s.add_mesh(np.array([[-2, 0, -2], [-2, 0, 2], [2, 0, 2], [2, 0, -2]], F), QUAD, m[0])
    s.add_mesh(np.array([[-2, 3, -2], [2, 3, -2], [2, 3, 2], [-2, 3, 2]], F), QUAD, m[1])
    s.add_mesh(np.array([[-2, 0, 2], [-2, 3, 2], [2, 3, 2], [2, 0, 2]], F), QUAD, m[2])
    s.add_mesh(np.array([[-2, 0, -2], [-2, 3, -2], [-2, 3, 2], [-2, 0, 2]], F), QUAD, m[3])
    s.add_mesh(np.array([[2, 0, -2], [2, 0, 2], [2, 3, 2], [2, 3, -2]], F), QUAD, m[4])
    b = np.array([[x, y, z] for x in (-0.7, 0.2) for y in (0.0, 1.0) for z in (-0.3, 0.6)], F)
    s.add_mesh(b, BOX_FACES, m[5])
    s.add_area_light((-0.5, 2.9, -0.5), (0.5, 2.9, -0.5), (-0.5, 2.9, 0.5), (1.0, 0.95, 0.9), 6.0, 2)
    s.set_camera((0.0, 1.5, -5.0), (0, 1.5, 0), (0.0, 2.5, -5.0), res, res, focal=1.4)
    s.build()
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--coated", action="store_true", help="also the room with every glossy surface coated")
    a = ap.parse_args()
    p = A.yk_render_params()
    A.lib().yk_render_params_default(C.byref(p))
    p.integrator = A.YK_INTEGRATOR_PATH
    p.width = p.height = a.res
    p.aa_samples = a.spp
    p.caustic_type = A.YK_CAUSTIC_NONE
    p.path_samples = 1
    p.bounces = 4
    dev = Device(0)
    for form in (("coated",) if a.coated else ()) + ("glossy", "shinydiffuse"):
        if form == "coated":
            p.raydepth = 2  # the other forms hold no specular material: raydepth does not reach them
        dev.upload(room(a.res, form))
        film = dev.new_film(p)

        def step(st):
            film.zero_()
            dev.render_shard(p, film, 0, 1, st)
            return dev.film_resolve(p, film)

        for _ in range(a.warmup):
            step(A.yk_stats())
        st = A.yk_stats()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            rgba = step(st)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert bool(torch.isfinite(rgba).all()) and float(rgba[..., :3].max()) > 0
        rays = st.closest_rays + st.shadow_rays
        print(json.dumps({"form": form, "res": a.res, "spp": a.spp, "steps": a.steps, "bounces": p.bounces,
                          "Mrays/s": round(rays / dt * 1e-6, 1), "ms_per_step": round(dt / a.steps * 1e3, 2),
                          "closest_rays": st.closest_rays // a.steps, "shadow_rays": st.shadow_rays // a.steps}))
    dev.close()


if __name__ == "__main__":
    main()
