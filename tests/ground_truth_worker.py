"""A fresh process for tests/test_ground_truth.py: settings libyk reads once
per process (YK_CROWDED_LEAF) come from this process's environment. Traces
the given rays on the hair scene and writes the answers.

  python -m tests.ground_truth_worker RAYS.npz ANSWERS.npz
"""
import os
import sys

import numpy as np


def main():
    src, dst = sys.argv[1], sys.argv[2]
    import torch  # noqa: F401  (before libyk: one HIP runtime)
    from core_amd.device import Device
    from core_amd.scene import probe_scene
    r = np.load(src)
    s, _ = probe_scene("hair", 32, 32, 300, 9)
    dev = Device(0)
    dev.upload(s)
    hits = dev.trace_closest(dev.rays_to_device(r["rays"])).cpu().numpy()
    occ = [dev.trace_shadow(dev.rays_to_device(r[k])).cpu().numpy() for k in ("shadow0", "shadow1")]
    dev.close()
    np.savez(dst, hits=hits, occ0=occ[0], occ1=occ[1], crowded_leaf=float(os.environ.get("YK_CROWDED_LEAF", "nan")))


if __name__ == "__main__":
    main()
