"""Writes tests/golden/ref_fpow.npz: inputs and the reference's own fPow, fLog2
and fExp2 (utilities/mathOptimizations.h:100-125,200-207, FAST_MATH), from a
throw-away program compiled HERE against the reference header by path. The
program only includes the header; none of its text is written or committed.

Flags: -O2 -DFAST_MATH, no -ffast-math and no contraction -- the functions "as
written", which is what the device and tests/glossy_common.py restate (integer
arithmetic on the float's bits, a Horner polynomial whose fourth constant is
a double literal).

Inputs: bases dense over [0, 1] plus -0.5, 0, 1 and their neighbours;
exponents 0.5, 1, 5, 50, 500, 5000 and the 1 / (e + 1) values Blinn_Sample
forms from them. At most 1 % of the results may be subnormal (asserted): a
device that flushes them reads zero there, and the tests bound that class.

Run in the build container (needs /root/reference):
    python tests/golden/gen/make_ref_fpow.py
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", "..", ".."))
REF_INCLUDE = os.environ.get("YK_REFERENCE", "/root/reference") + "/include"

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#define __BEGIN_YAFRAY namespace yafaray {
#define __END_YAFRAY }
#include <utilities/mathOptimizations.h>
int main(int argc, char** argv) {
  FILE* f = fopen(argv[1], "rb");
  unsigned n = 0;
  if (!f || fread(&n, 4, 1, f) != 1) return 1;
  std::vector<float> a(n), b(n);
  if (fread(a.data(), 4, n, f) != n || fread(b.data(), 4, n, f) != n) return 1;
  fclose(f);
  std::vector<float> p(n), l(n), e(n);
  for (unsigned i = 0; i < n; ++i) {
    p[i] = yafaray::fPow(a[i], b[i]);
    l[i] = yafaray::fLog2(a[i]);
    e[i] = yafaray::fExp2(b[i]);
  }
  f = fopen(argv[2], "wb");
  fwrite(p.data(), 4, n, f);
  fwrite(l.data(), 4, n, f);
  fwrite(e.data(), 4, n, f);
  fclose(f);
  return 0;
}
"""


def inputs():
    F = np.float32
    rng = np.random.default_rng(20260)
    dense = np.concatenate([np.linspace(0.0, 1.0, 513, dtype=F), rng.random(384, dtype=F),
                            (F(1.0) - rng.random(128, dtype=F) * F(0.01)).astype(F)])
    edge = []
    for v in (-0.5, 0.0, 1.0):
        v = F(v)
        edge += [np.nextafter(v, F(-2)), v, np.nextafter(v, F(2))]
    bases = np.concatenate([dense, np.array(edge, F)])
    exps = np.array([0.5, 1, 5, 50, 500, 5000], F)
    exps = np.concatenate([exps, (F(1.0) / (exps + F(1.0))).astype(F)])
    a, b = np.meshgrid(bases, exps, indexing="ij")
    return np.ascontiguousarray(a.ravel(), F), np.ascontiguousarray(b.ravel(), F)


def main():
    a, b = inputs()
    n = len(a)
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "fpow_probe.cc"), os.path.join(d, "fpow_probe")
        with open(src, "w") as f:
            f.write(PROGRAM)
        subprocess.run(["g++", "-O2", "-DFAST_MATH", "-ffp-contract=off", "-I", REF_INCLUDE, "-o", exe, src],
                       check=True)
        with open(os.path.join(d, "in.bin"), "wb") as f:
            f.write(np.uint32(n).tobytes() + a.tobytes() + b.tobytes())
        subprocess.run([exe, os.path.join(d, "in.bin"), os.path.join(d, "out.bin")], check=True)
        out = np.fromfile(os.path.join(d, "out.bin"), np.uint32).reshape(3, n)
    res = out[0].view(np.float32)
    sub = (res != 0) & (np.abs(res) < np.finfo(np.float32).tiny)
    assert sub.mean() <= 0.01, f"{sub.sum()} of {n} fPow results are subnormal"
    dst = os.path.join(ROOT, "tests", "golden", "ref_fpow.npz")
    np.savez_compressed(dst, a=a, b=b, fpow=out[0], flog2=out[1], fexp2=out[2])
    print(dst, n, "inputs,", int(sub.sum()), "subnormal results,", os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    sys.exit(main())
