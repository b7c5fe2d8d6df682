#!/usr/bin/env python3
"""The tile arithmetic and the ray rule of dustraytracer_amd/csrc/ambient.hpp on the host under AddressSanitizer and
UndefinedBehaviorSanitizer: builds tools/ambient_host_check.cpp as a stand-alone program, lets it walk the tiling of
every sample count (every (point, sample) pair exactly once, 64-bit tile counts at n = 2^32 - 1 with S = 4096), and compares the
origin, the direction and the three bent terms of every sample it makes -- finite points, NaN and infinite ones, zero and huge
normals, `first` at the end of its range -- with the restatement in tests/ambient_ref.py, bit for bit.  No GPU and no library of the
product.

    python tools/ambient_host_check.py [--points 300]
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import ambient_ref as ar  # noqa: E402

F = np.float32


def hostile_points(n, seed):
    """[n, 8] drt_ao_point: unit normals mostly, then zero, tiny, huge, NaN and infinite ones, NaN positions, every kind of max_dist."""
    rng = np.random.default_rng(seed)
    pts = np.zeros((n, 8), F)
    pts[:, 0:3] = rng.normal(size=(n, 3)) * 3
    nrm = rng.normal(size=(n, 3))
    pts[:, 4:7] = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    pts[:, 3] = rng.uniform(0, 5, n)
    pts[:, 7] = rng.choice([0.001, 0.0, -0.01, 1.0], n)
    kind = rng.integers(0, 16, n)
    pts[kind == 0, 4:7] = 0
    pts[kind == 1, 4:7] *= F(1e-30)
    pts[kind == 2, 4:7] *= F(1e30)
    pts[kind == 3, 4] = np.nan
    pts[kind == 4, 5] = np.inf
    pts[kind == 5, 0] = np.nan
    pts[kind == 6, 3] = np.inf
    pts[kind == 7, 3] = -1
    pts[kind == 8, 3] = np.nan
    pts[kind == 9, 7] = np.nan
    pts[kind == 10, 4:7] *= F(1e-20)
    return pts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=300)
    args = ap.parse_args()
    failures = 0
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "ambient_host_check")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tools", "ambient_host_check.cpp"), "-o", exe], check=True)
        subprocess.run([exe, "tiles"], check=True)                            # a sanitizer report or a mismatch ends it with a non-zero status
        for round_, (samples, seed, first) in enumerate([(1, 7, 0), (16, 0xDEADBEEF, 5), (7, 3, 2 ** 32 - args.points), (33, 0, 1), (64, 11, 0),
                                                         (65, 12, 77), (200, 2024, 0), (4096, 1, 2 ** 31)]):
            n = args.points if samples < 4096 else 6
            pts = hostile_points(n, 20 + round_)
            src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
            with open(src, "wb") as f:
                f.write(np.array([n, samples, seed, first], np.uint32).tobytes() + pts.tobytes())
            subprocess.run([exe, "rays", src, dst], check=True)
            got = np.fromfile(dst, np.uint32).reshape(n, samples, 9)
            o, d, tries = ar.rays(pts[:, 0:3], pts[:, 4:7], pts[:, 7], samples, seed, first)
            with np.errstate(invalid="ignore"):
                live = pts[:, 3] >= 0
            terms = np.where(live[:, None, None], ar.bent_terms(d), -1).astype(np.int32)
            want = np.concatenate([np.broadcast_to(o[:, None, :], d.shape).view(np.uint32), d.view(np.uint32), terms.view(np.uint32)], axis=2)
            # a NaN is a NaN whatever its payload and sign
            both_nan = np.zeros(want.shape, bool)
            both_nan[:, :, :6] = np.isnan(got[:, :, :6].view(F)) & np.isnan(want[:, :, :6].view(F))
            same = bool(((got == want) | both_nan).all())
            print("round %d: S = %d, %d points (%d directions NaN, %d skipped), first %d, longest rejection run %d: %s"
                  % (round_, samples, n, int(np.isnan(d).any(axis=2).sum()), int((~live).sum()), first, tries.max(), "equal" if same else "DIFFER"))
            failures += not same
    print("no sanitizer report" if not failures else "%d comparisons differ" % failures)
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())
