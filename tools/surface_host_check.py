#!/usr/bin/env python3
"""The per-record routines of dustraytracer_amd/csrc/surface.hpp on the host under AddressSanitizer and UndefinedBehaviorSanitizer
(DESIGN 5.29): builds tools/surface_host_check.cpp as a stand-alone program, runs it on a synthetic scene with every kind of material
and a texel pool allocated at its exact size, with references that include prim -1, n_tris, INT_MIN, INT_MAX and NaN, infinite and
far-out u / v, and compares every word it writes with the restatement in tests/surface_ref.py.  No GPU and no library of the product.

    python tools/surface_host_check.py [--tris 700] [--refs 4000] [--samples 4000]
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import surface_ref as sr  # noqa: E402


def pack_input(s, prim, u, v, with_normals, normals, n_samples, seed, first):
    n = len(s.v0)
    hot = np.concatenate([s.v0, s.e1, s.e2, s.fn], axis=1).astype(np.float32)
    cold = np.zeros((n, 8), np.float32)
    cold[:, 0:6] = s.uv.reshape(n, 6)
    cold.view(np.int32)[:, 6] = s.material
    mats = np.zeros((len(s.mats), 4), np.float32)
    mats[:, 0:3] = s.mats["albedo"]
    mats.view(np.int32)[:, 3] = s.mats["albedo_tex"]
    ext = np.zeros((len(s.mats), 8), np.float32)
    ext[:, 0:3], ext[:, 3], ext[:, 6] = s.mats["emissive"], s.mats["roughness"], s.mats["refractive_index"]
    ext.view(np.int32)[:, 4], ext.view(np.int32)[:, 5] = s.mats["metallic"], s.mats["transmission"]
    texs = np.array(s.texs, np.int64).astype(np.uint32).reshape(-1, 4)
    refs = np.zeros((len(prim), 4), np.float32)
    refs.view(np.int32)[:, 1], refs[:, 2], refs[:, 3] = prim, u, v
    head = np.array([n, len(s.mats), len(texs), len(s.pool), len(prim), int(with_normals), n_samples, seed, first], np.uint32)
    return b"".join(np.ascontiguousarray(x).tobytes() for x in (head, hot, cold, mats, ext, texs, s.pool, s.normals, s.order, normals, refs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=700)
    ap.add_argument("--refs", type=int, default=4000)
    ap.add_argument("--samples", type=int, default=4000)
    args = ap.parse_args()
    failures = 0
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "surface_host_check")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tools", "surface_host_check.cpp"), "-o", exe], check=True)
        for round_, (with_normals, seed, first) in enumerate([(0, 7, 0), (1, 0xDEADBEEF, 2 ** 32 - args.samples)]):
            s = sr.synthetic(args.tris, 11 + round_)
            prim, u, v = sr.hostile_refs(args.tris, args.refs, 5 + round_)
            normals = np.random.default_rng(3).normal(size=(args.tris, 3, 3)).astype(np.float32)
            src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
            with open(src, "wb") as f:
                f.write(pack_input(s, prim, u, v, with_normals, normals, args.samples, seed, first))
            subprocess.run([exe, src, dst], check=True)                      # a sanitizer report ends it with a non-zero status
            raw = open(dst, "rb").read()
            a, b = 96 * args.refs, 96 * args.refs + 8 * args.tris
            records = np.frombuffer(raw[:a], np.uint32).reshape(-1, 24)
            cdf = np.frombuffer(raw[a:b], np.uint64)
            samples = np.frombuffer(raw[b:], np.float32).reshape(-1, 4)
            want_cdf = sr.weights(s)
            ok = (sr.same(records, sr.lookup(s, prim, u, v, normals if with_normals else None)), [int(x) for x in cdf] == want_cdf,
                  samples.tobytes() == sr.sample(s, seed, first, args.samples, want_cdf).tobytes())
            hostile = int(((prim < 0) | (prim >= args.tris)).sum()), int((~np.isfinite(u) | ~np.isfinite(v)).sum())
            print("round %d: %d records (%d with prim out of range, %d with a NaN or infinite u / v) %s, %d weights %s, %d samples %s"
                  % (round_, len(records), hostile[0], hostile[1], "equal" if ok[0] else "DIFFER", len(cdf), "equal" if ok[1] else "DIFFER",
                     len(samples), "equal" if ok[2] else "DIFFER"))
            failures += ok.count(False)
    print("no sanitizer report" if not failures else "%d comparisons differ" % failures)
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())
