#!/usr/bin/env python3
"""Generates tests/golden/kat_ref3.json: the reference's randomInUnitSphere (Random.cu:50-58) on 50 000 seeds, and
Interval::surrounds / Bounds3f::getCentroid on 5 000 intervals and huge boxes, run through oracle/_ref/ref_kat, so that
test_oracle_kat.py compares the oracle with them in every checkout and not only where the reference binary can be built.
The inputs come from a fixed integer hash (inputs() below); the file keeps, per output, the SHA-256 of all of its bytes
and its first 256 values as bit patterns (data, no source).
Build container only:   make -C oracle ref && python tests/golden/make_kat_golden3.py"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import ref_kat as rk  # noqa: E402

HEAD = 256


def _hash32(n, salt):
    """n well-mixed u32 values (splitmix64 finaliser of index + salt): the same on every machine and numpy version."""
    x = (np.arange(n, dtype=np.uint64) + np.uint64(salt)) * np.uint64(0x9E3779B97F4A7C15)
    x ^= x >> np.uint64(30)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(27)
    x *= np.uint64(0x94D049BB133111EB)
    x ^= x >> np.uint64(31)
    return (x >> np.uint64(32)).astype(np.uint32)


def _uniform(n, salt, lo, hi):
    return (lo + (hi - lo) * (_hash32(n, salt).astype(np.float64) / 2.0 ** 32)).astype(np.float32)


def inputs():
    """sphere_seeds u32 [50000]; iv f32 [5000, 3] (min, max, x); boxes f32 [5000, 6] (lo, hi), |coordinates| up to 1e30."""
    return {"sphere_seeds": _hash32(50000, 7),
            "iv": _uniform(15000, 11, -3.0, 3.0).reshape(5000, 3),
            "boxes": (_uniform(30000, 13, -1.0, 1.0) * np.float32(1e30)).reshape(5000, 6)}


def summary(a):
    """SHA-256 of the little-endian bytes, and the first HEAD elements as u32 / i32 bit patterns."""
    a = np.ascontiguousarray(a)
    a = a.astype(a.dtype.newbyteorder("<"))
    bits = a.view("<u4" if a.dtype.kind in "fu" else "<i4").reshape(-1)
    return {"dtype": a.dtype.str, "shape": list(a.shape), "sha256": hashlib.sha256(a.tobytes()).hexdigest(),
            "head_bits": [int(b) for b in bits[:HEAD]]}


def main():
    if not rk.available():
        sys.exit("oracle/_ref/ref_kat missing: run `make -C oracle ref` in the build container first")
    x = inputs()
    v, seed_end = rk.unitsphere(x["sphere_seeds"])
    out = {"sphere_v": summary(v.astype("<f4")), "sphere_seed_end": summary(seed_end.astype("<u4")),
           "surrounds": summary(rk.surrounds(x["iv"]).astype("<i4")),
           "boundscentroid": summary(rk.boundscentroid(x["boxes"]).astype("<f4"))}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kat_ref3.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("wrote", path, os.path.getsize(path), "bytes; surrounded", int(rk.surrounds(x["iv"]).sum()), "/", len(x["iv"]))


if __name__ == "__main__":
    main()
