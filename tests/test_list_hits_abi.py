"""The hit-list entry point of include/drt.h without a GPU: exported, bound, the result tuples as declared, the argument checks that
come before any device work, the header states the rule and its limits, and the C++ wrapper compiles and links against it."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests.scenes import ROOT

drt = pytest.importorskip("dustraytracer_amd")


def test_the_symbol_is_exported_and_bound():
    lib = ctypes.CDLL(drt.LIB_PATH)
    assert hasattr(lib, "drt_renderer_list_hits")
    fn = drt._lib.drt_renderer_list_hits
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 9
    assert fn.argtypes[5] is ctypes.c_uint32 and fn.argtypes[7] is ctypes.c_uint32                       # hits_capacity, n
    assert all(fn.argtypes[i] is ctypes.c_void_p for i in (0, 1, 2, 3, 4, 6, 8))
    for method in ("firstHits", "listHits"):
        assert callable(getattr(drt.Renderer, method)), method
    assert drt.FirstHits._fields == ("t", "prim", "u", "v", "count")
    assert drt.HitList._fields == ("splits", "t", "prim", "u", "v")
    assert drt._lib.drt_abi_version() == 2


def test_null_handles_are_invalid_without_a_gpu():
    L = drt._lib
    sc = drt.Scene()
    assert L.drt_renderer_list_hits(None, sc._h, None, None, None, 0, None, 4, None) == drt.ERR_INVALID
    assert b"null" in L.drt_last_error()
    assert L.drt_renderer_list_hits(None, None, None, None, None, 0, None, 0, None) == drt.ERR_INVALID     # the handles are checked before n == 0


def test_a_bad_k_is_refused_before_any_device_work():
    r = drt.Renderer.__new__(drt.Renderer)                                     # (no device: only the argument check runs)
    r._device = 0
    sc = drt.Scene()
    rays = np.zeros((3, 8), np.float32)
    for k in (0, -1, 2.5, None, True):
        with pytest.raises(drt.DrtError) as e:
            r.firstHits(sc, rays, k=k)
        assert e.value.code == drt.ERR_INVALID and "k" in str(e.value)
    # N * k >= 2^31 records: refused by the shape alone (a broadcast view: no memory behind it)
    many = np.broadcast_to(np.zeros((1, 8), np.float32), (2 ** 20, 8))
    with pytest.raises(drt.DrtError) as e:
        r.firstHits(sc, many, k=2 ** 11)
    assert e.value.code == drt.ERR_INVALID and "2^31" in str(e.value)


def test_the_header_states_the_rule_and_its_limits():
    text = open(os.path.join(ROOT, "include", "drt.h")).read()
    sec = text[text.index("ordered hit lists of rays (new"):text.index("int           drt_renderer_list_hits")]
    flat = re.sub(r"\s*\n \*\s*", " ", sec)
    for phrase in ("read as drt_renderer_trace_rays reads it", "on the stored (v0, e1, e2)", "carry the bits drt_renderer_trace_rays reports",
                   "listed iff the test hits, t > tmin and t < tmax", "Alpha cut-outs are ignored", "the root is skipped if d < 0 || d > tmax",
                   "a child is pushed iff d >= 0 && !(d > tmax)", "farther child is pushed first", "total == drt_crossings.count",
                   "ascending t; equal t by ascending prim", "a.t < b.t || (a.t == b.t && a.prim < b.prim)", "never NaN and always > 1e-6",
                   "does not depend on the traversal", "offsets holds n + 1 uint32 values", "hits[offsets[i] .. offsets[i+1])",
                   "cap_i = offsets[i+1] > offsets[i] ? offsets[i+1] - offsets[i] : 0", "offsets[i] + cap_i <= hits_capacity",
                   "offsets[i] >= hits_capacity gives 0", "and nothing else in hits", "the miss record {tmax, -1, 0, 0}", "the ray's own word, bit for bit",
                   "counts[i] = total_i", "not just the stored ones", "the ray, the scene and cap_i only", "are the list at capacity K",
                   "counts may be NULL", "hits may be NULL iff hits_capacity == 0", "both NULL is DRT_ERR_INVALID"):
        assert phrase in flat, phrase
    limits = flat[flat.index("What this is not:"):]
    for phrase in ("alpha-tested lists", "per-hit normals or materials", "NOT culled by the K-th distance", "would no longer be the total",
                   "do not order consistently", "handles are checked before n == 0", "n == 0 is a no-op", "n < 2^31", "rays and hits 16-byte aligned",
                   "offsets and counts 4-byte aligned", "the call only enqueues", "refitted device copy", "sharded renderer",
                   "DRT_ERR_UNSUPPORTED beyond 64 levels", "DRT_ERR_INVALID while an asynchronous batch is pending",
                   "counters, kernel info and kernel span are not touched"):
        assert phrase in limits, phrase
    assert "drt_renderer_list_hits" in text[:text.index("#define DRT_ABI_VERSION 2")]
    # the crossings section points here
    crossings = re.sub(r"\s*\n \*\s*", " ", text[text.index("crossing counts, inside / outside and signed distance (new"):text.index("typedef struct drt_crossings")])
    assert "first K hits per ray is drt_renderer_list_hits, below" in crossings


def test_cpp_wrapper_compiles_and_links(tmp_path):
    src = tmp_path / "list_hits_calls.cpp"
    src.write_text(r"""
#include <cstdio>
#include "DustRayTracer.hpp"
// the statements only -- main() runs none of them without arguments
int main(int argc, char **) {
    if (argc < 2) { std::printf("%zu %zu %d\n", sizeof(drt_hit), sizeof(drt_ray), DRT_ABI_VERSION); return 0; }
    Scene scene;
    Renderer r(0);
    const drt_ray *rays = nullptr;
    const uint32_t *offsets = nullptr;
    drt_hit *hits = nullptr;
    uint32_t *counts = nullptr;
    r.ListHits(scene, rays, offsets, hits, 0u, counts, 0u);
    r.ListHits(scene, rays, offsets, hits, 0u, counts, 0u, nullptr);
    return 0;
}
""")
    lib_dir = os.path.dirname(drt.LIB_PATH)
    exe = tmp_path / "list_hits_calls"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib_dir, "-ldrt_hip",
                    "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["16", "32", "2"]
