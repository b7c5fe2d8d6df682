"""The isosurface entry point of include/drt.h without a GPU: exported, bound, drt_iso_tri's size and offsets, every argument check
that comes before any device work, the header states the rule with the restatement's table row for row and says what it is not, the
Python wrappers refuse bad arguments, and the C++ wrapper compiles and links."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import isosurface_ref as iso
from tests.scenes import ROOT

drt = pytest.importorskip("dustraytracer_amd")

NAN = float("nan")


def test_the_symbol_is_exported_and_bound():
    lib = ctypes.CDLL(drt.LIB_PATH)
    P, U, I, Fl = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32, ctypes.c_float
    assert hasattr(lib, "drt_renderer_isosurface")
    assert list(drt._lib.drt_renderer_isosurface.argtypes) == [P, P, P, Fl, Fl, I, P, P, U, P, P]
    for name in ("isosurface", "remesh"):
        assert callable(getattr(drt.Renderer, name)), name
    for name in ("records", "faceNormals", "toScene"):
        assert callable(getattr(drt.Isosurface, name)), name
    assert drt.Isosurface._fields == ("splits", "tris", "cube", "code")
    assert ctypes.sizeof(drt._Grid) == 36 and iso.RECORD.itemsize == 48
    doc = " ".join(drt.Renderer.isosurface.__doc__.split())
    for phrase in ("no vertex index buffer", "a sample exactly equal to level is above", "no gradient normals",
                   "roughly twice the triangles of marching cubes", "the piecewise-linear interpolant and no better",
                   "no simplification, no smoothing and no dual or sharp-feature methods", "no RendererGroup and no command line"):
        assert phrase in doc, phrase
    assert drt._lib.drt_abi_version() == 2


def grid(dims=(4, 3, 2), lo=(0, 0, 0), cell=(1, 1, 1)):
    g = drt._Grid()
    g.lo[:], g.cell[:], g.dims[:] = lo, cell, dims
    return g


def test_every_check_returns_its_error_code_with_no_launch():
    L = drt._lib
    stand_in = ctypes.create_string_buffer(1 << 16)              # a block of zeros stands in for the renderer: it is not looked at yet
    h = ctypes.addressof(stand_in)
    buf = ctypes.create_string_buffer(1 << 12)
    A = (ctypes.addressof(buf) + 15) & ~15                        # field, offsets, counts and out all point into host memory
    F, OFF, CNT, OUT = A, A + 256, A + 512, A + 1024
    g = grid()

    def call(r=h, field=F, gr=g, level=0.0, border=NAN, flip=0, offsets=OFF, out=OUT, cap=4, counts=CNT):
        return L.drt_renderer_isosurface(r, field, ctypes.byref(gr) if gr is not None else None, level, border, flip, offsets, out, cap, counts, None)

    def refused(what, **kw):
        assert call(**kw) == drt.ERR_INVALID, kw
        assert what in L.drt_last_error(), (kw, L.drt_last_error())

    refused(b"null argument", r=None)
    refused(b"null argument", field=None)
    refused(b"null argument", gr=None)
    refused(b"flip", flip=2)
    refused(b"flip", flip=-1)
    refused(b"both null", out=None, cap=0, counts=None)
    refused(b"if and only if", out=None, cap=4)
    refused(b"if and only if", out=OUT, cap=0)
    refused(b"offset", offsets=None)
    refused(b"aligned", out=OUT + 8)
    refused(b"aligned", field=F + 2)
    refused(b"aligned", offsets=OFF + 1)
    refused(b"aligned", counts=CNT + 2)
    refused(b"border", border=float("inf"))
    refused(b"border", border=-float("inf"))
    for k in range(3):
        dims = [4, 3, 2]
        dims[k] = 1
        refused(b"dims[%d]" % k, gr=grid(dims))
        assert call(gr=grid(dims), border=-1.0) in (drt.ERR_INVALID, drt.ERR_DEVICE) and b"dims" not in L.drt_last_error()   # 1 is enough with a border
        dims[k] = 0
        refused(b"dims[%d]" % k, gr=grid(dims), border=-1.0)
    refused(b"2^31", gr=grid((2048, 2048, 512)))                  # 2^31 samples
    refused(b"2^31", gr=grid((0x7fffffff, 2, 2)))
    refused(b"2^31", gr=grid((1290, 1290, 1290)), border=0.0)     # 1290^3 samples < 2^31 <= 1291^3 cubes
    for level in (NAN, float("inf"), -float("inf")):
        refused(b"level", level=level)
    refused(b"lo and cell", gr=grid(lo=(0, NAN, 0)))
    refused(b"lo and cell", gr=grid(cell=(1, 1, float("inf"))))
    # the order: an earlier check answers first
    refused(b"flip", flip=3, level=NAN, out=OUT + 8)
    refused(b"aligned", out=OUT + 8, level=NAN, gr=grid((1, 1, 1)))
    refused(b"dims", gr=grid((1, 3, 2)), level=NAN)
    refused(b"level", level=NAN, gr=grid(lo=(NAN, 0, 0)))
    # all of them passed: only now the renderer is looked at (zeros: no batch pending) and the device asked for -- host memory or no
    # device, either way the call fails after the checks
    for kw in ({}, dict(out=None, cap=0, offsets=None), dict(counts=None), dict(border=-1.0, flip=1)):
        assert call(**kw) in (drt.ERR_INVALID, drt.ERR_DEVICE), kw
        assert b"device" in L.drt_last_error().lower() or b"hip" in L.drt_last_error().lower()
    pending = ctypes.create_string_buffer(b"\xff" * (1 << 16), 1 << 16)      # every flag of the stand-in set: a batch is pending
    refused(b"pending", r=ctypes.addressof(pending))


def test_bad_arguments_are_refused_by_the_python_interface_before_any_device_work():
    r = drt.Renderer.__new__(drt.Renderer)                                     # (no device: only the argument check runs)
    r._device = 0
    sc = drt.Scene()
    f = np.zeros((3, 3, 3), np.float32)
    box = ((0, 0, 0), (1, 1, 1))
    cases = [(lambda: r.remesh(sc, 0), "resolution"), (lambda: r.remesh(sc, (4, 4)), "resolution"), (lambda: r.remesh(sc, 2.5), "resolution"),
             (lambda: r.remesh(sc, (4, -1, 4)), "resolution"), (lambda: r.remesh(sc, True), "resolution"),
             (lambda: r.remesh(sc, 8, field="occupancy"), "field"), (lambda: r.remesh(sc, 8, field=None), "field"),
             (lambda: r.remesh(sc, 8, margin=-1), "margin"), (lambda: r.remesh(sc, 8, margin=0.5), "margin"),
             (lambda: r.remesh(sc, 8, level=NAN), "level"), (lambda: r.remesh(sc, 8, level="x"), "level"),
             (lambda: r.remesh(sc, 8, level=float("inf")), "level"),
             (lambda: r.isosurface(f, NAN, *box), "level"), (lambda: r.isosurface(f, float("inf"), *box), "level"),
             (lambda: r.isosurface(f, None, *box), "level"), (lambda: r.isosurface(f, 0.0, *box, border=float("inf")), "border"),
             (lambda: r.isosurface(f, 0.0, (0, 0), (1, 1, 1)), "lo and hi"), (lambda: r.isosurface(f, 0.0, (0, 0, NAN), (1, 1, 1)), "lo and hi")]
    for call, word in cases:
        with pytest.raises(drt.DrtError) as e:
            call()
        assert e.value.code == drt.ERR_INVALID and word in str(e.value), (word, str(e.value))


def _flat(text):
    return re.sub(r" +", " ", re.sub(r"\s*\n \*\s*", " ", text))


def test_the_header_states_the_rule_and_what_it_is_not():
    text = open(os.path.join(ROOT, "include", "drt.h")).read()
    flat = _flat(text[text.index("isosurface extraction (new"):text.index("typedef struct drt_grid")])
    for phrase in ("fp32 with one rounding per operation, in the order written", "lo + ((float)idx + 0.5f) * cell",
                   "c = dx + 2 dy + 4 dz", "(0,1,3,7) (0,1,5,7) (0,2,3,7) (0,2,6,7) (0,4,5,7) (0,4,6,7)", "above iff f >= level",
                   "fabsf(f) <= FLT_MAX", "t = (level - fa) / (fb - fa), P = pa + (pb - pa) * t per component",
                   "from the end a = p with the smaller corner number", "0 = (0,1), 1 = (0,2), 2 = (0,3), 3 = (1,2), 4 = (1,3), 5 = (2,3)",
                   "Tetrahedra 1, 2 and 5 are mirror images", "flip = 1 makes them change places once more",
                   "cross(v1 - v0, v2 - v0) points to the above side", "ascending cube index (z, then y, then x), then tetrahedron 0..5",
                   "code = tetrahedron | case << 4", "cube = 0xffffffff and zeros everywhere else", "lattice indices -1 and dims[k]",
                   "(X+1)(Y+1)(Z+1) cubes", "Nothing of the padded field is materialised", "row = cy + ny * cz",
                   "out is NULL iff out_capacity == 0", "every dims[k] >= 2 (>= 1 with a border)", "level finite; lo and cell finite"):
        assert phrase in flat, phrase
    # the table, row for row
    for case, row in enumerate(iso.TABLE):
        want = "%d: %s" % (case, " ".join("(%d,%d,%d)" % t for t in row) if row else "--")
        assert re.search(r"(?<!\d)" + re.escape(want) + r"(?! ?\()", flat), want
    limits = flat[flat.index("What this is not:"):]
    for phrase in ("no vertex index buffer", "drt_tri_edge_adjacency recovers the connectivity", "a sample exactly equal to level is above",
                   "which the adjacency marks -2", "no gradient normals", "roughly twice the triangles of marching cubes",
                   "the piecewise-linear interpolant and is no better", "no simplification, no smoothing and no dual or sharp-feature methods",
                   "no drt_group_* form and no command line"):
        assert phrase in limits, phrase
    assert "the isosurface entry point (drt_renderer_isosurface)" in _flat(text[:text.index("#define DRT_ABI_VERSION 2")])


def test_the_kernel_table_is_the_restatements():
    src = open(os.path.join(ROOT, "dustraytracer_amd", "csrc", "isosurface.hpp")).read()
    rows = re.findall(r"DRT_ISO_ROW([012])\(([0-9, ]*)\)", src[src.index("#define DRT_ISO_TABLE"):])
    assert len(rows) == 16
    for case, (n, args) in enumerate(rows):
        e = [int(v) for v in args.split(",")] if args.strip() else []
        assert int(n) == len(iso.TABLE[case]) and tuple(tuple(e[3 * j:3 * j + 3]) for j in range(int(n))) == iso.TABLE[case], case
    tets = [(0, (1, 1, 2, 2, 4, 4)[i], (3, 5, 3, 6, 5, 6)[i], 7) for i in range(6)]
    assert tuple(tets) == iso.TETS and iso.MIRROR == (0, 1, 1, 0, 0, 1)


def test_cpp_wrapper_compiles_and_links(tmp_path):
    src = tmp_path / "isosurface_calls.cpp"
    src.write_text(r"""
#include <cstddef>
#include <cstdio>
#include "DustRayTracer.hpp"
static_assert(sizeof(drt_iso_tri) == sizeof(drt_tri), "a fill's output is a drt_tri batch");
// the statements only -- main() runs none of them without arguments
int main(int argc, char **) {
    if (argc < 2) {
        std::printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(drt_iso_tri), offsetof(drt_iso_tri, v), offsetof(drt_iso_tri, cube),
                    offsetof(drt_iso_tri, code), offsetof(drt_iso_tri, zero), sizeof(drt_grid), offsetof(drt_grid, cell), offsetof(drt_grid, dims));
        return 0;
    }
    Renderer r(0);
    const float *field = nullptr;
    drt_grid grid = {{0, 0, 0}, {1, 1, 1}, {2, 2, 2}};
    uint32_t *offsets = nullptr, *counts = nullptr;
    drt_iso_tri *out = nullptr;
    r.Isosurface(field, grid, 0.0f, nullptr, nullptr, 0u, counts);
    r.Isosurface(field, grid, 0.5f, offsets, out, 16u, nullptr, true, 0.0f, nullptr);
    return 0;
}
""")
    lib_dir = os.path.dirname(drt.LIB_PATH)
    exe = tmp_path / "isosurface_calls"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib_dir, "-ldrt_hip",
                    "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["48", "0", "36", "40", "44", "36", "12", "24"]
