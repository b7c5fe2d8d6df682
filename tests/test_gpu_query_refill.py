"""The claim of the batched query kernels (csrc/query_frame.hpp) at other refill thresholds: DRT_RQ_REFILL = 1 (a wave claims as soon
as one lane is idle) and = 64 (only when all are) against the default, for one kernel with the closest-hit stack (nearest), one with
the occlusion stack (occluded) and one list kernel (overlapBoxes in mode LIST).  A result depends only on its query and the scene, so
every output is bit-equal to the default's and to the restatement's (tests/nearest_ref.py, ray_query_ref.py, overlap_ref.py)."""
import os

import numpy as np
import pytest

import oracle
from tests import nearest_ref as nr
from tests import overlap_ref as ov
from tests import ray_query_ref as rq
from tests.scenes import scene_path

drt = pytest.importorskip("dustraytracer_amd")
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

NAME = "suzanne_plane"
N = 1000                                        # more than a 256-thread workgroup, and no multiple of a wave; 65 = one wave and a lane


def renderer_with_refill(value):
    """A fresh renderer that read DRT_RQ_REFILL = value (None: unset, the default); the environment is restored."""
    old = os.environ.get("DRT_RQ_REFILL")
    if value is None:
        os.environ.pop("DRT_RQ_REFILL", None)
    else:
        os.environ["DRT_RQ_REFILL"] = str(value)
    try:
        return drt.Renderer(0)
    finally:
        if old is None:
            os.environ.pop("DRT_RQ_REFILL", None)
        else:
            os.environ["DRT_RQ_REFILL"] = old


def run(r, sc, kind, q, n):
    """The query's outputs for the first n inputs, as a tuple of host arrays."""
    if kind == "nearest":
        return tuple(np.ascontiguousarray(f) for f in r.nearest(sc, q[:n]))
    if kind == "occluded":
        return (r.occluded(sc, q[0][:n], q[1][:n]),)
    got = r.overlapBoxes(sc, q[:n])
    return (got.splits, got.prim)


@pytest.fixture(scope="module")
def world():
    """The scene, the inputs of the three queries, and for each its outputs at n = N from the restatement (computed once, left
    unchanged: the outputs at a smaller n are their prefix) and from a renderer at the default setting."""
    sc = drt.Scene()
    sc.loadGLTFmodel(scene_path(NAME))
    b = drt.BVHBuilder()
    b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
    b.buildIterative(sc)
    osc = oracle.Scene.load_glb(scene_path(NAME)).build_bvh(20, 8)
    g = nr.from_oracle(osc)
    rng = np.random.default_rng(23)
    points = np.concatenate([nr.surface_points(g, N // 2, rng), nr.box_points(g, N - N // 2, rng)]).astype(np.float32)
    org, dirs = rq.surface_rays(osc, N, rng)
    lo, hi = nr.bounds(g)
    half = (rng.uniform(0, 1, (N, 3)) ** 3 * np.float32(0.1) * np.float32((hi - lo).max())).astype(np.float32)
    rot, _ = np.linalg.qr(rng.normal(size=(N, 3, 3)))
    axes = rot.astype(np.float32)
    axes[::2] = np.eye(3, dtype=np.float32)
    boxes = ov.pack(nr.surface_points(g, N, rng), half, axes)
    queries = {"nearest": points, "occluded": (org, dirs), "overlap": boxes}
    near = nr.nearest(g, points)
    occ = rq.occluded(osc, org, dirs, np.float32(0), np.float32(np.inf))
    _, totals = ov.overlap(g, boxes, 0)
    lists, _ = ov.overlap(g, boxes, totals)
    assert (near.prim >= 0).all() and occ.any() and not occ.all() and totals.max() > 1 and (totals == 0).any()
    ref = {"nearest": tuple(np.ascontiguousarray(f) for f in near), "occluded": (occ,), "overlap": (totals, lists)}
    default = renderer_with_refill(None)
    base = {(kind, n): run(default, sc, kind, queries[kind], n) for kind in queries for n in (65, N)}
    return sc, queries, ref, base


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8) if a.dtype == np.bool_ else a.view(np.uint32)


def reference(ref, kind, n):
    """The restatement's outputs for the first n inputs, in run()'s form."""
    if kind != "overlap":
        return tuple(f[:n] for f in ref[kind])
    totals, lists = ref[kind]
    splits = np.concatenate([[0], np.cumsum(totals[:n].astype(np.int64))])
    return (splits.astype(np.int32), lists[:splits[-1]])


@pytest.mark.parametrize("refill", [1, 64])
@pytest.mark.parametrize("n", [65, N])
@pytest.mark.parametrize("kind", ["nearest", "occluded", "overlap"])
def test_outputs_do_not_depend_on_the_refill_threshold(world, kind, n, refill):
    sc, queries, ref, base = world
    got = run(renderer_with_refill(refill), sc, kind, queries[kind], n)
    want, default = reference(ref, kind, n), base[(kind, n)]
    assert len(got) == len(want) == len(default)
    for k, (a, b, c) in enumerate(zip(got, default, want)):
        what = "%s n=%d DRT_RQ_REFILL=%d output %d" % (kind, n, refill, k)
        assert a.shape == b.shape == c.shape and a.dtype == b.dtype, what
        assert (bits(a) == bits(b)).all(), what + ": differs from the default setting"
        assert (bits(a) == bits(c.astype(a.dtype))).all(), what + ": differs from the restatement"
