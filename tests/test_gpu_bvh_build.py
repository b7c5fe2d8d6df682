"""The GPU BVH build (drt_scene_build_bvh_device, kernel_bvh_build.hip) against the host restatement of
BVHBuilder.cu (drt_scene_build_bvh): same nodes in the same order, same triangle order, for every shipped scene, for
synthetic soups and for the catalogue of tests/bvh_build_cases.py (hostile meshes, costs that are no numbers, inf and NaN
vertices, chunk edges below the root, deep chains, refused builds), over several (leaf, bins) settings -- and the same
image and the same query answers afterwards.  The oracle's own builder (oracle/drt_oracle.c) is the third voice.

Every comparison is bit equality.  The one freedom of the device builder, the sign of a bound that is a zero, is pinned to
the order-independent value in _assert_same_tree and shown to be invisible to traversal in
test_zero_signs_are_invisible_to_traversal.  tests/test_bvh_build_cases.py pins the references on the catalogue (CPU) and
shows what each case meets.

Not reached here: error bit 2 of finalize_kernel (the reference's 512-entry stack) and kMaxLevels.  A chain peels one
triangle per level only with centroids in geometric progression, and float32's exponent range ends such a chain near 250
levels; a chain of 240 is refused by both CPU builders already (see tests/test_bvh_build_cases.py)."""
import numpy as np
import pytest

import oracle
from tests import bvh_build_cases as bc
from tests import nearest_ref as nr
from tests import overlap_ref as ov
from tests import ray_query_ref as rq
from tests import section_ref as sr
from tests.scenes import SCENES, scene_path

drt = pytest.importorskip("dustraytracer_amd")
pytestmark = pytest.mark.gpu

INT_FIELDS = ("is_leaf", "child1", "child2", "prim_count", "prim_start")
NEG_ZERO = np.float32(-0.0)


def _build(scene_factory, leaf, bins, device):
    sc = scene_factory()
    b = drt.BVHBuilder()
    b.m_TargetLeafPrimitivesCount, b.m_BinCount, b.m_BuildDevice = leaf, bins, device
    b.buildIterative(sc)
    return sc, b


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _order_independent_bounds(v):
    """(bmin, bmax) of one axis of a node as the device builder stores them, from the node's vertex coordinates v: the extremes skip
    NaNs; a zero minimum is -0 if any -0 is present, a zero maximum +0 if any +0 is; bmax = lo + (hi - lo) in float32."""
    v = v[~np.isnan(v)]
    lo, hi = v.min(), v.max()
    if lo == 0:
        lo = NEG_ZERO if ((v == 0) & np.signbit(v)).any() else np.float32(0.0)
    if hi == 0:
        hi = np.float32(0.0) if ((v == 0) & ~np.signbit(v)).any() else NEG_ZERO
    with np.errstate(all="ignore"):
        return np.float32(lo), np.float32(lo + np.float32(hi - lo))


def _assert_same_tree(host, dev, what):
    """Everything byte-equal, but for the sign of a bound that is a zero on both sides; there the device has the order-independent
    zero.  Returns the number of such words."""
    hn, dn = host.m_BVHNodes, dev.m_BVHNodes
    assert len(hn) == len(dn), what
    for f in INT_FIELDS:
        assert np.array_equal(hn[f], dn[f]), (what, f)
    tris = host.m_PrimitivesBuffer
    assert tris.tobytes() == dev.m_PrimitivesBuffer.tobytes(), what                           # triangle order, byte for byte
    assert host.triangleOrder().tobytes() == dev.triangleOrder().tobytes(), what
    pos = tris["vertex"]["position"]
    words = 0
    for k, f in enumerate(("bmin", "bmax")):
        diff = _bits(hn[f]) != _bits(dn[f])
        assert ((hn[f][diff] == 0) & (dn[f][diff] == 0)).all(), (what, f, hn[f][diff][:4], dn[f][diff][:4])
        for node, axis in np.argwhere(diff):
            s, c = int(hn["prim_start"][node]), int(hn["prim_count"][node])
            want = _order_independent_bounds(pos[s:s + c, :, axis].ravel())[k]
            assert _bits(dn[f][node, axis]) == _bits(want), (what, f, node, axis)
            words += 1
    return words


def _file_scene(name):
    def make():
        sc = drt.Scene()
        sc.loadGLTFmodel(scene_path(name))
        return sc
    return make


def _soup(n, seed, clustered=False):
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-10, 10, (n, 1, 3))
    size = 0.2
    if clustered:                                   # half of the triangles in a tight cluster: deep, unbalanced tree
        centre[: n // 2] = rng.normal(0, 0.5, (n // 2, 1, 3)) + 3.0
        size = 0.02
    pos = (centre + rng.uniform(-size, size, (n, 3, 3))).astype(np.float32)
    nrm = np.tile(np.array([0, 1, 0], np.float32), (n, 3, 1))
    uv = np.zeros((n, 3, 2), np.float32)
    mat = np.zeros(n, np.int32)

    def make():
        sc = drt.Scene()
        sc.addMaterial((0.8, 0.8, 0.8), -1)
        sc.setGeometry(pos, nrm, uv, mat)
        return sc
    return make


def _case_scene(name):
    return lambda: bc.product_scene(drt, bc.cases()[name].pos)


@pytest.mark.parametrize("leaf,bins", [(20, 8), (6, 8), (1, 4), (3, 16), (40, 2)])
def test_device_build_equals_host_build_on_every_scene(leaf, bins):
    refused = 0
    for name in sorted(SCENES):
        make = _file_scene(name)
        try:
            host, _ = _build(make, leaf, bins, -1)
        except drt.DrtError as e:                      # coincident triangles and small leaves: the reference would never return
            assert e.code == drt.ERR_BVH
            with pytest.raises(drt.DrtError) as e2:
                _build(make, leaf, bins, 0)
            assert e2.value.code == drt.ERR_BVH, name
            refused += 1
            continue
        dev, _ = _build(make, leaf, bins, 0)
        _assert_same_tree(host, dev, (name, leaf, bins))          # every scene is exact, up to the rule for a zero's sign
    assert refused < len(SCENES)


@pytest.mark.parametrize("n,seed,clustered,leaf,bins", [(1000, 1, False, 4, 8), (70_000, 2, False, 20, 8), (70_000, 3, True, 12, 8),
                                                       (300_000, 4, False, 20, 8), (513, 5, False, 1, 3)])
def test_device_build_equals_host_build_on_soups(n, seed, clustered, leaf, bins):
    make = _soup(n, seed, clustered)
    host, _ = _build(make, leaf, bins, -1)
    dev, b = _build(make, leaf, bins, 0)
    _assert_same_tree(host, dev, (n, seed, leaf, bins))
    assert b.m_LastBuildDeviceMs > 0


def _assert_oracle_tree(dev, osc, what):
    """The oracle's nodes: integers equal, bounds equal as floats (a NaN equal to a NaN; the oracle's zeros are the serial loop's)."""
    on, dn = osc.nodes, dev.m_BVHNodes
    assert len(on) == len(dn), what
    for f in INT_FIELDS:
        assert np.array_equal(dn[f].astype(np.int32), on[f]), (what, f)
    for f in ("bmin", "bmax"):
        assert ((dn[f] == on[f]) | (np.isnan(dn[f]) & np.isnan(on[f]))).all(), (what, f)
    assert dev.m_PrimitivesBuffer["vertex"]["position"].tobytes() == osc.tris["p"].tobytes(), what


def test_device_build_agrees_with_the_oracle_builder():
    """Not only with our own host code: the oracle's C restatement of BVHBuilder.cu gives the same nodes."""
    for name in ("cornell_box", "room", "suzanne_plane"):
        dev, _ = _build(_file_scene(name), 20, 8, 0)
        _assert_oracle_tree(dev, oracle.Scene.load_glb(scene_path(name)).build_bvh(20, 8), name)


@pytest.mark.parametrize("entry", bc.entries(), ids=bc.entry_id)
def test_device_build_equals_host_build_on_the_catalogue(entry):
    name, leaf, bins, returns = entry
    make = _case_scene(name)
    if returns:
        host, _ = _build(make, leaf, bins, -1)
        dev, _ = _build(make, leaf, bins, 0)
        _assert_same_tree(host, dev, entry)
        _assert_oracle_tree(dev, bc.oracle_scene(bc.cases()[name].pos).build_bvh(leaf, bins), entry)
        return
    good = bc.a_returning_setting(name)
    sc, _ = _build(make, *good, -1)                               # the tree and the triangle order that have to survive
    nodes, tris, order = sc.m_BVHNodes.tobytes(), sc.m_PrimitivesBuffer.tobytes(), sc.triangleOrder().tobytes()
    with pytest.raises(drt.DrtError) as e:
        bc.build(drt, sc, leaf, bins, 0)
    assert e.value.code == drt.ERR_BVH
    assert sc.m_BVHNodes.tobytes() == nodes and sc.m_PrimitivesBuffer.tobytes() == tris and sc.triangleOrder().tobytes() == order
    # and the scene still builds: on the device it gets what the host makes of the same triangles in the same order
    twice, _ = _build(make, *good, -1)
    bc.build(drt, twice, *good, -1)
    bc.build(drt, sc, *good, 0)
    _assert_same_tree(twice, sc, (entry, good))


def test_one_leaf_and_degenerate_inputs():
    make = _soup(10, 7)
    host, _ = _build(make, 20, 8, -1)
    dev, _ = _build(make, 20, 8, 0)                       # a single leaf: nothing to split
    assert host.m_BVHNodes.tobytes() == dev.m_BVHNodes.tobytes() and len(dev.m_BVHNodes) == 1
    # 50 copies of one triangle: every plane leaves a side empty; the reference loops forever, both builders refuse
    pos = np.tile(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), (50, 1, 1))

    def same():
        sc = drt.Scene()
        sc.addMaterial((1, 1, 1), -1)
        sc.setGeometry(pos, np.zeros_like(pos), np.zeros((50, 3, 2), np.float32), np.zeros(50, np.int32))
        return sc
    for device in (-1, 0):
        with pytest.raises(drt.DrtError) as e:
            _build(same, 4, 8, device)
        assert e.value.code == drt.ERR_BVH
    with pytest.raises(drt.DrtError) as e:
        _build(make, 2, 1, 0)
    assert e.value.code == drt.ERR_INVALID


def test_image_after_a_device_build_is_the_same_image():
    cam = drt.Camera((3.6, 1.25, 0.0))
    cam.m_Forward_dir = np.array((-1, 0, 0), np.float32)
    images = []
    for device in (-1, 0):
        sc, _ = _build(_file_scene("cornell_box"), 20, 8, device)
        r = drt.Renderer(0)
        r.m_RendererSettings = drt.RendererSettings(ray_bounce_limit=4, max_samples=100)
        r.ResizeBuffer(160, 90)
        r.RenderBatch(cam, sc, 4)
        images.append(r.GetRenderTargetImage())
    assert np.array_equal(images[0], images[1])


# ---------------------------------------------------------------- the zero-sign freedom

def _signed_zero(rng, n):
    return np.where(rng.uniform(size=n) < 0.5, np.float32(0.0), NEG_ZERO).astype(np.float32)


def _zero_sign_queries(osc, hn, where, seed):
    """Queries around the bounds whose zero differs in sign between the two trees (`where`: [k, 2] node, axis; the coordinate of
    every such plane is 0 on its axis): (rays, points, boxes, planes)."""
    rng = np.random.default_rng(seed)
    k = len(where)
    node, axis = where[:, 0], where[:, 1]
    rows = np.arange(k)
    lo, hi = hn["bmin"][node], hn["bmax"][node]

    def in_box(spread):
        p = (lo + rng.uniform(-spread, 1 + spread, (k, 3)) * (hi - lo)).astype(np.float32)
        p[rows, axis] = _signed_zero(rng, k)                                        # exactly on the plane
        return p

    # rays: the generators of tests/ray_query_ref.py (zero direction components of either sign, origins on vertex coordinates), the
    # same with the origin put on a differing plane, rays that graze along such a plane from inside and from beside the box, and
    # rays that start on it and leave it
    n_gen = 800
    o1, d1 = rq.axis_rays(osc, n_gen, rng)
    o2, d2 = rq.axis_rays(osc, n_gen, rng)
    pick = rng.integers(0, k, n_gen)
    o2[np.arange(n_gen), axis[pick]] = _signed_zero(rng, n_gen)
    o3, o4, o5 = in_box(0.0), in_box(0.6), in_box(0.1)
    d3, d4, d5 = (rng.normal(size=(k, 3)).astype(np.float32) for _ in range(3))
    d3[rows, axis] = _signed_zero(rng, k)                                           # along the plane
    d4[rows, axis] = _signed_zero(rng, k)
    o6, d6 = rq.surface_rays(osc, 200, rng)
    target, _ = rq.surface_rays(osc, 400, rng)                                      # and rays from outside aimed at the surface
    o7 = (target + rng.normal(0, 2, (400, 3))).astype(np.float32)
    d7 = (target - o7).astype(np.float32)
    rays = (np.concatenate([o1, o2, o3, o4, o5, o6, o7]), np.concatenate([d1, d2, d3, d4, d5, d6, d7]))
    points = np.concatenate([in_box(0.0), in_box(0.5), o2[:200]])
    # boxes that touch the plane from either side (centre = +-half on the axis), boxes of half 0 on it, boxes across it
    half = (rng.uniform(0, 0.3, (k, 3)) ** 2).astype(np.float32)
    centre = in_box(0.2)
    side = np.where(rng.uniform(size=k) < 0.5, np.float32(1), np.float32(-1))
    touching = centre.copy()
    touching[rows, axis] = side * half[rows, axis]
    flat = half.copy()
    flat[rows, axis] = 0
    boxes = np.concatenate([ov.pack(touching, half), ov.pack(centre, flat), ov.pack(centre, half), ov.pack(centre, 0.0)])
    # the planes themselves (n = +-e_axis, d = +-0), tilted a little, and shifted by one ulp of nothing: d = +-FLT_TRUE_MIN
    e = np.eye(3, dtype=np.float32)[axis] * side[:, None]
    tilt = (e + rng.normal(0, 1e-3, (k, 3))).astype(np.float32)
    planes = np.concatenate([sr.pack(e, _signed_zero(rng, k)), sr.pack(tilt, _signed_zero(rng, k)),
                             sr.pack(e, np.where(rng.uniform(size=k) < 0.5, np.float32(1e-45), np.float32(-1e-45)))])
    return rays, points.astype(np.float32), boxes.astype(np.float32), planes.astype(np.float32)


def _same_arrays(a, b, what):
    """Bit for bit, field by field (floats by their words, so a zero's sign counts; a NaN equals a NaN)."""
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        assert x.shape == y.shape and x.dtype.kind == y.dtype.kind and x.dtype.itemsize == y.dtype.itemsize, (what, i, x.dtype, y.dtype)
        same = x.view(np.uint32) == y.view(np.uint32) if x.dtype == np.float32 else x == y
        if x.dtype == np.float32:
            same |= np.isnan(x) & np.isnan(y)
        assert same.all(), "%s: field %d differs in %d of %d" % (what, i, (~same).sum(), same.size)


@pytest.mark.parametrize("name,cameras", [("zeros", [((0.0, 0.3, 7.0), (0, -0.05, -1)), ((-0.0, 0.2, 0.5), (0.3, 0.1, -1))]),
                                          ("flat", [((9.0, 0.5, 0.0), (-1, -0.05, 0)), ((1.0, 2.0, -0.0), (-1, -0.3, 0)), ((0.5, 0.25, 9.0), (0, 0.05, -1))])])
def test_zero_signs_are_invisible_to_traversal(name, cameras):
    """The claim behind the one freedom: no query and no pixel can tell a tree with the serial loop's zeros from one with the
    order-independent zeros."""
    make = _case_scene(name)
    host, _ = _build(make, 4, 8, -1)
    dev, _ = _build(make, 4, 8, 0)
    assert _assert_same_tree(host, dev, name) > 0
    hn, dn = host.m_BVHNodes, dev.m_BVHNodes
    where = np.concatenate([np.argwhere(_bits(hn[f]) != _bits(dn[f])) for f in ("bmin", "bmax")])
    assert len(where) >= 20                                                         # or this test proves nothing
    osc = bc.oracle_scene(bc.cases()[name].pos).build_bvh(4, 8)
    (org, dirs), points, boxes, planes = _zero_sign_queries(osc, hn, where, 31)
    assert len(org) >= 2000
    answers = []
    for sc in (host, dev):
        r = drt.Renderer(0)
        hits, near, over, sect = r.traceRays(sc, org, dirs, 0.0, np.inf), r.nearest(sc, points), r.overlapBoxes(sc, boxes), r.planeSections(sc, planes)
        images = []
        for position, forward in cameras:
            cam = drt.Camera(position)
            cam.m_Forward_dir = np.array(forward, np.float32)
            r.m_RendererSettings = drt.RendererSettings(ray_bounce_limit=4, max_samples=100)
            r.ResizeBuffer(96, 64)
            r.resetAccumulationBuffer()
            r.RenderBatch(cam, sc, 2)
            images.append(r.GetRenderTargetImage())
        answers.append({"traceRays": (hits.t, hits.prim, hits.u, hits.v), "occluded": (r.occluded(sc, org, dirs, 0.0, np.inf),),
                        "nearest": (near.point, near.d2, near.prim, near.u, near.v, near.side), "overlapBoxes": (over.splits, over.prim),
                        "planeSections": (sect.splits, sect.p, sect.q, sect.prim, sect.code), "images": tuple(images)})
    for kind in answers[0]:
        _same_arrays(answers[0][kind], answers[1][kind], "%s %s" % (name, kind))
    a = answers[0]
    # the queries meet the mesh: hits and misses, lists that are not empty, a picture that is not one colour
    assert (a["traceRays"][1] >= 0).sum() >= 200 and (a["traceRays"][1] < 0).sum() >= 200 and (a["nearest"][2] >= 0).all()
    assert a["overlapBoxes"][0][-1] > 0 and a["planeSections"][0][-1] > 0
    assert any(np.ptp(img[..., :3].reshape(-1, 3), axis=0).max() > 0.02 for img in a["images"])


def test_queries_on_a_device_built_hostile_tree():
    """The tree on the card, and not only the one read back, is the tree: nearest and traceRays on hostile_x4, built on the device,
    against the restatements on the oracle's scene."""
    sc, _ = _build(_case_scene("hostile_x4"), 4, 8, 0)
    osc = bc.oracle_scene(bc.cases()["hostile_x4"].pos).build_bvh(4, 8)
    g = nr.from_oracle(osc)
    rng = np.random.default_rng(41)
    r = drt.Renderer(0)
    points = nr.point_sets(g, 300, rng)
    near = r.nearest(sc, points)
    _same_arrays(tuple(getattr(near, f) for f in nr.Nearest._fields), tuple(nr.nearest(g, points)), "nearest")
    o1, d1 = rq.surface_rays(osc, 200, rng)
    o2, d2 = rq.axis_rays(osc, 100, rng)
    o3, d3 = rq.box_rays(osc, 100, rng)
    org, dirs = np.concatenate([o1, o2, o3]), np.concatenate([d1, d2, d3])
    ref = rq.closest(osc, org, dirs, 0.0, np.inf)
    got = r.traceRays(sc, org, dirs, 0.0, np.inf)
    _same_arrays((got.t, got.prim, got.u, got.v), tuple(ref), "traceRays")
    assert (ref.prim >= 0).sum() >= 50 and (ref.prim < 0).sum() >= 50
