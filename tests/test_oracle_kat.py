"""Pins the oracle's leaf arithmetic against the REFERENCE's own compiled functions.

tests/golden/kat_ref.npz was produced by oracle/_ref/ref_kat (the reference's Random.cu, Bounds.cu,
Intersection.cu, Camera.cu, Texture.cu compiled in place; recipe oracle/Makefile, generator
tests/golden/make_kat_golden.py).  Everything here is bit-exact: these functions decide control flow
(rejection sampling, hit/miss), so one ulp is a different image.
"""
import numpy as np
import pytest

import oracle


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_pcg_hash_matches_reference(kat_golden):
    g = kat_golden
    assert np.array_equal(oracle.kat_pcg(g["seeds"]), g["pcg"])


def test_pcg_hash_independent_bigint():
    # independent restatement with Python integers (CudaMath/Random.cu:6-11)
    def pcg(v):
        state = (v * 747796405 + 2891336453) & 0xFFFFFFFF
        word = (((state >> ((state >> 28) + 4)) ^ state) * 277803737) & 0xFFFFFFFF
        return (word >> 22) ^ word
    vals = [0, 1, 2, 0xFFFFFFFF, 0x80000000, 123456789, 1920 * 1080 * 8]
    assert [int(x) for x in oracle.kat_pcg(vals)] == [pcg(v) for v in vals]


def test_random_float_sequence(kat_golden):
    g = kat_golden
    out, end = oracle.kat_randfloat(12345, 1024)
    assert np.array_equal(bits(out), bits(g["randfloat"]))
    assert end == int(g["randfloat_seed_end"])
    assert out.min() >= 0.0 and out.max() <= 1.0          # range is [0,1] INCLUSIVE


def test_random_float_can_return_one():
    # (float)seed rounds up to 2^32 for seed >= 2^32-128: the division then yields exactly 1.0f
    # find a preimage-free check: apply the float conversion rule directly
    assert np.float32(np.uint32(0xFFFFFFFF)) / np.float32(4294967296.0) == np.float32(1.0)


@pytest.mark.parametrize("name,width", [("unitvec", 3), ("unitsphere", 3), ("unitdisk", 2)])
def test_random_vectors(kat_golden, name, width):
    g = kat_golden
    res = getattr(oracle, "kat_" + name)(g["seeds"])
    assert np.array_equal(bits(res[0]), bits(g[name])), name
    assert np.array_equal(res[1], g[name + "_seed"]), name + " seed stream desynchronised"


def test_unit_sphere_rejection_is_rounding_noise(kat_golden):
    # normalise-then-reject (Random.cu:50-58): the loop runs ~3 times on average, not once
    _, _, iters = oracle.kat_unitsphere(kat_golden["seeds"])
    assert iters.min() >= 1 and 2.0 < iters.mean() < 4.0


def test_slab_matches_reference(kat_golden):
    g = kat_golden
    out = oracle.kat_slab(g["slab_rays"], g["slab_boxes"])
    assert np.array_equal(bits(out), bits(g["slab"]))
    assert (out >= 0).sum() > 1000 and (out == -1).sum() > 500      # both branches exercised


def test_slab_nan_lane_device_semantics():
    """Origin on a slab plane with a zero direction component: (pMin-o)*invDir = 0*inf = NaN.
    CUDA device fminf/fmaxf return the non-NaN operand (Bounds.cu:23-24 "switched order ... to guard
    NaNs"); helper_math.cuh:58-66's host fallback does not, so this case is hand-derived, not
    compared with ref_kat."""
    ray = np.array([[0.0, 0.5, 0.5, 0.0, 0.0, 1.0]], np.float32)        # origin x == pMin.x, dir.x == 0
    box = np.array([[0.0, 0.0, 1.0, 1.0, 1.0, 2.0]], np.float32)
    # x slab: t0 = NaN, t1 = +inf -> tmin = inf?? no: fminf(NaN, inf) = inf, fmaxf(inf, NaN) = inf
    # y slab: dir 0 -> t0 = -inf, t1 = +inf; z slab: t0 = 0.5, t1 = 1.5
    # tenter = max(inf, -inf, 0.5) = inf ; texit = min(inf, inf, 1.5) = 1.5 -> miss
    assert oracle.kat_slab(ray, box)[0] == -1.0
    ray2 = np.array([[1.0, 0.5, 0.5, 0.0, 0.0, 1.0]], np.float32)       # origin x == pMax.x
    # x slab: t0 = (0-1)*inf = -inf, t1 = 0*inf = NaN -> tmin = -inf, tmax = fmaxf(NaN,-inf) = -inf
    # texit = min(-inf, inf, 1.5) = -inf < 0 -> miss
    assert oracle.kat_slab(ray2, box)[0] == -1.0


def test_intersection_matches_reference(kat_golden):
    g = kat_golden
    tuvw, hit = oracle.kat_intersect(g["isect_rays"], g["isect_tris"])
    assert np.array_equal(hit, g["isect_hit"])
    assert np.array_equal(bits(tuvw[:, 0]), bits(g["isect_tuvw"][:, 0]))
    h = hit.astype(bool)
    assert np.array_equal(bits(tuvw[h]), bits(g["isect_tuvw"][h]))
    assert h.sum() > 3000 and (~h).sum() > 200
    # edge rules (Intersection.cu:19,24,28): u==0, v==0, u+v==1 and vertices are hits; parallel/behind are not
    assert hit[256:304].all() and not hit[304:320].any()


def test_closest_hit_matches_reference(kat_golden):
    g = kat_golden
    pos, nrm, front = oracle.kat_closest_hit(g["ch_rays"], g["ch_t"], g["ch_fn"])
    assert np.array_equal(front, g["ch_front"])
    assert np.array_equal(bits(pos), bits(g["ch_pos"]))
    assert np.array_equal(bits(nrm), bits(g["ch_normal"]))
    assert front[:64].all()                      # dot == 0: the strict > keeps the face normal (ClosestHit.cuh:17)
    assert 0.3 < front.mean() < 0.7


def test_triangle_centroid_matches_reference(kat_golden):
    """Triangle.cuh:11 (p0 + p1 + p2) / 3 -- the value the SAH builder bins by."""
    g = kat_golden
    p = g["isect_tris"].reshape(-1, 3, 3)
    n = len(p)
    z3, z2 = np.zeros((n * 3, 3), np.float32), np.zeros((n * 3, 2), np.float32)
    tris = np.zeros(n, oracle.TRI_DTYPE)
    pos = np.ascontiguousarray(p.reshape(-1, 3), np.float32)
    nrm = np.ascontiguousarray(z3 + np.float32([0, 0, 1]), np.float32)
    mat = np.zeros(n, np.int32)
    oracle.lib().o_build_triangles(pos.ctypes.data, nrm.ctypes.data, z2.ctypes.data, mat.ctypes.data, n, tris.ctypes.data)
    assert np.array_equal(bits(tris["centroid"]), bits(g["centroid"]))


def test_node_surface_area_matches_reference(kat_golden):
    g = kat_golden
    sa = oracle.kat_surface_area(g["slab_boxes"], g["sa_count"])
    assert np.array_equal(bits(sa), bits(g["surfacearea"]))
    assert (sa[g["sa_count"] == 0] == 0).all() and (sa[g["sa_count"] > 0] != 0).any()


def test_get_ray_matches_reference(kat_golden):
    g = kat_golden
    for k, cam in enumerate(g["cams"]):
        c = oracle.default_camera(exposure=float(cam[0]), vfov_rad=float(cam[1]), defocus_angle=float(cam[2]),
                                  focus_dist=float(cam[3]), position=[float(v) for v in cam[4:7]],
                                  forward=[float(v) for v in cam[7:10]])
        rays, seeds = oracle.kat_getray(c, float(cam[10]), float(cam[11]), g["uv"], g["seeds"])
        assert np.array_equal(seeds, g["getray_seed"][k]), "camera %d seed stream" % k
        assert np.array_equal(bits(rays), bits(g["getray"][k])), "camera %d" % k


def test_texture_fetch_matches_reference(kat_golden):
    g = kat_golden
    assert np.array_equal(bits(oracle.kat_texpixel(g["tex3"], g["tex_uv"])), bits(g["texpixel3"]))
    assert np.array_equal(bits(oracle.kat_texpixel(g["tex4"], g["tex_uv"])), bits(g["texpixel4"]))
    assert np.array_equal(bits(oracle.kat_texalpha(g["tex4"], g["tex_uv"])), bits(g["texalpha4"]))
    assert np.array_equal(bits(oracle.kat_texalpha(g["tex3"], g["tex_uv"])), bits(g["texalpha3"]))
    assert (g["texalpha3"] == 1).all()                      # <4 channels: opaque (Texture.cu:62-63)


def _kat3():
    """tests/golden/kat_ref3.json and the inputs its generator (tests/golden/make_kat_golden3.py) ran the reference binary on."""
    import importlib.util
    import json
    import os
    from tests.scenes import ROOT
    gen = os.path.join(ROOT, "tests", "golden", "make_kat_golden3.py")
    spec = importlib.util.spec_from_file_location("make_kat_golden3", gen)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(os.path.join(ROOT, "tests", "golden", "kat_ref3.json")) as f:
        return mod, mod.inputs(), json.load(f)


def _equals_stored(mod, got, want, what):
    """Bit for bit: every byte through its SHA-256; on a mismatch, the first stored values say where."""
    s = mod.summary(got)
    assert (s["dtype"], s["shape"]) == (want["dtype"], want["shape"]), what
    assert s["head_bits"] == want["head_bits"], "%s: first difference at element %d" % (
        what, next(i for i, (a, b) in enumerate(zip(s["head_bits"], want["head_bits"])) if a != b))
    assert s["sha256"] == want["sha256"], "%s: differs beyond the first %d elements" % (what, len(want["head_bits"]))


def test_live_reference_binary_when_present(kat_golden):
    """50 000 seeds through the reference's randomInUnitSphere: its outputs are pinned in tests/golden/kat_ref3.json
    (tests/golden/make_kat_golden3.py); where oracle/_ref/ref_kat is built, the binary itself is re-run on the same seeds."""
    from oracle import ref_kat as rk
    mod, x, g = _kat3()
    seeds = x["sphere_seeds"]
    assert len(np.unique(seeds)) > 49000                          # the hash spreads them
    v, s, _ = oracle.kat_unitsphere(seeds)
    _equals_stored(mod, np.asarray(v, "<f4"), g["sphere_v"], "unit-sphere vectors")
    _equals_stored(mod, np.asarray(s, "<u4"), g["sphere_seed_end"], "seeds after the draw")
    if rk.available():
        rv, rs = rk.unitsphere(seeds)
        assert np.array_equal(bits(v), bits(rv)) and np.array_equal(s, rs)


def test_sphere_accept_shortcut():
    """The HIP kernels test  dot(p,p) < 1  instead of  len*len < 1, len = sqrtf(dot(p,p))  (Random.cu:54-55).
    Equivalence for every float the dot product can take: all of [0.5, 2) exhaustively (the candidates are
    normalised, so dot(p,p) is within a few ulp of 1), plus a random sample of the rest and the specials."""
    one = np.float32(1)
    lo, hi = np.float32(0.5).view(np.uint32), np.float32(2.0).view(np.uint32)
    d = np.arange(lo, hi, dtype=np.uint32).view(np.float32)
    length = np.sqrt(d)
    assert np.array_equal((length * length) < one, d < one)
    rng = np.random.default_rng(3)
    d = rng.integers(0, 0x7F800001, 2_000_000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    d = np.concatenate([d, np.array([0.0, np.inf, np.nan, 1.0, np.nextafter(np.float32(1), np.float32(0))], np.float32)])
    with np.errstate(invalid="ignore", over="ignore"):
        length = np.sqrt(d)
        assert np.array_equal((length * length) < one, d < one)


@pytest.mark.parametrize("name,W,H,spp,depth,pose,want", [
    ("cornell_box", 256, 256, 1, 4, None, (3.69, 14.5, 7.35, 89.7)),
    ("cornell_box", 480, 270, 8, 8, None, (3.26, 11.2, 5.62, 69.6)),
    ("cornell_box", 480, 270, 8, 8, ((0, 2, 5), (0, 0, -1)), (1.22, 0.72, 0.44, 4.1)),
    ("suzanne_plane", 480, 270, 8, 2, None, (1.53, 6.2, 4.74, 13.6)),
    ("dense_monkey", 480, 270, 16, 2, None, (1.20, 9.3, 8.44, 12.4)),
    ("room", 480, 270, 2, 16, None, (11.7, 114.8, 85.4, 425.5)),
    ("cs16_dust", 320, 180, 2, 2, ((0, 2, 5), (0, 0, -1)), (2.62, 70.0, 63.4, 89.7))])
def test_work_per_sample_matches_the_figures_measured_on_the_reference_sources(name, W, H, spp, depth, pose, want):
    """BASELINE.md section 2 / SURVEY.md 8(d): rays, node visits, interior visits and triangle tests per sample that the
    survey measured by running the reference's OWN traversal / shading sources on the CPU.  They pin the composition
    (traversal order, culls, path termination) statistically: a different pop rule or cull moves them by far more than
    the 1.5 % allowed here for the lower resolution and for the survey's compiler drawing x, y, z in the other order."""
    from tests.scenes import SCENES, scene_path
    _, pos, fwd, _ = SCENES[name]
    if pose:
        pos, fwd = pose
    sc = oracle.Scene.load_glb(scene_path(name)).build_bvh(20, 8)
    _, _, c = oracle.render(sc, oracle.default_camera(position=pos, forward=fwd), oracle.default_settings(ray_bounce_limit=depth),
                            W, H, 1, spp, want_counters=True)
    d = c.as_dict()
    n = d["samples"]
    got = (d["rays"] / n, d["node_visits"] / n, d["inner_visits"] / n, d["tri_tests"] / n)
    for g, w in zip(got, want):
        assert abs(g - w) <= 0.015 * w + 0.006, (got, want)


def test_remaining_reference_leaf_functions(kat_golden):
    """tests/golden/kat_ref2.npz (tests/golden/make_kat_golden2.py): Interval::surrounds, Miss and Bounds3f::getCentroid from the
    reference's own sources compiled here -- the last of its functions that build without thrust."""
    import os
    from tests.scenes import ROOT
    g = np.load(os.path.join(ROOT, "tests", "golden", "kat_ref2.npz"))
    assert np.array_equal(oracle.kat_surrounds(g["iv"]), g["surrounds"])
    assert g["surrounds"][:8].tolist() == [0, 0, 1, 1, 0, 0, 0, 0]          # (-1, FLT_MAX) around -1, FLT_MAX, 0, -0, inf, -inf, NaN, < -1
    col, t, has_prim, front = oracle.kat_miss(g["miss_rays"], g["miss_color"])
    assert np.array_equal(bits(col), bits(g["miss_out_color"])) and np.array_equal(bits(t), bits(g["miss_t"]))
    assert np.array_equal(has_prim, g["miss_has_prim"]) and np.array_equal(front, g["miss_front"]) and not has_prim.any() and (t == -1).all()
    assert np.array_equal(bits(oracle.kat_bounds_centroid(g["boxes"])), bits(g["boundscentroid"]))
    # random intervals and huge boxes: the reference's outputs pinned in kat_ref3.json (tests/golden/make_kat_golden3.py)
    mod, x, g3 = _kat3()
    iv, boxes = x["iv"], x["boxes"]
    _equals_stored(mod, np.asarray(oracle.kat_surrounds(iv), "<i4"), g3["surrounds"], "Interval::surrounds")
    _equals_stored(mod, np.asarray(oracle.kat_bounds_centroid(boxes), "<f4"), g3["boundscentroid"], "Bounds3f::getCentroid")
    from oracle import ref_kat as rk
    if rk.available():                                       # build container: the reference binary itself, same inputs
        assert np.array_equal(oracle.kat_surrounds(iv), rk.surrounds(iv))
        assert np.array_equal(bits(oracle.kat_bounds_centroid(boxes)), bits(rk.boundscentroid(boxes)))


def tie_scene():
    """Two coplanar triangles in two leaves whose boxes a straight-down ray enters at the same distance and which it hits at
    the same t -- every number dyadic, so 'the same' is exact:  ray o = (-0.5, -0.5, 5), d = (0, 0, -1);
    A = (-2,-2,.5) (2,-2,.5) (-2,2,.5): det 16, t = 72/16 = 4.5;  B = (-4,-4,.5) (4,-4,.5) (-4,4,.5): det 64, t = 288/64 = 4.5;
    both (flat) boxes are entered at 4.5.  Hand-derived from BVHTraversal.cuh:51,63-70: d1 > d2 is false, so child 2 is pushed
    first and child 1 is VISITED first; its triangle sets closest.t = 4.5; child 2 survives `closest.t < d` (4.5 < 4.5 is
    false) and its triangle fails `t < closest.t`: the triangle of child 1 wins."""
    pos = np.float32([[[-2, -2, .5], [2, -2, .5], [-2, 2, .5]], [[-4, -4, .5], [4, -4, .5], [-4, 4, .5]]])
    nrm = np.tile(np.float32([0, 0, 1]), (2, 3, 1))
    materials = [((1.0, 0.0, 0.0), -1), ((0.0, 1.0, 0.0), -1)]      # A red, B green
    return pos, nrm, np.zeros((2, 3, 2), np.float32), np.int32([0, 1]), materials


def tie_winner_albedo(nodes, tris_material, materials):
    root = nodes[-1]
    assert len(nodes) == 3 and not root["is_leaf"]
    c1, c2 = nodes[int(root["child1"])], nodes[int(root["child2"])]
    assert c1["is_leaf"] and c2["is_leaf"] and c1["prim_count"] == c2["prim_count"] == 1
    return np.float32(materials[int(tris_material[int(c1["prim_start"])])][0])


def test_equal_distances_and_equal_hits_resolve_as_in_the_reference():
    """Oracle side of the hand-derived traversal KAT (see tie_scene): debug view ALBEDO shows the winner's colour."""
    pos, nrm, uv, mat, materials = tie_scene()
    tris = np.zeros(2, oracle.TRI_DTYPE)
    a = [np.ascontiguousarray(x, np.float32) for x in (pos.reshape(-1, 3), nrm.reshape(-1, 3), uv.reshape(-1, 2))]
    oracle.lib().o_build_triangles(a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, mat.ctypes.data, 2, tris.ctypes.data)
    osc = oracle.Scene(tris, materials, []).build_bvh(1, 8)
    want = tie_winner_albedo(osc.nodes, osc.tris["material"], materials)
    cam = oracle.default_camera(position=(-0.5, -0.5, 5.0), forward=(0, 0, -1), vfov_rad=0.0)     # zero field of view: every pixel's ray is exactly (o, d)
    img, _, _ = oracle.render(osc, cam, oracle.default_settings(render_mode=1, debug_mode=0, ray_bounce_limit=0, tone_mapping=0, gamma_correction=0), 4, 4, 1, 1)
    assert np.array_equal(img[..., :3], np.broadcast_to(want, (4, 4, 3))), (img[0, 0], want)
    # and the other way round when the near box differs: lift A's plane a little -> A is closer, A wins whatever the order
    pos2 = pos.copy(); pos2[0, :, 2] = 0.75
    oracle.lib().o_build_triangles(np.ascontiguousarray(pos2.reshape(-1, 3)).ctypes.data, a[1].ctypes.data, a[2].ctypes.data, mat.ctypes.data, 2, tris.ctypes.data)
    osc2 = oracle.Scene(tris, materials, []).build_bvh(1, 8)
    img2, _, _ = oracle.render(osc2, cam, oracle.default_settings(render_mode=1, debug_mode=0, ray_bounce_limit=0, tone_mapping=0, gamma_correction=0), 4, 4, 1, 1)
    assert np.array_equal(img2[0, 0, :3], np.float32([1, 0, 0]))
