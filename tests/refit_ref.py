"""Restatement of the BVH refit (include/drt.h drt_scene_refit / drt_renderer_refit) for the tests.  No tests of its own.

Triangles: the oracle's o_build_triangles (Scene.cu:272-302) on the load-order streams, gathered by the scene's triangle order.
Nodes: a bottom-up float32 pass over the tree's topology (drt_scene_get_nodes): a node's exact extent lo / hi is the min / max over
the vertices of its subtree (an interior node's: min / max of its children's exact lo / hi), with -0 < +0 in both; the stored box
is bmin = lo, bmax = lo + (hi - lo), as set_bounds (BVHBuilder.cuh:48-95) stores it.  Min and max run on order-preserving
integer keys of the floats, which gives that order of the zeros and makes the reduction order irrelevant.
"""
import numpy as np

import oracle

FLT_MAX = np.float32(np.finfo(np.float32).max)


def streams(tris):
    """(pos [n, 3, 3], nrm [n, 3, 3], uv [n, 3, 2], mat [n]) of a product triangle array (Scene.m_PrimitivesBuffer): the load-order
    streams when taken before a build."""
    v = tris["vertex"]
    return (np.ascontiguousarray(v["position"], np.float32), np.ascontiguousarray(v["normal"], np.float32),
            np.ascontiguousarray(v["uv"], np.float32), np.ascontiguousarray(tris["material"], np.int32))


def triangles(pos, nrm, uv, mat, order=None):
    """oracle.TRI_DTYPE records of the load-order streams, gathered by `order` (Scene.triangleOrder()) when given."""
    n = len(mat)
    out = np.zeros(n, oracle.TRI_DTYPE)
    a = [np.ascontiguousarray(x, np.float32) for x in (np.reshape(pos, (-1, 3)), np.reshape(nrm, (-1, 3)), np.reshape(uv, (-1, 2)))]
    m = np.ascontiguousarray(mat, np.int32)
    oracle.lib().o_build_triangles(a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, m.ctypes.data, n, out.ctypes.data)
    return out if order is None else out[np.asarray(order)]


def _key(f):
    b = np.ascontiguousarray(f, np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def _float(k):
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def nodes(tree, p):
    """`tree` (product NODE_DTYPE, root last) with every bmin / bmax refitted to the vertex positions p [n, 3, 3] (triangle order)."""
    out = tree.copy()
    n_nodes = len(tree)
    leaf = tree["is_leaf"] != 0
    lo = np.empty((n_nodes, 3), np.uint32)
    hi = np.empty((n_nodes, 3), np.uint32)
    lo[:], hi[:] = _key(FLT_MAX), _key(-FLT_MAX)
    keys = _key(np.reshape(p, (-1, 3, 3)))
    tri_lo, tri_hi = keys.min(axis=1), keys.max(axis=1)
    for i in np.nonzero(leaf)[0]:
        s, c = int(tree["prim_start"][i]), int(tree["prim_count"][i])
        if c:
            lo[i], hi[i] = tri_lo[s:s + c].min(axis=0), tri_hi[s:s + c].max(axis=0)
    inner = np.nonzero(~leaf)[0]
    c1, c2 = tree["child1"][inner], tree["child2"][inner]
    height = np.zeros(n_nodes, np.int64)
    while True:                                  # height = distance to the deepest leaf below, by relaxation
        h = 1 + np.maximum(height[c1], height[c2])
        if np.array_equal(h, height[inner]):
            break
        height[inner] = h
    for hh in range(1, int(height.max()) + 1 if len(inner) else 1):
        sel = height[inner] == hh
        i, a, b = inner[sel], c1[sel], c2[sel]
        lo[i], hi[i] = np.minimum(lo[a], lo[b]), np.maximum(hi[a], hi[b])
    lo_f, hi_f = _float(lo), _float(hi)
    out["bmin"] = lo_f
    out["bmax"] = lo_f + (hi_f - lo_f)
    return out


def oracle_tree(tree):
    """The product's nodes as oracle.NODE_DTYPE."""
    out = np.zeros(len(tree), oracle.NODE_DTYPE)
    for f in oracle.NODE_DTYPE.names:
        out[f] = tree[f]
    return out
