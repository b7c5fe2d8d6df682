"""Restatement of drt_renderer_radiance (include/drt.h): RayGen's path loop (Shaders/RayGen.cuh:88-169, oracle/drt_oracle.c ray_gen)
for one sample per ray, started from make_ray(org, dir) and a given seed state, over the oracle's scene.  No tests of its own.

Vectorised over rays: every trip of the loop is one bounce of every path still alive.  The traversals are tests/ray_query_ref.py's
closest (TraceRay: tmin 0, tmax FLT_MAX) and occluded (RayTest: tmin 0, tmax inf); the closest-hit frame, texel fetch, unit vector
and unit-sphere draws are the oracle's pinned known-answer entries.  Only the shading arithmetic -- sky, tone curve, gamma, the
material model's lobes and the PCG draw of the dielectric -- is restated, in float32 numpy, in the reference's order.
"""
import ctypes as C

import numpy as np

import oracle
from tests import ray_query_ref as rq

F = np.float32
_libm = C.CDLL("libm.so.6")
_libm.sinf.restype = _libm.cosf.restype = C.c_float
_libm.sinf.argtypes = _libm.cosf.argtypes = [C.c_float]


def _dot(a, b):
    return ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]).astype(F)


def _normalize(v):
    inv = (F(1) / np.sqrt(_dot(v, v))).astype(F)
    return (v * inv[:, None]).astype(F)


def _rays6(o, d):
    return np.ascontiguousarray(np.concatenate([o, d], axis=1), F)


def pcg_hash(x):
    """CudaMath/Random.cu:6-11 in uint32."""
    with np.errstate(over="ignore"):
        state = (x.astype(np.uint32) * np.uint32(747796405) + np.uint32(2891336453)).astype(np.uint32)
        word = (((state >> ((state >> np.uint32(28)) + np.uint32(4))) ^ state) * np.uint32(277803737)).astype(np.uint32)
    return ((word >> np.uint32(22)) ^ word).astype(np.uint32)


def random_float(seed):
    """(new seed, (float)seed / 2^32) (Random.cu:13-17)."""
    s = pcg_hash(seed)
    return s, (s.astype(F) / F(4294967296.0)).astype(F)


def sun_frame(st):
    """RayGen.cuh:68-72 with the C library's sinf / cosf, as the renderer and the oracle compute it on the host."""
    sx, sy, cx = _libm.sinf(st.sunlight_dir[0]), _libm.sinf(st.sunlight_dir[1]), _libm.cosf(st.sunlight_dir[0])
    sx, sy, cx = F(sx), F(sy), F(cx)
    sunpos = np.array([sx * (F(1) - sy), sy, cx * (F(1) - sy)], F) * F(100)
    suncol = np.array(st.sunlight_color[:], F) * F(st.sunlight_intensity)
    return sunpos.astype(F), suncol.astype(F)


def sky(dirs, st):
    """SkyModel (RayGen.cuh:54-61)."""
    t = (F(0.5) * (F(1) + _normalize(dirs)[:, 1])).astype(F)
    c = ((F(1) - t)[:, None] * np.ones(3, F) + t[:, None] * np.array(st.sky_color[:], F)).astype(F)
    return (c * c).astype(F)


def _partial(x):
    A, B, Cc, D, E, Fc = F(0.15), F(0.50), F(0.10), F(0.20), F(0.02), F(0.30)
    num = x * (A * x + Cc * B) + D * E
    den = x * (A * x + B) + D * Fc
    return (num / den - E / Fc).astype(F)


def tone(light, exposure):
    """uncharted2_filmic (RayGen.cuh:34-42) with a per-ray exposure."""
    curr = _partial((light * exposure[:, None]).astype(F))
    white = (F(1) / _partial(np.full(3, F(11.2), F))).astype(F)
    return (curr * white).astype(F)


def radiance(osc, org, dirs, seeds, exposure, st):
    """One sample of every ray: float32 [n, 3], the light after the tone curve and gamma of `st` (oracle settings).  The material
    model is osc.material_model, as oracle.render reads it."""
    n = len(org)
    o, d = rq._f32(org).copy(), rq._f32(dirs).copy()
    seed = np.ascontiguousarray(seeds, np.uint32).copy()
    light, thr = np.zeros((n, 3), F), np.ones((n, 3), F)
    mm = tuple(osc.material_model) + (0,) * (4 - len(osc.material_model))
    ext_em, ext_spec, ext_scale, ext_trans = int(mm[0]), int(mm[1]), F(mm[2]), int(mm[3])
    sunpos, suncol = sun_frame(st)
    alive = np.ones(n, bool)
    for i in range(st.ray_bounce_limit + 1):                                       # :88
        idx = np.nonzero(alive)[0]
        if len(idx) == 0:
            break
        hits = rq.closest(osc, o[idx], d[idx], F(0), rq.FLT_MAX)
        seed[idx] += np.uint32(i)                                                  # :91
        miss = hits.prim < 0
        m = idx[miss]                                                              # :99-108
        light[m] = light[m] + (sky(d[m], st) * thr[m]) * F(st.sky_intensity)
        alive[m] = False
        h, sel = idx[~miss], ~miss
        if len(h) == 0:
            continue
        prim, t = hits.prim[sel], hits.t[sel]
        u, v = hits.u[sel], hits.v[sel]
        uvw = np.stack([(F(1) - u) - v, u, v], axis=1).astype(F)                   # Intersection.cu:31
        pos, nrm, front = oracle.kat_closest_hit(_rays6(o[h], d[h]), t, osc.tris["face_n"][prim])
        mat = osc.tris["material"][prim]
        ext = osc.mats_ext[mat]
        if ext_em:                                                                 # opt-in emissive term
            light[h] = light[h] + (ext["emissive"].astype(F) * ext_scale) * thr[h]
        tex = osc.mats["albedo_tex"][mat]
        alb = osc.mats["albedo"][mat].astype(F)
        for ti in np.unique(tex[tex >= 0]):                                        # :111-118
            s = np.nonzero(tex == ti)[0]
            alb[s] = oracle.kat_texpixel(osc.textures[int(ti)], rq._interp_uv(osc.tris["uv"][prim[s]], uvw[s]))
        thr[h] = thr[h] * alb
        origin = (pos + nrm * F(0.001)).astype(F)                                  # :121
        if st.enable_sunlight:                                                     # :124-128
            vec, seed[h] = oracle.kat_unitvec(seed[h])
            occ = rq.occluded(osc, origin, (sunpos + vec * F(1.5)).astype(F), F(0), F(np.inf))
            lit = h[~occ]
            light[lit] = light[lit] + suncol * thr[lit]
        if i == st.ray_bounce_limit:                                               # nothing after the last bounce is read
            alive[h] = False
            continue
        glass = np.zeros(len(h), bool) if not ext_trans else ext["transmission"] != 0
        mirror = ~glass & (ext["metallic"] != 0) if ext_spec else np.zeros(len(h), bool)
        new_o, new_d = origin.copy(), np.zeros((len(h), 3), F)
        g = np.nonzero(glass)[0]
        if len(g):                                                                 # Random.cu:26-40
            vg, ng = _normalize(d[h[g]]), nrm[g]
            cos_t = np.fmin(_dot(vg * F(-1), ng), F(1)).astype(F)
            ior = ext["refractive_index"][g].astype(F)
            ri = np.where(front[g] != 0, F(1) / ior, ior).astype(F)
            sin_t = np.sqrt(F(1) - cos_t * cos_t).astype(F)
            refl = ri * sin_t > F(1)
            r0 = ((F(1) - ri) / (F(1) + ri)).astype(F)
            r0 = (r0 * r0).astype(F)
            om = (F(1) - cos_t).astype(F)
            schlick = (r0 + (F(1) - r0) * (((om * om) * (om * om)) * om)).astype(F)
            draw = np.nonzero(~refl)[0]
            sg = seed[h[g]]
            sg[draw], rf = random_float(sg[draw])
            seed[h[g]] = sg
            refl[draw] = schlick[draw] > rf
            mir = (vg - ng * (F(2) * _dot(vg, ng))[:, None]).astype(F)
            perp = ((vg + ng * cos_t[:, None]) * ri[:, None]).astype(F)
            par = (ng * (-np.sqrt(np.abs(F(1) - _dot(perp, perp))))[:, None]).astype(F)
            new_d[g] = np.where(refl[:, None], mir, (perp + par).astype(F))
            new_o[g] = np.where(refl[:, None], origin[g], (pos[g] - ng * F(0.001)).astype(F))
        rest = np.nonzero(~glass)[0]
        if len(rest):
            fuzz, seed[h[rest]], _ = oracle.kat_unitsphere(seed[h[rest]])
            nr = nrm[rest]
            new_d[rest] = (nr + fuzz).astype(F)                                    # :133-134
            mi = np.nonzero(mirror[rest])[0]
            if len(mi):                                                            # opt-in mirror lobe
                vm = _normalize(d[h[rest[mi]]])
                refl_d = (vm - nr[mi] * (F(2) * _dot(vm, nr[mi]))[:, None]).astype(F)
                dm = (refl_d + fuzz[mi] * ext["roughness"][rest[mi]].astype(F)[:, None]).astype(F)
                new_d[rest[mi]] = dm
                alive[h[rest[mi][~(_dot(dm, nr[mi]) > 0)]]] = False                # scattered into the surface: absorbed
        o[h], d[h] = new_o, new_d
    if st.tone_mapping:                                                            # :165-169
        light = tone(light, np.ascontiguousarray(exposure, F))
    if st.gamma_correction:
        light = np.sqrt(light).astype(F)
    return light
