"""-m gpu: the grid of a path_pool launch that shares the device (csrc/pool_share.hpp; drt_renderer_set_frames_in_flight).  The share is
1 / min(hint, launches that reliably run side by side), the second from DRT_POOL_SHARE_MAX or from the hardware queue count: the hint
below it, half of it from there on (GPU_MAX_HW_QUEUES as the process started with it; DRT_POOL_HW_QUEUES stands in for it per renderer).
What the launcher does with it is read from DRT_POOL_VERBOSE's line; whatever grid comes out, every build gives the oracle's bits --
sample ids are static per workgroup up to grid x P and drawn from the counters above that, so the grid moves that border -- and
four renderers that render side by side on four streams each give the image they give alone.

96 x 64, 2 frames, depth 4 = 12 288 samples: 12 workgroups of work with the default pool, 192 with pools of 64 paths (DRT_POOL_PATHS=64),
which is where a share of the slots is smaller than the work."""
import math
import os
import re

import numpy as np
import pytest

import oracle
from tests.scenes import SCENES, bits, scene_path

pytestmark = pytest.mark.gpu
drt = pytest.importorskip("dustraytracer_amd")

W, H, FRAMES, DEPTH = 96, 64, 2, 4
WORK = (W // 8) * (H // 8) * FRAMES        # workgroups of work at 64 paths per pool: one 8 x 8 tile of one frame each

# name: (scene, sunlight, environment, material model or None) -- FLAGS 0, 2, 4 of the lds-scene kernel, its deep-tree build, an
# hbm-scene build and a material-model build (path_pool<16>, the other translation unit: emissive cubes and a mirror sphere)
CASES = {
    "lean": ("cornell_box", 0, {}, None),
    "sun": ("sunshadow_test", 1, {}, None),
    "alpha": ("uv_texture_test", 0, {}, None),
    "deep": ("room", 0, {"DRT_POOL_STACK_LDS": "1"}, None),
    "hbm": ("cs16_dust", 0, {}, None),
    "materials": ("emissive_test", 0, {}, (1, 1, 2.5)),
}
PROCESS_QUEUES = int(os.environ.get("GPU_MAX_HW_QUEUES") or 0)        # what the library's first renderer of the process reads
# (hint, DRT_POOL_SHARE_MAX, DRT_POOL_HW_QUEUES; None = not in the environment)
SHARES = [(1, None, None), (2, None, None), (3, None, "4"), (4, None, "4"), (4, None, "8"), (64, None, None), (64, None, "8"), (64, None, "128"),
          (64, "64", None), (4, "1", "8"), (64, "5", "4")]
_scenes, _refs = {}, {}


def _pair(name):
    if name not in _scenes:
        sc = drt.Scene()
        sc.loadGLTFmodel(scene_path(name))
        b = drt.BVHBuilder()
        b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
        b.buildIterative(sc)
        _scenes[name] = (sc, oracle.Scene.load_glb(scene_path(name)).build_bvh(20, 8))
    return _scenes[name]


def _cameras(name):
    _, pos, fwd, _ = SCENES[name]
    cam = drt.Camera(pos)
    cam.m_Forward_dir = np.array(fwd, np.float32)
    return cam, oracle.default_camera(position=pos, forward=fwd)


def _reference(name, sun, model=None, frames=FRAMES):
    """The oracle's image of a case: computed once, shared, never written to."""
    key = (name, sun, model, frames)
    if key not in _refs:
        o = oracle.default_settings(ray_bounce_limit=DEPTH, enable_sunlight=sun)
        osc = _pair(name)[1]
        if model:
            osc.material_model = model
        try:
            ref, acc, _ = oracle.render(osc, _cameras(name)[1], o, W, H, 1, frames)
        finally:
            osc.material_model = (0, 0, 1.0)
        ref.setflags(write=False)
        acc.setflags(write=False)
        _refs[key] = (ref, acc)
    return _refs[key]


def _cap(hint, share_max, queues):
    """pool_share.hpp's rule, restated: the override, else the hint below the queue count, else half the queues (none given: 4)."""
    if share_max:
        return int(share_max)
    q = int(queues) if queues else PROCESS_QUEUES
    q = q if q > 0 else 4
    return hint if hint < q else max(1, q // 2)


def _renderer(env):
    """A renderer created under `env` (a value of None: the variable is absent).  The knobs are read at creation; the HIP runtime
    has read its own variables before (device_count() first), so what this sets reaches the library alone."""
    assert drt.device_count() > 0
    env = dict(env, DRT_KERNEL="path_pool")
    old = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        return drt.Renderer(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _launch_lines(text):
    return [tuple(int(v) for v in m) for m in re.findall(r"path_pool launch: (\d+) workgroups of (\d+) slots \(frames in flight (\d+), share max (\d+)\)", text)]


@pytest.mark.parametrize("share", SHARES, ids=lambda s: "hint%s-max%s-queues%s" % s)
@pytest.mark.parametrize("case", sorted(CASES))
def test_every_share_gives_the_oracles_bits(case, share, capfd):
    name, sun, env, model = CASES[case]
    hint, share_max, queues = share
    r = _renderer(dict(env, DRT_POOL_PATHS="64", DRT_POOL_VERBOSE="1", DRT_POOL_SHARE_MAX=share_max, DRT_POOL_HW_QUEUES=queues))
    r.m_RendererSettings = drt.RendererSettings(ray_bounce_limit=DEPTH, enableSunlight=sun)
    if model:
        r.setMaterialModel(*model)
    r.setFramesInFlight(hint)
    r.ResizeBuffer(W, H)
    capfd.readouterr()
    r.RenderBatch(_cameras(name)[0], _pair(name)[0], FRAMES)       # (raises unless the status is DRT_OK)
    lines = _launch_lines(capfd.readouterr().err)
    assert " paths=64 " in r.kernelInfo() and ("path_pool<materials" in r.kernelInfo()) == bool(model), r.kernelInfo()
    assert len(lines) == 1, lines
    grid, slots, seen_hint, cap = lines[0]
    assert (seen_hint, cap) == (hint, _cap(hint, share_max, queues)), lines
    sharers = min(hint, cap)
    assert grid == (min(WORK, slots) if sharers == 1 else min(WORK, slots, math.ceil(slots / sharers))), lines
    ref, acc = _reference(name, sun, model)
    assert np.array_equal(bits(r.GetRenderTargetImage()), bits(ref)), "%s, %r: image differs from the oracle's" % (case, share)
    assert np.array_equal(bits(r.GetAccumulationBuffer()), bits(acc)), "%s, %r: accumulation buffer differs" % (case, share)


def test_the_share_bites_only_where_it_should(capfd):
    """The same launch under three caps: a hint of 64 honoured in full leaves it a 64th of the slots -- fewer workgroups than it has
    work for -- and a cap of 3 leaves it a third, which is more than its work, as it is for the default pool's 12 workgroups."""
    grids = {}
    for cap, paths in (("64", "64"), ("3", "64"), ("3", None)):
        r = _renderer({"DRT_POOL_PATHS": paths, "DRT_POOL_VERBOSE": "1", "DRT_POOL_SHARE_MAX": cap})
        r.m_RendererSettings = drt.RendererSettings(ray_bounce_limit=DEPTH)
        r.setFramesInFlight(64)
        r.ResizeBuffer(W, H)
        capfd.readouterr()
        r.RenderBatch(_cameras("cornell_box")[0], _pair("cornell_box")[0], FRAMES)
        (grid, slots, _, _), = _launch_lines(capfd.readouterr().err)
        grids[(cap, paths)] = (grid, slots)
    grid, slots = grids[("64", "64")]
    assert grid == math.ceil(slots / 64) < WORK, grids
    grid, slots = grids[("3", "64")]
    assert grid == WORK <= math.ceil(slots / 3), grids
    grid, slots = grids[("3", None)]
    assert grid == math.ceil(W * H * FRAMES / 1024) <= math.ceil(slots / 3), grids


@pytest.mark.parametrize("hint,share_max", [(4, None), (64, "64")], ids=["hint4", "hint64-max64"])
def test_one_frame_launches_and_a_shard_match_the_oracle(hint, share_max, capfd):
    """A launch of one frame resolves inline (no sample buffer, no resolve kernel) and a sharded renderer traces only its stripes
    (setShard(8, 1, 3): rows 8-15, 32-39, 56-63): both are sized by the same rule and both give the oracle's bits -- under a hint of 4,
    and under a 64th of the slots, which is fewer workgroups than either has work for."""
    cam, sc = _cameras("cornell_box")[0], _pair("cornell_box")[0]
    env = {"DRT_POOL_PATHS": "64", "DRT_POOL_VERBOSE": "1", "DRT_POOL_SHARE_MAX": share_max, "DRT_POOL_HW_QUEUES": "4"}
    one = _renderer(env)
    one.m_RendererSettings = drt.RendererSettings(ray_bounce_limit=DEPTH)
    one.setFramesInFlight(hint)
    one.ResizeBuffer(W, H)
    capfd.readouterr()
    one.RenderBatch(cam, sc, 1)
    (grid, slots, _, cap), = _launch_lines(capfd.readouterr().err)
    assert cap == _cap(hint, share_max, "4") and grid == min(WORK // FRAMES, math.ceil(slots / min(hint, cap))), (grid, slots, cap)
    ref, acc = _reference("cornell_box", 0, None, 1)
    assert np.array_equal(bits(one.GetRenderTargetImage()), bits(ref))
    assert np.array_equal(bits(one.GetAccumulationBuffer()), bits(acc))

    shard = _renderer(env)
    shard.m_RendererSettings = drt.RendererSettings(ray_bounce_limit=DEPTH)
    shard.setFramesInFlight(hint)
    shard.setShard(8, 1, 3)
    shard.ResizeBuffer(W, H)
    rows = [y for y in range(H) if (y // 8) % 3 == 1]
    assert shard.getLocalRows() == len(rows) == 24
    capfd.readouterr()
    shard.RenderBatch(cam, sc, FRAMES)
    (grid, slots, _, cap), = _launch_lines(capfd.readouterr().err)
    assert grid == min((W // 8) * (len(rows) // 8) * FRAMES, math.ceil(slots / min(hint, cap))), (grid, slots, cap)
    if share_max:
        assert grid < (W // 8) * (len(rows) // 8) * FRAMES and math.ceil(slots / 64) < WORK // FRAMES      # (the cut bit both launches)
    ref, acc = _reference("cornell_box", 0)
    assert np.array_equal(bits(shard.GetRenderTargetImage()), bits(ref[rows]))
    assert np.array_equal(bits(shard.GetAccumulationBuffer()), bits(acc[rows]))


def test_four_neighbours_each_render_what_they_render_alone():
    """Four renderers on four streams, hint 4, asynchronous, each at its own frame index, twenty rounds: every image equals the one an
    identical renderer computes alone with blocking calls, and launchesOfLastBatch() / kernelInfo() say the same."""
    torch = pytest.importorskip("torch")
    cam, sc = _cameras("cornell_box")[0], _pair("cornell_box")[0]

    def make(hint):
        r = _renderer({"DRT_POOL_PATHS": "64"})
        r.m_RendererSettings = drt.RendererSettings(ray_bounce_limit=DEPTH)
        r.setFramesInFlight(hint)
        r.ResizeBuffer(W, H)
        return r

    crowd, streams = [make(4) for _ in range(4)], [torch.cuda.Stream() for _ in range(4)]
    for i, (r, s) in enumerate(zip(crowd, streams)):
        r.setStream(s.cuda_stream)
        r.RenderBatch(cam, sc, i + 1)                    # (renderer i goes on from frame index i + 2)
    for _ in range(20):
        for r in crowd:
            r.RenderBatchAsync(cam, sc, FRAMES)
        for r in crowd:
            r.Wait()                                     # (raises unless the status is DRT_OK)
    for i, r in enumerate(crowd):
        alone = make(1)
        alone.RenderBatch(cam, sc, i + 1)
        for _ in range(20):
            alone.RenderBatch(cam, sc, FRAMES)
        assert np.array_equal(bits(r.GetRenderTargetImage()), bits(alone.GetRenderTargetImage())), "renderer %d" % i
        assert r.launchesOfLastBatch() == alone.launchesOfLastBatch() == 1
        assert r.kernelInfo() == alone.kernelInfo()
