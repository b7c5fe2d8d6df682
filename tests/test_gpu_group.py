"""The N-device group (csrc/drt_group.cpp) end to end on one GPU: a group of 2, 3 or 8 renderers that share device 0
(DRT_GROUP_SHARE_DEVICE=1), each on its own stream, gathering over a stand-in transport with NCCL's semantics that moves bytes
with hipMemcpyAsync (tests/cpp/mock_rccl.cpp, bound through DRT_RCCL_LIB).  The product's own gather code runs -- the Send /
Recv loop over ranks 1 .. world-1, staging slots, ranks without rows, the strided copy of device 0's stripes, the assemble
pass, drain on error, resize and destroy with work in flight -- and every image is compared bit for bit with a plain
Renderer(0), itself pinned to the oracle (test_gpu_parity.py), and here once with the oracle directly.  Only the real
multi-GPU transport is not exercised."""
import ctypes as C
import gc
import os
import subprocess

import numpy as np
import pytest

import oracle
from tests import ray_query_ref as rq
from tests.scenes import ROOT, SCENES, bits, scene_path

drt = pytest.importorskip("dustraytracer_amd")

pytestmark = pytest.mark.gpu

STRIPE = 8
# the entry points csrc/drt_group.cpp binds (dlsym)
NCCL_NAMES = ("ncclCommInitAll", "ncclCommDestroy", "ncclGroupStart", "ncclGroupEnd", "ncclSend", "ncclRecv", "ncclGetErrorString")
# call kinds of the mock's log and of mock_rccl_fail
INIT_ALL, SEND, RECV, GROUP_END, GROUP_START, DESTROY = range(6)
SHAPES = [(64, 44), (33, 1), (7, 8), (16, 129), (200, 61)]      # (33, 1), (7, 8): ranks 1 .. world-1 own no rows; (200, 61): short last stripe
FAR = ((0.0, 0.5, 12.0), (0.0, -0.05, -1.0))                     # the ray-query tests' view of the programmatic soup


def build_mock_rccl(out_dir):
    """Compiles tests/cpp/mock_rccl.cpp into out_dir; returns the library's path."""
    lib = os.path.join(str(out_dir), "libmock_rccl.so")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "cpp", "mock_rccl.cpp"), "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib",
                    "-o", lib], check=True)
    return lib


class Mock:
    """The mock transport's control functions, through the handle the product's dlopen also got (same path)."""

    def __init__(self, path):
        self.path = path
        self.lib = C.CDLL(path)
        for name, res in (("mock_rccl_depth", C.c_int), ("mock_rccl_queued", C.c_uint64), ("mock_rccl_violations", C.c_uint64),
                          ("mock_rccl_pairs_moved", C.c_uint64), ("mock_rccl_live_comms", C.c_int), ("mock_rccl_log_size", C.c_uint64)):
            getattr(self.lib, name).restype = res
        self.lib.mock_rccl_fail.argtypes = [C.c_int, C.c_uint64]
        self.lib.mock_rccl_log_entry.argtypes = [C.c_uint64] + [C.c_void_p] * 6

    def reset(self):
        self.lib.mock_rccl_reset()

    def fail(self, kind, k):
        assert self.lib.mock_rccl_fail(kind, k) == 0

    def depth(self):
        return self.lib.mock_rccl_depth()

    def queued(self):
        return self.lib.mock_rccl_queued()

    def violations(self):
        return self.lib.mock_rccl_violations()

    def live_comms(self):
        return self.lib.mock_rccl_live_comms()

    def last_violation(self):
        buf = C.create_string_buffer(512)
        self.lib.mock_rccl_last_violation(buf, 512)
        return buf.value.decode()

    def log(self):
        """[(kind, rank, peer, count, stream, result)] in call order."""
        out = []
        kind, rank, peer, res = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        count, stream = C.c_uint64(), C.c_void_p()
        for i in range(self.lib.mock_rccl_log_size()):
            assert self.lib.mock_rccl_log_entry(i, C.byref(kind), C.byref(rank), C.byref(peer), C.byref(count), C.byref(stream), C.byref(res)) == 0
            out.append((kind.value, rank.value, peer.value, count.value, stream.value, res.value))
        return out

    def assert_idle(self):
        """No open group, nothing queued, no misuse seen."""
        assert self.depth() == 0 and self.queued() == 0
        assert self.violations() == 0, self.last_violation()


@pytest.fixture(scope="module")
def mock_path(tmp_path_factory):
    return build_mock_rccl(tmp_path_factory.mktemp("mock_rccl"))


@pytest.fixture
def mock(mock_path, monkeypatch):
    monkeypatch.setenv("DRT_RCCL_LIB", mock_path)
    monkeypatch.setenv("DRT_GROUP_SHARE_DEVICE", "1")
    monkeypatch.delenv("DRT_GROUP_FORCE_RCCL", raising=False)
    monkeypatch.delenv("DRT_GROUP_GATHER", raising=False)
    m = Mock(mock_path)
    m.reset()
    gc.collect()                         # (a group an earlier failure kept alive goes now, not in the middle of a count)
    yield m
    m.reset()


_scenes = {}


def scene(name):
    """(product scene, camera): glTF scenes with the editor's BVH (leaf 20, 8 bins); "soup" = a programmatic tree beyond 32 767 nodes."""
    if name not in _scenes:
        if name == "soup":
            sc, _ = rq.programmatic_scene(drt, *rq.soup(90000, 1, spread=10.0), 2, 8)
            assert len(sc.m_BVHNodes) > 32767
            pos, fwd = FAR
        else:
            sc = drt.Scene()
            sc.loadGLTFmodel(scene_path(name))
            b = drt.BVHBuilder()
            b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
            b.buildIterative(sc)
            _, pos, fwd, _ = SCENES[name]
        cam = drt.Camera(pos)
        cam.m_Forward_dir = np.array(fwd, np.float32)
        _scenes[name] = (sc, cam)
    return _scenes[name]


def setup(xs, W, H, **settings):
    for x in xs:
        x.m_RendererSettings = drt.RendererSettings(**settings)
        x.ResizeBuffer(W, H)


def assert_same(g, r, what=""):
    assert g.getSampleCount() == r.getSampleCount(), what
    a, b = g.GetRenderTargetImage(), r.GetRenderTargetImage()
    assert a.shape == b.shape, what
    bad = int((bits(a) != bits(b)).any(axis=-1).sum())
    assert bad == 0, "%s: %d pixels not bit-equal to the single renderer" % (what, bad)


def expected_transfers(W, H, world, gather):
    """[(rank, count)] of one batch's gather, in issue order: one Send / Recv pair per rank >= 1 that owns rows (its whole shard),
    or per stripe of ranks >= 1 (DRT_GROUP_GATHER=stripes)."""
    out = []
    for rank in range(1, world):
        if gather == "stripes":
            k = 0
            while (s := drt.shard_stripe(W, H, STRIPE, rank, world, k)) is not None:
                out.append((rank, s[2]))
                k += 1
        else:
            n = drt.shard_rows(H, STRIPE, rank, world)
            if n:
                out.append((rank, W * n * 4))
    return out


def assert_gather_log(log, W, H, world, gather, batches):
    """The mock saw `batches` gathers, each GroupStart, (Send rank -> 0, Recv 0 <- rank) per expected transfer, GroupEnd; every call
    succeeded; the sends ran on the ranks' own streams (one per rank, none of them rank 0's), the receives on rank 0's."""
    calls = [e for e in log if e[0] in (SEND, RECV, GROUP_START, GROUP_END)]
    assert all(e[5] == 0 for e in calls), calls
    want = []
    for rank, count in expected_transfers(W, H, world, gather):
        want += [(SEND, rank, 0, count), (RECV, 0, rank, count)]
    per_batch = [(GROUP_START, -1, -1, 0)] + want + [(GROUP_END, -1, -1, len(want))]
    assert [e[:4] for e in calls] == per_batch * batches
    send_streams = {}
    for e in calls:
        if e[0] == SEND:
            assert send_streams.setdefault(e[1], e[4]) == e[4]
    recv_streams = {e[4] for e in calls if e[0] == RECV}
    assert len(recv_streams) <= 1 and not recv_streams & set(send_streams.values())
    assert len(set(send_streams.values())) == len(send_streams)


@pytest.mark.parametrize("gather", ["shards", "stripes"])
@pytest.mark.parametrize("world", [2, 3, 8])
def test_group_equals_single_renderer_across_worlds_and_shapes(mock, monkeypatch, world, gather):
    """Worlds 2, 3, 8 on one device through both gathers, at shapes where ranks own no rows and where the last stripe is short,
    resized in turn on the same group: 2 frames then 1 more (the second batch continues the accumulation), same bits and sample
    count as the single renderer; the transport saw exactly the expected transfers and was left idle."""
    if gather == "stripes":
        monkeypatch.setenv("DRT_GROUP_GATHER", "stripes")
    sc, cam = scene("cornell_box")
    before = mock.live_comms()
    g, r = drt.RendererGroup([0] * world), drt.Renderer(0)
    assert g.size() == world and mock.live_comms() == before + world
    for W, H in SHAPES:
        what = "world %d, %s, %dx%d" % (world, gather, W, H)
        setup((g, r), W, H, ray_bounce_limit=4)
        mock.reset()
        g.RenderBatch(cam, sc, 2); r.RenderBatch(cam, sc, 2)
        mock.assert_idle()
        assert g.getSampleCount() == 3
        assert_same(g, r, what)
        g.RenderBatch(cam, sc, 1); r.RenderBatch(cam, sc, 1)
        mock.assert_idle()
        assert g.getSampleCount() == 4
        assert_same(g, r, what + ", second batch")
        assert_gather_log(mock.log(), W, H, world, gather, batches=2)
    del g
    assert mock.live_comms() == before


KERNEL_CASES = [
    ("cornell_box", dict(ray_bounce_limit=8), ("path_pool<", "lds-scene")),
    ("cs16_dust", dict(ray_bounce_limit=3, enableSunlight=1), ("path_pool<", "+sun", "hbm-scene")),
    ("mc_transparency", dict(ray_bounce_limit=3, enableSunlight=1), ("path_pool<", "+alpha")),
    ("cornell_box", dict(RenderMode=1, DebugMode=1), ("wave_queue<general",)),
    ("soup", dict(ray_bounce_limit=3), ("wave_queue<",)),
]


@pytest.mark.parametrize("name,settings,kernel", KERNEL_CASES, ids=["lds-scene", "hbm-scene", "alpha", "debug-view", "large-tree"])
def test_group_equals_single_renderer_on_every_tracing_kernel(mock, name, settings, kernel):
    """Every family of tracing kernel on shards of a world of 3 -- 96 x 61 (rank 1's last stripe is short), then 7 x 8 (ranks 1
    and 2 own no rows): bit-equal to the single renderer, and rank 0 ran the expected kernel."""
    sc, cam = scene(name)
    g, r = drt.RendererGroup([0] * 3), drt.Renderer(0)
    for W, H in ((96, 61), (7, 8)):
        setup((g, r), W, H, **settings)
        mock.reset()
        g.RenderBatch(cam, sc, 2); r.RenderBatch(cam, sc, 2)
        mock.assert_idle()
        assert_same(g, r, "%s %dx%d" % (name, W, H))
        for k in kernel:
            assert k in g.kernelInfo(0), g.kernelInfo(0)
            assert k in r.kernelInfo(), r.kernelInfo()
        assert_gather_log(mock.log(), W, H, 3, "shards", batches=1)


def test_group_equals_the_oracle(mock):
    """World 3, cornell_box 64 x 44, depth 4, 2 frames: the assembled image equals the oracle's render of the whole frame."""
    name = "cornell_box"
    _, pos, fwd, _ = SCENES[name]
    sc, cam = scene(name)
    g = drt.RendererGroup([0] * 3)
    setup((g,), 64, 44, ray_bounce_limit=4)
    g.RenderBatch(cam, sc, 2)
    mock.assert_idle()
    img = g.GetRenderTargetImage()
    osc = oracle.Scene.load_glb(scene_path(name)).build_bvh(20, 8)
    ref, _, _ = oracle.render(osc, oracle.default_camera(position=pos, forward=fwd), oracle.default_settings(ray_bounce_limit=4), 64, 44, 1, 2)
    assert np.array_equal(bits(img), bits(ref))


@pytest.mark.parametrize("gather", ["shards", "stripes"])
def test_group_of_eight_at_1080p(mock, monkeypatch, gather):
    """World 8 at 1920 x 1080 (135 stripes: 17 for ranks 0 .. 6, 16 for rank 7), cornell_box depth 8, 2 frames: the single renderer's bits."""
    if gather == "stripes":
        monkeypatch.setenv("DRT_GROUP_GATHER", "stripes")
    sc, cam = scene("cornell_box")
    g, r = drt.RendererGroup([0] * 8), drt.Renderer(0)
    setup((g, r), 1920, 1080, ray_bounce_limit=8)
    g.RenderBatch(cam, sc, 2); r.RenderBatch(cam, sc, 2)
    mock.assert_idle()
    assert_same(g, r, "1080p " + gather)
    assert_gather_log(mock.log(), 1920, 1080, 8, gather, batches=1)


def test_group_async_resize_destroy_and_two_groups(mock):
    """A batch left in flight is drained by ResizeBuffer (then the image is right at the new size) and by the destructor; two
    groups on device 0 alive and in flight at once; every communicator is destroyed with its group."""
    sc, cam = scene("cornell_box")
    before = mock.live_comms()
    g, r = drt.RendererGroup([0] * 3), drt.Renderer(0)
    setup((g, r), 64, 44, ray_bounce_limit=4)
    g.RenderBatchAsync(cam, sc, 2)
    setup((g, r), 50, 27, ray_bounce_limit=4)                           # drains the batch in flight, then reallocates
    mock.assert_idle()
    g.RenderBatch(cam, sc, 2); r.RenderBatch(cam, sc, 2)
    assert_same(g, r, "after a resize with a batch in flight")
    g.RenderBatchAsync(cam, sc, 1); g.RenderBatchAsync(cam, sc, 2)      # a second batch queued behind the first, then one wait
    r.RenderBatch(cam, sc, 1); r.RenderBatch(cam, sc, 2)
    assert g.Wait() > 0
    assert_same(g, r, "two batches in flight")

    g2, r2 = drt.RendererGroup([0] * 2), drt.Renderer(0)
    assert mock.live_comms() == before + 5
    setup((g2, r2), 50, 27, ray_bounce_limit=4)
    g.RenderBatchAsync(cam, sc, 1); g2.RenderBatchAsync(cam, sc, 3)      # both in flight
    r.RenderBatch(cam, sc, 1); r2.RenderBatch(cam, sc, 3)
    assert g.Wait() > 0 and g2.Wait() > 0
    assert_same(g, r, "first group"); assert_same(g2, r2, "second group")

    g.RenderBatchAsync(cam, sc, 2)
    del g                                                                # with a batch pending
    assert mock.live_comms() == before + 2
    g2.RenderBatch(cam, sc, 1); r2.RenderBatch(cam, sc, 1)
    assert_same(g2, r2, "second group after the first is gone")
    mock.assert_idle()
    del g2
    assert mock.live_comms() == before


def test_group_stops_at_max_samples(mock):
    """max_samples stops the group and the single renderer at the same count (Renderer.cu:82); the image stays the same after."""
    sc, cam = scene("cornell_box")
    g, r = drt.RendererGroup([0] * 3), drt.Renderer(0)
    setup((g, r), 40, 21, ray_bounce_limit=4, max_samples=4)
    for n, count in ((2, 3), (5, 4), (2, 4)):
        g.RenderBatch(cam, sc, n); r.RenderBatch(cam, sc, n)
        assert g.getSampleCount() == r.getSampleCount() == count
        assert_same(g, r, "max_samples, batch of %d" % n)
    mock.assert_idle()


@pytest.mark.parametrize("gather", ["shards", "stripes"])
@pytest.mark.parametrize("fault", ["send_rank1", "send_last_rank", "recv", "group_end"])
def test_group_recovers_from_a_failed_transfer(mock, monkeypatch, gather, fault):
    """A failed ncclSend (rank 1's, the last rank's), ncclRecv or ncclGroupEnd -- host return codes only -- makes RenderBatch raise
    ERR_DEVICE naming the call; the group is drained (not pending), the transport idle; after resetAccumulationBuffer the group
    renders the single renderer's bits again, and resize and destroy work."""
    if gather == "stripes":
        monkeypatch.setenv("DRT_GROUP_GATHER", "stripes")
    world, W, H = 3, 64, 44
    sc, cam = scene("cornell_box")
    before = mock.live_comms()
    g, r = drt.RendererGroup([0] * world), drt.Renderer(0)
    setup((g, r), W, H, ray_bounce_limit=4)
    g.RenderBatch(cam, sc, 1)
    ranks = [rank for rank, _ in expected_transfers(W, H, world, gather)]
    kind, k, name = {"send_rank1": (SEND, ranks.index(1) + 1, "ncclSend"),
                     "send_last_rank": (SEND, ranks.index(world - 1) + 1, "ncclSend"),
                     "recv": (RECV, 1, "ncclRecv"),
                     "group_end": (GROUP_END, 1, "ncclGroupEnd")}[fault]
    mock.reset()
    mock.fail(kind, k)
    with pytest.raises(drt.DrtError) as e:
        g.RenderBatch(cam, sc, 2)
    code, msg = e.value.code, str(e.value)
    del e                                                                # (its traceback holds the group)
    assert code == drt.ERR_DEVICE and name in msg, msg
    assert g.Wait() == 0.0                                               # drained: nothing pending
    mock.assert_idle()
    failed = [x[0] for x in mock.log() if x[5] != 0]
    assert failed == ([kind] if kind == GROUP_END else [kind, GROUP_END])      # (a failed Send / Recv poisons the group: GroupEnd reports it)
    for x in (g, r):
        x.resetAccumulationBuffer()
    g.RenderBatch(cam, sc, 2); r.RenderBatch(cam, sc, 2)
    assert_same(g, r, "after a failed " + name)
    setup((g, r), 40, 21, ray_bounce_limit=4)
    g.RenderBatch(cam, sc, 1); r.RenderBatch(cam, sc, 1)
    assert_same(g, r, "after a failed %s and a resize" % name)
    mock.assert_idle()
    del g
    gc.collect()
    assert mock.live_comms() == before


def test_group_creation_fails_cleanly_when_comm_init_fails(mock):
    """A failed ncclCommInitAll: RendererGroup raises naming it, leaves no communicator behind, and the next group works."""
    before = mock.live_comms()
    mock.fail(INIT_ALL, 1)
    with pytest.raises(drt.DrtError) as e:
        drt.RendererGroup([0] * 3)
    assert e.value.code == drt.ERR_DEVICE and "ncclCommInitAll" in str(e.value), str(e.value)
    assert mock.live_comms() == before
    sc, cam = scene("cornell_box")
    g, r = drt.RendererGroup([0] * 2), drt.Renderer(0)
    setup((g, r), 33, 20, ray_bounce_limit=4)
    g.RenderBatch(cam, sc, 2); r.RenderBatch(cam, sc, 2)
    assert_same(g, r, "after a failed ncclCommInitAll")
    mock.assert_idle()


def _read_pfm_bytes(path):
    with open(path, "rb") as f:
        return f.read()


def test_cli_on_a_group_of_three(mock, mock_path, tmp_path):
    """examples/drt_render with DRT_DEVICES=0,0,0 (and both hooks) writes the same PFM bytes as the one-device run."""
    exe = tmp_path / "drt_render"
    lib_dir = os.path.dirname(drt.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "drt_render.cpp"),
                    "-L" + lib_dir, "-ldrt_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    _, pos, fwd, depth = SCENES["cornell_box"]
    single, group = str(tmp_path / "single.pfm"), str(tmp_path / "group.pfm")
    args = lambda out: [str(exe), scene_path("cornell_box"), out, "64", "44", "3", str(depth)] + ["%g" % v for v in pos + fwd]
    env = dict(os.environ)
    for k in ("DRT_DEVICES", "DRT_RCCL_LIB", "DRT_GROUP_SHARE_DEVICE", "DRT_GROUP_GATHER", "DRT_GROUP_FORCE_RCCL"):
        env.pop(k, None)
    out = subprocess.run(args(single), env=env, capture_output=True, text=True, timeout=300, check=True).stdout
    assert "on 1 GPU:" in out
    env.update(DRT_DEVICES="0,0,0", DRT_RCCL_LIB=mock_path, DRT_GROUP_SHARE_DEVICE="1")
    out = subprocess.run(args(group), env=env, capture_output=True, text=True, timeout=300, check=True).stdout
    assert "on 3 GPUs:" in out
    a, b = _read_pfm_bytes(single), _read_pfm_bytes(group)
    assert len(a) == len(b) > 64 * 44 * 12 and a == b
