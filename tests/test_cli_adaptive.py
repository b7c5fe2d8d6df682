"""examples/drt_render.cpp --adaptive SPP [--target-error E] [--adaptive-calls K] on the GPU: the image it writes is the one the
Python calls produce, it stops once every pixel is converged, and the filters read what it rendered."""
import os
import subprocess

import numpy as np
import pytest

from tests.scenes import ROOT, SCENES, scene_path

drt = pytest.importorskip("dustraytracer_amd")

pytestmark = pytest.mark.gpu


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"PF"
        W, H = map(int, f.readline().split())
        f.readline()
        return np.frombuffer(f.read(), np.float32).reshape(H, W, 3)


def test_cli_adaptive(tmp_path):
    exe = tmp_path / "drt_render"
    lib_dir = os.path.dirname(drt.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "drt_render.cpp"),
                    "-L" + lib_dir, "-ldrt_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    _, pos, fwd, _ = SCENES["cornell_box"]
    plain, den, sky = str(tmp_path / "ad.pfm"), str(tmp_path / "ad_den.pfm"), str(tmp_path / "sky.pfm")
    head = [scene_path("cornell_box"), None, "48", "32", "1", "3"]
    args = head + ["%g" % v for v in pos + fwd] + ["--adaptive", "4", "--adaptive-calls", "2"]
    out = subprocess.run([str(exe)] + args[:1] + [plain] + args[2:], capture_output=True, text=True, check=True).stdout
    assert "adaptive: 2 calls" in out and "denoised" not in out
    out = subprocess.run([str(exe)] + args[:1] + [den] + args[2:] + ["--denoise"], capture_output=True, text=True, check=True).stdout
    assert "adaptive: 2 calls" in out and "denoised: 5 passes" in out
    # a camera that sees only sky: converged after the first call, so the second finds nothing to do and the loop ends there
    away = head + ["1000", "1000", "1000", "1", "0.2", "0"] + ["--adaptive", "4", "--target-error", "0.001"]
    out = subprocess.run([str(exe)] + away[:1] + [sky] + away[2:], capture_output=True, text=True, check=True).stdout
    assert "adaptive: 2 calls, %d samples" % (4 * 48 * 32) in out
    sc = drt.Scene()
    sc.loadGLTFmodel(scene_path("cornell_box"))
    b = drt.BVHBuilder()
    b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
    b.buildIterative(sc)
    cam = drt.Camera(pos)
    cam.m_Forward_dir = np.array(fwd, np.float32)
    r = drt.Renderer(0)
    r.m_RendererSettings = drt.RendererSettings(ray_bounce_limit=3, max_samples=2)
    r.ResizeBuffer(48, 32)
    for _ in range(2):
        r.RenderAdaptive(cam, sc, spp=4)
    got = _read_pfm(plain)
    assert got.shape == (32, 48, 3)
    assert (u32(got) == u32(r.GetRenderTargetImage()[..., :3])).all()
    assert (u32(_read_pfm(den)) == u32(r.Denoise(cam, sc)[..., :3])).all()
