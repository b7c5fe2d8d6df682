"""examples/drt_render.cpp --upscale OW OH on the GPU: the image it writes is the Python call's, from the framebuffer and, with
--temporal or --denoise, from the denoised target."""
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


def test_cli_upscale(tmp_path):
    exe = tmp_path / "drt_render"
    lib_dir = os.path.dirname(drt.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "drt_render.cpp"),
                    "-L" + lib_dir, "-ldrt_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    _, pos, fwd, _ = SCENES["cornell_box"]
    plain, den = str(tmp_path / "up.pfm"), str(tmp_path / "up_den.pfm")
    args = [scene_path("cornell_box"), None, "48", "32", "2", "3"] + ["%g" % v for v in pos + fwd] + ["--upscale", "96", "64"]
    out = subprocess.run([str(exe)] + args[:1] + [plain] + args[2:], capture_output=True, text=True, check=True).stdout
    assert "upscaled: 48 x 32 -> 96 x 64" in out and "denoised" not in out
    out = subprocess.run([str(exe)] + args[:1] + [den] + args[2:] + ["--denoise"], capture_output=True, text=True, check=True).stdout
    assert "denoised: 5 passes" in out and "upscaled: 48 x 32 -> 96 x 64" in out
    sc = drt.Scene()
    sc.loadGLTFmodel(scene_path("cornell_box"))
    b = drt.BVHBuilder()
    b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
    b.buildIterative(sc)
    cam = drt.Camera(pos)
    cam.m_Forward_dir = np.array(fwd, np.float32)
    r = drt.Renderer(0)
    r.m_RendererSettings = drt.RendererSettings(ray_bounce_limit=3, max_samples=3)
    r.ResizeBuffer(48, 32)
    r.RenderBatch(cam, sc, 2)
    got = _read_pfm(plain)
    assert got.shape == (64, 96, 3)
    assert (u32(got) == u32(r.Upscale(cam, sc, 96, 64)[..., :3])).all()
    r.Denoise(cam, sc)
    assert (u32(_read_pfm(den)) == u32(r.Upscale(cam, sc, 96, 64, source=1)[..., :3])).all()
