// drt_render.cpp -- headless use of the reference-shaped C++ API: scene.glb -> RGBA32F -> PFM or PNG file.
// (.png output reproduces the editor's "save png": 8-bit clamp of the GL read-back + vertical flip, EditorLayer.cpp:23-31,85-96)
//   g++ -std=c++17 -Iinclude examples/drt_render.cpp -Ldustraytracer_amd -ldrt_hip -Wl,-rpath,$PWD/dustraytracer_amd -o drt_render
//   ./drt_render models/cornell_box.glb out.pfm 1920 1080 8 8  3.6 1.25 0  -1 0 0
//   ./drt_render models/cornell_box.glb out.png 1920 1080 4 8  3.6 1.25 0  -1 0 0  --denoise     (writes the a-trous denoised frame)
//   ./drt_render models/cornell_box.glb out.png 1920 1080 1 8  3.6 1.25 0  -1 0 0  --temporal 12  (12 poses of a small orbit ending at the
//                                                  given pose, 1 spp each, temporally accumulated and filtered: writes the last pose)
//   ./drt_render models/cornell_box.glb out.png 960 540 1 8  3.6 1.25 0  -1 0 0  --upscale 1920 1080 --temporal 12   (rendered and filtered
//                                                  at 960 x 540, rebuilt at 1920 x 1080 from full-size first-hit guides: writes the large image)
//   ./drt_render models/cornell_box.glb out.png 1920 1080 1 8  3.6 1.25 0  -1 0 0  --adaptive 4 --target-error 0.01 --adaptive-calls 8
//                                                  (up to 8 adaptive calls of 4 samples per pixel each, spent where the noise is, until every
//                                                  pixel's relative error is below 1 %: writes sum / n; the spp argument is not used)
//   DRT_DEVICES=0,1,2,3,4,5,6,7 ./drt_render models/room.glb out.pfm 3840 2160 64 16  0 1.4 2  0 0 -1     (all GPUs of the node: stripes + RCCL gather)
#include <DustRayTracer.hpp>
#include <DustRayTracerGL.hpp>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using drtgl::write_png_rgba8;      // the minimal PNG writer lives in DustRayTracerGL.hpp (the editor shim's "save png")

int main(int argc, char **argv) {
    const bool denoise = argc > 1 && std::strcmp(argv[argc - 1], "--denoise") == 0;     // optional, always last
    if (denoise) argc--;
    int temporal = 0;                                     // --temporal K: optional, last (before --denoise)
    if (argc > 2 && std::strcmp(argv[argc - 2], "--temporal") == 0) {
        temporal = std::atoi(argv[argc - 1]);
        argc -= 2;
    }
    long up_w = 0, up_h = 0;                              // --upscale OW OH: optional, last (before --temporal)
    const bool upscale = argc > 3 && std::strcmp(argv[argc - 3], "--upscale") == 0;
    if (upscale) {
        up_w = std::atol(argv[argc - 2]);
        up_h = std::atol(argv[argc - 1]);
        argc -= 3;
    }
    int adaptive_calls = 8;                               // --adaptive SPP [--target-error E] [--adaptive-calls K]: optional, last (before --upscale)
    double adaptive_spp = 0, target_error = 0;
    const bool calls_given = argc > 2 && std::strcmp(argv[argc - 2], "--adaptive-calls") == 0;
    if (calls_given) {
        adaptive_calls = std::atoi(argv[argc - 1]);
        argc -= 2;
    }
    const bool error_given = argc > 2 && std::strcmp(argv[argc - 2], "--target-error") == 0;
    if (error_given) {
        target_error = std::atof(argv[argc - 1]);
        argc -= 2;
    }
    const bool adaptive = argc > 2 && std::strcmp(argv[argc - 2], "--adaptive") == 0;
    if (adaptive) {
        adaptive_spp = std::atof(argv[argc - 1]);
        argc -= 2;
    }
    if (argc < 7 || temporal < 0 || (upscale && (up_w <= 0 || up_h <= 0)) || ((calls_given || error_given) && !adaptive) ||
        (adaptive && (!(adaptive_spp >= 1) || adaptive_calls < 1 || !(target_error >= 0)))) {
        std::fprintf(stderr, "usage: %s scene.glb out.pfm width height spp depth [px py pz fx fy fz] [--adaptive SPP [--target-error E] [--adaptive-calls K]] "
                             "[--upscale OW OH] [--temporal K] [--denoise]\n", argv[0]);
        return 2;
    }
    try {
        uint32_t W = (uint32_t)std::atoi(argv[3]), H = (uint32_t)std::atoi(argv[4]);
        const uint32_t spp = (uint32_t)std::atoi(argv[5]);
        Scene scene;
        scene.loadGLTFmodel(argv[1]);
        BVHBuilder builder;                               // EditorLayer.cpp:52-55
        builder.m_TargetLeafPrimitivesCount = 20;
        builder.m_BinCount = 8;
        builder.buildIterative(scene);
        Camera cam;
        if (argc >= 13) {
            cam.m_Position = { (float)std::atof(argv[7]), (float)std::atof(argv[8]), (float)std::atof(argv[9]) };
            cam.m_Forward_dir = { (float)std::atof(argv[10]), (float)std::atof(argv[11]), (float)std::atof(argv[12]) };
        }
        std::vector<int> devices;                         // DRT_DEVICES=0,1,...: several GPUs of the node behind the same Renderer calls
        if (const char *list = std::getenv("DRT_DEVICES"))
            for (const char *p = list; *p;) { devices.push_back(std::atoi(p)); while (*p && *p != ',') p++; if (*p == ',') p++; }
        if (devices.empty()) devices.push_back(0);
        Renderer renderer(devices);
        renderer.m_RendererSettings.ray_bounce_limit = std::atoi(argv[6]);
        renderer.m_RendererSettings.max_samples = (int)spp + 1;
        renderer.ResizeBuffer(W, H);
        float ms = 0;
        std::vector<float> rgba((size_t)W * H * 4);
        if (adaptive) {
            // K adaptive calls of SPP samples per pixel each instead of the frame loop; over once every pixel is converged
            drt_adaptive_params p;
            drt_default_adaptive_params(&p);
            p.budget = (uint32_t)std::min(adaptive_spp * (double)W * (double)H, 4294967295.0);       // (the library refuses 2^31 and more)
            p.target_error = (float)target_error;
            unsigned long long samples = 0;
            int calls = 0;
            while (calls < adaptive_calls) {
                const drt_adaptive_info info = renderer.RenderAdaptive(&cam, scene, &p);
                calls++;
                samples += info.samples;
                ms += info.ms;
                if (info.active_pixels == 0) break;
            }
            renderer.ReadRenderTarget(rgba.data());
            std::printf("%zu triangles, %u x %u, adaptive: %d calls, %llu samples (%.2f per pixel): %.3f ms\n", scene.trianglesCount(), W, H, calls,
                        samples, (double)samples / ((double)W * H), ms);
        } else {
            renderer.RenderBatch(&cam, scene, spp, &ms);
            renderer.ReadRenderTarget(rgba.data());
            std::printf("%zu triangles, %u x %u, %u spp on %d GPU%s: %.3f ms (%.1f Msamples/s)\n", scene.trianglesCount(), W, H, spp,
                        renderer.deviceCount(), renderer.deviceCount() > 1 ? "s" : "", ms, (double)W * H * spp / ms / 1e3);
        }
        if (denoise) {                                    // the a-trous filter of the frame, default parameters (drt_default_denoise_params)
            drt_denoise_params p;
            drt_default_denoise_params(&p);
            float dms = 0;
            renderer.Denoise(&cam, scene, &dms, p.iterations, p.sigma_color, p.sigma_normal, p.sigma_albedo);
            renderer.ReadDenoisedTarget(rgba.data());
            std::printf("denoised: %d passes, %.3f ms\n", p.iterations, dms);
        }
        if (temporal > 0) {
            // K poses at 1 spp each on an orbit (0.01 rad per pose about the vertical through the point 3 units ahead) that ends
            // at the given pose; every pose is reset, rendered and handed to the temporal filter, which carries the history
            const float px = cam.m_Position.x, pz = cam.m_Position.z, fx = cam.m_Forward_dir.x, fz = cam.m_Forward_dir.z;
            const float fl = std::sqrt(fx * fx + cam.m_Forward_dir.y * cam.m_Forward_dir.y + fz * fz);
            const float cx = px + fx / fl * 3.0f, cz = pz + fz / fl * 3.0f;
            float tms = 0, total = 0;
            for (int k = 0; k < temporal; k++) {
                const float ang = 0.01f * (float)(k - (temporal - 1)), co = std::cos(ang), si = std::sin(ang);
                Camera pose = cam;
                pose.m_Position.x = cx + (px - cx) * co - (pz - cz) * si;
                pose.m_Position.z = cz + (px - cx) * si + (pz - cz) * co;
                pose.m_Forward_dir.x = fx * co - fz * si;
                pose.m_Forward_dir.z = fx * si + fz * co;
                renderer.resetAccumulationBuffer();
                renderer.RenderBatch(&pose, scene, 1, &ms);
                renderer.TemporalDenoise(&pose, scene, &tms);
                total += tms;
            }
            renderer.ReadDenoisedTarget(rgba.data());
            std::printf("temporal: %d poses, %.3f ms per pose\n", temporal, total / (float)temporal);
        }
        if (upscale) {
            // the frame (the filtered one when --denoise or --temporal made it) rebuilt at OW x OH, default parameters otherwise
            drt_upscale_params p;
            drt_default_upscale_params(&p);
            p.source = (denoise || temporal > 0) ? 1 : 0;
            float ums = 0;
            renderer.Upscale(&cam, scene, (uint32_t)up_w, (uint32_t)up_h, &ums, &p);
            std::printf("upscaled: %u x %u -> %ld x %ld, %.3f ms\n", W, H, up_w, up_h, ums);
            W = (uint32_t)up_w; H = (uint32_t)up_h;
            rgba.resize((size_t)W * H * 4);
            renderer.ReadUpscaledTarget(rgba.data());
        }
        const std::string out(argv[2]);
        if (out.size() > 4 && out.compare(out.size() - 4, 4, ".png") == 0) {
            // glGetTexImage(GL_RGBA, GL_UNSIGNED_BYTE) clamps to [0,1] and rounds to 8 bits; stbi_flip_vertically_on_write(true)
            std::vector<uint8_t> bytes((size_t)W * H * 4);
            for (uint32_t y = 0; y < H; y++)
                for (uint32_t x = 0; x < W; x++)
                    for (int c = 0; c < 4; c++) {
                        float v = rgba[((size_t)(H - 1 - y) * W + x) * 4 + c];
                        v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
                        bytes[((size_t)y * W + x) * 4 + c] = (uint8_t)(v * 255.0f + 0.5f);
                    }
            if (!write_png_rgba8(argv[2], W, H, bytes)) { std::perror(argv[2]); return 1; }
        } else {
            FILE *f = std::fopen(argv[2], "wb");           // PFM stores rows bottom-up, like the framebuffer
            if (!f) { std::perror(argv[2]); return 1; }
            std::fprintf(f, "PF\n%u %u\n-1.0\n", W, H);
            for (size_t p = 0; p < (size_t)W * H; p++) std::fwrite(&rgba[4 * p], sizeof(float), 3, f);
            std::fclose(f);
        }
    } catch (const drt::Error &e) {
        std::fprintf(stderr, "drt error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
