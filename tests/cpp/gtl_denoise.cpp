// gtl_denoise.cpp -- gtlDenoise (include/gtl/gi/Gi.h -> giCDenoise) from a C++ client, as a render delegate would call it.
//   gtl_denoise refuse   no device: a call without buffers is refused with GiStatus::Error (never a crash)
//   gtl_denoise run      on a device: five gtl render buffers, synthetic guides sent from host memory (source 1), a noisy constant colour filtered over a flat
//                        surface beside a background column; the result must be closer to the constant than the input, the background and alpha untouched
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include <gtl/gi/Gi.h>

using namespace gtl;

int main(int argc, char** argv)
{
  if (argc > 1 && !strcmp(argv[1], "refuse")) {
    GtlDenoiseParams p;
    if (gtlDenoise(p) != GiStatus::Error) { printf("a call without buffers was accepted\n"); return 1; }
    printf("gtl_denoise refuse ok\n");
    return 0;
  }
  std::vector<std::string> noPaths;
  GiInitParams ip{"", "", noPaths, nullptr, ""};
  if (giInitialize(ip) != GiStatus::Ok) { printf("giInitialize failed\n"); return 1; }
  const uint32_t w = 40, h = 24;
  GtlDenoiseParams p;
  p.color = giCreateRenderBuffer(w, h, GiRenderBufferFormat::Float32Vec4); p.normal = giCreateRenderBuffer(w, h, GiRenderBufferFormat::Float32Vec4);
  p.albedo = giCreateRenderBuffer(w, h, GiRenderBufferFormat::Float32Vec4); p.depth = giCreateRenderBuffer(w, h, GiRenderBufferFormat::Float32);
  p.output = giCreateRenderBuffer(w, h, GiRenderBufferFormat::Float32Vec4);
  if (!p.color || !p.normal || !p.albedo || !p.depth || !p.output) { printf("giCreateRenderBuffer failed\n"); return 1; }
  float* C = (float*)giGetRenderBufferMem(p.color); float* N = (float*)giGetRenderBufferMem(p.normal); float* B = (float*)giGetRenderBufferMem(p.albedo);
  float* Z = (float*)giGetRenderBufferMem(p.depth);
  uint32_t s = 12345u;
  for (uint32_t i = 0; i < w * h; i++) {
    s = s * 1664525u + 1013904223u;
    const float noise = ((s >> 8) * (1.0f / 16777216.0f) - 0.5f) * 0.5f;
    const bool background = i % w == 0;
    C[4 * i] = C[4 * i + 1] = C[4 * i + 2] = 0.5f + noise; C[4 * i + 3] = 0.25f;
    N[4 * i] = 0.5f; N[4 * i + 1] = 0.5f; N[4 * i + 2] = 1.0f; N[4 * i + 3] = 0.0f;
    B[4 * i] = B[4 * i + 1] = B[4 * i + 2] = 0.8f; B[4 * i + 3] = 1.0f;
    Z[i] = background ? 1.0f : 0.5f;
  }
  p.source = 1;
  if (gtlDenoise(p) != GiStatus::Ok) { printf("gtlDenoise failed\n"); return 1; }
  const float* O = (const float*)giGetRenderBufferMem(p.output);
  double before = 0.0, after = 0.0;
  for (uint32_t i = 0; i < w * h; i++) {
    if (O[4 * i + 3] != 0.25f) { printf("alpha changed at %u\n", i); return 1; }
    if (i % w == 0) { if (memcmp(O + 4 * i, C + 4 * i, 16)) { printf("background pixel %u changed\n", i); return 1; } continue; }
    before += fabs(C[4 * i] - 0.5); after += fabs(O[4 * i] - 0.5);
  }
  if (!(after < 0.25 * before)) { printf("not denoised: %g -> %g\n", before, after); return 1; }
  GtlDenoiseParams alias = p; alias.output = p.color;
  if (gtlDenoise(alias) != GiStatus::Error) { printf("aliasing was accepted\n"); return 1; }
  giDestroyRenderBuffer(p.color); giDestroyRenderBuffer(p.normal); giDestroyRenderBuffer(p.albedo); giDestroyRenderBuffer(p.depth); giDestroyRenderBuffer(p.output);
  giTerminate();
  printf("gtl_denoise ok (%g -> %g)\n", before, after);
  return 0;
}
