// gtl_denoise_variance.cpp -- gtlDenoiseVariance (include/gtl/gi/Gi.h -> giCDenoiseVariance) from a C++ client, as a render delegate would call it.
//   gtl_denoise_variance refuse   no device: a call without a moments buffer is refused with GiStatus::Error (never a crash)
//   gtl_denoise_variance run      on a device: six gtl render buffers, synthetic guides and moments sent from host memory (source 1).  A flat surface beside a
//                                 background column; the left half's pixels are noisy with a sample variance that says so, the right half's are exact with a
//                                 variance of zero.  The noisy half must come out closer to the constant than it went in; the converged half, from two
//                                 columns past the border on (the border column's 3 x 3 variance average still sees the noisy pixels' variance, and the
//                                 variance that travels with the colour reaches its neighbour), must move less than a tenth of what gtlDenoise's fixed
//                                 sigma moves the same pixels -- a converged pixel's colour weight is scaled by its own variance, not by one sigma for the
//                                 whole image; background and alpha untouched
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
    GtlDenoiseVarianceParams p;
    if (gtlDenoiseVariance(p) != GiStatus::Error) { printf("a call without buffers was accepted\n"); return 1; }
    printf("gtl_denoise_variance refuse ok\n");
    return 0;
  }
  std::vector<std::string> noPaths;
  GiInitParams ip{"", "", noPaths, nullptr, ""};
  if (giInitialize(ip) != GiStatus::Ok) { printf("giInitialize failed\n"); return 1; }
  const uint32_t w = 40, h = 24, n = 16;
  GtlDenoiseVarianceParams p;
  GtlDenoiseParams& b = p.base;
  b.color = giCreateRenderBuffer(w, h, GiRenderBufferFormat::Float32Vec4); b.normal = giCreateRenderBuffer(w, h, GiRenderBufferFormat::Float32Vec4);
  b.depth = giCreateRenderBuffer(w, h, GiRenderBufferFormat::Float32); b.output = giCreateRenderBuffer(w, h, GiRenderBufferFormat::Float32Vec4);
  p.moments = giCreateRenderBuffer(w, h, GiRenderBufferFormat::Float32Vec4);
  if (!b.color || !b.normal || !b.depth || !b.output || !p.moments) { printf("giCreateRenderBuffer failed\n"); return 1; }
  float* C = (float*)giGetRenderBufferMem(b.color); float* N = (float*)giGetRenderBufferMem(b.normal); float* Z = (float*)giGetRenderBufferMem(b.depth);
  float* M = (float*)giGetRenderBufferMem(p.moments);
  uint32_t s = 12345u;
  for (uint32_t i = 0; i < w * h; i++) {
    s = s * 1664525u + 1013904223u;
    const bool background = i % w == 0, noisy = i % w < w / 2;
    const float noise = noisy ? ((s >> 8) * (1.0f / 16777216.0f) - 0.5f) * 0.5f : 0.0f;
    const float c = (noisy ? 0.5f : 0.75f) + noise; // (grey: the luminance is the value to a rounding)
    C[4 * i] = C[4 * i + 1] = C[4 * i + 2] = c; C[4 * i + 3] = 0.25f;
    N[4 * i] = 0.5f; N[4 * i + 1] = 0.5f; N[4 * i + 2] = 1.0f; N[4 * i + 3] = 0.0f;
    Z[i] = background ? 1.0f : 0.5f;
    // n samples of mean c: the noisy half with a per-sample standard deviation of 0.15 * sqrt(n) (the mean's is 0.15, what the noise above has), the other none
    const float sd = noisy ? 0.15f * sqrtf((float)n) : 0.0f;
    M[4 * i] = n * c; M[4 * i + 1] = n * (c * c + sd * sd * (float)(n - 1) / (float)n); M[4 * i + 2] = (float)n; M[4 * i + 3] = 0.0f;
  }
  b.source = 1;
  if (gtlDenoiseVariance(p) != GiStatus::Ok) { printf("gtlDenoiseVariance failed\n"); return 1; }
  std::vector<float> guided((const float*)giGetRenderBufferMem(b.output), (const float*)giGetRenderBufferMem(b.output) + 4 * w * h);
  if (gtlDenoise(b) != GiStatus::Ok) { printf("gtlDenoise failed\n"); return 1; } // the fixed filter over the same buffers, for comparison
  const float* F = (const float*)giGetRenderBufferMem(b.output);
  const float* O = guided.data();
  double before = 0.0, after = 0.0, moved = 0.0, movedFixed = 0.0;
  for (uint32_t i = 0; i < w * h; i++) {
    if (O[4 * i + 3] != 0.25f) { printf("alpha changed at %u\n", i); return 1; }
    if (i % w == 0) { if (memcmp(O + 4 * i, C + 4 * i, 16)) { printf("background pixel %u changed\n", i); return 1; } continue; }
    if (i % w < w / 2) { before += fabs(C[4 * i] - 0.5); after += fabs(O[4 * i] - 0.5); }
    else if (i % w >= w / 2 + 2) { moved = fmax(moved, fabs(O[4 * i] - 0.75)); movedFixed = fmax(movedFixed, fabs(F[4 * i] - 0.75)); }
  }
  if (!(after < 0.5 * before)) { printf("not denoised: %g -> %g\n", before, after); return 1; }
  if (!(moved < 0.1 * movedFixed)) { printf("the converged half moved by %g (fixed sigma: %g)\n", moved, movedFixed); return 1; }
  GtlDenoiseVarianceParams alias = p; alias.base.output = p.moments;
  if (gtlDenoiseVariance(alias) != GiStatus::Error) { printf("aliasing was accepted\n"); return 1; }
  giDestroyRenderBuffer(b.color); giDestroyRenderBuffer(b.normal); giDestroyRenderBuffer(b.depth); giDestroyRenderBuffer(b.output); giDestroyRenderBuffer(p.moments);
  giTerminate();
  printf("gtl_denoise_variance ok (%g -> %g, converged half moved %g, with the fixed sigma %g)\n", before, after, moved, movedFixed);
  return 0;
}
