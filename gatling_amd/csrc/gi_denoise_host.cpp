// gi_denoise_host.cpp -- giCDenoise (include/gi_c.h; DESIGN.md section 6 "Denoiser"): argument checks, where every input comes from, the library's scratch
// planes, the launches of gi_denoise.hip on the primary device's stream, and the host form (gi_denoise.h), which runs without a device.
#include "gi_host.h"

#include "gi_denoise.h"

namespace {

// The library's scratch on the primary device: the two ping-pong x planes and the guide plane, one staging plane per input sent from host memory (colour,
// normal, depth, albedo; allocated when one is first sent), and the events around the launches.  Allocated under g_ctx.resourceMutex, reused while the pixel
// count does not change, freed by giCTerminate.  g_denoiseMutex serialises the calls (the scratch and the statistics are the library's, not a scene's)
struct DenoiseScratch {
  DeviceBuffer<F4> x[2], guide, stage[5]; // (stage[4]: the moments, giCDenoiseVariance)
  DeviceBuffer<DnV> v[2];                 // the ping-pong V planes: allocated by the first giCDenoiseVariance, never by giCDenoise
  DeviceBuffer<float> vt;                 // GATLING_OPTIONS=denoise_form=3 alone: the vt plane of the direct-load passes
  size_t pixels = 0;
  static constexpr uint32_t EVENTS = 4u + kDenoiseMaxIterations; // start, sent, prepared, one per pass, copied
  hipEvent_t ev[EVENTS] = {};
  bool haveEvents = false;
  void release()
  {
    x[0].release(); x[1].release(); guide.release(); v[0].release(); v[1].release(); vt.release();
    for (auto& b : stage) b.release();
    pixels = 0;
    if (haveEvents) for (hipEvent_t& e : ev) { (void)hipEventDestroy(e); e = nullptr; }
    haveEvents = false;
  }
};
DenoiseScratch g_scratch;
std::mutex g_denoiseMutex;
GiCDenoiseStats g_denoiseStats{};

bool positiveFinite(float v) { return std::isfinite(v) && v > 0.0f; }

// `call`: the entry point the messages name
int refuse(const char* call, const std::string& what) { setError(std::string(call) + ": " + what); return GI_C_ERROR; }

int checkParams(const char* call, const GiCDenoiseParams* p)
{
  if (!p) return refuse(call, "null params");
  if (!p->color || !p->normal || !p->depth || !p->output) return refuse(call, "a required buffer (color, normal, depth, output) is NULL");
  const GiCRenderBuffer* all[] = {p->color, p->normal, p->depth, p->albedo, p->output};
  for (const GiCRenderBuffer* rb : all)
    if (rb && (rb->width != p->color->width || rb->height != p->color->height)) return refuse(call, "the buffers differ in size");
  const auto vec4 = [](const GiCRenderBuffer* rb) { return rb->format == GI_C_FORMAT_FLOAT32_VEC4 && rb->stride == 16u; };
  if (!vec4(p->color) || !vec4(p->normal) || !vec4(p->output) || (p->albedo && !vec4(p->albedo))) return refuse(call, "color, normal, albedo and output must be Float32Vec4 buffers");
  if (p->depth->format != GI_C_FORMAT_FLOAT32 || p->depth->stride != 4u) return refuse(call, "depth must be a Float32 buffer");
  const GiCRenderBuffer* inputs[] = {p->color, p->normal, p->depth, p->albedo};
  for (const GiCRenderBuffer* rb : inputs) if (rb == p->output) return refuse(call, "output aliases an input (inputs are never written: progressive accumulation reads the colour buffer back)");
  if (p->iterations < 1u || p->iterations > kDenoiseMaxIterations) return refuse(call, "iterations must lie in 1 .. 6");
  if (p->normalSquarings > kDenoiseMaxSquarings) return refuse(call, "normalSquarings must be at most 6");
  if (!positiveFinite(p->sigmaColor) || !positiveFinite(p->sigmaDepth) || !positiveFinite(p->albedoFloor)) return refuse(call, "sigmaColor, sigmaDepth and albedoFloor must be finite and positive");
  if (!std::isfinite(p->backgroundDepth)) return refuse(call, "backgroundDepth is not finite");
  if (p->source != GI_C_DENOISE_SOURCE_AUTO && p->source != GI_C_DENOISE_SOURCE_HOST && p->source != GI_C_DENOISE_SOURCE_HOST_FORM) return refuse(call, "unknown source");
  if (p->color->width > 65535u || p->color->height > 65535u) return refuse(call, "image dimensions exceed 65535");
  const float invSc0 = denoiseInvSc(p->sigmaColor, 0), invSz = 1.0f / p->sigmaDepth;
  if (!positiveFinite(invSc0) || !positiveFinite(denoiseInvSc(p->sigmaColor, p->iterations - 1u)) || !positiveFinite(invSz))
    return refuse(call, "a sigma is too small or too large for its reciprocal to be finite and positive");
  return GI_C_OK;
}

DenoisePass makePass(const GiCDenoiseParams* p, uint32_t i)
{
  DenoisePass P{};
  P.width = p->color->width; P.height = p->color->height; P.step = 1u << i; P.normalSquarings = p->normalSquarings;
  P.invSz = 1.0f / p->sigmaDepth; P.invSc = denoiseInvSc(p->sigmaColor, i); P.albedoFloor = p->albedoFloor; P.last = i + 1u == p->iterations ? 1u : 0u;
  return P;
}

// what giCDenoiseVariance adds to a call (null: the fixed-sigma filter)
struct VarianceArgs { GiCRenderBuffer* moments; float sv2, varianceFloor; uint32_t minSamples; };

int denoiseHostForm(const GiCDenoiseParams* p, const VarianceArgs* va, GiCDenoiseStats& S)
{
  const uint32_t w = p->color->width, h = p->color->height;
  const size_t n = (size_t)w * h;
  const F4* color = (const F4*)p->color->hostMem; const F4* normal = (const F4*)p->normal->hostMem; const float* depth = (const float*)p->depth->hostMem;
  const F4* albedo = p->albedo ? (const F4*)p->albedo->hostMem : nullptr;
  std::vector<F4> X[2], G(n);
  X[0].resize(n); X[1].resize(n);
  double t0 = nowMs();
  denoisePrepareHost(color, normal, depth, albedo, w, h, p->albedoFloor, p->backgroundDepth, X[0].data(), G.data());
  std::vector<DnV> V[2];
  if (va) {
    V[0].resize(n); V[1].resize(n);
    denoisePrepareVarianceHost(X[0].data(), (const F4*)va->moments->hostMem, albedo, w, h, p->albedoFloor, va->minSamples, V[0].data());
  }
  S.prepareMs = nowMs() - t0;
  for (uint32_t i = 0; i < p->iterations; i++) {
    const DenoisePass P = makePass(p, i);
    t0 = nowMs();
    F4* dst = P.last ? (F4*)p->output->hostMem : X[(i + 1u) & 1u].data();
    if (va) denoiseVarPassHost(DenoiseVarPass{P, va->sv2, va->varianceFloor}, X[i & 1u].data(), G.data(), V[i & 1u].data(), dst, V[(i + 1u) & 1u].data(), color, albedo);
    else denoisePassHost(P, X[i & 1u].data(), G.data(), dst, color, albedo);
    S.passMs[i] = nowMs() - t0;
  }
  S.source = GI_C_DENOISE_SOURCE_HOST_FORM;
  return GI_C_OK;
}

int denoiseOnDevice(const char* call, const GiCDenoiseParams* p, const VarianceArgs* va, GiCDenoiseStats& S)
{
  if (!g_ctx.initialized) return refuse(call, "before giCInitialize (only GI_C_DENOISE_SOURCE_HOST_FORM runs without a device)");
  if (p->output->hostOnly) return refuse(call, "output is a host render buffer: only GI_C_DENOISE_SOURCE_HOST_FORM can write it");
  GiCRenderBuffer* inputs[5] = {p->color, p->normal, p->depth, p->albedo, va ? va->moments : nullptr};
  bool send[5] = {false, false, false, false, false};
  for (uint32_t k = 0; k < 5u; k++) {
    GiCRenderBuffer* rb = inputs[k];
    if (!rb) continue;
    const bool fromDevice = p->source == GI_C_DENOISE_SOURCE_AUTO && rb->wholeFrame && !rb->hostOnly;
    if (!fromDevice && rb->deviceOnly && p->source == GI_C_DENOISE_SOURCE_AUTO)
      return refuse(call, "a deviceOnly input holds no whole frame (its last giCRender was a row share or a multi-device render, or it was never rendered)");
    send[k] = !fromDevice;
  }
  HIP_TRY(hipSetDevice(g_ctx.device));
  const uint32_t w = p->color->width, h = p->color->height;
  const size_t n = (size_t)w * h;
  DenoiseScratch& Z = g_scratch;
  {
    std::lock_guard<std::mutex> g(g_ctx.resourceMutex);
    if (Z.pixels != n) { HIP_TRY(hipStreamSynchronize(g_ctx.stream)); Z.x[0].release(); Z.x[1].release(); Z.guide.release(); Z.v[0].release(); Z.v[1].release(); Z.vt.release(); for (auto& b : Z.stage) b.release(); Z.pixels = n; }
    if (Z.x[0].alloc(n) || Z.x[1].alloc(n) || Z.guide.alloc(n)) { setError(std::string(call) + ": out of device memory (scratch planes)"); return GI_C_ERROR; }
    if (va && (Z.v[0].alloc(n) || Z.v[1].alloc(n) || (optionValue("denoise_form", 0) == 3 && Z.vt.alloc(n)))) { setError(std::string(call) + ": out of device memory (variance planes)"); return GI_C_ERROR; }
    for (uint32_t k = 0; k < 5u; k++)
      if (send[k] && Z.stage[k].alloc(k == 2u ? (n + 3u) / 4u : n)) { setError(std::string(call) + ": out of device memory (staging plane)"); return GI_C_ERROR; }
    if (!Z.haveEvents) {
      for (hipEvent_t& e : Z.ev) HIP_TRY(hipEventCreate(&e));
      Z.haveEvents = true;
    }
  }
  hipStream_t st = g_ctx.stream;
  const void* src[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  uint32_t e = 0;
  HIP_TRY(hipEventRecord(Z.ev[e++], st));
  for (uint32_t k = 0; k < 5u; k++) {
    GiCRenderBuffer* rb = inputs[k];
    if (!rb) continue;
    if (send[k]) {
      HIP_TRY(hipMemcpyAsync(Z.stage[k].ptr, rb->hostMem, rb->size, hipMemcpyHostToDevice, st));
      src[k] = Z.stage[k].ptr; S.sentInputs |= 1u << k; S.bytesSent += rb->size;
    } else { src[k] = rb->deviceMem; S.deviceInputs |= 1u << k; }
  }
  HIP_TRY(hipEventRecord(Z.ev[e++], st));
  const F4* color = (const F4*)src[0]; const F4* albedo = (const F4*)src[3];
  if (!launchDenoisePrepare(st, color, (const F4*)src[1], (const float*)src[2], albedo, w, h, p->albedoFloor, p->backgroundDepth, Z.x[0].ptr, Z.guide.ptr))
    return refuse(call, "k_denoise_prepare was not launched (bad arguments)");
  if (va && !launchDenoisePrepareVariance(st, Z.x[0].ptr, (const F4*)src[4], albedo, w, h, p->albedoFloor, va->minSamples, Z.v[0].ptr))
    return refuse(call, "k_denoise_prepare_var was not launched (bad arguments)");
  HIP_TRY(hipEventRecord(Z.ev[e++], st));
  const uint32_t form = (uint32_t)optionValue("denoise_form", 0);
  for (uint32_t i = 0; i < p->iterations; i++) {
    const DenoisePass P = makePass(p, i);
    F4* dst = P.last ? (F4*)p->output->deviceMem : Z.x[(i + 1u) & 1u].ptr;
    if (va ? !launchDenoiseVarPass(st, DenoiseVarPass{P, va->sv2, va->varianceFloor}, Z.x[i & 1u].ptr, Z.guide.ptr, Z.v[i & 1u].ptr, dst, Z.v[(i + 1u) & 1u].ptr, color, albedo, form, Z.vt.ptr)
           : !launchDenoisePass(st, P, Z.x[i & 1u].ptr, Z.guide.ptr, dst, color, albedo, form))
      return refuse(call, "k_denoise_pass was not launched (bad arguments)");
    HIP_TRY(hipEventRecord(Z.ev[e++], st));
  }
  HIP_TRY(hipGetLastError());
  if (!p->output->deviceOnly) HIP_TRY(hipMemcpyAsync(p->output->hostMem, p->output->deviceMem, p->output->size, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipEventRecord(Z.ev[e++], st));
  HIP_TRY(hipStreamSynchronize(st)); // the one host wait
  p->output->wholeFrame = false;     // (the device copy is the filtered image, not a render: a later AUTO call that takes it as an input sends host memory)
  float ms = 0.0f;
  uint32_t q = 0;
  HIP_TRY(hipEventElapsedTime(&ms, Z.ev[q], Z.ev[q + 1u])); S.sendMs = ms; q++;
  HIP_TRY(hipEventElapsedTime(&ms, Z.ev[q], Z.ev[q + 1u])); S.prepareMs = ms; q++;
  for (uint32_t i = 0; i < p->iterations; i++, q++) { HIP_TRY(hipEventElapsedTime(&ms, Z.ev[q], Z.ev[q + 1u])); S.passMs[i] = ms; }
  HIP_TRY(hipEventElapsedTime(&ms, Z.ev[q], Z.ev[q + 1u])); S.copyMs = p->output->deviceOnly ? 0.0 : ms;
  S.source = S.sentInputs ? GI_C_DENOISE_SOURCE_HOST : GI_C_DENOISE_SOURCE_AUTO;
  return GI_C_OK;
}

} // namespace

void releaseDenoiseScratch()
{
  std::lock_guard<std::mutex> g(g_ctx.resourceMutex);
  g_scratch.release();
}

extern "C" {

void giCDenoiseDefaults(GiCDenoiseParams* params)
{
  if (!params) return;
  *params = GiCDenoiseParams{};
  params->iterations = 5u; params->normalSquarings = 4u;
  params->sigmaColor = 2.0f; params->sigmaDepth = 0.02f; params->backgroundDepth = 1.0f; params->albedoFloor = 1.0e-3f;
  params->source = GI_C_DENOISE_SOURCE_AUTO;
}

static int runDenoise(const char* call, const GiCDenoiseParams* params, const VarianceArgs* va)
{
  std::lock_guard<std::mutex> g(g_denoiseMutex);
  try {
    GiCDenoiseStats S{};
    S.iterations = params->iterations; S.width = params->color->width; S.height = params->color->height;
    const double t0 = nowMs();
    if (S.width != 0u && S.height != 0u) { // (an empty image: nothing to do, as giCRender)
      const int rc = params->source == GI_C_DENOISE_SOURCE_HOST_FORM ? denoiseHostForm(params, va, S) : denoiseOnDevice(call, params, va, S);
      if (rc != GI_C_OK) return rc;
    } else S.source = params->source;
    S.totalMs = nowMs() - t0;
    g_denoiseStats = S;
  } catch (const std::exception& e) { setError(std::string(call) + ": " + e.what()); return GI_C_ERROR; }
  return GI_C_OK;
}

int giCDenoise(const GiCDenoiseParams* params)
{
  const char* call = "giCDenoise";
  if (checkParams(call, params) != GI_C_OK) return GI_C_ERROR;
  return runDenoise(call, params, nullptr);
}

void giCDenoiseVarianceDefaults(GiCDenoiseVarianceParams* params)
{
  if (!params) return;
  *params = GiCDenoiseVarianceParams{};
  giCDenoiseDefaults(&params->base);
  params->sigmaVariance = 4.0f; params->varianceFloor = 1.0e-6f; params->minSamples = 2u;
}

int giCDenoiseVariance(const GiCDenoiseVarianceParams* params)
{
  const char* call = "giCDenoiseVariance";
  if (!params) return refuse(call, "null params");
  if (checkParams(call, &params->base) != GI_C_OK) return GI_C_ERROR;
  const GiCDenoiseParams* p = &params->base;
  GiCRenderBuffer* m = params->moments;
  if (!m) return refuse(call, "moments is NULL (giCDenoise is the fixed-sigma filter)");
  if (m->format != GI_C_FORMAT_FLOAT32_VEC4 || m->stride != 16u) return refuse(call, "moments must be a Float32Vec4 buffer");
  if (m->width != p->color->width || m->height != p->color->height) return refuse(call, "the buffers differ in size (moments)");
  if (m == p->output) return refuse(call, "output aliases the moments (inputs are never written)");
  if (params->minSamples < 2u) return refuse(call, "minSamples must be at least 2 (a sample variance needs two samples)");
  if (!positiveFinite(params->sigmaVariance) || !positiveFinite(params->varianceFloor)) return refuse(call, "sigmaVariance and varianceFloor must be finite and positive");
  const float sv2 = params->sigmaVariance * params->sigmaVariance;
  if (!positiveFinite(sv2) || !positiveFinite(sv2 * params->varianceFloor)) return refuse(call, "sigmaVariance squared, times varianceFloor, is not finite and positive");
  const VarianceArgs va{m, sv2, params->varianceFloor, params->minSamples};
  return runDenoise(call, p, &va);
}

int giCGetDenoiseStats(GiCDenoiseStats* out)
{
  if (!out) { setError("giCGetDenoiseStats: null argument"); return GI_C_ERROR; }
  std::lock_guard<std::mutex> g(g_denoiseMutex);
  *out = g_denoiseStats;
  return GI_C_OK;
}

} // extern "C"
