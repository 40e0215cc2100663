// Kernel lab for the fused ConvNeXt MLP kernels (development aid, not part of the product library):
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I conette-audio-captioning_amd/csrc -I tools/lab tools/lab/mlp_lab.hip -o tools/lab/mlp_lab
//   tools/lab/mlp_lab [C] [batch] [iters]
// Checks every variant against a naive bf16-operand reference kernel on a small M (full tensors), then times it on
// the benchmark shape (batch x positions-per-clip rows) with HIP events, interleaved rounds.
#include <stdarg.h>
#include <math.h>
#include <stdlib.h>
#include <vector>
#include <string>
#include <algorithm>

#include "mlp_rc2.h"
#include "gelu_sig2.h"
#include "mlp_f8.h"
#include "mlp_rs.h"
#include "mlp_rs16.h"

void cn_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stderr, fmt, ap);
  va_end(ap);
  fprintf(stderr, "\n");
}

#define CK(x)                                                                      \
  do {                                                                             \
    hipError_t e_ = (x);                                                           \
    if (e_ != hipSuccess) {                                                        \
      fprintf(stderr, "%s:%d %s -> %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
      exit(1);                                                                     \
    }                                                                              \
  } while (0)

// naive reference: bf16 operands (y, W1, W2, hidden), fp32 accumulation, exact erf GELU
__global__ void ref_hidden(const bf16_t* Y, const float* W1, const float* b1, int C, int M, bf16_t* H) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)M * 4 * C) return;
  const int m = (int)(i / (4 * C)), n = (int)(i % (4 * C));
  float a = 0.f;
  for (int k = 0; k < C; ++k) a = fmaf((float)Y[(size_t)m * C + k], (float)(bf16_t)W1[(size_t)n * C + k], a);
  a += b1[n];
  H[i] = (bf16_t)(0.5f * a * (1.0f + erff(a * 0.70710678118654752440f)));
}
// folded = 1: LayerScale folded into the bf16 W2 operand (mlp_rc2.h): x += sum h * bf16(s W2) + s b2
__global__ void ref_out(const bf16_t* H, const float* W2, const float* b2, const float* scale, int C, int M, float* X, int folded) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)M * C) return;
  const int m = (int)(i / C), n = (int)(i % C);
  float a = 0.f;
  const float sc = scale[n];
  for (int k = 0; k < 4 * C; ++k) {
    const float w = W2[(size_t)n * 4 * C + k];
    a = fmaf((float)H[(size_t)m * 4 * C + k], (float)(bf16_t)(folded ? sc * w : w), a);
  }
  X[i] += folded ? a + sc * b2[n] : sc * (a + b2[n]);
}


// ---- FP8 (e4m3) variant: same quantisation points as mlp_rc2_f8.h, plain loops ----------------------------------------
__device__ __forceinline__ float q8(float v) {
  const int w = __builtin_amdgcn_cvt_pk_fp8_f32(v, 0.f, 0, false);
  return __builtin_amdgcn_cvt_f32_fp8(w, 0);
}
__global__ void to_fp8(const float* src, unsigned char* dst, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = (unsigned char)(__builtin_amdgcn_cvt_pk_fp8_f32(src[i], 0.f, 0, false) & 0xff);
}
__global__ void ref_hidden_f8(const unsigned char* Y, const float* W1, const float* b1, const float* aux, int C, int M, float* H) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)M * 4 * C) return;
  const int m = (int)(i / (4 * C)), n = (int)(i % (4 * C));
  const float is1 = aux[7 * C], s1 = 1.0f / is1;
  float a = 0.f;
  for (int k = 0; k < C; ++k) a = fmaf(__builtin_amdgcn_cvt_f32_fp8((int)Y[(size_t)m * C + k], 0), q8(s1 * W1[(size_t)n * C + k]), a);
  H[i] = q8(cn_gelu_sig2(fmaf(a, is1, b1[n])));
}
__global__ void ref_out_f8(const float* H, const float* W2, const float* ls, const float* aux, int C, int M, float* X) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)M * C) return;
  const int m = (int)(i / C), n = (int)(i % C);
  const float f = ls[n] * aux[5 * C + n];
  float a = X[i] * aux[5 * C + n];
  for (int k = 0; k < 4 * C; ++k) a = fmaf(H[(size_t)m * 4 * C + k], q8(f * W2[(size_t)n * 4 * C + k]), a);
  X[i] = fmaf(a, aux[4 * C + n], aux[6 * C + n]);
}

static int g_full = 0;
static uint32_t rng_state = 12345u;
static float frand() {  // uniform [-1, 1)
  rng_state = rng_state * 1664525u + 1013904223u;
  return (float)((rng_state >> 8) & 0xFFFFFF) / 8388608.0f - 1.0f;
}

template <typename T> static T* dalloc(size_t n) {
  T* p;
  CK(hipMalloc(&p, n * sizeof(T)));
  return p;
}

struct Variant {
  std::string name;
  int (*run)(const bf16_t* Y, const bf16_t* WS, void* X, int M, int nb, hipStream_t s);
  int pack = 1;  // mlp_rc2.h stream with NCK = 1 / 2; 4: role-split entries
  int xh = 0;    // 1: the residual stream is fp16 (round 5)
};
#define XF (float*)X
#define XH (half_t*)X

template <int C> static std::vector<Variant> variants();

template <> std::vector<Variant> variants<96>() {
  return {
      {"rc2_resident<96,8,nck2>",
       [](const bf16_t* Y, const bf16_t* WS, void* X, int M, int nb, hipStream_t s) { return cn_launch_mlp_rc2_resident<96, 8, 2>(Y, WS, XF, M, nb, s); }, 2},
      {"rc2_resident<96,8,nck1>",
       [](const bf16_t* Y, const bf16_t* WS, void* X, int M, int nb, hipStream_t s) { return cn_launch_mlp_rc2_resident<96, 8, 1>(Y, WS, XF, M, nb, s); }, 1},
      {"rc2_resident<96,12,nck1>",
       [](const bf16_t* Y, const bf16_t* WS, void* X, int M, int nb, hipStream_t s) { return cn_launch_mlp_rc2_resident<96, 12, 1>(Y, WS, XF, M, nb, s); }, 1},
      {"ABL rc2_resident<96,12> no residual loads",
       [](const bf16_t* Y, const bf16_t* WS, void* X, int M, int nb, hipStream_t s) { return cn_launch_mlp_rc2_resident<96, 12, 1, 1>(Y, WS, XF, M, nb, s); }, 1},
      {"ABL rc2_resident<96,12> no stores",
       [](const bf16_t* Y, const bf16_t* WS, void* X, int M, int nb, hipStream_t s) { return cn_launch_mlp_rc2_resident<96, 12, 1, 2>(Y, WS, XF, M, nb, s); }, 1},
      {"ABL rc2_resident<96,12> neither",
       [](const bf16_t* Y, const bf16_t* WS, void* X, int M, int nb, hipStream_t s) { return cn_launch_mlp_rc2_resident<96, 12, 1, 3>(Y, WS, XF, M, nb, s); }, 1},
      {"ABL rc2_resident<96,12> no global traffic at all",
       [](const bf16_t* Y, const bf16_t* WS, void* X, int M, int nb, hipStream_t s) { return cn_launch_mlp_rc2_resident<96, 12, 1, 11>(Y, WS, XF, M, nb, s); }, 1},
      {"x16 rc2_resident<96,12,nck1>",
       [](const bf16_t* Y, const bf16_t* WS, void* X, int M, int nb, hipStream_t s) { return cn_launch_mlp_rc2_resident<96, 12, 1>(Y, WS, XH, M, nb, s); }, 1, 1},
      {"x16 rc2_resident<96,8,nck1>",
       [](const bf16_t* Y, const bf16_t* WS, void* X, int M, int nb, hipStream_t s) { return cn_launch_mlp_rc2_resident<96, 8, 1>(Y, WS, XH, M, nb, s); }, 1, 1},
      {"x16 rc2_resident<96,8,nck2>",
       [](const bf16_t* Y, const bf16_t* WS, void* X, int M, int nb, hipStream_t s) { return cn_launch_mlp_rc2_resident<96, 8, 2>(Y, WS, XH, M, nb, s); }, 2, 1},
      {"ABL x16 rc2_resident<96,12> no residual loads",
       [](const bf16_t* Y, const bf16_t* WS, void* X, int M, int nb, hipStream_t s) { return cn_launch_mlp_rc2_resident<96, 12, 1, 1>(Y, WS, XH, M, nb, s); }, 1, 1},
      {"ABL x16 rc2_resident<96,12> no stores",
       [](const bf16_t* Y, const bf16_t* WS, void* X, int M, int nb, hipStream_t s) { return cn_launch_mlp_rc2_resident<96, 12, 1, 2>(Y, WS, XH, M, nb, s); }, 1, 1},
      {"ABL x16 rc2_resident<96,12> neither",
       [](const bf16_t* Y, const bf16_t* WS, void* X, int M, int nb, hipStream_t s) { return cn_launch_mlp_rc2_resident<96, 12, 1, 3>(Y, WS, XH, M, nb, s); }, 1, 1},
      {"ABL x16 rc2_resident<96,12> no global traffic at all",
       [](const bf16_t* Y, const bf16_t* WS, void* X, int M, int nb, hipStream_t s) { return cn_launch_mlp_rc2_resident<96, 12, 1, 11>(Y, WS, XH, M, nb, s); }, 1, 1},
      {"rs<96,np8,nst8>",
       [](const bf16_t* Y, const bf16_t* WS, void* X, int M, int nb, hipStream_t s) { return cn_launch_mlp_rs<96, 8, 8>(Y, WS, XF, M, nb, s); }, 4},
  };
}
template <> std::vector<Variant> variants<192>() {
  return {
      {"rc2_ring<192,8,nck1,nst5>",
       [](const bf16_t* Y, const bf16_t* WS, void* X, int M, int nb, hipStream_t s) { return cn_launch_mlp_rc2_ring<192, 8, 1, 5>(Y, WS, XF, M, nb, s); }, 1},
      {"rc2_ring<192,8,nck2,nst3>",
       [](const bf16_t* Y, const bf16_t* WS, void* X, int M, int nb, hipStream_t s) { return cn_launch_mlp_rc2_ring<192, 8, 2, 3>(Y, WS, XF, M, nb, s); }, 2},
      {"x16 rc2_ring<192,8,nck2,nst3>",
       [](const bf16_t* Y, const bf16_t* WS, void* X, int M, int nb, hipStream_t s) { return cn_launch_mlp_rc2_ring<192, 8, 2, 3>(Y, WS, XH, M, nb, s); }, 2, 1},
      {"x16 rc2_ring<192,8,nck1,nst5>",
       [](const bf16_t* Y, const bf16_t* WS, void* X, int M, int nb, hipStream_t s) { return cn_launch_mlp_rc2_ring<192, 8, 1, 5>(Y, WS, XH, M, nb, s); }, 1, 1},
      {"rs<192,np4,nst5>",
       [](const bf16_t* Y, const bf16_t* WS, void* X, int M, int nb, hipStream_t s) { return cn_launch_mlp_rs<192, 4, 5>(Y, WS, XF, M, nb, s); }, 4},
      {"rs<192,np8,nst5>",
       [](const bf16_t* Y, const bf16_t* WS, void* X, int M, int nb, hipStream_t s) { return cn_launch_mlp_rs<192, 8, 5>(Y, WS, XF, M, nb, s); }, 4},
  };
}
template <> std::vector<Variant> variants<384>() {
  return {
      {"rc2_ring<384,4,nck1,nst3>",
       [](const bf16_t* Y, const bf16_t* WS, void* X, int M, int nb, hipStream_t s) { return cn_launch_mlp_rc2_ring<384, 4, 1, 3>(Y, WS, XF, M, nb, s); }, 1},
      {"rs<384,np4,nst3>",
       [](const bf16_t* Y, const bf16_t* WS, void* X, int M, int nb, hipStream_t s) { return cn_launch_mlp_rs<384, 4, 3>(Y, WS, XF, M, nb, s); }, 4},
      {"x16 rs<384,np4,nst3>",
       [](const bf16_t* Y, const bf16_t* WS, void* X, int M, int nb, hipStream_t s) { return cn_launch_mlp_rs<384, 4, 3>(Y, WS, XH, M, nb, s); }, 4, 1},
      {"x16 rs<384> prio B",
       [](const bf16_t* Y, const bf16_t* WS, void* X, int M, int nb, hipStream_t s) { return cn_launch_mlp_rs<384, 4, 3, 8>(Y, WS, XH, M, nb, s); }, 4, 1},
      {"x16 rs16<384,np4,nst3>",
       [](const bf16_t* Y, const bf16_t* WS, void* X, int M, int nb, hipStream_t s) { return cn_launch_mlp_rs16<384, 4, 3>(Y, WS, XH, M, nb, s); }, 5, 1},
      {"x16 rs16<384> prio B",
       [](const bf16_t* Y, const bf16_t* WS, void* X, int M, int nb, hipStream_t s) { return cn_launch_mlp_rs16<384, 4, 3, 8>(Y, WS, XH, M, nb, s); }, 5, 1},
      {"ABL x16 rs16<384> none of the three",
       [](const bf16_t* Y, const bf16_t* WS, void* X, int M, int nb, hipStream_t s) { return cn_launch_mlp_rs16<384, 4, 3, 7>(Y, WS, XH, M, nb, s); }, 5, 1},
      {"x16 rs<384> prio A",
       [](const bf16_t* Y, const bf16_t* WS, void* X, int M, int nb, hipStream_t s) { return cn_launch_mlp_rs<384, 4, 3, 16>(Y, WS, XH, M, nb, s); }, 4, 1},
      {"ABL x16 rs<384> no DMA",
       [](const bf16_t* Y, const bf16_t* WS, void* X, int M, int nb, hipStream_t s) { return cn_launch_mlp_rs<384, 4, 3, 1>(Y, WS, XH, M, nb, s); }, 4, 1},
      {"ABL x16 rs<384> no GELU",
       [](const bf16_t* Y, const bf16_t* WS, void* X, int M, int nb, hipStream_t s) { return cn_launch_mlp_rs<384, 4, 3, 2>(Y, WS, XH, M, nb, s); }, 4, 1},
      {"ABL x16 rs<384> no tile I/O",
       [](const bf16_t* Y, const bf16_t* WS, void* X, int M, int nb, hipStream_t s) { return cn_launch_mlp_rs<384, 4, 3, 4>(Y, WS, XH, M, nb, s); }, 4, 1},
      {"ABL x16 rs<384> none of the three",
       [](const bf16_t* Y, const bf16_t* WS, void* X, int M, int nb, hipStream_t s) { return cn_launch_mlp_rs<384, 4, 3, 7>(Y, WS, XH, M, nb, s); }, 4, 1},
      {"x16 rc2_ring<384,4,nck1,nst3>",
       [](const bf16_t* Y, const bf16_t* WS, void* X, int M, int nb, hipStream_t s) { return cn_launch_mlp_rc2_ring<384, 4, 1, 3>(Y, WS, XH, M, nb, s); }, 1, 1},
      {"rs<384> prio B",
       [](const bf16_t* Y, const bf16_t* WS, void* X, int M, int nb, hipStream_t s) { return cn_launch_mlp_rs<384, 4, 3, 8>(Y, WS, XF, M, nb, s); }, 4},
      {"rs<384> prio A",
       [](const bf16_t* Y, const bf16_t* WS, void* X, int M, int nb, hipStream_t s) { return cn_launch_mlp_rs<384, 4, 3, 16>(Y, WS, XF, M, nb, s); }, 4},
      {"ABL rs<384> one barrier per step (racy)",
       [](const bf16_t* Y, const bf16_t* WS, void* X, int M, int nb, hipStream_t s) { return cn_launch_mlp_rs<384, 4, 3, 32>(Y, WS, XF, M, nb, s); }, 4},
      {"ABL rs<384> no DMA",
       [](const bf16_t* Y, const bf16_t* WS, void* X, int M, int nb, hipStream_t s) { return cn_launch_mlp_rs<384, 4, 3, 1>(Y, WS, XF, M, nb, s); }, 4},
      {"ABL rs<384> no GELU",
       [](const bf16_t* Y, const bf16_t* WS, void* X, int M, int nb, hipStream_t s) { return cn_launch_mlp_rs<384, 4, 3, 2>(Y, WS, XF, M, nb, s); }, 4},
      {"ABL rs<384> no tile I/O",
       [](const bf16_t* Y, const bf16_t* WS, void* X, int M, int nb, hipStream_t s) { return cn_launch_mlp_rs<384, 4, 3, 4>(Y, WS, XF, M, nb, s); }, 4},
      {"ABL rs<384> none of the three",
       [](const bf16_t* Y, const bf16_t* WS, void* X, int M, int nb, hipStream_t s) { return cn_launch_mlp_rs<384, 4, 3, 7>(Y, WS, XF, M, nb, s); }, 4},
  };
}

template <int C> static int run(int batch, int iters) {
  const int pos_per_clip = C == 96 ? 252 * 56 : C == 192 ? 126 * 28 : 63 * 14;
  const int M = batch * pos_per_clip;
  const int Mc = 4096 + 19;  // check size (ragged last tile)
  printf("== C = %d, M = %d (batch %d), check M = %d\n", C, M, batch, Mc);
  std::vector<float> hW1((size_t)4 * C * C), hW2((size_t)4 * C * C), hb1(4 * C), hb2(C), hsc(C);
  const float s1 = 1.7f / sqrtf((float)C), s2 = 1.7f / sqrtf(4.0f * C);
  for (auto& v : hW1) v = frand() * s1;
  for (auto& v : hW2) v = frand() * s2;
  for (auto& v : hb1) v = frand() * 0.5f;
  for (auto& v : hb2) v = frand() * 0.5f;
  for (auto& v : hsc) v = 0.1f + 0.4f * fabsf(frand());
  std::vector<bf16_t> hY((size_t)(M + 64) * C);
  std::vector<float> hX((size_t)M * C);
  for (auto& v : hY) v = (bf16_t)(frand() * 1.5f);
  for (auto& v : hX) v = (float)(half_t)frand();  // (representable in fp16: the fp32 and fp16 residual streams start from the same numbers)
  float *W1 = dalloc<float>(hW1.size()), *W2 = dalloc<float>(hW2.size()), *b1 = dalloc<float>(4 * C), *b2 = dalloc<float>(C),
        *sc = dalloc<float>(C);
  bf16_t* Y = dalloc<bf16_t>(hY.size());
  half_t* Xh = dalloc<half_t>(hX.size() + 64 * C);
  std::vector<half_t> hXh(hX.size() + 64 * C);
  for (size_t i = 0; i < hXh.size(); ++i) hXh[i] = (half_t)(i < hX.size() ? hX[i] : 0.f);
  float *X = dalloc<float>(hX.size() + 64 * C), *Xref = dalloc<float>((size_t)Mc * C), *Xref2 = dalloc<float>((size_t)Mc * C);
  bf16_t* H = dalloc<bf16_t>((size_t)Mc * 4 * C);
  bf16_t* WS2[6] = {nullptr, dalloc<bf16_t>(Rc2Geom<C, 1>::TOTAL_BYTES / 2), dalloc<bf16_t>(Rc2Geom<C, 2>::TOTAL_BYTES / 2),
                    dalloc<bf16_t>(Rc2Geom<C, 1>::TOTAL_BYTES / 2), dalloc<bf16_t>(Rc2Geom<C, 1>::TOTAL_BYTES / 2),
                    dalloc<bf16_t>(Rs16Geom<C>::TOTAL_BYTES / 2)};  // [5]: role-split entries for the 16x16x32 kernel; [3]: NCK = 1, skewed entries; [4]: role-split entries
  CK(hipMemcpy(W1, hW1.data(), hW1.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(W2, hW2.data(), hW2.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(b1, hb1.data(), 4 * C * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(b2, hb2.data(), C * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(sc, hsc.data(), C * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(Y, hY.data(), hY.size() * 2, hipMemcpyHostToDevice));
  {
    for (int nck = 1; nck <= 2; ++nck) {
      const int u2 = ((C / 8) * (C / 8 + 1) + C / 32) * 64;
      hipLaunchKernelGGL(pk_mlp_rc2, dim3((u2 + 255) / 256), dim3(256), 0, 0, W1, b1, W2, b2, sc, C, nck, WS2[nck]);
    }
    const int u3 = ((C / 8) * (C / 8 + 1) + C / 32) * 64;
    hipLaunchKernelGGL(pk_mlp_rs, dim3((u3 + 255) / 256), dim3(256), 0, 0, W1, b1, W2, b2, sc, C, WS2[4]);
    const int u5 = Rs16Geom<C>::NCH * Rs16Geom<C>::FR * 64;
    hipLaunchKernelGGL(pk_mlp_rs16, dim3((u5 + 255) / 256), dim3(256), 0, 0, W1, b1, W2, b2, sc, C, WS2[5]);
  }
  // reference on the first Mc rows
  CK(hipMemcpy(Xref, hX.data(), (size_t)Mc * C * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(ref_hidden, dim3((unsigned)(((long)Mc * 4 * C + 255) / 256)), dim3(256), 0, 0, Y, W1, b1, C, Mc, H);
  hipLaunchKernelGGL(ref_out, dim3((unsigned)(((long)Mc * C + 255) / 256)), dim3(256), 0, 0, H, W2, b2, sc, C, Mc, Xref, 0);
  CK(hipMemcpy(Xref2, hX.data(), (size_t)Mc * C * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(ref_out, dim3((unsigned)(((long)Mc * C + 255) / 256)), dim3(256), 0, 0, H, W2, b2, sc, C, Mc, Xref2, 1);
  CK(hipDeviceSynchronize());
  std::vector<float> href0((size_t)Mc * C), href1((size_t)Mc * C), hgot((size_t)(Mc + 64) * C);
  CK(hipMemcpy(href0.data(), Xref, href0.size() * 4, hipMemcpyDeviceToHost));
  CK(hipMemcpy(href1.data(), Xref2, href1.size() * 4, hipMemcpyDeviceToHost));

  auto vs = variants<C>();
  int bad = 0;
  for (int nbc : {256, 5, 3})
  for (auto& v : vs) {
    if (v.xh) {
      CK(hipMemcpy(Xh, hXh.data(), (size_t)(Mc + 64) * C * 2, hipMemcpyHostToDevice));
      if (v.run(Y, WS2[v.pack], Xh, Mc, nbc, 0) != CN_OK) return 1;
      CK(hipDeviceSynchronize());
      std::vector<half_t> hg((size_t)(Mc + 64) * C);
      CK(hipMemcpy(hg.data(), Xh, hg.size() * 2, hipMemcpyDeviceToHost));
      for (size_t i = 0; i < hg.size(); ++i) hgot[i] = (float)hg[i];
    } else {
    CK(hipMemcpy(X, hX.data(), (size_t)(Mc + 64) * C * 4, hipMemcpyHostToDevice));
    if (v.run(Y, WS2[v.pack], X, Mc, nbc, 0) != CN_OK) return 1;
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(hgot.data(), X, hgot.size() * 4, hipMemcpyDeviceToHost));
    }
    const std::vector<float>& href = href1;  // LayerScale folded into the bf16 W2 operand
    double max_err = 0, sum_err = 0, max_ref = 0;
    size_t n_bad = 0;
    for (size_t i = 0; i < href.size(); ++i) {
      const double e = fabs((double)hgot[i] - href[i]);
      max_err = std::max(max_err, e);
      sum_err += e;
      max_ref = std::max(max_ref, (double)fabs(href[i] - hX[i]));
      if (e > (v.xh ? 2e-3 : 1e-3) + 1e-3 * fabs(href[i])) ++n_bad;
    }
    size_t touched = 0;  // rows beyond Mc must be untouched
    for (size_t i = href.size(); i < hgot.size(); ++i) touched += hgot[i] != (i < hX.size() ? hX[i] : 0.f);
    if (v.name.rfind("ABL", 0) == 0 || v.name.find("prio") != std::string::npos) continue;
    printf("  check nb %3d %-30s max|err| %.3e  mean %.3e  (max |delta| %.3f)  out-of-tol %zu  rows>=M touched %zu  %s\n", nbc, v.name.c_str(),
           max_err, sum_err / href.size(), max_ref, n_bad, touched, (n_bad == 0 && touched == 0) ? "OK" : "FAIL");
    bad += (n_bad != 0 || touched != 0);
  }

  // timing: interleaved rounds
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  CK(hipMemcpy(X, hX.data(), hX.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(Xh, hXh.data(), hXh.size() * 2, hipMemcpyHostToDevice));
  std::vector<std::vector<float>> times(vs.size());
  const double flops = 16.0 * C * C * (double)M;
  for (int round = 0; round < 5; ++round)
    for (size_t vi = 0; vi < vs.size(); ++vi) {
      void* Xv = vs[vi].xh ? (void*)Xh : (void*)X;
      vs[vi].run(Y, WS2[vs[vi].pack], Xv, M, 256, 0);  // warm
      CK(hipEventRecord(e0, 0));
      for (int it = 0; it < iters; ++it) vs[vi].run(Y, WS2[vs[vi].pack], Xv, M, 256, 0);
      CK(hipEventRecord(e1, 0));
      CK(hipEventSynchronize(e1));
      float ms;
      CK(hipEventElapsedTime(&ms, e0, e1));
      times[vi].push_back(ms * 1000.0f / iters);
    }
  for (size_t vi = 0; vi < vs.size(); ++vi) {
    std::sort(times[vi].begin(), times[vi].end());
    const double med = times[vi][times[vi].size() / 2], mn = times[vi][0];
    printf("  time  %-34s median %8.1f us  min %8.1f us  -> %7.1f TFLOP/s (%.3f of 2.5 PF)\n", vs[vi].name.c_str(), med, mn,
           flops / med * 1e-6, flops / med * 1e-6 / 2500.0);
  }
  // phase profile of the ring kernels (separate instrumented instantiation)
  if constexpr (C != 96) {
    unsigned long long* prof = dalloc<unsigned long long>(8);
    CK(hipMemset(prof, 0, 64));
    if constexpr (C == 192) cn_launch_mlp_rc2_ring<192, 8, 1, 5, 1>(Y, WS2[1], X, M, 256, 0, prof);
    else cn_launch_mlp_rc2_ring<384, 4, 1, 3, 1>(Y, WS2[1], X, M, 256, 0, prof);
    CK(hipDeviceSynchronize());
    unsigned long long h[8];
    CK(hipMemcpy(h, prof, 64, hipMemcpyDeviceToHost));
    const char* nm[5] = {"wait DMA", "barrier", "DMA issue (+ tile init)", "step compute", "tile boundary / loop"};
    const double n = (double)h[5];
    printf("  phase profile (cycles per valid wave-step, %llu wave-steps):\n", h[5]);
    for (int i = 0; i < 5; ++i) printf("    %-26s %9.1f\n", nm[i], h[i] / n);
  }

  // ---- FP8 variant (only with a 4th argument) -----------------------------------------------------------------------
  if (g_full) {
    typedef Rc2F8Geom<C> G8;
    char* WS8 = dalloc<char>(G8::TOTAL_BYTES);
    if (cn_pack_mlp_f8(W1, b1, W2, b2, sc, C, WS8, 0) != CN_OK) return 1;
    const float* aux8 = (const float*)(WS8 + G8::STREAM_BYTES);
    float* Yf = dalloc<float>(hY.size());
    std::vector<float> hYf(hY.size());
    for (size_t i = 0; i < hY.size(); ++i) hYf[i] = (float)hY[i];
    CK(hipMemcpy(Yf, hYf.data(), hYf.size() * 4, hipMemcpyHostToDevice));
    unsigned char* Y8 = dalloc<unsigned char>(hY.size());
    hipLaunchKernelGGL(to_fp8, dim3((unsigned)((hY.size() + 255) / 256)), dim3(256), 0, 0, Yf, Y8, hY.size());
    float* H8 = dalloc<float>((size_t)Mc * 4 * C);
    CK(hipMemcpy(Xref, hX.data(), (size_t)Mc * C * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(ref_hidden_f8, dim3((unsigned)(((long)Mc * 4 * C + 255) / 256)), dim3(256), 0, 0, Y8, W1, b1, aux8, C, Mc, H8);
    hipLaunchKernelGGL(ref_out_f8, dim3((unsigned)(((long)Mc * C + 255) / 256)), dim3(256), 0, 0, H8, W2, sc, aux8, C, Mc, Xref);
    CK(hipDeviceSynchronize());
    std::vector<float> href8((size_t)Mc * C);
    CK(hipMemcpy(href8.data(), Xref, href8.size() * 4, hipMemcpyDeviceToHost));
    auto run8 = [&](float* Xp, int Mr, int nb) -> int {
      if constexpr (C == 96) return cn_launch_mlp_f8_resident<96, 12>(Y8, WS8, Xp, Mr, nb, 0);
      else if constexpr (C == 192) return cn_launch_mlp_f8_ring<192, 8, 5>(Y8, WS8, Xp, Mr, nb, 0);
      else return cn_launch_mlp_f8_ring<384, 4, 4>(Y8, WS8, Xp, Mr, nb, 0);
    };
    for (int nbc : {256, 5}) {
      CK(hipMemcpy(X, hX.data(), (size_t)(Mc + 64) * C * 4, hipMemcpyHostToDevice));
      if (run8(X, Mc, nbc) != CN_OK) return 1;
      CK(hipDeviceSynchronize());
      CK(hipMemcpy(hgot.data(), X, hgot.size() * 4, hipMemcpyDeviceToHost));
      double max_err = 0, sum_err = 0, dev_bf16 = 0, ref_mag = 0;
      size_t n_bad = 0, touched = 0;
      for (size_t i = 0; i < href8.size(); ++i) {
        const double e = fabs((double)hgot[i] - href8[i]);
        max_err = std::max(max_err, e);
        sum_err += e;
        if (!(e <= 2e-3 + 2e-3 * fabs(href8[i]))) ++n_bad;
        dev_bf16 += fabs((double)hgot[i] - href1[i]);
        ref_mag += fabs((double)href1[i] - hX[i]);
      }
      for (size_t i = href8.size(); i < hgot.size(); ++i) touched += hgot[i] != hX[i];
      printf("  check nb %3d fp8 kernel vs fp8-operand reference: max|err| %.3e mean %.3e out-of-tol %zu (%.4f %%) rows>=M touched %zu %s;"
             "  vs bf16-operand reference: mean|diff| %.3e = %.2f %% of mean|delta|\n", nbc, max_err, sum_err / href8.size(), n_bad,
             100.0 * n_bad / href8.size(), touched, (n_bad <= href8.size() / 2000 && touched == 0) ? "OK" : "FAIL", dev_bf16 / href8.size(),
             100.0 * dev_bf16 / ref_mag);
      bad += !(n_bad <= href8.size() / 2000 && touched == 0);
    }
    CK(hipMemcpy(X, hX.data(), hX.size() * 4, hipMemcpyHostToDevice));
    std::vector<float> ts;
    for (int round = 0; round < 5; ++round) {
      run8(X, M, 256);
      CK(hipEventRecord(e0, 0));
      for (int it = 0; it < iters; ++it) run8(X, M, 256);
      CK(hipEventRecord(e1, 0));
      CK(hipEventSynchronize(e1));
      float ms;
      CK(hipEventElapsedTime(&ms, e0, e1));
      ts.push_back(ms * 1000.0f / iters);
    }
    std::sort(ts.begin(), ts.end());
    printf("  time  fp8 %-30s median %8.1f us  min %8.1f us  -> %7.1f TFLOP/s (%.3f of 5 PF)\n", "", ts[2], ts[0], flops / ts[2] * 1e-6,
           flops / ts[2] * 1e-6 / 5000.0);
  }
  return bad;
}

int main(int argc, char** argv) {
  const int C = argc > 1 ? atoi(argv[1]) : 96;
  const int batch = argc > 2 ? atoi(argv[2]) : 64;
  const int iters = argc > 3 ? atoi(argv[3]) : 10;
  g_full = argc > 4;
  if (C == 96) return run<96>(batch, iters);
  if (C == 192) return run<192>(batch, iters);
  if (C == 384) return run<384>(batch, iters);
  fprintf(stderr, "C must be 96, 192 or 384\n");
  return 2;
}
