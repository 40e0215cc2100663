// Tag timeline: conette_tag_frames / conette_tag_events (include/conette_hip.h).  The rule both are held to is stated in
// conette_amd/tagging.py.
//
//   cn_window_pool_ln_kernel  the clip head's pooling (max over time + mean over time, LayerNorm) over a window of frames around
//                             every frame t instead of over the whole clip: one row of GEMM operands per frame.  The head itself
//                             is the clip head's cn_mm with M = B T rows
//   cn_tag_zero_rows_kernel   rows t >= n of the probabilities become exact zeros (the GEMM leaves sigmoid(bias) there)
//   cn_tag_events_kernel      hysteresis thresholding, gap merging and the minimum length for every (clip, tag) sequence, one
//                             thread each, in one walk over the frames; compared in fp32, so it is exact
#pragma once
#include <type_traits>

#include "common.h"

#define CN_TAG_TT 8   // output frames per block of the window kernel and of the zero pass

// Grid (ceil(Tn / CN_TAG_TT), B), 256 threads; thread tid owns channels tid, tid + 256, tid + 512 as cn_clip_pool_ln_kernel does.
// Every frame's window [a, e) = [max(0, t - lo), min(n, t + hi + 1)) is recomputed from the frame embeddings (L2-resident: a
// clip's are Tn x 3 KB), summed in ascending frame order in fp32; nothing is carried from frame to frame, so the order of every sum
// is fixed by (t, n, window) alone.  e <= n <= Tn: no frame at or beyond the clip's length is read.  Rows t >= n get zero operands
// (defined input for the GEMM; cn_tag_zero_rows_kernel overwrites what it makes of them).
template <typename T>
__global__ __launch_bounds__(256) void cn_window_pool_ln_kernel(const float* __restrict__ fe, const int32_t* __restrict__ lens,
                                                                int Tn, int lo, int hi, const float* __restrict__ ln_w,
                                                                const float* __restrict__ ln_b, T* __restrict__ out) {
  __shared__ float s_red[8];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int n = min(max(lens[b], 0), Tn);
  const int t0 = blockIdx.x * CN_TAG_TT, t1 = min(t0 + CN_TAG_TT, Tn);
  const float* clip = fe + (size_t)b * Tn * CN_FEAT + tid;
  float gw[3], gb[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    gw[i] = ln_w[tid + 256 * i];
    gb[i] = ln_b[tid + 256 * i];
  }
  for (int t = t0; t < t1; ++t) {
    T* o = out + ((size_t)b * Tn + t) * CN_FEAT + tid;
    if (t >= n) {  // (the same in every thread of the block)
#pragma unroll
      for (int i = 0; i < 3; ++i) o[256 * i] = cn_from_f32<T>(0.0f);
      continue;
    }
    const int a = max(0, t - lo), e = min(n, t + hi + 1);
    float mx[3] = {-INFINITY, -INFINITY, -INFINITY}, sm[3] = {0.f, 0.f, 0.f};
    int u = a;
    for (; u + 8 <= e; u += 8) {  // 24 loads in flight, then the sums in ascending frame order
      float x[8][3];
#pragma unroll
      for (int k = 0; k < 8; ++k)
#pragma unroll
        for (int i = 0; i < 3; ++i) x[k][i] = clip[(size_t)(u + k) * CN_FEAT + 256 * i];
#pragma unroll
      for (int k = 0; k < 8; ++k)
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          mx[i] = fmaxf(mx[i], x[k][i]);
          sm[i] += x[k][i];
        }
    }
    for (; u < e; ++u) {
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const float x = clip[(size_t)u * CN_FEAT + 256 * i];
        mx[i] = fmaxf(mx[i], x);
        sm[i] += x;
      }
    }
    float v[3];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      v[i] = mx[i] + sm[i] / (float)(e - a);
      s += v[i];
    }
    // (s_red[0..3] / [4..7] are rewritten one barrier after every thread has read them: no barrier between frames is needed)
    s = cn_wave_sum(s);
    if ((tid & 63) == 0) s_red[tid >> 6] = s;
    __syncthreads();
    const float mean = (s_red[0] + s_red[1] + s_red[2] + s_red[3]) * (1.0f / CN_FEAT);
    float s2 = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const float d = v[i] - mean;
      s2 = fmaf(d, d, s2);
    }
    s2 = cn_wave_sum(s2);
    if ((tid & 63) == 0) s_red[4 + (tid >> 6)] = s2;
    __syncthreads();
    const float rstd = 1.0f / sqrtf((s_red[4] + s_red[5] + s_red[6] + s_red[7]) * (1.0f / CN_FEAT) + 1e-6f);
#pragma unroll
    for (int i = 0; i < 3; ++i) o[256 * i] = cn_from_f32<T>((v[i] - mean) * rstd * gw[i] + gb[i]);
  }
}

// Grid (ceil(Tn / CN_TAG_TT), B): rows max(n, t0) .. min(Tn, t0 + CN_TAG_TT) of clip b are one contiguous range of `probs`.
__global__ __launch_bounds__(256) void cn_tag_zero_rows_kernel(float* __restrict__ probs, const int32_t* __restrict__ lens, int Tn,
                                                               int n_tags) {
  const int b = blockIdx.y;
  const int n = min(max(lens[b], 0), Tn);
  const int t0 = max(n, (int)blockIdx.x * CN_TAG_TT), t1 = min((int)blockIdx.x * CN_TAG_TT + CN_TAG_TT, Tn);
  if (t0 >= t1) return;
  float* p = probs + ((size_t)b * Tn + t0) * n_tags;
  const int count = (t1 - t0) * n_tags;
  for (int i = threadIdx.x; i < count; i += 256) p[i] = 0.0f;
}

struct CnTagEventsArgs {
  const float* probs;     // (B, T, C)
  const int32_t* lens;    // (B)
  int batch, t_audio, n_tags;
  float on, off;
  int min_frames, max_gap, max_events;
  int32_t* spans;         // (B, C, max_events, 2)
  float* peaks;           // (B, C, max_events)
  int32_t* peak_frames;   // (B, C, max_events)
  int32_t* counts;        // (B, C)
};

// One thread per (clip, tag), consecutive threads on consecutive tags: the load of p[b, t, c] is coalesced at every step.  A thread
// keeps the current run [rs, t) (its peak, and whether it has reached `on`), the pending merged event [es, ee) and the number of
// events so far in registers; an event goes out when a later run does not join it, or at the end.  Every slot of the four outputs is
// written: the unused ones with (-1, -1), 0 and -1.
__global__ __launch_bounds__(256) void cn_tag_events_kernel(CnTagEventsArgs a) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)a.batch * a.n_tags) return;
  const int b = (int)(idx / a.n_tags), c = (int)(idx - (long)b * a.n_tags);
  const int n = min(max(a.lens[b], 0), a.t_audio);
  const size_t C = (size_t)a.n_tags;
  const float* p = a.probs + (size_t)b * a.t_audio * C + c;
  int32_t* spans = a.spans + (size_t)idx * a.max_events * 2;
  float* peaks = a.peaks + (size_t)idx * a.max_events;
  int32_t* peak_frames = a.peak_frames + (size_t)idx * a.max_events;
  int count = 0;
  bool in_run = false, hit = false, pend = false;
  int rs = 0, rpf = 0, es = 0, ee = 0, epf = 0;
  float rpk = 0.f, epk = 0.f;
  auto emit = [&]() {
    if (ee - es >= a.min_frames) {
      if (count < a.max_events) {
        spans[2 * count] = es;
        spans[2 * count + 1] = ee;
        peaks[count] = epk;
        peak_frames[count] = epf;
      }
      ++count;
    }
  };
  auto close = [&](int t) {  // the run [rs, t) has ended
    if (hit) {
      if (pend && rs - ee <= a.max_gap) {
        ee = t;
        if (rpk > epk) {
          epk = rpk;
          epf = rpf;
        }
      } else {
        if (pend) emit();
        es = rs;
        ee = t;
        epk = rpk;
        epf = rpf;
        pend = true;
      }
    }
    in_run = false;
  };
  auto step = [&](int t, float x) {
    if (x >= a.off) {  // (false for a NaN)
      if (!in_run) {
        in_run = true;
        hit = false;
        rs = t;
        rpk = x;
        rpf = t;
      } else if (x > rpk) {
        rpk = x;
        rpf = t;
      }
      hit |= x >= a.on;
    } else if (in_run) {
      close(t);
    }
  };
  // the walk is a chain of load round trips (a long recording: 1875 frames in 3 blocks of threads): 16 loads in flight while the
  // frames last, then 4, then 1
  int t = 0;
  auto walk = [&](auto width) {
    constexpr int K = decltype(width)::value;
    for (; t + K <= n; t += K) {
      float x[K];
#pragma unroll
      for (int k = 0; k < K; ++k) x[k] = p[(size_t)(t + k) * C];
#pragma unroll
      for (int k = 0; k < K; ++k) step(t + k, x[k]);
    }
  };
  walk(std::integral_constant<int, 16>{});
  walk(std::integral_constant<int, 4>{});
  walk(std::integral_constant<int, 1>{});
  if (in_run) close(n);
  if (pend) emit();
  a.counts[idx] = count;
  for (int k = min(count, a.max_events); k < a.max_events; ++k) {
    spans[2 * k] = -1;
    spans[2 * k + 1] = -1;
    peaks[k] = 0.0f;
    peak_frames[k] = -1;
  }
}
