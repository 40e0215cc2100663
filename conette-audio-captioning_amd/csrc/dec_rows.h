// The row-wise decoder kernels, one wave per row (d_model == 256): operand conversion, embedding, LayerNorm, the KV-cached
// self-attention of the step path, cross-attention, the causal self-attention of the one-pass teacher forcing, and the small
// kernels that feed the step loop with a given caption.  Launched by decode_impl / dec_sublayer_layer / forcing_prefill_impl
// (decoder.hip); dec_align.h reuses the load / dot / online-softmax helpers.
#pragma once

template <typename T>
__global__ void cn_cvt_kernel(const float* __restrict__ in, T* __restrict__ out, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    out[i] = cn_from_f32<T>(in[i]);
}

// x = E[tok] * sqrt(d) + PE[pos]   (aac_tfmer.py:100-106); d == 256, one wave per row.  The step path (cap_len == 0) embeds every
// row's current token at position `step`; the one-pass teacher forcing embeds row r = caption * cap_len + position at r % cap_len.
template <typename T>
__global__ __launch_bounds__(256) void cn_embed_kernel(const int* __restrict__ tok, const float* __restrict__ emb,
                                                       const float* __restrict__ pe, int step, int cap_len, int R, float scale,
                                                       float* __restrict__ x, T* __restrict__ xt) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= R) return;
  const int pos = cap_len > 0 ? r % cap_len : step;
  const f32x4 e = *(const f32x4*)(emb + (size_t)tok[r] * 256 + 4 * lane);
  const f32x4 p = *(const f32x4*)(pe + (size_t)pos * 256 + 4 * lane);
  f32x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = e[i] * scale + p[i];
  *(f32x4*)(x + (size_t)r * 256 + 4 * lane) = o;
  cn_store4(xt + (size_t)r * 256 + 4 * lane, o[0], o[1], o[2], o[3]);
}

// x = LayerNorm(sum of nslab partial slabs [+ bias + residual]) (eps 1e-5, d == 256); one wave per row.
// With nslab == 1 and no bias / residual this is the plain LayerNorm of a finished GEMM output.
template <typename T>
__global__ __launch_bounds__(256) void cn_ln256_kernel(const float* __restrict__ in, int nslab, size_t slab_stride,
                                                       const float* __restrict__ bias,
                                                       const float* __restrict__ resid, const float* __restrict__ w,
                                                       const float* __restrict__ b, int R, float* __restrict__ x,
                                                       T* __restrict__ xt) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= R) return;
  f32x4 v = *(const f32x4*)(in + (size_t)r * 256 + 4 * lane);
  for (int sl = 1; sl < nslab; ++sl) {
    const f32x4 u = *(const f32x4*)(in + sl * slab_stride + (size_t)r * 256 + 4 * lane);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] += u[i];
  }
  if (bias) {
    const f32x4 u = *(const f32x4*)(bias + 4 * lane);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] += u[i];
  }
  if (resid) {
    const f32x4 u = *(const f32x4*)(resid + (size_t)r * 256 + 4 * lane);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] += u[i];
  }
  const float mean = cn_wave_sum(v[0] + v[1] + v[2] + v[3]) * (1.0f / 256.0f);
  float s2 = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) s2 = fmaf(v[i] - mean, v[i] - mean, s2);
  const float rstd = 1.0f / sqrtf(cn_wave_sum(s2) * (1.0f / 256.0f) + 1e-5f);
  const f32x4 ww = *(const f32x4*)(w + 4 * lane), bb = *(const f32x4*)(b + 4 * lane);
  f32x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = (v[i] - mean) * rstd * ww[i] + bb[i];
  *(f32x4*)(x + (size_t)r * 256 + 4 * lane) = o;
  cn_store4(xt + (size_t)r * 256 + 4 * lane, o[0], o[1], o[2], o[3]);
}

template <typename T> __device__ __forceinline__ f32x4 cn_load4(const T* p);
template <> __device__ __forceinline__ f32x4 cn_load4<float>(const float* p) { return *(const f32x4*)p; }
template <> __device__ __forceinline__ f32x4 cn_load4<bf16_t>(const bf16_t* p) {
  const bf16x4 v = *(const bf16x4*)p;
  return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}

template <> __device__ __forceinline__ f32x4 cn_load4<half_t>(const half_t* p) {
  const cn_h4<half_t> v = *(const cn_h4<half_t>*)p;
  return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}
template <> __device__ __forceinline__ f32x4 cn_load4<sp16_t>(const sp16_t* p) {
  const u32x4 v = *(const u32x4*)p;
  return f32x4{cn_sp16_value(v[0]), cn_sp16_value(v[1]), cn_sp16_value(v[2]), cn_sp16_value(v[3])};
}

__device__ __forceinline__ float cn_dot8(f32x4 a, f32x4 b) {  // 32-dim head dot: 4 local + 8-lane reduce
  float d = a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
  d += __shfl_xor(d, 1);
  d += __shfl_xor(d, 2);
  d += __shfl_xor(d, 4);
  return d;
}

// Online-softmax update with a batch of NB scores / values (all loads were issued before the math,
// so a row pays one memory latency per batch instead of one per key).
template <int NB>
__device__ __forceinline__ void cn_attn_update(const float (&sc)[NB], const f32x4 (&vv)[NB], float& m, float& l,
                                               f32x4& acc) {
  float mb = sc[0];
#pragma unroll
  for (int u = 1; u < NB; ++u) mb = fmaxf(mb, sc[u]);
  const float mn = fmaxf(m, mb);
  const float corr = __expf(m - mn);
  l *= corr;
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] *= corr;
#pragma unroll
  for (int u = 0; u < NB; ++u) {
    const float p = __expf(sc[u] - mn);  // masked entries carry -inf -> p = 0
    l += p;
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = fmaf(p, vv[u][i], acc[i]);
  }
  m = mn;
}

// Causal self-attention of ONE new position per row over the cached prefix (8 heads x 32).
// lane l owns dims 4l..4l+3 (head l>>3).  Writes this step's K/V into the cache.
template <typename T>
__global__ __launch_bounds__(256) void cn_self_attn_kernel(const float* __restrict__ qkv, T* __restrict__ kc,
                                                           T* __restrict__ vc, const int* __restrict__ anc, int step,
                                                           int R, int beam, int maxp, float scale,
                                                           T* __restrict__ out,
                                                           const unsigned long long* __restrict__ kvalid) {
  constexpr int NB = 8;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= R) return;
  const unsigned long long valid = kvalid ? kvalid[r] : ~0ull;  // teacher forcing: padded caption positions are no keys
  const float* row = qkv + (size_t)r * 768 + 4 * lane;
  f32x4 q = *(const f32x4*)row;
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] *= scale;
  const f32x4 kn = *(const f32x4*)(row + 256), vn = *(const f32x4*)(row + 512);
  T* kdst = kc + ((size_t)step * R + r) * 256 + 4 * lane;
  T* vdst = vc + ((size_t)step * R + r) * 256 + 4 * lane;
  cn_store4(kdst, kn[0], kn[1], kn[2], kn[3]);
  cn_store4(vdst, vn[0], vn[1], vn[2], vn[3]);
  const int rb = (r / beam) * beam;
  float m = -INFINITY, l = 0.f;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int s0 = 0; s0 < step; s0 += NB) {
    f32x4 kk[NB], vv[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const int s = min(s0 + u, step - 1);
      const int src = rb + anc[(size_t)r * maxp + s];
      kk[u] = cn_load4<T>(kc + ((size_t)s * R + src) * 256 + 4 * lane);
      vv[u] = cn_load4<T>(vc + ((size_t)s * R + src) * 256 + 4 * lane);
    }
    float sc[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u)
      sc[u] = (s0 + u < step && ((valid >> (s0 + u)) & 1)) ? cn_dot8(q, kk[u]) : -INFINITY;
    cn_attn_update<NB>(sc, vv, m, l, acc);
  }
  if ((valid >> step) & 1) {  // own entry, at cache precision
    const f32x4 kk = f32x4{cn_to_f32(cn_from_f32<T>(kn[0])), cn_to_f32(cn_from_f32<T>(kn[1])),
                           cn_to_f32(cn_from_f32<T>(kn[2])), cn_to_f32(cn_from_f32<T>(kn[3]))};
    const f32x4 v1[1] = {f32x4{cn_to_f32(cn_from_f32<T>(vn[0])), cn_to_f32(cn_from_f32<T>(vn[1])),
                               cn_to_f32(cn_from_f32<T>(vn[2])), cn_to_f32(cn_from_f32<T>(vn[3]))}};
    const float s1[1] = {cn_dot8(q, kk)};
    cn_attn_update<1>(s1, v1, m, l, acc);
  }
  const float inv = 1.0f / l;
  cn_store4(out + (size_t)r * 256 + 4 * lane, acc[0] * inv, acc[1] * inv, acc[2] * inv, acc[3] * inv);
}

// Cross-attention of one query per row over its clip's projected audio memory (shared by beams);
// frames >= frame_lens[clip] are masked (key_padding_mask, conette.py:460-462).
template <typename T>
__global__ __launch_bounds__(256) void cn_cross_attn_kernel(const float* __restrict__ q, const T* __restrict__ kv,
                                                            int kv_ld, int kv_off, const int* __restrict__ lens,
                                                            int R, int beam, int Ta, float scale,
                                                            T* __restrict__ out) {
  constexpr int NB = 8;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= R) return;
  const int b = r / beam;
  f32x4 qq = *(const f32x4*)(q + (size_t)r * 256 + 4 * lane);
#pragma unroll
  for (int i = 0; i < 4; ++i) qq[i] *= scale;
  int n = lens[b];
  n = n < 1 ? 1 : (n > Ta ? Ta : n);
  const T* base = kv + (size_t)b * Ta * kv_ld + kv_off + 4 * lane;
  float m = -INFINITY, l = 0.f;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int t0 = 0; t0 < n; t0 += NB) {
    f32x4 kk[NB], vv[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const int t = min(t0 + u, n - 1);
      kk[u] = cn_load4<T>(base + (size_t)t * kv_ld);
      vv[u] = cn_load4<T>(base + (size_t)t * kv_ld + 256);
    }
    float sc[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) sc[u] = (t0 + u < n) ? cn_dot8(qq, kk[u]) : -INFINITY;
    cn_attn_update<NB>(sc, vv, m, l, acc);
  }
  const float inv = 1.0f / l;
  cn_store4(out + (size_t)r * 256 + 4 * lane, acc[0] * inv, acc[1] * inv, acc[2] * inv, acc[3] * inv);
}

// Self-attention of the one-pass teacher forcing (rows r = caption * cap_len + position): position t attends to the valid
// (non-pad) positions <= t of its caption, read from this pass's own QKV output at cache precision.
template <typename T>
__global__ __launch_bounds__(256) void cn_self_attn_causal_kernel(const float* __restrict__ qkv, const int32_t* __restrict__ caps,
                                                                  int cap_len, int R, int pad_id, float scale,
                                                                  T* __restrict__ out) {
  constexpr int NB = 8;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= R) return;
  const int b = r / cap_len, t = r % cap_len;
  f32x4 q = *(const f32x4*)(qkv + (size_t)r * 768 + 4 * lane);
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] *= scale;
  const float* base = qkv + (size_t)b * cap_len * 768 + 256 + 4 * lane;
  const int32_t* cap = caps + (size_t)b * cap_len;
  float m = -INFINITY, l = 0.f;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int s0 = 0; s0 <= t; s0 += NB) {
    f32x4 kk[NB], vv[NB];
    float sc[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const int sidx = min(s0 + u, t);
      const f32x4 k4 = *(const f32x4*)(base + (size_t)sidx * 768), v4 = *(const f32x4*)(base + (size_t)sidx * 768 + 256);
#pragma unroll
      for (int i = 0; i < 4; ++i) {  // cache precision
        kk[u][i] = cn_to_f32(cn_from_f32<T>(k4[i]));
        vv[u][i] = cn_to_f32(cn_from_f32<T>(v4[i]));
      }
    }
#pragma unroll
    for (int u = 0; u < NB; ++u) sc[u] = (s0 + u <= t && cap[min(s0 + u, t)] != pad_id) ? cn_dot8(q, kk[u]) : -INFINITY;
    cn_attn_update<NB>(sc, vv, m, l, acc);
  }
  const float inv = 1.0f / l;
  cn_store4(out + (size_t)r * 256 + 4 * lane, acc[0] * inv, acc[1] * inv, acc[2] * inv, acc[3] * inv);
}

// ---- teacher forcing (nn/decoding/forcing.py:12-71): the step loop fed with the given caption instead of the search
__global__ void cn_force_init_kernel(const int32_t* __restrict__ caps, int B, int cap_len, int pad_id,
                                     unsigned long long* __restrict__ kvalid, int* __restrict__ anc) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= B) return;
  unsigned long long m = 0;
  for (int j = 0; j < cap_len; ++j) {
    if (caps[(size_t)r * cap_len + j] != pad_id) m |= 1ull << j;  // tensor_to_pad_mask(caps_in, pad_value=pad_id)
    anc[(size_t)r * cap_len + j] = 0;                             // beam 1: every ancestor is the row itself
  }
  kvalid[r] = m;
}
__global__ void cn_force_tok_kernel(const int32_t* __restrict__ caps, int B, int cap_len, int step, int* __restrict__ cur_tok) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < B) cur_tok[r] = caps[(size_t)r * cap_len + step];
}
__global__ void cn_force_store_kernel(const float* __restrict__ logits, int ldv, int V, int cap_len, int step,
                                      float* __restrict__ out) {
  const int r = blockIdx.y;
  for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < V; v += gridDim.x * blockDim.x)
    out[((size_t)r * cap_len + step) * V + v] = logits[(size_t)r * ldv + v];
}
