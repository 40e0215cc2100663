// Word-to-audio alignment: the cross-attention of the one-pass teacher forcing with its weights kept (conette_align, decoder.hip).
//
// cn_cross_attn_align_kernel<T> is cn_cross_attn_kernel<T> (dec_rows.h) for a row -- same row / lane layout, same online soft-max, the same
// context vector bit for bit -- and additionally writes the row's attention weights, averaged over the 8 heads:
//   pass 1  the online soft-max over the clip's frames; each batch's 8 x 8 scores are parked in LDS, [head][frame] per wave
//           (the first lane of each head stores its 8 scores as two 16-byte writes; the head stride of AL_LD = AL_TILE + 8 floats
//           keeps them 16-byte aligned and spreads the heads over the banks)
//   pass 2  lane-parallel over frames: lane j takes frame t0 + j, reads its 8 scores (consecutive lanes, consecutive words), forms
//           p_h = exp(s_h - m_h) * (1 / l_h) with the row's final maxima and sums, adds the heads in ascending order and stores
//           a = sum / 8 -- 64 consecutive floats per wave and store
// The LDS holds AL_TILE frames per wave; the scores of later tiles are recomputed from K (which the row read in pass 1 a moment
// ago) tile by tile, so t_audio is unbounded and nothing of size rows x frames x heads exists anywhere.
// Every output element has one writer per layer: the plane of layer l is stored, and the accumulated map is written by the first
// selected layer, read-added by the later ones (the layer loop is serial on the stream) and scaled by 1 / n_selected by the last.
// Frames at or behind the clip's length, and all frames of a row whose input token is pad_id, are stored as 0.
#pragma once

#define AL_TILE 256            // frames whose scores a wave keeps in LDS
#define AL_LD (AL_TILE + 8)    // head stride in floats

struct CnAlignOut {  // conette_align's outputs of the layer loop
  float* attn;         // (R, Ta)
  float* attn_layers;  // (n_layers, R, Ta) or null
  uint32_t layer_mask; // bit l = layer l is part of `attn`; never 0 here
};

#define AL_FIRST 1  // this layer stores into attn (no read)
#define AL_ADD 2    // this layer adds to attn
#define AL_LAST 4   // this layer scales attn by inv_sel

__device__ __forceinline__ void cn_align_park(float* sw, const float (&sc)[8], int lane, int col) {
  if ((lane & 7) == 0) {  // (the 8 lanes of a head hold the same 8 scores)
    float* dst = sw + (lane >> 3) * AL_LD + col;
    *(f32x4*)dst = f32x4{sc[0], sc[1], sc[2], sc[3]};
    *(f32x4*)(dst + 4) = f32x4{sc[4], sc[5], sc[6], sc[7]};
  }
}

template <typename T>
__global__ __launch_bounds__(256) void cn_cross_attn_align_kernel(const float* __restrict__ q, const T* __restrict__ kv, int kv_ld,
                                                                  int kv_off, const int* __restrict__ lens,
                                                                  const int32_t* __restrict__ caps, int pad_id, int R, int beam,
                                                                  int Ta, float scale, T* __restrict__ out,
                                                                  float* __restrict__ plane, float* __restrict__ attn, int mode,
                                                                  float inv_sel) {
  constexpr int NB = 8;
  __shared__ __attribute__((aligned(16))) float s_sc[4][8 * AL_LD];
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= R) return;
  float* sw = s_sc[threadIdx.x >> 6];
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
    if (t0 < AL_TILE) cn_align_park(sw, sc, lane, t0);  // (AL_TILE is a multiple of NB: the batch lies inside the tile)
    cn_attn_update<NB>(sc, vv, m, l, acc);
  }
  const float inv = 1.0f / l;
  cn_store4(out + (size_t)r * 256 + 4 * lane, acc[0] * inv, acc[1] * inv, acc[2] * inv, acc[3] * inv);

  // ---- pass 2: the weights ----
  float mh[8], ih[8];
#pragma unroll
  for (int h = 0; h < 8; ++h) {
    mh[h] = __shfl(m, 8 * h);
    ih[h] = __shfl(inv, 8 * h);
  }
  const bool is_pad = caps[r] == pad_id;
  float* prow = plane ? plane + (size_t)r * Ta : nullptr;
  float* arow = attn + (size_t)r * Ta;
  for (int tile = 0; tile < Ta; tile += AL_TILE) {
    if (tile > 0 && tile < n && !is_pad) {  // a later tile: its scores again, from K alone
      __builtin_amdgcn_wave_barrier();
      const int tend = min(tile + AL_TILE, n);
      for (int t0 = tile; t0 < tend; t0 += NB) {
        float sc[NB];
#pragma unroll
        for (int u = 0; u < NB; ++u) {
          const f32x4 kk = cn_load4<T>(base + (size_t)min(t0 + u, n - 1) * kv_ld);
          sc[u] = (t0 + u < n) ? cn_dot8(qq, kk) : -INFINITY;
        }
        cn_align_park(sw, sc, lane, t0 - tile);
      }
    }
    __builtin_amdgcn_wave_barrier();  // (one wave writes and reads its own tile: LDS operations of a wave complete in order)
    const int tend = min(tile + AL_TILE, Ta);
    for (int t0 = tile; t0 < tend; t0 += 64) {
      const int t = t0 + lane;
      if (t >= tend) continue;
      float a = 0.f;
      if (t < n && !is_pad) {
#pragma unroll
        for (int h = 0; h < 8; ++h) a += __expf(sw[h * AL_LD + (t - tile)] - mh[h]) * ih[h];
        a *= 0.125f;
      }
      if (prow) prow[t] = a;
      if (mode & (AL_FIRST | AL_ADD)) {
        float v = a;
        if (mode & AL_ADD) v = arow[t] + a;
        if (mode & AL_LAST) v *= inv_sel;
        arow[t] = v;
      }
    }
  }
}
