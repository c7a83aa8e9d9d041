// Shared code of the row-wise kernels (rowops.hip, embed.hip, encoder_in.hip, fc7.hip, ragged.hip): everything that is neither a GEMM nor attention.
// Included after common.h by those translation units only.  One copy each of
//   ld4 / st4          4 consecutive elements <-> four floats (bf16, fp32, fp16 sources; bf16, fp32 destinations)
//   RowDropout         the hidden-state dropout of a launch: host-side preparation, device-side keep mask of 4 columns
//   partial_rows_sum   the fixed-order column reduction of per-block partial rows (LayerNorm backward, colsum, input-encoder backward)
//   l2norm_row         F.normalize of one row held in registers, packed to the destination type
//   nch_dispatch       run-time chunks-per-lane count -> template argument
#pragma once
#include <type_traits>
#include "common.h"

// ------------------------------------------------------------------------------------------ 4-wide loads and stores
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void ld4(const bf16_t* p, float* v) {
  const uint2 x = *reinterpret_cast<const uint2*>(p);
  v[0] = bf_lo(x.x); v[1] = bf_hi(x.x); v[2] = bf_lo(x.y); v[3] = bf_hi(x.y);
}
__device__ __forceinline__ void ld4(const float* p, float* v) {
  const float4 x = *reinterpret_cast<const float4*>(p);
  v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
}
__device__ __forceinline__ void ld4(const _Float16* p, float* v) {      // fp16 -> fp32 is exact
  const h16x4 x = *reinterpret_cast<const h16x4*>(p);
  v[0] = (float)x[0]; v[1] = (float)x[1]; v[2] = (float)x[2]; v[3] = (float)x[3];
}
// the same through an untyped base pointer and an element index (kernels templated on the element type)
template <typename T>
__device__ __forceinline__ void ld4(const void* p, int64_t idx, float* v) { ld4(reinterpret_cast<const T*>(p) + idx, v); }
__device__ __forceinline__ void st4(bf16_t* p, const float* v) { *reinterpret_cast<uint2*>(p) = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])); }
__device__ __forceinline__ void st4(float* p, const float* v) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
__device__ __forceinline__ float bf_round(float x) { return bf2f(f2bf(x)); }

// ------------------------------------------------------------------------------------------ hidden-state dropout
struct RowDropout {
  unsigned thr16; float inv_keep;                 // element kept iff rnd16 >= thr16 (0 = dropout off), kept elements scaled by inv_keep
  unsigned seed_lo, seed_hi, off_lo, off_hi;
  const unsigned long long* rng_state;
  __device__ __forceinline__ void resolve() { rng_resolve(rng_state, seed_lo, seed_hi, off_lo, off_hi); }
};
// `who`: the caller's prefix of the error message
inline int row_dropout_fill(RowDropout& d, float p_drop, uint64_t seed, uint64_t offset, const char* who) {
  SAM_REQUIRE(p_drop >= 0.f && p_drop < 1.f, "%s: p_drop out of range", who);
  d.thr16 = dropout_thr16(p_drop);
  d.inv_keep = d.thr16 ? 1.0f / (1.0f - (float)d.thr16 / 65536.0f) : 1.0f;
  d.seed_lo = (unsigned)seed; d.seed_hi = (unsigned)(seed >> 32); d.off_lo = (unsigned)offset; d.off_hi = (unsigned)(offset >> 32);
  d.rng_state = sam_get_rng_state();
  return SAM_OK;
}
// four columns against the two random words that cover them (16 bits per column)
__device__ __forceinline__ void keep4_words(float* v, unsigned lo, unsigned hi, unsigned thr16, float inv_keep) {
  v[0] = (lo & 0xffffu) >= thr16 ? v[0] * inv_keep : 0.f;
  v[1] = (lo >> 16) >= thr16 ? v[1] * inv_keep : 0.f;
  v[2] = (hi & 0xffffu) >= thr16 ? v[2] * inv_keep : 0.f;
  v[3] = (hi >> 16) >= thr16 ? v[3] * inv_keep : 0.f;
}
// keep mask of the 4 columns of chunk c (= col / 4) of `row`: half of the (row, col / 8) draw the GEMM / LayerNorm epilogues use (d resolved)
__device__ __forceinline__ void keep4(float* v, unsigned row, int c, const RowDropout& d) {
  const u32x4 rn = hidden_dropout_bits(row, (unsigned)(c >> 1), d.off_lo, d.off_hi, d.seed_lo, d.seed_hi);
  keep4_words(v, (c & 1) ? rn.z : rn.x, (c & 1) ? rn.w : rn.y, d.thr16, d.inv_keep);
}

// ------------------------------------------------------------------------------------------ partial-row reduction
// sum_r base[r * stride] over nrows partial rows in a fixed order, for a block of 64 columns (threadIdx.x & 63; `base` is this thread's column) x FIN_RL
// row lanes (threadIdx.x >> 6).  Every thread keeps 8 independent, unconditional loads in flight (the kernels are pure latency: one dependent load per
// trip was 128 L2 round trips in a row, 27 us per call): ((t0 + t1) + (t2 + t3)) + ((t4 + t5) + (t6 + t7)) per trip, accumulated over the trips, then
// the row lanes 0..15 in order through `red`.  The total is returned to row lane 0 (0 elsewhere); nrows == 0 reads nothing.
constexpr int FIN_RL = 16;
__device__ __forceinline__ float partial_rows_sum(const float* base, int nrows, int64_t stride, float (*red)[64]) {
  const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
  float s = 0.f;
  for (int r = ry; r < nrows; r += FIN_RL * 8) {
    float t[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) t[u] = base[(int64_t)min(r + FIN_RL * u, nrows - 1) * stride];
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (r + FIN_RL * u >= nrows) t[u] = 0.f;
    s += ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]));
  }
  red[ry][cx] = s;
  __syncthreads();
  float tot = 0.f;
  if (ry == 0) {
#pragma unroll
    for (int u = 0; u < FIN_RL; ++u) tot += red[u][cx];
  }
  return tot;
}

// ------------------------------------------------------------------------------------------ L2-normalise and pack
// One wave per row of up to 256 * NCH columns (width % 4 == 0), the whole row in registers: all of its loads in flight at once (unconditional, at clamped
// chunk indices, as in the LayerNorm kernels), one pass over memory.  dst[0 .. width) = src / max(||src||, eps), or src itself, rounded once to DstT.
// The fp32, bf16 and fp16 entry points share this body, so equal values give equal bits whatever format carried them.
template <int NCH, typename SrcT, typename DstT>
__device__ __forceinline__ void l2norm_row(const SrcT* src, DstT* dst, int width, bool normalize, float eps, int lane) {
  const int nchunk = width >> 2;
  float v[NCH][4];
#pragma unroll
  for (int j = 0; j < NCH; ++j) ld4(src + 4 * min(lane + 64 * j, nchunk - 1), v[j]);
  float scale = 1.f;
  if (normalize) {
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < NCH; ++j)
      if (lane + 64 * j < nchunk) q += (v[j][0] * v[j][0] + v[j][1] * v[j][1]) + (v[j][2] * v[j][2] + v[j][3] * v[j][3]);
    scale = 1.0f / fmaxf(sqrtf(wave_sum(q)), eps);       // x / max(||x||, eps)
  }
#pragma unroll
  for (int j = 0; j < NCH; ++j) {
    const int c = lane + 64 * j;
    if (c < nchunk) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[j][e] *= scale;
      st4(dst + 4 * c, v[j]);
    }
  }
}

// ------------------------------------------------------------------------------------------ NCH dispatch
// f(std::integral_constant<int, N>) for the first N of NS... with nch <= N; false (and no call) when nch exceeds them all
template <int... NS, typename F>
inline bool nch_dispatch(int nch, F&& f) {
  return ((nch <= NS ? (f(std::integral_constant<int, NS>{}), true) : false) || ...);
}
