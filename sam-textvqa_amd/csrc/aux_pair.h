// Device code shared by the spatial auxiliary heads' kernels: aux_heads.hip (pair scores, their backward from a dense G) and aux_loss.hip (the BCE loss
// on the pair scores and its backward, with G formed in registers).  ONE copy of the per-pair score, of the backward block and of the fixed-order
// partial-sum kernels; both translation units are compiled from it.
#pragma once
#include "common.h"

namespace auxp {

constexpr int AUX_C = 32;   // SimpleClassifier(hidden, 128, 32) output width
constexpr int AUX_R = 12;   // spatial relation logits, nn.Linear(32, 12)
constexpr int AUX_WB = AUX_R * AUX_C + AUX_R;   // per-block dW + dbias partial

// forward tiling: 4 waves; 64 consecutive j (one per lane) x 16 rows i (4 per wave)
constexpr int FWD_JT = 64, FWD_RW = 4, FWD_WAVES = 4;
// backward tiling: block (b, i tile of 64 rows, j tile of 32 columns), rows staged 16 at a time
constexpr int BWD_JT = 32, BWD_IC = 16, BWD_IT = 64;
constexpr int BWD_F4 = BWD_IC * BWD_JT * AUX_R / 4;   // float4 per staged chunk (1536)

inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// D[j] of a lane into registers (zeros past n)
__device__ __forceinline__ void load_d_row(const float* __restrict__ D, int64_t row, bool in_range, float (&d)[AUX_C]) {
  if (in_range) {
    const float4* dp = reinterpret_cast<const float4*>(D + row * AUX_C);
#pragma unroll
    for (int k = 0; k < AUX_C / 4; ++k) {
      const float4 v = dp[k];
      d[4 * k] = v.x; d[4 * k + 1] = v.y; d[4 * k + 2] = v.z; d[4 * k + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int c = 0; c < AUX_C; ++c) d[c] = 0.f;
  }
}

// the 12 scores of one pair: acc[r] = sum_c f(o[c], d[c]) W[r, c] + bias[r], c ascending
template <bool MUL>
__device__ __forceinline__ void pair_scores(const float* o, const float (&d)[AUX_C], const float* __restrict__ W, const float* __restrict__ bias,
                                            float (&acc)[AUX_R]) {
  float p[AUX_C];
#pragma unroll
  for (int c = 0; c < AUX_C; ++c) p[c] = MUL ? o[c] * d[c] : o[c] + d[c];
#pragma unroll
  for (int r = 0; r < AUX_R; ++r) {
    float a = 0.f;
#pragma unroll
    for (int c = 0; c < AUX_C; ++c) a = fmaf(p[c], W[r * AUX_C + c], a);
    acc[r] = a + bias[r];
  }
}

// what the loss's backward reads in place of a dense G: G = (sigmoid(S) - Y) * M * gscale, rebuilt per pair
struct LossArgs {
  const float* bias;        // [12]
  const uint8_t* codes;     // [B, n, n]: 0 none, 1..12 relation (label channel code - 1)
  const uint8_t* valid;     // [B, n]
  const float* grad_out;    // device scalar or NULL (= 1)
  const float* count;       // device scalar: number of valid pairs, written by the forward
};

// The backward block.  Thread (c = t & 31, q = t >> 5) owns column c and the four j of the tile q, q + 8, q + 16, q + 24.  The G tile of 16 rows sits in
// LDS: read ONCE from memory (LOSS = false, coalesced float4 loads of the rows' contiguous (j, r) stretches) or rebuilt from O, D, W, bias, the pair's
// code and the two valid flags (LOSS = true: thread t forms the 12 values of the pairs (il = (t >> 5) + 8 k, jl = t & 31), k = 0, 1; rows and columns
// that are not valid contribute exact zeros and their O / D values are never used).  Per (i, j): H = G . W[:, c] (12 FMA), then the dO / dD / dW
// contributions.  dD over the block's i tile is complete in one thread; dO over the thread's four j is summed over the 8 q in LDS per row; dW / dbias
// are summed over the block at the end.
template <bool MUL, bool LOSS>
__device__ __forceinline__ void pair_bwd_block(const float* __restrict__ G, const LossArgs la, const float* __restrict__ O, const float* __restrict__ D,
                                               const float* __restrict__ W, int n, int n_it, int n_jt, float* __restrict__ dO_part,
                                               float* __restrict__ dD_part, float* __restrict__ w_part) {
  __shared__ float4 gs[BWD_F4];
  __shared__ float os[BWD_IC][AUX_C];
  __shared__ float red[BWD_IC][8][AUX_C];
  const int t = threadIdx.x, c = t & 31, q = t >> 5;
  const int jt = blockIdx.x, it = blockIdx.y, b = blockIdx.z;
  const int j0 = jt * BWD_JT, i0 = it * BWD_IT;
  const int nj = min(BWD_JT, n - j0), ni = min(BWD_IT, n - i0);
  const int64_t sb = (int64_t)b * n;
  float wc[AUX_R];
#pragma unroll
  for (int r = 0; r < AUX_R; ++r) wc[r] = W[r * AUX_C + c];
  float dj[4], dd[4] = {0.f, 0.f, 0.f, 0.f}, dw[AUX_R];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int jl = q + 8 * u;
    bool use = jl < nj;
    if (LOSS) use = use && la.valid[sb + j0 + jl] != 0;
    dj[u] = use ? D[(sb + j0 + jl) * AUX_C + c] : 0.f;
  }
#pragma unroll
  for (int r = 0; r < AUX_R; ++r) dw[r] = 0.f;
  // dbias: the float4 a thread stages at chunk position g = t + 256 k holds r = 4 (g % 3) .. +3 of one j (a row is 96 float4, a multiple of 3)
  float4 bs0 = make_float4(0.f, 0.f, 0.f, 0.f), bs1 = bs0, bs2 = bs0;
  const int grp0 = t % 3;
  float gscale = 0.f;
  bool vj = false;
  if (LOSS) {
    gscale = (la.grad_out ? la.grad_out[0] : 1.f) / fmaxf(la.count[0], 1.f);
    vj = c < nj && la.valid[sb + j0 + c] != 0;          // (here c = t & 31 is the pair's column jl)
  }
  for (int ic0 = 0; ic0 < ni; ic0 += BWD_IC) {
    const int nic = min(BWD_IC, ni - ic0);
    __syncthreads();                       // the previous chunk's readers are done with gs / os / red
    for (int k = t; k < BWD_IC * AUX_C; k += 256) {
      const int il = k >> 5;
      bool use = il < nic;
      if (LOSS) use = use && la.valid[sb + i0 + ic0 + il] != 0;
      os[il][k & 31] = use ? O[(sb + i0 + ic0 + il) * AUX_C + (k & 31)] : 0.f;
    }
    if (LOSS) {
      __syncthreads();                     // os is read below
      float d[AUX_C];
      load_d_row(D, sb + j0 + c, vj, d);
#pragma unroll 1
      for (int k = 0; k < 2; ++k) {
        const int il = q + 8 * k;
        float g[AUX_R];
#pragma unroll
        for (int r = 0; r < AUX_R; ++r) g[r] = 0.f;
        if (vj && il < nic && la.valid[sb + i0 + ic0 + il] != 0) {
          float s[AUX_R];
          pair_scores<MUL>(os[il], d, W, la.bias, s);
          const int code = la.codes[(sb + i0 + ic0 + il) * n + j0 + c];
#pragma unroll
          for (int r = 0; r < AUX_R; ++r) {
            const float e = expf(-fabsf(s[r]));
            const float sig = (s[r] >= 0.f ? 1.f : e) / (1.f + e);
            g[r] = (sig - (code == r + 1 ? 1.f : 0.f)) * gscale;
          }
        }
        float4* gp = &gs[il * 96 + c * 3];
        gp[0] = make_float4(g[0], g[1], g[2], g[3]);
        gp[1] = make_float4(g[4], g[5], g[6], g[7]);
        gp[2] = make_float4(g[8], g[9], g[10], g[11]);
        bs0.x += g[0]; bs0.y += g[1]; bs0.z += g[2]; bs0.w += g[3];
        bs1.x += g[4]; bs1.y += g[5]; bs1.z += g[6]; bs1.w += g[7];
        bs2.x += g[8]; bs2.y += g[9]; bs2.z += g[10]; bs2.w += g[11];
      }
    } else {
#pragma unroll
      for (int k = 0; k < BWD_F4 / 256; ++k) {
        const int g = t + 256 * k;
        const int il = g / 96, m = g - il * 96;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (il < nic && m < nj * 3) v = reinterpret_cast<const float4*>(G + ((sb + i0 + ic0 + il) * n + j0) * AUX_R)[m];
        gs[g] = v;
        const int grp = (grp0 + k) % 3;
        if (grp == 0) { bs0.x += v.x; bs0.y += v.y; bs0.z += v.z; bs0.w += v.w; }
        else if (grp == 1) { bs1.x += v.x; bs1.y += v.y; bs1.z += v.z; bs1.w += v.w; }
        else { bs2.x += v.x; bs2.y += v.y; bs2.z += v.z; bs2.w += v.w; }
      }
    }
    __syncthreads();
    for (int il = 0; il < nic; ++il) {
      const float oi = os[il][c];
      float po = 0.f;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float4* gp = &gs[il * 96 + (q + 8 * u) * 3];
        const float4 g0 = gp[0], g1 = gp[1], g2 = gp[2];
        const float g[AUX_R] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w, g2.x, g2.y, g2.z, g2.w};
        float h = 0.f;
#pragma unroll
        for (int r = 0; r < AUX_R; ++r) h = fmaf(g[r], wc[r], h);
        float f;
        if (MUL) {
          po = fmaf(h, dj[u], po);
          dd[u] = fmaf(h, oi, dd[u]);
          f = oi * dj[u];
        } else {
          po += h;
          dd[u] += h;
          f = oi + dj[u];
        }
#pragma unroll
        for (int r = 0; r < AUX_R; ++r) dw[r] = fmaf(g[r], f, dw[r]);
      }
      red[il][q][c] = po;
    }
    __syncthreads();
    for (int k = t; k < nic * AUX_C; k += 256) {
      const int il = k >> 5, cc = k & 31;
      float s = 0.f;
#pragma unroll
      for (int qq = 0; qq < 8; ++qq) s += red[il][qq][cc];
      dO_part[(((int64_t)b * n_jt + jt) * n + i0 + ic0 + il) * AUX_C + cc] = s;
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int jl = q + 8 * u;
    if (jl < nj) dD_part[(((int64_t)b * n_it + it) * n + j0 + jl) * AUX_C + c] = dd[u];
  }
  // block partial of dW (sum over the 8 q of a column) and dbias (wave sums, then the 4 waves), fixed order
  __syncthreads();
  float* wred = reinterpret_cast<float*>(gs);          // [8][12][32]
#pragma unroll
  for (int r = 0; r < AUX_R; ++r) wred[(q * AUX_R + r) * AUX_C + c] = dw[r];
  const float bv[AUX_R] = {bs0.x, bs0.y, bs0.z, bs0.w, bs1.x, bs1.y, bs1.z, bs1.w, bs2.x, bs2.y, bs2.z, bs2.w};
  float* bred = &red[0][0][0];                          // [4 waves][12]
  const int lane = t & 63, wave = t >> 6;
#pragma unroll
  for (int r = 0; r < AUX_R; ++r) {
    const float s = wave_sum(bv[r]);
    if (lane == 0) bred[wave * AUX_R + r] = s;
  }
  __syncthreads();
  float* wp = w_part + (((int64_t)b * n_it + it) * n_jt + jt) * AUX_WB;
  for (int k = t; k < AUX_R * AUX_C; k += 256) {
    const int r = k >> 5, cc = k & 31;
    float s = 0.f;
#pragma unroll
    for (int qq = 0; qq < 8; ++qq) s += wred[(qq * AUX_R + r) * AUX_C + cc];
    wp[k] = s;
  }
  if (t < AUX_R) wp[AUX_R * AUX_C + t] = ((bred[t] + bred[AUX_R + t]) + bred[2 * AUX_R + t]) + bred[3 * AUX_R + t];
}

// dO[b,i,:] = sum over the j tiles of dO_part (blockIdx.y = 0), dD[b,j,:] = sum over the i tiles of dD_part (blockIdx.y = 1), tiles in order
static __global__ __launch_bounds__(256) void aux_reduce_rows_kernel(const float* __restrict__ dO_part, const float* __restrict__ dD_part, int B, int n,
                                                                     int n_jt, int n_it, float* __restrict__ dO, float* __restrict__ dD) {
  const int64_t per = (int64_t)n * AUX_C, e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)B * per) return;
  const int64_t bb = e / per, rem = e - bb * per;
  const bool rows = blockIdx.y == 0;
  const int tiles = rows ? n_jt : n_it;
  const float* src = (rows ? dO_part : dD_part) + bb * tiles * per + rem;
  float s = 0.f;
  for (int k = 0; k < tiles; ++k) s += src[k * per];
  (rows ? dO : dD)[e] = s;
}

// dW / dbias: one block per output element, 256 threads stride over the block partials, then a fixed butterfly + the 4 waves in order
static __global__ __launch_bounds__(256) void aux_reduce_w_kernel(const float* __restrict__ w_part, int nblk, float* __restrict__ dW,
                                                                  float* __restrict__ dbias, int accumulate) {
  __shared__ float sw[4];
  const int o = blockIdx.x, t = threadIdx.x;
  float s = 0.f;
  for (int k = t; k < nblk; k += 256) s += w_part[(int64_t)k * AUX_WB + o];
  s = wave_sum(s);
  if ((t & 63) == 0) sw[t >> 6] = s;
  __syncthreads();
  if (t == 0) {
    const float v = ((sw[0] + sw[1]) + sw[2]) + sw[3];
    float* dst = o < AUX_R * AUX_C ? dW + o : dbias + (o - AUX_R * AUX_C);
    *dst = accumulate ? *dst + v : v;
  }
}

inline int64_t pair_bwd_ws_floats(int B, int n) {
  const int64_t n_it = cdiv(n, BWD_IT), n_jt = cdiv(n, BWD_JT);
  return (int64_t)B * (n_jt + n_it) * n * AUX_C + (int64_t)B * n_it * n_jt * AUX_WB;
}

// the two reductions behind a backward block launch; ws as laid out by pair_bwd_ws_floats: dO_part | dD_part | w_part
struct BwdWs { float *dO_part, *dD_part, *w_part; int n_it, n_jt; };
inline BwdWs pair_bwd_ws(float* ws, int B, int n) {
  BwdWs p;
  p.n_it = cdiv(n, BWD_IT);
  p.n_jt = cdiv(n, BWD_JT);
  p.dO_part = ws;
  p.dD_part = p.dO_part + (int64_t)B * p.n_jt * n * AUX_C;
  p.w_part = p.dD_part + (int64_t)B * p.n_it * n * AUX_C;
  return p;
}
inline void launch_bwd_reductions(const BwdWs& p, int B, int n, float* dO, float* dD, float* dW, float* dbias, int accumulate, hipStream_t st) {
  const int64_t rows = (int64_t)B * n * AUX_C;
  aux_reduce_rows_kernel<<<dim3((unsigned)((rows + 255) / 256), 2), dim3(256), 0, st>>>(p.dO_part, p.dD_part, B, n, p.n_jt, p.n_it, dO, dD);
  aux_reduce_w_kernel<<<dim3(AUX_WB), dim3(256), 0, st>>>(p.w_part, B * p.n_it * p.n_jt, dW, dbias, accumulate);
}

}  // namespace auxp
