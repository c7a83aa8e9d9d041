// SA-M4C spatial auxiliary heads (sam/sa_m4c.py:173-177, 316-347): the pair scoring spatial_classifier(f(O_i, D_j)), f = * or +, for every
// (object/OCR, object/OCR) pair of a sample, without the reference's repeated [B, n, n, 32] pair features.
//
//   forward   out[b,i,j,r] = sum_c f(O[b,i,c], D[b,j,c]) W[r,c] + bias[r]            fp32 [B, n, n, 12]
//   backward  H[b,i,j,c] = sum_r G[b,i,j,r] W[r,c]
//             mul: dO[i] = sum_j H D[j]   dD[j] = sum_i H O[i]   dW[r,c] = sum G O D
//             add: dO[i] = sum_j H        dD[j] = sum_i H        dW[r,c] = sum G (O + D)
//             dbias[r] = sum G
//
// Inner products run on the VALU in fp32 (K = 32, 12 outputs per pair: too small a contraction to feed an MFMA tile without padding it 4x, and fp32
// keeps the head at the reference's precision).  Both kernels stream one fp32 [B, n, n, 12] tensor; at B = 64, n = 150 that is 69.1 MB, and the
// VALU work per pair (32 + 384 FMA forward, ~27 per (pair, c) backward) is of the same order as the store / load time -- DESIGN.md section 8.
//
// Determinism: no atomics.  The backward writes per-block partials (dO over the block's j tile, dD over its i tile, dW / dbias over both) and two
// reduction kernels sum them in a fixed order.  Every grid is sized from the shape alone (never from the CU count), so sam_set_cu_reserve does not
// change a bit of the result.
#include "common.h"
#include "sam_hip.h"

namespace {

constexpr int AUX_C = 32;   // SimpleClassifier(hidden, 128, 32) output width
constexpr int AUX_R = 12;   // spatial relation logits, nn.Linear(32, 12)
constexpr int AUX_WB = AUX_R * AUX_C + AUX_R;   // per-block dW + dbias partial

// ---------------------------------------------------------------------------------------------------------------- forward
// Block: 4 waves; 64 consecutive j (one per lane) x 16 rows i (4 per wave).  A lane keeps D[j] in registers; O[i], W and bias are wave-uniform
// (scalar loads).  The 12 results of a lane for row i are 48 contiguous bytes; they go through a per-wave LDS stage so that the stores are float4
// runs over the (j, r) stretch of the row: 3 KB contiguous per wave and row.
constexpr int FWD_JT = 64, FWD_RW = 4, FWD_WAVES = 4;

template <bool MUL>
__global__ __launch_bounds__(256) void aux_pair_fwd_kernel(const float* __restrict__ O, const float* __restrict__ D, const float* __restrict__ W,
                                                           const float* __restrict__ bias, int n, float* __restrict__ out) {
  __shared__ float4 stage[FWD_WAVES][FWD_JT * AUX_R / 4];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.z, j0 = blockIdx.x * FWD_JT;
  const int j = j0 + lane;
  const int nj = min(FWD_JT, n - j0);
  const int64_t sb = (int64_t)b * n;
  float d[AUX_C];
  if (j < n) {
    const float4* dp = reinterpret_cast<const float4*>(D + (sb + j) * AUX_C);
#pragma unroll
    for (int k = 0; k < AUX_C / 4; ++k) {
      const float4 v = dp[k];
      d[4 * k] = v.x; d[4 * k + 1] = v.y; d[4 * k + 2] = v.z; d[4 * k + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int c = 0; c < AUX_C; ++c) d[c] = 0.f;
  }
  float4* st = stage[wave];
  const int i_base = blockIdx.y * (FWD_WAVES * FWD_RW) + wave * FWD_RW;
  for (int u = 0; u < FWD_RW; ++u) {
    const int i = i_base + u;
    if (i >= n) break;
    const float* o = O + (sb + i) * AUX_C;
    float p[AUX_C];
#pragma unroll
    for (int c = 0; c < AUX_C; ++c) p[c] = MUL ? o[c] * d[c] : o[c] + d[c];
    float acc[AUX_R];
#pragma unroll
    for (int r = 0; r < AUX_R; ++r) {
      float a = 0.f;
#pragma unroll
      for (int c = 0; c < AUX_C; ++c) a = fmaf(p[c], W[r * AUX_C + c], a);
      acc[r] = a + bias[r];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) st[lane * 3 + k] = make_float4(acc[4 * k], acc[4 * k + 1], acc[4 * k + 2], acc[4 * k + 3]);
    __builtin_amdgcn_wave_barrier();
    float4* dst = reinterpret_cast<float4*>(out + ((sb + i) * n + j0) * AUX_R);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int q = lane + 64 * k;
      if (q < nj * 3) dst[q] = st[q];
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// ---------------------------------------------------------------------------------------------------------------- backward
// Block (b, i tile of 64 rows, j tile of 32 columns), 256 threads: thread (c = t & 31, q = t >> 5) owns column c and the four j of the tile
// q, q + 8, q + 16, q + 24.  G is read ONCE, 16 rows at a time, through LDS (coalesced float4 loads of the rows' contiguous (j, r) stretches).
// Per (i, j): H = G . W[:, c] (12 FMA), then the dO / dD / dW contributions.  dD over the block's i tile is complete in one thread; dO over the
// thread's four j is summed over the 8 q in LDS per row; dW / dbias are summed over the block at the end.
constexpr int BWD_JT = 32, BWD_IC = 16, BWD_IT = 64;
constexpr int BWD_F4 = BWD_IC * BWD_JT * AUX_R / 4;   // float4 per staged chunk (1536)

template <bool MUL>
__global__ __launch_bounds__(256) void aux_pair_bwd_kernel(const float* __restrict__ G, const float* __restrict__ O, const float* __restrict__ D,
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
    dj[u] = jl < nj ? D[(sb + j0 + jl) * AUX_C + c] : 0.f;
  }
#pragma unroll
  for (int r = 0; r < AUX_R; ++r) dw[r] = 0.f;
  // dbias: the float4 a thread stages at chunk position g = t + 256 k holds r = 4 (g % 3) .. +3 of one j (a row is 96 float4, a multiple of 3)
  float4 bs0 = make_float4(0.f, 0.f, 0.f, 0.f), bs1 = bs0, bs2 = bs0;
  const int grp0 = t % 3;
  for (int ic0 = 0; ic0 < ni; ic0 += BWD_IC) {
    const int nic = min(BWD_IC, ni - ic0);
    __syncthreads();                       // the previous chunk's readers are done with gs / os / red
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
    for (int k = t; k < BWD_IC * AUX_C; k += 256) {
      const int il = k >> 5;
      os[il][k & 31] = il < nic ? O[(sb + i0 + ic0 + il) * AUX_C + (k & 31)] : 0.f;
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
__global__ __launch_bounds__(256) void aux_reduce_rows_kernel(const float* __restrict__ dO_part, const float* __restrict__ dD_part, int B, int n, int n_jt,
                                                              int n_it, float* __restrict__ dO, float* __restrict__ dD) {
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
__global__ __launch_bounds__(256) void aux_reduce_w_kernel(const float* __restrict__ w_part, int nblk, float* __restrict__ dW, float* __restrict__ dbias,
                                                           int accumulate) {
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

inline int cdiv(int a, int b) { return (a + b - 1) / b; }

}  // namespace

extern "C" int sam_aux_pair_fwd(const float* O, const float* D, const float* W, const float* bias, int B, int n, int fusion, float* out, void* stream) {
  SAM_REQUIRE(O && D && W && bias && out, "sam_aux_pair_fwd: null pointer");
  SAM_REQUIRE(B > 0 && n > 0, "sam_aux_pair_fwd: empty shape (B=%d n=%d)", B, n);
  SAM_REQUIRE(fusion == SAM_AUX_MUL || fusion == SAM_AUX_ADD, "sam_aux_pair_fwd: unknown fusion %d", fusion);
  SAM_REQUIRE((uintptr_t)O % 16 == 0 && (uintptr_t)D % 16 == 0 && (uintptr_t)out % 16 == 0, "sam_aux_pair_fwd: O / D / out must be 16-byte aligned");
  SAM_REQUIRE(B <= 65535, "sam_aux_pair_fwd: B=%d exceeds the grid", B);
  const dim3 grid(cdiv(n, FWD_JT), cdiv(n, FWD_WAVES * FWD_RW), B);
  hipStream_t st = (hipStream_t)stream;
  if (fusion == SAM_AUX_MUL)
    aux_pair_fwd_kernel<true><<<grid, dim3(256), 0, st>>>(O, D, W, bias, n, out);
  else
    aux_pair_fwd_kernel<false><<<grid, dim3(256), 0, st>>>(O, D, W, bias, n, out);
  SAM_LAUNCH_CHECK();
  return SAM_OK;
}

extern "C" int64_t sam_aux_pair_bwd_ws_bytes(int B, int n) {
  if (B <= 0 || n <= 0) return 0;
  const int64_t n_it = cdiv(n, BWD_IT), n_jt = cdiv(n, BWD_JT);
  return ((int64_t)B * (n_jt + n_it) * n * AUX_C + (int64_t)B * n_it * n_jt * AUX_WB) * (int64_t)sizeof(float);
}

extern "C" int sam_aux_pair_bwd(const float* G, const float* O, const float* D, const float* W, int B, int n, int fusion, float* dO, float* dD, float* dW,
                                float* dbias, int accumulate, float* ws, int64_t ws_bytes, void* stream) {
  SAM_REQUIRE(G && O && D && W && dO && dD && dW && dbias && ws, "sam_aux_pair_bwd: null pointer");
  SAM_REQUIRE(B > 0 && n > 0, "sam_aux_pair_bwd: empty shape (B=%d n=%d)", B, n);
  SAM_REQUIRE(fusion == SAM_AUX_MUL || fusion == SAM_AUX_ADD, "sam_aux_pair_bwd: unknown fusion %d", fusion);
  SAM_REQUIRE((uintptr_t)G % 16 == 0 && (uintptr_t)ws % 16 == 0, "sam_aux_pair_bwd: G / ws must be 16-byte aligned");
  SAM_REQUIRE(B <= 65535, "sam_aux_pair_bwd: B=%d exceeds the grid", B);
  SAM_REQUIRE(ws_bytes >= sam_aux_pair_bwd_ws_bytes(B, n), "sam_aux_pair_bwd: workspace of %lld bytes, need %lld", (long long)ws_bytes,
              (long long)sam_aux_pair_bwd_ws_bytes(B, n));
  const int n_it = cdiv(n, BWD_IT), n_jt = cdiv(n, BWD_JT);
  float* dO_part = ws;
  float* dD_part = dO_part + (int64_t)B * n_jt * n * AUX_C;
  float* w_part = dD_part + (int64_t)B * n_it * n * AUX_C;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(n_jt, n_it, B);
  if (fusion == SAM_AUX_MUL)
    aux_pair_bwd_kernel<true><<<grid, dim3(256), 0, st>>>(G, O, D, W, n, n_it, n_jt, dO_part, dD_part, w_part);
  else
    aux_pair_bwd_kernel<false><<<grid, dim3(256), 0, st>>>(G, O, D, W, n, n_it, n_jt, dO_part, dD_part, w_part);
  const int64_t rows = (int64_t)B * n * AUX_C;
  aux_reduce_rows_kernel<<<dim3((unsigned)((rows + 255) / 256), 2), dim3(256), 0, st>>>(dO_part, dD_part, B, n, n_jt, n_it, dO, dD);
  aux_reduce_w_kernel<<<dim3(AUX_WB), dim3(256), 0, st>>>(w_part, B * n_it * n_jt, dW, dbias, accumulate);
  SAM_LAUNCH_CHECK();
  return SAM_OK;
}
