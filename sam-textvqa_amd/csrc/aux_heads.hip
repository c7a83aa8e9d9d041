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
#include "aux_pair.h"
#include "sam_hip.h"

namespace {

using namespace auxp;

// ---------------------------------------------------------------------------------------------------------------- forward
// Block: 4 waves; 64 consecutive j (one per lane) x 16 rows i (4 per wave).  A lane keeps D[j] in registers; O[i], W and bias are wave-uniform
// (scalar loads).  The 12 results of a lane for row i are 48 contiguous bytes; they go through a per-wave LDS stage so that the stores are float4
// runs over the (j, r) stretch of the row: 3 KB contiguous per wave and row.
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
  load_d_row(D, sb + j, j < n, d);
  float4* st = stage[wave];
  const int i_base = blockIdx.y * (FWD_WAVES * FWD_RW) + wave * FWD_RW;
  for (int u = 0; u < FWD_RW; ++u) {
    const int i = i_base + u;
    if (i >= n) break;
    float acc[AUX_R];
    pair_scores<MUL>(O + (sb + i) * AUX_C, d, W, bias, acc);
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
// auxp::pair_bwd_block with the G tile read from memory (aux_pair.h)
template <bool MUL>
__global__ __launch_bounds__(256) void aux_pair_bwd_kernel(const float* __restrict__ G, const float* __restrict__ O, const float* __restrict__ D,
                                                           const float* __restrict__ W, int n, int n_it, int n_jt, float* __restrict__ dO_part,
                                                           float* __restrict__ dD_part, float* __restrict__ w_part) {
  pair_bwd_block<MUL, false>(G, LossArgs{}, O, D, W, n, n_it, n_jt, dO_part, dD_part, w_part);
}

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
  return pair_bwd_ws_floats(B, n) * (int64_t)sizeof(float);
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
  const BwdWs p = pair_bwd_ws(ws, B, n);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(p.n_jt, p.n_it, B);
  if (fusion == SAM_AUX_MUL)
    aux_pair_bwd_kernel<true><<<grid, dim3(256), 0, st>>>(G, O, D, W, n, p.n_it, p.n_jt, p.dO_part, p.dD_part, p.w_part);
  else
    aux_pair_bwd_kernel<false><<<grid, dim3(256), 0, st>>>(G, O, D, W, n, p.n_it, p.n_jt, p.dO_part, p.dD_part, p.w_part);
  launch_bwd_reductions(p, B, n, dO, dD, dW, dbias, accumulate, st);
  SAM_LAUNCH_CHECK();
  return SAM_OK;
}
