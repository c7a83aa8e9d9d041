// The loss that trains the spatial auxiliary heads (include/sam_hip_aux_loss.h): masked BCE-with-logits on the pair scores
// spatial_classifier(f(O_i, D_j)) against the one-hot of the pair's relation code, forward and backward, with no [B, n, n, 12] tensor in memory.
//
//   forward   sam_aux_pair_fwd's tile (64 j per wave with D[j] in registers, 16 rows i per block, O[i] / W / bias wave-uniform); in place of the store a
//             lane reads its code byte and the two valid flags and sums max(s,0) - s y + log1p(exp(-|s|)) over its 12 scores.  Block partials
//             (loss sum fp32, pair count u32) -> workspace; one block sums them in a fixed order -> loss = sum / max(count, 1), count.
//   backward  sam_aux_pair_bwd's block (aux_pair.h) with the G tile rebuilt in registers: G = (sigmoid(S) - Y) M grad_out / max(count, 1).
//   codes     boxes -> relation code per pair through csrc/spatial_pair.h, the copy relation_kernel and boxes_wave_kernel are compiled from.
//
// Determinism: no atomics, every grid sized from the shape alone.
#include "aux_pair.h"
#include "sam_hip.h"
#include "spatial_pair.h"

namespace {

using namespace auxp;

template <bool MUL>
__global__ __launch_bounds__(256) void aux_pair_loss_fwd_kernel(const float* __restrict__ O, const float* __restrict__ D, const float* __restrict__ W,
                                                                const float* __restrict__ bias, const uint8_t* __restrict__ codes,
                                                                const uint8_t* __restrict__ valid, int n, float* __restrict__ part_loss,
                                                                uint32_t* __restrict__ part_count) {
  __shared__ float sl[FWD_WAVES];
  __shared__ uint32_t sc[FWD_WAVES];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.z, j = blockIdx.x * FWD_JT + lane;
  const int64_t sb = (int64_t)b * n;
  const bool vj = j < n && valid[sb + j] != 0;
  float d[AUX_C];
  load_d_row(D, sb + j, vj, d);                           // (a row that is not valid is never read: it may hold anything)
  float lsum = 0.f;
  uint32_t cnt = 0;
  const int i_base = blockIdx.y * (FWD_WAVES * FWD_RW) + wave * FWD_RW;
  for (int u = 0; u < FWD_RW; ++u) {
    const int i = i_base + u;
    if (i >= n) break;
    if (valid[sb + i] == 0) continue;                     // wave-uniform
    float s[AUX_R];
    pair_scores<MUL>(O + (sb + i) * AUX_C, d, W, bias, s);
    if (vj) {
      const int code = codes[(sb + i) * n + j];
      float e = 0.f;
#pragma unroll
      for (int r = 0; r < AUX_R; ++r) e += fmaxf(s[r], 0.f) - (code == r + 1 ? s[r] : 0.f) + log1pf(expf(-fabsf(s[r])));
      lsum += e;
      cnt += 1;
    }
  }
  lsum = wave_sum(lsum);
  cnt = (uint32_t)wave_sum((float)cnt);                  // at most 64 * FWD_RW = 256: exact in fp32
  if (lane == 0) { sl[wave] = lsum; sc[wave] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int64_t blk = ((int64_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    part_loss[blk] = ((sl[0] + sl[1]) + sl[2]) + sl[3];
    part_count[blk] = ((sc[0] + sc[1]) + sc[2]) + sc[3];
  }
}

// one block: 256 threads stride over the block partials, then a fixed butterfly + the 4 waves in order
__global__ __launch_bounds__(256) void aux_loss_finish_kernel(const float* __restrict__ part_loss, const uint32_t* __restrict__ part_count, int64_t nblk,
                                                              float* __restrict__ loss, float* __restrict__ count) {
  __shared__ float sl[4];
  __shared__ unsigned long long sc[4];
  const int t = threadIdx.x;
  float s = 0.f;
  unsigned long long c = 0;
  for (int64_t k = t; k < nblk; k += 256) { s += part_loss[k]; c += part_count[k]; }
  s = wave_sum(s);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
  if ((t & 63) == 0) { sl[t >> 6] = s; sc[t >> 6] = c; }
  __syncthreads();
  if (t == 0) {
    const float total = ((sl[0] + sl[1]) + sl[2]) + sl[3];
    const float pairs = (float)(((sc[0] + sc[1]) + sc[2]) + sc[3]);
    loss[0] = total / fmaxf(pairs, 1.f);
    count[0] = pairs;
  }
}

template <bool MUL>
__global__ __launch_bounds__(256) void aux_pair_loss_bwd_kernel(const LossArgs la, const float* __restrict__ O, const float* __restrict__ D,
                                                                const float* __restrict__ W, int n, int n_it, int n_jt, float* __restrict__ dO_part,
                                                                float* __restrict__ dD_part, float* __restrict__ w_part) {
  pair_bwd_block<MUL, true>(nullptr, la, O, D, W, n, n_it, n_jt, dO_part, dD_part, w_part);
}

template <bool F64>
__global__ __launch_bounds__(256) void relation_codes_kernel(const void* obj, int64_t ld_obj, int n_obj, const void* ocr, int64_t ld_ocr, int n_ocr, int B,
                                                             double limit, uint8_t* __restrict__ codes) {
  const int N = n_obj + n_ocr;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)B * N * N) return;
  const int bcol = idx % N, arow = (idx / N) % N, b = idx / ((int64_t)N * N);
  const Box A = load_oo_box<F64>(obj, ld_obj, n_obj, ocr, ld_ocr, n_ocr, b, arow), Bx = load_oo_box<F64>(obj, ld_obj, n_obj, ocr, ld_ocr, n_ocr, b, bcol);
  codes[idx] = (uint8_t)pair_code(A, Bx, arow, bcol, limit);
}

inline int64_t fwd_blocks(int B, int n) { return (int64_t)B * cdiv(n, FWD_JT) * cdiv(n, FWD_WAVES * FWD_RW); }

}  // namespace

extern "C" int64_t sam_aux_pair_loss_fwd_ws_bytes(int B, int n) {
  if (B <= 0 || n <= 0) return 0;
  return fwd_blocks(B, n) * (int64_t)(sizeof(float) + sizeof(uint32_t));
}

extern "C" int sam_aux_pair_loss_fwd(const float* O, const float* D, const float* W, const float* bias, const uint8_t* codes, const uint8_t* valid, int B,
                                     int n, int fusion, float* loss, float* count, float* ws, int64_t ws_bytes, void* stream) {
  SAM_REQUIRE(O && D && W && bias && codes && valid && loss && count && ws, "sam_aux_pair_loss_fwd: null pointer");
  SAM_REQUIRE(B > 0 && n > 0, "sam_aux_pair_loss_fwd: empty shape (B=%d n=%d)", B, n);
  SAM_REQUIRE(fusion == SAM_AUX_MUL || fusion == SAM_AUX_ADD, "sam_aux_pair_loss_fwd: unknown fusion %d", fusion);
  SAM_REQUIRE((uintptr_t)O % 16 == 0 && (uintptr_t)D % 16 == 0 && (uintptr_t)ws % 16 == 0, "sam_aux_pair_loss_fwd: O / D / ws must be 16-byte aligned");
  SAM_REQUIRE(B <= 65535, "sam_aux_pair_loss_fwd: B=%d exceeds the grid", B);
  SAM_REQUIRE(ws_bytes >= sam_aux_pair_loss_fwd_ws_bytes(B, n), "sam_aux_pair_loss_fwd: workspace of %lld bytes, need %lld", (long long)ws_bytes,
              (long long)sam_aux_pair_loss_fwd_ws_bytes(B, n));
  const int64_t nblk = fwd_blocks(B, n);
  float* part_loss = ws;
  uint32_t* part_count = reinterpret_cast<uint32_t*>(ws + nblk);
  const dim3 grid(cdiv(n, FWD_JT), cdiv(n, FWD_WAVES * FWD_RW), B);
  hipStream_t st = (hipStream_t)stream;
  if (fusion == SAM_AUX_MUL)
    aux_pair_loss_fwd_kernel<true><<<grid, dim3(256), 0, st>>>(O, D, W, bias, codes, valid, n, part_loss, part_count);
  else
    aux_pair_loss_fwd_kernel<false><<<grid, dim3(256), 0, st>>>(O, D, W, bias, codes, valid, n, part_loss, part_count);
  aux_loss_finish_kernel<<<dim3(1), dim3(256), 0, st>>>(part_loss, part_count, nblk, loss, count);
  SAM_LAUNCH_CHECK();
  return SAM_OK;
}

extern "C" int64_t sam_aux_pair_loss_bwd_ws_bytes(int B, int n) {
  if (B <= 0 || n <= 0) return 0;
  return pair_bwd_ws_floats(B, n) * (int64_t)sizeof(float);
}

extern "C" int sam_aux_pair_loss_bwd(const float* grad_out, const float* count, const float* O, const float* D, const float* W, const float* bias,
                                     const uint8_t* codes, const uint8_t* valid, int B, int n, int fusion, float* dO, float* dD, float* dW, float* dbias,
                                     int accumulate, float* ws, int64_t ws_bytes, void* stream) {
  SAM_REQUIRE(count && O && D && W && bias && codes && valid && dO && dD && dW && dbias && ws, "sam_aux_pair_loss_bwd: null pointer");
  SAM_REQUIRE(B > 0 && n > 0, "sam_aux_pair_loss_bwd: empty shape (B=%d n=%d)", B, n);
  SAM_REQUIRE(fusion == SAM_AUX_MUL || fusion == SAM_AUX_ADD, "sam_aux_pair_loss_bwd: unknown fusion %d", fusion);
  SAM_REQUIRE((uintptr_t)O % 16 == 0 && (uintptr_t)D % 16 == 0 && (uintptr_t)ws % 16 == 0, "sam_aux_pair_loss_bwd: O / D / ws must be 16-byte aligned");
  SAM_REQUIRE(B <= 65535, "sam_aux_pair_loss_bwd: B=%d exceeds the grid", B);
  SAM_REQUIRE(ws_bytes >= sam_aux_pair_loss_bwd_ws_bytes(B, n), "sam_aux_pair_loss_bwd: workspace of %lld bytes, need %lld", (long long)ws_bytes,
              (long long)sam_aux_pair_loss_bwd_ws_bytes(B, n));
  const BwdWs p = pair_bwd_ws(ws, B, n);
  const LossArgs la = {bias, codes, valid, grad_out, count};
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(p.n_jt, p.n_it, B);
  if (fusion == SAM_AUX_MUL)
    aux_pair_loss_bwd_kernel<true><<<grid, dim3(256), 0, st>>>(la, O, D, W, n, p.n_it, p.n_jt, p.dO_part, p.dD_part, p.w_part);
  else
    aux_pair_loss_bwd_kernel<false><<<grid, dim3(256), 0, st>>>(la, O, D, W, n, p.n_it, p.n_jt, p.dO_part, p.dD_part, p.w_part);
  launch_bwd_reductions(p, B, n, dO, dD, dW, dbias, accumulate, st);
  SAM_LAUNCH_CHECK();
  return SAM_OK;
}

extern "C" int sam_relation_codes_from_boxes(const void* obj_boxes, int64_t ld_obj, int n_obj, const void* ocr_boxes, int64_t ld_ocr, int n_ocr,
                                             int boxes_f64, int B, double distance_threshold, uint8_t* codes, void* stream) {
  SAM_REQUIRE(obj_boxes && codes, "sam_relation_codes_from_boxes: null pointer");
  SAM_REQUIRE(n_obj > 0 && n_ocr >= 0, "sam_relation_codes_from_boxes: need n_obj > 0 and n_ocr >= 0 (n_obj=%d n_ocr=%d)", n_obj, n_ocr);
  SAM_REQUIRE(ocr_boxes || n_ocr == 0, "sam_relation_codes_from_boxes: ocr_boxes is NULL with n_ocr = %d", n_ocr);
  SAM_REQUIRE(B > 0, "sam_relation_codes_from_boxes: empty batch (B=%d)", B);
  SAM_REQUIRE(ld_obj >= 4 && (n_ocr == 0 || ld_ocr >= 4), "sam_relation_codes_from_boxes: box rows need a stride of at least 4 elements (ld_obj=%lld ld_ocr=%lld)",
              (long long)ld_obj, (long long)ld_ocr);
  const uintptr_t al = boxes_f64 ? 8 : 4;
  SAM_REQUIRE(((uintptr_t)obj_boxes % al) == 0 && ((uintptr_t)ocr_boxes % al) == 0, "sam_relation_codes_from_boxes: box pointers must be aligned to their element size");
  const int64_t N = (int64_t)n_obj + n_ocr, total = (int64_t)B * N * N;
  SAM_REQUIRE(N <= 0x7fffffff && (total + 255) / 256 <= 0x7fffffff, "sam_relation_codes_from_boxes: B * n * n out of range");
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  const double limit = distance_threshold * sqrt(2.0);
  if (boxes_f64)
    relation_codes_kernel<true><<<grid, block, 0, (hipStream_t)stream>>>(obj_boxes, ld_obj, n_obj, ocr_boxes, ld_ocr, n_ocr, B, limit, codes);
  else
    relation_codes_kernel<false><<<grid, block, 0, (hipStream_t)stream>>>(obj_boxes, ld_obj, n_obj, ocr_boxes, ld_ocr, n_ocr, B, limit, codes);
  SAM_LAUNCH_CHECK();
  return SAM_OK;
}
