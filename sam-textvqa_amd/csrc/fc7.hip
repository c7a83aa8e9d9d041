// Faster R-CNN fc7 fine-tuning of the object / OCR input encoders (sam/textvqa_encoders.py FinetuneFasterRcnnFpnFc7: relu(fc6 W^T + b), then
// F.normalize in SAM4C._forward_obj_encoding / _forward_ocr_encoding, sam/sa_m4c.py:217-220, 236-238).  The GEMM itself runs on the GEMM family
// with the SAM_EPI_BIAS_RELU epilogue; the two row passes around it live here (gfx950, one wave per row, the whole row in registers):
//   l2norm_pack_from_bf16  <- F.normalize(fc7, dim=-1) of the bf16 GEMM output, written at its column offset of the K-padded encoder operand
//                             (the bf16 twin of embed.hip's l2norm_pack: no fp32 round trip)
//   fc7_bwd_rows           <- the backward of F.normalize fused with the ReLU mask: dz = [y > 0] * (g - yh (yh . g)) / max(||y||, eps)
#include "common.h"
#include "rowwise.h"
#include "sam_hip.h"

namespace {

// NCH chunks of 4 columns per lane (D <= 256 * NCH): the row body of embed.hip's l2norm_pack_reg_kernel (l2norm_row, rowwise.h) on a bf16 source
template <int NCH>
__global__ __launch_bounds__(256) void l2norm_pack_from_bf16_kernel(const bf16_t* x, int64_t ldx, int M, int D, int normalize, float eps, bf16_t* out,
                                                                    int64_t ldo, int col0, int zero_upto) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const bf16_t* xr = x + (int64_t)row * ldx;
  bf16_t* orow = out + (int64_t)row * ldo;
  l2norm_row<NCH>(xr, orow + col0, D, normalize != 0, eps, lane);
  for (int c = col0 + D + lane; c < zero_upto; c += 64) orow[c] = 0;
}

// y = relu(z) (bf16, what the forward normalised), g = d out / d F.normalize(y) (bf16) -> dz = d out / d z (bf16).
//   ||y|| > eps : d/dy = (g - yh (yh . g)) / ||y|| = g / n - y (y . g) / n^3
//   ||y|| <= eps: the clamp is active, y / eps is linear in y: d/dy = g / eps   (what torch's autograd of F.normalize gives)
// then the ReLU mask recomputed from the saved output (y > 0; z is not kept)
template <int NCH>
__global__ __launch_bounds__(256) void fc7_bwd_rows_kernel(const bf16_t* g, int64_t ldg, const bf16_t* y, int64_t ldy, int M, int D, int normalize, float eps,
                                                           bf16_t* dz, int64_t ldz) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const bf16_t* gr = g + (int64_t)row * ldg;
  const bf16_t* yr = y + (int64_t)row * ldy;
  bf16_t* dr = dz + (int64_t)row * ldz;
  const int nchunk = D >> 2;
  float gv[NCH][4], yv[NCH][4];
#pragma unroll
  for (int j = 0; j < NCH; ++j) {
    const int c = min(lane + 64 * j, nchunk - 1);
    ld4(gr + 4 * c, gv[j]);
    ld4(yr + 4 * c, yv[j]);
  }
  float a = 1.f, b = 0.f;                                  // dz = a * g - b * y  (before the mask)
  if (normalize) {
    float q = 0.f, d = 0.f;
#pragma unroll
    for (int j = 0; j < NCH; ++j)
      if (lane + 64 * j < nchunk) {
        q += (yv[j][0] * yv[j][0] + yv[j][1] * yv[j][1]) + (yv[j][2] * yv[j][2] + yv[j][3] * yv[j][3]);
        d += (yv[j][0] * gv[j][0] + yv[j][1] * gv[j][1]) + (yv[j][2] * gv[j][2] + yv[j][3] * gv[j][3]);
      }
    q = wave_sum(q);
    d = wave_sum(d);
    const float n = sqrtf(q);
    if (n > eps) {
      a = 1.0f / n;
      b = d * a * a * a;
    } else {
      a = 1.0f / eps;
    }
  }
#pragma unroll
  for (int j = 0; j < NCH; ++j) {
    const int c = lane + 64 * j;
    if (c < nchunk) {
      float o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = yv[j][e] > 0.f ? a * gv[j][e] - b * yv[j][e] : 0.f;
      st4(dr + 4 * c, o);
    }
  }
}

bool rows_ok(const void* p, int64_t ld) { return ((uintptr_t)p % 8) == 0 && ld % 4 == 0; }

}  // namespace

extern "C" int sam_l2norm_pack_from_bf16(const void* x, int64_t ldx, int M, int D, int normalize, float eps, void* out, int64_t ldo, int col0,
                                         int zero_upto, void* stream) {
  SAM_REQUIRE(x && out, "sam_l2norm_pack_from_bf16: null pointer");
  SAM_REQUIRE(M > 0 && D > 0 && D % 4 == 0 && D <= 2048, "sam_l2norm_pack_from_bf16: need 0 < D <= 2048, D %% 4 == 0 (M=%d D=%d)", M, D);
  SAM_REQUIRE(col0 >= 0 && col0 % 4 == 0 && col0 + D <= ldo && zero_upto <= ldo && ldx >= D, "sam_l2norm_pack_from_bf16: need col0 %% 4 == 0, col0 + D <= ldo, "
              "zero_upto <= ldo, ldx >= D (D=%d col0=%d ldo=%ld ldx=%ld)", D, col0, (long)ldo, (long)ldx);
  SAM_REQUIRE(rows_ok(x, ldx) && rows_ok(out, ldo), "sam_l2norm_pack_from_bf16: x / out must be 8-byte aligned with row strides a multiple of 4");
  SAM_REQUIRE(eps > 0.f, "sam_l2norm_pack_from_bf16: eps must be positive");
  const int nch = (D / 4 + 63) / 64;
  const dim3 grid((M + 3) / 4), blk(256);
  hipStream_t st = (hipStream_t)stream;
  nch_dispatch<1, 2, 4, 8>(nch, [&](auto n) {      // D <= 2048
    l2norm_pack_from_bf16_kernel<decltype(n)::value><<<grid, blk, 0, st>>>((const bf16_t*)x, ldx, M, D, normalize, eps, (bf16_t*)out, ldo, col0, zero_upto);
  });
  SAM_LAUNCH_CHECK();
  return SAM_OK;
}

extern "C" int sam_fc7_bwd_rows(const void* g, int64_t ldg, const void* y, int64_t ldy, int M, int D, int normalize, float eps, void* dz, int64_t ldz,
                                void* stream) {
  SAM_REQUIRE(g && y && dz, "sam_fc7_bwd_rows: null pointer");
  SAM_REQUIRE(M > 0 && D > 0 && D % 4 == 0 && D <= 2048, "sam_fc7_bwd_rows: need 0 < D <= 2048, D %% 4 == 0 (M=%d D=%d)", M, D);
  SAM_REQUIRE(ldg >= D && ldy >= D && ldz >= D, "sam_fc7_bwd_rows: row strides must cover D=%d", D);
  SAM_REQUIRE(rows_ok(g, ldg) && rows_ok(y, ldy) && rows_ok(dz, ldz), "sam_fc7_bwd_rows: operands must be 8-byte aligned with row strides a multiple of 4");
  SAM_REQUIRE(eps > 0.f, "sam_fc7_bwd_rows: eps must be positive");
  const int nch = (D / 4 + 63) / 64;
  const dim3 grid((M + 3) / 4), blk(256);
  hipStream_t st = (hipStream_t)stream;
  nch_dispatch<1, 2, 4, 8>(nch, [&](auto n) {      // D <= 2048
    fc7_bwd_rows_kernel<decltype(n)::value><<<grid, blk, 0, st>>>((const bf16_t*)g, ldg, (const bf16_t*)y, ldy, M, D, normalize, eps, (bf16_t*)dz, ldz);
  });
  SAM_LAUNCH_CHECK();
  return SAM_OK;
}
