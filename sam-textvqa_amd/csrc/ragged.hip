// Ragged region features -> what the object / OCR encoders consume (gfx950): one launch per token group.
//   ragged_expand  <- _pad_features of the dataset (sam/datasets/textvqa_dataset.py:285-305: zero-fill every sample to max_obj_num / max_ocr_num and build
//                     the padding mask) fused with the F.normalize / torch.cat chain of SAM4C.forward_obj_encoding / forward_ocr_encoding
//                     (sam/sa_m4c.py:217-253) that embed.hip's l2norm_pack runs on padded fp32 rows.
// A batch carries only its valid rows (fp32 or fp16), sample after sample, and an int32 count per sample; the kernel derives every sample's row offset from
// the counts itself (B is small: each wave sums the counts in front of its sample), so nothing is read by the host and the launch can sit in a captured step.
// Row-parallel like embed.hip: one wave per destination row (and part), four rows per 256-thread block, the whole row's loads in flight, vector stores,
// no atomics, no cross-block communication.
#include "common.h"
#include "rowwise.h"
#include "sam_hip.h"

namespace {

constexpr int RAGGED_MAX_PARTS = SAM_RAGGED_MAX_PARTS;

struct Part {
  const void* src; int64_t ld_src;
  void* dst; int64_t ld_dst;
  int width, col0, zero_upto;
  int flags;               // bit 0: fp16 source, bit 1: fp32 destination, bit 2: normalize, bit 3: vector path (8- / 16-byte accesses)
};
struct Args {
  const int32_t* counts; int B, n_max, cap_rows, n_parts;
  float eps;
  int64_t* mask;
  Part parts[RAGGED_MAX_PARTS];
};
enum { F_SRC16 = 1, F_DST32 = 2, F_NORM = 4, F_VEC = 8 };

__device__ __forceinline__ int clamp_count(int c, int n_max) { return c < 0 ? 0 : (c > n_max ? n_max : c); }

__device__ __forceinline__ float ld1(const _Float16* p) { return (float)*p; }
__device__ __forceinline__ float ld1(const float* p) { return *p; }
__device__ __forceinline__ void st1(float* p, float v) { *p = v; }
__device__ __forceinline__ void st1(bf16_t* p, float v) { *p = f2bf(v); }

// any width / alignment (the 5-column boxes; rows wider than 2048): scalar accesses, the row read twice when it is normalised
template <typename SrcT, typename DstT>
__device__ __forceinline__ void row_scalar(const SrcT* srow, DstT* drow, int width, bool normalize, float eps, int lane) {
  float scale = 1.f;
  if (normalize) {
    float q = 0.f;
    for (int c = lane; c < width; c += 64) { const float x = ld1(srow + c); q += x * x; }
    scale = 1.0f / fmaxf(sqrtf(wave_sum(q)), eps);
  }
  for (int c = lane; c < width; c += 64) {
    const float x = ld1(srow + c);
    st1(drow + c, normalize ? x * scale : x);
  }
}

// SrcT: float or _Float16; DstT: bf16_t or float.  A valid row of up to 2048 aligned columns goes through l2norm_row (rowwise.h): the row body of
// embed.hip's l2norm_pack_reg_kernel, hence its bits
template <typename SrcT, typename DstT>
__device__ __forceinline__ void part_row(const Part& p, int64_t src_row, int64_t dst_row, bool valid, float eps, int lane) {
  const SrcT* srow = (const SrcT*)p.src + src_row * p.ld_src;
  DstT* drow = (DstT*)p.dst + dst_row * p.ld_dst;
  const bool vec = p.flags & F_VEC, normalize = p.flags & F_NORM;
  const int nch = ((p.width >> 2) + 63) >> 6;
  if (valid) {
    if (vec && nch <= 2) l2norm_row<2>(srow, drow + p.col0, p.width, normalize, eps, lane);
    else if (vec && nch <= 4) l2norm_row<4>(srow, drow + p.col0, p.width, normalize, eps, lane);
    else if (vec && nch <= 8) l2norm_row<8>(srow, drow + p.col0, p.width, normalize, eps, lane);
    else row_scalar(srow, drow + p.col0, p.width, normalize, eps, lane);
  } else if (vec) {       // padded row: zeros over the part's columns
    const float z[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = lane; c < (p.width >> 2); c += 64) st4(drow + p.col0 + 4 * c, z);
  } else {
    for (int c = lane; c < p.width; c += 64) st1(drow + p.col0 + c, 0.f);
  }
  for (int c = p.col0 + p.width + lane; c < p.zero_upto; c += 64) st1(drow + c, 0.f);
}

// grid (ceil(B * n_max / 4), max(n_parts, 1)): wave (row, part)
__global__ __launch_bounds__(256) void ragged_expand_kernel(Args a) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.B * a.n_max) return;
  const int b = row / a.n_max, i = row - b * a.n_max;
  // exclusive prefix sum of the clamped counts in front of sample b; a count outside [0, n_max] is clamped, never trusted
  int part_sum = 0;
  for (int s = lane; s < b; s += 64) part_sum += clamp_count(a.counts[s], a.n_max);
  const int off = wave_sum_i(part_sum);
  const int cnt = clamp_count(a.counts[b], a.n_max);
  const bool valid = i < cnt;
  const int pi = blockIdx.y;
  if (pi == 0 && a.mask && lane == 0) a.mask[row] = valid ? 1 : 0;
  if (pi >= a.n_parts) return;
  const Part& p = a.parts[pi];
  const int64_t src_row = min(off + i, a.cap_rows - 1);          // in bounds whatever the counts hold
  const bool s16 = p.flags & F_SRC16, d32 = p.flags & F_DST32;
  if (s16 && d32) part_row<_Float16, float>(p, src_row, row, valid, a.eps, lane);
  else if (s16) part_row<_Float16, bf16_t>(p, src_row, row, valid, a.eps, lane);
  else if (d32) part_row<float, float>(p, src_row, row, valid, a.eps, lane);
  else part_row<float, bf16_t>(p, src_row, row, valid, a.eps, lane);
}

}  // namespace

extern "C" int sam_ragged_expand(const int32_t* counts, int B, int n_max, int cap_rows, const sam_ragged_part* parts, int n_parts, float eps, int64_t* mask,
                                 void* stream) {
  SAM_REQUIRE(counts, "sam_ragged_expand: null counts");
  SAM_REQUIRE(n_parts >= 0 && n_parts <= RAGGED_MAX_PARTS, "sam_ragged_expand: %d parts (at most %d)", n_parts, RAGGED_MAX_PARTS);
  SAM_REQUIRE(n_parts == 0 || parts, "sam_ragged_expand: null parts");
  SAM_REQUIRE(n_parts > 0 || mask, "sam_ragged_expand: nothing to write (no parts, no mask)");
  SAM_REQUIRE(B > 0 && n_max > 0 && cap_rows > 0 && (int64_t)B * n_max < (int64_t)1 << 31, "sam_ragged_expand: bad shape B=%d n_max=%d cap_rows=%d", B, n_max, cap_rows);
  SAM_REQUIRE(eps > 0.f, "sam_ragged_expand: eps must be positive");
  SAM_REQUIRE(((uintptr_t)counts % 4) == 0 && ((uintptr_t)mask % 8) == 0, "sam_ragged_expand: misaligned counts / mask");
  Args a;
  a.counts = counts; a.B = B; a.n_max = n_max; a.cap_rows = cap_rows; a.n_parts = n_parts; a.eps = eps; a.mask = mask;
  for (int k = 0; k < RAGGED_MAX_PARTS; ++k) a.parts[k] = Part{nullptr, 0, nullptr, 0, 0, 0, 0, 0};
  for (int k = 0; k < n_parts; ++k) {
    const sam_ragged_part& s = parts[k];
    SAM_REQUIRE(s.src && s.dst, "sam_ragged_expand: part %d: null pointer", k);
    SAM_REQUIRE(s.width > 0 && s.ld_src >= s.width, "sam_ragged_expand: part %d: need 0 < width <= ld_src (width=%d ld_src=%ld)", k, s.width, (long)s.ld_src);
    SAM_REQUIRE(s.col0 >= 0 && (int64_t)s.col0 + s.width <= s.ld_dst && s.zero_upto <= s.ld_dst,
                "sam_ragged_expand: part %d: need col0 + width <= ld_dst and zero_upto <= ld_dst (col0=%d width=%d zero_upto=%d ld_dst=%ld)", k, s.col0, s.width,
                s.zero_upto, (long)s.ld_dst);
    const int esz_s = s.src_f16 ? 2 : 4, esz_d = s.dst_f32 ? 4 : 2;
    SAM_REQUIRE(((uintptr_t)s.src % esz_s) == 0 && ((uintptr_t)s.dst % esz_d) == 0, "sam_ragged_expand: part %d: misaligned pointer", k);
    // 4 elements per access: 16-byte fp32 / 8-byte fp16 loads, 16-byte fp32 / 8-byte bf16 stores
    const bool vec = s.width % 4 == 0 && s.ld_src % 4 == 0 && s.ld_dst % 4 == 0 && s.col0 % 4 == 0 && ((uintptr_t)s.src % (4 * esz_s)) == 0 &&
                     ((uintptr_t)s.dst % (4 * esz_d)) == 0;
    a.parts[k] = Part{s.src, s.ld_src, s.dst, s.ld_dst, s.width, s.col0, s.zero_upto,
                      (s.src_f16 ? F_SRC16 : 0) | (s.dst_f32 ? F_DST32 : 0) | (s.normalize ? F_NORM : 0) | (vec ? F_VEC : 0)};
  }
  const int64_t rows = (int64_t)B * n_max;
  ragged_expand_kernel<<<dim3((unsigned)((rows + 3) / 4), (unsigned)(n_parts > 0 ? n_parts : 1)), dim3(256), 0, (hipStream_t)stream>>>(a);
  SAM_LAUNCH_CHECK();
  return SAM_OK;
}
