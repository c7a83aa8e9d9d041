// Spatial allow bits straight from the batch's boxes (include/sam_hip_pipeline.h: sam_mask_bits_from_boxes): the two launches
//   sam_spatial_relation_tensor (spatial_graph.hip: boxes -> int8 [B,n,n,12])  ->  sam_mask_bits_spatial (masks.hip: int8 tensor & base -> bits)
// as one, with no relation tensor in memory.  Replaces, on the dataset side of the reference, sam/spatial_utils.py:92-218 + :33-52 +
// sam/datasets/textvqa_dataset.py:378-409 and the int8 [B,150,150,12] tensor per context every batch ships; on the model side sa_m4c.py:470-552,568.
// Same shape as masks.hip's spatial_wave_kernel: ONE WAVE per (batch, query) row, one key per lane, every head's 64 key bits out of a ballot, AND-ed
// with the base bits.  What was a 12-byte load per (query, key) pair is the pair's classification (spatial_pair.h, the copy relation_kernel inlines):
// float64, divergent only where the reference's own branches are (covers / IoU / distance / sector).
#include "common.h"
#include "sam_hip_pipeline.h"
#include "spatial_pair.h"

namespace {

__device__ __forceinline__ int region_of(int x, int T, int n_oo) { return x < T ? 0 : (x < T + n_oo ? 1 : 2); }   // text | obj + ocr | dec, as masks.hip

template <bool F64>
__global__ __launch_bounds__(256) void boxes_wave_kernel(const uint32_t* base, const void* obj, int64_t ld_obj, int n_obj, const void* ocr, int64_t ld_ocr, int n_ocr,
                                                         int B, int N, int NW, int T, int H, int width, double limit, unsigned quadrant_bits, uint32_t* out) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B * N) return;
  const int n_oo = n_obj + n_ocr;
  const int b = row / N, q = row - b * N;
  const int rq = region_of(q, T, n_oo);
  const uint32_t* brow = base + (int64_t)row * NW;
  Box A = {0.0, 0.0, 0.0, 0.0};
  if (rq == 1) A = load_oo_box<F64>(obj, ld_obj, n_obj, ocr, ld_ocr, n_ocr, b, q - T);      // the query's box: once per wave (one address for all lanes)
  for (int c = 0; c * 64 < NW * 32; ++c) {                 // 64 keys per pass = two words of every head; ALL NW words of the row are written (padding words read 0)
    const int key = c * 64 + lane;
    unsigned bits = 0;                                      // bit h: key visible for head h
    if (key < N) {
      const int rk = region_of(key, T, n_oo);
      const bool zeroed = (quadrant_bits >> (3 * rq + rk + 1)) & 1u;
      if (!zeroed) {
        if (rq == 1 && rk == 1) {
          const Box Bx = load_oo_box<F64>(obj, ld_obj, n_obj, ocr, ld_ocr, n_ocr, b, key - T);
          bits = channel_word(pair_code(A, Bx, q - T, key - T, limit), width);
        } else {
          bits = 0xffffu;
        }
      }
    }
    const int w0 = 2 * c;
    const uint32_t b0 = w0 < NW ? brow[w0] : 0u, b1 = w0 + 1 < NW ? brow[w0 + 1] : 0u;
    unsigned long long mine = ~0ull;                         // lane h ends up with head h's 64 key bits (heads >= 12: no spatial restriction)
    for (int h = 0; h < 12; ++h) {
      const unsigned long long m = __ballot((bits >> h) & 1u);
      if (lane == h) mine = m;
    }
    for (int h = lane; h < H; h += 64) {                     // one store instruction for all heads
      uint32_t* o = out + (((int64_t)b * H + h) * N + q) * NW;
      if (w0 < NW) o[w0] = b0 & (uint32_t)mine;
      if (w0 + 1 < NW) o[w0 + 1] = b1 & (uint32_t)(mine >> 32);
    }
  }
}

}  // namespace

extern "C" int sam_mask_bits_from_boxes(const uint32_t* base, const void* obj_boxes, int64_t ld_obj, int n_obj, const void* ocr_boxes, int64_t ld_ocr, int n_ocr,
                                        int boxes_f64, int B, int N, int NW, int T, int H, int context, double distance_threshold, unsigned quadrant_bits,
                                        uint32_t* out, void* stream) {
  SAM_REQUIRE(base && obj_boxes && out, "sam_mask_bits_from_boxes: null pointer");
  SAM_REQUIRE(n_obj > 0 && n_ocr >= 0, "sam_mask_bits_from_boxes: need n_obj > 0 and n_ocr >= 0 (n_obj=%d n_ocr=%d)", n_obj, n_ocr);
  SAM_REQUIRE(ocr_boxes || n_ocr == 0, "sam_mask_bits_from_boxes: ocr_boxes is NULL with n_ocr = %d", n_ocr);
  SAM_REQUIRE(context == 1 || context == 3 || context == 5 || context == 7 || context == 9, "sam_mask_bits_from_boxes: context must be 1,3,5,7 or 9 (got %d)", context);
  SAM_REQUIRE(H >= 12, "sam_mask_bits_from_boxes: need H >= 12, one head per spatial relation (H=%d)", H);
  SAM_REQUIRE(B > 0 && N > 0 && NW > 0 && (int64_t)NW * 32 >= N, "sam_mask_bits_from_boxes: bad shape B=%d N=%d NW=%d (need NW * 32 >= N)", B, N, NW);
  SAM_REQUIRE(T >= 0 && (int64_t)T + n_obj + n_ocr <= N, "sam_mask_bits_from_boxes: T + n_obj + n_ocr exceeds N (N=%d T=%d n_obj=%d n_ocr=%d)", N, T, n_obj, n_ocr);
  SAM_REQUIRE((int64_t)B * N <= 0x7fffffff, "sam_mask_bits_from_boxes: B * N out of range");
  SAM_REQUIRE(ld_obj >= 4 && (n_ocr == 0 || ld_ocr >= 4), "sam_mask_bits_from_boxes: box rows need a stride of at least 4 elements (ld_obj=%lld ld_ocr=%lld)",
              (long long)ld_obj, (long long)ld_ocr);
  const uintptr_t al = boxes_f64 ? 8 : 4;
  SAM_REQUIRE(((uintptr_t)obj_boxes % al) == 0 && ((uintptr_t)ocr_boxes % al) == 0, "sam_mask_bits_from_boxes: box pointers must be aligned to their element size");
  // legal quadrant ids are 1,2,4,7,8,9 (sa_m4c.py:505-549 raises ValueError on 3,5,6)
  SAM_REQUIRE((quadrant_bits & ~((1u << 1) | (1u << 2) | (1u << 4) | (1u << 7) | (1u << 8) | (1u << 9))) == 0, "sam_mask_bits_from_boxes: illegal quadrant id in 0x%x", quadrant_bits);
  const dim3 grid((unsigned)(((int64_t)B * N + 3) / 4)), block(256);
  const int width = (context - 1) / 2;
  const double limit = distance_threshold * sqrt(2.0);
  if (boxes_f64)
    boxes_wave_kernel<true><<<grid, block, 0, (hipStream_t)stream>>>(base, obj_boxes, ld_obj, n_obj, ocr_boxes, ld_ocr, n_ocr, B, N, NW, T, H, width, limit, quadrant_bits, out);
  else
    boxes_wave_kernel<false><<<grid, block, 0, (hipStream_t)stream>>>(base, obj_boxes, ld_obj, n_obj, ocr_boxes, ld_ocr, n_ocr, B, N, NW, T, H, width, limit, quadrant_bits, out);
  SAM_LAUNCH_CHECK();
  return SAM_OK;
}
