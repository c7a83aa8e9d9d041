// Spatial relation graph on the GPU: one thread per ordered box pair, float64 in the reference's operation
// order, emitting the multi-hot int8 [B,N,N,12] relation tensor the model consumes (batch_dict["spatial_adj_matrices"][c]).
// Replaces the O(N^2) Python loop of /root/reference/sam/spatial_utils.py:92-218 (0.49 s/sample) + the one-hot broadcast
// (:33-52) + the context composition of sam/datasets/textvqa_dataset.py:378-409.
// Relation codes: 1 a covers b, 2 a inside b, 3 IoU >= 0.5, 4..11 sector of the centre direction (if centre distance <
// threshold*sqrt(2)), 12 self; channel = code-1; context c adds the sector channels within +-(c-1)/2 (wrapping in 4..11).
#include "common.h"
#include "sam_hip.h"
#include "spatial_pair.h"   // Box, pair_code, channel_word: the pair classification, shared with mask_boxes.hip

namespace {

__device__ __forceinline__ Box load_box(const double* p) { return {p[0], p[1], p[2], p[3]}; }

__global__ __launch_bounds__(256) void relation_kernel(const double* boxes, int B, int N, int width, double limit, int8_t* out) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)B * N * N) return;
  const int bcol = idx % N, arow = (idx / N) % N, b = idx / ((int64_t)N * N);
  const Box A = load_box(boxes + ((int64_t)b * N + arow) * 4), Bx = load_box(boxes + ((int64_t)b * N + bcol) * 4);
  const unsigned chan = channel_word(pair_code(A, Bx, arow, bcol, limit), width);
  // 12 channels = 3 aligned dwords
  unsigned w[3] = {0, 0, 0};
#pragma unroll
  for (int h = 0; h < 12; ++h) w[h >> 2] |= ((chan >> h) & 1u) << (8 * (h & 3));
  unsigned* dst = reinterpret_cast<unsigned*>(out + idx * 12);
  dst[0] = w[0]; dst[1] = w[1]; dst[2] = w[2];
}

}  // namespace

extern "C" int sam_spatial_relation_tensor(const double* boxes, int B, int N, int context, double distance_threshold, int8_t* out, void* stream) {
  SAM_REQUIRE(boxes && out, "sam_spatial_relation_tensor: null pointer");
  SAM_REQUIRE(B > 0 && N > 0, "sam_spatial_relation_tensor: empty problem");
  SAM_REQUIRE(context == 1 || context == 3 || context == 5 || context == 7 || context == 9, "sam_spatial_relation_tensor: context must be 1,3,5,7 or 9 (got %d)", context);
  SAM_REQUIRE(((uintptr_t)out % 4) == 0, "sam_spatial_relation_tensor: output must be 4-byte aligned");
  const int64_t total = (int64_t)B * N * N;
  relation_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(boxes, B, N, (context - 1) / 2, distance_threshold * sqrt(2.0), out);
  SAM_LAUNCH_CHECK();
  return SAM_OK;
}
