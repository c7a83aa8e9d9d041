// What the spatial aux heads' loss reads, from what a batch ships, in one launch (include/sam_hip_aux_targets.h):
//   valid[b, i] = (obj_mask | ocr_mask)[b, i] != 0                        u8 [B, n]
//   codes[b, i, j] = valid[b, i] & valid[b, j] ? sum_r (r + 1) rel[b, i, j, r] : 0      u8 [B, n, n] from int8 [B, n, n, 12]
//
// Layout: the relation tensor is a flat list of P = B n n pairs of 12 bytes, whatever n is.  A thread owns FOUR consecutive pairs: 48 bytes = three
// 16-byte loads in, one dword of codes out; a block of 256 threads owns 1024 pairs (12 KiB in, 1 KiB out).  The block finds the sample of its first
// pair with one wave-uniform 64-bit division; a thread finds (b, i, j) of its first pair with 32-bit divisions (n <= 32767, so n n + 1024 < 2^31)
// and steps to the next three.  A thread none of whose four pairs is valid loads nothing: an invalid row i is a run of n such pairs (12 n bytes that
// never leave memory).  The mask elements come through the caches (B n elements, read O(n) times each).
//
// Three forms of the same bytes: `rel` 16-byte aligned -> three 16-byte loads per thread; 4-byte aligned -> dword loads (the compiler may merge
// them: multi-dword global loads need dword alignment only); otherwise, and for a `codes` that is not dword aligned -> byte loads and byte stores.  The
// last P % 4 pairs take the byte form in every kernel.  The first B n threads of the grid also write `valid`.
#include "common.h"
#include "sam_hip_aux_targets.h"

namespace {

constexpr int AT_THREADS = 256, AT_PAIRS = 4, AT_BLOCK_PAIRS = AT_THREADS * AT_PAIRS, AT_CH = 12;

struct Masks {
  const void *obj, *ocr;
  int64_t ld_obj, ld_ocr;
  int n_obj;
};

template <int ELEM>
__device__ __forceinline__ bool elem_set(const void* p, int64_t idx) {
  if (ELEM == 1) return static_cast<const uint8_t*>(p)[idx] != 0;
  if (ELEM == 4) return static_cast<const uint32_t*>(p)[idx] != 0;
  return static_cast<const uint64_t*>(p)[idx] != 0;
}

// element k of the concatenated mask rows of sample b; no branch: the object / OCR choice selects the address, so a thread's lookups are independent loads
template <int ELEM>
__device__ __forceinline__ bool row_valid(const Masks& m, int b, int k) {
  const bool is_obj = k < m.n_obj;
  const void* base = is_obj ? m.obj : m.ocr;
  const int64_t idx = is_obj ? (int64_t)b * m.ld_obj + k : (int64_t)b * m.ld_ocr + (k - m.n_obj);
  return elem_set<ELEM>(base, idx);
}

// 48 bytes -> 12 little-endian dwords
template <int ALIGN>
__device__ __forceinline__ void load_pairs(const int8_t* __restrict__ src, uint32_t (&w)[AT_CH]) {
  if (ALIGN == 16) {
    const uint4* q = reinterpret_cast<const uint4*>(src);
    const uint4 a = q[0], b = q[1], c = q[2];
    w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
    w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
    w[8] = c.x; w[9] = c.y; w[10] = c.z; w[11] = c.w;
  } else if (ALIGN == 4) {
    const uint32_t* q = reinterpret_cast<const uint32_t*>(src);
#pragma unroll
    for (int k = 0; k < AT_CH; ++k) w[k] = q[k];
  } else {
    const uint8_t* q = reinterpret_cast<const uint8_t*>(src);
#pragma unroll
    for (int k = 0; k < AT_CH; ++k)
      w[k] = (uint32_t)q[4 * k] | ((uint32_t)q[4 * k + 1] << 8) | ((uint32_t)q[4 * k + 2] << 16) | ((uint32_t)q[4 * k + 3] << 24);
  }
}

// sum_r (r + 1) * int8 channel r of the pair held in three dwords, as a byte (what narrowing the int16 sum to uint8 gives)
__device__ __forceinline__ uint32_t pair_code(uint32_t w0, uint32_t w1, uint32_t w2) {
  const uint32_t w[3] = {w0, w1, w2};
  int s = 0;
#pragma unroll
  for (int d = 0; d < 3; ++d)
#pragma unroll
    for (int k = 0; k < 4; ++k) s += (4 * d + k + 1) * (int)(int8_t)(w[d] >> (8 * k));
  return (uint32_t)s & 0xffu;
}

template <int ELEM, int ALIGN>
__global__ __launch_bounds__(AT_THREADS) void aux_targets_kernel(const int8_t* __restrict__ rel, const Masks m, int n, int64_t rows, int64_t pairs,
                                                                 uint8_t* __restrict__ codes, uint8_t* __restrict__ valid) {
  const int64_t g = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x;
  if (g < rows) {                                          // rows = B n <= 2^31 - 1
    const uint32_t r = (uint32_t)g;
    valid[g] = row_valid<ELEM>(m, (int)(r / (uint32_t)n), (int)(r % (uint32_t)n)) ? 1 : 0;
  }
  const int64_t p0 = (int64_t)blockIdx.x * AT_BLOCK_PAIRS;           // wave-uniform
  if (p0 >= pairs) return;                                 // (pairs = 0 without a relation tensor)
  const uint32_t nn = (uint32_t)n * (uint32_t)n;
  const int64_t b0 = p0 / nn;
  const int64_t p = p0 + (int64_t)threadIdx.x * AT_PAIRS;
  if (p >= pairs) return;
  const uint32_t r0 = (uint32_t)(p0 - b0 * nn) + threadIdx.x * AT_PAIRS;       // < n n + 1024
  int b = (int)b0 + (int)(r0 / nn);
  const uint32_t rr = r0 % nn;
  int i = (int)(rr / (uint32_t)n), j = (int)(rr % (uint32_t)n);
  const int cnt = pairs - p < AT_PAIRS ? (int)(pairs - p) : AT_PAIRS;
  // (b, i, j) of the four pairs, then eight independent mask loads (one latency, not a chain); a pair past the end looks at the first pair's rows, so no
  // mask element outside [B, n] is read
  int pb[AT_PAIRS], pi[AT_PAIRS], pj[AT_PAIRS];
#pragma unroll
  for (int q = 0; q < AT_PAIRS; ++q) {
    pb[q] = b; pi[q] = i; pj[q] = j;
    if (++j == n) {
      j = 0;
      if (++i == n) { i = 0; ++b; }
    }
    if (q >= cnt) { pb[q] = pb[0]; pi[q] = pi[0]; pj[q] = pj[0]; }
  }
  bool v[AT_PAIRS];
#pragma unroll
  for (int q = 0; q < AT_PAIRS; ++q) {
    const bool vi = row_valid<ELEM>(m, pb[q], pi[q]), vj = row_valid<ELEM>(m, pb[q], pj[q]);
    v[q] = q < cnt && vi && vj;
  }
  const int8_t* src = rel + p * AT_CH;
  if (cnt == AT_PAIRS) {
    uint32_t out = 0;
    if (v[0] | v[1] | v[2] | v[3]) {
      uint32_t w[AT_CH];
      load_pairs<ALIGN>(src, w);
#pragma unroll
      for (int q = 0; q < AT_PAIRS; ++q)                  // (arithmetic masking: all of the 48 bytes are used whichever pairs are valid, so the loads stay whole)
        out |= (pair_code(w[3 * q], w[3 * q + 1], w[3 * q + 2]) & (0u - (uint32_t)v[q])) << (8 * q);
    }
    if (ALIGN >= 4) {
      *reinterpret_cast<uint32_t*>(codes + p) = out;       // p % 4 == 0 and codes is dword aligned in these forms
    } else {
#pragma unroll
      for (int q = 0; q < AT_PAIRS; ++q) codes[p + q] = (uint8_t)(out >> (8 * q));
    }
  } else {
    for (int q = 0; q < cnt; ++q) {                        // the last P % 4 pairs: bytes
      int s = 0;
      if (v[q])
        for (int r = 0; r < AT_CH; ++r) s += (r + 1) * (int)src[q * AT_CH + r];
      codes[p + q] = (uint8_t)s;
    }
  }
}

template <int ELEM>
void launch(int align, dim3 grid, hipStream_t st, const int8_t* rel, const Masks& m, int n, int64_t rows, int64_t pairs, uint8_t* codes, uint8_t* valid) {
  if (align == 16)
    aux_targets_kernel<ELEM, 16><<<grid, dim3(AT_THREADS), 0, st>>>(rel, m, n, rows, pairs, codes, valid);
  else if (align == 4)
    aux_targets_kernel<ELEM, 4><<<grid, dim3(AT_THREADS), 0, st>>>(rel, m, n, rows, pairs, codes, valid);
  else
    aux_targets_kernel<ELEM, 1><<<grid, dim3(AT_THREADS), 0, st>>>(rel, m, n, rows, pairs, codes, valid);
}

}  // namespace

extern "C" int sam_aux_targets(const int8_t* rel, const void* obj_mask, int64_t ld_obj, int n_obj, const void* ocr_mask, int64_t ld_ocr, int n_ocr,
                               int mask_elem_bytes, int B, int n, uint8_t* codes, uint8_t* valid, void* stream) {
  SAM_REQUIRE(B >= 0 && n >= 0 && n_obj >= 0 && n_ocr >= 0, "sam_aux_targets: negative size (B=%d n=%d n_obj=%d n_ocr=%d)", B, n, n_obj, n_ocr);
  SAM_REQUIRE((int64_t)n_obj + n_ocr == n, "sam_aux_targets: n_obj + n_ocr = %d + %d is not n = %d", n_obj, n_ocr, n);
  SAM_REQUIRE(mask_elem_bytes == 1 || mask_elem_bytes == 4 || mask_elem_bytes == 8, "sam_aux_targets: mask elements of %d bytes (1, 4 or 8: bool or an integer type)",
              mask_elem_bytes);
  SAM_REQUIRE(valid && (obj_mask || n_obj == 0) && (ocr_mask || n_ocr == 0) && (codes || !rel), "sam_aux_targets: null pointer");
  SAM_REQUIRE(((uintptr_t)obj_mask % mask_elem_bytes) == 0 && ((uintptr_t)ocr_mask % mask_elem_bytes) == 0,
              "sam_aux_targets: mask pointers must be aligned to their element size");
  SAM_REQUIRE(ld_obj >= n_obj && ld_ocr >= n_ocr, "sam_aux_targets: mask row strides below the row length (ld_obj=%lld ld_ocr=%lld)", (long long)ld_obj,
              (long long)ld_ocr);
  if (B == 0 || n == 0) return SAM_OK;
  const int64_t rows = (int64_t)B * n, pairs = rel ? rows * n : 0;
  SAM_REQUIRE(n <= 32767 && rows <= 0x7fffffff, "sam_aux_targets: n=%d above 32767 or B * n out of range", n);
  const int64_t by_pairs = (pairs + AT_BLOCK_PAIRS - 1) / AT_BLOCK_PAIRS, by_rows = (rows + AT_THREADS - 1) / AT_THREADS;
  const int64_t blocks = by_pairs > by_rows ? by_pairs : by_rows;
  SAM_REQUIRE(blocks <= 0x7fffffff, "sam_aux_targets: B * n * n out of range");
  const int align = !rel || (uintptr_t)codes % 4 ? 1 : (uintptr_t)rel % 16 == 0 ? 16 : (uintptr_t)rel % 4 == 0 ? 4 : 1;
  const Masks m = {obj_mask, ocr_mask, ld_obj, ld_ocr, n_obj};
  const dim3 grid((unsigned)blocks);
  hipStream_t st = (hipStream_t)stream;
  if (mask_elem_bytes == 1)
    launch<1>(align, grid, st, rel, m, n, rows, pairs, codes, valid);
  else if (mask_elem_bytes == 4)
    launch<4>(align, grid, st, rel, m, n, rows, pairs, codes, valid);
  else
    launch<8>(align, grid, st, rel, m, n, rows, pairs, codes, valid);
  SAM_LAUNCH_CHECK();
  return SAM_OK;
}
