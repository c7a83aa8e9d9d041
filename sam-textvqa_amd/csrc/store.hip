// Region features resident in device memory -> the ragged batch of ragged.hip, gathered by index (gfx950).
//   store_gather_ragged  <- ImageFeaturesH5Reader(in_memory=True).__getitem__ + the features[1:] / _pad_features(min(num_boxes, max)) of
//                           TextVQADataset.__getitem__ (sam/datasets/_image_features_reader.py:121-188, textvqa_dataset.py:307-334), with the whole
//                           feature set in HBM in place of host memory: a batch is a list of indices and no feature byte crosses the host link.
//   store_gather_fixed   <- the per-question / per-image tensors of the same batch (packed text, ids, answer tables): row idx of [N, ...] -> row b.
// Same layout as ragged_expand_kernel: one wave per (destination slot (b, i), part), four waves per 256-thread block, every wave derives its sample's
// destination offset from the clamped counts in front (B is small), no atomics, no cross-block communication.  Rows are copied as bytes: 16-byte
// accesses when the addresses and strides allow, else 4-byte, else bytes; up to four accesses per lane (a 4 KB row at 16 bytes) are in flight before
// the first store.  Nothing read from device memory (indices, image_of, row_off) is trusted: see include/sam_hip_store.h.
#include "common.h"
#include "sam_hip_store.h"

namespace {

constexpr int STORE_MAX_PARTS = 8;
enum { ST_BAD_INDEX = 1, ST_BAD_RANGE = 2 };

struct Part {
  const char* src; int64_t ld_src;
  char* dst; int64_t ld_dst;
  int64_t row_bytes;
  int vec;                 // bytes per access: 16, 4 or 1
  int key;                 // fixed tables: 0 row = the question, 1 row = its image
};
struct Args {
  const int32_t *sample_idx, *image_of;
  const int64_t* row_off;
  int32_t *counts_out, *status;
  int64_t total_rows;
  int B, n_questions, n_images, n_max, cap_rows, n_parts;
  Part parts[STORE_MAX_PARTS];
};

struct Sample { int64_t img, lo; int cnt, flags; };

// sample_idx[b] -> its image (or -1 with ST_BAD_INDEX)
__device__ __forceinline__ int64_t resolve_image(const Args& a, int b, bool& q_ok) {
  const int q = a.sample_idx[b];
  q_ok = q >= 0 && q < a.n_questions;
  if (!q_ok) return -1;
  const int64_t g = a.image_of ? (int64_t)a.image_of[q] : (int64_t)q;
  return (g >= 0 && g < a.n_images) ? g : -1;
}

// the source range of sample b: [lo, lo + cnt) inside [0, total_rows] and cnt in [0, n_max], whatever row_off holds
__device__ __forceinline__ Sample resolve_rows(const Args& a, int b) {
  bool q_ok;
  Sample s{resolve_image(a, b, q_ok), 0, 0, 0};
  if (s.img < 0) { s.flags = ST_BAD_INDEX; return s; }
  const int64_t lo = a.row_off[s.img], hi = a.row_off[s.img + 1];
  const uint64_t d = hi > lo ? (uint64_t)hi - (uint64_t)lo : 0;            // (exact for hi > lo: no signed overflow on corrupted offsets)
  int cnt = d > (uint64_t)a.n_max ? a.n_max : (int)d;
  if (cnt == 0) return s;
  if (lo > a.total_rows) { cnt = 0; s.flags = ST_BAD_RANGE; }
  else if (lo < 0) {
    const int64_t end = lo + cnt;                                           // lo < 0 < cnt: cannot overflow
    cnt = end > 0 ? (int)(end < a.total_rows ? end : a.total_rows) : 0;
    s.flags = ST_BAD_RANGE;
  } else {
    s.lo = lo;
    if ((int64_t)cnt > a.total_rows - lo) { cnt = (int)(a.total_rows - lo); s.flags = ST_BAD_RANGE; }
  }
  s.cnt = cnt;
  return s;
}

typedef __attribute__((ext_vector_type(4))) unsigned b16;                  // 16 bytes, 16-byte aligned: one global_load / store_dwordx4
__device__ __forceinline__ void clear(b16& v) { v = b16{0u, 0u, 0u, 0u}; }
__device__ __forceinline__ void clear(unsigned& v) { v = 0u; }
__device__ __forceinline__ void clear(unsigned char& v) { v = 0; }

// n accesses of sizeof(V) bytes, lane-strided, four per lane loaded before the first is stored; zero: store zeros, read nothing
template <typename V>
__device__ __forceinline__ void copy_chunks(const char* s, char* d, int64_t n, bool zero, int lane) {
  const V* sv = (const V*)s;
  V* dv = (V*)d;
  for (int64_t c0 = 0; c0 < n; c0 += 256) {
    V r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t c = c0 + k * 64 + lane;
      clear(r[k]);
      if (!zero && c < n) r[k] = sv[c];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t c = c0 + k * 64 + lane;
      if (c < n) dv[c] = r[k];
    }
  }
}

// one row of a part: src_row / dst_row are row numbers (64-bit: a fp16 store passes 2^32 bytes at 1 M rows)
__device__ __forceinline__ void copy_row(const Part& p, int64_t src_row, int64_t dst_row, bool zero, int lane) {
  const char* s = p.src + src_row * p.ld_src;
  char* d = p.dst + dst_row * p.ld_dst;
  const int64_t body = p.row_bytes / p.vec;
  if (p.vec == 16) copy_chunks<b16>(s, d, body, zero, lane);
  else if (p.vec == 4) copy_chunks<unsigned>(s, d, body, zero, lane);
  else copy_chunks<unsigned char>(s, d, body, zero, lane);
  const int64_t done = body * p.vec;                                        // the bytes past the last whole access: fewer than 16
  if (done + lane < p.row_bytes) d[done + lane] = zero ? (char)0 : s[done + lane];
}

// grid (ceil(B * n_max / 4), n_parts): wave (slot, part)
__global__ __launch_bounds__(256) void store_gather_ragged_kernel(Args a) {
  const int lane = threadIdx.x & 63, slot = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (slot >= a.B * a.n_max) return;
  const int b = slot / a.n_max, i = slot - b * a.n_max, pi = blockIdx.y;
  const Sample own = resolve_rows(a, b);
  if (i == 0 && pi == 0 && lane == 0) {                                     // one lane per sample and launch: no atomics
    a.counts_out[b] = own.cnt;
    if (own.flags) a.status[b] |= own.flags;
  }
  if (i >= own.cnt) return;                                                 // (wave-uniform)
  int part_sum = 0;
  for (int s = lane; s < b; s += 64) part_sum += resolve_rows(a, s).cnt;
  const int off = wave_sum_i(part_sum);                                     // < B * n_max < 2^31
  if (off + i >= a.cap_rows) return;
  copy_row(a.parts[pi], own.lo + i, (int64_t)off + i, false, lane);
}

// grid (ceil(B / 4), n_parts): wave (sample, part)
__global__ __launch_bounds__(256) void store_gather_fixed_kernel(Args a) {
  const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6), pi = blockIdx.y;
  if (b >= a.B) return;
  bool q_ok;
  const int64_t img = resolve_image(a, b, q_ok);
  if (pi == 0 && lane == 0 && img < 0) a.status[b] |= ST_BAD_INDEX;
  const Part& p = a.parts[pi];
  const int64_t row = p.key ? img : (q_ok ? (int64_t)a.sample_idx[b] : -1);
  copy_row(p, row < 0 ? 0 : row, b, row < 0, lane);
}

int fill_parts(Args& a, const int64_t* parts, int n_parts, int words, const char* who) {
  if (n_parts > STORE_MAX_PARTS) {
    sam_set_error("%s: %d parts (at most %d per call)", who, n_parts, STORE_MAX_PARTS);
    return SAM_ERR_UNSUPPORTED;
  }
  SAM_REQUIRE(n_parts >= 1 && parts, "%s: no parts", who);
  for (int k = 0; k < STORE_MAX_PARTS; ++k) a.parts[k] = Part{nullptr, 0, nullptr, 0, 0, 1, 0};
  for (int k = 0; k < n_parts; ++k) {
    const int64_t* w = parts + (int64_t)k * words;
    const uintptr_t src = (uintptr_t)w[0], dst = (uintptr_t)w[2];
    const int64_t ld_src = w[1], ld_dst = w[3], row_bytes = w[4], key = words > 5 ? w[5] : 0;
    SAM_REQUIRE(src && dst, "%s: part %d: null pointer", who, k);
    SAM_REQUIRE(row_bytes >= 1 && ld_src >= row_bytes && ld_dst >= row_bytes, "%s: part %d: need 1 <= row_bytes <= ld_src_bytes, ld_dst_bytes (row_bytes=%ld ld_src=%ld ld_dst=%ld)",
                who, k, (long)row_bytes, (long)ld_src, (long)ld_dst);
    SAM_REQUIRE(key == 0 || key == 1, "%s: part %d: key %ld (0: by question, 1: by image)", who, k, (long)key);
    const uintptr_t all = src | dst | (uintptr_t)ld_src | (uintptr_t)ld_dst;
    a.parts[k] = Part{(const char*)src, ld_src, (char*)dst, ld_dst, row_bytes, (all % 16) == 0 ? 16 : ((all % 4) == 0 ? 4 : 1), (int)key};
  }
  a.n_parts = n_parts;
  return SAM_OK;
}

}  // namespace

extern "C" int sam_store_gather_ragged(const int32_t* sample_idx, int B, const int32_t* image_of, int n_questions, const int64_t* row_off, int n_images,
                                       int64_t total_rows, int n_max, const int64_t* parts, int n_parts, int32_t* counts_out, int32_t* status, int cap_rows,
                                       void* stream) {
  const char* who = "sam_store_gather_ragged";
  SAM_REQUIRE(sample_idx && row_off && counts_out && status, "%s: null pointer (sample_idx, row_off, counts_out, status)", who);
  SAM_REQUIRE(B >= 1 && n_max >= 1 && cap_rows >= 1 && (int64_t)B * n_max < (int64_t)1 << 31, "%s: bad shape B=%d n_max=%d cap_rows=%d (need B, n_max, cap_rows >= 1 and B * n_max < 2^31)",
              who, B, n_max, cap_rows);
  SAM_REQUIRE(n_questions >= 1 && n_images >= 1 && total_rows >= 0, "%s: bad store n_questions=%d n_images=%d total_rows=%ld", who, n_questions, n_images, (long)total_rows);
  SAM_REQUIRE(image_of || n_questions == n_images, "%s: without image_of the samples are image indices: n_questions (%d) must equal n_images (%d)", who, n_questions, n_images);
  SAM_REQUIRE(((uintptr_t)sample_idx % 4) == 0 && ((uintptr_t)image_of % 4) == 0 && ((uintptr_t)counts_out % 4) == 0 && ((uintptr_t)status % 4) == 0 &&
              ((uintptr_t)row_off % 8) == 0, "%s: misaligned index / offset / count / status pointer", who);
  Args a;
  a.sample_idx = sample_idx; a.image_of = image_of; a.row_off = row_off; a.counts_out = counts_out; a.status = status; a.total_rows = total_rows;
  a.B = B; a.n_questions = n_questions; a.n_images = n_images; a.n_max = n_max; a.cap_rows = cap_rows;
  if (const int rc = fill_parts(a, parts, n_parts, 5, who)) return rc;
  const int64_t slots = (int64_t)B * n_max;
  store_gather_ragged_kernel<<<dim3((unsigned)((slots + 3) / 4), (unsigned)n_parts), dim3(256), 0, (hipStream_t)stream>>>(a);
  SAM_LAUNCH_CHECK();
  return SAM_OK;
}

extern "C" int sam_store_gather_fixed(const int32_t* sample_idx, int B, const int32_t* image_of, int n_questions, int n_images, const int64_t* parts,
                                      int n_parts, int32_t* status, void* stream) {
  const char* who = "sam_store_gather_fixed";
  SAM_REQUIRE(sample_idx && status, "%s: null pointer (sample_idx, status)", who);
  SAM_REQUIRE(B >= 1, "%s: bad shape B=%d (need B >= 1)", who, B);
  SAM_REQUIRE(n_questions >= 1 && n_images >= 1, "%s: bad store n_questions=%d n_images=%d", who, n_questions, n_images);
  SAM_REQUIRE(image_of || n_questions == n_images, "%s: without image_of the samples are image indices: n_questions (%d) must equal n_images (%d)", who, n_questions, n_images);
  SAM_REQUIRE(((uintptr_t)sample_idx % 4) == 0 && ((uintptr_t)image_of % 4) == 0 && ((uintptr_t)status % 4) == 0, "%s: misaligned index / status pointer", who);
  Args a;
  a.sample_idx = sample_idx; a.image_of = image_of; a.row_off = nullptr; a.counts_out = nullptr; a.status = status; a.total_rows = 0;
  a.B = B; a.n_questions = n_questions; a.n_images = n_images; a.n_max = 1; a.cap_rows = B;
  if (const int rc = fill_parts(a, parts, n_parts, 6, who)) return rc;
  store_gather_fixed_kernel<<<dim3((unsigned)((B + 3) / 4), (unsigned)n_parts), dim3(256), 0, (hipStream_t)stream>>>(a);
  SAM_LAUNCH_CHECK();
  return SAM_OK;
}
