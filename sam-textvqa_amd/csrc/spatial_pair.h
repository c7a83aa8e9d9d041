// Classification of one ordered box pair of the spatial relation graph (sam/spatial_utils.py:92-218), float64 in the reference's operation order.
// ONE copy of the arithmetic for the two kernels that need it: relation_kernel (spatial_graph.hip: boxes -> int8 [B,N,N,12]) and boxes_wave_kernel
// (mask_boxes.hip: boxes -> allow bits).  Both are compiled from these functions; nothing forces the compiler to contract the two inlined copies alike,
// so that they derive the same bits from a pair, sector boundaries included, is what tests/test_mask_boxes_gpu.py checks bit for bit.
// Relation codes: 1 a covers b, 2 a inside b, 3 IoU >= 0.5, 4..11 sector of the centre direction (if centre distance < limit), 12 self, 0 none / padding;
// channel = code-1; a context of width w adds the sector channels within +-w (wrapping in 4..11).
#pragma once
#include "common.h"

struct Box { double x0, y0, x1, y1; };
__device__ __forceinline__ bool covers(const Box& a, const Box& b) { return a.x0 < b.x0 && a.x1 > b.x1 && a.y0 < b.y0 && a.y1 > b.y1; }
// padding rows are all-zero boxes (textvqa_dataset.py pads with zeros; spatial_utils.py:104-106 skips rows whose coordinates sum to 0)
__device__ __forceinline__ bool box_valid(const Box& a) { return (a.x0 + a.y0 + a.x1 + a.y1) != 0.0; }

// sector codes of the pair (i, j), i < j: first = i -> j, second = j -> i   (spatial_utils.py:168-203)
__device__ __forceinline__ void sector_pair(const Box& bi, const Box& bj, int& cij, int& cji) {
  const double pi = 3.141592653589793;
  const double dy = 0.5 * (bi.y0 + bi.y1) - 0.5 * (bj.y0 + bj.y1);
  const double dx = 0.5 * (bi.x0 + bi.x1) - 0.5 * (bj.x0 + bj.x1);
  const double dist = sqrt(dy * dy + dx * dx);
  if (dist == 0.0) { cij = cji = 4; return; }    // reference: 0/0 -> nan -> both codes 4
  const double s = dy / dist, c = dx / dist;
  double li, lj;
  if (s >= 0 && c >= 0) { li = asin(s); lj = pi + li; }
  else if (s < 0 && c >= 0) { li = asin(s) + 2 * pi; lj = li - pi; }
  else if (s >= 0 && c < 0) { li = acos(c); lj = li + pi; }
  else { li = 2 * pi - acos(c); lj = li - pi; }
  const double q = pi / 4.0;
  cij = (int)ceil(li / q) + 3;
  cji = (int)ceil(lj / q) + 3;
}

// relation code of the ordered pair (row arow with box A) -> (column bcol with box Bx); limit = distance_threshold * sqrt(2)
__device__ __forceinline__ int pair_code(const Box& A, const Box& Bx, int arow, int bcol, double limit) {
  int code = 0;
  if (box_valid(A) && box_valid(Bx)) {
    if (arow == bcol) code = 12;
    else if (covers(A, Bx)) code = 1;
    else if (covers(Bx, A)) code = 2;
    else {
      const double iw = fmax(0.0, fmin(A.x1, Bx.x1) - fmax(A.x0, Bx.x0)), ih = fmax(0.0, fmin(A.y1, Bx.y1) - fmax(A.y0, Bx.y0));
      const double inter = iw * ih;
      const double areaA = (A.x1 - A.x0) * (A.y1 - A.y0), areaB = (Bx.x1 - Bx.x0) * (Bx.y1 - Bx.y0);
      // reference evaluates IoU(i, j) with i < j: boxAArea + boxBArea - interArea in that order
      const double uni = arow < bcol ? (areaA + areaB) - inter : (areaB + areaA) - inter;
      if (inter / uni >= 0.5) code = 3;
      else {
        const Box& bi = arow < bcol ? A : Bx;
        const Box& bj = arow < bcol ? Bx : A;
        const double dy = 0.5 * (bi.y0 + bi.y1) - 0.5 * (bj.y0 + bj.y1), dx = 0.5 * (bi.x0 + bi.x1) - 0.5 * (bj.x0 + bj.x1);
        if (sqrt(dy * dy + dx * dx) < limit) {
          int cij, cji;
          sector_pair(bi, bj, cij, cji);
          code = arow < bcol ? cij : cji;
        }
      }
    }
  }
  return code;
}

// bit h set <=> relation channel h (head h) sees the pair: the code's own channel plus, for the sector codes, the neighbours within +-width
__device__ __forceinline__ unsigned channel_word(int code, int width) {
  unsigned chan = 0;
  if (code > 0) chan |= 1u << (code - 1);
  if (code >= 4 && code <= 11)
    for (int k = 1; k <= width; ++k) {
      chan |= 1u << (4 + ((code - 4 + k) & 7) - 1);
      chan |= 1u << (4 + ((code - 4 - k) & 7) - 1);
    }
  return chan;
}

// a box row of the batch: fp32 or float64 elements, row stride ld >= 4, xyxy in columns 0..3
template <bool F64>
__device__ __forceinline__ Box load_box(const void* boxes, int64_t row, int64_t ld) {
  if (F64) {
    const double* p = static_cast<const double*>(boxes) + row * ld;
    return {p[0], p[1], p[2], p[3]};
  }
  const float* p = static_cast<const float*>(boxes) + row * ld;      // (row stride 5 in the batch: four scalar loads; fp32 -> f64 is exact)
  return {(double)p[0], (double)p[1], (double)p[2], (double)p[3]};
}

// box j of sample b in the concatenation obj | ocr
template <bool F64>
__device__ __forceinline__ Box load_oo_box(const void* obj, int64_t ld_obj, int n_obj, const void* ocr, int64_t ld_ocr, int n_ocr, int b, int j) {
  return j < n_obj ? load_box<F64>(obj, (int64_t)b * n_obj + j, ld_obj) : load_box<F64>(ocr, (int64_t)b * n_ocr + (j - n_obj), ld_ocr);
}
