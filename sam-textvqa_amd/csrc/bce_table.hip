// Masked BCE loss, its analytic gradient and the greedy predictions straight from the per-sample answer tables:
// M4CDecodingBCEWithMaskLoss (sam/task_utils.py:19-30) on the targets answer_sample_kernel (answers.hip) would have written for the drawn sequence, and
// the argmax the metric starts from (sam/datasets/metrics.py:26) -- without the dense [B, L, V + No] target tensor ever existing in memory.
//
// The grid of bce_kernel (rowops.hip): one decoding row per blockIdx.x, column chunks on blockIdx.y.  An unmasked row's block rebuilds the row's targets in
// LDS: zero-fill W = V + No floats (16-byte stores), barrier, scatter the handful of non-zeros with the sampler's own clamps, barrier; then bce_kernel's
// column loop runs with t read from LDS.  The per-element expressions are bce_kernel's, in its order, and so is the count reduction that feeds the gradient
// scale: the gradients are bit-identical to sam_bce_loss on the materialised targets.  Duplicate indices of a list all write one value (the tables list a
// step-0 index once; a hand-made table that lists one twice with two values races in the dense sampler as it does here): no atomics in the scatter.
// LDS: 4 * W bytes per block (20 KB at W = 5050: eight blocks per CU fit the 160 KB).  The row must fit the 64 KB a launch gets without opting in to
// more: W <= kMaxWidth = 16000, wider rows are refused by the entry point.
//
// Predictions: with `pred` the row is not split (gridDim.y = 1), so ONE block sees every score of the row and the argmax is deterministic without atomics:
// per thread in ascending column order, then a (value, lower index) butterfly across the wave and the four waves through LDS.  Masked rows are scanned too.
// NaN compares false with everything and is never selected; a row of nothing but NaN predicts 0.  +-inf order as usual.
//
// The loss itself is summed in a FIXED order, so that two runs on the same inputs return the same bits (fp32 atomicAdd per block lands in arrival order:
// one or two ulps of difference from run to run; sam_bce_loss in rowops.hip uses the same scheme).  Every block stores its part in a slot of a small device-resident scratch area
// and takes a ticket; the block that takes the last ticket adds the parts in index order and writes the loss (the "last block reduces" scheme).  Parts and
// tickets are agent-scope accesses (written through to / read from the memory side, past the per-XCD L2), ordered by an s_waitcnt between the part store
// and the ticket, as in gemm8w.hip's exchange: a release / acquire fence pair would write back the XCD's whole L2, full of this kernel's own gradient
// stores (measured: + 11 us per launch at B = 64).  No memset node, no second launch, no workspace argument.  The launch picks one
// of kLossSlots slots round-robin, so launches that overlap on other streams do not share one unless eight are in flight at once; grids of more than
// kMaxParts blocks (B * L > 16384) keep the atomic sum.
#include <atomic>

#include "common.h"
#include "sam_hip.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxWidth = 16000;
constexpr int kLossSlots = 8;
constexpr int kMaxParts = 16384;

__device__ float g_loss_part[kLossSlots][kMaxParts];
__device__ unsigned g_loss_arrived[kLossSlots];      // zero at load; the last block of a launch puts it back to zero

// rowops.hip's softplus_neg_abs, word for word: log(1 + e), e = exp(-|x|) in (0, 1]
__device__ __forceinline__ float softplus_neg_abs(float e) {
  return e < 1e-3f ? e * (1.0f - e * (0.5f - e * 0.33333334f)) : __logf(1.0f + e);
}

__device__ __forceinline__ void arg_better(float v, int c, float& bv, int& bc) {      // greater value, or the same value at a lower column
  if (v > bv || (v == bv && c < bc)) { bv = v; bc = c; }
}

template <int VEC, bool PRED>      // VEC 2: adjacent column pairs (everything even and 8-byte aligned), 1: any shape; PRED: also the row's argmax
__global__ __launch_bounds__(kThreads) void bce_table_kernel(const float* fixed, int64_t ldf, const float* ocr, int64_t ldoc, const int32_t* __restrict__ meta,
                                                             const int32_t* __restrict__ seq_len, const int16_t* __restrict__ seq_grp,
                                                             const int32_t* __restrict__ step0_idx, const float* __restrict__ step0_val,
                                                             const int32_t* __restrict__ grp_off, const int32_t* __restrict__ grp_extra, int S, int L, int G, int E,
                                                             const int32_t* __restrict__ choice, const float* mask, int R, int V, int No, float gscale,
                                                             const float* global_count, float* loss, bf16_t* d_fixed, int64_t lddf, float* d_ocr, int64_t lddo,
                                                             int64_t* pred, int slot) {
  extern __shared__ __align__(16) float trow[];          // the row's targets, W floats
  __shared__ float sred[4];
  __shared__ float smax[4];
  __shared__ int sarg[4];
  __shared__ int s_last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float cnt = 0.f;
  for (int r = tid; r < R; r += 256) cnt += mask[r];
  cnt = wave_sum(cnt);
  if (lane == 0) sred[wave] = cnt;
  __syncthreads();
  cnt = fmaxf(global_count ? global_count[0] : sred[0] + sred[1] + sred[2] + sred[3], 1.0f);      // (data parallel: see bce_kernel)
  __syncthreads();
  const float inv_cnt = 1.0f / cnt;
  const int W = V + No, r = blockIdx.x;
  const float m = mask[r];
  const float gs = m * inv_cnt * gscale;
  const bool grads = d_fixed != nullptr;
  float bv = -INFINITY;
  int bc = 0x7fffffff;
  float acc = 0.f;

  if (m == 0.f) {                    // a masked decoding step: zero gradient, nothing for the loss; its scores are read for the prediction only
    for (int c = VEC * (blockIdx.y * 256 + tid); c < W; c += VEC * 256 * gridDim.y) {
      const bool in_fixed = c < V;
      if (PRED) {
        if (VEC == 2) {
          const float2 x2 = in_fixed ? *reinterpret_cast<const float2*>(fixed + (int64_t)r * ldf + c) : *reinterpret_cast<const float2*>(ocr + (int64_t)r * ldoc + (c - V));
          arg_better(x2.x, c, bv, bc);
          arg_better(x2.y, c + 1, bv, bc);
        } else {
          arg_better(in_fixed ? fixed[(int64_t)r * ldf + c] : ocr[(int64_t)r * ldoc + (c - V)], c, bv, bc);
        }
      }
      if (grads) {
        if (VEC == 2) {
          if (in_fixed) *reinterpret_cast<unsigned*>(d_fixed + (int64_t)r * lddf + c) = 0u;
          else *reinterpret_cast<float2*>(d_ocr + (int64_t)r * lddo + (c - V)) = make_float2(0.f, 0.f);
        } else {
          if (in_fixed) d_fixed[(int64_t)r * lddf + c] = (bf16_t)0;
          else d_ocr[(int64_t)r * lddo + (c - V)] = 0.f;
        }
      }
    }
  } else {
    // ---- the row's targets, as answer_sample_kernel writes them (same clamps on every table entry) ----
    const int b = r / L, t = r - b * L;
    const int32_t* mt = meta + 4 * (int64_t)b;
    const int n_seq = min(mt[0], S), n0 = max(0, min(mt[1], S)), n_grp = max(0, min(mt[2], G)), n_ex = max(0, min(mt[3], E));
    int k = choice[b];
    if (k < 0 || k >= n_seq) k = -1;
    int dec = 0;
    const int16_t* grp_row = nullptr;
    if (k >= 0) {
      dec = min(1 + max(0, min(seq_len[(int64_t)b * S + k], L)), L);
      grp_row = seq_grp + ((int64_t)b * S + k) * L;
    }
    {
      const int n4 = W >> 2;
      float4* r4 = reinterpret_cast<float4*>(trow);
      for (int i = tid; i < n4; i += kThreads) r4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int i = 4 * n4 + tid; i < W; i += kThreads) trow[i] = 0.f;
    }
    __syncthreads();
    if (k >= 0 && t == 0) {
      const int32_t* si = step0_idx + (int64_t)b * S;
      const float* sv = step0_val + (int64_t)b * S;
      for (int i = tid; i < n0; i += kThreads) {
        const int idx = si[i];
        if (idx >= 0 && idx < W) trow[idx] = sv[i];
      }
    } else if (k >= 0 && t < dec) {
      const int g = grp_row[t];
      if (g >= 0 && g < n_grp) {
        const int32_t* off = grp_off + (int64_t)b * (G + 1);
        const int lo = max(0, min(off[g], n_ex)), hi = max(lo, min(off[g + 1], n_ex));
        const int32_t* ex = grp_extra + (int64_t)b * E;
        for (int i = lo + tid; i < hi; i += kThreads) {
          const int idx = ex[i];
          if (idx >= 0 && idx < W) trow[idx] = 1.0f;
        }
      }
    }
    __syncthreads();

    // ---- bce_kernel's column loop, targets from LDS ----
    for (int c = VEC * (blockIdx.y * 256 + tid); c < W; c += VEC * 256 * gridDim.y) {
      const bool in_fixed = c < V;
      float xs[2] = {0.f, 0.f}, ts[2] = {0.f, 0.f};
      if (VEC == 2) {
        const float2 x2 = in_fixed ? *reinterpret_cast<const float2*>(fixed + (int64_t)r * ldf + c) : *reinterpret_cast<const float2*>(ocr + (int64_t)r * ldoc + (c - V));
        const float2 t2 = *reinterpret_cast<const float2*>(trow + c);
        xs[0] = x2.x; xs[1] = x2.y; ts[0] = t2.x; ts[1] = t2.y;
      } else {
        xs[0] = in_fixed ? fixed[(int64_t)r * ldf + c] : ocr[(int64_t)r * ldoc + (c - V)];
        ts[0] = trow[c];
      }
      float gx[2];
#pragma unroll
      for (int e_ = 0; e_ < VEC; ++e_) {
        const float x = xs[e_], t_ = ts[e_];
        const float e = __expf(-fabsf(x));
        acc += fmaxf(x, 0.f) - x * t_ + softplus_neg_abs(e);
        const float inv = __builtin_amdgcn_rcpf(1.0f + e);
        const float sig = x >= 0.f ? inv : e * inv;
        gx[e_] = (sig - t_) * gs;
        if (PRED) arg_better(x, c + e_, bv, bc);
      }
      if (grads) {
        if (VEC == 2) {
          if (in_fixed) *reinterpret_cast<unsigned*>(d_fixed + (int64_t)r * lddf + c) = pack_bf16x2(gx[0], gx[1]);
          else *reinterpret_cast<float2*>(d_ocr + (int64_t)r * lddo + (c - V)) = make_float2(gx[0], gx[1]);
        } else {
          if (in_fixed) d_fixed[(int64_t)r * lddf + c] = f2bf(gx[0]);
          else d_ocr[(int64_t)r * lddo + (c - V)] = gx[0];
        }
      }
    }
  }

  if (PRED) {                        // (gridDim.y == 1: this block has seen the whole row)
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oc = __shfl_xor(bc, o, 64);
      arg_better(ov, oc, bv, bc);
    }
    if (lane == 0) { smax[wave] = bv; sarg[wave] = bc; }
  }
  acc = wave_sum(acc * m);
  if (lane == 0) sred[wave] = acc;
  __syncthreads();
  const unsigned nblk = gridDim.x * gridDim.y;
  if (tid == 0) {
    const float part = m != 0.f ? (sred[0] + sred[1] + sred[2] + sred[3]) * inv_cnt : 0.f;
    if (slot < 0) {
      if (m != 0.f) atomicAdd(loss, part);
    } else {
      __hip_atomic_store(&g_loss_part[slot][blockIdx.x * gridDim.y + blockIdx.y], part, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      s_last = __hip_atomic_fetch_add(&g_loss_arrived[slot], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nblk - 1u ? 1 : 0;
    }
    if (PRED) {
#pragma unroll
      for (int w = 1; w < 4; ++w) arg_better(smax[w], sarg[w], bv, bc);
      pred[r] = bc < W ? (int64_t)bc : 0;
    }
  }
  if (slot >= 0) {
    __syncthreads();
    if (s_last) {                    // every part was written through before its ticket was taken: the last ticket sees them all
      float a = 0.f;
      for (unsigned i = tid; i < nblk; i += kThreads) a += __hip_atomic_load(&g_loss_part[slot][i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      a = wave_sum(a);
      if (lane == 0) sred[wave] = a;
      __syncthreads();
      if (tid == 0) {
        loss[0] = (sred[0] + sred[1]) + (sred[2] + sred[3]);
        __hip_atomic_store(&g_loss_arrived[slot], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}

}  // namespace

extern "C" int sam_bce_loss_table(const float* fixed_scores, int64_t ld_fixed, const float* ocr_scores, int64_t ld_ocr, const int32_t* meta, const int32_t* seq_len,
                                  const int16_t* seq_grp, const int32_t* step0_idx, const float* step0_val, const int32_t* grp_idx, const int32_t* grp_off,
                                  const int32_t* grp_extra, int B, int S, int L, int G, int E, const int32_t* choice, const float* loss_mask, int R, int V, int No,
                                  float grad_scale, const float* global_count, float* loss, void* d_fixed, int64_t ld_dfixed, float* d_ocr, int64_t ld_docr,
                                  int64_t* pred, void* stream) {
  SAM_REQUIRE(fixed_scores && ocr_scores && loss_mask && loss && choice, "sam_bce_loss_table: null pointer");
  SAM_REQUIRE(meta && seq_len && seq_grp && step0_idx && step0_val && grp_idx && grp_off && grp_extra, "sam_bce_loss_table: null table pointer");
  SAM_REQUIRE((d_fixed == nullptr) == (d_ocr == nullptr), "sam_bce_loss_table: d_fixed and d_ocr must be given or omitted together");
  SAM_REQUIRE(R > 0 && V > 0 && No >= 0, "sam_bce_loss_table: bad shape");
  SAM_REQUIRE(B > 0 && L > 0 && (int64_t)B * L == R, "sam_bce_loss_table: R = %d rows, but B * L = %d * %d", R, B, L);
  SAM_REQUIRE(S > 0 && G > 0 && E > 0, "sam_bce_loss_table: table capacities must be positive (S %d, G %d, E %d)", S, G, E);
  SAM_REQUIRE(G <= 32767, "sam_bce_loss_table: G = %d does not fit the int16 group ids", G);
  SAM_REQUIRE((int64_t)V + No <= kMaxWidth, "sam_bce_loss_table: a row of V + No = %lld scores does not fit the %d-float LDS row", (long long)V + No, kMaxWidth);
  SAM_REQUIRE(ld_fixed >= V && ld_ocr >= No && (!d_fixed || (ld_dfixed >= V && ld_docr >= No)), "sam_bce_loss_table: a row stride is shorter than its row");
  SAM_REQUIRE(((uintptr_t)seq_grp % 2) == 0 && ((uintptr_t)pred % 8) == 0, "sam_bce_loss_table: misaligned operand");
  hipStream_t st = (hipStream_t)stream;
  const bool pairs = V % 2 == 0 && No % 2 == 0 && ld_fixed % 2 == 0 && ld_ocr % 2 == 0 && ld_dfixed % 2 == 0 && ld_docr % 2 == 0 &&
                     ((uintptr_t)fixed_scores % 8 == 0) && ((uintptr_t)ocr_scores % 8 == 0) && ((uintptr_t)d_ocr % 8 == 0) && ((uintptr_t)d_fixed % 4 == 0);
  const int per = pairs ? 2 : 1, W = V + No;
  // sam_bce_loss's chunking (one fp32 atomic per block lands on `loss`); a row that is predicted stays whole
  const int chunks = pred ? 1 : max(1, min(min(8, 1024 / R), ((W + per - 1) / per + 255) / 256));
  const size_t lds = (size_t)((W + 3) & ~3) * sizeof(float);
  const dim3 grid(R, chunks), block(kThreads);
  static std::atomic<unsigned> next_slot{0};
  const int slot = (int64_t)R * chunks <= kMaxParts ? (int)(next_slot.fetch_add(1u) % kLossSlots) : -1;
  if (slot < 0) {                    // the atomic sum starts from zero
    hipError_t e = hipMemsetAsync(loss, 0, sizeof(float), st);
    if (e != hipSuccess) { sam_set_error("sam_bce_loss_table: memset: %s", hipGetErrorString(e)); return (int)e; }
  }
#define SAM_BCE_TABLE_LAUNCH(VEC_, PRED_)                                                                                                                       \
  bce_table_kernel<VEC_, PRED_><<<grid, block, lds, st>>>(fixed_scores, ld_fixed, ocr_scores, ld_ocr, meta, seq_len, seq_grp, step0_idx, step0_val, grp_off,    \
                                                          grp_extra, S, L, G, E, choice, loss_mask, R, V, No, grad_scale, global_count, loss, (bf16_t*)d_fixed, \
                                                          ld_dfixed, d_ocr, ld_docr, pred, slot)
  if (pairs) {
    if (pred) SAM_BCE_TABLE_LAUNCH(2, true); else SAM_BCE_TABLE_LAUNCH(2, false);
  } else {
    if (pred) SAM_BCE_TABLE_LAUNCH(1, true); else SAM_BCE_TABLE_LAUNCH(1, false);
  }
#undef SAM_BCE_TABLE_LAUNCH
  SAM_LAUNCH_CHECK();
  return SAM_OK;
}
