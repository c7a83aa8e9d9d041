// M4C answer targets sampled on the GPU from per-sample answer tables (M4CAnswerProcessor.__call__, sam/datasets/processors.py:586-692,
// called for every drawn sample by sam/datasets/textvqa_dataset.py:350-365).  The string matching has no randomness and is done once per sample on the
// host (answers.build_answer_table); what is left per step -- draw one decoding sequence, write the dense targets, the previous-index inputs and both
// masks -- runs here, as a node of the (captured) training step, so every replay draws afresh.  (targets == NULL: everything but the dense targets; the
// loss then rebuilds each row from the tables, bce_table.hip.)
//
// One block per (decoding step t, sample b): the block zero-fills its targets row with 16-byte stores, waits at a barrier, then scatters that row's
// non-zeros: t = 0 the pre-merged (index, max score) list of the sample, 1 <= t < dec_step_num 1.0 at every index of the group of seq[t] (EOS past the
// end of the sequence).  No atomics: every value written is a pure function of the table and the draw, so the output is bit-reproducible.
// The draw: k = mulhi32(lowbias32 chain over (key, step, sample), n_seq), step read from device memory (the Trainer's step counter) plus a by-value delta.
#include "common.h"
#include "sam_hip.h"

namespace {

constexpr int kThreads = 256;

// keep in step with answers.draw_hash (the host twin)
__device__ __forceinline__ unsigned answer_draw_hash(unsigned long long key, long long step, unsigned sample) {
  const unsigned long long s = (unsigned long long)step;
  unsigned h = mix32((unsigned)key ^ 0xA0761D65u);
  h = mix32(h ^ (unsigned)(key >> 32));
  h = mix32(h ^ (unsigned)s);
  h = mix32(h ^ (unsigned)(s >> 32));
  return mix32(h ^ (sample * 0x9E3779B1u));
}

__global__ __launch_bounds__(kThreads) void answer_sample_kernel(const int32_t* __restrict__ meta, const int32_t* __restrict__ seq_len,
                                                                 const int16_t* __restrict__ seq_grp, const int32_t* __restrict__ step0_idx,
                                                                 const float* __restrict__ step0_val, const int32_t* __restrict__ grp_idx,
                                                                 const int32_t* __restrict__ grp_off, const int32_t* __restrict__ grp_extra, int S, int L, int G,
                                                                 int E, int W, int bos, unsigned long long key, const int64_t* step_dev, long long step,
                                                                 const int32_t* force_choice, float* targets, int64_t ld, int64_t* prev_inds, float* loss_mask,
                                                                 float* acc_mask, int32_t* choice) {
  const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int32_t* m = meta + 4 * (int64_t)b;
  const int n_seq = min(m[0], S), n0 = max(0, min(m[1], S)), n_grp = max(0, min(m[2], G)), n_ex = max(0, min(m[3], E));
  int k = -1;
  if (n_seq > 0) {
    if (force_choice) {
      k = force_choice[b];
      if (k < 0 || k >= n_seq) k = -1;                   // a forced choice outside the sample's list: no sequence (all-zero outputs, choice -1)
    } else {
      const long long st = (step_dev ? (long long)*step_dev : 0ll) + step;
      k = (int)(((unsigned long long)answer_draw_hash(key, st, (unsigned)b) * (unsigned)n_seq) >> 32);
    }
  }
  int dec = 0;
  const int16_t* grp_row = nullptr;
  if (k >= 0) {
    dec = min(1 + max(0, min(seq_len[(int64_t)b * S + k], L)), L);
    grp_row = seq_grp + ((int64_t)b * S + k) * L;
  }

  if (targets) {                                         // (NULL: the loss reads the tables itself, sam_bce_loss_table -- no dense row is written)
    float* row = targets + ((int64_t)b * L + t) * ld;
    if (((uintptr_t)row & 15) == 0) {
      const int n4 = W >> 2;
      float4* r4 = reinterpret_cast<float4*>(row);
      for (int i = tid; i < n4; i += kThreads) r4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int i = 4 * n4 + tid; i < W; i += kThreads) row[i] = 0.f;
    } else {
      for (int i = tid; i < W; i += kThreads) row[i] = 0.f;
    }
    __syncthreads();                                       // (workgroup release / acquire: the zeros land before the scatter below)

    if (k >= 0 && t == 0) {
      const int32_t* si = step0_idx + (int64_t)b * S;
      const float* sv = step0_val + (int64_t)b * S;
      for (int i = tid; i < n0; i += kThreads) {
        const int idx = si[i];
        if (idx >= 0 && idx < W) row[idx] = sv[i];
      }
    } else if (k >= 0 && t < dec) {
      const int g = grp_row[t];
      if (g >= 0 && g < n_grp) {
        const int32_t* off = grp_off + (int64_t)b * (G + 1);
        const int lo = max(0, min(off[g], n_ex)), hi = max(lo, min(off[g + 1], n_ex));
        const int32_t* ex = grp_extra + (int64_t)b * E;
        for (int i = lo + tid; i < hi; i += kThreads) {
          const int idx = ex[i];
          if (idx >= 0 && idx < W) row[idx] = 1.0f;
        }
      }
    }
  }

  if (tid == 0) {                                        // this step's entries of the per-sample vectors
    int64_t prev = 0;
    if (k >= 0 && t < dec) {
      if (t == 0) {
        prev = bos;
      } else {
        const int g = grp_row[t - 1];
        prev = (g >= 0 && g < n_grp) ? (int64_t)grp_idx[(int64_t)b * G + g] : 0;
      }
    }
    prev_inds[(int64_t)b * L + t] = prev;
    loss_mask[(int64_t)b * L + t] = (k >= 0 && t < dec) ? 1.0f : 0.0f;
    acc_mask[(int64_t)b * L + t] = (k >= 0 && t < dec - 1) ? 1.0f : 0.0f;
    if (t == 0) choice[b] = k;
  }
}

}  // namespace

extern "C" int sam_answer_sample(const int32_t* meta, const int32_t* seq_len, const int16_t* seq_grp, const int32_t* step0_idx, const float* step0_val,
                                 const int32_t* grp_idx, const int32_t* grp_off, const int32_t* grp_extra, int B, int S, int L, int G, int E, int W, int bos,
                                 uint64_t key, const int64_t* step_dev, int64_t step, const int32_t* force_choice, float* targets, int64_t ld,
                                 int64_t* prev_inds, float* loss_mask, float* acc_mask, int32_t* choice, void* stream) {
  SAM_REQUIRE(meta && seq_len && seq_grp && step0_idx && step0_val && grp_idx && grp_off && grp_extra, "sam_answer_sample: null table pointer");
  SAM_REQUIRE(prev_inds && loss_mask && acc_mask && choice, "sam_answer_sample: null output pointer");
  SAM_REQUIRE(B > 0 && B <= 65535, "sam_answer_sample: batch %d outside 1..65535", B);
  SAM_REQUIRE(L > 0 && L <= 65535, "sam_answer_sample: %d decoding steps outside 1..65535", L);
  SAM_REQUIRE(S > 0 && G > 0 && E > 0, "sam_answer_sample: table capacities must be positive (S %d, G %d, E %d)", S, G, E);
  SAM_REQUIRE(G <= 32767, "sam_answer_sample: G = %d does not fit the int16 group ids", G);
  SAM_REQUIRE(W > 0 && (!targets || ld >= W), "sam_answer_sample: need 0 < W <= ld (W %d, ld %lld)", W, (long long)ld);
  SAM_REQUIRE(bos >= 0 && bos < W, "sam_answer_sample: bos %d outside [0, %d)", bos, W);
  SAM_REQUIRE(((uintptr_t)targets % 4) == 0 && ((uintptr_t)prev_inds % 8) == 0 && ((uintptr_t)seq_grp % 2) == 0, "sam_answer_sample: misaligned operand");
  // without targets only thread 0 of a block has work: one wave per block
  answer_sample_kernel<<<dim3((unsigned)L, (unsigned)B), dim3(targets ? kThreads : 64), 0, (hipStream_t)stream>>>(
      meta, seq_len, seq_grp, step0_idx, step0_val, grp_idx, grp_off, grp_extra, S, L, G, E, W, bos, (unsigned long long)key, step_dev, (long long)step,
      force_choice, targets, ld, prev_inds, loss_mask, acc_mask, choice);
  SAM_LAUNCH_CHECK();
  return SAM_OK;
}
