// PyTorch-ROCm custom ops (namespace sam_hip) over the C ABI of libsam_hip.so.
//
// The reference has no operator layer (eager PyTorch inside sam/sa_m4c.py); BASELINE.json's north star asks for the hot path to be "exposed to
// Python through PyTorch-ROCm custom ops".  This file is that layer: TORCH_LIBRARY schemas + ROCm implementations that check their tensors
// (TORCH_CHECK -> RuntimeError), allocate outputs through ATen, enqueue on c10::hip::getCurrentHIPStream() and never synchronise.
// No arithmetic happens here: every op is one or several calls into include/sam_hip.h.
//   fine-grained ops   sam_hip::linear, spatial_attn_fwd / _bwd, layernorm_fwd / _bwd, pack_masks, mask_bits_prefix_lm, mask_bits_from_additive,
//                      pack_relations (+ _bhnn), ptr_scores (+ _bwd), bce_loss (+ _table), sumsq, adam_step, step_advance, answer_sample (+ _notargets)   (SURVEY 8(b)'s op list; the model's
//                      masks, pointer scores, loss and optimizer go through these)
//   coarse ops         sam_hip::encoder_layer_fwd / _bwd: one SpatialBertLayer / BertLayer (sam/sa_m4c.py:660-684) = 7 launches forward,
//                      ~12 backward, enqueued from C++ -- the Python/ctypes route costs ~20 us of host time per launch, 5.7 ms per training
//                      step against 8 ms of GPU time.
// Built by sam_textvqa_amd/_build.py with g++ against the torch headers; links libsam_hip.so from its own directory.
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <tuple>
#include <string>
#include <cstdlib>
#include <map>
#include <mutex>
#include <vector>

#include "sam_hip.h"
#include "sam_hip_text.h"
#include "sam_hip_answers.h"
#include "sam_hip_step.h"
#include "sam_hip_question.h"
#include "sam_hip_fasttext.h"
#include "sam_hip_metrics.h"
#include "sam_hip_eval.h"
#include "sam_hip_textprep.h"
#include "sam_hip_unicode.h"
#include "sam_hip_aux_targets.h"
#include "sam_hip_aux_stats.h"

namespace {

using at::Tensor;
using c10::optional;

void* cur_stream() { return (void*)c10::hip::getCurrentHIPStream().stream(); }

void ok(int rc, const char* what) { TORCH_CHECK(rc == 0, what, " failed (rc=", rc, "): ", sam_last_error()); }

const Tensor& need(const Tensor& t, at::ScalarType dt, const char* name) {
  TORCH_CHECK(t.defined() && t.is_cuda(), name, " must be a GPU tensor (this package has no CPU path)");
  TORCH_CHECK(t.scalar_type() == dt, name, ": expected dtype ", dt, ", got ", t.scalar_type());
  return t;
}
void need2d(const Tensor& t, const char* name) {
  need(t, at::kBFloat16, name);
  TORCH_CHECK(t.dim() == 2 && t.stride(1) == 1, name, ": need a 2-D bf16 tensor with contiguous last dim");
}
void* p(const Tensor& t) { return t.defined() ? t.data_ptr() : nullptr; }
void* p(const optional<Tensor>& t) { return t.has_value() && t->defined() ? t->data_ptr() : nullptr; }

// ---------------------------------------------------------------------------------------------------------------- GEMM (mirror of ops.gemm)
struct GemmOpt {
  int epilogue = SAM_EPI_NONE;
  const Tensor* bias = nullptr;
  const Tensor* residual = nullptr;
  const Tensor* aux_in = nullptr;
  Tensor* aux_out = nullptr;
  float p_drop = 0.f;
  int64_t seed = 0, offset = 0;
  bool out_f32 = false;
  sam_ln_fuse* ln = nullptr;       // gemm_ln: LayerNorm behind a BIAS_DROPOUT_RES epilogue, fused into the split-K reduction pass when there is one
};

Tensor gemm(const Tensor& a, const Tensor& b, bool a_kc, bool b_kc, const GemmOpt& o) {
  need2d(a, "gemm A"); need2d(b, "gemm B");
  const int64_t M = a_kc ? a.size(0) : a.size(1), K = a_kc ? a.size(1) : a.size(0), N = b_kc ? b.size(0) : b.size(1);
  Tensor out = at::empty({M, N}, a.options().dtype(o.out_f32 ? at::kFloat : at::kBFloat16));
  sam_gemm_desc d = {};
  d.M = (int32_t)M; d.N = (int32_t)N; d.K = (int32_t)K;
  d.a_kcontig = a_kc; d.b_kcontig = b_kc; d.c_is_f32 = o.out_f32; d.epilogue = o.epilogue;
  d.A = a.data_ptr(); d.lda = a.stride(0); d.B = b.data_ptr(); d.ldb = b.stride(0); d.C = out.data_ptr(); d.ldc = out.stride(0);
  d.bias = o.bias ? (const float*)o.bias->data_ptr() : nullptr;
  if (o.residual) { d.residual = o.residual->data_ptr(); d.ldr = o.residual->stride(0); }
  if (o.aux_out) { d.aux_out = o.aux_out->data_ptr(); d.ld_aux = o.aux_out->stride(0); }
  if (o.aux_in) { d.aux_in = o.aux_in->data_ptr(); d.ld_aux = o.aux_in->stride(0); }
  d.p_drop = o.p_drop; d.seed = (uint64_t)o.seed; d.offset = (uint64_t)o.offset;
  d.ln = o.ln;
  Tensor ws;
  if (M <= 4096 && K >= 1536 && M * N <= (4 << 20)) {   // skinny problem with a long K (TextBert's 20 tokens/sample): the library may split K
    d.split_k = -1;                                      // and fold the epilogue into the partial-sum reduction
    const int64_t bytes = std::min<int64_t>(8 * (M * N + M) * 4, (int64_t)96 << 20);
    ws = at::empty({(bytes + 3) / 4}, a.options().dtype(at::kFloat));
    d.ws = (float*)ws.data_ptr(); d.ws_bytes = ws.numel() * 4; d.defer_reduce = 1;
  }
  ok(sam_gemm_bf16(&d, cur_stream()), "sam_gemm_bf16");
  return out;
}

std::tuple<Tensor, Tensor, Tensor> ln_fwd(const Tensor& x, const Tensor& gamma, const Tensor& beta, double eps);
// LayerNorm(gemm(...)) -> (z, y, mean, rstd): mirror of ops.gemm_ln (sam_ln_fuse when the library splits K, sam_layernorm_fwd otherwise: same bits)
std::tuple<Tensor, Tensor, Tensor, Tensor> gemm_ln(const Tensor& a, const Tensor& b, const Tensor& gamma, const Tensor& beta, double eps, GemmOpt o) {
  const int64_t M = a.size(0), N = b.size(0);
  if (N % 4 || N > 2048 || gamma.scalar_type() != at::kFloat || beta.scalar_type() != at::kFloat) {
    Tensor z = gemm(a, b, true, true, o);
    auto [y, mean, rstd] = ln_fwd(z, gamma, beta, eps);
    return {z, y, mean, rstd};
  }
  Tensor y = at::empty({M, N}, a.options()), mean = at::empty({M}, a.options().dtype(at::kFloat)), rstd = at::empty({M}, a.options().dtype(at::kFloat));
  sam_ln_fuse ln = {(const float*)gamma.data_ptr(), (const float*)beta.data_ptr(), (float)eps, y.data_ptr(), y.stride(0), (float*)mean.data_ptr(), (float*)rstd.data_ptr(), 0, nullptr, 0};
  if (M >= 2048) {
    // MMT-size products: the exchange workspace of the LayerNorm inside the launch -- one zero-filled buffer per (device, stream), grown on demand; every launch
    // leaves its counters zero again (include/sam_hip.h: sam_ln_fuse.xws)
    static std::map<std::pair<int, void*>, Tensor> cache;
    const int64_t bytes = sam_gemm_ln_ws_bytes((int)M, (int)N);
    Tensor& xws = cache[{(int)a.get_device(), cur_stream()}];
    if (!xws.defined() || xws.numel() * 4 < bytes) xws = at::zeros({(bytes + 3) / 4}, a.options().dtype(at::kFloat));
    ln.xws = (float*)xws.data_ptr(); ln.xws_bytes = xws.numel() * 4;
  }
  o.ln = &ln;
  Tensor z = gemm(a, b, true, true, o);
  if (ln.done) return {z, y, mean, rstd};
  auto [y2, mean2, rstd2] = ln_fwd(z, gamma, beta, eps);
  return {z, y2, mean2, rstd2};
}

// dW += dy^T x (and db += colsum(dy)) for up to 8 jobs in one launch
struct WgradJob { const Tensor* dy; const Tensor* x; const Tensor* dw; const Tensor* db; };
void wgrad_grouped(const std::vector<WgradJob>& jobs, bool accumulate = true) {
  sam_gemm_desc d[20] = {};
  TORCH_CHECK(jobs.size() >= 1 && jobs.size() <= 20, "wgrad_grouped: 1..20 jobs");
  for (size_t q = 0; q < jobs.size(); ++q) {
    const WgradJob& j = jobs[q];
    d[q].M = (int32_t)j.dy->size(1); d[q].N = (int32_t)j.x->size(1); d[q].K = (int32_t)j.dy->size(0);
    d[q].c_is_f32 = 1; d[q].accumulate = accumulate ? 1 : 0; d[q].epilogue = SAM_EPI_NONE;
    d[q].A = j.dy->data_ptr(); d[q].lda = j.dy->stride(0); d[q].B = j.x->data_ptr(); d[q].ldb = j.x->stride(0);
    d[q].C = j.dw->data_ptr(); d[q].ldc = j.dw->stride(0);
    d[q].bias_grad = j.db ? (float*)j.db->data_ptr() : nullptr;
  }
  // exchange workspace of the 8-wave grouped kernel: one zero-filled buffer per (device, stream), grown on demand; the kernel leaves its flag words
  // zero and launches on one stream are ordered, so consecutive calls share it
  {
    static std::mutex mu;
    static std::map<std::pair<int, void*>, Tensor> cache;
    const int64_t bytes = sam_gemm_grouped_ws_bytes(d, (int)jobs.size());
    std::lock_guard<std::mutex> lock(mu);
    Tensor& ws = cache[{(int)jobs[0].dy->get_device(), cur_stream()}];
    if (!ws.defined() || ws.numel() * 4 < bytes) ws = at::zeros({(bytes + 3) / 4}, jobs[0].dy->options().dtype(at::kFloat));
    d[0].ws = (float*)ws.data_ptr(); d[0].ws_bytes = ws.numel() * 4;
  }
  ok(sam_gemm_bf16_grouped(d, (int)jobs.size(), cur_stream()), "sam_gemm_bf16_grouped");
}

// ---------------------------------------------------------------------------------------------------------------- attention / layernorm
std::tuple<Tensor, Tensor, Tensor> attn_fwd(const Tensor& qkv, const Tensor& allow, int64_t batch, int64_t heads, double scale, double p_drop, int64_t seed,
                                            int64_t offset) {
  need2d(qkv, "qkv"); need(allow, at::kInt, "allow");
  TORCH_CHECK(allow.dim() == 4 && allow.is_contiguous(), "allow must be a contiguous int32 [B, H|1, N, NW] tensor");
  const int64_t rows = qkv.size(0), d_model = qkv.size(1) / 3, n = rows / batch;
  Tensor out = at::empty({rows, d_model}, qkv.options());
  Tensor lse2 = at::empty({batch, heads, n}, qkv.options().dtype(at::kFloat));
  Tensor keep = p_drop > 0 ? at::empty({batch, heads, n, allow.size(3)}, allow.options()) : Tensor();
  ok(sam_attn_fwd(qkv.data_ptr(), (const uint32_t*)allow.data_ptr(), allow.stride(0), allow.size(1) == 1 ? 0 : allow.stride(1), (int)batch, (int)n, (int)heads,
                  (int)(d_model / heads), (float)scale, (float)p_drop, (uint64_t)seed, (uint64_t)offset, out.data_ptr(), (float*)lse2.data_ptr(),
                  (uint32_t*)p(keep), cur_stream()),
     "sam_attn_fwd");
  return {out, lse2, keep.defined() ? keep : at::empty({0}, allow.options())};
}

// training forward: also returns the bf16 rounding residual of the output (what the one-pass backward takes delta from)
std::tuple<Tensor, Tensor, Tensor, Tensor> attn_fwd_train(const Tensor& qkv, const Tensor& allow, int64_t batch, int64_t heads, double scale, double p_drop, int64_t seed,
                                                          int64_t offset) {
  need2d(qkv, "qkv"); need(allow, at::kInt, "allow");
  TORCH_CHECK(allow.dim() == 4 && allow.is_contiguous(), "allow must be a contiguous int32 [B, H|1, N, NW] tensor");
  const int64_t rows = qkv.size(0), d_model = qkv.size(1) / 3, n = rows / batch;
  Tensor out = at::empty({rows, d_model}, qkv.options());
  Tensor out_lo = at::empty({rows, d_model}, qkv.options());
  Tensor lse2 = at::empty({batch, heads, n}, qkv.options().dtype(at::kFloat));
  Tensor keep = p_drop > 0 ? at::empty({batch, heads, n, allow.size(3)}, allow.options()) : Tensor();
  ok(sam_attn_fwd_train(qkv.data_ptr(), (const uint32_t*)allow.data_ptr(), allow.stride(0), allow.size(1) == 1 ? 0 : allow.stride(1), (int)batch, (int)n, (int)heads,
                        (int)(d_model / heads), (float)scale, (float)p_drop, (uint64_t)seed, (uint64_t)offset, out.data_ptr(), out_lo.data_ptr(), (float*)lse2.data_ptr(),
                        (uint32_t*)p(keep), cur_stream()),
     "sam_attn_fwd_train");
  return {out, lse2, keep.defined() ? keep : at::empty({0}, allow.options()), out_lo};
}

static bool fused_attn_bwd_enabled(int64_t n) {
  // read on every call, as ops.attn_bwd does: a test or an A/B script that flips SAM_ATTN_BWD_FUSED between calls must see the same route on the
  // per-kernel (Python) path and on this coarse one
  const char* s = getenv("SAM_ATTN_BWD_FUSED");
  return !(s && s[0] == '0') && n <= sam_attn_bwd_fused_max_n();
}

Tensor attn_bwd_fused(const Tensor& dout, const Tensor& qkv, const Tensor& out, const Tensor& out_lo, const Tensor& lse2, const Tensor& allow, const Tensor& keep,
                      int64_t batch, int64_t heads, double scale, double p_drop) {
  need2d(dout, "dout"); need2d(qkv, "qkv"); need2d(out, "out"); need2d(out_lo, "out_lo"); need(lse2, at::kFloat, "lse2"); need(allow, at::kInt, "allow");
  const int64_t rows = qkv.size(0), d_model = qkv.size(1) / 3, n = rows / batch;
  Tensor dqkv = at::empty_like(qkv);
  const bool has_keep = keep.defined() && keep.numel() > 0;
  ok(sam_attn_bwd_fused(dout.data_ptr(), qkv.data_ptr(), out.data_ptr(), out_lo.data_ptr(), (const float*)lse2.data_ptr(), (const uint32_t*)allow.data_ptr(),
                        allow.stride(0), allow.size(1) == 1 ? 0 : allow.stride(1), has_keep ? (const uint32_t*)keep.data_ptr() : nullptr, (int)batch, (int)n, (int)heads,
                        (int)(d_model / heads), (float)scale, (float)p_drop, dqkv.data_ptr(), cur_stream()),
     "sam_attn_bwd_fused");
  return dqkv;
}

Tensor attn_bwd(const Tensor& dout, const Tensor& qkv, const Tensor& lse2, const Tensor& allow, const Tensor& keep, int64_t batch, int64_t heads, double scale,
                double p_drop) {
  need2d(dout, "dout"); need2d(qkv, "qkv"); need(lse2, at::kFloat, "lse2"); need(allow, at::kInt, "allow");
  const int64_t rows = qkv.size(0), d_model = qkv.size(1) / 3, n = rows / batch;
  Tensor dqkv = at::empty_like(qkv);
  Tensor delta = at::empty({batch, heads, n}, lse2.options());
  const bool has_keep = keep.defined() && keep.numel() > 0;
  ok(sam_attn_bwd(dout.data_ptr(), qkv.data_ptr(), (const float*)lse2.data_ptr(), (const uint32_t*)allow.data_ptr(), allow.stride(0),
                  allow.size(1) == 1 ? 0 : allow.stride(1), has_keep ? (const uint32_t*)keep.data_ptr() : nullptr, (int)batch, (int)n, (int)heads,
                  (int)(d_model / heads), (float)scale, (float)p_drop, dqkv.data_ptr(), (float*)delta.data_ptr(), cur_stream()),
     "sam_attn_bwd");
  return dqkv;
}

std::tuple<Tensor, Tensor, Tensor> ln_fwd(const Tensor& x, const Tensor& gamma, const Tensor& beta, double eps) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.stride(1) == 1 && (x.scalar_type() == at::kBFloat16 || x.scalar_type() == at::kFloat),
              "layernorm_fwd: need a 2-D bf16/fp32 GPU tensor with contiguous rows");
  need(gamma, at::kFloat, "gamma"); need(beta, at::kFloat, "beta");
  const int64_t m = x.size(0), d = x.size(1);
  Tensor y = at::empty({m, d}, x.options().dtype(at::kBFloat16));
  Tensor mean = at::empty({m}, x.options().dtype(at::kFloat)), rstd = at::empty({m}, x.options().dtype(at::kFloat));
  ok(sam_layernorm_fwd(x.data_ptr(), x.scalar_type() == at::kFloat, x.stride(0), (const float*)gamma.data_ptr(), (const float*)beta.data_ptr(), (float)eps, (int)m,
                       (int)d, y.data_ptr(), y.stride(0), (float*)mean.data_ptr(), (float*)rstd.data_ptr(), cur_stream()),
     "sam_layernorm_fwd");
  return {y, mean, rstd};
}

// -> (dx, dx_dropped or undefined); dgamma / dbeta / dbias accumulated in place
// Deferred LayerNorm finalizes (include/sam_hip.h: sam_layernorm_bwd_finalize_batch): when switched on (set_ln_defer, by the Trainer for the span of
// a backward pass) the LayerNorm backwards of the coarse encoder-layer op leave their partial sums in private workspaces queued here, and
// ln_finalize_flush reduces all of them in one launch.  One queue per process (the backward pass runs on one thread at a time).
struct LnQueue {
  std::mutex mu;
  bool defer = false;
  int64_t D = 0;
  std::vector<sam_ln_finalize_item> items;
  std::vector<Tensor> keep;
};
LnQueue& ln_queue() { static LnQueue q; return q; }

std::tuple<Tensor, Tensor> ln_bwd(const Tensor& dy, const Tensor& x, const Tensor& mean, const Tensor& rstd, const Tensor& gamma, const Tensor& dgamma,
                                  const Tensor& dbeta, const Tensor* dbias, bool want_dropped, double p_drop, int64_t seed, int64_t offset, bool accumulate = true,
                                  bool may_defer = false) {
  need2d(dy, "dy");
  const int64_t m = x.size(0), d = x.size(1);
  Tensor dx = at::empty({m, d}, dy.options());
  Tensor dxd = (want_dropped && p_drop > 0) ? at::empty({m, d}, dy.options()) : Tensor();
  Tensor ws = at::empty({(sam_layernorm_bwd_ws_bytes((int)d) + 3) / 4}, dy.options().dtype(at::kFloat));
  LnQueue& q = ln_queue();
  bool defer = false;
  if (may_defer) {
    std::lock_guard<std::mutex> lock(q.mu);
    defer = q.defer && (q.items.empty() || q.D == d);
    if (defer) {
      q.D = d;
      q.items.push_back({(const float*)ws.data_ptr(), (int32_t)sam_layernorm_bwd_partial_rows((int)m), accumulate ? 1 : 0, (float*)dgamma.data_ptr(),
                         (float*)dbeta.data_ptr(), dbias ? (float*)dbias->data_ptr() : nullptr});
      q.keep.push_back(ws);
    }
  }
  ok(sam_layernorm_bwd(dy.data_ptr(), dy.stride(0), x.data_ptr(), x.scalar_type() == at::kFloat, x.stride(0), (const float*)mean.data_ptr(),
                       (const float*)rstd.data_ptr(), (const float*)gamma.data_ptr(), (int)m, (int)d, dx.data_ptr(), p(dxd), dx.stride(0), (float)p_drop,
                       (uint64_t)seed, (uint64_t)offset, (float*)dgamma.data_ptr(), (float*)dbeta.data_ptr(), dbias ? (float*)dbias->data_ptr() : nullptr,
                       (accumulate ? 1 : 0) | (defer ? 4 : 0), (float*)ws.data_ptr(), cur_stream()),
     "sam_layernorm_bwd");
  return {dx, dxd.defined() ? dxd : (want_dropped ? dx : Tensor())};
}

void set_ln_defer(bool on) {
  LnQueue& q = ln_queue();
  std::lock_guard<std::mutex> lock(q.mu);
  q.defer = on;
}

void ln_finalize_flush() {
  LnQueue& q = ln_queue();
  std::lock_guard<std::mutex> lock(q.mu);
  if (q.items.empty()) return;
  ok(sam_layernorm_bwd_finalize_batch(q.items.data(), (int)q.items.size(), (int)q.D, cur_stream()), "sam_layernorm_bwd_finalize_batch");
  q.items.clear();
  q.keep.clear();          // (the flush runs on the stream the partials were written on: stream order protects the workspaces)
}

void ln_finalize_clear() {      // a backward pass that raised: drop what it queued (the partial-sum workspaces may already be gone) and stop deferring
  LnQueue& q = ln_queue();
  std::lock_guard<std::mutex> lock(q.mu);
  q.items.clear();
  q.keep.clear();
  q.defer = false;
}

// ---------------------------------------------------------------------------------------------------------------- masks (pack_relations)
int64_t words_per_row(int64_t n) {
  const int nw = sam_attn_words_per_row((int)n);
  TORCH_CHECK(nw > 0, "sequence length ", n, " exceeds the fused-attention limit (384 keys)");
  return nw;
}
// question / object / OCR padding masks (int64) -> (key_valid u8 [B, T+No+Nc], question u8 [B,T], ocr u8 [B,Nc]); sa_m4c.py:805-812, :386, :889
std::tuple<Tensor, Tensor, Tensor> pack_masks(const Tensor& q, const Tensor& o, const Tensor& c) {
  need(q, at::kLong, "question_mask"); need(o, at::kLong, "pad_obj_mask"); need(c, at::kLong, "pad_ocr_mask");
  TORCH_CHECK(q.dim() == 2 && o.dim() == 2 && c.dim() == 2 && q.is_contiguous() && o.is_contiguous() && c.is_contiguous(), "pack_masks: contiguous [B, n] masks");
  const int64_t b = q.size(0), t = q.size(1), no = o.size(1), nc = c.size(1);
  auto u8 = q.options().dtype(at::kByte);
  Tensor kv = at::empty({b, t + no + nc}, u8), q8 = at::empty({b, t}, u8), c8 = at::empty({b, nc}, u8);
  ok(sam_pack_masks_u8((const int64_t*)q.data_ptr(), (int)t, (const int64_t*)o.data_ptr(), (int)no, (const int64_t*)c.data_ptr(), (int)nc, (int)b,
                       (uint8_t*)kv.data_ptr(), (uint8_t*)q8.data_ptr(), (uint8_t*)c8.data_ptr(), cur_stream()), "sam_pack_masks_u8");
  return {kv, q8, c8};
}
Tensor mask_bits_prefix_lm(const Tensor& key_valid, int64_t n_dec) {                  // sa_m4c.py:805-844
  need(key_valid, at::kByte, "key_valid");
  TORCH_CHECK(key_valid.dim() == 2 && key_valid.is_contiguous(), "key_valid: contiguous uint8 [B, n_enc]");
  const int64_t b = key_valid.size(0), n_enc = key_valid.size(1), n = n_enc + n_dec, nw = words_per_row(n);
  Tensor out = at::empty({b, 1, n, nw}, key_valid.options().dtype(at::kInt));
  ok(sam_mask_bits_prefix_lm((const uint8_t*)key_valid.data_ptr(), (int)b, (int)n_enc, (int)n_dec, (int)nw, (uint32_t*)out.data_ptr(), cur_stream()), "sam_mask_bits_prefix_lm");
  return out;
}
Tensor mask_bits_from_additive(const Tensor& mask) {                                  // sa_m4c.py:453-455
  need(mask, at::kFloat, "attention_mask");
  TORCH_CHECK(mask.dim() == 4 && mask.size(1) == 1 && mask.size(2) == mask.size(3) && mask.is_contiguous(), "attention_mask must be a contiguous [B,1,N,N] tensor");
  const int64_t b = mask.size(0), n = mask.size(2), nw = words_per_row(n);
  Tensor out = at::empty({b, 1, n, nw}, mask.options().dtype(at::kInt));
  ok(sam_mask_bits_from_additive((const float*)mask.data_ptr(), (int)b, (int)n, (int)nw, (uint32_t*)out.data_ptr(), cur_stream()), "sam_mask_bits_from_additive");
  return out;
}
// the relation tensor of the batch (int8 [B, Noo, Noo, R] multi-hot, dataset layout) AND-ed into the base bits, per head; sa_m4c.py:470-552,568
Tensor pack_relations(const Tensor& base_bits, const Tensor& adj, int64_t n_txt, int64_t heads, int64_t quadrant_bits) {
  need(base_bits, at::kInt, "base_bits"); need(adj, at::kChar, "spatial_adj_matrix");
  TORCH_CHECK(base_bits.dim() == 4 && base_bits.is_contiguous() && adj.dim() == 4 && adj.is_contiguous(), "pack_relations: contiguous base [B,1,N,NW], adj [B,Noo,Noo,R]");
  const int64_t b = base_bits.size(0), n = base_bits.size(2), nw = base_bits.size(3);
  Tensor out = at::empty({b, heads, n, nw}, base_bits.options());
  ok(sam_mask_bits_spatial((const uint32_t*)base_bits.data_ptr(), (const int8_t*)adj.data_ptr(), (int)b, (int)n, (int)nw, (int)n_txt, (int)adj.size(1), (int)adj.size(3),
                           (int)heads, (unsigned)quadrant_bits, (uint32_t*)out.data_ptr(), cur_stream()), "sam_mask_bits_spatial");
  return out;
}
Tensor pack_relations_bhnn(const Tensor& rel, const optional<Tensor>& base_bits) {       // north-star layout int8 [B,H,N,N]
  need(rel, at::kChar, "rel");
  TORCH_CHECK(rel.dim() == 4 && rel.size(2) == rel.size(3) && rel.is_contiguous(), "rel must be a contiguous int8 [B,H,N,N] tensor");
  const int64_t b = rel.size(0), h = rel.size(1), n = rel.size(2), nw = words_per_row(n);
  Tensor out = at::empty({b, h, n, nw}, rel.options().dtype(at::kInt));
  ok(sam_mask_bits_from_int8_bhnn((const int8_t*)rel.data_ptr(), (const uint32_t*)p(base_bits), (int)b, (int)h, (int)n, (int)nw, (uint32_t*)out.data_ptr(), cur_stream()),
     "sam_mask_bits_from_int8_bhnn");
  return out;
}

// ---------------------------------------------------------------------------------------------------------------- pointer net / loss / optimizer
Tensor ptr_scores_fwd(const Tensor& q, const Tensor& k, const Tensor& ocr_mask, double scale) {      // sa_m4c.py:891-893
  need(q, at::kBFloat16, "q"); need(k, at::kBFloat16, "k"); need(ocr_mask, at::kByte, "ocr_mask");
  TORCH_CHECK(q.dim() == 3 && k.dim() == 3 && q.is_contiguous() && k.is_contiguous() && ocr_mask.is_contiguous(), "ptr_scores: contiguous q [B,S,D], k [B,No,D], mask [B,No]");
  const int64_t b = q.size(0), s = q.size(1), d = q.size(2), no = k.size(1);
  Tensor out = at::empty({b, s, no}, q.options().dtype(at::kFloat));
  ok(sam_ptr_scores_fwd(q.data_ptr(), k.data_ptr(), (const uint8_t*)ocr_mask.data_ptr(), (int)b, (int)s, (int)no, (int)d, (float)scale, (float*)out.data_ptr(), out.stride(0),
                        out.stride(1), cur_stream()), "sam_ptr_scores_fwd");
  return out;
}
std::tuple<Tensor, Tensor> ptr_scores_bwd(const Tensor& ds, const Tensor& q, const Tensor& k, double scale) {
  need(ds, at::kFloat, "dscores"); need(q, at::kBFloat16, "q"); need(k, at::kBFloat16, "k");
  TORCH_CHECK(ds.dim() == 3 && ds.stride(2) == 1 && q.is_contiguous() && k.is_contiguous(), "ptr_scores_bwd: dscores [B,S,No] with unit last stride");
  const int64_t b = q.size(0), s = q.size(1), d = q.size(2), no = k.size(1);
  Tensor dq = at::empty_like(q), dk = at::empty_like(k);
  ok(sam_ptr_scores_bwd((const float*)ds.data_ptr(), ds.stride(0), ds.stride(1), q.data_ptr(), k.data_ptr(), (int)b, (int)s, (int)no, (int)d, (float)scale, dq.data_ptr(),
                        dk.data_ptr(), cur_stream()), "sam_ptr_scores_bwd");
  return {dq, dk};
}
// M4CDecodingBCEWithMaskLoss (task_utils.py:19-30): value + analytic gradient -> (loss f32 [1], d_fixed bf16 [R,V], d_ocr f32 [R,No])
std::tuple<Tensor, Tensor, Tensor> bce_loss(const Tensor& fixed, const Tensor& ocr, const Tensor& targets, const Tensor& loss_mask, double grad_scale,
                                            const optional<Tensor>& global_count) {
  need(fixed, at::kFloat, "fixed_scores"); need(ocr, at::kFloat, "ocr_scores"); need(targets, at::kFloat, "targets"); need(loss_mask, at::kFloat, "loss_mask");
  TORCH_CHECK(fixed.dim() == 2 && ocr.dim() == 2 && targets.dim() == 2 && fixed.stride(1) == 1 && ocr.stride(1) == 1 && targets.stride(1) == 1 && loss_mask.is_contiguous(),
              "bce_loss: 2-D score / target blocks with unit last stride");
  const int64_t r = fixed.size(0), v = fixed.size(1), no = ocr.size(1);
  Tensor loss = at::empty({1}, fixed.options()), d_fixed = at::empty({r, v}, fixed.options().dtype(at::kBFloat16)), d_ocr = at::empty({r, no}, fixed.options());
  ok(sam_bce_loss((const float*)fixed.data_ptr(), fixed.stride(0), (const float*)ocr.data_ptr(), ocr.stride(0), (const float*)targets.data_ptr(), targets.stride(0),
                  (const float*)loss_mask.data_ptr(), (int)r, (int)v, (int)no, (float)grad_scale, (const float*)p(global_count), (float*)loss.data_ptr(), d_fixed.data_ptr(),
                  d_fixed.stride(0), (float*)d_ocr.data_ptr(), d_ocr.stride(0), cur_stream()), "sam_bce_loss");
  return {loss, d_fixed, d_ocr};
}
Tensor& workspace(const char* tag, int64_t bytes, const Tensor& like) {      // per (tag, device, stream) scratch that only grows
  static std::mutex mu;
  static std::map<std::tuple<std::string, int, void*>, Tensor> cache;
  std::lock_guard<std::mutex> lock(mu);
  Tensor& ws = cache[{std::string(tag), (int)like.get_device(), cur_stream()}];
  if (!ws.defined() || ws.numel() * 4 < bytes) ws = at::empty({(bytes + 3) / 4}, like.options().dtype(at::kFloat));
  return ws;
}
// row-sparse region from its schema form: region = [lo, hi, row_len] (empty: none), touched = uint8 [rows]
const sam_sparse_rows* sparse_of(sam_sparse_rows& s, at::IntArrayRef region, const optional<Tensor>& touched) {
  if (region.size() != 3 || !touched.has_value() || !touched->defined()) return nullptr;
  need(*touched, at::kByte, "touched");
  s.lo = region[0]; s.hi = region[1]; s.row_len = (int32_t)region[2]; s.touched = (const uint8_t*)touched->data_ptr();
  TORCH_CHECK(touched->numel() * region[2] >= region[1] - region[0], "row-sparse region: fewer flags than rows");
  return &s;
}
void sumsq(const Tensor& g, Tensor out, at::IntArrayRef region, const optional<Tensor>& touched) {      // clip_grad_norm_'s norm, train.py:139
  need(g, at::kFloat, "g"); need(out, at::kFloat, "out");
  Tensor& ws = workspace("sumsq", sam_sumsq_ws_bytes(), g);
  sam_sparse_rows s;
  ok(sam_sumsq_f32((const float*)g.data_ptr(), g.numel(), sparse_of(s, region, touched), (float*)out.data_ptr(), (float*)ws.data_ptr(), cur_stream()), "sam_sumsq_f32");
}
// clip + Adam + bf16 shadow refresh over the flat buffers (train.py:139-142, task_utils.py:33-57).  dev_sched given: schedule read from device memory
// (captured steps, see step_advance); else seg_lr / step by value.
void adam_step(Tensor p_, Tensor g, Tensor m, Tensor v, const optional<Tensor>& p_bf16, at::IntArrayRef seg_end, at::ArrayRef<double> seg_lr, int64_t step,
               double beta1, double beta2, double eps, const optional<Tensor>& gnorm_sq, double max_norm, const optional<Tensor>& dev_sched, at::IntArrayRef region,
               const optional<Tensor>& touched) {
  need(p_, at::kFloat, "p"); need(g, at::kFloat, "g"); need(m, at::kFloat, "exp_avg"); need(v, at::kFloat, "exp_avg_sq");
  TORCH_CHECK(seg_end.size() >= 1 && seg_end.size() <= 8, "adam_step: 1..8 segments");
  int64_t ends[8]; float lrs[8] = {};
  for (size_t s = 0; s < seg_end.size(); ++s) { ends[s] = seg_end[s]; lrs[s] = s < seg_lr.size() ? (float)seg_lr[s] : 0.f; }
  sam_sparse_rows s;
  const sam_sparse_rows* sp = sparse_of(s, region, touched);
  if (dev_sched.has_value() && dev_sched->defined())
    ok(sam_adam_step_dev((float*)p_.data_ptr(), (float*)g.data_ptr(), (float*)m.data_ptr(), (float*)v.data_ptr(), p(p_bf16), p_.numel(), ends, (int)seg_end.size(),
                         (float)beta1, (float)beta2, (float)eps, (const float*)dev_sched->data_ptr(), (const float*)p(gnorm_sq), (float)max_norm, sp, cur_stream()), "sam_adam_step_dev");
  else
    ok(sam_adam_step((float*)p_.data_ptr(), (float*)g.data_ptr(), (float*)m.data_ptr(), (float*)v.data_ptr(), p(p_bf16), p_.numel(), ends, lrs, (int)seg_end.size(),
                     (float)beta1, (float)beta2, (float)eps, step, (const float*)p(gnorm_sq), (float)max_norm, sp, cur_stream()), "sam_adam_step");
}
// head node of a captured training step (include/sam_hip.h: sam_step_advance)
void step_advance(const optional<Tensor>& rng_state, int64_t offset_stride, Tensor step_counter, at::ArrayRef<double> base_lr, int64_t warmup_iters, double warmup_factor,
                  at::IntArrayRef decay_iters, double lr_decay, double beta1, double beta2, Tensor dev_sched) {
  need(step_counter, at::kLong, "step_counter"); need(dev_sched, at::kFloat, "dev_sched");
  TORCH_CHECK(base_lr.size() >= 1 && base_lr.size() <= 8 && decay_iters.size() <= 4 && (int64_t)dev_sched.numel() >= (int64_t)base_lr.size() + 2, "step_advance: bad schedule sizes");
  sam_lr_schedule sc = {};
  sc.nseg = (int32_t)base_lr.size();
  for (size_t s = 0; s < base_lr.size(); ++s) sc.base_lr[s] = base_lr[s];
  sc.warmup_iters = warmup_iters; sc.warmup_factor = warmup_factor; sc.n_decay = (int32_t)decay_iters.size();
  for (size_t q = 0; q < decay_iters.size(); ++q) sc.decay_iters[q] = decay_iters[q];
  sc.lr_decay = lr_decay; sc.beta1 = beta1; sc.beta2 = beta2;
  ok(sam_step_advance((unsigned long long*)p(rng_state), (uint64_t)offset_stride, (int64_t*)step_counter.data_ptr(), &sc, (float*)dev_sched.data_ptr(), cur_stream()),
     "sam_step_advance");
}

// answer targets from the collated answer tables (include/sam_hip.h: sam_answer_sample).  targets fp32 [B, L, W] with unit column stride and any row stride
// ld >= W (a view into [B, L, ld]); key: the 64-bit draw key as a signed int; step_dev: int64 [1] device step counter (or None: step by value)
// (targets == nullptr: sam_answer_sample without the dense tensor, `width` columns; see answer_sample_notargets)
void answer_sample_impl(const Tensor& meta, const Tensor& seq_len, const Tensor& seq_grp, const Tensor& step0_idx, const Tensor& step0_val, const Tensor& grp_idx,
                        const Tensor& grp_off, const Tensor& grp_extra, int64_t bos, int64_t key, const optional<Tensor>& step_dev, int64_t step,
                        const optional<Tensor>& force_choice, const Tensor* targets_or_null, int64_t width, Tensor prev_inds, Tensor loss_mask, Tensor acc_mask,
                        Tensor choice) {
  const bool dense = targets_or_null != nullptr;
  const Tensor targets = dense ? *targets_or_null : Tensor();
  need(meta, at::kInt, "meta"); need(seq_len, at::kInt, "seq_len"); need(seq_grp, at::kShort, "seq_grp"); need(step0_idx, at::kInt, "step0_idx");
  need(step0_val, at::kFloat, "step0_val"); need(grp_idx, at::kInt, "grp_idx"); need(grp_off, at::kInt, "grp_off"); need(grp_extra, at::kInt, "grp_extra");
  if (dense) need(targets, at::kFloat, "targets");
  need(prev_inds, at::kLong, "prev_inds"); need(loss_mask, at::kFloat, "loss_mask"); need(acc_mask, at::kFloat, "acc_mask");
  need(choice, at::kInt, "choice");
  for (const Tensor* t : std::initializer_list<const Tensor*>{&meta, &seq_len, &seq_grp, &step0_idx, &step0_val, &grp_idx, &grp_off, &grp_extra, &prev_inds, &loss_mask, &acc_mask, &choice})
    TORCH_CHECK(t->is_contiguous(), "answer_sample: table and per-sample outputs must be contiguous");
  TORCH_CHECK(seq_grp.dim() == 3 && meta.dim() == 2 && meta.size(1) == 4, "answer_sample: meta [B, 4], seq_grp [B, S, L]");
  const int64_t B = seq_grp.size(0), S = seq_grp.size(1), L = seq_grp.size(2), G = grp_idx.size(-1), E = grp_extra.size(-1);
  TORCH_CHECK(meta.size(0) == B && seq_len.numel() == B * S && step0_idx.numel() == B * S && step0_val.numel() == B * S && grp_idx.numel() == B * G &&
              grp_off.numel() == B * (G + 1) && grp_extra.numel() == B * E, "answer_sample: table tensors of inconsistent sizes");
  TORCH_CHECK(!dense || (targets.dim() == 3 && targets.size(0) == B && targets.size(1) == L && targets.stride(2) == 1 && targets.stride(0) == L * targets.stride(1)),
              "answer_sample: targets must be fp32 [B, L, W] with unit column stride over a [B, L, ld] buffer");
  TORCH_CHECK(prev_inds.numel() == B * L && loss_mask.numel() == B * L && acc_mask.numel() == B * L && choice.numel() == B, "answer_sample: output sizes");
  const int32_t* force = nullptr;
  if (force_choice.has_value() && force_choice->defined()) {
    need(*force_choice, at::kInt, "force_choice");
    TORCH_CHECK(force_choice->is_contiguous() && force_choice->numel() == B, "answer_sample: force_choice int32 [B]");
    force = (const int32_t*)force_choice->data_ptr();
  }
  const int64_t* sd = nullptr;
  if (step_dev.has_value() && step_dev->defined()) {
    need(*step_dev, at::kLong, "step_dev");
    sd = (const int64_t*)step_dev->data_ptr();
  }
  ok(sam_answer_sample((const int32_t*)meta.data_ptr(), (const int32_t*)seq_len.data_ptr(), (const int16_t*)seq_grp.data_ptr(), (const int32_t*)step0_idx.data_ptr(),
                       (const float*)step0_val.data_ptr(), (const int32_t*)grp_idx.data_ptr(), (const int32_t*)grp_off.data_ptr(), (const int32_t*)grp_extra.data_ptr(),
                       (int)B, (int)S, (int)L, (int)G, (int)E, (int)(dense ? targets.size(2) : width), (int)bos, (uint64_t)key, sd, step, force,
                       dense ? (float*)targets.data_ptr() : nullptr, dense ? targets.stride(1) : 0, (int64_t*)prev_inds.data_ptr(), (float*)loss_mask.data_ptr(),
                       (float*)acc_mask.data_ptr(), (int32_t*)choice.data_ptr(), cur_stream()),
     "sam_answer_sample");
}
void answer_sample(const Tensor& meta, const Tensor& seq_len, const Tensor& seq_grp, const Tensor& step0_idx, const Tensor& step0_val, const Tensor& grp_idx,
                   const Tensor& grp_off, const Tensor& grp_extra, int64_t bos, int64_t key, const optional<Tensor>& step_dev, int64_t step,
                   const optional<Tensor>& force_choice, Tensor targets, Tensor prev_inds, Tensor loss_mask, Tensor acc_mask, Tensor choice) {
  answer_sample_impl(meta, seq_len, seq_grp, step0_idx, step0_val, grp_idx, grp_off, grp_extra, bos, key, step_dev, step, force_choice, &targets, 0, prev_inds,
                     loss_mask, acc_mask, choice);
}
// the same draw without the dense targets (sam_answer_sample with targets = NULL): train_prev_inds, both masks and the choice only; width = V + No
void answer_sample_notargets(const Tensor& meta, const Tensor& seq_len, const Tensor& seq_grp, const Tensor& step0_idx, const Tensor& step0_val,
                             const Tensor& grp_idx, const Tensor& grp_off, const Tensor& grp_extra, int64_t width, int64_t bos, int64_t key,
                             const optional<Tensor>& step_dev, int64_t step, const optional<Tensor>& force_choice, Tensor prev_inds, Tensor loss_mask,
                             Tensor acc_mask, Tensor choice) {
  answer_sample_impl(meta, seq_len, seq_grp, step0_idx, step0_val, grp_idx, grp_off, grp_extra, bos, key, step_dev, step, force_choice, nullptr, width, prev_inds,
                     loss_mask, acc_mask, choice);
}

// M4CDecodingBCEWithMaskLoss + the metric's argmax straight from the answer tables (include/sam_hip.h: sam_bce_loss_table).  table: the eight collated
// tensors in ops.ANSWER_TABLE_KEYS order; choice int32 [B] as the sampler wrote it.  -> (loss f32 [1], d_fixed bf16 [R,V], d_ocr f32 [R,No]); without
// want_grads both gradients come back empty ([0, V] / [0, No]) and nothing is stored.  pred int64 [R] (optional) receives the row argmax in place.
std::tuple<Tensor, Tensor, Tensor> bce_loss_table(const Tensor& fixed, const Tensor& ocr, at::TensorList table, const Tensor& choice, const Tensor& loss_mask,
                                                  double grad_scale, const optional<Tensor>& global_count, bool want_grads, const optional<Tensor>& pred) {
  need(fixed, at::kFloat, "fixed_scores"); need(ocr, at::kFloat, "ocr_scores"); need(loss_mask, at::kFloat, "loss_mask"); need(choice, at::kInt, "choice");
  TORCH_CHECK(fixed.dim() == 2 && ocr.dim() == 2 && fixed.stride(1) == 1 && ocr.stride(1) == 1 && ocr.size(0) == fixed.size(0) && loss_mask.is_contiguous() &&
              choice.is_contiguous(), "bce_loss_table: 2-D score blocks with unit last stride, contiguous loss_mask and choice");
  TORCH_CHECK(table.size() == 8, "bce_loss_table: the answer table is eight tensors (meta, seq_len, seq_grp, step0_idx, step0_val, grp_idx, grp_off, grp_extra)");
  const Tensor &meta = table[0], &seq_len = table[1], &seq_grp = table[2], &step0_idx = table[3], &step0_val = table[4], &grp_idx = table[5], &grp_off = table[6],
               &grp_extra = table[7];
  need(meta, at::kInt, "meta"); need(seq_len, at::kInt, "seq_len"); need(seq_grp, at::kShort, "seq_grp"); need(step0_idx, at::kInt, "step0_idx");
  need(step0_val, at::kFloat, "step0_val"); need(grp_idx, at::kInt, "grp_idx"); need(grp_off, at::kInt, "grp_off"); need(grp_extra, at::kInt, "grp_extra");
  for (const Tensor& t : table) TORCH_CHECK(t.is_contiguous(), "bce_loss_table: table tensors must be contiguous");
  TORCH_CHECK(seq_grp.dim() == 3 && meta.dim() == 2 && meta.size(1) == 4, "bce_loss_table: meta [B, 4], seq_grp [B, S, L]");
  const int64_t B = seq_grp.size(0), S = seq_grp.size(1), L = seq_grp.size(2), G = grp_idx.size(-1), E = grp_extra.size(-1);
  TORCH_CHECK(meta.size(0) == B && seq_len.numel() == B * S && step0_idx.numel() == B * S && step0_val.numel() == B * S && grp_idx.numel() == B * G &&
              grp_off.numel() == B * (G + 1) && grp_extra.numel() == B * E, "bce_loss_table: table tensors of inconsistent sizes");
  const int64_t r = fixed.size(0), v = fixed.size(1), no = ocr.size(1);
  TORCH_CHECK(r == B * L && loss_mask.numel() == r && choice.numel() == B, "bce_loss_table: ", r, " score rows for a table of ", B, " x ", L, " decoding steps");
  int64_t* pr = nullptr;
  if (pred.has_value() && pred->defined()) {
    need(*pred, at::kLong, "pred");
    TORCH_CHECK(pred->is_contiguous() && pred->numel() == r, "bce_loss_table: pred int64 [R]");
    pr = (int64_t*)pred->data_ptr();
  }
  const int64_t rg = want_grads ? r : 0;
  Tensor loss = at::empty({1}, fixed.options()), d_fixed = at::empty({rg, v}, fixed.options().dtype(at::kBFloat16)), d_ocr = at::empty({rg, no}, fixed.options());
  ok(sam_bce_loss_table((const float*)fixed.data_ptr(), fixed.stride(0), (const float*)ocr.data_ptr(), ocr.stride(0), (const int32_t*)meta.data_ptr(),
                        (const int32_t*)seq_len.data_ptr(), (const int16_t*)seq_grp.data_ptr(), (const int32_t*)step0_idx.data_ptr(), (const float*)step0_val.data_ptr(),
                        (const int32_t*)grp_idx.data_ptr(), (const int32_t*)grp_off.data_ptr(), (const int32_t*)grp_extra.data_ptr(), (int)B, (int)S, (int)L, (int)G, (int)E,
                        (const int32_t*)choice.data_ptr(), (const float*)loss_mask.data_ptr(), (int)r, (int)v, (int)no, (float)grad_scale, (const float*)p(global_count),
                        (float*)loss.data_ptr(), want_grads ? d_fixed.data_ptr() : nullptr, want_grads ? d_fixed.stride(0) : 0,
                        want_grads ? (float*)d_ocr.data_ptr() : nullptr, want_grads ? d_ocr.stride(0) : 0, pr, cur_stream()), "sam_bce_loss_table");
  return {loss, d_fixed, d_ocr};
}

// VQA soft accuracy, ST-VQA accuracy and ANLS of a batch of predictions (include/sam_hip.h: sam_score_answers).  pred int64 [B, L]; table: the eight collated
// score-table tensors in ops.SCORE_TABLE_KEYS order; vocab_cp int32 [V, Lw] / vocab_len int32 [V].  scores fp32 [B, 3] and flags int32 [B] are written in
// place; totals float64 [4] (optional) is added to.
void score_answers(const Tensor& pred, at::TensorList table, const Tensor& vocab_cp, const Tensor& vocab_len, int64_t eos, Tensor scores, Tensor flags,
                   const optional<Tensor>& totals) {
  need(pred, at::kLong, "pred"); need(vocab_cp, at::kInt, "vocab_cp"); need(vocab_len, at::kInt, "vocab_len"); need(scores, at::kFloat, "scores");
  need(flags, at::kInt, "flags");
  TORCH_CHECK(table.size() == 8, "score_answers: the score table is eight tensors (meta, gt_norm, gt_norm_len, gt_score, gt_raw, gt_raw_len, ocr, ocr_len)");
  const Tensor &meta = table[0], &gt_norm = table[1], &gt_norm_len = table[2], &gt_score = table[3], &gt_raw = table[4], &gt_raw_len = table[5], &ocr = table[6],
               &ocr_len = table[7];
  need(meta, at::kInt, "meta"); need(gt_norm, at::kInt, "gt_norm"); need(gt_norm_len, at::kInt, "gt_norm_len"); need(gt_score, at::kFloat, "gt_score");
  need(gt_raw, at::kInt, "gt_raw"); need(gt_raw_len, at::kInt, "gt_raw_len"); need(ocr, at::kInt, "ocr"); need(ocr_len, at::kInt, "ocr_len");
  for (const Tensor& t : table) TORCH_CHECK(t.is_contiguous(), "score_answers: table tensors must be contiguous");
  TORCH_CHECK(pred.dim() == 2 && pred.is_contiguous() && vocab_cp.dim() == 2 && vocab_cp.is_contiguous() && vocab_len.is_contiguous() && scores.is_contiguous() &&
              flags.is_contiguous(), "score_answers: contiguous pred [B, L], vocab_cp [V, Lw], vocab_len [V], scores [B, 3], flags [B]");
  TORCH_CHECK(gt_norm.dim() == 3 && ocr.dim() == 3 && meta.dim() == 2 && meta.size(1) == 4, "score_answers: meta [B, 4], gt_norm [B, A, Lg], ocr [B, No, Lw]");
  const int64_t B = pred.size(0), L = pred.size(1), A = gt_norm.size(1), Lg = gt_norm.size(2), No = ocr.size(1), Lw = ocr.size(2), V = vocab_cp.size(0);
  TORCH_CHECK(meta.size(0) == B && gt_norm.size(0) == B && gt_norm_len.numel() == B * A && gt_score.numel() == B * A && gt_raw.numel() == B * A * Lg &&
              gt_raw_len.numel() == B * A && ocr.size(0) == B && ocr_len.numel() == B * No && vocab_cp.size(1) == Lw && vocab_len.numel() == V &&
              scores.numel() == B * 3 && flags.numel() == B, "score_answers: tensors of inconsistent sizes");
  double* tot = nullptr;
  if (totals.has_value() && totals->defined()) {
    need(*totals, at::kDouble, "totals");
    TORCH_CHECK(totals->is_contiguous() && totals->numel() == 4, "score_answers: totals float64 [4]");
    tot = (double*)totals->data_ptr();
  }
  ok(sam_score_answers((const int64_t*)pred.data_ptr(), (const int32_t*)meta.data_ptr(), (const int32_t*)gt_norm.data_ptr(), (const int32_t*)gt_norm_len.data_ptr(),
                       (const float*)gt_score.data_ptr(), (const int32_t*)gt_raw.data_ptr(), (const int32_t*)gt_raw_len.data_ptr(), (const int32_t*)ocr.data_ptr(),
                       (const int32_t*)ocr_len.data_ptr(), (const int32_t*)vocab_cp.data_ptr(), (const int32_t*)vocab_len.data_ptr(), (int)B, (int)L, (int)A, (int)Lg,
                       (int)No, (int)Lw, (int)V, (int)eos, (float*)scores.data_ptr(), (int32_t*)flags.data_ptr(), tot, cur_stream()), "sam_score_answers");
}

// ---------------------------------------------------------------------------------------------------------------- ragged region features (csrc/ragged.hip)
// counts int32 [B]; srcs[k] [cap_rows, width_k] fp32 / fp16, dsts[k] [B * n_max, ld_k] bf16 / fp32 (written in place); mask int64 [B, n_max] (optional).
void ragged_expand(const Tensor& counts, int64_t n_max, at::TensorList srcs, at::TensorList dsts, at::IntArrayRef col0, at::IntArrayRef normalize,
                   at::IntArrayRef zero_upto, const optional<Tensor>& mask, double eps) {
  need(counts, at::kInt, "counts");
  TORCH_CHECK(counts.is_contiguous(), "ragged_expand: counts must be contiguous");
  const size_t n = srcs.size();
  TORCH_CHECK(n <= SAM_RAGGED_MAX_PARTS && dsts.size() == n && col0.size() == n && normalize.size() == n && zero_upto.size() == n,
              "ragged_expand: at most ", SAM_RAGGED_MAX_PARTS, " parts, one src / dst / col0 / normalize / zero_upto each");
  const int64_t B = counts.numel();
  int64_t cap = n ? srcs[0].size(0) : 1;
  sam_ragged_part parts[SAM_RAGGED_MAX_PARTS] = {};
  for (size_t k = 0; k < n; ++k) {
    const Tensor &s = srcs[k], &d = dsts[k];
    TORCH_CHECK(s.is_cuda() && d.is_cuda() && s.dim() == 2 && d.dim() == 2 && s.stride(1) == 1 && d.stride(1) == 1, "ragged_expand: part ", k, ": row-major 2-D GPU tensors");
    TORCH_CHECK(s.scalar_type() == at::kFloat || s.scalar_type() == at::kHalf, "ragged_expand: part ", k, ": src must be fp32 or fp16");
    TORCH_CHECK(d.scalar_type() == at::kBFloat16 || d.scalar_type() == at::kFloat, "ragged_expand: part ", k, ": dst must be bf16 or fp32");
    TORCH_CHECK(s.size(0) == cap && d.size(0) == B * n_max, "ragged_expand: part ", k, ": src rows ", s.size(0), " (others ", cap, "), dst rows ", d.size(0),
                " (B * n_max = ", B * n_max, ")");
    parts[k].src = s.data_ptr(); parts[k].ld_src = s.stride(0); parts[k].src_f16 = s.scalar_type() == at::kHalf; parts[k].width = (int32_t)s.size(1);
    parts[k].dst = d.data_ptr(); parts[k].ld_dst = d.stride(0); parts[k].dst_f32 = d.scalar_type() == at::kFloat; parts[k].col0 = (int32_t)col0[k];
    parts[k].normalize = normalize[k] != 0; parts[k].zero_upto = (int32_t)zero_upto[k];
  }
  int64_t* m = nullptr;
  if (mask.has_value() && mask->defined()) {
    need(*mask, at::kLong, "mask");
    TORCH_CHECK(mask->is_contiguous() && mask->numel() == B * n_max, "ragged_expand: mask int64 [B, n_max]");
    m = (int64_t*)mask->data_ptr();
  }
  ok(sam_ragged_expand((const int32_t*)counts.data_ptr(), (int)B, (int)n_max, (int)cap, parts, (int)n, (float)eps, m, cur_stream()), "sam_ragged_expand");
}

// the slot text phoc_from_text and fasttext_from_text read: text int32 [B, n_max, Lw] (or [B * n_max, Lw], row stride >= Lw), text_len int32 [B * n_max],
// counts int32 [B] or none -> the flattened text, its row stride, the counts (null when none), rows = B * n_max and Lw
struct SlotText { const int32_t* text; int64_t ld; const int32_t* counts; int64_t rows, lw; };
static SlotText slot_text(const char* who, const Tensor& text, const Tensor& text_len, const optional<Tensor>& counts, int64_t batch, int64_t n_max) {
  need(text, at::kInt, "text"); need(text_len, at::kInt, "text_len");
  TORCH_CHECK(text.dim() >= 2 && text.stride(-1) == 1 && text_len.is_contiguous(), who, ": text must be row-major [..., Lw], text_len contiguous");
  const int64_t rows = batch * n_max, lw = text.size(-1);
  TORCH_CHECK(text.numel() == rows * lw && text_len.numel() == rows, who, ": text must hold B * n_max = ", rows, " rows and text_len as many lengths");
  const Tensor t2 = text.dim() == 2 ? text : text.flatten(0, -2);          // (a view: the check below refuses a copy)
  TORCH_CHECK(t2.data_ptr() == text.data_ptr() && (rows == 1 || t2.stride(0) >= lw), who, ": the rows of text must share one stride");
  const int32_t* c = nullptr;
  if (counts.has_value() && counts->defined()) {
    need(*counts, at::kInt, "counts");
    TORCH_CHECK(counts->is_contiguous() && counts->numel() == batch, who, ": counts int32 [B]");
    c = (const int32_t*)counts->data_ptr();
  }
  return {(const int32_t*)t2.data_ptr(), rows == 1 ? lw : t2.stride(0), c, rows, lw};
}

// the OCR tokens' PHOC rows from their text (include/sam_hip_text.h): the slot text above; dst 2-D [B * n_max, ld] fp32 / bf16
void phoc_from_text(const Tensor& text, const Tensor& text_len, const optional<Tensor>& counts, int64_t batch, int64_t n_max, Tensor dst, int64_t col0,
                    bool normalize, double eps) {
  const SlotText t = slot_text("phoc_from_text", text, text_len, counts, batch, n_max);
  TORCH_CHECK(dst.is_cuda() && dst.dim() == 2 && dst.stride(1) == 1 && dst.size(0) == t.rows, "phoc_from_text: dst must be a row-major 2-D GPU tensor of B * n_max rows");
  TORCH_CHECK(dst.scalar_type() == at::kBFloat16 || dst.scalar_type() == at::kFloat, "phoc_from_text: dst must be bf16 or fp32");
  TORCH_CHECK(col0 >= 0 && col0 + 604 <= dst.size(1), "phoc_from_text: columns [", col0, ", ", col0 + 604, ") exceed dst's ", dst.size(1));
  ok(sam_phoc_from_text(t.text, t.ld, (const int32_t*)text_len.data_ptr(), t.counts, (int)batch, (int)n_max, (int)t.lw, dst.data_ptr(), dst.stride(0), (int)col0,
                        dst.scalar_type() == at::kFloat, normalize, (float)eps, cur_stream()), "sam_phoc_from_text");
}

// the answer tables of a batch from text (include/sam_hip_answers.h): answer_text int32 [B, A, La], answer_len int32 [B, A], ocr_text int32 [B, No, Lw],
// ocr_len int32 [B, No], the vocabulary index (vocab_cp int32 [V, Lv], vocab_len int32 [V], slots int32 [T]); out: the eight table tensors in
// answers.TABLE_KEYS order at their capacities (seq_grp int16 [B, S, L], grp_idx [B, G], grp_extra [B, E]) and status int32 [B]
void answer_table_from_text(const Tensor& answer_text, const Tensor& answer_len, const Tensor& ocr_text, const Tensor& ocr_len, const Tensor& vocab_cp,
                            const Tensor& vocab_len, const Tensor& slots, int64_t unk, int64_t eos, int64_t max_match_num, at::TensorList out) {
  const Tensor* in[] = {&answer_text, &answer_len, &ocr_text, &ocr_len, &vocab_cp, &vocab_len, &slots};
  const char* in_names[] = {"answer_text", "answer_text_len", "ocr_text", "ocr_text_len", "vocab cp", "vocab len", "vocab slots"};
  for (int i = 0; i < 7; ++i) {
    need(*in[i], at::kInt, in_names[i]);
    TORCH_CHECK(in[i]->is_contiguous(), "answer_table_from_text: ", in_names[i], " must be contiguous");
  }
  TORCH_CHECK(answer_text.dim() == 3 && ocr_text.dim() == 3 && vocab_cp.dim() == 2, "answer_table_from_text: answer_text [B, A, La], ocr_text [B, No, Lw], vocab cp [V, Lv]");
  const int64_t B = answer_text.size(0), A = answer_text.size(1), La = answer_text.size(2), No = ocr_text.size(1), Lw = ocr_text.size(2), V = vocab_cp.size(0),
                Lv = vocab_cp.size(1), T = slots.numel();
  TORCH_CHECK(ocr_text.size(0) == B && answer_len.numel() == B * A && ocr_len.numel() == B * No && vocab_len.numel() == V,
              "answer_table_from_text: answer_text_len [B, A], ocr_text [B, No, Lw] with ocr_text_len [B, No], vocab len [V]");
  TORCH_CHECK(out.size() == 9, "answer_table_from_text: out holds the eight table tensors and status");
  const at::ScalarType dt[] = {at::kInt, at::kInt, at::kShort, at::kInt, at::kFloat, at::kInt, at::kInt, at::kInt, at::kInt};
  const char* names[] = {"meta", "seq_len", "seq_grp", "step0_idx", "step0_val", "grp_idx", "grp_off", "grp_extra", "status"};
  for (int i = 0; i < 9; ++i) {
    need(out[i], dt[i], names[i]);
    TORCH_CHECK(out[i].is_contiguous() && out[i].dim() >= 1 && out[i].size(0) == B, "answer_table_from_text: ", names[i], " must be contiguous with B = ", B, " rows");
  }
  TORCH_CHECK(out[2].dim() == 3 && out[5].dim() == 2 && out[7].dim() == 2, "answer_table_from_text: seq_grp [B, S, L], grp_idx [B, G], grp_extra [B, E]");
  const int64_t S = out[2].size(1), L = out[2].size(2), G = out[5].size(1), E = out[7].size(1);
  TORCH_CHECK(out[0].numel() == B * 4 && out[1].numel() == B * S && out[3].numel() == B * S && out[4].numel() == B * S && out[6].numel() == B * (G + 1) &&
              out[8].numel() == B, "answer_table_from_text: table tensors of inconsistent sizes");
  ok(sam_answer_table_from_text((const int32_t*)answer_text.data_ptr(), La, (const int32_t*)answer_len.data_ptr(), (const int32_t*)ocr_text.data_ptr(), Lw,
                                (const int32_t*)ocr_len.data_ptr(), (const int32_t*)vocab_cp.data_ptr(), Lv, (const int32_t*)vocab_len.data_ptr(),
                                (const int32_t*)slots.data_ptr(), (int)B, (int)A, (int)La, (int)No, (int)Lw, (int)V, (int)Lv, (int)T, (int)unk, (int)eos, (int)S, (int)L,
                                (int)G, (int)E, (int)max_match_num, (int32_t*)out[0].data_ptr(), (int32_t*)out[1].data_ptr(), (int16_t*)out[2].data_ptr(),
                                (int32_t*)out[3].data_ptr(), (float*)out[4].data_ptr(), (int32_t*)out[5].data_ptr(), (int32_t*)out[6].data_ptr(),
                                (int32_t*)out[7].data_ptr(), (int32_t*)out[8].data_ptr(), cur_stream()), "sam_answer_table_from_text");
}

// the metrics' score tables of a batch from text (include/sam_hip_metrics.h): answer_text int32 [B, A, La], answer_len int32 [B, A], ocr_text int32
// [B, No, Lw], ocr_len int32 [B, No], ocr_count int32 [B]; out: the eight table tensors in metrics.SCORE_TABLE_KEYS order at the capacities (A, Lw, Lg)
// (gt_norm / gt_raw int32 [B, A, Lg], ocr int32 [B, max(No, 1), Lw]) and status int32 [B]
void score_table_from_text(const Tensor& answer_text, const Tensor& answer_len, const Tensor& ocr_text, const Tensor& ocr_len, const Tensor& ocr_count,
                           at::TensorList out) {
  const Tensor* in[] = {&answer_text, &answer_len, &ocr_text, &ocr_len, &ocr_count};
  const char* in_names[] = {"answer_text", "answer_text_len", "ocr_text", "ocr_text_len", "ocr_count"};
  for (int i = 0; i < 5; ++i) {
    need(*in[i], at::kInt, in_names[i]);
    TORCH_CHECK(in[i]->is_contiguous(), "score_table_from_text: ", in_names[i], " must be contiguous");
  }
  TORCH_CHECK(answer_text.dim() == 3 && ocr_text.dim() == 3, "score_table_from_text: answer_text [B, A, La], ocr_text [B, No, Lw]");
  const int64_t B = answer_text.size(0), A = answer_text.size(1), La = answer_text.size(2), No = ocr_text.size(1), Lw = ocr_text.size(2);
  TORCH_CHECK(ocr_text.size(0) == B && answer_len.numel() == B * A && ocr_len.numel() == B * No && ocr_count.numel() == B,
              "score_table_from_text: answer_text_len [B, A], ocr_text [B, No, Lw] with ocr_text_len [B, No], ocr_count [B]");
  TORCH_CHECK(out.size() == 9, "score_table_from_text: out holds the eight table tensors and status");
  const char* names[] = {"meta", "gt_norm", "gt_norm_len", "gt_score", "gt_raw", "gt_raw_len", "ocr", "ocr_len", "status"};
  for (int i = 0; i < 9; ++i) {
    need(out[i], i == 3 ? at::kFloat : at::kInt, names[i]);
    TORCH_CHECK(out[i].is_contiguous() && out[i].dim() >= 1 && out[i].size(0) == B, "score_table_from_text: ", names[i], " must be contiguous with B = ", B, " rows");
  }
  TORCH_CHECK(out[1].dim() == 3 && out[1].size(1) == A, "score_table_from_text: gt_norm [B, A, Lg]");
  const int64_t Lg = out[1].size(2), NoOut = No > 0 ? No : 1;
  TORCH_CHECK(out[0].numel() == B * 4 && out[2].numel() == B * A && out[3].numel() == B * A && out[4].numel() == B * A * Lg && out[5].numel() == B * A &&
              out[6].numel() == B * NoOut * Lw && out[7].numel() == B * NoOut && out[8].numel() == B, "score_table_from_text: table tensors of inconsistent sizes");
  ok(sam_score_table_from_text((const int32_t*)answer_text.data_ptr(), La, (const int32_t*)answer_len.data_ptr(), (const int32_t*)ocr_text.data_ptr(), Lw,
                               (const int32_t*)ocr_len.data_ptr(), (const int32_t*)ocr_count.data_ptr(), (int)B, (int)A, (int)La, (int)No, (int)Lw, (int)Lg,
                               (int32_t*)out[0].data_ptr(), (int32_t*)out[1].data_ptr(), (int32_t*)out[2].data_ptr(), (float*)out[3].data_ptr(),
                               (int32_t*)out[4].data_ptr(), (int32_t*)out[5].data_ptr(), (int32_t*)out[6].data_ptr(), (int32_t*)out[7].data_ptr(),
                               (int32_t*)out[8].data_ptr(), cur_stream()), "sam_score_table_from_text");
}

// beam-search output to per-question results (include/sam_hip_eval.h): seqs int64 [B * K, S], cum fp32 [B * K], table: the eight score-table tensors of B
// samples in ops.SCORE_TABLE_KEYS order, vocab_cp int32 [V, Lw] / vocab_len int32 [V]; out: beam_scores fp32 [B * K, 3], beam_flags int32 [B * K], best int32
// [B], best_ids int64 [B, L], best_scores fp32 [B, 3], best_flags int32 [B], oracle fp32 [B, 3], answer int32 [B, L * (Lw + 1)], answer_len int32 [B], all
// written in place; totals float64 [4] (optional) is added to.
void eval_beams(const Tensor& seqs, const Tensor& cum, at::TensorList table, const Tensor& vocab_cp, const Tensor& vocab_len, int64_t eos, int64_t K, int64_t skip,
                at::TensorList out, const optional<Tensor>& totals) {
  need(seqs, at::kLong, "seqs"); need(cum, at::kFloat, "cum"); need(vocab_cp, at::kInt, "vocab_cp"); need(vocab_len, at::kInt, "vocab_len");
  TORCH_CHECK(table.size() == 8, "eval_beams: the score table is eight tensors (meta, gt_norm, gt_norm_len, gt_score, gt_raw, gt_raw_len, ocr, ocr_len)");
  for (int i = 0; i < 8; ++i) {
    need(table[i], i == 3 ? at::kFloat : at::kInt, "score table");
    TORCH_CHECK(table[i].is_contiguous(), "eval_beams: table tensors must be contiguous");
  }
  const Tensor &meta = table[0], &gt_norm = table[1], &gt_norm_len = table[2], &gt_score = table[3], &gt_raw = table[4], &gt_raw_len = table[5], &ocr = table[6],
               &ocr_len = table[7];
  TORCH_CHECK(seqs.dim() == 2 && seqs.is_contiguous() && cum.is_contiguous() && vocab_cp.dim() == 2 && vocab_cp.is_contiguous() && vocab_len.is_contiguous(),
              "eval_beams: contiguous seqs [B * K, S], cum [B * K], vocab_cp [V, Lw], vocab_len [V]");
  TORCH_CHECK(gt_norm.dim() == 3 && ocr.dim() == 3 && meta.dim() == 2 && meta.size(1) == 4, "eval_beams: meta [B, 4], gt_norm [B, A, Lg], ocr [B, No, Lw]");
  const int64_t R = seqs.size(0), S = seqs.size(1), B = meta.size(0), A = gt_norm.size(1), Lg = gt_norm.size(2), No = ocr.size(1), Lw = ocr.size(2),
                V = vocab_cp.size(0), L = S - skip;
  TORCH_CHECK(K >= 1 && R == B * K && cum.numel() == R, "eval_beams: seqs has ", R, " rows and cum ", cum.numel(), " elements for B = ", B, " samples of K = ", K, " beams");
  TORCH_CHECK(gt_norm.size(0) == B && gt_norm_len.numel() == B * A && gt_score.numel() == B * A && gt_raw.numel() == B * A * Lg && gt_raw_len.numel() == B * A &&
              ocr.size(0) == B && ocr_len.numel() == B * No && vocab_cp.size(1) == Lw && vocab_len.numel() == V, "eval_beams: tensors of inconsistent sizes");
  TORCH_CHECK(out.size() == 9, "eval_beams: out holds beam_scores, beam_flags, best, best_ids, best_scores, best_flags, oracle, answer, answer_len");
  const char* names[] = {"beam_scores", "beam_flags", "best", "best_ids", "best_scores", "best_flags", "oracle", "answer", "answer_len"};
  const at::ScalarType kinds[] = {at::kFloat, at::kInt, at::kInt, at::kLong, at::kFloat, at::kInt, at::kFloat, at::kInt, at::kInt};
  const int64_t Lp = L > 0 ? L : 0;
  const int64_t sizes[] = {R * 3, R, B, B * Lp, B * 3, B, B * 3, B * Lp * (Lw + 1), B};
  for (int i = 0; i < 9; ++i) {
    need(out[i], kinds[i], names[i]);
    TORCH_CHECK(out[i].is_contiguous() && out[i].numel() == sizes[i], "eval_beams: ", names[i], " must be contiguous with ", sizes[i], " elements");
  }
  double* tot = nullptr;
  if (totals.has_value() && totals->defined()) {
    need(*totals, at::kDouble, "totals");
    TORCH_CHECK(totals->is_contiguous() && totals->numel() == 4, "eval_beams: totals float64 [4]");
    tot = (double*)totals->data_ptr();
  }
  ok(sam_eval_beams((const int64_t*)seqs.data_ptr(), (const float*)cum.data_ptr(), (const int32_t*)meta.data_ptr(), (const int32_t*)gt_norm.data_ptr(),
                    (const int32_t*)gt_norm_len.data_ptr(), (const float*)gt_score.data_ptr(), (const int32_t*)gt_raw.data_ptr(), (const int32_t*)gt_raw_len.data_ptr(),
                    (const int32_t*)ocr.data_ptr(), (const int32_t*)ocr_len.data_ptr(), (const int32_t*)vocab_cp.data_ptr(), (const int32_t*)vocab_len.data_ptr(), (int)B,
                    (int)K, (int)S, (int)skip, (int)A, (int)Lg, (int)No, (int)Lw, (int)V, (int)eos, (float*)out[0].data_ptr(), (int32_t*)out[1].data_ptr(),
                    (int32_t*)out[2].data_ptr(), (int64_t*)out[3].data_ptr(), (float*)out[4].data_ptr(), (int32_t*)out[5].data_ptr(), (float*)out[6].data_ptr(),
                    (int32_t*)out[7].data_ptr(), (int32_t*)out[8].data_ptr(), tot, cur_stream()), "sam_eval_beams");
}

// the resident Unicode table (include/sam_hip_unicode.h): block int32 [8704], rec int32 [n_blocks, 128, 2], pool int32 [n_pool]
static void need_table(const Tensor& block, const Tensor& rec, const Tensor& pool, const char* who) {
  need(block, at::kInt, "unicode block"); need(rec, at::kInt, "unicode rec"); need(pool, at::kInt, "unicode pool");
  TORCH_CHECK(block.is_contiguous() && rec.is_contiguous() && pool.is_contiguous() && rec.numel() >= 256 && rec.numel() % 256 == 0 && pool.numel() >= 1 &&
              block.numel() <= 0x7fffffffLL && rec.numel() / 256 <= 0x7fffffffLL && pool.numel() <= 0x7fffffffLL,
              who, ": the table is contiguous block int32 [8704], rec int32 [n_blocks, 128, 2] and pool int32 [n_pool >= 1]");
}
#define SAM_TABLE_ARGS(block, rec, pool) \
  (const int32_t*)(block).data_ptr(), (int)(block).numel(), (const int32_t*)(rec).data_ptr(), (int)((rec).numel() / 256), (const int32_t*)(pool).data_ptr(), (int)(pool).numel()

// what the entry points that start from raw UTF-8 share: raw uint8 [nbytes], raw_off int32 [n + 1]; text int32 [n * width], text_len / status int32 [n] -> n.
// The messages speak as the entry point does: of S slots of L code points into text, or of B questions of Lq into question_text.
struct Utf8Names { const char *who, *n, *unit, *width, *text; };
static int64_t utf8_io(const Utf8Names& s, const Tensor& raw, const Tensor& raw_off, int64_t width, int64_t max_width, const Tensor& text, const Tensor& text_len,
                       const Tensor& status) {
  const std::string len_name = std::string(s.text) + "_len";
  need(raw, at::kByte, "raw"); need(raw_off, at::kInt, "raw_off");
  need(text, at::kInt, s.text); need(text_len, at::kInt, len_name.c_str()); need(status, at::kInt, "status");
  TORCH_CHECK(raw.dim() == 1 && raw.is_contiguous() && raw_off.dim() == 1 && raw_off.is_contiguous() && raw_off.numel() >= 2,
              s.who, ": contiguous raw uint8 [nbytes] and raw_off int32 [", s.n, " + 1], ", s.n, " >= 1");
  const int64_t n = raw_off.numel() - 1;
  TORCH_CHECK(n <= 0x7fffffffLL && width >= 1 && width <= max_width,
              s.who, ": ", s.n, " = ", n, " ", s.unit, " of ", s.width, " = ", width, " code points (1 <= ", s.width, " <= ", max_width, ")");
  TORCH_CHECK(text.is_contiguous() && text.numel() == n * width && text_len.is_contiguous() && text_len.numel() == n && status.is_contiguous() && status.numel() == n,
              s.who, ": ", s.text, " must be contiguous with ", s.n, " * ", s.width, " = ", n * width, " elements, ", len_name, " and status with ", s.n, " = ", n);
  return n;
}

// raw UTF-8 strings to cleaned code points (include/sam_hip_textprep.h); with the table (all three or none) lowered as str.lower() lowers (sam_hip_unicode.h)
static void text_from_utf8_impl(const char* who, const Tensor& raw, const Tensor& raw_off, int64_t L, int64_t mode, const Tensor* block, const Tensor* rec,
                                const Tensor* pool, Tensor& text, Tensor& text_len, Tensor& status) {
  const int64_t S = utf8_io({who, "S", "slots", "L", "text"}, raw, raw_off, L, 128, text, text_len, status);
  const uint8_t* r = (const uint8_t*)raw.data_ptr();
  const int32_t* off =(const int32_t*)raw_off.data_ptr();
  int32_t *t = (int32_t*)text.data_ptr(), *tl = (int32_t*)text_len.data_ptr(), *st = (int32_t*)status.data_ptr();
  if (!block) {
    ok(sam_text_from_utf8(r, raw.numel(), off, (int)S, (int)L, (int)mode, t, tl, st, cur_stream()), "sam_text_from_utf8");
    return;
  }
  need_table(*block, *rec, *pool, who);
  ok(sam_text_from_utf8_unicode(r, raw.numel(), off, (int)S, (int)L, (int)mode, SAM_TABLE_ARGS(*block, *rec, *pool), t, tl, st, cur_stream()), "sam_text_from_utf8_unicode");
}

void text_from_utf8(const Tensor& raw, const Tensor& raw_off, int64_t L, int64_t mode, Tensor text, Tensor text_len, Tensor status) {
  text_from_utf8_impl("text_from_utf8", raw, raw_off, L, mode, nullptr, nullptr, nullptr, text, text_len, status);
}

void text_from_utf8_unicode(const Tensor& raw, const Tensor& raw_off, int64_t L, int64_t mode, const Tensor& block, const Tensor& rec, const Tensor& pool, Tensor text,
                            Tensor text_len, Tensor status) {
  text_from_utf8_impl("text_from_utf8_unicode", raw, raw_off, L, mode, &block, &rec, &pool, text, text_len, status);
}

// the questions' raw UTF-8 to their packed text: question_text int32 [B * Lq], question_text_len / status int32 [B]
void question_from_utf8(const Tensor& raw, const Tensor& raw_off, int64_t Lq, const Tensor& block, const Tensor& rec, const Tensor& pool, Tensor text, Tensor text_len,
                        Tensor status) {
  const int64_t B = utf8_io({"question_from_utf8", "B", "questions", "Lq", "question_text"}, raw, raw_off, Lq, 1024, text, text_len, status);
  need_table(block, rec, pool, "question_from_utf8");
  ok(sam_question_from_utf8((const uint8_t*)raw.data_ptr(), raw.numel(), (const int32_t*)raw_off.data_ptr(), (int)B, (int)Lq, SAM_TABLE_ARGS(block, rec, pool),
                            (int32_t*)text.data_ptr(), (int32_t*)text_len.data_ptr(), (int32_t*)status.data_ptr(), cur_stream()), "sam_question_from_utf8");
}

// the build's status int32 [B] folded into the sticky record state int64 [4] (include/sam_hip_step.h); the step is step_dev[0] + step with step_dev int64 [1]
void answer_status_fold(const Tensor& status, const optional<Tensor>& step_dev, int64_t step, Tensor state) {
  need(status, at::kInt, "status");
  need(state, at::kLong, "state");
  TORCH_CHECK(status.is_contiguous() && status.numel() >= 1 && state.is_contiguous() && state.numel() == 4, "answer_status_fold: contiguous status int32 [B >= 1], state int64 [4]");
  const int64_t* sd = nullptr;
  if (step_dev.has_value() && step_dev->defined()) {
    need(*step_dev, at::kLong, "step_dev");
    TORCH_CHECK(step_dev->numel() >= 1, "answer_status_fold: step_dev int64 [1]");
    sd = (const int64_t*)step_dev->data_ptr();
  }
  ok(sam_answer_status_fold((const int32_t*)status.data_ptr(), (int)status.numel(), sd, step, (int64_t*)state.data_ptr(), cur_stream()), "sam_answer_status_fold");
}

// the questions' WordPiece ids from their text (include/sam_hip_question.h): text int32 [B, Lq], text_len int32 [B], the vocabulary index (vocab_cp int32
// [V, Lv], vocab_len int32 [V], slots int32 [n_slots]); indices / mask int64 [B, T] (row-major, row stride >= T: T columns of a wider row are allowed),
// count int32 [B]
void wordpiece_from_text(const Tensor& text, const Tensor& text_len, const Tensor& vocab_cp, const Tensor& vocab_len, const Tensor& slots, int64_t unk, int64_t cls,
                         int64_t sep, Tensor indices, Tensor mask, Tensor count) {
  const Tensor* in[] = {&text, &text_len, &vocab_cp, &vocab_len, &slots, &count};
  const char* in_names[] = {"question_text", "question_text_len", "vocab cp", "vocab len", "vocab slots", "count"};
  for (int i = 0; i < 6; ++i) {
    need(*in[i], at::kInt, in_names[i]);
    TORCH_CHECK(in[i]->is_contiguous(), "wordpiece_from_text: ", in_names[i], " must be contiguous");
  }
  need(indices, at::kLong, "indices");
  need(mask, at::kLong, "mask");
  TORCH_CHECK(text.dim() == 2 && vocab_cp.dim() == 2 && indices.dim() == 2 && mask.dim() == 2, "wordpiece_from_text: text [B, Lq], vocab cp [V, Lv], indices / mask [B, T]");
  const int64_t B = text.size(0), Lq = text.size(1), V = vocab_cp.size(0), Lv = vocab_cp.size(1), T = indices.size(1);
  TORCH_CHECK(text_len.numel() == B && vocab_len.numel() == V && count.numel() == B, "wordpiece_from_text: text_len [B], vocab len [V], count [B]");
  TORCH_CHECK(indices.size(0) == B && mask.size(0) == B && mask.size(1) == T && indices.stride(1) == 1 && mask.stride(1) == 1 &&
              (B == 1 || (indices.stride(0) >= T && mask.stride(0) >= T)), "wordpiece_from_text: indices and mask must be row-major [B, T] with a row stride >= T");
  ok(sam_wordpiece_from_text((const int32_t*)text.data_ptr(), Lq, (const int32_t*)text_len.data_ptr(), (const int32_t*)vocab_cp.data_ptr(), Lv,
                             (const int32_t*)vocab_len.data_ptr(), (const int32_t*)slots.data_ptr(), (int)B, (int)Lq, (int)V, (int)Lv, (int)slots.numel(), (int)unk,
                             (int)cls, (int)sep, (int)T, (int64_t*)indices.data_ptr(), B == 1 ? T : indices.stride(0), (int64_t*)mask.data_ptr(),
                             B == 1 ? T : mask.stride(0), (int32_t*)count.data_ptr(), cur_stream()), "sam_wordpiece_from_text");
}

// the OCR tokens' FastText vectors from their text (include/sam_hip_fasttext.h): text int32 [B, n_max, Lw] (or [B * n_max, Lw], row stride >= Lw), text_len int32
// [B * n_max], counts int32 [B] or none; matrix fp32 [nwords + bucket, dim]; the index (index_cp int32 [nwords, Lv], index_len int32 [nwords], slots int32
// [n_slots]); dst 2-D [B * n_max, ld] fp32 / bf16
void fasttext_from_text(const Tensor& text, const Tensor& text_len, const optional<Tensor>& counts, int64_t batch, int64_t n_max, const Tensor& matrix,
                        const Tensor& index_cp, const Tensor& index_len, const Tensor& slots, int64_t minn, int64_t maxn, int64_t bucket, int64_t nwords, int64_t eos,
                        Tensor dst, int64_t col0, bool normalize, double eps) {
  const SlotText t = slot_text("fasttext_from_text", text, text_len, counts, batch, n_max);
  need(matrix, at::kFloat, "matrix"); need(index_cp, at::kInt, "index cp"); need(index_len, at::kInt, "index len"); need(slots, at::kInt, "index slots");
  TORCH_CHECK(matrix.dim() == 2 && matrix.stride(1) == 1 && matrix.size(0) == nwords + bucket && nwords >= 1 && bucket >= 0,
              "fasttext_from_text: matrix must be row-major fp32 [nwords + bucket, dim] = [", nwords + bucket, ", dim]");
  TORCH_CHECK(index_cp.dim() == 2 && index_cp.is_contiguous() && index_cp.size(0) == nwords && index_len.is_contiguous() && index_len.numel() == nwords &&
              slots.is_contiguous(), "fasttext_from_text: index cp [nwords, Lv], len [nwords] and slots must be contiguous");
  const int64_t dim = matrix.size(1);
  TORCH_CHECK(dst.is_cuda() && dst.dim() == 2 && dst.stride(1) == 1 && dst.size(0) == t.rows, "fasttext_from_text: dst must be a row-major 2-D GPU tensor of B * n_max rows");
  TORCH_CHECK(dst.scalar_type() == at::kBFloat16 || dst.scalar_type() == at::kFloat, "fasttext_from_text: dst must be bf16 or fp32");
  TORCH_CHECK(col0 >= 0 && col0 + dim <= dst.size(1), "fasttext_from_text: columns [", col0, ", ", col0 + dim, ") exceed dst's ", dst.size(1));
  ok(sam_fasttext_from_text(t.text, t.ld, (const int32_t*)text_len.data_ptr(), t.counts, (int)batch, (int)n_max, (int)t.lw, (const float*)matrix.data_ptr(),
                            matrix.size(0) == 1 ? dim : matrix.stride(0), (const int32_t*)index_cp.data_ptr(), index_cp.size(1), (const int32_t*)index_len.data_ptr(),
                            (const int32_t*)slots.data_ptr(), (int)index_cp.size(1), (int)slots.numel(), (int)minn, (int)maxn, (int)bucket, (int)nwords, (int)eos, (int)dim,
                            dst.data_ptr(), t.rows == 1 ? dst.size(1) : dst.stride(0), (int)col0, dst.scalar_type() == at::kFloat, normalize, (float)eps, cur_stream()),
     "sam_fasttext_from_text");
}

// ---------------------------------------------------------------------------------------------------------------- coarse: one encoder layer
// params: wqkv bf16 [3D,D], bqkv f32 [3D], wo bf16 [D,D], bo f32, ln1_w, ln1_b, w1 bf16 [I,D], b1 f32, w2 bf16 [D,I], b2 f32, ln2_w, ln2_b
enum { P_WQKV, P_BQKV, P_WO, P_BO, P_LN1W, P_LN1B, P_W1, P_B1, P_W2, P_B2, P_LN2W, P_LN2B, P_COUNT };
// saved: x, qkv, ctx, lse2, keep, z1, mean1, rstd1, a, pre, h, z2, mean2, rstd2
// (+ ctx_lo, the output residual of the attention forward, last: empty when the sequence is too long for the one-pass attention backward)
enum { S_X, S_QKV, S_CTX, S_LSE, S_KEEP, S_Z1, S_MEAN1, S_RSTD1, S_A, S_PRE, S_H, S_Z2, S_MEAN2, S_RSTD2, S_CTXLO, S_COUNT };

std::vector<Tensor> encoder_layer_fwd(const Tensor& x, const Tensor& allow, at::TensorList params, int64_t batch, int64_t heads, double scale, double p_attn,
                                      double p_hid, at::IntArrayRef seeds, double eps1, double eps2) {
  TORCH_CHECK(params.size() == P_COUNT, "encoder_layer_fwd: expected ", (int)P_COUNT, " parameter tensors");
  TORCH_CHECK(seeds.size() == 6, "encoder_layer_fwd: seeds = (seed, offset) x 3 dropout sites");
  need2d(x, "x");
  GemmOpt o;
  o.epilogue = SAM_EPI_BIAS; o.bias = &params[P_BQKV];
  Tensor qkv = gemm(x, params[P_WQKV], true, true, o);                                                   // sa_m4c.py:554-560
  Tensor ctx, lse2, keep, ctx_lo;
  if (fused_attn_bwd_enabled(x.size(0) / batch)) std::tie(ctx, lse2, keep, ctx_lo) = attn_fwd_train(qkv, allow, batch, heads, scale, p_attn, seeds[0], seeds[1]);      // :563-598
  else { std::tie(ctx, lse2, keep) = attn_fwd(qkv, allow, batch, heads, scale, p_attn, seeds[0], seeds[1]); ctx_lo = at::empty({0}, x.options()); }
  o = GemmOpt(); o.epilogue = SAM_EPI_BIAS_DROPOUT_RES; o.bias = &params[P_BO]; o.residual = &x; o.p_drop = (float)p_hid; o.seed = seeds[2]; o.offset = seeds[3];
  auto [z1, a, mean1, rstd1] = gemm_ln(ctx, params[P_WO], params[P_LN1W], params[P_LN1B], eps1, o);      // BertSelfOutput via :653
  Tensor pre = at::empty({x.size(0), params[P_W1].size(0)}, x.options());
  o = GemmOpt(); o.epilogue = SAM_EPI_BIAS_GELU_GRAD; o.bias = &params[P_B1]; o.aux_out = &pre;      // pre := gelu'(a W1^T + b1): the backward multiplies, no erf there
  Tensor h = gemm(a, params[P_W1], true, true, o);                                                        // BertIntermediate via :678
  o = GemmOpt(); o.epilogue = SAM_EPI_BIAS_DROPOUT_RES; o.bias = &params[P_B2]; o.residual = &a; o.p_drop = (float)p_hid; o.seed = seeds[4]; o.offset = seeds[5];
  auto [z2, y, mean2, rstd2] = gemm_ln(h, params[P_W2], params[P_LN2W], params[P_LN2B], eps2, o);          // BertOutput via :680
  return {y, x, qkv, ctx, lse2, keep, z1, mean1, rstd1, a, pre, h, z2, mean2, rstd2, ctx_lo};
}

// grads: same order as params, fp32 views into the flat gradient buffer (accumulated in place).  Returns dx (undefined-size-0 when !need_dx).
static std::vector<Tensor> encoder_layer_bwd_impl(const Tensor& dy_in, at::TensorList saved, const Tensor& allow, at::TensorList params, at::TensorList grads, int64_t batch,
                                                  int64_t heads, double scale, double p_attn, double p_hid, at::IntArrayRef seeds, bool need_dx, bool accumulate, bool defer_wgrad) {
  // accumulate = false: every one of the twelve gradients is OVERWRITTEN (each is written exactly once by this call) -- the caller then need not
  // zero them before the backward pass, and the weight-gradient kernels skip the read half of their read-modify-write
  TORCH_CHECK(saved.size() == S_COUNT && params.size() == P_COUNT && grads.size() == P_COUNT, "encoder_layer_bwd: bad list sizes");
  Tensor dy = dy_in;
  if (dy.scalar_type() != at::kBFloat16 || !dy.is_contiguous()) dy = dy.to(at::kBFloat16).contiguous();
  const Tensor &x = saved[S_X], &qkv = saved[S_QKV], &ctx = saved[S_CTX], &lse2 = saved[S_LSE], &keep = saved[S_KEEP], &z1 = saved[S_Z1], &a = saved[S_A],
               &pre = saved[S_PRE], &h = saved[S_H], &z2 = saved[S_Z2];
  // ---- output block: y = LN(dropout(h W2^T + b2) + a)
  auto [dz2, dy2] = ln_bwd(dy, z2, saved[S_MEAN2], saved[S_RSTD2], params[P_LN2W], grads[P_LN2W], grads[P_LN2B], &grads[P_B2], true, p_hid, seeds[4], seeds[5], accumulate, true);
  GemmOpt o;
  o.epilogue = SAM_EPI_MUL_AUX; o.aux_in = &pre;
  Tensor dpre = gemm(dy2, params[P_W2], true, false, o);
  // ---- intermediate: h = gelu(a W1^T + b1)
  o = GemmOpt(); o.epilogue = SAM_EPI_BIAS_DROPOUT_RES; o.residual = &dz2;
  Tensor da = gemm(dpre, params[P_W1], true, false, o);
  // ---- attention output block: a = LN(dropout(ctx Wo^T + bo) + x)
  auto [dz1, dy1] = ln_bwd(da, z1, saved[S_MEAN1], saved[S_RSTD1], params[P_LN1W], grads[P_LN1W], grads[P_LN1B], &grads[P_BO], true, p_hid, seeds[2], seeds[3], accumulate, true);
  Tensor dctx = gemm(dy1, params[P_WO], true, false, GemmOpt());
  // ---- attention core + fused QKV projection
  Tensor dqkv = saved[S_CTXLO].numel() ? attn_bwd_fused(dctx, qkv, ctx, saved[S_CTXLO], lse2, allow, keep, batch, heads, scale, p_attn)
                                       : attn_bwd(dctx, qkv, lse2, allow, keep, batch, heads, scale, p_attn);
  const Tensor dw2 = grads[P_W2], dw1 = grads[P_W1], db1 = grads[P_B1], dwo = grads[P_WO], dwqkv = grads[P_WQKV], dbqkv = grads[P_BQKV];
  // defer_wgrad: the four weight gradients are left to the caller, which runs them for several layers in ONE grouped launch (TextBert's three
  // 1280-row layers: 3 x 38 us of launches that cannot fill the chip -> one); the gradient operands come back with dx
  if (!defer_wgrad) wgrad_grouped({{&dy2, &h, &dw2, nullptr}, {&dpre, &a, &dw1, &db1}, {&dy1, &ctx, &dwo, nullptr}, {&dqkv, &x, &dwqkv, &dbqkv}}, accumulate);
  Tensor dx = at::empty({0}, x.options());
  if (need_dx) {
    o = GemmOpt(); o.epilogue = SAM_EPI_BIAS_DROPOUT_RES; o.residual = &dz1;
    dx = gemm(dqkv, params[P_WQKV], true, false, o);
  }
  if (defer_wgrad) return {dx, dy2, dpre, dy1, dqkv};
  return {dx};
}
Tensor encoder_layer_bwd(const Tensor& dy_in, at::TensorList saved, const Tensor& allow, at::TensorList params, at::TensorList grads, int64_t batch, int64_t heads,
                         double scale, double p_attn, double p_hid, at::IntArrayRef seeds, bool need_dx, bool accumulate) {
  return encoder_layer_bwd_impl(dy_in, saved, allow, params, grads, batch, heads, scale, p_attn, p_hid, seeds, need_dx, accumulate, false)[0];
}
std::vector<Tensor> encoder_layer_bwd_nowgrad(const Tensor& dy_in, at::TensorList saved, const Tensor& allow, at::TensorList params, at::TensorList grads, int64_t batch,
                                              int64_t heads, double scale, double p_attn, double p_hid, at::IntArrayRef seeds, bool need_dx, bool accumulate) {
  return encoder_layer_bwd_impl(dy_in, saved, allow, params, grads, batch, heads, scale, p_attn, p_hid, seeds, need_dx, accumulate, true);
}
// dW_q (+)= dy_q^T x_q (and db_q (+)= column sums of dy_q) for up to 20 problems in one launch
void wgrad_grouped_op(at::TensorList dys, at::TensorList xs, at::TensorList dws, at::TensorList dbs, bool accumulate) {
  TORCH_CHECK(dys.size() == xs.size() && dys.size() == dws.size() && dys.size() == dbs.size(), "wgrad_grouped: list sizes differ");
  std::vector<WgradJob> jobs;
  for (size_t q = 0; q < dys.size(); ++q) jobs.push_back({&dys[q], &xs[q], &dws[q], dbs[q].numel() ? &dbs[q] : nullptr});
  wgrad_grouped(jobs, accumulate);
}

// ---------------------------------------------------------------------------------------------------------------- fine-grained op wrappers
std::tuple<Tensor, Tensor> linear_op(const Tensor& x, const Tensor& w, const optional<Tensor>& bias, int64_t epilogue, const optional<Tensor>& residual,
                                     const optional<Tensor>& aux_in, bool want_aux_out, double p_drop, int64_t seed, int64_t offset, bool b_kcontig, bool out_f32) {
  GemmOpt o;
  o.epilogue = (int)epilogue; o.p_drop = (float)p_drop; o.seed = seed; o.offset = offset; o.out_f32 = out_f32;
  Tensor b_, r_, ai_, aux;
  if (bias.has_value() && bias->defined()) { b_ = need(*bias, at::kFloat, "bias"); o.bias = &b_; }
  if (residual.has_value() && residual->defined()) { r_ = *residual; need2d(r_, "residual"); o.residual = &r_; }
  if (aux_in.has_value() && aux_in->defined()) { ai_ = *aux_in; need2d(ai_, "aux_in"); o.aux_in = &ai_; }
  const int64_t N = b_kcontig ? w.size(0) : w.size(1);
  if (want_aux_out) { aux = at::empty({x.size(0), N}, x.options()); o.aux_out = &aux; }
  Tensor y = gemm(x, w, true, b_kcontig, o);
  return {y, want_aux_out ? aux : at::empty({0}, x.options())};
}

std::tuple<Tensor, Tensor, Tensor> layernorm_fwd_op(const Tensor& x, const Tensor& gamma, const Tensor& beta, double eps) { return ln_fwd(x, gamma, beta, eps); }

std::tuple<Tensor, Tensor, Tensor> layernorm_bwd_op(const Tensor& dy, const Tensor& x, const Tensor& mean, const Tensor& rstd, const Tensor& gamma) {
  Tensor dg = at::zeros_like(gamma), db = at::zeros_like(gamma);
  auto r = ln_bwd(dy, x, mean, rstd, gamma, dg, db, nullptr, false, 0.0, 0, 0);
  return {std::get<0>(r), dg, db};
}

// ---------------------------------------------------------------------------------------------------------------- the aux heads' loss from relation codes
// (include/sam_hip_aux_loss.h, which sam_hip.h includes)  O, D f32 [B, n, 32]; W f32 [12, 32]; bias f32 [12]; codes u8 [B, n, n]; valid u8 [B, n]
void aux_loss_operands(const Tensor& o, const Tensor& d, const Tensor& w, const Tensor& bias, const Tensor& codes, const Tensor& valid, const char* who) {
  need(o, at::kFloat, "O"); need(d, at::kFloat, "D"); need(w, at::kFloat, "W"); need(bias, at::kFloat, "bias"); need(codes, at::kByte, "codes"); need(valid, at::kByte, "valid");
  TORCH_CHECK(o.dim() == 3 && o.size(2) == 32 && o.sizes() == d.sizes() && o.size(0) > 0 && o.size(1) > 0 && o.is_contiguous() && d.is_contiguous(), who,
              ": contiguous O, D [B, n, 32] of one shape");
  const int64_t b = o.size(0), n = o.size(1);
  TORCH_CHECK(w.is_contiguous() && w.dim() == 2 && w.size(0) == 12 && w.size(1) == 32 && bias.is_contiguous() && bias.numel() == 12, who, ": W [12, 32] and bias [12]");
  TORCH_CHECK(codes.is_contiguous() && codes.dim() == 3 && codes.size(0) == b && codes.size(1) == n && codes.size(2) == n && valid.is_contiguous() && valid.dim() == 2 &&
              valid.size(0) == b && valid.size(1) == n, who, ": codes u8 [B, n, n] and valid u8 [B, n]");
}
// -> (loss f32 [1], count f32 [1])
std::tuple<Tensor, Tensor> aux_pair_loss(const Tensor& o, const Tensor& d, const Tensor& w, const Tensor& bias, const Tensor& codes, const Tensor& valid, int64_t fusion) {
  aux_loss_operands(o, d, w, bias, codes, valid, "aux_pair_loss");
  const int b = (int)o.size(0), n = (int)o.size(1);
  Tensor out = at::empty({2}, o.options());
  const int64_t bytes = sam_aux_pair_loss_fwd_ws_bytes(b, n);
  Tensor& ws = workspace("aux_loss", bytes, o);
  ok(sam_aux_pair_loss_fwd((const float*)o.data_ptr(), (const float*)d.data_ptr(), (const float*)w.data_ptr(), (const float*)bias.data_ptr(), (const uint8_t*)codes.data_ptr(),
                           (const uint8_t*)valid.data_ptr(), b, n, (int)fusion, (float*)out.data_ptr(), (float*)out.data_ptr() + 1, (float*)ws.data_ptr(), ws.numel() * 4,
                           cur_stream()), "sam_aux_pair_loss_fwd");
  return {out.narrow(0, 0, 1), out.narrow(0, 1, 1)};
}
// -> (dO, dD); dW [12, 32] / dbias [12] are added to (accumulate) or overwritten
std::tuple<Tensor, Tensor> aux_pair_loss_bwd(const optional<Tensor>& grad_out, const Tensor& count, const Tensor& o, const Tensor& d, const Tensor& w, const Tensor& bias,
                                             const Tensor& codes, const Tensor& valid, Tensor dw, Tensor dbias, int64_t fusion, bool accumulate) {
  aux_loss_operands(o, d, w, bias, codes, valid, "aux_pair_loss_bwd");
  need(count, at::kFloat, "count"); need(dw, at::kFloat, "dW"); need(dbias, at::kFloat, "dbias");
  if (grad_out.has_value() && grad_out->defined()) { need(*grad_out, at::kFloat, "grad_out"); TORCH_CHECK(grad_out->numel() == 1, "aux_pair_loss_bwd: grad_out holds one value"); }
  TORCH_CHECK(count.numel() == 1 && dw.is_contiguous() && dw.numel() == 384 && dbias.is_contiguous() && dbias.numel() == 12, "aux_pair_loss_bwd: count [1], dW [12, 32], dbias [12]");
  const int b = (int)o.size(0), n = (int)o.size(1);
  Tensor d_o = at::empty_like(o), d_d = at::empty_like(d);
  const int64_t bytes = sam_aux_pair_loss_bwd_ws_bytes(b, n);
  Tensor& ws = workspace("aux", bytes, o);
  ok(sam_aux_pair_loss_bwd((const float*)p(grad_out), (const float*)count.data_ptr(), (const float*)o.data_ptr(), (const float*)d.data_ptr(), (const float*)w.data_ptr(),
                           (const float*)bias.data_ptr(), (const uint8_t*)codes.data_ptr(), (const uint8_t*)valid.data_ptr(), b, n, (int)fusion, (float*)d_o.data_ptr(),
                           (float*)d_d.data_ptr(), (float*)dw.data_ptr(), (float*)dbias.data_ptr(), accumulate ? 1 : 0, (float*)ws.data_ptr(), ws.numel() * 4, cur_stream()),
     "sam_aux_pair_loss_bwd");
  return {d_o, d_d};
}
// boxes f32 / f64 [B, n, >= 4] with unit column stride (ocr_boxes optional) -> codes u8 [B, n_obj + n_ocr, n_obj + n_ocr]
Tensor relation_codes_from_boxes(const Tensor& obj_boxes, const optional<Tensor>& ocr_boxes, double distance_threshold) {
  TORCH_CHECK(obj_boxes.defined() && obj_boxes.is_cuda() && (obj_boxes.scalar_type() == at::kFloat || obj_boxes.scalar_type() == at::kDouble), "obj_boxes: f32 or f64 on the GPU");
  const bool has_ocr = ocr_boxes.has_value() && ocr_boxes->defined() && ocr_boxes->dim() == 3 && ocr_boxes->size(1) > 0;
  auto rows = [](const Tensor& t, const char* name) {
    TORCH_CHECK(t.dim() == 3 && t.size(2) >= 4, name, ": [B, n, >= 4]");
    return (t.stride(2) == 1 && t.stride(1) >= 4 && t.stride(0) == t.size(1) * t.stride(1)) ? t : t.contiguous();
  };
  Tensor ob = rows(obj_boxes, "obj_boxes"), cb;
  TORCH_CHECK(ob.size(0) > 0 && ob.size(1) > 0, "relation_codes_from_boxes: need at least one sample and one object row");
  if (has_ocr) {
    TORCH_CHECK(ocr_boxes->is_cuda() && ocr_boxes->scalar_type() == ob.scalar_type() && ocr_boxes->size(0) == ob.size(0), "ocr_boxes: dtype and batch size of obj_boxes");
    cb = rows(*ocr_boxes, "ocr_boxes");
  }
  const int64_t b = ob.size(0), n_obj = ob.size(1), n_ocr = has_ocr ? cb.size(1) : 0;
  Tensor codes = at::empty({b, n_obj + n_ocr, n_obj + n_ocr}, ob.options().dtype(at::kByte));
  ok(sam_relation_codes_from_boxes(ob.data_ptr(), ob.stride(1), (int)n_obj, has_ocr ? cb.data_ptr() : nullptr, has_ocr ? cb.stride(1) : 0, (int)n_ocr,
                                   ob.scalar_type() == at::kDouble ? 1 : 0, (int)b, distance_threshold, (uint8_t*)codes.data_ptr(), cur_stream()), "sam_relation_codes_from_boxes");
  return codes;
}

// ---------------------------------------------------------------------------------------------------------------- the aux loss's targets in one launch
// (include/sam_hip_aux_targets.h)  rel i8 [B, n, n, 12] (optional); obj_mask [B, n_obj], ocr_mask [B, n_ocr]: bool or an integer type of 1, 4 or 8 bytes, one
// dtype, unit column stride -> (codes u8 [B, n, n], valid u8 [B, n]); without rel the codes come back empty ([0]), as the other absent outputs here do
std::tuple<Tensor, Tensor> aux_targets(const optional<Tensor>& rel, const Tensor& obj_mask, const Tensor& ocr_mask) {
  auto mask = [](const Tensor& t, const char* name) {
    TORCH_CHECK(t.defined() && t.is_cuda() && t.dim() == 2, name, ": [B, n] on the GPU (this package has no CPU path)");
    TORCH_CHECK(!at::isFloatingType(t.scalar_type()) && !at::isComplexType(t.scalar_type()) && (t.element_size() == 1 || t.element_size() == 4 || t.element_size() == 8),
                name, ": bool or an integer type of 1, 4 or 8 bytes, got ", t.scalar_type());
    return (t.size(1) == 0 || t.stride(1) == 1) && (t.size(0) <= 1 || t.stride(0) >= t.size(1)) ? t : t.contiguous();
  };
  Tensor om = mask(obj_mask, "obj_mask"), cm = mask(ocr_mask, "ocr_mask");
  TORCH_CHECK(om.scalar_type() == cm.scalar_type() && om.size(0) == cm.size(0), "aux_targets: the two masks share dtype and batch size");
  const int64_t b = om.size(0), n_obj = om.size(1), n_ocr = cm.size(1), n = n_obj + n_ocr;
  const bool has_rel = rel.has_value() && rel->defined();
  if (has_rel) {
    need(*rel, at::kChar, "rel");
    TORCH_CHECK(rel->is_contiguous() && rel->dim() == 4 && rel->size(0) == b && rel->size(1) == n && rel->size(2) == n && rel->size(3) == 12,
                "aux_targets: rel must be a contiguous int8 [", b, ", ", n, ", ", n, ", 12], got ", rel->sizes());
  }
  Tensor valid = at::empty({b, n}, om.options().dtype(at::kByte));
  Tensor codes = has_rel ? at::empty({b, n, n}, valid.options()) : at::empty({0}, valid.options());
  auto ld = [](const Tensor& t) { return t.size(0) > 1 ? t.stride(0) : t.size(1); };
  ok(sam_aux_targets(has_rel ? (const int8_t*)rel->data_ptr() : nullptr, n_obj ? om.data_ptr() : nullptr, ld(om), (int)n_obj, n_ocr ? cm.data_ptr() : nullptr, ld(cm), (int)n_ocr,
                     (int)om.element_size(), (int)b, (int)n, has_rel ? (uint8_t*)codes.data_ptr() : nullptr, (uint8_t*)valid.data_ptr(), cur_stream()), "sam_aux_targets");
  return {codes, valid};
}

// ---------------------------------------------------------------------------------------------------------------- the aux heads' confusion counts
// (include/sam_hip_aux_stats.h)  operands as aux_pair_loss; confusion i64 [13, 13] and fired i64 [13, 12] are overwritten, or added to (accumulate)
void aux_pair_stats(const Tensor& o, const Tensor& d, const Tensor& w, const Tensor& bias, const Tensor& codes, const Tensor& valid, int64_t fusion, Tensor confusion,
                    Tensor fired, bool accumulate) {
  aux_loss_operands(o, d, w, bias, codes, valid, "aux_pair_stats");
  need(confusion, at::kLong, "confusion"); need(fired, at::kLong, "fired");
  TORCH_CHECK(confusion.is_contiguous() && confusion.numel() == 169 && fired.is_contiguous() && fired.numel() == 156, "aux_pair_stats: confusion [13, 13] and fired [13, 12]");
  const int b = (int)o.size(0), n = (int)o.size(1);
  int64_t bytes = 0;
  ok(sam_aux_pair_stats_ws_bytes(b, n, &bytes), "sam_aux_pair_stats_ws_bytes");
  Tensor& ws = workspace("aux_stats", bytes, o);
  ok(sam_aux_pair_stats((const float*)o.data_ptr(), (const float*)d.data_ptr(), (const float*)w.data_ptr(), (const float*)bias.data_ptr(), (const uint8_t*)codes.data_ptr(),
                        (const uint8_t*)valid.data_ptr(), b, n, (int)fusion, (int64_t*)confusion.data_ptr(), (int64_t*)fired.data_ptr(), accumulate ? 1 : 0, ws.data_ptr(),
                        ws.numel() * 4, cur_stream()), "sam_aux_pair_stats");
}

}  // namespace

TORCH_LIBRARY(sam_hip, m) {
  m.def("linear(Tensor x, Tensor w, Tensor? bias, int epilogue, Tensor? residual, Tensor? aux_in, bool want_aux_out, float p_drop, int seed, int offset, "
        "bool b_kcontig, bool out_f32) -> (Tensor, Tensor)");
  m.def("spatial_attn_fwd(Tensor qkv, Tensor allow, int batch, int heads, float scale, float p_drop, int seed, int offset) -> (Tensor, Tensor, Tensor)");
  m.def("spatial_attn_bwd(Tensor dout, Tensor qkv, Tensor lse2, Tensor allow, Tensor keep, int batch, int heads, float scale, float p_drop) -> Tensor");
  m.def("spatial_attn_fwd_train(Tensor qkv, Tensor allow, int batch, int heads, float scale, float p_drop, int seed, int offset) -> (Tensor, Tensor, Tensor, Tensor)");
  m.def("spatial_attn_bwd_fused(Tensor dout, Tensor qkv, Tensor out, Tensor out_lo, Tensor lse2, Tensor allow, Tensor keep, int batch, int heads, float scale, float p_drop) -> Tensor");
  m.def("layernorm_fwd(Tensor x, Tensor gamma, Tensor beta, float eps) -> (Tensor, Tensor, Tensor)");
  m.def("layernorm_bwd(Tensor dy, Tensor x, Tensor mean, Tensor rstd, Tensor gamma) -> (Tensor, Tensor, Tensor)");
  m.def("set_ln_defer(bool on) -> ()");
  m.def("ln_finalize_flush() -> ()");
  m.def("ln_finalize_clear() -> ()");
  m.def("pack_masks(Tensor question_mask, Tensor obj_mask, Tensor ocr_mask) -> (Tensor, Tensor, Tensor)");
  m.def("mask_bits_prefix_lm(Tensor key_valid, int n_dec) -> Tensor");
  m.def("mask_bits_from_additive(Tensor mask) -> Tensor");
  m.def("pack_relations(Tensor base_bits, Tensor adj, int n_txt, int heads, int quadrant_bits) -> Tensor");
  m.def("pack_relations_bhnn(Tensor rel, Tensor? base_bits) -> Tensor");
  m.def("ptr_scores(Tensor q, Tensor k, Tensor ocr_mask, float scale) -> Tensor");
  m.def("ptr_scores_bwd(Tensor dscores, Tensor q, Tensor k, float scale) -> (Tensor, Tensor)");
  m.def("bce_loss(Tensor fixed, Tensor ocr, Tensor targets, Tensor loss_mask, float grad_scale, Tensor? global_count) -> (Tensor, Tensor, Tensor)");
  m.def("sumsq(Tensor g, Tensor(a!) out, int[] sparse_region, Tensor? touched) -> ()");
  m.def("adam_step(Tensor(a!) p, Tensor(e!) g, Tensor(b!) m, Tensor(c!) v, Tensor(d!)? p_bf16, int[] seg_end, float[] seg_lr, int step, float beta1, float beta2, float eps, "
        "Tensor? gnorm_sq, float max_norm, Tensor? dev_sched, int[] sparse_region, Tensor? touched) -> ()");
  m.def("step_advance(Tensor(a!)? rng_state, int offset_stride, Tensor(b!) step_counter, float[] base_lr, int warmup_iters, float warmup_factor, int[] decay_iters, "
        "float lr_decay, float beta1, float beta2, Tensor(c!) dev_sched) -> ()");
  m.def("encoder_layer_fwd(Tensor x, Tensor allow, Tensor[] params, int batch, int heads, float scale, float p_attn, float p_hid, int[] seeds, float eps1, "
        "float eps2) -> Tensor[]");
  m.def("encoder_layer_bwd(Tensor dy, Tensor[] saved, Tensor allow, Tensor[] params, Tensor(a!)[] grads, int batch, int heads, float scale, float p_attn, "
        "float p_hid, int[] seeds, bool need_dx, bool accumulate) -> Tensor");
  m.def("encoder_layer_bwd_nowgrad(Tensor dy, Tensor[] saved, Tensor allow, Tensor[] params, Tensor(a!)[] grads, int batch, int heads, float scale, float p_attn, "
        "float p_hid, int[] seeds, bool need_dx, bool accumulate) -> Tensor[]");
  m.def("wgrad_grouped(Tensor[] dys, Tensor[] xs, Tensor(a!)[] dws, Tensor(b!)[] dbs, bool accumulate) -> ()");
  m.def("answer_sample(Tensor meta, Tensor seq_len, Tensor seq_grp, Tensor step0_idx, Tensor step0_val, Tensor grp_idx, Tensor grp_off, Tensor grp_extra, "
        "int bos, int key, Tensor? step_dev, int step, Tensor? force_choice, Tensor(a!) targets, Tensor(b!) prev_inds, Tensor(c!) loss_mask, "
        "Tensor(d!) acc_mask, Tensor(e!) choice) -> ()");
  m.def("answer_sample_notargets(Tensor meta, Tensor seq_len, Tensor seq_grp, Tensor step0_idx, Tensor step0_val, Tensor grp_idx, Tensor grp_off, Tensor grp_extra, "
        "int width, int bos, int key, Tensor? step_dev, int step, Tensor? force_choice, Tensor(b!) prev_inds, Tensor(c!) loss_mask, Tensor(d!) acc_mask, "
        "Tensor(e!) choice) -> ()");
  m.def("bce_loss_table(Tensor fixed, Tensor ocr, Tensor[] table, Tensor choice, Tensor loss_mask, float grad_scale, Tensor? global_count, bool want_grads, "
        "Tensor(a!)? pred) -> (Tensor, Tensor, Tensor)");
  m.def("score_answers(Tensor pred, Tensor[] table, Tensor vocab_cp, Tensor vocab_len, int eos, Tensor(a!) scores, Tensor(b!) flags, Tensor(c!)? totals) -> ()");
  m.def("ragged_expand(Tensor counts, int n_max, Tensor[] srcs, Tensor(a!)[] dsts, int[] col0, int[] normalize, int[] zero_upto, Tensor(b!)? mask, float eps) -> ()");
  m.def("phoc_from_text(Tensor text, Tensor text_len, Tensor? counts, int batch, int n_max, Tensor(a!) dst, int col0, bool normalize, float eps) -> ()");
  m.def("answer_table_from_text(Tensor answer_text, Tensor answer_len, Tensor ocr_text, Tensor ocr_len, Tensor vocab_cp, Tensor vocab_len, Tensor slots, int unk, "
        "int eos, int max_match_num, Tensor(a!)[] out) -> ()");
  m.def("answer_status_fold(Tensor status, Tensor? step_dev, int step, Tensor(a!) state) -> ()");
  m.def("wordpiece_from_text(Tensor text, Tensor text_len, Tensor vocab_cp, Tensor vocab_len, Tensor slots, int unk, int cls, int sep, Tensor(a!) indices, "
        "Tensor(b!) mask, Tensor(c!) count) -> ()");
  m.def("fasttext_from_text(Tensor text, Tensor text_len, Tensor? counts, int batch, int n_max, Tensor matrix, Tensor index_cp, Tensor index_len, Tensor slots, "
        "int minn, int maxn, int bucket, int nwords, int eos, Tensor(a!) dst, int col0, bool normalize, float eps) -> ()");
  m.def("score_table_from_text(Tensor answer_text, Tensor answer_len, Tensor ocr_text, Tensor ocr_len, Tensor ocr_count, Tensor(a!)[] out) -> ()");
  m.def("eval_beams(Tensor seqs, Tensor cum, Tensor[] table, Tensor vocab_cp, Tensor vocab_len, int eos, int K, int skip, Tensor(a!)[] out, Tensor(b!)? totals) -> ()");
  m.def("text_from_utf8(Tensor raw, Tensor raw_off, int L, int mode, Tensor(a!) text, Tensor(b!) text_len, Tensor(c!) status) -> ()");
  m.def("text_from_utf8_unicode(Tensor raw, Tensor raw_off, int L, int mode, Tensor block, Tensor rec, Tensor pool, Tensor(a!) text, Tensor(b!) text_len, "
        "Tensor(c!) status) -> ()");
  m.def("aux_pair_loss(Tensor o, Tensor d, Tensor w, Tensor bias, Tensor codes, Tensor valid, int fusion) -> (Tensor, Tensor)");
  m.def("aux_pair_loss_bwd(Tensor? grad_out, Tensor count, Tensor o, Tensor d, Tensor w, Tensor bias, Tensor codes, Tensor valid, Tensor(a!) dw, Tensor(b!) dbias, int fusion, "
        "bool accumulate) -> (Tensor, Tensor)");
  m.def("relation_codes_from_boxes(Tensor obj_boxes, Tensor? ocr_boxes, float distance_threshold) -> Tensor");
  m.def("aux_targets(Tensor? rel, Tensor obj_mask, Tensor ocr_mask) -> (Tensor, Tensor)");
  m.def("aux_pair_stats(Tensor o, Tensor d, Tensor w, Tensor bias, Tensor codes, Tensor valid, int fusion, Tensor(a!) confusion, Tensor(b!) fired, bool accumulate) -> ()");
  m.def("question_from_utf8(Tensor raw, Tensor raw_off, int Lq, Tensor block, Tensor rec, Tensor pool, Tensor(a!) question_text, Tensor(b!) question_text_len, "
        "Tensor(c!) status) -> ()");
}

TORCH_LIBRARY_IMPL(sam_hip, CompositeExplicitAutograd, m) {      // no tensor arguments to dispatch on
  m.impl("set_ln_defer", set_ln_defer);
  m.impl("ln_finalize_flush", ln_finalize_flush);
  m.impl("ln_finalize_clear", ln_finalize_clear);
}

TORCH_LIBRARY_IMPL(sam_hip, CUDA, m) {      // (the ROCm backend registers under the CUDA dispatch key)
  m.impl("linear", linear_op);
  m.impl("spatial_attn_fwd", attn_fwd);
  m.impl("spatial_attn_bwd", attn_bwd);
  m.impl("spatial_attn_fwd_train", attn_fwd_train);
  m.impl("spatial_attn_bwd_fused", attn_bwd_fused);
  m.impl("layernorm_fwd", layernorm_fwd_op);
  m.impl("layernorm_bwd", layernorm_bwd_op);
  m.impl("encoder_layer_fwd", encoder_layer_fwd);
  m.impl("encoder_layer_bwd", encoder_layer_bwd);
  m.impl("encoder_layer_bwd_nowgrad", encoder_layer_bwd_nowgrad);
  m.impl("wgrad_grouped", wgrad_grouped_op);
  m.impl("pack_masks", pack_masks);
  m.impl("mask_bits_prefix_lm", mask_bits_prefix_lm);
  m.impl("mask_bits_from_additive", mask_bits_from_additive);
  m.impl("pack_relations", pack_relations);
  m.impl("pack_relations_bhnn", pack_relations_bhnn);
  m.impl("ptr_scores", ptr_scores_fwd);
  m.impl("ptr_scores_bwd", ptr_scores_bwd);
  m.impl("bce_loss", bce_loss);
  m.impl("sumsq", sumsq);
  m.impl("adam_step", adam_step);
  m.impl("step_advance", step_advance);
  m.impl("answer_sample", answer_sample);
  m.impl("answer_sample_notargets", answer_sample_notargets);
  m.impl("bce_loss_table", bce_loss_table);
  m.impl("score_answers", score_answers);
  m.impl("ragged_expand", ragged_expand);
  m.impl("phoc_from_text", phoc_from_text);
  m.impl("answer_table_from_text", answer_table_from_text);
  m.impl("answer_status_fold", answer_status_fold);
  m.impl("wordpiece_from_text", wordpiece_from_text);
  m.impl("fasttext_from_text", fasttext_from_text);
  m.impl("score_table_from_text", score_table_from_text);
  m.impl("eval_beams", eval_beams);
  m.impl("text_from_utf8", text_from_utf8);
  m.impl("text_from_utf8_unicode", text_from_utf8_unicode);
  m.impl("question_from_utf8", question_from_utf8);
  m.impl("aux_pair_loss", aux_pair_loss);
  m.impl("aux_pair_loss_bwd", aux_pair_loss_bwd);
  m.impl("relation_codes_from_boxes", relation_codes_from_boxes);
  m.impl("aux_targets", aux_targets);
  m.impl("aux_pair_stats", aux_pair_stats);
}
