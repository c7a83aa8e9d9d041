// How well the spatial auxiliary heads classify (include/sam_hip_aux_stats.h): the 13 x 13 confusion counts of the argmax rule and
// the 13 x 12 fired-channel counts over the valid pairs, from O, D, W, bias, the relation codes and the valid flags, with no [B, n, n, 12] tensor in memory.
//
//   counting  sam_aux_pair_loss_fwd's tile (64 j per wave with D[j] in registers, 16 rows i per block, O[i] / W / bias wave-uniform) and aux_pair.h's
//             pair_scores: the scores sam_aux_pair_fwd stores.  In place of the BCE sum a lane derives (c, p, f) of its pair and adds into its WAVE's LDS
//             table of 325 u32 (169 confusion cells, then 156 fired cells): one integer add for the confusion cell, one per fired channel.  The block's
//             four tables are summed in wave order -> u32 block partials in the workspace, cell-major ([325][blocks]: the finishing reads are contiguous).
//   finish    one block per cell: 256 threads stride over the block partials in int64, a fixed butterfly + the 4 waves in order; stores, or adds to what the
//             destination holds.
//
// No global atomics, every grid sized from the shape alone; the sums are integers, so the order of the LDS adds cannot show: bit-identical from run to run.
#include "aux_pair.h"
#include "sam_hip_aux_stats.h"

namespace {

using namespace auxp;

constexpr int ST_K = AUX_R + 1;                       // classes: 0 none, 1..12
constexpr int ST_CONF = ST_K * ST_K;                  // 169
constexpr int ST_CELLS = ST_CONF + ST_K * AUX_R;      // 325

template <bool MUL>
__global__ __launch_bounds__(256) void aux_pair_stats_kernel(const float* __restrict__ O, const float* __restrict__ D, const float* __restrict__ W,
                                                             const float* __restrict__ bias, const uint8_t* __restrict__ codes,
                                                             const uint8_t* __restrict__ valid, int n, int64_t nblk, uint32_t* __restrict__ part) {
  __shared__ uint32_t tabs[FWD_WAVES][ST_CELLS];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.z, j = blockIdx.x * FWD_JT + lane;
  const int64_t sb = (int64_t)b * n;
  uint32_t* tab = tabs[wave];
  for (int k = lane; k < ST_CELLS; k += 64) tab[k] = 0;
  const bool vj = j < n && valid[sb + j] != 0;
  float d[AUX_C];
  load_d_row(D, sb + j, vj, d);                           // (a row that is not valid is never read: it may hold anything)
  __syncthreads();
  const int i_base = blockIdx.y * (FWD_WAVES * FWD_RW) + wave * FWD_RW;
  for (int u = 0; u < FWD_RW; ++u) {
    const int i = i_base + u;
    if (i >= n) break;
    if (valid[sb + i] == 0) continue;                     // wave-uniform
    float s[AUX_R];
    pair_scores<MUL>(O + (sb + i) * AUX_C, d, W, bias, s);
    if (vj) {
      const int code = codes[(sb + i) * n + j];
      const int c = code <= AUX_R ? code : 0;             // (a code above 12 is an all-zero target in the loss: class 0)
      float best = 0.f;
      int p = 0;
#pragma unroll
      for (int r = 0; r < AUX_R; ++r)
        if (s[r] > best) { best = s[r]; p = r + 1; }      // first maximum wins; a NaN compares false
      atomicAdd(&tab[c * ST_K + p], 1u);
      uint32_t* frow = tab + ST_CONF + c * AUX_R;
#pragma unroll
      for (int r = 0; r < AUX_R; ++r)
        if (s[r] > 0.f) atomicAdd(&frow[r], 1u);
    }
  }
  __syncthreads();
  const int64_t blk = ((int64_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
  for (int k = threadIdx.x; k < ST_CELLS; k += 256) part[(int64_t)k * nblk + blk] = ((tabs[0][k] + tabs[1][k]) + tabs[2][k]) + tabs[3][k];
}

// one block per cell: 256 threads stride over the cell's block partials, then a fixed butterfly + the 4 waves in order
__global__ __launch_bounds__(256) void aux_stats_finish_kernel(const uint32_t* __restrict__ part, int64_t nblk, int64_t* __restrict__ confusion,
                                                               int64_t* __restrict__ fired, int accumulate) {
  __shared__ unsigned long long sc[4];
  const int cell = blockIdx.x, t = threadIdx.x;
  const uint32_t* src = part + (int64_t)cell * nblk;
  unsigned long long c = 0;
  for (int64_t k = t; k < nblk; k += 256) c += src[k];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
  if ((t & 63) == 0) sc[t >> 6] = c;
  __syncthreads();
  if (t == 0) {
    const int64_t v = (int64_t)(((sc[0] + sc[1]) + sc[2]) + sc[3]);
    int64_t* dst = cell < ST_CONF ? confusion + cell : fired + (cell - ST_CONF);
    *dst = accumulate ? *dst + v : v;
  }
}

inline int64_t stats_blocks(int B, int n) { return (int64_t)B * cdiv(n, FWD_JT) * cdiv(n, FWD_WAVES * FWD_RW); }

}  // namespace

extern "C" int sam_aux_pair_stats_ws_bytes(int B, int n, int64_t* bytes) {
  SAM_REQUIRE(bytes, "sam_aux_pair_stats_ws_bytes: null pointer");
  SAM_REQUIRE(B > 0 && n > 0, "sam_aux_pair_stats_ws_bytes: empty shape (B=%d n=%d)", B, n);
  SAM_REQUIRE(B <= 65535, "sam_aux_pair_stats_ws_bytes: B=%d exceeds the grid", B);
  *bytes = stats_blocks(B, n) * (int64_t)(ST_CELLS * sizeof(uint32_t));
  return SAM_OK;
}

extern "C" int sam_aux_pair_stats(const float* O, const float* D, const float* W, const float* bias, const uint8_t* codes, const uint8_t* valid, int B, int n,
                                  int fusion, int64_t* confusion, int64_t* fired, int accumulate, void* ws, int64_t ws_bytes, void* stream) {
  SAM_REQUIRE(O && D && W && bias && codes && valid && confusion && fired && ws, "sam_aux_pair_stats: null pointer");
  SAM_REQUIRE(B > 0 && n > 0, "sam_aux_pair_stats: empty shape (B=%d n=%d)", B, n);
  SAM_REQUIRE(fusion == SAM_AUX_MUL || fusion == SAM_AUX_ADD, "sam_aux_pair_stats: unknown fusion %d", fusion);
  SAM_REQUIRE((uintptr_t)O % 16 == 0 && (uintptr_t)D % 16 == 0 && (uintptr_t)ws % 16 == 0, "sam_aux_pair_stats: O / D / ws must be 16-byte aligned");
  SAM_REQUIRE((uintptr_t)confusion % 8 == 0 && (uintptr_t)fired % 8 == 0, "sam_aux_pair_stats: confusion / fired must be 8-byte aligned");
  SAM_REQUIRE(B <= 65535, "sam_aux_pair_stats: B=%d exceeds the grid", B);
  const int64_t nblk = stats_blocks(B, n), need = nblk * (int64_t)(ST_CELLS * sizeof(uint32_t));
  SAM_REQUIRE(ws_bytes >= need, "sam_aux_pair_stats: workspace of %lld bytes, need %lld", (long long)ws_bytes, (long long)need);
  uint32_t* part = static_cast<uint32_t*>(ws);
  const dim3 grid(cdiv(n, FWD_JT), cdiv(n, FWD_WAVES * FWD_RW), B);
  hipStream_t st = (hipStream_t)stream;
  if (fusion == SAM_AUX_MUL)
    aux_pair_stats_kernel<true><<<grid, dim3(256), 0, st>>>(O, D, W, bias, codes, valid, n, nblk, part);
  else
    aux_pair_stats_kernel<false><<<grid, dim3(256), 0, st>>>(O, D, W, bias, codes, valid, n, nblk, part);
  aux_stats_finish_kernel<<<dim3(ST_CELLS), dim3(256), 0, st>>>(part, nblk, confusion, fired, accumulate);
  SAM_LAUNCH_CHECK();
  return SAM_OK;
}
