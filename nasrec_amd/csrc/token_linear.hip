// Token-axis Linear at large batch (modules.py:222-234, 358-361, 648-650): out[b, i, e] = sum_k A(i, k) x[b, k, e] over the 16 embedding
// columns e of every sample b — the forward product (A = W, binding KC / TOKR / TOKJ, K-concatenated input segments) and the input
// gradient (A = W^T, binding RC / TOKR / TOKJ, a batch of independent problems).  M = output tokens <= 80, K = input tokens, and
// B * 16 columns: a memory-bound stream (per sample (K + M) * 64 bytes) with as many flops as the fp32 MFMA does in the same time.
//
// The general GEMM template tiles this as 64 x 64 (i, (b, e)) blocks: every workgroup re-reads the weights from L2, stages 18 KB
// through LDS with dword loads and runs two k-tiles — 52-78 us per launch at B = 4096 whatever its size, 3-7x its HBM bytes.
// Here the roles are turned round:
//   * the WEIGHTS live in LDS for the whole workgroup (k-major [k][MP], MP = 16 / 48 / 80 so that the four k-groups of an MFMA
//     operand read land on disjoint banks), staged once per workgroup of 16 wavefronts;
//   * a wavefront owns one SAMPLE at a time: x[b] is a contiguous [K, 16] block, and the B operand of v_mfma_f32_16x16x4_f32
//     (lane = (k-group g, column e)) for k-step kk is exactly the 64 consecutive floats x[b][4 kk .. 4 kk + 3][0 .. 15] —
//     one fully coalesced 256-byte load per MFMA k-step, straight to registers (buffer loads bounded by the sample's K * 64
//     bytes: the ragged last k-step reads zeros), no LDS round trip for the streamed operand;
//   * the A operand of each MFMA is one ds_read_b32; the accumulators D[i = 4 g + r][e] of the M / 16 row blocks go straight
//     to out[b][i][e] (64-byte segments) through the same epilogue as the general kernel (bias on rows, activation, prefix
//     mask on rows, saved pre-activation, accumulation).
// Exact fp32 FMA chains; the k order inside a sample is the natural one, so results do not depend on the launch geometry.
// (This file holds the fp32 products, the eligibility rules and the launch geometry; the kernels' bodies are in token_linear_common.h,
// shared with token_linear_bf16.hip, which a descriptor that permits bf16 products — MEDIUM for the forward / input-gradient kernel,
// HIGH or MEDIUM for the weight gradient — runs on the same eligibility rule, geometry and LDS image size.)
#include "token_linear_common.h"

struct TlF32 {
  typedef float slot_t;
  static __device__ __forceinline__ float slot(float w) { return w; }
  template <int RB, int MP>
  static __device__ __forceinline__ void chunk(const float* wchunk, int live, float (&xv)[TL_CHUNK], f32x4 (&acc)[RB]) {
    // Every load of the chunk is issued before its first product, and the first k-step's LDS reads (live >= 1) go out before the wave
    // waits for them: the empty statement ties the loads to this place.  Left alone, the compiler sinks a load whose only use sits in
    // the next (uniform) branch below into that branch, behind MFMAs that wait for the others — a second memory round trip per chunk
    // (measured: 19.4 us with all loads up front, 22.0 us with one sunk, B = 4096, M = 45, K = 26 + 72 + 72).
    float w0[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) w0[rb] = wchunk[rb * 16];
#pragma unroll
    for (int u = 0; u < TL_CHUNK; ++u) asm volatile("" : "+v"(xv[u]));
#pragma unroll
    for (int u = 0; u < TL_CHUNK; ++u) {
      if (u < live) {  // (uniform) LDS rows beyond the staged weights are not zero
        const float* wrow = wchunk + 4 * u * MP;
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
          acc[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(u == 0 ? w0[rb] : wrow[rb * 16], xv[u], acc[rb], 0, 0, 0);
      }
    }
  }
};

template <int AM, int RB>
__global__ __launch_bounds__(1024) void token_linear_kernel(const nasrec_gemm_desc_t d, int wgs) {
  token_linear_body<AM, RB, TlF32>(d, wgs);
}

// a problem's staged k: its live segments (all of the descriptor's, K-concatenated, or the p-th of a zmode batch), each padded to whole
// k-steps of 4
static long tl_staged_k(const nasrec_gemm_desc_t* d, int p) {
  long kp = 0;
  for (int q = d->zmode ? p : 0; q < (d->zmode ? p + 1 : d->nseg); ++q)
    if (d->seg[q].A && d->seg[q].K > 0) kp += (d->seg[q].K + 3) & ~3;
  return kp;
}

// Which launches take this path (the general template keeps everything else: small batches, ReLU-mask operands, split-K, ...)
bool token_linear_eligible(const nasrec_gemm_desc_t* d) {
  if (d->cmode != NASREC_CM_TOKJ || d->bmode != NASREC_AM_TOKR) return false;
  if (d->amode != NASREC_AM_KC && d->amode != NASREC_AM_RC) return false;
  if (d->splitk > 1 || d->pre_add || d->save_act || d->mul_nseg > 0) return false;
  const int nprob = d->zmode ? d->nseg : 1;
  for (int p = 0; p < nprob; ++p) {
    const nasrec_gemm_seg_t& s0 = d->seg[p];
    if (s0.M < 1 || s0.M > 80 || (s0.N & 15) || (s0.N >> 4) < 1024 || s0.ones_col) return false;
    if (s0.Mvalid > 0 && s0.Mvalid < s0.M) return false;
    for (int q = d->zmode ? p : 0; q < (d->zmode ? p + 1 : d->nseg); ++q) {
      const nasrec_gemm_seg_t& s = d->seg[q];
      if (s.Aaux || s.Baux) return false;
      if (!d->zmode && (s.M != s0.M || s.N != s0.N)) return false;
      if ((long)s.K * 64 > 0x7fffffffL) return false;
    }
    if (tl_staged_k(d, p) * tl_pad((s0.M + 15) / 16) * 4 + TL_BIAS_FLOATS * 4 > TL_MAX_LDS) return false;
    if (d->zmode && p > 0 && (s0.N != d->seg[0].N || (s0.M + 15) / 16 != (d->seg[0].M + 15) / 16)) return false;  // one grid, one row-block count
  }
  return true;
}

int launch_token_linear(hipStream_t st, const nasrec_gemm_desc_t* d) {
  const int nprob = d->zmode ? d->nseg : 1;
  const int Bs = d->seg[0].N >> 4;
  const int rb = (d->seg[0].M + 15) / 16;
  long kp_max = 0;
  for (int p = 0; p < nprob; ++p) kp_max = std::max(kp_max, tl_staged_k(d, p));
  // a wavefront per sample, 16 per workgroup: the chip holds 256-512 workgroups; with several problems each one gets fewer
  // workgroups (more samples per wavefront, the weights are staged less often)
  int wgs = 256 / nprob;
  if (wgs < 64) wgs = 64;
  const int need = (Bs + TL_WAVES - 1) / TL_WAVES;
  if (wgs > need) wgs = need;
  const size_t lds = (size_t)(kp_max > 0 ? kp_max : 4) * tl_pad(rb) * 4 + TL_BIAS_FLOATS * 4;
  if (d->precision == NASREC_PRECISION_MEDIUM)
    launch_token_linear_bf16(st, d, rb, wgs * nprob, wgs, lds);  // (token_linear_bf16.hip; HIGH stays here: DESIGN.md "Matmul precision")
  else
    tl_blocks(rb, [&](auto RB) {
      if (d->amode == NASREC_AM_KC)
        tl_launch<token_linear_kernel<NASREC_AM_KC, decltype(RB)::value>>(st, wgs * nprob, 1024, lds, *d, wgs);
      else
        tl_launch<token_linear_kernel<NASREC_AM_RC, decltype(RB)::value>>(st, wgs * nprob, 1024, lds, *d, wgs);
    });
  return nasrec_check_launch("token_linear");
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Token-axis weight gradient at large batch (binding TOKK / TOKK / PLAIN): dW[i, j] = sum_b sum_e dz[b, i, e] x[b, j, e]
// (+ the bias gradient as a virtual ones-column), a batch of independent problems, K = B * 16.
// Per sample the product is [M, 16] x [16, N]: with the MFMA's k index taken as e = 4 g + step (g = lane >> 4) a lane's four
// A values for the four k-steps are ONE 16-byte load of row i = lane & 15 (all 64 lanes together read a contiguous 1 KB block
// of 16 rows), likewise for B — RB + CB loads and 4 RB CB MFMAs per sample, nothing staged through LDS.  A wavefront sums its
// samples in registers, the 16 wavefronts of a workgroup are added in fixed order through LDS, every workgroup writes one split-K
// slab and the general second pass (gemm_splitk_epilogue: fixed-order sum over the S slabs, row mask, accumulation, bias column)
// finishes — desc.splitk = S workgroups per problem, chosen by the plan.
// ---------------------------------------------------------------------------------------------------------------------------------
struct TdwF32 {
  typedef f32x4 frag_t;
  static constexpr int STEPS = 4;
  static __device__ __forceinline__ f32x4 frag(const f32x4 v) { return v; }
  static __device__ __forceinline__ f32x4 mma(int st, const f32x4 a, const f32x4 x, const f32x4 acc) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a[st], x[st], acc, 0, 0, 0);
  }
};

template <int RB, int CB>
__global__ __launch_bounds__(64 * TDW_WAVES) void token_dw_kernel(const nasrec_gemm_desc_t d, int Mmax, int Nmax) {
  token_dw_body<RB, CB, TdwF32>(d, Mmax, Nmax);
}

bool token_dw_eligible(const nasrec_gemm_desc_t* d) {
  if (d->amode != NASREC_AM_TOKK || d->bmode != NASREC_AM_TOKK || d->cmode != NASREC_CM_PLAIN || !d->zmode) return false;
  if (d->splitk < 2 || !d->workspace) return false;
  for (int q = 0; q < d->nseg; ++q) {
    const nasrec_gemm_seg_t& s = d->seg[q];
    if (s.Aaux || s.Baux) return false;
    if (s.M < 1 || s.M > 80 || s.N < 1 || s.N > 80) return false;
    if ((s.K & 15) || (s.K >> 4) < 1024) return false;
  }
  return true;
}

// main pass only: the caller (launch_gemm) runs the split-K second pass as for every other split launch
int launch_token_dw(hipStream_t st, const nasrec_gemm_desc_t* d, int Mmax, int Nmax) {
  const int rb = (Mmax + 15) / 16, cb = (Nmax + 15) / 16;
  const int grid = d->nseg * d->splitk;
  if (d->precision != NASREC_PRECISION_HIGHEST)
    launch_token_dw_bf16(st, d, rb, cb, grid, Mmax, Nmax);  // (token_linear_bf16.hip)
  else
    tl_blocks(rb, [&](auto RB) {
      tl_blocks(cb, [&](auto CB) {
        tl_launch<token_dw_kernel<decltype(RB)::value, decltype(CB)::value>>(st, grid, 64 * TDW_WAVES, 0, *d, Mmax, Nmax);
      });
    });
  return 0;
}
