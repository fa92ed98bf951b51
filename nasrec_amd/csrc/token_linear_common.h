// The large-batch token-axis kernels, everything but the matrix-core product: token_linear_body (forward product and input gradient)
// and token_dw_body (weight gradient), each entered once per product policy — token_linear.hip (fp32 products; the work mapping is
// described there, with the eligibility rules and the launch geometry) and token_linear_bf16.hip (bf16 products: token_linear at
// NASREC_PRECISION_MEDIUM, token_dw at _HIGH / _MEDIUM).  One eligibility rule, one launch geometry, one LDS budget for both.
#pragma once
#include <type_traits>

#include "gemm_tile.h"

#define TL_WAVES 16
#define TL_CHUNK 8        // k-steps (of 4 k) loaded before their MFMAs
#define TL_MAX_LDS 147456  // bytes of staged weights per workgroup (one 16-wave workgroup per CU; 160 KB LDS)
#define TL_BIAS_FLOATS 80  // the row biases sit in front of the weights (M <= 80)

// rows of the staged weight image for RB row blocks of 16: 16 / 48 / 80, so that the four k-groups of an MFMA operand read land on
// disjoint banks
constexpr int tl_pad(int rb) { return rb == 1 ? 16 : (rb <= 3 ? 48 : 80); }

#define TDW_WAVES 16

// token_linear_bf16.hip: the same launches with the geometry launch_token_linear / launch_token_dw worked out
void launch_token_linear_bf16(hipStream_t st, const nasrec_gemm_desc_t* d, int rb, int grid, int wgs, size_t lds);
void launch_token_dw_bf16(hipStream_t st, const nasrec_gemm_desc_t* d, int rb, int cb, int grid, int Mmax, int Nmax);

// a runtime block count 1..5 as a compile-time constant: f(std::integral_constant<int, n>)
template <class F>
static inline void tl_blocks(int n, F&& f) {
  switch (n) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    default: f(std::integral_constant<int, 5>{}); break;
  }
}

template <auto Kernel, class... Args>
static inline void tl_launch(hipStream_t st, int grid, int threads, size_t lds, const Args&... args) {
  static unsigned long long big_lds_devices = 0;  // more than the default 64 KB of dynamic LDS must be requested once per kernel and device
  if (lds > 65536 && nasrec_lds_attr_needed(big_lds_devices))
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, TL_MAX_LDS);
  hipLaunchKernelGGL(Kernel, dim3(grid), dim3(threads), lds, st, args...);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// token_linear_kernel / token_linear_bf16_kernel.  The policy P is the product of one chunk (TL_CHUNK k-steps of one sample):
//   P::slot_t, P::slot(w)               what a 32-bit slot of the staged weight image holds
//   P::chunk<RB, MP>(wchunk, live, xv, acc)
//                                       acc[rb] += W[rb-th row block, the chunk's k] x[the chunk's k]: wchunk = the lane's slot (k-group
//                                       g, row e) of the chunk's first k-step, k-step u at + 4 u MP, row block rb at + 16 rb; live >= 1
//                                       = the chunk's k-steps inside the segment (LDS rows beyond them are NOT zero); xv[u] = the lane's
//                                       element of the 64 floats x[b][4 u .. 4 u + 3][0 .. 15], zero beyond the segment's K
// ---------------------------------------------------------------------------------------------------------------------------------
template <int AM, int RB, class P>
__device__ __forceinline__ void token_linear_body(const nasrec_gemm_desc_t& d, int wgs) {
  typedef typename P::slot_t slot_t;
  extern __shared__ __attribute__((aligned(16))) float lds_all[];
  float* const Bl = lds_all;                                                 // row biases (or zeros)
  slot_t* const Wl = reinterpret_cast<slot_t*>(lds_all + TL_BIAS_FLOATS);  // weights
  constexpr int MP = tl_pad(RB);
  // (the wave index as a SCALAR: the buffer resources below are built from it, and a resource the compiler takes for lane-dependent is
  // wrapped in a readfirstlane loop around every load)
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int z = d.zmode ? (int)blockIdx.x / wgs : 0;
  const int wg = (int)blockIdx.x - z * wgs;
  const int s_lo = d.zmode ? z : 0, s_hi = d.zmode ? z + 1 : d.nseg;
  const nasrec_gemm_seg_t& s0 = d.seg[s_lo];
  const int M = s0.M, Bs = s0.N >> 4;

  // ---- weights -> LDS, k-major, zero-padded to MP rows and to whole k-steps ---------------------------------------------------
  int kbase = 0;
  for (int s = s_lo; s < s_hi; ++s) {
    const nasrec_gemm_seg_t& sg = d.seg[s];
    if (!sg.A || sg.K <= 0) continue;
    const int Kp = (sg.K + 3) & ~3;
    const int total = Kp * MP;
    for (int idx = tid; idx < total; idx += 1024) {
      int i, k;
      if (AM == NASREC_AM_KC) {  // A(i,k) = a[i * lda + k]: k fastest
        i = idx / Kp;
        k = idx - i * Kp;
      } else {                   // A(i,k) = a[k * lda + i]: i fastest
        k = idx / MP;
        i = idx - k * MP;
      }
      float v = 0.f;
      if (i < M && k < sg.K) v = AM == NASREC_AM_KC ? sg.A[(long)i * sg.lda + k] : sg.A[(long)k * sg.lda + i];
      Wl[(kbase + k) * MP + i] = P::slot(v);
    }
    kbase += Kp;
  }
  // the row biases go through LDS too: an LDS read in the epilogue is counted by lgkmcnt, a global one by vmcnt — behind the stores
  if (tid < TL_BIAS_FLOATS) Bl[tid] = (d.bias && d.bias_on_rows && tid < M) ? d.bias[tid] : 0.f;
  __syncthreads();

  const int g = lane >> 4, e = lane & 15;
  const bool acc_c = d.zmode ? s0.accumulate != 0 : d.beta != 0;
  // what the epilogue needs of the descriptor, once per workgroup (registers)
  const bool has_bias = d.bias != nullptr, bias_rows = d.bias_on_rows != 0, mask_rows = d.mask_on_rows != 0;
  const int dims = d.dims_in_use, act = d.act;
  float* const zbase = d.save_z;
  for (int b = wg * TL_WAVES + wave; b < Bs; b += wgs * TL_WAVES) {
    f32x4 acc[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) acc[rb] = (f32x4){0.f, 0.f, 0.f, 0.f};
    int kb = 0;
    for (int s = s_lo; s < s_hi; ++s) {
      const nasrec_gemm_seg_t& sg = d.seg[s];
      if (!sg.A || sg.K <= 0) continue;
      const int K4 = (sg.K + 3) >> 2;
      const __amdgpu_buffer_rsrc_t rs =
          __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(sg.B) + (long)b * sg.ldb, 0, sg.K * 64, 0x00020000);
      for (int c0 = 0; c0 < K4; c0 += TL_CHUNK) {
        float xv[TL_CHUNK];
#pragma unroll
        for (int u = 0; u < TL_CHUNK; ++u)  // beyond the sample's K rows: zeros (hardware range check)
          xv[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, (c0 + u) * 256 + lane * 4, 0, 0));
        P::template chunk<RB, MP>(Wl + (kb + 4 * c0 + g) * MP + e, K4 - c0, xv, acc);
      }
      kb += 4 * K4;
    }
    // ---- epilogue == epilogue_store<NASREC_CM_TOKJ> (gemm_tile.h); D: row = 4 * (lane >> 4) + reg, column = lane & 15 ---------
    // Everything the sample's elements READ comes first (the accumulation target: 4 RB loads in flight; the row biases wait in LDS), ONE
    // wait, then nothing but arithmetic and stores: vmcnt counts loads and stores in one in-order queue, so a load behind a store —
    // element by element: bias, C, store, bias, C, store — makes the wave wait for the store's acknowledgement each time.
    float* C = s0.C + (long)b * s0.ldc + e;
    float* Z = zbase ? zbase + (long)b * s0.ldc + e : nullptr;
    float cv[RB][4];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int r = 0; r < 4; ++r) cv[rb][r] = 0.f;
    if (acc_c) {
#pragma unroll
      for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int r = 0; r < 4; ++r) cv[rb][r] = C[min(rb * 16 + 4 * g + r, M - 1) * 16];  // (clamped: rows >= M are never stored)
    }
    const float bcol = (has_bias && !bias_rows) ? d.bias[b * 16 + e] : 0.f;
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), spelled out: the compiler cannot count the conditional stores below
    const bool dead_col = dims >= 0 && !mask_rows && b * 16 + e >= dims;
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = rb * 16 + 4 * g + r;
        if (i >= M) continue;
        float v = acc[rb][r];
        if (has_bias) v += bias_rows ? Bl[i] : bcol;
        if (Z) Z[i * 16] = v;
        v = act_apply(v, act);
        if (dead_col || (dims >= 0 && mask_rows && i >= dims)) v = 0.f;
        if (acc_c) v += cv[rb][r];
        C[i * 16] = v;
      }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// token_dw_kernel / token_dw_bf16_kernel.  The policy P is the product of one (row block, column block) pair of one sample:
//   P::frag_t, P::frag(v)     the MFMA operand made of a lane's 16-byte load v (row lane & 15 of the block, e = 4 g .. 4 g + 3)
//   P::STEPS, P::mma(st, a, x, acc)
//                             acc + step st of a x^T over those four e; for one acc the steps run in ascending order
// The operands go to the policy BY VALUE, a block at a time, and every fragment is made after the last load is issued.  The 4-5 x 4-5
// block instantiations sit at the 128 VGPRs of 1024 threads, and what the compiler makes of them follows the form: with the arrays handed
// over by reference (one product(a, x, acc) call) they spill 36 .. 216 bytes more than with the product written in place, with each
// fragment made where its load is the bf16 x 3 product of 4 x 5 blocks ran 15 % slower (profiles/token_linear_shared_body.txt).
// ---------------------------------------------------------------------------------------------------------------------------------
template <int RB, int CB, class P>
__device__ __forceinline__ void token_dw_body(const nasrec_gemm_desc_t& d, int Mmax, int Nmax) {
  __shared__ __attribute__((aligned(16))) float red[4 * RB * CB * 4 * 64];
  // (the wave index as a SCALAR, as in token_linear_body)
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int S = d.splitk;
  const int z = (int)blockIdx.x / S, ks = (int)blockIdx.x - z * S;
  const nasrec_gemm_seg_t& sg = d.seg[z];
  const int M = sg.M, N = sg.N, Nr = sg.ones_col ? N - 1 : N;
  const int Bs = sg.K >> 4;
  const int i16 = lane & 15, g = lane >> 4;
  f32x4 acc[RB][CB];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb)
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) acc[rb][cb] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int ones_cb = sg.ones_col ? (N - 1) >> 4 : -1, ones_j = (N - 1) & 15;
  if (sg.A) {
    for (int b = ks * TDW_WAVES + wave; b < Bs; b += S * TDW_WAVES) {
      const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(sg.A) + (long)b * sg.lda, 0, M * 64, 0x00020000);
      const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(sg.B) + (long)b * sg.ldb, 0, Nr * 64, 0x00020000);
      f32x4 a[RB], x[CB];
#pragma unroll
      for (int rb = 0; rb < RB; ++rb)  // rows beyond M: zeros (range check)
        a[rb] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ra, ((rb * 16 + i16) * 16 + 4 * g) * 4, 0, 0));
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) {
        x[cb] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rx, ((cb * 16 + i16) * 16 + 4 * g) * 4, 0, 0));
        if (cb == ones_cb && i16 == ones_j) x[cb] = (f32x4){1.f, 1.f, 1.f, 1.f};
      }
      typename P::frag_t af[RB], xf[CB];
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) af[rb] = P::frag(a[rb]);
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) xf[cb] = P::frag(x[cb]);
#pragma unroll
      for (int st = 0; st < P::STEPS; ++st)
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
          for (int cb = 0; cb < CB; ++cb) acc[rb][cb] = P::mma(st, af[rb], xf[cb], acc[rb][cb]);
    }
  }
  // ---- the workgroup's 16 partial sums: four LDS accumulators, wave w joins accumulator w % 4 in round w / 4 (fixed order) ------
  for (int round = 0; round < TDW_WAVES / 4; ++round) {
    if ((wave >> 2) == round) {
      float* mine = red + (wave & 3) * (RB * CB * 256);
#pragma unroll
      for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float* p = &mine[((rb * CB + cb) * 4 + r) * 64 + lane];
            *p = round == 0 ? acc[rb][cb][r] : *p + acc[rb][cb][r];
          }
    }
    __syncthreads();
  }
  // ---- slab of this split: D row = 4 * (lane >> 4) + reg, column = lane & 15 -----------------------------------------------------
  const int Mv = (sg.Mvalid > 0 && sg.Mvalid < M) ? sg.Mvalid : M;
  float* slab = d.workspace + ((long)(z * S + ks)) * Mmax * Nmax;
  for (int idx = tid; idx < RB * CB * 256; idx += 64 * TDW_WAVES) {
    const int blk = idx >> 8, r = (idx >> 6) & 3, l = idx & 63;
    const int rb = blk / CB, cb = blk - rb * CB;
    const int i = rb * 16 + 4 * (l >> 4) + r, j = cb * 16 + (l & 15);
    const int o = (blk * 4 + r) * 64 + l;
    const float v = (red[o] + red[RB * CB * 256 + o]) + (red[2 * RB * CB * 256 + o] + red[3 * RB * CB * 256 + o]);
    if (i < M && j < N) slab[(long)i * N + j] = i < Mv ? v : 0.f;
  }
}
