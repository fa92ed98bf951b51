// Large-batch token-axis Linear kernels with bf16 matrix-core products: the second body of NASREC_GEMM_ROUTE_TOKEN_LINEAR launches at
// nasrec_gemm_desc_t.precision = NASREC_PRECISION_MEDIUM and of NASREC_GEMM_ROUTE_TOKEN_DW launches at _HIGH / _MEDIUM (token_linear.hip
// is every other case).  Same eligibility rules, same work mapping, same launch geometry (token_linear_common.h).
//
// Memory is fp32 on both sides and the accumulators are fp32; what changes is what the matrix cores multiply.  With â = bf16(a),
// round to nearest even:
//   MEDIUM  acc += â b̂                                  (bf16 x bf16 is exact in fp32)
//   HIGH    a ~ a_hi + a_lo, a_hi = bf16(a), a_lo = bf16(a - a_hi); acc += a_lo b_hi, then a_hi b_lo, then a_hi b_hi: three MFMAs
//           in that fixed order (the lo x lo term, <= 2^-18 |a||b|, is dropped); a = dz, b = x
//
// token_linear_bf16_kernel (MEDIUM).  The fp32 body spends its time on v_mfma_f32_16x16x4_f32: eight of them (32 cycles each) per row
// block and TL_CHUNK of 32 k.  Here one v_mfma_f32_16x16x32_bf16 (16 cycles) takes their place:
//   * the streamed operand keeps its load pattern.  The eight 256-byte loads of a chunk give lane (g, e) the rows 4 u + g, u = 0..7,
//     of 32 consecutive k; four v_cvt_pk_bf16_f32 make them the lane's B fragment, MFMA k = 8 g + u  <->  chunk k = 4 u + g.  The
//     permutation is free as long as A agrees;
//   * the weights keep the fp32 body's LDS image — k-major [k][MP] 32-bit slots, zero-padded to whole k-steps of 4 — so the staging
//     needs exactly the bytes the shared eligibility rule budgets (TL_MAX_LDS), whatever the segments' K: a slot holds bf16(w) in its
//     low half, rounded ONCE per workgroup at staging.  A lane's A fragment is the same eight ds_read_b32 the fp32 body issues (slot
//     (4 u + g, i)), packed pairwise by four VALU ops;
//   * k-steps beyond a segment's K inside its last chunk are not staged: their slots are read at an address clamped into the
//     segment and masked to zero (uniform arithmetic, no branch), and the streamed side reads zeros there by the buffer range check.
// The k order inside a sample is fixed (segments in order, chunks ascending, the MFMA's own chain inside a chunk): the result of a
// descriptor does not depend on launch geometry or timing.  The epilogue is that of token_linear_kernel.
// A HIGH variant of this kernel (both halves of the slot, three MFMAs) was built and measured and is not here: DESIGN.md.
//
// token_dw_bf16_kernel (MEDIUM, HIGH).  A lane's 16-byte load holds e = 4 g .. 4 g + 3 of its row: the operand layout of the 16-deep
// v_mfma_f32_16x16x16_bf16 with k = e.  Per sample and (rb, cb) one MFMA (HIGH: three) instead of four fp32 ones; the virtual ones
// column stays exact (1.0 is a bf16 value, its lo part 0).  Per-wave accumulation, the fixed-order reduction over the 16 waves, the
// slab write and the general second pass are those of token_dw_kernel.
#include "token_linear_common.h"

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned tb_bits(__bf16 h) { return (unsigned)__builtin_bit_cast(unsigned short, h); }

// MEDIUM only (HIGH keeps token_linear_kernel: its three products per k did not pay on every measured launch — DESIGN.md)
template <int AM, int RB>
__global__ __launch_bounds__(1024) void token_linear_bf16_kernel(const nasrec_gemm_desc_t d, int wgs) {
  extern __shared__ __attribute__((aligned(16))) float lds_all[];
  float* const Bl = lds_all;                                                   // row biases (or zeros), fp32
  unsigned* const Wl = reinterpret_cast<unsigned*>(lds_all + TL_BIAS_FLOATS);  // weights: bf16(w) in the low half of a 32-bit slot
  constexpr int MP = TlPad<RB>::v;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int z = d.zmode ? (int)blockIdx.x / wgs : 0;
  const int wg = (int)blockIdx.x - z * wgs;
  const int s_lo = d.zmode ? z : 0, s_hi = d.zmode ? z + 1 : d.nseg;
  const nasrec_gemm_seg_t& s0 = d.seg[s_lo];
  const int M = s0.M, Bs = s0.N >> 4;

  // ---- weights -> LDS, k-major, zero-padded to MP rows and to whole k-steps (the fp32 body's image, converted) ----------------
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
      Wl[(kbase + k) * MP + i] = tb_bits((__bf16)v);
    }
    kbase += Kp;
  }
  if (tid < TL_BIAS_FLOATS) Bl[tid] = (d.bias && d.bias_on_rows && tid < M) ? d.bias[tid] : 0.f;
  __syncthreads();

  const int g = lane >> 4, e = lane & 15;
  const bool acc_c = d.zmode ? s0.accumulate != 0 : d.beta != 0;
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
        // The last chunk of a segment may hold k-steps beyond the staged weights: their LDS address is clamped into the segment and their
        // slots are masked to zero — all of it uniform (scalar) arithmetic and ONE straight-line body for full and partial chunks, so
        // that the loads of x and the LDS reads go out together: a branch between them puts an LDS round trip (two, with the reads the
        // compiler hoists above it) behind every load, which a launch of short segments out of the caches feels (measured: 7.1 us as
        // fp32, 7.7 us with the branch, B = 8192, M = 10, K = 10 + 10).
        const unsigned* const wchunk = Wl + (kb + 4 * c0 + g) * MP + e;
        const int live = K4 - c0;  // k-steps of this chunk inside the segment: >= 1
        int roff[TL_CHUNK];
        unsigned msk[TL_CHUNK / 2];  // of the packed pair (2 p, 2 p + 1)
#pragma unroll
        for (int u = 0; u < TL_CHUNK; ++u) roff[u] = 4 * min(u, live - 1) * MP;
#pragma unroll
        for (int p = 0; p < TL_CHUNK / 2; ++p) msk[p] = live >= 2 * p + 2 ? 0xffffffffu : (live == 2 * p + 1 ? 0xffffu : 0u);
        auto slots = [&](int rb, unsigned (&w)[TL_CHUNK]) {
#pragma unroll
          for (int u = 0; u < TL_CHUNK; ++u) w[u] = wchunk[roff[u] + rb * 16];
        };
        // The first row block's LDS reads go out BEFORE the wave waits for x: the empty statement ties the conversion of x (which that
        // wait precedes) to this place, behind them.
        unsigned w0[TL_CHUNK];
        slots(0, w0);
#pragma unroll
        for (int u = 0; u < TL_CHUNK; ++u) asm volatile("" : "+v"(xv[u]));
        bf16x8 xh;
#pragma unroll
        for (int u = 0; u < TL_CHUNK; ++u) xh[u] = (__bf16)xv[u];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
          unsigned w[TL_CHUNK];
          if (rb == 0) {
#pragma unroll
            for (int u = 0; u < TL_CHUNK; ++u) w[u] = w0[u];
          } else {
            slots(rb, w);
          }
          u32x4 ph;
#pragma unroll
          for (int p = 0; p < 4; ++p) ph[p] = ((w[2 * p] & 0xffffu) | (w[2 * p + 1] << 16)) & msk[p];
          acc[rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, ph), xh, acc[rb], 0, 0, 0);
          if (RB == 5) __builtin_amdgcn_sched_barrier(0);  // (five row blocks' slots read ahead at once cost registers the epilogue needs)
        }
      }
      kb += 4 * K4;
    }
    // ---- epilogue == token_linear_kernel's; D: row = 4 * (lane >> 4) + reg, column = lane & 15 ------------------------------------
    // everything the sample's elements READ first, ONE wait, then arithmetic and stores (vmcnt counts loads and stores in one queue)
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

template <int AM, int RB>
static void launch_token_linear_bf16_rb(hipStream_t st, const nasrec_gemm_desc_t* d, int grid, int wgs, size_t lds) {
  static unsigned long long big_lds_devices = 0;  // more than the default 64 KB of dynamic LDS must be requested once per kernel and device
  if (lds > 65536 && nasrec_lds_attr_needed(big_lds_devices))
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&token_linear_bf16_kernel<AM, RB>), hipFuncAttributeMaxDynamicSharedMemorySize, TL_MAX_LDS);
  hipLaunchKernelGGL((token_linear_bf16_kernel<AM, RB>), dim3(grid), dim3(1024), lds, st, *d, wgs);
}

template <int AM>
static void launch_token_linear_bf16_t(hipStream_t st, const nasrec_gemm_desc_t* d, int rb, int grid, int wgs, size_t lds) {
  switch (rb) {
    case 1: launch_token_linear_bf16_rb<AM, 1>(st, d, grid, wgs, lds); break;
    case 2: launch_token_linear_bf16_rb<AM, 2>(st, d, grid, wgs, lds); break;
    case 3: launch_token_linear_bf16_rb<AM, 3>(st, d, grid, wgs, lds); break;
    case 4: launch_token_linear_bf16_rb<AM, 4>(st, d, grid, wgs, lds); break;
    default: launch_token_linear_bf16_rb<AM, 5>(st, d, grid, wgs, lds); break;
  }
}

void launch_token_linear_bf16(hipStream_t st, const nasrec_gemm_desc_t* d, int rb, int grid, int wgs, size_t lds) {
  if (d->amode == NASREC_AM_KC)
    launch_token_linear_bf16_t<NASREC_AM_KC>(st, d, rb, grid, wgs, lds);
  else
    launch_token_linear_bf16_t<NASREC_AM_RC>(st, d, rb, grid, wgs, lds);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Token-axis weight gradient (binding TOKK / TOKK / PLAIN), bf16 products
// ---------------------------------------------------------------------------------------------------------------------------------
template <bool LO>
__device__ __forceinline__ s16x4 tb_frag4(const f32x4 v) {
  bf16x4 h;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    h[j] = (__bf16)v[j];
    if (LO) h[j] = (__bf16)(v[j] - (float)h[j]);
  }
  return __builtin_bit_cast(s16x4, h);
}

template <int RB, int CB, int NTERMS>
__global__ __launch_bounds__(64 * TDW_WAVES) void token_dw_bf16_kernel(const nasrec_gemm_desc_t d, int Mmax, int Nmax) {
  __shared__ __attribute__((aligned(16))) float red[4 * RB * CB * 4 * 64];
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
      s16x4 ah[RB], al[RB], xh[CB], xl[CB];
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) {
        ah[rb] = tb_frag4<false>(a[rb]);
        if (NTERMS == 3) al[rb] = tb_frag4<true>(a[rb]);
      }
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) {
        xh[cb] = tb_frag4<false>(x[cb]);
        if (NTERMS == 3) xl[cb] = tb_frag4<true>(x[cb]);
      }
#pragma unroll
      for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) {
          if (NTERMS == 3) {  // fixed order: lo x hi, hi x lo, hi x hi
            acc[rb][cb] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(al[rb], xh[cb], acc[rb][cb], 0, 0, 0);
            acc[rb][cb] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(ah[rb], xl[cb], acc[rb][cb], 0, 0, 0);
          }
          acc[rb][cb] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(ah[rb], xh[cb], acc[rb][cb], 0, 0, 0);
        }
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

template <int RB, int CB>
static void launch_token_dw_bf16_rc(hipStream_t st, const nasrec_gemm_desc_t* d, int grid, int Mmax, int Nmax) {
  if (d->precision == NASREC_PRECISION_HIGH)
    hipLaunchKernelGGL((token_dw_bf16_kernel<RB, CB, 3>), dim3(grid), dim3(64 * TDW_WAVES), 0, st, *d, Mmax, Nmax);
  else
    hipLaunchKernelGGL((token_dw_bf16_kernel<RB, CB, 1>), dim3(grid), dim3(64 * TDW_WAVES), 0, st, *d, Mmax, Nmax);
}

template <int RB>
static void launch_token_dw_bf16_rb(hipStream_t st, const nasrec_gemm_desc_t* d, int cb, int grid, int Mmax, int Nmax) {
  switch (cb) {
    case 1: launch_token_dw_bf16_rc<RB, 1>(st, d, grid, Mmax, Nmax); break;
    case 2: launch_token_dw_bf16_rc<RB, 2>(st, d, grid, Mmax, Nmax); break;
    case 3: launch_token_dw_bf16_rc<RB, 3>(st, d, grid, Mmax, Nmax); break;
    case 4: launch_token_dw_bf16_rc<RB, 4>(st, d, grid, Mmax, Nmax); break;
    default: launch_token_dw_bf16_rc<RB, 5>(st, d, grid, Mmax, Nmax); break;
  }
}

void launch_token_dw_bf16(hipStream_t st, const nasrec_gemm_desc_t* d, int rb, int cb, int grid, int Mmax, int Nmax) {
  switch (rb) {
    case 1: launch_token_dw_bf16_rb<1>(st, d, cb, grid, Mmax, Nmax); break;
    case 2: launch_token_dw_bf16_rb<2>(st, d, cb, grid, Mmax, Nmax); break;
    case 3: launch_token_dw_bf16_rb<3>(st, d, cb, grid, Mmax, Nmax); break;
    case 4: launch_token_dw_bf16_rb<4>(st, d, cb, grid, Mmax, Nmax); break;
    default: launch_token_dw_bf16_rb<5>(st, d, cb, grid, Mmax, Nmax); break;
  }
}
