// Large-batch token-axis Linear kernels with bf16 matrix-core products: NASREC_GEMM_ROUTE_TOKEN_LINEAR launches at
// nasrec_gemm_desc_t.precision = NASREC_PRECISION_MEDIUM and NASREC_GEMM_ROUTE_TOKEN_DW launches at _HIGH / _MEDIUM (token_linear.hip
// is every other case).  Same eligibility rules, same launch geometry, and the same kernel bodies around the product
// (token_linear_common.h: token_linear_body, token_dw_body).
//
// Memory is fp32 on both sides and the accumulators are fp32; what changes is what the matrix cores multiply.  With â = bf16(a),
// round to nearest even:
//   MEDIUM  acc += â b̂                                  (bf16 x bf16 is exact in fp32)
//   HIGH    a ~ a_hi + a_lo, a_hi = bf16(a), a_lo = bf16(a - a_hi); acc += a_lo b_hi, then a_hi b_lo, then a_hi b_hi: three MFMAs
//           in that fixed order (the lo x lo term, <= 2^-18 |a||b|, is dropped); a = dz, b = x
//
// token_linear_bf16_kernel (MEDIUM).  The fp32 product spends its time on v_mfma_f32_16x16x4_f32: eight of them (32 cycles each) per row
// block and TL_CHUNK of 32 k.  Here one v_mfma_f32_16x16x32_bf16 (16 cycles) takes their place:
//   * the streamed operand keeps its load pattern.  The eight 256-byte loads of a chunk give lane (g, e) the rows 4 u + g, u = 0..7,
//     of 32 consecutive k; four v_cvt_pk_bf16_f32 make them the lane's B fragment, MFMA k = 8 g + u  <->  chunk k = 4 u + g.  The
//     permutation is free as long as A agrees;
//   * the weights keep the fp32 kernel's LDS image — k-major [k][MP] 32-bit slots, zero-padded to whole k-steps of 4 — so the staging
//     needs exactly the bytes the shared eligibility rule budgets (TL_MAX_LDS), whatever the segments' K: a slot holds bf16(w) in its
//     low half, rounded ONCE per workgroup at staging.  A lane's A fragment is the same eight ds_read_b32 the fp32 product issues (slot
//     (4 u + g, i)), packed pairwise by four VALU ops;
//   * k-steps beyond a segment's K inside its last chunk are not staged: their slots are read at an address clamped into the
//     segment and masked to zero (uniform arithmetic, no branch), and the streamed side reads zeros there by the buffer range check.
// The k order inside a sample is fixed (segments in order, chunks ascending, the MFMA's own chain inside a chunk): the result of a
// descriptor does not depend on launch geometry or timing.
// A HIGH variant of this kernel (both halves of the slot, three MFMAs) was built and measured and is not here: DESIGN.md.
//
// token_dw_bf16_kernel (MEDIUM, HIGH).  A lane's 16-byte load holds e = 4 g .. 4 g + 3 of its row: the operand layout of the 16-deep
// v_mfma_f32_16x16x16_bf16 with k = e.  Per sample and (rb, cb) one MFMA (HIGH: three) instead of four fp32 ones; the virtual ones
// column stays exact (1.0 is a bf16 value, its lo part 0).
#include "token_linear_common.h"

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned tb_bits(__bf16 h) { return (unsigned)__builtin_bit_cast(unsigned short, h); }

// MEDIUM only (HIGH keeps token_linear_kernel: its three products per k did not pay on every measured launch — DESIGN.md)
struct TlBf16 {
  typedef unsigned slot_t;  // bf16(w) in the low half of a 32-bit slot
  static __device__ __forceinline__ unsigned slot(float w) { return tb_bits((__bf16)w); }
  template <int RB, int MP>
  static __device__ __forceinline__ void chunk(const unsigned* wchunk, int live, float (&xv)[TL_CHUNK], f32x4 (&acc)[RB]) {
    // The last chunk of a segment may hold k-steps beyond the staged weights: their LDS address is clamped into the segment and their
    // slots are masked to zero — all of it uniform (scalar) arithmetic and ONE straight-line body for full and partial chunks, so
    // that the loads of x and the LDS reads go out together: a branch between them puts an LDS round trip (two, with the reads the
    // compiler hoists above it) behind every load, which a launch of short segments out of the caches feels (measured: 7.1 us as
    // fp32, 7.7 us with the branch, B = 8192, M = 10, K = 10 + 10).
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
};

template <int AM, int RB>
__global__ __launch_bounds__(1024) void token_linear_bf16_kernel(const nasrec_gemm_desc_t d, int wgs) {
  token_linear_body<AM, RB, TlBf16>(d, wgs);
}

void launch_token_linear_bf16(hipStream_t st, const nasrec_gemm_desc_t* d, int rb, int grid, int wgs, size_t lds) {
  tl_blocks(rb, [&](auto RB) {
    if (d->amode == NASREC_AM_KC)
      tl_launch<token_linear_bf16_kernel<NASREC_AM_KC, decltype(RB)::value>>(st, grid, 1024, lds, *d, wgs);
    else
      tl_launch<token_linear_bf16_kernel<NASREC_AM_RC, decltype(RB)::value>>(st, grid, 1024, lds, *d, wgs);
  });
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

template <int NTERMS>
struct TdwBf16 {
  struct frag_t {
    s16x4 hi, lo;
  };
  static constexpr int STEPS = 1;
  static __device__ __forceinline__ frag_t frag(const f32x4 v) {
    frag_t f;
    f.hi = tb_frag4<false>(v);
    if (NTERMS == 3) f.lo = tb_frag4<true>(v);
    return f;
  }
  static __device__ __forceinline__ f32x4 mma(int, const frag_t a, const frag_t x, f32x4 acc) {
    if (NTERMS == 3) {  // fixed order: lo x hi, hi x lo, hi x hi
      acc = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a.lo, x.hi, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a.hi, x.lo, acc, 0, 0, 0);
    }
    return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a.hi, x.hi, acc, 0, 0, 0);
  }
};

template <int RB, int CB, int NTERMS>
__global__ __launch_bounds__(64 * TDW_WAVES) void token_dw_bf16_kernel(const nasrec_gemm_desc_t d, int Mmax, int Nmax) {
  token_dw_body<RB, CB, TdwBf16<NTERMS>>(d, Mmax, Nmax);
}

void launch_token_dw_bf16(hipStream_t st, const nasrec_gemm_desc_t* d, int rb, int cb, int grid, int Mmax, int Nmax) {
  tl_blocks(rb, [&](auto RB) {
    tl_blocks(cb, [&](auto CB) {
      if (d->precision == NASREC_PRECISION_HIGH)
        tl_launch<token_dw_bf16_kernel<decltype(RB)::value, decltype(CB)::value, 3>>(st, grid, 64 * TDW_WAVES, 0, *d, Mmax, Nmax);
      else
        tl_launch<token_dw_bf16_kernel<decltype(RB)::value, decltype(CB)::value, 1>>(st, grid, 64 * TDW_WAVES, 0, *d, Mmax, Nmax);
    });
  });
}
