// Throughput-regime GEMM with bf16 matrix-core products: the second body of NASREC_GEMM_ROUTE_FAST launches, taken when the
// descriptor permits it (nasrec_gemm_desc_t.precision = NASREC_PRECISION_HIGH / _MEDIUM; gemm_fast.hip is HIGHEST).
//
// Memory is fp32 on both sides and the accumulators are fp32; what changes is what the matrix cores multiply.  With â = bf16(a),
// round to nearest even:
//   MEDIUM  acc += â b̂                                  one v_mfma_f32_32x32x16_bf16 per 16 k (bf16 x bf16 is exact in fp32)
//   HIGH    a ~ a_hi + a_lo, a_hi = bf16(a), a_lo = bf16(a - a_hi); acc += a_lo b_hi, then a_hi b_lo, then a_hi b_hi: three MFMAs
//           per 16 k in that fixed order (the lo x lo term, <= 2^-18 |a||b|, is dropped)
// v_mfma_f32_32x32x16_bf16 does 8x the k of v_mfma_f32_32x32x2_f32 in half the cycles.
//
// Tiles, tile order, schedules (plain, split-K slabs, balanced pieces + gemm_fast_fixup_kernel), acc_init, the virtual ones column,
// Mvalid and the epilogue are those of gemm_fast.hip (gemm_fast_common.h): the D layout of the two instructions is the same.  New
// is the staging and the k-loop:
//   * operands are read as fp32 with the same bounds-checked 16-byte buffer loads; a thread owns a 4 x 4 block of an operand tile
//     (k-contiguous memory: 4 rows x 4 consecutive k; row-contiguous memory: 4 consecutive k x 4 rows), converts it when it parks it
//     (v_cvt_pk_bf16_f32; HIGH: both planes) and writes 4 consecutive k of one row per 8-byte LDS store — a row-contiguous operand is
//     transposed in registers on the way;
//   * LDS holds bf16 as [row][32 + 8] for BOTH bindings, so a lane's MFMA fragment (k = 16 s + 8 (lane >> 5) + j, j = 0..7, of row
//     lane & 31) is one ds_read_b128.  The 80-byte pitch is the row plus one access width: the 16 rows of a ds_read_b128 lane group
//     fall on 16 different 16-byte slots of the 256-byte bank row (5 r mod 16), conflict-free;
//   * double buffered, one barrier per k-tile; 2 (buffers) x 2 (operands) x planes x 10 KB = 40 KB (MEDIUM) / 80 KB (HIGH) per
//     workgroup, two workgroups per CU;
//   * the k order inside a tile is the natural one for A and B alike; a tile's sum is the MFMA's own chain, tiles are added in
//     ascending k: the result of a descriptor does not depend on timing.
#include "gemm_fast_common.h"

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

#define BT_LD 40                      // bf16 per LDS row: 32 k + 8 (one 16-byte access width)
#define BT_PLANE (FT_BM * BT_LD)      // one 128-row operand plane

// A thread's 4 x 4 block of a 128-row x 32-k operand tile.  Register v[it][e] (16-byte load `it`, element e) holds
//   k-contiguous memory:   row bt_row(tid, it), k = bt_kbase(tid) + e        (8 lanes cover the 128 bytes of a row)
//   row-contiguous memory: row bt_row(tid, e),  k = bt_kbase(tid) + it       (4 lanes cover 64 bytes of a k-row)
// either way 4 consecutive k of each of 4 rows: one 8-byte LDS store per row.
template <int MODE>
__device__ __forceinline__ int bt_kbase(int tid) { return MODE == NASREC_AM_KC ? (tid & 7) << 2 : ((tid >> 2) & 7) << 2; }
template <int MODE>
__device__ __forceinline__ int bt_row(int tid, int ri) { return MODE == NASREC_AM_KC ? (tid >> 3) + 32 * ri : 4 * ((tid & 3) + 4 * (tid >> 5)) + ri; }
template <int MODE>
__device__ __forceinline__ int bt_ri(int it, int e) { return MODE == NASREC_AM_KC ? it : e; }  // which of the 4 rows / k register (it, e) holds
template <int MODE>
__device__ __forceinline__ int bt_ki(int it, int e) { return MODE == NASREC_AM_KC ? e : it; }

// convert and park one block.  ones_rows: bit ri set = that row is the virtual ones column; kvalid: bit j set = k bt_kbase + j lies inside
// the segment (a partial tile arrives with its other elements already zero)
template <int MODE, int PL, bool ONES>
__device__ __forceinline__ void bt_park(__bf16* hi, __bf16* lo, int tid, const f32x4 (&v)[4], int ones_rows, int kvalid) {
  const int kb = bt_kbase<MODE>(tid);
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    float x[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      x[j] = MODE == NASREC_AM_KC ? v[w][j] : v[j][w];
      if (ONES && ((ones_rows >> w) & 1)) x[j] = ((kvalid >> j) & 1) ? 1.f : 0.f;
    }
    bf16x4 h;
#pragma unroll
    for (int j = 0; j < 4; ++j) h[j] = (__bf16)x[j];
    const int o = bt_row<MODE>(tid, w) * BT_LD + kb;
    *reinterpret_cast<bf16x4*>(&hi[o]) = h;
    if (PL == 2) {
      bf16x4 l;
#pragma unroll
      for (int j = 0; j < 4; ++j) l[j] = (__bf16)(x[j] - (float)h[j]);
      *reinterpret_cast<bf16x4*>(&lo[o]) = l;
    }
  }
}

// NTERMS: 1 = MEDIUM, 3 = HIGH.  sk_tiles > 0: balanced schedule (gemm_fast_common.h)
template <int AM, int BMODE, bool ONES, int NTERMS>
__global__ __launch_bounds__(256, 2) void gemm_fast_bf16_kernel(const nasrec_gemm_desc_t d, int Mmax, int Nmax, int tiles_m, int tiles_n,
                                                                int sk_tiles, int sk_T) {
  constexpr int PL = NTERMS == 3 ? 2 : 1;  // planes per operand: hi (, lo)
  __shared__ __attribute__((aligned(16))) __bf16 smem[2][2][PL][BT_PLANE];  // [buffer][A, B][plane]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 31, fg = lane >> 5;
  const int S = d.splitk > 1 ? d.splitk : 1;

  long g, g_end;
  int lin_dp, w_sk;
  ft_work_begin(sk_tiles, sk_T, g, g_end, lin_dp, w_sk);
  for (int piece = 0; g < g_end; ++piece) {
    int lin, pa, pb;
    ft_work_next(sk_T, lin_dp, g, g_end, lin, pa, pb);
    int z, ks, by, bx;
    if (!ft_decode(d, lin, S, tiles_m, tiles_n, z, ks, by, bx)) continue;
    const nasrec_gemm_seg_t& s0 = d.seg[z];
    const int M = s0.M, N = s0.N;
    const int m0 = by * FT_BM, n0 = bx * FT_BN;
    if (m0 >= M || n0 >= N) continue;

    // ---- k range of this split / piece ----------------------------------------------------------------------------------
    const int T = ft_ktiles(d, s0);
    const bool sk_piece = lin_dp < 0;
    const int t0 = sk_piece ? pa : (int)((long)T * ks / S), t1 = sk_piece ? pb : (int)((long)T * (ks + 1) / S);
    int s, kt;
    ft_seek(d, z, t0, s, kt);

    const bool acc_init = ft_acc_init(d, s0, S, lin_dp);
    f32x16 acc[2][2];
    ft_acc_start(acc, acc_init, s0, m0, n0, wm, wn, fr, fg);

    // ---- staging state (per segment) ------------------------------------------------------------------------------------
    const bool has_ones = ONES && s0.ones_col != 0;  // (ONES = some problem of the launch has the virtual column; this one: has_ones)
    const int Rb = has_ones ? N - 1 : N;             // real rows of B
    const float* pA = nullptr;
    const float* pB = nullptr;
    __amdgpu_buffer_rsrc_t rsA = ft_rsrc(nullptr, 0), rsB = ft_rsrc(nullptr, 0);
    int cK = 0, lda = 0, ldb = 0;
    int stepA = 0, stepB = 0;  // bytes per k-tile
    int voffA[4], voffB[4];    // byte offset of 16-byte load `it` at k-tile 0 (rows beyond the operand: bounds-checked garbage / 0, never stored)
    auto load_seg = [&](int sq) {
      const nasrec_gemm_seg_t& sg = d.seg[sq];
      pA = sg.A;
      pB = sg.B;
      cK = sg.K;
      lda = sg.lda;
      ldb = sg.ldb;
      // extents: last element any in-range (row, k) can touch
      rsA = ft_rsrc(pA, AM == NASREC_AM_KC ? (long)(M - 1) * lda + cK : (long)(cK - 1) * lda + M);
      rsB = ft_rsrc(pB, BMODE == NASREC_AM_KC ? (long)(Rb - 1) * ldb + cK : (long)(cK - 1) * ldb + Rb);
      stepA = 4 * FT_BK * (AM == NASREC_AM_KC ? 1 : lda);
      stepB = 4 * FT_BK * (BMODE == NASREC_AM_KC ? 1 : ldb);
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        // k-contiguous: load `it` is a row (redirected to the last row beyond the operand: the offset stays inside 31 bits for any
        // shape); row-contiguous: load `it` is a k-row, its 4 rows simply run on into the next k-row
        voffA[it] = 4 * (int)(AM == NASREC_AM_KC ? (long)min(m0 + bt_row<AM>(tid, it), M - 1) * lda + bt_kbase<AM>(tid)
                                                 : (long)(bt_kbase<AM>(tid) + it) * lda + (m0 + bt_row<AM>(tid, 0)));
        voffB[it] = 4 * (int)(BMODE == NASREC_AM_KC ? (long)min(n0 + bt_row<BMODE>(tid, it), Rb - 1) * ldb + bt_kbase<BMODE>(tid)
                                                    : (long)(bt_kbase<BMODE>(tid) + it) * ldb + (n0 + bt_row<BMODE>(tid, 0)));
      }
    };
    int onesB = 0;  // which of the thread's 4 rows of B is the virtual column N - 1
    if (has_ones) {
#pragma unroll
      for (int ri = 0; ri < 4; ++ri) onesB |= (n0 + bt_row<BMODE>(tid, ri) == N - 1) ? (1 << ri) : 0;
    }

    auto park = [&](int buf, const f32x4 (&va)[4], const f32x4 (&vb)[4], int kvalidA, int kvalidB) {
      bt_park<AM, PL, false>(smem[buf][0][0], smem[buf][0][PL - 1], tid, va, 0, kvalidA);
      bt_park<BMODE, PL, ONES>(smem[buf][1][0], smem[buf][1][PL - 1], tid, vb, onesB, kvalidB);
    };
    // A partial k-tile goes global -> LDS in one synchronous, fully checked step: every index clamped into the operand, every element
    // beyond the segment's K zero
    auto commit_tail = [&](int buf, int ktq) {
      const int k0 = ktq * FT_BK;
      f32x4 va[4], vb[4];
      int kvA = 0, kvB = 0;
#pragma unroll
      for (int it = 0; it < 4; ++it)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          {
            const int k = k0 + bt_kbase<AM>(tid) + bt_ki<AM>(it, e), kk = min(k, cK - 1);
            const int rr = min(m0 + bt_row<AM>(tid, bt_ri<AM>(it, e)), M - 1);
            const float x = pA[AM == NASREC_AM_KC ? (long)rr * lda + kk : (long)kk * lda + rr];
            va[it][e] = k < cK ? x : 0.f;
            if (k < cK) kvA |= 1 << bt_ki<AM>(it, e);
          }
          {
            const int k = k0 + bt_kbase<BMODE>(tid) + bt_ki<BMODE>(it, e), kk = min(k, cK - 1);
            const int rr = max(min(n0 + bt_row<BMODE>(tid, bt_ri<BMODE>(it, e)), Rb - 1), 0);
            const float x = pB[BMODE == NASREC_AM_KC ? (long)rr * ldb + kk : (long)kk * ldb + rr];
            vb[it][e] = k < cK ? x : 0.f;
            if (k < cK) kvB |= 1 << bt_ki<BMODE>(it, e);
          }
        }
      park(buf, va, vb, kvA, kvB);
    };
    // the MFMAs of one parked k-tile: 2 k-steps of 16, fragments = 8 consecutive k of the lane's row
    auto compute = [&](int buf) {
      const int offA = (wm * 64 + fr) * BT_LD + 8 * fg, offB = (wn * 64 + fr) * BT_LD + 8 * fg;
#pragma unroll
      for (int ksub = 0; ksub < 2; ++ksub) {
        bf16x8 fa[PL][2], fb[PL][2];
#pragma unroll
        for (int p = 0; p < PL; ++p)
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            fa[p][t] = *reinterpret_cast<const bf16x8*>(&smem[buf][0][p][offA + t * 32 * BT_LD + 16 * ksub]);
            fb[p][t] = *reinterpret_cast<const bf16x8*>(&smem[buf][1][p][offB + t * 32 * BT_LD + 16 * ksub]);
          }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b) {
            if (NTERMS == 3) {  // fixed order: lo x hi, hi x lo, hi x hi
              acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[PL - 1][a], fb[0][b], acc[a][b], 0, 0, 0);
              acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0][a], fb[PL - 1][b], acc[a][b], 0, 0, 0);
            }
            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0][a], fb[0][b], acc[a][b], 0, 0, 0);
          }
      }
    };

    // ---- main loop: one barrier per k-tile ------------------------------------------------------------------------------
    f32x4 ra[4], rb[4];
    if (t0 < t1) {
      load_seg(s);
      if ((kt + 1) * FT_BK <= cK) {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
          ra[it] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsA, voffA[it], kt * stepA, 0));
          rb[it] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsB, voffB[it], kt * stepB, 0));
        }
        park(0, ra, rb, 15, 15);
      } else {
        commit_tail(0, kt);
      }
      __syncthreads();
    }
    const __amdgpu_buffer_rsrc_t rs_null = ft_rsrc(nullptr, 0);  // num_records 0: every load returns 0 without touching memory
    int seg_tiles = (cK + FT_BK - 1) / FT_BK;  // k-tiles of the current segment
    for (int t = t0; t < t1; ++t) {
      const int buf = (t - t0) & 1;
      ++kt;
      const bool more = t + 1 < t1;
      if (more && kt >= seg_tiles) {  // segment exhausted (rare): next live segment
        if (!d.zmode) {
          do {
            ++s;
          } while (s < d.nseg && (!d.seg[s].A || d.seg[s].K <= 0));
          kt = 0;
        }
        load_seg(s);
        seg_tiles = (cK + FT_BK - 1) / FT_BK;
      }
      const bool next_full = more && (kt + 1) * FT_BK <= cK;
      // the next tile's loads go out ahead of this tile's MFMAs — unconditionally (no branch between them and their use), against the
      // null resource when there is no full next tile
      const __amdgpu_buffer_rsrc_t curA = next_full ? rsA : rs_null;
      const __amdgpu_buffer_rsrc_t curB = next_full ? rsB : rs_null;
      const int soffA = next_full ? kt * stepA : 0, soffB = next_full ? kt * stepB : 0;
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        ra[it] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(curA, voffA[it], soffA, 0));
        rb[it] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(curB, voffB[it], soffB, 0));
      }
      compute(buf);
      if (next_full)
        park(buf ^ 1, ra, rb, 15, 15);
      else if (more)
        commit_tail(buf ^ 1, kt);
      __syncthreads();
    }

    // ---- epilogue ---------------------------------------------------------------------------------------------------------
    if (sk_piece && !(t0 == 0 && t1 == T)) {
      ft_store_piece(d, w_sk, piece, tid, acc);
      continue;  // (the main loop ends on a barrier: the next piece may restage the LDS buffers)
    }
    if (S > 1) {
      ft_store_slab(d, s0, z, ks, S, Mmax, Nmax, m0, n0, wm, wn, fr, fg, acc);
      continue;
    }
    ft_epilogue(d, s0, m0, n0, wm, wn, fr, fg, acc, acc_init);
  }
}

template <int AM, int BMODE>
static int launch_fast_bf16_t(hipStream_t st, const nasrec_gemm_desc_t* d, int Mmax, int Nmax, int zdim, bool ones) {
  int tm, tn, sk_tiles, sk_T;
  long blocks;
  const int rc = ft_schedule(d, Mmax, Nmax, zdim, tm, tn, blocks, sk_tiles, sk_T);
  if (rc) return rc;
  const dim3 grid((unsigned)blocks);
  const bool high = d->precision == NASREC_PRECISION_HIGH;
  if (ones && high)
    hipLaunchKernelGGL((gemm_fast_bf16_kernel<AM, BMODE, true, 3>), grid, dim3(256), 0, st, *d, Mmax, Nmax, tm, tn, sk_tiles, sk_T);
  else if (ones)
    hipLaunchKernelGGL((gemm_fast_bf16_kernel<AM, BMODE, true, 1>), grid, dim3(256), 0, st, *d, Mmax, Nmax, tm, tn, sk_tiles, sk_T);
  else if (high)
    hipLaunchKernelGGL((gemm_fast_bf16_kernel<AM, BMODE, false, 3>), grid, dim3(256), 0, st, *d, Mmax, Nmax, tm, tn, sk_tiles, sk_T);
  else
    hipLaunchKernelGGL((gemm_fast_bf16_kernel<AM, BMODE, false, 1>), grid, dim3(256), 0, st, *d, Mmax, Nmax, tm, tn, sk_tiles, sk_T);
  if (sk_tiles > 0) launch_gemm_fast_fixup(st, d, tm, tn, sk_tiles, sk_T);
  return 0;
}

int launch_gemm_fast_bf16(hipStream_t st, const nasrec_gemm_desc_t* d, int Mmax, int Nmax, int zdim) {
  bool ones = false;
  for (int q = 0; q < d->nseg; ++q) ones = ones || d->seg[q].ones_col != 0;
  if (d->amode == NASREC_AM_KC && d->bmode == NASREC_AM_KC) return launch_fast_bf16_t<NASREC_AM_KC, NASREC_AM_KC>(st, d, Mmax, Nmax, zdim, ones);
  if (d->amode == NASREC_AM_KC && d->bmode == NASREC_AM_RC) return launch_fast_bf16_t<NASREC_AM_KC, NASREC_AM_RC>(st, d, Mmax, Nmax, zdim, ones);
  return launch_fast_bf16_t<NASREC_AM_RC, NASREC_AM_RC>(st, d, Mmax, Nmax, zdim, ones);
}
