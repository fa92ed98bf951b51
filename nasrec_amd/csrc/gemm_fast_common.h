// What the two bodies of the throughput-regime GEMM share (gemm_fast.hip: fp32 operands on v_mfma_f32_32x32x2_f32;
// gemm_fast_bf16.hip: bf16 operands on v_mfma_f32_32x32x16_bf16): the 128 x 128 x 32 tiling, the order of the tiles, the schedules
// (plain, split-K slabs, balanced pieces) and the epilogue.  Both instructions leave the accumulators in the same D layout
// (col = lane & 31, row = 8 * (reg >> 2) + 4 * (lane >> 5) + (reg & 3)), so everything behind the k-loop is one copy.
#pragma once
#include "gemm_tile.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

#define FT_BM 128
#define FT_BN 128
#define FT_BK 32
#define FT_KC_LD 36                        // [row][32 + 4]
#define FT_TILE_FLOATS (FT_BM * FT_KC_LD)  // 4608 >= 32 * 128 (the [k][row] form)
#define FT_FENCE() __builtin_amdgcn_sched_barrier(0)

__device__ __forceinline__ __amdgpu_buffer_rsrc_t ft_rsrc(const float* base, long extent_floats) {
  const long bytes = extent_floats * 4;
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, bytes > 0x7fffffffL ? 0x7fffffff : (int)bytes, 0x00020000);
}

#define FT_SK_WGS 512            // workgroups that share the odd tiles' iterations (2 per CU)
#define FT_SK_PIECES 3           // a share of < 2 tiles touches at most 3 tiles
#define FT_PIECE_FLOATS (FT_BM * FT_BN)

// Order of the tiles of one problem: groups of FT_GROUP_M tile rows, inside a group column by column.  The ~64 workgroups an
// XCD runs at a time then cover 8 rows x 8 columns (8 A panels + 8 B panels in its 4 MB L2) instead of 1.5 rows x 41 columns,
// and an XCD's contiguous run re-reads the B panels once per group instead of once per row: fabric reads of the
// 4096 x 5133 x 1024 product 634 MB -> (see profiles/) against 122 MB of operands.
#define FT_GROUP_M 8
__device__ __forceinline__ void ft_grouped(int t, int tm, int tn, int& by, int& bx) {
  const int per_group = FT_GROUP_M * tn;
  const int grp = t / per_group, first = grp * FT_GROUP_M;
  const int rows = tm - first < FT_GROUP_M ? tm - first : FT_GROUP_M;
  const int r = t - grp * per_group;
  bx = r / rows;
  by = first + (r - bx * rows);
}

// tile index (live tiles, problem-major, then k-split, grouped (m, n) order) -> problem z, k-split ks, tile row / column; false: no such tile
__device__ __forceinline__ bool ft_decode(const nasrec_gemm_desc_t& d, int lin, int S, int tiles_m, int tiles_n, int& z, int& ks, int& by,
                                          int& bx) {
  z = 0;
  if (d.zmode) {
    // a batch of independent problems: the grid holds exactly their LIVE tiles, so the eight contiguous runs the XCDs get
    // carry equal work whatever the mix of problem sizes (a grid padded to Mmax x Nmax handed six XCDs 72 tiles each — more
    // than their 64 workgroup slots — and two XCDs 8)
    int rem = lin, tn = 1, per = 1;
    for (;; ++z) {
      if (z >= d.nseg) return false;
      tn = (d.seg[z].N + FT_BN - 1) / FT_BN;
      per = ((d.seg[z].M + FT_BM - 1) / FT_BM) * tn;
      if (rem < per * S) break;
      rem -= per * S;
    }
    ks = rem / per;
    ft_grouped(rem - ks * per, per / tn, tn, by, bx);
  } else {
    const int per_z = tiles_m * tiles_n;
    ks = lin / per_z;
    ft_grouped(lin - ks * per_z, tiles_m, tiles_n, by, bx);
  }
  return true;
}

// XCD-aware order: ids are dealt round-robin to the 8 XCDs; give every XCD one contiguous run of [0, total) (bijective)
__device__ __forceinline__ int ft_xcd_run(int id, int total) {
  const int xcd = id & 7, q = id >> 3;
  const int chunk = total >> 3, rem = total & 7;
  return xcd * chunk + (xcd < rem ? xcd : rem) + q;
}

// first global k-iteration of share w of W iterations split over FT_SK_WGS workgroups
__device__ __host__ __forceinline__ long ft_share_begin(long W, int w) { return W * w / FT_SK_WGS; }

// epilogue of one finished 128 x 128 tile held in the D layout of v_mfma_f32_32x32x2_f32:
// col = lane & 31, row = 8 * (reg >> 2) + 4 * (lane >> 5) + (reg & 3)
__device__ __forceinline__ void ft_epilogue(const nasrec_gemm_desc_t& d, const nasrec_gemm_seg_t& s0, int m0, int n0, int wm, int wn, int fr,
                                            int fg, const f32x16 (&acc)[2][2], bool acc_in_tile) {
  const int M = s0.M, N = s0.N;
  const int Mv = (s0.Mvalid > 0 && s0.Mvalid < M) ? s0.Mvalid : M;
  // plain product (the common case of the large launches: LayerNorm / the split-K pass own the epilogue): straight stores
  // (acc_in_tile: the accumulators were started from the output tile — the accumulation is already in them)
  const bool plain = acc_in_tile || (!d.bias && !d.pre_add && !d.save_z && !d.save_act && d.act == NASREC_ACT_NONE && d.mul_nseg == 0 &&
                                     d.dims_in_use < 0 && !(d.zmode ? s0.accumulate : d.beta) && !s0.ones_col);
  if (plain) {
    float* Cp = s0.C;
    const int ldc = s0.ldc;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int i = m0 + wm * 64 + a * 32 + 8 * (r >> 2) + 4 * fg + (r & 3), j = n0 + wn * 64 + b * 32 + fr;
          if (i < M && j < N) Cp[(long)i * ldc + j] = i < Mv ? acc[a][b][r] : 0.f;
        }
    return;
  }
  // general epilogue == epilogue_store<NASREC_CM_PLAIN> element by element (gemm_tile.h), with everything that depends on the
  // column alone looked up once per lane and column: a lane owns 2 columns x 32 rows, and the gating product's segment search
  // (mul_lookup: a scalar loop over up to 8 k-segments) used to run for each of its 64 elements
  const bool acc_c = d.zmode ? s0.accumulate != 0 : d.beta != 0;
  const bool has_pre = d.pre_add != nullptr;
  float* rs = s0.rowsum ? s0.rowsum : d.rowsum_out;
  // per column of the lane: the gating operand's pointer / stride, the bias, the dead-column flag
  const float* mp[2] = {nullptr, nullptr};
  int mld[2] = {0, 0};
  float bias_c[2];
  bool dead_c[2];
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int j = min(n0 + wn * 64 + b * 32 + fr, N - 1);
    if (d.mul_nseg > 0) {
      for (int q = 0; q < d.mul_nseg; ++q) {
        const int jj = j - d.mul_off[q];
        if (jj >= 0 && jj < d.mul_width[q]) {
          mp[b] = d.mul_ptr[q] ? d.mul_ptr[q] + jj : nullptr;
          mld[b] = d.mul_ld[q];
          break;
        }
      }
    }
    bias_c[b] = d.bias ? d.bias[j] : 0.f;  // (a bias over rows belongs to the token-axis layout: gemm_fast_eligible)
    dead_c[b] = d.dims_in_use >= 0 && !d.mask_on_rows && j >= d.dims_in_use;
  }
  // one element from accumulator to memory: the same operations in the same order whichever way its operands were fetched.  NO load
  // in here: vmcnt counts loads and stores in one in-order queue, so a load between two stores makes the wave wait for every earlier
  // store to be acknowledged — once per element
  float* const Cp = s0.C;
  float* const zp = d.save_z;
  float* const ap = d.save_act;
  const long ldc = s0.ldc;
  const int act = d.act;
  const bool has_bias = d.bias != nullptr, has_mulv = d.mul_nseg > 0;
  const int dead_rows = (d.dims_in_use >= 0 && d.mask_on_rows) ? d.dims_in_use : 0x7fffffff;
  auto finish = [&](int i, int j, int b, float v, float prevv, float mulv, float cvv) {
    const long o = (long)i * ldc + j;
    if (has_pre) v += prevv;
    if (has_bias) v += bias_c[b];
    if (zp) zp[o] = v;
    v = act_apply(v, act);
    if (ap) ap[o] = v;
    if (has_mulv) v *= mulv;
    if (dead_c[b] || i >= dead_rows) v = 0.f;
    if (acc_c) v += cvv;
    Cp[o] = v;
  };
  const int nread = (d.mul_nseg > 0 ? 1 : 0) + (has_pre ? 1 : 0) + (acc_c ? 1 : 0);
  if (nread <= 1 && !s0.ones_col) {
    // ONE array is read (the accumulation target of a dx product, the gating operand, or the residual): all 64 of the lane's values are
    // in flight before its first store.  Sixteen at a time — load, wait, store, and vmcnt counts loads and stores in one queue, so the next
    // sixteen loads wait for the previous stores to be acknowledged — a 4096 x 1024 x 128 dx product took 39.7 us with accumulation against
    // 18.2 us without; a tile alone on its CU (256-tile launches) has nothing to hide four such round trips behind.
    float rd[2][2][16] = {};
    bool live_c[2] = {false, false};
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      if (nread == 0) break;  // (bias / activation / saved planes only: nothing to read)
      const int j = min(n0 + wn * 64 + b * 32 + fr, N - 1);
      const float* base = acc_c ? s0.C + j : has_pre ? d.pre_add + j : mp[b];
      const bool live = base != nullptr;  // (a column outside every gating segment: the loads go to C — unconditional, no branch — and count as 0)
      live_c[b] = live;
      const float* bp = live ? base : s0.C + j;
      const long ld = (acc_c || has_pre || !live) ? s0.ldc : mld[b];
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int i = min(m0 + wm * 64 + a * 32 + 8 * (r >> 2) + 4 * fg + (r & 3), M - 1);  // (clamped: rows >= M are never stored)
          rd[a][b][r] = bp[(long)i * ld];  // (straight into its register: a select here and the compiler loads one element at a time)
        }
    }
    // ONE wait for the whole batch, spelled out: the stores below sit behind uniform branches (saved planes present or not), the
    // compiler cannot count them, and without this it waits with vmcnt(0) — every earlier store acknowledged — at the first use of each
    // of the 64 loaded registers
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), expcnt / lgkmcnt untouched
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int j = n0 + wn * 64 + b * 32 + fr;
      if (j >= N) continue;
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int i = m0 + wm * 64 + a * 32 + 8 * (r >> 2) + 4 * fg + (r & 3);
          if (i >= M) continue;
          const float x = live_c[b] ? rd[a][b][r] : 0.f;
          finish(i, j, b, i < Mv ? acc[a][b][r] : 0.f, x, x, x);
        }
    }
    return;
  }
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int j = n0 + wn * 64 + b * 32 + fr;
    if (j >= N) continue;
    const bool ones_j = s0.ones_col && j == N - 1;
    // Everything the 16 rows of a fragment READ (the gating operand, the residual, the accumulation target) is loaded before the first of
    // their stores (round 4): element by element — load, use, store, and the next load may not pass that store, the arrays could
    // alias — a lane paid a dependent memory round trip per element, 64 per tile (the gated 4096 x 5133 x 1024 product: 96 TFLOP/s
    // against 131 for the plain product of the same shape).  Same arithmetic per element: same bits.
    const bool has_mul = d.mul_nseg > 0 && mp[b] != nullptr;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      float mulv[16] = {}, prev[16] = {}, cv[16] = {};
      long off[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) off[r] = min(m0 + wm * 64 + a * 32 + 8 * (r >> 2) + 4 * fg + (r & 3), M - 1);  // (clamped: rows >= M are never stored)
      // (one uniform branch per ARRAY, sixteen loads inside: a branch per element makes the compiler wait for element r before it issues r + 1)
      if (has_mul) {
#pragma unroll
        for (int r = 0; r < 16; ++r) mulv[r] = mp[b][off[r] * mld[b]];
      }
      // (The virtual ones column j = N - 1 has no element in C or pre_add: (i, N - 1) is (i + 1, 0) of a dense [M, N - 1] array, and for
      // the last row the float BEHIND it — an illegal access when the array ends where a mapping ends.  Its lanes read nothing; their
      // values were never used.  Still one branch per array, sixteen loads inside.)
      if (has_pre && !ones_j) {
#pragma unroll
        for (int r = 0; r < 16; ++r) prev[r] = d.pre_add[off[r] * ldc + j];
      }
      if (acc_c && !ones_j) {
#pragma unroll
        for (int r = 0; r < 16; ++r) cv[r] = Cp[off[r] * ldc + j];
      }
      __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): one wait per batch of sixteen (see above)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = m0 + wm * 64 + a * 32 + 8 * (r >> 2) + 4 * fg + (r & 3);
        if (i >= M) continue;
        const float v = i < Mv ? acc[a][b][r] : 0.f;
        if (ones_j) {
          rs[i] = v;
          continue;
        }
        finish(i, j, b, v, prev[r], mulv[r], cv[r]);
      }
    }
  }
}


// ---- host side ------------------------------------------------------------------------------------------------------------
// grid of a launch: tm x tn tiles per problem (of the largest problem), `blocks` workgroups; balanced schedule: sk_tiles > 0 odd tiles
// of sk_T k-iterations each, shared by the first FT_SK_WGS workgroups (0: every workgroup runs whole tiles)
static inline int ft_schedule(const nasrec_gemm_desc_t* d, int Mmax, int Nmax, int zdim, int& tm, int& tn, long& blocks, int& sk_tiles, int& sk_T) {
  tm = (Mmax + FT_BM - 1) / FT_BM, tn = (Nmax + FT_BN - 1) / FT_BN;
  blocks = (long)tm * tn * zdim;
  if (d->zmode) {  // live tiles only (zdim = problems x split-K)
    const int S = d->splitk > 1 ? d->splitk : 1;
    blocks = 0;
    for (int q = 0; q < d->nseg; ++q)
      blocks += (long)((d->seg[q].M + FT_BM - 1) / FT_BM) * ((d->seg[q].N + FT_BN - 1) / FT_BN) * S;
  }
  sk_tiles = 0, sk_T = 0;
  if (d->splitk == NASREC_SPLITK_BALANCED) {
    // every tile of the launch must have the same number of k-iterations
    int T = 0;
    if (d->zmode) {
      for (int q = 0; q < d->nseg; ++q) {
        const int tq = d->seg[q].A ? (d->seg[q].K + FT_BK - 1) / FT_BK : 0;
        if (q > 0 && tq != T) return nasrec_set_error(-2, "gemm: balanced schedule needs equal K over the batch (problem %d)", q);
        T = tq;
      }
    } else {
      for (int q = 0; q < d->nseg; ++q)
        if (d->seg[q].A) T += (d->seg[q].K + FT_BK - 1) / FT_BK;
    }
    if (T < 1) return nasrec_set_error(-2, "gemm: balanced schedule on an empty product");
    if (!d->workspace) return nasrec_set_error(-3, "gemm: balanced schedule needs a workspace of NASREC_SK_WORKSPACE_FLOATS floats");
    const long tiles = blocks;
    if (tiles % FT_SK_WGS != 0) {
      sk_tiles = (int)(tiles >= FT_SK_WGS ? FT_SK_WGS + tiles % FT_SK_WGS : tiles);
      sk_T = T;
      blocks = FT_SK_WGS + (tiles - sk_tiles);
    }
  }
  return 0;
}

// second pass of the balanced schedule (gemm_fast.hip: the accumulators of both bodies are fp32 in one layout)
void launch_gemm_fast_fixup(hipStream_t st, const nasrec_gemm_desc_t* d, int tiles_m, int tiles_n, int sk_tiles, int sk_T);
// the bf16 body (gemm_fast_bf16.hip): d->precision is NASREC_PRECISION_HIGH or NASREC_PRECISION_MEDIUM
int launch_gemm_fast_bf16(hipStream_t st, const nasrec_gemm_desc_t* d, int Mmax, int Nmax, int zdim);

// ---- the parts of the kernel prologue / epilogue that do not depend on how operands are staged --------------------------------
// The work of a workgroup.  Plain schedule: one (tile, k-split), lin_dp >= 0.  Balanced schedule (sk_tiles > 0): workgroup w < FT_SK_WGS
// runs the global k-iterations [W w / 512, W (w + 1) / 512) of the first sk_tiles tiles (W = sk_tiles * sk_T), i.e. up to FT_SK_PIECES
// pieces [g, g_end); the other workgroups one whole tile each.
__device__ __forceinline__ void ft_work_begin(int sk_tiles, int sk_T, long& g, long& g_end, int& lin_dp, int& w_sk) {
  g = 0, g_end = 1, lin_dp = -1, w_sk = 0;
  if (sk_tiles > 0) {
    if ((int)blockIdx.x < FT_SK_WGS) {
      w_sk = ft_xcd_run(blockIdx.x, FT_SK_WGS);
      const long W = (long)sk_tiles * sk_T;
      g = ft_share_begin(W, w_sk);
      g_end = ft_share_begin(W, w_sk + 1);
    } else {
      lin_dp = sk_tiles + ft_xcd_run(blockIdx.x - FT_SK_WGS, gridDim.x - FT_SK_WGS);
    }
  } else {
    lin_dp = ft_xcd_run(blockIdx.x, gridDim.x);
  }
}

// next piece: tile lin, and for a balanced piece its k-tiles [pa, pb); advances g
__device__ __forceinline__ void ft_work_next(int sk_T, int lin_dp, long& g, long g_end, int& lin, int& pa, int& pb) {
  pa = pb = 0;
  if (lin_dp >= 0) {
    lin = lin_dp;
    g = g_end;
  } else {
    lin = (int)(g / sk_T);
    pa = (int)(g - (long)lin * sk_T);
    const long left = g_end - g;
    pb = left < sk_T - pa ? pa + (int)left : sk_T;
    g += pb - pa;
  }
}

// k-tiles of a tile of problem z
__device__ __forceinline__ int ft_ktiles(const nasrec_gemm_desc_t& d, const nasrec_gemm_seg_t& s0) {
  if (d.zmode) return s0.A ? (s0.K + FT_BK - 1) / FT_BK : 0;
  int T = 0;
  for (int q = 0; q < d.nseg; ++q)
    if (d.seg[q].A) T += (d.seg[q].K + FT_BK - 1) / FT_BK;
  return T;
}

// k-tile t0 of the product -> segment s and k-tile kt inside it
__device__ __forceinline__ void ft_seek(const nasrec_gemm_desc_t& d, int z, int t0, int& s, int& kt) {
  s = z, kt = t0;
  if (d.zmode) return;
  s = 0;
  int skip = t0;
  while (s < d.nseg) {
    const int nt = d.seg[s].A ? (d.seg[s].K + FT_BK - 1) / FT_BK : 0;
    if (skip < nt) break;
    skip -= nt;
    ++s;
  }
  kt = skip;
}

// Does a whole tile of an unsplit launch that only ACCUMULATES into its output start its accumulators from the output tile?  (See
// gemm_fast_kernel: the sum is C + (k-tiles in order), and the epilogue is the plain store.)
__device__ __forceinline__ bool ft_acc_init(const nasrec_gemm_desc_t& d, const nasrec_gemm_seg_t& s0, int S, int lin_dp) {
  return S == 1 && lin_dp >= 0 && (d.zmode ? s0.accumulate != 0 : d.beta != 0) && !d.bias && !d.pre_add && !d.save_z && !d.save_act &&
         d.act == NASREC_ACT_NONE && d.mul_nseg == 0 && d.dims_in_use < 0 && !s0.ones_col && !(s0.Mvalid > 0 && s0.Mvalid < s0.M);
}

__device__ __forceinline__ void ft_acc_start(f32x16 (&acc)[2][2], bool acc_init, const nasrec_gemm_seg_t& s0, int m0, int n0, int wm, int wn,
                                             int fr, int fg) {
  if (acc_init) {
    const float* Cp = s0.C;
    const long ldc = s0.ldc;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) {  // (clamped: what lies outside the product is read and never stored)
          const int i = min(m0 + wm * 64 + a * 32 + 8 * (r >> 2) + 4 * fg + (r & 3), s0.M - 1), j = min(n0 + wn * 64 + b * 32 + fr, s0.N - 1);
          acc[a][b][r] = Cp[(long)i * ldc + j];
        }
  } else {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
  }
}

// a partial run of a tile's k-iterations (balanced schedule): raw accumulators to the workgroup's piece slot (gemm_fast_fixup_kernel sums)
__device__ __forceinline__ void ft_store_piece(const nasrec_gemm_desc_t& d, int w_sk, int piece, int tid, const f32x16 (&acc)[2][2]) {
  float* slot = d.workspace + ((long)w_sk * FT_SK_PIECES + piece) * FT_PIECE_FLOATS;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) slot[((a * 2 + b) * 16 + r) * 256 + tid] = acc[a][b][r];
}

// one k-split of a tile (plain split-K): to its slab; the second pass of launch_gemm sums the slabs and runs the epilogue
__device__ __forceinline__ void ft_store_slab(const nasrec_gemm_desc_t& d, const nasrec_gemm_seg_t& s0, int z, int ks, int S, int Mmax, int Nmax,
                                              int m0, int n0, int wm, int wn, int fr, int fg, const f32x16 (&acc)[2][2]) {
  const int M = s0.M, N = s0.N;
  const int Mv = (s0.Mvalid > 0 && s0.Mvalid < M) ? s0.Mvalid : M;
  float* slab = d.workspace + ((long)(z * S + ks)) * Mmax * Nmax;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = m0 + wm * 64 + a * 32 + 8 * (r >> 2) + 4 * fg + (r & 3), j = n0 + wn * 64 + b * 32 + fr;
        if (i < M && j < N) slab[(long)i * N + j] = i < Mv ? acc[a][b][r] : 0.f;
      }
}
