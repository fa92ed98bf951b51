// Adam and momentum SGD of the fused training step (NASREC_OP_OPT_MOMENTS, include/nasrec_hip.h): torch.optim.Adam / torch.optim.SGD
// (main_train.py:150-160) on the dense arena and on EVERY table row.  Phase 0 takes the place of Adagrad's apply launch (clip
// coefficient, dense chunks, the batch's touched rows, which it marks in a bitmap); phase 1 streams the untouched rows of every table
// (a zero gradient still moves a row whose moments are non-zero: W and its one or two moment arrays, read and written once) and,
// in the workgroup that finishes last, counts the step of every parameter it updated.
// Phase 0 is one kernel, opt_moments_phase0_kernel<Rows>; what happens to one touched row, and whether the launch marks the bitmap or
// counts the steps itself, is the row policy `Rows` (DenseRows, SparseAdamRows, LazyRmspropRows, AdagradTableRows, RowwiseAdagradRows over
// fp32 or bf16 rows, RowwiseSparseAdamRows below); which descriptor takes which policy, and what it must bring, is ROW_FORMS.
// The other forms (include/nasrec_hip.h) move the batch's rows only: the same clip and dense chunks, no bitmap, and no phase 1 unless
// weight decay has gradients to restore.  RMSprop (momentum 0, not centered) among them lets a row whose gradient is zero rest while
// its square_avg only decays: opt_moments_flush_kernel (phase 2) brings every row's square_avg current for whoever reads the state.
#include "optimizer_bodies.h"

namespace {

// which moment arrays an algorithm keeps: m = exp_avg / momentum_buffer (not RMSprop), v = exp_avg_sq / square_avg (not SGD)
template <int ALGO>
constexpr bool HAS_M = ALGO != NASREC_OPTIM_RMSPROP;
template <int ALGO>
constexpr bool HAS_V = ALGO != NASREC_OPTIM_SGD;

template <int ALGO>
__device__ __forceinline__ void moments_vec(const nasrec_opt_moments_desc_t& d, const f32x4& g, f32x4& p, f32x4& m, f32x4& v, float lr,
                                            float ss, float bs) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float pe = p[e], me = HAS_M<ALGO> ? m[e] : 0.f, ve = HAS_V<ALGO> ? v[e] : 0.f;
    moments_elem<ALGO>(d, g[e], pe, me, ve, lr, ss, bs);
    p[e] = pe;
    if (HAS_M<ALGO>) m[e] = me;
    if (HAS_V<ALGO>) v[e] = ve;
  }
}

// per-table scalars into LDS (threads [first, first + Fs)); the caller synchronises
template <int ALGO>
__device__ __forceinline__ void table_scalars(const nasrec_opt_moments_desc_t& d, int first, float lr, float* ss, float* bs) {
  const int f = (int)threadIdx.x - first;
  if (ALGO == NASREC_OPTIM_ADAM && f >= 0 && f < d.Fs) adam_scalars(d, d.step[d.table_step0 + f], lr, ss[f], bs[f]);
}

// The workgroup that arrives last at d.counter (of the launch's `nblk`) adds 1 to step[inc[i]] and leaves the counter zero.  It may:
// every workgroup has read its step counters (dense_chunks, the tables' scalars) when it arrives.
__device__ __forceinline__ void count_steps_in_last_workgroup(const nasrec_opt_moments_desc_t& d, unsigned nblk) {
  __shared__ int last;
  const int tid = threadIdx.x;
  __syncthreads();
  if (tid == 0) {
    __threadfence();
    last = atomicAdd(d.counter, 1u) == nblk - 1u;
  }
  __syncthreads();
  if (!last) return;
  __threadfence();
  for (long i = tid; i < d.n_inc; i += 256) d.step[d.inc[i]] += 1.f;
  if (tid == 0) *d.counter = 0u;
}

// phase 0's dense arena (workgroups [0, dense_blocks)): one parameter per chunk (its step counter), float4 pieces, then the chunk's tail
template <int ALGO>
__device__ __forceinline__ void dense_chunks(const nasrec_opt_moments_desc_t& d, float coef, float lr) {
  const int tid = threadIdx.x, blk = blockIdx.x;
  for (long c = blk; c < d.nchunks; c += d.dense_blocks) {
    const long off = d.chunks[3 * c], n = d.chunks[3 * c + 1], k = d.chunks[3 * c + 2], n4 = n >> 2;
    float ss = 0.f, bs = 1.f;
    if (ALGO == NASREC_OPTIM_ADAM) adam_scalars(d, d.step[k], lr, ss, bs);
    float* pp = d.p + off;
    float* mp = HAS_M<ALGO> ? d.m + off : nullptr;
    float* vp = HAS_V<ALGO> ? d.v + off : nullptr;
    const float* gp = d.g + off;
    for (long i = tid; i < n4; i += 256) {
      f32x4 g4 = *reinterpret_cast<const f32x4*>(gp + 4 * i);
      f32x4 p4 = *reinterpret_cast<const f32x4*>(pp + 4 * i), m4 = {}, v4 = {};
      if (HAS_M<ALGO>) m4 = *reinterpret_cast<const f32x4*>(mp + 4 * i);
      if (HAS_V<ALGO>) v4 = *reinterpret_cast<const f32x4*>(vp + 4 * i);
      g4 *= coef;
      moments_vec<ALGO>(d, g4, p4, m4, v4, lr, ss, bs);
      *reinterpret_cast<f32x4*>(pp + 4 * i) = p4;
      if (HAS_M<ALGO>) *reinterpret_cast<f32x4*>(mp + 4 * i) = m4;
      if (HAS_V<ALGO>) *reinterpret_cast<f32x4*>(vp + 4 * i) = v4;
    }
    for (long j = 4 * n4 + tid; j < n; j += 256) {
      float pe = pp[j], me = HAS_M<ALGO> ? mp[j] : 0.f, ve = HAS_V<ALGO> ? vp[j] : 0.f;
      moments_elem<ALGO>(d, gp[j] * coef, pe, me, ve, lr, ss, bs);
      pp[j] = pe;
      if (HAS_M<ALGO>) mp[j] = me;
      if (HAS_V<ALGO>) vp[j] = ve;
    }
  }
}

// Row policies of phase 0: a small struct in LDS.  DENSE = the ALGO dense_chunks runs with; COUNTS = a launch without zero_chunks
// counts the steps itself (there is no phase 1 behind it); scalars(d, lr) = the per-table scalars, by threads [64, 64 + Fs) of a row
// workgroup (the kernel synchronises); row(d, f, row, q, g4, lr) = quarter q of touched row `row` of table f, g4 = the clipped quarter
// of its summed gradient.  RowsOnly = what the policies that move the batch's rows alone start from.
struct RowsOnly {
  static constexpr int DENSE = NASREC_OPTIM_ADAM;
  static constexpr bool COUNTS = true;
  __device__ __forceinline__ void scalars(const nasrec_opt_moments_desc_t&, float) {}
};

// Adam / momentum SGD on every row: the touched rows here, marked in the bitmap, the others in phase 1 (which counts the steps)
template <int ALGO>
struct DenseRows {
  static constexpr int DENSE = ALGO;
  static constexpr bool COUNTS = false;
  float ss[NASREC_MAX_TABLES], bs[NASREC_MAX_TABLES];
  __device__ __forceinline__ void scalars(const nasrec_opt_moments_desc_t& d, float lr) { table_scalars<ALGO>(d, 64, lr, ss, bs); }
  __device__ __forceinline__ void row(const nasrec_opt_moments_desc_t& d, int f, long row, int q, const f32x4& g4, float lr) const {
    const long o = row * 16 + q * 4;
    f32x4 p4 = *reinterpret_cast<const f32x4*>(d.table[f] + o), m4 = *reinterpret_cast<const f32x4*>(d.tm[f] + o), v4 = {};
    if (ALGO == NASREC_OPTIM_ADAM) v4 = *reinterpret_cast<const f32x4*>(d.tv[f] + o);
    moments_vec<ALGO>(d, g4, p4, m4, v4, lr, ALGO == NASREC_OPTIM_ADAM ? ss[f] : 0.f, ALGO == NASREC_OPTIM_ADAM ? bs[f] : 1.f);
    *reinterpret_cast<f32x4*>(d.table[f] + o) = p4;
    *reinterpret_cast<f32x4*>(d.tm[f] + o) = m4;
    if (ALGO == NASREC_OPTIM_ADAM) *reinterpret_cast<f32x4*>(d.tv[f] + o) = v4;
    if (q == 0) atomicOr(d.bitmap + 2 * d.tile_off[f] + (row >> 5), 1u << (row & 31));  // (a set of bits: no value depends on the order)
  }
};

struct SparseAdamStepSizes : RowsOnly {  // (the per-table scalars of both row-sparse Adam policies)
  float ss[NASREC_MAX_TABLES];
  __device__ __forceinline__ void scalars(const nasrec_opt_moments_desc_t& d, float lr) {
    const int f = (int)threadIdx.x - 64;
    if (f >= 0 && f < d.Fs) ss[f] = sparse_adam_step_size(d, d.step[d.table_step0 + f], lr);
  }
};
// Row-sparse Adam (sparse_rows): a touched row takes torch.optim.SparseAdam's update with its summed gradient, zero or not; no bit is
// marked, and no other row moves.
struct SparseAdamRows : SparseAdamStepSizes {
  __device__ __forceinline__ void row(const nasrec_opt_moments_desc_t& d, int f, long row, int q, const f32x4& g4, float) const {
    const long o = row * 16 + q * 4;
    f32x4 p4 = *reinterpret_cast<const f32x4*>(d.table[f] + o), m4 = *reinterpret_cast<const f32x4*>(d.tm[f] + o);
    f32x4 v4 = *reinterpret_cast<const f32x4*>(d.tv[f] + o);
    const float step_size = ss[f];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float pe = p4[e], me = m4[e], ve = v4[e];
      sparse_adam_elem(d, g4[e], pe, me, ve, step_size);
      p4[e] = pe;
      m4[e] = me;
      v4[e] = ve;
    }
    *reinterpret_cast<f32x4*>(d.table[f] + o) = p4;
    *reinterpret_cast<f32x4*>(d.tm[f] + o) = m4;
    *reinterpret_cast<f32x4*>(d.tv[f] + o) = v4;
  }
};

// RMSprop (p / g / v): a touched row first pays the decay its square_avg owes since its stamp (lazy_decay, optimizer_bodies.h), then
// takes torch.optim.RMSprop's update with its summed gradient, and is stamped with this step; no bit is marked.  The four lanes of a
// row read its stamp before lane 0 writes it: they sit in one wavefront, and the store follows the loads in program order.
struct LazyRmspropRows : RowsOnly {
  static constexpr int DENSE = NASREC_OPTIM_RMSPROP;
  __device__ __forceinline__ void row(const nasrec_opt_moments_desc_t& d, int f, long row, int q, const f32x4& g4, float lr) const {
    const long o = row * 16 + q * 4;
    const long step = (long)d.step[d.table_step0 + f] + 1;
    const long n = step - 1 - (long)d.stamp[f][row];
    f32x4 p4 = *reinterpret_cast<const f32x4*>(d.table[f] + o), v4 = *reinterpret_cast<const f32x4*>(d.tv[f] + o), m4 = {};
#pragma unroll
    for (int e = 0; e < 4; ++e) v4[e] = lazy_decay(v4[e], d.beta2, n);
    moments_vec<NASREC_OPTIM_RMSPROP>(d, g4, p4, m4, v4, lr, 0.f, 1.f);
    *reinterpret_cast<f32x4*>(d.table[f] + o) = p4;
    *reinterpret_cast<f32x4*>(d.tv[f] + o) = v4;
    if (q == 0) d.stamp[f][row] = (uint32_t)step;
  }
};

// The split optimizer (table_algo = NASREC_TABLE_ALGO_ADAGRAD; Adam on the dense chunks): a touched row takes torch.optim.Adagrad's
// update with its summed gradient, at the tables' own learning rate lr * table_lr_scale and eps; tv holds the accumulator `sum`, tm is
// never read or written, no bit is marked.  A zero gradient leaves sum and W as they are (table_eps > 0: the quotient is an exact zero),
// so every row outside the batch AND a touched row whose gradient sums to zero keep their bits: exact, nothing is owed.
struct AdagradTableRows : RowsOnly {
  __device__ __forceinline__ void row(const nasrec_opt_moments_desc_t& d, int f, long row, int q, const f32x4& g4, float lr) const {
    const long o = row * 16 + q * 4;
    const float tlr = lr * d.table_lr_scale;
    f32x4 p4 = *reinterpret_cast<const f32x4*>(d.table[f] + o), s4 = *reinterpret_cast<const f32x4*>(d.tv[f] + o);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float pe = p4[e], se = s4[e];
      adagrad_elem(g4[e], se, pe, tlr, d.table_eps);
      p4[e] = pe;
      s4[e] = se;
    }
    *reinterpret_cast<f32x4*>(d.table[f] + o) = p4;
    *reinterpret_cast<f32x4*>(d.tv[f] + o) = s4;
  }
};

// Row-wise Adagrad on the tables (table_algo = NASREC_TABLE_ALGO_ROWWISE_ADAGRAD; Adam on the dense chunks): tv[f] holds ONE float per
// row, the accumulator of the mean of the row's squared gradient; sum += mean(g^2), then Adagrad's weight statement with that one sum
// for all 16 elements, at lr * table_lr_scale and table_eps.  A zero gradient leaves sum and W as they are, as with AdagradTableRows.
struct RowwiseAdagradTableRows : RowsOnly {
  __device__ __forceinline__ void row(const nasrec_opt_moments_desc_t& d, int f, long row, int q, const f32x4& g4, float lr) const {
    const long o = row * 16 + q * 4;
    const float tlr = lr * d.table_lr_scale;
    f32x4 p4 = *reinterpret_cast<const f32x4*>(d.table[f] + o);
    float s = d.tv[f][row];  // (all four lanes load it; lane q == 0 stores it below, after the loads in program order)
    const float sq = row_sum_of_squares(g4);
    s += sq * 0.0625f;  // (the mean of 16: an exact scaling)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float pe = p4[e];
      adagrad_weight(g4[e], s, pe, tlr, d.table_eps);
      p4[e] = pe;
    }
    *reinterpret_cast<f32x4*>(d.table[f] + o) = p4;
    if (q == 0) d.tv[f][row] = s;
  }
};

// The same rule on bfloat16 tables (table_algo = NASREC_TABLE_ALGO_ROWWISE_ADAGRAD_BF16): table[f] is [rows, 16] bfloat16 with 32-byte
// rows behind the float pointer; a lane loads its quarter's 8 bytes, widens it exactly (bits << 16), takes RowwiseAdagradTableRows'
// statements in fp32 and stores each new weight with stochastic rounding, out16 = (bits + r) >> 16, four results in one 8-byte store.
// r = the top 16 bits of a counter hash of (seed, t, f, row, e) (include/nasrec_hip.h; utils/optim.stochastic_round_bf16 is the
// definition): t is the table's step count after this step, read from the device counter, so the descriptor stays constant from step
// to step; the (seed, t, f) prefix of the chain is a per-table scalar in LDS.  A non-finite weight is stored truncated.  A weight that
// did not move has low bits zero and keeps its bits, so a zero gradient leaves the row alone as above.
__device__ __forceinline__ uint32_t sr_mix(uint32_t h) {
  h ^= h >> 16;
  h *= 0x7feb352du;
  h ^= h >> 15;
  h *= 0x846ca68bu;
  h ^= h >> 16;
  return h;
}
__device__ __forceinline__ uint32_t sr_round_bf16(float x, uint32_t h) {
  const uint32_t bits = __float_as_uint(x);
  const uint32_t r = (bits & 0x7f800000u) == 0x7f800000u ? 0u : sr_mix(h) >> 16;
  return (bits + r) >> 16;  // (a finite x is at most 0xff7fffff: the sum cannot wrap)
}

struct RowwiseAdagradBf16TableRows : RowsOnly {
  uint32_t prefix[NASREC_MAX_TABLES];
  __device__ __forceinline__ void scalars(const nasrec_opt_moments_desc_t& d, float) {
    const int f = (int)threadIdx.x - 64;
    if (f >= 0 && f < d.Fs) {
      const uint32_t seed = (uint32_t)(d.sr_seed ^ (d.sr_seed >> 32));
      const uint32_t t = (uint32_t)(long)d.step[d.table_step0 + f] + 1u;
      prefix[f] = sr_mix(sr_mix(seed ^ t * 0x9E3779B9u) ^ (uint32_t)f * 0x85EBCA6Bu);
    }
  }
  __device__ __forceinline__ void row(const nasrec_opt_moments_desc_t& d, int f, long row, int q, const f32x4& g4, float lr) const {
    const float tlr = lr * d.table_lr_scale;
    uint2* wp = reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(d.table[f]) + row * 16 + q * 4);
    const uint2 w = *wp;
    f32x4 p4 = {__uint_as_float(w.x << 16), __uint_as_float(w.x & 0xffff0000u), __uint_as_float(w.y << 16), __uint_as_float(w.y & 0xffff0000u)};
    float s = d.tv[f][row];  // (all four lanes load it; lane q == 0 stores it below, after the loads in program order)
    const float sq = row_sum_of_squares(g4);
    s += sq * 0.0625f;
    const uint32_t h = prefix[f], pos = (uint32_t)row * 16u + (uint32_t)q * 4u;  // (row * 16 + e may wrap in 32 bits: part of the definition)
    uint32_t o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float pe = p4[e];
      adagrad_weight(g4[e], s, pe, tlr, d.table_eps);
      o[e] = sr_round_bf16(pe, h ^ (pos + (uint32_t)e));
    }
    *wp = make_uint2(o[0] | (o[1] << 16), o[2] | (o[3] << 16));
    if (q == 0) d.tv[f][row] = s;
  }
};

// Row-wise row-sparse Adam (table_algo = NASREC_TABLE_ALGO_ROWWISE_ADAM; Adam on the dense chunks): SparseAdamRows with ONE second
// moment per row.  tm[f] is [rows, 16] as there; tv[f] holds one float per row, the moving average of the mean of the row's squared
// gradient (row_sum_of_squares, under its invariant), and divides the whole row.  The statements and the step size are
// SparseAdamRows'.  A touched row moves with its summed gradient, zero or not; no bit is marked, and no other row moves.
struct RowwiseSparseAdamRows : SparseAdamStepSizes {
  __device__ __forceinline__ void row(const nasrec_opt_moments_desc_t& d, int f, long row, int q, const f32x4& g4, float) const {
    const long o = row * 16 + q * 4;
    f32x4 p4 = *reinterpret_cast<const f32x4*>(d.table[f] + o), m4 = *reinterpret_cast<const f32x4*>(d.tm[f] + o);
    float v = d.tv[f][row];  // (all four lanes load it; lane q == 0 stores it below, after the loads in program order)
    const float sq = row_sum_of_squares(g4);
    const float w1 = (float)(1.0 - d.beta1), w2 = (float)(1.0 - d.beta2), step_size = ss[f];
    const float den = sparse_adam_second_moment(w2, d.eps, sq * 0.0625f, v);  // (the mean of 16: an exact scaling)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float pe = p4[e], me = m4[e];
      sparse_adam_first_moment(w1, g4[e], me);
      sparse_adam_weight(me, den, pe, step_size);
      p4[e] = pe;
      m4[e] = me;
    }
    *reinterpret_cast<f32x4*>(d.table[f] + o) = p4;
    *reinterpret_cast<f32x4*>(d.tm[f] + o) = m4;
    if (q == 0) d.tv[f][row] = v;
  }
};

template <class Rows>
__global__ __launch_bounds__(256) void opt_moments_phase0_kernel(const nasrec_opt_moments_desc_t d) {
  __shared__ float sh_coef;
  __shared__ Rows rows;
  const int tid = threadIdx.x, blk = blockIdx.x;
  const float lr = *d.lr;
  clip_head(d.clip, &sh_coef);
  if (blk >= d.dense_blocks) rows.scalars(d, lr);
  __syncthreads();
  const float coef = sh_coef;
  if (blk < d.dense_blocks) {
    dense_chunks<Rows::DENSE>(d, coef, lr);
  } else {
    // touched rows: 4 lanes x float4 per (sample, field) pair; the leader of a row id carries the row's summed gradient
    const long t = (long)(blk - d.dense_blocks) * 256 + tid;
    const long pair = t >> 2;
    const int q = (int)(t & 3);
    if (pair < (long)d.B * d.Fs && d.leader[pair]) {
      const int f = (int)(pair % d.Fs);
      const long row = d.idx[pair];
      if (row >= 0 && row < d.rows[f]) {  // (flagged by the gather; never written outside a table)
        f32x4 g4 = *reinterpret_cast<const f32x4*>(d.gsum + gsum_row_offset(pair, d.Fs, d.rank_B, d.rank_stride) + q * 4);
        g4 *= coef;
        rows.row(d, f, row, q, g4, lr);
      }
    }
  }
  if (!Rows::COUNTS || d.n_zero > 0) return;  // (phase 1 counts; with zero_chunks it also restores g over them)
  count_steps_in_last_workgroup(d, gridDim.x);
}

// RMSprop's flush (phase 2): every row of every table whose stamp lies behind its table's step count pays the decay it owes and is
// stamped current; a second flush finds nothing to do.  The bitmap is all zero and only read (untouched_rows_pass hands over every row).
struct FlushRows {
  const nasrec_opt_moments_desc_t& d;
  long n[TABLE_PASS_UNROLL];
  uint32_t now[TABLE_PASS_UNROLL];
  f32x4 v[TABLE_PASS_UNROLL];
  __device__ __forceinline__ void load(int u, int f, long off) {
    now[u] = (uint32_t)d.step[d.table_step0 + f];
    n[u] = (long)now[u] - (long)d.stamp[f][off >> 4];
    if (n[u] > 0) v[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(d.tv[f] + off));
  }
  __device__ __forceinline__ void update(int u, int f, long off) {
    if (n[u] <= 0) return;
    const double k = pow(d.beta2, (double)n[u]);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[u][e] = (float)((double)v[u][e] * k);
    __builtin_nontemporal_store(v[u], reinterpret_cast<f32x4*>(d.tv[f] + off));
    if ((off & 15) == 0) d.stamp[f][off >> 4] = now[u];
  }
};

__global__ __launch_bounds__(256) void opt_moments_flush_kernel(const nasrec_opt_moments_desc_t d) {
  FlushRows r{d};
  untouched_rows_pass(d.tile_off, d.rows, d.Fs, d.bitmap, blockIdx.x, d.nblocks, r);
}

// phase 1's row update: the optimizer with g = 0, or g = 2 wd W * coef on a regularised table (untouched_rows_pass, optimizer_bodies.h)
template <int ALGO>
struct MomentRows {
  const nasrec_opt_moments_desc_t& d;
  const float lr, coef, two_r;
  const float* ss;
  const float* bs;
  f32x4 w[TABLE_PASS_UNROLL], m[TABLE_PASS_UNROLL], v[TABLE_PASS_UNROLL];
  __device__ __forceinline__ void load(int u, int f, long off) {
    w[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(d.table[f] + off));
    if (HAS_M<ALGO>) m[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(d.tm[f] + off));
    if (HAS_V<ALGO>) v[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(d.tv[f] + off));
  }
  __device__ __forceinline__ void update(int u, int f, long off) {
    f32x4 g = {0.f, 0.f, 0.f, 0.f};
    if ((d.reg_mask >> f) & 1u) {
#pragma unroll
      for (int e = 0; e < 4; ++e) g[e] = (two_r * w[u][e]) * coef;
    }
    moments_vec<ALGO>(d, g, w[u], m[u], v[u], lr, ALGO == NASREC_OPTIM_ADAM ? ss[f] : 0.f, ALGO == NASREC_OPTIM_ADAM ? bs[f] : 1.f);
    __builtin_nontemporal_store(w[u], reinterpret_cast<f32x4*>(d.table[f] + off));
    if (HAS_M<ALGO>) __builtin_nontemporal_store(m[u], reinterpret_cast<f32x4*>(d.tm[f] + off));
    if (HAS_V<ALGO>) __builtin_nontemporal_store(v[u], reinterpret_cast<f32x4*>(d.tv[f] + off));
  }
};

template <int ALGO>
__global__ __launch_bounds__(256) void opt_moments_phase1_kernel(const nasrec_opt_moments_desc_t d) {
  __shared__ float t_ss[NASREC_MAX_TABLES], t_bs[NASREC_MAX_TABLES];
  const int tid = threadIdx.x, blk = blockIdx.x, nblk = d.nblocks;
  const float lr = *d.lr, coef = *d.coef, two_r = 2.f * d.wd;
  table_scalars<ALGO>(d, 0, lr, t_ss, t_bs);
  // weight decay's unreached regularised ranges: their gradient (g = 2 wd W, read by phase 0) goes back to zero
  for (long c = blk; c < d.n_zero; c += nblk) {
    const long off = d.zero_chunks[2 * c], n = d.zero_chunks[2 * c + 1];
    for (long i = tid; i < n; i += 256) d.g[off + i] = 0.f;
  }
  __syncthreads();
  MomentRows<ALGO> r{d, lr, coef, two_r, t_ss, t_bs};
  untouched_rows_pass(d.tile_off, d.rows, d.Fs, d.bitmap, blk, nblk, r);
  // the step counters move once every workgroup has read them (phase 0 read them in the launch before)
  count_steps_in_last_workgroup(d, (unsigned)nblk);
}

template <class Rows>
void launch_phase0(hipStream_t st, const nasrec_opt_moments_desc_t* d, int nblk) {
  hipLaunchKernelGGL(opt_moments_phase0_kernel<Rows>, dim3((unsigned)nblk), dim3(256), 0, st, *d);
}

template <int ALGO>
void launch_phase1(hipStream_t st, const nasrec_opt_moments_desc_t* d) {
  hipLaunchKernelGGL(opt_moments_phase1_kernel<ALGO>, dim3((unsigned)d->nblocks), dim3(256), 0, st, *d);
}

// The row forms: what a launch does to the tables, one line each; launch_opt_moments reads nothing else about a form.  algo,
// sparse_rows, table_algo = the descriptors that take it; name = how the refusals call a rows-only form.  ROWS_ONLY = it moves the
// batch's rows only, so its phase 0 counts the steps unless zero_chunks call for a phase 1, which then owns no tile (the dense forms
// move every row: bitmap + phase 1); OWN_TM = a rule of the tables' own whose rows read tm[f] as a first moment; TV_PER_ROW = tv[f] is
// one float per row, not [rows, 16] (for the reader: a length cannot be checked here); STAMPS = per-row stamps in tm's storage; BF16 =
// table[f] is bfloat16, tm[0]'s storage the seed; EPS_POSITIVE = table_eps > 0 (a zero gradient must leave its row alone).
enum : unsigned { ROWS_ONLY = 1, OWN_TM = 2, TV_PER_ROW = 4, STAMPS = 8, BF16 = 16, EPS_POSITIVE = 32 };
struct RowForm {
  int algo, sparse_rows, table_algo;
  const char* name;
  unsigned flags;
  int last_phase;  // (2 = the flush)
  void (*phase0)(hipStream_t, const nasrec_opt_moments_desc_t*, int);
  void (*phase1)(hipStream_t, const nasrec_opt_moments_desc_t*);  // (null: no phase 1, which last_phase says too)
};
constexpr int ADAM = NASREC_OPTIM_ADAM, SGD = NASREC_OPTIM_SGD, RMSPROP = NASREC_OPTIM_RMSPROP, SAME = NASREC_TABLE_ALGO_SAME;
constexpr RowForm ROW_FORMS[] = {
    {ADAM, 0, SAME, "", 0, 1, launch_phase0<DenseRows<ADAM>>, launch_phase1<ADAM>},
    {SGD, 0, SAME, "", 0, 1, launch_phase0<DenseRows<SGD>>, launch_phase1<SGD>},
    {ADAM, 1, SAME, "sparse_rows", ROWS_ONLY, 1, launch_phase0<SparseAdamRows>, launch_phase1<ADAM>},
    {RMSPROP, 0, SAME, "RMSprop", ROWS_ONLY | STAMPS, 2, launch_phase0<LazyRmspropRows>, launch_phase1<RMSPROP>},
    {ADAM, 0, NASREC_TABLE_ALGO_ADAGRAD, "table_algo", ROWS_ONLY | EPS_POSITIVE, 1, launch_phase0<AdagradTableRows>, launch_phase1<ADAM>},
    {ADAM, 0, NASREC_TABLE_ALGO_ROWWISE_ADAGRAD, "table_algo", ROWS_ONLY | TV_PER_ROW | EPS_POSITIVE, 1, launch_phase0<RowwiseAdagradTableRows>, launch_phase1<ADAM>},
    {ADAM, 0, NASREC_TABLE_ALGO_ROWWISE_ADAGRAD_BF16, "table_algo", ROWS_ONLY | TV_PER_ROW | BF16 | EPS_POSITIVE, 0, launch_phase0<RowwiseAdagradBf16TableRows>, nullptr},
    {ADAM, 0, NASREC_TABLE_ALGO_ROWWISE_ADAM, "table_algo", ROWS_ONLY | TV_PER_ROW | OWN_TM, 1, launch_phase0<RowwiseSparseAdamRows>, launch_phase1<ADAM>},
};

// (algo, sparse_rows, table_algo) -> the row form, or a refusal (its return code; 0 = *form is set).  A table_algo other than SAME is a
// rule of the tables' own: it goes with Adam on the rest and without sparse_rows, and its refusals come first.
int resolve_row_form(const nasrec_opt_moments_desc_t* d, const RowForm** form) {
  bool known = false;
  *form = nullptr;
  for (const RowForm& r : ROW_FORMS) {
    known |= r.table_algo == d->table_algo;
    if (r.algo == d->algo && r.sparse_rows == (d->sparse_rows != 0) && r.table_algo == d->table_algo) *form = &r;
  }
  const bool adam = d->algo == ADAM, own = d->table_algo != SAME;
  if (!known) return nasrec_set_error(-1, "opt_moments: table_algo %d", d->table_algo);
  if (own && !adam)
    return nasrec_set_error(-1, "opt_moments: table_algo %d (a rule of their own on the tables) goes with Adam on the rest (algo %d)", d->table_algo, d->algo);
  if (own && d->sparse_rows) return nasrec_set_error(-1, "opt_moments: table_algo with sparse_rows: the tables take one rule");
  if (d->algo == RMSPROP && d->momentum != 0.f) return nasrec_set_error(-1, "opt_moments: RMSprop with momentum %g moves untouched rows", (double)d->momentum);
  if (d->sparse_rows && !adam) return nasrec_set_error(-1, "opt_moments: sparse_rows is row-sparse Adam (algo %d)", d->algo);
  return *form ? 0 : nasrec_set_error(-1, "opt_moments: algo %d", d->algo);
}

}  // namespace

// Every refusal comes before anything is launched, in one order: the form's (resolve_row_form), then what the form's flags ask of the
// descriptor, then the phase's.
int launch_opt_moments(hipStream_t st, const nasrec_opt_moments_desc_t* d) {
  if (d->Fs < 0 || d->Fs > NASREC_MAX_TABLES) return nasrec_set_error(-1, "opt_moments: Fs = %d", d->Fs);
  if (!d->lr || !d->step) return nasrec_set_error(-1, "opt_moments: lr / step missing");
  const RowForm* form;
  if (const int rc = resolve_row_form(d, &form)) return rc;
  const RowForm& r = *form;
  const bool rows_only = r.flags & ROWS_ONLY, bf16 = r.flags & BF16, own = d->table_algo != SAME;  // (own: the tables take a rule of their own)
  if ((r.flags & EPS_POSITIVE) && !(d->table_eps > 0.f))
    return nasrec_set_error(-1, "opt_moments: table_eps %g must be positive (a zero gradient must leave its row alone)", (double)d->table_eps);
  if (own && d->reg_mask != 0u)
    return nasrec_set_error(-1, "opt_moments: table_algo with reg_mask %u: a regularised table moves in every row", d->reg_mask);
  if (bf16 && d->phase != 0)
    return nasrec_set_error(-1, "opt_moments: table_algo %d (bf16 tables) has phase 0 only: phase %d knows fp32 tables", d->table_algo, d->phase);
  for (int f = 1; bf16 && f < NASREC_MAX_TABLES; ++f)  // (a caller that filled tm expects a first moment: there is none, and tm[0] is the seed)
    if (d->tm[f]) return nasrec_set_error(-1, "opt_moments: table_algo %d (bf16 tables) keeps the seed in tm[0]'s storage and takes no tm (tm[%d] is set)", d->table_algo, f);
  if (d->phase < 0 || d->phase > r.last_phase || (d->phase == 1 && !r.phase1)) return nasrec_set_error(-1, "opt_moments: phase %d", d->phase);
  for (int f = 0; (r.flags & STAMPS) && f < d->Fs; ++f)
    if (!d->stamp[f] || !d->tv[f]) return nasrec_set_error(-1, "opt_moments: RMSprop without the stamps / square_avg of table %d", f);
  if (d->phase == 0) {
    const long threads = (long)d->B * d->Fs * 4;
    const int nrows = (int)((threads + 255) / 256), nblk = d->dense_blocks + nrows;
    if (d->dense_blocks < 0 || nblk < 1) return nasrec_set_error(-2, "opt_moments: empty launch");
    if (nrows > 0 && (!d->idx || !d->leader || !d->gsum || (!d->bitmap && !rows_only))) return nasrec_set_error(-1, "opt_moments: row inputs missing");
    for (int f = 0; own && nrows > 0 && f < d->Fs; ++f) {
      if (!d->table[f] || !d->tv[f]) return nasrec_set_error(-1, "opt_moments: table_algo without the weights / accumulator (tv) of table %d", f);
      if ((r.flags & OWN_TM) && !d->tm[f]) return nasrec_set_error(-1, "opt_moments: table_algo %d (row-wise Adam) without the first moment (tm) of table %d", d->table_algo, f);
    }
    if (d->rank_B < 0 || (d->rank_B > 0 && (d->rank_stride < (int64_t)d->rank_B * d->Fs * 16 || d->B % d->rank_B != 0)))
      return nasrec_set_error(-2, "opt_moments: rank layout %d / %ld", d->rank_B, (long)d->rank_stride);
    if (rows_only && d->n_zero <= 0 && (!d->counter || (d->n_inc > 0 && !d->inc)))
      return nasrec_set_error(-1, "opt_moments: %s without zero_chunks counts the steps: counter / inc missing", r.name);
    r.phase0(st, d, nblk);
  } else if (d->phase == 1) {
    if (d->nblocks <= 0) return nasrec_set_error(-1, "opt_moments: nblocks must be positive");
    if (!d->bitmap || !d->counter || !d->coef) return nasrec_set_error(-1, "opt_moments: phase 1 inputs missing");
    if (rows_only && (d->n_zero <= 0 || d->tile_off[d->Fs] != 0))
      return nasrec_set_error(-1, "opt_moments: %s has a phase 1 only to restore zero_chunks, and no table owns a tile", r.name);
    r.phase1(st, d);
  } else {
    if (d->nblocks <= 0 || !d->bitmap) return nasrec_set_error(-1, "opt_moments: flush needs nblocks > 0 and the (all-zero) bitmap");
    if (d->tile_off[d->Fs] <= 0) return 0;
    hipLaunchKernelGGL(opt_moments_flush_kernel, dim3((unsigned)d->nblocks), dim3(256), 0, st, *d);
  }
  return nasrec_check_launch("opt_moments");
}
