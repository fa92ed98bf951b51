// Exponential moving average of the weights (NASREC_OP_WEIGHT_EMA, include/nasrec_hip.h; utils/optim.WeightEMA): the dense statement
// s = fmaf(w, p - s, s) on the dense arena and on the batch's table rows after every optimizer step.  A table row outside the batch
// rests, and its average obeys s <- p + decay^n (s - p) over n resting steps: per-row stamps record when a row's average is current,
// phase 0 pays what the batch's rows owe BEFORE the optimizer moves them, phase 1 averages them after it, and the flush (phase 2) and
// the exchange (phase 3, flush + p <-> s) walk every row for whoever reads the averaged weights.  Its own launches in the optimizer
// tail: no optimizer kernel knows of it.
#include "optimizer_bodies.h"

namespace {

// what a row (or element) whose weights rested for n > 0 updates owes: fp64, rounded once
__device__ __forceinline__ float ema_catch_up(float p, float s, double k) { return (float)((double)p + k * ((double)s - (double)p)); }

__device__ __forceinline__ void ema_vec(f32x4& s, const f32x4& p, float w) {
#pragma unroll
  for (int e = 0; e < 4; ++e) s[e] = fmaf(w, p[e] - s[e], s[e]);
}

// leader rows of the batch: 4 lanes x float4 per (sample, field) pair, thread t of the row workgroups.  UPDATE = phase 1's dense
// statement and stamp = count + 1; else phase 0's catch-up.  The four lanes of a row read its stamp before lane 0 writes it: they sit
// in one wavefront, and the store follows the loads in program order.
// Two memory round trips, as in adagrad_rows_body (optimizer_bodies.h): what does not depend on the row id — leader flag, id, the
// field's row count and its three base pointers (per-lane loads from the argument arrays) — is issued together, then the row's stamp,
// weights and average together.
template <bool UPDATE>
__device__ __forceinline__ void ema_batch_rows(const nasrec_weight_ema_desc_t& d, long t, uint32_t count) {
  const long pair = t >> 2;
  const int q = (int)(t & 3);
  if (pair >= (long)d.B * d.Fs) return;
  const int f = (int)(pair % d.Fs);
  const int lead = d.leader[pair];
  const long row = d.idx[pair];
  const long nrows = d.rows[f];
  const float* const tbase = d.table[f];
  float* const sbase = d.shadow[f];
  uint32_t* const stbase = d.stamp[f];
  asm volatile("" ::"v"(lead), "v"((int)row), "v"((int)nrows), "v"(tbase), "v"(sbase), "v"(stbase));  // (all six in flight before the first test)
  if (!lead) return;
  if (row < 0 || row >= nrows) return;  // (flagged by the gather; never read or written outside a table)
  const long o = row * 16 + q * 4;
  const uint32_t stamp = stbase[row];
  const f32x4 p4 = *reinterpret_cast<const f32x4*>(tbase + o);
  f32x4 s4 = *reinterpret_cast<const f32x4*>(sbase + o);
  if (UPDATE) {
    ema_vec(s4, p4, (float)(1.0 - d.decay));
    *reinterpret_cast<f32x4*>(sbase + o) = s4;
    if (q == 0) stbase[row] = count + 1u;
  } else {
    const long n = (long)count - (long)stamp;
    if (n <= 0) return;  // (current: a row in every batch keeps the bits of the dense statement)
    const double k = pow(d.decay, (double)n);
#pragma unroll
    for (int e = 0; e < 4; ++e) s4[e] = ema_catch_up(p4[e], s4[e], k);
    *reinterpret_cast<f32x4*>(sbase + o) = s4;
    if (q == 0) stbase[row] = count;
  }
}

__global__ __launch_bounds__(256) void weight_ema_catch_up_kernel(const nasrec_weight_ema_desc_t d) {
  ema_batch_rows<false>(d, (long)blockIdx.x * 256 + threadIdx.x, *d.count);
}

// phase 1: workgroups [0, dense_blocks) on the whole dense arena (float4 pieces, the tail in workgroup 0), the others on the leader
// rows; the workgroup that arrives last at d.counter counts the update (count_steps_in_last_workgroup's pattern, csrc/optim_moments.hip:
// every workgroup has read *count when it arrives, and the counter is left zero for the next launch or replay)
__global__ __launch_bounds__(256) void weight_ema_update_kernel(const nasrec_weight_ema_desc_t d) {
  __shared__ int last;
  const int tid = threadIdx.x, blk = blockIdx.x;
  const uint32_t count = *d.count;
  if (blk < d.dense_blocks) {
    const float w = (float)(1.0 - d.decay);
    const long n4 = d.n >> 2, stride = (long)d.dense_blocks * 256;
    long i = (long)blk * 256 + tid;
    for (; i + stride < n4; i += 2 * stride) {  // two pieces per trip, their four loads in flight together
      const f32x4 pa = *reinterpret_cast<const f32x4*>(d.p + 4 * i), pb = *reinterpret_cast<const f32x4*>(d.p + 4 * (i + stride));
      f32x4 sa = *reinterpret_cast<const f32x4*>(d.s + 4 * i), sb = *reinterpret_cast<const f32x4*>(d.s + 4 * (i + stride));
      ema_vec(sa, pa, w);
      ema_vec(sb, pb, w);
      *reinterpret_cast<f32x4*>(d.s + 4 * i) = sa;
      *reinterpret_cast<f32x4*>(d.s + 4 * (i + stride)) = sb;
    }
    if (i < n4) {
      const f32x4 p4 = *reinterpret_cast<const f32x4*>(d.p + 4 * i);
      f32x4 s4 = *reinterpret_cast<const f32x4*>(d.s + 4 * i);
      ema_vec(s4, p4, w);
      *reinterpret_cast<f32x4*>(d.s + 4 * i) = s4;
    }
    const long j = 4 * n4 + tid;
    if (blk == 0 && j < d.n) d.s[j] = fmaf(w, d.p[j] - d.s[j], d.s[j]);
  } else {
    ema_batch_rows<true>(d, (long)(blk - d.dense_blocks) * 256 + tid, count);
  }
  // The arrival is a relaxed add without fences: nothing a workgroup WROTE is read in this launch.  All that has to come first is its
  // threads' read of *count, and a thread that uses the value (the stamp store) has it in a register before the barrier.  A release
  // fence per workgroup in front of the arrival made this launch 41 us instead of 17.5 (cfg-2 arena, profiles/optim_step_cfg2.txt).
  __syncthreads();
  if (tid == 0) last = __hip_atomic_fetch_add(d.counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1u;
  __syncthreads();
  if (!last || tid != 0) return;
  *d.count = count + 1u;
  *d.counter = 0u;
}

// the table pass of the flush and of the exchange (untouched_rows_pass hands over every row: the bitmap is all zero and only read)
template <bool SWAP>
struct EmaTableRows {
  const nasrec_weight_ema_desc_t& d;
  const uint32_t count;
  long n[TABLE_PASS_UNROLL];
  f32x4 p[TABLE_PASS_UNROLL], s[TABLE_PASS_UNROLL];
  __device__ __forceinline__ void load(int u, int f, long off) {
    n[u] = (long)count - (long)d.stamp[f][off >> 4];
    if (SWAP || n[u] > 0) {
      p[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(d.table[f] + off));
      s[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(d.shadow[f] + off));
    }
  }
  __device__ __forceinline__ void update(int u, int f, long off) {
    if (n[u] > 0) {
      const double k = pow(d.decay, (double)n[u]);
#pragma unroll
      for (int e = 0; e < 4; ++e) s[u][e] = ema_catch_up(p[u][e], s[u][e], k);
      if ((off & 15) == 0) d.stamp[f][off >> 4] = count;
    }
    if (SWAP) {
      __builtin_nontemporal_store(s[u], reinterpret_cast<f32x4*>(d.table[f] + off));
      __builtin_nontemporal_store(p[u], reinterpret_cast<f32x4*>(d.shadow[f] + off));
    } else if (n[u] > 0) {
      __builtin_nontemporal_store(s[u], reinterpret_cast<f32x4*>(d.shadow[f] + off));
    }
  }
};

__global__ __launch_bounds__(256) void weight_ema_flush_kernel(const nasrec_weight_ema_desc_t d) {
  EmaTableRows<false> r{d, *d.count};
  untouched_rows_pass(d.tile_off, d.rows, d.Fs, d.bitmap, blockIdx.x, d.nblocks, r);
}

// phase 3: workgroups [0, dense_blocks) exchange the dense arena with its shadow, the other nblocks flush and exchange the tables
__global__ __launch_bounds__(256) void weight_ema_exchange_kernel(const nasrec_weight_ema_desc_t d) {
  const int tid = threadIdx.x, blk = blockIdx.x;
  if (blk < d.dense_blocks) {
    const long n4 = d.n >> 2, stride = (long)d.dense_blocks * 256;
    for (long i = (long)blk * 256 + tid; i < n4; i += stride) {
      const f32x4 p4 = *reinterpret_cast<const f32x4*>(d.p + 4 * i), s4 = *reinterpret_cast<const f32x4*>(d.s + 4 * i);
      *reinterpret_cast<f32x4*>(d.p + 4 * i) = s4;
      *reinterpret_cast<f32x4*>(d.s + 4 * i) = p4;
    }
    const long j = 4 * n4 + tid;
    if (blk == 0 && j < d.n) {
      const float pe = d.p[j], se = d.s[j];
      d.p[j] = se;
      d.s[j] = pe;
    }
    return;
  }
  EmaTableRows<true> r{d, *d.count};
  untouched_rows_pass(d.tile_off, d.rows, d.Fs, d.bitmap, blk - d.dense_blocks, d.nblocks, r);
}

}  // namespace

// Every refusal comes before anything is launched.
int launch_weight_ema(hipStream_t st, const nasrec_weight_ema_desc_t* d) {
  if (d->Fs < 0 || d->Fs > NASREC_MAX_TABLES) return nasrec_set_error(-1, "weight_ema: Fs = %d", d->Fs);
  if (d->phase < 0 || d->phase > 3) return nasrec_set_error(-1, "weight_ema: phase %d", d->phase);
  if (!(d->decay > 0.0 && d->decay < 1.0)) return nasrec_set_error(-1, "weight_ema: decay %g is not inside (0, 1)", d->decay);
  for (int f = 0; f < d->Fs; ++f)
    if (!d->stamp[f] || !d->shadow[f] || !d->table[f] || d->rows[f] < 0)
      return nasrec_set_error(-1, "weight_ema: table %d without its weights, shadow or stamps", f);
  if (!d->count) return nasrec_set_error(-1, "weight_ema: count missing");
  if (d->B < 0 || d->n < 0 || d->dense_blocks < 0) return nasrec_set_error(-1, "weight_ema: B %d, n %ld, dense_blocks %d", d->B, (long)d->n, d->dense_blocks);
  if (d->n > 0 && (!d->p || !d->s)) return nasrec_set_error(-1, "weight_ema: dense arena or its shadow missing");
  const long row_threads = (long)d->B * d->Fs * 4;
  const int nrows = (int)((row_threads + 255) / 256);
  if (d->phase <= 1 && nrows > 0 && (!d->idx || !d->leader)) return nasrec_set_error(-1, "weight_ema: ids / leaders missing");
  if (d->phase == 0) {
    if (nrows == 0) return 0;
    hipLaunchKernelGGL(weight_ema_catch_up_kernel, dim3((unsigned)nrows), dim3(256), 0, st, *d);
  } else if (d->phase == 1) {
    if (!d->counter) return nasrec_set_error(-1, "weight_ema: counter missing");
    if (d->n > 0 && d->dense_blocks < 1) return nasrec_set_error(-1, "weight_ema: a dense arena and no workgroup for it");
    const int nblk = d->dense_blocks + nrows;  // (an empty launch still counts the update: one workgroup)
    hipLaunchKernelGGL(weight_ema_update_kernel, dim3((unsigned)(nblk > 0 ? nblk : 1)), dim3(256), 0, st, *d);
  } else {
    const bool tiles = d->tile_off[d->Fs] > 0;
    if (tiles && (d->nblocks <= 0 || !d->bitmap)) return nasrec_set_error(-1, "weight_ema: the table pass needs nblocks > 0 and the (all-zero) bitmap");
    if (d->phase == 2) {
      if (!tiles) return 0;
      hipLaunchKernelGGL(weight_ema_flush_kernel, dim3((unsigned)d->nblocks), dim3(256), 0, st, *d);
    } else {
      if (d->n > 0 && d->dense_blocks < 1) return nasrec_set_error(-1, "weight_ema: a dense arena and no workgroup for it");
      const int nblk = d->dense_blocks + (tiles ? d->nblocks : 0);
      if (nblk <= 0) return 0;
      hipLaunchKernelGGL(weight_ema_exchange_kernel, dim3((unsigned)nblk), dim3(256), 0, st, *d);
    }
  }
  return nasrec_check_launch("weight_ema");
}
