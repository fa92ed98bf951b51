// Decoupled weight decay (NASREC_OP_DECOUPLED_DECAY, include/nasrec_hip.h; utils/optim.DecoupledWeightDecay): the dense statement
// p = p * (float)(1 - lr lambda) on the selected ranges of the dense arena and on the batch's table rows, in front of the optimizer's
// update.  A table row outside the batch receives nothing else, so it rests and owes the product of the factors it missed: level[f]
// is the running sum of log1p(-lr lambda) of table f, a row's stamp the fp32 value of the level at which its weights are current.
// Phase 0 pays what the batch's rows owe BEFORE the gather reads them, phase 1 decays them with the dense arena, and the flush
// (phase 2) walks every row for whoever reads the tables and re-bases stamps and levels to 0.  Its own launches: no optimizer kernel
// knows of it.
#include "optimizer_bodies.h"

namespace {

// log of one step's factor, and a level advanced by it: __dadd_rn keeps the sum out of any contraction, so the row workgroups (the
// new stamps) and the last workgroup (the new level) round the same value
__device__ __forceinline__ double decay_log_step(float lr, double lambda) { return log1p(-((double)lr * lambda)); }
__device__ __forceinline__ double decay_next_level(double level, double log_step) { return __dadd_rn(level, log_step); }

__device__ __forceinline__ void decay_scale(f32x4& w, double k) {
#pragma unroll
  for (int e = 0; e < 4; ++e) w[e] = (float)((double)w[e] * k);  // (fp64, rounded once)
}

// phase 0: 4 lanes x float4 per (sample, field) pair of the raw ids.  The claim: lane 0 exchanges the row's stamp with the current
// level; among the pairs that carry one row exactly one reads a stamp that is not current, and that pair alone multiplies the row.
// The four lanes of a pair sit side by side in one wavefront and take the same branches, so lane 0 is active whenever the others ask
// for its value.
__global__ __launch_bounds__(256) void decoupled_decay_catch_up_kernel(const nasrec_decoupled_decay_desc_t d) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  const long pair = t >> 2;
  const int q = (int)(t & 3);
  if (pair >= (long)d.B * d.Fs) return;
  const int f = (int)(pair % d.Fs);
  if (!((d.mask >> f) & 1u)) return;
  const long row = d.idx[pair];
  if (row < 0 || row >= d.rows[f]) return;  // (flagged by the gather; never read or written outside a table)
  const double level = d.level[f];
  const float now = (float)level;
  float old = now;
  if (q == 0) old = __uint_as_float(atomicExch(reinterpret_cast<unsigned int*>(d.stamp[f] + row), __float_as_uint(now)));
  old = __shfl(old, (int)(threadIdx.x & 63u) & ~3);
  if (__float_as_uint(old) == __float_as_uint(now)) return;  // (current, or claimed by another pair of this launch)
  f32x4* const wp = reinterpret_cast<f32x4*>(d.table[f] + row * 16 + q * 4);
  f32x4 w = *wp;
  decay_scale(w, exp(level - (double)old));
  *wp = w;
}

// phase 1: workgroups [0, dense_blocks) on the chunks of the dense arena (float4 pieces where the chunk starts on 16 bytes), the
// others on the leader rows.  With rows in the launch, the workgroup that arrives last at d.counter advances the levels
// (weight_ema_update_kernel's pattern, csrc/weight_ema.hip: a relaxed arrival — nothing a workgroup WROTE is read in this launch, and
// a thread that uses a level has it in a register before the barrier; the counter is left zero for the next launch or replay).
__global__ __launch_bounds__(256) void decoupled_decay_step_kernel(const nasrec_decoupled_decay_desc_t d) {
  __shared__ int last;
  const int tid = threadIdx.x, blk = blockIdx.x;
  const float lr = *d.lr;
  const float factor = (float)(1.0 - (double)lr * d.lambda);
  if (blk < d.dense_blocks) {
    for (long c = blk; c < d.n_chunks; c += d.dense_blocks) {
      const long off = d.chunks[2 * c], n = d.chunks[2 * c + 1];
      float* const p = d.p + off;
      if ((off & 3) == 0) {
        const long n4 = n >> 2;
        for (long i = tid; i < n4; i += 256) {
          f32x4 w = *reinterpret_cast<const f32x4*>(p + 4 * i);
#pragma unroll
          for (int e = 0; e < 4; ++e) w[e] *= factor;
          *reinterpret_cast<f32x4*>(p + 4 * i) = w;
        }
        for (long j = 4 * n4 + tid; j < n; j += 256) p[j] *= factor;
      } else {
        for (long j = tid; j < n; j += 256) p[j] *= factor;
      }
    }
  } else {
    const long t = (long)(blk - d.dense_blocks) * 256 + tid;
    const long pair = t >> 2;
    const int q = (int)(t & 3);
    if (pair < (long)d.B * d.Fs) {
      const int f = (int)(pair % d.Fs);
      const long row = d.idx[pair];
      if (((d.mask >> f) & 1u) && d.leader[pair] && row >= 0 && row < d.rows[f]) {
        const float stamp = (float)decay_next_level(d.level[f], decay_log_step(lr, d.lambda));
        f32x4* const wp = reinterpret_cast<f32x4*>(d.table[f] + row * 16 + q * 4);
        f32x4 w = *wp;
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] *= factor;
        *wp = w;
        if (q == 0) d.stamp[f][row] = stamp;
      }
    }
  }
  if (d.B == 0) return;  // (no gradient reaches the tables: no level moves, nobody is counted)
  __syncthreads();
  if (tid == 0) last = __hip_atomic_fetch_add(d.counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1u;
  __syncthreads();
  if (!last) return;
  if (tid < d.Fs && ((d.mask >> tid) & 1u)) d.level[tid] = decay_next_level(d.level[tid], decay_log_step(lr, d.lambda));
  if (tid == 0) *d.counter = 0u;
}

// the table pass of the flush (untouched_rows_pass hands over every row of the tables that own tiles: the bitmap is all zero and only
// read).  A row whose stamp is the current level owes nothing; every stamp goes back to 0.
struct DecayFlushRows {
  const nasrec_decoupled_decay_desc_t& d;
  float stamp[TABLE_PASS_UNROLL];
  double owed[TABLE_PASS_UNROLL];
  bool pay[TABLE_PASS_UNROLL];
  f32x4 w[TABLE_PASS_UNROLL];
  __device__ __forceinline__ void load(int u, int f, long off) {
    const double level = d.level[f];
    stamp[u] = d.stamp[f][off >> 4];
    pay[u] = __float_as_uint(stamp[u]) != __float_as_uint((float)level);
    owed[u] = level - (double)stamp[u];
    if (pay[u]) w[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(d.table[f] + off));
  }
  __device__ __forceinline__ void update(int u, int f, long off) {
    if (pay[u]) {
      decay_scale(w[u], exp(owed[u]));
      __builtin_nontemporal_store(w[u], reinterpret_cast<f32x4*>(d.table[f] + off));
    }
    if ((off & 15) == 0 && __float_as_uint(stamp[u]) != 0u) d.stamp[f][off >> 4] = 0.f;
  }
};

// phase 2: every workgroup reads the levels while it walks its tiles; the one that arrives last sets them to 0
__global__ __launch_bounds__(256) void decoupled_decay_flush_kernel(const nasrec_decoupled_decay_desc_t d) {
  __shared__ int last;
  const int tid = threadIdx.x;
  DecayFlushRows r{d};
  untouched_rows_pass(d.tile_off, d.rows, d.Fs, d.bitmap, blockIdx.x, d.nblocks, r);
  __syncthreads();
  if (tid == 0) last = __hip_atomic_fetch_add(d.counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1u;
  __syncthreads();
  if (!last) return;
  if (tid < d.Fs && ((d.mask >> tid) & 1u)) d.level[tid] = 0.0;
  if (tid == 0) *d.counter = 0u;
}

}  // namespace

// Every refusal comes before anything is launched.
int launch_decoupled_decay(hipStream_t st, const nasrec_decoupled_decay_desc_t* d) {
  if (d->Fs < 0 || d->Fs > NASREC_MAX_TABLES) return nasrec_set_error(-1, "decoupled_decay: Fs = %d", d->Fs);
  if (d->phase < 0 || d->phase > 2) return nasrec_set_error(-1, "decoupled_decay: phase %d", d->phase);
  if (!(d->lambda >= 0.0)) return nasrec_set_error(-1, "decoupled_decay: lambda %g is negative", d->lambda);
  if (!(d->lr_max >= 0.0) || !(d->lr_max * d->lambda < 1.0))
    return nasrec_set_error(-1, "decoupled_decay: lr %g x lambda %g is not below 1", d->lr_max, d->lambda);
  if (d->B < 0 || d->n_chunks < 0 || d->dense_blocks < 0) return nasrec_set_error(-1, "decoupled_decay: B %d, n_chunks %d, dense_blocks %d", d->B, d->n_chunks, d->dense_blocks);
  if (d->Fs < 32 && (d->mask >> d->Fs) != 0u) return nasrec_set_error(-1, "decoupled_decay: mask %#x names a table past Fs = %d", d->mask, d->Fs);
  if (d->mask != 0u && !d->level) return nasrec_set_error(-1, "decoupled_decay: levels missing");
  for (int f = 0; f < d->Fs; ++f)
    if (((d->mask >> f) & 1u) && (!d->stamp[f] || !d->table[f] || d->rows[f] < 0))
      return nasrec_set_error(-1, "decoupled_decay: table %d without its weights or stamps", f);
  const long row_threads = d->mask != 0u ? (long)d->B * d->Fs * 4 : 0;
  const int nrows = (int)((row_threads + 255) / 256);
  if (d->phase == 0) {
    if (nrows == 0) return 0;
    if (!d->idx) return nasrec_set_error(-1, "decoupled_decay: ids missing");
    hipLaunchKernelGGL(decoupled_decay_catch_up_kernel, dim3((unsigned)nrows), dim3(256), 0, st, *d);
  } else if (d->phase == 1) {
    if (d->n_chunks > 0 && (!d->p || !d->chunks || d->dense_blocks < 1)) return nasrec_set_error(-1, "decoupled_decay: dense ranges without the arena, the chunk table or a workgroup");
    if (nrows > 0 && (!d->idx || !d->leader || !d->counter)) return nasrec_set_error(-1, "decoupled_decay: ids, leaders or counter missing");
    const int dense = d->n_chunks > 0 ? d->dense_blocks : 0;
    if (dense + nrows == 0) return 0;
    if (!d->lr) return nasrec_set_error(-1, "decoupled_decay: lr missing");
    nasrec_decoupled_decay_desc_t k = *d;
    k.dense_blocks = dense;
    if (nrows == 0) k.B = 0;
    hipLaunchKernelGGL(decoupled_decay_step_kernel, dim3((unsigned)(dense + nrows)), dim3(256), 0, st, k);
  } else {
    if (d->mask == 0u || d->tile_off[d->Fs] <= 0) return 0;
    if (d->nblocks <= 0 || !d->bitmap || !d->counter) return nasrec_set_error(-1, "decoupled_decay: the table pass needs nblocks > 0, the (all-zero) bitmap and the counter");
    hipLaunchKernelGGL(decoupled_decay_flush_kernel, dim3((unsigned)d->nblocks), dim3(256), 0, st, *d);
  }
  return nasrec_check_launch("decoupled_decay");
}
