// L2 weight decay of the fused training step (NASREC_OP_WEIGHT_DECAY, include/nasrec_hip.h): the gradient 2 wd W of get_l2_loss
// (train_utils.py:91-115) on the dense arena and on EVERY table row.  Phase 0 adds it where the backward left gradients and collects
// what the clip norm gains; phase 1, behind the Adagrad of the touched rows, streams the untouched rows of the tables (W and its state,
// read and written once: the bandwidth-bound part of a step with weight decay).
#include "optimizer_bodies.h"

namespace {

constexpr int kTile = TABLE_PASS_TILE;     // rows per tile: 256 threads x one float4 = 64 rows of 16 floats
constexpr int kUnroll = TABLE_PASS_UNROLL; // tiles per workgroup and trip (four independent 16-byte loads in flight per thread)

// table of tile t (tile_off ascending; tables outside reg_mask own no tile)
__device__ __forceinline__ int tile_table(const nasrec_weight_decay_desc_t& d, long t) { return table_of_tile(d.tile_off, d.Fs, t); }

// fixed-order tree over the workgroup: every thread's pair (a, b) -> thread 0
__device__ __forceinline__ void block_sum2(double& a, double& b, double* red) {
  const int tid = threadIdx.x;
  red[tid] = a;
  red[256 + tid] = b;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      red[tid] += red[tid + o];
      red[256 + tid] += red[256 + tid + o];
    }
    __syncthreads();
  }
  a = red[0];
  b = red[256];
}

__global__ __launch_bounds__(256) void weight_decay_phase0_kernel(const nasrec_weight_decay_desc_t d) {
  __shared__ double red[512];
  __shared__ int last;
  const int tid = threadIdx.x, blk = blockIdx.x, nblk = d.nblocks;
  const float two_r = 2.f * d.wd;
  double ex = 0.0, s = 0.0;  // gain of the norm's sum of squares, sum of W^2
  // dense parameters the backward reached: g += 2 wd p
  for (long c = blk; c < d.n_add; c += nblk) {
    const long off = d.add_chunks[2 * c], n = d.add_chunks[2 * c + 1];
    for (long i = tid; i < n; i += 256) {
      const float w = d.p[off + i], g0 = d.g[off + i];
      const float g1 = g0 + two_r * w;
      d.g[off + i] = g1;
      ex += (double)g1 * g1 - (double)g0 * g0;
      s += (double)w * w;
    }
  }
  // regularised parameters it did not reach: the L2 term is their whole gradient
  for (long c = blk; c < d.n_set; c += nblk) {
    const long off = d.set_chunks[2 * c], n = d.set_chunks[2 * c + 1];
    for (long i = tid; i < n; i += 256) {
      const float w = d.p[off + i];
      const float g1 = two_r * w;
      d.g[off + i] = g1;
      ex += (double)g1 * g1;
      s += (double)w * w;
    }
  }
  // touched rows: the leader's summed row += 2 wd W (the reduce launch squared the row without it; the table pass below counts (2 wd W)^2)
  const long lanes = (long)d.B * d.Fs * 4;
  for (long t = (long)blk * 256 + tid; t < lanes; t += (long)nblk * 256) {
    const long pair = t >> 2;
    const int q = (int)(t & 3);
    const int f = (int)(pair % d.Fs);
    if (!((d.reg_mask >> f) & 1u) || !d.leader[pair]) continue;
    const long row = d.idx[pair];
    if (row < 0 || row >= d.rows[f]) continue;  // (flagged by the gather; never read outside a table)
    const f32x4 w = *reinterpret_cast<const f32x4*>(d.table[f] + row * 16 + q * 4);
    f32x4* gp = reinterpret_cast<f32x4*>(d.gsum + gsum_row_offset(pair, d.Fs, d.rank_B, d.rank_stride) + q * 4);  // (read and written in place)
    const f32x4 g0 = *gp;
    f32x4 g1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      g1[e] = g0[e] + two_r * w[e];
      ex += (double)g1[e] * g1[e] - (double)g0[e] * g0[e] - 4.0 * (double)d.wd * (double)d.wd * ((double)w[e] * w[e]);
    }
    *gp = g1;
    if (q == 0) atomicOr(d.bitmap + 2 * d.tile_off[f] + (row >> 5), 1u << (row & 31));
  }
  // every row of every regularised table: W^2, and (2 wd W)^2 as 4 wd^2 sum W^2 (fp32 sums over a trip's 16 elements, fp64 across trips:
  // no fp64 dependency chain per element in the pass that streams the tables)
  const long ntiles = d.tile_off[d.Fs];
  const int sub = tid >> 2, q = tid & 3;
  double s_tab = 0.0;
  for (long t0 = blk; t0 < ntiles; t0 += (long)nblk * kUnroll) {
    f32x4 w[kUnroll];
    bool ok[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const long t = t0 + (long)u * nblk;
      ok[u] = false;
      if (t < ntiles) {
        const int f = tile_table(d, t);
        const long row = (t - d.tile_off[f]) * kTile + sub;
        if (row < d.rows[f]) {
          ok[u] = true;
          w[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(d.table[f] + row * 16 + q * 4));
        }
      }
    }
    float trip = 0.f;
#pragma unroll
    for (int u = 0; u < kUnroll; ++u)
      if (ok[u]) trip += (w[u][0] * w[u][0] + w[u][1] * w[u][1]) + (w[u][2] * w[u][2] + w[u][3] * w[u][3]);
    s_tab += (double)trip;
  }
  ex += 4.0 * (double)d.wd * (double)d.wd * s_tab;
  s += s_tab;
  block_sum2(ex, s, red);
  if (tid == 0) {
    d.block_part[2 * blk] = ex;
    d.block_part[2 * blk + 1] = s;
    __threadfence();
    last = atomicAdd(d.counter, 1u) == (unsigned)(nblk - 1);
  }
  __syncthreads();
  if (!last) return;
  // the last workgroup: every partial in workgroup order (the same sum whichever workgroup this is)
  __threadfence();
  double a = 0.0, b = 0.0;
  for (int i = tid; i < nblk; i += 256) {
    a += __hip_atomic_load(d.block_part + 2 * i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    b += __hip_atomic_load(d.block_part + 2 * i + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  block_sum2(a, b, red);
  if (tid == 0) {
    d.clip_partial[0] = (float)a;
    d.l2_sumsq[0] = b;
    *d.counter = 0u;
  }
}

// phase 1's row update: Adagrad with g = 2 wd W * coef (untouched_rows_pass, optimizer_bodies.h)
struct AdagradDecayRows {
  const nasrec_weight_decay_desc_t& d;
  const float lr, coef, two_r, eps;
  f32x4 w[TABLE_PASS_UNROLL], st[TABLE_PASS_UNROLL];
  __device__ __forceinline__ void load(int u, int f, long off) {
    w[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(d.table[f] + off));
    st[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(d.state[f] + off));
  }
  __device__ __forceinline__ void update(int u, int f, long off) {
    f32x4 p = w[u], s = st[u];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float g = (two_r * p[e]) * coef;
      s[e] = fmaf(g, g, s[e]);
      p[e] = p[e] - lr * (g / (sqrtf(s[e]) + eps));
    }
    __builtin_nontemporal_store(s, reinterpret_cast<f32x4*>(d.state[f] + off));
    __builtin_nontemporal_store(p, reinterpret_cast<f32x4*>(d.table[f] + off));
  }
};

__global__ __launch_bounds__(256) void weight_decay_phase1_kernel(const nasrec_weight_decay_desc_t d) {
  const int tid = threadIdx.x, blk = blockIdx.x, nblk = d.nblocks;
  // the set chunks' gradient (phase 0's g = 2 wd W, read by the apply launch) goes back to zero: the backward never writes those ranges,
  // and a later plan of the same engine that walks the whole arena must find them as they were
  for (long c = blk; c < d.n_set; c += nblk) {
    const long off = d.set_chunks[2 * c], n = d.set_chunks[2 * c + 1];
    for (long i = tid; i < n; i += 256) d.g[off + i] = 0.f;
  }
  AdagradDecayRows r{d, *d.lr, *d.coef, 2.f * d.wd, d.eps};
  untouched_rows_pass(d.tile_off, d.rows, d.Fs, d.bitmap, blk, nblk, r);
}

}  // namespace

int launch_weight_decay(hipStream_t st, const nasrec_weight_decay_desc_t* d) {
  if (d->nblocks <= 0) return nasrec_set_error(-1, "weight_decay: nblocks must be positive");
  if (d->Fs < 0 || d->Fs > NASREC_MAX_TABLES) return nasrec_set_error(-1, "weight_decay: Fs = %d", d->Fs);
  if (d->phase == 0) {
    if (!d->block_part || !d->counter || !d->clip_partial || !d->l2_sumsq) return nasrec_set_error(-1, "weight_decay: phase 0 outputs missing");
    if (d->rank_B < 0 || (d->rank_B > 0 && (d->rank_stride < (int64_t)d->rank_B * d->Fs * 16 || d->B % d->rank_B != 0)))
      return nasrec_set_error(-2, "weight_decay: rank layout %d / %ld", d->rank_B, (long)d->rank_stride);
    hipLaunchKernelGGL(weight_decay_phase0_kernel, dim3((unsigned)d->nblocks), dim3(256), 0, st, *d);
  } else if (d->phase == 1) {
    if ((d->Fs == 0 || d->tile_off[d->Fs] == 0) && d->n_set == 0) return 0;
    if (!d->lr || !d->coef || !d->bitmap) return nasrec_set_error(-1, "weight_decay: phase 1 inputs missing");
    hipLaunchKernelGGL(weight_decay_phase1_kernel, dim3((unsigned)d->nblocks), dim3(256), 0, st, *d);
  } else {
    return nasrec_set_error(-1, "weight_decay: phase %d", d->phase);
  }
  return nasrec_check_launch("weight_decay");
}
