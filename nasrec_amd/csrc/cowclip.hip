// CowClip (NASREC_OP_COWCLIP, include/nasrec_hip.h; utils/optim.CowClip): per-row adaptive gradient clipping of the embedding tables,
// a pre-scaling of the leaders' summed gradient rows between the row dedup and the optimizer.  A row's globally clipped gradient
// norm G = coef ||g|| is held to T = cnt max(r ||w||, zeta), cnt = how often the row's id occurs in the batch: a frequent id may move
// as far as its count allows, a rare one no further than its own weight norm.  Phase 0 counts the ids into a per-table scratch of one
// word per row (all zero between steps), phase 1 scales the rows that exceed their threshold in place and takes the counts back to
// zero.  Its own launches: no optimizer kernel knows of it, so every table rule (ROW_FORMS, csrc/optim_moments.hip) and plain Adagrad
// read the scaled rows as they read any other.
#include "optimizer_bodies.h"

namespace {

// phase 0: one thread per (sample, field) pair; a set of increments, no value depends on their order
__global__ __launch_bounds__(256) void cowclip_count_kernel(const nasrec_cowclip_desc_t d) {
  const long pair = (long)blockIdx.x * 256 + threadIdx.x;
  if (pair >= (long)d.B * d.Fs) return;
  const int f = (int)(pair % d.Fs);
  const long row = d.idx[pair];
  if (row < 0 || row >= d.rows[f]) return;  // (flagged by the gather; never counted outside a table)
  atomicAdd(d.cnt[f] + row, 1u);
}

// phase 1: the thread layout of opt_moments' phase 0 — 4 lanes x float4 per (sample, field) pair, the leader of a row id carries the
// row's summed gradient.  Every branch in front of row_sum_of_squares is a function of `pair` alone (its invariant).  The four lanes
// of a row read its count before lane 0 takes it back to zero: they sit in one wavefront, and the store follows the loads in program
// order; no other pair of the launch reads that word (one leader per row and table).
__global__ __launch_bounds__(256) void cowclip_clip_kernel(const nasrec_cowclip_desc_t d) {
  __shared__ float sh_coef;
  clip_head(d.clip, &sh_coef);
  __syncthreads();
  const float coef = sh_coef;
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  const long pair = t >> 2;
  const int q = (int)(t & 3);
  if (pair >= (long)d.B * d.Fs || !d.leader[pair]) return;
  const int f = (int)(pair % d.Fs);
  const long row = d.idx[pair];
  if (row < 0 || row >= d.rows[f]) return;  // (flagged by the gather; never read outside a table)
  f32x4* const gp = reinterpret_cast<f32x4*>(d.gsum + pair * 16 + q * 4);
  f32x4 g4 = *gp;
  const f32x4 w4 = *reinterpret_cast<const f32x4*>(d.table[f] + row * 16 + q * 4);
  uint32_t* const cp = d.cnt[f] + row;
  const uint32_t cnt = *cp;
  const float sg = row_sum_of_squares(g4);
  const float sw = row_sum_of_squares(w4);
  if (q == 0) *cp = 0u;
  const float G = coef * sqrtf(sg);
  const float T = (float)cnt * fmaxf(d.r * sqrtf(sw), d.zeta);
  const bool clipped = G > T;  // (false for G = 0 and for a NaN: the row keeps its bits)
  if (clipped) {
    const float s = T / G;
#pragma unroll
    for (int e = 0; e < 4; ++e) g4[e] = g4[e] * s;
    *gp = g4;
  }
  if (q == 0 && d.stat) {
    atomicAdd(d.stat, 1u);
    if (clipped) atomicAdd(d.stat + 1, 1u);
  }
}

}  // namespace

// Every refusal comes before anything is launched.
int launch_cowclip(hipStream_t st, const nasrec_cowclip_desc_t* d) {
  if (d->Fs < 0 || d->Fs > NASREC_MAX_TABLES) return nasrec_set_error(-1, "cowclip: Fs = %d", d->Fs);
  if (d->phase < 0 || d->phase > 1) return nasrec_set_error(-1, "cowclip: phase %d", d->phase);
  if (d->B < 0) return nasrec_set_error(-1, "cowclip: B = %d", d->B);
  if (!(d->r >= 0.f)) return nasrec_set_error(-1, "cowclip: r %g is negative", (double)d->r);
  if (!(d->zeta > 0.f)) return nasrec_set_error(-1, "cowclip: zeta %g must be positive", (double)d->zeta);
  const long pairs = (long)d->B * d->Fs;
  if (pairs > 0 && !d->idx) return nasrec_set_error(-1, "cowclip: idx missing");
  for (int f = 0; pairs > 0 && f < d->Fs; ++f)
    if (!d->cnt[f]) return nasrec_set_error(-1, "cowclip: cnt[%d] missing", f);
  if (d->phase == 0) {
    if (pairs == 0) return 0;
    hipLaunchKernelGGL(cowclip_count_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, st, *d);
    return nasrec_check_launch("cowclip");
  }
  if (pairs > 0 && !d->leader) return nasrec_set_error(-1, "cowclip: leader missing");
  if (pairs > 0 && !d->gsum) return nasrec_set_error(-1, "cowclip: gsum missing");
  for (int f = 0; pairs > 0 && f < d->Fs; ++f)
    if (!d->table[f]) return nasrec_set_error(-1, "cowclip: table[%d] missing", f);
  if (d->clip.n_a < 0 || d->clip.n_b < 0 || (d->clip.n_a > 0 && !d->clip.partial_a) || (d->clip.n_b > 0 && !d->clip.partial_b) || !d->clip.out)
    return nasrec_set_error(-1, "cowclip: clip partials / out missing");
  if (pairs == 0) return 0;
  hipLaunchKernelGGL(cowclip_clip_kernel, dim3((unsigned)((pairs * 4 + 255) / 256)), dim3(256), 0, st, *d);
  return nasrec_check_launch("cowclip");
}
