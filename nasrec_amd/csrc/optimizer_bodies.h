// Device bodies of the optimizer tail (clip_grad_norm_ + Adagrad, train_utils.py:285-286 / main_train.py:152-154), shared
// by the stand-alone kernels and by the two fused launches NASREC_OP_OPT_REDUCE / NASREC_OP_OPT_APPLY.
#pragma once
#include "common.h"

// row of (sample, field) pair `pair` in per-sample row gradients: one contiguous [B,Fs,16] array (rank_B = 0), or the receive buffer
// of an all-gather whose per-rank chunks of rank_B samples lie rank_stride floats apart (dd_row, dedup_bodies.h: the same mapping)
__device__ __forceinline__ long gsum_row_offset(long pair, int Fs, int rank_B, long rank_stride) {
  if (rank_B > 0) {
    const long b = pair / Fs, f = pair - b * Fs, r = b / rank_B;
    return r * rank_stride + ((b - r * rank_B) * Fs + f) * 16;
  }
  return pair * 16;
}

// sum of squares of x[0, n) (or of the chunk table's ranges): workgroup `blk` of `nblk` (256 threads), fixed-order tree -> partial[blk]
__device__ __forceinline__ void sumsq_body(const nasrec_sumsq_desc_t& d, int blk, int nblk, float* red) {
  const int tid = threadIdx.x;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;  // four independent chains keep several cold loads in flight
  if (d.chunks) {
    for (long c = blk; c < d.nchunks; c += nblk) {
      const float* x = d.x + d.chunks[2 * c];
      const long n = d.chunks[2 * c + 1], n4 = n >> 2;
      long i = tid;
      for (; i + 768 < n4; i += 1024) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(x + 4 * i), b = *reinterpret_cast<const f32x4*>(x + 4 * (i + 256));
        const f32x4 c2 = *reinterpret_cast<const f32x4*>(x + 4 * (i + 512)), e = *reinterpret_cast<const f32x4*>(x + 4 * (i + 768));
        s0 += (a[0] * a[0] + a[1] * a[1]) + (a[2] * a[2] + a[3] * a[3]);
        s1 += (b[0] * b[0] + b[1] * b[1]) + (b[2] * b[2] + b[3] * b[3]);
        s2 += (c2[0] * c2[0] + c2[1] * c2[1]) + (c2[2] * c2[2] + c2[3] * c2[3]);
        s3 += (e[0] * e[0] + e[1] * e[1]) + (e[2] * e[2] + e[3] * e[3]);
      }
      for (; i < n4; i += 256) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(x + 4 * i);
        s0 += (a[0] * a[0] + a[1] * a[1]) + (a[2] * a[2] + a[3] * a[3]);
      }
      for (long j = 4 * n4 + tid; j < n; j += 256) s1 = fmaf(x[j], x[j], s1);
    }
  } else {
    // 16-byte loads, four in flight per thread and trip (the arena is 16-byte aligned): with one float per load a thread of the
    // batch-256 step (2.2 M gradients over 256 workgroups) made nine dependent trips to memory, now two
    const long stride = (long)nblk * 256, n4 = d.n >> 2;
    long i = (long)blk * 256 + tid;
    for (; i + 3 * stride < n4; i += 4 * stride) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(d.x + 4 * i), b = *reinterpret_cast<const f32x4*>(d.x + 4 * (i + stride));
      const f32x4 c = *reinterpret_cast<const f32x4*>(d.x + 4 * (i + 2 * stride)), e = *reinterpret_cast<const f32x4*>(d.x + 4 * (i + 3 * stride));
      s0 += (a[0] * a[0] + a[1] * a[1]) + (a[2] * a[2] + a[3] * a[3]);
      s1 += (b[0] * b[0] + b[1] * b[1]) + (b[2] * b[2] + b[3] * b[3]);
      s2 += (c[0] * c[0] + c[1] * c[1]) + (c[2] * c[2] + c[3] * c[3]);
      s3 += (e[0] * e[0] + e[1] * e[1]) + (e[2] * e[2] + e[3] * e[3]);
    }
    {  // up to three more pieces per thread, loaded together
      f32x4 r[3];
#pragma unroll
      for (int u = 0; u < 3; ++u) r[u] = *reinterpret_cast<const f32x4*>(d.x + 4 * (i + u * stride < n4 ? i + u * stride : 0));
#pragma unroll
      for (int u = 0; u < 3; ++u)
        if (i + u * stride < n4) s0 += (r[u][0] * r[u][0] + r[u][1] * r[u][1]) + (r[u][2] * r[u][2] + r[u][3] * r[u][3]);
    }
    for (long j = 4 * n4 + (long)blk * 256 + tid; j < d.n; j += stride) s1 = fmaf(d.x[j], d.x[j], s1);
  }
  red[tid] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) d.partial[blk] = red[0];
}

// one wavefront: lanes take the partials round-robin (fixed assignment), fp64 butterfly -> the same value in every lane
__device__ __forceinline__ float clip_coef_wave(const nasrec_clip_coef_desc_t& d, int lane, float* total_out) {
  // eight partials per lane and trip in flight, the first trip of list b beside list a's (a plain loop is load -> wait -> add per
  // partial: 256 + 26 partials were five dependent round trips at the head of EVERY workgroup of the apply launch).  The additions
  // per lane are in the same order as before — all of a, then all of b: same bits.
  double s = 0.0;
  const int na = d.n_a, nb = d.n_b;
  if (na > 0 || nb > 0) {
    const float* pa = na > 0 ? d.partial_a : d.partial_b;  // (an empty list is read at the other list's first element and dropped)
    const float* pb = nb > 0 ? d.partial_b : d.partial_a;
    const int ca = max(na - 1, 0), cb = max(nb - 1, 0);
    float vb0[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) vb0[u] = pb[min(lane + 64 * u, cb)];
    for (int i0 = lane; i0 < na; i0 += 64 * 8) {
      float va[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) va[u] = pa[min(i0 + 64 * u, ca)];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (i0 + 64 * u < na) s += (double)va[u];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (lane + 64 * u < nb) s += (double)vb0[u];
    for (int i0 = lane + 64 * 8; i0 < nb; i0 += 64 * 8) {
      float vb[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) vb[u] = pb[min(i0 + 64 * u, cb)];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (i0 + 64 * u < nb) s += (double)vb[u];
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  const float total = (float)sqrt(s);
  float coef = 1.f;
  if (d.max_norm > 0.f) coef = fminf(d.max_norm / (total + 1e-6f), 1.f);
  *total_out = total;
  return coef;
}

// head of the apply launch and of Adam / SGD / RMSprop's phase 0: wavefront 0 of every workgroup computes the clip coefficient into
// *sh_coef (workgroup 0 writes clip.out); the caller synchronises
__device__ __forceinline__ void clip_head(const nasrec_clip_coef_desc_t& clip, float* sh_coef) {
  const int tid = threadIdx.x;
  if (tid < 64) {
    float total;
    const float c = clip_coef_wave(clip, tid, &total);
    if (tid == 0) {
      *sh_coef = c;
      if (blockIdx.x == 0) {
        clip.out[0] = c;
        clip.out[1] = total;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// One element of each optimizer, g = the clipped gradient: Adagrad (the apply launch, NASREC_OP_OPT_APPLY) and Adam / momentum SGD
// (NASREC_OP_OPT_MOMENTS); NASREC_OP_LAST_LAYER_STEP calls the same functions.  D = a descriptor with beta1, beta2, eps, momentum,
// nesterov.
// ---------------------------------------------------------------------------------------------------
// Adagrad's weight statement with the accumulator `s` already current (shared with row-wise Adagrad, whose s is one number per row)
__device__ __forceinline__ void adagrad_weight(float g, float s, float& p, float lr, float eps) { p = p - lr * (g / (sqrtf(s) + eps)); }
__device__ __forceinline__ void adagrad_elem(float g, float& s, float& p, float lr, float eps) {
  s = fmaf(g, g, s);
  adagrad_weight(g, s, p, lr, eps);
}

// Adam's per-parameter scalars of this step, from the step counter as torch computes them in Python doubles (torch/optim/adam.py,
// _multi_tensor_adam): step_size = lr / (1 - b1^t), bc2_sqrt = sqrt(1 - b2^t), t = step + 1
template <class D>
__device__ __forceinline__ void adam_scalars(const D& d, float step, float lr, float& step_size, float& bc2_sqrt) {
  const double t = (double)step + 1.0;
  step_size = (float)((double)lr / (1.0 - pow(d.beta1, t)));
  bc2_sqrt = (float)sqrt(1.0 - pow(d.beta2, t));
}

// one element; g = the clipped gradient.  The statements follow torch's foreach calls one by one (lerp_; mul_ + addcmul_; sqrt, div_,
// add_; addcdiv_): -ffp-contract=on fuses within a statement only.  RMSprop (momentum 0, not centered; alpha travels in beta2): mul_,
// addcmul_; sqrt, add_; addcdiv_ — m is unused.
template <int ALGO, class D>
__device__ __forceinline__ void moments_elem(const D& d, float g, float& p, float& m, float& v, float lr,
                                             float step_size, float bc2_sqrt) {
  if (ALGO == NASREC_OPTIM_ADAM) {
    const float w1 = (float)(1.0 - d.beta1), b2 = (float)d.beta2, w2 = (float)(1.0 - d.beta2);
    m = w1 < 0.5f ? m + w1 * (g - m) : g - (g - m) * (1.f - w1);  // (torch's lerp)
    v = v * b2;
    v = v + w2 * (g * g);
    float den = sqrtf(v) / bc2_sqrt;
    den = den + d.eps;
    p = p + (-step_size) * (m / den);
  } else if (ALGO == NASREC_OPTIM_RMSPROP) {
    const float a = (float)d.beta2, w = (float)(1.0 - d.beta2);
    v = v * a;
    v = v + w * (g * g);
    float den = sqrtf(v);
    den = den + d.eps;
    p = p + (-lr) * (g / den);
  } else {
    m = m * d.momentum;
    m = m + g;
    float dir = m;
    if (d.nesterov) dir = g + d.momentum * m;
    p = p + (-lr) * dir;
  }
}

// Row-sparse Adam on a touched table row (torch.optim.SparseAdam, torch/optim/_functional.py sparse_adam): the step size carries both
// bias corrections, in Python doubles: lr sqrt(1 - b2^t) / (1 - b1^t), t = step + 1; eps is added to sqrt(v) itself
template <class D>
__device__ __forceinline__ float sparse_adam_step_size(const D& d, float step, float lr) {
  const double t = (double)step + 1.0;
  return (float)((double)lr * sqrt(1.0 - pow(d.beta2, t)) / (1.0 - pow(d.beta1, t)));
}

// g = the clipped summed gradient.  One statement per torch call, as in moments_elem, in the three groups a row-wise second moment
// takes apart: the first moment (sub, mul_, add_); the second moment from its g^2 term — g * g, or the row's mean of it — and the
// denominator it gives (pow, sub_, mul_, add_; sqrt_, add_); the weight statement (div_, mul, add_)
__device__ __forceinline__ void sparse_adam_first_moment(float w1, float g, float& m) {  // (w1 = 1 - beta1)
  float mu = g - m;
  mu = mu * w1;
  m = m + mu;
}
__device__ __forceinline__ float sparse_adam_second_moment(float w2, float eps, float g2, float& v) {  // (w2 = 1 - beta2) -> the denominator
  float vu = g2 - v;
  vu = vu * w2;
  v = v + vu;
  return sqrtf(v) + eps;
}
__device__ __forceinline__ void sparse_adam_weight(float m, float den, float& p, float step_size) {
  float u = m / den;
  u = (-step_size) * u;
  p = p + u;
}
template <class D>
__device__ __forceinline__ void sparse_adam_elem(const D& d, float g, float& p, float& m, float& v, float step_size) {
  const float w1 = (float)(1.0 - d.beta1), w2 = (float)(1.0 - d.beta2);
  sparse_adam_first_moment(w1, g, m);
  const float den = sparse_adam_second_moment(w2, d.eps, g * g, v);
  sparse_adam_weight(m, den, p, step_size);
}

// The sum of the squares of a row's 16 gradient elements, in each of its four lanes (g4 = the lane's quarter); the callers scale it to
// the mean (* 0.0625f: exact) in a statement of their own.  The sum over the four lanes goes into each of them (a + b is commutative:
// the four totals have the same bits).  The quad is the aligned lanes 4k .. 4k + 3 of one wavefront, and its lanes arrive here
// together or not at all: every branch in front of a call (pair < B * Fs, leader[pair], the row-range test) is a function of
// `pair` = t >> 2 alone.  quad_perm reads inside the quad only, so the other quads of the wavefront may be inactive.  A branch on q in
// front of a call would break it.
__device__ __forceinline__ float row_sum_of_squares(const f32x4& g4) {
  float sq = g4[0] * g4[0];
  sq = fmaf(g4[1], g4[1], sq);
  sq = fmaf(g4[2], g4[2], sq);
  sq = fmaf(g4[3], g4[3], sq);
  sq += dpp_mov<0xb1>(sq);  // quad_perm:[1,0,3,2]
  sq += dpp_mov<0x4e>(sq);  // quad_perm:[2,3,0,1]
  return sq;
}

// RMSprop's lazily decayed table rows: a row whose gradient was zero for n steps owes its square_avg the factor alpha^n; power and
// product in fp64, rounded once (n = 0: v as it is, so a row touched every step has the bits of the dense statements)
__device__ __forceinline__ float lazy_decay(float v, double alpha, long n) {
  return n > 0 ? (float)((double)v * pow(alpha, (double)n)) : v;
}

__device__ __forceinline__ void adagrad_dense_body(const nasrec_adagrad_dense_desc_t& d, int blk, int nblk, float lr, float coef) {
  if (d.chunks) {
    for (long c = blk; c < d.nchunks; c += nblk) {
      const long off = d.chunks[2 * c], n = d.chunks[2 * c + 1], n4 = n >> 2;
      const float* gp = d.g + off;
      float* sp = d.state + off;
      float* pp = d.p + off;
      for (long i = threadIdx.x; i < n4; i += 256) {
        const f32x4 g4 = *reinterpret_cast<const f32x4*>(gp + 4 * i);
        f32x4 s4 = *reinterpret_cast<const f32x4*>(sp + 4 * i), p4 = *reinterpret_cast<const f32x4*>(pp + 4 * i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float se = s4[e], pe = p4[e];
          adagrad_elem(g4[e] * coef, se, pe, lr, d.eps);
          s4[e] = se;
          p4[e] = pe;
        }
        *reinterpret_cast<f32x4*>(sp + 4 * i) = s4;
        *reinterpret_cast<f32x4*>(pp + 4 * i) = p4;
      }
      for (long j = 4 * n4 + threadIdx.x; j < n; j += 256) {
        float s = sp[j], p = pp[j];
        adagrad_elem(gp[j] * coef, s, p, lr, d.eps);
        sp[j] = s;
        pp[j] = p;
      }
    }
    return;
  }
  for (long i = (long)blk * 256 + threadIdx.x; i < d.n; i += (long)nblk * 256) {
    float s = d.state[i], p = d.p[i];
    adagrad_elem(d.g[i] * coef, s, p, lr, d.eps);
    d.state[i] = s;
    d.p[i] = p;
  }
}

// Row-sparse clip + Adagrad on the touched rows only (4 lanes x float4 per row); workgroup `blk` of 256 threads
__device__ __forceinline__ void adagrad_rows_body(const nasrec_adagrad_rows_desc_t& d, int blk, float lr, float coef) {
  const long t = (long)blk * 256 + threadIdx.x;
  const long pair = t >> 2;
  const int q = (int)(t & 3);
  if (pair >= (long)d.B * d.Fs) return;
  // Two memory round trips instead of five: everything that does not depend on the row id — leader flag, id, the field's row count and
  // its two base pointers (per-lane loads from the argument arrays: f differs inside a wavefront), the gradient piece — is issued
  // together; written as `if (!leader) return; row = idx; if (row >= rows[f]) return; ...` every test was a load, a wait and a branch.
  const int f = (int)(pair % d.Fs);
  const int lead = d.leader[pair];
  const long row = d.idx[pair];
  const long nrows = d.rows[f];
  float* const sbase = d.state[f];
  float* const tbase = d.table[f];
  const float* grow = d.gsum + pair * 16;
  if (d.rank_B > 0) {  // gsum = the receive buffer of an all-gather whose per-rank chunks are rank_stride floats apart
    const long b = pair / d.Fs, r = b / d.rank_B;
    grow = d.gsum + r * d.rank_stride + ((b - r * d.rank_B) * d.Fs + f) * 16;
  }
  float4 g = *reinterpret_cast<const float4*>(grow + q * 4);
  asm volatile("" ::"v"(lead), "v"((int)row), "v"((int)nrows), "v"(sbase), "v"(tbase), "v"(g.x));  // (all six in flight before the first test)
  if (!lead) return;
  if (row < 0 || row >= nrows) return;  // never write outside a table
  float4* sp = reinterpret_cast<float4*>(sbase + row * 16 + q * 4);
  float4* pp = reinterpret_cast<float4*>(tbase + row * 16 + q * 4);
  float4 s = *sp, p = *pp;
  float gg[4] = {g.x * coef, g.y * coef, g.z * coef, g.w * coef};
  float ssv[4] = {s.x, s.y, s.z, s.w};
  float pv[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    ssv[e] = fmaf(gg[e], gg[e], ssv[e]);
    pv[e] = pv[e] - lr * (gg[e] / (sqrtf(ssv[e]) + d.eps));
  }
  *sp = make_float4(ssv[0], ssv[1], ssv[2], ssv[3]);
  *pp = make_float4(pv[0], pv[1], pv[2], pv[3]);
}

static inline int adagrad_dense_blocks(long n) {
  long blocks = (n + 255) / 256;
  return (int)(blocks > 2048 ? 2048 : blocks);
}

// ---------------------------------------------------------------------------------------------------
// The untouched-row pass over the embedding tables (weight decay's phase 1 under Adagrad, csrc/weight_decay.hip; Adam / SGD's
// phase 1, csrc/optim_moments.hip).  Tables are walked in tiles of 64 rows (256 threads x one float4: thread `tid` takes row
// tid / 4, quarter tid % 4), the tiles of the tables that take part numbered consecutively: table f owns tiles
// [tile_off[f], tile_off[f+1]) and the bits [2 tile_off[f], 2 tile_off[f+1]) words of `bitmap` (bit row & 31 of word
// 2 tile_off[f] + row / 32).  Each workgroup takes TABLE_PASS_UNROLL tiles per trip; a row whose bit is NOT set is handed to
// `rows.load(u, f, offset)` (all loads of the trip in flight together), then to `rows.update(u, f, offset)`; the bitmap is left all zero.
// ---------------------------------------------------------------------------------------------------
constexpr int TABLE_PASS_TILE = 64;
constexpr int TABLE_PASS_UNROLL = 4;

// table of tile t (tile_off ascending; a table outside the pass owns no tile)
__device__ __forceinline__ int table_of_tile(const int64_t* tile_off, int Fs, long t) {
  int f = 0;
  while (f + 1 < Fs && tile_off[f + 1] <= t) ++f;
  return f;
}

template <class Rows>
__device__ __forceinline__ void untouched_rows_pass(const int64_t* tile_off, const int64_t* rows, int Fs, uint32_t* bitmap, int blk, int nblk,
                                                    Rows& r) {
  const int tid = threadIdx.x, sub = tid >> 2, q = tid & 3;
  const long ntiles = tile_off[Fs];
  for (long t0 = blk; t0 < ntiles; t0 += (long)nblk * TABLE_PASS_UNROLL) {
    long off[TABLE_PASS_UNROLL];
    int tf[TABLE_PASS_UNROLL];
    uint32_t* word[TABLE_PASS_UNROLL];
    uint32_t bits[TABLE_PASS_UNROLL];
    bool ok[TABLE_PASS_UNROLL];
#pragma unroll
    for (int u = 0; u < TABLE_PASS_UNROLL; ++u) {
      const long t = t0 + (long)u * nblk;
      ok[u] = false;
      word[u] = nullptr;
      bits[u] = 0u;
      if (t < ntiles) {
        const int f = table_of_tile(tile_off, Fs, t);
        const long row = (t - tile_off[f]) * TABLE_PASS_TILE + sub;
        word[u] = bitmap + 2 * t + (sub >> 5);  // (2 words per tile: 2 tile_off[f] + row / 32)
        bits[u] = *word[u];
        if (row < rows[f] && !((bits[u] >> (row & 31)) & 1u)) {
          ok[u] = true;
          tf[u] = f;
          off[u] = row * 16 + q * 4;
          r.load(u, f, off[u]);
        }
      }
    }
    __syncthreads();  // every thread has read its word: the first thread of each word's 32 rows clears it
#pragma unroll
    for (int u = 0; u < TABLE_PASS_UNROLL; ++u)
      if ((tid & 127) == 0 && bits[u] != 0u) *word[u] = 0u;
#pragma unroll
    for (int u = 0; u < TABLE_PASS_UNROLL; ++u)
      if (ok[u]) r.update(u, tf[u], off[u]);
  }
}
