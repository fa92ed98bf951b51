// The optimizer tail of a last-layer fine-tune step (NASREC_OP_LAST_LAYER_STEP, include/nasrec_hip.h): the searcher scores a candidate
// by training _final.{weight [1, K], bias [1]} alone (SuperNet.set_mode_to_finelune_last_only).  The torch route for that is a gradient
// clone, clip_grad_norm_ over every parameter of the model and the torch optimizer — a dozen launches for K + 1 numbers.  Here it is one
// workgroup behind the final-logit backward: gradient (summing the split backward's partials), weight decay, clip, optimizer.
// Latency-bound: four waves, every value held in LDS between the phases; fixed orders throughout, so equal inputs give equal bits.
#include "optimizer_bodies.h"

namespace {

constexpr int LL_THREADS = 256;

template <int ALGO>
__global__ __launch_bounds__(LL_THREADS) void last_layer_step_kernel(const nasrec_last_layer_step_desc_t d) {
  __shared__ float g_sh[NASREC_LAST_LAYER_MAX];
  __shared__ double red[LL_THREADS];
  __shared__ float sh_coef;
  const int tid = threadIdx.x, K = d.K, n = K + 1;
  const float lr = *d.lr, two_r = 2.f * d.wd;
  // (a) + (b): the gradient of every element, and this thread's share of ||g||^2 (elements tid, tid + 256, ..)
  double s = 0.0;
  for (int j = tid; j < n; j += LL_THREADS) {
    float g;
    if (d.nsplit > 1) {
      g = d.partial[j];
      for (int r = 1; r < d.nsplit; ++r) g += d.partial[(long)r * n + j];
      if (j < K) d.dw[j] = g;
      else d.dbias[0] = g;
    } else {
      g = j < K ? d.dw[j] : d.dbias[0];
    }
    if (d.decay_w && j < K) g = g + two_r * d.w[j];
    g_sh[j] = g;
    s += (double)g * g;
  }
  // (c) fixed-order tree over the 256 partial sums -> clip coefficient
  red[tid] = s;
  __syncthreads();
  for (int o = LL_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    const float total = (float)sqrt(red[0]);
    float coef = 1.f;
    if (d.max_norm > 0.f) coef = fminf(d.max_norm / (total + 1e-6f), 1.f);
    sh_coef = coef;
    if (d.norm_out) {
      d.norm_out[0] = coef;
      d.norm_out[1] = total;
    }
  }
  float ss_w = 0.f, bs_w = 1.f, ss_b = 0.f, bs_b = 1.f;
  if (ALGO == NASREC_OPTIM_ADAM) {  // (read before the barrier below: thread 0 moves the counters after the second one)
    adam_scalars(d, d.step[0], lr, ss_w, bs_w);
    adam_scalars(d, d.step[1], lr, ss_b, bs_b);
  }
  __syncthreads();
  const float coef = sh_coef;
  // (d) the optimizer, element by element
  for (int j = tid; j < n; j += LL_THREADS) {
    const float g = g_sh[j] * coef;
    if (d.g_out) d.g_out[j] = g;
    const bool wt = j < K;
    float& p = wt ? d.w[j] : d.bias[0];
    float& m = wt ? d.s_w[j] : d.s_b[0];
    if (ALGO == NASREC_OPTIM_ADAGRAD) {
      float sv = m, pv = p;
      adagrad_elem(g, sv, pv, lr, d.eps);
      m = sv;
      p = pv;
    } else {
      float pv = p, mv = m, vv = 0.f;
      if (ALGO == NASREC_OPTIM_ADAM) vv = wt ? d.v_w[j] : d.v_b[0];
      moments_elem<ALGO>(d, g, pv, mv, vv, lr, wt ? ss_w : ss_b, wt ? bs_w : bs_b);
      p = pv;
      m = mv;
      if (ALGO == NASREC_OPTIM_ADAM) (wt ? d.v_w[j] : d.v_b[0]) = vv;
    }
  }
  if (ALGO != NASREC_OPTIM_ADAGRAD) {
    __syncthreads();  // every thread has read the counters
    if (tid == 0) {
      d.step[0] += 1.f;
      d.step[1] += 1.f;
    }
  }
}

}  // namespace

int launch_last_layer_step(hipStream_t st, const nasrec_last_layer_step_desc_t* d) {
  if (d->K < 1 || d->K + 1 > NASREC_LAST_LAYER_MAX)
    return nasrec_set_error(-1, "last_layer_step: K = %d (1 .. %d)", d->K, NASREC_LAST_LAYER_MAX - 1);
  if (d->nsplit > 32) return nasrec_set_error(-1, "last_layer_step: nsplit = %d (at most 32)", d->nsplit);
  if (!d->lr || !d->w || !d->bias || !d->s_w || !d->s_b || !d->dw || !d->dbias || (d->nsplit > 1 && !d->partial))
    return nasrec_set_error(-1, "last_layer_step: missing pointer");
  if (d->algo != NASREC_OPTIM_ADAGRAD && !d->step) return nasrec_set_error(-1, "last_layer_step: step counters missing");
  if (d->algo == NASREC_OPTIM_ADAM && (!d->v_w || !d->v_b)) return nasrec_set_error(-1, "last_layer_step: exp_avg_sq missing");
  switch (d->algo) {
    case NASREC_OPTIM_ADAGRAD: hipLaunchKernelGGL(last_layer_step_kernel<NASREC_OPTIM_ADAGRAD>, dim3(1), dim3(LL_THREADS), 0, st, *d); break;
    case NASREC_OPTIM_ADAM: hipLaunchKernelGGL(last_layer_step_kernel<NASREC_OPTIM_ADAM>, dim3(1), dim3(LL_THREADS), 0, st, *d); break;
    case NASREC_OPTIM_SGD: hipLaunchKernelGGL(last_layer_step_kernel<NASREC_OPTIM_SGD>, dim3(1), dim3(LL_THREADS), 0, st, *d); break;
    default: return nasrec_set_error(-1, "last_layer_step: algo %d", d->algo);
  }
  return nasrec_check_launch("last_layer_step");
}
