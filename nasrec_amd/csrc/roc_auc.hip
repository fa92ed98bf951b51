// ROC AUC of binary labels and float32 scores (NASREC_OP_ROC_AUC, include/nasrec_hip.h), bit-identical to scikit-learn's
// roc_auc_score on numpy's float64 arithmetic (the contract: DESIGN.md "ROC AUC on the device").  A chain of launches on the caller's stream:
//   keys        score -> order-preserving uint32 key of the DESCENDING order (+0 and -0 one key), input checks, pass-0 histogram
//   4 x radix   stable 8-bit LSD passes over (key, label): per-tile digit histogram, per-digit scan over tiles, stable scatter (ranks
//               inside a wave from 64-bit ballots)
//   groups      per tile (positives, group ends) -> one-workgroup int64 scan -> tps / fps at every group end
//   keep        sklearn's drop_intermediate flags -> one-workgroup int64 scan -> the kept (fps, tps), written over the sorted keys
//   chunks      one workgroup per 8192 terms (numpy's reduction buffer): each thread sums one <= 128-term leaf of numpy's pairwise
//               tree, one thread combines the leaves along the same tree
//   final       the chunk sums in order from 0.0, the status word
// No workgroup waits on another (every hand-off is a launch boundary), every count is an integer and every floating-point operation
// has a fixed order, so equal inputs give equal bits.  The per-point counts are stored as int32 (n <= NASREC_ROC_AUC_MAX_N = 2^30): the
// workspace is 18 bytes per sample.
#include "common.h"

namespace {

constexpr int RT = 256;                    // threads of every workgroup here
constexpr int ITEMS = 16;                  // elements per thread of a tile
constexpr int TILE = RT * ITEMS;           // 4096
constexpr int CHUNK = 8192;                // numpy's reduction buffer (NPY_BUFSIZE elements)
constexpr int LEAF = 128;                  // numpy's PW_BLOCKSIZE
constexpr int MAX_LEAVES = RT;             // a chunk has at most 8192 / 57 leaves

struct RocLayout {
  size_t key_a, key_b, lab_a, lab_b, hist, dtot, tbad, part_p, part_e, scal, e_tps, e_fps, csum, total;
  int ntiles, nchunks;
};

size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

RocLayout roc_layout(int64_t n) {
  RocLayout L;
  L.ntiles = (int)((n + TILE - 1) / TILE);
  L.nchunks = (int)((n + CHUNK - 1) / CHUNK);
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t at = o; o = align_up(o + bytes); return at; };
  L.key_a = take(4 * (size_t)n);
  L.key_b = take(4 * (size_t)n);
  L.lab_a = take((size_t)n);
  L.lab_b = take((size_t)n);
  L.hist = take(4 * (size_t)256 * L.ntiles);
  L.dtot = take(4 * 256);
  L.tbad = take(4 * (size_t)L.ntiles);
  L.part_p = take(8 * (size_t)L.ntiles);
  L.part_e = take(8 * (size_t)L.ntiles);
  L.scal = take(8 * 4);  // positives, groups, kept points
  L.e_tps = take(4 * (size_t)n);
  L.e_fps = take(4 * (size_t)n);  // (the kept points reuse key_a / key_b: the keys are dead once the group ends are written)
  L.csum = take(8 * (size_t)L.nchunks);
  L.total = o;
  return L;
}

// exclusive scan over the workgroup (Hillis-Steele in LDS); `total` = sum over every thread
template <typename T>
__device__ T block_excl_scan(T v, T* sh, T& total) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int o = 1; o < RT; o <<= 1) {
    const T x = t >= o ? sh[t - o] : T(0);
    __syncthreads();
    sh[t] += x;
    __syncthreads();
  }
  total = sh[RT - 1];
  const T incl = sh[t];
  __syncthreads();
  return incl - v;
}

// +0 and -0 one key; larger score -> smaller key
__device__ __forceinline__ uint32_t desc_key(float s) {
  uint32_t u = __float_as_uint(s);
  if (u == 0x80000000u) u = 0u;
  const uint32_t asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ~asc;
}

// lanes of this wave whose digit equals this lane's (inactive and invalid lanes excluded); every lane of the wave must call it
__device__ __forceinline__ unsigned long long match_digit(uint32_t d, bool valid) {
  unsigned long long m = __ballot(valid);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const bool bit = (d >> b) & 1u;
    const unsigned long long bb = __ballot(bit);
    m &= bit ? bb : ~bb;
  }
  return m;
}

__device__ __forceinline__ unsigned long long lanes_below() { return (1ull << (threadIdx.x & 63)) - 1ull; }

// per-tile histogram of one digit: one LDS add per (wave, digit) present
__device__ void tile_hist(const uint32_t (&keys)[ITEMS], int base, int64_t n, int shift, uint32_t* cnt) {
#pragma unroll
  for (int c = 0; c < ITEMS; ++c) {
    const int i = base + c * RT + threadIdx.x;
    const bool valid = i < n;
    const uint32_t d = (keys[c] >> shift) & 255u;
    const unsigned long long m = match_digit(d, valid);
    if (valid && (m & lanes_below()) == 0) atomicAdd(&cnt[d], (uint32_t)__popcll(m));
  }
}

__global__ __launch_bounds__(RT) void roc_keys_kernel(const float* __restrict__ score, const float* __restrict__ label, int64_t n,
                                                      int ntiles, uint32_t* __restrict__ key, uint8_t* __restrict__ lab,
                                                      uint32_t* __restrict__ hist, uint32_t* __restrict__ tbad) {
  __shared__ uint32_t cnt[256];
  __shared__ uint32_t bad_sh;
  const int tile = blockIdx.x, base = tile * TILE;
  cnt[threadIdx.x] = 0;
  if (threadIdx.x == 0) bad_sh = 0;
  __syncthreads();
  uint32_t keys[ITEMS];
  uint32_t bad = 0;
#pragma unroll
  for (int c = 0; c < ITEMS; ++c) {
    const int i = base + c * RT + threadIdx.x;
    keys[c] = 0;
    if (i < n) {
      const float s = score[i], y = label[i];
      if (!isfinite(s)) bad |= NASREC_ROC_AUC_NOT_FINITE;
      if (!(y == 0.f || y == 1.f)) bad |= NASREC_ROC_AUC_BAD_LABEL;
      keys[c] = desc_key(s);
      key[i] = keys[c];
      lab[i] = y == 1.f;
    }
  }
  tile_hist(keys, base, n, 0, cnt);
  if (bad) atomicOr(&bad_sh, bad);
  __syncthreads();
  hist[(int64_t)threadIdx.x * ntiles + tile] = cnt[threadIdx.x];
  if (threadIdx.x == 0) tbad[tile] = bad_sh;
}

__global__ __launch_bounds__(RT) void roc_hist_kernel(const uint32_t* __restrict__ key, int64_t n, int ntiles, int shift,
                                                      uint32_t* __restrict__ hist) {
  __shared__ uint32_t cnt[256];
  const int tile = blockIdx.x, base = tile * TILE;
  cnt[threadIdx.x] = 0;
  __syncthreads();
  uint32_t keys[ITEMS];
#pragma unroll
  for (int c = 0; c < ITEMS; ++c) {
    const int i = base + c * RT + threadIdx.x;
    keys[c] = i < n ? key[i] : 0u;
  }
  tile_hist(keys, base, n, shift, cnt);
  __syncthreads();
  hist[(int64_t)threadIdx.x * ntiles + tile] = cnt[threadIdx.x];
}

// workgroup d: exclusive scan of digit d's counts over the tiles (in place), dtot[d] = its total
__global__ __launch_bounds__(RT) void roc_digit_scan_kernel(uint32_t* __restrict__ hist, int ntiles, uint32_t* __restrict__ dtot) {
  __shared__ uint32_t sh[RT];
  uint32_t* h = hist + (int64_t)blockIdx.x * ntiles;
  uint32_t carry = 0;
  for (int b = 0; b < ntiles; b += RT) {
    const int t = b + threadIdx.x;
    const uint32_t v = t < ntiles ? h[t] : 0u;
    uint32_t tot;
    const uint32_t ex = block_excl_scan(v, sh, tot);
    if (t < ntiles) h[t] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) dtot[blockIdx.x] = carry;
}

// stable scatter of one 8-bit digit: element (chunk c, wave w, lane l) of a tile lands at
//   start of its digit + count of that digit in earlier tiles + in earlier chunks of this tile + in earlier waves of this chunk
//   + in earlier lanes of this wave
__global__ __launch_bounds__(RT) void roc_scatter_kernel(const uint32_t* __restrict__ key_in, const uint8_t* __restrict__ lab_in,
                                                         uint32_t* __restrict__ key_out, uint8_t* __restrict__ lab_out, int64_t n,
                                                         int ntiles, int shift, const uint32_t* __restrict__ hist,
                                                         const uint32_t* __restrict__ dtot) {
  __shared__ uint32_t sh[RT];
  __shared__ uint32_t start[256];
  __shared__ uint32_t wcnt[RT / 64][256];
  const int tile = blockIdx.x, base = tile * TILE, t = threadIdx.x, w = t >> 6;
  uint32_t tot;
  const uint32_t dbase = block_excl_scan(dtot[t], sh, tot);
  start[t] = dbase + hist[(int64_t)t * ntiles + tile];
#pragma unroll
  for (int v = 0; v < RT / 64; ++v) wcnt[v][t] = 0;
  __syncthreads();
  for (int c = 0; c < ITEMS; ++c) {
    if (base + c * RT >= n) break;  // (uniform over the workgroup)
    const int i = base + c * RT + t;
    const bool valid = i < n;
    const uint32_t k = valid ? key_in[i] : 0u;
    const uint8_t y = valid ? lab_in[i] : (uint8_t)0;
    const uint32_t d = (k >> shift) & 255u;
    const unsigned long long m = match_digit(d, valid);
    const uint32_t rank = (uint32_t)__popcll(m & lanes_below());
    if (valid && rank == 0) wcnt[w][d] = (uint32_t)__popcll(m);
    __syncthreads();
    if (valid) {
      uint32_t pos = start[d] + rank;
      for (int v = 0; v < w; ++v) pos += wcnt[v][d];
      key_out[pos] = k;
      lab_out[pos] = y;
    }
    __syncthreads();
    uint32_t add = 0;
#pragma unroll
    for (int v = 0; v < RT / 64; ++v) {
      add += wcnt[v][t];
      wcnt[v][t] = 0;
    }
    start[t] += add;
    __syncthreads();
  }
}

// one workgroup: exclusive scan of a[0..nt) (and of b, if given) in place, totals into tot_a / tot_b
__global__ __launch_bounds__(RT) void roc_parts_scan_kernel(int64_t* __restrict__ a, int64_t* __restrict__ b, int nt,
                                                            int64_t* __restrict__ tot_a, int64_t* __restrict__ tot_b) {
  __shared__ int64_t sh[RT];
  int64_t ca = 0, cb = 0;
  for (int o = 0; o < nt; o += RT) {
    const int t = o + threadIdx.x;
    int64_t ta, tb;
    const int64_t ea = block_excl_scan<int64_t>(t < nt ? a[t] : 0, sh, ta);
    if (t < nt) a[t] = ca + ea;
    ca += ta;
    if (b) {
      const int64_t eb = block_excl_scan<int64_t>(t < nt ? b[t] : 0, sh, tb);
      if (t < nt) b[t] = cb + eb;
      cb += tb;
    }
  }
  if (threadIdx.x == 0) {
    *tot_a = ca;
    if (b) *tot_b = cb;
  }
}

// thread t of a tile owns the ITEMS consecutive elements from base + t * ITEMS; the sorted keys end a group where the next key differs
__device__ __forceinline__ void load_run(const uint32_t* key, const uint8_t* lab, int64_t n, int first, uint8_t (&y)[ITEMS],
                                         bool (&end)[ITEMS]) {
  uint32_t k[ITEMS + 1];
#pragma unroll
  for (int j = 0; j <= ITEMS; ++j) k[j] = first + j < n ? key[first + j] : 0u;
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    const int i = first + j;
    y[j] = i < n ? lab[i] : (uint8_t)0;
    end[j] = i < n && (i == n - 1 || k[j] != k[j + 1]);
  }
}

// per tile: positives and group ends (a count only, so element c * 256 + t of the tile goes to thread t: coalesced)
__global__ __launch_bounds__(RT) void roc_group_count_kernel(const uint32_t* __restrict__ key, const uint8_t* __restrict__ lab, int64_t n,
                                                             int64_t* __restrict__ part_p, int64_t* __restrict__ part_e) {
  __shared__ int64_t sh[RT];
  int64_t p = 0, e = 0;
#pragma unroll
  for (int c = 0; c < ITEMS; ++c) {
    const int i = blockIdx.x * TILE + c * RT + threadIdx.x;
    if (i < n) {
      p += lab[i];
      e += i == n - 1 || key[i] != key[i + 1];
    }
  }
  int64_t tp, te;
  block_excl_scan(p, sh, tp);
  block_excl_scan(e, sh, te);
  if (threadIdx.x == 0) {
    part_p[blockIdx.x] = tp;
    part_e[blockIdx.x] = te;
  }
}

// at the g-th group end (sorted position i): tps = positives in [0, i], fps = i + 1 - tps
__global__ __launch_bounds__(RT) void roc_group_write_kernel(const uint32_t* __restrict__ key, const uint8_t* __restrict__ lab, int64_t n,
                                                             const int64_t* __restrict__ part_p, const int64_t* __restrict__ part_e,
                                                             int32_t* __restrict__ e_tps, int32_t* __restrict__ e_fps) {
  __shared__ int64_t sh[RT];
  const int first = blockIdx.x * TILE + threadIdx.x * ITEMS;
  uint8_t y[ITEMS];
  bool end[ITEMS];
  load_run(key, lab, n, first, y, end);
  int64_t p = 0, e = 0;
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    p += y[j];
    e += end[j];
  }
  int64_t tp, te;
  p = part_p[blockIdx.x] + block_excl_scan(p, sh, tp);
  e = part_e[blockIdx.x] + block_excl_scan(e, sh, te);
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    p += y[j];
    if (end[j]) {
      e_tps[e] = (int32_t)p;
      e_fps[e] = (int32_t)(first + j + 1 - p);
      ++e;
    }
  }
}

// sklearn's drop_intermediate: with more than two groups, keep the first, the last and every group where (fps, tps) has a non-zero
// second difference, i.e. where the step into the group differs from the step out of it
__device__ __forceinline__ bool keep_group(const int32_t* tps, const int32_t* fps, int64_t g, int64_t m) {
  if (g >= m) return false;
  if (m <= 2 || g == 0 || g == m - 1) return true;
  return fps[g] - fps[g - 1] != fps[g + 1] - fps[g] || tps[g] - tps[g - 1] != tps[g + 1] - tps[g];
}

// per tile of groups: the kept ones (a count only: group c * 256 + t of the tile goes to thread t, coalesced)
__global__ __launch_bounds__(RT) void roc_keep_count_kernel(const int32_t* __restrict__ e_tps, const int32_t* __restrict__ e_fps,
                                                            const int64_t* __restrict__ scal, int64_t* __restrict__ part) {
  __shared__ int64_t sh[RT];
  const int64_t m = scal[1];
  int64_t c = 0;
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) c += keep_group(e_tps, e_fps, (int64_t)blockIdx.x * TILE + j * RT + threadIdx.x, m);
  int64_t tc;
  block_excl_scan(c, sh, tc);
  if (threadIdx.x == 0) part[blockIdx.x] = tc;
}

__global__ __launch_bounds__(RT) void roc_keep_write_kernel(const int32_t* __restrict__ e_tps, const int32_t* __restrict__ e_fps,
                                                            const int64_t* __restrict__ scal, const int64_t* __restrict__ part,
                                                            int32_t* __restrict__ k_tps, int32_t* __restrict__ k_fps) {
  __shared__ int64_t sh[RT];
  const int64_t m = scal[1], first = (int64_t)blockIdx.x * TILE + threadIdx.x * ITEMS;
  bool keep[ITEMS];
  int64_t c = 0;
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    keep[j] = keep_group(e_tps, e_fps, first + j, m);
    c += keep[j];
  }
  int64_t tc;
  int64_t k = part[blockIdx.x] + block_excl_scan(c, sh, tc);
#pragma unroll
  for (int j = 0; j < ITEMS; ++j)
    if (keep[j]) {
      k_tps[k] = e_tps[first + j];
      k_fps[k] = e_fps[first + j];
      ++k;
    }
}

// numpy's leaf of pairwise_sum over the terms [s, s + len) of the curve: term k = (fpr[k] - fpr[k-1]) * (tpr[k] + tpr[k-1]) / 2.0 with
// (fpr, tpr)[-1] = (0, 0), fpr = fps / N and tpr = tps / P each one IEEE division.  No contraction anywhere below.
__device__ double leaf_sum(const int32_t* __restrict__ k_tps, const int32_t* __restrict__ k_fps, int s, int len, double dN, double dP) {
#pragma clang fp contract(off)
  double f0 = 0.0, t0 = 0.0;
  if (s > 0) {
    f0 = (double)k_fps[s - 1] / dN;
    t0 = (double)k_tps[s - 1] / dP;
  }
  auto term = [&](int k) {
    const double f1 = (double)k_fps[k] / dN, t1 = (double)k_tps[k] / dP;
    const double r = (f1 - f0) * (t1 + t0) / 2.0;
    f0 = f1;
    t0 = t1;
    return r;
  };
  if (len < 8) {
    double res = 0.0;
    for (int i = 0; i < len; ++i) res = res + term(s + i);
    return res;
  }
  double r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = term(s + j);
  int i = 8;
  for (; i < len - len % 8; i += 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = r[j] + term(s + i + j);
  }
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < len; ++i) res = res + term(s + i);
  return res;
}

struct Seg {
  int s, n, split;
};

// numpy's split of a block longer than 128: n2 = n / 2 rounded down to a multiple of 8
__device__ __forceinline__ int pw_split(int n) {
  const int n2 = n / 2;
  return n2 - n2 % 8;
}

// chunk c = terms [c * 8192, min(K, (c + 1) * 8192)): leaves in tree order (thread 0), one leaf per thread, the tree (thread 0)
__global__ __launch_bounds__(RT) void roc_chunk_kernel(const int32_t* __restrict__ k_tps, const int32_t* __restrict__ k_fps,
                                                       const int64_t* __restrict__ scal, int64_t n, double* __restrict__ csum) {
#pragma clang fp contract(off)
  __shared__ int leaf_s[MAX_LEAVES], leaf_n[MAX_LEAVES];
  __shared__ double leaf_v[MAX_LEAVES];
  __shared__ int nleaves;
  const int64_t P = scal[0], K = scal[2];
  const int64_t c0 = (int64_t)blockIdx.x * CHUNK;
  if (c0 >= K) return;
  const int len = (int)(K - c0 < CHUNK ? K - c0 : CHUNK);
  if (threadIdx.x == 0) {
    Seg st[32];
    int sp = 0, L = 0;
    st[sp++] = {0, len, 0};
    while (sp) {
      const Seg x = st[--sp];
      if (x.n <= LEAF) {
        leaf_s[L] = x.s;
        leaf_n[L] = x.n;
        ++L;
      } else {
        const int n2 = pw_split(x.n);
        st[sp++] = {x.s + n2, x.n - n2, 0};
        st[sp++] = {x.s, n2, 0};
      }
    }
    nleaves = L;
  }
  __syncthreads();
  const double dP = (double)P, dN = (double)(n - P);
  if ((int)threadIdx.x < nleaves)
    leaf_v[threadIdx.x] = leaf_sum(k_tps, k_fps, (int)c0 + leaf_s[threadIdx.x], leaf_n[threadIdx.x], dN, dP);
  __syncthreads();
  if (threadIdx.x == 0) {  // post-order walk of the same tree: pairwise(left) + pairwise(right)
    Seg st[32];
    double val[32];
    int sp = 0, vp = 0, li = 0;
    st[sp++] = {0, len, 0};
    while (sp) {
      const Seg x = st[--sp];
      if (x.n <= LEAF) {
        val[vp++] = leaf_v[li++];
      } else if (x.split) {
        const double right = val[--vp], left = val[--vp];
        val[vp++] = left + right;
      } else {
        const int n2 = pw_split(x.n);
        st[sp++] = {x.s, x.n, 1};
        st[sp++] = {x.s + n2, x.n - n2, 0};
        st[sp++] = {x.s, n2, 0};
      }
    }
    csum[blockIdx.x] = val[0];
  }
}

__global__ __launch_bounds__(RT) void roc_final_kernel(const double* __restrict__ csum, const int64_t* __restrict__ scal, int64_t n,
                                                       const uint32_t* __restrict__ tbad, int ntiles, void* out) {
#pragma clang fp contract(off)
  __shared__ uint32_t bad_sh;
  if (threadIdx.x == 0) bad_sh = 0;
  __syncthreads();
  uint32_t bad = 0;
  for (int t = threadIdx.x; t < ntiles; t += RT) bad |= tbad[t];
  if (bad) atomicOr(&bad_sh, bad);
  __syncthreads();
  if (threadIdx.x == 0) {
    const int64_t P = scal[0], K = scal[2];
    const int64_t nch = (K + CHUNK - 1) / CHUNK;
    double acc = 0.0;
    for (int64_t c = 0; c < nch; ++c) acc = acc + csum[c];
    uint32_t status = bad_sh;
    if (P == 0 || P == n) status |= NASREC_ROC_AUC_ONE_CLASS;
    *(double*)out = acc;
    *(int32_t*)((char*)out + 8) = (int32_t)status;
  }
}

__global__ void roc_too_few_kernel(void* out) {
  *(double*)out = __builtin_nan("");
  *(int32_t*)((char*)out + 8) = NASREC_ROC_AUC_TOO_FEW;
}

}  // namespace

extern "C" int64_t nasrec_roc_auc_workspace_bytes(int64_t n) {
  if (n < 2 || n > NASREC_ROC_AUC_MAX_N) return 0;
  return (int64_t)roc_layout(n).total;
}

int launch_roc_auc(hipStream_t st, const nasrec_roc_auc_desc_t* d) {
  const int64_t n = d->n;
  if (!d->out) return nasrec_set_error(-1, "roc_auc: missing output");
  if (n > NASREC_ROC_AUC_MAX_N) return nasrec_set_error(-1, "roc_auc: n = %lld (at most %lld)", (long long)n, (long long)NASREC_ROC_AUC_MAX_N);
  if (n < 2) {
    hipLaunchKernelGGL(roc_too_few_kernel, dim3(1), dim3(1), 0, st, d->out);
    return nasrec_check_launch("roc_auc");
  }
  if (!d->score || !d->label || !d->workspace) return nasrec_set_error(-1, "roc_auc: missing pointer");
  const RocLayout L = roc_layout(n);
  if (d->workspace_bytes < (int64_t)L.total)
    return nasrec_set_error(-1, "roc_auc: workspace of %lld bytes, %lld needed", (long long)d->workspace_bytes, (long long)L.total);
  if (((uintptr_t)d->workspace & 255) != 0) return nasrec_set_error(-1, "roc_auc: workspace not 256-byte aligned");
  char* ws = (char*)d->workspace;
  uint32_t *key_a = (uint32_t*)(ws + L.key_a), *key_b = (uint32_t*)(ws + L.key_b), *hist = (uint32_t*)(ws + L.hist);
  uint8_t *lab_a = (uint8_t*)(ws + L.lab_a), *lab_b = (uint8_t*)(ws + L.lab_b);
  uint32_t *dtot = (uint32_t*)(ws + L.dtot), *tbad = (uint32_t*)(ws + L.tbad);
  int64_t *part_p = (int64_t*)(ws + L.part_p), *part_e = (int64_t*)(ws + L.part_e), *scal = (int64_t*)(ws + L.scal);
  int32_t *e_tps = (int32_t*)(ws + L.e_tps), *e_fps = (int32_t*)(ws + L.e_fps);
  int32_t *k_tps = (int32_t*)key_a, *k_fps = (int32_t*)key_b;  // written by the keep launch, after the last reader of the keys
  double* csum = (double*)(ws + L.csum);
  const dim3 tiles(L.ntiles), blk(RT);

  hipLaunchKernelGGL(roc_keys_kernel, tiles, blk, 0, st, d->score, d->label, n, L.ntiles, key_a, lab_a, hist, tbad);
  for (int pass = 0; pass < 4; ++pass) {  // A -> B -> A -> B -> A
    uint32_t* kin = pass % 2 ? key_b : key_a;
    uint32_t* kout = pass % 2 ? key_a : key_b;
    uint8_t* lin = pass % 2 ? lab_b : lab_a;
    uint8_t* lout = pass % 2 ? lab_a : lab_b;
    if (pass > 0) hipLaunchKernelGGL(roc_hist_kernel, tiles, blk, 0, st, kin, n, L.ntiles, 8 * pass, hist);
    hipLaunchKernelGGL(roc_digit_scan_kernel, dim3(256), blk, 0, st, hist, L.ntiles, dtot);
    hipLaunchKernelGGL(roc_scatter_kernel, tiles, blk, 0, st, kin, lin, kout, lout, n, L.ntiles, 8 * pass, hist, dtot);
  }
  hipLaunchKernelGGL(roc_group_count_kernel, tiles, blk, 0, st, key_a, lab_a, n, part_p, part_e);
  hipLaunchKernelGGL(roc_parts_scan_kernel, dim3(1), blk, 0, st, part_p, part_e, L.ntiles, scal + 0, scal + 1);
  hipLaunchKernelGGL(roc_group_write_kernel, tiles, blk, 0, st, key_a, lab_a, n, part_p, part_e, e_tps, e_fps);
  hipLaunchKernelGGL(roc_keep_count_kernel, tiles, blk, 0, st, e_tps, e_fps, scal, part_p);
  hipLaunchKernelGGL(roc_parts_scan_kernel, dim3(1), blk, 0, st, part_p, (int64_t*)nullptr, L.ntiles, scal + 2, (int64_t*)nullptr);
  hipLaunchKernelGGL(roc_keep_write_kernel, tiles, blk, 0, st, e_tps, e_fps, scal, part_p, k_tps, k_fps);
  hipLaunchKernelGGL(roc_chunk_kernel, dim3(L.nchunks), blk, 0, st, k_tps, k_fps, scal, n, csum);
  hipLaunchKernelGGL(roc_final_kernel, dim3(1), blk, 0, st, csum, scal, n, tbad, L.ntiles, d->out);
  return nasrec_check_launch("roc_auc");
}
