// Permutation feature importance of the 0D signals (reference src/feature_importance.py:29-134) as one device-side sweep:
// md_window_gather builds the windows of every permuted variant of a chunk of samples from ONE resident table (no permuted
// copy of the table exists), md_eval_accumulate turns the logits of all variants into what compute_loss (:29-71) keeps:
// the per-batch loss value, the confusion counts and, optionally, softmax column 0.
#include "common.h"
#include "softmax_loss.h"

// out[v][i][t][f] = table[p_{v,f}(start[i] + t*tau)][f];  p_{v,f} = perms[colperm[v][f]] or the identity for -1.
// One thread per element: f is the fastest index, so the table row and the output are read / written coalesced; only a
// permuted column is a scattered 4-byte read.  Table and permutations are re-read by overlapping windows and by every variant
// and are served from L2 / infinity cache.  A row outside [0, R) (the host wrappers refuse such starts) reads as 0.
__global__ __launch_bounds__(256) void k_window_gather(const float* __restrict__ table, long long R, int F,
                                                       const int64_t* __restrict__ start, int n, int T, int tau,
                                                       const int32_t* __restrict__ perms, int P,
                                                       const int32_t* __restrict__ colperm, long long total,
                                                       float* __restrict__ out) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int f = (int)(e % F);
  long long q = e / F;
  const int t = (int)(q % T); q /= T;
  const int i = (int)(q % n);
  const int v = (int)(q / n);
  long long row = (long long)start[i] + (long long)t * tau;
  float val = 0.f;
  if (row >= 0 && row < R) {
    const int cp = colperm[v * F + f];
    if (cp >= 0 && cp < P) row = perms[(long long)cp * R + row];
    if (row >= 0 && row < R) val = table[row * F + f];
  }
  out[e] = val;
}

extern "C" int md_window_gather(const float* table, int64_t R, int32_t F, const int64_t* start, int32_t n, int32_t T,
                                int32_t tau, const int32_t* perms, int32_t P, const int32_t* colperm, int32_t V, float* out,
                                void* stream) {
  if (!table || !start || !colperm || !out) return MD_ERR_NULL;
  if (P > 0 && !perms) return MD_ERR_NULL;
  if (R <= 0 || F <= 0 || n <= 0 || T <= 0 || tau <= 0 || P < 0 || V <= 0) return MD_ERR_BAD_SHAPE;
  if (R > 0x7fffffffLL) return MD_ERR_UNSUPPORTED;                  // permutations are int32 row numbers
  const long long total = (long long)V * n * T * F;
  const long long blocks = (total + 255) / 256;
  if (blocks > 0x7fffffffLL) return MD_ERR_UNSUPPORTED;
  MD_KLAUNCH(k_window_gather, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, table, (long long)R, F, start, n, T,
             tau, perms, P, colperm, total, out);
  MD_CHECK_LAUNCH();
  return MD_OK;
}

// One workgroup per (segment, variant).  A segment is one batch of the loader inside the chunk: samples seg[s] .. seg[s+1]-1.
// Thread t takes samples lo+t, lo+t+256, ... in increasing order (fp64 running sums of the fp32 terms, as k_softmax_loss), the
// 64 lanes of a wave are folded with shuffles (offsets 32, 16, .., 1), the four waves are added in wave order by thread 0:
// a fixed order, two runs give the same bits.  The counts go through LDS and integer atomics.  A target outside [0, K)
// contributes nothing.
#define MD_EVAL_MAXK 8
__device__ __forceinline__ double md_wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void k_eval_accumulate(int kind, const float* __restrict__ x, const int64_t* __restrict__ y,
                                                         int n, int K, const int32_t* __restrict__ seg,
                                                         const float* __restrict__ cw, const float* __restrict__ margins,
                                                         float gs, float* __restrict__ loss, long long loss_stride,
                                                         int32_t* __restrict__ conf, float* __restrict__ p0) {
  __shared__ double red[4], redw[4];
  __shared__ int cnt[MD_EVAL_MAXK * MD_EVAL_MAXK];
  const int t = threadIdx.x, s = blockIdx.x, v = blockIdx.y;
  if (t < K * K) cnt[t] = 0;
  __syncthreads();
  int lo = seg[s], hi = seg[s + 1];
  lo = lo < 0 ? 0 : lo; hi = hi > n ? n : hi;
  const float* xv = x + (long long)v * n * K;
  double lsum = 0.0, wsum = 0.0;
  for (int b = lo + t; b < hi; b += 256) {
    const long long yl = y[b];
    const float* xr = xv + (long long)b * K;
    if (p0) {
      float mx = xr[0];
      for (int k = 1; k < K; ++k) mx = fmaxf(mx, xr[k]);
      float se = 0.f;
      for (int k = 0; k < K; ++k) se += expf(xr[k] - mx);
      p0[(long long)v * n + b] = expf(xr[0] - mx) / se;
    }
    if (yl < 0 || yl >= K) continue;
    float z[MD_LOSS_MAXK];
    const MdSampleLoss r = md_sample_loss(kind, xr, (int)yl, K, cw, margins, gs, z);
    lsum += (double)r.term;
    wsum += (double)r.w;
    atomicAdd(&cnt[(int)yl * K + r.arg], 1);
  }
  lsum = md_wave_sum(lsum); wsum = md_wave_sum(wsum);
  if ((t & 63) == 0) { red[t >> 6] = lsum; redw[t >> 6] = wsum; }
  __syncthreads();
  if (t == 0) {
    const double L = ((red[0] + red[1]) + red[2]) + red[3];
    const double W = ((redw[0] + redw[1]) + redw[2]) + redw[3];
    loss[(long long)v * loss_stride + s] = (float)(kind == 1 ? L / W : L);
  }
  if (conf && t < K * K && cnt[t]) atomicAdd(&conf[(long long)v * K * K + t], cnt[t]);
}

extern "C" int md_eval_accumulate(int32_t kind, const float* logits, const int64_t* target, int32_t V, int32_t n, int32_t K,
                                  const int32_t* seg, int32_t S, const float* class_weight, const float* margins,
                                  float gamma_or_s, float* loss, int64_t loss_stride, int32_t* confusion, float* p0,
                                  void* stream) {
  if (!logits || !target || !seg || !loss) return MD_ERR_NULL;
  if (kind < 0 || kind > 2) return MD_ERR_UNSUPPORTED;
  if (V <= 0 || n <= 0 || K <= 0 || S <= 0 || loss_stride < S) return MD_ERR_BAD_SHAPE;
  if (K > MD_EVAL_MAXK || V > 65535) return MD_ERR_UNSUPPORTED;
  MD_KLAUNCH(k_eval_accumulate, dim3((unsigned)S, (unsigned)V), dim3(256), 0, (hipStream_t)stream, kind, logits, target, n, K,
             seg, class_weight, margins, gamma_or_s, loss, (long long)loss_stride, confusion, p0);
  MD_CHECK_LAUNCH();
  return MD_OK;
}
