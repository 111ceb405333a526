// Latent-space maps: the reductions behind src/visualization/visualize_latent_space.py.
//
// Exact t-SNE (what scikit-learn's TSNE(method="exact") computes) in five stages -- pairwise squared distances in the direct form,
// the per-row perplexity bisection with the row held in LDS, the symmetrised joint P, one pass over P per iteration for the
// gradient (Y tiled through LDS, a wave owns four rows of P), and the gains / momentum step -- and the three tall-skinny pieces an
// incremental PCA by subspace iteration needs (column means, W = M V, Z = M^T W with the batch centring and the few extra rows of
// scikit-learn's stacked matrix applied while M is read).
//
// Every reduction is fixed-order: per-lane partials in index order, a shuffle tree inside a wave, waves / workgroups summed in index
// order by a second stage.  No atomics: two runs on the same input give the same bits.  Long sums are carried in fp64.
#include "common.h"

#include <math.h>

namespace {

constexpr double kEps = 2.220446049250313e-16;   // MACHINE_EPSILON of scikit-learn's t-SNE

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return __shfl(v, 0, 64);
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return __shfl(v, 0, 64);
}
// sum over a 256-thread workgroup, every thread gets the result; `red` is 4 doubles the caller does not reuse before its next barrier
__device__ __forceinline__ double block_sum(double v, double* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// ------------------------------------------------------------------------------------------------------------ distances
constexpr int SQ_T = 64, SQ_K = 16;

// out[i][j] = sum_k (x[i][k] - x[j][k])^2.  64 x 64 tile per workgroup, 4 x 4 per thread, 16 columns of x per LDS stage.  (i, j) and
// (j, i) see the same differences with opposite sign in the same order, so the result is symmetric to the bit and the diagonal is 0.
__global__ __launch_bounds__(256) void k_sqdist(const float* __restrict__ x, int N, int D, float* __restrict__ out) {
  __shared__ float As[SQ_K][SQ_T + 1], Bs[SQ_K][SQ_T + 1];
  const int tx = threadIdx.x % 16, ty = threadIdx.x / 16;
  const int i0 = blockIdx.y * SQ_T, j0 = blockIdx.x * SQ_T;
  float acc[4][4] = {};
  for (int k0 = 0; k0 < D; k0 += SQ_K) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int idx = threadIdx.x + e * 256, r = idx / SQ_K, k = idx % SQ_K;
      const bool kin = k0 + k < D;
      As[k][r] = (kin && i0 + r < N) ? x[(size_t)(i0 + r) * D + k0 + k] : 0.f;
      Bs[k][r] = (kin && j0 + r < N) ? x[(size_t)(j0 + r) * D + k0 + k] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SQ_K; ++k) {
      float a[4], b[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) { a[u] = As[k][ty + 16 * u]; b[u] = Bs[k][tx + 16 * u]; }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) { const float d = a[u] - b[v]; acc[u][v] = fmaf(d, d, acc[u][v]); }
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int i = i0 + ty + 16 * u;
    if (i >= N) continue;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int j = j0 + tx + 16 * v;
      if (j < N) out[(size_t)i * N + j] = acc[u][v];
    }
  }
}

// ------------------------------------------------------------------------------------------------------------ conditional P
// One workgroup per row; the row of squared distances sits in LDS for all (at most 100) bisection steps.  Steps follow
// sklearn.manifold._utils._binary_search_perplexity: beta from 1, doubling / halving while a bound is infinite, stop at
// |H - ln(perplexity)| <= 1e-5.  exp in fp32 (its argument rounded once from the fp64 product), sums in fp64.  p_cond may be d2.
__global__ __launch_bounds__(256) void k_tsne_conditional(const float* d2, int N, float perplexity, float* p_cond) {
  extern __shared__ float row[];
  __shared__ double red[2][2][4];
  const int i = blockIdx.x, tid = threadIdx.x;
  const float* src = d2 + (size_t)i * N;
  for (int j = tid; j < N; j += 256) row[j] = src[j];
  __syncthreads();
  const double target = log((double)perplexity);
  double beta = 1.0, lo = -INFINITY, hi = INFINITY, used = 1.0, sum = 1.0;
  for (int it = 0; it < 100; ++it) {
    double s = 0.0, sd = 0.0;
    for (int j = tid; j < N; j += 256) {
      if (j == i) continue;
      const float d = row[j];
      const float p = expf((float)(-(double)d * beta));
      s += (double)p;
      sd += (double)d * (double)p;
    }
    double* r0 = red[it & 1][0];
    double* r1 = red[it & 1][1];
    s = wave_sum(s); sd = wave_sum(sd);
    if ((tid & 63) == 0) { r0[tid >> 6] = s; r1[tid >> 6] = sd; }
    __syncthreads();
    s = ((r0[0] + r0[1]) + r0[2]) + r0[3];
    sd = ((r1[0] + r1[1]) + r1[2]) + r1[3];
    if (s == 0.0) s = 1e-8;
    used = beta; sum = s;
    const double diff = log(s) + beta * (sd / s) - target;
    if (fabs(diff) <= 1e-5) break;
    if (diff > 0.0) {
      lo = beta;
      beta = hi == INFINITY ? beta * 2.0 : (beta + hi) * 0.5;
    } else {
      hi = beta;
      beta = lo == -INFINITY ? beta * 0.5 : (beta + lo) * 0.5;
    }
  }
  float* dst = p_cond + (size_t)i * N;
  for (int j = tid; j < N; j += 256)
    dst[j] = j == i ? 0.f : (float)((double)expf((float)(-(double)row[j] * used)) / sum);
}

// ------------------------------------------------------------------------------------------------------------ joint P
__global__ __launch_bounds__(256) void k_row_sum(const float* __restrict__ m, int N, double* __restrict__ rs) {
  __shared__ double red[4];
  const float* src = m + (size_t)blockIdx.x * N;
  double s = 0.0;
  for (int j = threadIdx.x; j < N; j += 256) s += (double)src[j];
  s = block_sum(s, red);
  if (threadIdx.x == 0) rs[blockIdx.x] = s;
}
// scale * sum of v[0..n) into out[0], one workgroup
__global__ __launch_bounds__(256) void k_vec_sum(const double* __restrict__ v, int n, double scale, double* __restrict__ out) {
  __shared__ double red[4];
  double s = 0.0;
  for (int j = threadIdx.x; j < n; j += 256) s += v[j];
  s = block_sum(s, red);
  if (threadIdx.x == 0) out[0] = s * scale;
}
// P[i][j] = P[j][i] = max((C[i][j] + C[j][i]) / max(total, eps), eps), diagonal 0.  A workgroup owns the tile pair (bi, bj), (bj, bi)
// with bj >= bi, reads both before it writes either: p may be p_cond.
__global__ __launch_bounds__(256) void k_tsne_joint(const float* c, int N, const double* __restrict__ total, float* p) {
  __shared__ float ta[32][33], tb[32][33];
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bj < bi) return;
  const int tx = threadIdx.x % 32, ty = threadIdx.x / 32;
  for (int r = ty; r < 32; r += 8) {
    const int i = bi * 32 + r, j = bj * 32 + tx;
    ta[r][tx] = (i < N && j < N) ? c[(size_t)i * N + j] : 0.f;
    const int i2 = bj * 32 + r, j2 = bi * 32 + tx;
    tb[r][tx] = (i2 < N && j2 < N) ? c[(size_t)i2 * N + j2] : 0.f;
  }
  __syncthreads();
  const double tot = fmax(total[0], kEps);
  for (int r = ty; r < 32; r += 8) {
    const int i = bi * 32 + r, j = bj * 32 + tx;
    if (i < N && j < N) {
      const double s = (double)ta[r][tx] + (double)tb[tx][r];
      p[(size_t)i * N + j] = i == j ? 0.f : (float)fmax(s / tot, kEps);
    }
    const int i2 = bj * 32 + r, j2 = bi * 32 + tx;
    if (bi != bj && i2 < N && j2 < N) {
      const double s = (double)ta[tx][r] + (double)tb[r][tx];
      p[(size_t)i2 * N + j2] = (float)fmax(s / tot, kEps);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------ gradient
constexpr int GR_ROWS = 4;       // rows of P per wave
constexpr int GR_TILE = 1024;    // embedding points per LDS stage

// One pass over P.  A wave owns GR_ROWS rows; its lanes walk the columns (coalesced reads of P), y_j comes from LDS.  With
// num = (1 + d / dof)^(-(dof + 1) / 2), dof = NC - 1 (1 for NC = 2): per row the attractive sum e P num (y_i - y_j), the repulsive sum
// num^2 (y_i - y_j), sum num, and for KL the row's sum e P ln(max(e P, eps) / num) and sum e P (the ln Z term is added once Z is known).
template <int NC, bool KL>
__global__ __launch_bounds__(256) void k_tsne_grad(const float* __restrict__ P, const float* __restrict__ y, int N, float ex,
                                                   float* __restrict__ rowpart, double* __restrict__ zpart,
                                                   double* __restrict__ klpart) {
  __shared__ float ys[NC][GR_TILE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row0 = (blockIdx.x * 4 + wave) * GR_ROWS;
  float yi[GR_ROWS][NC], at[GR_ROWS][NC], rp[GR_ROWS][NC];
  const float* prow[GR_ROWS];
  double zs[GR_ROWS], kls[GR_ROWS], ps[GR_ROWS];
#pragma unroll
  for (int r = 0; r < GR_ROWS; ++r) {
    const int i = row0 + r < N ? row0 + r : N - 1;      // rows past the end repeat the last one and are not written
    prow[r] = P + (size_t)i * N;
    zs[r] = kls[r] = ps[r] = 0.0;
#pragma unroll
    for (int c = 0; c < NC; ++c) { yi[r][c] = y[(size_t)i * NC + c]; at[r][c] = rp[r][c] = 0.f; }
  }
  for (int j0 = 0; j0 < N; j0 += GR_TILE) {
    __syncthreads();
    for (int t = tid; t < GR_TILE; t += 256) {
      const int j = j0 + t;
#pragma unroll
      for (int c = 0; c < NC; ++c) ys[c][t] = j < N ? y[(size_t)j * NC + c] : 0.f;
    }
    __syncthreads();
    const int tend = N - j0 < GR_TILE ? N - j0 : GR_TILE;
    for (int t = lane; t < tend; t += 64) {
      const int j = j0 + t;
      float yj[NC], pv[GR_ROWS];
#pragma unroll
      for (int c = 0; c < NC; ++c) yj[c] = ys[c][t];
#pragma unroll
      for (int r = 0; r < GR_ROWS; ++r) pv[r] = prow[r][j];
#pragma unroll
      for (int r = 0; r < GR_ROWS; ++r) {
        float df[NC], d = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) { df[c] = yi[r][c] - yj[c]; d = fmaf(df[c], df[c], d); }
        float num;
        if (NC == 2) {
          num = 1.f / (1.f + d);
        } else {
          const float u = fmaf(d, 0.5f, 1.f);
          num = 1.f / (u * sqrtf(u));
        }
        if (j == row0 + r) num = 0.f;                    // the diagonal takes no part in Z
        const float pe = ex * pv[r], w = pe * num, n2 = num * num;
#pragma unroll
        for (int c = 0; c < NC; ++c) { at[r][c] = fmaf(w, df[c], at[r][c]); rp[r][c] = fmaf(n2, df[c], rp[r][c]); }
        zs[r] += (double)num;
        if (KL && pe > 0.f && num > 0.f) {
          kls[r] += (double)pe * log(fmax((double)pe, kEps) / (double)num);
          ps[r] += (double)pe;
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < GR_ROWS; ++r) {
    const int i = row0 + r;
    float a[NC], b[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) { a[c] = wave_sum(at[r][c]); b[c] = wave_sum(rp[r][c]); }
    const double z = wave_sum(zs[r]);
    double k = 0.0, s = 0.0;
    if (KL) { k = wave_sum(kls[r]); s = wave_sum(ps[r]); }
    if (lane == 0 && i < N) {
#pragma unroll
      for (int c = 0; c < NC; ++c) { rowpart[(size_t)i * 2 * NC + c] = a[c]; rowpart[(size_t)i * 2 * NC + NC + c] = b[c]; }
      zpart[i] = z;
      if (KL) { klpart[i] = k; klpart[N + i] = s; }
    }
  }
}

// Second stage: Z = sum zpart (fp64, fixed order), grad = c (attractive - repulsive / Z), c = 2 (dof + 1) / dof; with KL also
// stats[1] = sum klpart + ln Z * sum e P.  stats[0] = Z.  One workgroup.
template <int NC>
__global__ __launch_bounds__(256) void k_tsne_finish(const float* __restrict__ rowpart, const double* __restrict__ zpart,
                                                     const double* __restrict__ klpart, int N, int want_kl,
                                                     float* __restrict__ grad, double* __restrict__ stats) {
  __shared__ double red[3][4];
  double z = 0.0, k = 0.0, s = 0.0;
  for (int i = threadIdx.x; i < N; i += 256) {
    z += zpart[i];
    if (want_kl) { k += klpart[i]; s += klpart[N + i]; }
  }
  z = block_sum(z, red[0]);
  if (want_kl) { k = block_sum(k, red[1]); s = block_sum(s, red[2]); }
  if (threadIdx.x == 0) {
    stats[0] = z;
    if (want_kl) { stats[1] = k + log(z) * s; stats[2] = s; }
  }
  const float cf = NC == 2 ? 4.f : 3.f;
  const float invz = (float)(1.0 / z);
  for (int e = threadIdx.x; e < N * NC; e += 256) {
    const int i = e / NC, c = e % NC;
    grad[e] = cf * (rowpart[(size_t)i * 2 * NC + c] - rowpart[(size_t)i * 2 * NC + NC + c] * invz);
  }
}

// scikit-learn's _gradient_descent step; gpart[block] = this workgroup's share of |gains * grad|^2
__global__ __launch_bounds__(256) void k_tsne_update(float* __restrict__ y, float* __restrict__ update, float* __restrict__ gains,
                                                     const float* __restrict__ grad, int n, float momentum, float lr,
                                                     float min_gain, double* __restrict__ gpart) {
  __shared__ double red[4];
  const int e = blockIdx.x * 256 + threadIdx.x;
  double sq = 0.0;
  if (e < n) {
    const float g = grad[e], u = update[e];
    float ga = gains[e];
    ga = u * g < 0.f ? ga + 0.2f : ga * 0.8f;
    ga = fmaxf(ga, min_gain);
    const float gg = ga * g;
    const float un = momentum * u - lr * gg;
    gains[e] = ga; update[e] = un; y[e] += un;
    sq = (double)gg * (double)gg;
  }
  sq = block_sum(sq, red);
  if (threadIdx.x == 0) gpart[blockIdx.x] = sq;
}

// ------------------------------------------------------------------------------------------------------------ tall-skinny (PCA)
constexpr int TS_Q = 8;          // columns of every skinny operand (k + oversampling, zero padded)

// Row r of the stacked matrix: a centred row of the batch (r < rows) or one of the E extra rows, taken as they are.
__device__ __forceinline__ float ts_elem(const float* M, int rows, int D, const float* mean, float mu, const float* extra, int r, int d) {
  return r < rows ? M[(size_t)r * D + d] - mu : extra[(size_t)(r - rows) * D + d];
}

// W[r][:] = row r of the stacked matrix times V[D][8]; a wave per row, fp64 FMA.
__global__ __launch_bounds__(256) void k_tsmm_mv(const float* __restrict__ M, int rows, int D, const float* __restrict__ mean,
                                                 const float* __restrict__ extra, int E, const float* __restrict__ V,
                                                 float* __restrict__ W) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows + E) return;
  double acc[TS_Q];
#pragma unroll
  for (int c = 0; c < TS_Q; ++c) acc[c] = 0.0;
  for (int d = lane; d < D; d += 64) {
    const float m = ts_elem(M, rows, D, mean, mean ? mean[d] : 0.f, extra, r, d);
    const float4 v0 = *(const float4*)(V + (size_t)d * TS_Q), v1 = *(const float4*)(V + (size_t)d * TS_Q + 4);
    const float v[TS_Q] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
    for (int c = 0; c < TS_Q; ++c) acc[c] = fma((double)m, (double)v[c], acc[c]);
  }
#pragma unroll
  for (int c = 0; c < TS_Q; ++c) acc[c] = wave_sum(acc[c]);
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < TS_Q; ++c) W[(size_t)r * TS_Q + c] = (float)acc[c];
  }
}

// part[split][d][:] = sum over this split's rows of stacked[r][d] * W[r][:]; a thread per column d, fp64 FMA.
__global__ __launch_bounds__(64) void k_tsmm_mtw(const float* __restrict__ M, int rows, int D, const float* __restrict__ mean,
                                                 const float* __restrict__ extra, int E, const float* __restrict__ W,
                                                 double* __restrict__ part) {
  const int d = blockIdx.x * 64 + threadIdx.x;
  if (d >= D) return;
  const int total = rows + E, per = (total + gridDim.y - 1) / gridDim.y;
  const int beg = blockIdx.y * per, end = beg + per < total ? beg + per : total;
  const float mu = mean ? mean[d] : 0.f;
  double acc[TS_Q];
#pragma unroll
  for (int c = 0; c < TS_Q; ++c) acc[c] = 0.0;
#pragma unroll 4
  for (int r = beg; r < end; ++r) {
    const float m = ts_elem(M, rows, D, mean, mu, extra, r, d);
    const float* w = W + (size_t)r * TS_Q;
#pragma unroll
    for (int c = 0; c < TS_Q; ++c) acc[c] = fma((double)m, (double)w[c], acc[c]);
  }
#pragma unroll
  for (int c = 0; c < TS_Q; ++c) part[((size_t)blockIdx.y * D + d) * TS_Q + c] = acc[c];
}
__global__ __launch_bounds__(256) void k_tsmm_mtw_fin(const double* __restrict__ part, int nsplit, int n, float* outf, double* outd) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  double s = 0.0;
  for (int k = 0; k < nsplit; ++k) s += part[(size_t)k * n + e];
  if (outf) outf[e] = (float)s;
  if (outd) outd[e] = s;
}

// part[split][d] = sum over this split's rows of x[r][d]
__global__ __launch_bounds__(64) void k_col_sum(const float* __restrict__ x, int rows, int D, double* __restrict__ part) {
  const int d = blockIdx.x * 64 + threadIdx.x;
  if (d >= D) return;
  const int per = (rows + gridDim.y - 1) / gridDim.y;
  const int beg = blockIdx.y * per, end = beg + per < rows ? beg + per : rows;
  double s = 0.0;
#pragma unroll 4
  for (int r = beg; r < end; ++r) s += (double)x[(size_t)r * D + d];
  part[(size_t)blockIdx.y * D + d] = s;
}
__global__ __launch_bounds__(256) void k_col_mean_fin(const double* __restrict__ part, int nsplit, int D, double inv, double* __restrict__ mean) {
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d >= D) return;
  double s = 0.0;
  for (int k = 0; k < nsplit; ++k) s += part[(size_t)k * D + d];
  mean[d] = s * inv;
}

// row splits of a column reduction: about 4096 waves in flight, at least 32 rows each
int ts_splits(int64_t rows, int D) {
  int64_t s = 4096 / md_cdiv(D, 64);
  const int64_t cap = md_cdiv64(rows, 32);
  if (s > cap) s = cap;
  if (s < 1) s = 1;
  return (int)s;
}

int embed_n_ok(int32_t N) { return N <= 0 ? MD_ERR_BAD_SHAPE : (N > MD_EMBED_MAX_N ? MD_ERR_UNSUPPORTED : MD_OK); }

}  // namespace

extern "C" {

int md_sqdist(const float* x, int32_t N, int32_t D, float* out, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!x || !out) return MD_ERR_NULL;
  if (D <= 0) return MD_ERR_BAD_SHAPE;
  if (int rc = embed_n_ok(N)) return rc;
  const int t = md_cdiv(N, SQ_T);
  MD_KLAUNCH(k_sqdist, dim3(t, t), dim3(256), 0, s, x, N, D, out);
  MD_CHECK_LAUNCH();
  return MD_OK;
}

int md_tsne_conditional(const float* d2, int32_t N, float perplexity, float* p_cond, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!d2 || !p_cond) return MD_ERR_NULL;
  if (int rc = embed_n_ok(N)) return rc;
  if (!(perplexity > 0.f)) return MD_ERR_BAD_SHAPE;
  const size_t lds = (size_t)N * sizeof(float);
  // above the default dynamic-LDS limit the attribute is raised on every such call: it is per device, cheap, and this entry point
  // runs once per map
  if (lds > 48 * 1024 && hipFuncSetAttribute((const void*)k_tsne_conditional, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)lds) != hipSuccess) {
    (void)hipGetLastError();
    return MD_ERR_UNSUPPORTED;
  }
  MD_KLAUNCH(k_tsne_conditional, dim3(N), dim3(256), lds, s, d2, N, perplexity, p_cond);
  MD_CHECK_LAUNCH();
  return MD_OK;
}

size_t md_tsne_joint_scratch_doubles(int32_t N) { return N > 0 ? (size_t)N + 1 : 0; }

int md_tsne_joint(const float* p_cond, int32_t N, float* p, double* scratch, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!p_cond || !p || !scratch) return MD_ERR_NULL;
  if (int rc = embed_n_ok(N)) return rc;
  MD_KLAUNCH(k_row_sum, dim3(N), dim3(256), 0, s, p_cond, N, scratch);
  MD_CHECK_LAUNCH();
  MD_KLAUNCH(k_vec_sum, dim3(1), dim3(256), 0, s, (const double*)scratch, N, 2.0, scratch + N);   // sum(C + C^T) = 2 sum(C)
  MD_CHECK_LAUNCH();
  const int t = md_cdiv(N, 32);
  MD_KLAUNCH(k_tsne_joint, dim3(t, t), dim3(256), 0, s, p_cond, N, (const double*)(scratch + N), p);
  MD_CHECK_LAUNCH();
  return MD_OK;
}

size_t md_tsne_rowpart_floats(int32_t N, int32_t nc) { return (N > 0 && (nc == 2 || nc == 3)) ? (size_t)N * 2 * nc : 0; }
size_t md_tsne_scratch_doubles(int32_t N) { return N > 0 ? (size_t)N * 3 : 0; }

int md_tsne_gradient(const float* p, const float* y, int32_t N, int32_t nc, float exaggeration, int32_t want_kl, float* rowpart,
                     double* scratch, float* grad, double* stats, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!p || !y || !rowpart || !scratch || !grad || !stats) return MD_ERR_NULL;
  if (int rc = embed_n_ok(N)) return rc;
  if (nc != 2 && nc != 3) return MD_ERR_UNSUPPORTED;
  double* zpart = scratch;
  double* klpart = scratch + N;
  const dim3 g(md_cdiv(N, 4 * GR_ROWS)), b(256);
  if (nc == 2) {
    if (want_kl) MD_KLAUNCH((k_tsne_grad<2, true>), g, b, 0, s, p, y, N, exaggeration, rowpart, zpart, klpart);
    else MD_KLAUNCH((k_tsne_grad<2, false>), g, b, 0, s, p, y, N, exaggeration, rowpart, zpart, klpart);
  } else {
    if (want_kl) MD_KLAUNCH((k_tsne_grad<3, true>), g, b, 0, s, p, y, N, exaggeration, rowpart, zpart, klpart);
    else MD_KLAUNCH((k_tsne_grad<3, false>), g, b, 0, s, p, y, N, exaggeration, rowpart, zpart, klpart);
  }
  MD_CHECK_LAUNCH();
  if (nc == 2)
    MD_KLAUNCH(k_tsne_finish<2>, dim3(1), b, 0, s, (const float*)rowpart, (const double*)zpart, (const double*)klpart, N, want_kl, grad, stats);
  else
    MD_KLAUNCH(k_tsne_finish<3>, dim3(1), b, 0, s, (const float*)rowpart, (const double*)zpart, (const double*)klpart, N, want_kl, grad, stats);
  MD_CHECK_LAUNCH();
  return MD_OK;
}

int32_t md_tsne_update_blocks(int64_t n) { return n > 0 ? (int32_t)md_cdiv64(n, 256) : 0; }

int md_tsne_update(float* y, float* update, float* gains, const float* grad, int64_t n, float momentum, float lr, float min_gain,
                   double* gpart, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!y || !update || !gains || !grad || !gpart) return MD_ERR_NULL;
  if (n <= 0 || n > (int64_t)MD_EMBED_MAX_N * 3) return MD_ERR_BAD_SHAPE;
  MD_KLAUNCH(k_tsne_update, dim3(md_tsne_update_blocks(n)), dim3(256), 0, s, y, update, gains, grad, (int)n, momentum, lr, min_gain, gpart);
  MD_CHECK_LAUNCH();
  return MD_OK;
}

size_t md_col_mean_scratch_doubles(int64_t rows, int32_t D) {
  return (rows > 0 && D > 0) ? (size_t)ts_splits(rows, D) * D : 0;
}

int md_col_mean(const float* x, int64_t rows, int32_t D, double* mean, double* scratch, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!x || !mean || !scratch) return MD_ERR_NULL;
  if (rows <= 0 || D <= 0 || rows > INT32_MAX) return MD_ERR_BAD_SHAPE;
  const int ns = ts_splits(rows, D);
  MD_KLAUNCH(k_col_sum, dim3(md_cdiv(D, 64), ns), dim3(64), 0, s, x, (int)rows, D, scratch);
  MD_CHECK_LAUNCH();
  MD_KLAUNCH(k_col_mean_fin, dim3(md_cdiv(D, 256)), dim3(256), 0, s, (const double*)scratch, ns, D, 1.0 / (double)rows, mean);
  MD_CHECK_LAUNCH();
  return MD_OK;
}

static int ts_check(const float* M, int64_t rows, int32_t D, const float* extra, int32_t E) {
  if (!M) return MD_ERR_NULL;
  if (rows <= 0 || D <= 0 || E < 0 || rows + E > INT32_MAX) return MD_ERR_BAD_SHAPE;
  if (E > 0 && !extra) return MD_ERR_NULL;
  return MD_OK;
}

int md_tsmm_mv(const float* M, int64_t rows, int32_t D, const float* mean, const float* extra, int32_t E, const float* V, float* W,
               void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!V || !W) return MD_ERR_NULL;
  if (int rc = ts_check(M, rows, D, extra, E)) return rc;
  MD_KLAUNCH(k_tsmm_mv, dim3((unsigned)md_cdiv64(rows + E, 4)), dim3(256), 0, s, M, (int)rows, D, mean, extra, E, V, W);
  MD_CHECK_LAUNCH();
  return MD_OK;
}

size_t md_tsmm_mtw_scratch_doubles(int64_t rows, int32_t D, int32_t E) {
  return (rows > 0 && D > 0 && E >= 0) ? (size_t)ts_splits(rows + E, D) * D * TS_Q : 0;
}

int md_tsmm_mtw(const float* M, int64_t rows, int32_t D, const float* mean, const float* extra, int32_t E, const float* W, float* out_f32,
                double* out_f64, double* scratch, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!W || !scratch || (!out_f32 && !out_f64)) return MD_ERR_NULL;
  if (int rc = ts_check(M, rows, D, extra, E)) return rc;
  const int ns = ts_splits(rows + E, D);
  MD_KLAUNCH(k_tsmm_mtw, dim3(md_cdiv(D, 64), ns), dim3(64), 0, s, M, (int)rows, D, mean, extra, E, W, scratch);
  MD_CHECK_LAUNCH();
  const int n = D * TS_Q;
  MD_KLAUNCH(k_tsmm_mtw_fin, dim3(md_cdiv(n, 256)), dim3(256), 0, s, (const double*)scratch, ns, n, out_f32, out_f64);
  MD_CHECK_LAUNCH();
  return MD_OK;
}

}  // extern "C"
