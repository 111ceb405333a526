// Deep CCA on the device (reference src/CCA.py:25-83): a batched symmetric eigensolver that lives in LDS, the CCA loss built on it and
// the loss's closed-form gradient.  DESIGN.md section 13 has the method, the LDS budget and the measurements.
//
//   k_sym_eig      one workgroup per matrix; A and V in LDS (fp32, odd pitch); parallel-order cyclic Jacobi
//   k_cca_center   column means (fp64) and the centred views
//   k_cca_cov      the three covariance products, fp64-accumulated FMAs
//   k_cca_gemm     the o x o (and m x o) products of the loss and its gradient: exact fp32 FMAs, fixed order, up to 3 per launch
//   k_cca_select   top-k selection, the loss value and the weights of G_M
//
// No atomics anywhere, every sum in a fixed order: the same input gives the same bits.
#include <mutex>
#include <map>
#include "common.h"

#define EIG_MAX_N 128
#define EIG_MAX_SWEEPS 30

// ------------------------------------------------------------------------------------------------------------ eigensolver
// LDS image: A[N2][N2+1], V[N2][N2+1] (N2 = n rounded up to even: an odd n gets one idle slot whose row and column are zero, so
// its pair never rotates and every 2 x 2 block is handled alike), then per pair c, s, p, q and per column the sort scratch.
static size_t eig_lds_bytes(int n) {
  const int N2 = (n + 1) & ~1, h = N2 / 2;
  return (size_t)(2 * N2 * (N2 + 1) + 2 * h + 2 * N2) * 4 + (size_t)(2 * h + 2 * N2) * 4;
}
// 16 * threads >= N2^2: the dense products of the refinement keep one n x n result in registers, 16 entries per thread
static int eig_threads(int n) { return n <= 16 ? 64 : n <= 64 ? 256 : 1024; }
#define EIG_ACC 16

struct EigLds { float *A, *V; float4* par; int N2, h, pitch; };

// Cyclic Jacobi sweeps in the parallel (round-robin) order until one whole sweep rotates nothing, or `limit` sweeps.  A pair is left
// alone when |a_pq| <= tol * sqrt(|a_pp a_qq|) or a_pq == 0.  Returns the sweeps run.  Every branch on `rot` / `any` is uniform.
__device__ __forceinline__ int eig_sweeps(const EigLds& L, float tol, int limit) {
  float* A = L.A; float* V = L.V;
  const int N2 = L.N2, h = L.h, pitch = L.pitch, tid = threadIdx.x, nt = blockDim.x;
  const int own = tid % h, grp = tid / h, groups = nt / h;     // phase 2: column pair, row group
  const int ring = N2 - 1;      // round-robin: slot N2-1 stays, the others walk round a ring of N2-1
  int sweeps = 0;
  while (sweeps < limit) {
    int any = 0;
    for (int step = 0; step < ring; ++step) {
      // phase 1: one thread per pair
      int did = 0;
      if (tid < h) {
        int p, q;
        if (tid == 0) { p = step; q = N2 - 1; }
        else { p = (step + tid) % ring; q = (step - tid + ring) % ring; }
        if (p > q) { const int t = p; p = q; q = t; }
        const float app = A[p * pitch + p], aqq = A[q * pitch + q], apq = A[p * pitch + q];
        float c = 1.f, s = 0.f;
        if (apq != 0.f && fabsf(apq) > tol * sqrtf(fabsf(app)) * sqrtf(fabsf(aqq))) {
          const float tau = (aqq - app) / (2.f * apq);
          const float t = (tau >= 0.f ? 1.f : -1.f) / (fabsf(tau) + sqrtf(1.f + tau * tau));
          if (t != 0.f) {       // t == 0: tau overflowed, the rotation is the identity to working precision
            c = 1.f / sqrtf(1.f + t * t); s = t * c; did = 1;
          }
        }
        L.par[tid] = make_float4(c, s, __int_as_float(p), __int_as_float(q));
      }
      const int rot = __syncthreads_or(did);
      if (!rot) continue;       // no pair of this step rotates
      any = 1;
      // phase 2: a thread owns one column pair Q (its c, s, p, q stay in registers) and walks over the row pairs P / the rows of V,
      // `groups` of them at a time; a wave reads P's parameters as one broadcast 16-byte load
      if (grp < groups) {
        const float4 mine = L.par[own];
        const float c2 = mine.x, s2 = mine.y;
        const int p2 = __float_as_int(mine.z), q2 = __float_as_int(mine.w);
        // A[P,Q] <- J_P^T A[P,Q] J_Q, J = [c s; -s c]
        for (int P = grp; P < h; P += groups) {
          const float4 other = L.par[P];
          const float c1 = other.x, s1 = other.y;
          if (s1 == 0.f && s2 == 0.f) continue;                // both identities: the block keeps its bits
          float* r0 = A + __float_as_int(other.z) * pitch;
          float* r1 = A + __float_as_int(other.w) * pitch;
          const float x00 = r0[p2], x01 = r0[q2], x10 = r1[p2], x11 = r1[q2];
          if (P == own) {       // the pair's own block: the off-diagonal is annihilated exactly
            const float t = s1 / c1;
            r0[p2] = x00 - t * x01; r1[q2] = x11 + t * x01; r0[q2] = 0.f; r1[p2] = 0.f;
          } else {
            const float y00 = c1 * x00 - s1 * x10, y01 = c1 * x01 - s1 * x11;
            const float y10 = s1 * x00 + c1 * x10, y11 = s1 * x01 + c1 * x11;
            r0[p2] = c2 * y00 - s2 * y01; r0[q2] = s2 * y00 + c2 * y01;
            r1[p2] = c2 * y10 - s2 * y11; r1[q2] = s2 * y10 + c2 * y11;
          }
        }
        // V[:,Q] <- V[:,Q] J_Q
        if (s2 != 0.f) {
          for (int r = grp; r < N2; r += groups) {
            float* row = V + r * pitch;
            const float vp = row[p2], vq = row[q2];
            row[p2] = c2 * vp - s2 * vq; row[q2] = s2 * vp + c2 * vq;
          }
        }
      }
      __syncthreads();
    }
    ++sweeps;
    if (!any) break;
  }
  return sweeps;
}

// acc[e] = sum_k fa(i, k) fb(k, j) in fp64 for entry idx = tid + e * threads of an N2 x N2 result, (i, j) = (idx / N2, idx % N2), or
// the other way round with `swap` (then consecutive lanes walk down a column).  The result stays in registers so that it may
// replace one of its own operands after a barrier.
template <typename FA, typename FB>
__device__ __forceinline__ void eig_prod(double (&acc)[EIG_ACC], int N2, bool swap, FA fa, FB fb) {
#pragma unroll
  for (int e = 0; e < EIG_ACC; ++e) {
    const int idx = threadIdx.x + e * blockDim.x;
    double s = 0.0;
    if (idx < N2 * N2) {
      int i = idx / N2, j = idx - i * N2;
      if (swap) { const int t = i; i = j; j = t; }
      for (int k = 0; k < N2; ++k) s = fma((double)fa(i, k), (double)fb(k, j), s);
    }
    acc[e] = s;
  }
}
template <typename FS>
__device__ __forceinline__ void eig_store(const double (&acc)[EIG_ACC], int N2, bool swap, FS fs) {
#pragma unroll
  for (int e = 0; e < EIG_ACC; ++e) {
    const int idx = threadIdx.x + e * blockDim.x;
    if (idx < N2 * N2) {
      int i = idx / N2, j = idx - i * N2;
      if (swap) { const int t = i; i = j; j = t; }
      fs(i, j, acc[e]);
    }
  }
}

// One Newton-Schulz step V <- V (3 I - V^T V) / 2 with fp64-accumulated products: a V that is orthonormal to 1e-5 (what a thousand
// fp32 rotations leave) becomes orthonormal to fp32 rounding.  Uses the A buffer for E = V^T V - I.
__device__ __forceinline__ void eig_orthonormalise(const EigLds& L) {
  float* A = L.A; float* V = L.V;
  const int N2 = L.N2, pitch = L.pitch;
  double acc[EIG_ACC];
  eig_prod(acc, N2, false, [&](int i, int k) { return V[k * pitch + i]; }, [&](int k, int j) { return V[k * pitch + j]; });
  eig_store(acc, N2, false, [&](int i, int j, double x) { A[i * pitch + j] = (float)(x - (i == j ? 1.0 : 0.0)); });
  __syncthreads();
  eig_prod(acc, N2, false, [&](int i, int k) { return V[i * pitch + k]; }, [&](int k, int j) { return A[k * pitch + j]; });
  __syncthreads();
  eig_store(acc, N2, false, [&](int i, int j, double x) { V[i * pitch + j] = (float)((double)V[i * pitch + j] - 0.5 * x); });
  __syncthreads();
}

// Matrix b of the launch has n_b = (b == 1 && n_alt > 0) ? n_alt : n columns (the two covariance matrices of the CCA loss may differ
// in width); its operands start at a + b * mat_stride, w + b * vec_stride, v + b * mat_stride.
//
// Three stages.  (1) Jacobi sweeps to the tolerance 2^-20: V diagonalises the matrix to about fp32 accuracy, but it is the
// product of ~1000 rotations per column, each rounded, and has lost orthogonality at the 1e-5 level.  (2) V is orthonormalised and
// A <- V^T A0 V is formed afresh from the input with fp64-accumulated products, which throws the accumulated rounding away.
// (3) Sweeps to the tight tolerance (2^-24) on that nearly diagonal matrix: only a few, tiny rotations.
__global__ void __launch_bounds__(1024) k_sym_eig(const float* __restrict__ a, int n_first, int n_alt, int64_t mat_stride,
                                                   int64_t vec_stride, float* __restrict__ w, float* __restrict__ v,
                                                   int32_t* __restrict__ sweeps_out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int b = blockIdx.x;
  const int n = (b == 1 && n_alt > 0) ? n_alt : n_first;
  const int N2 = (n + 1) & ~1, h = N2 / 2, pitch = N2 + 1;
  float* A = (float*)smem;
  float* V = A + N2 * pitch;
  float4* par = (float4*)(V + N2 * pitch);      // [h] per pair (c, s, p, q); 16-byte aligned: 2 N2 pitch is a multiple of 4
  float* wv = (float*)(par + h);                // [N2] eigenvalues
  float* sg = wv + N2;                          // [N2] sign of each column
  int* rank = (int*)(sg + N2);                  // [N2] position of column i in ascending order
  int* inv = rank + N2;                         // [N2] column at position j
  const EigLds L = {A, V, par, N2, h, pitch};
  const int tid = threadIdx.x, nt = blockDim.x;
  a += (int64_t)b * mat_stride; v += (int64_t)b * mat_stride; w += (int64_t)b * vec_stride;

  for (int i = tid; i < N2 * N2; i += nt) {
    const int r = i / N2, c = i - r * N2;
    A[r * pitch + c] = (r < n && c < n) ? a[(int64_t)r * n + c] : 0.f;
    V[r * pitch + c] = r == c ? 1.f : 0.f;
  }
  __syncthreads();

  int sweeps = eig_sweeps(L, 9.5367432e-7f, EIG_MAX_SWEEPS - 2);
  if (sweeps > 1) {             // (a single sweep rotated nothing: A and V are still the input and the identity, nothing to refine)
    eig_orthonormalise(L);
    double acc[EIG_ACC];
    // W = A0 V (A0 symmetric, read as A0[k][i]: consecutive lanes read consecutive addresses), then A = V^T W
    eig_prod(acc, N2, true, [&](int i, int k) { return (i < n && k < n) ? a[(int64_t)k * n + i] : 0.f; },
             [&](int k, int j) { return V[k * pitch + j]; });
    eig_store(acc, N2, true, [&](int i, int j, double x) { A[i * pitch + j] = (float)x; });
    __syncthreads();
    eig_prod(acc, N2, false, [&](int i, int k) { return V[k * pitch + i]; }, [&](int k, int j) { return A[k * pitch + j]; });
    __syncthreads();
    eig_store(acc, N2, false, [&](int i, int j, double x) { A[i * pitch + j] = (float)x; });
    __syncthreads();
  }
  const int more = eig_sweeps(L, 5.9604645e-8f, EIG_MAX_SWEEPS - sweeps);
  sweeps += more;
  for (int i = tid; i < n; i += nt) wv[i] = A[i * pitch + i];
  __syncthreads();
  if (more > 1) eig_orthonormalise(L);       // the few rotations of stage 3 are rounded too (A is scratch from here on)

  // ascending order (ties by column index), the largest-magnitude component of every vector positive (ties: lowest row)
  for (int i = tid; i < n; i += nt) {
    const float wi = wv[i];
    int r = 0;
    for (int j = 0; j < n; ++j) { const float wj = wv[j]; r += (wj < wi || (wj == wi && j < i)) ? 1 : 0; }
    rank[i] = r; inv[r] = i;
    float best = -1.f, sign = 1.f;
    for (int k = 0; k < n; ++k) {
      const float x = V[k * pitch + i];
      if (fabsf(x) > best) { best = fabsf(x); sign = x < 0.f ? -1.f : 1.f; }
    }
    sg[i] = sign;
  }
  __syncthreads();
  for (int i = tid; i < n; i += nt) w[rank[i]] = wv[i];
  for (int i = tid; i < n * n; i += nt) {
    const int r = i / n, j = i - r * n, src = inv[j];
    v[(int64_t)r * n + j] = sg[src] * V[r * pitch + src];
  }
  if (tid == 0 && sweeps_out) sweeps_out[b] = sweeps;
}

static bool eig_prepare() {     // n > 64 needs more than the default 64 KiB of dynamic LDS: opt in once per device
  static std::mutex mu;
  static std::map<int, bool> done;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  std::lock_guard<std::mutex> lock(mu);
  auto it = done.find(dev);
  if (it != done.end()) return it->second;
  // what n = 128 needs (132 KiB), not the whole 160 KiB: the kernel also has 256 B of static LDS (the workgroup-wide OR), and the
  // two together must fit
  const bool ok = hipFuncSetAttribute((const void*)k_sym_eig, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)eig_lds_bytes(EIG_MAX_N)) == hipSuccess;
  done[dev] = ok;
  return ok;
}

static int eig_launch(const float* a, int batch, int n, int n_alt, int64_t mat_stride, int64_t vec_stride, float* w, float* v,
                      int32_t* sweeps, hipStream_t s) {
  const int nmax = n_alt > n ? n_alt : n;
  const size_t lds = eig_lds_bytes(nmax);
  if (lds > 64 * 1024 && !eig_prepare()) return MD_ERR_LAUNCH;
  MD_KLAUNCH(k_sym_eig, dim3(batch), dim3(eig_threads(nmax)), lds, s, a, n, n_alt, mat_stride, vec_stride, w, v, sweeps);
  MD_CHECK_LAUNCH();
  return MD_OK;
}

extern "C" int md_sym_eig(const float* a, int32_t batch, int32_t n, float* w, float* v, int32_t* sweeps_out, void* stream) {
  if (batch < 1 || n < 1 || batch > 65535) return MD_ERR_BAD_SHAPE;
  if (n > EIG_MAX_N) return MD_ERR_UNSUPPORTED;
  if (!a || !w || !v) return MD_ERR_NULL;
  return eig_launch(a, batch, n, 0, (int64_t)n * n, n, w, v, sweeps_out, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------------------ loss pieces
// Column means in fp64 and hb = h - mean; one thread per column of [h1 | h2], rows read coalesced across the columns.
__global__ void __launch_bounds__(64) k_cca_center(const float* __restrict__ h1, const float* __restrict__ h2, int m, int o1, int o2,
                                                   float* __restrict__ hb1, float* __restrict__ hb2) {
  int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= o1 + o2) return;
  const float* src = h1; float* dst = hb1; int o = o1;
  if (c >= o1) { src = h2; dst = hb2; o = o2; c -= o1; }
  double sum = 0.0;
  for (int r = 0; r < m; ++r) sum += (double)src[(int64_t)r * o + c];
  const double mean = sum / (double)m;
  for (int r = 0; r < m; ++r) dst[(int64_t)r * o + c] = (float)((double)src[(int64_t)r * o + c] - mean);
}

// out_z[i][j] = sum_r X[r][i] Y[r][j] / (m - 1) + ridge [i == j], z = 0: (hb1, hb1), 1: (hb2, hb2), 2: (hb1, hb2).  fp64 FMAs in row
// order, so S11 and S22 are symmetric to the bit.
__global__ void __launch_bounds__(256) k_cca_cov(const float* __restrict__ hb1, const float* __restrict__ hb2, int m, int o1, int o2,
                                                 float r1, float r2, float* __restrict__ s11, float* __restrict__ s22,
                                                 float* __restrict__ s12) {
  __shared__ float Xs[16][17], Ys[16][17];
  const int z = blockIdx.z;
  const float* X = z == 1 ? hb2 : hb1;
  const float* Y = z == 0 ? hb1 : hb2;
  const int ox = z == 1 ? o2 : o1, oy = z == 0 ? o1 : o2;
  float* out = z == 0 ? s11 : z == 1 ? s22 : s12;
  const float ridge = z == 0 ? r1 : z == 1 ? r2 : 0.f;
  const int i0 = blockIdx.y * 16, j0 = blockIdx.x * 16;
  if (i0 >= ox || j0 >= oy) return;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  double acc = 0.0;
  for (int r0 = 0; r0 < m; r0 += 16) {
    const int r = r0 + ty;
    Xs[ty][tx] = (r < m && i0 + tx < ox) ? X[(int64_t)r * ox + i0 + tx] : 0.f;
    Ys[ty][tx] = (r < m && j0 + tx < oy) ? Y[(int64_t)r * oy + j0 + tx] : 0.f;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) acc = fma((double)Xs[k][ty], (double)Ys[k][tx], acc);
    __syncthreads();
  }
  const int i = i0 + ty, j = j0 + tx;
  if (i < ox && j < oy) out[(int64_t)i * oy + j] = (float)(acc / (double)(m - 1) + (i == j ? (double)ridge : 0.0));
}

// One small product C = alpha * g * X' diag(s') Y  (+ C when acc), X'(i,k) = X[i*xrs + k*xcs] or its symmetric part, Y(k,j) = Y[k*yrs + j*ycs].
//   smode 0: no scale; 1: s' = s; 2: s' = s > eps ? 1/sqrt(s) : 0 (the kept eigenvalues to the power -1/2)
//   emode 0: nothing; 1: + rho on the diagonal; 2: times K(i,j), the divided difference of f(d) = d^-1/2 on the kept eigenvalues
//   g = *alpha_dev when given (the incoming gradient stays on the device)
struct CcaGemm {
  const float* X; const float* Y; const float* s; const float* d; const float* alpha_dev; float* C;
  int xrs, xcs, yrs, ycs, ldc, M, N, K;
  float alpha, eps, rho;
  int smode, emode, xsym, acc;
};
struct CcaGemmBatch { CcaGemm j[3]; };

__device__ __forceinline__ float cca_divdiff(float di, float dj, float eps) {
  const bool ki = di > eps, kj = dj > eps;
  if (ki && kj) { const float si = sqrtf(di), sj = sqrtf(dj); return -1.f / (si * sj * (si + sj)); }
  if (ki) return (1.f / sqrtf(di)) / (di - dj);
  if (kj) return (1.f / sqrtf(dj)) / (dj - di);
  return 0.f;
}

__global__ void __launch_bounds__(256) k_cca_gemm(CcaGemmBatch b) {
  __shared__ float Xs[16][17], Ys[16][17];
  const CcaGemm& g = b.j[blockIdx.z];
  const int i0 = blockIdx.y * 16, j0 = blockIdx.x * 16;
  if (i0 >= g.M || j0 >= g.N) return;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  float acc = 0.f;
  for (int k0 = 0; k0 < g.K; k0 += 16) {
    {
      const int i = i0 + ty, k = k0 + tx;
      float x = 0.f;
      if (i < g.M && k < g.K) {
        x = g.X[(int64_t)i * g.xrs + (int64_t)k * g.xcs];
        if (g.xsym) x = 0.5f * (x + g.X[(int64_t)k * g.xrs + (int64_t)i * g.xcs]);
      }
      Xs[ty][tx] = x;
    }
    {
      const int k = k0 + ty, j = j0 + tx;
      float y = 0.f;
      if (k < g.K && j < g.N) {
        y = g.Y[(int64_t)k * g.yrs + (int64_t)j * g.ycs];
        if (g.smode == 1) y *= g.s[k];
        else if (g.smode == 2) { const float d = g.s[k]; y = d > g.eps ? y * (1.f / sqrtf(d)) : 0.f; }
      }
      Ys[ty][tx] = y;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) acc = fmaf(Xs[ty][k], Ys[k][tx], acc);
    __syncthreads();
  }
  const int i = i0 + ty, j = j0 + tx;
  if (i >= g.M || j >= g.N) return;
  float r = acc * g.alpha;
  if (g.alpha_dev) r *= g.alpha_dev[0];
  if (g.emode == 1) r += i == j ? g.rho : 0.f;
  else if (g.emode == 2) r *= cca_divdiff(g.d[i], g.d[j], g.eps);
  float* c = g.C + (int64_t)i * g.ldc + j;
  *c = g.acc ? *c + r : r;
}

static CcaGemm cca_job(const float* X, int xrs, int xcs, const float* Y, int yrs, int ycs, float* C, int M, int N, int K, float alpha = 1.f) {
  CcaGemm g = {};
  g.X = X; g.xrs = xrs; g.xcs = xcs; g.Y = Y; g.yrs = yrs; g.ycs = ycs; g.C = C; g.ldc = N; g.M = M; g.N = N; g.K = K; g.alpha = alpha;
  return g;
}
static int cca_gemm_launch(const CcaGemm* jobs, int n, hipStream_t s) {
  CcaGemmBatch b = {};
  int M = 0, N = 0;
  for (int i = 0; i < n; ++i) { b.j[i] = jobs[i]; M = jobs[i].M > M ? jobs[i].M : M; N = jobs[i].N > N ? jobs[i].N : N; }
  MD_KLAUNCH(k_cca_gemm, dim3(md_cdiv(N, 16), md_cdiv(M, 16), n), dim3(256), 0, s, b);
  MD_CHECK_LAUNCH();
  return MD_OK;
}

// lam ascending (k_sym_eig).  mode k > 0: lt = max(lam, eps), S = the k largest lt (ties: lower index first); k = 0: lt = max(lam, 0),
// S = all.  loss = -sum_S sqrt(lt) (fp64, index order); gmw[i] = 1 / (2 sqrt(lam_i)) for i in S with lam_i > eps, else 0.
__global__ void __launch_bounds__(128) k_cca_select(const float* __restrict__ lam, int o2, int k, float eps, float* __restrict__ gmw,
                                                    float* __restrict__ loss) {
  __shared__ float lt[EIG_MAX_N], term[EIG_MAX_N];
  const int i = threadIdx.x;
  float li = 0.f;
  if (i < o2) { li = lam[i]; lt[i] = k > 0 ? fmaxf(li, eps) : fmaxf(li, 0.f); }
  __syncthreads();
  if (i < o2) {
    bool sel = true;
    if (k > 0) {
      int r = 0;
      for (int j = 0; j < o2; ++j) r += (lt[j] > lt[i] || (lt[j] == lt[i] && j < i)) ? 1 : 0;
      sel = r < k;
    }
    term[i] = sel ? sqrtf(lt[i]) : 0.f;
    gmw[i] = (sel && li > eps) ? 0.5f / sqrtf(li) : 0.f;
  }
  __syncthreads();
  if (i == 0) {
    double sum = 0.0;
    for (int j = 0; j < o2; ++j) sum += (double)term[j];
    loss[0] = (float)(-sum);
  }
}

// ------------------------------------------------------------------------------------------------------------ workspace
struct CcaLayout {
  size_t hb1, hb2, S, Vv, dd, s12, A, B, P, Q, T, M, W, lam, gmw, sweeps, GM, GT, GA, GB, R, G12, X1, X2, Y1, Y2, G11, G22, total;
  size_t sq;    // stride of the paired (view 1, view 2) square buffers: max(o1, o2)^2
  int omax;
};
static CcaLayout cca_layout(int m, int o1, int o2) {
  CcaLayout L;
  const size_t om = o1 > o2 ? o1 : o2, sq = om * om, rect = (size_t)o1 * o2;
  size_t at = 0;
  auto take = [&](size_t n) { const size_t here = at; at += (n + 3) & ~(size_t)3; return here; };
  L.omax = (int)om; L.sq = sq;
  L.hb1 = take((size_t)m * o1); L.hb2 = take((size_t)m * o2);
  L.S = take(2 * sq); L.Vv = take(2 * sq); L.dd = take(2 * om);
  L.s12 = take(rect); L.A = take(sq); L.B = take(sq); L.P = take(rect); L.Q = take(rect); L.T = take(rect);
  L.M = take(sq); L.W = take(sq); L.lam = take(om); L.gmw = take(om); L.sweeps = take(4);
  L.GM = take(sq); L.GT = take(rect); L.GA = take(sq); L.GB = take(sq); L.R = take(rect); L.G12 = take(rect);
  L.X1 = take(sq); L.X2 = take(sq); L.Y1 = take(sq); L.Y2 = take(sq); L.G11 = take(sq); L.G22 = take(sq);
  L.total = at;
  return L;
}
static int cca_check(int m, int o1, int o2, int k) {
  if (m < 2 || o1 < 1 || o2 < 1) return MD_ERR_BAD_SHAPE;
  if (o1 > EIG_MAX_N || o2 > EIG_MAX_N) return MD_ERR_UNSUPPORTED;
  if (k < 0 || k > o2) return MD_ERR_BAD_SHAPE;
  return MD_OK;
}

extern "C" size_t md_cca_workspace_floats(int32_t m, int32_t o1, int32_t o2) {
  if (cca_check(m, o1, o2, 0) != MD_OK) return 0;
  return cca_layout(m, o1, o2).total;
}

extern "C" int64_t md_cca_workspace_offset(int32_t m, int32_t o1, int32_t o2, int32_t which) {
  if (cca_check(m, o1, o2, 0) != MD_OK) return -1;
  const CcaLayout L = cca_layout(m, o1, o2);
  switch (which) {
    case 0: return (int64_t)L.lam;
    case 1: return (int64_t)L.sweeps;
    case 2: return (int64_t)L.T;
    case 3: return (int64_t)L.dd;
    case 4: return (int64_t)(L.dd + L.omax);
    default: return -1;
  }
}

#define CCA_TRY(expr) do { const int rc__ = (expr); if (rc__ != MD_OK) return rc__; } while (0)

extern "C" int md_cca_loss_fwd(const float* h1, const float* h2, int32_t m, int32_t o1, int32_t o2, int32_t k, float r1, float r2,
                               float eps, float* workspace, float* loss, void* stream) {
  CCA_TRY(cca_check(m, o1, o2, k));
  if (!h1 || !h2 || !workspace || !loss) return MD_ERR_NULL;
  hipStream_t s = (hipStream_t)stream;
  const CcaLayout L = cca_layout(m, o1, o2);
  float* ws = workspace;
  float *hb1 = ws + L.hb1, *hb2 = ws + L.hb2, *S11 = ws + L.S, *S22 = S11 + L.sq, *V1 = ws + L.Vv, *V2 = V1 + L.sq;
  float *d1 = ws + L.dd, *d2 = d1 + L.omax, *S12 = ws + L.s12, *A = ws + L.A, *B = ws + L.B, *P = ws + L.P, *Q = ws + L.Q;
  float *T = ws + L.T, *M = ws + L.M, *W = ws + L.W, *lam = ws + L.lam, *gmw = ws + L.gmw;
  int32_t* sweeps = (int32_t*)(ws + L.sweeps);

  MD_KLAUNCH(k_cca_center, dim3(md_cdiv(o1 + o2, 64)), dim3(64), 0, s, h1, h2, m, o1, o2, hb1, hb2);
  MD_CHECK_LAUNCH();
  MD_KLAUNCH(k_cca_cov, dim3(md_cdiv(L.omax, 16), md_cdiv(L.omax, 16), 3), dim3(256), 0, s, (const float*)hb1, (const float*)hb2, m, o1,
             o2, r1, r2, S11, S22, S12);
  MD_CHECK_LAUNCH();
  CCA_TRY(eig_launch(S11, 2, o1, o2, (int64_t)L.sq, L.omax, d1, V1, sweeps, s));
  CcaGemm j[3];
  j[0] = cca_job(V1, o1, 1, V1, 1, o1, A, o1, o1, o1); j[0].s = d1; j[0].smode = 2; j[0].eps = eps;     // A = V1 D1^-1/2 V1^T
  j[1] = cca_job(V2, o2, 1, V2, 1, o2, B, o2, o2, o2); j[1].s = d2; j[1].smode = 2; j[1].eps = eps;
  CCA_TRY(cca_gemm_launch(j, 2, s));
  j[0] = cca_job(A, o1, 1, S12, o2, 1, P, o1, o2, o1);                                                  // P = A S12
  j[1] = cca_job(S12, o2, 1, B, o2, 1, Q, o1, o2, o2);                                                  // Q = S12 B
  CCA_TRY(cca_gemm_launch(j, 2, s));
  j[0] = cca_job(P, o2, 1, B, o2, 1, T, o1, o2, o2);                                                    // T = A S12 B
  CCA_TRY(cca_gemm_launch(j, 1, s));
  j[0] = cca_job(T, 1, o2, T, o2, 1, M, o2, o2, o1); j[0].emode = 1; j[0].rho = k > 0 ? r1 : 0.f;       // M = T^T T + rho I
  CCA_TRY(cca_gemm_launch(j, 1, s));
  CCA_TRY(eig_launch(M, 1, o2, 0, (int64_t)L.sq, L.omax, lam, W, sweeps + 2, s));
  MD_KLAUNCH(k_cca_select, dim3(1), dim3(128), 0, s, (const float*)lam, o2, k, eps, gmw, loss);
  MD_CHECK_LAUNCH();
  return MD_OK;
}

extern "C" int md_cca_loss_bwd(const float* grad_out, int32_t m, int32_t o1, int32_t o2, int32_t k, float eps, float* workspace,
                               float* dh1, float* dh2, void* stream) {
  CCA_TRY(cca_check(m, o1, o2, k));
  if (!grad_out || !workspace || !dh1 || !dh2) return MD_ERR_NULL;
  hipStream_t s = (hipStream_t)stream;
  const CcaLayout L = cca_layout(m, o1, o2);
  float* ws = workspace;
  float *hb1 = ws + L.hb1, *hb2 = ws + L.hb2, *V1 = ws + L.Vv, *V2 = V1 + L.sq, *d1 = ws + L.dd, *d2 = d1 + L.omax;
  float *A = ws + L.A, *B = ws + L.B, *P = ws + L.P, *Q = ws + L.Q, *T = ws + L.T, *W = ws + L.W, *gmw = ws + L.gmw;
  float *GM = ws + L.GM, *GT = ws + L.GT, *GA = ws + L.GA, *GB = ws + L.GB, *R = ws + L.R, *G12 = ws + L.G12;
  float *X1 = ws + L.X1, *X2 = ws + L.X2, *Y1 = ws + L.Y1, *Y2 = ws + L.Y2, *G11 = ws + L.G11, *G22 = ws + L.G22;
  CcaGemm j[3];
  j[0] = cca_job(W, o2, 1, W, 1, o2, GM, o2, o2, o2); j[0].s = gmw; j[0].smode = 1;                     // G_M = W diag(gmw) W^T
  CCA_TRY(cca_gemm_launch(j, 1, s));
  j[0] = cca_job(T, o2, 1, GM, o2, 1, GT, o1, o2, o2, 2.f);                                             // G_T = 2 T G_M
  CCA_TRY(cca_gemm_launch(j, 1, s));
  j[0] = cca_job(GT, o2, 1, Q, 1, o2, GA, o1, o1, o2);                                                  // G_A = G_T (S12 B)^T
  j[1] = cca_job(P, 1, o2, GT, o2, 1, GB, o2, o2, o1);                                                  // G_B = (A S12)^T G_T
  j[2] = cca_job(A, o1, 1, GT, o2, 1, R, o1, o2, o1);                                                   // R = A G_T
  CCA_TRY(cca_gemm_launch(j, 3, s));
  j[0] = cca_job(R, o2, 1, B, o2, 1, G12, o1, o2, o2);                                                  // G_S12 = A G_T B
  j[1] = cca_job(GA, o1, 1, V1, o1, 1, X1, o1, o1, o1); j[1].xsym = 1;                                  // X = sym(G_A) V
  j[2] = cca_job(GB, o2, 1, V2, o2, 1, X2, o2, o2, o2); j[2].xsym = 1;
  CCA_TRY(cca_gemm_launch(j, 3, s));
  j[0] = cca_job(V1, 1, o1, X1, o1, 1, Y1, o1, o1, o1); j[0].emode = 2; j[0].d = d1; j[0].eps = eps;    // Y = K o (V^T X)
  j[1] = cca_job(V2, 1, o2, X2, o2, 1, Y2, o2, o2, o2); j[1].emode = 2; j[1].d = d2; j[1].eps = eps;
  CCA_TRY(cca_gemm_launch(j, 2, s));
  j[0] = cca_job(V1, o1, 1, Y1, o1, 1, X1, o1, o1, o1);                                                 // Z = V Y (over X)
  j[1] = cca_job(V2, o2, 1, Y2, o2, 1, X2, o2, o2, o2);
  CCA_TRY(cca_gemm_launch(j, 2, s));
  j[0] = cca_job(X1, o1, 1, V1, 1, o1, G11, o1, o1, o1);                                                // G_S11 = Z V^T
  j[1] = cca_job(X2, o2, 1, V2, 1, o2, G22, o2, o2, o2);
  CCA_TRY(cca_gemm_launch(j, 2, s));
  const float a = -1.f / (float)(m - 1);
  j[0] = cca_job(hb1, o1, 1, G11, 1, o1, dh1, m, o1, o1, 2.f * a); j[0].alpha_dev = grad_out;           // dh1 = -g (2 Hb1 G11^T + Hb2 G12^T) / (m-1)
  j[1] = cca_job(hb2, o2, 1, G22, 1, o2, dh2, m, o2, o2, 2.f * a); j[1].alpha_dev = grad_out;
  CCA_TRY(cca_gemm_launch(j, 2, s));
  j[0] = cca_job(hb2, o2, 1, G12, 1, o2, dh1, m, o1, o2, a); j[0].alpha_dev = grad_out; j[0].acc = 1;
  j[1] = cca_job(hb1, o1, 1, G12, o2, 1, dh2, m, o2, o1, a); j[1].alpha_dev = grad_out; j[1].acc = 1;   // dh2 = -g (2 Hb2 G22^T + Hb1 G12) / (m-1)
  CCA_TRY(cca_gemm_launch(j, 2, s));
  return MD_OK;
}
