// Eval-mode backward pieces (BatchNorm with running statistics): what a `score.backward()` through a trained model needs below
// the head.  With the folded per-channel constants of md_bn_eval_params a unit is a = leaky(scale * y + shift), so
//   d_raw = dA * leaky'(scale * y + shift) * scale
// with no statistics, no reduction and no finalize.  All kernels here are streaming HBM-bound passes over channels-last fp32
// tensors [rows][Cp]: a thread owns one 16-byte channel chunk (its constants stay in registers) and walks rows, four rows in
// flight per trip; the grid is sized from the CU count.  Also here: the data gradient of the R(2+1)D stem's 1x7x7 / stride-2
// convolution (3 input channels; training never needs it) and the saliency map of an input gradient.
#include "common.h"

#include <math.h>

namespace {

struct EView { const float* p; const float* scale; const float* shift; float slope; };
inline EView to_eview(const MdActView* v) {
  EView o; o.p = v ? v->data : nullptr; o.scale = v ? v->scale : nullptr; o.shift = v ? v->shift : nullptr;
  o.slope = v ? v->slope : 1.f; return o;
}

// per-channel constants of one 4-channel chunk; pad channels get scale 0 and `live` 0
struct EConst { float sc[4], sh[4], live[4]; };
__device__ __forceinline__ EConst load_ec(const EView& v, int c4, int C) {
  EConst k;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int c = c4 * 4 + e;
    k.live[e] = c < C ? 1.f : 0.f;
    k.sc[e] = v.scale ? (c < C ? v.scale[c] : 0.f) : 1.f;
    k.sh[e] = v.scale ? (c < C ? v.shift[c] : 0.f) : 0.f;
  }
  return k;
}
// dA * leaky'(p) * scale with p = fmaf(scale, y, shift) exactly as the forward kernels evaluate it (bn_elem.hip::pre_of)
__device__ __forceinline__ float eval_d1(float d, float y, float sc, float sh, float slope, bool has_bn) {
  if (!has_bn) return d;
  return d * md_dleaky(fmaf(y, sc, sh), slope) * sc;
}

int cu_count() {
  static int n = 0;
  if (!n) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) {
      (void)hipGetLastError(); v = 256;
    }
    n = v;
  }
  return n;
}
// workgroups of a streaming pass: enough to give every CU eight, never more than there are 8-row trips
int pass_blocks(int64_t rows, int C4) {
  const int nr = 256 / C4;
  int64_t b = md_cdiv64(rows, (int64_t)nr * 8);
  const int64_t cap = (int64_t)cu_count() * 8;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}

struct Walk { int c4, r, nr; int64_t beg, end; bool active; };
__device__ __forceinline__ Walk walk_of(int64_t rows, int C4) {
  Walk w;
  w.nr = blockDim.x / C4; w.c4 = threadIdx.x % C4; w.r = threadIdx.x / C4; w.active = w.r < w.nr;
  const int64_t per = (rows + gridDim.x - 1) / gridDim.x;
  w.beg = (int64_t)blockIdx.x * per;
  w.end = w.beg + per < rows ? w.beg + per : rows;
  return w;
}

__global__ __launch_bounds__(256) void k_bn_eval_bwd(const float* dA, EView y, int64_t rows, int C, int C4,
                                                     float* d_raw) {   // (d_raw may be dA: no __restrict__)
  const Walk w = walk_of(rows, C4);
  if (!w.active) return;
  const EConst k = load_ec(y, w.c4, C);
  const bool bn = y.scale != nullptr;
  auto one = [&](size_t o, float4 d, float4 v) {
    float4 r;
    r.x = eval_d1(d.x, v.x, k.sc[0], k.sh[0], y.slope, bn);
    // pad channels (never the first of a chunk) are written as +0 whatever dA holds there
    r.y = k.live[1] != 0.f ? eval_d1(d.y, v.y, k.sc[1], k.sh[1], y.slope, bn) : 0.f;
    r.z = k.live[2] != 0.f ? eval_d1(d.z, v.z, k.sc[2], k.sh[2], y.slope, bn) : 0.f;
    r.w = k.live[3] != 0.f ? eval_d1(d.w, v.w, k.sc[3], k.sh[3], y.slope, bn) : 0.f;
    *(float4*)(d_raw + o) = r;
  };
  int64_t row = w.beg + w.r;
  for (; row + 3 * (int64_t)w.nr < w.end; row += 4 * (int64_t)w.nr) {
    size_t o[4]; float4 d[4], v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      o[u] = ((size_t)(row + u * (int64_t)w.nr) * C4 + w.c4) * 4;
      d[u] = *(const float4*)(dA + o[u]);
      v[u] = *(const float4*)(y.p + o[u]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) one(o[u], d[u], v[u]);
  }
  for (; row < w.end; row += w.nr) {
    const size_t o = ((size_t)row * C4 + w.c4) * 4;
    one(o, *(const float4*)(dA + o), *(const float4*)(y.p + o));
  }
}

// Block close z = leaky(a_skip + a_main, alpha): d = dZ * (z > 0 ? 1 : alpha) (the sign of the sum is the sign of z);
// d_main_raw = d * leaky'(p_main) * scale_main; dS = d for a plain skip, d * leaky'(p_skip) * scale_skip for a unit's view.
__global__ __launch_bounds__(256) void k_residual_eval_bwd(const float* dZ, const float* __restrict__ z, EView mainv,
                                                           EView skipv, int has_skip_view, float alpha, int64_t rows, int C, int C4,
                                                           float* d_main, float* dS, int accumulate) {   // (dS may be dZ)
  const Walk w = walk_of(rows, C4);
  if (!w.active) return;
  const EConst km = load_ec(mainv, w.c4, C);
  EConst ks = km;
  const bool sbn = has_skip_view && skipv.scale != nullptr;
  if (sbn) ks = load_ec(skipv, w.c4, C);
  const bool mbn = mainv.scale != nullptr;
  for (int64_t row = w.beg + w.r; row < w.end; row += w.nr) {
    const size_t o = ((size_t)row * C4 + w.c4) * 4;
    const float4 g4 = *(const float4*)(dZ + o), z4 = *(const float4*)(z + o), m4 = *(const float4*)(mainv.p + o);
    float4 s4 = make_float4(0.f, 0.f, 0.f, 0.f), a4 = s4;
    if (sbn) s4 = *(const float4*)(skipv.p + o);
    if (accumulate) a4 = *(const float4*)(dS + o);
    const float g[4] = {g4.x, g4.y, g4.z, g4.w}, zz[4] = {z4.x, z4.y, z4.z, z4.w}, m[4] = {m4.x, m4.y, m4.z, m4.w};
    const float sv[4] = {s4.x, s4.y, s4.z, s4.w}, acc[4] = {a4.x, a4.y, a4.z, a4.w};
    float rm[4], rs[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float d = g[e] * md_dleaky(zz[e], alpha);
      rm[e] = km.live[e] != 0.f ? eval_d1(d, m[e], km.sc[e], km.sh[e], mainv.slope, mbn) : 0.f;
      const float s = km.live[e] != 0.f ? eval_d1(d, sv[e], ks.sc[e], ks.sh[e], skipv.slope, sbn) : 0.f;
      rs[e] = accumulate ? acc[e] + s : s;
    }
    *(float4*)(d_main + o) = make_float4(rm[0], rm[1], rm[2], rm[3]);
    *(float4*)(dS + o) = make_float4(rs[0], rs[1], rs[2], rs[3]);
  }
}

// ------------------------------------------------------------------------------------------------------------------------------
// Data gradient of a 1 x kh x kw convolution with few input channels (the stem: 3 channels, 7 x 7, stride 2, 45 output channels) in
// gather form: one thread per input pixel, dx[n,t,y,x,ci] = sum over taps (ky,kx) with (y + ph - ky) % sh == 0 etc. and over co of
// dY[n,t,oy,ox,co] * w[co,ci,0,ky,kx].  The weights sit in LDS as [ky][kx][co][4] (ci padded to 4), dY is read in 16-byte chunks;
// exact fp32 FMA in a fixed order.  A quarter of the taps is live per pixel at stride 2.
// (Measured slower, 10.4 against 5.2 ms for the whole input gradient at the bench shape: a workgroup per stride class of pixels, so
// that the tap loop is uniform over a wave, two pixels per thread.)
// ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_stem_dgrad(const float* __restrict__ dy, const float* __restrict__ w, MdConvDesc d, int Cpo,
                                                    int64_t npix, float* __restrict__ dx) {
  extern __shared__ float4 wl[];      // [kh*kw][Cpo] of float4 (ci = 0..3)
  const int taps = d.kh * d.kw;
  for (int e = threadIdx.x; e < taps * Cpo; e += blockDim.x) {
    const int tap = e / Cpo, co = e - tap * Cpo;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (co < d.Cout)
      for (int ci = 0; ci < d.Cin; ++ci) v[ci] = w[((size_t)co * d.Cin + ci) * taps + tap];
    wl[e] = make_float4(v[0], v[1], v[2], v[3]);
  }
  __syncthreads();
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= npix) return;
  const int x = (int)(idx % d.Wi); int64_t r = idx / d.Wi;
  const int y = (int)(r % d.Hi); r /= d.Hi;           // r = n * Ti + t  (kt = 1, st = 1, pt = 0: To == Ti)
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int ky = 0; ky < d.kh; ++ky) {
    const int ny = y + d.ph - ky;
    if (ny < 0 || ny % d.sh) continue;
    const int oy = ny / d.sh;
    if (oy >= d.Ho) continue;
    for (int kx = 0; kx < d.kw; ++kx) {
      const int nx = x + d.pw - kx;
      if (nx < 0 || nx % d.sw) continue;
      const int ox = nx / d.sw;
      if (ox >= d.Wo) continue;
      const float4* g = (const float4*)(dy + (((size_t)r * d.Ho + oy) * d.Wo + ox) * Cpo);
      const float4* wt = wl + (size_t)(ky * d.kw + kx) * Cpo;
      for (int c4 = 0; c4 < Cpo / 4; ++c4) {
        const float4 gv = g[c4];
        const float gg[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float4 ww = wt[c4 * 4 + e];
          a.x = fmaf(gg[e], ww.x, a.x); a.y = fmaf(gg[e], ww.y, a.y); a.z = fmaf(gg[e], ww.z, a.z); a.w = fmaf(gg[e], ww.w, a.w);
        }
      }
    }
  }
  *(float4*)(dx + (size_t)idx * 4) = a;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Saliency map of an input gradient (B,3,T,H,W) -> (B,T,H,W): max | sum over channels of |dx|, then per-clip min-max.
// Launch 1: SAL_SLICES workgroups per clip write the reduced values and one (min, max) pair each; launch 2: every workgroup
// combines its clip's pairs (min / max do not depend on the order) and normalises its slice.  No atomics.
// ------------------------------------------------------------------------------------------------------------------------------
constexpr int SAL_SLICES = 64;

__device__ __forceinline__ float wmin(float v) { for (int o = 32; o; o >>= 1) v = fminf(v, __shfl_xor(v, o)); return v; }
__device__ __forceinline__ float wmax(float v) { for (int o = 32; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o)); return v; }

__global__ __launch_bounds__(256) void k_saliency_reduce(const float* __restrict__ dx, int C, int64_t thw, int mode,
                                                         float* __restrict__ maps, float* __restrict__ mm) {
  __shared__ float smn[4], smx[4];
  const int b = blockIdx.y, sl = blockIdx.x;
  const int64_t per = (thw + SAL_SLICES - 1) / SAL_SLICES;
  const int64_t beg = (int64_t)sl * per, end = beg + per < thw ? beg + per : thw;
  const float* xb = dx + (size_t)b * C * thw;
  float mn = INFINITY, mx = -INFINITY;
  for (int64_t p = beg + threadIdx.x; p < end; p += blockDim.x) {
    float v = 0.f;
    for (int c = 0; c < C; ++c) {
      const float a = fabsf(xb[(size_t)c * thw + p]);
      v = mode == 0 ? fmaxf(v, a) : v + a;
    }
    maps[(size_t)b * thw + p] = v;
    mn = fminf(mn, v); mx = fmaxf(mx, v);
  }
  mn = wmin(mn); mx = wmax(mx);
  if ((threadIdx.x & 63) == 0) { smn[threadIdx.x >> 6] = mn; smx[threadIdx.x >> 6] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    mm[((size_t)b * SAL_SLICES + sl) * 2] = fminf(fminf(smn[0], smn[1]), fminf(smn[2], smn[3]));
    mm[((size_t)b * SAL_SLICES + sl) * 2 + 1] = fmaxf(fmaxf(smx[0], smx[1]), fmaxf(smx[2], smx[3]));
  }
}

__global__ __launch_bounds__(256) void k_saliency_norm(const float* __restrict__ mm, int64_t thw, float* __restrict__ maps) {
  const int b = blockIdx.y, sl = blockIdx.x;
  float mn = INFINITY, mx = -INFINITY;
  for (int i = 0; i < SAL_SLICES; ++i) {
    mn = fminf(mn, mm[((size_t)b * SAL_SLICES + i) * 2]); mx = fmaxf(mx, mm[((size_t)b * SAL_SLICES + i) * 2 + 1]);
  }
  const float den = mx - mn;
  const int64_t per = (thw + SAL_SLICES - 1) / SAL_SLICES;
  const int64_t beg = (int64_t)sl * per, end = beg + per < thw ? beg + per : thw;
  for (int64_t p = beg + threadIdx.x; p < end; p += blockDim.x) {
    const size_t o = (size_t)b * thw + p;
    maps[o] = den > 0.f ? (maps[o] - mn) / den : 0.f;
  }
}

}  // namespace

static int check_rows_c(int64_t rows, int32_t C) {
  if (rows <= 0 || C <= 0) return MD_ERR_BAD_SHAPE;
  if (md_cpad(C) / 4 > 256) return MD_ERR_UNSUPPORTED;
  return MD_OK;
}

extern "C" int md_bn_eval_bwd(const float* dA, const MdActView* y_view, int64_t rows, int32_t C, float* d_raw, void* stream) {
  if (!dA || !y_view || !y_view->data || !d_raw) return MD_ERR_NULL;
  if ((y_view->scale == nullptr) != (y_view->shift == nullptr)) return MD_ERR_NULL;
  int rc = check_rows_c(rows, C); if (rc) return rc;
  const int C4 = md_cpad(C) / 4;
  MD_KLAUNCH(k_bn_eval_bwd, dim3(pass_blocks(rows, C4)), dim3(256), 0, (hipStream_t)stream, dA, to_eview(y_view), rows, C, C4, d_raw);
  MD_CHECK_LAUNCH();
  return MD_OK;
}

extern "C" int md_residual_eval_bwd(const float* dZ, const float* z, const MdActView* main_view, const MdActView* skip_view, float alpha,
                                    int64_t rows, int32_t C, float* d_main_raw, float* dS, int accumulate_dS, void* stream) {
  if (!dZ || !z || !main_view || !main_view->data || !d_main_raw || !dS) return MD_ERR_NULL;
  if ((main_view->scale == nullptr) != (main_view->shift == nullptr)) return MD_ERR_NULL;
  if (skip_view && (!skip_view->data || (skip_view->scale == nullptr) != (skip_view->shift == nullptr))) return MD_ERR_NULL;
  if (d_main_raw == dS) return MD_ERR_UNSUPPORTED;
  int rc = check_rows_c(rows, C); if (rc) return rc;
  const int C4 = md_cpad(C) / 4;
  MD_KLAUNCH(k_residual_eval_bwd, dim3(pass_blocks(rows, C4)), dim3(256), 0, (hipStream_t)stream, dZ, z, to_eview(main_view),
             to_eview(skip_view), skip_view ? 1 : 0, alpha, rows, C, C4, d_main_raw, dS, accumulate_dS ? 1 : 0);
  MD_CHECK_LAUNCH();
  return MD_OK;
}

extern "C" int md_stem_dgrad_supported(const MdConvDesc* d) {
  if (!d) return 0;
  if (d->kt != 1 || d->st != 1 || d->pt != 0 || d->To != d->Ti) return 0;
  if (d->Cin < 1 || d->Cin > 4 || d->Cout < 1 || d->kh < 1 || d->kw < 1 || d->sh < 1 || d->sw < 1) return 0;
  if (d->Ho != (d->Hi + 2 * d->ph - d->kh) / d->sh + 1 || d->Wo != (d->Wi + 2 * d->pw - d->kw) / d->sw + 1) return 0;
  if (d->Ho <= 0 || d->Wo <= 0 || d->N <= 0) return 0;
  return (size_t)d->kh * d->kw * md_cpad(d->Cout) * 16 <= 65536 ? 1 : 0;
}

extern "C" int md_stem_dgrad(const MdConvDesc* d, const float* dy_raw, const float* w, float* dx, void* stream) {
  if (!d || !dy_raw || !w || !dx) return MD_ERR_NULL;
  if (!md_stem_dgrad_supported(d)) return MD_ERR_UNSUPPORTED;
  const int Cpo = md_cpad(d->Cout);
  const int64_t npix = (int64_t)d->N * d->Ti * d->Hi * d->Wi;
  if (md_cdiv64(npix, 256) > 0x7fffffff) return MD_ERR_UNSUPPORTED;
  const size_t lds = (size_t)d->kh * d->kw * Cpo * 16;
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)k_stem_dgrad, hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
    attr_set = true;
  }
  MD_KLAUNCH(k_stem_dgrad, dim3((unsigned)md_cdiv64(npix, 256)), dim3(256), lds, (hipStream_t)stream, dy_raw, w, *d, Cpo, npix, dx);
  MD_CHECK_LAUNCH();
  return MD_OK;
}

extern "C" size_t md_saliency_scratch_floats(int32_t B) { return B > 0 ? (size_t)B * SAL_SLICES * 2 : 0; }

extern "C" int md_saliency_map(const float* dx, int32_t B, int32_t C, int32_t T, int32_t H, int32_t W, int32_t mode, float* maps,
                               float* scratch, void* stream) {
  if (!dx || !maps || !scratch) return MD_ERR_NULL;
  if (B <= 0 || C <= 0 || T <= 0 || H <= 0 || W <= 0 || B > 65535 || (mode != 0 && mode != 1)) return MD_ERR_BAD_SHAPE;
  const int64_t thw = (int64_t)T * H * W;
  hipStream_t s = (hipStream_t)stream;
  MD_KLAUNCH(k_saliency_reduce, dim3(SAL_SLICES, B), dim3(256), 0, s, dx, C, thw, mode, maps, scratch);
  MD_CHECK_LAUNCH();
  MD_KLAUNCH(k_saliency_norm, dim3(SAL_SLICES, B), dim3(256), 0, s, (const float*)scratch, thw, maps);
  MD_CHECK_LAUNCH();
  return MD_OK;
}
