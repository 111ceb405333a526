// Explainability maps (reference src/visualization/visualize_cam.py:57-132 and visualize_attention.py:28-135) for models trained
// with this library: the eval-mode input gradient of the classifier head, the Grad-CAM map read straight from the trunk executor's
// last materialised activation, the head-fused attention probabilities of ViViT, and the three stages of attention rollout
// (discard, the (A+I)/2 chain product, the normalised mask).  fp32 FMA throughout (the attention scores summed in fp64), batched over
// clips; stores are vector stores.
#include "common.h"

#include <math.h>

static __device__ __forceinline__ float wave_sum(float v) {
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
static __device__ __forceinline__ float wave_max(float v) {
  for (int o = 32; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
static __device__ __forceinline__ float wave_min(float v) {
  for (int o = 32; o; o >>= 1) v = fminf(v, __shfl_xor(v, o));
  return v;
}

// ------------------------------------------------------------------------------------------------------------------------------
// (a) d logit[b, target[b]] / d feat[b, :] through Linear -> BatchNorm1d (running statistics) -> ELU(alpha) | LeakyReLU(-alpha)
//     -> Linear.  One workgroup per clip: g[j] = W1[t, j] * act'(y_j) * gamma_j / sqrt(rv_j + eps), dfeat = W0^T g.
// ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_head_eval_dfeat(const float* __restrict__ feat, int D, int Hd, int K,
                                                         const float* __restrict__ w0, const float* __restrict__ b0,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         const float* __restrict__ rmean, const float* __restrict__ rvar, float eps,
                                                         float alpha, const float* __restrict__ w1, const int64_t* __restrict__ target,
                                                         const float* __restrict__ dlogits, float* __restrict__ dfeat) {
  extern __shared__ float sm[];
  float* fs = sm;        // [D]
  float* g = sm + D;     // [Hd]
  const int b = blockIdx.x, t = threadIdx.x, nt = blockDim.x;
  // target != nullptr: the one-hot gradient of md_head_eval_dfeat; otherwise an arbitrary dlogits row (md_head_eval_bwd)
  const int64_t tg = target ? target[b] : 0;
  const bool ok = tg >= 0 && tg < K;
  for (int d = t; d < D; d += nt) fs[d] = feat[(size_t)b * D + d];
  __syncthreads();
  for (int j = t; j < Hd; j += nt) {
    float a = b0[j];
    for (int d = 0; d < D; ++d) a = fmaf(fs[d], w0[(size_t)j * D + d], a);
    const float is = 1.f / sqrtf(rvar[j] + eps);
    const float y = (a - rmean[j]) * is * gamma[j] + beta[j];
    const float da = y > 0.f ? 1.f : (alpha >= 0.f ? alpha * expf(y) : -alpha);     // ELU'(y) | LeakyReLU'(y), as md_head_fwd
    float up;
    if (target) {
      up = ok ? w1[(size_t)tg * Hd + j] : __builtin_nanf("");
    } else {
      up = 0.f;
      for (int k = 0; k < K; ++k) up = fmaf(dlogits[(size_t)b * K + k], w1[(size_t)k * Hd + j], up);
    }
    g[j] = up * da * gamma[j] * is;
  }
  __syncthreads();
  for (int d = t; d < D; d += nt) {
    float a = 0.f;
    for (int j = 0; j < Hd; ++j) a = fmaf(w0[(size_t)j * D + d], g[j], a);
    dfeat[(size_t)b * D + d] = a;
  }
}

extern "C" int md_head_eval_dfeat(const float* feat, int32_t B, int32_t D, int32_t Hd, int32_t K, const float* w0, const float* b0,
                                  const float* gamma, const float* beta, const float* rmean, const float* rvar, float eps,
                                  float elu_alpha, const float* w1, const int64_t* target, float* dfeat, void* stream) {
  if (!feat || !w0 || !b0 || !gamma || !beta || !rmean || !rvar || !w1 || !target || !dfeat) return MD_ERR_NULL;
  if (B <= 0 || D <= 0 || Hd <= 0 || K <= 0 || !(eps >= 0.f)) return MD_ERR_BAD_SHAPE;
  const size_t lds = (size_t)(D + Hd) * 4;
  if (lds > 65536) return MD_ERR_UNSUPPORTED;
  MD_KLAUNCH(k_head_eval_dfeat, dim3(B), dim3(256), lds, (hipStream_t)stream, feat, D, Hd, K, w0, b0, gamma, beta, rmean, rvar, eps,
             elu_alpha, w1, target, (const float*)nullptr, dfeat);
  MD_CHECK_LAUNCH();
  return MD_OK;
}

extern "C" int md_head_eval_bwd(const float* dlogits, const float* feat, int32_t B, int32_t D, int32_t Hd, int32_t K, const float* w0,
                                const float* b0, const float* gamma, const float* beta, const float* rmean, const float* rvar, float eps,
                                float elu_alpha, const float* w1, float* dfeat, void* stream) {
  if (!dlogits || !feat || !w0 || !b0 || !gamma || !beta || !rmean || !rvar || !w1 || !dfeat) return MD_ERR_NULL;
  if (B <= 0 || D <= 0 || Hd <= 0 || K <= 0 || !(eps >= 0.f)) return MD_ERR_BAD_SHAPE;
  const size_t lds = (size_t)(D + Hd) * 4;
  if (lds > 65536) return MD_ERR_UNSUPPORTED;
  MD_KLAUNCH(k_head_eval_dfeat, dim3(B), dim3(256), lds, (hipStream_t)stream, feat, D, Hd, K, w0, b0, gamma, beta, rmean, rvar, eps,
             elu_alpha, w1, (const int64_t*)nullptr, dlogits, dfeat);
  MD_CHECK_LAUNCH();
  return MD_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// (b) Grad-CAM.  Launch 1: one wave per activation row, cam_raw[row] = ReLU(sum_c dfeat[b,c] / thw * act[row, c]).
//     Launch 2: one workgroup per clip, every frame resized bilinearly (align_corners=False, F.interpolate's source index),
//     the mean over frames, then min-max normalisation (a constant map becomes zeros).
// ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gradcam_raw(const float* __restrict__ act, int64_t rows, int rpc, int C, int Cp,
                                                     const float* __restrict__ dfeat, float thw, float* __restrict__ cam_raw) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int64_t b = r / rpc;
  const float* a = act + r * Cp;
  const float* w = dfeat + b * C;
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s = fmaf(w[c] / thw, a[c], s);
  s = wave_sum(s);
  if (lane == 0) cam_raw[r] = fmaxf(s, 0.f);
}

static __device__ __forceinline__ float gradcam_sample(const float* cs, int Tq, int h, int w, int OW, float sh, float sw, int p) {
  const int oy = p / OW, ox = p - oy * OW;
  const float sy = fmaxf(sh * (oy + 0.5f) - 0.5f, 0.f), sx = fmaxf(sw * (ox + 0.5f) - 0.5f, 0.f);
  const int y0 = (int)sy, x0 = (int)sx;
  const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
  const float ly = sy - y0, lx = sx - x0, hy = 1.f - ly, hx = 1.f - lx;
  float acc = 0.f;
  for (int t = 0; t < Tq; ++t) {
    const float* f = cs + t * h * w;
    acc += hy * (hx * f[y0 * w + x0] + lx * f[y0 * w + x1]) + ly * (hx * f[y1 * w + x0] + lx * f[y1 * w + x1]);
  }
  return acc / (float)Tq;
}

__global__ __launch_bounds__(512) void k_gradcam_map(const float* __restrict__ cam_raw, int Tq, int h, int w, int OH, int OW, float sh,
                                                     float sw, int use_lds, float* __restrict__ out) {
  extern __shared__ float cs_lds[];     // [Tq][h][w] of this clip (use_lds), else the clip is sampled from memory
  __shared__ float wmn[8], wmx[8];
  const int b = blockIdx.x, t = threadIdx.x, nt = blockDim.x, nw = nt >> 6;
  const int n = Tq * h * w, np = OH * OW;
  const float* cs = cam_raw + (size_t)b * n;
  if (use_lds) {
    for (int e = t; e < n; e += nt) cs_lds[e] = cam_raw[(size_t)b * n + e];
    __syncthreads();
    cs = cs_lds;
  }
  float mn = INFINITY, mx = -INFINITY;
  for (int p = t; p < np; p += nt) {
    const float v = gradcam_sample(cs, Tq, h, w, OW, sh, sw, p);
    mn = fminf(mn, v); mx = fmaxf(mx, v);
  }
  mn = wave_min(mn); mx = wave_max(mx);
  if ((t & 63) == 0) { wmn[t >> 6] = mn; wmx[t >> 6] = mx; }
  __syncthreads();
  mn = wmn[0]; mx = wmx[0];
  for (int i = 1; i < nw; ++i) { mn = fminf(mn, wmn[i]); mx = fmaxf(mx, wmx[i]); }
  const float den = mx - mn;
  float* o = out + (size_t)b * np;
  for (int p = t; p < np; p += nt) {
    const float v = gradcam_sample(cs, Tq, h, w, OW, sh, sw, p);
    o[p] = den > 0.f ? (v - mn) / den : 0.f;
  }
}

extern "C" int md_gradcam(const float* act, int32_t act_rows_per_clip, int32_t C, int32_t Cpad, int32_t Tq, int32_t h, int32_t w,
                          const float* dfeat, int32_t B, int32_t OH, int32_t OW, float* cam_raw, float* out, void* stream) {
  if (!act || !dfeat || !cam_raw || !out) return MD_ERR_NULL;
  if (B <= 0 || C <= 0 || Cpad < C || Tq <= 0 || h <= 0 || w <= 0 || OH <= 0 || OW <= 0) return MD_ERR_BAD_SHAPE;
  if ((int64_t)Tq * h * w != act_rows_per_clip) return MD_ERR_BAD_SHAPE;
  if ((int64_t)OH * OW > (1LL << 30)) return MD_ERR_BAD_SHAPE;
  const size_t lds = (size_t)act_rows_per_clip * 4;
  if (lds > 65536) return MD_ERR_UNSUPPORTED;
  const int64_t rows = (int64_t)B * act_rows_per_clip;
  hipStream_t s = (hipStream_t)stream;
  MD_KLAUNCH(k_gradcam_raw, dim3((unsigned)md_cdiv64(rows, 4)), dim3(256), 0, s, act, rows, act_rows_per_clip, C, Cpad, dfeat,
             (float)act_rows_per_clip, cam_raw);
  MD_CHECK_LAUNCH();
  MD_KLAUNCH(k_gradcam_map, dim3(B), dim3(512), lds, s, (const float*)cam_raw, Tq, h, w, OH, OW, (float)h / (float)OH,
             (float)w / (float)OW, 1, out);
  MD_CHECK_LAUNCH();
  return MD_OK;
}

// Grad-CAM at a layer where the gradient is not uniform (visualize_cam.py:87-103 as written: alpha = mean over (T', h, w) of the
// gradient).  Launch 1: GC_SLICES workgroups per clip sum their rows of dact per channel; launch 2: one workgroup per clip adds the
// slices in ascending order and divides by T'*h*w; then k_gradcam_raw (with thw = 1: the weights are means already) and
// k_gradcam_map exactly as md_gradcam.  A layer whose (T', h, w) does not fit the LDS is sampled from memory instead.
constexpr int GC_SLICES = 32;

__global__ __launch_bounds__(256) void k_gradcam_wsum(const float* __restrict__ dact, int64_t rpc, int C4, float* __restrict__ part) {
  __shared__ float4 red[256];
  const int b = blockIdx.y, sl = blockIdx.x;
  const int nr = blockDim.x / C4, c4 = threadIdx.x % C4, r = threadIdx.x / C4;
  const int64_t per = (rpc + GC_SLICES - 1) / GC_SLICES;
  const int64_t beg = (int64_t)sl * per, end = beg + per < rpc ? beg + per : rpc;
  const float* xb = dact + (size_t)b * rpc * C4 * 4;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  if (r < nr)
    for (int64_t row = beg + r; row < end; row += nr) {
      const float4 v = *(const float4*)(xb + ((size_t)row * C4 + c4) * 4);
      a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
  red[threadIdx.x] = a;
  __syncthreads();
  if (r == 0) {
    float4 s = red[c4];
    for (int q = 1; q < nr; ++q) { const float4 v = red[q * C4 + c4]; s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w; }
    *(float4*)(part + (((size_t)b * GC_SLICES + sl) * C4 + c4) * 4) = s;
  }
}
__global__ __launch_bounds__(256) void k_gradcam_wfin(const float* __restrict__ part, int C, int Cp, float thw, float* __restrict__ wts) {
  const int b = blockIdx.x;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float s = 0.f;
    for (int i = 0; i < GC_SLICES; ++i) s += part[((size_t)b * GC_SLICES + i) * Cp + c];
    wts[(size_t)b * C + c] = s / thw;
  }
}

extern "C" size_t md_gradcam_grad_scratch_floats(int32_t B, int32_t C) {
  return (B > 0 && C > 0) ? (size_t)B * GC_SLICES * md_cpad(C) : 0;
}

extern "C" int md_gradcam_grad(const float* act, const float* dact, int32_t B, int32_t Tq, int32_t h, int32_t w, int32_t C, int32_t OH,
                               int32_t OW, float* weights, float* cam_raw, float* out, float* scratch, void* stream) {
  if (!act || !dact || !weights || !cam_raw || !out || !scratch) return MD_ERR_NULL;
  if (B <= 0 || B > 65535 || C <= 0 || Tq <= 0 || h <= 0 || w <= 0 || OH <= 0 || OW <= 0) return MD_ERR_BAD_SHAPE;
  const int Cp = md_cpad(C), C4 = Cp / 4;
  if (C4 > 256) return MD_ERR_UNSUPPORTED;
  const int64_t rpc = (int64_t)Tq * h * w;
  if (rpc > 0x7fffffff || (int64_t)OH * OW > (1LL << 30)) return MD_ERR_BAD_SHAPE;
  const int64_t rows = (int64_t)B * rpc;
  hipStream_t s = (hipStream_t)stream;
  MD_KLAUNCH(k_gradcam_wsum, dim3(GC_SLICES, B), dim3(256), 0, s, dact, rpc, C4, scratch);
  MD_CHECK_LAUNCH();
  MD_KLAUNCH(k_gradcam_wfin, dim3(B), dim3(256), 0, s, (const float*)scratch, C, Cp, (float)rpc, weights);
  MD_CHECK_LAUNCH();
  MD_KLAUNCH(k_gradcam_raw, dim3((unsigned)md_cdiv64(rows, 4)), dim3(256), 0, s, act, rows, (int)rpc, C, Cp, (const float*)weights, 1.f,
             cam_raw);
  MD_CHECK_LAUNCH();
  const int use_lds = (size_t)rpc * 4 <= 65536 ? 1 : 0;
  MD_KLAUNCH(k_gradcam_map, dim3(B), dim3(512), use_lds ? (size_t)rpc * 4 : 0, s, (const float*)cam_raw, Tq, h, w, OH, OW,
             (float)h / (float)OH, (float)w / (float)OW, use_lds, out);
  MD_CHECK_LAUNCH();
  return MD_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// (c) out[b] = fuse_h softmax(q_h k_h^T * dh^-0.5), fuse = mean | max | min.  A workgroup takes XR query rows of one sequence and
//     walks the heads: the rows' q in LDS, one key per thread, the scores of the XR rows in LDS, a softmax per row by one wave, the
//     fused value kept in LDS.  The per-head matrices never reach memory.  The fp32 products are accumulated and scaled in fp64
//     (half-rate FMA on CDNA4), so a probability carries only the rounding of expf and of the normalisation, not that of a
//     32-bit score (which alone reaches 1e-6 on a sharp softmax): the discard step downstream is discontinuous.
// ------------------------------------------------------------------------------------------------------------------------------
constexpr int XR = 8;

__global__ __launch_bounds__(256) void k_attn_probs_fused(const float* __restrict__ qkv, int S, int B, int D, int H, int bf, int fusion,
                                                          double scale, float* __restrict__ out) {
  extern __shared__ float sm[];
  const int dh = D / H;
  float* qs = sm;                           // [XR][dh]
  double* sc = (double*)(qs + XR * dh);     // [XR][S]  (XR * dh * 4 bytes: a multiple of 8)
  float* fu = (float*)(sc + XR * S);        // [XR][S]
  const int nblk = (S + XR - 1) / XR;
  const int b = blockIdx.x / nblk, i0 = (blockIdx.x - b * nblk) * XR;
  const int t = threadIdx.x, nt = blockDim.x, lane = t & 63, wv = t >> 6, nw = nt >> 6;
  const size_t D3 = (size_t)3 * D;
  auto row = [&](int s) -> const float* { return qkv + (bf ? ((size_t)b * S + s) : ((size_t)s * B + b)) * D3; };
  for (int hh = 0; hh < H; ++hh) {
    for (int e = t; e < XR * dh; e += nt) {
      const int r = e / dh, d = e - r * dh;
      qs[e] = i0 + r < S ? row(i0 + r)[hh * dh + d] : 0.f;
    }
    __syncthreads();
    for (int j = t; j < S; j += nt) {
      const f32x4* kp = (const f32x4*)(row(j) + D + hh * dh);
      double acc[XR];
#pragma unroll
      for (int r = 0; r < XR; ++r) acc[r] = 0.0;
      for (int d4 = 0; d4 < dh / 4; ++d4) {
        const f32x4 kv = kp[d4];
#pragma unroll
        for (int r = 0; r < XR; ++r) {
          const f32x4 qv = *(const f32x4*)(qs + r * dh + 4 * d4);
          acc[r] = fma((double)qv.x, (double)kv.x, acc[r]); acc[r] = fma((double)qv.y, (double)kv.y, acc[r]);
          acc[r] = fma((double)qv.z, (double)kv.z, acc[r]); acc[r] = fma((double)qv.w, (double)kv.w, acc[r]);
        }
      }
#pragma unroll
      for (int r = 0; r < XR; ++r) sc[r * S + j] = acc[r] * scale;
    }
    __syncthreads();
    for (int r = wv; r < XR; r += nw) {
      const double* sr = sc + r * S; float* fr = fu + r * S;
      double m = -INFINITY;
      for (int j = lane; j < S; j += 64) m = fmax(m, sr[j]);
      for (int o = 32; o; o >>= 1) m = fmax(m, __shfl_xor(m, o));
      double z = 0.0;
      for (int j = lane; j < S; j += 64) z += (double)expf((float)(sr[j] - m));
      for (int o = 32; o; o >>= 1) z += __shfl_xor(z, o);
      for (int j = lane; j < S; j += 64) {
        const float p = (float)((double)expf((float)(sr[j] - m)) / z);
        fr[j] = hh == 0 ? p : (fusion == 0 ? fr[j] + p : (fusion == 1 ? fmaxf(fr[j], p) : fminf(fr[j], p)));
      }
    }
    __syncthreads();
  }
  for (int e = t; e < XR * S; e += nt) {
    const int r = e / S, j = e - r * S;
    if (i0 + r < S) out[((size_t)b * S + i0 + r) * S + j] = fusion == 0 ? fu[e] / (float)H : fu[e];
  }
}

extern "C" int md_attention_probs_fused(const float* qkv, int32_t S, int32_t B, int32_t D, int32_t H, int32_t batch_first,
                                        int32_t fusion, float* out, void* stream) {
  if (!qkv || !out) return MD_ERR_NULL;
  if (S <= 0 || B <= 0 || D <= 0 || H <= 0 || D % H != 0) return MD_ERR_BAD_SHAPE;
  if (fusion < 0 || fusion > 2 || (batch_first != 0 && batch_first != 1)) return MD_ERR_BAD_SHAPE;
  const int dh = D / H;
  if (dh % 4 != 0 || ((uintptr_t)qkv & 15) != 0) return MD_ERR_UNSUPPORTED;
  const size_t lds = (size_t)XR * dh * 4 + (size_t)XR * S * 12;
  if (lds > 65536) return MD_ERR_UNSUPPORTED;
  const int64_t grid = (int64_t)B * md_cdiv(S, XR);
  if (grid > 0x7fffffff) return MD_ERR_UNSUPPORTED;
  MD_KLAUNCH(k_attn_probs_fused, dim3((unsigned)grid), dim3(256), lds, (hipStream_t)stream, qkv, S, B, D, H, batch_first, fusion,
             pow((double)dh, -0.5), out);
  MD_CHECK_LAUNCH();
  return MD_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// (d) Discard (visualize_attention.py:86-90, :122-126).  fused_out = fused; then for every sequence the k smallest entries of its
//     flattened S x S map are found (radix select, 8 bits a pass, over order-preserving keys of the fp32 bit patterns; histograms in
//     LDS) and written as zeros into the FIRST sequence of its clip, flat index 0 excepted.  Exactly k entries are taken per
//     sequence: every entry below the k-th smallest value, then the entries equal to it in ascending flat index order.
// ------------------------------------------------------------------------------------------------------------------------------
static __device__ __forceinline__ uint32_t order_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(1024) void k_rollout_discard(const float* __restrict__ fused, int nspc, int64_t n, int k,
                                                          float* __restrict__ fused_out) {
  __shared__ uint32_t hist[256];
  __shared__ uint32_t s_prefix, s_krem;
  __shared__ uint32_t wtot[16];
  const int seq = blockIdx.x, t = threadIdx.x, nt = blockDim.x, lane = t & 63, wv = t >> 6, nw = nt >> 6;
  const float* src = fused + (size_t)seq * n;
  float* dst = fused_out + (size_t)(seq / nspc) * nspc * n;
  uint32_t prefix = 0, mask = 0, krem = (uint32_t)k;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    for (int i = t; i < 256; i += nt) hist[i] = 0u;
    __syncthreads();
    for (int64_t e = t; e < n; e += nt) {
      const uint32_t key = order_key(src[e]);
      if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (t == 0) {
      uint32_t c = 0; int bin = 0;
      for (; bin < 255; ++bin) {
        if (c + hist[bin] >= krem) break;
        c += hist[bin];
      }
      s_prefix = prefix | ((uint32_t)bin << shift);
      s_krem = krem - c;
    }
    __syncthreads();
    prefix = s_prefix; krem = s_krem; mask |= 0xFFu << shift;
    __syncthreads();
  }
  // prefix: key of the k-th smallest entry; krem (>= 1): how many entries equal to it are taken
  uint32_t taken = 0;
  for (int64_t base = 0; base < n; base += nt) {
    const int64_t e = base + t;
    const uint32_t key = e < n ? order_key(src[e]) : 0xFFFFFFFFu;
    const bool lt = e < n && key < prefix, eq = e < n && key == prefix;
    const uint64_t bal = __ballot(eq);
    const uint32_t rank = (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wtot[wv] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t before = taken, tot = taken;
    for (int i = 0; i < nw; ++i) { tot += wtot[i]; if (i < wv) before += wtot[i]; }
    if ((lt || (eq && before + rank < krem)) && e != 0) dst[e] = 0.f;
    taken = tot;
    __syncthreads();
  }
}

extern "C" int md_rollout_discard(const float* fused, int32_t n_seq_per_clip, int32_t B_clips, int32_t S, int32_t k, float* fused_out,
                                  void* stream) {
  if (!fused || !fused_out) return MD_ERR_NULL;
  if (n_seq_per_clip <= 0 || B_clips <= 0 || S <= 0) return MD_ERR_BAD_SHAPE;
  const int64_t n = (int64_t)S * S;
  if (k < 0 || k > n || n > 0x7fffffff) return MD_ERR_BAD_SHAPE;
  const int64_t nseq = (int64_t)n_seq_per_clip * B_clips;
  if (nseq > 0x7fffffff) return MD_ERR_BAD_SHAPE;
  const size_t bytes = (size_t)nseq * n * 4;
  // the selection reads `fused` while zeros land in `fused_out`: the two must not overlap
  const uintptr_t a = (uintptr_t)fused, o = (uintptr_t)fused_out;
  if (a < o + bytes && o < a + bytes) return MD_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemcpyAsync(fused_out, fused, bytes, hipMemcpyDeviceToDevice, s) != hipSuccess) return MD_ERR_LAUNCH;
  if (k == 0) return MD_OK;
  MD_KLAUNCH(k_rollout_discard, dim3((unsigned)nseq), dim3(1024), 0, s, fused, n_seq_per_clip, n, k, fused_out);
  MD_CHECK_LAUNCH();
  return MD_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// (e) result = (A_{L-1}+I)/2 ... (A_0+I)/2 per sequence (torch.bmm(a, result), newest layer on the left).  Rows are independent
//     when the chain is taken from the left: a workgroup holds CR rows of the partial product in LDS, starting from the newest
//     layer's rows, and multiplies them by each older layer in turn, (A+I)/2 formed as it is read.  Exact fp32 FMA.
// ------------------------------------------------------------------------------------------------------------------------------
constexpr int CR = 8;

__global__ __launch_bounds__(256) void k_rollout_chain(const float* __restrict__ fused, int L, int nseq, int S, float* __restrict__ result) {
  extern __shared__ float sm[];
  const int Sp = (S + 3) & ~3;
  float* V = sm;                  // [CR][Sp], zero beyond S
  float* W = sm + CR * Sp;
  const int nblk = (S + CR - 1) / CR;
  const int seq = blockIdx.x / nblk, i0 = (blockIdx.x - seq * nblk) * CR;
  const int t = threadIdx.x, nt = blockDim.x;
  const size_t SS = (size_t)S * S;
  {
    const float* a = fused + ((size_t)(L - 1) * nseq + seq) * SS;
    for (int e = t; e < CR * Sp; e += nt) {
      const int r = e / Sp, j = e - r * Sp, i = i0 + r;
      V[e] = 0.f;
      W[e] = 0.f;
      if (i < S && j < S) V[e] = 0.5f * (a[(size_t)i * S + j] + (i == j ? 1.f : 0.f));
    }
  }
  __syncthreads();
  for (int l = L - 2; l >= 0; --l) {
    const float* a = fused + ((size_t)l * nseq + seq) * SS;
    for (int j = t; j < S; j += nt) {
      float acc[CR];
#pragma unroll
      for (int r = 0; r < CR; ++r) acc[r] = 0.f;
      for (int m = 0; m < Sp; m += 4) {
        float am[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) am[q] = m + q < S ? 0.5f * (a[(size_t)(m + q) * S + j] + (m + q == j ? 1.f : 0.f)) : 0.f;
#pragma unroll
        for (int r = 0; r < CR; ++r) {
          const f32x4 v = *(const f32x4*)(V + r * Sp + m);
          acc[r] = fmaf(v.x, am[0], acc[r]); acc[r] = fmaf(v.y, am[1], acc[r]);
          acc[r] = fmaf(v.z, am[2], acc[r]); acc[r] = fmaf(v.w, am[3], acc[r]);
        }
      }
#pragma unroll
      for (int r = 0; r < CR; ++r) W[r * Sp + j] = acc[r];
    }
    __syncthreads();
    float* tmp = V; V = W; W = tmp;
  }
  for (int e = t; e < CR * S; e += nt) {
    const int r = e / S, j = e - r * S;
    if (i0 + r < S) result[((size_t)seq * S + i0 + r) * S + j] = V[r * Sp + j];
  }
}

extern "C" int md_rollout_chain(const float* fused_layers, int32_t L, int32_t n_seq, int32_t S, float* result, void* stream) {
  if (!fused_layers || !result) return MD_ERR_NULL;
  if (L <= 0 || n_seq <= 0 || S <= 0) return MD_ERR_BAD_SHAPE;
  const size_t lds = (size_t)2 * CR * ((S + 3) & ~3) * 4;
  if (lds > 65536) return MD_ERR_UNSUPPORTED;
  const int64_t grid = (int64_t)n_seq * md_cdiv(S, CR);
  if (grid > 0x7fffffff) return MD_ERR_UNSUPPORTED;
  MD_KLAUNCH(k_rollout_chain, dim3((unsigned)grid), dim3(256), lds, (hipStream_t)stream, fused_layers, L, n_seq, S, result);
  MD_CHECK_LAUNCH();
  return MD_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// (f) Masks divided by the per-clip maximum.  kind 0 (space, :92-96): out[c][s][p] = result[c*nspc+s][0][1+p];
//     kind 1 (temporal, :128-131): out[c][s][i][j] = result[c*nspc+s][1+i][1+j].  One workgroup per clip.
// ------------------------------------------------------------------------------------------------------------------------------
static __device__ __forceinline__ float mask_value(const float* res, int c, int nspc, int S, int kind, int64_t e) {
  const int64_t S1 = S - 1;
  if (kind == 0) {
    const int64_t s = e / S1, p = e - s * S1;
    return res[(((int64_t)c * nspc + s) * S) * S + 1 + p];
  }
  const int64_t s = e / (S1 * S1), rem = e - s * S1 * S1, i = rem / S1, j = rem - i * S1;
  return res[(((int64_t)c * nspc + s) * S + 1 + i) * S + 1 + j];
}

__global__ __launch_bounds__(256) void k_rollout_mask(const float* __restrict__ result, int nspc, int S, int kind, int64_t n,
                                                      float* __restrict__ out) {
  __shared__ float wmx[4];
  const int c = blockIdx.x, t = threadIdx.x, nt = blockDim.x;
  float mx = -INFINITY;
  for (int64_t e = t; e < n; e += nt) mx = fmaxf(mx, mask_value(result, c, nspc, S, kind, e));
  mx = wave_max(mx);
  if ((t & 63) == 0) wmx[t >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(wmx[0], wmx[1]), fmaxf(wmx[2], wmx[3]));
  for (int64_t e = t; e < n; e += nt) out[(size_t)c * n + e] = mask_value(result, c, nspc, S, kind, e) / mx;
}

extern "C" int md_rollout_mask(const float* result, int32_t B_clips, int32_t n_seq_per_clip, int32_t S, int32_t kind, float* out,
                               void* stream) {
  if (!result || !out) return MD_ERR_NULL;
  if (B_clips <= 0 || n_seq_per_clip <= 0 || S < 2 || (kind != 0 && kind != 1)) return MD_ERR_BAD_SHAPE;
  const int64_t n = kind == 0 ? (int64_t)n_seq_per_clip * (S - 1) : (int64_t)n_seq_per_clip * (S - 1) * (S - 1);
  MD_KLAUNCH(k_rollout_mask, dim3(B_clips), dim3(256), 0, (hipStream_t)stream, result, n_seq_per_clip, S, kind, n, out);
  MD_CHECK_LAUNCH();
  return MD_OK;
}
