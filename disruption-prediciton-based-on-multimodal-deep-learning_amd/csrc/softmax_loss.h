// Per-sample arithmetic of the fused softmax + Focal / LDAM / CE loss, shared by k_softmax_loss (head_loss.hip) and
// k_eval_accumulate (importance.hip) so that both evaluate one batch to the same floats.
// kind 0 focal : term = w[y] (1-p)^gamma ce                                (src/loss.py:25-34)
// kind 1 LDAM  : z = s*(x - m[y] onehot); term = w[y] nll                  (src/loss.py:58-69; the caller divides by sum w)
// kind 2 CE    : term = w[y] nll                                           (src/loss.py:80-81)
// arg = argmax_k softmax(x) on the UNMODIFIED logits, first maximal index (src/train.py:70).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#define MD_LOSS_MAXK 16

struct MdSampleLoss {
  float lse;    // log-sum-exp of the (margin-shifted, scaled) logits z
  float w;      // class weight of the target
  float term;   // this sample's contribution to the loss sum
  float coef;   // d term / d ce
  int arg;
};

// x: one row of K <= MD_LOSS_MAXK logits; z receives the logits the cross entropy is taken of; 0 <= yy < K.
__device__ __forceinline__ MdSampleLoss md_sample_loss(int kind, const float* __restrict__ x, int yy, int K,
                                                       const float* __restrict__ cw, const float* __restrict__ margins,
                                                       float gs, float* z) {
  MdSampleLoss r;
  float mx = -INFINITY; int arg = 0; float rawmx = -INFINITY;
  for (int k = 0; k < K; ++k) {
    float v = x[k];
    if (v > rawmx) { rawmx = v; arg = k; }
    if (kind == 1) { if (k == yy && margins) v -= margins[k]; v *= gs; }
    z[k] = v; mx = fmaxf(mx, v);
  }
  r.arg = arg;
  float se = 0.f;
  for (int k = 0; k < K; ++k) se += expf(z[k] - mx);
  const float lse = mx + logf(se);
  const float ce = lse - z[yy];
  const float w = cw ? cw[yy] : 1.f;
  if (kind == 0) {
    const float p = expf(-ce);
    const float q = 1.f - p;
    const float qg = powf(q, gs);
    r.term = w * qg * ce;
    float dq = 0.f;
    if (gs != 0.f && q > 0.f) dq = gs * powf(q, gs - 1.f) * p * ce;
    r.coef = w * (qg + dq);
  } else {
    r.term = w * ce;
    r.coef = w;
  }
  r.lse = lse; r.w = w;
  return r;
}
