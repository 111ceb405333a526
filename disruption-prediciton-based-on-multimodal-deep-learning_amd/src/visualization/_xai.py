"""Thin launchers of the explainability kernels (include/mi355x_disrupt.h, csrc/xai.hip).  Every tensor lives on the GPU; every
output is allocated here and returned."""
from __future__ import annotations

import torch

from .. import _native as N
from .. import ops
from ..ops import _p, _stream

FUSION = {"mean": 0, "max": 1, "min": 2}


def head_eval_dfeat(feat: torch.Tensor, lin0, bn, lin1, alpha: float, target) -> torch.Tensor:
    """d logit[b, target[b]] / d feat[b] of Linear -> BatchNorm1d (running statistics) -> ELU(alpha) | LeakyReLU(-alpha) -> Linear
    (md_head_eval_dfeat).  target: an int (every clip) or a (B,) integer tensor."""
    feat = ops.f32(feat).contiguous()
    B, D = feat.shape
    K = lin1.out_features
    if isinstance(target, torch.Tensor):
        tgt = target.to(device=feat.device, dtype=torch.int64).reshape(-1).contiguous()
        if tgt.numel() != B:
            raise ValueError("target: %d entries for %d clips" % (tgt.numel(), B))
    else:
        if not 0 <= int(target) < K:
            raise ValueError("target %d outside [0, %d)" % (int(target), K))
        tgt = torch.full((B,), int(target), dtype=torch.int64, device=feat.device)
    ws = [lin0.weight, lin0.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, lin1.weight]
    ops.require_cuda(feat, *ws)
    dfeat = torch.empty_like(feat)
    N.check(N.lib().md_head_eval_dfeat(_p(feat), B, D, lin0.out_features, K, *[_p(w) for w in ws[:6]], float(bn.eps), float(alpha),
                                       _p(lin1.weight), _p(tgt), _p(dfeat), _stream()), "md_head_eval_dfeat")
    return dfeat


def gradcam(act: torch.Tensor, C: int, Tq: int, h: int, w: int, dfeat: torch.Tensor, OH: int, OW: int):
    """act [B*Tq*h*w, Cpad] channels-last, dfeat (B, C) -> (cam_raw (B, Tq, h, w), map (B, OH, OW)) (md_gradcam)."""
    B = dfeat.shape[0]
    ops.require_cuda(act, dfeat)
    if act.shape[0] != B * Tq * h * w:
        raise ValueError("activation rows %d != B*T'*h*w = %d" % (act.shape[0], B * Tq * h * w))
    cam_raw = torch.empty((B, Tq, h, w), device=act.device)
    out = torch.empty((B, OH, OW), device=act.device)
    N.check(N.lib().md_gradcam(_p(act), Tq * h * w, C, act.shape[1], Tq, h, w, _p(ops.f32(dfeat).contiguous()), B, OH, OW, _p(cam_raw),
                               _p(out), _stream()), "md_gradcam")
    return cam_raw, out


def head_eval_bwd(feat: torch.Tensor, lin0, bn, lin1, alpha: float, dlogits: torch.Tensor) -> torch.Tensor:
    """Eval-mode input gradient of the head for an arbitrary dlogits (B, K) (md_head_eval_bwd)."""
    feat = ops.f32(feat).contiguous()
    dlogits = ops.f32(dlogits).contiguous()
    B, D = feat.shape
    ws = [lin0.weight, lin0.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, lin1.weight]
    ops.require_cuda(feat, dlogits, *ws)
    if tuple(dlogits.shape) != (B, lin1.out_features):
        raise ValueError("dlogits %s for logits (%d, %d)" % (tuple(dlogits.shape), B, lin1.out_features))
    dfeat = torch.empty_like(feat)
    N.check(N.lib().md_head_eval_bwd(_p(dlogits), _p(feat), B, D, lin0.out_features, lin1.out_features, *[_p(w) for w in ws[:6]],
                                     float(bn.eps), float(alpha), _p(lin1.weight), _p(dfeat), _stream()), "md_head_eval_bwd")
    return dfeat


def gradcam_grad(act: torch.Tensor, dact: torch.Tensor, C: int, B: int, Tq: int, h: int, w: int, OH: int, OW: int):
    """act, dact [B*Tq*h*w, cpad(C)] channels-last -> (weights (B, C), cam_raw (B, Tq, h, w), map (B, OH, OW)) (md_gradcam_grad)."""
    ops.require_cuda(act, dact)
    rows = B * Tq * h * w
    if act.shape[0] != rows or tuple(dact.shape) != tuple(act.shape) or act.shape[1] != ops.cpad(C):
        raise ValueError("activation %s / gradient %s for B*T'*h*w = %d rows of %d channels" % (tuple(act.shape), tuple(dact.shape), rows, C))
    L = N.lib()
    wts = torch.empty((B, C), device=act.device)
    cam_raw = torch.empty((B, Tq, h, w), device=act.device)
    out = torch.empty((B, OH, OW), device=act.device)
    scratch = torch.empty(L.md_gradcam_grad_scratch_floats(B, C), device=act.device)
    N.check(L.md_gradcam_grad(_p(ops.f32(act)), _p(ops.f32(dact)), B, Tq, h, w, C, OH, OW, _p(wts), _p(cam_raw), _p(out), _p(scratch),
                              _stream()), "md_gradcam_grad")
    return wts, cam_raw, out


SALIENCY_MODE = {"max": 0, "sum": 1}


def saliency_map(dx: torch.Tensor, mode: str = "max") -> torch.Tensor:
    """dx (B, C, T, H, W) -> (B, T, H, W) in [0, 1]: max | sum over channels of |dx|, per-clip min-max (md_saliency_map)."""
    if mode not in SALIENCY_MODE:
        raise ValueError("mode must be one of %s, got %r" % (sorted(SALIENCY_MODE), mode))
    dx = ops.f32(dx).contiguous()
    ops.require_cuda(dx)
    B, Cc, T, H, W = dx.shape
    L = N.lib()
    maps = torch.empty((B, T, H, W), device=dx.device)
    scratch = torch.empty(L.md_saliency_scratch_floats(B), device=dx.device)
    N.check(L.md_saliency_map(_p(dx), B, Cc, T, H, W, SALIENCY_MODE[mode], _p(maps), _p(scratch), _stream()), "md_saliency_map")
    return maps


def attention_probs_fused(qkv: torch.Tensor, heads: int, fusion: str, batch_first: bool = True, out=None) -> torch.Tensor:
    """(B, S, S) head-fused softmax(q k^T / sqrt(d_head)) of a qkv projection (md_attention_probs_fused)."""
    if fusion not in FUSION:
        raise ValueError("head_fusion must be one of %s, got %r" % (sorted(FUSION), fusion))
    qkv = ops.f32(qkv).contiguous()
    ops.require_cuda(qkv)
    B, S, D3 = qkv.shape if batch_first else (qkv.shape[1], qkv.shape[0], qkv.shape[2])
    if out is None:
        out = torch.empty((B, S, S), device=qkv.device)
    N.check(N.lib().md_attention_probs_fused(_p(qkv), S, B, D3 // 3, int(heads), int(bool(batch_first)), FUSION[fusion], _p(out),
                                             _stream()), "md_attention_probs_fused")
    return out


def rollout_discard(fused: torch.Tensor, n_seq_per_clip: int, k: int) -> torch.Tensor:
    """fused (..., S, S) whose leading axes flatten to clips of n_seq_per_clip sequences -> the discarded copy (md_rollout_discard)."""
    fused = ops.f32(fused).contiguous()
    ops.require_cuda(fused)
    S = fused.shape[-1]
    nseq = fused.numel() // (S * S)
    out = torch.empty_like(fused)
    N.check(N.lib().md_rollout_discard(_p(fused), int(n_seq_per_clip), nseq // int(n_seq_per_clip), S, int(k), _p(out), _stream()),
            "md_rollout_discard")
    return out


def rollout_chain(fused_layers: torch.Tensor) -> torch.Tensor:
    """(L, n_seq, S, S) -> prod_l (A_l + I) / 2, newest layer on the left (md_rollout_chain)."""
    fused_layers = ops.f32(fused_layers).contiguous()
    ops.require_cuda(fused_layers)
    L, nseq, S, _ = fused_layers.shape
    result = torch.empty((nseq, S, S), device=fused_layers.device)
    N.check(N.lib().md_rollout_chain(_p(fused_layers), L, nseq, S, _p(result), _stream()), "md_rollout_chain")
    return result


def rollout_mask(result: torch.Tensor, n_clips: int, kind: int) -> torch.Tensor:
    """kind 0: (B, n_seq_per_clip, S-1) = result[:, 0, 1:]; kind 1: (B, n_seq_per_clip, S-1, S-1) = result[:, 1:, 1:]; each clip
    divided by its maximum (md_rollout_mask)."""
    result = ops.f32(result).contiguous()
    ops.require_cuda(result)
    nseq, S, _ = result.shape
    nspc = nseq // int(n_clips)
    shape = (n_clips, nspc, S - 1) if kind == 0 else (n_clips, nspc, S - 1, S - 1)
    out = torch.empty(shape, device=result.device)
    N.check(N.lib().md_rollout_mask(_p(result), int(n_clips), nspc, S, int(kind), _p(out), _stream()), "md_rollout_mask")
    return out
