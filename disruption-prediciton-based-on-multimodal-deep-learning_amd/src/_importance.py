"""Device-side engine of the permutation feature importance (tensor level, no pandas): one resident table of rows x signals, one
list of window starts, P permutations of the row numbers and a (variant, column) -> permutation map.  Per chunk of whole loader
batches: ONE ``md_window_gather`` builds the windows of every variant (no permuted table is ever materialised), ONE eval-mode
forward runs all V*n windows (evaluation BatchNorm uses running statistics and NoiseLayer is the identity, so windows do not
interact -- src/utils/prob_curve.py relies on the same fact), ONE ``md_eval_accumulate`` turns the logits into the per-batch loss
values, the confusion counts and (optionally) softmax column 0.  Nothing is read back before the end.

The numbers are the reference's (src/feature_importance.py:29-71): ``loss`` of a variant is ``total_loss += loss.item()`` over the
loader's batches -- fp32 batch values added in Python doubles, batch sums for Focal / CE and the weighted batch mean for LDAM, so the
loader's batch size is part of the definition -- and the score is the macro-F1 of ``argmax softmax`` over all samples.
"""
from __future__ import annotations

import os
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import ops
from .utils.graphed import graphed_forward
from .utils.metrics import macro_f1

_GRAPH = os.environ.get("MD_GRAPH_STEP") == "1"


def loss_spec(loss_fn, device):
    """(kind, class weights, margins, gamma or s) of a Focal / LDAM / CE loss module, by its ``model_type`` attribute."""
    kind = getattr(loss_fn, "model_type", None)

    def dev(t):
        return None if t is None else torch.as_tensor(t).to(device=device, dtype=torch.float32).contiguous()

    if kind == "Focal":
        return "focal", dev(loss_fn.weight), None, float(loss_fn.gamma)
    if kind == "LDAM":
        return "ldam", dev(loss_fn.weight), dev(getattr(loss_fn, "m_list", None)), float(loss_fn.s)
    if kind == "CE":
        return "ce", dev(loss_fn.weight), None, 0.0
    raise RuntimeError("permutation_sweep: the loss must be a FocalLoss, LDAMLoss or CELoss (model_type attribute), got %r"
                       % type(loss_fn).__name__)


def _blend_parts(loss_fn):
    """GradientBlending: [(loss module, weight)] in the order (fused, video, 0D) of the model's outputs, and the scale."""
    return ([(loss_fn.loss_vis_ts, loss_fn.vis_ts_weight), (loss_fn.loss_vis, loss_fn.vis_weight), (loss_fn.loss_ts, loss_fn.ts_weight)],
            loss_fn.loss_scale)


def blend(l_fused, l_vis, l_ts, loss_fn) -> float:
    """GradientBlending.forward on three fp32 batch losses, in its order of operations (fp32, as the tensors are)."""
    f = np.float32
    sc = f(loss_fn.loss_scale)
    return float(f(f(f(f(l_vis) * sc) * f(loss_fn.vis_weight)) + f(f(f(l_ts) * sc) * f(loss_fn.ts_weight)))
                 + f(f(f(l_fused) * sc) * f(loss_fn.vis_ts_weight)))


def check_geometry(n_rows: int, starts: np.ndarray, seq_len: int, tau: int, perms: Optional[np.ndarray], colperm: np.ndarray,
                   n_cols: int) -> None:
    """Host-side refusal of everything md_window_gather would have to read outside the table."""
    if seq_len <= 0 or tau <= 0:
        raise ValueError("permutation_sweep: seq_len and tau must be positive")
    if starts.ndim != 1 or len(starts) == 0:
        raise ValueError("permutation_sweep: starts must be a non-empty vector of row positions")
    if int(starts.min()) < 0 or int(starts.max()) + (seq_len - 1) * tau >= n_rows:
        raise ValueError("permutation_sweep: a window leaves the table (rows %d .. %d of %d)"
                         % (int(starts.min()), int(starts.max()) + (seq_len - 1) * tau, n_rows))
    P = 0 if perms is None else perms.shape[0]
    if colperm.ndim != 2 or colperm.shape[1] != n_cols:
        raise ValueError("permutation_sweep: colperm must be (variants, %d)" % n_cols)
    if int(colperm.min()) < -1 or int(colperm.max()) >= P:
        raise ValueError("permutation_sweep: colperm names a permutation that does not exist")
    if P and (perms.shape[1] != n_rows or int(perms.min()) < 0 or int(perms.max()) >= n_rows):
        raise ValueError("permutation_sweep: perms must be (P, %d) row numbers inside the table" % n_rows)


def _f1_from_confusion(c: np.ndarray) -> float:
    K = c.shape[0]
    idx = np.arange(K)
    labels = np.repeat(np.repeat(idx, K), c.reshape(-1))
    preds = np.repeat(np.tile(idx, K), c.reshape(-1))
    return macro_f1(labels, preds)


def permutation_sweep(model: torch.nn.Module, table, starts, labels, seq_len: int, tau: int, perms, colperm, loss_fn,
                      model_type: str = "single", batch_size: int = 32, drop_last: bool = False,
                      video_batches: Optional[Sequence[torch.Tensor]] = None, windows_per_launch: int = 8192,
                      device=None, want_p0: bool = False, keep_logits: bool = False, timings: Optional[dict] = None) -> dict:
    """Loss, confusion matrix and macro-F1 of every variant of a test set in one device-side sweep.

    table (R, F) fp32 | starts (N,) row positions | labels (N,) | perms (P, R) int32 or None | colperm (V, F) int32, -1 = unchanged.
    Window i of variant v is ``table[p_{v,f}(starts[i] + t*tau), f]``, t < seq_len.  ``batch_size`` / ``drop_last`` are the loader's:
    they define the batches whose losses are summed.  model_type "multi" / "multi-GB": ``video_batches`` are the loader's own
    ``data['video']`` tensors in order; the video side is encoded ONCE per sample (``model.encode_video``) and every variant runs
    ``model.forward_from_video_latent``.  Returns {"loss": [V floats], "batch_loss": (V, S) fp32, "confusion": (V, K, K) int64,
    "score": [V floats]} (+ "p0" (V, N), "logits" (V, N, K) or a list of three for multi-GB, on request).
    ``timings``: a dict that receives the milliseconds of the three stages (gather, forward, accumulate) from device events."""
    if device is None:
        device = next(model.parameters()).device
    device = torch.device(device)
    table_h = table.detach().cpu().numpy() if isinstance(table, torch.Tensor) else np.asarray(table)
    starts_h = np.ascontiguousarray(np.asarray(starts), dtype=np.int64)
    colperm_h = np.ascontiguousarray(np.asarray(colperm), dtype=np.int32)
    perms_h = None if perms is None or len(perms) == 0 else np.ascontiguousarray(np.asarray(perms), dtype=np.int32)
    R, F = table_h.shape
    check_geometry(R, starts_h, int(seq_len), int(tau), perms_h, colperm_h, F)
    labels_h = np.ascontiguousarray(np.asarray(labels).reshape(-1), dtype=np.int64)
    if len(labels_h) != len(starts_h):
        raise ValueError("permutation_sweep: one label per window")
    if model_type not in ("single", "multi", "multi-GB"):
        raise ValueError("permutation_sweep: model_type is 'single', 'multi' or 'multi-GB'")
    bs = int(batch_size)
    N = len(starts_h)
    if drop_last:
        N = (N // bs) * bs
        if N == 0:
            raise ValueError("permutation_sweep: drop_last leaves no batch")
    V = colperm_h.shape[0]
    S_total = (N + bs - 1) // bs

    tab = (table if isinstance(table, torch.Tensor) and table.is_cuda else torch.from_numpy(np.ascontiguousarray(table_h, dtype=np.float32)))
    tab = tab.to(device=device, dtype=torch.float32).contiguous()
    st = torch.from_numpy(starts_h[:N]).to(device)
    tgt = torch.from_numpy(labels_h[:N]).to(device)
    pm = None if perms_h is None else torch.from_numpy(perms_h).to(device)
    cp = torch.from_numpy(colperm_h).to(device)

    gb = model_type == "multi-GB"
    if gb:
        parts, _ = _blend_parts(loss_fn)
        specs = [loss_spec(m, device) for m, _ in parts]
    else:
        specs = [loss_spec(loss_fn, device)]
    n_out = len(specs)

    model.to(device)
    model.eval()
    vis = None
    if model_type != "single":
        if video_batches is None:
            raise ValueError("permutation_sweep: model_type %r needs video_batches" % model_type)
        with torch.no_grad():
            vis = torch.cat([model.encode_video(vb.to(device)) for vb in video_batches], 0)[:N].contiguous()
        if vis.shape[0] != N:
            raise ValueError("permutation_sweep: video_batches hold %d clips for %d windows" % (vis.shape[0], N))

    per_chunk = max(1, int(windows_per_launch) // (V * bs))          # whole loader batches per chunk, V*n <= windows_per_launch
    chunk = per_chunk * bs
    full_seg = torch.arange(0, chunk + 1, bs, dtype=torch.int32, device=device)
    tail_n = N % chunk
    tail_seg = None
    if tail_n:
        tail_seg = torch.tensor(list(range(0, tail_n, bs)) + [tail_n], dtype=torch.int32, device=device)

    loss_buf = [torch.zeros((V, S_total), device=device, dtype=torch.float32) for _ in range(n_out)]
    conf = None
    p0 = torch.empty((V, N), device=device, dtype=torch.float32) if want_p0 else None
    kept: List[List[torch.Tensor]] = [[] for _ in range(n_out)]
    ev = [] if timings is not None else None

    def mark():
        if ev is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            ev.append(e)

    with torch.no_grad():
        for a in range(0, N, chunk):
            n = min(chunk, N - a)
            seg = full_seg if n == chunk else tail_seg
            mark()
            x = ops.window_gather(tab, st[a:a + n], int(seq_len), int(tau), pm, cp).view(V * n, int(seq_len), F)
            mark()
            if model_type == "single":
                out = graphed_forward(model, [x], "_md_graphed_importance") if (_GRAPH and n == chunk) else model(x)
                outs = (out,)
            else:
                out = model.forward_from_video_latent(vis[a:a + n].repeat(V, 1), x)
                outs = tuple(out) if gb else (out,)
            mark()
            outs = tuple(o.contiguous().float() for o in outs)
            K = outs[0].shape[1]
            if conf is None:
                conf = torch.zeros((V, K, K), device=device, dtype=torch.int32)
            p0_chunk = torch.empty((V, n), device=device, dtype=torch.float32) if want_p0 else None
            s0 = a // bs
            for j, (o, (kind, w, m, g)) in enumerate(zip(outs, specs)):
                ops.eval_accumulate(kind, o, tgt[a:a + n], V, seg, w, m, g, loss_buf[j][:, s0:s0 + seg.shape[0] - 1],
                                    conf if j == 0 else None, p0_chunk if j == 0 else None)
                if keep_logits:
                    kept[j].append(o.view(V, n, K).clone())
            if want_p0:
                p0[:, a:a + n] = p0_chunk
            mark()

    # ---- the one read-back
    batch_loss = [b.cpu().numpy() for b in loss_buf]
    conf_h = conf.cpu().numpy().astype(np.int64)
    if ev is not None:
        torch.cuda.synchronize(device)
        g = f = c = 0.0
        for i in range(0, len(ev), 4):
            g += ev[i].elapsed_time(ev[i + 1]); f += ev[i + 1].elapsed_time(ev[i + 2]); c += ev[i + 2].elapsed_time(ev[i + 3])
        timings.update({"gather_ms": g, "forward_ms": f, "accumulate_ms": c, "chunks": len(ev) // 4, "windows_per_chunk": V * chunk})
    if gb:
        per_batch = np.array([[blend(batch_loss[0][v, s], batch_loss[1][v, s], batch_loss[2][v, s], loss_fn) for s in range(S_total)]
                              for v in range(V)], dtype=np.float32)
    else:
        per_batch = batch_loss[0]
    totals = []
    for v in range(V):
        t = 0.0
        for s in range(S_total):
            t += float(per_batch[v, s])                    # total_loss += loss.item()
        totals.append(t)
    res = {"loss": totals, "batch_loss": per_batch, "confusion": conf_h, "score": [_f1_from_confusion(conf_h[v]) for v in range(V)]}
    if want_p0:
        res["p0"] = p0.cpu().numpy()
    if keep_logits:
        logits = [torch.cat(k, 1).cpu().numpy() for k in kept]
        res["logits"] = logits if gb else logits[0]
    return res
