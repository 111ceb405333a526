"""Latent-space reductions on the MI355X (csrc/embed.hip): collect ``model.encode`` latents on the GPU, incremental PCA as
scikit-learn's ``IncrementalPCA(n_components=k).fit_transform`` computes it, and exact t-SNE as ``TSNE(method="exact")`` computes it.

PCA.  Batches as scikit-learn cuts them (``batch_size = 5 D``, a tail shorter than k joins the previous batch).  Per batch the top-k
right singular pairs of the stacked matrix [S V^T of the batches so far; X_b - mean_b; sqrt(n_seen n_b / (n_seen + n_b)) (mean - mean_b)]
come from a subspace iteration on 8 columns: W = M V and Z = M^T W run on the GPU with the centring and the extra rows applied while
the batch is read (md_tsmm_mv / md_tsmm_mtw, fp64 accumulation); the 8 x 8 Gram matrices V^T V and W^T W come back to the host once
per round, where a generalised Rayleigh-Ritz step in fp64 gives the singular values, the rotation to Ritz vectors and the next
(rescaled) basis.  The D x D Gram matrix is never formed.  Signs: the largest-magnitude entry of every component is positive.

t-SNE.  md_sqdist -> md_tsne_conditional -> md_tsne_joint share one N x N buffer; then per iteration md_tsne_gradient (two launches)
and md_tsne_update, queued without a host round trip.  The stopping rules are evaluated at scikit-learn's checkpoints only (every
50 iterations), each of which costs one read-back of a few doubles (``_readback``).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np
import torch

from .. import _native as N
from .. import ops
from ..ops import _p, _stream

Q = 8                       # columns of the iterated subspace: k + oversampling, k <= 3
MAX_N = 32768               # MD_EMBED_MAX_N
PCA_ROUNDS = 200
PCA_TOL = 1e-7
N_ITER_CHECK = 50
EXPLORATION_ITERS = 250
MIN_GRAD_NORM = 1e-7


def _readback(t: torch.Tensor) -> np.ndarray:
    """The one device-to-host copy (and synchronisation) of a checkpoint or a Rayleigh-Ritz round."""
    return t.cpu().numpy()


def _latent(latent: torch.Tensor) -> torch.Tensor:
    if not isinstance(latent, torch.Tensor):
        raise TypeError("latent must be a torch.Tensor on the GPU")
    if latent.dim() != 2:
        raise ValueError("latent must be (N, D), got %s" % (tuple(latent.shape),))
    latent = latent.detach()
    if not latent.is_cuda:
        raise RuntimeError("mi355x hot path: CPU tensor given; this path runs on the GPU only (no CPU fallback)")
    return ops.f32(latent).contiguous()


# ---------------------------------------------------------------------------------------------------------------------- collect
def collect_latents(model, dataloader, device, limit_iters: int, multi: bool = False, with_probs: bool = False):
    """(latents, labels) resident on `device`: latents is one (N, D) tensor, or for ``multi`` the (fused, video, 0D) triple.
    With ``with_probs`` (single-model form) also softmax(model(batch))[:, 0] of the very batch that was encoded, as a third result:
    the loader is walked once, so a loader that shuffles keeps latents, labels and probabilities of one window together.

    The loop bound is the reference's: its ``break`` sits after the batch, so ``limit_iters = n > 0`` consumes n + 1 batches and
    ``limit_iters <= 0`` the whole loader."""
    if with_probs and multi:
        raise ValueError("with_probs is defined for the single-model form only")
    model.to(device)
    model.eval()
    parts: List[Tuple[torch.Tensor, ...]] = []
    labels = []
    probs = []
    with torch.no_grad():
        for idx, (data, target) in enumerate(dataloader):
            if multi:
                video, sig = data["video"].to(device), data["0D"].to(device)
                batch = video.size(0)
                lat = tuple(model.encode(video, sig))
            else:
                data = data.to(device)
                batch = data.size(0)
                lat = (model.encode(data),)
                if with_probs:
                    probs.append(torch.softmax(model(data), dim=1)[:, 0].detach())
            parts.append(tuple(v.detach().reshape(batch, -1) for v in lat))
            labels.append(target.detach().to(device).reshape(-1))
            if limit_iters > 0 and idx + 1 > limit_iters:
                break
    if not parts:
        raise ValueError("the dataloader yielded no batch")
    cat = tuple(torch.cat([p[i] for p in parts], 0).float().contiguous() for i in range(len(parts[0])))
    label = torch.cat(labels, 0).to(torch.int64)
    if with_probs:
        return cat[0], label, torch.cat(probs, 0)
    return (cat if multi else cat[0]), label


# ---------------------------------------------------------------------------------------------------------------------- PCA
def gen_batches(n: int, batch_size: int, min_batch_size: int = 0):
    """sklearn.utils.gen_batches as (start, stop) pairs."""
    out, start = [], 0
    for _ in range(int(n // batch_size)):
        end = start + batch_size
        if end + min_batch_size > n:
            continue
        out.append((start, end))
        start = end
    if start < n:
        out.append((start, n))
    return out


def col_mean(x: torch.Tensor) -> torch.Tensor:
    """Column means of x (rows, D) as float64 (md_col_mean)."""
    L = N.lib()
    rows, D = x.shape
    mean = torch.empty(D, dtype=torch.float64, device=x.device)
    scratch = torch.empty(L.md_col_mean_scratch_doubles(rows, D), dtype=torch.float64, device=x.device)
    N.check(L.md_col_mean(_p(x), rows, D, _p(mean), _p(scratch), _stream()), "md_col_mean")
    return mean


def tsmm_mv(M: torch.Tensor, mean: Optional[torch.Tensor], extra: Optional[torch.Tensor], V: torch.Tensor) -> torch.Tensor:
    """[M - mean; extra] V for V (D, 8) -> (rows + E, 8) (md_tsmm_mv)."""
    rows, D = M.shape
    E = 0 if extra is None else extra.shape[0]
    W = torch.empty((rows + E, Q), device=M.device)
    N.check(N.lib().md_tsmm_mv(_p(M), rows, D, _p(mean), _p(extra), E, _p(V), _p(W), _stream()), "md_tsmm_mv")
    return W


def tsmm_mtw(M: torch.Tensor, mean: Optional[torch.Tensor], extra: Optional[torch.Tensor], W: torch.Tensor, f64: bool = False):
    """[M - mean; extra]^T W for W (rows + E, 8) -> (D, 8), float32 or float64 (md_tsmm_mtw)."""
    L = N.lib()
    rows, D = M.shape
    E = 0 if extra is None else extra.shape[0]
    out = torch.empty((D, Q), device=M.device, dtype=torch.float64 if f64 else torch.float32)
    scratch = torch.empty(L.md_tsmm_mtw_scratch_doubles(rows, D, E), dtype=torch.float64, device=M.device)
    N.check(L.md_tsmm_mtw(_p(M), rows, D, _p(mean), _p(extra), E, _p(W), None if f64 else _p(out), _p(out) if f64 else None,
                          _p(scratch), _stream()), "md_tsmm_mtw")
    return out


def _rayleigh_ritz(gv: np.ndarray, h: np.ndarray):
    """Generalised Rayleigh-Ritz on the host in fp64: gv = V^T V, h = V^T M^T M V (8 x 8) -> (theta descending, E with V E the
    orthonormal Ritz basis).  Directions of V that are numerically dependent are dropped (their columns of E are zero)."""
    gv = (gv + gv.T) * 0.5
    h = (h + h.T) * 0.5
    lam, u = np.linalg.eigh(gv)
    keep = lam > lam.max() * 1e-10
    t = u[:, keep] / np.sqrt(lam[keep])
    th, r = np.linalg.eigh(t.T @ h @ t)
    order = np.argsort(-th, kind="stable")
    th, r = th[order], r[:, order]
    e = np.zeros((Q, Q))
    e[:, :th.size] = t @ r
    theta = np.zeros(Q)
    theta[:th.size] = np.maximum(th, 0.0)
    return theta, e


def _start_basis(D: int, device) -> torch.Tensor:
    """The deterministic start of the subspace iteration: a fixed-seed Gaussian D x 8 block drawn on the host."""
    return torch.from_numpy(np.random.RandomState(20240).standard_normal((D, Q)).astype(np.float32)).to(device)


def _top_singular(M: torch.Tensor, mean: Optional[torch.Tensor], extra: Optional[torch.Tensor], k: int):
    """Top-k right singular vectors (k, D) and singular values of the stacked matrix, by subspace iteration."""
    rows, D = M.shape
    dev = M.device
    V = _start_basis(D, dev)
    prev = last_delta = remaining = None
    rate = 0.0
    theta = e = None
    for _ in range(PCA_ROUNDS):
        W = tsmm_mv(M, mean, extra, V)
        gv = tsmm_mtw(V, None, None, V, f64=True)                  # V^T V
        h = tsmm_mtw(W, None, None, W, f64=True)                   # W^T W = V^T M^T M V
        small = _readback(torch.stack([gv, h]))
        theta, e = _rayleigh_ritz(small[0], small[1])
        sv = np.sqrt(theta[:k])
        # Singular values converge like rho^(2t), the vectors only like rho^t, and fp32 operands cannot resolve a value change below
        # ~1e-8.  So: measure the contraction of the value change per round while it is above that noise, and once the change is
        # below PCA_TOL run the rounds that bring it down by another factor PCA_TOL at that rate (vectors then sit at ~PCA_TOL).
        if prev is not None:
            delta = float(np.max(np.abs(sv - prev) / np.maximum(sv, 1e-300)))
            if last_delta is not None and last_delta > 1e-6:
                rate = max(rate, min(delta / last_delta, 0.95))
            if remaining is None and delta <= PCA_TOL:
                r = rate if rate > 0.0 else (delta / last_delta if last_delta else 0.0)
                remaining = int(math.ceil(math.log(PCA_TOL) / math.log(min(max(r, 1e-3), 0.95))))
            last_delta = delta
        if remaining is not None:
            if remaining == 0:
                break
            remaining -= 1
        prev = sv
        Z = tsmm_mtw(M, mean, extra, W)                            # M^T M V
        scale = np.where(theta > theta[0] * 1e-14, 1.0 / np.maximum(theta, 1e-300), 0.0)
        T = torch.from_numpy((e * scale[None, :]).astype(np.float32)).to(dev)
        V = tsmm_mv(Z, None, None, T)                              # Z E / theta: nearly orthonormal once V E are Ritz vectors
    if theta[k - 1] <= 0.0:
        raise ValueError("the latents have rank below n_components = %d" % k)
    comp = tsmm_mv(V, None, None, torch.from_numpy(e.astype(np.float32)).to(dev))[:, :k].t().contiguous()
    j = comp.abs().argmax(dim=1, keepdim=True)                     # svd_flip(u_based_decision=False)
    sign = torch.sign(comp.gather(1, j))
    sign[sign == 0] = 1.0
    return comp * sign, np.sqrt(theta[:k])


def _check_k(n_components: int) -> int:
    k = int(n_components)
    if k not in (2, 3):
        raise ValueError("n_components must be 2 or 3, got %r" % (n_components,))
    return k


def pca_fit(latent: torch.Tensor, n_components: int, batch_size: Optional[int] = None):
    """(components (k, D) float32, singular values (k,) float64 on the host, mean (D,) float64) of the incremental fit."""
    k = _check_k(n_components)
    x = _latent(latent)
    n, D = x.shape
    if min(n, D) < k:
        raise ValueError("n_components = %d needs at least %d rows and columns, got (%d, %d)" % (k, k, n, D))
    bs = 5 * D if batch_size is None else int(batch_size)
    mean = torch.zeros(D, dtype=torch.float64, device=x.device)
    comp = sv = None
    seen = 0
    for a, b in gen_batches(n, bs, min_batch_size=k):
        xb = x[a:b]
        nb = b - a
        bmean = col_mean(xb)
        extra = None
        if seen:
            corr = math.sqrt(seen * nb / (seen + nb)) * (mean - bmean)
            extra = torch.cat([torch.from_numpy(sv).to(x.device)[:, None] * comp.double(), corr[None]], 0).float().contiguous()
        comp, sv = _top_singular(xb, bmean.float(), extra, k)
        mean = (mean * seen + bmean * nb) / (seen + nb)
        seen += nb
    return comp, sv, mean


def pca_embed(latent: torch.Tensor, n_components: int) -> torch.Tensor:
    """IncrementalPCA(n_components).fit_transform(latent) as an (N, k) float32 tensor on the GPU."""
    _check_k(n_components)
    x = _latent(latent)
    comp, _, mean = pca_fit(x, n_components)
    k, D = comp.shape
    V = torch.zeros((D, Q), device=x.device)
    V[:, :k] = comp.t()
    return tsmm_mv(x, mean.float(), None, V)[:, :k].contiguous()


# ---------------------------------------------------------------------------------------------------------------------- t-SNE
@dataclass
class TSNEResult:
    kl_divergence: float
    n_iter: int
    learning_rate: float
    history: List[Tuple[int, float, float]] = field(default_factory=list)      # (iteration, error, gradient norm) per checkpoint


def sqdist(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    x = _latent(x)
    n, D = x.shape
    if out is None:
        out = torch.empty((n, n), device=x.device)
    N.check(N.lib().md_sqdist(_p(x), n, D, _p(out), _stream()), "md_sqdist")
    return out


def joint_probabilities(latent: torch.Tensor, perplexity: float) -> torch.Tensor:
    """The joint P (N, N) of exact t-SNE; distances, conditional and joint stages share the one buffer."""
    x = _latent(latent)
    n = x.shape[0]
    L = N.lib()
    P = sqdist(x)
    N.check(L.md_tsne_conditional(_p(P), n, float(perplexity), _p(P), _stream()), "md_tsne_conditional")
    scratch = torch.empty(L.md_tsne_joint_scratch_doubles(n), dtype=torch.float64, device=x.device)
    N.check(L.md_tsne_joint(_p(P), n, _p(P), _p(scratch), _stream()), "md_tsne_joint")
    return P


class _Descent:
    """The per-iteration launches of one map and their buffers."""

    def __init__(self, P: torch.Tensor, y: torch.Tensor):
        L = N.lib()
        self.L, self.P, self.y = L, P, y
        self.n, self.nc = y.shape
        dev = y.device
        self.rowpart = torch.empty(L.md_tsne_rowpart_floats(self.n, self.nc), device=dev)
        self.scratch = torch.empty(L.md_tsne_scratch_doubles(self.n), dtype=torch.float64, device=dev)
        self.grad = torch.empty_like(y)
        self.nblk = L.md_tsne_update_blocks(self.n * self.nc)
        self.stats = torch.zeros(8 + self.nblk, dtype=torch.float64, device=dev)      # [Z, KL, sum P, ...] + |gains grad|^2 shares
        self.gpart = self.stats[8:]

    def gradient(self, exaggeration: float, want_kl: bool) -> None:
        N.check(self.L.md_tsne_gradient(_p(self.P), _p(self.y), self.n, self.nc, float(exaggeration), int(want_kl), _p(self.rowpart),
                                        _p(self.scratch), _p(self.grad), _p(self.stats), _stream()), "md_tsne_gradient")

    def update(self, upd: torch.Tensor, gains: torch.Tensor, momentum: float, lr: float, min_gain: float = 0.01) -> None:
        N.check(self.L.md_tsne_update(_p(self.y), _p(upd), _p(gains), _p(self.grad), self.n * self.nc, float(momentum), float(lr),
                                      float(min_gain), _p(self.gpart), _stream()), "md_tsne_update")

    def phase(self, it: int, max_iter: int, exaggeration: float, momentum: float, lr: float, patience: int, history):
        """scikit-learn's _gradient_descent from iteration `it`: fresh update / gains, stopping rules at the checkpoints."""
        upd, gains = torch.zeros_like(self.y), torch.ones_like(self.y)
        error = best = float(np.finfo(float).max)
        best_iter = i = it
        for i in range(it, max_iter):
            check = (i + 1) % N_ITER_CHECK == 0
            want = check or i == max_iter - 1
            self.gradient(exaggeration, want)
            self.update(upd, gains, momentum, lr)
            if want:
                s = _readback(self.stats)
                error = float(s[1])
            if check:
                gnorm = math.sqrt(float(np.sum(s[8:])))
                history.append((i + 1, error, gnorm))
                if error < best:
                    best, best_iter = error, i
                elif i - best_iter > patience:
                    break
                if gnorm <= MIN_GRAD_NORM:
                    break
        return error, i


def pca_init(x: torch.Tensor, nc: int) -> torch.Tensor:
    """First nc components of an exact PCA of x (one batch), scaled so that column 0 has standard deviation 1e-4."""
    comp, _, mean = pca_fit(x, nc, batch_size=max(x.shape[0], 1))
    k, D = comp.shape
    V = torch.zeros((D, Q), device=x.device)
    V[:, :k] = comp.t()
    e = tsmm_mv(x, mean.float(), None, V)[:, :k].contiguous()
    return (e / e[:, 0].std(unbiased=False) * 1e-4).contiguous()


def tsne_embed(latent: torch.Tensor, n_components: int = 2, perplexity: float = 30.0, early_exaggeration: float = 12.0,
               learning_rate="auto", max_iter: int = 1000, init="pca", n_iter_without_progress: int = 300):
    """Exact t-SNE of latent (N, D) -> (embedding (N, nc) float32 on the GPU, TSNEResult)."""
    nc = _check_k(n_components)
    if isinstance(latent, torch.Tensor) and latent.dim() == 2 and perplexity >= latent.shape[0]:
        raise ValueError("perplexity must be less than n_samples")          # scikit-learn's check, before anything touches the GPU
    x = _latent(latent)
    n = x.shape[0]
    if n > MAX_N:
        raise ValueError("exact t-SNE holds a dense N x N matrix; N = %d is above the limit %d" % (n, MAX_N))
    if max_iter < EXPLORATION_ITERS:
        raise ValueError("max_iter must be at least %d" % EXPLORATION_ITERS)
    lr = max(n / early_exaggeration / 4.0, 50.0) if learning_rate == "auto" else float(learning_rate)
    if isinstance(init, str):
        if init != "pca":
            raise ValueError("init must be 'pca' or an (N, n_components) array")
        y = pca_init(x, nc)
    else:
        y = torch.as_tensor(np.asarray(init.detach().cpu() if isinstance(init, torch.Tensor) else init), dtype=torch.float32)
        if tuple(y.shape) != (n, nc):
            raise ValueError("init must be (%d, %d), got %s" % (n, nc, tuple(y.shape)))
        y = y.to(x.device).contiguous().clone()
    P = joint_probabilities(x, perplexity)
    d = _Descent(P, y)
    res = TSNEResult(kl_divergence=float("nan"), n_iter=0, learning_rate=lr)
    error, it = d.phase(0, EXPLORATION_ITERS, early_exaggeration, 0.5, lr, EXPLORATION_ITERS, res.history)
    if it < EXPLORATION_ITERS or max_iter - EXPLORATION_ITERS > 0:
        error, it = d.phase(it + 1, max_iter, 1.0, 0.8, lr, int(n_iter_without_progress), res.history)
    res.kl_divergence, res.n_iter = error, it
    return y, res
