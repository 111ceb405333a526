"""Deep CCA -- MI355X-native mirror of the reference's ``src/CCA.py`` (DeepCCA :8-21, CCALoss :25-83, the loops :85-222).

Same names, constructor arguments and return values.  ``CCALoss.forward`` is one ``torch.autograd.Function`` over
``md_cca_loss_fwd`` / ``md_cca_loss_bwd`` (csrc/cca.hip): covariances, a device-side symmetric eigensolver that lives in LDS, the
whitened cross-covariance T and the closed-form gradient, in a fixed number of launches with no host synchronisation, so a training
step with this loss can be captured in a HIP graph.  Deliberate deviations from the reference:

  * ``use_all_singular_values=True`` is the sum of ALL singular values of T (the nuclear norm), as Andrew et al. define it, not the
    reference's element-wise square root of T^T T (whose gradient is NaN);
  * ``o2`` is the second view's own width (the reference reads ``h1.size(0)`` twice and fails on unequal widths);
  * the gradient is the closed form of DESIGN.md section 13, which divides by no gap between two selected eigenvalues and stays
    finite for m <= o;
  * the loops print nothing per batch and read the summed loss back once per epoch.
"""
from typing import Optional

import torch
import torch.nn as nn
from torch.utils.data import DataLoader

from . import ops

try:
    from tqdm.auto import tqdm
except ImportError:  # pragma: no cover
    def tqdm(it, **k):
        return it

MAX_WIDTH = ops.CCA_MAX_O


class DeepCCA(nn.Module):
    """Two encoders side by side: forward(x1, x2) -> (z1, z2)."""

    def __init__(self, encoder_1: nn.Module, encoder_2: nn.Module):
        super().__init__()
        self.encoder_1, self.encoder_2 = encoder_1, encoder_2

    def forward(self, x1: torch.Tensor, x2: torch.Tensor):
        return self.encoder_1(x1), self.encoder_2(x2)


class _CCALossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h1, h2, k, r1, r2, eps):
        h1 = h1.contiguous().float()
        h2 = h2.contiguous().float()
        loss, ws = ops.cca_loss_fwd(h1, h2, k, r1, r2, eps)
        ctx.save_for_backward(ws)
        ctx.dims = (h1.shape[0], h1.shape[1], h2.shape[1], k, eps)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        (ws,) = ctx.saved_tensors
        m, o1, o2, k, eps = ctx.dims
        dh1, dh2 = ops.cca_loss_bwd(g.contiguous().float().view(1), ws, m, o1, o2, k, eps)
        return dh1, dh2, None, None, None, None


class CCALoss(nn.Module):
    def __init__(self, output_dim: int, use_all_singular_values: bool):
        super().__init__()
        self.output_dim, self.use_all_singular_values = output_dim, use_all_singular_values
        self.r1 = self.r2 = 1e-3           # ridge on the two covariance matrices
        self.eps = 1e-6                    # eigenvalues at or below it are discarded / clamped

    def forward(self, h1: torch.Tensor, h2: torch.Tensor):
        if not (h1.is_cuda and h2.is_cuda):
            raise RuntimeError("mi355x hot path: CPU tensor given; this path runs on the GPU only (no CPU fallback)")
        if h1.dim() != 2 or h2.dim() != 2 or h1.size(0) != h2.size(0):
            raise ValueError("CCALoss: h1 is (m, o1) and h2 is (m, o2) with the same m")
        m, o1, o2 = h1.size(0), h1.size(1), h2.size(1)
        if o1 > MAX_WIDTH or o2 > MAX_WIDTH:
            raise ValueError("CCALoss: latent widths (%d, %d) exceed the limit of %d of the device eigensolver" % (o1, o2, MAX_WIDTH))
        if m < 2 or o1 < 1 or o2 < 1:
            raise ValueError("CCALoss: needs at least 2 samples and 1 latent dimension per view")
        k = 0
        if not self.use_all_singular_values:
            k = int(self.output_dim)
            if k < 1 or k > o2:
                raise ValueError("CCALoss: output_dim = %d, but the second view has %d dimensions" % (k, o2))
        return _CCALossFunction.apply(h1, h2, k, self.r1, self.r2, self.eps)


def _views(data, device):
    return data["video"].to(device), data["0D"].to(device)


def _mean_loss(total: Optional[torch.Tensor], batches: int) -> float:
    """The one read-back of an epoch: the loss was summed on the device."""
    if batches == 0:
        raise ValueError("CCA loop: the loader yielded no batch")
    return float(total) / batches


def _train_per_epoch(
    train_loader: DataLoader,
    model: DeepCCA,
    optimizer: torch.optim.Optimizer,
    loss_fn: CCALoss,
    scheduler: Optional[torch.optim.lr_scheduler._LRScheduler],
    device: str = "cpu",
    max_norm_grad: Optional[float] = None,
):
    model.train()
    model.to(device)
    total, batches = None, 0
    for data, _ in train_loader:
        optimizer.zero_grad()
        loss = loss_fn(*model(*_views(data, device)))
        loss.backward()
        if max_norm_grad:
            torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm_grad)
        optimizer.step()
        step_loss = loss.detach()
        total = step_loss.clone() if total is None else total.add_(step_loss)
        batches += 1
    if scheduler:
        scheduler.step()
    return _mean_loss(total, batches)


def _eval_epoch(loader, model, loss_fn, device):
    model.eval()
    model.to(device)
    total, batches = None, 0
    with torch.no_grad():
        for data, _ in loader:
            loss = loss_fn(*model(*_views(data, device)))
            total = loss.clone() if total is None else total.add_(loss)
            batches += 1
    return _mean_loss(total, batches)


def _valid_per_epoch(
    valid_loader: DataLoader,
    model: torch.nn.Module,
    optimizer: torch.optim.Optimizer,
    loss_fn: torch.nn.Module,
    device: str = "cpu",
):
    optimizer.zero_grad()
    return _eval_epoch(valid_loader, model, loss_fn, device)


def evaluate_cca_loss(
    test_loader: DataLoader,
    model: torch.nn.Module,
    loss_fn: torch.nn.Module,
    device: str = "cpu",
):
    return _eval_epoch(test_loader, model, loss_fn, device)


def train_cca(
    train_loader: DataLoader,
    valid_loader: DataLoader,
    model: DeepCCA,
    optimizer: torch.optim.Optimizer,
    scheduler: Optional[torch.optim.lr_scheduler._LRScheduler],
    loss_fn: CCALoss,
    device: str = "cpu",
    num_epoch: int = 64,
    verbose: Optional[int] = 8,
    save_best_dir: str = "./weights/cca_best.pt",
    save_last_dir: str = "./weights/cca_last.pt",
    max_norm_grad: Optional[float] = None,
):
    """Returns (train losses, validation losses) per epoch.  The state dict goes to ``save_last_dir`` after every epoch and to
    ``save_best_dir`` whenever the validation loss improves (src/CCA.py:211-218)."""
    history = ([], [])
    best = (torch.inf, 0)
    for epoch in tqdm(range(num_epoch), desc="training CCA process"):
        losses = (_train_per_epoch(train_loader, model, optimizer, loss_fn, scheduler, device, max_norm_grad),
                  _valid_per_epoch(valid_loader, model, optimizer, loss_fn, device))
        for log, value in zip(history, losses):
            log.append(value)
        if verbose and epoch % verbose == 0:
            print("epoch : {}, train loss : {:.3f}, valid loss : {:.3f}".format(epoch + 1, *losses))
        if losses[1] < best[0]:
            best = (losses[1], epoch)
            torch.save(model.state_dict(), save_best_dir)
        torch.save(model.state_dict(), save_last_dir)
    print("(Report) training CCA process finished, best loss : {:.3f}, best epoch : {}".format(*best))
    return history
