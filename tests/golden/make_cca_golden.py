#!/usr/bin/env python3
"""Generate the Deep-CCA fixtures (cca_loss.npz, cca_loss_E.npz, cca_train.npz) in this directory from the REFERENCE implementation.

Run in the build container only (needs the reference checkout; never on the GPU box):

    python tests/golden/make_cca_golden.py

The reference's ``src/CCA.py`` is imported unmodified.  ``torch.symeig``, which current PyTorch no longer has, is supplied by
``torch.linalg.eigh``; the module's per-batch debug prints go to a swallowed stdout.  Everything runs on the CPU in float64 on
inputs stored as float32 (tests/cca_util.py::planted, seeded).

cca_loss.npz (cases A-D, F, G) and cca_loss_E.npz (case E, a file of its own to stay under the size limit; m = 384), per case X:
  h1/X, h2/X              the inputs, float32 (m, o)
  topk/loss/X             the reference's CCALoss(k, False) in float64
  topk/g1/X, topk/g2/X    its gradients by autograd in float64 (stored as float32 for D and E; not for G, where m < o and the
                          selected subspace is not unique)
  sv/X                    singular values of T, descending
  all/loss/X              -(nuclear norm of T): tests/cca_util.py in float64 (the reference's use_all_singular_values branch takes
                          an element-wise square root and cannot produce it); checked here against autograd through
                          torch.linalg.matrix_norm(T, 'nuc')
  all/g1/X, all/g2/X      its gradients, for the cases with sigma_min >= 1e-2 (A, C, F)
  self32/<key>            the deviation of the float32 run of tests/cca_util.py from <key> (relative; L2 for gradients): the
                          rounding floor.  Tests allow 10 x this figure, or 1e-6 (loss) / 1e-5 (gradients).
The generator ASSERTS what makes the comparisons meaningful: the float64 closed form agrees with the reference's autograd to 1e-6,
sigma_k - sigma_{k+1} >= 2e-3 for every top-k gradient case, sigma_min >= 1e-2 for every all-values gradient case.

cca_train.npz: the reference's train_cca, 3 epochs, DeepCCA(nn.Linear(12, 6), nn.Linear(9, 6)) in float64, CCALoss(3, False), SGD
lr 1e-2 without momentum, the loaders of tests/cca_util.py::train_setup (unshuffled):
  sd/<key>                the initial state dict (float32 values)
  train_loss, valid_loss  per epoch
"""
import contextlib
import importlib.util
import io
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("REFERENCE_ROOT", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cca_util as cu                                                     # noqa: E402

try:
    import tqdm.auto                                                      # noqa: F401
except ImportError:                                                       # the progress bar is not part of what is recorded
    import types
    sys.modules["tqdm"] = types.ModuleType("tqdm")
    sys.modules["tqdm.auto"] = types.ModuleType("tqdm.auto")
    sys.modules["tqdm.auto"].tqdm = lambda it, **k: it
torch.symeig = lambda A, eigenvectors=True, upper=True: torch.linalg.eigh(A, UPLO="U" if upper else "L")
_spec = importlib.util.spec_from_file_location("reference_cca", os.path.join(REF, "src", "CCA.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)
ref.tqdm = lambda it, **k: it

E_ROWS = 384
F32_GRADS = ("D", "E")


def reference_topk(h1, h2, k):
    a = torch.from_numpy(h1).double().requires_grad_()
    b = torch.from_numpy(h2).double().requires_grad_()
    loss = ref.CCALoss(k, False)(a, b)
    loss.backward()
    return float(loss.detach()), a.grad.numpy(), b.grad.numpy()


def autograd_nuclear(h1, h2):
    a = torch.from_numpy(h1).double().requires_grad_()
    b = torch.from_numpy(h2).double().requires_grad_()
    m, o = a.shape
    H1, H2 = (a - a.mean(0, keepdim=True)).t(), (b - b.mean(0, keepdim=True)).t()
    eye = torch.eye(o, dtype=torch.float64)
    S12, S11, S22 = H1 @ H2.t() / (m - 1), H1 @ H1.t() / (m - 1) + cu.R1 * eye, H2 @ H2.t() / (m - 1) + cu.R2 * eye

    def isq(S):
        d, V = torch.linalg.eigh(S)
        return V @ torch.diag(d ** -0.5) @ V.t()
    loss = -torch.linalg.matrix_norm(isq(S11) @ S12 @ isq(S22), "nuc")
    loss.backward()
    return float(loss.detach()), a.grad.numpy(), b.grad.numpy()


def make_loss():
    outs = {"main": {}, "E": {}}
    for name, (m, o, k, rho) in cu.CASES.items():
        if name == "E":
            m = E_ROWS
        out = outs["E" if name == "E" else "main"]
        h1, h2 = cu.planted(m, o, rho)
        out["h1/" + name], out["h2/" + name] = h1, h2
        L, g1, g2 = reference_topk(h1, h2, k)
        cL, c1, c2, sv = cu.cca_closed_form(h1, h2, k, False)
        nL, n1, n2, _ = cu.cca_closed_form(h1, h2, k, True)
        s32 = cu.cca_closed_form(h1, h2, k, False, np.float32)
        a32 = cu.cca_closed_form(h1, h2, k, True, np.float32)
        gap, smin = float(sv[k - 1] - sv[k]), float(sv.min())
        assert cu.rel_abs(cL, L) < 1e-9, (name, cL, L)
        out["topk/loss/" + name], out["sv/" + name] = np.float64(L), sv
        out["self32/topk/loss/" + name] = cu.rel_abs(s32[0], L)
        out["all/loss/" + name] = np.float64(nL)
        out["self32/all/loss/" + name] = cu.rel_abs(a32[0], nL)
        line = "%s (%d, %d, %d) gap %.4f sigma_min %.4f | self32 loss topk %.1e all %.1e" % (
            name, m, o, k, gap, smin, out["self32/topk/loss/" + name], out["self32/all/loss/" + name])
        dt = np.float32 if name in F32_GRADS else np.float64
        if name in cu.TOPK_GRAD:
            assert gap >= 2e-3, (name, gap)
            assert cu.rel_l2(c1, g1) < 1e-6 and cu.rel_l2(c2, g2) < 1e-6, (name, cu.rel_l2(c1, g1), cu.rel_l2(c2, g2))
            out["topk/g1/" + name], out["topk/g2/" + name] = g1.astype(dt), g2.astype(dt)
            out["self32/topk/g1/" + name], out["self32/topk/g2/" + name] = cu.rel_l2(s32[1], g1), cu.rel_l2(s32[2], g2)
            line += " | closed form vs autograd %.1e %.1e | self32 g %.1e %.1e" % (
                cu.rel_l2(c1, g1), cu.rel_l2(c2, g2), out["self32/topk/g1/" + name], out["self32/topk/g2/" + name])
        if name in cu.ALL_GRAD:
            assert smin >= 1e-2, (name, smin)
            bL, b1, b2 = autograd_nuclear(h1, h2)
            assert cu.rel_abs(nL, bL) < 1e-9 and cu.rel_l2(n1, b1) < 1e-6 and cu.rel_l2(n2, b2) < 1e-6, name
            out["all/g1/" + name], out["all/g2/" + name] = n1.astype(dt), n2.astype(dt)
            out["self32/all/g1/" + name], out["self32/all/g2/" + name] = cu.rel_l2(a32[1], n1), cu.rel_l2(a32[2], n2)
            line += " | all: vs autograd %.1e | self32 g %.1e %.1e" % (
                cu.rel_l2(n1, b1), out["self32/all/g1/" + name], out["self32/all/g2/" + name])
        print(line)
    outs["E"]["rows/E"] = np.int64(E_ROWS)
    for tag, fn in (("main", "cca_loss.npz"), ("E", "cca_loss_E.npz")):
        path = os.path.join(HERE, fn)
        np.savez_compressed(path, **outs[tag])
        print(fn, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < 1000 * 1000


def make_train():
    train, valid = cu.train_setup()
    dbl = lambda bs: [({k: v.double() for k, v in d.items()}, t) for d, t in bs]          # noqa: E731
    torch.manual_seed(cu.SEED + 2)
    model = ref.DeepCCA(torch.nn.Linear(12, 6), torch.nn.Linear(9, 6))
    out = {"sd/" + k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    model.double()
    opt = torch.optim.SGD(model.parameters(), lr=1e-2)
    with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(io.StringIO()):
        tl, vl = ref.train_cca(dbl(train), dbl(valid), model, opt, None, ref.CCALoss(3, False), "cpu", 3, None,
                               os.path.join(tmp, "best.pt"), os.path.join(tmp, "last.pt"), None)
    out["train_loss"], out["valid_loss"] = np.array(tl, dtype=np.float64), np.array(vl, dtype=np.float64)
    np.savez_compressed(os.path.join(HERE, "cca_train.npz"), **out)
    print("cca_train.npz train", tl, "valid", vl)


if __name__ == "__main__":
    make_loss()
    make_train()
