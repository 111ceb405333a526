"""Restatement of the CCA loss and of its closed-form gradient in numpy, at a chosen precision (float64: what the GPU kernels of
csrc/cca.hip are compared with; float32: the rounding floor recorded as ``self32/...`` in tests/golden/cca_loss.npz), and the seeded
inputs of the fixtures.  tests/golden/make_cca_golden.py checks the float64 run against autograd through the reference's own
``CCALoss`` (src/CCA.py:25-83).

The gradient divides by no gap between two selected eigenvalues:
    G_M = sum_{i in S, lam_i > eps} w_i w_i^T / (2 sqrt(lam_i)),  G_T = 2 T G_M,  G_S12 = A G_T B,
    G_A = G_T (S12 B)^T,  G_B = (A S12)^T G_T,  G_S11 = V1 [K1 o (V1^T sym(G_A) V1)] V1^T,
    K1_ij = -1 / (sqrt(d_i) sqrt(d_j) (sqrt(d_i) + sqrt(d_j)))      (the divided difference of d^-1/2; no special case for d_i = d_j)
    dH1 = (2 G_S11 H1 + G_S12 H2) / (m - 1),  dH2 = (2 G_S22 H2 + G_S12^T H1) / (m - 1),  negated for the loss.
"""
import numpy as np
import torch

R1 = R2 = 1e-3
EPS = 1e-6
SEED = 7

# name -> (m, o, k, rho or None)
CASES = {
    "A": (40, 5, 2, [.95, .8, .6, .35, .1]),
    "B": (96, 16, 4, np.linspace(.95, .05, 16)),
    "C": (200, 33, 6, np.linspace(.97, .03, 33)),
    "D": (256, 64, 8, np.linspace(.98, .02, 64)),
    "E": (512, 128, 10, np.linspace(.98, .02, 128)),
    "F": (24, 16, 4, np.linspace(.95, .05, 16)),
    "G": (8, 16, 4, None),
}
TOPK_GRAD = ("A", "B", "C", "D", "E", "F")        # sigma_k - sigma_{k+1} >= 2e-3 asserted by the generator
ALL_GRAD = ("A", "C", "F")                        # sigma_min >= 1e-2 asserted by the generator


def planted(m, o, rho, seed=SEED):
    """h1 = z a + shift, h2 = (z rho + e sqrt(1 - rho^2)) b - shift as float32 arrays (m, o); rho None: plain random inputs."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)              # noqa: E731
    z, e = rn(m, o), rn(m, o)
    a, b = rn(o, o) / o ** 0.5, rn(o, o) / o ** 0.5
    if rho is None:
        h1, h2 = z @ a + 0.3 * rn(1, o), e @ b - 0.2
    else:
        r = torch.tensor(np.asarray(rho, dtype=np.float64))
        h1 = z @ a + 0.3 * rn(1, o)
        h2 = (z * r + e * (1 - r * r).sqrt()) @ b - 0.2
    return h1.numpy().astype(np.float32), h2.numpy().astype(np.float32)


def case_inputs(name):
    m, o, k, rho = CASES[name]
    return planted(m, o, rho)


def train_setup():
    """The loaders of cca_train.npz as lists of (dict, target): 4 training and 2 validation batches of 48 pairs, 'video' (48, 12) and
    '0D' (48, 9), float32, sharing a 6-dimensional latent."""
    g = torch.Generator().manual_seed(SEED + 1)
    n = 48 * 6
    z = torch.randn(n, 6, generator=g)
    x1 = z @ torch.randn(6, 12, generator=g) + 0.3 * torch.randn(n, 12, generator=g)
    x2 = z @ torch.randn(6, 9, generator=g) + 0.3 * torch.randn(n, 9, generator=g)
    batches = [({"video": x1[i:i + 48].clone(), "0D": x2[i:i + 48].clone()}, torch.zeros(48, dtype=torch.long)) for i in range(0, n, 48)]
    return batches[:4], batches[4:]


def _inv_sqrt_parts(S, eps):
    d, V = np.linalg.eigh(S)
    keep = d > eps
    f = np.where(keep, np.where(keep, d, 1) ** -0.5, 0).astype(S.dtype)
    return d, V, keep, f


def _back(G, d, V, keep, f):
    """Gradient of S -> V f(d) V^T through the divided differences of f = d^-1/2 on the kept eigenvalues (f = 0 on the others)."""
    s = np.sqrt(np.where(keep, d, 1))
    both = keep[:, None] & keep[None, :]
    K = np.where(both, -1.0 / (s[:, None] * s[None, :] * (s[:, None] + s[None, :])), 0.0)
    one = keep[:, None] ^ keep[None, :]
    if one.any():
        dd = d[:, None] - d[None, :]
        K = np.where(one, (f[:, None] - f[None, :]) / np.where(one, dd, 1), K)
    K = K.astype(G.dtype)
    return V @ (K * (V.T @ (0.5 * (G + G.T)) @ V)) @ V.T


def cca_closed_form(h1, h2, k, use_all, dtype=np.float64, r1=R1, r2=R2, eps=EPS):
    """Returns (loss, dh1 (m, o1), dh2 (m, o2), singular values of T descending), all in ``dtype``.  k is ignored with use_all."""
    h1, h2 = np.asarray(h1, dtype=dtype), np.asarray(h2, dtype=dtype)
    m, o1 = h1.shape
    o2 = h2.shape[1]
    H1, H2 = (h1 - h1.mean(0, keepdims=True)).T, (h2 - h2.mean(0, keepdims=True)).T
    c = dtype(1.0) / dtype(m - 1)
    S12 = c * (H1 @ H2.T)
    S11 = c * (H1 @ H1.T) + dtype(r1) * np.eye(o1, dtype=dtype)
    S22 = c * (H2 @ H2.T) + dtype(r2) * np.eye(o2, dtype=dtype)
    d1, V1, k1, f1 = _inv_sqrt_parts(S11, eps)
    d2, V2, k2, f2 = _inv_sqrt_parts(S22, eps)
    A, B = (V1 * f1) @ V1.T, (V2 * f2) @ V2.T
    T = A @ S12 @ B
    M = T.T @ T + dtype(0.0 if use_all else r1) * np.eye(o2, dtype=dtype)
    lam, W = np.linalg.eigh(M)
    lt = np.maximum(lam, dtype(0.0 if use_all else eps))
    idx = np.argsort(-lt, kind="stable")[:(o2 if use_all else k)]
    loss = -np.sqrt(lt[idx]).sum(dtype=dtype)
    ok = lam[idx] > eps
    wgt = np.where(ok, 0.5 / np.sqrt(np.where(ok, lam[idx], 1)), 0).astype(dtype)
    GM = (W[:, idx] * wgt) @ W[:, idx].T
    GT = 2 * T @ GM
    G12 = A @ GT @ B
    GA, GB = GT @ (S12 @ B).T, (A @ S12).T @ GT
    G11, G22 = _back(GA, d1, V1, k1, f1), _back(GB, d2, V2, k2, f2)
    dH1 = c * (2 * G11 @ H1 + G12 @ H2)
    dH2 = c * (2 * G22 @ H2 + G12.T @ H1)
    return dtype(loss), (-dH1.T).astype(dtype), (-dH2.T).astype(dtype), np.linalg.svd(T, compute_uv=False)


def rel_l2(x, ref):
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(x - ref) / max(np.linalg.norm(ref), 1e-300))


def rel_abs(x, ref):
    return float(abs(float(x) - float(ref)) / max(abs(float(ref)), 1e-300))
