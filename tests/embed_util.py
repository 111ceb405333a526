"""NumPy restatements of the latent-space reductions (csrc/embed.hip, src/visualization/_embed.py): the five stages of exact
t-SNE as scikit-learn's ``method="exact"`` computes them, incremental PCA as ``IncrementalPCA(n_components=k).fit_transform``
computes it, and trustworthiness.  float64 by default; ``dtype=np.float32`` gives the rounding floor of the arithmetic the kernels
use (the ``self32/<name>`` entries of tests/golden/embed_*.npz).  Needs numpy only.

Also here: the seeded input recipes of the fixtures (tests/golden/make_embed_golden.py stores no inputs)."""
import numpy as np

MACHINE_EPSILON = float(np.finfo(np.double).eps)        # 2.220446e-16
PERPLEXITY_TOLERANCE = 1e-5
EPSILON_DBL = 1e-8
TSNE_CASES = {"a": (300, 64, 2, 64.0), "b": (400, 128, 3, 64.0), "c": (256, 32, 2, 30.0)}      # N, D, nc, perplexity
PCA_CASES = {"one": (200, 64), "multi": (1000, 64), "tail": (700, 48), "wide": (150, 1089), "flat": (600, 40)}   # N, D
TSNE_SEEDS = {"a": 7101, "b": 7102, "c": 7103}
PCA_SEEDS = {"one": 7201, "multi": 7202, "tail": 7203, "wide": 7204, "flat": 7205}


# ------------------------------------------------------------------------------------------------------------------ recipes
def clustered(N, D, seed, centres=4, spread=4.0):
    """`centres` Gaussian blobs (unit noise) around seeded centres of scale `spread`, as float32; labels = blob index % 2."""
    rng = np.random.default_rng(seed)
    c = rng.normal(size=(centres, D)) * spread / np.sqrt(D) * 4.0
    idx = rng.integers(0, centres, size=N)
    x = c[idx] + rng.normal(size=(N, D))
    return x.astype(np.float32), (idx % 2).astype(np.int64)


def decaying(N, D, seed):
    """Latents with a decaying spectrum and a non-zero, drifting mean (so that incremental batches see different means)."""
    rng = np.random.default_rng(seed)
    r = min(N, D, 24)
    s = 8.0 * 0.7 ** np.arange(r)
    z = rng.normal(size=(N, r)) * s
    z[:, 0] += np.linspace(-6.0, 6.0, N)                        # drift along the sample axis: batch means differ
    b = rng.normal(size=(r, D)) / np.sqrt(D)
    x = z @ b + 0.05 * rng.normal(size=(N, D)) + rng.normal(size=(1, D)) * 2.0
    return x.astype(np.float32)


def flat_tail(N, D, seed):
    """Three leading directions (8, 6, 4.5) over a flat tail of twelve at 4.0: sigma_9 / sigma_3 is about 0.9, so a subspace
    iteration on 8 columns converges slowly for the third component (several batches at N > 5 D)."""
    rng = np.random.default_rng(seed)
    s = np.array([8.0, 6.0, 4.5] + [4.0] * 12)
    q, _ = np.linalg.qr(rng.normal(size=(D, s.size)))
    u, _ = np.linalg.qr(rng.normal(size=(N, s.size)))
    x = (u * s * np.sqrt(N)) @ q.T + 0.01 * rng.normal(size=(N, D)) + rng.normal(size=(1, D))
    return x.astype(np.float32)


def pca_input(case):
    """The seeded latents of a case of PCA_CASES."""
    N, D = PCA_CASES[case]
    return (flat_tail if case == "flat" else decaying)(N, D, PCA_SEEDS[case])


def spread_y(N, nc, seed):
    """A spread-out embedding at which the objective and its gradient are recorded."""
    return (np.random.default_rng(seed).normal(size=(N, nc)) * 5.0).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ t-SNE stages
def sqdist(x, dtype=np.float64):
    """md_sqdist: squared Euclidean distances in the direct form sum_k (x_ik - x_jk)^2."""
    x = np.asarray(x, dtype=dtype)
    N = x.shape[0]
    out = np.empty((N, N), dtype=dtype)
    for i in range(N):
        d = x - x[i]
        out[i] = np.einsum("jk,jk->j", d, d)
    return out


def conditional(d2, perplexity, dtype=np.float64, rows=None):
    """md_tsne_conditional: sklearn.manifold._utils._binary_search_perplexity row by row (sums in float64, exp in `dtype`).
    With ``rows`` d2 holds only those rows of the distance matrix (len(rows), N) and only they are returned."""
    d2 = np.asarray(d2, dtype=np.float32)                      # scikit-learn hands float32 distances to the search
    N = d2.shape[1]
    target = np.log(perplexity)
    P = np.zeros(d2.shape, dtype=dtype)
    for r, i in enumerate(range(N) if rows is None else rows):
        d = np.delete(d2[r], i).astype(dtype)
        lo, hi, beta = -np.inf, np.inf, 1.0
        for _ in range(100):
            p = np.exp(-d * dtype(beta))
            s = float(np.sum(p, dtype=np.float64))
            if s == 0.0:
                s = EPSILON_DBL
            sdp = float(np.sum(d.astype(np.float64) * p, dtype=np.float64)) / s
            diff = np.log(s) + beta * sdp - target
            if abs(diff) <= PERPLEXITY_TOLERANCE:
                break
            if diff > 0.0:
                lo = beta
                beta = beta * 2.0 if hi == np.inf else (beta + hi) / 2.0
            else:
                hi = beta
                beta = beta / 2.0 if lo == -np.inf else (beta + lo) / 2.0
        row = (p / dtype(s)).astype(dtype)
        P[r, :i] = row[:i]
        P[r, i + 1:] = row[i:]
    return P


def joint(p_cond, dtype=np.float64):
    """md_tsne_joint: (C + C^T) / max(sum, eps), off-diagonal clamped to eps, diagonal 0."""
    c = np.asarray(p_cond, dtype=dtype)
    s = c + c.T
    tot = max(float(np.sum(s, dtype=np.float64)), MACHINE_EPSILON)
    P = np.maximum(s / dtype(tot), dtype(MACHINE_EPSILON)).astype(dtype)
    np.fill_diagonal(P, 0.0)
    return P


def joint_probabilities(x, perplexity, dtype=np.float64):
    return joint(conditional(sqdist(x, dtype), perplexity, dtype), dtype)


def kl_gradient(P, y, exaggeration=1.0, dtype=np.float64):
    """md_tsne_gradient: sklearn.manifold._t_sne._kl_divergence on the full matrix -> (kl, grad (N, nc), Z)."""
    P = np.asarray(P, dtype=dtype) * dtype(exaggeration)
    y = np.asarray(y, dtype=dtype)
    N, nc = y.shape
    dof = max(nc - 1, 1)
    d = sqdist(y, dtype)
    num = (dtype(1.0) + d / dtype(dof)) ** dtype(-(dof + 1.0) / 2.0)
    np.fill_diagonal(num, 0.0)
    Z = float(np.sum(num, dtype=np.float64))
    Q = np.maximum(num / dtype(Z), dtype(MACHINE_EPSILON))
    off = ~np.eye(N, dtype=bool)
    kl = float(np.sum(P[off] * np.log(np.maximum(P[off], dtype(MACHINE_EPSILON)) / Q[off]), dtype=np.float64))
    pn, nn = P * num, num * num
    grad = np.empty((N, nc), dtype=dtype)
    for c in range(nc):                                        # attractive and repulsive sums apart, accumulated in `dtype`
        diff = y[:, None, c] - y[None, :, c]
        grad[:, c] = np.sum(pn * diff, axis=1) - np.sum(nn * diff, axis=1) / dtype(Z)
    return kl, (dtype(2.0 * (dof + 1.0) / dof) * grad).astype(dtype), Z


def update(y, upd, gains, grad, momentum, lr, min_gain=0.01, dtype=np.float64):
    """md_tsne_update: one step of _gradient_descent -> (y, update, gains, |gains * grad|^2)."""
    y, upd, gains, grad = (np.array(a, dtype=dtype) for a in (y, upd, gains, grad))
    inc = upd * grad < 0.0
    gains = np.where(inc, gains + dtype(0.2), gains * dtype(0.8))
    gains = np.maximum(gains, dtype(min_gain))
    g = grad * gains
    upd = dtype(momentum) * upd - dtype(lr) * g
    return y + upd, upd, gains, float(np.sum(g.astype(np.float64) ** 2))


def descend(P, y0, steps, exaggeration, momentum, lr, dtype=np.float64):
    """`steps` iterations from y0 with fresh update / gains; the list of Y after each step."""
    y = np.asarray(y0, dtype=dtype)
    upd, gains = np.zeros_like(y), np.ones_like(y)
    out = []
    for _ in range(steps):
        _, g, _ = kl_gradient(P, y, exaggeration, dtype)
        y, upd, gains, _ = update(y, upd, gains, g, momentum, lr, dtype=dtype)
        out.append(y.copy())
    return out


def auto_learning_rate(N, early_exaggeration=12.0):
    return max(N / early_exaggeration / 4.0, 50.0)


# ------------------------------------------------------------------------------------------------------------------ PCA
def gen_batches(n, batch_size, min_batch_size=0):
    """sklearn.utils.gen_batches as (start, stop) pairs: a tail shorter than min_batch_size joins the previous batch."""
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


def flip_rows(vt):
    """svd_flip(u_based_decision=False): the largest-magnitude entry of every row positive."""
    vt = np.array(vt)
    j = np.argmax(np.abs(vt), axis=1)
    s = np.sign(vt[np.arange(vt.shape[0]), j])
    s[s == 0] = 1
    return vt * s[:, None], s


def incremental_pca(x, k, dtype=np.float64):
    """IncrementalPCA(n_components=k).fit_transform(x) -> (embedding (N, k), components (k, D), singular values, mean)."""
    x = np.asarray(x, dtype=dtype)
    N, D = x.shape
    mean = np.zeros(D, dtype=np.float64)
    comp = sv = None
    seen = 0
    for a, b in gen_batches(N, 5 * D, min_batch_size=k):
        xb = x[a:b]
        nb = b - a
        bmean = np.sum(xb, axis=0, dtype=np.float64) / nb
        new_mean = (mean * seen + bmean * nb) / (seen + nb)
        m = (xb - bmean.astype(dtype)).astype(dtype)
        if seen:
            corr = np.sqrt(seen * nb / (seen + nb)) * (mean - bmean)
            m = np.vstack([(sv[:, None] * comp).astype(dtype), m, corr[None].astype(dtype)])
        _, s, vt = np.linalg.svd(m, full_matrices=False)
        vt, _ = flip_rows(vt)
        comp, sv, mean = vt[:k], s[:k], new_mean
        seen += nb
    emb = (x - mean.astype(dtype)) @ comp.T
    return emb.astype(dtype), comp, sv, mean


def pca_init(x, nc, dtype=np.float64):
    """The deterministic t-SNE start: first nc components of an exact PCA, column 0 scaled to standard deviation 1e-4."""
    x = np.asarray(x, dtype=dtype)
    m = x - np.mean(x, axis=0, dtype=np.float64).astype(dtype)
    _, _, vt = np.linalg.svd(m, full_matrices=False)
    vt, _ = flip_rows(vt)
    e = m @ vt[:nc].T
    return (e / np.std(e[:, 0]) * 1e-4).astype(dtype)


# ------------------------------------------------------------------------------------------------------------------ quality
def trustworthiness(x, y, n_neighbors=10):
    """sklearn.manifold.trustworthiness(x, y, n_neighbors) with the Euclidean metric."""
    dx = sqdist(x)
    np.fill_diagonal(dx, np.inf)
    ind_x = np.argsort(dx, axis=1, kind="stable")
    dy = sqdist(y)
    np.fill_diagonal(dy, np.inf)
    ind_y = np.argsort(dy, axis=1, kind="stable")[:, :n_neighbors]
    N = dx.shape[0]
    rank = np.zeros((N, N), dtype=np.int64)
    rank[np.arange(N)[:, None], ind_x] = np.arange(1, N + 1)
    r = rank[np.arange(N)[:, None], ind_y] - n_neighbors
    t = float(np.sum(r[r > 0]))
    return 1.0 - t * (2.0 / (N * n_neighbors * (2.0 * N - 3.0 * n_neighbors - 1.0)))


def tsne_kl(x, y, perplexity):
    """KL(P || Q) of an embedding on the exact P of the inputs, all in float64."""
    return kl_gradient(joint_probabilities(x, perplexity), y, 1.0)[0]


def range_dev(a, b):
    """max|a - b| / (max b - min b)."""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b))) / float(np.max(b) - np.min(b))


def max_dev(a, b):
    """max|a - b| / max|b|."""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b))) / (float(np.max(np.abs(b))) or 1.0)


def l2_dev(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))
