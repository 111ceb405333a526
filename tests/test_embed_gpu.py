"""GPU tests of the latent-space maps (csrc/embed.hip, src/visualization/_embed.py, visualize_latent_space.py).

Every comparison is against a recording of tests/golden/embed_*.npz or against the float64 restatements of tests/embed_util.py
(which tests/test_embed_cpu.py pins to the recordings at 1e-15 ... 4e-7), never against another run of the code under test.  Bar of a
kernel stage: 10 x the recorded ``self32`` figure (the deviation of the restatement run in float32; the factor covers the different
summation order of a tiled kernel).  Whole t-SNE runs: the reference's own run-to-run spread over its five recorded runs.

Measured on an MI355X (deviation / bar): see DESIGN section 11.
"""
import math
import os

import numpy as np
import pytest
import torch

from tests import embed_util as eu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS32 = 2.0 ** -24


@pytest.fixture(scope="module")
def tsne(golden_dir):
    return np.load(os.path.join(golden_dir, "embed_tsne.npz"))


@pytest.fixture(scope="module")
def pca(golden_dir):
    return np.load(os.path.join(golden_dir, "embed_pca.npz"))


_CACHE = {}


def case_data(case):
    """(x float32, exact P float64) of a t-SNE case; P by the float64 restatement (equal to scikit-learn's to 1e-15, CPU test)."""
    if case not in _CACHE:
        N, D, nc, perp = eu.TSNE_CASES[case]
        x = eu.clustered(N, D, eu.TSNE_SEEDS[case])[0]
        _CACHE[case] = (x, eu.joint_probabilities(x, perp))
    return _CACHE[case]


def cuda(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV).contiguous()


# ---------------------------------------------------------------------------------------------------------- distances
def sqdist_bar(D):
    """Direct form in fp32: a difference is rounded once (2^-24 relative, so 2^-23 in its square), the square once, and D positive
    terms are added one after the other (at most D 2^-24 relative): (D + 4) 2^-24 of the distance itself."""
    return (D + 4) * EPS32


@pytest.mark.parametrize("case", sorted(eu.TSNE_CASES))
def test_sqdist_matches_float64(case):
    from src.visualization import _embed
    x, _ = case_data(case)
    d = _embed.sqdist(cuda(x)).cpu().numpy()
    ref = eu.sqdist(x)
    off = ~np.eye(len(x), dtype=bool)
    dev = float(np.max(np.abs(d[off] - ref[off]) / ref[off]))
    print(case, "sqdist max relative deviation", dev, "bar", sqdist_bar(x.shape[1]))
    assert dev <= sqdist_bar(x.shape[1])
    assert np.array_equal(d, d.T) and not np.diag(d).any()


def test_sqdist_keeps_small_distances():
    from src.visualization import _embed
    rng = np.random.default_rng(11)
    x = (rng.normal(size=(70, 37)) + 10.0).astype(np.float32)
    x[5] = x[4]                                                    # two identical rows
    x[9] = x[8] + np.float32(1e-4)                                 # two rows 1e-4 apart at |x| ~ 10
    d = _embed.sqdist(cuda(x)).cpu().numpy()
    ref = eu.sqdist(x)                                             # float64 distances of the float32 rows
    assert d[4, 5] == 0.0 and d[5, 4] == 0.0
    assert ref[8, 9] < 1e-6                                        # 37 (1e-4)^2 ~ 4e-7 against |x|^2 ~ 3700: the expanded form loses it
    print("near rows:", d[8, 9], "float64", ref[8, 9])
    assert abs(d[8, 9] - ref[8, 9]) <= sqdist_bar(37) * ref[8, 9]
    off = ref > 0
    assert float(np.max(np.abs(d[off] - ref[off]) / ref[off])) <= sqdist_bar(37)
    assert np.array_equal(d, d.T)


# ---------------------------------------------------------------------------------------------------------- P
@pytest.mark.parametrize("case", sorted(eu.TSNE_CASES))
def test_joint_p_matches_scikit_learn(tsne, case):
    from src.visualization import _embed
    N, D, nc, perp = eu.TSNE_CASES[case]
    x, _ = case_data(case)
    P = _embed.joint_probabilities(cuda(x), perp).cpu().numpy().astype(np.float64)
    pmax = float(tsne["Pmax/" + case])
    if "P/" + case in tsne.files:
        rec, mine, key = tsne["P/" + case], P, "P/" + case
    else:
        rec, mine, key = tsne["Prows/" + case], P[tsne["Pidx/" + case]], "Prows/" + case
    bar = 10.0 * float(tsne["self32/" + key])
    dev = float(np.max(np.abs(mine - rec))) / pmax
    sdev = float(np.max(np.abs(P.sum(1) - tsne["Psum/" + case])))
    print(case, "P deviation / max P", dev, "bar", bar, "| row sums", sdev, "bar", N * bar * pmax)
    assert dev <= bar
    assert sdev <= N * bar * pmax                                  # N entries, each within the bar
    assert np.array_equal(P, P.T) and not np.diag(P).any()
    assert abs(P.sum() - 1.0) <= 1e-6


# ---------------------------------------------------------------------------------------------------------- gradient, update
@pytest.mark.parametrize("case", sorted(eu.TSNE_CASES))
@pytest.mark.parametrize("ex", [1, 12])
def test_kl_and_gradient_match_scikit_learn(tsne, case, ex):
    from src.visualization import _embed
    N, D, nc, perp = eu.TSNE_CASES[case]
    _, P = case_data(case)
    y = eu.spread_y(N, nc, eu.TSNE_SEEDS[case] + 50)
    d = _embed._Descent(cuda(P), cuda(y))
    d.gradient(float(ex), True)
    stats = d.stats.cpu().numpy()
    grad = d.grad.cpu().numpy()
    rk, rg = float(tsne["kl%d/%s" % (ex, case)]), tsne["grad%d/%s" % (ex, case)]
    kdev, gdev = abs(stats[1] - rk) / abs(rk), eu.l2_dev(grad, rg)
    kbar, gbar = 10.0 * float(tsne["self32/kl%d/%s" % (ex, case)]), 10.0 * float(tsne["self32/grad%d/%s" % (ex, case)])
    print(case, "exaggeration", ex, "KL relative deviation", kdev, "bar", kbar, "| gradient relative L2", gdev, "bar", gbar)
    assert math.isfinite(stats[1]) and abs(stats[2] - ex) <= 1e-5 * ex        # sum of the exaggerated P
    assert kdev <= kbar
    assert gdev <= gbar
    d.gradient(float(ex), False)                                   # the variant without the KL terms computes the same gradient
    assert torch.equal(d.grad.cpu(), torch.from_numpy(grad))


@pytest.mark.parametrize("nc", [2, 3])
def test_kl_and_gradient_across_several_lds_tiles(nc):
    """N = 1500: two LDS tiles of embedding points per row, the second one partial.  Reference: the float64 restatement (equal to
    scikit-learn's _kl_divergence to 1e-15, CPU test); bar: 10 x the deviation of the same restatement run in float32, as for the
    recorded cases."""
    from src.visualization import _embed
    N = 1500
    x, _ = eu.clustered(N, 16, 7401)
    P = eu.joint_probabilities(x, 40.0)
    y = eu.spread_y(N, nc, 7402 + nc)
    for ex in (1.0, 12.0):
        kl, grad, Z = eu.kl_gradient(P, y, ex)
        kl32, grad32, _ = eu.kl_gradient(P.astype(np.float32), y, ex, np.float32)
        kbar, gbar = 10.0 * abs(kl32 - kl) / abs(kl), 10.0 * eu.l2_dev(grad32, grad)
        d = _embed._Descent(cuda(P), cuda(y))
        d.gradient(ex, True)
        stats = d.stats.cpu().numpy()
        kdev, gdev = abs(stats[1] - kl) / abs(kl), eu.l2_dev(d.grad.cpu().numpy(), grad)
        print("N = 1500, nc", nc, "exaggeration", ex, "KL", kdev, "bar", kbar, "| gradient", gdev, "bar", gbar, "| Z", abs(stats[0] - Z) / Z)
        assert kdev <= kbar and gdev <= gbar
        assert abs(stats[0] - Z) / Z <= 10.0 * EPS32                # num in float32, its sum in float64


def test_conditional_p_with_the_row_above_48_kib_of_lds():
    """N = 12800 (> 12288): the row needs more dynamic LDS than the default limit.  Checked by what the bisection guarantees, on
    every row for the sum and on sampled rows for the entropy: a row sums to 1, its diagonal is 0, and its entropy is within the
    search tolerance 1e-5 of ln(perplexity) -- plus 2e-6 for probabilities rounded to float32 (2^-24 (H + 1) each way, H = ln 64)."""
    from src import _native
    from src.ops import _p, _stream
    N, perp = 12800, 64.0
    gen = torch.Generator(device=DEV).manual_seed(3)
    d2 = torch.rand((N, N), device=DEV, generator=gen) * 30.0
    rows = [0, 1, 255, 256, 6399, 12287, 12288, 12799]
    keep = d2[rows].cpu().numpy()
    _native.check(_native.lib().md_tsne_conditional(_p(d2), N, perp, _p(d2), _stream()), "md_tsne_conditional")      # in place
    sums = d2.double().sum(1).cpu().numpy()
    assert float(np.max(np.abs(sums - 1.0))) <= 1e-6 and not bool(d2.diagonal().any())
    got = d2[rows].double().cpu().numpy()
    want = eu.conditional(keep, perp, rows=rows)
    for r, g, w in zip(rows, got, want):
        nz = g[g > 0]
        H = float(-np.sum(nz * np.log(nz)))
        print("row", r, "entropy - ln(perplexity)", H - math.log(perp), "| deviation from the float64 search / max p", float(np.max(np.abs(g - w))) / w.max())
        assert abs(H - math.log(perp)) <= 1e-5 + 2e-6


@pytest.mark.parametrize("case", sorted(eu.TSNE_CASES))
def test_descent_matches_scikit_learn_after_1_and_5_steps(tsne, case):
    from src.visualization import _embed
    N, D, nc, perp = eu.TSNE_CASES[case]
    _, P = case_data(case)
    y = cuda(tsne["y0/" + case])
    d = _embed._Descent(cuda(P), y)
    upd, gains = torch.zeros_like(y), torch.ones_like(y)
    lr = eu.auto_learning_rate(N)
    for step in range(1, 6):
        d.gradient(12.0, False)
        d.update(upd, gains, 0.5, lr)
        if step in (1, 5):
            rec = tsne["y%d/%s" % (step, case)]
            dev, bar = eu.max_dev(y.cpu().numpy(), rec), 10.0 * float(tsne["self32/y%d/%s" % (step, case)])
            print(case, step, "steps: deviation / max|Y|", dev, "bar", bar)
            assert dev <= bar
    g = (d.grad * gains).double().cpu().numpy()
    assert abs(float(d.gpart.sum().cpu()) - float(np.sum(g * g))) <= 1e-6 * float(np.sum(g * g))


# ---------------------------------------------------------------------------------------------------------- PCA
@pytest.mark.parametrize("case", sorted(eu.PCA_CASES))
@pytest.mark.parametrize("k", [2, 3])
def test_pca_matches_the_reference(pca, case, k):
    from src.visualization import _embed
    N, D = eu.PCA_CASES[case]
    emb = _embed.pca_embed(cuda(eu.pca_input(case)), k).cpu().numpy()
    key = "emb%d/%s" % (k, case)
    dev, bar = eu.range_dev(emb, pca[key]), 10.0 * float(pca["self32/" + key])
    print(key, "deviation / range (signs included)", dev, "bar", bar)
    assert emb.shape == (N, k) and emb.dtype == np.float32
    assert dev <= bar


def test_pca_matches_the_reference_multi_form(pca):
    from src.visualization import _embed
    vis, x0 = eu.decaying(700, 48, 7211), eu.decaying(700, 16, 7212)
    for name, x in (("fusion", np.concatenate([vis, x0], 1)), ("vis", vis), ("0D", x0)):
        dev = eu.range_dev(_embed.pca_embed(cuda(x), 2).cpu().numpy(), pca["multi/" + name])
        print("multi", name, dev, "bar", 10.0 * float(pca["self32/multi/" + name]))
        assert dev <= 10.0 * float(pca["self32/multi/" + name])


def test_col_mean_and_tall_skinny_products():
    from src.visualization import _embed
    rng = np.random.default_rng(5)
    M = (rng.normal(size=(531, 203)) + 3.0).astype(np.float32)
    extra = rng.normal(size=(3, 203)).astype(np.float32)
    V = rng.normal(size=(203, 8)).astype(np.float32)
    mean = _embed.col_mean(cuda(M))
    ref_mean = M.astype(np.float64).mean(0)
    assert float(np.max(np.abs(mean.cpu().numpy() - ref_mean))) <= 1e-12 * 4.0       # fp64 sums of 531 float32 values
    mu = mean.float()
    S = np.vstack([(M - mu.cpu().numpy()).astype(np.float64), extra.astype(np.float64)])
    W = _embed.tsmm_mv(cuda(M), mu, cuda(extra), cuda(V))
    ref_w = S @ V.astype(np.float64)
    assert eu.max_dev(W.cpu().numpy(), ref_w) <= 2 * EPS32                            # fp64 accumulation, one rounding to float32
    Z = _embed.tsmm_mtw(cuda(M), mu, cuda(extra), W, f64=True)
    assert eu.max_dev(Z.cpu().numpy(), S.T @ W.double().cpu().numpy()) <= 1e-12
    Zf = _embed.tsmm_mtw(cuda(M), mu, cuda(extra), W)
    assert torch.equal(Zf, Z.float())


# ---------------------------------------------------------------------------------------------------------- whole t-SNE
@pytest.mark.parametrize("case", sorted(eu.TSNE_CASES))
def test_tsne_embed_reaches_the_reference_quality(tsne, case):
    from src.visualization import _embed
    N, D, nc, perp = eu.TSNE_CASES[case]
    x, P = case_data(case)
    y, res = _embed.tsne_embed(cuda(x), nc, perplexity=perp)
    y2, res2 = _embed.tsne_embed(cuda(x), nc, perplexity=perp)
    emb = y.cpu().numpy().astype(np.float64)
    kl = eu.kl_gradient(P, emb, 1.0)[0]
    trust = eu.trustworthiness(x, emb, 10)
    kr, tr = tsne["kl_ref/" + case], tsne["trust_ref/" + case]
    kl_bar, trust_bar = kr.max() + (kr.max() - kr.min()), tr.min() - (tr.max() - tr.min())
    print(case, "n_iter", res.n_iter, "reported KL", res.kl_divergence, "KL on the exact P", kl, "bar", kl_bar, "reference runs", kr.min(),
          kr.max(), "| trustworthiness", trust, "bar", trust_bar, "reference runs", tr.min(), tr.max())
    assert y.shape == (N, nc) and y.dtype == torch.float32 and y.is_cuda
    assert 250 <= res.n_iter <= 999 and math.isfinite(res.kl_divergence) and np.isfinite(emb).all()
    assert kl <= kl_bar
    assert trust >= trust_bar
    assert torch.equal(y, y2) and res.kl_divergence == res2.kl_divergence and res.n_iter == res2.n_iter


def test_tsne_embed_larger_run_syncs_once_per_checkpoint(monkeypatch):
    from src.visualization import _embed
    x, _ = eu.clustered(4096, 128, 7301)
    xc = cuda(x)
    y0 = _embed.pca_init(xc, 2)                                    # the start is computed outside the counted region
    reads = []
    real = _embed._readback
    monkeypatch.setattr(_embed, "_readback", lambda t: (reads.append(1), real(t))[1])
    y, res = _embed.tsne_embed(xc, 2, perplexity=30.0, max_iter=500, init=y0)
    errs = dict((it, e) for it, e, _ in res.history)
    print("N = 4096: n_iter", res.n_iter, "read-backs", len(reads), "error at 300", errs.get(300), "at 500", errs.get(500))
    assert res.n_iter == 499 and bool(torch.isfinite(y).all())
    assert errs[500] < errs[300]
    assert len(reads) <= 500 // 50


# ---------------------------------------------------------------------------------------------------------- end to end
def pca_bar(x, k):
    """Embedding deviation allowed for float32 operands: 100 eps32 sigma_1 / (smallest gap among sigma_1 .. sigma_(k+1)) of the
    float64 restatement (the sensitivity of a singular vector to a perturbation of relative size eps32), at least 1e-5."""
    s = np.linalg.svd(x.astype(np.float64) - x.astype(np.float64).mean(0), compute_uv=False)
    gap = np.min(s[:k] - s[1:k + 1])
    return max(100.0 * EPS32 * s[0] / gap, 1e-5)


def loader_of(xs, labels, batch):
    return [(xs[i:i + batch], labels[i:i + batch]) for i in range(0, len(labels), batch)]


def test_r2plus1d_end_to_end(tmp_path):
    from src.models.R2Plus1D import R2Plus1DClassifier
    from src.visualization import _embed
    from src.visualization.visualize_latent_space import visualize_2D_latent_space, visualize_3D_latent_space
    torch.manual_seed(3)
    m = R2Plus1DClassifier(input_size=(3, 5, 24, 24), num_classes=2, layer_sizes=[1, 1, 1, 1], alpha=0.01)
    x = torch.randn(24, 3, 5, 24, 24) * 40.0
    lab = torch.arange(24) % 2
    ld = loader_of(x, lab, 6)
    emb, label = visualize_3D_latent_space(m, ld, device=DEV, save_dir=None, limit_iters=2, method="PCA")
    assert emb.shape == (18, 3) and np.array_equal(label, lab[:18].numpy())       # limit_iters = 2 consumes three batches
    lat, _ = _embed.collect_latents(m, ld, DEV, 2)
    assert lat.is_cuda and lat.shape[0] == 18
    with torch.no_grad():
        for i in range(3):
            assert torch.equal(lat[6 * i:6 * i + 6], m.encode(x[6 * i:6 * i + 6].to(DEV)).reshape(6, -1))
    ref = eu.incremental_pca(lat.cpu().numpy(), 3)[0]
    print("R(2+1)D latents", tuple(lat.shape), "PCA deviation / range", eu.range_dev(emb, ref), "bar", pca_bar(lat.cpu().numpy(), 3))
    assert eu.range_dev(emb, ref) <= pca_bar(lat.cpu().numpy(), 3)
    emb_all, label_all = visualize_2D_latent_space(m, ld, device=DEV, save_dir=None, limit_iters=-1, method="PCA")
    assert emb_all.shape == (24, 2) and np.array_equal(label_all, lab.numpy())
    assert not list(tmp_path.iterdir())                              # save_dir=None draws nothing
    with pytest.raises(ValueError):                                  # the reference's perplexity 64 on 24 rows, as scikit-learn
        visualize_2D_latent_space(m, ld, device=DEV, save_dir=None, limit_iters=-1, method="tSNE")


def transformer_case():
    from src.models.transformer import Transformer
    torch.manual_seed(9)
    m = Transformer(n_features=18, kernel_size=5, feature_dims=64, max_len=21, n_layers=2, n_heads=4, dim_feedforward=96, dropout=0.3,
                    cls_dims=32, n_classes=2)
    x = torch.randn(80, 21, 18)
    lab = torch.arange(80) % 2
    return m, x, lab, loader_of(x, lab, 20)


def test_transformer0d_end_to_end():
    from src.visualization.visualize_latent_space import visualize_2D_decision_boundary, visualize_2D_latent_space
    m, x, lab, ld = transformer_case()
    emb, label = visualize_2D_latent_space(m, ld, device=DEV, save_dir=None, limit_iters=-1, method="PCA")
    with torch.no_grad():
        lat = torch.cat([m.encode(b.to(DEV)).reshape(len(b), -1) for b, _ in ld], 0).cpu().numpy()
    print("Transformer latents", lat.shape, "PCA deviation / range", eu.range_dev(emb, eu.incremental_pca(lat, 2)[0]), "bar", pca_bar(lat, 2))
    assert emb.shape == (80, 2) and eu.range_dev(emb, eu.incremental_pca(lat, 2)[0]) <= pca_bar(lat, 2)
    emb_b, label_b, probs = visualize_2D_decision_boundary(m, ld, device=DEV, save_dir=None, limit_iters=1, method="PCA")
    with torch.no_grad():
        want = torch.softmax(m(x[:40].to(DEV)), dim=1)[:, 0].cpu().numpy()
    assert emb_b.shape == (40, 2) and np.array_equal(label_b, lab[:40].numpy())
    assert float(np.max(np.abs(probs - want))) <= 1e-5


class Reshuffling:
    """A loader that, like a DataLoader with a random sampler, yields another order every time it is iterated.  The label of a
    window is its index, so a result row can be traced back to its input."""

    def __init__(self, x, batch, seed):
        self.x, self.batch, self.gen, self.passes = x, batch, torch.Generator().manual_seed(seed), 0

    def __iter__(self):
        self.passes += 1
        perm = torch.randperm(len(self.x), generator=self.gen)
        for i in range(0, len(perm), self.batch):
            idx = perm[i:i + self.batch]
            yield self.x[idx], idx


def test_decision_boundary_probabilities_belong_to_the_embedded_windows():
    """Probabilities, labels and latents of the decision-boundary map come from one pass over the loader: with a loader that
    reshuffles on every iteration probs[i] is softmax(model(x_i))[0] of the very window whose latent is row i.  Bar 1e-5 absolute
    on a probability: float32 forward of the same window inside another batch (a wrong pairing differs in the first or second digit)."""
    from src.visualization import _embed
    from src.visualization.visualize_latent_space import visualize_2D_decision_boundary
    m, x, _, _ = transformer_case()
    ld = Reshuffling(x, 20, 5)
    emb, label, probs = visualize_2D_decision_boundary(m, ld, device=DEV, save_dir=None, limit_iters=2, method="PCA")
    assert ld.passes == 1                                              # the loader is walked once
    assert emb.shape == (60, 2) and len(set(label.tolist())) == 60    # limit_iters = 2: three batches of distinct windows
    assert not np.array_equal(label, np.arange(60))                    # the order really is a shuffled one
    with torch.no_grad():
        xs = x[torch.from_numpy(label)].to(DEV)
        want = torch.softmax(m(xs), dim=1)[:, 0].cpu().numpy()
        lat = m.encode(xs).reshape(60, -1).cpu().numpy()
    spread = float(want.max() - want.min())
    print("decision boundary: max |probs - softmax(model(x_label))|", float(np.max(np.abs(probs - want))), "spread of probs", spread)
    assert spread > 1e-3                                               # the check can tell windows apart
    assert float(np.max(np.abs(probs - want))) <= 1e-5
    assert eu.range_dev(emb, eu.incremental_pca(lat, 2)[0]) <= pca_bar(lat, 2)
    lat2, label2, probs2 = _embed.collect_latents(m, ld, DEV, -1, with_probs=True)
    assert ld.passes == 2 and lat2.shape[0] == 80 and probs2.shape == (80,) and sorted(label2.tolist()) == list(range(80))


# ---------------------------------------------------------------------------------------------------------- drawing
def test_single_model_maps_are_drawn(tmp_path):
    pytest.importorskip("matplotlib").use("Agg")
    from src.visualization.visualize_latent_space import visualize_2D_latent_space, visualize_3D_latent_space
    m, x, lab, ld = transformer_case()
    for name, fn, nc in (("latent2d.png", visualize_2D_latent_space, 2), ("latent3d.png", visualize_3D_latent_space, 3)):
        emb0, _ = fn(m, ld, device=DEV, save_dir=None, limit_iters=-1, method="PCA")
        out = tmp_path / name
        emb, label = fn(m, ld, device=DEV, save_dir=str(out), limit_iters=-1, method="PCA")
        assert out.exists() and out.stat().st_size > 1000
        assert emb.shape == (80, nc) and np.array_equal(emb, emb0) and np.array_equal(label, lab.numpy())


def test_decision_boundary_is_drawn(tmp_path):
    pytest.importorskip("matplotlib").use("Agg")
    pytest.importorskip("scipy")
    from src.visualization.visualize_latent_space import visualize_2D_decision_boundary
    m, x, lab, ld = transformer_case()
    out = tmp_path / "boundary.png"
    emb, label, probs = visualize_2D_decision_boundary(m, ld, device=DEV, save_dir=str(out), limit_iters=-1, method="PCA")
    assert out.exists() and out.stat().st_size > 1000
    assert emb.shape == (80, 2) and probs.shape == (80,) and np.array_equal(label, lab.numpy())


def multimodal_case():
    from src.models.MultiModal import MultiModalModel
    torch.manual_seed(4)
    av = dict(image_size=32, patch_size=8, n_frames=5, dim=16, depth=1, n_heads=2, in_channels=3, d_head=8, dropout=0.0,
              embedd_dropout=0.0, scale_dim=2, pool="mean")
    a0 = dict(n_features=6, kernel_size=3, feature_dims=16, max_len=5, n_layers=1, n_heads=2, dim_feedforward=24, dropout=0.0)
    m = MultiModalModel(2, av, a0)
    xv, x0 = torch.randn(40, 3, 5, 32, 32), torch.randn(40, 5, 6)
    lab = torch.arange(40) % 2
    return m, xv, x0, lab, [({"video": xv[i:i + 8], "0D": x0[i:i + 8]}, lab[i:i + 8]) for i in range(0, 40, 8)]


def test_multi_maps_are_drawn(tmp_path):
    pytest.importorskip("matplotlib").use("Agg")
    from src.visualization.visualize_latent_space import visualize_2D_latent_space_multi, visualize_3D_latent_space_multi
    m, xv, x0, lab, ld = multimodal_case()
    for name, fn, nc in (("multi2d.png", visualize_2D_latent_space_multi, 2), ("multi3d.png", visualize_3D_latent_space_multi, 3)):
        out = tmp_path / name
        embs, label = fn(m, ld, device=DEV, save_dir=str(out), limit_iters=-1, method="PCA")
        assert out.exists() and out.stat().st_size > 1000
        assert len(embs) == 3 and all(e.shape == (40, nc) for e in embs) and np.array_equal(label, lab.numpy())


def test_multimodal_end_to_end():
    from src.visualization import _embed
    from src.visualization.visualize_latent_space import visualize_2D_latent_space_multi
    m, xv, x0, lab, ld = multimodal_case()
    embs, label = visualize_2D_latent_space_multi(m, ld, device=DEV, save_dir=None, limit_iters=3, method="PCA")
    assert len(embs) == 3 and all(e.shape == (32, 2) for e in embs) and np.array_equal(label, lab[:32].numpy())
    lats, _ = _embed.collect_latents(m, ld, DEV, 3, multi=True)
    with torch.no_grad():
        first = m.encode(xv[:8].to(DEV), x0[:8].to(DEV))
    for name, emb, lat, f in zip(("fused", "video", "0D"), embs, lats, first):
        assert torch.equal(lat[:8], f.reshape(8, -1))
        ln = lat.cpu().numpy()
        print(name, ln.shape, "PCA deviation / range", eu.range_dev(emb, eu.incremental_pca(ln, 2)[0]), "bar", pca_bar(ln, 2))
        assert eu.range_dev(emb, eu.incremental_pca(ln, 2)[0]) <= pca_bar(ln, 2)
