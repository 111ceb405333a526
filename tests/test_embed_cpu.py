"""CPU tests of the latent-space maps: the float64 restatements of tests/embed_util.py (what tests/test_embed_gpu.py compares the
kernels with) against the recordings of tests/golden/embed_*.npz (written by tests/golden/make_embed_golden.py from the reference's
functions and scikit-learn's exact helpers), the reference's loop-bound quirk, the argument checks of the engine, and the header
<-> binding <-> library check for the new symbols.

Bar of every comparison with a recording: 10 x the recorded ``self32`` figure (the deviation of the same restatement run in float32)
or 1e-6 relative, whichever is larger."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from src import _native
from tests import embed_util as eu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("md_sqdist", "md_tsne_conditional", "md_tsne_joint_scratch_doubles", "md_tsne_joint", "md_tsne_rowpart_floats",
               "md_tsne_scratch_doubles", "md_tsne_gradient", "md_tsne_update_blocks", "md_tsne_update", "md_col_mean_scratch_doubles",
               "md_col_mean", "md_tsmm_mv", "md_tsmm_mtw_scratch_doubles", "md_tsmm_mtw")


def bar(g, key):
    return max(10.0 * float(g["self32/" + key]), 1e-6)


@pytest.fixture(scope="module")
def tsne(golden_dir):
    return np.load(os.path.join(golden_dir, "embed_tsne.npz"))


@pytest.fixture(scope="module")
def pca(golden_dir):
    return np.load(os.path.join(golden_dir, "embed_pca.npz"))


_P = {}


def exact_p(case):
    if case not in _P:
        N, D, nc, perp = eu.TSNE_CASES[case]
        _P[case] = eu.joint_probabilities(eu.clustered(N, D, eu.TSNE_SEEDS[case])[0], perp)
    return _P[case]


# ---------------------------------------------------------------------------------------------------------- t-SNE restatements
@pytest.mark.parametrize("case", sorted(eu.TSNE_CASES))
def test_joint_probabilities_restatement_matches_scikit_learn(tsne, case):
    P = exact_p(case)
    pmax = float(tsne["Pmax/" + case])
    if "P/" + case in tsne.files:
        rec, mine, key = tsne["P/" + case], P, "P/" + case
    else:
        rec, mine, key = tsne["Prows/" + case], P[tsne["Pidx/" + case]], "Prows/" + case
    dev = float(np.max(np.abs(mine - rec))) / pmax
    print(case, "P deviation / max P", dev, "bar", bar(tsne, key))
    assert dev <= max(bar(tsne, key), 1e-6)                     # the recording is stored as float32: 6e-8 relative
    assert float(np.max(np.abs(P.sum(1) - tsne["Psum/" + case]))) <= 1e-6 * float(np.max(tsne["Psum/" + case]))
    assert np.array_equal(P, P.T) and not np.diag(P).any()


@pytest.mark.parametrize("case", sorted(eu.TSNE_CASES))
@pytest.mark.parametrize("ex", [1, 12])
def test_kl_and_gradient_restatement_matches_scikit_learn(tsne, case, ex):
    N, D, nc, perp = eu.TSNE_CASES[case]
    y = eu.spread_y(N, nc, eu.TSNE_SEEDS[case] + 50)
    kl, grad, _ = eu.kl_gradient(exact_p(case), y, float(ex))
    rk, rg = float(tsne["kl%d/%s" % (ex, case)]), tsne["grad%d/%s" % (ex, case)]
    print(case, ex, "kl", abs(kl - rk) / abs(rk), "grad", eu.l2_dev(grad, rg))
    assert abs(kl - rk) / abs(rk) <= bar(tsne, "kl%d/%s" % (ex, case))
    assert eu.l2_dev(grad, rg) <= bar(tsne, "grad%d/%s" % (ex, case))


@pytest.mark.parametrize("case", sorted(eu.TSNE_CASES))
def test_descent_restatement_matches_scikit_learn_after_1_and_5_steps(tsne, case):
    N, D, nc, perp = eu.TSNE_CASES[case]
    ys = eu.descend(exact_p(case), tsne["y0/" + case], 5, 12.0, 0.5, eu.auto_learning_rate(N))
    for steps in (1, 5):
        dev = eu.max_dev(ys[steps - 1], tsne["y%d/%s" % (steps, case)])
        print(case, steps, "steps: deviation / max|Y|", dev)
        assert dev <= bar(tsne, "y%d/%s" % (steps, case))


@pytest.mark.parametrize("case", sorted(eu.TSNE_CASES))
def test_pca_start_restatement(tsne, case):
    N, D, nc, perp = eu.TSNE_CASES[case]
    y0 = eu.pca_init(eu.clustered(N, D, eu.TSNE_SEEDS[case])[0], nc)
    assert eu.max_dev(y0, tsne["y0/" + case]) <= 1e-6
    assert abs(float(np.std(y0[:, 0])) - 1e-4) <= 1e-10


def test_reference_runs_are_recorded(tsne):
    for case in eu.TSNE_CASES:
        assert tsne["kl_ref/" + case].shape == (5,) and tsne["trust_ref/" + case].shape == (5,)
        assert np.all(tsne["kl_ref/" + case] > 0) and np.all(tsne["trust_ref/" + case] > 0.9)


def test_trustworthiness_restatement():
    x, _ = eu.clustered(120, 16, 5)
    assert eu.trustworthiness(x, x.astype(np.float64), 10) == 1.0
    y = np.random.default_rng(0).normal(size=(120, 2))
    assert 0.3 < eu.trustworthiness(x, y, 10) < 0.7              # an unrelated embedding: about one half


# ---------------------------------------------------------------------------------------------------------- PCA restatement
@pytest.mark.parametrize("case", sorted(eu.PCA_CASES))
@pytest.mark.parametrize("k", [2, 3])
def test_incremental_pca_restatement_matches_the_reference(pca, case, k):
    N, D = eu.PCA_CASES[case]
    emb = eu.incremental_pca(eu.pca_input(case), k)[0]
    key = "emb%d/%s" % (k, case)
    dev = eu.range_dev(emb, pca[key])
    print(key, "deviation / range", dev, "bar", bar(pca, key))
    assert dev <= bar(pca, key)


def test_incremental_pca_restatement_matches_the_reference_multi_form(pca):
    vis, x0 = eu.decaying(700, 48, 7211), eu.decaying(700, 16, 7212)
    for name, x in (("fusion", np.concatenate([vis, x0], 1)), ("vis", vis), ("0D", x0)):
        assert eu.range_dev(eu.incremental_pca(x, 2)[0], pca["multi/" + name]) <= bar(pca, "multi/" + name)


def test_batches_follow_scikit_learn():
    assert eu.gen_batches(700, 240, 2) == [(0, 240), (240, 480), (480, 700)]
    assert eu.gen_batches(481, 240, 2) == [(0, 240), (240, 481)]          # a 1-row tail joins the previous batch
    assert eu.gen_batches(200, 320, 2) == [(0, 200)]
    from src.visualization import _embed
    for args in ((700, 240, 2), (481, 240, 2), (200, 320, 3), (1000, 320, 3)):
        assert _embed.gen_batches(*args) == eu.gen_batches(*args)


# ---------------------------------------------------------------------------------------------------------- engine contract
class Identity(torch.nn.Module):
    def encode(self, x, x0=None):
        return x if x0 is None else (torch.cat([x, x0], 1), x, x0)


def test_limit_iters_keeps_the_reference_row_count(pca):
    from src.visualization import _embed
    x = torch.from_numpy(eu.decaying(60, 16, 7213))
    loader = [(x[i:i + 10], torch.arange(i, i + 10) % 2) for i in range(0, 60, 10)]
    for lim in (2, -1):
        lat, lab = _embed.collect_latents(Identity(), loader, "cpu", lim)
        assert lat.shape[0] == int(pca["rows/%d" % lim]) == lab.shape[0]
        assert torch.equal(lat, x[:lat.shape[0]])
    assert int(pca["rows/2"]) == 30 and int(pca["rows/-1"]) == 60      # limit_iters = n consumes n + 1 batches
    multi = [({"video": x[i:i + 10], "0D": x[i:i + 10, :4]}, torch.zeros(10)) for i in range(0, 60, 10)]
    (fused, vis, sig), lab = _embed.collect_latents(Identity(), multi, "cpu", 1, multi=True)
    assert fused.shape == (20, 20) and vis.shape == (20, 16) and sig.shape == (20, 4) and lab.dtype == torch.int64


def test_probabilities_are_taken_in_the_same_pass_as_the_latents():
    """A loader that reshuffles on every iteration (as the scripts' random samplers do): latent, label and probability of a row belong
    to one window, and the loader is walked once."""
    from src.visualization import _embed

    class Model(Identity):
        def forward(self, x):
            return x[:, :2] * 3.0

    class Reshuffling:
        def __init__(self, x):
            self.x, self.gen, self.passes = x, torch.Generator().manual_seed(1), 0

        def __iter__(self):
            self.passes += 1
            perm = torch.randperm(len(self.x), generator=self.gen)
            for i in range(0, len(perm), 10):
                yield self.x[perm[i:i + 10]], perm[i:i + 10]

    x = torch.from_numpy(eu.decaying(60, 16, 7213))
    ld = Reshuffling(x)
    lat, lab, probs = _embed.collect_latents(Model(), ld, "cpu", 2, with_probs=True)
    assert ld.passes == 1 and lat.shape == (30, 16) and probs.shape == (30,)
    assert torch.equal(lat, x[lab]) and torch.equal(probs, torch.softmax(x[lab][:, :2] * 3.0, dim=1)[:, 0])
    with pytest.raises(ValueError):
        _embed.collect_latents(Model(), ld, "cpu", 2, multi=True, with_probs=True)


def test_engine_rejects_bad_input_without_a_gpu():
    from src.visualization import _embed
    x = torch.randn(40, 8)
    with pytest.raises(ValueError):
        _embed.tsne_embed(x, 2, perplexity=40.0)                 # perplexity >= N, as scikit-learn
    with pytest.raises(ValueError):
        _embed.tsne_embed(x, 2, perplexity=64.0)
    with pytest.raises(RuntimeError):
        _embed.tsne_embed(x, 2, perplexity=10.0)                 # a CPU tensor: the path runs on the GPU only
    with pytest.raises(RuntimeError):
        _embed.pca_embed(x, 2)
    with pytest.raises(ValueError):
        _embed.pca_embed(x, 4)
    with pytest.raises(ValueError):
        _embed.tsne_embed(x, 1, perplexity=10.0)


def test_reference_names_and_defaults():
    from src.visualization import visualize_latent_space as v
    expect = {"visualize_2D_latent_space": "./results/latent_2d_space.png", "visualize_3D_latent_space": "./results/latent_2d_space.png",
              "visualize_2D_latent_space_multi": "./results/fusion_latent_3d_space.png",
              "visualize_3D_latent_space_multi": "./results/fusion_latent_3d_space.png",
              "visualize_2D_decision_boundary": "./results/decision_boundary_2D_space.png"}
    for name, save in expect.items():
        p = inspect.signature(getattr(v, name)).parameters
        assert list(p) == ["model", "dataloader", "device", "save_dir", "limit_iters", "method"], name
        assert (p["device"].default, p["save_dir"].default, p["limit_iters"].default, p["method"].default) == ("cpu", save, 2, "PCA")
    assert v.SINGLE_PERPLEXITY == 64.0 and v.MULTI_PERPLEXITY == 30.0


# ---------------------------------------------------------------------------------------------------------- ABI
def test_new_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mi355x_disrupt.h")).read()
    declared = set(re.findall(r"\b(md_[a-z0-9_]+)\s*\(", hdr))
    lib = _native.lib()
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in the header"
        assert name in _native.SIGNATURES, f"{name} has no ctypes prototype"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert "#define MD_EMBED_MAX_N 32768" in hdr


def test_embed_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _native.lib()
    a = C.c_void_p(64)                                             # a non-null pointer that is never dereferenced: every call is refused
    NULL, SHAPE, UNSUP = -5, -1, -2
    assert lib.md_sqdist(None, 4, 4, a, None) == NULL and lib.md_sqdist(a, 4, 4, None, None) == NULL
    assert lib.md_sqdist(a, 0, 4, a, None) == SHAPE and lib.md_sqdist(a, 4, 0, a, None) == SHAPE
    assert lib.md_sqdist(a, 32769, 4, a, None) == UNSUP
    assert lib.md_tsne_conditional(None, 4, 2.0, a, None) == NULL
    assert lib.md_tsne_conditional(a, -1, 2.0, a, None) == SHAPE and lib.md_tsne_conditional(a, 4, 0.0, a, None) == SHAPE
    assert lib.md_tsne_conditional(a, 40000, 2.0, a, None) == UNSUP
    assert lib.md_tsne_joint(a, 4, a, None, None) == NULL and lib.md_tsne_joint(a, 0, a, a, None) == SHAPE
    assert lib.md_tsne_joint(a, 32769, a, a, None) == UNSUP
    assert lib.md_tsne_gradient(a, a, 4, 2, 1.0, 0, a, a, None, a, None) == NULL
    assert lib.md_tsne_gradient(a, a, 0, 2, 1.0, 0, a, a, a, a, None) == SHAPE
    for nc in (1, 4):
        assert lib.md_tsne_gradient(a, a, 4, nc, 1.0, 0, a, a, a, a, None) == UNSUP
    assert lib.md_tsne_gradient(a, a, 32769, 2, 1.0, 0, a, a, a, a, None) == UNSUP
    assert lib.md_tsne_update(a, a, None, a, 8, 0.5, 50.0, 0.01, a, None) == NULL
    assert lib.md_tsne_update(a, a, a, a, 0, 0.5, 50.0, 0.01, a, None) == SHAPE
    assert lib.md_col_mean(None, 4, 4, a, a, None) == NULL and lib.md_col_mean(a, 0, 4, a, a, None) == SHAPE
    assert lib.md_tsmm_mv(a, 4, 4, None, None, 0, None, a, None) == NULL
    assert lib.md_tsmm_mv(a, 4, 4, None, None, 2, a, a, None) == NULL          # extra rows announced, none given
    assert lib.md_tsmm_mv(a, 0, 4, None, None, 0, a, a, None) == SHAPE
    assert lib.md_tsmm_mtw(a, 4, 4, None, None, 0, a, None, None, a, None) == NULL
    assert lib.md_tsmm_mtw(a, 4, 0, None, None, 0, a, a, None, a, None) == SHAPE
    assert lib.md_tsne_joint_scratch_doubles(100) == 101 and lib.md_tsne_scratch_doubles(100) == 300
    assert lib.md_tsne_rowpart_floats(100, 3) == 600 and lib.md_tsne_rowpart_floats(100, 4) == 0
    assert lib.md_tsne_update_blocks(600) == 3
    assert lib.md_col_mean_scratch_doubles(1000, 64) >= 64 and lib.md_tsmm_mtw_scratch_doubles(1000, 64, 4) >= 64 * 8
