#!/usr/bin/env python3
"""Generate the latent-space fixtures (embed_pca.npz, embed_tsne.npz) in this directory from the REFERENCE implementation and the
installed scikit-learn.

Run in the build container only (needs the reference checkout, scikit-learn and scipy; never on the GPU box):

    python tests/golden/make_embed_golden.py

The reference's ``src/visualization/visualize_latent_space.py`` is imported unmodified.  Its model is a stand-in whose ``encode``
returns the batch it is given (the loader is a list of (latent batch, labels) pairs cut from a seeded recipe of tests/embed_util.py,
which the tests regenerate: no input is stored), matplotlib is replaced by an object whose every call is a no-op, and the
``IncrementalPCA`` / ``TSNE`` names the reference module imported are subclasses that record what ``fit_transform`` returned.

  embed_pca.npz   ``emb2/<case>``, ``emb3/<case>``: what visualize_2D_/3D_latent_space(method="PCA") embedded for the five cases of
                  embed_util.PCA_CASES (the last with a flat tail behind the third singular value); ``multi/{fusion,vis,0D}``: the 2D ``_multi`` form on N = 700 rows of a (48 | 16)-column pair
                  (fusion = both, 64 columns); ``rows/2``, ``rows/-1``: rows the reference embedded from a 6-batch loader of 10-row
                  batches with limit_iters = 2 and -1.
  embed_tsne.npz  per case of embed_util.TSNE_CASES (clustered recipe, 4 centres): the joint P of scikit-learn's
                  ``_joint_probabilities`` (``P/<case>`` in full for N <= 300, else ``Prows/<case>`` = 32 seeded rows, ``Pidx/<case>``
                  their indices; ``Psum/<case>`` all row sums), ``_kl_divergence`` value and gradient at embed_util.spread_y with P and
                  12 P (``kl1``, ``grad1``, ``kl12``, ``grad12``), the PCA start ``y0`` and Y after 1 and 5 steps of
                  ``_gradient_descent`` (12 P, momentum 0.5, automatic learning rate) from it (``y1``, ``y5``), and from R = 5 runs of
                  the reference's own function (np.random.seed(r) before run r; Barnes-Hut, as the reference calls it) the KL of each
                  returned embedding on the exact P (``kl_ref``) and its trustworthiness at 10 neighbours (``trust_ref``).
  self32/<name>   next to every recorded array: the deviation of tests/embed_util.py run in float32 from the recording -- the rounding
                  floor of the arithmetic the kernels use.  Tests allow 10 x this figure.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("REFERENCE_ROOT", "/root/reference")
sys.path.insert(0, REF)                                   # the reference's own `src` package
sys.path.insert(1, os.path.join(ROOT, "tests"))

import embed_util as eu                                                   # noqa: E402
from scipy.spatial.distance import squareform                            # noqa: E402
from sklearn.manifold import _t_sne, trustworthiness                     # noqa: E402
from sklearn.metrics import pairwise_distances                           # noqa: E402
import src.visualization.visualize_latent_space as ref                   # noqa: E402  (reference)

torch.set_num_threads(8)
R = 5


class _Noop:
    def __getattr__(self, name):
        return self

    def __call__(self, *a, **k):
        return self


ref.plt = _Noop()
ref.tqdm = lambda it, **k: it
RECORDED = []


def _recording(cls):
    class Rec(cls):
        def fit_transform(self, X, y=None, **kw):
            out = super().fit_transform(X, y, **kw)
            RECORDED.append((np.array(X), np.array(out)))
            return out
    Rec.__name__ = cls.__name__
    return Rec


ref.IncrementalPCA = _recording(ref.IncrementalPCA)
ref.TSNE = _recording(ref.TSNE)


class Identity(torch.nn.Module):
    def encode(self, x, x0=None):
        if x0 is None:
            return x
        return torch.cat([x, x0], 1), x, x0

    def forward(self, x):
        return x[:, :2]


def loader(x, y, batch):
    return [(torch.from_numpy(x[i:i + batch]), torch.from_numpy(y[i:i + batch])) for i in range(0, len(x), batch)]


def run_ref(fn, ld, method):
    del RECORDED[:]
    fn(Identity(), ld, device="cpu", save_dir=None, limit_iters=-1, method=method)
    return list(RECORDED)


def make_pca():
    out = {}
    for case, (N, D) in eu.PCA_CASES.items():
        x = eu.pca_input(case)
        lab = np.zeros(N, dtype=np.int64)
        for nc, fn in ((2, ref.visualize_2D_latent_space), (3, ref.visualize_3D_latent_space)):
            (xin, emb), = run_ref(fn, loader(x, lab, 64), "PCA")
            assert xin.shape == (N, D) and xin.dtype == np.float32
            key = "emb%d/%s" % (nc, case)
            out[key] = emb.astype(np.float32)
            out["self32/" + key] = eu.range_dev(eu.incremental_pca(x, nc, np.float32)[0], emb)
            print(key, "fp64 restatement", eu.range_dev(eu.incremental_pca(x, nc)[0], emb), "self32", out["self32/" + key])
    vis, x0 = eu.decaying(700, 48, 7211), eu.decaying(700, 16, 7212)
    ld = [({"video": torch.from_numpy(vis[i:i + 64]), "0D": torch.from_numpy(x0[i:i + 64])}, torch.zeros(len(vis[i:i + 64])))
          for i in range(0, 700, 64)]
    rec = run_ref(ref.visualize_2D_latent_space_multi, ld, "PCA")
    for name, (xin, emb) in zip(("fusion", "vis", "0D"), rec):
        out["multi/" + name] = emb.astype(np.float32)
        out["self32/multi/" + name] = eu.range_dev(eu.incremental_pca(xin, 2, np.float32)[0], emb)
        print("multi", name, xin.shape, "self32", out["self32/multi/" + name])
    x = eu.decaying(60, 16, 7213)
    for lim in (2, -1):
        del RECORDED[:]
        ref.visualize_2D_latent_space(Identity(), loader(x, np.zeros(60, dtype=np.int64), 10), device="cpu", save_dir=None,
                                      limit_iters=lim, method="PCA")
        out["rows/%d" % lim] = np.int64(RECORDED[0][0].shape[0])
    np.savez_compressed(os.path.join(HERE, "embed_pca.npz"), **out)


def make_tsne():
    out = {}
    for case, (N, D, nc, perp) in eu.TSNE_CASES.items():
        x, lab = eu.clustered(N, D, eu.TSNE_SEEDS[case])
        dof = max(nc - 1, 1)
        d2 = pairwise_distances(x, metric="euclidean", squared=True)
        Pc = _t_sne._joint_probabilities(d2, perp, 0)
        P = squareform(Pc)

        def rec(name, value, dev):
            out["%s/%s" % (name, case)] = value
            out["self32/%s/%s" % (name, case)] = dev
            print(case, name, "self32", dev)

        P32 = eu.joint_probabilities(x, perp, np.float32)
        P64 = eu.joint_probabilities(x, perp)
        print(case, "P fp64 restatement", float(np.max(np.abs(P64 - P))) / P.max())
        pdev = float(np.max(np.abs(P32 - P))) / float(P.max())
        if N <= 300:
            rec("P", P.astype(np.float32), pdev)
        else:
            idx = np.sort(np.random.default_rng(eu.TSNE_SEEDS[case]).choice(N, 32, replace=False))
            out["Pidx/" + case] = idx
            rec("Prows", P[idx].astype(np.float32), pdev)
        out["Psum/" + case] = P.sum(1)
        out["Pmax/" + case] = P.max()
        y = eu.spread_y(N, nc, eu.TSNE_SEEDS[case] + 50).astype(np.float64)
        for e in (1, 12):
            kl, g = _t_sne._kl_divergence(y.ravel(), Pc * e, dof, N, nc)
            kl32, g32, _ = eu.kl_gradient(P32, y, float(e), np.float32)
            kl64, g64, _ = eu.kl_gradient(P, y, float(e))
            print(case, e, "fp64 restatement kl", abs(kl64 - kl) / abs(kl), "grad", eu.l2_dev(g64, g.reshape(N, nc)))
            rec("kl%d" % e, np.float64(kl), abs(kl32 - kl) / abs(kl))
            rec("grad%d" % e, g.reshape(N, nc), eu.l2_dev(g32, g.reshape(N, nc)))
        y0 = eu.pca_init(x, nc)
        out["y0/" + case] = y0
        lr = eu.auto_learning_rate(N)
        y32 = eu.descend(P32, y0, 5, 12.0, 0.5, lr, np.float32)
        for steps in (1, 5):
            p, _, _ = _t_sne._gradient_descent(_t_sne._kl_divergence, y0.ravel().copy(), 0, steps, n_iter_check=50,
                                               n_iter_without_progress=250, momentum=0.5, learning_rate=lr,
                                               args=[Pc * 12.0, dof, N, nc], kwargs={})
            rec("y%d" % steps, p.reshape(N, nc), eu.max_dev(y32[steps - 1], p.reshape(N, nc)))
        fn = {("a"): ref.visualize_2D_latent_space, ("b"): ref.visualize_3D_latent_space, ("c"): ref.visualize_2D_latent_space_multi}[case]
        kls, trusts = [], []
        for r in range(R):
            np.random.seed(r)
            if case == "c":                                   # the *_multi forms use scikit-learn's default perplexity, 30
                ld = [({"video": torch.from_numpy(x[i:i + 64]), "0D": torch.from_numpy(x[i:i + 64])}, torch.from_numpy(lab[i:i + 64]))
                      for i in range(0, N, 64)]
                runs = run_ref(fn, ld, "tSNE")
                xin, emb = runs[1]                            # the video branch: the recipe itself (fusion is both copies)
            else:
                (xin, emb), = run_ref(fn, loader(x, lab, 64), "tSNE")
            assert np.array_equal(xin, x) and emb.shape == (N, nc)
            kls.append(_t_sne._kl_divergence(emb.astype(np.float64).ravel(), Pc, dof, N, nc)[0])
            trusts.append(trustworthiness(x, emb, n_neighbors=10))
        out["kl_ref/" + case] = np.array(kls)
        out["trust_ref/" + case] = np.array(trusts)
        t_own = eu.trustworthiness(x, emb, 10)
        print(case, "reference runs: kl", kls, "trust", trusts, "| own trustworthiness of the last run", t_own)
        assert abs(t_own - trusts[-1]) < 1e-12
        assert abs(eu.tsne_kl(x, emb, perp) - kls[-1]) / kls[-1] < 1e-4
    np.savez_compressed(os.path.join(HERE, "embed_tsne.npz"), **out)


if __name__ == "__main__":
    make_pca()
    make_tsne()
