#!/usr/bin/env python3
"""Time the latent-space reductions on the GPU and print one JSON line (also written to --out): for exact t-SNE at
N in {1024, 4096, 16384} (D = 128, 2 components, perplexity 64) the ms of distances + affinities, the ms per iteration (median over
--repeats device-event intervals around --iters queued iterations, after a warm-up) and the wall-clock total of a 1000-iteration
``tsne_embed`` call; for incremental PCA the ms of ``pca_embed`` at (16384, 128) and (4096, 16641).  If scikit-learn is importable,
its exact and Barnes-Hut wall times at N = 1024 / 4096 on at most 16 threads go in as ``cpu_baseline`` (--no-cpu skips them).
Usage: python tools/latent_time.py [--iters N] [--repeats R] [--sizes 1024,4096,16384] [--no-cpu] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "disruption-prediciton-based-on-multimodal-deep-learning_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402


def recipe(N, D, seed):
    rng = np.random.default_rng(seed)
    c = rng.normal(size=(4, D)) * 16.0 / np.sqrt(D)
    return (c[rng.integers(0, 4, size=N)] + rng.normal(size=(N, D))).astype(np.float32)


def _events(fn, repeats, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def cpu_baseline():
    """Wall seconds of scikit-learn's exact and Barnes-Hut t-SNE (1000 iterations) on at most 16 threads; None without scikit-learn."""
    try:
        from sklearn.manifold import TSNE
        from threadpoolctl import threadpool_limits
    except ImportError:
        return None
    cpu = {}
    with threadpool_limits(limits=16):
        for n in (1024, 4096):
            x = recipe(n, 128, n)
            for method in ("exact", "barnes_hut"):
                t0 = time.perf_counter()
                TSNE(n_components=2, perplexity=64, method=method, init="pca", random_state=0, n_jobs=16).fit_transform(x)
                cpu["%s_%d_s" % (method, n)] = round(time.perf_counter() - t0, 2)
    return cpu


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", default="1024,4096,16384")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--cpu-only", action="store_true", help="only the scikit-learn baseline (needs no GPU)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.cpu_only:
        line = json.dumps({"metric": "latent_map_cpu_baseline", "cpu_baseline": cpu_baseline()})
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    if not torch.cuda.is_available():
        raise SystemExit("latent_time.py measures on the GPU; none is visible")
    from src.visualization import _embed
    dev = torch.device("cuda:0")
    tsne = {}
    _embed.tsne_embed(torch.from_numpy(recipe(512, 128, 1)).to(dev), 2, perplexity=64.0, max_iter=250)    # warm-up: the process's first
    torch.cuda.synchronize()                                                                            # map carries one-time costs
    for n in [int(v) for v in a.sizes.split(",")]:
        x = torch.from_numpy(recipe(n, 128, n)).to(dev)
        aff = _events(lambda: _embed.joint_probabilities(x, 64.0), a.repeats)
        P = _embed.joint_probabilities(x, 64.0)
        y = torch.randn(n, 2, device=dev) * 1e-4
        d = _embed._Descent(P, y)
        upd, gains = torch.zeros_like(y), torch.ones_like(y)

        def run(kl=False):
            for _ in range(a.iters):
                d.gradient(12.0, kl)
                d.update(upd, gains, 0.5, 200.0)
        per_iter = _events(run, a.repeats) / a.iters
        with_kl = _events(lambda: d.gradient(1.0, True), a.repeats)
        del d, P
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, res = _embed.tsne_embed(x, 2, perplexity=64.0, max_iter=1000)
        torch.cuda.synchronize()
        total = (time.perf_counter() - t0) * 1e3
        tsne[str(n)] = {"affinities_ms": round(aff, 3), "iteration_ms": round(per_iter, 4), "gradient_with_kl_ms": round(with_kl, 4),
                        "total_1000_iter_ms": round(total, 1), "n_iter": res.n_iter, "kl": round(res.kl_divergence, 5)}
        torch.cuda.empty_cache()
    pca = {}
    for n, dd in ((16384, 128), (4096, 16641)):
        x = torch.from_numpy(recipe(n, dd, n + dd)).to(dev)
        pca["%dx%d" % (n, dd)] = round(_events(lambda: _embed.pca_embed(x, 2), max(1, a.repeats // 2)), 2)
        del x
        torch.cuda.empty_cache()
    out = {"metric": "latent_map_ms", "tsne_exact_d128_perp64": tsne, "pca_embed_ms": pca, "iters": a.iters, "repeats": a.repeats,
           "note": "total_1000_iter_ms is wall clock of tsne_embed (PCA start, affinities, 1000 iterations, 20 read-backs)"}
    if not a.no_cpu:
        out["cpu_baseline"] = cpu_baseline()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
