#!/usr/bin/env python3
"""Time the permutation feature importance on the GPU and print one JSON line (also written to --out).  One synthetic test set of
script-like size (--rows table rows, F = 18 signals, windows of 21 rows every --stride rows, the script-default 0D Transformer,
loader batch 32, FocalLoss):

  (a) ``host_loop``: the reference's procedure as it runs on the parent commit -- the frame's column shuffled on the host, a
      DataLoader over a dataset that cuts every window out of the frame with ``.loc``, this package's GPU model, ``loss.item()``
      after every batch; F + 1 passes.  Timed on --host-variants passes (baseline + the first features) and scaled to F + 1.
  (b) ``sweep``: ``compute_permute_feature_importance`` (guard included), all F + 1 variants in one device-side sweep.
  (c) ``stages``: gather / forward / accumulate of the sweep from device events around them.

Wall-clock with a device synchronisation before every reading of the clock; after a warm-up; median and (min, max) of --repeats runs.
Usage: python tools/importance_time.py [--rows 60000] [--stride 2] [--repeats 5] [--host-variants 2] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "disruption-prediciton-based-on-multimodal-deep-learning_amd")]

import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402
import torch  # noqa: E402

SEQ_LEN, F = 21, 18


class FrameWindows(torch.utils.data.Dataset):
    """Serves windows the way the scripts' 0D dataset does: a label-based slice of the frame per sample."""

    def __init__(self, frame, cols, indices, labels):
        self.ts_data, self.cols, self.indices, self.labels = frame, cols, indices, labels
        self.seq_len, self.get_shot_num = SEQ_LEN, False

    def __len__(self):
        return len(self.indices)

    def __getitem__(self, i):
        k = self.indices[i]
        data = self.ts_data[self.cols].loc[k + 1:k + self.seq_len].values
        return torch.from_numpy(data).float(), torch.from_numpy(np.array(self.labels[i]))


def timed(fn, repeats, warmup=1):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return {"median_s": round(statistics.median(out), 4), "min_s": round(min(out), 4), "max_s": round(max(out), 4), "runs": len(out)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=60000)
    ap.add_argument("--stride", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-variants", type=int, default=2)
    ap.add_argument("--windows-per-launch", type=int, default=8192)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from src import _importance, feature_importance as fi
    from src.loss import FocalLoss
    from src.models.transformer import Transformer

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    cols = ["s%02d" % i for i in range(F)]
    frame = pd.DataFrame(rng.standard_normal((a.rows, F)).astype(np.float32), columns=cols)
    indices = list(range(0, a.rows - SEQ_LEN - 1, a.stride))
    labels = list(rng.integers(0, 2, len(indices)))
    loader = torch.utils.data.DataLoader(FrameWindows(frame, cols, indices, labels), batch_size=32, shuffle=False)
    torch.manual_seed(0)
    model = Transformer(n_features=F, kernel_size=5, feature_dims=128, max_len=SEQ_LEN, n_layers=4, n_heads=8, dim_feedforward=1024,
                        dropout=0.1, cls_dims=128, n_classes=2).to(dev).eval()
    loss_fn = FocalLoss(torch.tensor([1.0, 1.0]), 2.0)
    N = len(indices)
    res = {"metric": "permutation_importance_s", "N": N, "F": F, "rows": a.rows, "seq_len": SEQ_LEN, "batch_size": 32,
           "model": "Transformer(n_features=18, kernel_size=5, feature_dims=128, n_layers=4, n_heads=8, dim_feedforward=1024, cls_dims=128)",
           "loss": "FocalLoss(gamma=2)", "windows_per_launch": a.windows_per_launch}

    # (b) the sweep through the public function
    def sweep():
        np.random.seed(0)
        return fi.compute_permute_feature_importance(model, loader, cols, loss_fn, dev, "single", "loss", None,
                                                     windows_per_launch=a.windows_per_launch)
    res["sweep"] = timed(sweep, a.repeats)

    # (c) its stages, from device events
    plan = fi.plan_sweep(loader, cols)
    np.random.seed(0)
    perms = fi.draw_permutations(a.rows, F)
    cp = fi.colperm_table(F, list(range(F)))
    stages = []
    for _ in range(a.repeats + 1):
        t = {}
        _importance.permutation_sweep(model, plan["table"], plan["starts"], plan["labels"], SEQ_LEN, 1, perms, cp, loss_fn, "single", 32,
                                      windows_per_launch=a.windows_per_launch, timings=t)
        stages.append(t)
    stages = stages[1:]
    res["stages_ms"] = {k: round(statistics.median(s[k] for s in stages), 3) for k in ("gather_ms", "forward_ms", "accumulate_ms")}
    res["stages_ms"]["chunks"] = stages[0]["chunks"]

    # (a) the host loop of the parent commit, on a few variants, scaled to F + 1 passes
    hv = max(1, min(a.host_variants, F + 1))

    def host():
        return fi.host_loop(model, loader, cols, loss_fn, dev, "single", perms, cp[:hv])
    h = timed(host, max(1, min(a.repeats, 2)), warmup=0)
    res["host_loop"] = {"variants_timed": hv, "per_pass_s": round(h["median_s"] / hv, 3), "min_s": h["min_s"], "max_s": h["max_s"],
                        "runs": h["runs"], "scaled_to_F_plus_1_s": round(h["median_s"] / hv * (F + 1), 2)}
    res["speedup"] = round(res["host_loop"]["scaled_to_F_plus_1_s"] / res["sweep"]["median_s"], 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
