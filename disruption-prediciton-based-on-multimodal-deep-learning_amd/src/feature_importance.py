"""Permutation feature importance of the 0D signals -- mirror of the reference's ``src/feature_importance.py`` (``compute_loss``
:29-71, ``compute_permute_feature_importance`` :75-134; same names, positional order and defaults).

The reference runs F + 1 complete passes over the test loader, cutting every window out of a pandas frame on the host and reading
the loss back after every batch.  Here the table of rows x signals is put into HBM once and ALL variants are evaluated in one
device-side sweep (src/_importance.py: ``md_window_gather`` -> one eval forward -> ``md_eval_accumulate`` per chunk, one read-back
at the end); for the multimodal models the video side is encoded once per sample instead of F + 1 times.

What is kept: the permutations are drawn exactly as the reference draws them (one ``np.random.shuffle`` of a length-R array per
feature, in feature order, from the global NumPy generator -- a script that seeds NumPy gets the reference's permutations and leaves
the stream where the reference leaves it); ``loss`` is ``total_loss += loss.item()`` over the loader's batches; the score is the
macro-F1 of ``argmax softmax``; both importance formulas; the ascending sort; the ``barh`` figure.

What differs, on purpose: the reference's undo (``dataset.ts_data = data_orig``) only works for the first feature,
so its importances of features 1 .. F-1 are cumulative (feature k is measured with features 1 .. k all permuted).  The default here
permutes every feature alone; ``cumulative=True`` reproduces the reference number for number.  The reference's side effect (the
caller's frame keeps column 0 shuffled, the dataset keeps columns 1 .. F-1 shuffled) is never reproduced: frame and dataset are
left untouched.  The sorted frame is returned (the reference returns nothing).

A dataset is taken by protocol: ``ts_data`` (DataFrame), ``cols`` (or ``ts_cols``), ``indices`` (or ``ts_data_indices``), ``labels``,
``seq_len``, optional ``tau``, ``get_shot_num``; window i = rows ``ts_data.index.get_indexer([indices[i]]) + 1 + t*tau``.  Before the
sweep the loader's own first and last batch are compared bit for bit with the gathered windows; on any mismatch (custom dataset,
a loader that is not sequential, a missing attribute, an index that does not map) the function warns once, naming the reason, and
runs the literal host loop on a copy of the frame with the same device model -- slow but right.
"""
from __future__ import annotations

import warnings
from typing import List, Literal, Optional

import numpy as np
import torch
from torch.utils.data import DataLoader

from . import _importance
from .train import _forward
from .utils.metrics import macro_f1


def compute_loss(dataloader: DataLoader, model: torch.nn.Module, loss_fn: torch.nn.Module, device: str = "cpu",
                 model_type: Literal["single", "multi", "multi-GB"] = "single"):
    """Reference :29-71, literally: one eval pass over the loader, ``total_loss += loss.item()`` per batch, macro-F1 of
    ``argmax softmax`` at the end.  (The predictions stay on the device until the loop is over.)"""
    model.eval()
    model.to(device)
    total_loss = 0
    total_pred, total_label = [], []
    for data, target in dataloader:
        with torch.no_grad():
            output, output_vis, output_ts = _forward(model, data, device, model_type)
            tgt = target.to(device)
            loss = loss_fn(output, output_vis, output_ts, tgt) if model_type == "multi-GB" else loss_fn(output, tgt)
            total_loss += loss.item()
            total_pred.append(torch.nn.functional.softmax(output, dim=1).max(1, keepdim=True)[1].view(-1))
            total_label.append(target.view(-1))
    preds = torch.concat(total_pred, dim=0).cpu().numpy()
    labels = torch.concat(total_label, dim=0).cpu().numpy()
    return total_loss, macro_f1(labels, preds)


# ------------------------------------------------------------------------------------------------------------ host-side planning
class _Mismatch(Exception):
    pass


def _attr(ds, *names):
    for n in names:
        if hasattr(ds, n):
            return getattr(ds, n)
    raise _Mismatch("the dataset has no attribute %s" % " / ".join(names))


def plan_sweep(dataloader: DataLoader, features: List) -> dict:
    """Everything the sweep needs from a loader, or a ``_Mismatch`` naming why the loader's windows cannot be gathered from one
    table.  Pure host work (no device, no model)."""
    ds = dataloader.dataset
    frame = _attr(ds, "ts_data")
    cols = list(_attr(ds, "cols", "ts_cols"))
    indices = _attr(ds, "ts_data_indices", "indices")
    labels = np.asarray(_attr(ds, "labels")).reshape(-1)
    seq_len = int(_attr(ds, "seq_len"))
    tau = int(getattr(ds, "tau", 1))
    missing = [f for f in features if f not in cols]
    if missing:
        raise ValueError("compute_permute_feature_importance: %r are not columns of the dataset" % missing)
    batch_size = dataloader.batch_size
    if batch_size is None or dataloader.batch_sampler is None:
        raise _Mismatch("the loader does not batch by batch_size")
    batches = [list(b) for b in dataloader.batch_sampler]
    flat = [i for b in batches for i in b]
    if flat != list(range(len(flat))):
        raise _Mismatch("the loader is not sequential")
    if any(len(b) != batch_size for b in batches[:-1]) or not batches or len(batches[-1]) > batch_size:
        raise _Mismatch("the loader's batches are not cut by batch_size")
    drop_last = len(flat) < len(indices)
    if drop_last and (len(indices) // batch_size) * batch_size != len(flat):
        raise _Mismatch("the loader visits %d of %d samples" % (len(flat), len(indices)))
    if len(labels) != len(indices):
        raise _Mismatch("labels and indices differ in length")
    if not frame.index.is_unique:
        raise _Mismatch("the frame's index is not unique")
    pos = frame.index.get_indexer(list(indices))
    if len(pos) == 0 or int(pos.min()) < 0:
        raise _Mismatch("an index of the dataset does not map to a row of ts_data")
    starts = pos.astype(np.int64) + 1
    if int(starts.max()) + (seq_len - 1) * tau >= len(frame):
        raise _Mismatch("a window runs past the last row of ts_data")
    table = np.ascontiguousarray(frame[cols].values, dtype=np.float32)
    return {"table": table, "cols": cols, "starts": starts, "labels": labels.astype(np.int64), "seq_len": seq_len, "tau": tau,
            "batch_size": int(batch_size), "drop_last": bool(drop_last), "first": batches[0], "last": batches[-1],
            "feature_cols": [cols.index(f) for f in features], "n_rows": len(frame)}


def draw_permutations(n_rows: int, n_perms: int) -> np.ndarray:
    """One ``np.random.shuffle`` of a length-R array per permutation, in order, from the global generator (reference :99): shuffling
    ``np.arange(R)`` consumes the stream exactly as shuffling a column does and yields the index form, permuted column = column[perm]."""
    out = np.empty((n_perms, n_rows), dtype=np.int32)
    for k in range(n_perms):
        a = np.arange(n_rows)
        np.random.shuffle(a)
        out[k] = a
    return out


def colperm_table(n_cols: int, feature_cols: List[int], cumulative: bool = False, n_repeats: int = 1) -> np.ndarray:
    """(1 + n_repeats*F, n_cols) int32 map variant x column -> permutation (-1: none).  Variant 0 is the baseline, variant 1 + r*F + k
    measures feature k in repeat r with permutation r*F + k.  ``cumulative``: the reference's literal behaviour -- its undo works for
    k = 0 only, so variant k >= 1 carries the permutations of features 1 .. k."""
    F = len(feature_cols)
    cp = -np.ones((1 + n_repeats * F, n_cols), dtype=np.int32)
    for r in range(n_repeats):
        for k in range(F):
            for j in (range(1, k + 1) if (cumulative and k >= 1) else [k]):
                cp[1 + r * F + k, feature_cols[j]] = r * F + j
    return cp


def _resolve_feature_map(feature_map):
    if feature_map is not None:
        return feature_map
    try:
        from src.config import Config                     # the user's overlay, if it provides one
        return Config().feature_map
    except Exception:
        return None


def importance_frame(features: List, losses, scores, criteria: str, n_repeats: int = 1, feature_map=None):
    """The reference's result frame (:92-124) from the per-variant totals (variant 0 = baseline): columns ``feature, loss, score,
    feature_importance`` sorted ascending by importance; with n_repeats > 1 the three numbers are means over the repeats and
    ``loss_std, score_std, feature_importance_std`` are added."""
    import pandas as pd
    F = len(features)
    loss_orig, score_orig = losses[0], scores[0]
    L = np.asarray(losses[1:], dtype=np.float64).reshape(n_repeats, F)
    Sc = np.asarray(scores[1:], dtype=np.float64).reshape(n_repeats, F)
    rows = []
    for k in range(F):
        fis = []
        for r in range(n_repeats):
            loss, score = float(L[r, k]), float(Sc[r, k])
            fis.append(abs(abs(loss - loss_orig) / loss_orig) if criteria == 'loss' else abs(score - score_orig) / score_orig)
        if n_repeats == 1:
            rows.append({"feature": features[k], "loss": float(L[0, k]), "score": float(Sc[0, k]), "feature_importance": fis[0]})
        else:
            rows.append({"feature": features[k], "loss": float(L[:, k].mean()), "score": float(Sc[:, k].mean()),
                         "feature_importance": float(np.mean(fis)), "loss_std": float(L[:, k].std()),
                         "score_std": float(Sc[:, k].std()), "feature_importance_std": float(np.std(fis))})
    df = pd.DataFrame(rows)
    fmap = _resolve_feature_map(feature_map)
    if fmap is not None:
        df['feature'] = df['feature'].apply(lambda x: fmap[x])
    return df.sort_values('feature_importance')


def _draw_figure(df, save_dir):
    try:
        import matplotlib
        matplotlib.use("Agg", force=False)
        import matplotlib.pyplot as plt
    except Exception:
        return
    n = len(df)
    fig = plt.figure(figsize=(8, 8))
    plt.barh(np.arange(n), df.feature_importance)
    plt.yticks(np.arange(n), df.feature.values)
    plt.title('0D data - feature importance')
    plt.ylim((-1, n + 1))
    plt.xlabel('Permutation feature importance')
    plt.ylabel('Feature', size=14)
    plt.savefig(save_dir)
    plt.close(fig)


# ------------------------------------------------------------------------------------------------------------ the two procedures
def _loader_windows(dataloader, idxs, device):
    items = [dataloader.dataset[i] for i in idxs]
    data, _ = dataloader.collate_fn(items) if dataloader.collate_fn is not None else torch.utils.data.default_collate(items)
    x = data['0D'] if isinstance(data, dict) else data
    return x.to(device)


def _guard(dataloader, plan, device):
    """The loader's own first and last batch against the gathered windows, bit for bit."""
    from . import ops
    tab = torch.from_numpy(plan["table"]).to(device)
    base = torch.full((1, tab.shape[1]), -1, dtype=torch.int32, device=device)
    for idxs in (plan["first"], plan["last"]):
        mine = _loader_windows(dataloader, idxs, device)
        st = torch.from_numpy(plan["starts"][idxs]).to(device)
        got = ops.window_gather(tab, st, plan["seq_len"], plan["tau"], None, base)[0]
        if mine.shape != got.shape or mine.dtype != got.dtype or not torch.equal(mine, got):
            raise _Mismatch("the loader's windows are not rows of ts_data[cols] (custom __getitem__?)")
    return tab


def host_loop(model, dataloader, features, loss_fn, device, model_type, perms, colperm):
    """The literal procedure on the host: per variant a permuted COPY of the frame is given to the dataset and the loader is iterated
    (``compute_loss``).  The dataset gets its own frame back afterwards."""
    ds = dataloader.dataset
    orig = ds.ts_data
    cols = list(getattr(ds, "cols", None) or getattr(ds, "ts_cols"))
    losses, scores = [], []
    try:
        for v in range(colperm.shape[0]):
            work = orig.copy()
            for f in np.nonzero(colperm[v] >= 0)[0]:
                work[cols[f]] = orig[cols[f]].values[perms[colperm[v, f]]]
            ds.ts_data = work
            loss, score = compute_loss(dataloader, model, loss_fn, device, model_type)
            losses.append(loss); scores.append(score)
    finally:
        ds.ts_data = orig
    return losses, scores


def compute_permute_feature_importance(model: torch.nn.Module, dataloader: DataLoader, features: List, loss_fn: torch.nn.Module,
                                       device: str, model_type: Literal["single", "multi", "multi-GB"],
                                       criteria: Literal['loss', 'score'], save_dir: Optional[str],
                                       cumulative: bool = False, n_repeats: int = 1, feature_map=None,
                                       windows_per_launch: int = 8192):
    """Reference :75-134.  Returns the sorted frame; draws the reference's figure into ``save_dir`` when it is given."""
    ds = dataloader.dataset
    ds.get_shot_num = False                                # :87
    features = list(features)
    F = len(features)
    n_repeats = max(1, int(n_repeats))
    plan, reason = None, None
    try:
        plan = plan_sweep(dataloader, features)
    except _Mismatch as e:
        reason = str(e)
    if plan is not None:
        n_rows, cols, fcols = plan["n_rows"], plan["cols"], plan["feature_cols"]
    else:
        if not hasattr(ds, "ts_data"):
            raise RuntimeError("compute_permute_feature_importance: %s; nothing to permute" % reason)
        cols = list(getattr(ds, "cols", None) or getattr(ds, "ts_cols"))
        n_rows, fcols = len(ds.ts_data), [cols.index(f) for f in features]
    perms = draw_permutations(n_rows, n_repeats * F)       # the global NumPy stream moves exactly as in the reference
    colperm = colperm_table(len(cols), fcols, cumulative, n_repeats)
    model.to(device)
    tab = None
    if plan is not None:
        try:
            tab = _guard(dataloader, plan, device)
        except _Mismatch as e:
            reason = str(e)
    if tab is None:
        warnings.warn("compute_permute_feature_importance: %s; falling back to the host loop over the loader (slow)" % reason,
                      RuntimeWarning, stacklevel=2)
        losses, scores = host_loop(model, dataloader, features, loss_fn, device, model_type, perms, colperm)
    else:
        video = None
        if model_type != "single":
            video = (data['video'] for data, _ in dataloader)          # the loader's own clips, once
        res = _importance.permutation_sweep(model, tab, plan["starts"], plan["labels"], plan["seq_len"], plan["tau"], perms, colperm,
                                            loss_fn, model_type, plan["batch_size"], plan["drop_last"], video, windows_per_launch,
                                            device)
        losses, scores = res["loss"], res["score"]
    df = importance_frame(features, losses, scores, criteria, n_repeats, feature_map)
    if save_dir:
        _draw_figure(df, save_dir)
    return df
