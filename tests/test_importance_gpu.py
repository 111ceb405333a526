"""GPU tests of the permutation feature importance: ``md_window_gather`` against torch indexing (bit for bit), ``md_eval_accumulate``
against the float64 restatement of tests/importance_util.py, and the sweep end to end against the recordings the reference produced
(tests/golden/importance_*.npz, tests/golden/make_importance_golden.py).

Bars: logits within 1e-3 of the recording (the project's standing forward bar), per-batch and total loss within 1e-3 relative
(SURVEY 8c), confusion matrices, macro-F1 and the order of the importance frame exact.  The fixtures guarantee |logit0 - logit1| >= 1e-2
for every sample of every variant, so no prediction can flip within the logit bar and no sample is excluded from the exact
comparisons.  A per-batch loss of ``md_eval_accumulate`` on given logits must lie within n * 2^-24 * sum |terms| of the float64
value (the fp32 summation bound for n terms).

Measured on an MI355X (printed by the tests, run with -s): see DESIGN section 12."""
import os
import warnings

import numpy as np
import pytest
import torch

from tests import importance_util as iu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "importance_single.npz"))


@pytest.fixture(scope="module")
def gm(golden_dir):
    return np.load(os.path.join(golden_dir, "importance_multi.npz"))


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


# ---------------------------------------------------------------------------------------------------------- md_window_gather
def torch_windows(table, start, T, tau, perms, colperm):
    rows = start.view(-1, 1) + torch.arange(T, device=table.device).view(1, -1) * tau              # (n, T)
    V, F = colperm.shape
    out = torch.empty((V, rows.shape[0], T, F), device=table.device, dtype=table.dtype)
    for v in range(V):
        for f in range(F):
            c = int(colperm[v, f])
            r = rows if c < 0 else perms[c].long()[rows]
            out[v, :, :, f] = table[r, f]
    return out


@pytest.mark.parametrize("F", [1, 14, 18])
@pytest.mark.parametrize("tau", [1, 2])
def test_window_gather_equals_torch_indexing_bit_for_bit(F, tau):
    from src import ops
    rng = np.random.default_rng(100 * F + tau)
    R, T, N = 700, 21, 150
    table = dev(rng.standard_normal((R, F)).astype(np.float32))
    starts = np.sort(rng.integers(0, R - (T - 1) * tau, N)).astype(np.int64)
    starts[-1] = R - 1 - (T - 1) * tau                                                # a window ending on the last row
    P = F + 1
    perms = dev(np.stack([rng.permutation(R) for _ in range(P)]).astype(np.int32))
    fc = list(range(F))
    cps = [iu.colperm_table(F, fc, False), iu.colperm_table(F, fc, True)]              # baseline + single-column, cumulative
    two = -np.ones((2, F), dtype=np.int32); two[1, 0] = P - 1                          # two permutations on one variant
    if F > 1:
        two[1, F - 1] = 0
    cps.append(two)
    st = dev(starts)
    for cp in cps:
        cpd = dev(cp)
        for a, b in ((0, N), (37, 101)):                                               # the whole list, and a chunk from mid-list
            got = ops.window_gather(table, st[a:b], T, tau, perms, cpd)
            want = torch_windows(table, st[a:b], T, tau, perms, cp)
            assert got.shape == want.shape and torch.equal(got, want)
            assert np.array_equal(got.cpu().numpy(), iu.windows(table.cpu().numpy(), starts[a:b], T, tau, perms.cpu().numpy(), cp))
    base = ops.window_gather(table, st, T, tau, None, dev(-np.ones((1, F), dtype=np.int32)))      # no permutation table at all
    assert torch.equal(base[0, -1, -1], table[R - 1])
    with pytest.raises(RuntimeError):
        ops.window_gather(table.cpu(), st, T, tau, perms, cpd)


# ---------------------------------------------------------------------------------------------------------- md_eval_accumulate
@pytest.mark.parametrize("kind", ["focal", "ldam", "ce"])
@pytest.mark.parametrize("weighted", [True, False])
def test_eval_accumulate_matches_the_float64_restatement(kind, weighted):
    from src import ops
    rng = np.random.default_rng(7 + len(kind) + weighted)
    V, K, bs = 5, 2, 32
    n = 4 * bs + 11                                                                    # a ragged last segment
    logits = (rng.standard_normal((V, n, K)) * 3).astype(np.float32)
    target = rng.integers(0, K, n).astype(np.int64)
    w = np.array([1.7, 0.4], dtype=np.float32) if weighted else None
    m = np.array([0.5, 0.31], dtype=np.float32) if kind == "ldam" else None
    gs = {"focal": 2.0, "ldam": 30.0, "ce": 0.0}[kind]
    bounds = iu.batch_bounds(n, bs)
    S = len(bounds) - 1
    seg = dev(bounds.astype(np.int32))
    runs = []
    for _ in range(2):
        loss = torch.zeros((V, S + 3), device=DEV)                                     # a wider buffer: the rows are a strided view
        conf = torch.zeros((V, K, K), device=DEV, dtype=torch.int32)
        p0 = torch.empty((V, n), device=DEV)
        ops.eval_accumulate(kind, dev(logits).view(V * n, K), dev(target), V, seg, None if w is None else dev(w),
                            None if m is None else dev(m), gs, loss[:, 1:1 + S], conf, p0)
        ops.eval_accumulate(kind, dev(logits).view(V * n, K), dev(target), V, seg, None if w is None else dev(w),
                            None if m is None else dev(m), gs, loss[:, 1:1 + S], conf, None)          # counts accumulate across launches
        runs.append((loss.cpu().numpy(), conf.cpu().numpy(), p0.cpu().numpy()))
    assert all(np.array_equal(a, b) for a, b in zip(runs[0], runs[1]))                 # two runs: the same bits
    loss, conf, p0 = runs[0]
    assert not loss[:, 0].any() and not loss[:, 1 + S:].any()
    worst = 0.0
    for v in range(V):
        want, mag, arg = iu.batch_losses(kind, logits[v], target, bounds, w, m, gs)
        assert np.array_equal(conf[v], 2 * iu.confusion(target, arg, K))
        sm = np.exp(logits[v].astype(np.float64) - logits[v].max(1, keepdims=True)); sm /= sm.sum(1, keepdims=True)
        assert np.max(np.abs(p0[v] - sm[:, 0])) <= 4 * EPS
        assert np.array_equal(p0[v] > 0.5, arg == 0)                                   # p0's arg-max
        nseg = np.diff(bounds)
        bound = nseg * EPS * mag
        d = np.abs(loss[v, 1:1 + S] - want)
        worst = max(worst, float(np.max(d / bound)))
        assert np.all(d <= bound), (kind, weighted, v, d, bound)
    print(kind, "weighted" if weighted else "unweighted", "largest per-batch deviation / bound", worst)


def test_eval_accumulate_agrees_with_the_loss_modules():
    """The same per-sample arithmetic as md_softmax_loss (csrc/softmax_loss.h): a segment's value is the module's value for that batch."""
    from src import ops
    from src.loss import CELoss, FocalLoss, LDAMLoss
    rng = np.random.default_rng(5)
    n, K = 75, 2
    x = dev((rng.standard_normal((n, K)) * 3).astype(np.float32)); y = dev(rng.integers(0, K, n).astype(np.int64))
    w = torch.tensor([1.7, 0.4])
    seg = dev(np.array([0, 32, 64, 75], dtype=np.int32))
    for kind, mod, m, gs in (("focal", FocalLoss(w, 2.0), None, 2.0), ("ldam", LDAMLoss([30, 90], 0.5, w, 30), "m", 30.0),
                             ("ce", CELoss(w), None, 0.0)):
        loss = torch.zeros((1, 3), device=DEV)
        ops.eval_accumulate(kind, x, y, 1, seg, w.to(DEV), mod.m_list.to(DEV) if m else None, gs, loss, None, None)
        want = torch.stack([mod(x[a:b], y[a:b]).detach() for a, b in ((0, 32), (32, 64), (64, 75))])
        rel = float(((loss[0] - want).abs() / want.abs()).max())
        print(kind, "segment value vs loss module, relative", rel)
        assert rel <= 4 * EPS


# ---------------------------------------------------------------------------------------------------------- end to end, single
def load_transformer(g):
    from src.models.transformer import Transformer
    m = Transformer(n_features=14, kernel_size=3, feature_dims=32, max_len=iu.SEQ_LEN, n_layers=1, n_heads=4, dim_feedforward=64,
                    dropout=0.1, cls_dims=16, n_classes=2)
    m.load_state_dict({k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd/")}, strict=True)
    return m.to(DEV).eval()


def losses_of(g):
    from src.loss import FocalLoss, LDAMLoss
    w = torch.from_numpy(g["weight"])
    return {"focal": (FocalLoss(w, 2.0), "loss"), "ldam": (LDAMLoss([int(c) for c in g["cls_num"]], 0.5, w, 30), "score")}


def check_against_recording(res, g, proc, tag, what):
    logits = g[proc + "/logits"]
    V, N, K = logits.shape
    dl = float(np.max(np.abs(res["logits"] - logits)))
    rb, rt = g["%s/%s/batch" % (proc, tag)], g["%s/%s/total" % (proc, tag)]
    db = float(np.max(np.abs(res["batch_loss"] - rb) / np.abs(rb)))
    dt = float(np.max(np.abs(np.asarray(res["loss"]) - rt) / np.abs(rt)))
    print("%s %s/%s: logits %.3g (bar 1e-3) | per-batch loss %.3g, total loss %.3g relative (bar 1e-3)" % (what, proc, tag, dl, db, dt))
    assert dl <= 1e-3 and db <= 1e-3 and dt <= 1e-3
    for v in range(V):
        assert np.array_equal(res["confusion"][v], iu.confusion(g["labels"], g[proc + "/pred"][v], K))
        assert res["score"][v] == iu.macro_f1(g["labels"], g[proc + "/pred"][v])          # exact; scikit-learn's own rounding: 1e-12
        assert abs(res["score"][v] - g["%s/%s/f1" % (proc, tag)][v]) <= 1e-12


@pytest.mark.parametrize("proc", ["lit", "cor"])
@pytest.mark.parametrize("tag", ["focal", "ldam"])
def test_sweep_matches_the_reference_recording(g, proc, tag):
    from src import _importance
    from src.feature_importance import importance_frame
    model = load_transformer(g)
    loss_fn, criteria = losses_of(g)[tag]
    cp = iu.colperm_table(14, list(range(14)), proc == "lit")
    res = _importance.permutation_sweep(model, g["table"], g["starts"], g["labels"], iu.SEQ_LEN, 1, g["perms"].astype(np.int32), cp,
                                        loss_fn, "single", 32, windows_per_launch=2048, keep_logits=True, want_p0=True)
    check_against_recording(res, g, proc, tag, "sweep")
    assert np.array_equal(res["p0"] > 0.5, g[proc + "/pred"] == 0)
    df = importance_frame(list(iu.COLS), res["loss"], res["score"], criteria)
    assert list(df.feature.values) == [iu.COLS[i] for i in g["%s/%s/order" % (proc, tag)]]


def test_sweep_equals_one_variant_and_one_batch_at_a_time(g):
    """The batched sweep against the same model run per variant and per loader batch on windows built with torch, through the
    package's own loss module -- and the chunking does not change a bit of it."""
    from src import _importance
    model = load_transformer(g)
    loss_fn, _ = losses_of(g)["focal"]
    perms = g["perms"].astype(np.int32)
    cp = iu.colperm_table(14, list(range(14)), False)[:6]
    table, starts, labels = dev(g["table"]), dev(g["starts"]), dev(g["labels"])
    res = _importance.permutation_sweep(model, g["table"], g["starts"], g["labels"], iu.SEQ_LEN, 1, perms, cp, loss_fn, "single", 32,
                                        windows_per_launch=1024, keep_logits=True)
    res2 = _importance.permutation_sweep(model, g["table"], g["starts"], g["labels"], iu.SEQ_LEN, 1, perms, cp, loss_fn, "single", 32,
                                         windows_per_launch=8192, keep_logits=True)
    assert np.array_equal(res["confusion"], res2["confusion"]) and res["score"] == res2["score"]
    assert np.max(np.abs(res["batch_loss"] - res2["batch_loss"]) / np.abs(res2["batch_loss"])) <= 1e-3
    N = len(g["starts"])
    wins = torch_windows(table, starts, iu.SEQ_LEN, 1, dev(perms), cp)
    worst_l = worst_b = 0.0
    with torch.no_grad():
        for v in range(cp.shape[0]):
            total, preds = 0.0, []
            for s, a in enumerate(range(0, N, 32)):
                out = model(wins[v, a:a + 32].contiguous())
                lb = float(loss_fn(out, labels[a:a + 32]).item())
                total += lb
                preds.append(out.argmax(1))
                worst_l = max(worst_l, float((out - dev(res["logits"][v, a:a + 32])).abs().max()))
                worst_b = max(worst_b, abs(lb - float(res["batch_loss"][v, s])) / abs(lb))
            assert abs(total - res["loss"][v]) <= 1e-3 * abs(total)
            pred = torch.cat(preds).cpu().numpy()
            assert np.array_equal(res["confusion"][v], iu.confusion(g["labels"], pred, 2))
            assert res["score"][v] == iu.macro_f1(g["labels"], pred)
    print("sweep vs one variant and one batch at a time: logits", worst_l, "per-batch loss relative", worst_b)
    assert worst_l <= 1e-3 and worst_b <= 1e-3


def make_loader(g, **kw):
    table, shot, time, starts, labels = iu.synthetic_table()
    frame = iu.frame_of(table, iu.COLS, shot, time)
    ds = iu.make_dataset(frame, iu.COLS, starts, labels, iu.SEQ_LEN)
    return frame, ds, torch.utils.data.DataLoader(ds, batch_size=32, **kw)


@pytest.mark.parametrize("cumulative,proc", [(True, "lit"), (False, "cor")])
def test_public_function_from_a_loader(g, tmp_path, cumulative, proc):
    from src.feature_importance import compute_permute_feature_importance
    model = load_transformer(g)
    frame, ds, loader = make_loader(g)
    before = frame.copy()
    for tag in ("focal", "ldam"):
        loss_fn, criteria = losses_of(g)[tag]
        np.random.seed(int(g["seed"]))
        png = str(tmp_path / ("fi_%s.png" % tag))
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            df = compute_permute_feature_importance(model, loader, list(iu.COLS), loss_fn, DEV, "single", criteria, png,
                                                    cumulative=cumulative)
        assert not [w for w in caught if "falling back" in str(w.message)]               # the guard accepts this loader
        assert np.array_equal(np.random.get_state()[1][:4], g["stream_after"])
        order = g["%s/%s/order" % (proc, tag)]
        assert list(df.feature.values) == [iu.COLS[i] for i in order]
        rt = g["%s/%s/total" % (proc, tag)][1:][order]
        assert np.max(np.abs(df.loss.values - rt) / np.abs(rt)) <= 1e-3
        assert np.max(np.abs(df.score.values - g["%s/%s/f1" % (proc, tag)][1:][order])) <= 1e-12
        rf = g["%s/%s/fi" % (proc, tag)][order]
        print(proc, tag, "importance deviation", float(np.max(np.abs(df.feature_importance.values - rf))))
        if criteria == "score":
            assert np.max(np.abs(df.feature_importance.values - rf)) <= 1e-12
        assert os.path.getsize(png) > 0
    assert ds.ts_data is frame and frame.equals(before)


def test_fallback_host_loop_equals_the_sweep(g):
    """A loader the guard refuses (its dataset serves windows that are not rows of the table) goes through the host loop; on the
    small case the host loop and the sweep agree."""
    from src import _importance, feature_importance as fi
    model = load_transformer(g)
    loss_fn, _ = losses_of(g)["focal"]
    frame, ds, loader = make_loader(g)
    feats = ["c03", "c00"]
    perms = g["perms"].astype(np.int32)[:2]
    cp = fi.colperm_table(14, [3, 0], False, 1)
    res = _importance.permutation_sweep(model, g["table"], g["starts"], g["labels"], iu.SEQ_LEN, 1, perms, cp, loss_fn, "single", 32)
    losses, scores = fi.host_loop(model, loader, feats, loss_fn, DEV, "single", perms, cp)
    rel = max(abs(a - b) / abs(b) for a, b in zip(res["loss"], losses))
    print("host loop vs sweep: total loss relative", rel)
    assert rel <= 1e-3 and scores == res["score"] and ds.ts_data is frame
    # the guard: a dataset whose windows are scaled on the fly is refused, with one warning, and still answered
    inner = type(ds).__getitem__
    type(ds).__getitem__ = lambda self, i: (inner(self, i)[0] * 2.0, inner(self, i)[1])
    with pytest.raises(fi._Mismatch):
        fi._guard(loader, fi.plan_sweep(loader, feats), DEV)
    np.random.seed(int(g["seed"]))
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        df = fi.compute_permute_feature_importance(model, loader, ["c00"], loss_fn, DEV, "single", "loss", None)
    assert len([w for w in caught if "falling back to the host loop" in str(w.message)]) == 1 and len(df) == 1


# ---------------------------------------------------------------------------------------------------------- multi, multi-GB
AV = dict(image_size=32, patch_size=8, n_frames=5, dim=16, depth=1, n_heads=2, in_channels=3, d_head=8, dropout=0.0, embedd_dropout=0.0,
          scale_dim=2)
A0 = dict(n_features=6, kernel_size=3, feature_dims=16, max_len=5, n_layers=1, n_heads=2, dim_feedforward=24, dropout=0.0)


def load_multi(gm, tag, tau):
    from src.models import MultiModal as MM
    if tag == "gb":
        m = MM.MultiModalModel_GB(2, dict(AV, n_classes=2, pool="cls", alpha=1.0), dict(A0, cls_dims=12, n_classes=2))
    else:
        m = MM.MultiModalModel(2, dict(AV, pool="mean"), dict(A0))
    pre = "%s/tau%d/sd/" % (tag, tau)
    m.load_state_dict({k[len(pre):]: torch.from_numpy(gm[k]) for k in gm.files if k.startswith(pre)}, strict=True)
    return m.to(DEV).eval()


@pytest.mark.parametrize("tag", ["mm", "gb"])
@pytest.mark.parametrize("tau", [1, 2])
def test_multimodal_sweep(gm, tag, tau):
    from src import _importance
    from src.GradientBlending import GradientBlending
    from src.loss import FocalLoss
    pre = "%s/tau%d/" % (tag, tau)
    model = load_multi(gm, tag, tau)
    w = torch.from_numpy(gm[pre + "weight"])
    if tag == "gb":
        loss_fn, mt = GradientBlending(FocalLoss(w, 2.0), FocalLoss(w, 2.0), FocalLoss(w, 2.0), 0.1, 0.4, 0.5, 1.0), "multi-GB"
    else:
        loss_fn, mt = FocalLoss(w, 2.0), "multi"
    table, starts, labels = gm[pre + "table"], gm[pre + "starts"], gm[pre + "labels"]
    N = len(starts)
    clips = torch.from_numpy(iu.synthetic_clips(N, int(gm[pre + "clip_seed"])))
    perms = gm[pre + "perms"].astype(np.int32)
    cp = iu.colperm_table(6, list(range(6)), True)
    seen = []                                                # (MultiModalModel_GB's video side is not a module call: next test)
    hook = (model.vis_model if tag == "gb" else model.encoder_video).register_forward_hook(
        lambda mod, args, out: seen.append(args[0].shape[0]))
    try:
        res = _importance.permutation_sweep(model, table, starts, labels, 5, tau, perms, cp, loss_fn, mt, 32,
                                            video_batches=[clips[:32], clips[32:]], windows_per_launch=7 * 32, keep_logits=True)
    finally:
        hook.remove()
    if tag == "mm":
        assert sum(seen) == N, seen                          # the video encoder ran exactly once per sample over the whole sweep
    names = ["logits", "logits_vis", "logits_ts"] if tag == "gb" else ["logits"]
    got = res["logits"] if tag == "gb" else [res["logits"]]
    for name, lg in zip(names, got):
        d = float(np.max(np.abs(lg - gm[pre + name])))
        print(pre, name, "vs recording", d)
        assert d <= 1e-3
    # logits from the cached video latent against a full two-input forward per variant
    wins = iu.windows(table, starts, 5, tau, perms, cp)
    worst = 0.0
    with torch.no_grad():
        for v in range(cp.shape[0]):
            full = model(clips.to(DEV), dev(wins[v]))
            full = full if isinstance(full, tuple) else (full,)
            for f, lg in zip(full, got):
                worst = max(worst, float((f - dev(lg[v])).abs().max()))
    print(pre, "cached video latent vs full forward", worst)
    assert worst <= 1e-3
    rb, rt = gm[pre + "lit/batch"], gm[pre + "lit/total"]
    db = float(np.max(np.abs(res["batch_loss"] - rb) / np.abs(rb))); dt = float(np.max(np.abs(np.asarray(res["loss"]) - rt) / np.abs(rt)))
    print(pre, "per-batch loss", db, "total loss", dt, "relative (bar 1e-3)")
    assert db <= 1e-3 and dt <= 1e-3
    for v in range(7):
        assert np.array_equal(res["confusion"][v], iu.confusion(labels, np.argmax(gm[pre + "logits"][v], 1), 2))
        assert abs(res["score"][v] - gm[pre + "lit/f1"][v]) <= 1e-12


def test_gb_video_encoder_runs_once_per_sample(gm):
    """MultiModalModel_GB's video side is ``vis_model._encode`` (not a module call): count the calls of its transformer trunk input,
    the patch embedding, instead."""
    from src import _importance
    from src.GradientBlending import GradientBlending
    from src.loss import FocalLoss
    pre = "gb/tau1/"
    model = load_multi(gm, "gb", 1)
    w = torch.from_numpy(gm[pre + "weight"])
    loss_fn = GradientBlending(FocalLoss(w, 2.0), FocalLoss(w, 2.0), FocalLoss(w, 2.0), 0.1, 0.4, 0.5, 1.0)
    N = len(gm[pre + "starts"])
    clips = torch.from_numpy(iu.synthetic_clips(N, int(gm[pre + "clip_seed"])))
    calls = []
    inner = model.vis_model._encode
    model.vis_model._encode = lambda x: (calls.append(x.shape[0]), inner(x))[1]
    _importance.permutation_sweep(model, gm[pre + "table"], gm[pre + "starts"], gm[pre + "labels"], 5, 1, gm[pre + "perms"].astype(np.int32),
                                  iu.colperm_table(6, list(range(6)), True), loss_fn, "multi-GB", 32,
                                  video_batches=[clips[:32], clips[32:]], windows_per_launch=64)
    assert sum(calls) == N, calls


# ---------------------------------------------------------------------------------------------------------- evaluate_detail
def test_evaluate_detail_matches_the_reference_csv(g, golden_dir, tmp_path):
    import pandas as pd
    from src.evaluate import evaluate_detail
    d = np.load(os.path.join(golden_dir, "importance_detail.npz"))
    model = load_transformer(g)
    table, shot, time, starts, labels = iu.synthetic_table()
    frame = iu.frame_of(table, iu.COLS, shot, time)
    loaders = []
    for name in ("train", "valid", "test"):
        idx = d["split/" + name]
        ds = iu.make_dataset(frame, iu.COLS, starts[idx], labels[idx], iu.SEQ_LEN, shot_num=[int(shot[starts[i]]) for i in idx])
        loaders.append(torch.utils.data.DataLoader(ds, batch_size=32))
    path = str(tmp_path / "detail.csv")
    evaluate_detail(loaders[0], loaders[1], loaders[2], model, DEV, path, "fixture", "single")
    assert all(ld.dataset.get_shot_num is True for ld in loaders)
    assert open(path).read().splitlines()[0] == str(d["header"])
    df = pd.read_csv(path)
    assert list(df.columns) == ["task", "label", "shot", "pred", "tag"]
    assert str(df.label.dtype) == str(d["label_dtype"]) and str(df.shot.dtype) == str(d["shot_dtype"])
    assert list(df.task.values) == list(d["task"]) and list(df.tag.values) == list(d["tag"])
    assert np.array_equal(df.label.values, d["label"]) and np.array_equal(df.shot.values, d["shot"])
    dev_p = float(np.max(np.abs(df.pred.values - d["pred"])))
    print("evaluate_detail: pred deviation", dev_p, "(bar 1e-3)")
    assert dev_p <= 1e-3
