"""CPU tests of the permutation feature importance: the float64 restatement of tests/importance_util.py (what
tests/test_importance_gpu.py compares the kernels with) against the recordings of tests/golden/importance_*.npz (written by
tests/golden/make_importance_golden.py from the reference's own functions), the permutation draw, the host-side planning of
src/feature_importance.py (fallback decisions, frame, names) and the header <-> binding <-> library check for the new symbols.

Bar of every loss comparison with a recording: 10 x the recorded ``self32`` figure (the deviation of the same restatement run in
float32) or 1e-6 relative, whichever is larger."""
import ctypes as C
import inspect
import os
import re
import sys
import types
import warnings

import numpy as np
import pytest
import torch

from src import _native
from tests import importance_util as iu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("md_window_gather", "md_eval_accumulate")
LOSSES = {"focal": ("loss", 2.0), "ldam": ("score", 30.0)}


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "importance_single.npz"))


@pytest.fixture(scope="module")
def gm(golden_dir):
    return np.load(os.path.join(golden_dir, "importance_multi.npz"))


def ldam_margins(cls_num, max_m=0.5):
    m = 1.0 / np.sqrt(np.sqrt(np.asarray(cls_num, dtype=np.float64)))
    return (m * (max_m / np.max(m))).astype(np.float32)


def spec(g, tag):
    if tag == "focal":
        return "focal", g["weight"], None, 2.0
    return "ldam", g["weight"], ldam_margins(g["cls_num"]), 30.0


def colperm_of(proc, F=14):
    return iu.colperm_table(F, list(range(F)), cumulative=(proc == "lit"))


# ---------------------------------------------------------------------------------------------------------- recipe and windows
def test_recorded_inputs_are_the_recipe(g):
    table, shot, time, starts, labels = iu.synthetic_table()
    assert np.array_equal(table, g["table"]) and np.array_equal(starts, g["starts"]) and np.array_equal(labels, g["labels"])
    assert table.dtype == np.float32 and table.shape[1] == 14 and 2000 <= len(table) <= 3000
    assert len(starts) % 32 != 0                                   # the test loader ends in a ragged batch
    assert int(starts.max()) + iu.SEQ_LEN - 1 < len(table)


def test_margin_condition_holds_for_every_sample_and_variant(g, gm):
    for proc in ("lit", "cor"):
        lg = g[proc + "/logits"]
        assert float(np.min(np.abs(lg[..., 0] - lg[..., 1]))) >= 1e-2
    for k in gm.files:
        if k.split("/")[-1].startswith("logits"):
            assert float(np.min(np.abs(gm[k][..., 0] - gm[k][..., 1]))) >= 1e-2, k


@pytest.mark.parametrize("proc", ["lit", "cor"])
def test_window_restatement_reproduces_the_recorded_windows_bit_for_bit(g, proc):
    perms = g["perms"].astype(np.int32)
    win = iu.windows(g["table"], g["starts"][g[proc + "/win_idx"]], iu.SEQ_LEN, 1, perms, colperm_of(proc))
    assert win.dtype == np.float32 and np.array_equal(win, g[proc + "/win"])
    # the two procedures differ exactly where the cumulative quirk says: variants 2.. carry the earlier permutations as well
    lit, cor = colperm_of("lit"), colperm_of("cor")
    assert np.array_equal(lit[:2], cor[:2]) and lit[1, 0] == 0 and (lit[2:, 0] == -1).all()
    for k in range(1, 14):
        assert list(np.nonzero(lit[1 + k] >= 0)[0]) == list(range(1, k + 1)) and list(np.nonzero(cor[1 + k] >= 0)[0]) == [k]


def test_multimodal_windows_follow_tau(gm):
    for tag in ("mm", "gb"):
        for tau in (1, 2):
            pre = "%s/tau%d/" % (tag, tau)
            table, starts = gm[pre + "table"], gm[pre + "starts"]
            assert int(starts[-1]) + 4 * tau == len(table) - 1                    # a window ending on the last row
            w = iu.windows(table, starts, 5, tau, gm[pre + "perms"].astype(np.int32), iu.colperm_table(6, list(range(6)), True))
            assert np.array_equal(w[0, -1, :, 0], table[starts[-1] + np.arange(5) * tau, 0])


# ---------------------------------------------------------------------------------------------------------- losses, totals, frame
@pytest.mark.parametrize("proc", ["lit", "cor"])
@pytest.mark.parametrize("tag", ["focal", "ldam"])
def test_per_batch_losses_totals_scores_and_importances_match_the_recording(g, proc, tag):
    kind, w, m, gs = spec(g, tag)
    labels, logits = g["labels"], g[proc + "/logits"]
    bounds = iu.batch_bounds(len(labels), 32)
    rec_b, rec_t, rec_f = g["%s/%s/batch" % (proc, tag)], g["%s/%s/total" % (proc, tag)], g["%s/%s/f1" % (proc, tag)]
    bar = max(10.0 * float(g["self32/%s/%s/batch" % (proc, tag)]), 1e-6)
    worst = 0.0
    tot, f1 = [], []
    for v in range(logits.shape[0]):
        b, _, arg = iu.batch_losses(kind, logits[v], labels, bounds, w, m, gs)
        worst = max(worst, float(np.max(np.abs(b - rec_b[v])) / np.max(np.abs(rec_b[v]))))
        assert np.array_equal(arg, g[proc + "/pred"][v])
        tot.append(iu.total_loss(b)); f1.append(iu.macro_f1(labels, arg))
        assert iu.total_loss(rec_b[v]) == rec_t[v]                     # total_loss += loss.item(), to the bit
        assert abs(tot[-1] - rec_t[v]) <= bar * abs(rec_t[v]) * len(b)
        assert abs(f1[-1] - rec_f[v]) <= 1e-12
    print(proc, tag, "per-batch deviation / largest batch loss", worst, "bar", bar)
    assert worst <= bar
    criteria = LOSSES[tag][0]
    fi = np.array([iu.importance(criteria, rec_t[v], rec_f[v], rec_t[0], rec_f[0]) for v in range(1, len(rec_t))])
    assert np.array_equal(fi, g["%s/%s/fi" % (proc, tag)])
    from src.feature_importance import importance_frame
    df = importance_frame(list(iu.COLS), list(rec_t), list(rec_f), criteria, 1, {c: c.upper() for c in iu.COLS})
    assert list(df.columns) == ["feature", "loss", "score", "feature_importance"]
    assert list(df.feature.values) == [iu.COLS[i].upper() for i in g["%s/%s/order" % (proc, tag)]]
    assert np.array_equal(df.feature_importance.values, fi[g["%s/%s/order" % (proc, tag)]])
    assert np.all(np.diff(df.feature_importance.values) >= 0)


def test_gradient_blending_total_is_the_blend_of_three_accumulations(gm):
    from src import _importance
    loss = types.SimpleNamespace(loss_scale=1.0, vis_weight=0.1, ts_weight=0.4, vis_ts_weight=0.5)
    for tau in (1, 2):
        pre = "gb/tau%d/" % tau
        labels, w = gm[pre + "labels"], gm[pre + "weight"]
        bounds = iu.batch_bounds(len(labels), 32)
        for v in range(7):
            parts = [iu.batch_losses("focal", gm[pre + n][v], labels, bounds, w, None, 2.0)[0] for n in ("logits", "logits_vis", "logits_ts")]
            mine = np.array([_importance.blend(np.float32(parts[0][s]), np.float32(parts[1][s]), np.float32(parts[2][s]), loss) for s in range(2)])
            assert np.max(np.abs(mine - gm[pre + "lit/batch"][v]) / np.abs(gm[pre + "lit/batch"][v])) <= 1e-6


# ---------------------------------------------------------------------------------------------------------- permutations
def test_permutation_draw_is_the_reference_stream(g):
    from src.feature_importance import draw_permutations
    state = np.random.get_state()
    try:
        np.random.seed(int(g["seed"]))
        perms = draw_permutations(len(g["table"]), 14)
        after = np.random.get_state()[1][:4].copy()
        np.random.seed(int(g["seed"]))
        col = g["table"][:, 3].copy()
        for k in range(4):
            x = g["table"][:, k].copy()
            np.random.shuffle(x)                                      # what the reference does to a column
            assert np.array_equal(x, g["table"][perms[k], k])
    finally:
        np.random.set_state(state)
    assert perms.dtype == np.int32 and np.array_equal(perms, g["perms"].astype(np.int32))
    assert np.array_equal(after, g["stream_after"])
    assert np.array_equal(col, g["table"][:, 3])


# ---------------------------------------------------------------------------------------------------------- the public function
def _loader(g, shuffle=False, drop=None, offset=iu.INDEX_OFFSET, batch_size=32):
    table, shot, time, starts, labels = iu.synthetic_table()
    frame = iu.frame_of(table, iu.COLS, shot, time)
    ds = iu.make_dataset(frame, iu.COLS, starts, labels, iu.SEQ_LEN, offset=offset)
    if drop:
        delattr(ds, drop)
    return frame, ds, torch.utils.data.DataLoader(ds, batch_size=batch_size, shuffle=shuffle)


class _Model(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))


def _fake_engine(monkeypatch, g, tag, seen):
    """The device stages replaced by the recordings: the sweep is given the spec the function built and answers with the recorded
    totals of whichever procedure that spec describes."""
    from src import feature_importance as fi

    def sweep(model, tab, starts, labels, seq_len, tau, perms, colperm, loss_fn, model_type, batch_size, drop_last, video, wpl, device):
        proc = "lit" if np.array_equal(colperm, colperm_of("lit")) else "cor"
        assert np.array_equal(colperm, colperm_of(proc))
        seen.update(proc=proc, perms=perms.copy(), starts=np.asarray(starts).copy(), batch_size=batch_size, drop_last=drop_last,
                    seq_len=seq_len, tau=tau, labels=np.asarray(labels).copy(), table=tab)
        return {"loss": list(g["%s/%s/total" % (proc, tag)]), "score": list(g["%s/%s/f1" % (proc, tag)])}

    monkeypatch.setattr(fi._importance, "permutation_sweep", sweep)
    monkeypatch.setattr(fi, "_guard", lambda loader, plan, device: plan["table"])
    return fi


@pytest.mark.parametrize("cumulative,proc", [(True, "lit"), (False, "cor")])
@pytest.mark.parametrize("tag", ["focal", "ldam"])
def test_cumulative_gives_the_literal_run_and_the_default_the_corrected_one(monkeypatch, g, cumulative, proc, tag):
    seen = {}
    fi = _fake_engine(monkeypatch, g, tag, seen)
    frame, ds, loader = _loader(g)
    before = frame.copy()
    ds.get_shot_num = True
    state = np.random.get_state()
    try:
        np.random.seed(int(g["seed"]))
        df = fi.compute_permute_feature_importance(_Model(), loader, list(iu.COLS), None, "cpu", "single", LOSSES[tag][0], None,
                                                   cumulative=cumulative, feature_map={c: c.upper() for c in iu.COLS})
        assert np.array_equal(np.random.get_state()[1][:4], g["stream_after"])
    finally:
        np.random.set_state(state)
    assert seen["proc"] == proc and np.array_equal(seen["perms"], g["perms"].astype(np.int32))
    assert np.array_equal(seen["starts"], g["starts"]) and np.array_equal(seen["labels"], g["labels"])
    assert (seen["batch_size"], seen["drop_last"], seen["seq_len"], seen["tau"]) == (32, False, iu.SEQ_LEN, 1)
    assert np.array_equal(seen["table"], g["table"])
    order = g["%s/%s/order" % (proc, tag)]
    assert list(df.feature.values) == [iu.COLS[i].upper() for i in order]
    assert np.array_equal(df.feature_importance.values, g["%s/%s/fi" % (proc, tag)][order])
    assert np.array_equal(df.loss.values, g["%s/%s/total" % (proc, tag)][1:][order])
    assert ds.ts_data is frame and frame.equals(before) and ds.get_shot_num is False      # nothing the caller holds was touched


def test_reference_names_positional_order_and_defaults():
    from src import feature_importance as fi
    p = inspect.signature(fi.compute_permute_feature_importance).parameters
    assert list(p)[:8] == ["model", "dataloader", "features", "loss_fn", "device", "model_type", "criteria", "save_dir"]
    assert [(k, p[k].default) for k in list(p)[8:]] == [("cumulative", False), ("n_repeats", 1), ("feature_map", None),
                                                          ("windows_per_launch", 8192)]
    q = inspect.signature(fi.compute_loss).parameters
    assert list(q) == ["dataloader", "model", "loss_fn", "device", "model_type"]
    assert (q["device"].default, q["model_type"].default) == ("cpu", "single")
    from src import _importance
    s = inspect.signature(_importance.permutation_sweep).parameters
    assert list(s)[:14] == ["model", "table", "starts", "labels", "seq_len", "tau", "perms", "colperm", "loss_fn", "model_type",
                            "batch_size", "drop_last", "video_batches", "windows_per_launch"]
    assert (s["drop_last"].default, s["video_batches"].default, s["windows_per_launch"].default) == (False, None, 8192)


def test_evaluate_detail_has_the_reference_signature(golden_dir):
    from src.evaluate import evaluate_detail
    p = inspect.signature(evaluate_detail).parameters
    assert list(p) == ["train_loader", "valid_loader", "test_loader", "model", "device", "save_csv", "tag", "model_type"]
    assert (p["device"].default, p["save_csv"].default, p["tag"].default, p["model_type"].default) == ("cpu", None, None, "single")
    d = np.load(os.path.join(golden_dir, "importance_detail.npz"))
    assert str(d["header"]) == "task,label,shot,pred,tag" and len(d["pred"]) == len(iu.synthetic_table()[3])
    assert list(d["task"][[0, 199, 200, 289, 290]]) == ["train", "train", "valid", "valid", "test"]


def test_a_feature_subset_permutes_only_those_columns(monkeypatch, g):
    from src import feature_importance as fi
    got = {}

    def sweep(model, tab, starts, labels, seq_len, tau, perms, colperm, *a):
        got.update(perms=perms, colperm=colperm)
        return {"loss": [2.0, 3.0, 1.0], "score": [0.5, 0.4, 0.5]}

    monkeypatch.setattr(fi._importance, "permutation_sweep", sweep)
    monkeypatch.setattr(fi, "_guard", lambda loader, plan, device: plan["table"])
    _, _, loader = _loader(g)
    df = fi.compute_permute_feature_importance(_Model(), loader, ["c05", "c02"], None, "cpu", "single", "loss", None)
    assert got["perms"].shape == (2, len(g["table"])) and got["colperm"].shape == (3, 14)
    want = -np.ones((3, 14), dtype=np.int32); want[1, 5] = 0; want[2, 2] = 1
    assert np.array_equal(got["colperm"], want)
    assert list(df.feature.values) == ["c05", "c02"] and list(df.feature_importance.values) == [0.5, 0.5]
    with pytest.raises(ValueError):
        fi.compute_permute_feature_importance(_Model(), loader, ["nope"], None, "cpu", "single", "loss", None)


def test_n_repeats_frame_carries_mean_and_std():
    from src.feature_importance import colperm_table, importance_frame
    losses = [2.0, 3.0, 2.5, 5.0, 2.5]                              # baseline, then repeat 0 (a, b), repeat 1 (a, b)
    scores = [0.8, 0.6, 0.8, 0.4, 0.8]
    df = importance_frame(["a", "b"], losses, scores, "loss", n_repeats=2).set_index("feature")
    assert list(df.columns) == ["loss", "score", "feature_importance", "loss_std", "score_std", "feature_importance_std"]
    assert df.shape == (2, 6)
    assert df.loc["a", "loss"] == 4.0 and df.loc["a", "loss_std"] == 1.0 and df.loc["a", "feature_importance"] == 1.0
    assert df.loc["a", "feature_importance_std"] == 0.5 and df.loc["b", "feature_importance"] == 0.25 and df.loc["b", "loss_std"] == 0.0
    assert abs(df.loc["a", "score"] - 0.5) < 1e-15 and abs(df.loc["a", "score_std"] - 0.1) < 1e-15
    assert list(df.index) == ["b", "a"]
    cp = colperm_table(5, [3, 1], False, 2)
    assert cp.shape == (5, 5) and cp[0].max() == -1
    assert [(int(np.argmax(r)), int(r.max())) for r in cp[1:]] == [(3, 0), (1, 1), (3, 2), (1, 3)]


def test_feature_map_precedence(monkeypatch):
    from src.feature_importance import importance_frame
    args = (["a", "b"], [2.0, 3.0, 2.5], [0.8, 0.6, 0.8], "loss", 1)
    monkeypatch.delitem(sys.modules, "src.config", raising=False)
    assert sorted(importance_frame(*args).feature.values) == ["a", "b"]                    # no overlay: names unchanged
    overlay = types.ModuleType("src.config")
    overlay.Config = type("Config", (), {"feature_map": {"a": "overlay-a", "b": "overlay-b"}})
    monkeypatch.setitem(sys.modules, "src.config", overlay)
    assert sorted(importance_frame(*args).feature.values) == ["overlay-a", "overlay-b"]     # the user's src.config
    assert sorted(importance_frame(*args, {"a": "A", "b": "B"}).feature.values) == ["A", "B"]   # the keyword wins
    assert not os.path.exists(os.path.join(os.path.dirname(_native.__file__), "config.py"))


# ---------------------------------------------------------------------------------------------------------- fallback decisions
def test_plan_accepts_the_sequential_loader_and_reads_its_geometry(g):
    from src.feature_importance import plan_sweep
    _, _, loader = _loader(g)
    plan = plan_sweep(loader, list(iu.COLS))
    assert np.array_equal(plan["starts"], g["starts"]) and plan["table"].dtype == np.float32
    assert plan["first"] == list(range(32)) and plan["last"] == list(range(len(g["starts"]) - len(g["starts"]) % 32, len(g["starts"])))
    assert plan["feature_cols"] == list(range(14)) and not plan["drop_last"]
    table, shot, time, starts, labels = iu.synthetic_table()
    ds = iu.make_dataset(iu.frame_of(table, iu.COLS), iu.COLS, starts, labels, iu.SEQ_LEN, multi_names=True)
    ds.tau = 1
    plan = plan_sweep(torch.utils.data.DataLoader(ds, batch_size=32, drop_last=True), ["c01"])     # the multimodal names
    assert plan["drop_last"] and plan["feature_cols"] == [1] and len(plan["last"]) == 32


@pytest.mark.parametrize("case,reason", [("no_indices", "no attribute"), ("shuffle", "not sequential"), ("unmapped", "does not map")])
def test_fallback_decision_and_its_warning(monkeypatch, g, case, reason):
    from src import feature_importance as fi
    frame, ds, loader = _loader(g, shuffle=(case == "shuffle"), drop=("indices" if case == "no_indices" else None),
                                offset=(iu.INDEX_OFFSET + 100000 if case == "unmapped" else iu.INDEX_OFFSET))
    with pytest.raises(fi._Mismatch, match=reason):
        fi.plan_sweep(loader, list(iu.COLS))
    called = {}

    def host_loop(model, dataloader, features, loss_fn, device, model_type, perms, colperm):
        called.update(perms=perms, colperm=colperm)
        return list(g["cor/focal/total"]), list(g["cor/focal/f1"])

    monkeypatch.setattr(fi, "host_loop", host_loop)
    monkeypatch.setattr(fi._importance, "permutation_sweep", lambda *a, **k: pytest.fail("the sweep must not run"))
    state = np.random.get_state()
    try:
        np.random.seed(int(g["seed"]))
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            df = fi.compute_permute_feature_importance(_Model(), loader, list(iu.COLS), None, "cpu", "single", "loss", None)
    finally:
        np.random.set_state(state)
    mine = [w for w in caught if "falling back to the host loop" in str(w.message)]
    assert len(mine) == 1 and reason in str(mine[0].message) and issubclass(mine[0].category, RuntimeWarning)
    assert np.array_equal(called["perms"], g["perms"].astype(np.int32)) and np.array_equal(called["colperm"], colperm_of("cor"))
    assert np.array_equal(df.feature_importance.values, g["cor/focal/fi"][g["cor/focal/order"]])


def test_host_loop_permutes_copies_and_gives_the_dataset_its_frame_back(monkeypatch, g):
    from src import feature_importance as fi
    frame, ds, loader = _loader(g)
    before = frame.copy()
    perms, colperm = g["perms"].astype(np.int32), colperm_of("lit")
    held = []

    def compute_loss(dataloader, model, loss_fn, device, model_type):
        held.append(dataloader.dataset.ts_data[iu.COLS].values.copy())
        return float(len(held)), 0.5

    monkeypatch.setattr(fi, "compute_loss", compute_loss)
    losses, scores = fi.host_loop(None, loader, list(iu.COLS), None, "cpu", "single", perms, colperm)
    assert losses == [float(i + 1) for i in range(15)] and ds.ts_data is frame and frame.equals(before)
    for v in range(15):
        for f in range(14):
            want = g["table"][:, f] if colperm[v, f] < 0 else g["table"][perms[colperm[v, f]], f]
            assert np.array_equal(held[v][:, f], want)


def test_geometry_is_refused_on_the_host():
    from src._importance import check_geometry
    cp = -np.ones((2, 3), dtype=np.int32); cp[1, 1] = 0
    perms = np.arange(10, dtype=np.int32)[None, :]
    check_geometry(10, np.array([0, 5]), 5, 1, perms, cp, 3)
    check_geometry(10, np.array([1]), 5, 2, perms, cp, 3)            # rows 1, 3, 5, 7, 9: ends on the last row
    for bad in (dict(starts=np.array([6])), dict(starts=np.array([-1])), dict(starts=np.array([2]), tau=2),
                dict(perms=np.arange(1, 11, dtype=np.int32)[None, :]), dict(perms=np.arange(9, dtype=np.int32)[None, :]),
                dict(colperm=np.array([[-1, 1, -1]], dtype=np.int32)), dict(colperm=np.array([[-2, 0, -1]], dtype=np.int32)),
                dict(colperm=cp[:, :2]), dict(tau=0)):
        kw = dict(starts=np.array([0, 5]), seq_len=5, tau=1, perms=perms, colperm=cp)
        kw.update(bad)
        with pytest.raises(ValueError):
            check_geometry(10, kw["starts"], kw["seq_len"], kw["tau"], kw["perms"], kw["colperm"], 3)


# ---------------------------------------------------------------------------------------------------------- ABI
def test_new_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mi355x_disrupt.h")).read()
    declared = set(re.findall(r"\b(md_[a-z0-9_]+)\s*\(", hdr))
    lib = _native.lib()
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in the header"
        assert name in _native.SIGNATURES, f"{name} has no ctypes prototype"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    src = open(os.path.join(ROOT, "disruption-prediciton-based-on-multimodal-deep-learning_amd", "csrc", "importance.hip")).read()
    assert "md_sample_loss" in src and "softmax_loss.h" in src                   # the loss arithmetic is shared, not restated
    assert "atomicAdd(&loss" not in src


def test_importance_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _native.lib()
    a = C.c_void_p(64)                                             # a non-null pointer that is never dereferenced: every call is refused
    NULL, SHAPE, UNSUP = -5, -1, -2
    assert lib.md_window_gather(None, 8, 2, a, 1, 2, 1, a, 1, a, 1, a, None) == NULL
    assert lib.md_window_gather(a, 8, 2, a, 1, 2, 1, None, 1, a, 1, a, None) == NULL       # a permutation announced, none given
    assert lib.md_window_gather(a, 8, 2, a, 1, 2, 1, a, 1, a, 1, None, None) == NULL
    for bad in ((0, 2, 1, 2, 1, 1), (8, 0, 1, 2, 1, 1), (8, 2, 0, 2, 1, 1), (8, 2, 1, 0, 1, 1), (8, 2, 1, 2, 0, 1), (8, 2, 1, 2, 1, 0)):
        R, F, n, T, tau, V = bad
        assert lib.md_window_gather(a, R, F, a, n, T, tau, a, 1, a, V, a, None) == SHAPE
    assert lib.md_window_gather(a, 2 ** 31, 2, a, 1, 2, 1, a, 1, a, 1, a, None) == UNSUP
    assert lib.md_eval_accumulate(0, None, a, 1, 4, 2, a, 1, None, None, 2.0, a, 1, a, None, None) == NULL
    assert lib.md_eval_accumulate(0, a, a, 1, 4, 2, None, 1, None, None, 2.0, a, 1, a, None, None) == NULL
    assert lib.md_eval_accumulate(3, a, a, 1, 4, 2, a, 1, None, None, 2.0, a, 1, a, None, None) == UNSUP
    assert lib.md_eval_accumulate(0, a, a, 1, 4, 9, a, 1, None, None, 2.0, a, 1, a, None, None) == UNSUP     # K <= 8
    assert lib.md_eval_accumulate(0, a, a, 0, 4, 2, a, 1, None, None, 2.0, a, 1, a, None, None) == SHAPE
    assert lib.md_eval_accumulate(0, a, a, 1, 4, 2, a, 0, None, None, 2.0, a, 1, a, None, None) == SHAPE
    assert lib.md_eval_accumulate(0, a, a, 2, 4, 2, a, 3, None, None, 2.0, a, 2, a, None, None) == SHAPE     # rows of loss overlap
