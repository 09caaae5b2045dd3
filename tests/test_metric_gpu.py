"""The evaluation metrics on the device (mrec_metric.hip, ops.auc_counts / ops.group_rank_hist, mindrec_amd.metrics) against the
numpy restatement tests/_metric_ref.py: every count compared exactly.  The restatement itself is held to sklearn and to the reference's
own MAP@12 by tests/test_metric_ref.py."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _metric_ref as R  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_multitable_map.npz")
# one row, one wave +- 1, one radix tile (2048 keys) +- 1, two count tiles (1024 rows) and a third started
SIZES = [2, 63, 64, 65, 2047, 2048, 2049, 4097]


def _auc(dev, pred, label):
    from mindrec_amd import ops
    out = ops.auc_counts(torch.from_numpy(np.ascontiguousarray(pred, np.float32)).to(dev),
                         torch.from_numpy(np.ascontiguousarray(label, np.float32)).to(dev))
    assert out.dtype == torch.int64 and out.shape == (4,) and out.is_cuda
    return tuple(out.tolist())


def _hist(dev, pred, label, group, **kw):
    from mindrec_amd import ops
    out = ops.group_rank_hist(torch.from_numpy(np.ascontiguousarray(pred, np.float32)).to(dev),
                              torch.from_numpy(np.ascontiguousarray(label, np.float32)).to(dev), torch.from_numpy(group).to(dev), **kw)
    topk = kw.get("topk", 12)
    assert out.dtype == torch.int64 and out.shape == (topk + 1,) and out.is_cuda
    out = out.tolist()
    return out[:topk], out[topk]


def _check_hist(dev, pred, label, group, **kw):
    hist, G = _hist(dev, pred, label, group, **kw)
    want, wantG = R.group_rank_hist(pred, label, group, **kw)
    assert G == wantG and hist == want.tolist()
    return hist, G


# ---- AUC ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_auc_counts_continuous(dev, n):
    rng = np.random.default_rng(n)
    pred = (rng.standard_normal(n) * 3).astype(np.float32)              # both signs: the key map's two branches
    label = (rng.random(n) < 0.3).astype(np.float32)
    assert _auc(dev, pred, label) == R.auc_counts(pred, label)


@pytest.mark.parametrize("n", SIZES)
def test_auc_counts_four_levels(dev, n):
    """Tie groups of about n / 4 rows: they straddle waves, count tiles and radix tiles."""
    rng = np.random.default_rng(1000 + n)
    pred = rng.choice(np.array([-0.5, 0.125, 0.25, 0.75], np.float32), size=n)
    label = (rng.random(n) < 0.5).astype(np.float32)
    assert _auc(dev, pred, label) == R.auc_counts(pred, label)


def test_auc_counts_all_equal(dev):
    n = 4097
    label = (np.random.default_rng(5).random(n) < 0.3).astype(np.float32)
    twoU, P, N, n_nan = _auc(dev, np.full(n, 0.625, np.float32), label)
    assert (P, N, n_nan) == (int(label.sum()), n - int(label.sum()), 0) and twoU == P * N


def test_auc_counts_special_keys(dev):
    # one positive at -0.0 against negatives at +0.0 (a tie), -1e-40 and -inf (below it) and 1e-40 (above it): 2 * 2 + 1
    pred = np.array([-0.0, 0.0, -1e-40, -np.inf, 1e-40], np.float32)
    assert pred[2] != 0 and pred[4] != 0                                # (denormals, not flushed on the way here)
    assert _auc(dev, pred, np.array([1, 0, 0, 0, 0], np.float32)) == (5, 1, 4, 0)
    keys = np.array([-0.0, 0.0, -1e-40, 1e-40, -np.inf, np.inf, -3.5, 3.5], np.float32)
    rng = np.random.default_rng(9)
    pred = rng.permutation(np.tile(keys, 37))
    label = (rng.random(pred.size) < 0.5).astype(np.float32)
    assert _auc(dev, pred, label) == R.auc_counts(pred, label)


def test_auc_rejections(dev):
    from mindrec_amd.metrics import DeviceAUCMetric
    rng = np.random.default_rng(3)
    pred = rng.random(300).astype(np.float32)
    label = (rng.random(300) < 0.5).astype(np.float32)
    pred[137] = np.nan
    got = _auc(dev, pred, label)
    assert got[3] == 1 and got == R.auc_counts(pred, label)             # the NaN row is in none of the other counts
    m = DeviceAUCMetric(capacity=64, device=dev)
    m.update(None, pred, label)
    with pytest.raises(ValueError, match="NaN"):
        m.eval()
    assert m.counts["n_nan"] == 1
    for one in (0.0, 1.0):
        m.clear()
        m.update(None, pred[:100], np.full(100, one, np.float32))
        with pytest.raises(ValueError, match="one class"):
            m.eval()


# ---- grouped rank histogram ---------------------------------------------------------------------------------------------------
def test_group_rank_hist_golden(dev):
    z = np.load(GOLDEN)
    hist, G = _hist(dev, z["pred"], z["label"], z["display_id"])
    assert G == int(z["G"]) and hist == z["hist"].tolist()


@pytest.mark.parametrize("dtype,ids", [(np.int32, [5, 2 ** 31 - 1, -7, 1 << 20, 0, 123456789]),
                                       (np.int64, [5, 2 ** 31 - 1, -(2 ** 40), 2 ** 32 + 1, 2 ** 32 + 2, 2 ** 62])],
                         ids=["int32", "int64"])
def test_group_rank_hist_display_sizes(dev, dtype, ids):
    """Displays of 1, 12, 13, 30, 31 and 2500 rows (around topk, around pad_to, many waves of one group), their rows interleaved in
    feed order, ids scattered; labels with none, one or several positives per display; predictions of both signs, with repeats."""
    rng = np.random.default_rng(77)
    sizes = [1, 12, 13, 30, 31, 2500]
    group = rng.permutation(np.repeat(np.array(ids, dtype), sizes))
    n = group.size
    pred = (np.round(rng.standard_normal(n) * 8) / 16).astype(np.float32)
    label = (rng.random(n) < 0.05).astype(np.float32)
    hist, G = _check_hist(dev, pred, label, group)
    assert G == 6
    _check_hist(dev, pred, label, group, topk=64, pad_to=40)
    _check_hist(dev, pred, label, group, topk=1, pad_to=0)
    # ... and fed display by display: one run per display inside a wave
    order = np.argsort(group, kind="stable")
    assert _hist(dev, pred[order], label[order], group[order]) == (hist, G)


def test_group_rank_hist_one_display_holding_every_row(dev):
    rng = np.random.default_rng(8)
    n = 4097
    pred = rng.random(n).astype(np.float32)
    label = np.zeros(n, np.float32)
    label[[3000, 4000]] = 1.0
    hist, G = _check_hist(dev, pred, label, np.full(n, 42, np.int32), topk=64)
    assert G == 1 and sum(hist) == int((pred > pred[3000]).sum() < 64)


def test_group_rank_hist_clicked_row_rules(dev):
    pred = np.array([0.3, 0.9, 0.5,   0.2, 0.7, 0.6,   -0.1, -0.2, -0.3, -0.4, -0.5], np.float32)
    label = np.array([0, 0, 0,        0, 1, 1,         1, 0, 0, 0, 0], np.float32)
    group = np.array([7, 7, 7,        3, 3, 3,         9, 9, 9, 9, 9], np.int32)
    # display 7 has no positive: its first row, two rows above it; display 3 has two: the first, nothing above it;
    # display 9's clicked prediction is negative in a display of 5: 25 pads rank above it
    hist, G = _check_hist(dev, pred, label, group)
    assert G == 3 and hist == [1, 0, 1] + [0] * 9
    hist, G = _check_hist(dev, pred, label, group, topk=30)
    assert hist[25] == 1 and sum(hist) == 3
    # equal predictions, and a clicked 0.0 against the pads, do not rank above the clicked row
    hist, G = _check_hist(dev, np.array([0.5, 0.5, 0.5, 0.0], np.float32), np.array([0, 1, 0, 1], np.float32), np.array([1, 1, 1, 2], np.int64))
    assert G == 2 and hist[0] == 2


# ---- the metric classes -------------------------------------------------------------------------------------------------------
def test_device_auc_metric_grows_and_matches_host_metric(dev, capsys):
    from mindrec_amd.metrics import DeviceAUCMetric
    from mindrec_amd.wide_deep_run import AUCMetric
    rng = np.random.default_rng(21)
    pred = (np.floor(rng.random((3, 50, 1)) * 32) / 32).astype(np.float32)
    label = (rng.random((3, 50, 1)) < 0.4).astype(np.float32)
    m, h = DeviceAUCMetric(capacity=64, device=dev), AUCMetric()
    for metric in (m, h):
        metric.update(None, torch.from_numpy(pred[0]).to(dev), torch.from_numpy(label[0]).to(dev))
        metric.update(None, pred[1], label[1])                          # host input
        metric.update(None, torch.from_numpy(pred[2]).to(dev), torch.from_numpy(label[2]).to(dev))
    capsys.readouterr()
    got = m.eval()
    out = capsys.readouterr().out.splitlines()
    assert out == ["====" * 20 + " auc_metric  end", "====" * 20 + " auc: {}".format(got)]
    twoU, P, N, n_nan = R.auc_counts(pred, label)
    assert m.counts == {"twoU": twoU, "P": P, "N": N, "n_nan": n_nan} and all(type(v) is int for v in m.counts.values())
    assert m._cap == 256 and got == R.auc(twoU, P, N)
    want = h.eval()
    print(f"|device - host AUC| = {abs(got - want):.3e}")
    assert abs(got - want) <= (150 + 2) * 2.0 ** -52
    m.clear()
    m.update(None, pred[0], label[0])
    assert m.eval() == R.auc(*R.auc_counts(pred[0], label[0])[:3])


def test_runner_eval_with_both_metrics(dev):
    from mindrec_amd.metrics import DeviceAUCMetric
    from mindrec_amd.wide_deep import WideDeepConfig, WideDeepEngine, synthetic_batch
    from mindrec_amd.wide_deep_run import AUCMetric, WideDeepRunner
    cfg = WideDeepConfig(vocab_size=10_000, emb_dim=16, field_size=39, batch_size=64, deep_layer_dim=[32], mlp_dtype="fp32")
    eng = WideDeepEngine(cfg, dev)
    data = [synthetic_batch(cfg, dev, "zipf", seed=s) for s in (3, 4, 5)]
    run = WideDeepRunner(eng, metrics={"auc": AUCMetric(), "device_auc": DeviceAUCMetric(capacity=64, device=dev)})
    out = run.eval(data)
    run.close()
    n = 3 * cfg.batch_size
    print(f"auc {out['auc']!r} device_auc {out['device_auc']!r}")
    assert 0.0 <= out["device_auc"] <= 1.0 and abs(out["auc"] - out["device_auc"]) <= (n + 2) * 2.0 ** -52


def test_device_auc_map_metric_on_the_reference_fixture(dev, capsys):
    from mindrec_amd.metrics import DeviceAUCMAPMetric
    z = np.load(GOLDEN)
    m = DeviceAUCMAPMetric(capacity=1024, device=dev)
    for lo in range(0, 5000, 1250):
        sl = slice(lo, lo + 1250)
        m.update(None, torch.from_numpy(z["pred"][sl]).to(dev), z["label"][sl], torch.from_numpy(z["display_id"][sl]).to(dev))
    auc = m.eval()
    assert capsys.readouterr().out.splitlines()[-1] == "Eval result: auc: {}, map: {}".format(auc, m.map)
    assert auc == R.auc(*R.auc_counts(z["pred"], z["label"])[:3])
    assert m.rank_hist == z["hist"].tolist() and m.groups == int(z["G"])
    print(f"|device MAP - reference MAP| = {abs(m.map - float(z['ref_map'])):.3e}")
    assert abs(m.map - float(z["ref_map"])) <= 1e-15


def test_both_ops_are_bit_reproducible(dev):
    from mindrec_amd import ops
    rng = np.random.default_rng(11)
    n = 4097
    pred = torch.from_numpy((np.floor(rng.random(n) * 64) / 64).astype(np.float32)).to(dev)
    label = torch.from_numpy((rng.random(n) < 0.2).astype(np.float32)).to(dev)
    group = torch.from_numpy(rng.integers(0, 300, n).astype(np.int64) * (2 ** 33 + 1)).to(dev)
    a, b = ops.auc_counts(pred, label).clone(), ops.auc_counts(pred, label).clone()
    assert torch.equal(a, b)
    c, d = ops.group_rank_hist(pred, label, group).clone(), ops.group_rank_hist(pred, label, group).clone()
    assert torch.equal(c, d) and int(c[-1]) == int(torch.unique(group).numel())
