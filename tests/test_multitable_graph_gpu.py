"""MultiTableWideDeep.train_step with graphs="step" on the GPU, on the small model of tests/test_multitable_train_gpu.py (vocabularies
16 / 40 / 50 / 30, deep_dims (16, 8), B = 64): the fused chain, its capture and its replays against a graphs="none" twin that runs the
launch list one by one -- every parameter, every Adam m and v, every FTRL accum and linear and every step's loss bit for bit
(torch.equal).  Steps 1 - 2 at a batch shape run eagerly, step 3 captures, later steps replay on changing inputs."""
import functools

import numpy as np
import pytest
import torch

import _multitable_ref as R
import test_multitable_train_gpu as T

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def batch_np(seed, B=T.B):
    rng = np.random.default_rng(1000 + seed)
    b = {"continue_val": rng.random((B, 32)).astype(np.float32),
         "indicator_id": rng.integers(0, T.VOCAB["indicator"], (B, 2)).astype(np.int32),
         "emb_128_id": rng.integers(0, T.VOCAB["emb128"] - 4, (B, 3)).astype(np.int32),
         "emb_64_single_id": rng.integers(0, T.VOCAB["emb64_single"] - 4, (B, 2)).astype(np.int32)}
    for key, L in zip(R.MULTI_KEYS, T.BAGS):
        b[key] = rng.integers(0, T.VOCAB["emb64_multi"], (B, L)).astype(np.int32)
        b[key + "_mask"] = (rng.random((B, L)) < 0.7).astype(np.float32)
    b["label"] = (rng.random(B) < 0.4).astype(np.float32)
    return b


def dev_batch(seed, B=T.B):
    return {k: torch.from_numpy(v).cuda() for k, v in batch_np(seed, B).items()}


def state_of(net):
    out = {"p:" + k: v for k, v in net.params.items()}
    for t, (m, v) in net._opt["adam"].items():
        out["m:" + t], out["v:" + t] = m, v
    for w, (acc, lin) in net._opt["ftrl"].items():
        out["accum:" + w], out["linear:" + w] = acc, lin
    out["dense_m"], out["dense_v"] = net._net.dense_m, net._net.dense_v
    return out


def assert_same_state(a, b, what):
    sa, sb = state_of(a), state_of(b)
    assert set(sa) == set(sb)
    for k in sorted(sa):
        assert torch.equal(sa[k], sb[k]), (what, k)


def run_pair(mlp_dtype, schedule, hook=None):
    """graphs="step" and its graphs="none" twin over `schedule` [(seed, B)]: losses equal step by step, the state equal at the end"""
    net, twin = T.model(mlp_dtype, graphs="step"), T.model(mlp_dtype, graphs="none")
    for i, (seed, B) in enumerate(schedule):
        batch = dev_batch(seed, B)
        loss = net.train_step(batch, batch["label"]).clone()          # (a static buffer from the third step on)
        if hook is not None:
            hook(i, net)
        want = twin.train_step(dict(batch), batch["label"])
        assert torch.equal(loss, want), (mlp_dtype, i, float(loss), float(want))
    assert_same_state(net, twin, mlp_dtype)
    return net, twin


@pytest.mark.parametrize("mlp_dtype", ["fp16", "fp32"])
def test_six_steps_eager_capture_replay_against_the_twin(mlp_dtype):
    seen = []
    net, twin = run_pair(mlp_dtype, [(0, T.B), (1, T.B), (2, T.B), (3, T.B), (0, T.B), (1, T.B)],
                         hook=lambda i, n: seen.append(n._graph is not None))
    assert seen == [False, False, True, True, True, True]            # a graph exists behind the step: 1 - 2 eager, 3 captures, 4 - 6 replay
    assert twin._graph is None and "state" not in twin._opt                                 # "none" keeps its launch list and state
    # predict_fused after a replay sees the new parameters: a fresh model loaded with them gives the same bits
    from mindrec_amd.multitable import MultiTableWideDeep
    batch = dev_batch(2)
    logit, prob = net.predict_fused(batch)
    fresh = MultiTableWideDeep(T.make_cfg(mlp_dtype))
    fresh.load_parameters({k: v.clone() for k, v in net.params.items()})
    logit2, prob2 = fresh.predict_fused(batch)
    assert torch.equal(logit, logit2) and torch.equal(prob, prob2)
    net.close()


def test_another_batch_shape_in_the_middle_recaptures():
    seen = []
    sched = [(0, 64), (1, 64), (2, 64), (3, 64), (0, 128), (1, 128), (2, 128), (3, 128), (1, 64), (2, 64), (3, 64), (0, 64)]
    net, _ = run_pair("fp16", sched, hook=lambda i, n: seen.append(n._graph is not None))
    assert seen == [False, False, True, True] * 3                     # every change of shape: two eager steps, then a new capture
    net.close()


def test_release_close_and_the_context_manager():
    from mindrec_amd.multitable import MultiTableWideDeep
    net, twin = T.model("fp16", graphs="step"), T.model("fp16", graphs="none")

    def step(seed):
        batch = dev_batch(seed)
        loss = net.train_step(batch, batch["label"]).clone()
        assert torch.equal(loss, twin.train_step(dict(batch), batch["label"])), seed

    for seed in (0, 1, 2, 3):
        step(seed)
    first = net._graph["graph"]
    net.release_graphs()
    assert net._graph is None
    step(0)                                                           # re-captured at once: two steps at this shape have run
    assert net._graph is not None and net._graph["graph"] is not first
    step(1)
    net.close()
    assert net._graph is None
    step(2)                                                           # close() followed by train_step works
    step(3)
    assert_same_state(net, twin, "after release and close")
    with MultiTableWideDeep(T.make_cfg("fp16", graphs="step")) as m:
        m.load_parameters(T.named_params())
        for seed in (0, 1, 2, 3):
            batch = dev_batch(seed)
            m.train_step(batch, batch["label"])
        assert m._graph is not None
    assert m._graph is None


def test_bogus_graphs_value():
    with pytest.raises(ValueError, match="graphs"):
        T.model("fp16", graphs="bogus")


def test_replay_does_not_call_back_into_the_eager_chain(monkeypatch):
    from mindrec_amd import ops
    net, twin = T.model("fp16", graphs="step"), T.model("fp16", graphs="none")
    for seed in (0, 1, 2):
        batch = dev_batch(seed)
        net.train_step(batch, batch["label"])
        twin.train_step(dict(batch), batch["label"])
    assert net._graph is not None
    real = ops.multitable_input

    def boom(*a, **k):
        raise AssertionError("the replay issued the eager chain")

    monkeypatch.setattr(ops, "multitable_input", boom)
    losses = []
    for seed in (3, 0):
        batch = dev_batch(seed)
        losses.append(net.train_step(batch, batch["label"]).clone())
    monkeypatch.setattr(ops, "multitable_input", real)
    for seed, loss in zip((3, 0), losses):
        batch = dev_batch(seed)
        assert torch.equal(loss, twin.train_step(dict(batch), batch["label"]))
    assert_same_state(net, twin, "replays under the patch")
    net.close()
