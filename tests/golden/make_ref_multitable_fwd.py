"""BUILD-CONTAINER-ONLY: the reference's own multitable model (unmodified, imported from /root/reference; see make_ref_fixtures.py for
what it runs on: compat/mindspore over the CPU kernel set tests/_ms_cpu_kernels.py) in evaluation:

  ref_multitable_fwd.npz   models/wide_and_deep_multitable/src/wide_and_deep.py: WideDeepModel (:146-427) under PredictWithSigmoid
                           (:617-650), its four tables at their hard-coded sizes (650 000 x 128, 17 300 x 64, 20 900 x 64, 16 x 64), the
                           5 x 1024 fp16 net; one batch of 256 samples, field counts 2 / 3 / 2, bags (3, 5, 4, 3, 4, 2)

The initial parameters are NOT stored (340 MB): both sides derive them by name from tests/_multitable_ref.py: ref_params
(tests/_ref_fixtures.py: cfgsize_param at ref_param_sigma); the generator puts them into the reference's model through
Parameter.set_data.  Stored: the batch (inputs by the reference's names), the 256 logits and probabilities the reference's code
computed, the parameters' shapes.  Data only, under 100 KB.  Usage: python tests/golden/make_ref_multitable_fwd.py"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_ref_fixtures as G  # noqa: E402  (sets up compat/mindspore + the CPU kernel set + the reference on sys.path)
import _multitable_ref as R  # noqa: E402
from mindspore import Tensor  # noqa: E402

B, N_IND, N_128, N_64, BAGS = 256, 2, 3, 2, (3, 5, 4, 3, 4, 2)
EXTRA = ("display_id", "ad_id", "display_ad_and_is_leak", "is_leak")


def make_batch(rng, vocab):
    b = {"label": (rng.random((B, 1)) < 0.3).astype(np.float32), "continue_val": rng.random((B, 32)).astype(np.float32),
         "indicator_id": rng.integers(0, vocab["emb64_indicator"], (B, N_IND)).astype(np.int32),
         "emb_128_id": rng.integers(0, vocab["emb128_embedding"], (B, N_128)).astype(np.int32),
         "emb_64_single_id": rng.integers(0, vocab["emb64_single"], (B, N_64)).astype(np.int32)}
    for key, L in zip(R.MULTI_KEYS, BAGS):
        b[key] = rng.integers(0, vocab["emb64_multi"], (B, L)).astype(np.int32)
        b[key + "_mask"] = (rng.random((B, L)) < 0.7).astype(np.float32)
    b["display_id"] = np.sort(rng.integers(0, B // 4, (B, 1)), axis=0).astype(np.int32)
    for k in EXTRA[1:]:
        b[k] = rng.integers(0, 2, (B, 1)).astype(np.int32)
    return b


def multitable_fwd(name="ref_multitable_fwd"):
    mt = G._ref_module("wide_and_deep_multitable", "wide_and_deep")
    cfg = types.SimpleNamespace(input_emb_dim=32 + N_IND * 64 + N_128 * 128 + N_64 * 64 + len(BAGS) * 64, batch_size=B, deep_layers_act="relu",
                                init_args=[-0.01, 0.01], weight_bias_init=["normal", "normal"], emb_init="normal", keep_prob=1.0,
                                dropout_flag=False)
    G.mindspore.set_seed(1000)
    net = mt.WideDeepModel(cfg)
    evaln = mt.PredictWithSigmoid(net)
    evaln.set_train(False)
    struct = dict(net.parameters_and_names())
    shapes = {k: [int(x) for x in p.shape] for k, p in struct.items()}
    for k, v in R.ref_params(shapes).items():
        struct[k].set_data(Tensor(v))
    batch = make_batch(np.random.default_rng(5150), {k: shapes[k][0] for k in ("emb64_indicator", "emb128_embedding", "emb64_single", "emb64_multi")})
    order = ["label", "continue_val", "indicator_id", "emb_128_id", "emb_64_single_id"]          # PredictWithSigmoid.construct's arguments
    for key in R.MULTI_KEYS:
        order += [key, key + "_mask"]
    logits, probs, label, display = evaln(*[Tensor(batch[k]) for k in order + list(EXTRA)])
    assert np.array_equal(G._np(label), batch["label"]) and np.array_equal(G._np(display), batch["display_id"])
    out = {"in/" + k: v for k, v in batch.items()}
    out.update(logits=G._np(logits).reshape(-1).astype(np.float32), probs=G._np(probs).reshape(-1).astype(np.float32),
               cfg=np.array(json.dumps(vars(cfg))), composition=np.array(json.dumps({"shapes": shapes, "multi_bags": list(BAGS), "argument_order": order})))
    G._save(name, out)
    return {"shapes": shapes, "logit_std": float(out["logits"].std()), "prob_std": float(out["probs"].std())}


if __name__ == "__main__":
    print(json.dumps(multitable_fwd(), indent=1, sort_keys=True))
