"""tests/golden/ref_multitable_fwd.npz -- what the REFERENCE's own WideDeepModel + PredictWithSigmoid computed for one batch
(tests/golden/make_ref_multitable_fwd.py) -- replayed through the float64 restatement the GPU tests use as their oracle
(tests/_multitable_ref.py: model_forward).  This pins the restatement's reading of the Concat order, the field order, the wide sum and
the DenseLayer casts by the reference's code; tests/test_multitable_ref_fixture_gpu.py replays the same file through the product.

Tolerance: 2e-2 on the probabilities, what tests/test_predict_fused_gpu.py applies between a 16-bit net and another evaluation of it.
Both sides here are the same fp16 net -- operands, biases and layer outputs rounded to fp16 -- and differ in the accumulation of the
MatMuls alone (float64 here, the kernel set's there), so the measured figure (printed) is far inside it."""
import numpy as np

import _multitable_ref as R


def test_float64_restatement_replays_the_references_forward(oracle):
    batch, ref_logits, ref_probs, params = R.load_fixture()
    assert ref_probs.shape == (256,) and ref_probs.std() > 0.1, "the fixture does not spread over the sigmoid"
    logit, prob = R.model_forward(params, batch, "f16")
    d = np.abs(prob - ref_probs).max()
    print(f"max |dprob| = {d:.3e}, max |dlogit| = {np.abs(logit - ref_logits).max():.3e}")
    assert d <= 2e-2
    assert np.allclose(1.0 / (1.0 + np.exp(-ref_logits.astype(np.float64))), ref_probs, rtol=0, atol=1e-6)      # PredictWithSigmoid's sigmoid


def test_the_fixture_tells_a_wrong_order_apart(oracle):
    """the pin has teeth: with two multi-hot fields of equal bag length exchanged, or the single-hot blocks of two tables' rows taken
    in another order, the restatement leaves the reference's probabilities by more than the tolerance (2e-2)"""
    batch, _, ref_probs, params = R.load_fixture()
    a, b = "multi_doc_ad_category_id", "multi_doc_event_topic_id"                      # both bags of 3
    swapped = dict(batch)
    swapped[a], swapped[b], swapped[a + "_mask"], swapped[b + "_mask"] = batch[b], batch[a], batch[b + "_mask"], batch[a + "_mask"]
    assert np.abs(R.model_forward(params, swapped, "f16")[1] - ref_probs).max() > 2e-2
    rev = dict(batch)
    rev["indicator_id"] = batch["indicator_id"][:, ::-1].copy()
    assert np.abs(R.model_forward(params, rev, "f16")[1] - ref_probs).max() > 2e-2
