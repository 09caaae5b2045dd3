"""tests/golden/ref_multitable_fwd.npz -- the reference's own WideDeepModel + PredictWithSigmoid over one batch of 256, its four tables
at their real sizes and the 5 x 1024 fp16 net (tests/golden/make_ref_multitable_fwd.py) -- replayed through MultiTableWideDeep on the
GPU: the parameters loaded by the reference's names, the batch fed by the reference's input names.  Tolerance: 2e-2 on the
probabilities (tests/test_predict_fused_gpu.py's for a 16-bit net)."""
import numpy as np
import pytest
import torch

import _multitable_ref as R

pytestmark = pytest.mark.gpu


def test_product_replays_the_references_forward(dev, oracle):
    from mindrec_amd.multitable import MultiTableConfig, MultiTableWideDeep
    batch, ref_logits, ref_probs, params = R.load_fixture()
    net = MultiTableWideDeep(MultiTableConfig(n_indicator=2, n_emb128=3, n_emb64_single=2, multi_bags=(3, 5, 4, 3, 4, 2)))
    assert {k: tuple(v.shape) for k, v in net.params.items()} == {k: tuple(v.shape) for k, v in params.items()}
    net.load_parameters(params)
    logit, prob = net.predict_fused({k: torch.from_numpy(np.array(v)).to(dev) for k, v in batch.items()})
    d = np.abs(prob.view(-1).cpu().numpy().astype(np.float64) - ref_probs).max()
    print(f"max |dprob| = {d:.3e}, max |dlogit| = {np.abs(logit.view(-1).cpu().numpy() - ref_logits).max():.3e}")
    assert d <= 2e-2
