"""The float64 per-operation references the GPU kernel tests use (tests/gpt2_ops_ref.py), composed into the whole model with a KV cache,
reproduce oracle/gpt2_ref.forward — the oracle that is itself pinned to the reference model's fixture.  CPU only."""
import numpy as np
import pytest
import torch

import gpt2_ops_ref as R
from clip_glass_amd import synth
from oracle import gpt2_ref


@pytest.mark.parametrize("n_embd,n_prefill", [(128, 5), (128, 1), (64, 7)])
def test_composed_op_references_match_the_oracle_forward(n_embd, n_prefill):
    sd = synth.make_state(synth.gpt2_spec(n_embd=n_embd, n_layer=2, vocab=2048, n_positions=64), 2)
    tok = np.random.RandomState(3).randint(0, 2048, size=(3, 11)).astype(np.int64)
    got = R.forward_cached(sd, tok, n_prefill, Tmax=16)
    with torch.no_grad():
        ref, _ = gpt2_ref.forward({k: torch.as_tensor(v) for k, v in sd.items()}, torch.tensor(tok))
    assert got.shape == tuple(ref.shape) and np.isfinite(got).all()
    np.testing.assert_allclose(got, ref.numpy(), rtol=2e-4, atol=2e-5)


def test_block_pairs_picks_the_lowest_index_on_ties():
    lg = np.zeros((2, 70), dtype=np.float32)
    lg[0, [5, 9, 40]] = 3.0
    lg[1, 69] = 1.0
    pv, pi = R.block_pairs(lg)
    assert pv.shape == (2, 3) and pi.tolist() == [[5, 40, 64], [0, 32, 69]] and pv.tolist() == [[3.0, 3.0, 0.0], [0.0, 0.0, 1.0]]
