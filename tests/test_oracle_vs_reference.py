"""CPU: the oracle (oracle/ref_cpu.py) against outputs of the reference on seeds and shapes that are NOT among the golden cases of
oracle/make_golden.py.  The reference's outputs were recorded by running it (oracle/make_golden_vs_reference.py) into
tests/golden/oracle_vs_reference.npz; the inputs are regenerated here from the same seeds, so nothing outside the repository is read."""
import json
import os

import numpy as np
import pytest
import torch

from oracle.make_golden_vs_reference import LOOP_CASES, PREP_CASES, loop_inputs, loop_key, prep_inputs, prep_key
from oracle.ref_cpu import Oracle


@pytest.fixture(scope="module")
def recorded(golden_dir):
    return np.load(os.path.join(golden_dir, "oracle_vs_reference.npz"))


@pytest.mark.parametrize(
    "dtype,sparse,n_sys,n_q,steps,seed",
    [
        (torch.float32, {}, 4, 9, 5, 7),
        (torch.bfloat16, {}, 6, 5, 4, 8),
        (torch.float32, dict(vision_keep_rate=0.5, use_instruct_predictor=True), 3, 15, 3, 9),
    ],
)
def test_oracle_equals_live_reference(recorded, dtype, sparse, n_sys, n_q, steps, seed):
    case = (dtype, sparse, n_sys, n_q, steps, seed)
    cfg, sd, clip, ids, images, forced = loop_inputs(*case)
    k = loop_key(LOOP_CASES.index(case))
    ref = {name: recorded[f"{k}_{name}"] for name in ("step_logits", "position_ids", "len_last", "len_first")}
    assert ref["step_logits"].shape[0] == steps + 1
    o = Oracle(cfg, sd, dtype, clip=clip, tie_break="torch")  # argsort called exactly as the reference does (DML:1902-1908): ties included
    pkv, cur = None, ids
    with torch.no_grad():
        for j in range(steps + 1):
            logits, pkv = o.forward(cur, images=images.to(dtype) if j == 0 else None, past_key_values=pkv)
            np.testing.assert_array_equal(logits[:, -1].float().numpy(), ref["step_logits"][j], err_msg=f"step {j}")
            if j == 0:
                np.testing.assert_array_equal(o.records["position_ids"].numpy(), ref["position_ids"])
            np.testing.assert_array_equal(pkv[1][-1].numpy(), ref["len_last"][j])
            np.testing.assert_array_equal(pkv[1][0].numpy(), ref["len_first"][j])
            cur = forced[j][:, None]


@pytest.mark.parametrize("side,tmax", [("right", None), ("left", None), ("right", 42), ("left", 42)])
def test_oracle_prepare_inputs_padding_and_truncation_equal_live_reference(recorded, side, tmax):
    """ARCH:493-579 -- tokenizer_model_max_length truncation and left / right padding of a ragged batch: embeddings, attention mask,
    position ids and the (shifted / clamped) segment dicts, bit for bit against the reference."""
    assert (side, tmax) in PREP_CASES
    cfg, sd, clip, ids, am, pos, images = prep_inputs()
    k = prep_key(side, tmax)
    r_emb, r_am, r_pos = recorded[f"{k}_emb"], recorded[f"{k}_am"], recorded[f"{k}_pos"]
    r_idx = json.loads(str(recorded[f"{k}_idx"]))
    cfg.tokenizer_padding_side = side
    cfg.tokenizer_model_max_length = tmax
    o = Oracle(cfg, sd, torch.float32, clip=clip)
    with torch.no_grad():
        (_, o_pos, o_am, _, o_emb, _), (o_idx,) = o.prepare_inputs_labels_for_multimodal(ids, pos, am, None, None, images)
    np.testing.assert_array_equal(o_emb.numpy(), r_emb)
    np.testing.assert_array_equal(o_am.numpy(), r_am)
    np.testing.assert_array_equal(o_pos.numpy(), r_pos)
    assert [{k: list(v) for k, v in d.items()} for d in o_idx] == r_idx
