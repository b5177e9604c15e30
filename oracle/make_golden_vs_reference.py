"""TEST INFRASTRUCTURE ONLY -- records the reference's outputs for tests/test_oracle_vs_reference.py by importing and RUNNING THE
REFERENCE (Osilly/dynamic_llava, located and loaded by oracle/_ref_import.py):

    python -m oracle.make_golden_vs_reference       ->  tests/golden/oracle_vs_reference.npz

The cases use seeds and shapes that are NOT among oracle/make_golden.py's CASES.  The file holds only the reference's outputs; the
inputs are regenerated from the seeds below by oracle/fixtures.py, so the test needs nothing outside the repository."""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

from oracle import fixtures as fx

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "oracle_vs_reference.npz")

# (dtype, sparse overrides, n_sys, n_q, steps, seed): greedy-free teacher-forced loops through the reference's forward()
LOOP_CASES = [
    (torch.float32, {}, 4, 9, 5, 7),
    (torch.bfloat16, {}, 6, 5, 4, 8),
    (torch.float32, dict(vision_keep_rate=0.5, use_instruct_predictor=True), 3, 15, 3, 9),
]
# (padding side, tokenizer_model_max_length): prepare_inputs_labels_for_multimodal on a ragged batch of two prompts
PREP_CASES = [("right", None), ("left", None), ("right", 42), ("left", 42)]


def loop_inputs(dtype, sparse, n_sys, n_q, steps, seed):
    cfg = fx.tiny_config(**sparse)
    sd = fx.make_state_dict(cfg, seed=seed, predictor_gain=50.0)
    clip = fx.build_clip(cfg, seed=seed + 1)
    ids = fx.make_prompt(cfg, n_sys, n_q, seed=seed)[None]
    images = fx.make_images(cfg, 1, seed=seed)
    forced = fx.make_forced_tokens(cfg, steps + 1, 1, seed=seed)
    return cfg, sd, clip, ids, images, forced


def prep_inputs():
    cfg = fx.tiny_config()
    sd = fx.make_state_dict(cfg, seed=5, predictor_gain=50.0)
    clip = fx.build_clip(cfg, seed=6)
    prompts = [fx.make_prompt(cfg, 4, 9, seed=1), fx.make_prompt(cfg, 2, 5, seed=2)]
    W = max(p.shape[0] for p in prompts)
    ids = torch.zeros(2, W, dtype=torch.long)
    am = torch.zeros(2, W, dtype=torch.bool)
    for b, p in enumerate(prompts):
        ids[b, : p.shape[0]] = p
        am[b, : p.shape[0]] = True
    images = fx.make_images(cfg, 2, seed=3)
    pos = torch.arange(W)[None].repeat(2, 1)
    return cfg, sd, clip, ids, am, pos, images


def loop_key(i):
    return f"loop{i}"


def prep_key(side, tmax):
    return f"prep_{side}_{tmax}"


def main():
    from oracle._ref_import import import_reference
    from oracle.make_golden import build_reference_model, run_reference

    dll = import_reference()
    out = {}
    for i, case in enumerate(LOOP_CASES):
        cfg, sd, clip, ids, images, forced = loop_inputs(*case)
        ref = run_reference(dll, cfg, sd, clip, case[0], ids, images, case[4], forced)
        for name in ("step_logits", "position_ids", "len_last", "len_first"):
            out[f"{loop_key(i)}_{name}"] = ref[name]
    cfg, sd, clip, ids, am, pos, images = prep_inputs()
    for side, tmax in PREP_CASES:
        model = build_reference_model(dll, cfg, sd, clip, torch.float32)
        model.config.tokenizer_padding_side = side
        model.config.tokenizer_model_max_length = tmax
        with torch.inference_mode():
            (_, r_pos, r_am, _, r_emb, _), (r_idx,) = model.prepare_inputs_labels_for_multimodal(ids, pos, am, None, None, images)
        k = prep_key(side, tmax)
        out[f"{k}_emb"] = r_emb.numpy()
        out[f"{k}_am"] = r_am.numpy()
        out[f"{k}_pos"] = r_pos.numpy()
        out[f"{k}_idx"] = np.array(json.dumps([{s: [int(v[0]), int(v[1])] for s, v in d.items()} for d in r_idx]))
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    sys.exit(main())
