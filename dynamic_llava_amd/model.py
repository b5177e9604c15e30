"""Host side of the MI355X-native Dynamic-LLaVA hot path: same API surface as the reference's
`DynamicLlavaLlamaForCausalLM` (llava/model/language_model/dynamic_llava_llama.py:50-169), different engine.

What stays on PyTorch-ROCm (per BASELINE.json north_star): CLIP ViT-L/14-336 + mm_projector, the embedding
lookup and the dense decoder GEMMs (fused QKV, O, fused gate|up, down, lm_head -> hipBLASLt/MFMA).
Everything else on the path is a hand-written HIP kernel behind the C ABI (include/dynllava.h):
RMSNorm(+residual), RoPE+KV append, varlen prefill attention, ragged split-KV decode attention, SiLU*up,
vision predictor, top-k select, token compaction, text predictor + eviction decision, greedy/advance.

This file is the API shell (construction, finalize(), forward(), generate(), score()); the parameter tree and the vision side live in modules.py, the prompt layout /
prefill planner / layer loop in prefill.py (PrefillEngine), the decode-step builders and their schedule in decode.py (DecodeScheduler) -- mixins of the one class the
reference's harness sees.  generate() reads: parse + route (request.py), layout and prefill (prefill.py), arm and decode loop (decode.py), _score / _finish (here).

Design (not a translation of the reference's op sequence):
  * activations are PACKED varlen [total_tokens, H] + cu_seqlens, never padded [B, N, H];
  * after layer `sparse_layer` the packed batch is physically compacted (k image tokens per row survive);
  * KV lives in a pre-allocated slab with device-side per-row lengths (cache.py); eviction = "do not
    advance the length"; the decode step has zero host syncs and is captured in a hipGraph;
  * all prefill shapes are host-known (k is constant per row), so prefill has no device->host sync either
    apart from reading `input_ids` (which the harness hands over on the GPU).
"""
from __future__ import annotations

import copy
import dataclasses
import operator
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import hip_ops as ops
from . import constraints, guidance, logprobs, request, sampling, scoring, stopping
from .cache import KVSlabCache
from .config import IGNORE_INDEX, IMAGE_TOKEN_INDEX, DynamicLlavaConfig

from .decode import DecodeScheduler, StepMode, _DecodeState, no_gc_during_capture  # noqa: F401
from .modules import (CLIPVisionTower, CausalLMOutputWithPast, DynamicLlamaDecoderLayer, DynamicLlavaLlamaModel, TextPredictor,  # noqa: F401 (re-exported:
                      VisionPredictor)  # tests, tools and the package's lazy attributes import these names from here)
from .prefill import USER_IDS, PrefillEngine  # noqa: F401

_DATA_PTR, _VERSION = operator.methodcaller("data_ptr"), operator.attrgetter("_version")


class DynamicLlavaLlamaForCausalLM(PrefillEngine, DecodeScheduler, nn.Module):
    """Drop-in for the reference class of the same name (dynamic_llava_llama.py:50-169)."""

    def __init__(self, config: DynamicLlavaConfig, with_vision_tower=True):
        super().__init__()
        self.config = config
        self.model = DynamicLlavaLlamaModel(config, with_vision_tower)
        self.vocab_size = config.vocab_size
        self.lm_head = nn.Linear(config.hidden_size, config.vocab_size, bias=False)
        self._packed = False
        self._rope = None
        self._dstate = None
        self._mode = StepMode()
        self._prefill_graphs = {}
        self._prefill_pool = None
        self._fork_src_pool = None  # generate(num_return_sequences=n): the B-row cache the prompts are prefilled into before dl_kv_fork (decode._fork_source)
        # captured prefill shapes kept (LRU).  288 GB of HBM: the graphs share one memory pool, an entry costs its static inputs (~0.7 MB of
        # pixels) and the graph object
        self.max_prefill_graphs = 64
        self.prefill_width_bucket = int(os.environ.get("DL_WIDTH_BUCKET", "16"))  # see _width_bucket
        self.use_hip_graph = True  # (DL_USE_HIP_GRAPH=0 in the environment forces every launch eager, whatever is assigned here: see the property)
        self.attn_inkernel_combine = True  # decode attention: split 0's workgroup merges the split-KV partials inside the launch (no combine launch)
        self.device_prompt_layout = True  # generate(): un-padded one-image-per-row prompts are laid out by a device kernel (no device->host copy)
        self.tp_side_stream = False  # run the text predictor as a parallel graph branch (measured slower: see DESIGN.md)
        self.gemv_max_decode_batch = 3  # B <= this: decode GEMMs run as hand-written weight-streaming GEMVs (dl_gemv)
        # B <= this (and past the GEMV range): dl_gemm_smallm; larger batches use the library GEMM.  tools/bench_decode_batch.py: 3.87 / 3.95 /
        # 4.24 ms per step at B = 4 / 8 / 16 against 5.1-5.3 on the library; a wash at 20-24 (4.64 / 4.80 vs 4.66 / 4.75) where the hand-written
        # path is kept for being deterministic and batch-invariant; 4 % behind at 32 (5.09 vs 4.89)
        self.smallm_max_decode_batch = 32
        self.fuse_qkv_attn = os.environ.get("DL_FUSE_QKV_ATTN", "1") == "1"
        self.fuse_gu_tp = os.environ.get("DL_FUSE_GU_TP", "1") == "1"
        # batch-1 decode, bf16: o_proj, gate|up, down_proj and the vocabulary projection stream losslessly packed 12-bit weights (bf16pack.py, dl_gemv_pk) --
        # the same bits out, ~0.79 of the bytes in.  The packed copies are made by finalize(); DL_WEIGHT_PACK=0: not made, not used
        self.decode_weight_pack = os.environ.get("DL_WEIGHT_PACK", "1") == "1"
        # ... o_proj and down_proj too.  Off: their packed launches (x in registers, one short stream per launch) measured no faster than the bf16 ones
        # (o 6.8 vs 6.7 us, down 17.0 vs 16.3 us), so only gate|up and the vocabulary projection are packed by default (down_proj's long
        # rows have since got a faster packed kernel and a knob of their own, decode_weight_pack_down below)
        self.decode_weight_pack_plain = os.environ.get("DL_WEIGHT_PACK_PLAIN", "0") == "1"
        # ... and every layer's q|k|v, which streams inside the fused q|k|v + attention launch (dl_gemv_qkv_attn_pk; the unfused launch: dl_gemv_pk).  The copy is
        # kept as layer.pk_qkv, beside layer.pk.  DL_WEIGHT_PACK_QKV=0: not made, not used (+2.5 GB of copies at 7B when on)
        self.decode_weight_pack_qkv = os.environ.get("DL_WEIGHT_PACK_QKV", "1") == "1"
        # ... and every layer's down_proj with long rows (K > 8192: 7B 11008, 13B 13824), whose packed launch keeps x in LDS at four workgroups per CU and beats
        # the bf16 one by 1.2-1.7 us at K = 11008 (stage 3).  The copy is kept as layer.pk_down, beside layer.pk (with decode_weight_pack_plain it IS
        # layer.pk["down"]).  DL_WEIGHT_PACK_DOWN=0: not made, not used (+2.3 GB of copies at 7B when on)
        self.decode_weight_pack_down = os.environ.get("DL_WEIGHT_PACK_DOWN", "1") == "1"
        # attention workgroups per head inside the fused launch: up to this many, one per 128 keys of the scheduled bound (DL_QA_SPLITS=1: always one)
        self.fused_attn_max_splits = max(1, min(4, int(os.environ.get("DL_QA_SPLITS", "4"))))  # the kernel takes 1..4 (kQaMaxSplits)
        self.gu_grid_cap = int(os.environ.get("DL_GU_GRID", "0"))  # workgroups of the batch-1 gate|up launch (0: the kernel's default, 1024)
        self.qkv_attn_grid_cap = int(os.environ.get("DL_QA_GRID", "0"))  # workgroups of the fused q|k|v + attention launch (0: the kernel's default)
        # o_proj of the post-compaction prefill layers (<= 192 rows) on dl_linear_splitk like down_proj: 17.3 vs 18.4-22 us per layer, prefill
        # 9.35 -> 9.17 ms (A/B on one box); DL_SPLITK_O=0 restores the library GEMM
        self.splitk_o_proj = os.environ.get("DL_SPLITK_O", "1") == "1"
        # round 5: q|k|v and gate|up (+ SiLU * up) of prefill layers with <= 256 packed rows on dl_linear_packed (operand-order weight copies made by
        # finalize(), activations handed over in fragment order by the norm launch that produces them).  tools/bench_linear_packed.py, M = 170:
        # q|k|v 36.2 us (two k ranges per unit set) vs the library's 41.4, gate|up + SiLU * up 57.2 vs 64.1.  DL_PACKED_GEMM=0: library GEMMs.
        self.packed_prefill_gemm = os.environ.get("DL_PACKED_GEMM", "1") == "1"
        # round 6: o_proj at <= 256 rows (post-compaction prefill layers, decode batches from `tiles_o_proj_min_decode_batch` rows) on dl_linear_tiles' partial sums
        # OFF by default: 10 % on the launch pair at M = 170, not visible in the prefill (8.26-8.42 ms with and without, box to box) and 1.07 GB of copies at 7B
        self.tiles_o_proj = os.environ.get("DL_TILES_O", "0") == "1"
        # (tools/bench_linear_tiles.py --oproj, with the consumer launch: M = 170 23.6 vs 26.4 us for dl_linear_splitk, M = 192 24.7 vs 26.4, M = 117 22.9 vs 24.0 but the library's 21.4;
        # 32 rows 17.3 vs 18.1 for dl_gemm_smallm, 16 rows 16.8 vs 16.1: used for 129..256 prefill rows; decode batches stay where they were -- 33 = off)
        self.tiles_o_proj_min_decode_batch = int(os.environ.get("DL_TILES_O_MIN_B", "33"))
        self.packed_down_proj = os.environ.get("DL_PACKED_DOWN", "1") == "1"  # down_proj too (partial sums for dl_add_rmsnorm_parts): A/B knob
        # batched decode (4..32 rows), tools/bench_decode_batch.py: the MLP on dl_linear_packed from 4 rows on (B = 16: 4.05 -> 3.79 ms per step, 24: 4.63 -> 4.03), q|k|v too from 16 rows
        # on (24: 4.05 -> 3.97, 32: 4.21 -> 4.11); o_proj stays on dl_gemm_smallm's partial sums up to 32 rows (against the library GEMM + add: 32 rows 4.20 -> 4.11)
        self.packed_decode_qkv_min_batch = int(os.environ.get("DL_PACKED_DECODE_QKV_MIN_B", "16"))
        self.packed_decode_qkv_parts = os.environ.get("DL_PACKED_DECODE_QKV_PARTS", "1") != "0"  # ... as fp32 partial sums of its two k ranges, added by dl_attn_decode_rope_parts
        self.packed_decode_qkv_parts_max_batch = int(os.environ.get("DL_PACKED_DECODE_QKV_PARTS_MAX_B", "24"))  # (tools/bench_decode_qkv_parts.py: -2.2 % per step at 16 rows, -1.8 % at 24; at 32 rows -0.6 % on equal prompts but +0.5 % on configs[2]'s ragged batch)
        self.packed_decode_mlp_min_batch = int(os.environ.get("DL_PACKED_DECODE_MLP_MIN_B", "4"))
        self.packed_qkv_parts = os.environ.get("DL_PACKED_QKV_PARTS", "1") == "1"  # prefill q|k|v: partial sums added by the RoPE / KV-append launch instead of the in-launch hand-over
        self.packed_decode_mlp = os.environ.get("DL_PACKED_DECODE_MLP", "1") == "1"  # decode batches 4..32: gate|up + SiLU * up and down_proj on dl_linear_packed
        self._lp_ws = None   # hand-over workspace of the k-split launches (zeroed once; the kernel leaves its flag words zero)
        self._lp_err = None  # bit 3: a reducing wave of dl_linear_packed gave up waiting
        # split-K slices of the two WIDE projections (q|k|v, gate|up: 768 / 1376 sixteen-neuron wave tiles without any split) on dl_gemm_smallm; 0 = the
        # kernel's own choice (8 / 4).  Round 4 measured the review's proposal -- fewer slices, so the consumers re-read fewer fp32 partial slabs --
        # and it LOSES at every batch: 2 slices 4.09 / 4.39 / 4.65 / 4.94 ms per step at B = 8 / 16 / 24 / 32 against 3.71 / 4.04 / 4.60 / 4.87 (library
        # 5.03 / 5.20 / 4.64 / 4.80): many short weight streams beat few long ones by more than the partial traffic costs (tools/bench_decode_batch.py)
        self.smallm_wide_slices = int(os.environ.get("DL_SMALLM_WIDE_SLICES", "0"))
        if os.environ.get("DL_SMALLM_MAX_B"):  # tuning experiments only
            self.smallm_max_decode_batch = int(os.environ["DL_SMALLM_MAX_B"])
        self.record_timing = False  # generate(): HIP events around the prefill / decode parts -> self.last_timing (tools/bench_varlen_stream.py)
        self.last_timing = None
        self.decode_sync_every = int(os.environ.get("DL_SYNC_EVERY", "8"))  # decode steps per chunk of the schedule (KVSlabCache.sched_*)
        self.force_text_decision = None  # tests only: forward() decode keeps / evicts the step's token as given, see forward()
        self.single_split_keys_override = None  # tests only: see _single_split_max_keys
        self.min_keys_per_split = 64  # tests only: KVSlabCache.min_keys_per_split of the caches this model schedules
        self.debug_records = None  # dict filled by forward passes when set to {} (tests)
        self.decode_weight_format = None  # "mxfp8": see set_decode_weight_format()
        # MXFP8 only: decode steps of gemv_max_decode_batch < B <= this many rows stream the codes too (dl_gemm_mx8); None: the codes are used in the GEMV range only
        self.mx8_max_decode_batch = None
        self.kv_cache_format = None  # "mxfp8": see set_kv_cache_format()
        self.eval()

    # ---- reference surface -----------------------------------------------------------------
    def get_model(self):
        return self.model

    def get_vision_tower(self):
        return self.model.get_vision_tower()

    @property
    def device(self):
        return self.lm_head.weight.device

    @property
    def dtype(self):
        return self.lm_head.weight.dtype

    def encode_images(self, images):  # dynamic_llava_arch.py:163-166
        f = self.get_vision_tower()(images)
        return self._project(f.to(self.dtype))

    def _pack_projector(self):
        """Operand-order copies of the mlp2x_gelu projector's two weights for dl_linear_tiles (multimodal_projector/builder.py:172-179; +42 MB at 7B)."""
        pj = self.model.mm_projector
        self._proj_tiles = None
        vt = self.get_vision_tower()
        ws = (pj[0].weight, pj[2].weight)
        if (vt is None or vt.tiles_gemm) and all(w.is_cuda and ops.linear_tiles_ok(1, w.shape[0], w.shape[1], w.dtype) for w in ws) and pj[0].weight.shape[0] % 64 == 0:
            self._proj_tiles = tuple(ops.pack_weight_tiles(w.detach().contiguous()) for w in ws)
        self._proj_src = [(w.data_ptr(), w._version) for w in ws]

    def _project(self, f):
        """mm_projector(f): Linear -> GELU -> Linear.  16-bit models, up to `tiles_max_batch` images: both Linears on dl_linear_tiles, the GELU in the first one's
        epilogue, the intermediate in fragment order (2 launches instead of 3 library launches)."""
        pj = self.model.mm_projector
        vt = self.get_vision_tower()
        if getattr(self, "_proj_src", None) != [(w.data_ptr(), w._version) for w in (pj[0].weight, pj[2].weight)]:
            self._pack_projector()
        B = f.shape[0] if f.dim() == 3 else 1
        if self._proj_tiles is None or f.dtype != pj[0].weight.dtype or not f.is_cuda or B > (vt.tiles_max_batch if vt is not None else 1) or pj[0].bias is None or pj[2].bias is None:
            return pj(f)
        C = f.shape[-1]
        x = f.reshape(-1, C)  # a view for one image (the CLS row is skipped by the offset), a copy for several
        if x.stride(1) != 1 or x.stride(0) % 8 or x.data_ptr() % 16:
            x = x.contiguous()
        M, H1, H2 = x.shape[0], pj[0].weight.shape[0], pj[2].weight.shape[0]
        g = ops.linear_tiles(x, self._proj_tiles[0], H1, bias=pj[0].bias, epilogue=ops.LT_GELU, y_packed=True)
        y = ops.linear_tiles(g, self._proj_tiles[1], H2, bias=pj[2].bias, x_packed_mk=(M, H1))
        return y.view(*f.shape[:-1], H2)

    def finalize(self):
        """Call once after weights are loaded / moved: fuses QKV and gate|up, builds the RoPE table."""
        ops.require_gpu()
        if self.device.type != "cuda":
            raise ops.HipOpsError("the model must live on the GPU (no CPU path exists)")
        if self.decode_weight_format == "mxfp8":
            self._quantize_decoder_weights()  # W -> W' in place, BEFORE anything below copies the weights
        for l in self.model.layers:
            l.pack(operand_copies=self.packed_prefill_gemm, o_copy=self.tiles_o_proj)  # (weights replaced later: call finalize() again -- the operand-order copies are made here)
        self._lp_err = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._lp_ws = None
        if any(l.wp_qkv is not None for l in self.model.layers):
            # hand-over workspace of the k-split launches, sized for the largest call this model makes (256 rows, the wider of the two projections);
            # allocated HERE, once: a captured prefill must never allocate it
            cfg = self.config
            need = 256
            for n_, pr in (((cfg.num_attention_heads + 2 * cfg.num_key_value_heads) * cfg.head_dim, False), (2 * cfg.intermediate_size, True)):
                nu_, ks_ = self._lp_config(n_ // 16, pr)
                ws_ = ops.linear_packed_workspace(256, n_, cfg.hidden_size, self.device, ops.LP_SILU_PAIR if pr else ops.LP_STORE, nu_, ks_)
                need = max(need, 0 if ws_ is None else ws_.numel())
            self._lp_ws = torch.zeros(need, dtype=torch.uint8, device=self.device)
        if self.get_vision_tower() is not None:
            self.get_vision_tower().pack()
        self._pack_projector()
        self._fp_params = [w for l in self.model.layers for w in (l.self_attn.q_proj.weight, l.self_attn.k_proj.weight, l.self_attn.v_proj.weight, l.self_attn.o_proj.weight,
                                                                   l.mlp.gate_proj.weight, l.mlp.up_proj.weight, l.mlp.down_proj.weight)]
        self._fp_params.append(self.lm_head.weight)  # (its packed copy below is detached from the parameter like the operand-order copies)
        self._fp = self._weights_fingerprint()
        for l in self.model.layers:  # the decode step's MXFP8 codes of the fused weights (quantising W' reproduces W''s codes: nothing is written)
            l.mx8 = None
            if self.decode_weight_format == "mxfp8":
                l.mx8 = {"qkv": ops.quantize_mx8(l.w_qkv), "o": ops.quantize_mx8(l.self_attn.o_proj.weight.data.contiguous()), "gu": ops.quantize_mx8(l.w_gu),
                         "down": ops.quantize_mx8(l.mlp.down_proj.weight.data.contiguous())}
        self._pack_decode_weights()
        self._packed = True
        self._build_rope(self.config.max_position_embeddings)
        self._dstate = None
        self._prefill_graphs = {}  # captured prefills hold the pointers of the tensors packed above
        return self

    # ---- MXFP8 decoder weights -------------------------------------------------------------------
    def set_decode_weight_format(self, fmt, max_batch=None):
        """Select the weight format the small-batch decode step streams.  None (default): the model dtype.  "mxfp8": OCP MXFP8 (mxfp8.py).

        "mxfp8" quantises every decoder layer's q|k|v, o_proj, gate|up and down_proj weight and OVERWRITES the parameters in place with
        W' = dequantize(quantize(W)), which is exact in the model dtype; finalize() then rebuilds every copy (operand-order copies, fingerprint, captured
        graphs) from W', and the MXFP8 codes are kept beside the weights (layer.mx8).  The model is from then on exactly the model-dtype model with weights W':
        prefill, CLIP, the projector, decode batches above gemv_max_decode_batch, use_cache=False and chunk-on-cache run their usual kernels on W'; decode
        steps of <= gemv_max_decode_batch rows run the four projections on dl_gemv_mx8 (the lm_head, the predictors, embeddings and norms stay in the model
        dtype).  Quantisation is idempotent (quantising W' again gives the same codes) but NOT reversible: set_decode_weight_format(None) restores the
        model-dtype kernels, not W.  A decoder weight changed afterwards (load_state_dict, in-place edits) is re-quantised -- W'' = quantize(new W) overwrites
        it -- by the next finalize(), which the weight-fingerprint check of generate() / forward() runs: FP8 codes of old weights are never served.
        The lm_head, the CLIP tower and the KV cache are not quantised.  Extra memory: decode_weight_bytes().

        max_batch (None, or gemv_max_decode_batch .. 32; "mxfp8" only): decode steps of gemv_max_decode_batch < B <= max_batch rows ALSO stream the codes -- the
        four projections run on dl_gemm_mx8 (q|k|v into dl_attn_decode_rope, o_proj / down_proj as fp32 partial sums into dl_add_rmsnorm_parts, gate|up into
        dl_silu_mul_parts) when the kernel takes all four shapes (16-bit model dtype, K % 256 == 0, N % 4 == 0; otherwise the step silently keeps its model-dtype
        kernels).  None (default): such steps run the model-dtype kernels on W'.  Larger batches, prefill, use_cache=False and chunk-on-cache are unaffected."""
        from .mxfp8 import check_decode_weight_format

        check_decode_weight_format(fmt, max_batch, self.gemv_max_decode_batch)
        self.decode_weight_format = fmt
        self.mx8_max_decode_batch = None if max_batch is None else int(max_batch)
        self._packed = False
        return self.finalize()  # (drops the decode state and its captured graphs: their keys and pointers belong to the old format)

    # ---- MXFP8 KV cache ---------------------------------------------------------------------------
    def set_kv_cache_format(self, fmt):
        """Select the storage format of the KV cache this model allocates.  None (default): the model dtype.  "mxfp8": the kept keys (after RoPE) and values are
        stored as MXFP8 codes along head_dim (cache.KVSlabCacheMX8: d + d/32 bytes per row, 0.516 of a 16-bit slab at d = 128; 0.26 of an fp32 one).

        The prefill is unchanged arithmetic -- its attention reads K/V from the packed projection -- and appends through a one-layer model-dtype scratch slab that
        dl_kv_quantize_mx8 moves into the layer's planes, so prefill logits are bit-identical to the format-off model's.  Decode steps run dl_attn_decode_rope_kv8:
        the new token is attended exactly and stored quantised, older rows are read as their dequantised values (exact in the model dtype).  The fused batch-1
        q|k|v + attention launch and the partial-sum attention launch are not used in this mode (the unfused branches run, as with MXFP8 weights).  Orthogonal to
        set_decode_weight_format.  Not built in this mode (NotImplementedError): a multi-token chunk on a non-empty cache and generate(past_key_values=...).
        use_cache=False is unaffected.  Changing the format drops the pooled cache and every graph captured on it."""
        from .mxfp8 import check_kv_cache_format

        check_kv_cache_format(fmt)
        if fmt != self.kv_cache_format:
            self.kv_cache_format = fmt
            self._cache_pool = None
            self._fork_src_pool = None
            self._dstate = None
            self._prefill_graphs = {}
        return self

    def _pack_decode_weights(self):
        """The 12-bit packed copies (bf16pack.pack) of the matrices the batch-1 decode step streams through dl_gemv_pk: every layer's gate|up and the vocabulary
        projection; with decode_weight_pack_plain also o_proj and down_proj.  Rebuilt by every finalize() -- i.e. whenever the weight fingerprint (lm_head included) moves -- and dropped
        for MXFP8 decoder weights, whose step streams the codes.  A matrix the kernel does not take (gemv_pk_ok) or that would not shrink below 0.9 of its
        size (pack() returns None) keeps its model-dtype launch.  With decode_weight_pack_qkv every layer's q|k|v is packed too, under the same rules, as
        layer.pk_qkv (not part of layer.pk: the fused q|k|v + attention launch streams it through dl_gemv_qkv_attn_pk), and with decode_weight_pack_down every
        layer's down_proj with K > 8192 as layer.pk_down (the same object as layer.pk["down"] where decode_weight_pack_plain has made that one)."""
        from . import bf16pack

        for l in self.model.layers:
            l.pk = None
            l.pk_qkv = None
            l.pk_down = None
        self._pk_lm_head = None
        if not self.decode_weight_pack or self.decode_weight_format is not None or self.dtype != torch.bfloat16:
            return
        A = ops.GEMV_ADDNORM
        pk = lambda w, mode: bf16pack.pack(w) if ops.gemv_pk_ok(mode, w.shape[1], w.dtype) else None
        plain = self.decode_weight_pack_plain
        for l in self.model.layers:
            l.pk = {"o": pk(l.self_attn.o_proj.weight.data, ops.GEMV_PLAIN) if plain else None, "gu": pk(l.w_gu, A),
                    "down": pk(l.mlp.down_proj.weight.data, ops.GEMV_PLAIN) if plain else None}
            if self.decode_weight_pack_qkv:
                l.pk_qkv = pk(l.w_qkv, A)
            if self.decode_weight_pack_down and l.mlp.down_proj.weight.shape[1] > 8192:
                l.pk_down = l.pk["down"] if plain else pk(l.mlp.down_proj.weight.data, ops.GEMV_PLAIN)
        self._pk_lm_head = pk(self.lm_head.weight.data, A)

    def weight_pack_bytes(self) -> dict:
        """Bytes of the packed decode copies kept beside the parameters, and of the bf16 matrices they stand for."""
        from . import bf16pack

        ps = [p for l in self.model.layers for p in (getattr(l, "pk", None) or {}).values() if p is not None]
        if getattr(self, "_pk_lm_head", None) is not None:
            ps.append(self._pk_lm_head)
        qs = [l.pk_qkv for l in self.model.layers if getattr(l, "pk_qkv", None) is not None]
        # (a pk_down that is layer.pk["down"] is counted there, once)
        ds = [l.pk_down for l in self.model.layers if getattr(l, "pk_down", None) is not None and l.pk_down is not (l.pk or {}).get("down")]
        side = lambda xs: {"matrices": len(xs), "packed": sum(bf16pack.packed_nbytes(p) for p in xs), "bf16": sum(bf16pack.raw_nbytes(p) for p in xs)}
        return {"matrices": len(ps), "packed": sum(bf16pack.packed_nbytes(p) for p in ps), "bf16": sum(bf16pack.raw_nbytes(p) for p in ps), "qkv": side(qs), "down": side(ds)}

    def _quantize_decoder_weights(self):
        from .mxfp8 import dequantize_mx8

        for l in self.model.layers:
            a, m = l.self_attn, l.mlp
            for lin in (a.q_proj, a.k_proj, a.v_proj, a.o_proj, m.gate_proj, m.up_proj, m.down_proj):  # (blocks run along K inside a row: the fused weights give the same codes)
                w = lin.weight.data
                q, sc = ops.quantize_mx8(w.contiguous())
                w.copy_(dequantize_mx8(q, sc, w.dtype))

    def decode_weight_bytes(self) -> dict:
        """Bytes the decode weight format keeps beside the parameters (MXFP8: codes + one scale byte per 32 weights of the four decoder projections).
        The same with and without set_decode_weight_format's max_batch: dl_gemm_mx8 reads the one row-major copy of the codes.  The operand-order weight copies
        of the model-dtype GEMMs (+11.9 GB at 7B) are still made in this mode -- the prefill runs on them -- and are not counted here."""
        nb = lambda t: t.numel() * t.element_size()
        mx8 = sum(nb(q) + nb(sc) for l in self.model.layers for q, sc in (getattr(l, "mx8", None) or {}).values())
        return {"format": self.decode_weight_format, "mxfp8": mx8, "total": mx8}

    def _build_rope(self, n_pos):
        """dynamic_modeling_llama.py:152-174,181-184: fp32 cos/sin of cat(freqs, freqs), rounded to the model dtype."""
        d, dev = self.config.head_dim, self.device
        inv_freq = 1.0 / (self.config.rope_theta ** (torch.arange(0, d, 2, device=dev).float() / d))
        t = torch.arange(n_pos, device=dev, dtype=torch.float32)
        emb = torch.cat((torch.outer(t, inv_freq),) * 2, dim=-1)
        self._rope = (emb.cos().to(self.dtype).contiguous(), emb.sin().to(self.dtype).contiguous())

    def _rope_tables(self, need):
        if self._rope is None or self._rope[0].shape[0] < need:
            self._build_rope(max(need, self.config.max_position_embeddings))
            self._dstate = None  # table pointers changed -> re-capture
        return self._rope

    # ---- decoder engine -----------------------------------------------------------------------
    def _check_ready(self, weights=True):
        if not self._packed:
            raise ops.HipOpsError("call model.finalize() after loading weights (done by the builders)")
        if not weights:
            return
        # the operand-order copies are detached from the parameters.  A load_state_dict() / an in-place edit / a replaced `.data` after
        # finalize() would otherwise leave the packed prefill and the packed decode batches on the OLD weights while the GEMV / library paths use the new ones
        # -- path-dependent results with no error.  (data_ptr, _version) of every decoder projection weight is compared and the model
        # re-finalized when one moved.  Checked by generate() and by every forward() that starts a sequence (0.1 ms: 224 parameters at 7B).
        if self._weights_fingerprint() != self._fp:
            self._packed = False
            self.finalize()

    @staticmethod
    def _tiles_o_config(rows, n_out):
        """(tile_shape, k_split) of o_proj on dl_linear_tiles' partial-sum form: up to 8 row tiles as ONE row block, more as two; 8 units (128 neurons) per workgroup;
        as many k ranges (<= 8) as keep one round of workgroups on the 256 CUs."""
        rt = (rows + 15) // 16
        n_mb = 1 if rt <= 8 else 2
        tm = -(-rt // n_mb)
        tm = {5: 6}.get(tm, tm)  # (5 row tiles are built with every epilogue under another shape code; 6 wastes one tile and keeps the table small)
        n_nb = -(-(n_out // 16) // 8)
        ks = max(1, min(8, 256 // (n_mb * n_nb)))
        return 100 * tm + 42 + (20000 if tm <= 2 else 0), ks

    def _weights_fingerprint(self):
        ps = self._fp_params
        return tuple(map(_DATA_PTR, ps)), tuple(map(_VERSION, ps))  # (C-level maps: ~45 us for the 224 projection weights of a 7B model)

    def parameter_bytes(self) -> int:
        """Bytes of the parameters and buffers the state dict holds (what the reference's `model memory` print measures, BIMG:59-67)."""
        seen, n = set(), 0
        for t in list(self.parameters()) + list(self.buffers()):
            if t.data_ptr() not in seen:
                seen.add(t.data_ptr())
                n += t.numel() * t.element_size()
        return n

    def operand_copy_bytes(self) -> dict:
        """Bytes this engine keeps BESIDE the parameters: second copies of weights in matrix-core operand order (decoder q|k|v, gate|up, down_proj for
        dl_linear_packed; the CLIP tower's and the projector's projections for dl_linear_tiles) and the tower's fused q|k|v.  The reference holds none of
        these: the harness counterparts report them separately so that `model memory` stays comparable."""
        nb = lambda t: 0 if t is None else t.numel() * t.element_size()
        dec = sum(nb(l.wp_qkv) + nb(l.wp_gu) + nb(l.wp_down) + nb(l.wp_o) for l in self.model.layers)
        vt = self.get_vision_tower()
        clip_tiles = int(getattr(vt, "tiles_bytes", 0) or 0) if vt is not None else 0
        clip_fused = sum(nb(w) + nb(b) for w, b in getattr(vt, "_qkv", [])) if vt is not None else 0
        proj = sum(nb(t) for t in (getattr(self, "_proj_tiles", None) or ()))
        return {"decoder_operand_order": dec, "clip_operand_order": clip_tiles, "clip_fused_qkv": clip_fused, "projector_operand_order": proj,
                "total": dec + clip_tiles + clip_fused + proj}

    # DL_USE_HIP_GRAPH=0: debugging switch that wins over any assignment -- e.g. the GPU tests under PYTORCH_NO_CUDA_MEMORY_CACHING=1 (every tensor its own
    # allocation, so that an out-of-bounds read faults instead of landing in a neighbour; stream capture is impossible without the caching allocator)
    _force_eager = os.environ.get("DL_USE_HIP_GRAPH", "1") == "0"

    @property
    def use_hip_graph(self):
        return self._use_hip_graph and not self._force_eager

    @use_hip_graph.setter
    def use_hip_graph(self, v):
        self._use_hip_graph = bool(v)

    # ---- one decode step; every buffer persistent, no host sync -> hipGraph-capturable ----
    def knobs(self) -> dict:
        """The resolved values of every tuning knob and test hook that decides WHICH kernels a request runs on (constructor defaults, DL_* environment
        values, attributes set later) -- recorded in the bench line so that a run can be reproduced.  The last three are test hooks:
        they must be None / 0 outside tests/."""
        return {
            "use_hip_graph": self.use_hip_graph, "attn_inkernel_combine": self.attn_inkernel_combine, "device_prompt_layout": self.device_prompt_layout,
            "tp_side_stream": self.tp_side_stream, "gemv_max_decode_batch": self.gemv_max_decode_batch, "smallm_max_decode_batch": self.smallm_max_decode_batch,
            "fuse_qkv_attn": self.fuse_qkv_attn, "fuse_gu_tp": self.fuse_gu_tp, "decode_weight_pack": self.decode_weight_pack, "decode_weight_pack_plain": self.decode_weight_pack_plain, "decode_weight_pack_qkv": self.decode_weight_pack_qkv, "decode_weight_pack_down": self.decode_weight_pack_down, "fused_attn_max_splits": self.fused_attn_max_splits, "gu_grid_cap": self.gu_grid_cap,
            "qkv_attn_grid_cap": self.qkv_attn_grid_cap, "splitk_o_proj": self.splitk_o_proj, "packed_prefill_gemm": self.packed_prefill_gemm, "packed_down_proj": self.packed_down_proj, "packed_qkv_parts": self.packed_qkv_parts, "packed_decode_mlp": self.packed_decode_mlp, "packed_decode_mlp_min_batch": self.packed_decode_mlp_min_batch, "packed_decode_qkv_min_batch": self.packed_decode_qkv_min_batch, "packed_decode_qkv_parts": self.packed_decode_qkv_parts, "packed_decode_qkv_parts_max_batch": self.packed_decode_qkv_parts_max_batch,
            "smallm_wide_slices": self.smallm_wide_slices, "decode_sync_every": self.decode_sync_every, "prefill_width_bucket": self.prefill_width_bucket,
            "max_prefill_graphs": self.max_prefill_graphs,
            "tiles_o_proj": self.tiles_o_proj, "tiles_o_proj_min_decode_batch": self.tiles_o_proj_min_decode_batch,
            "clip_tiles_gemm": getattr(self.get_vision_tower(), "tiles_gemm", None), "clip_tiles_max_batch": getattr(self.get_vision_tower(), "tiles_max_batch", None),
            "clip_tiles_ksplit": [getattr(self.get_vision_tower(), "tiles_ksplit_out", None), getattr(self.get_vision_tower(), "tiles_ksplit_fc2", None)],
            "decode_weight_format": self.decode_weight_format, "mx8_max_decode_batch": self.mx8_max_decode_batch, "kv_cache_format": self.kv_cache_format,
            "device_sampling": True,  # generate(do_sample=True, seed=...) draws inside the captured graphs (dl_decode_sample)
            "device_logits_processors": True,  # repetition_penalty / no_repeat_ngram_size / bad_words_ids act inside the captured graphs (dl_logits_process)
            "device_logprobs": True,  # generate(output_logprobs=True, top_logprobs=n) reads the log-probabilities off inside the captured graphs (dl_decode_logprobs)
            "device_stop_sequences": True,  # generate(stop_sequences= / stopping_criteria=[keyword criterion]) finishes rows inside the captured graphs (dl_decode_stop)
            "device_fork": True,  # generate(do_sample=True, seed=..., num_return_sequences=n) prefills a prompt once and forks its K/V into n decode rows (dl_kv_fork)
            "test_hook_force_text_decision": self.force_text_decision is not None, "test_hook_single_split_keys_override": self.single_split_keys_override,
            "test_hook_min_keys_per_split": getattr(self, "min_keys_per_split", None),
        }

    # ---- public API -----------------------------------------------------------------------------
    @torch.no_grad()
    def forward(
        self, input_ids=None, attention_mask=None, position_ids=None, past_key_values=None, inputs_embeds=None, labels=None, use_cache=None,
        output_attentions=None, output_hidden_states=None, images=None, image_sizes=None, return_dict=None, input_embeds_indices=None,
        image_features=None,
    ):
        """dynamic_llava_llama.py:68-115 + dynamic_modeling_llama.py:2631-2813 (inference; no labels / loss).
        logits: fp32 [B, N', V] for ALL positions like the reference (DML:2709-2710); rows are right-padded with
        zeros when their lengths differ.

        Host synchronisation of DECODE steps (a one-token call on a non-empty cache): the step's launches are scheduled by the same rule generate()
        follows, which reads the evicted layers' longest row back from the device ONCE PER CHUNK of steps -- steps 1, 5, 9, then every
        `decode_sync_every` (8) steps block on a device->host copy and check the error word of the fused launches (check_device_errors()).  All other
        steps enqueue and return.  A caller that captures forward() steps in its own hipGraph / stream pipeline sets `model.decode_sync_every = 0`:
        then no decode step ever reads the device (launches are sized for the longest possible rows; logits in the same rounding class, not
        bit-identical to generate()'s), and calling check_device_errors() at a convenient sync point is the caller's job."""
        self._check_ready(weights=past_key_values is None)  # (the ~0.1 ms weight-fingerprint check runs where a sequence starts, not on every decode step of a forward() loop)
        if labels is not None:
            raise NotImplementedError("labels / loss are training-side (DML:2713-2800), out of scope; score() gives the teacher-forced NLL of a labelled continuation")
        if output_attentions or output_hidden_states:
            raise NotImplementedError("output_attentions / output_hidden_states are not produced by the fused path")
        if use_cache is False:
            return self._forward_nocache(input_ids, attention_mask, past_key_values, inputs_embeds, images, image_features, input_embeds_indices)
        if (input_ids is None) == (inputs_embeds is None):
            raise ValueError("You have to specify either input_ids or inputs_embeds")  # DML:1686-1695
        cache = past_key_values
        if cache is not None and not isinstance(cache, KVSlabCache):
            cache = KVSlabCache.from_legacy_cache(cache, self.config.sparse_config["sparse_layer"], device=self.device, kv_format=self.kv_cache_format)
        decode = cache is not None and max(cache.full_len_host) > 0
        if decode:
            if input_ids is None:
                raise NotImplementedError("inputs_embeds on a non-empty cache")
            if input_ids.shape[1] != 1:
                return self._forward_chunk(input_ids, attention_mask, cache)
            B = input_ids.shape[0]
            st = self._get_dstate(B, 0)
            self._bind_schedule(st, cache)
            cache.ensure_capacity(2)
            self._rope_tables(max(cache.full_len_host) + 2)
            st.cur_ids.copy_(input_ids[:, 0])
            self._mode = StepMode()
            # the decode schedule (KVSlabCache.sched_*): the same rule generate() follows, evaluated step by step -- a forward()-driven loop
            # replays the same kernels as generate() on the same request.  Costs one device->host copy of the lengths per CHUNK of steps
            if self.decode_sync_every <= 0:
                # sync-free decode steps: nothing is read back from the device -- the launches are scheduled from the host-known dense
                # length (every row of the evicting layers is at most that long).  For callers that capture forward() steps in their own graph or
                # pipeline; the kernels chosen are the ones for the LONGEST possible rows, so a request decoded this way and through generate()
                # may differ in the last bits of its logits (same rounding class).  check_device_errors() is then the caller's job.
                if cache.sched_active():
                    cache.sched_drop()
                cache.set_bounds(max(cache.full_len_host) + 1, max(cache.full_len_host) + 1)
            else:
                if not cache.sched_active():  # a cache of unknown history (imported legacy tuple, a chunk appended): start from what is there now
                    cache.sched_begin(max(cache.full_len_host), int(cache.lens[1].max()), self.decode_sync_every)
                if cache.sched_at_boundary():
                    if cache._sch["chunks"] > 0:
                        cache.sched_observe(cache._sch["produced"], int(cache.lens[1].max()))
                        self.check_device_errors()  # the queue has just been drained anyway: a fused launch that gave up must not go unnoticed in a forward() loop either
                    cache.sched_chunk()
            st.clear_granules()  # callers may interleave caches at equal positions on this state: every call
            self._decode_step_kernels(st, cache, False)
            use_tp = self._use_tp()
            cache.lens[0] += 1
            dec_ = st.decision if use_tp else 1
            if use_tp and self.force_text_decision is not None:
                # test hook (the oracle has the same one): continue a comparison past a keep/evict logit pair that sits on the decision boundary.
                # Only the bookkeeping is overridden -- the step's own logits never depend on its decision (the token always attends itself,
                # DML:1061-1076); debug_records keeps the predictor's own decision and logits
                dec_ = torch.as_tensor(self.force_text_decision).to(device=self.device, dtype=torch.int32).reshape(st.decision.shape)
            cache.lens[1] += dec_
            cache.full_len_host = [n + 1 for n in cache.full_len_host]
            cache.seen_tokens += 1
            if cache.sched_active():
                cache.sched_advance(1)
            if self.debug_records is not None:
                self.debug_records.update(text_decision=st.decision.clone() if use_tp else None, text_logit=st.tp_logits.clone())
            logits = st.logits.to(torch.float32, copy=True).unsqueeze(1)  # never alias the persistent step buffer
            return CausalLMOutputWithPast(logits=logits, past_key_values=cache)
        # ---- prefill ----
        if inputs_embeds is not None:
            embeds, lens, indices = self._unpad_embeds(inputs_embeds, attention_mask, input_embeds_indices)
        else:
            embeds, lens, indices = self._prepare_packed(input_ids, attention_mask, None, images, image_features)
        x, cache, lens2, cu_list = self._prefill(embeds, lens, indices, cache, reserve=256, last_only=False)
        logits_packed = F.linear(x, self.lm_head.weight).float()[: cu_list[-1]]  # (x may be sized for a width bucket: rows past the last sequence are padding)
        B = len(lens2)
        if len(set(lens2)) == 1:
            logits = logits_packed.view(B, lens2[0], -1)
        else:
            logits = logits_packed.new_zeros((B, max(lens2), logits_packed.shape[-1]))
            for b in range(B):
                logits[b, : lens2[b]] = logits_packed[cu_list[b] : cu_list[b + 1]]
        return CausalLMOutputWithPast(logits=logits, past_key_values=cache)

    @torch.no_grad()
    def _generate_sample(self, inputs, images, greedy=False, **kwargs):
        """`greedy=True` (round 4): the same plain loop over forward() taking the argmax -- the route for requests the device-side greedy loop does not
        take (more than three EOS ids: dl_decode_advance compares three).  do_sample=True: temperature / top_k / top_p sampling as HF's logits warpers define them (TemperatureLogitsWarper,
        TopKLogitsWarper, TopPLogitsWarper: the smallest set of most probable tokens whose mass reaches top_p is kept), drawn with
        torch's generator -- a plain loop over forward() (no hipGraph: this is the convenience path, the harness default is greedy).
        Token streams cannot match HF's draw for draw (different RNG consumption); the distribution per step is the same.
        repetition_penalty / no_repeat_ngram_size / bad_words_ids: logits_rules.process on every step's logits before anything else, on the tokens emitted in this call.
        output_logprobs / top_logprobs: logprobs.reference_rows on every step's raw fp32 logits (the rule dl_decode_logprobs implements), masked behind a row's EOS."""
        req = request.parse(kwargs, self.config, batch=inputs.shape[0])
        attention_mask, image_features = req.attention_mask, req.image_features
        if req.n_return > 1:  # n answers per prompt on a host route: every prompt n times in the batch (rows b * n .. b * n + n - 1, HF's order), no fork
            rep = lambda t: t.repeat_interleave(req.n_return, dim=0) if torch.is_tensor(t) else t
            inputs, images, attention_mask, image_features = rep(inputs), rep(images), rep(attention_mask), rep(image_features)
        out = self.forward(inputs.to(self.device), attention_mask=attention_mask, images=images, image_features=image_features)
        cache = out.past_key_values
        max_new = req.max_new(cache.full_len_host)
        # last VALID position of every row: the logits are right-padded with zeros when rows differ in length; the last layer's KV length is the (compacted) row length
        last = cache[1][-1].to(self.device).long() - 1
        last_logits = lambda o, at: o.logits[torch.arange(o.logits.shape[0], device=self.device), at].float()
        neg = None
        if req.guidance is not None:  # the negative prompts: a second stream on a cache of its own, advanced with the same picked tokens (request.host_loop)
            n_ids, n_mask, n_images, n_feats = guidance.negative_inputs(kwargs, inputs, images, IMAGE_TOKEN_INDEX)
            n_out = self.forward(n_ids.to(self.device), attention_mask=n_mask, images=n_images, image_features=n_feats)
            neg = (last_logits(n_out, n_out.past_key_values[1][-1].to(self.device).long() - 1), n_out.past_key_values)
        return self._host_decode(req, cache, last_logits(out, last), max_new, greedy, neg)

    def _host_decode(self, req, cache, logits, max_new, greedy, neg=None):
        """A host route behind its first forward(): request.host_loop over single decode steps on `cache` -> the tokens [B, T_new], or generate()'s dict.
        neg = (the negative stream's first logits, its cache): a guided request."""
        self.last_prefill_logits = logits.clone()
        finish = []  # the rows' finish columns, asked for only where a row can finish on more than EOS
        more = dict(finish=finish) if (req.stops or req.criteria) else {}
        if neg is not None:
            more["negative"] = (neg[0], lambda nxt: self.forward(nxt[:, None], past_key_values=neg[1]).logits[:, -1].float())
        toks, scores, raw = request.host_loop(logits, lambda nxt: self.forward(nxt[:, None], past_key_values=cache).logits[:, -1].float(), req, max_new, greedy, **more)
        seq, self.last_cache = torch.stack(toks, dim=1), cache
        if not req.want_dict:
            return seq
        res = {"sequences": seq, "past_key_values": cache}
        if req.want_scores:
            res["scores"] = tuple(scores)
        if req.n_lp >= 0:
            res.update(logprobs.host_result(raw, seq, req.eos, req.n_lp, finish[0] if (req.stops or req.criteria) else None))
        if req.constraint is not None:
            res["constraint_complete"] = constraints.complete(req.constraint, seq.cpu()).to(seq.device)
        return res

    @torch.no_grad()
    def _generate_on_cache(self, inputs, images, **kwargs):
        """generate(new_ids, past_key_values=cache): greedy continuation of a dialogue whose earlier turns (image included) are in `cache` (what
        a previous call returned: `return_dict_in_generate=True`, or forward()).  `inputs` holds ONLY the new turn's token ids [B, T] -- with
        the image placeholder of the first turn the reference's `input_ids[:, past_length:]` slicing (DML:2831-2853) has no consistent meaning,
        and its own multi-round harness drives forward() (model_lvis_multi_round_for_ppl.py:108-220).  The new chunk goes through the
        chunk-on-cache path (DML:2506-2521: the instruct predictor decides which of its K/V rows stay in layers >= sparse_layer), the new
        tokens through single decode steps; plain loop over forward(), no hipGraph.  repetition_penalty / no_repeat_ngram_size / bad_words_ids: logits_rules.process
        on every step's logits, on the tokens emitted in this call."""
        req = request.parse(kwargs, self.config, batch=inputs.shape[0])
        if images is not None or req.image_features is not None:
            raise NotImplementedError("generate(past_key_values=...) continues a dialogue: the image belongs to the first call")
        cache = kwargs["past_key_values"]
        if self.kv_cache_format is not None or getattr(cache, "kv_format", None) is not None:
            raise NotImplementedError(f"generate(past_key_values=...) starts with a multi-token chunk on the cache, which is not built for the KV cache format "
                                      f"{self.kv_cache_format or cache.kv_format!r} (the chunk-on-cache attention reads model-dtype rows)")
        if not isinstance(cache, KVSlabCache):
            cache = KVSlabCache.from_legacy_cache(cache, self.config.sparse_config["sparse_layer"], device=self.device)
        inputs = inputs.to(self.device)
        if inputs.shape[0] != cache.batch:
            raise ValueError(f"{inputs.shape[0]} rows of new tokens for a cache of {cache.batch} rows")
        if bool((inputs == IMAGE_TOKEN_INDEX).any()):
            # HF's convention (prepare_inputs_for_generation, DML:2835-2848) passes the FULL dialogue and slices input_ids[:, past_length:]; with
            # the image placeholder in the ids and 576 features in the cache that slice is meaningless, so it is refused instead of appending
            # the whole prompt to the cache a second time
            raise ValueError("generate(past_key_values=...) takes ONLY the new turn's token ids; these ids contain the image placeholder, i.e. the full dialogue "
                             "(the first turn, image included, is already in the cache)")
        # max_length counts what is already cached plus the new turn (the reference's own length accounting includes the 576 image tokens)
        max_new = req.max_new([cache.seen_tokens + inputs.shape[1]])
        out = self.forward(inputs, attention_mask=req.attention_mask, past_key_values=cache)
        req = dataclasses.replace(req, temperature=1.0, top_k=0, top_p=None)  # this route has never warped: the loop then is the plain argmax loop, bit for bit
        return self._host_decode(req, out.past_key_values, out.logits[:, -1].float(), max_new, True)

    @torch.no_grad()
    def score(self, input_ids, labels, images=None, image_sizes=None, *, attention_mask=None, image_features=None, sync_every=None, output_logits=False, **kwargs):
        """Teacher-forced negative log-likelihood of a labelled continuation, on the device inside generate()'s captured graphs: the reference's
        generation-time perplexity driver (llava/dynamic_eval/model_lvis_for_ppl.py:136-191 -- forward, take the last position's logits, record the
        label, feed the label) with dl_decode_score where greedy decoding has dl_decode_advance (the rule is scoring.py).
        input_ids [B, W]: the prompt exactly as generate() takes it.  labels: int64 [B, T], T >= 1; -100 marks "no label" and is allowed only as the
        tail of a row (column 0 holds a label in every row); anything else outside [0, V), or a row count other than input_ids', raises ValueError
        before any launch.  Step j scores labels[:, j] on the logits after prompt + labels[:, :j], then feeds labels[:, j]: one prefill + T - 1
        decode steps (the last label of the longest row is scored and never run through the decoder, as in the reference loop).
        -> dict: nll fp32 [B, T] (0 where there is no label), n_labels int64 [B], ppl fp32 [B] = exp(sum nll / n_labels), top1 int64 [B, T] (the greedy
        token of every scored step, -1 where there is no label), past_key_values (the caller's own: an independent copy of the cache, so the pooled slab and
        the graphs captured on it serve the next call of the same shape);
        output_logits=True adds logits: a tuple of fp32 [B, V], one per step (the step-by-step route of generate(output_logits=True), for tests)."""
        if any(k in constraints.KEYWORDS for k in kwargs):  # (constrained decoding restricts what a row may say; a label sequence is scored as it stands)
            raise ValueError(f"score() takes no constraint ({', '.join(k for k in kwargs if k in constraints.KEYWORDS)}): a label is scored on the model's own logits")
        if any(k in guidance.KEYWORDS for k in kwargs):  # (guidance changes which token is picked; a label sequence is scored as it stands)
            raise ValueError(f"score() takes no guidance ({', '.join(k for k in kwargs if k in guidance.KEYWORDS)}): a label is scored on the model's own logits")
        if kwargs:
            raise TypeError(f"score() got an unexpected keyword argument {next(iter(kwargs))!r}")
        if not torch.is_tensor(input_ids) or input_ids.dim() != 2:
            raise ValueError("input_ids must be a tensor [B, W]")
        if self.config.vocab_size > sampling.MAX_VOCAB:
            raise ValueError(f"score() takes vocabularies of up to {sampling.MAX_VOCAB} entries (dl_decode_score's 64-bit fixed-point masses)")
        n_labels = scoring.validate_labels(labels, input_ids.shape[0], self.config.vocab_size)
        kw = dict(max_new_tokens=int(labels.shape[1]), min_new_tokens=0, eos_token_id=None, return_dict_in_generate=True, output_logits=bool(output_logits),
                  attention_mask=attention_mask, image_features=image_features, _score_labels=labels.detach().to("cpu").contiguous())
        if sync_every is not None:
            kw["sync_every"] = sync_every
        res = self.generate(input_ids, images=images, image_sizes=image_sizes, **kw)
        nll = res["nll"]
        n_dev = n_labels.to(nll.device)
        out = {"nll": nll, "n_labels": n_dev, "ppl": torch.exp(nll.sum(dim=1) / n_dev.to(torch.float32)), "top1": res["top1"], "past_key_values": res["past_key_values"]}
        if output_logits:
            out["logits"] = res["logits"]
        return out

    @torch.no_grad()
    def generate(self, inputs=None, images=None, image_sizes=None, **kwargs):
        """dynamic_llava_llama.py:117-152: greedy decoding; returns the NEW tokens only [B, T_new] (HF behaviour when
        generation is driven by inputs_embeds).  Supported kwargs: max_new_tokens / max_length, min_new_tokens (EOS banned from
        the argmax until then, as HF's MinNewTokensLengthLogitsProcessor), do_sample (True: temperature / top_k / top_p sampling --
        with seed=<int> on the device, inside the same captured graphs as greedy decoding (dl_decode_sample; the rule is sampling.py;
        sample_row_base=<int> offsets the rows' random streams for sharded batches); without seed, or with generator=, through
        _generate_sample on torch's RNG), num_beams(1), use_cache(True), eos_token_id, pad_token_id, attention_mask,
        return_dict_in_generate (+ output_scores), image_features (pre-computed projector output, testing),
        num_return_sequences=n (n sampled answers per prompt; needs do_sample=True): `sequences` is [B * n, T] with prompt b's answers in rows b * n .. b * n + n - 1 (HF's
        order), and every per-row result (scores, logits, logprobs, top_logprobs, top_logprob_ids, the returned cache) has B * n rows.  With seed=<int> the B prompts are
        prefilled ONCE, at batch B exactly as a plain call of them would be, and inside the captured prefill graph dl_kv_fork copies every prompt's live K/V into its n decode
        rows; row b * n + r draws with the random stream of row sample_row_base + b * n + r (a sharded batch passes sample_row_base = its first global prompt * n), so the
        n first tokens already differ.  On the host routes (generator=, no seed, past the device caps) the prompts are repeated n times in the batch instead.  n > 1 without
        do_sample or in score() raises ValueError, with past_key_values NotImplementedError, before any launch,
        repetition_penalty / no_repeat_ngram_size / bad_words_ids (HF's RepetitionPenalty / NoRepeatNGram / NoBadWords logits processors, bit for bit, on the
        tokens generated in this call -- the prompt is never part of the history, as for HF driven by inputs_embeds; on the device inside the same captured
        graphs (dl_logits_process; the rule is logits_rules.py), in front of the EOS ban of min_new_tokens and of temperature / top_k / top_p; a request past
        logits_rules.MAX_NGRAM / MAX_BAD_WORDS / MAX_BAD_WORD_LEN runs the plain loop over forward() with the same rule; `scores` are the processed logits,
        `logits` the raw ones).  Bad values of these raise ValueError before any launch.
        output_logprobs=True (with return_dict_in_generate=True) adds `logprobs`: fp32 [B, T], the log-probability of sequences[b, t]; top_logprobs=n (an int in
        0..logprobs.MAX_TOP_LOGPROBS, default 0) adds `top_logprobs` fp32 [B, T, n] and `top_logprob_ids` int64 [B, T, n], the step's n most probable tokens (logit
        descending, index ascending).  The distribution is always that of the model's OWN step logits -- the raw ones output_logits=True reports, the quantity score()
        uses -- before the logits processors, before the EOS ban of min_new_tokens and before temperature / top_k / top_p, also for a sampled token.  Read off on the
        device inside the same captured graphs (dl_decode_logprobs behind the step-closing launch; the rule is logprobs.py): no [B, V] tensor reaches the host and
        the decode loop keeps its chunks.  Columns after a row's first EOS (pad in `sequences`) hold 0.0 / -1, the EOS token's own entry is real; the host routes
        (_generate_sample, _generate_on_cache) return the same keys from the same rule.  Bad values raise ValueError before any launch.
        stop_sequences=[ids, ...] (non-empty lists of token ids or 1-D integer tensors) and stopping_criteria=[...] (a list or HF StoppingCriteriaList): a row finishes
        when the tokens generated in this call end in a stop sequence -- the token-tail rule of the reference's KeywordsStoppingCriteria (llava/mm_utils.py:257-267),
        per row; an item of stopping_criteria with a `keyword_ids` attribute contributes its sequences (its decoded-text substring check needs a tokenizer and is not
        built).  The matched tokens stay in `sequences`, pad follows, and the result is trimmed where the last row finishes, exactly as for EOS; min_new_tokens does
        not hold a match back; `logprobs` / `top_logprobs` report 0.0 / -1 behind it.  Up to stopping.MAX_STOPS sequences of up to stopping.MAX_STOP_LEN tokens are
        matched on the device inside the same captured graphs (dl_decode_stop behind the step-closing launch; the rule is stopping.py; the list is device data, one
        graph serves every list); a longer list, and any other item of stopping_criteria -- a callable (ids [B, t], scores [B, V]) -> bool | BoolTensor [B], called
        once per step on the tokens generated in this call -- runs the plain loop over forward() with the same rule.  Bad values raise ValueError before any launch.
        streamer= (any object with put(tensor) and end(), e.g. HF's TextStreamer / TextIteratorStreamer), on every route: put(an empty int64 CPU tensor [B, 0])
        first, then put(sequences[:, j].cpu()) for every column of the returned `sequences`, in order and once each, then end().  On the device route the first
        token is put after the prefill and a chunk's tokens when the loop consumes that chunk's observation (the same pinned, non-blocking copies; the schedule,
        the tokens and the captured graphs are those of the call without a streamer); sync_every=1 is the knob for token-by-token latency.
        constraint= (a constraints.TokenAutomaton, or a list of B, one per prompt), guided_choice= (a list of token-id sequences: every row says exactly one of them,
        then EOS), allowed_token_ids= (a whitelist) and prefix_allowed_tokens_fn= (HF's fn(batch_id, ids_1d) -> allowed ids, called with the tokens generated in this
        call) -- at most one of the four: constrained decoding.  Every row walks a deterministic token automaton; at every step the tokens with no edge out of the
        row's state are -inf, behind the logits processors above and in front of temperature, top-k, top-p and the pick (HF's order for
        PrefixConstrainedLogitsProcessor); every accepting state takes the request's EOS ids.  The first three run on the device inside the same captured graphs
        (dl_logits_constrain between dl_logits_process and the step-closing launch; the rule is constraints.py; the automaton is device data, one graph serves every
        automaton) up to constraints.MAX_STATES / MAX_EDGES, past them -- and the callable always -- on the plain loop over forward() with the same rule.  `scores`
        are the constrained logits, `logits` and the log-probabilities stay the model's own; with return_dict_in_generate the result has `constraint_complete`, bool
        [rows]: the row ended through an EOS edge instead of being cut off by max_new_tokens.  A dead end, an EOS id that is an edge of an accepting state,
        min_new_tokens > 0, two of the keywords, or any of them in score() raise ValueError before any launch; a row that processors and constraint together leave all
        -inf is the caller's error, as in HF.
        guidance_scale=s (a finite float >= 0; None and 1.0 are the request without the keyword) with negative_prompt_ids= (int64 [B, Wn] or [1, Wn], laid out as
        `inputs` are: a row with the <image> placeholder takes an image, a row without it is text-only) and / or negative_images= (the images of the negative rows
        that hold a placeholder, default the request's; without negative_prompt_ids the negative ids are `inputs`: same text, another image), negative_prompt_attention_mask=
        (belongs to negative_prompt_ids), guidance_cutoff=beta in (0, 1): classifier-free guidance / visual contrastive decoding.  Every step's scores are
        s * (logprob_cond - logprob_neg) + logprob_neg, with beta only where logprob_cond >= max logprob_cond + log(beta) (-inf elsewhere) -- HF's
        UnbatchedClassifierFreeGuidanceLogitsProcessor, in HF's place: in front of the logits processors, the constraint, the EOS ban, temperature, top-k and top-p (the
        rule is guidance.py).  On the device the negative prompt is a second ROW of the same captured decode step: state and cache have 2 B rows (row B + b is prompt
        b's negative), prompts and negatives are prefilled as two batches of B and placed by dl_kv_place, dl_logits_guide writes the guided scores of a pair to both
        its rows in front of the other logits launches, dl_pair_follow keeps the negative row on its prompt's tokens; scale and cutoff are device data, one graph
        serves every setting.  Every per-row result is the B prompts'; with output_logits=True the dict also has `negative_logits` (the negative rows' raw logits per
        step), and the returned cache is an independent B-row copy of the prompts' rows.  `logits` and the log-probabilities stay the conditional rows' own.  The host
        routes run two streams on two caches with the same rule.  A bad scale or cutoff, an active scale without negative_prompt_ids / negative_images, a cutoff without
        an active scale, or any of these keywords in score() raise ValueError; with num_return_sequences > 1 or past_key_values NotImplementedError; before any launch.
        Still ignored without a word: logits_processor, suppress_tokens, sequence_bias.
        Steady state (same prompt SHAPE as a previous call): the whole prefill -- CLIP, projector, embedding assembly,
        32 layers, first-token argmax -- is one hipGraph replay and every decode step is another; the host only copies
        the new token ids / pixels into static buffers."""
        self._check_ready()
        req = request.parse(kwargs, self.config, self.decode_sync_every, batch=inputs.shape[0] if torch.is_tensor(inputs) and inputs.dim() == 2 else None)  # every keyword is validated here, before any launch
        if req.route == "on_cache":
            return self._generate_on_cache(inputs, images, **kwargs)
        if req.route == "host_sample":
            return self._generate_sample(inputs, images, **kwargs)
        if req.route == "host_greedy":
            return self._generate_sample(inputs, images, greedy=True, **{k: v for k, v in kwargs.items() if k not in ("do_sample", "sync_every")})
        # ---- the device route: layout, cache / RoPE / state, arm, prefill (+ first token), decode loop, finish ----
        inputs = inputs.to(self.device)
        tm = {"ev": [torch.cuda.Event(enable_timing=True) for _ in range(3)], "path": None} if self.record_timing else None
        if tm is not None:
            tm["ev"][0].record()
        lay, dev_layout = self._generate_layout(inputs, req, self._n_feat(images, req.image_features))
        lens, B, max_new = lay["lens"], lay["B"], req.max_new(lay["lens"])
        # num_return_sequences = n > 1: the B prompts are prefilled once, into a source cache of B rows; inside the prefill closure dl_kv_fork copies every prompt's live
        # K/V into n rows of the B * n-row cache and the first-step logits are repeated, so the n rows of a prompt draw n first tokens (row b * n + r: Philox counter row
        # row_base + b * n + r).  Everything behind the prefill serves a B * n-row state as it serves any batch
        n = req.n_return
        # guidance_scale (active): the pair layout -- decode state and cache have 2 B rows, rows [0, B) the prompts, row B + b prompt b's negative; prompts and negatives are
        # prefilled as two batches of B, each exactly as a plain call of them would be, into the pooled source cache and from there (dl_kv_place) into their rows; every
        # per-row result of the call is rows [:B]
        neg = None if req.guidance is None else self._guided_negatives(kwargs, inputs, images, req)
        rows, longest = B * n * (1 if neg is None else 2), max(lens if neg is None else lens + neg["lay"]["lens"])
        cache = self._pooled_cache(rows, longest + max_new + 1)
        fork = None if n == 1 else (self._fork_source(B, max(lens) + 1), n)
        self._rope_tables(longest + max_new + 1)
        st = self._get_dstate(rows, max_new)
        self._bind_schedule(st, cache)
        self._arm(st, req, max_new)
        ents = []
        if neg is None:
            ent, prefill_path = self._generate_prefill(lay, dev_layout, inputs, images, req.image_features, cache, st, max_new, fork)
            ents.append((ent, dev_layout))
        else:
            maps = self._pair_maps(B)
            ent, prefill_path = self._generate_prefill(lay, dev_layout, inputs, images, req.image_features, cache, st, max_new, place=(self._fork_source(B, longest + 1), maps[0], 0, False))
            nent, _ = self._generate_prefill(neg["lay"], neg["dev"], neg["ids"], neg["images"], neg["feats"], cache, st, max_new, place=(self._fork_source(B, longest + 1), maps[1], B, True))
            ents += [(ent, dev_layout), (nent, neg["dev"])]

        def layout_failed():  # a device layout met a row without exactly one image token: what was computed is meaningless (the flag is read with the call's own synchronisation)
            bad = [e for e, d in ents if d and int(e["didx"]["err"].item()) != 0]
            for e in bad:
                e["didx"]["err"].zero_()
            return bool(bad)

        self.last_prefill_logits = self._prefill_logits_buf if neg is None else self._prefill_logits_buf[:B]  # (a guided request: the prompts' rows, like every per-row result)
        if tm is not None:
            tm["ev"][1].record()
            tm["path"] = prefill_path
        scores, raw_logits, neg_logits = [], [], []
        on_step = (lambda j: self._score(req, st, j, scores, raw_logits, neg_logits)) if (req.want_scores or req.want_logits) else None
        if on_step is not None:
            on_step(0)
        feed = None
        if req.streamer is not None:
            if layout_failed():  # (the check below, made before a token of a meaningless run reaches the streamer)
                return self.generate(inputs, images=images, image_sizes=image_sizes, _host_layout=True, **kwargs)
            feed = stopping.Feed(req.streamer, B * n, req.eos, req.stops)
            feed.push(st.out_ids[: B * n, :1].cpu())  # the first token: the caller waits for it
        produced = self._decode_loop(st, cache, max_new, req.sync_every, on_step, feed)
        if rows == 1 or self._lp_ws is not None:
            self.check_device_errors()  # (B > 1 too: dl_linear_packed's k ranges hand over in-kernel, through _lp_err; generate() is about to synchronise for its result anyway)
        if layout_failed():
            # a row without exactly one image token (text-only row, several images): what was computed is meaningless -- repeat the
            # call with the host-side layout, which handles (or rejects) those rows like the reference does
            return self.generate(inputs, images=images, image_sizes=image_sizes, _host_layout=True, **kwargs)
        res = self._finish(req, st, cache, produced, scores, raw_logits, tm, neg_logits)
        if feed is not None:
            feed.finish(res["sequences"] if isinstance(res, dict) else res)
        return res

    def _guided_negatives(self, kwargs, inputs, images, req):
        """The negative rows of a guided request, laid out as the prompts are -> dict(ids, images, feats, lay, dev)."""
        ids, mask, n_images, n_feats = guidance.negative_inputs(kwargs, inputs, images, IMAGE_TOKEN_INDEX)
        ids = ids.to(self.device)
        lay, dev = self._generate_layout(ids, dataclasses.replace(req, attention_mask=mask, image_features=n_feats), self._n_feat(n_images, n_feats))
        return dict(ids=ids, images=n_images, feats=n_feats, lay=lay, dev=dev)

    def _pair_maps(self, B):
        """dl_kv_place's row maps of a guided request of B pairs, on the device (made once: captured prefills hold their pointers): source rows 0 .. B - 1 -> the
        prompts' rows 0 .. B - 1 (also the way back, into the caller's B-row cache) and -> the negatives' rows B .. 2 B - 1."""
        maps = getattr(self, "_pair_maps_dev", None)
        if maps is None:
            maps = self._pair_maps_dev = {}
        if B not in maps:
            r = list(range(B))
            maps[B] = (ops.kv_place_maps(r, r, B, 2 * B, self.device), ops.kv_place_maps(r, [B + b for b in r], B, 2 * B, self.device))
        return maps[B]

    def _score(self, req, st, step_idx, scores, raw_logits, neg_logits=None):
        """The device route's per-step callback: appends HF's `scores` of the step (the processed logits, EOS at -inf while step < min_new_tokens) and the raw logits.
        A guided request (rows [:P] the prompts, [P:] their negatives): all of rows [:P]; the negative rows' raw logits go to neg_logits."""
        z = (self._prefill_logits_buf if step_idx == 0 else st.logits).float().clone()
        P = z.shape[0] // 2 if req.guidance is not None else z.shape[0]
        if req.want_logits:
            raw_logits.append(z[:P].clone())
            if req.guidance is not None:
                neg_logits.append(z[P:].clone())
        if req.guidance is not None:  # what dl_logits_guide left: both rows of a pair hold the pair's guided scores
            z = st.guide_logits[:P].clone()
        if req.rules.on or req.constraint is not None:  # what dl_logits_process / dl_logits_constrain left for this step's bookkeeping launch
            z = st.proc_logits[:P].clone()
        banned = list(req.eos) if step_idx < req.min_new else []
        if req.sampled is not None:  # z = logit / T with -inf outside the kept set, as HF reports a sampled step: on the host, with the contract's own arithmetic (sampling.py)
            z = sampling.processed_logits(z.cpu(), *req.sampled[:3], banned).to(z.device)
        elif banned:
            z[:, banned] = float("-inf")
        scores.append(z)

    def _finish(self, req, st, cache, produced, scores, raw_logits, tm, neg_logits=()):
        """The device route's result: the host mirrors of what the loop advanced, the EOS trim, then the tokens, generate()'s dict or score()'s.  A guided request
        (rows [:P] the prompts, [P:] their negatives) reports rows [:P], and its cache is an independent P-row copy of the conditional rows (dl_kv_place)."""
        cache.full_len_host = [n + produced - 1 for n in cache.full_len_host]  # every row's un-evicted length grows by one per decode step
        cache.seen_tokens += produced - 1
        P = st.B // 2 if req.guidance is not None else st.B
        out, finish = st.out_ids[:P, :produced].clone(), None
        if req.eos or req.stops:  # HF stops as soon as every row has finished (an EOS id, or a stop sequence's last token): trim the columns produced after that
            finish = stopping.finish_columns(out, req.eos, req.stops)
            first = int(finish.max().item())
            if first < out.shape[1]:
                out, scores, raw_logits, neg_logits = out[:, : first + 1], scores[: first + 1], raw_logits[: first + 1], neg_logits[: first + 1]
        self.last_cache = cache
        if tm is not None:
            tm["ev"][2].record()
            tm["new_tokens"] = int(out.shape[1])
            self.last_timing = tm
        if req.forced is not None:
            T = req.forced.shape[1]  # (the cache: an independent COPY -- a perplexity run is many calls of one shape, and detaching the slab, as below, would drop the graphs after each)
            return {"sequences": out, "past_key_values": cache.detached_copy(), "logits": tuple(raw_logits), "nll": st.nll[:, :T].clone(), "top1": st.top1[:, :T].clone()}
        if not req.want_dict:
            return out
        # the caller keeps this cache (the reference returns an independent one per call): detach it from the pool, the next generate() allocates a fresh
        # slab instead of overwriting this one; captured graphs hold raw pointers into the slab the caller now owns (and may free): drop them
        if req.guidance is not None:  # the conditional rows, copied out: the 2 P-row slab and the graphs captured on it stay with the model
            pairs = cache
            cache = self._new_cache(P, pairs.t_cap)
            ops.kv_place(pairs, cache, *self._pair_maps(P)[0], max_len=max(pairs.full_len_host[:P]))
            cache.full_len_host, cache.seen_tokens = list(pairs.full_len_host[:P]), max(pairs.full_len_host[:P])
            cache.logical_cap, cache.sparse_cap = pairs.logical_cap, pairs.sparse_cap
            # ... and what a continuation under forward() schedules by, as the plain path's cache carries it: the pair cache's bounds hold for all 2 P rows, so for these P
            cache.prefill_sparse_max = pairs.prefill_sparse_max
            cache.set_bounds(pairs.full_bound, pairs.sparse_bound)
            cache._sch = copy.deepcopy(pairs._sch)
            self.last_cache = cache
        else:
            self._cache_pool = None
            self._drop_graphs_on(cache.slab.data_ptr())
        res = {"sequences": out, "past_key_values": cache}
        if req.want_scores:
            res["scores"] = tuple(scores)
        if req.want_logits:
            res["logits"] = tuple(raw_logits)
            if req.guidance is not None:
                res["negative_logits"] = tuple(neg_logits)
        if req.n_lp >= 0:  # the columns `sequences` kept; after a row's first EOS (pad in `sequences`) 0.0 / -1
            W, n = out.shape[1], req.n_lp
            lp, top_lp, top_ids = st.lp[:P, :W].clone(), st.top_lp[:P, :W, :n].clone(), st.top_ids[:P, :W, :n].clone()
            if req.stops:  # (a row also finishes on a stop sequence: by its finish column)
                logprobs.mask_after_columns(finish, lp, top_lp, top_ids)
            else:
                logprobs.mask_after_eos(out, req.eos, lp, top_lp, top_ids)
            res["logprobs"] = lp
            if n > 0:
                res["top_logprobs"], res["top_logprob_ids"] = top_lp, top_ids
        if req.constraint is not None:  # replayed on the host over `sequences`: a row is complete when it ended through an EOS edge
            res["constraint_complete"] = constraints.complete(req.constraint, out.cpu()).to(out.device)
        return res
