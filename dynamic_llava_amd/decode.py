"""Decode side of the engine: the persistent step state (stable pointers for the hipGraph), the three step builders (GEMV / small-M / library), the pooled KV slab, the schedule that picks a captured step from the observed lengths, device-error reporting; of generate()'s stages, arming the state for a request (_bind_schedule, _arm) and the chunked decode loop (_decode_loop).  A mixin of DynamicLlavaLlamaForCausalLM (model.py)."""
from __future__ import annotations

import contextlib
import gc
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from . import hip_ops as ops
from .cache import KVSlabCache, KVSlabCacheMX8
from .config import IGNORE_INDEX


@dataclass(frozen=True)
class StepMode:
    """How the current request closes its steps (_bookkeep): which kernel picks the token and the host-side constants of the rule it then applies.  Hashable:
    one element of the graph keys."""
    eos: object = -1  # -1 (none), one id, or a tuple of up to three (the EOS set)
    pad: int = 0
    min_new: int = 0  # EOS is banned while step < min_new (HF semantics)
    sampled: bool = False  # dl_decode_sample: generate(do_sample=True, seed=...)
    forced: bool = False  # dl_decode_score: score() -- score the label, feed the label
    processed: bool = False  # dl_logits_process in front of the kernel; an all-neutral request is exactly the request without the keywords
    logprobs: int = -1  # dl_decode_logprobs behind the kernel: generate(output_logprobs=True, top_logprobs=n) -- -1: off, else n
    stop: bool = False  # dl_decode_stop as the last launch: generate(stop_sequences= / stopping_criteria=[keyword criterion]); the list itself is device data
    constrained: bool = False  # dl_logits_constrain in front of the kernel: generate(constraint= / guided_choice= / allowed_token_ids=); the automaton itself is device data
    guided: bool = False  # dl_logits_guide in front of everything, dl_pair_follow behind the kernel: generate(guidance_scale=) on paired rows; scale and cutoff are device data

    @classmethod
    def of(cls, req, max_new):
        """The mode of a parsed request (request.Request) of max_new steps; the one place the EOS tuple becomes the kernels' -1 / id / tuple."""
        return cls(eos=-1 if not req.eos else (req.eos[0] if len(req.eos) == 1 else req.eos), pad=req.pad, min_new=min(req.min_new, max_new), sampled=req.sampled is not None,
                   forced=req.forced is not None, processed=req.rules.on, logprobs=req.n_lp, stop=bool(req.stops), constrained=req.constraint is not None, guided=req.guidance is not None)


class _DecodeState:
    def __init__(self, model, B, device, dtype, out_cap):
        cfg = model.config
        H, I, V = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size
        nH, nKV, d = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
        self.B = B
        self.cur_ids = torch.zeros(B, dtype=torch.int64, device=device)
        self.out_ids = torch.zeros((B, max(out_cap, 1)), dtype=torch.int64, device=device)
        self.step = torch.zeros(B, dtype=torch.int32, device=device)
        self.finished = torch.zeros(B, dtype=torch.int32, device=device)
        self.decision = torch.ones(B, dtype=torch.int32, device=device)
        self.tp_logits = torch.zeros((B, 2), dtype=torch.float32, device=device)
        self.tp_ws = ops.text_predictor_workspace(B, cfg.sparse_config["d_model"], device)
        self.tp_x = torch.empty((B, H), dtype=dtype, device=device)  # snapshot of the hidden state entering layer `sparse_layer`
        self.tp_stream = torch.cuda.Stream(device=device)  # the predictor runs beside layers >= sparse_layer (graph fork/join)
        self.cu = torch.arange(0, B + 1, dtype=torch.int32, device=device)
        self.h = torch.empty((B, H), dtype=dtype, device=device)
        self.h2 = torch.empty((B, H), dtype=dtype, device=device)  # residual ping-pong partner (dl_gemv ADDNORM)
        self.x = torch.empty((B, H), dtype=dtype, device=device)
        self.qkv = torch.empty((B, (nH + 2 * nKV) * d), dtype=dtype, device=device)
        self.o = torch.empty((B, H), dtype=dtype, device=device)
        self.gu = torch.empty((B, I), dtype=dtype, device=device)  # act = silu(gate)*up, produced by the gate|up GEMV epilogue
        self.dn = torch.empty((B, H), dtype=dtype, device=device)
        # weight-streaming GEMV path for small decode batches (else torch/hipBLASLt GEMMs)
        self.use_gemv = B <= min(model.gemv_max_decode_batch, ops.gemv_max_batch(I, dtype), ops.gemv_max_batch(H, dtype))
        self.attn = torch.empty((B, nH * d), dtype=dtype, device=device)
        self.act = torch.empty((B, I), dtype=dtype, device=device)
        self.logits = torch.empty((B, V), dtype=dtype, device=device)
        # split-KV: enough workgroups to cover the chip (256 CUs) without drowning in partials
        self.n_splits = max(1, min(32, 1024 // max(1, B * nH)))
        self.attn_ws = ops.attn_decode_workspace(B, nH, d, 32, device)
        # decode batches past the GEMV range: dl_gemm_smallm (weights streamed into the matrix cores) up to smallm_max_decode_batch rows
        self.use_smallm = (not self.use_gemv) and B <= model.smallm_max_decode_batch and all(
            ops.gemm_smallm_ok(B, n, k, dtype) for n, k in (((nH + 2 * nKV) * d, H), (H, nH * d), (2 * I, H), (H, I), (V, H))
        )
        self.lin_ws = torch.empty(8 * B * max(2 * I, V), dtype=torch.float32, device=device) if self.use_smallm else None
        # MXFP8 decoder weights with set_decode_weight_format(max_batch=): the four projections of such a batch stream the codes (dl_gemm_mx8) -- row-major x, no
        # operand-order copies on this route; the lm_head keeps the route chosen above
        mx_shapes = (((nH + 2 * nKV) * d, H), (H, nH * d), (2 * I, H), (H, I))
        mb = getattr(model, "mx8_max_decode_batch", None)
        self.use_mx8_gemm = ((not self.use_gemv) and model.decode_weight_format == "mxfp8" and mb is not None and B <= mb
                             and getattr(model.model.layers[0], "mx8", None) is not None and all(ops.gemm_mx8_ok(B, n, k, dtype) for n, k in mx_shapes))
        self.mx8_ws = torch.empty(max(int(ops.lib().dl_gemm_mx8_workspace_bytes(B, n, k, 0)) for n, k in mx_shapes) // 4, dtype=torch.float32, device=device) if self.use_mx8_gemm else None
        # round 5: decode batches of packed_decode_mlp_min_batch..32 rows (configs[2] / [3]: 32) run their MLP on dl_linear_packed -- gate|up with the SiLU * up
        # epilogue writing `act` in fragment order, down_proj leaving 4 k ranges of fp32 partial sums for the residual-add / RMSNorm launch
        # (tools/bench_linear_packed.py, M = 32: 38.4 vs 44.8 us and 25.5 vs 31.7 us against the library) -- whatever q|k|v and o_proj run on
        l0 = model.model.layers[0]
        self.use_lp_mlp = (not self.use_gemv and not self.use_mx8_gemm and model.packed_decode_mlp_min_batch <= B <= 32 and model.packed_decode_mlp and getattr(l0, "wp_gu", None) is not None
                           and getattr(l0, "wp_down", None) is not None)
        if self.use_lp_mlp:
            n_el = lambda cols: int(ops.lib().dl_packed_x_bytes(B, cols)) // 2
            self.x_pk = torch.empty(n_el(H), dtype=dtype, device=device)
            self.act_pk = torch.empty(n_el(I), dtype=dtype, device=device)
            self.lp_parts = torch.empty(4 * B * H, dtype=torch.float32, device=device)
            self.qkv_parts = torch.empty(2 * B * (nH + 2 * nKV) * d, dtype=torch.float32, device=device)  # q|k|v's two k ranges, added by the attention launch
        self.o_parts = torch.empty(8 * B * H, dtype=torch.float32, device=device) if (self.use_smallm and not self.use_mx8_gemm and B <= 32 and getattr(l0, "wp_o", None) is not None) else None  # o_proj's k-range slices (dl_linear_tiles)
        self.graphs = {}  # captured decode steps, keyed by (slab, split factors, ...): see _run_decode_steps
        # dl_decode_sample's parameter block (temperature, top-k, top-p, seed, row base): device memory the captured launches read, rewritten by
        # generate() before the first launch of a sampled request -- one graph serves every setting
        self.sample_params = ops.sample_params_block(device)
        # dl_decode_score's label sequence and outputs (score()): refilled by the host before the first launch of a scoring request, outside any graph -- the
        # pointers are stable, so one captured graph serves every label sequence.  Slot j belongs to step j, like out_ids
        self.labels = torch.full(self.out_ids.shape, -100, dtype=torch.int64, device=device)
        self.nll = torch.zeros(self.out_ids.shape, dtype=torch.float32, device=device)
        self.top1 = torch.full(self.out_ids.shape, -1, dtype=torch.int64, device=device)
        # dl_logits_process (generate(repetition_penalty= / no_repeat_ngram_size= / bad_words_ids=)): its fp32 output, which the bookkeeping launch then reads in the place
        # of `logits`, its parameter block and its bad-word table -- device memory the captured launches read, rewritten by generate() before the first launch of
        # a processed request, like sample_params: one graph serves every setting
        self.proc_logits = torch.empty((B, V), dtype=torch.float32, device=device)
        self.logits_params = ops.logits_params_block(device)
        self.bad_words = ops.bad_words_table((), device)
        # dl_decode_logprobs' outputs (generate(output_logprobs=True)): made by need_logprobs() on the first such request -- a model that never asks keeps its
        # footprint -- and with the state thereafter; slot j belongs to step j, like out_ids
        self.lp = self.top_lp = self.top_ids = None
        # dl_decode_stop's table (generate(stop_sequences=)): device memory the captured launch reads, rewritten by generate() before the first launch of such a
        # request, like sample_params -- one graph serves every stop list
        self.stop_table = ops.stop_table_block(device)
        # dl_logits_constrain's automaton, start states and state history (generate(constraint= / guided_choice= / allowed_token_ids=)): made by need_constraint() on
        # the first such request and with the state thereafter; rewritten by generate() before the first launch of a constrained request -- one graph serves every automaton
        self.con_table = self.con_start = self.con_hist = None
        # dl_logits_guide's output and parameter block (generate(guidance_scale=): rows [0, B / 2) the prompts, row B / 2 + b prompt b's negative): made by
        # need_guidance() on the first such request and with the state thereafter; the block is rewritten before the first launch of a guided request
        self.guide_logits = self.guide_params = None
        self.tok_host = None  # generate(streamer=): ring of pinned token words beside obs_host, made by need_stream() on the first such request
        # dl_gemv_gu_tp's granules (batch 1; the predictor's stage 1 stages the row in LDS: H <= 5120)
        tpm = getattr(model.model, "output_text_score_predictor", None)
        self.tp_gran = ops.gemv_gu_tp_workspace(tpm.d_model, device) if (B == 1 and tpm is not None and dtype in (torch.bfloat16, torch.float16) and H <= 5120 and H % 8 == 0 and tpm.d_model % 32 == 0) else None
        # dl_gemv_qkv_attn's granules (batch 1, 16-bit dtypes at the decoder widths the kernel takes)
        self.qa_gran = ops.gemv_qkv_attn_workspace(nH, nKV, d, device) if (B == 1 and dtype in (torch.bfloat16, torch.float16) and d in (64, 128) and H * 2 <= 48 * 1024) else None
        self.blk_err = torch.zeros(1, dtype=torch.int32, device=device)
        # generate(): ring of pinned host words [lens (2 x B) | finished (B)] + events -- the decode loop observes the evicted lengths and the
        # EOS flags with non-blocking copies and reads them one chunk of steps late (the launch queue never drains)
        self.obs_host = torch.empty((4, 3 * B), dtype=torch.int32).pin_memory()
        self.obs_ev = [torch.cuda.Event() for _ in range(4)]
        self.n_cu = torch.cuda.get_device_properties(device).multi_processor_count

    def clear_granules(self):
        """The decode attention's in-kernel split merge validates its granules by tag = (position of the new token, layer): within a request positions only grow, but a slot left
        by an EARLIER REQUEST (or another cache, in a forward() loop) at the same position would match.  Tag 0 is never expected: one clear makes every older granule unmatchable."""
        self.attn_ws.zero_()
        if self.qa_gran is not None:
            self.qa_gran.zero_()  # and of dl_gemv_qkv_attn
        if self.tp_gran is not None:
            self.tp_gran.zero_()  # and of dl_gemv_gu_tp

    def need_logprobs(self):
        """Allocates the log-probability buffers once per state (the captured launches hold their pointers)."""
        if self.lp is None:
            from .logprobs import MAX_TOP_LOGPROBS

            B, cap, dev = *self.out_ids.shape, self.out_ids.device
            self.lp = torch.zeros((B, cap), dtype=torch.float32, device=dev)
            self.top_lp = torch.zeros((B, cap, MAX_TOP_LOGPROBS), dtype=torch.float32, device=dev)
            self.top_ids = torch.full((B, cap, MAX_TOP_LOGPROBS), -1, dtype=torch.int64, device=dev)


    def need_constraint(self):
        """Allocates dl_logits_constrain's table, start states and state history once per state (the captured launches hold their pointers)."""
        if self.con_table is None:
            B, cap, dev = *self.out_ids.shape, self.out_ids.device
            self.con_table = ops.constraint_table_block(dev)
            self.con_start = torch.full((B,), -1, dtype=torch.int32, device=dev)
            self.con_hist = torch.full((B, cap + 1), -1, dtype=torch.int32, device=dev)  # slot j: the state in which token j is chosen

    def need_guidance(self):
        """Allocates dl_logits_guide's fp32 [B, V] output and its parameter block once per state (the captured launches hold their pointers)."""
        if self.guide_logits is None:
            self.guide_logits = torch.empty(self.logits.shape, dtype=torch.float32, device=self.logits.device)
            self.guide_params = ops.guide_params_block(self.logits.device)

    def need_stream(self, chunk):
        """The pinned ring the chunks' tokens leave through (generate(streamer=)): 4 slots of B x chunk int64 words, one per observation in flight."""
        if self.tok_host is None or self.tok_host.shape[1] < self.B * chunk:
            self.tok_host = torch.empty((4, self.B * chunk), dtype=torch.int64).pin_memory()


@contextlib.contextmanager
def no_gc_during_capture():
    """Keeps Python's cyclic garbage collector from running while a stream is being captured.  A collection that starts in the middle of a capture can free a dead
    object cycle that owns device resources -- an abandoned model with its captured graphs, streams and pinned host buffers (a prefill entry's `run` closure
    makes a model such a cycle) -- and their destructors call runtime functions that are not permitted while any stream captures: the process aborts.
    torch.cuda.graph() of current torch no longer collects before it begins (only with torch.compiler.config.force_cudagraph_gc).  Whatever is dead is
    collected after the capture, at a time when freeing is legal."""
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was_enabled:
            gc.enable()


class DecodeScheduler:
    """Decode-step builders and their scheduling (methods of DynamicLlavaLlamaForCausalLM)."""

    def check_device_errors(self):
        """Raises if a launch with in-kernel hand-offs (dl_gemv_qkv_attn, dl_gemv_gu_tp) gave up on a wait since the last check (such a launch
        poisons its output instead of hanging).  Costs one device->host copy: call it where a sync is acceptable."""
        if self._lp_err is not None and self._lp_ws is not None:
            code = int(self._lp_err.item())
            if code != 0:
                self._lp_err.zero_()
                self._lp_ws.zero_()
                raise ops.HipOpsError("in-kernel hand-off aborted: dl_linear_packed (a k range's partial tiles never arrived)")
        st = self._dstate
        if st is not None:
            code = int(st.blk_err.item())
            if code != 0:
                st.blk_err.zero_()
                what = [n for bit, n in ((1, "dl_gemv_qkv_attn (attention never received its projection outputs)"), (2, "dl_gemv_gu_tp (a predictor stage never received its inputs)")) if code & bit]
                if code & ~3:
                    what.append(f"unknown error bits {code & ~3:#x}")
                raise ops.HipOpsError("in-kernel hand-off aborted: " + "; ".join(what))

    def _decode_step_kernels(self, st: _DecodeState, cache: KVSlabCache, advance: bool):
        if st.use_gemv:
            self._decode_step_gemv(st, cache)
        else:
            self._decode_step_gemm(st, cache)
        if advance:
            self._bookkeep(st, cache)

    def _bookkeep(self, st, cache):
        """The launch that closes a step: pick the token (argmax, a sampled one, or the label, scored), append it, set the EOS flags and advance the KV lengths
        by the predictor's decision.  cache None: the first token -- the prompt's KV lengths are already in place, so neither they nor the decision are passed."""
        lf, ls = (None, None) if cache is None else (cache.len_full, cache.len_sparse)
        dec = st.decision if cache is not None and self._use_tp() else None
        logits, m = st.logits, self._mode
        if m.guided:  # generate(guidance_scale=): HF's first processor -- both rows of a pair get the pair's guided scores (fp32, a buffer of its own); st.logits is never written
            if m.forced:
                raise ValueError("score() takes no guidance: a label is scored on the model's own logits")
            logits = ops.logits_guide(st.logits, st.guide_logits, st.guide_params)
        if m.processed:  # generate() with logits processors: they edit the step's logits on the row's own history (HF's order: before the selection rule)
            if m.forced:
                raise ValueError("score() takes no logits processors: a label is scored on the model's own logits")
            logits = ops.logits_process(logits, st.proc_logits, st.logits_params, st.out_ids, st.step, st.bad_words)
        if m.constrained:  # generate() with a constraint: behind the processors (HF's order), every token without an edge out of the row's state becomes -inf; st.logits is never written
            if m.forced:
                raise ValueError("score() takes no constraint: a label is scored on the model's own logits")
            logits = ops.logits_constrain(logits, st.proc_logits, st.con_table, st.con_start, st.con_hist, st.out_ids, st.step)
        if m.forced:  # score(): the same bookkeeping around the label, scored
            ops.decode_score(st.logits, st.cur_ids, st.labels, st.nll, st.top1, st.out_ids, st.step, st.finished, m.pad, lf, ls, dec)
        elif m.sampled:  # generate(do_sample=True, seed=...): the same bookkeeping around a sampled token
            ops.decode_sample(logits, st.cur_ids, st.sample_params, st.out_ids, st.step, st.finished, m.eos, m.pad, lf, ls, dec, min_new_tokens=m.min_new)
        else:  # EOS is banned while step < min_new (HF semantics)
            ops.decode_advance(logits, st.cur_ids, st.out_ids, st.step, st.finished, m.eos, m.pad, lf, ls, dec, min_new_tokens=m.min_new)
        if m.guided:  # the negative row follows its prompt's row (token, out_ids slot, finished flag): one history per pair, also when the two rows drew from two random streams
            ops.pair_follow(st.cur_ids, st.out_ids, st.step, st.finished)
        if m.logprobs >= 0:  # generate(output_logprobs=True): the committed token's log-probability on the step's RAW logits (slot step - 1)
            ops.decode_logprobs(st.logits, st.cur_ids, st.step, st.lp, m.logprobs, st.top_lp, st.top_ids)
        if m.stop:  # generate(stop_sequences=): a row whose tokens now end in a stop sequence is finished, as by an EOS token -- the last launch, so all above see today's flags
            ops.decode_stop(st.out_ids, st.step, st.finished, st.stop_table)

    def _use_tp(self):
        """The output text predictor decides in the decode step (it sits in front of a layer that exists)."""
        sc = self.config.sparse_config
        return bool(sc["use_text_predictor"] and sc["use_output_text_predictor"]) and sc["sparse_layer"] < self.config.num_hidden_layers

    def _attn_call_tag(self, i):
        """Layer i's call_tag for the stand-alone attention launches: >= 0 lets a split-KV launch merge its splits itself, -1 keeps the separate merge launch."""
        return (i & 0xff) if self.attn_inkernel_combine and self.config.num_hidden_layers >= 2 else -1

    def _tp_decide(self, st, h, side_stream):
        """F6: the text predictor's decision on h, the hidden state entering layer `sparse_layer` (DML:2377-2391).  Only the end-of-step length advance consumes
        it, so with side_stream it runs on a snapshot of h on st.tp_stream (a parallel branch of the captured graph), off the layer chain's critical
        path; the caller joins the stream before anything reads st.decision."""
        tp = self.model.output_text_score_predictor
        if side_stream:
            st.tp_x.copy_(h)
            st.tp_stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st.tp_stream):
                tp.decide(st.tp_x, st.tp_ws, st.tp_logits, st.decision)
        else:
            tp.decide(h, st.tp_ws, st.tp_logits, st.decision)

    def _streams_packed(self, st):
        """Batch 1, model-dtype format: the matrices that have a 12-bit packed copy (model._pack_decode_weights) stream it -- same bits out."""
        return self.decode_weight_pack and st.B == 1 and self.decode_weight_format is None

    def _layer_streams(self, st, layer):
        """-> what this step reads (q|k|v, o_proj, gate|up, down_proj) of `layer` from: the MXFP8 codes as a (q, scale) pair (set_decode_weight_format), the
        bf16pack.PackedBf16 copy where one exists and applies, else the model-dtype tensor.  ops.gemv_any and the fused launches' front doors take any of them."""
        if self.decode_weight_format == "mxfp8":
            m = layer.mx8
            return m["qkv"], m["o"], m["gu"], m["down"]
        pk = (getattr(layer, "pk", None) or {}) if self._streams_packed(st) else {}
        pk_qkv = getattr(layer, "pk_qkv", None) if self._streams_packed(st) and self.decode_weight_pack_qkv else None
        pk_down = pk.get("down")
        if pk_down is None and self._streams_packed(st) and self.decode_weight_pack_down:  # long rows only (model._pack_decode_weights)
            pk_down = getattr(layer, "pk_down", None)
        src = lambda p, w: w if p is None else p
        return src(pk_qkv, layer.w_qkv), src(pk.get("o"), layer.self_attn.o_proj.weight), src(pk.get("gu"), layer.w_gu), src(pk_down, layer.mlp.down_proj.weight)

    def _lm_head_stream(self, st):
        """The vocabulary projection's source, chosen as _layer_streams chooses (it has no MXFP8 codes)."""
        p = getattr(self, "_pk_lm_head", None) if self._streams_packed(st) else None
        return self.lm_head.weight if p is None else p

    def _decode_step_gemv(self, st: _DecodeState, cache: KVSlabCache):
        """Small-batch decode step: 5 weight-streaming launches per layer (GEMVs with fused residual-add+RMSNorm / SiLU*up prologues) + RoPE/KV append +
        split-KV attention.  One launch order for every weight storage (_layer_streams); per projection the step decides only whether the launch is the
        fused one.  The residual stream ping-pongs between st.h / st.h2."""
        cfg = self.config
        nH, nKV, d = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
        eps, SL = cfg.rms_norm_eps, cfg.sparse_config["sparse_layer"]
        cos, sin = self._rope
        use_tp = self._use_tp()
        torch.index_select(self.model.embed_tokens.weight, 0, st.cur_ids, out=st.h)
        h_cur, h_alt, delta = st.h, st.h2, None
        A = ops.GEMV_ADDNORM
        # MXFP8 decoder weights are a storage the two fused launches (dl_gemv_qkv_attn, dl_gemv_gu_tp) do not take: the unfused sequence runs instead (stand-alone
        # attention, the predictor's decide).  gu_grid_cap sizes the model-dtype and the packed gate|up launch only: dl_gemv_mx8 runs its default grid
        mx8 = self.decode_weight_format == "mxfp8"
        gu_grid = {} if mx8 else {"grid_cap": self.gu_grid_cap}
        for i, layer in enumerate(self.model.layers):
            lens = cache.len_of_layer(i)
            ns = cache.n_splits(i, st.B * nH)
            w_qkv, w_o, w_gu, w_down = self._layer_streams(st, layer)
            # q|k|v projection + single-split attention of a batch-1 layer in ONE launch (dl_gemv_qkv_attn: the attention workgroups fetch their
            # K/V rows while the weights stream and receive the projection as granules).  Same bodies as the two launches below, so the
            # results are bit-identical to them WHEN the stand-alone attention also runs four waves (KVSlabCache.eight_wave_single_split =
            # False, as the kernel tests set it); by default the stand-alone single-split launch of a small batch runs eight waves -- another
            # (equally valid) summation order, so DL_FUSE_QKV_ATTN=0 is an A/B of speed, not of bits (tokens / KV lengths: tested equal)
            fused_attn = self.fuse_qkv_attn and st.B == 1 and ns == 1 and st.qa_gran is not None and cache.kv_format is None and not mx8
            if fused_attn:
                ops.gemv_qkv_attn_any(w_qkv, st.qkv, h_cur, h_alt, delta, layer.input_layernorm.weight, eps, cos, sin, cache.len_full, lens, cache.k[i], cache.v[i],
                                      st.attn, st.qa_gran, i & 0xff, nH, nKV, d, err=st.blk_err, grid_cap=self.qkv_attn_grid_cap,
                                      n_splits=cache.fused_attn_splits(i, self.fused_attn_max_splits))
            else:
                ops.gemv_any(w_qkv, st.qkv, mode=A, h_in=h_cur, h_out=h_alt, delta=delta, norm_w=layer.input_layernorm.weight, eps=eps)
            if delta is not None:
                h_cur, h_alt = h_alt, h_cur
            # the predictor as extra workgroups of this layer's gate|up launch (dl_gemv_gu_tp): its input is that launch's h_in
            fused_tp = i == SL and use_tp and self.fuse_gu_tp and not self.tp_side_stream and st.B == 1 and st.tp_gran is not None and not mx8
            if i == SL and use_tp and not fused_tp:
                self._tp_decide(st, h_cur, self.tp_side_stream)
            # F8+F10+F9: RoPE, KV append at slot len[b] and ragged attention in one launch (1024-thread workgroups; split-KV
            # only when the row is long enough to need more than one workgroup per head)
            if not fused_attn:
                self._attn_decode_rope(st, cache, i, st.qkv, lens, ns, self._attn_call_tag(i))
            ops.gemv_any(w_o, st.o, x=st.attn)
            if fused_tp:
                tp = self.model.output_text_score_predictor
                ops.gemv_gu_tp_any(w_gu, st.gu, h_cur, h_alt, st.o, layer.post_attention_layernorm.weight, eps, tp._weights(), tp.d_model, st.tp_ws, st.tp_logits,
                                   st.decision, cache.len_full, st.tp_gran, i & 0xff, err=st.blk_err)
            else:
                ops.gemv_any(w_gu, st.gu, mode=A | ops.GEMV_OUT_SILU_PAIR, h_in=h_cur, h_out=h_alt, delta=st.o, norm_w=layer.post_attention_layernorm.weight, eps=eps, **gu_grid)
            h_cur, h_alt = h_alt, h_cur
            ops.gemv_any(w_down, st.dn, x=st.gu)
            delta = st.dn
        ops.gemv_any(self._lm_head_stream(st), st.logits, mode=A, h_in=h_cur, h_out=h_alt, delta=delta, norm_w=self.model.norm.weight, eps=eps)
        if use_tp and self.tp_side_stream:
            torch.cuda.current_stream().wait_stream(st.tp_stream)  # join before anything reads st.decision

    def _attn_decode_rope(self, st, cache, i, qkv, lens, ns, call_tag):
        """F8+F10+F9 of one decode layer: RoPE, KV append at slot len[b] and ragged split-KV attention, qkv [B, (nH+2nKV)*d] -> st.attn.  THE place that knows the
        cache's storage format: model-dtype slabs run dl_attn_decode_rope, an MXFP8 cache (KVSlabCacheMX8) dl_attn_decode_rope_kv8 -- same schedule (split factor,
        speculative chunk, four / eight waves); a lane holds 16 codes instead of 8 elements, so its trips request twice the keys (the same bytes); no in-launch merge."""
        cfg = self.config
        nH, nKV, d = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
        cos, sin = self._rope
        kif = cache.keys_in_flight(ns, st.B * nH)
        if cache.kv_format == "mxfp8":
            ops.attn_decode_rope_kv8(qkv, cos, sin, cache.len_full, lens, cache.k[i], cache.ks[i], cache.v[i], cache.vs[i], st.attn, st.attn_ws, ns, nH, nKV, d,
                                     keys_in_flight=2 * kif, chunk_keys=cache.spec_chunk(ns))
        else:
            ops.attn_decode_rope(qkv, cos, sin, cache.len_full, lens, cache.k[i], cache.v[i], st.attn, st.attn_ws, ns, nH, nKV, d, keys_in_flight=kif, chunk_keys=cache.spec_chunk(ns),
                                 call_tag=call_tag)

    def _kv_format_key(self, cache):
        """What a captured graph depends on beyond the code / slab pointer: the cache's storage format and its scale allocation."""
        sc = getattr(cache, "scales", None)
        return (cache.kv_format, None if sc is None else sc.data_ptr())

    def _new_cache(self, B, t_cap):
        """A KV cache in the model's storage format (set_kv_cache_format)."""
        cfg = self.config
        cls = KVSlabCacheMX8 if self.kv_cache_format == "mxfp8" else KVSlabCache
        return cls(cfg.num_hidden_layers, cfg.sparse_config["sparse_layer"], B, cfg.num_key_value_heads, cfg.head_dim, int(t_cap), self.dtype, self.device)

    def _decode_step_gemm(self, st: _DecodeState, cache: KVSlabCache):
        """Decode step for batches past the GEMV range (round 5, `profiles/r05_decode_batch_paths.txt`).  Up to smallm_max_decode_batch (32) rows:
        o_proj -- and q|k|v below packed_decode_qkv_min_batch (16) rows -- on dl_gemm_smallm (row-major weights streamed into the matrix cores, fp32
        split-K partials added by the residual-add / RMSNorm launch); from packed_decode_mlp_min_batch (4) rows the MLP, from 16 rows q|k|v too, on
        dl_linear_packed (operand-order weight copies; SiLU * up in the epilogue, down_proj as 4 k ranges of partial sums; the norm launches write the
        GEMMs' input in fragment order): 7 launches per layer.  Larger batches, or a model without operand copies: library GEMMs.
        MXFP8 decoder weights with max_batch >= B (st.use_mx8_gemm): the four projections of every layer on dl_gemm_mx8 instead (_decode_layer_gemm_mx8)."""
        cfg, sc = self.config, self.config.sparse_config
        nH, nKV, d = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
        eps, L, SL = cfg.rms_norm_eps, cfg.num_hidden_layers, sc["sparse_layer"]
        cos, sin = self._rope
        use_tp = self._use_tp()
        sm, ws = st.use_smallm, st.lin_ws
        torch.index_select(self.model.embed_tokens.weight, 0, st.cur_ids, out=st.h)
        lp_qkv = st.use_lp_mlp and st.B >= self.packed_decode_qkv_min_batch and getattr(self.model.layers[0], "wp_qkv", None) is not None
        qkv_parts = False
        if lp_qkv:
            nu_q, ks_q = self._lp_config(st.qkv.shape[1] // 16, False)
            qkv_parts = self.packed_decode_qkv_parts and st.B <= self.packed_decode_qkv_parts_max_batch and ks_q == 2 and self.dtype in (torch.bfloat16, torch.float16)
        ops.rmsnorm(st.h, self.model.layers[0].input_layernorm.weight, eps, out=st.x_pk if lp_qkv else st.x, packed=lp_qkv)
        for i, layer in enumerate(self.model.layers):
            if i == SL and use_tp:
                self._tp_decide(st, st.h, False)  # (this step keeps the predictor on the layer chain)
            lens = cache.len_of_layer(i)
            ns = cache.n_splits(i, st.B * nH)
            tag = self._attn_call_tag(i)
            if st.use_mx8_gemm:
                self._decode_layer_gemm_mx8(st, cache, i, layer, lens, ns, tag)
                continue
            if lp_qkv and qkv_parts and cache.keys_in_flight(ns, st.B * nH) == 64 and cache.kv_format is None:
                # round 6 (verdict r5 item 2c): the projection's two k ranges stay fp32 partial sums and the RoPE / append / attention launch adds them (each (row, head)
                # workgroup the 3 x head_dim values it reads): no hand-over inside the projection's launch.  In the step (profiles/r06_decode_qkv_parts.txt): the
                # projection 22.7 -> 20.5 us at 32 rows; the attention launch pays for the wider loads in front of its first score (24.3 -> 28.2 us in the first build,
                # most of it removed by taking q's RoPE partner half from the neighbouring lane instead of loading it): -2.2 % per step at 16 rows, -1.8 % at 24; at 32 rows
                # -0.6 % on equal prompts, +0.5 % on configs[2]'s ragged batch => up to packed_decode_qkv_parts_max_batch (24) rows
                parts_q = ops.linear_packed(st.x_pk, layer.wp_qkv, st.qkv.shape[1], out=st.qkv_parts, epilogue=ops.LP_PARTS, units_per_workgroup=nu_q, k_split=ks_q, x_packed_mk=(st.B, st.h.shape[1]))
                ops.attn_decode_rope_parts(parts_q, cos, sin, cache.len_full, lens, cache.k[i], cache.v[i], st.attn, st.attn_ws, ns, nH, nKV, d, chunk_keys=cache.spec_chunk(ns), call_tag=tag)
            else:
                if lp_qkv:
                    qkv = ops.linear_packed(st.x_pk, layer.wp_qkv, st.qkv.shape[1], out=st.qkv, units_per_workgroup=nu_q, k_split=ks_q, workspace=self._lp_ws if ks_q > 1 else None, err=self._lp_err,
                                            x_packed_mk=(st.B, st.h.shape[1]))
                else:
                    qkv = ops.gemm_smallm(st.x, layer.w_qkv, out=st.qkv, workspace=ws, n_slices=self.smallm_wide_slices) if sm else F.linear(st.x, layer.w_qkv)
                self._attn_decode_rope(st, cache, i, qkv, lens, ns, tag)
            nw = self.model.norm.weight if i + 1 == L else self.model.layers[i + 1].input_layernorm.weight
            lp = st.use_lp_mlp
            x_mlp = st.x_pk if lp else st.x  # the packed MLP reads its input in fragment order: the norm launch writes it that way
            if sm and self.tiles_o_proj and st.o_parts is not None and st.B >= self.tiles_o_proj_min_decode_batch and getattr(layer, "wp_o", None) is not None:
                # round 6: o_proj on dl_linear_tiles -- 1-2 row tiles x 128 neurons x 8 k ranges (256 workgroups), each consumer wave streaming its own operand-order
                # weight fragments five steps ahead; the slices go to the same residual-add / RMSNorm launch (dl_gemm_smallm's partial sums: 13.0 us at 32 rows)
                shp, ks_ = self._tiles_o_config(st.B, st.h.shape[1])
                parts = ops.linear_tiles(st.attn, layer.wp_o, st.h.shape[1], out=st.o_parts[: ks_ * st.B * st.h.shape[1]], epilogue=ops.LT_PARTS, tile_shape=shp, k_split=ks_)
                ops.add_rmsnorm_parts(st.h, parts, layer.post_attention_layernorm.weight, eps, out=x_mlp, packed=lp)
            elif sm:  # (o_proj on dl_linear_packed's partial sums instead: a tie at 8..32 rows, measured and dropped)
                parts, _ = ops.gemm_smallm_parts(st.attn, layer.self_attn.o_proj.weight, ws)
                ops.add_rmsnorm_parts(st.h, parts, layer.post_attention_layernorm.weight, eps, out=x_mlp, packed=lp)
            else:
                o = F.linear(st.attn, layer.self_attn.o_proj.weight)
                ops.add_rmsnorm(st.h, o, layer.post_attention_layernorm.weight, eps, out=x_mlp, packed=lp)
            if lp:
                H_, I2 = st.h.shape[1], layer.w_gu.shape[0]
                nu_g, ks_g = self._lp_config(I2 // 16, True)
                ops.linear_packed(st.x_pk, layer.wp_gu, I2, out=st.act_pk, epilogue=ops.LP_SILU_PAIR, units_per_workgroup=nu_g, k_split=ks_g, workspace=self._lp_ws if ks_g > 1 else None,
                                  err=self._lp_err, x_packed_mk=(st.B, H_), y_packed=True)
                nu_d, ks_d = self._lp_config_parts(H_ // 16)
                parts = ops.linear_packed(st.act_pk, layer.wp_down, H_, out=st.lp_parts, epilogue=ops.LP_PARTS, units_per_workgroup=nu_d, k_split=ks_d, x_packed_mk=(st.B, I2 // 2))
                nxt_pk = lp_qkv and i + 1 < L  # the final norm feeds lm_head: row-major
                ops.add_rmsnorm_parts(st.h, parts, nw, eps, out=st.x_pk if nxt_pk else st.x, packed=nxt_pk)
            elif sm:
                parts, _ = ops.gemm_smallm_parts(st.x, layer.w_gu, ws, n_slices=self.smallm_wide_slices)
                ops.silu_mul_parts(parts, st.act)
                parts, _ = ops.gemm_smallm_parts(st.act, layer.mlp.down_proj.weight, ws)
                ops.add_rmsnorm_parts(st.h, parts, nw, eps, out=st.x)
            else:
                ops.silu_mul(F.linear(st.x, layer.w_gu), out=st.act)
                dn = F.linear(st.act, layer.mlp.down_proj.weight)
                ops.add_rmsnorm(st.h, dn, nw, eps, out=st.x)
        if sm:
            ops.gemm_smallm(st.x, self.lm_head.weight, out=st.logits, workspace=ws)
        else:
            torch.matmul(st.x, self.lm_head.weight.t(), out=st.logits)

    def _decode_layer_gemm_mx8(self, st, cache, i, layer, lens, ns, tag):
        """One layer of _decode_step_gemm on MXFP8 weights (set_decode_weight_format(max_batch=)): its dl_gemm_smallm sequence with dl_gemm_mx8 streaming layer.mx8 --
        q|k|v in the model dtype for the RoPE / append / attention launch, o_proj, gate|up and down_proj as fp32 split-K partial sums that the residual-add / RMSNorm and
        SiLU * up launches add.  7 launches per layer (8 when q|k|v is split over K), x row-major throughout."""
        cfg = self.config
        nH, nKV, d, eps, L = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim, cfg.rms_norm_eps, cfg.num_hidden_layers
        cos, sin = self._rope
        m, ws = layer.mx8, st.mx8_ws
        ops.gemm_mx8(st.x, *m["qkv"], out=st.qkv, workspace=ws)
        self._attn_decode_rope(st, cache, i, st.qkv, lens, ns, tag)
        parts, _ = ops.gemm_mx8_parts(st.attn, *m["o"], ws)
        ops.add_rmsnorm_parts(st.h, parts, layer.post_attention_layernorm.weight, eps, out=st.x)
        parts, _ = ops.gemm_mx8_parts(st.x, *m["gu"], ws)
        ops.silu_mul_parts(parts, st.act)
        parts, _ = ops.gemm_mx8_parts(st.act, *m["down"], ws)
        nw = self.model.norm.weight if i + 1 == L else self.model.layers[i + 1].input_layernorm.weight
        ops.add_rmsnorm_parts(st.h, parts, nw, eps, out=st.x)

    def _pooled_cache(self, B, t_need):
        """generate() owns its cache, so the slab is reused across calls: stable pointers keep the captured hipGraphs valid."""
        cfg = self.config
        c = getattr(self, "_cache_pool", None)
        if c is None or c.batch != B or c.t_cap < t_need or c.dtype != self.dtype or c.sparse_layer != cfg.sparse_config["sparse_layer"] or c.kv_format != self.kv_cache_format:
            # slots are allocated in steps of 128: a stream of requests of slightly different lengths (VQAL:123-196) keeps ONE slab -- and with it
            # every captured graph that holds pointers into it -- instead of re-allocating whenever a prompt is a few tokens longer than any before
            old_ptr = None if c is None else c.slab.data_ptr()
            c = self._cache_pool = None  # (the old slab goes before the new one comes)
            c = self._cache_pool = self._new_cache(B, -(-int(t_need) // 128) * 128)
            if old_ptr is not None:  # graphs captured on the slab that has just been freed can never be replayed again
                self._drop_graphs_on(old_ptr)
        c.lens.zero_()
        c.full_len_host = [0] * B
        c.seen_tokens = 0
        c.logical_cap = int(t_need)  # a pooled (possibly larger) slab must compute exactly like a fresh one of the requested size
        c.sparse_cap = c.logical_cap
        c.set_bounds(None, None)
        return c

    def _fork_source(self, B, t_need):
        """generate(num_return_sequences=n)'s prefill target: a second pooled cache, of the PROMPT batch B and without a decode reserve (nothing is ever decoded on it),
        whose live rows dl_kv_fork copies into the B * n-row cache.  Made with it: the model-dtype [B, V] buffer of the prompts' last-position logits (_first_token)."""
        cfg = self.config
        c = self._fork_src_pool
        if c is None or c.batch != B or c.t_cap < t_need or c.dtype != self.dtype or c.sparse_layer != cfg.sparse_config["sparse_layer"] or c.kv_format != self.kv_cache_format:
            old_ptr = None if c is None else c.slab.data_ptr()
            c = self._fork_src_pool = None
            c = self._fork_src_pool = self._new_cache(B, -(-int(t_need) // 128) * 128)
            self._fork_logits = torch.empty((B, cfg.vocab_size), dtype=self.dtype, device=self.device)
            if old_ptr is not None:  # (the prefill graphs of forked requests hold both slabs' pointers, and their keys say so)
                self._drop_graphs_on(old_ptr)
        c.full_len_host = [0] * B
        c.seen_tokens = 0
        c.logical_cap = c.sparse_cap = int(t_need)
        c.set_bounds(None, None)
        return c

    def _fork_host_mirrors(self, src, cache, n):
        """The host mirrors of the B * n-row cache behind dl_kv_fork: every prompt's value n times (what _prefill_host_update left on the source)."""
        cache.full_len_host = [v for v in src.full_len_host for _ in range(n)]
        cache.seen_tokens = src.seen_tokens
        cache.sparse_cap = cache.logical_cap - (src.logical_cap - src.sparse_cap)  # the same slots dropped from a larger reserve
        cache.prefill_sparse_max = src.prefill_sparse_max
        cache.set_bounds(None, None)
        cache.sched_begin(max(cache.full_len_host), cache.prefill_sparse_max, self.decode_sync_every)

    def _place_host_mirrors(self, src, cache, row0, close):
        """The host mirrors of the 2 B-row cache of a guided request behind one of its two dl_kv_place launches: rows row0 .. take what _prefill_host_update left on the
        source; the bounds that hold for every row are the looser of the two prefills' (a text-only negative drops no image tokens).  close: the second one."""
        B = src.batch
        cache.full_len_host[row0 : row0 + B] = list(src.full_len_host)
        drop = src.logical_cap - src.sparse_cap
        first = row0 == 0
        cache.seen_tokens = src.seen_tokens if first else max(cache.seen_tokens, src.seen_tokens)
        cache._place_drop = drop if first else min(cache._place_drop, drop)
        cache.prefill_sparse_max = src.prefill_sparse_max if first else max(cache.prefill_sparse_max, src.prefill_sparse_max)
        if close:
            cache.sparse_cap = cache.logical_cap - cache._place_drop
            cache.set_bounds(None, None)
            cache.sched_begin(max(cache.full_len_host), cache.prefill_sparse_max, self.decode_sync_every)

    def _drop_graphs_on(self, ptr):
        """Forget every captured prefill and decode step whose key holds the slab pointer `ptr`: the slab was freed, or handed to a caller who may free it."""
        self._prefill_graphs = {k: v for k, v in self._prefill_graphs.items() if ptr not in k}
        if self._dstate is not None:
            self._dstate.graphs = {k: v for k, v in self._dstate.graphs.items() if ptr not in k}

    def _bind_schedule(self, st, cache):
        """The thresholds cache.n_splits / fused_attn_splits schedule this cache's decode steps by: this model's, for this state."""
        (cache.single_split_max_keys, cache.fused_single_keys), cache.min_keys_per_split = self._single_split_max_keys(st), self.min_keys_per_split

    def _arm(self, st, req, max_new):
        """Readies the persistent state for a request (request.Request) of max_new steps, outside any graph.  What it sets beyond the mode -- sampling parameters,
        the processors' settings and word list, score()'s labels -- is device data the captured launches read: one graph serves every value of them."""
        st.step.zero_(); st.finished.zero_(); st.decision.fill_(1)
        st.clear_granules()
        self._mode = StepMode.of(req, max_new)  # which bookkeeping kernel _first_token / the decode steps launch (and capture), and what it is told
        if req.sampled is not None:
            st.sample_params.copy_(ops.sample_params_words(*req.sampled))
        if req.rules.on:
            st.logits_params.copy_(ops.logits_params_words(req.rules.repetition_penalty, req.rules.no_repeat_ngram_size, len(req.rules.bad_words)))
            st.bad_words.copy_(ops.bad_words_table(req.rules.bad_words, "cpu"))
        if req.stops:
            st.stop_table.copy_(ops.stop_table_words(req.stops))
        if req.constraint is not None:
            st.need_constraint()
            ops.constraint_table_write(st.con_table, *req.constraint.words())
            pairs = 2 if req.guidance is not None else 1  # (a guided request: row B + b walks prompt b's automaton beside row b)
            st.con_start.copy_(torch.tensor(req.constraint.starts(st.B // (req.constraint.n_return * pairs)) * pairs, dtype=torch.int32))
            st.con_hist.fill_(-1)  # DONE: a slot no launch of this request reaches shows no earlier request's state
        if req.guidance is not None:
            st.need_guidance()
            st.guide_params.copy_(ops.guide_params_words(*req.guidance))
        if req.forced is not None:
            st.labels.fill_(IGNORE_INDEX)
            st.labels[:, : req.forced.shape[1]].copy_(req.forced)
            st.nll.zero_()
            st.top1.fill_(-1)
        if req.n_lp >= 0:  # dl_decode_logprobs' outputs: slots of this request that no launch reaches must not show an earlier request's values
            st.need_logprobs()
            st.lp.zero_(); st.top_lp.zero_(); st.top_ids.fill_(-1)
        if getattr(self, "_prefill_logits_buf", None) is None or self._prefill_logits_buf.shape != st.logits.shape:
            self._prefill_logits_buf = torch.empty(st.logits.shape, dtype=torch.float32, device=self.device)

    def _single_split_max_keys(self, st):
        """-> (largest row, in keys, that the fused q|k|v + attention launch takes; largest row it takes with ONE attention workgroup per head).
        Stand-alone launches: 256 keys as one workgroup per (row, head) (cache.py).  Inside dl_gemv_qkv_attn the slab part of the attention runs while
        the q|k|v weights still stream, so the break-even against `dl_gemv` + a split launch moves out with the stream's length, and further with
        several attention workgroups per head (round 4).  tools/bench_qkv_attn.py on 1x MI355X, one launch with 1 / 4 workgroups per head vs the two
        launches: 7B (100.7 MB of q|k|v, 17.8 us) 22.8 / 23.4 vs 26.8 at 256 keys, 25.2 / 23.6 vs 28.0 at 448, 27.8 / 25.7 vs 28.5 at 640, 29.1 / 28.2 vs
        28.3 at 768; 13B (157 MB, 28 us) 32.2 / 33.6 vs 37.5 at 384, 36.0 / 34.1 vs 38.1 at 640, 36.5 / 36.5 vs 39.0 at 768, 39.7 / 42.1 vs 39.9 at 1024."""
        from .cache import _SINGLE_SPLIT_MAX_KEYS
        if self.single_split_keys_override is not None:  # tests: force the schedule to change inside a short generation
            return int(self.single_split_keys_override), int(self.single_split_keys_override)
        if not (self.fuse_qkv_attn and st.B == 1 and st.use_gemv and st.qa_gran is not None) or self.decode_weight_format == "mxfp8" or self.kv_cache_format == "mxfp8":
            return _SINGLE_SPLIT_MAX_KEYS, _SINGLE_SPLIT_MAX_KEYS
        w = self.model.layers[0].w_qkv
        big = (w.numel() * w.element_size()) >= 130e6  # 13B-class stream
        if self.fused_attn_max_splits <= 1:
            return (576 if big else 384), (576 if big else 384)
        return (768 if big else 704), (576 if big else 256)

    def _get_dstate(self, B, out_cap):
        st = self._dstate
        if st is None or st.B != B or st.out_ids.shape[1] < out_cap:
            st = self._dstate = _DecodeState(self, B, self.device, self.dtype, out_cap)
            self._prefill_graphs = {}
        return st

    @staticmethod
    def _capture(fn, warm):
        """Warm `fn` up on a side stream (lazy hipBLASLt / allocator state), then capture it into a hipGraph."""
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            warm()
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with no_gc_during_capture(), torch.cuda.graph(g):
            out = fn()
        return g, out

    def _run_decode_steps(self, st, cache, n_steps):
        """Enqueue n greedy steps (graph replay when enabled)."""
        # what the captured launches depend on: the slab (pointers, strides), the split-KV factor of each length group (the only thing
        # the REQUESTED capacity changes -- keying on logical_cap / sparse_cap themselves would re-capture for every new prompt
        # length of a variable-length workload such as the VQA loader), tables, stop ids and the switches that pick kernels
        cfg = self.config
        nH, SL = cfg.num_attention_heads, cfg.sparse_config["sparse_layer"]
        splits = (cache.n_splits(0, st.B * nH), cache.n_splits(min(SL, cfg.num_hidden_layers - 1), st.B * nH), cache.n_splits(cfg.num_hidden_layers - 1, st.B * nH))
        fused_ns = (cache.fused_attn_splits(0, self.fused_attn_max_splits), cache.fused_attn_splits(cfg.num_hidden_layers - 1, self.fused_attn_max_splits)) if (st.B == 1 and st.qa_gran is not None) else (1, 1)
        key = (cache.slab.data_ptr(), cache.t_cap, splits, fused_ns, self._rope[0].data_ptr(),
               repr(cfg.sparse_config), self.attn_inkernel_combine, self.tp_side_stream, self.smallm_max_decode_batch, self.gemv_max_decode_batch, self.fuse_qkv_attn, self.fuse_gu_tp, KVSlabCache.eight_wave_single_split,
               self.decode_weight_pack, self.decode_weight_pack_plain, self.decode_weight_pack_qkv, self.decode_weight_pack_down, self.fused_attn_max_splits, self.qkv_attn_grid_cap, self.gu_grid_cap, self.packed_decode_qkv_min_batch, self.packed_decode_qkv_parts, self.packed_decode_qkv_parts_max_batch, self.decode_weight_format, self.mx8_max_decode_batch,
               self._kv_format_key(cache), self._mode)  # (the mode: sampled, scored or greedy -- which bookkeeping kernel was captured, its constants, and whether dl_logits_process runs in front of it; the sampling parameters, the labels, the processors' settings and the automaton of a constraint are device data, not part of the key)
        if not self.use_hip_graph:
            for _ in range(n_steps):
                self._decode_step_kernels(st, cache, True)
            return
        g = st.graphs.get(key)
        if g is None:
            # the warm-up executes one real step: snapshot / restore the state it advances.  (dl_decode_logprobs' outputs need no entry: the warm-up writes slot
            # `step` of st.lp / top_lp / top_ids from the logits of this very step, and the first replay below, back at the same `step`, writes that slot again)
            snap = (st.cur_ids.clone(), st.out_ids.clone(), st.step.clone(), st.finished.clone(), cache.lens.clone(), st.decision.clone())

            def warm():
                self._decode_step_kernels(st, cache, True)

            g, _ = self._capture(lambda: self._decode_step_kernels(st, cache, True), warm)
            st.cur_ids.copy_(snap[0]); st.out_ids.copy_(snap[1]); st.step.copy_(snap[2]); st.finished.copy_(snap[3]); cache.lens.copy_(snap[4]); st.decision.copy_(snap[5])
            if len(st.graphs) >= 12:  # a long generation walks through a few split factors as its rows grow (one capture each)
                st.graphs.pop(next(iter(st.graphs)))
            st.graphs[key] = g
        for _ in range(n_steps):
            g.replay()

    def _first_token(self, st, x_last, fork=None, place=None):
        """fork = (source cache, cache, n, host bound of the prompt lengths): generate(num_return_sequences=n) -- x_last holds the B prompts' last rows; their logits are computed at B rows, on the route a
        plain call of B rows takes (the same bits), the prompts' K/V is forked into the B * n-row cache and every logits row repeated n times in front of the bookkeeping.
        place: (source cache, cache, maps, row0, close, host bound of the prompt lengths): one of the two prefills of a guided request (generate(guidance_scale=)) -- x_last holds
        B rows' last rows, prompts (row0 = 0) or negative prompts (row0 = B); their logits are computed at B rows as above, dl_kv_place puts their K/V into rows row0 .. of the
        2 B-row cache and the logits go to the same rows of st.logits; only the closing one (the negatives') runs the first token's bookkeeping, on all 2 B rows."""
        logits, use_gemv = st.logits, st.use_gemv
        if fork is not None or place is not None:
            cfg, logits = self.config, self._fork_logits
            use_gemv = logits.shape[0] <= min(self.gemv_max_decode_batch, ops.gemv_max_batch(cfg.intermediate_size, self.dtype), ops.gemv_max_batch(cfg.hidden_size, self.dtype))  # _DecodeState.use_gemv at B rows
        if use_gemv and x_last.dim() == 2 and x_last.is_contiguous():
            # up to three rows: the weight-streaming GEMV the decode steps use for the same matrix (41 vs 61 us for the library's skinny GEMM at B=1)
            ops.gemv(self.lm_head.weight, logits, x=x_last)
        else:
            torch.matmul(x_last, self.lm_head.weight.t(), out=logits)
        if fork is not None:
            src, cache, n, max_len = fork
            ops.kv_fork(src, cache, n, max_len=max_len)  # (the prompts' lengths are read on the device; max_len, the longest row the plan allows, sizes the grid)
            st.logits.view(logits.shape[0], n, -1).copy_(logits[:, None, :].expand(-1, n, -1))
        if place is not None:
            src, cache, maps, row0, close, max_len = place
            ops.kv_place(src, cache, *maps, max_len=max_len)
            st.logits[row0 : row0 + logits.shape[0]].copy_(logits)
            if not close:
                return
        self._prefill_logits_buf.copy_(st.logits)
        self._bookkeep(st, None)  # first token: the prompt's KV lengths are already in place; label 0 is scored on / token 0 drawn (step = 0) from the prompt's last logits

    def _decode_loop(self, st, cache, max_new, sync_every, on_step=None, feed=None):
        """generate()'s decode loop behind the first token: chunks of captured steps, scheduled from the lengths the predictor actually leaves (DML:2377-2391,
        CU:153-164) -> the number of tokens produced (the first included).  on_step(j), when given, runs after step j: the steps are then enqueued one by one
        (the caller reads the step buffer after each); the schedule (chunks, bounds) is the same.  Before a chunk the host knows the un-evicted group's length
        exactly, and the evicted group's as OBSERVED after an earlier chunk (non-blocking copy into pinned memory, consumed one chunk late so that the host never
        waits for steps it has just enqueued) plus the steps enqueued since.  Those bounds pick the split-KV factor / the fused q|k|v+attention launch
        (cache.n_splits), i.e. which captured graph is replayed; the values are data, never timing, so the schedule is deterministic for a given request.
        feed (stopping.Feed, generate(streamer=)): a chunk's tokens travel with its observation -- one more non-blocking copy into pinned memory in front of the same
        event -- and are pushed when that observation is consumed; the chunks, the bounds and what is replayed do not change."""
        B, has_eos = st.B, self._mode.eos != -1 or self._mode.stop  # (a stop sequence ends a row as an EOS id does)
        stops = has_eos or self._mode.forced  # (score(): finished = labels exhausted)
        produced, chunks, pending = 1, 0, []  # pending: (ring slot, produced-when-copied, tokens in the chunk)
        if feed is not None:
            st.need_stream(max(1, int(sync_every)))
        cache.sched_begin(max(cache.full_len_host), getattr(cache, "prefill_sparse_max", None) or max(cache.full_len_host), sync_every)
        while produced < max_new:
            # EOS of a short answer (VQA: a few tokens) must not cost two chunks of wasted steps: the first chunks' flags are read blocking (one
            # ~50 us queue drain each), later ones one chunk late.  The SCHEDULE never uses an observation newer than one chunk old either way.
            keep_newest = 0 if (has_eos and chunks <= 2) else 1
            all_done = False
            while len(pending) > keep_newest:
                slot, at, n_tok = pending.pop(0)
                st.obs_ev[slot].synchronize()
                row = st.obs_host[slot]
                if feed is not None:
                    feed.push(st.tok_host[slot, : B * n_tok].view(B, n_tok)[: feed.seen.shape[0]].clone())  # (a guided request: the prompts' rows, the first half)
                cache.sched_observe(at, int(row[B : 2 * B].max()))
                all_done = all_done or (stops and int(row[2 * B :].min()) != 0)
            if all_done:
                break
            n = min(cache.sched_chunk(), max_new - produced)
            if on_step is None:
                self._run_decode_steps(st, cache, n)
            else:
                for i in range(n):
                    self._run_decode_steps(st, cache, 1)
                    on_step(produced + i)
            produced += n
            chunks += 1
            cache.sched_advance(n)
            if produced < max_new:
                slot = chunks % 4
                st.obs_host[slot, : 2 * B].copy_(cache.lens.view(-1), non_blocking=True)
                if stops:
                    st.obs_host[slot, 2 * B :].copy_(st.finished, non_blocking=True)
                if feed is not None:
                    st.tok_host[slot, : B * n].view(B, n).copy_(st.out_ids[:, produced - n : produced], non_blocking=True)
                st.obs_ev[slot].record()
                pending.append((slot, produced, n))
        return produced
