"""SrgptEngine: the region-grounded forward/generate path on one MI355X.

Stage map (reference file:line -> method):
  A1  VisionTower.forward            multimodal_encoder/vision_encoder.py:115-132   -> vit()
  A2  feature_refinement             region_extractor/base_extractor.py:137-147     -> feature_refinement()
  A3/4 MaskPooling + connectors      region_extractor/base_extractor.py:32-84,149-173 -> region_extractor()
  A5  mlp_downsample projector       multimodal_projector/base_projector.py:32-94   -> mm_projector()
  A6  token-stream splice            llava_arch.py:333-650                           -> prepare_inputs()
  A7-13 Llama prefill + greedy loop  modeling_llama.py + HF GenerationMixin          -> prefill()/generate_ids()
Every arithmetic step is a HIP kernel (spatialrgpt_amd/ops.py -> libsrgpt_hip.so); torch allocates buffers.
"""
from __future__ import annotations

import ctypes as C
import warnings
from typing import Dict, List, Optional, Sequence

import torch

from . import _lib as L
from . import ops
from .config import SrgptConfig
from .constants import IGNORE_INDEX, IMAGE_TOKEN_INDEX
from .generation import StopJudge
from .weights import PreparedWeights


class DecodeState:
    """Static KV cache + device-side decode bookkeeping for a (batch, max_pos) geometry."""

    def __init__(self, eng: "SrgptEngine", batch: int, max_pos: int, ws_tokens: int, max_new: int):
        cfg, dev, dt = eng.cfg, eng.device, eng.dtype
        self.batch, self.max_pos, self.ws_tokens, self.max_new = batch, max_pos, ws_tokens, max_new
        shape = (cfg.layers, batch, cfg.kv_heads, max_pos, cfg.head_dim)
        self.kcache = torch.empty(shape, device=dev, dtype=dt)
        self.vcache = torch.empty(shape, device=dev, dtype=dt)
        self.pos = torch.zeros((batch,), device=dev, dtype=torch.int32)
        self.tok = torch.zeros((batch,), device=dev, dtype=torch.int64)
        self.out_ids = torch.zeros((batch, max_new), device=dev, dtype=torch.int64)
        self.step = torch.zeros((1,), device=dev, dtype=torch.int32)
        self.logits = torch.empty((batch, eng.w.vocab), device=dev, dtype=torch.float32)
        lib = L.load()
        nbytes = lib.srgpt_llm_ws_bytes(C.byref(eng.w.llm), batch, ws_tokens)
        if nbytes < 0:
            raise RuntimeError("srgpt_llm_ws_bytes failed")
        self.ws = torch.zeros((nbytes,), device=dev, dtype=torch.uint8)  # zeroed once: holds the decode-attention arrival tickets
        st = L.LlmState()
        st.batch, st.max_pos, st.max_new, st.ws_tokens = batch, max_pos, max_new, ws_tokens
        st.kcache, st.vcache = self.kcache.data_ptr(), self.vcache.data_ptr()
        st.pos, st.tok, st.out_ids, st.step = self.pos.data_ptr(), self.tok.data_ptr(), self.out_ids.data_ptr(), self.step.data_ptr()
        st.ws, st.logits = self.ws.data_ptr(), self.logits.data_ptr()
        st.sampling = None
        self.c = st
        self.host_len = [0] * batch  # cached positions per row as known on the host (prefill lengths + steps taken)
        self.graphs = {}             # "greedy" / "sample" / "sample_full" (+ "+proc") -> captured decode step (the pick kernels differ);
        #                              "lookup" (+ "+sample" / "+sample_full") -> captured lookup step; "lookup_batch" (+ the same) -> the batched one
        self.sampler = L.SAMPLER_TOPK64  # which device sampler draws while c.sampling is set (SRGPT_SAMPLER_*)
        self.sampling: Optional[ops.SamplingParams] = None  # device parameter block of the draw; ONE address for the state's lifetime
        self.logits_proc: Optional[ops.LogitsProcParams] = None  # device block of the logits processors; ONE address likewise
        self.proc = None             # its device pointer while the processors are on for the running request, else None
        # the PENDING token of every row after a decode loop: picked (the last id the request kept) but not yet cached -- the next
        # append has to feed it first.  (ids [B, n] as the loop left them, kept ids per row), or None: nothing is pending
        self.pending = None
        self._pos_stale = False      # the device `pos` ran ahead of host_len (a decode loop that stopped early): see truncate()
        self.lookup = None           # prompt-lookup decoding: the lookup step's buffers and parameter block (ensure_lookup)
        self.lookup_b = None         # ... for a batch: the batched lookup step's buffers and parameter block (ensure_lookup_batch)
        self._eng = eng

    def seq_len(self) -> int:
        """cached positions (longest row) -- what `past_key_values[-1][-1].shape[-2]` is for the reference (llava_arch.py:364)."""
        return max(self.host_len)

    def pending_ids(self) -> Optional[torch.Tensor]:
        """the pending token of every row (int64 [B], device), or None when every picked token is in the cache"""
        if self.pending is None:
            return None
        ids, n = self.pending
        return ids[torch.arange(self.batch, device=ids.device), torch.tensor([k - 1 for k in n], device=ids.device)]

    def truncate(self, lens) -> "DecodeState":
        """Cut every row back to lens[b] <= its current length (an int: every row): the device `pos` and host_len are set, the rows
        beyond stay in memory and are overwritten by the next append.  This is what makes a shared prefix reusable (truncate to the
        prefix, append the next question) and what rolls back the step a stopped decode loop ran ahead.  A row that is cut drops
        its pending token."""
        lens = [int(lens)] * self.batch if isinstance(lens, int) else [int(v) for v in (lens.tolist() if isinstance(lens, torch.Tensor) else lens)]
        if len(lens) != self.batch or any(n < 0 or n > have for n, have in zip(lens, self.host_len)):
            raise ValueError(f"truncate: lens {lens} must be one length per row, each within 0 .. the row's {self.host_len} cached positions")
        if lens != self.host_len:
            self.pending = None
        self.pos.copy_(torch.tensor(lens, dtype=torch.int32), non_blocking=False)
        self.host_len = lens
        self._pos_stale = False
        return self

    def set_sampling(self, sampling: Optional[dict]):
        """None: the step picks argmax.  dict(temperature, top_k, top_p, seed[, sampler]): the step DRAWS (sample.hip) with the
        sampler kind `sampler` (default: the top-k-64 sampler); the parameters go to the state's device block (one small H2D copy),
        so the graph captured for a sampler kind serves every setting."""
        if sampling is None:
            self.c.sampling = None
            self.sampler = L.SAMPLER_TOPK64
            return
        self.sampler = int(sampling.get("sampler", L.SAMPLER_TOPK64))
        if self.sampling is None:
            self.sampling = ops.SamplingParams(self._eng.device, self.batch)
        self.sampling.set(sampling["temperature"], sampling.get("top_k"), sampling.get("top_p"), sampling.get("seed", 0))
        self.c.sampling = self.sampling.ptr()

    def set_logits_proc(self, proc: Optional[dict]):
        """None: the step picks from the raw logits (the entry points and graphs without processors).  dict(repetition_penalty,
        no_repeat_ngram_size, min_new_tokens, eos_token_ids): the step runs HF's logits processors on st.logits in front of the pick
        (logits_proc.hip); the parameters go to the state's device block, so the "+proc" graph of a pick kind serves every setting."""
        if proc is None:
            self.proc = None
            return
        if self.max_new > L.LOGITS_PROC_HISTORY_MAX:
            raise NotImplementedError(f"logits processors over {self.max_new} new tokens (served: {L.LOGITS_PROC_HISTORY_MAX})")
        if self.logits_proc is None:
            self.logits_proc = ops.LogitsProcParams(self._eng.device)
        self.logits_proc.set(**proc)
        self.proc = self.logits_proc.ptr()

    def _graph(self, key: str, create):
        """the captured graph `key`; first use: create(stream, out) captures it"""
        if key not in self.graphs:
            g = L.vp()
            L.check(create(ops._stream(), C.byref(g)))
            self.graphs[key] = g
        return self.graphs[key]

    def ensure_graph(self):
        key = "greedy" if not self.c.sampling else ("sample_full" if self.sampler == L.SAMPLER_FULL else "sample")
        if self.proc:
            key += "+proc"
        # proc = None goes as NULL: exactly the graph of the _ex form (same launches)
        return self._graph(key, lambda stream, g: L.load().srgpt_llm_decode_graph_create_proc(
            C.byref(self._eng.w.llm), C.byref(self.c), self.sampler, self.proc, stream, g))

    def ensure_lookup(self, K: int, max_ngram: int, prompt_ids: Optional[torch.Tensor]):
        """The lookup step's buffers (first use: workspace -- zeroed, it holds arrival tickets --, the [T, vocab] logits, the stats
        block, the prompt-id buffer) and parameter block for T = K + 1 rows; a change of T, of max_ngram or a prompt longer than the
        buffer rebuilds them and drops the captured lookup graphs.  While the state samples (set_sampling) the block also gets the
        workspace of that sampler kind for T rows, made on first use (lk["sample_ws"][kind]).  The prompt ids sit RIGHT-aligned in a
        buffer of fixed length behind -1 sentinels (which never match and are never drafted): one captured graph serves every prompt."""
        eng, dev = self._eng, self._eng.device
        T, n = int(K) + 1, 0 if prompt_ids is None else int(prompt_ids.numel())
        lk = self.lookup
        if lk is None or lk["T"] != T or lk["max_ngram"] != max_ngram or n > lk["cap"]:
            for key in [k for k in self.graphs if k.startswith("lookup")]:
                L.load().srgpt_graph_destroy(self.graphs.pop(key))
            nbytes = L.load().srgpt_llm_lookup_ws_bytes(C.byref(eng.w.llm), T)
            if nbytes < 0:
                raise RuntimeError("srgpt_llm_lookup_ws_bytes failed")
            cap = max(self.max_pos, n)
            lk = dict(T=T, max_ngram=max_ngram, cap=cap, ws=torch.zeros((nbytes,), device=dev, dtype=torch.uint8),
                      logits=torch.empty((T, eng.w.vocab), device=dev, dtype=torch.float32),
                      stats=torch.zeros((3,), device=dev, dtype=torch.int32),
                      prompt=torch.full((cap,), -1, device=dev, dtype=torch.int64), c=L.Lookup(), sample_ws={})
            c = lk["c"]
            c.T, c.max_ngram, c.prompt_ids, c.n_prompt = T, max_ngram, lk["prompt"].data_ptr(), cap
            c.ws, c.logits, c.stats = lk["ws"].data_ptr(), lk["logits"].data_ptr(), lk["stats"].data_ptr()
            self.lookup = lk
        lk["prompt"].fill_(-1)
        if n:
            lk["prompt"][lk["cap"] - n:].copy_(prompt_ids.reshape(-1).to(device=dev, dtype=torch.int64))
        lk["stats"].zero_()
        if self.c.sampling and self.sampler not in lk["sample_ws"]:
            nbytes = L.load().srgpt_llm_lookup_sample_ws_bytes(C.byref(eng.w.llm), T, self.sampler)
            if nbytes < 0:
                raise RuntimeError("srgpt_llm_lookup_sample_ws_bytes failed")
            lk["sample_ws"][self.sampler] = torch.empty((nbytes,), device=dev, dtype=torch.uint8)
        return lk

    def ensure_lookup_batch(self, K: int, max_ngram: int, prompt_ids: Optional[torch.Tensor], prompt_mask: Optional[torch.Tensor] = None):
        """ensure_lookup for the BATCHED step (srgpt_llm_lookup_step_batch): buffers for self.batch sequences of T = K + 1 rows, keyed
        by (batch, T) -- workspace (zeroed: arrival tickets), [B * T, vocab] logits, stats, the per-row emission counts `steps` [B],
        the prompt rows [B, cap] and their lengths `n_prompt` [B] on the device.  prompt_ids int64 [B, P] (None: no prompt ids, the
        rows draft from their generated ids alone), prompt_mask [B, P] (None: every id is valid): every row contributes its valid
        ids in order, packed to the front, sentinels included (they never match).  The addresses are fixed, so one captured graph
        serves every prompt.  While the state samples the block also gets that sampler kind's workspace for the B * T rows, as
        ensure_lookup's does."""
        eng, dev, B = self._eng, self._eng.device, self.batch
        T, n = int(K) + 1, 0 if prompt_ids is None else int(prompt_ids.shape[1])
        if prompt_ids is not None and (prompt_ids.dim() != 2 or prompt_ids.shape[0] != B):
            raise ValueError(f"ensure_lookup_batch: prompt_ids must be [{B}, P]")
        lk = self.lookup_b
        if lk is None or lk["T"] != T or lk["max_ngram"] != max_ngram or n > lk["cap"]:
            for key in [k for k in self.graphs if k.startswith("lookup_batch")]:
                L.load().srgpt_graph_destroy(self.graphs.pop(key))
            nbytes = L.load().srgpt_llm_lookup_batch_ws_bytes(C.byref(eng.w.llm), B, T)
            if nbytes < 0:
                raise RuntimeError("srgpt_llm_lookup_batch_ws_bytes failed")
            cap = max(self.max_pos, n)
            lk = dict(B=B, T=T, max_ngram=max_ngram, cap=cap, ws=torch.zeros((nbytes,), device=dev, dtype=torch.uint8),
                      logits=torch.empty((B * T, eng.w.vocab), device=dev, dtype=torch.float32),
                      stats=torch.zeros((3,), device=dev, dtype=torch.int32), steps=torch.zeros((B,), device=dev, dtype=torch.int32),
                      prompt=torch.full((B, cap), -1, device=dev, dtype=torch.int64),
                      n_prompt=torch.zeros((B,), device=dev, dtype=torch.int32), c=L.LookupBatch(), sample_ws={})
            c = lk["c"]
            c.T, c.max_ngram, c.prompt_ids, c.ld_prompt, c.n_prompt = T, max_ngram, lk["prompt"].data_ptr(), cap, lk["n_prompt"].data_ptr()
            c.steps, c.ws, c.logits, c.stats = lk["steps"].data_ptr(), lk["ws"].data_ptr(), lk["logits"].data_ptr(), lk["stats"].data_ptr()
            self.lookup_b = lk
        lk["prompt"].fill_(-1)
        lk["n_prompt"].zero_()
        if n:
            ids = prompt_ids.to(device=dev, dtype=torch.int64)
            keep = torch.ones_like(ids, dtype=torch.bool) if prompt_mask is None else prompt_mask.to(dev).bool()
            # a stable sort of the keep flags moves every row's valid ids to the front, order preserved (as generate() packs the embeddings)
            order = torch.argsort((~keep).to(torch.int8), dim=1, stable=True)
            lens = keep.sum(dim=1)
            packed = torch.where(torch.arange(n, device=dev)[None, :] < lens[:, None], torch.gather(ids, 1, order), torch.full_like(ids, -1))
            lk["prompt"][:, :n].copy_(packed)
            lk["n_prompt"].copy_(lens.to(torch.int32))
        lk["stats"].zero_()
        if self.c.sampling and self.sampler not in lk["sample_ws"]:
            nbytes = L.load().srgpt_llm_lookup_batch_sample_ws_bytes(C.byref(eng.w.llm), B, T, self.sampler)
            if nbytes < 0:
                raise RuntimeError("srgpt_llm_lookup_batch_sample_ws_bytes failed")
            lk["sample_ws"][self.sampler] = torch.empty((nbytes,), device=dev, dtype=torch.uint8)
        return lk

    def ensure_lookup_batch_graph(self):
        """the captured batched lookup step of the running request's pick: greedy, or sampled by the state's sampler kind (a graph
        key of its own each)"""
        key = "lookup_batch" + ("" if not self.c.sampling else ("+sample_full" if self.sampler == L.SAMPLER_FULL else "+sample"))
        return self._graph(key, lambda stream, g: L.load().srgpt_llm_lookup_graph_create_batch_ex(
            C.byref(self._eng.w.llm), C.byref(self.c), C.byref(self.lookup_b["c"]), self.sampler, self.lookup_sample_ws(True), stream, g))

    def lookup_sample_ws(self, batched: Optional[bool] = None):
        """device pointer of the running request's sampler workspace for the lookup step, sized for the state's B * T rows -- the
        batch-1 block's, or (batched; default: a state of 2+ rows) the batched block's; None: a greedy request"""
        if not self.c.sampling:
            return None
        batched = self.batch > 1 if batched is None else batched
        return (self.lookup_b if batched else self.lookup)["sample_ws"][self.sampler].data_ptr()

    def ensure_lookup_graph(self):
        """the captured lookup step of the running request's pick: greedy, or sampled by the state's sampler kind"""
        key = "lookup" if not self.c.sampling else ("lookup+sample_full" if self.sampler == L.SAMPLER_FULL else "lookup+sample")
        return self._graph(key, lambda stream, g: L.load().srgpt_llm_lookup_graph_create_ex(
            C.byref(self._eng.w.llm), C.byref(self.c), C.byref(self.lookup["c"]), self.sampler, self.lookup_sample_ws(), stream, g))

    def __del__(self):
        try:
            for g in self.graphs.values():
                L.load().srgpt_graph_destroy(g)
        except Exception:
            pass


class SplicePlan:
    """what srgpt_splice_plan left on the device (row -> source table, per-prompt facts) + the host's copy of the facts"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class SrgptEngine:
    def __init__(self, cfg: SrgptConfig, state_dict: Dict[str, torch.Tensor], device="cuda", dtype=torch.bfloat16,
                 rope_positions: int = 0, consume_state_dict: bool = False, llm_weight_format: str = "native", parts=None,
                 decode_layout: str = "packed", pack13=None, mxfp4_packed: bool = False, decode_pass_rows: int = 16,
                 mxfp4_prefill_direct: bool = False):
        L.load()  # fail loudly if the HIP extension is missing
        self.cfg, self.device, self.dtype = cfg, torch.device(device), dtype
        if self.device.type != "cuda":
            raise RuntimeError("SrgptEngine runs on an MI355X (torch device 'cuda'); there is no CPU path")
        if cfg.mm_projector_type != "mlp_downsample":
            raise ValueError(f"Unknown projector type: {cfg.mm_projector_type}")
        if cfg.enable_region and cfg.region_extractor_type != "regiongpt":
            raise NotImplementedError(f"{cfg.region_extractor_type} not implemented")  # base_extractor.py:160-161
        if cfg.select_feature not in ("cls_patch", "patch"):
            raise ValueError(f"Unexpected select feature: {cfg.select_feature}")
        # llm_weight_format: "native", "fp8", "fp8_w8a8", "mxfp4" or "mxfp4_w4a8" (= "mxfp4" whose prefill multiplies per-token e4m3
        # activations with the codes on the block-scaled MFMA, nothing expanded; the batched choice) -- weights.py
        # decode_layout "packed": fp8 LLM weights also get MFMA-operand-order copies for the batched decode step (weights.py)
        # pack13: bf16 weights also get lossless 13-bit copies the batch-1 decode step streams (weights.py; None: its default, True / False, "all" for tests)
        # decode_pass_rows: 16, or 32 = steps of 17 - 32 rows stream every weight matrix once (weights.py; read-only afterwards)
        # mxfp4_packed: "mxfp4" weights also get packed copies, bound, for the MFMA product of every step of 2+ rows (weights.py; default off)
        self.w = PreparedWeights(cfg, state_dict, self.device, dtype, rope_positions, consume=consume_state_dict,
                                 llm_weight_format=llm_weight_format, parts=parts, decode_layout=decode_layout, pack13=pack13,
                                 mxfp4_packed=mxfp4_packed, decode_pass_rows=decode_pass_rows,
                                 mxfp4_prefill_direct=mxfp4_prefill_direct)
        self._state: Optional[DecodeState] = None
        self._vit_ws: Optional[torch.Tensor] = None
        self.use_graph = True
        # the decode loop runs on its own stream: hipGraph capture is illegal on the legacy default stream
        self.stream = torch.cuda.Stream(device=self.device)

    @property
    def decode_pass_rows(self) -> int:
        """rows per weight pass of the decode step's MFMA products (16, or 32: the wide pass); set at construction"""
        return self.w.decode_pass_rows

    @property
    def mxfp4_prefill_direct(self) -> bool:
        """"mxfp4" weights: the prefill multiplies the codes inside the whole-M kernel too (weights.py); set at construction"""
        return self.w.mxfp4_prefill_direct

    # ------------------------------------------------------------------ A1
    def vit(self, images: torch.Tensor, out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
        """[n,3,S,S] (any float dtype: cast to the engine dtype at the boundary, vision_encoder.py:127) ->
        hidden_states[select_layer] [n, grid^2, C] in the ENGINE dtype; `out_dtype` reproduces the module-level cast back
        to the caller's image dtype (vision_encoder.py:130) for callers that use the tower on its own."""
        self._need("vit")
        x = images.to(device=self.device, dtype=self.dtype).contiguous()  # vision_encoder.py:127
        n, ch, S, S2 = x.shape
        if ch != 3 or S != self.cfg.image_size or S2 != S:
            raise ValueError(f"vision tower expects [n,3,{self.cfg.image_size},{self.cfg.image_size}] images, got {tuple(x.shape)}")
        lib = L.load()
        need = lib.srgpt_vit_ws_bytes(C.byref(self.w.vit), n)
        if self._vit_ws is None or self._vit_ws.numel() < need:
            self._vit_ws = torch.empty((need,), device=self.device, dtype=torch.uint8)
        out = torch.empty((n, self.cfg.tower_tokens, self.cfg.vit_hidden), device=self.device, dtype=self.dtype)
        L.check(lib.srgpt_vit_forward(C.byref(self.w.vit), x.data_ptr(), out.data_ptr(), self._vit_ws.data_ptr(), n, ops._stream()))
        if self.cfg.select_feature == "patch":
            out = out[:, 1:]  # feature_select drops token 0 whatever the tower (vision_encoder.py:28-29)
        return out if out_dtype is None or out_dtype == out.dtype else out.to(out_dtype)  # vision_encoder.py:130

    # ------------------------------------------------------------------ A2
    def _need(self, part: str):
        if part not in self.w.parts:
            raise RuntimeError(f"this engine was built without its {part!r} component (parts = {self.w.parts})")

    def feature_refinement(self, tower: torch.Tensor):
        self._need("region")
        tower = tower.to(device=self.device, dtype=self.dtype)
        n, HW, Cc = tower.shape
        g = int(HW ** 0.5)
        if g * g != HW:
            raise ValueError(f"feature_refinement needs a square token grid, got {HW} tokens")  # einops error in the reference
        w = self.w
        x = tower.reshape(n * HW, Cc)
        # ConvT(2,2) -> LayerNorm2d -> GELU -> ConvT(2,2) -> GELU, all channels-last
        y = ops.gemm(x, w.dc1_w, w.dc1_b, bias_mod=Cc, out_mode=L.OUT_DECONV2X, gw=g, out_shape=(n * 4 * HW, Cc))
        y = ops.layernorm(y, w.ln2d_w, w.ln2d_b, 1e-6, act=L.ACT_GELU_ERF)
        hres = ops.gemm(y, w.dc2_w, w.dc2_b, act=L.ACT_GELU_ERF, bias_mod=Cc, out_mode=L.OUT_DECONV2X, gw=2 * g,
                        out_shape=(n * 16 * HW, Cc))
        lres = ops.avgpool(hres, n, 4 * g, 27)  # AdaptiveAvgPool2d(27) is hard-coded (base_extractor.py:123)
        return hres.reshape(n, 16 * HW, Cc), lres

    # ------------------------------------------------------------------ A3 / A4
    def mask_pooling(self, feats: torch.Tensor, masks: Optional[Sequence[Optional[torch.Tensor]]]):
        n = feats.shape[0]
        if masks is None:
            masks = [None] * n
        out = []
        for i in range(n):
            m = masks[i]
            if m is None:
                out.append(None)
            elif m.dtype == torch.uint8:
                # raw uint8 masks [K, H, W]
                if self.cfg.image_aspect_ratio == "pad":
                    # process_regions' pad mode (mm_utils.py:505-531): zero square + the processor's bicubic resize on the device,
                    # then the pooling of float masks (soft edges: the nearest-tap fusion below does not apply)
                    from .mm_utils import masks_pad_resize_device

                    S = self.cfg.image_size
                    out.append(ops.region_pool(feats[i].to(self.dtype), masks_pad_resize_device(m.to(self.device), S, S, self.dtype)))
                    continue
                if self.cfg.image_aspect_ratio != "resize":
                    raise NotImplementedError(f"raw uint8 masks: image_aspect_ratio {self.cfg.image_aspect_ratio!r} "
                                              "(process_regions handles 'resize' and 'pad')")
                # "resize": nearest resize to the processor size + float + resample fused into the pooling kernel
                out.append(ops.region_pool_u8(feats[i].to(self.dtype), m.to(self.device), self.cfg.image_size))
            else:
                out.append(ops.region_pool(feats[i].to(self.dtype), m.to(self.device)))
        return out

    def region_extractor(self, hres, depth_features, masks):
        self._need("region")
        w = self.w

        def connect(pooled, W, b):
            return [None if p is None else ops.gemm(p, W, b) for p in pooled]

        mask_embeds = connect(self.mask_pooling(hres, masks), w.rgb_w, w.rgb_b)
        depth_embeds = None
        if depth_features is not None:
            depth_embeds = connect(self.mask_pooling(depth_features, masks), w.depth_w, w.depth_b)
        return mask_embeds, depth_embeds

    # ------------------------------------------------------------------ A5
    def mm_projector(self, lres: torch.Tensor) -> torch.Tensor:
        self._need("projector")
        w = self.w
        lres = lres.to(device=self.device, dtype=self.dtype)
        n = lres.shape[0]
        x = ops.s2d(lres)
        tokens = x.shape[1]
        x = ops.layernorm(x.reshape(n * tokens, -1), w.mp_ln_w, w.mp_ln_b, 1e-5)
        x = ops.gemm(x, w.mp_w1, w.mp_b1, act=L.ACT_GELU_ERF)
        x = ops.gemm(x, w.mp_w2, w.mp_b2)
        return x.reshape(n, tokens, -1)

    # ------------------------------------------------------------------ llava_arch.py:387-411
    def encode_visual(self, images, depths, masks, stages: Optional[dict] = None):
        cfg = self.cfg
        if isinstance(images, (list, tuple)):
            images = torch.cat(list(images), dim=0)
        elif images.ndim == 5:
            images = images.flatten(0, 1)
        if depths is not None:
            if isinstance(depths, (list, tuple)):
                depths = torch.cat(list(depths), dim=0)
            elif depths.ndim == 5:
                depths = depths.flatten(0, 1)
        n = images.shape[0]
        use_depth = cfg.enable_region and cfg.enable_depth and depths is not None
        # RGB and depth go through the tower as ONE batch of 2n images (same weights)
        # fp16 / fp32 callers (the reference's loader builds fp16: builder.py:62, eval_region_cls.py:316-317) are cast to the
        # engine dtype here and every intermediate stays in it -- the weights are only held in the engine dtype
        images = images.to(device=self.device, dtype=self.dtype)
        both = torch.cat([images, depths.to(device=self.device, dtype=self.dtype)], dim=0) if use_depth else images
        feats = self.vit(both)
        tower = feats[:n]
        mask_embeds = depth_embeds = None
        if cfg.enable_region:
            hres, lres = self.feature_refinement(tower.contiguous())
            depth_features = feats[n:].contiguous() if use_depth else None
            mask_embeds, depth_embeds = self.region_extractor(hres, depth_features, masks)
            if stages is not None:
                stages.update(hres=hres, lres=lres, depth_features=depth_features)
        else:
            lres = tower
        image_features = self.mm_projector(lres)
        if stages is not None:
            stages.update(tower_features=tower, image_features=image_features, mask_embeds=mask_embeds,
                          depth_embeds=depth_embeds)
        return image_features, mask_embeds, depth_embeds

    # ------------------------------------------------------------------ A6
    def _region_counts(self, masks, n_images: int):
        """rows of region embeddings each image will get (None: none) -- known from the mask list before any kernel runs"""
        if not self.cfg.enable_region:
            return None
        if masks is None:
            return [None] * n_images
        return [None if m is None else int(m.shape[0]) for m in masks]

    def splice_plan(self, input_ids: torch.Tensor, attention_mask, n_images: int, region_counts, have_depths: bool,
                    nimg_feat: Optional[int] = None, stats_buf: Optional[torch.Tensor] = None) -> "SplicePlan":
        """Token-stream splice, step 1 (llava_arch.py:420-611): the row -> source table of the whole batch, built ON THE DEVICE from
        the ids (csrc/splice.hip) -- the ids never travel; what comes back is 8 ints per prompt (lengths, counts, id range) for the
        batch length T and the reference's error / warning conditions.  prepare_inputs() calls this BEFORE it launches the vision
        tower, so the one read-back of the request waits for nothing."""
        cfg, dev = self.cfg, self.device
        ids = input_ids.detach().to(device=dev, dtype=torch.int64).contiguous()
        B, P = ids.shape
        am8 = None
        if attention_mask is not None:
            am8 = attention_mask.detach().to(device=dev).ne(0).to(torch.uint8).contiguous()
        nf = cfg.llm_image_tokens if nimg_feat is None else int(nimg_feat)
        use_masks = bool(cfg.enable_region and region_counts is not None)
        use_depths = bool(cfg.enable_region and cfg.enable_depth and have_depths and region_counts is not None)
        info, off = [], 0
        for i in range(n_images):
            c = region_counts[i] if (region_counts is not None and i < len(region_counts)) else None
            info += [-1 if c is None else c, off]
            off += 0 if c is None else c
        info_dev = torch.tensor(info or [0, 0], dtype=torch.int32).to(dev)
        Tcap = max(P + n_images * max(nf - 1, 0), 1)
        lib = L.load()
        desc = torch.empty((B, Tcap, 2), device=dev, dtype=torch.int32)
        if stats_buf is None:
            stats = torch.empty((B, L.SPLICE_STATS), device=dev, dtype=torch.int32)
        else:
            assert stats_buf.dtype == torch.int32 and stats_buf.is_contiguous() and stats_buf.numel() >= B * L.SPLICE_STATS
            stats = stats_buf[:B * L.SPLICE_STATS].view(B, L.SPLICE_STATS)
        scratch = torch.empty((max(int(lib.srgpt_splice_scratch_ints(B, n_images)), 1),), device=dev, dtype=torch.int32)
        mx = cfg.tokenizer_model_max_length
        L.check(lib.srgpt_splice_plan(ids.data_ptr(), None if am8 is None else am8.data_ptr(), B, P, nf, n_images, info_dev.data_ptr(),
                                      int(use_masks), int(use_depths), int(cfg.mask_token_id), int(cfg.depth_token_id),
                                      int(mx) if mx is not None else 0, Tcap, desc.data_ptr(), stats.data_ptr(), scratch.data_ptr(),
                                      ops._stream()))
        tail = None
        if stats_buf is None:
            host = stats.cpu().tolist()  # the request's one device -> host copy (B x 8 ints)
        else:
            flat = stats_buf.cpu().tolist()  # the same one copy, the caller's ints behind the statistics included
            host = [flat[b * L.SPLICE_STATS:(b + 1) * L.SPLICE_STATS] for b in range(B)]
            tail = flat[B * L.SPLICE_STATS:]
        for b, (ln, ln_raw, n_img, n_mask, n_depth, first_img, mn, mxid) in enumerate(host):
            if n_img > 0:
                if first_img + n_img > n_images:
                    raise IndexError(f"index {first_img + n_img - 1} is out of bounds for dimension 0 with size {n_images}: "
                                     "more <image> tokens than images")
                me = region_counts[first_img] if region_counts is not None else None
                if cfg.enable_region and me is None and n_mask > 0:
                    print("Error: mask embed is None, but the num of <mask> is not 0!!!")
                if cfg.enable_region and cfg.enable_depth and have_depths and me is None and n_depth > 0:
                    print("Error: depth embed is None, but the num of <depth> is not 0!!!")
                if use_masks and me is not None and n_mask > me:
                    raise RuntimeError(f"shape mismatch: {n_mask} <mask> tokens but only {me} mask embeddings")
                if use_depths and me is not None and n_depth > me:
                    raise RuntimeError(f"shape mismatch: {n_depth} <depth> tokens but only {me} depth embeddings")
        lo, hi = min(r[6] for r in host), max(r[7] for r in host)  # (0, 0) for a prompt without text rows
        if lo < 0 or hi >= self.w.vocab:
            raise IndexError(f"index out of range in self: token ids must be in [0, {self.w.vocab}), got [{lo}, {hi}]")
        if mx is not None and any(r[1] > mx for r in host):
            warnings.warn("Inputs truncated!")
        lens = [r[0] for r in host]
        return SplicePlan(ids=ids, B=B, P=P, nimg_feat=nf, n_images=n_images, Tcap=Tcap, desc=desc, stats=stats, lens=lens,
                          T=max(max(lens), 1), have_attention_mask=attention_mask is not None,
                          am_dtype=None if attention_mask is None else attention_mask.dtype,
                          region_counts=region_counts, have_depths=have_depths, attention_mask=attention_mask, stats_tail=tail)

    def splice_apply(self, plan: "SplicePlan", image_features, mask_embeds, depth_embeds, labels=None):
        """Token-stream splice, step 2: ONE gather launch writes every row of inputs_embeds [B, T, H] from its source (embedding
        table, image features, region embeddings, zeros for padding) and, when asked, the spliced labels / attention mask."""
        cfg, dev = self.cfg, self.device
        B, T, H = plan.B, plan.T, cfg.hidden
        # the plan's offsets into the concatenated region tables were computed from PREDICTED row counts (masks[i].shape[0]) before
        # the tower ran: what is gathered must have exactly those shapes, or the kernel reads the wrong rows / past a table
        if image_features.shape[0] != plan.n_images or image_features.shape[1] != plan.nimg_feat:
            raise RuntimeError(f"splice: planned for {plan.n_images} x {plan.nimg_feat} image rows, got {tuple(image_features.shape[:2])}")
        counts = plan.region_counts
        for what, embeds, planned in (("mask", mask_embeds, cfg.enable_region and counts is not None),
                                     ("depth", depth_embeds, cfg.enable_region and cfg.enable_depth and plan.have_depths and counts is not None)):
            if not planned:
                continue
            got = [] if embeds is None else [None if e is None else int(e.shape[0]) for e in embeds]
            got += [None] * (plan.n_images - len(got))
            if got != [counts[i] if i < len(counts) else None for i in range(plan.n_images)]:
                raise RuntimeError(f"splice: planned for {what} embeddings of {list(counts)} rows per image, got {got}")
        out = torch.empty((B * T, H), device=dev, dtype=self.dtype)
        feats = image_features.reshape(-1, H).to(dtype=self.dtype).contiguous()
        me = de = None
        if mask_embeds is not None and any(e is not None for e in mask_embeds):
            me = torch.cat([e for e in mask_embeds if e is not None], 0).to(self.dtype).contiguous()
        if depth_embeds is not None and any(e is not None for e in depth_embeds):
            de = torch.cat([e for e in depth_embeds if e is not None], 0).to(self.dtype).contiguous()
        lab = None if labels is None else labels.detach().to(device=dev, dtype=torch.int64).contiguous()
        lab_out = torch.empty((B, T), device=dev, dtype=torch.int64) if labels is not None else None
        am_out = torch.empty((B, T), device=dev, dtype=torch.uint8) if plan.have_attention_mask else None
        L.check(L.load().srgpt_splice_gather(plan.desc.data_ptr(), plan.stats.data_ptr(), B, plan.Tcap, T,
                                             int(cfg.padding_side == "left"), H, ops.dt_code(out), self.w.embed.data_ptr(),
                                             feats.data_ptr(), None if me is None else me.data_ptr(),
                                             None if de is None else de.data_ptr(), None if lab is None else lab.data_ptr(), plan.P,
                                             IGNORE_INDEX, out.data_ptr(), None if lab_out is None else lab_out.data_ptr(),
                                             None if am_out is None else am_out.data_ptr(), ops._stream()))
        am = None if am_out is None else am_out.to(plan.am_dtype)
        if labels is not None:
            return out.reshape(B, T, H), am, plan.lens, lab_out
        return out.reshape(B, T, H), am, plan.lens

    def splice(self, input_ids: torch.Tensor, attention_mask, image_features, mask_embeds, depth_embeds, have_depths,
               labels=None):
        """plan + gather for callers that already hold the visual features.
        Returns (inputs_embeds [B,T,H], attention_mask|None, lengths list); with `labels` ([B,P] int64) a 4th value: the
        spliced labels [B,T] on the device (IGNORE_INDEX over image rows and padding, llava_arch.py:513-533, :558-611)."""
        counts = None
        if self.cfg.enable_region and mask_embeds is not None:
            counts = [None if e is None else int(e.shape[0]) for e in mask_embeds]
        plan = self.splice_plan(input_ids, attention_mask, image_features.shape[0], counts,
                                have_depths and depth_embeds is not None, nimg_feat=image_features.shape[1])
        return self.splice_apply(plan, image_features, mask_embeds, depth_embeds, labels)

    def prepare_inputs(self, input_ids, images, depths=None, masks=None, attention_mask=None, stages=None, labels=None):
        # the splice is PLANNED first: its read-back (lengths, the reference's error conditions) happens while the GPU has nothing
        # queued; then the tower / refinement / pooling / projector launches go out back to back and the gather follows them
        if isinstance(images, (list, tuple)):
            n_images = sum(int(im.shape[0]) for im in images)
        else:
            n_images = int(images.shape[0] * images.shape[1]) if images.ndim == 5 else int(images.shape[0])
        counts = self._region_counts(masks, n_images)
        use_depth = self.cfg.enable_region and self.cfg.enable_depth and depths is not None
        plan = self.splice_plan(input_ids, attention_mask, n_images, counts, use_depth)
        image_features, mask_embeds, depth_embeds = self.encode_visual(images, depths, masks, stages)
        if image_features.shape[1] != plan.nimg_feat or image_features.shape[0] != plan.n_images:  # a geometry the config did not predict
            plan = self.splice_plan(input_ids, attention_mask, image_features.shape[0], counts, use_depth,
                                    nimg_feat=image_features.shape[1])
        res = self.splice_apply(plan, image_features, mask_embeds, depth_embeds, labels)
        if stages is not None:
            stages["inputs_embeds"] = res[0]
        return res

    def _check_ids(self, ids) -> None:
        """nn.Embedding raises IndexError for ids outside [0, vocab); the row-gather kernel would read out of bounds
        (e.g. the -200 sentinel on an images=None path, or <mask>/<depth> ids past a table that was never resized)."""
        if isinstance(ids, torch.Tensor):
            if ids.numel() == 0:
                return
            lo, hi = int(ids.min()), int(ids.max())
        else:
            if not ids:
                return
            lo, hi = min(ids), max(ids)
        if lo < 0 or hi >= self.w.vocab:
            raise IndexError(f"index out of range in self: token ids must be in [0, {self.w.vocab}), got [{lo}, {hi}]")

    def embed_tokens(self, input_ids: torch.Tensor) -> torch.Tensor:
        B, P = input_ids.shape
        self._check_ids(input_ids)
        return ops.embed_rows(self.w.embed, input_ids.to(self.device)).reshape(B, P, -1)

    # ------------------------------------------------------------------ A7-A13
    def _get_state(self, batch: int, T: int, max_new: int, fresh: bool = False) -> DecodeState:
        """Cache/workspace for `batch` sequences of T prompt positions + max_new generated ones.  The pooled state serves the
        internal generate() path; `fresh=True` allocates an independent one (a handle returned to the caller as
        `past_key_values` must not be overwritten by the next call -- the reference returns independent caches)."""
        self._need("llm")
        need_pos = T + max_new
        if need_pos > self.w.rope_len:
            raise ValueError(f"sequence of {need_pos} positions exceeds the RoPE table ({self.w.rope_len})")
        # positions are capped by the RoPE table: a cache longer than it would let decode steps index past its end
        max_pos = min((need_pos + 127) // 128 * 128, self.w.rope_len)
        if fresh:
            return DecodeState(self, batch, max_pos, max(T, 1), max_new)
        s = self._state
        if s is None or s.batch != batch or s.max_pos < need_pos or s.ws_tokens < T or s.max_new < max_new:
            self._state = None
            s = DecodeState(self, batch, max_pos, max(T, 1), max_new)
            self._state = s
        return s

    def new_state(self, batch: int, capacity: int, max_new: int, ws_tokens: Optional[int] = None) -> DecodeState:
        """An independent, empty DecodeState whose cache holds `capacity` positions per row -- the caller's choice, where _get_state
        derives it from one request: the handle of a conversation (append() turn after turn) or of a shared prefix.  ws_tokens:
        rows per sequence one prefill / append call may carry (default: capacity); longer segments are appended in chunks."""
        self._need("llm")
        if capacity <= 0 or capacity > self.w.rope_len:
            raise ValueError(f"cache of {capacity} positions: must be within 1 .. the RoPE table ({self.w.rope_len})")
        return DecodeState(self, batch, int(capacity), max(min(int(ws_tokens or capacity), int(capacity)), 1), max(int(max_new), 1))

    def prefill(self, inputs_embeds: torch.Tensor, max_new: int = 1, all_logits: bool = False, hidden_states: bool = False,
                lens: Optional[torch.Tensor] = None, fresh_state: bool = False, state: Optional[DecodeState] = None):
        """inputs_embeds [B,T,H]; `lens` (int [B]) marks a RIGHT-padded ragged batch: row b has lens[b] valid positions,
        its logits come from position lens[b]-1 and decoding continues there.  `state`: prefill THIS state (new_state) instead of
        the pooled / a derived one.  Returns (state, logits_all|None, hiddens|None)."""
        B, T, H = inputs_embeds.shape
        x = inputs_embeds.to(device=self.device, dtype=self.dtype).contiguous()
        if state is not None:
            if state.batch != B or T > state.ws_tokens or T + max_new > state.max_pos or max_new > state.max_new:
                raise ValueError(f"prefill: the given state (batch {state.batch}, {state.max_pos} positions, {state.ws_tokens} rows per "
                                 f"call, {state.max_new} new tokens) cannot hold {B} x {T} rows + {max_new} new tokens")
            st = state
        else:
            st = self._get_state(B, T, max_new, fresh=fresh_state)
        al = torch.empty((B, T, self.w.vocab), device=self.device, dtype=torch.float32) if all_logits else None
        hs = torch.empty((self.cfg.layers + 1, B, T, H), device=self.device, dtype=self.dtype) if hidden_states else None
        if lens is None:
            L.check(L.load().srgpt_llm_prefill(C.byref(self.w.llm), C.byref(st.c), x.data_ptr(), T,
                                               None if al is None else al.data_ptr(), None if hs is None else hs.data_ptr(),
                                               ops._stream()))
        else:
            ld = lens.to(device=self.device, dtype=torch.int32).contiguous()
            if ld.shape != (B,):
                raise ValueError(f"prefill: lens must have shape ({B},)")
            L.check(L.load().srgpt_llm_prefill_ragged(C.byref(self.w.llm), C.byref(st.c), x.data_ptr(), T, ld.data_ptr(),
                                                      None if al is None else al.data_ptr(),
                                                      None if hs is None else hs.data_ptr(), ops._stream()))
        st.host_len = [T] * B if lens is None else [int(v) for v in lens.tolist()]
        st.pending, st._pos_stale = None, False
        return st, al, hs

    def append(self, st: DecodeState, inputs_embeds: torch.Tensor, lens: Optional[torch.Tensor] = None, all_logits: bool = False,
               hidden_states: bool = False):
        """Continue every row of a live state with a multi-token segment (HF `forward(input_ids[B, T > 1], past_key_values=...)`,
        srgpt_llm_prefill_append): inputs_embeds [B,T,H] RIGHT-padded, `lens` (int [B]) the rows to append per sequence (None: T
        each).  Row b continues at its live length; st.logits holds the logits of every row's last appended position afterwards.
        With lens = None a segment longer than st.ws_tokens runs as consecutive appends of at most ws_tokens rows (chunked prefill
        with a bounded workspace).  Returns (state, logits_all [B,T,V]|None, hiddens [layers+1,B,T,H]|None) for the NEW rows."""
        B, T, H = inputs_embeds.shape
        if B != st.batch or T < 1:
            raise ValueError(f"append: inputs_embeds must be [{st.batch}, T >= 1, hidden]")
        cap = min(st.max_pos, self.w.rope_len)
        if max(st.host_len) + T > cap:
            raise ValueError(f"KV cache full ({cap} positions, {max(st.host_len)} live + {T} appended): re-run forward() with a larger "
                             "cache_reserve / a longer RoPE table")
        ld, lens_h = None, None
        if lens is not None:
            if T > st.ws_tokens:
                raise ValueError(f"append: a ragged segment of {T} rows exceeds the state's {st.ws_tokens} rows per call")
            lens_h = [int(v) for v in (lens.tolist() if isinstance(lens, torch.Tensor) else lens)]
            if len(lens_h) != B or min(lens_h) < 1 or max(lens_h) > T:
                raise ValueError(f"append: lens must be {B} lengths within 1 .. {T}")
            ld = torch.tensor(lens_h, dtype=torch.int32).to(self.device)
        if st._pos_stale:
            st.truncate(list(st.host_len))  # a decode loop stopped early: the device position ran ahead of the kept tokens
        x = inputs_embeds.to(device=self.device, dtype=self.dtype).contiguous()
        lib, als, hss = L.load(), [], []
        for t0 in range(0, T, st.ws_tokens):
            n = min(st.ws_tokens, T - t0)
            xc = x if n == T else x[:, t0:t0 + n].contiguous()
            al = torch.empty((B, n, self.w.vocab), device=self.device, dtype=torch.float32) if all_logits else None
            hs = torch.empty((self.cfg.layers + 1, B, n, H), device=self.device, dtype=self.dtype) if hidden_states else None
            L.check(lib.srgpt_llm_prefill_append(C.byref(self.w.llm), C.byref(st.c), xc.data_ptr(), n, None if ld is None else ld.data_ptr(),
                                                 max(st.host_len), None if al is None else al.data_ptr(),
                                                 None if hs is None else hs.data_ptr(), ops._stream()))
            st.host_len = [a + (n if lens_h is None else lens_h[b]) for b, a in enumerate(st.host_len)]
            als.append(al)
            hss.append(hs)
        st.pending = None
        return (st, (als[0] if len(als) == 1 else torch.cat(als, 1)) if all_logits else None,
                (hss[0] if len(hss) == 1 else torch.cat(hss, 2)) if hidden_states else None)

    def step(self, st: DecodeState, input_ids: torch.Tensor) -> torch.Tensor:
        """One incremental forward over a cached state (HF `forward(input_ids[B,1], past_key_values=...)`): appends the
        tokens at every row's next position and returns the fp32 logits [B, vocab]."""
        if input_ids.shape != (st.batch, 1):
            raise ValueError(f"step: input_ids must be [{st.batch}, 1]")
        if max(st.host_len) >= min(st.max_pos, self.w.rope_len):
            raise ValueError(f"KV cache full ({min(st.max_pos, self.w.rope_len)} positions): re-run forward() with a larger "
                             "cache_reserve / a longer RoPE table")
        self._check_ids(input_ids)
        st.tok.copy_(input_ids[:, 0].to(device=self.device, dtype=torch.int64))
        L.check(L.load().srgpt_llm_decode_step(C.byref(self.w.llm), C.byref(st.c), ops._stream()))
        st.host_len = [n + 1 for n in st.host_len]
        st.pending = None
        return st.logits.clone()

    def greedy_decode(self, st: DecodeState, max_new_tokens: int, eos_token_id=None, pad_token_id=None,
                      stopping_criteria=None, sampling: Optional[dict] = None, logits_proc: Optional[dict] = None,
                      lookup: Optional[dict] = None) -> torch.Tensor:
        """HF generation-loop semantics (new ids only, finished rows padded), device-side steps via hipGraph.
        sampling = None: greedy.  sampling = dict(temperature, top_k, top_p, seed[, sampler]): every step DRAWS its token on the
        device (temperature -> top-k -> top-p -> categorical, sample.hip; `sampler` = L.SAMPLER_FULL for the settings the top-k-64
        sampler does not serve) -- same loop, same graph mechanism, no per-token host work.
        logits_proc = dict(repetition_penalty, no_repeat_ngram_size, min_new_tokens, eos_token_ids): HF's logits processors run on
        the device in front of every pick (DecodeState.set_logits_proc); None: the steps without them.
        lookup = dict(K, max_ngram, prompt_ids): prompt-lookup decoding (batch 1, no processors -- the caller checks): every step
        carries the next token and K ids drafted from prompt_ids + the generated ids (srgpt_llm_lookup_step_ex) and emits 1 .. K + 1
        tokens.  Greedy: the same ids, stop step and state as the plain loop.  With `sampling`: every row's token is DRAWN (row t at
        Philox counter + t), the drafts are kept up to the first draw that differs -- generated id i is a draw from the model's
        distribution at counter c0 + i, as in the plain sampled loop.  self.last_lookup_stats = what it did.
        A state of 2+ rows (batch * (K + 1) <= 16; lookup also carries prompt_ids [B, P] and prompt_mask): batched lookup
        steps (srgpt_llm_lookup_step_batch_ex) -- every row drafted from its own ids and advanced by its own
        accepted drafts; ids, padding and length as the plain batched loop's.  With `sampling` every one of the B * (K + 1) rows
        is drawn, row t of sequence b at the Philox address the plain sampled batched loop reads for that id (csrc/draw_addr.h)."""
        batched = lookup is not None and st.batch > 1  # the caller opted in (LlavaLlamaModel.lookup_batch; generation.plan_lookup)
        if lookup is not None and logits_proc is not None:
            raise ValueError("greedy_decode(lookup=...) takes a batch-1 request without logits processors")
        if batched and st.batch * (lookup["K"] + 1) > L.LOOKUP_ROWS_MAX:
            raise ValueError(f"greedy_decode(lookup=...) on batch {st.batch}: a request of batch * (K + 1) <= {L.LOOKUP_ROWS_MAX} rows")
        cur = torch.cuda.current_stream(self.device)
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            st.set_sampling(sampling)
            st.set_logits_proc(logits_proc)
            try:
                if lookup is not None:
                    n_keep, eos, n_rows = self._lookup_loop(st, max_new_tokens, eos_token_id, stopping_criteria, lookup)
                else:
                    n_keep, eos, n_rows = self._decode_loop(st, max_new_tokens, eos_token_id, stopping_criteria)
            finally:
                st.c.sampling = None
                st.sampler = L.SAMPLER_TOPK64
                st.proc = None
        cur.wait_stream(self.stream)
        # the decode attention hands partials between workgroups inside a launch (arrival tickets): a ticket left non-zero means a
        # launch merged nothing and later steps used stale attention output -- fail loudly, never return such ids
        if batched:
            L.check(L.load().srgpt_llm_lookup_sync_state_batch(C.byref(self.w.llm), C.byref(st.c), C.byref(st.lookup_b["c"]), ops._stream()))
        elif lookup is not None:  # the lookup workspace's own tickets, then the same check
            L.check(L.load().srgpt_llm_lookup_sync_state(C.byref(self.w.llm), C.byref(st.c), C.byref(st.lookup["c"]), ops._stream()))
        else:
            L.check(L.load().srgpt_llm_decode_sync_state(C.byref(self.w.llm), C.byref(st.c), ops._stream()))
        out = st.out_ids[:, :n_keep].clone()
        # n kept tokens of a row (up to and including its first EOS) are n - 1 cached positions behind the prompt: the last one is
        # PENDING, picked but not cached.  The device position may be ahead (a finished row of a batch keeps stepping; a stopped
        # loop ran one step ahead): truncate() rolls it back before the state is continued
        st.host_len = [a + n - 1 for a, n in zip(st.host_len, n_rows)]
        st.pending, st._pos_stale = (out, n_rows), True
        if eos:
            # rows that finished early are padded with pad_token_id (HF behaviour)
            pad = pad_token_id if pad_token_id is not None else eos[0]  # HF: pad defaults to the FIRST eos id
            is_eos = (out[:, :, None] == torch.tensor(eos, device=out.device, dtype=out.dtype)[None, None, :]).any(-1)
            after = (is_eos.int().cumsum(dim=1) - is_eos.int()) > 0  # strictly after a row's first EOS
            out = torch.where(after, torch.full_like(out, pad), out)
        return out

    def _decode_loop(self, st: DecodeState, max_new_tokens: int, eos_token_id, stopping_criteria):
        lib, stream = L.load(), ops._stream()
        L.check(lib.srgpt_llm_sample_first_proc(C.byref(self.w.llm), C.byref(st.c), st.sampler, st.proc, stream))  # proc None: NULL
        judge = StopJudge(st.batch, eos_token_id, stopping_criteria, max_new_tokens)
        graph = st.ensure_graph() if self.use_graph and max_new_tokens > 1 else None

        def launch(n=1):
            if graph is not None:
                L.check(lib.srgpt_graph_launch(graph, n, stream))
            else:
                for _ in range(n):
                    L.check(lib.srgpt_llm_decode_step_proc(C.byref(self.w.llm), C.byref(st.c), st.sampler, st.proc, stream))

        if judge.can_stop:
            # anything that can end the request early is judged EVERY step, one step behind the device.  Round 3 scanned for EOS
            # every `check_every` = 8 steps: a request that ends in EOS -- the reference's real eval mode, eval_spatial.py:221-237,
            # answers of a few dozen tokens -- ran 3.5 steps (10 ms at 2.9 ms per token) past its end on average; the run-ahead
            # loop wastes at most ONE step and costs 1.6 % while it runs (profiles/r04_sampling.txt)
            n_keep = self._run_ahead(judge, launch, _ColumnSource(st, max_new_tokens))
            return n_keep, judge.eos, judge.rows(n_keep)
        # nothing can stop the request early (the benchmark: EOS disabled): all steps are queued at once, no host work per token
        if max_new_tokens > 1:
            launch(max_new_tokens - 1)
        return max_new_tokens, judge.eos, [max_new_tokens] * st.batch

    def _lookup_loop(self, st: DecodeState, max_new_tokens: int, eos_token_id, stopping_criteria, lookup: dict):
        """The run-ahead loop over lookup steps: srgpt_llm_lookup_step_ex for one sequence, srgpt_llm_lookup_step_batch_ex for B
        rows (greedy or sampled, both).  A step emits a number of tokens per row only the device knows, so every
        round reads the per-row counts (st.step / lk["steps"]), the stats block and out_ids[:, :max_new_tokens] behind the previous
        step (_PrefixSource) -- after the NEXT step went out -- and StopJudge judges them as the plain loop would: the same ids, stop
        step and state.  What the device emitted behind the kept ids (the rest of an accepted run, the step that ran ahead, rows
        that accepted more than the others) lies beyond them and the live cache rows, exactly like the plain loop's one step ahead:
        truncate() rolls the device positions back.  A row at st.max_new ids is frozen on the device until the others arrive.
        With nothing that can stop the request the loop still reads the counts: how many steps max_new_tokens ids take is not
        known in advance."""
        lib, stream, B = L.load(), ops._stream(), st.batch
        judge = StopJudge(B, eos_token_id, stopping_criteria, max_new_tokens)
        if B == 1:
            lk = st.ensure_lookup(lookup["K"], lookup["max_ngram"], lookup.get("prompt_ids"))
        else:
            lk = st.ensure_lookup_batch(lookup["K"], lookup["max_ngram"], lookup.get("prompt_ids"), lookup.get("prompt_mask"))
        L.check(lib.srgpt_llm_sample_first_proc(C.byref(self.w.llm), C.byref(st.c), st.sampler, None, stream))
        if B > 1:
            lk["steps"].fill_(1)  # every row has emitted its first id
        graph = None
        if self.use_graph and max_new_tokens > 1:
            graph = st.ensure_lookup_graph() if B == 1 else st.ensure_lookup_batch_graph()

        def launch():
            if graph is not None:
                L.check(lib.srgpt_graph_launch(graph, 1, stream))
            elif B == 1:
                L.check(lib.srgpt_llm_lookup_step_ex(C.byref(self.w.llm), C.byref(st.c), C.byref(lk["c"]), st.sampler,
                                                     st.lookup_sample_ws(), stream))
            else:
                L.check(lib.srgpt_llm_lookup_step_batch_ex(C.byref(self.w.llm), C.byref(st.c), C.byref(lk["c"]), st.sampler,
                                                           st.lookup_sample_ws(), stream))

        source = _PrefixSource(st, max_new_tokens, st.step if B == 1 else lk["steps"], lk["stats"])
        n_keep = self._run_ahead(judge, launch, source)
        rows = judge.rows(n_keep)
        steps, drafted, accepted = source.stats()
        self.last_lookup_stats = dict(steps=steps, tokens=sum(rows), drafted=drafted, accepted=accepted, **({"batch": B} if B > 1 else {}))
        return n_keep, judge.eos, rows

    def _run_ahead(self, judge: StopJudge, launch, source) -> int:
        """A stopping criterion (the demo's KeywordsStoppingCriteria, gradio_web_server_multi.py:195-197; model_vqa.py's conv stop
        strings) is host Python over the ids so far: HF evaluates it after every token.  Round 3 did launch -> D2H -> Python ->
        launch, serialising the device behind the host every token.  Here step t + 1 is launched BEFORE step t is judged: the
        ids of step t travel on a side stream behind an event recorded after step t (so the copy does not wait for step t + 1),
        the judge runs while step t + 1 computes, and a stop discards the one step that ran ahead (it only wrote cache rows
        and ids beyond the kept prefix).  Same ids, same stop step as the serial loop.
        `launch()` queues one step; `source` (_ColumnSource / _PrefixSource) queues the copies of what a step left and reads them
        on the host.  -> the columns the request keeps."""
        if getattr(self, "_copy_stream", None) is None:
            self._copy_stream = torch.cuda.Stream(device=self.device)
        dec = torch.cuda.current_stream(self.device)

        def mark():
            ev = torch.cuda.Event()
            ev.record(dec)
            return ev

        ev = mark()  # the first token of every row (srgpt_llm_sample_first) is on the stream
        try:
            for t in range(judge.max_new_tokens + 1):  # every step emits at least one id per live row
                with torch.cuda.stream(self._copy_stream):
                    self._copy_stream.wait_event(ev)
                    source.queue(t)
                    ready = torch.cuda.Event()
                    ready.record(self._copy_stream)
                if source.more(t):
                    launch()  # run ahead: the next step goes out before the ids behind `ev` are judged
                    ev = mark()
                ready.synchronize()
                n_keep = judge.feed(source.ids, source.have(t))
                if n_keep is not None:
                    return n_keep
            raise RuntimeError("decode loop: a row's device step counter did not advance")
        finally:
            dec.wait_stream(self._copy_stream)


class _ColumnSource:
    """What a PLAIN step leaves, for _run_ahead: after step t every row has t + 1 ids (the host knows without a read-back), so only
    the column out_ids[:, t] travels, and the last step goes out in round max_new_tokens - 2."""

    def __init__(self, st: DecodeState, max_new_tokens: int):
        # One step's ids are the COLUMN out_ids[:, t]: a strided source for B > 1, and torch serves a strided D2H through a pageable
        # temporary plus a host-side copy that no event covers.  So the column is gathered into a contiguous device
        # scratch on the copy stream and leaves as ONE contiguous copy into a pinned, step-major buffer: the round's event covers
        # everything the judge reads.
        self.st, self.n = st, max_new_tokens
        self.host_t = torch.empty((max_new_tokens, st.batch), dtype=torch.int64).pin_memory()
        self.ids = self.host_t.t()  # [B, steps] view for the judge (HF criteria index ids[b, -n:])
        self.scratch = torch.empty((st.batch,), dtype=torch.int64, device=st.out_ids.device)
        assert self.host_t.is_pinned() and self.host_t[0].is_contiguous() and self.scratch.is_contiguous()

    def more(self, t: int) -> bool:
        return t + 1 < self.n

    def queue(self, t: int):
        self.scratch.copy_(self.st.out_ids[:, t])               # device gather (copy stream: ordered behind the previous D2H)
        self.host_t[t].copy_(self.scratch, non_blocking=True)   # contiguous, pinned: truly asynchronous

    def have(self, t: int) -> List[int]:
        return [t + 1] * self.st.batch


class _PrefixSource:
    """What a LOOKUP step leaves, for _run_ahead: every row emitted a number of ids only the device knows, so the per-row counts
    (`counts`, int32 [B]), the three-int stats block and out_ids[:, :max_new_tokens] travel every round, and a next step goes out
    every round."""

    def __init__(self, st: DecodeState, max_new_tokens: int, counts: torch.Tensor, stats: torch.Tensor):
        B = st.batch
        self.B, self.n, self.counts, self.stats_dev = B, max_new_tokens, counts, stats
        self.ids = torch.empty((B, max_new_tokens), dtype=torch.int64).pin_memory()
        self.cnt = torch.empty((B + 3,), dtype=torch.int32).pin_memory()  # the rows' counts, then the stats block
        self.src, self.dst, self.scratch = st.out_ids[:, :max_new_tokens], self.ids, None
        if B == 1:  # one row: contiguous as it lies, it leaves as it is
            self.src, self.dst = self.src[0], self.dst[0]
        else:
            # out_ids[:, :max_new_tokens] is strided when the state holds more ids per row: gathered into a contiguous device scratch on
            # the copy stream, it leaves as one contiguous copy into pinned memory (the reason _ColumnSource gives)
            self.scratch = torch.empty((B, max_new_tokens), dtype=torch.int64, device=st.out_ids.device)

    def more(self, t: int) -> bool:
        return self.n > 1

    def queue(self, t: int):
        self.cnt[:self.B].copy_(self.counts, non_blocking=True)
        self.cnt[self.B:].copy_(self.stats_dev, non_blocking=True)
        if self.scratch is None:
            self.dst.copy_(self.src, non_blocking=True)
        else:
            self.scratch.copy_(self.src)
            self.dst.copy_(self.scratch, non_blocking=True)

    def have(self, t: int) -> List[int]:
        return [min(int(v), self.n) for v in self.cnt[:self.B].tolist()]

    def stats(self):
        """(steps, drafted, accepted) as last read"""
        return tuple(int(v) for v in self.cnt[self.B:].tolist())
