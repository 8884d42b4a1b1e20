"""Weight layout in HBM.

Input: a state dict with the reference's checkpoint key names (llava/model/llava_arch.py:181-250:
sub-dirs llm/ vision_tower/ mm_projector/ region_extractor/; HF 4.37.2 key names inside).
Output: device tensors arranged for the kernels --
  * q/k/v rows concatenated ([q;k;v], one GEMM / one weight stream per layer), gate/up rows concatenated
  * patch-embed conv flattened to [C, 3*p*p] and zero-padded to a 16-byte multiple
  * ConvTranspose2d(k=2,s=2) weights [Cin,Cout,2,2] re-laid as [(a,b,co), ci] so the deconv is a GEMM whose
    output columns are contiguous channels of one output pixel
  * RoPE cos/sin tables (fp32 angle, cast to the model dtype -- modeling_llama.py:81-130)
and the ctypes structs (include/srgpt.h) that point at them.
"""
from __future__ import annotations

from typing import Dict, List

import torch

from . import _lib as L
from .config import SrgptConfig

VT = "vision_tower.vision_tower.vision_model."
RE = "region_extractor."
MP = "mm_projector.layers."
LM = "llm."

# Lossless 13-bit packed copies (include/srgpt.h, srgpt_pack13) of the matrices the batch-1 bf16 decode step streams: which products
# get one, by the per-product measurement of profiles/pack13.txt -- a product is listed only where its packed kernel's median beat
# the raw kernel's minimum: gate/up (37.1 -> 33.7 us) and lm_head (163 -> 137 us); q/k/v (10.3 -> 11.8) and down_proj (21.1 ->
# 26.6) stay raw.  o_proj was never a candidate: its raw register kernel reads weights the attention launch prefetched into L2.
PACK13_PRODUCTS = ("wgu", "lm_head")
PACK13_DEFAULT = True


def _ptr_array(tensors: List[torch.Tensor]):
    arr = (L.vp * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = None if t is None else t.data_ptr()
    return arr


def rope_tables(cfg: SrgptConfig, n_pos: int, dtype, device):
    d = cfg.head_dim
    inv_freq = 1.0 / (cfg.rope_theta ** (torch.arange(0, d, 2, dtype=torch.int64).float() / d))
    pos = torch.arange(n_pos, dtype=torch.int64).float()
    if cfg.rope_factor != 1.0:
        # linear scaling (context_length_extension, language_model/builder.py:31-38): the reference's vendored
        # LlamaLinearScalingRotaryEmbedding divides the fp32 POSITIONS (modeling_llama.py:133-140); dividing inv_freq instead
        # rounds differently for factors that are not powers of two (pinned by tests/golden/vendored_llama_kat.npz)
        pos = pos / cfg.rope_factor
    freqs = pos[:, None] * inv_freq[None, :]  # fp32, as LlamaRotaryEmbedding (autocast disabled)
    return freqs.cos().to(dtype).to(device).contiguous(), freqs.sin().to(dtype).to(device).contiguous()


class PreparedWeights:
    """Owns the device tensors and the C structs pointing at them."""

    ALL_PARTS = ("vit", "region", "projector", "llm")

    def __init__(self, cfg: SrgptConfig, sd: Dict[str, torch.Tensor], device, dtype, rope_positions: int = 0,
                 consume: bool = False, llm_weight_format: str = "native", parts=None, decode_layout: str = "packed",
                 pack13=None, mxfp4_packed: bool = False, decode_pass_rows: int = 16, mxfp4_prefill_direct: bool = False):
        """llm_weight_format: "native" (the engine dtype) or "fp8" -- weight-only OCP e4m3fn quantisation of the five
        streamed LLM matrices with one fp32 (power-of-two) scale per output row (BASELINE config 5; bf16 engines only).  The
        fp8 bytes are the ONLY copy of those matrices in HBM: decode streams them (srgpt_gemv_w8), prefill multiplies them
        (srgpt_gemm_w8); `dequantised(name, layer)` rebuilds the bf16 values for checks.
        "mxfp4": the 4-bit option (bf16 engines only) -- the four per-layer matrices as OCP e2m1 codes with one E8M0 scale per 32
        values (ops.quantize_mxfp4_rows; include/srgpt.h, srgpt_gemv_w4), a quarter of the bf16 bytes and the only copy in HBM;
        lm_head is held as under "fp8".  Decode streams the codes (srgpt_gemv_w4); prefill expands each matrix into a bf16 scratch
        just before its product.  Opt-in, it changes the numbers; its accuracy cost on a trained checkpoint is unmeasured.
        "mxfp4_w4a8": the same codes and scales (`llm_weight_format` then reads "mxfp4" and `fp8_act` True, as "fp8_w8a8" reads
        "fp8"); prefill, ragged prefill and append prefill quantise every GEMM input per token to e4m3 and multiply it with the
        codes on the block-scaled fp8 x fp4 MFMA (srgpt_gemm_w4a8) -- no bf16 expansion at any row count and no expansion scratch in
        the workspace; the decode steps are "mxfp4"'s.  Widths must be multiples of 128.  Changes the prefill's numbers once more
        (quantised activations); the batched choice, "mxfp4" + mxfp4_prefill_direct being the batch-1 one.
        pack13 (bf16 engines, "native" only): also hold the PACK13_PRODUCTS as lossless 13-bit codes and bind them, so that the
        batch-1 decode step streams 0.8125 of their bytes and computes the same bits.  None: PACK13_DEFAULT; True / False: on /
        off.  On packs the matrices whose copy is smaller than the matrix (K % 2048 == 0).  "all" is for tests: q/k/v and
        down_proj too (measured slower) and every K % 512 == 0 (a padded copy can be larger than the matrix).  The raw matrices
        stay (prefill, batched rows, lookup steps and exception rows read them), so the copies are additional HBM: 0.8125 of
        the packed matrices' bytes, +7.0 GB for the 8B model (32 gate/up matrices of 190.8 MB and lm_head of 853.7 MB: 16.1 ->
        23.1 GB of weights; pack13_bytes()).  The binding table is global to the process and keyed by the raw matrix's address, so a
        matrix this object binds is always its own: where the state dict's tensor would be used as it is (already on the device in
        the engine dtype), it is cloned first -- otherwise a second engine built from the same tensors would share, replace and
        tear down this one's binding.
        mxfp4_packed ("mxfp4" only; default off): also hold every layer matrix's codes and scale bytes in the packed decode layout
        (ops.pack_mxfp4: MFMA-operand order) and bind the copies (srgpt_mxfp4_bind), so that every decode-shaped step of 2+ rows --
        batches, lookup steps, their graphs -- runs the MFMA product srgpt_gemv_w4p instead of passes of the 4-row VALU kernel.  All
        four matrices of all layers, or none where a shape is outside the layout's domain (K % 128 == 0, inter % 16 == 0):
        `self.mxfp4_packed` reports the outcome.  The row-major codes stay (the one-row kernel and the prefill expansion read them),
        so the copies are additional HBM: 0.53125 bytes per weight, +3.7 GB for the 8B model (mxfp4_packed_bytes()).
        decode_pass_rows (16 or 32; default 16): rows per weight pass of the decode step's MFMA products.  32: a step of 17 - 32 rows
        streams every matrix once instead of twice (srgpt_gemv_rowss_wide / srgpt_gemv_w4p_wide) for the products gemv_route.h's
        gemv_wide_route runs wide; rows 16 and up of a step of 17 - 31 rows then differ in the last bits from the default's (there
        they are a pass of fewer than 9 rows, which sums on two accumulators).  Fixed at construction: captured graphs hold launches.
        mxfp4_prefill_direct ("mxfp4" only; default off): prefill and append prefill call the `_direct` W4 entry points
        (srgpt_llm_weights::mxfp4_direct = 1) -- q/k/v, gate/up and down_proj of a 225 .. 272-row prefill multiply the codes inside the
        whole-M kernel instead of expanding each matrix to bf16 first.  Every byte the prefill writes is the same."""
        if decode_pass_rows not in (16, 32) or isinstance(decode_pass_rows, bool):
            raise ValueError(f"decode_pass_rows must be 16 or 32, got {decode_pass_rows!r}")
        self._decode_pass_rows = int(decode_pass_rows)
        if mxfp4_prefill_direct and llm_weight_format != "mxfp4":  # (under "mxfp4_w4a8" no product expands: it would do nothing)
            raise ValueError(f"mxfp4_prefill_direct needs llm_weight_format='mxfp4', got {llm_weight_format!r}")
        self._mxfp4_prefill_direct = bool(mxfp4_prefill_direct)
        self.cfg, self.device, self.dtype = cfg, torch.device(device), dtype
        # parts: which components to materialise -- all of them for the model, ONE for the module-level factories
        # (spatialrgpt_amd/factories.py: the reference's build_vision_tower / build_mm_projector / build_region_extractor /
        # build_llm_and_tokenizer seams); a missing part's weights are neither read nor required
        self.parts = tuple(self.ALL_PARTS if parts is None else parts)
        for p_ in self.parts:
            if p_ not in self.ALL_PARTS:
                raise ValueError(f"unknown part {p_!r}")
        self.vit = self.llm = None
        self.vocab = 0
        self.rope_len = 0
        if llm_weight_format not in ("native", "fp8", "fp8_w8a8", "mxfp4", "mxfp4_w4a8"):
            raise ValueError(f"unknown llm_weight_format {llm_weight_format!r}")
        # "fp8_w8a8": the same fp8 weights; prefill additionally quantises every GEMM input per token to e4m3 and multiplies on
        # the fp8 matrix pipe (srgpt_gemm_w8a8) -- opt-in, it changes the numbers; decode stays W8A16
        # "mxfp4_w4a8": the same with the MXFP4 weights (srgpt_gemm_w4a8); decode stays W4A16
        self.fp8_act = llm_weight_format in ("fp8_w8a8", "mxfp4_w4a8")
        if self.fp8_act:
            if cfg.hidden % 128 or cfg.inter % 128 or (cfg.heads * cfg.head_dim) % 128:
                raise ValueError(f"{llm_weight_format} needs hidden, inter and heads * head_dim to be multiples of 128")
            llm_weight_format = llm_weight_format.split("_")[0]
        if llm_weight_format == "fp8" and dtype != torch.bfloat16:
            raise ValueError("fp8 LLM weights need a bf16 engine")
        if llm_weight_format == "mxfp4":
            if dtype != torch.bfloat16:
                raise ValueError("mxfp4 LLM weights need a bf16 engine")
            if cfg.hidden % 32 or cfg.inter % 32 or (cfg.heads * cfg.head_dim) % 32:
                raise ValueError("mxfp4 needs hidden, inter and heads * head_dim to be multiples of 32")
        self.llm_weight_format = llm_weight_format
        if decode_layout not in ("packed", "rowmajor"):
            raise ValueError(f"unknown decode_layout {decode_layout!r}")
        self.decode_layout = decode_layout  # fp8 weights: also keep the MFMA-operand-order copies the batched decode step streams
        self._keep: List[object] = []
        if pack13 not in (None, True, False, "all"):
            raise ValueError(f"unknown pack13 {pack13!r}")
        self.pack13_mode = PACK13_DEFAULT if pack13 is None else bool(pack13)
        self.pack13_all = isinstance(pack13, str)  # "all"
        self.mxfp4_packed = False  # set by _prepare_llm: are all MXFP4 layer matrices packed and bound?
        self._mxfp4_want = bool(mxfp4_packed)
        self.p4: Dict[str, list] = {}  # name -> per layer (codes, packed) of a bound MXFP4 matrix
        self._aliased = set()  # data_ptr of every tensor get() handed out without a copy: the caller's own storage
        self.p13: Dict[str, list] = {}  # name -> per layer (raw, packed, flags, exception rows) of a bound matrix, or None
        code = {torch.float32: L.F32, torch.bfloat16: L.BF16}[dtype]

        def get(name):
            t = sd.pop(name) if consume else sd[name]
            out = t.to(device=self.device, dtype=dtype).contiguous()
            if out.data_ptr() == t.data_ptr():
                self._aliased.add(out.data_ptr())
            return out

        if "vit" in self.parts:
            self._prepare_vit(cfg, get, code)
        if "region" in self.parts and cfg.enable_region:
            self._prepare_region(cfg, get)
        if "projector" in self.parts:
            # ---------------- projector (mlp_downsample) ----------------
            self.mp_ln_w, self.mp_ln_b = get(MP + "1.weight"), get(MP + "1.bias")
            self.mp_w1, self.mp_b1 = get(MP + "2.weight"), get(MP + "2.bias")
            self.mp_w2, self.mp_b2 = get(MP + "4.weight"), get(MP + "4.bias")
        if "llm" in self.parts:
            self._prepare_llm(cfg, get, code, llm_weight_format, rope_positions)

    def _prepare_vit(self, cfg, get, code):
        dtype = self.dtype
        # ---------------- vision tower ----------------
        C_, p = cfg.vit_hidden, cfg.patch_size
        kk = 3 * p * p
        self.kp = (kk + 7) // 8 * 8
        pw = get(VT + "embeddings.patch_embedding.weight").reshape(C_, kk)
        patch_w = torch.zeros((C_, self.kp), device=self.device, dtype=dtype)
        patch_w[:, :kk] = pw
        self.patch_w = patch_w
        clip = cfg.tower == "clip"
        self.patch_b = None if clip else get(VT + "embeddings.patch_embedding.bias")
        self.pos_emb = get(VT + "embeddings.position_embedding.weight")
        if self.pos_emb.shape[0] != cfg.tower_tokens:
            raise ValueError(f"position embedding has {self.pos_emb.shape[0]} rows, tower expects {cfg.tower_tokens}")
        self.cls_emb = get(VT + "embeddings.class_embedding").reshape(-1) if clip else None
        self.pre_ln_w = get(VT + "pre_layrnorm.weight") if clip else None
        self.pre_ln_b = get(VT + "pre_layrnorm.bias") if clip else None
        n_run = cfg.vit_layers_run
        self.inter_pad = (cfg.vit_inter + 63) // 64 * 64
        v = {k: [] for k in ("ln1_w", "ln1_b", "wqkv", "bqkv", "wo", "bo", "ln2_w", "ln2_b", "w1", "b1", "w2", "b2")}
        for i in range(n_run):
            q = f"{VT}encoder.layers.{i}."
            v["ln1_w"].append(get(q + "layer_norm1.weight"))
            v["ln1_b"].append(get(q + "layer_norm1.bias"))
            v["wqkv"].append(torch.cat([get(q + f"self_attn.{n}_proj.weight") for n in "qkv"], 0).contiguous())
            v["bqkv"].append(torch.cat([get(q + f"self_attn.{n}_proj.bias") for n in "qkv"], 0).contiguous())
            v["wo"].append(get(q + "self_attn.out_proj.weight"))
            v["bo"].append(get(q + "self_attn.out_proj.bias"))
            v["ln2_w"].append(get(q + "layer_norm2.weight"))
            v["ln2_b"].append(get(q + "layer_norm2.bias"))
            v["w1"].append(get(q + "mlp.fc1.weight"))
            v["b1"].append(get(q + "mlp.fc1.bias"))
            w2 = get(q + "mlp.fc2.weight")  # [hidden, inter] -> [hidden, inter_pad], zero columns (fc2's K tiles exactly by 64)
            if self.inter_pad != cfg.vit_inter:
                w2p = torch.zeros((C_, self.inter_pad), device=self.device, dtype=dtype)
                w2p[:, :cfg.vit_inter] = w2
                w2 = w2p
            v["w2"].append(w2)
            v["b2"].append(get(q + "mlp.fc2.bias"))
        self.vit_t = v
        vw = L.VitWeights()
        vw.dtype, vw.hidden, vw.inter, vw.heads = code, C_, cfg.vit_inter, cfg.vit_heads
        vw.n_layers_run, vw.image_size, vw.patch, vw.kp, vw.eps = n_run, cfg.image_size, p, self.kp, cfg.vit_eps
        vw.inter_pad = self.inter_pad
        vw.act = L.ACT_QUICK_GELU if clip else L.ACT_GELU_TANH
        vw.patch_w, vw.pos_emb = self.patch_w.data_ptr(), self.pos_emb.data_ptr()
        vw.patch_b = None if self.patch_b is None else self.patch_b.data_ptr()
        vw.cls_emb = None if self.cls_emb is None else self.cls_emb.data_ptr()
        vw.pre_ln_w = None if self.pre_ln_w is None else self.pre_ln_w.data_ptr()
        vw.pre_ln_b = None if self.pre_ln_b is None else self.pre_ln_b.data_ptr()
        for k, ts in v.items():
            arr = _ptr_array(ts)
            self._keep.append(arr)
            setattr(vw, k, arr)
        self.vit = vw

    def _prepare_region(self, cfg, get):
        # ---------------- region extractor ----------------
        fr = RE + "feature_refinement_module."

        def deconv_w(name):
            w = get(name)  # [Cin, Cout, 2, 2]
            cin, cout = w.shape[0], w.shape[1]
            return w.permute(2, 3, 1, 0).reshape(4 * cout, cin).contiguous()

        self.dc1_w, self.dc1_b = deconv_w(fr + "0.weight"), get(fr + "0.bias")
        self.ln2d_w, self.ln2d_b = get(fr + "1.weight"), get(fr + "1.bias")
        self.dc2_w, self.dc2_b = deconv_w(fr + "3.weight"), get(fr + "3.bias")
        self.rgb_w, self.rgb_b = get(RE + "rgb_projector.weight"), get(RE + "rgb_projector.bias")
        self.depth_w, self.depth_b = get(RE + "depth_projector.weight"), get(RE + "depth_projector.bias")

    def _prepare_llm(self, cfg, get, code, llm_weight_format, rope_positions):
        dtype = self.dtype
        # ---------------- language model ----------------
        self.embed = get(LM + "model.embed_tokens.weight")
        self.final_norm = get(LM + "model.norm.weight")
        self.lm_head = get(LM + "lm_head.weight")
        lt = {k: [] for k in ("attn_norm", "wqkv", "wo", "mlp_norm", "wgu", "wdown")}
        for i in range(cfg.layers):
            q = f"{LM}model.layers.{i}."
            lt["attn_norm"].append(get(q + "input_layernorm.weight"))
            lt["wqkv"].append(torch.cat([get(q + f"self_attn.{n}_proj.weight") for n in "qkv"], 0).contiguous())
            lt["wo"].append(get(q + "self_attn.o_proj.weight"))
            lt["mlp_norm"].append(get(q + "post_attention_layernorm.weight"))
            lt["wgu"].append(torch.cat([get(q + "mlp.gate_proj.weight"), get(q + "mlp.up_proj.weight")], 0).contiguous())
            lt["wdown"].append(get(q + "mlp.down_proj.weight"))
        self.llm_t = lt
        self.llm_q = None   # fp8: name -> (codes per layer, row scales per layer); {} under "mxfp4" (lm_head alone is fp8)
        self.llm_q4 = None  # mxfp4: name -> (codes per layer, E8M0 block scales per layer)
        if llm_weight_format == "mxfp4":
            from . import ops  # local import: ops needs the loaded library

            q4 = {k: ([], []) for k in ("wqkv", "wo", "wgu", "wdown")}
            for k in q4:
                for i in range(cfg.layers):
                    codes, scales, _ = ops.quantize_mxfp4_rows(lt[k][i])
                    lt[k][i] = None  # the bf16 matrix is dropped: nothing reads it
                    q4[k][0].append(codes)
                    q4[k][1].append(scales)
            self.lm_head8, self.lm_head_scale, _ = ops.quantize_fp8_rows(self.lm_head)
            self.lm_head = None
            self.llm_q4, self.llm_q = q4, {}
            self.llm_pk, self.pk_rows = {}, {}
            if self._mxfp4_want:
                self._mxfp4_pack_bind()
        if llm_weight_format == "fp8":
            from . import ops  # local import: ops needs the loaded library

            qd = {k: ([], []) for k in ("wqkv", "wo", "wgu", "wdown")}
            for k in qd:
                for i in range(cfg.layers):
                    q8, sc, _ = ops.quantize_fp8_rows(lt[k][i])
                    lt[k][i] = None  # the bf16 matrix is dropped: nothing reads it
                    qd[k][0].append(q8)
                    qd[k][1].append(sc)
            self.lm_head8, self.lm_head_scale, _ = ops.quantize_fp8_rows(self.lm_head)
            self.lm_head = None
            self.llm_q = qd
            # Packed copies for the batched decode step (2+ sequences per GPU; srgpt_pack_decode_weights, include/srgpt.h ABI 9): the
            # same fp8 bytes in MFMA-operand order.  The row-major copies stay: prefill (srgpt_gemm_w8 / _w8a8) and the one-row
            # decode kernel read those -- +6.5 GB of the 288 for an 8B model.  Granule rows per matrix from the measured table
            # (profiles/r06_skinny_packed_gr.txt): 16 (1 KiB per instruction) where a CU owns a single 16-column tile, else 4.
            # (Load-time layout; what the kernel then does with a granule -- column width in whole granules, gr_shift -- is
            # gemv_skinny_launch of csrc/gemv_route.h.)
            self.llm_pk, self.pk_rows = {}, {}
            if self.decode_layout == "packed":
                n_cu = int(L.load().srgpt_device_cus())
                for k in qd:
                    rows_total, K = qd[k][0][0].shape
                    n_out = rows_total // 2 if k == "wgu" else rows_total
                    rows = 16 if (n_out + n_cu - 1) // n_cu <= 16 else 4
                    if K % 64 or n_out % rows:
                        continue  # (tiny test geometries: this product streams the row-major copy)
                    self.llm_pk[k] = [ops.pack_decode_weights(q8, rows) for q8 in qd[k][0]]
                    self.pk_rows[k] = rows
        n_pos = rope_positions or cfg.max_position_embeddings
        self.rope_len = n_pos
        self.rope_cos, self.rope_sin = rope_tables(cfg, n_pos, dtype, self.device)
        lw = L.LlmWeights()
        lw.dtype, lw.hidden, lw.inter, lw.layers = code, cfg.hidden, cfg.inter, cfg.layers
        lw.heads, lw.kv_heads, lw.head_dim, lw.vocab, lw.rms_eps = cfg.heads, cfg.kv_heads, cfg.head_dim, self.embed.shape[0], cfg.rms_eps
        lw.rope_cos, lw.rope_sin = self.rope_cos.data_ptr(), self.rope_sin.data_ptr()
        lw.embed, lw.final_norm = self.embed.data_ptr(), self.final_norm.data_ptr()
        lw.lm_head = None if self.lm_head is None else self.lm_head.data_ptr()
        for k, ts in lt.items():
            arr = _ptr_array(ts)
            self._keep.append(arr)
            setattr(lw, k, arr)
        if self.llm_q is not None:
            lw.lm_head8, lw.lm_head_scale = self.lm_head8.data_ptr(), self.lm_head_scale.data_ptr()
            for k, (qs, scs) in self.llm_q.items():
                a8, asc = _ptr_array(qs), _ptr_array(scs)
                self._keep += [a8, asc]
                setattr(lw, k + "8", a8)
                setattr(lw, k + "_scale", asc)
            for k, field in (("wqkv", "pk_rows_qkv"), ("wo", "pk_rows_o"), ("wgu", "pk_rows_gu"), ("wdown", "pk_rows_down")):
                if k in self.llm_pk:
                    ap = _ptr_array(self.llm_pk[k])
                    self._keep.append(ap)
                    setattr(lw, k + "8p", ap)
                    setattr(lw, field, self.pk_rows[k])
        if self.llm_q4 is not None:
            for k, (cs, scs) in self.llm_q4.items():
                a4, asc = _ptr_array(cs), _ptr_array(scs)
                self._keep += [a4, asc]
                setattr(lw, k + "4", a4)
                setattr(lw, k + "4_scale", asc)
        lw.fp8_act = 1 if self.fp8_act else 0
        lw.decode_pass_rows = self._decode_pass_rows
        lw.mxfp4_direct = 1 if self._mxfp4_prefill_direct else 0
        self.llm = lw
        self.vocab = self.embed.shape[0]
        if self.pack13_mode and llm_weight_format == "native" and dtype == torch.bfloat16:
            for k in ("wqkv", "wgu", "wdown", "lm_head") if self.pack13_all else PACK13_PRODUCTS:
                ts = [self.lm_head] if k == "lm_head" else lt[k]
                for i, t in enumerate(ts):
                    if self._pack13_wanted(t) and t.data_ptr() in self._aliased:  # the caller's tensor: bind a matrix of our own
                        ts[i] = t.clone()
                        if k == "lm_head":
                            self.lm_head, lw.lm_head = ts[i], ts[i].data_ptr()
                        else:
                            getattr(lw, k)[i] = ts[i].data_ptr()
                self.p13[k] = [self._pack13_bind(t) for t in ts]

    # ---- the 13-bit packed copies: packed, bound and unbound HERE and nowhere else (a stale binding is a silent wrong answer: the
    # step would stream the copy of a matrix that is gone) ----
    def _pack13_wanted(self, raw) -> bool:
        from . import ops  # local import: ops needs the loaded library

        return ops.pack13_eligible(raw) and (self.pack13_all or raw.shape[1] % 2048 == 0)

    def _pack13_bind(self, raw):
        from . import ops

        if not self._pack13_wanted(raw):
            return None
        if ops.pack13_bound(raw):
            # somebody else's binding (a C caller's, or another object's on storage we share after all): theirs to unbind, and
            # replacing it would leave them streaming a copy we free -- this matrix runs the raw kernel here
            return None
        packed, flags, n_exc = ops.pack13(raw)
        ops.pack13_bind(raw, packed, flags)
        return (raw, packed, flags, n_exc)

    def pack13_unbind(self, names=None) -> None:
        """drop the bindings (and the copies) of the named products, default all: before a raw matrix is replaced, and at teardown"""
        from . import ops

        for k in list(self.p13) if names is None else names:
            for ent in self.p13.pop(k, []):
                if ent is not None:
                    ops.pack13_unbind(ent[0])

    # ---- the packed MXFP4 copies: packed, bound and unbound here and nowhere else, like the 13-bit copies ----
    def _mxfp4_pack_bind(self) -> None:
        from . import ops

        shapes = {k: (cs[0].shape[0] // 2 if k == "wgu" else cs[0].shape[0], cs[0].shape[1] * 2, k == "wgu")
                  for k, (cs, _) in self.llm_q4.items() if cs}
        if not shapes or any(ops.mxfp4_packed_bytes(n, K, sw) == 0 for n, K, sw in shapes.values()):
            return  # all or nothing: the step takes the MFMA product only with every matrix bound
        if any(ops.mxfp4_bound(c) for cs, _ in self.llm_q4.values() for c in cs):
            return  # somebody else's binding on storage we share: theirs to unbind (see _pack13_bind)
        for k, (cs, scs) in self.llm_q4.items():
            ents = []
            for c, sc in zip(cs, scs):
                packed = ops.pack_mxfp4(c, sc, swiglu=shapes[k][2])
                ops.mxfp4_bind(c, packed, swiglu=shapes[k][2])
                ents.append((c, packed))
            self.p4[k] = ents
        self.mxfp4_packed = True

    def mxfp4_unbind(self) -> None:
        """drop the bindings (and the packed copies) of the MXFP4 matrices: every step is again the unbound engine's"""
        from . import ops

        for k in list(self.p4):
            for c, _ in self.p4.pop(k):
                ops.mxfp4_unbind(c)
        self.mxfp4_packed = False

    def mxfp4_packed_bytes(self) -> int:
        """HBM the packed MXFP4 copies take, on top of the row-major codes and scales"""
        return sum(packed.numel() for ents in self.p4.values() for _, packed in ents)

    @property
    def decode_pass_rows(self) -> int:
        return self._decode_pass_rows

    @property
    def mxfp4_prefill_direct(self) -> bool:
        return self._mxfp4_prefill_direct

    def pack13_bytes(self) -> int:
        """HBM the packed copies and their flags take, on top of the raw matrices"""
        return sum(ent[1].numel() + 4 * ent[2].numel() for ents in self.p13.values() for ent in ents if ent is not None)

    def pack13_exception_rows(self) -> int:
        return sum(ent[3] for ents in self.p13.values() for ent in ents if ent is not None)

    def __del__(self):
        try:
            self.pack13_unbind()
        except Exception:
            pass
        try:
            self.mxfp4_unbind()
        except Exception:
            pass

    def resize_vocab(self, n: int) -> None:
        """HF `resize_token_embeddings` on the live weights (the reference's loader calls it after adding `<mask>` / `<depth>`,
        builder.py:186-199 -> PreTrainedModel._get_resized_embeddings / _get_resized_lm_head): embed_tokens and lm_head grow or shrink to
        `n` rows, the common rows are kept, new rows = the mean of the old rows -- what spatialrgpt_amd.builder gives the rows it adds
        at load (transformers' mean-resizing; 4.37.2 drew them N(0, initializer_range): untrained rows either way).
        fp8 lm_head: the new rows are quantised with the loader's rule and appended."""
        old = self.embed.shape[0]
        if n == old:
            return
        if n <= 0:
            raise ValueError(f"resize_token_embeddings({n})")
        keep = min(old, n)

        def resized(t):
            out = torch.empty((n, t.shape[1]), device=t.device, dtype=t.dtype)
            out[:keep] = t[:keep]
            if n > keep:
                out[keep:] = t.float().mean(0, keepdim=True).to(t.dtype)
            return out

        self.embed = resized(self.embed)
        lw = self.llm
        if self.llm_q is None:
            repack = "lm_head" in self.p13
            self.pack13_unbind(["lm_head"])  # before the raw matrix goes
            self.lm_head = resized(self.lm_head)
            lw.lm_head = self.lm_head.data_ptr()
            if repack:
                self.p13["lm_head"] = [self._pack13_bind(self.lm_head)]
        else:
            from . import ops
            q8, sc = self.lm_head8[:keep], self.lm_head_scale[:keep]
            if n > keep:
                fresh = self.dequantised("lm_head").float().mean(0, keepdim=True).to(self.dtype).expand(n - keep, -1).contiguous()
                nq, nsc, _ = ops.quantize_fp8_rows(fresh)
                q8, sc = torch.cat([q8, nq], 0), torch.cat([sc, nsc], 0)
            self.lm_head8, self.lm_head_scale = q8.contiguous(), sc.contiguous()
            lw.lm_head8, lw.lm_head_scale = self.lm_head8.data_ptr(), self.lm_head_scale.data_ptr()
        lw.embed, lw.vocab = self.embed.data_ptr(), n
        self.vocab = n

    def dequantised(self, name: str, layer: int = 0) -> torch.Tensor:
        """bf16 values of an fp8- or mxfp4-held matrix ("wqkv" | "wo" | "wgu" | "wdown" | "lm_head"): code * scale, exact in bf16."""
        if self.llm_q is None:
            raise ValueError("weights are not fp8 or mxfp4")
        if self.llm_q4 is not None and name != "lm_head":
            from . import ops
            return ops.dequant_mxfp4(self.llm_q4[name][0][layer], self.llm_q4[name][1][layer])
        q8, sc = (self.lm_head8, self.lm_head_scale) if name == "lm_head" else (self.llm_q[name][0][layer], self.llm_q[name][1][layer])
        return (q8.view(torch.float8_e4m3fn).float() * sc[:, None]).to(self.dtype)

    def llm_weight_bytes(self) -> int:
        """bytes streamed from HBM per decoded token AT BATCH 1 (everything but embed_tokens): of a matrix with a bound 13-bit copy,
        the copy and its flags (exception rows, read from the raw matrix besides, are not counted).  Steps of 2+ rows, lookup steps
        and the prefill read the raw matrices whatever is bound: for them the figure is low by pack13_bytes() * 3 / 13."""
        es = self.embed.element_size()
        if self.llm_q is None:
            n = self.final_norm.numel() + self.lm_head.numel()
            for ts in self.llm_t.values():
                n += sum(t.numel() for t in ts)
            n *= es
            for ents in self.p13.values():
                for ent in ents:
                    if ent is not None:
                        n += ent[1].numel() + 4 * (ent[2].numel() - 1) - ent[0].numel() * es
            return n
        n = (self.final_norm.numel() + sum(t.numel() for k in ("attn_norm", "mlp_norm") for t in self.llm_t[k])) * es
        n += self.lm_head8.numel() + 4 * self.lm_head_scale.numel()
        for qs, scs in self.llm_q.values():
            n += sum(t.numel() for t in qs) + 4 * sum(t.numel() for t in scs)
        for cs, scs in (self.llm_q4 or {}).values():
            n += sum(t.numel() for t in cs) + sum(t.numel() for t in scs)
        return n


def weight_shapes(cfg: SrgptConfig) -> Dict[str, tuple]:
    C_, I, H, F_, V, d = cfg.vit_hidden, cfg.vit_inter, cfg.hidden, cfg.inter, cfg.vocab, cfg.head_dim
    s: Dict[str, tuple] = {}
    s[VT + "embeddings.patch_embedding.weight"] = (C_, 3, cfg.patch_size, cfg.patch_size)
    if cfg.tower == "clip":
        s[VT + "embeddings.class_embedding"] = (C_,)
        s[VT + "pre_layrnorm.weight"] = (C_,)
        s[VT + "pre_layrnorm.bias"] = (C_,)
    else:
        s[VT + "embeddings.patch_embedding.bias"] = (C_,)
    s[VT + "embeddings.position_embedding.weight"] = (cfg.tower_tokens, C_)
    for i in range(cfg.vit_layers_run):  # layers past select_layer never influence the output
        p = f"{VT}encoder.layers.{i}."
        for n in ("layer_norm1", "layer_norm2"):
            s[p + n + ".weight"] = (C_,)
            s[p + n + ".bias"] = (C_,)
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            s[p + f"self_attn.{n}.weight"] = (C_, C_)
            s[p + f"self_attn.{n}.bias"] = (C_,)
        s[p + "mlp.fc1.weight"] = (I, C_)
        s[p + "mlp.fc1.bias"] = (I,)
        s[p + "mlp.fc2.weight"] = (C_, I)
        s[p + "mlp.fc2.bias"] = (C_,)
    p = RE + "feature_refinement_module."
    s[p + "0.weight"] = (C_, C_, 2, 2)
    s[p + "0.bias"] = (C_,)
    s[p + "1.weight"] = (C_,)
    s[p + "1.bias"] = (C_,)
    s[p + "3.weight"] = (C_, C_, 2, 2)
    s[p + "3.bias"] = (C_,)
    for n in ("rgb_projector", "depth_projector"):
        s[RE + n + ".weight"] = (H, C_)
        s[RE + n + ".bias"] = (H,)
    s[MP + "1.weight"] = (4 * C_,)
    s[MP + "1.bias"] = (4 * C_,)
    s[MP + "2.weight"] = (H, 4 * C_)
    s[MP + "2.bias"] = (H,)
    s[MP + "4.weight"] = (H, H)
    s[MP + "4.bias"] = (H,)
    s[LM + "model.embed_tokens.weight"] = (V, H)
    for i in range(cfg.layers):
        p = f"{LM}model.layers.{i}."
        s[p + "input_layernorm.weight"] = (H,)
        s[p + "post_attention_layernorm.weight"] = (H,)
        s[p + "self_attn.q_proj.weight"] = (cfg.heads * d, H)
        s[p + "self_attn.k_proj.weight"] = (cfg.kv_heads * d, H)
        s[p + "self_attn.v_proj.weight"] = (cfg.kv_heads * d, H)
        s[p + "self_attn.o_proj.weight"] = (H, cfg.heads * d)
        s[p + "mlp.gate_proj.weight"] = (F_, H)
        s[p + "mlp.up_proj.weight"] = (F_, H)
        s[p + "mlp.down_proj.weight"] = (H, F_)
    s[LM + "model.norm.weight"] = (H,)
    s[LM + "lm_head.weight"] = (V, H)
    return s


def synth_state_dict(cfg: SrgptConfig, seed: int, dtype, device, std: float = 0.02) -> Dict[str, torch.Tensor]:
    """Seeded random weights of the named architecture, generated on `device` (no checkpoints exist offline).
    Matrices/biases ~ N(0, std), norm gains 1 + N(0, std), embeddings ~ N(0, 0.5)."""
    g = torch.Generator(device=device).manual_seed(seed)
    sd = {}
    for name, shape in weight_shapes(cfg).items():
        t = torch.randn(shape, generator=g, device=device, dtype=torch.float32)
        is_gain = name.endswith(("norm.weight", "layernorm.weight", "layrnorm.weight", "layer_norm1.weight", "layer_norm2.weight")) or \
            name in (RE + "feature_refinement_module.1.weight", MP + "1.weight")
        if "position_embedding" in name or "embed_tokens" in name or "class_embedding" in name:
            t = t * 0.5
        elif is_gain:
            t = 1.0 + t * std
        else:
            t = t * std
        sd[name] = t.to(dtype)
    return sd
