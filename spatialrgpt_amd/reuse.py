"""Prefix reuse across requests: an UNCHANGED caller that re-sends the whole conversation every turn -- the demo,
eval_spatial.py -- continues the last request's live KV cache instead of paying for the towers and the full prefill again.

What is kept of the last request (`ReuseRecord`): the engine-dtype media the tower and the pooling read, the tower's products
(`hres`, `depth_features`, `image_features`), the splice table of its prompt, and its own DecodeState.  A new request is compared
with it ON THE DEVICE, bytes and row descriptors, never hashes (csrc/reuse.hip): a miss costs a full request, a false hit would be a
wrong answer.  `plan_reuse` is the decision, a pure function; `PrefixReuse` runs the sequence for `LlavaLlamaModel.generate`."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import _lib as L_
from . import ops


def plan_reuse(matched_rows: int, live_len: int, len_new: int, cap: int, max_new: int, state_max_new: int) -> Tuple[str, int]:
    """-> (mode, L).  L = the rows of the retained state the new prompt keeps: what matched, what is live in the cache, and at most
    len_new - 1 -- at least one row is always appended, so that there are logits to pick from (the same prompt asked twice).
    "append": truncate the state to L rows and append the prompt's rows from L on.  "fresh": nothing matched, or the prompt and its
    max_new tokens do not fit the state's `cap` positions, or the state was built for fewer new tokens -- not an error: the request
    builds a state that fits and that one is retained."""
    L = max(min(int(matched_rows), int(live_len), int(len_new) - 1), 0)
    if L == 0 or L + (len_new - L) + max_new > cap or max_new > state_max_new:
        return "fresh", L
    return "append", L


@dataclass
class ReuseRecord:
    """the last request, as the next one is compared with it"""
    images: torch.Tensor                  # [n, 3, S, S] engine dtype, exactly what the tower read (a copy the caller cannot reach)
    depths: Optional[torch.Tensor]
    masks: Optional[list]                 # per image: the mask tensor the pooling read, or None
    hres: Optional[torch.Tensor]
    depth_features: Optional[torch.Tensor]
    image_features: torch.Tensor
    desc: torch.Tensor                    # [n_rows, 2] int32: the prompt's rows of srgpt_splice_plan
    n_rows: int
    region_counts: Optional[list]
    state: object                         # the request's own DecodeState (new_state with cache_reserve; never the pooled one)
    n_gen: int                            # ids the request kept: state.out_ids[0, :n_gen]
    live_len: int                         # cached rows behind it: n_rows + n_gen - 1 (the last id is pending)

    def nbytes(self) -> int:
        ts = [self.images, self.depths, self.hres, self.depth_features, self.image_features, self.desc, self.state.kcache,
              self.state.vcache, self.state.ws, self.state.logits] + [m for m in (self.masks or []) if m is not None]
        return sum(t.numel() * t.element_size() for t in ts if t is not None)


def _own(t: torch.Tensor, src: torch.Tensor) -> torch.Tensor:
    """`t` (what .to() gave for `src`) as memory the caller cannot write to afterwards"""
    return t.clone() if t.data_ptr() == src.data_ptr() else t


class PrefixReuse:
    """the reuse path of LlavaLlamaModel.generate (batch 1, no beams): `prefill` leaves the request's prompt in a state and returns
    it, the model's decode loop runs on it unchanged, `commit` retains the request."""

    def __init__(self, model):
        self.model = model
        self.record: Optional[ReuseRecord] = None
        self.last: Optional[dict] = None
        self._pending = None

    def drop(self):
        self.record, self._pending = None, None

    # ------------------------------------------------------------------ media, as encode_visual flattens and casts them
    def _media(self, images, depths, masks):
        eng = self.model.engine
        cfg = eng.cfg

        def flat(x):
            if isinstance(x, (list, tuple)):
                x = torch.cat(list(x), dim=0)
            elif x.ndim == 5:
                x = x.flatten(0, 1)
            return x.to(device=eng.device, dtype=eng.dtype).contiguous()

        im = flat(images)
        use_depth = cfg.enable_region and cfg.enable_depth and depths is not None
        dp = flat(depths) if use_depth else None
        ms = None
        if masks is not None and cfg.enable_region:
            ms = [None if m is None else m.to(eng.device).contiguous() for m in masks]
        return im, dp, ms

    def _compare_media(self, rec: ReuseRecord, im, dp, ms, out: torch.Tensor) -> Optional[int]:
        """enqueue the byte compares into out[0] (images), out[1] (depths), out[2] (masks of the first image); -> the mask rows
        compared (what out[2] can reach), or None: the media differ by shape already -- nothing was enqueued"""
        if im.shape != rec.images.shape or (dp is None) != (rec.depths is None) or (dp is not None and dp.shape != rec.depths.shape):
            return None
        ops.rows_match(im.reshape(1, -1), rec.images.reshape(1, -1), 1, out[0:1])
        if dp is not None:
            ops.rows_match(dp.reshape(1, -1), rec.depths.reshape(1, -1), 1, out[1:2])
        new0 = ms[0] if ms else None
        old0 = rec.masks[0] if rec.masks else None
        n = 0
        if new0 is not None and old0 is not None and new0.dtype == old0.dtype and new0.shape[1:] == old0.shape[1:]:
            n = min(int(new0.shape[0]), int(old0.shape[0]))
        if n > 0:
            ops.rows_match(new0, old0, n, out[2:3])
        return n

    # ------------------------------------------------------------------ the request's prompt into a state
    def prefill(self, input_ids, images, depths, masks, attention_mask, max_new: int):
        """steps 1-6 of the reuse path; -> the DecodeState holding the prompt, its last row's logits in st.logits"""
        m, eng = self.model, self.model.engine
        cfg, dev = eng.cfg, eng.device
        rec = self.record
        if rec is not None and (rec.state.pending is None or rec.state.host_len[0] != rec.live_len):
            rec = self.record = None  # somebody continued the retained state by hand: it no longer is what the record says
        self._pending = None
        im, dp, ms = self._media(images, depths, masks)
        n_images = int(im.shape[0])
        counts = eng._region_counts(masks, n_images)
        # 1. media compare, enqueued in front of the splice plan: its results ride on the plan's own read-back (stats_buf)
        buf = torch.empty((L_.SPLICE_STATS + 4,), device=dev, dtype=torch.int32)
        tail = buf[L_.SPLICE_STATS:]
        mask_rows = self._compare_media(rec, im, dp, ms, tail) if rec is not None else None
        # 3. the plan on the new ids, unchanged
        plan = eng.splice_plan(input_ids, attention_mask, n_images, counts, dp is not None, stats_buf=buf)
        len_new = plan.lens[0]
        # 2. media outcomes
        same_media = False
        regions_common = 0
        if mask_rows is not None:
            t = plan.stats_tail
            same_media = t[0] == 1 and (dp is None or t[1] == 1)
            regions_common = t[2] if (same_media and mask_rows > 0) else 0
        mode, L = "fresh", 0
        st = None
        if same_media and plan.nimg_feat == rec.image_features.shape[1] and plan.n_images == rec.image_features.shape[0]:
            # 4. match: the one additional device -> host copy of the request (4 bytes)
            st = rec.state
            res = torch.empty((1,), device=dev, dtype=torch.int32)
            ops.splice_match(plan.desc[0], len_new, rec.desc, rec.n_rows, st.out_ids[0], rec.n_gen, regions_common, res)
            matched = int(res.cpu()[0])
            # 5. decide
            mode, L = plan_reuse(matched, rec.live_len, len_new, min(st.max_pos, eng.w.rope_len), max_new, st.max_new)
        stages = m.reuse_stages
        if mode == "append":
            # 6. the towers, the refinement and the projector do not run: region embeddings of ALL the request's masks from the
            # retained features (the same call at the same M as a fresh request), one gather, then the rows from L on are appended
            hres, dfeat, imf = rec.hres, rec.depth_features, rec.image_features
            mask_embeds = depth_embeds = None
            if cfg.enable_region:
                mask_embeds, depth_embeds = eng.region_extractor(hres, dfeat, ms)
            emb = eng.splice_apply(plan, imf, mask_embeds, depth_embeds)[0]
            st.truncate(L)  # drops the pending token: the new prompt carries it
            eng.append(st, emb[:, L:])
            im, dp = rec.images, rec.depths  # equal bytes: keep the copies already owned
        else:
            L = 0
            got = {}
            imf, mask_embeds, depth_embeds = eng.encode_visual(im, dp, ms, got)
            if imf.shape[1] != plan.nimg_feat or imf.shape[0] != plan.n_images:  # a geometry the config did not predict
                plan = eng.splice_plan(input_ids, attention_mask, imf.shape[0], counts, dp is not None, nimg_feat=imf.shape[1])
                len_new = plan.lens[0]
            emb = eng.splice_apply(plan, imf, mask_embeds, depth_embeds)[0]
            hres, dfeat = got.get("hres"), got.get("depth_features")
            # a state of the request's own, as _state_for_generate makes one: never the pooled state
            need = len_new + max_new
            if need > eng.w.rope_len:
                raise ValueError(f"sequence of {need} positions exceeds the RoPE table ({eng.w.rope_len})")
            st = eng.new_state(1, min(need + m.cache_reserve, eng.w.rope_len), max(max_new, m.cache_reserve), ws_tokens=len_new)
            eng.prefill(emb, max_new=max_new, state=st)
            im = _own(im, images) if isinstance(images, torch.Tensor) else im
            dp = dp if dp is None or not isinstance(depths, torch.Tensor) else _own(dp, depths)
        if ms is not None:
            ms = [None if t is None else (_own(t, s) if isinstance(s, torch.Tensor) else t) for t, s in zip(ms, masks)]
        if stages is not None:
            stages.update(inputs_embeds=emb, mask_embeds=mask_embeds, depth_embeds=depth_embeds, image_features=imf)
        self.last = dict(mode=mode, rows_reused=L, rows_appended=len_new - L, towers_skipped=mode == "append",
                         regions_common=regions_common)
        self._pending = ReuseRecord(images=im, depths=dp, masks=ms, hres=hres, depth_features=dfeat, image_features=imf,
                                    desc=plan.desc[0, :len_new].clone(), n_rows=len_new, region_counts=counts, state=st, n_gen=0,
                                    live_len=0)
        self.record = None  # the state is being written: the record returns with commit()
        return st

    def commit(self):
        """7. after the decode loop: the request just served is the one the next request is compared with"""
        rec, self._pending = self._pending, None
        st = rec.state
        rec.n_gen = int(st.pending[1][0]) if st.pending is not None else 0
        rec.live_len = int(st.host_len[0])
        self.record = rec if rec.n_gen > 0 else None

