"""CPU restatement of the device logits processors (csrc/logits_proc.hip) and the HF processor list they stand for.

`process_ref` states what srgpt_logits_process computes -- including what HF's classes do not define (history ids outside the
vocabulary are skipped) -- in a few lines of torch; tests/test_logits_proc_abi.py pins it to the installed transformers'
RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor and MinLength / MinNewTokensLength processors, and
tests/test_gpu_logits_proc.py compares the kernel with it bit for bit."""
import torch

NEG = float("-inf")


def process_ref(scores, ids, n, repetition_penalty=1.0, no_repeat_ngram=0, min_new_tokens=0, eos=()):
    """scores fp32 [B, V] (CPU), ids int64 [B, ld]: the first n ids of a row are its history.  Returns the processed copy."""
    scores = scores.detach().cpu()
    out = scores.clone()
    B, V = scores.shape
    g = int(no_repeat_ngram)
    for b in range(B):
        h = [int(t) for t in ids[b, :n]]
        if repetition_penalty != 1.0:
            seen = torch.tensor(sorted({t for t in h if 0 <= t < V}), dtype=torch.int64)
            s = scores[b, seen]  # the ORIGINAL scores: an id that occurs twice is penalised once
            out[b, seen] = torch.where(s < 0, s * repetition_penalty, s / repetition_penalty)
        if g > 0 and n + 1 >= g:
            tail = h[n - (g - 1):]
            for i in range(n - g + 1):
                t = h[i + g - 1]
                if h[i:i + g - 1] == tail and 0 <= t < V:
                    out[b, t] = NEG
        if n < min_new_tokens:
            for e in eos:
                if 0 <= int(e) < V:
                    out[b, int(e)] = NEG
    return out


def hf_processors(repetition_penalty=1.0, no_repeat_ngram=0, min_new_tokens=0, eos=()):
    """the list HF's `_get_logits_processor` builds for these settings when generate() is fed `inputs_embeds` (input_ids start
    empty: the prompt length to skip is 0), in its order"""
    from transformers import (MinNewTokensLengthLogitsProcessor, NoRepeatNGramLogitsProcessor,
                              RepetitionPenaltyLogitsProcessor)

    procs = []
    if repetition_penalty != 1.0:
        procs.append(RepetitionPenaltyLogitsProcessor(penalty=float(repetition_penalty)))
    if no_repeat_ngram > 0:
        procs.append(NoRepeatNGramLogitsProcessor(int(no_repeat_ngram)))
    if min_new_tokens > 0 and len(eos) > 0:
        procs.append(MinNewTokensLengthLogitsProcessor(0, int(min_new_tokens), [int(e) for e in eos]))
    return procs


def hf_process(procs, input_ids, scores):
    """scores fp32 [B, V] (CPU) through the HF processors over input_ids int64 [B, n] (n may be 0)"""
    scores = scores.detach().cpu().clone()
    input_ids = input_ids.detach().cpu()
    for p in procs:
        scores = p(input_ids, scores)
    return scores
