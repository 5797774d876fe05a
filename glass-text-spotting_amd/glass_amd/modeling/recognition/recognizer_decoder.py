"""Attention decoder (`ASTER_V2` -> `AttentionRecognitionHead.sample`) behind ONE ABI call: glass_attention_decode_persistent (ONE
launch for all steps: GRU rows and sEmbed resident in registers, h / context handed between the 16 workgroups of a 16-RoI group
inside the launch) or, with Routing.rnn == "steps", glass_attention_decode (two kernels per decoding step spread over the chip);
arg-max feedback on the device, the per-image early break applied by a mask kernel afterwards.

Mirrors reference glass/modeling/recognition/recognizer_decoder.py:65-93 and
prediction_aster.py:63-99 (greedy sampling, eos index 0, pre-zeroed [R,26,97] output with
the batch-global early break), AttentionUnit :247-266, DecoderUnit :291-302.
xEmbed(x) is recomputed at every step by the reference; it is step-invariant, so it is one
MFMA GEMM here.

Beam search (`AttentionRecognitionHead.beam_search`, prediction_aster.py:101-222, unused by the reference's inference path):
`ASTER_V2.beam_search` is the readable host statement (one decoder-step call per step, the search in torch and Python);
`ASTER_V2.beam_decode` is the same search as ONE ABI call on the device (glass_beam_search), which
`MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH` switches the recognizer head to.

Forced decoding (`AttentionRecognitionHead.forward`, prediction_aster.py:33-60, the teacher-forced call): `ASTER_V2.score`
runs the decoder with the emitted symbols given (glass_forced_decode, one ABI call, x / xproj not inflated) - the
log-likelihood of a transcription; `ASTER_V2.forward(features, labels)` is the reference's surface on top of it, and
`beam_decode(..., distributions=...)` replays the search's hypotheses for their full per-step distributions.

Lexicon-constrained decoding: `beam_decode(..., lexicon=LexiconTrie, segments=...)` is the search restricted to the words of
a lexicon (glass_beam_search_lexicon, include/glass_hip_ext.h; the reference has no counterpart): the k most likely lexicon
words under the model, with their log-likelihoods.

Pattern-constrained decoding: `beam_decode(..., pattern=DecodePattern, segments=...)` is the same search with the trie
generalised to a finite automaton over the same fold symbols (glass_beam_search_dfa, include/glass_hip_feature_dfa.h;
evaluation/pattern.py compiles a regex, a character set or a trie): the k most likely strings the pattern accepts.

Weighted patterns: with a `WeightedPattern` (evaluation/weighted_pattern.py: a character n-gram model, word priors, a length
bonus) the same call runs glass_beam_search_wdfa (include/glass_hip_feature_wdfa.h): the beams are ranked by the model score
plus `weight_scale` times the automaton's weights; the model's own scores and the path rows stay what they were.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from ...utils.module import InferenceModule

from ...checkpoint import conv_weight, dev
from ...ops import native as K
from ...utils.registry import Registry

RECOGNIZER_DECODER_REGISTRY = Registry("RECOGNIZER_DECODER")


class _BeamFields(NamedTuple):
    symbols: torch.Tensor                   # int32 [B, k, L]
    scores: torch.Tensor                    # float32 [B, k] sum of log-probabilities; -inf = no such hypothesis
    lengths: torch.Tensor                   # int32 [B, k] t + 1 for a sequence that ended at step t, else L
    path_probs: Optional[torch.Tensor]      # float32 [B, L, C] rows of the best hypothesis, or None


class BeamResult(_BeamFields):
    """`ASTER_V2.beam_decode`: device tensors, hypotheses in final (best first) order.  The tuple keeps its four fields
    (code that unpacks a result or rebuilds one from its fields is unaffected); `distributions` rides as an attribute:
    float32 full per-step rows, [B, L, C] ("best") / [B, k, L, C] ("all"), default None.  So does `words` of a
    lexicon-constrained search: int32 [B, k], the lexicon word of every hypothesis (index into `LexiconTrie.upper`), -1
    where there is none; default None.  A pattern-constrained search puts its tags there: the word index for a pattern built
    with `DecodePattern.from_trie`, 0 for a regex, -1 where there is no hypothesis.  With a `WeightedPattern` `scores` are
    the FUSED scores the search ranked by, and `model_scores` rides as an attribute: float32 [B, k], the model's own sums of
    log-probabilities (what `path_probs` is made from); default None."""

    def __new__(cls, symbols, scores, lengths, path_probs=None, distributions=None, words=None, model_scores=None):
        self = super().__new__(cls, symbols, scores, lengths, path_probs)
        self.distributions = distributions
        self.words = words
        self.model_scores = model_scores
        self.attention = None           # beam_decode(attention=True): the replayed attention rows, float32 [B, L, T] / [B, k, L, T]
        return self


class _ForcedFields(NamedTuple):
    step_logp: torch.Tensor                 # float32 [B, n, L] log-probability of targets[t] at step t; 0 from the length on
    scores: torch.Tensor                    # float32 [B, n] float32 sum of step_logp[:length] in step order
    lengths: torch.Tensor                   # int32 [B, n] steps computed
    probs: Optional[torch.Tensor]           # float32 [B, n, L, C] softmax rows (zero from the length on), or None
    logits: Optional[torch.Tensor]          # float32 [B, n, L, C] raw rows (zero from the length on), or None


class ForcedResult(_ForcedFields):
    """`ASTER_V2.score`: device tensors; the n axis is absent where the targets were given as [B, L].  The tuple keeps its five
    fields (code that unpacks a result is unaffected); `attention` rides as an attribute, as `BeamResult.model_scores` does:
    float32 [B, n, L, T], row t = the attention weights over the T encoder positions that formed the context of step t (zero
    from the length on), with `score(..., attention=True)`; default None."""

    def __new__(cls, step_logp, scores, lengths, probs=None, logits=None, attention=None):
        self = super().__new__(cls, step_logp, scores, lengths, probs, logits)
        self.attention = attention
        return self


def build_recognizer_decoderv2(cfg, input_shape):
    return RECOGNIZER_DECODER_REGISTRY.get(cfg.MODEL.ROI_RECOGNIZER_HEAD.RECOGNIZER_HEAD.DECODER.NAME)(cfg, input_shape)


@RECOGNIZER_DECODER_REGISTRY.register()
class ASTER_V2(InferenceModule):
    def __init__(self, cfg, input_shape):
        super().__init__()
        self.num_classes = len(cfg.MODEL.ROI_RECOGNIZER_HEAD.CHARACTER_SET) + 2
        self.max_word_len = int(cfg.MODEL.ROI_RECOGNIZER_HEAD.MAX_WORD_LENGTH) + 1
        self.in_channels = input_shape.channels
        self.w = {}

    def import_weights(self, sd, device, prefix: str) -> None:
        q = prefix + "recognizer.decoder."
        f = lambda k: sd[q + k].float()
        self.w = {
            "sW": dev(K.pack_kblocked(f("attention_unit.sEmbed.weight")), device),
            "sB": dev(f("attention_unit.sEmbed.bias"), device),
            "xW": conv_weight(f("attention_unit.xEmbed.weight"), device),
            "xB": dev(f("attention_unit.xEmbed.bias"), device),
            "wW": dev(f("attention_unit.wEmbed.weight").reshape(-1), device),
            "wB": dev(f("attention_unit.wEmbed.bias").reshape(-1), device),
            "emb": dev(f("tgt_embedding.weight"), device),
            "w_ih": dev(f("gru.weight_ih_l0"), device),          # [3D, 2D] row-major (MFMA GRU kernel)
            "w_hh": dev(f("gru.weight_hh_l0"), device),          # [3D, D]
            "b_ih": dev(f("gru.bias_ih_l0"), device),
            "b_hh": dev(f("gru.bias_hh_l0"), device),
            "fcW": dev(K.pack_kblocked(f("fc.weight")), device),
            "fcB": dev(f("fc.bias"), device),
            "temperature": float(sd[q + "temperature"].reshape(-1)[0]) if (q + "temperature") in sd else 1.0,
        }
        # the one-launch decoder (glass_attention_decode_persistent): sEmbed as torch stores it, and the embedding half of the
        # GRU input as a table - W_ih[:, :D] emb[c] + b_ih for every class c, computed once (fp64, stored fp32)
        D = f("gru.weight_hh_l0").shape[1]
        self.w["sW_rm"] = dev(f("attention_unit.sEmbed.weight").contiguous(), device)
        self.w["emb_gi"] = dev((f("tgt_embedding.weight").double() @ f("gru.weight_ih_l0")[:, :D].double().t()
                                + f("gru.bias_ih_l0").double()).float().contiguous(), device)

    def beam_search(self, x: torch.Tensor, beam_width: int, eos: int = 0):
        """`AttentionRecognitionHead.beam_search` (reference prediction_aster.py:101-222; never called by the reference's
        inference path, which samples greedily): x [B,T,D] -> (symbols [B, max_word_len] of the best beam, its score [B]).
        The per-step arithmetic - attention, GRU cell, fc - is one `glass_attention_decode_step` on the B x beam_width
        inflated batch; the search itself is the reference's host logic on small device tensors: log-softmax + running
        scores, top-k over beam x classes, predecessor re-indexing of the state, <eos> beams frozen at -inf, and the
        back-tracking pass including its "ended sequences replace the worst beams" bookkeeping.  One deliberate difference:
        `candidates / num_classes` is floor division here, as it was under the torch version the reference was written for -
        on a current torch the reference line yields a float index and `index_select` raises (oracle/make_golden.py --beam
        generates the golden from the reference function with exactly that operator restored)."""
        x = x.contiguous()
        B, T, D = x.shape
        k, C, L = int(beam_width), self.num_classes, self.max_word_len
        dev_ = x.device
        xproj = K.linear(x.view(B * T, D), self.w["xW"], self.w["xB"]).view(B, T, D)
        xi = x.unsqueeze(1).expand(B, k, T, D).reshape(B * k, T, D).contiguous()              # ABC -> AABBCC
        xpi = xproj.unsqueeze(1).expand(B, k, T, D).reshape(B * k, T, D).contiguous()
        state = torch.zeros((B * k, D), dtype=torch.float32, device=dev_)
        pos_index = (torch.arange(B, device=dev_) * k).view(-1, 1)
        sequence_scores = torch.full((B * k, 1), -float("inf"), device=dev_)
        sequence_scores[torch.arange(B, device=dev_) * k] = 0.0
        y_prev = torch.zeros((B * k,), dtype=torch.int32, device=dev_)
        stored_scores, stored_predecessors, stored_emitted_symbols = [], [], []
        for _ in range(L):
            logits, _, state = K.attention_decode_step(xi, xpi, self.w, state, y_prev, C)
            log_softmax_output = torch.log_softmax(logits, dim=1)
            sequence_scores = sequence_scores.repeat(1, C) + log_softmax_output
            scores, candidates = sequence_scores.view(B, -1).topk(k, dim=1)
            y_prev = (candidates % C).view(B * k).to(torch.int32)
            sequence_scores = scores.view(B * k, 1)
            predecessors = (candidates // C + pos_index.expand_as(candidates)).view(B * k, 1)
            state = state.index_select(0, predecessors.squeeze(1)).contiguous()
            stored_scores.append(sequence_scores.clone())
            sequence_scores = sequence_scores.masked_fill(y_prev.view(-1, 1) == eos, -float("inf"))
            stored_predecessors.append(predecessors)
            stored_emitted_symbols.append(y_prev.long())
        # ---- back-tracking (host bookkeeping of the reference, :165-222), on CPU copies of the small decision tables
        sc = [t.cpu() for t in stored_scores]
        pr = [t.cpu() for t in stored_predecessors]
        sy = [t.cpu() for t in stored_emitted_symbols]
        pos = pos_index.cpu()
        p = []
        lens = [[L] * k for _ in range(B)]
        sorted_score, sorted_idx = sc[-1].view(B, k).topk(k)
        s = sorted_score.clone()
        batch_eos_found = [0] * B
        t_pred = (sorted_idx + pos.expand_as(sorted_idx)).view(B * k)
        for t in range(L - 1, -1, -1):
            current_symbol = sy[t].index_select(0, t_pred)
            t_pred = pr[t].index_select(0, t_pred).squeeze(1)
            eos_indices = sy[t].eq(eos).nonzero()
            for i in range(eos_indices.size(0) - 1, -1, -1):
                idx = int(eos_indices[i][0])
                b_idx = idx // k
                res_k_idx = k - (batch_eos_found[b_idx] % k) - 1
                batch_eos_found[b_idx] += 1
                res_idx = b_idx * k + res_k_idx
                t_pred[res_idx] = pr[t][idx, 0]
                current_symbol[res_idx] = sy[t][idx]
                s[b_idx, res_k_idx] = sc[t][idx, 0]
                lens[b_idx][res_k_idx] = t + 1
            p.append(current_symbol)
        s, re_sorted_idx = s.topk(k)
        re_sorted_idx = (re_sorted_idx + pos.expand_as(re_sorted_idx)).view(B * k)
        p = [step.index_select(0, re_sorted_idx).view(B, k, -1) for step in reversed(p)]
        p = torch.cat(p, -1)[:, 0, :]
        return p.to(dev_), s[:, 0].to(dev_)

    def _targets_to_device(self, targets, lengths, B: int, device):
        """targets / lengths as `score` takes them -> (int32 [B,n,L] on `device`, int32 [B,n] | None, had_n_axis).  What comes
        from the host (lists, numpy arrays, CPU tensors) is checked here, before anything is uploaded: shape, an integer
        dtype, every symbol in [0, num_classes), every length in [0, L]; ValueError otherwise.  Device tensors are passed
        through unread (the kernel checks the range itself and ends a sequence at a symbol outside it)."""
        L, C = self.max_word_len, self.num_classes

        def one(v, name, lo, hi, what):
            on_device = torch.is_tensor(v) and v.device.type != "cpu"
            t = v if torch.is_tensor(v) else torch.as_tensor(v)
            if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
                raise ValueError(f"score: {name} must hold integers (got {t.dtype})")
            if not on_device and t.numel() and (int(t.min()) < lo or int(t.max()) > hi):
                raise ValueError(f"score: {name} outside {what} (found {int(t.min())}..{int(t.max())})")
            return t, on_device
        t, t_dev = one(targets, "targets", 0, C - 1, f"[0, {C})")
        if t.dim() not in (2, 3) or t.shape[0] != B or t.shape[-1] != L:
            raise ValueError(f"score: targets must be [B={B}, {L}] or [B={B}, n, {L}] (got {tuple(t.shape)})")
        had_n = t.dim() == 3
        t = t if had_n else t.unsqueeze(1)
        if not 1 <= t.shape[1] <= 16:
            raise ValueError(f"score: 1..16 sequences per item (got n={t.shape[1]})")
        ln = None
        if lengths is not None:
            ln, l_dev = one(lengths, "lengths", 0, L, f"[0, {L}]")
            ln = ln if had_n else ln.unsqueeze(-1)
            if tuple(ln.shape) != tuple(t.shape[:2]):
                raise ValueError(f"score: lengths {tuple(ln.shape)} do not match targets {tuple(t.shape)}")
            ln = ln.to(torch.int32).contiguous() if l_dev else K.upload(ln.contiguous(), torch.int32, device)
        t = t.to(torch.int32).contiguous() if t_dev else K.upload(t.contiguous(), torch.int32, device)
        return t, ln, had_n

    def score(self, x: torch.Tensor, targets, lengths=None, eos: int = 0, probs: bool = False, logits: bool = False,
              attention: bool = False) -> "ForcedResult":
        """Forced decoding as ONE ABI call (glass_forced_decode): the decoder run with the emitted symbols GIVEN - "how likely
        is this transcription under the model".  x [B,T,D]; targets [B,L] or [B,n,L] (L = max_word_len; n <= 16 sequences per
        item share the item's x rows, which are not inflated): the symbol emitted at each step; lengths [B] / [B,n] or None
        (None: each sequence runs up to and including its first `eos`).  -> ForcedResult on the device: per-step
        log-probabilities of the given symbols, their float32 sum in step order, the lengths, and on request the full softmax
        rows and raw logits per step; everything from a sequence's length on is zero.
        `attention`: the same replay through glass_forced_attention (include/glass_hip_feature_chars.h) - every field bit for
        bit, and `.attention` [B,n,L,T]: per step the weights over the T encoder positions that formed its context vector
        (what postprocess.char_boxes turns into character positions)."""
        x = x.contiguous()
        B, T, D = x.shape
        t, ln, had_n = self._targets_to_device(targets, lengths, B, x.device)
        xproj = K.linear(x.view(B * T, D), self.w["xW"], self.w["xB"]).view(B, T, D) if B else x
        out = K.forced_decode(x, xproj, self.w, t, ln, self.num_classes, self.max_word_len, int(eos), probs=probs, logits=logits,
                              attention=bool(attention))
        if not had_n:
            out = tuple(o.squeeze(1) if o is not None else None for o in out)
        return ForcedResult(*out)

    def _lexicon_segments(self, trie, segments, B: int, eos: int, device, what: str = "lexicon trie") -> torch.Tensor:
        """the checks of `beam_decode(lexicon=trie, segments=...)` (and of `pattern=`, `what` = "pattern") -> item segments
        int32 [B] on the device.  Host-given segments are checked before they are uploaded; a device tensor is passed through
        unread (the kernel gives an item whose segment is out of range no hypothesis)."""
        for name, have, want in (("classes", trie.num_classes, self.num_classes), ("max_len", trie.max_len, self.max_word_len),
                                 ("eos", trie.eos, int(eos))):
            if have != want:
                raise ValueError(f"beam_decode: the {what} was built for {name} = {have}, the decoder has {want}")
        S = len(trie.keys)
        if segments is None:
            if S != 1:
                raise ValueError(f"beam_decode: segments=None needs a one-segment {what.split()[0]} (this one has {S})")
            return torch.zeros((B,), dtype=torch.int32, device=device)
        if torch.is_tensor(segments) and segments.device.type != "cpu":
            if segments.dtype != torch.int32 or tuple(segments.shape) != (B,):
                raise ValueError(f"beam_decode: device segments must be int32 [B={B}] (got {segments.dtype} {tuple(segments.shape)})")
            return segments.contiguous()
        seg = torch.as_tensor(segments)
        if seg.dtype.is_floating_point or seg.dtype.is_complex or seg.dtype == torch.bool:
            raise ValueError(f"beam_decode: segments must hold integers (got {seg.dtype})")
        if tuple(seg.shape) != (B,):
            raise ValueError(f"beam_decode: segments must be [B={B}] (got {tuple(seg.shape)})")
        if seg.numel() and (int(seg.min()) < 0 or int(seg.max()) >= S):
            raise ValueError(f"beam_decode: segments outside [0, {S}) (found {int(seg.min())}..{int(seg.max())})")
        return K.upload(seg.contiguous(), torch.int32, device)

    def beam_decode(self, x: torch.Tensor, beam_width: int, eos: int = 0, path_probs: bool = False,
                    distributions: Optional[str] = None, lexicon=None, segments=None, pattern=None,
                    weight_scale: float = 1.0, merge_case: bool = False, attention: bool = False) -> "BeamResult":
        """`beam_search` as ONE ABI call (glass_beam_search): every step and the back-tracking on the device, no host
        synchronisation, x / xproj not inflated.  x [B,T,D] -> all `beam_width` hypotheses in final order, on the device;
        `path_probs`: also the best hypothesis as [B, max_word_len, num_classes] rows that the consumers of the greedy
        decoder's `pred_text_prob` read unchanged (arg-max = symbol, max = conditional probability of the step, zero rows
        from the hypothesis's length on).  Ties are ordered by flat candidate index, which `torch.topk` in `beam_search`
        leaves open.
        `distributions`: "best" / "all" - after the search, ONE forced replay (glass_forced_decode) of hypothesis 0 / of all
        k hypotheses with the search's lengths gives their FULL per-step softmax rows, [B,L,C] / [B,k,L,C]: what a consumer
        that weighs every class of a step needs (the path rows hold one entry per step).  Rows from the length on, and every
        row of a hypothesis whose score is -inf (its length is replaced by 0, on the device), are zero.
        `lexicon` (evaluation.lexicon.LexiconTrie): the search can only spell words of the lexicon (glass_beam_search_lexicon)
        - the hypotheses are the k most likely lexicon words of each item's segment, complete ones only, and the result
        carries `.words` int32 [B,k] (index into `lexicon.upper`; two case variants of a word are two hypotheses with one
        index).  With fewer than k words the rest have score -inf, length 0, word -1.  `segments`: int32 [B] on the device,
        a host sequence of segment numbers (checked here), or None = all 0 (a one-segment lexicon only).  ValueError if the
        trie was built for another number of classes, max_len or eos.
        `pattern` (evaluation.pattern.DecodePattern; not together with `lexicon`): the search can only spell strings the
        pattern accepts (glass_beam_search_dfa) - the k most likely of them, complete ones only, at most max_word_len - 1
        characters; `segments` and the checks as for a lexicon, and `.words` carries the tags: the word index for
        `DecodePattern.from_trie`, 0 for a regex, -1 for an absent hypothesis (score -inf, length 0).
        A `WeightedPattern` (evaluation.weighted_pattern) runs glass_beam_search_wdfa: the hypotheses are ranked by the model
        score + `weight_scale` * the weights of the automaton; `.scores` are these fused scores, `.model_scores` the model's
        own, and the path rows (and the replayed distributions) are made from the model's, as without weights.
        `merge_case` (with `pattern` only; include/glass_hip_feature_merged.h has the contract): the classes of one fold symbol
        - with a case-insensitive pattern a letter's two cases - are ONE candidate per beam, scored with the log of their
        summed probability and emitted as the likelier of them, so the k hypotheses are k distinct folded strings and a score
        is the probability of the word, not of one casing.  The hidden state follows the emitted class only.  With a
        case-sensitive pattern every group is one class and the result equals the unmerged search bit for bit.  The replayed
        `distributions` are those of the emitted symbols.  ValueError without `pattern`; with `lexicon=` it names
        `DecodePattern.from_trie`, the route for a lexicon.
        `attention`: the replay of hypothesis 0 (with distributions="all": of all k) runs through glass_forced_attention and the
        result carries `.attention`, float32 [B,L,T] ([B,k,L,T]): per step the weights over the T encoder positions that formed
        its context vector, zero from the hypothesis's length on (a hypothesis with score -inf: all zero).  With
        `distributions` it is the SAME replay - one, not two - and the distributions are what they are without it, bit for bit."""
        if merge_case and lexicon is not None:
            raise ValueError("beam_decode: merge_case with lexicon= (pass pattern=DecodePattern.from_trie(lexicon): the merged "
                             "search runs on the pattern tables)")
        if merge_case and pattern is None:
            raise ValueError("beam_decode: merge_case needs pattern= (the groups are the pattern's fold symbols)")
        if distributions not in (None, "best", "all"):
            raise ValueError(f'beam_decode: distributions must be None, "best" or "all" (got {distributions!r})')
        if lexicon is not None and pattern is not None:
            raise ValueError("beam_decode: lexicon and pattern together (DecodePattern.from_trie turns a lexicon into a pattern)")
        if lexicon is None and pattern is None and segments is not None:
            raise ValueError("beam_decode: segments without a lexicon")
        x = x.contiguous()
        B, T, D = x.shape
        seg = self._lexicon_segments(lexicon, segments, B, eos, x.device) if lexicon is not None else None
        if pattern is not None:
            seg = self._lexicon_segments(pattern, segments, B, eos, x.device, what="pattern")
        xproj = K.linear(x.view(B * T, D), self.w["xW"], self.w["xB"]).view(B, T, D) if B else x      # empty batch: empty results
        words = model_scores = None
        from ...evaluation.weighted_pattern import WeightedPattern
        if pattern is not None or lexicon is not None:
            weighted = isinstance(pattern, WeightedPattern)
            family = "wdfa" if weighted else "dfa" if pattern is not None else "lexicon"
            res = K.constrained_beam_search(family, x, xproj, self.w, int(beam_width), self.num_classes, self.max_word_len,
                                            int(eos), (pattern if pattern is not None else lexicon).tensors, seg, path_probs,
                                            bool(merge_case), **({"weight_scale": float(weight_scale)} if weighted else {}))
            words, model_scores = res.get("tags", res.get("words")), res.get("model_scores")
            out = (res["symbols"], res["scores"], res["lengths"], res["path"])
        else:
            out = K.beam_search(x, xproj, self.w, int(beam_width), self.num_classes, self.max_word_len, int(eos), path_probs=path_probs)
        dist = att = None
        if distributions is not None or attention:
            n = int(beam_width) if distributions == "all" else 1
            sym, sc, ln = out[0][:, :n].contiguous(), out[1][:, :n], out[2][:, :n]
            ln = torch.where(torch.isneginf(sc), torch.zeros_like(ln), ln).contiguous()
            replay = K.forced_decode(x, xproj, self.w, sym, ln, self.num_classes, self.max_word_len, int(eos),
                                     probs=distributions is not None, attention=bool(attention))
            if distributions is not None:
                dist = replay[3] if distributions == "all" else replay[3][:, 0]
            if attention:
                att = replay[5] if distributions == "all" else replay[5][:, 0]
        res = BeamResult(out[0], out[1], out[2], out[3] if path_probs else None, dist, words, model_scores)
        res.attention = att
        return res

    def forward(self, features: torch.Tensor, labels=None, roi_image: Optional[torch.Tensor] = None,
                num_images: int = 1, rnn=None, status=None) -> torch.Tensor:
        """features [R,T,D] -> probabilities [R,max_word_len,num_classes].  `roi_image` (int32 [R],
        image id per RoI) scopes the reference's early break to one image's RoIs; default: one call =
        one image, as in the reference.  `rnn` / `status`: as in BiLSTMBlockV2.forward_nhwc; without a `status` word
        (the reference's call surface) the hand-off status is read here and a give-up re-runs the decoder on the step kernels.
        With `labels` [R, max_word_len + 1] as TextEncoder.encode lays them out (slot 0 = [GO], the word from slot 1): the
        reference's teacher-forced forward (AttentionRecognitionHead.forward, prediction_aster.py:33-60) - all max_word_len
        steps, no stop, y_prev = labels[:, i] at step i - and the result is the LOGITS [R,max_word_len,num_classes]."""
        assert not self.training, "inference only"
        if labels is not None:
            L = self.max_word_len
            lab = labels if torch.is_tensor(labels) else torch.as_tensor(labels)
            if lab.dim() != 2 or lab.shape[0] != features.shape[0] or lab.shape[1] != L + 1:
                raise ValueError(f"forward: labels must be [R={features.shape[0]}, {L + 1}] (got {tuple(lab.shape)})")
            # the reference's step i >= 1 reads y_prev = labels[:, i]: the symbol "emitted" at step t is labels[:, t + 1]
            # (slot 0 is the [GO] the decoder starts from by itself; the last slot feeds no step)
            targets = lab[:, 1:]
            full = torch.full((lab.shape[0],), L, dtype=torch.int32)
            return self.score(features, targets, full, eos=0, logits=True).logits
        if status is None and rnn != "steps":
            guard = K.HandoffGuard(features.device, owner=self)
            out = self.forward(features, labels, roi_image, num_images, rnn=getattr(self, "rnn_override", None) or rnn, status=guard.status)
            guard.retry = lambda: self.forward(features, labels, roi_image, num_images, rnn="steps")
            again = guard.resolve(guard.status.item())
            return out if again is None else again
        x = features.contiguous()
        R, T, D = x.shape
        if roi_image is None:
            roi_image = torch.zeros((R,), dtype=torch.int32, device=x.device)
            num_images = 1
        xproj = K.linear(x.view(R * T, D), self.w["xW"], self.w["xB"]).view(R, T, D)
        return K.attention_decode(x, xproj, self.w, roi_image, num_images, self.num_classes, self.max_word_len, 0,
                                  mode=rnn if rnn is not None else K.routing_of(self.w["xW"]).rnn, status=status)
