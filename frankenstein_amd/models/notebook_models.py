"""The model classes the reference defines only inside its trainer notebooks, on the HIP kernels:

  BrainEncoder   notebooks_trainer/franky_baseline_gpt2.ipynb cell 3  (encoder + perceiver -> ``to_words`` features)
  Franky         notebooks_trainer/franky_baseline_gpt2.ipynb cell 4  (brain features as GPT prefix, CE loss)
  BrainFormerCE  notebooks_trainer/train_brainformer.ipynb cell 3     (``BrainFormer`` there: vocab head + CE)
  BrainFormerCTC no counterpart in the reference: the same read-out under a CTC loss, with greedy and prefix-beam decoding

Same constructor / forward signatures and state-dict keys as the notebook classes, so a notebook can
``from frankenstein_amd.models.notebook_models import BrainEncoder, Franky`` instead of defining them inline.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import engine as E
from .brainformer import BrainFormer as _FileBrainFormer
from .brainformer import Config


BEAM_BATCH_ROWS = 16    # rows (sentences x beams) of a batched beam search by default: the most the weight-streaming decode step takes


class BrainEncoder(_FileBrainFormer):
    """forward(x) -> logits/features [B, n_output_tokens, output_dim] (no loss)."""
    config = Config
    head_name = 'to_words'

    def forward(self, x, targets=None, date_info=None):
        return self.features(x, date_info)


class BrainFormerCE(_FileBrainFormer):
    """forward(x, targets) -> (CE loss over all output tokens with ignore_index=-100, logits)."""
    config = Config
    head_name = 'to_words'

    def forward(self, x, targets=None, date_info=None):
        if targets is not None and getattr(self, "fuse_head_loss", False):
            # loss only (train_utils.enable_fused_head_loss): perceiver.ln_f -> to_words -> CE without the [B, tokens, V] logits
            q = self.queries_out(x, date_info)
            head, ln = self.perceiver[self.head_name], self.perceiver.ln_f
            return E.head_cross_entropy(q, ln.weight, ln.bias, head.weight, head.bias, targets, ln.eps, -100, getattr(self, "head_chunk", 8192)), None
        logits = self.features(x, date_info)
        if targets is None:
            return None, logits
        return E.cross_entropy(logits, targets, -100), logits


class BrainFormerCTC(_FileBrainFormer):
    """The read-out of BrainFormerCE under a CTC loss: the `n_output_tokens` read-out tokens are the time axis, `output_dim` is the number
    of classes with the blank among them.  The blank defaults to the LAST class (output_dim - 1), so GPT-2 BPE targets keep their ids
    (50258 classes, blank 50257) and a phoneme inventory keeps its numbering.

    forward(x, targets) -> (CTC loss, logits [B, n_output_tokens, output_dim]); targets int64 [B, Lmax] padded with -100, at most 255
    labels.  The loss is the mean of torch's F.ctc_loss with zero_infinity=True: a sentence that does not fit into the read-out (more
    labels plus adjacent repeats than read-out tokens) contributes 0 and no gradient instead of turning the run into inf.
    decode(x) -> (ids int64 [B, n_output_tokens] padded with -100, lengths int64 [B]): the best path, repeats merged and blanks dropped.
    decode(x, beam_width=W, topk=None, nbest=1): prefix beam search (engine.ctc_beam_decode), the most probable labelling in the same
    form; nbest > 1 -> (ids [B, nbest, n_output_tokens], lengths [B, nbest], scores [B, nbest]), best first, for rescoring.
    decode(x, beam_width=W, nbest=k, lm=gpt, lm_prefix=None, lm_weight=1.0, length_bonus=0.0, eos_token_id=None): the whole final beam
    (W hypotheses) is rescored by the GPT `lm` on the device (GPT.rescore_nbest: total = CTC score + lm_weight * log p_lm + length_bonus *
    length; lm_prefix = the brain features a Franky conditions on) and the first k of the new order come back in the same forms, the
    scores being the totals.  A hypothesis that holds the blank id or another token outside the LM's vocabulary is not scored and ranks last.
    decode(x, beam_width=W, nbest=k, ngram=m, ngram_weight=1.0, ngram_bonus=0.0, ngram_eos=True): the backoff n-gram model `m`
    (utils.ngram.NGramLM over the output_dim classes) takes part in every selection of the search (engine.ctc_beam_decode_lm), the way a
    phoneme head gets a language model at all; same forms, the scores being the fused totals.  With ngram= AND lm= the fused search fills
    the whole beam, the GPT rescores it with the PURE CTC score as its acoustic score (the n-gram only decides which hypotheses reach the
    list; its own score is not added a second time), and the first k of the GPT's order come back.
    decode(..., beam_width=W, nbest=k, mbr=True, mbr_scale=1.0): minimum-Bayes-risk selection as the last step.  The WHOLE final list (W
    hypotheses) of whichever path was asked for, with that path's ranking score (the CTC score, the fused total, the GPT's total), goes
    through engine.mbr_rerank: the hypothesis with the smallest expected edit distance under softmax(mbr_scale * score) comes first.  The
    first k of that order come back in the same forms, the scores being -risk.
    decode_words(x, lexicon, sep, beam_width=W, nbest=1, ngram=word_lm, ...): WORDS out of a phoneme / letter head whose class `sep` separates
    words: the search constrained to the pronunciations of a utils.lexicon.Lexicon with a word-level n-gram model at word ends
    (engine.ctc_beam_decode_lexicon) -> (words, word_lengths[, scores]); word_error_rate(x, target_words, lexicon, sep, ...) is its
    engine.error_rate.  decode itself is unchanged by it.
    utils.metrics.token_error_rate(targets, ids) of that result is the phoneme / token error rate; error_rate(x, targets, **decode
    arguments) computes the same number on the device (engine.error_rate).
    mwer_weight (constructor argument or attribute, default None = off): forward's loss becomes ctc + mwer_weight * mwer, one
    engine.ctc_mwer_loss over the n-best list of a prefix beam search (mwer_beam = 8 wide, mwer_nbest = 4 hypotheses); the logits are expanded
    mwer_nbest times for it (engine.ctc_mwer_loss says what that costs).
    align(x, targets): forced alignment (engine.ctc_forced_align), where in the read-out every label of a transcript or hypothesis sits and
    how confident the head is of it."""
    config = Config
    head_name = 'to_words'

    def __init__(self, config: Config, blank=None, mwer_weight=None, mwer_beam=8, mwer_nbest=4):
        super().__init__(config)
        self.mwer_weight, self.mwer_beam, self.mwer_nbest = mwer_weight, mwer_beam, mwer_nbest
        self.blank = config.output_dim - 1 if blank is None else int(blank)
        if not 0 <= self.blank < config.output_dim:
            raise ValueError(f"blank = {self.blank} outside [0, output_dim = {config.output_dim})")

    def forward(self, x, targets=None, date_info=None):
        logits = self.features(x, date_info)
        if targets is None:
            return None, logits
        if self.mwer_weight is None:
            return E.ctc_loss(logits, targets, blank=self.blank, reduction='mean', zero_infinity=True, pad_value=-100), logits
        return E.ctc_mwer_loss(logits, targets, beam_width=self.mwer_beam, nbest=self.mwer_nbest, blank=self.blank, ce_weight=1.0, pad_value=-100,
                               mwer_weight=self.mwer_weight, zero_infinity=True), logits

    @torch.no_grad()
    def error_rate(self, x, targets, date_info=None, **decode_kwargs):
        """decode(x, **decode_kwargs), its best hypothesis against targets (int64 [B, Lmax] padded with -100) -> engine.error_rate's (rate,
        errors, ref_lengths): the corpus error rate as a device scalar, no synchronisation"""
        out = self.decode(x, date_info=date_info, **decode_kwargs)
        ids, lengths = (out[0][:, 0], out[1][:, 0]) if out[0].dim() == 3 else (out[0], out[1])
        return E.error_rate(targets, ids, hypothesis_lengths=lengths, pad_value=-100)

    @torch.no_grad()
    def align(self, x, targets, input_lengths=None, target_lengths=None, date_info=None):
        """Forced alignment of the read-out to `targets` (int64 [B, Lmax] padded with -100, or with target_lengths): the most probable
        alignment as an engine.CtcAlignment (score, path, index, start, end, label_lp, .confidence), frames being read-out tokens.  To
        align a hypothesis of the beam search (ids, lengths, scores = decode(x, beam_width=W, nbest=k)): align(x, ids[:, 0, :Lmax],
        target_lengths=lengths[:, 0]) with Lmax <= 255 at least the longest hypothesis; its confidence flags the shaky tokens."""
        return E.ctc_forced_align(self.features(x, date_info), targets, input_lengths, target_lengths, blank=self.blank, pad_value=-100, pad=-100)

    @torch.no_grad()
    def decode(self, x, beam_width=None, topk=None, nbest=1, lm=None, lm_prefix=None, lm_weight=1.0, length_bonus=0.0, eos_token_id=None,
               am_weight=1.0, bos_token_id=50256, max_nodes=None, ngram=None, ngram_weight=1.0, ngram_bonus=0.0, ngram_eos=True, mbr=False,
               mbr_scale=1.0, date_info=None):
        logits = self.features(x, date_info)
        if mbr:
            if beam_width is None:
                raise ValueError("decode(mbr=True) re-ranks a beam: give a beam_width")
            return self._decode_mbr(logits, beam_width, topk, nbest, lm, lm_prefix, lm_weight, length_bonus, eos_token_id, am_weight, bos_token_id,
                                    max_nodes, ngram, ngram_weight, ngram_bonus, ngram_eos, mbr_scale)
        if beam_width is None:
            if lm is not None or ngram is not None:
                raise ValueError("decode(lm=...) rescores a beam and decode(ngram=...) steers one: give a beam_width")
            return E.ctc_greedy_decode(logits, blank=self.blank, pad=-100)
        fused = dict(blank=self.blank, beam_width=beam_width, topk=topk, lm_weight=ngram_weight, length_bonus=ngram_bonus, use_eos=ngram_eos, pad=-100)
        if lm is None and ngram is not None:
            ids, lengths, _, _, total = E.ctc_beam_decode_lm(logits, ngram, nbest=nbest, **fused)
            return (ids[:, 0], lengths[:, 0]) if nbest == 1 else (ids, lengths, total)
        if lm is None:
            ids, lengths, scores = E.ctc_beam_decode(logits, blank=self.blank, beam_width=beam_width, topk=topk, nbest=nbest, pad=-100)
            return (ids[:, 0], lengths[:, 0]) if nbest == 1 else (ids, lengths, scores)
        # the WHOLE final beam is rescored (GPT.rescore_nbest) and the first nbest places of the new order come back; scores = total
        if ngram is not None:                             # the n-gram decides which hypotheses reach the list; the GPT scores them on am
            ids, lengths, scores, _, _ = E.ctc_beam_decode_lm(logits, ngram, nbest=beam_width, **fused)
        else:
            ids, lengths, scores = E.ctc_beam_decode(logits, blank=self.blank, beam_width=beam_width, topk=topk, nbest=beam_width, pad=-100)
        ids, lengths, _, _, total, _, _ = lm.rescore_nbest(ids, lengths, scores, prefix=lm_prefix, lm_weight=lm_weight, am_weight=am_weight,
                                                           length_bonus=length_bonus, bos_token_id=bos_token_id, eos_token_id=eos_token_id,
                                                           max_nodes=max_nodes)
        return (ids[:, 0], lengths[:, 0]) if nbest == 1 else (ids[:, :nbest], lengths[:, :nbest], total[:, :nbest])

    @torch.no_grad()
    def decode_words(self, x, lexicon, sep, beam_width=8, topk=None, nbest=1, ngram=None, ngram_weight=1.0, word_bonus=0.0, ngram_eos=True,
                     mbr=False, mbr_scale=1.0, date_info=None):
        """Words out of a phoneme / letter head (engine.ctc_beam_decode_lexicon): the beam search constrained to the pronunciations of
        `lexicon` (utils.lexicon.Lexicon) with the class `sep` between words and the WORD-level n-gram model `ngram` (utils.ngram.NGramLM over
        the lexicon's word ids, or None) at word ends -> (words int64 [B, L] padded with -100, word_lengths int64 [B]), L = (n_output_tokens +
        1) // 2; nbest > 1 -> (words [B, nbest, L], word_lengths [B, nbest], scores [B, nbest]), best first, the scores being the totals.
        mbr=True: the whole final list (beam_width hypotheses) goes through engine.mbr_rerank over its WORDS with the total as its score, and
        the first nbest of that order come back, the scores being -risk.  lexicon.text(words, word_lengths) gives the strings."""
        logits = self.features(x, date_info)
        r = E.ctc_beam_decode_lexicon(logits, lexicon, ngram, sep=sep, blank=self.blank, beam_width=beam_width, topk=topk,
                                      nbest=beam_width if mbr else nbest, lm_weight=ngram_weight, word_bonus=word_bonus, use_eos=ngram_eos, pad=-100)
        words, word_lengths, scores = r.words, r.word_lengths, r.total
        if mbr:
            m = E.mbr_rerank(words, word_lengths, scores, scale=mbr_scale, pad=-100)
            words, word_lengths, scores = m.ids[:, :nbest], m.lengths[:, :nbest], -m.risk[:, :nbest]
        return (words[:, 0], word_lengths[:, 0]) if nbest == 1 else (words, word_lengths, scores)

    @torch.no_grad()
    def word_error_rate(self, x, target_words, lexicon, sep, date_info=None, **decode_kwargs):
        """decode_words(x, lexicon, sep, **decode_kwargs), its best hypothesis against target_words (int64 [B, Lmax] word ids padded with
        -100) -> engine.error_rate's (rate, errors, ref_lengths): the corpus word error rate as a device scalar, no synchronisation"""
        out = self.decode_words(x, lexicon, sep, date_info=date_info, **decode_kwargs)
        words, lengths = (out[0][:, 0], out[1][:, 0]) if out[0].dim() == 3 else (out[0], out[1])
        return E.error_rate(target_words, words, hypothesis_lengths=lengths, pad_value=-100)

    def _decode_mbr(self, logits, beam_width, topk, nbest, lm, lm_prefix, lm_weight, length_bonus, eos_token_id, am_weight, bos_token_id, max_nodes,
                    ngram, ngram_weight, ngram_bonus, ngram_eos, mbr_scale):
        """the whole final list of the path asked for, with that path's ranking score, through engine.mbr_rerank"""
        if ngram is not None:
            ids, lengths, am, _, score = E.ctc_beam_decode_lm(logits, ngram, blank=self.blank, beam_width=beam_width, topk=topk, nbest=beam_width,
                                                              lm_weight=ngram_weight, length_bonus=ngram_bonus, use_eos=ngram_eos, pad=-100)
        else:
            ids, lengths, score = E.ctc_beam_decode(logits, blank=self.blank, beam_width=beam_width, topk=topk, nbest=beam_width, pad=-100)
            am = score
        if lm is not None:
            ids, lengths, _, _, score, _, _ = lm.rescore_nbest(ids, lengths, am, prefix=lm_prefix, lm_weight=lm_weight, am_weight=am_weight,
                                                               length_bonus=length_bonus, bos_token_id=bos_token_id, eos_token_id=eos_token_id,
                                                               max_nodes=max_nodes)
        r = E.mbr_rerank(ids, lengths, score, scale=mbr_scale, pad=-100)
        return (r.ids[:, 0], r.lengths[:, 0]) if nbest == 1 else (r.ids[:, :nbest], r.lengths[:, :nbest], -r.risk[:, :nbest])


class Franky(nn.Module):
    """Brain features -> GPT prefix; targets' -100 padding is replaced by token 50256 for the input ids."""

    def __init__(self, brain_model, llm_model, tokenizer=None):
        super().__init__()
        self.brain_model = brain_model
        self.llm_model = llm_model
        self.tokenizer = tokenizer
        print("Full Franky: number of parameters: %.2fM" % (self.get_num_params() / 1e6,))

    def get_num_params(self):
        return sum(p.numel() for p in self.parameters())

    @property
    def dtype(self) -> torch.dtype:
        return next(self.parameters()).dtype

    @property
    def device(self) -> torch.device:
        return next(self.parameters()).device

    def _brain(self, x, date_info):
        """brain_model(x), with the sessions of the samples when there are any (a brain model without the argument keeps working)"""
        return self.brain_model(x) if date_info is None else self.brain_model(x, date_info=date_info)

    def forward(self, x, targets=None, date_info=None):
        features = self._brain(x, date_info)
        new_idx = targets.clone()
        new_idx[new_idx == -100] = 50256
        return self.llm_model.forward(idx=new_idx, prefix=features, targets=targets)

    @torch.no_grad()
    def rescore(self, x, ids, lengths, scores, date_info=None, **weights):
        """Re-rank the n-best lists (ids [S, n, T], lengths, scores [S, n]: BrainFormerCTC.decode(..., nbest=n) of the same trials) under the
        decoder conditioned on the brain features of x (tensor [S, T, C]): brain_model(x) is the prefix of llm_model.rescore_nbest, whose
        keyword arguments (lm_weight, am_weight, length_bonus, eos_token_id, max_nodes, ...) and ranked outputs these are."""
        return self.llm_model.rescore_nbest(ids, lengths, scores, prefix=self._brain(x, date_info), **weights)

    @torch.no_grad()
    def generate(self, x, max_new_tokens=25, temperature=1.0, top_k=10, eot=50256, stop=False, top_p=None, repetition_penalty=1.0,
                 no_repeat_ngram_size=0, min_new_tokens=0, date_info=None):
        """x: numpy [T, C].  Returns generated token ids (the notebook's version is unfinished; this one runs).
        stop=True ends a sentence at its first generated `eot` (what the notebook's cell tried with its undefined stop_tokens): the ids come
        back trimmed behind that token; x: numpy [S, T, C] then decodes S trials, returns [S, 1 + max_new_tokens] padded with `eot` and sets
        last_lengths [S] (generated tokens, `eot` included).
        top_p: nucleus sampling behind the top-k crop (GPT.generate), with and without stop; None or 1.0: off, outside (0, 1] raises.
        repetition_penalty / no_repeat_ngram_size / min_new_tokens: GPT.generate's rules on the tokens already emitted.  `eot`, which is the
        prompt here, is exempt from the penalty and from the n-gram ban (a deliberate departure from the usual implementations: penalising
        it would push every sentence away from ending); min_new_tokens keeps it from being emitted too early and needs stop=True."""
        self.llm_model._check_top_p(top_p)                                  # before the encoder runs
        rules = self._rules(repetition_penalty, no_repeat_ngram_size, min_new_tokens, eot if stop else None, max_new_tokens, top_k or 1)
        if stop:
            xin = torch.from_numpy(x if x.ndim == 3 else x[None]).to(self.device).float()
            prefix = self._brain(xin, date_info)
            ids = torch.full((xin.shape[0], 1), eot, dtype=torch.long, device=self.device)
            self.llm_model.generate(ids, max_new_tokens, prefix=prefix, temperature=temperature, top_k=top_k, eos_token_id=eot, top_p=top_p, **rules)
            self.last_lengths = self.llm_model.last_lengths.cpu()           # int64 on the host, as generate_beam leaves it
            if x.ndim == 3:
                return self.llm_model.last_tokens
            return self.llm_model.last_tokens[0, :1 + int(self.last_lengths[0])]
        xin = torch.from_numpy(x[None]).to(self.device).float()
        prefix = self._brain(xin, date_info)
        ids = torch.full((1, 1), eot, dtype=torch.long, device=self.device)
        return self.llm_model.generate(ids, max_new_tokens, prefix=prefix, temperature=temperature, top_k=top_k, top_p=top_p, **rules)

    def _rules(self, repetition_penalty, no_repeat_ngram_size, min_new_tokens, eos, max_new_tokens, keep):
        """GPT._check_logit_rules for a prompt of one token, before the encoder runs -> the keyword arguments to pass on ({}: all off)"""
        rules = self.llm_model._check_logit_rules(repetition_penalty, no_repeat_ngram_size, min_new_tokens, eos, self.llm_model.config.vocab_size,
                                                  1 + max_new_tokens, keep)
        return {} if rules is None else {k: v for k, v in rules.items() if k != "eos_token_id"}

    @torch.no_grad()
    def generate_beam(self, x, max_new_tokens=25, temperature=1.0, topk=20, beam_width=5, eot=50256, batch_sentences=None, stop=False,
                      length_penalty=0.0, repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, ctc=None, ctc_weight=0.0,
                      date_info=None):
        """x: numpy [T, C].  Brain features -> prefix -> the stochastic beam search of the decoder on its key/value caches
        (GPT.generate_beam_search, use_cache=True).  Returns the best beam's ids, `eot` first.
        x: numpy [S, T, C] decodes S trials and returns ids [S, 1 + max_new_tokens]: the encoder and the search run in chunks of
        `batch_sentences` trials that share every decode step (default: BEAM_BATCH_ROWS // beam_width, the rows that stay on the
        weight-streaming route of the decode step).
        stop=True makes `eot` the end-of-text id of the search (finished beams, ranking by score / length^length_penalty, early exit):
        [T, C] returns the best beam trimmed behind its first generated `eot`, [S, T, C] the padded [S, 1 + max_new_tokens] and sets
        last_lengths [S].
        repetition_penalty / no_repeat_ngram_size / min_new_tokens: GPT.generate_beam_search's rules on every beam's own tokens; `eot` is
        exempt from the penalty and the n-gram ban (see generate), min_new_tokens needs stop=True.
        ctc (a BrainFormerCTC over the same token ids) with ctc_weight > 0: one-pass joint CTC / attention decoding
        (GPT.generate_beam_search's ctc_* arguments): ctc.features of the same chunk of trials are the frames, ctc.blank the blank, and the
        prompt `eot` counts as the first label of the transcript, because the targets the head was trained on begin with it.  ctc None or
        ctc_weight 0: off, the head does not run and the result is the one without the arguments."""
        rules = self._rules(repetition_penalty, no_repeat_ngram_size, min_new_tokens, eot if stop else None, max_new_tokens,
                            2 * beam_width if topk is None else topk)
        if not 0.0 <= float(ctc_weight) <= 1.0:                              # before the encoder runs
            raise ValueError(f"ctc_weight must lie in [0, 1], got {ctc_weight!r}")
        if float(ctc_weight) > 0.0 and ctc is None:
            raise ValueError("ctc_weight > 0 needs the CTC model `ctc`")

        def days(s0, n):                                                     # the sessions of trials s0 .. s0 + n - 1
            return date_info[s0:s0 + n] if isinstance(date_info, torch.Tensor) and date_info.dim() > 0 else date_info

        def ctc_kw(xin, di):                                                 # the head runs on the chunk of trials the encoder just saw
            if ctc is None or float(ctc_weight) == 0.0:
                return {}
            return dict(ctc_logits=ctc.features(xin, di), ctc_weight=float(ctc_weight), ctc_blank=ctc.blank, ctc_from_prompt=1)

        eos_kw = dict(eos_token_id=eot if stop else None, length_penalty=length_penalty) if (stop or length_penalty != 0.0) else {}
        if x.ndim == 2:
            xin = torch.from_numpy(x[None]).to(self.device).float()
            prefix = self._brain(xin, date_info)
            ids = torch.full((1, 1), eot, dtype=torch.long, device=self.device)
            out = self.llm_model.generate_beam_search(ids, max_new_tokens, prefix, temperature=temperature, topk=topk, beam_width=beam_width,
                                                      use_cache=True, **eos_kw, **rules, **ctc_kw(xin, date_info))
            if eos_kw:
                self.last_lengths = torch.tensor([self.llm_model.last_beam_lengths[0]])
            return out[:1 + int(self.last_lengths[0])] if stop else out
        if batch_sentences is None:
            batch_sentences = max(1, BEAM_BATCH_ROWS // beam_width)
        outs, lengths = [], []
        for s0 in range(0, x.shape[0], batch_sentences):
            xin = torch.from_numpy(x[s0:s0 + batch_sentences]).to(self.device).float()
            di = days(s0, xin.shape[0])
            prefix = self._brain(xin, di)
            ids = torch.full((xin.shape[0], 1), eot, dtype=torch.long, device=self.device)
            out = self.llm_model.generate_beam_search(ids, max_new_tokens, prefix, temperature=temperature, topk=topk, beam_width=beam_width,
                                                      use_cache=True, **eos_kw, **rules, **ctc_kw(xin, di))
            outs.append(out.view(xin.shape[0], -1))
            if eos_kw:
                lens = self.llm_model.last_beam_lengths
                lengths += [lens[0]] if xin.shape[0] == 1 else [l[0] for l in lens]
        if eos_kw:
            self.last_lengths = torch.tensor(lengths)
        return torch.cat(outs)
