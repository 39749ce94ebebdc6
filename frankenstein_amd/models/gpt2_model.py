"""MI355X-native GPT-2 decoder with the reference's ``models/gpt2_model.py`` surface: ``GPTConfig``,
``GPT(config).forward(idx, prefix=None, targets=None) -> (loss, logits)`` with brain-feature *prefix*
embeddings, tied ``lm_head``/``wte``, and the same state-dict keys.  Forward/backward run on the HIP
kernels (fused c_attn GEMM + causal flash attention + GELU MLP + CE).

Reference map: LayerNorm models/gpt2_model.py:18-27, CausalSelfAttention :29-76, MLP :78-92,
Block :94-106, GPTConfig :108-116, GPT :118-216 (+ crop_block_size :218-227, from_pretrained :229-284,
configure_optimizers :286-310, estimate_mfu :312-326, generate :328-353).
"""
from __future__ import annotations

import math
import numbers
from dataclasses import dataclass

import torch
import torch.nn as nn

from .. import engine as E
from .. import kernels as K
from ..kernels import MASK_CAUSAL, Mask
from .brainformer import Linear, _prep

CAUSAL = Mask(MASK_CAUSAL)


class LayerNorm(nn.Module):
    """LayerNorm with an optional bias (eps 1e-5)."""

    def __init__(self, ndim, bias):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(ndim))
        self.bias = nn.Parameter(torch.zeros(ndim)) if bias else None
        self.eps = 1e-5

    def forward(self, input):
        return E.LayerNormFn.apply(_prep(input), self.weight, self.bias, self.eps, K.NORM_LAYER)


LORA_TARGETS = ("c_attn", "attn.c_proj", "c_fc", "mlp.c_proj")      # the adaptable Linears of a block (GPT.add_lora)


def _lora_of(lin):
    """(lora_A, lora_B, scale) of an adapted Linear (GPT.add_lora), else None"""
    a = getattr(lin, "lora_A", None)
    return None if a is None else (a, lin.lora_B, lin.lora_scale)


class CausalSelfAttention(nn.Module):
    def __init__(self, config):
        super().__init__()
        assert config.n_embd % config.n_head == 0
        self.c_attn = Linear(config.n_embd, 3 * config.n_embd, bias=config.bias)
        self.c_proj = Linear(config.n_embd, config.n_embd, bias=config.bias)
        self.n_head = config.n_head
        self.n_embd = config.n_embd
        self.dropout = config.dropout

    def branch(self, x, ln, residual: bool, mask=None):
        """mask: a kernels.Mask in place of the causal one (the ancestor table of a packed n-best forward); None: CAUSAL"""
        spec = (self.n_head, self.n_embd // self.n_head, CAUSAL if mask is None else mask, None, residual, 0.0 if ln is None else ln.eps, K.NORM_LAYER)
        if self.dropout and self.training:          # SDPA dropout_p + resid_dropout (models/gpt2_model.py:64,75): two sites
            spec = spec + (E.drop_spec(self.dropout, x.device, 2),)
        la, lp = _lora_of(self.c_attn), _lora_of(self.c_proj)
        if la is not None or lp is not None:
            return E.AttnBranchLora.apply(x, None if ln is None else ln.weight, None if ln is None else ln.bias,
                                          self.c_proj.weight, self.c_proj.bias, self.c_attn.bias, spec, (la or lp)[2],
                                          *(la or (None, None))[:2], *(lp or (None, None))[:2], self.c_attn.weight)
        return E.AttnBranch.apply(x, None if ln is None else ln.weight, None if ln is None else ln.bias,
                                  self.c_proj.weight, self.c_proj.bias, self.c_attn.bias, spec, self.c_attn.weight)

    def forward(self, x):
        return self.branch(_prep(x), None, False)


class MLP(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.c_fc = Linear(config.n_embd, 4 * config.n_embd, bias=config.bias)
        self.gelu = nn.GELU()
        self.c_proj = Linear(4 * config.n_embd, config.n_embd, bias=config.bias)
        self.dropout = nn.Dropout(config.dropout)

    def branch(self, x, ln, residual: bool):
        spec = (residual, 0.0 if ln is None else ln.eps, K.NORM_LAYER)
        if self.dropout.p and self.training:        # models/gpt2_model.py:91
            spec = spec + (E.drop_spec(self.dropout.p, x.device, 1),)
        lf, lp = _lora_of(self.c_fc), _lora_of(self.c_proj)
        if lf is not None or lp is not None:
            return E.MlpBranchLora.apply(x, None if ln is None else ln.weight, None if ln is None else ln.bias,
                                         self.c_fc.weight, self.c_fc.bias, None, self.c_proj.weight, self.c_proj.bias, spec, (lf or lp)[2],
                                         *(lf or (None, None))[:2], *(lp or (None, None))[:2])
        return E.MlpBranch.apply(x, None if ln is None else ln.weight, None if ln is None else ln.bias,
                                 self.c_fc.weight, self.c_fc.bias, None, self.c_proj.weight, self.c_proj.bias, spec)

    def forward(self, x):
        return self.branch(_prep(x), None, False)


class Block(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.ln_1 = LayerNorm(config.n_embd, bias=config.bias)
        self.attn = CausalSelfAttention(config)
        self.ln_2 = LayerNorm(config.n_embd, bias=config.bias)
        self.mlp = MLP(config)

    def forward(self, x, mask=None):
        x = self.attn.branch(_prep(x), self.ln_1, True, mask)
        return self.mlp.branch(x, self.ln_2, True)

    @torch.no_grad()
    def forward_cached(self, x, kv, pos):
        """Incremental inference step: x [B, t, d] are the tokens at positions pos..pos+t-1, kv [B, Tmax, 2d] this layer's
        key|value cache (rows < pos filled by earlier calls).  Same kernels as the training forward; attention is the
        causal mask with the query offset pos, so a t = 1 step costs O(pos) instead of re-running the whole sequence
        (the reference re-forwards everything per token, models/gpt2_model.py:336-340)."""
        B, t, d = x.shape
        at, ml = self.attn, self.mlp
        H, D = at.n_head, d // at.n_head
        x2 = x.reshape(B * t, d)
        qkv = _step_linear(x2, at.c_attn, ln=self.ln_1)
        q3 = qkv.view(B, t, 3 * d)
        for b in range(B):                                   # append k|v rows of the new tokens
            K.copy2d(q3[b, :, d:], kv[b, pos:pos + t])
        k = kv[:, :pos + t, :d].unflatten(-1, (H, D))
        v = kv[:, :pos + t, d:].unflatten(-1, (H, D))
        o, _ = K.attn_fwd(q3[..., :d].unflatten(-1, (H, D)), k, v, Mask(MASK_CAUSAL, q_off=pos))
        x2 = _step_linear(o.view(B * t, d), at.c_proj, residual=x2)
        a = _step_linear(x2, ml.c_fc, ln=self.ln_2, gelu=True)
        x2 = _step_linear(a, ml.c_proj, residual=x2)
        return x2.view(B, t, d)


def _bias(lin):
    return None if lin.bias is None else E.shadow([lin.bias])


GEMV_MAX_ROWS = 16      # the envelope of K.gemv_nt (fk_gemv_nt: 1 <= M <= 16)


def _step_linear(x, lin, ln=None, gelu=False, residual=None, step_rows=None, head_vocab=None):
    """One linear layer of a cached inference step, x [rows, K]: act(LN(x) W^T + bias) + residual.
    A step of at most GEMV_MAX_ROWS rows (step_rows = B * t, by default the rows of x) is a decode step: the layer is ONE
    weight-streaming launch (K.gemv_nt) with the LayerNorm in front, the bias, the GELU and the residual folded in.  Anything
    larger (the prefill) runs the training kernels: norm, MFMA GEMM, GELU.  The host-position step (forward_cached,
    _cached_logits) and the device-position step (forward_decode, _decode_logits_dev) both come through here, so they take
    the same route.  head_vocab = V: the vocabulary head, fp32 logits [rows, V] from the 16-byte-padded shadow of the weight."""
    rows = x.shape[0] if step_rows is None else step_rows
    lo = _lora_of(lin)
    if lo is not None:              # an adapted Linear: the shadow of the merged weight, refreshed in place with the adapters
        assert head_vocab is None
        w, n, odt = E.shadow_lora(lin.weight, *lo), None, None
    elif head_vocab is None:
        w, n, odt = E.shadow([lin.weight]), None, None
    else:
        w, n, odt = E.shadow([lin.weight], pad_n=(head_vocab + 7) // 8 * 8), head_vocab, torch.float32   # 16-byte rows for the vector GEMM epilogue
    lnp = None if ln is None else (ln.weight.detach(), None if ln.bias is None else ln.bias.detach(), ln.eps)
    if rows <= GEMV_MAX_ROWS:
        return K.gemv_nt(x, w, _bias(lin), residual=residual, ln=lnp, act="gelu" if gelu else None, out_dtype=odt, n=n)
    if lnp is not None:
        x, _, _ = K.norm_fwd(x, *lnp)
    y = K.gemm_nt(x, w, _bias(lin), residual=residual, out_dtype=odt)
    if gelu:
        y = K.gelu_fwd(y)
    return y if head_vocab is None else y[:, :head_vocab]


def _block_forward_decode(self, x, kv, pos, anc=None, groups=None):
    """One new token per sample with the position in a device int32 (graph-capturable): x [B, d], kv [B, Tmax, 2d].
    anc (int32 [B, Tmax]): the samples are beams that share the caches, row j of beam b is read from slot anc[b, j] (K.attn_decode_beam).
    groups = S: the B rows are S sentences x B / S beams and anc holds slots counted inside the sentence; the append of the new key|value
    row is part of the attention launch (K.attn_decode_beam_grouped)."""
    at, ml = self.attn, self.mlp
    qkv = _step_linear(x, at.c_attn, ln=self.ln_1)
    if groups is not None:
        o = K.attn_decode_beam_grouped(qkv, kv, anc, pos, at.n_head, groups, append=True)
    else:
        K.kv_append_(qkv, kv, pos)
        o = K.attn_decode(qkv, kv, pos, at.n_head) if anc is None else K.attn_decode_beam(qkv, kv, anc, pos, at.n_head)
    x = _step_linear(o, at.c_proj, residual=x)
    a = _step_linear(x, ml.c_fc, ln=self.ln_2, gelu=True)
    return _step_linear(a, ml.c_proj, residual=x)


Block.forward_decode = _block_forward_decode


def _beam_step_host(top_lp, top_ix, picks, scores, lens, fin, eos, inv_lenpow):
    """One selection step of the stochastic beam search with the end-of-text rules of fk_beam_select_eos, on host tensors (the
    re-forward path; the draws `picks` [W, W] are the caller's).  A live beam i proposes its W picks, raw = scores[i] + top_lp[i, pick]
    (one fp32 add), L = lens[i] + 1; a finished beam proposes itself once (candidate r = 0: token eos, raw = scores[i], L = lens[i]).
    The W best candidates by raw * inv_lenpow[clamp(L)] (one fp32 multiply) survive, ties by candidate number i * W + r.
    top_lp fp32 / top_ix int64 [W, k], scores fp32 [W], lens int [W], fin bool [W], eos an id or -1, inv_lenpow fp32 [n]
    -> parent int64 [W], token int64 [W], scores fp32 [W] (raw), lens [W], fin bool [W]."""
    W = scores.numel()
    done = fin.bool()[:, None]
    raw = torch.where(done, scores.float()[:, None], scores.float()[:, None] + top_lp.float().gather(1, picks))
    tok = torch.where(done, torch.full_like(picks, eos), top_ix.gather(1, picks))
    L = torch.where(done, lens.long()[:, None], lens.long()[:, None] + 1).expand(W, W)
    norm = (raw * inv_lenpow.float()[L.clamp(0, inv_lenpow.numel() - 1)]).reshape(-1)
    valid = (~done | (torch.arange(W, device=scores.device)[None, :] == 0)).reshape(-1).nonzero().squeeze(1)
    order = valid[torch.sort(norm[valid], descending=True, stable=True).indices[:W]]
    parent = order // W
    new_tok = tok.reshape(-1)[order]
    new_fin = fin.bool()[parent] | ((new_tok == eos) & (eos >= 0))
    return parent, new_tok, raw.reshape(-1)[order], L.reshape(-1)[order].to(lens.dtype), new_fin


class _CtcPrefixHost:
    """The CTC prefix scorer of joint decoding for the W beams of ONE sentence as torch ops: the rule of fk_ctc_prefix_init /
    fk_ctc_prefix_score (include/franken_hip.h) in fp32 on the logits' device, for the re-forward paths of generate_beam_search.
    State: r_n / r_b [W, Tg], psi [W], last [W] (-1: the empty hypothesis, -2: one that took a label outside the classes)."""
    FLOOR = K.CTC_PREFIX_FLOOR

    def __init__(self, logits, Tg, blank, weight, eos, W, prompt_labels=()):
        T, self.C = logits.shape
        self.Tg = max(0, min(int(Tg), T))
        self.blank, self.eos = int(blank), -1 if eos is None else int(eos)
        self.w = torch.tensor(float(weight), dtype=torch.float32, device=logits.device)
        self.y = torch.log_softmax(logits[:self.Tg].float(), dim=-1)
        dev = logits.device
        self.r_n = torch.full((W, self.Tg), -math.inf, device=dev)
        self.r_b = torch.cumsum(self.y[:, self.blank], 0)[None, :].repeat(W, 1)
        self.psi = torch.zeros(W, device=dev)
        self.last = torch.full((W,), -1, dtype=torch.int64, device=dev)
        for c in prompt_labels:
            self.advance(torch.arange(W, device=dev), torch.full((W,), int(c), dtype=torch.int64, device=dev))

    def _valid(self, c):
        return (c >= 0) & (c < self.C) & (c != self.blank)

    def _phi(self, same):
        """phi [n, Tg] of n (hypothesis, label) pairs laid out like `same` [W, m]: column 0 stands for n[0] (0: the empty hypothesis)"""
        diff = torch.logaddexp(self.r_n, self.r_b)
        first = torch.where(self.last == -1, 0.0, -math.inf)[:, None, None].expand(-1, same.shape[1], 1)
        rest = torch.where(same[:, :, None], self.r_b[:, None, :-1], diff[:, None, :-1])
        return torch.cat((first, rest), dim=2)                                   # [W, m, Tg]

    def score(self, top_lp, top_id, fin=None):
        """(1 - weight) * top_lp + weight * delta for top_lp / top_id [W, k]; rows of finished beams come back as they are"""
        if self.Tg == 0:
            delta = torch.full_like(top_lp, self.FLOOR)
        else:
            ok = self._valid(top_id)
            ycol = self.y[:, torch.where(ok, top_id, 0)].permute(1, 2, 0)        # [W, k, Tg]
            ycol = torch.where(ok[:, :, None], ycol, -math.inf)
            psi2 = torch.logsumexp(self._phi(top_id == self.last[:, None]) + ycol, dim=2)
            if self.eos >= 0:
                psi2 = torch.where(top_id == self.eos, torch.logaddexp(self.r_n[:, -1], self.r_b[:, -1])[:, None], psi2)
            good = torch.isfinite(psi2) & torch.isfinite(self.psi)[:, None]
            delta = torch.where(good, psi2 - torch.where(good, self.psi[:, None], 0.0), self.FLOOR)
        out = (1.0 - self.w) * top_lp.float() + self.w * delta
        return out if fin is None else torch.where(fin.bool()[:, None], top_lp.float(), out)

    def advance(self, parent, tok):
        """row b becomes extend(state of row parent[b], tok[b])"""
        r_n, r_b, last = self.r_n[parent], self.r_b[parent], self.last[parent]
        ok = self._valid(tok)
        self.r_n, self.r_b, self.last = r_n, r_b, last                           # _phi reads the parents' states
        phi = self._phi((tok == last)[:, None])[:, 0]                            # [W, Tg]
        y = torch.where(ok[:, None], self.y[:, torch.where(ok, tok, 0)].t(), -math.inf)
        n, b = torch.full_like(r_n, -math.inf), torch.full_like(r_b, -math.inf)
        if self.Tg > 0:
            self.psi = torch.logsumexp(phi + y, dim=1)
            n_prev, b_prev = phi[:, 0] + y[:, 0], b[:, 0]
            n[:, 0] = n_prev
            for t in range(1, self.Tg):
                n_new = torch.logaddexp(n_prev, phi[:, t]) + y[:, t]
                b_prev = torch.logaddexp(n_prev, b_prev) + self.y[t, self.blank]
                n_prev = n_new
                n[:, t], b[:, t] = n_prev, b_prev
        else:
            self.psi = torch.full_like(self.psi, -math.inf)
        self.r_n, self.r_b, self.last = n, b, torch.where(ok, tok, -2)


@dataclass
class GPTConfig:
    block_size: int = 1024
    vocab_size: int = 50304
    n_layer: int = 12
    n_head: int = 12
    n_embd: int = 768
    dropout: float = 0.0
    bias: bool = True


class _GptEmbed(torch.autograd.Function):
    """x[b, t] = (t < t_ctx ? prefix[b, t] : wte[idx[b, t - t_ctx]]) + wpe[t]   (models/gpt2_model.py:183-196)."""

    @staticmethod
    def forward(ctx, idx, prefix, wte, wpe):
        out = K.gpt_embed_fwd(idx.contiguous(), prefix, wte.detach(), wpe.detach(), E.compute_dtype())
        ctx.t_ctx = 0 if prefix is None else prefix.shape[1]
        ctx.shapes = (wte.shape, wpe.shape)
        ctx.save_for_backward(idx)
        return out

    @staticmethod
    def backward(ctx, dx):
        (idx,) = ctx.saved_tensors
        dx = dx.contiguous()
        B, t_full, d = dx.shape
        t_ctx = ctx.t_ctx
        dprefix = None
        if t_ctx:
            dprefix = torch.empty((B, t_ctx, d), dtype=dx.dtype, device=dx.device)
            K.copy2d(dx.view(B, t_full * d)[:, :t_ctx * d], dprefix.view(B, t_ctx * d))
        dwte = dwpe = None
        if ctx.needs_input_grad[2]:                   # frozen embeddings: no [V, d] buffer, no scatter
            dwte = torch.zeros(ctx.shapes[0], dtype=torch.float32, device=dx.device)
            K.gpt_embed_bwd_wte(idx.contiguous(), dx, dwte, t_ctx)
        if ctx.needs_input_grad[3]:
            dwpe = torch.zeros(ctx.shapes[1], dtype=torch.float32, device=dx.device)
            K.colsum(dx.view(B, t_full * d), out=dwpe.view(-1)[: t_full * d])
        return None, dprefix, dwte, dwpe


class GPT(nn.Module):
    def __init__(self, config):
        super().__init__()
        assert config.vocab_size is not None
        assert config.block_size is not None
        self.config = config
        self.transformer = nn.ModuleDict(dict(
            wte=nn.Embedding(config.vocab_size, config.n_embd),
            wpe=nn.Embedding(config.block_size, config.n_embd),
            drop=nn.Dropout(config.dropout),
            h=nn.ModuleList([Block(config) for _ in range(config.n_layer)]),
            ln_f=LayerNorm(config.n_embd, bias=config.bias),
        ))
        self.lm_head = Linear(config.n_embd, config.vocab_size, bias=False)
        self.transformer.wte.weight = self.lm_head.weight   # weight tying
        self.apply(self._init_weights)
        for pn, p in self.named_parameters():
            if pn.endswith('c_proj.weight'):
                torch.nn.init.normal_(p, mean=0.0, std=0.02 / math.sqrt(2 * config.n_layer))
        print("number of parameters: %.2fM" % (self.get_num_params() / 1e6,))

    def get_num_params(self, non_embedding=True):
        n_params = sum(p.numel() for p in self.parameters())
        if non_embedding:
            n_params -= self.transformer.wpe.weight.numel()
        return n_params

    @property
    def dtype(self) -> torch.dtype:
        return next(self.parameters()).dtype

    @property
    def device(self) -> torch.device:
        return next(self.parameters()).device

    def _init_weights(self, module):
        if isinstance(module, nn.Linear):
            torch.nn.init.normal_(module.weight, mean=0.0, std=0.02)
            if module.bias is not None:
                torch.nn.init.zeros_(module.bias)
        elif isinstance(module, nn.Embedding):
            torch.nn.init.normal_(module.weight, mean=0.0, std=0.02)

    def forward(self, idx, prefix=None, targets=None):
        t_words = idx.size(1)
        dropping = bool(self.transformer.drop.p) and self.training
        if dropping:
            E.dropout_begin(idx.device)               # this forward's masks: step word + 1, sites from 0
        if prefix is not None:
            prefix = _prep(prefix)
        x = _GptEmbed.apply(idx, prefix, self.transformer.wte.weight, self.transformer.wpe.weight)
        if dropping:                                  # transformer.drop(tok_emb + pos_emb), models/gpt2_model.py:190
            x = E.Dropout.apply(x, E.drop_spec(self.transformer.drop.p, x.device, 1))
        for block in self.transformer.h:
            x = block(x)
        x = _prep(x[:, -t_words:])            # keep only the text positions (strided-copy kernel)
        ln = self.transformer.ln_f
        if targets is not None:
            # CE(logits[:, :-1], targets[:, 1:], ignore_index=-100) == CE over all rows with the targets shifted
            # left and the last position ignored (ignored rows contribute nothing to the mean)
            shifted = torch.full_like(targets, -100)
            shifted[:, :-1] = targets[:, 1:]
            if getattr(self, "fuse_head_loss", False):
                # the caller only wants the loss (train_utils.enable_fused_head_loss): the [B, t, 50257] logits are never materialised
                loss = E.head_cross_entropy(x, ln.weight, ln.bias, self.lm_head.weight, None, shifted, ln.eps, -100, getattr(self, "head_chunk", 8192))
                return loss, None
            logits = E.NormLinear.apply(x, ln.weight, ln.bias, self.lm_head.weight, None, ln.eps, False)
            loss = E.cross_entropy(logits, shifted, -100)
        else:
            last = _prep(x[:, -1:, :])
            logits = E.NormLinear.apply(last, ln.weight, ln.bias, self.lm_head.weight, None, ln.eps, False)
            loss = None
        return loss, logits

    @torch.no_grad()
    def _nbest_packed(self, ids, lengths, prefix, am_scores, bos_token_id, eos_token_id, max_nodes, am_weight=1.0, lm_weight=1.0, length_bonus=0.0):
        """The one route of score_nbest and rescore_nbest: trie -> ancestor mask -> packed forward -> head statistics -> scores and ranking
        (csrc/rescore.hip; semantics in include/franken_hip.h) -> (lm in input order, n_nodes, the ranked outputs)."""
        cfg = self.config
        if ids.dim() != 3 or ids.dtype != torch.int64:
            raise ValueError(f"ids must be int64 [B, n, T], got {ids.dtype} {tuple(ids.shape)}")
        B, n, T = ids.shape
        if not 1 <= n <= K.NBEST_MAX_HYPS or not 1 <= T <= K.NBEST_MAX_T:
            raise ValueError(f"n = {n} hypotheses of T = {T} tokens outside the envelope (1 .. {K.NBEST_MAX_HYPS}, 1 .. {K.NBEST_MAX_T})")
        P = 0 if prefix is None else prefix.shape[1]
        if P + 1 + T > cfg.block_size:
            raise ValueError(f"prefix ({P}) + start token + T ({T}) exceeds block_size = {cfg.block_size}")
        V = cfg.vocab_size
        bos = int(bos_token_id)
        eos = None if eos_token_id is None else int(eos_token_id)
        if not 0 <= bos < V or (eos is not None and not 0 <= eos < V):
            raise ValueError(f"bos_token_id {bos} / eos_token_id {eos} outside the vocabulary of {V}")
        if ids.stride(2) != 1:
            ids = ids.contiguous()
        lengths = lengths.to(torch.int64).contiguous()
        am = None if am_scores is None else am_scores.float().contiguous()
        if prefix is not None:
            prefix = _prep(prefix)
        if max_nodes is None:                               # the worst case (index arrays only), then ONE host read sizes the forward
            nmax = int(K.nbest_trie(ids, lengths, am, V, bos, eos, 1 + n * T, P, heads=False).n_nodes.max())
            N = (P + nmax + 7) // 8 * 8 - P                 # whole 8-row groups for the GEMMs
        else:
            N = int(max_nodes)
        if N < 1 or P + N > K.NBEST_MAX_ROWS:
            raise ValueError(f"{N} node rows behind {P} prefix rows outside the envelope (N >= 1, P + N <= {K.NBEST_MAX_ROWS})")
        trie = K.nbest_trie(ids, lengths, am, V, bos, eos, N, P)
        mask = K.nbest_trie_mask(trie.parent, trie.n_nodes, P)
        x = K.gpt_embed_pos(trie.tok, trie.depth, prefix, self.transformer.wte.weight.detach(), self.transformer.wpe.weight.detach(), E.compute_dtype())
        for block in self.transformer.h:
            x = block(x, mask)
        ln = self.transformer.ln_f
        rows = K.gather_rows(_prep(x), trie.head_src)        # [B, N - 1 + n, d]: every head row's hidden row
        h, _, _ = K.norm_fwd(rows.view(-1, rows.shape[-1]), ln.weight.detach(), None if ln.bias is None else ln.bias.detach(), ln.eps)
        vec = 8 if h.dtype == torch.bfloat16 else 4
        wsh = E.shadow([self.lm_head.weight], pad_n=(V + vec - 1) // vec * vec)
        stats = K.head_ce_stats(h, wsh, None, trie.head_tgt.view(-1), V)
        lm, ranked = K.nbest_rescore(stats, trie, ids, lengths, am, eos is not None, float(am_weight), float(lm_weight), float(length_bonus))
        return lm, trie.n_nodes, ranked

    @torch.no_grad()
    def score_nbest(self, ids, lengths, prefix=None, am_scores=None, bos_token_id=50256, eos_token_id=None, max_nodes=None):
        """Log-probability of every hypothesis of every sentence's n-best list under this model: ids int64 [B, n, T] (what
        engine.ctc_beam_decode returns; entries behind a length are never read), lengths [B, n], prefix [B, P, d] or None ->
        (lm fp32 [B, n] in input order, n_nodes int32 [B]).  lm[h] = sum_j log p(ids[h, j] | prefix, bos, ids[h, :j]), plus
        log p(eos | ...) with an eos_token_id.  The hypotheses of a sentence are packed as a trie: every distinct token prefix is ONE row of
        ONE forward under an ancestor mask (exact, not an approximation), the head never forms [rows, V] logits, nothing is copied back.
        Unscored (lm = -inf): a slot whose am_scores entry is not finite (the beam search's empty slot), a token outside the vocabulary
        inside the length, or a hypothesis that does not fit max_nodes.  A length 0 with a finite score is the empty hypothesis.
        max_nodes=None: the trie is first built at the worst-case capacity 1 + n T (index arrays only, a few KB) and ONE host read of
        n_nodes.max() sizes the forward, padded up to whole 8-row groups.  max_nodes=int: that many node rows per sentence, nothing waits
        for the host (graph-capturable like the rest of the decode path); a hypothesis whose new nodes do not all fit is unscored and later
        ones are still tried.  Raises ValueError before any launch when P + 1 + T > block_size."""
        lm, n_nodes, _ = self._nbest_packed(ids, lengths, prefix, am_scores, bos_token_id, eos_token_id, max_nodes)
        return lm, n_nodes

    @torch.no_grad()
    def rescore_nbest(self, ids, lengths, scores, prefix=None, lm_weight=1.0, am_weight=1.0, length_bonus=0.0, bos_token_id=50256,
                      eos_token_id=None, max_nodes=None):
        """Re-rank an n-best list by total = am_weight * scores + lm_weight * lm + length_bonus * length (fp32), lm as in score_nbest ->
        (ids [B, n, T] padded with -100, lengths, am, lm, total, order int64 [B, n], n_scored int64 [B]), everything in the new order:
        scored hypotheses by total descending (exact ties by original index), unscored ones (lm = total = -inf) behind them in original
        order; order[b, r] is the original index of place r.  The same bits every run; arguments as score_nbest."""
        return self._nbest_packed(ids, lengths, prefix, scores, bos_token_id, eos_token_id, max_nodes, am_weight, lm_weight, length_bonus)[2]

    def crop_block_size(self, block_size):
        assert block_size <= self.config.block_size
        self.config.block_size = block_size
        self.transformer.wpe.weight = nn.Parameter(self.transformer.wpe.weight[:block_size])

    @classmethod
    def from_pretrained(cls, model_type, override_args=None):
        """Load OpenAI GPT-2 weights through HF transformers (needs network / a local HF cache)."""
        sizes = {'gpt2': (12, 12, 768), 'gpt2-medium': (24, 16, 1024), 'gpt2-large': (36, 20, 1280),
                 'gpt2-xl': (48, 25, 1600)}
        assert model_type in sizes
        override_args = override_args or {}
        assert all(k == 'dropout' for k in override_args)
        from transformers import GPT2LMHeadModel
        n_layer, n_head, n_embd = sizes[model_type]
        config = GPTConfig(block_size=1024, vocab_size=50257, n_layer=n_layer, n_head=n_head, n_embd=n_embd,
                           dropout=override_args.get('dropout', 0.0), bias=True)
        model = cls(config)
        sd = model.state_dict()
        hf = GPT2LMHeadModel.from_pretrained(model_type).state_dict()
        conv1d = ('attn.c_attn.weight', 'attn.c_proj.weight', 'mlp.c_fc.weight', 'mlp.c_proj.weight')
        with torch.no_grad():
            for k, v in hf.items():
                if k.endswith('.attn.masked_bias') or k.endswith('.attn.bias'):
                    continue
                src = v.t() if k.endswith(conv1d) else v   # HF stores Conv1D weights transposed
                assert sd[k].shape == src.shape, (k, sd[k].shape, src.shape)
                sd[k].copy_(src)
        return model

    def configure_optimizers(self, weight_decay, learning_rate, betas, device_type):
        """models/gpt2_model.py:286-310: tensors with dim() >= 2 decayed, biases and LayerNorm weights not.  device_type 'cuda' (where the
        reference picks torch's fused AdamW) with the parameters on the GPU: the arena optimizer train_step, GraphedTrainStep and
        run_train_model drive (utils.train_utils.FusedAdamW), with these two groups; otherwise torch.optim.AdamW."""
        from ..utils import train_utils as tu
        groups = tu.decay_groups(self, weight_decay)
        if device_type == 'cuda' and all(p.is_cuda for g in groups for p in g['params']):
            return tu.FusedAdamW(self, lr=learning_rate, betas=betas, param_groups=groups)
        return torch.optim.AdamW(groups, lr=learning_rate, betas=betas)

    # ------------------------------------------------------------------------------------------- low-rank adapters (LoRA)
    def _lora_linears(self, targets=LORA_TARGETS):
        """[(name relative to the model, Linear)] of the chosen targets, block by block"""
        bad = [t for t in targets if t not in LORA_TARGETS]
        if bad:
            raise ValueError(f"unknown LoRA targets {bad}: choose from {LORA_TARGETS}")
        pick = {"c_attn": lambda b: b.attn.c_attn, "attn.c_proj": lambda b: b.attn.c_proj, "c_fc": lambda b: b.mlp.c_fc,
                "mlp.c_proj": lambda b: b.mlp.c_proj}
        full = {"c_attn": "attn.c_attn", "attn.c_proj": "attn.c_proj", "c_fc": "mlp.c_fc", "mlp.c_proj": "mlp.c_proj"}
        return [(f"transformer.h.{i}.{full[t]}", pick[t](b)) for i, b in enumerate(self.transformer.h) for t in LORA_TARGETS if t in targets]

    def lora_config(self):
        """dict(rank, alpha, targets) of the live adapters, or None"""
        return getattr(self, "_lora_cfg", None)

    def add_lora(self, rank=8, alpha=16.0, targets=LORA_TARGETS):
        """Freeze the GPT and put a trainable low-rank correction on the chosen Linears of every block:
            y = x W^T + b + (alpha / rank) * (x A^T) B^T,   lora_A [rank, in] (Kaiming-uniform, as nn.Linear), lora_B [out, rank] = 0
        so a fresh adapter changes nothing.  Every other parameter of the GPT gets requires_grad = False (re-enable some before building
        the optimizer if wanted); the base state-dict keys are untouched, so load the pre-trained checkpoint first and call this after.
        The kernels take 4 <= rank <= 64 with rank % 4 == 0 (fk_lora_route)."""
        if self.lora_config() is not None:
            raise RuntimeError("the model already has adapters: merge_lora() first")
        if not (4 <= rank <= 64 and rank % 4 == 0):
            raise ValueError(f"LoRA rank {rank} outside the kernels' envelope: 4 <= rank <= 64, rank % 4 == 0")
        for p in self.parameters():
            p.requires_grad_(False)
        for _, lin in self._lora_linears(targets):
            w = lin.weight
            a = torch.empty((rank, w.shape[1]), dtype=torch.float32, device=w.device)
            nn.init.kaiming_uniform_(a, a=math.sqrt(5))
            lin.lora_A = nn.Parameter(a)
            lin.lora_B = nn.Parameter(torch.zeros((w.shape[0], rank), dtype=torch.float32, device=w.device))
            lin.lora_scale = float(alpha) / rank
        self._lora_cfg = dict(rank=int(rank), alpha=float(alpha), targets=tuple(t for t in LORA_TARGETS if t in targets))
        return self

    @torch.no_grad()
    def merge_lora(self):
        """Fold the adapters into the fp32 masters (fk_lora_merge, in place), remove them and bump the weight epoch: the state dict has
        exactly the reference's keys again.  Parameters stay frozen as they are."""
        cfg = self.lora_config()
        if cfg is None:
            return self
        for _, lin in self._lora_linears(cfg["targets"]):
            K.lora_merge(lin.weight.data, lin.lora_A.data.contiguous(), lin.lora_B.data.contiguous(), lin.lora_scale, out=lin.weight.data)
            del lin.lora_A, lin.lora_B, lin.lora_scale
        self._lora_cfg = None
        E.bump_weight_epoch()
        return self

    def lora_state_dict(self):
        """{'<linear>.lora_A' / '<linear>.lora_B': tensor} of the adapters alone"""
        cfg = self.lora_config()
        out = {}
        for name, lin in (self._lora_linears(cfg["targets"]) if cfg else ()):
            out[name + ".lora_A"] = lin.lora_A.detach()
            out[name + ".lora_B"] = lin.lora_B.detach()
        return out

    @torch.no_grad()
    def load_lora_state_dict(self, sd):
        """copy adapters saved by lora_state_dict into this model's (add_lora with the same rank and targets first)"""
        own = self.lora_state_dict()
        if set(own) != set(sd):
            raise KeyError(f"adapter keys differ: missing {sorted(set(own) - set(sd))}, unexpected {sorted(set(sd) - set(own))}")
        for k, v in own.items():
            if tuple(v.shape) != tuple(sd[k].shape):
                raise ValueError(f"{k}: shape {tuple(sd[k].shape)} does not fit {tuple(v.shape)}")
            v.copy_(sd[k].to(v.device, v.dtype))
        E.bump_weight_epoch()

    def estimate_mfu(self, fwdbwd_per_iter, dt, peak_flops=2.5e15):
        """model flops utilisation vs the MI355X dense bf16 MFMA peak (the reference hard-codes A100 312 TF)."""
        N = self.get_num_params()
        cfg = self.config
        L, H, Q, T = cfg.n_layer, cfg.n_head, cfg.n_embd // cfg.n_head, cfg.block_size
        flops_per_iter = (6 * N + 12 * L * H * Q * T) * T * fwdbwd_per_iter
        return flops_per_iter / dt / peak_flops

    @torch.no_grad()
    def _cached_logits(self, idx_new, cache, pos, prefix=None):
        """last-position logits [B, V] after feeding prefix (first call only) + idx_new [B, t] at positions pos..; updates cache."""
        wte, wpe = self.transformer.wte.weight, self.transformer.wpe.weight
        x = K.gpt_embed_fwd(idx_new.contiguous(), prefix, wte.detach(), wpe.detach()[pos:], E.compute_dtype())
        t = x.shape[1]
        for li, block in enumerate(self.transformer.h):
            x = block.forward_cached(x, cache[li], pos)
        ln = self.transformer.ln_f
        last = x[:, -1, :].contiguous()
        logits = _step_linear(last, self.lm_head, ln=ln, step_rows=x.shape[0] * t, head_vocab=self.config.vocab_size)
        return logits, pos + t

    @torch.no_grad()
    def _decode_logits_dev(self, cur, cache, pos, anc=None, groups=None):
        """last-position logits [B, V] for the tokens `cur` [B] at device position pos (int32[1]); appends to the caches.
        anc: the beam ancestry table of a cached beam search, groups: its number of sentences (Block.forward_decode)."""
        x = K.gpt_embed_step(cur, self.transformer.wte.weight.detach(), self.transformer.wpe.weight.detach(), pos, E.compute_dtype())
        for li, block in enumerate(self.transformer.h):
            x = block.forward_decode(x, cache[li], pos, anc, groups)
        return _step_linear(x, self.lm_head, ln=self.transformer.ln_f, head_vocab=self.config.vocab_size)

    @staticmethod
    def _check_top_p(top_p):
        """None or 1.0: no nucleus crop (None comes back and the calls are those without the argument); otherwise a float in (0, 1)"""
        if top_p is None:
            return None
        if not 0.0 < float(top_p) <= 1.0:                               # NaN fails both comparisons
            raise ValueError(f"top_p must lie in (0, 1], got {top_p}")
        return None if float(top_p) >= 1.0 else float(top_p)

    @staticmethod
    def _check_logit_rules(repetition_penalty, no_repeat_ngram_size, min_new_tokens, eos_token_id, vocab_size, total_len, keep):
        """The arguments of the history rules (_apply_logit_rules), checked before any GPU work.  All three at their defaults: None comes back
        and the calls are those without them; otherwise the keyword arguments of _apply_logit_rules.  repetition_penalty must be finite and
        > 0, the other two integers >= 0, min_new_tokens needs an eos_token_id, and since the rules can remove at most total_len + 1 tokens
        (total_len = prompt + new tokens) the vocabulary must keep `keep` (the top-k of the draw) candidates: V - (total_len + 1) >= keep."""
        try:
            p = float(repetition_penalty)
        except (TypeError, ValueError):
            raise ValueError(f"repetition_penalty must be a finite number > 0, got {repetition_penalty!r}") from None
        if not (math.isfinite(p) and p > 0.0):
            raise ValueError(f"repetition_penalty must be a finite number > 0, got {repetition_penalty!r}")
        for name, v in (("no_repeat_ngram_size", no_repeat_ngram_size), ("min_new_tokens", min_new_tokens)):
            if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 0:
                raise ValueError(f"{name} must be an integer >= 0, got {v!r}")
        n, m = int(no_repeat_ngram_size), int(min_new_tokens)
        if m > 0 and eos_token_id is None:
            raise ValueError("min_new_tokens needs an eos_token_id: it keeps that token from being emitted")
        if p == 1.0 and n == 0 and m == 0:
            return None
        if vocab_size - (int(total_len) + 1) < max(int(keep), 1):
            raise ValueError(f"the rules can remove up to {int(total_len) + 1} tokens of a vocabulary of {vocab_size}: fewer than {max(int(keep), 1)} candidates may be left")
        return dict(repetition_penalty=p, no_repeat_ngram_size=n, min_new_tokens=m, eos_token_id=None if eos_token_id is None else int(eos_token_id))

    @staticmethod
    def _check_ctc(ctc_logits, ctc_weight, ctc_blank, ctc_input_lengths, ctc_from_prompt, idx):
        """The arguments of joint CTC / attention decoding, checked before any GPU work.  Off (no logits, or weight 0): None comes back and the
        calls are those without them; otherwise dict(logits [S, T, C] with unit column stride, weight, blank, lengths int64 [S] or None,
        from_prompt).  0 <= ctc_weight <= 1, the logits [S, T, C] ([T, C] with one sentence) in fp32 or bf16 with C >= 2, 0 <= blank < C,
        ctc_input_lengths one integer per sentence, 0 <= ctc_from_prompt <= the prompt's length."""
        try:
            w = float(ctc_weight)
        except (TypeError, ValueError):
            raise ValueError(f"ctc_weight must be a number in [0, 1], got {ctc_weight!r}") from None
        if not 0.0 <= w <= 1.0:                                          # NaN fails both comparisons
            raise ValueError(f"ctc_weight must lie in [0, 1], got {ctc_weight!r}")
        if ctc_logits is None:
            if w != 0.0:
                raise ValueError("ctc_weight > 0 needs ctc_logits")
            return None
        S, t0 = idx.shape
        lg = ctc_logits[None] if ctc_logits.dim() == 2 else ctc_logits
        if lg.dim() != 3 or lg.shape[0] != S or lg.shape[1] < 1 or lg.shape[2] < 2:
            raise ValueError(f"ctc_logits must be [S = {S}, T >= 1, C >= 2] (or [T, C] for one sentence), got {tuple(ctc_logits.shape)}")
        if lg.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"ctc_logits must be fp32 or bf16, got {lg.dtype}")
        Cn = lg.shape[2]
        blank = Cn - 1 if ctc_blank is None else ctc_blank
        if isinstance(blank, bool) or not isinstance(blank, numbers.Integral) or not 0 <= blank < Cn:
            raise ValueError(f"ctc_blank must be a class in [0, {Cn}), got {ctc_blank!r}")
        if isinstance(ctc_from_prompt, bool) or not isinstance(ctc_from_prompt, numbers.Integral) or not 0 <= ctc_from_prompt <= t0:
            raise ValueError(f"ctc_from_prompt must be an integer in [0, {t0}] (the prompt's length), got {ctc_from_prompt!r}")
        lengths = ctc_input_lengths
        if lengths is not None:
            lengths = torch.as_tensor(lengths)
            if lengths.dim() != 1 or lengths.numel() != S or lengths.dtype.is_floating_point or lengths.dtype == torch.bool:
                raise ValueError(f"ctc_input_lengths must hold one integer per sentence ({S}), got {tuple(lengths.shape)} {lengths.dtype}")
            lengths = lengths.to(device=lg.device, dtype=torch.int64)
        if w == 0.0:
            return None
        return dict(logits=lg if lg.stride(2) == 1 else lg.contiguous(), weight=w, blank=int(blank), lengths=lengths, from_prompt=int(ctc_from_prompt))

    @staticmethod
    def _ctc_kwargs_of(ctc, g):
        """the ctc_* arguments of generate_beam_search for sentence g alone"""
        return dict(ctc_logits=ctc["logits"][g:g + 1], ctc_weight=ctc["weight"], ctc_blank=ctc["blank"], ctc_from_prompt=ctc["from_prompt"],
                    ctc_input_lengths=None if ctc["lengths"] is None else ctc["lengths"][g:g + 1])

    @staticmethod
    def _ctc_host(ctc, g, idx, W, eos):
        """the torch form of the prefix scorer (_CtcPrefixHost) for the W beams of sentence g, advanced by the prompt's labels"""
        lg = ctc["logits"][g]
        P = ctc["from_prompt"]
        return _CtcPrefixHost(lg, lg.shape[0] if ctc["lengths"] is None else int(ctc["lengths"][g]), ctc["blank"], ctc["weight"], eos, W,
                              idx[g, idx.shape[1] - P:].tolist() if P else ())

    @staticmethod
    def _gumbel_picks(top_lp, W):
        """W entries per row without replacement with probability ~ exp(top_lp), by Gumbel keys like fk_beam_select (torch.multinomial refuses
        rows with fewer than W entries of non-zero probability, which the finite floor of the CTC term can produce) -> int64 [rows, W]"""
        u = torch.rand(top_lp.shape, device=top_lp.device).clamp_(1e-7, 1.0 - 1e-7)
        return (top_lp.float() - torch.log(-torch.log(u))).topk(W, dim=1).indices

    @staticmethod
    def _device_rules(rules, prompt, steps, width=None):
        """the device-side state (K.LogitRules) of the checked rules `rules` (_check_logit_rules), or None"""
        if rules is None:
            return None
        if prompt.shape[1] + steps > K.LOGIT_RULES_MAX_HISTORY:
            raise ValueError(f"the history rules on the caches hold up to {K.LOGIT_RULES_MAX_HISTORY} tokens per row, got {prompt.shape[1] + steps}")
        return K.LogitRules(prompt, steps, rules["repetition_penalty"], rules["no_repeat_ngram_size"], rules["min_new_tokens"], rules["eos_token_id"], width)

    @staticmethod
    def _apply_logit_rules(logits, history, generated, repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, eos_token_id=None):
        """The rules that depend on the tokens already emitted, as torch ops (the restatement of fk_logit_rules, include/franken_hip.h, bit for
        bit): logits fp32 [B, V], history int [B, L] (prompt ids, then the generated tokens; the brain prefix is not part of it), generated =
        the number of generated tokens.  In this order, before the temperature:
        1. every distinct in-range token v of the history except the end-of-text id: z[v] = z[v] * (1 / p) if z[v] > 0 else z[v] * p, one fp32
           multiply with 1 / p rounded once from float64; 2. with n = no_repeat_ngram_size >= 1 and L >= n, every token that would complete
           an n-gram the history already holds (its last n - 1 tokens, followed by that token) becomes -inf, except the end-of-text id;
        3. while generated < min_new_tokens the end-of-text id is -inf.  A banned token is -inf whatever 1 made of it; ids outside [0, V)
        are ignored.  The end-of-text id is exempt from 1 and 2, unlike the usual implementations: Franky's prompt is that marker itself, and
        penalising it would push every sentence away from ending.  Defaults: the input comes back as it is."""
        p, n, m = float(repetition_penalty), int(no_repeat_ngram_size), int(min_new_tokens)
        if p == 1.0 and n == 0 and m == 0:
            return logits
        z = logits.float().clone()
        B, V = z.shape
        e = -1 if eos_token_id is None else int(eos_token_id)
        h = history.long().to(z.device)
        L = h.shape[1]
        ok = (h >= 0) & (h < V) & (h != e)                              # the positions whose token a rule may touch
        at = torch.where(ok, h, torch.full_like(h, V))                  # everything else lands in a column behind the row
        if p != 1.0 and L > 0:
            pf, inv = (torch.tensor(x, dtype=torch.float32, device=z.device) for x in K.inv_penalty(p))
            seen = torch.zeros((B, V + 1), dtype=torch.bool, device=z.device).scatter_(1, at, True)[:, :V]
            z = torch.where(seen, torch.where(z > 0, z * inv, z * pf), z)
        if n >= 1 and L >= n:
            match = torch.ones((B, L - n + 1), dtype=torch.bool, device=z.device)
            if n > 1:                                                   # window j = h[j .. j+n-2] against the last n - 1 tokens, j = 0 .. L - n
                match = (h.unfold(1, n - 1, 1)[:, :L - n + 1] == h[:, None, L - n + 1:]).all(-1)
            hit = torch.where(match, at[:, n - 1:], torch.full_like(at[:, n - 1:], V))
            banned = torch.zeros((B, V + 1), dtype=torch.bool, device=z.device).scatter_(1, hit, True)[:, :V]
            z = z.masked_fill(banned, -float('Inf'))
        if generated < m and 0 <= e < V:
            z[:, e] = -float('Inf')
        return z

    @staticmethod
    def _sample(logits, temperature, top_k, state=None, top_p=None, rules=None, history=None, generated=0):
        """temperature -> top-k crop -> [nucleus crop] -> softmax -> multinomial (models/gpt2_model.py:340-351).  On the device this is ONE
        launch (fk_sample_topk or, with top_p, fk_sample_topp; Philox keyed by a seed drawn from torch's generator); the torch-op form is
        kept for host tensors.  top_p: of the tokens the top-k crop keeps, token i stays iff the tokens with a strictly larger logit hold
        less than top_p of the kept probability (include/franken_hip.h, fk_sample_topp).
        rules (the dict _check_logit_rules returns, or None) with history [B, L] and generated: those rules run first, as torch ops (the
        paths whose token ids the Python loop holds; the cached paths run fk_logit_rules instead and pass no rules here)."""
        top_p = GPT._check_top_p(top_p)
        if rules is not None:
            logits = GPT._apply_logit_rules(logits, history, generated, **rules)
        if logits.is_cuda:
            lg = logits.float()
            lg = lg if lg.stride(-1) == 1 else lg.contiguous()
            st = state if state is not None else K.SampleState(logits.device)
            if top_p is not None:
                return K.sample_topp(lg, temperature, top_k, top_p, st).view(-1, 1).clone()
            return K.sample_topk(lg, temperature, top_k, st).view(-1, 1).clone()
        logits = logits.float() / temperature
        if top_k is not None:
            v, _ = torch.topk(logits, min(top_k, logits.size(-1)))
            logits = logits.masked_fill(logits < v[:, -1:], -float('Inf'))
        if top_p is not None:
            v, _ = torch.sort(logits, dim=-1, descending=True)
            p = torch.softmax(v, dim=-1)
            kept = ((p.cumsum(-1) - p) < top_p).sum(-1, keepdim=True)   # exclusive sum: at the first of equal values it is mass_gt, and the kept ones are a prefix
            logits = logits.masked_fill(logits < v.gather(-1, kept - 1), -float('Inf'))     # below the smallest kept value, so ties stay
        return torch.multinomial(torch.softmax(logits, dim=-1), num_samples=1)

    @torch.no_grad()
    def generate(self, idx, max_new_tokens, prefix=None, temperature=1.0, top_k=None, use_cache=True, use_graph=None, eos_token_id=None,
                 check_every=8, top_p=None, repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0):
        """Sampling loop of the reference (models/gpt2_model.py:328-353: temperature, top-k crop, softmax, multinomial; returns
        the first sample's ids).  With use_cache (default) the prefix + prompt are run once and every new token is one
        incremental step against per-layer key/value caches; with use_graph (default: on from 64 new tokens, where the one-off
        capture has paid for itself)
        that step — embedding, blocks, head AND the sampling — reads its position from the device and is captured once as a
        hipGraph that is replayed per token (the step is launch-bound: ~25 small kernels).  When the sequence would outgrow
        block_size the reference's crop-and-re-forward path is used instead.
        eos_token_id: a row that draws this id is done: it emits the id from then on and draws nothing (its tokens up to and including
        the id are the ones the call without it draws from the same seed); the loop asks the device every `check_every` steps whether any
        row is still live and stops early if none is.  Returns row 0 at full length, padded with the id, and sets last_tokens
        [B, t0 + max_new_tokens], last_lengths [B] (generated tokens, the id counted once) and last_steps (steps run).
        top_p: nucleus sampling behind the top-k crop, on every path: of the tokens the crop keeps, the smallest set of most likely ones whose
        probability reaches top_p stays (ties with its last member stay too; _sample has the rule).  None or 1.0: off, the calls and the
        tokens of a torch seed are those without it; outside (0, 1] raises.
        repetition_penalty / no_repeat_ngram_size / min_new_tokens: rules on the tokens already emitted (prompt and generated; not the
        prefix), applied to the logits before the temperature on every path (_apply_logit_rules has the rule; on the caches it is one more
        launch, K.logit_rules_, which keeps the history on the device): seen tokens are penalised once, a token that would repeat an n-gram
        of that size is never emitted, and the end-of-text id is never emitted among the first min_new_tokens.  The end-of-text id is
        exempt from the first two, a deliberate departure from the usual implementations: Franky's prompt is that marker itself.  On the
        caches a row's history (prompt + new tokens) holds up to 4096 tokens (K.LOGIT_RULES_MAX_HISTORY); a longer one raises ValueError
        before any GPU work.  All three at their defaults: off, the calls and the tokens are those without them."""
        top_p = self._check_top_p(top_p)
        B, t0 = idx.shape
        rules = self._check_logit_rules(repetition_penalty, no_repeat_ngram_size, min_new_tokens, eos_token_id, self.config.vocab_size,
                                        t0 + max_new_tokens, top_k or 1)
        t_ctx = 0 if prefix is None else prefix.shape[1]
        total = t_ctx + t0 + max_new_tokens
        cached = use_cache and total <= self.config.block_size and max_new_tokens > 0
        if use_graph is None:
            use_graph = max_new_tokens >= 64
        if eos_token_id is not None:
            return self._generate_eos(idx, max_new_tokens, prefix, temperature, top_k, cached, use_graph, int(eos_token_id), int(check_every), top_p, rules)
        state = K.SampleState(idx.device) if idx.is_cuda else None      # one Philox stream per call, seeded from torch's generator
        if cached and use_graph and idx.is_cuda:                        # _generate_dev draws its own seed BEHIND this one: keep both, or the tokens of a torch seed move
            return self._generate_dev(idx, max_new_tokens, prefix, temperature, top_k, True, top_p=top_p, rules=rules)
        dev_rules = self._device_rules(rules, idx, max_new_tokens) if cached and idx.is_cuda else None      # refuses before the prefill runs
        if cached:
            d = self.config.n_embd
            cache = [torch.empty((B, total, 2 * d), dtype=E.compute_dtype(), device=idx.device) for _ in self.transformer.h]
            logits, pos = self._cached_logits(idx, cache, 0, None if prefix is None else _prep(prefix))
        for it in range(max_new_tokens):
            if cached:
                if it > 0:
                    logits, pos = self._cached_logits(idx[:, -1:], cache, pos)
            else:
                idx_cond = idx if idx.size(1) <= self.config.block_size else idx[:, -self.config.block_size:]
                _, lg = self(idx_cond, prefix=prefix)
                logits = lg[:, -1, :]
            if dev_rules is not None:                                   # the sampler advances state.step, which counts the generated tokens
                logits = logits.float()
                logits = K.logit_rules_(logits if logits.stride(-1) == 1 else logits.contiguous(), dev_rules, state.step, idx[:, -1].contiguous())
                tok = self._sample(logits, temperature, top_k, state, top_p)
            else:
                tok = self._sample(logits, temperature, top_k, state, top_p, rules, idx, it)
            idx = torch.cat((idx, tok), dim=1)
        return idx[0]

    @staticmethod
    def _run_steps(step, max_new_tokens, use_graph, live=None, check_every=None):
        """Steps 2 .. max_new_tokens of a decode loop whose first step the caller has run: eager on the current stream, or (use_graph) on a
        side stream two eager warm-up steps, one capture and replays.  live (int32 [1], written by the step): before a step, after every
        `check_every`-th one, it is read with one 4-byte copy and the loop ends when it is 0; None: never asked, all steps run.
        -> the number of steps run, the first included."""
        n = 1

        def stopped():                                      # asked before a step: every check_every-th step is followed by one read
            return live is not None and n % check_every == 0 and int(live.item()) == 0

        if not (use_graph and max_new_tokens > 1):
            while n < max_new_tokens and not stopped():
                step()
                n += 1
            return n
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            warm = 1 + min(2, max_new_tokens - 1)           # warm-up (allocator, lazy shadows) before the capture
            stop = False
            while n < warm and not stop:
                stop = stopped()
                if not stop:
                    step()
                    n += 1
            if not stop and n < max_new_tokens:
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=side):      # records the step, does not run it
                    step()
                while n < max_new_tokens and not stopped():
                    graph.replay()
                    n += 1
        torch.cuda.current_stream().wait_stream(side)
        return n

    @torch.no_grad()
    def _generate_dev(self, idx, max_new_tokens, prefix, temperature, top_k, use_graph, eos=None, check_every=None, top_p=None, rules=None):
        """generate on the caches with the position on the device: prefill, then a step that is embed -> blocks -> head -> one sampling
        launch, which writes cur / out[:, step] and advances both the step counter and `pos` (_run_steps).  eos: K.sample_topk_eos is
        that launch (done rows, lengths and the live count live on the device) and last_tokens / last_lengths / last_steps are set.
        top_p (a float below 1, or None): K.sample_topp is that launch, with or without eos.
        rules (_check_logit_rules): K.logit_rules_ runs in front of that launch, on the prefill logits and inside the step; it reads the step
        counter of the sampler and its `cur`, so it records into the captured step like everything else."""
        (B, t0), dev, d = idx.shape, idx.device, self.config.n_embd
        lr = self._device_rules(rules, idx, max_new_tokens)
        t_ctx = 0 if prefix is None else prefix.shape[1]
        cache = [torch.empty((B, t_ctx + t0 + max_new_tokens, 2 * d), dtype=E.compute_dtype(), device=dev) for _ in self.transformer.h]
        logits0, pos0 = self._cached_logits(idx, cache, 0, None if prefix is None else _prep(prefix))
        if eos is None:
            out = torch.empty((B, max_new_tokens), dtype=torch.int64, device=dev)
        else:
            out = torch.full((B, max_new_tokens), eos, dtype=torch.int64, device=dev)
        cur = torch.empty(B, dtype=torch.int64, device=dev)
        state = K.SampleState(dev)                       # step counter = the column of `out` the next token goes to
        es = None if eos is None else K.SampleEosState(dev, B, eos)

        def sample(logits, pos_inc=None):
            if lr is not None:
                K.logit_rules_(logits, lr, state.step, cur)
            if top_p is not None:
                K.sample_topp(logits, temperature, top_k, top_p, state, es, cur=cur, out=out, pos_inc=pos_inc)
            elif es is None:
                K.sample_topk(logits, temperature, top_k, state, cur=cur, out=out, pos_inc=pos_inc)
            else:
                K.sample_topk_eos(logits, temperature, top_k, state, es, cur=cur, out=out, pos_inc=pos_inc)

        lg0 = logits0.float()
        sample(lg0 if lg0.stride(-1) == 1 else lg0.contiguous())
        pos = torch.tensor([pos0], dtype=torch.int32, device=dev)
        steps = self._run_steps(lambda: sample(self._decode_logits_dev(cur, cache, pos), pos), max_new_tokens, use_graph,
                                None if es is None else es.live, check_every)
        tokens = torch.cat((idx, out), dim=1)
        if es is not None:
            self.last_steps, self.last_tokens, self.last_lengths = steps, tokens, es.len.to(torch.int64)
        return tokens[0]

    @torch.no_grad()
    def _generate_eos(self, idx, max_new_tokens, prefix, temperature, top_k, cached, use_graph, eos, check_every, top_p=None, rules=None):
        """generate with an end-of-text id.  On the caches it is _generate_dev; the re-forward loop applies the same rule with torch.where
        on the host."""
        assert 0 <= eos < self.config.vocab_size, f"eos_token_id {eos} outside the vocabulary"
        assert check_every >= 1
        B, dev = idx.shape[0], idx.device
        if cached and idx.is_cuda:
            return self._generate_dev(idx, max_new_tokens, prefix, temperature, top_k, use_graph, eos, check_every, top_p, rules)
        state = K.SampleState(dev) if idx.is_cuda else None
        done = torch.zeros(B, dtype=torch.bool, device=dev)
        lens = torch.zeros(B, dtype=torch.int64, device=dev)
        n = 0
        while n < max_new_tokens:
            if n > 0 and n % check_every == 0 and bool(done.all()):
                break
            idx_cond = idx if idx.size(1) <= self.config.block_size else idx[:, -self.config.block_size:]
            _, lg = self(idx_cond, prefix=prefix)
            tok = torch.where(done, torch.full_like(lens, eos), self._sample(lg[:, -1, :], temperature, top_k, state, top_p, rules, idx, n).view(-1))
            lens += (~done).long()
            done = done | (tok == eos)
            idx = torch.cat((idx, tok[:, None]), dim=1)
            n += 1
        pad = torch.full((B, max_new_tokens - n), eos, dtype=idx.dtype, device=dev)
        self.last_steps, self.last_tokens, self.last_lengths = n, torch.cat((idx, pad), dim=1), lens
        return self.last_tokens[0]

    @torch.no_grad()
    def generate_beam_search(self, idx, max_new_tokens, prefix, temperature=1.0, topk=20, beam_width=5, use_cache=False, use_graph=None, seeds=None,
                             eos_token_id=None, length_penalty=0.0, check_every=8, repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0,
                             ctc_logits=None, ctc_weight=0.0, ctc_blank=None, ctc_input_lengths=None, ctc_from_prompt=0):
        """Stochastic beam search of the reference (models/gpt2_model.py:355-416): every step each of the `beam_width` beams draws
        `beam_width` continuations WITHOUT replacement from its `topk` most likely tokens, the `beam_width` best-scoring
        (cumulative log-probability) of the beam_width^2 candidates survive; returns the best beam's ids.
        idx [1, t0] is the reference's call and returns the 1-D ids; idx [S, t0] with prefix [S, t_ctx, d] searches S sentences (prompts of
        equal length), each with its own beams, and returns [S, t0 + max_new_tokens].
        Default: host-side bookkeeping around the kernel forward (one batched forward of all beams per step, torch.multinomial draws).
        use_cache=True: the prefix and the prompt run once, every step is one cached decode step of all beams with the draw, the
        selection and the bookkeeping on the device (_beam_search_cached; its draws are a Philox stream seeded from torch's generator,
        not torch.multinomial's); S > 1 sentences share that step (S * beam_width rows, one Philox key per sentence, `seeds` = S ints
        fixes them).  Outside its envelope (sequence longer than block_size, beam_width > 16, topk > 64 or > vocabulary, host tensors)
        the call takes the re-forward loop, sentence by sentence.
        eos_token_id / length_penalty (alpha): a beam that has emitted the id is finished: it stays a candidate with its score and its
        length and draws nothing more; candidates and final beams are ranked by score / length^alpha (length = generated tokens, the id
        counted once); the search stops once every beam of every sentence is finished, which the host asks the device every `check_every`
        steps.  The result is padded with the id to t0 + max_new_tokens; last_beams / last_beam_scores (raw sums) are ordered best
        first, last_beam_lengths and last_steps are set as well.  Both arguments at their defaults: the search above, unchanged.
        repetition_penalty / no_repeat_ngram_size / min_new_tokens: the rules of generate (_apply_logit_rules) on every beam's own history,
        applied to its logits before the temperature and the log-softmax; the end-of-text id is exempt from the first two (a deliberate
        departure from the usual implementations).  On the caches it is one more launch in front of K.beam_topk, which also carries the
        histories along with the beams (K.logit_rules_).  All three at their defaults: off, the calls are those without them.
        ctc_logits / ctc_weight: one-pass joint CTC / attention decoding.  ctc_logits [S, T, C] (or [T, C] for one sentence; fp32 / bf16, NOT
        log-softmaxed) are the frames of a frame-synchronous CTC head over the same token ids; every candidate c of every beam h is then
        ranked by (1 - ctc_weight) * log p(c | h) + ctc_weight * (psi(h c) - psi(h)), psi = the CTC prefix log-probability (the rule:
        fk_ctc_prefix_score in include/franken_hip.h), and the draw, the selection and the scores run on these joint values.  ctc_blank
        (default C - 1), ctc_input_lengths int64 [S] (default T each), ctc_from_prompt = P: the last P prompt tokens are labels of the CTC
        transcript too (a target that begins with the start token).  On the caches it is one launch between K.beam_topk and the select
        (K.ctc_prefix_score_; T <= 1024, P <= 64); the re-forward paths apply the same rule as torch ops (_CtcPrefixHost) and draw by
        Gumbel keys.  ctc_logits None or ctc_weight 0: off, the calls and launches are those without them."""
        if topk is None:
            topk = 2 * beam_width
        ctc = self._check_ctc(ctc_logits, ctc_weight, ctc_blank, ctc_input_lengths, ctc_from_prompt, idx)
        rules = self._check_logit_rules(repetition_penalty, no_repeat_ngram_size, min_new_tokens, eos_token_id, self.config.vocab_size,
                                        idx.shape[1] + max_new_tokens, topk)
        self.eval()
        total = (0 if prefix is None else prefix.shape[1]) + idx.shape[1] + max_new_tokens
        in_envelope = (use_cache and idx.is_cuda and max_new_tokens > 0 and total <= self.config.block_size
                       and 1 <= beam_width <= K.BEAM_MAX_WIDTH and beam_width <= topk <= min(K.BEAM_MAX_TOPK, self.config.vocab_size))
        if ctc is not None:
            in_envelope = (in_envelope and ctc["logits"].is_cuda and ctc["logits"].shape[1] <= K.CTC_PREFIX_MAX_T
                           and ctc["from_prompt"] <= K.CTC_PREFIX_MAX_PROMPT)
        eos_mode = eos_token_id is not None or length_penalty != 0.0
        eos = None if eos_token_id is None else int(eos_token_id)
        if eos_mode:
            assert eos is None or 0 <= eos < self.config.vocab_size, f"eos_token_id {eos} outside the vocabulary"
            assert check_every >= 1
            check_every = int(check_every)
        if in_envelope:
            return self._beam_search_cached(idx, max_new_tokens, prefix, temperature, topk, beam_width, use_graph, seeds, eos,
                                            float(length_penalty), check_every, eos_mode, rules, ctc)
        if eos_mode:
            return self._beam_search_host_eos(idx, max_new_tokens, prefix, temperature, topk, beam_width, eos, float(length_penalty), check_every, rules,
                                              ctc)
        S = idx.shape[0]
        if S > 1:
            kw = {} if rules is None else {k: v for k, v in rules.items() if k != "eos_token_id"}
            return torch.stack([self.generate_beam_search(idx[g:g + 1], max_new_tokens, None if prefix is None else prefix[g:g + 1], temperature,
                                                          topk, beam_width, **kw, **({} if ctc is None else self._ctc_kwargs_of(ctc, g)))
                                for g in range(S)])
        beams = idx.repeat(beam_width, 1)
        scores = torch.zeros(beam_width, device=idx.device)
        prefix = prefix.expand(beam_width, -1, -1)
        joint = None if ctc is None else self._ctc_host(ctc, 0, idx, beam_width, None)
        for it in range(max_new_tokens):
            _, logits = self(beams, prefix=prefix.contiguous())
            last = logits[:, -1, :].float()
            if rules is not None:
                last = self._apply_logit_rules(last, beams, it, **rules)
            logp = torch.log_softmax(last / temperature, dim=-1)
            top_lp, top_ix = logp.topk(topk, dim=-1)
            if joint is None:
                picks = torch.multinomial(top_lp.exp(), beam_width, replacement=False)       # [beam, beam_width] indices into top-k
            else:
                top_lp = joint.score(top_lp, top_ix)
                picks = self._gumbel_picks(top_lp, beam_width)
            cand_score = (scores[:, None] + top_lp.gather(1, picks)).reshape(-1)
            cand_tok = top_ix.gather(1, picks).reshape(-1)
            cand_beam = torch.arange(beam_width, device=idx.device).repeat_interleave(beam_width)
            order = torch.sort(cand_score, descending=True, stable=True).indices[:beam_width]
            beams = torch.cat((beams[cand_beam[order]], cand_tok[order, None]), dim=1)
            scores = cand_score[order]
            if joint is not None:
                joint.advance(cand_beam[order], cand_tok[order])
        if joint is not None:
            self.last_beams, self.last_beam_scores = beams.tolist(), scores.tolist()
        return beams[scores.argmax()]

    @torch.no_grad()
    def _beam_search_cached(self, idx, max_new_tokens, prefix, temperature, topk, W, use_graph, seeds, eos=None, alpha=0.0, check_every=None,
                            eos_mode=False, rules=None, ctc=None):
        """generate_beam_search for S >= 1 sentences on per-layer caches [S * W, total, 2d] that are never reordered: row g * W + b is beam b
        of sentence g, slot b of a sentence holds the rows its beam position b wrote, the int32 ancestry table names the slot (counted
        inside the sentence, so the sentences cannot read each other's rows) of every row of every beam, and the select kernel rewrites
        that table when it picks the survivors.  The prefix and the prompts are prefilled in one pass into the slots g * W; the first step
        draws every sentence's beams from its one row; then a step is embed -> blocks -> head -> K.beam_topk -> select.  Nothing in it
        waits for the host, so with use_graph (default: from 64 new tokens, as in generate) it is captured once and replayed (_run_steps).
        The blocks' attention is K.attn_decode_beam behind K.kv_append_ for one sentence and K.attn_decode_beam_grouped, which also appends
        the new key|value row, for more; up to 16 rows the linear layers stream the weights once (K.gemv_nt), beyond that they are MFMA
        GEMMs (_step_linear).  The select is K.beam_select (S = 1) or K.beam_select_grouped (one block per sentence; one position and one
        step counter for all), and the host walks every final beam back through the logs: last_beams (W id lists, prompt included, in
        beam order; S > 1: S such lists) and last_beam_scores are set and the best beam of every sentence is returned.
        eos_mode (an end-of-text id `eos` or a length penalty `alpha`): K.beam_select_eos is the select (one block per sentence, S = 1
        included), the live count is read every `check_every` steps, and K.beam_backtrack replaces the host's walk: the ids come back
        ranked, [S, W, t0 + max_new_tokens], padded behind the steps that ran; last_beam_lengths and last_steps are set as well.
        rules (_check_logit_rules): K.logit_rules_ runs in front of both K.beam_topk calls; it follows the parents in the log of the last
        select, so every row's history is that of the beam it now continues.
        ctc (_check_ctc): K.ctc_prefix_score_ runs between both K.beam_topk calls and their select: it follows the same log, so every row's
        CTC state is that of the beam it now continues, and rewrites top_lp with the joint values the select then draws and ranks on."""
        dev, d = idx.device, self.config.n_embd
        S, t0 = idx.shape
        lr = self._device_rules(rules, idx, max_new_tokens, width=W)
        cs = None
        if ctc is not None:
            P = ctc["from_prompt"]
            cs = K.ctc_prefix_init(ctc["logits"], W, ctc["weight"], ctc["blank"], ctc["lengths"], idx[:, t0 - P:].to(torch.int64) if P else None)
        p0 = (0 if prefix is None else prefix.shape[1]) + t0
        total = p0 + max_new_tokens
        if use_graph is None:
            use_graph = max_new_tokens >= 64
        select = K.beam_select_eos if eos_mode else K.beam_select if S == 1 else K.beam_select_grouped
        groups = None if S == 1 else S                      # one sentence: the one-sentence attention
        cache = [torch.empty((S * W, total, 2 * d), dtype=E.compute_dtype(), device=dev) for _ in self.transformer.h]
        # slot g * W <- prefix + prompt of sentence g
        logits0, _ = self._cached_logits(idx, [c[:1] if S == 1 else c[::W] for c in cache], 0, None if prefix is None else _prep(prefix))
        state = K.BeamState(dev, W, max_new_tokens, total, seed=seeds, groups=S, eos=eos, length_penalty=alpha)     # plain: no end-of-text state
        state.anc[:, :p0] = 0
        cur = torch.empty(S * W, dtype=torch.int64, device=dev)
        top_lp = torch.empty((S * W, topk), dtype=torch.float32, device=dev)
        top_id = torch.empty((S * W, topk), dtype=torch.int64, device=dev)
        lg0 = logits0.float()
        # first step: the beams of a sentence are its one prefilled sequence and draw from the same row; no row has been appended, the table stays
        lg0 = lg0 if lg0.stride(-1) == 1 else lg0.contiguous()
        if lr is not None:
            K.logit_rules_(lg0, lr, state.step, cur, state.parent_log, broadcast=True)
        K.beam_topk(lg0, temperature, topk, top_lp[:S], top_id[:S])
        if cs is not None:
            K.ctc_prefix_score_(top_lp[:S], top_id[:S], cs, state, broadcast=True)
        select(top_lp[:S], top_id[:S], state, cur, torch.tensor([-1], dtype=torch.int32, device=dev), broadcast=True)
        pos = torch.tensor([p0], dtype=torch.int32, device=dev)

        def step():
            lg = self._decode_logits_dev(cur, cache, pos, state.anc, groups=groups)
            if lr is not None:
                K.logit_rules_(lg, lr, state.step, cur, state.parent_log)
            K.beam_topk(lg, temperature, topk, top_lp, top_id)
            if cs is not None:
                K.ctc_prefix_score_(top_lp, top_id, cs, state)
            select(top_lp, top_id, state, cur, pos, pos_inc=pos)

        steps = self._run_steps(step, max_new_tokens, use_graph, state.live if eos_mode else None, check_every)
        if eos_mode:
            self.last_steps = steps
            ids = torch.empty((S, W, t0 + max_new_tokens), dtype=torch.int64, device=dev)
            ids[:, :, :t0] = idx[:, None, :]
            scores, lens = K.beam_backtrack(state, ids, t0, 0 if eos is None else eos)
            beams, scores, lens = ids.cpu().tolist(), scores.cpu().tolist(), lens.cpu().tolist()
            if S == 1:
                self.last_beams, self.last_beam_scores, self.last_beam_lengths = beams[0], scores[0], lens[0]
                return ids[0, 0].to(idx.dtype)
            self.last_beams, self.last_beam_scores, self.last_beam_lengths = beams, scores, lens
            return ids[:, 0].to(idx.dtype)
        parents, toks, scores = state.parent_log.cpu().tolist(), state.tok_log.cpu().tolist(), state.scores.cpu().view(S, W)
        prompts = idx.cpu().tolist()
        beams = [[] for _ in range(S)]
        for g in range(S):
            for b in range(W):                              # walk every final beam back through its parents (beam numbers inside the sentence)
                seq = []
                for t in range(max_new_tokens - 1, -1, -1):
                    seq.append(toks[t][g * W + b])
                    b = parents[t][g * W + b]
                beams[g].append(prompts[g] + seq[::-1])
        best = [beams[g][int(scores[g].argmax())] for g in range(S)]
        self.last_beams, self.last_beam_scores = (beams[0], scores[0].tolist()) if S == 1 else (beams, scores.tolist())
        return torch.tensor(best[0] if S == 1 else best, dtype=idx.dtype, device=dev)

    @torch.no_grad()
    def _beam_search_host_eos(self, idx, max_new_tokens, prefix, temperature, topk, W, eos, alpha, check_every, rules=None, ctc=None):
        """The re-forward loop of generate_beam_search with the end-of-text rules (_beam_step_host), sentence by sentence; draws by
        torch.multinomial.  Sets last_beams, last_beam_scores, last_beam_lengths (best first) and last_steps like the cached search."""
        S, t0 = idx.shape
        dev = idx.device
        pad_id = 0 if eos is None else eos
        table = K.inv_lenpow_table(max(max_new_tokens, 1) + 2, alpha).to(dev)
        all_beams, all_scores, all_lens, steps = [], [], [], 0
        for g in range(S):
            beams = idx[g:g + 1].repeat(W, 1)
            scores = torch.zeros(W, device=dev)
            lens = torch.zeros(W, dtype=torch.int64, device=dev)
            fin = torch.zeros(W, dtype=torch.bool, device=dev)
            pf = None if prefix is None else prefix[g:g + 1].expand(W, -1, -1).contiguous()
            joint = None if ctc is None else self._ctc_host(ctc, g, idx, W, eos)
            n = 0
            while n < max_new_tokens:
                if n > 0 and n % check_every == 0 and bool(fin.all()):
                    break
                cond = beams if beams.size(1) <= self.config.block_size else beams[:, -self.config.block_size:]
                _, logits = self(cond, prefix=pf)
                last = logits[:, -1, :].float()
                if rules is not None:
                    last = self._apply_logit_rules(last, beams, n, **rules)
                logp = torch.log_softmax(last / temperature, dim=-1)
                top_lp, top_ix = logp.topk(topk, dim=-1)
                if joint is None:
                    picks = torch.multinomial(top_lp.exp(), W, replacement=False)
                else:
                    top_lp = joint.score(top_lp, top_ix, fin)
                    picks = self._gumbel_picks(top_lp, W)
                parent, tok, scores, lens, fin = _beam_step_host(top_lp, top_ix, picks, scores, lens, fin, -1 if eos is None else eos, table)
                if joint is not None:
                    joint.advance(parent, tok)
                beams = torch.cat((beams[parent], tok[:, None]), dim=1)
                n += 1
            steps = max(steps, n)
            beams = torch.cat((beams, torch.full((W, max_new_tokens - n), pad_id, dtype=beams.dtype, device=dev)), dim=1)
            order = torch.sort(scores * table[lens.clamp(0, table.numel() - 1)], descending=True, stable=True).indices
            all_beams.append(beams[order])
            all_scores.append(scores[order].tolist())
            all_lens.append(lens[order].tolist())
        self.last_steps = steps
        if S == 1:
            self.last_beams, self.last_beam_scores, self.last_beam_lengths = all_beams[0].tolist(), all_scores[0], all_lens[0]
            return all_beams[0][0]
        self.last_beams, self.last_beam_scores, self.last_beam_lengths = [b.tolist() for b in all_beams], all_scores, all_lens
        return torch.stack([b[0] for b in all_beams])

    @torch.no_grad()
    def beam_search(self, idx, max_new_tokens, prefix, temperature=1.0, topk=20, beam_width=3, use_cache=False):
        """Deterministic beam search of the reference (models/gpt2_model.py:419-454), including its quirk: the running context
        `idx` is shared by all beams and grows by every beam's last token in turn (it is not forked per beam), so the scores are
        those of that merged sequence.  Returns the token list of the best entry [idx[0, 0], t1, t2, ...].  Batch size 1.
        use_cache=True: that one growing sequence is prefilled once and every beam entry costs one cached decode step at batch 1
        and one K.beam_topk instead of a forward of the whole context (same tokens, same scores)."""
        self.eval()
        t_ctx = 0 if prefix is None else prefix.shape[1]
        total = t_ctx + idx.shape[1] + max(0, max_new_tokens - 1) * beam_width
        cached = (use_cache and idx.is_cuda and idx.shape[0] == 1 and total <= self.config.block_size
                  and 1 <= beam_width <= min(K.BEAM_MAX_TOPK, self.config.vocab_size))
        if cached:
            dev = idx.device
            cache = [torch.empty((1, total, 2 * self.config.n_embd), dtype=E.compute_dtype(), device=dev) for _ in self.transformer.h]
            logits, p0 = self._cached_logits(idx, cache, 0, None if prefix is None else _prep(prefix))
            pos = torch.tensor([p0], dtype=torch.int32, device=dev)
            lg = logits.float()
            lp, ix = K.beam_topk(lg if lg.stride(-1) == 1 else lg.contiguous(), 1.0, beam_width)
        else:
            _, logits = self(idx, prefix=prefix)
            lp, ix = torch.topk(torch.log_softmax(logits[:, -1, :].float(), dim=-1), beam_width)
        first = idx[0, 0].item()
        beam = [(ix[0, i], lp[0, i], [first, ix[0, i].item()]) for i in range(beam_width)]
        for _ in range(max_new_tokens - 1):
            cands = []
            for last, score, toks in beam:
                if cached:
                    lp, ix = K.beam_topk(self._decode_logits_dev(last.reshape(1).clone(), cache, pos), 1.0, beam_width)
                    pos += 1
                else:
                    idx = torch.cat((idx, last.reshape(1, 1)), dim=-1)
                    _, logits = self(idx, prefix=prefix)
                    lp, ix = torch.topk(torch.log_softmax(logits[:, -1, :].float(), dim=-1), beam_width)
                for i in range(beam_width):
                    cands.append((ix[0, i], score + lp[0, i], toks + [ix[0, i].item()]))
            beam = sorted(cands, key=lambda c: float(c[1]), reverse=True)[:beam_width]
        self.last_beam_scores = [float(b[1]) for b in beam]
        return beam[0][2]
