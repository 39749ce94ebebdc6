"""Float64 restatement of the n-best rescoring (csrc/rescore.hip; semantics in include/franken_hip.h, "n-best rescoring"):

  trie()          the trie rules: validity, first-seen numbering, leaves, the overflow rule, dead nodes
  head_rows()     the rows of the vocabulary head of a packed forward
  visibility()    the [P + N, P + N] table: prefix causal, a live node sees the prefix and its ancestors-or-self, a dead node itself
  packed_lm()     the packed forward (the model's blocks under that table) and the sums along the trie
  flat_lm()       the yardstick: every hypothesis on its own through oracle.ref_models.gpt_forward (full logits, log_softmax, gather, sum)
  combine_rank()  totals and the ranking

Everything runs in the dtype of the state dict it is given (float64 for the reference, float32 for the error yardstick e32)."""
import numpy as np
import torch

from oracle import ref_models as RM

IGNORE = -100


def clamp_lengths(lengths, T):
    return np.clip(np.asarray(lengths, dtype=np.int64), 0, T)


def trie(ids, lengths, am, V, bos, node_cap):
    """one sentence: ids [n, T], lengths [n], am [n] or None -> dict(tok, depth, parent [node_cap], leaf [n], n_nodes)"""
    ids = np.asarray(ids)
    n, T = ids.shape
    lens = clamp_lengths(lengths, T)
    tok, depth, parent = [int(bos)], [0], [-1]
    children = {}
    leaf = np.full(n, -1, dtype=np.int64)
    for h in range(n):
        seq = [int(t) for t in ids[h, :lens[h]]]
        if am is not None and not np.isfinite(am[h]):
            continue
        if any(t < 0 or t >= V for t in seq):
            continue
        node, j = 0, 0
        while j < len(seq) and (node, seq[j]) in children:              # the part of the path that exists
            node = children[(node, seq[j])]
            j += 1
        if len(tok) + (len(seq) - j) > node_cap:                        # all new nodes fit, or none is made
            continue
        for t in seq[j:]:
            children[(node, t)] = len(tok)
            tok.append(t); depth.append(depth[node] + 1); parent.append(node)
            node = len(tok) - 1
        leaf[h] = node
    nn = len(tok)
    dead = node_cap - nn
    return dict(tok=np.array(tok + [int(bos)] * dead, dtype=np.int64), depth=np.array(depth + [0] * dead, dtype=np.int64),
                parent=np.array(parent + [-1] * dead, dtype=np.int64), leaf=leaf, n_nodes=nn)


def head_rows(tr, n, P, eos):
    """-> (src [N - 1 + n] hidden row of every head row, tgt [N - 1 + n] its target or -100)"""
    N = len(tr["tok"])
    nn = tr["n_nodes"]
    src = np.full(N - 1 + n, P, dtype=np.int64)
    tgt = np.full(N - 1 + n, IGNORE, dtype=np.int64)
    for i in range(1, nn):
        src[i - 1], tgt[i - 1] = P + tr["parent"][i], tr["tok"][i]
    for h in range(n):
        if tr["leaf"][h] >= 0:
            src[N - 1 + h] = P + tr["leaf"][h]
            if eos is not None:
                tgt[N - 1 + h] = eos
    return src, tgt


def visibility(tr, P, sibling_leak=False):
    """uint8 [P + N, P + N].  sibling_leak: the plain causal table over the packed rows (a node sees every earlier row), the mistake the
    cases must be sensitive to"""
    N = len(tr["tok"])
    R = P + N
    m = np.zeros((R, R), dtype=np.uint8)
    for q in range(P):
        m[q, :q + 1] = 1
    for i in range(N):
        if i >= tr["n_nodes"]:
            m[P + i, P + i] = 1
            continue
        m[P + i, :P] = 1
        if sibling_leak:
            m[P + i, P:P + i + 1] = 1
            continue
        a = i
        while a >= 0:
            m[P + i, P + a] = 1
            a = tr["parent"][a]
    return m


def _blocks(sd, cfg, x, mask):
    """the model's blocks under a boolean table mask [R, R] (oracle.ref_models.gpt_block with that table in place of the causal one)"""
    d, H = cfg.n_embd, cfg.n_head
    for i in range(cfg.n_layer):
        p = f"transformer.h.{i}."
        h = RM.layer_norm(x, sd[p + "ln_1.weight"], sd.get(p + "ln_1.bias"))
        qkv = RM.linear(h, sd[p + "attn.c_attn.weight"], sd.get(p + "attn.c_attn.bias"))
        q, k, v = (t.view(1, -1, H, d // H).transpose(1, 2) for t in qkv.split(d, dim=2))
        y = RM.sdpa(q, k, v, mask).transpose(1, 2).reshape(1, -1, d)
        x = x + RM.linear(y, sd[p + "attn.c_proj.weight"], sd.get(p + "attn.c_proj.bias"))
        h = RM.layer_norm(x, sd[p + "ln_2.weight"], sd.get(p + "ln_2.bias"))
        h = RM.gelu_erf(RM.linear(h, sd[p + "mlp.c_fc.weight"], sd.get(p + "mlp.c_fc.bias")))
        x = x + RM.linear(h, sd[p + "mlp.c_proj.weight"], sd.get(p + "mlp.c_proj.bias"))
    return x


def packed_lm(sd, cfg, tr, n, prefix, eos, sibling_leak=False):
    """one sentence: the packed forward over the trie -> lm [n] (-inf for an unscored hypothesis); prefix [P, d] or None"""
    wte, wpe = sd["transformer.wte.weight"], sd["transformer.wpe.weight"]
    P = 0 if prefix is None else prefix.shape[0]
    N = len(tr["tok"])
    x = wte[torch.from_numpy(tr["tok"])] + wpe[P + torch.from_numpy(tr["depth"])]
    if P:
        x = torch.cat([prefix.to(wte.dtype) + wpe[:P], x], dim=0)
    x = _blocks(sd, cfg, x[None], torch.from_numpy(visibility(tr, P, sibling_leak)).bool())[0]
    src, tgt = head_rows(tr, n, P, eos)
    hid = RM.layer_norm(x[torch.from_numpy(src)], sd["transformer.ln_f.weight"], sd.get("transformer.ln_f.bias"))
    logp = torch.log_softmax(RM.linear(hid, wte), dim=-1)
    lp = logp[torch.arange(len(tgt)), torch.from_numpy(np.where(tgt < 0, 0, tgt))]
    cum = [lp.new_zeros(())]
    for i in range(1, tr["n_nodes"]):
        cum.append(cum[tr["parent"][i]] + lp[i - 1])
    lm = np.full(n, -np.inf)
    for h in range(n):
        if tr["leaf"][h] >= 0:
            v = cum[tr["leaf"][h]]
            if eos is not None:
                v = v + lp[N - 1 + h]
            lm[h] = float(v)
    return lm


def flat_lm(sd, cfg, ids, lengths, scored, prefix, bos, eos):
    """one sentence, every scored hypothesis on its own: [bos, tokens] (behind the prefix) through gpt_forward, log_softmax of the full
    logits, the tokens' entries gathered and summed (+ the end-of-text entry behind the last token) -> lm [n]"""
    ids = np.asarray(ids)
    n, T = ids.shape
    lens = clamp_lengths(lengths, T)
    lm = np.full(n, -np.inf)
    for h in range(n):
        if not scored[h]:
            continue
        seq = [int(bos)] + [int(t) for t in ids[h, :lens[h]]]
        idx = torch.tensor([seq], dtype=torch.int64)
        _, logits = RM.gpt_forward(sd, idx, None if prefix is None else prefix[None].to(sd["transformer.wte.weight"].dtype), idx, cfg)
        logp = torch.log_softmax(logits[0], dim=-1)
        v = sum((logp[j, seq[j + 1]] for j in range(len(seq) - 1)), logp.new_zeros(()))
        if eos is not None:
            v = v + logp[len(seq) - 1, eos]
        lm[h] = float(v)
    return lm


def combine_rank(am, lm, lens, scored, am_weight=1.0, lm_weight=1.0, length_bonus=0.0):
    """-> (total [n] in input order, order [n]: the original index of every place, n_scored)"""
    n = len(lm)
    amv = np.zeros(n) if am is None else np.asarray(am, dtype=np.float64)
    total = np.full(n, -np.inf)
    for h in range(n):
        if scored[h]:
            total[h] = am_weight * amv[h] + lm_weight * lm[h] + length_bonus * lens[h]
    good = sorted((h for h in range(n) if scored[h]), key=lambda h: (-total[h], h))
    order = np.array(good + [h for h in range(n) if not scored[h]], dtype=np.int64)
    return total, order, len(good)


def smallest_gap(total, scored):
    """the smallest non-zero difference between two scored totals (what the ranking has to separate); inf when there is none"""
    t = np.sort(np.array([total[h] for h in range(len(total)) if scored[h]]))
    d = np.diff(t)
    d = d[d > 0]
    return float(d.min()) if d.size else np.inf
