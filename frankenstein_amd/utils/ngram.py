"""Backoff n-gram language models for the fused CTC prefix beam search (engine.ctc_beam_decode_lm, fk_ctc_beam_search_lm).

NGramLM holds a model in ARPA form, natural logs: `ngrams` maps (w_1, .., w_k) -> ln P(w_k | w_1 .. w_{k-1}) and `bows` maps a context
-> ln of its backoff weight, orders 1 .. 8.  A token id is a class id of the CTC head (the blank has an id like any class; the search never
looks it up), the end of sentence is id `n_classes` (self.eos) and the start of sentence is id `n_classes + 1` (self.bos), which occurs
only inside contexts.  Every id in [0, n_classes] has a unigram.

    score(context, token)   the plain recursive backoff definition in float64, straight from the dicts: the yardstick
    compile()               the same model as flat tables for the device, a state machine (CompiledNGram)
    from_arpa / from_corpus an ARPA text, or interpolated Witten-Bell estimates written out in backoff form

A state of the compiled model is a context that occurs (as the context of an n-gram, or with a backoff weight); state 0 is the empty
context.  The state of a history is its longest suffix that is a state: a longer suffix has neither n-grams nor a backoff weight, so
skipping it changes no score.  That needs the usual closure of ARPA files, which compile() checks: a context that occurs is itself an
n-gram (so that a hit at a backed-off level also knows the longest state of the extended history).
"""
from __future__ import annotations

import math
import os
from typing import Dict, Iterable, Optional, Sequence, Tuple

import numpy as np

MAX_ORDER = 8
LN10 = math.log(10.0)


def hash_slot(state, token, cap: int):
    """fk_ngram_hash of include/franken_hip.h; ints or integer arrays"""
    h = (np.asarray(state, dtype=np.uint64) * np.uint64(0x9E3779B1) ^ np.asarray(token, dtype=np.uint64) * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x2C1B3C6D)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(12)
    return (h & np.uint64(cap - 1)).astype(np.int64)


class CompiledNGram:
    """The device tables of an NGramLM (layout: include/franken_hip.h, fk_ctc_beam_search_lm).

    table    int32 [cap, 4]   open addressing, linear probing from hash_slot(state, token, cap): {state, token, bits of the fp32 ln p,
                              next state}; state -1 is an empty entry; cap a power of two >= 2 * entries
    bow      fp32  [S]        ln of the state's backoff weight;  backoff int32 [S]: the state of the context without its first symbol
                              (its context is strictly shorter; state 0 backs off to itself and is never asked to)
    uni_lp   fp32  [C + 1]    state 0, dense: ln P(token);  uni_next int32 [C + 1]: the state of the history (token,)
    depth    int32 [S]        the length of the state's context (host only: what validate() holds the backoff chain to)
    max_probe                 the largest number of entries a successful look-up reads;  start_state: the state of (<s>,)
    """

    def __init__(self, table, bow, backoff, uni_lp, uni_next, depth, max_probe, start_state, order, n_classes):
        self.table = np.ascontiguousarray(table, dtype=np.int32)
        self.bow = np.ascontiguousarray(bow, dtype=np.float32)
        self.backoff = np.ascontiguousarray(backoff, dtype=np.int32)
        self.uni_lp = np.ascontiguousarray(uni_lp, dtype=np.float32)
        self.uni_next = np.ascontiguousarray(uni_next, dtype=np.int32)
        self.depth = np.ascontiguousarray(depth, dtype=np.int32)
        self.max_probe, self.start_state, self.order, self.n_classes = int(max_probe), int(start_state), int(order), int(n_classes)
        self.validate()
        self._dev = {}

    @property
    def cap(self) -> int:
        return int(self.table.shape[0])

    @property
    def n_states(self) -> int:
        return int(self.bow.shape[0])

    @property
    def n_entries(self) -> int:
        return int((self.table[:, 0] >= 0).sum())

    def validate(self) -> None:
        """everything the device loop relies on; ValueError with the first thing that does not hold"""
        S, C, cap = self.n_states, self.n_classes, self.cap
        if not 1 <= self.order <= MAX_ORDER:
            raise ValueError(f"order = {self.order} outside 1 .. {MAX_ORDER}")
        if self.table.ndim != 2 or self.table.shape[1] != 4 or cap < 1 or cap & (cap - 1):
            raise ValueError(f"table shape {self.table.shape}: [cap, 4] with cap a power of two")
        if S < 1 or self.backoff.shape != (S,) or self.depth.shape != (S,) or self.uni_lp.shape != (C + 1,) or self.uni_next.shape != (C + 1,):
            raise ValueError("table shapes disagree")
        used = self.table[self.table[:, 0] >= 0]
        if 2 * len(used) > cap and len(used) > 0:
            raise ValueError(f"cap = {cap} below twice the {len(used)} entries")
        if not 1 <= self.max_probe <= cap:
            raise ValueError(f"max_probe = {self.max_probe} outside 1 .. cap = {cap}")
        if np.any(self.table[:, 0] < -1) or np.any(used[:, 0] >= S) or np.any(used[:, 0] == 0):
            raise ValueError("an entry's state outside [1, S)")
        if np.any(used[:, 1] < 0) or np.any(used[:, 1] > C):
            raise ValueError("an entry's token outside [0, C]")
        if np.any(used[:, 3] < 0) or np.any(used[:, 3] >= S) or np.any(self.uni_next < 0) or np.any(self.uni_next >= S):
            raise ValueError("a next state outside [0, S)")
        if not 0 <= self.start_state < S:
            raise ValueError(f"start_state = {self.start_state} outside [0, S = {S})")
        if np.any(self.backoff < 0) or np.any(self.backoff >= S) or self.backoff[0] != 0 or self.depth[0] != 0:
            raise ValueError("a backoff state outside [0, S), or state 0 is not the empty context")
        if np.any(self.depth[1:] < 1) or np.any(self.depth >= max(self.order, 2)):
            raise ValueError("a state's context is longer than order - 1")
        if np.any(self.depth[self.backoff[1:]] >= self.depth[1:]):
            raise ValueError("a backoff state whose context is not strictly shorter")
        lp = used[:, 2].copy().view(np.float32)
        if np.any(np.isnan(lp)) or np.any(lp > 0) or np.any(np.isnan(self.uni_lp)) or np.any(self.uni_lp > 0) or np.any(~np.isfinite(self.bow)):
            raise ValueError("a log-probability above 0 or NaN, or a backoff weight that is not finite")
        if len(used):                                    # every entry is found again within max_probe reads, and only once
            idx = np.nonzero(self.table[:, 0] >= 0)[0]
            dist = (idx - hash_slot(used[:, 0], used[:, 1], cap)) & (cap - 1)
            if np.any(dist >= self.max_probe):
                raise ValueError("an entry lies beyond max_probe")
            for i, d in zip(idx[dist > 0], dist[dist > 0]):   # no empty entry between an entry and its home
                if np.any(self.table[(i - np.arange(1, d + 1)) & (cap - 1), 0] < 0):
                    raise ValueError("an empty entry inside a probe sequence")
            keys = used[:, 0].astype(np.int64) * (C + 1) + used[:, 1]
            if len(np.unique(keys)) != len(keys):
                raise ValueError("an n-gram occurs twice")

    def lookup(self, state: int, token: int) -> Tuple[float, int]:
        """(ln P(token | state) as fp32, next state): the device loop, statement by statement"""
        S, mask, f32 = self.n_states, self.cap - 1, np.float32
        s = min(max(int(state), 0), S - 1)
        token = min(max(int(token), 0), self.n_classes)
        acc = f32(0.0)
        for _ in range(self.order):                      # at most `order` rounds
            if s == 0:
                break
            h = int(hash_slot(s, token, self.cap))
            for p in range(self.max_probe):
                e = self.table[(h + p) & mask]
                if e[0] == s and e[1] == token:
                    return float(f32(acc + e[2:3].copy().view(f32)[0])), min(max(int(e[3]), 0), S - 1)
                if e[0] == -1:
                    break
            acc = f32(acc + self.bow[s])
            s = min(max(int(self.backoff[s]), 0), S - 1)
        return float(f32(acc + self.uni_lp[token])), min(max(int(self.uni_next[token]), 0), S - 1)

    def to(self, device):
        """the tables as tensors on `device` (cached): dict(table int32 [cap, 4], bow, backoff, uni_lp, uni_next)"""
        import torch
        key = str(torch.device(device))
        if key not in self._dev:
            self._dev[key] = {n: torch.from_numpy(getattr(self, n)).to(device) for n in ("table", "bow", "backoff", "uni_lp", "uni_next")}
        return self._dev[key]


class NGramLM:
    def __init__(self, ngrams: Dict[tuple, float], bows: Dict[tuple, float], order: int, n_classes: int):
        if not 1 <= order <= MAX_ORDER:
            raise ValueError(f"order = {order} outside 1 .. {MAX_ORDER}")
        self.ngrams, self.bows, self.order, self.n_classes = ngrams, bows, int(order), int(n_classes)
        self.eos, self.bos = self.n_classes, self.n_classes + 1
        for g in ngrams:
            if not 1 <= len(g) <= order or not 0 <= g[-1] <= self.eos or any(not 0 <= w <= self.bos or w == self.eos for w in g[:-1]):
                raise ValueError(f"n-gram {g}: at most {order} ids, the last in [0, {self.eos}], </s> only there")
        missing = [c for c in range(self.eos + 1) if (c,) not in ngrams]
        if missing:
            raise ValueError(f"{len(missing)} ids without a unigram, the first {missing[0]}")
        self._compiled = None

    # ---- the definition ---------------------------------------------------------------------------------------------------------
    @property
    def start_context(self) -> tuple:
        """what precedes a sentence: (<s>,) when the model knows the symbol, else nothing"""
        knows = (self.bos,) in self.bows or any(g[0] == self.bos for g in self.ngrams if len(g) > 1)
        return (self.bos,) if knows else ()

    def score(self, context: Sequence[int], token: int) -> float:
        """ln P(token | context), float64: the n-gram itself if it is listed, else bow(context) + the score under the context without its
        first symbol (a context without a weight has weight 1)"""
        ctx = tuple(int(w) for w in context)
        ctx = ctx[len(ctx) - (self.order - 1):] if len(ctx) > self.order - 1 else ctx
        acc = 0.0
        while True:
            lp = self.ngrams.get(ctx + (int(token),))
            if lp is not None:
                return acc + lp
            if not ctx:
                raise KeyError(f"token {token} has no unigram")
            acc += self.bows.get(ctx, 0.0)
            ctx = ctx[1:]

    # ---- sources -----------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_arpa(cls, text_or_path, token_to_id: Dict[str, int], n_classes: int, unk_logp: Optional[float] = None) -> "NGramLM":
        """An ARPA text (or the path of one; log10 values).  token_to_id maps the file's words to class ids; <s> and </s> are the start
        and the end of sentence; an n-gram with any other word that has no id is left out.  A class without a unigram gets the value of
        <unk>, or unk_logp (natural log; required when the file has no <unk>)."""
        text = str(text_or_path)
        if "\n" not in text and os.path.exists(text):
            with open(text) as f:
                text = f.read()
        eos, bos = n_classes, n_classes + 1
        ids = dict(token_to_id)
        ids["<s>"], ids["</s>"] = bos, eos
        ngrams, bows, order, k, unk = {}, {}, 0, 0, None
        for line in text.splitlines():
            line = line.strip()
            if not line or line == "\\data\\" or line.startswith("ngram "):
                continue
            if line == "\\end\\":
                break
            if line.startswith("\\") and line.endswith("-grams:"):
                k = int(line[1:-len("-grams:")])
                order = max(order, k)
                continue
            if k == 0:
                continue
            f = line.split()
            if len(f) not in (k + 1, k + 2):
                raise ValueError(f"ARPA line with {len(f)} fields in the {k}-grams: {line!r}")
            lp, words = float(f[0]) * LN10, f[1:k + 1]
            bow = float(f[k + 1]) * LN10 if len(f) == k + 2 else None
            if k == 1 and words[0] in ("<unk>", "<UNK>") and words[0] not in token_to_id:
                unk = lp
                continue
            if any(w not in ids for w in words):
                continue
            g = tuple(ids[w] for w in words)
            if g[-1] != bos:                              # <s> is never predicted: its line carries a backoff weight only
                ngrams[g] = lp
            if bow is not None and eos not in g:
                bows[g] = bow
        floor = unk if unk is not None else unk_logp
        for c in range(n_classes + 1):
            if (c,) not in ngrams:
                if floor is None:
                    raise ValueError(f"class {c} has no unigram and the file has no <unk>: give unk_logp")
                ngrams[(c,)] = float(floor)
        return cls(ngrams, bows, max(order, 1), n_classes)

    @classmethod
    def from_corpus(cls, sequences: Iterable[Sequence[int]], order: int, n_classes: int) -> "NGramLM":
        """Interpolated Witten-Bell estimates from sequences of class ids, written out in backoff form:
            P(c | ctx) = (n(ctx c) + T(ctx) P(c | ctx')) / (n(ctx) + T(ctx)),   ctx' = ctx without its first symbol,
        n(ctx) the count of ctx as a context, T(ctx) the number of distinct symbols seen after it; the unigram level is interpolated with
        the uniform distribution over the n_classes + 1 symbols (classes and </s>).  A listed n-gram holds ln P, and bow(ctx) =
        T / (n + T) gives an unlisted one exactly the interpolated value, so every context's distribution sums to 1."""
        if not 1 <= order <= MAX_ORDER:
            raise ValueError(f"order = {order} outside 1 .. {MAX_ORDER}")
        eos, bos = n_classes, n_classes + 1
        counts = [dict() for _ in range(order)]           # counts[k][ctx of length k][c]
        for seq in sequences:
            s = (bos,) + tuple(int(w) for w in seq) + (eos,)
            if any(not 0 <= w < n_classes for w in s[1:-1]):
                raise ValueError(f"a sequence holds an id outside [0, {n_classes})")
            for j in range(1, len(s)):
                for k in range(min(order - 1, j) + 1):
                    d = counts[k].setdefault(s[j - k:j], {})
                    d[s[j]] = d.get(s[j], 0) + 1
        V = n_classes + 1
        uni = counts[0].get((), {})
        n0, t0 = sum(uni.values()), len(uni)
        p_uni = np.full(V, (t0 / V) / (n0 + t0) if n0 else 1.0 / V)
        for c, n in uni.items():
            p_uni[c] = (n + t0 / V) / (n0 + t0)
        prob = {(c,): float(p_uni[c]) for c in range(V)}   # P of every listed n-gram, level by level
        bows = {}
        for k in range(1, order):
            for ctx, d in counts[k].items():
                n, t = sum(d.values()), len(d)
                bows[ctx] = math.log(t / (n + t))
                for c, m in d.items():
                    prob[ctx + (c,)] = (m + t * prob[ctx[1:] + (c,)]) / (n + t)
        return cls({g: math.log(p) for g, p in prob.items()}, bows, order, n_classes)

    def to_arpa(self, id_to_token: Dict[int, str]) -> str:
        """the model as an ARPA text (log10, 17 significant digits); ids eos / bos are written </s> / <s>"""
        names = dict(id_to_token)
        names[self.eos], names[self.bos] = "</s>", "<s>"
        levels = [[] for _ in range(self.order)]
        for g in self.ngrams:
            levels[len(g) - 1].append(g)
        extra = [ctx for ctx in self.bows if ctx not in self.ngrams]      # (<s>,), and weights of contexts that are no n-gram
        for ctx in extra:
            levels[len(ctx) - 1].append(ctx)
        out = ["\\data\\"] + [f"ngram {k + 1}={len(level)}" for k, level in enumerate(levels)]
        for k, level in enumerate(levels):
            out += ["", f"\\{k + 1}-grams:"]
            for g in sorted(level):
                lp = self.ngrams[g] / LN10 if g in self.ngrams else -99.0
                line = f"{lp:.17g}\t" + " ".join(names[w] for w in g)
                if g in self.bows:
                    line += f"\t{self.bows[g] / LN10:.17g}"
                out.append(line)
        return "\n".join(out + ["", "\\end\\", ""])

    # ---- the device form ---------------------------------------------------------------------------------------------------------
    def compile(self) -> CompiledNGram:
        if self._compiled is not None:
            return self._compiled
        C, order = self.n_classes, self.order
        contexts = {g[:-1] for g in self.ngrams if len(g) > 1} | {ctx for ctx, w in self.bows.items() if w != 0.0}
        contexts = {ctx for ctx in contexts if 1 <= len(ctx) <= order - 1}
        for ctx in contexts:
            if ctx != (self.bos,) and ctx not in self.ngrams:
                raise ValueError(f"context {ctx} occurs but is no n-gram itself: the model is not closed under prefixes")
        states = [()] + sorted(contexts, key=lambda c: (len(c), c))
        sid = {ctx: i for i, ctx in enumerate(states)}

        def state_of(hist):
            hist = hist[len(hist) - (order - 1):] if order > 1 and len(hist) > order - 1 else (hist if order > 1 else ())
            while hist not in sid:
                hist = hist[1:]
            return sid[hist]

        S = len(states)
        bow = np.array([self.bows.get(ctx, 0.0) for ctx in states], dtype=np.float32)
        backoff = np.array([0] + [state_of(ctx[1:]) for ctx in states[1:]], dtype=np.int32)
        depth = np.array([len(ctx) for ctx in states], dtype=np.int32)
        uni_lp = np.array([self.ngrams[(c,)] for c in range(C + 1)], dtype=np.float32)
        uni_next = np.array([state_of((c,)) for c in range(C)] + [0], dtype=np.int32)
        grams = [g for g in self.ngrams if len(g) > 1]
        cap = 2
        while cap < 2 * len(grams):
            cap *= 2
        table = np.full((cap, 4), -1, dtype=np.int32)
        max_probe = 1
        if grams:
            st = np.array([sid[g[:-1]] for g in grams], dtype=np.int64)
            tok = np.array([g[-1] for g in grams], dtype=np.int64)
            bits = np.array([self.ngrams[g] for g in grams], dtype=np.float32).view(np.int32)
            nxt = np.array([0 if g[-1] == self.eos else state_of(g) for g in grams], dtype=np.int64)
            home = hash_slot(st, tok, cap)
            filled = np.zeros(cap, dtype=bool)
            for i in np.lexsort((tok, st)):               # a fixed order of insertion: the same table every time
                p, n = int(home[i]), 1
                while filled[p]:
                    p, n = (p + 1) & (cap - 1), n + 1
                filled[p] = True
                table[p] = (st[i], tok[i], bits[i], nxt[i])
                max_probe = max(max_probe, n)
        self._compiled = CompiledNGram(table, bow, backoff, uni_lp, uni_next, depth, max_probe, state_of(self.start_context), order, C)
        return self._compiled

    def state_of(self, context: Sequence[int]) -> int:
        """the compiled state of a history: its longest suffix that is a state (walks the compiled machine from state 0)"""
        t, s = self.compile(), 0
        for w in tuple(context)[-(self.order - 1):] if self.order > 1 else ():
            s = t.lookup(s, w)[1] if w != self.bos else t.start_state
        return s


def zipf_sequences(n: int, n_classes: int, blank: int, length: Tuple[int, int], seed: int, exponent: float = 1.1, n_types: Optional[int] = None):
    """n seeded sequences of non-blank class ids with Zipf-distributed frequencies (rank r ~ r^-exponent over a seeded permutation of
    n_types classes), lengths uniform in [length[0], length[1]]: the corpus the tests and tools/ctc_bench.py build their models from"""
    rng = np.random.default_rng(seed)
    ids = np.delete(np.arange(n_classes), blank)
    ids = rng.permutation(ids)[:n_types or len(ids)]
    p = np.arange(1, len(ids) + 1, dtype=np.float64) ** -exponent
    p /= p.sum()
    return [tuple(int(c) for c in rng.choice(ids, size=int(rng.integers(length[0], length[1] + 1)), p=p)) for _ in range(n)]
