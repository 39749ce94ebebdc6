"""Pronunciation lexicons for the lexicon-constrained CTC prefix beam search (engine.ctc_beam_decode_lexicon, fk_ctc_beam_search_lex).

A Lexicon maps pronunciations (non-empty tuples of class ids of the CTC head, none of them the blank or the word separator) to word ids
in [0, V).  Several words may share a pronunciation (homophones, at most MAX_HOMOPHONES of them), a word may have several pronunciations.

    Lexicon(entries)                   (word, pronunciation ids) pairs; word ids in the order of first appearance
    Lexicon.from_text(text, ph_to_id)  `WORD PH PH ...` lines; `WORD(2)` is a variant of WORD, `;;;` starts a comment
    compile()                          the trie as flat tables for the device (CompiledLexicon; layout: include/franken_hip.h)
    pronounce(word_ids, sep)           the labelling of a transcript: how CTC targets for such a head are built
    text(words, lengths)               strings from decoded word ids

The trie: node 0 is the root (a word start); a node where a pronunciation ends is terminal and lists its words by ascending id.
"""
from __future__ import annotations

import os
import re
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from frankenstein_amd.utils.ngram import hash_slot

MAX_HOMOPHONES = 8


class CompiledLexicon:
    """The device tables of a Lexicon.

    table       int32 [cap, 4]      open addressing, linear probing from hash_slot(node, class, cap): {node, class, child, 0}; node -1 is an
                                    empty entry; cap a power of two >= 2 * entries
    node_words  int32 [n_nodes, 2]  {first, count} into word_list; count 0: not terminal
    word_list   int32 [n_list]      the words of the terminal nodes, each node's by ascending id
    max_probe                       the largest number of entries a successful look-up reads;  n_words: V
    """

    def __init__(self, table, node_words, word_list, max_probe, n_words):
        self.table = np.ascontiguousarray(table, dtype=np.int32)
        self.node_words = np.ascontiguousarray(node_words, dtype=np.int32)
        self.word_list = np.ascontiguousarray(word_list, dtype=np.int32)
        self.max_probe, self.n_words = int(max_probe), int(n_words)
        self.validate()
        self.classes = frozenset(int(c) for c in np.unique(self.table[self.table[:, 0] >= 0, 1]))   # the classes pronunciations use
        self._dev = {}
        self._null = None

    @property
    def cap(self) -> int:
        return int(self.table.shape[0])

    @property
    def n_nodes(self) -> int:
        return int(self.node_words.shape[0])

    @property
    def n_entries(self) -> int:
        return int((self.table[:, 0] >= 0).sum())

    def validate(self) -> None:
        """everything the device loop relies on; ValueError with the first thing that does not hold"""
        cap, N, L, V = self.cap, self.n_nodes, len(self.word_list), self.n_words
        if self.table.ndim != 2 or self.table.shape[1] != 4 or cap < 1 or cap & (cap - 1):
            raise ValueError(f"table shape {self.table.shape}: [cap, 4] with cap a power of two")
        if self.node_words.ndim != 2 or self.node_words.shape[1] != 2 or N < 1 or L < 1 or V < 1:
            raise ValueError("node_words [n_nodes, 2] with at least the root, a word list and a vocabulary that are not empty")
        used = self.table[self.table[:, 0] >= 0]
        if 2 * len(used) > cap and len(used) > 0:
            raise ValueError(f"cap = {cap} below twice the {len(used)} entries")
        if not 1 <= self.max_probe <= cap:
            raise ValueError(f"max_probe = {self.max_probe} outside 1 .. cap = {cap}")
        if np.any(self.table[:, 0] < -1) or np.any(used[:, 0] >= N):
            raise ValueError("an entry's node outside [0, n_nodes)")
        if np.any(used[:, 1] < 0):
            raise ValueError("an entry's class below 0")
        if np.any(used[:, 2] < 1) or np.any(used[:, 2] >= N):
            raise ValueError("a child outside [1, n_nodes)")
        if len(np.unique(used[:, 2])) != len(used) or len(used) != N - 1:
            raise ValueError("every node but the root is the child of exactly one entry")
        first, count = self.node_words[:, 0].astype(np.int64), self.node_words[:, 1].astype(np.int64)
        if np.any(count < 0) or np.any(count > MAX_HOMOPHONES) or count[0] != 0:
            raise ValueError(f"a word count outside 0 .. {MAX_HOMOPHONES}, or the root ends a word")
        if np.any(first < 0) or np.any(first + count > L):
            raise ValueError("a node's words lie outside the word list")
        if np.any(self.word_list < 0) or np.any(self.word_list >= V):
            raise ValueError("a word id outside [0, V)")
        for n in np.nonzero(count > 1)[0]:
            if np.any(np.diff(self.word_list[first[n]:first[n] + count[n]]) <= 0):
                raise ValueError(f"the words of node {n} are not in ascending order")
        if len(used):
            idx = np.nonzero(self.table[:, 0] >= 0)[0]
            dist = (idx - hash_slot(used[:, 0], used[:, 1], cap)) & (cap - 1)
            if np.any(dist >= self.max_probe):
                raise ValueError("an entry lies beyond max_probe")
            for i, d in zip(idx[dist > 0], dist[dist > 0]):
                if np.any(self.table[(i - np.arange(1, d + 1)) & (cap - 1), 0] < 0):
                    raise ValueError("an empty entry inside a probe sequence")
            keys = used[:, 0].astype(np.int64) * (int(used[:, 1].max()) + 1) + used[:, 1]
            if len(np.unique(keys)) != len(keys):
                raise ValueError("a (node, class) pair occurs twice")

    def child(self, node: int, c: int) -> int:
        """the child of `node` under class `c`, or -1: the device loop, statement by statement"""
        mask = self.cap - 1
        h = int(hash_slot(int(node), int(c), self.cap))
        for p in range(self.max_probe):
            e = self.table[(h + p) & mask]
            if e[0] == -1:
                return -1
            if e[0] == node and e[1] == c:
                return min(max(int(e[2]), 0), self.n_nodes - 1)
        return -1

    def words_at(self, node: int) -> List[int]:
        """the words whose pronunciation ends at `node` (ascending ids; empty: not terminal)"""
        first, count = (int(v) for v in self.node_words[node])
        return [int(w) for w in self.word_list[first:first + count]] if node > 0 else []

    def null_lm(self):
        """the tables of `no word model` over this vocabulary (cached, so that its device copy is made once)"""
        if self._null is None:
            self._null = null_word_lm(self.n_words)
        return self._null

    def to(self, device):
        """the tables as tensors on `device` (cached): dict(table int32 [cap, 4], node_words int32 [n_nodes, 2], word_list)"""
        import torch
        key = str(torch.device(device))
        if key not in self._dev:
            self._dev[key] = {n: torch.from_numpy(getattr(self, n)).to(device) for n in ("table", "node_words", "word_list")}
        return self._dev[key]


class Lexicon:
    def __init__(self, entries: Iterable[Tuple[str, Sequence[int]]]):
        self.words: List[str] = []
        self.word_to_id: Dict[str, int] = {}
        self.pronunciations: Dict[tuple, List[int]] = {}            # pronunciation -> word ids, ascending
        self._first: Dict[int, tuple] = {}                         # word id -> its first pronunciation
        for word, pron in entries:
            pron = tuple(int(c) for c in pron)
            if not pron or any(c < 0 for c in pron):
                raise ValueError(f"word {word!r}: a pronunciation is a non-empty tuple of class ids, got {pron}")
            w = self.word_to_id.setdefault(word, len(self.words))
            if w == len(self.words):
                self.words.append(word)
            self._first.setdefault(w, pron)
            ws = self.pronunciations.setdefault(pron, [])
            if w not in ws:
                ws.append(w)
        if not self.words:
            raise ValueError("a lexicon needs at least one word")
        for ws in self.pronunciations.values():
            ws.sort()
        self._compiled = None

    def __len__(self) -> int:
        return len(self.words)

    @classmethod
    def from_text(cls, text_or_path, phoneme_to_id: Dict[str, int]) -> "Lexicon":
        """`WORD PH PH ...` lines (or the path of such a file).  `WORD(2)` is another pronunciation of WORD; text from `;;;` on is a
        comment; an unknown phoneme raises a ValueError with its line number."""
        text = str(text_or_path)
        if "\n" not in text and os.path.exists(text):
            with open(text) as f:
                text = f.read()
        entries = []
        for no, line in enumerate(text.splitlines(), 1):
            f = line.split(";;;")[0].split()
            if not f:
                continue
            if len(f) < 2:
                raise ValueError(f"line {no}: word {f[0]!r} has no pronunciation")
            unknown = [p for p in f[1:] if p not in phoneme_to_id]
            if unknown:
                raise ValueError(f"line {no}: unknown phoneme {unknown[0]!r}")
            entries.append((re.sub(r"\(\d+\)$", "", f[0]), [phoneme_to_id[p] for p in f[1:]]))
        return cls(entries)

    def prefixes(self) -> set:
        """every proper or full prefix of a pronunciation, the empty one included: the nodes of the trie"""
        return {p[:k] for p in self.pronunciations for k in range(len(p) + 1)}

    def compile(self) -> CompiledLexicon:
        if self._compiled is not None:
            return self._compiled
        for pron, ws in self.pronunciations.items():
            if len(ws) > MAX_HOMOPHONES:
                raise ValueError(f"pronunciation {pron} is shared by {len(ws)} words, at most {MAX_HOMOPHONES} may share one")
        nodes = sorted(self.prefixes(), key=lambda p: (len(p), p))  # a fixed order: the same tables every time; the root first
        nid = {p: i for i, p in enumerate(nodes)}
        node_words = np.zeros((len(nodes), 2), dtype=np.int32)
        word_list = []
        for p in nodes:
            ws = self.pronunciations.get(p, [])
            node_words[nid[p]] = (len(word_list), len(ws))
            word_list += ws
        edges = [(nid[p[:-1]], p[-1], nid[p]) for p in nodes[1:]]
        cap = 2
        while cap < 2 * len(edges):
            cap *= 2
        table = np.full((cap, 4), -1, dtype=np.int32)
        max_probe = 1
        home = hash_slot(np.array([e[0] for e in edges]), np.array([e[1] for e in edges]), cap)
        filled = np.zeros(cap, dtype=bool)
        for (n, c, ch), h in zip(edges, home):
            p, k = int(h), 1
            while filled[p]:
                p, k = (p + 1) & (cap - 1), k + 1
            filled[p] = True
            table[p] = (n, c, ch, 0)
            max_probe = max(max_probe, k)
        self._compiled = CompiledLexicon(table, node_words, np.array(word_list, dtype=np.int32), max_probe, len(self.words))
        return self._compiled

    def pronounce(self, word_ids: Sequence[int], sep: int, trailing_sep: bool = True) -> List[int]:
        """the labelling of a transcript: each word's first pronunciation, `sep` between the words and, with trailing_sep, behind the last"""
        out: List[int] = []
        for j, w in enumerate(word_ids):
            if j:
                out.append(int(sep))
            out += self._first[int(w)]
        if trailing_sep and len(word_ids):
            out.append(int(sep))
        return out

    def text(self, words, lengths=None):
        """decoded word ids [..., L] (a tensor, an array or nested lists) and their lengths [...] -> strings of the same nesting"""
        w = np.asarray(words.cpu() if hasattr(words, "cpu") else words)
        if lengths is None:
            n = np.full(w.shape[:-1], w.shape[-1], dtype=np.int64)
        else:
            n = np.asarray(lengths.cpu() if hasattr(lengths, "cpu") else lengths)
        if w.ndim == 1:
            return " ".join(self.words[int(i)] for i in w[:int(n)])
        return [self.text(w[i], n[i]) for i in range(w.shape[0])]


def zipf_lexicon(n_words: int, n_classes: int, blank: int, sep: int, length: Tuple[int, int] = (2, 6), seed: int = 0, homophone_rate: float = 0.1,
                 exponent: float = 1.1) -> Lexicon:
    """A seeded synthetic lexicon of n_words words `w0` .. over the classes other than blank and sep: pronunciation lengths uniform in
    [length[0], length[1]], classes Zipf-distributed over a seeded permutation; with probability homophone_rate a word takes the
    pronunciation of an earlier word (never more than MAX_HOMOPHONES on one).  What the tests and tools/ctc_bench.py decode with."""
    rng = np.random.default_rng(seed)
    ids = rng.permutation(np.array([c for c in range(n_classes) if c not in (blank, sep)]))
    p = np.arange(1, len(ids) + 1, dtype=np.float64) ** -exponent
    p /= p.sum()
    count: Dict[tuple, int] = {}
    prons: List[tuple] = []
    for _ in range(n_words):
        while True:
            if prons and rng.random() < homophone_rate:
                pron = prons[int(rng.integers(len(prons)))]
            else:
                pron = tuple(int(c) for c in rng.choice(ids, size=int(rng.integers(length[0], length[1] + 1)), p=p))
            if count.get(pron, 0) < MAX_HOMOPHONES:
                break
        count[pron] = count.get(pron, 0) + 1
        prons.append(pron)
    return Lexicon((f"w{i}", pron) for i, pron in enumerate(prons))


def null_word_lm(n_words: int):
    """the tables of `no word model`: a unigram model whose every ln P is 0, so that only word_bonus acts and w* is the lowest id"""
    from frankenstein_amd.utils.ngram import CompiledNGram
    z = np.zeros(n_words + 1)
    return CompiledNGram(np.full((2, 4), -1), np.zeros(1), np.zeros(1), z, z, np.zeros(1), 1, 0, 1, n_words)
