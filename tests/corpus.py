"""A deterministic boundary corpus for the match kernels (every list below is
written out or derived from a fixed rule; batches are tiled in an order
shuffled with a fixed seed).

`build()` returns the filters (unique bytes; a filter's id is its index), the
distinct topics, a family tag and the level count per topic, and the intended
adjacency of the neighbour-bait pairs.  The families sit on the constants at
which the kernels switch behaviour (egm_kernels.h / egm_kernels.hip):

  FIX_WORDS = 8            sorted batch: <= 8 levels read the fixed-stride words
  first-pass sub-chunk     64 topics up to 7 levels, 32 from 8
  DEEP_MIN = 12            a chunk with a 13-level topic goes to the deep pass
  S * dmax <= 448          the deep pass's sub-chunk halves at 14/15, 28/29,
                           56/57, 112/113, 224/225
  light_dmax(504, 448)     = 440: a chunk with a 441-level topic goes to k_heavy

`reference()` is the expectation of record: oracle.trie_ref brute force over
the filter list, per distinct topic and mode, computed once per process.
`gather()` turns per-topic expectations into the CSR of a batch assembled from
the distinct topics by repetition.
"""
from __future__ import annotations

import functools
import time
from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import numpy as np

LADDER = (1, 2, 7, 8, 9, 12, 13, 14, 15, 28, 29, 56, 57, 112, 113, 224, 225, 440, 441)
BAIT_DMAX = (2, 7, 8, 12)
W16, W17, W20 = b"w16-0123456789ab", b"w17-0123456789abc", b"w20-0123456789abcdef"
# the ladder's words: no empty word, no '$', so every prefix is an ordinary name
LW = [b"a", b"b", b"c"] + [b"k%d" % i for i in range(10)] + [W16, W17, W20]
FAN_D = 9
FAN_TOPIC = [b"k%d" % i for i in range(FAN_D)]
FAN_TRIE = (2 ** FAN_D - 1) + (2 ** (FAN_D + 1) - 1)   # '+'-substitutions but the exact one + every prefix-substitution/#
PLUS, HASH = b"+", b"#"


def J(ws) -> bytes:
    return b"/".join(ws)


def ladder_words(D: int, v: int) -> List[bytes]:
    """The D-level ladder topic of variant v: a prefix of one periodic chain,
    so the topics of all depths share their prefixes."""
    return [LW[(l + 5 * v) % len(LW)] for l in range(D)]


@dataclass
class Corpus:
    filters: List[bytes]
    topics: List[bytes]
    tags: List[str]                      # family of each topic ("ladder:13", "bait:8", "wild", ...)
    depth: np.ndarray                    # levels of each topic
    bait_pairs: List[Tuple[int, int]]    # (bait topic, the neighbour to place directly behind it)
    wild_present: List[int]              # wildcard topics whose exact filter is in the table
    wild_absent: List[int]               # ... and whose exact filter is not
    index: Dict[bytes, int] = field(default_factory=dict)

    def family(self, prefix: str) -> List[int]:
        return [i for i, t in enumerate(self.tags) if t == prefix or t.startswith(prefix + ":")]

    def t(self, topic: bytes) -> int:
        return self.index[topic]


@functools.lru_cache(maxsize=None)
def build() -> Corpus:
    filters: Dict[bytes, None] = {}
    topics: Dict[bytes, str] = {}

    def F(*fs):
        for f in fs:
            filters.setdefault(f if isinstance(f, bytes) else J(f))

    def T(tag, t) -> bytes:
        t = t if isinstance(t, bytes) else J(t)
        topics.setdefault(t, tag)
        return t

    # ---- depth ladder ----
    for D in LADDER:
        F([PLUS] * D, [PLUS] * D + [HASH])
        for v in ((0, 1) if D < 112 else (0,)):   # one variant of the longest: they dominate the brute force's time
            w = ladder_words(D, v)
            tag = "ladder:%d" % D
            T(tag, w)
            T(tag + ":lastdiff", w[:-1] + [b"z"])
            if D > 1:
                T(tag + ":short", w[:-1])
            T(tag + ":long", ladder_words(D + 1, v))
            F(w, w[:-1] + [PLUS], [PLUS] + w[1:])                    # literal chain, '+' last, '+' first
            if D >= 3:
                m = D // 2
                F(w[:m] + [PLUS] + w[m + 1:])                        # '+' in the middle: the child's '+' child
            for cut in sorted({1, max(1, D // 2), max(1, D - 1), D}):
                F(w[:cut] + [HASH])                                  # prefix/# at several cut points
            F(w[:-1] + [b"z", HASH], w + [PLUS])                     # near-miss filters: last differs, one long

    # ---- neighbour bait for the '+' skip ----
    n0 = T("neigh", [b"z", b"y"])
    n1 = T("neigh", [b"z", b"y"] * 3 + [b"z"])
    F(b"z/+", b"z/y/#", b"z/y/z/+/#")
    bait = []
    for dmax in BAIT_DMAX:
        for v in ((0,) if dmax == 2 else (0, 1)):
            pre = [[b"a", b"b", b"c"][(l + v) % 3] for l in range(dmax - 2)]
            t = pre + [b"p", b"q"]
            P, P2 = t[:-1], t[:-2]
            tb = T("bait:%d" % dmax, t)
            base = [P + [PLUS], P + [PLUS, b"z"], P + [b"q", b"z"], P + [PLUS, b"z", b"y"], P + [PLUS, PLUS],
                    P + [b"q", PLUS, b"y"], P2 + [PLUS, b"q"], P2 + [PLUS, PLUS, b"z"], P2 + [PLUS, b"q", b"z", b"y"]]
            for f in base:
                F(f, f + [HASH])
            F(P + [b"q", HASH])
            bait.append((tb, n0))
            if dmax >= 7:
                bait.append((tb, n1))

    # ---- wildcard publish topics: exact filter present / absent ----
    t13, t441 = ladder_words(13, 0), ladder_words(441, 0)
    w9 = FAN_TOPIC[:4] + [PLUS] + FAN_TOPIC[5:]
    present = [b"+", b"#", b"a/+", b"a/#", b"a/+/#", b"+/+/+", b"a/#/b", J(w9), J(t13[:-1] + [HASH]),
               J(t441[:-1] + [PLUS])]
    absent = [b"+/c", b"#/c", b"a/+/c", b"a/#/c", b"a/+/#/c", b"+/+/+/c", b"a/#/b/c", J(w9[:-1] + [b"c"]),
              J(t13[:-2] + [PLUS, HASH]), J(t441[:-2] + [PLUS, b"z"])]
    F(*present)
    for t in present:
        T("wild", t)
    for t in absent:
        T("wild:absent", t)

    # ---- '$' topics ----
    for t in (b"$", b"$SYS", b"$SYS/a", b"$x/b/c"):
        T("dollar", t)
    F(b"#", b"+", b"+/a", b"$SYS/#", b"$SYS/+", b"$SYS", b"$", b"+/#")

    # ---- empty words ----
    for t in (b"", b"/", b"//", b"a/", b"/a", b"a//b"):
        T("empty", t)
    F(b"+", b"+/+", b"/+", b"+/", b"/#", b"#", b"a/+/b", b"", b"/", b"a/")

    # ---- high fan-out: every '+'-substitution of k0/../k8 and every prefix-substitution/# ----
    for m in range(1 << FAN_D):
        F([PLUS if (m >> l) & 1 else FAN_TOPIC[l] for l in range(FAN_D)])
    for p in range(FAN_D + 1):
        for m in range(1 << p):
            F([PLUS if (m >> l) & 1 else FAN_TOPIC[l] for l in range(p)] + [HASH])
    T("fanout", FAN_TOPIC)
    T("fanout8", FAN_TOPIC[:-1])
    T("zero", [b"$k0"] + FAN_TOPIC[1:])

    # ---- zero-match topics and words the dictionary does not hold ----
    for t in (b"$u", b"$u/v", b"$nope/a/b/c/k0/k1/k2/k3"):
        T("zero", t)
    t12 = ladder_words(12, 0)
    for t in (b"u0", b"u0/u1", b"a/u0", b"u0/b/c", J(FAN_TOPIC[:1] + [b"u1"] + FAN_TOPIC[2:]),
              J(t12[:6] + [b"nope"] + t12[7:]), J(ladder_words(7, 0) + [b"nope"]), J(t13[:12] + [b"u0"])):
        T("unknown", t)

    fl, tl = list(filters), list(topics)
    index = {t: i for i, t in enumerate(tl)}
    fset = set(fl)
    assert all(t in fset for t in present) and not any(t in fset for t in absent)
    return Corpus(fl, tl, [topics[t] for t in tl], np.array([t.count(b"/") + 1 for t in tl], np.int64),
                  [(index[a], index[b]) for a, b in bait], [index[t] for t in present], [index[t] for t in absent],
                  index)


class Reference:
    """Per distinct topic and mode: the expected ids (sorted) as one CSR."""

    def __init__(self, sets: Dict[int, List[List[int]]], seconds: float):
        self.seconds = seconds           # what the brute force took
        self.sets = sets
        self.row, self.ids = {}, {}
        for mode, rows in sets.items():
            cnt = np.fromiter((len(r) for r in rows), np.int64, len(rows))
            row = np.zeros(len(rows) + 1, np.int64)
            np.cumsum(cnt, out=row[1:])
            self.row[mode] = row
            self.ids[mode] = np.fromiter((x for r in rows for x in r), np.uint32, int(row[-1]))

    def count(self, mode: int) -> np.ndarray:
        return np.diff(self.row[mode])

    def gather(self, mode: int, idx: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """The CSR (row_ptr u64, ids u32 sorted within each row) of the batch
        whose k-th topic is the distinct topic idx[k]."""
        return gather(self.row[mode], self.ids[mode], idx)


def gather(row0: np.ndarray, ids0: np.ndarray, idx: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    idx = np.asarray(idx, np.int64)
    cnt = (row0[idx + 1] - row0[idx]).astype(np.int64)
    row = np.zeros(len(idx) + 1, np.uint64)
    row[1:] = np.cumsum(cnt)
    tot = int(row[-1])
    first = np.repeat(row0[idx] - row[:-1].astype(np.int64), cnt)   # source index minus destination index, per row
    return row, ids0[first + np.arange(tot, dtype=np.int64)]


@functools.lru_cache(maxsize=None)
def reference() -> Reference:
    """Brute force: oracle.trie_ref.trie_semantics / routes_semantics of every
    distinct topic over the whole filter list."""
    from oracle import trie_ref as R
    c = build()
    fid = {f: i for i, f in enumerate(c.filters)}
    t0 = time.perf_counter()
    sets = {0: [sorted(fid[f] for f in R.trie_semantics(t, c.filters)) for t in c.topics],
            1: [sorted(fid[f] for f in R.routes_semantics(t, c.filters)) for t in c.topics]}
    return Reference(sets, time.perf_counter() - t0)


def pack(c: Corpus, idx) -> Tuple[np.ndarray, np.ndarray]:
    """The batch of the distinct topics idx -> (blob u8, offsets u32[n + 1])."""
    idx = np.asarray(idx, np.int64)
    lens0 = np.fromiter((len(t) for t in c.topics), np.int64, len(c.topics))
    off0 = np.zeros(len(c.topics) + 1, np.int64)
    np.cumsum(lens0, out=off0[1:])
    blob0 = np.frombuffer(b"".join(c.topics), np.uint8)
    row, blob = gather(off0, blob0, idx)
    assert int(row[-1]) < 2 ** 32
    out = np.zeros(len(blob) + 8, np.uint8)
    out[:len(blob)] = blob
    return out, row.astype(np.uint32)


def tile(idx, n: int, seed: int = 0) -> np.ndarray:
    """n topics: idx in a fixed shuffled order, repeated."""
    idx = np.asarray(idx, np.int64)
    order = np.random.default_rng(0xC0FFEE + seed).permutation(len(idx))
    return np.resize(idx[order], n)


# ---- the mixed chunk (tests/test_gpu_path_matrix.py, asserted from the expectation in tests/test_corpus.py) ----
CHUNK = 64            # topics per walk chunk at n >= 131 072 (walk_chunk_topics)
STAGE = 480           # emits per flush record, first pass (EGM_WALK_STAGE)
REC_DIR = 64          # record offsets in a chunk's directory; a longer chunk continues along the chain
MIXED_FAN = 24        # copies of the fan-out topic in a loaded chunk: 24 x 1 534 ids > REC_DIR x STAGE


def mixed_chunk(c: Corpus, deep: bool, loaded: bool) -> np.ndarray:
    """64 topics, interleaved: 1-, 8-, 9- and 12-level topics, wildcard, '$',
    empty-word and zero-match topics and the fan-out topic (MIXED_FAN copies
    if loaded, else one); with `deep` also 13-level topics, which send the
    chunk to the deep pass."""
    lad = {D: c.t(J(ladder_words(D, 0))) for D in (1, 8, 9, 12, 13)}
    wild = [i for i in c.wild_present + c.wild_absent if c.depth[i] <= 12]
    w13 = [i for i in c.wild_present + c.wild_absent if c.depth[i] == 13]
    dollar, empty, zero = c.family("dollar"), c.family("empty"), [c.t(b"$u/v"), c.t(b"$u")]
    nfan = MIXED_FAN if loaded else 1
    slots = [c.t(J(FAN_TOPIC))] * nfan
    k = 0
    while len(slots) < CHUNK:
        group = [lad[1], lad[8], lad[9], lad[12], wild[k % len(wild)], dollar[k % len(dollar)], zero[k % len(zero)],
                 empty[k % len(empty)]]
        if deep:
            group += [lad[13], w13[k % len(w13)]]
        slots += group[:CHUNK - len(slots)]
        k += 1
    slots = np.array(slots, np.int64)
    return slots[(np.arange(CHUNK) * 37) % CHUNK]   # 37 is odd: a permutation that spreads the fan-out copies


def mixed_batch(c: Corpus, deep: bool, n_chunks: int = 2048, every: int = 128) -> np.ndarray:
    """n_chunks chunks of 64; every `every`-th one is loaded."""
    a, b = mixed_chunk(c, deep, True), mixed_chunk(c, deep, False)
    return np.concatenate([a if k % every == 0 else b for k in range(n_chunks)])
