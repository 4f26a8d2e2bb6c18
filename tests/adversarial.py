"""Adversarial inputs for the two hash tables every reader probes (egm_common.h):
colliding dictionary words (tests/golden/hash_collisions.json) and an edge
table whose probe chains are displaced, wrap the table end and run through
tombstones.  Shared by tests/test_hash_adversarial.py (host image + the walk
emulator) and tests/test_gpu_hash_adversarial.py (the kernels).

    python -m tests.adversarial        # search the salts again (prints candidates)
"""
import json
import os

import numpy as np

from emqx_amd.engine import TableImage, pack_strings
from oracle import trie_ref as R

NONE, TOMB = 0xFFFFFFFF, 0xFFFFFFFE
WID_MAX = 0xFFFFFFF0
SIG_SHIFT, SIG_BITS = 4, 28
M64 = (1 << 64) - 1

HERE = os.path.dirname(os.path.abspath(__file__))
WORD_CLASSES = ["w12", "w16", "w17", "w28", "w29", "w30", "w31"]


# ---- hashing restated (egm_common.h) ------------------------------------------
def mix64(x):
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & M64
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & M64
    x ^= x >> 33
    return x


def py_word_hash(data: bytes) -> int:
    h = 0xCBF29CE484222325
    for i in range(0, len(data), 4):   # the last chunk is zero-padded
        h = ((h ^ int.from_bytes(data[i:i + 4], "little")) * 0x100000001B3) & M64
    return mix64(h ^ ((len(data) & 0xFF) << 56))


def sig_index(wid: int) -> int:
    return (((mix64(0x9E3779B97F4A7C15 ^ wid) >> 32) * SIG_BITS) >> 32)


def sig_bit(wid: int) -> int:
    return 1 << (SIG_SHIFT + sig_index(wid))


# ---- the collision fixture ------------------------------------------------------
def load_collisions():
    """class -> [(a, b)] as bytes."""
    with open(os.path.join(HERE, "golden", "hash_collisions.json")) as fh:
        doc = json.load(fh)
    return {n: [(a.encode(), b.encode()) for a, b in p] for n, p in doc["classes"].items()}


def both_filters(a, b):
    """A table in which both colliding words are dictionary words."""
    return [a + b"/x", b + b"/y", a, b"+/" + b, a + b"/#", b"q/" + a + b"/" + b]


def one_filters(a, b):
    """both_filters without every filter that contains b."""
    return [f for f in both_filters(a, b) if b not in f.split(b"/")]


def pair_topics(a, b):
    return [a + b"/x", b + b"/x", a + b"/y", b + b"/y", a, b, b"z/" + b, b"q/" + a + b"/" + b, b"q/" + b + b"/" + a]


def image_loop(filters, ids=None):
    """The insert loop + relayout(): egm_table_build below the bulk threshold."""
    im = TableImage()
    for k, f in enumerate(filters):
        assert im.insert(f, k if ids is None else ids[k]) == 0, f
    im.relayout()
    return im


def image_bulk(filters, ids=None):
    im = TableImage()
    blob, off = pack_strings(filters)
    im.bulk_build(blob, off, None if ids is None else np.asarray(ids, np.uint32))
    return im


def expected(topic, fmap, mode):
    """Sorted filter ids the oracle returns; fmap: filter bytes -> id; mode 0 trie, 1 routes."""
    sem = R.routes_semantics if mode == 1 else R.trie_semantics
    return sorted(fmap[f] for f in sem(topic, list(fmap)))


# ---- displaced edge chains ------------------------------------------------------
N_P, N_O, N_DEEP = 200, 44, 4   # 2 + 200 + 44 + 4 = 250 literal edges: 256 lines of two slots, slot load 0.49
# Picked by search() below: the image conditions of the displaced-chain tests
# hold for this salt and these deleted children of p.  The tests assert them,
# so after a change of the hashes or of the table sizing: search again.
CHAIN_SALT = 738
CHAIN_DELETES = [9, 54, 141, 19, 8, 89, 80, 55]


class ChainCase:
    """Filters p/w<salt>_<i> (+ the same /#, so that reaching a child shows in
    both match modes), o/v<salt>_<j>, and a few deeper filters under the
    first N_DEEP children of p.  The filter id is the list index.

    Edge homes hash (parent node id, word id), not the words' bytes, so the
    salt also shapes the table: salt % 190 more children of p get a '+' child
    (every '+' node shifts the ids of p, o and their children by one,
    NODE_LAYOUT_VERSION 2) and an odd salt // 190 inserts o's filters first
    (other word ids)."""

    def __init__(self, salt):
        self.salt = salt
        self.pw = [b"w%d_%d" % (salt, i) for i in range(N_P)]
        self.ov = [b"v%d_%d" % (salt, j) for j in range(N_O)]
        fp = [b"p/" + w for w in self.pw] + [b"p/" + w + b"/#" for w in self.pw]
        fo = [b"o/" + v for v in self.ov] + [b"o/" + v + b"/#" for v in self.ov[:8]]
        f = fo + fp if (salt // 190) & 1 else fp + fo
        for w in self.pw[:N_DEEP]:
            f += [b"p/" + w + b"/+", b"p/" + w + b"/k", b"p/" + w + b"/+/#"]
        f += [b"p/" + w + b"/+" for w in self.pw[N_DEEP:N_DEEP + salt % 190]]
        self.filters = f
        self.fmap = {x: k for k, x in enumerate(f)}

    def delete_filters(self, idx):
        """The filters whose removal frees child idx of p (its edge slot becomes a tombstone)."""
        w = b"p/" + self.pw[idx]
        assert idx >= N_DEEP
        return [f for f in (w, w + b"/#", w + b"/+") if f in self.fmap]

    def image(self):
        return image_loop(self.filters)


def edge_chain_case(salt=None):
    return ChainCase(CHAIN_SALT if salt is None else salt)


def word_ids(a):
    """word bytes -> id, from the image's word store."""
    blob, off = a["dict_blob"].tobytes(), a["dict_off"]
    return {blob[int(off[k]):int(off[k + 1])]: k for k in range(len(off) - 1)}


def node_of(im, a, path):
    """Node reached from the root by the literal words of path (host-side probe)."""
    from tests.walk_emul import Emul
    e = Emul(im, a)
    n = 0
    for w in path:
        n = e.edge(n, e.word_id(w))[0]
        assert n != NONE, path
    return n


class Chains:
    """Where every live edge key sits relative to its home line."""

    def __init__(self, im, a):
        self.a = a
        e = a["edges"]
        self.nk = len(e) // (int(a["edge_mask"]) + 1)     # slots per bucket (EDGE_BUCKET)
        self.nlines = len(e) // 2                         # 64-B lines of two slots
        self.parent = e[:, 0].astype(np.int64)
        self.live = {}                                    # (parent, wid) -> (slot, home line, distance in lines)
        for s in np.nonzero((e[:, 0] != NONE) & (e[:, 0] != TOMB))[0].tolist():
            p, w = int(e[s, 0]), int(e[s, 1])
            home = (self.nk // 2) * im.edge_bucket(p, w, a["edge_mask"])
            self.live[(p, w)] = (s, home, (s // 2 - home) % self.nlines)
        self.im = im

    def home(self, p, w):
        return (self.nk // 2) * self.im.edge_bucket(p, w, self.a["edge_mask"])

    def wraps(self, key):
        s, home, d = self.live[key]
        return home + d >= self.nlines

    def chain_slots(self, key):
        """The slots a probe of the live key reads before it reaches the key's."""
        s, home, d = self.live[key]
        out, k = [], 2 * home
        while k != s:
            out.append(k)
            k = (k + 1) % (2 * self.nlines)
        return out

    def tombs_before(self, key):
        return [k for k in self.chain_slots(key) if self.parent[k] == TOMB]

    def line_full(self, line):
        return self.parent[2 * line] != NONE and self.parent[2 * line + 1] != NONE

    def absent_run(self, p, w):
        """Lines a probe of the absent key (p, w) reads past its home line
        (0: the home line has an empty slot); wraps: it passes the table end."""
        line, n = self.home(p, w), 0
        while self.line_full(line):
            n += 1
            line = (line + 1) % self.nlines
            assert n <= self.nlines
        return n, self.home(p, w) + n >= self.nlines


def absent_keys(case, im, a, ch):
    """[(topic, parent, wid, lines read past home, wraps)] for the absent
    (parent, word) pairs whose word is in the dictionary (it is a child of the
    other parent), whose signature bit is set at the parent (or the walk skips
    the probe) and whose home line is full."""
    wid = word_ids(a)
    pn, on = node_of(im, a, [b"p"]), node_of(im, a, [b"o"])
    out = []
    for par, node, words in ((b"p", pn, case.ov), (b"o", on, case.pw)):
        flags = int(a["nodes"][node, 3])
        for w in words:
            k = wid[w]
            if (node, k) in ch.live or not (flags & sig_bit(k)):
                continue
            n, wr = ch.absent_run(node, k)
            if n >= 1:
                out.append((par + b"/" + w, node, k, n, wr))
    return out


def chain_conditions(case, im=None):
    """The image conditions (a), (b), (d), (e) of the displaced-chain case:
    -> dict of the keys that witness each (empty list: the condition fails)."""
    im = im or case.image()
    a = im.arrays()
    ch = Chains(im, a)
    pn = node_of(im, a, [b"p"])
    mine = {k: v for k, v in ch.live.items() if k[0] == pn}
    ab = absent_keys(case, im, a, ch)
    return {
        "im": im, "a": a, "ch": ch, "p": pn,
        "far": [k for k, v in mine.items() if v[2] >= 2],
        "wrap": [k for k in mine if ch.wraps(k)],
        "absent_full": ab,
        "absent_wrap": [x for x in ab if x[4]],
    }


def topic_of_key(case, a, key):
    """p/<word> for a live key of node p."""
    blob, off = a["dict_blob"].tobytes(), a["dict_off"]
    return b"p/" + blob[int(off[key[1]]):int(off[key[1] + 1])]


def tomb_conditions(case, c, ch2):
    """Condition (c) on the image after the deletes (ch2): live keys of p with
    a tombstone earlier in their chain, and those among them that sit in slot 1
    of a line whose slot 0 is a tombstone."""
    behind = [k for k in ch2.live if k[0] == c["p"] and ch2.tombs_before(k)]
    s1 = [k for k in behind if ch2.live[k][0] % 2 == 1 and ch2.parent[ch2.live[k][0] - 1] == TOMB]
    return behind, s1


def pick_deletes(case, c):
    """Children of p (indices) to delete so that tombstones sit in front of
    live keys: slot 0 of the home line of displaced keys and of lines whose
    slot 1 is a key at home.  The witnesses of (a) and (b) stay."""
    ch, a = c["ch"], c["a"]
    wid = word_ids(a)
    idx_of = {wid[w]: i for i, w in enumerate(case.pw)}
    keep = set(c["far"][:2] + c["wrap"][:2])
    dels = []

    def try_del(slot):
        p, w = int(a["edges"][slot, 0]), int(a["edges"][slot, 1])
        if p != c["p"] or (p, w) in keep or idx_of.get(w, 0) < N_DEEP or idx_of[w] in dels:
            return False
        dels.append(idx_of[w])
        return True

    for k in list(keep):                          # a tombstone in front of a far / wrapped key
        for s in ch.chain_slots(k)[:1]:
            try_del(s)
    for k, (s, home, d) in sorted(ch.live.items(), key=lambda kv: kv[1][0]):
        if len(dels) >= 8:
            break
        if k[0] == c["p"] and s % 2 == 1 and d == 0 and k not in keep:   # slot 0 tombstone, slot 1 the key
            if try_del(s - 1):
                keep.add(k)
    return dels


def chain_topics(case):
    """Every child of p and of o, every word of one parent under the other
    (absent keys), and the deeper levels under some children."""
    t = [b"p/" + w for w in case.pw] + [b"o/" + v for v in case.ov]
    t += [b"p/" + v for v in case.ov] + [b"o/" + w for w in case.pw]
    for w in case.pw[:2 * N_DEEP] + case.pw[-2:]:
        t += [b"p/" + w + b"/k", b"p/" + w + b"/z", b"p/" + w + b"/z/k", b"p/" + w + b"/k/z"]
    return t + [b"p", b"o", b"p/k", b"k/" + case.pw[0], b"zz/" + case.pw[1]]


DEEP_TAIL = b"/k" + b"/d" * 12   # 13 more levels: a topic of 15, past the first pass's depth


def search(lo=0, hi=4000):   # pragma: no cover - run by hand when the hash or the table sizing changes
    for salt in range(lo, hi):
        case = ChainCase(salt)
        c = chain_conditions(case)
        if not (c["far"] and c["wrap"] and c["absent_full"] and c["absent_wrap"]):
            continue
        dels = pick_deletes(case, c)
        im = c["im"]
        for i in dels:
            for f in case.delete_filters(i):
                assert im.remove(f) == 0
        behind, s1 = tomb_conditions(case, c, Chains(im, im.arrays()))
        if behind and s1 and len(dels) >= 4:
            print("CHAIN_SALT =", salt, " CHAIN_DELETES =", dels, " far", len(c["far"]), "wrap", len(c["wrap"]),
                  "absent", len(c["absent_full"]), "absent wrap", len(c["absent_wrap"]), flush=True)


if __name__ == "__main__":   # pragma: no cover
    search()
