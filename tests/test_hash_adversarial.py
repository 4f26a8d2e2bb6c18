"""The hard paths of the two hash tables, on the host image (no GPU): words
and filters whose 64-bit word_hash collides (tests/golden/hash_collisions.json)
and an edge table with keys lines away from home, a chain that wraps the table
end, tombstones in front of live keys and absent keys with a full home line
(tests/adversarial.py).  Results are compared, as id sets, with the Python
oracle (oracle/trie_ref.py) through the walk emulator (tests/walk_emul.py)."""
import random

import numpy as np
import pytest

from emqx_amd.engine import TableImage, pack_strings
from oracle.cpp import OracleTrie
from tests import adversarial as A
from tests.walk_emul import Emul, WID_NONE

COLL = A.load_collisions()
WORD_PAIRS = [(c, k) for c in A.WORD_CLASSES for k in range(len(COLL[c]))]
BUILDERS = {"loop": A.image_loop, "bulk": A.image_bulk}


def test_fixture_pairs_collide_and_the_hash_is_the_restated_one():
    assert set(COLL) == set(A.WORD_CLASSES) | {"f"}
    im = TableImage()
    alphabet = set(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789_-")
    for name, pairs in COLL.items():
        assert len(pairs) >= 3, name
        for a, b in pairs:
            assert a != b and len(a) == len(b), (name, a, b)
            assert im.word_hash(a) == im.word_hash(b) == A.py_word_hash(a) == A.py_word_hash(b), (name, a, b)
            if name == "f":
                assert a[:4] == b[:4] == b"a/b/" and a[-2:] == b[-2:] == b"/x" and len(a) == 18
                assert set(a[4:-2] + b[4:-2]) <= alphabet
            else:
                assert len(a) == int(name[1:]) and set(a + b) <= alphabet
    # what each class is for
    for a, b in COLL["w16"] + COLL["w17"]:
        assert a[:4] == b[:4] and a[:16] != b[:16]
    for c in ("w28", "w29", "w30", "w31"):
        for a, b in COLL[c]:
            assert a[:16] == b[:16]   # the dictionary slot's inline bytes cannot tell them apart
    rng = random.Random(7)
    for _ in range(1000):
        s = bytes(rng.randrange(256) for _ in range(rng.randint(0, 40)))
        assert im.word_hash(s) == A.py_word_hash(s), s


def check_topics(im, filters, ids, topics):
    a = im.arrays()
    em = Emul(im, a)
    fmap = dict(zip(filters, ids))
    for mode in (0, 1):
        for t in topics:
            assert sorted(em.match(t, mode)) == A.expected(t, fmap, mode), (t, mode)
    return em, a


@pytest.mark.parametrize("builder", sorted(BUILDERS))
@pytest.mark.parametrize("cls,k", WORD_PAIRS)
def test_word_collisions(cls, k, builder):
    a, b = COLL[cls][k]
    topics = A.pair_topics(a, b) + [b"+/" + b, b"+/" + a]
    both = A.both_filters(a, b)
    ids = [100 + i for i in range(len(both))]
    im = BUILDERS[builder](both, ids)
    em, arr = check_topics(im, both, ids, topics)
    wa, wb = em.word_id(a), em.word_id(b)
    assert wa != wb and WID_NONE not in (wa, wb)
    # two slots of dict[] with the colliding hash and length, one per word id
    d = arr["dict"]
    h = im.word_hash(a)
    same = d[(d[:, 0] == (h & 0xFFFFFFFF)) & (d[:, 1] == (h >> 32)) & (d[:, 2] != A.NONE)]
    assert sorted(same[:, 2].tolist()) == sorted([wa, wb]) and set(same[:, 3].tolist()) == {len(a)}
    one = A.one_filters(a, b)
    assert len(one) == 3
    im1 = BUILDERS[builder](one, ids[:3])
    em1, _ = check_topics(im1, one, ids[:3], topics)
    assert em1.word_id(b) == WID_NONE and em1.word_id(a) != WID_NONE


@pytest.mark.parametrize("k", range(len(COLL["f"])))
def test_filter_collisions(k):
    f, g = COLL["f"][k]
    topics = [f, g, f + b"/y", b"a/b"]
    im = TableImage()
    assert im.insert(f, 5) == 0
    assert im.remove(g) != 0                       # not the stored filter, whatever its hash
    assert im.arrays()["n_filters"] == 1
    check_topics(im, [f], [5], topics)
    assert im.insert(f, 9) == 1                    # the duplicate is still one
    assert im.insert(g, 6) == 0                    # new, not a duplicate
    assert im.arrays()["n_filters"] == 2
    check_topics(im, [f, g], [5, 6], topics)
    assert im.remove(g) == 0 and im.remove(g) != 0
    assert im.arrays()["n_filters"] == 1
    check_topics(im, [f], [5], topics)
    # bulk dedup: the first occurrence's id
    bl = TableImage()
    blob, off = pack_strings([f, g, f])
    bl.bulk_build(blob, off, np.asarray([11, 12, 13], np.uint32))
    assert bl.arrays()["n_filters"] == 2
    check_topics(bl, [f, g], [11, 12], topics)
    assert bl.insert(f, 14) == 1 and bl.insert(g, 15) == 1


# ---- displaced edge chains -------------------------------------------------------
@pytest.fixture(scope="module")
def chain():
    case = A.edge_chain_case()
    return case, A.chain_conditions(case)


def oracle_rows(filters, ids, topics, mode):
    o = OracleTrie(True, mode)
    fb, fo = pack_strings(filters)
    o.add(fb, fo, np.asarray(ids, np.uint32))
    tb, to = pack_strings(topics)
    row, out = o.match(tb, to)
    return [sorted(out[int(row[i]):int(row[i + 1])].tolist()) for i in range(len(topics))]


def check_chain_topics(im, fmap, special, topics):
    """The keys under test against the Python oracle, every topic against the C++ one."""
    a = im.arrays()
    em = Emul(im, a)
    filters, ids = list(fmap), list(fmap.values())
    for mode in (0, 1):
        for t in special:
            assert sorted(em.match(t, mode)) == A.expected(t, fmap, mode), (t, mode)
        for t, want in zip(topics, oracle_rows(filters, ids, topics, mode)):
            assert sorted(em.match(t, mode)) == want, (t, mode)


def test_displaced_edge_chains(chain):
    case, c = chain
    im, a, ch = c["im"], c["a"], c["ch"]
    msg = "the image lost the condition: re-pick CHAIN_SALT (python -m tests.adversarial)"
    assert ch.nlines == 256 and a["n_edges"] == 250, msg
    assert c["far"], msg                # (a) a live key two or more lines past home
    assert c["wrap"], msg               # (b) a live key whose chain wraps from the last line to line 0
    assert c["absent_full"], msg        # (d) an absent key, word known, signature bit set, home line full
    assert c["absent_wrap"], msg        # (e) one of them with a chain that wraps
    for k in c["wrap"]:
        assert ch.live[k][1] > ch.live[k][0] // 2
    special = [A.topic_of_key(case, a, k) for k in c["far"] + c["wrap"]]
    special += [x[0] for x in c["absent_full"][:8] + c["absent_wrap"]]
    assert all(A.expected(t, case.fmap, 0) for t in special[:len(c["far"]) + len(c["wrap"])])
    assert not any(A.expected(x[0], case.fmap, 1) for x in c["absent_full"])
    topics = A.chain_topics(case)
    check_chain_topics(im, case.fmap, special + [t + b"/k" for t in special] + [t + b"/+" for t in special], topics)

    # (c) tombstones in front of live keys
    fmap = dict(case.fmap)
    for i in A.CHAIN_DELETES:
        for f in case.delete_filters(i):
            assert im.remove(f) == 0
            del fmap[f]
    a2 = im.arrays()
    ch2 = A.Chains(im, a2)
    assert a2["edge_mask"] == a["edge_mask"] and int(np.count_nonzero(a2["edges"][:, 0] == A.TOMB)) == len(A.CHAIN_DELETES)
    behind, slot1 = A.tomb_conditions(case, c, ch2)
    assert behind and slot1, msg
    gone = [b"p/" + case.pw[i] for i in A.CHAIN_DELETES]
    special2 = [A.topic_of_key(case, a2, k) for k in behind] + gone
    assert all(A.expected(t, fmap, 0) for t in special2[:len(behind)])
    assert not any(A.expected(t, fmap, 1) for t in gone)
    check_chain_topics(im, fmap, special2, topics)

    # two deleted filters come back: into tombstone slots, the table is not rebuilt
    tombs = set(np.nonzero(a2["edges"][:, 0] == A.TOMB)[0].tolist())
    back = [case.delete_filters(i)[1] for i in A.CHAIN_DELETES[:2]]
    for n, f in enumerate(back):
        assert im.insert(f, 5000 + n) == 0
        fmap[f] = 5000 + n
    a3 = im.arrays()
    ch3 = A.Chains(im, a3)
    new = set(ch3.live) - set(ch2.live)
    assert len(new) == 2 and {ch3.live[k][0] for k in new} <= tombs and a3["edge_mask"] == a["edge_mask"]
    assert int(np.count_nonzero(a3["edges"][:, 0] == A.TOMB)) == len(A.CHAIN_DELETES) - 2
    check_chain_topics(im, fmap, special2 + [f[:-2] for f in back], topics)
