"""The node-id layout (egm_common.h NODE_LAYOUT_VERSION): after relayout() and
after a bulk build the root is node 0, the P nodes reached by a '+' word hold
the ids 1..P in the order a breadth-first walk from the root meets them, and
every other node follows from P+1 in that same order among themselves.

The breadth-first order is the builder's: a parent's children in the id order
they had BEFORE the layout (on a freshly inserted table, creation order).  The
checks therefore rank the trie of the image taken before the layout and look
every node up, by its path of words, in the image taken after it.  Matching
goes through the walk emulator against the Python oracle.  No GPU."""
import random

import numpy as np
import pytest

from emqx_amd.engine import TableImage, pack_strings
from oracle import trie_ref as R
from tests.test_capi_cpu import rand_filter, rand_topic
from tests.walk_emul import Emul

NONE, TOMB = 0xFFFFFFFF, 0xFFFFFFFE
PLUS, HASH = "+", "#"

TOPICS = [b"a", b"a/b", b"a/x/b", b"a/x/c", b"x", b"x/y", b"x/y/z/w", b"x/y/z/w/v", b"", b"/", b"$SYS/x", b"$x",
          b"$", b"$x/a/b", b"a/b/c/d", b"+", b"a/+/b", b"a/#"]


def children(a):
    """node -> [(token, child)], tokens '+', '#' or a word id, in child-id order."""
    kids = {}
    nodes, hc, e = a["nodes"], a["hash_child"], a["edges"]
    for n in np.nonzero(nodes[:, 0] != NONE)[0].tolist():
        kids.setdefault(n, []).append((PLUS, int(nodes[n, 0])))
    for n in np.nonzero(hc != NONE)[0].tolist():
        kids.setdefault(n, []).append((HASH, int(hc[n])))
    for s in e[(e[:, 0] != NONE) & (e[:, 0] != TOMB)].tolist():
        kids.setdefault(s[0], []).append((s[1], s[2]))
    for v in kids.values():
        v.sort(key=lambda x: x[1])
    return kids


def bfs(a):
    """[(path, id)] breadth-first from the root, siblings in id order; the root (path ()) first."""
    kids = children(a)
    out = [((), 0)]
    for path, n in out:   # grows while it is read
        for tok, c in kids.get(n, ()):
            out.append((path + (tok,), c))
    return out


def check_layout(pre, post):
    """post is pre laid out: returns P."""
    order = [p for p, _ in bfs(pre)]
    ids = dict(bfs(post))
    assert set(ids) == set(order), "the layout changed the trie"
    L = len(order)
    assert len(post["nodes"]) == L == post["n_live_nodes"], "dead nodes survive a layout"
    assert ids[()] == 0
    plus = [ids[p] for p in order[1:] if p[-1] == PLUS]
    rest = [ids[p] for p in order[1:] if p[-1] != PLUS]
    P = len(plus)
    pc = post["nodes"][:, 0]
    # the '+' children are exactly 1..P, no other node but the root has an id <= P
    assert set(pc[pc != NONE].tolist()) == set(range(1, P + 1))
    assert all(i > P for i in rest)
    # '+' children in the order the walk meets them; the others keep their relative order
    assert plus == list(range(1, P + 1))
    assert rest == list(range(P + 1, L))
    # reading plus_child of the nodes in BFS order: strictly ascending
    seen = [int(pc[ids[p]]) for p in order if pc[ids[p]] != NONE]
    assert all(x < y for x, y in zip(seen, seen[1:])) and len(seen) == P
    check_slots(post)
    return P


def check_slots(a):
    e = a["edges"]
    live = e[(e[:, 0] != NONE) & (e[:, 0] != TOMB)]
    assert np.array_equal(live[:, 4], a["nodes"][live[:, 2].astype(np.int64), 0]), "child_plus is stale"


def check_matching(im, live, extra=()):
    em = Emul(im, im.arrays())
    for t in list(TOPICS) + list(extra):
        for mode in (0, 1):
            got = em.match(t, mode)
            assert len(got) == len(set(got)), t
            want = R.trie_semantics(t, live.values()) if mode == 0 else R.routes_semantics(t, live.values())
            assert sorted(live[i] for i in got) == sorted(want), (t, mode)


def inserted(filters):
    im, live = TableImage(), {}
    for i, f in enumerate(filters):
        if im.insert(f, i) == 0:
            live[i] = f
    return im, live


def random_filters():
    rng = random.Random(5)
    return [rand_filter(rng) for _ in range(400)]


CASES = {
    "no_plus": ([b"a/b", b"a/#", b"c", b"$SYS/x", b"#", b"a/b/c/d"], 0),
    "single_plus": ([b"+"], 1),
    "plus_chain": ([b"+/+/+/+"], 4),
    "plus_beside_hash": ([b"a/+/b", b"a/#"], 1),
    "random": (random_filters(), None),
}


@pytest.mark.parametrize("name", list(CASES))
def test_layout_after_relayout_and_bulk_build(name):
    filters, want_p = CASES[name]
    im, live = inserted(filters)
    pre = im.arrays()
    im.relayout()
    post = im.arrays()
    P = check_layout(pre, post)
    assert want_p is None or P == want_p
    if name == "random":
        assert 20 < P < len(post["nodes"]) - 20
    if name == "plus_chain":   # each '+' child's '+' child is the next record of the region
        assert post["nodes"][:4, 0].tolist() == [1, 2, 3, 4]
    rng = random.Random(9)
    extra = [rand_topic(rng) for _ in range(40)]
    check_matching(im, live, extra)
    blob, off = pack_strings(filters)
    for threads in (1, 4):
        bi = TableImage()
        bi.bulk_build(blob, off, None, threads)
        b = bi.arrays()
        assert check_layout(pre, b) == P
        for k in ("nodes", "hash_child", "edges"):
            assert np.array_equal(post[k], b[k]), (k, threads)
        check_matching(bi, live, extra)


def test_layout_is_kept_on_a_second_relayout():
    """A relayout of a laid-out table ranks a '+' child before its siblings
    (id order), so it may renumber; the properties hold against that order."""
    im, live = inserted(random_filters())
    im.relayout()
    pre = im.arrays()
    im.relayout()
    check_layout(pre, im.arrays())
    check_matching(im, live)


def test_inserts_after_a_layout_are_appended_until_the_next_one():
    filters = list(dict.fromkeys(random_filters() + [b"q/+/r"]))
    im, live = inserted(filters)
    pre = im.arrays()
    im.relayout()
    a0 = im.arrays()
    P = check_layout(pre, a0)
    n0 = len(a0["nodes"])
    # remove a '+' filter (frees its private nodes), insert one that needs six new nodes
    assert im.remove(b"q/+/r") == 0
    live = {k: v for k, v in live.items() if v != b"q/+/r"}
    a1 = im.arrays()
    freed = set(range(n0)) - {i for _, i in bfs(a1)}
    assert 1 <= len(freed) <= 3
    new = b"n1/+/n2/+/n3/+"
    assert im.insert(new, 9000) == 0
    live[9000] = new
    a2 = im.arrays()
    old_plus = set(a1["nodes"][:, 0].tolist())
    new_plus = [c for c in a2["nodes"][:, 0].tolist() if c != NONE and c not in old_plus]
    assert len(new_plus) == 3
    # a new node reuses a freed id or is appended: the appended ones lie outside the dense region
    assert all(c in freed or c >= n0 for c in new_plus)
    appended = [c for c in new_plus if c >= n0]
    assert appended and all(c > P for c in appended)
    check_slots(a2)
    check_matching(im, live, [b"n1/x/n2/y/n3/z", b"n1/x/n2", b"q/x/r"])
    # the next relayout repacks: the dead nodes are gone, the new '+' children are in the region
    im.relayout()
    a3 = im.arrays()
    P3 = check_layout(a2, a3)
    assert len(a3["nodes"]) == len(bfs(a2))
    assert P3 == len([c for c in a2["nodes"][:, 0].tolist() if c != NONE])
    check_matching(im, live, [b"n1/x/n2/y/n3/z", b"n1/x/n2", b"q/x/r"])
