"""delete_message/2 with filters on the device (egm_rstore_delete_matching,
DESIGN §4.3) and the store's size limit (egm_rstore_set_max_retained).

Every delete runs on the store and on oracle/retainer_ref.py alike: the
returned ids are exactly the ids of the records the oracle removed, each once,
and the store answers matches like the oracle afterwards, in both modes, at a
clock (1000) that separates the expiries 500 / 1000 / 1500.  The size limit is
checked against the rule of emqx_retainer_mnesia.erl:75-99 stated in the test;
the oracle has no limit.
"""
import random

import pytest

from emqx_amd import _lib as L
from emqx_amd.retainer import RetainedStore
from oracle import retainer_ref as RR

pytestmark = pytest.mark.gpu

NOW = 1000
EXPIRIES = (0, 500, 1000, 1500)      # never, past, the clock itself (alive for read_messages only), future
WAVES = (63, 64, 65, 129)            # children of one parent: around one wave, and two waves and one
CHECK = [b"#", b"+/#", b"a/+", b"w65/#", b"$SYS/#", b"a/b", b"w129", b"ov/a"]


@pytest.fixture()
def store():
    s = RetainedStore(0)
    yield s
    s.close()


class Pair:
    """The store and the oracle, driven together; a message is its topic."""

    def __init__(self, store):
        self.s = store
        self.ref = RR.RetainedTable()

    def put(self, t, e=0):
        ok = self.s.store_retained(t, t, e)
        if ok:
            self.ref.store_retained(t, t, e)
        return ok

    def delete_matching(self, filters):
        """One device call for the batch; the oracle one delete_message per
        filter.  Returns the ids, checked against the records the oracle removed."""
        ids_of = dict(self.s._by_topic)
        before = dict(self.ref.recs)
        for f in filters:
            self.ref.delete_message(f)
        want = sorted(ids_of[before[k][0]] for k in before.keys() - self.ref.recs.keys())
        got = self.s.delete_matching(filters)
        assert len(set(got)) == len(got), filters
        assert sorted(got) == want, filters
        assert self.s.size() == self.ref.size()
        assert len(self.s._msgs) == self.ref.size() == len(self.s._by_topic)
        return got

    def parity(self, filters=CHECK):
        for mode in (L.EGM_RMODE_MATCH, L.EGM_RMODE_DISPATCH):
            for f, row in zip(filters, self.s.match_ids(filters, NOW, mode)):
                ids = row.tolist()
                assert len(set(ids)) == len(ids), (f, mode)
                exp = self.ref.match_messages(f, NOW) if mode == L.EGM_RMODE_MATCH else self.ref.dispatch(f, NOW)
                assert sorted(self.s._msgs[i][0] for i in ids) == sorted(exp), (f, mode)
        assert self.s.size() == self.ref.size()


def image_topics():
    """About 300 topics of 1-4 levels."""
    rng = random.Random(41)
    ts = [b"a", b"a/b", b"a/c", b"a/b/c", b"a/b/c/d", b"a//b", b"a/", b"/a", b"/", b"b", b"b/a", b"$SYS",
          b"$SYS/x", b"$SYS/x/y", b"$SYS/brokers/n1/uptime", b"$share/g/t"]
    for k in WAVES:
        ts.append(b"w%d" % k)
        ts += [b"w%d/c%d" % (k, i) for i in range(k)]
    ts += [b"w129/c5/x", b"w129/c5/x/y", b"w65/c64/z"]
    words = [b"a", b"b", b"c", b"x", b"", b"$SYS"]
    while len(set(ts)) < 360:
        ts.append(b"/".join(rng.choice(words) for _ in range(rng.randint(1, 4))))
    return sorted(set(ts) - {b""})


IMAGE = image_topics()
OVERLAY = ([b"ov", b"ov/a", b"ov/a/b", b"a/new", b"a/b/new", b"a/new/x/y", b"/new", b"new/", b"$SYS/new", b"$SYS/x/new",
            b"w65/new", b"w129/new", b"w129/c5/new", b"w63/c0/new"] + [b"ov/t%d" % i for i in range(26)])
assert len(OVERLAY) == 40 and not set(OVERLAY) & set(IMAGE)


def prepared(store):
    """The mixed state: an image, 40 overlay topics, 10 tombstones, 10 overwrites."""
    rng = random.Random(42)
    p = Pair(store)
    for t in IMAGE:
        p.put(t, rng.choice(EXPIRIES))
    store.rebuild()
    for t in OVERLAY:
        p.put(t, rng.choice(EXPIRIES))
    pool = [t for t in IMAGE if not t.startswith(b"w") and t not in (b"a", b"a/b", b"a/b/c")]
    picked = rng.sample(pool, 17)
    p.tombs = picked[:8] + [b"w64/c7", b"a/b/c"]         # 10 deletes: tombstones
    for t in p.tombs:
        store.delete_message(t)
        p.ref.delete_message(t)
    for t in picked[8:] + [b"w65/c64"]:                  # 10 overwrites: patches
        p.put(t, rng.choice(EXPIRIES))
    return p


def image_dead(p):
    """Tombstones of the image: its topics the oracle no longer holds."""
    return sum(1 for t in IMAGE if RR.RetainedTable.key(t) not in p.ref.recs)


FILTERS = [b"#", b"+/#", b"a/#", b"a/+", b"+", b"+/+/+", b"a/#/b", b"w65/+", b"w129/#", b"$SYS/#",
           b"w64/c3",      # a plain topic of the image
           b"ov/a",        # ... of the overlay
           b"no/such"]     # ... the store does not hold


@pytest.mark.parametrize("flt", FILTERS, ids=[f.decode() for f in FILTERS])
def test_parity_on_a_mixed_store(store, flt):
    p = prepared(store)
    size0 = p.ref.size()
    got = p.delete_matching([flt])
    if flt in (b"#", b"+/#"):
        assert len(got) == size0 and store.size() == 0
    if flt == b"a/#":
        assert RR.RetainedTable.key(b"a") not in p.ref.recs and len(got) > 3
    if flt == b"a/#/b":
        assert got == []
    if flt == b"w65/+":
        assert len(got) == 65 + 1            # the 65 children and the overlay's w65/new
    if flt in (b"w64/c3", b"ov/a"):
        assert len(got) == 1
    p.parity()
    # the delete tombstones on the device and stages nothing; the next commit
    # rebuilds only by the tombstone rule: dead ranks > live ranks of the image
    dead = image_dead(p)
    store.commit()
    st = store.last_commit()
    assert st["rebuilt"] == (1 if dead > len(IMAGE) - dead else 0), (st, dead)
    if flt in (b"#", b"+/#"):
        assert st["rebuilt"] == 1
    if flt in (b"a/+", b"w65/+", b"a/#/b", b"w64/c3", b"ov/a", b"no/such"):
        assert st["rebuilt"] == 0
        # a commit with nothing to apply leaves the report of the one before the delete
        ov_changed = any(store._by_topic.get(t) is None for t in OVERLAY)
        assert st["dead_ranks"] == (dead if ov_changed else len(p.tombs)), st
    p.parity()


def test_overlapping_filters_in_one_batch(store):
    p = prepared(store)
    n = p.ref.size()
    got = p.delete_matching([b"a/#", b"a/+", b"a/b", b"#"])
    assert len(got) == n and store.size() == 0
    assert all(len(r) == 0 for r in store.match_ids([b"#", b"a/b", b"ov"], 0, L.EGM_RMODE_DISPATCH))
    p.parity()


@pytest.mark.parametrize("committed", (True, False))
def test_expired_or_not(store, committed):
    """:209-211 has no expiry condition: a record long expired goes with `+` too."""
    p = Pair(store)
    p.put(b"old", 1)
    p.put(b"keep", 0)
    p.put(b"deeper/x", 1)
    if committed:
        store.rebuild()                      # the image; otherwise the overlay
    assert [len(r) for r in store.match_ids([b"+"], NOW, L.EGM_RMODE_MATCH)] == [1]   # `old` is expired for a match
    got = p.delete_matching([b"+"])
    assert len(got) == 2
    assert store.size() == 1
    p.parity([b"#", b"+", b"old", b"keep", b"deeper/x"])


def test_revival(store):
    p = prepared(store)
    got = p.delete_matching([b"w64/#"])
    assert len(got) == 65 - 1                # w64 and its children, less the tombstoned w64/c7
    store.commit()
    p.put(b"w64/c9", 1500)
    store.commit()
    st = store.last_commit()
    assert (st["rebuilt"], st["patched"], st["overlay_topics"]) == (0, 1, len(OVERLAY)), st
    assert st["dead_ranks"] == image_dead(p)
    mid = store._by_topic[b"w64/c9"]
    assert store.match_ids([b"w64/c9", b"w64/+"], NOW, L.EGM_RMODE_MATCH)[1].tolist() == [mid]
    p.parity(CHECK + [b"w64/#", b"w64/c9"])
    assert p.delete_matching([b"w64/#"]) == [mid]
    p.parity(CHECK + [b"w64/#", b"w64/c9"])


def test_empty_inputs(store):
    p = Pair(store)
    assert store.delete_matching([]) == []
    assert p.delete_matching([b"#", b"a/+", b"a"]) == []          # an empty store
    for i, t in enumerate(OVERLAY[:20]):                           # the overlay alone: never rebuilt
        p.put(t, EXPIRIES[i % 4])
    assert store.delete_matching([]) == []
    store.commit()
    assert store.last_commit()["rebuilt"] == 0
    assert len(p.delete_matching([b"a/+", b"nothing/#"])) == 1     # a/new
    p.parity()
    assert len(p.delete_matching([b"ov/#", b"ov/a", b"+/+"])) >= 10
    p.parity()
    p.delete_matching([b"#"])
    assert store.size() == 0
    store.commit()
    assert store.last_commit()["rebuilt"] == 0
    p.put(b"again", 0)
    p.parity([b"#", b"again"])


def test_delete_message_through_the_mirror(store, monkeypatch):
    p = prepared(store)
    calls = []
    real = store.lib.egm_rstore_delete
    monkeypatch.setattr(store, "_drop", lambda t: (calls.append(t), real(store.h, t, len(t))))
    store.delete_message(b"w63/+")           # a wildcard topic: one device call, no per-topic delete
    p.ref.delete_message(b"w63/+")
    assert calls == []
    assert b"w63/c1" not in store._by_topic and b"w63" in store._by_topic
    p.parity(CHECK + [b"w63/#", b"w63/c1"])
    monkeypatch.undo()
    store.delete_message(b"w63")             # a plain topic
    p.ref.delete_message(b"w63")
    assert b"w63" not in store._by_topic
    p.parity(CHECK + [b"w63/#", b"w63"])
    assert len(store._msgs) == p.ref.size()


def test_size_limit(store):
    """is_table_full/0 (:230-240) and store_retained/2 (:75-99): with
    table_size() >= Limit > 0, a topic without a record is not written
    (:92-97), a topic with one is overwritten (:85-91)."""
    def topics_of(flt):
        return sorted(store._msgs[i][0] for i in store.match_ids([flt], 0, L.EGM_RMODE_MATCH)[0].tolist())

    store.set_max_retained(3)
    for t in (b"l/a", b"l/b", b"l/c"):
        assert store.store_retained(t) is True
    assert store.size() == 3
    assert store.store_retained(b"l/d") is False
    assert store.size() == 3 and b"l/d" not in store._by_topic
    assert topics_of(b"#") == [b"l/a", b"l/b", b"l/c"] and topics_of(b"l/d") == []
    old = store._by_topic[b"l/b"]
    assert store.store_retained(b"l/b", b"again") is True         # a held topic: overwritten
    new = store._by_topic[b"l/b"]
    assert new != old and store.size() == 3
    assert store.match_ids([b"l/b"], 0, L.EGM_RMODE_MATCH)[0].tolist() == [new]
    store.rebuild()                                                # the same rule for topics of the image
    assert store.store_retained(b"l/d") is False
    assert store.store_retained(b"l/a", b"again") is True
    store.delete_message(b"l/a")
    assert store.size() == 2
    assert store.store_retained(b"l/d") is True                    # room again
    assert store.store_retained(b"l/a") is False                   # its rank is a tombstone: not held
    assert topics_of(b"#") == [b"l/b", b"l/c", b"l/d"]
    assert store.delete_matching([b"l/+"]) and store.size() == 0
    assert store.store_retained(b"l/a") is True
    store.set_max_retained(0)                                      # no limit
    for i in range(5):
        assert store.store_retained(b"m/%d" % i) is True
    assert store.size() == 6
    assert len(topics_of(b"#")) == 6


def test_past_the_small_scan_and_past_one_grid_pass(store):
    """The two sizes at which the kill takes another path: more than 65 536
    ranges (the scan of their lengths leaves its one-block form) and more than
    8192 x 256 covered ranks (a lane takes a second rank)."""
    n = 70_000
    topics = [b"big/%d/%d" % (i % 97, i) for i in range(n)]
    for i, t in enumerate(topics):
        assert store.store_retained(t, None, (0, 1, 1500)[i % 3])
    store.rebuild()
    plain = topics[:66_000]                                        # one single-rank range per filter
    want = sorted(store._by_topic[t] for t in plain)
    got = store.delete_matching(plain + plain[:500])               # 500 of them twice
    assert sorted(got) == want
    assert store.size() == n - len(plain)
    rest = sorted(store._by_topic[t] for t in topics[66_000:])
    assert sorted(store.match_ids([b"#"], 0, L.EGM_RMODE_MATCH)[0].tolist()) == rest
    assert store.last_commit()["rebuilt"] == 1                     # tombstones outnumbered the live ranks
    got = store.delete_matching([b"#", b"big/#", b"big/+/+"] * 200)   # 600 x 4000 ranks > 2 097 152
    assert sorted(got) == rest
    assert store.size() == 0 and not store._msgs
    assert store.match_ids([b"#"], 0, L.EGM_RMODE_MATCH)[0].tolist() == []
