"""The retained store's incremental commits: puts on image
topics patched in place, deletes as tombstones, new topics in the device
overlay matched on bytes, clear_expired on the device -- every result against
oracle/retainer_ref.py as exact sorted sets, at now in {0, 1000, 1200} and in
both modes, with duplicate-free rows."""
import ctypes as C
import random

import pytest

from emqx_amd import _lib as L
from emqx_amd.retainer import RetainedStore
from oracle import retainer_ref as RR
from oracle import trie_ref as R
from tests.adversarial import load_collisions
from tests.test_gpu_retained import WORDS, _filter, _topic

pytestmark = pytest.mark.gpu

NOWS = (0, 1000, 1200)
EXPIRIES = (0, 500, 1000, 1500)
FIXED = [b"#", b"+", b"+/+", b"", b"/", b"$SYS/#", b"a/#", b"a/+", b"a/#/b", b"+/#"]


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
        self.s.store_retained(t, t, e)
        self.ref.store_retained(t, t, e)

    def delete(self, t):
        self.s.delete_message(t)
        self.ref.delete_message(t)

    def clean(self):
        self.s.clean()
        self.ref.clean()

    def clear_expired(self, now):
        """The topics the oracle removed; the store must return exactly their ids."""
        before = dict(self.ref.recs)
        self.ref.clear_expired(now)
        gone = sorted(before[k][0] for k in before.keys() - self.ref.recs.keys())
        by_id = {m: rec[0] for m, rec in self.s._msgs.items()}
        got = self.s.clear_expired(now)
        assert len(set(got)) == len(got)
        assert sorted(by_id[m] for m in got) == gone, now
        assert len(by_id) - len(got) == len(self.s._msgs)
        return gone

    def commit(self):
        self.s.commit()
        return self.s.last_commit()


def rows_of(store, filters):
    """{(now, mode): [sorted topics per filter]}; every id is the topic's current one."""
    out = {}
    for now in NOWS:
        for mode in (L.EGM_RMODE_MATCH, L.EGM_RMODE_DISPATCH):
            rows = []
            for f, row in zip(filters, store.match_ids(filters, now, mode)):
                ids = row.tolist()
                assert len(set(ids)) == len(ids), (f, now, mode)
                rows.append(sorted(store._msgs[i][0] for i in ids))
            out[now, mode] = rows
    return out


def parity(p, filters):
    got = rows_of(p.s, filters)
    for (now, mode), rows in got.items():
        for f, g in zip(filters, rows):
            exp = p.ref.match_messages(f, now) if mode == L.EGM_RMODE_MATCH else p.ref.dispatch(f, now)
            assert g == sorted(exp), (f, now, mode)
    assert p.s.size() == p.ref.size()
    return got


def base_topics(rng, n):
    return list(dict.fromkeys(_topic(rng) for _ in range(4 * n)))[:n]


def filters_for(rng, topics, n):
    return [_filter(rng, topics) for _ in range(n)] + FIXED


def test_patch_only(store):
    rng = random.Random(11)
    p = Pair(store)
    topics = base_topics(rng, 500)
    for t in topics:
        p.put(t, rng.choice(EXPIRIES))
    store.rebuild()
    st = store.last_commit()
    assert st["rebuilt"] == 1 and st["overlay_topics"] == 0 and st["dead_ranks"] == 0
    for t in rng.sample(topics, 50):
        p.put(t, rng.choice(EXPIRIES))
    st = p.commit()
    assert (st["rebuilt"], st["patched"], st["tombstoned"], st["overlay_topics"]) == (0, 50, 0, 0), st
    assert 0 < st["h2d_bytes"] <= 50 * 16
    parity(p, filters_for(rng, topics, 80) + rng.sample(topics, 40))


def test_tombstone_and_revive(store):
    rng = random.Random(12)
    p = Pair(store)
    topics = base_topics(rng, 500)
    for t in topics:
        p.put(t, rng.choice(EXPIRIES))
    store.rebuild()
    gone = rng.sample(topics, 50)
    for t in gone:
        p.delete(t)
    st = p.commit()
    assert (st["rebuilt"], st["patched"], st["tombstoned"], st["dead_ranks"]) == (0, 0, 50, 50), st
    rest = sorted(set(topics) - set(gone))
    rows = store.match_ids([b"#"] + gone, 0, L.EGM_RMODE_MATCH)
    assert sorted(store._msgs[int(i)][0] for i in rows[0]) == rest
    assert all(len(r) == 0 for r in rows[1:])
    filters = filters_for(rng, topics, 80) + gone
    parity(p, filters)
    p.put(gone[0], 1500)                      # the same rank comes back by a patch
    st = p.commit()
    assert (st["rebuilt"], st["patched"], st["dead_ranks"], st["overlay_topics"]) == (0, 1, 49, 0), st
    assert [store._msgs[int(i)][0] for i in store.match_ids([gone[0]], 0, L.EGM_RMODE_MATCH)[0]] == [gone[0]]
    parity(p, filters)


def special_topics(base):
    """New topics the image cannot express: unknown words, empty words, a
    prefix and an extension of an image topic, words past the dictionary's
    16-byte inline part."""
    have = set(base)
    deep = max(base, key=lambda t: t.count(b"/"))
    prefix = next(t.rsplit(b"/", k)[0] for t in sorted(base, key=len, reverse=True)
                  for k in (1, 2) if t.count(b"/") >= k and t.rsplit(b"/", k)[0] not in have)
    sp = [b"zebra/quagga", b"/okapi", b"okapi//a", b"okapi/", b"$SYS/okapi/x", b"solo", prefix, deep + b"/ext",
          b"q" * 17, b"a/" + b"q" * 18, b"a/" + b"w" * 17 + b"x", b"", b"a/zebra"]
    sp = [t for t in dict.fromkeys(sp) if t not in have]
    assert prefix in sp and len(sp) >= 10
    return sp


@pytest.mark.parametrize("P", [1, 63, 64, 65, 129])
def test_overlay_shapes(store, P):
    rng = random.Random(13)
    p = Pair(store)
    base = base_topics(rng, 300)
    for t in base:
        p.put(t, rng.choice(EXPIRIES))
    store.rebuild()
    new = special_topics(base)
    have = set(base) | set(new)
    while len(new) < P:       # words of the image and new ones, mixed
        t = b"/".join(rng.choice(WORDS + [b"nu%d" % rng.randint(0, 9)]) for _ in range(rng.randint(1, 6)))
        if t not in have:
            have.add(t)
            new.append(t)
    new = new[:P]
    for t in new:
        p.put(t, rng.choice(EXPIRIES))
    st = p.commit()
    assert (st["rebuilt"], st["overlay_topics"], st["patched"]) == (0, P, 0), st
    pool = base + new
    for n in (1, 64, 65):
        parity(p, filters_for(rng, pool, n) + rng.sample(new, min(P, 8)))
    # overlay topics are overwritten and deleted on the host; the list is uploaded again
    p.put(new[0], 1500)
    if P > 1:
        p.delete(new[-1])
    st = p.commit()
    assert (st["rebuilt"], st["overlay_topics"]) == (0, P - (P > 1)), st
    parity(p, filters_for(rng, pool, 20) + [new[0], new[-1]])


def test_overlay_hash_collisions(store):
    """Two words with one 64-bit hash and one length: the overlay compares
    bytes, so the stored word matches itself and never its partner."""
    p = Pair(store)
    for t in (b"a/b", b"hc/x", b"c"):
        p.put(t)
    store.rebuild()
    pairs = [ab for cls in load_collisions().values() for ab in cls]
    assert len(pairs) >= 16
    stored, filters = [], []
    for a, b in pairs:
        stored += [a, b"hc/" + a]
        filters += [a, b, b"hc/" + a, b"hc/" + b, b"+/" + b, b"+/" + a]
    for t in stored:
        p.put(t, 0)
    st = p.commit()
    assert (st["rebuilt"], st["overlay_topics"]) == (0, len(stored)), st
    got = parity(p, filters + FIXED)
    rows = dict(zip(filters, got[0, L.EGM_RMODE_MATCH]))
    for a, b in pairs:
        assert rows[a] == [a] and rows[b] == []
        assert rows[b"hc/" + a] == [b"hc/" + a] and rows[b"hc/" + b] == []


def test_overlay_only_store(store):
    rng = random.Random(14)
    p = Pair(store)
    for t in base_topics(rng, 40):
        p.put(t)
    store.rebuild()
    p.clean()
    new = [b"a", b"a/b", b"a/b/c", b"", b"/", b"$SYS/x", b"x//y", b"b/", b"w" * 18, b"a/b/c/d/e/f/g"]
    for t, e in zip(new, EXPIRIES * 3):
        p.put(t, e)
    st = p.commit()
    assert (st["rebuilt"], st["overlay_topics"], st["dead_ranks"]) == (0, 10, 0), st
    filters = filters_for(rng, new, 30) + new
    live = parity(p, filters)
    assert store.match_ids([b"#"], 0, L.EGM_RMODE_MATCH)[0].size == 10
    store.rebuild()
    st = store.last_commit()
    assert (st["rebuilt"], st["overlay_topics"]) == (1, 0), st
    assert parity(p, filters) == live
    # a store that was never cleaned or rebuilt lives in the overlay too
    s2 = RetainedStore(0)
    try:
        s2.store_retained(b"k/1", b"k/1", 0)
        s2.commit()
        st = s2.last_commit()
        assert (st["rebuilt"], st["overlay_topics"]) == (0, 1), st
        assert [s2._msgs[int(i)][0] for i in s2.match_ids([b"k/+"], 0, L.EGM_RMODE_MATCH)[0]] == [b"k/1"]
    finally:
        s2.close()


def test_cap_and_rebuild_rules(store):
    rng = random.Random(15)
    p = Pair(store)
    base = base_topics(rng, 100)
    for t in base:
        p.put(t, rng.choice(EXPIRIES))
    store.rebuild()
    store.set_overlay_cap(64)
    for i in range(64):
        p.put(b"cap/%d" % i, rng.choice(EXPIRIES))
    st = p.commit()
    assert (st["rebuilt"], st["overlay_topics"]) == (0, 64), st
    filters = filters_for(rng, base, 20) + [b"cap/+", b"cap/#", b"cap/7", b"cap/64"]
    parity(p, filters)
    p.put(b"cap/64", 0)                       # the 65th
    st = p.commit()
    assert (st["rebuilt"], st["overlay_topics"], st["dead_ranks"]) == (1, 0, 0), st
    parity(p, filters)
    # tombstones: 165 image topics; 82 dead ones are still fewer than the 83 alive
    image = base + [b"cap/%d" % i for i in range(65)]
    assert len(image) == 165
    for t in image[:82]:
        p.delete(t)
    st = p.commit()
    assert (st["rebuilt"], st["tombstoned"], st["dead_ranks"]) == (0, 82, 82), st
    parity(p, filters)
    p.delete(image[82])                       # 83 dead, 82 alive
    st = p.commit()
    assert (st["rebuilt"], st["dead_ranks"], st["overlay_topics"]) == (1, 0, 0), st
    parity(p, filters)
    # cap 0: every commit that changes anything rebuilds
    store.set_overlay_cap(0)
    for change in (lambda: p.put(image[100], 1500), lambda: p.put(b"fresh/topic", 0), lambda: p.delete(image[101])):
        change()
        st = p.commit()
        assert (st["rebuilt"], st["overlay_topics"], st["dead_ranks"], st["patched"]) == (1, 0, 0, 0), st
        parity(p, filters + [b"fresh/+"])


def expected_rows(ref, filters):
    """The oracle's rows for many filters over a large table: its own
    condition/1 and pattern_match, asked only about the keys whose length the
    pattern's first test admits; then its two alive rules."""
    by_len = {}
    for k, v in ref.recs.items():
        by_len.setdefault(len(k), []).append((k, v))
    out = {(now, mode): [] for now in NOWS for mode in (L.EGM_RMODE_MATCH, L.EGM_RMODE_DISPATCH)}
    for f in filters:
        pat = RR.condition(R.words(f))
        if isinstance(pat, RR.Tail):
            cand = [kv for n, kvs in by_len.items() if n >= len(pat.head) for kv in kvs]
        else:
            cand = by_len.get(len(pat), [])
        hit = [v for k, v in cand if RR.pattern_match(pat, list(k))]
        for now in NOWS:
            m = sorted(msg for msg, et in hit if et == 0 or et > now)
            out[now, L.EGM_RMODE_MATCH].append(m)
            out[now, L.EGM_RMODE_DISPATCH].append(m if R.wildcard(f) else sorted(ref.read_messages(f, now)))
    return out


def churn_round(rng, rnd, known, each, ref):
    """One round of test_incremental_equals_rebuild on every store in `each`."""
    fresh = []
    while len(fresh) < 60:
        t = b"/".join(rng.choice(WORDS + [b"r%d" % rnd, b"zz"]) for _ in range(rng.randint(1, 6)))
        if ref.key(t) not in ref.recs and t not in fresh:
            fresh.append(t)
    for t in fresh + rng.sample(known, 60):
        e = rng.choice(CHURN_EXPIRIES)
        each(lambda x: x.store_retained(t, t, e))
    known += fresh
    for t in rng.sample(known, 40):
        each(lambda x: x.delete_message(t))
    for f in (b"a/+/#", b"+/b"):
        each(lambda x: x.delete_message(f))


# Half of the records never expire, so that eight rounds of deletes and one
# clear_expired(501) per round leave the image with more live ranks than
# tombstones: the incremental store must get through without a rebuild.
CHURN_EXPIRIES = (0, 0, 0, 500, 1000, 1500)


def test_incremental_equals_rebuild():
    rng = random.Random(16)
    inc, full = RetainedStore(0), RetainedStore(0)
    try:
        full.set_overlay_cap(0)
        ref = RR.RetainedTable()

        def each(fn):
            for x in (inc, full, ref):
                fn(x)

        topics = base_topics(rng, 3000)
        for t in topics:
            e = rng.choice(CHURN_EXPIRIES)
            each(lambda x: x.store_retained(t, t, e))
        inc.rebuild()
        full.rebuild()
        known = list(topics)
        for rnd in range(8):
            churn_round(rng, rnd, known, each, ref)
            before = len(ref.recs)
            ref.clear_expired(501)
            n_gone = before - len(ref.recs)
            assert len(inc.clear_expired(501)) == n_gone and len(full.clear_expired(501)) == n_gone
            assert n_gone > 0
            inc.commit()
            assert inc.last_commit()["rebuilt"] == 0, (rnd, inc.last_commit())
            assert inc.size() == full.size() == ref.size()
            filters = [_filter(rng, known) for _ in range(600)]
            a, b = rows_of(inc, filters), rows_of(full, filters)
            assert a == b, rnd
            assert a == expected_rows(ref, filters), rnd
            for f in filters[:5] + [b"#"]:    # the shortcut above is the oracle's dispatch
                assert expected_rows(ref, [f])[1000, L.EGM_RMODE_DISPATCH][0] == sorted(ref.dispatch(f, 1000))
        st = inc.last_commit()
        assert st["overlay_topics"] > 0 and st["dead_ranks"] > 0, st
        assert full.last_commit()["rebuilt"] == 1
    finally:
        inc.close()
        full.close()


def test_clear_expired(store):
    rng = random.Random(17)
    p = Pair(store)
    now = 1000
    image = base_topics(rng, 200)
    for i, t in enumerate(image):
        p.put(t, (0, now - 1, now, now + 1)[i % 4])
    store.rebuild()
    over = [b"ov/%d" % i for i in range(70)] + [b"ov//", b"$SYS/ov"]
    for i, t in enumerate(over):
        p.put(t, (0, now - 1, now, now + 1)[i % 4])
    p.put(image[0], now - 1)                  # the patched expiry counts, not the image's
    p.put(image[1], now + 1)
    p.delete(image[5])                        # already deleted: not returned
    gone = p.clear_expired(now)
    assert set(gone) == {t for i, t in enumerate(image) if i % 4 == 1 and i not in (1, 5)} | {image[0]} | \
        {t for i, t in enumerate(over) if i % 4 == 1}
    assert store.size() == p.ref.size()
    st = store.last_commit()
    assert st["rebuilt"] == 0
    alive0 = store.match_ids([b"#"], 0, L.EGM_RMODE_MATCH)[0]      # at now = 0 an expired record would be alive
    left = sorted(store._msgs[int(i)][0] for i in alive0)
    assert left == sorted(p.ref.match_messages(b"#", 0)) and not set(left) & set(gone)
    parity(p, filters_for(rng, image + over, 40) + gone[:20])
    assert p.clear_expired(now) == [] and store.clear_expired(now) == []
    assert sorted(p.clear_expired(now + 1)) == sorted(
        [t for i, t in enumerate(image) if i % 4 == 2] + [t for i, t in enumerate(over) if i % 4 == 2])
    parity(p, filters_for(rng, image + over, 40))


def test_argument_checks(store):
    lib, h = store.lib, store.h
    assert lib.egm_rstore_put(h, b"a/b", 3, 0xFFFFFFFF, 0) == L.EGM_E_INVAL
    assert lib.egm_rstore_put(h, b"a/b", 3, 0xFFFFFFFE, 0) == L.EGM_OK
    assert store.size() == 1
    rb, v = C.c_int(), [C.c_uint64() for _ in range(5)]
    refs = [C.byref(rb)] + [C.byref(x) for x in v]
    assert lib.egm_rstore_last_commit(None, *refs) == L.EGM_E_INVAL
    for k in range(6):
        args = list(refs)
        args[k] = None
        assert lib.egm_rstore_last_commit(h, *args) == L.EGM_E_INVAL, k
    assert lib.egm_rstore_last_commit(h, *refs) == L.EGM_OK
    ids, n = L._u32p(), C.c_uint64()
    assert lib.egm_rstore_clear_expired(None, 5, C.byref(ids), C.byref(n)) == L.EGM_E_INVAL
    assert lib.egm_rstore_clear_expired(h, 5, None, C.byref(n)) == L.EGM_E_INVAL
    assert lib.egm_rstore_clear_expired(h, 5, C.byref(ids), None) == L.EGM_E_INVAL
    assert lib.egm_rstore_rebuild(None) == L.EGM_E_INVAL
    assert lib.egm_rstore_set_overlay_cap(None, 4) == L.EGM_E_INVAL
    assert lib.egm_rstore_clear_expired(h, 5, C.byref(ids), C.byref(n)) == L.EGM_OK
    assert n.value == 0 and not ids
    assert store.size() == 1
