"""The kernels on the hard paths of the two hash tables: dictionary words
whose 64-bit hash and length collide (tests/golden/hash_collisions.json),
through every tokenise path, the heavy kernel, the ROUTES exact lookup, a
dictionary patch and the retained store; and an edge table with displaced,
wrapping and tombstoned probe chains (tests/adversarial.py), through the
first pass's continued probes, the deep pass, the heavy kernel and the exact
lookup.  Every result is compared exactly, as id sets, with the C++ oracle
(std::string keys: no hashing to collide) in both match modes, through
egm_match_device and egm_match_device_ordered."""
import numpy as np
import pytest

from emqx_amd import _lib as L
from emqx_amd.engine import GpuMatcher, pack_strings
from emqx_amd.retainer import RetainedStore
from oracle import retainer_ref as RR
from oracle.cpp import OracleTrie
from tests import adversarial as A
from tests.test_gpu_node_layout import MODES, build_bulk, check_both_paths

pytestmark = pytest.mark.gpu

COLL = A.load_collisions()
SORT_MIN_TOPICS = 16384   # egm_kernels.hip: from here on the batch is sorted (the wfix stride)
TOK_LDS, TOK_WORDS = 16256, 2528


@pytest.fixture(scope="module")
def gm():
    m = GpuMatcher(0)
    yield m
    m.close()


@pytest.fixture(autouse=True)
def sorted_walk(monkeypatch):
    monkeypatch.setenv("EGM_WALK_SORT_MIN_BYTES", "0")   # sort the batch whatever the table size


class Table:
    """A filter list with explicit ids, its oracle per mode, and the matcher built from it."""

    def __init__(self, filters, ids=None):
        self.filters = list(filters)
        self.ids = list(range(len(filters))) if ids is None else list(ids)
        self.blob, self.off = pack_strings(self.filters)

    def oracle(self, mode):
        o = OracleTrie(True, mode)
        o.add(self.blob, self.off, np.asarray(self.ids, np.uint32))
        return o

    def build(self, gm, bulk=False):
        if bulk:
            class F:
                blob, off = self.blob, self.off
            build_bulk(gm, F, np.asarray(self.ids, np.uint32))
        else:
            gm.build(self.blob, self.off, np.asarray(self.ids, np.uint32))

    def insert(self, gm, filters, ids):
        gm.apply(inserts=filters, insert_ids=ids)
        self.filters += filters
        self.ids += ids
        self.blob, self.off = pack_strings(self.filters)

    def delete(self, gm, filters):
        gm.apply(deletes=filters)
        keep = [k for k, f in enumerate(self.filters) if f not in set(filters)]
        self.filters = [self.filters[k] for k in keep]
        self.ids = [self.ids[k] for k in keep]
        self.blob, self.off = pack_strings(self.filters)

    def check(self, gm, topics, debug=0, want=None, spot=()):
        """Both modes, both device entry points.  The C++ oracle's rows are
        first pinned themselves: want: topic -> {mode: ids} written out by
        hand; spot: topics whose rows must equal the Python oracle's."""
        tb, to = pack_strings(topics)
        fmap = dict(zip(self.filters, self.ids))
        for mode in MODES:
            row, ids = self.oracle(mode).match(tb, to)
            pins = [(t, exp[mode]) for t, exp in (want or {}).items()] + [(t, A.expected(t, fmap, mode)) for t in spot]
            for t, exp in pins:
                k = topics.index(t)
                assert sorted(ids[int(row[k]):int(row[k + 1])].tolist()) == sorted(exp), (t, mode)
            check_both_paths(gm, tb, to, row, ids, mode, debug=debug)


def pair_tables(cls):
    a, b = COLL[cls][0]
    both = Table(A.both_filters(a, b) + [a + b"/+"], [100, 101, 102, 103, 104, 105, 106])
    one = Table(A.one_filters(a, b) + [a + b"/+"], [100, 102, 104, 106])
    return a, b, both, one


def filler(n, a, b):
    """Topics beside the ones under test: unknown words, known words at other levels, other depths."""
    out = []
    for k in range(n):
        r = k % 6
        out.append([b"fill%d/x" % k, a + b"/fill%d" % k, b"q/" + a + b"/n%d" % k, b"x/" + b, b"q/%d/" % k + b,
                    b"fill%d/x/y/%d/z" % (k, k)][r])
    return out


def lds_batch(a, b, n=600):
    sp = A.pair_topics(a, b) + [b"+/" + b, b"+/" + a, a + b"/+", b + b"/#"]   # the last four: wildcard topics
    fl = filler(n, a, b)
    step = n // len(sp)
    out = []
    for k, t in enumerate(sp):   # spread over the blocks and segments
        out += fl[k * step:(k + 1) * step] + [t]
    return out + fl[len(sp) * step:]


def exact_expect(a, b, table):
    """ROUTES exact lookup of wildcard topics: '+/b' is a filter of `both` only, '+/a' of neither."""
    has = b"+/" + b in table.filters
    return {b"+/" + b: {L.EGM_MODE_TRIE: [], L.EGM_MODE_ROUTES: [103] if has else []},
            b"+/" + a: {L.EGM_MODE_TRIE: [], L.EGM_MODE_ROUTES: []},
            b"z/" + b: {m: [103] if has else [] for m in MODES},
            a + b"/y": {L.EGM_MODE_TRIE: [104, 106], L.EGM_MODE_ROUTES: [104, 106]}}


@pytest.mark.parametrize("cls", A.WORD_CLASSES)
def test_collisions_lds_tokenise(gm, cls):
    """dict_resolve: several blocks and segments, both builders, and the ROUTES exact lookup."""
    a, b, both, one = pair_tables(cls)
    topics = lds_batch(a, b)
    for tab in (both, one):
        for bulk in (False, True):
            tab.build(gm, bulk)
            tab.check(gm, topics, want=exact_expect(a, b, tab))


@pytest.mark.parametrize("cls", A.WORD_CLASSES)
def test_collisions_sorted_batch(gm, cls):
    """SORT_MIN_TOPICS + 1 topics: word ids at the fixed stride, the walk in sorted order."""
    a, b, both, one = pair_tables(cls)
    topics = lds_batch(a, b, SORT_MIN_TOPICS + 1 - 13)
    assert len(topics) == SORT_MIN_TOPICS + 1
    for tab in (both, one):
        tab.build(gm)
        tab.check(gm, topics, want=exact_expect(a, b, tab))


@pytest.mark.parametrize("cls", A.WORD_CLASSES)
def test_collisions_long_topics(gm, cls):
    """dict_probe: a topic longer than the tokenise block's LDS (read from
    global memory) and one with more words than the block's word table."""
    a, b, both, one = pair_tables(cls)
    tail = b"h" * 17000
    words = b"w/" * 3000
    assert len(tail) > TOK_LDS and len(words) // 2 > TOK_WORDS
    topics = [b + b"/" + tail, a + b"/x", a + b"/" + tail, b + b"/" + words, a + b"/" + words, b + b"/y"]
    for tab in (both, one):
        tab.build(gm)
        tab.check(gm, topics, spot=topics, want={
            topics[0]: {m: [] for m in MODES},                            # not a's filters
            topics[2]: {m: [104, 106] for m in MODES},                    # 'a/#' and 'a/+'
            topics[3]: {m: [] for m in MODES},
            topics[4]: {m: [104] for m in MODES}})


@pytest.mark.parametrize("cls", A.WORD_CLASSES)
def test_collisions_heavy_kernel(gm, cls):
    a, b, both, one = pair_tables(cls)
    topics = lds_batch(a, b)
    for tab in (both, one):
        tab.build(gm)
        tab.check(gm, topics, debug=L.EGM_DEBUG_FORCE_HEAVY, want=exact_expect(a, b, tab))


@pytest.mark.parametrize("cls", A.WORD_CLASSES)
def test_collisions_incremental(gm, cls):
    """The colliding word arrives in a dictionary patch; then the first word's filters leave."""
    a, b, _, tab = pair_tables(cls)
    topics = lds_batch(a, b)
    tab.build(gm)
    tab.check(gm, topics)
    for k in range(2):   # both device copies hold the table: the next commit patches records, dict[] among them
        tab.insert(gm, [b"warm%d/+" % k], [300 + k])
        gm.commit()
    tab.insert(gm, [b + b"/y", b + b"/+"], [201, 202])
    gm.commit()
    tab.check(gm, topics, want={b + b"/y": {L.EGM_MODE_TRIE: [202], L.EGM_MODE_ROUTES: [201, 202]},
                                b + b"/x": {m: [202] for m in MODES},
                                a + b"/y": {m: [104, 106] for m in MODES}})
    tab.delete(gm, [a + b"/x", a, a + b"/#", b"q/" + a + b"/" + b])
    gm.commit()
    tab.check(gm, topics, want={b + b"/y": {L.EGM_MODE_TRIE: [202], L.EGM_MODE_ROUTES: [201, 202]},
                                a + b"/y": {m: [106] for m in MODES}})


@pytest.mark.parametrize("cls", A.WORD_CLASSES)
def test_collisions_retained_store(cls):
    a, b = COLL[cls][0]
    filters = [a + b"/+", b + b"/+", b"+/x", a + b"/x", b + b"/x", a + b"/#", b + b"/#", b"#"]
    store = RetainedStore(0)
    try:
        for stored in ([a + b"/x", b + b"/x"], [a + b"/x"]):
            store.clean()
            ref = RR.RetainedTable()
            for t in stored:
                store.store_retained(t, t)
                ref.store_retained(t, t)
            got = store.dispatch_batch(filters, 0)
            rows = store.match_ids(filters, 0, L.EGM_RMODE_MATCH)
            for f, g, r in zip(filters, got, rows):
                assert sorted(g) == sorted(ref.dispatch(f, 0)), (f, stored)
                assert sorted(store._msgs[int(i)][1] for i in r) == sorted(ref.match_messages(f, 0)), (f, stored)
            k = filters.index(b + b"/x")
            assert got[k] == ([b + b"/x"] if len(stored) == 2 else [])
            assert got[filters.index(b + b"/+")] == ([b + b"/x"] if len(stored) == 2 else [])
    finally:
        store.close()


# ---- displaced edge chains -------------------------------------------------------
MSG = "the image lost the condition: re-pick CHAIN_SALT (python -m tests.adversarial)"


def test_displaced_edge_chains(gm):
    case = A.edge_chain_case()
    c = A.chain_conditions(case)   # the host image, built as gm.build builds a table of this size
    im, a, ch = c["im"], c["a"], c["ch"]
    assert ch.nlines == 256 and a["n_edges"] == 250, MSG
    assert c["far"] and c["wrap"] and c["absent_full"] and c["absent_wrap"], MSG   # (a), (b), (d), (e)
    tab = Table(case.filters)
    tab.build(gm)
    assert gm.stats()["edges"] == a["n_edges"] and gm.stats()["nodes"] == a["n_live_nodes"]

    keys = c["far"] + c["wrap"]
    key_topics = [A.topic_of_key(case, a, k) for k in keys]
    hit = {t: {m: [case.fmap[t + b"/#"]] + ([case.fmap[t]] if m == L.EGM_MODE_ROUTES else []) for m in MODES}
           for t in key_topics}
    miss = {x[0]: {m: [] for m in MODES} for x in c["absent_full"][:4] + c["absent_wrap"]}
    sp = list(hit) + list(miss)
    topics = A.chain_topics(case)

    # first pass: continued probes (M_CONT items), their wrap, full home lines of absent keys
    tab.check(gm, topics, want={**hit, **miss}, spot=sp)
    assert gm.walk_counters()["slow_probes"] > 0

    # deep pass: the same keys from topics of 15 levels (edge_probe_from from slot 2 on)
    deep = [t + A.DEEP_TAIL for t in key_topics + list(miss)] + [b"p/" + w + A.DEEP_TAIL for w in case.pw[:8]]
    tab.check(gm, deep + topics[:64], spot=deep)
    assert all(A.expected(t + A.DEEP_TAIL, case.fmap, m) for t in key_topics for m in MODES)

    # the heavy kernel
    tab.check(gm, topics, debug=L.EGM_DEBUG_FORCE_HEAVY, want={**hit, **miss})

    # ROUTES exact lookup of wildcard topics through displaced and wrapped edges
    wild = [t + b"/+" for t in key_topics + list(miss)] + [t + b"/#" for t in key_topics]
    assert any(t in case.fmap for t in wild[:len(keys)])
    tab.check(gm, wild + topics[:32], spot=wild,
              want={t: {L.EGM_MODE_TRIE: [], L.EGM_MODE_ROUTES: [case.fmap[t]] if t in case.fmap else []} for t in wild})

    # the deletes as a delta: tombstones in front of live keys
    dels = [f for i in A.CHAIN_DELETES for f in case.delete_filters(i)]
    tab.delete(gm, dels)
    gm.commit()
    for f in dels:
        assert im.remove(f) == 0
    a2 = im.arrays()
    ch2 = A.Chains(im, a2)
    behind, slot1 = A.tomb_conditions(case, c, ch2)
    assert a2["edge_mask"] == a["edge_mask"] and behind and slot1, MSG   # (c)
    gone = [b"p/" + case.pw[i] for i in A.CHAIN_DELETES]
    bt = [A.topic_of_key(case, a2, k) for k in behind]
    want2 = {t: {m: [case.fmap[t + b"/#"]] + ([case.fmap[t]] if m == L.EGM_MODE_ROUTES else []) for m in MODES}
             for t in bt}
    want2.update({t: {m: [] for m in MODES} for t in gone})
    tab.check(gm, topics, want=want2, spot=list(want2))
    deep2 = [t + A.DEEP_TAIL for t in bt + gone]
    tab.check(gm, deep2 + topics[:64], spot=deep2)
    tab.check(gm, topics, debug=L.EGM_DEBUG_FORCE_HEAVY, want=want2)
    tab.check(gm, [t + b"/#" for t in bt + gone] + topics[:32])

    # two of them come back, into tombstone slots
    back = [case.delete_filters(i)[1] for i in A.CHAIN_DELETES[:2]]
    tab.insert(gm, back, [5000, 5001])
    gm.commit()
    tombs = set(np.nonzero(a2["edges"][:, 0] == A.TOMB)[0].tolist())
    for n, f in enumerate(back):
        assert im.insert(f, 5000 + n) == 0
    ch3 = A.Chains(im, im.arrays())
    new = set(ch3.live) - set(ch2.live)
    assert len(new) == 2 and {ch3.live[k][0] for k in new} <= tombs, MSG
    want3 = dict(want2)
    want3.update({f[:-2]: {m: [5000 + n] for m in MODES} for n, f in enumerate(back)})
    tab.check(gm, topics, want=want3, spot=list(want3))
    tab.check(gm, topics, debug=L.EGM_DEBUG_FORCE_HEAVY, want=want3)
