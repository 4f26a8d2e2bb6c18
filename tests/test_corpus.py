"""The boundary corpus (tests/corpus.py) on the CPU: its brute-force
expectation (oracle.trie_ref over the whole filter list: the reference of
record) against the C++ oracle and against the walk emulator over the host
table image, id for id in both modes, and the corpus's own invariants — the
families tests/test_gpu_path_matrix.py relies on are really there.  No GPU."""
import numpy as np
import pytest

from emqx_amd.engine import TableImage, pack_strings
from oracle import trie_ref as R
from oracle.cpp import OracleTrie
from tests import corpus as K
from tests.test_capi_cpu import image_of
from tests.walk_emul import Emul

MODES = [0, 1]
BRUTE_FORCE_BUDGET_S = 15.0


@pytest.fixture(scope="module")
def c():
    return K.build()


@pytest.fixture(scope="module")
def ref():
    return K.reference()


def test_corpus_shape(c, ref):
    print("corpus: %d filters, %d distinct topics, brute force %.1f s" % (len(c.filters), len(c.topics), ref.seconds))
    assert len(set(c.filters)) == len(c.filters) and 1500 < len(c.filters) < 3000
    assert len(set(c.topics)) == len(c.topics) < 1000
    assert ref.seconds < BRUTE_FORCE_BUDGET_S
    words = {w for f in c.filters for w in f.split(b"/")}
    assert {len(w) for w in words} >= {0, 1, 2, 4, 16, 17, 20}   # '' ... '$SYS' ... the long words


def test_every_ladder_depth_present_with_its_filters(c, ref):
    fid = {f: i for i, f in enumerate(c.filters)}
    for D in K.LADDER:
        w = K.ladder_words(D, 0)
        t = c.t(K.J(w))
        assert c.depth[t] == D and c.tags[t].startswith("ladder")
        trie = set(ref.sets[0][t])
        want = [w[:-1] + [K.PLUS], [K.PLUS] + w[1:], [K.PLUS] * D, w[:1] + [K.HASH], w + [K.HASH]]
        if D >= 3:
            want.append(w[:D // 2] + [K.PLUS] + w[D // 2 + 1:])
        for f in want:
            assert fid[K.J(f)] in trie, (D, K.J(f)[:40])
        assert fid[K.J(w)] not in trie and fid[K.J(w)] in ref.sets[1][t]      # the literal chain: ROUTES only
        # near misses: the last word differs, one level short, one level long
        last_plus, all_plus = fid[K.J(w[:-1] + [K.PLUS])], fid[K.J([K.PLUS] * D)]
        diff, long_ = c.t(K.J(w[:-1] + [b"z"])), c.t(K.J(K.ladder_words(D + 1, 0)))
        assert c.depth[diff] == D and c.depth[long_] == D + 1
        assert last_plus in ref.sets[0][diff]
        assert D == 1 or fid[K.J([K.PLUS] + w[1:])] not in ref.sets[0][diff]   # (D = 1: both are '+')
        assert all_plus not in ref.sets[0][long_] and last_plus not in ref.sets[0][long_]
        if D > 1:
            short = c.t(K.J(w[:-1]))
            assert c.depth[short] == D - 1 and all_plus not in ref.sets[0][short]
    depths = set(c.depth.tolist())
    assert depths >= set(K.LADDER) | {442}


def test_fanout_topic_has_the_derived_count(c, ref):
    """2^9 '+'-substitutions of k0/../k8 (one of them the topic itself: no
    wildcard, so ROUTES only) and 2^10 - 1 prefix-substitutions ending in '#'."""
    t = c.t(K.J(K.FAN_TOPIC))
    assert K.FAN_TRIE == 1534
    assert ref.count(0)[t] == K.FAN_TRIE and ref.count(1)[t] == K.FAN_TRIE + 1
    # its 8-level prefix: the prefix-substitutions of up to 8 levels, and the ladder's eight '+'
    assert ref.count(0)[c.t(K.J(K.FAN_TOPIC[:-1]))] == (2 ** 9 - 1) + 1
    assert ref.count(0)[c.t(K.J([b"$k0"] + K.FAN_TOPIC[1:]))] == 0 == ref.count(1)[c.t(b"$u/v")]


def test_wildcard_topics_have_an_excluded_name_match(c, ref):
    fid = {f: i for i, f in enumerate(c.filters)}
    for i in c.wild_present + c.wild_absent:
        t = c.topics[i]
        assert R.wildcard(t)
        named = [f for f in c.filters if f != t and R.match(t, f)]
        assert named, t[:40]                       # a filter matches it as a name ...
        assert ref.sets[0][i] == []                # ... TRIE returns nothing,
        assert ref.sets[1][i] == ([fid[t]] if i in c.wild_present else [])   # ROUTES only F == T
    assert {9, 13, 441} <= {int(c.depth[i]) for i in c.wild_present}
    assert {9, 13, 441} <= {int(c.depth[i]) for i in c.wild_absent}


def test_bait_is_armed_and_is_bait_for_the_kernel_only(c, ref):
    """A walker that read the neighbour's first words as the bait topic's
    levels D and D + 1 would match more filters: such filters exist for every
    pair.  The expectation of a topic is computed from that topic alone, so
    the neighbour (or dropping it) cannot change it."""
    assert {int(c.depth[b]) for b, _ in c.bait_pairs} == set(K.BAIT_DMAX)
    for b, nb in c.bait_pairs:
        t, nw = c.topics[b], c.topics[nb].split(b"/")
        assert nw[:2] == [b"z", b"y"]
        alone = sorted(R.trie_semantics(t, c.filters))
        assert alone == sorted(c.filters[i] for i in ref.sets[0][b])
        for extra in (nw[:1], nw[:2]):
            spill = set(R.trie_semantics(t + b"/" + K.J(extra), c.filters)) - set(alone)
            assert spill, (t, extra)


def test_mixed_chunk_exceeds_the_record_directory(c, ref):
    """The loaded mixed chunk's expected ids fill more than REC_DIR flush
    records at the default stage: 64 x its ids > 64 x 64 x 480."""
    for deep in (False, True):
        for mode in MODES:
            chunk = K.mixed_chunk(c, deep, True)
            ids = int(ref.count(mode)[chunk].sum())
            assert K.CHUNK * ids > K.CHUNK * K.REC_DIR * K.STAGE, (deep, mode, ids)
            assert int(c.depth[chunk].max()) == (13 if deep else 12)
            tags = {c.tags[i].split(":")[0] for i in chunk}
            assert tags >= {"ladder", "wild", "dollar", "zero", "fanout", "empty"}
            assert {1, 8, 9, 12} <= set(c.depth[chunk].tolist())
            assert ref.count(mode)[chunk].min() == 0 and ref.count(mode)[chunk].max() > 1500


@pytest.mark.parametrize("mode", MODES)
def test_cpp_oracle_agrees_id_for_id(c, ref, mode):
    o = OracleTrie(True, mode)
    o.add(*pack_strings(c.filters))
    blob, off = pack_strings(c.topics)
    row, ids = o.match(blob, off, threads=4)
    want_row, want_ids = ref.gather(mode, np.arange(len(c.topics)))
    assert np.array_equal(row, want_row)
    for i in range(len(c.topics)):
        assert sorted(ids[int(row[i]):int(row[i + 1])].tolist()) == ref.sets[mode][i], (mode, c.topics[i][:40])
    tot, vt = o.visited_counts(blob, off, threads=4)
    assert tot == int(vt.sum()) > 0
    wild = np.array([R.wildcard(t) for t in c.topics])
    assert np.all(vt[wild] == 0) and np.all(vt[~wild] >= 1)


@pytest.mark.parametrize("how", ["relayout", "bulk"])
def test_walk_emulator_over_the_table_image_agrees(c, ref, how):
    if how == "relayout":
        im, live = image_of(c.filters)
        assert len(live) == len(c.filters)
    else:
        im = TableImage()
        im.bulk_build(*pack_strings(c.filters), None, 4)
    em = Emul(im, im.arrays())
    blob, off = pack_strings(c.topics)
    vts = {}
    for mode in MODES:
        o = OracleTrie(True, mode)
        o.add(*pack_strings(c.filters))
        vts[mode] = o.visited_counts(blob, off, threads=4)[1]
    for i, t in enumerate(c.topics):
        for mode in MODES:
            got = em.match(t, mode)
            assert len(got) == len(set(got)), t[:40]
            assert sorted(got) == ref.sets[mode][i], (how, mode, t[:40])
            assert em.states == int(vts[mode][i]), (how, mode, t[:40])   # V_t: the kernels' `visited`
