"""Dispatch on the device (egm_subs_set_dead, egm_share_*, egm_dispatch_*):
the liveness check of emqx_broker:dispatch/2 (emqx_broker.erl:297-302), the
$share member pick (emqx_shared_sub.erl:239-290) and the per-filter route
counts (emqx_broker.erl:283-295) done by k_disp_resolve on the compact
fan-out's deliveries.

* the Broker mirror with device_dispatch=True returns exactly what its host
  path returns for the two hash strategies (and both agree with the oracle);
* hand-built subscriber rows and match CSRs at the window, inline-record,
  FAN_BIG, shard-threshold and group-size edges, element for element against
  a numpy/Python model of the host lists;
* the strategies' own properties (round robin's even spread and persistent
  cursor, sticky's stickiness, random's determinism);
* liveness updates, share deltas and commits, capacity overflow, argument
  errors.
"""
import random
import zlib

import numpy as np
import pytest

from emqx_amd import _lib as L
from emqx_amd.broker import Broker
from emqx_amd.engine import GpuMatcher
from oracle import trie_ref as R
from tests.test_capi_cpu import rand_filter, rand_topic

pytestmark = pytest.mark.gpu
GB = L.GROUP_BIT
NONE = L.EGM_SUB_NONE
CAP = 1 << 16
SENTINEL = 0xABABABAB


def _dev(a, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt).view({4: np.int32, 8: np.int64}[np.dtype(dt).itemsize])
                            ).to(torch.device("cuda:0"))


def _host(t, dt):
    return t.cpu().numpy().view(dt)


def dispatch(gm, mrow, mids, keys=None, strategy="hash_clientid", seed=0, cap=CAP, stream=None, sync=True):
    """egm_dispatch_device on a host-built match CSR; every output is filled
    with SENTINEL on the launch stream first.  Returns the device tensors'
    host copies (after a sync) or, sync=False, a function that does."""
    import torch
    n, nids = len(mrow) - 1, len(mids)
    s = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(s):
        t_mrow, t_mids = _dev(mrow, np.uint64), _dev(np.append(mids, 0), np.uint32)
        t_key = None if keys is None else _dev(keys, np.uint32)
        t_drow = _dev(np.zeros(n + 1), np.uint64)
        t_pos = _dev(np.full(nids + 1, SENTINEL), np.uint64)
        t_sub = _dev(np.full(cap + 64, SENTINEL), np.uint32)
        t_live = _dev(np.full(nids + 1, SENTINEL), np.uint32)
        t_sh = _dev(np.full(nids + 1, SENTINEL), np.uint32)
    gm.dispatch_device(t_mrow.data_ptr(), t_mids.data_ptr(), nids, n, 0 if t_key is None else t_key.data_ptr(),
                       L.PICK[strategy], seed, s.cuda_stream, t_drow.data_ptr(), t_pos.data_ptr(), t_sub.data_ptr(),
                       cap, t_live.data_ptr(), t_sh.data_ptr())

    def read():
        s.synchronize()
        keep = (t_mrow, t_mids, t_key)   # alive until the kernels have run
        del keep
        return {"drow": _host(t_drow, np.uint64), "pos": _host(t_pos, np.uint64)[:nids + 1],
                "sub": _host(t_sub, np.uint32), "live": _host(t_live, np.uint32)[:nids],
                "shared": _host(t_sh, np.uint32)[:nids]}

    return read() if sync else read


def compact(gm, mrow, mids, cap=CAP):
    import torch
    n, nids = len(mrow) - 1, len(mids)
    t_mrow, t_mids = _dev(mrow, np.uint64), _dev(np.append(mids, 0), np.uint32)
    t_drow, t_pos = _dev(np.zeros(n + 1), np.uint64), _dev(np.zeros(nids + 1), np.uint64)
    t_sub = _dev(np.zeros(cap), np.uint32)
    gm.fanout_device_compact(t_mrow.data_ptr(), t_mids.data_ptr(), nids, n, torch.cuda.current_stream().cuda_stream,
                             t_drow.data_ptr(), t_pos.data_ptr(), t_sub.data_ptr(), cap)
    torch.cuda.synchronize()
    return {"drow": _host(t_drow, np.uint64), "pos": _host(t_pos, np.uint64), "sub": _host(t_sub, np.uint32)}


def subs_build(gm, rows):
    row = np.zeros(len(rows) + 1, dtype=np.uint64)
    row[1:] = np.cumsum([len(x) for x in rows])
    gm.subs_build(row, np.fromiter((s for x in rows for s in x), dtype=np.uint32, count=int(row[-1])))


def one_topic_per_entry(mids):
    return np.arange(len(mids) + 1, dtype=np.uint64), np.asarray(mids, dtype=np.uint32)


# ---------------------------------------------------------------- 1. parity ----
def _scenario(strategy, device_dispatch):
    rng = random.Random(17)
    br = Broker(shared_strategy=strategy, device_dispatch=device_dispatch)
    o = R.Router()
    subs = {}
    fl = list(dict.fromkeys(rand_filter(rng) for _ in range(120)))
    sid = 0
    for f in fl:
        if rng.random() < 0.8:
            for _ in range(rng.randint(1, 3)):
                br.subscribe(f, sid, clientid=b"c%d" % sid)
                subs.setdefault(f, []).append(sid)
                sid += 1
            o.do_add_route(f, ("node", "local"))
        if rng.random() < 0.2:
            g = b"g%d" % rng.randint(0, 2)
            for _ in range(rng.randint(1, 5)):
                br.subscribe(b"$share/" + g + b"/" + f, sid)
                sid += 1
            o.do_add_route(f, ("group", g))
    for x in rng.sample(range(sid), sid // 4):
        br.kill(x)
    topics = [rand_topic(rng) for _ in range(300)]
    clients = [b"pub%d" % rng.randint(0, 40) for _ in topics]
    return br, o, subs, topics, clients


@pytest.mark.parametrize("strategy", ["hash_clientid", "hash_topic"])
def test_device_path_equals_host_path(strategy):
    """test_publish_result_random_vs_oracle's scenario (120 random filters, 300
    topics, a quarter of the subscribers killed, groups g0..g2 of 1-5 members)
    built twice: the device path's publish_batch and publish_result_batch
    return what the host path returns, metrics included.  (The host path's
    publish_batch expands to every subscriber whatever its liveness and only
    publish_result counts the live ones; the device path follows it in both.)"""
    host, o, subs, topics, clients = _scenario(strategy, False)
    devb = _scenario(strategy, True)[0]
    assert devb.dead == host.dead and len(host.dead) > 20
    got_h = host.publish_batch(topics, clients)
    got_d = devb.publish_batch(topics, clients)
    n_group = 0
    for t, h, d in zip(topics, got_h, got_d):
        assert sorted(d, key=repr) == sorted(h, key=repr), t
        want = R.deliveries(o, subs, t)
        assert set(x[:3] for x in h) == want and set(x[:3] for x in d) == want, t
        n_group += sum(1 for x in d if x[0] == "group")
    assert n_group > 10
    assert devb.last_dispatch["missing_groups"] == 0
    res_h = host.publish_result_batch(topics, clients)
    res_d = devb.publish_result_batch(topics, clients)
    assert res_d == res_h
    assert devb.metrics == host.metrics and host.metrics["messages.dropped"] > 0
    assert devb.last_dispatch["dead_dropped"] > 0
    # membership churn between publishes goes in as share deltas: still the host path's picks
    for b in (host, devb):
        (g, f), mem = next((k, v) for k, v in b.shared.items() if len(v) >= 3)
        b.unsubscribe(b"$share/" + g + b"/" + f, mem[1])
        b.subscribe(b"$share/" + g + b"/" + f, 90001)
        b.subscribe(b"$share/" + g + b"/" + f, mem[0])   # already a member: nothing
        b.subscriber_down(next(iter(sorted(b.dead))))
    assert devb.publish_result_batch(topics, clients) == host.publish_result_batch(topics, clients)
    for h, d in zip(host.publish_batch(topics, clients), devb.publish_batch(topics, clients)):
        assert sorted(d, key=repr) == sorted(h, key=repr)
    assert devb.metrics == host.metrics


# ------------------------------------------------------- 2. boundary shapes ----
PLAIN = (0, 1, 3, 4, 127, 128, 129, 1100)       # inline record, first table read, FAN_BIG, the 1024 shard threshold
GSIZES = (1, 2, 63, 64, 65, 200)                # one lane up to 64 members, the whole wave beyond
PATTERNS = ("all", "first", "last", "none")


class Shapes:
    """Filters 0-7: PLAIN[k] subscribers, dead at positions 0, 2, 3 and last;
    8: five subscribers, all dead; 9-14: two plain subscribers (one dead) and
    four group entries of GSIZES[k] members, one per liveness pattern; 15: a
    plain subscriber and a group entry whose key the share table lacks."""

    def __init__(self):
        self.rows, self.dead, self.share = [], set(), {}
        for k, c in enumerate(PLAIN):
            row = [k * 2000 + j for j in range(c)]
            self.dead |= {row[p] for p in (0, 2, 3, c - 1) if 0 <= p < c}
            self.rows.append(row)
        self.rows.append([17000 + j for j in range(5)])
        self.dead |= set(self.rows[8])
        for k, size in enumerate(GSIZES):
            fid, row = 9 + k, [20000 + 10 * k, 20001 + 10 * k]
            self.dead.add(row[1])
            for p, pat in enumerate(PATTERNS):
                gid = 4 * k + p
                mem = [100000 + 256 * gid + j for j in range(size)]
                alive = {"all": mem, "first": mem[:1], "last": mem[-1:], "none": []}[pat]
                self.dead |= set(mem) - set(alive)
                self.share[(fid, gid)] = mem
                row.insert(1 + p // 2, GB | gid)      # group entries between and after the plain ones
            self.rows.append(row)
        self.rows.append([30000, GB | 99])

    def install(self, gm):
        subs_build(gm, self.rows)
        gm.share_build([(f, g, m) for (f, g), mem in self.share.items() for m in mem])
        gm.subs_set_dead(sorted(self.dead), True)

    def csr(self, total):
        """`total` match entries over topics with an empty row first, in the middle and last."""
        mids = np.array([(k * 7 + 13) % 16 for k in range(total)], dtype=np.uint32)
        sizes, left, k = [], total, 0
        while left:
            c = min(left, (1, 3, 2, 5, 70)[k % 5])
            sizes.append(c)
            left -= c
            k += 1
        sizes.insert(len(sizes) // 2, 0)
        sizes = [0] + sizes + [0]
        mrow = np.zeros(len(sizes) + 1, dtype=np.uint64)
        mrow[1:] = np.cumsum(sizes)
        return mrow, mids

    def expect(self, mrow, mids, keys):
        sub, live, shared, pos = [], [], [], [0]
        st = dict(dead_dropped=0, groups_resolved=0, groups_empty=0, missing_groups=0)
        for t in range(len(mrow) - 1):
            for i in range(int(mrow[t]), int(mrow[t + 1])):
                fid, nl, ns = int(mids[i]), 0, 0
                for s in self.rows[fid]:
                    if not s & GB:
                        nl += s not in self.dead
                        st["dead_dropped"] += s in self.dead
                        sub.append(NONE if s in self.dead else s)
                    elif (fid, s & ~GB) not in self.share:
                        st["missing_groups"] += 1
                        sub.append(NONE)
                    else:
                        al = [m for m in self.share[(fid, s & ~GB)] if m not in self.dead]
                        st["groups_resolved" if al else "groups_empty"] += 1
                        ns += bool(al)
                        sub.append(al[int(keys[t]) % len(al)] if al else NONE)
                live.append(nl)
                shared.append(ns)
                pos.append(len(sub))
        return (np.array(sub, dtype=np.uint32), np.array(live, dtype=np.uint32), np.array(shared, dtype=np.uint32),
                np.array(pos, dtype=np.uint64), st)


@pytest.fixture(scope="module")
def shapes():
    sh = Shapes()
    gm = GpuMatcher(0)
    sh.install(gm)
    yield sh, gm
    gm.close()


@pytest.mark.parametrize("total", [1, 63, 64, 65, 129])
def test_boundary_shapes_match_the_host_lists(shapes, total):
    sh, gm = shapes
    mrow, mids = sh.csr(total)
    keys = np.random.default_rng(total).integers(0, 2 ** 32, len(mrow) - 1, dtype=np.uint64).astype(np.uint32)
    sub, live, shared, pos, st = sh.expect(mrow, mids, keys)
    got = dispatch(gm, mrow, mids, keys, "hash_clientid")
    assert gm.last_fanout() == {"deliveries": len(sub), "overflow": 0}
    assert np.array_equal(got["sub"][:len(sub)], sub)
    assert np.all(got["sub"][len(sub):] == SENTINEL)
    assert np.array_equal(got["live"], live) and np.array_equal(got["shared"], shared)
    assert gm.last_dispatch() == st
    raw = compact(gm, mrow, mids)
    assert np.array_equal(got["pos"], pos) and np.array_equal(raw["pos"], pos)
    assert np.array_equal(got["drow"], raw["drow"]) and np.array_equal(got["drow"], pos[mrow.astype(np.int64)])
    rs = raw["sub"][:len(sub)]
    plain_live = ((rs & GB) == 0) & ~np.isin(rs, np.fromiter(sh.dead, dtype=np.uint32))
    assert plain_live.sum() == live.sum() and np.array_equal(sub[plain_live], rs[plain_live])
    if total >= 63:   # every case of the docstring occurs
        assert all(v > 0 for v in st.values())
    # `hash` is hash_clientid
    assert np.array_equal(dispatch(gm, mrow, mids, keys, "hash")["sub"][:len(sub)], sub)


# ------------------------------------------------------------- 6. capacity ----
def test_capacity_overflow_writes_nothing_it_should_not(shapes):
    sh, gm = shapes
    mrow, mids = sh.csr(129)
    keys = np.arange(len(mrow) - 1, dtype=np.uint32)
    sub, live, shared, pos, st = sh.expect(mrow, mids, keys)
    total = len(sub)
    got = dispatch(gm, mrow, mids, keys, "hash_topic", cap=total - 1)
    assert gm.last_fanout() == {"deliveries": total, "overflow": 1}
    assert np.all(got["sub"][total - 1:] == SENTINEL)                       # nothing past deliv_cap
    assert np.all(got["live"] == SENTINEL) and np.all(got["shared"] == SENTINEL)
    assert gm.last_dispatch() == dict(dead_dropped=0, groups_resolved=0, groups_empty=0, missing_groups=0)
    assert np.array_equal(got["pos"], pos)                                  # the sizes are still reported
    got = dispatch(gm, mrow, mids, keys, "hash_topic", cap=total)
    assert gm.last_fanout() == {"deliveries": total, "overflow": 0}
    assert np.array_equal(got["sub"][:total], sub) and np.all(got["sub"][total:] == SENTINEL)
    assert np.array_equal(got["live"], live) and np.array_equal(got["shared"], shared)
    assert gm.last_dispatch() == st


def test_host_form_retries_on_capacity(shapes):
    """egm_dispatch_batch (its first guess is 2 x ids + 1024 deliveries)."""
    from emqx_amd.engine import MatchResult
    sh, gm = shapes
    mids = np.full(40, 7, dtype=np.uint32)           # 40 x 1100 subscribers
    mrow = np.array([0, 0, 25, 40], dtype=np.uint64)
    keys = np.array([5, 6, 7], dtype=np.uint32)
    sub, live, shared, pos, st = sh.expect(mrow, mids, keys)
    m = MatchResult(mrow, mids, np.zeros(3, np.uint8), 0, 0, 0, 0)
    d = gm.dispatch(m, keys, L.EGM_PICK_HASH_CLIENTID)
    assert np.array_equal(d["sub"], sub) and np.array_equal(d["entry_pos"], pos)
    assert np.array_equal(d["entry_live"], live) and np.array_equal(d["entry_shared"], shared)
    assert np.array_equal(d["row_ptr"], pos[mrow.astype(np.int64)])
    assert gm.last_dispatch() == st
    with pytest.raises(L.EgmError) as e:
        gm.dispatch(m, None, L.EGM_PICK_HASH_TOPIC)
    assert e.value.code == L.EGM_E_INVAL


# ----------------------------------------------------------- 3. strategies ----
MEMBERS = [10, 11, 12, 13]


def group_ctx(members=MEMBERS):
    gm = GpuMatcher(0)
    subs_build(gm, [[GB | 0]])
    gm.share_build([(0, 0, m) for m in members])
    return gm


def picks(gm, k, strategy, seed=0):
    """k deliveries of the group of filter 0 in one batch (64 entries per topic)."""
    mids = np.zeros(k, dtype=np.uint32)
    mrow = np.minimum(np.arange(0, k + 64, 64, dtype=np.uint64), k)
    if mrow[-1] != k:
        mrow = np.append(mrow, np.uint64(k))
    got = dispatch(gm, mrow, mids, None, strategy, seed)
    assert np.all(got["shared"] == 1) and np.all(got["live"] == 0)
    return got["sub"][:k]


def test_round_robin_spreads_evenly_and_keeps_its_cursor():
    gm = group_ctx()
    p = picks(gm, 4096, "round_robin")
    assert sorted(np.unique(p).tolist()) == MEMBERS
    assert all(int((p == m).sum()) == 1024 for m in MEMBERS)
    p = picks(gm, 6, "round_robin")          # cursor values 4096..4101
    assert sorted(p.tolist()) == [10, 10, 11, 11, 12, 13]
    gm.close()


def test_sticky_keeps_a_member_until_it_is_gone():
    gm = group_ctx()
    p = picks(gm, 4096, "sticky", seed=3)
    first = int(p[0])
    assert first in MEMBERS and np.all(p == first)
    assert np.all(picks(gm, 100, "sticky", seed=4) == first)
    gm.subs_set_dead([first], True)
    p = picks(gm, 4096, "sticky", seed=5)
    second = int(p[0])
    assert second in MEMBERS and second != first and np.all(p == second)
    assert np.all(picks(gm, 100, "sticky", seed=6) == second)
    gm.subs_set_dead([first], False)         # revived: the new one is kept
    assert np.all(picks(gm, 100, "sticky", seed=7) == second)
    gm.close()


def test_random_is_live_and_deterministic():
    def run(seed):
        gm = group_ctx()
        gm.subs_set_dead([12], True)
        out = [picks(gm, 4096, "random", seed), picks(gm, 500, "random", seed)]
        gm.close()
        return out
    a, b, c = run(1), run(1), run(2)
    for x in a + c:
        assert set(np.unique(x).tolist()) == {10, 11, 13}
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert not np.array_equal(a[0], c[0])
    assert not np.array_equal(a[0][:500], a[1])    # the dispatch sequence number is part of the pick
    assert min(int((a[0] == m).sum()) for m in (10, 11, 13)) > 1000   # 4096 / 3 = 1365 expected, sd 30


def test_random_and_sticky_in_a_group_the_wave_resolves():
    mem = list(range(500, 700))              # 200 members: the ballot path
    gm = group_ctx(mem)
    gm.subs_set_dead(mem[:150], True)
    p = picks(gm, 1000, "random", 9)
    assert set(p.tolist()) <= set(mem[150:]) and len(set(p.tolist())) > 40
    p = picks(gm, 1000, "round_robin")
    assert all(int((p == m).sum()) == 20 for m in mem[150:])
    p = picks(gm, 1000, "sticky", 9)
    assert int(p[0]) in mem[150:] and np.all(p == p[0])
    gm.close()


# ------------------------------------------------------ 4. liveness updates ----
def test_liveness_updates_and_bitmap_growth():
    gm = GpuMatcher(0)
    row = [0, 7, 5_000_000]
    subs_build(gm, [row])
    mrow, mids = one_topic_per_entry([0])

    def now():
        got = dispatch(gm, mrow, mids, None, "random")
        assert int(got["live"][0]) == int((got["sub"][:3] != NONE).sum())
        return got["sub"][:3].tolist()

    assert now() == row                                   # no bitmap at all: everybody is alive
    gm.subs_set_dead([0], True)
    assert now() == [NONE, 7, 5_000_000]
    gm.subs_set_dead([0], False)
    assert now() == row
    gm.subs_set_dead([0, 7], True)
    assert now() == [NONE, NONE, 5_000_000]               # 5 000 000 is past the bitmap: alive
    gm.subs_set_dead([5_000_000], False)                  # reviving an id past the bitmap: nothing to do
    assert now() == [NONE, NONE, 5_000_000]
    gm.subs_set_dead([5_000_000], True)                   # the bitmap grows between two dispatches
    assert now() == [NONE, NONE, NONE]
    assert gm.last_dispatch()["dead_dropped"] == 3
    gm.subs_set_dead([7, 5_000_000], False)
    assert now() == [NONE, 7, 5_000_000]
    with pytest.raises(L.EgmError) as e:                  # bit 31: refused, nothing applied
        gm.subs_set_dead([7, 0x80000001], True)
    assert e.value.code == L.EGM_E_INVAL
    assert now() == [NONE, 7, 5_000_000]
    gm.close()


# --------------------------------------------------------- 5. share deltas ----
def test_share_deltas_commits_and_streams():
    import torch
    gm = GpuMatcher(0)
    subs_build(gm, [[GB | 0], [GB | 1]])
    gm.share_build([(0, 0, 1), (0, 0, 2), (0, 0, 3), (0, 0, 2), (1, 1, 7), (1, 1, 8)])   # a duplicate is kept once

    def row_of(fid, k=8, read=True, stream=None):
        """The key's member row as the hash picks with keys 0..k-1 show it."""
        mrow, mids = one_topic_per_entry([fid] * k)
        got = dispatch(gm, mrow, mids, np.arange(k, dtype=np.uint32), "hash_clientid", stream=stream, sync=read)
        return got["sub"][:k].tolist() if read else got

    def cyc(mem, k=8):
        return [mem[i % len(mem)] for i in range(k)]

    def rr(fid):
        return int(dispatch(gm, *one_topic_per_entry([fid]), None, "round_robin")["sub"][0])

    assert row_of(0) == cyc([1, 2, 3]) and row_of(1) == cyc([7, 8])
    assert rr(1) == 7 and rr(0) == 1                       # cursors: key (1,1) -> 1, key (0,0) -> 1
    gm.share_apply_delta(add=[(0, 0, 4)])
    assert row_of(0) == cyc([1, 2, 3])                     # staged, not committed
    gm.share_commit()
    assert row_of(0) == cyc([1, 2, 3, 4])
    assert rr(1) == 8                                      # an untouched key's cursor continues across a commit
    gm.share_apply_delta(delete=[(0, 0, 2), (0, 0, 55)])   # a middle member; an absent one does nothing
    gm.share_commit()
    assert row_of(0) == cyc([1, 3, 4])
    assert rr(1) == 7
    with pytest.raises(L.EgmError) as e:                   # a triple in both lists: refused, nothing applied
        gm.share_apply_delta(add=[(0, 0, 9), (0, 0, 3)], delete=[(0, 0, 3)])
    assert e.value.code == L.EGM_E_INVAL
    with pytest.raises(L.EgmError):                        # a member id has bit 31 clear
        gm.share_apply_delta(add=[(0, 0, GB | 5)])
    gm.share_commit()
    assert row_of(0) == cyc([1, 3, 4])
    # a dispatch launched on a side stream before a commit returns the old membership
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    pending = row_of(0, read=False, stream=side)
    gm.share_apply_delta(add=[(0, 0, 6)], delete=[(0, 0, 1)])
    gm.share_commit()
    assert pending()["sub"][:8].tolist() == cyc([1, 3, 4])
    torch.cuda.synchronize()
    assert row_of(0) == cyc([3, 4, 6])
    # the last members of the key leave: the (filter, group) entry leaves the subscriber table
    gm.share_apply_delta(delete=[(0, 0, 3), (0, 0, 4), (0, 0, 6)])
    gm.share_commit()
    got = dispatch(gm, *one_topic_per_entry([0]), None, "random")   # the entry is still subscribed: a missing group
    assert got["sub"][0] == NONE and gm.last_dispatch()["missing_groups"] == 1
    gm.subs_apply_delta(delete=[(0, GB | 0)])
    gm.subs_commit()
    got = dispatch(gm, *one_topic_per_entry([0, 1]), None, "round_robin")
    assert got["pos"].tolist() == [0, 0, 1] and got["sub"][0] == 8 and got["shared"].tolist() == [0, 1]
    # added again it is a new key: a new slot, so its cursor starts afresh (the old one stood at 1)
    gm.subs_apply_delta(add=[(0, GB | 0)])
    gm.subs_commit()
    gm.share_apply_delta(add=[(0, 0, 5), (0, 0, 6)])
    gm.share_commit()
    assert row_of(0) == cyc([5, 6])
    assert rr(0) == 5 and rr(0) == 6 and rr(1) == 7
    gm.close()


def test_states_and_argument_errors():
    import torch
    gm = GpuMatcher(0)
    mrow, mids = one_topic_per_entry([0, 1])
    with pytest.raises(L.EgmError) as e:                   # before egm_subs_build
        dispatch(gm, mrow, mids, None, "random")
    assert e.value.code == L.EGM_E_STATE
    with pytest.raises(L.EgmError) as e:
        gm.last_dispatch()
    assert e.value.code == L.EGM_E_STATE
    subs_build(gm, [[3, GB | 0], [GB | 1, 4]])
    for strategy in ("hash", "hash_clientid", "hash_topic"):
        with pytest.raises(L.EgmError) as e:               # a hash strategy without keys
            dispatch(gm, mrow, mids, None, strategy)
        assert e.value.code == L.EGM_E_INVAL
    t = _dev(np.zeros(4), np.uint64)
    for strategy in (-1, 6):
        rc = gm.lib.egm_dispatch_device(gm.ctx, t.data_ptr(), t.data_ptr(), 0, 0, None, strategy, 0, None,
                                        t.data_ptr(), t.data_ptr(), t.data_ptr(), 0, t.data_ptr(), t.data_ptr())
        assert rc == L.EGM_E_INVAL
    torch.cuda.synchronize()
    # no share table: every group entry resolves to NONE and is counted as missing
    got = dispatch(gm, mrow, mids, None, "round_robin")
    assert got["sub"][:4].tolist() == [3, NONE, NONE, 4]
    assert got["live"].tolist() == [1, 1] and got["shared"].tolist() == [0, 0]
    assert gm.last_dispatch() == dict(dead_dropped=0, groups_resolved=0, groups_empty=0, missing_groups=2)
    # an empty batch
    got = dispatch(gm, np.zeros(3, dtype=np.uint64), np.zeros(0, dtype=np.uint32), None, "random")
    assert got["drow"].tolist() == [0, 0, 0] and gm.last_fanout() == {"deliveries": 0, "overflow": 0}
    gm.close()
