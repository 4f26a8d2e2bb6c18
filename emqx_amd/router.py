"""Host mirror of ``emqx_router`` (apps/emqx/src/emqx_router.erl) on the GPU table.

The route table is a bag of ``Route(topic, dest)`` (apps/emqx/include/emqx.hrl:90-93).
``match_routes/1`` (:129-134) = the exact routes of the topic itself plus the
routes of every trie-matched wildcard filter.  Here one GPU table holds every
filter with at least one route, exact and wildcard alike, and the
EGM_MODE_ROUTES walk returns exactly that union in one pass; the host then
expands each matched filter to its destinations.

Route add/delete keep the reference's rules: a route is added once
(:116-117); a filter enters the table with its first route and leaves with its
last (:230-248).

``Router(device_routes=True)`` also keeps the route-node table on the GPU
(egm_routes_*): every dest that is a node (not a ``("group", G)`` tuple) gets a
small node id on first sight, the (filter id, node id) changes since the last
commit are published with the table commit, and ``cleanup_routes(node)``
(emqx_router_helper.erl:137-146) drops a node's routes in one device pass.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Dict, List, Optional, Sequence

from . import _lib as L
from .engine import GpuMatcher
from .topic import wildcard

Route = namedtuple("Route", "topic dest")


def _check_bin(x):
    if not isinstance(x, (bytes, bytearray)):
        raise TypeError("function_clause: topic must be a binary")
    return bytes(x)


class Router:
    def __init__(self, matcher: Optional[GpuMatcher] = None, device: int = 0, node: str = "local",
                 device_routes: bool = False):
        self.m = matcher or GpuMatcher(device)
        self.node = node
        self.routes: Dict[bytes, List[object]] = {}
        self._ids: Dict[bytes, int] = {}
        self._names: Dict[int, bytes] = {}
        self._next = 0
        self._dirty = False
        # the route-node table on the GPU (egm_routes_*): built at the first commit, then kept by deltas
        self.device_routes = device_routes
        self.node_ids: Dict[object, int] = {node: 0}
        self.node_names: List[object] = [node]
        self._r_built = False
        self._r_touched: Dict[tuple, None] = {}   # (filter id, node id) pairs changed since the last commit

    @staticmethod
    def is_node(dest) -> bool:
        """An atom dest of emqx_route (a node), not a {Group, Node} one."""
        return not (isinstance(dest, tuple) and len(dest) == 2 and dest[0] == "group")

    def node_id(self, dest) -> int:
        """The node id of a dest in the route-node table, assigned on first sight."""
        nid = self.node_ids.get(dest)
        if nid is None:
            if len(self.node_names) >= L.EGM_ROUTE_MAX_NODES:
                raise ValueError("more than EGM_ROUTE_MAX_NODES nodes")
            nid = self.node_ids[dest] = len(self.node_names)
            self.node_names.append(dest)
        return nid

    def _route_mask(self, fid: int) -> int:
        f = self._names.get(fid)
        return sum(1 << self.node_id(d) for d in self.routes.get(f, ()) if self.is_node(d)) if f is not None else 0

    def _commit_routes(self):
        if not self._r_built:
            import numpy as np
            masks = np.zeros(self._next, dtype=np.uint64)
            for fid in self._names:
                masks[fid] = self._route_mask(fid)
            self.m.routes_build(masks, 0)
            self._r_built = True
        elif self._r_touched:
            # each touched pair's net effect, read from the host lists
            add = [p for p in self._r_touched if self._route_mask(p[0]) >> p[1] & 1]
            dele = [p for p in self._r_touched if not self._route_mask(p[0]) >> p[1] & 1]
            self.m.routes_apply_delta(add=add, delete=dele)
            self.m.routes_commit()
        self._r_touched.clear()

    # -- table maintenance (emqx_router.erl:114-125,164-170,227-248) ----------
    def add_route(self, topic: bytes, dest=None) -> str:
        return self.do_add_route(topic, dest)

    def do_add_route(self, topic: bytes, dest=None) -> str:
        topic = _check_bin(topic)
        dest = self.node if dest is None else dest
        cur = self.routes.setdefault(topic, [])
        if dest in cur:
            return "ok"
        if not cur:
            fid = self._next
            self._next += 1
            self.m.apply(inserts=[topic], insert_ids=[fid])
            self._ids[topic] = fid
            self._names[fid] = topic
            self._dirty = True
        cur.append(dest)
        if self._r_built and self.is_node(dest):
            self._r_touched[(self._ids[topic], self.node_id(dest))] = None
        return "ok"

    def delete_route(self, topic: bytes, dest=None) -> str:
        return self.do_delete_route(topic, dest)

    def do_delete_route(self, topic: bytes, dest=None) -> str:
        topic = _check_bin(topic)
        dest = self.node if dest is None else dest
        cur = self.routes.get(topic)
        if not cur or dest not in cur:
            return "ok"
        cur.remove(dest)
        if self._r_built and self.is_node(dest):
            self._r_touched[(self._ids[topic], self.node_id(dest))] = None
        if not cur:
            del self.routes[topic]
            fid = self._ids.pop(topic)
            del self._names[fid]
            self.m.apply(deletes=[topic])
            self._dirty = True
        return "ok"

    def commit(self):
        if self._dirty:
            self.m.commit()
            self._dirty = False
        if self.device_routes:
            self._commit_routes()

    def cleanup_routes(self, node) -> List[bytes]:
        """cleanup_routes/1 (emqx_router_helper.erl:137-146, 175-179) for the
        atom-dest pattern: every route to `node` goes; the filters left without
        a route leave the table and are returned.  With ``device_routes`` the
        device drops the node's bit in one pass (egm_routes_drop_node) and says
        which filters it emptied."""
        hit = [t for t, ds in self.routes.items() if node in ds]
        if self.device_routes:
            self.commit()   # (assigns the ids of the nodes routed to)
        if self.device_routes and node in self.node_ids:
            emptied = self.m.routes_drop_node(self.node_ids[node]).tolist()
            # (a filter that keeps only {Group, Node} routes has no node left, and stays in the table)
            want = sorted(self._ids[t] for t in hit if not any(self.is_node(d) and d != node for d in self.routes[t]))
            if emptied != want:
                raise RuntimeError("cleanup_routes: the device's emptied filters differ from the host's")
        gone = []
        for topic in hit:
            key = (self._ids[topic], self.node_ids.get(node))
            self.do_delete_route(topic, node)
            self._r_touched.pop(key, None)   # the device pass has done it
            if topic not in self.routes:
                gone.append(topic)
        return gone

    # -- lookups ----------------------------------------------------------------
    def lookup_routes(self, topic: bytes) -> List[Route]:
        return [Route(topic, d) for d in self.routes.get(topic, [])]

    def has_routes(self, topic: bytes) -> bool:
        return topic in self.routes

    def topics(self) -> List[bytes]:
        return list(self.routes)

    def match_filters_batch(self, topics: Sequence[bytes]):
        """GPU batch -> per topic the list of matched filter ids."""
        topics = [_check_bin(t) for t in topics]
        self.commit()
        res = self.m.match_strings(topics, L.EGM_MODE_ROUTES)
        return res

    def match_routes(self, topic: bytes) -> List[Route]:
        return self.match_routes_batch([_check_bin(topic)])[0]

    def match_routes_batch(self, topics: Sequence[bytes]) -> List[List[Route]]:
        res = self.match_filters_batch(topics)
        out = []
        for k in range(len(topics)):
            rs = []
            for fid in res.row(k).tolist():
                f = self._names[fid]
                rs.extend(Route(f, d) for d in self.routes[f])
            out.append(rs)
        return out

    def print_routes(self, topic: bytes) -> None:
        for r in self.match_routes(topic):
            print(f"{r.topic.decode(errors='replace')} -> {r.dest}")

    def filter_id(self, topic: bytes) -> Optional[int]:
        return self._ids.get(topic)

    def filter_of(self, fid: int) -> bytes:
        return self._names[fid]

    @staticmethod
    def is_wildcard(topic: bytes) -> bool:
        return wildcard(topic)
