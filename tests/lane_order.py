"""The partial order that a command list's event edges define, and replays of it in orders of the test's own choosing.

A recorded step (csrc/runtime.hip) is a few hundred commands on up to four lanes; the only ordering between lanes comes
from the event edges that net.py places by hand (lane_sync, lane_mark / lane_wait, the cross-replay slots).  If those
edges are sufficient, EVERY linearisation of the partial order they define computes the same bits as the eager step; if
one is missing, some legal linearisation runs a consumer in front of its producer.  This module rebuilds the partial
order from ``CmdList.describe()`` exactly as ``disyolo_cmdlist_run_ex`` enqueues it, produces linearisations by a list
scheduler, and (``execute``, the only part that needs a GPU) replays a recorded program one command at a time in such an
order with a device synchronise after every command -- so the host order IS the execution order, and nothing depends on
how long anything takes.

The model, per replay ``(descriptors, fork, join)`` of a sequence of replays on the same lanes:

  * every lane is FIFO over the whole sequence (the lanes are the same streams replay after replay);
  * kind 0 (launch): one node on ``lane``;
  * kind 1 (sync): a record node on ``from``, a wait node on ``to`` behind it;
  * kind 2 (mark): a record node on ``from``;  kind 3 (wait): a wait node on ``to`` behind the mark at list index
    ``from`` of the SAME replay;
  * kind 4 (mark_slot): a record node on ``from`` for slot ``to``;  kind 5 (wait_slot): a wait node on ``to`` behind the
    most recent kind-4 node of slot ``from`` in (replay, index) order -- the previous replay's where the wait comes
    first in the list, none at all before the slot was ever marked (``slot_recorded`` is false: nothing is enqueued);
  * fork: a wait node at the head of every side lane the list uses, behind everything lane 0 holds in front of the
    replay;  join: one node at the end of lane 0 behind the last node of every side lane the list uses (all replays so
    far: the lanes are FIFO).  A lane is "used" when a command of the list names it, as ``CmdList::uses`` has it;
  * an optional host node in front of a replay: work the caller's stream (lane 0) does between two replays, such as
    ``set_batch``; with ``joins`` it orders behind every lane (``sync_lanes`` and the stream-ordered copies behind it).

Scratch buffers: no rule was needed.  Wherever two lanes of the tested programs reuse a buffer, an event edge orders
the reuse (tests/test_gpu_lane_order.py holds every policy to the eager step's bits); a reuse ordered by nothing but
luck would show there as a difference and would be a bug of the step, not of this model.
"""
import collections
import itertools
import random as _random

LAUNCH, SYNC, MARK, WAIT, MARK_SLOT, WAIT_SLOT = range(6)
NLANES = 4

Replay = collections.namedtuple("Replay", "cmds fork join host host_joins")
Replay.__new__.__defaults__ = (True, True, None, False)
# what: "launch" | "record" | "wait" | "fork" | "join" | "host";  index: the command's index in its replay's list (None for
# fork / join / host);  seq: the node's position in the order the executor enqueues (its id: nodes[seq] is the node)
Node = collections.namedtuple("Node", "seq replay index what lane kind")


class OrderError(Exception):
    """the descriptors do not describe something the executor could run to completion"""


def lanes_used(cmds):
    used = {0}
    for kind, lane, src, dst in cmds:
        if kind == LAUNCH:
            used.add(lane)
        elif kind == SYNC:
            used.update((src, dst))
        elif kind in (MARK, MARK_SLOT):
            used.add(src)
        else:
            used.add(dst)
    return sorted(used)


class Graph:
    """nodes in enqueue order, ``lanes[l]`` = the node ids of lane l in FIFO order, ``deps[n]`` = the nodes
    (records, or lane 0's last node in front of a fork, ...) that n waits for; the FIFO edges are implied by ``lanes``"""

    def __init__(self, replays):
        self.replays = [r if isinstance(r, Replay) else Replay(*r) for r in replays]
        self.nodes, self.deps, self.lanes = [], [], collections.defaultdict(list)
        slot_mark = {}
        for r, rep in enumerate(self.replays):
            cmds = [tuple(int(v) for v in c) for c in rep.cmds]
            for i, (kind, lane, src, dst) in enumerate(cmds):
                bad = (kind not in range(6) or (kind == LAUNCH and not 0 <= lane < NLANES)
                       or (kind in (SYNC, MARK, MARK_SLOT) and not 0 <= src < NLANES)
                       or (kind in (SYNC, WAIT, WAIT_SLOT) and not 0 <= dst < NLANES) or (kind == SYNC and src == dst))
                if bad:
                    raise OrderError("replay %d command %d: bad descriptor %r" % (r, i, cmds[i]))
            used = lanes_used(cmds)
            if rep.host is not None:
                self._add(r, None, "host", 0, None, [ids[-1] for l, ids in sorted(self.lanes.items()) if l and ids]
                          if rep.host_joins else [])
            if rep.fork:
                before = self.lanes[0][-1:]
                for l in used[1:]:
                    self._add(r, None, "fork", l, None, before)
            mark_node, mark_waits = {}, []
            for i, (kind, lane, src, dst) in enumerate(cmds):
                if kind == LAUNCH:
                    self._add(r, i, "launch", lane, kind, [])
                elif kind == SYNC:
                    rec = self._add(r, i, "record", src, kind, [])
                    self._add(r, i, "wait", dst, kind, [rec])
                elif kind == MARK:
                    mark_node[i] = self._add(r, i, "record", src, kind, [])
                elif kind == WAIT:
                    if not (0 <= src < len(cmds) and cmds[src][0] == MARK):
                        raise OrderError("replay %d command %d waits for %d, which is not a mark of its list" % (r, i, src))
                    # (the recorder refuses a mark that comes later in the list; here the edge is kept as written, and the
                    #  scheduler raises where the wait sits in front of what would have to run first)
                    mark_waits.append((self._add(r, i, "wait", dst, kind, []), src))
                elif kind == MARK_SLOT:
                    slot_mark[dst] = self._add(r, i, "record", src, kind, [])
                else:
                    self._add(r, i, "wait", dst, kind, [slot_mark[src]] if src in slot_mark else [])
            for n, src in mark_waits:
                self.deps[n].append(mark_node[src])
            if rep.join:
                self._add(r, None, "join", 0, None, [self.lanes[l][-1] for l in used[1:] if self.lanes[l]])
        self.deps = [sorted(set(ds)) for ds in self.deps]
        self.lanes = {l: ids for l, ids in self.lanes.items() if ids}

    def _add(self, replay, index, what, lane, kind, deps):
        n = len(self.nodes)
        self.nodes.append(Node(n, replay, index, what, lane, kind))
        self.deps.append(list(deps))
        self.lanes[lane].append(n)
        return n

    def commands(self):
        """the nodes at which the executor issues a command: launches, waits, and the records of pure marks"""
        return [n.seq for n in self.nodes if issues_command(n)]


def issues_command(node):
    return node.what in ("launch", "wait") or (node.what == "record" and node.kind in (MARK, MARK_SLOT))


# ---- policies: which ready lane runs its head next -------------------------------------------------------------------
def recorded():
    return ("recorded",)


def priority(perm):
    return ("priority", tuple(perm))


def random(seed):
    return ("random", int(seed))


def policy_name(policy):
    return policy[0] if len(policy) == 1 else "%s(%s)" % (policy[0], policy[1])


def schedule(graph, policy):
    """a linearisation of ``graph``: again and again the ready head node of one lane, chosen by ``policy``"""
    heads = {l: 0 for l in graph.lanes}
    done = [False] * len(graph.nodes)
    order = []
    rng = _random.Random(policy[1]) if policy[0] == "random" else None
    if policy[0] == "priority":
        if sorted(policy[1]) != sorted(graph.lanes):
            raise ValueError("priority%r is no permutation of the lanes %r" % (policy[1], sorted(graph.lanes)))
    elif policy[0] not in ("recorded", "random"):
        raise ValueError("unknown policy %r" % (policy,))
    while len(order) < len(graph.nodes):
        ready = [l for l in sorted(graph.lanes) if heads[l] < len(graph.lanes[l])
                 and all(done[d] for d in graph.deps[graph.lanes[l][heads[l]]])]
        if not ready:
            stuck = [graph.nodes[graph.lanes[l][heads[l]]] for l in sorted(graph.lanes) if heads[l] < len(graph.lanes[l])]
            raise OrderError("no lane can go on: every head waits for something behind a waiting head: %r" % (stuck,))
        if policy[0] == "recorded":
            lane = min(ready, key=lambda l: graph.lanes[l][heads[l]])
        elif policy[0] == "priority":
            lane = min(ready, key=policy[1].index)
        else:
            lane = rng.choice(ready)
        n = graph.lanes[lane][heads[lane]]
        heads[lane] += 1
        done[n] = True
        order.append(n)
    return order


def is_legal(order, graph):
    """every node exactly once, every lane in FIFO order, every wait behind its source"""
    if sorted(order) != list(range(len(graph.nodes))):
        return False
    at = {n: p for p, n in enumerate(order)}
    for ids in graph.lanes.values():
        if any(at[a] > at[b] for a, b in zip(ids, ids[1:])):
            return False
    return all(at[d] < at[n] for n in range(len(graph.nodes)) for d in graph.deps[n])


def all_policies(graph, seeds=(0, 1, 2, 3)):
    lanes = sorted(graph.lanes)
    return [recorded()] + [priority(p) for p in itertools.permutations(lanes)] + [random(s) for s in seeds]


def linearisations(graph):
    """every legal order, by brute force (for small graphs: the count grows like a binomial coefficient)"""
    lanes = sorted(graph.lanes)
    heads = {l: 0 for l in lanes}
    done = [False] * len(graph.nodes)
    order = []

    def go():
        if len(order) == len(graph.nodes):
            yield list(order)
            return
        for l in lanes:
            if heads[l] == len(graph.lanes[l]):
                continue
            n = graph.lanes[l][heads[l]]
            if not all(done[d] for d in graph.deps[n]):
                continue
            heads[l] += 1
            done[n] = True
            order.append(n)
            yield from go()
            order.pop()
            done[n] = False
            heads[l] -= 1
    return go()


def hybrid(order, k, graph):
    """the first k nodes of ``order``, then every other node as recorded.  Legal whenever ``order`` is: a prefix of a legal
    order is closed under "comes before", and every edge points forward in the recorded order.  hybrid(0) is the recorded
    order and hybrid(len(order)) is ``order``, so a bisect over k finds a node whose run in that place changes a result."""
    head = list(order[:k])
    inhead = set(head)
    return head + [n for n in range(len(graph.nodes)) if n not in inhead]


def launch_inversions(order, graph):
    """pairs of launches that ``order`` runs the other way round than the recorded order (in which a node's id is its
    position).  A lane is FIFO in every legal order, so each such pair sits on two different lanes."""
    import bisect
    seen, inv = [], 0
    for n in order:
        if graph.nodes[n].what == "launch":
            at = bisect.bisect(seen, n)
            inv += len(seen) - at
            seen.insert(at, n)
    return inv


def cross_replay_inversions(order, graph):
    """pairs (launch of a later replay, launch of an earlier replay) that ``order`` runs in that order -- on two lanes, for
    the same reason: how far the next replay's head ran into the previous replay's tail"""
    seen, inv = collections.Counter(), 0
    for n in order:
        node = graph.nodes[n]
        if node.what == "launch":
            inv += sum(c for r, c in seen.items() if r > node.replay)
            seen[node.replay] += 1
    return inv


# ---- the executor (GPU): one command at a time, the device synchronised after each ----------------------------------
def execute(order, graph, progs, hosts=None):
    """Replay ``order``.  ``progs[r]`` is the CmdList of replay r (the pipelined step alternates two), ``hosts[r]`` the
    function of replay r's host node.  A launch is ``prog.run(i, i + 1)`` without fork or join; an event command is the same
    call, issued once: when its wait half is scheduled, or for a pure mark at its record node -- under the synchronise
    after every node the events order nothing, the schedule does.  Returns how often each (replay, index) was issued."""
    import torch
    issued = collections.Counter()
    for n in order:
        node = graph.nodes[n]
        if node.what == "host":
            hosts[node.replay]()
        elif issues_command(node):
            progs[node.replay].run(node.index, node.index + 1, fork=False, join=False)
            issued[(node.replay, node.index)] += 1
        torch.cuda.synchronize()
    torch.cuda.synchronize()
    return issued


# ---- disyolo_cmdlist_describe against a list recorded through the C ABI ------------------------------------------------
def describe_round_trip(all_kinds):
    """Record add_bf16 launches on lanes 0 and 1 and every kind of edge through the library (host buffers: nothing is
    run), and hold ``describe()`` to what was recorded and ``count()`` to the counts derived from it, for every `what`
    and lane.  An event edge owns a HIP event: a machine without a device cannot create one, the recorder answers
    DISYOLO_E_HIP and records nothing -- there only launches and slot waits are left (``all_kinds`` false); with a device
    all six kinds must be in the list."""
    import ctypes
    from disyolo_amd import lib as L
    lib = L.load()
    a, b = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
    add = lambda: lib.disyolo_add_bf16(ctypes.cast(a, ctypes.c_void_p), ctypes.cast(b, ctypes.c_void_p), 16, 0, None)
    want = []

    def rec(rc, d):
        if rc >= 0:
            want.append(d)
        else:
            assert not all_kinds and rc == -3 and d[0] in (SYNC, MARK, MARK_SLOT), (rc, d, lib.disyolo_last_error())
        return rc
    prog = L.CmdList()
    with prog:
        rec(add(), (LAUNCH, 0, 0, 0))
        L.set_lane(1)
        rec(add(), (LAUNCH, 1, 0, 0))
        rec(add(), (LAUNCH, 1, 0, 0))
        rec(lib.disyolo_cmdlist_sync(1, 0), (SYNC, 0, 1, 0))
        m = rec(lib.disyolo_cmdlist_mark(1), (MARK, 0, 1, 0))
        if m >= 0:
            assert m == len(want) - 1
            rec(lib.disyolo_cmdlist_wait(m, 2), (WAIT, 0, m, 2))
        rec(lib.disyolo_cmdlist_wait_slot(5, 0), (WAIT_SLOT, 0, 5, 0))
        rec(lib.disyolo_cmdlist_mark_slot(1, 5), (MARK_SLOT, 0, 1, 5))
        rec(lib.disyolo_cmdlist_wait_slot(5, 2), (WAIT_SLOT, 0, 5, 2))
        L.set_lane(0)
        rec(add(), (LAUNCH, 0, 0, 0))
    got = prog.describe()
    assert got == want and len(got) == prog.size()
    kinds = {d[0] for d in got}
    assert kinds == set(range(6)) if all_kinds else {LAUNCH, WAIT_SLOT} <= kinds
    assert {d[1] for d in got if d[0] == LAUNCH} == {0, 1}
    for lane in range(NLANES):
        derived = {"launches": sum(d[0] == LAUNCH and d[1] == lane for d in got),
                   "records": sum(d[0] in (SYNC, MARK, MARK_SLOT) and d[2] == lane for d in got),
                   "waits": sum(d[0] in (SYNC, WAIT, WAIT_SLOT) and d[3] == lane for d in got)}
        for what, n in derived.items():
            assert prog.count(what, lane) == n, (what, lane)
    g = Graph([Replay(got, True, True)])
    assert len(g.commands()) == len(got)
    out = (ctypes.c_int32 * 4)()
    for bad in (-1, len(got), 1 << 30):
        assert lib.disyolo_cmdlist_describe(prog.h, bad, out) == -1 and b"cmdlist_describe" in lib.disyolo_last_error()
    return got
