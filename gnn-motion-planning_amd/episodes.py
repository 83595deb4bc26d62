"""Device-side supervision of the explorer's training step (train_explorer.py:124-176) for a batch of problems.

One optimizer step is: sample graphs -> label (maze problems) -> shortest paths -> forward -> episodes -> loss -> backward,
with the stages in ``libgnnmp.so`` (csrc/train_episode_kernels.hip, C ABI ``gnnmp_episode_*``) and nothing read back to the
host after the graph build (whose edge count / per-problem edge offsets are the one read-back).

  maze_training_graphs     construct_graph (algorithm/dijkstra.py:15-31) for maze problems: kNN (k = 5, loop) + reversed,
                           coalesced, MazeEnv._edge_fp on the float64 samples, numpy's norm as the cost
  TrainingGraphs.from_reference   the reference's pickled (points, neighbors, edge_cost, edge_index, edge_free) datasets
  shortest_paths           dijkstra(nodes, neighbors, edge_cost, goal)   (dijkstra.py:49-76), prev[goal] = goal
  explore_steps            explore(edge_cost, policy, start, goal, 1000) (train_explorer.py:42-63)
  policy_frontier          policy_data(...)                              (train_explorer.py:66-93)
  frontier_loss            -policy[frontier].log_softmax(0)[next_edge_idx] (train_explorer.py:172), per problem
  draw_device / draw_host  the random choices of :129, :148, :165, :170
  forward_scores           the training forward, one pass per distinct loop value (forward_scores_batched: one pass in all)
  training_step            all of it for one batch: losses of the problems that were not skipped, ready for backward

Per-problem status: 0 ok, 1 skipped (only the goal is reachable, :133), 2 skipped (the frontier emptied inside explore,
:166-169), 3 bad input.  Edge sets must be the symmetric, coalesced sets construct_graph builds.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .batch import GraphBatch
from .graph_build import build_edges_gpu

STATUS_OK, STATUS_SINGLE, STATUS_EMPTY, STATUS_BAD = 0, 1, 2, 3


def _prefix(counts, device):
    p = torch.zeros(len(counts) + 1, dtype=torch.int64)
    p[1:] = torch.tensor(list(counts), dtype=torch.int64).cumsum(0)
    return p.to(torch.int32).to(device)


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


class TrainingGraphs:
    """B labelled problems on one device: v [sumN, C] fp32, edge_index [2, sumE] int64 (graph-local, coalesced),
    node_ptr / edge_ptr int32 [B + 1] (with host copies), edge_free uint8 / edge_cost float64 [sumE], the obstacles of the
    training forward (obstacles [sumO, S], obs_ptr) -- what ``GraphBatch`` and the episode kernels read."""

    def __init__(self, v, edge_index, node_ptr_host, edge_ptr_host, edge_free, edge_cost, obstacles, obs_ptr_host,
                 points64=None, device_ptrs=None):
        """``device_ptrs``: ``(node_ptr, edge_ptr, obs_ptr)`` as int32 device tensors that already hold (or, in stream order,
        will hold) the values of the three host sequences; without it the host sequences are uploaded."""
        dev = v.device
        if dev.type != 'cuda':
            raise RuntimeError('gnnmp.episodes runs on the GPU only (got %s tensors); there is no CPU fallback' % dev)
        self.v, self.edge_index = v.contiguous(), edge_index.contiguous()
        self.node_ptr_host, self.edge_ptr_host, self.obs_ptr_host = list(node_ptr_host), list(edge_ptr_host), list(obs_ptr_host)
        if device_ptrs is None:
            self.node_ptr = torch.tensor(self.node_ptr_host, dtype=torch.int32).to(dev)
            self.edge_ptr = torch.tensor(self.edge_ptr_host, dtype=torch.int32).to(dev)
            self.obs_ptr = torch.tensor(self.obs_ptr_host, dtype=torch.int32).to(dev)
        else:
            self.node_ptr, self.edge_ptr, self.obs_ptr = device_ptrs
        self.edge_free, self.edge_cost = edge_free.contiguous(), edge_cost.contiguous()
        self.obstacles = obstacles.contiguous()
        self.points64 = points64
        self.n_problems = len(self.node_ptr_host) - 1
        self.total_nodes, self.total_edges = self.node_ptr_host[-1], self.edge_ptr_host[-1]
        self._ws = None

    @property
    def device(self):
        return self.v.device

    def sizes(self):
        return [self.node_ptr_host[i + 1] - self.node_ptr_host[i] for i in range(self.n_problems)]

    def c_graphs(self):
        return _lib.EpisodeGraphs(self.n_problems, self.total_nodes, self.total_edges, self.node_ptr.data_ptr(),
                                  self.edge_ptr.data_ptr(), self.edge_index.data_ptr())

    def workspace(self):
        if self._ws is None:
            need = ctypes.c_size_t()
            cg = self.c_graphs()
            _lib.check(_lib.lib().gnnmp_episode_workspace_bytes(ctypes.byref(cg), ctypes.byref(need)), 'episode workspace')
            self._ws = torch.empty(max(need.value, 256), dtype=torch.uint8, device=self.device)
        return self._ws

    def problem_of_node(self):
        counts = self.node_ptr[1:].long() - self.node_ptr[:-1].long()
        return torch.repeat_interleave(torch.arange(self.n_problems, device=self.device), counts, output_size=self.total_nodes)

    def batch(self, goal_index, lo=0, hi=None):
        """A :class:`GraphBatch` of problems [lo, hi) with goal = v[goal_index] (device gather, no read-back)."""
        hi = self.n_problems if hi is None else hi
        n0, n1 = self.node_ptr_host[lo], self.node_ptr_host[hi]
        e0, e1 = self.edge_ptr_host[lo], self.edge_ptr_host[hi]
        o0, o1 = self.obs_ptr_host[lo], self.obs_ptr_host[hi]
        goal = self.v[self.node_ptr[lo:hi].long() + goal_index[lo:hi].long()]
        obs_counts = [self.obs_ptr_host[i + 1] - self.obs_ptr_host[i] for i in range(lo, hi)]
        return GraphBatch(self.v[n0:n1], goal, self.obstacles[o0:o1], self.edge_index[:, e0:e1],
                          (self.node_ptr[lo:hi + 1] - n0).contiguous(), (self.edge_ptr[lo:hi + 1] - e0).contiguous(),
                          (self.obs_ptr[lo:hi + 1] - o0).contiguous(), max(obs_counts + [0]),
                          dense_floats=sum((self.node_ptr_host[i + 1] - self.node_ptr_host[i]) ** 2 for i in range(lo, hi)))

    def subset(self, problems, goal_index):
        """A :class:`GraphBatch` of the listed problems (any order, host ints) with goal = v[goal_index], and the positions
        [sum of their E] of its edges in this batch's edge list.  The gathers use host-known offsets: no read-back."""
        rng = lambda ptr: np.concatenate([np.arange(ptr[i], ptr[i + 1]) for i in problems] + [np.zeros(0, np.int64)])  # noqa: E731
        dev = self.device
        nodes, edges, obs = (torch.from_numpy(rng(p).astype(np.int64)).to(dev)
                             for p in (self.node_ptr_host, self.edge_ptr_host, self.obs_ptr_host))
        size = lambda ptr, i: ptr[i + 1] - ptr[i]                                                                  # noqa: E731
        probs = torch.tensor(list(problems), dtype=torch.int64).to(dev)
        goal = self.v[self.node_ptr.long()[probs] + goal_index.long()[probs]]
        obs_counts = [size(self.obs_ptr_host, i) for i in problems]
        b = GraphBatch(self.v[nodes], goal, self.obstacles[obs], self.edge_index[:, edges],
                       _prefix([size(self.node_ptr_host, i) for i in problems], dev),
                       _prefix([size(self.edge_ptr_host, i) for i in problems], dev), _prefix(obs_counts, dev),
                       max(obs_counts + [0]), dense_floats=sum(size(self.node_ptr_host, i) ** 2 for i in problems))
        return b, edges

    @staticmethod
    def from_reference(items, obstacles, device):
        """``items``: the reference's dataset entries (points, neighbors, edge_cost, edge_index, edge_free)
        (dijkstra.py:139-141): edge_index [E, 2] (source, target) coalesced, edge_cost[t] / neighbors[t] per target in edge
        order, edge_free per edge.  ``obstacles``: per problem the [O, S] obstacle rows the forward attends over."""
        vs, eis, frees, costs, obs = [], [], [], [], []
        for (points, _neighbors, edge_cost, edge_index, edge_free), ob in zip(items, obstacles):
            ei = np.asarray(edge_index, dtype=np.int64).reshape(-1, 2).T
            cursor, cost = {}, np.empty(ei.shape[1])
            for e in range(ei.shape[1]):
                t = int(ei[1, e])
                k = cursor.get(t, 0)
                cost[e] = edge_cost[t][k]
                cursor[t] = k + 1
            vs.append(torch.tensor(np.asarray(points), dtype=torch.float32))
            eis.append(torch.from_numpy(ei))
            frees.append(torch.tensor(np.asarray(edge_free, dtype=np.uint8).reshape(-1)))
            costs.append(torch.from_numpy(cost))
            obs.append(torch.tensor(np.asarray(ob), dtype=torch.float32).reshape(len(ob), -1))
        S = obs[0].shape[1] if obs else 2
        return TrainingGraphs(torch.cat(vs).to(device), torch.cat(eis, dim=1).to(device),
                              _prefix([x.shape[0] for x in vs], 'cpu').tolist(), _prefix([x.shape[1] for x in eis], 'cpu').tolist(),
                              torch.cat(frees).to(device), torch.cat(costs).to(device),
                              torch.cat(obs).reshape(-1, S).to(device), _prefix([x.shape[0] for x in obs], 'cpu').tolist())


def maze_obstacles(maze_map):
    """MazeEnv.obstacles (maze_env.py:75-80): cell (i, j) of every obstacle / w - 0.5, float32 as obs_data hands it on."""
    m = np.asarray(maze_map)
    idx = np.array([(i, j) for i in range(m.shape[0]) for j in range(m.shape[1]) if m[i, j] == 1]).reshape(-1, 2)
    return np.asarray(idx / m.shape[0] - 0.5, dtype=np.float32)


def maze_training_graphs(points64, node_ptr, maps, dim):
    """construct_graph for B maze problems on the device.  ``points64``: float64 [sumN, dim] samples (cuda); ``node_ptr``:
    host sequence [B + 1]; ``maps``: [B, w, w] occupancy (host or device, 1 = obstacle).  The kNN runs on the float32 rows
    (FloatTensor(points)), the collision checks on the float64 ones."""
    dev = points64.device
    if dev.type != 'cuda':
        raise RuntimeError('maze_training_graphs needs device tensors')
    if dim not in (2, 3) or points64.shape[1] != dim:
        raise ValueError('maze problems are 2-D (point robot) or 3-D (stick robot), got dim %d / points %s'
                         % (dim, tuple(points64.shape)))
    nptr = [int(x) for x in node_ptr]
    B = len(nptr) - 1
    p64 = points64.to(torch.float64).contiguous()
    v = p64.float().contiguous()
    nptr_d = torch.tensor(nptr, dtype=torch.int32).to(dev)
    sizes = nptr_d[1:] - nptr_d[:-1]
    ei, eptr = build_edges_gpu(v, nptr_d, sizes, torch.full((B,), 5, dtype=torch.int32, device=dev))
    eptr_h = eptr.cpu().tolist()                          # the stream is idle here: build_edges_gpu read the edge count back
    maps_h = maps.cpu().numpy() if torch.is_tensor(maps) else np.asarray(maps)
    maps_d = torch.as_tensor(maps_h, dtype=torch.float64).to(dev).contiguous()
    E = int(ei.shape[1])
    free = torch.empty(E, dtype=torch.uint8, device=dev)
    cost = torch.empty(E, dtype=torch.float64, device=dev)
    obs = [maze_obstacles(m) for m in maps_h]
    g = TrainingGraphs(v, ei, nptr, eptr_h, free, cost,
                       torch.from_numpy(np.concatenate(obs).reshape(-1, 2)).to(dev), _prefix([len(o) for o in obs], 'cpu').tolist(),
                       points64=p64)
    label_maze(g, p64, maps_d, dim)
    return g


def label_maze(graphs, points64, maps, dim):
    """Fill graphs.edge_free / edge_cost with construct_graph's labels of its (given) edges: MazeEnv._edge_fp on the float64
    rows ``points64`` [sumN, dim] (device), ``maps`` [B, w, w] float64 (device)."""
    dev = graphs.device
    p64 = points64.to(torch.float64).contiguous()
    maps_d = maps.to(device=dev, dtype=torch.float64).contiguous()
    cg = graphs.c_graphs()
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().gnnmp_episode_label_maze(ctypes.byref(cg), int(dim), int(maps_d.shape[1]), p64.data_ptr(),
                                                       maps_d.data_ptr(), graphs.edge_free.data_ptr(), graphs.edge_cost.data_ptr(),
                                                       _stream(dev)), 'gnnmp_episode_label_maze')
    graphs._keep = (p64, maps_d)                           # alive until the stream has used them
    return graphs


def _i32(x, dev):
    return torch.as_tensor(x).to(device=dev, dtype=torch.int32).contiguous()


def shortest_paths(graphs, goal_index):
    """dist [sumN] float64 (+inf unreachable), prev [sumN] int32 (-1 unreachable, prev[goal] = goal), n_valid [B]."""
    dev = graphs.device
    goal = _i32(goal_index, dev)
    dist = torch.empty(graphs.total_nodes, dtype=torch.float64, device=dev)
    prev = torch.empty(graphs.total_nodes, dtype=torch.int32, device=dev)
    n_valid = torch.empty(graphs.n_problems, dtype=torch.int32, device=dev)
    ws = graphs.workspace()
    cg = graphs.c_graphs()
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().gnnmp_episode_paths(ctypes.byref(cg), graphs.edge_cost.data_ptr(), goal.data_ptr(), dist.data_ptr(),
                                                  prev.data_ptr(), n_valid.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)),
                   'gnnmp_episode_paths')
    return {'goal': goal, 'dist': dist, 'prev': prev, 'n_valid': n_valid}


def explore_steps(graphs, scores, start, goal, n_valid, max_steps=1000):
    """(step [B], status [B]) of explore() on the detached scores [sumE]."""
    dev = graphs.device
    sc = scores.detach().float().contiguous()
    st, go, nv = _i32(start, dev), _i32(goal, dev), _i32(n_valid, dev)
    step = torch.empty(graphs.n_problems, dtype=torch.int32, device=dev)
    status = torch.empty(graphs.n_problems, dtype=torch.int32, device=dev)
    ws = graphs.workspace()
    cg = graphs.c_graphs()
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().gnnmp_episode_explore(ctypes.byref(cg), sc.data_ptr(), graphs.edge_free.data_ptr(), go.data_ptr(),
                                                    st.data_ptr(), nv.data_ptr(), int(max_steps), step.data_ptr(),
                                                    status.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)),
                   'gnnmp_episode_explore')
    return step, status


def policy_frontier(graphs, scores, paths, start, goal, step, status):
    """policy_data() after exactly step[b] steps: frontier (edge ids, problem b from 2 edge_ptr[b] + b), frontier_len,
    label (position of next_edge in the frontier), next to status."""
    dev = graphs.device
    sc = scores.detach().float().contiguous()
    st, go, sp, ss = _i32(start, dev), _i32(goal, dev), _i32(step, dev), _i32(status, dev)
    frontier = torch.empty(2 * graphs.total_edges + graphs.n_problems, dtype=torch.int32, device=dev)
    flen = torch.empty(graphs.n_problems, dtype=torch.int32, device=dev)
    label = torch.empty(graphs.n_problems, dtype=torch.int32, device=dev)
    ws = graphs.workspace()
    cg = graphs.c_graphs()
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().gnnmp_episode_frontier(ctypes.byref(cg), sc.data_ptr(), graphs.edge_free.data_ptr(), go.data_ptr(),
                                                     st.data_ptr(), _i32(paths['n_valid'], dev).data_ptr(), paths['dist'].data_ptr(),
                                                     paths['prev'].data_ptr(), sp.data_ptr(), ss.data_ptr(), frontier.data_ptr(),
                                                     flen.data_ptr(), label.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)),
                   'gnnmp_episode_frontier')
    return {'frontier': frontier, 'frontier_len': flen, 'label': label, 'status': ss, 'edge_ptr': graphs.edge_ptr,
            'total_edges': graphs.total_edges}


def frontier_slices(fr, b):
    """Host view of problem b's frontier edge ids and label (reads back; for tests and inspection)."""
    e0 = int(fr['edge_ptr'][b])
    n = int(fr['frontier_len'][b])
    off = 2 * e0 + b
    return fr['frontier'][off:off + n].cpu().numpy(), int(fr['label'][b])


def frontier_loss(scores, fr):
    """Per-problem policy loss -(s[label] - logsumexp(s[frontier])) [B] (0 for skipped problems) and the mask of the
    problems that count.  ``scores``: the per-edge scores of ``train_scores`` (autograd flows back through them)."""
    dev = scores.device
    B = int(fr['frontier_len'].numel())
    eptr = fr['edge_ptr'].long()
    cap = 2 * (eptr[1:] - eptr[:-1]) + 1
    base = 2 * eptr[:-1] + torch.arange(B, device=dev)
    n_slots = 2 * int(fr['total_edges']) + B
    prob = torch.repeat_interleave(torch.arange(B, device=dev), cap, output_size=n_slots)
    pos = torch.arange(n_slots, device=dev) - base[prob]
    ok = (fr['status'] == 0) & (fr['frontier_len'] > 0) & (fr['label'] >= 0)
    valid = (pos < fr['frontier_len'].long()[prob]) & ok[prob]
    # per edge: how often it sits in its problem's frontier (0, 1, or 2 for the start's duplicated row); integer adds are
    # exact in any order, and invalid slots add 0 to edges spread over the batch
    E = int(fr['total_edges'])
    spread = torch.arange(n_slots, device=dev) % max(E, 1)
    count = torch.zeros(max(E, 1), dtype=torch.int32, device=dev).index_add_(
        0, torch.where(valid, fr['frontier'].long(), spread), valid.to(torch.int32))[:E]
    eprob = torch.repeat_interleave(torch.arange(B, device=dev), eptr[1:] - eptr[:-1], output_size=E)
    inf_ = torch.full((), float('-inf'), device=dev, dtype=scores.dtype)
    m = torch.full((B,), float('-inf'), device=dev, dtype=scores.dtype).scatter_reduce(
        0, eprob, torch.where(count > 0, scores.detach(), inf_), 'amax', include_self=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    # edges outside the frontier take the maximum BEFORE the exp: no inf (and no 0 * inf in the backward) can arise
    sv = torch.where(count > 0, scores, m[eprob])
    t = torch.where(count > 0, count.to(scores.dtype) * torch.exp(sv - m[eprob]), torch.zeros_like(scores))
    # per-problem sums as differences of one float64 prefix sum: a fixed order (scan), exact to far below float32
    cs = torch.cat((torch.zeros(1, dtype=torch.float64, device=dev), torch.cumsum(t.double(), 0)))
    sumexp = cs[eptr[1:]] - cs[eptr[:-1]]
    lab = fr['frontier'].long()[(base + fr['label'].long().clamp(min=0)).clamp(max=n_slots - 1)]
    s_lab = scores[torch.where(ok, lab, torch.zeros_like(lab))]
    # log_softmax's own order: -((s[label] - max) - log(sum exp(s - max))), no cancellation against the maximum
    loss = torch.log(torch.where(ok, sumexp, torch.ones_like(sumexp))).to(scores.dtype) - (s_lab - m)
    return torch.where(ok, loss, torch.zeros_like(loss)), ok


# ---------------------------------------------------------------------------------------------------------------- draws
def draw_device(graphs, loop, generator=None, cpu_generator=None):
    """Goals (uniform node id) and loops (randint(1, loop), :148, one independent draw per problem) without synchronisation;
    ``generator``: a torch.Generator on the graphs' device, ``cpu_generator``: the host one the loops come from (their values
    decide the forward launches, :func:`forward_scores`)."""
    dev = graphs.device
    sizes = (graphs.node_ptr[1:] - graphs.node_ptr[:-1]).double()
    u = torch.rand(graphs.n_problems, dtype=torch.float64, device=dev, generator=generator)
    goal = torch.minimum((u * sizes).floor(), sizes - 1).to(torch.int32)
    loops = torch.randint(1, max(int(loop), 2), (graphs.n_problems,), generator=cpu_generator).tolist()
    return goal, loops


def forward_scores(model, graphs, goal, loops):
    """The training forward of every problem at its own loop count: one ``model.train_scores`` per distinct loop value over
    the problems that drew it, the per-edge scores put back into the batch's edge order [sumE] (autograd flows through)."""
    groups = {}
    for b, lp in enumerate(loops):
        groups.setdefault(int(lp), []).append(b)
    parts, pos = [], []
    for lp in sorted(groups):
        bt, edges = graphs.subset(groups[lp], goal)
        parts.append(model.train_scores(bt, lp))
        pos.append(edges)
    if len(parts) == 1 and groups[next(iter(groups))] == list(range(graphs.n_problems)):
        return parts[0]
    inv = torch.empty(graphs.total_edges, dtype=torch.int64, device=graphs.device)
    allpos = torch.cat(pos)
    inv[allpos] = torch.arange(allpos.numel(), device=graphs.device)
    return torch.cat(parts)[inv]


def forward_scores_batched(model, graphs, goal, loops):
    """:func:`forward_scores` as ONE ``model.train_scores_batch`` over all problems, each at its own loop count: one forward
    and one backward per optimizer step, their launch count set by ``max(loops)`` alone (:func:`forward_scores` makes one
    pass per distinct loop value).  Scores [sumE] in the batch's edge order; the sizes come from the host copies of the prefix
    arrays, nothing is read back.

    Both are fp32 evaluations of the same function and differ in the last bits: the launchers size their work by the row count
    of the call -- the weight gradients stage their partial sums by it -- so the two sum in different orders.  A near-tie
    between two edge scores inside an episode may therefore resolve differently."""
    size = lambda ptr: [ptr[i + 1] - ptr[i] for i in range(graphs.n_problems)]          # noqa: E731
    return model.train_scores_batch(graphs.batch(goal), loops, size(graphs.node_ptr_host), size(graphs.edge_ptr_host))


def draw_start(graphs, paths, generator=None):
    """start = the floor(u * n_valid)-th valid node in id order (the goal itself when n_valid <= 1)."""
    dev = graphs.device
    prob = graphs.problem_of_node()
    valid = torch.isfinite(paths['dist'])
    local = torch.arange(graphs.total_nodes, device=dev) - graphs.node_ptr.long()[prob]
    rank = torch.cumsum(valid.long(), 0)
    before = torch.cat((torch.zeros(1, dtype=torch.long, device=dev), rank))[graphs.node_ptr.long()[:-1]]
    rank = rank - before[prob]                             # 1-based rank of a valid node inside its problem
    nv = paths['n_valid'].double().clamp(min=0)
    u = torch.rand(graphs.n_problems, dtype=torch.float64, device=dev, generator=generator)
    k = torch.minimum((u * nv).floor(), (nv - 1).clamp(min=0)).long()
    hit = valid & (rank == k[prob] + 1)
    start = torch.full((graphs.n_problems,), -1, dtype=torch.long, device=dev).scatter_reduce(
        0, prob, torch.where(hit, local, torch.full_like(local, -1)), 'amax', include_self=True)
    return torch.where(paths['n_valid'] > 1, start, paths['goal'].long()).to(torch.int32)


def draw_step(step, generator=None):
    """s = floor(u * (step + 1)) in [0, step] (np.random.randint(0, step + 1), :170); -1 stays -1."""
    u = torch.rand(step.numel(), dtype=torch.float64, device=step.device, generator=generator)
    s = torch.minimum((u * (step.double() + 1)).floor(), step.double()).to(torch.int32)
    return torch.where(step >= 0, s, step)


def draw_host(sizes, valid_of, step_of, loop, rng=np.random):
    """The reference's draws in its own order, problem after problem (:129, :148, :165, :170), from numpy's global generator
    (or ``rng``).  ``valid_of(b, goal)``: problem b's valid-node mask for that goal (e.g. ``isfinite`` of
    :func:`shortest_paths`' dist); ``step_of(b, goal, loop, start)``: the explore step, None when the frontier emptied.  Each
    draw depends on the previous problem's outcome, so this synchronises once per problem.  Returns per problem
    (goal, loop, start, replay step), None for the draws the reference never makes."""
    out = []
    for b, size in enumerate(sizes):
        goal = int(rng.choice(size))
        valid = np.asarray(valid_of(b, goal), dtype=bool)
        if int(valid.sum()) == 1:
            out.append((goal, None, None, None))
            continue
        lp = int(rng.randint(1, loop))
        start = int(rng.choice(np.arange(len(valid))[valid]))
        step = step_of(b, goal, lp, start)
        out.append((goal, lp, start, None if step is None else int(rng.randint(0, step + 1))))
    return out


# ---------------------------------------------------------------------------------------------------------------- driver
def training_step(model, graphs, loop=10, max_steps=1000, generator=None, cpu_generator=None, batched=False):
    """Supervision + loss of one batch in device mode: draws, shortest paths, the training forward (one ``train_scores`` per
    loop value; ``batched=True``: one ``train_scores_batch`` for all of them, :func:`forward_scores_batched`), explore,
    replay, frontier loss.  Returns (loss = sum of the per-problem losses, info dict).  ``loss`` is ready for ``backward()``;
    nothing is read back to the host.  The two forwards agree to fp32 rounding, not bit for bit (different summation orders
    in the dense layers), so a near-tie inside an episode may resolve differently between them."""
    goal, loops = draw_device(graphs, loop, generator, cpu_generator)
    paths = shortest_paths(graphs, goal)
    start = draw_start(graphs, paths, generator)
    scores = (forward_scores_batched if batched else forward_scores)(model, graphs, paths['goal'], loops)
    step, status = explore_steps(graphs, scores, start, paths['goal'], paths['n_valid'], max_steps)
    s = draw_step(step, generator)
    fr = policy_frontier(graphs, scores, paths, start, paths['goal'], s, status)
    losses, ok = frontier_loss(scores, fr)
    return losses.sum(), {'goal': paths['goal'], 'start': start, 'loops': loops, 'paths': paths, 'step': step,
                          'replay_step': s, 'status': status, 'frontier': fr, 'losses': losses, 'counted': ok,
                          'scores': scores}
