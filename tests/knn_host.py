"""Host reference for the nearest-neighbour kernels with the tie rule written out: on equal distance the LOWER INDEX wins
(csrc/graph_kernels.hip gb_knn, csrc/smoother_kernels.hip sm_knn, csrc/explorer_kernels.hip goal arg-min).

The oracle's kNN (oracle/ref_cpu.knn, gnnmp.graph_build.knn_indices) is ``cdist(...).topk(...)``, whose order among equal
distances is unspecified, so it cannot check a tied input.  Here the distances are the kernels' own numbers and the order
is a stable sort: squared distances accumulated coordinate by coordinate (``d = d + df * df``), in float64 from the float32
coordinates for the graph builder (``df`` of two float32 values of similar magnitude and its square are exact in float64,
so the sum equals the kernel's fma chain), in float32 for the explorer's goal node.

``lattice`` makes the tied inputs: points of a dyadic lattice (step a power of two, a few bits per coordinate), so that
every squared distance is exact in float32 and float64 and equal distances are equal bit for bit, plus duplicated rows.
"""
import numpy as np
import torch

from gnnmp import graph_build


def sqdist64(y, x):
    """[len(y), len(x)] float64 squared distances from the rows of ``y`` to the rows of ``x`` (float32 tensors or arrays)."""
    y = np.asarray(y, dtype=np.float32).astype(np.float64)
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    d = np.zeros((y.shape[0], x.shape[0]))
    for c in range(x.shape[1]):
        df = y[:, c].reshape(-1, 1) - x[:, c].reshape(1, -1)
        d = d + df * df
    return d


def knn_stable(x, k):
    """int64 array [n, min(k, n)]: for every row of ``x`` the k nearest rows (itself included) in ascending
    (squared distance, index) order."""
    k = min(int(k), x.shape[0])
    return np.argsort(sqdist64(x, x), axis=1, kind='stable')[:, :k]


def _knn_edges(x, k):
    """knn_graph(x, k, loop=True): [2, n * k], row 0 = neighbour (source), row 1 = centre (target)."""
    nb = knn_stable(x, k)
    centre = np.broadcast_to(np.arange(x.shape[0]).reshape(-1, 1), nb.shape)
    return torch.from_numpy(np.stack((nb.reshape(-1), centre.reshape(-1)))).long()


def build_edges_stable(v, n_free, k1):
    """``create_data``'s edge set (kNN(all) + reversed + kNN(free only) + reversed, coalesced) on top of knn_stable.
    The free set is the first min(n_free, N) rows; an empty graph has no edges."""
    n = v.shape[0]
    if n == 0:
        return torch.zeros((2, 0), dtype=torch.int64)
    e = _knn_edges(v, k1)
    ef = _knn_edges(v[:min(int(n_free), n)], k1)
    return graph_build.coalesce(torch.cat((e, e.flip(0), ef, ef.flip(0)), dim=1), n)


def bucket_sizes(v, n_free, k1):
    """int64 array [N]: columns per source BEFORE coalescing (what gb_count counts and gb_unique sorts): a centre c with
    neighbour a adds one to a (a -> c) and one to c (c -> a), in the pass over all nodes and in the pass over the free ones."""
    n = v.shape[0]
    cnt = np.zeros(n, dtype=np.int64)
    for x in (v, v[:min(int(n_free), n)]):
        if x.shape[0] == 0:
            continue
        nb = knn_stable(x, k1)
        cnt[:x.shape[0]] += nb.shape[1]                                        # the centre's own side of every pair
        cnt += np.bincount(nb.reshape(-1), minlength=n)
    return cnt


def argmin_stable32(v, goal):
    """Lowest index at the minimum of the float32 squared distance from ``goal`` to the rows of ``v``."""
    v = np.asarray(v, dtype=np.float32)
    g = np.asarray(goal, dtype=np.float32).reshape(-1)
    d = np.zeros(v.shape[0], dtype=np.float32)
    for c in range(v.shape[1]):
        df = v[:, c] - g[c]
        d = d + df * df
    return int(np.flatnonzero(d == d.min())[0])


def lattice(n, C, step, seed, duplicates, side=None):
    """float32 tensor [n, C]: rows drawn from the dyadic lattice {(j - side // 2) * step}^C in a shuffled order, then
    ``duplicates`` rows overwritten by copies of earlier rows.  ``side`` defaults to the smallest lattice that holds n
    distinct points; a smaller one is drawn with replacement (a dense input: many rows per lattice point)."""
    assert step > 0 and np.log2(step) == np.round(np.log2(step)), 'the step must be a power of two'
    rng = np.random.RandomState(seed)
    if side is None:
        side = 2
        while side ** C < n:
            side += 1
    assert side <= 64, 'more than 6 bits per coordinate'
    cells = side ** C
    flat = rng.permutation(cells)[:n] if cells >= n else rng.randint(0, cells, size=n)
    x = np.stack([(flat // side ** c) % side for c in range(C)], axis=1) - side // 2
    x = (x * step).astype(np.float32)
    for _ in range(duplicates):
        dst = rng.randint(1, n)
        x[dst] = x[rng.randint(0, dst)]
    return torch.from_numpy(x)


def has_tie_at_kth(x, k):
    """True where a row's k-th and (k+1)-th nearest are at the same distance: the tie rule decides that row's neighbours."""
    d = np.sort(sqdist64(x, x), axis=1)
    k = int(k)
    if k >= x.shape[0]:
        return np.zeros(x.shape[0], dtype=bool)
    return d[:, k - 1] == d[:, k]


def tied(n, C, seed):
    """The tied input of the graph-builder tests: distinct lattice points at step 1/8 with two duplicated rows."""
    return lattice(n, C, 0.125, seed, min(2, max(n - 1, 0)))


# ---------------------------------------------------------------------------------------------------------------------
# smoother problems (tests/test_smoother_parity.py and the child process it starts build the same inputs from here)
# ---------------------------------------------------------------------------------------------------------------------
SMOOTHER_SAMPLE_COUNTS = (9, 63, 64, 65, 1024, 1025, 2047, 2048)


def smoother_lattice_problem(ns, P=9, seed=0):
    """(path [P, 2], free, collided, edge_index) with ``ns`` samples in all: distinct points of the 64 x 64 lattice with step
    1/32 (the smallest square block of it that holds them), shuffled across free and collided; waypoints alternately on
    lattice points and on cell centres of the block.  Around a lattice point the samples come in shells of 1, 4, 4, 4, 8 ...
    equidistant ones, around a cell centre of 4, 8, ..., so the tenth neighbour lies inside a shell and the tie rule picks."""
    from gnnmp.planner import chain_edge_index
    rng = np.random.RandomState(seed + ns)
    side = max(3, int(np.ceil(np.sqrt(ns))))
    assert side <= 64 and (side - 1) ** 2 >= P // 2
    cells = rng.permutation(side * side)[:ns]
    samples = (np.stack((cells % side, cells // side), axis=1) - side // 2) / 32.0
    lat = rng.permutation(side * side)[:(P + 1) // 2]
    cen = rng.permutation((side - 1) ** 2)[:P // 2]
    path = np.zeros((P, 2))
    path[0::2] = np.stack((lat % side, lat // side), axis=1) - side // 2
    path[1::2] = np.stack((cen % (side - 1), cen // (side - 1)), axis=1) - side // 2 + 0.5
    path = path / 32.0
    F = ns // 2 + 1
    t = lambda a: torch.from_numpy(a.astype(np.float32))                   # noqa: E731
    return t(path), t(samples[:F]), t(samples[F:]), chain_edge_index(P)


def smoother_random_problem(ns, P=12, seed=0):
    """The same sample counts with continuous random coordinates (no ties)."""
    from gnnmp.planner import chain_edge_index
    gen = torch.Generator().manual_seed(7000 + seed + ns)
    F = ns // 2 + 1
    path, free, coll = (torch.rand(n, 2, generator=gen) * 2 - 1 for n in (P, F, ns - F))
    return path, free, coll, chain_edge_index(P)
