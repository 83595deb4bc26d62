#!/usr/bin/env python
"""The ranking launch of the ranked frontier (gnnmp_frontier_rank) by HIP events, next to the policy stage of the forward that
produces its scores, at two shapes: one 1002-node k = 30 graph (k1 = 41, the default planner's forward) and 256 graphs of 1000
nodes at k1 = 8.  Prints one JSON line per shape; profiles/frontier_rank_bench.txt keeps the numbers."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402
import gnnmp  # noqa: E402
from gnnmp.frontier import RankedRows, rank_rows  # noqa: E402
from gnnmp.synth import synth_batch_gpu  # noqa: E402
from gnnmp.weights import load_weights  # noqa: E402


def main():
    dev = torch.device('cuda:0')
    m = gnnmp.EncoderProcessDecoder(2, 2, 32, 2).eval()
    m.load_state_dict(load_weights('weights_maze'))
    for n_graphs, n_nodes, k1 in ((1, 1002, 41), (256, 1000, 8)):
        graphs = synth_batch_gpu('maze2', n_nodes, k1, n_graphs, dev)
        gb = gnnmp.GraphBatch.from_graphs(graphs, 2, dev)
        nf = torch.tensor([int(g['n_free']) for g in graphs], dtype=torch.int32, device=dev)
        scores = m.forward_batch(gb, 5)
        holder = RankedRows()
        args = (scores, gb.edge_index, nf, gb.node_ptr, gb.edge_ptr)
        for _ in range(3):
            rank_rows(*args, n_nodes=gb.total_nodes, out=holder)
        torch.cuda.synchronize()
        reps, times = 20, []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            rank_rows(*args, n_nodes=gb.total_nodes, out=holder)
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b))
        m.profile(dev, True)
        m.profile_read(dev)
        for _ in range(reps):
            m.forward_batch(gb, 5)
        prof = m.profile_read(dev)
        m.profile(dev, False)
        times.sort()
        print(json.dumps({'graphs': n_graphs, 'nodes_per_graph': n_nodes, 'k1': k1, 'edges': gb.total_edges,
                          'rank_ms_median': round(times[reps // 2], 4), 'rank_ms_min': round(times[0], 4),
                          'policy_ms_mean': round(prof['policy'][0] / max(prof['policy'][1], 1), 4),
                          'forward_ms_mean': round(sum(v[0] for v in prof.values()) / reps, 4),
                          'note': 'rank = memset + 3 launches between two events on the stream, host enqueue included'}))


if __name__ == '__main__':
    main()
