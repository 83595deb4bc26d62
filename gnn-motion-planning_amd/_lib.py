"""ctypes binding of libgnnmp.so (C ABI: include/gnnmp.h).  There is no fallback: if the
library is missing every model constructor raises."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('GNNMP_LIB') or os.path.join(_HERE, 'libgnnmp.so')      # GNNMP_LIB: an experiment build (tools/diag/build_variant.sh)

ABI_VERSION = 9                        # include/gnnmp.h gnnmp_abi_version(): what this binding was written against

c_float_p = ctypes.POINTER(ctypes.c_float)
c_int32_p = ctypes.POINTER(ctypes.c_int32)
c_int64_p = ctypes.POINTER(ctypes.c_int64)


class ExplorerDims(ctypes.Structure):
    _fields_ = [('config_size', ctypes.c_int32), ('embed_size', ctypes.c_int32), ('obs_size', ctypes.c_int32),
                ('mlp_dtype', ctypes.c_int32)]          # 0 = fp32, 1 = bf16 MFMA operands (gnnmp.h)


class Batch(ctypes.Structure):
    _fields_ = [('n_graphs', ctypes.c_int32), ('total_nodes', ctypes.c_int32), ('total_edges', ctypes.c_int32),
                ('total_obstacles', ctypes.c_int32), ('max_obstacles', ctypes.c_int32),
                ('v', ctypes.c_void_p), ('goal', ctypes.c_void_p), ('obstacles', ctypes.c_void_p),
                ('edge_index', ctypes.c_void_p), ('node_ptr', ctypes.c_void_p), ('edge_ptr', ctypes.c_void_p),
                ('obs_ptr', ctypes.c_void_p)]


class SmootherDims(ctypes.Structure):
    _fields_ = [('config_size', ctypes.c_int32), ('embed_size', ctypes.c_int32), ('scale', ctypes.c_float),
                ('mlp_dtype', ctypes.c_int32)]


class SmoothBatch(ctypes.Structure):
    _fields_ = [('n_problems', ctypes.c_int32), ('total_path', ctypes.c_int32), ('total_free', ctypes.c_int32),
                ('total_collided', ctypes.c_int32), ('total_edges', ctypes.c_int32), ('max_path', ctypes.c_int32),
                ('max_samples', ctypes.c_int32), ('max_edges', ctypes.c_int32),
                ('path', ctypes.c_void_p), ('free_pts', ctypes.c_void_p), ('collided', ctypes.c_void_p),
                ('edge_index', ctypes.c_void_p), ('path_ptr', ctypes.c_void_p), ('free_ptr', ctypes.c_void_p),
                ('coll_ptr', ctypes.c_void_p), ('edge_ptr', ctypes.c_void_p)]


STAGES = ('prep', 'obs', 'node_pre', 'edge_pre', 'mp', 'policy')

class GraphBuildBatch(ctypes.Structure):
    _fields_ = [('n_graphs', ctypes.c_int32), ('total_nodes', ctypes.c_int32), ('k1_max', ctypes.c_int32),
                ('config_size', ctypes.c_int32), ('v', ctypes.c_void_p), ('node_ptr', ctypes.c_void_p),
                ('n_free', ctypes.c_void_p), ('k1', ctypes.c_void_p)]


class MazeBatch(ctypes.Structure):
    _fields_ = [('n_problems', ctypes.c_int32), ('total_nodes', ctypes.c_int32), ('total_edges', ctypes.c_int32),
                ('width', ctypes.c_int32), ('v', ctypes.c_void_p), ('node_ptr', ctypes.c_void_p),
                ('edge_ptr', ctypes.c_void_p), ('n_free', ctypes.c_void_p), ('edge_index', ctypes.c_void_p),
                ('scores', ctypes.c_void_p), ('maps', ctypes.c_void_p), ('goal_states', ctypes.c_void_p)]


class MazeResume(ctypes.Structure):
    _fields_ = [('n_explored', ctypes.c_void_p), ('explored', ctypes.c_void_p), ('prev', ctypes.c_void_p),
                ('n_pairs', ctypes.c_void_p), ('pairs', ctypes.c_void_p), ('pair_ptr', ctypes.c_void_p)]


class MazeSampleBatch(ctypes.Structure):
    _fields_ = [('n_problems', ctypes.c_int32), ('width', ctypes.c_int32), ('n_free', ctypes.c_int32), ('n_attempts', ctypes.c_int64),
                ('attempts', ctypes.c_void_p), ('maps', ctypes.c_void_p), ('init_states', ctypes.c_void_p),
                ('goal_states', ctypes.c_void_p)]


class MazeRoundsState(ctypes.Structure):
    _fields_ = [('n_problems', ctypes.c_int32), ('cap', ctypes.c_int32), ('pair_cap', ctypes.c_int32),
                ('free_pool', ctypes.c_void_p), ('coll_pool', ctypes.c_void_p), ('n_free', ctypes.c_void_p),
                ('n_coll', ctypes.c_void_p), ('tree_explored', ctypes.c_void_p), ('tree_prev', ctypes.c_void_p),
                ('tree_n_explored', ctypes.c_void_p), ('tree_pairs', ctypes.c_void_p), ('tree_n_pairs', ctypes.c_void_p),
                ('tree_success', ctypes.c_void_p), ('tree_path_len', ctypes.c_void_p), ('tree_path', ctypes.c_void_p),
                ('tree_checks', ctypes.c_void_p)]


class MazeStreamsBatch(ctypes.Structure):
    _fields_ = [('n_problems', ctypes.c_int32), ('width', ctypes.c_int32), ('n_free', ctypes.c_int32), ('cap', ctypes.c_int32),
                ('n_attempts', ctypes.c_int64), ('attempts', ctypes.c_void_p), ('att_ptr', ctypes.c_void_p),
                ('att_ptr_host', ctypes.c_void_p), ('maps', ctypes.c_void_p), ('init_states', ctypes.c_void_p),
                ('goal_states', ctypes.c_void_p), ('active', ctypes.c_void_p)]


class LazySPState(ctypes.Structure):
    _fields_ = [('n_problems', ctypes.c_int32), ('cap', ctypes.c_int32), ('pair_cap', ctypes.c_int32),
                ('pool', ctypes.c_void_p), ('n_nodes', ctypes.c_void_p), ('pairs', ctypes.c_void_p), ('pair_state', ctypes.c_void_p),
                ('n_pairs', ctypes.c_void_p), ('checks', ctypes.c_void_p), ('dijkstra_runs', ctypes.c_void_p),
                ('path_len', ctypes.c_void_p), ('path', ctypes.c_void_p), ('solved', ctypes.c_void_p), ('status', ctypes.c_void_p)]


class RRTStarBatch(ctypes.Structure):
    _fields_ = [('n_problems', ctypes.c_int32), ('dim', ctypes.c_int32), ('width', ctypes.c_int32), ('t_max', ctypes.c_int32),
                ('stop_when_success', ctypes.c_int32), ('draws_per_problem', ctypes.c_int64), ('maps', ctypes.c_void_p),
                ('init_states', ctypes.c_void_p), ('goal_states', ctypes.c_void_p), ('draws', ctypes.c_void_p)]


class RRTStarTree(ctypes.Structure):
    _fields_ = [('states', ctypes.c_void_p), ('parents', ctypes.c_void_p), ('rewired_parents', ctypes.c_void_p),
                ('flags', ctypes.c_void_p), ('costs', ctypes.c_void_p), ('path_lengths', ctypes.c_void_p),
                ('cumulated_checks', ctypes.c_void_p), ('path', ctypes.c_void_p), ('n_nodes', ctypes.c_void_p),
                ('success', ctypes.c_void_p), ('last_iter', ctypes.c_void_p), ('used', ctypes.c_void_p), ('path_len', ctypes.c_void_p),
                ('status', ctypes.c_void_p)]


class BITStarBatch(ctypes.Structure):
    _fields_ = [('n_problems', ctypes.c_int32), ('dim', ctypes.c_int32), ('width', ctypes.c_int32), ('batch', ctypes.c_int32),
                ('n_batches', ctypes.c_int32), ('n_nodes', ctypes.c_int32), ('flags', ctypes.c_int32), ('edge_cap', ctypes.c_int64),
                ('maps', ctypes.c_void_p), ('pool', ctypes.c_void_p), ('r_by_batch', ctypes.c_void_p),
                ('checks_by_batch', ctypes.c_void_p)]


class BITStarResult(ctypes.Structure):
    _fields_ = [('g', ctypes.c_void_p), ('parents', ctypes.c_void_p), ('vertices', ctypes.c_void_p), ('path', ctypes.c_void_p),
                ('n_vertices', ctypes.c_void_p), ('batches_run', ctypes.c_void_p), ('success', ctypes.c_void_p),
                ('path_len', ctypes.c_void_p), ('status', ctypes.c_void_p), ('counters', ctypes.c_void_p)]


class NextPbForward(ctypes.Structure):
    _fields_ = [('n_problems', ctypes.c_int32), ('dim', ctypes.c_int32), ('width', ctypes.c_int32), ('iters', ctypes.c_int32),
                ('maps', ctypes.c_void_p), ('goals', ctypes.c_void_p), ('weights', ctypes.c_void_p), ('pb_rep', ctypes.c_void_p)]


class NextStateForward(ctypes.Structure):
    _fields_ = [('n_states', ctypes.c_int32), ('n_problems', ctypes.c_int32), ('dim', ctypes.c_int32), ('width', ctypes.c_int32),
                ('states', ctypes.c_void_p), ('problem_of_state', ctypes.c_void_p), ('pb_rep', ctypes.c_void_p),
                ('weights', ctypes.c_void_p), ('y', ctypes.c_void_p), ('status', ctypes.c_void_p)]


class NextTrain(ctypes.Structure):              # gnnmp_next_train
    _fields_ = [('n_problems', ctypes.c_int32), ('n_states', ctypes.c_int32), ('dim', ctypes.c_int32), ('width', ctypes.c_int32),
                ('iters', ctypes.c_int32), ('maps', ctypes.c_void_p), ('goals', ctypes.c_void_p), ('states', ctypes.c_void_p),
                ('problem_of_state', ctypes.c_void_p), ('weights', ctypes.c_void_p), ('pb_rep', ctypes.c_void_p),
                ('y', ctypes.c_void_p), ('status', ctypes.c_void_p), ('workspace', ctypes.c_void_p),
                ('workspace_bytes', ctypes.c_size_t)]


class NextTrainBwd(ctypes.Structure):           # gnnmp_next_train_bwd
    _fields_ = [('n_problems', ctypes.c_int32), ('n_states', ctypes.c_int32), ('dim', ctypes.c_int32), ('width', ctypes.c_int32),
                ('iters', ctypes.c_int32), ('goals', ctypes.c_void_p), ('states', ctypes.c_void_p),
                ('problem_of_state', ctypes.c_void_p), ('weights', ctypes.c_void_p), ('weights_t', ctypes.c_void_p),
                ('pb_rep', ctypes.c_void_p), ('dy', ctypes.c_void_p), ('dpb_rep', ctypes.c_void_p), ('dweights', ctypes.c_void_p),
                ('workspace', ctypes.c_void_p), ('workspace_bytes', ctypes.c_size_t)]


class NextReplay(ctypes.Structure):             # gnnmp_next_replay
    _fields_ = [('dim', ctypes.c_int32), ('cap_paths', ctypes.c_int32), ('cap_states', ctypes.c_int32),
                ('states64', ctypes.c_void_p), ('states32', ctypes.c_void_p), ('actions', ctypes.c_void_p),
                ('values', ctypes.c_void_p), ('path_ptr', ctypes.c_void_p), ('problem', ctypes.c_void_p),
                ('counts', ctypes.c_void_p), ('status', ctypes.c_void_p), ('pending', ctypes.c_void_p)]


class NextReplayTrees(ctypes.Structure):        # gnnmp_next_replay_trees
    _fields_ = [('n_problems', ctypes.c_int32), ('t_max', ctypes.c_int32), ('states', ctypes.c_void_p), ('path', ctypes.c_void_p),
                ('path_len', ctypes.c_void_p), ('success', ctypes.c_void_p), ('problem_ids', ctypes.c_void_p)]


class NextReplayPaths(ctypes.Structure):        # gnnmp_next_replay_paths
    _fields_ = [('n_paths', ctypes.c_int32), ('n_states', ctypes.c_int32), ('paths64', ctypes.c_void_p),
                ('path_ptr', ctypes.c_void_p), ('problem_ids', ctypes.c_void_p)]


class NextPathLoss(ctypes.Structure):           # gnnmp_next_path_loss_desc
    _fields_ = [('n_paths', ctypes.c_int32), ('n_states', ctypes.c_int32), ('dim', ctypes.c_int32), ('divisor', ctypes.c_int32),
                ('y', ctypes.c_void_p), ('actions', ctypes.c_void_p), ('values', ctypes.c_void_p), ('ptr', ctypes.c_void_p),
                ('terms', ctypes.c_void_p), ('loss', ctypes.c_void_p), ('dy', ctypes.c_void_p)]


class SmoothReplay(ctypes.Structure):           # gnnmp_smooth_replay
    _fields_ = [('config_size', ctypes.c_int32), ('cap_samples', ctypes.c_int32), ('cap_path_rows', ctypes.c_int32),
                ('cap_free_rows', ctypes.c_int32), ('cap_coll_rows', ctypes.c_int32), ('epoch', ctypes.c_int32),
                ('path', ctypes.c_void_p), ('target', ctypes.c_void_p), ('free_pts', ctypes.c_void_p), ('collided', ctypes.c_void_p),
                ('path_ptr', ctypes.c_void_p), ('free_ptr', ctypes.c_void_p), ('coll_ptr', ctypes.c_void_p),
                ('problem', ctypes.c_void_p), ('counts', ctypes.c_void_p), ('status', ctypes.c_void_p), ('pending', ctypes.c_void_p)]


class SmoothReplaySrc(ctypes.Structure):        # gnnmp_smooth_replay_src
    _fields_ = [('n_samples', ctypes.c_int32), ('total_path', ctypes.c_int32), ('total_nodes', ctypes.c_int32),
                ('take_upper', ctypes.c_int32), ('path', ctypes.c_void_p), ('target', ctypes.c_void_p), ('v', ctypes.c_void_p),
                ('path_ptr', ctypes.c_void_p), ('node_ptr', ctypes.c_void_p), ('n_free', ctypes.c_void_p), ('take', ctypes.c_void_p),
                ('problem_ids', ctypes.c_void_p)]


class EpisodeDataset(ctypes.Structure):         # gnnmp_episode_dataset
    _fields_ = [('n_problems', ctypes.c_int32), ('total_nodes', ctypes.c_int32), ('total_edges', ctypes.c_int32),
                ('total_obs', ctypes.c_int32), ('config_size', ctypes.c_int32), ('obs_size', ctypes.c_int32),
                ('v', ctypes.c_void_p), ('points64', ctypes.c_void_p), ('edge_index', ctypes.c_void_p), ('edge_free', ctypes.c_void_p),
                ('edge_cost', ctypes.c_void_p), ('obstacles', ctypes.c_void_p), ('node_ptr', ctypes.c_void_p),
                ('edge_ptr', ctypes.c_void_p), ('obs_ptr', ctypes.c_void_p), ('status', ctypes.c_void_p)]


class EpisodeDatasetBatch(ctypes.Structure):    # gnnmp_episode_dataset_batch
    _fields_ = [('n_problems', ctypes.c_int32), ('total_nodes', ctypes.c_int32), ('total_edges', ctypes.c_int32),
                ('total_obs', ctypes.c_int32),
                ('v', ctypes.c_void_p), ('points64', ctypes.c_void_p), ('edge_index', ctypes.c_void_p), ('edge_free', ctypes.c_void_p),
                ('edge_cost', ctypes.c_void_p), ('obstacles', ctypes.c_void_p), ('node_ptr', ctypes.c_void_p),
                ('edge_ptr', ctypes.c_void_p), ('obs_ptr', ctypes.c_void_p)]


class EpisodeFrontierLoss(ctypes.Structure):    # gnnmp_episode_frontier_loss_desc
    _fields_ = [('n_problems', ctypes.c_int32), ('total_edges', ctypes.c_int32), ('divisor', ctypes.c_double),
                ('frontier', ctypes.c_void_p), ('frontier_len', ctypes.c_void_p), ('label', ctypes.c_void_p),
                ('status', ctypes.c_void_p), ('edge_ptr', ctypes.c_void_p), ('scores', ctypes.c_void_p), ('terms', ctypes.c_void_p),
                ('counted', ctypes.c_void_p), ('loss', ctypes.c_void_p), ('dscores', ctypes.c_void_p), ('bad', ctypes.c_void_p)]


class SmoothPathLoss(ctypes.Structure):         # gnnmp_smooth_path_loss_desc
    _fields_ = [('n_paths', ctypes.c_int32), ('total_rows', ctypes.c_int32), ('config_size', ctypes.c_int32),
                ('divisor', ctypes.c_int32), ('path_ptr', ctypes.c_void_p), ('pred', ctypes.c_void_p), ('target', ctypes.c_void_p),
                ('terms', ctypes.c_void_p), ('loss', ctypes.c_void_p), ('d_pred', ctypes.c_void_p)]


class Next3dPbForward(ctypes.Structure):
    _fields_ = [('n_problems', ctypes.c_int32), ('dim', ctypes.c_int32), ('point_dim', ctypes.c_int32), ('width', ctypes.c_int32),
                ('iters', ctypes.c_int32), ('maps', ctypes.c_void_p), ('goals', ctypes.c_void_p), ('weights', ctypes.c_void_p),
                ('pb_rep', ctypes.c_void_p), ('workspace', ctypes.c_void_p), ('workspace_bytes', ctypes.c_size_t)]


class Next3dStateForward(ctypes.Structure):
    _fields_ = [('n_states', ctypes.c_int32), ('n_problems', ctypes.c_int32), ('dim', ctypes.c_int32), ('point_dim', ctypes.c_int32),
                ('width', ctypes.c_int32), ('inputs', ctypes.c_void_p), ('problem_of_state', ctypes.c_void_p),
                ('pb_rep', ctypes.c_void_p), ('weights', ctypes.c_void_p), ('y', ctypes.c_void_p), ('status', ctypes.c_void_p)]


class Next3dTrain(ctypes.Structure):            # gnnmp_next3d_train
    _fields_ = [('n_problems', ctypes.c_int32), ('n_states', ctypes.c_int32), ('dim', ctypes.c_int32), ('point_dim', ctypes.c_int32),
                ('width', ctypes.c_int32), ('iters', ctypes.c_int32), ('maps', ctypes.c_void_p), ('goals', ctypes.c_void_p),
                ('inputs', ctypes.c_void_p), ('problem_of_state', ctypes.c_void_p), ('weights', ctypes.c_void_p),
                ('pb_rep', ctypes.c_void_p), ('y', ctypes.c_void_p), ('status', ctypes.c_void_p), ('workspace', ctypes.c_void_p),
                ('workspace_bytes', ctypes.c_size_t)]


class Next3dTrainBwd(ctypes.Structure):         # gnnmp_next3d_train_bwd
    _fields_ = [('n_problems', ctypes.c_int32), ('n_states', ctypes.c_int32), ('dim', ctypes.c_int32), ('point_dim', ctypes.c_int32),
                ('width', ctypes.c_int32), ('iters', ctypes.c_int32), ('goals', ctypes.c_void_p), ('inputs', ctypes.c_void_p),
                ('problem_of_state', ctypes.c_void_p), ('weights', ctypes.c_void_p), ('weights_t', ctypes.c_void_p),
                ('pb_rep', ctypes.c_void_p), ('dy', ctypes.c_void_p), ('dpb_rep', ctypes.c_void_p), ('dweights', ctypes.c_void_p),
                ('workspace', ctypes.c_void_p), ('workspace_bytes', ctypes.c_size_t)]


class NextPlanBatch(ctypes.Structure):
    _fields_ = RRTStarBatch._fields_ + [('g_explore_eps', ctypes.c_double), ('c', ctypes.c_double), ('k', ctypes.c_int32),
                                        ('eps_rows', ctypes.c_int32), ('scale', ctypes.c_float), ('pb_rep', ctypes.c_void_p),
                                        ('weights', ctypes.c_void_p), ('eps', ctypes.c_void_p)]


class NextPlanTree(ctypes.Structure):
    _fields_ = RRTStarTree._fields_ + [('expanded_by_rrt', ctypes.c_void_p), ('state_values', ctypes.c_void_p), ('w', ctypes.c_void_p),
                                       ('visits', ctypes.c_void_p), ('w_sum', ctypes.c_void_p), ('guided', ctypes.c_void_p)]


class MtUniformBatch(ctypes.Structure):
    _fields_ = [('n_streams', ctypes.c_int32), ('dim', ctypes.c_int32), ('out_rows', ctypes.c_int64), ('counts', ctypes.c_void_p),
                ('out_ptr', ctypes.c_void_p), ('active', ctypes.c_void_p), ('low', ctypes.c_double * 3), ('range', ctypes.c_double * 3)]


class EpisodeGraphs(ctypes.Structure):
    _fields_ = [('n_problems', ctypes.c_int32), ('total_nodes', ctypes.c_int32), ('total_edges', ctypes.c_int32),
                ('node_ptr', ctypes.c_void_p), ('edge_ptr', ctypes.c_void_p), ('edge_index', ctypes.c_void_p)]


class OracleSmoothBatch(ctypes.Structure):
    _fields_ = [('n_paths', ctypes.c_int32), ('total_points', ctypes.c_int32), ('dim', ctypes.c_int32), ('width', ctypes.c_int32),
                ('iters', ctypes.c_int32), ('random_iter', ctypes.c_int32), ('prune_iter', ctypes.c_int32),
                ('ratio', ctypes.c_int32), ('stop', ctypes.c_int32),
                ('path_ptr', ctypes.c_void_p), ('paths', ctypes.c_void_p), ('is32', ctypes.c_void_p), ('maps', ctypes.c_void_p),
                ('action', ctypes.c_void_p), ('node_idx', ctypes.c_void_p), ('u', ctypes.c_void_p)]


class FrontierBatch(ctypes.Structure):
    _fields_ = [('n_graphs', ctypes.c_int32), ('total_nodes', ctypes.c_int32), ('total_edges', ctypes.c_int32),
                ('edge_index', ctypes.c_void_p), ('scores', ctypes.c_void_p), ('node_ptr', ctypes.c_void_p),
                ('edge_ptr', ctypes.c_void_p), ('n_free', ctypes.c_void_p)]


class TrainGeom(ctypes.Structure):
    """gnnmp_train_geom: filled by gnnmp_train_geom_build, handed back to gnnmp_train_op (test hooks only)."""
    _fields_ = [('n_graphs', ctypes.c_int32), ('config_size', ctypes.c_int32), ('n_pad', ctypes.c_int32), ('e_pad', ctypes.c_int32),
                ('v', ctypes.c_void_p), ('goal', ctypes.c_void_p),
                ('node_ptr', ctypes.c_void_p), ('node_ptr_pad', ctypes.c_void_p), ('ntile_graph', ctypes.c_void_p),
                ('goal_node', ctypes.c_void_p), ('row_beg', ctypes.c_void_p), ('deg', ctypes.c_void_p),
                ('csr', ctypes.c_void_p),
                ('out_beg', ctypes.c_void_p), ('out_cnt', ctypes.c_void_p), ('out_cur', ctypes.c_void_p), ('out_slot', ctypes.c_void_p)]


# operator numbers of gnnmp_train_op, in the order of the header's enum
TRAIN_OPS = ('LINEAR', 'LINEAR_DX', 'LINEAR_DW', 'RELU_BWD', 'FILL', 'NODE_IN', 'EDGE_IN', 'H0', 'H0_BWD', 'CONCAT', 'SPLIT', 'MSG_IN',
             'MSG_IN_BWD', 'POL_IN', 'POL_IN_BWD', 'SEGMENT_MAX', 'SEGMENT_MAX_BWD', 'SCORES_OUT', 'SCORES_IN', 'SM_NODES_IN', 'BN_FWD',
             'BN_BWD', 'SM_MSG_IN', 'SM_MSG_IN_BWD', 'SM_SCATTER_ADD', 'SM_SCATTER_ADD_BWD', 'ADD_ROWS', 'SM_PATH_UPDATE',
             'SM_PATH_UPDATE_BWD', 'SM_COORDS_BWD', 'SCALE',
             'SM_NODES_IN_SEG', 'BN_SEG_FWD', 'BN_SEG_BWD', 'BN_SEG_DGB', 'SM_MSG_IN_SEG', 'SM_MSG_IN_BWD_SEG', 'SM_SCATTER_ADD_SEG',
             'SM_SCATTER_ADD_BWD_SEG', 'SM_ADD_PATH_SEG', 'SM_ADD_PATH_BWD_SEG', 'SM_PATH_UPDATE_SEG', 'SM_PATH_UPDATE_BWD_SEG',
             'SM_COORDS_BWD_SEG', 'FINAL_CAT', 'SEED_DH', 'LINEAR_DW_ORDER')


_lib = None


def lib():
    """The loaded library (raises RuntimeError with a build hint if it is not there)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            'libgnnmp.so not found at %s -- build it with `python -c "import __graft_entry__ as g; g.build()"` '
            '(hipcc --offload-arch=gfx950).  There is no CPU / PyTorch fallback for the forward passes.' % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    L.gnnmp_status_string.restype = ctypes.c_char_p
    L.gnnmp_status_string.argtypes = [ctypes.c_int]
    L.gnnmp_last_hip_error.restype = ctypes.c_char_p
    # the ABI number is checked before anything else is bound: a stale build (an experiment library left in GNNMP_LIB, an
    # in-tree .so older than this binding) would otherwise change results or crash with no indication
    if not hasattr(L, 'gnnmp_abi_version'):
        raise RuntimeError('%s exports no gnnmp_abi_version: not a libgnnmp build this binding can use' % LIB_PATH)
    L.gnnmp_abi_version.restype = ctypes.c_int
    abi = L.gnnmp_abi_version()
    if abi != ABI_VERSION:
        raise RuntimeError('%s has ABI version %d, this binding expects %d -- rebuild it (`python -c "import __graft_entry__ '
                           'as g; g.build(force=True)"`)%s' % (LIB_PATH, abi, ABI_VERSION,
                                                               ' or unset GNNMP_LIB' if os.environ.get('GNNMP_LIB') else ''))
    if os.environ.get('GNNMP_LIB'):
        import sys
        print('[gnnmp] GNNMP_LIB is set: using the experiment build %s (ABI %d) instead of the in-tree libgnnmp.so'
              % (LIB_PATH, abi), file=sys.stderr, flush=True)
    L.gnnmp_explorer_manifest.argtypes = [ctypes.POINTER(ExplorerDims), ctypes.c_int, ctypes.c_char_p, sz, c_int64_p]
    L.gnnmp_explorer_create.argtypes = [ctypes.POINTER(vp), ctypes.POINTER(ExplorerDims), vp, sz, ctypes.c_int]
    L.gnnmp_explorer_destroy.argtypes = [vp]
    L.gnnmp_explorer_workspace_bytes.argtypes = [vp, ctypes.POINTER(Batch), ctypes.POINTER(sz)]
    L.gnnmp_explorer_forward.argtypes = [vp, ctypes.POINTER(Batch), ctypes.c_int, ctypes.c_int, vp, vp, vp, sz, vp]
    L.gnnmp_explorer_debug_tap.argtypes = [vp, ctypes.POINTER(Batch), ctypes.c_int, vp, vp, sz, vp]
    L.gnnmp_smoother_grad_floats.restype = ctypes.c_int64
    L.gnnmp_smoother_grad_floats.argtypes = [vp]
    L.gnnmp_smoother_train_workspace_bytes.argtypes = [vp, ctypes.POINTER(SmoothBatch), ctypes.c_int, ctypes.POINTER(sz)]
    L.gnnmp_smoother_train_forward.argtypes = [vp, ctypes.POINTER(SmoothBatch), ctypes.c_int, vp, vp, vp, sz, vp]
    L.gnnmp_smoother_train_backward.argtypes = [vp, ctypes.POINTER(SmoothBatch), ctypes.c_int, vp, vp, vp, sz, vp]
    i32p = ctypes.POINTER(ctypes.c_int32)
    L.gnnmp_smoother_train_batch_workspace_bytes.argtypes = [vp, ctypes.POINTER(SmoothBatch), i32p, ctypes.POINTER(sz)]
    L.gnnmp_smoother_train_batch_forward.argtypes = [vp, ctypes.POINTER(SmoothBatch), i32p, vp, vp, vp, sz, vp]
    L.gnnmp_smoother_train_batch_backward.argtypes = [vp, ctypes.POINTER(SmoothBatch), i32p, vp, vp, vp, sz, vp]
    L.gnnmp_explorer_grad_floats.restype = ctypes.c_int64
    L.gnnmp_explorer_grad_floats.argtypes = [vp]
    L.gnnmp_explorer_train_workspace_bytes.argtypes = [vp, ctypes.POINTER(Batch), ctypes.c_int, ctypes.POINTER(sz)]
    L.gnnmp_explorer_train_forward.argtypes = [vp, ctypes.POINTER(Batch), ctypes.c_int, ctypes.c_int, vp, vp, sz, vp]
    L.gnnmp_explorer_train_backward.argtypes = [vp, ctypes.POINTER(Batch), ctypes.c_int, vp, vp, vp, sz, vp]
    L.gnnmp_explorer_train_batch_workspace_bytes.argtypes = [vp, ctypes.POINTER(Batch), i32p, i32p, i32p, ctypes.POINTER(sz)]
    L.gnnmp_explorer_train_batch_forward.argtypes = [vp, ctypes.POINTER(Batch), i32p, i32p, i32p, ctypes.c_int, vp, vp, sz, vp]
    L.gnnmp_explorer_train_batch_backward.argtypes = [vp, ctypes.POINTER(Batch), i32p, i32p, i32p, vp, vp, vp, sz, vp]
    L.gnnmp_explorer_train_batch_plan.argtypes = [ctypes.c_int32, i32p, i32p, i32p, ctypes.c_int32, i32p, i32p, i32p, i32p]
    L.gnnmp_explorer_forward_ex.argtypes = [vp, ctypes.POINTER(Batch), ctypes.c_int, ctypes.c_int, vp, vp, vp, sz, vp, vp]
    L.gnnmp_explorer_status_words.argtypes = [ctypes.POINTER(Batch), ctypes.POINTER(sz)]
    L.gnnmp_explorer_status.argtypes = [vp, ctypes.POINTER(Batch), vp, sz, vp, c_int32_p]
    L.gnnmp_status_copy.argtypes = [vp, vp, ctypes.c_int32, vp]
    L.gnnmp_explorer_status_region.argtypes = [vp, ctypes.POINTER(Batch), ctypes.POINTER(sz), ctypes.POINTER(sz)]
    L.gnnmp_explorer_status_decode.argtypes = [vp, ctypes.c_int, c_int32_p]
    L.gnnmp_smoother_status.argtypes = [vp, ctypes.POINTER(SmoothBatch), vp, sz, vp, c_int32_p]
    L.gnnmp_smoother_status_region.argtypes = [vp, ctypes.POINTER(SmoothBatch), ctypes.POINTER(sz), ctypes.POINTER(sz)]
    L.gnnmp_smoother_status_decode.argtypes = [vp, ctypes.c_int, c_int32_p]
    L.gnnmp_explorer_profile.argtypes = [vp, ctypes.c_int]
    L.gnnmp_explorer_profile_read.argtypes = [vp, ctypes.POINTER(ctypes.c_double), c_int64_p]
    L.gnnmp_graph_workspace_bytes.argtypes = [ctypes.POINTER(GraphBuildBatch), ctypes.POINTER(sz)]
    L.gnnmp_graph_build.argtypes = [ctypes.POINTER(GraphBuildBatch), vp, ctypes.c_int64, vp, vp, sz, vp]
    L.gnnmp_maze_explore_workspace_bytes.argtypes = [ctypes.POINTER(MazeBatch), ctypes.POINTER(sz)]
    L.gnnmp_maze_explore.argtypes = [ctypes.POINTER(MazeBatch), vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.gnnmp_maze_explore_ex.argtypes = [ctypes.POINTER(MazeBatch), ctypes.c_int32, ctypes.POINTER(MazeResume), vp, vp, vp, vp, vp,
                                        vp, vp, vp, vp, vp, sz, vp]
    L.gnnmp_maze_sample.argtypes = [ctypes.POINTER(MazeSampleBatch), vp, vp, vp, vp, vp, vp]
    L.gnnmp_stick_sample.argtypes = [ctypes.POINTER(MazeSampleBatch), vp, vp, vp, vp, vp, vp, vp]
    L.gnnmp_maze_sample_streams.argtypes = [ctypes.POINTER(MazeStreamsBatch), ctypes.c_int32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.gnnmp_mt19937_seed.argtypes = [ctypes.c_int32, vp, vp, vp]
    L.gnnmp_mt19937_uniform.argtypes = [ctypes.POINTER(MtUniformBatch), vp, vp, ctypes.c_int32, vp, vp]
    L.gnnmp_maze_rounds_gather.argtypes = [ctypes.POINTER(MazeRoundsState), ctypes.c_int32, vp, ctypes.c_int32, ctypes.c_int64, vp, vp, vp, vp,
                                           ctypes.POINTER(MazeResume), vp]
    L.gnnmp_maze_rounds_carry.argtypes = [ctypes.POINTER(MazeRoundsState), ctypes.c_int32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                          vp, vp, vp, vp]
    L.gnnmp_lazysp_pair_cap.argtypes = [ctypes.c_int32, ctypes.c_int32, i32p, c_int64_p]
    L.gnnmp_lazysp_sample.argtypes = [ctypes.POINTER(MazeStreamsBatch), ctypes.c_int32, ctypes.POINTER(LazySPState), vp, vp, vp, vp]
    L.gnnmp_lazysp_gather.argtypes = [ctypes.POINTER(LazySPState), ctypes.c_int32, ctypes.c_int32, vp, vp, ctypes.c_int64, vp, vp, vp,
                                      vp, vp]
    L.gnnmp_lazysp_workspace_bytes.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.POINTER(sz)]
    L.gnnmp_lazysp_lds_nodes.argtypes = []
    L.gnnmp_lazysp_round.argtypes = [ctypes.POINTER(LazySPState), ctypes.c_int32, ctypes.c_int32, vp, vp, ctypes.c_int64, vp, vp,
                                     ctypes.c_int32, vp, sz, vp]
    L.gnnmp_rrtstar_workspace_bytes.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(sz)]
    L.gnnmp_rrtstar_lds_nodes.argtypes = []
    L.gnnmp_rrtstar_plan.argtypes = [ctypes.POINTER(RRTStarBatch), ctypes.POINTER(RRTStarTree), vp, sz, vp]
    L.gnnmp_bitstar_sample.argtypes = [ctypes.POINTER(MazeStreamsBatch), ctypes.c_int32, ctypes.c_int32, vp, vp, vp, vp, vp]
    L.gnnmp_bitstar_workspace_bytes.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.POINTER(sz)]
    L.gnnmp_bitstar_lds_nodes.argtypes = []
    L.gnnmp_bitstar_plan.argtypes = [ctypes.POINTER(BITStarBatch), ctypes.POINTER(BITStarResult), vp, sz, vp]
    L.gnnmp_next_weights_floats.argtypes = [ctypes.c_int32, ctypes.POINTER(sz)]
    L.gnnmp_next_pb_forward.argtypes = [ctypes.POINTER(NextPbForward), vp]
    L.gnnmp_next_state_forward.argtypes = [ctypes.POINTER(NextStateForward), vp]
    L.gnnmp_next_train_workspace_bytes.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(sz)]
    L.gnnmp_next_weights_t_floats.argtypes = [ctypes.c_int32, ctypes.POINTER(sz)]
    L.gnnmp_next_train_forward.argtypes = [ctypes.POINTER(NextTrain), vp]
    L.gnnmp_next_state_backward.argtypes = [ctypes.POINTER(NextTrainBwd), vp]
    L.gnnmp_next_pb_backward.argtypes = [ctypes.POINTER(NextTrainBwd), vp]
    L.gnnmp_next_replay_append_trees.argtypes = [ctypes.POINTER(NextReplay), ctypes.POINTER(NextReplayTrees), vp]
    L.gnnmp_next_replay_append_paths.argtypes = [ctypes.POINTER(NextReplay), ctypes.POINTER(NextReplayPaths), vp]
    L.gnnmp_next_path_loss.argtypes = [ctypes.POINTER(NextPathLoss), vp]
    L.gnnmp_smooth_replay_append.argtypes = [ctypes.POINTER(SmoothReplay), ctypes.POINTER(SmoothReplaySrc), vp]
    L.gnnmp_smooth_replay_gather.argtypes = [ctypes.POINTER(SmoothReplay), ctypes.c_int32, ctypes.c_int32, vp,
                                             ctypes.POINTER(SmoothBatch), vp, vp]
    L.gnnmp_smooth_path_loss.argtypes = [ctypes.POINTER(SmoothPathLoss), vp]
    L.gnnmp_episode_dataset_gather.argtypes = [ctypes.POINTER(EpisodeDataset), ctypes.c_int32, vp, ctypes.POINTER(EpisodeDatasetBatch), vp]
    L.gnnmp_episode_frontier_loss.argtypes = [ctypes.POINTER(EpisodeFrontierLoss), vp]
    L.gnnmp_next3d_weights_floats.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(sz)]
    L.gnnmp_next3d_workspace_bytes.argtypes = [ctypes.c_int32, ctypes.POINTER(sz)]
    L.gnnmp_next3d_pb_forward.argtypes = [ctypes.POINTER(Next3dPbForward), vp]
    L.gnnmp_next3d_state_forward.argtypes = [ctypes.POINTER(Next3dStateForward), vp]
    L.gnnmp_next3d_train_workspace_bytes.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(sz)]
    L.gnnmp_next3d_weights_t_floats.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(sz)]
    L.gnnmp_next3d_train_forward.argtypes = [ctypes.POINTER(Next3dTrain), vp]
    L.gnnmp_next3d_state_backward.argtypes = [ctypes.POINTER(Next3dTrainBwd), vp]
    L.gnnmp_next3d_pb_backward.argtypes = [ctypes.POINTER(Next3dTrainBwd), vp]
    L.gnnmp_next_plan_max_nodes.argtypes = []
    L.gnnmp_next_plan.argtypes = [ctypes.POINTER(NextPlanBatch), ctypes.POINTER(NextPlanTree), vp]
    L.gnnmp_maze_steer.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.gnnmp_stick_steer.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.gnnmp_episode_label_maze.argtypes = [ctypes.POINTER(EpisodeGraphs), ctypes.c_int32, ctypes.c_int32, vp, vp, vp, vp, vp]
    L.gnnmp_episode_workspace_bytes.argtypes = [ctypes.POINTER(EpisodeGraphs), ctypes.POINTER(sz)]
    L.gnnmp_episode_paths.argtypes = [ctypes.POINTER(EpisodeGraphs), vp, vp, vp, vp, vp, vp, sz, vp]
    L.gnnmp_episode_explore.argtypes = [ctypes.POINTER(EpisodeGraphs), vp, vp, vp, vp, vp, ctypes.c_int32, vp, vp, vp, sz, vp]
    L.gnnmp_episode_frontier.argtypes = [ctypes.POINTER(EpisodeGraphs), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz,
                                         vp]
    L.gnnmp_frontier_limits.argtypes = [c_int32_p, c_int32_p]
    L.gnnmp_frontier_workspace_bytes.argtypes = [ctypes.POINTER(FrontierBatch), ctypes.POINTER(sz)]
    L.gnnmp_frontier_rank.argtypes = [ctypes.POINTER(FrontierBatch), vp, vp, vp, vp, vp, vp, sz, vp]
    L.gnnmp_oracle_smooth_limits.argtypes = [c_int32_p, c_int32_p]
    L.gnnmp_oracle_smooth.argtypes = [ctypes.POINTER(OracleSmoothBatch), vp, vp, vp, vp, vp, vp]
    L.gnnmp_stick_oracle_smooth.argtypes = [ctypes.POINTER(OracleSmoothBatch), vp, vp, vp, vp, vp, vp]
    L.gnnmp_train_geom_workspace_bytes.argtypes = [ctypes.POINTER(Batch), ctypes.c_int32, ctypes.POINTER(sz)]
    L.gnnmp_train_geom_build.argtypes = [ctypes.POINTER(Batch), ctypes.c_int32, vp, sz, ctypes.POINTER(TrainGeom), vp]
    L.gnnmp_train_op.argtypes = [ctypes.c_int, c_int64_p, ctypes.c_int, ctypes.POINTER(vp), ctypes.c_int, ctypes.POINTER(TrainGeom),
                                 ctypes.c_float, vp]
    L.gnnmp_train_dw_scratch_floats.restype = ctypes.c_int64
    L.gnnmp_train_dw_scratch_floats.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64]
    L.gnnmp_train_op_path.argtypes = [ctypes.c_int, c_int64_p, ctypes.c_int]
    L.gnnmp_pack_a_tiles.restype = ctypes.c_int64
    L.gnnmp_pack_a_tiles.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp]
    L.gnnmp_pack_a_small.restype = ctypes.c_int64
    L.gnnmp_pack_a_small.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp]
    L.gnnmp_pack_f64_ops.restype = ctypes.c_int64
    L.gnnmp_pack_f64_ops.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp]
    L.gnnmp_pack_vec.restype = ctypes.c_int64
    L.gnnmp_pack_vec.argtypes = [vp, ctypes.c_int, vp]
    if hasattr(L, 'gnnmp_smoother_create'):
        L.gnnmp_smoother_manifest.argtypes = [ctypes.POINTER(SmootherDims), ctypes.c_int, ctypes.c_char_p, sz, c_int64_p]
        L.gnnmp_smoother_create.argtypes = [ctypes.POINTER(vp), ctypes.POINTER(SmootherDims), vp, sz, ctypes.c_int]
        L.gnnmp_smoother_destroy.argtypes = [vp]
        L.gnnmp_smoother_workspace_bytes.argtypes = [vp, ctypes.POINTER(SmoothBatch), ctypes.POINTER(sz)]
        L.gnnmp_smoother_forward.argtypes = [vp, ctypes.POINTER(SmoothBatch), ctypes.c_int, vp, vp, sz, vp]
        L.gnnmp_smoother_forward_ex.argtypes = [vp, ctypes.POINTER(SmoothBatch), ctypes.c_int, vp, vp, sz, vp, vp]
    _lib = L
    return L


def check(status, what):
    if status != 0:
        L = lib()
        msg = L.gnnmp_status_string(status).decode()
        hip = L.gnnmp_last_hip_error().decode()
        raise RuntimeError('%s failed: %s%s' % (what, msg, (' [' + hip + ']') if hip else ''))


class StatusWatch:
    """Non-blocking reader of the device-side status of forwards (gnnmp.h: gnnmp_*_forward_ex / _status_decode).

    forward() never synchronises, so what only the device can see -- a graph with more obstacles than the batch promised, a
    smoothing problem beyond its caps, a node id outside its graph -- is written by the forward's own kernels into a slot of
    PINNED host memory handed to gnnmp_*_forward_ex (no copy, no extra launch).  ``acquire`` picks the next slot of a ring that is
    allocated once (a slot's buffer only ever grows), ``commit`` records the slot's event behind the forward, ``poll`` decodes the
    slots whose event has completed and raises RuntimeError naming every bad forward among them -- called at the start of the
    module's NEXT forward (no wait) and by ``check_status()`` (waits).  When all ``depth`` slots are pending the oldest is waited
    for, so an error can lag by at most ``depth`` forwards.  Slots that have not completed stay pending across an error (their
    kernels may still be writing them); nothing is ever handed back to an allocator while a forward could write it."""

    class _Slot:
        __slots__ = ('words', 'event', 'dev', 'n', 'what')

        def __init__(self):
            self.words, self.event, self.dev, self.n, self.what = None, None, -1, 0, ''

    def __init__(self, kind, depth=32):
        import threading
        self.kind, self.depth = kind, depth
        self.free = [StatusWatch._Slot() for _ in range(depth)]
        self.order = []                                 # pending slots, oldest first
        self.lock = threading.Lock()                    # planner workers run forwards of one module from several host threads

    def acquire(self, n_words, n, what):
        """A slot of >= n_words pinned ints for the forward about to be enqueued, or None while the stream is being captured."""
        import torch
        if torch.cuda.is_current_stream_capturing():    # a caller capturing forwards into a graph: no host-side bookkeeping inside
            return None
        while True:
            with self.lock:
                slot = self.free.pop() if self.free else None
            if slot is not None:
                break
            self.poll(wait_oldest=True)
        if slot.words is None or slot.words.numel() < n_words:
            slot.words = torch.empty(max(int(n_words), 64), dtype=torch.int32, pin_memory=True)       # only ever grows
        dev = torch.cuda.current_device()
        if slot.event is None or slot.dev != dev:       # an event belongs to the device it was first recorded on
            slot.event, slot.dev = torch.cuda.Event(), dev
        slot.n, slot.what = n, what
        return slot

    def commit(self, slot):
        slot.event.record()                             # current stream = the one the forward was enqueued on
        with self.lock:
            self.order.append(slot)

    def release(self, slot):                            # the forward call itself failed: nothing was enqueued
        with self.lock:
            self.free.append(slot)

    def poll(self, wait=False, wait_oldest=False):
        import torch
        if torch.cuda.is_current_stream_capturing():    # hipEventQuery is not capture-safe
            return
        bad = []
        while True:
            with self.lock:
                if not self.order:
                    break
                slot = self.order[0]
                if not (wait or wait_oldest) and not slot.event.query():
                    break
                self.order.pop(0)
            if wait or wait_oldest:
                slot.event.synchronize()
            wait_oldest = False
            first = ctypes.c_int32(-1)
            fn = lib().gnnmp_explorer_status_decode if self.kind == 'explorer' else lib().gnnmp_smoother_status_decode
            rc = fn(slot.words.data_ptr(), slot.n, ctypes.byref(first))
            if rc != 0:
                bad.append('%s (%d %ss): %s (first offending %s: %d)' % (slot.what[0], slot.what[1], 'graph' if self.kind == 'explorer' else 'problem', lib().gnnmp_status_string(rc).decode(),
                                                               'graph' if self.kind == 'explorer' else 'problem', first.value))
            with self.lock:
                self.free.append(slot)
        if bad:
            raise RuntimeError('; '.join(bad) + ' -- the results of %s wrong' % ('that forward are' if len(bad) == 1 else 'those forwards are'))


def train_op_raw(op, dims, bufs, geom=None, scalar=0.0, stream=None):
    """gnnmp_train_op (a TEST HOOK: one launcher of the training path on the caller's device buffers) -> status code.
    op: a name of TRAIN_OPS or a number; bufs: device addresses (int) or None."""
    num = TRAIN_OPS.index(op) if isinstance(op, str) else int(op)
    d = (ctypes.c_int64 * max(len(dims), 1))(*[int(x) for x in dims])
    b = (ctypes.c_void_p * max(len(bufs), 1))(*[ctypes.c_void_p(x) if x else ctypes.c_void_p() for x in bufs])
    return lib().gnnmp_train_op(num, d, len(dims), b, len(bufs), ctypes.byref(geom) if geom is not None else None,
                                ctypes.c_float(scalar), stream)


def train_op(op, dims, bufs, geom=None, scalar=0.0, stream=None):
    check(train_op_raw(op, dims, bufs, geom, scalar, stream), 'gnnmp_train_op(%s)' % (op,))


def train_op_path(op, R, K, O):
    """'mfma' or 'plain': the kernel LINEAR / LINEAR_DX / LINEAR_DW / LINEAR_DW_ORDER dispatch to at these sizes."""
    d = (ctypes.c_int64 * 3)(R, K, O)
    rc = lib().gnnmp_train_op_path(TRAIN_OPS.index(op), d, 3)
    if rc < 0:
        check(rc, 'gnnmp_train_op_path')
    return 'mfma' if rc else 'plain'


def train_dw_scratch_floats(R, K, O):
    n = lib().gnnmp_train_dw_scratch_floats(R, K, O)
    if n < 0:
        check(int(n), 'gnnmp_train_dw_scratch_floats')
    return int(n)


TRAIN_BATCH_MAX_LOOP = 64              # GNNMP_TRAIN_BATCH_MAX_LOOP of the header


def i32_array(values):
    return (ctypes.c_int32 * max(len(values), 1))(*[int(x) for x in values])


def explorer_train_batch_plan_raw(loops, node_counts, edge_counts):
    """gnnmp_explorer_train_batch_plan (host only) -> (status, active, node_rows, edge_rows): per iteration the graphs still
    running and their padded node / edge rows; the lists are empty when the status is not 0."""
    L = lib()
    G = len(loops)
    lp, nc, ec = i32_array(loops), i32_array(node_counts), i32_array(edge_counts)
    n_it = ctypes.c_int32(0)
    rc = L.gnnmp_explorer_train_batch_plan(G, lp, nc, ec, 0, None, None, None, ctypes.byref(n_it))
    if rc != 0:
        return rc, [], [], []
    cap = n_it.value
    a, nr, er = ((ctypes.c_int32 * cap)() for _ in range(3))
    rc = L.gnnmp_explorer_train_batch_plan(G, lp, nc, ec, cap, a, nr, er, ctypes.byref(n_it))
    if rc != 0:
        return rc, [], [], []
    return 0, list(a), list(nr), list(er)


def explorer_train_batch_plan(loops, node_counts, edge_counts):
    rc, a, nr, er = explorer_train_batch_plan_raw(loops, node_counts, edge_counts)
    check(rc, 'gnnmp_explorer_train_batch_plan')
    return a, nr, er


def manifest(kind, dims):
    """[(reference parameter name, numel)] in blob order."""
    L = lib()
    fn = L.gnnmp_explorer_manifest if kind == 'explorer' else L.gnnmp_smoother_manifest
    n = fn(ctypes.byref(dims), -1, None, 0, None)
    if n < 0:
        check(n, 'gnnmp_%s_manifest' % kind)
    out = []
    buf = ctypes.create_string_buffer(256)
    numel = ctypes.c_int64()
    for i in range(n):
        check(fn(ctypes.byref(dims), i, buf, 256, ctypes.byref(numel)), 'gnnmp_%s_manifest' % kind)
        out.append((buf.value.decode(), int(numel.value)))
    return out


def grads_by_manifest(grad, manifest, tensors, trainable):
    """The flat gradient blob of a train_backward call cut by ``manifest`` into one gradient per parameter of ``tensors``,
    ``None`` where ``trainable(name)`` is false.  Parameters may live on the host (the reference keeps them wherever .to() put
    them): gradients follow them."""
    out, off = [], 0
    for (name, numel), t in zip(manifest, tensors):
        out.append(grad[off:off + numel].view_as(t).to(t.device) if trainable(name) else None)
        off += numel
    return tuple(out)


class NativeHandle:
    """Owns one gnnmp_*_create handle: destroyed when the last reference goes (the module drops its reference when the
    weights change; an autograd graph keeps the handle its forward ran with until its backward is done)."""

    def __init__(self, ptr, destroy):
        self._as_parameter_ = ptr            # ctypes passes this where a void* is expected
        self._destroy = destroy

    def __del__(self):
        try:
            self._destroy(self._as_parameter_)
        except Exception:
            pass
