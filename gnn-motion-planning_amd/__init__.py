"""MI355X-native GNN path-explorer / path-smoother inference (hot path of
rainorangelemon/gnn-motion-planning), behind the reference's ``nn.Module`` call boundary.

Host side is Python (tensor glue only); all arithmetic of the forward passes runs in
hand-written HIP kernels for gfx950 inside ``libgnnmp.so`` (C ABI: ``include/gnnmp.h``).
There is no CPU fallback: constructing a model without the library, or calling it with CPU
tensors, raises.
"""
from . import dist, graph_build, hostenv, serve, synth  # noqa: F401  (host-side helpers, no native code needed)
from .batch import GraphBatch  # noqa: F401
from .explorer import EncoderProcessDecoder  # noqa: F401
from .smoother import ModelSmoother, SmoothBatch  # noqa: F401
from . import episodes  # noqa: F401,E402  (training supervision: gnnmp_episode_* entry points)
from . import oracle_smooth  # noqa: F401,E402  (the smoother's training targets: gnnmp_oracle_smooth)
from . import frontier  # noqa: F401,E402  (ranked frontier rows for the host-checked planner: gnnmp_frontier_rank)
from . import rng  # noqa: F401,E402  (numpy's MT19937 per problem on the device: gnnmp_mt19937_*)
from . import lazysp  # noqa: F401,E402  (the LazySP baseline on maze problems: gnnmp_lazysp_*)
from .lazysp import eval_lazysp_device, plan_host as lazysp_plan_host, plan_maze_batch as plan_lazysp_maze_batch  # noqa: F401,E402
from . import rrtstar  # noqa: F401,E402  (the RRT* baseline on maze problems: gnnmp_rrtstar_*)
from .rrtstar import eval_rrt_device, plan_host as rrtstar_plan_host, plan_maze_batch as plan_rrtstar_maze_batch  # noqa: F401,E402
from . import bitstar  # noqa: F401,E402  (the BIT* baseline on maze problems: gnnmp_bitstar_*)
from .bitstar import eval_bit_device, plan_host as bitstar_plan_host, plan_maze_batch as plan_bitstar_maze_batch  # noqa: F401,E402
from . import next_model, next_plan  # noqa: F401,E402  (the NEXT planning network on maze problems: gnnmp_next_*; NEXT_plan on the host)
from .next_model import Model2D, NextNet  # noqa: F401,E402
from .next_plan import plan_host as next_plan_host  # noqa: F401,E402
from . import next_model3d  # noqa: F401,E402  (the NEXT planning network of the arm families: gnnmp_next3d_*)
from .next_model3d import Model3D, NextNet3D  # noqa: F401,E402
from . import next_train  # noqa: F401,E402  (NEXT training: labels, loss, packing and its adjoint, NextNetTrain on the device)
from . import next_train3d  # noqa: F401,E402  (NEXT training of the arm families: NextNet3DTrain, gnnmp_next3d_train_*)
from .next_train3d import NextNet3DTrain  # noqa: F401,E402
from . import next_replay  # noqa: F401,E402  (NEXT's training loop on mazes: the replay on the device, train(), train_env: gnnmp_next_replay_*)
from .next_replay import ReplayStore, collect_replay, path_loss, train_env_maze, train_replay  # noqa: F401,E402
from . import smoother_replay  # noqa: F401,E402  (the smoother's training loop on mazes: replay, gather, loss, train_env: gnnmp_smooth_replay_*)
from .smoother_replay import SmoothReplayStore, train_smoother_maze  # noqa: F401,E402
from . import explorer_replay  # noqa: F401,E402  (the explorer's training loop on mazes: dataset, gather, loss, schedule: gnnmp_episode_dataset_gather / _frontier_loss)
from .explorer_replay import ExplorerDataset, train_explorer_maze  # noqa: F401,E402

__all__ = ['graph_build', 'hostenv', 'synth', 'GraphBatch', 'EncoderProcessDecoder', 'ModelSmoother', 'SmoothBatch', 'episodes',
           'oracle_smooth', 'frontier', 'rng', 'lazysp', 'eval_lazysp_device', 'lazysp_plan_host', 'plan_lazysp_maze_batch', 'rrtstar',
           'eval_rrt_device', 'rrtstar_plan_host', 'plan_rrtstar_maze_batch', 'bitstar', 'eval_bit_device', 'bitstar_plan_host',
           'plan_bitstar_maze_batch', 'next_model', 'next_plan', 'Model2D', 'NextNet', 'next_plan_host',
           'next_model3d', 'Model3D', 'NextNet3D', 'next_train', 'next_train3d',
           'NextNet3DTrain', 'next_replay', 'ReplayStore', 'collect_replay', 'path_loss', 'train_env_maze', 'train_replay',
           'smoother_replay', 'SmoothReplayStore', 'train_smoother_maze', 'explorer_replay', 'ExplorerDataset',
           'train_explorer_maze']
