// kernels.hpp -- parameter blocks and launcher prototypes shared by api.cpp and the .hip files.
#pragma once
#include <hip/hip_runtime.h>
#include "layout.hpp"

namespace gnnmp {

struct PrepParams {
    int G, E, C;
    const long long* edge_index;                 // [2, E] graph-local ids
    const int *node_ptr, *edge_ptr;              // caller prefix arrays [G+1]
    const float *v, *goal;
    int *node_ptr_pad, *edge_ptr_pad;            // [G+1]
    long long* dense_ptr;                        // [G+1]
    int *deg, *cursor, *row_beg;                 // [Npad]
    int *ntile_graph, *etile_graph;              // per 32-row tile
    int4* csr;                                   // [Epad] {source, target, caller column, 0}; -1 = pad slot
    int* goal_node;                              // [G] padded node id
    int* tile_meta;                              // per 32-edge tile, see prep_graph_body
    int2* blk_span;                              // per 256-row block of the padded node space: its graph's four-tile groups [first, end)
    int* single_out;                             // non-null: ONE graph given by its totals; node_ptr / edge_ptr / obs_ptr point here
    int single_n, single_e, single_o;            //           ([0,N | 0,E | 0,O], written by the prep stage before anything reads them)
    int n_etiles;
    // device-side status of the forward (gnnmp_explorer_status): 17 ints per graph, every slot written unconditionally by exactly
    // one thread per forward (no zero-fill, no atomics): [17 g] = GNNMP_STATUS_OBSTACLES when the graph has more obstacles than
    // obs_cap (the K/V slabs are sized for max_obstacles; the attention then sees only the first obs_cap), [17 g + 1 + part] =
    // GNNMP_STATUS_NODE_ID when part `part` of the prep stage met a node id outside [0, N_g)
    const int* obs_ptr;                          // caller prefix array or nullptr (single graph: single_o)
    int obs_cap;                                 // 32 * ot_max, or INT_MAX when the forward ignores obstacles
    int* gstat;
    int lds_rows;                                // one-launch form: assemble a slice's CSR rows in LDS and write them out in slot order
};
constexpr int kGstatStride = 17;                 // 1 + the largest `parts` of the prep stage

struct ObsParams {
    const float* obstacles;
    const int* obs_ptr;
    int S;
    const float* w[2];       // packed ObsBlob for node side / edge side
    ObsBlob blob;
    float* kv[2];            // K/V slabs, node side / edge side
    int kv_stride;           // floats per (graph, block) slab = 2 * ot_max * NT * 1024
    int ot_max;
};

// node side, block 0 in fp64: extra workgroups of the obstacle launch (node_f64_body)
struct NodeF64Params {
    const float* v;
    int C;
    const int *node_ptr, *node_ptr_pad, *ntile_graph;      // ntile_graph: graph of every 32-row tile of the padded node space
    const float* w;          // F64Blob
    F64Blob blob;
    float* m0;               // out [Npad, d]: node_free_code after the attention sub-block of block 0 (input of its map_feed)
    int n_rows;              // Npad: rows of the padded node space (the last workgroup's run may end behind it)
    int n_wg;                // workgroups of this role (64 * groups padded node rows each); 0 = role not used
    int f64_first;           // dispatch order inside the obstacle launch: 1 = these workgroups before the obstacle ones
    int groups;              // 64-row groups per workgroup: 1 (few graphs: shortest chains), 4 (obstacle operands built once per 256
                             // rows) or a multiple of 4 (several 256-row blocks: the operands are rebuilt only where the graph changes)
};

struct PreParams {
    const float *v, *goal;
    int C;
    const int *node_ptr, *node_ptr_pad;
    const int* tile_graph;
    const int4* csr;
    int* rec32;              // out (EDGE): packed per-edge record of the message-passing kernels
    const int* obs_ptr;
    const int* goal_node;
    const float* enc;
    EncBlob encb;
    const float* att;        // 3 consecutive AttBlob
    const float* out;
    int out_size;
    const float* kv;
    int kv_stride, ot_max, ot_chunk;
    int wregion;             // floats reserved for the weight region of LDS
    int n_wg;                // workgroup tiles in the padded index space (set by launch_pre)
    // resident variant only
    const int* ptr_pad_total;   // node_ptr_pad or edge_ptr_pad [G+1] (the index space this launch tiles)
    const int* tile_meta;       // per 32-edge tile (EDGE only)
    int G;
    int use_obstacles;
    int out_in_lds;          // resident variant: the epilogue blob is staged into LDS too (it fits)
    float *o0, *o1, *o2, *o3, *o4;
    const float* m0;         // NODE only, optional: rows produced by node_f64_body; the kernel then skips node_free_code's encoder
                             // and the attention sub-block of block 0
    float* om;               // optional: the attention output itself (node_free_code / edge_free_code after the 3 blocks),
                             // row-major [rows of this launch's padded index space, d]: frozen input of the training path
};

struct MpFusedParams {
    const int* rec32;
    const int *row_beg, *deg, *ntile_graph, *node_ptr_pad;
    const float *A, *B, *Ke, *X, *R;
    const float *we, *wn;        // MpEBlob (staged into LDS), MpNBlob (read from global)
    const float* wn_std;         // the MpNBlob of the non-last iterations (its m3 = W_dst: B' of a tile is recomputed from its X rows)
    int last;                    // last iteration: wn holds the decoder / policy matrices and the node phase writes PT where B' went
    float *Hout, *Xout, *Aout, *Bout;
    int n_tiles;                 // 32-node tiles of the padded node space
    int store_h;
    int tpw;                     // adjacent four-tile groups per workgroup (set by launch_mp_fused)
    int G;                       // graphs: node_ptr_pad[G] / 32 = tiles actually in use (n_tiles is an upper bound)
    int order;                   // order of the four-tile groups: 0 plain, 1 mirrored pairs (tpw == 2), 2 persistent workgroups on a snake (mp_fused_kernel)
    const int2* blk_span;        // order 2: PrepParams::blk_span
    long long* trace;            // diagnostics builds only (-DGNNMP_MP_TRACE): per-wave timestamps, else nullptr
};

struct PolicyParams {
    const int4* csr;
    const int *etile_graph, *node_ptr, *node_ptr_pad;
    const long long* dense_ptr;
    const float *PS, *PT, *PE, *w;
    float *scores, *dense;
    int n_tiles;
};

struct SmParams {
    int B, C, total_path, total_edges;
    float scale;
    const float *path, *free_pts, *collided;
    const long long* edge_index;
    const int *path_ptr, *free_ptr, *coll_ptr, *edge_ptr;
    const float* w;
    SmLayout L;
    float *cur, *cur_next;            // scaled working path [total_path, C]
    int* knn;                         // [total_path, kSmK] sample index or -1
    int *e_src, *e_dst, *e_count;     // sorted unique edges per problem (padded space), count per problem
    int *seg_beg, *seg_cnt;           // per padded path node: its run of incoming edges
    int *etile_prob, *ptile_prob;     // tile -> problem (-1 unused)
    float* msg;                       // [edge capacity, d]
    float* tgt;                       // [path capacity, d] per padded path node: b00 + (W_c - W_a) x_i, written by the target role of the
    int* tgt_flag;                    //   split message kernel; [path tiles] 1 = that tile's rows are published (reset by the graph stage); may be null
    int *tile_cnt, *elist, *plist;    // [2][2] counters {edge tiles, path tiles in use} per iteration parity + the tiles' indices (any order): appended by
    int parity;                       //   the graph stage of iteration `parity`, which also zeroes the other pair; may be null (training path)
    int cand_cap, n_etiles, n_ptiles;
    int samp_cap, path_cap;           // caller's upper bounds max_b (F_b + Co_b), max_b P_b (sm_graph_kernel's LDS carve-up)
    int one_free, one_coll;           // path_ptr == nullptr: ONE problem, its sample counts (waypoints / edges: total_path / total_edges)
    int init_from_path;               // first iteration: the knn kernel also writes cur = path / scale
    float* out;                       // last iteration: the node kernel also writes out = cur * scale (else nullptr)
    int* stat;                        // [B] device-side status (gnnmp_smoother_status): 1 = the problem exceeds the caller's max_path /
                                      //   max_samples / max_edges promises and got NO edges; written unconditionally by the graph stage
};

hipError_t launch_sm_init(int n, float scale, const float* path, float* cur, hipStream_t st);
hipError_t launch_sm_final(int n, float scale, const float* cur, float* out, hipStream_t st);
hipError_t launch_sm_iter(int D, int P, const SmParams& p, hipStream_t st, int force_fallback = 0);

struct GbParams {
    int G, C, total_nodes, kmax;
    const float* v;
    const int *node_ptr, *n_free, *k1;
    int *nb_all, *nb_free;            // [total_nodes, kmax] neighbour ids (graph-local) or -1
    int *cnt, *cur, *off, *ucnt, *uoff, *gtotal;
    int *large_cnt, *large;           // nodes of graphs beyond 1024 nodes, listed by the first kNN launch for the second (large aliases uoff)
    int* bucket;                      // [4 * kmax * total_nodes] targets grouped by source
    int* edge_ptr;                    // out [G+1]
    long long* edge_index;            // out [2, out_cap]
    long long out_cap;
};
hipError_t launch_graph_build(const GbParams& p, hipStream_t st);

struct MazeParams {
    int B, total_edges, w;
    const float* v;                       // [sumN, 2]
    const int *node_ptr, *edge_ptr, *n_free;
    const long long* edge_index;          // [2, sumE] graph-local
    const float* scores;                  // [sumE]
    const double *maps, *goal_states;     // [B, w, w], [B, 2]
    int *in_ptr, *cnt, *pos, *prev;
    int2* in_rec;                         // [sumE] visible cells grouped by row: (column | dead bit 31, score bits)
    float* rb_val;                        // cached best live cell per explored row (value, column, slot in in_rec)
    int *rb_src, *rb_eid;
    int *success, *n_explored, *explored, *n_pairs, *explored_edges, *path_len, *path;
    long long* checks;
    int dim;                              // 2 (point robot, v [.,2]) or 3 (stick robot, v [.,3])
    // resume (all nullptr = fresh trees): tree and pair list of the earlier rounds
    const int *n_explored0, *explored0, *prev0, *n_pairs0, *pairs0, *pair_ptr0;
    int* prev_out;                        // optional [sumN]: parent of every explored node
};
hipError_t launch_maze_explore(const MazeParams& p, hipStream_t st);

// collision-checked steering of the smoothing stage (smoother.py:194-216) for 2-D mazes (dim = 2) and the stick robot (dim = 3)
struct MazeSteerParams {
    int B, w;
    const double* maps;                   // [B, w, w]
    const int* path_ptr;                  // [B + 1]
    const float *old_path, *new_path;     // [sumP, dim]
    float *out_path, *tmp;                // [sumP, dim]
    long long* checks;                    // [B], incremented
    int dim = 2;
    int* status = nullptr;                // dim = 3: [B], 0 = ok, 1 = MazeEnv.interpolate's orientation assert would have fired
};
hipError_t launch_maze_steer(const MazeSteerParams& p, hipStream_t st);

// rejection sampling of the explore stage for 2-D mazes on the device (eval_gnn.py:180-184 through MazeEnv.sample_n_points)
struct MazeSampleParams {
    int B, w, n;                          // problems, map width, free samples wanted per problem
    const double* attempts;               // [M, 2] the raw uniform(-1, 1) draws of the host generator, stream order
    long long M;
    const double *maps, *init_states, *goal_states;      // [B, w, w], [B, 2], [B, 2]
    float* v;                             // out: node rows [init, goal, free x n, rejected x min(rejected, n)] per problem, compact
    int* node_ptr;                        // out [B + 1]
    int* used;                            // out [B]: attempts consumed (= collision checks of the sampling)
    long long* cursor;                    // in / out: index of the next unconsumed attempt
    int* ok;                              // out: 0 = the stream ran out before the last problem had its n free samples
    long long* checks = nullptr;          // stick robot only, out [B]: collision checks of the draws consumed (0 .. 9 per draw)
};
hipError_t launch_maze_sample(const MazeSampleParams& p, hipStream_t st);
// the stick robot's (MazeEnv(dim=3)): attempts [M, 3], init / goal states [B, 3], node rows of width 3, checks required
hipError_t launch_stick_sample(const MazeSampleParams& p, hipStream_t st);

// resample rounds for a whole batch, every problem on its own sample stream (maze_kernels.hip, eval_gnn.py:191-247)
struct MazeStreamsParams {
    int B, w, n, cap, dim;                // problems, map width, free draws to append, pool capacity (rows behind init / goal), 2 / 3
    const double* attempts;               // [M, dim] the host's uniform draws, problem b's block at att_ptr[b]
    long long M;
    const long long* att_ptr;             // [B + 1]
    const double *maps, *init_states, *goal_states;      // [B, w, w], [B, dim], [B, dim]
    const unsigned char* active;          // [B] or nullptr (= all): 0 = the problem is skipped entirely
    float *free_pool, *coll_pool;         // [B, cap + 2, dim] each
    int *n_free, *n_coll;                 // [B] in / out
    int* used;                            // out [B]: draws consumed
    long long* checks;                    // out [B]: collision checks of the consumed draws
    int* status;                          // out [B]: 0 done, 1 the block ended first, 2 no room in the pools / block outside attempts
};
hipError_t launch_maze_sample_streams(const MazeStreamsParams& p, hipStream_t st);

// numpy's RandomState (MT19937) per problem on the device (rng_kernels.hip): the streams planner's draws.  A stream's state is
// uint32 key[624] + int32 pos = 625 words, get_state()'s layout.
struct MtUniformParams {
    int n, dim, commit;                   // streams, columns per row (1..3), store the advanced state
    long long out_rows;                   // rows `out` holds
    const int* counts;                    // [n] rows per stream
    const long long* out_ptr;             // [n + 1] row offset of stream b's block in out (read only when out is given)
    const unsigned char* active;          // [n] or nullptr (= all): 0 = the stream is skipped entirely
    unsigned* state;                      // [n, 625] in / out
    double* out;                          // [out_rows, dim] or nullptr: skip the rows instead of writing them
    int* status;                          // out [n]: 0 done, 2 negative count / block outside out / pos outside [0, 624] (untouched)
    double low0, low1, low2, range0, range1, range2;     // element (r, c) = low[c] + range[c] * d (scalars: an array in a
                                          // by-value kernel argument that is indexed at run time is copied to scratch)
};
hipError_t launch_mt_seed(int n, const unsigned* seeds, unsigned* state, hipStream_t st);
hipError_t launch_mt_uniform(const MtUniformParams& p, hipStream_t st);

struct MazeGatherParams {
    int A, B, dim, cap, pair_cap;         // problems of the round (the [A] / [A + 1] outputs), slots of the store
    long long v_rows;                     // rows v can hold
    const float *free_pool, *coll_pool;
    const int *n_free, *n_coll;
    const unsigned char* active;          // [B] or nullptr
    float* v;                             // out: free rows then collided rows of every active problem, compact
    int *node_ptr, *n_free_out, *slot_of; // out [A + 1], [A], [A]
    const int *tree_explored, *tree_prev, *tree_n_explored, *tree_n_pairs;      // the store ([B, cap + 2], [B, cap + 2], [B], [B])
    int *res_explored, *res_prev, *res_n_explored, *res_n_pairs, *res_pair_ptr; // out (all or none): the round's gnnmp_maze_resume
};
hipError_t launch_maze_rounds_gather(const MazeGatherParams& p, hipStream_t st);

struct MazeCarryParams {
    int A, B, cap, pair_cap;              // problems of the round, slots of the store
    const int *slot_of, *node_ptr, *edge_ptr;
    const int *success, *n_explored, *explored, *prev, *n_pairs, *pairs, *path_len, *path;      // gnnmp_maze_explore_ex's outputs
    const long long* checks;
    int *tree_explored, *tree_prev, *tree_n_explored, *tree_pairs, *tree_n_pairs, *tree_success, *tree_path_len, *tree_path;
    long long* tree_checks;
    int* status;                          // out [A]
};
hipError_t launch_maze_rounds_carry(const MazeCarryParams& p, hipStream_t st);

// ---- the LazySP baseline on maze problems (lazysp_kernels.hip, algorithm/lazy_sp.py:147-196)
struct LspSampleParams {
    int B, w, n, cap, dim;                // problems, map width, free draws to append, pool capacity (rows behind goal / start), 2 / 3
    const double* attempts;               // [M, dim], problem b's block at att_ptr[b]
    long long M;
    const long long* att_ptr;             // [B + 1]
    const double *maps, *init_states, *goal_states;      // [B, w, w], [B, dim], [B, dim]
    const unsigned char* active;          // [B] or nullptr (= all)
    double* pool;                         // [B, cap + 2, dim]: row 0 = goal, row 1 = start, then the free draws
    int* n_nodes;                         // [B] in / out
    long long* checks;                    // [B] the store's running total: incremented
    int* used;                            // out [B]
    long long* checks_out;                // out [B]: this call's checks
    int* status;                          // out [B]: 0 done, 1 the block ended first, 2 no room / block outside attempts
};
hipError_t launch_lsp_sample(const LspSampleParams& p, hipStream_t st);

struct LspGatherParams {
    int A, B, cap, dim;
    long long v_rows;
    const int* slot_of;                   // [A]
    const double* pool;
    const int* n_nodes;                   // [B]
    const int* k1_table;                  // [cap + 3]: k1 by node count
    float* v;                             // out [v_rows, dim]
    int *node_ptr, *n_free_out, *k1_out;  // out [A + 1], [A], [A]
};
hipError_t launch_lsp_gather(const LspGatherParams& p, hipStream_t st);

struct LspRoundParams {
    int A, B, cap, pair_cap, dim, w;
    long long total_edges;                // row stride of edge_index
    const int* slot_of;                   // [A] or nullptr (= j)
    const int* edge_ptr;                  // [A + 1]
    const long long* edge_index;          // [2, total_edges]
    const double* maps;                   // [B, w, w] by slot
    const double* pool;                   // the store
    const int* n_nodes;
    int *pairs, *n_pairs, *dijkstra_runs, *path_len, *path, *status, *solved;
    unsigned char* pair_state;
    long long* checks;
    double* ws_cost;                      // workspace: [total_edges]
    unsigned char* ws_flag;               // [total_edges]
    unsigned long long* ws_dist;          // [A, cap + 3] (problems beyond the LDS node count)
    int *ws_prev, *ws_rb;                 // [A, cap + 3] each
};
hipError_t launch_lsp_round(const LspRoundParams& p, hipStream_t st);
int lsp_lds_nodes();

// ---- the RRT* baseline on maze problems (rrtstar_kernels.hip, algorithm/tsa.py:12-139, 222-281)
struct RrtParams {
    int B, w, t_max, stop, dim;           // problems, map width, iterations, stop_when_success, 2 / 3
    long long draw_len;                   // raw doubles per problem
    const double *maps, *init_states, *goal_states;      // [B, w, w], [B, dim], [B, dim]
    const double* draws;                  // [B, draw_len] doubles of [0, 1)
    double* states;                       // out [B, t_max + 1, dim]
    int *parents, *rewired;               // out [B, t_max + 1], -1 for the root
    unsigned char* flags;                 // out [B, t_max + 1]: bit 0 freesp, bit 1 in_goal_region
    double *costs, *path_lengths;         // out [B, t_max + 1]
    long long* cum_checks;                // out [B, t_max + 1]
    int* path;                            // out [B, t_max + 1]
    int *n_nodes, *success, *last_iter, *used, *path_len, *status;      // out [B]
    double *ws_x, *ws_y, *ws_z, *ws_c;    // workspace [B, t_max + 1] each (trees beyond the LDS node count)
    unsigned char* ws_f;
};
hipError_t launch_rrtstar_plan(const RrtParams& p, hipStream_t st);
int rrtstar_lds_nodes();

// ---- the NEXT planning network on maze problems (next_kernels.hip, next_model/model2D.py:84-210)
struct NextPbParams {
    int B, dim, iters;                    // problems, 2 / 3, LSTM rounds
    const float *maps, *goals;            // [B, 15, 15], [B, dim]
    const float* weights;                 // next_weights_floats() packed floats
    float* pb_rep;                        // out [B, 64, 15, 15]
};
struct NextStateParams {
    int S, B, dim;                        // states, problems, 2 / 3
    const float* states;                  // [S, dim]
    const int* problem_of_state;          // [S]
    const float *pb_rep, *weights;        // [B, 64, 15, 15]
    float* y;                             // out [S, dim + 1]
    int* status;                          // [2], accumulated: rows outside [0, B), last such row + 1
};
hipError_t launch_next_pb_forward(const NextPbParams& p, hipStream_t st);
hipError_t launch_next_state_forward(const NextStateParams& p, hipStream_t st);
size_t next_weights_floats();

// ---- training the NEXT network on maze problems (next_train_kernels.hip): the forward that keeps its activations, the backward
// byte offsets into the caller's workspace, every one a multiple of 256 and computed in size_t
struct NextTrainCarve {
    size_t saved;                         // float [B][saved_floats]: x9, hl, H [iters + 1], C [iters], X [iters] as [cell][channel] rows
    size_t saved_floats;                  // floats a problem
    size_t dg;                            // float [B][256][256]: a round's gate gradients
    size_t part_pb;                       // double [B][conv / lstm range of the packed weights]
    size_t part_goal;                     // double [B][attention range]
    size_t goal_d;                        // double [B][225][8]: the gradient of x9's attention channels
    size_t part_state;                    // double [S][per-state range]
    size_t st_d;                          // double [S][528]: a12, dT, da12, da3 of a state
    size_t attn_acc;                      // double [per-state range]: the sum over the states
    size_t total;
};
void next_train_carve(int B, int iters, int S, NextTrainCarve& c);
struct NextTrainBwdParams {
    int B, S, dim, iters;
    const float *goals, *states;          // [B, dim], [S, dim]
    const int* problem_of_state;          // [S]
    const float *weights, *weights_t;     // packed; the transposed packing (next_weights_t_floats())
    const float *pb_rep, *dy;             // [B, 64, 15, 15] of the forward, [S, dim + 1]
    float *dpb_rep, *dweights;            // [B, 64, 15, 15]; next_weights_floats()
    char* ws;
    NextTrainCarve c;
};
hipError_t launch_next_train_forward(const NextPbParams& pb, const NextStateParams& st, char* ws, const NextTrainCarve& c, hipStream_t s);
hipError_t launch_next_state_backward(const NextTrainBwdParams& p, hipStream_t st);
hipError_t launch_next_pb_backward(const NextTrainBwdParams& p, hipStream_t st);
size_t next_weights_t_floats();

// ---- the replay of NEXT's training loop (next_replay_kernels.hip, train_next.py:25-68, 88-108)
struct NextReplayStore {
    int dim, cap_paths, cap_states;
    double* states64;                     // [cap_states, dim]
    float *states32, *actions, *values;   // [cap_states, dim] x 2, [cap_states]
    int *path_ptr, *problem;              // [cap_paths + 1], [cap_paths]
    int *counts, *status, *pending;       // [2] paths and states in use; [1] bits 1 / 2 / 4; [4] the append call in flight
};
struct NextReplaySrc {
    int n;                                // source paths: problems of a tree batch, or packed paths
    int t1;                               // trees: t_max + 1 rows a problem
    long long n_rows;                     // packed: rows of paths64
    const double* rows;                   // trees: states [n, t1, dim]; packed: paths64 [n_rows, dim]
    const int *path, *path_len, *success; // trees: [n, t1], [n], [n]
    const int* ptr;                       // packed: [n + 1]
    const int* problem_ids;               // [n]
};
struct NextPathLossParams {
    int G, S, dim, divisor;
    const float *y, *actions, *values;    // [S, dim + 1], [S, dim], [S]
    const int* ptr;                       // [G + 1]
    double *terms, *loss;                 // [G, 2], [1]
    float* dy;                            // [S, dim + 1]
};
hipError_t launch_next_replay_append(const NextReplayStore& st, const NextReplaySrc& s, bool trees, hipStream_t stream);
hipError_t launch_next_path_loss(const NextPathLossParams& p, hipStream_t stream);

// ---- the replay of the smoother's training loop (smoother_replay_kernels.hip, train_smoother.py:20-61, 91-99)
struct SmoothReplayStore {
    int C, cap_samples, cap_path, cap_free, cap_coll, epoch;
    float *path, *target, *free_pts, *coll;            // [cap_path, C] x 2, [cap_free, C], [cap_coll, C]
    int *path_ptr, *free_ptr, *coll_ptr, *problem;     // [cap_samples + 1] x 3, [cap_samples]
    int *counts, *status, *pending;                    // [2, 4] banks (epoch & 1 is current); [1] bits 1 / 2 / 4; [8]
};
struct SmoothReplaySrc {
    int B, total_path, total_nodes, take_upper;
    const float *path, *target, *v;                    // [total_path, C] x 2, [total_nodes, C]
    const int *path_ptr, *node_ptr, *n_free, *take, *problem_ids;      // [B + 1] x 2, [B] x 3
};
struct SmoothGatherParams {
    int G, n_samples;                                  // group entries; samples in the store (the caller's mirror)
    int total_path, total_free, total_coll, total_edges;               // the caller's totals: the sizes of the arrays below
    const int* idx;                                    // [G]
    float *path, *target, *free_pts, *coll;            // out
    long long* edge_index;                             // out [2, total_edges]
    int *path_ptr, *free_ptr, *coll_ptr, *edge_ptr;    // out [G + 1]
};
struct SmoothPathLossParams {
    int G, total_rows, C, divisor;
    const int* path_ptr;                               // [G + 1]
    const float *pred, *target;                        // [total_rows, C]
    double* terms;                                     // [G]
    float *loss, *d_pred;                              // [1], [total_rows, C]
};
hipError_t launch_smooth_replay_append(const SmoothReplayStore& st, const SmoothReplaySrc& s, hipStream_t stream);
hipError_t launch_smooth_replay_gather(const SmoothReplayStore& st, const SmoothGatherParams& p, hipStream_t stream);
hipError_t launch_smooth_path_loss(const SmoothPathLossParams& p, hipStream_t stream);

// ---- the explorer's training loop around one step (explorer_replay_kernels.hip, train_explorer.py:96-210, dijkstra.py:91-97)
struct EpisodeDatasetStore {
    int n, total_nodes, total_edges, total_obs, C, S;  // problems; rows of the arrays below; config size; obstacle row size
    const float* v;                                    // [total_nodes, C]
    const double* points64;                            // [total_nodes, C]
    const long long* edge_index;                       // [2, total_edges] graph-local
    const unsigned char* edge_free;                    // [total_edges]
    const double* edge_cost;                           // [total_edges]
    const float* obstacles;                            // [total_obs, S]
    const int *node_ptr, *edge_ptr, *obs_ptr;          // [n + 1]
    int* status;                                       // [1] bits 1 / 2
};
struct EpisodeGatherParams {
    int G, total_nodes, total_edges, total_obs;        // group entries; the caller's totals: the sizes of the arrays below
    const int* idx;                                    // [G]
    float* v;                                          // out, as in the store
    double* points64;
    long long* edge_index;                             // out [2, total_edges]
    unsigned char* edge_free;
    double* edge_cost;
    float* obstacles;
    int *node_ptr, *edge_ptr, *obs_ptr;                // out [G + 1]
};
struct EpisodeFrontierLossParams {
    int B, total_edges;
    double divisor;
    const int *frontier, *frontier_len, *label, *status, *edge_ptr;    // [2 total_edges + B], [B] x 3, [B + 1]
    const float* scores;                               // [total_edges]
    float* terms;                                      // out [B]
    int* counted;                                      // out [B]
    float *loss, *dscores;                             // out [1], [total_edges]
    int* bad;                                          // [1] bits 1 / 2 / 4, accumulated
};
hipError_t launch_episode_dataset_gather(const EpisodeDatasetStore& st, const EpisodeGatherParams& p, hipStream_t stream);
hipError_t launch_episode_frontier_loss(const EpisodeFrontierLossParams& p, hipStream_t stream);

// ---- the NEXT planning network of the arm families (next3d_kernels.hip, next_model/model3D.py:87-213)
struct Next3dPbParams {
    int B, dim, pd, iters;                // problems, state size 1 .. 15, point size 3 / 6, LSTM rounds
    const float *maps, *goals;            // [B, 15, 15, 15], [B, pd + dim]
    const float* weights;                 // next3d_weights_floats() packed floats
    float* pb_rep;                        // out [B, 64, 15, 15, 15]
    float* workspace;                     // next3d_workspace_bytes(B) bytes, 16-byte aligned
};
struct Next3dStateParams {
    int S, B, dim, pd;                    // states, problems
    const float* inputs;                  // [S, pd + dim]
    const int* problem_of_state;          // [S]
    const float* pb_rep;                  // [B, 64, 15, 15, 15]
    const float* weights;
    float* y;                             // out [S, dim + 1]
    int* status;                          // [2], accumulated: rows outside [0, B), last such row + 1
};
hipError_t launch_next3d_pb_forward(const Next3dPbParams& p, hipStream_t st);
hipError_t launch_next3d_state_forward(const Next3dStateParams& p, hipStream_t st);
size_t next3d_weights_floats();
size_t next3d_workspace_bytes(int B);

// ---- training the 3-D NEXT network (next3d_train_kernels.hip): the forward that keeps its activations, the backward
// byte offsets into the caller's workspace, every one a multiple of 256 and computed in size_t
struct Next3dTrainCarve {
    size_t saved;                         // float [B][saved_floats]: x9 [3376][16], then [3376][64] slots: hl, H [iters + 1], C [iters + 1], X [iters]
    size_t saved_floats;                  // floats a problem
    size_t bwd;                           // float [B][3][3376][64]: dh, dc, dx of the round in flight
    size_t dg;                            // float [B][3456][256]: a round's gate gradients
    size_t part_pb;                       // double [B][conv / lstm range of the packed weights]
    size_t part_goal;                     // double [B][attention range]
    size_t goal_d;                        // double [B][3375][8]: the gradient of x9's attention channels
    size_t part_state;                    // double [S][per-state range]
    size_t st_d;                          // double [S][6824]: a123, da123, dT, da3 of a row
    size_t attn_acc;                      // double [per-state range]: the sum over the rows
    size_t total;
};
void next3d_train_carve(int B, int iters, int S, Next3dTrainCarve& c);
struct Next3dTrainBwdParams {
    int B, S, dim, pd, iters;
    const float *goals, *inputs;          // [B, pd + dim], [S, pd + dim]
    const int* problem_of_state;          // [S]
    const float *weights, *weights_t;     // packed; the transposed packing (next3d_weights_t_floats())
    const float *pb_rep, *dy;             // [B, 64, 15, 15, 15] of the forward, [S, dim + 1]
    float *dpb_rep, *dweights;            // [B, 64, 15, 15, 15]; next3d_weights_floats()
    char* ws;
    Next3dTrainCarve c;
};
hipError_t launch_next3d_train_forward(const Next3dPbParams& pb, const Next3dStateParams& st, char* ws, const Next3dTrainCarve& c,
                                       hipStream_t s);
hipError_t launch_next3d_state_backward(const Next3dTrainBwdParams& p, hipStream_t st);
hipError_t launch_next3d_pb_backward(const Next3dTrainBwdParams& p, hipStream_t st);
size_t next3d_weights_t_floats();

// ---- NEXT's guided tree loop on maze problems (next_plan_kernels.hip, algorithm/tsa.py:12-81, 141-220)
struct NextPlanParams {
    RrtParams t;                          // the RRT* fields (the workspace pointers are unused: the node state lives in LDS)
    double g_explore_eps, c;              // the RRT branch's share of the non-goal iterations; the exploration weight of the scores
    int k, eps_rows;                      // candidates of a guided step (1 .. 16); rows of eps per problem
    float scale;                          // diagonal of the Cholesky factor of the policy's covariance
    const float *pb_rep, *weights;        // [B, 64, 15, 15], next_weights_floats() packed floats
    const float* eps;                     // [B, eps_rows, k, dim] standard normal draws
    signed char* by_rrt;                  // out [B, t_max + 1]: 1 RRT branch, 0 guided, -1 the root
    float* state_values;                  // out [B, t_max + 1]
    double* w;                            // out [B, t_max + 1]
    int* visits;                          // out [B, t_max + 1]
    double* w_sum;                        // out [B]
    int* guided;                          // out [B]: rows of eps used
};
hipError_t launch_next_plan(const NextPlanParams& p, hipStream_t st);
int next_plan_max_nodes();

// ---- the BIT* baseline on maze problems (bitstar_kernels.hip, algorithm/bit_star.py:18-334)
struct BitSampleParams {
    int B, w, batch, n_batches, rows, dim;   // problems, map width, free draws a batch, batches, pool rows a problem, 2 / 3
    const double* attempts;               // [M, dim], problem b's block at att_ptr[b]
    long long M;
    const long long* att_ptr;             // [B + 1]
    const double *maps, *init_states, *goal_states;      // [B, w, w], [B, dim], [B, dim]
    const unsigned char* active;          // [B] or nullptr (= all)
    double* pool;                         // out [B, rows, dim]: row 0 = start, row 1 = goal, then the free draws
    long long *used_by_batch, *checks_by_batch;          // out [B, n_batches]: cumulative attempts / sampling checks
    int* status;                          // out [B]: 0 done, 1 the block ended first, 2 block outside attempts
};
hipError_t launch_bit_sample(const BitSampleParams& p, hipStream_t st);

struct BitPlanParams {
    int B, w, batch, n_batches, rows, dim, flags;
    long long edge_cap;                   // entries of a problem's edge queue
    const double *maps, *pool, *r_by_batch;              // [B, w, w], [B, rows, dim], [B, n_batches]
    const long long* checks_by_batch;     // [B, n_batches]
    double* g;                            // out [B, rows]
    int *parents, *vertices, *path;       // out [B, rows]
    int *n_vertices, *batches_run, *success, *path_len, *status;      // out [B]
    long long* counters;                  // out [B, 8]
    double *ws_eval, *ws_vval;            // workspace: [B, edge_cap], [B, rows] (problems beyond the LDS node count)
    int *ws_esrc, *ws_etgt;               // [B, edge_cap] each
    unsigned char* ws_flag;               // [B, rows]
};
hipError_t launch_bit_plan(const BitPlanParams& p, hipStream_t st);
int bit_lds_nodes();

// ---- supervision of the explorer's training step (train_episode_kernels.hip, train_explorer.py:124-176)
struct EpLabelParams {                    // (a) edge_free / edge_cost of construct_graph for maze problems
    int B, dim, w;
    long long total_edges;
    const double* points;                 // [sumN, dim] float64
    const int *node_ptr, *edge_ptr;       // [B + 1]
    const long long* edge_index;          // [2, sumE] graph-local, coalesced
    const double* maps;                   // [B, w, w]
    unsigned char* edge_free;             // out [sumE]
    double* edge_cost;                    // out [sumE]
};
hipError_t launch_ep_label(const EpLabelParams& p, hipStream_t st);

struct EpPathsParams {                    // (b) dijkstra to goal_index[b]
    int B;
    long long total_edges;
    const int *node_ptr, *edge_ptr, *goal_index;
    const long long* edge_index;
    const double* edge_cost;              // [sumE]
    double* dist;                         // out [sumN]
    int *prev, *n_valid;                  // out [sumN], [B]
    int* row_beg;                         // ws [sumN + B]
    unsigned char* done;                  // ws [sumN]
};
hipError_t launch_ep_paths(const EpPathsParams& p, hipStream_t st);

struct EpEpisodeParams {                  // (c) explore (replay = 0) / policy_data (replay = 1)
    int B, replay, max_steps;
    long long total_edges;
    const int *node_ptr, *edge_ptr, *goal_index, *start_index, *n_valid;
    const long long* edge_index;
    const float* scores;                  // [sumE] detached edge scores
    const unsigned char* edge_free;       // [sumE]
    const double* dist;                   // [sumN] (replay)
    const int* prev;                      // [sumN] (replay)
    int *step, *status;                   // [B]: explore writes both; replay reads them
    int *frontier, *frontier_len, *label; // replay out: frontier [2 sumE + B] (problem b at 2 edge_ptr[b] + b), [B], [B]
    int *row_beg, *rev, *explored, *key_col, *key_slot;     // ws: [sumN + B], [sumE], 3 x [sumN + 2B]
    unsigned* key;                        // ws [sumN + 2B]
    unsigned char *dead, *colkill;        // ws [sumE], [sumN]
};
hipError_t launch_ep_episode(const EpEpisodeParams& p, hipStream_t st);

// ---- the smoother's training targets (oracle_smooth_kernels.hip, smoother.py:67-151), 2-D / 3-D maze paths, one wave per path
constexpr int kOracleSmoothCap = 128;         // waypoints per path
constexpr int kOracleSmoothMaxWidth = 64;     // map cells per side
struct OracleSmoothParams {
    int B, total_points, w, iters, random_iter, prune_iter, ratio, stop;
    int dim;                              // 2 (point robot) or 3 (stick robot): row width of paths / out / action
    const int* path_ptr;                  // [B + 1]
    const double* paths;                  // [sumP, dim] float64 (float32 rows upcast)
    const unsigned char* in_is32;         // [sumP] 1 = the waypoint is a float32 row; nullptr = all of them
    const unsigned char* maps;            // [B, w, w] 0 = free
    const double* action;                 // [B, iters, random_iter, dim]
    const int* node_idx;                  // [B, iters, random_iter] replayed indices, or nullptr
    const double* u;                      // [B, iters, random_iter] in [0, 1) when node_idx == nullptr
    double* out;                          // [sumP, dim], path b from row path_ptr[b], out_len[b] rows
    unsigned char* out_is32;              // [sumP]
    int* out_len;                         // [B]
    long long* checks;                    // [B] collision_check_count
    int* status;                          // [B] bits, gnnmp.h
};
hipError_t launch_oracle_smooth(const OracleSmoothParams& p, hipStream_t st);

// ---- ranked frontier rows for the host-checked planner (frontier_kernels.hip)
constexpr int kFrWaveCells = 256;             // rows up to this many cells: one wave, the row in LDS
constexpr int kFrTileCells = 2048;            // longer rows: a workgroup streams the row through LDS tiles of this many cells
struct FrontierParams {
    int G, total_nodes, total_edges;
    const long long* edge_index;          // [2, sumE] graph-local (row 0 = source b, row 1 = target a)
    const float* scores;                  // [sumE]
    const int *node_ptr, *edge_ptr;       // [G + 1] or nullptr (G == 1)
    const int* n_free;                    // [G]
    int *row_beg, *row_len, *cols;        // out [sumN], [sumN], [sumE]
    float* vals;                          // out [sumE]
    int* status;                          // out [G]
    int *cnt, *deg, *long_cnt, *long_list;        // ws: [sumN] x 2 and one int, zero on entry; [sumN]
    int *st_b, *st_e;                     // ws [sumE]: staged cells grouped by row (source, column)
    float* st_v;                          // ws [sumE]: staged score, 0 = dead
};
hipError_t launch_frontier_rank(const FrontierParams& p, hipStream_t st);

// ---- training path (train_kernels.hip)
struct TrainGeom {
    int G, C, Npad, Epad;
    const float *v, *goal;
    const int *node_ptr, *node_ptr_pad, *ntile_graph, *goal_node, *row_beg, *deg;
    const int4* csr;
    int *out_beg, *out_cnt, *out_cur, *out_slot;      // edges grouped by source (t_out_csr): [Npad] x 3, [Epad] CSR slots
};
hipError_t t_out_csr(const TrainGeom& q, hipStream_t st);
hipError_t t_sort_csr(int Npad, int4* csr, const int* row_beg, const int* deg, hipStream_t st);
size_t t_linear_dw_scratch_floats(int R, int K, int O);
// the launchers' own dispatch: true = the fp32 MFMA kernel, false = the plain one (also what the test hooks report)
bool t_linear_mfma(int K, int O);
bool t_linear_dx_mfma(int K, int O);
bool t_linear_dw_mfma(int K, int O);
hipError_t t_linear(int R, int K, int O, const float* X, const float* W, const float* b, float* Y, bool relu, hipStream_t st);
hipError_t t_linear_dx(int R, int K, int O, const float* dY, const float* W, float* dX, bool accumulate, hipStream_t st);
// R_order > R: the second stage cuts its eight slices as it would for R_order rows, so a call over a prefix of R rows sums in the
// order of the call over all R_order rows whose other rows have dY = 0 (the ragged-loop training path); 0 = R itself
hipError_t t_linear_dw(int R, int K, int O, const float* dY, const float* X, float* dW, float* db, float* scratch, hipStream_t st,
                       int R_order = 0);
hipError_t t_relu_bwd(size_t n, const float* y, float* dy, hipStream_t st);
hipError_t t_fill(size_t n, float* x, float val, hipStream_t st);
hipError_t t_node_in(const TrainGeom& q, float* out, hipStream_t st);
hipError_t t_edge_in(const TrainGeom& q, float* out, hipStream_t st);
hipError_t t_h0(const TrainGeom& q, int D, const float* goal_encoder, float* H0, hipStream_t st);
hipError_t t_h0_bwd(const TrainGeom& q, int D, const float* dH0, float* d_goal_encoder, hipStream_t st);
hipError_t t_concat(int R, int D, int parts, const float* a0, const float* a1, const float* a2, const float* a3, float* out,
                    hipStream_t st);
hipError_t t_split(int R, int D, int parts, int part, const float* d_in, float* dst, bool accumulate, hipStream_t st);
hipError_t t_msg_in(const TrainGeom& q, int D, const float* X, const float* EF, const float* EC, float* out, hipStream_t st);
hipError_t t_msg_in_bwd(const TrainGeom& q, int D, const float* dZ, float* dX, float* dEC, hipStream_t st);
hipError_t t_pol_in(const TrainGeom& q, int D, const float* Dn, const float* EF, float* out, hipStream_t st);
hipError_t t_pol_in_bwd(const TrainGeom& q, int D, const float* dP, float* dDn, hipStream_t st);
hipError_t t_segment_max(const TrainGeom& q, int D, const float* M, float* A, int* arg, hipStream_t st);
hipError_t t_segment_max_bwd(int Npad, int D, const float* dA, const int* arg, float* dM, hipStream_t st);
hipError_t t_scores_out(const TrainGeom& q, const float* slot_scores, float* out, hipStream_t st);
hipError_t t_scores_in(const TrainGeom& q, const float* d_out, float* d_slot, hipStream_t st);

// the explorer's training path with a loop count per graph, longest first (gnnmp_explorer_train_batch_*): rows[it] = padded node
// rows of the graphs still running in iteration it -- non-increasing multiples of kPad, rows[0] = all graphs
constexpr int kTrainBatchMaxLoop = 64;      // GNNMP_TRAIN_BATCH_MAX_LOOP: the table travels as a kernel argument
struct TrainLoopRows {
    int n_it;
    int rows[kTrainBatchMaxLoop];
};
// out[n] = [NC[n], H of iteration (loop count of n's graph) - 1 [n]]  (model.py:143), n < lr.rows[0]; H_it0 = iteration 0's H, the
// others it_stride floats apart.  D in {32, 64}
hipError_t t_final_cat(const TrainLoopRows& lr, int D, const float* NC, const float* H_it0, size_t it_stride, float* out, hipStream_t st);
// its adjoint, per backward iteration: dH[n] = d_dec[n] for rows in [rows_next, rows_it) (graphs whose LAST iteration this is: the
// decoder's input gradient), dH[n] = dXin[n, 3D:4D] below rows_next (graphs that ran the next iteration: h_{i-1} of its encoder input)
hipError_t t_seed_dh(int rows_it, int rows_next, int D, const float* d_dec, const float* dXin, float* dH, hipStream_t st);

hipError_t t_sm_nodes_in(int P, int F, int Co, int C, float scale, const float* cur, const float* free_pts, const float* coll, float* out,
                         hipStream_t st);
hipError_t t_bn_fwd(int N, int D, const float* x, const float* gamma, const float* beta, float* y, float* stats, bool relu, hipStream_t st);
hipError_t t_bn_bwd(int N, int D, const float* x, const float* dy, const float* gamma, const float* stats, float* dx, float* dgamma,
                    float* dbeta, hipStream_t st);
hipError_t t_sm_msg_in(const int* n_edges, int D, const int* e_src, const int* e_dst, const float* X, float* out, int cap, hipStream_t st);
hipError_t t_sm_msg_in_bwd(const int* n_edges, int D, const int* e_src, const int* e_dst, const float* dZ, float* dX, int n_rows, hipStream_t st);
hipError_t t_sm_scatter_add(const int* n_edges, int D, const int* e_dst, const float* M, float* S, int n_rows, hipStream_t st);
hipError_t t_sm_scatter_add_bwd(const int* n_edges, int D, const int* e_dst, const float* dS, float* dM, int cap, hipStream_t st);
hipError_t t_add_rows(size_t n, const float* a, const float* b, float* out, hipStream_t st);
hipError_t t_sm_path_update(int P, int C, const float* prev, const float* proposal, float* next, hipStream_t st);
hipError_t t_sm_path_update_bwd(int P, int C, const float* d_next, float* d_proposal, float* d_prev, hipStream_t st);
hipError_t t_sm_coords_bwd(int P, int C, const float* dXin, float* d_prev, hipStream_t st);
hipError_t t_scale(int n, float s, const float* x, float* y, hipStream_t st);
hipError_t launch_sm_knn_edges(const SmParams& p, hipStream_t st);      // kNN + coalesced edge list only (training path)

// the batched training path of the smoother: the batch's prefix arrays (device) and, per iteration, how many problems still run
struct SmSeg {
    const int *path_ptr, *free_ptr, *coll_ptr, *edge_ptr;   // [B + 1] each
    int B, A;                                                // problems; [0, A) are active in this iteration (loop counts descend)
    int P, Nn, Ec;                                           // total path rows, node rows (path + free + collided), padded edge slots
};
hipError_t t_sm_nodes_in_seg(const SmSeg& g, int C, float scale, const float* cur, const float* free_pts, const float* coll, float* out,
                             hipStream_t st);
hipError_t t_bn_seg_fwd(const SmSeg& g, int D, const float* x, const float* gamma, const float* beta, float* y, float* stats,
                        float* out_stats, size_t out_stride, bool relu, hipStream_t st);
hipError_t t_bn_seg_bwd(const SmSeg& g, int D, const float* x, const float* dy, const float* gamma, const float* stats, float* dx,
                        float* part, hipStream_t st);
hipError_t t_bn_seg_dgb(int L, int B, int D, const float* part, float* dgamma, float* dbeta, hipStream_t st);
hipError_t t_sm_msg_in_seg(const SmSeg& g, const int* n_edges, int D, const int* e_src, const int* e_dst, const float* X, float* out,
                           hipStream_t st);
hipError_t t_sm_msg_in_bwd_seg(const SmSeg& g, const int* n_edges, int D, const int* e_src, const int* e_dst, const float* dZ, float* dX,
                               hipStream_t st);
hipError_t t_sm_scatter_add_seg(const SmSeg& g, const int* n_edges, int D, const int* e_dst, const float* M, float* S, hipStream_t st);
hipError_t t_sm_scatter_add_bwd_seg(const SmSeg& g, const int* n_edges, int D, const int* e_dst, const float* dS, float* dM, hipStream_t st);
hipError_t t_sm_add_path_seg(const SmSeg& g, int D, const float* X, const float* Y, float* out, hipStream_t st);
hipError_t t_sm_add_path_bwd_seg(const SmSeg& g, int D, const float* dH, float* dX, hipStream_t st);
hipError_t t_sm_path_update_seg(const SmSeg& g, int C, const float* prev, const float* proposal, float* next, hipStream_t st);
hipError_t t_sm_path_update_bwd_seg(const SmSeg& g, int C, const float* d_next, float* d_proposal, float* d_prev, hipStream_t st);
hipError_t t_sm_coords_bwd_seg(const SmSeg& g, int C, const float* dXin, float* d_prev, hipStream_t st);

int prep_parts(int G, int E);
int prep_lds_row_capacity(int nodes_per_slice);   // records per workgroup (slice of a graph) that the one-launch form assembles in LDS
hipError_t launch_prep(const PrepParams& q, int Npad, int Epad, int* hist, hipStream_t st);
hipError_t launch_obs(int D, int P, const ObsParams& p, const NodeF64Params& q, int G, hipStream_t st);
int obs_f64_slots(int D, int P, const ObsParams& p, const NodeF64Params& q);    // resident workgroups of that launch, device-wide (0: no fp64 role)
hipError_t launch_pre(int D, int P, bool edge, int waves, const PreParams& p, int n_tiles32, size_t lds_bytes, hipStream_t st);
hipError_t launch_pre_resident_both(int D, int P, const PreParams& pn, const PreParams& pe, size_t lds_bytes, int node_blocks,
                                    int edge_blocks, hipStream_t st);
hipError_t launch_pre_resident(int D, int P, bool edge, const PreParams& p, size_t lds_bytes, int n_cu, hipStream_t st);
hipError_t launch_mp_fused(int D, int P, const MpFusedParams& p, hipStream_t st);
hipError_t launch_policy(int D, int P, const PolicyParams& p, hipStream_t st);
hipError_t launch_unpad_rows(int G, int total_nodes, int D, const int* node_ptr, const int* node_ptr_pad,
                             const float* src, float* dst, hipStream_t st);
hipError_t launch_zero_dense(float* dense, const long long* n_ptr, hipStream_t st);
hipError_t launch_goal_tap(int G, const int* goal_node, const int* node_ptr_pad, float* dst, hipStream_t st);

}  // namespace gnnmp
