/*
 * gnnmp.h -- C ABI of libgnnmp.so: MI355X (gfx950) implementation of the GNN path-explorer and
 * path-smoother forward passes of rainorangelemon/gnn-motion-planning.
 *
 * The reference has no FFI layer; its boundary for this path is the torch.nn.Module protocol
 * of two classes.  Each entry point below names the reference interface it replaces:
 *
 *   gnnmp_explorer_manifest / _create / _destroy
 *       EncoderProcessDecoder.__init__ + load_state_dict      model.py:49-105, eval_gnn.py:99-101
 *   gnnmp_explorer_workspace_bytes / gnnmp_explorer_forward
 *       EncoderProcessDecoder.forward                         model.py:115-150 (call eval_gnn.py:194)
 *   gnnmp_smoother_manifest / _create / _destroy
 *       ModelSmoother.__init__ + load_state_dict              model_smoother.py:51-94, eval_gnn.py:102-104
 *   gnnmp_smoother_workspace_bytes / gnnmp_smoother_forward
 *       ModelSmoother.forward                                 model_smoother.py:104-142 (call smoother.py:243)
 *   gnnmp_explorer_forward_ex / gnnmp_smoother_forward_ex, gnnmp_*_status*          (ABI 4 / ABI 3)
 *       no counterpart: what the reference reports by raising (a node id outside the graph: tensor indexing, model.py:120) or does
 *       not have at all (it attends over ALL obstacles it is given, model.py:125-130), reported without synchronising the forward
 *   gnnmp_next_weights_floats / gnnmp_next_pb_forward / gnnmp_next_state_forward      (ABI 8)
 *       PPN.pb_forward / PPN.state_forward, batched           next_model/model2D.py:151-210 (calls model2D.py:244, 254)
 *   gnnmp_next_train_workspace_bytes / gnnmp_next_train_forward / gnnmp_next_state_backward / gnnmp_next_pb_backward
 *       one training step of PPN: forward with saved activations, backward    train_next.py:41-69 (next_model/model2D.py:84-210)
 *   gnnmp_next_replay_append_trees / gnnmp_next_replay_append_paths / gnnmp_next_path_loss
 *       train_env's replay with get_label's labels, and train()'s loss        train_next.py:25-68, 88-108
 *   gnnmp_smooth_replay_append / gnnmp_smooth_replay_gather / gnnmp_smooth_path_loss
 *       the smoother's replay, train()'s per-step batch and its loss          train_smoother.py:20-61, 91-99
 *   gnnmp_episode_dataset_gather / gnnmp_episode_frontier_loss
 *       the explorer's labelled-graph dataset, a step's batch and its loss    train_explorer.py:96-210, 172
 *   gnnmp_next_plan / gnnmp_next_plan_max_nodes                                       (ABI 9)
 *       NEXT_plan with a model, batched, one launch            algorithm/tsa.py:12-81, 141-220 (call eval_next.py:65)
 *   gnnmp_next3d_weights_floats / gnnmp_next3d_workspace_bytes / gnnmp_next3d_pb_forward / gnnmp_next3d_state_forward
 *       PPN.pb_forward / PPN.state_forward of the arm families, batched   next_model/model3D.py:154-213 (calls model3D.py:251, 265)
 *   gnnmp_next3d_train_workspace_bytes / gnnmp_next3d_weights_t_floats / gnnmp_next3d_train_forward /
 *   gnnmp_next3d_state_backward / gnnmp_next3d_pb_backward
 *       one training step of the arm families' PPN            train_next.py:41-69 (next_model/model3D.py:87-213)
 *   gnnmp_graph_workspace_bytes / gnnmp_graph_build
 *       create_data's edge construction                       eval_gnn.py:159-164
 *   gnnmp_maze_sample
 *       explore()'s rejection sampling (classification + compaction)   eval_gnn.py:180-184, environment/maze_env.py
 *   gnnmp_stick_sample
 *       the same for MazeEnv(dim=3): _stick_in_free_space per draw     environment/maze_env.py:279-314
 *   gnnmp_maze_sample_streams / gnnmp_maze_rounds_gather / gnnmp_maze_rounds_carry
 *       explore()'s resample rounds for a batch, one sample stream per problem     eval_gnn.py:191-247
 *   gnnmp_mt19937_seed / gnnmp_mt19937_uniform
 *       np.random.seed(s_b) + uniform_sample's draws, one numpy generator per problem    eval_gnn.py:180, 241-245, environment/maze_env.py
 *   gnnmp_maze_steer / gnnmp_stick_steer
 *       proposed_path_smootherv2 (steering of the smoothing stage)  smoother.py:194-216
 *   gnnmp_maze_explore_workspace_bytes / gnnmp_maze_explore / gnnmp_maze_explore_ex
 *       explore()'s greedy loop + MazeEnv._edge_fp            eval_gnn.py:198-233, environment/maze_env.py:270-326
 *   gnnmp_frontier_workspace_bytes / gnnmp_frontier_rank / gnnmp_frontier_limits
 *       explore()'s masking and the order its argmax visits a row's cells in, for a host loop that checks edges itself   eval_gnn.py:198-204
 *
 * Conventions
 *   - plain C types only; every pointer in a batch / forward call is a DEVICE pointer unless the
 *     name ends in _host; tensors are contiguous row-major fp32 / int64 / int32.
 *   - the library owns only the opaque handle (device copy of the packed weights).  Inputs,
 *     outputs and workspace are caller-allocated; nothing is retained past the call.
 *   - every kernel is enqueued on the hipStream_t passed in (as void*); no hidden device
 *     synchronisation (gnnmp_*_status and gnnmp_explorer_profile_read are the documented exceptions), no allocation inside forward -> forward is hipGraph-capturable.
 *   - functions return 0 (GNNMP_OK) or a negative gnnmp_status; no C++ exception crosses the ABI.
 *   - a handle is immutable after create: concurrent forwards from several host threads are legal
 *     with distinct workspaces / streams.
 */
#ifndef GNNMP_H
#define GNNMP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    GNNMP_OK = 0,
    GNNMP_ERR_NULL = -1,          /* required pointer is NULL                               */
    GNNMP_ERR_DIMS = -2,          /* unsupported / inconsistent dimensions                   */
    GNNMP_ERR_WEIGHTS = -3,       /* weight blob size does not match the manifest            */
    GNNMP_ERR_WORKSPACE = -4,     /* workspace too small or misaligned                       */
    GNNMP_ERR_HIP = -5,           /* a HIP runtime call failed (see gnnmp_last_hip_error)    */
    GNNMP_ERR_ARG = -6,           /* bad scalar argument (loop < 1, negative counts, ...)    */
    /* the two below are found ON THE DEVICE during a forward and returned by gnnmp_*_status (never by forward itself, which
     * does not synchronise): the scores / waypoints of that forward are WRONG */
    GNNMP_ERR_CAPS = -7,          /* a caller promise sizing the kernels was exceeded: a graph has more obstacles than
                                     max_obstacles; a smoothing problem exceeds max_path / max_samples / max_edges */
    GNNMP_ERR_INDEX = -8          /* edge_index holds a node id outside [0, N_g)             */
} gnnmp_status;

const char* gnnmp_status_string(int status);
/* hipGetErrorString of the last failing HIP call on this host thread ("" if none). */
const char* gnnmp_last_hip_error(void);
/* ABI version of this build (bumped on any incompatible change). */
int gnnmp_abi_version(void);

/* ------------------------------------------------------------------------------------------
 * Explorer   (EncoderProcessDecoder, model.py:48-150)
 * ---------------------------------------------------------------------------------------- */
typedef struct gnnmp_explorer gnnmp_explorer;   /* opaque */
enum { GNNMP_F32 = 0, GNNMP_BF16 = 1, GNNMP_BF16X3 = 2 };

typedef struct {
    int32_t config_size;   /* C  (model.py:49 config_size)                                    */
    int32_t embed_size;    /* d  (embed_size): 32 or 64 (every shipped checkpoint)             */
    int32_t obs_size;      /* S  (obs_size): obstacles are viewed as [-1, S] (model.py:126)   */
    int32_t mlp_dtype;     /* GNNMP_F32 (exact fp32 MFMA, the reference's precision) or GNNMP_BF16:
                              MFMA operands rounded to bf16, fp32 accumulate, fp32 everywhere else
                              (BASELINE configs[2], [4]); or GNNMP_BF16X3: every fp32 operand split exactly
                              into three bf16 pieces, six piece products per MAC on the bf16 matrix pipe,
                              fp32 accumulate -> fp32-class results (explorer only).  Inputs and outputs
                              stay fp32 in every mode */
} gnnmp_explorer_dims;

/* Manifest of the state_dict tensors forward() actually uses (142 of the 200 keys), in the
 * order the weight blob of gnnmp_explorer_create must concatenate them (row-major fp32, exactly
 * as stored in the reference's .pt files).  Returns the number of entries when index < 0;
 * otherwise writes the reference parameter name (NUL-terminated, <= name_cap) and its element
 * count and returns 0. */
int gnnmp_explorer_manifest(const gnnmp_explorer_dims* dims, int index,
                            char* name, size_t name_cap, int64_t* numel);

/* weights_host: HOST pointer to the concatenated manifest tensors; n_floats must equal the
 * manifest total.  device: HIP device ordinal the handle lives on (the packed weights are allocated
 * there; forward must be given streams, inputs and workspace of the SAME device).  The calling
 * thread's current HIP device is saved and restored: creating a handle never changes it. */
int gnnmp_explorer_create(gnnmp_explorer** out, const gnnmp_explorer_dims* dims,
                          const float* weights_host, size_t n_floats, int device);
int gnnmp_explorer_destroy(gnnmp_explorer* h);

/* A block-diagonal batch of independent planning graphs (the reference processes one graph per
 * call; G = 1 reproduces that).  Graph g owns node rows [node_ptr[g], node_ptr[g+1]) of v,
 * columns [edge_ptr[g], edge_ptr[g+1]) of edge_index and rows [obs_ptr[g], obs_ptr[g+1]) of
 * obstacles.  edge_index holds GRAPH-LOCAL node ids (what each problem's create_data produced),
 * row 0 = message source j, row 1 = message target i (PyG flow source_to_target); any order,
 * duplicates allowed (each column is scored independently).  Node ids must lie in [0, N_g): the reference's
 * tensor indexing would raise; here the prep stage replaces an out-of-range id by node 0 (every kernel stays inside the
 * graph's rows) and raises GNNMP_ERR_INDEX in the device-side status (gnnmp_explorer_status).
 * One graph (G = 1, the reference's own call, model.py:115) may leave node_ptr, edge_ptr and obs_ptr all NULL: the
 * three totals describe it (inference entry points only; the training entry points take explicit prefix arrays). */
typedef struct {
    int32_t n_graphs;            /* G >= 1                                                    */
    int32_t total_nodes;         /* sum_g N_g                                                 */
    int32_t total_edges;         /* sum_g E_g                                                 */
    int32_t total_obstacles;     /* sum_g O_g (may be 0)                                      */
    int32_t max_obstacles;       /* >= max_g O_g (upper bound is fine; sizes the K/V slabs).  A PROMISE: obs_ptr lives on
                                    the device and forward never reads it back.  A graph with more obstacles than
                                    this (rounded up to 32) is attended over its first ones only -- the reference
                                    attends over ALL obstacles (model.py:125-130) -- and the forward's device-side
                                    status becomes GNNMP_ERR_CAPS (gnnmp_explorer_status)     */
    const float* v;              /* [total_nodes, C]                                          */
    const float* goal;           /* [G, C]                                                    */
    const float* obstacles;      /* [total_obstacles, S]                                      */
    const int64_t* edge_index;   /* [2, total_edges]                                          */
    const int32_t* node_ptr;     /* [G+1]   (or all three NULL when G == 1)                   */
    const int32_t* edge_ptr;     /* [G+1]                                                     */
    const int32_t* obs_ptr;      /* [G+1]                                                     */
} gnnmp_batch;

int gnnmp_explorer_workspace_bytes(const gnnmp_explorer* h, const gnnmp_batch* shape /* counts only */,
                                   size_t* bytes);

/* edge_scores [total_edges]: score of every edge_index column, in the caller's column order
 *   (= policy_output[target, source] of model.py:149).
 * dense_or_null: if non-NULL, sum_g N_g^2 floats; graph g's block starts at sum_{g'<g} N_g'^2 and
 *   is the reference's zero-filled policy_output[N_g, N_g] with P[target, source] = score.
 * loop >= 1 (model.py:139); use_obstacles mirrors the attribute read at model.py:125.
 * workspace must be 256-byte aligned. */
int gnnmp_explorer_forward(const gnnmp_explorer* h, const gnnmp_batch* batch, int loop, int use_obstacles,
                           float* edge_scores, float* dense_or_null,
                           void* workspace, size_t workspace_bytes, void* hip_stream);

/* gnnmp_explorer_forward with the forward's status words (see gnnmp_explorer_status below) written to `status_out` instead of
 * the workspace region: status_out points at gnnmp_explorer_status_words(batch) ints the DEVICE can write -- normally pinned
 * (hipHostMalloc'ed) host memory: the few threads that own a status word store it straight across the bus, so there is no copy
 * behind the forward and nothing to synchronise with except an event the caller records after this call; decode with
 * gnnmp_explorer_status_decode once that event has completed.  status_out == NULL is gnnmp_explorer_forward.  (What the Python
 * wrapper does on every forward, the reference's one-graph call included: a ring of pinned slots, looked at on a later call.) */
int gnnmp_explorer_forward_ex(const gnnmp_explorer* h, const gnnmp_batch* batch, int loop, int use_obstacles,
                              float* edge_scores, float* dense_or_null,
                              void* workspace, size_t workspace_bytes, void* hip_stream, int32_t* status_out_or_null);
int gnnmp_explorer_status_words(const gnnmp_batch* shape, size_t* n_words);

/* Device-side status of the LAST forward that ran on `workspace` (same batch shape): GNNMP_OK, or GNNMP_ERR_CAPS (a graph with
 * more obstacles than batch->max_obstacles: its scores are NOT the reference's), or GNNMP_ERR_INDEX (a node id outside
 * [0, N_g)); *first_graph_or_null = the first offending graph (-1 if none).  forward() itself never synchronises, so the
 * conditions it can only see on the device are collected in a small status region of the workspace (17 ints per graph, each
 * written unconditionally by one thread per forward: no fill launch, no atomics) and read HERE: this call copies the region
 * to the host on hip_stream and WAITS for the stream (the only synchronising entry point besides profile_read).  Callers that
 * must not block use gnnmp_explorer_status_region + their own asynchronous copy + gnnmp_explorer_status_decode (what the
 * Python wrapper does: the copy rides behind the forward and is looked at on a later call).  The reference has no counterpart:
 * it attends over all obstacles it is given and its indexing raises. */
int gnnmp_explorer_status(const gnnmp_explorer* h, const gnnmp_batch* shape, const void* workspace, size_t workspace_bytes,
                          void* hip_stream, int32_t* first_graph_or_null);
int gnnmp_explorer_status_region(const gnnmp_explorer* h, const gnnmp_batch* shape, size_t* offset, size_t* bytes);
/* The non-blocking copy itself: n_words ints from a status region (device) into HOST memory that the device can write (pinned /
 * hipHostMalloc'ed), as a one-block kernel on hip_stream -- not a hipMemcpyAsync, which would order the next forward behind a DMA
 * engine that may be busy with the caller's own result copies.  Record an event behind it, decode when the event has completed. */
int gnnmp_status_copy(const int32_t* src_device, int32_t* dst_host_mapped, int32_t n_words, void* hip_stream);
int gnnmp_explorer_status_decode(const int32_t* words_host, int n_graphs, int32_t* first_graph_or_null);

/* Optional per-stage timing.  While enabled, every forward on this handle records a HIP event pair
 * around each stage ON THE STREAM THE STAGE IS LAUNCHED ON; gnnmp_explorer_profile_read waits for
 * the recorded events, returns the summed milliseconds and the number of launches per stage since
 * the last read, and recycles the events.  Profiling mutates the handle: use it from one host
 * thread.  (There is no reference counterpart; eval_gnn.py:193-196 only wall-clocks the call.) */
enum {
    GNNMP_STAGE_PREP = 0,      /* memsets + CSR-by-destination build + goal node                */
    GNNMP_STAGE_OBS = 1,       /* obstacle codes and K/V operands                               */
    GNNMP_STAGE_NODE_PRE = 2,  /* node encoders + 3 attention blocks + loop invariants          */
    GNNMP_STAGE_EDGE_PRE = 3,  /* edge encoders + 3 attention blocks + loop invariants (dominant) */
    GNNMP_STAGE_MP = 4,        /* message passing: message MLP + max aggregation + node update, ONE fused launch
                                  per loop iteration                                            */
    GNNMP_STAGE_POLICY = 5,    /* per-edge policy head                                          */
    GNNMP_N_STAGES = 6
};
int gnnmp_explorer_profile(gnnmp_explorer* h, int enable);
int gnnmp_explorer_profile_read(gnnmp_explorer* h, double* ms_sum /* [GNNMP_N_STAGES] */,
                                int64_t* launches /* [GNNMP_N_STAGES] */);

/* Test hook: after a forward, copy an intermediate out of `workspace` into `dst` (device, fp32,
 * row-major, caller node/edge order).  which: 0 = loop-invariant part of the encoder output [total_nodes, d]
 * (model.py:141 without the h_i term), 1 = final h_i [total_nodes, d] (model.py:142), 2 = decode [total_nodes, d]
 * (model.py:143), 3 = goal node per graph as float [G], 4 = node_free_code after the attention sub-block of node block 0 as the
 * double-precision node role left it [total_nodes, d] (forwards with obstacles).  Returns GNNMP_ERR_ARG if unknown; tap 2 is kept in
 * bf16 in the GNNMP_BF16 mode (its only reader is an MFMA operand) and returns GNNMP_ERR_DIMS there, as does tap 4 where that role
 * is off (GNNMP_BF16, GNNMP_NODE_F64=0). */
int gnnmp_explorer_debug_tap(const gnnmp_explorer* h, const gnnmp_batch* batch, int which, float* dst,
                             void* workspace, size_t workspace_bytes, void* hip_stream);

/* ------------------------------------------------------------------------------------------
 * Training path of the explorer   (train_explorer.py:156-186: loss.backward() through model.py:115-150)
 * ------------------------------------------------------------------------------------------
 * The reference detaches node_free_code / edge_free_code before every use (model.py:141,142,146), so its policy loss
 * trains node_code, edge_code, goal_encoder, encoder, process.lin_0 / lin_1, decoder and policy and leaves the
 * obstacle-attention stack untouched.  train_forward computes the same scores as forward (the frozen attention outputs
 * come from the inference kernels, the trainable part is re-evaluated in the reference's formulation with activations
 * kept in `workspace`); train_backward turns d loss / d edge_scores into d loss / d parameters.
 * grad: DEVICE buffer of gnnmp_explorer_grad_floats(h) floats in MANIFEST order (the layout of the weight blob given to
 * gnnmp_explorer_create); entries of frozen tensors are zero.  The handle must be GNNMP_F32.  The same workspace
 * (>= gnnmp_explorer_train_workspace_bytes, 256-byte aligned) must be passed to forward and backward, untouched in
 * between; both enqueue on hip_stream and never synchronise.  No kernel of the training path uses float atomics and every
 * sum has a fixed order (CSR segments are sorted by caller column first): the same inputs give the same gradient bits on
 * every run. */
int64_t gnnmp_explorer_grad_floats(const gnnmp_explorer* h);
int gnnmp_explorer_train_workspace_bytes(const gnnmp_explorer* h, const gnnmp_batch* shape, int loop, size_t* bytes);
int gnnmp_explorer_train_forward(const gnnmp_explorer* h, const gnnmp_batch* batch, int loop, int use_obstacles,
                                 float* edge_scores, void* workspace, size_t workspace_bytes, void* hip_stream);
int gnnmp_explorer_train_backward(const gnnmp_explorer* h, const gnnmp_batch* batch, int loop, const float* d_edge_scores,
                                  float* grad, void* workspace, size_t workspace_bytes, void* hip_stream);

/* The same with a loop count PER GRAPH (train_explorer.py:148 draws one per sample): graph g's scores are the reference's
 * model(..., loop = loops_host[g]) -- its hidden state after loops_host[g] iterations goes through decoder and policy
 * (model.py:139-146) -- and after that the graph takes part in nothing: no message, no aggregation, no weight gradient.
 * loops_host [G] is HOST memory (it decides how many launches are made): every entry >= 1 and at most
 * GNNMP_TRAIN_BATCH_MAX_LOOP, and the graphs must come longest loop first (loops_host non-increasing; the Python wrapper
 * sorts and restores the caller's order).  The graphs still running in iteration `it` are then a prefix of the batch and,
 * because every graph's rows start at a multiple of 256 in the padded node space and in the padded CSR edge space, a
 * prefix of both: iteration `it`'s launches cover only those rows, and the number of launches depends on loops_host[0]
 * alone, never on G or on how many distinct loop values occur.  node_counts_host / edge_counts_host [G]: host copies of
 * the per-graph node and edge counts (batch->node_ptr / edge_ptr are device memory and nothing is read back); they must
 * sum to batch->total_nodes / total_edges.  train_batch_backward returns the SUM over graphs of d loss / d parameters in
 * manifest order, frozen tensors zero, bit-identical for identical inputs (no float atomics, fixed summation orders).
 * With all loops equal the result is the uniform call's, bit for bit.  The workspace is the uniform call's at
 * loop = loops_host[0]; the same workspace, loops and counts go to forward and backward.
 * GNNMP_ERR_NULL for NULL arguments (the prefix arrays included), GNNMP_ERR_ARG for a loop below 1 or above the limit, an
 * ascending pair, a negative count or counts that do not sum to the batch totals, GNNMP_ERR_DIMS for a non-fp32 handle,
 * GNNMP_ERR_WORKSPACE as elsewhere. */
#define GNNMP_TRAIN_BATCH_MAX_LOOP 64
int gnnmp_explorer_train_batch_workspace_bytes(const gnnmp_explorer* h, const gnnmp_batch* shape, const int32_t* loops_host,
                                               const int32_t* node_counts_host, const int32_t* edge_counts_host, size_t* bytes);
int gnnmp_explorer_train_batch_forward(const gnnmp_explorer* h, const gnnmp_batch* batch, const int32_t* loops_host,
                                       const int32_t* node_counts_host, const int32_t* edge_counts_host, int use_obstacles,
                                       float* edge_scores, void* workspace, size_t workspace_bytes, void* hip_stream);
int gnnmp_explorer_train_batch_backward(const gnnmp_explorer* h, const gnnmp_batch* batch, const int32_t* loops_host,
                                        const int32_t* node_counts_host, const int32_t* edge_counts_host,
                                        const float* d_edge_scores, float* grad, void* workspace, size_t workspace_bytes,
                                        void* hip_stream);
/* Host only (no device needed): the launch sizes of the two calls above.  For it in [0, loops_host[0]): active[it] = the
 * number of graphs with loops_host[g] > it (a prefix of the batch), node_rows[it] / edge_rows[it] = the sum over those
 * graphs of the node / edge count rounded up to 256 -- the prep stage's rule for node_ptr_pad and the CSR ranges.
 * *n_iters = loops_host[0]; the three arrays hold `cap` entries each and may be NULL together with cap = 0 to ask for
 * n_iters alone.  Same argument errors as above, and GNNMP_ERR_ARG when 0 < cap < loops_host[0].  The forward and the
 * backward size their launches with this very function. */
int gnnmp_explorer_train_batch_plan(int32_t n_graphs, const int32_t* loops_host, const int32_t* node_counts_host,
                                    const int32_t* edge_counts_host, int32_t cap, int32_t* active, int32_t* node_rows,
                                    int32_t* edge_rows, int32_t* n_iters);

/* ------------------------------------------------------------------------------------------
 * Smoother   (ModelSmoother, model_smoother.py:46-142)
 * ---------------------------------------------------------------------------------------- */
typedef struct gnnmp_smoother gnnmp_smoother;   /* opaque */

typedef struct {
    int32_t config_size;   /* C                                                               */
    int32_t embed_size;    /* d (128 in every shipped checkpoint; 32/64/128 supported)         */
    float scale;           /* ModelSmoother(scale=...) (model_smoother.py:51, str2name.py:40)   */
    int32_t mlp_dtype;     /* GNNMP_F32 or GNNMP_BF16 (MFMA operands only, as for the explorer)   */
} gnnmp_smoother_dims;

int gnnmp_smoother_manifest(const gnnmp_smoother_dims* dims, int index,
                            char* name, size_t name_cap, int64_t* numel);
/* device semantics as for gnnmp_explorer_create (current device saved and restored) */
int gnnmp_smoother_create(gnnmp_smoother** out, const gnnmp_smoother_dims* dims,
                          const float* weights_host, size_t n_floats, int device);
int gnnmp_smoother_destroy(gnnmp_smoother* h);

/* A batch of independent smoothing problems.  Problem b: path rows [path_ptr[b], path_ptr[b+1]),
 * free rows [free_ptr[b], ...), collided rows [coll_ptr[b], ...), edge columns
 * [edge_ptr[b], ...) with node ids local to that problem's [path; free; collided] stacking
 * (model_smoother.py:121).  The caller's path is never written. */
typedef struct {
    int32_t n_problems;
    int32_t total_path, total_free, total_collided, total_edges;
    /* The three max_* fields are caller PROMISES that size the kernels' LDS carve-up; the prefix arrays live on the device
     * and forward() never reads them back (no hidden synchronisation), so they are not checked against the arrays on the
     * host.  A problem that exceeds any of them gets NO kNN / chain edges (its interior waypoints then follow smooth_node of
     * the plain node codes: a wrong path) and the forward's device-side status becomes GNNMP_ERR_CAPS
     * (gnnmp_smoother_status).  Compute them from the same host-side counts the prefix arrays are built from (the Python
     * wrapper does). */
    int32_t max_path;            /* >= max_b P_b                                              */
    int32_t max_samples;         /* >= max_b (F_b + Co_b)                                     */
    int32_t max_edges;           /* >= max_b E_b                                              */
    const float* path;           /* [total_path, C]                                           */
    const float* free_pts;       /* [total_free, C]                                           */
    const float* collided;       /* [total_collided, C]                                       */
    const int64_t* edge_index;   /* [2, total_edges]                                          */
    const int32_t* path_ptr;     /* [B+1]                                                     */
    const int32_t* free_ptr;     /* [B+1]                                                     */
    const int32_t* coll_ptr;     /* [B+1]                                                     */
    const int32_t* edge_ptr;     /* [B+1]                                                     */
} gnnmp_smooth_batch;

int gnnmp_smoother_workspace_bytes(const gnnmp_smoother* h, const gnnmp_smooth_batch* shape, size_t* bytes);

/* out_path [total_path, C]: the new waypoints (end points copied through, model_smoother.py:139).
 * ONE problem (n_problems == 1, the reference's own call) may leave path_ptr, free_ptr, coll_ptr and edge_ptr all NULL:
 * the totals describe it (inference entry point only).
 * Per-problem limits of the kernels (GNNMP_ERR_DIMS beyond them, nothing is silently truncated): at most 2048 samples
 * (free + collided; the reference's planner passes at most 500 + 500, smoother.py:57-58) and at most 7500 candidate
 * edges (caller edges + 10 kNN edges per waypoint). */
int gnnmp_smoother_forward(const gnnmp_smoother* h, const gnnmp_smooth_batch* batch, int loop,
                           float* out_path, void* workspace, size_t workspace_bytes, void* hip_stream);

/* As gnnmp_explorer_forward_ex: the status words of this forward (one int per problem) go to `status_out` (device-writable,
 * normally pinned host memory) instead of the workspace; NULL = gnnmp_smoother_forward. */
int gnnmp_smoother_forward_ex(const gnnmp_smoother* h, const gnnmp_smooth_batch* batch, int loop,
                              float* out_path, void* workspace, size_t workspace_bytes, void* hip_stream, int32_t* status_out_or_null);

/* Device-side status of the LAST forward on `workspace`, as for the explorer: GNNMP_OK or GNNMP_ERR_CAPS (a problem exceeded
 * max_path / max_samples / max_edges and was smoothed WITHOUT its edges); one int per problem.  gnnmp_smoother_status
 * synchronises hip_stream; _region / _decode are the non-blocking pieces. */
int gnnmp_smoother_status(const gnnmp_smoother* h, const gnnmp_smooth_batch* shape, const void* workspace, size_t workspace_bytes,
                          void* hip_stream, int32_t* first_problem_or_null);
int gnnmp_smoother_status_region(const gnnmp_smoother* h, const gnnmp_smooth_batch* shape, size_t* offset, size_t* bytes);
int gnnmp_smoother_status_decode(const int32_t* words_host, int n_problems, int32_t* first_problem_or_null);

/* ------------------------------------------------------------------------------------------
 * Training path of the smoother   (train_smoother.py:33-61 through model_smoother.py:104-142 under model.train())
 * ------------------------------------------------------------------------------------------
 * One problem per call (batch->n_problems == 1, anything else is GNNMP_ERR_DIMS; gnnmp_smoother_train_batch_* below take B),
 * fp32 handle.  The training forward differs from the inference one where
 * the reference's does: BatchNorm (node_code.1) normalises with the statistics of THIS call's node rows (path + free +
 * collided) in every loop iteration, and activations are kept.  bn_stats_or_null [loop][2][d] receives, per iteration, the
 * batch mean and the UNBIASED batch variance (what a caller needs to update running_mean / running_var the way
 * torch.nn.BatchNorm1d does).  train_backward: d loss / d out_path [P, C] -> d loss / d parameters in manifest order
 * (gnnmp_smoother_grad_floats floats; running_mean / running_var entries stay zero).  Same workspace for both calls. */
int64_t gnnmp_smoother_grad_floats(const gnnmp_smoother* h);
int gnnmp_smoother_train_workspace_bytes(const gnnmp_smoother* h, const gnnmp_smooth_batch* shape, int loop, size_t* bytes);
int gnnmp_smoother_train_forward(const gnnmp_smoother* h, const gnnmp_smooth_batch* batch, int loop, float* out_path,
                                 float* bn_stats_or_null, void* workspace, size_t workspace_bytes, void* hip_stream);
int gnnmp_smoother_train_backward(const gnnmp_smoother* h, const gnnmp_smooth_batch* batch, int loop, const float* d_out_path,
                                  float* grad, void* workspace, size_t workspace_bytes, void* hip_stream);

/* The same for B problems per call (the eight module calls of one optimizer step, train_smoother.py:33-61, as one): the result
 * equals B independent calls above.  loops_host [B] (HOST memory: it decides how many launches are made) gives every problem
 * its own loop count >= 1, and the problems must come ordered by it, longest first (loops_host non-increasing; the Python
 * wrapper sorts and restores the caller's order), so that the problems still running in an iteration are a prefix of every
 * row range.  BatchNorm normalises every problem with the statistics of its own P_b + F_b + Co_b rows; problem b stops after
 * loops_host[b] iterations, out_path holds its state at that point (times scale), and in later iterations its rows contribute
 * nothing: no statistics, no edges, no weight gradient.  bn_stats_or_null [B][max loop][2][d]: per (problem, iteration) the
 * batch mean and the UNBIASED variance, rows past loops_host[b] zero.  train_batch_backward: d loss / d out_path
 * [total_path, C] -> the SUM over problems of d loss / d parameters, manifest order; bit-identical for identical inputs.
 * All four prefix arrays are required.  GNNMP_ERR_NULL for NULL arguments, GNNMP_ERR_ARG for a loop count below 1 or an
 * ascending pair, GNNMP_ERR_DIMS for a bf16 handle or a problem beyond the per-problem limits above, GNNMP_ERR_WORKSPACE as
 * elsewhere.  Same workspace (and the same loops_host) for forward and backward. */
int gnnmp_smoother_train_batch_workspace_bytes(const gnnmp_smoother* h, const gnnmp_smooth_batch* shape, const int32_t* loops_host,
                                               size_t* bytes);
int gnnmp_smoother_train_batch_forward(const gnnmp_smoother* h, const gnnmp_smooth_batch* batch, const int32_t* loops_host,
                                       float* out_path, float* bn_stats_or_null, void* workspace, size_t workspace_bytes,
                                       void* hip_stream);
int gnnmp_smoother_train_batch_backward(const gnnmp_smoother* h, const gnnmp_smooth_batch* batch, const int32_t* loops_host,
                                        const float* d_out_path, float* grad, void* workspace, size_t workspace_bytes,
                                        void* hip_stream);

/* ------------------------------------------------------------------------------------------
 * Graph construction on the device   (create_data, eval_gnn.py:150-165; knn_graph :160,162; coalesce :164)
 * ---------------------------------------------------------------------------------------- */
/* Graph g owns node rows [node_ptr[g], node_ptr[g+1]) of v; its first n_free[g] rows are the
 * collision-free samples; k1[g] = ceil(k * ln(n_free) / ln(100)) (eval_gnn.py:159) is computed by the
 * caller.  The result is the reference's edge set: kNN_k1(all) + reversed + kNN_k1(free only) + reversed,
 * self loops included, coalesced (sorted by (source, target), duplicates dropped), graph-local ids. */
typedef struct {
    int32_t n_graphs;
    int32_t total_nodes;
    int32_t k1_max;              /* >= max_g k1[g]                                            */
    int32_t config_size;         /* C                                                         */
    const float* v;              /* [total_nodes, C]                                          */
    const int32_t* node_ptr;     /* [G+1]                                                     */
    const int32_t* n_free;       /* [G]                                                       */
    const int32_t* k1;           /* [G]                                                       */
} gnnmp_graph_batch;

int gnnmp_graph_workspace_bytes(const gnnmp_graph_batch* shape, size_t* bytes);
/* edge_index_out: [2, out_cap] int64 with row stride out_cap (row 0 = source, row 1 = target); graph g's
 * columns are [edge_ptr_out[g], edge_ptr_out[g+1]).  4 * k1_max * total_nodes columns always suffice (the
 * no-duplicate worst case); with a smaller out_cap the columns beyond it are not written while edge_ptr_out
 * still reports the true totals, so a caller may try an estimate and repeat with edge_ptr_out[G] columns.
 * edge_ptr_out: [G+1] int32 (device). */
int gnnmp_graph_build(const gnnmp_graph_batch* batch, int64_t* edge_index_out, int64_t out_cap,
                      int32_t* edge_ptr_out, void* workspace, size_t workspace_bytes, void* hip_stream);

/* ------------------------------------------------------------------------------------------
 * Explore stage on the device for 2-D maze problems
 *   (greedy best-edge expansion eval_gnn.py:198-233 + MazeEnv collision checker maze_env.py:270-326)
 * ---------------------------------------------------------------------------------------- */
/* Problem b: node rows [node_ptr[b], node_ptr[b+1]) of v (float32 [.,2]; the first n_free[b] rows are the free
 * samples, row 0 = start, row 1 = goal sample), edge columns [edge_ptr[b], ...) of edge_index (graph-local ids)
 * with their explorer scores, its width x width occupancy map (float64, 1 = obstacle, map[x][y]) and float64
 * goal state.  One explorer forward per problem, fresh search tree (the reference's default batch = t_max). */
typedef struct {
    int32_t n_problems, total_nodes, total_edges, width;
    const float* v;
    const int32_t *node_ptr, *edge_ptr, *n_free;
    const int64_t* edge_index;
    const float* scores;
    const double* maps;          /* [B, width, width]                                         */
    const double* goal_states;   /* [B, 2]                                                    */
} gnnmp_maze_batch;

int gnnmp_maze_explore_workspace_bytes(const gnnmp_maze_batch* shape, size_t* bytes);
/* Outputs (device): success [B]; n_explored [B] and explored [total_nodes] (explored node ids in order, problem b
 * at node_ptr[b]); n_pairs [B] and explored_edges [2 * (2 * total_edges + B)] ((a, b) pairs in order, starting
 * with the reference's initial [0, 0]; problem b at int offset 2 * (2 * edge_ptr[b] + b)); path_len [B] and
 * path [total_nodes] (node ids start -> goal); checks [B] = collision-check count of the explore stage. */
int gnnmp_maze_explore(const gnnmp_maze_batch* batch, int32_t* success, int32_t* n_explored, int32_t* explored,
                       int32_t* n_pairs, int32_t* explored_edges, int32_t* path_len, int32_t* path, int64_t* checks,
                       void* workspace, size_t workspace_bytes, void* hip_stream);

/* The general form: `dim` = 2 (point robot, as above) or 3 (the stick robot of MazeEnv(dim=3): v [.,3], goal_states
 * [B,3], collision model maze_env.py:254-302,330-347), and optionally the search trees of EARLIER rounds, which is what
 * the reference's resample loop carries across explorer forwards (eval_gnn.py:235-247; node ids of free samples are
 * stable because new samples are appended behind the old ones).  resume == NULL or resume->n_explored == NULL: fresh
 * trees.  Otherwise, per problem b: n_explored[b] >= 1 explored node ids at explored[node_ptr[b] ..] (order kept),
 * prev[node_ptr[b] + node] = tree parent of every explored node, and the (a, b) pairs recorded so far
 * (n_pairs[b] of them, starting with the initial [0, 0]) at pairs[2 * pair_ptr[b] ..]; they feed the reference's
 * legacy-index mask (eval_gnn.py:202) on the new scores.  Outputs as for gnnmp_maze_explore, except that in resume mode
 * explored_edges / n_pairs hold only the pairs added by THIS round (from index 0 of the problem's slot), and
 * prev_out_or_null [total_nodes] receives the parents of all explored nodes (for the next round). */
typedef struct {
    const int32_t* n_explored;   /* [B] or NULL                                               */
    const int32_t* explored;     /* [total_nodes]                                             */
    const int32_t* prev;         /* [total_nodes]                                             */
    const int32_t* n_pairs;      /* [B]                                                       */
    const int32_t* pairs;        /* 2 ints per pair                                           */
    const int32_t* pair_ptr;     /* [B+1] (in pairs)                                          */
} gnnmp_maze_resume;
int gnnmp_maze_explore_ex(const gnnmp_maze_batch* batch, int32_t dim, const gnnmp_maze_resume* resume_or_null,
                          int32_t* success, int32_t* n_explored, int32_t* explored, int32_t* n_pairs,
                          int32_t* explored_edges, int32_t* path_len, int32_t* path, int64_t* checks,
                          int32_t* prev_out_or_null, void* workspace, size_t workspace_bytes, void* hip_stream);

/* Collision-checked steering of the smoothing stage for 2-D mazes: proposed_path_smootherv2 (smoother.py:194-216)
 * with MazeEnv's checker (maze_env.py:270-326), batched.  Problem b owns waypoints [path_ptr[b], path_ptr[b+1])
 * of old_path / new_path (float32 [.,2]: the current path and the smoother network's proposal, smoother.py:243-245).
 * out_path receives the steered path (may NOT alias old_path / new_path); tmp: [total_path, 2] float32 scratch;
 * checks [B] (int64) is INCREMENTED by the collision checks spent.  All pointers are device pointers. */
int gnnmp_maze_steer(int32_t n_problems, int32_t total_path, int32_t width, const double* maps, const int32_t* path_ptr,
                     const float* old_path, const float* new_path, float* out_path, float* tmp, int64_t* checks,
                     void* hip_stream);

/* The same steering for the 3-DoF stick robot, MazeEnv(dim=3): waypoints are float32 [.,3]; the candidate of a waypoint is
 * MazeEnv.interpolate (maze_env.py:151-172, orientation wrapped across +-0.4), every edge check is the stick's
 * (maze_env.py:316-347).  The contract is gnnmp_maze_steer's (device pointers, out_path may NOT alias old_path / new_path,
 * checks INCREMENTED, one launch on the stream); tmp [total_path, 3] float32 must be given like the 2-D entry's, but the
 * stick kernel steers in place in out_path and never touches it.  Plus status [B] (int32), written for every problem:
 * 0 = steered; 1 = one of the two asserts of the reference's interpolate would have fired, where the reference raises: the
 * displacement's orientation still exceeds 0.4 after one wrap (a proposal more than 1.2 in orientation from its waypoint),
 * or the interpolated orientation still lies outside +-0.4 after one wrap (for example a waypoint whose own orientation is
 * out of range).  That problem's out_path is its old_path and its checks entry is left as it was. */
int gnnmp_stick_steer(int32_t n_problems, int32_t total_path, int32_t width, const double* maps, const int32_t* path_ptr,
                      const float* old_path, const float* new_path, float* out_path, float* tmp, int64_t* checks,
                      int32_t* status, void* hip_stream);

/* Rejection sampling of the explore stage for 2-D mazes (eval_gnn.py:180-184 through MazeEnv.sample_n_points / uniform_sample,
 * environment/maze_env.py): the raw draws stay with the host's numpy generator (`attempts` is the stream of uniform(-1, 1) pairs in
 * draw order, float64, DEVICE memory); the device classifies every draw against the problem's occupancy map (float64 arithmetic of
 * maze_env's cell lookup), finds the n_free-th free draw of every problem IN STREAM ORDER (problem b + 1 starts behind the last
 * draw problem b consumed, like the reference's one global generator), and writes the float32 node rows the graph builder and the
 * explorer read: per problem [init_state, goal_state, the n_free free draws, the first min(rejected, n_free) rejected draws]
 * (eval_gnn.py:182: collided[:len(free)]), compact, with node_ptr_out [B + 1].  v_out must hold n_problems * (2 + 2 * n_free) rows.
 * *cursor (device, in / out): index of the first unconsumed draw; used_out [B]: draws consumed per problem (the sampling's collision
 * checks, maze_env.py counts one per draw); *ok_out = 1, or 0 when the stream ran out before the last problem was complete (nothing
 * is consumed then: *cursor is unchanged -- append draws and call again).  One launch on hip_stream, no synchronisation. */
typedef struct {
    int32_t n_problems, width, n_free;
    int64_t n_attempts;
    const double* attempts;      /* [n_attempts, 2]  (gnnmp_stick_sample: 3 columns here ...) */
    const double* maps;          /* [B, width, width]                                         */
    const double* init_states;   /* [B, 2]           (... and in these two)                   */
    const double* goal_states;   /* [B, 2]                                                    */
} gnnmp_maze_sample_batch;
int gnnmp_maze_sample(const gnnmp_maze_sample_batch* batch, int64_t* cursor, float* v_out, int32_t* node_ptr_out,
                      int32_t* used_out, int32_t* ok_out, void* hip_stream);

/* The same for the 3-DoF stick robot, MazeEnv(dim=3).  The batch struct is gnnmp_maze_sample's with every row three wide:
 * attempts [n_attempts, 3] float64 is the host's np.random.uniform(-LIMITS, LIMITS, ...) stream with LIMITS = (1, 1, 0.4) in draw
 * order, init_states / goal_states are [B, 3], v_out rows are (x, y, z) float32 and v_out must hold n_problems * (2 + 2 * n_free)
 * of them.  A draw is free iff _stick_in_free_space holds for the float64 draw (maze_env.py:279-291), entirely in float64:
 * theta = z / 0.4 * pi, ends = centre -+ 0.1 * (cos theta, sin theta); end a is queried, then end b, then the midpoints of
 * _iterative_check_segment (maze_env.py:301-314: split while the end cells are more than one grid step apart and the ends more than
 * 0.05 apart in L1, left half before right half), stopping at the first blocked query.  An end outside [-1, 1]^2 fails without a
 * check; every in-bounds point query is one check, so a draw costs 0 .. 9 (a stick is 0.2 long: its bisection has at most three
 * levels, seven midpoints).  cos / sin are the device's float64 library functions: against numpy an outcome can differ only for a
 * stick end within an ulp of a cell boundary.
 * The contract is gnnmp_maze_sample's: problems are walked in stream order, *cursor (device, in / out) is the first unconsumed draw,
 * used_out [B] the draws consumed per problem, node_ptr_out [B + 1] the row offsets, *ok_out = 0 with *cursor unchanged (and
 * node_ptr_out[b + 1] = -1 for the problem the stream ended in) when the stream runs out.  Added: checks_out [B] (int64), the
 * collision checks of the draws problem b CONSUMED -- those up to and including its n_free-th free one -- which is what
 * MazeEnv.collision_check_count grows by during sample_n_points.  One launch on hip_stream, no synchronisation, no allocation. */
int gnnmp_stick_sample(const gnnmp_maze_sample_batch* batch, int64_t* cursor, float* v_out, int32_t* node_ptr_out,
                       int32_t* used_out, int64_t* checks_out, int32_t* ok_out, void* hip_stream);

/* ------------------------------------------------------------------------------------------
 * Resample rounds for a whole batch (the general loop of explore(), eval_gnn.py:191-247): every problem owns its sample
 * stream -- what np.random.seed(s_b) before explore() of problem b alone gives -- so a problem's result no longer depends on
 * the problems before it, and round r of all unfinished problems is one batch around gnnmp_maze_explore_ex:
 *   gnnmp_maze_sample_streams   sample_n_points + the two truncations of the collided list      eval_gnn.py:180, 241-245
 *   gnnmp_maze_rounds_gather    the round's node rows (create_data's v) and the carried trees    eval_gnn.py:150-158, 235-247
 *   gnnmp_maze_rounds_carry     the round's trees, pairs, paths and checks back into the store
 * The per-problem state lives in caller-allocated device arrays with one fixed-size slot per problem
 * (gnnmp_maze_rounds_state); `cap` = t_max rounded up to a multiple of the per-round sample count.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int32_t n_problems, cap, pair_cap;
    float* free_pool;            /* [B, cap + 2, dim]  rows 0 / 1 = init / goal state, then the free draws in draw order */
    float* coll_pool;            /* [B, cap + 2, dim]  the rejected draws the reference keeps                            */
    int32_t* n_free;             /* [B]  rows in use; 0 = nothing sampled yet                                           */
    int32_t* n_coll;             /* [B]                                                                                 */
    int32_t* tree_explored;      /* [B, cap + 2]  explored node ids in order (only free nodes are ever explored)         */
    int32_t* tree_prev;          /* [B, cap + 2]  parent by node id                                                      */
    int32_t* tree_n_explored;    /* [B]  a fresh tree is n_explored = 1, explored[0] = prev[0] = 0                       */
    int32_t* tree_pairs;         /* [B, pair_cap, 2]  the (a, b) pairs recorded so far; fresh = one pair [0, 0]          */
    int32_t* tree_n_pairs;       /* [B]                                                                                 */
    int32_t* tree_success;       /* [B]  success flag of the problem's last round                                       */
    int32_t* tree_path_len;      /* [B]                                                                                 */
    int32_t* tree_path;          /* [B, cap + 2]  node ids start -> goal of a solved problem                             */
    int64_t* tree_checks;        /* [B]  collision checks of the explore stage, summed over the rounds                   */
} gnnmp_maze_rounds_state;

/* Rejection sampling that APPENDS.  Problem b owns the draws [att_ptr[b], att_ptr[b + 1]) of attempts [n_attempts, dim]
 * (float64, the host's uniform(-LIMITS, LIMITS) values in draw order, as for gnnmp_maze_sample / gnnmp_stick_sample; dim 2 =
 * point robot, 3 = stick robot with gnnmp_stick_sample's classification and check counts).  One workgroup per problem, one
 * launch on hip_stream; no allocation, no synchronisation, no atomics on global memory, deterministic.
 * n_free[b] == 0 on entry (round 0): init / goal go to rows 0 / 1 of free_pool, the n_free free draws behind them, and the
 * first min(rejected, n_free) rejected draws are kept (eval_gnn.py:180: the cut happens before init / goal join).
 * Later rounds: n_free free draws are appended, and rejected draws are appended while n_coll[b] < the NEW n_free[b] (init /
 * goal counted: (collided + new)[:len(free)], eval_gnn.py:243-245 -- the cap goes n, 2n + 2, 3n + 2, ...; a round's own
 * rejected draws are not first cut to n).
 * used_out [B]: draws consumed; checks_out [B]: their collision checks (dim 2: = used); status_out [B]: 0 = done; 1 = the
 * problem's block ended before its n_free-th free draw: its pools and counts are untouched (used / checks 0) and the other
 * problems complete -- hand that problem a longer block and call again with the others masked out; 2 = n_free more rows
 * would not fit cap, or the block lies outside attempts: untouched as well.  active [B] (uint8) or NULL = all: a problem
 * with 0 is skipped entirely (none of its outputs is written).  att_ptr_host: optional host copy of att_ptr; when given it
 * is checked (ascending, inside [0, n_attempts]).
 * Returns GNNMP_ERR_DIMS for dim not 2 / 3, GNNMP_ERR_NULL for NULL pointers, GNNMP_ERR_ARG for n_problems / width / n_free
 * < 1, cap < n_free, n_attempts < 0 or a bad att_ptr_host; nothing is launched then.  What only the device can see (the
 * counts, att_ptr without a host copy) is guarded by the kernel itself: status 2, never a write outside a slot. */
typedef struct {
    int32_t n_problems, width, n_free, cap;
    int64_t n_attempts;
    const double* attempts;      /* [n_attempts, dim]                                          */
    const int64_t* att_ptr;      /* [B + 1]                                                    */
    const int64_t* att_ptr_host; /* [B + 1] on the HOST, or NULL                               */
    const double* maps;          /* [B, width, width]                                          */
    const double* init_states;   /* [B, dim]                                                   */
    const double* goal_states;   /* [B, dim]                                                   */
    const uint8_t* active;       /* [B] or NULL                                                */
} gnnmp_maze_streams_batch;
int gnnmp_maze_sample_streams(const gnnmp_maze_streams_batch* batch, int32_t dim, float* free_pool, int32_t* n_free,
                              float* coll_pool, int32_t* n_coll, int32_t* used_out, int64_t* checks_out, int32_t* status_out,
                              void* hip_stream);

/* The node rows of a round.  For the A = n_active problems with active[b] != 0 (NULL = all), in slot order: v_out = free rows
 * then collided rows, compact; node_ptr_out [A + 1]; n_free_out [A]; slot_out [A] = the slot of the round's j-th problem -- the
 * layout gnnmp_graph_build, gnnmp_batch and gnnmp_maze_explore_ex read.  The [A] / [A + 1] arrays are the caller's, sized from
 * n_active: should `active` hold more set entries than that, the slots beyond the first n_active are left out (nothing of
 * theirs is written anywhere); with fewer, the entries behind the last one keep what the caller put there.  The offsets depend on what the sampler just found,
 * so they are summed on the device (every workgroup adds up the counts of the active slots before its own); nothing is read
 * back.  v_rows: rows v_out can hold (a problem that would not fit is left out of v_out; its node_ptr entry is still
 * written).  resume_out (or NULL): device arrays the caller allocated -- n_explored [A], explored [v_rows], prev [v_rows],
 * n_pairs [A], pair_ptr [A + 1] (pair_ptr[j] = slot * pair_cap: the slots are not adjacent, so pair_ptr[A] = n_problems *
 * pair_cap only closes the array); `pairs` is ignored -- that receive the trees of the store at this round's offsets:
 * together with pairs = state->tree_pairs they ARE the gnnmp_maze_resume of the round's gnnmp_maze_explore_ex call (with the
 * fresh tree above in the store, round 0 runs in resume mode too and every round's explored_edges hold only its new
 * pairs).  One launch.  GNNMP_ERR_DIMS / GNNMP_ERR_NULL / GNNMP_ERR_ARG (n_problems < 1, cap < 1, pair_cap < 1 or
 * n_problems * pair_cap beyond 2^30, v_rows < 0, n_active outside [1, n_problems]). */
int gnnmp_maze_rounds_gather(const gnnmp_maze_rounds_state* state, int32_t dim, const uint8_t* active, int32_t n_active,
                             int64_t v_rows, float* v_out, int32_t* node_ptr_out, int32_t* n_free_out, int32_t* slot_out,
                             const gnnmp_maze_resume* resume_out_or_null, void* hip_stream);

/* After gnnmp_maze_explore_ex (resume mode, prev_out given) on the round's n_active problems: problem j's tree (explored
 * order; parents by node id -- free-node ids are stable across rounds, only node_ptr moves), path and flags replace those of
 * slot slot_of[j] (NULL = j), its checks are added, and its new pairs -- n_pairs[j] of them at int offset
 * 2 * (2 * edge_ptr[j] + j) of explored_edges -- are appended to the slot's pair list.  The next gnnmp_maze_rounds_gather
 * places the trees at the next round's offsets.
 * Capacity of the pair list: a step of the greedy loop picks a live cell (a, b) with a explored, b a free node not yet
 * explored, and whatever the outcome the unordered pair {a, b} is dead for the rest of the round; it records 2 pairs.  A
 * round on F free nodes with k1 neighbours has at most 2 * k1 * F unordered free-free edges (k1 per node from each of the two
 * kNN graphs), so pair_cap = 1 + sum over the rounds of 4 * k1_r * F_r always suffices: a derived bound, not the edge
 * counts.  status_out [n_active]: bit 0 = the new pairs did not fit pair_cap (none appended: the caller raises), bit 1 = a
 * node id or count beyond cap + 2 (skipped).  Nothing is ever written outside the slot.  One wave per problem, one launch. */
int gnnmp_maze_rounds_carry(const gnnmp_maze_rounds_state* state, int32_t n_active, const int32_t* slot_of,
                            const int32_t* node_ptr, const int32_t* edge_ptr, const int32_t* success,
                            const int32_t* n_explored, const int32_t* explored, const int32_t* prev, const int32_t* n_pairs,
                            const int32_t* explored_edges, const int32_t* path_len, const int32_t* path, const int64_t* checks,
                            int32_t* status_out, void* hip_stream);

/* ------------------------------------------------------------------------------------------
 * The per-problem sample streams themselves, drawn on the device: numpy's legacy generator (np.random.RandomState = MT19937),
 * bit for bit.  Problem b of the streams planner draws what np.random.seed(s_b) followed by the reference's one-by-one
 * uniform_sample calls gives (eval_gnn.py:180, 241-245 through environment/maze_env.py uniform_sample =
 * np.random.uniform(-LIMITS, LIMITS)); with one generator per problem those are B independent recurrences, so they can be
 * produced where gnnmp_maze_sample_streams reads them.
 * A stream's state is 625 words: uint32 key[624] followed by int32 pos -- RandomState.get_state()[1:3], so a state can be
 * compared with numpy's or taken from it (any pos in [0, 624], odd ones included).  The twist is numpy's LAZY one: a block
 * of 624 words is regenerated when a word is needed and pos == 624, so a stream that consumed exactly to the end of a block
 * keeps pos = 624 and the old key.
 * ---------------------------------------------------------------------------------------- */
/* np.random.RandomState(seeds[i]) for i < n_streams: init_genrand (key[0] = seed, key[j] = 1812433253 * (key[j-1] ^
 * (key[j-1] >> 30)) + j, pos = 624) into state [n_streams, 625].  One launch.  GNNMP_ERR_NULL / GNNMP_ERR_ARG (n_streams < 1). */
int gnnmp_mt19937_seed(int32_t n_streams, const uint32_t* seeds, uint32_t* state, void* hip_stream);

/* RandomState.uniform(low, high, (counts[b], dim)) of every stream: each double takes two consecutive tempered words a, b --
 * d = ((a >> 5) * 67108864.0 + (b >> 6)) / 9007199254740992.0 -- and element (r, c), in C order, is low[c] + range[c] * d with
 * range = high - low taken by the caller in double (numpy's uniform with array bounds); two rounded operations, never fused.
 * Three modes:
 *   out, commit = 0    fill: counts[b] rows at row out_ptr[b] of out [out_rows, dim]; the stored state is left alone, so the
 *                      same state can be filled from again (with a longer count);
 *   out, commit = 1    fill and store the advanced state;
 *   out NULL, commit   advance: skip counts[b] rows (counts is int32 so that gnnmp_maze_sample_streams' used_out can be
 *                      passed as it is; out_ptr is not read).
 * status_out [n_streams]: 0 = done; 2 = a negative count, a block [out_ptr[b], out_ptr[b] + counts[b]) outside
 * [0, out_rows], or a pos outside [0, 624]: neither the stream's state nor out is touched and the other streams complete.
 * active [n_streams] (uint8) or NULL = all: a stream with 0 is skipped entirely (its status word included).  out_ptr is
 * int64 [n_streams + 1] like gnnmp_maze_streams_batch's att_ptr, which can be passed here.  One workgroup per stream, one
 * launch on hip_stream; no allocation, no synchronisation, no atomics, deterministic.
 * Returns, before any launch: GNNMP_ERR_NULL (batch, counts, state, status_out, or out given without out_ptr),
 * GNNMP_ERR_DIMS (dim outside 1..3), GNNMP_ERR_ARG (n_streams < 1, out_rows < 0, a bound of a used column not finite, or
 * neither out nor commit). */
typedef double gnnmp_mt_bounds[3];
typedef struct {
    int32_t n_streams, dim;
    int64_t out_rows;
    const int32_t* counts;       /* [n_streams]                                                */
    const int64_t* out_ptr;      /* [n_streams + 1], or NULL when out is NULL                  */
    const uint8_t* active;       /* [n_streams] or NULL                                        */
    gnnmp_mt_bounds low, range;  /* by value; entries behind dim are ignored                   */
} gnnmp_mt_uniform_batch;
int gnnmp_mt19937_uniform(const gnnmp_mt_uniform_batch* batch, uint32_t* state, double* out_or_null, int32_t commit,
                          int32_t* status_out, void* hip_stream);

/* ------------------------------------------------------------------------------------------
 * The LazySP baseline on maze problems (algorithm/lazy_sp.py:147-196 over algorithm/dijkstra.py:34-76), batched, every
 * problem on its own sample stream: problem b computes what np.random.seed(s_b); LazySP(env, batch_size, T, k).plan() of that
 * problem alone computes (eval_bit.eval_lazysp's one global stream over consecutive problems is NOT reproduced).  The host
 * loops over rounds only; round r of all unfinished problems is
 *   gnnmp_lazysp_sample    informed_sample: `batch` more free draws into a float64 pool          lazy_sp.py:78-103, 154
 *   gnnmp_lazysp_gather    the round's float32 node rows, node_ptr, n_free, k1                   lazy_sp.py:125-126, 159
 *   gnnmp_graph_build      coalesce(knn_graph(float32 points, k1, loop=True) + flipped)         lazy_sp.py:126-128
 *   gnnmp_lazysp_round     Dijkstra / walk / check / invalidate until the round ends            lazy_sp.py:162-193
 * Node 0 is the GOAL and node 1 the START (lazy_sp.py:61).  The per-problem state lives in caller-allocated device arrays,
 * one fixed-size slot per problem; a fresh store is all zeros.  `cap` >= the free draws a problem can ever hold.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int32_t n_problems, cap, pair_cap;
    double* pool;                /* [B, cap + 2, dim]  row 0 = goal state, row 1 = init state, then the free draws in draw order */
    int32_t* n_nodes;            /* [B]  rows in use; 0 = nothing sampled yet                                              */
    int32_t* pairs;              /* [B, pair_cap, 2]  every edge (n1, n2) the planner checked, in the order it checked them  */
    uint8_t* pair_state;         /* [B, pair_cap]  1 = free (valid_edges), 2 = blocked (invalid_edges); the 2s in list order
                                  * are the order in which edges were invalidated                                           */
    int32_t* n_pairs;            /* [B]                                                                                    */
    int64_t* checks;             /* [B]  collision checks so far, sampling included                                        */
    int32_t* dijkstra_runs;      /* [B]  dijkstra() calls so far                                                           */
    int32_t* path_len;           /* [B]  nodes of the solution path, 0 = none                                              */
    int32_t* path;               /* [B, cap + 2]  node ids start -> goal (1 ... 0); scratch while a problem is unsolved     */
    int32_t* solved;             /* [B]  1 = a fully valid path was found                                                  */
    int32_t* status;             /* [B]  sticky bits: 1 = the pair list was full, 2 = a loop bound was hit, 4 = bad graph   */
} gnnmp_lazysp_state;

/* Pairs a problem's list can reach: every checked pair is an unordered non-loop edge of SOME round's graph and is checked at
 * most once, and round r's graph (k1_r nearest + reversed on N_r = 2 + r * batch nodes) has at most min(k1_r * N_r,
 * N_r (N_r - 1) / 2) of them; k1 = k1_by_round[r - 1] for r = 1 .. n_rounds (host array: the caller's ceil(k ln N / ln 100)).
 * GNNMP_ERR_NULL / GNNMP_ERR_ARG (batch < 1, n_rounds < 1, a k1 < 1, or a sum beyond 2^30). */
int gnnmp_lazysp_pair_cap(int32_t batch, int32_t n_rounds, const int32_t* k1_by_round, int64_t* pair_cap);

/* Rejection sampling that APPENDS `batch->n_free` free draws to every active problem's float64 pool.  The batch struct and its
 * att_ptr convention are gnnmp_maze_sample_streams' (problem b owns attempts [att_ptr[b], att_ptr[b + 1]), float64
 * [n_attempts, dim], host-drawn or filled by gnnmp_mt19937_uniform; active; att_ptr_host checked when given; batch->cap is not
 * read, the store's is).  A draw is free iff _state_fp holds for the float64 draw: dim 2 one point query (one check), dim 3
 * the stick with gnnmp_stick_sample's classification and 0 .. 9 checks; rejected draws are dropped.  n_nodes[b] == 0 on entry:
 * goal / init state go to rows 0 / 1 first.  state->checks[b] is INCREMENTED by the checks of the draws consumed (those up to
 * and including the n_free-th free one).  used_out / checks_out / status_out [B] as gnnmp_maze_sample_streams: status 0 =
 * done; 1 = the block ended before the n_free-th free draw, pool and counts untouched, used / checks 0: hand that problem a
 * longer block; 2 = no room in the pool (n_nodes + n_free > cap + 2) or the block lies outside attempts: untouched.  One wave
 * per problem, one launch on hip_stream; no allocation, no synchronisation, no atomics, deterministic.
 * GNNMP_ERR_DIMS (dim not 2 / 3), GNNMP_ERR_NULL, GNNMP_ERR_ARG (n_problems / width / n_free < 1, n_problems differing from
 * the store's, cap < n_free, n_attempts < 0, a bad att_ptr_host); nothing is launched then. */
int gnnmp_lazysp_sample(const gnnmp_maze_streams_batch* batch, int32_t dim, const gnnmp_lazysp_state* state, int32_t* used_out,
                        int64_t* checks_out, int32_t* status_out, void* hip_stream);

/* The node rows of a round for the n_active problems slot_of[0 .. n_active) (device, distinct slots): v_out = float32 of the
 * pool rows, compact, in slot_of order; node_ptr_out [A + 1]; n_free_out [A] = the node counts (every LazySP node is free, so
 * gnnmp_graph_build's second kNN pass repeats the first); k1_out [A] = k1_table[node count], k1_table [cap + 3] (device) being
 * the caller's ceil(k ln N / ln 100) by node count -- the layout gnnmp_graph_build reads.  The offsets are summed on the
 * device; nothing is read back.  A problem that would not fit v_rows is left out of v_out (its node_ptr entry is still
 * written); a slot outside the store counts as empty.  One launch.  GNNMP_ERR_DIMS / GNNMP_ERR_NULL / GNNMP_ERR_ARG
 * (n_active outside [1, n_problems], v_rows < 0, cap < 1). */
int gnnmp_lazysp_gather(const gnnmp_lazysp_state* state, int32_t dim, int32_t n_active, const int32_t* slot_of,
                        const int32_t* k1_table, int64_t v_rows, float* v_out, int32_t* node_ptr_out, int32_t* n_free_out,
                        int32_t* k1_out, void* hip_stream);

/* Workspace of gnnmp_lazysp_round (256-byte aligned): per edge a float64 cost and a flag, per problem the node state used
 * beyond the LDS node count.  GNNMP_ERR_NULL / GNNMP_ERR_ARG (n_active < 1, cap < 1, total_edges < 0). */
int gnnmp_lazysp_workspace_bytes(int32_t n_active, int32_t cap, int64_t total_edges, size_t* bytes);
/* Problems up to this many nodes keep dist / prev / block starts in LDS; larger ones use the workspace. */
int gnnmp_lazysp_lds_nodes(void);

/* One round of LazySP for the n_active problems slot_of[j] (NULL = j), each independent, one wave per problem, one launch.
 * edge_index [2, total_edges] (row stride total_edges) / edge_ptr [A + 1]: the round's coalesced graphs as gnnmp_graph_build
 * wrote them (columns of problem j sorted by (source, target), symmetric, graph-local ids); maps [B, width, width] BY SLOT.
 *   - carried pairs are looked up in the new graph: both directions of an invalid pair are dead (out of both neighbour
 *     lists), those of a valid pair need no check; a pair that is no longer an edge marks nothing and stays in the list;
 *   - edge cost = np.linalg.norm(points[t] - points[s]) on the float64 pool rows (numpy's fused dot for dim 2 / 3);
 *   - repeat: dijkstra from node 0 (least distance, lowest id among equals, strict improvement; stopped when node 1 is
 *     extracted, which cannot change dist[1] or its prev chain); dist[1] infinite ends the round; else the path is walked from
 *     node 1 along prev and its unknown edges are checked with _edge_fp on the float64 states -- in parallel, keeping only
 *     those up to and including the first blocked one in path order, so pairs, flags and the check count are the sequential
 *     loop's; a blocked edge is invalidated and dijkstra runs again; a fully valid path sets solved, path_len, path.
 * Updated in the store: pairs / pair_state / n_pairs (appended), checks and dijkstra_runs (incremented), path, path_len,
 * solved, status.  A slot with solved or status already set is skipped.  status bit 1: the pair list was full (the pairs of
 * that pass are not written: nothing is ever written outside the slot); bit 2: more dijkstra runs than E / 2 + 1, more
 * extractions than nodes, or a walk longer than the node count; bit 4: node count outside [2, cap + 2], an edge block outside
 * edge_index or a node id outside the graph.  Any bit ends the problem.
 * GNNMP_ERR_DIMS / GNNMP_ERR_NULL / GNNMP_ERR_ARG (n_active outside [1, n_problems], width < 1, total_edges < 0) /
 * GNNMP_ERR_WORKSPACE (workspace too small); nothing is launched then. */
int gnnmp_lazysp_round(const gnnmp_lazysp_state* state, int32_t dim, int32_t n_active, const int32_t* slot_of,
                       const int64_t* edge_index, int64_t total_edges, const int32_t* edge_ptr, const double* maps, int32_t width,
                       void* workspace, size_t workspace_bytes, void* hip_stream);

/* ------------------------------------------------------------------------------------------
 * The RRT* baseline on maze problems -- eval_rrt.py's NEXT_plan(env, model=None, T=t_max, g_explore_eps=1., stop_when_success)
 * (algorithm/tsa.py:12-139, 222-281 over algorithm/search_tree.py:5-98 and environment/maze_env.py:127-208, 266-347): a
 * goal-biased RRT with RRT*-style rewiring of the newest node -- batched, every problem on its own sample stream: problem b
 * computes what np.random.seed(s_b); env.init_new_problem(i_b); NEXT_plan(...) of that problem alone computes (eval_rrt's one
 * global stream over consecutive problems is NOT reproduced).  The whole t_max loop of all problems is ONE launch, one wave
 * per problem; per iteration: the sample (1 or 2 + dim raw doubles), the nearest non-terminal node (lowest index among
 * equals), RRT_steer, env.step with every collision check counted (the goal test of a free edge included), the insertion --
 * EVERY new state joins the tree, collided ones too -- and RRTS_rewire_last's two passes.  All decisions are float64, one
 * rounded operation at a time.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int32_t n_problems, dim, width;      /* dim 2 = point robot, 3 = stick robot; maps are width x width              */
    int32_t t_max, stop_when_success;    /* NEXT_plan's T; non-zero: the loop ends with the first node in the goal region */
    int64_t draws_per_problem;           /* doubles in a problem's block; t_max * (2 + dim) always suffices             */
    const double* maps;                  /* [B, width, width]  0 = free                                                 */
    const double* init_states;           /* [B, dim]                                                                    */
    const double* goal_states;           /* [B, dim]                                                                    */
    const double* draws;                 /* [B, draws_per_problem]  the RAW doubles of [0, 1) of the problem's generator
                                          * (RandomState.random_sample; gnnmp_mt19937_uniform with dim 1, low 0, range 1), in
                                          * draw order: an iteration takes one (rand() < 0.05: the sample is the goal state)
                                          * or 2 + dim (a second rand() that is dropped, then low + (high - low) * d per
                                          * coordinate, the transform applied here)                                     */
} gnnmp_rrtstar_batch;

typedef struct {                         /* all out; rows of a problem behind its n_nodes are left as they were         */
    double* states;                      /* [B, t_max + 1, dim]  row 0 = init state, row i + 1 = the new state of iteration i */
    int32_t* parents;                    /* [B, t_max + 1]  the node a state was grown from; -1 for the root             */
    int32_t* rewired_parents;            /* [B, t_max + 1]  after rewiring                                               */
    uint8_t* flags;                      /* [B, t_max + 1]  bit 0 = freesp, bit 1 = in_goal_region                        */
    double* costs;                       /* [B, t_max + 1]  2 for collided nodes                                         */
    double* path_lengths;                /* [B, t_max + 1]  -1 until a node reaches the goal region                       */
    int64_t* cumulated_checks;           /* [B, t_max + 1]  collision checks after every iteration; 0 for the root        */
    int32_t* path;                       /* [B, t_max + 1]  search_tree.path(): node ids root -> last node along
                                          * rewired_parents; path_len entries, 0 unless the last node is in the goal region */
    int32_t* n_nodes;                    /* [B]  iterations run + 1                                                      */
    int32_t* success;                    /* [B]  1 = some first step of an iteration ended in the goal region            */
    int32_t* last_iter;                  /* [B]  NEXT_plan's returned i: index of the last iteration run                  */
    int32_t* used;                       /* [B]  doubles consumed from the block                                         */
    int32_t* path_len;                   /* [B]                                                                          */
    int32_t* status;                     /* [B]  0, or bits: 1 = the draw block ended before an iteration had its doubles
                                          * (the tree holds the iterations before it; nothing is read beyond the block),
                                          * 2 = rewired_parents hold a cycle (the reference would not return): no path     */
} gnnmp_rrtstar_tree;

/* Workspace of gnnmp_rrtstar_plan (256-byte aligned): node coordinates, cost and flags (8 dim + 9 bytes a node, sized for
 * dim 3) of every problem when t_max + 1 exceeds gnnmp_rrtstar_lds_nodes(), else 0 bytes (the node state lives in LDS and
 * workspace may be NULL).  GNNMP_ERR_NULL / GNNMP_ERR_ARG (n_problems < 1, t_max < 1). */
int gnnmp_rrtstar_workspace_bytes(int32_t n_problems, int32_t t_max, size_t* bytes);
/* Trees of up to this many nodes (t_max + 1) keep their node state in LDS; longer runs use the workspace. */
int gnnmp_rrtstar_lds_nodes(void);

/* RRT* for batch->n_problems maze problems, one launch on hip_stream: no allocation, no synchronisation, no atomics,
 * deterministic.  Semantics as restated above and in gnnmp.rrtstar.plan_host; in particular
 *   - distance = sqrt((dx^2 + dy^2) + dz^2), dz = min(|dz|, ||dz| - 0.8|) for the stick;
 *   - env.step(a, new): x, y clipped to +-1, z wrapped, _edge_fp(a, new) -- both _valid_state, both counted _state_fp in that
 *     order, then the bisection (point) or the K = int(d / 0.015) interpolated sticks (stick) -- and ONLY for a free edge the
 *     goal test, which counts one more _state_fp(new) when new is within RRT_EPS of the goal;
 *   - rewiring, newest node free: near = distance < 3 RRT_EPS over ALL earlier nodes; pass 1 in index order over the free near
 *     nodes, a candidate checked (env.step(node, new)) only if dist + cost beats the RUNNING minimum; pass 2 over all near
 *     nodes, collided ones (cost 2) included: checked if min_cost + dist < cost, a free edge sets the node's cost and rewired
 *     parent, descendants keep their costs;
 *   - success comes from the first step of an iteration only; path_lengths[-1] changes only when the newest node is in the
 *     goal region.
 * All argument errors come back before anything is launched: GNNMP_ERR_NULL (a NULL struct or array; workspace when
 * gnnmp_rrtstar_workspace_bytes is not 0), GNNMP_ERR_DIMS (dim not 2 / 3), GNNMP_ERR_ARG (n_problems / width / t_max < 1,
 * draws_per_problem < 2 + dim -- shorter than one iteration -- or beyond 2^31 - 1), GNNMP_ERR_WORKSPACE (too small or
 * misaligned). */
int gnnmp_rrtstar_plan(const gnnmp_rrtstar_batch* batch, const gnnmp_rrtstar_tree* tree, void* workspace, size_t workspace_bytes,
                       void* hip_stream);

/* ------------------------------------------------------------------------------------------
 * The BIT* baseline on maze problems -- eval_bit.eval_bit's BITStar(env, batch_size, T, sampling=None).plan(INF,
 * time_budget=300, refine_time_budget=0) and get_best_path() (algorithm/bit_star.py:18-334 over
 * environment/maze_env.py:236-347) -- batched, every problem on its own sample stream: problem b computes what
 * np.random.seed(s_b); env.init_new_problem(i_b); BITStar(...).plan(...) of that problem alone computes (eval_bit's one global
 * stream over consecutive problems is NOT reproduced).  Reproduced is the search for the FIRST solution: with
 * refine_time_budget = 0 the loop ends with the iteration that reaches the goal, c_best is infinite at every sampling call,
 * prune removes nothing; refinement and the wall-clock budgets are not.  Node 0 is the START, node 1 the GOAL, then the free
 * draws in order.  All decisions are float64, one rounded operation at a time; the radius comes from the host.
 *   gnnmp_bitstar_sample    the free draws of all n_batches batches, per batch the attempts and checks    bit_star.py:111-140
 *   gnnmp_bitstar_plan      the search                                                                    bit_star.py:212-334
 * ---------------------------------------------------------------------------------------- */
/* Sampling.  `batch` is a gnnmp_maze_streams_batch as gnnmp_maze_sample_streams reads it: n_free = free draws per BIT* batch,
 * cap = rows per problem of pool (>= 2 + n_batches * n_free), problem b's attempts (float64 [n_attempts, dim], the states
 * bounds[:, 0] + random(dim) * ranges in draw order) at [att_ptr[b], att_ptr[b + 1]).  One launch, one wave per active problem.
 * A draw is free iff _state_fp holds (counted).  pool [B, cap, dim]: row 0 the init state, row 1 the goal state, then the
 * n_batches * n_free free draws in order.  used_by_batch / checks_by_batch [B, n_batches]: attempts consumed and sampling
 * checks spent when batch k was complete (cumulative).  status_out [B]: 0; 1 = the block ended before the last batch was
 * complete -- pool and tables of that problem are untouched, hand it a longer block; 2 = the block lies outside attempts.
 * GNNMP_ERR_DIMS (dim not 2 / 3) / GNNMP_ERR_NULL / GNNMP_ERR_ARG (n_problems, width, n_free or n_batches < 1, cap too small,
 * n_attempts < 0, att_ptr_host not ascending inside [0, n_attempts]); nothing is launched then. */
int gnnmp_bitstar_sample(const gnnmp_maze_streams_batch* batch, int32_t dim, int32_t n_batches, double* pool,
                         int64_t* used_by_batch, int64_t* checks_by_batch, int32_t* status_out, void* hip_stream);

typedef struct {
    int32_t n_problems, dim, width;      /* dim 2 = point robot, 3 = stick robot; maps are width x width              */
    int32_t batch, n_batches;            /* free draws per batch; ceil(t_max / batch) batches at most                  */
    int32_t n_nodes;                     /* rows per problem of pool and of the per-node outputs, >= 2 + n_batches * batch */
    int32_t flags;                       /* bit 0: keep the node state in the outputs and the workspace whatever the node
                                          * count (the path of problems beyond gnnmp_bitstar_lds_nodes(); same results);
                                          * other bits must be 0                                                       */
    int64_t edge_cap;                    /* entries of a problem's edge queue, 1 .. n_nodes * (n_nodes - 1)             */
    const double* maps;                  /* [B, width, width]  0 = free                                                 */
    const double* pool;                  /* [B, n_nodes, dim]  gnnmp_bitstar_sample's                                   */
    const double* r_by_batch;            /* [B, n_batches]  the radius after batch k: radius_init() * (log(q) / q) ** (1 / dim)
                                          * with the reference's own expressions, computed by the host                  */
    const int64_t* checks_by_batch;      /* [B, n_batches]  gnnmp_bitstar_sample's                                      */
} gnnmp_bitstar_batch;

typedef struct {                         /* all out                                                                     */
    double* g;                           /* [B, n_nodes]  g_scores by node id, inf off the tree                         */
    int32_t* parents;                    /* [B, n_nodes]  edges[x] by node id, -1 = none                                */
    int32_t* vertices;                   /* [B, n_nodes]  node ids in the order they joined the tree; n_vertices entries, -1 behind */
    int32_t* path;                       /* [B, n_nodes]  get_best_path(): node ids start -> goal; path_len entries      */
    int32_t* n_vertices;                 /* [B]                                                                         */
    int32_t* batches_run;                /* [B]  batches drawn: T = batches_run * batch                                 */
    int32_t* success;                    /* [B]  1 = g_scores[goal] is finite                                           */
    int32_t* path_len;                   /* [B]                                                                         */
    int32_t* status;                     /* [B]  0, or bits: 1 = the edge queue was full (run the problem again with a larger
                                          * edge_cap), 2 = a loop bound was hit or the parents hold a cycle, 4 = a radius that
                                          * is not positive or a negative check count (tables not filled).  Any bit ends the
                                          * problem; the other problems of the batch are not affected                  */
    int64_t* counters;                   /* [B, 8]  collision checks (sampling of the batches drawn + edges),
                                          * vertex_expansions, edge_pops, edge_checks, rewired, filtered, max_edge_queue,
                                          * ties_at_pop                                                                 */
} gnnmp_bitstar_result;

/* Workspace of gnnmp_bitstar_plan (256-byte aligned): per problem the edge queue (16 bytes an entry) and per node the queued
 * value and a flag byte (the per-node part is sized at every node count).  GNNMP_ERR_NULL / GNNMP_ERR_ARG (n_problems < 1, n_nodes < 3, edge_cap outside
 * [1, n_nodes * (n_nodes - 1)]). */
int gnnmp_bitstar_workspace_bytes(int32_t n_problems, int32_t n_nodes, int64_t edge_cap, size_t* bytes);
/* Launches of up to this many nodes per problem (2 + n_batches * batch) keep their node state in LDS; larger ones, and those
 * with bit 0 of flags set, use the outputs and the workspace. */
int gnnmp_bitstar_lds_nodes(void);

/* BIT* for batch->n_problems maze problems, one launch on hip_stream, one wave per problem: no allocation, no
 * synchronisation, no atomics, deterministic.  Semantics as restated above and in gnnmp.bitstar.plan_host; in particular
 *   - a batch is drawn only when both queues are empty; the loop test T < t_max stands at the top of every iteration, so the
 *     iteration that draws the last batch still pops one edge;
 *   - both queues pop in heapq's tuple order: value, then the source point's coordinates, then the target point's;
 *   - distance = np.linalg.norm(a - b) in all dim coordinates (left-to-right fused dot product), no wrap of the angle;
 *   - an accepted edge removes every queued edge with the same target; descendants keep their costs.
 * All argument errors come back before anything is launched: GNNMP_ERR_NULL (a NULL struct, array or workspace),
 * GNNMP_ERR_DIMS (dim not 2 / 3), GNNMP_ERR_ARG (n_problems / width / batch / n_batches < 1, n_nodes < 2 + n_batches * batch,
 * edge_cap outside [1, n_nodes * (n_nodes - 1)], flags beyond bit 0), GNNMP_ERR_WORKSPACE (too small or misaligned). */
int gnnmp_bitstar_plan(const gnnmp_bitstar_batch* batch, const gnnmp_bitstar_result* result, void* workspace,
                       size_t workspace_bytes, void* hip_stream);

/* ------------------------------------------------------------------------------------------
 * The NEXT planning network on maze problems (ABI 8) -- the PPN of next_model/model2D.py:84-210 with env_width 15,
 * cap = g = 8, latent 64; dim 2 = point robot (next_2), 3 = stick robot (next_3).  Batched over problems and over states:
 *   gnnmp_next_pb_forward      pb_rep of B problems: the goal attention (1 x 1-conv MLP 4-16-16-32-32-64-1 over the 225 cells,
 *                              softmax over cells, times softmax(dim-64-8 MLP)), hidden (3 x 3, 9 -> 64), h0 / c0 (3 x 3, 64 -> 64)
 *                              and `iters` rounds of { conv 3 x 3 64 -> 64 on h; LSTMCell(64, 64) per cell }, in exact fp32 MFMA
 *   gnnmp_next_state_forward   y = [action mean, value] of S states, each read out of its problem's pb_rep through the state
 *                              attention, the sum over cells and cap (accumulated in double) and the policy MLP 8-128-64-(dim+1)
 * The last coordinate of every goal and state is divided by 0.4 (LIMITS[2]) in float32 first; for dim 2 that is y, and the 2-D
 * attention sees the divided y.  Cell (row i, column j) enters the attention as [s0, s1, j, i].  Both calls run on hip_stream
 * and do not synchronise or allocate; results are bit-identical from run to run.
 *
 * Packed weights (gnnmp_next_weights_floats floats, the same count for both dim; gnnmp.next_model.pack_weights writes them):
 * the attention's six shared layers as [out][in] weight then bias (the last bias padded to 4 floats), its dim-64-8 MLP (first
 * layer [64][3], column 2 zero for dim 2), the policy MLP (last layer padded to [4][64] + 4), then hidden / h0 / c0 / conv as
 * [9 taps x (cin padded to 16s) / 16][4 column tiles][64 lanes][4 steps] + 64 biases and the LSTM as [8][16][64][4] over
 * K = [input 64 | hidden 64], N = the 256 gate rows, + 256 summed biases: element (k group, tile, lane, step) is
 * weight[k = 16 group + 4 (lane / 16) + step][n = 16 tile + lane % 16].
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int32_t n_problems, dim, width;      /* B >= 0 (0: nothing is done); dim 2 / 3; width must be 15                      */
    int32_t iters;                       /* LSTM rounds >= 0; the reference runs 20; 0 returns h0                         */
    const float* maps;                   /* [B, 15, 15]  0 = free                                                          */
    const float* goals;                  /* [B, dim]                                                                       */
    const float* weights;                /* packed, see above                                                              */
    float* pb_rep;                       /* out [B, 64, 15, 15]: pb_forward(...) viewed as [B, g * cap, H, W], c = 8 g + cap */
} gnnmp_next_pb;

typedef struct {
    int32_t n_states, n_problems, dim, width;   /* S >= 0 (0: nothing is done), B >= 0, dim 2 / 3, width must be 15        */
    const float* states;                 /* [S, dim]                                                                       */
    const int32_t* problem_of_state;     /* [S]  any order, repeats allowed                                                */
    const float* pb_rep;                 /* [B, 64, 15, 15]                                                                */
    const float* weights;                /* packed, see above                                                              */
    float* y;                            /* out [S, dim + 1]: the action mean, then the value                              */
    int32_t* status;                     /* [2] device-writable, ACCUMULATED (zero it first): [0] += states whose
                                          * problem_of_state is outside [0, B) -- such a row reads no pb_rep, is not clamped and
                                          * gets NaN in y; the other rows are unaffected -- [1] = max(last such row + 1)       */
} gnnmp_next_states;

/* GNNMP_ERR_NULL (n_floats), GNNMP_ERR_DIMS (dim not 2 / 3). */
int gnnmp_next_weights_floats(int32_t dim, size_t* n_floats);
/* All argument errors come back before anything is launched, in this order: GNNMP_ERR_NULL (the struct), GNNMP_ERR_DIMS (dim not
 * 2 / 3, width not 15), GNNMP_ERR_ARG (n_problems / n_states < 0, iters < 0), GNNMP_ERR_NULL (an array). */
int gnnmp_next_pb_forward(const gnnmp_next_pb* desc, void* hip_stream);
int gnnmp_next_state_forward(const gnnmp_next_states* desc, void* hip_stream);

/* ------------------------------------------------------------------------------------------
 * Training the NEXT planning network on maze problems (additive to ABI 9; next_train_kernels.hip) -- the forward that keeps its
 * activations and the backward, for dim 2 / 3, width 15.
 *   gnnmp_next_train_forward   what gnnmp_next_pb_forward followed by gnnmp_next_state_forward computes, with the same bits in
 *                              pb_rep and y, and into the workspace x9, the hidden layer, every round's h and c going in and the
 *                              conv output (about 3.6 MB a problem at 20 rounds).
 *   gnnmp_next_state_backward  dy [S, dim + 1] -> dpb_rep [B, 64, 15, 15] and dweights[0, per-state range): the shared attention
 *                              MLP, mlp.0, mlp.2 and the policy MLP, summed over the states in ascending state index in double.
 *   gnnmp_next_pb_backward     dpb_rep -> dweights of hidden, h0, c0, conv and lstm, summed over the problems in ascending
 *                              problem index in double.  The gradient also reaches the goal attention through x9: this call
 *                              REWRITES the attention range of dweights (the six shared layers, mlp.0, mlp.2) as float(the state
 *                              call's double sum, kept in the workspace, + the goals' sum in ascending problem index).  So it
 *                              runs after gnnmp_next_state_backward on the same struct and workspace; with n_states == 0 the
 *                              state sum counts as zero and the policy range is written as zero.
 * dweights is float32, gnnmp_next_weights_floats long, in the packed layout; padding lanes receive zero.  When there is work
 * (below) dweights and dpb_rep are overwritten, never accumulated into.  No floating-point atomics: two runs are bit-identical.
 * A problem_of_state outside [0, B) is counted in the forward's status words, its row of y is NaN, and nothing is read or
 * written for it in the forward or the backward.
 *
 * weights_t (gnnmp_next_weights_t_floats floats; gnnmp.next_train.pack_weights_t writes them): conv, h0 and c0 with flipped taps
 * and the channel matrix transposed, in the convolution packing above, the LSTM's [256 gate rows][x 64 | h 64] in the MFMA
 * packing, and 64 zeros.
 *
 * Checks, in this order, each before any HIP call: GNNMP_ERR_NULL (the struct), GNNMP_ERR_DIMS (dim not 2 / 3, width not 15),
 * GNNMP_ERR_ARG (a negative count), GNNMP_ERR_NULL (an array), then GNNMP_OK WITHOUT ANY HIP CALL AND WITHOUT WRITING ANYTHING
 * when there is no work -- n_problems == 0, and for gnnmp_next_state_backward n_states == 0 as well (gnnmp_next_train_forward
 * with n_states == 0 computes pb_rep only) -- then GNNMP_ERR_WORKSPACE (workspace_bytes below
 * gnnmp_next_train_workspace_bytes, or the workspace not 256-byte aligned).
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int32_t n_problems, n_states, dim, width, iters;
    const float* maps;                   /* [B, 15, 15]                                                                    */
    const float* goals;                  /* [B, dim]                                                                       */
    const float* states;                 /* [S, dim]                                                                       */
    const int32_t* problem_of_state;     /* [S]  any order, repeats allowed                                                */
    const float* weights;                /* packed, gnnmp_next_weights_floats floats                                       */
    float* pb_rep;                       /* out [B, 64, 15, 15]                                                            */
    float* y;                            /* out [S, dim + 1]                                                               */
    int32_t* status;                     /* [2] accumulated, as gnnmp_next_states.status                                   */
    void* workspace;                     /* device memory, 256-byte aligned; the backward reads it                         */
    size_t workspace_bytes;
} gnnmp_next_train;

typedef struct {
    int32_t n_problems, n_states, dim, width, iters;      /* as in the forward                                              */
    const float* goals;                  /* [B, dim]                                                                       */
    const float* states;                 /* [S, dim]                                                                       */
    const int32_t* problem_of_state;     /* [S]                                                                            */
    const float* weights;                /* packed                                                                         */
    const float* weights_t;              /* the transposed packing, see above                                              */
    const float* pb_rep;                 /* [B, 64, 15, 15]  the forward's                                                 */
    const float* dy;                     /* [S, dim + 1]                                                                   */
    float* dpb_rep;                      /* [B, 64, 15, 15]  out of the state call, in of the pb call                      */
    float* dweights;                     /* out, gnnmp_next_weights_floats floats                                          */
    void* workspace;                     /* the forward's                                                                  */
    size_t workspace_bytes;
} gnnmp_next_train_bwd;

/* GNNMP_ERR_NULL (bytes), GNNMP_ERR_ARG (a negative count).  A multiple of 256, strictly increasing in each argument. */
int gnnmp_next_train_workspace_bytes(int32_t n_problems, int32_t iters, int32_t n_states, size_t* bytes);
int gnnmp_next_weights_t_floats(int32_t dim, size_t* n_floats);
int gnnmp_next_train_forward(const gnnmp_next_train* desc, void* hip_stream);
int gnnmp_next_state_backward(const gnnmp_next_train_bwd* desc, void* hip_stream);
int gnnmp_next_pb_backward(const gnnmp_next_train_bwd* desc, void* hip_stream);

/* ------------------------------------------------------------------------------------------
 * The replay of NEXT's training loop on maze problems (additive to ABI 9; next_replay_kernels.hip) -- train_next.py:25-68,
 * 88-108: the (problem, path) samples train() draws from, with get_label's actions and values, kept on the device, and the loss
 * train() differentiates.
 *
 * The store is a struct of caller-owned device arrays; counts, status and path_ptr[0] start as zeros.  Path i is rows
 * path_ptr[i] : path_ptr[i + 1] of states64 / states32 / actions / values and belongs to problem[i].
 *   gnnmp_next_replay_append_trees   the path of every successful problem (success != 0 and path_len > 0) of one gnnmp_next_plan
 *                                    batch, in ascending batch position: rows states[b, path[b, j]], j < path_len[b] -- what
 *                                    search_tree.path()[0] returns.
 *   gnnmp_next_replay_append_paths   every packed path (BIT*'s get_best_path() rows, anything collected elsewhere), in order.
 * Both compute the slots and offsets with one exclusive scan (one wave, integers, no atomic ordering), then run get_label in
 * float64, one wave per path, rounding to float32 once: edge = np.linalg.norm(next - prev); the running cost ONE serial
 * left-to-right chain, value = cost - cost[last]; action = interpolate(prev, next, RRT_EPS / edge) - prev when edge > RRT_EPS
 * (the stick robot's interpolate wraps the orientation gap and the result by one period), else next - prev; zero for the last
 * state.  states32 is the float32 rounding of the rows, what Model2D.net_forward feeds the network.
 * An append is all or nothing: when the new paths or states would not fit (status bit 1), or the source is malformed (bit 2: a
 * path_len outside [0, t_max + 1]; path_ptr not from 0 to n_states or a path without a state; counts outside the capacities),
 * counts and every row in use stay as they are.  Bit 4: a node id outside [0, t_max] in an appended path; its row is zeros.
 * status is accumulated (OR), never cleared.  pending is the call's scratch: {first slot, first state, paths, states} of the
 * last append; problem[] of the new slots holds source indices between the call's two launches.
 *
 *   gnnmp_next_path_loss   for a group of G paths over y [S, dim + 1] (path g is rows ptr[g] : ptr[g + 1]):
 *                          terms[g] = {mean_s (values - y[:, dim])^2, mean_{s, j} (actions - y[:, :dim])^2} in double, one wave a
 *                          path and every sum one ascending chain; loss = (sum_g terms[g, 0] + terms[g, 1]) / divisor in
 *                          train()'s order; dy = d loss / d y in float32.  divisor is train()'s 8, whatever G is.  terms, loss
 *                          and dy are optional (NULL: not computed; loss needs terms).  A path outside [0, S) or without rows
 *                          gets NaN terms and touches no row; rows of dy outside every path are not written.
 * No floating-point atomics, no scratch, no allocation, no synchronisation: two runs give the same bits.
 *
 * Checks, in this order, each before any HIP call: GNNMP_ERR_NULL (a struct), GNNMP_ERR_DIMS (dim not 2 / 3), GNNMP_ERR_ARG (a
 * negative count or capacity, t_max + 1 beyond int32, divisor < 1), GNNMP_ERR_NULL (an array: the store's first, then the
 * source's; loss without terms), then GNNMP_OK WITHOUT ANY HIP CALL AND WITHOUT WRITING ANYTHING when there is no work --
 * n_problems == 0, n_paths == 0, or terms and dy both NULL.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int32_t dim, cap_paths, cap_states;
    double* states64;                    /* [cap_states, dim]                                                              */
    float* states32;                     /* [cap_states, dim]                                                              */
    float* actions;                      /* [cap_states, dim]                                                              */
    float* values;                       /* [cap_states]                                                                   */
    int32_t* path_ptr;                   /* [cap_paths + 1]                                                                */
    int32_t* problem;                    /* [cap_paths]                                                                    */
    int32_t* counts;                     /* [2]  paths and states in use                                                   */
    int32_t* status;                     /* [1]  bits 1 / 2 / 4, see above                                                 */
    int32_t* pending;                    /* [4]  scratch of an append call                                                 */
} gnnmp_next_replay;

typedef struct {
    int32_t n_problems, t_max;           /* the batch and T of the gnnmp_next_plan call                                    */
    const double* states;                /* [B, t_max + 1, dim]  gnnmp_next_plan_tree.states                               */
    const int32_t* path;                 /* [B, t_max + 1]       node ids, start first                                     */
    const int32_t* path_len;             /* [B]                                                                            */
    const int32_t* success;              /* [B]                                                                            */
    const int32_t* problem_ids;          /* [B]  what problem[] receives                                                   */
} gnnmp_next_replay_trees;

typedef struct {
    int32_t n_paths, n_states;
    const double* paths64;               /* [n_states, dim]                                                                */
    const int32_t* path_ptr;             /* [n_paths + 1]  from 0 to n_states, every path a state at least                 */
    const int32_t* problem_ids;          /* [n_paths]                                                                      */
} gnnmp_next_replay_paths;

typedef struct {
    int32_t n_paths, n_states, dim, divisor;
    const float* y;                      /* [S, dim + 1]                                                                   */
    const float* actions;                /* [S, dim]                                                                       */
    const float* values;                 /* [S]                                                                            */
    const int32_t* ptr;                  /* [G + 1]                                                                        */
    double* terms;                       /* out [G, 2], optional                                                           */
    double* loss;                        /* out [1], optional                                                              */
    float* dy;                           /* out [S, dim + 1], optional                                                     */
} gnnmp_next_path_loss_desc;

int gnnmp_next_replay_append_trees(const gnnmp_next_replay* store, const gnnmp_next_replay_trees* trees, void* hip_stream);
int gnnmp_next_replay_append_paths(const gnnmp_next_replay* store, const gnnmp_next_replay_paths* paths, void* hip_stream);
int gnnmp_next_path_loss(const gnnmp_next_path_loss_desc* desc, void* hip_stream);

/* ------------------------------------------------------------------------------------------
 * The replay of the smoother's training loop on maze problems (additive to ABI 9; smoother_replay_kernels.hip) --
 * train_smoother.py:20-61, 91-99: the (path, path_smooth, free, collided) samples train() draws from, kept on the device, the
 * gnnmp_smooth_batch of one optimizer step gathered from them, and the loss train() differentiates.  C = config_size, 2 .. 14.
 *
 * The store is a struct of caller-owned device arrays, all zero at first.  Sample i is rows path_ptr[i] : path_ptr[i + 1] of
 * path and target, free_ptr[i] : free_ptr[i + 1] of free_pts, coll_ptr[i] : coll_ptr[i + 1] of collided, and belongs to
 * problem[i].  counts holds TWO banks of {samples, path rows, free rows, collided rows}: a call reads bank (epoch & 1) and
 * writes bank ((epoch + 1) & 1), so the workgroups of one launch never read a word another one writes; the caller passes the
 * number of append calls it has made on the store so far as `epoch`.  INVARIANT: `epoch` counts every append call on these
 * arrays that got past the no-work return, whether it appended or not, for the store's whole life, and ONE owner keeps it; a
 * second owner of the same arrays (two wrappers over one allocation) would read the stale bank.  Nothing on the device detects
 * that: pending[0 .. 4) reports the counts the call started from, and a caller that mirrors the store compares them with its own
 * (the Python wrapper raises on a difference).
 *
 *   gnnmp_smooth_replay_append   ONE launch, one workgroup per source sample.  Every taken sample (take != 0), in ascending
 *       position, receives the next slot: its P path rows and P target rows, its first min(n_free, 500) sample rows as free
 *       rows and its first min(n_coll, 500) rows behind the free ones as collided rows, n_coll = (node_ptr[b + 1] -
 *       node_ptr[b]) - n_free; a side without rows receives ONE all-zero filler row (obs_data of train_smoother.py:20-30).
 *       Wave 0 of every workgroup runs the same exclusive scan over all B sources (integers, no atomics) and so knows its own
 *       slot and four row offsets and whether the call fits; workgroup 0 alone writes the prefix arrays, problem[], pending[],
 *       status and the other counts bank.  All or nothing: when a capacity would be exceeded (status bit 1) or the source is
 *       malformed (bit 2: a taken sample with P <= 2, rows outside [0, total_path) / [0, total_nodes), n_free outside its node
 *       rows, more taken samples than take_upper, counts outside the capacities) no row and no prefix entry is written and the
 *       new bank repeats the old counts.  pending = {samples, path rows, free rows, collided rows before the call; the four
 *       numbers the call added}.  status is accumulated (OR) and cleared by the caller.
 *   gnnmp_smooth_replay_gather   ONE launch, one workgroup per group entry: the gnnmp_smooth_batch of samples idx[0 .. G) in
 *       that order (repeats allowed): path, free_pts and collided rows, `target` rows aligned with path, edge_index
 *       [2, sum (3 P - 2)] in chain_edge_index's order (i + 1 -> i for i < P - 1, then i -> i + 1, then the P self loops;
 *       path-local ids) and the four prefix arrays [G + 1].  The totals of `out` are the caller's (it mirrors the store's
 *       prefix arrays); when an index lies outside [0, n_samples) or the totals the kernel finds differ from out's, NOTHING is
 *       written but status bit 4.  The arrays `out` points to are written although the struct declares them const.
 *   gnnmp_smooth_path_loss       ONE launch, one workgroup, one wave per path (8 waves take the paths in turn): for path g of
 *       P = path_ptr[g + 1] - path_ptr[g] rows, terms[g] = sum over the interior rows 1 .. P - 2 and the C columns of
 *       (pred - target)^2, ONE ascending chain in double in (row, column) order, / ((P - 2) C) -- MSELoss(target[1:-1],
 *       pred[1:-1]); loss = (sum_g terms[g], ascending g, one lane) / divisor rounded to float32 once; d_pred = 2 (pred -
 *       target) / ((P - 2) C divisor) evaluated in double and rounded once on interior rows, exactly 0 on every other row of
 *       the path.  P <= 2 (or path_ptr outside [0, total_rows]): terms[g] = 0 and, for a path inside the rows, zero rows.
 * No floating-point atomics, no scratch, no allocation, no synchronisation: two runs give the same bits.
 *
 * Checks, in this order, each before any HIP call: GNNMP_ERR_NULL (a struct), GNNMP_ERR_DIMS (config_size outside 2 .. 14),
 * GNNMP_ERR_ARG (a negative count, capacity, total or epoch; take_upper > n_samples; divisor < 1), GNNMP_ERR_NULL (an array:
 * the store's first, then the call's own), then GNNMP_OK WITHOUT ANY HIP CALL AND WITHOUT WRITING ANYTHING when there is no
 * work: n_samples == 0 or take_upper == 0 (append), n_group == 0 (gather), n_paths == 0 (path loss).
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int32_t config_size, cap_samples, cap_path_rows, cap_free_rows, cap_coll_rows, epoch;
    float* path;                         /* [cap_path_rows, C]                                                             */
    float* target;                       /* [cap_path_rows, C]                                                             */
    float* free_pts;                     /* [cap_free_rows, C]                                                             */
    float* collided;                     /* [cap_coll_rows, C]                                                             */
    int32_t* path_ptr;                   /* [cap_samples + 1]                                                              */
    int32_t* free_ptr;                   /* [cap_samples + 1]                                                              */
    int32_t* coll_ptr;                   /* [cap_samples + 1]                                                              */
    int32_t* problem;                    /* [cap_samples]                                                                  */
    int32_t* counts;                     /* [2, 4]  two banks, see above                                                   */
    int32_t* status;                     /* [1]  bits 1 / 2 / 4, see above                                                 */
    int32_t* pending;                    /* [8]  the last append call                                                      */
} gnnmp_smooth_replay;

typedef struct {
    int32_t n_samples, total_path, total_nodes;
    int32_t take_upper;                  /* an upper bound of the set take flags (n_samples when unknown); 0: no work      */
    const float* path;                   /* [total_path, C]                                                                */
    const float* target;                 /* [total_path, C]                                                                */
    const float* v;                      /* [total_nodes, C]  per sample its free rows, then its collided rows             */
    const int32_t* path_ptr;             /* [B + 1]                                                                        */
    const int32_t* node_ptr;             /* [B + 1]                                                                        */
    const int32_t* n_free;               /* [B]                                                                            */
    const int32_t* take;                 /* [B]                                                                            */
    const int32_t* problem_ids;          /* [B]  what problem[] receives                                                   */
} gnnmp_smooth_replay_src;

typedef struct {
    int32_t n_paths, total_rows, config_size, divisor;
    const int32_t* path_ptr;             /* [G + 1]                                                                        */
    const float* pred;                   /* [total_rows, C]                                                                */
    const float* target;                 /* [total_rows, C]                                                                */
    double* terms;                       /* out [G]                                                                        */
    float* loss;                         /* out [1]                                                                        */
    float* d_pred;                       /* out [total_rows, C]                                                            */
} gnnmp_smooth_path_loss_desc;

int gnnmp_smooth_replay_append(const gnnmp_smooth_replay* store, const gnnmp_smooth_replay_src* src, void* hip_stream);
int gnnmp_smooth_replay_gather(const gnnmp_smooth_replay* store, int32_t n_group, int32_t n_samples, const int32_t* idx,
                               const gnnmp_smooth_batch* out, float* out_target, void* hip_stream);
int gnnmp_smooth_path_loss(const gnnmp_smooth_path_loss_desc* desc, void* hip_stream);

/* ------------------------------------------------------------------------------------------
 * The explorer's training loop around one optimizer step on maze problems (additive to ABI 9; explorer_replay_kernels.hip) --
 * train_explorer.py:96-210 over the labelled graphs of algorithm/dijkstra.py:91-97: the batch of a group of problems gathered
 * out of a device-resident dataset, and the policy loss of :172 with its gradient.
 *
 * The dataset is a struct of caller-owned device arrays: problem i is rows node_ptr[i] : node_ptr[i + 1] of v and points64,
 * columns edge_ptr[i] : edge_ptr[i + 1] of edge_index (graph-local node ids), edge_free and edge_cost, and rows obs_ptr[i] :
 * obs_ptr[i + 1] of obstacles.  C = config_size (2 .. 14), S = obs_size (1 .. 16).
 *
 *   gnnmp_episode_dataset_gather   ONE launch, one workgroup per group entry: the arrays of problems idx[0 .. G) in that order
 *       (repeats allowed) and the three prefix arrays [G + 1] of the batch.  Wave 0 of every workgroup runs the same exclusive
 *       scan over the G entries, so no workgroup reads what another writes.  The totals of `out` are the caller's (it mirrors
 *       the prefix arrays).  An index outside [0, n_problems) is NOT clamped: that slot is empty (its prefix entries repeat
 *       the previous ones, nothing is copied for it) and status bit 1 is set; the other slots are written as usual.  When the
 *       prefix entries of a selected problem do not ascend inside the store's totals, or the totals the kernel finds differ
 *       from out's, NOTHING is written but status bit 2.  status is accumulated (OR) and cleared by the caller.
 *   gnnmp_episode_frontier_loss    what follows gnnmp_episode_frontier: one launch of one wave per problem plus a one-lane sum.
 *       Problem b's frontier is frontier[2 edge_ptr[b] + b ...][0 .. frontier_len[b]) (edge ids of the batch), label[b] the
 *       position of the next edge in it.  With m = the maximum of the listed scores and sum = sum over the LIST of exp(s - m)
 *       in double (lane l of the wave adds the entries l, l + 64, ... in ascending order, the 64 partial sums meet in a fixed
 *       butterfly; an edge listed twice counts twice, as policy[frontier] does), terms[b] = log(sum) - (s_label - m) rounded
 *       to float32 once -- log_softmax's order --, counted[b] = 1, and dscores[e] = (count_e exp(s_e - m) / sum - [e is the
 *       label's edge]) / divisor, evaluated in double and rounded once, exactly 0 for an edge of the problem that is not
 *       listed.  A problem with status != 0, frontier_len == 0 or label < 0 is not counted: terms[b] = 0, counted[b] = 0,
 *       dscores 0 over its whole edge range.  loss = (terms[0] + terms[1] + ..., ascending, in double) / divisor, rounded
 *       once.  `bad` (accumulated by an integer OR, cleared by the caller): bit 1 a frontier entry outside its problem's edge
 *       range (it contributes nothing), or frontier_len outside [0, 2 E + 1], label >= frontier_len or the label's entry
 *       outside the range (the problem is not counted); bit 2 edge_ptr entries that do not ascend inside [0, total_edges]
 *       (term 0, counted 0, no dscores written); bit 4 a problem of more than 16384 edges (not counted).
 * No floating-point atomics, no scratch, no allocation, no synchronisation: two runs give the same bits.
 *
 * Checks, in this order, each before any HIP call: GNNMP_ERR_NULL (a struct), GNNMP_ERR_DIMS (gather: config_size outside
 * 2 .. 14 or obs_size outside 1 .. 16), GNNMP_ERR_ARG (a negative count or total; out->n_problems != n_group; a divisor that
 * is not a finite number above 0), GNNMP_ERR_NULL (an array: the store's first, then the call's own), then GNNMP_OK WITHOUT
 * ANY HIP CALL AND WITHOUT WRITING ANYTHING when there is no work: n_group == 0 (gather), n_problems == 0 (loss).
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int32_t n_problems, total_nodes, total_edges, total_obs, config_size, obs_size;
    const float* v;                      /* [total_nodes, C]                                                               */
    const double* points64;              /* [total_nodes, C]                                                               */
    const int64_t* edge_index;           /* [2, total_edges]  graph-local node ids                                         */
    const uint8_t* edge_free;            /* [total_edges]                                                                  */
    const double* edge_cost;             /* [total_edges]                                                                  */
    const float* obstacles;              /* [total_obs, S]                                                                 */
    const int32_t* node_ptr;             /* [n_problems + 1]                                                               */
    const int32_t* edge_ptr;             /* [n_problems + 1]                                                               */
    const int32_t* obs_ptr;              /* [n_problems + 1]                                                               */
    int32_t* status;                     /* [1]  bits 1 / 2, see above                                                     */
} gnnmp_episode_dataset;

typedef struct {
    int32_t n_problems, total_nodes, total_edges, total_obs;     /* the group's size and the caller's totals               */
    float* v;                            /* out [total_nodes, C]                                                           */
    double* points64;                    /* out [total_nodes, C]                                                           */
    int64_t* edge_index;                 /* out [2, total_edges]                                                           */
    uint8_t* edge_free;                  /* out [total_edges]                                                              */
    double* edge_cost;                   /* out [total_edges]                                                              */
    float* obstacles;                    /* out [total_obs, S]                                                             */
    int32_t* node_ptr;                   /* out [G + 1]                                                                    */
    int32_t* edge_ptr;                   /* out [G + 1]                                                                    */
    int32_t* obs_ptr;                    /* out [G + 1]                                                                    */
} gnnmp_episode_dataset_batch;

typedef struct {
    int32_t n_problems, total_edges;
    double divisor;
    const int32_t* frontier;             /* [2 total_edges + B]  gnnmp_episode_frontier's                                  */
    const int32_t* frontier_len;         /* [B]                                                                            */
    const int32_t* label;                /* [B]                                                                            */
    const int32_t* status;               /* [B]                                                                            */
    const int32_t* edge_ptr;             /* [B + 1]                                                                        */
    const float* scores;                 /* [total_edges]                                                                  */
    float* terms;                        /* out [B]                                                                        */
    int32_t* counted;                    /* out [B]                                                                        */
    float* loss;                         /* out [1]                                                                        */
    float* dscores;                      /* out [total_edges]                                                              */
    int32_t* bad;                        /* [1]  bits 1 / 2 / 4, see above                                                 */
} gnnmp_episode_frontier_loss_desc;

int gnnmp_episode_dataset_gather(const gnnmp_episode_dataset* store, int32_t n_group, const int32_t* idx,
                                 const gnnmp_episode_dataset_batch* out, void* hip_stream);
int gnnmp_episode_frontier_loss(const gnnmp_episode_frontier_loss_desc* desc, void* hip_stream);

/* ------------------------------------------------------------------------------------------
 * The NEXT planning network of the arm families (additive to ABI 9) -- the PPN of next_model/model3D.py:87-213 behind Model3D
 * (next_7, next_ur5, next_13: point_dim 3; next_14: point_dim 6) with env_width 15 (3375 voxels), cap = g = 8, latent 64.  A
 * network input row is [point (point_dim), state (dim)]; no coordinate is scaled.  Batched over problems and over states:
 *   gnnmp_next3d_pb_forward     pb_rep of B problems: the goal attention (1 x 1 x 1-conv MLP (point_dim + 3)-16-16-32-32-64-1 over
 *                               the voxels, voxel (i, j, k) entering as [point, j, i, k]; softmax over the 3375 voxels, times
 *                               softmax(dim-64-8 MLP of the state part), in double), hidden (3 x 3 x 3, 9 -> 64), h0 / c0
 *                               (3 x 3 x 3, 64 -> 64) and `iters` rounds of { conv 3 x 3 x 3 64 -> 64 on h; LSTMCell(64, 64) per
 *                               voxel }, in exact fp32 MFMA (hidden, h0, c0 and the first round, whose sums reach the hundreds,
 *                               accumulate on the double-precision MFMA and store fp32).  One launch per stage and per round over (problem, tile of 128
 *                               voxels); h (double-buffered), c, the hidden layer and the 9-channel input live in `workspace` as
 *                               channel-last rows, gnnmp_next3d_workspace_bytes(B) bytes (about 3.7 MB a problem), 16-byte
 *                               aligned, caller-owned, contents undefined before and after the call.
 *   gnnmp_next3d_state_forward  y = [action mean, value] of S input rows, each read out of its problem's pb_rep through the state
 *                               attention, the sum over voxels and cap (accumulated in double) and the policy MLP 8-128-64-(dim+1)
 * Both calls run on hip_stream and do not synchronise or allocate; results are bit-identical from run to run and a problem's
 * pb_rep does not depend on the batch it is in.
 *
 * Packed weights (gnnmp_next3d_weights_floats floats, the same count for every (dim, point_dim);
 * gnnmp.next_model3d.pack_weights writes them): the attention's six shared layers as [out][in] weight then bias (the first layer's
 * rows padded to 12 inputs, the last bias padded to 4 floats), its dim-64-8 MLP (first layer [64][16], columns >= dim zero), the
 * policy MLP (last layer padded to [16][64] + 16), then hidden / h0 / c0 / conv as [27 taps x (cin padded to 16s) / 16][4 column
 * tiles][64 lanes][4 steps] + 64 biases (tap = (di 3 + dj) 3 + dk) and the LSTM as [8][16][64][4] over K = [input 64 | hidden 64],
 * N = the 256 gate rows, + 256 summed biases, element order as for gnnmp_next_weights_floats.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int32_t n_problems, dim, point_dim, width;   /* B >= 0 (0: nothing is done); 1 <= dim <= 15; point_dim 3 / 6; width 15  */
    int32_t iters;                       /* LSTM rounds >= 0; the reference runs 20; 0 returns h0                         */
    const float* maps;                   /* [B, 15, 15, 15]  0 = free                                                      */
    const float* goals;                  /* [B, point_dim + dim]                                                           */
    const float* weights;                /* packed, see above                                                              */
    float* pb_rep;                       /* out [B, 64, 15, 15, 15]: pb_forward(...) viewed as [B, g * cap, ...], c = 8 g + cap */
    void* workspace;                     /* device memory, 16-byte aligned                                                 */
    size_t workspace_bytes;              /* >= gnnmp_next3d_workspace_bytes(B)                                             */
} gnnmp_next3d_pb;

typedef struct {
    int32_t n_states, n_problems, dim, point_dim, width;   /* S >= 0 (0: nothing is done), B >= 0                          */
    const float* inputs;                 /* [S, point_dim + dim]                                                           */
    const int32_t* problem_of_state;     /* [S]  any order, repeats allowed                                                */
    const float* pb_rep;                 /* [B, 64, 15, 15, 15]                                                            */
    const float* weights;                /* packed, see above                                                              */
    float* y;                            /* out [S, dim + 1]: the action mean, then the value                              */
    int32_t* status;                     /* [2] device-writable, ACCUMULATED (zero it first), as gnnmp_next_states.status  */
} gnnmp_next3d_states;

/* GNNMP_ERR_NULL (n_floats), GNNMP_ERR_DIMS (dim outside 1 .. 15, point_dim not 3 / 6). */
int gnnmp_next3d_weights_floats(int32_t dim, int32_t point_dim, size_t* n_floats);
/* GNNMP_ERR_NULL (bytes), GNNMP_ERR_ARG (n_problems < 0).  Monotone in n_problems. */
int gnnmp_next3d_workspace_bytes(int32_t n_problems, size_t* bytes);
/* All argument errors come back before anything is launched, in this order: GNNMP_ERR_NULL (the struct), GNNMP_ERR_DIMS (dim,
 * point_dim, width not 15), GNNMP_ERR_ARG (n_problems / n_states < 0, iters < 0, workspace_bytes too small, a workspace that is
 * not 16-byte aligned), GNNMP_ERR_NULL (an array, the workspace included). */
int gnnmp_next3d_pb_forward(const gnnmp_next3d_pb* desc, void* hip_stream);
int gnnmp_next3d_state_forward(const gnnmp_next3d_states* desc, void* hip_stream);

/* ------------------------------------------------------------------------------------------
 * Training the 3-D NEXT network of the arm families (additive to ABI 9; next3d_train_kernels.hip) -- the forward that keeps its
 * activations and the backward, for 1 <= dim <= 15, point_dim 3 / 6, width 15.  The 2-D training calls above, for Model3D:
 *   gnnmp_next3d_train_forward   what gnnmp_next3d_pb_forward followed by gnnmp_next3d_state_forward computes, with the same bits
 *                                in pb_rep and y, and into the workspace x9, the hidden layer, h and c of every round (round r
 *                                reads slot r and writes slot r + 1) and every round's conv output, as [3376][64] rows whose last
 *                                row stays zero (about 0.86 MB a slot, 55 MB a problem at 20 rounds).
 *   gnnmp_next3d_state_backward  dy [S, dim + 1] -> dpb_rep [B, 64, 15, 15, 15] and dweights[0, per-state range): the shared
 *                                attention MLP, mlp.0, mlp.2 and the policy MLP, summed over the rows in ascending row index in
 *                                double.
 *   gnnmp_next3d_pb_backward     dpb_rep -> dweights of hidden, h0, c0, conv and lstm, summed over the problems in ascending
 *                                problem index in double.  As gnnmp_next_pb_backward it REWRITES the attention range of dweights
 *                                as float(the state call's double sum, kept in the workspace, + the goals' sum in ascending
 *                                problem index): it runs after gnnmp_next3d_state_backward on the same struct and workspace; with
 *                                n_states == 0 the state sum counts as zero and the policy range is written as zero.
 * dweights is float32, gnnmp_next3d_weights_floats long, in the packed layout; padding lanes receive zero.  When there is work
 * dweights and dpb_rep are overwritten, never accumulated into.  No floating-point atomics: two runs are bit-identical.  A
 * problem_of_state outside [0, B) is counted in the forward's status words, its row of y is NaN, and nothing is read or written
 * for it in the forward or the backward.
 *
 * weights_t (gnnmp_next3d_weights_t_floats floats; gnnmp.next_train3d.pack_weights_t writes them): conv, h0 and c0 with the taps
 * flipped on all three axes and the channel matrix transposed, in the convolution packing above, the LSTM's
 * [256 gate rows][x 64 | h 64] in the MFMA packing, and 64 zeros.
 *
 * Checks, in this order, each before any HIP call: GNNMP_ERR_NULL (the struct), GNNMP_ERR_DIMS (dim, point_dim, width not 15),
 * GNNMP_ERR_ARG (a negative count), GNNMP_ERR_NULL (an array), then GNNMP_OK WITHOUT ANY HIP CALL AND WITHOUT WRITING ANYTHING
 * when there is no work -- n_problems == 0, and for gnnmp_next3d_state_backward n_states == 0 as well
 * (gnnmp_next3d_train_forward with n_states == 0 computes pb_rep only) -- then GNNMP_ERR_WORKSPACE (workspace_bytes below
 * gnnmp_next3d_train_workspace_bytes, or the workspace not 256-byte aligned).
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int32_t n_problems, n_states, dim, point_dim, width, iters;
    const float* maps;                   /* [B, 15, 15, 15]                                                                */
    const float* goals;                  /* [B, point_dim + dim]                                                           */
    const float* inputs;                 /* [S, point_dim + dim]                                                           */
    const int32_t* problem_of_state;     /* [S]  any order, repeats allowed                                                */
    const float* weights;                /* packed, gnnmp_next3d_weights_floats floats                                     */
    float* pb_rep;                       /* out [B, 64, 15, 15, 15]                                                        */
    float* y;                            /* out [S, dim + 1]                                                               */
    int32_t* status;                     /* [2] accumulated, as gnnmp_next3d_states.status                                 */
    void* workspace;                     /* device memory, 256-byte aligned; the backward reads it                         */
    size_t workspace_bytes;
} gnnmp_next3d_train;

typedef struct {
    int32_t n_problems, n_states, dim, point_dim, width, iters;   /* as in the forward                                     */
    const float* goals;                  /* [B, point_dim + dim]                                                           */
    const float* inputs;                 /* [S, point_dim + dim]                                                           */
    const int32_t* problem_of_state;     /* [S]                                                                            */
    const float* weights;                /* packed                                                                         */
    const float* weights_t;              /* the transposed packing, see above                                              */
    const float* pb_rep;                 /* [B, 64, 15, 15, 15]  the forward's                                             */
    const float* dy;                     /* [S, dim + 1]                                                                   */
    float* dpb_rep;                      /* [B, 64, 15, 15, 15]  out of the state call, in of the pb call                  */
    float* dweights;                     /* out, gnnmp_next3d_weights_floats floats                                        */
    void* workspace;                     /* the forward's                                                                  */
    size_t workspace_bytes;
} gnnmp_next3d_train_bwd;

/* GNNMP_ERR_NULL (bytes), GNNMP_ERR_ARG (a negative count).  A multiple of 256, strictly increasing in each argument, computed
 * in size_t. */
int gnnmp_next3d_train_workspace_bytes(int32_t n_problems, int32_t iters, int32_t n_states, size_t* bytes);
/* GNNMP_ERR_NULL (n_floats), GNNMP_ERR_DIMS (dim outside 1 .. 15, point_dim not 3 / 6). */
int gnnmp_next3d_weights_t_floats(int32_t dim, int32_t point_dim, size_t* n_floats);
int gnnmp_next3d_train_forward(const gnnmp_next3d_train* desc, void* hip_stream);
int gnnmp_next3d_state_backward(const gnnmp_next3d_train_bwd* desc, void* hip_stream);
int gnnmp_next3d_pb_backward(const gnnmp_next3d_train_bwd* desc, void* hip_stream);

/* ------------------------------------------------------------------------------------------
 * NEXT's guided planner on maze problems (ABI 9) -- eval_next.py's NEXT_plan(env, model, T=t_max, g_explore_eps=0.1,
 * stop_when_success, c=1, k=10) (algorithm/tsa.py:12-81, 141-220 over algorithm/search_tree.py) as
 * gnnmp.next_plan.plan_host restates it -- batched, every problem on its own streams, the whole t_max loop of all problems in
 * ONE launch, one workgroup of 256 threads per problem.  It is gnnmp_rrtstar_plan's iteration plus the branch a model adds.
 * Per iteration the raw double r0 is read: r0 < 0.05 -> the sample is the goal state (1 double); else r1 is read and
 * r1 < g_explore_eps -> the RRT step (2 + dim doubles, as gnnmp_rrtstar_plan); else the guided step (2 doubles):
 *   - select: the first maximum over the non-terminal nodes of (double)state_value + c * sqrt(log(w_sum) / w);
 *   - one network evaluation of that parent gives the action mean; the k actions are fl32(mean + fl32(scale * eps[g][j])) --
 *     two float32 roundings -- with g the problem's count of guided iterations so far;
 *   - candidates parent + (double)action, x and y clipped to +-1, the angle wrapped, no collision check; k network
 *     evaluations give their values Q_j, w_j = w(candidate) over the tree as it stands; the first maximum of
 *     (double)Q_j + c * sqrt(log(w_sum) / w_j) is stepped to with the counted env.step(parent, candidate).  k = 1 takes the
 *     only candidate without evaluating it.
 * Insertion, both branches: one network evaluation of the new state (its value), visits[parent] += 1, w_sum -= w[parent],
 * w[parent] recomputed over the tree INCLUDING the new state, w_sum += w[parent], w[new] over the same tree, w_sum += w[new]
 * (three separately rounded operations), then RRTS_rewire_last.  w(s) = sum over the nodes of max(exp(-(dist / 0.05)^2), 1e-3)
 * in double, in a fixed order.  A network evaluation has the bits gnnmp_next_state_forward gives for the float32 state.
 * UCB_type 'GP' and Model3D (the arm families) are not built.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int32_t n_problems, dim, width;      /* dim 2 = point robot, 3 = stick robot; width must be 15                      */
    int32_t t_max, stop_when_success;    /* NEXT_plan's T, t_max + 1 <= gnnmp_next_plan_max_nodes(); non-zero: the loop ends
                                          * with the first node in the goal region                                      */
    int64_t draws_per_problem;           /* doubles in a problem's block; t_max * (2 + dim) always suffices             */
    const double* maps;                  /* [B, 15, 15]  0 = free                                                       */
    const double* init_states;           /* [B, dim]                                                                    */
    const double* goal_states;           /* [B, dim]                                                                    */
    const double* draws;                 /* [B, draws_per_problem]  the RAW doubles of [0, 1) of the problem's generator  */
    double g_explore_eps;                /* the reference runs 0.1                                                      */
    double c;                            /* exploration weight of both scores; the reference runs 1                     */
    int32_t k;                           /* candidates of a guided step, 1 .. 16; the reference runs 10                 */
    int32_t eps_rows;                    /* rows of eps per problem, >= 1; t_max always suffices                        */
    float scale;                         /* float32 diagonal of the Cholesky factor of eye * std^2: 0.015f at the default std */
    const float* pb_rep;                 /* [B, 64, 15, 15]  gnnmp_next_pb_forward's                                    */
    const float* weights;                /* packed, gnnmp_next_weights_floats floats                                    */
    const float* eps;                    /* [B, eps_rows, k, dim]  standard normal draws; row g feeds the problem's g-th
                                          * guided iteration                                                            */
} gnnmp_next_plan_batch;

typedef struct {                         /* all out; rows of a problem behind its n_nodes are left as they were         */
    double* states;                      /* [B, t_max + 1, dim]  as gnnmp_rrtstar_tree, down to status                  */
    int32_t* parents;
    int32_t* rewired_parents;
    uint8_t* flags;
    double* costs;
    double* path_lengths;
    int64_t* cumulated_checks;
    int32_t* path;
    int32_t* n_nodes;
    int32_t* success;
    int32_t* last_iter;
    int32_t* used;
    int32_t* path_len;
    int32_t* status;                     /* [B]  0, or bits: 1 and 2 as gnnmp_rrtstar_tree; 4 = the eps block ended before a
                                          * guided iteration (the tree holds the iterations before it; nothing is read beyond
                                          * the block); 8 = a score was not finite.  Any of 1, 4, 8 ends the problem: the
                                          * tree, `used` and `guided` are those of the iterations before it                 */
    int8_t* expanded_by_rrt;             /* [B, t_max + 1]  1 = goal or RRT step, 0 = guided step, -1 for the root       */
    float* state_values;                 /* [B, t_max + 1]  the network's value of every node                            */
    double* w;                           /* [B, t_max + 1]                                                               */
    int32_t* visits;                     /* [B, t_max + 1]  1 for the root plus one per child                            */
    double* w_sum;                       /* [B]                                                                          */
    int32_t* guided;                     /* [B]  guided iterations run = rows of eps used                                */
} gnnmp_next_plan_tree;

/* Trees are capped at this many nodes (t_max + 1): the node state lives in LDS next to the problem's pb_rep. */
int gnnmp_next_plan_max_nodes(void);

/* One launch on hip_stream: no allocation, no synchronisation, no atomics, deterministic (w included).  All argument errors
 * come back before anything is launched: GNNMP_ERR_NULL (a NULL struct or array), GNNMP_ERR_DIMS (dim not 2 / 3, width not
 * 15), GNNMP_ERR_ARG (n_problems / t_max < 1, t_max + 1 above gnnmp_next_plan_max_nodes(), k outside 1 .. 16, eps_rows < 1,
 * draws_per_problem < 2 + dim -- shorter than one iteration -- or beyond 2^31 - 1). */
int gnnmp_next_plan(const gnnmp_next_plan_batch* batch, const gnnmp_next_plan_tree* tree, void* hip_stream);

/* ------------------------------------------------------------------------------------------
 * Supervision of the explorer's training step (train_explorer.py:124-176): edge labels, shortest paths to the goal,
 * the greedy roll-out of the detached policy and the frontier / label of the loss, for a batch of problems.
 *   gnnmp_episode_label_maze      construct_graph's collision checks and costs     algorithm/dijkstra.py:15-31
 *   gnnmp_episode_paths           dijkstra(nodes, neighbors, edge_cost, goal)     algorithm/dijkstra.py:49-76
 *   gnnmp_episode_explore         explore(edge_cost, policy, start, goal, steps)  train_explorer.py:42-63
 *   gnnmp_episode_frontier        policy_data(...)                                train_explorer.py:66-93
 * Problem b owns node rows [node_ptr[b], node_ptr[b+1]) and edge columns [edge_ptr[b], edge_ptr[b+1]) of edge_index
 * (graph-local ids).  The edge set of a problem must be the coalesced, symmetric set construct_graph builds (columns sorted
 * by (source, target); (s, t) present iff (t, s) present).  Cell (a, c) of the reference's dense P[target][source] is the
 * edge (c -> a).  All pointers are device pointers; every call is one launch on hip_stream, no synchronisation.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int32_t n_problems, total_nodes, total_edges;
    const int32_t *node_ptr, *edge_ptr;
    const int64_t* edge_index;   /* [2, total_edges]                                          */
} gnnmp_episode_graphs;

/* Maze problems: edge_free [total_edges] (1 = MazeEnv._edge_fp(points[source], points[target])) and edge_cost
 * [total_edges] (norm(points[target] - points[source]) as numpy computes it, +inf when blocked).  points: float64
 * [total_nodes, dim], dim 2 (point robot) or 3 (stick robot); maps: float64 [B, width, width] (1 = obstacle). */
int gnnmp_episode_label_maze(const gnnmp_episode_graphs* graphs, int32_t dim, int32_t width, const double* points,
                             const double* maps, uint8_t* edge_free, double* edge_cost, void* hip_stream);
/* One workspace serves paths, explore and frontier (256-byte aligned). */
int gnnmp_episode_workspace_bytes(const gnnmp_episode_graphs* graphs, size_t* bytes);
/* Shortest paths to goal_index[b] over the reversed edges: dist [total_nodes] float64 (+inf when unreachable), prev
 * [total_nodes] (next node towards the goal; prev[goal] = goal; -1 when unreachable), n_valid [B] = finite distances
 * (-1 when the edge set is not symmetric). */
int gnnmp_episode_paths(const gnnmp_episode_graphs* graphs, const double* edge_cost, const int32_t* goal_index,
                        double* dist, int32_t* prev, int32_t* n_valid, void* workspace, size_t workspace_bytes,
                        void* hip_stream);
/* Greedy roll-out of the detached scores [total_edges] from start_index[b] for at most max_steps steps: step [B] = the
 * step at which the goal was taken, or max_steps - 1; status [B] = 0 ok, 1 skipped (n_valid == 1: only the goal is
 * reachable), 2 skipped (the frontier emptied), 3 bad input (ids out of range, edge set not symmetric); step = -1 when
 * skipped. */
int gnnmp_episode_explore(const gnnmp_episode_graphs* graphs, const float* scores, const uint8_t* edge_free,
                          const int32_t* goal_index, const int32_t* start_index, const int32_t* n_valid, int32_t max_steps,
                          int32_t* step, int32_t* status, void* workspace, size_t workspace_bytes, void* hip_stream);
/* The same roll-out for exactly step[b] steps, then the frontier: frontier [2 * total_edges + B] holds problem b's cells
 * as edge ids (batch-wide column numbers of edge_index) from int offset 2 * edge_ptr[b] + b, in the reference's order
 * (explored position, then column), frontier_len [B]; label [B] = next_edge_idx, the label's position in that list
 * (-1 for skipped problems: status[b] != 0, frontier_len 0). */
int gnnmp_episode_frontier(const gnnmp_episode_graphs* graphs, const float* scores, const uint8_t* edge_free,
                           const int32_t* goal_index, const int32_t* start_index, const int32_t* n_valid,
                           const double* dist, const int32_t* prev, const int32_t* step, const int32_t* status,
                           int32_t* frontier, int32_t* frontier_len, int32_t* label, void* workspace,
                           size_t workspace_bytes, void* hip_stream);

/* ------------------------------------------------------------------------------------------
 * Ranked frontier rows for planners whose collision checks stay on the host (eval_gnn.py:198-233 without the checks):
 * for every node row a of every graph, the live cells P[a, b] sorted by score descending, ties by source id b ascending.
 * The host loop then walks the rows of the explored nodes and touches only the cells it tries.
 *
 * A batch in the gnnmp_batch convention: column e of edge_index (row stride total_edges; row 0 = source b, row 1 = target
 * a, graph-local ids) is the dense cell P[a, b] with score scores[e]; graph g owns node rows [node_ptr[g], node_ptr[g+1])
 * and columns [edge_ptr[g], edge_ptr[g+1]).  With n_graphs == 1 either prefix array may be NULL (the whole batch is the
 * graph).  The free samples are a prefix of a graph's nodes: node id >= n_free[g] means collided.
 *
 * A cell (a, b) is live iff a != b, its score != 0 (+0 and -0 are zero) and a, b < n_free[g].  If several columns name the
 * same (a, b) the column with the highest index decides (index_put); if that value is 0 the cell is dead.  Scores are
 * finite and compared as floats; a NaN cannot hang or fault anything, but the order of its row's cells is unspecified.
 *
 * Outputs (device): graph g's cells live in [edge_ptr[g], edge_ptr[g+1]) of cols (int32 source ids) and vals; row a of
 * graph g starts at row_beg[node_ptr[g] + a] (an absolute index into cols / vals: the by-target CSR position) and its first
 * row_len[node_ptr[g] + a] slots are the ranked live cells; the rest of the row's in-degree range is unspecified.  The
 * live prefixes are bit-identical from run to run.  status [n_graphs]: GNNMP_OK, or GNNMP_ERR_INDEX for a graph with a node
 * id outside [0, N_g) (such a column is dropped, never used as an address) or with a prefix-array range outside the batch
 * (nothing of that graph is read); the other graphs of the launch are unaffected.
 * Everything is enqueued on hip_stream: no allocation, no synchronisation.  Rows of any length up to the graph's edge count.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int32_t n_graphs, total_nodes, total_edges;
    const int64_t* edge_index;   /* [2, total_edges]                                          */
    const float* scores;         /* [total_edges]                                             */
    const int32_t *node_ptr, *edge_ptr;   /* [G+1]; NULL allowed for one graph                */
    const int32_t* n_free;       /* [G]                                                       */
} gnnmp_frontier_batch;

int gnnmp_frontier_workspace_bytes(const gnnmp_frontier_batch* shape, size_t* bytes);
int gnnmp_frontier_rank(const gnnmp_frontier_batch* batch, int32_t* row_beg, int32_t* row_len, int32_t* cols, float* vals,
                        int32_t* status, void* workspace, size_t workspace_bytes, void* hip_stream);
/* The row lengths at which the implementation changes path: rows of up to wave_row_cells cells are ranked by one wave,
 * longer ones by a workgroup that streams the row through tiles of block_tile_cells cells. */
int gnnmp_frontier_limits(int32_t* wave_row_cells, int32_t* block_tile_cells);

/* ------------------------------------------------------------------------------------------
 * The smoother's training targets (train_smoother.py:98): joint_smoother_ratio / joint_smoother (smoother.py:67-151) for
 * a batch of maze paths, MazeEnv's collision checks and their count included, in one launch (one wave per path, the
 * whole iters x [random_path_smoother -> prune_path -> re-spacing] loop on the device).  Two entry points share the batch
 * struct: gnnmp_oracle_smooth for the point robot (MazeEnv(dim=2), rows of two) and gnnmp_stick_oracle_smooth for the
 * stick robot (MazeEnv(dim=3), rows (x, y, z) with z the orientation coordinate in [-0.4, 0.4]; a perturbed waypoint whose
 * z leaves that range is rejected like one that leaves the map, nothing wraps).
 *
 * A waypoint is a float32 row (an untouched input waypoint) or a float64 one (perturbed or re-spaced); the reference's
 * arithmetic follows numpy's promotion per expression, so every waypoint carries a flag next to its float64 value.  The
 * random draws are the caller's: action [B, iters, random_iter, dim] (np.random.uniform(-eps, eps, dim) per trial) and either
 * node_idx [B, iters, random_iter] (the reference's randint(1, len - 1), replayed) or u in [0, 1) with
 * node_idx = 1 + min(floor(u (len - 2)), len - 3) taken at the path's current length.
 *
 * Per-path status bits (the other paths of the batch are unaffected):
 *   1 two waypoints with identical coordinates (the reference merges them as dictionary keys): path handed through
 *   2 more than max_waypoints waypoints: path handed through
 *   4 a prune round could not reach its segment's end (the reference's swallowed exception): path as before that round
 *   8 the pruned path is not a subsequence of its input (the reference's re-spacing would raise): stopped there
 *  16 bisection stack overflow (cannot happen for states inside [-1, 1]^2)
 *  32 a replayed node_idx outside [1, len - 2]: that trial was skipped
 *  64 dijkstra met two unvisited waypoints of exactly equal finite distance (the reference pops them in hash order, the
 *     device the lowest index): the result may differ from a reference run
 * 128 path_ptr[b] .. path_ptr[b + 1] is not a range inside [0, total_points]: nothing read or written for that path
 * All pointers are device pointers; one launch on hip_stream, no allocation, no synchronisation.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int32_t n_paths, total_points;
    int32_t dim;                 /* the entry point's: 2 (point robot) or 3 (stick robot); else GNNMP_ERR_DIMS */
    int32_t width;               /* map cells per side, 1 .. max_width                        */
    int32_t iters, random_iter, prune_iter;
    int32_t ratio;               /* 1 = joint_smoother_ratio (waypoint count kept), 0 = joint_smoother (paths shrink) */
    int32_t stop;                /* 0 = run to the end; 1 = end after the last iteration's random stage; 2 = after its
                                    prune (before any re-spacing): the recorded stages of the reference               */
    const int32_t* path_ptr;     /* [n_paths + 1]                                             */
    const double* paths;         /* [total_points, dim] float64 (float32 rows upcast)         */
    const uint8_t* is32;         /* [total_points] 1 = float32 row; NULL = all of them        */
    const uint8_t* maps;         /* [n_paths, width, width] 0 = free                          */
    const double* action;        /* [n_paths, iters, random_iter, dim]                        */
    const int32_t* node_idx;     /* [n_paths, iters, random_iter] or NULL                     */
    const double* u;             /* [n_paths, iters, random_iter], read when node_idx is NULL */
} gnnmp_oracle_smooth_batch;
/* The kernel's per-path limits, the same for both entry points: waypoints per path and map cells per side. */
int gnnmp_oracle_smooth_limits(int32_t* max_waypoints, int32_t* max_width);
/* out [total_points, 2] / out_is32 [total_points]: path b from row path_ptr[b], out_len[b] rows (the rest of its rows is
 * not written); checks [n_paths] = collision_check_count of the call; status [n_paths] as above. */
int gnnmp_oracle_smooth(const gnnmp_oracle_smooth_batch* batch, double* out, uint8_t* out_is32, int32_t* out_len,
                        int64_t* checks, int32_t* status, void* hip_stream);
/* The same for the stick robot: batch->dim == 3 (anything else is GNNMP_ERR_DIMS), paths / out [total_points, 3], action
 * [n_paths, iters, random_iter, 3]; the argument checks are the point robot's, in the same order. */
int gnnmp_stick_oracle_smooth(const gnnmp_oracle_smooth_batch* batch, double* out, uint8_t* out_is32, int32_t* out_len,
                              int64_t* checks, int32_t* status, void* hip_stream);

/* ------------------------------------------------------------------------------------------
 * TEST HOOKS for the training operators   (train_kernels.hip; no product module calls these)
 * ------------------------------------------------------------------------------------------
 * gnnmp_train_op runs ONE launcher of the training path -- the very function the training entry points above call, so its
 * dispatch between the MFMA and the plain kernels is what runs -- on caller-owned device buffers, on hip_stream, without
 * synchronising.  dims / bufs per operator (a buffer marked ? may be NULL; `geom` is read by the operators marked G and
 * ignored by the others; `scalar` by FILL (value), SCALE (factor) and SM_NODES_IN (scale)):
 *
 *   LINEAR           [R, K, O, relu]             X [R,K], W [O,K], b? [O], Y [R,O]          Y = act(X W^T + b)
 *   LINEAR_DX        [R, K, O, accumulate]       dY [R,O], W [O,K], dX [R,K]                dX (+)= dY W
 *   LINEAR_DW        [R, K, O]                   dY, X, dW [O,K], db? [O], scratch          dW += dY^T X, db += sum_r dY;
 *                                                scratch: gnnmp_train_dw_scratch_floats(R, K, O) floats
 *   RELU_BWD         [n]                         y, dy                                      dy = 0 where y <= 0
 *   FILL             [n]                         x
 *   NODE_IN       G  []                          out [Npad, 4C]
 *   EDGE_IN       G  []                          out [Epad, 2C]
 *   H0            G  [D]                         goal_encoder [D], H0 [Npad, D]
 *   H0_BWD        G  [D]                         dH0 [Npad, D], d_goal_encoder [D] (+=)
 *   CONCAT           [R, D, parts]               a0 .. a3 (the first `parts` are read), out [R, parts D]
 *   SPLIT            [R, D, parts, part, accumulate]   d_in [R, parts D], dst [R, D]
 *   MSG_IN        G  [D]                         X [Npad,D], EF [Epad,D], EC [Epad,D], out [Epad, 5D]
 *   MSG_IN_BWD    G  [D]                         dZ [Epad,5D], dX [Npad,D] (+=), dEC [Epad,D] (+=)
 *   POL_IN        G  [D]                         Dn [Npad,D], EF [Epad,D], out [Epad,3D]
 *   POL_IN_BWD    G  [D]                         dP [Epad,3D], dDn [Npad,D] (+=)
 *   SEGMENT_MAX   G  [D]                         M [Epad,D], A [Npad,D], arg [Npad,D] int32
 *   SEGMENT_MAX_BWD  [Npad, D]                   dA [Npad,D], arg, dM [Epad,D] (written at arg only)
 *   SCORES_OUT    G  []                          slot_scores [Epad], out [total_edges]
 *   SCORES_IN     G  []                          d_out [total_edges], d_slot [Epad]
 *   SM_NODES_IN      [P, F, Co, C]               cur [P,C], free_pts? [F,C], collided? [Co,C], out [P+F+Co, C+3]
 *   BN_FWD           [N, D, relu]                x [N,D], gamma [D], beta [D], y [N,D], stats [3,D]
 *   BN_BWD           [N, D]                      x, dy, gamma, stats, dx [N,D], dgamma [D] (+=), dbeta [D] (+=)
 *   SM_MSG_IN        [D, cap]                    n_edges (one int32), e_src, e_dst (int32), X, out [cap, 3D]
 *   SM_MSG_IN_BWD    [D, n_rows]                 n_edges, e_src, e_dst, dZ [cap,3D], dX [n_rows,D] (+=)
 *   SM_SCATTER_ADD   [D, n_rows]                 n_edges, e_dst, M [cap,D], S [n_rows,D] (+=)
 *   SM_SCATTER_ADD_BWD [D, cap]                  n_edges, e_dst, dS [n_rows,D], dM [cap,D]
 *   ADD_ROWS         [n]                         a, b, out
 *   SM_PATH_UPDATE   [P, C]                      prev, proposal, next [P,C]
 *   SM_PATH_UPDATE_BWD [P, C]                    d_next, d_proposal, d_prev
 *   SM_COORDS_BWD    [P, C]                      dXin [., C+3], d_prev [P,C] (+=)
 *   SCALE            [n]                         x, y
 *
 * The batched smoother path (the `_seg` launchers).  Every segmented operator takes the fields of the launchers' SmSeg as its
 * first dims -- S = B, A, P, Nn, Ec: problems, active problems (the prefix [0, A)), total path rows, total node rows, padded
 * edge slots -- and the four prefix arrays as its first buffers -- ptr = path_ptr, free_ptr, coll_ptr, edge_ptr, [B+1] int32
 * each, on the device.  The remaining buffers follow the launcher's own argument order.  Problem b's node rows start at
 * path_ptr[b] + free_ptr[b] + coll_ptr[b], its edge slots at round32(edge_ptr[b] + 10 path_ptr[b]) + 32 b; n_edges is [B] int32,
 * e_src / e_dst [Ec] int32 hold problem-local node ids.  `scalar` is read by SM_NODES_IN_SEG (scale).
 *
 *   SM_NODES_IN_SEG  [S, C]                      ptr, cur [P,C], free_pts, collided, out [Nn, C+3]    rows of b >= A left alone
 *   BN_SEG_FWD       [S, D, relu, out_stride]    ptr, x [Nn,D], gamma, beta, y [Nn,D], stats [B,3,D], out_stats?
 *                                                out_stats + b out_stride receives [mean; unbiased variance]; b >= A left alone
 *   BN_SEG_BWD       [S, D]                      ptr, x, dy, gamma, stats, dx [Nn,D], part [B,2,D]    dx rows, part of b >= A = 0
 *   BN_SEG_DGB       [L, B, D]                   part [L,B,2,D], dgamma [D] (+=), dbeta [D] (+=)      iterations last to first
 *   SM_MSG_IN_SEG    [S, D]                      ptr, n_edges, e_src, e_dst, X [Nn,D], out [Ec,3D]    0 in every slot not in use
 *   SM_MSG_IN_BWD_SEG [S, D]                     ptr, n_edges, e_src, e_dst, dZ [Ec,3D], dX [Nn,D] (+=)   rows of b >= A left alone
 *   SM_SCATTER_ADD_SEG [S, D]                    ptr, n_edges, e_dst, M [Ec,D], S [P,D] (assigned)    0 for b >= A
 *   SM_SCATTER_ADD_BWD_SEG [S, D]                ptr, n_edges, e_dst, dS [P,D], dM [Ec,D]             0 in every slot not in use
 *   SM_ADD_PATH_SEG  [S, D]                      ptr, X [Nn,D], Y [P,D], out [P,D]                    rows of b >= A left alone
 *   SM_ADD_PATH_BWD_SEG [S, D]                   ptr, dH [P,D], dX [Nn,D]                             0 off the active path rows
 *   SM_PATH_UPDATE_SEG [S, C]                    ptr, prev, proposal, next [P,C]                      b >= A: next = prev
 *   SM_PATH_UPDATE_BWD_SEG [S, C]                ptr, d_next, d_proposal, d_prev [P,C]                b >= A: d_prev = d_next
 *   SM_COORDS_BWD_SEG [S, C]                     ptr, dXin [Nn, C+3], d_prev [P,C] (+=)               rows of b >= A left alone
 *
 * The explorer's path with a loop count per graph:
 *
 *   FINAL_CAT        [D, it_stride, n_it, rows[0] .. rows[n_it-1]]   NC [rows[0], D], H_it0 (iteration i's H [rows[0], D] at
 *                                                i it_stride floats), out [rows[0], 2D]      out[n] = [NC[n], H of n's last iteration [n]]
 *   SEED_DH          [rows_it, rows_next, D]     d_dec [rows_it, D], dXin [rows_it, 4D], dH [rows_it, D]
 *   LINEAR_DW_ORDER  [R, K, O, R_order]          as LINEAR_DW                               the sums of LINEAR_DW over R_order rows whose
 *                                                rows >= R have dY = 0; R_order = 0 or R: LINEAR_DW itself
 *
 * Everything is validated before any launch: unknown op, n_dims / n_bufs not the operator's, a negative size (or one
 * beyond int32), a size of 0 (the launchers do not guard an empty grid; only R of the three LINEAR operators, n of FILL and
 * SCALE, and F / Co of SM_NODES_IN may be 0), a flag that is not 0 / 1, parts outside 1 .. 4 or part outside [0, parts),
 * a geometry with n_graphs, config_size, n_pad or e_pad below 1 -> GNNMP_ERR_ARG; a required buffer, or a geometry or one
 * of its arrays, NULL -> GNNMP_ERR_NULL; D of a geometry operator not an embed size of the explorer (32, 64), or a
 * geometry whose n_pad / e_pad is not a multiple of 32 -> GNNMP_ERR_DIMS.
 * The operators of the two batched paths add: B < 1 or A outside [0, B] (A, P, Nn, Ec and out_stride may be 0), n_it outside
 * 1 .. GNNMP_TRAIN_BATCH_MAX_LOOP (n_dims must be 3 + n_it), an ascending pair in rows[] or rows_next > rows_it (rows_next may be
 * 0), R_order inside (0, R) -> GNNMP_ERR_ARG; D of FINAL_CAT / SEED_DH not 32 or 64, an entry of rows[], rows_it or rows_next
 * that is not a multiple of 256, an it_stride that is not a multiple of 4, or a buffer of FINAL_CAT / SEED_DH that is not
 * 16-byte aligned (rows are moved in 16-byte pieces) -> GNNMP_ERR_DIMS.
 * New operators are appended in front of GNNMP_TOP_COUNT and existing ones keep their numbers, so adding one is a compatible
 * change: gnnmp_abi_version stays. */
enum {
    GNNMP_TOP_LINEAR = 0, GNNMP_TOP_LINEAR_DX, GNNMP_TOP_LINEAR_DW, GNNMP_TOP_RELU_BWD, GNNMP_TOP_FILL,
    GNNMP_TOP_NODE_IN, GNNMP_TOP_EDGE_IN, GNNMP_TOP_H0, GNNMP_TOP_H0_BWD, GNNMP_TOP_CONCAT, GNNMP_TOP_SPLIT,
    GNNMP_TOP_MSG_IN, GNNMP_TOP_MSG_IN_BWD, GNNMP_TOP_POL_IN, GNNMP_TOP_POL_IN_BWD, GNNMP_TOP_SEGMENT_MAX,
    GNNMP_TOP_SEGMENT_MAX_BWD, GNNMP_TOP_SCORES_OUT, GNNMP_TOP_SCORES_IN, GNNMP_TOP_SM_NODES_IN, GNNMP_TOP_BN_FWD,
    GNNMP_TOP_BN_BWD, GNNMP_TOP_SM_MSG_IN, GNNMP_TOP_SM_MSG_IN_BWD, GNNMP_TOP_SM_SCATTER_ADD,
    GNNMP_TOP_SM_SCATTER_ADD_BWD, GNNMP_TOP_ADD_ROWS, GNNMP_TOP_SM_PATH_UPDATE, GNNMP_TOP_SM_PATH_UPDATE_BWD,
    GNNMP_TOP_SM_COORDS_BWD, GNNMP_TOP_SCALE,
    GNNMP_TOP_SM_NODES_IN_SEG, GNNMP_TOP_BN_SEG_FWD, GNNMP_TOP_BN_SEG_BWD, GNNMP_TOP_BN_SEG_DGB, GNNMP_TOP_SM_MSG_IN_SEG,
    GNNMP_TOP_SM_MSG_IN_BWD_SEG, GNNMP_TOP_SM_SCATTER_ADD_SEG, GNNMP_TOP_SM_SCATTER_ADD_BWD_SEG, GNNMP_TOP_SM_ADD_PATH_SEG,
    GNNMP_TOP_SM_ADD_PATH_BWD_SEG, GNNMP_TOP_SM_PATH_UPDATE_SEG, GNNMP_TOP_SM_PATH_UPDATE_BWD_SEG, GNNMP_TOP_SM_COORDS_BWD_SEG,
    GNNMP_TOP_FINAL_CAT, GNNMP_TOP_SEED_DH, GNNMP_TOP_LINEAR_DW_ORDER, GNNMP_TOP_COUNT
};

/* The padded index space of a batch as the training path sees it (TrainGeom of kernels.hpp): device pointers into the
 * workspace given to gnnmp_train_geom_build, plus the caller's own v / goal / node_ptr.  csr: e_pad records of four ints
 * {source, target, caller column, 0} in padded node ids, -1 = pad slot; node n's incoming edges are the slots
 * [row_beg[n], row_beg[n] + deg[n]); its outgoing edges are the CSR slots out_slot[out_beg[n] .. + out_cnt[n]). */
typedef struct {
    int32_t n_graphs, config_size, n_pad, e_pad;
    const float *v, *goal;
    const int32_t *node_ptr, *node_ptr_pad, *ntile_graph, *goal_node, *row_beg, *deg;
    const int32_t* csr;
    int32_t *out_beg, *out_cnt, *out_cur, *out_slot;
} gnnmp_train_geom;

/* The prep stage of the forward, the segment sort and the out-list build of the training forward for `batch` (explicit
 * node_ptr / edge_ptr; obs_ptr may be NULL, obstacles play no part), enqueued on hip_stream; *geom_out is filled on the host at once.  workspace:
 * 256-byte aligned, >= gnnmp_train_geom_workspace_bytes. */
int gnnmp_train_geom_workspace_bytes(const gnnmp_batch* shape, int32_t config_size, size_t* bytes);
/* Test hook: the prep stage's one-launch form assembles the CSR rows of a workgroup's slice of a graph's target nodes in LDS and
 * writes them out in slot order when the slice has at most this many records and the graph at most 65536 nodes
 * (GNNMP_PREP_LDS_ROWS=0: never); other slices are scattered record by record.  Both give the same slots.  nodes_per_slice:
 * padded nodes of the batch / (graphs x slices per graph), which picks the LDS layout of the launch. */
int gnnmp_prep_lds_row_capacity(int32_t nodes_per_slice);
int gnnmp_train_geom_build(const gnnmp_batch* batch, int32_t config_size, void* workspace, size_t workspace_bytes,
                           gnnmp_train_geom* geom_out, void* hip_stream);
int gnnmp_train_op(int op, const int64_t* dims, int n_dims, void* const* bufs, int n_bufs,
                   const gnnmp_train_geom* geom_or_null, float scalar, void* hip_stream);
/* Floats of LINEAR_DW's scratch (negative status on negative sizes). */
int64_t gnnmp_train_dw_scratch_floats(int64_t R, int64_t K, int64_t O);
/* Which kernel LINEAR / LINEAR_DX / LINEAR_DW / LINEAR_DW_ORDER dispatch to at dims [R, K, O, ...]: 1 = fp32 MFMA, 0 = plain; asked of the
 * launchers' own predicate.  GNNMP_ERR_ARG for another op or bad dims. */
int gnnmp_train_op_path(int op, const int64_t* dims, int n_dims);

/* ------------------------------------------------------------------------------------------
 * Host-only helpers exported for the CPU test-suite (no device needed)
 * ---------------------------------------------------------------------------------------- */
/* Pack a row-major weight matrix W[out_f, in_f] (leading dimension ld, column offset col0, n_in
 * columns used) into the MFMA A-operand tile format consumed by the kernels:
 * dst[((ot*NTI + it)*1024) + ((r>>2)*64 + lane)*4 + (r&3)] =
 *     W[32*ot + (lane&31)][col0 + 32*it + phi(r, lane>>5)],  phi(r,h) = (r&3) + 8*(r>>2) + 4*h.
 * out_f and n_in must be multiples of 32.  Returns the number of floats written. */
int64_t gnnmp_pack_a_tiles(const float* w, int out_f, int ld, int col0, int n_in, float* dst);
/* Pack the first-layer ("raw input") form: dst[(ot*ksteps + st)*64 + lane] =
 *     W[32*ot + (lane&31)][col0 + 2*st + (lane>>5)]  (0 beyond n_in); ksteps = ceil(n_in/2). */
int64_t gnnmp_pack_a_small(const float* w, int out_f, int ld, int col0, int n_in, float* dst);
/* Per-feature vector in register order: dst[(t*2 + h)*16 + r] = b[32*t + phi(r,h)]. */
int64_t gnnmp_pack_vec(const float* b, int n, float* dst);
/* A operands of v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32 for the double-precision stretch of the node side
 * (node_free_code encoder and the attention sub-block of node_attentions.0, reference model.py:122,164-181):
 * dst[(ob*ceil(n_in/4) + ks)*64 + lane] = W[16*ob + i'][col0 + 4*ks + (lane>>4)] (0 beyond n_in) with i = lane&15 and
 * i' = i, or i' = 4*(i%4) + i/4 when row_perm (matrices multiplied by the f32 instruction, whose result register r of lane
 * group g is row 4g + r where the f64 instruction's is 4r + g).  Returns the floats written; out_f a multiple of 16. */
int64_t gnnmp_pack_f64_ops(const float* w, int out_f, int ld, int col0, int n_in, int row_perm, float* dst);

#ifdef __cplusplus
}
#endif
#endif /* GNNMP_H */
