/*
 * gll.h -- C ABI of the MI355X (gfx950) Graph Learning Layer hot path.
 *
 * Drop-in boundary for `LaplaceLearningSparseHard.apply(X, label_matrix, tau, epsilon)`
 * of jwcalder/GraphLearningLayer.  Each entry point names the reference interface it
 * replaces (file:line in the reference snapshot).  Plain pointers and sizes only: device
 * pointers are HIP device memory, `stream` is a hipStream_t passed as void*.  Row-major,
 * int32 indices.  The graph entry points read fp32 features; gll_features_forward makes them
 * from fp32, fp16 or bf16 rows (optionally unit-norm) and gll_features_backward takes the
 * gradient back.  Inputs and outputs are caller-owned; the caller also owns
 * one workspace block per call (size from gll_workspace_bytes) that carries the graph from
 * gll_forward to gll_backward (the reference keeps the same state on `ctx`,
 * GLL.py:69-70).  Nothing here synchronises the host; nothing allocates; every call is
 * stream-ordered and reentrant per stream.  Return codes: 0 ok, < 0 error (no exceptions
 * cross the ABI).
 */
#ifndef GLL_H
#define GLL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GLL_OK 0
#define GLL_ERR_INVALID_ARG (-1)
#define GLL_ERR_UNSUPPORTED (-2)
#define GLL_ERR_HIP (-3)

/* dtype codes of label_matrix / grad_output (the reference accepts float32 and int64
 * one-hot label matrices: FullySup.py:153, train_and_adversarial.py:712) */
#define GLL_DT_F32 0
#define GLL_DT_F64 1
#define GLL_DT_I64 2

/* status words the device writes into the workspace (gll_view.status).  gll_forward zeroes the
 * block's words; the solves then atomicMax / atomicAdd into them, so the adjoint words of several
 * gll_backward calls on one workspace accumulate until the next forward.  A column that hits
 * max_iter keeps its last iterate (U / wadj hold the x after max_iter updates); converging on
 * iteration max_iter itself counts as converged. */
#define GLL_ST_TINY_EPS 0      /* eps_i < 1e-10 seen (GLL.py:240-241 warns) */
#define GLL_ST_FWD_NONCONV 1   /* forward CG columns that hit max_iter */
#define GLL_ST_FWD_ITERS 2     /* max forward CG iterations over columns */
#define GLL_ST_BWD_NONCONV 3   /* adjoint CG columns that hit max_iter */
#define GLL_ST_BWD_ITERS 4     /* max adjoint CG iterations over columns */
#define GLL_ST_KNN_RESCAN 5    /* kNN rows whose candidate set failed the Gram error certificate
                                * and were re-ranked exactly over every column under the bound
                                * (diagnostic count; the result is exact either way) */
#define GLL_ST_SOLVE_FAILED 6  /* nonzero: the fused backward's gradient workgroups gave up
                                * waiting for the adjoint solves (1 s of wall clock); the gradient was written
                                * as NaN.  The Python layer raises RuntimeError on it */
#define GLL_ST_KNN_MERGE 7     /* kNN rows with more than 64 columns at the threshold scan's
                                * bound (ties): the full-row fallback ran (diagnostic count) */
                               /* (words 8, 9, 11 are internal) */
#define GLL_ST_GRID_RESCUED 10 /* whole-GPU CG solves whose grid barrier timed out (a workgroup
                                * was not resident: other kernels held the CUs) and that one
                                * workgroup then solved alone -- correct, slower (count) */
#define GLL_ST_GRAD_SPLIT 12   /* rows the last fused backward (cg_grad_fused_kernel) ran as 2 or 4
                                * waves, each over a part of the row's features (diagnostic: the
                                * gradient is bitwise the same either way; 0 when rows ran whole) */
#define GLL_ST_LIST_DROPPED 13 /* entries of caller-supplied neighbour lists (gll_forward_lists_batched,
                                * gll_graph_lists) that were dropped and the caller should hear
                                * about: an index outside [0, n), or a repeat of an earlier entry of
                                * the same row (count; the Python layer warns) */
#define GLL_ST_NWORDS 16

/* gll_problem.flags: code-path choices for tests and A/B runs; none changes a result beyond
 * fp32 summation order (each is compared against the default path in tests/) */
#define GLL_FLAG_CG_GRID 1      /* solve Luu with the whole-GPU CG even for small m */
#define GLL_FLAG_CG_PERCOL 8    /* single graphs with m > 2048: per-column CG instead of the whole-GPU CG */
#define GLL_FLAG_DIAG_GRID_OVERSUB 128 /* tests: size the whole-GPU CG at one row per workgroup,
                                        * far past its co-resident capacity -- the launch must
                                        * be refused */
#define GLL_FLAG_DIAG_GRID_FAIL 256    /* tests: inject a grid-barrier failure into the
                                        * whole-GPU CG (the rescue solve takes over) */
#define GLL_FLAG_CG_ELL 512     /* per-column CG: register-ELL kernel even where the balanced
                                 * (virtual-row) kernel would run */
#define GLL_FLAG_CG_VR 1024     /* per-column CG: balanced (virtual-row) kernel wherever it can
                                 * run (m <= 2048) */
#define GLL_FLAG_GRAD_ROWS 2048 /* feature gradient: whole-row kernel even where the
                                 * feature-chunked one would run */
#define GLL_FLAG_GRAD_CHUNK 4096 /* feature gradient: feature-chunked kernel wherever it can
                                  * run (d >= 128, d % 4 == 0) */
#define GLL_FLAG_GRAM_INLINE 8192 /* 128-tile Gram: split each tile's rows inline instead of
                                   * pre-split planes + LDS-DMA */
#define GLL_FLAG_BWD_UNFUSED 16384 /* single small graphs, fixed eps: adjoint CG and feature
                                    * gradient as two launches instead of the fused one */
#define GLL_FLAG_KNN_PANEL 65536   /* single graphs: build the kNN in row panels of 1,024 rows
                                    * (an O(panel x n) distance buffer instead of n x n; automatic
                                    * past 32 GiB of n x n distances, panels of 8 GiB) */
#define GLL_FLAG_D2_F32 131072     /* pre-split Gram route (batches): keep the distance matrix
                                    * fp32 instead of fp16 x 2^e */
#define GLL_FLAG_ROW_ORDER_OFF 262144 /* large single graphs: process the kNN select and the
                                       * chunked gradient in row-index order instead of the
                                       * pivot-grouped locality order (A/B; results identical) */
#define GLL_FLAG_KNN_GIVEN 524288  /* the neighbour lists come from the caller (gll_forward_lists_batched,
                                    * gll_graph_lists): no search, and the workspace holds no distance
                                    * buffer, Gram planes or locality order -- gll_workspace_bytes loses
                                    * its n x n term.  Unlike the flags above it belongs to the problem:
                                    * every call on that workspace carries it.  GLL_ERR_INVALID_ARG
                                    * together with a flag that only steers the search (KNN_PANEL,
                                    * GRAM_INLINE, D2_F32, ROW_ORDER_OFF) */
#define GLL_FLAG_ALL (1 | 8 | 128 | 256 | 512 | 1024 | 2048 | 4096 | 8192 | 16384 | 65536 | \
                      131072 | 262144 | 524288)
/* (Retired, rejected with GLL_ERR_INVALID_ARG: 2 GRAM_NARROW, 4 CG_CLASSIC, 16 GRAM_F32,
 * 32 CG_PIPE, 64 GRAM_NOSPLIT, 32768 CG_PAIRS -- variants that lost their A/B runs.) */

/* Process-wide test knobs (gll_set_knob): each forces a code path that the automatic choice
 * would not take on the test's shape; 0 = automatic.  None changes a result. */
#define GLL_KNOB_VR_RV 0      /* balanced CG: virtual rows per thread (4 / 8 / 10) */
#define GLL_KNOB_GRID_CAP 1   /* whole-GPU CG: co-resident workgroup capacity */
#define GLL_KNOB_GRAM_TILE 2  /* pre-split Gram: 128- or 256-row tiles */
#define GLL_KNOB_SEL_FORM 3   /* kNN select form: 1 latency (PG 2), 2 occupancy (knn_route.h select_route) */
#define GLL_KNOB_GRAM_TAIL 4  /* 256-tile Gram's short last round: 1 none, 2 as 128-subtiles
                               * instead of 64-subtiles (gram.hip launch_gram) */
#define GLL_KNOB_ROW_PRE 5    /* row build label prefetch: 1 on, 2 off (rows.hip) */
#define GLL_KNOB_GRAD_SPLIT 6 /* fused backward: long rows in feature parts: 0 automatic (on where
                               * a row holds more than one f32x4 per lane, d > 256), 1 the same,
                               * 2 off: the launch of one wave per row (fused_bwd.hip) */
#define GLL_KNOB_COUNT 7
int gll_set_knob(int knob, int value);

typedef struct gll_problem {
    int32_t n;        /* rows of X = base + m; labeled rows first (GLL.py:11,32) */
    int32_t d;        /* feature dimension */
    int32_t base;     /* labeled rows = label_matrix.shape[0] (GLL.py:32) */
    int32_t C;        /* classes = label_matrix.shape[1] */
    int32_t K;        /* neighbours incl. self, 2 <= K <= 257 (K >= n is clamped to n); the reference
                       * hard-codes 25 (GLL.py:27) */
    int32_t max_iter; /* CG iteration cap per column; 0 => 1000 */
    float tau;        /* diagonal regulariser of Luu (GLL.py:48) */
    float eps;        /* > 0: fixed epsilon (GLL.py:226); <= 0: 'auto' (GLL.py:200-205) */
    float rtol;       /* CG stop: ||r_c|| <= rtol ||b_c|| per column; 0 => 1e-6 */
    int32_t flags;    /* GLL_FLAG_* bits, 0 by default */
    int32_t* status_sink; /* optional device words (GLL_ST_NWORDS): when non-NULL the public
                           * status words accumulate there across calls (sticky; the caller
                           * reads and clears them when it likes) instead of the workspace.
                           * Batched calls: GLL_ST_FWD_ITERS / BWD_ITERS in a sink hold the
                           * iterations of graph 0 and of every column that hit max_iter --
                           * not of every column workgroup of the batch, which would all
                           * update one word (B = 64 NS: 640 same-address atomics per CG
                           * launch, ~4 us) */
} gll_problem;

/* Bytes of device workspace one forward+backward pair needs. */
size_t gll_workspace_bytes(const gll_problem* p);

/* Replaces LaplaceLearningSparseHard.forward (GLL.py:14-73) incl. knn_sym_dist
 * (GLL.py:180-244), csgraph.laplacian (GLL.py:29) and the spsolve of GLL.py:53.
 * X: n x d fp32 (16-B aligned for the vector path), Y: base x C of y_dtype,
 * U: m x C float64 output (the reference returns float64, GLL.py:66). */
int gll_forward(const gll_problem* p, const float* X, const void* Y, int y_dtype,
                void* workspace, double* U, void* stream);

/* Replaces LaplaceLearningSparseHard.backward (GLL.py:76-177): adjoint solve (GLL.py:93),
 * edge gradient loop (GLL.py:111-120), auto-eps term (GLL.py:124-139) and the Laplacian
 * SpMM (GLL.py:146-159).  gbar: m x C of g_dtype; gradX: n x d fp32 output.
 * `workspace` must be the block the matching gll_forward filled. */
int gll_backward(const gll_problem* p, const float* X, const void* Y, int y_dtype,
                 void* workspace, const void* gbar, int g_dtype, float* gradX, void* stream);

/* Batched variants (no reference counterpart -- B independent calls of
 * GLL.py:14-177 on graphs of one shape, e.g. the 6 PGD calls of one minibatch in
 * train_and_adversarial.py:711-749, or one minibatch per rank-local stream).  Graph g reads
 * X + g*n*d, Y + g*base*C and writes U + g*m*C (gbar + g*m*C, gradX + g*n*d in the
 * backward); `workspace` holds B consecutive blocks of gll_workspace_bytes(p) bytes.  Each
 * kernel is launched once for all B graphs (grid.y = graph), so small graphs fill the GPU.
 * Results are bitwise those of B single calls.  1 <= B <= 65535. */
int gll_forward_batched(const gll_problem* p, int B, const float* X, const void* Y, int y_dtype,
                        void* workspace, double* U, void* stream);
int gll_backward_batched(const gll_problem* p, int B, const float* X, void* workspace,
                         const void* gbar, int g_dtype, float* gradX, void* stream);

/* Gradients of the inputs the reference leaves without one (GLL.py:177 returns None for
 * label_matrix, tau and epsilon).  For the frozen kNN graph, with w = [0; Luu^-1 gbar] (the
 * adjoint gll_backward leaves in the workspace), P = [Y; U], W_ij = exp(-4 d_ij^2 / eps^2) and
 * G_ij = sum_c (w_ic - w_jc)(P_jc - P_ic):
 *   grad_Y[j, c] = sum_{i in N(j)} W_ji w_ic                        rows j < base
 *   grad_tau     = - sum_{i >= base, c} w_ic U_ic
 *   grad_eps     = 1/2 sum_{directed edges (i, j)} G_ij W_ij 8 d_ij^2 / eps^3      fixed eps only
 * (grad_Y and grad_tau hold for fixed and for 'auto' eps.)  Call after gll_backward(_batched)
 * on the same workspace(s) and problem.  `what`: GLL_PG_* bits; gradY: B x base x C fp32;
 * grad_tau, grad_eps: B float64 (one per graph); an output not selected in `what` may be NULL.
 * `scratch`: gll_param_grad_scratch_bytes(p, B) bytes of device memory (float64 row partials;
 * may be NULL when neither scalar is selected).  One pass over the graph rows, then a fixed-order
 * float64 sum per graph: no atomics, bitwise reproducible, and graph g of a batch equals the
 * single call.  base == 0 with GLL_PG_Y writes nothing. */
#define GLL_PG_Y   1
#define GLL_PG_TAU 2
#define GLL_PG_EPS 4   /* GLL_ERR_INVALID_ARG when p->eps <= 0 ('auto') */
size_t gll_param_grad_scratch_bytes(const gll_problem* p, int B);
int gll_param_grad_batched(const gll_problem* p, int B, void* workspace, int what,
                           float* gradY, double* grad_tau, double* grad_eps,
                           void* scratch, void* stream);

/* Cross-entropy head: replaces custom_ce_loss (losses.py:128-136) and the argmax accuracy its
 * callers take next to it (FullySup.py:156-171), read from the fp32 predictions gll_forward
 * left in the workspace (gll_view.U32; the float64 U is exactly double(U32)).  With m = n - base,
 * t_i = targets[g*m + i] and everything evaluated in float64:
 *   p_i        = double(U32[i, t_i]) + 1e-8
 *   row_loss_i = -log(p_i)               no clamp: p_i <= 0 gives the NaN / inf PyTorch gives
 *   loss[g]    = (sum_i row_loss_i) / m
 *   gbar[i, c] = float(-(1/m) / p_i) at c == t_i, 0 elsewhere   (= dloss/dU: fp32 m x C, dense,
 *                                                  what gll_backward_batched takes as GLL_DT_F32)
 *   pred_label_i = lowest index among the maxima of row i; correct[g] = #{i: pred_label_i == t_i}
 * A target outside [0, C) masks its row (the way to leave rows out): row_loss 0, a zero gbar
 * row, never counted as correct, U never indexed with it; the divisor stays m, as
 * custom_ce_loss divides by batch_size.  Call after gll_forward(_batched) on the same
 * workspace(s) and problem.  targets: B x m int64; loss: B float64; gbar: B x m x C fp32;
 * row_loss: B x m float64; pred_label: B x m int64; correct: B int64 -- all device memory, all but
 * targets and loss may be NULL.  `scratch`: gll_ce_head_scratch_bytes(p, B) bytes (0 for
 * m <= 4096: one launch, grid = B; past that a row pass plus a reduce).  The sum runs in a fixed
 * order that depends on (m, C) alone: no atomics, bitwise reproducible, and graph g of a batch
 * equals the single call.  m == 0 writes loss = 0 and nothing else. */
size_t gll_ce_head_scratch_bytes(const gll_problem* p, int B);
int gll_ce_head_batched(const gll_problem* p, int B, void* workspace, const int64_t* targets,
                        double* loss, float* gbar, double* row_loss, int64_t* pred_label,
                        int64_t* correct, void* scratch, void* stream);

/* Carlini-Wagner margin head: replaces what the attack loop of adversarial.py:688-751 computes
 * from the layer's output in PyTorch -- the two best classes of every row (its argmax, the -1e6
 * edit, argmax again) and loss2 = clamp(max(output, 1)[0] - output[idx, other], min=0).sum() --
 * read from the fp32 predictions gll_forward left in the workspace, as the cross-entropy head
 * does.  With m = n - base, o_i = other[g*m + i] and everything evaluated in float64:
 *   label_i      = a_i = lowest index among the maxima of row i   (pred_label of the ce head)
 *   second_i     = s_i = lowest index among the maxima of the row with entry a_i removed (what
 *                  the -1e6 edit finds); 0 for C = 1
 *   d_i          = double(U32[i, a_i]) - double(U32[i, o_i])
 *   row_margin_i = d_i when d_i >= 0 or d_i is NaN, else 0     (torch.clamp propagates NaN)
 *   loss[g]      = (sum_i row_margin_i) / m      (the caller applies its own c and divisor: the
 *                  reference divides by len(target) = base + m)
 *   gbar[i, c]   = float(1/m) * ([c == a_i] - [c == o_i])   fp32 m x C, dense; a zero row when
 *                  a_i == o_i.  d_i >= 0 by construction, so the clamp never cuts a finite row
 *                  and the gradient passes wherever PyTorch's passes
 *   moved[g]     = #{i : a_i == o_i}             rows the attack has already flipped
 * Ranking: numbers by value descending, NaN entries after every number, each by index ascending;
 * a row of NaN has label 0 and second 1.  An o_i outside [0, C) masks its row: margin 0, a zero
 * gbar row, not counted in moved, U never addressed with it (U[i, o_i] is picked from the
 * registers that hold the row); label and second are written all the same and the divisor stays
 * m.  other == NULL masks every row: a pure top-2 query, the attack's set-up step.  Call after
 * gll_forward(_batched) on the same workspace(s) and problem.  other: B x m int64; loss: B
 * float64; gbar: B x m x C fp32; row_margin: B x m float64; label, second: B x m int64; moved: B
 * int64 -- all device memory, all but loss may be NULL.  `scratch`:
 * gll_margin_head_scratch_bytes(p, B) bytes (0 for m <= 4096: one launch, grid = B; past that a
 * row pass plus a reduce).  The sum runs in a fixed order that depends on (m, C) alone: no
 * atomics, bitwise reproducible, and graph g of a batch equals the single call.  m == 0 writes
 * loss = 0 and moved = 0 and nothing else.  Timed under GLL_K_LOSS. */
size_t gll_margin_head_scratch_bytes(const gll_problem* p, int B);
int gll_margin_head_batched(const gll_problem* p, int B, void* workspace,
                            const int64_t* other /* B x m, may be NULL = all masked */,
                            double* loss, float* gbar, double* row_margin,
                            int64_t* label, int64_t* second, int64_t* moved,
                            void* scratch, void* stream);

/* Score/objective head: the cross-entropy head plus what a score-driven training step takes from
 * the same predictions -- the regularisers for unlabeled rows (losses.py:100-101 entropy,
 * :111-112 l2), the per-sample scores of FullySup.py:165-173 and their store
 * (train_dataset.update_score, one Python iteration per sample in the reference).  Read from the
 * fp32 predictions gll_forward left in the workspace, as the other heads do.  With m = n - base,
 * u_c = double(U32[i, c]), t_i = targets[g*m + i] and everything evaluated in float64:
 *   p_i      = u_{t_i} + 1e-8
 *   ce_i     = -log(p_i)                      t_i outside [0, C): masked, ce_i = 0
 *   ent_i    = -sum_c u_c log(u_c + 1e-8)
 *   sq_i     = sum_c u_c^2
 *   loss[g]  = (sum_i (w_ce ce_i + w_ent ent_i - w_l2 sq_i)) / m
 *   gbar[i, c] = float((1/m) (w_ce (-1/p_i) [c == t_i]
 *                             - w_ent (log(u_c + 1e-8) + u_c / (u_c + 1e-8)) - w_l2 2 u_c))
 *   row_ce = ce_i, row_entropy = ent_i, row_l2 = 1 - sq_i (the l2 score of FullySup.py:171),
 *   pred_label and correct as the cross-entropy head's.
 * No clamp: where PyTorch's formula gives NaN or inf, so does this.  A term whose weight is exactly
 * 0 is not evaluated and contributes exactly 0, even where it would be NaN: w = (1, 0, 0) is the
 * cross-entropy head, bitwise.  Masking by target touches the ce term, row_ce and correct alone --
 * ent_i and sq_i are computed for every row (regularising rows without a label is what they are
 * for) -- and the divisor stays m.  targets == NULL masks every row.
 * Score scatter: score_kind GLL_SCORE_ENTROPY stores ce_i, GLL_SCORE_L2 stores row_l2_i:
 * score_out[indices[g*m + i]] = float(score_i) for every row that is not masked and whose index
 * lies in [0, score_len); the index forms an address only after that test and a target never does.
 * Duplicate indices within one call are the caller's error: one of the candidate values is stored,
 * which one is not specified.  One score_out (score_len fp32) serves all B graphs.
 * Call after gll_forward(_batched) on the same workspace(s) and problem.  targets, indices: B x m
 * int64; loss: B float64; gbar: B x m x C fp32; row_ce, row_entropy, row_l2: B x m float64;
 * pred_label: B x m int64; correct: B int64 -- all device memory, all but loss may be NULL
 * (score_out and indices only with GLL_SCORE_NONE).  `scratch`:
 * gll_objective_head_scratch_bytes(p, B) bytes (0 for m <= 4096: one launch, one workgroup a graph
 * -- plus helper workgroups that write row_entropy when it is an output only, w_ent == 0; past
 * that a row pass plus a reduce).  The sums over rows run in the cross-entropy head's fixed order, over
 * the per-row combined term: no atomics, bitwise reproducible, and graph g of a batch equals the
 * single call.  m == 0 writes loss = 0 and nothing else.  Timed under GLL_K_LOSS. */
#define GLL_SCORE_NONE    0
#define GLL_SCORE_ENTROPY 1   /* -log(pred[i, t_i] + 1e-8), FullySup.py:169 */
#define GLL_SCORE_L2      2   /* 1 - sum(pred[i]^2), FullySup.py:171 */
size_t gll_objective_head_scratch_bytes(const gll_problem* p, int B);
int gll_objective_head_batched(const gll_problem* p, int B, void* workspace,
                               const int64_t* targets /* B x m, may be NULL = all masked */,
                               double w_ce, double w_ent, double w_l2,
                               double* loss, float* gbar, double* row_ce, double* row_entropy,
                               double* row_l2, int64_t* pred_label, int64_t* correct,
                               int score_kind, float* score_out, int64_t score_len,
                               const int64_t* indices, void* scratch, void* stream);

/* Graph only (the device half of knn_sym_dist, GLL.py:180-244): kNN search, symmetric
 * CSR, eps, weights and degrees into the workspace; no solve.  Requires p->base == 0
 * (no labeled block; size the workspace for that problem).  Read the arrays with
 * gll_workspace_view. */
int gll_graph(const gll_problem* p, const float* X, void* workspace, void* stream);

/* Device pointers of the arrays held in a workspace (for the host mirror and tests). */
typedef struct gll_view {
    int32_t* knn_idx;  /* n x K  neighbour indices, self first, ascending distance */
    float* knn_d2;     /* n x K  squared distances (fp32, exact difference form)    */
    float* eps;        /* n      epsilon_i                                           */
    int32_t* row_start; /* n     first entry of graph row i (symmetric kNN graph,   */
    int32_t* row_len;   /* n     no diagonal); entries row_start..+row_len          */
    int32_t* col;      /* E      column indices, ascending within a row             */
    float* w;          /* E      W_ij = exp(-4 d_ij^2 / (eps_i eps_j))               */
    float* d2;         /* E      d_ij^2                                              */
    float* deg;        /* n      weighted degree                                     */
    float* U32;        /* m x C  forward solution, fp32                              */
    float* wadj;       /* m x C  adjoint solution (after gll_backward)               */
    int32_t* status;   /* GLL_ST_NWORDS status words                                 */
} gll_view;
int gll_workspace_view(const gll_problem* p, void* workspace, gll_view* out);

/* The arrays the row build writes for the Luu solves (m = n - base unlabeled rows, u = i - base
 * the U index of row i), for tests of the row build alone.  Append-only beside gll_view, which
 * stays as it is.  The solves only read them, so they stand as the row build left them after
 * gll_forward(_batched).
 *   ELL slice: SE slots per U row, column-major, two slots per 16-B record: slot s of row u is
 *     the int32 pair (col - base, float bits of w) at ell[((s / 2) * m + u) * 4 + (s % 2) * 2];
 *     the row's first SE U-block entries in column order, (0, 0.0f) past ucnt[u]; a suffix
 *     longer than SE keeps its tail in the CSR only.  SE = 0: no slice (m > 4096).
 *   Virtual rows: VRM slots of 48 bytes per U row (slot j of row u at vr + (u * VRM + j) * 48):
 *     8 uint16 offsets 4 * (col - base), then 8 fp32 weights -- entries 8 j .. 8 j + 7 of the
 *     row's U block; min(ceil(ucnt[u] / 8), VRM) slots are written, the last one padded with
 *     (0, 0.0f), the rest of the row's slots untouched; a longer suffix keeps its tail in the
 *     CSR only.  VRM = 0: the problem's solves do not run the balanced kernel, nothing is
 *     written.  (VRM follows p->flags and GLL_KNOB_VR_RV as the workspace layout does.) */
typedef struct gll_solve_view {
    int32_t* ucnt;  /* m      entries of row base + u with col >= base: the row's sorted suffix */
    float* diag;    /* m      deg + tau                                                      */
    float* rhs;     /* m x C  sum over the row's labeled entries of W_ij Y_j                 */
    float* P;       /* n x C  [Y as fp32; U32]: the labeled rows are written by the row build */
    int32_t* ell;   /* SE x m (col, w) slots, see above                                      */
    void* vr;       /* m x VRM 48-byte slots, see above                                      */
    int32_t SE;     /* ELL slots per U row the row build writes: 24, 16, 4 or 0, by m        */
    int32_t VRM;    /* virtual-row slots per U row, 0 when unused                            */
    int32_t Wcap;   /* row slot width 5 (K - 1) + 8: a row with at most Wcap forward + reverse
                     * entries starts at i * Wcap, longer ones in the bump region behind n Wcap */
    int32_t RCAP;   /* reverse-list capacity per row 8 (K - 1) + 8; entries past it go through
                     * the overflow list */
} gll_solve_view;
int gll_workspace_solve_view(const gll_problem* p, void* workspace, gll_solve_view* out);

/* What the first stage of the graph build -- the Gram (gram.hip) and the locality order
 * (order.hip) -- leaves in a workspace, for tests of that stage alone.  Append-only beside the
 * other views.  `out` describes block 0 of a launch over B graphs (planes, fp16 storage and the
 * pre-split arrays depend on B); graph g's arrays lie g * gll_workspace_bytes(p) further on.  The
 * select and everything after it only read these arrays, so they stand as the Gram left them.
 *   D2: `planes` planes of `rows` x ldD elements, `plane_stride` elements apart; the select sums
 *     the planes in order.  rows = n, or the panel height PR < n of a row-panel build, where D2
 *     holds what the last panels left (panel r0 writes buffer rows 0 .. min(PR, n - r0) - 1).
 *     d2_half: the elements are fp16 of D2 x *d2_scale (element (i, j) the (i * ldD + j)-th half
 *     of the buffer), d2_scale a power of two every tile of the GEMM stores; else fp32 and
 *     d2_scale is not written.
 *   xhi / xlo / xnrm: the bf16 planes n x dp of a = x - x_0 (hi = bf16(a), lo = bf16(a - hi),
 *     zero from d to dp) and |a_i|^2, written on the pre-split route only (gll_gram_route).
 *   pid / perm: the locality order, written for single graphs with n >= 1024 and more than
 *     4 MB of X (and no row panels, no GLL_FLAG_ROW_ORDER_OFF): pid[i] = pivot | rank << 8 with
 *     rank the row's position among the rows of its 64-row block at that pivot, perm the rows
 *     grouped by pivot, blocks in order within a pivot. */
typedef struct gll_knn_view {
    void* D2;             /* fp32, or fp16 when d2_half                                    */
    float* d2_scale;      /* the fp16 scale word s                                         */
    void* xhi;            /* n x dp bf16                                                   */
    void* xlo;            /* n x dp bf16                                                   */
    float* xnrm;          /* n                                                             */
    int32_t* pid;         /* n                                                             */
    int32_t* perm;        /* n                                                             */
    int64_t plane_stride; /* elements between D2 planes                                    */
    int32_t planes;       /* planes the Gram writes: 1 or 2                                */
    int32_t ldD;          /* leading dimension of a D2 plane (n rounded up to 4)           */
    int32_t rows;         /* rows of the D2 buffer (PR)                                    */
    int32_t d2_half;      /* 1: D2 holds fp16 x s                                          */
    int32_t dp;           /* d rounded up to 64                                            */
    int32_t order;        /* 1: the build writes pid / perm                                */
} gll_knn_view;
int gll_workspace_knn_view(const gll_problem* p, int B, void* workspace, gll_knn_view* out);

/* Diagnostic: the kernels of gram.hip a graph build over B graphs launches on a device with
 * `cus` compute units, x_aligned saying whether X is 16-B aligned.  No HIP call: it runs without
 * a GPU, and the launchers launch from the same record.  out[0] = kernel family (0 gram_bf3,
 * 1 gram_bf3h, 2 gram_bf3s, 3 gram_bf3w, 4 gram_split + gram_pk<H, 128>, 5 gram_split +
 * gram_pk2<H>), out[1] = VEC of the inline-split kernel or of gram_split, out[2] = D2 planes,
 * out[3] = 1 on the pre-split route, out[4] = H (fp16 D2), out[5] = 1 for 256-tiles, out[6] =
 * 256-tiles of the last round that run as subtiles on gram_pk<H, TS>, out[7] = subtiles per such
 * tile (16: TS = 64, 4: TS = 128, 0: no tail), out[8] = row panels (0: the whole matrix in one
 * launch).  Reads GLL_KNOB_GRAM_TILE and GLL_KNOB_GRAM_TAIL. */
#define GLL_GRAM_ROUTE_WORDS 9
int gll_gram_route(const gll_problem* p, int B, int x_aligned, int cus,
                   int32_t out[GLL_GRAM_ROUTE_WORDS]);

/* Multi-RHS Jacobi-preconditioned CG on a general SPD CSR matrix (device replacement of
 * stable_conjgrad, GLL.py:247-276, as used by utils.laplace, utils.py:589).
 * A: m x m CSR (row_ptr m+1, col, val) fp32; b, x: m x C row-major fp32 (x is output).
 * Stops per column when ||r_c||_2 <= atol (absolute, like stable_conjgrad's tol) or
 * max_iter (0 => 100000); a column with ||b_c||_2 <= atol takes 0 iterations and x_c = 0.  A
 * column that hits max_iter returns its last iterate in x_c (the x after max_iter updates), not
 * zero and not NaN.  `iters` and `nonconv` (device ints, may be NULL) ACCUMULATE: the kernels
 * atomicMax the largest per-column iteration count into `iters` and atomicAdd the number of
 * columns that hit max_iter into `nonconv`, so the caller zeroes both before the call (or keeps
 * them as running maximum / sum over several calls); converging on iteration max_iter itself
 * counts as converged.  `workspace`
 * (gll_cg_csr_workspace_bytes) holds the Krylov vectors: required when m > 2048 (those
 * systems run on the whole GPU as one ordinary launch sized within the co-resident
 * workgroup capacity, C <= 16; a lost grid barrier is rescued by one workgroup solving
 * alone, counted in GLL_ST_GRID_RESCUED), may be NULL when 5 m floats fit in LDS. */
size_t gll_cg_csr_workspace_bytes(int m, int C);
int gll_cg_csr(int m, int C, const int32_t* row_ptr, const int32_t* col, const float* val,
               const float* b, float* x, float atol, int max_iter, int32_t* iters,
               int32_t* nonconv, void* workspace, void* stream);

/* Instrumentation for bench.py: with period p > 0, every p-th launch of kernel `kid` is
 * bracketed by HIP events on its stream (p = 0 disables); gll_prof_read synchronises those
 * events and returns the summed milliseconds and the number of bracketed launches, then
 * clears them. */
#define GLL_K_GRAM 0      /* gram_d2_kernel: squared distances on split-bf16 MFMA (x = hi + lo,
                           * three bf16 products; candidates only, the select re-ranks exactly) */
#define GLL_K_SELECT 1    /* knn_select_kernel: top-K + exact re-rank + reverse scatter */
#define GLL_K_FINALIZE 2  /* row_build_kernel: symmetric rows, W, degree, rhs */
#define GLL_K_CG 3        /* cg_*_kernel: Jacobi-CG solves (forward and adjoint) */
#define GLL_K_EDGE 4      /* edge_coef_kernel: auto-eps edge coefficients */
#define GLL_K_GRAD 5      /* grad_spmm_kernel: feature gradient */
#define GLL_K_BWD 6       /* cg_grad_fused_kernel: adjoint CG + feature gradient in one launch
                           * (single small graphs, fixed eps) */
#define GLL_K_PARAM 7     /* param_grad_kernel (+ param_reduce_kernel): label_matrix / tau / eps
                           * gradients (gll_param_grad_batched) */
#define GLL_K_LOSS 8      /* ce_head_kernel: cross-entropy head (gll_ce_head_batched) */
#define GLL_K_COUNT 9
int gll_prof_enable(int kid, int period);
int gll_prof_read(int kid, double* ms_total, int* count);
const char* gll_kernel_name(int kid);

/* Diagnostic: which instantiation of the kNN select a launch over `rows` rows (p->n, or one of
 * the problem's row panels) of each of B graphs runs, x_aligned saying whether X is 16-B
 * aligned.  No HIP call: it runs without a GPU.  out[0] = 1 for knn_select_wide_kernel, whose
 * template arguments (V, NP, CAP, KMX, TOP) are out[1..5]; 0 for knn_select_kernel, whose
 * (KC, V, NP, PG, NU, XQ, R, CH, H) are out[1..9]; out[10] = the variant's row in the table
 * of instantiated kernels (-1, and GLL_ERR_UNSUPPORTED, when it has none: the launch would
 * fail), out[11] = the table's length.  Reads GLL_KNOB_SEL_FORM. */
#define GLL_SEL_ROUTE_WORDS 12
int gll_select_route(const gll_problem* p, int B, int x_aligned, int rows,
                     int32_t out[GLL_SEL_ROUTE_WORDS]);

/* Diagnostic: the launch of the fused backward (cg_grad_fused_kernel) for this problem on a
 * device that holds `capacity` of its workgroups at once (occupancy x compute units), x_aligned as
 * above.  With capacity >= 0 no HIP call: it runs without a GPU, and the launcher sizes its launch
 * from the same record.  out[0] = threads per workgroup, out[1] = f32x4 vectors a lane holds of a feature row
 * (1, 2, 4), out[2] = workgroups launched, out[3] = the base grid C + ceil(n / waves per
 * workgroup) the route requires to be co-resident, out[4] = gradient waves, out[5] = spare waves
 * (out[4] - n) that take the parts of long rows, out[6] = 1 when rows may run in parts, out[7] =
 * dynamic LDS bytes.  GLL_ERR_UNSUPPORTED when the backward takes two launches instead.  Reads
 * GLL_KNOB_GRAD_SPLIT.  capacity < 0: the current device's (this form does query HIP: the
 * occupancy of the kernel a float64 grad_output runs; the float32 one has the same resources). */
#define GLL_FUSED_PLAN_WORDS 8
int gll_fused_plan(const gll_problem* p, int x_aligned, int capacity,
                   int32_t out[GLL_FUSED_PLAN_WORDS]);

/* Diagnostic: which kernel solves the Luu systems of this problem in a launch over B graphs (the
 * forward solve, and the backward's when it runs unfused).  No HIP call: it runs without a GPU,
 * and the launcher launches from the same route (cg_route.h cg_route, solve.hip's table).
 * out[0] = 1 when the whole-GPU CG (cg_gv_kernel, gridcg.hip) is tried first; out[1..5] = the
 * per-column variant the solve takes -- or falls back to when no grid configuration holds the
 * system: family (0 cg_ell_kernel, 1 cg_vr_kernel, 2 cg_lds_kernel), threads NT, rows per thread
 * R, register ELL slots S (cg_ell) or virtual rows per thread RV (cg_vr), MODE (cg_ell: 3 the
 * Neumann-1 preconditioner, 1 Jacobi; cg_vr 1; cg_lds 0, classic PCG with Jacobi); out[6] = 1 when
 * cg_lds keeps its vectors in LDS; out[7] = that variant's row in the table of instantiated
 * kernels (-1, and GLL_ERR_UNSUPPORTED, when it has none: the launch would fail), out[8] = the
 * table's length.  Reads GLL_KNOB_VR_RV. */
#define GLL_CG_ROUTE_WORDS 9
int gll_cg_route(const gll_problem* p, int B, int32_t out[GLL_CG_ROUTE_WORDS]);

/* Build identity: sha256 (16 hex) of the sources, headers and flags this library was built
 * from (graphlearninglayer_amd/build.py source_digest).  bench.py cites only profiles
 * recorded against the same identity. */
const char* gll_build_id(void);

/* Human-readable message for a return code. */
const char* gll_strerror(int code);

/* The layer's front end.  Every network of the reference ends in F.normalize(feat, dim=1)
 * (networks/BuildNet.py:101, preact_resnet.py:101, customCNN.py:36,
 * train_and_adversarial.py:420) and GLL.py:24 leaves that to the caller; under AMP the features
 * arrive as fp16 / bf16.  gll_features_forward turns `rows` feature rows Z (rows x d of z_dtype,
 * row-major, contiguous) into the fp32 rows X that gll_forward(_batched) reads, in one launch.
 * With a_k = float(z_k) (exact):
 *   flags 0:           X[i,k] = a_k; rnorm is not touched and may be NULL
 *   GLL_UF_NORMALIZE:  s = sum_k a_k^2 (fp32), r = 1 / max(sqrtf(s), 1e-12f) (F.normalize's
 *                      clamp; no rescaling against overflow of s, as torch has none),
 *                      X[i,k] = a_k r, rnorm[i] = r
 * gll_features_backward is its backward, one launch: from fp32 gX (the gradient gll_backward wrote
 * for X), X and rnorm as the forward left them,
 *   GLL_UF_NORMALIZE:  t = sum_k X[i,k] gX[i,k] (fp32), out_k = r (gX[i,k] - X[i,k] t); a clamped
 *                      row (rnorm[i] >= 1e12f) takes out_k = r gX[i,k], as the backward of torch's
 *                      clamp_min does
 *   flags 0:           out_k = gX[i,k]; X and rnorm may be NULL
 * and gZ[i,k] = out_k rounded once to z_dtype (to nearest even; an fp16 overflow gives inf).
 * One wave per row, 1 <= d <= 4096; 16-B vector accesses where d is a multiple of 16 B /
 * sizeof(element) and the arrays are 16-B aligned, scalar ones of the same elements otherwise.
 * The sums run in a fixed order that depends on d and z_dtype alone: no atomics, and a row's result
 * does not depend on rows, on its place in the call or on the alignment.  rows == 0 returns GLL_OK
 * and launches nothing; more rows than one grid holds take several launches.  Argument checks
 * come before any HIP call. */
#define GLL_XT_F32 0
#define GLL_XT_F16 1
#define GLL_XT_BF16 2
#define GLL_UF_NORMALIZE 1
int gll_features_forward(int64_t rows, int32_t d, const void* Z, int z_dtype, int flags,
                         float* X, float* rnorm, void* stream);
int gll_features_backward(int64_t rows, int32_t d, const float* gX, const float* X,
                          const float* rnorm, int flags, void* gZ, int z_dtype, void* stream);
int64_t gll_features_calls(void);  /* launches of either kernel so far in this process (host counter) */

/* Fused SupCon / SimCLR loss (losses.py:11-98: SupConLoss, and SimCLR with labels == NULL), its
 * forward and its gradient, without the R x R logits ever in memory.  Z is the contiguous
 * features tensor [bsz, V, d] in memory order: row r = b V + v is view v of sample b, R = rows =
 * bsz V.  lab(r) = labels[r / V], or r / V when labels is NULL.  Row r is an anchor always
 * (GLL_SC_ALL) or when v == 0 (GLL_SC_ONE); A = R or bsz anchors.  For an anchor r:
 *   l_rj   = (z_r . z_j) / T                       every j in [0, R)
 *   m_r    = max_j l_rj                            (the diagonal included, losses.py:73)
 *   E_r    = sum_{j != r} exp(l_rj - m_r)
 *   pos(r) = { j != r : lab(j) == lab(r) },  c_r = |pos(r)|,  P_r = sum_{j in pos(r)} l_rj
 *   row_loss_r = -(T / Tb) (P_r / c_r - m_r - log E_r)
 *   loss   = (sum_{anchors r} row_loss_r) / A
 * and with gl = *grad_loss
 *   q_rj   = (1 / (A Tb)) ([j != r] exp(l_rj - m_r) / E_r - [j in pos(r)] / c_r)  for an anchor r, else 0
 *   gZ_r   = gl sum_j (q_rj + q_jr) z_j
 * No clamps: an anchor with c_r = 0 gives 0/0, a NaN loss and an all-NaN gZ, as the reference
 * does.  Labels are only compared for equality (any int64 value).  The contract covers logits
 * whose spread m_r - l_rj stays inside the fp32 exp range (unit-norm rows at T >= 0.03 always
 * do); outside it the reference underflows to +-inf and this implementation may stay finite.
 * The explicit mask= of losses.py:29-30 is not built.
 *
 * Forward: two launches.  `stats` (rows x 4 floats) receives per row (m_r, log E_r, c_r, 1/E_r),
 * of every row, anchor or not; row_loss (A floats, may be NULL) the anchors' losses in the
 * reference's order (view-major: v bsz + b; GLL_SC_ONE: b); *loss the float64 loss.  Backward:
 * two launches, from the same Z, labels and the forward's stats; gZ is rows x d fp32.
 * The dot products run on the fp32-input MFMA (bit-for-bit an fmaf chain over the features);
 * the row sums are float64; no atomics: every sum order depends on (rows, V, d, mode) alone, so
 * two runs are bitwise equal.  `scratch`: gll_supcon_scratch_bytes(rows, d) bytes, 8-B aligned,
 * = 32 rows fchunks + 4 d rows chunks: the forward's row partials of `fchunks` column chunks and
 * the backward's gZ partials of `chunks` column chunks, both chosen from (rows, d) alone, the
 * second held to max(2 rows^2, 3 MiB) bytes (one chunk: none, the backward then writes gZ in
 * its first launch): O(rows chunks (d + 8)), never rows x rows (0 for arguments out of range).  Z needs 4-B alignment only: rows are read with 16-B loads where d % 4 == 0 and
 * Z is 16-B aligned and with scalar loads of the same elements otherwise.  2 <= rows <= 65,536,
 * 1 <= d <= 4,096 (GLL_ERR_UNSUPPORTED past them), V >= 1, rows % V == 0, T and Tb positive and
 * finite (GLL_ERR_INVALID_ARG).  Stream-ordered, no allocation, no host synchronisation;
 * argument checks come before any HIP call. */
#define GLL_SC_ALL 0
#define GLL_SC_ONE 1
size_t gll_supcon_scratch_bytes(int64_t rows, int32_t d);
int gll_supcon_forward(int64_t rows, int32_t V, int32_t d, const float* Z, const int64_t* labels,
                       int mode, float T, float Tb, double* loss, float* row_loss, float* stats,
                       void* scratch, void* stream);
int gll_supcon_backward(int64_t rows, int32_t V, int32_t d, const float* Z, const int64_t* labels,
                        int mode, float T, float Tb, const float* stats, const double* grad_loss,
                        float* gZ, void* scratch, void* stream);
int64_t gll_supcon_launches(void);  /* kernel launches of either call so far in this process (host counter) */

/* Exact query-vs-database kNN and the out-of-sample extension of a solved graph (query.hip,
 * DESIGN.md §3.12; no reference counterpart: the reference predicts for new points by rebuilding
 * and re-solving the whole graph, utils.py:637-660).  The extension's backward is
 * gll_extend_backward below.
 *
 * gll_knn_query: for every row q of Xq (Q x d fp32) the k rows of Xdb (N x d fp32) with the
 * smallest float64 sum_f (q_f - x_f)^2 of the fp32 inputs, equal distances to the lower index --
 * exact for any finite input, no near-tie allowance.  idx / d2 (Q x k): the list ordered by
 * (d2, idx), d2 the fp32 difference-form value: feature f on lane (f / 4) % 8 of an 8-lane group,
 * one fmaf chain a lane in ascending f, then a 3-level tree -- within (4 ceil(d / 32) + 8) 2^-24
 * relative of the float64 value.  Nominating distances run on the fp32-input MFMA over rows centred
 * on row 0 of Xdb, |D2 - d^2| <= (d + 16) 2^-24 (|a_q| + |a_j|)^2, a panel of min(Q, cap) query rows
 * at a time (cap: 128 MiB of panel, a multiple of 64 rows, at least 64; GLL_QF_SMALL_PANELS: 64),
 * never Q x N; three launches a panel.  status (4 device words, accumulate; the caller zeroes
 * them): [0] rows that took the exact rescan (certificate failed, or more than 512 columns at the
 * scan's threshold), diagnostic; [1] rows with a non-finite nominating or returned distance: their
 * values are unspecified, every index is in [0, N) all the same; [2] gll_extend rows with a zero
 * or NaN weight sum; [3] unused.  Xq, Xdb need 4-B alignment only (16-B loads where d % 4 == 0
 * and both are 16-B aligned, scalar loads of the same elements otherwise: the same bits);
 * workspace: gll_query_workspace_bytes bytes, 16-B aligned.  A row's result does not depend on
 * the rows that share the call or the panel; two runs are bitwise equal.
 * 1 <= k <= N (GLL_ERR_INVALID_ARG), k <= 256, 1 <= d <= 4096, N <= INT32_MAX / 2
 * (GLL_ERR_UNSUPPORTED), Q >= 1; gll_query_workspace_bytes returns 0 for arguments out of range.
 *
 * gll_extend: u(q) = sum_i w_i P[idx[q, i]] / sum_i w_i over the kn listed neighbours, in float64
 * in list order, w_i = exp(-4 double(d2[q, i]) / (eps_q eps_j)): eps > 0: eps_q = eps_j = eps;
 * eps <= 0 ('auto'): eps_q = sqrtf(d2[q, kn - 1]) (the list's last entry: what GLL.py:205 gives a
 * point with these neighbours) and eps_j = eps_db[j].  IEEE as written (no clamps): a zero or NaN
 * weight sum gives a NaN row, counted in status[2]; an index outside [0, N) is not followed and
 * gives a NaN weight.  label: the margin head's rule -- lowest index among the maxima, NaN after
 * every number.  One launch.  1 <= kn <= 256, 1 <= C <= 256.
 * Both calls are stream-ordered, allocate nothing, do not synchronise the host and check their
 * arguments before any HIP call. */
#define GLL_QF_SMALL_PANELS 1
size_t gll_query_workspace_bytes(int64_t Q, int64_t N, int32_t d, int32_t k, int flags);
int gll_knn_query(int64_t Q, int64_t N, int32_t d, int32_t k, int flags,
                  const float* Xq, const float* Xdb,
                  int32_t* idx /*Q x k*/, float* d2 /*Q x k*/,
                  int32_t* status /*4 words, accumulate*/, void* workspace, void* stream);
int gll_extend(int64_t Q, int64_t N, int32_t kn, int32_t C,
               const int32_t* idx, const float* d2 /*Q x kn*/,
               const float* P /*N x C*/, const float* eps_db /*N, or NULL*/, float eps /*>0, or <=0: auto*/,
               double* Uq /*Q x C*/, int64_t* label /*Q*/, int32_t* status, void* stream);
int64_t gll_query_launches(void);  /* kernel launches of either call (and of gll_knn_rerank) so far in this process (host counter) */

/* gll_knn_query's lists from caller-supplied candidates (rerank.hip): idx / d2 as
 * gll_extend and gll_extend_backward take them, without the search.  cand: Q x c int32, for every
 * query row c database rows -- an earlier search's lists, a wider pool searched once while the
 * queries move, an approximate index's answer.  Distances follow gll_knn_query's contract: the value
 * returned is the fp32 difference form (feature f on lane (f / 4) % 8 of an 8-lane group, one fmaf
 * chain a lane in ascending f, then the 3-level tree), the value ranked the float64 fma chain over
 * the same loads, NaN as +inf -- a pair (q, j) gets the bits gll_knn_query returns for it, from 16-B
 * or scalar loads alike.
 *   flags 0 (pool mode, k <= c): an entry is valid when it lies in [0, N) and no earlier entry of
 *     its row holds the same index.  idx / d2 (Q x k): the k valid candidates nearest by (float64
 *     d^2, index), in (returned fp32 d^2, index) order, NaN as +inf: gll_knn_query's list whenever
 *     the pool holds the k nearest.  An invalid entry is never chosen; a row with fewer than k
 *     valid candidates ends in (-1, +inf) entries and is counted in status[3] -- gll_extend gives
 *     such a row NaN and counts it in status[2].
 *   GLL_RR_KEEP_ORDER (list mode, c == k, else GLL_ERR_INVALID_ARG): idx = cand, entry by entry in
 *     the caller's order; nothing is dropped and a repeat counts twice.  An index outside [0, N) is
 *     kept, is not followed and gets d2 = +inf (gll_extend: a NaN weight).  The last column is what
 *     'auto' takes eps_q from, as the layer takes eps_i from knn_ind[:, -1].
 * status (4 device words, accumulate; the caller zeroes them): [1] rows with a non-finite returned
 * distance among the kept (list mode: the +inf of an index out of range included); [3] pool-mode
 * rows with fewer than k valid candidates; [0], [2] untouched.  One ordinary launch, one wave per
 * row, four rows per 256-thread workgroup, no workspace, no atomics but atomicAdd on the status
 * words; counted by gll_query_launches.  A row's result depends on that row, its candidates and Xdb
 * only -- not on the rows that share the call, not on the alignment -- and two runs are bitwise
 * equal.  Xq, Xdb need 4-B alignment only.  Q, N, d, k >= 1, k <= c (GLL_ERR_INVALID_ARG); c <= 512,
 * k <= 256, d <= 4096, N, Q <= INT32_MAX / 2 (GLL_ERR_UNSUPPORTED); k may exceed N (the rows are
 * short).  Stream-ordered, no allocation, no host synchronisation; argument checks come before any
 * HIP call. */
#define GLL_RR_KEEP_ORDER 1
int gll_knn_rerank(int64_t Q, int64_t N, int32_t d, int32_t c, int32_t k, int flags,
                   const float* Xq, const float* Xdb, const int32_t* cand /* Q x c */,
                   int32_t* idx /* Q x k */, float* d2 /* Q x k */,
                   int32_t* status /* 4 words, accumulate */, void* stream);

/* Backward of gll_extend (extend_grad.hip).  The neighbour lists are frozen, as
 * the layer's kNN graph is.  For query q and list entry i, with j = idx[q, i], d_i =
 * double(d2[q, i]) (the fp32 value gll_knn_query returned), e_q and e_j as in gll_extend,
 *   t_i = 4 d_i / (e_q e_j),  w_i = exp(-t_i),  S = sum_i w_i,  u = sum_i w_i P[j] / S
 * and g = gU[q] (float64 Q x C, dL/dUq):
 *   r_i = sum_c g_c (P[j, c] - u_c)        beta_i = w_i r_i / S        a_i = w_i / S
 *   c_i = -4 beta_i / (e_q e_j)            'auto': c_(kn-1) += (sum_i beta_i t_i) / (2 d_(kn-1))
 *   gXq[q]   =  2 sum_i c_i (x_q - x_j)
 *   gXdb[j]  = -2 sum_{(q, i): idx[q, i] = j} c_i (x_q - x_j)
 *   gP[j, c] =    sum_{(q, i): idx[q, i] = j} a_i g[q, c]
 *   grad_eps =    sum_q sum_i 2 beta_i t_i / eps                          fixed eps only
 * eps_db is a constant of the fitted graph: it gets no gradient.  The differences x_q - x_j are
 * exact in float64; every product and sum is float64, rounded to nearest, in a fixed order (list
 * order within a query row, ascending query within a database row, ascending row for grad_eps);
 * u is recomputed with gll_extend's operations, so it has gll_extend's bits; each output is
 * rounded once to fp32 (grad_eps stays float64).  No floating-point atomics: two runs are bitwise
 * equal, gXq[q] does not depend on the other rows of the call, and the bits do not depend on
 * `what`, `flags` or the alignment.  IEEE as written (no clamps): a row whose weight sum is zero
 * or NaN has a NaN gXq row and makes the database rows it lists NaN (and grad_eps), every other
 * row is unaffected.  An index outside [0, N) is not followed: the entry contributes to no
 * database row and its query row's gradients are NaN.
 * `what`: GLL_EG_* bits, at least one; gXq: Q x d, gXdb: N x d, gP: N x C fp32, grad_eps: one
 * float64; an output not selected may be NULL.  GLL_EG_EPS with eps <= 0 ('auto') is
 * GLL_ERR_INVALID_ARG.  status (4 device words, accumulate, the caller zeroes them): [2] query
 * rows with a zero or NaN weight sum; [3] database rows whose list did not fit the in-LDS
 * capacity (512 entries; GLL_EGF_SMALL_LISTS: 64) and was ordered in global memory, diagnostic;
 * [0], [1] unused.  workspace: gll_extend_grad_workspace_bytes bytes, 16-B aligned (0 for
 * arguments out of range).  Launches: 1 (the row kernel) + 4 when GLL_EG_XDB or GLL_EG_P is
 * selected (count, scan, fill, database rows) + 1 with GLL_EG_EPS; counted by
 * gll_extend_grad_launches alone.  Xq, Xdb need 4-B alignment only (16-B loads where d % 4 == 0
 * and both are 16-B aligned, scalar loads of the same elements otherwise).  1 <= kn, C <= 256,
 * 1 <= d <= 4096, N, Q <= INT32_MAX / 2 (GLL_ERR_UNSUPPORTED past them).  Stream-ordered, no
 * allocation, no host synchronisation; argument checks come before any HIP call. */
#define GLL_EG_XQ 1
#define GLL_EG_XDB 2
#define GLL_EG_P 4
#define GLL_EG_EPS 8
#define GLL_EGF_SMALL_LISTS 1   /* tests: shrink the in-LDS list capacity to 64 entries */
size_t gll_extend_grad_workspace_bytes(int64_t Q, int64_t N, int32_t kn, int32_t d, int32_t C,
                                       int what, int flags);
int gll_extend_backward(int64_t Q, int64_t N, int32_t kn, int32_t d, int32_t C,
                        const float* Xq, const float* Xdb, const int32_t* idx, const float* d2,
                        const float* P, const float* eps_db, float eps, const double* gU,
                        int what, int flags,
                        float* gXq, float* gXdb, float* gP, double* grad_eps,
                        int32_t* status, void* workspace, void* stream);
int64_t gll_extend_grad_launches(void);  /* kernel launches of gll_extend_backward so far in this process (host counter) */

/* The layer on caller-supplied neighbour lists (ingest.hip).  The reference defines
 * every stage after the neighbour search on an arbitrary knn_ind (GLL.py:186-205: the symmetrisation
 * by the larger directed distance, eps_i = the distance to the entry in the last column, then the
 * weights, the Laplacian and both solves); these entry points start there.  p->flags must hold
 * GLL_FLAG_KNN_GIVEN (and gll_forward* / gll_graph refuse it), so the workspace has no n x n term.
 * nbr: B x n x (K - 1) int32 device memory, K = min(p->K, n): for every row the OTHER rows, in the
 * caller's order, which is kept -- column K - 2 is the reference's knn_ind[:, -1], the 'auto'
 * eps_i and the kth-neighbour term of the gradient come from it.  Per row, one wave:
 *   d2_ij = sum_f (x_if - x_jf)^2 in float64 over the fp32 features, rounded once to fp32 (the wide
 *           select's and gll_knn_query's contract; bitwise symmetric in (i, j))
 *   dropped and counted in GLL_ST_LIST_DROPPED: an index outside [0, n); a repeat of an earlier
 *           entry of the row (the reference would sum a duplicate's distance in coo -> csr)
 *   dropped silently: the row itself, d2 = 0 (a duplicated point), a non-finite d2 -- as the
 *           search drops them and sparse.find does (GLL.py:198)
 *   kept entries stay in the caller's order at the front of knn_idx / knn_d2 row i (column 0 is
 *   (i, 0), the self slot), the tail is padded with (i, 0) as the search pads a row with fewer
 *   valid candidates; eps_i = p->eps, or for 'auto' sqrtf(knn_d2[i][K - 1]) -- a padded last
 *   column gives 0 and GLL_ST_TINY_EPS (GLL.py:240-241).
 * Then the row build and, for the forward, the Luu solve, exactly as after a search: launches =
 * one reset, the ingest, the row build (+ the CG).  Everything downstream (gll_backward_batched,
 * gll_param_grad_batched, the three heads, gll_workspace_view) takes the same problem and workspace.
 * No floating-point atomics; knn_idx, knn_d2 and eps are bitwise reproducible, and so is everything
 * after them (the row build sorts each row by column).  Any list is accepted -- e.g. one column
 * named by every row: a row's reverse entries past RCAP go through the overflow list, rows longer
 * than a slot through the bump region, whose sizes (n (K - 1) triples, 2 n (K - 1) entries) bound any
 * list.  nbr == NULL is GLL_ERR_INVALID_ARG before any GPU call.  gll_graph_lists needs base == 0. */
int gll_forward_lists_batched(const gll_problem* p, int B, const float* X, const int32_t* nbr,
                              const void* Y, int y_dtype, void* workspace, double* U, void* stream);
int gll_graph_lists(const gll_problem* p, const float* X, const int32_t* nbr, void* workspace,
                    void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GLL_H */
