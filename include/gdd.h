/*
 * gdd.h — C ABI of libgdd, the MI355X-native (gfx950) hot path of ClustGDD graph distillation.
 *
 * The reference (Tyler-Linchenwei/Graph-Distillation-for-Recommendation, ClustGDD/) has no FFI layer:
 * its hot path is inline Python inside ClustGDD.pretrained_clustering and distill_recsys.kmeans_cluster.
 * Each entry point below replaces one of those call sites; the cited file:line is the reference code
 * whose arithmetic the entry point restates (paths relative to the reference's ClustGDD/ directory,
 * or to scikit-learn 1.7.2 for the k-means internals the reference calls).
 *
 * Conventions (all entry points):
 *   - every array argument is a DEVICE pointer, caller-owned (PyTorch allocates), row-major, dense;
 *   - work is enqueued on `stream` (the caller's torch.cuda.current_stream()); no entry point
 *     synchronises the host except where its comment says so;
 *   - the library keeps no device memory and no global mutable state; scratch comes from a caller
 *     workspace sized by the matching *_ws_bytes() query;
 *   - return 0 on success, otherwise a GDD_E_* code or a hipError_t value; gdd_last_error() gives a
 *     thread-local message. Shapes are validated on the host before any launch.
 */
#ifndef GDD_H_
#define GDD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* gdd_stream_t; /* == hipStream_t */

#define GDD_OK 0
#define GDD_E_INVALID 0x10001   /* bad shape / null pointer / unsupported parameter */
#define GDD_E_WORKSPACE 0x10002 /* workspace too small */
#define GDD_E_NODEVICE 0x10003  /* no gfx950 device visible */

/* ---------------------------------------------------------------------------------------------- */
/* Library                                                                                          */
/* ---------------------------------------------------------------------------------------------- */
const char* gdd_last_error(void);
int gdd_abi_version(void); /* bumps on any signature change */
/* The bound of the library's LDS arrival-counter spins (1 << 16; 0 in the `make SPIN0=1` twin
   whose every bounded wait gives up, so that the redo paths run — tests/test_gpu_spin0.py). */
int gdd_spin_limit(void);
/* 1 if the current HIP device is gfx950 and the embedded code objects can run on it. */
int gdd_device_ok(void);
/* Streaming device copy (16-byte aligned, bytes % 16 == 0): the bench's measured HBM copy peak     */
/* (SURVEY §8(d) roofline: "measure the achievable peak on the box with a copy kernel").           */
int gdd_stream_copy(const void* src, void* dst, size_t bytes, gdd_stream_t stream);

/* ---------------------------------------------------------------------------------------------- */
/* (a2) normalisation:  Â = D^-1/2 (A + I) D^-1/2                                                   */
/* Replaces deep_robust_utils.normalize_adj_tensor(adj, sparse=True)  (deep_robust_utils.py:245-256)  */
/*   -> to_scipy (:408-417) -> normalize_adj (:180-207) -> sparse_mx_to_torch_sparse_tensor (:389-396) */
/* Input: canonical CSR of A (rows ascending, columns strictly ascending per row, no duplicates);    */
/*   val == NULL means every stored value is 1.0f (binary adjacency).                               */
/* self_loops: -1 = reference rule (add I iff A[0,0] == 0, deep_robust_utils.py:199-200),            */
/*              0 = never, 1 = always.                                                              */
/* When I is added the row sums, r = rowsum^-1/2 (inf -> 0) and both scalings are done in fp64 and    */
/* the result is rounded to fp32 (sp.eye promotes the matrix to float64); otherwise in fp32.         */
/* Output: canonical CSR; entries whose scaled value is exactly 0 are dropped (scipy csr_matmat       */
/* drops them). col_out / val_out must hold nnz + n entries; rowptr_out[n] receives nnz_out.         */
/* ---------------------------------------------------------------------------------------------- */
size_t gdd_normalize_ws_bytes(int64_t n, int64_t nnz);
int gdd_normalize_csr(int64_t n, int64_t nnz, const int32_t* rowptr, const int32_t* col,
                      const float* val, int self_loops, int32_t* rowptr_out, int32_t* col_out,
                      float* val_out, void* ws, size_t ws_bytes, gdd_stream_t stream);

/* ---------------------------------------------------------------------------------------------- */
/* (a3) feature propagation                                                                         */
/* Replaces the loop clustgdd_agent_transduct.py:59-65 (and clustgdd_agent_induct.py:72-94):          */
/*   t = 0:      p = X,                 target = fp32(1-alpha) * X                                   */
/*   t = 1..T-1: p = (fp32(alpha) * Â) @ p,  target = target + fp32(1-alpha) * p                    */
/* Canonical summation order of one output row: its stored entries in CSR order are cut into         */
/* segments of GDD_PROP_SEG entries; each segment is an fp32 fma chain from +0 in entry order; the   */
/* segment partials are added left to right. `p_last` receives p after the last hop (X if T == 1).   */
/* X, target, p_last, p_tmp: n x d fp32; p_tmp is scratch (may alias nothing else).                  */
/* ---------------------------------------------------------------------------------------------- */
#define GDD_PROP_SEG 256
size_t gdd_propagate_ws_bytes(int64_t n, int64_t nnz, int d);
/* r06: from 1M rows a one-workgroup probe samples the CSR; where half the sampled entries point within */
/* 4,096 rows of their row (ids that carry locality) the hops walk the rows in order, else longest     */
/* rows first — a schedule only, the results are the same bits.                                       */
int gdd_propagate(int64_t n, int64_t nnz, const int32_t* rowptr, const int32_t* col, const float* val,
                  int d, const float* X, int T, float alpha, float* target, float* p_last,
                  float* p_tmp, void* ws, size_t ws_bytes, gdd_stream_t stream);
/* The same propagation with the intermediate hops in a relabelled node order (r05):  */
/* rho (device, a permutation of [0, n)) gives node r's row of the intermediate p at rho[r] and the   */
/* gathers after the first go through rho[col]; every row keeps its entries in CSR order, so target  */
/* and p_last (both by the original ids: the first hop reads X by them, the last hop stores by them)  */
/* are bit-identical to gdd_propagate's. A locality order (hubs first, RCM, communities) lets the    */
/* gathered rows of a hop share cache lines and pages; no separate permutation pass. r06: every hop's */
/* work list walks the rows in the new order (consecutive items gather neighbouring rows). rho is not */
/* checked on the device: a non-permutation writes out of bounds (gdd.propagate checks it on the host).*/
size_t gdd_propagate_relabeled_ws_bytes(int64_t n, int64_t nnz, int d);
int gdd_propagate_relabeled(int64_t n, int64_t nnz, const int32_t* rowptr, const int32_t* col,
                            const float* val, const int32_t* rho, int d, const float* X, int T,
                            float alpha, float* target, float* p_last, float* p_tmp, void* ws,
                            size_t ws_bytes, gdd_stream_t stream);
/* A community node order for that rho: deterministic synchronous label propagation over the CSR     */
/* structure (values ignored), CAP = 256. deg[v] = rowptr[v+1] - rowptr[v]; labels start as lab[v] = */
/* v. A sweep reads the previous sweep's labels and writes a second buffer: row r collects one vote  */
/* for lab[r] itself (whether or not the diagonal is stored) and one vote for lab[c] of each of its  */
/* first min(deg[r], CAP) stored entries c with c != r and deg[c] <= CAP (an entry that points at a  */
/* hub casts no vote); its new label is the one with the most votes, among equals the smallest. All  */
/* counts are integers: no rounding, no dependence on scheduling. After `sweeps` sweeps, order = the */
/* nodes sorted by (final label, node id) and rho[order[j]] = j. A sweep that changes nothing is a   */
/* fixed point: the sweeps after it are skipped on the device (same answer, no host round trip).     */
/* labels (nullable, n): the final labels. changed (nullable, int32[sweeps]): labels changed per     */
/* sweep; skipped sweeps write 0. n = 0 and nnz = 0 are valid (the identity). n < 0, nnz < 0,        */
/* sweeps < 0 and a short workspace are rejected on the host. A rowptr pair outside [0, nnz] makes   */
/* its row empty and an out-of-range column casts no vote; neither is dereferenced, both set a flag  */
/* the call reads back (one stream synchronise at its end) and reports as GDD_E_INVALID.             */
size_t gdd_community_order_ws_bytes(int64_t n, int64_t nnz);
int gdd_community_order(int64_t n, int64_t nnz, const int32_t* rowptr, const int32_t* col, int sweeps,
                        int32_t* rho, int32_t* labels, int32_t* changed, void* ws, size_t ws_bytes,
                        gdd_stream_t stream);
/* one hop: y = (scale * Â) @ x with the canonical order above; if acc != NULL also                   */
/*   acc = acc + acc_scale * y  (two fp32 roundings, no contraction).                               */
int gdd_spmm(int64_t n, int64_t nnz, const int32_t* rowptr, const int32_t* col, const float* val,
             int d, float scale, const float* x, float* y, float* acc, float acc_scale, void* ws,
             size_t ws_bytes, gdd_stream_t stream);
/* The same hop split in two: gdd_spmm_plan builds the row-segment work list of a CSR structure in  */
/* ws (gdd_propagate_ws_bytes(n, nnz, d)); gdd_spmm_planned then runs hops against it without      */
/* rebuilding it (one k_hop + one fix-up launch per call) — the unit the bench times per launch.     */
int gdd_spmm_plan(int64_t n, int64_t nnz, const int32_t* rowptr, int d, void* ws, size_t ws_bytes,
                  gdd_stream_t stream);
int gdd_spmm_planned(int64_t n, int64_t nnz, const int32_t* rowptr, const int32_t* col,
                     const float* val, int d, float scale, const float* x, float* y, float* acc,
                     float acc_scale, const void* ws, size_t ws_bytes, gdd_stream_t stream);
/* The hop kernel's form for feature width d and the common alignment of a hop's buffers in bytes    */
/* (16, 8 or 4; x, y, acc and the propagation's internal rows), host only: "v<V>/g<G>/s<S>" with V   */
/* floats per lane (4, 2, 1), G lanes per work item (16, 32, 64) and S feature slices mapped onto the */
/* XCDs (8, 4, 2, 1; 0 = a two-dimensional grid over items and feature chunks). Every form computes   */
/* the same bits. "invalid" for d <= 0 or another align. The string is the calling thread's until its */
/* next call.                                                                                         */
const char* gdd_hop_path(int d, int align);

/* ---------------------------------------------------------------------------------------------- */
/* (a5/a6/a8) k-means building blocks (scikit-learn 1.7.2 semantics, fp32 data)                      */
/* Replace MiniBatchKMeans/KMeans(...).fit at clustgdd_agent_transduct.py:102-105,                    */
/* clustgdd_agent_induct.py:131-134, distill_recsys.py:174-180. Loop control and the MT19937 draws    */
/* stay on the host (numpy RandomState is the reference's own RNG).                                 */
/* ---------------------------------------------------------------------------------------------- */

/* out[i] = sum_j X[i,j]^2 in numpy's einsum("ij,ij->i") float32 order (sklearn row_norms,           */
/* sklearn/utils/extmath.py:76): 4 lanes, 16-element blocks fed in reverse vector order, mul+add     */
/* (no fma), lanes reduced (l0+l1)+(l2+l3). Bit-exact with numpy on x86-64 SSE3 builds.              */
int gdd_row_norms(int64_t n, int dim, const float* X, float* out, gdd_stream_t stream);

/* Assignment (E-step) of sklearn _update_chunk_dense (sklearn/cluster/_k_means_lloyd.pyx:172-213):  */
/*   d[i,j] = fma(-2, sum_t X[i,t]*C[j,t] as a t-ordered fp32 fma chain, c_norm2[j])                */
/*   labels[i] = first j with minimal d  (strict <, lowest index wins)                              */
/* computed with v_mfma_f32_32x32x2_f32 (exact k-ordered fma chain = OpenBLAS sgemm, bit-exact).     */
/* rows == NULL: rows are 0..n-1; otherwise row i of the batch is X[rows[i]] (minibatch gather).     */
/* sq_dist (nullable): per-sample ||x - c_label||^2 in sklearn _euclidean_dense_dense order          */
/* (sklearn/cluster/_k_means_common.pyx:26-48: 4-term groups, mul+add, no fma).                      */
/* dim <= 512. Workspace: gdd_kmeans_assign_ws_bytes(n) (one 64-bit key per sample).              */
size_t gdd_kmeans_assign_ws_bytes(int64_t n);
int gdd_kmeans_assign(int64_t n, int dim, const float* X, const int64_t* rows, int k,
                      const float* C, const float* c_norm2, int32_t* labels, float* sq_dist,
                      void* ws, size_t ws_bytes, gdd_stream_t stream);
/* bf16 distance variant (configs 2, 3, 5 carry fp32 and bf16 distances). Same        */
/* arguments and outputs; the X and C operands are rounded to bf16 (nearest even) and the dot       */
/* products run as v_mfma_f32_32x32x16_bf16 chains with fp32 accumulation; distances use the fp32    */
/* c_norm2 (NULL: computed on the device, no separate launch on the common shapes).                  */
/* Guaranteed: labels[i] is the nearest centre under exact products of the bf16-rounded operands     */
/* with the fp32 c_norm2, i.e. it minimises c_norm2[j] / 2 - sum_t bf16(X[i,t]) bf16(C[j,t]), up to   */
/* the fp32 accumulation (~2^-17 of the terms' magnitudes; tests/bf16_model.py derives the bound,     */
/* tests/test_gpu_bf16_labels.py checks it on every kernel form). Where centres tie within that, the  */
/* r03 and tiles forms return the first, the r06 form any of them. NOT bit-compatible with sklearn:   */
/* the distance to the fp32 answer is the operands' rounding, a label may differ where two centres'   */
/* fp32 distances lie within ~2^-7 ||x|| ||c|| of each other. sq_dist is the exact fp32 distance      */
/* (_euclidean_dense_dense order) to the chosen centre. dim <= 512 (497 .. 512: two-wave blocks).     */
int gdd_kmeans_assign_bf16(int64_t n, int dim, const float* X, const int64_t* rows, int k,
                           const float* C, const float* c_norm2, int32_t* labels, float* sq_dist,
                           void* ws, size_t ws_bytes, gdd_stream_t stream);
/* the launch path a labels pass takes under the current GDD_FORCE, by name (host only, no device   */
/* call), for the workspace gdd_kmeans_assign_ws_bytes(n). flags say what the pointers would:        */
#define GDD_ASSIGN_ROWS 1        /* a row list is given                                              */
#define GDD_ASSIGN_X_UNALIGNED 2 /* X is not 16-byte aligned                                         */
#define GDD_ASSIGN_C_UNALIGNED 4 /* C is not 16-byte aligned                                         */
#define GDD_ASSIGN_BF16 8        /* gdd_kmeans_assign_bf16                                           */
#define GDD_ASSIGN_TOP2 16       /* the Lloyd loop's bounded E-step (best and second-best distance)  */
#define GDD_ASSIGN_PADDED 32     /* ... with the zero-padded copy of X offered for its row lists     */
/* small/w<waves>/vec|scalar, waves[_top2]/w<waves>/contig|rows|row4/<chunk>x<chunks>[/prefill],      */
/* persist/<chunk>x<chunks>[/prefill], tiles/w<waves>/vec|scalar/<chunk>x<chunks>/prefill,            */
/* bf16q/w<waves>, bf16p/per<loads>, bf16_tiles/<chunk>x<chunks>/prefill; "invalid" for a shape the   */
/* entry point refuses (and for n = 0, which launches nothing). The string is the calling thread's    */
/* until its next call.                                                                               */
const char* gdd_kmeans_assign_path(int64_t n, int dim, int k, int flags);

/* out[0] = sequential fp32 sum of sq_dist[i] * w[i] in sample order (w == NULL: ones); this is      */
/* sklearn _inertia_dense with one OpenMP thread (_k_means_common.pyx:92-121).                       */
/* Evaluated in parallel with the sequential result bit for bit (gdd_seqsum.hip: per-binade integer   */
/* advances with a round-to-even parity carry, scanned by one workgroup). Non-negative finite terms   */
/* take the parallel form; NaN, infinite or negative terms are added one at a time from there.       */
int gdd_inertia(int64_t n, const float* sq_dist, const float* w, float* out, gdd_stream_t stream);
/* The same sum for long arrays in three launches over ~2048-term segments (per-segment advances for  */
/* the two likeliest binades, then one resolving workgroup); ws: gdd_inertia_ws_bytes(n) bytes.       */
size_t gdd_inertia_ws_bytes(int64_t n);
int gdd_inertia_ws(int64_t n, const float* sq_dist, const float* w, float* out, void* ws,
                   size_t ws_bytes, gdd_stream_t stream);

/* MiniBatchKMeans center update, sklearn _minibatch_update_dense (_k_means_minibatch.pyx:11-108):    */
/* for each cluster c with batch weight ws > 0: C_new[c] = (C_old[c]*W[c] + sum_{i in c, batch order} */
/* X_i*w_i) * fp32(1/(W[c]+ws)), W[c] += ws; otherwise C_new[c] = C_old[c].                        */
size_t gdd_minibatch_update_ws_bytes(int64_t b, int k);
int gdd_minibatch_update(int64_t b, int dim, const float* X, const int64_t* rows, const float* w,
                         const int32_t* labels, int k, const float* C_old, float* C_new,
                         float* weight_sums, void* ws, size_t ws_bytes, gdd_stream_t stream);

/* One MiniBatchKMeans step on the device: sklearn _mini_batch_step without the reassignment        */
/* branch (_kmeans.py:1556-1638) — ||C_old||^2, MFMA assignment of the gathered batch X[rows],       */
/* sequential batch inertia, centre update into C_new — followed, with GDD_STEP_CONVERGE, by         */
/* _mini_batch_convergence (:1960-2027, EWA of inertia/b in unfused fp64, max_no_improvement; -1 =   */
/* None; the test reads only the batch inertia, so it may precede the host's reassignment).          */
/* `state` (gdd_minibatch_state_bytes(), zero-initialised) carries the EWA state and, as an int32 at */
/* offset 16, stop_at = 0 while running or s+1 once the test fired at step s: every kernel of a      */
/* later step is then a no-op, so the host may enqueue steps ahead of the decision. Each step leaves */
/* ||C_new||^2 in the workspace; pass GDD_STEP_NORMS_VALID when C_old is the previous step's C_new  */
/* (unmodified by the host) to reuse them. batch b <= 13312.                                         */
#define GDD_STEP_CONVERGE 1
#define GDD_STEP_NORMS_VALID 2
size_t gdd_minibatch_state_bytes(void);
size_t gdd_minibatch_step_ws_bytes(int64_t b, int k);
int gdd_minibatch_step(int64_t b, int dim, const float* X, const int64_t* rows, int k,
                       const float* C_old, float* C_new, float* weight_sums, int32_t* labels,
                       int step_i, int64_t n_samples, int max_no_improvement, int flags,
                       void* state, void* ws, size_t ws_bytes, gdd_stream_t stream);
int gdd_minibatch_converge(int64_t b, int k, int step_i, int64_t n_samples, int max_no_improvement,
                           void* state, void* ws, size_t ws_bytes, gdd_stream_t stream);
/* The form a step's launches take, by name (host only, no device call): w<waves per assignment block:  */
/* 4, 2 or 1 by the LDS a dim needs>/vec|scalar (16-byte loads: dim % 4 == 0 and aligned X and C)/       */
/* g<centre-tile groups>xp<32-point groups> (the assignment's grid); "invalid" for a shape the step      */
/* refuses (b > 13312, dim > 512, a size <= 0). The string is the calling thread's until its next call.   */
#define GDD_STEP_PATH_UNALIGNED 1 /* X or C is not 16-byte aligned                                       */
const char* gdd_minibatch_step_path(int64_t b, int dim, int k, int flags);

/* numpy legacy RandomState state: ('MT19937', key[624], pos, has_gauss, cached_gaussian).          */
typedef struct gdd_mt_state {
  uint32_t key[624];
  int32_t pos;
  int32_t has_gauss;
  double gauss;
} gdd_mt_state;

/* MiniBatchKMeans(n_clusters=k, batch_size, max_iter, max_no_improvement (-1 = None),              */
/* reassignment_ratio, init_size, n_init).fit(X) in one call (sklearn/cluster/_kmeans.py:2046-2200):  */
/* validation/init subsets, k-means++ seeding, the step loop with reassignment and early stopping,   */
/* and (compute_labels) the final labels pass + inertia. `rng` is the caller's RandomState, advanced */
/* exactly as scikit-learn advances it. argsort_cb must reproduce np.argsort(weight_sums); it is    */
/* only called when more than batch/2 centres are due for reassignment (possible only if k > b/2).   */
/* Host syncs: the step loop is device-resident (draws, reassignments and the convergence test run   */
/* there), so the host waits once per 16-step chunk, for the chunk before the one just enqueued, and  */
/* once at the end; only a step whose reassignment needs np.argsort (more than batch/2 centres due)   */
/* and the steps after it while a weight sum is zero run host-driven, with one sync per reassignment. */
/* centers_out k x dim, labels_out n,                                                                */
/* inertia_out (device): compute_labels 1 -> 1 float, the inertia; compute_labels 2 -> n floats, the  */
/* per-sample squared distances (the caller folds them, e.g. on a side stream); n_steps_out, ewa_out  */
/* (nullable) host.                                                                                  */
size_t gdd_minibatch_kmeans_fit_ws_bytes(int64_t n, int dim, int k, int64_t batch_size,
                                         int64_t init_size);
int gdd_minibatch_kmeans_fit(int64_t n, int dim, const float* X, int k, int64_t batch_size,
                             int max_iter, int max_no_improvement, float reassignment_ratio,
                             int64_t init_size, int n_init, int compute_labels, void* rng,
                             void (*argsort_cb)(const float*, int64_t, int64_t*), float* centers_out,
                             int32_t* labels_out, float* inertia_out, int64_t* n_steps_out,
                             double* ewa_out, void* ws, size_t ws_bytes, void* host_ws,
                             size_t host_ws_bytes, gdd_stream_t stream);
/* pinned host staging the fit needs (host_ws: page-locked, caller-owned, e.g. a pinned torch tensor) */
size_t gdd_minibatch_kmeans_fit_host_ws_bytes(int64_t n, int k, int64_t batch_size, int64_t init_size);
/* The loop a fit takes, by name (host only, no device call): dev/par or dev/chain, the device-resident */
/* loop with the reassignment kernel's parallel row copies or, where their index tables do not fit    */
/* the LDS, one copy chain per reassigned cluster; host, the host-driven loop (GDD_HOST_LOOP set, or   */
/* the reassignment's swap table exceeds the LDS); "invalid" for a shape the fit refuses.              */
const char* gdd_minibatch_fit_path(int64_t n, int dim, int k, int64_t batch_size);
/* The device loop's schedule of steps [i0, i0 + m) of a segment that starts at step i0 (host only; for */
/* tests): rr_base the last reassignment step, norms_valid0 whether the workspace norms match step     */
/* i0's centres. out[j] describes step i0 + j: GDD_SCHED_* bits, then the indices of its C_old (bit 4), */
/* its rows buffer (bit 5) and its generator slot (bits 6-7).                                          */
#define GDD_SCHED_REASSIGN 1    /* the reassignment launch follows the update                          */
#define GDD_SCHED_HAS_NEXT 2    /* the step draws the next batch                                       */
#define GDD_SCHED_NORMS_VALID 4 /* GDD_STEP_NORMS_VALID                                                */
#define GDD_SCHED_NO_TAIL 8     /* no tail for the step before (the host ran its convergence test)     */
int gdd_minibatch_schedule(int64_t i0, int64_t rr_base, int norms_valid0, int64_t n_steps, int k,
                           int64_t batch_size, float reassignment_ratio, int64_t m, int32_t* out);
/* The host loop's reassignment decision (_mini_batch_step's branch, numpy float32 semantics; host    */
/* only, for tests): weight_sums k floats, rng a gdd_mt_state advanced as numpy advances it. pairs     */
/* (2k int64) receives (cluster, batch position) per reassigned centre and *n_pairs their count;        */
/* weight_sums_out the sums after the fill; *any_zero whether one of them is zero.                      */
int gdd_minibatch_reassign_host(const float* weight_sums, int k, int64_t batch_size,
                                float reassignment_ratio, void* rng,
                                void (*argsort_cb)(const float*, int64_t, int64_t*), int64_t* pairs,
                                int64_t* n_pairs, float* weight_sums_out, int* any_zero);

/* Host-only numpy-legacy draws used by the native loops (exposed for parity tests):                */
/* randint(low, high, count) (int64), random_sample(count), permutation(n), and                      */
/* choice(n, p=w/w.sum()) for unit fp32 weights. `state` is a gdd_mt_state, advanced in place.       */
int gdd_rng_randint(void* state, int64_t low, int64_t high, int64_t count, int64_t* out);
int gdd_rng_random_sample(void* state, int64_t count, double* out);
int gdd_rng_permutation(void* state, int64_t n, int64_t* out);
int gdd_rng_choice_unit_weights(void* state, int64_t n, int64_t* out);

/* Stable grouping of samples by label: perm[offsets[c] .. offsets[c+1]) lists the samples of        */
/* cluster c in ascending sample order; counts[c] = offsets[c+1]-offsets[c]. Labels outside [0, k)    */
/* belong to no cluster (offsets[k] counts the others), as in the reference's `labels == i` loop.     */
size_t gdd_group_ws_bytes(int64_t n, int k);
int gdd_group_by_label(int64_t n, const int32_t* labels, int k, int32_t* perm, int32_t* offsets,
                       void* ws, size_t ws_bytes, gdd_stream_t stream);
/* the form that grouping takes under the current GDD_FORCE, by name (host only, no device call):      */
/* small/m1|m2 (one workgroup, tiles of m x 1024 labels), count/m<m>/w<waves per block> (histograms,   */
/* scan, scatter), radix (a pair sort on the labels); "invalid" for a shape gdd_group_by_label refuses. The string   */
/* is the calling thread's until its next call.                                                        */
const char* gdd_group_path(int64_t n, int k);

/* Lloyd M-step accumulation, sklearn lloyd_iter_chunked_dense with one OpenMP thread                */
/* (_k_means_lloyd.pyx:111-160, 208-213): sums[c,:] = sequential fp32 sum over the samples of c in    */
/* sample order of X_i*w_i, wsum[c] = sequential fp32 sum of w_i.  Uses gdd_group_by_label output.    */
int gdd_segment_sum_f32(int64_t n, int dim, const float* X, const float* w, const int32_t* perm,
                        const int32_t* offsets, int k, float* sums, float* wsum, gdd_stream_t stream);

/* The same sums for clusters [c0, c1) only, written as a slice (row c - c0): the cluster-partitioned */
/* M-step of the multi-GPU Lloyd loop (gdd/sharded.py), bit-identical to the full call's rows.        */
int gdd_segment_sum_f32_part(int64_t n, int dim, const float* X, const float* w, const int32_t* perm,
                             const int32_t* offsets, int k, int c0, int c1, float* sums_part,
                             float* wsum_part, gdd_stream_t stream);

/* The kernel form an ordered fold takes, by name (host only, no device call): the Lloyd sums of n     */
/* rows in k clusters over dim columns of rows of ld floats (0: dim) — gdd_segment_sum_f32, the Lloyd  */
/* loop's M-step (over its zero-padded copy of X, dim % 4 != 0 from 65,536 rows on, dim is rounded up  */
/* to a multiple of 4), a column range of gdd_lloyd_mstep (dim = f1 - f0, ld = the full dim) — or with */
/* GDD_FOLD_MEAN the cluster means. flags say what the pointers would:                                 */
#define GDD_FOLD_WEIGHTED 1    /* sample weights are given                                             */
#define GDD_FOLD_MEAN 2        /* gdd_cluster_mean (fp64 chains); not with GDD_FOLD_WEIGHTED           */
#define GDD_FOLD_X_UNALIGNED 4 /* X (at its first folded column) is not 16-byte aligned                */
/* big_rows: clusters of at least that many members fold in 16-column slices where a chunk is wider    */
/* (0: none, what every entry point but the Lloyd loop passes; < 0: the Lloyd loop's own rule under    */
/* the current GDD_FORCE, 1.5 x n / k and at least 4096).                                              */
/* cm/<columns>x<rows per chunk>[/sliced<rows per chunk of a sliced cluster>] (column-major chunks),   */
/* seg/f32|mean/vec|scalar[/w][/small]/<column slices>x<rows per chunk>[/sliced<rows>] (row-major      */
/* chunks; w: weighted, small: 8 KiB chunks for clusters of at most 64 rows on average); "invalid" for */
/* n, dim or k below 1. The string is the calling thread's until its next call.                        */
const char* gdd_fold_path(int64_t n, int dim, int ld, int k, int flags, int big_rows);

/* sklearn _average_centers (_k_means_common.pyx:215-236): w>0: C[c,:] *= fp32(1.0/(double)w);       */
/* w==0: C[c,:] = C[argmax(w),:] (first maximum; averaged already iff argmax < c, sklearn's loop     */
/* order). Then center_shift[c] = sqrt(||C_new[c]-C_old[c]||^2) in the          */
/* _euclidean_dense_dense order (_center_shift :239-251).                                           */
int gdd_average_centers(int k, int dim, float* C_new, const float* wsum, const float* C_old,
                        float* center_shift, gdd_stream_t stream);

/* Per-sample squared distance to a given center: out[i] = ||X[i] - C[labels[i]]||^2 in the          */
/* _euclidean_dense_dense order; with the final labels this is the per-sample term of sklearn        */
/* _inertia_dense (_k_means_common.pyx:92-121) used after the last Lloyd iteration.                  */
int gdd_point_center_sqdist(int64_t n, int dim, const float* X, const int32_t* labels,
                            const float* C, float* out, gdd_stream_t stream);

/* Relocation input of _relocate_empty_clusters_dense (_k_means_common.pyx:124-164):               */
/* out[i] = ((X[i] - C[labels[i]])**2).sum() in numpy's pairwise order over the row (fp32).           */
int gdd_relocate_distances(int64_t n, int dim, const float* X, const int32_t* labels,
                           const float* C, float* out, gdd_stream_t stream);

/* The device-resident Lloyd loop of sklearn _kmeans_single_lloyd (sklearn/cluster/_kmeans.py:       */
/* 690-735), replacing the per-iteration host loop of the reference's KMeans.fit call sites          */
/* (clustgdd_agent_transduct.py:104-105, clustgdd_agent_induct.py:133-134, distill_recsys.py:178).   */
/* Iteration i reads centres C[i%2] (C0/C1) and writes C[(i+1)%2]: labels (MFMA assignment), the     */
/* ordered M-step, _average_centers, _center_shift, strict convergence (labels == labels_old), then */
/* sum(shift^2) <= tol. Runs iterations it0.. until a stop or max_iter; chunks of iterations are    */
/* enqueued ahead of the decision (later kernels no-op through `state`). Returns *out_reason:       */
/* 0 max_iter, 1 strict, 2 tol, 3 an empty cluster needs _relocate_empty_clusters at iteration      */
/* *out_done (the caller relocates on C[(i+1)%2]/wsum, then calls again with it0=i, resume=1).      */
/* Otherwise *out_done = iterations completed. labels_old starts as -1 (the caller fills it).      */
/* state: gdd_lloyd_state_bytes() of device memory; host_ws: pinned, gdd_kmeans_lloyd_host_ws_bytes. */
/* For dim <= 48 with every centre in one LDS chunk, the E-step is bounded: a row whose Hamerly      */
/* bounds, widened by the fp32 rounding margin, prove sklearn's argmin keeps its label skips the     */
/* distance pass (labels identical; the workspace holds the bounds; GDD_LLOYD_PRUNE=0 disables).     */
/* The state's layout (64 bytes, int32 words; the phase entry points below share it). Iteration i    */
/* runs as steps 2i (E-step, sums, empty-cluster check) and 2i+1 (average, shift, convergence):      */
/*   offset  0  stop_at  0 while running, s+1 once step s stopped: every later step's kernels no-op  */
/*   offset  4  reason   0 running / max_iter, 1 strict, 2 tol, 3 an empty cluster needs relocation  */
/*   offset  8  iter     the iteration the reason refers to                                          */
/*   offset 12  changed  labels changed in the current iteration (kept across a relocation's resume) */
/*   offset 16  done     iterations completed                                                        */
/*   offset 20  11 words of padding                                                                  */
/* A caller of the phase entry points zeroes stop_at, reason and iter before each run, and changed   */
/* too unless it resumes after a relocation (gdd._lib.LloydState mirrors the struct).                */
size_t gdd_lloyd_state_bytes(void);
size_t gdd_kmeans_lloyd_ws_bytes(int64_t n, int dim, int k);
size_t gdd_kmeans_lloyd_host_ws_bytes(void);
int gdd_kmeans_lloyd_run(int64_t n, int dim, const float* X, int k, float* C0, float* C1,
                         int32_t* labels, int32_t* labels_old, float* wsum, float* shift, int it0,
                         int resume, int max_iter, double tol, void* state, int32_t* out_done,
                         int32_t* out_reason, void* ws, size_t ws_bytes, void* host_ws,
                         size_t host_ws_bytes, gdd_stream_t stream);

/* One iteration of the same loop in three phases, for a process group over the GPUs of a node      */
/* (gdd.sharded.ShardedKMeans): rank r runs the E-step (bounded as above) on its rows [r0, r1) and   */
/* the ordered M-step fold on its feature columns [f0, f1) of every cluster; between the phases the  */
/* caller all-gathers the labels and the column slices (RCCL, stream-ordered), and every rank runs  */
/* the same update. ws: gdd_kmeans_lloyd_ws_bytes(n, dim, k), kept across iterations (it holds the   */
/* rows' bounds); state as above, its stop word gating every kernel (iteration `it` = steps 2it and */
/* 2it+1), so chunks of iterations can be enqueued ahead of the host's read of the state.           */
/* gdd_lloyd_estep: labels[r0:r1) for centres C (shift: the previous update's, unless `first` — the */
/* first E-step of a fit or after a relocation, which sets the rows' bounds).                        */
/* gdd_lloyd_mstep: groups the full labels, sums_cols = k x (f1-f0) column sums, wsum = k weights,    */
/* then the empty-cluster check (reason 3).                                                          */
/* gdd_lloyd_update: C_new = the column slices in `parts` (slot r of k*fw floats: rank r's columns   */
/* [r*fw, min(dim, (r+1)*fw)) as a row-major k x w_r block; parts NULL: C_new already holds the      */
/* sums), _average_centers,                                                                          */
/* _center_shift, the labels-changed flag and the convergence test.                                  */
int gdd_lloyd_estep(int64_t n, int64_t r0, int64_t r1, int dim, const float* X, int k, const float* C,
                    const float* shift, int first, int32_t* labels, void* state, int it, void* ws,
                    size_t ws_bytes, gdd_stream_t stream);
int gdd_lloyd_mstep(int64_t n, int dim, const float* X, const int32_t* labels, int k, int f0, int f1,
                    float* sums_cols, float* wsum, void* state, int it, void* ws, size_t ws_bytes,
                    gdd_stream_t stream);
int gdd_lloyd_update(int64_t n, int dim, int k, const float* parts, int fw, float* C_new,
                     const float* wsum, const float* C_old, float* shift, const int32_t* labels,
                     int32_t* labels_old, double tol, void* state, int it, gdd_stream_t stream);

/* The order-free M-step of the same phase loop (gdd.sharded.ShardedKMeans(mstep="reduce")): int64   */
/* fixed-point partial sums, exact and associative, so the result is bit-identical for any number of */
/* ranks, any row split and any reduction order; it does NOT keep scikit-learn's ordered fp32 chain. */
/* Exponents (gdd_lloyd_reduce_exponents, once per fit, on the centred input Xc of n_total rows):     */
/*   L = bit_length(n_total - 1); E_f = frexp exponent of max_i |Xc[i,f]|; exps[f] = 62 - L - E_f,    */
/*   or 0 for an all-zero column. Then |sum q| <= 2^62 for any labelling: nothing can overflow.       */
/* Quantise: q[i,f] = rint(ldexp((double)Xc[i,f], exps[f])) as int64, round-half-even.                */
/* Buffer (int64, gdd_lloyd_reduce_words(dim, k) = k*dim + k + 1 words): [0, k*dim) the row-major     */
/*   k x dim sums of q, [k*dim, k*dim + k) the member counts, then 1 word: the rows whose label       */
/*   differs from labels_old.                                                                         */
/* gdd_lloyd_reduce_local (step 2*it): zeroes buf (always, also past a stop), then for this rank's    */
/*   rows [r0, r1) (r0 == r1 allowed) writes its sums, counts and changed count into buf and sets     */
/*   labels_old[i] = labels[i] on those rows. labels/labels_old are the full n-row arrays.            */
/*   ws: gdd_lloyd_reduce_ws_bytes(n, dim, k). The caller then SUM-all-reduces buf over the ranks.    */
/* gdd_lloyd_reduce_update (step 2*it + 1), on the reduced buf: C_new[c,f] = ldexpf((float)S[c,f],    */
/*   -exps[f]) (one round-to-nearest int64 -> fp32 conversion, then an exact scaling), wsum[c] =      */
/*   (float)count[c] (a conversion of the exact integer count: unlike the ordered M-step's fp32       */
/*   count, it does not stick at 2^24), the labels-changed flag = (changed word != 0); a cluster with */
/*   count 0 stops the loop there with reason 3 (C_new holds the sums, wsum the counts, the flag      */
/*   stays in the state). Otherwise _average_centers, _center_shift and the convergence test exactly  */
/*   as gdd_lloyd_update. from_cnew != 0 (the resume after a relocation): buf is not read, C_new      */
/*   already holds the relocated sums.                                                                */
size_t gdd_lloyd_reduce_words(int dim, int k);
size_t gdd_lloyd_reduce_ws_bytes(int64_t n, int dim, int k);
int gdd_lloyd_reduce_exponents(int64_t n, int dim, const float* X, int32_t* exps, gdd_stream_t stream);
int gdd_lloyd_reduce_local(int64_t n, int64_t r0, int64_t r1, int dim, const float* X,
                           const int32_t* labels, int32_t* labels_old, int k, const int32_t* exps,
                           int64_t* buf, void* state, int it, void* ws, size_t ws_bytes,
                           gdd_stream_t stream);
int gdd_lloyd_reduce_update(int dim, int k, const int64_t* buf, const int32_t* exps, int from_cnew,
                            float* C_new, float* wsum, const float* C_old, float* shift, double tol,
                            void* state, int it, gdd_stream_t stream);

/* ---------------------------------------------------------------------------------------------- */
/* Greedy k-means++ seeding, sklearn _kmeans_plusplus (sklearn/cluster/_kmeans.py:174-272) on the    */
/* device. Host supplies the reference RNG draws: first_id (random_state.choice) and                 */
/* uniforms[(k-1) * n_trials] (random_state.uniform(size=n_trials) per center, concatenated).        */
/* Distances: fp64 upcast -2<x_c,x> + |x_c|^2 + |x|^2, stored fp32, clipped at 0 (pairwise.py:582-650), */
/* in OpenBLAS's per-shape summation orders (gdd_skl_sqdist). Potentials: the first as sdot, the     */
/* trials' as sgemv_t (_kmeans.py:239-251). Writes centers (k x dim) and indices. 1 <= n_trials <= 16. */
/* ---------------------------------------------------------------------------------------------- */
size_t gdd_kmeans_plusplus_ws_bytes(int64_t n, int dim, int n_trials);  /* bound for every k <= n */
/* the workspace for this k: the n x n distance tables only where they are built (the multi-block  */
/* table when (k - 1) 2.5e7 >= n^2 dim, i.e. when the rounds it saves cover its one-off build)      */
size_t gdd_kmeans_plusplus_ws_bytes_k(int64_t n, int dim, int n_trials, int k);
/* the launch path this shape takes under the current GDD_FORCE, by name (host only, no device call): */
/* first_only, single_table_pair, single_table, single_fused/seq|blas, single_two_launch/seq|blas,    */
/* split, big_pair, big, block_table, block/seq|blas; "invalid" for a shape gdd_kmeans_plusplus       */
/* refuses. A static string.                                                                          */
const char* gdd_kmeans_plusplus_path(int64_t n, int dim, int n_trials, int k);
int gdd_kmeans_plusplus(int64_t n, int dim, const float* X, const float* w, int k, int n_trials,
                        int64_t first_id, const double* uniforms, float* centers, int64_t* indices,
                        void* ws, size_t ws_bytes, gdd_stream_t stream);

/* sklearn.metrics.pairwise._euclidean_distances(C, X, squared=True) for fp32 C (n_rows x dim) and X  */
/* (n x dim), as scikit-learn 1.7.2 computes it for k-means++ (_kmeans.py:229, 245): X in chunks of   */
/* batch_size rows upcast to fp64, numpy einsum norms, the OpenBLAS 0.3.29 SkylakeX summation order of */
/* each chunk's product, fp32, max(., 0). out: n_rows x n. Device pointers.                            */
int gdd_skl_sqdist(int n_rows, const float* C, int64_t n, int dim, const float* X, float* out,
                   gdd_stream_t stream);

/* ---------------------------------------------------------------------------------------------- */
/* (a8) StandardScaler(with_mean=True, with_std=True).fit_transform(X) on fp32 X                    */
/* Replaces the scaling step of distill_recsys.kmeans_cluster (distill_recsys.py:172), scikit-learn  */
/* 1.7.2 semantics (preprocessing/_data.py partial_fit/transform, utils/extmath.py                  */
/* _incremental_mean_and_var): fp64 column sums in row order, corrected two-pass variance,          */
/* near-constant columns scaled by 1, X_out = fp32(fp32(x - mean) / scale). mean/scale: dim doubles. */
/* ---------------------------------------------------------------------------------------------- */
int gdd_standard_scaler(int64_t n, int dim, const float* X, float* X_out, double* mean,
                        double* scale, gdd_stream_t stream);
/* KMeans.fit's centring (sklearn/cluster/_kmeans.py:1476-1487, _tolerance :279-288): mean = X.mean(0), */
/* var = X.var(0) (numpy: sequential fp32 column sums over the rows, quotient by n rounded to fp32), */
/* X_out = X - mean (fp32). mean/var: dim floats. X_out may not alias X.                           */
int gdd_center_columns(int64_t n, int dim, const float* X, float* X_out, float* mean, float* var,
                       gdd_stream_t stream);
/* The same with a workspace (r05): from 65,536 rows and 2 <= dim <= 256 the column chains run in the   */
/* exact parallel form (gdd_colsum.hip: per-segment transducers of the sequential fp32 sum, signed     */
/* terms); otherwise, or with GDD_CENTER_PAR=0, gdd_center_columns. Same bits either way.              */
size_t gdd_center_columns_ws_bytes(int64_t n, int dim);
int gdd_center_columns_ws(int64_t n, int dim, const float* X, float* X_out, float* mean, float* var,
                          void* ws, size_t ws_bytes, gdd_stream_t stream);
/* StandardScaler.transform with a fitted mean/scale (utils_graphsaint.py:41-44 fits on the train   */
/* rows and transforms every row): X_out = fp32(fp32(x - mean) / scale).                            */
int gdd_standard_scaler_transform(int64_t n, int dim, const float* X, const double* mean,
                                  const double* scale, float* X_out, gdd_stream_t stream);

/* ---------------------------------------------------------------------------------------------- */
/* (a7) cluster-feature mean. Replaces clustgdd_agent_transduct.py:116-127 (induct :143-154) and the  */
/* teacher index_add_/bincount means of distill_recsys.py:623-636.                                   */
/* feat_syn[c,:] = fp32( (sequential fp64 sum over members of c in sample order) / count_c );         */
/* count_c == 0 -> NaN row (reference: mean of an empty selection) unless empty_as_zero != 0          */
/* (distill_recsys clamp_min(1) semantics -> zero row). counts: int64 per cluster.                   */
/* ---------------------------------------------------------------------------------------------- */
int gdd_cluster_mean(int64_t n, int d, const float* feat, const int32_t* perm, const int32_t* offsets,
                     int k, int empty_as_zero, float* feat_syn, long long* counts,
                     gdd_stream_t stream);
/* gdd_cluster_mean for clusters [c0, c1) only, written as a slice (row c - c0): the cluster-         */
/* partitioned cluster mean of the multi-GPU path, bit-identical to the full call's rows.             */
int gdd_cluster_mean_part(int64_t n, int d, const float* feat, const int32_t* perm,
                          const int32_t* offsets, int k, int c0, int c1, int empty_as_zero,
                          float* feat_part, long long* counts_part, gdd_stream_t stream);
/* labels_syn[c] = argmax_j centers[c,j] (first max wins, torch.argmax; transduct:126).              */
int gdd_argmax_rows(int k, int dim, const float* centers, int64_t* out, gdd_stream_t stream);

/* ---------------------------------------------------------------------------------------------- */
/* (f1/f2) graph condensation: ClustGDD.graph_sparse + ClustGDD.graph_compress                      */
/* (clustgdd_agent_transduct.py:131-250, induct:156-274) and the effective-resistance estimators    */
/* of utils_clustgdd.py:149-182. Edges are the entries of a canonical CSR; rows[e] is each entry's */
/* row (gdd_coo_rows). Orders restated bit for bit by oracle/condense.py.                           */
/* ---------------------------------------------------------------------------------------------- */
int gdd_coo_rows(int64_t n, const int32_t* rowptr, int32_t* rows, gdd_stream_t stream);
size_t gdd_er_ws_bytes(int64_t n, int C);
/* attaw_ER_estimator (utils_clustgdd.py:162-182): rew[e] = val[e] * cos(ebd[src], ebd[dst])         */
/* (ebd: n x C logits), deg = row sums of rew (CSR order), er[e] = rew/deg[src] + rew/deg[dst].     */
int gdd_attaw_er(int64_t n, int64_t nnz, const int32_t* rowptr, const int32_t* rows,
                 const int32_t* col, const float* val, int C, const float* ebd, float* rew, float* er,
                 void* ws, size_t ws_bytes, gdd_stream_t stream);
/* ER_estimator (utils_clustgdd.py:149-159): the same bound on val (NULL = binary).                 */
int gdd_vanilla_er(int64_t n, int64_t nnz, const int32_t* rowptr, const int32_t* rows,
                   const int32_t* col, const float* val, float* er, void* ws, size_t ws_bytes,
                   gdd_stream_t stream);
/* F.softmax(x, dim=-1) on n x C rows (e = fp32(exp(double(x - max))), sequential sum, e / sum).     */
int gdd_softmax_rows(int64_t n, int C, const float* x, float* p, gdd_stream_t stream);
size_t gdd_topk_ws_bytes(int64_t nnz, int nsets);
/* torch.topk(weight, m) per set, as the ascending edge ids of the m largest (NaN largest, ties to   */
/* the lower id): probs (n x nsets) given -> set i weighs edge e by (probs[src,i]*probs[dst,i])*er  */
/* (graph_sparse 'attaw', :154-182); probs NULL -> one set weighed by er ('vanilla'/'single').      */
/* sel: nsets x m int32.                                                                             */
int gdd_class_topk(int64_t nnz, const int32_t* rows, const int32_t* col, const float* er, int nsets,
                   const float* probs, int64_t m, int32_t* sel, void* ws, size_t ws_bytes,
                   gdd_stream_t stream);
size_t gdd_compress_ws_bytes(int kk);
/* graph_compress (:234-250) for one edge set (all m edges, or the m edge ids in sel):               */
/* out (kk x kk) = P^T A P with P = onehot(labels)/cluster sizes, diagonal removed; an empty        */
/* cluster gives a NaN row and column (the reference's 0/0 column of P). kk = max label + 1.        */
/* A node whose label is outside [0, kk) belongs to no cluster: it is not counted and its edges    */
/* add nothing (gdd.condense refuses such labels before calling).                                  */
int gdd_graph_compress(int64_t n, const int32_t* labels, int kk, int64_t m, const int32_t* rows,
                       const int32_t* col, const float* val, const int32_t* sel, float* out, void* ws,
                       size_t ws_bytes, gdd_stream_t stream);
size_t gdd_select_csr_ws_bytes(int64_t n);
/* the selected edges (ascending ids, so already in CSR order) as a CSR: rowptr_out n+1, col/val m. */
int gdd_select_csr(int64_t n, const int32_t* rows, const int32_t* col, const float* val, int64_t m,
                   const int32_t* sel, int32_t* rowptr_out, int32_t* col_out, float* val_out, void* ws,
                   size_t ws_bytes, gdd_stream_t stream);

/* ---------------------------------------------------------------------------------------------- */
/* induced sub-graph adj_full[np.ix_(idx, idx)] as canonical CSR (utils_graphsaint.py:34-36; the   */
/* inductive agent's train/val/test graphs, clustgdd_agent_induct.py:38-94). idx: m strictly        */
/* increasing node ids. Two calls: _count writes rowptr_out (m+1; nnz_out = rowptr_out[m], read by  */
/* the caller to size col/val), _fill writes col_out / val_out (val_out NULL: binary) and copies a  */
/* flag (nonzero if idx was not strictly increasing or out of range) to bad_out (device, nullable). */
/* Both calls share one workspace (gdd_subgraph_ws_bytes), which _count fills and _fill reads.      */
/* ---------------------------------------------------------------------------------------------- */
size_t gdd_subgraph_ws_bytes(int64_t n, int64_t m);
int gdd_subgraph_count(int64_t n, const int32_t* rowptr, const int32_t* col, int64_t m,
                       const int32_t* idx, int32_t* rowptr_out, void* ws, size_t ws_bytes,
                       gdd_stream_t stream);
int gdd_subgraph_fill(int64_t n, const int32_t* rowptr, const int32_t* col, const float* val, int64_t m,
                      const int32_t* idx, const int32_t* rowptr_out, int32_t* col_out, float* val_out,
                      int32_t* bad_out, void* ws, size_t ws_bytes, gdd_stream_t stream);

/* ---------------------------------------------------------------------------------------------- */
/* CSR transpose Aᵀ of an n x n_cols matrix (output n_cols x n, canonical: each row's entries by    */
/* ascending column). The backward of the GCN evaluator's SpMM (models/gcn.py:36-51, d(A @ S)/dS =  */
/* Aᵀ @ grad) and the item side of the recommender's bipartite propagation (distill_recsys.py        */
/* :336-346). val may be NULL (binary: val_t gets 1.0f); val_t may be NULL (structure only);         */
/* perm_out (nullable, nnz) receives the source entry of every transposed entry, so callers whose    */
/* values change (learned edge weights) re-gather val_t = val[perm] without re-sorting.              */
/* ---------------------------------------------------------------------------------------------- */
size_t gdd_csr_transpose_ws_bytes(int64_t n, int64_t n_cols, int64_t nnz);
int gdd_csr_transpose(int64_t n, int64_t n_cols, int64_t nnz, const int32_t* rowptr, const int32_t* col,
                      const float* val, int32_t* rowptr_t, int32_t* col_t, float* val_t, int32_t* perm_out,
                      void* ws, size_t ws_bytes, gdd_stream_t stream);

/* ---------------------------------------------------------------------------------------------- */
/* (f4) recommender condensation. build_condensed_bipartite (distill_recsys.py:184-201): the       */
/* interactions (train_u[e], train_i[e]) become super-node pairs (u2cu[u], i2ci[i]); the output is   */
/* the num_cu x num_ci matrix of pair counts as canonical CSR (what scipy's coo -> sum_duplicates -> */
/* tocsr gives): rowptr_out (num_cu+1), col_out / val_out with capacity E, the stored count written */
/* to nnz_out (device int). bad_out (device, nullable): nonzero if an id was out of range.          */
/* gdd_edge_dots: out[e] = sum_f a[ra[e],f] * b[rb[e],f] (fp32 fma chain, f ascending) - the edge   */
/* gradient of the LightGCN message passing (RecsysModel.propagate, :336-346). a has na rows, b nb:   */
/* an out-of-range row id is not read (out[e] = NaN) and sets *bad (device int, nullable).           */
/* ---------------------------------------------------------------------------------------------- */
size_t gdd_bipartite_condense_ws_bytes(int64_t E, int num_cu);
int gdd_bipartite_condense(int64_t E, const int32_t* train_u, const int32_t* train_i, int64_t num_users,
                           int64_t num_items, const int32_t* u2cu, const int32_t* i2ci, int num_cu,
                           int num_ci, int32_t* rowptr_out, int32_t* col_out, float* val_out,
                           int32_t* nnz_out, int32_t* bad_out, void* ws, size_t ws_bytes,
                           gdd_stream_t stream);
int gdd_edge_dots(int64_t E, int d, const int32_t* ra, const float* a, int64_t na, const int32_t* rb,
                  const float* b, int64_t nb, float* out, int32_t* bad, gdd_stream_t stream);

/* ---------------------------------------------------------------------------------------------- */
/* (f4) the recommender's refinement loop (distill_recsys.py:641-733).                              */
/* gdd_bpr_sample replaces sample_bpr_triplets_from_condensed (:217-272): host-only, draws from the  */
/* caller's numpy RandomState (`state`, a gdd_mt_state, advanced in place) in the reference's order; */
/* positive lists are CSR rows (indptr int64 [num_users+1], int32 indices in list order; `sorted`,   */
/* nullable, the rows sorted for the membership test when `indices` is not). u/pos/neg: batch.      */
/* gdd_recall_at_k replaces recall_at_k's masking, torch.topk and hit count (:475-497) for B users:   */
/* scores (device, B x I, overwritten), tr_ptr/tr_col their training positives, te_ptr/te_col their   */
/* sorted de-duplicated test items (device CSR, B rows); hits (device u64) += |top-k ∩ test|. Equal  */
/* scores rank in ascending item order; k <= 256.                                                    */
/* ---------------------------------------------------------------------------------------------- */
int gdd_bpr_sample(const int64_t* indptr, const int32_t* indices, const int32_t* sorted,
                   int64_t num_users, int64_t num_items, int64_t batch, void* state, int64_t* u_out,
                   int64_t* pos_out, int64_t* neg_out);
int gdd_recall_at_k(int B, int64_t I, int k, float* scores, const int32_t* tr_ptr, const int32_t* tr_col,
                    const int32_t* te_ptr, const int32_t* te_col, unsigned long long* hits,
                    gdd_stream_t stream);

/* ---------------------------------------------------------------------------------------------- */
/* (f4) the refinement epoch on the device (gdd_refine.hip; DESIGN.md §4 "Refinement loop on the    */
/* device"): the LightGCN forward (distill_recsys.py:316-350), bpr_loss with its regularisers        */
/* (:353-384), the KD term (:698-708), the backward of all of it and manual_adam_step (:402-439) as a */
/* fixed chain of 7 + 2L plain launches on `stream`. No floating-point atomic: every sum has a fixed */
/* order, two calls from the same state give the same bits.                                         */
/* gdd_refine_problem: the condensed graph as _Bipartite holds it (rowptr/col: CSR of B, cu: the row */
/*   of every entry; rowptr_t/col_t/perm: gdd_csr_transpose's output), the five parameters (device,   */
/*   fp32 row-major, updated in place by gdd_refine_epochs), the teacher's super-node means (both    */
/*   null: no KD term), 1 <= d <= 256, L >= 0, B triplets per epoch. E may be 0.                     */
/* A batch record is gdd_refine_batch_words(B, num_cu, num_ci) int32 words, written by gdd_bpr_group  */
/*   (host only, needs no device): u[B] pos[B] neg[B] uptr[num_cu+1] uidx[B] iptr[num_ci+1] ient[2B]  */
/*   - the triplet indices grouped by user and the entries 2t+s (s = 0: t's positive, 1: its         */
/*   negative) grouped by item, rows in ascending entry order (a stable counting sort). It refuses   */
/*   an id outside [0, num_cu) / [0, num_ci). The device reads records from device memory and checks  */
/*   every id again before it indexes anything: a bad one is skipped and sets *bad (device int,      */
/*   nullable; bit 0: a triplet or group entry, bit 1: a graph entry), as gdd_edge_dots does.         */
/* gdd_refine_grads (:353-384, :698-708 and loss.backward(), :709): the loss (device float) and the   */
/*   five gradients of one batch; nothing is updated.                                                */
/* gdd_refine_adam_step (:402-439): Adam with bias correction over the five parameters from given    */
/*   gradients; `step` counts from 1. m / (1 - beta^step) is a true fp32 division here.             */
/* gdd_refine_epochs (:689-711): n_epochs consecutive epochs, steps first_step .. first_step +        */
/*   n_epochs - 1, over n_epochs consecutive batch records; losses[ep] (device) receives each loss.   */
/*   No host synchronisation; read losses and *bad after synchronising the stream.                   */
/* ---------------------------------------------------------------------------------------------- */
typedef struct gdd_refine_problem {
  int32_t num_cu, num_ci, d, L;
  int64_t E, B;
  const int32_t *rowptr, *col, *cu, *rowptr_t, *col_t, *perm;
  float *user_emb, *item_emb, *user_delta, *item_delta, *edge_logit;
  const float *t_user, *t_item;
  double reg_lambda, kd_lambda;
} gdd_refine_problem;
typedef struct gdd_refine_adam {
  float* m[5]; /* first and second moments, in the order user_emb, item_emb, user_delta, item_delta, */
  float* v[5]; /* edge_logit                                                                        */
  double lr, beta1, beta2, eps;
} gdd_refine_adam;
int64_t gdd_refine_batch_words(int64_t B, int num_cu, int num_ci);
int gdd_bpr_group(int64_t B, int num_cu, int num_ci, const int64_t* u, const int64_t* pos,
                  const int64_t* neg, int32_t* record);
size_t gdd_refine_ws_bytes(const gdd_refine_problem* p);
int gdd_refine_grads(const gdd_refine_problem* p, const int32_t* batch, float* loss_out, float* g_user_emb,
                     float* g_item_emb, float* g_user_delta, float* g_item_delta, float* g_edge_logit,
                     int32_t* bad, void* ws, size_t ws_bytes, gdd_stream_t stream);
int gdd_refine_adam_step(const gdd_refine_problem* p, const float* g_user_emb, const float* g_item_emb,
                         const float* g_user_delta, const float* g_item_delta, const float* g_edge_logit,
                         const gdd_refine_adam* adam, int64_t step, gdd_stream_t stream);
int gdd_refine_epochs(const gdd_refine_problem* p, const gdd_refine_adam* adam, const int32_t* batches,
                      int64_t first_step, int n_epochs, float* losses, int32_t* bad, void* ws,
                      size_t ws_bytes, gdd_stream_t stream);

/* ---------------------------------------------------------------------------------------------- */
/* (f1) the recommender's clustering embeddings. compute_svd_embeddings (distill_recsys.py:124-155):  */
/* a truncated SVD of the interaction matrix, here a deterministic fp64 block subspace iteration     */
/* with Rayleigh-Ritz (DESIGN.md "Device truncated SVD"; the loop is gdd/svd.py). Every matrix below  */
/* is fp64 row-major with b <= gdd_svd_max_block() (128) columns. No entry point uses floating-point */
/* atomics: two calls on the same input give the same bits.                                         */
/* gdd_spmm_f64 (:124-155, the products behind svds): Y = A X, A CSR n_rows x n_cols with fp32       */
/*   values (val NULL: all ones); each output element is one multiply-then-add chain from +0 in CSR  */
/*   entry order (no fma); empty rows give zeros.                                                    */
/* gdd_gram_f64 (:124-155): G = Wᵀ W (b x b, symmetric bit for bit). form: 0 = fp64 MFMA, 1 = plain  */
/*   fp64 fma, -1 = the library's default. gdd_tsmm_f64 (:124-155): out = W Q, Q b x b, out != W.     */
/* gdd_chol_inv_f64 (:124-155): G = Rᵀ R by Cholesky in one workgroup's LDS, Rinv = R⁻¹ (upper).      */
/*   A pivot at or below b 2^-52 max diag(G) sets *flag (device int, never cleared here) to 1 and    */
/*   gives Rinv = I. gdd_cholqr2_f64 (:124-155): V = orthonormal basis of Z's columns by two passes of*/
/*   gram, chol_inv, tsmm (V may be Z); after a breakdown V is not orthonormal and *flag says so.    */
/* gdd_svd_segment (:124-155): `steps` times W = A V, Z = Aᵀ W, V = CholeskyQR2(Z) with no host       */
/*   synchronisation; A is n_big x n_small CSR, (rowptr_t, col_t, val_t) its transpose               */
/*   (gdd_csr_transpose), V and Z n_small x b, W n_big x b.                                           */
/* gdd_svd_residuals (:124-155): r[j] = ||Z_j - lam[j] V_j||_2 for j < k (lam: device, b values).      */
/* gdd_svd_finalize (:124-155, :148-155 the sqrt(S) scaling): S[j] = sqrt(max(lam[j], 0)); the sign   */
/*   of pair j makes the largest-magnitude entry of V_j positive (lowest row on ties); V_out          */
/*   (n_small x k) = ±V_j, U_out (n_big x k) = ±W_j / S[j] (a zero column where S[j] == 0);           */
/*   emb_small / emb_big (fp32) = those times sqrt(max(S[j], 1e-12)). Outputs but S are nullable;     */
/*   sign: k doubles of scratch.                                                                     */
/* ---------------------------------------------------------------------------------------------- */
int gdd_svd_max_block(void);
int gdd_spmm_f64(int64_t n_rows, int64_t n_cols, const int32_t* rowptr, const int32_t* col,
                 const float* val, int b, const double* X, double* Y, gdd_stream_t stream);
size_t gdd_gram_f64_ws_bytes(int64_t n_rows, int b);
int gdd_gram_f64(int64_t n_rows, int b, const double* W, double* G, int form, void* ws, size_t ws_bytes,
                 gdd_stream_t stream);
int gdd_tsmm_f64(int64_t n_rows, int b, const double* W, const double* Q, double* out,
                 gdd_stream_t stream);
int gdd_chol_inv_f64(int b, const double* G, double* Rinv, int32_t* flag, gdd_stream_t stream);
size_t gdd_cholqr2_ws_bytes(int64_t n_rows, int b);
int gdd_cholqr2_f64(int64_t n_rows, int b, const double* Z, double* V, int32_t* flag, void* ws,
                    size_t ws_bytes, gdd_stream_t stream);
size_t gdd_svd_segment_ws_bytes(int64_t n_big, int64_t n_small, int b);
int gdd_svd_segment(int64_t n_big, int64_t n_small, const int32_t* rowptr, const int32_t* col,
                    const float* val, const int32_t* rowptr_t, const int32_t* col_t, const float* val_t,
                    int b, int steps, double* V, double* W, double* Z, int32_t* flag, void* ws,
                    size_t ws_bytes, gdd_stream_t stream);
size_t gdd_svd_residuals_ws_bytes(int64_t n, int k);
int gdd_svd_residuals(int64_t n, int b, int k, const double* Z, const double* V, const double* lam,
                      double* r, void* ws, size_t ws_bytes, gdd_stream_t stream);
int gdd_svd_finalize(int64_t n_small, int64_t n_big, int b, int k, const double* V, const double* W,
                     const double* lam, double* S, double* V_out, double* U_out, float* emb_small,
                     float* emb_big, double* sign, gdd_stream_t stream);

/* ---------------------------------------------------------------------------------------------- */
/* The Rankformer teacher's layer (Rankformer/code/rec.py:143-274; DESIGN.md "Rankformer teacher").  */
/* Both passes run over a CSR of n_rows x n_cols with nnz stored entries (int32 rowptr / col), fp32   */
/* row-major tables of d columns, 1 <= d <= gdd_rank_max_dim() (256).                                 */
/* gdd_rank_rowpass (rec.py:202-239): per row r and stored entry e = (r, c): s_out[e] = <Q_r, K_c>,   */
/*   s_sum[r] = sum_e s_e, SK[r] = sum_e K_c, SV[r] = sum_e V_c, A[r] = sum_e s_e V_c. Q, s_sum, SK,   */
/*   SV, A have n_rows rows, K and V n_cols rows.                                                     */
/* gdd_rank_wsum (rec.py:135-137, :249-254): Y[r] = sum_e w[e] V_c; with a / b non-null also          */
/*   ta[r] = sum_e a[e], tb[r] = sum_e b[e]. w, a, b are in this CSR's entry order (for a transposed   */
/*   CSR the caller permutes them with gdd_csr_transpose's perm_out). With nnz == 0 (an empty edge     */
/*   array may be a null pointer) a non-null ta / tb is written all the same: zeros.                  */
/* Empty rows give zeros. A column outside [0, n_cols) is not read: it sets *bad (device int,          */
/* nullable), contributes nothing, and its s_out is NaN. No floating-point atomics: the entries are   */
/* cut into fixed chunks, one wave each, a row cut by a chunk end leaves partial sums in ws            */
/* (gdd_rank_ws_bytes, shared by both passes) and a second launch adds them in chunk order, so the     */
/* summation order depends on the CSR alone and two runs give the same bits.                          */
/* ---------------------------------------------------------------------------------------------- */
int gdd_rank_max_dim(void);
size_t gdd_rank_ws_bytes(int64_t nnz, int d);
int gdd_rank_rowpass(int64_t n_rows, int64_t n_cols, int64_t nnz, const int32_t* rowptr,
                     const int32_t* col, int d, const float* Q, const float* K, const float* V,
                     float* s_out, float* s_sum, float* SK, float* SV, float* A, int32_t* bad, void* ws,
                     size_t ws_bytes, gdd_stream_t stream);
int gdd_rank_wsum(int64_t n_rows, int64_t n_cols, int64_t nnz, const int32_t* rowptr, const int32_t* col,
                  int d, const float* w, const float* V, const float* a, const float* b, float* Y,
                  float* ta, float* tb, int32_t* bad, void* ws, size_t ws_bytes, gdd_stream_t stream);

/* ---------------------------------------------------------------------------------------------- */
/* Ranked top-K lists and the ranking metrics (Rankformer/code/model.py:252-343 evaluate: score     */
/* GEMM, training mask, torch.topk; :27-53 test: precision, recall, NDCG; DESIGN.md "Ranked top-K").  */
/* gdd_score_topk (model.py:304-317): for b < B, user row r = users[b] (users NULL: r = b) of U      */
/*   (nu x d, nu >= 1) against all I rows of V (I x d), 1 <= d <= gdd_rank_max_dim(), 1 <= K <= 256, */
/*   K <= I < 2^31, B >= 0 (B == 0 returns without a launch). The score s(u, i) is the fp32 chain    */
/*   s = fmaf(U[r,f], V[i,f], s) over f = 0 .. d-1 ascending, starting from +0: a function of the    */
/*   two rows alone, the same bits whatever B, users, K or the item's place in a tile. An item       */
/*   listed in the user's mask row (mask_ptr / mask_col: CSR of B rows in the order of the call,     */
/*   columns ascending; mask_ptr NULL: no mask) is not removed, its score is mask_value (the         */
/*   reference's -1024, model.py:313), so masked items fill the tail when K exceeds the unmasked.    */
/*   top_item[b, 0 .. K) are the items in descending score, equal scores in ascending item id (the   */
/*   order of gdd_recall_at_k); top_score (nullable) their scores, the bits above. A user id outside */
/*   [0, nu) or a mask column outside [0, I) is not dereferenced: *bad (device int, nullable, not    */
/*   cleared here) is incremented once for that row and the row is all -1 (top_score NaN). No score  */
/*   is written to memory, no workspace, no floating-point atomics: two runs give the same bits.     */
/* gdd_cluster_expand_topk (model.py:304-317 for a condensed model, DESIGN.md "Top-K from the        */
/*   condensed model"): the lists gdd_score_topk gives on the expanded tables U[b] = cu_z[u2cu[b]],  */
/*   V[i] = ci_z[i2ci[i]], from a ranking of the item clusters. cl_item / cl_score (G x L) are the   */
/*   output of gdd_score_topk(G, num_ci, d, L, the G distinct user clusters, cu_z, num_cu, ci_z, no  */
/*   mask, scores) with L = min(num_ci, 256) (1 <= L <= 256, L <= num_ci): row g lists the best L    */
/*   item clusters of one user cluster, descending in key order, with the exact score bits.          */
/*   For b < B: r = users[b] (users NULL: r = b; used for the range check alone), cl_row[b] the row  */
/*   of cl_* of the user's cluster, mem_ptr [num_ci + 1] / mem_item [I] the members of every item    */
/*   cluster in ascending item id (each item in exactly one cluster; empty clusters allowed),        */
/*   mask_ptr / mask_col, mask_value, K, top_item, top_score and bad as in gdd_score_topk, the mask  */
/*   columns of a row strictly ascending. 1 <= K <= 256, K <= I < 2^31.                              */
/*   The clusters c_0 .. c_{L-1} of the row are walked in order. Of cluster c_j the unmasked         */
/*   members (binary search in the mask row) with the K lowest ids enter with score s_j = cl_score;  */
/*   the first min(K, row length) items of the mask row enter with mask_value; the K largest keys    */
/*   are the list. The walk stops after the first j at which K entered-or-thresholded members of     */
/*   c_0 .. c_j score strictly above s_{j+1} (key order; past the row, s_L = s_{L-1}: an unseen      */
/*   cluster may tie the last one): they beat every item not examined. A row whose walk ends without */
/*   that, with L < num_ci, is incomplete: incomplete[b] = 1 (else 0; B ints, written for every b)   */
/*   and *n_incomplete (device int, not cleared here) is incremented; its list is to be recomputed   */
/*   by gdd_score_topk on V = ci_z[i2ci]. With L == num_ci no row is incomplete.                     */
/*   A user id outside [0, nu), a cl_row outside [0, G), a cluster id of the row outside [0, num_ci) */
/*   or a mask column outside [0, I) is not dereferenced: the row is all -1 (top_score NaN), *bad is */
/*   incremented once and incomplete[b] = 0. mem_ptr values are clamped to [0, I]. No score matrix,  */
/*   no workspace, integer atomics on the two counters only: two runs give the same bits.            */
/* gdd_rank_metrics (model.py:27-53): per user b with n = te_deg[b] (te_deg NULL: the row length;     */
/*   the reference counts repeated lines of the split, dataloader.py:65-70) and per cut-off          */
/*   k = topks[j] (device, nk <= 8 ascending values in [1, K]; an entry outside is clamped):         */
/*   hits = |top_item[b, :k] ∩ row b| by binary search in te_ptr / te_col (B rows, ascending,         */
/*   distinct), precision = hits / k, recall = hits / min(n, k) (the reference's clamp, :43-47),     */
/*   ndcg = (sum_{r<k} hit_r inv_log2[r]) / (sum_{r<min(n,k)} inv_log2[r]), both sums in rank order; */
/*   inv_log2 (device, K doubles) = 1 / log2(r + 2) from the host. All fp64. per_user is             */
/*   B x 3 x nk (precision, recall, ndcg); a user with n == 0 gets zeros. sums (3 x nk) adds the     */
/*   users in a fixed order (a second one-workgroup launch; no atomics), count (device int64) is the */
/*   number of users with n > 0: the reference's means are sums / count.                             */
/* ---------------------------------------------------------------------------------------------- */
int gdd_score_topk(int64_t B, int64_t I, int d, int K, const int32_t* users, const float* U, int64_t nu,
                   const float* V, const int32_t* mask_ptr, const int32_t* mask_col, float mask_value,
                   int32_t* top_item, float* top_score, int32_t* bad, gdd_stream_t stream);
int gdd_cluster_expand_topk(int64_t B, int64_t I, int64_t num_ci, int L, int K, const int32_t* users,
                            int64_t nu, const int32_t* cl_row, int64_t G, const int32_t* cl_item,
                            const float* cl_score, const int32_t* mem_ptr, const int32_t* mem_item,
                            const int32_t* mask_ptr, const int32_t* mask_col, float mask_value,
                            int32_t* top_item, float* top_score, int32_t* incomplete, int32_t* n_incomplete,
                            int32_t* bad, gdd_stream_t stream);
int gdd_rank_metrics(int64_t B, int K, const int32_t* top_item, const int32_t* te_ptr, const int32_t* te_col,
                     const int32_t* te_deg, int nk, const int32_t* topks, const double* inv_log2,
                     double* per_user, double* sums, int64_t* count, gdd_stream_t stream);

/* ---------------------------------------------------------------------------------------------- */
/* Full-ranking positions (Rankformer/code/model.py:252-343 evaluate, :27-53 test, for metrics past  */
/* a list of 256: any cut-off, MRR, mean rank, fidelity; DESIGN.md "Full-ranking positions").        */
/* With key(b, i) the u64 order of gdd_score_topk (score chain or mask_value, then item id):         */
/*   pos(b, t) = #{ i in [0, I) : key(b, i) > key(b, t) },                                           */
/* the index at which gdd_score_topk with K = I would list t. Targets are a CSR of B rows in the     */
/* order of the call (tg_ptr [B + 1], tg_col, int32): any order, repeats allowed, rows of any length */
/* (0 included), a masked target carries mask_value. pos (int32, one per entry of tg_col, same       */
/* order). A user id outside [0, nu), a mask column or a target column outside [0, I) is not         */
/* dereferenced: every position of that row is -1 and *bad (device int, nullable, not cleared here)  */
/* is incremented once. No B x I buffer, integer atomics only: two runs give the same integers.      */
/* gdd_score_positions (model.py:252-343, :27-53): users, U, nu, V, mask_ptr / mask_col (columns     */
/*   ascending), mask_value and the limits on B, I, d as in gdd_score_topk. No workspace. A          */
/*   workgroup of 16 users passes over V once per 256 targets of its longest row.                    */
/* gdd_cluster_positions_ws_bytes (model.py:252-343, :27-53): the workspace of                       */
/*   gdd_cluster_positions: the score of every (user cluster, item cluster) pair, 4 G num_ci bytes,  */
/*   and for num_ci <= 4096 each user cluster's row in ranked order with the prefix sums of the      */
/*   cluster sizes, 4 G (2 num_ci + 1) bytes more.                                                   */
/* gdd_cluster_positions (model.py:252-343, :27-53 for a condensed model): the same integers for     */
/*   U[b] = cu_z[u2cu[b]], V[i] = ci_z[i2ci[i]] without either table. cu_z (num_cu x d), ci_z        */
/*   (num_ci x d); groups [G] the distinct user clusters of the call, cl_row[b] in [0, G) the entry  */
/*   of groups that is user b's cluster; users (nullable) for the range check alone; i2ci [I] the    */
/*   cluster of every item (device); mem_ptr / mem_item as in gdd_cluster_expand_topk; the mask      */
/*   columns of a row strictly ascending. With o(.) the high word of the key, o_t = o(mask_value) if */
/*   t is masked, else o(S[i2ci[t]]), S the chain scores of the user's cluster:                      */
/*     pos = sum over clusters c of [o(S[c]) > o_t] size_c + [o(S[c]) == o_t] #{members below t}     */
/*         + sum over masked m of [mask_value ranks m above t] - [S[i2ci[m]] ranks m above t].       */
/*   With ranked rows (num_ci <= 4096) the first sum is one binary search and one prefix entry per   */
/*   target and only tied clusters and the mask row are walked; else every cluster is visited.       */
/*   Besides the cases above, a cl_row outside [0, G), a group outside [0, num_cu) or an i2ci of a   */
/*   mask or target column outside [0, num_ci) gives the -1 row. mem_ptr is clamped to [0, I].       */
/* ---------------------------------------------------------------------------------------------- */
int gdd_score_positions(int64_t B, int64_t I, int d, const int32_t* users, const float* U, int64_t nu,
                        const float* V, const int32_t* mask_ptr, const int32_t* mask_col, float mask_value,
                        const int32_t* tg_ptr, const int32_t* tg_col, int32_t* pos, int32_t* bad,
                        gdd_stream_t stream);
size_t gdd_cluster_positions_ws_bytes(int64_t G, int64_t num_ci);
int gdd_cluster_positions(int64_t B, int64_t I, int64_t num_cu, int64_t num_ci, int d, const float* cu_z,
                          const float* ci_z, const int32_t* users, int64_t nu, const int32_t* cl_row, int64_t G,
                          const int32_t* groups, const int32_t* i2ci, const int32_t* mem_ptr,
                          const int32_t* mem_item, const int32_t* mask_ptr, const int32_t* mask_col,
                          float mask_value, const int32_t* tg_ptr, const int32_t* tg_col, int32_t* pos,
                          int32_t* bad, void* ws, size_t ws_bytes, gdd_stream_t stream);

/* ---------------------------------------------------------------------------------------------- */
/* The teacher's contrastive loss (Rankformer/code/model.py:10-24 InfoNCE, :449-465 its use in the   */
/* loss; DESIGN.md "Contrastive loss"). A, Y: B x d fp32 row-major (the caller normalises; unit rows */
/* are not assumed), 1 <= d <= gdd_rank_max_dim(), 0 <= B < 2^31 (B == 0 returns without a launch),  */
/* inv_tau = 1/tau > 0. l_rc = inv_tau <A_r, Y_c>, the fp32 fmaf chain over f = 0 .. d-1 from +0     */
/* (f32-input MFMA), the same bits in both passes. No logit is stored: Y (A) streams through the LDS */
/* in tiles of 32 rows in ascending order. No floating-point atomics, a fixed order for every sum:   */
/* two runs give the same bits.                                                                      */
/* gdd_infonce_ws_bytes (model.py:10-24, :449-465): the workspace both passes ask for; 0 (the        */
/*   columns are not split over workgroups, so there is nothing to merge).                           */
/* gdd_infonce_rows (model.py:10-24, :449-465): lse[r] = log sum_c exp(l_rc) by online softmax,      */
/*   diag[r] = l_rr (the row's loss is lse[r] - diag[r]), pd[r] (nullable unless R is given) =       */
/*   P_rr = exp(l_rr - lse[r]) taken from the running sums, and with R non-null                      */
/*   R[r] = sum_c exp(l_rc - lse[r]) Y_c (B x d), which the backward needs:                          */
/*   dA_r = inv_tau G_r (R_r - Y_r). The diagonal term P_rr Y_r is added last, so that this          */
/*   difference does not carry the large term's rounding through the chain.                          */
/* gdd_infonce_cols (model.py:10-24, :449-465; the backward of the log-softmax there): with lse and  */
/*   pd from gdd_infonce_rows and an upstream per-row gradient G [B],                                */
/*   C[c] = sum_r G_r exp(l_rc - lse[r]) A_r (B x d): dY_c = inv_tau (C_c - G_c A_c). The diagonal   */
/*   term is G_c pd[c] A_c, added last (the fp32 lse alone gives P_cc only to u |lse|).              */
/* ---------------------------------------------------------------------------------------------- */
size_t gdd_infonce_ws_bytes(int64_t B, int d);
int gdd_infonce_rows(int64_t B, int d, const float* A, const float* Y, float inv_tau, float* lse,
                     float* diag, float* pd, float* R, void* ws, size_t ws_bytes, gdd_stream_t stream);
int gdd_infonce_cols(int64_t B, int d, const float* A, const float* Y, float inv_tau, const float* lse,
                     const float* pd, const float* G, float* C, void* ws, size_t ws_bytes,
                     gdd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GDD_H_ */
