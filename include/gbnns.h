/* gbnns.h -- C ABI of libgbnns_hip.so: the MI355X (gfx950) implementation of the two-stage
 * graph-based ANN search of Shekhale/gbnns_dim_red.
 *
 * The reference has no FFI: its "interface" for this path is the set of free functions in
 * search/search_function.h that search/final_test.cpp calls.  Each entry point below names the
 * reference code it replaces (paths relative to the reference repository root).  The C++ drop-in
 * headers in gbnns_dim_red_amd/search/ keep the reference's names and signatures and call these
 * functions; INTEGRATION.md shows the binding.
 *
 * Conventions: plain pointers and sizes only; every function returns a gbnns_status (0 = OK) and
 * never throws; gbnns_last_error() gives a thread-local message for the last failure.  A handle
 * may be used by one host thread at a time; distinct handles are independent.  All vectors are
 * IEEE binary32, row-major; ids are uint32 (n < 2^31).  There is NO CPU fallback: without a
 * usable gfx950 device gbnns_index_create fails with GBNNS_ERR_NO_DEVICE.
 *
 * Streams: the calls of one handle share its workspace and are ordered by stream order.  A call that names
 * another stream than the handle's previous call first makes the new stream wait for what that call left in
 * flight (the previous stream must still exist, or the device is synchronised) -- results never depend on
 * which stream a call was given.  To overlap batches use one handle per stream (handles may share borrowed
 * device tensors).
 *
 * Device memory per handle besides the index data, per workspace ("lane": one for plain calls, one more per batch in
 * flight with GBNNS_FLAG_DEFER_JOIN, at most four): per-batch buffers (n_q x (d_low + 2 d_hidden + ef + 6) x 4 bytes at
 * most) plus the exact fall-back walk's 64 slots of two n-bit sets and an ef-entry list: 16 n + 512 ef bytes
 * (16 MB at n = 10^6, 160 MB at 10^7).  The large-ef first pass (ef >= 385, deep batches) adds one n-bit set
 * per resident wavefront, capped at 8 GiB.  An index with a net also keeps, beside the net itself, the weights in the
 * order the one-launch projection stages them, once per form of that kernel: about 2 x 1.13 x the net (SIFT net
 * 128 -> 256 -> 256 -> 32: 0.43 MB + 0.95 MB), built when the index is created.
 *
 * Ids in DEVICE buffers are not validated on the host.  An entry id >= n is never dereferenced: that query
 * gets answer 0xFFFFFFFF, an all-0xFFFFFFFF candidate row and zero counters.  Candidate ids >= n passed to
 * gbnns_rerank read row 0 instead.  HOST buffers are validated (GBNNS_ERR_INVALID).
 *
 * HOST buffers of gbnns_search_ex / gbnns_search_batch / gbnns_project / gbnns_rerank may be pageable or page-locked.
 * Page-locked ones (hipHostMalloc, hipHostRegister, gbnns_host_pin) are copied from / to directly.  Pageable ones pass
 * through 4 MB of page-locked staging per workspace, so the runtime never page-locks a caller's array on the fly: it
 * keeps such mappings, and a caller whose allocator later reuses the addresses of a freed array would have a copy fault
 * on the stale one ("an illegal memory access", seen only in long-lived processes).  Costs one pass over host memory.
 */
#ifndef GBNNS_H_
#define GBNNS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GBNNS_VERSION 100 /* 0.1.0 */

typedef enum {
    GBNNS_OK = 0,
    GBNNS_ERR_INVALID = 1,     /* bad argument / inconsistent sizes / id out of range */
    GBNNS_ERR_NO_DEVICE = 2,   /* no HIP device, or device ordinal out of range */
    GBNNS_ERR_HIP = 3,         /* a HIP runtime call failed (message in gbnns_last_error) */
    GBNNS_ERR_OOM = 4,         /* host or device allocation failed */
    GBNNS_ERR_UNSUPPORTED = 5, /* valid request outside what this build implements */
    GBNNS_ERR_INTERNAL = 6     /* the library contradicted itself (a bug): with profiling on, a first pass that launched another kernel than planned */
} gbnns_status;

/* support_func.h:87-163: the Metric* slot.  L2 = L2Metric::Dist (:107-128, drops d%4 tail
 * dims); NEG_DOT = Angular::Dist (:131-163, negative dot product). */
typedef enum { GBNNS_METRIC_L2 = 0, GBNNS_METRIC_NEG_DOT = 1 } gbnns_metric;

typedef enum { GBNNS_MEM_HOST = 0, GBNNS_MEM_DEVICE = 1 } gbnns_mem_kind;

/* Which per-query body of the reference harness one batch call reproduces:
 *   NET   search_function.h:353-362  MLP projection -> walk(ef,k=ef) in low-dim space -> re-rank
 *   LOWQ  search_function.h:158-164  same with caller-supplied low-dim queries (performTest)
 *   PLAIN search_function.h:174-181  walk(ef,k) directly in the space of `db`, answer = top of the heap trimmed
 *         to k, i.e. the k-th best (the best for k = 1, which is what the reference's drivers pass) */
typedef enum { GBNNS_MODE_NET = 0, GBNNS_MODE_LOWQ = 1, GBNNS_MODE_PLAIN = 2 } gbnns_mode;

typedef struct gbnns_index gbnns_index;

/* Everything final_test.cpp:50-76 loads for one dataset.  The callee copies HOST buffers to HBM
 * (caller keeps ownership and may free them after create returns); DEVICE buffers (mem_kind =
 * GBNNS_MEM_DEVICE, pointers valid on `device`) are borrowed and must outlive the index.  The
 * graph is always given in host memory as CSR (neighbour order preserved: it drives tie
 * behaviour through visit order); it is converted once to the device layout. */
typedef struct {
    uint32_t struct_size;          /* = sizeof(gbnns_index_desc) */
    int32_t device;                /* HIP device ordinal */
    int32_t metric;                /* gbnns_metric, used by walk and re-rank */
    int32_t mem_kind;              /* gbnns_mem_kind of db, db_low, net_* */
    uint64_t n;                    /* base vectors */
    uint32_t d;                    /* original dimension */
    uint32_t d_low;                /* low dimension (0: PLAIN mode only) */
    uint32_t d_hidden;             /* MLP width (0: no net -> NET mode unavailable) */
    uint32_t reserved0;
    const float* db;               /* [n x d]          final_test.cpp:50 */
    const float* db_low;           /* [n x d_low]      final_test.cpp:56; may be NULL */
    const uint64_t* graph_offsets; /* [n + 1] host     final_test.cpp:61-63 (loadEdges) */
    const uint32_t* graph_nbrs;    /* [offsets[n]] host */
    const float* net_l1;           /* [d_hidden x (d+1)]        rows = [W | b], final_test.cpp:73-76 */
    const float* net_l2;           /* [d_hidden x (d_hidden+1)] */
    const float* net_l3;           /* [d_low x (d_hidden+1)]    */
} gbnns_index_desc;

/* Replaces the data/graph/net set-up half of final_test.cpp main (:50-76) + the per-call
 * VisitedListPool allocation (search_function.h:331). */
int gbnns_index_create(const gbnns_index_desc* desc, gbnns_index** out);
/* The same index over uint8 base vectors (SIFT / BIGANN .bvecs): db_bytes is [n x d] of desc->mem_kind, desc->db must be NULL, d_low > 0
 * and db_low are required (GBNNS_ERR_INVALID else); graph and net as above.  On the device a row is round_up(d, 16) bytes, zero padded,
 * on a 16-byte aligned base: a HOST table is copied into that layout; a DEVICE table with d % 16 == 0 and a 16-byte aligned address is
 * borrowed (it must outlive the index), any other is re-laid once into an owned copy.  No float32 copy of the table exists on a byte
 * handle: n x round_up(d, 16) bytes instead of n x round_up(d, 4) x 4.
 * Contract: every call on a byte handle returns what the same call returns on the handle created with db = float32(db_bytes), bit for
 * bit -- ids, pop-order candidates, hops, dist_calc, and the exact top-k distances of gbnns_search_topk / gbnns_rerank_topk.  (Every byte
 * value is a binary32 value: nothing is rounded, and the distances are evaluated in the same operation order.)
 * Served: gbnns_search_ex / gbnns_search_batch in NET and LOWQ mode, gbnns_search_topk, gbnns_search_tagged (with and without
 * GBNNS_FLAG_TAG_BRIDGE), gbnns_rerank, gbnns_rerank_topk, gbnns_project, with every flag that applies to them, several entry points,
 * HOST or DEVICE buffers; and, with GBNNS_FLAG_BYTE_WALK (below), gbnns_search_ex and gbnns_search_tagged in GBNNS_MODE_PLAIN, which walks
 * the uint8 rows themselves.  GBNNS_MODE_PLAIN without that flag stays GBNNS_ERR_UNSUPPORTED on a byte handle.  gbnns_multi_create has no
 * byte form.
 * Kernels: with L2, d % 16 == 0, 128-byte walked rows, a compact index, adjacency rows of at most 32 slots and ef <= 128 the first pass
 * (walk_hot_bytes_kernel, walk_hot2_bytes_kernel) re-ranks its own query over the byte rows and hands what it cannot finish to
 * walk_general_bytes_kernel, without a retry pass; every other call runs the very first-pass kernel a float handle would run, without the
 * fused re-rank, followed by the stand-alone byte re-rank kernel (gbnns_debug_byte_plan tells which). */
int gbnns_index_create_bytes(const gbnns_index_desc* desc, const uint8_t* db_bytes, gbnns_index** out);
int gbnns_index_is_bytes(const gbnns_index* index);   /* 1: created by gbnns_index_create_bytes; 0: not (or NULL) */
/* The same index over IEEE binary16 base vectors -- the float datasets (deep, gist, glove) at half the table: db_half is [n x d] binary16 bit
 * patterns of desc->mem_kind, desc->db must be NULL, d_low > 0 and db_low are required (GBNNS_ERR_INVALID else); graph and net as above.  On
 * the device a row is round_up(d, 8) halves, zero padded, on a 16-byte aligned base: a HOST table is copied into that layout; a DEVICE table
 * with d % 8 == 0 and a 16-byte aligned address is borrowed (it must outlive the index), any other is re-laid once into an owned copy of
 * exactly n x round_up(d, 8) x 2 bytes.  No float32 copy of the table exists on a half-base handle.
 * The library does not round a float32 table itself: a caller who has float32 data rounds it with gbnns_round_to_half and passes the bits.
 * Contract: every call on a half-base handle returns what the same call returns on the handle created with db = float32(db_half), bit for
 * bit -- ids, pop-order candidates, out_cand_dist, hops, dist_calc, and the exact top-k distances of gbnns_search_topk / gbnns_rerank_topk.
 * (Widening binary16 to binary32 is exact -- subnormals, both zeros, +-65 504; all arithmetic stays float32 in the reference's order,
 * multiply and add separate; the query is never rounded.)
 * Served: gbnns_search_ex / gbnns_search_batch in NET and LOWQ mode with every flag that applies (GBNNS_FLAG_HALF_ROWS for the walked table
 * included: it is orthogonal), gbnns_search_topk, gbnns_search_tagged (with and without GBNNS_FLAG_TAG_BRIDGE), gbnns_rerank,
 * gbnns_rerank_topk, gbnns_project, gbnns_index_tag_census, several entry points, the auxiliary graph, HOST or DEVICE buffers, batches in
 * flight.  Every search runs the very first-pass kernel a float handle runs under GBNNS_FLAG_NO_FUSED_RERANK, and the stand-alone half
 * re-rank (rerank_half.hip; gbnns_debug_half_base_plan tells which kernel) follows on the same stream.
 * With GBNNS_FLAG_HALF_WALK (below), gbnns_search_ex and gbnns_search_tagged also run in GBNNS_MODE_PLAIN, which walks the binary16 rows themselves.
 * Refused: GBNNS_MODE_PLAIN without that flag (GBNNS_ERR_UNSUPPORTED: there is no float table to walk), gbnns_index_exact_knn, gbnns_index_exact_knn_gather and
 * gbnns_search_tagged_auto (GBNNS_ERR_UNSUPPORTED: they scan the resident table), GBNNS_FLAG_BYTE_WALK and gbnns_search_byte_queries
 * (GBNNS_ERR_INVALID, as on a float handle).  gbnns_multi_create has no half form.
 * Out of scope so far: a half re-rank fused into the walk kernels, resident exact scans over a half table, half queries. */
int gbnns_index_create_half_base(const gbnns_index_desc* desc, const uint16_t* db_half, gbnns_index** out);
int gbnns_index_is_half_base(const gbnns_index* index);   /* 1: created by gbnns_index_create_half_base; 0: not (or NULL) */
int gbnns_index_destroy(gbnns_index* index);
/* what the handle was created with */
uint64_t gbnns_index_n(const gbnns_index* index);
uint32_t gbnns_index_d(const gbnns_index* index);
uint32_t gbnns_index_d_low(const gbnns_index* index);
int gbnns_index_device(const gbnns_index* index);

/* The `auxiliary_graph` argument of getOneSearchResults (search_function.h:44; naive_test.cpp:103-105
 * passes the KL graph): host CSR over the same n nodes, neighbour order preserved, copied to the device
 * layout.  NULL, NULL removes it.  Used by searches that set GBNNS_FLAG_AUX_GRAPH.  Synchronises the
 * device. */
int gbnns_index_set_aux_graph(gbnns_index* index, const uint64_t* offsets, const uint32_t* nbrs);

typedef struct {
    uint32_t struct_size;      /* = sizeof(gbnns_search_args) */
    int32_t mode;              /* gbnns_mode */
    int32_t ef;                /* beam width (= recheck_size in NET/LOWQ, search_function.h:432-434) */
    int32_t k;                 /* PLAIN: heap is trimmed to k, answer = its top = the k-th best (reference uses 1) */
    int32_t mem_kind;          /* gbnns_mem_kind of every buffer below */
    int32_t hash_capacity;     /* 0 = auto (sized from the LDS budget and earlier batches); else entries
                                  (>= 128) of the per-query LDS visited set */
    uint64_t n_q;
    const float* queries;      /* [n_q x d] */
    const float* queries_low;  /* LOWQ: [n_q x d_low], else NULL */
    const uint32_t* entry_ids; /* [n_q x max(n_entries, 1)] entry node(s) per query, NULL = node 0
                                  (search_function.h:417-427) */
    uint32_t* out_ids;         /* [n_q] answers (ans[i], search_function.h:361) */
    int32_t* out_hops;         /* optional [n_q]  TripleResult.hops */
    int32_t* out_dist_calc;    /* optional [n_q]  TripleResult.dist_calc (walk only, without the
                                  "+ recheck_size" the harness adds at :362) */
    uint32_t* out_cand;        /* optional [n_q x min(k,ef)] result heap in POP order (worst->best),
                                  0xFFFFFFFF padded; k = ef in NET/LOWQ */
    float* out_cand_dist;      /* optional, same shape: low-dim distances of out_cand (+inf pad) */
    float* out_q_low;          /* optional NET: [n_q x d_low] projected queries */
    int32_t* out_edges;        /* optional [n_q]: neighbour ids read by the walk (sum of the degrees of
                                  the expanded nodes) -- feeds the algorithmic-bytes figure.  The degrees are
                                  those of the rows as the index keeps them: an id that repeats inside a row
                                  of graph_nbrs is kept once (its first occurrence) and counted once; with
                                  GBNNS_FLAG_AUX_GRAPH the auxiliary rows a hop reads count as well */
    void* stream;              /* hipStream_t to enqueue on (NULL = default stream) */
    uint32_t flags;            /* GBNNS_FLAG_* */
    uint32_t hops_bound;       /* with GBNNS_FLAG_AUX_GRAPH: auxiliary rows are expanded while hops < hops_bound
                                  (search_function.h:73; the harness passes 50, :273/:338) */
    uint32_t n_entries;        /* entry points per query (inter_points[i].size(), search_function.h:54); 0 or 1 =
                                  one.  More than one: one walk per entry point over a shared result heap, exactly
                                  as :54-93 -- served by the general kernel (exact, not tuned: no driver of the
                                  reference uses it) */
    uint32_t defer_depth;      /* with GBNNS_FLAG_DEFER_JOIN: batches in flight, 2 .. 4 (0 = 3, the measured optimum) */
} gbnns_search_args;

/* The throughput option (opt-in; never a default, never what bench.py reports as `value`): the projection's three layers
 * as GEMMs on the matrix cores (v_mfma_f32_32x32x2_f32, csrc/mlp.hip: mlp_layer_mfma_kernel).  An output is then ONE
 * k-ordered fma chain instead of the reference's eight separately rounded running sums (support_func.h:131-163): q_low
 * differs from the exact kernels' in its last bits (a few 1e-7), and a few answers of a batch may differ from the
 * reference's -- bench.py states how many (throughput_option.id_mismatches_vs_reference).  (Rounds 1-2 had this option on
 * flag bit 1; removed in round 3, rebuilt in round 5 on bit 8.) */
#define GBNNS_FLAG_MFMA_PROJECTION 256u
/* Diagnostic: keep the re-rank (getRealNearest, search_function.h:105-125) in its own kernel launch even
 * where the walk kernels could re-rank each query at the end of its walk.  Results are identical either
 * way; the flag exists for A/B measurements and for timing the two stages separately. */
#define GBNNS_FLAG_NO_FUSED_RERANK 2u

/* use_second_graph = true (search_function.h:73-89): while a query has made fewer than `hops_bound` hops,
 * the auxiliary row of the expanded node (gbnns_index_set_aux_graph) is offered before its main row.  With
 * GBNNS_FLAG_LLF (the reference's `llf`) the main row is skipped on a hop whose auxiliary step inserted
 * something (:82).  Bit-identical to the reference. */
#define GBNNS_FLAG_AUX_GRAPH 4u
#define GBNNS_FLAG_LLF 8u

/* Diagnostic: run the kernels an index of n >= 2^24 nodes or tables >= 4 GiB would get (64-bit offsets, 4-byte
 * visited-set slots) on a small index, so that the tests can reach them.  Same results. */
#define GBNNS_FLAG_WIDE_INDEX 16u

/* Diagnostic: take the first pass with HBM visited bitmaps (persistent wavefronts, LDS-list kernel) whatever ef and
 * batch size -- by default it serves ef >= 385 on batches deeper than 1.5 rounds of the wavefronts an LDS visited
 * table would allow.  Same results. */
#define GBNNS_FLAG_BITMAP_PASS 32u

/* Batches in flight.  A handle owns up to four workspaces with an internal HIP stream each ("lanes"); plain calls use
 * the first one on the caller's stream.  Every query is independent (search_function.h:348), so the answers never
 * depend on how a call is laid out.
 *   GBNNS_FLAG_DEFER_JOIN  DEVICE buffers: the batch runs on the next of `defer_depth` lanes (consecutive calls rotate)
 *                          after what was enqueued on args->stream before the call, and the call returns WITHOUT
 *                          making args->stream wait for it.  That wait is enqueued by the (defer_depth - 1)-th following
 *                          call on this handle -- after that call's own batch has been released, so `defer_depth`
 *                          batches are in flight: the half-empty tail of batch i's walk kernel (a 10 k batch is < 2
 *                          "rounds" of resident wavefronts) runs beside the projection and the head of batch i+1, and
 *                          batches too small to fill the machine (the reference's 1 000 GIST queries are one
 *                          wavefront per SIMD) run side by side -- or by gbnns_index_join, or by any call without the
 *                          flag.  Until then the outputs of the call must not be read and its inputs / outputs must
 *                          not be reused: a serving loop rotates `defer_depth` sets of buffers.  args->stream must
 *                          stay alive until the call has been joined.
 *   GBNNS_FLAG_SERIAL      the caller's stream, kernels back to back, whatever else is asked (what per-kernel timing
 *                          needs; gbnns_profile_enable(..., 1) implies it).  HOST-buffer calls run this way and
 *                          synchronously unless they ask for GBNNS_FLAG_DEFER_JOIN with page-locked buffers (below). */
#define GBNNS_FLAG_SERIAL 64u
#define GBNNS_FLAG_DEFER_JOIN 128u

/* Half rows (opt-in; never a default, never what bench.py reports): the walk gathers its low-dimensional rows from a table of IEEE
 * binary16 values, half the bytes a hop reads.  The feature has an exact definition: a search with GBNNS_FLAG_HALF_ROWS is the
 * reference's search run on the table R = float32(float16(db_low)) -- every coordinate rounded once to nearest-even binary16
 * (gbnns_round_to_half below IS that rounding) and widened back, which is exact.  All arithmetic stays float32 in the reference's
 * order, the query is never rounded (NET: the exact projection, as always), and the re-rank in the space of `db` is untouched.  Every
 * output keeps its meaning with db_low read as R: ids, pop order, hops, dist_calc, and out_cand_dist = the distances to rows of R,
 * bit for bit.  NET / LOWQ only (PLAIN walks the answer space: GBNNS_ERR_INVALID); the handle must have been prepared with
 * gbnns_index_enable_half_rows (else GBNNS_ERR_INVALID).  Applies to gbnns_search_ex, gbnns_search_topk and the gbnns_multi_*
 * searches (which pass the flag through: the caller enables each gbnns_multi_replica) and combines with every other flag,
 * hash_capacity, several entry points, the auxiliary graph, batches in flight and HOST or DEVICE buffers.  The first pass gathers
 * 2-byte rows (walk_reg_half_kernel / walk_reg_big_half_kernel in gbnns_profile.walk_kernel) for a compact index (tables < 4 GiB,
 * n < 2^24) with one entry point per query and no auxiliary graph, over rows of 32 / 48 / 64 floats with L2 and 32 floats with the
 * negative dot at every beam up to 1 024, and of 144 floats with L2 at beams above 128; every other case -- and the retry pass, the
 * general kernel, the bitmap pass, the two-wavefront walk -- runs the float32 kernels on a float32 copy of R: same results.  No call
 * without the flag changes in any way. */
#define GBNNS_FLAG_HALF_ROWS 512u
/* Host code, no device needed: out_bits[i] = in[i] rounded to binary16 (nearest, ties to even; subnormals and the sign of zero
 * kept), out_widened[i] = that value as a float.  Either output may be NULL.  A value that is not finite or whose rounding leaves the
 * binary16 range (|x| >= 65 520) gives GBNNS_ERR_UNSUPPORTED with the index of the first such value in gbnns_last_error(); outputs
 * before it have been written. */
int gbnns_round_to_half(const float* in, uint64_t count, uint16_t* out_bits, float* out_widened);
/* Builds, on the handle's device and from its db_low (copied from the host or borrowed from the device), the two tables flagged
 * searches walk: R as binary16 rows of round_up(d_low, 8) values, zero padded, and R as float32 rows in db_low's layout.  Device
 * memory: 1.5 x the low-dimensional table ON TOP of it -- db_low itself stays and searches without the flag keep using it (the
 * option halves the bytes a hop reads, not the memory).  Synchronises the device; idempotent.  GBNNS_ERR_INVALID without db_low,
 * GBNNS_ERR_UNSUPPORTED when a value is not finite or rounds out of the binary16 range (the handle stays as it was),
 * GBNNS_ERR_OOM. */
int gbnns_index_enable_half_rows(gbnns_index* index);
/* out [n x d_low] = R, the table flagged searches walk (HOST: synchronous; DEVICE: enqueued on `stream`).  GBNNS_ERR_INVALID before
 * gbnns_index_enable_half_rows. */
int gbnns_index_low_rows(gbnns_index* index, float* out, int mem_kind, void* stream);

/* Replaces the timed query loop of performNetTest (search_function.h:346-387) / performTest
 * (:151-188): one call = the whole batch.  With HOST buffers the call copies in, runs and
 * copies out synchronously (what the drop-in harness times).  With DEVICE buffers everything is
 * enqueued on args->stream and the call returns without synchronising.
 * Queries are independent (the reference's loop is an OpenMP parallel for over them): the order in which the device
 * serves the queries of a batch is the library's business -- batches of >= 32 768 queries are walked in a locality
 * order -- and every output row i always belongs to query i. */
int gbnns_search_ex(gbnns_index* index, const gbnns_search_args* args);

/* Enqueues, on the streams of the GBNNS_FLAG_DEFER_JOIN calls not yet joined, the waits for their batches (no-op when
 * nothing is owed).  Everything enqueued on those streams afterwards sees the calls' outputs. */
int gbnns_index_join(gbnns_index* index);

/* Host batches in flight.  GBNNS_FLAG_DEFER_JOIN also takes HOST buffers when every one of them is page-locked
 * (hipHostMalloc / hipHostRegister; with a pageable buffer among them the flag is ignored and the call is the plain
 * synchronous one -- a caller that follows the protocol below is correct either way): the copy of the queries to the device, the kernels and
 * the copies out all go to the lane's stream and the call returns at once, so the wire time of batch i+1 (0.10 ms of
 * a 0.54 ms synchronous call for 10 000 x 128 floats) passes under the kernels of batches i and i-1.  The ids are
 * stored by the kernel straight into the page-locked out_ids (so are they in a synchronous HOST call whose out_ids
 * happens to be page-locked).  gbnns_index_wait blocks the calling thread until every deferred batch but the `keep`
 * most recent has finished: their host buffers then hold the results and may be refilled (keep = depth - 1 after
 * each call keeps the pipeline full; keep = 0 drains it).  Defined in terms of the reference: each call is still one
 * run of the timed loop of search_function.h:346-387 over its own batch. */
int gbnns_index_wait(gbnns_index* index, uint32_t keep);

/* Page-locks (hipHostRegister) / releases a host buffer, for callers that do not link the HIP runtime themselves: HOST
 * buffers that are page-locked are copied in by DMA without a staging pass, take ids, hop counts, dist_calc and edge
 * counts straight from the kernels (no copies out), and may be used with GBNNS_FLAG_DEFER_JOIN.  The drop-in's
 * perform*Test functions pin the query / answer vectors before their timed region (the reference builds its
 * VisitedListPool there, search_function.h:333) and release them after it.  Pinning an already page-locked buffer
 * and releasing one that was not pinned here are no-ops.  Registrations are made in whole pages and never overlap:
 * small buffers that share a page share its registration (counted), which is released with its last user. */
int gbnns_host_pin(void* ptr, size_t bytes);
int gbnns_host_unpin(void* ptr);

/* Convenience form of the above: NET mode, host buffers, synchronous. */
int gbnns_search_batch(gbnns_index* index, const float* queries, size_t n_q, int ef,
                       const uint32_t* entry_ids, uint32_t* out_ids, int32_t* out_hops,
                       int32_t* out_dist_calc, uint32_t* out_cand);

/* GetLowQueryFromNet (support_func.h:645-658) over a batch: x [n_x x d] -> out [n_x x d_low].
 * Also what produces `<name>_base_angular_optimal.fvecs` from the base set. */
int gbnns_project(gbnns_index* index, const float* x, uint64_t n_x, float* out, int mem_kind,
                  void* stream);

/* getRealNearest (search_function.h:105-125) over a batch: for query i, cand[i*stride ..] holds
 * count[i] (NULL: stride) candidate ids in POP order (worst -> best in the low-dim space); the
 * answer is the strict minimum of the exact distance in the space of `db`, earlier entries
 * winning ties. */
int gbnns_rerank(gbnns_index* index, const float* queries, uint64_t n_q, const uint32_t* cand,
                 uint32_t cand_stride, const int32_t* count, uint32_t* out_ids, int mem_kind,
                 void* stream);

/* Candidates in, k best out -- the k-answer form of gbnns_rerank.  The reference has no such function (getRealNearest
 * returns one id); this is its natural extension, chosen so that k = 1 reproduces it.  With dist_r = Dist(db[cand_r], q_i)
 * in the space of `db`, in the reference's arithmetic (the very bits gbnns_rerank minimises over) and r = 0 .. count[i] - 1
 * the pop index, row i of out_ids [n_q x k] holds the min(k, count[i]) smallest candidates in ascending order of
 * (dist_r, r): distances compare as everywhere in the library (-0 equals +0), the lower pop index wins ties.  Column 0
 * is therefore always exactly the id gbnns_rerank -- or a search's fused re-rank -- returns for that list.  out_dist
 * (optional, [n_q x k]) receives each distance's own bit pattern as computed.  Columns from count[i] on hold 0xFFFFFFFF
 * and +inf; a candidate that occurs twice is reported twice.  1 <= k <= cand_stride (GBNNS_ERR_INVALID).  HOST buffers are
 * validated (an id >= n or a count above the stride: GBNNS_ERR_INVALID) and the call is synchronous; DEVICE buffers are
 * enqueued on `stream`, an id >= n is read as row 0 and reported as given, as in gbnns_rerank.  One wavefront per query
 * keeps the list's keys and distances in LDS beside the query: a shape whose 4 * d + 12 * cand_stride bytes exceed the
 * 160 KiB of a workgroup is refused (GBNNS_ERR_UNSUPPORTED). */
int gbnns_rerank_topk(gbnns_index* index, const float* queries, uint64_t n_q, const uint32_t* cand,
                      uint32_t cand_stride, const int32_t* count, int k, uint32_t* out_ids, float* out_dist,
                      int mem_kind, void* stream);

/* gbnns_search_ex plus the k best of each query's ef candidates in the original space (the contract of
 * gbnns_rerank_topk over the walk's candidate list in pop order): out_top_ids [n_q x k], out_top_dist (optional)
 * likewise, buffers of args->mem_kind.  Everything gbnns_search_ex writes is written as before, the very same search
 * runs, and out_top_ids[i * k] == args->out_ids[i]; a query with an entry id >= n gets a row of 0xFFFFFFFF / +inf.
 * NET / LOWQ only: a PLAIN walk's out_cand / out_cand_dist already are the answer in the walked space
 * (GBNNS_ERR_INVALID).  1 <= k <= ef.  GBNNS_FLAG_DEFER_JOIN holds as for gbnns_search_ex (HOST buffers: the two arrays
 * must be page-locked too); the selection runs behind the re-rank and is part of gbnns_profile.rerank_ms. */
int gbnns_search_topk(gbnns_index* index, const gbnns_search_args* args, int k, uint32_t* out_top_ids,
                      float* out_top_dist);

/* Tag-filtered search (opt-in: an entry point of its own; no other call changes in any way).  Every row j of the index has a 32-bit tag
 * word T[j], every query i a word Q[i], and row j is ALLOWED for query i when (T[j] & Q[i]) != 0: deleted rows, tenants, categories, "not
 * the item itself".  The definition: a tagged search of query i is the reference's search of query i on the graph G'(i) -- the index's graph
 * with every adjacency row keeping only the neighbours allowed for query i, in their original order; the auxiliary graph, where used, is
 * cut the same way.  Nothing else changes: the arithmetic, the visit order among the kept neighbours, the tie behaviour, the fused or
 * separate re-rank (whose candidates are all allowed by construction), and the meaning of every output -- ids, hops, dist_calc, edges (the
 * degrees in G'), out_cand / out_cand_dist in pop order, out_q_low, the top-k rows.  Consequences:
 *   - a disallowed row is never claimed in the visited set, never has its distance computed and is never counted;
 *   - the expected value of every output is the CPU oracle's on the CSR cut with NumPy (gbnns_dim_red_amd.cut_graph), one oracle call per
 *     distinct value of Q -- bit for bit, the tests take no tolerance;
 *   - the entry point is the reference's: it enters the heap untested.  A query whose entry row is not allowed for it (with several entry
 *     points: any of them) gets the row an entry id >= n gets: answer 0xFFFFFFFF, an all-0xFFFFFFFF candidate row, +inf distances, zero
 *     counters, 0xFFFFFFFF / +inf top-k rows.  That includes every query with Q[i] == 0.  In a tagged call this is data, not an argument
 *     error, for HOST and DEVICE buffers alike (an entry id >= n in a HOST buffer too);
 *   - with T all 0xFFFFFFFF and Q all 0xFFFFFFFF every output equals the untagged search's bit for bit, counters included;
 *   - restricting the walk to G' can strand a query in a small component when few rows are allowed.  That is the definition, not a
 *     defect: raise ef, or supply entry points that are allowed (and close).  DESIGN.md 5.1 ("Tagged search") has the measured recall by allowed fraction.
 *
 * gbnns_index_set_tags: the handle owns an n x 4-byte device table, created on first use and initialised to 0xFFFFFFFF.  The call
 * overwrites rows [first, first + count) from a HOST (synchronous) or DEVICE buffer, ordered on `stream` like a search on that stream.
 * tags == NULL with count == 0 drops the table (synchronises the device).  A range outside n: GBNNS_ERR_INVALID.
 *
 * gbnns_search_tagged: query_tags [n_q], a buffer of args->mem_kind.  With k == 0 and both outputs NULL it is gbnns_search_ex under the
 * contract above, with 1 <= k <= ef gbnns_search_topk under it (k > ef, or PLAIN mode with k != 0: GBNNS_ERR_INVALID).  NET, LOWQ and
 * PLAIN modes.  Needs gbnns_index_set_tags and query_tags (else GBNNS_ERR_INVALID).  Combines with hash_capacity, several entry points,
 * GBNNS_FLAG_AUX_GRAPH / GBNNS_FLAG_LLF, GBNNS_FLAG_WIDE_INDEX, GBNNS_FLAG_SERIAL, GBNNS_FLAG_NO_FUSED_RERANK and GBNNS_FLAG_DEFER_JOIN
 * (query_tags then obeys the lifetime and page-lock rules of the other inputs); GBNNS_FLAG_BITMAP_PASS is ignored.  With
 * GBNNS_FLAG_HALF_ROWS or GBNNS_FLAG_MFMA_PROJECTION: GBNNS_ERR_UNSUPPORTED for now.  The gbnns_multi_* searches have no tagged form yet.
 * The first pass is a tag instance (walk_reg_tag_kernel / walk_reg_big_tag_kernel in gbnns_profile.walk_kernel: the tag test per neighbour,
 * inside the hop) for a compact index (tables < 4 GiB, n < 2^24) with one entry point per query and no auxiliary graph, over rows of
 * 32 / 48 / 64 floats with L2 and 32 floats with the negative dot at every beam up to 1 024 and of 144 floats with L2 at beams above 128;
 * what it hands over goes straight to the general kernel (there is no tagged retry pass), and every other case runs whole on the general
 * kernel: same results.  gbnns_profile.walk_kernel and gbnns_debug_tag_plan then say "walk_general_kernel": the name stands for the general
 * kernel in both its forms -- what a tagged call launches is its instance with the tag test, walk_general_tag_kernel.  Device memory: 4 n bytes. */
int gbnns_index_set_tags(gbnns_index* index, const uint32_t* tags, uint64_t first, uint64_t count, int mem_kind, void* stream);
int gbnns_search_tagged(gbnns_index* index, const gbnns_search_args* args, const uint32_t* query_tags, int k, uint32_t* out_top_ids,
                        float* out_top_dist);

/* Bridged tagged search (a flag of gbnns_search_tagged, with and without k): the walk looks THROUGH a disallowed neighbour instead of
 * dropping it -- one-level two-hop expansion, the ACORN-1 rule -- so that a filter which allows few rows no longer strands the walk (DESIGN.md
 * 5.1, "Bridged tagged search", has the measured recall and cost).  Tags, query words and the allowed test are gbnns_search_tagged's.  The
 * definition: a bridged tagged search of query i is the reference's search of query i on the graph G''(i), whose row of node u is built from
 * the slots of u's row in the index's graph, in order:
 *   - an allowed neighbour v contributes v;
 *   - a disallowed neighbour v contributes, in v's place, the allowed entries of v's own row, in their order;
 *   - one level only: a disallowed entry of v's row is dropped, not looked through;
 *   - the row is a plain concatenation: it may hold u itself and the same id more than once -- the reference's visited test disposes of both
 *     (of equal ids the first occurrence is the one claimed, measured and offered);
 *   - the auxiliary graph, where used, is bridged through itself;
 *   - "u's row" and "v's own row" are the rows as the index keeps them: an id that repeats inside a row of graph_nbrs is kept once, at its
 *     first occurrence (no walk can tell; out_edges counts the degrees of this G'').
 * Nothing else changes: ids, pop order, distance bits, hops, dist_calc, out_q_low and the top-k rows are the CPU oracle's on G''
 * (gbnns_dim_red_amd.bridge_graph builds it with NumPy), bit for bit.  Looking through v is not a hop; a disallowed row is never claimed in
 * the visited set, never has a distance computed and is never counted in dist_calc; out_edges is the degree in G'' of the expanded nodes,
 * repeated ids included.  The entry row enters untested and must be allowed: a bad or disallowed entry gives the bad-entry row of a tagged
 * call, so every expanded node is allowed.  With every row allowed G'' is the index's graph and every output equals the untagged search's,
 * counters and edges included.
 * The flag combines with everything a tagged call combines with (hash_capacity, several entry points, GBNNS_FLAG_AUX_GRAPH / GBNNS_FLAG_LLF,
 * GBNNS_FLAG_WIDE_INDEX, GBNNS_FLAG_SERIAL, GBNNS_FLAG_NO_FUSED_RERANK, GBNNS_FLAG_DEFER_JOIN, HOST and DEVICE buffers, NET / LOWQ / PLAIN);
 * GBNNS_FLAG_HALF_ROWS and GBNNS_FLAG_MFMA_PROJECTION stay GBNNS_ERR_UNSUPPORTED.  In gbnns_search_ex, gbnns_search_topk and the
 * gbnns_multi_* searches the flag is GBNNS_ERR_INVALID.
 * The first pass is a bridge instance (walk_bridge_kernel in gbnns_profile.walk_kernel) for a compact index with one entry point per query and
 * no auxiliary graph, over rows of 32 / 48 / 64 floats with L2 and 32 floats with the negative dot at beams up to 128; what it hands over,
 * and every other case (beams above 128 and 144-float rows included), runs on the general kernel's bridged instance ("walk_general_kernel"
 * in the profile and in gbnns_debug_bridge_plan): same results. */
#define GBNNS_FLAG_TAG_BRIDGE 1024u
/* The byte-row PLAIN walk: gbnns_search_ex and gbnns_search_tagged (with and without GBNNS_FLAG_TAG_BRIDGE, k == 0) with
 * mode == GBNNS_MODE_PLAIN on a byte handle (gbnns_index_create_bytes) walk the graph in the space of the handle's uint8 table -- the hnsw
 * half of the reference's final_test over .bvecs data.
 * Contract: Every output equals, bit for bit, what the same call without the flag returns on the handle created with
 * db = float32(db_bytes).  The outputs are ids, out_cand in pop order, out_cand_dist bit patterns, hops, dist_calc and edges.  This holds
 * for every k, both metrics, any d (the L2 d % 4 tail ignored, the dot's masked tail against the zero padding), and several entry points;
 * with GBNNS_FLAG_AUX_GRAPH / GBNNS_FLAG_LLF, GBNNS_FLAG_WIDE_INDEX, hash_capacity, GBNNS_FLAG_SERIAL, GBNNS_FLAG_DEFER_JOIN, and HOST or
 * DEVICE buffers.  GBNNS_FLAG_BITMAP_PASS is ignored.  A bad entry id gives the documented all-0xFFFFFFFF row.  (Each byte is widened with
 * one exact conversion and the sums run in the reference's order -- four running sums, separately rounded subtract, multiply and add.)
 * No float copy of the table is made, on the device or the host, at any point: the memory promise of the byte handle holds for PLAIN calls.
 * Refused with GBNNS_ERR_INVALID: the flag on a float handle; the flag with NET / LOWQ (the walked space is db_low, which is float32); the
 * flag in the gbnns_multi_* searches.  gbnns_search_topk in PLAIN mode and GBNNS_FLAG_HALF_ROWS in PLAIN mode stay GBNNS_ERR_INVALID.
 * The walk is opt-in for now: GBNNS_MODE_PLAIN without the flag on a byte handle stays GBNNS_ERR_UNSUPPORTED.  Lifting the flag requirement
 * -- PLAIN on a byte handle simply meaning this walk -- is a later, separate change.
 * Kernels: L2 with d == 128, a compact index (n < 2^24, tables < 4 GiB), one entry point per query, no auxiliary graph, untagged and
 * ef <= 1 024 run a byte-walk first pass (walk_reg_bytes_kernel<R, ONE_CHUNK>, walk_reg_big_bytes_kernel<ONE_PASS> in
 * gbnns_profile.walk_kernel): two lanes per neighbour over packed 16-byte chunks, the query in LDS.  It has no retry pass; what it hands
 * over, and every other flagged call -- other dimensions, the negative dot, several entry points, the auxiliary graph, GBNNS_FLAG_WIDE_INDEX,
 * beams above 1 024, every tagged or bridged call -- runs on the general kernel's byte-walk instance ("walk_general_kernel" in the profile
 * and in gbnns_debug_byte_walk_plan), which is exact, not tuned: a lane per row. */
#define GBNNS_FLAG_BYTE_WALK 2048u

/* Half-row PLAIN walk on a half-base handle (gbnns_index_create_half_base): GBNNS_MODE_PLAIN in gbnns_search_ex / gbnns_search_batch and in
 * gbnns_search_tagged (cut and with GBNNS_FLAG_TAG_BRIDGE) walks the binary16 rows themselves -- the hnsw half of the reference's
 * final_test, the efs_hnsw sweeps, on the handle that keeps the original table at two bytes a coordinate.
 * Contract: every output equals, bit for bit, what the same call WITHOUT this flag returns on the float handle created with
 * db = float32(db_half): ids, out_cand in pop order, out_cand_dist bit patterns, hops, dist_calc and edges -- for every k, both metrics, any
 * d (the L2 d % 4 tail is never read into a sum and may hold any bit pattern; the dot reads all d and its masked tail the zero padding),
 * several entry points, GBNNS_FLAG_AUX_GRAPH / GBNNS_FLAG_LLF, GBNNS_FLAG_WIDE_INDEX, hash_capacity, GBNNS_FLAG_SERIAL,
 * GBNNS_FLAG_DEFER_JOIN, HOST or DEVICE buffers.  GBNNS_FLAG_BITMAP_PASS is ignored.  (Widening binary16 is exact, the query is never
 * rounded, and the sums run in float32 in the reference's order.)  No float copy of the table is made, on the device or the host, at any
 * point.
 * Refused with GBNNS_ERR_INVALID: the flag on a float or a byte handle; the flag with NET / LOWQ (the walked space is db_low, which is
 * float32); the flag together with GBNNS_FLAG_BYTE_WALK; the flag in the gbnns_multi_* searches.  uint8 and float16 queries stay refused,
 * and gbnns_search_topk in PLAIN mode stays GBNNS_ERR_INVALID as on every handle.  The walk is opt-in: GBNNS_MODE_PLAIN without the flag on
 * a half-base handle stays GBNNS_ERR_UNSUPPORTED.
 * Kernels: L2 on a compact index (n < 2^24, the half table and the adjacency table < 4 GiB), one entry point per query, no auxiliary graph,
 * untagged, ef <= 1 024 run a half-walk first pass (walk_reg_hwalk_kernel<STEPS, R, ONE_CHUNK> / walk_reg_big_hwalk_kernel<STEPS, ONE_PASS>
 * in gbnns_profile.walk_kernel): d == 96 the 24-step pair form (six 16-byte loads a lane, packed until widened); d >= 128 with d % 4 == 0
 * the run-time-length form, two lanes per row over 16-byte chunks -- built and exact, but not measured against the general instance yet, so
 * only a handle whose knob "half_walk_fast" is 2 takes it (default 1: such a call runs on the general instance).  They have no retry pass; what they hand over, and every other flagged
 * call -- other dimensions, the negative dot, several entry points, the auxiliary graph, GBNNS_FLAG_WIDE_INDEX, beams above 1 024, every
 * tagged or bridged call, and every call of a handle whose knob "half_walk_fast" is 0 -- runs on the general kernel's half-walk instance
 * ("walk_general_kernel" in the profile and in gbnns_debug_half_walk_plan), which is exact, not tuned: a lane per row. */
#define GBNNS_FLAG_HALF_WALK 8192u

/* Byte queries on a byte handle (gbnns_index_create_bytes): the search whose queries are uint8 as well -- BIGANN's query files are .bvecs too.
 * `queries_u8` is [n_q x d] dense bytes, a buffer of args->mem_kind; args->queries must be NULL.  query_tags == NULL: untagged; k / out_top_*
 * as in gbnns_search_tagged (k == 0 and both NULL: no k-answer rows).
 * Contract: every output equals, bit for bit, what the corresponding existing call -- gbnns_search_ex, gbnns_search_topk or
 * gbnns_search_tagged -- returns on the same handle with queries = float32(queries_u8): ids, out_cand in pop order, out_cand_dist bit
 * patterns, hops, dist_calc, edges, out_q_low and the k-answer rows.  This holds in NET, LOWQ (queries_low stays float32) and PLAIN mode
 * (GBNNS_FLAG_BYTE_WALK required, as for float queries), with HOST and DEVICE buffers, GBNNS_FLAG_DEFER_JOIN (the byte buffer obeys the
 * lifetime and page-lock rules of the other inputs), GBNNS_FLAG_SERIAL, hash_capacity, several entry points, the auxiliary graph, tags and
 * the bridge.  The library widens the bytes on the device into a buffer of its own (uint8 -> float32 rounds nothing) and every kernel runs
 * unchanged on that copy -- it IS the definition -- but one family: inside the byte-walk first pass's domain (PLAIN, L2, d == 128, compact
 * index, one entry point, no auxiliary graph, untagged, ef <= 1 024) the first pass is the integer twin of the byte-walk instance
 * (beam_u8_kernel<R, ONE_CHUNK> / beam_u8_big_kernel<ONE_PASS> in gbnns_profile.walk_kernel), which reads the byte queries themselves and
 * computes sum q^2 + sum x^2 - 2 sum q x in uint32, four products an instruction.  For d <= 256 every intermediate of the reference's distance
 * is an integer below 2^24 (256 * 255^2), so its float32 sums are exact in any order and float(uint32) has the reference's bits.  The handle
 * knob "byte_query_int" (a mask over the beam classes ef <= 64 / <= 128 / <= 1 024; 0 = never) switches that first pass off: the byte-walk
 * instances then serve the call on the widened copy.  gbnns_profile.project_ms of a PLAIN call is the widening kernel's time.
 * Refused: a float handle and a non-NULL args->queries with GBNNS_ERR_INVALID; whatever the corresponding float call refuses, with that
 * call's own code.  The gbnns_multi_* searches, gbnns_rerank, gbnns_rerank_topk and gbnns_project have no byte-query form. */
int gbnns_search_byte_queries(gbnns_index* index, const gbnns_search_args* args, const uint8_t* queries_u8, const uint32_t* query_tags, int k,
                              uint32_t* out_top_ids, float* out_top_dist);

/* Per-kernel device timing (hipEvent pairs on the launch stream), accumulated since the last
 * reset.  Reading synchronises the recorded events. */
typedef struct {
    uint32_t struct_size;         /* in: the caller's sizeof(gbnns_profile) (0 = the 160-byte layout of rounds 1-4, which ends before
                                     project_kernel; 192 = the layout that ends before retry_kernel); out: the bytes gbnns_profile_read filled in -- never more than the caller said */
    uint32_t calls;               /* search calls accumulated */
    double project_ms;            /* MLP layers + normalise */
    double walk_ms;               /* LDS-resident beam-walk kernel */
    double walk_general_ms;       /* exact general-case kernel (queries the LDS kernel handed over) */
    double rerank_ms;             /* original-space re-rank kernel (~0 when the walk kernels re-rank: then it is part of walk_ms) */
    double total_ms;              /* first launch .. last launch of each call */
    uint64_t queries;             /* queries processed */
    uint64_t general_queries;     /* of which were (re)run by the general kernel */
    char walk_kernel[96];         /* first-pass walk kernel of the last profiled call, template arguments included */
    char project_kernel[32];      /* kernel family of the handle's last projection: "mlp_net_kernel" (one launch) or "mlp_layer_kernels" */
    /* The retry pass of the last profiled call (304-byte layout; a caller that says 192 gets the fields above only).  The first pass
     * hands the queries its visited set cannot finish to the retry pass (list A), which walks them again with a CU's whole LDS and
     * hands what it cannot finish either on to the general kernel (list B). */
    char retry_kernel[96];        /* retry-pass kernel that call launched, template arguments included; empty when it launched none (batches of
                                     a beam that have been calm, a retry pass with nothing to gain, the general kernel taking the whole batch) */
    uint64_t retry_queries;       /* queries the first pass of that call handed over */
    uint64_t retry_general_queries; /* of those, how many went on to the general kernel (all of them when no retry kernel was launched) */
} gbnns_profile;

int gbnns_profile_enable(gbnns_index* index, int on);
/* Diagnostic knobs (tests, A/B runs); results never depend on them.  Since round 6 every knob that steers a handle's searches
 * belongs to the handle: gbnns_index_knob(index, name, value) sets it for that handle alone, and gbnns_debug_knob(name, value)
 * only changes the process-wide DEFAULT a handle created afterwards starts from (initial defaults: the environment variables
 * named below).  Two handles of one process can therefore run with different settings side by side.  The three "knn_*" knobs
 * steer gbnns_exact_knn, which has no handle, and stay process-wide (gbnns_debug_knob only).
 * "coop": the two-wavefront walk for small batches (one query per workgroup of two wavefronts: one keeps the result lists, one
 * expands the predicted next node) -- -1 (default) where the shape has it and the batch leaves the room, 0 never,
 * 1 wherever the shape has it (GBNNS_COOP).
 * "quotient": 0 keeps the walk_hot*
 * kernels' visited set in its packed form (default 1: the denser quotient form where it fits; initial value from the
 * environment variable GBNNS_QUOTIENT).  "vs_disp": probe number at which a probe sequence of the quotient form gives
 * up and the id goes to the stash / the query is handed over, 1 .. 15 (default 15; <= 0 restores it; GBNNS_DEBUG_VS_DISP).
 * "max_waves": most first-pass wavefronts per CU the LDS shares are cut for (0 = default; GBNNS_MAX_WAVES).
 * "spec_min_nq": smallest batch whose ef <= 64 first pass requests a hop's rows before its visited test
 * (walk_hot_spec_kernel; default 32 768, 0 = never; GBNNS_SPEC_MIN_NQ) -- on indexes whose visited sets are not in the
 * quotient form (more than 2^21 rows or so), unless "spec_any_form" is 1 (tests; GBNNS_SPEC_ANY_FORM).
 * "spec_tail": a synchronous call whose last round of wavefronts fills at most this many percent of the device's 8 192
 * slots runs that round with the rows requested before the visited test, and a synchronous batch of at most 60 % of the
 * slots runs so throughout (default 50, 0 = neither; GBNNS_SPEC_TAIL).
 * "mlp_small": smallest batch in flight (GBNNS_FLAG_DEFER_JOIN) whose hidden projection layers run on the small-footprint
 * kernel (mlp_layer_sw_kernel; default 4 096, up to 32 times that, 0 = never; GBNNS_MLP_SMALL).
 * "mlp_net": 1 (default) = batches of 2 048 queries and more whose net has d % 8 == 0 and d_hidden % 8 == 0 are projected
 * by the one-launch kernel (mlp_net_kernel: the three layers of a strip of queries in one workgroup, activations in LDS),
 * 0 = always the per-layer kernels; identical outputs either way (GBNNS_MLP_NET).  The kernel has two forms: workgroups of a
 * whole CU (8 wavefronts) and of half a CU (4 wavefronts, at most 80 KB of LDS: nets up to 256 hidden units or so), which a
 * batch in flight (GBNNS_FLAG_DEFER_JOIN) takes where it fits -- its workgroups start on CUs the other batches' walks have half
 * left.  2 = always the whole-CU form, 3 = the half-CU form wherever it fits.  "mlp_net_form" (gbnns_index_knob_get only): the
 * form of the handle's last one-launch projection, 0 whole-CU, 1 half-CU, -1 none yet.  "cus" (gbnns_index_knob_get only): the
 * compute units of the handle's device, which the projection's launch rules count rounds of the machine in.
 * "mlp_slab": 1 (default) = a projection layer that is one round of the machine for mlp_slab_kernel (small batches; the GIST
 * shape's 1 000 queries through 960 -> 1 024 -> 1 024 -> 64) takes it, 0 = never; identical outputs either way (GBNNS_MLP_SLAB).
 * "late_rows": the wide-row instances that have both forms (walk_reg_wide_kernel: 192- / 256-byte rows at ef <= 64; the two-list kernel
 * over 576-byte rows) request a hop's rows before its visited test (0) or after it, for the new ids only (1); -1 (default) = by
 * shape and residency (576-byte rows with at least five wavefronts per CU, 192-byte rows at ef <= 64: after; GBNNS_LATE_ROWS).
 * "hot": 0 = the first pass takes the generic register-list / two-list instances also where the plan has a hand-laid-out walk_hot* or
 * walk_reg_wide instance (default 1; GBNNS_HOT) -- the family the tag instances of gbnns_search_tagged are built from, untagged, for A/B runs.
 * "knn_chunk": most base rows per filtered chunk of gbnns_exact_knn (default 32 768; the pool path, and every chunk of
 * gbnns_exact_knn_bytes, takes four times that; GBNNS_KNN_CHUNK).
 * "knn_pool_min_k": shortest list gbnns_exact_knn's filter path and gbnns_exact_knn_bytes keep as an unordered pool with a
 * radix select (one wavefront per query) instead of a binary heap (default 64; GBNNS_KNN_POOL_MIN_K).
 * "knn_filter": gbnns_exact_knn's matrix-core filter -- 0 never, 1 by size (default), 2 whenever the shape allows
 * (GBNNS_KNN_FILTER).
 * "knn_slab": most queries gbnns_exact_knn's pool path and gbnns_exact_knn_bytes serve at a time -- 0 (default) = as many as keep their
 * key lists within 4 GiB (the slab formula at gbnns_exact_knn_bytes); v > 0 caps a slab at max(128, v & ~127) queries, so that a few
 * hundred queries already run several slabs (tests).  gbnns_debug_knn_slab reports the slab of a shape.
 * "gather_budget" (handle knob): list entries the id lists of one round of gbnns_index_exact_knn_gather may hold together (default 2^26, at
 * least 1; the call never takes less than n; GBNNS_GATHER_BUDGET) -- not for tuning: a test forces several rounds at a few thousand rows.
 * "gather_timing" (handle knob): 1 = a gathered call times its stages with events, its rounds one after the other (default 0); the last
 * such call's figures through gbnns_index_knob_get only: "gather_census_us", "gather_fill_us", "gather_scan_us", "gather_rounds".
 * "order_min" (handle knob): smallest batch of a GBNNS_MODE_NET / GBNNS_MODE_LOWQ search over at least 16 walked coordinates that is walked
 * in locality order -- the batch sorted by the sign bits of its queries' first walked-space coordinates, so that wavefronts resident
 * together walk neighbouring regions; only the order of the work changes, every answer goes to its query's own slot (default 32 768,
 * 0 = never, negative values count as 0; GBNNS_ORDER_MIN).  "order_bits" (handle knob): the width of that key, 10 .. 16, clamped (default 12;
 * GBNNS_ORDER_BITS).  "order_last" (gbnns_index_knob_get only): the queries the handle's last search call walked in locality order -- its
 * batch size, or 0 when it was not ordered.  gbnns_index_knob_get(NULL, "order_min" / "order_bits", &v) reads the process-wide default;
 * every other name needs a handle. */
int gbnns_debug_knob(const char* name, int value);
int gbnns_index_knob(gbnns_index* index, const char* name, int value);   /* GBNNS_ERR_INVALID: not a handle knob */
int gbnns_index_knob_get(gbnns_index* index, const char* name, int* out_value);   /* the handle's current value */
int gbnns_profile_read(gbnns_index* index, gbnns_profile* out, int reset);
/* Diagnostic, no device needed: which first-pass walk kernel the library plans for a shape, and that instance's LDS bytes per wavefront
 * without the visited set.  The inputs are what a search derives from its index and arguments: metric, walked dimension and row stride
 * (floats, a multiple of 4), rows, adjacency stride (slots, a multiple of 16), auxiliary-graph stride (0: no GBNNS_FLAG_AUX_GRAPH), beam,
 * entry points per query, GBNNS_FLAG_WIDE_INDEX, the resolved "coop" / "late_rows" / speculative-rows decisions (0 / 1; the two-wavefront
 * walk only where the shape has it, as in a search), the pass (0 first pass, 1 bitmap first pass -- GBNNS_FLAG_BITMAP_PASS --, 2 retry
 * pass) and the bytes the bitmap pass reserves for the re-rank query.  `name` receives the kernel's name, template arguments included
 * ("walk_general_kernel" for several entry points per query); GBNNS_ERR_INVALID for inputs no index or search can produce. */
int gbnns_debug_walk_plan(int metric, uint32_t dim, uint32_t dstride, uint64_t n, uint32_t ell_stride, uint32_t aux_stride, int ef,
                          uint32_t n_entries, int force_wide, int coop, int late_rows, int spec_rows, int pass, uint32_t rr_reserve,
                          char* name, uint32_t name_bytes, uint64_t* lds_bytes);
/* Diagnostic, no device needed: the first-pass kernel a gbnns_search_tagged call of that shape gets ("walk_general_kernel": the whole
 * batch runs on the general kernel), rows requested before the visited test where an instance has both orders.  Inputs as for gbnns_debug_walk_plan. */
int gbnns_debug_tag_plan(int metric, uint32_t dim, uint32_t dstride, uint64_t n, uint32_t ell_stride, uint32_t aux_stride, int ef,
                         uint32_t n_entries, int force_wide, uint32_t rr_reserve, char* name, uint32_t name_bytes, uint64_t* lds_bytes);
/* The same for a gbnns_search_tagged call with GBNNS_FLAG_TAG_BRIDGE; *lds_bytes: that instance's LDS bytes per wavefront without the visited set. */
int gbnns_debug_bridge_plan(int metric, uint32_t dim, uint32_t dstride, uint64_t n, uint32_t ell_stride, uint32_t aux_stride, int ef,
                            uint32_t n_entries, int force_wide, uint32_t rr_reserve, char* name, uint32_t name_bytes, uint64_t* lds_bytes);
/* Diagnostic, no device needed: the first-pass kernel an untagged search of that shape gets on a byte handle (gbnns_index_create_bytes)
 * whose original dimension the chunk-pair re-rank serves (L2, d % 16 == 0) and whose call does not set GBNNS_FLAG_NO_FUSED_RERANK, and
 * whether that kernel re-ranks its own query (*fused = 1) or the stand-alone byte re-rank kernel follows it (*fused = 0: `name` is then
 * exactly gbnns_debug_walk_plan's).  Inputs as for gbnns_debug_walk_plan. */
int gbnns_debug_byte_plan(int metric, uint32_t dim, uint32_t dstride, uint64_t n, uint32_t ell_stride, uint32_t aux_stride, int ef,
                          uint32_t n_entries, int force_wide, int coop, int late_rows, int spec_rows, int pass, uint32_t rr_reserve,
                          char* name, uint32_t name_bytes, int* fused);
/* Diagnostic, no device needed: the distance form that re-ranks rows of d coordinates under `metric` -- float rows (bytes = 0) or the uint8
 * rows of a byte handle (bytes != 0) --, from the predicate every launcher, the pair kernels and the search itself decide with.  `name`: the
 * kernel gbnns_rerank launches ("rerank_pair_kernel<0>": two lanes per row; "rerank_kernel<1>": a lane per row; "rerank_bytes_pair_kernel";
 * "rerank_bytes_kernel<0>"; the argument is the metric; gbnns_rerank_topk runs the same form's k-answer kernel).  *deep: the 16-byte row loads
 * a lane has in flight in the first loop of its ladder -- 24 (L2, d >= 384) or 8 in the float pair form, 4 in the byte chunk-pair form, 0 a
 * lane per row.  *fused: 1 where a GBNNS_MODE_NET / GBNNS_MODE_LOWQ search may leave the re-rank of such rows to its walk kernels (the pair
 * forms; whether a call does depends on its flags, beam and LDS room as well), 0 where a re-rank launch always follows.  GBNNS_ERR_INVALID: a
 * null output, an unknown metric, d == 0. */
int gbnns_debug_rerank_plan(int metric, uint32_t d, int bytes, char* name, uint32_t name_bytes, int* deep, int* fused);
/* The same for the binary16 rows of a half-base handle (gbnns_index_create_half_base), from the predicate its launchers and the search decide
 * with.  `name`: the kernel gbnns_rerank launches ("rerank_half_pair_kernel": L2, d % 4 == 0, two lanes per row, a 16-byte chunk of eight
 * halves at a time; "rerank_half_kernel<0>" / "rerank_half_kernel<1>": a lane per row -- L2 with a d % 4 tail, the negative dot).  *deep: the
 * 16-byte row loads a lane has in flight in the first loop of its ladder (the measured depth for d >= 384, 4 below, 0 a lane per row).
 * *fused: always 0 -- no walk kernel re-ranks half rows, a re-rank launch always follows.  GBNNS_ERR_INVALID: a null output, an unknown
 * metric, d == 0. */
int gbnns_debug_half_base_plan(int metric, uint32_t d, char* name, uint32_t name_bytes, int* deep, int* fused);
/* Diagnostic, no device needed: the first-pass kernel a GBNNS_MODE_PLAIN call with GBNNS_FLAG_BYTE_WALK of that shape gets on a byte handle
 * ("walk_general_kernel": the general kernel's byte-walk instance takes the whole batch) and its LDS bytes per wavefront without the
 * visited set.  `dim` is the original dimension -- the walked row is round_up(dim, 16) bytes --, `tagged` != 0 a gbnns_search_tagged call;
 * the other inputs as for gbnns_debug_walk_plan. */
int gbnns_debug_byte_walk_plan(int metric, uint32_t dim, uint64_t n, uint32_t ell_stride, uint32_t aux_stride, int ef, uint32_t n_entries, int force_wide,
                               int tagged, char* name, uint32_t name_bytes, uint64_t* lds_bytes);
/* Diagnostic, no device needed: the same for a GBNNS_MODE_PLAIN call with GBNNS_FLAG_HALF_WALK on a half-base handle (knob "half_walk_fast" = 2: every
 * first-pass instance the library has, also those of a dimension class the default, 1, leaves to the general instance).
 * `dim` is the original dimension -- the walked row is round_up(dim, 8) halves. */
int gbnns_debug_half_walk_plan(int metric, uint32_t dim, uint64_t n, uint32_t ell_stride, uint32_t aux_stride, int ef, uint32_t n_entries, int force_wide,
                               int tagged, char* name, uint32_t name_bytes, uint64_t* lds_bytes);
/* The same for a gbnns_search_byte_queries call of that shape with the knob "byte_query_int" = 7 (every beam class): the integer instance
 * inside the byte-walk first pass's domain (its query lives in registers: 512 bytes of LDS less), "walk_general_kernel" outside it. */
int gbnns_debug_byte_query_plan(int metric, uint32_t dim, uint64_t n, uint32_t ell_stride, uint32_t aux_stride, int ef, uint32_t n_entries, int force_wide,
                                int tagged, char* name, uint32_t name_bytes, uint64_t* lds_bytes);
/* Diagnostic, no device needed: LDS bytes of a workgroup of the one-launch projection for a net d -> d_hidden -> d_hidden -> d_low, in
 * the whole-CU form (form 0) or the half-CU form (form 1), with a queries per lane (2 .. 5), and whether that form takes the net at all
 * (*admitted: a workgroup with a = 4 fits 160 KB / 80 KB). */
int gbnns_debug_net_lds(uint32_t d, uint32_t d_hidden, uint32_t d_low, int form, int a, uint64_t* lds_bytes, int* admitted);
/* Diagnostic, no device needed: the kernel instances the projection of a batch launches, in launch order -- what run_project decides for a
 * net d -> d_hidden -> d_hidden -> d_low, n_q queries, a device of `cus` compute units, a call in flight (GBNNS_FLAG_DEFER_JOIN, on a lane
 * stream) or not, GBNNS_FLAG_MFMA_PROJECTION or not, and the handle knobs "mlp_net" / "mlp_slab" / "mlp_small".  Buffers count as 16-byte
 * aligned, as the handle's are.  `names` receives the instances separated by '\n', template arguments as in the source --
 * "mlp_net_kernel<8, 5, 8, 2, 2>", "mlp_slab_kernel<2, 2, false, true>", "mlp_layer_vec_kernel<true, false>", "mlp_mfma_net_kernel<3>",
 * "normalize_kernel" (a launch of its own where normalizeVector is not fused) --, cut short and terminated when the buffer is too small.
 * The same pick functions the launchers switch on compute it.  GBNNS_ERR_INVALID: a null or empty buffer, a zero dimension or batch,
 * n_q >= 2^31, cus < 1, a knob value outside its range. */
int gbnns_debug_project_plan(uint32_t d, uint32_t d_hidden, uint32_t d_low, uint64_t n_q, int cus, int in_flight, int mfma, int mlp_net,
                             int mlp_slab, int mlp_small, char* names, uint32_t names_bytes);
/* The instances the handle's last projection (a GBNNS_MODE_NET search, gbnns_project) actually launched, as its launchers reported them:
 * same format; the empty string before the first one.  The knob "cus" (gbnns_index_knob_get only) is the compute-unit count the handle plans with. */
int gbnns_index_project_last(gbnns_index* index, char* names, uint32_t names_bytes);
/* The permutation the handle's last ORDERED search call walked its batch in (knobs "order_min" / "order_bits"; "order_last" tells whether
 * the very last call was one): out_order[b] = the query the b-th work item walked, copied to the host array from that call's lane once all
 * the work enqueued on the device has completed (a call in flight included).  capacity: the entries out_order holds; *out_n: that call's
 * n_q, the entries written.  GBNNS_ERR_INVALID: a null index or out_n, no ordered call yet (*out_n = 0), out_order NULL or too little room
 * (*out_n is set, nothing is copied: a caller may ask for the size first). */
int gbnns_index_order_last(gbnns_index* index, uint32_t* out_order, uint64_t capacity, uint64_t* out_n);
/* Diagnostic: the locality order alone, on the current device -- HOST queries [n_q x qstride] floats (qstride >= dim), the key the sign
 * bits of the first `bits` coordinates (clamped to 10 .. 16), coordinate 0 the most significant, a coordinate counting as 1 exactly where
 * it compares > 0.  out_order [n_q] receives a permutation of 0 .. n_q-1 with non-decreasing keys; the order inside a bucket is not
 * defined.  GBNNS_ERR_INVALID: a null pointer, dim == 0, qstride < dim, n_q == 0 or >= 2^31, bits < 0; GBNNS_ERR_HIP ("invalid argument"):
 * dim < bits after clamping, the sort's own refusal. */
int gbnns_debug_query_order(const float* queries, uint32_t qstride, uint32_t dim, uint64_t n_q, int bits, uint32_t* out_order);

/* hnswlikeGD (support_func.h:521-575, need_const_degree = false) + addReverseEdgesForGD
 * (:402-445): prunes a kNN graph (CSR, host) over `ds` [n x d] (host) into the search graph, as
 * prepare_graph.cpp:70 does with M = 30, reverse = true.  Host code (OpenMP); returns malloc'ed
 * CSR arrays the caller releases with gbnns_free. */
int gbnns_build_graph_gd(const uint64_t* knn_offsets, const uint32_t* knn_nbrs, const float* ds,
                         uint64_t n, uint32_t d, int M, int metric, int reverse, int threads,
                         uint64_t** out_offsets, uint32_t** out_nbrs);
void gbnns_free(void* p);

/* The same builder with the per-node pruning (support_func.h:528-563) on the device, one node per wavefront.
 * The reference sorts a node's candidates with std::sort on the distance alone, which leaves the order of EQUAL
 * distances to the library's algorithm; nodes whose list contains equal distances (and lists longer than 1024)
 * are therefore finished on the host by that very call, so the result is always the host builder's, bit for bit.
 * The reverse-edge pass (:402-445) is serial and order dependent and stays on the host.  *out_host_nodes
 * (optional) = nodes that went to the host.  M > 64 or d > 128: everything runs on the host. */
int gbnns_build_graph_gd_device(int device, const uint64_t* knn_offsets, const uint32_t* knn_nbrs, const float* ds,
                                uint64_t n, uint32_t d, int M, int metric, int reverse, int threads,
                                uint64_t** out_offsets, uint32_t** out_nbrs, uint64_t* out_host_nodes);

/* Exact brute-force nearest neighbours on the device, in the reference's distance arithmetic.
 *   k = 1: getTruth (support_func.h:270-290) -- the strict minimum of Dist(base_j, q_i) over ascending j;
 *   k > 1: the exact kNN lists that feed the graph builder (dim_red/support_func.py:374-384 writes
 *          `<name>_knn_1k_<style>.ivecs`, prepare_graph.cpp:66 reads it).
 * out_ids [n_q x k] (and optional out_dist): the k smallest (distance, id) pairs of each query in ascending
 * pair order, ties towards the lower id; 0xFFFFFFFF / +inf where fewer than k rows qualify.
 * self_offset >= 0 says query i IS base row i + self_offset and must not be reported as its own neighbour
 * (kNN graph of a set over itself, possibly computed in slices of queries); -1 turns that off.
 * Large L2 problems (d % 4 == 0, d <= 128, n >= 2^17, n_q >= 2048, k <= 4096) go through a matrix-core filter first
 * (v_mfma_f32_32x32x16_bf16 on hi / lo bf16 halves, error-bounded) and only the rows it cannot rule out get their exact
 * distance: same output, byte for byte, several times faster.  Lists of 64 entries and more are kept as
 * unordered pools with a radix select per chunk (one wavefront per query) instead of binary heaps: 1 000-NN lists of
 * 10^6 x 32 in 1.4 s (7.6 s).
 * d <= 8192 (d > 128 runs a kernel that streams the query through in chunks); GBNNS_METRIC_NEG_DOT needs
 * d % 8 == 0 (else GBNNS_ERR_UNSUPPORTED).  Buffers are all host or all
 * device (mem_kind); the work runs on `stream` and the call returns when it has finished (a k x n_q x 8-byte
 * workspace lives for the duration of the call). */
int gbnns_exact_knn(int device, const float* base, uint64_t n, const float* queries, uint64_t n_q,
                    uint32_t d, int k, int metric, int64_t self_offset, uint32_t* out_ids, float* out_dist,
                    int mem_kind, void* stream);

/* gbnns_exact_knn over uint8 rows (SIFT / BIGANN .bvecs tables: the ground truth and the kNN lists a byte index needs), without a float
 * copy of anything: the result -- ids, and the bit patterns of out_dist -- is that of
 * gbnns_exact_knn(float(base), float(queries), ...), argument for argument (rows dense, d bytes each; L2 over the first 4 floor(d / 4)
 * dimensions; GBNNS_METRIC_NEG_DOT needs d % 8 == 0).  For bytes and d <= 256 every intermediate of the reference's distance is an integer
 * below 2^24 (sums <= 256 * 255^2 = 16 646 400), so its float arithmetic is exact in any order and the int32 result of the int8 matrix
 * cores (v_mfma_i32_32x32x32_i8 on x - 128) is that distance itself: one matrix product per pair, no error bound, nothing to rescore.
 * One scheme for every shape: the rows in chunks, a query's rows at or below its current k-th distance appended as keys, the keys offered
 * to a heap (k < "knn_pool_min_k") or an unordered pool with a radix select; a chunk that overflows a query's key list is swept again in
 * pieces that cannot.  GBNNS_ERR_UNSUPPORTED: d > 256 (the 2^24 bound), k > 4096 -- widen the rows and call gbnns_exact_knn.  No CPU path.
 * Device workspace for the duration of the call, dp = d rounded up to 32, cap = 4 k + 64, slab = min(n_q, max(1024, floor(2^32 / (8 cap)) & ~127))
 * queries served at a time (gbnns_exact_knn's pool path: the same with 4 cap; the knob "knn_slab" caps both):
 * n dp + 4 (n + 64) bytes of packed rows and row terms, and slab (dp + 8 cap + 8 k + 20) bytes of packed queries, key lists and
 * heaps / pools; HOST buffers add n d + n_q d bytes of uploaded rows and 4 (or 8) n_q k bytes of results. */
int gbnns_exact_knn_bytes(int device, const uint8_t* base, uint64_t n, const uint8_t* queries, uint64_t n_q,
                          uint32_t d, int k, int metric, int64_t self_offset, uint32_t* out_ids, float* out_dist,
                          int mem_kind, void* stream);
/* Diagnostic, no device needed: what gbnns_exact_knn_bytes does with a shape under the current "knn_chunk" / "knn_pool_min_k" knobs --
 * the padded row bytes (*dp, a multiple of the K step 32), a query's key slots per chunk (*cap), the rows of the first chunk, swept with
 * thresholds at "everything passes" (*first_rows <= *cap; also the piece length when a chunk is swept again), the most rows of a later
 * chunk (*max_chunk = 4 "knn_chunk"; a chunk is never longer than everything before it) and whether lists are pools (*pool).
 * GBNNS_ERR_INVALID for a shape the call refuses. */
int gbnns_debug_knn_bytes_plan(uint64_t n, uint64_t n_q, uint32_t d, int k,
                               uint32_t* dp, uint32_t* cap, uint64_t* first_rows, uint64_t* max_chunk, int* pool);
/* Diagnostic, no device needed: the queries a call with n_q queries and lists of k serves at a time under the current "knn_slab" knob --
 * bytes = 1: gbnns_exact_knn_bytes and its tagged / handle forms (keys of 8 bytes), bytes = 0: the pool path of gbnns_exact_knn (keys of 4).
 * *slab = n_q, or a multiple of 128.  GBNNS_ERR_INVALID: k outside 1 .. 4096, n_q >= 2^31. */
int gbnns_debug_knn_slab(int bytes, uint64_t n_q, int k, uint32_t* slab);
/* Diagnostic, no device needed: the kernel that sweeps the rows of an exact-kNN call of that shape under the current "knn_filter" /
 * "knn_pool_min_k" knobs, template arguments included, and whether the lists are pools (*pool = 1) or heaps (0).  bytes = 0:
 * gbnns_exact_knn -- "knn_filter_kernel<KSTEPS, QB, TAG>" where the matrix-core filter takes the call (the first rows of its heap path,
 * and a chunk whose lists overflowed, still go through the scan), else "knn_scan_kernel<METRIC, S, QPT, TAG>" (d <= 128) or
 * "knn_scan_wide_kernel<METRIC, R, TAG>"; bytes = 1: gbnns_exact_knn_bytes -- "knn_bytes_sweep_kernel<KSTEPS, QB, TAG>".  tagged != 0:
 * the _tagged call (gbnns_index_exact_knn with query_tags).  The name comes from the decision and the table the call itself launches
 * from.  GBNNS_ERR_INVALID / GBNNS_ERR_UNSUPPORTED for a shape the call refuses. */
int gbnns_debug_knn_plan(int bytes, int metric, uint64_t n, uint64_t n_q, uint32_t d, int k, int tagged, char* name, uint32_t name_bytes,
                         int* pool);
/* Diagnostic, no device needed: the dedupe table of a gbnns_index_tag_census over n_q queries has *cap slots (a power of two >= 2 n_q,
 * at least 64) and a query word's probe sequence starts at *slot, going up by one and wrapping at *cap -- so that a test can build
 * colliding words without restating the hash.  GBNNS_ERR_INVALID: n_q outside 1 .. 2^30. */
int gbnns_debug_census_slot(uint32_t word, uint64_t n_q, uint32_t* slot, uint32_t* cap);

/* Exact TAGGED nearest neighbours: the exact answer of a tagged query -- the ground truth of gbnns_search_tagged and of
 * GBNNS_FLAG_TAG_BRIDGE, and what a caller falls back to when a filter is selective.  Row j is allowed for query i when
 * (row_tags[j] & query_tags[i]) != 0, gbnns_search_tagged's test.  The result of query i is that of gbnns_exact_knn (gbnns_exact_knn_bytes)
 * over the rows allowed for i, reported under their original ids: the k smallest (Dist(base_j, q_i), j) pairs among the allowed j in
 * ascending pair order, ties towards the lower id, the distances in the reference's arithmetic.  Where fewer than k rows are allowed the
 * rest is 0xFFFFFFFF / +inf; a query with query_tags[i] == 0 gets nothing else (data, not an error).  self_offset keeps its meaning in
 * original ids: row i + self_offset is dropped whether allowed or not.  With every word of both tag arrays all ones every output byte is
 * the untagged call's; the byte form equals the float form on the widened arrays, ids and distance bits.
 * Arguments, refusals and status codes are those of the untagged twins; row_tags [n] and query_tags [n_q] are buffers of mem_kind, a NULL
 * one is GBNNS_ERR_INVALID.  The same kernels with a compile-time tag test: a disallowed row is not offered by the scan, a disallowed pair
 * is not a hit of the matrix-core sweeps (neither counted nor stored), so thresholds come from lists of allowed rows and a later chunk
 * keeps about k ALLOWED rows per query.  Workspace beside the untagged call's: 4 (n + 64) bytes of padded row tags (and 4 n_q for HOST). */
int gbnns_exact_knn_tagged(int device, const float* base, uint64_t n, const float* queries, uint64_t n_q, uint32_t d, int k, int metric,
                           int64_t self_offset, const uint32_t* row_tags, const uint32_t* query_tags,
                           uint32_t* out_ids, float* out_dist, int mem_kind, void* stream);
int gbnns_exact_knn_bytes_tagged(int device, const uint8_t* base, uint64_t n, const uint8_t* queries, uint64_t n_q, uint32_t d, int k, int metric,
                                 int64_t self_offset, const uint32_t* row_tags, const uint32_t* query_tags,
                                 uint32_t* out_ids, float* out_dist, int mem_kind, void* stream);
/* The same computation over a handle's resident original-space table, read in place at its device row stride (d_pad floats on a float
 * handle, d_pad bytes on a byte handle): nothing of the table is uploaded and no float copy of a byte table is made.  The handle's metric.
 * Exactly one of queries [n_q x d] float32 / queries_u8 [n_q x d] uint8 is non-NULL (else GBNNS_ERR_INVALID): a float handle takes
 * `queries` (queries_u8 there: GBNNS_ERR_INVALID, as in gbnns_search_byte_queries), a byte handle takes queries_u8 (`queries` there:
 * GBNNS_ERR_UNSUPPORTED -- there is no mixed-pair scan).  query_tags [n_q] != NULL: the tagged answer over the table of
 * gbnns_index_set_tags (without one: GBNNS_ERR_INVALID, as in gbnns_search_tagged); NULL: the untagged answer, no tag table needed.
 * queries, query_tags and the outputs are buffers of mem_kind.  The result is byte-identical to the free function's on the same table and
 * tags.  The call obeys the stream rule above (it is ordered after a gbnns_index_set_tags on that stream), first joins the
 * GBNNS_FLAG_DEFER_JOIN calls still owed, allocates its packed workspace per call, uses none of the lanes' workspaces, and returns when
 * the work has finished, as gbnns_exact_knn does.  There is no deferred form and no gbnns_multi_* form. */
int gbnns_index_exact_knn(gbnns_index* index, const float* queries, const uint8_t* queries_u8, uint64_t n_q, const uint32_t* query_tags,
                          int k, int64_t self_offset, uint32_t* out_ids, float* out_dist, int mem_kind, void* stream);

/* The census of the tag table T of gbnns_index_set_tags, exact: for every query word Q[i] of query_tags [n_q]
 *     out_allowed[i] = |{ j : (T[j] & Q[i]) != 0 }|      out_first[i] = the lowest such j, 0xFFFFFFFF when there is none.
 * Both outputs are [n_q] buffers of mem_kind; either may be NULL, not both.  GBNNS_ERR_INVALID without a tag table, on NULL query_tags with
 * n_q > 0 and for n_q >= 2^31; n_q == 0 returns GBNNS_OK and does nothing.  With DEVICE buffers the work is enqueued on `stream` under the
 * stream rule of gbnns_index_exact_knn (ordered after a gbnns_index_set_tags on that stream; the deferred calls still owed are joined) and
 * the call does not synchronise; with HOST buffers it is synchronous.  Nothing is cached across calls: gbnns_index_set_tags may change
 * the table at any time.  The device work is n x U for the U DISTINCT words of the batch, not n x n_q (tag_census.hip: the words are
 * deduplicated on the device, then every workgroup runs the U words over a tile of the table held in registers).  Workspace on the handle:
 * 44 .. 76 bytes per query. */
int gbnns_index_tag_census(gbnns_index* index, const uint32_t* query_tags, uint64_t n_q, uint32_t* out_allowed, uint32_t* out_first,
                           int mem_kind, void* stream);

/* Tagged search that routes itself: the census above, then per query the exact scan (gbnns_index_exact_knn with query_tags) or the tagged
 * walk (gbnns_search_tagged, or on a byte handle gbnns_search_byte_queries with query_tags), entered at an allowed row.
 *   - Routing rule: query i takes the scan when allowed[i] <= scan_below, boundary included -- a query that may see nothing has count 0
 *     and always scans; otherwise it takes the walk.  scan_below has no default: 0 sends only the empty queries to the scan, UINT64_MAX
 *     every query.  out_allowed [n_q] (the census count) and out_route [n_q] (0 = walk, 1 = scan) are optional.
 *   - A scan-routed query: row i of out_top_ids / out_top_dist ([n_q x k]; dist optional) is row i of gbnns_index_exact_knn(index, ...,
 *     query_tags, k, self_offset = -1) -- ascending (distance, id), padded with 0xFFFFFFFF / +inf --, args->out_ids[i] is column 0 of that
 *     row, and the walk-only outputs of `args` hold the bad-entry row of a tagged call: out_cand all 0xFFFFFFFF, out_cand_dist +inf, hops,
 *     dist_calc and edges 0.
 *   - A walk-routed query: every output is that query's row of gbnns_search_tagged(index, args', query_tags, k, ...), args' = args except
 *     for the entry points: with args->entry_ids == NULL query i enters at first[i], the lowest row it may see, so no walk-routed query has
 *     a disallowed entry; entry_ids given are used as they are, under the rules of a tagged call.  GBNNS_FLAG_TAG_BRIDGE keeps its meaning.
 *   - out_q_low (NET mode) is every query's projection, whichever its route.
 * Queries are independent in both calls, so every row of this call is bit for bit a row of one of the two; nothing new is defined about
 * arithmetic.  A float handle takes args->queries (queries_u8 there: GBNNS_ERR_INVALID); a byte handle takes queries_u8 with args->queries
 * NULL (float queries there: GBNNS_ERR_UNSUPPORTED, there is no mixed-pair scan).  In LOWQ mode queries_low serves the walk, the
 * original-space queries the scan and the re-rank.
 * Refused before any work, whatever the data -- everything either route would refuse: PLAIN mode, k outside 1 .. min(ef, 4096), no tag
 * table, NULL query_tags / out_top_ids: GBNNS_ERR_INVALID; GBNNS_FLAG_HALF_ROWS / GBNNS_FLAG_MFMA_PROJECTION, d > 256 on a byte handle, the
 * negative dot with d % 8 != 0, gbnns_search_topk's LDS limit, and GBNNS_FLAG_DEFER_JOIN (the call reads the census on the host):
 * GBNNS_ERR_UNSUPPORTED.  HOST buffers are uploaded, served by the same path and downloaded.  The call returns when its work has finished,
 * as gbnns_index_exact_knn does; there is no gbnns_multi_* form, and gbnns_profile sees the walk only. */
int gbnns_search_tagged_auto(gbnns_index* index, const gbnns_search_args* args, const uint8_t* queries_u8, const uint32_t* query_tags, int k,
                             uint64_t scan_below, uint32_t* out_top_ids, float* out_top_dist, uint32_t* out_allowed, uint8_t* out_route);

/* Gathered exact tagged kNN: gbnns_index_exact_knn(index, ..., query_tags, ...) computed from distances to the rows a query's tag word
 * allows and to no others.  Every output byte is what gbnns_index_exact_knn returns for the same arguments on the same handle: each row
 * holds the k smallest (Dist, id) pairs among the rows with (T[j] & Q[i]) != 0, distances in the reference's arithmetic, ties towards the
 * lower id, padded with 0xFFFFFFFF / +inf; self_offset in original ids; the handle's metric; float and byte handles; the same stream rule
 * (the deferred calls still owed are joined; the call returns when the work has finished).  Opt-in: nothing else calls it unless
 * GBNNS_FLAG_SCAN_GATHER asks.
 *   Pipeline (one host round trip): the census of gbnns_index_tag_census gives allowed[i]; the host groups the queries by word and deals
 *   the groups into rounds whose id lists together fit "gather_budget" list entries (a handle knob: default 2^26 = 256 MiB, never less than
 *   n; a test's means to force several rounds, not a tuning knob); per round one kernel writes the allowed row ids of every distinct word
 *   of the round into the word's list (in whatever order its atomics give: selection is by the (distance, id) key) and one kernel lets the
 *   queries of a word scan the word's list -- gbnns_exact_knn's scan loop with the rows read through the list, the same operations in the
 *   same order per distance; byte rows are widened while they are staged (every partial sum is an integer below 2^24: exact), no float copy
 *   of a byte table, no packed copy of any table.  Work: sum over the queries of allowed[i] x d, plus n x U for the U distinct words.
 *   Covered by the gathered kernel: d <= 128, L2 at any d, the negative dot at d % 8 == 0, 1 <= k <= 4 096 (heaps; k >= 64 is untuned: there
 *   is no pool path).  Any other shape the call accepts is NOT refused: the same call runs gbnns_index_exact_knn's scan and returns the same
 *   bytes (gbnns_debug_gather_plan tells which).
 * Refusals and status codes are gbnns_index_exact_knn's, and one more: query_tags == NULL is GBNNS_ERR_INVALID (an untagged call has nothing
 * to gather).  Workspace per call: the heaps (8 k bytes a query), the census' workspace, 16 bytes a query, 44 bytes a distinct word, and the
 * largest round's lists (4 bytes an entry). */
int gbnns_index_exact_knn_gather(gbnns_index* index, const float* queries, const uint8_t* queries_u8, uint64_t n_q, const uint32_t* query_tags,
                                 int k, int64_t self_offset, uint32_t* out_ids, float* out_dist, int mem_kind, void* stream);
/* gbnns_search_tagged_auto only: the scan-routed queries are served by gbnns_index_exact_knn_gather's computation instead of
 * gbnns_index_exact_knn's.  Every output is unchanged.  In every other search call the flag is GBNNS_ERR_INVALID, like GBNNS_FLAG_TAG_BRIDGE
 * outside the tagged calls. */
#define GBNNS_FLAG_SCAN_GATHER 4096u
/* Diagnostic, no device needed: the kernel instance that serves a gbnns_index_exact_knn_gather call on a float (bytes = 0) or byte (1) handle
 * of that metric, d and k -- "knn_gather_kernel<METRIC, S, QPT, U8>" with *queries_per_workgroup = W, the queries one of its workgroups serves;
 * or, for a shape the gathered kernel does not cover (d > 128, k > 4 096), the tagged instance of the existing scan ("knn_scan_wide_kernel<...>",
 * "knn_bytes_sweep_kernel<...>", ...) with W = 0: the fallback.  GBNNS_ERR_INVALID / GBNNS_ERR_UNSUPPORTED for a shape the call refuses. */
int gbnns_debug_gather_plan(int bytes, int metric, uint32_t d, int k, char* name, uint32_t name_bytes, uint32_t* queries_per_workgroup);
/* Diagnostic, no device needed: the schedule gbnns_index_exact_knn_gather builds -- the very host function -- from the queries' words [n_q] and
 * census counts allowed [n_q] (each <= n), a budget of list entries per round and W queries per workgroup.
 *   Groups: the queries with allowed > 0 by word, groups in ascending word order, queries inside a group in ascending index.  A word that
 *   allows nothing has no group.  order [n_q]: the permutation that lists the groups' queries in that order, then the queries without a group
 *   in ascending index.
 *   Rounds: the groups, in order, fill a round while its lists' entries stay within `budget`; a group that does not fit opens the next
 *   round, so a group longer than the budget has a round of its own.  round_of [n_q]: the round of query i's group (0xFFFFFFFF: none);
 *   list_offset_of [n_q]: the first entry of its group's list in the round's list buffer (lists lie back to back in group order).
 *   Workgroups: a group of g queries takes ceil(g / W) workgroups on its one list.  *n_rounds, *n_workgroups: the totals.
 * GBNNS_ERR_INVALID: a NULL array, n outside [1, 2^32 - 1), n_q >= 2^31, W == 0, budget == 0, allowed[i] > n. */
int gbnns_debug_gather_schedule(const uint32_t* words, const uint32_t* allowed, uint64_t n_q, uint64_t n, uint64_t budget, uint32_t W,
                                uint32_t* order, uint32_t* round_of, uint64_t* list_offset_of, uint32_t* n_rounds, uint32_t* n_workgroups);

/* ---- several devices of one node: query-sharded replicas ----------------------------------------------------
 * The reference's only parallelism on this path is `#pragma omp parallel for` over the queries of a batch
 * (search_function.h:152; the loop body :348-385 is pure per query).  Here that loop is cut into contiguous blocks,
 * one per replica of the index: one gbnns_index per entry of `devices` (NULL / 0 = every visible device; an ordinal
 * may repeat: the replicas then share that device), each driven by its own host thread on its own HIP stream.
 * Nothing is exchanged while searching; results are combined as described per call.  desc as for
 * gbnns_index_create (HOST buffers; desc->device is ignored).  What the drop-in uses when GBNNS_DEVICES=0,1,...
 * names more than one device. */
typedef struct gbnns_multi gbnns_multi;
int gbnns_multi_create(const gbnns_index_desc* desc, const int32_t* devices, int32_t n_devices, gbnns_multi** out);
int gbnns_multi_destroy(gbnns_multi* multi);
int gbnns_multi_size(const gbnns_multi* multi);                    /* replicas */
gbnns_index* gbnns_multi_replica(gbnns_multi* multi, int32_t i);   /* borrowed */
int gbnns_multi_device_of(const gbnns_multi* multi, int32_t i);
void* gbnns_multi_stream(gbnns_multi* multi, int32_t i);           /* hipStream_t of replica i */
int gbnns_multi_set_aux_graph(gbnns_multi* multi, const uint64_t* offsets, const uint32_t* nbrs);
/* Block of part `part` of `parts` parts of a batch: [*lo, *hi), contiguous, sizes differ by at most one. */
void gbnns_shard_bounds(uint64_t n_q, int32_t parts, int32_t part, uint64_t* lo, uint64_t* hi);
/* One batch over all replicas, HOST buffers holding the WHOLE batch (args as gbnns_search_ex; args->stream is
 * ignored): replica r searches rows gbnns_shard_bounds(n_q, R, r) and writes its answers, counters and candidate
 * rows straight into the caller's arrays -- identical to what one gbnns_search_ex call would have written.
 * Returns when every replica has finished. */
int gbnns_multi_search_ex(gbnns_multi* multi, const gbnns_search_args* args);
/* Device-resident form (NET / PLAIN): query_blocks[r] = rows gbnns_shard_bounds(n_q, R, r) of the batch, resident on
 * replica r's device ([rows x d]); entry_blocks likewise or NULL; out_ids_all[r] = [n_q] uint32 on replica r's
 * device.  Every replica searches its block, then the answer ids are all-gathered (ONE ncclAllGather of uint32
 * per batch over RCCL / xGMI, sends padded to the largest block; librccl is loaded on first use; replicas must then
 * sit on distinct devices) so that every out_ids_all[r] holds the whole answer vector.  `args` supplies mode, ef,
 * k, flags, hops_bound, hash_capacity; its buffers and n_q are ignored.  Enqueued on the replicas' streams:
 * gbnns_multi_synchronize waits for them. */
int gbnns_multi_search_device(gbnns_multi* multi, const gbnns_search_args* args, uint64_t n_q,
                              const float* const* query_blocks, const uint32_t* const* entry_blocks,
                              uint32_t* const* out_ids_all);
int gbnns_multi_synchronize(gbnns_multi* multi);
/* A handle with ONE replica copies its answers instead of gathering them.  on != 0: it goes through the exchange leg as
 * well -- librccl loaded, a one-rank communicator (ncclCommInitAll over its device), ncclAllGather of the single block --
 * so that symbol resolution, stream order and the gather buffer's layout can be exercised on a one-GPU machine. */
int gbnns_multi_rccl_single_rank(gbnns_multi* multi, int on);
/* ncclGetVersion() of the librccl this handle has loaded (e.g. 22707), 0 while it has not loaded one. */
int gbnns_multi_rccl_version(gbnns_multi* multi);
const char* gbnns_multi_last_error(void);

int gbnns_device_count(void);
int gbnns_version(void);
const char* gbnns_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* GBNNS_H_ */
