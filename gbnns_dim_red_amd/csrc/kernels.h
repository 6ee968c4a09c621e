// kernels.h -- launch interface between the C-ABI host layer (handle.cpp, lanes.cpp, search_core.cpp, sizing.cpp, graph_api.cpp, pin.cpp) and the gfx950 kernels
// (the .hip units beside it: the walk units behind launch_walk, walk_general, rerank, mlp, gd_order, knn).  Plain structs of device pointers and sizes; no HIP
// types besides hipStream_t.  Which walk instance serves a shape, and its LDS layout, is walk_plan.h's.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "rerank_plan.h"

namespace gbnns {

constexpr uint32_t kInvalidId = 0xFFFFFFFFu;
constexpr int kWave = 64;
constexpr int kTieCap = 64;            // LDS tie list of the fast walk kernel (one slot per lane)
constexpr int kGeneralSlots = 64;      // persistent waves of the general walk kernel
constexpr int kRetrySlots = 256;       // persistent waves of the retry pass (one per CU: it takes all the LDS)

// Beam walk (search_function.h:43-102 + :15-40).  One query per wavefront.
struct WalkParams {
    const float* q;          // [nq x qstride] query vectors in the walked space
    uint32_t qstride;        // floats
    const float* db;         // [n x dstride] base vectors in the walked space (rows 16-B aligned)
    uint32_t dstride;        // floats, multiple of 4
    uint32_t dim;            // true dimension of the walked space
    const uint32_t* ell;     // [n x ell_stride] padded adjacency, kInvalidId-terminated rows
    uint32_t ell_stride;     // multiple of 16
    uint32_t n;
    uint32_t nq;
    int32_t ef;
    int32_t k;               // results kept (<= ef); cand_stride = min(k, ef)
    const uint32_t* entries; // [nq x n_entries] or nullptr (= node 0)
    uint32_t n_entries;      // entry points per query (0 / 1: one); more than one runs on the general kernel only
    // LDS visited set of the fast kernel
    uint32_t hash_cap;       // entries of the LDS visited set (any size >= 128)
    uint32_t hash_limit;     // max entries before a query is handed to the general kernel
    // outputs
    uint32_t* cand;          // [nq x cand_stride] pop order (worst -> best), kInvalidId pad
    float* cand_dist;        // optional, same shape
    uint32_t zero_dist_bits; // bit pattern of a zero distance on output: 0 (L2), 0x80000000 (negative dot: -0)
    uint32_t cand_stride;
    int32_t* count;          // [nq] valid entries in cand
    int32_t* hops;           // [nq]
    int32_t* dist_calc;      // [nq]
    int32_t* edges;          // optional [nq]: neighbour ids read (sum of degrees of expanded nodes)
    uint32_t* best;          // optional [nq]: id of the best result (PLAIN mode answer)
    // hand-over lists: first pass -> A -> retry pass (largest LDS visited set) -> B -> general kernel
    uint32_t* ovf_count;     // [1]   list A
    uint32_t* ovf_list;      // [nq]
    uint32_t* ovf2_count;    // [1]   list B
    uint32_t* ovf2_list;     // [nq]
    uint32_t* r_cursor;      // [1]   work-queue head of the retry pass
    // general kernel workspace: per slot [visited bits | tie bits: 2 x bitmap_words][keys ef]
    // first pass with the visited set in HBM (large ef): per-slot bitmaps and the work-queue head
    uint32_t* fp_bitmap;     // [slots x bitmap_words]
    uint32_t* fp_cursor;     // [1]
    uint32_t rr_reserve;     // bytes the bitmap first pass of the two-list kernel sets aside for the re-rank query (0: none)
    uint32_t* g_cursor;      // [1] work-queue head
    uint32_t* g_total;       // [1] running count of queries the general kernel processed
    uint32_t* max_dc;        // [1] max dist_calc over the batch (feeds the host's visited-set sizing)
    uint32_t* next_ctrl;     // [5] control words of the NEXT call: the general kernel clears them
    uint32_t* g_bitmap;      // [slots x 2 x bitmap_words]: visited bits, then the tie set (one bit per node)
    uint64_t* g_keys;        // [slots x (ef + n_entries - 1)]
    uint32_t bitmap_words;
    int32_t all_general;     // 1: the general kernel takes every query (fast kernel skipped)
    // fused re-rank (rr_db != nullptr): every walk kernel re-ranks its own query at the end of the walk
    // (pair form: rr_dim % 8 == 0; rr_dstride * 4 bytes of LDS available) and writes the answer to rr_out
    const float* rr_q;       // [nq x rr_qstride] original-space queries
    uint32_t rr_qstride;
    const float* rr_db;      // [n x rr_dstride] original-space vectors
    uint32_t rr_dstride, rr_dim, rr_n;
    int32_t rr_metric;       // gbnns_metric of the re-rank
    uint32_t* rr_out;        // [nq]
    // auxiliary graph (search_function.h:73-89, use_second_graph): while hops < hops_bound a node's auxiliary
    // row is expanded before its main row; with llf the main row is skipped when that step inserted anything
    const uint32_t* aux_ell; // [n x aux_stride] or nullptr (= use_second_graph false)
    uint32_t aux_stride;
    uint32_t hops_bound;
    int32_t llf;
    // visited-set form of the walk_hot* first pass: vs_shr == 0 -> five 24-bit ids per 16-byte bucket; else the quotient
    // form (seven 16-bit entries per bucket; n <= 2^W): vs_shr = (32 - W + floor(log2 buckets)) | (32 - W) << 8 |
    // (13 remainder bits ? 1 << 16 : 0) | limit << 28 (top four bits: a probe sequence gives up -- stash, hand-over -- when
    // its probe number reaches 15, or 7 << 1 with 13 remainder bits; less in test runs)
    uint32_t vs_shr;
    int32_t spec_rows;       // ef <= 64 hot first pass: 1 = request the rows before the visited test (big launches, see sizing.cpp)
    int32_t late_rows;       // generic two-list kernels over 192- / 256- / 576-byte rows: 1 = request a hop's rows after its visited test (new ids only)
    uint32_t spec_from;      // ... and in the tested-first instances, for the wavefronts from this work item on (the last, partial round
                             // of a launch walks a draining machine: the shorter hop wins there); 0xFFFFFFFF = none
    const uint32_t* order;   // optional [nq]: work item b of a first pass runs query order[b] (a permutation: locality order of a deep batch)
    int32_t coop;            // 1: the first pass is the two-wavefront walk (walk_coop.hip: kCoopExtraLds, walk_plan.h, more bytes of LDS per query)
    int32_t force_wide;      // diagnostic: treat the index as a large one (64-bit offsets, 4-byte visited-set slots)
    unsigned long long* stamps;  // diagnostic builds only (GBNNS_STAMPS): [32] segment cycle sums / histograms
    int32_t stamps_on;           // 1 in diagnostic builds: use the instrumented generic kernel
    // GBNNS_FLAG_HALF_ROWS (last, so that no other field moves): the walked table is R = float32(float16(db_low)) -- `db` above is then the
    // float32 copy of R, which every kernel but the half instances reads
    const void* db_h;        // [n x dstride] binary16 rows of R (dstride a multiple of 8, no padding), or nullptr
    int32_t half_rows;       // 1: the first pass takes a half instance where the plan has one (walk_plan.cpp)
    // gbnns_search_tagged (last again): row j is allowed for query i when (tags[j] & qtags[i]) != 0; the walk is the reference's on the graph
    // whose adjacency rows keep the allowed neighbours only -- a disallowed neighbour is an empty slot
    const uint32_t* tags;    // [n] tag word of every row, or nullptr
    const uint32_t* qtags;   // [nq] tag word of every query
    int32_t tagged;          // 1: the first pass takes a tag instance (walk_tag.hip) or the general kernel the whole batch (walk_plan.cpp)
    int32_t generic_only;    // diagnostic (knob "hot" = 0): the generic instances also where the plan has a walk_hot* / walk_reg_wide instance
    // GBNNS_FLAG_TAG_BRIDGE (last again; with `tagged`): a disallowed neighbour is looked through -- its place in the adjacency row is taken by
    // the allowed entries of its own row, one level deep (walk_bridge.hip)
    int32_t bridged;         // 1: the first pass takes a bridge instance (walk_bridge.hip) or the general kernel the whole batch (walk_plan.cpp)
    // gbnns_index_create_bytes (last again): the fused re-rank of the byte instances (walk_hot_bytes_kernel, walk_hot2_bytes_kernel,
    // walk_general_bytes_kernel) reads uint8 rows -- rr_db stays nullptr, rr_dstride is then the BYTES of a row (a multiple of 16, zero
    // padded) and the floats of the staged query, rr_dim % 16 == 0, rr_metric L2.  No other kernel looks at it.
    const uint8_t* rr_db_b;  // [n x rr_dstride] original-space byte rows, 16-byte aligned, or nullptr
    uint32_t bytes_dim;      // a byte handle's call that wants its re-rank fused: d of the uint8 rows (walk_plan.cpp: a byte instance where there is one); 0: not asked for
    // GBNNS_FLAG_BYTE_WALK (last again): a PLAIN walk over a byte handle's table -- the walked rows are uint8, `db` above is nullptr, `dstride`
    // is the BYTES of a row (round_up(dim, 16), zero padded) and the floats of the staged query.  The distances are the float walk's on
    // float32(db_b), operation for operation; no float copy of the table exists.
    const uint8_t* db_b;     // [n x dstride] walked byte rows, 16-byte aligned, or nullptr
    int32_t walk_bytes;      // 1: the first pass takes a byte-walk instance (walk_bytes.hip) or the general kernel's the whole batch (walk_plan.cpp)
    // gbnns_search_byte_queries (last again): the call brought its queries as uint8 -- `q` above is their float32 widening (widen.hip), which
    // every kernel reads but the integer byte-walk instances (walk_bytes_q.hip): those read the bytes themselves and compute the distance in
    // uint32, which for d <= 256 is the float walk's value exactly.
    uint32_t bq_classes;     // beam classes whose byte-walk first pass takes the integer instance: bit 0 one list register, bit 1 two, bit 2 the two-list kernel (in the struct's former tail padding)
    const uint8_t* q_b;      // [nq x dim] the queries as bytes, rows 16-byte aligned, or nullptr
    // GBNNS_FLAG_HALF_WALK (last again): a PLAIN walk over a half-base handle's table -- the walked rows are binary16, `db` above is nullptr,
    // `db_h` the handle's table (gbnns_index_create_half_base) and `dstride` the HALVES of a row (round_up(dim, 8), zero padded) = the floats
    // of the staged query.  The distances are the float walk's on float32(db_h), operation for operation; no float copy of the table exists.
    int32_t walk_half;       // 1: the first pass takes a half-walk instance (walk_half_base.hip) or the general kernel's the whole batch (walk_plan.cpp)
    int32_t half_general;    // (with walk_half) 1: the handle knob "half_walk_fast" is 0 -- the general kernel's instance takes the whole batch also where the plan has a fast one
    int32_t half_unkept;     // (with walk_half) 1: the knob is 2 -- also the fast instances of the dimension classes the measurement rule has not kept (walk_plan.cpp)
};
// uint8 -> float32, `count` values (every byte value is a binary32 value: nothing is rounded)
hipError_t launch_widen_u8(const uint8_t* src, float* dst, size_t count, hipStream_t s);

// `form` of a visited set: 0 = 4-byte slots, 1 = five 24-bit ids per 16-byte bucket, 2 = quotient form (seven 16-bit entries)
size_t walk_hash_bytes(uint32_t entries, int form);             // LDS bytes of a visited set of `entries` ids
uint32_t walk_hash_entries(size_t bytes, int form);             // ids that fit into `bytes` (whole buckets)
// Which instance runs a pass, and on what LDS layout: plan_walk (walk_plan.h).  launch_walk launches the plan's instance (bitmap first pass:
// `slots` persistent wavefronts) and fails with hipErrorInvalidValue when no unit holds it.
struct WalkPlan;
hipError_t launch_walk(const WalkPlan& pl, const WalkParams& p, unsigned slots, hipStream_t s);
const char* walk_plan_name(const WalkPlan& pl);   // printable name of the plan's instance, template arguments included (no device needed); nullptr: none
const char* walk_first_pass_name(hipStream_t s);  // (mangled) name of the first-pass kernel this thread launched last
const char* walk_retry_pass_name(hipStream_t s);  // ... and of the retry-pass kernel
hipError_t launch_walk_general(const WalkParams& p, int metric, hipStream_t s);  // (p.tagged: its instance with the tag test; p.bridged too: the one that looks through disallowed neighbours; p.walk_bytes: their byte-walk twins; p.walk_half: their half-walk twins)
// GBNNS_FLAG_HALF_ROWS (walk_half.hip): src [n x sstride] (dim coordinates a row) -> out_h [n x hstride] binary16 bits, round to nearest even,
// columns from dim on zero; out_f [n x fstride] the same values widened back (fstride <= hstride).  *bad_row (preset to 0xFFFFFFFF) receives the
// lowest row that holds a coordinate which is not finite or rounds out of the binary16 range.
hipError_t launch_half_rows_convert(const float* src, uint32_t sstride, uint32_t dim, uint64_t n, uint16_t* out_h, uint32_t hstride, float* out_f,
                                    uint32_t fstride, uint32_t* bad_row, hipStream_t s);

// Re-rank (search_function.h:105-125).  One query per wavefront, one candidate per lane.
struct RerankParams {
    const float* q;          // [nq x qstride] original-space queries
    uint32_t qstride;
    const float* db;         // [n x dstride]
    uint32_t dstride;        // floats, multiple of 4
    uint32_t dim;
    const uint32_t* cand;    // [nq x cand_stride] pop order
    uint32_t cand_stride;
    const int32_t* count;    // [nq]
    uint32_t nq;
    uint32_t n;              // rows of db (ids are clamped against it)
    uint32_t* out;           // [nq]
};
hipError_t launch_rerank(const RerankParams& p, int metric, hipStream_t s);
// The k best of every list instead of the best one: `out` is [nq x k] (ascending (distance, pop index); 0xFFFFFFFF from column count on),
// `out_dist` (optional) the distances' bits beside it (+inf from column count on).  1 <= k <= cand_stride; one wavefront per query.
struct RerankTopkParams : RerankParams {
    uint32_t k;
    float* out_dist;         // [nq x k] or nullptr
};
// (LDS of a workgroup: the staged query, cand_stride 8-byte keys -- an even number of slots: they are swept two at a time -- and 4-byte distances)
constexpr uint32_t rerank_topk_key_slots(uint32_t cand_stride) { return (cand_stride + 1u) & ~1u; }
size_t rerank_topk_lds(uint32_t dstride, uint32_t cand_stride);
hipError_t launch_rerank_topk(const RerankTopkParams& p, int metric, hipStream_t s);
// The same two over the uint8 rows of a byte handle (rerank_bytes.hip): `db` stays nullptr, `dstride` is the BYTES of a row -- round_up(dim, 16),
// zero padded, which is also the floats of the staged query -- and `k` / `out_dist` are read by the k-answer launch only.  The distances are
// the float kernels' on float32(db_b), bit for bit.  L2 with dim % 16 == 0: the chunk-pair form; else a lane per row (rerank_plan.h).
struct RerankBytesParams : RerankTopkParams {
    const uint8_t* db_b;     // [n x dstride] bytes, rows 16-byte aligned
};
hipError_t launch_rerank_bytes(const RerankBytesParams& p, int metric, hipStream_t s);
hipError_t launch_rerank_topk_bytes(const RerankBytesParams& p, int metric, hipStream_t s);
// The same two over the binary16 rows of a half-base handle (rerank_half.hip): `db` stays nullptr, `dstride` is the HALVES of a row --
// round_up(dim, 8), zero padded, which is also the floats of the staged query.  The distances are the float kernels' on float32(db_h), bit
// for bit.  L2 with dim % 4 == 0: the half chunk-pair form; else a lane per row (rerank_plan.h: rerank_half_plan).
struct RerankHalfParams : RerankTopkParams {
    const uint16_t* db_h;    // [n x dstride] binary16 bit patterns, rows 16-byte aligned
};
hipError_t launch_rerank_half(const RerankHalfParams& p, int metric, hipStream_t s);
hipError_t launch_rerank_topk_half(const RerankHalfParams& p, int metric, hipStream_t s);
// diagnostic (tests): one batch merge of a sorted list [size] with up to 64 survivor keys (~0 = none)
hipError_t launch_debug_merge(int regs, const uint64_t* entries, int size, const uint64_t* surv, int ef, uint64_t* out,
                              int* out_size, hipStream_t s);

// MLP projection (support_func.h:624-658).  W is repacked by the host: [dout x wstride] weights
// (zero padded, wstride multiple of 8) + separate bias[dout].
struct LayerParams {
    const float* x;          // [nq x xstride]
    uint32_t xstride;
    const float* w;          // [dout x wstride]
    uint32_t wstride;
    const float* bias;       // [dout]
    float* out;              // [nq x ostride]
    uint32_t ostride;
    uint32_t nq, din, dout;
    int32_t relu;
    int32_t normalize;       // 1: follow the layer by normalizeVector over its dout outputs (fused when dout <= 64)
    int32_t small_footprint; // 1: hidden layers on the 60-register / 9 KB kernel (batches in flight: its blocks fit beside walk wavefronts)
};
// Which instance of a projection kernel a launch runs: decided by the *_pick functions below from shapes, strides and pointer ALIGNMENT alone
// (no device, nothing dereferenced), and every launcher switches on the descriptor its pick returned.  An argument the family does not have stays
// 0 / false.
enum class ProjFamily : uint8_t {
    None,       // nothing to launch (an empty batch or layer), or no instance serves the shape
    Net,        // mlp_net_kernel<NW, A, BH, B3, GO>              (mlp_net.hip)
    Slab,       // mlp_slab_kernel<NW, A, RELU, NORM>             (mlp_net.hip)
    Layer,      // mlp_layer_kernel<RELU, NORM>                   (mlp.hip)
    LayerVec,   // mlp_layer_vec_kernel<RELU, NORM>
    LayerSw,    // mlp_layer_sw_kernel<RELU>
    Narrow,     // mlp_narrow_kernel<RELU, NORM>
    LayerMfma,  // mlp_layer_mfma_kernel<RELU>
    MfmaNet,    // mlp_mfma_net_kernel<RB>                        (mlp_mfma_net.hip)
    Normalize,  // normalize_kernel                               (mlp.hip)
};
struct ProjInstance {
    ProjFamily family;
    int nw, a, bh, b3, go;   // wavefronts, queries per lane, neurons per lane group (hidden / last layer), neuron groups per row of 16 lanes
    bool relu, norm;
    int rb;                  // row blocks of 16 queries per workgroup
};
// the instance as the source spells it: "mlp_net_kernel<8, 5, 8, 2, 2>", "mlp_layer_vec_kernel<true, false>", "normalize_kernel"
void proj_instance_name(const ProjInstance& i, char* out, size_t cap);
// the launches of one projection, in launch order (at most three layers and a normalize_kernel of its own)
struct ProjPlan {
    int count;
    ProjInstance inst[4];
    void add(const ProjInstance& i) { if (i.family != ProjFamily::None && count < 4) inst[count++] = i; }
};
// a layer's kernel and whether a normalize_kernel launch follows it (normalizeVector not fused)
struct LayerPick { ProjInstance inst; bool normalize_after; };
LayerPick mlp_layer_pick(const LayerParams& p);
LayerPick mlp_layer_mfma_pick(const LayerParams& p);
// (every launcher adds what it launched to `ran` when given one)
hipError_t launch_mlp_layer(const LayerParams& p, hipStream_t s, ProjPlan* ran = nullptr);
// the throughput option (GBNNS_FLAG_MFMA_PROJECTION): the same layer as a v_mfma_f32_32x32x2_f32 GEMM -- NOT bit-exact
hipError_t launch_mlp_layer_mfma(const LayerParams& p, hipStream_t s, ProjPlan* ran = nullptr);
// The whole three-layer net in one launch (mlp_net.hip): activations stay in LDS, one block per 16 .. 40 queries (8 .. 20 in the
// half-CU form, which a batch in flight takes: its blocks start on half-drained CUs).  Same
// arithmetic as three launch_mlp_layer calls (relu, relu, normalize), bit for bit.
struct NetLaunch {
    const float* x;          // [nq x xstride]
    uint32_t xstride, nq;
    const float* w[3];       // [dout x wstride], rows zero padded
    uint32_t wstride[3];
    const float* bias[3];
    uint32_t din[3], dout[3];
    float* out;              // [nq x ostride]; columns [dout[2], ostride) are written as zero
    uint32_t ostride;
    int32_t cus;             // compute units of the device (0: 256)
    int32_t force_a;         // diagnostic: queries per lane group (2 .. 5; 0 = chosen by the launcher)
    unsigned long long* stamps;  // diagnostic builds (-DGBNNS_NET_STAMPS): [blocks x 8] 100 MHz timestamps of the phase ends
    int32_t form;            // kNetWholeCu: blocks of 8 wavefronts, one per CU; kNetHalfCu: of 4 wavefronts and half the LDS, two per CU
    uint32_t lds_floor;      // diagnostic: request at least this much LDS per block (> 80 KB: half-CU blocks one per CU)
    const float* img[3];     // the layers' weights as the staged-order image of `form` (pack_net_image below), 16-byte aligned
};
constexpr int32_t kNetWholeCu = 0, kNetHalfCu = 1;
// The staged-order weight image of a layer of the one-launch kernel: what a wavefront's staging buffer holds for each of its chunks,
// byte for byte, so that a chunk goes from memory to LDS by DMA (mlp_net.hip).  A layer is cut into slices of go x b neurons (go
// neuron groups per row of 16 lanes: 2 in the whole-CU form, 4 in the half-CU form; b neurons per lane group: 8 in the hidden
// layers, net_image_b3 in the last) and chunks of ck inputs; the image is [slice][chunk][rows x ldw floats]: staged row r holds
// neuron obase + (interleaved ? (r % go) * b + r / go : r) of the slice, clamped to the layer's last neuron, the chunk's ck inputs
// permuted in blocks of 16 (input 16 m + 4 q + t at float 16 m + 4 t + 2 (q / 2) + q % 2), zero from the row's padded end
// ((din + 15) & ~15) on, and ldw - ck padding floats (zero).
struct NetImageGeom {
    uint32_t ck, ldw, rows, buf;   // inputs per chunk, floats per staged row, rows (go x b) and floats (rows x ldw) per chunk
    uint32_t nch, slices;          // chunks per slice, slices of the layer
    bool interleaved;
};
constexpr NetImageGeom net_image_geom(uint32_t din, uint32_t dout, uint32_t b, uint32_t go) {
    const uint32_t ck = b >= 4 ? 32u : 64u;
    return NetImageGeom{ck, ck + 4u, go * b, go * b * (ck + 4u), (din + ck - 1u) / ck, (dout + go * b - 1u) / (go * b), go == 4 && b >= 4};
}
constexpr uint32_t net_image_b3(uint32_t d_low) { return (d_low + 15u) / 16u <= 2u ? 2u : 4u; }  // the last layer's neurons per lane group
constexpr uint32_t net_image_go(int32_t form) { return form == kNetHalfCu ? 4u : 2u; }
constexpr size_t net_image_floats(uint32_t din, uint32_t dout, uint32_t b, uint32_t go) {
    const NetImageGeom g = net_image_geom(din, dout, b, go);
    return (size_t)g.slices * g.nch * g.buf;
}
// host only, no device needed (handle.cpp): w [dout x wstride] rows -> out [net_image_floats]
void pack_net_image(const float* w, uint32_t wstride, uint32_t din, uint32_t dout, uint32_t b, uint32_t go, float* out);
bool mlp_net_serves(const NetLaunch& n);   // shape, alignment and batch size fit the one-launch kernel
bool mlp_net_half_serves(const NetLaunch& n);   // ... and the half-CU form's block (16 queries and more) fits 80 KB of LDS
size_t mlp_net_lds_bytes(const NetLaunch& n, int form, int A);   // LDS of a block of `form` with A queries per lane (2 .. 5)
// the instance of n.form a batch takes (A: the strip that needs the fewest rounds of the machine x A among those whose LDS fits; B3 by d_low)
// and the LDS layout of its block; false: the kernel, or the form, does not serve the call
struct NetPick { ProjInstance inst; size_t lds; uint32_t bufa, bufb; };
bool mlp_net_pick(const NetLaunch& n, NetPick* pick);
hipError_t launch_mlp_net(const NetLaunch& n, hipStream_t s, ProjPlan* ran = nullptr);
// The throughput option as ONE launch (mlp_mfma_net.hip): v_mfma_f32_16x16x4_f32, one workgroup per CU over its share of the batch, weights
// repacked once per handle into the instruction's B-operand order, activations in LDS.  NOT bit-exact.
bool mlp_mfma_net_serves(uint32_t d, uint32_t d_hidden, uint32_t d_low);
size_t mlp_mfma_net_packed_floats(uint32_t d, uint32_t d_hidden, uint32_t d_low);
hipError_t launch_mlp_mfma_pack(const NetLaunch& n, float* packed, hipStream_t s);
// RB = row blocks of 16 queries per workgroup, `rows` = its queries: ceil(nq / CUs), at most what the LDS holds; false: the net does not fit
struct MfmaNetPick { ProjInstance inst; uint32_t rows; };
bool mlp_mfma_net_pick(const NetLaunch& n, MfmaNetPick* pick);
hipError_t launch_mlp_mfma_net(const NetLaunch& n, const float* packed, hipStream_t s, ProjPlan* ran = nullptr);
// y [nq x stride]: y /= sqrt(L2(y, 0)) over dim (4-lane order, d%4 tail ignored in the norm),
// pad columns [dim, stride) are written as zero.
hipError_t launch_normalize(float* y, uint32_t stride, uint32_t dim, uint32_t nq, hipStream_t s, ProjPlan* ran = nullptr);
// One wide layer of a small batch with the one-launch kernel's inner loop (mlp_net.hip, mlp_slab_kernel): 8 A queries x 128 neurons
// per workgroup, inputs a slab of 256 at a time.
bool mlp_slab_serves(const LayerParams& p);
bool mlp_slab_wins(const LayerParams& p, int cus);  // ... and the layer is one round of the machine in its workgroup shape
// the workgroup shape (NW, A), the ReLU / normalise variant and the grid of a layer; false: mlp_slab_serves says no
struct SlabPick { ProjInstance inst; bool normalize_after; uint64_t blocks; unsigned gx, gy; };
bool mlp_slab_pick(const LayerParams& p, int cus, int force_a, SlabPick* pick);
hipError_t launch_mlp_slab(const LayerParams& p, int cus, hipStream_t s, int force_a = 0, ProjPlan* ran = nullptr);

// Exact brute-force kNN scan (knn.hip): getTruth (support_func.h:270-290) generalised to k results per query.
struct KnnParams {
    const float* base;       // [n x bstride]
    uint32_t bstride;        // floats
    uint64_t n;
    const float* q;          // [nq x qstride]
    uint32_t qstride;
    uint32_t nq;
    uint32_t dim;            // <= 128
    int32_t k;
    int64_t self_offset;     // >= 0: query i is base row i + self_offset and is not its own neighbour; -1: off
    uint64_t* heap;          // workspace [k x heap_stride], pre-filled with all-ones
    size_t heap_stride;      // >= nq
    uint32_t* out_ids;       // [nq x k] ascending (distance, id); 0xFFFFFFFF where fewer than k rows exist
    float* out_dist;         // optional [nq x k]
    uint64_t row0;           // id of `base` row 0 (scans of a slice of the base set; 0 = the whole set)
    int32_t keep_heap;       // 1: leave the heaps as they are (no sort, no outputs): more rows follow
    // gbnns_exact_knn_tagged (last, so that no other field moves): row j is offered to query i only when (row_tags[j] & query_tags[i]) != 0 --
    // the tagged instances of the scan kernels; the rescore / pool kernels see allowed candidates only and do not look
    const uint32_t* row_tags;   // [row0 + n] tag words by row ID (not by row of `base`), or nullptr: the untagged instances
    const uint32_t* query_tags; // [nq]
};
hipError_t launch_knn_scan(const KnnParams& p, int metric, hipStream_t s);
// Host only, no device needed: the name, template arguments included, of the instance launch_knn_scan / launch_knn_filter /
// launch_knn_bytes_sweep start for that shape -- taken from the table the launch itself reads (nullptr: no instance).  `tagged`: a launch
// with row tags; dp: the packed row length (KnnFilterParams::dp, KnnBytesSweepParams::dp).
const char* knn_scan_kernel_name(int metric, uint32_t dim, bool tagged);
const char* knn_filter_kernel_name(uint32_t dp, bool tagged);
const char* knn_bytes_sweep_kernel_name(uint32_t dp, bool tagged);

// Matrix-core filter in front of the exact scan (knn.hip, round 4; L2 metric, d % 4 == 0, d <= 128).
// Rows packed for v_mfma_f32_32x32x16_bf16: per row, per group of 8 dims, 8 bf16 "hi" parts then 8 bf16 "lo" parts
// (x = hi + lo + r, |r| <= 2^-16 |x|), dims zero-padded to a multiple of 16; and the row's squared norm.
hipError_t launch_knn_pack(const float* x, uint32_t stride, uint32_t dim, uint64_t rows, uint16_t* packed, float* norms, hipStream_t s);
struct KnnFilterParams {
    const uint16_t* qpack;   // [nq x 2 dp] packed queries
    const uint16_t* bpack;   // [rows x 2 dp] packed base rows of this chunk
    const float* bnorm;      // [rows] squared norms of the chunk's rows
    const float* rhs;        // [nq] 0.5 ((1 - c) |q|^2 - T_q): a row passes when  q.x - 0.5 (1 - c) |x|^2 >= rhs  (-inf: everything passes)
    uint32_t nq, dp;         // dp = padded dimension (multiple of 16)
    uint32_t rows;           // rows of the chunk
    uint32_t row0;           // id of the chunk's first row
    uint32_t cap;            // candidate slots per query
    uint32_t* cand;          // [nq x cap] ids that passed
    uint32_t* count;         // [nq] how many passed (may exceed cap: then *overflow is set and the chunk is scanned exactly)
    uint32_t* overflow;      // [1]
    // gbnns_exact_knn_tagged (last): a pair whose row is not allowed for its query is not a hit -- neither counted nor stored
    const uint32_t* btag;    // [rows] tag words of the chunk's rows, 16-byte aligned and readable (any value) up to the end of the chunk's last block of 32, or nullptr: the untagged instances
    const uint32_t* qtag;    // [nq]
};
hipError_t launch_knn_filter(const KnnFilterParams& p, hipStream_t s);
// thresholds from the heaps: rhs[q] = 0.5 ((1 - c) |q|^2 - d_k(q)), -inf while the heap is not full
hipError_t launch_knn_thresholds(const uint64_t* heap, size_t heap_stride, int k, const float* qnorm, uint32_t nq, float* rhs, hipStream_t s);
// exact distances (the reference's arithmetic) of the candidates, offered to the heaps; then the new thresholds
struct KnnRescoreParams {
    KnnParams k;             // base = the WHOLE base set, heap, q, ...
    const uint32_t* cand;
    const uint32_t* count;
    uint32_t cap;
    const float* qnorm;
    float* rhs;
};
hipError_t launch_knn_rescore(const KnnRescoreParams& p, hipStream_t s);
hipError_t launch_knn_finalize(const KnnParams& p, hipStream_t s);   // heap sort + outputs
// long lists (64 <= k <= 4 096): the k smallest keys of a query as an unordered pool, one wavefront per query and chunk (knn.hip)
struct KnnPoolParams {
    KnnParams k;             // base = the WHOLE base set, q, dims, self_offset, outputs (heap unused)
    uint64_t* pool;          // [nq x k] keys, all-ones = no entry
    uint64_t* root;          // [nq] largest key of the pool (all-ones while it is not full)
    const uint32_t* cand;    // [nq x cap] rows the filter kept
    const uint32_t* count;   // [nq]
    uint32_t cap;
    const float* qnorm;
    float* rhs;              // [nq] the filter's thresholds, rewritten from `root`
};
hipError_t launch_knn_pool_update(const KnnPoolParams& p, hipStream_t s);
hipError_t launch_knn_pool_finalize(const KnnPoolParams& p, hipStream_t s);   // ascending order + outputs
constexpr float kKnnFilterSlack = 1.0f / 4096.0f;  // c: |approximate - reference distance| <= c (|q|^2 + |x|^2) with room to spare (knn.hip)

// Exact kNN over uint8 rows on the int8 matrix cores (knn_bytes.hip; d <= 256: every distance is an integer below 2^24, so
// the int32 result of v_mfma_i32_32x32x32_i8 IS the reference's float distance).  Rows are packed as signed bytes x - 128,
// dp = d rounded up to the K step of 32 with signed zeros, row-major: the operand fragment of lane (row, half) at K step s
// is the 16 bytes at 32 s + 16 half.  Per row one int32 term that folds its norm (L2) or its sum (negative dot):
//   base row x:  bterm = -|x'|^2          (L2)    128 sum(x')                   (NEG_DOT)
//   query q:     qterm =  |q'|^2          (L2)   -128 sum(q') - 16384 d         (NEG_DOT)
// and with s = (x'.q' << shift) + bterm (shift 1 for L2, 0 for NEG_DOT) the exact distance is  qterm - s.
constexpr uint32_t kKnnBytesKStep = 32;    // K of one v_mfma_i32_32x32x32_i8
constexpr uint32_t kKnnBytesRowBlock = 32; // base rows of one product
// (`stride` = bytes between rows of x, >= dim: d for a caller's array, d_pad for a byte handle's resident table)
hipError_t launch_knn_bytes_pack(const uint8_t* x, uint32_t stride, uint32_t dim, uint32_t dp, int metric, int query_side, uint64_t rows, int8_t* packed,
                                 int32_t* term, hipStream_t s);
struct KnnBytesSweepParams {
    const int8_t* qpack;     // [nq x dp]
    const int8_t* bpack;     // [rows x dp] packed base rows of this chunk (the chunk starts on a multiple of 4 rows)
    const int32_t* bterm;    // [rows rounded up to 32] the chunk's row terms (readable, any value, beyond the set)
    const int32_t* qterm;    // [nq]
    const int32_t* thr;      // [nq] qterm - T_q: a row is kept when s >= thr, i.e. distance <= T_q (INT32_MIN: everything passes)
    uint32_t nq, dp;
    uint32_t rows;           // rows of the chunk
    uint32_t row0;           // id of the chunk's first row
    uint32_t cap;            // key slots per query
    int32_t shift;           // 1 = L2, 0 = NEG_DOT
    uint64_t* cand;          // [nq x cap] keys (knn_fkey(float(distance)) << 32 | id) of the rows kept
    uint32_t* count;         // [nq] how many were kept (may exceed cap: then *overflow is set and the chunk is swept again in pieces)
    uint32_t* overflow;      // [1]
    // gbnns_exact_knn_bytes_tagged (last): as KnnFilterParams::btag / qtag
    const uint32_t* btag;    // [rows] tag words of the chunk's rows (16-byte aligned, readable to the end of the last block of 32), or nullptr
    const uint32_t* qtag;    // [nq]
};
hipError_t launch_knn_bytes_sweep(const KnnBytesSweepParams& p, hipStream_t s);
// the kept keys offered to a query's heap (pool == nullptr; [k x heap_stride]) or pool ([nq x k] + root [nq]); then the new thresholds
struct KnnBytesOfferParams {
    uint64_t* heap;
    size_t heap_stride;
    uint64_t* pool;
    uint64_t* root;
    const uint64_t* cand;
    const uint32_t* count;
    uint32_t cap;
    uint32_t nq;
    int32_t k;
    int64_t self_offset;     // >= 0: query i is base row i + self_offset and is not its own neighbour; -1: off
    const int32_t* qterm;
    int32_t* thr;
};
hipError_t launch_knn_bytes_offer(const KnnBytesOfferParams& p, hipStream_t s);

// Gathered exact scan (knn_gather.hip; gbnns_index_exact_knn_gather): the queries of a batch that share a tag word scan the list of the
// rows that word allows instead of the table.  gather_schedule (host, pure) groups and deals the work; the fill kernel materialises the
// lists of a round; knn_gather_kernel is knn_scan_kernel's loop with the tile's rows read through a list and a thread's queries through
// the schedule's permutation.  d <= 128, heaps [k x heap_stride] as the scan's, finished by launch_knn_finalize.
struct GatherGroup {         // the queries of one distinct word with allowed > 0
    uint32_t word;
    uint32_t len;            // rows the word allows (the census count): the length of its list
    uint32_t q_begin, q_count;  // its queries: order[q_begin .. q_begin + q_count), ascending index
    uint32_t round;
    uint64_t list_off;       // first entry of its list in the round's list buffer
};
struct GatherWorkgroup {     // one workgroup of knn_gather_kernel: up to W queries of one group
    uint32_t list_off_lo, list_off_hi;  // (two words: the struct is read by the device as uint32 x 6)
    uint32_t list_len;
    uint32_t q_begin, q_count;  // order[q_begin .. q_begin + q_count), q_count <= W
    uint32_t pad;
};
struct GatherSchedule {
    std::vector<uint32_t> order;           // [nq] a permutation: groups in ascending word order, queries of a group in ascending index, then the queries that may see nothing
    std::vector<GatherGroup> groups;       // ascending word, hence ascending round
    std::vector<GatherWorkgroup> wgs;      // round by round, group by group
    std::vector<uint32_t> round_group0;    // [n_rounds + 1] first group of every round
    std::vector<uint32_t> round_wg0;       // [n_rounds + 1] first workgroup of every round
    std::vector<uint64_t> round_entries;   // [n_rounds] list entries of the round
};
// words / allowed [nq]: every query's tag word and census count (<= n); budget: list entries a round may hold (a group longer than that gets a
// round of its own); W: queries a workgroup serves.  Throws std::bad_alloc only.
void gather_schedule(const uint32_t* words, const uint32_t* allowed, uint64_t nq, uint64_t n, uint64_t budget, uint32_t W, GatherSchedule& out);
struct GatherFillParams {
    const uint32_t* tags;    // [n] the handle's tag table, 16-byte aligned
    uint64_t n;
    const uint32_t* words;   // [groups] the round's words
    const uint32_t* caps;    // [groups] their census counts: entries of a word's list; a store beyond is dropped
    const uint64_t* offs;    // [groups] first entry of each word's list in `list`
    uint32_t groups;
    uint32_t* cursor;        // [groups] zero at launch
    uint32_t* list;          // the round's list buffer
};
hipError_t launch_gather_fill(const GatherFillParams& p, hipStream_t s);
struct KnnGatherParams {
    const float* base;       // [n x bstride] float rows, or nullptr:
    const uint8_t* base_b;   // [n x bstride] byte rows (16-byte aligned, zero padded to bstride), widened while staged
    uint32_t bstride;        // elements between rows
    const float* q;          // [nq x qstride], or nullptr:
    const uint8_t* q_b;      // [nq x qstride] byte queries, widened into registers
    uint32_t qstride;
    uint32_t dim;            // <= 128
    int32_t k;
    int64_t self_offset;     // >= 0: query i is row i + self_offset (original ids) and is not its own neighbour; -1: off
    uint64_t* heap;          // [k x heap_stride], by ORIGINAL query index
    size_t heap_stride;
    const uint32_t* order;   // [nq] the schedule's permutation
    const GatherWorkgroup* wgs;  // the round's workgroups
    uint32_t n_wgs;
    const uint32_t* list;    // the round's list buffer, filled
};
hipError_t launch_knn_gather(const KnnGatherParams& p, int metric, hipStream_t s);
// Host only, no device needed: the instance launch_knn_gather starts for a shape and the queries W one of its workgroups serves (nullptr / 0: d > 128)
const char* knn_gather_kernel_name(int metric, uint32_t dim, bool bytes, uint32_t* W);

// GD pruning of a kNN graph, one node per wavefront (support_func.h:521-563).  deg[i] = 0xFFFFFFFF marks a node
// left to the host (equal distances in its list, list longer than 1024, id out of range).
struct GdParams {
    const float* ds;         // [n x dstride], rows zero-padded to a multiple of 4 floats
    uint32_t dstride, dim;
    uint32_t n;
    int32_t M;               // 2 .. 64
    const uint64_t* knn_off; // [n + 1]
    const uint32_t* knn_nbr;
    uint32_t* adj;           // [n x 2M]
    uint32_t* deg;           // [n]
};
hipError_t launch_gd_prune(const GdParams& p, int metric, hipStream_t s);

// Locality order of a batch (counting sort on the sign bits of the first `bits` = 10 .. 16 walked-space coordinates;
// dim >= bits): hist [2^bits] u32 scratch, order [nq] u32 out.
hipError_t launch_query_order(const float* q, uint32_t qstride, uint32_t dim, uint32_t nq, uint32_t bits, uint32_t* hist, uint32_t* order,
                              hipStream_t s);

// helpers
hipError_t launch_fill_u32(uint32_t* p, uint32_t v, size_t count, hipStream_t s);

}  // namespace gbnns
